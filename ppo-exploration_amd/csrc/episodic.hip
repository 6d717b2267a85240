// Episodic novelty bonus of PPO(episodic=True): the per-episode half of NGU, on the exact
// integer embeddings of ppox_simhash_sums_u8.  include/ppox.h holds the semantics, tests/episodic_twin.py their
// numpy restatement.  Two kernels per collect step, nothing read back to the host:
//
//   episodic_knn_kernel     one wave per env, four envs per 256-thread block (es_novelty.hip's layout).  Lane j
//                           takes the ring rows j, j + 64, ... (a row is 64 contiguous bytes, read as four 16-byte
//                           loads, so the wave reads 4 KB runs), computes the squared distance in int64 and keeps
//                           its KMAX smallest as an ascending list in registers (an unrolled compare-exchange
//                           chain, INT64_MAX where it has seen fewer rows).  The k = min(K, live rows) smallest of
//                           the wave leave by k rounds of a wave-wide minimum; the lowest lane holding it pops it,
//                           so equal distances leave one at a time.  Then lanes 0..15 append the embedding to the
//                           ring and lane 0 advances / resets the count.  No LDS, no scratch, no atomics.
//   episodic_reward_kernel  one workgroup, all f64, contraction off (Makefile): the adjacent-pair tree sum of the
//                           envs' mean distances, the running mean dm, and the reward formula per env.
//   ngu_reward_kernel       PPO_NGU's (tests/ngu_twin.py) in place of the one above, from the same
//                           __device__ pieces: that bonus times a modulator from the RND error's running moments.
//   elliptical_kernel       kind="elliptical" (tests/elliptical_twin.py) in place of the first two:
//                           b = phi' C^-1 phi and the rank-one update of C^-1, 16 lanes per env; and
//   ngu_modulate_kernel     ngu_reward_kernel's modulator half on that bonus.
// The distances are integers, so any order of evaluation gives the same bits; the f64 sums are in a fixed order.
#include <cmath>

#include "common.h"

namespace {

using i32x4 = __attribute__((ext_vector_type(4))) int;

constexpr int KMAX = 16, EMB = 16;
constexpr long long I64_MAX = 0x7FFFFFFFFFFFFFFFll;

__device__ inline long long wave_min_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long u = __shfl_xor(v, o, 64);
        v = u < v ? u : v;
    }
    return v;
}

__global__ void __launch_bounds__(256)
    episodic_knn_kernel(const int32_t* __restrict__ emb, const uint8_t* __restrict__ done, long long N, long long L,
                        int K, int32_t* __restrict__ mem, int32_t* __restrict__ count, double* __restrict__ dk,
                        int32_t* __restrict__ kfound, double* __restrict__ mk) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long n = (long long)blockIdx.x * 4 + wv;
    if (n >= N) return;  // wave-uniform
    const i32x4* qv = reinterpret_cast<const i32x4*>(emb + n * EMB);
    const i32x4 q[4] = {qv[0], qv[1], qv[2], qv[3]};
    int32_t c = count[n];
    if (c < 0) c = 0;  // (never written by this kernel: a caller's count starts at 0)
    const long long m = c < L ? c : L;
    int32_t* ring = mem + n * L * EMB;
    long long a[KMAX];  // ascending
#pragma unroll
    for (int i = 0; i < KMAX; ++i) a[i] = I64_MAX;
    for (long long j = lane; j < m; j += 64) {
        const i32x4* row = reinterpret_cast<const i32x4*>(ring + j * EMB);
        long long d = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const i32x4 x = row[v];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long long diff = (long long)q[v][e] - (long long)x[e];
                d += diff * diff;
            }
        }
        if (d < a[KMAX - 1]) {  // else the chain would leave the list as it is
#pragma unroll
            for (int i = 0; i < KMAX; ++i) {
                const bool lt = d < a[i];
                const long long lo = lt ? d : a[i];
                d = lt ? a[i] : d;
                a[i] = lo;
            }
        }
    }
    const int k = (int)(K < m ? K : m);
    double mine = 0.0, sum = 0.0;  // lane r keeps the r-th smallest
    for (int r = 0; r < k; ++r) {
        const long long mn = wave_min_i64(a[0]);
        const unsigned long long holders = __ballot(a[0] == mn);
        const int winner = __ffsll(holders) - 1;  // holders != 0: the minimum is some lane's head
        if (lane == winner) {
#pragma unroll
            for (int i = 0; i + 1 < KMAX; ++i) a[i] = a[i + 1];
            a[KMAX - 1] = I64_MAX;
        }
        const double f = (double)mn;  // round to nearest
        if (lane == r) mine = f;
        sum = sum + f;
    }
    if (lane < K) dk[n * K + lane] = mine;  // zero past k
    // every lane's ring reads are complete: their values fed the minimum rounds above
    const long long slot = c % L;
    if (lane < EMB) ring[slot * EMB + lane] = emb[n * EMB + lane];
    if (lane == 0) {
        kfound[n] = k;
        mk[n] = k > 0 ? sum / (double)k : 0.0;
        count[n] = done[n] != 0 ? 0 : c + 1;
    }
}

// s[i] = s[2i] + s[2i + 1] over `len` (a power of two) consecutive values x(i0 + i): a binary counter of partial sums
// held in registers (every index a constant after unrolling)
template <typename F>
__device__ inline double pair_tree(long long i0, long long len, F x) {
    constexpr int LEVELS = 24;  // len <= 2^31 / RT
    double st[LEVELS];
#pragma unroll
    for (int b = 0; b < LEVELS; ++b) st[b] = 0.0;
    for (long long i = 0; i < len; ++i) {
        double v = x(i0 + i);
        bool carry = true;
#pragma unroll
        for (int b = 0; b < LEVELS; ++b) {
            if (carry) {
                if ((i >> b) & 1) {
                    v = st[b] + v;
                } else {
                    st[b] = v;
                    carry = false;
                }
            }
        }
    }
    // len = 2^j: the last element (all j low bits set) carried through levels 0 .. j-1 and was stored at level j
    double r = 0.0;
#pragma unroll
    for (int b = 0; b < LEVELS; ++b)
        if ((len >> b) == 1) r = st[b];
    return r;
}

// one workgroup of RT threads (RW waves): the tree sum needs every env before any reward, and at 4,096 envs the f64
// divides of 4 envs per thread are short next to a second launch
constexpr int RT = 1024, RW = RT / 64;

// the values per thread of the padded length: a power of two, at least one value per thread
__device__ inline long long tree_per_thread(long long N) {
    long long P = RT;
    while (P < N) P <<= 1;
    return P / RT;
}

// the tree over x(0 .. N) up to the wave: this thread's `per` consecutive values, then lane pairs, pairs of pairs
// ... (the tree's next six levels); every lane returns its wave's sum
template <typename F>
__device__ inline double wave_tree(long long per, F x) {
    double v = pair_tree(threadIdx.x * per, per, x);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

// the tree's last levels, over the waves' sums (one thread; wsum is overwritten)
__device__ inline double waves_tree(double* wsum) {
    for (int s = 1; s < RW; s <<= 1)
        for (int w = 0; w < RW; w += 2 * s) wsum[w] = wsum[w] + wsum[w + s];
    return wsum[0];
}

// #{kfound > 0} among this wave's envs (every lane returns it)
__device__ inline long long wave_valid_count(const int32_t* __restrict__ kfound, long long N, long long per) {
    const long long tid = threadIdx.x;
    long long cnt = 0;
    for (long long i = tid * per; i < (tid + 1) * per && i < N; ++i) cnt += kfound[i] > 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) cnt += __shfl_xor(cnt, o, 64);
    return cnt;
}

// the running mean of the squared kNN distance advanced by this step's tree sum S over nv valid envs (one thread)
__device__ inline double dm_update(double* __restrict__ dm, double S, long long nv, double decay) {
    double d0 = dm[0];
    if (nv > 0) {
        const double mu = S / (double)nv;
        d0 = dm[1] == 0.0 ? mu : decay * d0 + (1.0 - decay) * mu;
        dm[0] = d0;
        dm[1] = dm[1] + 1.0;
    }
    return d0;
}

// env n's bonus from its k nearest and the updated dm[0]
__device__ inline double episodic_r(const double* __restrict__ dk, const int32_t* __restrict__ kfound, long long n,
                                    int K, double d0, double eps, double xi, double c, double smax) {
    const int k = kfound[n] < K ? kfound[n] : K;  // (the knn kernel writes at most K)
    if (k <= 0) return 0.0;
    double acc = 0.0;
    for (int i = 0; i < k; ++i) {
        double q = d0 > 0.0 ? dk[n * K + i] / d0 : 0.0;
        q = q - xi;
        q = q > 0.0 ? q : 0.0;
        acc = acc + eps / (q + eps);
    }
    const double s = sqrt(acc) + c;
    return s > smax ? 0.0 : 1.0 / s;
}

__global__ void __launch_bounds__(RT)
    episodic_reward_kernel(const double* __restrict__ dk, const int32_t* __restrict__ kfound,
                           const double* __restrict__ mk, long long N, int K, double* __restrict__ dm, double decay,
                           double beta, double eps, double xi, double c, double smax, float* __restrict__ rewards,
                           float* __restrict__ bonus) {
    __shared__ double wsum[RW];
    __shared__ long long wcnt[RW];
    __shared__ double dm0;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long per = tree_per_thread(N);
    const long long cnt = wave_valid_count(kfound, N, per);
    const double v = wave_tree(per, [&](long long i) { return i < N && kfound[i] > 0 ? mk[i] : 0.0; });
    if (lane == 0) {
        wsum[wv] = v;
        wcnt[wv] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        long long nv = 0;
        for (int w = 0; w < RW; ++w) nv += wcnt[w];
        dm0 = dm_update(dm, waves_tree(wsum), nv, decay);
    }
    __syncthreads();
    const double d0 = dm0;
    for (long long n = tid; n < N; n += RT) {
        const double r = episodic_r(dk, kfound, n, K, d0, eps, xi, c, smax);
        bonus[n] = (float)r;
        rewards[n] = rewards[n] + (float)(beta * r);
    }
}

// Chan's merge of the batch moments (mb, vb, n) into em = (mean, variance, count), left to right as written
// (util.py:30-44); out = the updated mean and sigma (one thread)
__device__ inline void chan_merge(double* __restrict__ em, double mb, double vb, double n, double* out) {
    const double m0 = em[0], v0 = em[1], c0 = em[2];
    const double delta = mb - m0;
    const double tot = c0 + n;
    const double m1 = m0 + delta * n / tot;
    const double M2 = v0 * c0 + vb * n + delta * delta * c0 * n / tot;
    const double v1 = M2 / tot;
    em[0] = m1;
    em[1] = v1;
    em[2] = tot;
    out[0] = m1;
    out[1] = sqrt(v1);
}

// the modulator of the error e against the updated moments, in [1, mod_max]
__device__ inline double ngu_mod(double e, double mean, double sigma, double mod_max) {
    const double a = sigma > 0.0 ? 1.0 + (e - mean) / sigma : 1.0;
    const double mod = a > 1.0 ? a : 1.0;
    return mod < mod_max ? mod : mod_max;
}

// NGU's reward: the episodic r of the kernel above times a modulator from the lifelong (RND) error's
// running moments.  Three tree sums, the third depending on the second's mean, so three rounds through the LDS:
//   1  S (the kNN means) and sum(e) side by side            -> thread 0: dm, mb
//   2  sum((e - mb)^2)                                      -> thread 0: the Chan merge into em
//   3  per env r, the modulator and their product
// err == nullptr (RND's warm-up): round 1 without e, no round 2, modulator 1, em neither read nor written.
__global__ void __launch_bounds__(RT)
    ngu_reward_kernel(const double* __restrict__ dk, const int32_t* __restrict__ kfound,
                      const double* __restrict__ mk, const float* __restrict__ err, long long N, int K,
                      double* __restrict__ dm, double* __restrict__ em, double decay, double eps, double xi, double c,
                      double smax, double mod_max, float* __restrict__ int_rewards, float* __restrict__ bonus,
                      float* __restrict__ modulator) {
    __shared__ double wsum[RW], wsum_e[RW];
    __shared__ long long wcnt[RW];
    __shared__ double bc[3];  // dm[0]; mb, then em[0]; sigma
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const bool has_err = err != nullptr;  // uniform over the workgroup
    const long long per = tree_per_thread(N);
    const long long cnt = wave_valid_count(kfound, N, per);
    const double v = wave_tree(per, [&](long long i) { return i < N && kfound[i] > 0 ? mk[i] : 0.0; });
    double ve = 0.0;
    if (has_err) ve = wave_tree(per, [&](long long i) { return i < N ? (double)err[i] : 0.0; });
    if (lane == 0) {
        wsum[wv] = v;
        wsum_e[wv] = ve;
        wcnt[wv] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        long long nv = 0;
        for (int w = 0; w < RW; ++w) nv += wcnt[w];
        bc[0] = dm_update(dm, waves_tree(wsum), nv, decay);
        if (has_err) bc[1] = waves_tree(wsum_e) / (double)N;
    }
    __syncthreads();
    const double d0 = bc[0];
    double mean = 0.0, sigma = 0.0;
    if (has_err) {
        const double mb = bc[1];
        const double vv = wave_tree(per, [&](long long i) {
            if (i >= N) return 0.0;
            const double d = (double)err[i] - mb;
            return d * d;
        });
        if (lane == 0) wsum_e[wv] = vv;  // (thread 0's reads of wsum_e lie before the barrier above)
        __syncthreads();                 // ... and every thread has read mb: bc[1] is free
        if (tid == 0) chan_merge(em, mb, waves_tree(wsum_e) / (double)N, (double)N, bc + 1);
        __syncthreads();
        mean = bc[1];
        sigma = bc[2];
    }
    for (long long n = tid; n < N; n += RT) {
        const double r = episodic_r(dk, kfound, n, K, d0, eps, xi, c, smax);
        const double mod = has_err ? ngu_mod((double)err[n], mean, sigma, mod_max) : 1.0;
        bonus[n] = (float)r;
        modulator[n] = (float)mod;
        int_rewards[n] = (float)(r * mod);
    }
}

// The modulator half of the kernel above for a bonus that is already there (eb, ppox_elliptical_bonus's; DESIGN.md
// §4.7): rounds 1 and 2 on the error alone, then per env r = eb[n] in place of episodic_r.
__global__ void __launch_bounds__(RT)
    ngu_modulate_kernel(const double* __restrict__ eb, const float* __restrict__ err, long long N,
                        double* __restrict__ em, double mod_max, float* __restrict__ int_rewards,
                        float* __restrict__ bonus, float* __restrict__ modulator) {
    __shared__ double wsum_e[RW];
    __shared__ double bc[3];  // -; mb, then em[0]; sigma
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const bool has_err = err != nullptr;  // uniform over the workgroup
    double mean = 0.0, sigma = 0.0;
    if (has_err) {
        const long long per = tree_per_thread(N);
        const double ve = wave_tree(per, [&](long long i) { return i < N ? (double)err[i] : 0.0; });
        if (lane == 0) wsum_e[wv] = ve;
        __syncthreads();
        if (tid == 0) bc[1] = waves_tree(wsum_e) / (double)N;
        __syncthreads();
        const double mb = bc[1];
        const double vv = wave_tree(per, [&](long long i) {
            if (i >= N) return 0.0;
            const double d = (double)err[i] - mb;
            return d * d;
        });
        if (lane == 0) wsum_e[wv] = vv;  // (thread 0's reads of wsum_e lie before the barrier above)
        __syncthreads();                 // ... and every thread has read mb: bc[1] is free
        if (tid == 0) chan_merge(em, mb, waves_tree(wsum_e) / (double)N, (double)N, bc + 1);
        __syncthreads();
        mean = bc[1];
        sigma = bc[2];
    }
    for (long long n = tid; n < N; n += RT) {
        const double r = eb[n];
        const double mod = has_err ? ngu_mod((double)err[n], mean, sigma, mod_max) : 1.0;
        bonus[n] = (float)r;
        modulator[n] = (float)mod;
        int_rewards[n] = (float)(r * mod);
    }
}

// Elliptical episodic bonus (tests/elliptical_twin.py): b = phi' M phi with M = (ridge I + sum of
// this episode's phi phi')^-1 kept per env as 16 x 16 f64 and advanced by a rank-one Sherman-Morrison update.
// 16 lanes per env, four envs per wave, 16 envs per 256-thread block.  Lane i of a group holds row i of M in 16
// f64 registers, forms u_i = sum_j M[i][j] phi_j in-lane, fetches the group's 16 u_j by width-16 shuffles, forms
// the same b as its 15 neighbours in the stated order, and updates and stores its own row.  All f64, one rounding
// per operation (contraction off), u_i * u_j commutes so M stays bitwise symmetric.  A group past N computes on
// zeros and neither loads nor stores: no lane leaves before the barriers / shuffles.
// The group's contiguous 2 KB goes through the LDS both ways: coalesced 16-B chunks (lane i takes chunks i, i + 16,
// ...) into rows padded to 17 doubles, so that the 16 lanes' row reads and writes (8 B each, 34 dwords apart) fall
// on distinct banks.  Lane i loading its row straight from global memory (8 x 16 B, lanes 128 B apart) measured
// 0.8 us slower per launch at 4,096 envs and is not kept.
using f64x2 = __attribute__((ext_vector_type(2))) double;
constexpr int ELL_ENVS = 16, ELL_PITCH = EMB + 1;

__global__ void __launch_bounds__(256)
    elliptical_kernel(const int32_t* __restrict__ emb, const uint8_t* __restrict__ done, long long N, double ridge,
                      double beta, double* __restrict__ minv, int32_t* __restrict__ count, double* __restrict__ eb,
                      float* __restrict__ rewards, float* __restrict__ bonus) {
    __shared__ double tile[ELL_ENVS * EMB * ELL_PITCH];
    const int i = threadIdx.x & 15, g = threadIdx.x >> 4;
    const long long n = (long long)blockIdx.x * ELL_ENVS + g;
    const bool live = n < N;  // uniform over the 16-lane group
    double phi[EMB], m[EMB], uj[EMB];
#pragma unroll
    for (int j = 0; j < EMB; ++j) phi[j] = m[j] = 0.0;
    f64x2* __restrict__ mat = reinterpret_cast<f64x2*>(minv + (live ? n : 0) * (EMB * EMB));
    double* __restrict__ mine = tile + g * EMB * ELL_PITCH;
    if (live) {
        const i32x4* qv = reinterpret_cast<const i32x4*>(emb + n * EMB);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const i32x4 q = qv[v];
#pragma unroll
            for (int e = 0; e < 4; ++e) phi[4 * v + e] = (double)q[e];
        }
#pragma unroll
        for (int k = 0; k < EMB / 2; ++k) {
            const int c = k * 16 + i;  // chunk c = elements 2c, 2c + 1 = row c / 8, columns 2 (c % 8), + 1
            const f64x2 x = mat[c];
            mine[(c >> 3) * ELL_PITCH + 2 * (c & 7)] = x[0];
            mine[(c >> 3) * ELL_PITCH + 2 * (c & 7) + 1] = x[1];
        }
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int j = 0; j < EMB; ++j) m[j] = mine[i * ELL_PITCH + j];
    }
    double u = 0.0;
#pragma unroll
    for (int j = 0; j < EMB; ++j) u = u + m[j] * phi[j];
#pragma unroll
    for (int j = 0; j < EMB; ++j) uj[j] = __shfl(u, j, 16);
    double b = 0.0;
#pragma unroll
    for (int j = 0; j < EMB; ++j) b = b + phi[j] * uj[j];
    b = b > 0.0 ? b : 0.0;  // a NaN goes to 0 too
    const double den = 1.0 + b;
#pragma unroll
    for (int j = 0; j < EMB; ++j) m[j] = m[j] - (u * uj[j]) / den;
    bool reset = false;
    if (live) {
        reset = done[n] != 0;
        if (i == 0) {
            const int32_t c = count[n];
            const double pay = c > 0 ? b : 0.0;  // an episode's first state is scored against no other
            eb[n] = pay;
            if (bonus) bonus[n] = (float)pay;
            if (rewards) rewards[n] = rewards[n] + (float)(beta * pay);
            count[n] = reset ? 0 : (c < 0x7FFFFFFF ? c + 1 : c);
        }
    }
    if (reset) {
        const double d = 1.0 / ridge;
#pragma unroll
        for (int j = 0; j < EMB; ++j) m[j] = j == i ? d : 0.0;
    }
    if (live) {
#pragma unroll
        for (int j = 0; j < EMB; ++j) mine[i * ELL_PITCH + j] = m[j];  // the row this lane read: no hazard
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int k = 0; k < EMB / 2; ++k) {
            const int c = k * 16 + i;
            f64x2 x;
            x[0] = mine[(c >> 3) * ELL_PITCH + 2 * (c & 7)];
            x[1] = mine[(c >> 3) * ELL_PITCH + 2 * (c & 7) + 1];
            mat[c] = x;
        }
    }
}

}  // namespace

extern "C" int ppox_episodic_knn(const int32_t* emb, const uint8_t* done, int64_t N, int64_t L, int32_t K,
                                 int32_t* mem, int32_t* count, double* dk, int32_t* kfound, double* mk,
                                 void* stream) {
    PPOX_REQUIRE(emb && done && mem && count && dk && kfound && mk, "ppox_episodic_knn: null pointer");
    PPOX_REQUIRE(N >= 1 && N <= 0x7FFFFFFFll, "ppox_episodic_knn: N must lie in [1, 2^31), not %lld", (long long)N);
    PPOX_REQUIRE(L >= 1 && L <= 0x7FFFFFFFll, "ppox_episodic_knn: L must lie in [1, 2^31), not %lld", (long long)L);
    PPOX_REQUIRE(K >= 1 && K <= KMAX, "ppox_episodic_knn: K must lie in [1, 16], not %d", (int)K);
    episodic_knn_kernel<<<ppox::ceil_div(N, 4), 256, 0, ppox::as_stream(stream)>>>(emb, done, N, L, K, mem, count, dk,
                                                                                   kfound, mk);
    PPOX_LAUNCHED("ppox_episodic_knn");
}

extern "C" int ppox_episodic_reward(const double* dk, const int32_t* kfound, const double* mk, int64_t N, int32_t K,
                                    double* dm, double decay, double beta, double eps, double xi, double c,
                                    double smax, float* rewards, float* bonus, void* stream) {
    PPOX_REQUIRE(dk && kfound && mk && dm && rewards && bonus, "ppox_episodic_reward: null pointer");
    PPOX_REQUIRE(N >= 1 && N <= 0x7FFFFFFFll, "ppox_episodic_reward: N must lie in [1, 2^31), not %lld", (long long)N);
    PPOX_REQUIRE(K >= 1 && K <= KMAX, "ppox_episodic_reward: K must lie in [1, 16], not %d", (int)K);
    episodic_reward_kernel<<<1, RT, 0, ppox::as_stream(stream)>>>(dk, kfound, mk, N, K, dm, decay, beta, eps, xi, c,
                                                                   smax, rewards, bonus);
    PPOX_LAUNCHED("ppox_episodic_reward");
}

extern "C" int ppox_ngu_reward(const double* dk, const int32_t* kfound, const double* mk, const float* err, int64_t N,
                               int32_t K, double* dm, double* em, double decay, double eps, double xi, double c,
                               double smax, double mod_max, float* int_rewards, float* bonus, float* modulator,
                               void* stream) {
    PPOX_REQUIRE(dk && kfound && mk && dm && em && int_rewards && bonus && modulator,
                 "ppox_ngu_reward: null pointer");
    PPOX_REQUIRE(N >= 1 && N <= 0x7FFFFFFFll, "ppox_ngu_reward: N must lie in [1, 2^31), not %lld", (long long)N);
    PPOX_REQUIRE(K >= 1 && K <= KMAX, "ppox_ngu_reward: K must lie in [1, 16], not %d", (int)K);
    PPOX_REQUIRE(mod_max >= 1.0, "ppox_ngu_reward: mod_max must be at least 1, not %g", mod_max);
    ngu_reward_kernel<<<1, RT, 0, ppox::as_stream(stream)>>>(dk, kfound, mk, err, N, K, dm, em, decay, eps, xi, c, smax,
                                                             mod_max, int_rewards, bonus, modulator);
    PPOX_LAUNCHED("ppox_ngu_reward");
}

extern "C" int ppox_elliptical_bonus(const int32_t* emb, const uint8_t* done, int64_t N, double ridge, double beta,
                                     double* minv, int32_t* count, double* eb, float* rewards, float* bonus,
                                     void* stream) {
    PPOX_REQUIRE(emb && done && minv && count && eb, "ppox_elliptical_bonus: null pointer");
    PPOX_REQUIRE(N >= 1 && N <= 0x7FFFFFFFll, "ppox_elliptical_bonus: N must lie in [1, 2^31), not %lld",
                 (long long)N);
    PPOX_REQUIRE(std::isfinite(ridge) && ridge > 0.0, "ppox_elliptical_bonus: ridge must be finite and positive, not %g",
                 ridge);
    PPOX_REQUIRE(std::isfinite(beta), "ppox_elliptical_bonus: beta must be finite, not %g", beta);
    elliptical_kernel<<<ppox::ceil_div(N, ELL_ENVS), 256, 0, ppox::as_stream(stream)>>>(emb, done, N, ridge, beta, minv,
                                                                                        count, eb, rewards, bonus);
    PPOX_LAUNCHED("ppox_elliptical_bonus");
}

extern "C" int ppox_ngu_modulate(const double* eb, const float* err, int64_t N, double* em, double mod_max,
                                 float* int_rewards, float* bonus, float* modulator, void* stream) {
    PPOX_REQUIRE(eb && em && int_rewards && bonus && modulator, "ppox_ngu_modulate: null pointer");
    PPOX_REQUIRE(N >= 1 && N <= 0x7FFFFFFFll, "ppox_ngu_modulate: N must lie in [1, 2^31), not %lld", (long long)N);
    PPOX_REQUIRE(mod_max >= 1.0, "ppox_ngu_modulate: mod_max must be at least 1, not %g", mod_max);
    ngu_modulate_kernel<<<1, RT, 0, ppox::as_stream(stream)>>>(eb, err, N, em, mod_max, int_rewards, bonus,
                                                               modulator);
    PPOX_LAUNCHED("ppox_ngu_modulate");
}
