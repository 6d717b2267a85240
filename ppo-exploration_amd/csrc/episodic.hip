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

__global__ void __launch_bounds__(RT)
    episodic_reward_kernel(const double* __restrict__ dk, const int32_t* __restrict__ kfound,
                           const double* __restrict__ mk, long long N, int K, double* __restrict__ dm, double decay,
                           double beta, double eps, double xi, double c, double smax, float* __restrict__ rewards,
                           float* __restrict__ bonus) {
    __shared__ double wsum[RW];
    __shared__ long long wcnt[RW];
    __shared__ double dm0;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    long long P = RT;  // the padded length: a power of two, at least one value per thread
    while (P < N) P <<= 1;
    const long long per = P / RT;
    long long cnt = 0;
    for (long long i = tid * per; i < (tid + 1) * per && i < N; ++i) cnt += kfound[i] > 0;
    double v = pair_tree(tid * per, per, [&](long long i) { return i < N && kfound[i] > 0 ? mk[i] : 0.0; });
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {  // lane pairs, then pairs of pairs: the tree's next six levels
        v = v + __shfl_xor(v, o, 64);
        cnt += __shfl_xor(cnt, o, 64);
    }
    if (lane == 0) {
        wsum[wv] = v;
        wcnt[wv] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        long long nv = 0;
        for (int w = 0; w < RW; ++w) nv += wcnt[w];
        for (int s = 1; s < RW; s <<= 1)  // the tree's last levels, over the waves
            for (int w = 0; w < RW; w += 2 * s) wsum[w] = wsum[w] + wsum[w + s];
        const double S = wsum[0];
        double d0 = dm[0];
        if (nv > 0) {
            const double mu = S / (double)nv;
            d0 = dm[1] == 0.0 ? mu : decay * d0 + (1.0 - decay) * mu;
            dm[0] = d0;
            dm[1] = dm[1] + 1.0;
        }
        dm0 = d0;
    }
    __syncthreads();
    const double d0 = dm0;
    for (long long n = tid; n < N; n += RT) {
        const int k = kfound[n] < K ? kfound[n] : K;  // (the knn kernel writes at most K)
        double r = 0.0;
        if (k > 0) {
            double acc = 0.0;
            for (int i = 0; i < k; ++i) {
                double q = d0 > 0.0 ? dk[n * K + i] / d0 : 0.0;
                q = q - xi;
                q = q > 0.0 ? q : 0.0;
                acc = acc + eps / (q + eps);
            }
            const double s = sqrt(acc) + c;
            r = s > smax ? 0.0 : 1.0 / s;
        }
        bonus[n] = (float)r;
        rewards[n] = rewards[n] + (float)(beta * r);
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
