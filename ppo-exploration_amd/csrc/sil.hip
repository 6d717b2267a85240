// K12 — self-imitation learning (PPO(sil=True)): a step-major prioritized replay ring on the
// device, its two f64 segment trees, proportional sampling and the fused SIL loss.
//
// Replaces (reference):
//   SilModule.add_episode / discount_with_dones   sil_module.py:40-55, 99-105
//   PrioritizedReplayBuffer.add                    buffer.py:429-444
//   sample_proportional + get (IS weights)         buffer.py:446-472
//   SilModule.train's loss                         sil_module.py:64-84
//   update_priorities                              buffer.py:454-459
// The reference's SilModule cannot be constructed; the definition these kernels follow is
// tests/sil_twin.py, pinned to the reference's running parts.
//
// Ring: S steps x N envs, slot (s, n) at s*N + n like the rollout; the flat env-major index
// i = n*S + s is the tree leaf and the minibatch index (convs.RolloutRows / ppox_gather_rows
// with T = S).  Trees: 2P f64 nodes each, node k's children 2k and 2k + 1, leaf i at P + i.
// Every internal node is exactly op(left, right) of its current children, so a bottom-up
// rebuild and a path update give the same bits as the reference's SegmentTree.__setitem__.
// No floating-point atomics and no order-dependent reductions: results repeat bit for bit.
#include "categorical.h"
#include "common.h"

namespace {

constexpr int LP = PPOX_LOSS_PARTIALS;
constexpr int NS = 4;  // partial columns of the loss: surrogate, masked entropy, value, advantage
constexpr uint8_t PENDING = 1, ACTIVE = 2;  // the slot's state byte (0: empty)
constexpr int TREE_CHUNK = 1024;  // nodes one block reduces to one

// p^alpha of a priority; alpha == 1 (plain proportional sampling) is the identity bit for bit, as in
// the host's libm, which the device's pow does not promise
__device__ inline double priority_pow(double p, double alpha) { return alpha == 1.0 ? p : pow(p, alpha); }

__device__ inline double inf64() { return __longlong_as_double(0x7FF0000000000000LL); }

__global__ void __launch_bounds__(256) append_kernel(const int32_t* __restrict__ actions,
                                                     const float* __restrict__ logp,
                                                     const float* __restrict__ rewards,
                                                     const uint8_t* __restrict__ dones, long long T, long long N,
                                                     int32_t* __restrict__ r_actions, float* __restrict__ r_logp,
                                                     float* __restrict__ r_ret, uint8_t* __restrict__ r_dones,
                                                     uint8_t* __restrict__ r_state, long long S, long long head,
                                                     double* __restrict__ sum_tree, double* __restrict__ min_tree,
                                                     long long P) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= T * N) return;
    const long long t = k / N, n = k % N;
    const long long s = (head + t) % S;
    const long long o = s * N + n;
    r_actions[o] = actions[k];
    r_logp[o] = logp[k];
    r_ret[o] = rewards[k];
    r_dones[o] = dones[k];
    r_state[o] = PENDING;
    const long long leaf = P + n * S + s;
    sum_tree[leaf] = 0.0;
    min_tree[leaf] = inf64();
}

// one lane per env: from the newest step backwards over the env's pending slots
__global__ void __launch_bounds__(64) returns_kernel(float* __restrict__ r_ret, const uint8_t* __restrict__ r_dones,
                                                     uint8_t* __restrict__ r_state, long long S, long long N,
                                                     long long newest, double gamma, double alpha,
                                                     const double* __restrict__ max_priority,
                                                     double* __restrict__ sum_tree, double* __restrict__ min_tree,
                                                     long long P) {
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const double pw = priority_pow(*max_priority, alpha);
    double R = 0.0;
    bool closed = false;  // a done was met: the slots from there on belong to finished episodes
    long long s = newest;
    for (long long k = 0; k < S; ++k) {
        const long long o = s * N + n;
        if (r_state[o] != PENDING) break;
        const bool done = r_dones[o] != 0;
        closed = closed || done;
        if (closed) {
            const double r = (double)r_ret[o];
            R = done ? r : r + gamma * R;
            r_ret[o] = (float)R;
            r_state[o] = ACTIVE;
            const long long leaf = P + n * S + s;
            sum_tree[leaf] = pw;
            min_tree[leaf] = pw;
        }
        s = s == 0 ? S - 1 : s - 1;
    }
}

__device__ inline double min2(double l, double r) { return r < l ? r : l; }

// Block b reduces the C nodes [W + b*C, W + (b+1)*C) of the level that has W nodes to the one
// node W/C + b, level by level (each parent = op of its two children, written before it is read).
__global__ void __launch_bounds__(256) tree_up_kernel(double* __restrict__ sum_tree, double* __restrict__ min_tree,
                                                      long long W, int C) {
    long long base = W + (long long)blockIdx.x * C;  // first child of this block at the current level
    for (int w = C >> 1; w >= 1; w >>= 1) {
        base >>= 1;  // first parent
        for (int t = threadIdx.x; t < w; t += blockDim.x) {
            const long long p = base + t;
            sum_tree[p] = sum_tree[2 * p] + sum_tree[2 * p + 1];
            min_tree[p] = min2(min_tree[2 * p], min_tree[2 * p + 1]);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) count_active_kernel(const uint8_t* __restrict__ state, long long slots,
                                                           unsigned long long* __restrict__ n_active) {
    __shared__ unsigned int red[256 / 64];
    unsigned int c = 0;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < slots; k += (long long)gridDim.x * blockDim.x)
        c += state[k] == ACTIVE;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int tot = red[0] + red[1] + red[2] + red[3];
        if (tot) atomicAdd(n_active, (unsigned long long)tot);  // integers: any order, same sum
    }
}

__global__ void __launch_bounds__(256) sample_kernel(const double* __restrict__ sum_tree,
                                                     const double* __restrict__ min_tree, long long P,
                                                     const long long* __restrict__ n_active,
                                                     const double* __restrict__ u, long long B, double beta,
                                                     long long* __restrict__ idx, float* __restrict__ weights) {
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double total = sum_tree[1];
    double mass = u[b] * total;
    long long k = 1;
    while (k < P) {
        const double l = sum_tree[2 * k], r = sum_tree[2 * k + 1];
        // find_prefixsum_idx, plus: never step into a right child that holds nothing
        if (l > mass || r == 0.0) {
            k = 2 * k;
        } else {
            mass -= l;
            k = 2 * k + 1;
        }
    }
    idx[b] = k - P;
    float w = 1.f;
    if (beta > 0.0) {
        const double n = (double)*n_active;
        const double p_min = min_tree[1] / total;
        const double max_w = pow(p_min * n, -beta);
        const double p = sum_tree[k] / total;
        w = (float)(pow(p * n, -beta) / max_w);
    }
    weights[b] = w;
}

struct SilBatch {
    const float* logits;
    const float* values;
    long long B;
    int A;
    const long long* idx;
    long long S, N;
    const int32_t* actions;
    const float* old_logp;
    const float* returns;
    const float* weights;
    float clip, ent_coef;
};

template <int MAXA>
__global__ void __launch_bounds__(256) sil_loss_kernel(SilBatch mb, float* __restrict__ dlogits,
                                                       float* __restrict__ dvalues, float* __restrict__ priority,
                                                       double* __restrict__ partials) {
    __shared__ double red[NS][256 / 64];
    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = 0.0;
    const float invB = (float)(1.0 / (double)mb.B);
    const float lo = 1.f - mb.clip, hi = 1.f + mb.clip;
    const long long slots = mb.S * mb.N;
    for (long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x; b < mb.B; b += (long long)gridDim.x * blockDim.x) {
        const long long i = mb.idx[b];
        float* dz = dlogits + b * mb.A;
        if (i < 0 || i >= slots) {  // never produced by ppox_sil_sample; keeps a bad index in bounds
            for (int j = 0; j < mb.A; ++j) dz[j] = 0.f;
            dvalues[b] = 0.f;
            priority[b] = 0.f;
            continue;
        }
        const long long e = elem(i, mb.S, mb.N);
        CatRow<MAXA> r;
        categorical_forward<MAXA>(mb.logits + b * mb.A, mb.A, r);
        const int a = mb.actions[e];
        float lpa = 0.f;
#pragma unroll
        for (int j = 0; j < MAXA; ++j)
            if (j == a) lpa = r.lp[j];
        const float w = mb.weights[b];
        const float delta = mb.returns[e] - mb.values[b];
        const float adv = clampf(delta, 0.f, 10.f);
        const bool better = delta > 0.f;
        const float ratio = expf(lpa - mb.old_logp[e]);
        const float s1 = adv * ratio;
        const float s2 = adv * clampf(ratio, lo, hi);
        acc[0] += (double)(w * fminf(s1, s2));
        acc[1] += better ? (double)r.ent : 0.0;
        acc[2] += (double)(0.5f * w * (adv * adv));
        acc[3] += (double)adv;
        priority[b] = adv;
        // L = 0.1 * (L_pol + ent_coef * L_ent) + 0.01 * L_val
        const float g_surr = -(0.1f * invB) * w;
        const float g_ent = better ? -(0.1f * mb.ent_coef) * invB : 0.f;
        const float g1 = s1 < s2 ? g_surr : (s1 == s2 ? g_surr * 0.5f : 0.f);
        const float g2 = s2 < s1 ? g_surr : (s1 == s2 ? g_surr * 0.5f : 0.f);
        const float g_ratio = g1 * adv + ((ratio >= lo && ratio <= hi) ? g2 * adv : 0.f);
        const float g_lpa = g_ratio * ratio;
        // back through log(clamp(q)), q = p / s, p = softmax(z) (as ppox_ppo_loss_backward)
        float gq[MAXA];
        float gs = 0.f;
#pragma unroll
        for (int j = 0; j < MAXA; ++j)
            if (j < mb.A) {
                const float g_lp = -g_ent * r.q[j] + (j == a ? g_lpa : 0.f);
                const float g_c = g_lp / r.c[j];
                const bool mask = r.q[j] >= F32_EPS && r.q[j] <= 1.0f - F32_EPS;
                gq[j] = -g_ent * r.lp[j] + (mask ? g_c : 0.f);
                gs += -gq[j] * (r.q[j] / r.s);
            }
        float dot = 0.f;
        float gp[MAXA];
#pragma unroll
        for (int j = 0; j < MAXA; ++j)
            if (j < mb.A) {
                gp[j] = gq[j] / r.s + gs;
                dot += gp[j] * r.p[j];
            }
#pragma unroll
        for (int j = 0; j < MAXA; ++j)
            if (j < mb.A) dz[j] = r.p[j] * (gp[j] - dot);
        // d(0.01 * mean(0.5 w a^2)) / dV, a = clamp(R - V, 0, 10) (clamp mask inclusive)
        dvalues[b] = (delta >= 0.f && delta <= 10.f) ? -((0.01f * invB) * w * adv) : 0.f;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        double x = acc[k];
        for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
        if (lane == 0) red[k][wv] = x;
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        double x = 0.0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) x += red[threadIdx.x][w];
        partials[blockIdx.x * NS + threadIdx.x] = x;
    }
}

__global__ void sil_loss_reduce(const double* __restrict__ partials, double B, float ent_coef,
                                double* __restrict__ loss_accum) {
    __shared__ double tot[NS];
    if (threadIdx.x < NS) {
        double x = 0.0;
        for (int p = 0; p < LP; ++p) x += partials[p * NS + threadIdx.x];
        tot[threadIdx.x] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double pol = -(tot[0] / B), ent = -(tot[1] / B), val = tot[2] / B;
        loss_accum[0] += 0.1 * (pol + (double)ent_coef * ent) + 0.01 * val;
        loss_accum[1] += tot[3] / B;
        loss_accum[2] += 1.0;
    }
}

// one workgroup: leaves (the last occurrence of a repeated index wins), max_priority, then the
// touched leaves' ancestors level by level
__global__ void __launch_bounds__(256) update_priorities_kernel(const long long* __restrict__ idx,
                                                                const float* __restrict__ priority, long long B,
                                                                double alpha, double* __restrict__ sum_tree,
                                                                double* __restrict__ min_tree, long long P,
                                                                double* __restrict__ max_priority) {
    __shared__ double red[256 / 64];
    double pmax = 0.0;
    for (long long b = threadIdx.x; b < B; b += blockDim.x) {
        const long long i = idx[b];
        if (i < 0 || i >= P) continue;
        const double p = fmax((double)priority[b], 1e-6);
        pmax = fmax(pmax, p);
        bool last = true;
        for (long long c = b + 1; c < B; ++c)
            if (idx[c] == i) {
                last = false;
                break;
            }
        if (last) {
            const double pw = priority_pow(p, alpha);
            sum_tree[P + i] = pw;
            min_tree[P + i] = pw;
        }
    }
    for (int o = 32; o > 0; o >>= 1) pmax = fmax(pmax, __shfl_down(pmax, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = pmax;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double m = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
        *max_priority = fmax(*max_priority, m);
    }
    for (int level = 1; (P >> level) >= 1; ++level) {  // leaf i's ancestor `level` levels up
        for (long long b = threadIdx.x; b < B; b += blockDim.x) {
            const long long i = idx[b];
            if (i < 0 || i >= P) continue;
            const long long k = (P + i) >> level;
            sum_tree[k] = sum_tree[2 * k] + sum_tree[2 * k + 1];
            min_tree[k] = min2(min_tree[2 * k], min_tree[2 * k + 1]);
        }
        __syncthreads();
    }
}

bool pow2(long long x) { return x > 0 && (x & (x - 1)) == 0; }

}  // namespace

extern "C" int ppox_sil_append(const void* obs, int64_t obs_step_bytes, const int32_t* actions,
                               const float* log_probs, const float* rewards, const uint8_t* dones, int64_t T,
                               int64_t N, void* ring_obs, int32_t* ring_actions, float* ring_log_probs,
                               float* ring_returns, uint8_t* ring_dones, uint8_t* ring_state, int64_t S,
                               int64_t head, double* sum_tree, double* min_tree, int64_t P, void* stream) {
    PPOX_REQUIRE(T > 0 && N > 0 && S > 0 && T <= S, "ppox_sil_append: need 0 < T <= S and N > 0 (T=%lld S=%lld N=%lld)",
                 (long long)T, (long long)S, (long long)N);
    PPOX_REQUIRE(head >= 0 && head < S, "ppox_sil_append: head %lld outside [0, %lld)", (long long)head, (long long)S);
    PPOX_REQUIRE(pow2(P) && P >= S * N, "ppox_sil_append: P=%lld must be a power of two >= S*N", (long long)P);
    PPOX_REQUIRE(actions && log_probs && rewards && dones && ring_actions && ring_log_probs && ring_returns &&
                     ring_dones && ring_state && sum_tree && min_tree,
                 "ppox_sil_append: null pointer");
    PPOX_REQUIRE((obs == nullptr) == (ring_obs == nullptr) && (!obs || obs_step_bytes > 0),
                 "ppox_sil_append: obs / ring_obs / obs_step_bytes disagree");
    hipStream_t s = ppox::as_stream(stream);
    if (obs) {  // the ring is step-major: a rollout is one range, or two where it wraps
        const int64_t first = T < S - head ? T : S - head;
        PPOX_HIP(hipMemcpyAsync(static_cast<char*>(ring_obs) + head * obs_step_bytes, obs, first * obs_step_bytes,
                                hipMemcpyDeviceToDevice, s),
                 "ppox_sil_append");
        if (first < T)
            PPOX_HIP(hipMemcpyAsync(ring_obs, static_cast<const char*>(obs) + first * obs_step_bytes,
                                    (T - first) * obs_step_bytes, hipMemcpyDeviceToDevice, s),
                     "ppox_sil_append");
    }
    append_kernel<<<ppox::ceil_div(T * N, 256), 256, 0, s>>>(actions, log_probs, rewards, dones, T, N, ring_actions,
                                                             ring_log_probs, ring_returns, ring_dones, ring_state, S,
                                                             head, sum_tree, min_tree, P);
    PPOX_LAUNCHED("ppox_sil_append");
}

extern "C" int ppox_sil_returns(float* ring_returns, const uint8_t* ring_dones, uint8_t* ring_state, int64_t S,
                                int64_t N, int64_t newest, double gamma, double alpha, const double* max_priority,
                                double* sum_tree, double* min_tree, int64_t P, void* stream) {
    PPOX_REQUIRE(S > 0 && N > 0 && newest >= 0 && newest < S, "ppox_sil_returns: bad sizes S=%lld N=%lld newest=%lld",
                 (long long)S, (long long)N, (long long)newest);
    PPOX_REQUIRE(pow2(P) && P >= S * N, "ppox_sil_returns: P=%lld must be a power of two >= S*N", (long long)P);
    PPOX_REQUIRE(ring_returns && ring_dones && ring_state && max_priority && sum_tree && min_tree,
                 "ppox_sil_returns: null pointer");
    returns_kernel<<<ppox::ceil_div(N, 64), 64, 0, ppox::as_stream(stream)>>>(
        ring_returns, ring_dones, ring_state, S, N, newest, gamma, alpha, max_priority, sum_tree, min_tree, P);
    PPOX_LAUNCHED("ppox_sil_returns");
}

extern "C" int ppox_sil_tree_rebuild(double* sum_tree, double* min_tree, int64_t P, const uint8_t* ring_state,
                                     int64_t slots, int64_t* n_active, void* stream) {
    PPOX_REQUIRE(pow2(P) && slots >= 0 && slots <= P, "ppox_sil_tree_rebuild: P=%lld must be a power of two >= slots=%lld",
                 (long long)P, (long long)slots);
    PPOX_REQUIRE(sum_tree && min_tree && (slots == 0 || ring_state) && n_active, "ppox_sil_tree_rebuild: null pointer");
    hipStream_t s = ppox::as_stream(stream);
    for (int64_t W = P; W > 1;) {
        const int C = (int)(W < TREE_CHUNK ? W : TREE_CHUNK);
        tree_up_kernel<<<(unsigned)(W / C), 256, 0, s>>>(sum_tree, min_tree, W, C);
        PPOX_LAUNCHED_NORET("ppox_sil_tree_rebuild");
        W /= C;
    }
    PPOX_HIP(hipMemsetAsync(n_active, 0, sizeof(int64_t), s), "ppox_sil_tree_rebuild");
    if (slots > 0) {
        const unsigned blocks = ppox::ceil_div(slots, 256 * 16);
        count_active_kernel<<<blocks < 1024u ? blocks : 1024u, 256, 0, s>>>(
            ring_state, slots, reinterpret_cast<unsigned long long*>(n_active));
    }
    PPOX_LAUNCHED("ppox_sil_tree_rebuild");
}

extern "C" int ppox_sil_sample(const double* sum_tree, const double* min_tree, int64_t P, const int64_t* n_active,
                               const double* u, int64_t B, double beta, int64_t* idx, float* weights, void* stream) {
    if (B == 0) return PPOX_OK;
    PPOX_REQUIRE(pow2(P) && B > 0 && beta >= 0.0, "ppox_sil_sample: bad sizes P=%lld B=%lld beta=%g", (long long)P,
                 (long long)B, beta);
    PPOX_REQUIRE(sum_tree && min_tree && n_active && u && idx && weights, "ppox_sil_sample: null pointer");
    sample_kernel<<<ppox::ceil_div(B, 256), 256, 0, ppox::as_stream(stream)>>>(
        sum_tree, min_tree, P, reinterpret_cast<const long long*>(n_active), u, B, beta,
        reinterpret_cast<long long*>(idx), weights);
    PPOX_LAUNCHED("ppox_sil_sample");
}

extern "C" int ppox_sil_loss(const float* logits, const float* values, int64_t B, int32_t A, const int64_t* idx,
                             int64_t S, int64_t N, const int32_t* ring_actions, const float* ring_log_probs,
                             const float* ring_returns, const float* weights, float clip, float ent_coef,
                             float* dlogits, float* dvalues, float* priority, double* partials, double* loss_accum,
                             void* stream) {
    PPOX_REQUIRE(A >= 1 && A <= 64, "ppox_sil_loss: n_actions=%d outside [1,64]", A);
    PPOX_REQUIRE(B >= 1 && S > 0 && N > 0, "ppox_sil_loss: bad sizes B=%lld S=%lld N=%lld", (long long)B, (long long)S,
                 (long long)N);
    PPOX_REQUIRE(logits && values && idx && ring_actions && ring_log_probs && ring_returns && weights && dlogits &&
                     dvalues && priority && partials && loss_accum,
                 "ppox_sil_loss: null pointer");
    SilBatch mb{logits, values, B, A, reinterpret_cast<const long long*>(idx), S, N, ring_actions, ring_log_probs,
                ring_returns, weights, clip, ent_coef};
    hipStream_t s = ppox::as_stream(stream);
    PPOX_DISPATCH_A(A, MA, { sil_loss_kernel<MA><<<LP, 256, 0, s>>>(mb, dlogits, dvalues, priority, partials); });
    PPOX_LAUNCHED_NORET("ppox_sil_loss");
    sil_loss_reduce<<<1, 64, 0, s>>>(partials, (double)B, ent_coef, loss_accum);
    PPOX_LAUNCHED("ppox_sil_loss");
}

extern "C" int ppox_sil_update_priorities(const int64_t* idx, const float* priority, int64_t B, double alpha,
                                          double* sum_tree, double* min_tree, int64_t P, double* max_priority,
                                          void* stream) {
    if (B == 0) return PPOX_OK;
    PPOX_REQUIRE(pow2(P) && B > 0, "ppox_sil_update_priorities: bad sizes P=%lld B=%lld", (long long)P, (long long)B);
    PPOX_REQUIRE(idx && priority && sum_tree && min_tree && max_priority, "ppox_sil_update_priorities: null pointer");
    update_priorities_kernel<<<1, 256, 0, ppox::as_stream(stream)>>>(reinterpret_cast<const long long*>(idx), priority,
                                                                      B, alpha, sum_tree, min_tree, P, max_priority);
    PPOX_LAUNCHED("ppox_sil_update_priorities");
}
