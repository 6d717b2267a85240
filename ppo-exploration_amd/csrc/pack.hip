// K6 — the per-optimizer-step weight packing of the NatureCNN: the f32 forms of the f32 math mode
// (ppox_nature_pack_weights, read by conv_f32.hip) and the split-f16 forms (PackAll: every packed form, its
// amax partials, scale exponent and PX bounds in two launches; read by the GEMMs of conv.hip, conv_split.hip
// and dconv.hip through gemm_layout.h and conv_common.h), the host record of the forms whose tail carries a
// finite PX bound (px_bound_ok), and the two operand-format kernels: a tensor's amax slots (ppox_amax) and
// its PX planes (ppox_px_split).
#include <algorithm>
#include <mutex>
#include <unordered_set>

#include "gemm_layout.h"

namespace {

// ---------------------------------------------------------------------------
// weight packing (once per optimizer step)
// ---------------------------------------------------------------------------
// packed-B position of natural element (k, col) of a [K][NOUT] matrix for conv_f32.hip's rgemm_kernel
__host__ __device__ constexpr int rg_index(int k, int col, int nout) {
    return (k >> 5) * 32 * nout + (col >> 5) * 1024 + ((k & 15) >> 2) * 256 + (((k >> 4) & 1) * 32 + (col & 31)) * 4 +
           (k & 3);
}

// RG: rgemm layout (rg_index); else the igemm's natural [K][NOUT]
template <bool RG>
__device__ inline int pack_pos(int k, int col, int nout, int i) {
    if constexpr (RG) return rg_index(k, col, nout);
    return i;
}
// forward: [K][COUT] in the kernel's K order
template <class L, bool NHWC_ORDER, bool RG>
__global__ void pack_fwd(const float* __restrict__ w, float* __restrict__ wp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L::K * L::COUT) return;
    const int k = i / L::COUT, co = i % L::COUT;
    int ci, ky, kx;
    if (NHWC_ORDER) {
        ci = k % L::CIN;
        const int tap = k / L::CIN;
        ky = tap / L::KW;
        kx = tap % L::KW;
    } else {
        kx = k % L::KW;
        ky = (k / L::KW) % L::KH;
        ci = k / (L::KW * L::KH);
    }
    wp[pack_pos<RG>(k, co, L::COUT, i)] = w[((co * L::CIN + ci) * L::KH + ky) * L::KW + kx];
}

// dgrad: [(ky, kx, co)][ci] — chunk (tap, 32 co) is a contiguous 32 x CIN block
template <class L, bool RG>
__device__ inline void pack_dgrad_elem(const float* __restrict__ w, float* __restrict__ wp, int i) {
    if (i >= L::KH * L::KW * L::COUT * L::CIN) return;
    const int ci = i % L::CIN, co = (i / L::CIN) % L::COUT, tap = i / (L::CIN * L::COUT);
    wp[pack_pos<RG>(tap * L::COUT + co, ci, L::CIN, i)] = w[((co * L::CIN + ci) * L::KH + tap / L::KW) * L::KW + tap % L::KW];
}
template <class L, bool RG>
__global__ void pack_dgrad(const float* __restrict__ w, float* __restrict__ wp) {
    pack_dgrad_elem<L, RG>(w, wp, blockIdx.x * blockDim.x + threadIdx.x);
}

// Every per-optimizer-step weight packing of the training step in two launches (the
// minibatch loop is launch-bound at small per-rank batches): wmax_kernel (each weight
// tensor's amax partials, into the tails of the forms packed from it), then pack_all_kernel
// (element ranges of the jobs laid end to end, null outputs skipped; each wave derives the
// tensors' scales from the partials, and the first wave writes every form's exponent).
struct PackAll {
    const float *w1, *w2, *w3, *wfc;
    float* wpd2;                                       // f32 dgrad2 [(tap, co)][ci]
    uint16_t *q1, *q2, *q3, *qd2, *qd3, *qfcf, *qfcd;  // split planes
    const float* wh = nullptr;                         // the heads' hidden layer (512 x 512)
    uint16_t *qhf = nullptr, *qhd = nullptr;           // its forward (W^T) and dgrad (W) forms
    const float* b1 = nullptr;                         // conv1 bias (with q1: the H1P exponent)
    uint32_t* zero = nullptr;                          // words zeroed by wmax_kernel (a pass's amax table)
    long long zero_words = 0;
    const float *b2 = nullptr, *b3 = nullptr;          // conv2 / conv3 biases (with q2 / q3: the PX bounds)
    // round 6: the tensors' amax partials as the Adam step recorded them ([PA_TENSORS][AMAX_SLOTS], the weights
    // unchanged since; null: the packing's own amax pass), and the partials buffer the next Adam step records into
    // (zeroed here; nullable)
    const uint32_t* amax_in = nullptr;
    uint32_t* amax_next = nullptr;
};
constexpr long long PA_N1 = 8 * 2 * 64 * 8;
// the split-GEMM jobs run in 8-element units (pack_frag_unit); q1 and wpd2 per element
constexpr long long PU_2 = PA_N2 / 8, PU_3 = PA_N3 / 8, PU_FC = PA_NFC / 8, PU_FCD = PA_NFCD / 8, PU_H = PA_NH / 8;

// source value (k, col) of layer L's forward [K][COUT] (NHWC K order) or dgrad [(tap, co)][ci]
// matrix, from the PyTorch [co][ci][ky][kx] weights
template <class L, bool DGRAD>
struct ConvSrc {
    const float* w;
    __device__ float operator()(int k, int col) const {
        int co, ci, tap;
        if (DGRAD) {
            ci = col;
            co = k % L::COUT;
            tap = k / L::COUT;
        } else {
            co = col;
            ci = k % L::CIN;
            tap = k / L::CIN;
        }
        return w[((co * L::CIN + ci) * L::KH + tap / L::KW) * L::KW + tap % L::KW];
    }
};
// source value (k, col) of column block cb of a GemmRows B (w[n][k] when TRANS, w[k][n] otherwise);
// PERM (the fc layer): its 3136-wide side (K of the forward, N of the dgrad) in NHWC feature order
template <class Prob, bool TRANS, bool PERM>
struct RowsSrc {
    const float* w;
    int cb;
    __device__ float operator()(int k, int col) const {
        const int n = cb * Prob::NOUT + col;
        if (n >= Prob::N) return 0.f;
        const int f = PERM ? fc_nchw_feature(TRANS ? k : n) : (TRANS ? k : n);
        return TRANS ? w[(long long)n * Prob::K + f] : w[(long long)k * Prob::N + f];
    }
};
template <class Prob, bool TRANS, bool PERM = true>
__device__ inline void pack_rows_unit(const float* w, float s, uint16_t* q, long long u) {
    constexpr long long per = (long long)Prob::K * Prob::NOUT / 8;
    const int cb = (int)(u / per);
    pack_frag_unit<Prob::NOUT>(RowsSrc<Prob, TRANS, PERM>{w, cb}, s, q + (long long)cb * Prob::K * Prob::NOUT * NPL,
                               u - cb * per);
}

// The fc forms, enumerated so that consecutive units read consecutive floats of w (the
// permutation f = p * 64 + c <- c * 49 + p otherwise turns every lane's reads into 49-float
// strides across all of W): unit u = (outer, c-group or k-group, p) with p (0..48) fastest.
//   TRANS (forward, B[k][n] = W[n][c * 49 + p], k = p * 64 + c): u = (n, g, p), values
//     c = 8g .. 8g + 7 of column n at k0 = p * 64 + 8g;
//   dgrad (B[k][n] = W[k][c * 49 + p], n = p * 64 + c): u = (kg, c, p), values k = 8kg .. 8kg + 7
//     of column n (block p, column c of the block).
template <bool TRANS>
__device__ inline void pack_fc_unit(const float* __restrict__ w, float s, uint16_t* __restrict__ q, long long u) {
    constexpr int K = TRANS ? 3136 : 512, NT = 2;
    const int p = (int)(u % 49);
    const long long r = u / 49;
    int k0, col, cb;
    float v[8];
    if constexpr (TRANS) {
        const int g = (int)(r & 7), n = (int)(r >> 3);
        const float* src = w + (long long)n * 3136 + 8 * g * 49 + p;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = src[e * 49];
        k0 = p * 64 + 8 * g, col = n & 63, cb = n >> 6;
    } else {
        const int c = (int)(r & 63), kg = (int)(r >> 6);
        const float* src = w + (long long)(8 * kg) * 3136 + c * 49 + p;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = src[(long long)e * 3136];
        k0 = 8 * kg, col = c, cb = p;
    }
    u32x4 p0, p1;
    split8h(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), s, p0, p1);
    const int cs = k0 >> 4, h = (k0 >> 3) & 1, j = col >> 5, l = h * 32 + (col & 31);
    u32x4* d = reinterpret_cast<u32x4*>(q + (long long)cb * K * 64 * NPL + ((long long)(cs * NT + j) * NPL) * 512) + l;
    d[0] = p0;
    d[64] = p1;
}

// the forms packed from weight tensor t (0: w1, 1: w2, 2: w3, 3: wfc) and their plane counts
__device__ inline void pa_forms(const PackAll& p, int t, uint16_t* (&f)[2], long long& planes) {
    switch (t) {
        case 0: f[0] = p.q1; f[1] = nullptr; planes = PL_Q1; break;
        case 1: f[0] = p.q2; f[1] = p.qd2; planes = PL_Q2; break;
        case 2: f[0] = p.q3; f[1] = p.qd3; planes = PL_Q3; break;
        case 3: f[0] = p.qfcf; f[1] = p.qfcd; planes = PL_FCF; break;
        default: f[0] = p.qhf; f[1] = p.qhd; planes = PL_H; break;
    }
}
constexpr int PA_TENSORS = 5;

// The H1P exponent of conv1's output (one workgroup): |h1| <= 255 max_c (sum_k |W1[c][k]|) +
// |b1[c]| for uint8 frames; thread t sums k-range t & 7 of channel t >> 3 in f64.  Stored in
// slot H1P_EXP_SLOT of q1's tail, read by the conv1 forward (output scale) and the H1P consumers.
// The bound carries a 2^-10 margin, so every value times 2^E stays below 2^15 (f16 max 65504).
__device__ void h1p_exp_block(const float* __restrict__ w1, const float* __restrict__ b1, uint16_t* __restrict__ q1) {
    const int t = threadIdx.x, c = t >> 3, part = t & 7;
    double sum = 0.0;
    for (int k = part * 32; k < part * 32 + 32; ++k) sum += fabs((double)w1[c * G1::K + k]);
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) sum += __shfl_xor(sum, o);
    double bound = 255.0 * sum + fabs((double)b1[c]);
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) bound = fmax(bound, __shfl_xor(bound, o));
    __shared__ double red[4];
    if ((t & 63) == 0) red[t >> 6] = bound;
    __syncthreads();
    if (t == 0) {
        const double m = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
        const float mf = (float)(m * (1.0 + 1.0 / 1024.0));
        pack_tail(q1, PL_Q1)[AMAX_SLOTS + H1P_EXP_SLOT] = (uint32_t)split_scale_exp(__float_as_uint(mf));
    }
}

// The PX output bounds (round 4): column l1-norms sum_k |B[k][n]| of a packed form's matrix, their
// maximum as AMAX_SLOTS partials in the form's tail (NORM_SLOT0; every slot written) and the bias
// bound max |b| (BMAX_SLOT; NaN without a bias, so a PX output bounded without it comes out NaN).
// Job 0: q2 (conv2 forward, n = co: W2[co][:], 512 contiguous), job 1: q3 (conv3 forward, 576),
// job 2: qfcd (fc dgrad, n = a feature q: W[:][q] over the 512 outputs, 16 features per workgroup),
// job 3: qd3 (conv3 dgrad, n = ci: W3[:][ci][:][:] over the 576 (co, ky, kx); no bias: bound 0 — the PX
// g2 of round 5).  Fixed summation orders (f32; the bound's 2^-10 margin covers their rounding):
// deterministic.
constexpr int PA_NORM_JOBS = 4;
__device__ void norm_block(const PackAll& p, int job, int b) {
    __shared__ float red[256];
    const int t = threadIdx.x;
    float colmax = 0.f;
    if (job == 3) {
        if (!p.qd3) return;
        float sum = 0.f;
        if (b < 64) {  // input channel b: threads stride its 576 (co, tap) weights
            for (int k = t; k < G3::K; k += 256) sum += fabsf(p.w3[((k / 9) * 64 + b) * 9 + k % 9]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if ((t & 63) == 0) red[t >> 6] = sum;
        __syncthreads();
        if (t == 0) {
            uint32_t* tail = pack_tail(p.qd3, PL_Q3);
            tail[NORM_SLOT0 + b] = __float_as_uint((red[0] + red[1]) + (red[2] + red[3]));
            if (b == 0) tail[AMAX_SLOTS + BMAX_SLOT] = 0u;
        }
        return;
    }
    if (job < 2) {
        uint16_t* q = job == 0 ? p.q2 : p.q3;
        if (!q) return;
        const float* w = job == 0 ? p.w2 : p.w3;
        const int K = job == 0 ? G2::K : G3::K;
        const float* bias = job == 0 ? p.b2 : p.b3;
        float sum = 0.f;
        if (b < 64) {  // output channel b (COUT = 64): threads stride its K weights
            for (int k = t; k < K; k += 256) sum += fabsf(w[b * K + k]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);  // a fixed butterfly: deterministic
        if ((t & 63) == 0) red[t >> 6] = sum;
        __syncthreads();
        if (t == 0) {
            const float tot = (red[0] + red[1]) + (red[2] + red[3]);
            uint32_t* tail = pack_tail(q, job == 0 ? PL_Q2 : PL_Q3);
            tail[NORM_SLOT0 + b] = __float_as_uint(tot);
            if (b == 0) {
                float bm = bias ? 0.f : __builtin_nanf("");
                if (bias)
                    for (int i = 0; i < 64; ++i) bm = fmaxf(bm, fabsf(bias[i]));
                tail[AMAX_SLOTS + BMAX_SLOT] = __float_as_uint(bm);
            }
        }
        return;
    }
    if (!p.qfcd) return;
    // features 16 b .. 16 b + 15 (b < 196): thread (part = t >> 4, f = t & 15) sums outputs 32 part ..
    const int f = 16 * b + (t & 15), part = t >> 4;
    float sum = 0.f;
    if (f < 3136) {
#pragma unroll 8
        for (int k = 32 * part; k < 32 * part + 32; ++k) sum += fabsf(p.wfc[(long long)k * 3136 + f]);
    }
    red[t] = sum;
    __syncthreads();
    if (t < 16) {
        float tot = 0.f;
        for (int i = 0; i < 16; ++i) tot += red[16 * i + t];
        colmax = tot;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) colmax = fmaxf(colmax, __shfl_xor(colmax, o, 16));
        if (t == 0) {
            uint32_t* tail = pack_tail(p.qfcd, PL_FCD);
            tail[NORM_SLOT0 + b] = __float_as_uint(colmax);
            if (b == 0) tail[AMAX_SLOTS + BMAX_SLOT] = 0u;  // the dgrad has no bias
        }
    }
}

// AMAX_SLOTS workgroups per weight tensor: workgroup b's max |w| over its stride into slot b of
// the tails of both forms (every slot written: no zeroing), so the packer's amax_read sees the
// tensor's max.  Then AMAX_SLOTS workgroups per PX norm job, one workgroup for the H1P exponent
// (with q1 and b1), then the workgroups zeroing p.zero (the next pass's amax table: no fill launch
// of its own)
// The packing's auxiliary workgroups (nb = 0, 1, ...): the PX norm jobs, the H1P exponent, the zeroing of p.zero
// (1,024 words per workgroup) and of p.amax_next, and — with p.amax_in — one workgroup per tensor copying the
// given amax partials into the tails of its forms (where the amax pass would have written them)
constexpr int PA_NEXT_WORDS = PA_TENSORS * AMAX_SLOTS, PA_NEXT_BLOCKS = (PA_NEXT_WORDS + 1023) / 1024;
static_assert(PA_NEXT_WORDS % 4 == 0, "amax_next: whole uint4 stores");
inline long long pack_aux_blocks(const PackAll& p) {
    return PA_NORM_JOBS * AMAX_SLOTS + 1 + ppox::ceil_div(p.zero_words, 1024LL) + (p.amax_next ? PA_NEXT_BLOCKS : 0) +
           (p.amax_in ? PA_TENSORS : 0);
}
__device__ void pack_aux_block(const PackAll& p, long long nb) {
    if (nb < PA_NORM_JOBS * AMAX_SLOTS) {
        norm_block(p, (int)(nb / AMAX_SLOTS), (int)(nb % AMAX_SLOTS));
        return;
    }
    nb -= PA_NORM_JOBS * AMAX_SLOTS;
    if (nb == 0) {
        if (p.q1 && p.b1) h1p_exp_block(p.w1, p.b1, p.q1);
        return;
    }
    nb -= 1;
    const long long zblocks = (p.zero_words + 1023) / 1024;
    if (nb < zblocks) {
        const long long i = (nb * 256 + threadIdx.x) * 4;  // this thread's four words
        if (i + 4 <= p.zero_words) {
            *reinterpret_cast<uint4*>(p.zero + i) = make_uint4(0u, 0u, 0u, 0u);
        } else {
            for (long long k = i; k < p.zero_words; ++k) p.zero[k] = 0u;  // a ragged tail
        }
        return;
    }
    nb -= zblocks;
    if (p.amax_next) {
        if (nb < PA_NEXT_BLOCKS) {
            const long long i = nb * 256 + threadIdx.x;
            if (4 * i < PA_NEXT_WORDS) reinterpret_cast<uint4*>(p.amax_next)[i] = make_uint4(0u, 0u, 0u, 0u);
            return;
        }
        nb -= PA_NEXT_BLOCKS;
    }
    if (p.amax_in && nb < PA_TENSORS) {
        uint16_t* f[2];
        long long planes;
        pa_forms(p, (int)nb, f, planes);
        const uint32_t v = p.amax_in[nb * AMAX_SLOTS + threadIdx.x];
        for (int k = 0; k < 2; ++k)
            if (f[k]) pack_tail(f[k], planes)[threadIdx.x] = v;
    }
}

__global__ void __launch_bounds__(256) wmax_kernel(PackAll p) {
    if (blockIdx.x >= PA_TENSORS * AMAX_SLOTS) {
        pack_aux_block(p, (long long)blockIdx.x - PA_TENSORS * AMAX_SLOTS);
        return;
    }
    const int t = blockIdx.x / AMAX_SLOTS, b = blockIdx.x % AMAX_SLOTS;
    uint16_t* f[2];
    long long planes;
    pa_forms(p, t, f, planes);
    if (!f[0] && !f[1]) return;
    const float4* w = reinterpret_cast<const float4*>(t == 0 ? p.w1 : t == 1 ? p.w2 : t == 2 ? p.w3 : t == 3 ? p.wfc : p.wh);
    const long long n4 =
        (t == 0 ? (long long)G1::K * G1::COUT : t == 1 ? PA_N2 : t == 2 ? PA_N3 : t == 3 ? 512LL * 3136 : PA_NH) / 4;
    float m = 0.f;
#pragma unroll 8
    for (long long i = (long long)b * 256 + threadIdx.x; i < n4; i += AMAX_SLOTS * 256) {  // (loads issue 8 at a time)
        const float4 v = w[i];
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
    __shared__ uint32_t red[4];
    const uint32_t wm = wave_max_u32(__float_as_uint(m));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = wm;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t v = max(max(red[0], red[1]), max(red[2], red[3]));
        for (int k = 0; k < 2; ++k)
            if (f[k]) pack_tail(f[k], planes)[b] = v;
    }
}

__device__ uint32_t kZeroTail[AMAX_SLOTS] = {};  // the amax partials of a tensor packed into no form

// npack: the packing workgroups; with p.amax_in the auxiliary ones follow them (the amax pass's, in this launch)
__global__ void __launch_bounds__(256) pack_all_kernel(PackAll p, long long total, unsigned npack) {
    if (blockIdx.x >= npack) {
        pack_aux_block(p, (long long)(blockIdx.x - npack));
        return;
    }
    // the tensors' scales (wave-uniform), from the partials of their first packed form (or the given ones); the
    // five reads are unconditional (a tensor with no form reads zeros), so they are one round trip
    float sc[PA_TENSORS];
    uint32_t am[PA_TENSORS];
#pragma unroll
    for (int t = 0; t < PA_TENSORS; ++t) {  // all five loads before the exponent stores below
        uint16_t* f[2];
        long long planes;
        pa_forms(p, t, f, planes);
        uint16_t* src = f[0] ? f[0] : f[1];
        am[t] = amax_read(!src ? kZeroTail : p.amax_in ? p.amax_in + t * AMAX_SLOTS : pack_tail(src, planes));
    }
#pragma unroll
    for (int t = 0; t < PA_TENSORS; ++t) {
        uint16_t* f[2];
        long long planes;
        pa_forms(p, t, f, planes);
        const int e = (f[0] || f[1]) ? split_scale_exp(am[t]) : 0;
        sc[t] = exp2i(e);
        if (blockIdx.x == 0 && threadIdx.x == 0)
            for (int k = 0; k < 2; ++k)
                if (f[k]) pack_tail(f[k], planes)[AMAX_SLOTS] = (uint32_t)e;
    }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)npack * 256) {
        long long j = i;
        if (j < PA_N1) { if (p.q1) pack_fwd1_split_elem(p.w1, sc[0], p.q1, (int)j); continue; }
        j -= PA_N1;
        if (j < PU_2) { if (p.q2) pack_frag_unit<G2::COUT>(ConvSrc<G2, false>{p.w2}, sc[1], p.q2, j); continue; }
        j -= PU_2;
        if (j < PU_3) { if (p.q3) pack_frag_unit<G3::COUT>(ConvSrc<G3, false>{p.w3}, sc[2], p.q3, j); continue; }
        j -= PU_3;
        if (j < PU_2) { if (p.qd2) pack_frag_unit<G2::CIN>(ConvSrc<G2, true>{p.w2}, sc[1], p.qd2, j); continue; }
        j -= PU_2;
        if (j < PU_3) { if (p.qd3) pack_frag_unit<G3::CIN>(ConvSrc<G3, true>{p.w3}, sc[2], p.qd3, j); continue; }
        j -= PU_3;
        if (j < PA_N2) { if (p.wpd2) pack_dgrad_elem<G2, false>(p.w2, p.wpd2, (int)j); continue; }
        j -= PA_N2;
        if (j < PU_FC) { if (p.qfcf) pack_fc_unit<true>(p.wfc, sc[3], p.qfcf, j); continue; }
        j -= PU_FC;
        if (j < PU_FCD) { if (p.qfcd) pack_fc_unit<false>(p.wfc, sc[3], p.qfcd, j); continue; }
        j -= PU_FCD;
        if (j < PU_H) { if (p.qhf) pack_rows_unit<HeadFwd, true, false>(p.wh, sc[4], p.qhf, j); continue; }
        j -= PU_H;
        if (p.qhd) pack_rows_unit<HeadDgrad, false, false>(p.wh, sc[4], p.qhd, j);
    }
}

// Host record of the packed forms whose tail holds a finite PX bias bound: q2 / q3 packed WITH
// their bias (pack_all with b2 / b3), and every fc dgrad form (no bias: its bound is 0).  A form
// packed without its bias (ppox_nature_pack_split, pack_all with a null b2 / b3) carries a NaN
// bound, so an entry point asked for a PX output (y_exp_out / g3_exp_out) refuses such a form
// instead of writing NaN activations.
std::mutex px_mu;
std::unordered_set<const void*> px_bounded;

void note_px_pack(const void* q, bool bounded) {
    if (!q) return;
    std::lock_guard<std::mutex> g(px_mu);
    if (bounded)
        px_bounded.insert(q);
    else
        px_bounded.erase(q);
}

int launch_pack_all(const PackAll& p, hipStream_t s, const char* name) {
    for (const void* q : {(const void*)p.wpd2, (const void*)p.q1, (const void*)p.q2, (const void*)p.q3,
                          (const void*)p.qd2, (const void*)p.qd3, (const void*)p.qfcf, (const void*)p.qfcd})
        PPOX_REQUIRE(!q || ppox::aligned16(q), "ppox_nature_pack: packed buffers must be 16-byte aligned");
    PPOX_REQUIRE((p.w1 || !p.q1) && (p.w2 || (!p.q2 && !p.qd2 && !p.wpd2)) && (p.w3 || (!p.q3 && !p.qd3)) &&
                     (p.wfc || (!p.qfcf && !p.qfcd)) && (p.wh || (!p.qhf && !p.qhd)),
                 "ppox_nature_pack: null weights");
    PPOX_REQUIRE((!p.qhf || ppox::aligned16(p.qhf)) && (!p.qhd || ppox::aligned16(p.qhd)),
                 "ppox_nature_pack: packed buffers must be 16-byte aligned");
    PPOX_REQUIRE(!p.zero_words || (p.zero && ppox::aligned16(p.zero)), "ppox_nature_pack_all: zero buffer");
    PPOX_REQUIRE((!p.amax_in || ppox::aligned16(p.amax_in)) && (!p.amax_next || ppox::aligned16(p.amax_next)) &&
                     (!p.amax_in || p.amax_in != p.amax_next),
                 "ppox_nature_pack_all: amax partials buffers");
    const long long aux = pack_aux_blocks(p);
    if (!p.amax_in) {  // the amax pass, then the packing
        wmax_kernel<<<(unsigned)(PA_TENSORS * AMAX_SLOTS + aux), 256, 0, s>>>(p);
        PPOX_LAUNCHED_NORET(name);
    }
    // element ranges end at the last job present (the head and fc dgrad ranges are the longest)
    const long long total = PA_N1 + 2 * PU_2 + 2 * PU_3 + PA_N2 + PU_FC +
                            (p.qhf || p.qhd ? PU_FCD + 2 * PU_H : (p.qfcd ? PU_FCD : 0));
    // every wave first reads the five tensors' 256 amax partials (5 KB): 4,096 workgroups re-read 80 MB of them
    // through L2 — a few hundred, each striding over more units, read a few MB
    const unsigned blocks = (unsigned)std::min<long long>((total + 255) / 256, 512);
    pack_all_kernel<<<blocks + (unsigned)(p.amax_in ? aux : 0), 256, 0, s>>>(p, total, blocks);
    PPOX_LAUNCHED_NORET(name);
    note_px_pack(p.q2, p.b2 != nullptr);
    note_px_pack(p.q3, p.b3 != nullptr);
    note_px_pack(p.qfcd, true);
    note_px_pack(p.qd3, true);
    return PPOX_OK;
}

}  // namespace

namespace ppox_conv {
bool px_bound_ok(const void* q) {
    std::lock_guard<std::mutex> g(px_mu);
    return px_bounded.count(q) != 0;
}

// split-f16 packing of the conv weights (called from conv_split.hip's entry point)
int pack_split(const float* w1, const float* w2, const float* w3, uint16_t* q1, uint16_t* q2, uint16_t* q3,
               uint16_t* qd2, uint16_t* qd3, hipStream_t s) {
    return launch_pack_all(PackAll{w1, w2, w3, nullptr, nullptr, q1, q2, q3, qd2, qd3, nullptr, nullptr}, s,
                           "ppox_nature_pack_split");
}

long long planes(int which) {
    switch (which) {
        case 1: return PL_Q1;
        case 2: case 12: return PL_Q2;
        case 3: case 13: return PL_Q3;
        case 4: return PL_FCF;
        default: return -1;
    }
}
}  // namespace ppox_conv

extern "C" int ppox_nature_pack_weights(const float* w1, const float* w2, const float* w3, float* wp1, float* wp2,
                                        float* wp3, float* wpd2, float* wpd3, void* stream) {
    // any packed buffer may be null: that packing is skipped (ops running in split math)
    PPOX_REQUIRE(w1 && w2 && w3, "ppox_nature_pack_weights: null weights");
    PPOX_REQUIRE((!wp1 || ppox::aligned16(wp1)) && (!wp2 || ppox::aligned16(wp2)) && (!wp3 || ppox::aligned16(wp3)) &&
                     (!wpd2 || ppox::aligned16(wpd2)) && (!wpd3 || ppox::aligned16(wpd3)),
                 "ppox_nature_pack_weights: packed buffers must be 16-byte aligned");
    hipStream_t s = ppox::as_stream(stream);
    if (wp1) pack_fwd<G1, false, true><<<ppox::ceil_div(G1::K * 32, 256), 256, 0, s>>>(w1, wp1);
    if (wp2) pack_fwd<G2, true, false><<<ppox::ceil_div(G2::K * 64, 256), 256, 0, s>>>(w2, wp2);
    if (wp3) pack_fwd<G3, true, false><<<ppox::ceil_div(G3::K * 64, 256), 256, 0, s>>>(w3, wp3);
    if (wpd2) pack_dgrad<G2, false><<<ppox::ceil_div(G2::K * G2::COUT, 256), 256, 0, s>>>(w2, wpd2);
    if (wpd3) pack_dgrad<G3, false><<<ppox::ceil_div(G3::K * G3::COUT, 256), 256, 0, s>>>(w3, wpd3);
    PPOX_LAUNCHED("ppox_nature_pack_weights");
}

extern "C" int64_t ppox_nature_fc_pack_elems(void) { return PL_FCF + 2 * PACK_TAIL32; }

extern "C" int ppox_nature_fc_pack(const float* w, uint16_t* q_fwd, uint16_t* q_dgrad, void* stream) {
    PPOX_REQUIRE(w && (q_fwd || q_dgrad), "ppox_nature_fc_pack: bad arguments");
    return launch_pack_all(PackAll{nullptr, nullptr, nullptr, w, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   q_fwd, q_dgrad},
                           ppox::as_stream(stream), "ppox_nature_fc_pack");
}

extern "C" int ppox_nature_pack_all(const float* w1, const float* b1, const float* w2, const float* b2,
                                    const float* w3, const float* b3, const float* wfc, float* wpd2, uint16_t* q1,
                                    uint16_t* q2, uint16_t* q3, uint16_t* qd2, uint16_t* qd3, uint16_t* qfc_fwd,
                                    uint16_t* qfc_dgrad, const float* wh, uint16_t* qh_fwd, uint16_t* qh_dgrad,
                                    uint32_t* zero, int64_t zero_words, void* stream) {
    PPOX_REQUIRE(w1 && w2 && w3 && (wfc || (!qfc_fwd && !qfc_dgrad)), "ppox_nature_pack_all: null weights");
    PPOX_REQUIRE(!q1 || b1, "ppox_nature_pack_all: q1 needs the conv1 bias b1 (the H1P exponent)");
    PPOX_REQUIRE(zero_words >= 0 && (zero_words == 0 || zero), "ppox_nature_pack_all: zero buffer");
    PackAll p{w1, w2, w3, wfc, wpd2, q1, q2, q3, qd2, qd3, qfc_fwd, qfc_dgrad, wh, qh_fwd, qh_dgrad, b1, zero,
              zero_words};
    p.b2 = b2;
    p.b3 = b3;
    return launch_pack_all(p, ppox::as_stream(stream), "ppox_nature_pack_all");
}

extern "C" int ppox_nature_pack_all_wmax(const float* w1, const float* b1, const float* w2, const float* b2,
                                         const float* w3, const float* b3, const float* wfc, float* wpd2,
                                         uint16_t* q1, uint16_t* q2, uint16_t* q3, uint16_t* qd2, uint16_t* qd3,
                                         uint16_t* qfc_fwd, uint16_t* qfc_dgrad, const float* wh, uint16_t* qh_fwd,
                                         uint16_t* qh_dgrad, const uint32_t* amax_in, uint32_t* amax_next,
                                         uint32_t* zero, int64_t zero_words, void* stream) {
    static_assert(PPOX_WMAX_TENSORS == PA_TENSORS && PPOX_WMAX_SLOTS == AMAX_SLOTS, "ppox.h: the amax partials");
    PPOX_REQUIRE(w1 && w2 && w3 && (wfc || (!qfc_fwd && !qfc_dgrad)), "ppox_nature_pack_all_wmax: null weights");
    PPOX_REQUIRE(!q1 || b1, "ppox_nature_pack_all_wmax: q1 needs the conv1 bias b1 (the H1P exponent)");
    PPOX_REQUIRE(zero_words >= 0 && (zero_words == 0 || zero), "ppox_nature_pack_all_wmax: zero buffer");
    PackAll p{w1, w2, w3, wfc, wpd2, q1, q2, q3, qd2, qd3, qfc_fwd, qfc_dgrad, wh, qh_fwd, qh_dgrad, b1, zero,
              zero_words};
    p.b2 = b2;
    p.b3 = b3;
    p.amax_in = amax_in;
    p.amax_next = amax_next;
    return launch_pack_all(p, ppox::as_stream(stream), "ppox_nature_pack_all_wmax");
}

// ---- the heads' hidden layer Linear(512, 512) + ReLU on the split-f16 GEMM -------------
extern "C" int64_t ppox_head_hidden_pack_elems(void) { return PL_H + 2 * PACK_TAIL32; }

// ---- amax slots (split-f16 operand scales) -------------------------------------------
__global__ void __launch_bounds__(256) amax_kernel(const float4* __restrict__ x, long long n4,
                                                   uint32_t* __restrict__ am) {
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 v = x[i];
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
    amax_record(am, m);
}

extern "C" int32_t ppox_amax_slots(void) { return AMAX_SLOTS; }

extern "C" int ppox_amax(const float* x, int64_t n, uint32_t* amax, void* stream) {
    PPOX_REQUIRE(amax && n >= 0 && n % 4 == 0 && (x || n == 0), "ppox_amax: bad arguments (n % 4 == 0)");
    PPOX_REQUIRE(ppox::aligned16(amax) && (!x || ppox::aligned16(x)), "ppox_amax: 16B alignment");
    if (n == 0) return PPOX_OK;
    const long long blocks = std::min<long long>(ppox::ceil_div(n / 4, 256LL), 1024);
    amax_kernel<<<(unsigned)blocks, 256, 0, ppox::as_stream(stream)>>>(reinterpret_cast<const float4*>(x), n / 4, amax);
    PPOX_LAUNCHED("ppox_amax");
}

// ---- PX planes of an f32 tensor whose amax is recorded (round 4: the fc layer's df) ----------
// y = the two f16 planes of x 2^E (include/ppox.h "PX"), E from x's amax slots — the scale a split
// GEMM would take for x as an f32 operand, so the planes are the split every consumer tile made
// in registers before (the fc dgrad split each df value once per 64-column tile: 49 times).
// A thread splits 4 consecutive values of a 32-group: 16 B in, 8 B to each plane out.
__global__ void __launch_bounds__(256) px_split_kernel(const float4* __restrict__ x, long long n4,
                                                       const uint32_t* __restrict__ am, uint16_t* __restrict__ y,
                                                       int* __restrict__ e_out) {
    const int e = split_scale_exp(amax_read(am));
    const float sc = exp2i(e);
    if (blockIdx.x == 0 && threadIdx.x == 0) *e_out = e;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        uint2 h, l;
        split4h(x[i], sc, h, l);
        uint16_t* q = y + px_index(4 * i);
        *reinterpret_cast<uint2*>(q) = h;
        *reinterpret_cast<uint2*>(q + 32) = l;
    }
}

extern "C" int ppox_px_split(const float* x, int64_t n, const uint32_t* amax, uint16_t* y, int* exp_out,
                             void* stream) {
    PPOX_REQUIRE(amax && y && exp_out && n >= 0 && n % 32 == 0 && (x || n == 0),
                 "ppox_px_split: bad arguments (n % 32 == 0)");
    PPOX_REQUIRE(ppox::aligned16(amax) && ppox::aligned16(y) && (!x || ppox::aligned16(x)),
                 "ppox_px_split: 16B alignment");
    if (n == 0) return PPOX_OK;
    const long long blocks = std::min<long long>(ppox::ceil_div(n / 4, 256LL), 2048);
    px_split_kernel<<<(unsigned)blocks, 256, 0, ppox::as_stream(stream)>>>(reinterpret_cast<const float4*>(x), n / 4,
                                                                           amax, y, exp_out);
    PPOX_LAUNCHED("ppox_px_split");
}
