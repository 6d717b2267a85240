// What the NatureCNN GEMM units share across the cut between them (not part of the ABI):
//   * the Problems (tile of a block, chunk walk, packed-B chunk, fused epilogue) that both the f32 implicit GEMM
//     (conv_f32.hip: igemm_kernel, with its register stagers) and the split-f16 GEMM (conv.hip: sgemm_kernel, with
//     its LDS-DMA row pointers) are instantiated from;
//   * the split-packed B layout, written by pack.hip and read by the GEMMs of conv.hip (and of dconv.hip, which
//     spells the indices out): pack_frag_unit, the fc / head column-block geometry (GemmRowsProblem) and the
//     packed forms' sizes.
#pragma once
#include "conv_common.h"

namespace {

constexpr int BK = 32;  // K chunk of the GEMMs

// ---------------------------------------------------------------------------
// Problems: tile of a block, chunk count, packed-B chunk, epilogue.  A unit adds
// how it stages A: register stagers (conv_f32.hip: FwdNHWCProblem, DgradPMProblem),
// or row pointers for the LDS-DMA (conv.hip: SgFwd, SgDgradPM, SgRows).
// ---------------------------------------------------------------------------
struct RowTile {  // forward: a contiguous run of output pixels
    long long m0, M;
};

template <class L, bool OUT_NCHW, int MT_>
struct FwdBase {
    static constexpr int NOUT = L::COUT, MT = MT_, BMR = 128 * MT;
    static constexpr bool A_PLANES = false;  // sg2: A rows are f32 (split in registers), not H1P planes
    static constexpr bool PLANES_OUT = false;  // sg2: the output as PX planes (Px<>, conv.hip)
    using Tile = RowTile;
    __device__ static bool tile(const Args& a, Tile& t) {
        t.m0 = (long long)blockIdx.x * BMR;
        t.M = a.batch * L::P;
        return true;
    }
    __device__ static int nchunk(const Tile&) { return L::K / BK; }
    __device__ static const float* bchunk(const Args& a, const Tile&, int c) { return a.wp + (long long)c * BK * NOUT; }
    __device__ static int bchunk_id(const Tile&, int c) { return c; }  // 32-row block of the packed [K][NOUT]
    __device__ static float prefetch(const Args& a, const Tile&, int, int co) { return a.bias[co]; }
    // stores one output element; returns it (0 for rows past the end: the amax of the output)
    __device__ static float store_pre(const Args& a, const Tile& t, int row, int co, float acc, float bias) {
        const long long m = t.m0 + row;
        if (m >= t.M) return 0.f;
        const float v = fmaxf(acc + bias, 0.f);
        if constexpr (OUT_NCHW) {
            const long long n = m / L::P;
            a.y[(n * L::COUT + co) * L::P + (m - n * L::P)] = v;
        } else {
            a.y[m * L::COUT + co] = v;
        }
        return v;
    }
    // PX epilogue (NHWC output): the value (0 past the end) and its f32-layout element index (-1: none)
    __device__ static float value(const Args&, const Tile& t, int row, int, float acc, float bias) {
        return t.m0 + row < t.M ? fmaxf(acc + bias, 0.f) : 0.f;
    }
    __device__ static long long out_elem(const Args&, const Tile& t, int row, int co) {
        const long long m = t.m0 + row;
        return m < t.M ? m * L::COUT + co : -1;
    }
};

// dgrad (transposed conv) of layer L, position-major: a block owns ONE input
// pixel (iy, ix) of 128*MT consecutive samples, so every row of the tile has the
// same contributing taps — exactly those (ky, kx) with iy = S*oy + ky inside the
// output grid.  The K walk covers only those taps (no zero MACs: conv3 borders
// have 4-6 of 9, every conv2 pixel 1-4 of 16).  K order (tap, co); chunk = 32
// output channels of one tap, gathered from the NHWC output grad G at the same
// (oy, ox) for every row.  Epilogue: x (previous activation > 0), NHWC.
// Blocks -> (sample tile, pixel) XCD-aware: one XCD walks the pixels of one
// sample tile, whose G rows then stay in that XCD's L2.
struct PixelTile {
    long long n0;
    int pos, iy, ix, ky0, kx0, nx, nchunk;
};

template <class L, int MT_>
struct DgradPMBase {
    static constexpr int NOUT = L::CIN, MT = MT_, BMR = 128 * MT, NPOS = L::IH * L::IW, CPT = L::COUT / BK;
    static constexpr bool A_PLANES = false;
    static constexpr bool PLANES_OUT = false;
    using Tile = PixelTile;
    __device__ static bool tile(const Args& a, Tile& t) {
        const long long w = xcd_remap(blockIdx.x, gridDim.x);
        t.n0 = (w / NPOS) * BMR;
        t.pos = (int)(w % NPOS);
        t.iy = t.pos / L::IW;
        t.ix = t.pos % L::IW;
        int ny, nx;
        tap_range<L::S, L::OH, L::KH>(t.iy, t.ky0, ny);
        tap_range<L::S, L::OW, L::KW>(t.ix, t.kx0, nx);
        t.nx = nx;
        t.nchunk = ny * nx * CPT;
        return true;
    }
    __device__ static int nchunk(const Tile& t) { return t.nchunk; }
    __device__ static const float* bchunk(const Args& a, const Tile& t, int c) {
        const int tap = c / CPT, ty = tap / t.nx, tx = tap - ty * t.nx;
        const int ky = t.ky0 + L::S * ty, kx = t.kx0 + L::S * tx;
        return a.wp + ((long long)(ky * L::KW + kx) * L::COUT + (c % CPT) * BK) * L::CIN;
    }
    __device__ static int bchunk_id(const Tile& t, int c) {
        const int tap = c / CPT, ty = tap / t.nx, tx = tap - ty * t.nx;
        return ((t.ky0 + L::S * ty) * L::KW + t.kx0 + L::S * tx) * CPT + c % CPT;
    }
    // the epilogue's ReLU-mask values are loaded before the K walk (their latency
    // hides under it) — 16 per lane per column tile, in the C/D layout
    __device__ static float prefetch(const Args& a, const Tile& t, int row, int ci) {
        long long n = t.n0 + row;
        n = n < a.batch ? n : t.n0;
        return a.mask[(n * NPOS + t.pos) * L::CIN + ci];
    }
    __device__ static float store_pre(const Args& a, const Tile& t, int row, int ci, float acc, float m) {
        const long long n = t.n0 + row;
        if (n >= a.batch) return 0.f;
        const float v = m > 0.f ? acc : 0.f;
        a.y[(n * NPOS + t.pos) * L::CIN + ci] = v;
        return v;
    }
    __device__ static float value(const Args& a, const Tile& t, int row, int, float acc, float m) {
        return t.n0 + row < a.batch && m > 0.f ? acc : 0.f;
    }
    __device__ static long long out_elem(const Args& a, const Tile& t, int row, int ci) {
        const long long n = t.n0 + row;
        return n < a.batch ? (n * NPOS + t.pos) * L::CIN + ci : -1;
    }
};

// ---------------------------------------------------------------------------
// Pre-split B operands of the split-f16 GEMMs (sgemm_kernel, the wgrad-free kernels): a
// [K][NOUT] matrix times 2^E as two fp16 planes in MFMA fragment order, followed by the
// buffer's tail (pack_tail): the weight tensor's amax partials and the exponent E.
// ---------------------------------------------------------------------------
// packed position of natural element (row k, col) of a [K][nout] matrix, plane p:
// chunk (k / 32) x k-step s x column tile j x plane x lane (h, col & 31) x e
__host__ __device__ constexpr long long split_frag_index(int k, int col, int nout, int p) {
    const int ch = k >> 5, kl = k & 31, s = kl >> 4, h = (kl >> 3) & 1, e = kl & 7;
    const int nt = nout / 32, j = col >> 5, l = h * 32 + (col & 31);
    return ((((long long)(ch * 2 + s) * nt + j) * NPL + p) * 64 + l) * 8 + e;
}

// Output-major split packing: unit u = one 16-B fragment run (8 consecutive k of one
// column, both planes) of the split_frag_index layout of a [K][NOUT] matrix — its
// eight source values are gathered (coalesced across lanes: adjacent units are adjacent
// columns), scaled by s and written as two 16-B stores, instead of 2-B stores scattered.
template <int NOUT, class Src>
__device__ inline void pack_frag_unit(const Src& src, float s, uint16_t* __restrict__ q, long long u) {
    constexpr int NT = NOUT / 32;
    const int l = (int)(u & 63);
    const long long r = u >> 6;
    const int j = (int)(r % NT);
    const long long cs = r / NT;  // 32-row chunk * 2 + 16-row step
    const int col = j * 32 + (l & 31), k0 = (int)(cs * 16) + (l >> 5) * 8;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = src(k0 + e, col);
    u32x4 p0, p1;
    split8h(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), s, p0, p1);
    u32x4* d = reinterpret_cast<u32x4*>(q + ((cs * NT + j) * NPL) * 512) + l;
    d[0] = p0;
    d[64] = p1;
}

// ---------------------------------------------------------------------------
// NatureCNN hidden linear layer Linear(3136, 512) (.ipynb_checkpoints/
// models-checkpoint.py:58-59) on the split-f16 implicit-GEMM kernel: a plain GEMM
// C[M][N] = A[M][K] B[K][N] with A f32 rows (split in registers), B pre-split per
// column block of NB (zero-padded), workgroups over (row tile, column block), the
// column blocks of a row tile on one XCD (its A rows then come from that XCD's L2).
//   FC_FWD:   A = h3 (M x 3136, Flatten order), B = W^T; epilogue relu(acc + bias)
//   FC_DGRAD: A = dL/df * relu'(f) (M x 512), B = W; epilogue: the element (m, c*49 + p)
//             goes to g3[m][p][c] (NHWC) times (h3 > 0) — the trunk's ReLU backward and
//             NCHW -> NHWC transpose fused (replaces the dh3 round trip + nchw_to_nhwc_mask)
// ---------------------------------------------------------------------------
//   HEAD_DGRAD: the 512-wide hidden head layer's input grad, accumulated and masked in place:
//             y (= df) <- (f > 0) ? y + acc : 0  (the grads of the heads before it already in y)
enum { FC_FWD = 0, FC_DGRAD = 1, HEAD_DGRAD = 2 };
// The split fc kernels run in NHWC feature order: feature f = p * 64 + c of the conv3 output
// (the layout conv3's split forward writes, 128-B channel runs) is the reference's Flatten
// feature c * 49 + p of Linear(3136, 512) — the weights are packed through this permutation,
// so the forward reads h3 rows and the dgrad writes g3 rows as they lie, no transposes.
__host__ __device__ constexpr int fc_nchw_feature(int f) { return (f & 63) * 49 + (f >> 6); }
struct GemmTile {
    long long m0, M;
    int cb;
};

template <int K_, int N_, int NB, int MODE>
struct GemmRowsProblem {
    static constexpr int K = K_, N = N_, NOUT = NB, MT = 1, BMR = 128, NCB = (N + NB - 1) / NB, KC = K / BK;
    static constexpr bool LATE_EPILOGUE = true;
    static constexpr bool A_PLANES = false;
    static constexpr bool PLANES_OUT = false;
    static_assert(K % BK == 0, "K multiple of 32");
    using Tile = GemmTile;
    __device__ static bool tile(const Args& a, Tile& t) {
        const long long w = xcd_remap(blockIdx.x, gridDim.x);
        t.cb = (int)(w % NCB);
        t.m0 = (w / NCB) * BMR;
        t.M = a.batch;
        return true;
    }
    __device__ static int nchunk(const Tile&) { return KC; }
    __device__ static int bchunk_id(const Tile& t, int c) { return t.cb * KC + c; }
    // B is packed in 64-column blocks; a 128-column tile (NB = 128) reads blocks 2 cb and 2 cb + 1
    // (past the last block: the last again, its columns never stored)
    static constexpr int NCB64 = (N + 63) / 64;
    __device__ static int bchunk_blk(const Tile& t, int c, int b) {
        const int blk = t.cb * (NB / 64) + b;
        return (blk < NCB64 ? blk : NCB64 - 1) * KC + c;
    }
    // branch-free (clamped indices), so an epilogue can issue all its loads before any wait
    // (HEAD_DGRAD: the mask and the accumulated grad)
    __device__ static auto prefetch(const Args& a, const Tile& t, int row, int col) {
        const int n = t.cb * NB + col, nc = n < N ? n : N - 1;
        long long m = t.m0 + row;
        m = m < t.M ? m : t.m0;
        if constexpr (MODE == FC_FWD)
            return a.bias[nc];
        else if constexpr (MODE == FC_DGRAD)
            return a.mask[m * N + nc];
        else
            return make_float2(a.mask[m * N + nc], a.y[m * N + nc]);
    }
    template <class Pre>
    __device__ static float store_pre(const Args& a, const Tile& t, int row, int col, float acc, Pre e) {
        const long long m = t.m0 + row;
        const int n = t.cb * NB + col;
        if (m >= t.M || n >= N) return 0.f;
        // FC_FWD: relu(acc + bias); FC_DGRAD: g3 (NHWC) times the ReLU mask of h3 (NHWC), the same
        // index; HEAD_DGRAD: (accumulated grad + acc) times the ReLU mask of f
        float v;
        if constexpr (MODE == FC_FWD)
            v = fmaxf(acc + e, 0.f);
        else if constexpr (MODE == FC_DGRAD)
            v = e > 0.f ? acc : 0.f;
        else
            v = e.x > 0.f ? e.y + acc : 0.f;
        a.y[m * N + n] = v;
        return v;
    }
    // PX epilogue: the fc dgrad's masked g3 (FC_DGRAD only)
    __device__ static float value(const Args&, const Tile& t, int row, int col, float acc, float e) {
        static_assert(MODE == FC_DGRAD, "PX output: the fc dgrad");
        return t.m0 + row < t.M && t.cb * NB + col < N && e > 0.f ? acc : 0.f;
    }
    __device__ static long long out_elem(const Args&, const Tile& t, int row, int col) {
        const long long m = t.m0 + row;
        const int n = t.cb * NB + col;
        return m < t.M && n < N ? m * N + n : -1;
    }
};

constexpr int FC_NB = 64;  // the packed fc / head B blocks (64 columns)
using FcFwd = GemmRowsProblem<3136, 512, FC_NB, FC_FWD>;
using FcDgrad = GemmRowsProblem<512, 3136, FC_NB, FC_DGRAD>;
// the heads' hidden layer Linear(512, 512) + ReLU (models-checkpoint.py:62-66 extra_layer)
using HeadFwd = GemmRowsProblem<512, 512, FC_NB, FC_FWD>;
using HeadDgrad = GemmRowsProblem<512, 512, FC_NB, HEAD_DGRAD>;
static_assert(FC_NB == 64, "sg2 runs the fc layer in 64-column blocks");

// elements of the split-packed matrices (the fc and head forms in zero-padded 64-column blocks)
constexpr long long PA_N2 = (long long)G2::K * G2::COUT, PA_N3 = (long long)G3::K * G3::COUT;
constexpr long long PA_NFC = (long long)FcFwd::NCB * FcFwd::K * FcFwd::NOUT;
constexpr long long PA_NFCD = (long long)FcDgrad::NCB * FcDgrad::K * FcDgrad::NOUT;
constexpr long long PA_NH = (long long)HeadFwd::NCB * HeadFwd::K * HeadFwd::NOUT;
// planes (uint16) of each packed form; a buffer is planes + 2 * PACK_TAIL32 uint16
constexpr long long PL_Q1 = FWD1_PACK, PL_Q2 = NPL * PA_N2, PL_Q3 = NPL * PA_N3, PL_FCF = NPL * PA_NFC,
                    PL_FCD = NPL * PA_NFCD, PL_H = NPL * PA_NH;
static_assert(PL_FCF == PL_FCD, "fc forms: one size");

}  // namespace
