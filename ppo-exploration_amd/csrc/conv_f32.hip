// K6 — NatureCNN convolutions as implicit GEMMs on the fp32 matrix cores
// (v_mfma_f32_32x32x2_f32: exact f32 FMAs at the gfx950 fp32 matrix rate,
// 157 TF/s dense).  Replaces torch.nn.Conv2d + ReLU (forward) and their
// autograd (backward) of .ipynb_checkpoints/models-checkpoint.py:52-58:
//   conv1 4->32 k8 s4 (84x84 -> 20x20), conv2 32->64 k4 s2 (-> 9x9),
//   conv3 64->64 k3 s1 (-> 7x7).
//
// Activation layout: NHWC between layers (a 32-channel run = one 128-byte row
// segment, so every im2col gather is coalesced); the trunk output is NCHW (the
// reference's Flatten order feeding Linear(3136, 512)).  conv1 reads the uint8
// frame stack (N, 4, 84, 84) directly: the torch.FloatTensor(obs) conversion is
// fused (u8 -> f32 is exact), and so is the minibatch gather (rows via idx).
//
// Forward / dgrad: M = output rows, N = channels, K = taps x channels.  One
// 256-thread workgroup owns BM = 128 rows x all N channels; each wave 32 rows
// (N/32 MFMA tiles).  K is walked in BK = 32 chunks, register-staged and
// double-buffered in LDS (one barrier per chunk) so the gathers of chunk c+1 fly
// under the MFMAs of chunk c.  Each thread's four staged rows are fixed for the
// whole K walk, so their base addresses are computed once.
//   forward epilogue: + bias, ReLU
//   dgrad epilogue:   x (previous activation > 0) — the previous layer's ReLU
//                     backward is fused, the result is that layer's output grad
//   conv2 dgrad (stride 2) runs as 4 parity classes of the input grid, each a
//   dense GEMM over its 2x2 contributing taps (no zero MACs).
// Wgrad: dW[k][co] = sum_m A[m][k] G[m][co] — a GEMM whose reduction runs over
// all output pixels.  Workgroups own a K-block and a slice of M (split-K over
// pixels), write partial slabs, and a reduce kernel sums the slabs in a FIXED
// order (deterministic) straight into the PyTorch [co][ci][ky][kx] layout; the
// bias gradient is fused into the k-block-0 workgroups.  The k-blocks of one
// M-slice are mapped to one XCD (blockIdx % 8) so their shared G rows and
// overlapping input patches are served from that XCD's L2.
// The slab reduce (wgrad_reduce) is shared with the split weight gradients and lives in
// wgrad.hip, behind ppox_conv::wgrad_reduce; the f32 weight packings (ppox_nature_pack_weights)
// are in pack.hip with the other packers.  This unit is the PPOX_CONV_MATH=f32 path; the
// split-f16 forms are in conv.hip, conv_split.hip, dconv.hip, wgrad.hip and pack.hip.
#include "gemm_layout.h"

namespace {

constexpr int AST = BK + 1;  // padded LDS row stride (floats): conflict-free column reads

// ---------------------------------------------------------------------------
// A stagers: global -> registers (load) -> LDS (store), 4*MT slots per thread.
// Slot i of thread t covers element w = i*256 + t of the (128*MT) x BK chunk.
// Rows past the end read a valid clamped address and are zeroed by a select: a
// conditional load would make hipcc branch around every load (execz) and
// serialise them.
// ---------------------------------------------------------------------------
// f32 rows of 32 floats (8 float4 per row) -> LDS
template <int SL>
__device__ inline void store_rows_f4(float* As, const float4 (&r)[SL]) {
#pragma unroll
    for (int i = 0; i < SL; ++i) {
        const int w = i * 256 + threadIdx.x;
        float* d = As + (w >> 3) * AST + (w & 7) * 4;
        d[0] = r[i].x;
        d[1] = r[i].y;
        d[2] = r[i].z;
        d[3] = r[i].w;
    }
}

// NHWC f32 forward (conv2, conv3): K order (ky, kx, ci); chunk = 32 channels of one tap.
template <class L, int MT>
struct StageFwdNHWC {
    static constexpr int SL = 4 * MT;
    const float* base[SL];
    bool ok[SL];
    float4 r[SL];
    __device__ StageFwdNHWC(const Args& a, const RowTile& t) {
        const float* x = reinterpret_cast<const float*>(a.x);
#pragma unroll
        for (int i = 0; i < SL; ++i) {
            const int w = i * 256 + threadIdx.x;
            const int row = w >> 3, q = w & 7;
            const long long m = t.m0 + row;
            ok[i] = m < t.M;
            const long long mm = ok[i] ? m : t.m0;
            const long long n = mm / L::P;
            const int p = (int)(mm - n * L::P), oy = p / L::OW, ox = p % L::OW;
            base[i] = x + ((n * L::IH + oy * L::S) * L::IW + ox * L::S) * L::CIN + q * 4;
        }
    }
    __device__ inline void load(int chunk) { load_to(chunk, r); }
    __device__ inline void load_to(int chunk, float4 (&r)[SL]) const {
        constexpr int CPT = L::CIN / BK;
        const int tap = chunk / CPT, ky = tap / L::KW, kx = tap % L::KW;
        const int off = (ky * L::IW + kx) * L::CIN + (chunk % CPT) * BK;
        // rows past the end read a clamped valid row; their C rows are never stored
#pragma unroll
        for (int i = 0; i < SL; ++i) r[i] = *reinterpret_cast<const float4*>(base[i] + off);
    }
    __device__ inline void store(float* As) const { store_rows_f4<SL>(As, r); }
};

template <int NOUT>
struct StageB {
    static constexpr int V = BK * NOUT / 4 / 256;  // float4 per thread
    float4 r[V];
    __device__ inline void load(const float* chunk_base) {
        const float4* src = reinterpret_cast<const float4*>(chunk_base);
#pragma unroll
        for (int i = 0; i < V; ++i) r[i] = src[i * 256 + threadIdx.x];
    }
    __device__ inline void store(float* Bs) const {
#pragma unroll
        for (int i = 0; i < V; ++i) reinterpret_cast<float4*>(Bs)[i * 256 + threadIdx.x] = r[i];
    }
};

template <class L, bool OUT_NCHW, int MT>
struct FwdNHWCProblem : FwdBase<L, OUT_NCHW, MT> {
    using Stager = StageFwdNHWC<L, MT>;
};

template <class L, int MT>
struct StageDgradPM {
    static constexpr int SL = 4 * MT, CPT = L::COUT / BK;
    const float* base[SL];
    bool ok[SL];
    float4 r[SL];
    int iy, ix, ky0, kx0, nx;
    __device__ StageDgradPM(const Args& a, const PixelTile& t)
        : iy(t.iy), ix(t.ix), ky0(t.ky0), kx0(t.kx0), nx(t.nx) {
        const float* g = reinterpret_cast<const float*>(a.x);
#pragma unroll
        for (int i = 0; i < SL; ++i) {
            const int w = i * 256 + threadIdx.x;
            const long long n = t.n0 + (w >> 3);
            ok[i] = n < a.batch;
            base[i] = g + (ok[i] ? n : t.n0) * (L::P * L::COUT) + (w & 7) * 4;
        }
    }
    __device__ inline void load(int chunk) { load_to(chunk, r); }
    __device__ inline void load_to(int chunk, float4 (&r)[SL]) const {
        const int tap = chunk / CPT, ty = tap / nx, tx = tap - ty * nx;
        const int oy = (iy - ky0) / L::S - ty, ox = (ix - kx0) / L::S - tx;
        const int off = (oy * L::OW + ox) * L::COUT + (chunk % CPT) * BK;
        // rows past the end read a clamped valid row; their C rows are never stored
#pragma unroll
        for (int i = 0; i < SL; ++i) r[i] = *reinterpret_cast<const float4*>(base[i] + off);
    }
    __device__ inline void store(float* As) const { store_rows_f4<SL>(As, r); }
};

template <class L, int MT>
struct DgradPMProblem : DgradPMBase<L, MT> {
    using Stager = StageDgradPM<L, MT>;
};

// One 256-thread workgroup: 128*MT rows x NOUT columns; each wave 32*MT rows
// (MT x NT MFMA tiles).  K walked in BK = 32 chunks, register-staged and
// double-buffered in LDS, one barrier per chunk.
template <class Prob>
__global__ void __launch_bounds__(256, 2) igemm_kernel(Args a) {
    constexpr int NOUT = Prob::NOUT, NT = NOUT / 32, MT = Prob::MT, BMR = 128 * MT;
    __shared__ float As[2][BMR * AST];
    __shared__ __attribute__((aligned(16))) float Bs[2][BK * NOUT];
    typename Prob::Tile t;
    if (!Prob::tile(a, t)) return;
    const int nchunk = Prob::nchunk(t);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = zero16();
    // epilogue operands (bias / ReLU mask) in the C/D layout, loaded up front
    f32x16 pre[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                pre[i][j][r] = Prob::prefetch(a, t, wave * 32 * MT + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5),
                                              j * 32 + (lane & 31));

    typename Prob::Stager sa(a, t);
    StageB<NOUT> sb;
    if (nchunk > 0) {
        sa.load(0);
        sb.load(Prob::bchunk(a, t, 0));
        sa.store(As[0]);
        sb.store(Bs[0]);
    }
    __syncthreads();

    const int arow = wave * 32 * MT + (lane & 31);
    const int khalf = lane >> 5;
    for (int c = 0; c < nchunk; ++c) {
        const int cur = c & 1;
        if (c + 1 < nchunk) {
            sa.load(c + 1);
            sb.load(Prob::bchunk(a, t, c + 1));
        }
        const float* A = As[cur] + arow * AST + khalf;
        const float* B = Bs[cur] + khalf * NOUT + (lane & 31);
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            float av[MT];
#pragma unroll
            for (int i = 0; i < MT; ++i) av[i] = A[i * 32 * AST + kk * 2];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const float bv = B[kk * 2 * NOUT + j * 32];
#pragma unroll
                for (int i = 0; i < MT; ++i)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv, acc[i][j], 0, 0, 0);
            }
        }
        if (c + 1 < nchunk) {
            sa.store(As[cur ^ 1]);
            sb.store(Bs[cur ^ 1]);
        }
        __syncthreads();
    }
    // C/D map: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int col = j * 32 + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r)
                Prob::store_pre(a, t, wave * 32 * MT + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), col,
                                acc[i][j][r], pre[i][j][r]);
        }
}

// ---------------------------------------------------------------------------
// Register-direct implicit GEMM (the default forward / dgrad path).
// Each wave owns 32*MT rows x all NOUT columns and is independent: no LDS, no
// barriers.  Within a 32-wide K chunk the MFMA k-slice of step kk is
// {kk, 16 + kk}: lane half h = lane >> 5 supplies k = 16h + kk, so every lane
// reads its row's 16 contiguous K values (4 x 16 B) straight into VGPRs.  B is
// packed so that load q of column tile j is one contiguous 1 KB run across the
// wave (lane L takes floats 4L..4L+3: k = 16h + 4q..4q+3 of column l32) —
// fully coalesced (pack.hip rg_index).  Chunk c+1 is loaded while chunk c runs on the
// matrix cores.  Used for conv1 forward (u8 input); the f32 layers keep the
// LDS-staged igemm: their 32-row x 32-B fragment loads cost more TA cycles than
// the LDS round trip (measured: profiles/README.md).
// Rows past the end load a clamped (valid) address; their C rows are never
// stored, and a GEMM row only ever reaches its own C row.
// ---------------------------------------------------------------------------
using f32x4 = __attribute__((ext_vector_type(4))) float;

// conv1: u8 NCHW frames; chunk c = channel c/2, kernel rows 4(c&1)..+3; lane
// half h takes kernel rows 4(c&1)+2h, +1: two 8-byte runs = four words
template <int MT_>
struct RgFwd1 {
    using L = G1;
    static constexpr int NOUT = L::COUT, MT = MT_, ROWS = 128 * MT;
    using Raw = uint32_t[MT][4];
    struct Tile {
        unsigned m0, M;  // this wave's first row, total rows (< 2^31, host-checked)
    };
    __device__ static bool tile(const Args& a, Tile& t, int wave) {
        const long long w = xcd_remap(blockIdx.x, gridDim.x);
        t.M = (unsigned)(a.batch * L::P);
        t.m0 = (unsigned)(w * ROWS) + wave * 32 * MT;
        return t.m0 < t.M;
    }
    __device__ static int nchunk(const Tile&) { return L::K / BK; }
    __device__ static const float* bchunk(const Args& a, const Tile&, int c) { return a.wp + c * BK * NOUT; }
    struct Loader {
        const uint8_t* base[MT];
        __device__ Loader(const Args& a, const Tile& t, int lane) {
            const uint8_t* x = reinterpret_cast<const uint8_t*>(a.x);
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                unsigned m = t.m0 + i * 32 + (lane & 31);
                m = m < t.M ? m : t.m0;
                const unsigned n = m / L::P, p = m - n * L::P, oy = p / L::OW, ox = p % L::OW;
                base[i] = x + u8_sample_base(a, n, (long long)L::CIN * L::IH * L::IW) +
                          (oy * L::S + (lane >> 5) * 2) * L::IW + ox * L::S;
            }
        }
        __device__ inline void load(int c, Raw& r) const {
            const int off = (c >> 1) * (L::IH * L::IW) + (c & 1) * 4 * L::IW;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const uint8_t* p = base[i] + off;
                r[i][0] = *reinterpret_cast<const uint32_t*>(p);
                r[i][1] = *reinterpret_cast<const uint32_t*>(p + 4);
                r[i][2] = *reinterpret_cast<const uint32_t*>(p + L::IW);
                r[i][3] = *reinterpret_cast<const uint32_t*>(p + L::IW + 4);
            }
        }
        __device__ static inline float elem(const Raw& r, int i, int kk) {
            return (float)((r[i][kk >> 2] >> (8 * (kk & 3))) & 0xFFu);
        }
    };
    __device__ static void store(const Args& a, const Tile& t, int row, int co, float acc, bool) {
        const unsigned m = t.m0 + row;
        if (m >= t.M) return;
        a.y[(long long)m * L::COUT + co] = fmaxf(acc + a.bias[co], 0.f);
    }
};

template <class Prob, bool OUT_NCHW = false>
__global__ void __launch_bounds__(256, 2) rgemm_kernel(Args a) {
    constexpr int NOUT = Prob::NOUT, NT = NOUT / 32, MT = Prob::MT;
    using Ld = typename Prob::Loader;
    using Raw = typename Prob::Raw;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    typename Prob::Tile t;
    if (!Prob::tile(a, t, wave)) return;  // wave-uniform; nothing below synchronises
    const int n = Prob::nchunk(t);
    const Ld ld(a, t, lane);

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = zero16();

    Raw a0, a1;
    f32x4 b0[NT][4], b1[NT][4];
    auto loadB = [&](int c, f32x4 (&b)[NT][4]) {
        const f32x4* p = reinterpret_cast<const f32x4*>(Prob::bchunk(a, t, c)) + lane;
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) b[j][q] = p[j * 256 + q * 64];
    };
    auto compute = [&](const Raw& ar, const f32x4 (&b)[NT][4]) {
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int i = 0; i < MT; ++i)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ld::elem(ar, i, kk), b[j][kk >> 2][kk & 3],
                                                                     acc[i][j], 0, 0, 0);
    };
    if (n > 0) {
        ld.load(0, a0);
        loadB(0, b0);
    }
    for (int c = 0; c < n; c += 2) {
        if (c + 1 < n) {
            ld.load(c + 1, a1);
            loadB(c + 1, b1);
        }
        compute(a0, b0);
        if (c + 2 < n) {
            ld.load(c + 2, a0);
            loadB(c + 2, b0);
        }
        if (c + 1 < n) compute(a1, b1);
    }
    // C/D map: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                Prob::store(a, t, i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), j * 32 + (lane & 31),
                            acc[i][j][r], OUT_NCHW);
}

// ---------------------------------------------------------------------------
// Wgrad.  WG = (k-block of KT rows of K) x (all COUT) x (slice of output pixels).
// Per step of MS = 32 pixels: stage X[32][KT] (im2col) and G[32][COUT] in LDS,
// then D(k x co) += X^T G on the MFMA (A operand = X^T: lane i <-> k, kk <-> pixel).
// Each thread's X unit (4 consecutive k) is fixed for the whole kernel, so its
// within-sample offset is computed once; its pixels advance by MS per step with
// 32-bit (sample, pixel) counters (MS <= P, so at most one wrap) — no divisions
// of 64-bit indices in the loop.
// ---------------------------------------------------------------------------

template <class L, bool U8>
struct WgCfg {
    static constexpr int KT = (L::COUT == 32) ? 128 : 64;  // 4 tiles of 32x32 per WG
    static constexpr int KB = L::K / KT;
    // row strides: +4 floats keeps the 16-B stores aligned and conflict-free (a half-wave's
    // 32 lanes write 512 contiguous bytes) and puts the two MFMA k-halves 4 banks apart
    static constexpr int XST = KT + 4, GST = L::COUT + 4;
    static constexpr int UPR = KT / 4;         // 4-element X units per pixel
    static constexpr int XV = MS * UPR / 256;  // X units per thread per step
    static constexpr int XPS = 256 / UPR;      // pixel stride between a thread's X units
    static constexpr int GUPR = L::COUT / 4;
    static constexpr int GV = MS * GUPR / 256;
    static constexpr int GPS = 256 / GUPR;
    static_assert(MS <= L::P, "one wrap per step");
};


template <class L, bool U8>
__global__ void __launch_bounds__(256, 2) wgrad_kernel(WArgs a) {
    using C = WgCfg<L, U8>;
    constexpr int KT = C::KT, KB = C::KB, XST = C::XST, GST = C::GST, COUT = L::COUT;
    constexpr int XV = C::XV, GV = C::GV, UPR = C::UPR, GUPR = C::GUPR;
    __shared__ __attribute__((aligned(16))) float Xs[2][MS * XST];
    __shared__ __attribute__((aligned(16))) float Gs[2][MS * GST];
    // XCD-aware block -> (split, kb): the KB k-blocks of a split share blockIdx % 8
    const int b = blockIdx.x, xcd = b & 7, q = b >> 3;
    const int kb = q % KB, split = (q / KB) * 8 + xcd;
    const unsigned M = (unsigned)(a.batch * L::P);
    const unsigned long long mb64 = (unsigned long long)split * (unsigned long long)a.px_per_split;
    const unsigned mbeg = mb64 < M ? (unsigned)mb64 : M;
    const unsigned mend = (unsigned)min((unsigned long long)M, (unsigned long long)mbeg + a.px_per_split);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kt = (COUT == 32) ? wave : (wave >> 1), ct = (COUT == 32) ? 0 : (wave & 1);
    f32x16 acc = zero16();

    // ---- fixed per-thread X unit ----
    const int u = threadIdx.x % UPR, px0 = threadIdx.x / UPR;
    const int k = kb * KT + u * 4;
    unsigned koff;
    if constexpr (U8) {
        koff = ((k >> 6) * L::IH + ((k >> 3) & 7)) * L::IW + (k & 7);  // (ci, ky, kx) in a NCHW frame stack
    } else {
        const int tap = k / L::CIN;
        koff = ((tap / L::KW) * L::IW + (tap % L::KW)) * L::CIN + (k % L::CIN);  // (ky, kx, ci) NHWC
    }
    // per X slot: its sample's base (bytes for u8, elements for f32) and its pixel in
    // that sample; both advance by MS pixels per step (at most one wrap: MS <= P)
    constexpr unsigned long long SAMPLE_F32 = (unsigned long long)L::IH * L::IW * L::CIN;
    const unsigned long long sstride = U8 ? (unsigned long long)a.sample_stride : SAMPLE_F32;
    unsigned long long sb[XV];
    unsigned xp[XV];
#pragma unroll
    for (int i = 0; i < XV; ++i) {
        const unsigned m = mbeg + px0 + i * C::XPS;
        const unsigned n = m / L::P;
        xp[i] = m - n * L::P;
        sb[i] = n * sstride;
    }
    const unsigned xn0 = mbeg / L::P, xp0 = mbeg - xn0 * L::P;  // a pixel that always exists
    const unsigned long long sb0 = xn0 * sstride;
    const int c4 = threadIdx.x % GUPR, gpx0 = threadIdx.x / GUPR;
    const uint8_t* xu8 = reinterpret_cast<const uint8_t*>(a.x);
    const float* xf = reinterpret_cast<const float*>(a.x);

    float4 xr[XV];
    uint32_t xw[XV];
    float4 gr[GV];
    float bsum0 = 0.f, bsum1 = 0.f, bsum2 = 0.f, bsum3 = 0.f;

    // FULL: every pixel of the step is inside the slice (all steps but possibly the
    // last of the last slice — splits are whole steps long); otherwise pixels past
    // the end read the slice's first pixel and are zeroed by a select
    auto load = [&](unsigned ms, auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
#pragma unroll
        for (int i = 0; i < XV; ++i) {
            bool ok = true;
            unsigned long long sbi = sb[i];
            unsigned pp = xp[i];
            if constexpr (!FULL) {
                ok = ms + px0 + i * C::XPS < mend;
                sbi = ok ? sbi : sb0;
                pp = ok ? pp : xp0;
            }
            const unsigned oy = pp / L::OW, ox = pp - oy * L::OW;
            if constexpr (U8) {
                const uint32_t v =
                    *reinterpret_cast<const uint32_t*>(xu8 + sbi + (oy * L::S * L::IW + ox * L::S + koff));
                xw[i] = ok ? v : 0u;
            } else {
                const float4 v = *reinterpret_cast<const float4*>(
                    xf + sbi + ((oy * L::S) * L::IW + ox * L::S) * L::CIN + koff);
                xr[i] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            xp[i] += MS;  // advance to the next step's pixel
            if (xp[i] >= (unsigned)L::P) {
                xp[i] -= L::P;
                sb[i] += sstride;
            }
        }
#pragma unroll
        for (int j = 0; j < GV; ++j) {
            const unsigned m = ms + gpx0 + j * C::GPS;
            bool ok = true;
            if constexpr (!FULL) ok = m < mend;
            const float4 v = *reinterpret_cast<const float4*>(a.g + (ok ? m : mbeg) * COUT + c4 * 4);
            gr[j] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto load_step = [&](unsigned ms) {
        if (ms + MS <= mend)
            load(ms, std::true_type{});
        else
            load(ms, std::false_type{});
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < XV; ++i) {
            float4* d = reinterpret_cast<float4*>(Xs[buf] + (px0 + i * C::XPS) * XST + u * 4);
            if constexpr (U8) {
                *d = make_float4((float)(xw[i] & 0xFFu), (float)((xw[i] >> 8) & 0xFFu), (float)((xw[i] >> 16) & 0xFFu),
                                 (float)(xw[i] >> 24));
            } else {
                *d = xr[i];
            }
        }
#pragma unroll
        for (int j = 0; j < GV; ++j) {
            *reinterpret_cast<float4*>(Gs[buf] + (gpx0 + j * C::GPS) * GST + c4 * 4) = gr[j];
            bsum0 += gr[j].x;
            bsum1 += gr[j].y;
            bsum2 += gr[j].z;
            bsum3 += gr[j].w;
        }
    };

    const unsigned nsteps = mend > mbeg ? (mend - mbeg + MS - 1) / MS : 0;
    if (nsteps > 0) {
        load_step(mbeg);
        store(0);
    }
    __syncthreads();
    const float* Xbase = &Xs[0][0] + (lane >> 5) * XST + kt * 32 + (lane & 31);
    const float* Gbase = &Gs[0][0] + (lane >> 5) * GST + ct * 32 + (lane & 31);
    for (unsigned s = 0; s < nsteps; ++s) {
        const int cur = (int)(s & 1);
        if (s + 1 < nsteps) load_step(mbeg + (s + 1) * MS);
        const float* X = Xbase + cur * (MS * XST);
        const float* G = Gbase + cur * (MS * GST);
#pragma unroll
        for (int kk = 0; kk < MS / 2; ++kk)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(X[kk * 2 * XST], G[kk * 2 * GST], acc, 0, 0, 0);
        if (s + 1 < nsteps) store(cur ^ 1);
        __syncthreads();
    }
    // partial slab [split][K][COUT]: row (k) = kb*KT + kt*32 + C-row, col (co) = ct*32 + (lane & 31)
    float* slab = a.slab + (long long)split * L::K * COUT;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int kr = kb * KT + kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        slab[kr * COUT + ct * 32 + (lane & 31)] = acc[r];
    }
    if (kb == 0) {
        // bias grad partial: column sums of this split's G rows (each thread owns columns c4*4..+3)
        constexpr int GROUPS = 256 / GUPR;
        __shared__ float bred[GROUPS * COUT];
        bred[gpx0 * COUT + c4 * 4 + 0] = bsum0;
        bred[gpx0 * COUT + c4 * 4 + 1] = bsum1;
        bred[gpx0 * COUT + c4 * 4 + 2] = bsum2;
        bred[gpx0 * COUT + c4 * 4 + 3] = bsum3;
        __syncthreads();
        if (threadIdx.x < COUT) {
            float t = 0.f;
            for (int g = 0; g < GROUPS; ++g) t += bred[g * COUT + threadIdx.x];
            a.bslab[(long long)split * COUT + threadIdx.x] = t;
        }
    }
}

// conv3 output grad: NCHW (Flatten order) -> NHWC, times the ReLU mask of h3 (NCHW)
__global__ void __launch_bounds__(256) nchw_to_nhwc_mask(const float* __restrict__ g, const float* __restrict__ h,
                                                         long long batch, float* __restrict__ out) {
    __shared__ float t[64 * 50];
    const long long n = blockIdx.x;
    const float* gs = g + n * 3136;
    const float* hs = h + n * 3136;
    for (int i = threadIdx.x; i < 3136; i += 256) {
        const int c = i / 49, p = i % 49;
        t[c * 50 + p] = hs[i] > 0.f ? gs[i] : 0.f;
    }
    __syncthreads();
    float* o = out + n * 3136;
    for (int i = threadIdx.x; i < 3136; i += 256) {
        const int p = i / 64, c = i % 64;
        o[i] = t[c * 50 + p];
    }
}

template <class Prob>
int launch_igemm(const Args& a, long long blocks, hipStream_t s, const char* name) {
    if (blocks == 0) return PPOX_OK;
    igemm_kernel<Prob><<<(unsigned)blocks, 256, 0, s>>>(a);
    PPOX_LAUNCHED(name);
}

template <class Prob, bool OUT_NCHW = false>
int launch_rgemm(const Args& a, long long blocks, hipStream_t s, const char* name) {
    if (blocks == 0) return PPOX_OK;
    rgemm_kernel<Prob, OUT_NCHW><<<(unsigned)blocks, 256, 0, s>>>(a);
    PPOX_LAUNCHED(name);
}
constexpr int RG_FWD1_MT = 2;

template <class L, bool U8>
int launch_wgrad(const WArgs& wa_in, hipStream_t s) {
    WArgs wa = wa_in;
    using C = WgCfg<L, U8>;
    const long long M = wa.batch * L::P;
    const int splits = wa.splits;
    wa.px_per_split = ppox::ceil_div(ppox::ceil_div(M, splits), MS) * MS;  // whole steps
    wgrad_kernel<L, U8><<<(unsigned)(C::KB * splits), 256, 0, s>>>(wa);
    PPOX_LAUNCHED("ppox_nature_conv_wgrad");
}

}  // namespace

extern "C" int ppox_nature_conv_fwd(int32_t layer, const void* x, int64_t batch, const int64_t* idx, int64_t T,
                                    int64_t N_env, int64_t x_sample_stride, const float* wp, const float* bias,
                                    float* y, void* stream) {
    if (batch == 0) return PPOX_OK;  // empty shard / minibatch: no pointers to check
    PPOX_REQUIRE(layer >= 1 && layer <= 3, "ppox_nature_conv_fwd: layer must be 1, 2 or 3");
    PPOX_REQUIRE(x && wp && bias && y && batch >= 0, "ppox_nature_conv_fwd: bad arguments");
    PPOX_REQUIRE(ppox::aligned16(wp), "ppox_nature_conv_fwd: packed weights must be 16-byte aligned");
    PPOX_REQUIRE(batch * G1::P < (1LL << 31), "ppox_nature_conv_fwd: batch too large for 32-bit row indexing");
    Args a{x, reinterpret_cast<const long long*>(idx), T, N_env, x_sample_stride, wp, bias, nullptr, y, batch};
    hipStream_t s = ppox::as_stream(stream);
    if (layer == 1) {
        PPOX_REQUIRE(!(reinterpret_cast<uintptr_t>(x) & 3) && (idx || x_sample_stride % 4 == 0),
                     "ppox_nature_conv_fwd: u8 input must be 4-byte aligned");
        if (idx) PPOX_REQUIRE(T > 0 && N_env > 0, "ppox_nature_conv_fwd: idx needs T and N_env");
        using R1 = RgFwd1<RG_FWD1_MT>;
        return launch_rgemm<R1>(a, ppox::ceil_div(batch * G1::P, R1::ROWS), s, "ppox_nature_conv_fwd");
    }
    PPOX_REQUIRE(ppox::aligned16(x) && !idx, "ppox_nature_conv_fwd: layer 2/3 input must be 16B-aligned NHWC");
    if (layer == 2) {
        using P2 = FwdNHWCProblem<G2, false, 1>;
        return launch_igemm<P2>(a, ppox::ceil_div(batch * G2::P, P2::BMR), s, "ppox_nature_conv_fwd");
    }
    using P3 = FwdNHWCProblem<G3, true, 1>;
    return launch_igemm<P3>(a, ppox::ceil_div(batch * G3::P, P3::BMR), s, "ppox_nature_conv_fwd");
}

extern "C" int ppox_nature_conv_dgrad(int32_t layer, const float* grad_out, int64_t batch, const float* wpd,
                                      const float* prev_act, float* grad_in, void* stream) {
    if (batch == 0) return PPOX_OK;  // empty shard / minibatch: no pointers to check
    PPOX_REQUIRE(layer == 2 || layer == 3, "ppox_nature_conv_dgrad: layer must be 2 or 3");
    PPOX_REQUIRE(grad_out && wpd && prev_act && grad_in && batch >= 0, "ppox_nature_conv_dgrad: bad arguments");
    PPOX_REQUIRE(ppox::aligned16(grad_out) && ppox::aligned16(wpd), "ppox_nature_conv_dgrad: 16B alignment");
    Args a{grad_out, nullptr, 0, 0, 0, wpd, nullptr, prev_act, grad_in, batch};
    hipStream_t s = ppox::as_stream(stream);
    if (layer == 2) {
        using D2 = DgradPMProblem<G2, 1>;
        return launch_igemm<D2>(a, ppox::ceil_div(batch, D2::BMR) * D2::NPOS, s, "ppox_nature_conv_dgrad");
    }
    using D3 = DgradPMProblem<G3, 1>;
    return launch_igemm<D3>(a, ppox::ceil_div(batch, D3::BMR) * D3::NPOS, s, "ppox_nature_conv_dgrad");
}

// split-K factor over pixels: ~4096 pixels per split, but enough splits that the
// grid (splits x k-blocks) fills the chip (>= ~1536 workgroups, 2 rounds of the
// ~768 resident slots) at small per-rank batches; at least 4 steps per split
extern "C" int64_t ppox_nature_wgrad_splits(int32_t layer, int64_t batch) {
    const long long P = layer == 1 ? G1::P : (layer == 2 ? G2::P : G3::P);
    const long long kb = layer == 1 ? WgCfg<G1, true>::KB : (layer == 2 ? WgCfg<G2, false>::KB : WgCfg<G3, false>::KB);
    const long long px = batch * P;
    long long s = (px + 4095) / 4096;
    const long long fill = (1536 + kb - 1) / kb, most = px / (4 * MS);
    if (s < fill) s = fill < most ? fill : most;
    s = s < 8 ? 8 : (s > 512 ? 512 : s);
    return (s + 7) / 8 * 8;
}

extern "C" int64_t ppox_nature_wgrad_workspace_bytes(int32_t layer, int64_t batch) {
    const long long splits = ppox_nature_wgrad_splits(layer, batch);
    const long long kc = layer == 1 ? G1::K * G1::COUT : (layer == 2 ? G2::K * G2::COUT : G3::K * G3::COUT);
    const long long c = layer == 1 ? G1::COUT : 64;
    return splits * (kc + c) * (long long)sizeof(float);
}

extern "C" int ppox_nature_conv_wgrad(int32_t layer, const void* x, int64_t batch, const int64_t* idx, int64_t T,
                                      int64_t N_env, int64_t x_sample_stride, const float* grad_out, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
    PPOX_REQUIRE(layer >= 1 && layer <= 3, "ppox_nature_conv_wgrad: layer must be 1, 2 or 3");
    PPOX_REQUIRE(x && grad_out && workspace && batch > 0, "ppox_nature_conv_wgrad: bad arguments");
    PPOX_REQUIRE(workspace_bytes >= ppox_nature_wgrad_workspace_bytes(layer, batch),
                 "ppox_nature_conv_wgrad: workspace too small");
    PPOX_REQUIRE(ppox::aligned16(grad_out), "ppox_nature_conv_wgrad: grad_out must be 16B aligned");
    const int splits = (int)ppox_nature_wgrad_splits(layer, batch);
    const long long kc = layer == 1 ? G1::K * G1::COUT : (layer == 2 ? G2::K * G2::COUT : G3::K * G3::COUT);
    float* slab = reinterpret_cast<float*>(workspace);
    WArgs wa{x, x_sample_stride, grad_out, slab, slab + (long long)splits * kc, batch, 0, splits};
    hipStream_t s = ppox::as_stream(stream);
    PPOX_REQUIRE(!idx, "ppox_nature_conv_wgrad: gathered (idx) input not supported; gather first");
    PPOX_REQUIRE(batch * (layer == 1 ? G1::P : layer == 2 ? G2::P : G3::P) < (1LL << 31) / 64,
                 "ppox_nature_conv_wgrad: batch too large for 32-bit pixel indexing");
    if (layer == 1) {
        PPOX_REQUIRE(!(reinterpret_cast<uintptr_t>(x) & 3) && x_sample_stride % 4 == 0,
                     "ppox_nature_conv_wgrad: u8 input 4-byte aligned");
        return launch_wgrad<G1, true>(wa, s);
    }
    PPOX_REQUIRE(ppox::aligned16(x) && !idx, "ppox_nature_conv_wgrad: layer 2/3 input must be 16B-aligned NHWC");
    if (layer == 2) return launch_wgrad<G2, false>(wa, s);
    return launch_wgrad<G3, false>(wa, s);
}

extern "C" int ppox_nature_wgrad_reduce(int32_t layer, int64_t batch, const void* workspace, float* dw, float* db,
                                        void* stream) {
    PPOX_REQUIRE(layer >= 1 && layer <= 3, "ppox_nature_wgrad_reduce: layer must be 1, 2 or 3");
    PPOX_REQUIRE(workspace && dw && db && batch > 0, "ppox_nature_wgrad_reduce: bad arguments");
    const int splits = (int)ppox_nature_wgrad_splits(layer, batch);
    const long long kc = layer == 1 ? G1::K * G1::COUT : (layer == 2 ? G2::K * G2::COUT : G3::K * G3::COUT);
    const float* slab = reinterpret_cast<const float*>(workspace);
    const float* bslab = slab + (long long)splits * kc;
    hipStream_t s = ppox::as_stream(stream);
    return ppox_conv::wgrad_reduce(layer, slab, bslab, splits, dw, db, s);
}

extern "C" int ppox_nchw_to_nhwc_relu_grad(const float* grad, const float* act, int64_t batch, float* out,
                                           void* stream) {
    if (batch == 0) return PPOX_OK;  // empty shard / minibatch: no pointers to check
    PPOX_REQUIRE(grad && act && out && batch >= 0, "ppox_nchw_to_nhwc_relu_grad: bad arguments");
    nchw_to_nhwc_mask<<<(unsigned)batch, 256, 0, ppox::as_stream(stream)>>>(grad, act, batch, out);
    PPOX_LAUNCHED("ppox_nchw_to_nhwc_relu_grad");
}
