// K6 — the NatureCNN weight gradients in split-f16 math, and the slab reduces of every form:
//   wgrad_split_kernel     the im2col form (conv1-3; the fc layer and the heads' hidden layer as row GEMMs)
//   wgrad2_planes_kernel   conv2, direct from H1P planes
//   wgrad1_frames_kernel   conv1, direct from the uint8 frames
//   fcwg_kernel            the fc layer, direct on PX df and PX h3
// (the direct conv3 form, dwgrad3, is in dconv.hip; the f32 math mode's wgrad_kernel in conv_f32.hip).
// Every form is a GEMM dW[k][co] = sum_m A[m][k] G[m][co] whose reduction runs over all output pixels:
// workgroups own a slice of M (split-K over pixels) and write partial slabs, and a reduce kernel sums the
// slabs in a FIXED order (deterministic) straight into the PyTorch [co][ci][ky][kx] layout (wgrad_reduce) or
// the Linear weight's (rows_wgrad_reduce, fc_wgrad_reduce_perm).  wgrad_reduce also serves conv_f32.hip,
// through ppox_conv::wgrad_reduce.
#include <algorithm>
#include <utility>

#include "gemm_layout.h"

namespace {

// sum the slabs, scatter to PyTorch [co][ci][ky][kx] (+ bias).  A block owns 4·E
// consecutive outputs (E float4 lanes of every slab row) x RG split groups; thread (e, g)
// sums splits g, g+RG, g+2RG, ... in order, then the RG group sums are combined by a
// fixed pairwise tree — one order per output, so the result is deterministic.  E x RG: 32 x 8 for the
// f32 kernels' <= 512 splits; for the split kernels' up to 2048, 32 x 32, or 8 x 128 when
// the layer has few outputs (conv1: 8,224 -> 257 blocks instead of 65, a fuller chip).
template <class L, bool NHWC_ORDER, int RED_E, int RG>
__global__ void __launch_bounds__(RED_E * RG) wgrad_reduce(const float* __restrict__ slab,
                                                         const float* __restrict__ bslab, int splits,
                                                         float* __restrict__ dw, float* __restrict__ db) {
    __shared__ float4 part[RG][RED_E];
    constexpr int KC = L::K * L::COUT;
    static_assert(KC % 4 == 0 && L::COUT % 4 == 0, "wgrad_reduce: float4 lanes");
    const int e = threadIdx.x % RED_E, grp = threadIdx.x / RED_E;
    const int i = (blockIdx.x * RED_E + e) * 4;  // first of this lane's four outputs
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    auto add = [](float4& a, const float4 b) {
        a.x += b.x;
        a.y += b.y;
        a.z += b.z;
        a.w += b.w;
    };
    // (unrolled: a lane's loads of several splits issue together; the adds keep split order)
    if (i < KC) {
#pragma unroll 8
        for (int sp = grp; sp < splits; sp += RG) add(s, *reinterpret_cast<const float4*>(slab + (long long)sp * KC + i));
    } else if (i < KC + L::COUT) {
#pragma unroll 8
        for (int sp = grp; sp < splits; sp += RG)
            add(s, *reinterpret_cast<const float4*>(bslab + (long long)sp * L::COUT + (i - KC)));
    }
    // the RG group sums combined by a fixed pairwise tree (deterministic, and its rounding
    // error grows with log2(RG) rather than RG)
    part[grp][e] = s;
    __syncthreads();
#pragma unroll
    for (int h = RG / 2; h >= 1; h >>= 1) {
        if (grp < h) add(part[grp][e], part[grp + h][e]);
        __syncthreads();
    }
    if (grp != 0) return;
    const float4 t = part[0][e];
    const float tv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int ic = i + c;
        if (ic < KC) {
            const int k = ic / L::COUT, co = ic % L::COUT;
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
            dw[((co * L::CIN + ci) * L::KH + ky) * L::KW + kx] = tv[c];
        } else if (ic < KC + L::COUT) {
            db[ic - KC] = tv[c];
        }
    }
}

template <class L, bool NHWC_ORDER>
int launch_wgrad_reduce(const float* slab, const float* bslab, int splits, float* dw, float* db, hipStream_t s) {
    ppox::ktime_mark(s);
    constexpr int N = L::K * L::COUT + L::COUT;
    if (splits >= 256 && N < 4 * 32 * 256) {  // few outputs, many splits: 8 lanes x 128 split groups
        wgrad_reduce<L, NHWC_ORDER, 8, 128><<<ppox::ceil_div(N, 32), 1024, 0, s>>>(slab, bslab, splits, dw, db);
    } else if (splits >= 256) {  // 32 split groups per element: shorter sequential chains
        wgrad_reduce<L, NHWC_ORDER, 32, 32><<<ppox::ceil_div(N, 128), 1024, 0, s>>>(slab, bslab, splits, dw, db);
    } else {
        wgrad_reduce<L, NHWC_ORDER, 32, 8><<<ppox::ceil_div(N, 128), 256, 0, s>>>(slab, bslab, splits, dw, db);
    }
    PPOX_LAUNCHED("ppox_nature_wgrad_reduce");
}

// ---------------------------------------------------------------------------
// Wgrad, split-f16.  Same decomposition as conv_f32.hip's wgrad_kernel (WG = k-block of KT rows x
// all COUT x a slice of output pixels; partial slabs reduced by wgrad_reduce), on
// v_mfma_f32_32x32x16_f16.  Per step of MS = 32 pixels the X (im2col) and G tiles
// are staged in LDS as f16 planes, row-major [pixel][k] / [pixel][co] (each f32
// value split once per workgroup into its two planes; conv1's u8 frames are
// one exact plane), and the MFMA fragments — 8 consecutive pixels of one k (A) or
// one co (B) per lane — come straight out of LDS with the transposing read
// ds_read_b64_tr_b16 (two per fragment).  32-byte chunks of a row are XOR-swizzled
// (tr_swz) so each 32-lane half's 4 rows x 2 chunks hit 8 distinct bank groups.
// conv1: 3 MFMAs per tile and k-step (x*g0, x*g1, x*g2, all exact); f32 layers: the
// six products of mfma_split6.  Loads of step s+1 fly under the MFMAs of step s.
// ---------------------------------------------------------------------------
template <class L, bool U8, int KT_>
struct WsCfg {
    static constexpr int KT = KT_, KB = L::K / KT, COUT = L::COUT;
    static constexpr int XP = U8 ? 1 : NPL;                      // X planes
    static constexpr int NKT = KT / 32, NCT = COUT / 32, TPW = NKT * NCT / 4;
    // wave grid: WC waves along co (WCT co-tiles each) x 4/WC along k (WKT k-tiles each)
    static constexpr int WCT = TPW % NCT == 0 ? NCT : (NCT % TPW == 0 ? TPW : 1);
    static constexpr int WC = NCT / WCT, WKT = NKT / (4 / WC);
    static constexpr int XR = KT * 2, GR = COUT * 2;             // LDS row bytes
    static constexpr int XPB = MS * XR, GPB = MS * GR;           // LDS plane bytes
    static constexpr int STAGE = XP * XPB + NPL * GPB;
    // staging: 8 threads per pixel row; a thread stages XU units of 8 consecutive k and GW
    // consecutive co of one pixel, so its addresses come from one (sample, pixel) pair
    static constexpr int UPX = KT / 8, XU = UPX / 8, GW = COUT / 8;
    static_assert(KB * KT == L::K && (NKT * NCT) % 4 == 0 && XU * 8 == UPX && (GW == 4 || GW == 8), "wgrad split shape");
    static_assert(WKT * WCT == TPW && 4 % WC == 0 && NKT % (4 / WC) == 0, "wave tiling");
};

// XOR on the 32-byte chunk index of row px (rows of ROWB bytes): the transposed reads
// of a 32-lane half (rows px..px+3, chunks 2t and 2t+1) then cover all 64 banks once
template <int ROWB>
__device__ inline int tr_swz(int px) {
    constexpr int m = (ROWB / 32) & 7;
    static_assert(m == 0 || m == 4 || m == 2, "tr_swz: row stride");
    if constexpr (m == 0) return 2 * (px & 3);
    else if constexpr (m == 4) return 2 * ((px >> 1) & 1);
    else return 0;
}

typedef short v4s16 __attribute__((ext_vector_type(4)));
__device__ inline uint2 lds_tr16(const uint8_t* p) {
    const v4s16 r = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s16*)p);
    return __builtin_bit_cast(uint2, r);
}

__device__ float kZeroG[64] = {};  // the G row of a pixel past a split's end (global AS: no flat loads)

// CB > 1: G rows hold CB blocks of COUT columns (row stride CB * COUT) and each
// workgroup owns one block — the fc layer's weight gradient (K = the 512 outputs,
// G = the NHWC conv3 activations, one 64-channel pixel per block); its grid is any
// number of (split, column-block, k-block) items, k-block fastest within an XCD.
// XPL / GPL (round 4): X / G are PX planes (conv_common.h; a.xexp / a.gexp): each unit's 8 values
// are read as their two 16-B plane runs and stored to LDS as they are (no split in registers)
template <class L, bool U8, int KT, bool ROWS, int CB = 1, bool XPL = false, bool GPL = false>
__global__ void __launch_bounds__(256, 2) wgrad_split_kernel(WArgs a) {
    using C = WsCfg<L, U8, KT>;
    static_assert(!(XPL && U8) && (!GPL || C::GW == 8), "PX operands: f32 X, 8 G values per thread");
    constexpr int COUT = L::COUT, XP = C::XP, XR = C::XR, GR = C::GR, XU = C::XU;
    constexpr int WKT = C::WKT, WCT = C::WCT, GS = CB * COUT;
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * C::STAGE];
    int kb, split, cb;
    if constexpr (CB == 1) {
        const int b = blockIdx.x, xcd = b & 7, q = b >> 3;
        kb = q % C::KB;
        split = (q / C::KB) * 8 + xcd;
        cb = 0;
    } else {
        // k-block fastest: the KB workgroups that read one G column block (CB > 1: a pixel of
        // the fc layer's h3) run together on one XCD and share it through its L2 (column-block
        // fastest re-streamed every block from HBM once per k-block: 3.5x the algorithmic bytes)
        const long long w = xcd_remap(blockIdx.x, gridDim.x);
        kb = (int)(w % C::KB);
        cb = (int)((w / C::KB) % CB);
        split = (int)(w / (CB * C::KB));
    }
    const unsigned M = (unsigned)(a.batch * L::P);
    const unsigned long long mb64 = (unsigned long long)split * (unsigned long long)a.px_per_split;
    const unsigned mbeg = mb64 < M ? (unsigned)mb64 : M;
    const unsigned mend = (unsigned)min((unsigned long long)M, (unsigned long long)mbeg + a.px_per_split);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kt0 = (wave / C::WC) * WKT, ct0 = (wave % C::WC) * WCT;

    f32x16 hi[WKT][WCT], lo[WKT][WCT];
#pragma unroll
    for (int i = 0; i < WKT; ++i)
#pragma unroll
        for (int j = 0; j < WCT; ++j) hi[i][j] = lo[i][j] = zero16();

    constexpr unsigned long long SAMPLE_F32 = (unsigned long long)L::IH * L::IW * L::CIN;
    const uint8_t* xu8 = reinterpret_cast<const uint8_t*>(a.x);
    const float* xf = reinterpret_cast<const float*>(a.x);
    constexpr int GW = C::GW;
    // raw global data of one step; the pipeline holds two (steps s+1 and s+2 during step s)
    struct Raw {
        uint32_t xw[XU][2];
        float4 xr[XU][2];
        float4 gr[2];
    };
    // one step's f16 planes in registers (split under the MFMAs of the step before)
    struct Planes {
        u32x4 x[XU][NPL];
        u32x4 g[NPL];
        uint2 g4[NPL];
    };
    // operand scales from the amax slots (uint8 X: exact at scale 1); the slab is unscaled
    const int ex = U8 ? 0 : (XPL ? *a.xexp : split_scale_exp(amax_read(a.amax_x)));
    const int eg = GPL ? *a.gexp : split_scale_exp(amax_read(a.amax_g));
    const float sx = exp2i(ex), sg = exp2i(eg), uo = exp2i(-ex) * exp2i(-eg);
    const float ub = GPL ? exp2i(-eg) : 1.f;  // GPL: the bias sums add the scaled values
    Raw raw[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {  // defined values: the last step splits a set it never stores
#pragma unroll
        for (int i = 0; i < XU; ++i) {
            raw[t].xw[i][0] = raw[t].xw[i][1] = 0u;
            raw[t].xr[i][0] = raw[t].xr[i][1] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        raw[t].gr[0] = raw[t].gr[1] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float bsum[GW];
#pragma unroll
    for (int e = 0; e < GW; ++e) bsum[e] = 0.f;
    // this thread's pixel row and units; the pixel advances by MS per step (at most one
    // wrap into the next sample: MS <= P), so no 64-bit index is divided in the loop
    // unit i of the thread is j = 8i + (tid & 7): the 8 threads of a pixel row write 128
    // contiguous bytes per store instruction (bank-conflict-free)
    const int pxl = tid >> 3, ju = tid & 7, gco = (tid & 7) * GW;
    const unsigned long long sstride = U8 ? (unsigned long long)a.sample_stride : SAMPLE_F32;
    // byte (u8) / float offset of sample n: through the rollout rows when a.idx is set (u8
    // only); the next sample's base is fetched one wrap ahead, so the idx load's latency
    // hides under the steps in between
    auto sbase = [&](unsigned n) -> unsigned long long {
        if constexpr (ROWS) {
            const unsigned nc = n < (unsigned)a.batch ? n : (unsigned)a.batch - 1;
            const long long i = a.idx[nc];
            return (unsigned long long)(((i % a.T) * a.Nenv + i / a.T) * (long long)(L::CIN * L::IH * L::IW));
        }
        return n * sstride;
    };
    unsigned xp, mcur = mbeg + pxl, ncur;
    unsigned long long sb, sbn;
    {
        const unsigned m = mcur < M ? mcur : mbeg;
        ncur = m / L::P;
        xp = m - ncur * L::P;
        sb = sbase(ncur);
        sbn = sbase(ncur + 1);
    }
    // a pixel that always exists (an empty split, mbeg == M, still issues its loads)
    const unsigned m0 = mbeg < M ? mbeg : M - 1;
    const unsigned xp0 = m0 - (m0 / L::P) * L::P;
    const unsigned long long sb00 = sbase(m0 / L::P);
    int koff[XU];
#pragma unroll
    for (int i = 0; i < XU; ++i) {
        const int k = kb * KT + 8 * (8 * i + ju);
        if constexpr (U8) {
            koff[i] = ((k >> 6) * L::IH + ((k >> 3) & 7)) * L::IW;
        } else {
            const int tap = k / L::CIN;
            koff[i] = ((tap / L::KW) * L::IW + tap % L::KW) * L::CIN + k % L::CIN;
        }
    }

    // loads of one step (steps are loaded in order; the state above advances).  Branch-free,
    // so the loads, the split of the step before and the MFMAs share one basic block: a pixel
    // past the split's end loads a valid pixel's X (finite) and a zero G row (kZeroG), so its
    // products vanish
    auto load = [&](Raw& r) {
        const bool ok = mcur < mend;
        const unsigned p = ok ? xp : xp0;
        const unsigned long long s0 = ok ? sb : sb00;
        const unsigned oy = p / L::OW, ox = p - oy * L::OW;
        if constexpr (U8) {
            const uint8_t* s = xu8 + s0 + oy * L::S * L::IW + ox * L::S;
#pragma unroll
            for (int i = 0; i < XU; ++i) {
                r.xw[i][0] = *reinterpret_cast<const uint32_t*>(s + koff[i]);
                r.xw[i][1] = *reinterpret_cast<const uint32_t*>(s + koff[i] + 4);
            }
        } else if constexpr (XPL) {
            // the unit's 8 channels lie in one 32-group: its high plane run, and 64 B on its low one
            const char* s = reinterpret_cast<const char*>(xf) + 4 * (s0 + (oy * L::S * L::IW + ox * L::S) * L::CIN);
#pragma unroll
            for (int i = 0; i < XU; ++i) {
                const char* q = s + 4 * (koff[i] & ~31) + 2 * (koff[i] & 31);
                r.xr[i][0] = *reinterpret_cast<const float4*>(q);
                r.xr[i][1] = *reinterpret_cast<const float4*>(q + 64);
            }
        } else {
            const float* s = xf + s0 + (oy * L::S * L::IW + ox * L::S) * L::CIN;
#pragma unroll
            for (int i = 0; i < XU; ++i) {
                r.xr[i][0] = *reinterpret_cast<const float4*>(s + koff[i]);
                r.xr[i][1] = *reinterpret_cast<const float4*>(s + koff[i] + 4);
            }
        }
        if constexpr (GPL) {
            const unsigned long long ge = (unsigned long long)mcur * GS + cb * COUT + gco;  // gco % 8 == 0
            const char* q = ok ? reinterpret_cast<const char*>(a.g) + 4 * (ge & ~31ULL) + 2 * (ge & 31)
                               : reinterpret_cast<const char*>(kZeroG) + 4 * (gco & ~31) + 2 * (gco & 31);
            r.gr[0] = *reinterpret_cast<const float4*>(q);
            r.gr[1] = *reinterpret_cast<const float4*>(q + 64);
        } else {
            const float* sg = ok ? a.g + (unsigned long long)mcur * GS + cb * COUT + gco : kZeroG + gco;
            r.gr[0] = *reinterpret_cast<const float4*>(sg);
            if constexpr (GW == 8) r.gr[1] = *reinterpret_cast<const float4*>(sg + 4);
        }
        mcur += MS;
        if constexpr (L::P == 1) {  // one pixel per sample (the fc layer): sample = pixel
            sb = (unsigned long long)mcur * sstride;
            return;
        }
        xp += MS;
        const bool wrap = xp >= (unsigned)L::P;
        xp = wrap ? xp - L::P : xp;
        if constexpr (ROWS) {
            if (wrap) {  // rollout rows: the next sample's base was fetched one wrap ahead
                ++ncur;
                sb = sbn;
                sbn = sbase(ncur + 1);
            }
        } else {
            sb = wrap ? sb + sstride : sb;
        }
    };
    auto to_planes = [&](const Raw& r, Planes& p) {
#pragma unroll
        for (int i = 0; i < XU; ++i) {
            if constexpr (U8) {
                p.x[i][0] = u8x8_to_f16(r.xw[i][0], r.xw[i][1]);
            } else if constexpr (XPL) {
                p.x[i][0] = __builtin_bit_cast(u32x4, r.xr[i][0]);
                p.x[i][1] = __builtin_bit_cast(u32x4, r.xr[i][1]);
            } else {
                split8h(r.xr[i][0], r.xr[i][1], sx, p.x[i][0], p.x[i][1]);
            }
        }
        if constexpr (GPL) {
            p.g[0] = __builtin_bit_cast(u32x4, r.gr[0]);
            p.g[1] = __builtin_bit_cast(u32x4, r.gr[1]);
        } else if constexpr (GW == 8) {
            split8h(r.gr[0], r.gr[1], sg, p.g[0], p.g[1]);
        } else {
            split4h(r.gr[0], sg, p.g4[0], p.g4[1]);
        }
    };
    auto store = [&](const Planes& p, const Raw& r, int buf) {
        uint8_t* base = lds + buf * C::STAGE;
#pragma unroll
        for (int i = 0; i < XU; ++i) {
            const int j = 8 * i + ju;
            const int off = pxl * XR + (((j >> 1) ^ tr_swz<XR>(pxl)) << 5) + ((j & 1) << 4);
#pragma unroll
            for (int q = 0; q < XP; ++q) *reinterpret_cast<u32x4*>(base + q * C::XPB + off) = p.x[i][q];
        }
        uint8_t* gb = base + XP * C::XPB;
        const int goff = pxl * GR + (((gco >> 4) ^ tr_swz<GR>(pxl)) << 5) + (gco & 15) * 2;
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            if constexpr (GW == 8)
                *reinterpret_cast<u32x4*>(gb + q * C::GPB + goff) = p.g[q];
            else
                *reinterpret_cast<uint2*>(gb + q * C::GPB + goff) = p.g4[q];
        }
        if constexpr (GPL) {
            if constexpr (CB == 1) {  // the bias gradient (the fc layer has none here): hi + lo, scaled
                const u32x4 hw = p.g[0], lw = p.g[1];
#pragma unroll
                for (int e = 0; e < 8; ++e) bsum[e] += px_value(hw[e >> 1], lw[e >> 1], e & 1);
            }
        } else {
            bsum[0] += r.gr[0].x;
            bsum[1] += r.gr[0].y;
            bsum[2] += r.gr[0].z;
            bsum[3] += r.gr[0].w;
            if constexpr (GW == 8) {
                bsum[4] += r.gr[1].x;
                bsum[5] += r.gr[1].y;
                bsum[6] += r.gr[1].z;
                bsum[7] += r.gr[1].w;
            }
        }
    };
    // per-lane transposed-read offsets (T10): lane 4qq+pp of each 16-lane group supplies
    // row qq, columns 4pp..4pp+3 of its 4-row x 16-column block; the block's rows are
    // pixels 16ks + 8h + 4r + qq, its columns chunk 2t + g16 of the row
    const int g16 = (lane >> 4) & 1, h = lane >> 5, qq = (lane >> 2) & 3, pp = lane & 3;
    const int rowx = (8 * h + qq) * XR + pp * 8, rowg = (8 * h + qq) * GR + pp * 8;
    const int swx = tr_swz<XR>(qq), swg = tr_swz<GR>(qq);
    auto frag = [&](const uint8_t* plane, int rowoff, int rowb, int chunk, int ks) {
        const uint8_t* p = plane + rowoff + 16 * ks * rowb + (chunk << 5);
        const uint2 r0 = lds_tr16(p), r1 = lds_tr16(p + 4 * rowb);
        u32x4 f;
        f[0] = r0.x;
        f[1] = r0.y;
        f[2] = r1.x;
        f[3] = r1.y;
        return f;
    };
    auto compute = [&](int buf) {
        const uint8_t* base = lds + buf * C::STAGE;
        const uint8_t* gb = base + XP * C::XPB;
#pragma unroll
        for (int ks = 0; ks < MS / 16; ++ks) {
            u32x4 bq[WCT][NPL];
#pragma unroll
            for (int j = 0; j < WCT; ++j)
#pragma unroll
                for (int p = 0; p < NPL; ++p)
                    bq[j][p] = frag(gb + p * C::GPB, rowg, GR, (2 * (ct0 + j) + g16) ^ swg, ks);
#pragma unroll
            for (int i = 0; i < WKT; ++i) {
                u32x4 aq[NPL];
#pragma unroll
                for (int p = 0; p < XP; ++p) aq[p] = frag(base + p * C::XPB, rowx, XR, (2 * (kt0 + i) + g16) ^ swx, ks);
#pragma unroll
                for (int j = 0; j < WCT; ++j) {
                    if constexpr (U8) {
                        hi[i][j] = mfma_f16(aq[0], bq[j][0], hi[i][j]);
                        lo[i][j] = mfma_f16(aq[0], bq[j][1], lo[i][j]);
                    } else {
                        mfma_split3(aq, bq[j], hi[i][j], lo[i][j]);
                    }
                }
            }
        }
    };

    // two-deep pipeline, one basic block per step: step s+1's raw registers (loaded during
    // step s-1) are split into planes, step s+2's loads are issued into the set just freed,
    // the compiler interleaves the split's VALU work with step s's fragment reads and MFMAs,
    // and the planes go to the other LDS buffer after them.  Raw sets and buffers alternate,
    // so both are static.  (Measured: 5-10 % faster than one-deep staging after the MFMAs;
    // forcing the interleave with sched_group_barrier was slower than the compiler's.)
    const unsigned nsteps = mend > mbeg ? (mend - mbeg + MS - 1) / MS : 0;
    load(raw[0]);
    load(raw[1]);
    if (nsteps > 0) {
        Planes p;
        to_planes(raw[0], p);
        store(p, raw[0], 0);
    }
    __syncthreads();
    auto step = [&](unsigned s, auto cur_tag) {
        constexpr int CUR = decltype(cur_tag)::value;  // LDS buffer and raw set of step s
        Planes p;
        to_planes(raw[CUR ^ 1], p);
        load(raw[CUR]);
        compute(CUR);
        // unconditional (one basic block): past the last step the set holds a zero-G step,
        // written to a buffer nothing reads again (bsum adds zeros)
        store(p, raw[CUR ^ 1], CUR ^ 1);
        __syncthreads();
    };
    for (unsigned s = 0; s < nsteps; s += 2) {
        step(s, std::integral_constant<int, 0>{});
        if (s + 1 < nsteps) step(s + 1, std::integral_constant<int, 1>{});
    }
    float* slab = a.slab + (long long)split * L::K * GS + cb * COUT;
#pragma unroll
    for (int i = 0; i < WKT; ++i)
#pragma unroll
        for (int j = 0; j < WCT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kr = kb * KT + (kt0 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                slab[kr * GS + (ct0 + j) * 32 + (lane & 31)] = (hi[i][j][r] + lo[i][j][r]) * uo;
            }
    if (CB == 1 && kb == 0) {
        // bias grad partial: column sums of this split's G rows, combined in a fixed order
        float* bred = reinterpret_cast<float*>(lds);  // the loop ended on a barrier
#pragma unroll
        for (int e = 0; e < GW; ++e) bred[pxl * COUT + gco + e] = bsum[e];
        __syncthreads();
        if (tid < COUT) {
            float t = 0.f;
            for (int g = 0; g < MS; ++g) t += bred[g * COUT + tid];
            a.bslab[(long long)split * COUT + tid] = t * ub;
        }
    }
}

constexpr int WS_KT2 = 128;
constexpr int WS_KT3 = 64;
constexpr int WS_PX = 2048;  // split wgrad: pixels per split-K slice
constexpr int WS_FILL = 512;  // split wgrad: workgroups at least (conv1 / conv2, small batches)
// split wgrad: its own split-K count (~WS_PX pixels per split so the grid fills the chip)
template <class L, bool U8, int KT, bool XPL = false, bool GPL = false>
struct WsLaunch {
    using C = WsCfg<L, U8, KT>;
    static long long splits(long long batch) {
        const long long px = batch * L::P;
        long long s = (px + WS_PX - 1) / WS_PX;
        // small batches (the 8-GPU per-rank minibatch): enough splits for two workgroups per CU
        // where the k-blocks are few (conv1/conv2 at B = 2048: 0.082 -> 0.074 / 0.100 -> 0.078 ms;
        // conv3's nine k-blocks already give 441 workgroups, and more splits measured slower)
        if constexpr (C::KB <= 4) {
            const long long fill = (WS_FILL + C::KB - 1) / C::KB;
            s = s < fill ? fill : s;
        }
        const long long most = (px + MS - 1) / MS;  // at least one step per split
        s = s > most ? most : s;
        s = s < 8 ? 8 : (s > 2048 ? 2048 : s);
        return (s + 7) / 8 * 8;
    }
    static long long workspace_bytes(long long batch) {
        return splits(batch) * (long long)(L::K * L::COUT + L::COUT) * (long long)sizeof(float);
    }
    static int run(const void* x, long long sample_stride, const float* g, long long batch, void* ws, float* dw,
                   float* db, const uint32_t* amax_x, const uint32_t* amax_g, hipStream_t s,
                   const long long* idx = nullptr, long long T = 0, long long Nenv = 0, const int* xexp = nullptr,
                   const int* gexp = nullptr) {
        const int sp = (int)splits(batch);
        float* slab = reinterpret_cast<float*>(ws);
        WArgs wa{x, sample_stride, g, slab, slab + (long long)sp * L::K * L::COUT, batch, 0, sp, idx, T, Nenv,
                 amax_x, amax_g};
        wa.xexp = xexp;
        wa.gexp = gexp;
        const long long M = batch * L::P;
        wa.px_per_split = ppox::ceil_div(ppox::ceil_div(M, sp), MS) * MS;
        if (U8 && idx != nullptr)
            wgrad_split_kernel<L, U8, KT, U8><<<(unsigned)(C::KB * sp), 256, 0, s>>>(wa);
        else
            wgrad_split_kernel<L, U8, KT, false, 1, XPL, GPL><<<(unsigned)(C::KB * sp), 256, 0, s>>>(wa);
        PPOX_LAUNCHED_NORET("ppox_nature_conv_wgrad_split");
        return launch_wgrad_reduce<L, !U8>(slab, wa.bslab, sp, dw, db, s);
    }
};
using Ws1 = WsLaunch<G1, true, 256>;
using Ws2 = WsLaunch<G2, false, WS_KT2>;
using Ws3 = WsLaunch<G3, false, WS_KT3>;
using Ws3PP = WsLaunch<G3, false, WS_KT3, true, true>;  // PX h2 and g3
using Ws3PF = WsLaunch<G3, false, WS_KT3, true, false>;
using Ws3FP = WsLaunch<G3, false, WS_KT3, false, true>;

// ---------------------------------------------------------------------------
// conv2 weight gradient from H1P planes, direct (no im2col):
//   dW[tap][ci][co] = sum over samples n and output pixels p = (oy, ox) of
//                     h1[n][2 oy + ky][2 ox + kx][ci] * g2[n][p][co]       (+ db[co] = sum g2)
// One 512-thread workgroup per CU walks its own run of samples.  Per sample the whole H1P image
// (20 x 20 x 32, both f16 planes: 51 KB) is DMA'd into LDS and the sample's 81 G rows (f32) are
// split there into two f16 planes: every h1 and g2 byte is read from HBM once (the im2col form,
// wgrad_split_kernel, re-fetched h1 ~3.2x through L2 and split every value once per k-block).
// The reduction runs over the sample's 81 pixels in 6 k-steps of 16 (G rows 81..95 are zero):
// wave w owns taps 2w, 2w + 1 x all 64 output channels (4 tiles, 12 MFMAs per k-step).  The A
// fragment rows are h1 pixels (2 oy + ky, 2 ox + kx), read with the transposing LDS read: the
// image is stored column-parity split (slot = y * 20 + (x & 1) * 10 + (x >> 1), 64 B per slot and
// plane), so consecutive output pixels of one tap are consecutive slots (conflict-free reads) and
// a tap is one uniform slot offset.  G rows are 128 B per plane with 32-B chunks XOR-swizzled
// (tr_swz<128>).  Double-buffered: sample s + 1's DMAs and G loads fly under sample s's MFMAs.
// Partial slabs per workgroup, summed in a fixed order by wgrad_reduce (deterministic).
// LDS: G planes of both buffers first (so every B read's offset is an immediate), then the H
// images: 2 x 24 KB + 2 x 50 KB = 148 KB.
// ---------------------------------------------------------------------------
constexpr int W2P_GP = 96 * 128;                 // one G plane: 96 rows x 64 co x f16
constexpr int W2P_GB = 2 * W2P_GP;               // both G planes of one buffer
constexpr int W2P_HP = 400 * 64;                 // one H1P plane image: 400 slots x 32 ci x f16
constexpr int W2P_HB = 2 * W2P_HP;               // both planes of one buffer
constexpr int W2P_H0 = 2 * W2P_GB;               // the H images follow both buffers' G planes
constexpr int W2P_LDS = 2 * W2P_GB + 2 * W2P_HB;  // 151,552 B
constexpr int W2P_NDMA = 7;                      // 1-KB DMAs per wave and sample (50 per sample)
constexpr int W2P_SAMPLE = 400 * 128;            // H1P bytes per sample
constexpr int W2P_G4 = 81 * 64 / 4;              // float4 of G per sample (1296)
static_assert(W2P_LDS <= 160 * 1024, "wgrad2 planes: LDS");
static_assert(8 * W2P_NDMA >= 2 * W2P_HP / 1024 && 2 * W2P_HP % 1024 == 0, "wgrad2 planes: DMA split");

struct W2PArgs {
    const uint16_t* h1p;     // H1P [batch][400][32 hi | 32 lo]
    const int* h1_exp;       // h1 * 2^E = hi + lo
    const float* g;          // g2 [batch][81][64] f32 NHWC (ReLU mask applied), or its PX planes (g_exp)
    const uint32_t* amax_g;  // g2's amax slots (f32 g2)
    const int* g_exp = nullptr;  // PX g2: the planes' exponent
    float* slab;             // [gridDim.x][512][64]
    float* bslab;            // [gridDim.x][64]
    long long batch;
    int per;                 // samples per workgroup (every workgroup has at least one)
};

typedef unsigned int u32x2v __attribute__((ext_vector_type(2)));
// transposing LDS read in inline asm: hipcc would otherwise wait for the in-flight LDS-DMA of the
// next sample (vmcnt(0)) before every read, exposing the prefetch
__device__ inline u32x2v w2p_tr(uint32_t addr) {
    u32x2v r;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r) : "v"(addr));
    return r;
}
template <int OFF>
__device__ inline u32x2v w2p_tr_o(uint32_t addr) {
    u32x2v r;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "i"(OFF));
    return r;
}
// one k-step's 16 fragment halves landed (tied, so the MFMAs use the post-wait values)
__device__ inline void w2p_lgkm_wait(u32x2v (&x)[16]) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]),
                   "+v"(x[8]), "+v"(x[9]), "+v"(x[10]), "+v"(x[11]), "+v"(x[12]), "+v"(x[13]), "+v"(x[14]),
                   "+v"(x[15]));
}
__device__ inline int w2p_tapoff(int t) {  // uniform slot offset of tap t = ky * 4 + kx
    const int ky = t >> 2, kx = t & 3;
    return 20 * ky + 10 * (kx & 1) + (kx >> 1);
}

// GPL: g2 arrives as its PX planes (round 5: the conv3 dgrad's planes output) — copied to LDS as they lie
// (no split), the bias partials summed from the planes
template <bool GPL>
__global__ void __launch_bounds__(512, 1) wgrad2_planes_kernel(W2PArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[W2P_LDS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long s0 = (long long)blockIdx.x * a.per;
    const long long s1 = min(a.batch, s0 + (long long)a.per);
    const uint32_t lds0 = (uint32_t)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) uint8_t*)lds);
    // operand scales: G by its tensor's amax (PX: its planes' exponent), h1 by its H1P exponent; the
    // slab is unscaled
    const int eg = GPL ? *a.g_exp : split_scale_exp(amax_read(a.amax_g)), ex = *a.h1_exp;
    const float sg = exp2i(eg), uo = exp2i(-eg) * exp2i(-ex);

    // H1P DMA sources of this wave's pieces (byte offsets within a sample): DMA i (0..49) fills
    // LDS bytes [1024 i, 1024 i + 1024) of the image (plane i / 25); lane l's 16 B are piece
    // (l & 3) of slot (1024 (i % 25) + 16 l) / 64.  DMAs past the 50th re-copy the 50th.
    uint32_t hsrc[W2P_NDMA];
#pragma unroll
    for (int j = 0; j < W2P_NDMA; ++j) {
        int i = wave * W2P_NDMA + j;
        i = i < 49 ? i : 49;
        const int P = i / 25, within = (i % 25) * 1024 + lane * 16;
        const int slot = within >> 6, piece = (within >> 4) & 3;
        const int y = slot / 20, xs = slot % 20, x = xs < 10 ? 2 * xs : 2 * (xs - 10) + 1;
        hsrc[j] = (uint32_t)((y * 20 + x) * 128 + P * 64 + piece * 16);
    }
    auto dma_h = [&](long long n, int buf) {
        const char* sb = reinterpret_cast<const char*>(a.h1p) + n * W2P_SAMPLE;  // uniform 64-bit sample base
#pragma unroll
        for (int j = 0; j < W2P_NDMA; ++j) {
            int i = wave * W2P_NDMA + j;
            i = i < 49 ? i : 49;
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void*)(sb + hsrc[j]),
                (__attribute__((address_space(3))) void*)(lds + W2P_H0 + buf * W2P_HB + i * 1024), 16, 0, 0);
        }
    };
    // G: float4 q = tid + 512 r of the sample's 1296 (row q >> 4, channels 4 (q & 15) ..); the third
    // only for tid < 272 (others re-load the last float4 and store nothing)
    const int gc4 = tid & 15;
    float4 graw[3];
    auto load_g = [&](long long n) {
        const float4* src = reinterpret_cast<const float4*>(a.g) + n * W2P_G4;
        graw[0] = src[tid];
        graw[1] = src[tid + 512];
        graw[2] = src[tid < W2P_G4 - 1024 ? tid + 1024 : W2P_G4 - 1];
    };
    // bias partials: f32 g2 — the thread's 4 channels (gc4); planes — the 8 channels of its 16-B piece gc4
    // of one plane (summed as values of that plane: hi and lo partials added at the end)
    float bsum[GPL ? 8 : 4] = {};
    auto store_g = [&](int buf, bool add_bias) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            if (GPL && (r < 2 || tid < W2P_G4 - 1024)) {
                // piece gc4 of a 256-B pixel: plane P = (gc4 >> 2) & 1, channels c0 .. c0 + 7
                const int row = (tid + 512 * r) >> 4, P = (gc4 >> 2) & 1, c0 = 32 * (gc4 >> 3) + 8 * (gc4 & 3);
                const int chunk = c0 >> 4;
                const int off = buf * W2P_GB + P * W2P_GP + row * 128 + ((chunk ^ (2 * ((row >> 1) & 1))) << 5) +
                                (c0 & 15) * 2;
                *reinterpret_cast<float4*>(lds + off) = graw[r];
                if (add_bias) {
                    const f16x8 hv = __builtin_bit_cast(f16x8, graw[r]);
#pragma unroll
                    for (int e = 0; e < 8; ++e) bsum[e] += (float)hv[e];
                }
            } else if (!GPL && (r < 2 || tid < W2P_G4 - 1024)) {
                const int row = (tid + 512 * r) >> 4, chunk = gc4 >> 2;
                const int off = buf * W2P_GB + row * 128 + ((chunk ^ (2 * ((row >> 1) & 1))) << 5) + (gc4 & 3) * 8;
                uint2 hv, lv;
                split4h(graw[r], sg, hv, lv);
                *reinterpret_cast<uint2*>(lds + off) = hv;
                *reinterpret_cast<uint2*>(lds + off + W2P_GP) = lv;
                if (add_bias) {
                    bsum[0] += graw[r].x;
                    bsum[1] += graw[r].y;
                    bsum[2] += graw[r].z;
                    bsum[3] += graw[r].w;
                }
            }
        }
    };
    // zero G rows 81..95 of both buffers and planes once (the loads never write them)
    if (tid < 480) {
        const int pl = tid / 120, o = (tid % 120) * 16;
        *reinterpret_cast<u32x4*>(lds + pl * W2P_GP + 81 * 128 + o) = u32x4{0u, 0u, 0u, 0u};
    }

    // fragment addresses: lane (h, g16, qq, pp) supplies row qq (+ 4 for the second read) of the
    // 8-row group h of k-step ks, 8 B at column chunk g16
    const int h = lane >> 5, g16 = (lane >> 4) & 1, qq = (lane >> 2) & 3, pp = lane & 3;
    uint32_t aaddr[6][2];
#pragma unroll
    for (int ks = 0; ks < 6; ++ks)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            int p = 16 * ks + 8 * h + 4 * r + qq;
            p = p < 81 ? p : 80;  // rows past the 81 pixels: any valid slot (their G rows are zero)
            aaddr[ks][r] = lds0 + W2P_H0 + (uint32_t)((40 * (p / 9) + p % 9) * 64 + g16 * 32 + pp * 8);
        }
    const uint32_t toff[2] = {(uint32_t)w2p_tapoff(2 * wave) * 64u, (uint32_t)w2p_tapoff(2 * wave + 1) * 64u};
    const int swz = 2 * ((qq >> 1) & 1);
    const uint32_t baddr[2] = {lds0 + (uint32_t)((8 * h + qq) * 128 + (((0 + g16) ^ swz) << 5) + pp * 8),
                               lds0 + (uint32_t)((8 * h + qq) * 128 + (((2 + g16) ^ swz) << 5) + pp * 8)};

    f32x16 hi[2][2], lo[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) hi[i][j] = lo[i][j] = zero16();

    auto compute = [&](auto BUF) {
        constexpr int buf = decltype(BUF)::value;
#pragma unroll
        for (int ks = 0; ks < 6; ++ks) {
            u32x2v v[16];  // [i or j][plane][r]: A halves 0..7, B halves 8..15
            // the k-step's two row addresses, laundered so the compiler does not hoist all 96
            // (k-step, row, tap, plane, buffer) sums out of the sample loop into registers
            uint32_t ab[2] = {aaddr[ks][0], aaddr[ks][1]};
            asm volatile("" : "+v"(ab[0]), "+v"(ab[1]));
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int P = 0; P < 2; ++P)
#pragma unroll
                    for (int r = 0; r < 2; ++r)
                        v[(i * 2 + P) * 2 + r] = w2p_tr(ab[r] + (toff[i] + (uint32_t)(buf * W2P_HB + P * W2P_HP)));
            // B: co-tile j, plane P, rows +0 / +4 of the k-step (offsets are immediates)
            constexpr int B0 = buf * W2P_GB;
            auto bread = [&](auto KS) {
                constexpr int o = B0 + decltype(KS)::value * 2048;
                v[8] = w2p_tr_o<o>(baddr[0]);
                v[9] = w2p_tr_o<o + 512>(baddr[0]);
                v[10] = w2p_tr_o<o + W2P_GP>(baddr[0]);
                v[11] = w2p_tr_o<o + W2P_GP + 512>(baddr[0]);
                v[12] = w2p_tr_o<o>(baddr[1]);
                v[13] = w2p_tr_o<o + 512>(baddr[1]);
                v[14] = w2p_tr_o<o + W2P_GP>(baddr[1]);
                v[15] = w2p_tr_o<o + W2P_GP + 512>(baddr[1]);
            };
            switch (ks) {  // ks is a constant of the unrolled loop
                case 0: bread(std::integral_constant<int, 0>{}); break;
                case 1: bread(std::integral_constant<int, 1>{}); break;
                case 2: bread(std::integral_constant<int, 2>{}); break;
                case 3: bread(std::integral_constant<int, 3>{}); break;
                case 4: bread(std::integral_constant<int, 4>{}); break;
                default: bread(std::integral_constant<int, 5>{}); break;
            }
            w2p_lgkm_wait(v);
            u32x4 af[2][NPL], bf[2][NPL];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int P = 0; P < 2; ++P) {
                    const u32x2v x0 = v[(i * 2 + P) * 2], x1 = v[(i * 2 + P) * 2 + 1];
                    const u32x2v y0 = v[8 + (i * 2 + P) * 2], y1 = v[8 + (i * 2 + P) * 2 + 1];
                    af[i][P] = u32x4{x0.x, x0.y, x1.x, x1.y};
                    bf[i][P] = u32x4{y0.x, y0.y, y1.x, y1.y};
                }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) mfma_split3(af[i], bf[j], hi[i][j], lo[i][j]);
        }
    };
    auto barrier = [] { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory"); };

    dma_h(s0, 0);
    load_g(s0);
    store_g(0, true);
    barrier();
    // one step: sample s + 1 (clamped: past the last sample a dummy copy of s into the idle
    // buffer, no bias) issued, sample s computed, s + 1's G split into the other buffer
    auto step = [&](long long s, auto BUF) {
        constexpr int buf = decltype(BUF)::value;
        const bool nxt = s + 1 < s1;
        const long long sn = nxt ? s + 1 : s;
        dma_h(sn, buf ^ 1);
        load_g(sn);
        compute(BUF);
        store_g(buf ^ 1, nxt);
        barrier();
    };
#pragma unroll 1
    for (long long s = s0; s < s1; s += 2) {
        step(s, std::integral_constant<int, 0>{});
        if (s + 1 < s1) step(s + 1, std::integral_constant<int, 1>{});
    }
    float* slab = a.slab + (long long)blockIdx.x * (G2::K * G2::COUT);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = (2 * wave + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                slab[k * G2::COUT + j * 32 + (lane & 31)] = (hi[i][j][r] + lo[i][j][r]) * uo;
            }
    // bias partial: threads with the same gc4 hold the same channels; summed in thread order
    float* red = reinterpret_cast<float*>(lds);  // the loop ended on a barrier
    constexpr int NB = GPL ? 8 : 4;
#pragma unroll
    for (int e = 0; e < NB; ++e) red[tid * NB + e] = bsum[e];
    __syncthreads();
    if (tid < G2::COUT) {
        float t = 0.f;
        if constexpr (GPL) {  // channel tid: the high plane's piece, then the low plane's (4 pieces on)
            const int ph = 8 * (tid >> 5) + ((tid & 31) >> 3), e = tid & 7;
            float th = 0.f, tl = 0.f;
            for (int k = 0; k < 32; ++k) th += red[(ph + 16 * k) * 8 + e];
            for (int k = 0; k < 32; ++k) tl += red[(ph + 4 + 16 * k) * 8 + e];
            t = (th + tl) * exp2i(-eg);
        } else {
            const int c4 = tid >> 2, e = tid & 3;
            for (int k = 0; k < 32; ++k) t += red[(c4 + 16 * k) * 4 + e];
        }
        a.bslab[(long long)blockIdx.x * G2::COUT + tid] = t;
    }
}

// ---------------------------------------------------------------------------
// conv1 weight gradient, direct (no im2col; round 3):
//   dW1[co][ci][ky][kx] = sum over samples n and output pixels (oy, ox) of
//                         x[n][ci][4 oy + ky][4 ox + kx] * g1[n][oy][ox][co]   (+ db1[co] = sum g1)
// One 512-thread workgroup per CU walks its own run of samples in units of half a sample: 10 output
// rows, whose input rows 40 hh .. 40 hh + 43 of the 4 channels are 14.8 KB of frame bytes and whose
// 200 g1 rows are 25.6 KB — every frame and g1 byte is read from HBM once (the im2col form,
// wgrad_split_kernel, re-read each frame byte ~3.6x through L2: 8x8 windows at stride 4, and ran
// latency-bound at small batches).  A unit's frame rows go global -> registers -> LDS phase-split:
// byte x of a row is stored at phase x & 3, position x >> 2, so the 8 output pixels (4 ox + kx) of
// one tap are 8 consecutive bytes of one phase row, from position ox + (kx >> 2) (an 8-B and a
// 4-B read, shifted by v_alignbyte).  Its g1 rows are split into two f16 planes in LDS (split-f16,
// the scale from g1's amax slots), 24 slots per output row (ox 20..23 hold zero rows, so the
// k-steps of 16 pixels never straddle a row).  MFMA D[k][co] += X[k][px] G[px][co], k = 64 ci +
// 8 ky + kx: eight tiles of 32 k; wave w owns tiles 2 (w & 3) and 2 (w & 3) + 1 (input channel
// w & 3) on the k-steps of parity w >> 2, two exact products per tile (x * g_hi, x * g_lo: frames
// are exact in f16) in separate accumulators.  Double-buffered: unit u + 1's loads fly under unit
// u's MFMAs.  Each workgroup writes two partial slabs (its two k-step parities), summed with the
// others in a fixed order by wgrad_reduce (deterministic).  LDS: 2 x (23.4 + 30 KB) = 107 KB.
// ---------------------------------------------------------------------------
constexpr int W1F_ROWS = 44;                   // input rows of a unit (per channel)
constexpr int W1F_PR = 32;                     // bytes per phase row (positions 0..20 real; reads reach 27)
constexpr int W1F_YS = 4 * W1F_PR + 8;         // bytes per (ci, y): four phase rows + 8 (spreads the banks)
constexpr int W1F_PH = 4 * W1F_ROWS * W1F_YS;  // phase image of a unit: 23,936 B
constexpr int W1F_GP = 240 * 64;               // one G plane: 10 rows x 24 slots x 32 co x f16
constexpr int W1F_BUF = W1F_PH + 2 * W1F_GP;   // one buffer: 54,656 B
constexpr int W1F_LDS = 2 * W1F_BUF;           // 109,312 B
constexpr int W1F_XU = 4 * W1F_ROWS * 6;       // frame pieces of a unit: (ci, y, 16-B group) = 1056
constexpr int W1F_G4 = 200 * 8;                // float4 of g1 per unit: 1600
constexpr int W1F_SAMPLE = 4 * 84 * 84;        // frame bytes per sample
constexpr int W1F_DEPTH = 2;  // units of loads in flight (register sets)
constexpr int W1F_FLUSH = 8;  // units per partial sum (4 samples: ~960 pixels per accumulation chain and parity)
static_assert(W1F_DEPTH == 2 || W1F_DEPTH == 3, "wgrad1 frames: two or three register sets");
static_assert(W1F_LDS <= 160 * 1024 && W1F_PH % 16 == 0 && W1F_YS % 8 == 0, "wgrad1 frames: LDS layout");
static_assert(W1F_XU <= 3 * 512 && W1F_G4 <= 4 * 512, "wgrad1 frames: loads per thread");

struct W1FArgs {
    const uint8_t* x;          // frames (u8), sample n at n * sample_stride, or rollout row idx[n]
    long long sample_stride;
    const long long* idx;      // optional env-major rollout rows of the step-major (T, Nenv, 4, 84, 84) frames
    long long T, Nenv;
    const float* g;            // g1 [batch][400][32] f32 NHWC (ReLU mask applied)
    const uint32_t* amax_g;    // g1's amax slots
    float* slab;               // [2 gridDim.x][256][32]
    float* bslab;              // [2 gridDim.x][32]
    long long batch;
    int per;                   // samples per workgroup (every workgroup has at least one)
};

typedef uint32_t u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));

template <bool IDX>
__global__ void __launch_bounds__(512, 1) wgrad1_frames_kernel(W1FArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[W1F_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n0 = (long long)blockIdx.x * a.per;
    const long long n1 = min(a.batch, n0 + (long long)a.per);
    const int nunits = (int)(2 * (n1 - n0));
    const int eg = split_scale_exp(amax_read(a.amax_g));
    const float sg = exp2i(eg), uo = exp2i(-eg);

    // frame base of a sample; through idx the next sample's row is fetched one sample ahead
    // (host-checked T * Nenv < 2^31: 32-bit row arithmetic)
    const uint32_t T32 = (uint32_t)a.T, N32 = (uint32_t)a.Nenv;
    auto row_base = [&](long long i) -> long long {
        const uint32_t i32 = (uint32_t)i, q = i32 / T32;
        return (long long)((i32 - q * T32) * N32 + q) * (long long)W1F_SAMPLE;
    };
    long long base = IDX ? row_base(a.idx[n0]) : n0 * a.sample_stride;
    long long pref = IDX ? a.idx[n0 + 1 < n1 ? n0 + 1 : n0] : 0;

    // this thread's loads of a unit: frame pieces q = tid + 512 j (ci, y, 16-B group), g1 float4s
    // q = tid + 512 j (pixel q >> 3, channels 4 (q & 7) ..); past the ends a clamped piece is loaded
    // and not stored.  W1F_DEPTH register sets: unit v's in set v % W1F_DEPTH, loaded that many units ahead
    struct Raw {
        u32x4 x[3];
        float4 g[4];
    };
    Raw raw[W1F_DEPTH];
    auto load = [&](Raw& r, long long b, long long n, int hh) {
        u32x4 (&xr)[3] = r.x;
        float4 (&gr)[4] = r.g;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            int q = tid + 512 * j;
            q = q < W1F_XU ? q : W1F_XU - 1;
            const int ci = q / (W1F_ROWS * 6), rem = q - ci * (W1F_ROWS * 6), y = rem / 6, jg = rem - y * 6;
            const long long off = b + ci * (84 * 84) + (40 * hh + y) * 84 + (jg < 5 ? 16 * jg : 68);
            const u32x4a4 v = *reinterpret_cast<const u32x4a4*>(a.x + off);
            xr[j] = u32x4{v.x, v.y, v.z, v.w};
        }
        const float4* gs = reinterpret_cast<const float4*>(a.g + (n * 400 + hh * 200) * 32);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = tid + 512 * j;
            gr[j] = gs[q < W1F_G4 ? q : W1F_G4 - 1];
        }
    };
    float bsum[4] = {0.f, 0.f, 0.f, 0.f};
    auto store = [&](const Raw& r, int buf, bool add_bias) {
        const u32x4 (&xr)[3] = r.x;
        const float4 (&gr)[4] = r.g;
        uint8_t* B = lds + buf * W1F_BUF;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int q = tid + 512 * j;
            if (q < W1F_XU) {
                const int ci = q / (W1F_ROWS * 6), rem = q - ci * (W1F_ROWS * 6), y = rem / 6, jg = rem - y * 6;
                // dwords d0..d3 = positions 4 jg .. 4 jg + 3 (jg = 5: only position 20, the load's last dword)
                const bool last = jg == 5;
                const uint32_t d0 = last ? xr[j][3] : xr[j][0], d1 = last ? 0u : xr[j][1];
                const uint32_t d2 = last ? 0u : xr[j][2], d3 = last ? 0u : xr[j][3];
                // 4 x 4 byte transpose: phase r's dword = byte r of d0..d3
                const uint32_t e01 = __builtin_amdgcn_perm(d1, d0, 0x06020400u), o01 = __builtin_amdgcn_perm(d1, d0, 0x07030501u);
                const uint32_t e23 = __builtin_amdgcn_perm(d3, d2, 0x06020400u), o23 = __builtin_amdgcn_perm(d3, d2, 0x07030501u);
                uint8_t* dst = B + (ci * W1F_ROWS + y) * W1F_YS + 4 * jg;
                *reinterpret_cast<uint32_t*>(dst + 0 * W1F_PR) = __builtin_amdgcn_perm(e23, e01, 0x05040100u);
                *reinterpret_cast<uint32_t*>(dst + 1 * W1F_PR) = __builtin_amdgcn_perm(o23, o01, 0x05040100u);
                *reinterpret_cast<uint32_t*>(dst + 2 * W1F_PR) = __builtin_amdgcn_perm(e23, e01, 0x07060302u);
                *reinterpret_cast<uint32_t*>(dst + 3 * W1F_PR) = __builtin_amdgcn_perm(o23, o01, 0x07060302u);
            }
        }
        uint8_t* G = B + W1F_PH;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = tid + 512 * j;
            if (q < W1F_G4) {
                const int px = q >> 3, slot = (px / 20) * 24 + px % 20;
                uint2 hv, lv;
                split4h(gr[j], sg, hv, lv);
                *reinterpret_cast<uint2*>(G + slot * 64 + (q & 7) * 8) = hv;
                *reinterpret_cast<uint2*>(G + W1F_GP + slot * 64 + (q & 7) * 8) = lv;
                if (add_bias) {
                    bsum[0] += gr[j].x;
                    bsum[1] += gr[j].y;
                    bsum[2] += gr[j].z;
                    bsum[3] += gr[j].w;
                }
            }
        }
    };
    // zero G rows of the pad slots (ox 20..23) of both buffers and planes once: 640 x 16 B
    for (int i = tid; i < 640; i += 512) {
        const int bp = i / 160, w = i % 160, row = w / 16, c = w % 16;  // (buffer, plane), output row, 16 B
        *reinterpret_cast<u32x4*>(lds + (bp >> 1) * W1F_BUF + W1F_PH + (bp & 1) * W1F_GP + (row * 24 + 20) * 64 + c * 16) =
            u32x4{0u, 0u, 0u, 0u};
    }

    // A: lane (m, h) of tile 2 tp + tt holds k = 64 tp + 32 tt + m: ky = 4 tt + (m >> 3), kx = m & 7
    const int tp = wave & 3, par = wave >> 2, m = lane & 31, h = lane >> 5;
    const int kx = m & 7, sh = kx >> 2;
    int abase[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) abase[tt] = (tp * W1F_ROWS + 4 * tt + (m >> 3)) * W1F_YS + (kx & 3) * W1F_PR;
    // B: the transposed-read lane offsets of wgrad_split_kernel (64-B rows, no swizzle)
    const int g16 = (lane >> 4) & 1, qq = (lane >> 2) & 3, pp = lane & 3;
    const int rowg = (8 * h + qq) * 64 + pp * 8 + (g16 << 5);

    // hi / lo: the running products of W1F_FLUSH units, then added into tot and restarted, so no
    // f32 accumulation chain grows past ~1,000 pixels however many samples the workgroup walks
    f32x16 hi[2], lo[2], tot[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) hi[tt] = lo[tt] = tot[tt] = zero16();

    auto compute = [&](int buf) {
        const uint8_t* B = lds + buf * W1F_BUF;
        const uint8_t* G = B + W1F_PH;
#pragma unroll
        for (int ks2 = 0; ks2 < 8; ++ks2) {
            const int ks = 2 * ks2 + par;  // this wave's k-steps (15 per unit: parity 1 has seven)
            if (ks < 15) {
                const int gi = 2 * ks + h, goff = (gi / 3) * 4 * W1F_YS + 8 * (gi % 3);
                u32x4 af[2];
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    const uint8_t* p = B + abase[tt] + goff;
                    const uint2 v = *reinterpret_cast<const uint2*>(p);
                    const uint32_t w2 = *reinterpret_cast<const uint32_t*>(p + 8);
                    af[tt] = u8x8_to_f16(__builtin_amdgcn_alignbyte(v.y, v.x, sh), __builtin_amdgcn_alignbyte(w2, v.y, sh));
                }
                u32x4 bq[2];
#pragma unroll
                for (int P = 0; P < 2; ++P) {
                    const uint8_t* p = G + P * W1F_GP + rowg + 16 * ks * 64;
                    const uint2 r0 = lds_tr16(p), r1 = lds_tr16(p + 4 * 64);
                    bq[P] = u32x4{r0.x, r0.y, r1.x, r1.y};
                }
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    hi[tt] = mfma_f16(af[tt], bq[0], hi[tt]);
                    lo[tt] = mfma_f16(af[tt], bq[1], lo[tt]);
                }
            }
        }
    };

    // unit v's loads into set v & 1 (past the last unit: the last again, stored to the idle buffer
    // without its bias); a new sample's frame base from the idx value prefetched a sample ahead
    // branch-free (selects, and the idx load issued for every unit): a load under a branch makes
    // hipcc's waits at the join drain every load in flight, the next units' prefetch included
    auto issue = [&](int v, auto SET) {
        const int vc = v < nunits ? v : nunits - 1;
        const long long nv = n0 + (vc >> 1);
        const bool fresh = (v & 1) == 0 && v < nunits && v > 0;
        if constexpr (IDX) {
            // base from the idx value loaded at the previous unit (the next sample's), then the
            // value for the sample after this one (the same load for both halves of a sample)
            base = fresh ? row_base(pref) : base;
            pref = a.idx[nv + 1 < n1 ? nv + 1 : n1 - 1];
        } else {
            base = fresh ? nv * a.sample_stride : base;
        }
        load(raw[decltype(SET)::value], base, nv, vc & 1);
    };
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, 1>;
    using S2 = std::integral_constant<int, 2>;
    issue(0, S0{});
    issue(1, S1{});
    if constexpr (W1F_DEPTH == 3) issue(2, S2{});
    store(raw[0], 0, true);
    __syncthreads();
    // step u (set SET = u % W1F_DEPTH): unit u + W1F_DEPTH's loads into the set unit u held, unit u
    // computed (LDS buffer u & 1), unit u + 1 (loaded earlier) split into the other buffer
    auto step = [&](int u, auto SET) {
        constexpr int set = decltype(SET)::value, nset = (set + 1) % W1F_DEPTH;
        issue(u + W1F_DEPTH, SET);
        compute(u & 1);
        if ((u + 1) % W1F_FLUSH == 0 || u + 1 == nunits) {
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
                for (int q = 0; q < 16; ++q) tot[tt][q] += hi[tt][q] + lo[tt][q];
                hi[tt] = lo[tt] = zero16();
            }
        }
        store(raw[nset], (u + 1) & 1, u + 1 < nunits);
        __syncthreads();
    };
#pragma unroll 1
    for (int u = 0; u < nunits; u += W1F_DEPTH) {
        step(u, S0{});
        if (u + 1 < nunits) step(u + 1, S1{});
        if constexpr (W1F_DEPTH == 3)
            if (u + 2 < nunits) step(u + 2, S2{});
    }

    const int split = 2 * blockIdx.x + par;
    float* slab = a.slab + (long long)split * (G1::K * G1::COUT);
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = 64 * tp + 32 * tt + (r & 3) + 8 * (r >> 2) + 4 * h;
            slab[k * G1::COUT + m] = tot[tt][r] * uo;
        }
    // bias partial: threads with the same tid & 7 hold the same four channels; summed in thread order
    float* red = reinterpret_cast<float*>(lds);  // the loop ended on a barrier
#pragma unroll
    for (int e = 0; e < 4; ++e) red[tid * 4 + e] = bsum[e];
    __syncthreads();
    if (tid < G1::COUT) {
        const int c4 = tid >> 2, e = tid & 3;
        float t = 0.f;
        for (int k = 0; k < 64; ++k) t += red[(c4 + 8 * k) * 4 + e];
        a.bslab[(long long)2 * blockIdx.x * G1::COUT + tid] = t;
        a.bslab[(long long)(2 * blockIdx.x + 1) * G1::COUT + tid] = 0.f;
    }
}

// wgrad2_planes_kernel / wgrad1_frames_kernel: samples per workgroup and workgroups (one per CU, none empty)
void w2p_grid(long long batch, int& per, long long& grid) {
    const long long cus = std::max(1, cu_count());
    per = (int)ppox::ceil_div(batch, std::min(batch, cus));
    grid = ppox::ceil_div(batch, (long long)per);
}

// the direct conv1 weight gradient (wgrad1_frames_kernel, one workgroup per CU) + its slab reduce;
// PPOX_WGRAD1_IM2COL=1 runs the im2col form (wgrad_split_kernel) instead
bool wgrad1_im2col() {
    static const int v = [] {
        const char* e = ppox::ab_env("PPOX_WGRAD1_IM2COL");
        return e && e[0] == '1' ? 1 : 0;
    }();
    return v != 0;
}
int launch_wgrad1_frames(const void* x, long long sample_stride, const long long* idx, long long T, long long Nenv,
                         const float* g, long long batch, void* ws, long long ws_bytes, float* dw, float* db,
                         const uint32_t* amax_g, hipStream_t s) {
    int per;
    long long grid;
    w2p_grid(batch, per, grid);
    PPOX_REQUIRE(2 * grid * (long long)(G1::K * G1::COUT + G1::COUT) * 4 <= ws_bytes,
                 "ppox_nature_conv_wgrad_split: workspace too small for the direct conv1 weight gradient");
    PPOX_REQUIRE(!idx || T * Nenv < (1LL << 31), "ppox_nature_conv_wgrad_split_idx: T * N_env must be < 2^31");
    float* slab = reinterpret_cast<float*>(ws);
    W1FArgs a{reinterpret_cast<const uint8_t*>(x), sample_stride, idx, T, Nenv, g, amax_g, slab,
              slab + 2 * grid * (G1::K * G1::COUT), batch, per};
    if (idx)
        wgrad1_frames_kernel<true><<<(unsigned)grid, 512, 0, s>>>(a);
    else
        wgrad1_frames_kernel<false><<<(unsigned)grid, 512, 0, s>>>(a);
    PPOX_LAUNCHED_NORET("ppox_nature_conv_wgrad_split");
    return launch_wgrad_reduce<G1, false>(slab, a.bslab, (int)(2 * grid), dw, db, s);
}

}  // namespace

namespace ppox_conv {
int wgrad_reduce(int layer, const float* slab, const float* bslab, int splits, float* dw, float* db, hipStream_t s) {
    if (layer == 1) return launch_wgrad_reduce<G1, false>(slab, bslab, splits, dw, db, s);
    if (layer == 2) return launch_wgrad_reduce<G2, true>(slab, bslab, splits, dw, db, s);
    return launch_wgrad_reduce<G3, true>(slab, bslab, splits, dw, db, s);
}
}  // namespace ppox_conv

// ---- NatureCNN fc layer (3136 -> 512): the weight gradient -------------------------
// Weight gradient dW = df^T h3 on the split wgrad kernel: "pixels" = samples (GFc has one
// output pixel), K = the 512 outputs (X = df rows), G = the NHWC conv3 activations in 49
// blocks of 64 channels (one spatial position each, NHWC feature order f = p * 64 + c).
// Split-K partial slabs [split][512][3136] are summed in a fixed order by fc_wgrad_reduce,
// which writes dW in the Flatten order of the fc weight.
using GFc = Geo<512, 1, 1, 1, 1, 1, 64>;
constexpr int FCW_KT = 128, FCW_CB = 49;
template <int CB, int MAXS>
struct RowsWgrad {
    using C = WsCfg<GFc, false, FCW_KT>;
    static constexpr long long TILES = (long long)C::KB * CB;
    static constexpr long long SLAB = (long long)GFc::K * CB * GFc::COUT;  // floats per split
    // the split count whose (rounds of 512 workgroup slots) x (steps per split + 3 of fixed
    // prologue / epilogue cost) is least: 13 at B = 16384 (4.98 rounds), 5 at B = 2048 (fc)
    static int splits(long long batch) {
        int best = 1;
        long long best_cost = -1;
        for (int sp = 1; sp <= MAXS; ++sp) {
            const long long steps = ppox::ceil_div(ppox::ceil_div(batch, (long long)sp), (long long)MS);
            if (sp > 1 && steps < 2) break;
            const long long cost = ppox::ceil_div(TILES * sp, 512LL) * (steps + 3);
            if (best_cost < 0 || cost < best_cost) {
                best_cost = cost;
                best = sp;
            }
        }
        return best;
    }
    static long long workspace_bytes(long long batch) { return splits(batch) * SLAB * (long long)sizeof(float); }
};
using FcWgrad = RowsWgrad<FCW_CB, 16>;
using HeadWgrad = RowsWgrad<512 / 64, 128>;  // the heads' hidden layer: G = f in 8 column blocks

// slabs [splits][512][N] summed in split order; PERM: the fc's NHWC features -> Flatten order
template <int N, bool PERM>
__global__ void __launch_bounds__(256) rows_wgrad_reduce(const float* __restrict__ slab, int splits,
                                                         float* __restrict__ dw) {
    constexpr long long SL = 512LL * N;
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;  // 4 slab elements (o, feature)
    if (i >= SL) return;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int sp = 0; sp < splits; ++sp) {  // (unrolled: the splits' loads issue together)
        const float4 v = *reinterpret_cast<const float4*>(slab + sp * SL + i);
        t.x += v.x;
        t.y += v.y;
        t.z += v.z;
        t.w += v.w;
    }
    if constexpr (PERM) {
        const int o = (int)(i / N), f = (int)(i - (long long)o * N);  // N % 4 == 0: one row
        float* row = dw + (long long)o * N;
        row[fc_nchw_feature(f)] = t.x;
        row[fc_nchw_feature(f + 1)] = t.y;
        row[fc_nchw_feature(f + 2)] = t.z;
        row[fc_nchw_feature(f + 3)] = t.w;
    } else {  // dw may be a 4-B aligned view (a parameter's grad in the flat buffer)
        dw[i] = t.x;
        dw[i + 1] = t.y;
        dw[i + 2] = t.z;
        dw[i + 3] = t.w;
    }
}

// The fc layer's reduce: one workgroup per output row o.  The row's 3136 NHWC-ordered sums (same
// split order as rows_wgrad_reduce: bitwise the same values) are staged in LDS, then written in
// Flatten order q = c * 49 + p (NHWC f = p * 64 + c) as coalesced stores; the staging row is padded
// one float per 64 (f + (f >> 6) = 65 p + c), so the strided reads of consecutive q hit distinct banks.
// (rows_wgrad_reduce<3136, true> scattered every store across 49-float strides.)
__global__ void __launch_bounds__(256) fc_wgrad_reduce_perm(const float* __restrict__ slab, int splits,
                                                            float* __restrict__ dw) {
    constexpr int N = 3136, N4 = N / 4, UPT = (N4 + 255) / 256;
    constexpr long long SL = 512LL * N;
    static_assert(N == 49 * 64 && UPT == 4, "fc reduce shape");
    __shared__ float row[N + N / 64];
    const int o = blockIdx.x, t = threadIdx.x;
    const float* base = slab + (long long)o * N;
    float4 acc[UPT];
    int uo[UPT];
#pragma unroll
    for (int k = 0; k < UPT; ++k) {
        acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        const int u = t + 256 * k;
        uo[k] = 4 * (u < N4 ? u : N4 - 1);  // clamped: loads unconditional, the extra unit not stored
    }
#pragma unroll 2
    for (int sp = 0; sp < splits; ++sp) {
        float4 v[UPT];
#pragma unroll
        for (int k = 0; k < UPT; ++k) v[k] = *reinterpret_cast<const float4*>(base + sp * SL + uo[k]);
#pragma unroll
        for (int k = 0; k < UPT; ++k) {
            acc[k].x += v[k].x;
            acc[k].y += v[k].y;
            acc[k].z += v[k].z;
            acc[k].w += v[k].w;
        }
    }
#pragma unroll
    for (int k = 0; k < UPT; ++k) {
        if (t + 256 * k >= N4) break;
        const int f = uo[k], r = f + (f >> 6);  // the 4 features share one 64-block
        row[r] = acc[k].x;
        row[r + 1] = acc[k].y;
        row[r + 2] = acc[k].z;
        row[r + 3] = acc[k].w;
    }
    __syncthreads();
    float* out = dw + (long long)o * N;
    for (int q = t; q < N; q += 256) {
        const int c = q / 49, pp = q - 49 * c;
        out[q] = row[65 * pp + c];
    }
}

// ---------------------------------------------------------------------------
// fc weight gradient, direct (round 6; models-checkpoint.py:60 Linear(3136, 512) trained by ppo.py:241):
//   dW[o][f] = sum over rows r of df[r][o] h3[r][f]      (f = p * 64 + c, NHWC; stored in Flatten order by the reduce)
// on PX df and PX h3 (both operands as their two f16 planes, as the fc dgrad and forward read them).  The split
// wgrad form (wgrad_split_kernel<GFc>) tiles 128 outputs x one pixel (64 features) per workgroup, two per CU, and
// needs 13 split-K slabs at 16,384 rows to fill the chip: its L2 -> LDS staging is ~0.5 KB per MFMA and its slabs
// + reduce 84 MB each way (PMC 2.0x the algorithmic bytes).  Here one 256-thread workgroup per
// CU owns 256 outputs x 2 pixels (128 features) over a fifth of the rows: 50 tiles x 5 splits = 250 workgroups,
// 0.33 KB staged per MFMA, 5 slabs.
//   * per 16-row k-step the workgroup stages 24 sub-images of 16 rows x 32 columns f16 (1 KB each): df (8 output
//     groups x 2 planes) and h3 (2 pixels x 2 channel halves x 2 planes), each lane one 16-B piece by a register
//     load (row lane >> 2, piece lane & 3), stored to LDS as it lies (a sub-image = 1 KB contiguous, the
//     transposing read's layout of dwgrad3_kernel: lane (h, g16, qq, pp) reads rows 8 h + qq (+ 4) at column
//     32 g16 + 8 pp, conflict-free);
//   * wave w: outputs 128 (w & 1) .. + 127 of the workgroup's 256 (4 tiles) x pixel w >> 1 (2 tiles): 8 tiles,
//     hi / lo accumulator pairs (hA hB | hA lB + lA hB, as the split wgrad form), 24 MFMAs per k-step;
//   * two-deep register pipeline (step s + 2's loads fly while step s + 1 goes to the other LDS slot under step
//     s's MFMAs), one barrier per k-step; rows past the split read a zero df piece;
//   * partial slabs [split][512][3136] (NHWC features) summed in split order by fc_wgrad_reduce_perm.
constexpr int FWG_KS = 16, FWG_GROUPS = 25, FWG_SPLITS = 5;    // k-step rows; 2-pixel groups (the 25th: pixel 48)
constexpr int FWG_NA = 16, FWG_NB = 8, FWG_SUB = FWG_KS * 64;  // df / h3 sub-images per k-step; bytes each
constexpr int FWG_STAGE = (FWG_NA + FWG_NB) * FWG_SUB, FWG_NSLOT = 3;  // 24 KB per slot
constexpr int FWG_P = (FWG_NA + FWG_NB) / 4;                   // pieces per thread per k-step: 6 (4 df, 2 h3)
constexpr long long FWG_DFROW = 1024 * 2, FWG_H3ROW = 49 * 256;  // PX row bytes

struct FwgArgs {
    const uint8_t* df;  // PX df [batch][16 groups: 32 hi | 32 lo f16]
    const uint8_t* h3;  // PX h3 [batch][49 pixels: (hi | lo) x 2 channel halves]
    const int *df_exp, *h3_exp;
    float* slab;  // [splits][512][3136]
    long long batch, rows_per_split;
};
__device__ __attribute__((aligned(16))) uint8_t kFwgZero[64] = {};  // the df piece of a row past the split

// the accumulators live in AGPRs (16 f32x16 = all 256 of them; hipcc, left to place them, shuttled them between
// the register files and spilled): the MFMAs are inline asm, the fragments VGPRs.  PAD: 2 wait states before the
// MFMA (a fragment assembled by a VALU move must not be read as an MFMA source sooner; hipcc pads nothing in asm
// and may place the move anywhere before its use — every MFMA here is padded: an s_nop issues inside the previous
// MFMA's 32 cycles)
__device__ inline void fwg_zero(f32x16& c, const u32x4& z) {  // c = 0 x 0 + 0, defined in AGPRs
    // padded too: hipcc writes z (v_mov) right before the first of these (read unpadded, stale lanes made NaN)
    asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_f16 %0, %1, %1, 0" : "=a"(c) : "v"(z));
}
template <bool PAD>
__device__ inline void fwg_mfma(f32x16& c, const u32x4& x, const u32x4& y) {
    static_assert(PAD, "fwg_mfma: every MFMA padded");
    asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(c) : "v"(x), "v"(y));
}

// wait for every outstanding LDS read of this wave; F's 24 registers named, so no use moves above the wait
template <class Frag>
__device__ inline void fwg_wait(Frag& F) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(F.b[0]), "+v"(F.b[1]), "+v"(F.b[2]), "+v"(F.b[3]), "+v"(F.b[4]), "+v"(F.b[5]), "+v"(F.b[6]),
                   "+v"(F.b[7]));
    asm volatile("" : "+v"(F.a0[0]), "+v"(F.a0[1]), "+v"(F.a0[2]), "+v"(F.a0[3]), "+v"(F.a0[4]), "+v"(F.a0[5]),
                      "+v"(F.a0[6]), "+v"(F.a0[7]));
    asm volatile("" : "+v"(F.a1[0]), "+v"(F.a1[1]), "+v"(F.a1[2]), "+v"(F.a1[3]), "+v"(F.a1[4]), "+v"(F.a1[5]),
                      "+v"(F.a1[6]), "+v"(F.a1[7]));
}

template <class Fn, int... I>
__device__ inline void fwg_unroll(Fn&& fn, std::integer_sequence<int, I...>) {
    (fn(std::integral_constant<int, I>{}), ...);
}
// the transposing fragment read at a compile-time offset (one base address per operand; asm so the offsets fold
// into the instruction: the compiler's own form kept a 64-bit generic address per sub-image)
template <int OFF>
__device__ inline uint2 fwg_tr(uint32_t addr) {
    uint2 r;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF) : "memory");
    return r;
}
// wait until at most N of this wave's LDS reads are outstanding; x: the registers those reads fill
template <int N, int K>
__device__ inline void fwg_lgkm(uint2 (&x)[K]) {
    static_assert(K == 8, "fwg_lgkm: 8 reads");
    asm volatile("s_waitcnt lgkmcnt(%8)"
                 : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7])
                 : "n"(N));
}

__global__ void __launch_bounds__(256, 1) fcwg_kernel(FwgArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[FWG_NSLOT * FWG_STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // item = (split, feature group, output half), the output half fastest: the workgroups of one XCD share their
    // split's df rows (and each h3 pixel pair with its other half) through its L2
    const long long w = xcd_remap(blockIdx.x, gridDim.x);
    const int oh = (int)(w & 1), fg = (int)((w >> 1) % FWG_GROUPS), split = (int)(w / (2 * FWG_GROUPS));
    const long long r0 = (long long)split * a.rows_per_split;
    const long long r1 = min(a.batch, r0 + a.rows_per_split);
    const int nsteps = r1 > r0 ? (int)((r1 - r0 + FWG_KS - 1) / FWG_KS) : 0;
    // this thread's pieces: sub-image wave + 4 i (i < 4: df output group 8 oh + ((wave + 4 i) >> 1), plane
    // (wave + 4 i) & 1; i >= 4: h3 pixel, half, plane), row lane >> 2, 16-B piece lane & 3.  Buffer loads: 32-bit
    // offsets, and a row past the split reads past the buffer's end, which returns zeros
    const int prow = lane >> 2, pc = lane & 3;
    uint32_t aoff[4], boff[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int sub = wave + 4 * i;
        aoff[i] = (uint32_t)((8 * oh + (sub >> 1)) * 128 + (sub & 1) * 64 + pc * 16);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int sub = wave + 4 * i;  // (pixel, half, plane) = (sub >> 2, (sub >> 1) & 1, sub & 1)
        const int px = min(2 * fg + (sub >> 2), 48);
        boff[i] = (uint32_t)(px * 256 + ((sub >> 1) & 1) * 128 + (sub & 1) * 64 + pc * 16);
    }
    const auto a_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(a.df + r0 * FWG_DFROW), 0,
                                                        (int)((r1 - r0) * FWG_DFROW), 0x00020000);
    const auto b_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(a.h3 + r0 * FWG_H3ROW), 0,
                                                        (int)((r1 - r0) * FWG_H3ROW), 0x00020000);
    struct Raw {
        u32x4 v[FWG_P];
    };
    auto load = [&](Raw& raw, int step) {
        const uint32_t r = (uint32_t)(step * FWG_KS + prow);  // split-relative; past the end: zeros
        const uint32_t ra = r * (uint32_t)FWG_DFROW, rb = r * (uint32_t)FWG_H3ROW;
#pragma unroll
        for (int i = 0; i < 4; ++i) raw.v[i] = __builtin_amdgcn_raw_buffer_load_b128(a_rs, (int)(ra + aoff[i]), 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i) raw.v[4 + i] = __builtin_amdgcn_raw_buffer_load_b128(b_rs, (int)(rb + boff[i]), 0, 0);
    };
    auto store = [&](const Raw& raw, int slot) {
        uint8_t* st = lds + slot * FWG_STAGE;
#pragma unroll
        for (int i = 0; i < FWG_P; ++i) *reinterpret_cast<u32x4*>(st + (tid + 256 * i) * 16) = raw.v[i];
    };
    // fragment reads (the transposing pattern of dwgrad3_kernel on 64-B rows): wave w reads df output groups
    // 4 (w & 1) .. + 3 of the workgroup's 8 and h3 pixel w >> 1
    const int h = lane >> 5, g16 = (lane >> 4) & 1, qq = (lane >> 2) & 3, pp = lane & 3;
    const int wo = wave & 1, wp = wave >> 1;
    const uint32_t lds0 = (uint32_t)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) uint8_t*)lds);
    const uint32_t lrow = (uint32_t)((8 * h + qq) * 64 + g16 * 32 + pp * 8);
    const uint32_t abase = lds0 + lrow + (uint32_t)(wo * 8 * FWG_SUB);
    const uint32_t bbase = lds0 + lrow + (uint32_t)((FWG_NA + wp * 4) * FWG_SUB);
    f32x16 hi[4][2], lo[4][2];
    {
        const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                fwg_zero(hi[i][j], z);
                fwg_zero(lo[i][j], z);
            }
    }
    auto cat = [](uint2 x0, uint2 x1) { return u32x4{x0.x, x0.y, x1.x, x1.y}; };
    // one k-step's fragments: h3 (j, plane, row half) and df tiles 0-1, 2-3 (tile, plane, row half)
    struct Frag {
        uint2 b[8], a0[8], a1[8];
    };
    // issue the 24 transposing reads of the k-step in LDS slot `slot` (they complete under the MFMAs of the
    // previous k-step: waited for by fwg_wait at the top of the next)
    auto issue = [&](Frag& F, int slot) {
        const uint32_t so = (uint32_t)(slot * FWG_STAGE), ab = abase + so, bb = bbase + so;
        fwg_unroll([&](auto X) {  // B: (j, P, half) = (x >> 2, (x >> 1) & 1, x & 1)
            constexpr int x = decltype(X)::value;
            F.b[x] = fwg_tr<((x >> 2) * 2 + ((x >> 1) & 1)) * FWG_SUB + (x & 1) * 256>(bb);
        }, std::make_integer_sequence<int, 8>{});
        fwg_unroll([&](auto X) {  // A tiles 0-1: (i, P, half)
            constexpr int x = decltype(X)::value;
            F.a0[x] = fwg_tr<((x >> 2) * 2 + ((x >> 1) & 1)) * FWG_SUB + (x & 1) * 256>(ab);
        }, std::make_integer_sequence<int, 8>{});
        fwg_unroll([&](auto X) {  // A tiles 2-3
            constexpr int x = decltype(X)::value;
            F.a1[x] = fwg_tr<((2 + (x >> 2)) * 2 + ((x >> 1) & 1)) * FWG_SUB + (x & 1) * 256>(ab);
        }, std::make_integer_sequence<int, 8>{});
    };
    auto mma = [&](const Frag& F) {
        const u32x4 bq[2][2] = {{cat(F.b[0], F.b[1]), cat(F.b[2], F.b[3])}, {cat(F.b[4], F.b[5]), cat(F.b[6], F.b[7])}};
        auto tile = [&](int i, const uint2 (&ra)[8], int t) {
            const u32x4 a0 = cat(ra[4 * t], ra[4 * t + 1]), a1 = cat(ra[4 * t + 2], ra[4 * t + 3]);
            // hA hB into hi, hA lB + lA hB into lo (mfma_split3)
            fwg_mfma<true>(hi[i][0], a0, bq[0][0]);
            fwg_mfma<true>(lo[i][0], a0, bq[0][1]);
            fwg_mfma<true>(lo[i][0], a1, bq[0][0]);
            fwg_mfma<true>(hi[i][1], a0, bq[1][0]);
            fwg_mfma<true>(lo[i][1], a0, bq[1][1]);
            fwg_mfma<true>(lo[i][1], a1, bq[1][0]);
        };
        tile(0, F.a0, 0);
        tile(1, F.a0, 1);
        tile(2, F.a1, 0);
        tile(3, F.a1, 1);
    };
    // three LDS slots, two register stages: at the top of k-step s, step s's fragments are in flight (issued in
    // step s - 1), step s + 1 sits in slot (s + 1) % 3, raw[s & 1] holds step s + 2.  Step s: wait for its
    // fragments, issue step s + 1's, its 24 MFMAs, store step s + 2 into slot (s + 2) % 3 (= (s - 1) % 3, whose
    // reads every wave waited for in step s - 1, before the barrier that ended it), load step s + 4, barrier
    Raw raw[2];
    load(raw[0], 0);
    load(raw[1], 1);
    store(raw[0], 0);  // (past the split: zeros, which an odd count's extra step reads)
    store(raw[1], 1);
    load(raw[0], 2);
    load(raw[1], 3);
    __syncthreads();
    Frag F[2];
    issue(F[0], 0);
    int sr = 1, sw = 2;  // slots read (step s + 1) and written (step s + 2)
    auto step = [&](int s, auto cur_tag) {
        constexpr int C = decltype(cur_tag)::value;
        fwg_wait(F[C]);
        issue(F[C ^ 1], sr);
        mma(F[C]);
        store(raw[C], sw);
        load(raw[C], s + 4);
        sr = sr == 2 ? 0 : sr + 1;
        sw = sw == 2 ? 0 : sw + 1;
        __syncthreads();
    };
    // whole pairs of k-steps (a branch inside the pair merged the two register stages' load counts, and hipcc then
    // waited for every load in flight at each store): an odd count's extra step reads rows past the split, zeros
    for (int s = 0; s < nsteps; s += 2) {
        step(s, std::integral_constant<int, 0>{});
        step(s + 1, std::integral_constant<int, 1>{});
    }
    // the last issued reads (past the end) land before the workgroup exits; >= 18 wait states between the last
    // MFMA writing an accumulator and its read; the statements name every accumulator, so no read is scheduled
    // above the nops
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_nop 7\n\ts_nop 7\n\ts_nop 4"
                 : "+a"(hi[0][0]), "+a"(hi[0][1]), "+a"(hi[1][0]), "+a"(hi[1][1]), "+a"(hi[2][0]), "+a"(hi[2][1]),
                   "+a"(hi[3][0]), "+a"(hi[3][1])
                 :
                 : "memory");
    asm volatile(""
                 : "+a"(lo[0][0]), "+a"(lo[0][1]), "+a"(lo[1][0]), "+a"(lo[1][1]), "+a"(lo[2][0]), "+a"(lo[2][1]),
                   "+a"(lo[3][0]), "+a"(lo[3][1])
                 :
                 : "memory");
    const int px = 2 * fg + wp;
    if (px > 48) return;  // the 25th group's second pixel (wave-uniform)
    const float uo = exp2i(-*a.df_exp) * exp2i(-*a.h3_exp);
    float* slab = a.slab + ((long long)split * 512 + oh * 256 + wo * 128) * 3136 + px * 64;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                slab[(long long)o * 3136 + j * 32 + (lane & 31)] = (hi[i][j][r] + lo[i][j][r]) * uo;
            }
}

// the direct form's split count: 5 (250 workgroups), fewer for batches below ~5 k-steps per split
inline int fcwg_splits(long long batch) {
    return (int)std::max<long long>(1, std::min<long long>(FWG_SPLITS, ppox::ceil_div(batch, 4LL * FWG_KS)));
}

extern "C" int64_t ppox_nature_wgrad_split_workspace_bytes(int32_t layer, int64_t batch) {
    if (batch <= 0) return 0;
    if (layer == 1 && !wgrad1_im2col()) {
        // the direct conv1 weight gradient: two partial slabs per workgroup, one workgroup per CU
        // (grid = min(batch, CUs): more than Ws1's 512-slab floor on a device with > 256 CUs)
        int per;
        long long grid;
        w2p_grid(batch, per, grid);
        return std::max(Ws1::workspace_bytes(batch), 2 * grid * (long long)(G1::K * G1::COUT + G1::COUT) * 4);
    }
    if (layer == 3)  // the im2col split form's slabs, or the direct form's (one per workgroup, PX operands)
        return std::max(Ws3::workspace_bytes(batch),
                        ppox_conv::dwgrad3_grid(batch) * (long long)(G3::K * G3::COUT + G3::COUT) * 4);
    return layer == 1 ? Ws1::workspace_bytes(batch) : layer == 2 ? Ws2::workspace_bytes(batch) : -1;
}

extern "C" int ppox_nature_conv_wgrad_split(int32_t layer, const void* x, int64_t batch, int64_t x_sample_stride,
                                            const float* grad_out, void* workspace, int64_t workspace_bytes, float* dw,
                                            float* db, const uint32_t* amax_x, const uint32_t* amax_g,
                                            const int* x_exp, const int* g_exp, void* stream) {
    PPOX_REQUIRE(layer >= 1 && layer <= 3, "ppox_nature_conv_wgrad_split: layer must be 1, 2 or 3");
    PPOX_REQUIRE(x && grad_out && workspace && dw && db && batch > 0, "ppox_nature_conv_wgrad_split: bad arguments");
    PPOX_REQUIRE((!x_exp && !g_exp) || layer == 3, "ppox_nature_conv_wgrad_split: PX operands are layer 3's (h2, g3)");
    PPOX_REQUIRE((amax_g || g_exp) && (layer == 1 || amax_x || x_exp) && (!amax_g || ppox::aligned16(amax_g)) &&
                     (!amax_x || ppox::aligned16(amax_x)),
                 "ppox_nature_conv_wgrad_split: amax slots of the operands (16B-aligned) required");
    PPOX_REQUIRE(workspace_bytes >= ppox_nature_wgrad_split_workspace_bytes(layer, batch),
                 "ppox_nature_conv_wgrad_split: workspace too small");
    PPOX_REQUIRE(ppox::aligned16(grad_out), "ppox_nature_conv_wgrad_split: grad_out must be 16B aligned");
    PPOX_REQUIRE((layer == 1 && !wgrad1_im2col()) ||
                     batch * (layer == 1 ? G1::P : layer == 2 ? G2::P : G3::P) < (1LL << 31) / 64,
                 "ppox_nature_conv_wgrad_split: batch too large for 32-bit pixel indexing");
    hipStream_t s = ppox::as_stream(stream);
    if (layer == 1) {
        PPOX_REQUIRE(!(reinterpret_cast<uintptr_t>(x) & 3) && x_sample_stride % 4 == 0,
                     "ppox_nature_conv_wgrad_split: u8 input 4-byte aligned");
        if (!wgrad1_im2col())
            return launch_wgrad1_frames(x, x_sample_stride, nullptr, 0, 0, grad_out, batch, workspace, workspace_bytes,
                                        dw, db, amax_g, s);
        return Ws1::run(x, x_sample_stride, grad_out, batch, workspace, dw, db, nullptr, amax_g, s);
    }
    PPOX_REQUIRE(ppox::aligned16(x), "ppox_nature_conv_wgrad_split: layer 2/3 input must be 16B-aligned NHWC");
    if (layer == 2) return Ws2::run(x, 0, grad_out, batch, workspace, dw, db, amax_x, amax_g, s);
    if (x_exp && g_exp && ppox_conv::dwgrad3_enabled(batch)) {  // the direct form (dconv.hip)
        float* slab = reinterpret_cast<float*>(workspace);
        float* bslab = slab + ppox_conv::dwgrad3_grid(batch) * (G3::K * G3::COUT);
        const int rc = ppox_conv::dwgrad3(x, grad_out, batch, x_exp, g_exp, slab, bslab, s);
        if (rc != PPOX_OK) return rc;
        return launch_wgrad_reduce<G3, true>(slab, bslab, (int)ppox_conv::dwgrad3_grid(batch), dw, db, s);
    }
    if (x_exp && g_exp) return Ws3PP::run(x, 0, grad_out, batch, workspace, dw, db, amax_x, amax_g, s, nullptr, 0, 0, x_exp, g_exp);
    if (x_exp) return Ws3PF::run(x, 0, grad_out, batch, workspace, dw, db, amax_x, amax_g, s, nullptr, 0, 0, x_exp, g_exp);
    if (g_exp) return Ws3FP::run(x, 0, grad_out, batch, workspace, dw, db, amax_x, amax_g, s, nullptr, 0, 0, x_exp, g_exp);
    return Ws3::run(x, 0, grad_out, batch, workspace, dw, db, amax_x, amax_g, s);
}

// conv1 split wgrad reading its frames straight from the rollout (sample n = env-major row
// idx[n] of the step-major (T, N_env, 4, 84, 84) buffer): the minibatch gather fused, as in
// ppox_nature_conv_fwd_split's idx form (replaces ppox_gather_rows + the strided call)
extern "C" int ppox_nature_conv_wgrad_split_idx(int32_t layer, const void* x, int64_t batch, const int64_t* idx,
                                                int64_t T, int64_t N_env, const float* grad_out, void* workspace,
                                                int64_t workspace_bytes, float* dw, float* db, const uint32_t* amax_g,
                                                void* stream) {
    PPOX_REQUIRE(layer == 1, "ppox_nature_conv_wgrad_split_idx: layer must be 1 (u8 frames)");
    PPOX_REQUIRE(x && idx && grad_out && workspace && dw && db && batch > 0 && T > 0 && N_env > 0,
                 "ppox_nature_conv_wgrad_split_idx: bad arguments");
    PPOX_REQUIRE(amax_g && ppox::aligned16(amax_g), "ppox_nature_conv_wgrad_split_idx: amax slots of G required");
    PPOX_REQUIRE(workspace_bytes >= ppox_nature_wgrad_split_workspace_bytes(layer, batch),
                 "ppox_nature_conv_wgrad_split_idx: workspace too small");
    PPOX_REQUIRE(ppox::aligned16(grad_out) && !(reinterpret_cast<uintptr_t>(x) & 3),
                 "ppox_nature_conv_wgrad_split_idx: alignment");
    if (!wgrad1_im2col())  // (the direct form indexes in 64 bits)
        return launch_wgrad1_frames(x, 0, reinterpret_cast<const long long*>(idx), T, N_env, grad_out, batch, workspace,
                                    workspace_bytes, dw, db, amax_g, ppox::as_stream(stream));
    PPOX_REQUIRE(batch * G1::P < (1LL << 31) / 64, "ppox_nature_conv_wgrad_split_idx: batch too large");
    return Ws1::run(x, 0, grad_out, batch, workspace, dw, db, nullptr, amax_g, ppox::as_stream(stream),
                    reinterpret_cast<const long long*>(idx), T, N_env);
}

extern "C" int64_t ppox_nature_conv2_wgrad_planes_workspace_bytes(int64_t batch) {
    if (batch <= 0) return 0;
    int per;
    long long grid;
    w2p_grid(batch, per, grid);
    return grid * (long long)(G2::K * G2::COUT + G2::COUT) * (long long)sizeof(float);
}

extern "C" int ppox_nature_conv2_wgrad_planes(const uint16_t* h1p, const uint16_t* q1, int64_t batch,
                                              const float* grad_out, void* workspace, int64_t workspace_bytes,
                                              float* dw, float* db, const uint32_t* amax_g, const int* g_exp,
                                              void* stream) {
    PPOX_REQUIRE(h1p && q1 && grad_out && workspace && dw && db && (amax_g || g_exp) && batch > 0,
                 "ppox_nature_conv2_wgrad_planes: bad arguments");
    PPOX_REQUIRE(ppox::aligned16(h1p) && ppox::aligned16(grad_out) && (!amax_g || ppox::aligned16(amax_g)) &&
                     ppox::aligned16(workspace),
                 "ppox_nature_conv2_wgrad_planes: 16B alignment");
    PPOX_REQUIRE(cu_count() > 0, "ppox_nature_conv2_wgrad_planes: no device");
    PPOX_REQUIRE(workspace_bytes >= ppox_nature_conv2_wgrad_planes_workspace_bytes(batch),
                 "ppox_nature_conv2_wgrad_planes: workspace too small");
    int per;
    long long grid;
    w2p_grid(batch, per, grid);
    float* slab = reinterpret_cast<float*>(workspace);
    W2PArgs wa{h1p, h1p_exp(q1, PL_Q1), grad_out, amax_g, nullptr, slab, slab + grid * (long long)(G2::K * G2::COUT),
               batch, per};
    wa.g_exp = g_exp;
    hipStream_t s = ppox::as_stream(stream);
    if (g_exp)
        wgrad2_planes_kernel<true><<<(unsigned)grid, 512, 0, s>>>(wa);
    else
        wgrad2_planes_kernel<false><<<(unsigned)grid, 512, 0, s>>>(wa);
    PPOX_LAUNCHED_NORET("ppox_nature_conv2_wgrad_planes");
    return launch_wgrad_reduce<G2, true>(slab, wa.bslab, (int)grid, dw, db, s);
}

extern "C" int64_t ppox_nature_fc_wgrad_workspace_bytes(int64_t batch) {
    if (batch <= 0) return 0;
    return std::max<int64_t>(FcWgrad::workspace_bytes(batch), (int64_t)fcwg_splits(batch) * FcWgrad::SLAB * 4);
}

extern "C" int ppox_nature_fc_wgrad(const float* df, int64_t batch, const float* h3, void* workspace,
                                    int64_t workspace_bytes, float* dw, const uint32_t* amax_df,
                                    const uint32_t* amax_h3, const int* h3_exp, const int* df_exp, void* stream) {
    PPOX_REQUIRE(dw && batch >= 0, "ppox_nature_fc_wgrad: bad arguments");
    hipStream_t s = ppox::as_stream(stream);
    if (batch == 0) {  // no rows: a zero gradient
        PPOX_REQUIRE(hipMemsetAsync(dw, 0, sizeof(float) * FcWgrad::SLAB, s) == hipSuccess,
                     "ppox_nature_fc_wgrad: memset failed");
        return PPOX_OK;
    }
    PPOX_REQUIRE(df && h3 && workspace && (amax_df || df_exp) && (amax_h3 || h3_exp), "ppox_nature_fc_wgrad: bad arguments");
    PPOX_REQUIRE((!amax_df || ppox::aligned16(amax_df)) && (!amax_h3 || ppox::aligned16(amax_h3)),
                 "ppox_nature_fc_wgrad: 16B alignment");
    PPOX_REQUIRE(workspace_bytes >= FcWgrad::workspace_bytes(batch), "ppox_nature_fc_wgrad: workspace too small");
    PPOX_REQUIRE(ppox::aligned16(df) && ppox::aligned16(h3), "ppox_nature_fc_wgrad: 16B alignment");
    PPOX_REQUIRE(batch < (1LL << 31) / 64, "ppox_nature_fc_wgrad: batch too large for 32-bit row indexing");
    float* slab = reinterpret_cast<float*>(workspace);
    // PX df and PX h3 (the product's training pass): the direct form (round 6; PPOX_FCWG=0 under PPOX_AB=1: the
    // split wgrad form)
    const char* fe = ppox::ab_env("PPOX_FCWG");
    if (h3_exp && df_exp && !(fe && fe[0] == '0')) {
        const int sp = fcwg_splits(batch);
        FwgArgs fa{reinterpret_cast<const uint8_t*>(df), reinterpret_cast<const uint8_t*>(h3), df_exp, h3_exp, slab,
                   batch, (long long)ppox::ceil_div((long long)batch, (long long)sp)};
        fcwg_kernel<<<(unsigned)(2 * FWG_GROUPS * sp), 256, 0, s>>>(fa);
        PPOX_LAUNCHED_NORET("ppox_nature_fc_wgrad");
        ppox::ktime_mark(s);
        fc_wgrad_reduce_perm<<<512, 256, 0, s>>>(slab, sp, dw);
        PPOX_LAUNCHED("ppox_nature_fc_wgrad");
    }
    const int sp = FcWgrad::splits(batch);
    WArgs wa{df, 0, h3, slab, nullptr, batch, 0, sp, nullptr, 0, 0, amax_df, amax_h3};
    wa.gexp = h3_exp;  // PX h3 (the G operand of this GEMM)
    wa.xexp = df_exp;  // PX df (the X operand)
    wa.px_per_split = ppox::ceil_div(ppox::ceil_div((long long)batch, (long long)sp), (long long)MS) * MS;
    const unsigned g = (unsigned)(FcWgrad::TILES * sp);
    if (h3_exp && df_exp)
        wgrad_split_kernel<GFc, false, FCW_KT, false, FCW_CB, true, true><<<g, 256, 0, s>>>(wa);
    else if (h3_exp)
        wgrad_split_kernel<GFc, false, FCW_KT, false, FCW_CB, false, true><<<g, 256, 0, s>>>(wa);
    else if (df_exp)
        wgrad_split_kernel<GFc, false, FCW_KT, false, FCW_CB, true, false><<<g, 256, 0, s>>>(wa);
    else
        wgrad_split_kernel<GFc, false, FCW_KT, false, FCW_CB><<<g, 256, 0, s>>>(wa);
    PPOX_LAUNCHED_NORET("ppox_nature_fc_wgrad");
    ppox::ktime_mark(s);
    fc_wgrad_reduce_perm<<<512, 256, 0, s>>>(slab, sp, dw);
    PPOX_LAUNCHED("ppox_nature_fc_wgrad");
}

extern "C" int64_t ppox_head_hidden_wgrad_workspace_bytes(int64_t rows) {
    return rows <= 0 ? 0 : HeadWgrad::workspace_bytes(rows);
}

extern "C" int ppox_head_hidden_wgrad(const float* de, int64_t rows, const float* f, void* workspace,
                                      int64_t workspace_bytes, float* dw, const uint32_t* amax_de,
                                      const uint32_t* amax_f, void* stream) {
    PPOX_REQUIRE(dw && rows >= 0, "ppox_head_hidden_wgrad: bad arguments");
    hipStream_t s = ppox::as_stream(stream);
    if (rows == 0) {  // no rows: a zero gradient
        PPOX_REQUIRE(hipMemsetAsync(dw, 0, sizeof(float) * HeadWgrad::SLAB, s) == hipSuccess,
                     "ppox_head_hidden_wgrad: memset failed");
        return PPOX_OK;
    }
    PPOX_REQUIRE(de && f && workspace && amax_de && amax_f, "ppox_head_hidden_wgrad: bad arguments");
    PPOX_REQUIRE(workspace_bytes >= HeadWgrad::workspace_bytes(rows), "ppox_head_hidden_wgrad: workspace too small");
    PPOX_REQUIRE(ppox::aligned16(de) && ppox::aligned16(f) && ppox::aligned16(amax_de) && ppox::aligned16(amax_f),
                 "ppox_head_hidden_wgrad: 16B alignment");
    PPOX_REQUIRE(rows < (1LL << 31) / 64, "ppox_head_hidden_wgrad: too many rows for 32-bit row indexing");
    const int sp = HeadWgrad::splits(rows);
    float* slab = reinterpret_cast<float*>(workspace);
    WArgs wa{de, 0, f, slab, nullptr, rows, 0, sp, nullptr, 0, 0, amax_de, amax_f};
    wa.px_per_split = ppox::ceil_div(ppox::ceil_div((long long)rows, (long long)sp), (long long)MS) * MS;
    wgrad_split_kernel<GFc, false, FCW_KT, false, 512 / 64><<<(unsigned)(HeadWgrad::TILES * sp), 256, 0, s>>>(wa);
    PPOX_LAUNCHED_NORET("ppox_head_hidden_wgrad");
    ppox::ktime_mark(s);
    rows_wgrad_reduce<512, false><<<(unsigned)ppox::ceil_div(HeadWgrad::SLAB, 1024LL), 256, 0, s>>>(slab, sp, dw);
    PPOX_LAUNCHED("ppox_head_hidden_wgrad");
}
