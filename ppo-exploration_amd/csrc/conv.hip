// K6 — the split-f16 GEMM ("sg2", sgemm_kernel) of the NatureCNN trunk and everything instantiated
// from it: the conv2 / conv3 forwards and the conv3 dgrad, the col2im conv2 dgrad
// (dgrad2_colp_kernel), and the forward / split-K / dgrad entry points of the fc layer
// Linear(3136, 512) and of the heads' hidden layer Linear(512, 512)
// (.ipynb_checkpoints/models-checkpoint.py:52-66).
//
// Activation layout: NHWC between layers (a 32-channel run = one 128-byte row segment, so every
// im2col gather is coalesced), as f32 or as PX planes (conv_common.h).  The operand formats (split-f16
// planes, amax slots, PX) are in conv_common.h; the Problems and the packed-B layout in gemm_layout.h.
// The other conv units: conv_f32.hip (the f32 MFMA math mode), wgrad.hip (weight gradients), pack.hip
// (weight packing, amax, PX split), conv_split.hip (the conv1 split forward), dconv.hip (direct forms).
#include <algorithm>

#include "gemm_layout.h"

namespace {

// a Problem with PX operands: A rows as f16 planes (a.xexp; no split in registers) and / or the
// output written as planes at a bound-derived exponent (a.yexp_out, conv_common.h)
template <class Base, bool AP, bool PO = false>
struct Px : Base {
    static constexpr bool A_PLANES = AP, PLANES_OUT = PO;
};

constexpr int FC_FWD_G = 8;  // fc forward: column blocks per tile group (SgRows): all 8, each h3 row tile read once
constexpr int FC_DGRAD_G = 12;  // fc dgrad: column blocks per tile group
// columns per sg2 tile of the fc / head GEMMs: 64; 128 (A staged once per 128 columns, four
// column tiles per wave) measured slower — 358 registers, one wave per SIMD (round 4 same-box
// A/B: 1-GPU 427.4k vs 439.6k env-steps/s, per-rank 225.8 vs 215.5 ms)
constexpr int SG_FC_NB = 64;
// column-block groups of the wide tiles: the same column span per group as the 64-column FC_*_G
constexpr int FC_FWD_GW = FC_FWD_G * 64 / SG_FC_NB, FC_DGRAD_GW = FC_DGRAD_G * 64 / SG_FC_NB;
constexpr int HEAD_GW = 512 / SG_FC_NB;

// ---------------------------------------------------------------------------
// conv2 dgrad in the col2im form (split-f16), the default conv2 split dgrad.
// GEMM rows = output-grad pixels (n, oy, ox), K = the 64 output channels, columns =
// (tap, ci): 16 taps x 32 = 512.  Every A value (one G row of 64 floats) is loaded
// once, split once into its two f16 planes and kept in registers for all 512
// columns — 16x the MFMA work per A byte of the position-major form, whose
// 32-column tiles re-gathered each G row for every one of its 16 input pixels.
// A triple (3 whole samples, 243 rows on 8 waves x 32) keeps the col2im overlap inside
// one workgroup: four passes, one per input-pixel parity class (py, px), each computing
// the class's four taps (ky in {py, py+2}, kx in {px, px+2}) and adding them, in the
// fixed tap order, into an LDS image of the class's 10x10 pixels (tap (ky, kx) sends
// row (oy, ox) to class pixel (oy + ky/2, ox + kx/2)).  The class image is then masked
// with the ReLU of the layer below and written NHWC.  B = the taps' split planes
// (position-major dgrad packing: ppox_nature_pack_split which = 12).  Deterministic: a
// fixed sum order per output.
//
// Persistent: one 512-thread workgroup per CU walks the triples t = blockIdx.x,
// + gridDim.x, ... so nothing is exposed at a triple's start:
//   * B lives in a 4-slot tap ring (tap k in slot k & 3, 12 KB each) refilled two taps at
//     a time at odd steps (taps k+3, k+4 by LDS-DMA), waited one step later;
//   * the NEXT triple's G rows are DMA'd into LDS (64 KB, 16-B chunks XOR-swizzled by row
//     so the boundary's b128 reads are conflict-free) during the current triple and split
//     into the A registers at the boundary;
//   * each class's ReLU-mask operands are loaded a class ahead (at the previous class's
//     output step), and the output stores are unconditional (threads with nothing to store
//     write a dummy), so every wave's vmcnt sequence is static and the waits are counted.
// LDS: 32 KB ring + 64 KB next rows + 37.5 KB class image = 134 KB (one workgroup per CU).
// (0.645 vs 0.695 ms for the one-triple-per-workgroup form at B = 16384, same box.)
// ---------------------------------------------------------------------------
constexpr int C2S = 3, C2ROWS = C2S * 81, C2PIX = 100;
constexpr int C2OV = (C2S * C2PIX * 8 + 511) / 512;  // float4 outputs per thread per pass
constexpr int C2_ROW_DMAS = 8;                       // dmaA: the next triple's G rows, DMAs per thread
constexpr int C2_TAP_DMAS = 2;                       // dmaB2: a tap pair, DMAs per thread
// s_waitcnt immediate (gfx9 encoding) waiting for all but the n youngest vector-memory operations:
// vmcnt bits [3:0] and [15:14], expcnt [6:4] and lgkmcnt [11:8] left at "don't wait"
constexpr int waitcnt_vm(int n) { return (n & 15) | ((n >> 4) << 14) | (0x7 << 4) | (0xF << 8); }
// the class-tap step i = 0 waits for the tap pair DMA'd at the step before (i = 3 of the previous
// class); behind it that step issued the class's C2OV output stores and the next class's C2OV
// mask loads (one memory instruction each: the stores are unconditional, the loads clamped), and
// after class 0 the next triple's row DMAs
constexpr int C2_WAIT_I0 = 2 * C2OV, C2_WAIT_I0_ROWS = 2 * C2OV + C2_ROW_DMAS;
static_assert(waitcnt_vm(0) == 0x0F70 && waitcnt_vm(10) == 0x0F7A && waitcnt_vm(18) == 0x4F72, "s_waitcnt encoding");
static_assert(C2_WAIT_I0_ROWS < 64, "vmcnt is 6 bits");

// workgroup barrier that waits only for this wave's LDS operations: global loads and
// stores stay in flight across it (__syncthreads also drains vmcnt, which would expose
// every output store and prefetch at each col2im step)
__device__ inline void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

constexpr int C2P_TAP = 4 * NPL * 64;                  // u32x4 per tap: 4 k-steps x 2 planes x 64 lanes
constexpr int C2P_AN = 256 * 16;                       // u32x4: 256 G rows x 64 f32
// u32x4: class image + the dummy region (the rows past a triple's 243 land there at any tap offset)
constexpr int C2P_IMG = (C2S * C2PIX * 32 + (11 * 32 + 32)) / 4;
__device__ float4 kC2Dummy[512];                       // store target of threads with nothing to store

__device__ inline int c2_nat_tap(int k) {  // class tap k (0..15) -> natural tap ky * 4 + kx
    k &= 15;
    const int cls = k >> 2, i = k & 3;
    return ((cls >> 1) + 2 * (i >> 1)) * G2::KW + (cls & 1) + 2 * (i & 1);
}

// BITS: the ReLU mask of conv1 from the forward's bitmask (a.bits_mask, 4 B per pixel) instead
// of its f32 activations (a.mask, 128 B per pixel): 26 MB instead of 839 MB at B = 16384
// SAFE: every counted wait is vmcnt(0) (PPOX_COLP_VMCNT0=1; the tests compare both bitwise)
template <bool BITS, bool SAFE = false>
__global__ void __launch_bounds__(512, 1) dgrad2_colp_kernel(Args a, const u32x4* __restrict__ wq,
                                                            long long ntriples) {
    using L = G2;
    __shared__ u32x4 lds[4 * C2P_TAP + C2P_AN + C2P_IMG];
    u32x4* Bring = lds;
    u32x4* An = lds + 4 * C2P_TAP;
    float* Ds = reinterpret_cast<float*>(lds + 4 * C2P_TAP + C2P_AN);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long rows_total = a.batch * L::P;
    const float* g2 = reinterpret_cast<const float*>(a.x);

    // operand scales: G by its tensor's amax, B as packed; the output is unscaled
    const int ex = split_scale_exp(amax_read(a.amax_x)), ew = *a.wexp;
    const float sg = exp2i(ex), uo = exp2i(-ex) * exp2i(-ew);
    float om = 0.f;  // the largest |value| this thread stored (the output's amax)
    // taps k, k+1 (class-tap indices, mod 16) -> ring slots: 2 DMAs per thread
    auto dmaB2 = [&](int k) {
        static_assert(2 * C2P_TAP / 512 == C2_TAP_DMAS, "dmaB2: DMAs per thread");
#pragma unroll
        for (int r = 0; r < C2_TAP_DMAS; ++r) {
            const int e0 = r * 512 + wave * 64, which = e0 / C2P_TAP, within0 = e0 - which * C2P_TAP;
            const int kk = (k + which) & 15;
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void*)(wq + c2_nat_tap(kk) * C2P_TAP + within0 + lane),
                (__attribute__((address_space(3))) void*)(Bring + (kk & 3) * C2P_TAP + within0), 16, 0, 0);
        }
    };
    // triple t's 256 G rows (rows past the batch clamped; rows 243.. are never stored) ->
    // An, row r's 16-B chunk c at position c ^ (r & 15): 8 DMAs per thread
    auto dmaA = [&](long long t) {
        long long row0 = t * C2ROWS;
        row0 = row0 < rows_total ? row0 : rows_total - 1;  // (past the last triple: clamped, never stored)
        // uniform 64-bit base at the triple's first row + 32-bit byte offset (< 64 KB): the saddr
        // form, whose address VGPR hipcc does not make each DMA wait for (vmcnt(0)) before reusing
        const char* base = reinterpret_cast<const char*>(g2) + row0 * 256;
        const long long last = rows_total - 1 - row0;
        static_assert(C2_ROW_DMAS * 512 * 16 == 256 * 256, "dmaA: 256 rows of 256 B per triple");
#pragma unroll
        for (int j = 0; j < C2_ROW_DMAS; ++j) {
            const int r = (wave * 8 + j) * 4 + (lane >> 4), c = (lane & 15) ^ (r & 15);
            const unsigned rr = (unsigned)(r < last ? r : last);
            const unsigned off = rr * 256u + (unsigned)c * 16u;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(base + off),
                                             (__attribute__((address_space(3))) void*)(An + (wave * 8 + j) * 64), 16,
                                             0, 0);
        }
    };
    // A: this lane's row of the triple in An, k = 16q + 8h .. +8 -> two f16 planes (scaled)
    u32x4 af[4][NPL];
    auto take_A = [&]() {
        const int r = wave * 32 + (lane & 31), sw = r & 15;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c0 = (lane >> 5) * 2 + 4 * q;
            const u32x4 v0 = An[r * 16 + (c0 ^ sw)], v1 = An[r * 16 + ((c0 + 1) ^ sw)];
            split8h(__builtin_bit_cast(float4, v0), __builtin_bit_cast(float4, v1), sg, af[q][0], af[q][1]);
        }
    };
    auto mfma_tap = [&](int k, f32x16& c) {
        const u32x4* Bt = Bring + (k & 3) * C2P_TAP + lane;
        c = zero16();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const u32x4 bf[NPL] = {Bt[q * NPL * 64], Bt[q * NPL * 64 + 64]};
            mfma_split3(af[q], bf, c, c);
        }
    };
    // col2im add of tap k into the class image: row (oy, ox) -> class pixel (oy + (i >> 1),
    // ox + (i & 1)); eight reads, then eight writes; rows past the samples -> dummy slot
    // this lane's 16 accumulator rows -> their class-image pixel at tap offset 0 (float index,
    // computed once: a tap adds only its constant offset, folded into the ds instructions);
    // rows past the triple's 243 -> the dummy region
    int dbase[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int rho = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const int s = rho / 81, p = rho - s * 81, oy = p / 9, ox = p - oy * 9;
        dbase[r] = (rho < C2ROWS ? (s * C2PIX + oy * 10 + ox) * 32 : C2S * C2PIX * 32) + (lane & 31);
    }
    auto rmw_tap = [&](auto i_tag, const f32x16& c) {
        constexpr int i = decltype(i_tag)::value;
        constexpr int toff = ((i >> 1) * 10 + (i & 1)) * 32;
#pragma unroll
        for (int r0 = 0; r0 < 16; r0 += 8) {
            float dv[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) dv[r] = Ds[dbase[r0 + r] + toff];
#pragma unroll
            for (int r = 0; r < 8; ++r) Ds[dbase[r0 + r] + toff] = dv[r] + c[r0 + r];
        }
    };
    std::conditional_t<BITS, uint32_t, float4> mk[C2OV];
    auto load_mask = [&](long long n0, int cls) {
        const int py = cls >> 1, px = cls & 1;
#pragma unroll
        for (int j = 0; j < C2OV; ++j) {
            const int e = j * 512 + tid, s = e / 800, rem = e - s * 800, pix = rem >> 3, c4 = rem & 7;
            const long long n = n0 + s;
            const int iy = 2 * (pix / 10) + py, ix = 2 * (pix % 10) + px;
            const bool ok = e < C2S * C2PIX * 8 && n < a.batch;
            const long long p = ok ? (n * L::IH + iy) * L::IW + ix : 0;
            if constexpr (BITS)
                mk[j] = a.bits_mask[p];  // one load either way: the counted vmcnt waits hold
            else
                mk[j] = *reinterpret_cast<const float4*>(a.mask + p * L::CIN + c4 * 4);
        }
    };
    // the image is read and re-zeroed with inline-asm LDS ops: a C++ access here, after the
    // step's tap DMAs, makes hipcc wait vmcnt(0) first (it cannot tell the two LDS regions apart)
    const uint32_t img0 = (uint32_t)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) float*)Ds);
    auto output = [&](long long n0, int cls) {
        const int py = cls >> 1, px = cls & 1;
        const u32x4 zero4 = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < C2OV; ++j) {
            const int e = j * 512 + tid, s = e / 800, rem = e - s * 800, pix = rem >> 3, c4 = rem & 7;
            const bool in = e < C2S * C2PIX * 8;
            const uint32_t da = img0 + (uint32_t)(in ? e : C2S * C2PIX * 8) * 16u;
            u32x4 dr;
            asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)\n\tds_write_b128 %1, %2"
                         : "=&v"(dr) : "v"(da), "v"(zero4) : "memory");
            const float4 d = __builtin_bit_cast(float4, dr);
            bool on[4];
            if constexpr (BITS) {
                const uint32_t w = mk[j] >> (c4 * 4);
                on[0] = w & 1u, on[1] = w & 2u, on[2] = w & 4u, on[3] = w & 8u;
            } else {
                on[0] = mk[j].x > 0.f, on[1] = mk[j].y > 0.f, on[2] = mk[j].z > 0.f, on[3] = mk[j].w > 0.f;
            }
            const float4 y = make_float4(on[0] ? d.x * uo : 0.f, on[1] ? d.y * uo : 0.f, on[2] ? d.z * uo : 0.f,
                                         on[3] ? d.w * uo : 0.f);
            const long long n = n0 + s;
            const float ym = fmaxf(fmaxf(fabsf(y.x), fabsf(y.y)), fmaxf(fabsf(y.z), fabsf(y.w)));
            om = (in && n < a.batch) ? fmaxf(om, ym) : om;  // the dummy slot's sums are not output
            const int iy = 2 * (pix / 10) + py, ix = 2 * (pix % 10) + px;
            float4* dst = (in && n < a.batch)
                              ? reinterpret_cast<float4*>(a.y + ((n * L::IH + iy) * L::IW + ix) * L::CIN + c4 * 4)
                              : kC2Dummy + tid;
            *dst = y;
        }
    };

    long long t = blockIdx.x;
    // prologue: the first triple's rows, taps 0..3, class 0's mask operands, a zero image
    dmaA(t);
    dmaB2(0);
    dmaB2(2);
    load_mask(t * C2S, 0);
    for (int e = tid; e < C2S * C2PIX * 8; e += 512) reinterpret_cast<float4*>(Ds)[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));  // the builtin, so hipcc's own wait bookkeeping sees it
    lds_barrier();
    take_A();
    lds_barrier();  // An free for the next triple's rows

    // one class-tap step (i = k & 3 at compile time): tap k+1's MFMAs beside tap k's col2im
    // adds.  vmcnt bookkeeping per wave (every count static: stores unconditional, loads
    // clamped): i = 1, 3 DMA the tap pair k+3, k+4; i = 3 then stores the class, loads the
    // next class's mask operands and (class 0) DMAs the next triple's rows; i = 0 waits for
    // the pair of the step before (behind it: 5 stores + 5 mask loads (+ 8 row DMAs after
    // class 0) = vmcnt(10) / vmcnt(18)); i = 2 drains everything (vmcnt(0)).
    auto step = [&](long long tt, int cls, auto i_tag, f32x16& next, const f32x16& cur) {
        constexpr int i = decltype(i_tag)::value;
        const int k = 4 * cls + i;
        const long long n0 = tt * C2S;
        if constexpr (i & 1) dmaB2(k + 3);  // taps k+3, k+4 (mod 16) into the slots of k-1, k
        if (i < 3 || cls < 3) mfma_tap(k + 1, next);
        rmw_tap(i_tag, cur);
        if constexpr (i == 0) {
            if (SAFE)
                __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
            else if (cls == 1)
                __builtin_amdgcn_s_waitcnt(waitcnt_vm(C2_WAIT_I0_ROWS));  // + class 0's row DMAs
            else
                __builtin_amdgcn_s_waitcnt(waitcnt_vm(C2_WAIT_I0));
        }
        if constexpr (i == 2) __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
        lds_barrier();
        if constexpr (i == 3) {
            output(n0, cls);
            // one load path (two paths would merge into register copies that wait vmcnt(0))
            load_mask(cls < 3 ? n0 : (tt + gridDim.x) * C2S, (cls + 1) & 3);
            if (cls == 0) dmaA(tt + gridDim.x);  // the next triple's rows (clamped past the end)
            lds_barrier();
        }
    };
    f32x16 acc0, acc1;
#pragma unroll 1
    for (; t < ntriples; t += gridDim.x) {
        mfma_tap(0, acc0);
#pragma unroll 1
        for (int cls = 0; cls < 4; ++cls) {
            step(t, cls, std::integral_constant<int, 0>{}, acc1, acc0);
            step(t, cls, std::integral_constant<int, 1>{}, acc0, acc1);
            step(t, cls, std::integral_constant<int, 2>{}, acc1, acc0);
            step(t, cls, std::integral_constant<int, 3>{}, acc0, acc1);
        }
        take_A();  // the next triple's rows (drained at class 1's i = 2, ordered by the barriers since)
        lds_barrier();
    }
    amax_record(a.amax_y, om);
}


// ---------------------------------------------------------------------------
// Split-f16 GEMM, LDS-DMA pipelined ("sg2"): the forward-style GEMMs (conv2/conv3
// forward, conv3 dgrad, fc forward, fc dgrad) with the Problems' fused epilogues (bias +
// ReLU, ReLU-mask, NHWC / Flatten order).  512-thread workgroups (8 waves, two per SIMD, one workgroup per
// CU), 256 rows x 64 columns per workgroup, each wave 32 rows x 64 columns (hi/lo f32
// accumulators for two 32x32 tiles: three v_mfma_f32_32x32x16_f16 per tile and 16-k step).
// Per 32-k chunk the A rows (f32, im2col-gathered: one 128-B run per row) and the
// pre-split B chunk (12 KB, split_frag_index order) are copied global -> LDS by
// global_load_lds_dwordx4 into a three-slot ring, so no VGPR staging and no ds_write:
//   * each wave DMAs exactly its own 32 A rows (4 x 1 KB), so A needs no cross-wave
//     ordering, only the wave's own counted vmcnt;
//   * B is shared: waves 0-3 DMA two 1 KB pieces, waves 4-7 one;
//   * K loop: wait for this wave's DMAs of chunk c (vmcnt = the DMAs of chunk c+1 still
//     allowed in flight), one raw s_barrier (everyone's B of chunk c has landed; everyone
//     has finished reading chunk c-1), DMA chunk c+2 into the slot chunk c-1 used, then
//     split A in registers and run the 24 MFMAs of chunk c.  No ordinary global load is in
//     flight in the loop (hipcc would wait vmcnt(0) on it): the epilogue operands are
//     loaded after it.
// A rows are 128 B in LDS with their 16-B pieces XOR-swizzled by (row >> 1) & 7, which
// makes every ds_read_b128 of the fragments conflict-free (rows 0-3 / 12-15 / 20-27 of a
// lane group land on distinct bank quads); the DMA writes LDS lane-linearly, so the
// swizzle is applied to each lane's GLOBAL source address.
// ---------------------------------------------------------------------------
constexpr int SG_BQ = 2 * 2 * NPL * 64;  // u32x4 per B chunk at 64 columns (8 KB)
constexpr int SG_BP = SG_BQ / 64;        // its 1 KB DMA pieces

// LDS fragment reads in inline asm: hipcc's wait insertion cannot tell a ds_read from the
// ring slot being read apart from the DMAs in flight into the other slots, and puts a
// vmcnt(0) before the first read of every chunk (which would drain the prefetch).  Issued
// here, the reads are ordered by the kernel's own counted vmcnt + barrier, and their data
// by an lgkmcnt wait that takes the destination registers as operands (so no use of them
// can be scheduled above it).
__device__ inline u32x4 sg_ds_read(uint32_t addr) {
    u32x4 r;
    asm volatile("ds_read_b128 %0, %1" : "=v"(r) : "v"(addr));
    return r;
}
template <int N>
__device__ inline void sg_lgkm_wait(u32x4 (&v)[6]) {
    asm volatile("s_waitcnt lgkmcnt(%6)"
                 : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5])
                 : "n"(N));
}
template <int N>
__device__ inline void sg_lgkm_wait(u32x4 (&v)[10]) {
    asm volatile("s_waitcnt lgkmcnt(%10)"
                 : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]),
                   "+v"(v[8]), "+v"(v[9])
                 : "n"(N));
}
template <int N>
__device__ inline void sg_vm_wait() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// WAVES waves x 32 rows per workgroup, SLOTS ring slots of one 32-k chunk (A: 128 B per row;
// B: 8 KB per 64 columns).  8 waves / 3 slots: one workgroup per CU, waves 4-7 staggered; 4 waves / 2 slots:
// two workgroups per CU (48 KB each), whose K walks, prologues and epilogues interleave on
// every SIMD.  A is split in registers with its tensor's scale (a.amax_x), B was packed with
// its own (a.wexp); the epilogue unscales, and records the output's amax (a.amax_y).
// Prob::NOUT = 128 (round 4, the fc layer and the heads' hidden layer: "wide" tiles): each wave
// runs 32 rows x 128 columns, the A fragments of a k-step feeding four column tiles, so A is
// staged once per 128 output columns instead of once per 64; B is two consecutive 64-column
// packed blocks (Prob::bchunk_blk), 16 KB per chunk.
template <class Prob, int WAVES, int SLOTS>
__global__ void __launch_bounds__(64 * WAVES, 8 / WAVES) sgemm_kernel(Args a, const u32x4* __restrict__ wq) {
    constexpr int NT = Prob::NOUT / 32, NBLK = NT / 2;  // column tiles; 64-column packed B blocks
    constexpr int ROWS = 32 * WAVES, AB = ROWS * BK * 4, SLOT = AB + NBLK * SG_BQ * 16;
    constexpr int BP = NBLK * SG_BP;                 // B pieces of a chunk (1 KB each)
    constexpr int BPW = (BP + WAVES - 1) / WAVES;    // B pieces DMA'd per wave
    constexpr int NDMA = 4 + BPW;                  // this wave's DMAs per chunk
    constexpr int NF = 2 + NT * NPL;                 // fragment reads per k-step
    constexpr bool STAGGER = WAVES == 8;
    static_assert((Prob::NOUT == 64 || (Prob::NOUT == 128 && !STAGGER)) && Prob::ROWS == ROWS,
                  "sg2: 32 rows per wave x 64 or 128 columns");
    static_assert(NF <= 15, "lgkmcnt is 4 bits");
    static_assert(SLOTS == 2 || SLOTS == 3, "sg2: two or three ring slots");
    // all LDS in ONE __shared__ object (a second one can make hipcc wait vmcnt(0) in the loop)
    __shared__ __attribute__((aligned(16))) uint8_t lds[SLOTS * SLOT];
    typename Prob::Tile t;
    if (!Prob::tile(a, t)) return;
    const int nchunk = Prob::nchunk(t);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // uniform: DMA bases go to M0

    // DMA sources: A instruction j of this wave covers its rows 8j + (lane >> 3), LDS piece
    // lane & 7, which holds global piece (lane & 7) ^ swz(row)
    const uint8_t* asrc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = 8 * j + (lane >> 3);
        asrc[j] = reinterpret_cast<const uint8_t*>(Prob::row_ptr(a, t, wave * 32 + r)) +
                  ((((lane & 7) ^ ((r >> 1) & 7))) << 4);
    }
    // B: BP pieces of 1 KB per chunk, BPW per wave (pieces past the last re-copy it: the
    // same bytes to the same place), so every wave issues NDMA DMAs per chunk; piece pc is piece
    // pc % SG_BP of the chunk of 64-column block pc / SG_BP
    int bp[BPW];
#pragma unroll
    for (int i = 0; i < BPW; ++i) bp[i] = min(BPW * wave + i, BP - 1);
    // operand scales: A by its tensor's amax (H1P planes: their exponent), B as packed; the epilogue
    // multiplies by both inverses
    const int ex = Prob::A_PLANES ? *a.xexp : split_scale_exp(amax_read(a.amax_x)), ew = *a.wexp;
    const float sa = exp2i(ex), ua = exp2i(-ex), uw = exp2i(-ew);
    // PX output: its exponent from the bound amax(x) * max column norm + max |bias| (every workgroup
    // derives the same; workgroup 0 publishes it).  A non-finite bound makes the output NaN (loud).
    float sy = 1.f;
    if constexpr (Prob::PLANES_OUT) {
        const uint32_t am = amax_read(a.amax_x), nm = amax_read(a.ynorm), bm = *a.ybias;
        const int ey = bound_exp(am, nm, bm);
        const float bnd = __uint_as_float(am) * __uint_as_float(nm) + __uint_as_float(bm);
        sy = __builtin_isfinite(bnd) ? exp2i(ey) : __builtin_nanf("");
        if (blockIdx.x == 0 && threadIdx.x == 0) *a.yexp_out = ey;
    }
    // chunk c into ring slot S; the chunk index is clamped, not branched on (past the end:
    // the last chunk again, never read)
    auto issue = [&](int c, auto S) {
        constexpr int slot = decltype(S)::value;
        c = c < nchunk ? c : nchunk - 1;
        uint8_t* base = lds + slot * SLOT;
        const long long off = (long long)Prob::chunk_off(t, c) * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void*)(asrc[j] + off),
                (__attribute__((address_space(3))) void*)(base + (wave * 32 + 8 * j) * 128), 16, 0, 0);
        if constexpr (NBLK == 1) {
            const u32x4* bsrc = wq + (long long)Prob::bchunk_id(t, c) * SG_BQ + lane;
#pragma unroll
            for (int i = 0; i < BPW; ++i)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bsrc + bp[i] * 64),
                                                 (__attribute__((address_space(3))) void*)(base + AB + bp[i] * 1024),
                                                 16, 0, 0);
        } else {
#pragma unroll
            for (int i = 0; i < BPW; ++i) {
                const u32x4* bsrc = wq + (long long)Prob::bchunk_blk(t, c, bp[i] / SG_BP) * SG_BQ + lane;
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void*)(bsrc + (bp[i] % SG_BP) * 64),
                    (__attribute__((address_space(3))) void*)(base + AB + bp[i] * 1024), 16, 0, 0);
            }
        }
    };

    f32x16 hi[NT], lo[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) hi[j] = lo[j] = zero16();
    const int r = lane & 31, h = lane >> 5, sw = (r >> 1) & 7;
    const uint32_t lds0 = (uint32_t)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) uint8_t*)lds);
    const uint32_t a_lane = lds0 + (wave * 32 + r) * 128, b_lane = lds0 + AB + lane * 16;
    // Stagger (8 waves: the two waves of a SIMD out of phase): waves 4-7 defer each chunk's
    // second k-step MFMAs past the next barrier, so right after a barrier one wave of every
    // SIMD runs matrix work (the deferred k-step) while its partner reads and splits (VALU).
    // The deferred k-step's operands (split A planes + B fragments) stay in registers.
    const bool late = STAGGER && wave >= 4;
    u32x4 daf[NPL], dbf[NT * NPL];
    auto mfma3 = [&](const u32x4 (&af)[NPL], const u32x4* bf) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const u32x4 b2[NPL] = {bf[NPL * j], bf[NPL * j + 1]};
            mfma_split3(af, b2, hi[j], lo[j]);
        }
    };
    auto split_a = [&](const u32x4 (&g)[NF], u32x4 (&af)[NPL]) {
        if constexpr (Prob::A_PLANES) {  // H1P: the two pieces read are the planes
            af[0] = g[0];
            af[1] = g[1];
        } else {
            split8h(__builtin_bit_cast(float4, g[0]), __builtin_bit_cast(float4, g[1]), sa, af[0], af[1]);
        }
    };
    // chunk in slot S: 2 NF fragment reads up front (k-step 0's NF, then k-step 1's), k-step 0
    // computed once its NF have landed (lgkmcnt(NF)) while k-step 1's are in flight
    auto compute = [&](auto S) {
        constexpr int slot = decltype(S)::value;
        u32x4 f[2][NF];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            // the lane's 8 k of k-step s: f32 pieces g0, g0 + 1 (16 B = 4 values each), or H1P
            // pieces 2s + h (hi plane: 8 f16) and 4 + 2s + h (lo plane)
            const int g0 = Prob::A_PLANES ? 2 * s + h : 4 * s + 2 * h, g1 = Prob::A_PLANES ? 4 + g0 : g0 + 1;
            f[s][0] = sg_ds_read(a_lane + slot * SLOT + ((g0 ^ sw) << 4));
            f[s][1] = sg_ds_read(a_lane + slot * SLOT + ((g1 ^ sw) << 4));
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int p = 0; p < NPL; ++p)
                    // column tile j: tile j & 1 of 64-column block j >> 1 (split_frag_index: [s][j][p][lane])
                    f[s][2 + NPL * j + p] = sg_ds_read(b_lane + slot * SLOT + (j >> 1) * (SG_BQ * 16) +
                                                       (((s * 2 + (j & 1)) * NPL + p) * 64) * 16);
        }
        u32x4 af[NPL];
        sg_lgkm_wait<NF>(f[0]);
        split_a(f[0], af);
        mfma3(af, f[0] + 2);
        sg_lgkm_wait<0>(f[1]);
        if (late) {  // k-step 1 split now, multiplied after the next barrier
            split_a(f[1], daf);
#pragma unroll
            for (int i = 0; i < NT * NPL; ++i) dbf[i] = f[1][2 + i];
        } else {
            split_a(f[1], af);
            mfma3(af, f[1] + 2);
        }
    };
    // one pipeline step: this wave's DMAs of chunk c waited for (those of the next SLOTS - 2
    // chunks may stay in flight: the clamped re-issues past the end count too, so the count is
    // the same in every step), one barrier (every wave's DMAs of chunk c landed, every wave done
    // with chunk c - 1), chunk c + SLOTS - 1 issued into the slot chunk c - 1 used, chunk c computed
    auto step = [&](int c, auto S, auto S2) {
        sg_vm_wait<NDMA * (SLOTS - 2)>();
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        issue(c + SLOTS - 1, S2);
        if (late && c > 0) mfma3(daf, dbf);  // chunk c - 1's deferred k-step
        compute(S);
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    issue(0, I0{});
    if constexpr (SLOTS == 3) {
        issue(1, I1{});
#pragma unroll 1
        for (int c = 0; c < nchunk; c += 3) {
            step(c, I0{}, I2{});
            if (c + 1 < nchunk) step(c + 1, I1{}, I0{});
            if (c + 2 < nchunk) step(c + 2, I2{}, I1{});
        }
    } else {
#pragma unroll 1
        for (int c = 0; c < nchunk; c += 2) {
            step(c, I0{}, I1{});
            if (c + 1 < nchunk) step(c + 1, I1{}, I0{});
        }
    }
    if (late && nchunk > 0) mfma3(daf, dbf);
    sg_vm_wait<0>();  // the clamped tail DMAs, before the LDS is released
    // epilogue, per column tile: its operand loads first (all issued before its first store);
    // om = the largest |value| this lane stored.  BITS_OUT: the ReLU bitmask word of tile row L and
    // column tile j is half (L >> 2) & 1 of the ballot of element q = (L & 3) + 4 (L >> 3) — lane L
    // (< 32) collects both words of its row and stores them together
    float om = 0.f;
    uint32_t bw[NT];
    const int qL = (lane & 3) + 4 * ((lane >> 3) & 3), hL = (lane >> 2) & 1;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        bw[j] = 0u;
        decltype(Prob::prefetch(a, t, 0, 0)) e[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) e[q] = Prob::prefetch(a, t, wave * 32 + (q & 3) + 8 * (q >> 2) + 4 * h, j * 32 + r);
        // one wait for all of them (a real s_waitcnt the compiler tracks): the row-bounded
        // stores below are branches, and a load pending at a branch makes hipcc wait vmcnt(0)
        // inside every one of them — behind every earlier store
        __builtin_amdgcn_s_waitcnt(0);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int row = wave * 32 + (q & 3) + 8 * (q >> 2) + 4 * h, col = j * 32 + r;
            float v;
            if constexpr (Prob::PLANES_OUT) {
                // every lane runs the pair swap; the pair (col & ~1, col | 1) shares its row, so both
                // lanes store or neither does
                v = Prob::value(a, t, row, col, (hi[j][q] + lo[j][q]) * ua * uw, e[q]);
                const uint32_t w = px_pair_word(v, sy, lane & 1);
                const long long el = Prob::out_elem(a, t, row, col & ~1);
                if (el >= 0) *reinterpret_cast<uint32_t*>(reinterpret_cast<uint16_t*>(a.y) + px_index(el) + 32 * (lane & 1)) = w;
            } else {
                v = Prob::store_pre(a, t, row, col, (hi[j][q] + lo[j][q]) * ua * uw, e[q]);
            }
            om = fmaxf(om, fabsf(v));
            if constexpr (Prob::BITS_OUT) {
                if (a.bits_y) {  // uniform
                    const unsigned long long b = __ballot(v > 0.f);
                    bw[j] = qL == q ? (uint32_t)(hL ? b >> 32 : b) : bw[j];
                }
            }
        }
    }
    if constexpr (Prob::BITS_OUT) {
        static_assert(NT == 2, "bitmask: 64 channels = two words per pixel");
        const long long m = t.m0 + wave * 32 + lane;
        if (a.bits_y && lane < 32 && m < t.M) *reinterpret_cast<uint2*>(a.bits_y + m * 2) = make_uint2(bw[0], bw[1]);
    }
    amax_record(a.amax_y, om);
}

constexpr int SG_WAVES = 4;  // 4: two 128-row workgroups per CU (2 ring slots); 8: one 256-row workgroup (3 slots)
// ring slots (chunks in flight + 1) per Problem (Prob::SLOTS): 3 for the plain fc / head GEMMs
// (their DMA latency was exposed with one chunk of lookahead: fc forward 0.190 -> 0.174 ms,
// dgrad 0.255 -> 0.238), 2 for the conv forms (3 measured slower for the conv3 dgrad, 0.31 ->
// 0.34 ms); 3 x 24 KB per workgroup keeps two workgroups per CU.
constexpr int SG_ROWS = 32 * SG_WAVES;
constexpr int SG_FWD2_PARITY = 1;  // conv2 forward taps in input-parity classes (SgFwd)

template <class Prob>
int launch_sgemm(const Args& a, const uint16_t* wq, long long blocks, hipStream_t s, const char* name) {
    if (blocks == 0) return PPOX_OK;
    constexpr int slots = SG_WAVES == 8 ? 3 : Prob::SLOTS;
    sgemm_kernel<Prob, SG_WAVES, slots><<<(unsigned)blocks, 64 * SG_WAVES, 0, s>>>(
        a, reinterpret_cast<const u32x4*>(wq));
    PPOX_LAUNCHED(name);
}

// sg2 Problems: the f32 Problems' chunk walk and epilogues on SG_ROWS-row tiles, plus
// each row's A base pointer (rows past the end clamped to a valid row, never stored) and
// the chunk's element offset within a row (the same for every row of the tile)
template <class L, bool OUT_NCHW>
struct SgFwd : FwdBase<L, OUT_NCHW, 1> {
    static constexpr int ROWS = SG_ROWS, CPT = L::CIN / BK;
    static constexpr bool BITS_OUT = true;  // a.bits_y: the output's ReLU bitmask (2 words per pixel)
    static constexpr int SLOTS = 2;
    __device__ static bool tile(const Args& a, RowTile& t) {
        t.m0 = xcd_remap(blockIdx.x, gridDim.x) * ROWS;
        t.M = a.batch * L::P;
        return true;
    }
    __device__ static const float* row_ptr(const Args& a, const RowTile& t, int row) {
        long long m = t.m0 + row;
        m = m < t.M ? m : t.M - 1;
        const long long n = m / L::P;
        const int p = (int)(m - n * L::P), oy = p / L::OW, ox = p % L::OW;
        return reinterpret_cast<const float*>(a.x) + ((n * L::IH + oy * L::S) * L::IW + ox * L::S) * L::CIN;
    }
    // conv2 (4x4 taps, stride 2, one chunk per tap): the taps walked in input-parity classes —
    // (ky, kx), (ky, kx + 2), (ky + 2, kx), (ky + 2, kx + 2) read the same input pixels (one output
    // column / row apart), so a class taken consecutively keeps a quarter of the tile's input
    // live in L2 instead of all of it for half the K walk
    static constexpr bool PARITY = SG_FWD2_PARITY && L::S == 2 && L::KH == 4 && L::KW == 4 && CPT == 1;
    __device__ static int tap_of(int c) {
        if constexpr (PARITY) {
            const int cls = c >> 2, i = c & 3;
            return ((cls >> 1) + 2 * (i >> 1)) * 4 + (cls & 1) + 2 * (i & 1);
        } else {
            return c / CPT;
        }
    }
    __device__ static int chunk_off(const RowTile&, int c) {
        const int tap = tap_of(c);
        return ((tap / L::KW) * L::IW + tap % L::KW) * L::CIN + (c % CPT) * BK;
    }
    __device__ static int bchunk_id(const RowTile&, int c) { return PARITY ? tap_of(c) : c; }
};

// the conv2 forward on H1P input (conv1's output as f16 planes): a pixel's 128 B are its 32 hi then
// 32 lo f16 instead of 32 f32, so the DMA addressing is unchanged and the k-step's two pieces are
// the fragments' planes (no split in registers)
struct SgFwd2P : SgFwd<G2, false> {
    static constexpr bool A_PLANES = true;
};

// BITS_IN: the ReLU mask of the layer below from its forward's bitmask (a.bits_mask, CIN / 32
// words per pixel) instead of its f32 activations
template <class L, bool BITS_IN = false>
struct SgDgradPM : DgradPMBase<L, 1> {
    using Base = DgradPMBase<L, 1>;
    static constexpr int ROWS = SG_ROWS, NPOS = Base::NPOS, CPT = Base::CPT;
    static constexpr bool BITS_OUT = false;
    static constexpr int SLOTS = 2;
    __device__ static float prefetch(const Args& a, const PixelTile& t, int row, int ci) {
        if constexpr (!BITS_IN) {
            return Base::prefetch(a, t, row, ci);
        } else {
            long long n = t.n0 + row;
            n = n < a.batch ? n : t.n0;
            const uint32_t w = a.bits_mask[(n * NPOS + t.pos) * (L::CIN / 32) + (ci >> 5)];
            return (float)((w >> (ci & 31)) & 1u);
        }
    }
    __device__ static bool tile(const Args& a, PixelTile& t) {
        const long long w = xcd_remap(blockIdx.x, gridDim.x);
        t.n0 = (w / NPOS) * ROWS;
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
    __device__ static const float* row_ptr(const Args& a, const PixelTile& t, int row) {
        long long n = t.n0 + row;
        n = n < a.batch ? n : a.batch - 1;
        return reinterpret_cast<const float*>(a.x) + n * (L::P * L::COUT);
    }
    __device__ static int chunk_off(const PixelTile& t, int c) {
        const int tap = c / CPT, ty = tap / t.nx, tx = tap - ty * t.nx;
        const int oy = (t.iy - t.ky0) / L::S - ty, ox = (t.ix - t.kx0) / L::S - tx;
        return (oy * L::OW + ox) * L::COUT + (c % CPT) * BK;
    }
};

// Tile order: column-block groups of G outermost, then row tiles, then the G column blocks of
// the group — so the workgroups an XCD runs together share one A row tile, and one group's B
// (G x 196 KB / 1.2 MB for the dgrad / forward) stays in that XCD's L2 while its row tiles
// stream past (A is read NCB / G times, B about once per XCD).
// BITS_IN (FC_DGRAD): h3's ReLU mask from the conv3 forward's bitmask (N / 32 words per row)
template <int K, int N, int MODE, int G, bool BITS_IN = false, int NB = 64>
struct SgRows : GemmRowsProblem<K, N, NB, MODE> {
    using Base = GemmRowsProblem<K, N, NB, MODE>;
    static constexpr int ROWS = SG_ROWS, NCB = Base::NCB;
    static constexpr bool BITS_OUT = false;
    static constexpr int SLOTS = 3;
    __device__ static auto prefetch(const Args& a, const GemmTile& t, int row, int col) {
        if constexpr (!BITS_IN) {
            return Base::prefetch(a, t, row, col);
        } else {
            static_assert(MODE == FC_DGRAD && N % 32 == 0, "bitmask: the fc dgrad's h3 mask");
            const int n = t.cb * NB + col, nc = n < N ? n : N - 1;
            long long m = t.m0 + row;
            m = m < t.M ? m : t.m0;
            const uint32_t w = a.bits_mask[m * (N / 32) + (nc >> 5)];
            return (float)((w >> (nc & 31)) & 1u);
        }
    }
    __device__ static bool tile(const Args& a, GemmTile& t) {
        const long long w = xcd_remap(blockIdx.x, gridDim.x);
        const long long rt = (a.batch + ROWS - 1) / ROWS;      // row tiles
        const long long grp = w / (rt * G), in = w - grp * rt * G;
        const int g0 = (int)grp * G, gn = NCB - g0 < G ? NCB - g0 : G;  // the last group may be narrower
        t.m0 = (in / gn) * ROWS;
        t.cb = g0 + (int)(in % gn);
        t.M = a.batch;
        return true;
    }
    __device__ static const float* row_ptr(const Args& a, const GemmTile& t, int row) {
        long long m = t.m0 + row;
        m = m < t.M ? m : t.M - 1;
        return reinterpret_cast<const float*>(a.x) + m * K;
    }
    __device__ static int chunk_off(const GemmTile&, int c) { return c * BK; }
};

// fc forward split over K for small batches (128-row tiles x 8 column blocks leave most CUs
// idle below ~8192 rows): S K-ranges per (row tile, column block), each workgroup's partial
// product stored to slab[ks][row][512]; fc_fwd_sk_reduce adds the S partials in order, then
// the bias, then the ReLU.
template <int K, int N, int S>
struct SgRowsSK : GemmRowsProblem<K, N, 64, FC_FWD> {
    using Base = GemmRowsProblem<K, N, 64, FC_FWD>;
    static constexpr int ROWS = SG_ROWS, NCB = Base::NCB, KC = Base::KC;
    static constexpr bool BITS_OUT = false;
    static constexpr int SLOTS = 3;
    struct Tile {
        long long m0, M;
        int cb, ks, c0, nc;
    };
    __device__ static bool tile(const Args& a, Tile& t) {
        const long long w = xcd_remap(blockIdx.x, gridDim.x);  // a row tile's S x 8 workgroups share an XCD
        t.cb = (int)(w % NCB);
        const long long r = w / NCB;
        t.ks = (int)(r % S);
        t.m0 = (r / S) * ROWS;
        t.M = a.batch;
        t.c0 = t.ks * KC / S;
        t.nc = (t.ks + 1) * KC / S - t.c0;
        return true;
    }
    __device__ static int nchunk(const Tile& t) { return t.nc; }
    __device__ static int bchunk_id(const Tile& t, int c) { return t.cb * KC + t.c0 + c; }
    __device__ static const float* row_ptr(const Args& a, const Tile& t, int row) {
        long long m = t.m0 + row;
        m = m < t.M ? m : t.M - 1;
        return reinterpret_cast<const float*>(a.x) + m * K;
    }
    __device__ static int chunk_off(const Tile& t, int c) { return (t.c0 + c) * BK; }
    __device__ static float prefetch(const Args&, const Tile&, int, int) { return 0.f; }
    __device__ static float store_pre(const Args& a, const Tile& t, int row, int col, float acc, float) {
        const long long m = t.m0 + row;
        if (m >= t.M) return 0.f;
        a.y[((long long)t.ks * t.M + m) * N + t.cb * 64 + col] = acc;
        return acc;
    }
};

// am (nullable): f's amax slots (the heads' split hidden layer reads f)
template <int N, int S>
__global__ void __launch_bounds__(256) fc_fwd_sk_reduce(const float4* __restrict__ slab, long long M,
                                                         const float* __restrict__ bias, float4* __restrict__ y,
                                                         uint32_t* __restrict__ am) {
    const long long i = blockIdx.x * 256LL + threadIdx.x, n4 = M * N / 4;
    float m = 0.f;
    if (i < n4) {
        float4 s = slab[i];
#pragma unroll
        for (int k = 1; k < S; ++k) {
            const float4 v = slab[k * n4 + i];
            s.x += v.x;
            s.y += v.y;
            s.z += v.z;
            s.w += v.w;
        }
        const int n = (int)((i * 4) % N);
        const float4 o = make_float4(fmaxf(s.x + bias[n], 0.f), fmaxf(s.y + bias[n + 1], 0.f),
                                     fmaxf(s.z + bias[n + 2], 0.f), fmaxf(s.w + bias[n + 3], 0.f));
        y[i] = o;
        m = fmaxf(fmaxf(o.x, o.y), fmaxf(o.z, o.w));
    }
    amax_record(am, m);
}

// the same reduce with the actor head fused (ppox_skinny_linear's arithmetic on the finished row,
// bitwise the same logits): one wave per row, lane l owns columns 4l .. 4l + 3 and 256 + 4l .. of
// the 512 (the skinny kernel's k order), the NO dot products wave-reduced in its butterfly order
template <int S, int NO>
__global__ void __launch_bounds__(256) fc_fwd_sk_reduce_actor(const float4* __restrict__ slab, long long M,
                                                               const float* __restrict__ bias, float4* __restrict__ y,
                                                               uint32_t* __restrict__ am, const float* __restrict__ wa,
                                                               const float* __restrict__ ba, float* __restrict__ logits) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    float m = 0.f;
    if (b < M) {  // wave-uniform
        const long long n4 = M * 128;
        float acc[NO];
#pragma unroll
        for (int o = 0; o < NO; ++o) acc[o] = 0.f;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int c4 = lane + 64 * half;
            const long long i = b * 128 + c4;
            float4 s = slab[i];
#pragma unroll
            for (int k = 1; k < S; ++k) {
                const float4 v = slab[k * n4 + i];
                s.x += v.x;
                s.y += v.y;
                s.z += v.z;
                s.w += v.w;
            }
            const int n = 4 * c4;
            const float4 o = make_float4(fmaxf(s.x + bias[n], 0.f), fmaxf(s.y + bias[n + 1], 0.f),
                                         fmaxf(s.z + bias[n + 2], 0.f), fmaxf(s.w + bias[n + 3], 0.f));
            y[i] = o;
            m = fmaxf(m, fmaxf(fmaxf(o.x, o.y), fmaxf(o.z, o.w)));
#pragma unroll
            for (int a = 0; a < NO; ++a) {
                const float4 wv = reinterpret_cast<const float4*>(wa)[a * 128 + c4];
                acc[a] = fmaf(o.x, wv.x, acc[a]);
                acc[a] = fmaf(o.y, wv.y, acc[a]);
                acc[a] = fmaf(o.z, wv.z, acc[a]);
                acc[a] = fmaf(o.w, wv.w, acc[a]);
            }
        }
#pragma unroll
        for (int a = 0; a < NO; ++a)
#pragma unroll
            for (int k = 32; k > 0; k >>= 1) acc[a] += __shfl_xor(acc[a], k, 64);
        if (lane < NO) {
            float r = acc[0];
#pragma unroll
            for (int a = 1; a < NO; ++a) r = lane == a ? acc[a] : r;
            logits[b * NO + lane] = r + ba[lane];
        }
    }
    amax_record(am, m);
}

// K-splits for a batch: enough (row tile, column block, split) workgroups for two per CU, at most 8
// (the heads' 512-deep hidden layer: splits up to 256 workgroups — 2 at 2,048 rows: 9.5 + 5.9 µs for the
// GEMM + reduce vs 10.9 + 6.2 with the fc layer's 512, whose K = 3136 gains from the fourth split)
inline int fc_fwd_splits(long long batch, long long wgs = 512) {
    const long long wg = ppox::ceil_div(batch, SG_ROWS) * FcFwd::NCB;
    int s = 1;
    while (s < 8 && wg * s < wgs) s *= 2;
    return s;
}

struct ActorHead {
    const float *w, *b;
    int n;          // actions (1..8); 0: no actor head fused
    float* logits;  // rows x n
};

// K = 3136: the fc layer (reduce: + bias, ReLU, f's amax, the actor head); K = 512: the heads' hidden
// layer (the same reduce with the critic head Linear(512, 1) fused, no amax)
template <int S>
int launch_fc_sk_reduce(const Args& a, float* slab, const float* bias, float* f, const ActorHead& act, hipStream_t st,
                        const char* name);
template <int K, int S, bool AP = false>
int launch_fc_fwd_sk(const Args& a, const uint16_t* q, float* slab, const float* bias, float* f, const ActorHead& act,
                     hipStream_t st, const char* name = "ppox_nature_fc_fwd_splitk") {
    Args b = a;
    b.y = slab;
    b.amax_y = nullptr;  // partial products: f's amax is recorded by the reduce
    const int rc = launch_sgemm<Px<SgRowsSK<K, 512, S>, AP>>(b, q, ppox::ceil_div(a.batch, SG_ROWS) * FcFwd::NCB * S,
                                                             st, name);
    if (rc != PPOX_OK) return rc;
    return launch_fc_sk_reduce<S>(a, slab, bias, f, act, st, name);
}
// the S partial products in order + bias, ReLU, f's amax (a.amax_y), the fused head
template <int S>
int launch_fc_sk_reduce(const Args& a, float* slab, const float* bias, float* f, const ActorHead& act, hipStream_t st,
                        const char* name) {
    const float4* sl = reinterpret_cast<const float4*>(slab);
    float4* f4 = reinterpret_cast<float4*>(f);
    const unsigned rows4 = (unsigned)ppox::ceil_div(a.batch, 4LL);
    switch (act.n) {
#define PPOX_FSA(N)                                                                                              \
    case N:                                                                                                      \
        fc_fwd_sk_reduce_actor<S, N><<<rows4, 256, 0, st>>>(sl, a.batch, bias, f4, a.amax_y, act.w, act.b, act.logits); \
        break;
        PPOX_FSA(1) PPOX_FSA(2) PPOX_FSA(3) PPOX_FSA(4) PPOX_FSA(5) PPOX_FSA(6) PPOX_FSA(7) PPOX_FSA(8)
#undef PPOX_FSA
        default:
            fc_fwd_sk_reduce<512, S><<<ppox::ceil_div(a.batch * 512 / 4, 256), 256, 0, st>>>(sl, a.batch, bias, f4,
                                                                                             a.amax_y);
    }
    PPOX_LAUNCHED(name);
}

}  // namespace

namespace ppox_conv {
int split_fwd23(int32_t layer, const void* x, int64_t batch, const uint16_t* wq, const float* bias, float* y,
                const uint32_t* amax_x, uint32_t* amax_y, uint32_t* relu_bits, const int* x_exp, int* y_exp_out,
                hipStream_t s) {
    PPOX_REQUIRE(ppox::aligned16(x), "ppox_nature_conv_fwd_split: layer 2/3 input must be 16B-aligned NHWC");
    // amax_x: the split of an f32 x and the bound of a PX output
    PPOX_REQUIRE((amax_x || (x_exp && !y_exp_out)) && (!amax_x || ppox::aligned16(amax_x)),
                 "ppox_nature_conv_fwd_split: amax slots of x required (layer 2/3)");
    PPOX_REQUIRE(!(reinterpret_cast<uintptr_t>(relu_bits) & 7), "ppox_nature_conv_fwd_split: relu_bits 8B alignment");
    PPOX_REQUIRE(!x_exp || layer == 3, "ppox_nature_conv_fwd_split: PX input (x_exp) is layer 3's (h2 planes)");
    Args a{x, nullptr, 0, 0, 0, nullptr, bias, nullptr, y, batch, amax_x, amax_y, pack_exp(wq, planes(layer))};
    a.bits_y = relu_bits;
    a.xexp = x_exp;
    a.yexp_out = y_exp_out;
    PPOX_REQUIRE(!y_exp_out || px_bound_ok(wq),
                 "ppox_nature_conv_fwd_split: a PX output needs wq packed with its bias (ppox_nature_pack_all)");
    a.ynorm = pack_norm(wq, planes(layer));
    a.ybias = pack_bmax(wq, planes(layer));
    constexpr const char* nm = "ppox_nature_conv_fwd_split";
    if (layer == 2) {
        const long long blocks = ppox::ceil_div(batch * G2::P, SG_ROWS);
        if (y_exp_out) return launch_sgemm<Px<SgFwd<G2, false>, false, true>>(a, wq, blocks, s, nm);
        return launch_sgemm<SgFwd<G2, false>>(a, wq, blocks, s, nm);
    }
    const long long blocks = ppox::ceil_div(batch * G3::P, SG_ROWS);
    if (x_exp && y_exp_out && dconv_enabled(3, batch))
        return dconv_fwd(3, x, batch, wq, bias, y, amax_x, amax_y, relu_bits, x_exp, y_exp_out, s);
    if (x_exp && y_exp_out) return launch_sgemm<Px<SgFwd<G3, false>, true, true>>(a, wq, blocks, s, nm);
    if (x_exp) return launch_sgemm<Px<SgFwd<G3, false>, true>>(a, wq, blocks, s, nm);
    if (y_exp_out) return launch_sgemm<Px<SgFwd<G3, false>, false, true>>(a, wq, blocks, s, nm);
    return launch_sgemm<SgFwd<G3, false>>(a, wq, blocks, s, nm);
}
}  // namespace ppox_conv

extern "C" int ppox_nature_conv_dgrad_split(int32_t layer, const float* grad_out, int64_t batch, const uint16_t* wqd,
                                            const float* prev_act, float* grad_in, const uint32_t* amax_g,
                                            uint32_t* amax_out, const uint32_t* relu_bits, const int* g_exp,
                                            int* y_exp_out, void* stream) {
    if (batch == 0) return PPOX_OK;  // empty shard / minibatch: no pointers to check
    PPOX_REQUIRE(layer == 2 || layer == 3, "ppox_nature_conv_dgrad_split: layer must be 2 or 3");
    PPOX_REQUIRE(grad_out && wqd && (prev_act || relu_bits) && grad_in && (amax_g || g_exp) && batch >= 0,
                 "ppox_nature_conv_dgrad_split: bad arguments");
    // relu_bits: the ReLU bitmask of the layer below (conv1's for layer 2, conv2's for layer 3)
    PPOX_REQUIRE(ppox::aligned16(grad_out) && ppox::aligned16(wqd) && (!amax_g || ppox::aligned16(amax_g)),
                 "ppox_nature_conv_dgrad_split: 16B alignment");
    Args a{grad_out, nullptr, 0, 0, 0, nullptr, nullptr, prev_act, grad_in, batch, amax_g, amax_out,
           pack_exp(wqd, ppox_conv::planes(10 + layer))};
    hipStream_t s = ppox::as_stream(stream);
    if (layer == 2 && g_exp) {  // PX g2 (the conv3 dgrad's planes output): the direct class-wise form
        PPOX_REQUIRE(relu_bits && !y_exp_out, "ppox_nature_conv_dgrad_split: a PX g2 needs conv1's ReLU bitmask "
                                              "(and writes an f32 g1)");
        return ppox_conv::ddgrad2(grad_out, batch, wqd, grad_in, relu_bits, amax_out, g_exp, a.wexp, s);
    }
    if (layer == 2) {
        PPOX_REQUIRE(!y_exp_out, "ppox_nature_conv_dgrad_split: layer 2 writes an f32 g1");
        const long long ntriples = ppox::ceil_div(batch, (long long)C2S);
        // one workgroup per CU (150 KB of LDS each), striding over the triples
        static int cus[64] = {};
        int dev = 0;
        PPOX_REQUIRE(hipGetDevice(&dev) == hipSuccess && dev < 64, "ppox_nature_conv_dgrad_split: no device");
        if (cus[dev] == 0)
            PPOX_REQUIRE(hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
                             cus[dev] > 0,
                         "ppox_nature_conv_dgrad_split: CU count");
        const long long grid = std::min<long long>(ntriples, cus[dev]);
        a.bits_mask = relu_bits;
        // PPOX_COLP_VMCNT0=1: every counted wait of the kernel as vmcnt(0) (the same result, bitwise)
        const char* safe_env = ppox::ab_env("PPOX_COLP_VMCNT0");
        const bool safe = safe_env && safe_env[0] == '1';
        const u32x4* wqv = reinterpret_cast<const u32x4*>(wqd);
        if (relu_bits && !safe)
            dgrad2_colp_kernel<true><<<(unsigned)grid, 512, 0, s>>>(a, wqv, ntriples);
        else if (relu_bits)
            dgrad2_colp_kernel<true, true><<<(unsigned)grid, 512, 0, s>>>(a, wqv, ntriples);
        else if (!safe)
            dgrad2_colp_kernel<false><<<(unsigned)grid, 512, 0, s>>>(a, wqv, ntriples);
        else
            dgrad2_colp_kernel<false, true><<<(unsigned)grid, 512, 0, s>>>(a, wqv, ntriples);
        PPOX_LAUNCHED("ppox_nature_conv_dgrad_split");
    }
    a.bits_mask = relu_bits;
    a.xexp = g_exp;  // PX g3 (the fc dgrad's planes output)
    PPOX_REQUIRE(!g_exp || relu_bits, "ppox_nature_conv_dgrad_split: a PX g3 needs conv2's ReLU bitmask");
    if (y_exp_out) {  // PX g2, bounded by amax(g3) x the dgrad matrix's column norms (no bias)
        PPOX_REQUIRE(relu_bits && amax_g && ppox::aligned16(amax_g),
                     "ppox_nature_conv_dgrad_split: a PX g2 needs conv2's ReLU bitmask and g3's amax slots");
        PPOX_REQUIRE(ppox_conv::px_bound_ok(wqd),
                     "ppox_nature_conv_dgrad_split: a PX g2 needs wqd packed by ppox_nature_pack_all");
        a.yexp_out = y_exp_out;
        a.ynorm = pack_norm(wqd, PL_Q3);
        a.ybias = pack_bmax(wqd, PL_Q3);
        if (g_exp && ppox_conv::ddgrad3_enabled(batch))  // the direct form (dconv.hip)
            return ppox_conv::ddgrad3(grad_out, batch, wqd, grad_in, amax_g, amax_out, relu_bits, g_exp, a.wexp, a.ynorm,
                                      a.ybias, y_exp_out, s);
        const long long blocks = ppox::ceil_div(batch, SG_ROWS) * SgDgradPM<G3>::NPOS;
        if (g_exp) return launch_sgemm<Px<SgDgradPM<G3, true>, true, true>>(a, wqd, blocks, s, "ppox_nature_conv_dgrad_split");
        return launch_sgemm<Px<SgDgradPM<G3, true>, false, true>>(a, wqd, blocks, s, "ppox_nature_conv_dgrad_split");
    }
    if (g_exp)
        return launch_sgemm<Px<SgDgradPM<G3, true>, true>>(a, wqd, ppox::ceil_div(batch, SG_ROWS) * SgDgradPM<G3>::NPOS,
                                                           s, "ppox_nature_conv_dgrad_split");
    if (relu_bits)
        return launch_sgemm<SgDgradPM<G3, true>>(a, wqd, ppox::ceil_div(batch, SG_ROWS) * SgDgradPM<G3>::NPOS, s,
                                                 "ppox_nature_conv_dgrad_split");
    return launch_sgemm<SgDgradPM<G3>>(a, wqd, ppox::ceil_div(batch, SG_ROWS) * SgDgradPM<G3>::NPOS, s,
                                       "ppox_nature_conv_dgrad_split");
}

// ---- conv2 on H1P (conv1's output as f16 planes, conv_common.h) --------------------------
extern "C" int ppox_nature_conv2_fwd_planes(const uint16_t* h1p, const uint16_t* q1, int64_t batch,
                                            const uint16_t* wq2, const float* bias, float* y, const uint32_t* amax_x,
                                            uint32_t* amax_y, uint32_t* relu_bits, int* y_exp_out, void* stream) {
    if (batch == 0) return PPOX_OK;
    PPOX_REQUIRE(h1p && q1 && wq2 && bias && y && batch > 0, "ppox_nature_conv2_fwd_planes: bad arguments");
    PPOX_REQUIRE(ppox::aligned16(h1p) && ppox::aligned16(wq2), "ppox_nature_conv2_fwd_planes: 16B alignment");
    PPOX_REQUIRE(!(reinterpret_cast<uintptr_t>(relu_bits) & 7), "ppox_nature_conv2_fwd_planes: relu_bits 8B alignment");
    PPOX_REQUIRE(!y_exp_out || (amax_x && ppox::aligned16(amax_x)),
                 "ppox_nature_conv2_fwd_planes: a PX output (y_exp_out) needs h1's amax slots (amax_x)");
    PPOX_REQUIRE(!y_exp_out || ppox_conv::px_bound_ok(wq2),
                 "ppox_nature_conv2_fwd_planes: a PX output needs wq2 packed with its bias (ppox_nature_pack_all)");
    Args a{h1p, nullptr, 0, 0, 0, nullptr, bias, nullptr, y, batch, amax_x, amax_y, pack_exp(wq2, PL_Q2)};
    a.bits_y = relu_bits;
    a.xexp = h1p_exp(q1, PL_Q1);
    a.yexp_out = y_exp_out;
    a.ynorm = pack_norm(wq2, PL_Q2);
    a.ybias = pack_bmax(wq2, PL_Q2);
    const long long blocks = ppox::ceil_div(batch * G2::P, SG_ROWS);
    if (y_exp_out && ppox_conv::dconv_enabled(2, batch))
        return ppox_conv::dconv_fwd(2, h1p, batch, wq2, bias, y, amax_x, amax_y, relu_bits, a.xexp, y_exp_out,
                                    ppox::as_stream(stream));
    if (y_exp_out)
        return launch_sgemm<Px<SgFwd2P, true, true>>(a, wq2, blocks, ppox::as_stream(stream), "ppox_nature_conv2_fwd_planes");
    return launch_sgemm<SgFwd2P>(a, wq2, blocks, ppox::as_stream(stream), "ppox_nature_conv2_fwd_planes");
}

// ---- NatureCNN fc layer (3136 -> 512) on the split-f16 GEMM -----------------------
extern "C" int ppox_nature_fc_fwd(const float* h3, int64_t batch, const uint16_t* q_fwd, const float* bias, float* f,
                                  const uint32_t* amax_h3, uint32_t* amax_f, const int* h3_exp, void* stream) {
    if (batch == 0) return PPOX_OK;  // empty shard / minibatch: no pointers to check
    PPOX_REQUIRE(h3 && q_fwd && bias && f && (amax_h3 || h3_exp) && batch >= 0, "ppox_nature_fc_fwd: bad arguments");
    PPOX_REQUIRE(ppox::aligned16(h3) && ppox::aligned16(q_fwd) && (!amax_h3 || ppox::aligned16(amax_h3)),
                 "ppox_nature_fc_fwd: 16B alignment");
    Args a{h3, nullptr, 0, 0, 0, nullptr, bias, nullptr, f, batch, amax_h3, amax_f, pack_exp(q_fwd, PL_FCF)};
    a.xexp = h3_exp;  // PX h3 (the conv3 forward's planes output)
    const long long blocks = ppox::ceil_div(batch, SG_ROWS) * (512 / SG_FC_NB);
    if (h3_exp && ppox_conv::fcw_enabled(batch))  // the wide-tile form (dconv.hip)
        return ppox_conv::fcw(h3, batch, q_fwd, bias, f, amax_f, h3_exp, a.wexp, ppox::as_stream(stream));
    if (h3_exp)
        return launch_sgemm<Px<SgRows<3136, 512, FC_FWD, FC_FWD_GW, false, SG_FC_NB>, true>>(
            a, q_fwd, blocks, ppox::as_stream(stream), "ppox_nature_fc_fwd");
    return launch_sgemm<SgRows<3136, 512, FC_FWD, FC_FWD_GW, false, SG_FC_NB>>(a, q_fwd, blocks, ppox::as_stream(stream),
                                                                             "ppox_nature_fc_fwd");
}

extern "C" int64_t ppox_nature_fc_fwd_splitk_workspace_bytes(int64_t batch) {
    if (batch <= 0) return 0;
    const long long s = ppox_conv::fcw_sk_enabled(batch) ? ppox_conv::FCW_SPLITS : fc_fwd_splits(batch);
    return (int64_t)s * batch * 512 * 4;
}

extern "C" int ppox_nature_fc_fwd_splitk(const float* h3, int64_t batch, const uint16_t* q_fwd, const float* bias,
                                         void* workspace, int64_t workspace_bytes, float* f, const uint32_t* amax_h3,
                                         uint32_t* amax_f, const float* w_actor, const float* b_actor,
                                         int32_t n_actions, float* logits, const int* h3_exp, void* stream) {
    if (batch == 0) return PPOX_OK;
    PPOX_REQUIRE(h3 && q_fwd && bias && f && workspace && (amax_h3 || h3_exp) && batch > 0,
                 "ppox_nature_fc_fwd_splitk: bad arguments");
    PPOX_REQUIRE(ppox::aligned16(h3) && ppox::aligned16(q_fwd) && ppox::aligned16(f) && ppox::aligned16(workspace) &&
                     (!amax_h3 || ppox::aligned16(amax_h3)),
                 "ppox_nature_fc_fwd_splitk: 16B alignment");
    PPOX_REQUIRE(workspace_bytes >= ppox_nature_fc_fwd_splitk_workspace_bytes(batch),
                 "ppox_nature_fc_fwd_splitk: workspace too small");
    PPOX_REQUIRE(!logits || (w_actor && b_actor && n_actions >= 1 && n_actions <= 8 && ppox::aligned16(w_actor)),
                 "ppox_nature_fc_fwd_splitk: the fused actor head needs 1..8 actions and a 16B-aligned weight");
    Args a{h3, nullptr, 0, 0, 0, nullptr, bias, nullptr, f, batch, amax_h3, amax_f, pack_exp(q_fwd, PL_FCF)};
    a.xexp = h3_exp;  // PX h3
    float* slab = reinterpret_cast<float*>(workspace);
    hipStream_t st = ppox::as_stream(stream);
    const ActorHead act{w_actor, b_actor, logits ? (int)n_actions : 0, logits};
    if (h3_exp && ppox_conv::fcw_sk_enabled(batch)) {  // the wide-tile form split 8 ways (dconv.hip)
        const int rc = ppox_conv::fcw_sk(h3, batch, q_fwd, slab, h3_exp, a.wexp, st);
        if (rc != PPOX_OK) return rc;
        static_assert(ppox_conv::FCW_SPLITS == 8, "the reduce's split count");
        return launch_fc_sk_reduce<8>(a, slab, bias, f, act, st, "ppox_nature_fc_fwd_splitk");
    }
    if (h3_exp) {
        switch (fc_fwd_splits(batch)) {
            case 1: return launch_fc_fwd_sk<3136, 1, true>(a, q_fwd, slab, bias, f, act, st);
            case 2: return launch_fc_fwd_sk<3136, 2, true>(a, q_fwd, slab, bias, f, act, st);
            case 4: return launch_fc_fwd_sk<3136, 4, true>(a, q_fwd, slab, bias, f, act, st);
            default: return launch_fc_fwd_sk<3136, 8, true>(a, q_fwd, slab, bias, f, act, st);
        }
    }
    switch (fc_fwd_splits(batch)) {
        case 1: return launch_fc_fwd_sk<3136, 1>(a, q_fwd, slab, bias, f, act, st);
        case 2: return launch_fc_fwd_sk<3136, 2>(a, q_fwd, slab, bias, f, act, st);
        case 4: return launch_fc_fwd_sk<3136, 4>(a, q_fwd, slab, bias, f, act, st);
        default: return launch_fc_fwd_sk<3136, 8>(a, q_fwd, slab, bias, f, act, st);
    }
}

extern "C" int ppox_nature_fc_dgrad(const float* df, int64_t batch, const uint16_t* q_dgrad, const float* h3, float* g3,
                                    const uint32_t* amax_df, uint32_t* amax_g3, const uint32_t* relu_bits,
                                    int* g3_exp_out, const int* df_exp, void* stream) {
    if (batch == 0) return PPOX_OK;  // empty shard / minibatch: no pointers to check
    PPOX_REQUIRE(df && q_dgrad && (h3 || relu_bits) && g3 && amax_df && batch >= 0,
                 "ppox_nature_fc_dgrad: bad arguments");
    PPOX_REQUIRE(ppox::aligned16(df) && ppox::aligned16(q_dgrad) && ppox::aligned16(amax_df),
                 "ppox_nature_fc_dgrad: 16B alignment");
    Args a{df, nullptr, 0, 0, 0, nullptr, nullptr, h3, g3, batch, amax_df, amax_g3, pack_exp(q_dgrad, PL_FCD)};
    a.bits_mask = relu_bits;  // h3's ReLU bitmask from the conv3 forward (instead of h3)
    a.xexp = df_exp;          // PX df (ppox_px_split): its planes are the A rows as they lie
    const long long blocks = ppox::ceil_div(batch, SG_ROWS) * ppox::ceil_div(3136, SG_FC_NB);
    hipStream_t s = ppox::as_stream(stream);
    const char* nm = "ppox_nature_fc_dgrad";
    using Bits = SgRows<512, 3136, FC_DGRAD, FC_DGRAD_GW, true, SG_FC_NB>;
    using Acts = SgRows<512, 3136, FC_DGRAD, FC_DGRAD_GW, false, SG_FC_NB>;
    if (g3_exp_out) {  // g3 as PX planes, bounded by amax(df) * the fc weight's column norms
        PPOX_REQUIRE(relu_bits, "ppox_nature_fc_dgrad: a PX g3 needs h3's ReLU bitmask");
        PPOX_REQUIRE(ppox_conv::px_bound_ok(q_dgrad),
                     "ppox_nature_fc_dgrad: a PX g3 needs q_dgrad packed by ppox_nature_pack_all / fc_pack");
        a.yexp_out = g3_exp_out;
        a.ynorm = pack_norm(q_dgrad, PL_FCD);
        a.ybias = pack_bmax(q_dgrad, PL_FCD);
        if (df_exp && ppox_conv::dfcd_enabled(batch))
            return ppox_conv::dfcd(df, batch, q_dgrad, g3, amax_df, amax_g3, relu_bits, g3_exp_out, df_exp, a.wexp,
                                   a.ynorm, a.ybias, s);
        return df_exp ? launch_sgemm<Px<Bits, true, true>>(a, q_dgrad, blocks, s, nm)
                      : launch_sgemm<Px<Bits, false, true>>(a, q_dgrad, blocks, s, nm);
    }
    if (relu_bits)
        return df_exp ? launch_sgemm<Px<Bits, true>>(a, q_dgrad, blocks, s, nm) : launch_sgemm<Bits>(a, q_dgrad, blocks, s, nm);
    return df_exp ? launch_sgemm<Px<Acts, true>>(a, q_dgrad, blocks, s, nm) : launch_sgemm<Acts>(a, q_dgrad, blocks, s, nm);
}

// ---- the heads' hidden layer Linear(512, 512) + ReLU on the split-f16 GEMM -------------
extern "C" int ppox_head_hidden_fwd(const float* f, int64_t rows, const uint16_t* q_fwd, const float* bias, float* e,
                                    const uint32_t* amax_f, void* stream) {
    if (rows == 0) return PPOX_OK;
    PPOX_REQUIRE(f && q_fwd && bias && e && amax_f && rows > 0, "ppox_head_hidden_fwd: bad arguments");
    PPOX_REQUIRE(ppox::aligned16(f) && ppox::aligned16(q_fwd) && ppox::aligned16(amax_f),
                 "ppox_head_hidden_fwd: 16B alignment");
    Args a{f, nullptr, 0, 0, 0, nullptr, bias, nullptr, e, rows, amax_f, nullptr, pack_exp(q_fwd, PL_H)};
    return launch_sgemm<SgRows<512, 512, FC_FWD, HEAD_GW, false, SG_FC_NB>>(
        a, q_fwd, ppox::ceil_div(rows, SG_ROWS) * (512 / SG_FC_NB), ppox::as_stream(stream), "ppox_head_hidden_fwd");
}

extern "C" int64_t ppox_head_hidden_fwd_splitk_workspace_bytes(int64_t rows) {
    return rows <= 0 ? 0 : (int64_t)fc_fwd_splits(rows, 256) * rows * 512 * 4;
}

// small batches: split over K like ppox_nature_fc_fwd_splitk (128 workgroups of 128 rows at 2,048 rows
// leave half the chip idle), the critic head v = e w_critic^T + b_critic fused into the reduce
extern "C" int ppox_head_hidden_fwd_splitk(const float* f, int64_t rows, const uint16_t* q_fwd, const float* bias,
                                           void* workspace, int64_t workspace_bytes, float* e, const uint32_t* amax_f,
                                           const float* w_critic, const float* b_critic, float* value, void* stream) {
    if (rows == 0) return PPOX_OK;
    PPOX_REQUIRE(f && q_fwd && bias && e && workspace && amax_f && rows > 0, "ppox_head_hidden_fwd_splitk: bad arguments");
    PPOX_REQUIRE(ppox::aligned16(f) && ppox::aligned16(q_fwd) && ppox::aligned16(e) && ppox::aligned16(workspace) &&
                     ppox::aligned16(amax_f),
                 "ppox_head_hidden_fwd_splitk: 16B alignment");
    PPOX_REQUIRE(workspace_bytes >= ppox_head_hidden_fwd_splitk_workspace_bytes(rows),
                 "ppox_head_hidden_fwd_splitk: workspace too small");
    PPOX_REQUIRE(!value || (w_critic && b_critic && ppox::aligned16(w_critic)),
                 "ppox_head_hidden_fwd_splitk: the fused critic head needs a 16B-aligned weight");
    Args a{f, nullptr, 0, 0, 0, nullptr, bias, nullptr, e, rows, amax_f, nullptr, pack_exp(q_fwd, PL_H)};
    float* slab = reinterpret_cast<float*>(workspace);
    hipStream_t st = ppox::as_stream(stream);
    const ActorHead crit{w_critic, b_critic, value ? 1 : 0, value};
    constexpr const char* nm = "ppox_head_hidden_fwd_splitk";
    switch (fc_fwd_splits(rows, 256)) {
        case 1: return launch_fc_fwd_sk<512, 1>(a, q_fwd, slab, bias, e, crit, st, nm);
        case 2: return launch_fc_fwd_sk<512, 2>(a, q_fwd, slab, bias, e, crit, st, nm);
        case 4: return launch_fc_fwd_sk<512, 4>(a, q_fwd, slab, bias, e, crit, st, nm);
        default: return launch_fc_fwd_sk<512, 8>(a, q_fwd, slab, bias, e, crit, st, nm);
    }
}

extern "C" int ppox_head_hidden_dgrad(const float* de, int64_t rows, const uint16_t* q_dgrad, const float* f, float* df,
                                      const uint32_t* amax_de, uint32_t* amax_df, void* stream) {
    if (rows == 0) return PPOX_OK;
    PPOX_REQUIRE(de && q_dgrad && f && df && amax_de && rows > 0, "ppox_head_hidden_dgrad: bad arguments");
    PPOX_REQUIRE(ppox::aligned16(de) && ppox::aligned16(q_dgrad) && ppox::aligned16(amax_de),
                 "ppox_head_hidden_dgrad: 16B alignment");
    Args a{de, nullptr, 0, 0, 0, nullptr, nullptr, f, df, rows, amax_de, amax_df, pack_exp(q_dgrad, PL_H)};
    return launch_sgemm<SgRows<512, 512, HEAD_DGRAD, HEAD_GW, false, SG_FC_NB>>(
        a, q_dgrad, ppox::ceil_div(rows, SG_ROWS) * (512 / SG_FC_NB), ppox::as_stream(stream), "ppox_head_hidden_dgrad");
}

// the heads' backward to the fc output in one launch (csrc/dconv.hip hbw_kernel): de = (e > 0) dv wc and
// df = (f > 0) (dout Wa + de Wh) — ppox_head_dgrad_outer + ppox_head_hidden_dgrad without de's HBM round trip
extern "C" int ppox_head_backward(const float* dout, const float* w_actor, const float* dv, const float* w_critic,
                                  const float* e, const float* f, const uint16_t* q_dgrad, int64_t rows, int64_t h,
                                  int64_t n_out, float* df, float* de, uint32_t* amax_de, uint32_t* amax_df,
                                  void* stream) {
    if (rows == 0) return PPOX_OK;
    PPOX_REQUIRE(dout && w_actor && dv && w_critic && e && f && q_dgrad && df && de && amax_de && amax_df && rows > 0,
                 "ppox_head_backward: bad arguments");
    PPOX_REQUIRE(h == 512, "ppox_head_backward: the hidden layer is 512 wide");
    PPOX_REQUIRE(ppox::aligned16(amax_de) && ppox::aligned16(amax_df), "ppox_head_backward: 16B alignment");
    return ppox_conv::head_backward(dout, w_actor, dv, w_critic, e, f, q_dgrad, pack_exp(q_dgrad, PL_H), rows,
                                    (int)n_out, df, de, amax_de, amax_df, ppox::as_stream(stream));
}
