// K8 on pixel observations — SimHash keys of uint8 frames, exact in integers.
//   a[b, d]  = popcount(w & 0xFFFF) - popcount(w >> 16),  w = word d % 4 of
//              philox4x32_10({d / 4, b, 0, 0xFFFFFFFE}, key = seed)         (int8, 16 x D)
//   key_n    = bit b set iff sum_d a[b, d] * obs_n[d] > 0                   (obs as unsigned bytes)
// The keys are a 16 x N x D integer GEMM.  The i8 MFMA multiplies signed bytes, so it is fed
// obs ^ 0x80 (= obs - 128 as int8) and 128 * rowsum[b] is added back at the end.  Integer sums
// are order-free: any tiling / split of D gives the same bits.
//
// Hot path (D % 16 == 0, rows 16-byte aligned): a workgroup of 4 waves owns 64 envs (4 MFMA
// column tiles) and a slice of D; a wave walks the slice in 128-byte units, loads one A8 fragment per
// 64 bytes and reuses it for its 4 env tiles (A8 is read once per 64 envs, not once per env).  Both
// MFMA operands take bytes [64 s + 16 (lane >> 4), +16) of row (lane & 15) — the same k on both
// sides, which is all the sum over k needs.  The 4 waves' accumulators are added in LDS and stored
// as one partial slab per (slice, env block); a second kernel adds the slabs in slice order, adds
// 128 * rowsum and writes the keys.  Everything else (odd D, unaligned rows) takes a plain kernel.
// ppox_simhash_sums_u8 (the episodic bonus's embedding) runs the same partial kernel and
// a finish that stores the 16 sums themselves; its plain kernel is the keys' with the other epilogue.
#include "common.h"
#include "philox.h"

namespace {

using i32x4 = __attribute__((ext_vector_type(4))) int;

constexpr int BITS = 16;
constexpr uint32_t HASH_TAG = 0xFFFFFFFEu;  // Philox counter word 3 of the hash-matrix domain
constexpr int PX_ENVS = 64;                 // envs per workgroup: 4 MFMA tiles of 16
constexpr int PX_TILES = PX_ENVS / 16;
constexpr int PX_WAVES = 4;
constexpr int PX_UNIT = 128;                // bytes of a row a wave takes per loop trip
constexpr int PX_H = PX_UNIT / 64;          // MFMA k-steps (64 bytes) per trip
constexpr int PX_SLAB = BITS * PX_ENVS;     // int32 per partial slab (fragment order)
constexpr long long PX_TARGET_WGS = 512;    // workgroups aimed at (2 per CU), measured best of 256 .. 4096
constexpr long long PX_MIN_UNITS = 8;       // least units per workgroup (two trips per wave): N = 512 9.3 vs 11.3 us
// |sum| <= 16 * 255 * D must fit int32
constexpr long long PX_MAX_D = 0x7FFFFFFFll / (16 * 255);

__device__ inline int hash_entry(uint32_t w) { return __popc(w & 0xFFFFu) - __popc(w >> 16); }

// one block per hash row b: the row's bytes and their sum
__global__ void __launch_bounds__(256) simhash_matrix_kernel(long long D, uint32_t k0, uint32_t k1,
                                                             int8_t* __restrict__ A8, int32_t* __restrict__ rowsum) {
    __shared__ int red[4];
    const uint32_t b = blockIdx.x;
    int8_t* row = A8 + (long long)b * D;
    int sum = 0;
    for (long long q = threadIdx.x; q * 4 < D; q += 256) {
        const ppox::u32x4 w = ppox::philox4x32_10(ppox::u32x4{(uint32_t)q, b, 0u, HASH_TAG}, k0, k1);
        const int a[4] = {hash_entry(w.x), hash_entry(w.y), hash_entry(w.z), hash_entry(w.w)};
        for (int j = 0; j < 4; ++j)
            if (q * 4 + j < D) {
                row[q * 4 + j] = (int8_t)a[j];
                sum += a[j];
            }
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) rowsum[b] = red[0] + red[1] + red[2] + red[3];
}

// 128-byte units of a row per workgroup (a multiple of the 4 waves), so that
// env blocks x slices is about PX_TARGET_WGS and never above max(env blocks, PX_TARGET_WGS)
inline long long px_units_per_wg(long long nblocks, long long units) {
    const long long want = PX_TARGET_WGS / nblocks > 1 ? PX_TARGET_WGS / nblocks : 1;
    long long per = (units + want - 1) / want;
    if (per < PX_MIN_UNITS) per = PX_MIN_UNITS;
    return (per + PX_WAVES - 1) / PX_WAVES * PX_WAVES;
}

__global__ void __launch_bounds__(256) simhash_px_partial_kernel(const uint8_t* __restrict__ obs, long long N,
                                                                 long long D, long long stride,
                                                                 const int8_t* __restrict__ A8, long long units,
                                                                 long long units_per_wg, int32_t* __restrict__ part) {
    __shared__ int red[PX_WAVES][PX_SLAB];  // 16 KB
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, g = lane >> 4;
    const long long blk = blockIdx.x, slice = blockIdx.y;
    const long long u0 = slice * units_per_wg;
    const long long u1 = u0 + units_per_wg < units ? u0 + units_per_wg : units;
    const int8_t* arow = A8 + (long long)col * D + 16 * g;
    const uint8_t* orow[PX_TILES];
    bool live[PX_TILES];
    for (int t = 0; t < PX_TILES; ++t) {
        const long long env = blk * PX_ENVS + t * 16 + col;
        live[t] = env < N;
        orow[t] = obs + (live[t] ? env : 0) * stride + 16 * g;
    }
    i32x4 acc[PX_TILES];
    for (int t = 0; t < PX_TILES; ++t) acc[t] = i32x4{0, 0, 0, 0};
    const i32x4 zero = {0, 0, 0, 0};
    for (long long u = u0 + wave; u < u1; u += PX_WAVES) {
        i32x4 a[PX_H], x[PX_H][PX_TILES];
#pragma unroll
        for (int h = 0; h < PX_H; ++h) {
            const long long k = u * PX_UNIT + h * 64;  // this lane's 16 bytes start at k + 16 g
            const bool in = k + 16 * g < D;            // D % 16 == 0: a 16-byte granule is whole or absent
            a[h] = in ? *reinterpret_cast<const i32x4*>(arow + k) : zero;
#pragma unroll
            for (int t = 0; t < PX_TILES; ++t)
                x[h][t] = in && live[t] ? *reinterpret_cast<const i32x4*>(orow[t] + k) : zero;
        }
#pragma unroll
        for (int h = 0; h < PX_H; ++h)
#pragma unroll
            for (int t = 0; t < PX_TILES; ++t) {
                const i32x4 xs = x[h][t] ^ (int)0x80808080;  // unsigned byte - 128 as int8
                acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[h], xs, acc[t], 0, 0, 0);
            }
    }
    // D[row = hash bit (lane >> 4) * 4 + r][col = env lane & 15], kept in fragment order
    for (int t = 0; t < PX_TILES; ++t)
        for (int r = 0; r < 4; ++r) red[wave][(t * 4 + r) * 64 + lane] = acc[t][r];
    __syncthreads();
    int32_t* slab = part + (slice * gridDim.x + blk) * PX_SLAB;
    for (int e = threadIdx.x; e < PX_SLAB; e += 256) slab[e] = red[0][e] + red[1][e] + red[2][e] + red[3][e];
}

// one block per env block: thread e owns slab element e = (tile * 4 + r) * 64 + lane
__global__ void __launch_bounds__(PX_SLAB) simhash_px_finish_kernel(const int32_t* __restrict__ part, long long N,
                                                                    long long slices,
                                                                    const int32_t* __restrict__ rowsum,
                                                                    int32_t* __restrict__ keys) {
    __shared__ int key[PX_ENVS];
    const int e = threadIdx.x;
    const long long blk = blockIdx.x;
    if (e < PX_ENVS) key[e] = 0;
    __syncthreads();
    const int lane = e & 63, r = (e >> 6) & 3, t = e >> 8;
    const int b = (lane >> 4) * 4 + r, env = t * 16 + (lane & 15);
    int s = 128 * rowsum[b];
    for (long long q = 0; q < slices; ++q) s += part[(q * gridDim.x + blk) * PX_SLAB + e];
    if (s > 0) atomicOr(&key[env], 1 << b);
    __syncthreads();
    if (e < PX_ENVS && blk * PX_ENVS + e < N) keys[blk * PX_ENVS + e] = key[e];
}

// as the finish above, storing the sums: sums[env * 16 + b]
__global__ void __launch_bounds__(PX_SLAB) simhash_px_finish_sums_kernel(const int32_t* __restrict__ part, long long N,
                                                                         long long slices,
                                                                         const int32_t* __restrict__ rowsum,
                                                                         int32_t* __restrict__ sums) {
    const int e = threadIdx.x;
    const long long blk = blockIdx.x;
    const int lane = e & 63, r = (e >> 6) & 3, t = e >> 8;
    const int b = (lane >> 4) * 4 + r;
    const long long env = blk * PX_ENVS + t * 16 + (lane & 15);
    int s = 128 * rowsum[b];
    for (long long q = 0; q < slices; ++q) s += part[(q * gridDim.x + blk) * PX_SLAB + e];
    if (env < N) sums[env * BITS + b] = s;
}

// any D, stride, alignment: one block per env (SUMS: out[n * 16 + b] = the sums, else out[n] = the key)
template <bool SUMS>
__global__ void __launch_bounds__(256) simhash_px_plain_kernel(const uint8_t* __restrict__ obs, long long D,
                                                               long long stride, const int8_t* __restrict__ A8,
                                                               int32_t* __restrict__ keys) {
    __shared__ int red[4][BITS];
    const long long n = blockIdx.x;
    const uint8_t* x = obs + n * stride;
    int s[BITS];
    for (int b = 0; b < BITS; ++b) s[b] = 0;
    for (long long d = threadIdx.x; d < D; d += 256) {
        const int v = x[d];
        for (int b = 0; b < BITS; ++b) s[b] += (int)A8[b * D + d] * v;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b = 0; b < BITS; ++b) {
        int v = s[b];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0) red[wave][b] = v;
    }
    __syncthreads();
    if (SUMS) {
        if (threadIdx.x < BITS) keys[n * BITS + lane] = red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
    } else if (wave == 0) {
        const bool set = lane < BITS && red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane] > 0;
        const unsigned long long m = __ballot(set);
        if (lane == 0) keys[n] = (int32_t)(m & 0xFFFFu);
    }
}

}  // namespace

extern "C" int ppox_simhash_matrix_i8(int64_t D, uint64_t seed, int8_t* A8, int32_t* rowsum, void* stream) {
    PPOX_REQUIRE(A8 && rowsum, "ppox_simhash_matrix_i8: null pointer");
    PPOX_REQUIRE(D >= 1 && D <= PX_MAX_D, "ppox_simhash_matrix_i8: bad sizes");
    simhash_matrix_kernel<<<BITS, 256, 0, ppox::as_stream(stream)>>>(D, (uint32_t)seed, (uint32_t)(seed >> 32), A8,
                                                                     rowsum);
    PPOX_LAUNCHED("ppox_simhash_matrix_i8");
}

extern "C" int64_t ppox_simhash_keys_u8_workspace_bytes(int64_t N) {
    if (N < 0) return -1;
    const long long nblocks = (N + PX_ENVS - 1) / PX_ENVS;
    return (nblocks > PX_TARGET_WGS ? nblocks : PX_TARGET_WGS) * PX_SLAB * (long long)sizeof(int32_t);
}

extern "C" int ppox_simhash_keys_u8(const uint8_t* obs, int64_t N, int64_t D, int64_t obs_stride, const int8_t* A8,
                                    const int32_t* rowsum, int32_t* acc, int32_t* keys, void* stream) {
    if (N == 0) return PPOX_OK;  // empty shard / minibatch: no pointers to check
    PPOX_REQUIRE(obs && A8 && rowsum && acc && keys, "ppox_simhash_keys_u8: null pointer");
    PPOX_REQUIRE(N >= 0 && N <= 0x7FFFFFFFll && D >= 1 && D <= PX_MAX_D && obs_stride >= D,
                 "ppox_simhash_keys_u8: bad sizes");
    hipStream_t s = ppox::as_stream(stream);
    if (D % 16 != 0 || obs_stride % 16 != 0 || !ppox::aligned16(obs) || !ppox::aligned16(A8)) {
        simhash_px_plain_kernel<false><<<(unsigned)N, 256, 0, s>>>(obs, D, obs_stride, A8, keys);
        PPOX_LAUNCHED("ppox_simhash_keys_u8");
    }
    const long long nblocks = (N + PX_ENVS - 1) / PX_ENVS, units = (D + PX_UNIT - 1) / PX_UNIT;
    const long long per = px_units_per_wg(nblocks, units), slices = (units + per - 1) / per;
    simhash_px_partial_kernel<<<dim3((unsigned)nblocks, (unsigned)slices), 256, 0, s>>>(obs, N, D, obs_stride, A8,
                                                                                        units, per, acc);
    PPOX_LAUNCHED_NORET("ppox_simhash_keys_u8");
    simhash_px_finish_kernel<<<(unsigned)nblocks, PX_SLAB, 0, s>>>(acc, N, slices, rowsum, keys);
    PPOX_LAUNCHED("ppox_simhash_keys_u8");
}

extern "C" int ppox_simhash_sums_u8(const uint8_t* obs, int64_t N, int64_t D, int64_t obs_stride, const int8_t* A8,
                                    const int32_t* rowsum, int32_t* acc, int32_t* sums, void* stream) {
    if (N == 0) return PPOX_OK;  // empty shard: no pointers to check
    PPOX_REQUIRE(obs && A8 && rowsum && acc && sums, "ppox_simhash_sums_u8: null pointer");
    PPOX_REQUIRE(N >= 0 && N <= 0x7FFFFFFFll && D >= 1 && D <= PX_MAX_D && obs_stride >= D,
                 "ppox_simhash_sums_u8: bad sizes");
    hipStream_t s = ppox::as_stream(stream);
    if (D % 16 != 0 || obs_stride % 16 != 0 || !ppox::aligned16(obs) || !ppox::aligned16(A8)) {
        simhash_px_plain_kernel<true><<<(unsigned)N, 256, 0, s>>>(obs, D, obs_stride, A8, sums);
        PPOX_LAUNCHED("ppox_simhash_sums_u8");
    }
    const long long nblocks = (N + PX_ENVS - 1) / PX_ENVS, units = (D + PX_UNIT - 1) / PX_UNIT;
    const long long per = px_units_per_wg(nblocks, units), slices = (units + per - 1) / per;
    simhash_px_partial_kernel<<<dim3((unsigned)nblocks, (unsigned)slices), 256, 0, s>>>(obs, N, D, obs_stride, A8,
                                                                                        units, per, acc);
    PPOX_LAUNCHED_NORET("ppox_simhash_sums_u8");
    simhash_px_finish_sums_kernel<<<(unsigned)nblocks, PX_SLAB, 0, s>>>(acc, N, slices, rowsum, sums);
    PPOX_LAUNCHED("ppox_simhash_sums_u8");
}
