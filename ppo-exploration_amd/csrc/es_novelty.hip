// Per-member novelty for NSR-ES (EvolutionStrategy(..., novelty="member")): the mean distance of each member's
// behaviour characterisation to its S = min(K, M) nearest archive rows — the reference's get_kNN / get_novelty
// (evolution_strategies.py:201-222, :273-289) for every member of a launch at once.  include/ppox.h holds the
// semantics, tests/es_novelty_twin.py their numpy restatement.
//
// One wave per member, four members per 256-thread block (es_eval_control_kernel's layout).  Lanes stride the
// archive rows; each lane keeps its KMAX smallest distances as an ascending list in registers (an unrolled
// compare-exchange chain: no dynamically indexed array, nothing in scratch), +inf where it has seen fewer rows.
// The merge is S rounds of a wave-wide minimum over the lanes' heads; in each round the lowest lane holding the
// minimum pops it, so equal distances leave one at a time and the sum runs in ascending order.  No atomics, no LDS.
// The unit is built with fp contraction off (Makefile), so the squares and their sum round one by one.
#include <cmath>

#include "common.h"

namespace {

constexpr int KMAX = 16, DMAX = 8;

__device__ inline double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double u = __shfl_xor(v, o, 64);
        v = u < v ? u : v;
    }
    return v;
}

template <int D>
__global__ void __launch_bounds__(256)
    es_knn_novelty_kernel(const double* __restrict__ bc, long long P, const double* __restrict__ archive, long long M,
                          int S, double* __restrict__ novelty) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long p = (long long)blockIdx.x * 4 + wv;
    if (p >= P) return;  // wave-uniform
    double q[D];
#pragma unroll
    for (int j = 0; j < D; ++j) q[j] = bc[p * D + j];
    const double inf = __builtin_huge_val();
    double a[KMAX];  // ascending
#pragma unroll
    for (int i = 0; i < KMAX; ++i) a[i] = inf;
    for (long long m = lane; m < M; m += 64) {
        const double* row = archive + m * D;
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const double diff = row[j] - q[j];
            acc = acc + diff * diff;
        }
        double d = sqrt(acc);
        if (d < a[KMAX - 1]) {  // else the chain would leave the list as it is
#pragma unroll
            for (int i = 0; i < KMAX; ++i) {
                const bool lt = d < a[i];
                const double lo = lt ? d : a[i];
                d = lt ? a[i] : d;
                a[i] = lo;
            }
        }
    }
    double sum = 0.0;
    for (int r = 0; r < S; ++r) {
        const double mn = wave_min(a[0]);
        const unsigned long long holders = __ballot(a[0] == mn);
        const int winner = __ffsll(holders) - 1;  // holders != 0: the minimum is some lane's head
        if (lane == winner) {
#pragma unroll
            for (int i = 0; i + 1 < KMAX; ++i) a[i] = a[i + 1];
            a[KMAX - 1] = inf;
        }
        sum = sum + mn;
    }
    if (lane == 0) {
        const double nov = sum / (double)S;
        novelty[p] = nov <= 1e-3 ? 5e-3 : nov;
    }
}

}  // namespace

extern "C" int ppox_es_knn_novelty(const double* bc, int64_t P, const double* archive, int64_t M, int32_t D, int32_t K,
                                   double* novelty, void* stream) {
    PPOX_REQUIRE(bc && archive && novelty, "ppox_es_knn_novelty: null pointer");
    PPOX_REQUIRE(P >= 1 && M >= 1, "ppox_es_knn_novelty: P and M must be positive (P %lld, M %lld)", (long long)P,
                 (long long)M);
    PPOX_REQUIRE(D >= 1 && D <= DMAX, "ppox_es_knn_novelty: D must lie in [1, 8], not %d", (int)D);
    PPOX_REQUIRE(K >= 1 && K <= KMAX, "ppox_es_knn_novelty: K must lie in [1, 16], not %d", (int)K);
    PPOX_REQUIRE((P + 3) / 4 <= 0x7FFFFFFFLL, "ppox_es_knn_novelty: population too large");
    const int S = (int)(K < M ? K : M);
    const unsigned blocks = ppox::ceil_div(P, 4);
    hipStream_t s = ppox::as_stream(stream);
#define PPOX_KNN(DD) es_knn_novelty_kernel<DD><<<blocks, 256, 0, s>>>(bc, P, archive, M, S, novelty)
    switch (D) {
        case 1: PPOX_KNN(1); break;
        case 2: PPOX_KNN(2); break;
        case 3: PPOX_KNN(3); break;
        case 4: PPOX_KNN(4); break;
        case 5: PPOX_KNN(5); break;
        case 6: PPOX_KNN(6); break;
        case 7: PPOX_KNN(7); break;
        default: PPOX_KNN(8); break;
    }
#undef PPOX_KNN
    PPOX_LAUNCHED("ppox_es_knn_novelty");
}
