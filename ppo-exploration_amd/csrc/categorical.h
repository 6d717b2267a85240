// The Categorical(probs=softmax(logits)) head shared by the fused loss kernels (loss.hip, sil.hip):
// torch's CPU arithmetic op by op in f32, the env-major index map and the action-count dispatch.
#pragma once
#include "common.h"

namespace {

constexpr float F32_EPS = 1.1920928955078125e-07f;

// index map: env-major flat i -> step-major element (t*N + n)
__device__ inline long long elem(long long i, long long T, long long N) { return (i % T) * N + (i / T); }

// ---- categorical head (models.py:62-64 via torch.distributions.Categorical) ----
template <int MAXA>
struct CatRow {
    float p[MAXA], q[MAXA], c[MAXA], lp[MAXA];
    float s;  // sum of p (renormaliser)
    float ent;
};

template <int MAXA>
__device__ inline void categorical_forward(const float* zp, int A, CatRow<MAXA>& r) {
    // the row's logits loaded unconditionally first (j >= A re-reads logit A - 1, never used):
    // a load under the j < A branches below would cost a memory round trip per logit
    float z[MAXA];
#pragma unroll
    for (int j = 0; j < MAXA; ++j) z[j] = zp[j < A ? j : A - 1];
    float m = z[0];
#pragma unroll
    for (int j = 1; j < MAXA; ++j)
        if (j < A) m = fmaxf(m, z[j]);
    float S = 0.f;
#pragma unroll
    for (int j = 0; j < MAXA; ++j)
        if (j < A) {
            r.p[j] = expf(z[j] - m);
            S += r.p[j];
        }
    const float inv = 1.0f / S;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < MAXA; ++j)
        if (j < A) {
            r.p[j] = r.p[j] * inv;
            s += r.p[j];
        }
    r.s = s;
    float ent = 0.f;
#pragma unroll
    for (int j = 0; j < MAXA; ++j)
        if (j < A) {
            r.q[j] = r.p[j] / s;
            r.c[j] = fminf(fmaxf(r.q[j], F32_EPS), 1.0f - F32_EPS);
            r.lp[j] = logf(r.c[j]);
            ent += r.lp[j] * r.q[j];
        }
    r.ent = -ent;
}

__device__ inline float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

#define PPOX_DISPATCH_A(A, MAXA_NAME, ...)      \
    if ((A) <= 4) {                             \
        constexpr int MAXA_NAME = 4;            \
        __VA_ARGS__;                            \
    } else if ((A) <= 8) {                      \
        constexpr int MAXA_NAME = 8;            \
        __VA_ARGS__;                            \
    } else if ((A) <= 18) {                     \
        constexpr int MAXA_NAME = 18;           \
        __VA_ARGS__;                            \
    } else if ((A) <= 32) {                     \
        constexpr int MAXA_NAME = 32;           \
        __VA_ARGS__;                            \
    } else {                                    \
        constexpr int MAXA_NAME = 64;           \
        __VA_ARGS__;                            \
    }

}  // namespace
