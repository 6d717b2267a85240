// The classic-control dynamics shared by the device environments (env_real.hip, one thread
// per env) and the ES episode kernel (es_control.hip, one wave per member): state layout,
// reset draw, observation and one physics step of CartPole, MountainCar, Acrobot and
// Pendulum.  DESIGN.md "Real-dynamics envs" holds the equations; tests/real_env_twin.py is
// their numpy restatement.  No explicit fma here and the build sets -ffp-contract=off: every
// operation rounds once, as the twin's does.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "philox.h"
#include "../../include/ppox.h"

namespace ppox {

constexpr uint32_t RESET_ACTION = 0xFFFFFFFFu;
constexpr double PI = 3.14159265358979323846;

constexpr int CARTPOLE = PPOX_CONTROL_CARTPOLE, MOUNTAINCAR = PPOX_CONTROL_MOUNTAINCAR,
              ACROBOT = PPOX_CONTROL_ACROBOT, PENDULUM = PPOX_CONTROL_PENDULUM;

template <int KIND>
struct Dims {
    static constexpr int S = (KIND == CARTPOLE || KIND == ACROBOT) ? 4 : 2;
    static constexpr int D = KIND == CARTPOLE ? 4 : KIND == MOUNTAINCAR ? 2 : KIND == ACROBOT ? 6 : 3;
};

__device__ inline double clip(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

// ((x + pi) mod 2pi) - pi with the floored (Python) mod: fmod is exact, so this matches the twin bit for bit
__device__ inline double wrap_pi(double x) {
    double r = fmod(x + PI, 2 * PI);
    if (r < 0) r += 2 * PI;
    return r - PI;
}

template <int KIND>
__device__ inline void reset_bounds(int j, double& lo, double& hi) {
    if (KIND == CARTPOLE) {
        lo = -0.05, hi = 0.05;
    } else if (KIND == MOUNTAINCAR) {
        lo = j == 0 ? -0.6 : 0.0, hi = j == 0 ? -0.4 : 0.0;
    } else if (KIND == ACROBOT) {
        lo = -0.1, hi = 0.1;
    } else {
        lo = j == 0 ? -PI : -1.0, hi = j == 0 ? PI : 1.0;
    }
}

template <int KIND>
__device__ inline void draw_state(double* s, uint32_t gid, uint32_t episode, uint32_t k0, uint32_t k1) {
    const ppox::u32x4 w = ppox::philox4x32_10(ppox::u32x4{0u, gid, episode, RESET_ACTION}, k0, k1);
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int j = 0; j < Dims<KIND>::S; ++j) {
        double lo, hi;
        reset_bounds<KIND>(j, lo, hi);
        s[j] = lo + (hi - lo) * (double)ppox::u01(ws[j]);
    }
}

template <int KIND>
__device__ inline void write_obs(const double* s, float* o) {
    if (KIND == CARTPOLE) {
        o[0] = (float)s[0], o[1] = (float)s[1], o[2] = (float)s[2], o[3] = (float)s[3];
    } else if (KIND == MOUNTAINCAR) {
        o[0] = (float)s[0], o[1] = (float)s[1];
    } else if (KIND == ACROBOT) {
        o[0] = (float)cos(s[0]), o[1] = (float)sin(s[0]), o[2] = (float)cos(s[1]), o[3] = (float)sin(s[1]);
        o[4] = (float)s[2], o[5] = (float)s[3];
    } else {
        o[0] = (float)cos(s[0]), o[1] = (float)sin(s[0]), o[2] = (float)s[1];
    }
}

// Acrobot "book" accelerations: ds = (dth1, dth2, ddth1, ddth2)
__device__ inline void acrobot_dsdt(const double* s, double torque, double* ds) {
    const double m1 = 1.0, m2 = 1.0, l1 = 1.0, lc1 = 0.5, lc2 = 0.5, I1 = 1.0, I2 = 1.0, g = 9.8;
    const double th1 = s[0], th2 = s[1], dth1 = s[2], dth2 = s[3];
    const double c2 = cos(th2), s2 = sin(th2);
    const double d1 = m1 * lc1 * lc1 + m2 * (l1 * l1 + lc2 * lc2 + 2 * l1 * lc2 * c2) + I1 + I2;
    const double d2 = m2 * (lc2 * lc2 + l1 * lc2 * c2) + I2;
    const double phi2 = m2 * lc2 * g * cos(th1 + th2 - PI / 2);
    const double phi1 = -m2 * l1 * lc2 * dth2 * dth2 * s2 - 2 * m2 * l1 * lc2 * dth2 * dth1 * s2 +
                        (m1 * lc1 + m2 * l1) * g * cos(th1 - PI / 2) + phi2;
    const double ddth2 = (torque + d2 / d1 * phi1 - m2 * l1 * lc2 * dth1 * dth1 * s2 - phi2) /
                         (m2 * lc2 * lc2 + I2 - d2 * d2 / d1);
    const double ddth1 = -(d2 * ddth2 + phi1) / d1;
    ds[0] = dth1, ds[1] = dth2, ds[2] = ddth1, ds[3] = ddth2;
}

// advances s by one step of action a (int for the Discrete kinds, float for Pendulum)
template <int KIND>
__device__ inline void physics(double* s, int ai, float af, float& rew, bool& term) {
    if (KIND == CARTPOLE) {
        double x = s[0], xd = s[1], th = s[2], thd = s[3];
        const double f = ai == 1 ? 10.0 : -10.0;
        const double cth = cos(th), sth = sin(th);
        const double temp = (f + 0.05 * thd * thd * sth) / 1.1;
        const double tha = (9.8 * sth - cth * temp) / (0.5 * (4.0 / 3.0 - 0.1 * cth * cth / 1.1));
        const double xa = temp - 0.05 * tha * cth / 1.1;
        x += 0.02 * xd;
        xd += 0.02 * xa;
        th += 0.02 * thd;
        thd += 0.02 * tha;
        s[0] = x, s[1] = xd, s[2] = th, s[3] = thd;
        term = fabs(x) > 2.4 || fabs(th) > 12 * 2 * PI / 360;
        rew = 1.f;
    } else if (KIND == MOUNTAINCAR) {
        double p = s[0], v = s[1];
        v += (double)(ai - 1) * 0.001 + cos(3 * p) * (-0.0025);
        v = clip(v, -0.07, 0.07);
        p += v;
        p = clip(p, -1.2, 0.6);
        if (p == -1.2 && v < 0) v = 0;
        s[0] = p, s[1] = v;
        term = p >= 0.5 && v >= 0;
        rew = -1.f;
    } else if (KIND == ACROBOT) {
        const double torque = (double)(ai - 1), dt = 0.2, dt2 = dt / 2;
        double k1[4], k2[4], k3[4], k4[4], y[4];
        acrobot_dsdt(s, torque, k1);
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = s[j] + dt2 * k1[j];
        acrobot_dsdt(y, torque, k2);
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = s[j] + dt2 * k2[j];
        acrobot_dsdt(y, torque, k3);
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = s[j] + dt * k3[j];
        acrobot_dsdt(y, torque, k4);
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = s[j] + dt / 6.0 * (k1[j] + 2 * k2[j] + 2 * k3[j] + k4[j]);
        s[0] = wrap_pi(s[0]);
        s[1] = wrap_pi(s[1]);
        s[2] = clip(s[2], -4 * PI, 4 * PI);
        s[3] = clip(s[3], -9 * PI, 9 * PI);
        term = -cos(s[0]) - cos(s[0] + s[1]) > 1.0;
        rew = term ? 0.f : -1.f;
    } else {
        const double th = s[0], thd = s[1];
        const double u = clip((double)af, -2.0, 2.0);
        const double w = wrap_pi(th);
        const double cost = w * w + 0.1 * thd * thd + 0.001 * u * u;
        const double nthd = clip(thd + (15.0 * sin(th) + 3.0 * u) * 0.05, -8.0, 8.0);
        s[0] = th + nthd * 0.05;
        s[1] = nthd;
        term = false;
        rew = (float)(-cost);
    }
}

inline bool known_control_kind(int kind) { return kind >= CARTPOLE && kind <= PENDULUM; }

}  // namespace ppox
