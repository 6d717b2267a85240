// Device environments with real dynamics: the gym classic-control tasks (CartPole, MountainCar,
// Acrobot, Pendulum) and Catch, a pixel task for the NatureCNN path.  The equations are the
// published gym classic-control tasks restated (DESIGN.md "Real-dynamics envs" is the
// specification; gym itself is not available, so parity with gym is unpinned — the parity that
// is pinned is with tests/real_env_twin.py, the numpy restatement of the same equations).
//
// Classic control: one thread per env, float64 state (N, S) owned by the caller, float32
// observation (N, D).  The build sets -ffp-contract=off and these kernels use no explicit fma:
// every operation rounds once, as the numpy twin's does, so the two differ only in the last
// ulp of sin/cos.
//
// Reset draw: philox4x32_10({0, GLOBAL env id, episode index, RESET_ACTION}, seed); component j
// of the state = lo_j + (hi_j - lo_j) * (double)u01(word_j).  Keyed by the global id, so a rank
// holding envs [off, off+n) produces exactly that slice of the one-GPU run.
//
// Step: physics -> reward, terminated -> done = terminated || ep_len + 1 >= max_len -> on done
// the episode is recorded, the episode index incremented and the state redrawn, and the
// observation written is the NEW episode's first (SB3 VecEnv auto-reset); the reward is the
// terminal step's.
#include "common.h"
#include "episode.h"
#include "philox.h"

namespace {

using ppox::Episode;
using ppox::episode_update;

constexpr uint32_t EVENT_BLOCK = 0xFFFFFFFFu;
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

template <int KIND>
__global__ void __launch_bounds__(256) control_reset_kernel(double* __restrict__ state, int32_t* __restrict__ episode,
                                                            float* __restrict__ obs, long long N, long long env_offset,
                                                            uint32_t k0, uint32_t k1, Episode ep) {
    constexpr int S = Dims<KIND>::S, D = Dims<KIND>::D;
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double s[4];
    draw_state<KIND>(s, (uint32_t)(env_offset + n), 0u, k0, k1);
#pragma unroll
    for (int j = 0; j < S; ++j) state[n * S + j] = s[j];
    episode[n] = 0;
    write_obs<KIND>(s, obs + n * D);
    ep.ep_ret[n] = 0.f;
    ep.ep_len[n] = 0;
}

template <int KIND>
__global__ void __launch_bounds__(256) control_step_kernel(double* __restrict__ state, int32_t* __restrict__ episode,
                                                           const void* __restrict__ actions, float* __restrict__ obs,
                                                           long long N, long long env_offset, uint32_t k0, uint32_t k1,
                                                           int max_len, float* __restrict__ rewards,
                                                           uint8_t* __restrict__ dones, Episode ep) {
    constexpr int S = Dims<KIND>::S, D = Dims<KIND>::D;
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double s[4];
#pragma unroll
    for (int j = 0; j < S; ++j) s[j] = state[n * S + j];
    const int ai = KIND == PENDULUM ? 0 : static_cast<const int32_t*>(actions)[n];
    const float af = KIND == PENDULUM ? static_cast<const float*>(actions)[n] : 0.f;
    float rew;
    bool term;
    physics<KIND>(s, ai, af, rew, term);
    const bool done = term || ep.ep_len[n] + 1 >= max_len;
    if (done) {
        const int32_t e = episode[n] + 1;
        episode[n] = e;
        draw_state<KIND>(s, (uint32_t)(env_offset + n), (uint32_t)e, k0, k1);
    }
#pragma unroll
    for (int j = 0; j < S; ++j) state[n * S + j] = s[j];
    write_obs<KIND>(s, obs + n * D);
    rewards[n] = rew;
    dones[n] = done ? 1 : 0;
    episode_update(ep, n, rew, done);
}

// ---------------------------------------------------------------------------------------------
// Catch: a ball falls down a 12 x 12 grid (cells of 7 x 7 pixels) and a 3-cell paddle on the
// bottom row has to be under it.  state (N, 4) int32 = ball column, ball row, ball dx, paddle
// column.  One block per env; the frame stack is handled as atari_step_kernel's (env.hip).
constexpr int FRAME = 84 * 84;
constexpr int CHUNKS = FRAME / 16;  // 441
constexpr int GRID = 12, CELL = 7;

struct CatchState {
    int col, row, dx, pad;
};

__device__ inline CatchState catch_draw(uint32_t gid, uint32_t episode, uint32_t k0, uint32_t k1) {
    const ppox::u32x4 w = ppox::philox4x32_10(ppox::u32x4{EVENT_BLOCK, gid, episode, RESET_ACTION}, k0, k1);
    return CatchState{(int)(w.x % GRID), 0, (int)(w.y % 3) - 1, 1 + (int)(w.z % 10)};
}

// 16 pixels of the frame, from pixel 16 * c: ball cell 255, the three paddle cells (bottom row) 128
__device__ inline uint4 catch_chunk(const CatchState& st, int c) {
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int p = c * 16 + i;
        const int cr = (p / 84) / CELL, cc = (p % 84) / CELL;
        const int d = cc - st.pad;
        const uint32_t v = (cr == st.row && cc == st.col) ? 255u : ((cr == GRID - 1 && d >= -1 && d <= 1) ? 128u : 0u);
        w[i >> 2] |= v << (8 * (i & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ void __launch_bounds__(256) catch_reset_kernel(uint8_t* __restrict__ obs, int32_t* __restrict__ state,
                                                          int32_t* __restrict__ episode, long long env_offset,
                                                          uint32_t k0, uint32_t k1, Episode ep) {
    const long long n = blockIdx.x;
    const CatchState st = catch_draw((uint32_t)(env_offset + n), 0u, k0, k1);
    uint4* o = reinterpret_cast<uint4*>(obs + n * 4LL * FRAME);
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (int c = threadIdx.x; c < CHUNKS; c += blockDim.x) {
        o[c] = z;
        o[CHUNKS + c] = z;
        o[2 * CHUNKS + c] = z;
        o[3 * CHUNKS + c] = catch_chunk(st, c);
    }
    if (threadIdx.x == 0) {
        state[n * 4 + 0] = st.col, state[n * 4 + 1] = st.row, state[n * 4 + 2] = st.dx, state[n * 4 + 3] = st.pad;
        episode[n] = 0;
        if (ep.ep_ret) {
            ep.ep_ret[n] = 0.f;
            ep.ep_len[n] = 0;
        }
    }
}

__global__ void __launch_bounds__(256) catch_step_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                         const int32_t* __restrict__ actions,
                                                         int32_t* __restrict__ state, int32_t* __restrict__ episode,
                                                         long long env_offset, uint32_t k0, uint32_t k1,
                                                         float* __restrict__ rewards, uint8_t* __restrict__ dones,
                                                         Episode ep) {
    const long long n = blockIdx.x;
    // every thread derives the same next state from the stored one; thread 0 stores it after the barrier
    CatchState st{state[n * 4 + 0], state[n * 4 + 1], state[n * 4 + 2], state[n * 4 + 3]};
    int32_t e = episode[n];
    const int a = actions[n];
    __syncthreads();
    st.pad += a == 1 ? -1 : (a == 2 ? 1 : 0);
    st.pad = st.pad < 1 ? 1 : (st.pad > GRID - 2 ? GRID - 2 : st.pad);
    st.row += 1;
    st.col += st.dx;
    if (st.col < 0) {
        st.col = -st.col;
        st.dx = -st.dx;
    } else if (st.col > GRID - 1) {
        st.col = 2 * (GRID - 1) - st.col;
        st.dx = -st.dx;
    }
    const bool done = st.row >= GRID - 1;
    const int miss = st.col - st.pad;
    const float rew = done ? ((miss >= -1 && miss <= 1) ? 1.f : -1.f) : 0.f;
    if (done) {
        e += 1;
        st = catch_draw((uint32_t)(env_offset + n), (uint32_t)e, k0, k1);
    }
    const uint4* s = reinterpret_cast<const uint4*>(in + n * 4LL * FRAME);
    uint4* o = reinterpret_cast<uint4*>(out + n * 4LL * FRAME);
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (int c = threadIdx.x; c < CHUNKS; c += blockDim.x) {
        const uint4 f1 = done ? z : s[CHUNKS + c];
        const uint4 f2 = done ? z : s[2 * CHUNKS + c];
        const uint4 f3 = done ? z : s[3 * CHUNKS + c];
        o[c] = f1;
        o[CHUNKS + c] = f2;
        o[2 * CHUNKS + c] = f3;
        o[3 * CHUNKS + c] = catch_chunk(st, c);
    }
    if (threadIdx.x == 0) {
        state[n * 4 + 0] = st.col, state[n * 4 + 1] = st.row, state[n * 4 + 2] = st.dx, state[n * 4 + 3] = st.pad;
        episode[n] = e;
        rewards[n] = rew;
        dones[n] = done ? 1 : 0;
        episode_update(ep, n, rew, done);
    }
}

inline bool known_kind(int kind) { return kind >= CARTPOLE && kind <= PENDULUM; }

}  // namespace

extern "C" int ppox_control_env_reset(int32_t kind, double* state, int32_t* episode, float* obs, int64_t N,
                                      int64_t env_offset, uint64_t seed, float* ep_ret, int32_t* ep_len,
                                      void* stream) {
    PPOX_REQUIRE(known_kind(kind), "ppox_control_env_reset: unknown kind %d", (int)kind);
    PPOX_REQUIRE(state && episode && obs && ep_ret && ep_len, "ppox_control_env_reset: null pointer");
    PPOX_REQUIRE(N > 0 && env_offset >= 0, "ppox_control_env_reset: N must be positive, env_offset non-negative");
    const Episode ep{ep_ret, ep_len, nullptr, nullptr};
    const dim3 grid(ppox::ceil_div(N, 256));
    hipStream_t s = ppox::as_stream(stream);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#define PPOX_RESET(K) control_reset_kernel<K><<<grid, 256, 0, s>>>(state, episode, obs, N, env_offset, k0, k1, ep)
    switch (kind) {
        case CARTPOLE: PPOX_RESET(CARTPOLE); break;
        case MOUNTAINCAR: PPOX_RESET(MOUNTAINCAR); break;
        case ACROBOT: PPOX_RESET(ACROBOT); break;
        default: PPOX_RESET(PENDULUM); break;
    }
#undef PPOX_RESET
    PPOX_LAUNCHED("ppox_control_env_reset");
}

extern "C" int ppox_control_env_step(int32_t kind, double* state, int32_t* episode, const void* actions, float* obs,
                                     int64_t N, int64_t env_offset, uint64_t seed, int32_t max_len, float* rewards,
                                     uint8_t* dones, float* ep_ret, int32_t* ep_len, float* done_ret,
                                     int32_t* done_len, void* stream) {
    PPOX_REQUIRE(known_kind(kind), "ppox_control_env_step: unknown kind %d", (int)kind);
    PPOX_REQUIRE(state && episode && actions && obs && rewards && dones && ep_ret && ep_len,
                 "ppox_control_env_step: null pointer");
    PPOX_REQUIRE(N > 0 && env_offset >= 0, "ppox_control_env_step: N must be positive, env_offset non-negative");
    PPOX_REQUIRE(max_len > 0, "ppox_control_env_step: max_len must be positive");
    const Episode ep{ep_ret, ep_len, done_ret, done_len};
    const dim3 grid(ppox::ceil_div(N, 256));
    hipStream_t s = ppox::as_stream(stream);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#define PPOX_STEP(K)                                                                                          \
    control_step_kernel<K><<<grid, 256, 0, s>>>(state, episode, actions, obs, N, env_offset, k0, k1, max_len, \
                                                rewards, dones, ep)
    switch (kind) {
        case CARTPOLE: PPOX_STEP(CARTPOLE); break;
        case MOUNTAINCAR: PPOX_STEP(MOUNTAINCAR); break;
        case ACROBOT: PPOX_STEP(ACROBOT); break;
        default: PPOX_STEP(PENDULUM); break;
    }
#undef PPOX_STEP
    PPOX_LAUNCHED("ppox_control_env_step");
}

extern "C" int ppox_catch_env_reset(uint8_t* obs, int32_t* state, int32_t* episode, int64_t N, int64_t env_offset,
                                    uint64_t seed, float* ep_ret, int32_t* ep_len, void* stream) {
    PPOX_REQUIRE(obs && state && episode && N > 0 && env_offset >= 0, "ppox_catch_env_reset: bad arguments");
    PPOX_REQUIRE(ppox::aligned16(obs), "ppox_catch_env_reset: obs must be 16B aligned");
    PPOX_REQUIRE((ep_ret == nullptr) == (ep_len == nullptr), "ppox_catch_env_reset: ep_ret/ep_len pair");
    const Episode ep{ep_ret, ep_len, nullptr, nullptr};
    catch_reset_kernel<<<(unsigned)N, 256, 0, ppox::as_stream(stream)>>>(obs, state, episode, env_offset,
                                                                         (uint32_t)seed, (uint32_t)(seed >> 32), ep);
    PPOX_LAUNCHED("ppox_catch_env_reset");
}

extern "C" int ppox_catch_env_step(const uint8_t* obs_in, uint8_t* obs_out, const int32_t* actions, int32_t* state,
                                   int32_t* episode, int64_t N, int64_t env_offset, uint64_t seed, float* rewards,
                                   uint8_t* dones, float* ep_ret, int32_t* ep_len, float* done_ret, int32_t* done_len,
                                   void* stream) {
    PPOX_REQUIRE(obs_in && obs_out && actions && state && episode && rewards && dones,
                 "ppox_catch_env_step: null pointer");
    PPOX_REQUIRE(N > 0 && env_offset >= 0, "ppox_catch_env_step: N must be positive, env_offset non-negative");
    PPOX_REQUIRE(ppox::aligned16(obs_in) && ppox::aligned16(obs_out), "ppox_catch_env_step: obs must be 16B aligned");
    PPOX_REQUIRE((ep_ret == nullptr) == (ep_len == nullptr), "ppox_catch_env_step: ep_ret/ep_len pair");
    const Episode ep{ep_ret, ep_len, done_ret, done_len};
    catch_step_kernel<<<(unsigned)N, 256, 0, ppox::as_stream(stream)>>>(obs_in, obs_out, actions, state, episode,
                                                                        env_offset, (uint32_t)seed,
                                                                        (uint32_t)(seed >> 32), rewards, dones, ep);
    PPOX_LAUNCHED("ppox_catch_env_step");
}
