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
#include "control_dyn.h"
#include "episode.h"
#include "philox.h"

namespace {

using ppox::Episode;
using ppox::episode_update;

using ppox::ACROBOT;
using ppox::CARTPOLE;
using ppox::Dims;
using ppox::draw_state;
using ppox::MOUNTAINCAR;
using ppox::PENDULUM;
using ppox::physics;
using ppox::RESET_ACTION;
using ppox::write_obs;

constexpr uint32_t EVENT_BLOCK = 0xFFFFFFFFu;

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

}  // namespace

extern "C" int ppox_control_env_reset(int32_t kind, double* state, int32_t* episode, float* obs, int64_t N,
                                      int64_t env_offset, uint64_t seed, float* ep_ret, int32_t* ep_len,
                                      void* stream) {
    PPOX_REQUIRE(ppox::known_control_kind(kind), "ppox_control_env_reset: unknown kind %d", (int)kind);
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
    PPOX_REQUIRE(ppox::known_control_kind(kind), "ppox_control_env_step: unknown kind %d", (int)kind);
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
