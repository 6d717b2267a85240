// KeyDoor-v0: a sparse-reward pixel gridworld of the Atari observation shape (DESIGN.md §11 is the
// specification; tests/keydoor_twin.py the numpy restatement the kernels are held to).
//
// A 12 x 12 grid of 7 x 7-pixel cells (Catch's geometry): the border ring is wall, column 6 a
// dividing wall with one door cell, the left room holds the key and every start, the right room
// the goal.  The layout is one per seed (ppox_keydoor_layout), shared by every env and episode,
// so the visit-count table `visits` (2, 12, 12) int64 = [has_key][row][col] means something
// across episodes and shards.  state (N, 4) int32 = row, column, has_key, 0.
//
// One block of 256 threads per env, as catch_step_kernel: every thread derives the next state
// from the stored one, the first 144 threads build the cell values in LDS, and after the barrier
// each thread expands its 16-byte chunks from that table while thread 0 stores the state and
// counts the visit (a 64-bit vector atomicAdd: integer adds commute, the table is exact).
#include "common.h"
#include "episode.h"
#include "philox.h"

namespace {

using ppox::Episode;
using ppox::episode_update;

constexpr uint32_t EVENT_BLOCK = 0xFFFFFFFFu;
constexpr uint32_t RESET_ACTION = 0xFFFFFFFFu;
constexpr uint32_t LAYOUT_GID = 0xFFFFFFFFu;  // the layout's counter word: no env id reaches it (entry-point check)

constexpr int FRAME = 84 * 84;
constexpr int CHUNKS = FRAME / 16;  // 441
constexpr int GRID = 12, CELL = 7, CELLS = GRID * GRID;
constexpr int DIVIDER = 6;  // the dividing wall's column

struct Layout {
    int door_row, key_row, key_col, goal_row, goal_col;
};

struct GridState {
    int row, col, has_key;
};

__host__ __device__ inline Layout keydoor_layout(uint32_t k0, uint32_t k1) {
    const ppox::u32x4 w = ppox::philox4x32_10(ppox::u32x4{EVENT_BLOCK, LAYOUT_GID, 0u, RESET_ACTION}, k0, k1);
    return Layout{1 + (int)(w.x % 10), 1 + (int)(w.y % 10), 1 + (int)((w.y >> 16) % 5), 1 + (int)(w.z % 10),
                  7 + (int)((w.z >> 16) % 4)};
}

// the start of episode `episode` of env `gid`: a left-room cell; the key is held at once if it lies there
__device__ inline GridState keydoor_draw(const Layout& L, uint32_t gid, uint32_t episode, uint32_t k0, uint32_t k1) {
    const ppox::u32x4 w = ppox::philox4x32_10(ppox::u32x4{EVENT_BLOCK, gid, episode, RESET_ACTION}, k0, k1);
    const int row = 1 + (int)(w.x % 10), col = 1 + (int)(w.y % 5);
    return GridState{row, col, (row == L.key_row && col == L.key_col) ? 1 : 0};
}

__device__ inline bool is_wall(const Layout& L, int r, int c) {
    return r <= 0 || r >= GRID - 1 || c <= 0 || c >= GRID - 1 || (c == DIVIDER && r != L.door_row);
}

// a later rule wins a shared cell: floor 0, wall 64, closed door 96, key 192 (both 0 once the key is held),
// goal 160, agent 255
__device__ inline uint8_t cell_value(const Layout& L, const GridState& st, int r, int c) {
    uint8_t v = is_wall(L, r, c) ? 64 : 0;
    if (r == L.door_row && c == DIVIDER) v = st.has_key ? 0 : 96;
    if (r == L.key_row && c == L.key_col) v = st.has_key ? 0 : 192;
    if (r == L.goal_row && c == L.goal_col) v = 160;
    if (r == st.row && c == st.col) v = 255;
    return v;
}

// 16 pixels of the frame, from pixel 16 * c, out of the block's cell table; indexed per pixel, since
// a chunk can straddle a pixel row (84 is no multiple of 16)
__device__ inline uint4 grid_chunk(const uint8_t* cells, int c) {
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int p = c * 16 + i;
        const uint32_t v = cells[((p / 84) / CELL) * GRID + (p % 84) / CELL];
        w[i >> 2] |= v << (8 * (i & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// (a state tensor the caller overwrote with cells off the grid is not counted)
__device__ inline void count_visit(unsigned long long* visits, const GridState& st) {
    if ((unsigned)st.row < (unsigned)GRID && (unsigned)st.col < (unsigned)GRID)
        atomicAdd(visits + (st.has_key * GRID + st.row) * GRID + st.col, 1ull);
}

__global__ void __launch_bounds__(256) keydoor_reset_kernel(uint8_t* __restrict__ obs, int32_t* __restrict__ state,
                                                            int32_t* __restrict__ episode,
                                                            unsigned long long* __restrict__ visits,
                                                            long long env_offset, uint32_t k0, uint32_t k1, Layout L,
                                                            Episode ep) {
    __shared__ uint8_t cells[CELLS];
    const long long n = blockIdx.x;
    const GridState st = keydoor_draw(L, (uint32_t)(env_offset + n), 0u, k0, k1);
    if (threadIdx.x < CELLS) cells[threadIdx.x] = cell_value(L, st, threadIdx.x / GRID, threadIdx.x % GRID);
    __syncthreads();
    uint4* o = reinterpret_cast<uint4*>(obs + n * 4LL * FRAME);
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (int c = threadIdx.x; c < CHUNKS; c += blockDim.x) {
        o[c] = z;
        o[CHUNKS + c] = z;
        o[2 * CHUNKS + c] = z;
        o[3 * CHUNKS + c] = grid_chunk(cells, c);
    }
    if (threadIdx.x == 0) {
        state[n * 4 + 0] = st.row, state[n * 4 + 1] = st.col, state[n * 4 + 2] = st.has_key, state[n * 4 + 3] = 0;
        episode[n] = 0;
        count_visit(visits, st);
        if (ep.ep_ret) {
            ep.ep_ret[n] = 0.f;
            ep.ep_len[n] = 0;
        }
    }
}

__global__ void __launch_bounds__(256) keydoor_step_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                           const int32_t* __restrict__ actions,
                                                           int32_t* __restrict__ state, int32_t* __restrict__ episode,
                                                           unsigned long long* __restrict__ visits,
                                                           long long env_offset, uint32_t k0, uint32_t k1, Layout L,
                                                           int max_len, float* __restrict__ rewards,
                                                           uint8_t* __restrict__ dones, Episode ep) {
    __shared__ uint8_t cells[CELLS];
    const long long n = blockIdx.x;
    // every thread derives the same next state from the stored one; thread 0 stores it after the barrier
    GridState st{state[n * 4 + 0], state[n * 4 + 1], state[n * 4 + 2] != 0 ? 1 : 0};
    int32_t e = episode[n];
    const int a = actions[n];
    const int len = ep.ep_len ? ep.ep_len[n] : 0;
    const int tr = st.row + (a == 1 ? -1 : (a == 2 ? 1 : 0));
    const int tc = st.col + (a == 3 ? -1 : (a == 4 ? 1 : 0));
    const bool refused = is_wall(L, tr, tc) || (tr == L.door_row && tc == DIVIDER && !st.has_key);
    if (!refused) st.row = tr, st.col = tc;
    if (st.row == L.key_row && st.col == L.key_col) st.has_key = 1;
    const bool reached = st.row == L.goal_row && st.col == L.goal_col;
    const float rew = reached ? 1.f : 0.f;
    const bool done = reached || len + 1 >= max_len;
    const GridState visited = st;  // the state just reached, counted before any reset
    if (done) {
        e += 1;
        st = keydoor_draw(L, (uint32_t)(env_offset + n), (uint32_t)e, k0, k1);
    }
    if (threadIdx.x < CELLS) cells[threadIdx.x] = cell_value(L, st, threadIdx.x / GRID, threadIdx.x % GRID);
    __syncthreads();
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
        o[3 * CHUNKS + c] = grid_chunk(cells, c);
    }
    if (threadIdx.x == 0) {
        state[n * 4 + 0] = st.row, state[n * 4 + 1] = st.col, state[n * 4 + 2] = st.has_key, state[n * 4 + 3] = 0;
        episode[n] = e;
        rewards[n] = rew;
        dones[n] = done ? 1 : 0;
        count_visit(visits, visited);
        if (done) count_visit(visits, st);
        episode_update(ep, n, rew, done);
    }
}

// env ids are Philox counter words below the layout's: env_offset + N < 0xFFFFFFFF
inline bool gids_fit(int64_t N, int64_t env_offset) {
    return env_offset < (int64_t)LAYOUT_GID && N < (int64_t)LAYOUT_GID - env_offset;
}

}  // namespace

extern "C" int ppox_keydoor_layout(uint64_t seed, int32_t* out5) {
    PPOX_REQUIRE(out5, "ppox_keydoor_layout: null pointer");
    const Layout L = keydoor_layout((uint32_t)seed, (uint32_t)(seed >> 32));
    out5[0] = L.door_row, out5[1] = L.key_row, out5[2] = L.key_col, out5[3] = L.goal_row, out5[4] = L.goal_col;
    return PPOX_OK;
}

extern "C" int ppox_keydoor_env_reset(uint8_t* obs, int32_t* state, int32_t* episode, int64_t* visits, int64_t N,
                                      int64_t env_offset, uint64_t seed, float* ep_ret, int32_t* ep_len,
                                      void* stream) {
    PPOX_REQUIRE(obs && state && episode && visits, "ppox_keydoor_env_reset: null pointer");
    PPOX_REQUIRE(N > 0 && env_offset >= 0, "ppox_keydoor_env_reset: N must be positive, env_offset non-negative");
    PPOX_REQUIRE(gids_fit(N, env_offset), "ppox_keydoor_env_reset: env_offset + N must be below 0xFFFFFFFF");
    PPOX_REQUIRE(ppox::aligned16(obs), "ppox_keydoor_env_reset: obs must be 16B aligned");
    PPOX_REQUIRE((ep_ret == nullptr) == (ep_len == nullptr), "ppox_keydoor_env_reset: ep_ret/ep_len pair");
    const Episode ep{ep_ret, ep_len, nullptr, nullptr};
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    keydoor_reset_kernel<<<(unsigned)N, 256, 0, ppox::as_stream(stream)>>>(
        obs, state, episode, reinterpret_cast<unsigned long long*>(visits), env_offset, k0, k1, keydoor_layout(k0, k1),
        ep);
    PPOX_LAUNCHED("ppox_keydoor_env_reset");
}

extern "C" int ppox_keydoor_env_step(const uint8_t* obs_in, uint8_t* obs_out, const int32_t* actions, int32_t* state,
                                     int32_t* episode, int64_t* visits, int64_t N, int64_t env_offset, uint64_t seed,
                                     int32_t max_len, float* rewards, uint8_t* dones, float* ep_ret, int32_t* ep_len,
                                     float* done_ret, int32_t* done_len, void* stream) {
    PPOX_REQUIRE(obs_in && obs_out && actions && state && episode && visits && rewards && dones,
                 "ppox_keydoor_env_step: null pointer");
    PPOX_REQUIRE(N > 0 && env_offset >= 0, "ppox_keydoor_env_step: N must be positive, env_offset non-negative");
    PPOX_REQUIRE(gids_fit(N, env_offset), "ppox_keydoor_env_step: env_offset + N must be below 0xFFFFFFFF");
    PPOX_REQUIRE(max_len > 0, "ppox_keydoor_env_step: max_len must be positive");
    PPOX_REQUIRE(ppox::aligned16(obs_in) && ppox::aligned16(obs_out),
                 "ppox_keydoor_env_step: obs must be 16B aligned");
    PPOX_REQUIRE((ep_ret == nullptr) == (ep_len == nullptr), "ppox_keydoor_env_step: ep_ret/ep_len pair");
    const Episode ep{ep_ret, ep_len, done_ret, done_len};
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    keydoor_step_kernel<<<(unsigned)N, 256, 0, ppox::as_stream(stream)>>>(
        obs_in, obs_out, actions, state, episode, reinterpret_cast<unsigned long long*>(visits), env_offset, k0, k1,
        keydoor_layout(k0, k1), max_len, rewards, dones, ep);
    PPOX_LAUNCHED("ppox_keydoor_env_step");
}
