"""Numpy twin of KeyDoor-v0 (ppo-exploration_amd/csrc/env_grid.hip), written from the rules of
DESIGN.md §11 on oracle.philox, in the shape of real_env_twin.CatchTwin.  It also keeps the
visit-count table, counts the events of every step (so a test can tell which branches a run
took), and provides a shortest-path policy and the tests' action stream.  Test infrastructure only.
"""
import numpy as np

from oracle import philox as P

GRID, CELL, DIVIDER = 12, 7, 6
N_ACTIONS = 5
MOVES = np.array([[0, 0], [-1, 0], [1, 0], [0, -1], [0, 1]])  # stay, up, down, left, right: (d row, d column)
LAYOUT_GID = 0xFFFFFFFF
FLOOR, WALL, DOOR, KEY, GOAL, AGENT = 0, 64, 96, 192, 160, 255
EVENTS = ("key_pickups", "refused_doors", "door_passages", "wall_bumps", "goals", "time_limits", "key_starts")

# the shape of the GPU parity run (test_keydoor_gpu.py); test_keydoor_twin.py checks on the CPU that the
# twin's own run with this seed takes every branch at least three times
PARITY_N, PARITY_T, PARITY_MAX_LEN, PARITY_SEED = 67, 64, 40, 11
# the seeds the GPU tests construct envs with: the random-policy success rate is asserted below 10 % for each
GPU_TEST_SEEDS = (11, 5)
ACTION_STREAM = 0x0AC711  # counter word that keeps the tests' action draws apart from the env's own


def _key(seed):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def layout(seed):
    """door_row, key (row, column), goal (row, column) from philox({EVENT_BLOCK, 0xFFFFFFFF, 0, RESET_ACTION}, seed)."""
    k0, k1 = _key(seed)
    w = P.philox4x32_10(np.uint32(P.EVENT_BLOCK), np.uint32(LAYOUT_GID), np.uint32(0), np.uint32(P.RESET_ACTION),
                        k0, k1)
    x, y, z = (int(v) for v in w[:3])
    return {"door_row": 1 + x % 10, "key": (1 + y % 10, 1 + (y >> 16) % 5), "goal": (1 + z % 10, 7 + (z >> 16) % 4)}


def wall_mask(lay):
    """(12, 12) bool: the border ring and column 6 except the door cell."""
    m = np.zeros((GRID, GRID), bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    m[:, DIVIDER] = True
    m[lay["door_row"], DIVIDER] = False
    return m


def reset_state(seed, gids, episodes, lay):
    """(n, 4) int32 = row, column, has_key, 0 from philox({EVENT_BLOCK, global env id, episode index, RESET_ACTION}, seed)."""
    k0, k1 = _key(seed)
    w = P.philox4x32_10(np.uint32(P.EVENT_BLOCK), np.asarray(gids, np.uint32), np.asarray(episodes, np.uint32),
                        np.uint32(P.RESET_ACTION), k0, k1)
    row = 1 + (w[0] % np.uint32(10)).astype(np.int32)
    col = 1 + (w[1] % np.uint32(5)).astype(np.int32)
    has = ((row == lay["key"][0]) & (col == lay["key"][1])).astype(np.int32)
    return np.stack([row, col, has, np.zeros_like(row)], axis=-1).astype(np.int32)


def physics(state, actions, lay):
    """-> (next state before any reset, reward f32, reached, events: dict of (n,) bool)."""
    s = np.array(state, np.int64)
    a = np.asarray(actions).reshape(-1).astype(np.int64)
    a = np.where((a >= 0) & (a < N_ACTIONS), a, 0)
    row, col, has = s[:, 0], s[:, 1], s[:, 2] != 0
    tr, tc = row + MOVES[a, 0], col + MOVES[a, 1]
    walls = wall_mask(lay)
    bump = walls[np.clip(tr, 0, GRID - 1), np.clip(tc, 0, GRID - 1)]
    at_door = (tr == lay["door_row"]) & (tc == DIVIDER)
    shut = at_door & ~has
    moved = ~(bump | shut)
    row, col = np.where(moved, tr, row), np.where(moved, tc, col)
    on_key = (row == lay["key"][0]) & (col == lay["key"][1])
    picked = on_key & ~has
    has = has | on_key
    reached = (row == lay["goal"][0]) & (col == lay["goal"][1])
    rew = np.where(reached, 1.0, 0.0).astype(np.float32)
    ev = dict(key_pickups=picked, refused_doors=shut, door_passages=at_door & moved & (a != 0), wall_bumps=bump)
    nxt = np.stack([row, col, has.astype(np.int64), np.zeros_like(row)], axis=-1).astype(np.int32)
    return nxt, rew, reached, ev


def cells(state, lay):
    """(n, 12, 12) uint8 cell values; a later rule wins a shared cell."""
    n = state.shape[0]
    base = np.where(wall_mask(lay), WALL, FLOOR).astype(np.uint8)
    out = np.repeat(base[None], n, axis=0)
    has = state[:, 2] != 0
    out[:, lay["door_row"], DIVIDER] = np.where(has, FLOOR, DOOR)
    out[:, lay["key"][0], lay["key"][1]] = np.where(has, FLOOR, KEY)
    out[:, lay["goal"][0], lay["goal"][1]] = GOAL
    out[np.arange(n), state[:, 0], state[:, 1]] = AGENT
    return out


def frame(state, lay):
    """(n, 84, 84) uint8: every cell a 7 x 7 block of its value."""
    return np.repeat(np.repeat(cells(state, lay), CELL, axis=1), CELL, axis=2)


def count_visits(visits, state):
    np.add.at(visits, (state[:, 2], state[:, 0], state[:, 1]), 1)


class KeyDoorTwin:
    """render=False skips the frames (the long random-policy runs need only the dynamics)."""

    def __init__(self, n_envs, seed=0, env_offset=0, max_len=200, render=True):
        self.num_envs, self.seed, self.max_len, self.render = n_envs, seed, max_len, render
        self.gids = np.arange(env_offset, env_offset + n_envs)
        self.layout = layout(seed)
        self.visits = np.zeros((2, GRID, GRID), np.int64)
        self.counts = dict.fromkeys(EVENTS, 0)
        self.reset()

    def reset(self):
        n = self.num_envs
        self.episode = np.zeros(n, np.int32)
        self.state = reset_state(self.seed, self.gids, self.episode, self.layout)
        self.ep_ret = np.zeros(n, np.float32)
        self.ep_len = np.zeros(n, np.int32)
        count_visits(self.visits, self.state)
        self.counts["key_starts"] += int(self.state[:, 2].sum())
        self.obs = np.zeros((n, 4, 84, 84) if self.render else (n, 0), np.uint8)
        if self.render:
            self.obs[:, 3] = frame(self.state, self.layout)
        return self.obs.copy()

    def step(self, actions):
        s, rew, reached, ev = physics(self.state, actions, self.layout)
        ln = self.ep_len + 1
        done = reached | (ln >= self.max_len)
        ret = (self.ep_ret + rew).astype(np.float32)
        done_ret = np.where(done, ret, np.float32(np.nan)).astype(np.float32)
        done_len = np.where(done, ln, 0).astype(np.int32)
        self.ep_ret = np.where(done, np.float32(0), ret).astype(np.float32)
        self.ep_len = np.where(done, 0, ln).astype(np.int32)
        count_visits(self.visits, s)
        self.episode = (self.episode + done).astype(np.int32)
        fresh = reset_state(self.seed, self.gids, self.episode, self.layout)
        count_visits(self.visits, fresh[done])
        self.state = np.where(done[:, None], fresh, s)
        ev = dict(ev, goals=reached, time_limits=done & ~reached, key_starts=done & (fresh[:, 2] != 0))
        for k, v in ev.items():
            self.counts[k] += int(v.sum())
        nxt = np.empty_like(self.obs)
        if self.render:
            nxt[:, :3] = self.obs[:, 1:]
            nxt[done, :3] = 0
            nxt[:, 3] = frame(self.state, self.layout)
        self.obs = nxt
        return dict(obs=nxt.copy(), reward=rew, done=done, reached=reached, done_ret=done_ret, done_len=done_len,
                    pre_reset_state=s, events=ev)


# ------------------------------------------------------------------------------------- policies
def bfs_policy(lay):
    """(2, 12, 12) int32 = [has_key][row][column] -> the first action of a shortest path to the goal over
    (row, column, has_key), and the (2, 12, 12) distances (-1: wall cells and states that cannot occur)."""
    walls = wall_mask(lay)
    states = [(h, r, c) for h in (0, 1) for r in range(GRID) for c in range(GRID) if not walls[r, c]]
    idx = np.array([[r, c, h, 0] for h, r, c in states], np.int32)
    nxt = np.stack([physics(idx, np.full(len(states), a), lay)[0] for a in range(N_ACTIONS)])  # (5, S, 4)
    dist = np.full((2, GRID, GRID), -1, np.int64)
    dist[:, lay["goal"][0], lay["goal"][1]] = 0
    for d in range(1, 2 * GRID * GRID):  # breadth first: the states whose best successor is at distance d - 1
        grew = False
        for i, (h, r, c) in enumerate(states):
            if dist[h, r, c] < 0 and any(dist[n[2], n[0], n[1]] == d - 1 for n in nxt[1:, i]):
                dist[h, r, c] = d
                grew = True
        if not grew:
            break
    policy = np.zeros((2, GRID, GRID), np.int32)
    for i, (h, r, c) in enumerate(states):
        if dist[h, r, c] > 0:
            policy[h, r, c] = 1 + next(a for a, n in enumerate(nxt[1:, i]) if dist[n[2], n[0], n[1]] == dist[h, r, c] - 1)
    return policy, dist


def draw_actions(seed, gids, t, state=None, policy=None):
    """The tests' actions at step t for global env ids `gids`, from philox({t, gid, ACTION_STREAM, 0}, seed):
    uniform over the five actions (word 0), except that an env with an even global id takes the shortest-path
    action of `policy` for its `state` with probability 1/2 (bit 0 of word 1).  A uniform stream alone hardly
    ever reaches the goal, a guided one alone never walks into the shut door.  Without a policy: uniform."""
    k0, k1 = _key(seed)
    gids = np.asarray(gids)
    w = P.philox4x32_10(np.uint32(t), gids.astype(np.uint32), np.uint32(ACTION_STREAM), np.uint32(0), k0, k1)
    a = (w[0] % np.uint32(N_ACTIONS)).astype(np.int32)
    if policy is None:
        return a
    guided = (gids % 2 == 0) & ((w[1] & np.uint32(1)) == 1)
    return np.where(guided, policy[state[:, 2], state[:, 0], state[:, 1]], a).astype(np.int32)


def random_policy_rate(seed, max_len=200, n_envs=256, steps=2000, action_seed=None):
    """(goal rate, episodes): the fraction of finished episodes of a uniform random policy that reached the goal."""
    tw = KeyDoorTwin(n_envs, seed=seed, max_len=max_len, render=False)
    for t in range(1, steps + 1):
        tw.step(draw_actions(seed if action_seed is None else action_seed, tw.gids, t))
    episodes = tw.counts["goals"] + tw.counts["time_limits"]
    return tw.counts["goals"] / episodes, episodes
