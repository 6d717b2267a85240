"""Device-resident rollout storage with the reference's interface
(reference: buffer.py:13-490 — RolloutStorage, IntrinsicStorage, PrioritizedReplayBuffer).

Layout in HBM, per rank (T = buffer_size, N = n_envs on this rank), STEP-MAJOR
like the reference's (buffer_size, n_envs, ...) arrays:
  obs_slots     (T+1, N, *obs)  uint8 frames (Atari) / f32 — slot t+1 is written
                                by the env step that consumes slot t; slot T is
                                the next rollout's first observation
  actions       (T, N) int32 (Discrete) or (T, N, A) f32 (Box)
  rewards, values, log_probs (T, N) f32 ((T, N, A) log_probs for Box)
  masks         (T, N) uint8  — done flag of transition t (buffer.py:180 / ppo.py:192)
  advantages, returns (T, N) f32  (+ int_* for IntrinsicStorage)
Minibatches use the reference's ENV-MAJOR flat index i = n*T + t and its
numpy-RNG permutation (buffer.py:239), mapped to (t, n) inside the kernels —
the rollout is never flattened or copied.  get() still yields the reference's
RolloutSample namedtuple (field names and per-field shapes of buffer.py:261-267)
for API compatibility.

PrioritizedReplayBuffer (buffer.py:397-490, PPO(sil=True)) is a ring of S steps in the same
step-major layout with two segment trees over its env-major index (csrc/sil.hip).
"""
from collections import namedtuple

import numpy as np
import torch

import logger
import native
from dist import DistContext
from phases import traced


def _space_dim(space):
    return 1 if space.__class__.__name__ == "Discrete" else space.shape[0]


def _to_dev(x, device, dtype=None):
    if isinstance(x, torch.Tensor):
        t = x.detach().to(device)
    else:
        t = torch.as_tensor(np.asarray(x), device=device)
    return t.to(dtype) if dtype is not None else t


# PPO(episodic=True)'s episodic_kwargs and their defaults (NGU's constants; capacity: PPO passes the env's max_len)
EPISODIC_DEFAULTS = {"k": 10, "capacity": 256, "beta": 0.1, "eps": 1e-3, "xi": 8e-3, "c": 1e-3, "smax": 8.0,
                     "decay": 0.99, "frames": "last"}
# PPO_NGU's episodic_kwargs: the bonus is not added to the rewards (no beta) and is multiplied by a modulator in
# [1, mod_max] (NGU's L)
NGU_DEFAULTS = dict({k: v for k, v in EPISODIC_DEFAULTS.items() if k != "beta"}, mod_max=5.0)
# episodic_kwargs["kind"]: "knn" (the two dicts above) or "elliptical" (DESIGN.md §4.7), whose keys are these;
# ridge is in the embedding's units (squared integer sums).  PPO_NGU: ridge, frames, mod_max (no beta, as above)
EPISODIC_KINDS = ("knn", "elliptical")
ELLIPTICAL_DEFAULTS = {"ridge": 2.0 ** 30, "beta": 0.1, "frames": "last"}
NGU_ELLIPTICAL_KEYS = ("ridge", "frames", "mod_max")


def pop_episodic_kind(kw):
    """Takes "kind" out of the episodic_kwargs dict `kw` (before any other key is looked at) and returns it."""
    kind = kw.pop("kind", "knn")
    if kind not in EPISODIC_KINDS:
        raise ValueError(f"episodic_kwargs: kind must be one of {', '.join(map(repr, EPISODIC_KINDS))}, not {kind!r}")
    return kind


def elliptical_config(kw, allowed=tuple(ELLIPTICAL_DEFAULTS)):
    """kind="elliptical"'s episodic_kwargs `kw` (without "kind") checked against the `allowed` keys ->
    ELLIPTICAL_DEFAULTS overridden by them."""
    unknown = sorted(set(kw) - set(allowed))
    if unknown:
        raise TypeError(f"episodic_kwargs: unknown keys {unknown} for kind='elliptical' ({', '.join(allowed)})")
    cfg = dict(ELLIPTICAL_DEFAULTS, **{k: v for k, v in kw.items() if k in ELLIPTICAL_DEFAULTS})
    ridge = float(cfg["ridge"])
    if not (np.isfinite(ridge) and ridge > 0.0):
        raise ValueError(f"episodic_kwargs: ridge must be finite and positive, not {cfg['ridge']}")
    if not np.isfinite(float(cfg["beta"])):
        raise ValueError(f"episodic_kwargs: beta must be finite, not {cfg['beta']}")
    return cfg


class BaseBuffer:
    """buffer.py:13-109 (size / reset / swap_and_flatten semantics)."""

    def __init__(self, buffer_size, observation_space, action_space, n_envs=1):
        self.buffer_size = buffer_size
        self.observation_space = observation_space
        self.obs_shape = tuple(observation_space.shape)
        self.action_space = action_space
        self.pos = 0
        self.full = False
        self.n_envs = n_envs
        self.action_dim = _space_dim(action_space)

    def size(self):
        return self.buffer_size if self.full else self.pos

    def reset(self):
        self.pos = 0
        self.full = False


class RolloutStorage(BaseBuffer):
    """buffer.py:111-267.  `RolloutBuffer` is an alias (north_star name)."""

    _fields = ("observations", "actions", "old_values", "old_log_probs", "advantages", "returns")

    def __init__(self, buffer_size, n_envs, obs_space, action_space, gae_lam=0.95, gamma=0.99, sim_hash=False,
                 device="cuda", obs_dtype=None, draw_hash_matrix=True, hash_seed=0, episodic=None):
        super().__init__(buffer_size, obs_space, action_space, n_envs=n_envs)
        self.gae_lam = gae_lam
        self.gamma = gamma
        self.device = torch.device(device)
        self.discrete = action_space.__class__.__name__ == "Discrete"
        if obs_dtype is None:
            obs_dtype = torch.uint8 if getattr(obs_space, "dtype", None) is np.uint8 else torch.float32
        self.obs_dtype = obs_dtype
        # buffer.py:137 draws the SimHash matrix from numpy's global RNG at
        # construction; keep the draw so every later permutation matches.
        self.A = np.random.randn(16, self.obs_shape[0]) if draw_hash_matrix else None
        T, N, d = buffer_size, n_envs, self.device
        self.do_hash, self.beta = bool(sim_hash), 0.1                  # buffer.py:141-146
        # uint8 observations of any rank hash through the int8 Philox matrix (an
        # extension pinned to tests/simhash_px_twin.py, not to the reference); the draw above stays
        self.hash_px = self.do_hash and obs_dtype == torch.uint8
        if self.do_hash:
            if self.hash_px:
                D = int(np.prod(self.obs_shape))
                self.hash_seed = int(hash_seed) & 0xFFFFFFFFFFFFFFFF
                self.hash_A8 = torch.empty((16, D), dtype=torch.int8, device=d)
                self.hash_rowsum = torch.empty(16, dtype=torch.int32, device=d)
                native.simhash_matrix_i8(D, self.hash_seed, self.hash_A8, self.hash_rowsum)
                self.hash_workspace = torch.empty(native.simhash_keys_u8_workspace_bytes(N) // 4, dtype=torch.int32,
                                                  device=d)
                # this rollout's keys, row t written by the hash of obs_slots[t]
                self.hash_keys = torch.zeros((T, N), dtype=torch.int32, device=d)
            elif len(self.obs_shape) != 1 or self.A is None:
                raise NotImplementedError("sim_hash supports float32 vector observations (A = randn(16, obs_dim), "
                                          "buffer.py:137) and uint8 observations of any shape (int8 Philox hash "
                                          f"matrix); got {obs_dtype} observations of shape {self.obs_shape}")
            else:
                self.hash_A = torch.from_numpy(self.A).to(d)
            # the count table (buffer.py:136) as one u32 counter per 16-bit key; outlives reset()
            self.count_table = torch.zeros(native.SIMHASH_KEYS, dtype=torch.int32, device=d)
        self.obs_slots = torch.zeros((T + 1, N) + self.obs_shape, dtype=obs_dtype, device=d)
        if self.discrete:
            self.actions = torch.zeros((T, N), dtype=torch.int32, device=d)
            self.log_probs = torch.zeros((T, N), device=d)
        else:
            self.actions = torch.zeros((T, N, self.action_dim), device=d)
            self.log_probs = torch.zeros((T, N, self.action_dim), device=d)
        self.rewards = torch.zeros((T, N), device=d)
        self.values = torch.zeros((T, N), device=d)
        self.masks = torch.zeros((T, N), dtype=torch.uint8, device=d)
        self.advantages = torch.zeros((T, N), device=d)
        self.returns = torch.zeros((T, N), device=d)
        self.done_ret = torch.full((T, N), float("nan"), device=d)
        self.done_len = torch.zeros((T, N), dtype=torch.int32, device=d)
        self.generator_ready = False
        self.RolloutSample = namedtuple("RolloutSample", list(self._fields))
        self.do_episodic = episodic is not None and episodic is not False
        if self.do_episodic:
            self._init_episodic(dict(episodic) if isinstance(episodic, dict) else {}, hash_seed)
        self.reset()

    def _init_episodic(self, kw, seed):
        """The episodic bonus's state (`episodic`: a dict of EPISODIC_DEFAULTS' keys, or
        True for the defaults; with "kind": "elliptical", of ELLIPTICAL_DEFAULTS' keys: DESIGN.md §4.7).  It
        outlives reset(): episodes span rollouts."""
        if self.obs_dtype != torch.uint8:
            raise NotImplementedError("episodic=True embeds uint8 observations through the int8 hash matrix; got "
                                      f"{self.obs_dtype} observations of shape {self.obs_shape}")
        if self.do_hash:
            raise NotImplementedError("episodic=True with sim_hash=True: two bonuses written into the same rewards "
                                      "are not implemented")
        self.epi_kind = pop_episodic_kind(kw)
        if self.epi_kind == "elliptical":
            cfg = elliptical_config(kw)
        else:
            unknown = sorted(set(kw) - set(EPISODIC_DEFAULTS))
            if unknown:
                raise TypeError(f"episodic_kwargs: unknown keys {unknown} ({', '.join(EPISODIC_DEFAULTS)})")
            cfg = dict(EPISODIC_DEFAULTS, **kw)
            K, L = int(cfg["k"]), int(cfg["capacity"])
            if not 1 <= K <= 16 or L < 1:
                raise ValueError(f"episodic_kwargs: k must lie in [1, 16] and capacity be positive (k {K}, "
                                 f"capacity {L})")
        frames = cfg["frames"]
        if frames == "last":
            if len(self.obs_shape) != 3:
                raise ValueError(f"episodic_kwargs: frames='last' needs (frames, H, W) observations, not "
                                 f"{self.obs_shape}")
            D = int(np.prod(self.obs_shape[1:]))
            self.epi_offset = (self.obs_shape[0] - 1) * D       # the newest frame, read in place
        elif frames == "stack":
            D, self.epi_offset = int(np.prod(self.obs_shape)), 0
        else:
            raise ValueError(f"episodic_kwargs: frames must be 'last' or 'stack', not {frames!r}")
        T, N, d = self.buffer_size, self.n_envs, self.device
        self.epi_frames, self.epi_D = frames, D
        self.epi_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.epi_A8 = torch.empty((16, D), dtype=torch.int8, device=d)
        self.epi_rowsum = torch.empty(16, dtype=torch.int32, device=d)
        native.simhash_matrix_i8(D, self.epi_seed, self.epi_A8, self.epi_rowsum)
        self.epi_workspace = torch.empty(native.simhash_keys_u8_workspace_bytes(N) // 4, dtype=torch.int32, device=d)
        self.epi_emb = torch.zeros((N, 16), dtype=torch.int32, device=d)
        self.count = torch.zeros(N, dtype=torch.int32, device=d)
        if self.epi_kind == "elliptical":
            # C^-1 per env, at its start diag(1 / ridge), and the step's bonus in f64 (what ngu() modulates)
            self.epi_ridge, self.epi_beta = float(cfg["ridge"]), float(cfg["beta"])
            self.minv = torch.zeros((N, 16, 16), dtype=torch.float64, device=d)
            self.minv.diagonal(dim1=1, dim2=2).fill_(1.0 / self.epi_ridge)
            self.eb = torch.zeros(N, dtype=torch.float64, device=d)
        else:
            self.epi_k, self.epi_capacity = K, L
            self.epi_coef = tuple(float(cfg[x]) for x in ("decay", "beta", "eps", "xi", "c", "smax"))
            self.mem = torch.zeros((N, L, 16), dtype=torch.int32, device=d)
            self.dm = torch.zeros(2, dtype=torch.float64, device=d)
            self.epi_dk = torch.zeros((N, K), dtype=torch.float64, device=d)
            self.epi_kfound = torch.zeros(N, dtype=torch.int32, device=d)
            self.epi_mk = torch.zeros(N, dtype=torch.float64, device=d)
        # this rollout's bonus before beta, row t written by the step on obs_slots[t]
        self.episodic_bonus = torch.zeros((T, N), device=d)

    @property
    def observations(self):
        return self.obs_slots[: self.buffer_size]

    def reset(self):
        """buffer.py:149-163 re-allocates; here the arrays are reused."""
        self.generator_ready = False
        super().reset()

    def tensors(self):
        """Step-major device arrays by role (what the fused loss kernels read)."""
        return {"actions": self.actions, "log_probs": self.log_probs, "values": self.values,
                "advantages": self.advantages, "returns": self.returns}

    def add(self, obs, action, reward, value, mask, log_prob):
        """buffer.py:165-186 (inputs may be numpy arrays or tensors on any device)."""
        t = self.pos
        self.obs_slots[t].copy_(_to_dev(obs, self.device).reshape(self.obs_slots[t].shape))
        if self.discrete:
            self.actions[t].copy_(_to_dev(action, self.device).reshape(self.n_envs))
            self.log_probs[t].copy_(_to_dev(log_prob, self.device).reshape(self.n_envs))
        else:
            self.actions[t].copy_(_to_dev(action, self.device).reshape(self.n_envs, self.action_dim))
            self.log_probs[t].copy_(_to_dev(log_prob, self.device).reshape(self.n_envs, self.action_dim))
        self.rewards[t].copy_(_to_dev(reward, self.device).reshape(self.n_envs))
        if self.do_hash:
            self.sim_hash(self.obs_slots[t], self.rewards[t], t)
        self.masks[t].copy_(_to_dev(mask, self.device).reshape(self.n_envs))
        if self.do_episodic:
            self._episodic_step(t)
        self.values[t].copy_(_to_dev(value, self.device).reshape(self.n_envs))
        self.pos += 1
        if self.pos == self.buffer_size:
            self.full = True

    def _episodic_step(self, t):
        """add()'s episodic step on row t (IntrinsicStorage pays the bonus on its intrinsic stream instead)."""
        self.episodic(self.obs_slots[t], self.rewards[t], self.masks[t], t)

    def sim_hash(self, obs, rewards, t=None):
        """buffer.py:188-200 on the device: count bonus added to `rewards` (this rank's
        (n_envs,) f32 row, mutated in place and returned).  Keys of all ranks are
        gathered so the replicated count table advances exactly as in one process.
        uint8 observations are hashed in place (no conversion, no allocation: graph-capturable
        without a process group) and their keys kept in hash_keys[t] (t: the step, default pos)."""
        x = obs.reshape(self.n_envs, -1)
        if self.hash_px:
            if x.dtype != torch.uint8 or x.stride(-1) != 1:
                raise TypeError("sim_hash: this storage hashes uint8 observations with contiguous rows")
            keys = self.hash_keys[self.pos if t is None else t]
            native.simhash_keys_u8(x, self.n_envs, x.shape[1], x.stride(0), self.hash_A8, self.hash_rowsum,
                                   self.hash_workspace, keys)
        else:
            if x.dtype != torch.float32 or x.stride(-1) != 1:
                x = x.float().contiguous()
            keys = torch.empty(self.n_envs, dtype=torch.int32, device=self.device)
            native.simhash_keys(x, self.n_envs, x.shape[1], x.stride(0), self.hash_A, keys)
        ctx = DistContext.current()
        if ctx.enabled:
            keys_all, offset, total = ctx.all_gather_cat(keys, dim=0), ctx.rank * self.n_envs, \
                self.n_envs * ctx.world
        else:
            keys_all, offset, total = keys, 0, self.n_envs
        native.simhash_apply(keys_all, total, offset, self.n_envs, self.count_table, self.beta, rewards)
        return rewards

    def episodic(self, obs, rewards, dones, t=None):
        """The episodic novelty bonus of one step, three launches on preallocated buffers
        (graph-capturable): the integer embedding of `obs` (uint8 frames read in place, the newest frame or
        the whole stack) -> the k nearest of the env's episode so far, then the embedding appended and the
        memory emptied where `dones` (uint8) is set -> the bonus into episodic_bonus[t] (t: the step, default
        pos) and beta times it added to `rewards` (this rank's (n_envs,) f32 row, mutated and returned).
        kind="elliptical" (DESIGN.md §4.7): two launches, the embedding -> the elliptical bonus, minv's update and
        the reward add in one kernel."""
        x = obs.reshape(self.n_envs, -1)
        if x.dtype != torch.uint8 or x.stride(-1) != 1:
            raise TypeError("episodic: this storage embeds uint8 observations with contiguous rows")
        if self.epi_offset:
            x = x[:, self.epi_offset:]
        N = self.n_envs
        native.simhash_sums_u8(x, N, self.epi_D, x.stride(0), self.epi_A8, self.epi_rowsum, self.epi_workspace,
                               self.epi_emb)
        if self.epi_kind == "elliptical":
            # kind="elliptical" (DESIGN.md §4.7): one launch for the bonus, the state's update and the reward add
            native.elliptical_bonus(self.epi_emb, dones, N, self.epi_ridge, self.epi_beta, self.minv, self.count,
                                    self.eb, rewards, self.episodic_bonus[self.pos if t is None else t])
            return rewards
        K = self.epi_k
        native.episodic_knn(self.epi_emb, dones, N, self.epi_capacity, K, self.mem, self.count, self.epi_dk,
                            self.epi_kfound, self.epi_mk)
        native.episodic_reward(self.epi_dk, self.epi_kfound, self.epi_mk, N, K, self.dm, *self.epi_coef, rewards,
                               self.episodic_bonus[self.pos if t is None else t])
        return rewards

    @traced("gae")
    def compute_returns_and_advantages(self, last_value, dones):
        """buffer.py:203-230 on the device (bit-identical), libppox ppox_gae."""
        lv = _to_dev(last_value, self.device, torch.float32).reshape(self.n_envs).contiguous()
        ld = _to_dev(dones, self.device, torch.uint8).reshape(self.n_envs).contiguous()
        native.gae(self.rewards, self.values, self.masks, lv, ld, self.gamma, self.gae_lam, self.advantages,
                   self.returns)

    # ------------------------------------------------------------------ get()
    def epoch_permutation(self):
        """buffer.py:239 — one numpy global-RNG permutation per get() call."""
        return np.random.permutation(self.buffer_size * self.n_envs)

    def _gather(self, x, idx):
        """(T, N, ...) step-major -> rows for env-major indices idx (device int64)."""
        T, N = self.buffer_size, self.n_envs
        x = x.contiguous()
        row = x[0, 0].numel() * x.element_size()
        out = torch.empty((idx.numel(),) + tuple(x.shape[2:]), dtype=x.dtype, device=self.device)
        native.gather_rows(x, T, N, row, row, idx, idx.numel(), out)
        return out

    def _sample(self, idx):
        B = idx.numel()
        acts = self._gather(self.actions, idx).reshape(B, self.action_dim).double()
        lps = self._gather(self.log_probs, idx).reshape(B, self.action_dim)
        return self.RolloutSample(self._gather(self.observations, idx), acts, self._gather(self.values, idx), lps,
                                  self._gather(self.advantages, idx).reshape(B, 1), self._gather(self.returns, idx))

    def get(self, batch_size=None):
        """buffer.py:233-254: minibatch generator over a fresh permutation."""
        assert self.full, ""
        perm = self.epoch_permutation()
        self.generator_ready = True
        total = self.buffer_size * self.n_envs
        bs = total if batch_size is None else batch_size
        perm_dev = torch.as_tensor(perm, device=self.device)
        for s in range(0, total, bs):
            yield self._sample(perm_dev[s:s + bs])


class IntrinsicStorage(RolloutStorage):
    """buffer.py:271-394: second (non-episodic) intrinsic reward stream."""

    _fields = ("observations", "actions", "old_values", "int_values", "old_log_probs", "advantages",
               "int_advantages", "returns", "int_returns")

    def __init__(self, buffer_size, n_envs, obs_space, action_space, gae_lam=0.95, gamma=0.99, int_gamma=0.99,
                 device="cuda", obs_dtype=None, draw_hash_matrix=True, episodic=None, hash_seed=0):
        do_ngu = episodic is not None and episodic is not False
        if do_ngu:
            # PPO_NGU: the episodic state of RolloutStorage, its bonus multiplied by a modulator
            # and written to the intrinsic stream instead of being added to the rewards
            episodic = dict(episodic) if isinstance(episodic, dict) else {}
            kind = pop_episodic_kind(episodic)
            if kind == "elliptical":
                elliptical_config(episodic, NGU_ELLIPTICAL_KEYS)
            else:
                unknown = sorted(set(episodic) - set(NGU_DEFAULTS))
                if unknown:
                    raise TypeError(f"episodic_kwargs: unknown keys {unknown} ({', '.join(NGU_DEFAULTS)})")
            self.ngu_mod_max = float(episodic.pop("mod_max", NGU_DEFAULTS["mod_max"]))
            if not self.ngu_mod_max >= 1.0:
                raise ValueError(f"episodic_kwargs: mod_max must be at least 1, not {self.ngu_mod_max}")
            episodic["kind"] = kind
        super().__init__(buffer_size, n_envs, obs_space, action_space, gae_lam, gamma, device=device,
                         obs_dtype=obs_dtype, draw_hash_matrix=draw_hash_matrix, hash_seed=hash_seed,
                         episodic=episodic if do_ngu else None)
        self.int_gamma = int_gamma
        T, N = buffer_size, n_envs
        self.int_rewards = torch.zeros((T, N), device=self.device)
        self.int_values = torch.zeros((T, N), device=self.device)
        self.int_advantages = torch.zeros((T, N), device=self.device)
        self.int_returns = torch.zeros((T, N), device=self.device)
        if do_ngu:
            # running mean, variance and count of the lifelong error (RunningMeanStd's start); outlives reset()
            self.em = torch.tensor([0.0, 1.0, 1e-4], dtype=torch.float64, device=self.device)
            self.ngu_modulator = torch.zeros((T, N), device=self.device)
            self.rnd_err = torch.zeros((T, N), device=self.device)

    def tensors(self):
        d = super().tensors()
        d.update(int_values=self.int_values, int_advantages=self.int_advantages, int_returns=self.int_returns)
        return d

    def add(self, obs, action, reward, int_reward, value, int_value, mask, log_prob):
        """With the episodic state (PPO_NGU) `int_reward` is the raw lifelong error (None before it is trained):
        int_rewards[t] is ngu()'s product and the rewards stay as given."""
        t = self.pos
        self.int_values[t].copy_(_to_dev(int_value, self.device).reshape(self.n_envs))
        if not self.do_episodic:
            self.int_rewards[t].copy_(_to_dev(int_reward, self.device).reshape(self.n_envs))
        elif int_reward is None:
            self._add_err = None
        else:
            self._add_err = self.rnd_err[t]
            self._add_err.copy_(_to_dev(int_reward, self.device).reshape(self.n_envs))
        super().add(obs, action, reward, value, mask, log_prob)

    def _episodic_step(self, t):
        self.ngu(self.obs_slots[t], self.masks[t], self._add_err, t)

    def ngu(self, obs, dones, err, t=None):
        """NGU's reward of one step, three launches on preallocated buffers with nothing read
        back: the embedding and the k nearest of RolloutStorage.episodic, then the episodic bonus into
        episodic_bonus[t], the modulator of the lifelong error `err` ((n_envs,) f32 on the device, or None: 1)
        into ngu_modulator[t] and their product into int_rewards[t] (t: the step, default pos).
        kind="elliptical" (DESIGN.md §4.7): sums -> elliptical_bonus (paid nowhere) -> ngu_modulate."""
        x = obs.reshape(self.n_envs, -1)
        if x.dtype != torch.uint8 or x.stride(-1) != 1:
            raise TypeError("ngu: this storage embeds uint8 observations with contiguous rows")
        if err is not None and (err.dtype != torch.float32 or err.shape != (self.n_envs,) or not err.is_contiguous()
                                or err.device != self.int_rewards.device):
            raise TypeError("ngu: err must be a contiguous (n_envs,) float32 tensor on the storage's device")
        if self.epi_offset:
            x = x[:, self.epi_offset:]
        N = self.n_envs
        t = self.pos if t is None else t
        native.simhash_sums_u8(x, N, self.epi_D, x.stride(0), self.epi_A8, self.epi_rowsum, self.epi_workspace,
                               self.epi_emb)
        if self.epi_kind == "elliptical":
            # kind="elliptical" (DESIGN.md §4.7): the bonus in f64, paid nowhere, then the modulator half alone
            native.elliptical_bonus(self.epi_emb, dones, N, self.epi_ridge, 0.0, self.minv, self.count, self.eb)
            native.ngu_modulate(self.eb, err, N, self.em, self.ngu_mod_max, self.int_rewards[t],
                                self.episodic_bonus[t], self.ngu_modulator[t])
            return self.int_rewards[t]
        K = self.epi_k
        decay, _, eps, xi, c, smax = self.epi_coef
        native.episodic_knn(self.epi_emb, dones, N, self.epi_capacity, K, self.mem, self.count, self.epi_dk,
                            self.epi_kfound, self.epi_mk)
        native.ngu_reward(self.epi_dk, self.epi_kfound, self.epi_mk, err, N, K, self.dm, self.em, decay, eps, xi, c,
                          smax, self.ngu_mod_max, self.int_rewards[t], self.episodic_bonus[t], self.ngu_modulator[t])
        return self.int_rewards[t]

    @traced("gae")
    def compute_returns_and_advantages(self, last_value, last_int_value, dones):
        """buffer.py:321-362, libppox ppox_gae_dual (both streams bit-identical)."""
        logger.record("rollout/mean_int_reward", float(self.int_rewards.mean().item()))
        lv = _to_dev(last_value, self.device, torch.float32).reshape(self.n_envs).contiguous()
        liv = _to_dev(last_int_value, self.device, torch.float32).reshape(self.n_envs).contiguous()
        ld = _to_dev(dones, self.device, torch.uint8).reshape(self.n_envs).contiguous()
        native.gae_dual(self.rewards, self.values, self.masks, lv, ld, self.int_rewards, self.int_values, liv,
                        self.gamma, self.int_gamma, self.gae_lam, self.advantages, self.returns,
                        self.int_advantages, self.int_returns)

    def _sample(self, idx):
        B = idx.numel()
        acts = self._gather(self.actions, idx).reshape(B, self.action_dim).double()
        lps = self._gather(self.log_probs, idx).reshape(B, self.action_dim)
        g = self._gather
        return self.RolloutSample(g(self.observations, idx), acts, g(self.values, idx), g(self.int_values, idx), lps,
                                  g(self.advantages, idx).reshape(B, 1), g(self.int_advantages, idx).reshape(B, 1),
                                  g(self.returns, idx), g(self.int_returns, idx))


class PrioritizedReplayBuffer(BaseBuffer):
    """buffer.py:397-490 on the device, for self-imitation learning: a ring of
    S steps x n_envs in the rollout's step-major layout, S = max(ceil(buffer_size / n_envs),
    min_steps), with a sum and a min segment tree (f64, 2P nodes, P the power of two >= S * n_envs)
    over the env-major slot index i = n * S + s.  A slot is empty, pending (its episode has not
    ended: no return yet, not sampled) or active.  Whole rollouts are appended (append_rollout) in
    time order; the reference adds an episode when it ends.

    Memory: the ring holds S * n_envs observations of the env's dtype.  The default buffer_size
    50,000 (ppo.py:164) is 1.4 GB of 4 x 84 x 84 uint8 frames at 4 envs; at 4,096 envs x 128 steps
    SilModule's floor min_steps = 2 * nstep makes it 256 steps = 29.6 GB."""

    def __init__(self, buffer_size, n_envs, obs_space, action_space, alpha=0.6, device="cuda", gamma=0.99,
                 min_steps=1):
        super().__init__(buffer_size, obs_space, action_space, n_envs=n_envs)
        if action_space.__class__.__name__ != "Discrete":
            raise NotImplementedError("PrioritizedReplayBuffer stores Discrete actions (self-imitation on a Box "
                                      "action space is not implemented)")
        self.alpha, self.gamma = float(alpha), float(gamma)
        self.device = d = torch.device(device)
        N = n_envs
        self.n_steps = S = max(-(-int(buffer_size) // N), int(min_steps))
        self.capacity = P = 1 << max(S * N - 1, 0).bit_length()
        obs_dtype = torch.uint8 if getattr(obs_space, "dtype", None) is np.uint8 else torch.float32
        self.observations = torch.zeros((S, N) + self.obs_shape, dtype=obs_dtype, device=d)
        self.actions = torch.zeros((S, N), dtype=torch.int32, device=d)
        self.log_probs = torch.zeros((S, N), device=d)
        self.returns = torch.zeros((S, N), device=d)           # the reward until the slot's episode ends
        self.dones = torch.zeros((S, N), dtype=torch.uint8, device=d)
        self.state = torch.zeros((S, N), dtype=torch.uint8, device=d)
        self.buffer_sum = torch.zeros(2 * P, dtype=torch.float64, device=d)
        self.buffer_min = torch.full((2 * P,), float("inf"), dtype=torch.float64, device=d)
        self.max_priority = torch.ones(1, dtype=torch.float64, device=d)
        self.n_active = torch.zeros(1, dtype=torch.int64, device=d)
        self.head = 0  # the ring step the next rollout starts at

    def tensors(self):
        """The ring's device arrays by role (what the ppox_sil_* kernels read and write)."""
        return {"obs": self.observations, "actions": self.actions, "log_probs": self.log_probs,
                "returns": self.returns, "dones": self.dones, "state": self.state,
                "sum_tree": self.buffer_sum, "min_tree": self.buffer_min}

    def __len__(self):
        """Active slots (one device read)."""
        return int(self.n_active.item())

    def append_rollout(self, observations, actions, log_probs, rewards, dones):
        """The rollout's T steps into the ring, then returns of the episodes that ended and both
        trees (ppox_sil_append -> ppox_sil_returns -> ppox_sil_tree_rebuild)."""
        T = actions.shape[0]
        ring = self.tensors()
        native.sil_append(observations, actions, log_probs, rewards, dones, ring, self.head)
        self.head = (self.head + T) % self.n_steps
        native.sil_returns(ring, (self.head - 1) % self.n_steps, self.gamma, self.alpha, self.max_priority)
        native.sil_tree_rebuild(self.buffer_sum, self.buffer_min, self.state, self.n_active)

    def _gather(self, x, idx):
        """(S, N, ...) step-major -> rows for env-major indices idx (as RolloutStorage._gather)."""
        row = x[0, 0].numel() * x.element_size()
        out = torch.empty((idx.numel(),) + tuple(x.shape[2:]), dtype=x.dtype, device=self.device)
        native.gather_rows(x, self.n_steps, self.n_envs, row, row, idx, idx.numel(), out)
        return out

    def sample(self, u, beta):
        """buffer.py:446-472 for the uniforms u (host float64 array in [0, 1)): env-major indices
        (device int64) and importance weights (device f32)."""
        u = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float64))
        if self.device.type == "cuda":
            u = u.pin_memory()
        u = u.to(self.device, non_blocking=True)
        idx = torch.empty(u.numel(), dtype=torch.int64, device=self.device)
        weights = torch.empty(u.numel(), device=self.device)
        native.sil_sample(self.buffer_sum, self.buffer_min, self.n_active, u, beta, idx, weights)
        return idx, weights

    def update_priorities(self, indexes, priorities):
        """buffer.py:454-459 (device int64 indexes, device f32 priorities)."""
        native.sil_update_priorities(indexes, priorities, self.alpha, self.buffer_sum, self.buffer_min,
                                     self.max_priority)


# north_star names (SURVEY.md API-name mismatch note)
RolloutBuffer = RolloutStorage
IntrinsicRolloutBuffer = IntrinsicStorage
