"""Self-imitation learning on the device (reference: sil_module.py:9-113, PPO(sil=True)).

The reference's SilModule cannot be constructed (sil_module.py:14 against buffer.py:406) and its
loss is wrong in three places; this module implements the corrected definition of DESIGN.md §4.4,
whose executable form is tests/sil_twin.py:

    step_rollout(rollout)   once per collect: the rollout's steps into the replay ring, returns of
                            the episodes that ended, both priority trees
                            (ppox_sil_append -> ppox_sil_returns -> ppox_sil_tree_rebuild)
    train(n_epochs, batch_size, clip_range, ent_coef)
                            per epoch: np.random.rand(B) -> ppox_sil_sample -> training forward on
                            the ring's rows -> ppox_sil_loss -> backward -> clip(1) + Adam on the
                            policy's own optimizer -> ppox_sil_update_priorities
"""
import numpy as np
import torch

import logger
import native
from buffer import PrioritizedReplayBuffer


class SilModule:
    """sil_module.py:9-113.  `algo` is the algorithm that owns `policy` and `optimizer`: its training
    forward / backward (BaseAlgorithm._train_obs, _fwd_train, _bwd_reduce) and learning rate are used
    as they are for PPO's own minibatches."""

    def __init__(self, size, policy, optimizer, n_envs, env, gamma=.99, nstep=128, alpha=0.6, beta=1.0, device="cuda",
                 algo=None):
        if algo is None:
            raise ValueError("SilModule needs algo=: the algorithm whose policy it trains")
        self.policy, self.optimizer, self.algo = policy, optimizer, algo
        self.gamma, self.beta = gamma, float(beta)
        self.device = torch.device(device)
        # at least two rollouts of steps: an episode's head stays pending until the episode ends
        self.buffer = PrioritizedReplayBuffer(size, n_envs, env.observation_space, env.action_space, alpha=alpha,
                                              device=self.device, gamma=gamma, min_steps=2 * nstep)
        self.n_actions = env.action_space.n
        self.loss_partials = torch.zeros(native.LOSS_PARTIALS * 4, dtype=torch.float64, device=self.device)
        self.loss_accum = torch.zeros(3, dtype=torch.float64, device=self.device)  # sum L, sum mean a, count

    def step_rollout(self, rollout):
        """sil_module.py:23-55 for a finished rollout (after its rewards are final)."""
        self.buffer.append_rollout(rollout.observations, rollout.actions, rollout.log_probs, rollout.rewards,
                                   rollout.masks)

    def train(self, n_epochs, batch_size, clip_range, ent_coef=0.01):
        """sil_module.py:57-97.  Trains only once more than 100 slots are active (:109)."""
        n = len(self.buffer)
        if not n > 100:
            return
        algo, buf = self.algo, self.buffer
        ring = buf.tensors()
        self.loss_accum.zero_()
        B = min(int(batch_size), n)
        for _ in range(n_epochs):
            # the reference draws its masses from numpy's global stream (buffer.py:449)
            idx, weights = buf.sample(np.random.rand(B), self.beta)
            algo._zero_policy_grad(B)
            out, v, _, ctx = algo._fwd_train(algo._train_obs(buf, idx))
            out_d, v_d = out.detach().contiguous(), v.detach().contiguous()
            dout, dv = torch.empty_like(out_d), torch.empty_like(v_d)
            priority = torch.empty(B, device=self.device)
            native.sil_loss(out_d, v_d, idx, ring, weights, clip_range, ent_coef, dout, dv, priority,
                            self.loss_partials, self.loss_accum)
            algo._bwd_reduce(ctx, out, v, None, dout, dv)
            self.optimizer.adam_step(algo.lr, 1.0)                             # sil_module.py:88-89
            buf.update_priorities(idx, priority)
        acc = self.loss_accum.cpu().numpy()
        logger.record("rollout/mean_sil_advantage", acc[1] / acc[2])
        logger.record("train/sil_loss", acc[0] / acc[2])
