"""The definition of self-imitation learning as this project implements it (test helper, not a test
module): a numpy twin of the replay ring, the discounted returns, the segment trees,
proportional sampling, importance weights and the priority update, and a torch-CPU autograd twin of
the loss.  tests/test_sil_twin.py pins it bit for bit to the reference's running parts
(tests/golden/sil.npz); tests/test_sil_gpu.py pins the ppox_sil_* kernels to it."""
import numpy as np

EMPTY, PENDING, ACTIVE = 0, 1, 2


def capacity(slots):
    """The power of two >= slots (buffer.py:417-419)."""
    P = 1
    while P < slots:
        P *= 2
    return P


def rebuild(leaves_sum, leaves_min):
    """Both trees (2P float64 nodes, node k's children 2k and 2k + 1, leaf i at P + i) bottom-up from
    their P leaves: every internal node is op(left, right), which is what util.SegmentTree.__setitem__
    (util.py:149-159) keeps true after any sequence of leaf writes."""
    P = len(leaves_sum)
    s, m = np.zeros(2 * P), np.full(2 * P, np.inf)
    s[P:], m[P:] = leaves_sum, leaves_min
    for k in range(P - 1, 0, -1):
        s[k] = s[2 * k] + s[2 * k + 1]
        m[k] = min(m[2 * k], m[2 * k + 1])
    return s, m


def set_leaf(tree, i, val, op):
    """SegmentTree.__setitem__ (util.py:149-159)."""
    P = len(tree) // 2
    k = P + i
    tree[k] = val
    k //= 2
    while k >= 1:
        tree[k] = op(tree[2 * k], tree[2 * k + 1])
        k //= 2


def find_prefixsum_idx(sum_tree, mass):
    """util.py:178-201 plus one guard: the descent also goes left when the right child's sum is 0,
    so rounding of mass - left can never end on an empty leaf."""
    P = len(sum_tree) // 2
    k = 1
    while k < P:
        left, right = sum_tree[2 * k], sum_tree[2 * k + 1]
        if left > mass or right == 0.0:
            k = 2 * k
        else:
            mass -= left
            k = 2 * k + 1
    return k - P


def sample_indices(sum_tree, u):
    """buffer.py:446-452 with the root as the total mass."""
    return np.array([find_prefixsum_idx(sum_tree, float(x) * sum_tree[1]) for x in u], np.int64)


def weights(sum_tree, min_tree, n, idx, beta):
    """buffer.py:464-472 (float64); ones when beta == 0."""
    if not beta > 0:
        return np.ones(len(idx))
    P = len(sum_tree) // 2
    p_min = min_tree[1] / sum_tree[1]
    max_weight = (p_min * n) ** (-beta)
    return np.array([((sum_tree[P + i] / sum_tree[1]) * n) ** (-beta) / max_weight for i in idx])


def discount_with_dones(rewards, dones, gamma):
    """sil_module.py:99-105 in float64."""
    out, r = [], 0.0
    for reward, done in zip(rewards[::-1], dones[::-1]):
        r = float(reward) + gamma * r * (1. - done)
        out.append(r)
    return out[::-1]


class Ring:
    """S steps x N envs, slot (s, n); leaf / minibatch index i = n * S + s."""

    def __init__(self, S, N, alpha=0.6, gamma=0.99):
        self.S, self.N, self.alpha, self.gamma = S, N, float(alpha), float(gamma)
        self.P = capacity(S * N)
        self.actions = np.zeros((S, N), np.int32)
        self.log_probs = np.zeros((S, N), np.float32)
        self.returns = np.zeros((S, N), np.float32)
        self.dones = np.zeros((S, N), np.uint8)
        self.state = np.zeros((S, N), np.uint8)
        self.sum_tree = np.zeros(2 * self.P)
        self.min_tree = np.full(2 * self.P, np.inf)
        self.max_priority = 1.0
        self.head = 0

    def leaf(self, s, n):
        return self.P + n * self.S + s

    def append(self, actions, log_probs, rewards, dones):
        for t in range(actions.shape[0]):
            s = (self.head + t) % self.S
            self.actions[s], self.log_probs[s], self.returns[s], self.dones[s] = \
                actions[t], log_probs[t], rewards[t], dones[t]
            self.state[s] = PENDING
            for n in range(self.N):
                self.sum_tree[self.leaf(s, n)] = 0.0
                self.min_tree[self.leaf(s, n)] = np.inf
        self.head = (self.head + actions.shape[0]) % self.S

    def compute_returns(self):
        """Per env, from the newest step backwards over its pending slots: slots newer than the
        newest done stay pending; from the first done on, R = done ? r : r + gamma * R (float64),
        stored float32, state active, both leaves max_priority ** alpha."""
        pw = self.max_priority ** self.alpha
        for n in range(self.N):
            R, closed, s = 0.0, False, (self.head - 1) % self.S
            for _ in range(self.S):
                if self.state[s, n] != PENDING:
                    break
                done = bool(self.dones[s, n])
                closed = closed or done
                if closed:
                    r = float(self.returns[s, n])
                    R = r if done else r + self.gamma * R
                    self.returns[s, n] = np.float32(R)
                    self.state[s, n] = ACTIVE
                    self.sum_tree[self.leaf(s, n)] = pw
                    self.min_tree[self.leaf(s, n)] = pw
                s = (s - 1) % self.S

    def rebuild(self):
        self.sum_tree, self.min_tree = rebuild(self.sum_tree[self.P:], self.min_tree[self.P:])

    @property
    def n_active(self):
        return int((self.state == ACTIVE).sum())

    def step_rollout(self, actions, log_probs, rewards, dones):
        self.append(actions, log_probs, rewards, dones)
        self.compute_returns()
        self.rebuild()

    def sample(self, u, beta):
        idx = sample_indices(self.sum_tree, u)
        return idx, weights(self.sum_tree, self.min_tree, self.n_active, idx, beta)

    def update_priorities(self, idx, priorities):
        update_priorities(self, idx, priorities)


def update_priorities(trees, idx, priorities):
    """buffer.py:454-459 on an object with sum_tree, min_tree, max_priority, alpha (in batch order, so
    the last occurrence of a repeated index wins)."""
    for i, p in zip(idx, priorities):
        p = np.maximum(np.float64(p), 1e-6)
        set_leaf(trees.sum_tree, int(i), p ** trees.alpha, lambda a, b: a + b)
        set_leaf(trees.min_tree, int(i), p ** trees.alpha, min)
        trees.max_priority = float(np.maximum(trees.max_priority, p))


def sil_loss(logits, values, actions, old_log_probs, returns, w, clip, ent_coef):
    """The SIL loss (sil_module.py:64-84 corrected: per-row products, no advantage normalisation, a
    squared value term) in torch-CPU float32 with autograd.
        delta = R - V;  a = clamp(delta, 0, 10);  m = [delta > 0];  rho = exp(log pi(a|s) - log pi_old)
        L_pol = -mean(w min(a rho, a clamp(rho, 1 - c, 1 + c)))   (a a constant here)
        L_ent = -mean(m H);   L_val = mean(w a^2 / 2)   (differentiated through V)
        L = 0.1 (L_pol + ent_coef L_ent) + 0.01 L_val
    The Categorical head is the policy's (models.py:52-73: Categorical(softmax(logits))).
    Returns (L, mean a, dL/dlogits, dL/dvalues, a, delta) as numpy."""
    import torch
    import torch.nn.functional as F
    z = torch.tensor(np.asarray(logits, np.float32), requires_grad=True)
    v = torch.tensor(np.asarray(values, np.float32), requires_grad=True)
    act = torch.as_tensor(np.asarray(actions)).long()
    old = torch.as_tensor(np.asarray(old_log_probs, np.float32))
    R = torch.as_tensor(np.asarray(returns, np.float32))
    w = torch.as_tensor(np.asarray(w, np.float32))
    dist = torch.distributions.Categorical(F.softmax(z, dim=-1))
    logp, H = dist.log_prob(act), dist.entropy()
    delta = R - v
    a = torch.clamp(delta, 0, 10)
    a_c = a.detach()
    m = (delta.detach() > 0).float()
    rho = torch.exp(logp - old)
    L_pol = -(w * torch.min(a_c * rho, a_c * torch.clamp(rho, 1 - clip, 1 + clip))).mean()
    L_ent = -(m * H).mean()
    L_val = (0.5 * w * a * a).mean()
    L = 0.1 * (L_pol + ent_coef * L_ent) + 0.01 * L_val
    L.backward()
    return (float(L.detach()), float(a_c.mean()), z.grad.numpy(), v.grad.numpy(), a_c.numpy(), delta.detach().numpy())
