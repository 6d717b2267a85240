"""Long-double references and derived tolerances for the ES kernels (csrc/es.hip): test helper,
not a test module.  tests/test_es_twin.py checks it on the CPU, tests/test_es_gpu.py holds the
kernels to it.

  evaluate_ld   oracle.es.evaluate restated in np.longdouble (80-bit x87: 64-bit significand)
                on the same env_matrix / env_noise.  The float64 constants 0.9, 0.1, 0.02, 0.05
                are the oracle's and the kernel's own doubles, widened: the function computed is
                the same one, only its arithmetic is wider.
  update_ld     sum_p coef[p] * eps[p][j] in long double.
  update_bound  the sequential-sum bound of the same sum in float64.
  CASES         the (D, H1, H2, A) table of the evaluate tests, weights scaled by 1/sqrt(fan_in).
  EVAL_TOL      16 x the float64 oracle's own worst error against evaluate_ld over CASES.

The episode is an iterated map: with un-scaled randn weights it can amplify rounding (one
draw at (32, 64, 64, 8) left the float64 oracle 1.6e-10 from its long-double restatement),
with fan-in-scaled weights it does not, so the shape tests use those."""
import numpy as np

from oracle import es as O

LD = np.longdouble

# seeds with a non-zero high key word (k1 = seed >> 32)
ENV_SEED = (0x9E3779B9 << 32) | 0x7F4A7C15
EPS_SEED = (5 << 32) | 77
T_EVAL, P_EVAL, SIGMA, GENERATION = 40, 5, 0.1, 3

# (D, H1, H2, A)
CASES = [
    (1, 1, 1, 1),        # D = 1: bc[:, 1] == 0
    (8, 16, 12, 2),
    (8, 64, 64, 2),      # last shape of es_eval_kernel<8, 2>
    (9, 5, 7, 2),        # first <32, 8> by D
    (8, 64, 1, 3),       # first <32, 8> by A
    (4, 3, 64, 1),       # InvertedPendulum
    (11, 64, 64, 3),     # Hopper
    (11, 7, 63, 1),      # InvertedDoublePendulum shape
    (24, 63, 33, 4),     # BipedalWalker
    (32, 64, 64, 8),     # the limits
    (32, 1, 1, 8),
]

# Measured on the CPU (test_es_twin.py recomputes it): the worst error of oracle.es.evaluate against
# evaluate_ld over CASES x P_EVAL members at T_EVAL steps, fitness and behaviour, relative to
# max(1, |value|), was 1.7174e-14 on the fitness, at (11, 64, 64, 3), and 1.09e-15 on the behaviour, at
# (32, 64, 64, 8); the nine other shapes stay below 6e-16.  The members are w + 0.1 eps with eps ~ N(0, 1), so
# at fan-in 64 their gain is about 1.3, not 1: the two large shapes amplify rounding a little.  (1.7175e-14 on
# a second CPU model.)  Written here rounded up to two digits.
ORACLE_WORST = 1.8e-14
# The kernel differs from numpy only in summation order, fma and the device's atan / tanh of a few ulp: the
# error class of the oracle's own, with room for a 2-ulp libm and for one table's luck.
EVAL_TOL = 16 * ORACLE_WORST


def ld_ok():
    return np.finfo(LD).eps < 1e-18


LD_SKIP_REASON = "np.longdouble is no wider than float64 here: no high-precision reference"


def _require_ld():
    if not ld_ok():
        raise RuntimeError(LD_SKIP_REASON)


def case_id(case):
    return "x".join(str(v) for v in case)


def case_weights(case):
    """[W0 (D, H1), W1 (H1, H2), W2 (H2, A)] float64, randn / sqrt(fan_in), one fixed draw per case."""
    sizes = list(case)
    D, H1, H2, A = sizes
    rs = np.random.RandomState(D * 1000003 + H1 * 10007 + H2 * 101 + A)
    return [rs.randn(a, b) / np.sqrt(a) for a, b in zip(sizes[:-1], sizes[1:])]


def n_params(case):
    return int(sum(a * b for a, b in zip(case[:-1], case[1:])))


def flat(weights):
    return np.concatenate([np.asarray(w).reshape(-1) for w in weights])


def members(weights, eps, sigma):
    """theta_p = w + sigma * eps_p per layer, in float64 as the kernel forms it (two roundings, no fma:
    the library is built with -ffp-contract=off) -> list of weight lists."""
    out = []
    for row in np.asarray(eps, np.float64):
        off, ws = 0, []
        for w in weights:
            ws.append(w + sigma * row[off:off + w.size].reshape(w.shape))
            off += w.size
        out.append(ws)
    return out


def case_members(case):
    """(weights, eps (P_EVAL, n) from the oracle's perturbation stream, members)"""
    w = case_weights(case)
    eps = O.perturbations(EPS_SEED, GENERATION, np.arange(P_EVAL), n_params(case))
    return w, eps, members(w, eps, SIGMA)


def predict_ld(weights, obs):
    out = np.asarray(obs, LD).reshape(len(obs), -1)
    for w in weights[:-1]:
        out = np.arctan(out @ w)
    return np.tanh(out @ weights[-1])


def evaluate_ld(weights_list, env_seed, T):
    """oracle.es.evaluate in long double -> (fitness (n,), behaviour (n, 2)) as np.longdouble."""
    _require_ld()
    wl = [[np.asarray(w, np.float64).astype(LD) for w in ws] for ws in weights_list]
    D, A = wl[0][0].shape[0], wl[0][-1].shape[1]
    B = O.env_matrix(env_seed, D, A).astype(LD)
    n = len(wl)
    s = np.zeros((n, D), LD)
    fit = np.zeros(n, LD)
    c9, c1, c02, c05 = LD(0.9), LD(0.1), LD(0.02), LD(0.05)
    for t in range(T):
        a = np.stack([predict_ld(w, s[m:m + 1])[0] for m, w in enumerate(wl)])
        s = c9 * s + c1 * (a @ B.T) + c02 * O.env_noise(env_seed, D, t).astype(LD)[None, :]
        fit += s[:, 0] - c05 * (a * a).sum(axis=1)
    b = np.zeros((n, 2), LD)
    b[:, :min(D, 2)] = s[:, :2]
    return fit, b


def behaviour64(b, D):
    """The oracle's (n, min(D, 2)) behaviour as the kernel's (n, 2): bc[:, 1] = 0 at D = 1."""
    out = np.zeros((len(b), 2))
    out[:, :min(D, 2)] = b
    return out


def rel_err(got, ref):
    """max |got - ref| / max(1, |ref|), in long double"""
    got, ref = np.asarray(got, LD), np.asarray(ref, LD)
    return float(np.max(np.abs(got - ref) / np.maximum(LD(1), np.abs(ref))))


def oracle_error(case, T=T_EVAL):
    """(fitness error, behaviour error) of the float64 oracle against evaluate_ld on the case's members."""
    _, _, mem = case_members(case)
    f64, b64 = O.evaluate(mem, ENV_SEED, T)
    f, b = evaluate_ld(mem, ENV_SEED, T)
    return rel_err(f64, f), rel_err(behaviour64(b64, case[0]), b)


def update_ld(coef, eps):
    """delta[j] = sum_p coef[p] * eps[p][j] in long double."""
    _require_ld()
    c = np.asarray(coef, np.float64).astype(LD)
    e = np.asarray(eps, np.float64).astype(LD)
    return (c[:, None] * e).sum(axis=0)


def update_bound(coef, eps):
    """Per column, gamma * sum_p |coef[p] * eps[p][j]| with gamma = (P+1) u / (1 - (P+1) u), u = 2^-53: the
    bound on a float64 sum of P rounded products added one after another in any fixed order (Higham, Accuracy and
    Stability of Numerical Algorithms, 2nd ed., eq. 3.5 / 4.4: P - 1 additions and one multiplication per term,
    gamma_P, taken one step wider).  It holds with a fused multiply-add too (one rounding fewer), and summing in
    chunks of 128 then over the chunks shortens every term's chain, so it can only lower the error."""
    c = np.abs(np.asarray(coef, np.float64))
    e = np.abs(np.asarray(eps, np.float64))
    P = len(c)
    u = 2.0 ** -53
    gamma = (P + 1) * u / (1 - (P + 1) * u)
    return gamma * (c[:, None] * e).sum(axis=0)
