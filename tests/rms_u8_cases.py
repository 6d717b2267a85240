"""Frame-like uint8 batches for the running-moments tests (test helper, not a test module).

Atari frames are mostly near-constant pixels; uniform-random bytes never show what a variance
formula does with them.  batch(rows, seed) returns a (rows, COLS) column slice of a wider
array (row_stride = WIDE > COLS) whose column c is of kind KINDS[c % len(KINDS)].
tests/test_pairwise_twin.py bounds numpy's own error on exactly these inputs, and
tests/test_rms_gpu.py holds the kernel to them."""
from fractions import Fraction

import numpy as np

COLS, WIDE, LEFT = 300, 320, 7  # two 256-column blocks; the slice starts 7 bytes into each wide row
ROWS = (1, 63, 64, 65, 257, 1000, 4099)
KINDS = ("zeros", "full", "one_up", "one_down", "alt2", "alt3", "outliers", "random")


def batch(rows, seed):
    rs = np.random.RandomState(seed)
    wide = rs.randint(0, 256, (rows, WIDE)).astype(np.uint8)  # the bytes around the slice are noise
    x = wide[:, LEFT:LEFT + COLS]
    r = np.arange(rows)
    for c in range(COLS):
        kind = KINDS[c % len(KINDS)]
        if kind == "zeros":
            x[:, c] = 0
        elif kind == "full":
            x[:, c] = 255
        elif kind == "one_up":  # 0 ... 0, 1
            x[:, c] = 0
            x[rs.randint(rows), c] = 1
        elif kind == "one_down":  # 255 ... 255, 254
            x[:, c] = 255
            x[rs.randint(rows), c] = 254
        elif kind == "alt2":  # 200, 201, 200, 201, ...
            x[:, c] = 200 + (r + c // len(KINDS)) % 2
        elif kind == "alt3":  # 200, 201, 201, 200, ...
            x[:, c] = 200 + ((r + c // len(KINDS)) % 3 > 0)
        elif kind == "outliers":  # three outliers on 255
            x[:, c] = 255
            x[rs.randint(rows, size=3), c] = (0, 17, 128)
        # "random": the uniform control, as drawn
    return wide, x


def sequence(rows):
    """Three successive updates of mixed row counts, the first with `rows` rows."""
    i = ROWS.index(rows)
    return [(ROWS[(i + 3 * k) % len(ROWS)], 1000 * rows + k) for k in range(3)]


def exact_moments(x):
    """Per column: the exact integer sums S, Q and the exact rational variance (n Q - S^2) / n^2."""
    n = x.shape[0]
    S = x.astype(np.int64).sum(0)
    Q = (x.astype(np.int64) ** 2).sum(0)
    return [int(s) for s in S], [int(q) for q in Q], [Fraction(n * int(q) - int(s) ** 2, n * n) for s, q in zip(S, Q)]
