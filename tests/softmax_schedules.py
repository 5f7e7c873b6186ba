"""Inputs whose score sequences force the rescale branch of the online softmax (include/hnh_attention.h), for the kernel tests and
their CPU check.

Every row belongs to one schedule g (row i: g = i % len(SCHEDULES)).  Its row operand is X_i = scale_g * e_g, and column g of the
gathered operand holds a map t_g(j) of the column index, so s_ij = LeakyReLU(scale_g * t_g(j)): the score of a nonzero is set by its
column, and a row's sequence of scores is designed by choosing its (sorted) columns.  The other columns of Y are random, so the
output is not trivial.  `build` returns the designed rise positions of every row (rises = max_rises of gat_pass_ref):

    monotone      t increasing in j, distinct columns                      every nonzero raises the max
    spike         t decreasing in j, one spike column at position k        rises at 0 and k, k = 0 .. 18; a hub row with its spike last
    window        a staircase over the column windows (higher per window)  rises at the first nonzero of every window the row has
    panel         the same staircase over the forced column panels         rises at the first nonzero of every panel the row has
    ties          t constant (repeated columns too)                        a rise at 0 only
    tie_spike     t = 1 on even columns, < 1 on odd ones, rows start even  a rise at 0 only: later even columns equal the max (f == 1)
    jump          scores 1000 and 2000 above a base in [-2, 0]             rises of more than 745 (exp underflows, f = 0), then lower scores"""
import numpy as np

SCHEDULES = ("monotone", "spike", "window", "panel", "ties", "tie_spike", "jump")
NMAP = len(SCHEDULES)
SCALE = {"monotone": 8.0, "spike": 4.0, "window": 12.0, "panel": 12.0, "ties": 3.0, "tie_spike": 3.0, "jump": 1000.0}
SPIKE_K = range(19)  # crosses two batch boundaries for every batch of U <= 8 nonzeros


def window_bounds(m, nwin):
    """Column bounds of nwin windows as the kernel tests pass them to hnh_csr_window_bounds (int(m * (b + 1) / nwin))."""
    return [0] + [int(m * (b + 1) / nwin) for b in range(nwin - 1)] + [m]


def panel_bounds(m, panels):
    """Column bounds of the row pass's column panels (panel q = columns [q * width, (q + 1) * width), width = ceil(m / panels))."""
    w = (m + panels - 1) // panels
    return [min(m, q * w) for q in range(panels)] + [m]


def staircase(m, bounds):
    """Per column: higher in every later segment, decreasing inside one ((q + 1 - 0.9 u) / n, u in [0, 1) the position in segment q)."""
    t = np.empty(m)
    n = len(bounds) - 1
    for q in range(n):
        lo, hi = bounds[q], bounds[q + 1]
        t[lo:hi] = (q + 1 - 0.9 * (np.arange(lo, hi) - lo) / (hi - lo)) / n
    return t


def maps(m, nwin, panels):
    j = np.arange(m)
    t = np.zeros((NMAP, m))
    t[0] = j / m
    t[1] = np.where(j % 64 == 63, 1.0, -0.5 * j / m)
    t[2] = staircase(m, window_bounds(m, nwin))
    t[3] = staircase(m, panel_bounds(m, panels))
    t[4] = 0.5
    t[5] = np.where(j % 2 == 0, 1.0, 0.9 * (1.0 - j / m))
    t[6] = np.where(j % 64 == 31, 1.0, np.where(j % 64 == 47, 2.0, -0.01 * j / m))
    return t


def _segment_rises(cols, bounds):
    seg = np.searchsorted(bounds, cols, side="right") - 1
    return np.nonzero(np.concatenate([[True], seg[1:] != seg[:-1]]))[0] if len(cols) else np.zeros(0, dtype=np.int64)


def build(m, width, seed, nwin=6, panels=5):
    """(rowptr, colidx, x, y, rises, group): a CSR block of m rows (sorted columns) over m columns, operands of `width` >= NMAP
    columns, and per row its designed rise positions and schedule name.  About one row in ten is empty."""
    assert width >= NMAP and m % 64 == 0 and m >= 1024
    rng = np.random.default_rng(seed)
    t = maps(m, nwin, panels)
    j = np.arange(m)
    spikes = j[j % 64 == 63]
    base = j[j % 64 != 63]
    jump_base = j[(j % 64 != 31) & (j % 64 != 47)]
    wb, pb = window_bounds(m, nwin), panel_bounds(m, panels)
    row_cols, rises, group = [], [], []
    spike_k = iter([k for k in SPIKE_K for _ in range(4)])
    first = {}
    for i in range(m):
        g = SCHEDULES[i % NMAP]
        group.append(g)
        first.setdefault(g, i)
        n = int(rng.integers(1, 41))
        if rng.random() < 0.1 and i != first[g]:
            row_cols.append(np.zeros(0, dtype=np.int64))
            rises.append(np.zeros(0, dtype=np.int64))
            continue
        if g == "monotone":
            if i == first[g]:
                n = 300
            c = np.sort(rng.choice(m, n, replace=False))
            r = np.arange(n)
        elif g == "spike":
            k = next(spike_k, None)
            if i == first[g]:  # a hub row whose last nonzero is the spike (column m - 1)
                c = np.concatenate([np.sort(rng.choice(base[base < m - 64], 699, replace=False)), [m - 1]])
                r = np.array([0, 699])
            else:
                if k is None:  # past the k = 0 .. 18 rows: a spike late in a row of 60 .. 120
                    n = int(rng.integers(60, 121))
                    k = int(rng.integers(n - 8, n))
                else:
                    n = k + 1 + int(rng.integers(0, 24))
                sc = spikes[int(rng.integers(k // 60 + 2, len(spikes) - 2))]
                before = np.sort(rng.choice(base[base < sc], k, replace=False))
                after = np.sort(rng.choice(base[base > sc], n - k - 1, replace=False))
                c = np.concatenate([before, [sc], after])
                r = np.array([0, k]) if k > 0 else np.array([0])
        elif g in ("window", "panel"):
            bounds = wb if g == "window" else pb
            c = np.sort(np.concatenate([rng.choice(np.arange(bounds[q], bounds[q + 1]), int(rng.integers(0, 5)), replace=False)
                                        for q in range(len(bounds) - 1)] + [rng.choice(m, 1)]))
            c = np.unique(c)
            r = _segment_rises(c, bounds)
        elif g == "ties":
            if i == first[g]:
                n = 300
            c = np.sort(rng.integers(0, m, n))
            r = np.array([0])
        elif g == "tie_spike":
            c0 = 2 * int(rng.integers(0, m // 4))
            rest = np.sort(rng.integers(c0 + 1, m, n))
            c = np.concatenate([[c0], rest, [c0 + 2 * int(rng.integers(1, (m - c0) // 2))]])
            c = np.sort(c)
            r = np.array([0])
        else:  # jump
            k1 = int(rng.integers(1, 11))
            two = rng.random() < 0.5
            s1 = 64 * int(rng.integers(4, m // 128)) + 31
            s2 = 64 * int(rng.integers(m // 128, m // 64 - 2)) + 47
            pre = np.sort(rng.choice(jump_base[jump_base < s1], k1, replace=False))
            mid = np.sort(rng.choice(jump_base[(jump_base > s1) & (jump_base < s2)], int(rng.integers(0, 6)), replace=False))
            post = np.sort(rng.choice(jump_base[jump_base > (s2 if two else s1)], int(rng.integers(1, 6)), replace=False))
            if two:
                c = np.concatenate([pre, [s1], mid, [s2], post])
                r = np.array([0, k1, k1 + 1 + len(mid)])
            else:
                c = np.concatenate([pre, [s1], np.sort(np.concatenate([mid, post]))])
                r = np.array([0, k1])
        row_cols.append(np.asarray(c, dtype=np.int64))
        rises.append(np.asarray(r, dtype=np.int64))
    deg = np.array([len(c) for c in row_cols])
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    colidx = np.concatenate(row_cols).astype(np.int32)
    x = np.zeros((m, width))
    for gi, g in enumerate(SCHEDULES):
        x[gi::NMAP, gi] = SCALE[g]
    y = rng.uniform(-1, 1, (m, width))
    y[:, :NMAP] = t.T
    return rowptr, colidx, x, y, rises, group
