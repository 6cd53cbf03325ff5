"""numpy / Python-int reference of the pair merges (csrc/trace_merge.hip, csrc/trace_merge.hpp;
include/hdpm.h states the formulas and the rules):

  * ``merge_gains_formula``: the Ka x Ka gains by the formulas, Binder in integers;
  * ``merge_gains_brute``: the same by relabelling b to a and recomputing the whole loss;
  * ``best_pair`` and ``gap``: the tie rule, and how far the best pair stands clear;
  * ``merge_path_ref``: the greedy path, each level's value recomputed from the labels;
  * ``refine_merge_ref``: the alternation with ``refine_ref.refine_ref``.

``SHAPES``, ``gains_case``, ``stall_case`` and ``path_case`` are what the GPU tests run;
tests/test_merge_ref_host.py checks on this reference alone that in every one of them the
best pair stands clear of the next, so that the GPU tests may demand the same pair.
"""
import math

import numpy as np

import refine_ref as R

LN2 = 0.6931471805599453


def vi_atol(N):
    """tests/test_gpu_refine.py's atol of a VI value"""
    return 1e-12 * 3 * math.log2(max(N, 2))


def f(s, t):
    """(s + t) log2(s + t) - s log2 s - t log2 t, 0 if s = 0 or t = 0, in the log1p form"""
    s, t = np.broadcast_arrays(np.asarray(s, np.float64), np.asarray(t, np.float64))
    ok = (s > 0) & (t > 0)
    s1, t1 = np.where(ok, s, 1.0), np.where(ok, t, 1.0)
    return np.where(ok, (s1 * np.log1p(t1 / s1) + t1 * np.log1p(s1 / t1)) / LN2, 0.0)


def f_products(s, t):
    """the same as the difference of the products: what the library must not evaluate"""
    s, t = float(s), float(t)
    return (s + t) * math.log2(s + t) - s * math.log2(s) - t * math.log2(t)


def merge_gains_formula(c, tr, Ka, loss):
    """Ka x Ka: float64 for VI, int64 for Binder; 0 on the diagonal and for empty classes"""
    c = np.asarray(c, np.int64)
    M, N = tr.shape
    Kz = int(tr.max()) + 1
    n = np.bincount(c, minlength=Ka).astype(np.int64)
    if loss == "VI":
        F = np.zeros((Ka, Ka))
        for z in tr:                                   # the non-zero rows of each column only
            T = R.table(c, z, Ka, Kz)
            for b in range(Kz):
                idx = np.flatnonzero(T[:, b])
                if idx.size > 1:
                    s = T[idx, b]
                    F[np.ix_(idx, idx)] += f(s[:, None], s[None, :])
        g = (M * f(n[:, None], n[None, :]) - 2.0 * F) / (float(M) * N)
        g[(n == 0)[:, None] | (n == 0)[None, :]] = 0.0
        g[np.arange(Ka), np.arange(Ka)] = 0.0
        return g
    cross = np.zeros((Ka, Ka), np.int64)
    for z in tr:
        T = R.table(c, z, Ka, Kz).astype(np.int64)
        cross += T @ T.T
    g = M * n[:, None] * n[None, :] - 2 * cross
    g[np.arange(Ka), np.arange(Ka)] = 0
    return g


def merge_gains_brute(c, tr, Ka, loss):
    """the upper triangle by relabelling b to a and recomputing the loss (Python ints for
    Binder): {(a, b): gain} over the non-empty pairs a < b"""
    c = np.asarray(c, np.int64)
    n = np.bincount(c, minlength=Ka)
    base = R.loss_of(c, tr, loss)
    out = {}
    for a in range(Ka):
        for b in range(a + 1, Ka):
            if n[a] and n[b]:
                d = c.copy()
                d[d == b] = a
                out[(a, b)] = R.loss_of(d, tr, loss) - base
    return out


def best_pair(g, n):
    """((a, b), gain): the smallest gain over the non-empty pairs a < b, the lowest a winning
    a tie and then the lowest b; ((-1, -1), 0) if there is no pair"""
    best, bg = (-1, -1), 0
    for a in range(len(n)):
        for b in range(a + 1, len(n)):
            if n[a] and n[b] and (best[0] < 0 or g[a, b] < bg):
                best, bg = (a, b), g[a, b]
    return best, bg


def gap(g, n):
    """the difference of the two smallest gains over the non-empty pairs (inf below two pairs)"""
    n = np.asarray(n)
    iu = np.triu_indices(len(n), 1)
    ok = (n[iu[0]] > 0) & (n[iu[1]] > 0)
    v = np.sort(np.asarray(g)[iu][ok].astype(np.float64))
    return float(v[1] - v[0]) if v.size > 1 else math.inf


def merge_path_ref(c, tr, Ka, loss, k_min=1):
    """{"merge", "step_gain", "value", "gap"}: the greedy path; value[s] recomputed from the
    labels of level s, gap[s] the clearance of step s's pair"""
    cur = np.asarray(c, np.int64).copy()
    out = {"merge": [], "step_gain": [], "value": [R.loss_of(cur, tr, loss)], "gap": []}
    steps = max(0, np.unique(cur).size - k_min)
    for _ in range(steps):
        g = merge_gains_formula(cur, tr, Ka, loss)
        n = np.bincount(cur, minlength=Ka)
        (a, b), bg = best_pair(g, n)
        out["merge"].append((a, b))
        out["step_gain"].append(bg)
        out["gap"].append(gap(g, n))
        cur[cur == b] = a
        out["value"].append(R.loss_of(cur, tr, loss))
    return out


def coarsen_ref(c, merge, steps):
    cur = np.asarray(c, np.int64).copy()
    for a, b in merge[:steps]:
        cur[cur == b] = a
    return R.relabel(cur)


def refine_merge_ref(c, tr, loss, max_rounds=100, max_merges=10):
    """the alternation of include/hdpm.h, step for step"""
    cur = np.asarray(c, np.int64)
    tot = {"rounds": 0, "trials": 0, "moved": 0, "merges": 0, "converged": False, "history": None}
    while True:
        r = R.refine_ref(cur, tr, loss, max_rounds - tot["rounds"])
        if tot["history"] is None:
            tot["start"], tot["history"] = r["start"], [r["start"]]
        tot["history"] += r["history"][1:]
        for k in ("rounds", "trials", "moved"):
            tot[k] += r[k]
        cur, K, L = r["cl"], r["K"], r["value"]
        if not r["converged"]:
            break
        g = merge_gains_formula(cur, tr, K, loss)
        (a, b), bg = best_pair(g, np.bincount(cur, minlength=K))
        if a < 0 or not bg < 0:
            tot["converged"] = True
            break
        if tot["merges"] >= max_merges:
            break
        nxt = cur.copy()
        nxt[nxt == b] = a
        nxt = R.relabel(nxt)
        Ln = R.loss_of(nxt, tr, loss)
        tot["trials"] += 1
        if not Ln < L:
            tot["converged"] = True
            break
        cur, L = nxt, Ln
        tot["merges"] += 1
        tot["history"].append(Ln)
    tot["cl"], tot["value"], tot["K"] = cur, L, int(cur.max()) + 1
    return tot


# ------------------------------------------------------------------ the cases

def dense(rows):
    """each row relabelled 0..K-1 by value, as LabelTrace does"""
    return np.stack([np.unique(r, return_inverse=True)[1] for r in np.atleast_2d(rows)]).astype(np.int64)


# N, M, Ka, Kz, used (the classes that may hold points; those above are empty), a draw of 255
# clusters, a hole (class 2 moved to label used + 1: an empty class below occupied ones), seed
SHAPES = [
    (1, 1, 1, 1, 1, False, False, 1),
    (15, 3, 2, 4, 2, False, False, 2),
    (17, 1, 5, 3, 5, False, False, 3),
    (200, 63, 11, 7, 11, False, False, 4),
    (200, 65, 12, 40, 12, False, False, 5),
    (300, 129, 64, 12, 64, False, False, 6),       # pairs of a class: one whole wave less one
    (300, 5, 65, 12, 65, False, False, 7),         # a wave, and a wave and a lane
    (1000, 37, 255, 255, 255, True, False, 8),
    (120, 9, 9, 6, 6, False, True, 9),             # Ka above the largest label + 1, and a hole
]


def gains_case(N, M, Ka, Kz, used, wide, hole, seed):
    """(c, trace): a truth of about used / 3 classes (at most Kz), draws equal to it with a
    tenth of their labels (more where N is small) redrawn from Kz labels, and the partition
    c = the truth with each class cut at random into about three, labels below `used`.  Where
    there is more than one draw, draw 0 is a random partition into exactly Kz clusters, so the
    device's Kz is the shape's."""
    rng = np.random.default_rng(seed)
    T = min(max(1, used // 3), Kz)
    truth = rng.integers(0, T, N)
    tr = np.tile(truth, (M, 1))
    for z in tr:
        idx = rng.choice(N, size=max(N // 10, min(N // 3, Kz), 1), replace=False)
        z[idx] = rng.integers(0, Kz, idx.size)
    if M > 1:
        tr[0] = rng.permutation(np.arange(N) % Kz)
    assert not wide or Kz == 255
    c = (truth + T * rng.integers(0, -(-used // T), N)) % used
    if hole:
        c[c == 2] = used + 1
    assert c.max() < Ka
    return c.astype(np.int64), dense(tr)


def stall_case():
    """(c, trace, merged): N = 20, M = 10; every draw has {0..11} and {12..19}, draws 0 to 3
    also split off points 6 to 11; the estimate holds the three blocks.  No single move helps;
    merging classes 0 and 1 takes Binder's integer from 216 to 144 and VI from 0.36 to 0.24."""
    c = np.array([0] * 6 + [1] * 6 + [2] * 8)
    tr = np.tile(np.array([0] * 12 + [1] * 8), (10, 1))
    tr[:4, 6:12] = 2
    return c, tr, np.array([0] * 12 + [1] * 8)


def alternation_case(seed=5):
    """(truth, trace, start): N = 240 in blocks of 100 / 80 / 60, M = 20; draws 0 to 7 cut
    blocks 0 and 2 in halves, and every draw has 5 % of its labels redrawn from 5 labels.  The
    start holds the four halves and block 1, with 12 points shifted to the next class: single
    moves put the points back, and only merges join the halves."""
    rng = np.random.default_rng(seed)
    truth = np.repeat(np.arange(3), [100, 80, 60])
    half = np.concatenate([np.arange(100) >= 50, np.zeros(80, bool), np.arange(60) >= 30])
    N, M = truth.size, 20
    tr = np.tile(truth, (M, 1))
    tr[:8, half] += 3
    for z in tr:
        idx = rng.choice(N, size=N * 5 // 100, replace=False)
        z[idx] = rng.integers(0, 5, idx.size)
    start = np.unique(truth + 3 * half, return_inverse=True)[1]
    idx = rng.choice(N, size=12, replace=False)
    start[idx] = (start[idx] + 1) % 5
    return truth, dense(tr), start.astype(np.int64)


PATH_SEED = 11


def path_case(seed=PATH_SEED):
    """(truth, trace, start): N = 300 in classes of 120 / 100 / 80, M = 21 draws equal to the
    truth with 8 % of the labels of each draw redrawn from 4 labels, and a start of 12 classes:
    each true class cut in four at random"""
    rng = np.random.default_rng(seed)
    truth = np.repeat(np.arange(3), [120, 100, 80])
    N, M = truth.size, 21
    tr = np.tile(truth, (M, 1))
    for z in tr:
        idx = rng.choice(N, size=N * 8 // 100, replace=False)
        z[idx] = rng.integers(0, 4, idx.size)
    start = truth * 4 + rng.integers(0, 4, N)
    return truth, dense(tr), start.astype(np.int64)
