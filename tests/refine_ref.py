"""numpy reference of the single-point moves (csrc/trace_refine.hip, csrc/trace_refine.hpp;
include/hdpm.h states the formulas and the round rule), in three parts:

  * ``gains_formula``: the N x (Ka + 1) gains by the formulas, VI's sum over the draws in
    draw order, Binder in integers;
  * ``gains_brute``: the same by moving the point and recomputing the whole loss (Python
    integers for Binder), for small N;
  * ``refine_ref``: the round rule, step for step.

Labels are 0-based and dense where a function says so.  ``planted`` and ``halving`` are the
two constructions the GPU tests run; tests/test_refine_ref_host.py runs them on this
reference alone.
"""
import math

import numpy as np


def h(t):
    """(t + 1) log2(t + 1) - t log2 t, h(0) = 0, as log2(t + 1) + t log1p(1 / t) / ln 2"""
    t = np.asarray(t, np.float64)
    s = np.maximum(t, 1.0)
    return np.where(t > 0, np.log2(s + 1.0) + s * np.log1p(1.0 / s) / math.log(2.0), 0.0)


def xlog2x(x):
    x = np.asarray(x, np.float64)
    return np.where(x > 0, x * np.log2(np.maximum(x, 1.0)), 0.0)


def c2(x):
    return x * (x - 1) // 2


def table(c, z, Ka, Kz):
    return np.bincount(c * Kz + z, minlength=Ka * Kz).reshape(Ka, Kz)


def relabel(c):
    """labels 0..K-1 by first appearance"""
    c = np.asarray(c)
    u, first, inv = np.unique(c, return_index=True, return_inverse=True)
    rank = np.empty(u.size, np.int64)
    rank[np.argsort(first)] = np.arange(u.size)
    return rank[inv]


# ------------------------------------------------------------------ the losses

def vi_loss(c, tr):
    """mcclust.ext VI(cls, cls.draw), the posterior expected VI"""
    M, N = tr.shape
    Ka, Kz = int(c.max()) + 1, int(tr.max()) + 1
    s = 0.0
    for z in tr:
        s += xlog2x(np.bincount(z)).sum() - 2 * xlog2x(table(c, z, Ka, Kz)).sum()
    return (xlog2x(np.bincount(c)).sum() + s / M) / N


def binder_int(c, tr):
    """M A + P - 2 Q as a Python int: M times Binder's loss"""
    M, N = tr.shape
    Ka, Kz = int(c.max()) + 1, int(tr.max()) + 1
    A = int(c2(np.bincount(c).astype(object)).sum())
    P = sum(int(c2(np.bincount(z).astype(object)).sum()) for z in tr)
    Q = sum(int(c2(table(c, z, Ka, Kz).astype(object)).sum()) for z in tr)
    return M * A + P - 2 * Q


def loss_of(c, tr, loss):
    return vi_loss(c, tr) if loss == "VI" else binder_int(c, tr)


# ------------------------------------------------------------------ the gains

def gains_formula(c, tr, Ka, loss):
    """N x (Ka + 1): float64 for VI, int64 for Binder (the new class at Ka = 255 is +inf for
    VI; Binder's matrix is then returned as float64 with +inf there)"""
    c = np.asarray(c, np.int64)
    M, N = tr.shape
    Kz = int(tr.max()) + 1
    L = Ka + 1
    me = np.arange(N)
    na = np.bincount(c, minlength=L).astype(np.int64)       # n_Ka = 0
    if loss == "VI":
        S = np.zeros((N, L))
        for z in tr:                                         # draw order
            T = table(c, z, Ka, Kz)
            col = h(T)[:, z].T
            col[me, c] = h(T - 1)[c, z]
            S[:, :Ka] = S[:, :Ka] + col
        g = (M * (h(na)[None, :] - h(na - 1)[c][:, None]) - 2.0 * (S - S[me, c][:, None])) / (float(M) * N)
        g[me, c] = 0.0
    else:
        aff = np.zeros((N, L), np.int64)
        for z in tr:
            aff[:, :Ka] += table(c, z, Ka, Kz)[:, z].T
        g = M * (na[None, :] - na[c][:, None] - 1) - 2 * (aff - aff[me, c][:, None])
        g[me, c] = 0
    if Ka == 255:
        g = g.astype(np.float64)
        g[:, 255] = np.inf
    return g


def gains_brute(c, tr, Ka, loss):
    """the same by moving the point and recomputing the loss; object array of Python ints for
    Binder, float64 for VI.  Ka < 255."""
    c = np.asarray(c, np.int64)
    N = c.size
    base = loss_of(c, tr, loss)
    g = np.zeros((N, Ka + 1), object if loss == "Binder" else np.float64)
    for i in range(N):
        for b in range(Ka + 1):
            if b == c[i]:
                continue
            d = c.copy()
            d[i] = b
            g[i, b] = loss_of(d, tr, loss) - base
    return g


def best_of(g, c):
    """(best, gain): the smallest gain per row; the own class wins a tie, then the lowest class"""
    c = np.asarray(c, np.int64)
    best, bg = c.copy(), np.zeros(c.size, g.dtype if g.dtype != object else np.float64)
    for b in range(g.shape[1]):
        m = g[:, b] < bg
        best[m] = b
        bg[m] = g[m, b]
    return best, bg


def runner_up_gap(g):
    """per row the difference of the two smallest gains"""
    s = np.sort(np.asarray(g, np.float64), axis=1)
    return s[:, 1] - s[:, 0] if g.shape[1] > 1 else np.full(g.shape[0], np.inf)


# ------------------------------------------------------------------ the round rule

def select(best, gain, Ka):
    """the moves of one round in the order they are tried: [(i, to, gain)]"""
    cand = [i for i in range(len(gain)) if gain[i] < 0]
    fresh = [i for i in cand if best[i] == Ka]
    if fresh:
        keep = min(fresh, key=lambda i: (gain[i], i))
        cand = [i for i in cand if best[i] != Ka or i == keep]
    cand.sort(key=lambda i: (gain[i], i))
    return [(i, int(best[i]), gain[i]) for i in cand]


def refine_ref(c, tr, loss, max_rounds=100, gains=gains_formula):
    cur = relabel(c)
    K = int(cur.max()) + 1
    L = loss_of(cur, tr, loss)
    out = {"rounds": 0, "trials": 0, "moved": 0, "converged": False, "start": L, "history": [L]}
    while True:
        g = gains(cur, tr, K, loss)
        best, bg = best_of(g, cur)
        mv = select(best, bg, K)
        if not mv:
            out["converged"] = True
            break
        if out["rounds"] >= max_rounds:
            break
        k, accepted = len(mv), False
        while True:
            nxt = cur.copy()
            for i, to, _ in mv[:k]:
                nxt[i] = to
            nxt = relabel(nxt)
            Ln = loss_of(nxt, tr, loss)
            out["trials"] += 1
            if Ln < L:
                cur, K, L = nxt, int(nxt.max()) + 1, Ln
                out["moved"] += k
                out["rounds"] += 1
                out["history"].append(L)
                accepted = True
                break
            if k == 1:
                break
            k = (k + 1) // 2
        if not accepted:
            out["converged"] = True
            break
    out["cl"], out["value"], out["K"] = cur, L, K
    return out


# ------------------------------------------------------------------ the two constructions

PLANTED_SEED = 7


def planted(seed=PLANTED_SEED):
    """(truth, trace, start): N = 300 in classes of 150 / 100 / 50, M = 21 draws equal to the
    truth with 8 % of the labels of each draw redrawn from 4 labels, and a start with 40
    points shifted to the next class"""
    rng = np.random.default_rng(seed)
    truth = np.repeat(np.arange(3), [150, 100, 50])
    N, M = truth.size, 21
    tr = np.tile(truth, (M, 1))
    for z in tr:
        idx = rng.choice(N, size=N * 8 // 100, replace=False)
        z[idx] = rng.integers(0, 4, idx.size)
    start = truth.copy()
    idx = rng.choice(N, size=40, replace=False)
    start[idx] = (start[idx] + 1) % 3
    return truth, tr, start


def halving():
    """(trace, start): N = 12, M = 5; points 0 and 1 share a draw cluster of their own in
    every draw, the start has them in two singleton classes and the other ten together"""
    z = np.array([0, 0] + [1] * 10)
    return np.tile(z, (5, 1)), np.array([0, 1] + [2] * 10)
