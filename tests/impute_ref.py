"""A plain numpy / math restatement of the predictive of rows with missing attributes
(include/hdpm.h: hdpm_predict_partial, hdpm_predict_impute), for the tests of csrc/predict.hip
and csrc/predict_host.hpp.  Code 0 in a row is a missing attribute.

Written from the definition, not from the kernel's running-maximum form: per draw the lse and
the r_k come from predict_ref (with the missing attributes left out of ll_k and ll_0), and

    pmf_l = sum_s exp(lse_s - max) q^s_l / sum_s exp(lse_s - max),
    q^s_l = r_0 / m_j + sum_k r_k * exp(dhamming(l, c_kj, sg_kj, m_j)),

which is p(y_j = l | y_O, data) = sum_s p(y_O, y_j = l | s) / sum_s p(y_O | s).
"""
import math

import numpy as np

import predict_ref as ref


def ll_matrix(Y, cen, sig, att) -> np.ndarray:
    """ll[y][k] over the observed attributes of each row, in attribute order."""
    Y, cen = np.asarray(Y, np.int64), np.asarray(cen, np.float64).astype(np.int64)
    ma, mi = ref.pair_tables(sig, att)
    acc = np.zeros((Y.shape[0], cen.shape[0]))
    for j in range(len(att)):
        t = np.where(Y[:, j, None] == cen[None, :, j], ma[None, :, j], mi[None, :, j])
        acc = acc + np.where(Y[:, j, None] == 0, 0.0, t)
    return acc


def ll0_row(y, att) -> float:
    s = 0.0
    for j, m in enumerate(att):
        if int(y[j]) != 0:
            s = s + math.log(float(m))
    return -s


def draw_terms(Y, labels, cen, sig, att, gamma):
    """(lse[y], r[y][0..K]) of one draw."""
    llm = ll_matrix(Y, cen, sig, att)
    K = llm.shape[1]
    n = np.bincount(np.asarray(labels), minlength=K)
    lses, rs = [], []
    for y in range(len(Y)):
        w = [math.log(gamma) + ll0_row(Y[y], att)] + [math.log(int(n[k])) + float(llm[y, k]) for k in range(K)]
        l, r = ref.responsibilities(w)
        lses.append(l)
        rs.append(r)
    return np.array(lses), np.array(rs)


def all_terms(Y, c_trace, centers, sigmas, att, gamma):
    """lse[M x ny] and the list of r (ny x (K_s + 1)) per draw."""
    out = [draw_terms(Y, c_trace[s], centers[s], sigmas[s], att, gamma) for s in range(len(centers))]
    return np.stack([o[0] for o in out]), [o[1] for o in out]


def partial(Y, c_trace, centers, sigmas, att, gamma, cl=None, Ka=0, terms=None):
    """(lpd, p_new, coclass | None); coclass from the definition, as predict_ref.new_rows."""
    c_trace = np.asarray(c_trace)
    M, N = c_trace.shape
    lses, rs = terms if terms is not None else all_terms(Y, c_trace, centers, sigmas, att, gamma)
    ny = len(Y)
    lpd = np.array([ref.lse_mean(lses[:, y]) - math.log(N + gamma) for y in range(ny)])
    pn = np.array([math.fsum(rs[s][y, 0] for s in range(M)) / M for y in range(ny)])
    co = None
    if cl is not None:
        cl = np.asarray(cl)
        co = np.zeros((ny, Ka))
        for a in range(Ka):
            mem = np.flatnonzero(cl == a)
            if mem.size == 0:
                continue
            for s in range(M):
                T = np.bincount(c_trace[s][mem], minlength=rs[s].shape[1] - 1)
                # sum over the members i of r_{z_s(i)}: every member of cluster k adds r_k
                co[:, a] += (rs[s][:, 1:] * T[None, :]).sum(axis=1) / mem.size
        co /= M
    return lpd, pn, co


def level_pmf(cen, sig, att, j):
    """E[k][l - 1] = exp(dhamming(l, c_kj, sg_kj, m_j)) for the K clusters of a draw."""
    m = int(att[j])
    E = np.zeros((cen.shape[0], m))
    for k in range(cen.shape[0]):
        ma, mi = ref.dhamming_pair(float(sig[k, j]), m)
        E[k, :] = math.exp(mi)
        E[k, int(cen[k, j]) - 1] = math.exp(ma)
    return E


def impute(Y, c_trace, centers, sigmas, att, gamma, ld=None, terms=None):
    """(rows, attrs, pmf, mode, lpd) as Predictive.impute returns them."""
    Y = np.asarray(Y)
    c_trace = np.asarray(c_trace)
    M = c_trace.shape[0]
    lses, rs = terms if terms is not None else all_terms(Y, c_trace, centers, sigmas, att, gamma)
    rows, attrs = np.nonzero(Y == 0)
    if ld is None:
        ld = int(np.asarray(att)[attrs].max()) if rows.size else 0
    pmf = np.zeros((rows.size, ld))
    tables = {}
    for e, (y, j) in enumerate(zip(rows, attrs)):
        m = int(att[j])
        if j not in tables:
            tables[j] = [level_pmf(np.asarray(centers[s]), np.asarray(sigmas[s]), att, j) for s in range(M)]
        top = max(lses[:, y])
        num, den = np.zeros(m), 0.0
        for s in range(M):
            r = rs[s][y]
            q = np.full(m, r[0] / m)
            for k in range(len(r) - 1):
                q = q + r[k + 1] * tables[j][s][k]
            f = math.exp(lses[s, y] - top)
            num += f * q
            den += f
        pmf[e, :m] = num / den
    mode = np.argmax(pmf, axis=1) + 1 if rows.size else np.zeros(0, np.int64)
    return rows, attrs, pmf, mode, partial(Y, c_trace, centers, sigmas, att, gamma, terms=(lses, rs))[0]


def mask(Y, pattern, rng=None):
    """A copy of Y with gaps: "none", "all", "first", "last", "alternate" (every other
    attribute), "one" (one random gap per row), "row" (the middle row all missing, the rest complete)."""
    Y = np.array(Y, np.uint8)
    if pattern == "all":
        Y[:] = 0
    elif pattern == "first":
        Y[:, 0] = 0
    elif pattern == "last":
        Y[:, -1] = 0
    elif pattern == "alternate":
        Y[:, ::2] = 0
    elif pattern == "one":
        Y[np.arange(len(Y)), rng.integers(0, Y.shape[1], size=len(Y))] = 0
    elif pattern == "row":
        Y[len(Y) // 2] = 0
    elif pattern != "none":
        raise ValueError(pattern)
    return Y
