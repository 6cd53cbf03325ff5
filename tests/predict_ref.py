"""A plain numpy / math restatement of the posterior predictive of include/hdpm.h
(hdpm_predict_*), for the tests of csrc/predict.hip and csrc/predict_host.hpp.

Per saved draw s: K_s clusters of sizes n_k (from the saved labels), centers c_kj, sigmas
sg_kj.  ll_k(y) = sum_j dhamming(y_j, c_kj, sg_kj, m_j) in attribute order; ll_0 =
-sum_j log m_j; w_k = log n_k + ll_k, w_0 = log gamma + ll_0; lse = log sum exp(w) with the
maximum subtracted; r_k = exp(w_k - lse).  math.exp / math.log are the host's libm, the one
the library's tables come from.
"""
import math

import numpy as np


def dhamming_pair(s: float, m: int):
    """(match, mismatch) exactly as csrc/rmath.hpp dhamming_pair writes them."""
    exp_term = math.exp(1.0 / s)
    attr_ratio = (m - 1.0) / exp_term
    denominator = math.log(1.0 + attr_ratio)
    num0 = 0.0 / s
    num1 = -1.0 / s
    return num0 - denominator, num1 - denominator


def pair_tables(sig, att):
    """match[k][j], mismatch[k][j] of a K x d array of sigmas."""
    sig = np.asarray(sig, np.float64)
    ma, mi = np.empty(sig.shape), np.empty(sig.shape)
    for k in range(sig.shape[0]):
        for j in range(sig.shape[1]):
            ma[k, j], mi[k, j] = dhamming_pair(float(sig[k, j]), int(att[j]))
    return ma, mi


def ll_scalar(y, cen, sig, att) -> float:
    """ll of one row under one cluster: a Python loop in attribute order."""
    acc = 0.0
    for j in range(len(att)):
        ma, mi = dhamming_pair(float(sig[j]), int(att[j]))
        acc = acc + (ma if int(y[j]) == int(cen[j]) else mi)
    return acc


def ll_matrix(Y, cen, sig, att) -> np.ndarray:
    """ll[y][k], the attribute loop in Python (same order, so the same bits as ll_scalar),
    rows and clusters through numpy's elementwise add."""
    Y, cen = np.asarray(Y, np.int64), np.asarray(cen, np.float64).astype(np.int64)
    ma, mi = pair_tables(sig, att)
    acc = np.zeros((Y.shape[0], cen.shape[0]))
    for j in range(len(att)):
        acc = acc + np.where(Y[:, j, None] == cen[None, :, j], ma[None, :, j], mi[None, :, j])
    return acc


def ll0(att) -> float:
    s = 0.0
    for m in att:
        s = s + math.log(float(m))
    return -s


def lse(w) -> float:
    mx = max(w)
    return mx + math.log(sum(math.exp(x - mx) for x in w))


def lse_mean(x) -> float:
    """log((1/M) sum exp(x))."""
    return lse(list(x)) - math.log(len(x))


def draw_weights(llm, labels, gamma, att):
    """w[y][0..K] of one draw from its ll matrix (ny x K) and its saved labels."""
    K = llm.shape[1]
    n = np.bincount(np.asarray(labels), minlength=K)
    w0 = math.log(gamma) + ll0(att)
    return [[w0] + [math.log(int(n[k])) + float(llm[y, k]) for k in range(K)] for y in range(llm.shape[0])]


def responsibilities(w):
    """(lse, r[0..K]) of one row's weights."""
    l = lse(w)
    return l, [math.exp(x - l) for x in w]


def new_rows(Y, c_trace, centers, sigmas, att, gamma, cl=None, Ka=0, table_form=False):
    """(lpd, p_new, coclass, lse[M x ny]) of the rows Y.  coclass from the definition: the
    mean over the points i of class a of r_{z_s(i)}, averaged over the draws; with
    table_form, from the contingency tables instead (the two agree to rounding)."""
    c_trace = np.asarray(c_trace)
    M, N = c_trace.shape
    ny = len(Y)
    lses = np.zeros((M, ny))
    pn = np.zeros(ny)
    co = np.zeros((ny, Ka)) if cl is not None else None
    if cl is not None:
        cl = np.asarray(cl)
        members = [np.flatnonzero(cl == a) for a in range(Ka)]
    for s in range(M):
        llm = ll_matrix(Y, centers[s], sigmas[s], att)
        W = draw_weights(llm, c_trace[s], gamma, att)
        K = llm.shape[1]
        for y in range(ny):
            l, r = responsibilities(W[y])
            lses[s, y] = l
            pn[y] += r[0]
            if cl is None:
                continue
            for a in range(Ka):
                if members[a].size == 0:
                    continue
                if table_form:
                    T = np.bincount(c_trace[s][members[a]], minlength=K)
                    co[y, a] += math.fsum(r[k + 1] * int(T[k]) for k in range(K)) / members[a].size
                else:
                    co[y, a] += math.fsum(r[int(z) + 1] for z in c_trace[s][members[a]]) / members[a].size
    lpd = np.array([lse_mean(lses[:, y]) - math.log(N + gamma) for y in range(ny)])
    if co is not None:
        co /= M
    return lpd, pn / M, co, lses


def own_ll(X, c_trace, centers, sigmas, att) -> np.ndarray:
    """l[s][i]: the ll of training row i under its own cluster in draw s."""
    c_trace = np.asarray(c_trace)
    M, N = c_trace.shape
    out = np.zeros((M, N))
    for s in range(M):
        llm = ll_matrix(X, centers[s], sigmas[s], att)
        out[s] = llm[np.arange(N), c_trace[s]]
    return out


def pointwise(X, c_trace, centers, sigmas, att):
    """(lppd, var, logcpo) of the training rows."""
    l = own_ll(X, c_trace, centers, sigmas, att)
    M, N = l.shape
    lppd = np.array([lse_mean(l[:, i]) for i in range(N)])
    cpo = np.array([-lse_mean(-l[:, i]) for i in range(N)])
    var = np.zeros(N)
    if M > 1:
        for i in range(N):
            mu = math.fsum(l[:, i]) / M
            var[i] = math.fsum((float(x) - mu) ** 2 for x in l[:, i]) / (M - 1)
    return lppd, var, cpo


def waic(lppd, var) -> float:
    return -2.0 * math.fsum(float(a) - float(b) for a, b in zip(lppd, var))


def lpml(cpo) -> float:
    return math.fsum(float(x) for x in cpo)


def problem(seed, N, d, Ks, att=None, sigma=(0.2, 1.5), noise=0.15):
    """A recorded chain made up for the tests: attrisize (mixed 2..255 unless given), M =
    len(Ks) draws whose labels cover exactly 0..K_s-1, their centers and sigmas, and N
    training rows scattered around the first draw's centers."""
    rng = np.random.default_rng(seed)
    if att is None:
        att = rng.choice([2, 3, 4, 6, 16, 17, 100, 255], size=d)
        att[0] = 255 if d > 1 else 2
        att[-1] = 2
    att = np.asarray(att, np.int32)
    cens, sigs, labs = [], [], []
    for K in Ks:
        cens.append(np.stack([rng.integers(1, att + 1) for _ in range(K)]).astype(np.float64))
        sigs.append(rng.uniform(sigma[0], sigma[1], size=(K, d)))
        z = rng.integers(0, K, size=N)
        z[rng.permutation(N)[:K]] = np.arange(K)     # every label present (N >= K)
        labs.append(z)
    c_trace = np.stack(labs).astype(np.int32)
    X = rows_near(rng, cens[0][c_trace[0]], att, noise)
    return {"att": att, "centers": cens, "sigmas": sigs, "c_trace": c_trace, "X": X, "rng": rng}


def rows_near(rng, base, att, noise):
    """Rows equal to `base` but for a share `noise` of the codes, redrawn uniformly."""
    base = np.asarray(base, np.int64)
    rand = rng.integers(1, np.asarray(att) + 1, size=base.shape)
    return np.where(rng.random(base.shape) < noise, rand, base).astype(np.uint8)
