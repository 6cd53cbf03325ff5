"""A plain Python restatement of the cluster profiles of include/hdpm.h (hdpm_predict_profile),
for the tests of csrc/profile.hip and csrc/profile_host.hpp.

For a point i of class a, draw s says "your center is c^s_{z_s(i)}, your sigma is
sg^s_{z_s(i)}".  With T^s[a][k] the contingency table of the partition against draw s and n_a
the class sizes:

  center_cnt[a][j][l-1] = sum_s sum_k T^s[a][k] [c^s_kj == l]
  sigma_trace[s][a][j]  = u_s = (sum_k float(T^s[a][k]) * sg^s_kj) / float(n_a)
  sigma_mean, sigma_var   Welford's recurrence over u_s in draw order
  code_pmf[a][j][l-1]   = (sum_s sum_k float(T^s[a][k]) * (em_kj if l == c^s_kj else ei_kj)) / (M n_a)

Every sum of a (class, attribute[, level]) runs over s in draw order and then over k in cluster
order, one multiply and one add per term, in doubles: numpy's elementwise multiply and add over
the attributes (and levels) are the same IEEE operations as Python's on floats, so a slice
updated per (s, a, k) holds what the scalar loops give, bit for bit.  Terms with T = 0 are
skipped: they add +0.0 to sums that are never negative, which changes no bit.  em / ei come
from math.exp of predict_ref.dhamming_pair.  center_cnt is computed twice, from the definition
over the points and from the tables, and the two are asserted equal here.
"""
import math

import numpy as np

from predict_ref import dhamming_pair, problem  # noqa: F401  (problem: the tests' recorded chains)


def tables(c_trace, cl, Ka):
    """T[s][a][k] as a list of Ka x K_s integer arrays."""
    c_trace, cl = np.asarray(c_trace), np.asarray(cl)
    out = []
    for z in c_trace:
        K = int(z.max()) + 1
        T = np.zeros((Ka, K), np.int64)
        np.add.at(T, (cl, z), 1)
        out.append(T)
    return out


def exp_pairs(sig, att):
    """em[k][j], ei[k][j] = math.exp of dhamming's (match, mismatch) of a K x d array of sigmas."""
    sig = np.asarray(sig, np.float64)
    em, ei = np.empty(sig.shape), np.empty(sig.shape)
    for k in range(sig.shape[0]):
        for j in range(sig.shape[1]):
            ma, mi = dhamming_pair(float(sig[k, j]), int(att[j]))
            em[k, j], ei[k, j] = math.exp(ma), math.exp(mi)
    return em, ei


def center_cnt_points(c_trace, centers, cl, Ka, d, ld):
    """sum_s sum_{i in a} [c^s_{z_s(i), j} == l]: the definition over the points."""
    c_trace, cl = np.asarray(c_trace), np.asarray(cl)
    cnt = np.zeros((Ka, d, ld), np.int64)
    jj = np.arange(d)
    for s, z in enumerate(c_trace):
        cen = np.asarray(centers[s]).astype(np.int64)
        for i in range(z.size):
            np.add.at(cnt, (int(cl[i]), jj, cen[int(z[i])] - 1), 1)
    return cnt


def profile(c_trace, centers, sigmas, att, cl, Ka, ld, want_pmf=True):
    """{"center_cnt", "code_pmf", "sigma_mean", "sigma_var", "sigma_trace", "sizes"}."""
    c_trace, cl, att = np.asarray(c_trace), np.asarray(cl), np.asarray(att)
    M, N = c_trace.shape
    d = att.size
    assert ld >= att.max()
    T = tables(c_trace, cl, Ka)
    na = np.bincount(cl, minlength=Ka).astype(np.int64)
    cnt = np.zeros((Ka, d, ld), np.int64)
    law = np.zeros((Ka, d, ld))
    trace = np.zeros((M, Ka, d))
    mean, m2 = np.zeros((Ka, d)), np.zeros((Ka, d))
    jj, lev = np.arange(d), np.arange(1, ld + 1)
    for s in range(M):
        cen, sig = np.asarray(centers[s]).astype(np.int64), np.asarray(sigmas[s], np.float64)
        K = cen.shape[0]
        assert T[s].shape[1] == K
        if want_pmf:
            em, ei = exp_pairs(sig, att)
        acc = np.zeros((Ka, d))
        for a in range(Ka):
            for k in range(K):
                t = int(T[s][a, k])
                if t == 0:
                    continue
                cnt[a, jj, cen[k] - 1] += t
                acc[a] = acc[a] + float(t) * sig[k]
                if want_pmf:
                    law[a] = law[a] + float(t) * np.where(lev[None, :] == cen[k][:, None], em[k][:, None], ei[k][:, None])
        u = np.zeros((Ka, d))
        for a in range(Ka):
            if na[a] > 0:
                u[a] = acc[a] / float(na[a])
        trace[s] = u
        delta = u - mean
        mean = mean + delta / float(s + 1)
        m2 = m2 + delta * (u - mean)
    var = m2 / float(M - 1) if M > 1 else np.zeros((Ka, d))
    pmf = np.zeros((Ka, d, ld))
    for a in range(Ka):
        if na[a] > 0:
            pmf[a] = law[a] / float(M * int(na[a]))
    pmf[:, lev[None, :] > att[:, None]] = 0.0
    assert np.array_equal(cnt, center_cnt_points(c_trace, centers, cl, Ka, d, ld))
    return {"center_cnt": cnt.astype(np.uint64), "code_pmf": pmf, "sigma_mean": mean, "sigma_var": var,
            "sigma_trace": trace, "sizes": na}


def mode_of(cnt, sizes):
    """The first arg-max level, 1-based; 0 for an empty class."""
    out = np.zeros(cnt.shape[:2], np.int64)
    for a in range(cnt.shape[0]):
        if sizes[a] == 0:
            continue
        for j in range(cnt.shape[1]):
            row = [int(x) for x in cnt[a, j]]
            out[a, j] = 1 + row.index(max(row))
    return out
