"""Posterior analysis of saved chains, as realdata_analysis/zoo_simulator.R:193-236, 339-344.

The reference script summarises every run with CRAN packages:
  * ``comp.psm(C)`` (mcclust) -- the posterior similarity matrix of the saved labels;
  * ``minVI(psm)`` (mcclust.ext) -- the partition minimising ``VI.lb``, the lower bound of
    the posterior expected variation of information (default method "avg": cuts of the
    average-linkage tree of 1 - psm into 1..ceiling(N / 8) clusters; "draws": the saved
    partitions themselves);
  * ``arandi(VI$cl, gt)`` (mcclust) -- the adjusted Rand index against the ground truth;
  * ``ESS`` and ``IAT`` (LaplacesDemon) of (total_cls, loglikelihood).

The N x N matrix is built and queried on the device (csrc/posterior.hip through
``hdpm_psm_*``): at C4 (N = 70k) it has 4.9e9 entries.  ``LabelTrace`` gives the same
summaries of candidate partitions (VI.lb, the expected VI, Binder's loss) from the saved
labels alone (csrc/trace_summary.hip through ``hdpm_trace_*``), for sizes where the matrix
cannot be held (C5: N = 1M would be 4 TB), and ``minvi_avg`` / ``minbinder_avg`` run minVI's
default search -- the cuts of the average-linkage tree -- on the groups of points whose
labels agree in every draw, again with no matrix.  ``credible_ball`` (mcclust.ext
``credibleball``) and ``LabelTrace.membership`` / ``cluster_similarity`` (the content of the
script's PSM plot ordered by ``VI$cl``) say how far that estimate can be trusted, from the
same tables (csrc/trace_uncertainty.hip), and ``refine`` improves it by single-point moves on
the expected VI or Binder's loss until no move helps (csrc/trace_refine.hip;
``LabelTrace.move_gains`` gives every point's best move) and, with ``merges``, by merging two
classes where single moves stall (csrc/trace_merge.hip; ``LabelTrace.merge_gains`` gives every
pair's gain, ``LabelTrace.merge_path`` with ``coarsen`` the greedy agglomeration and the loss of
each of its levels).  ``Predictive`` reads the recorded centers and
sigmas beside the labels (csrc/predict.hip through ``hdpm_predict_*``): the posterior
predictive of rows the chain never saw -- their density, their class of a point estimate, the
probability of a cluster of their own -- and the pointwise log-likelihood of the training rows
behind ``waic`` and ``lpml``; ``Predictive.profile`` (csrc/profile.hip) says what each class of
an estimate is, the posterior law of its center codes and its sigmas with their spread, with no
matching of labels between draws.  ``arandi``, ``ess`` and ``iat`` are
restated on the host.  None of these packages is installed here (no R), so their parity is
unpinned; ``arandi`` is checked against scikit-learn's adjusted Rand score.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import ptr


class PSM:
    """comp.psm(C) on the device: ``c_trace`` is the M x N matrix of saved labels
    (results$c_i, any integers).  The PSM depends only on which points share a label within
    an iteration, so each saved row is relabelled 0..K_m-1 first (the device packs one byte
    per label: at most 255 clusters in one iteration, else ValueError).  Rows come back as
    doubles (count / M)."""

    def __init__(self, c_trace, engine=None, device: int = 0):
        from .sampler import Engine
        tr = np.ascontiguousarray(c_trace, dtype=np.int32)
        if tr.ndim != 2:
            raise ValueError("c_trace must be M x N")
        self.M, self.N = tr.shape
        dense = np.empty_like(tr)
        for q in range(self.M):
            u, dense[q] = np.unique(tr[q], return_inverse=True)
            if u.size > 255:
                raise ValueError(f"iteration {q} has {u.size} clusters; the device PSM packs at most 255")
        tr = np.ascontiguousarray(dense, dtype=np.int32)
        self._own = engine is None
        self.eng = Engine(device) if engine is None else engine
        self.eng._check(self.eng._L.hdpm_psm_build(self.eng._h, ptr(tr), self.M, self.N))

    def close(self):
        if self._own and self.eng is not None:
            self.eng.close()
        self.eng = None

    def rows(self, row0: int, nrows: int) -> np.ndarray:
        out = np.zeros((nrows, self.N))
        self.eng._check(self.eng._L.hdpm_psm_rows(self.eng._h, int(row0), int(nrows), ptr(out)))
        return out

    def matrix(self) -> np.ndarray:
        return self.rows(0, self.N)

    def vi_lb(self, cls) -> np.ndarray:
        """mcclust.ext VI.lb(cls, psm) of each row of ``cls`` (candidate partitions)."""
        c = np.ascontiguousarray(np.atleast_2d(cls), dtype=np.int32)
        if c.shape[1] != self.N:
            raise ValueError("partitions must have N labels")
        c = np.stack([np.unique(r, return_inverse=True)[1] for r in c]).astype(np.int32)
        out = np.zeros(c.shape[0])
        self.eng._check(self.eng._L.hdpm_psm_vi_lb(self.eng._h, ptr(c), c.shape[0], ptr(out)))
        return out


def _relabel(rows: np.ndarray, what: str) -> np.ndarray:
    """Each row relabelled 0..K-1 (int32); ValueError above 255 clusters in a row."""
    dense = np.empty(rows.shape, np.int32)
    small = np.issubdtype(rows.dtype, np.integer) and rows.size > 0 and rows.min() >= 0 and rows.max() < (1 << 20)
    for q in range(rows.shape[0]):
        if small:
            # ranks of the labels present, by counting (no sort): what np.unique's inverse is
            present = np.bincount(rows[q]) > 0
            k = int(present.sum())
            if k <= 255:
                dense[q] = (np.cumsum(present) - 1).astype(np.int32)[rows[q]]
        else:
            u, dense[q] = np.unique(rows[q], return_inverse=True)
            k = u.size
        if k > 255:
            raise ValueError(f"{what} {q} has {k} clusters; the device packs at most 255")
    return dense


class LabelTrace:
    """The posterior summaries of ``PSM`` from the saved labels alone, with no N x N matrix
    (csrc/trace_summary.hip through ``hdpm_trace_*``): O(M N) work and bytes per candidate
    partition, so it runs at sizes where the matrix cannot be held (C5: N = 1M).

    ``c_trace`` is the M x N matrix of saved labels (results$c_i, any integers), relabelled
    0..K_m-1 per iteration as ``PSM`` does; ValueError above 255 clusters in an iteration or
    in a candidate partition.  The device keeps one byte per saved label and, per block of
    candidates, their contingency tables against every draw; ``table_budget`` (bytes, None:
    the library's default) bounds that table array and changes no result.

    With T^m the table of a candidate c against draw z_m and n^m the draw's cluster sizes:
    ``terms`` gives the integer sums M sum_j psm_ij and M sum_{j: c_j = c_i} psm_ij,
    ``vi_lb`` mcclust.ext VI.lb(c, psm) (the value ``PSM.vi_lb`` gives), ``vi`` the posterior
    expected VI (mcclust.ext VI(cls, cls.draw)), and ``binder`` Binder's loss
    sum_{i<j} |1(c_i = c_j) - psm_ij|.  mcclust's own scaling of Binder's loss is unpinned
    (the package is absent here); only the argmin matters to ``minbinder``."""

    def __init__(self, c_trace, engine=None, device: int = 0, table_budget: int | None = None):
        from .sampler import Engine
        tr = np.asarray(c_trace)
        if tr.ndim != 2 or tr.size == 0:
            raise ValueError("c_trace must be M x N")
        self.M, self.N = tr.shape
        self._lo, self._hi = tr.min(axis=1), tr.max(axis=1)     # the saved labels' range per draw (Predictive)
        tr = np.ascontiguousarray(_relabel(tr, "iteration"))
        self._own = engine is None
        self.eng = Engine(device) if engine is None else engine
        self.eng._check(self.eng._L.hdpm_trace_build(self.eng._h, ptr(tr), self.M, self.N,
                                                     int(table_budget or 0)))

    def close(self):
        if self._own and self.eng is not None:
            self.eng.close()
        self.eng = None

    def _cands(self, cls) -> np.ndarray:
        c = np.atleast_2d(np.asarray(cls))
        if c.ndim != 2 or c.shape[1] != self.N:
            raise ValueError("partitions must have N labels")
        return np.ascontiguousarray(_relabel(c, "candidate partition"))

    def terms(self, cls):
        """(all, same): all[i] = sum_m n^m[z_m(i)] (N) and same[c][i] = sum_m
        T^m[c_i][z_m(i)] (ncand x N), uint64, exact."""
        c = self._cands(cls)
        all_ = np.zeros(self.N, np.uint64)
        same = np.zeros(c.shape, np.uint64)
        self.eng._check(self.eng._L.hdpm_trace_terms(self.eng._h, ptr(c), c.shape[0], ptr(all_), ptr(same)))
        return all_, same

    def _losses(self, cls, vi_lb=False, vi=False, binder=False):
        c = self._cands(cls)
        k = c.shape[0]
        lb = np.zeros(k) if vi_lb else None
        v = np.zeros(k) if vi else None
        q = np.zeros(k, np.uint64) if binder else None
        p = np.zeros(1, np.uint64) if binder else None
        self.eng._check(self.eng._L.hdpm_trace_losses(self.eng._h, ptr(c), k, ptr(lb), ptr(v), ptr(q), ptr(p)))
        return c, lb, v, q, p

    def vi_lb(self, cls) -> np.ndarray:
        """mcclust.ext VI.lb(cls, psm) of each row of ``cls``."""
        return self._losses(cls, vi_lb=True)[1]

    def vi(self, cls) -> np.ndarray:
        """mcclust.ext VI(cls, cls.draw), the posterior expected variation of information,
        of each row of ``cls``."""
        return self._losses(cls, vi=True)[2]

    def binder_terms(self, cls):
        """The integers of Binder's loss A + (P - 2 Q) / M as Python ints: ([A_c], P, [Q_c])."""
        c, _, _, q, p = self._losses(cls, binder=True)
        A = []
        for r in c:
            n = np.bincount(r).tolist()
            A.append(sum(x * (x - 1) // 2 for x in n))
        return A, int(p[0]), [int(x) for x in q]

    def binder(self, cls) -> np.ndarray:
        """Binder's loss sum_{i<j} |1(c_i = c_j) - psm_ij| of each row of ``cls``: the three
        integer sums combined as Python ints, one division."""
        A, P, Q = self.binder_terms(cls)
        return np.array([a + (P - 2 * q) / self.M for a, q in zip(A, Q)], np.float64)

    def tables(self, cls, m0: int = 0, nm: int | None = None) -> np.ndarray:
        """T^m of each row of ``cls`` for draws m0 .. m0 + nm - 1 (ncand x nm x 256 x 256
        uint32; testing and inspection)."""
        c = self._cands(cls)
        nm = self.M - int(m0) if nm is None else int(nm)
        if m0 < 0 or nm <= 0 or m0 + nm > self.M:
            raise ValueError("draws m0 .. m0 + nm - 1 must lie in 0 .. M - 1")
        out = np.zeros((c.shape[0], nm, 256, 256), np.uint32)
        self.eng._check(self.eng._L.hdpm_trace_tables(self.eng._h, ptr(c), c.shape[0], int(m0), nm, ptr(out)))
        return out

    # ---- how far an estimate can be trusted (csrc/trace_uncertainty.hip)

    def distances(self, cls):
        """(vi, binder, draw_k): the distance of each row of ``cls`` to every saved draw.
        vi[c][m] is the variation of information (ncand x M doubles; draws with equal labels
        give bit-equal values), binder[c][m] the number of pairs i < j on which the two
        partitions disagree (ncand x M uint64, exact: the pair count, not mcclust's scaling of
        Binder's loss, which is unpinned here), draw_k[m] the number of clusters of draw m."""
        c = self._cands(cls)
        vi = np.zeros((c.shape[0], self.M))
        binder = np.zeros((c.shape[0], self.M), np.uint64)
        draw_k = np.zeros(self.M, np.int32)
        self.eng._check(self.eng._L.hdpm_trace_distances(self.eng._h, ptr(c), c.shape[0], ptr(vi), ptr(binder),
                                                         ptr(draw_k)))
        return vi, binder, draw_k

    def _one(self, cl) -> np.ndarray:
        c = self._cands(cl)
        if c.shape[0] != 1:
            raise ValueError("one partition of N labels is needed")
        return c

    def affinity(self, cl):
        """(aff, cross) of one partition ``cl`` (relabelled 0..Ka-1 as the candidates are):
        aff[i][a] = sum_m T^m[a][z_m(i)] = M sum_{j: c_j = a} psm_ij (N x Ka) and cross[a][b] =
        sum_m sum_z T^m[a][z] T^m[b][z] = M sum_{i in a, j in b} psm_ij (Ka x Ka, symmetric),
        uint64, exact.  aff comes off the device in blocks of points within the table budget."""
        c = self._one(cl)
        Ka = int(c.max()) + 1
        aff = np.zeros((self.N, Ka), np.uint64)
        cross = np.zeros((Ka, Ka), np.uint64)
        self.eng._check(self.eng._L.hdpm_trace_affinity(self.eng._h, ptr(c), Ka, ptr(aff), ptr(cross)))
        return aff, cross

    def membership(self, cl) -> np.ndarray:
        """N x Ka doubles: the mean psm of point i with the members of cluster a of ``cl``, the
        point itself excluded, (aff[i][a] - M [c_i = a]) / (M (n_a - [c_i = a])); 1.0 by
        convention for a point alone in its own cluster.  A row whose arg-max over a differs
        from c_i marks a point the estimate places against its own average similarity."""
        c = self._one(cl)[0]
        Ka = int(c.max()) + 1
        aff = np.zeros((self.N, Ka), np.uint64)
        self.eng._check(self.eng._L.hdpm_trace_affinity(self.eng._h, ptr(c), Ka, ptr(aff), None))
        own = np.zeros((self.N, Ka), np.int64)
        own[np.arange(self.N), c] = 1
        num = aff.astype(np.int64) - self.M * own          # aff <= M N < 2^63
        den = self.M * (np.bincount(c, minlength=Ka).astype(np.int64)[None, :] - own)
        out = np.ones((self.N, Ka))
        np.divide(num, den, out=out, where=den > 0)
        return out

    def cluster_similarity(self, cl) -> np.ndarray:
        """Ka x Ka doubles: the mean psm between the members of clusters a and b of ``cl``,
        cross[a][b] / (M n_a n_b); on the diagonal the self pairs are excluded,
        (cross[a][a] - M n_a) / (M n_a (n_a - 1)), 1.0 for a singleton.  This is the block
        mean of the PSM ordered by the classes of ``cl``.  The integers are combined as Python
        ints and divided once."""
        c = self._one(cl)[0]
        Ka = int(c.max()) + 1
        cross = np.zeros((Ka, Ka), np.uint64)
        self.eng._check(self.eng._L.hdpm_trace_affinity(self.eng._h, ptr(c), Ka, None, ptr(cross)))
        n = np.bincount(c, minlength=Ka).tolist()
        x = cross.tolist()
        out = np.ones((Ka, Ka))
        for a in range(Ka):
            for b in range(Ka):
                if a != b:
                    out[a, b] = x[a][b] / (self.M * n[a] * n[b])
                elif n[a] > 1:
                    out[a, a] = (x[a][a] - self.M * n[a]) / (self.M * n[a] * (n[a] - 1))
        return out

    # ---- single-point moves (csrc/trace_refine.hip)

    def move_gains(self, cl, loss: str = "VI", full: bool = False, Ka: int | None = None):
        """(best, gain[, gains]): what moving each point alone to another class of ``cl``
        (relabelled 0..Ka-1 as the candidates are; with ``Ka`` given, labels 0..Ka-1 as they
        stand, so a class may be empty) would change in ``loss``: "VI", the change of ``vi``, or
        "Binder", the change of the exact integer M A + P - 2 Q (M times ``binder``), as a
        double that holds it.  gains is N x (Ka + 1), column Ka a new class of its own (+inf at
        Ka = 255) and the own class 0; best[i] is the class with the smallest gain (the own
        class wins a tie, then the lowest class) and gain[i] that gain.  Only best and gain
        leave the device unless ``full``."""
        code = _loss_code(loss)
        if Ka is None:
            c = self._one(cl)[0]
            Ka = int(c.max()) + 1
        else:
            c = np.ascontiguousarray(cl, dtype=np.int32).ravel()
            if c.size != self.N:
                raise ValueError("the partition must have N labels")
        best, gain = np.zeros(self.N, np.int32), np.zeros(self.N)
        gains = np.zeros((self.N, max(int(Ka), 0) + 1)) if full else None
        self.eng._check(self.eng._L.hdpm_trace_move_gains(self.eng._h, ptr(c), int(Ka), code, ptr(best), ptr(gain),
                                                          ptr(gains)))
        return (best, gain, gains) if full else (best, gain)

    # ---- pair merges (csrc/trace_merge.hip)

    def _as_given(self, cl, Ka):
        """(labels, Ka): relabelled 0..Ka-1 as the candidates are, or, with ``Ka`` given, the
        labels 0..Ka-1 as they stand"""
        if Ka is None:
            c = self._one(cl)[0]
            return c, int(c.max()) + 1
        c = np.ascontiguousarray(cl, dtype=np.int32).ravel()
        if c.size != self.N:
            raise ValueError("the partition must have N labels")
        return c, int(Ka)

    def merge_gains(self, cl, loss: str = "VI", Ka: int | None = None):
        """(gain, best, best_gain): what merging two classes of ``cl`` (relabelled 0..Ka-1 as the
        candidates are; with ``Ka`` given, labels 0..Ka-1 as they stand, so a class may be empty)
        would change in ``loss``: "VI", the change of ``vi``, or "Binder", the change of the
        exact integer M A + P - 2 Q (M times ``binder``), as a double that holds it.  gain is
        Ka x Ka, symmetric, 0 on the diagonal and for a pair with an empty class; best is the
        pair a < b of non-empty classes with the smallest gain (the lowest a wins a tie, then the
        lowest b), (-1, -1) with gain 0 if there are fewer than two.  One table pass, whatever
        the number of pairs."""
        code = _loss_code(loss)
        c, Ka = self._as_given(cl, Ka)
        gain = np.zeros((max(Ka, 0), max(Ka, 0)))
        best, bg = np.zeros(2, np.int32), np.zeros(1)
        self.eng._check(self.eng._L.hdpm_trace_merge_gains(self.eng._h, ptr(c), Ka, code, ptr(gain), ptr(best),
                                                           ptr(bg)))
        return gain, (int(best[0]), int(best[1])), float(bg[0])

    def merge_path(self, cl, loss: str = "VI", k_min: int = 1, Ka: int | None = None) -> dict:
        """Greedy agglomeration of the classes of ``cl`` (labels as in ``merge_gains``) down to
        ``k_min`` classes: each step merges the pair with the smallest gain, negative or not, and
        the merged class keeps the lower label.  Returns {"merge" (steps x 2: the labels a < b of
        each step), "step_gain" (steps), "value" (steps + 1: the loss of ``cl`` and after each
        step, evaluated from the merged tables: ``vi``, or Binder's integer M A + P - 2 Q as a
        double)}.  ``coarsen`` gives the labels of a level.  One pass over the points in all."""
        code = _loss_code(loss)
        c, Ka = self._as_given(cl, Ka)
        rows = max(Ka - 1, 0)
        merge, gain, value = np.zeros((rows, 2), np.int32), np.zeros(rows), np.zeros(rows + 1)
        steps = C.c_int32(0)
        self.eng._check(self.eng._L.hdpm_trace_merge_path(self.eng._h, ptr(c), Ka, code, int(k_min), ptr(merge),
                                                          ptr(gain), ptr(value), C.byref(steps)))
        s = int(steps.value)
        return {"merge": merge[:s], "step_gain": gain[:s], "value": value[:s + 1]}

    # ---- the average-linkage tree without the matrix (hdpm_trace_groups .. _cut_labels)

    def groups(self, max_groups: int = 8192, hash_bits: int = 0) -> dict:
        """The groups of points whose labels agree in every draw, numbered by ascending
        smallest member: {"U", "first" (U), "weight" (U), "group_of" (N), "counts" (U x U
        uint32: the draws in which two groups share a cluster)}.  More than ``max_groups``
        distinct label columns (at most 16384) raise ``HdpmError``: such a trace is too
        unsettled for the tree.  ``hash_bits`` (1..32) truncates the device's hash (testing);
        it changes no result."""
        U = C.c_int32(0)
        self.eng._check(self.eng._L.hdpm_trace_groups(self.eng._h, int(max_groups), int(hash_bits), C.byref(U)))
        self.U = U = int(U.value)
        first, weight = np.zeros(U, np.int32), np.zeros(U, np.int32)
        group_of, counts = np.zeros(self.N, np.int32), np.zeros((U, U), np.uint32)
        self.eng._check(self.eng._L.hdpm_trace_group_info(self.eng._h, ptr(first), ptr(weight), ptr(group_of),
                                                          ptr(counts)))
        return {"U": U, "first": first, "weight": weight, "group_of": group_of, "counts": counts}

    def avg_tree(self):
        """(merge, height) of weighted average linkage on the groups (``groups`` first):
        hclust(as.dist(1 - psm), "average") above height 0.  merge is (U - 1) x 2, each
        cluster named by its lowest-numbered group, column 0 the name the merged cluster
        keeps; ties are broken as include/hdpm.h states, in exact integer arithmetic.
        height = 1 - the average psm between the two clusters (inspection only)."""
        U = getattr(self, "U", 1)
        merge, height = np.zeros((max(U - 1, 0), 2), np.int32), np.zeros(max(U - 1, 0))
        self.eng._check(self.eng._L.hdpm_trace_avg_tree(self.eng._h, ptr(merge), ptr(height)))
        return merge, height

    def cut(self, k: int) -> np.ndarray:
        """cutree(k): the tree's partition into k clusters (1..U), labels 0..k-1 in order of
        first appearance (``avg_tree`` first)."""
        cl = np.zeros(self.N, np.int32)
        self.eng._check(self.eng._L.hdpm_trace_cut_labels(self.eng._h, int(k), ptr(cl)))
        return cl

    def cut_losses(self, k0: int, nk: int):
        """(vi_lb, vi, binder_A, binder_Q) of the cuts k0 .. k0 + nk - 1 (at most min(U, 255)),
        from tables over the groups: the values ``vi_lb`` / ``vi`` / ``binder_terms`` give for
        ``cut(k)``."""
        lb, v = np.zeros(nk), np.zeros(nk)
        a, q = np.zeros(nk, np.uint64), np.zeros(nk, np.uint64)
        self.eng._check(self.eng._L.hdpm_trace_cut_losses(self.eng._h, int(k0), int(nk), ptr(lb), ptr(v), ptr(a),
                                                          ptr(q)))
        return lb, v, a, q


class Predictive:
    """The posterior predictive from the recorded draws (csrc/predict.hip through
    ``hdpm_predict_*``; the model and the orders of summation are in include/hdpm.h).

    ``trace`` is the ``LabelTrace`` of the saved labels; ``centers`` and ``sigmas`` are the
    lists of K_s x d arrays that ``run_markov_chain(..., keep_params=True)`` returns for the
    same saved iterations; ``attrisize`` and ``gamma`` are the chain's.  Label k of draw s
    names row k of that draw's parameters, so the saved labels of draw s must be exactly
    0..K_s-1 (ValueError otherwise): ``LabelTrace``'s relabelling is then the identity.  Rows
    hold codes 1..m_j; ``partial`` and ``impute`` alone take 0 for a missing attribute.  The
    trace's ``table_budget`` bounds the device staging of a block of rows and changes no
    result."""

    def __init__(self, trace: LabelTrace, centers, sigmas, attrisize, gamma: float):
        if not isinstance(trace, LabelTrace):
            raise ValueError("Predictive needs a LabelTrace")
        if len(centers) != trace.M or len(sigmas) != trace.M:
            raise ValueError("centers and sigmas must hold one array per saved iteration")
        self.trace, self.M, self.N = trace, trace.M, trace.N
        self.att = np.ascontiguousarray(attrisize, dtype=np.int32).ravel()
        self.d = int(self.att.size)
        cen = [np.asarray(c, np.float64).reshape(-1, self.d) for c in centers]
        sig = [np.asarray(s, np.float64).reshape(-1, self.d) for s in sigmas]
        self.K = np.array([c.shape[0] for c in cen], np.int32)
        eng = trace.eng
        # K_s distinct labels with smallest 0 and largest K_s - 1 are exactly 0..K_s-1
        draw_k, one = np.zeros(self.M, np.int32), np.zeros((1, self.N), np.int32)
        eng._check(eng._L.hdpm_trace_distances(eng._h, ptr(one), 1, None, None, ptr(draw_k)))
        for s in range(self.M):
            if sig[s].shape != cen[s].shape:
                raise ValueError(f"draw {s}: centers and sigmas differ in shape")
            if trace._lo[s] != 0 or trace._hi[s] != self.K[s] - 1 or draw_k[s] != self.K[s]:
                raise ValueError(f"draw {s}: the saved labels must be exactly 0..{self.K[s] - 1}")
        cen_all, sig_all = np.ascontiguousarray(np.concatenate(cen)), np.ascontiguousarray(np.concatenate(sig))
        eng._check(eng._L.hdpm_predict_build(eng._h, self.d, ptr(self.att), float(gamma), ptr(self.K), ptr(cen_all),
                                             ptr(sig_all)))

    def _rows(self, Y) -> np.ndarray:
        y = np.asarray(Y)
        if y.ndim != 2 or y.shape[1] != self.d or y.shape[0] == 0:
            raise ValueError("rows must be ny x d")
        if y.min() < 0 or y.max() > 255:
            raise ValueError("codes must lie in 1..attrisize[j]")
        return np.ascontiguousarray(y, dtype=np.uint8)

    def density(self, Y) -> np.ndarray:
        """lpd[y]: the log posterior predictive density of each row of ``Y``."""
        return self._new(Y, None, True, False)[0]

    def _new(self, Y, cl, want_lpd, want_pnew, Ka=None, call="hdpm_predict_new"):
        y = self._rows(Y)
        eng = self.trace.eng
        lpd = np.zeros(y.shape[0]) if want_lpd else None
        pn = np.zeros(y.shape[0]) if want_pnew else None
        co, c = None, None
        if cl is not None and Ka is not None:
            c = np.ascontiguousarray(cl, dtype=np.int32).ravel()
            if c.size != self.N:
                raise ValueError("the partition must have N labels")
        elif cl is not None:
            c = self.trace._one(cl)[0]
            Ka = int(c.max()) + 1
        if cl is not None:
            co = np.zeros((y.shape[0], max(int(Ka), 0)))
        eng._check(getattr(eng._L, call)(eng._h, ptr(y), y.shape[0], ptr(c), int(Ka or 0), ptr(lpd), ptr(pn), ptr(co)))
        return lpd, pn, co

    def classify(self, Y, cl, Ka: int | None = None):
        """(class, coclass, p_new) of each row of ``Y`` against the partition ``cl`` of the
        training points (relabelled 0..Ka-1 in order of the labels' values, as the trace's
        candidates are; with ``Ka`` given, taken as labels 0..Ka-1 as they stand, so a class
        may be empty: its column is 0): coclass[y][a] is the mean over the points i of class a of the
        posterior probability that y is clustered with i, class its arg-max, and p_new[y] the
        posterior probability that y opens a cluster of its own."""
        _, pn, co = self._new(Y, cl, False, True, Ka)
        return np.argmax(co, axis=1), co, pn

    def partial(self, Y, cl=None, Ka: int | None = None):
        """(lpd, p_new, coclass | None) of rows in which code 0 marks a missing attribute:
        ``density`` and ``classify``'s numbers from the observed attributes alone (the missing
        ones are summed out exactly: they drop out of every sum).  A row without a 0 gets the
        bytes of ``density`` / ``classify``; ``cl`` and ``Ka`` as in ``classify``."""
        return self._new(Y, cl, True, True, Ka, call="hdpm_predict_partial")

    def impute(self, Y, ld: int | None = None):
        """(rows, attrs, pmf, mode, lpd): the posterior law of every missing code (0) of ``Y``
        given the observed codes of its row.  Entry e is (rows[e], attrs[e]), in row-major
        order; pmf[e, l - 1] = p(y_j = l | observed, data) for l = 1..m_j and 0.0 beyond
        (``ld`` slots, by default the largest m_j among the missing attributes); mode[e] is the
        first arg-max level, 1-based; lpd[y] is ``partial``'s.  The pmfs of several gaps of one
        row are marginals, not their joint law."""
        y = self._rows(Y)
        eng = self.trace.eng
        rows, attrs = np.nonzero(y == 0)
        if ld is None:
            ld = int(self.att[attrs].max()) if rows.size else 0
        pmf, lpd = np.zeros((rows.size, int(ld))), np.zeros(y.shape[0])
        eng._check(eng._L.hdpm_predict_impute(eng._h, ptr(y), y.shape[0], int(rows.size), int(ld),
                                              ptr(pmf) if rows.size else None, ptr(lpd)))
        mode = np.argmax(pmf, axis=1) + 1 if rows.size and ld else np.zeros(rows.size, np.int64)
        return rows, attrs, pmf, mode, lpd

    def profile(self, cl, Ka: int | None = None, ld: int | None = None, trace: bool = False) -> dict:
        """What each class of the partition ``cl`` is (csrc/profile.hip; ``cl`` and ``Ka`` as in
        ``classify``): per class a and attribute j, the posterior law of the center code and the
        sigma of the members of a.  A member i takes its draw's parameters, those of its cluster
        z_s(i), so the averages over members and draws need no matching of labels between draws.
        ``ld`` is the number of level slots (default the largest attrisize).  Keys:

        "center_cnt" (Ka x d x ld uint64, exact) and "center_pmf" = center_cnt / (M n_a): the
        posterior probability that the center of a member of a has code l at attribute j;
        "mode" (Ka x d: the first arg-max level, 1-based, 0 for an empty class) and "mode_prob";
        "code_pmf" (Ka x d x ld): the model's predictive law of a member's code, to hold against
        the class's observed code frequencies; "sigma_mean" and "sigma_sd" (Ka x d): the mean and
        the standard deviation (ddof 1; 0 when M = 1) over the draws of the members' mean sigma;
        "sigma_trace" (M x Ka x d, only with ``trace``): that mean per draw, the relabelled
        parameter trace for quantiles, trace plots and ``ess``; "sizes" (Ka).  An empty class
        has 0 everywhere."""
        eng = self.trace.eng
        if Ka is None:
            c = self.trace._one(cl)[0]
            Ka = int(c.max()) + 1
        else:
            c = np.ascontiguousarray(cl, dtype=np.int32).ravel()
            if c.size != self.N:
                raise ValueError("the partition must have N labels")
        Ka = int(Ka)
        ld = int(self.att.max()) if ld is None else int(ld)
        shape = (max(Ka, 0), self.d, max(ld, 0))
        cnt, pmf = np.zeros(shape, np.uint64), np.zeros(shape)
        mean, var = np.zeros(shape[:2]), np.zeros(shape[:2])
        tr = np.zeros((self.M,) + shape[:2]) if trace else None
        eng._check(eng._L.hdpm_predict_profile(eng._h, ptr(c), Ka, ld, ptr(cnt), ptr(pmf), ptr(mean), ptr(var),
                                               ptr(tr)))
        sizes = np.bincount(c, minlength=Ka).astype(np.int64)
        den = (self.M * sizes).astype(np.float64)[:, None, None]
        cpmf = np.zeros(shape)
        np.divide(cnt, den, out=cpmf, where=den > 0)
        mode = np.where(sizes[:, None] > 0, np.argmax(cnt, axis=2) + 1, 0)
        out = {"center_cnt": cnt, "center_pmf": cpmf, "mode": mode, "mode_prob": cpmf.max(axis=2), "code_pmf": pmf,
               "sigma_mean": mean, "sigma_sd": np.sqrt(var), "sizes": sizes}
        if trace:
            out["sigma_trace"] = tr
        return out

    def pointwise(self, X):
        """(lppd, var, logcpo) of the N training rows ``X`` (the rows the chain ran on): per
        row the log mean likelihood under its own cluster over the draws, the sample variance
        of that log-likelihood, and the log conditional predictive ordinate."""
        x = self._rows(X)
        if x.shape[0] != self.N:
            raise ValueError("pointwise needs the N training rows")
        eng = self.trace.eng
        lppd, var, cpo = np.zeros(self.N), np.zeros(self.N), np.zeros(self.N)
        eng._check(eng._L.hdpm_predict_own(eng._h, ptr(x), ptr(lppd), ptr(var), ptr(cpo)))
        return lppd, var, cpo

    def loglik(self, s: int, Y):
        """(ll, resp) of draw ``s`` alone: ll[y][k] the log-density of row y under cluster k
        (ny x K_s) and resp[y] the urn's probabilities, slot 0 the new cluster (ny x (K_s + 1));
        testing and inspection."""
        y = self._rows(Y)
        eng = self.trace.eng
        K = int(self.K[s]) if 0 <= int(s) < self.M else 1
        ll, resp = np.zeros((y.shape[0], K)), np.zeros((y.shape[0], K + 1))
        eng._check(eng._L.hdpm_predict_loglik(eng._h, int(s), ptr(y), y.shape[0], ptr(ll), ptr(resp)))
        return ll, resp


def waic(pointwise) -> float:
    """WAIC = -2 sum_i (lppd[i] - var[i]) of ``Predictive.pointwise``'s result, the sum exact
    (``math.fsum``)."""
    lppd, var, _ = pointwise
    return -2.0 * math.fsum(float(a) - float(b) for a, b in zip(lppd, var))


def lpml(pointwise) -> float:
    """LPML = sum_i logcpo[i] of ``Predictive.pointwise``'s result (``math.fsum``)."""
    return math.fsum(float(x) for x in pointwise[2])


def _avg_cuts(trace, max_k, max_groups):
    if not isinstance(trace, LabelTrace):
        raise ValueError("the matrix-free average-linkage search needs a LabelTrace")
    U = trace.groups(max_groups)["U"] if max_groups is not None else trace.groups()["U"]
    trace.avg_tree()
    kmax = max_k if max_k is not None else math.ceil(trace.N / 8)
    if kmax < 1:
        raise ValueError("max_k must be at least 1")
    # cuts into more than U clusters split groups of identical points and never win; the
    # trace tables hold at most 255 clusters
    return min(int(kmax), U, 255)


def minvi_avg(trace: LabelTrace, max_k: int | None = None, loss: str = "VI.lb", max_groups: int | None = None):
    """mcclust.ext::minVI(method = "avg") from a ``LabelTrace``, with no N x N matrix: the
    cuts k = 1..max_k (default ceiling(N / 8); at most min(U, 255)) of the average-linkage
    tree of 1 - psm, built on the U groups of identical label columns.  ``loss`` as in
    ``minvi``.  Returns (cl, value) with cl 1-based."""
    if loss not in ("VI.lb", "VI"):
        raise ValueError(f"unknown loss {loss!r}")
    kmax = _avg_cuts(trace, max_k, max_groups)
    lb, v, _, _ = trace.cut_losses(1, kmax)
    vals = v if loss == "VI" else lb
    best = int(np.argmin(vals))
    return trace.cut(best + 1) + 1, float(vals[best])


def minbinder_avg(trace: LabelTrace, max_k: int | None = None, max_groups: int | None = None):
    """mcclust::minbinder(method = "avgl") from a ``LabelTrace``: the cut of the same tree
    minimising Binder's loss, the argmin taken on the exact integers M A + P - 2 Q.  Returns
    (cl, value) with cl 1-based and the value of ``LabelTrace.binder``."""
    kmax = _avg_cuts(trace, max_k, max_groups)
    _, _, A, Q = trace.cut_losses(1, kmax)
    c, p = np.zeros((1, trace.N), np.int32), np.zeros(1, np.uint64)      # P alone: no table pass
    trace.eng._check(trace.eng._L.hdpm_trace_losses(trace.eng._h, ptr(c), 1, None, None, None, ptr(p)))
    P = int(p[0])
    A, Q = [int(x) for x in A], [int(x) for x in Q]
    num = [trace.M * a + P - 2 * q for a, q in zip(A, Q)]
    best = min(range(len(num)), key=num.__getitem__)
    return trace.cut(best + 1) + 1, float(A[best] + (P - 2 * Q[best]) / trace.M)


def _loss_code(loss: str) -> int:
    if loss not in ("VI", "Binder"):
        raise ValueError(f"unknown loss {loss!r}")
    return 0 if loss == "VI" else 1       # HDPM_LOSS_VI, HDPM_LOSS_BINDER


def coarsen(cl, merge, k: int) -> np.ndarray:
    """The labels of ``cl`` (as ``LabelTrace.merge_path`` took them) after the first K0 - k
    merges of ``merge``, K0 the classes of ``cl``: the path's level of k classes, relabelled
    0..k-1 by first appearance.  Host numpy."""
    c = np.asarray(cl).ravel().copy()
    K0 = np.unique(c).size
    steps = K0 - int(k)
    merge = np.asarray(merge).reshape(-1, 2)
    if steps < 0 or steps > merge.shape[0]:
        raise ValueError("k must lie between K0 - len(merge) and K0")
    for a, b in merge[:steps]:
        c[c == b] = a
    u, first, inv = np.unique(c, return_index=True, return_inverse=True)
    rank = np.empty(u.size, np.int64)
    rank[np.argsort(first)] = np.arange(u.size)
    return rank[inv]


def refine(trace: LabelTrace, cl, loss: str = "VI", max_rounds: int = 100, merges: int = 0) -> dict:
    """A point estimate improved by single-point moves (the local search of mcclust.ext's
    ``greedy`` and of SALSO, without their splits and restarts; with ``merges`` > 0, with up
    to that many merges of two classes), with no N x N
    matrix and no limit on the number of distinct label columns.  Each round takes every
    point's best move from ``LabelTrace.move_gains``, at most one new class among them, and
    applies the moves together, halving their number until the loss itself (``vi``, or
    Binder's exact integer) falls strictly; include/hdpm.h states the rule.  It ends at a
    partition that no single move improves (``converged``) or after ``max_rounds`` rounds.

    Single moves stall where the draws leave open whether two classes are one.  With
    ``merges`` > 0 the descent alternates with merges: at its end the pair of classes whose
    merge lowers the loss most (``LabelTrace.merge_gains``) is merged if the evaluated loss
    falls strictly, and the descent resumes; the run ends at a partition that neither a single
    move nor a merge of two classes improves, or after ``merges`` merges with one still to be
    had (``converged`` False).

    Returns {"cl" (1-based, labelled by first appearance), "value", "start", "rounds",
    "trials", "moved", "converged", "history"}, and "merges" (the accepted merges) if ``merges``
    > 0: history holds the loss at the start and after each accepted round or merge.  For
    "Binder" value and start are ``LabelTrace.binder``'s values, which
    history begins and ends with; between them it holds the integers M A + P - 2 Q divided by
    M (the same numbers, rounded once instead of twice).  All are combined as Python ints."""
    if not isinstance(trace, LabelTrace):
        raise ValueError("refine needs a LabelTrace")
    code = _loss_code(loss)
    if max_rounds < 0:
        raise ValueError("max_rounds must be at least 0")
    if merges < 0:
        raise ValueError("merges must be at least 0")
    c = trace._one(cl)[0]
    out = np.zeros(trace.N, np.int32)
    info = _lib.RefineInfo()
    hist = np.zeros(int(max_rounds) + int(merges) + 1)
    eng = trace.eng
    nm = C.c_int32(0)
    if merges:
        eng._check(eng._L.hdpm_trace_refine_merge(eng._h, ptr(c), code, int(max_rounds), int(merges), ptr(out),
                                                  C.byref(info), C.byref(nm), ptr(hist)))
    else:
        eng._check(eng._L.hdpm_trace_refine(eng._h, ptr(c), code, int(max_rounds), ptr(out), C.byref(info),
                                            ptr(hist)))
    hist = hist[:info.rounds + nm.value + 1]
    start, value = float(info.start), float(info.value)
    if loss == "Binder":
        # the value of LabelTrace.binder, A + (P - 2 Q) / M, with P - 2 Q = (M A + P - 2 Q) - M A
        def binder(num, labels):
            n = np.bincount(labels).tolist()
            A = sum(x * (x - 1) // 2 for x in n)
            return float(A + (int(num) - trace.M * A) / trace.M)
        start, value = binder(info.start, c), binder(info.value, out)
        hist = np.array([int(x) / trace.M for x in hist])
        hist[0], hist[-1] = start, value if hist.size > 1 else start
    r = {"cl": out + 1, "value": value, "start": start, "rounds": int(info.rounds), "trials": int(info.trials),
         "moved": int(info.moved), "converged": bool(info.converged), "history": hist}
    if merges:
        r["merges"] = int(nm.value)
    return r


def comp_psm(c_trace, device: int = 0) -> np.ndarray:
    """mcclust::comp.psm: the full N x N matrix (moderate N)."""
    p = PSM(c_trace, device=device)
    try:
        return p.matrix()
    finally:
        p.close()


def minvi(psm, cls_draw=None, method: str = "avg", max_k: int | None = None, loss: str = "VI.lb"):
    """mcclust.ext::minVI for the methods "avg" (cuts of the average-linkage tree of
    1 - psm, k = 1..max_k, default ceiling(N / 8); the tree on the host, needs the full
    matrix) and "draws" (the saved partitions).  Returns (cl, value) with cl 1-based.

    ``psm`` is a ``PSM`` or, for "draws", a ``LabelTrace`` (no matrix: "avg" raises
    ValueError; ``minvi_avg`` is the same search from a ``LabelTrace``).  ``loss`` is "VI.lb" (the lower bound minVI minimises) or "VI" (the
    posterior expected VI itself, mcclust.ext VI(cls, cls.draw); needs a ``LabelTrace``)."""
    if loss not in ("VI.lb", "VI"):
        raise ValueError(f"unknown loss {loss!r}")
    trace = isinstance(psm, LabelTrace)
    if loss == "VI" and not trace:
        raise ValueError("loss 'VI' needs a LabelTrace")
    if trace and method == "avg":
        raise ValueError("method 'avg' needs the matrix: use a PSM")
    if method == "draws":
        if cls_draw is None:
            raise ValueError("method 'draws' needs cls_draw")
        cand = np.atleast_2d(np.asarray(cls_draw))
    elif method == "avg":
        from scipy.cluster.hierarchy import cut_tree, linkage
        from scipy.spatial.distance import squareform
        m = psm.matrix()
        dist = 1.0 - m
        np.fill_diagonal(dist, 0.0)
        Z = linkage(squareform(dist, checks=False), method="average")
        kmax = max_k if max_k is not None else math.ceil(psm.N / 8)
        cand = cut_tree(Z, n_clusters=list(range(1, kmax + 1))).T
    else:
        raise ValueError(f"unknown method {method!r}")
    vals = psm.vi(cand) if loss == "VI" else psm.vi_lb(cand)
    best = int(np.argmin(vals))
    cl = np.unique(cand[best], return_inverse=True)[1] + 1
    return cl, float(vals[best])


def minbinder(trace: LabelTrace, cls_draw=None, method: str = "draws"):
    """mcclust::minbinder for the method "draws": the saved partition minimising Binder's
    loss sum_{i<j} |1(c_i = c_j) - psm_ij|, from a ``LabelTrace``.  Returns (cl, value) with
    cl 1-based.  The argmin is chosen on exact integers (M A + P - 2 Q); the value is
    ``LabelTrace.binder``'s.  mcclust is absent here, so its scaling of the reported value
    is unpinned, as minVI's tie conventions are; the argmin does not depend on it."""
    if not isinstance(trace, LabelTrace):
        raise ValueError("minbinder needs a LabelTrace")
    if method != "draws":
        raise ValueError(f"unknown method {method!r}: only 'draws' runs without the matrix")
    if cls_draw is None:
        raise ValueError("method 'draws' needs cls_draw")
    cand = np.atleast_2d(np.asarray(cls_draw))
    A, P, Q = trace.binder_terms(cand)
    num = [trace.M * a + P - 2 * q for a, q in zip(A, Q)]
    best = min(range(len(num)), key=num.__getitem__)
    cl = np.unique(cand[best], return_inverse=True)[1] + 1
    return cl, float(A[best] + (P - 2 * Q[best]) / trace.M)


def _ball(d, k, alpha: float) -> dict:
    """The selection of mcclust.ext::credibleball on the host: ``d`` the M distances of the
    draws to the estimate (integers or floats), ``k`` their cluster counts.  With r the
    ceil((1 - alpha) M)-th smallest distance (the index clamped to 1..M), the ball is every
    draw with d <= r; every tie is kept, in the ball and in each bound.  Returns draw indices
    (ascending) and the distances of the bounds."""
    d, k = np.asarray(d), np.asarray(k)
    if d.ndim != 1 or d.size == 0 or k.shape != d.shape:
        raise ValueError("d and k must be vectors of the same length M >= 1")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError("alpha must lie in [0, 1]")
    M = d.size
    idx = min(max(math.ceil((1 - alpha) * M), 1), M)
    r = np.sort(d)[idx - 1]
    ball = np.flatnonzero(d <= r)

    def farthest(sel):
        far = d[sel].max()
        return sel[d[sel] == far], far.item()

    horizontal, dh = farthest(ball)
    upper, du = farthest(ball[k[ball] == k[ball].min()])      # the fewest clusters
    lower, dl = farthest(ball[k[ball] == k[ball].max()])      # the most clusters
    return {"ball": ball, "horizontal": horizontal, "upper_vertical": upper, "lower_vertical": lower,
            "radius": r.item(), "horizontal_distance": dh, "upper_vertical_distance": du,
            "lower_vertical_distance": dl}


def credible_ball(trace: LabelTrace, cl, dist: str = "VI", alpha: float = 0.05) -> dict:
    """mcclust.ext::credibleball(c.star, cls.draw, c.dist, alpha) from a ``LabelTrace``: the
    smallest ball around the estimate ``cl``, in the VI or Binder distance (``dist`` "VI" or
    "Binder"; the latter as the count of disagreeing pairs), that holds a share 1 - alpha of
    the saved draws, and its three bounds.  With d the M distances of ``LabelTrace.distances``
    and r the ceil((1 - alpha) M)-th smallest, the ball is the draws with d <= r; the
    horizontal bound is the ball's draws at the largest distance, the upper vertical bound
    those at the largest distance among the ball's draws with the fewest clusters, the lower
    vertical bound the same among those with the most clusters.  All ties are returned.

    The result holds draw indices (the caller keeps the draws): "ball", "horizontal",
    "upper_vertical", "lower_vertical"; and "radius", "horizontal_distance",
    "upper_vertical_distance", "lower_vertical_distance" and "distances" (the M values).
    R is absent here, so parity with the package (its handling of ties at the radius
    included) is unpinned, as minVI's is."""
    if not isinstance(trace, LabelTrace):
        raise ValueError("credible_ball needs a LabelTrace")
    if dist not in ("VI", "Binder"):
        raise ValueError(f"unknown distance {dist!r}")
    c = trace._one(cl)
    vi, binder, k = trace.distances(c)
    d = vi[0] if dist == "VI" else binder[0]
    out = _ball(d, k, alpha)
    out["distances"] = d
    return out


def arandi(cl1, cl2, adjust: bool = True) -> float:
    """mcclust::arandi (Hubert & Arabie's adjusted Rand index)."""
    a, b = np.asarray(cl1), np.asarray(cl2)
    if a.shape != b.shape:
        raise ValueError("cl1 and cl2 must have same length")
    _, ia = np.unique(a, return_inverse=True)
    _, ib = np.unique(b, return_inverse=True)
    tab = np.zeros((ia.max() + 1, ib.max() + 1), np.int64)
    np.add.at(tab, (ia, ib), 1)

    def ch2(x):
        x = np.asarray(x, np.float64)
        return x * (x - 1) / 2

    n = a.size
    t1, t2 = tab.sum(1), tab.sum(0)
    if adjust:
        correc = ch2(t1).sum() * ch2(t2).sum() / ch2(n)
        return float((ch2(tab).sum() - correc) / (0.5 * ch2(t1).sum() + 0.5 * ch2(t2).sum() - correc))
    return float(1 + ((tab.astype(np.float64) ** 2).sum() - 0.5 * (t1 ** 2).sum() - 0.5 * (t2 ** 2).sum()) / ch2(n))


def _ar_yw_spectrum0(x: np.ndarray) -> float:
    """R's ar(x, aic = TRUE) (Yule-Walker, ar.yw) and its spectral density at 0:
    var.pred / (1 - sum(ar))^2 (coda spectrum0.ar, used by LaplacesDemon::ESS)."""
    n = x.size
    xc = x - x.mean()
    order_max = min(n - 1, int(math.floor(10 * math.log10(n))))
    r = np.array([np.dot(xc[:n - k], xc[k:]) / n for k in range(order_max + 1)])
    # Levinson-Durbin (R's eureka): coefficients and prediction variances per order
    var = [r[0]]
    coefs = []
    a = np.zeros(0)
    v = r[0]
    for k in range(1, order_max + 1):
        if v <= 0:
            break
        kappa = (r[k] - np.dot(a, r[1:k][::-1])) / v
        a = np.concatenate([a - kappa * a[::-1], [kappa]])
        v = v * (1 - kappa * kappa)
        coefs.append(a.copy())
        var.append(v)
    var = np.array(var)
    aic = n * np.log(var) + 2 * np.arange(var.size) + 2
    order = int(np.argmin(aic))
    ar = coefs[order - 1] if order > 0 else np.zeros(0)
    vp = var[order] * n / (n - (order + 1))
    return float(vp / (1 - ar.sum()) ** 2)


def ess(x) -> np.ndarray:
    """LaplacesDemon::ESS (per column): n var(x) / spectrum0.ar(x), clamped to [1, n]
    (0 spectrum -> 0 -> 1)."""
    X = np.asarray(x, np.float64)
    if X.ndim == 1:
        X = X[:, None]
    n = X.shape[0]
    out = []
    for col in X.T:
        z = np.arange(1, n + 1, dtype=np.float64)
        resid = col - np.polyval(np.polyfit(z, col, 1), z)
        if np.isclose(resid.std(ddof=1), 0.0):
            out.append(1.0)
            continue
        spec = _ar_yw_spectrum0(col)
        e = n * col.var(ddof=1) / spec if spec != 0 else 0.0
        out.append(float(min(max(e, 1.0) if e > 0 else 1.0, n)))
    return np.array(out)


def iat(x) -> float:
    """LaplacesDemon::IAT: -1 + 2 sum of the autocorrelations up to the first non-positive
    one (Geyer's initial positive sequence on single lags), at most n / 2 lags."""
    dt = np.asarray(x, np.float64).ravel()
    n = dt.size
    mu, s2 = dt.mean(), dt.var(ddof=1)
    maxlag = max(3, n // 2)
    g1 = s2 * (n - 1) / n
    m = 1
    g2 = np.dot(dt[:n - m] - mu, dt[m:] - mu) / n
    t = g1 / s2
    while g2 > 0.0 and m < maxlag:
        m += 1
        g1 = g2
        g2 = np.dot(dt[:n - m] - mu, dt[m:] - mu) / n
        t += g1 / s2
    return float(-1 + 2 * t)
