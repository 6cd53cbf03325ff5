"""CPU-side predictions of what update_phi (cf:511-591) meets on a given state: numpy
restatements of the reference's decisions, used by the device update_phi tests to say -- from
the inputs alone, never from the device's status word -- whether an update can be committed by
the device (csrc/phi.hip) or must be handed back to the host, and with which status.

TEST INFRASTRUCTURE ONLY (imported by tests/test_gpu_phi_edges.py and tests/test_gpu_parity.py).

Per (cluster, attribute) item of an update, from the cluster's frequency table f over the m_j
levels, its size n and the item's current sigma (compute_prob_centers, cf:461-509, then Rcpp
sample's FixupProb):
  fixed   the center pick does not depend on the uniform: the largest normalised
          exp(-(n - f_l) / sigma) is >= 1.0 after the two normalisations (pr[0] >= 1.0 after
          revsort; a one-level attribute has nothing to pick)
  nc      #{l: m_j p_l > 0.1}; Rcpp sample() takes Walker's alias method iff nc > 200
and, for the center the oracle's update then drew (level c with f_c members sharing it), rhig's
branch test (hyperg.cpp:359) on (v + f_c, w + n - f_c, m_j):
  beta path iff qbeta(0.1, w' + 1, v' - 1) < (m - 1) / m and (m - 1) / m > 4 / 5 (integer 0),
  i.e. pbeta((m - 1) / m, w' + 1, v' - 1) > 0.1 with x > 0; else the bisection branch.
  margin = |pbeta - 0.1| where the test comes down to that comparison (inf otherwise)."""
import math

import numpy as np

# kernels.hpp PhiStatus
OK, WALKER, BISECT, AMBIG, WINDOW, SHORT, PROB, INACTIVE, CAP, NONDET, OFF = range(11)
AMBIG_MARGIN = 1e-6         # a branch test closer than this to its threshold is no prediction

_exp = np.frompyfunc(math.exp, 1, 1)          # libm's exp, the one the reference calls


def _seqsum(a):
    """Row sums in index order (the reference's running sums; numpy's sum is pairwise)."""
    return np.cumsum(a, axis=1)[:, -1]


def freq_tables(codes, attrisize, c, K):
    """Per attribute j the K x m_j table of level counts of each cluster, and the cluster sizes."""
    c = np.asarray(c, np.int64)
    n = np.bincount(c, minlength=K)[:K].astype(np.float64)
    F = []
    for j, m in enumerate(attrisize):
        t = np.zeros((K, int(m)), np.float64)
        np.add.at(t, (c, codes[:, j].astype(np.int64) - 1), 1.0)
        F.append(t)
    return F, n


def center_probs(F_j, n, sig_j):
    """FixupProb-normalised center probabilities of one attribute, K x m_j."""
    x = (-(n[:, None] - F_j)) / sig_j[:, None]
    x = x - x.max(axis=1, keepdims=True)
    e = _exp(x).astype(np.float64)
    p = e / _seqsum(e)[:, None]
    return p / _seqsum(p)[:, None]            # FixupProb: the sum over the positive entries


def item_predicates(codes, attrisize, c, K, sigma):
    """fixed (K x d bool), nc (K x d int), the frequency tables and the cluster sizes of the
    update of every cluster of the state (labels c, K clusters, current sigmas)."""
    F, n = freq_tables(codes, attrisize, c, K)
    d = len(attrisize)
    fixed = np.zeros((K, d), bool)
    nc = np.zeros((K, d), np.int64)
    for j, m in enumerate(attrisize):
        p = center_probs(F[j], n, np.asarray(sigma)[:K, j])
        fixed[:, j] = (int(m) == 1) | (p.max(axis=1) >= 1.0)
        nc[:, j] = (int(m) * p > 0.1).sum(axis=1)
    return fixed, nc, F, n


_branch_cache = {}


def rhig_branch(oracle, v, w, m):
    """(beta_path, margin) of rhig(1, v, w, m)'s branch test, from the oracle's pbeta."""
    key = (float(v), float(w), float(m))
    hit = _branch_cache.get(key)
    if hit is None:
        x = (m - 1.0) / m
        a, b = w + 1.0, v - 1.0
        if not x > 0 or math.isnan(a) or math.isnan(b) or a < 0 or b < 0 or b == 0:
            hit = (False, math.inf)
        elif a == 0:
            hit = (True, math.inf)
        else:
            pb = oracle.lib().orc_ffi_pbeta(x, a, b)
            hit = (pb > 0.1, abs(pb - 0.1))
            assert hit[0] == bool(oracle.lib().orc_ffi_qbeta01_lt(a, b, x))
        _branch_cache[key] = hit
    return hit


def picked_branches(oracle, attrisize, v, w, F, n, centers):
    """For the centers an update drew (K x d, 1-based levels): bisect (K x d bool: the sigma
    draw takes rhig's bisection branch) and near (K x d bool: margin < AMBIG_MARGIN)."""
    K, d = centers.shape
    bis = np.zeros((K, d), bool)
    near = np.zeros((K, d), bool)
    for j, m in enumerate(attrisize):
        fc = F[j][np.arange(K), centers[:, j].astype(np.int64) - 1]
        for k in range(K):
            beta, margin = rhig_branch(oracle, v[j] + fc[k], w[j] + n[k] - fc[k], float(m))
            bis[k, j] = not beta
            near[k, j] = margin < AMBIG_MARGIN
    return bis, near


def any_level_near(oracle, attrisize, v, w, F, n):
    """Some level of some item has a branch test within AMBIG_MARGIN of its threshold (the device
    may then answer kPhiAmbig whatever is picked): a superset of the pickable levels."""
    for j, m in enumerate(attrisize):
        for k in range(F[j].shape[0]):
            for f in np.unique(F[j][k]):
                if rhig_branch(oracle, v[j] + f, w[j] + n[k] - f, float(m))[1] < AMBIG_MARGIN:
                    return True
    return False


def stream_distance(oracle, before, after, limit):
    """Uniforms drawn between two states of R's Mersenne-Twister (oracle rng states), < limit."""
    u = oracle.runif(np.array(before, copy=True), limit + 4)
    nxt = oracle.runif(np.array(after, copy=True), 4)
    hits = np.flatnonzero(u[:limit] == nxt[0])
    hits = [int(h) for h in hits if np.array_equal(u[h:h + 4], nxt)]
    assert len(hits) == 1, hits
    return hits[0]


# The device's drift-window model (csrc/kernels.hpp phi_lo / phi_hi, csrc/engine.cpp phi_plan): a
# sigma draw takes 2 uniforms per rbeta attempt, an attempt is rejected with probability p (0.12
# before the engine has seen an update), so the extra uniforms per draw have mean 2 p / (1 - p)
# and standard deviation 2 sqrt(p) / (1 - p); the windows span 4.75 (fast path) to 7 of them.
P_REJ0 = 0.12
DRIFT_RATE = 2 * P_REJ0 / (1 - P_REJ0)
DRIFT_SD = 2 * math.sqrt(P_REJ0) / (1 - P_REJ0)
Z_INSIDE = 3.0              # an end drift within 3 sd of the model's mean is inside every window


class UpdatePrediction:
    """What one update_phi of every cluster meets, from the state before it (labels, sigmas)
    and, for the branch tests, the centers the oracle's update drew."""

    def __init__(self, oracle, ds, c, K, sigma_before, centers_after, consumed=None):
        self.fixed, self.nc, F, n = item_predicates(ds.codes, ds.attrisize, c, K, sigma_before)
        self.bis, self.near = picked_branches(oracle, ds.attrisize, ds.v, ds.w, F, n, np.asarray(centers_after)[:K])
        self.items = K * ds.d
        self.min_count = int(n.min())
        self.all_fixed = bool(self.fixed.all())
        self.walker = bool((self.nc > 200).any())
        self.bisect = bool((self.bis & ~self.near).any())      # a clear bisection item
        self.n_near = int(self.near.sum())
        # the update's drift against the window model: a center draw takes 1 uniform, a sigma draw
        # 2 + its extra uniforms (the bisection branch: 1, no extras).  z: the end drift's distance
        # from the model's mean in model standard deviations.  Beyond Z_INSIDE the drift may have
        # left the device's windows (kPhiWindow / kPhiShort: the update goes to the host), and the
        # test then claims neither outcome.
        self.z = None
        if consumed is not None:
            nb = int(self.bis.sum())
            draws = self.items - nb
            drift = consumed - 3 * draws - 2 * nb
            self.z = (drift - DRIFT_RATE * draws) / (DRIFT_SD * math.sqrt(max(draws, 1)))
        self.may_leave_window = self.z is not None and abs(self.z) > Z_INSIDE
        self._amb_args = (oracle, ds.attrisize, ds.v, ds.w, F, n)
        self._amb = None

    @property
    def ambiguous(self):
        if self._amb is None:
            self._amb = any_level_near(*self._amb_args)
        return self._amb

    @property
    def handed_back(self):
        """The device cannot commit this update (Walker table or bisection branch)."""
        return self.walker or self.bisect

    def allowed_mask(self):
        """Status bits a hand-back of this update may show (atomicMax keeps the largest)."""
        m = 0
        if self.walker:
            m |= 1 << WALKER
        if self.bis.any():
            m |= 1 << BISECT
        if not self.all_fixed:
            m |= 1 << NONDET           # a speculated update dropped for its uniform-dependent picks
        if self.ambiguous:
            m |= 1 << AMBIG
        if self.may_leave_window:
            m |= 1 << WINDOW | 1 << SHORT
        return m
