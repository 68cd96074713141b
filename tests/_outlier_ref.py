"""fp64 numpy reference of pt_remove_outliers (include/pt_api.h), from GIVEN neighbour lists: scores, mean / stddev / threshold with
math.fsum (exactly rounded sums, so the reference's own error is a few ulps of the division and the square root), the mask, and the
radius filter's count.  No kernel of the library produces anything in here."""
import math

import numpy as np

NOIDX = 0xFFFFFFFF


def cap_lists(idx, d2, r):
    """the lists under reach r: every entry with d2 > r * r becomes (NOIDX, +inf) -- the rule of "max_dist" (R2 = r * r in double, inclusive)"""
    if r is None or math.isinf(r):
        return idx, d2
    out = d2 > r * r
    return np.where(out, np.uint32(NOIDX), idx).astype(np.uint32), np.where(out, np.inf, d2)


def scores(idx, d2):
    """s_i = (sum over the entries j >= 1 that name a point of sqrt(d2_j)) / (c - 1), c the number of entries that name a point;
    +inf when c <= 1.  Entry 0 is the point itself (or a lower-indexed duplicate) at d2 = 0."""
    valid = idx != NOIDX
    c = valid.sum(axis=1)
    dist = np.sqrt(np.where(valid, d2, 0.0))
    s = np.full(idx.shape[0], np.inf)
    for i in np.flatnonzero(c >= 2):
        s[i] = math.fsum(dist[i, 1:c[i]]) / (c[i] - 1)
    return s, c


def stats(s, alpha):
    """(n_f, mean, population stddev, threshold) over the finite scores; the stddev from a second pass, sum((s - mean)^2) / n_f"""
    f = s[np.isfinite(s)]
    if not f.size:
        return 0, 0.0, 0.0, 0.0
    mu = math.fsum(f) / f.size
    sd = math.sqrt(math.fsum((f - mu) ** 2) / f.size)
    return int(f.size), mu, sd, mu + alpha * sd


def statistical(idx, d2, alpha, max_dist=None):
    """(scores, keep, (n_f, mean, stddev, T)) of the statistical filter on the lists as given (their width is k), capped when max_dist is"""
    idx, d2 = cap_lists(idx, d2, max_dist)
    s, _ = scores(idx, d2)
    st = stats(s, alpha)
    return s, s <= st[3], st


def radius(idx, d2, r, max_dist=None):
    """(scores, keep) of the radius filter: the lists (width k = m + 1) under reach min(r, max_dist); score = c - 1, kept iff c == k"""
    reach = r if max_dist is None else min(r, max_dist)
    idx, _ = cap_lists(idx, d2, reach)
    c = (idx != NOIDX).sum(axis=1)
    return np.maximum(c - 1, 0).astype(np.float64), c == idx.shape[1]


def band(s, T, rel):
    """the points whose score lies within rel * T of the threshold: their side of it is not asserted"""
    return np.abs(s - T) <= rel * T
