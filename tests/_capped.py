"""Expectations under the max_dist cap (shared by the GPU suites): the oracle's uncapped lists truncated at d2 <= r*r, exact list
comparison, and the blend check that leaves rows without a neighbour as the caller's outputs held them."""
import numpy as np

TOL = 1e-5
NOIDX = 0xFFFFFFFF


def truncate(idx, d2, r):
    """the oracle's lists under the cap r: entries with d2 > r*r become (NOIDX, +inf)"""
    R2 = float(r) * float(r)
    idx = idx.copy(); d2 = d2.copy()
    far = d2 > R2
    idx[far] = NOIDX; d2[far] = np.inf
    return idx, d2


def check_exact(got, want, what):
    gi, gd = got
    wi, wd = want
    assert np.array_equal(gi, wi), "%s: indices differ in %d of %d rows" % (what, (gi != wi).any(axis=1).sum(), gi.shape[0])
    assert np.array_equal(gd, wd), "%s: d2 differ" % what


def check_blend(got_c, got_n, idx, d2, rgb, nrm, mode, sentinel_c, sentinel_n, oracle, what):
    """rows with an entry: the oracle's blend of the truncated lists within 1e-5; rows without: the caller's values, bit for bit"""
    empty = (idx == NOIDX).all(axis=1)
    rc, rn = oracle.blend(idx, d2, rgb, nrm, mode=mode)
    full = ~empty
    if full.any():
        assert np.abs(got_c[full] - rc[full]).max() / 255.0 <= TOL, what + ": colour"
        assert np.abs(got_n[full] - rn[full]).max() <= TOL, what + ": normal"
    assert np.array_equal(got_c[empty].view(np.uint32), sentinel_c[empty].view(np.uint32)), what + ": an empty row's colour was written"
    assert np.array_equal(got_n[empty].view(np.uint32), sentinel_n[empty].view(np.uint32)), what + ": an empty row's normal was written"
    return int(empty.sum())
