"""CPU suite of the outlier-removal reference (tests/_outlier_ref.py) and of the inputs the GPU suite uses (tests/_outlier_cases.py):
the reference against answers worked out by hand, the radius count against a direct O(n^2) count, and the band condition -- on every
case of the GPU matrix no score lies within 1e-9 T of the threshold, so the GPU suite leaves no point out of its mask comparison."""
import math

import numpy as np
import pytest

import _outlier_cases as OC
import _outlier_ref as R

NOIDX = R.NOIDX
INF = np.inf


def test_five_collinear_points_by_hand():
    """points at x = 0, 1, 2, 4, 8, k = 3; ties at equal d2 go to the lower index"""
    idx = np.array([[0, 1, 2], [1, 0, 2], [2, 1, 0], [3, 2, 1], [4, 3, 2]], np.uint32)
    d2 = np.array([[0, 1, 4], [0, 1, 1], [0, 1, 4], [0, 4, 9], [0, 16, 36]], np.float64)
    s, c = R.scores(idx, d2)
    assert c.tolist() == [3, 3, 3, 3, 3]
    assert s.tolist() == [1.5, 1.0, 1.5, 2.5, 5.0]
    nf, mu, sd, T = R.stats(s, 1.0)
    assert nf == 5 and mu == 11.5 / 5
    # deviations -0.8 -1.3 -0.8 0.2 2.7 -> squares 0.64 1.69 0.64 0.04 7.29, sum 10.3, variance 2.06
    assert abs(sd - math.sqrt(2.06)) <= 4e-16 and abs(T - (2.3 + math.sqrt(2.06))) <= 8e-16
    _, keep, st = R.statistical(idx, d2, 1.0)
    assert keep.tolist() == [True, True, True, True, False] and st == (nf, mu, sd, T)
    _, keep2, st2 = R.statistical(idx, d2, 2.0)                   # T = 2.3 + 2 * 1.435 = 5.17: nobody leaves
    assert keep2.all() and abs(st2[3] - (2.3 + 2 * math.sqrt(2.06))) <= 8e-16
    # the oracle's own lists for these points are the ones written out above
    from oracle import oracle as O
    x = np.array([[0.0, 1.0, 2.0, 4.0, 8.0], [0.0] * 5, [0.0] * 5])
    oi, od = O.knn_bruteforce(x, x, 3)
    assert np.array_equal(oi, idx) and np.array_equal(od, d2)


def test_capped_rows():
    """c = 1 (the point alone under the cap) scores +inf and is left out of mean and stddev; c = 2 divides by 1; an empty row is +inf too"""
    idx = np.array([[0, 1, 2], [1, 0, 2], [2, 1, 0], [3, 2, 1]], np.uint32)
    d2 = np.array([[0, 1, 4], [0, 1, 1], [0, 1, 4], [0, 100, 121]], np.float64)
    ci, cd = R.cap_lists(idx, d2, 2.0)                           # reach 2: d2 <= 4 stays (inclusive), row 3 keeps itself only
    assert ci.tolist() == [[0, 1, 2], [1, 0, 2], [2, 1, 0], [3, NOIDX, NOIDX]] and cd[3].tolist() == [0, INF, INF]
    s, keep, (nf, mu, sd, T) = R.statistical(idx, d2, 0.0, max_dist=2.0)
    assert s.tolist() == [1.5, 1.0, 1.5, INF] and nf == 3 and mu == 4.0 / 3
    assert abs(sd - math.sqrt((2 * (1.5 - 4 / 3) ** 2 + (1 - 4 / 3) ** 2) / 3)) <= 4e-16 and T == mu
    assert keep.tolist() == [False, True, False, False]           # alpha = 0: above the mean leaves, and +inf always does
    s1, _ = R.scores(*R.cap_lists(idx, d2, 1.0))                 # reach 1: rows 0 and 2 keep one neighbour
    assert s1.tolist() == [1.0, 1.0, 1.0, INF]
    s0, c0 = R.scores(np.full((1, 3), NOIDX, np.uint32), np.full((1, 3), INF))
    assert s0.tolist() == [INF] and c0.tolist() == [0]
    assert R.stats(np.array([INF, INF]), 2.0) == (0, 0.0, 0.0, 0.0)
    sc, kp = R.radius(idx, d2, 2.0)
    assert sc.tolist() == [2, 2, 2, 0] and kp.tolist() == [True, True, True, False]
    sc, kp = R.radius(idx, d2, 2.0, max_dist=1.0)                # reach min(r, max_dist)
    assert sc.tolist() == [1, 2, 1, 0] and kp.tolist() == [False, True, False, False]


@pytest.mark.parametrize("m", [1, 8, 31])
def test_radius_count_against_direct_count(oracle, m):
    """2 000 points: kept iff at least m OTHER points lie within r (d2 <= r * r with the library's metric, summed (x + y) + z)"""
    rng = np.random.default_rng(40)
    x = rng.random((3, 2000))
    x[:, :50] = rng.random((3, 50)) * 3 - 1
    r = {1: 0.07, 8: 0.11, 31: 0.2}[m]                            # (about 3, 11 and 67 points expected within r inside the cube)
    d = x[:, :, None] - x[:, None, :]
    dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    others = (dd <= r * r).sum(axis=1) - 1
    idx, d2 = oracle.knn_bruteforce(x, x, m + 1)
    sc, keep = R.radius(idx, d2, r)
    assert np.array_equal(keep, others >= m)
    assert np.array_equal(sc, np.minimum(others, m).astype(np.float64))
    assert 0 < keep.sum() < 2000


@pytest.mark.parametrize("dtype", OC.DTYPES)
@pytest.mark.parametrize("name", OC.NAMES)
def test_band_condition(name, dtype):
    """For every (k, alpha) the GPU suite asserts a mask for -- and alpha = 1 at every k besides -- no score lies within 1e-9 T of T, the
    filter removes between 456 and 497 points, and nearly all of them are injected ones."""
    stray = OC.cloud(name, dtype)[3]
    for k in OC.KS:
        for alpha in (1.0, 2.0):
            idx, d2 = OC.self_lists(name, dtype, k)
            s, keep, (nf, mu, sd, T) = R.statistical(idx, d2, alpha)
            nb = int(R.band(s, T, OC.BAND).sum())
            removed = np.flatnonzero(~keep)
            hit = int(np.isin(removed, stray).sum())
            print("%s %s k=%d alpha=%g: T %.6g, band %d, removed %d, injected among them %d" % (name, dtype, k, alpha, T, nb, removed.size, hit))
            assert nf == OC.N and np.isfinite(s).all()
            assert nb == 0 and nb <= OC.N // 1000
            assert 456 <= removed.size <= 497 and hit >= removed.size - 10


@pytest.mark.parametrize("dtype", OC.DTYPES)
@pytest.mark.parametrize("name", OC.NAMES)
def test_capped_and_radius_inputs(name, dtype):
    """what the GPU suite's capped and radius cases rely on: the cap isolates hundreds of injected points (and nobody else), the band
    around the capped threshold is empty, and every radius case keeps some points and removes some"""
    stray = OC.cloud(name, dtype)[3]
    idx, d2 = OC.self_lists(name, dtype, 16)
    s, keep, (nf, mu, sd, T) = R.statistical(idx, d2, 2.0, OC.CAP)
    alone = np.flatnonzero(np.isinf(s))
    assert 400 <= alone.size <= OC.N_STRAY and np.isin(alone, stray).all() and nf == OC.N - alone.size
    assert not R.band(s, T, OC.BAND).any() and not keep[alone].any()
    r = OC.radius_for(name, dtype)
    for m in (1, 8, 31):
        _, kp = R.radius(*OC.self_lists(name, dtype, m + 1), r)
        assert 0 < kp.sum() < OC.N
