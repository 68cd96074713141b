"""A plain reference for the attribute stage (PCA normals, k-neighbour blend): numpy only, np.longdouble where sums are formed.

It shares no code and no algorithm with the kernels of csrc/pt_attr.hip or with oracle/pt_oracle.c: the covariance is centred on the
neighbours' mean (two passes, extended precision) and decomposed by LAPACK (np.linalg.eigh), where kernel and oracle both run the same
cyclic Jacobi sweep.  tests/test_attr_ref.py pins this file on the CPU (against the oracle and against closed forms) before
tests/test_gpu_attr_reference.py holds the kernels to it.
"""
import numpy as np

NOIDX = 0xFFFFFFFF
LD = np.longdouble
EPS64 = 2.0 ** -52


def _gather(idx, n):
    idx = np.asarray(idx, np.uint32)
    valid = (idx != NOIDX) & (idx < n)
    return np.where(valid, idx, 0).astype(np.int64), valid


def pca_ref(idx, xyz64, nrm=None):
    """idx (m, k) uint32, xyz64 planar (3, n) float64, nrm (n, 3) or None.  Returns (normal (m, 3) float64, eigvals (m, 3) ascending,
    ke (m,)): the eigenvector of the smallest eigenvalue of the covariance of the valid neighbours (id != NOIDX and id < n), oriented so
    that dot(normal, sum of the neighbours' stored normals) >= 0 -- normal_z >= 0 without stored normals -- and (0, 0, 1) for ke < 3."""
    xyz64 = np.asarray(xyz64, np.float64)
    assert xyz64.ndim == 2 and xyz64.shape[0] == 3
    n = xyz64.shape[1]
    ids, valid = _gather(idx, n)
    ke = valid.sum(axis=1)
    w = valid[:, :, None].astype(LD)
    P = xyz64.T.astype(LD)[ids] if n else np.zeros(ids.shape + (3,), LD)          # (m, k, 3)
    mu = (P * w).sum(axis=1, keepdims=True) / np.maximum(ke, 1).astype(LD)[:, None, None]
    D = (P - mu) * w
    cov = np.einsum("mka,mkb->mab", D, D).astype(np.float64)
    lam, vec = np.linalg.eigh(cov)
    normal = vec[:, :, 0].copy()
    if nrm is not None:
        s = (np.asarray(nrm).astype(LD)[ids] * w).sum(axis=1).astype(np.float64)
        ref = (normal * s).sum(axis=1)
    else:
        ref = normal[:, 2]
    normal[ref < 0] *= -1.0
    normal[ke < 3] = (0.0, 0.0, 1.0)
    return normal, lam, ke


def pca_bound(k, eigvals):
    """Allowed sine of the angle between a kernel's normal and pca_ref's: 2 (k+2)^2 2^-52 trace / (l1 - l0) + 2^-22.
    First term: Davis-Kahan, sin(theta) <= 2 |E| / gap, with |E| bounded by the fp64 rounding of a k-term uncentred moment sum, itself at
    most (k + 1) trace because the shift point is one of the neighbours.  Second term: the fp32 rounding of the three output components."""
    lam = np.asarray(eigvals, np.float64)
    gap = lam[..., 1] - lam[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        first = np.where(gap > 0, 2.0 * (k + 2) ** 2 * EPS64 * lam.sum(axis=-1) / gap, np.inf)
    return first + 2.0 ** -22


def comparable(eigvals):
    """rows whose normal is defined well enough to be compared: l1 - l0 > 1e-6 trace"""
    lam = np.asarray(eigvals, np.float64)
    return (lam[:, 1] - lam[:, 0]) > 1e-6 * lam.sum(axis=1)


def sign_decided(idx, n, want, nrm=None):
    """rows whose orientation is decided clearly enough to be checked: |dot(want, sum of normals)| > 1e-6 |sum of normals|, or
    |want_z| > 1e-6 without stored normals"""
    if nrm is None:
        return np.abs(want[:, 2]) > 1e-6
    ids, valid = _gather(idx, n)
    s = (np.asarray(nrm).astype(LD)[ids] * valid[:, :, None].astype(LD)).sum(axis=1).astype(np.float64)
    return np.abs((want * s).sum(axis=1)) > 1e-6 * np.linalg.norm(s, axis=1)


def sin_angle(a, b):
    """|a x b| for rows of unit vectors: the sine of the angle between the two LINES (blind to orientation)"""
    return np.linalg.norm(np.cross(np.asarray(a, np.float64), np.asarray(b, np.float64)), axis=1)


def check_pca(got, idx, xyz64, nrm, what, min_share=0.99, either_sign=False):
    """The whole comparison of section "PCA" of the suite: every row finite and of unit length within 1e-6; rows with ke < 3 exactly
    (0, 0, 1); every comparable row within pca_bound of pca_ref; the same half-space wherever the orientation is decided (either_sign:
    not checked).  Returns a dict of figures (printed by the callers before they assert nothing further)."""
    got = np.asarray(got)
    idx = np.asarray(idx, np.uint32)
    k = idx.shape[1]
    want, lam, ke = pca_ref(idx, xyz64, nrm)
    g64 = got.astype(np.float64)
    assert np.isfinite(g64).all(), what + ": non-finite normal"
    unit = np.abs(np.linalg.norm(g64, axis=1) - 1.0)
    assert unit.max(initial=0.0) <= 1e-6, "%s: |normal| off by %.3g" % (what, unit.max())
    few = ke < 3
    assert np.array_equal(got[few], np.tile(np.float32([0, 0, 1]), (int(few.sum()), 1))), what + ": a row with ke < 3 is not exactly (0, 0, 1)"
    full = ~few
    cmp_ = comparable(lam) & full
    share = cmp_[full].mean() if full.any() else 1.0
    s = sin_angle(g64, want)
    bound = pca_bound(k, lam)
    worst = (s[cmp_] / bound[cmp_]).max(initial=0.0)
    print("%s: k=%d rows=%d ke<3=%d compared=%.4f max sin/bound=%.3g max sin=%.3g" % (what, k, len(got), few.sum(), share, worst, s[cmp_].max(initial=0.0)))
    assert share >= min_share, "%s: only %.4f of the rows are comparable" % (what, share)
    bad = cmp_ & (s > bound)
    assert not bad.any(), "%s: %d rows outside the bound, worst sin %.3g against %.3g (row %d)" % (
        what, bad.sum(), s[bad].max(), bound[bad][np.argmax(s[bad])], np.flatnonzero(bad)[np.argmax(s[bad])])
    if not either_sign:
        sg = cmp_ & sign_decided(idx, np.asarray(xyz64).shape[1], want, nrm)
        flipped = sg & ((g64 * want).sum(axis=1) <= 0)
        assert not flipped.any(), "%s: %d rows point into the other half-space (first: row %d)" % (what, flipped.sum(), np.flatnonzero(flipped)[0])
    return dict(share=share, worst=worst, few=int(few.sum()), compared=int(cmp_.sum()))


def blend_ref(idx, d2, rgb, nrm, mode):
    """The k-neighbour blend as include/pt_api.h and oracle/pt_oracle.c define it, in np.longdouble: weights 1 (mode 0) or
    1 / (d2 + 1e-12) (mode 1) over the valid entries (id != NOIDX and id < n), normalised by their sum; the blended normal is divided by
    its length where that is >= 1e-12 and left as it is below.  Rows without a valid entry give zeros.  Returns (rgb (m, 3), nrm (m, 3))
    as float64, the values before any store to fp32."""
    rgb = np.asarray(rgb); nrm = np.asarray(nrm)
    n = rgb.shape[0]
    assert nrm.shape[0] == n
    ids, valid = _gather(idx, n)
    if mode == 1:
        w = LD(1.0) / (np.asarray(d2, np.float64).astype(LD) + LD(1e-12))
    else:
        w = np.ones(ids.shape, LD)
    w = np.where(valid, w, LD(0.0))
    wsum = w.sum(axis=1)
    has = valid.any(axis=1)
    wn = w / np.where(has, wsum, LD(1.0))[:, None]
    c = (wn[:, :, None] * rgb.astype(LD)[ids]).sum(axis=1)
    v = (wn[:, :, None] * nrm.astype(LD)[ids]).sum(axis=1)
    ln = np.sqrt((v * v).sum(axis=1))
    big = ln >= LD(1e-12)
    v = np.where(big[:, None], v / np.where(big, ln, LD(1.0))[:, None], v)
    c[~has] = 0; v[~has] = 0
    return c.astype(np.float64), v.astype(np.float64)
