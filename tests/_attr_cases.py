"""Inputs of the attribute reference tests, shared by tests/test_attr_ref.py (CPU: reference against oracle) and
tests/test_gpu_attr_reference.py (GPU: kernels against reference), so that both read the same clouds and the same lists."""
import functools

import numpy as np

NOIDX = 0xFFFFFFFF
N = 50000
M = 2000
KS = (1, 2, 3, 5, 8, 13, 16, 20, 31, 32)
DTYPES = {"f32": np.float32, "f64": np.float64, "f16": np.float16}
FAR = np.array([[1e6], [-2e6], [3e6]])


@functools.lru_cache(maxsize=None)
def cloud(name, dtype):
    """(xyz planar (3, N) of the cloud's own type, stored normals (N, 3) float32).  "surface": the noisy surface of test_pca_normals
    (seed 5); "volume": uniform in the unit cube; "far": the surface scaled by 1e-3 and moved to (1e6, -2e6, 3e6), fp64 only.
    The fp16 clouds are roundings of the fp32 ones; the fp64 clouds hold full-width values."""
    rng = np.random.default_rng(5)
    if name == "volume":
        rng = np.random.default_rng(6)
        p = rng.random((3, N))
        nrm = rng.standard_normal((N, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    else:
        p = rng.random((3, N))
        noise = 1e-3 * rng.standard_normal(N)
        if dtype in ("f32", "f16"):              # value for value the cloud of test_pca_normals
            p = p.astype(np.float32)
            p[2] = (0.3 + 0.1 * p[0] + 0.05 * np.sin(6 * p[1]) + noise).astype(np.float32)
        else:
            p[2] = 0.3 + 0.1 * p[0] + 0.05 * np.sin(6 * p[1]) + noise
        nrm = np.stack([-0.1 * np.ones(N), -0.3 * np.cos(6 * p[1].astype(np.float64)), np.ones(N)], axis=1) + 0.2 * rng.standard_normal((N, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        if name == "far":
            assert dtype == "f64"
            p = p * 1e-3 + FAR
    return np.ascontiguousarray(p.astype(DTYPES[dtype])), np.ascontiguousarray(nrm.astype(np.float32))


@functools.lru_cache(maxsize=None)
def lists32(name, dtype):
    """the exact 32 nearest neighbours (d2, id order) of the cloud's first M points, from the oracle's brute force: the first k columns
    are the exact k-lists, so no search kernel stands between these tests and the attribute stage"""
    from oracle import oracle as O
    xyz, _ = cloud(name, dtype)
    x64 = xyz.astype(np.float64)
    return O.knn_bruteforce(x64, np.ascontiguousarray(x64[:, :M]), 32)


def lists(name, dtype, k):
    idx, d2 = lists32(name, dtype)
    return np.ascontiguousarray(idx[:, :k]), np.ascontiguousarray(d2[:, :k])


def knock_out(idx, n, seed=11):
    """An exact k = 20 list with entries made missing: per row a random subset becomes NOIDX (rows 0..39 keep exactly 0, 1, 2 or 3
    entries, ten rows each), some ids become n or 0xFFFFFFFE, and blocks of rows lose the FIRST slot of a group of four (or the whole
    first group and the first slot of the second), so that the first valid neighbour sits at q != 0."""
    rng = np.random.default_rng(seed)
    out = np.array(idx, np.uint32, copy=True)
    m, k = out.shape
    keep = rng.random((m, k)) < rng.random((m, 1))
    for r in range(40):
        keep[r] = False
        keep[r, rng.choice(k, r // 10, replace=False)] = True
    keep[40:140] = True
    out[~keep] = NOIDX
    big = rng.random((m, k)) < 0.05
    big[:40] = False
    out[big] = np.where(rng.random(int(big.sum())) < 0.5, np.uint32(n), np.uint32(0xFFFFFFFE))
    out[40:60, 0] = NOIDX                         # first slot of the first group
    out[60:80, 4] = NOIDX                         # first slot of the second group
    out[80:100, 0:4] = NOIDX; out[80:100, 4] = n  # a whole group, then an id >= n: the origin is slot 5
    out[100:120, 0:3] = NOIDX                     # the origin is the last slot of its group
    out[120:140, 0:k - 3] = NOIDX                 # exactly the last three survive
    return out


def rotation(deg=40.0):
    """a rotation about (1, 1, 0) / sqrt 2 (tens of degrees: a stale table cannot pass for the rotated cloud's)"""
    a = np.deg2rad(deg)
    u = np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def blend_case(k, n=5000, m=640, seed=3):
    """Hand-built lists for the blend, the same for the CPU and the GPU suite: (idx (m, k), d2 (m, k), rgb (n, 3) u8, nrm (n, 3) f32).
    Blocks of 64 rows: 0 random; 1 exact d2 = 0 hits next to neighbours 1e6 times farther than the near ones (mode 1 weights 1e12, 1e6,
    1e-6); 2 pairs of exactly opposite normals at equal d2 (the sum is below 1e-12 and stays unnormalised; an odd k leaves the last
    slot empty, k = 1 has no such rows); 3 NOIDX at the head, 4 in the middle, 5 at the tail; 6 ids >= n sprinkled in; 7 rows without
    any valid entry (all NOIDX); 8 rows of ids >= n only; 9 random again with every d2 equal."""
    rng = np.random.default_rng(seed + k)
    rgb = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    nrm = rng.standard_normal((n, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[1:64:2] = -nrm[0:64:2]                                    # records 2i, 2i + 1: exactly opposite normals
    idx = rng.integers(64, n, (m, k)).astype(np.uint32)
    d2 = (rng.random((m, k)) * 1e-2) ** 2
    b = lambda i: slice(64 * i, 64 * (i + 1))
    tier = rng.integers(0, 3, (64, k)); tier[:, 0] = 0
    d2[b(1)] = np.choose(tier, [0.0, 1e-6, 1e6])
    if k >= 2:
        kp = k - k % 2
        start = rng.integers(0, 32 - kp // 2 + 1, 64) * 2
        bi, bd = idx[b(2)], d2[b(2)]                                # views
        bi[:, :kp] = (start[:, None] + np.arange(kp)[None, :]).astype(np.uint32)
        bi[:, kp:] = NOIDX
        bd[:, 1:kp:2] = bd[:, 0:kp:2]
    nh = rng.integers(1, max(k, 2), 64)                           # 1 .. k-1 missing (k = 1: the one entry)
    col = np.arange(k)[None, :]
    idx[b(3)] = np.where(col < nh[:, None], NOIDX, idx[b(3)])
    lo = rng.integers(0, k, 64)
    idx[b(4)] = np.where((col >= lo[:, None]) & (col < lo[:, None] + np.maximum(nh[:, None] // 2, 1)) & (col > 0) & (col < k - 1), NOIDX, idx[b(4)])
    idx[b(5)] = np.where(col >= k - nh[:, None], NOIDX, idx[b(5)])
    big = rng.random((64, k)) < 0.3
    idx[b(6)] = np.where(big, rng.choice(np.array([n, n + 7, 0xFFFFFFFE], np.uint32), (64, k)), idx[b(6)])
    idx[b(7)] = NOIDX
    idx[b(8)] = rng.choice(np.array([n, n + 1, 0xFFFFFFFE], np.uint32), (64, k))
    d2[b(9)] = 0.25
    d2[idx == NOIDX] = np.inf
    return idx, d2, rgb, nrm
