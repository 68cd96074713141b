"""Inputs of the outlier-removal tests, shared by tests/test_outlier_ref.py (CPU: the reference and the band condition) and
tests/test_gpu_outliers.py (GPU: pt_remove_outliers against the reference), so that both read the same clouds and the same lists."""
import functools

import numpy as np

import _attr_cases as cases

N = cases.N
N_STRAY = 500
KS = (2, 8, 16, 32)
ALPHAS = ((16, 1.0),) + tuple((k, 2.0) for k in KS)            # (k, alpha) of the GPU matrix: every k at alpha = 2, k = 16 at alpha = 1 too
NAMES = ("surface", "volume")
DTYPES = ("f32", "f16", "f64")
BAND = 1e-9                                                    # relative half-width of the band around T inside which a point may be left out
CAP = 0.05                                                     # the max_dist of the capped case: most injected points have nobody that near


@functools.lru_cache(maxsize=None)
def cloud(name, dtype):
    """(xyz planar (3, N) of the cloud's own type, rgb (N, 3) u8, nrm (N, 3) f32, stray (N_STRAY,) indices): _attr_cases' cloud with 500
    of its points replaced by points uniform in [-1, 2)^3 -- flyers around and between the unit-cube clouds."""
    xyz = np.array(cases.cloud(name, dtype)[0], copy=True)
    rng = np.random.default_rng(21)
    stray = rng.choice(N, N_STRAY, replace=False)
    xyz[:, stray] = (rng.random((N_STRAY, 3)) * 3 - 1).T.astype(xyz.dtype)
    arng = np.random.default_rng(22)
    rgb = arng.integers(0, 256, (N, 3)).astype(np.uint8)
    nrm = arng.standard_normal((N, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.ascontiguousarray(xyz), rgb, np.ascontiguousarray(nrm), np.sort(stray)


@functools.lru_cache(maxsize=None)
def self_lists32(name, dtype):
    """the exact 32 nearest neighbours, (d2, id) order, of EVERY point of the cloud among the cloud's points (oracle brute force)"""
    from oracle import oracle as O
    x64 = cloud(name, dtype)[0].astype(np.float64)
    return O.knn_bruteforce(x64, x64, 32)


def self_lists(name, dtype, k):
    idx, d2 = self_lists32(name, dtype)
    return np.ascontiguousarray(idx[:, :k]), np.ascontiguousarray(d2[:, :k])


def radius_for(name, dtype):
    """the RADIUS cases' r: 1.5 x the median distance to the 9th neighbour (column 9 of the lists: column 0 is the point itself)"""
    _, d2 = self_lists32(name, dtype)
    return 1.5 * float(np.sqrt(np.median(d2[:, 9])))
