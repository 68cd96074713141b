"""Inputs of the voxel-downsampling tests, shared by tests/test_voxel_ref.py (CPU: the reference and the properties of the cases) and
tests/test_gpu_voxel.py (GPU: pt_voxel_downsample against the reference): the clouds of the outlier tests -- N = 50 000 points, 500 of
them strays in [-1, 2)^3, so N is no multiple of any tile size -- and the far fp64 surface of the attribute tests."""
import functools

import numpy as np

import _attr_cases as cases
import _outlier_cases as OC
import _voxel_ref as R

N = OC.N
NAMES = OC.NAMES
DTYPES = OC.DTYPES
VOXELS = (0.004, 0.05, 0.5, 10.0)            # 4, 3, 2 and 0 radix passes; 0.5 and 10 have voxels of more than 256 members (the blocked path)
V_WIDE = 0.0002                              # ~15000 voxels per axis: 42 key bits, the 64-bit key, 6 passes
FAR_VOXELS = (5e-5, 2e-4)

# (name, dtype, voxel) of the GPU matrix
MATRIX = [(name, dtype, v) for name in NAMES for dtype in DTYPES for v in VOXELS] + [("volume", "f32", V_WIDE), ("volume", "f64", V_WIDE)] + \
         [("far", "f64", v) for v in FAR_VOXELS]


@functools.lru_cache(maxsize=None)
def cloud(name, dtype):
    """(xyz planar (3, N), rgb (N, 3) u8, nrm (N, 3) f32)"""
    if name == "far":
        xyz, nrm = cases.cloud("far", dtype)
        rgb = np.random.default_rng(24).integers(0, 256, (N, 3)).astype(np.uint8)
        return xyz, rgb, nrm
    return OC.cloud(name, dtype)[:3]


@functools.lru_cache(maxsize=None)
def ref(name, dtype, v, origin=None):
    """the reference's answer (tests/_voxel_ref.py), computed once per case and shared: treat it as read-only"""
    xyz, rgb, nrm = cloud(name, dtype)
    return R.downsample(xyz, v, origin, rgb, nrm)
