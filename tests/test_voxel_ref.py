"""The voxel-downsampling reference (tests/_voxel_ref.py) against answers worked out by hand, and the properties of the shared cases
(tests/_voxel_cases.py) that the GPU suite relies on -- so that a change of a cloud cannot silently stop a case from covering its path."""
import numpy as np
import pytest

import _voxel_cases as VC
import _voxel_ref as R


def _planar(points, dtype=np.float64):
    return np.ascontiguousarray(np.array(points, dtype=np.float64).T.astype(dtype))


def test_points_on_voxel_faces():
    # v = 0.25 and every coordinate a multiple of 2^-12: all arithmetic is exact.  A face belongs to the voxel above it
    xs = [0.0, 0.25, 0.4998779296875, 0.5, 0.2498779296875, 0.75]
    r = R.downsample(_planar([(x, 0.0, 0.0) for x in xs]), 0.25, (0.0, 0.0, 0.0))
    assert list(r["voxel_of"]) == [0, 1, 1, 2, 0, 3] and list(r["counts"]) == [2, 2, 1, 1]
    assert r["dims"] == [4, 1, 1] and r["bits"] == [2, 0, 0] and r["passes"] == 1
    assert list(r["xyz"][0]) == [(0.0 + 0.2498779296875) / 2, (0.25 + 0.4998779296875) / 2, 0.5, 0.75]
    # the order is (iz, iy, ix), z highest: a point one voxel up in z comes after every point of the z = 0 layer
    r = R.downsample(_planar([(0.0, 0.0, 0.25), (0.75, 0.25, 0.0), (0.0, 0.25, 0.0), (0.5, 0.0, 0.0)]), 0.25, (0.0, 0.0, 0.0))
    assert list(r["voxel_of"]) == [3, 2, 1, 0]


def test_caller_origin_with_rounded_arithmetic():
    # 0.3 - 0.1 = 0.19999999999999998 in double, and that over 0.1 is 1.9999999999999998: voxel 1, although 0.2 / 0.1 "is" 2.
    # 0.7 - 0.1 = 0.6 (rounded up), over 0.1 = 5.999999999999999: voxel 5.  0.5 - 0.1 = 0.4, over 0.1 = 4 exactly
    r = R.downsample(_planar([(0.3, 0.1, 0.1), (0.7, 0.1, 0.1), (0.5, 0.1, 0.1), (0.1, 0.1, 0.1)]), 0.1, (0.1, 0.1, 0.1))
    assert list(r["voxel_of"]) == [1, 3, 2, 0] and r["dims"] == [6, 1, 1] and r["origin"] == [0.1, 0.1, 0.1]
    # without an origin the cloud's minimum is taken: the same answer here
    assert list(R.downsample(_planar([(0.3, 0.1, 0.1), (0.7, 0.1, 0.1), (0.5, 0.1, 0.1), (0.1, 0.1, 0.1)]), 0.1)["voxel_of"]) == [1, 3, 2, 0]
    with pytest.raises(ValueError):
        R.downsample(_planar([(0.3, 0.1, 0.1)]), 0.1, (0.1, 0.2, 0.1))             # origin above the cloud
    with pytest.raises(ValueError):
        R.downsample(_planar([(0.0, 0.0, 0.0), (3.0, 0.0, 0.0)]), 1e-6)            # an index reaches 2^21
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            R.downsample(_planar([(0.0, 0.0, 0.0)]), bad)


def test_blocked_sum_differs_from_the_sequential_sum():
    # 300 members of one voxel: rank 0 is 1.0, every other one 2^-53.  Added one by one, 1.0 + 2^-53 is a tie that rounds back to 1.0,
    # 299 times: the sequential sum is 1.0.  Blocked: P_0 = 1.0 (the same ties), P_1 = 44 * 2^-53 exactly, S = 1.0 + 22 * 2^-52
    t = 2.0 ** -53
    vals = np.array([1.0] + [t] * 299)
    assert R.plain_sum(vals) == 1.0
    assert R.blocked_sum(vals) == 1.0 + 22 * 2.0 ** -52 != R.plain_sum(vals)
    r = R.downsample(_planar([(x, 0.0, 0.0) for x in vals]), 2.0, (0.0, 0.0, 0.0))
    assert r["n_voxels"] == 1 and r["max_count"] == 300
    assert r["xyz"][0, 0] == (1.0 + 22 * 2.0 ** -52) / 300.0 != 1.0 / 300.0
    # at 256 members and below the two are the same sum
    assert R.blocked_sum(vals[:256]) == R.plain_sum(vals[:256]) == 1.0
    # normals take the same blocked sum (2^-53 is a float32 value), and the quotient is rounded to float32
    n = np.zeros((300, 3), np.float32); n[:, 0] = vals.astype(np.float32)
    rn = R.downsample(_planar([(x, 0.0, 0.0) for x in vals]), 2.0, (0.0, 0.0, 0.0), np.zeros((300, 3), np.uint8), n)
    assert rn["nrm"][0, 0] == np.float32((1.0 + 22 * 2.0 ** -52) / 300.0)


def test_colour_rounds_half_up():
    pts = _planar([(0.1, 0.1, 0.1), (0.2, 0.1, 0.1), (1.1, 0.1, 0.1), (1.2, 0.1, 0.1), (1.3, 0.1, 0.1)])
    rgb = np.array([[1, 0, 255], [2, 1, 254], [1, 0, 7], [1, 0, 7], [2, 1, 8]], np.uint8)
    r = R.downsample(pts, 1.0, (0.0, 0.0, 0.0), rgb, np.zeros((5, 3), np.float32))
    # voxel 0: means 1.5, 0.5, 254.5 -> 2, 1, 255;  voxel 1: means 4/3, 1/3, 22/3 -> 1, 0, 7
    assert r["rgb"].tolist() == [[2, 1, 255], [1, 0, 7]]


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.float16])
def test_a_single_member_voxel_reproduces_its_point(dtype):
    pts = _planar([(0.1234567890123, -0.0, 5.5), (7.3, 2.000001, -0.75), (3.14159, 1e-5, 0.3)], dtype)
    nrm = np.array([[0.1, -0.2, 0.3], [-0.0, 1.0, 0.0], [0.6, 0.0, 0.8]], np.float32)
    rgb = np.array([[1, 2, 3], [255, 0, 128], [9, 9, 9]], np.uint8)
    r = R.downsample(pts, 0.5, None, rgb, nrm)
    assert r["n_voxels"] == 3 and r["max_count"] == 1 and r["xyz"].dtype == dtype
    order = np.argsort(r["voxel_of"])
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize]
    assert np.array_equal(r["xyz"].view(u), np.ascontiguousarray(pts[:, order]).view(u))          # bit for bit, the -0.0 included
    assert np.array_equal(r["nrm"].view(np.uint32), nrm[order].view(np.uint32)) and np.array_equal(r["rgb"], rgb[order])


def test_fp16_is_rounded_through_fp32():
    # the mean 1 + 2^-11 + 2^-25 lies just above a tie of the fp16 grid: directly it rounds up to 1 + 2^-10; through fp32 the 2^-25 is
    # lost first (a tie of the fp32 grid, to even), and the fp16 tie then rounds to even: 1.0
    q = np.float64(1.0 + 2.0 ** -11 + 2.0 ** -25)
    assert np.float16(q) == np.float16(1.0 + 2.0 ** -10) and q.astype(np.float32).astype(np.float16) == np.float16(1.0)


def test_the_cases_cover_what_the_gpu_suite_needs():
    for name in VC.NAMES:
        big, small, one = VC.ref(name, "f32", 0.5), VC.ref(name, "f32", 0.05), VC.ref(name, "f32", 10.0)
        assert big["max_count"] > R.BLOCK and (big["counts"] > R.BLOCK).sum() == 8 and big["passes"] == 2
        assert small["max_count"] <= R.BLOCK and small["passes"] == 3
        assert one["n_voxels"] == 1 and one["max_count"] == VC.N and one["passes"] == 0 and one["bits"] == [0, 0, 0]
        assert VC.ref(name, "f32", 0.004)["passes"] == 4
    wide = VC.ref("volume", "f32", VC.V_WIDE)
    assert sum(wide["bits"]) > 32 and wide["passes"] == 6
    assert (VC.ref("surface", "f32", 0.004)["n_voxels"], VC.ref("volume", "f32", 0.004)["n_voxels"]) == (38627, 49922)
    assert (VC.ref("surface", "f32", 0.05)["n_voxels"], VC.ref("volume", "f32", 0.05)["n_voxels"]) == (1059, 9129)
    far = [VC.ref("far", "f64", v) for v in VC.FAR_VOXELS]
    assert [f["n_voxels"] for f in far] == [518, 26] and [f["max_count"] for f in far] == [160, 2120]
    assert [int((f["counts"] > R.BLOCK).sum()) for f in far] == [0, 25]
    assert VC.N % 4096 and VC.N % 256                                    # no multiple of the sort's tile or of the block
    for name, dtype, v in VC.MATRIX:                                     # every voxel holds its members, every point has a voxel
        r = VC.ref(name, dtype, v)
        assert np.array_equal(np.bincount(r["voxel_of"], minlength=r["n_voxels"]), r["counts"]) and r["counts"].sum() == VC.N
