"""Independent reference of pt_voxel_downsample (include/pt_api.h), numpy fp64: a stable np.lexsort instead of the radix sort, explicit
loops for the blocked sums.  It follows the header's definition to the letter:

  voxel      i = floor((p - o) / v) per axis on the coordinates widened to double, one rounding per operation, a true division;
             o = the caller's origin, or the per-axis minimum of the cloud;
  order      voxels ascending in (iz, iy, ix), members ascending in original index (lexsort is stable);
  blocked sum  P_b = ranks [256 b, 256 (b + 1)) added left to right starting from the first term, S = P_0, P_1, ... added left to right;
  position   S / c, rounded to the cloud's width -- fp16 through fp32 (.astype(float32).astype(float16));
  colour     per byte (2 s + c) // (2 c) on exact integer sums;
  normal     blocked sum of the floats widened to double, / c, rounded to float32; not renormalised."""
import numpy as np

BLOCK = 256
MAX_INDEX = 1 << 21


def voxel_indices(xyz, v, origin=None):
    """(idx int64 (3, n), origin float64 (3,), dims int64 (3,)); ValueError where the call returns PT_ERR_ARG"""
    p = np.asarray(xyz).astype(np.float64)
    o = p.min(axis=1) if origin is None else np.asarray(origin, np.float64).reshape(3)
    if not (np.isfinite(v) and v > 0) or not np.isfinite(o).all():
        raise ValueError("voxel / origin")
    i = np.floor((p - o[:, None]) / np.float64(v))
    if (i < 0).any():
        raise ValueError("origin above the cloud")
    if (i >= MAX_INDEX).any():
        raise ValueError("voxel too small for the cloud's extent")
    dims = np.floor((p.max(axis=1) - o) / np.float64(v)).astype(np.int64) + 1
    return i.astype(np.int64), o, dims


def key_bits(dims):
    return [int(d - 1).bit_length() for d in dims]          # ceil(log2 d): 0 for one voxel


def plain_sum(vals):
    """the left-to-right sum, starting from the first term"""
    s = np.float64(vals[0])
    for x in vals[1:]:
        s = s + np.float64(x)
    return s


def blocked_sum(vals):
    """the header's blocked sum of one voxel's values in rank order"""
    parts = [plain_sum(vals[a:a + BLOCK]) for a in range(0, len(vals), BLOCK)]
    return plain_sum(parts)


def _blocked_sums(vals, start, count):
    """blocked_sum of every segment vals[start[j] : start[j] + count[j]] at once (vals: (n, q) float64 in sorted order).  The loops run
    over the rank inside a block and over the block number; every addition is an elementwise fp64 addition, so each segment sees exactly
    the additions of blocked_sum, in its order."""
    nb = (count + BLOCK - 1) // BLOCK
    seg = np.repeat(np.arange(len(count)), nb)                                   # the voxel of every block
    first = np.cumsum(nb) - nb
    b = np.arange(nb.sum()) - first[seg]                                         # its number inside the voxel
    bstart = start[seg] + b * BLOCK
    bcount = np.minimum(BLOCK, count[seg] - b * BLOCK)
    P = vals[bstart].copy()                                                      # rank 0: the first term
    for r in range(1, int(bcount.max())):
        live = np.flatnonzero(bcount > r)
        P[live] = P[live] + vals[bstart[live] + r]
    S = P[first].copy()                                                          # P_0
    for k in range(1, int(nb.max())):
        live = np.flatnonzero(nb > k)
        S[live] = S[live] + P[first[live] + k]
    return S


def downsample(xyz, v, origin=None, rgb=None, nrm=None):
    """xyz planar (3, n) of the cloud's own type; rgb (n, 3) u8 and nrm (n, 3) f32 or None.  Returns a dict: voxel_of (n,) u32, counts
    (n_voxels,) u32, n_voxels, max_count, dims, origin, bits (per axis), passes, xyz (3, n_voxels) in the cloud's type, and rgb / nrm."""
    xyz = np.asarray(xyz)
    n = xyz.shape[1]
    idx, o, dims = voxel_indices(xyz, v, origin)
    order = np.lexsort((idx[0], idx[1], idx[2]))                                  # primary key last: (iz, iy, ix); stable
    s = idx[:, order]
    head = np.ones(n, bool)
    head[1:] = (s[:, 1:] != s[:, :-1]).any(axis=0)
    start = np.flatnonzero(head)
    count = np.diff(np.append(start, n))
    nv = len(start)
    voxel_of = np.empty(n, np.uint32)
    voxel_of[order] = (np.cumsum(head) - 1).astype(np.uint32)
    c = count.astype(np.float64)
    S = _blocked_sums(np.ascontiguousarray(xyz.astype(np.float64).T[order]), start, count)
    q = (S / c[:, None]).T
    out = q.astype(np.float32).astype(np.float16) if xyz.dtype == np.float16 else q.astype(xyz.dtype)
    bits = key_bits(dims)
    res = dict(voxel_of=voxel_of, counts=count.astype(np.uint32), n_voxels=nv, max_count=int(count.max()), dims=[int(d) for d in dims],
               origin=[float(x) for x in o], bits=bits, passes=(sum(bits) + 7) // 8, xyz=np.ascontiguousarray(out), rgb=None, nrm=None)
    if rgb is not None:
        sums = np.add.reduceat(np.asarray(rgb)[order].astype(np.int64), start, axis=0)          # exact integers: the order does not matter
        res["rgb"] = ((2 * sums + count[:, None]) // (2 * count[:, None])).astype(np.uint8)
    if nrm is not None:
        N = _blocked_sums(np.asarray(nrm, np.float32)[order].astype(np.float64), start, count)
        res["nrm"] = (N / c[:, None]).astype(np.float32)
    return res
