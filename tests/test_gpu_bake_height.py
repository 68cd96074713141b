"""GPU suite: pt_bake_maps_h (csrc/pt_bake.hip) -- the height map beside the colour atlas and the normal map, one face pass.  Bars: the
colour and normal planes equal pt_bake_maps' byte for byte; the height plane is the same whichever planes are baked beside it, shares
their coverage and pads like them; wherever the exact and the fp64 predicates agree (asserted, never skipped) it equals the numpy
float64 restatement tests/_bake_height_ref.py byte for byte, and max_abs_height equals the reference's exactly."""
import ctypes as C

import numpy as np
import pytest

import _bake_height_ref as HR
import _bake_normal_ref as NR
import _bake_ref as B
from _bake_cases import ROW_NAMES, NOIDX, UNIT, _Mesh, cloud_as, make_case, make_face_cases, merged, _interior, _outside, _rot

pytestmark = pytest.mark.gpu

ROWS = {r["name"]: r for r in make_face_cases()}
H_ROWS = 0.02            # the rows lift their interior points by 0.01 |edge| N(0, 1): most texels inside the range, a few saturate


def records(pkg, xyz, rgb, uv=None, nrm=None):
    a = np.zeros(xyz.shape[1], dtype=pkg.POINT_DTYPE)
    a["ver"] = np.ascontiguousarray(xyz.T); a["color"] = np.asarray(rgb).astype(np.int32)
    if uv is not None:
        a["U"] = uv[:, 0]; a["V"] = uv[:, 1]
    if nrm is not None:
        a["normal"] = nrm
    return a


def normals(n, seed):
    return np.random.default_rng(seed).standard_normal((n, 3)).astype(np.float32)


def resident(pkg, p, src, rgb, ctype, seed=5):
    """the cloud made resident as `ctype`, with normals for the normal plane"""
    nrm = normals(src.shape[1], seed)
    if ctype == "f64":
        p.build_aos(records(pkg, src, rgb, nrm=nrm.astype(np.float64)))
    else:
        p.build(src.astype(np.float16 if ctype == "f16" else np.float32), rgb, nrm)


def general(row, src):
    return NR.faces_in_general_position(src, row["verts"], row["uv"], row["faces"], row["lists"])


def triangulation(row):
    return B.scipy_delaunay if row.get("tri", "scipy") == "scipy" else B.exact_delaunay


def grey(hgt):
    """the height bytes of the covered pixels; checks the pixel layout on the way"""
    cov = hgt[:, :, 3] == 255
    assert not hgt[~cov].any(), "uncovered pixels must be 0"
    px = hgt[cov]
    assert (px[:, 0] == px[:, 1]).all() and (px[:, 0] == px[:, 2]).all()
    return px[:, 0]


def check_planes(pkg, p, row, src, R, H, what, reference):
    """every claim that holds for any row; the height plane and max_abs_height against the reference when `reference`.
    Returns (unpadded height plane, info)."""
    vrec = records(pkg, row["verts"], row["vrgb"], row["uv"], normals(row["verts"].shape[1], 6).astype(np.float64))
    f, nb = row["faces"], row["lists"]
    want_c, want_n = p.bake_maps(vrec, f, nb, R)
    col, nrm, hgt, info = p.bake_maps_h(vrec, f, nb, R, height_range=H)
    assert np.array_equal(col, want_c), "%s R=%d: colour plane differs from bake_maps" % (what, R)
    assert np.array_equal(nrm, want_n), "%s R=%d: normal plane differs from bake_maps" % (what, R)
    for color, nrms in ((False, False), (True, False), (False, True)):           # the other three map sets with the height bit
        c2, n2, h2, i2 = p.bake_maps_h(vrec, f, nb, R, color=color, normals=nrms, height_range=H)
        assert (c2 is None) == (not color) and (n2 is None) == (not nrms)
        assert np.array_equal(h2, hgt), "%s R=%d: the height plane depends on the planes beside it (%s, %s)" % (what, R, color, nrms)
        assert i2 == info
        assert (c2 is None or np.array_equal(c2, want_c)) and (n2 is None or np.array_equal(n2, want_n))
    assert np.array_equal(hgt[:, :, 3], col[:, :, 3]) and np.array_equal(nrm[:, :, 3], col[:, :, 3]), "%s R=%d: the planes disagree on coverage" % (what, R)
    grey(hgt)
    pc, pn, ph, _ = p.bake_maps_h(vrec, f, nb, R, pad_ksize=25, height_range=H)
    assert np.array_equal(ph, p.texture_pad(hgt, 25)), "%s R=%d: padded height plane" % (what, R)
    assert np.array_equal(pc, p.texture_pad(col, 25)) and np.array_equal(pn, p.texture_pad(nrm, 25))
    assert info["max_abs_height"] >= 0.0
    if reference:
        want, top = HR.bake(src, row["verts"], row["uv"], f, nb, R, H, triangulation(row))
        bad = (hgt != want).any(axis=2)
        assert not bad.any(), "%s R=%d: %d of %d covered pixels differ from the reference" % (what, R, bad.sum(), (want[:, :, 3] == 255).sum())
        assert info["max_abs_height"] == top, "%s: max_abs_height %r, reference %r" % (what, info["max_abs_height"], top)
    return hgt, info


@pytest.mark.parametrize("name", ROW_NAMES)
def test_rows(pkg, name):
    row = ROWS[name]
    for ctype in row["types"]:
        src = cloud_as(row, ctype)
        in_gp = general(row, src)
        assert in_gp or row["tri"] == "exact", "a row of random points must be in general position"      # (lattice rows need not be)
        with pkg.PointsTransfer(device=0, k_hint=row["k"]) as p:
            resident(pkg, p, src, row["rgb"], ctype)
            for R in row["R"]:
                hgt, info = check_planes(pkg, p, row, src, R, H_ROWS, "%s %s" % (name, ctype), in_gp)
            if name == "verts_bad":                    # only the two well-formed faces have interior points; the six others are flat
                only_bad = dict(row, faces=row["faces"][1:7])
                flat, i2 = check_planes(pkg, p, only_bad, src, R, H_ROWS, "verts_bad, the bad faces", in_gp)
                g = grey(flat)
                assert len(g) and (g == 128).all() and i2["max_abs_height"] == 0.0 and info["max_abs_height"] > 0.0


# ---- this file's own cases: points well off the plane, on both sides -------------------------------------------------------------------
PERM = dict(px=[[0, 0, 1], [0, 1, 0], [-1, 0, 0]], nx=[[0, 0, -1], [0, 1, 0], [1, 0, 0]], py=[[1, 0, 0], [0, 0, 1], [0, -1, 0]],
            ny=[[1, 0, 0], [0, 0, -1], [0, 1, 0]], nz=[[1, 0, 0], [0, -1, 0], [0, 0, -1]], rand=_rot(71))


def lifted_case(k, seed):
    """six faces, one per frame of PERM (normal along +x, -x, +y, -y, -z and a seeded rotation), in three corner orders, each with
    interior points lifted by 0.25 |edge| N(0, 1) and a few outside ones; for k = 32 the first face has 96 candidates, all inside
    (the second 64-lane chunk of the projection loop carries heights)"""
    rng = np.random.default_rng(seed)
    m = _Mesh(k, 6)
    shift = np.array([3.0, -2.0, 5.0])
    for s, M in enumerate(PERM.values()):
        M = np.array(M, np.float64)
        corners = UNIT @ M.T + shift
        n_in = 3 * k if (s == 0 or k < 8) else min(3 * k - 4, 20)
        pts = np.concatenate([_interior(rng, n_in, UNIT, lift=0.25) @ M.T + shift, (_outside(rng, 3 * k - n_in) + [0, 0, 0.3]) @ M.T + shift])
        m.face(corners, m.cloud(pts), order=((0, 1, 2), (1, 2, 0), (0, 2, 1))[s % 3], rng=rng)
    return m.row("lifted_k%d" % k, (128,), ("f32", "f64"), "scipy", None)


@pytest.mark.parametrize("ctype", ["f32", "f64"])
@pytest.mark.parametrize("k", [1, 8, 20, 32])
def test_points_far_off_the_plane(pkg, k, ctype):
    row = lifted_case(k, 800 + k)
    src = cloud_as(row, ctype)
    assert general(row, src), "the seeds are checked before they are committed"
    faces0 = row["faces"][0]
    P, _, h, _ = HR.face_heights(src, row["verts"], row["uv"], faces0, row["lists"])
    if k == 32:
        assert len(P) == 99                                 # 96 kept points: candidates 64..95 are kept ones
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        resident(pkg, p, src, row["rgb"], ctype)
        _, info = check_planes(pkg, p, row, src, 128, 0.1, "lifted k=%d %s, H below max |h|" % (k, ctype), True)
        top = info["max_abs_height"]
        assert top > 0.1
        low, _ = check_planes(pkg, p, row, src, 128, top / 8.0, "lifted k=%d %s, H = max |h| / 8" % (k, ctype), True)
        g = grey(low)
        assert (g == 0).any() and (g == 255).any(), "both ends of the range must be reached"
        high, i3 = check_planes(pkg, p, row, src, 128, 1.25 * top, "lifted k=%d %s, H = 1.25 max |h|" % (k, ctype), True)
        g = grey(high)
        assert i3["max_abs_height"] == top                  # the maximum does not depend on H
        assert 0 < g.min() < 128 < g.max() < 255, "H >= max |h|: nothing saturates, both signs appear"


def test_height_sign_follows_the_winding(pkg):
    """one point above UNIT (winding faces +z): bright; the same face wound the other way: dark (a texel a hair below the plane
    truncates to 127, one a hair above stays 128)"""
    for order, bright in (((0, 1, 2), True), ((0, 2, 1), False)):
        m = _Mesh(4, 1)
        m.face(UNIT, m.cloud(np.array([[0.3, 0.3, 0.5]])), order=order)
        row = m.row("sign", (64,), ("f64",), "scipy", None)
        with pkg.PointsTransfer(device=0, k_hint=4) as p:
            resident(pkg, p, row["src"], row["rgb"], "f64")
            hgt, info = check_planes(pkg, p, row, row["src"], 64, 1.0, "sign", True)
        g = grey(hgt)
        assert info["max_abs_height"] == 0.5 and (g.max() > 180 and g.min() == 128 if bright else g.min() < 76 and g.max() <= 128)


@pytest.mark.parametrize("ctype", ["f32", "f64"])
def test_all_rows_as_one_mesh(pkg, ctype):
    """waves on different paths in one workgroup, the last workgroup not full; max_abs_height is the maximum over the rows"""
    m = _Mesh(4, 1)
    m.face(UNIT, m.cloud(np.array([[0.3, 0.3, 0.5], [0.2, 0.6, -0.25]])))
    rows = [r for r in ROWS.values() if not r.get("covers_atlas")] + [lifted_case(32, 832), m.row("two", (64,), ("f64",), "scipy", None)]
    row = merged(rows)
    src = cloud_as(row, ctype)
    assert len(row["faces"]) % 4 != 0
    with pkg.PointsTransfer(device=0, k_hint=32) as p:
        resident(pkg, p, src, row["rgb"], ctype)
        hgt, info = check_planes(pkg, p, row, src, 640, 0.1, "merged " + ctype, False)
    assert (hgt[:, :, 3] == 255).mean() > 0.15 and len(np.unique(grey(hgt))) > 100
    tops = []
    for r in rows:                                          # per row: the reference's maximum (heights do not depend on the triangulation)
        s = cloud_as(r, ctype)
        nv = r["verts"].shape[1]
        for fv in r["faces"]:
            if any(v < 0 or v >= nv for v in fv):
                continue
            h = HR.face_heights(s, r["verts"], r["uv"], fv, r["lists"])[2][3:]
            tops.extend(np.abs(h[np.isfinite(h)]))
    assert info["max_abs_height"] == max(tops)


def hole_case():
    """a height-field cloud with a hole the mesh spans, and the mesh under it"""
    src, rgb, verts, uv, vrgb, faces = make_case(21, n=4000, grid=6)
    keep = ~((np.abs(src[0] - 0.5) < 0.24) & (np.abs(src[1] - 0.45) < 0.24))
    return np.ascontiguousarray(src[:, keep]), np.ascontiguousarray(rgb[keep]), verts, uv, vrgb.astype(np.int32), faces


def test_capped_lists_over_a_hole(pkg):
    """lists from a max_dist query: PT_NOIDX entries and empty rows; a face without interior points is 128 throughout"""
    src, rgb, verts, uv, vrgb, faces = hole_case()
    n, nv, k, R = src.shape[1], verts.shape[1], 20, 256
    with pkg.PointsTransfer(device=0, k_hint=k, max_dist=0.07) as p:
        resident(pkg, p, src, rgb, "f64")
        idx, _ = p.query(verts, k=k)
        empty = (idx == NOIDX).all(axis=1)
        assert 0 < empty.sum() < nv // 2 and (idx == NOIDX).any(axis=1).sum() > empty.sum()
        idx[0, 0] = n + 5; idx[7, 3] = n
        row = dict(verts=verts, uv=uv, vrgb=vrgb, faces=faces, lists=idx, k=k, tri="scipy")
        bare = np.array([f for f in faces if empty[f].all()], np.int32)
        assert len(bare), "no face lies wholly over the hole"
        assert general(row, src)
        _, info = check_planes(pkg, p, row, src, R, 0.05, "hole", True)
        assert info["max_abs_height"] > 0.0
        flat, i2 = check_planes(pkg, p, dict(row, faces=bare), src, R, 0.05, "hole, bare faces", True)
        g = grey(flat)
        assert len(g) > 100 and (g == 128).all() and i2["max_abs_height"] == 0.0


def test_argument_contract(pkg):
    row = ROWS["np66"]
    src = cloud_as(row, "f32")
    L = pkg.capi.lib()
    vrec = records(pkg, row["verts"], row["vrgb"], row["uv"])
    f = np.ascontiguousarray(row["faces"], np.int32); nb = np.ascontiguousarray(row["lists"], np.uint32)
    R = 64
    a, b, h = (np.empty((R, R, 4), np.uint8) for _ in range(3))
    ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    ERR_ARG, OK = pkg.capi.ERR_ARG, pkg.capi.OK

    def call(p, maps, H, color, normal, height, res=None):
        return L.pt_bake_maps_h(p._h, ptr(vrec), len(vrec), ptr(f), len(f), ptr(nb), nb.shape[1], R, 0, maps, H, ptr(color), ptr(normal), ptr(height),
                                None if res is None else C.byref(res))

    def old(p, maps, color, normal):
        return L.pt_bake_maps(p._h, ptr(vrec), len(vrec), ptr(f), len(f), ptr(nb), nb.shape[1], R, 0, maps, ptr(color), ptr(normal))
    with pkg.PointsTransfer(device=0) as p:
        assert call(p, 7, 1.0, a, b, h) == pkg.capi.ERR_STATE == old(p, 3, a, b)               # no cloud resident
        resident(pkg, p, src, row["rgb"], "f32")
        for maps in (0, 8, -1, 15):
            assert call(p, maps, 1.0, a, b, h) == ERR_ARG, maps
        for maps, color, normal, height in ((4, a, b, None), (7, a, b, None), (5, None, b, h), (6, a, None, h), (1, None, b, h), (2, a, None, h)):
            assert call(p, maps, 1.0, color, normal, height) == ERR_ARG, (maps, color is None, normal is None, height is None)
        for H in (0.0, -0.0, -1.0, float("nan"), float("inf"), float("-inf")):
            for maps in (4, 5, 7):
                assert call(p, maps, H, a, b, h) == ERR_ARG, (maps, H)
        res = pkg.capi.BakeResult(-1.0)
        assert call(p, 7, 0.05, a, b, h, res) == OK and res.max_abs_height > 0.0
        assert call(p, 7, 0.05, a, b, h, None) == OK                                           # the result is optional
        assert p.stats()["ms_bake"] > 0
        h1 = np.empty_like(h)
        assert call(p, 4, 0.05, None, None, h1) == OK and np.array_equal(h1, h)               # null pointers for planes not asked for
        c0, n0 = np.empty_like(a), np.empty_like(b)
        assert old(p, 3, c0, n0) == OK and np.array_equal(c0, a) and np.array_equal(n0, b)
        for H in (0.0, -1.0, float("nan"), float("inf"), 3.0):                                 # the bit clear: any H, pt_bake_maps' results
            c1, n1 = np.empty_like(a), np.empty_like(b)
            res = pkg.capi.BakeResult(-1.0)
            assert call(p, 3, H, c1, n1, None, res) == OK and np.array_equal(c1, c0) and np.array_equal(n1, n0) and res.max_abs_height == 0.0
        c1 = np.empty_like(a)
        assert call(p, 1, float("nan"), c1, None, None) == OK and np.array_equal(c1, c0)
        assert old(p, 4, a, b) == ERR_ARG and old(p, 7, a, b) == ERR_ARG                       # pt_bake_maps still refuses the height bit
        with pytest.raises(ValueError):
            p.bake_maps_h(vrec, f, nb, R, color=False, normals=False)
        c2, n2, none, info = p.bake_maps_h(vrec, f, nb, R)
        assert none is None and info == {"max_abs_height": 0.0} and np.array_equal(c2, c0) and np.array_equal(n2, n0)
    with pkg.PointsTransfer(device=0) as p:                                    # a slab context
        half = np.flatnonzero(src[0] < 0.5).astype(np.uint32)
        p.build(np.ascontiguousarray(src[:, half], dtype=np.float32), gidx=half)
        assert call(p, 7, 1.0, a, b, h) == pkg.capi.ERR_UNSUPPORTED == old(p, 3, a, b)
    with pkg.PointsTransfer(device=0) as p:                                    # no attribute table
        p.build(src.astype(np.float32))
        assert call(p, 4, 1.0, None, None, h) == old(p, 1, a, None)
