"""GPU suite: pt_bake_maps (csrc/pt_bake.hip) -- the colour atlas and the object-space normal map from one face pass.  Bars: the colour
plane equals pt_bake_texture's byte for byte (which the existing suites pin to the oracle); the normal plane equals the numpy float64
restatement tests/_bake_normal_ref.py byte for byte wherever the exact and the fp64 predicates agree (asserted, never skipped), and
on the degenerate rows it carries the colour plane's coverage and, for one normal everywhere, that normal's encoding.
PT_STRESS_BAKE_CASES sets the number of randomised cases (default 16)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import _bake_normal_ref as NR
import _bake_ref as B
from _bake_cases import ROW_NAMES, NOIDX, cloud_as, make_case, make_face_cases, merged, _interior, _outside, _rot

pytestmark = pytest.mark.gpu

ROWS = {r["name"]: r for r in make_face_cases()}
ONE = np.array([0.25, -0.5, 0.8125])                 # exact in float32; not unit: the map normalises per pixel


def source_normals(n, seed):
    """random, non-unit normals with a few zero and a few NaN records"""
    rng = np.random.default_rng(seed)
    nrm = (rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 1))).astype(np.float32)
    nrm[rng.random(n) < 0.04] = 0.0
    nrm[rng.random(n) < 0.03, int(rng.integers(3))] = np.nan
    return nrm


def vertex_normals(nv, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((nv, 3)) * 10.0 ** rng.uniform(-3, 3, (nv, 1))
    if nv > 4:
        v[1] = 0.0; v[4, 1] = np.nan
    return v


def records(pkg, xyz, rgb, uv=None, nrm=None):
    a = np.zeros(xyz.shape[1], dtype=pkg.POINT_DTYPE)
    a["ver"] = np.ascontiguousarray(xyz.T); a["color"] = np.asarray(rgb).astype(np.int32)
    if uv is not None:
        a["U"] = uv[:, 0]; a["V"] = uv[:, 1]
    if nrm is not None:
        a["normal"] = nrm
    return a


def resident(pkg, p, src, rgb, nrm, ctype):
    """the cloud made resident as `ctype` with its normals; returns the normals as the GPU holds them (float32, widened)"""
    held = np.asarray(nrm).astype(np.float32)
    if ctype == "f64":
        p.build_aos(records(pkg, src, rgb, nrm=np.asarray(nrm, np.float64)))
    else:
        p.build(src.astype(np.float16 if ctype == "f16" else np.float32), rgb, held)
    return held.astype(np.float64)


def general(row, src):
    return NR.faces_in_general_position(src, row["verts"], row["uv"], row["faces"], row["lists"])


def check_planes(pkg, p, row, src, held, vnrm, R, what, reference):
    """every claim that holds for any row; the normal plane against the reference when `reference`.  Returns the unpadded normal plane."""
    vrec = records(pkg, row["verts"], row["vrgb"], row["uv"], vnrm)
    want_c = p.bake_texture(vrec, row["faces"], row["lists"], R)
    col, nrm = p.bake_maps(vrec, row["faces"], row["lists"], R)
    assert np.array_equal(col, want_c), "%s R=%d: colour plane differs from bake_texture" % (what, R)
    only_c, none = p.bake_maps(vrec, row["faces"], row["lists"], R, normals=False)
    assert none is None and np.array_equal(only_c, want_c)
    none, only_n = p.bake_maps(vrec, row["faces"], row["lists"], R, color=False)
    assert none is None and np.array_equal(only_n, nrm), "%s R=%d: the normal plane alone differs from the one baked beside the colours" % (what, R)
    assert np.array_equal(nrm[:, :, 3], col[:, :, 3]), "%s R=%d: the planes disagree on coverage" % (what, R)
    assert not nrm[nrm[:, :, 3] == 0].any()
    pc, pn = p.bake_maps(vrec, row["faces"], row["lists"], R, pad_ksize=25)
    assert np.array_equal(pc, p.bake_texture(vrec, row["faces"], row["lists"], R, pad_ksize=25)), "%s R=%d: padded colour plane" % (what, R)
    assert np.array_equal(pn, p.texture_pad(nrm, 25)), "%s R=%d: padded normal plane" % (what, R)
    if reference:
        want = NR.bake(src, held, row["verts"], row["uv"], vnrm, row["faces"], row["lists"], R, B.exact_delaunay)
        bad = (nrm != want).any(axis=2)
        assert not bad.any(), "%s R=%d: %d of %d covered pixels differ from the reference" % (what, R, bad.sum(), (want[:, :, 3] == 255).sum())
    return nrm


@pytest.mark.parametrize("name", ROW_NAMES)
def test_rows(pkg, name):
    """every row of the bake's case table: colour plane unchanged, coverage shared, padding; the normal plane against the reference on
    the rows in general position; one normal everywhere gives its encoding on every row"""
    row = ROWS[name]
    n, nv = row["src"].shape[1], row["verts"].shape[1]
    for ctype in row["types"]:
        src = cloud_as(row, ctype)
        in_gp = general(row, src)
        assert in_gp or row["tri"] == "exact", "a row of random points must be in general position"      # (lattice rows need not be)
        with pkg.PointsTransfer(device=0, k_hint=row["k"]) as p:
            held = resident(pkg, p, src, row["rgb"], source_normals(n, 100), ctype)
            for R in row["R"]:
                check_planes(pkg, p, row, src, held, vertex_normals(nv, 101), R, "%s %s" % (name, ctype), in_gp)
        with pkg.PointsTransfer(device=0, k_hint=row["k"]) as p:
            resident(pkg, p, src, row["rgb"], np.tile(ONE, (n, 1)), ctype)
            vrec = records(pkg, row["verts"], row["vrgb"], row["uv"], np.tile(ONE, (nv, 1)))
            R = row["R"][-1]
            _, nrm = p.bake_maps(vrec, row["faces"], row["lists"], R, color=False)
            covered = nrm[:, :, 3] == 255
            assert (nrm[covered] == NR.encode(ONE)).all(), "%s %s: one normal everywhere" % (name, ctype)


def test_one_normal_has_room():
    """the encoding of ONE does not hang on the last ulp: every t + 0.5 is far from an integer"""
    t = ONE / np.sqrt((ONE * ONE).sum()) * 127.5 + 127.5 + 0.5
    assert np.minimum(t - np.floor(t), np.ceil(t) - t).min() > 1e-3


@pytest.mark.parametrize("ctype", ["f32", "f64"])
def test_all_rows_as_one_mesh(pkg, ctype):
    row = merged(list(ROWS.values()))
    src = cloud_as(row, ctype)
    n, nv = src.shape[1], row["verts"].shape[1]
    with pkg.PointsTransfer(device=0, k_hint=32) as p:
        held = resident(pkg, p, src, row["rgb"], source_normals(n, 102), ctype)
        nrm = check_planes(pkg, p, row, src, held, vertex_normals(nv, 103), 640, "merged " + ctype, False)
    assert (nrm[:, :, 3] == 255).mean() > 0.15


def random_case(case):
    """test_gpu_bake_paths.test_random_faces_match_oracle's construction (same seeds, same draws), plus normals"""
    rng = np.random.default_rng(7000 + case)
    k = int(rng.choice([1, 3, 8, 20, 27, 32])); R = int(rng.choice([97, 256])); ctype = ["f32", "f64"][case % 2]
    nf = int(rng.choice([1, 3, 5, 6, 7]))
    M = _rot(int(rng.integers(1 << 30))); shift = rng.standard_normal(3) * float(rng.choice([0.0, 1.0, 100.0]))
    pts, verts, uv, lists, faces = [], [], [], [], []
    g = int(np.ceil(np.sqrt(nf)))
    for f in range(nf):
        corners = (rng.random((3, 3)) * np.array([1.0, 1.0, 0.3]) * 10.0 ** rng.uniform(-2, 1)) @ M.T + shift
        n_in = int(rng.integers(0, min(96, 3 * k) + 1)); n_out = int(rng.integers(0, 3 * k - n_in + 1))
        xyz = np.concatenate([_interior(rng, n_in, corners), _outside(rng, n_out, corners)]).reshape(-1, 3)
        ids = len(pts) + rng.permutation(len(xyz))
        pts.extend(xyz)
        full = np.full(3 * k, NOIDX, np.uint32)
        full[:len(ids)] = ids
        if len(ids) and rng.random() < 0.5:
            free = np.nonzero(full == NOIDX)[0]
            full[free[:len(free) // 2]] = rng.choice(ids, size=len(free) // 2)
        lists.extend(rng.permutation(full).reshape(3, k))
        s = 1.0 / g
        o = np.array([(f % g) * s, (f // g) * s])
        uv.extend(o + s * (0.02 + 0.96 * rng.random((3, 2))))
        verts.extend(corners); faces.append(list(3 * f + rng.permutation(3)))
    if not pts:
        pts = [np.zeros(3)]
    n = len(pts)
    row = dict(src=np.ascontiguousarray(np.array(pts).T), rgb=rng.integers(0, 256, size=(n, 3), dtype=np.uint8), verts=np.ascontiguousarray(np.array(verts).T),
               uv=np.array(uv), vrgb=rng.integers(0, 256, size=(3 * nf, 3)).astype(np.int32), faces=np.array(faces, np.int32), lists=np.array(lists, np.uint32), k=k)
    return row, k, R, ctype, source_normals(n, 9000 + case), vertex_normals(3 * nf, 9500 + case)


@pytest.mark.parametrize("case", range(int(os.environ.get("PT_STRESS_BAKE_CASES", "16"))))
def test_random_faces_match_reference(pkg, case):
    row, k, R, ctype, snrm, vnrm = random_case(case)
    src = cloud_as(row, ctype)
    assert general(row, src), "case %d is not in general position: the seeds are checked before they are committed" % case
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        held = resident(pkg, p, src, row["rgb"], snrm, ctype)
        check_planes(pkg, p, row, src, held, vnrm, R, "case %d: k=%d %s" % (case, k, ctype), True)


def hole_case():
    """a height-field cloud with a hole the mesh spans, and the mesh under it"""
    src, rgb, verts, uv, vrgb, faces = make_case(21, n=4000, grid=6)
    keep = ~((np.abs(src[0] - 0.5) < 0.24) & (np.abs(src[1] - 0.45) < 0.24))
    return np.ascontiguousarray(src[:, keep]), np.ascontiguousarray(rgb[keep]), verts, uv, vrgb.astype(np.int32), faces


def test_capped_lists_over_a_hole(pkg):
    """lists from a max_dist query: PT_NOIDX entries, empty rows, and two out-of-range entries put there by hand"""
    src, rgb, verts, uv, vrgb, faces = hole_case()
    n, nv, k, R = src.shape[1], verts.shape[1], 20, 256
    snrm, vnrm = source_normals(n, 104), vertex_normals(nv, 105)
    with pkg.PointsTransfer(device=0, k_hint=k, max_dist=0.07) as p:
        held = resident(pkg, p, src, rgb, snrm, "f64")
        idx, _ = p.query(verts, k=k)
        empty = (idx == NOIDX).all(axis=1)
        assert 0 < empty.sum() < nv // 2 and (idx == NOIDX).any(axis=1).sum() > empty.sum()
        idx[0, 0] = n + 5; idx[7, 3] = n
        row = dict(verts=verts, uv=uv, vrgb=vrgb, faces=faces, lists=idx, k=k)
        bare = [f for f in faces if empty[f].all()]
        assert bare, "no face lies wholly over the hole"
        assert general(row, src)
        check_planes(pkg, p, row, src, held, vnrm, R, "hole", True)


def test_argument_contract(pkg):
    row = ROWS["np66"]
    src = cloud_as(row, "f32")
    L = pkg.capi.lib()
    vrec = records(pkg, row["verts"], row["vrgb"], row["uv"])
    f = np.ascontiguousarray(row["faces"], np.int32); nb = np.ascontiguousarray(row["lists"], np.uint32)
    R = 64
    a, b = np.empty((R, R, 4), np.uint8), np.empty((R, R, 4), np.uint8)
    ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)

    def call(p, maps, color, normal):
        return L.pt_bake_maps(p._h, ptr(vrec), len(vrec), ptr(f), len(f), ptr(nb), nb.shape[1], R, 0, maps, ptr(color), ptr(normal))
    with pkg.PointsTransfer(device=0) as p:
        assert call(p, 3, a, b) == pkg.capi.ERR_STATE                          # no cloud resident
        resident(pkg, p, src, row["rgb"], source_normals(src.shape[1], 1), "f32")
        for maps, color, normal in ((0, a, b), (4, a, b), (7, a, b), (-1, a, b), (1, None, b), (2, a, None), (3, a, None), (3, None, b)):
            assert call(p, maps, color, normal) == pkg.capi.ERR_ARG, (maps, color is None, normal is None)
        assert call(p, 3, a, b) == pkg.capi.OK
        c1, n2 = np.empty_like(a), np.empty_like(b)
        assert call(p, 1, c1, None) == pkg.capi.OK and call(p, 2, None, n2) == pkg.capi.OK      # a null pointer for a plane not asked for
        assert np.array_equal(c1, a) and np.array_equal(n2, b)
        assert p.stats()["ms_bake"] > 0
        with pytest.raises(ValueError):
            p.bake_maps(vrec, f, nb, R, color=False, normals=False)
    with pkg.PointsTransfer(device=0) as p:                                    # a slab context
        half = np.flatnonzero(src[0] < 0.5).astype(np.uint32)
        p.build(np.ascontiguousarray(src[:, half], dtype=np.float32), gidx=half)
        assert call(p, 3, a, b) == pkg.capi.ERR_UNSUPPORTED


def _write_plys(pc, mesh, src, rgb, snrm, verts, uv, vrgb, vnrm, faces):
    n, m = src.shape[1], verts.shape[1]
    cd = np.dtype([("p", "<f8", 3), ("n", "<f4", 3), ("c", "u1", 3)])
    a = np.zeros(n, cd); a["p"] = src.T; a["n"] = snrm; a["c"] = rgb
    with open(pc, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\n"
                 "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % n).encode())
        f.write(a.tobytes())
    md = np.dtype([("p", "<f8", 3), ("n", "<f8", 3), ("uv", "<f8", 2), ("c", "<i4", 3)])
    b = np.zeros(m, md); b["p"] = verts.T; b["n"] = vnrm; b["uv"] = uv; b["c"] = vrgb
    fd = np.dtype([("k", "u1"), ("v", "<i4", 3)])
    fc = np.zeros(len(faces), fd); fc["k"] = 3; fc["v"] = faces
    with open(mesh, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\n"
                 "property double nx\nproperty double ny\nproperty double nz\nproperty double s\nproperty double t\nproperty int red\n"
                 "property int green\nproperty int blue\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n" % (m, len(faces))).encode())
        f.write(b.tobytes()); f.write(fc.tobytes())


def _read_png_bgra(path):
    import struct, zlib
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    off, idat, w, h = 8, [], 0, 0
    while off < len(data):
        ln, typ = struct.unpack(">I4s", data[off:off + 8])
        body = data[off + 8:off + 8 + ln]
        if typ == b"IHDR":
            w, h = struct.unpack(">II", body[:8])
        elif typ == b"IDAT":
            idat.append(body)
        off += 12 + ln
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(h, w * 4 + 1)
    assert not raw[:, 0].any()                                                 # filter type 0 on every row
    return raw[:, 1:].reshape(h, w, 4)[:, :, [2, 1, 0, 3]]


def _cli_case(tmp_path):
    src, rgb, verts, uv, vrgb, faces = make_case(22, n=3000, grid=5)
    n, nv = src.shape[1], verts.shape[1]
    rng = np.random.default_rng(23)
    snrm = rng.standard_normal((n, 3)).astype(np.float32); vnrm = rng.standard_normal((nv, 3)).round(3)
    _write_plys(tmp_path / "cloud.ply", tmp_path / "mesh.ply", src, rgb, snrm, verts, uv, vrgb, vnrm, faces)
    return src, rgb, snrm, verts, uv, vrgb, vnrm, faces


def _expected_maps(pkg, case, k, R):
    src, rgb, snrm, verts, uv, vrgb, vnrm, faces = case
    vrec = records(pkg, verts, vrgb, uv, vnrm)
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        p.build(src, rgb, snrm)
        idx, _ = p.query_aos(vrec, k=k)
        return p.bake_maps(vrec, faces, idx, R)


@pytest.mark.parametrize("texture", [True, False])
def test_cli_normal_map(tmp_path, pkg, texture):
    case = _cli_case(tmp_path)
    k, R = 8, 256
    exe = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "pointsTransfer")
    cmd = [exe, "cloud.ply", "mesh.ply", "--k", str(k), "--normal-map", "n.png", "--texture", "t.png" if texture else "", "--resolution", str(R), "--pad", "0",
           "--json", "run.json"]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path, timeout=600)
    assert res.returncode == 0, res.stderr
    heads = [l.split(":")[0] for l in res.stdout.strip().splitlines()]
    assert heads == ["PC Point count", "Read point set in", "Built Kd tree in", "Mesh vertex count", "Mesh face count", "Read mesh faces",
                     "Neighbor search total time", "Draw triangles total time", "Output time", "Total real time", "VIRT", "RES"]
    assert json.load(open(tmp_path / "run.json"))["normal_map"] == "n.png"
    col, nrm = _expected_maps(pkg, case, k, R)
    assert (nrm[:, :, 3] == 255).mean() > 0.5
    assert np.array_equal(_read_png_bgra(tmp_path / "n.png"), nrm)
    assert os.path.exists(tmp_path / "t.png") == texture
    if texture:
        assert np.array_equal(_read_png_bgra(tmp_path / "t.png"), col)


def test_cli_json_escapes_the_file_name(tmp_path, pkg):
    _cli_case(tmp_path)
    name = 'n "q\\.png'                                        # a quote and a backslash: legal in a file name, not in a JSON string
    exe = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "pointsTransfer")
    res = subprocess.run([exe, "cloud.ply", "mesh.ply", "--k", "8", "--normal-map", name, "--texture", "", "--resolution", "64", "--pad", "0", "--json", "run.json"],
                         capture_output=True, text=True, cwd=tmp_path, timeout=600)
    assert res.returncode == 0, res.stderr
    assert json.load(open(tmp_path / "run.json"))["normal_map"] == name and os.path.exists(tmp_path / name)


@pytest.mark.parametrize("texture", [True, False])
def test_cli_normal_map_sharded(tmp_path, pkg, texture):
    """--gpus 1: launcher -> one rank process -> the finalize process, which bakes on the cloud of referenced points (their normals travel
    in the rank file).  The PNGs equal bake_maps on the whole cloud, and so the single-process run's."""
    case = _cli_case(tmp_path)
    k, R = 8, 256
    exe = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "pointsTransfer")
    cmd = [exe, "cloud.ply", "mesh.ply", "--k", str(k), "--gpus", "1", "--normal-map", "n.png", "--texture", "t.png" if texture else "", "--resolution", str(R),
           "--pad", "25", "--rendezvous-root", str(tmp_path)]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path, timeout=600)
    assert res.returncode == 0, res.stderr
    col, nrm = _expected_maps(pkg, case, k, R)
    with pkg.PointsTransfer(device=0) as p:
        assert np.array_equal(_read_png_bgra(tmp_path / "n.png"), p.texture_pad(nrm, 25))
        assert os.path.exists(tmp_path / "t.png") == texture
        if texture:
            assert np.array_equal(_read_png_bgra(tmp_path / "t.png"), p.texture_pad(col, 25))


def test_cli_rejects_normal_map_without_a_mesh(tmp_path, pkg):
    exe = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "pointsTransfer")
    r = subprocess.run([exe, "a", "b", "--synthetic", "1000", "100", "1", "--normal-map", "x.png"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 2 and "--normal-map" in r.stderr and not os.path.exists(tmp_path / "x.png")
