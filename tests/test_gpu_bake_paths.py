"""GPU suite: the texture-bake kernels (csrc/pt_bake.hip) on the paths a k-NN query of the corners never reaches -- more than 66 kept
points (the Delaunay loop's second 64-lane chunk), compaction from the upper half of the candidates, the 255-triangle cap, tilted
frames, mirrored UVs, slivers, coincident and collinear points, overlapping faces, every early return.  The neighbour lists are the
caller's (_bake_cases.make_face_cases()).  Bar: the atlas equals the oracle's byte for byte, with and without edge padding; that the
oracle took the path is asserted on its face report (tests/test_bake_oracle.py checks the oracle itself against scipy, exact predicates
and a numpy restatement on the same rows).  PT_STRESS_BAKE_CASES sets the number of randomised cases (default 16)."""
import os

import numpy as np
import pytest

from _bake_cases import ROW_NAMES, NOIDX, cloud_as, face_reports, make_face_cases, merged, point_records, _interior, _outside, _rot

pytestmark = pytest.mark.gpu

ROWS = {r["name"]: r for r in make_face_cases()}


def _resident(pkg, p, src, rgb, ctype):
    """the cloud (float64 image of its storage type) made resident as that type, with its colours"""
    if ctype == "f64":
        p.build_aos(point_records(pkg.POINT_DTYPE, src, rgb))
    else:
        p.build(src.astype(np.float16 if ctype == "f16" else np.float32), rgb, np.zeros((src.shape[1], 3), np.float32))


def _compare(pkg, oracle, p, row, src, R, what):
    vrec = point_records(pkg.POINT_DTYPE, row["verts"], row["vrgb"], row["uv"])           # colours as the int32 fields hold them
    want = oracle.bake_texture(src, row["rgb"], row["verts"], row["uv"], np.clip(row["vrgb"], 0, 255).astype(np.uint8), row["faces"], row["lists"], R)
    got = p.bake_texture(vrec, row["faces"], row["lists"], R)
    assert np.array_equal(got, want), "%s R=%d: %d of %d covered pixels differ" % (what, R, (got != want).any(axis=2).sum(), (want[:, :, 3] == 255).sum())
    wpad = oracle.dilate_pad(want, 25)
    assert np.array_equal(p.bake_texture(vrec, row["faces"], row["lists"], R, pad_ksize=25), wpad), "%s R=%d: padded atlas differs" % (what, R)
    return want


@pytest.mark.parametrize("name", ROW_NAMES)
def test_row_matches_oracle(pkg, oracle, name):
    row = ROWS[name]
    for ctype in row["types"]:
        src = cloud_as(row, ctype)
        row["reach"](face_reports(oracle, row, ctype))
        with pkg.PointsTransfer(device=0, k_hint=row["k"]) as p:
            _resident(pkg, p, src, row["rgb"], ctype)
            for R in row["R"]:
                want = _compare(pkg, oracle, p, row, src, R, "%s %s" % (name, ctype))
                if R >= 16:                                   # (at R = 1, 2 the row j = R clamps to y = R - 1 and a face may cover nothing)
                    assert (want[:, :, 3] == 255).any() == (len(row["faces"]) > 0)


@pytest.mark.parametrize("ctype", ["f32", "f64"])
def test_all_rows_as_one_mesh(pkg, oracle, ctype):
    """every row's faces in ONE call, each row in its own UV cell: waves on different paths share workgroups (four faces each, whole
    waves leave early, no workgroup barrier) and the last workgroup is not full"""
    row = merged(list(ROWS.values()))
    assert len(row["faces"]) > 70 and len(row["faces"]) % 4 != 0
    src = cloud_as(row, ctype)
    with pkg.PointsTransfer(device=0, k_hint=32) as p:
        _resident(pkg, p, src, row["rgb"], ctype)
        want = _compare(pkg, oracle, p, row, src, 640, "merged " + ctype)
    assert (want[:, :, 3] == 255).mean() > 0.15


@pytest.mark.parametrize("case", range(int(os.environ.get("PT_STRESS_BAKE_CASES", "16"))))
def test_random_faces_match_oracle(pkg, oracle, case):
    """random rotation, face shape, lists (0..96 interior points among outside ones, missing entries, duplicates), k, R and cloud type"""
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
        if len(ids) and rng.random() < 0.5:                                   # duplicates: some free slots repeat listed points
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
    src = cloud_as(row, ctype)
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        _resident(pkg, p, src, row["rgb"], ctype)
        _compare(pkg, oracle, p, row, src, R, "case %d: k=%d nf=%d %s" % (case, k, nf, ctype))
