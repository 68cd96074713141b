"""Small textured-mesh cases for the texture-bake tests (shared by the CPU and GPU suites)."""
import numpy as np


def make_case(seed, n=6000, grid=6, k=20, jitter=0.02, degenerate=False):
    """A bumpy height-field cloud over the unit square and a (grid x grid x 2)-triangle mesh under it, UV = xy scaled into
    (0.05, 0.95).  Returns (src_xyz (3,n) f64, src_rgb (n,3) u8, vert POINT_DTYPE-like dict, faces (F,3) i32)."""
    rng = np.random.default_rng(seed)
    x = rng.random(n); y = rng.random(n)
    z = 0.1 * np.sin(5 * x) * np.cos(4 * y) + jitter * rng.standard_normal(n)
    src = np.stack([x, y, z])
    if degenerate:                                   # exact duplicates and points exactly on mesh vertices / edges
        src[:, 1::7] = src[:, 0:-1:7][:, : src[:, 1::7].shape[1]]
    rgb = rng.integers(0, 256, size=(n, 3), dtype=np.uint8)
    g = np.linspace(0.0, 1.0, grid + 1)
    vx, vy = np.meshgrid(g, g, indexing="xy")
    vx = vx.ravel(); vy = vy.ravel()
    vz = 0.1 * np.sin(5 * vx) * np.cos(4 * vy)
    verts = np.stack([vx, vy, vz])
    if degenerate:
        src[:, :verts.shape[1]] = verts             # cloud points exactly on the mesh vertices
    uv = np.stack([0.05 + 0.9 * vx, 0.05 + 0.9 * vy], axis=1)
    vrgb = rng.integers(0, 256, size=(verts.shape[1], 3), dtype=np.uint8)
    faces = []
    for j in range(grid):
        for i in range(grid):
            a = j * (grid + 1) + i
            faces.append([a, a + 1, a + grid + 2]); faces.append([a, a + grid + 2, a + grid + 1])
    faces = np.array(faces, np.int32)
    if degenerate:
        faces = np.vstack([faces, [[0, 0, 1]], [[2, 2, 2]]]).astype(np.int32)        # zero-area faces
    return src, rgb, verts, uv, vrgb, faces


def point_records(dtype, xyz, rgb, uv=None):
    """reference Point records (80 B) from planar xyz, colours and optional UVs"""
    n = xyz.shape[1]
    a = np.zeros(n, dtype=dtype)
    a["ver"] = np.ascontiguousarray(xyz.T)
    a["color"] = rgb.astype(np.int32)
    if uv is not None:
        a["U"] = uv[:, 0]; a["V"] = uv[:, 1]
    return a


# ---- rows that reach the bake's kernel paths one by one (tests/test_bake_oracle.py on the CPU, tests/test_gpu_bake_paths.py on the GPU) ----
# Every row is a tiny mesh with CALLER-SUPPLIED neighbour lists (a k-NN query of the corners only ever keeps the wedge of each corner's
# disc that lies inside the face: a few dozen points at most).  `reach` is asserted on the oracle's per-face reports.
NOIDX = 0xFFFFFFFF
ROW_NAMES = ("full99", "upper_half", "np67", "np66", "lattice_cap", "cap_edge", "tilted_px", "tilted_nx", "tilted_py", "tilted_ny", "tilted_nz",
             "tilted_rand", "mirrored_uv", "sliver", "stacked", "collinear", "overlap", "big", "uv_edge", "uv_bad", "verts_bad", "colours",
             "ids_k1", "ids_k32", "nf0", "malformed")
UNIT = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])          # the axis-aligned unit right triangle: images are (x, y) exactly
# 1/16-lattice points strictly inside UNIT, in (i, j) order: the first 96 of the 105
LATTICE = [(i, j) for i in range(1, 16) for j in range(1, 16) if i + j < 16]
# LATTICE[:96] without the listed positions: subsets whose uncapped number of empty-circle triples is exactly 255 / 256 (found by a seeded search on the CPU)
CAP_255 = [i for i in range(96) if i not in (8, 9, 16, 36, 37, 39, 55, 57, 58, 61, 64, 73, 85, 89)]
CAP_256 = [i for i in range(96) if i not in (1, 8, 11, 23, 26, 39, 40, 47, 58, 69, 70, 75, 77, 78, 79, 80, 86, 92)]


class _Mesh:
    """collects faces that each own their three vertices, a UV window per face and one cloud"""
    def __init__(self, k, windows):
        self.k, self.w, self.g = k, 0, int(np.ceil(np.sqrt(windows)))
        self.verts, self.uv, self.vrgb, self.lists, self.faces, self.pts, self.rgb = [], [], [], [], [], [], []

    def window(self):
        """the next cell of a g x g grid over the unit square, as a UV triangle a little inside it (different margins per axis)"""
        s = 1.0 / self.g
        ox, oy = (self.w % self.g) * s, (self.w // self.g) * s
        self.w += 1
        return np.array([[ox + 0.03 * s, oy + 0.04 * s], [ox + 0.97 * s, oy + 0.05 * s], [ox + 0.06 * s, oy + 0.95 * s]])

    def cloud(self, xyz, rgb=None):
        """append points (m, 3); returns their indices"""
        i0 = len(self.pts)
        self.pts.extend(np.asarray(xyz, np.float64).reshape(-1, 3))
        m = len(self.pts) - i0
        self.rgb.extend(rgb if rgb is not None else [((37 * i + 11) % 256, (91 * i + 5) % 256, (53 * i + 200) % 256) for i in range(i0, i0 + m)])
        return np.arange(i0, i0 + m, dtype=np.uint32)

    def face(self, corners, ids, uv=None, vrgb=None, order=(0, 1, 2), rng=None):
        """a face on three new vertices; `ids` (any length <= 3 k) are dealt over the three corners' lists, the rest is NOIDX"""
        v0 = len(self.verts)
        self.verts.extend(np.asarray(corners, np.float64).reshape(3, 3))
        self.uv.extend(self.window() if uv is None else np.asarray(uv, np.float64).reshape(3, 2))
        self.vrgb.extend(vrgb if vrgb is not None else [[250, 40, 30], [20, 240, 60], [10, 50, 230]])
        ids = np.asarray(ids, np.uint32)
        assert len(ids) <= 3 * self.k
        if rng is not None:
            ids = rng.permutation(ids)
        full = np.full(3 * self.k, NOIDX, np.uint32)
        full[:len(ids)] = ids
        self.lists.extend(full.reshape(self.k, 3).T)            # dealt round-robin: each corner's list holds a third
        self.faces.append([v0 + order[0], v0 + order[1], v0 + order[2]])
        return v0

    def row(self, name, R, types, tri, reach, **extra):
        n = max(len(self.pts), 1)
        src = np.zeros((3, n)); rgb = np.zeros((n, 3), np.uint8)
        if self.pts:
            src = np.ascontiguousarray(np.array(self.pts).T); rgb = np.array(self.rgb, np.uint8).reshape(n, 3)
        nv = len(self.verts)
        d = dict(name=name, src=src, rgb=rgb, verts=np.ascontiguousarray(np.array(self.verts).reshape(nv, 3).T), uv=np.array(self.uv).reshape(nv, 2),
                 vrgb=np.array(self.vrgb, np.int64).reshape(nv, 3).astype(np.int32), faces=np.array(self.faces, np.int32).reshape(-1, 3),
                 lists=np.array(self.lists, np.uint32).reshape(nv, self.k), k=self.k, R=tuple(R), types=tuple(types), tri=tri, reach=reach)
        d.update(extra)
        return d


def cloud_as(row, ctype):
    """the row's cloud as the GPU holds it for that cloud type ("f32", "f64", "f16"), in float64"""
    t = {"f32": np.float32, "f64": np.float64, "f16": np.float16}[ctype]
    with np.errstate(over="ignore"):
        return row["src"].astype(t).astype(np.float64)


def _interior(rng, m, corners=UNIT, lift=0.01, margin=0.02):
    """m random points inside the triangle (barycentrics >= margin), lifted off its plane by lift * N(0, 1) * |edge|"""
    c = np.asarray(corners, np.float64)
    b = margin + (1.0 - 3.0 * margin) * rng.dirichlet([1, 1, 1], m)
    nrm = np.cross(c[1] - c[0], c[2] - c[0])
    ln = np.linalg.norm(nrm)
    nrm = nrm / ln if ln > 0 else nrm
    return b @ c + (lift * np.linalg.norm(c[1] - c[0])) * rng.standard_normal((m, 1)) * nrm


def _outside(rng, m, corners=UNIT):
    """m random points whose projection is outside the triangle (one barycentric <= -0.1)"""
    c = np.asarray(corners, np.float64)
    b = rng.dirichlet([1, 1, 1], m) * 1.6
    b[:, 0] = -0.1 - 0.5 * rng.random(m)
    b[:, 2] = 1.0 - b[:, 0] - b[:, 1]
    return b @ c


def _rot(seed):
    q = np.random.default_rng(seed).standard_normal(4); q /= np.linalg.norm(q); a, b, c, d = q
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)], [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


def _lattice_xyz(pairs, z=0.0):
    return np.array([[i / 16.0, j / 16.0, z] for i, j in pairs])


def _all(reps, **want):
    for r in reps:
        for key, v in want.items():
            assert r[key] == v, (key, r[key], v)


def make_face_cases():
    """The rows of the table in DESIGN.md section 8 ("Checked instead"), in ROW_NAMES order.  Each is a dict: name, src (3, n) f64,
    rgb (n, 3) u8, verts (3, nv), uv (nv, 2), vrgb (nv, 3) int32 (as the 80-byte records hold them: may lie outside 0..255), faces, lists
    (nv, k) u32, k, R (resolutions), types (cloud types to run), tri ("scipy": general position, checked; "exact": lattice data) and
    reach(reports): asserts on the oracle's per-face reports that the row takes the path it is there for."""
    rows = []

    def general(name, seed, n_in, n_out=0, k=32, types=("f32", "f64"), front_outside=False, reach=None, R=(256,)):
        rng = np.random.default_rng(seed)
        m = _Mesh(k, 1)
        if front_outside:                      # ascending index = sorted order: the first n_out candidates are the outside ones
            out_ids = m.cloud(_outside(rng, n_out)); in_ids = m.cloud(_interior(rng, n_in))
            ids = np.concatenate([out_ids, in_ids])
        else:                                  # outside points scattered through the index range
            xyz = np.concatenate([_interior(rng, n_in), _outside(rng, n_out)])
            ids = m.cloud(xyz[rng.permutation(len(xyz))])
        m.face(UNIT, ids, rng=rng)
        rows.append(m.row(name, R, types, "scipy", reach))

    general("full99", 11, 96, types=("f32", "f64", "f16"), reach=lambda r: _all(r, nid=96, np=99, ntri_all=193))

    def upper(r):
        _all(r, nid=96, np=35)
        assert (r[0]["ids"][3:] >= 64).all()                                # every kept point is one of candidates 64..95 (h = 1)
    general("upper_half", 12, 32, 64, front_outside=True, reach=upper)
    general("np67", 13, 64, 32, reach=lambda r: _all(r, nid=96, np=67))      # kb = 66 holds lane 0 alone
    general("np66", 14, 63, 33, reach=lambda r: _all(r, nid=96, np=66))      # the kb loop ends after one chunk

    m = _Mesh(32, 1)
    m.face(UNIT, m.cloud(_lattice_xyz(LATTICE[:96])), rng=np.random.default_rng(15))

    def cap(r):
        _all(r, nid=96, np=99, ntri=255)
        assert r[0]["ntri_all"] > 255
    rows.append(m.row("lattice_cap", (256,), ("f32", "f64", "f16"), "exact", cap))

    m = _Mesh(32, 2)
    for sub in (CAP_255, CAP_256):
        m.face(UNIT, m.cloud(_lattice_xyz([LATTICE[i] for i in sub])), rng=np.random.default_rng(16))

    def edge(r):
        assert (r[0]["ntri_all"], r[0]["ntri"]) == (255, 255) and (r[1]["ntri_all"], r[1]["ntri"]) == (256, 255)
    rows.append(m.row("cap_edge", (256,), ("f32",), "exact", edge))

    # full99 under rotations: z -> +x, -x, +y, -y, -z (signed permutations, det +1) and one seeded rotation; three corner orders each
    perm = dict(px=[[0, 0, 1], [0, 1, 0], [-1, 0, 0]], nx=[[0, 0, -1], [0, 1, 0], [1, 0, 0]], py=[[1, 0, 0], [0, 0, 1], [0, -1, 0]],
                ny=[[1, 0, 0], [0, 0, -1], [0, 1, 0]], nz=[[1, 0, 0], [0, -1, 0], [0, 0, -1]], rand=_rot(23))
    for s, (tag, M) in enumerate(perm.items()):
        M = np.array(M, np.float64)
        assert abs(np.linalg.det(M) - 1.0) < 1e-12
        rng = np.random.default_rng(30 + s)
        shift = np.array([3.0, -2.0, 5.0])
        m = _Mesh(32, 3)
        for order in ((0, 1, 2), (1, 2, 0), (0, 2, 1)):
            m.face(UNIT @ M.T + shift, m.cloud(_interior(rng, 96) @ M.T + shift), order=order, rng=rng)
        rows.append(m.row("tilted_" + tag, (256,), ("f32", "f64"), "scipy", lambda r: _all(r, nid=96, np=99, ntri_all=193),
                          normal=M @ np.array([0.0, 0.0, 1.0])))

    rng = np.random.default_rng(40)
    m = _Mesh(32, 1)
    w = m.window()
    m.face(UNIT, m.cloud(_interior(rng, 60)), uv=w[[0, 2, 1]], rng=rng)        # UV triangle of negative area
    rows.append(m.row("mirrored_uv", (256,), ("f32", "f64"), "scipy", lambda r: _all(r, np=63), uv_area_negative=True))

    rng = np.random.default_rng(41)
    m = _Mesh(8, 3)
    for corners in (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 1e-4, 0.0]]),               # aspect 1e4
                    UNIT @ _rot(42).T * 1.4e-6,                                                    # area ~ 1e-12
                    UNIT @ _rot(43).T + np.array([1e6, -1e6, 1e6])):                               # far from the origin
        m.face(corners, m.cloud(_interior(rng, 12, corners, margin=0.05)), rng=rng)

    def sliver(r):
        _all(r, frame_ok=True, np=15)
        assert all(np.isfinite(x["xy"]).all() for x in r)
    rows.append(m.row("sliver", (256,), ("f64",), "scipy", sliver))

    m = _Mesh(16, 2)
    col = [(4, 4), (4, 4), (4, 4), (2, 9), (2, 9)]                             # two stacks along the normal ...
    a = m.cloud(np.array([[i / 16.0, j / 16.0, 0.25 * s - 0.5] for s, (i, j) in enumerate(col)]))
    b = m.cloud(_lattice_xyz([(0, 0), (16, 0), (0, 16), (8, 0), (0, 5), (8, 8), (3, 13), (6, 3), (1, 1)]))   # ... the corners, the edges, three plain
    m.face(UNIT, np.concatenate([a, b]))
    m.face(UNIT, np.concatenate([b, a])[::-1].copy())
    rows.append(m.row("stacked", (128,), ("f32", "f64", "f16"), "exact", lambda r: _all(r, nid=14, ninside=14, np=11)))   # 3 of 5 stacked and the 3 corner points go

    m = _Mesh(4, 2)
    m.face(UNIT, m.cloud(_lattice_xyz([(2 * i, i) for i in range(1, 6)])))      # on the line y = x / 2 through corner 0
    m.face(UNIT, m.cloud(_lattice_xyz([(16 - 2 * i, i) for i in range(1, 8)])))   # on a line through corner 1, up to the far edge
    rows.append(m.row("collinear", (128,), ("f32", "f64"), "exact", lambda r: (_all(r[:1], np=8), _all(r[1:], np=10))))

    rng = np.random.default_rng(44)
    m = _Mesh(16, 2)
    w = m.window()
    m.face(UNIT, m.cloud(_interior(rng, 30)), uv=w, rng=rng)
    m.face(UNIT, m.cloud(_interior(rng, 40)), uv=w, rng=rng)                   # same UV triangle, another list: the later face shows
    m.face(UNIT, m.cloud(_interior(rng, 20)), rng=rng)
    m.faces.append(list(m.faces[-1])); m.faces.append(list(m.faces[0]))        # the same faces again, one of them over the two others
    rows.append(m.row("overlap", (256,), ("f32",), "scipy", lambda r: (_all(r[:1], np=33), _all(r[1:2], np=43))))

    rng = np.random.default_rng(45)
    m = _Mesh(8, 1)
    m.face(UNIT, m.cloud(_interior(rng, 20)), uv=[[-0.5, -0.4], [2.6, -0.5], [-0.45, 2.5]], rng=rng)
    rows.append(m.row("big", (1, 2, 63, 64, 65, 1000), ("f32",), "scipy", lambda r: _all(r, np=23), covers_atlas=True))

    m = _Mesh(8, 2)                                                            # R = 64, UV = k / 16: every U R, V R is an integer
    sq = np.array([[1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
    m.face(UNIT, m.cloud(_lattice_xyz([(4, 4), (8, 4), (4, 8), (2, 2), (8, 8), (12, 2), (2, 12), (6, 5)])), uv=UNIT[:, :2])
    m.face(sq, m.cloud(_lattice_xyz([(12, 12), (8, 12), (12, 8), (14, 14), (8, 8), (15, 5), (10, 11)])), uv=sq[:, :2])
    rows.append(m.row("uv_edge", (64, 16), ("f32", "f64", "f16"), "exact", lambda r: (_all(r[:1], np=11), _all(r[1:], np=10))))

    rng = np.random.default_rng(46)
    m = _Mesh(4, 9)
    good = m.window()
    big = 2.0 ** 31 / 64.0
    for uv in (good, np.full((3, 2), np.nan), good + [[np.inf, 0]] * 3, good - [[0, np.inf]] * 3, good + 1e10, np.vstack([good[:2], [[1e10, 0.5]]]),
               good + [[big + 0.5, 0.0]] * 3, good - [[0.0, big + 0.5]] * 3, m.window()):
        m.face(UNIT, m.cloud(_interior(rng, 6)), uv=uv, rng=rng)
    rows.append(m.row("uv_bad", (64,), ("f32",), "scipy", lambda r: _all(r, np=9)))

    rng = np.random.default_rng(47)
    m = _Mesh(4, 8)
    nanv = UNIT.copy(); nanv[2, 1] = np.nan
    infv = UNIT.copy(); infv[1, 0] = np.inf
    bad = (nanv, infv, UNIT[[0, 0, 2]], np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]]), UNIT * 1e200, UNIT * 1e-200)
    for corners in (UNIT,) + bad + (UNIT,):
        m.face(corners, m.cloud(_interior(rng, 6)), rng=rng)

    def verts_bad(r):
        _all(r[:1] + r[-1:], frame_ok=True, np=9)
        _all(r[1:-1], frame_ok=False, np=3, nid=6)
    rows.append(m.row("verts_bad", (128,), ("f64",), "scipy", verts_bad))

    rng = np.random.default_rng(48)
    m = _Mesh(4, 2)
    imin, imax = -2 ** 31, 2 ** 31 - 1
    m.face(UNIT, [], vrgb=[[-7, 300, imin], [imax, 128, -1], [256, 0, 255]])                       # the plain face mixes the corner colours
    m.face(UNIT, m.cloud(_interior(rng, 6)), vrgb=[[imin, imax, 300], [-7, -7, 1000], [255, 256, 254]], rng=rng)
    rows.append(m.row("colours", (128,), ("f32",), "scipy", lambda r: (_all(r[:1], np=3), _all(r[1:], np=9)), colours_out_of_range=True))

    for k in (1, 32):
        rng = np.random.default_rng(49 + k)
        m = _Mesh(k, 6)
        per = min(3 * k, 30)
        for f in range(6):
            m.face(UNIT, m.cloud(_interior(rng, per)), rng=rng)
        L = np.array(m.lists, np.uint32).reshape(18, k)
        n = len(m.pts)
        L[0, 0] = n; L[1, 0] = n + 12345                                        # face 0: indices >= n
        L[3:6, ::2] = NOIDX                                                    # face 1: NOIDX scattered through the lists
        L[6] = NOIDX                                                           # face 2: one corner's list missing
        L[9:12] = NOIDX                                                        # face 3: all three missing
        L[12] = L[12, 0]; L[13, k // 2:] = L[14, :k - k // 2]                   # face 4: duplicates within a list and across corners
        m.lists = list(L)

        def ids(r, L=L, n=n, per=per):
            for f in range(6):
                u = np.unique(L[3 * f:3 * f + 3])
                assert r[f]["nid"] == (u < n).sum()
            assert r[3]["np"] == 3 and r[5]["np"] == 3 + per
        rows.append(m.row("ids_k%d" % k, (128,), ("f32", "f64"), "scipy", ids))

    m = _Mesh(4, 1)
    m.face(UNIT, m.cloud(_interior(np.random.default_rng(60), 6)))
    m.faces = []
    rows.append(m.row("nf0", (64,), ("f32",), "scipy", lambda r: None))

    rng = np.random.default_rng(61)
    m = _Mesh(8, 4)
    for f in range(3):
        m.face(UNIT, m.cloud(_interior(rng, 12)), rng=rng)
    m.faces = [m.faces[0], [0, -1, 2], m.faces[1], [3, 4, 9], [2 ** 31 - 1, 0, 1], m.faces[2], [-2 ** 31, 1, 2]]

    def malformed(r):
        assert [x["valid"] for x in r] == [True, False, True, False, False, True, False]
        _all(r[:1] + r[2:3] + r[5:6], np=15)
    rows.append(m.row("malformed", (128,), ("f32",), "scipy", malformed))

    assert tuple(r["name"] for r in rows) == ROW_NAMES
    return rows


def face_reports(oracle, row, ctype):
    """the oracle's report of every face of the row, for the cloud as that cloud type holds it"""
    src = cloud_as(row, ctype)
    vrgb = np.clip(row["vrgb"], 0, 255).astype(np.uint8)
    return [oracle.bake_face_report(src, row["rgb"], row["verts"], row["uv"], vrgb, row["faces"], row["lists"], f) for f in range(len(row["faces"]))]


def merged(rows):
    """All rows' faces as ONE mesh over ONE cloud, k = 32: each row's UVs are mapped into its own cell of a grid over the unit square,
    indices are shifted, lists padded with NOIDX; out-of-range vertex and cloud indices stay out of range.  A row that covers the whole
    atlas (covers_atlas) would cover the other rows' cells and is left out."""
    rows = [r for r in rows if not r.get("covers_atlas")]
    g = int(np.ceil(np.sqrt(len(rows))))
    src, rgb, verts, uv, vrgb, faces, lists = [], [], [], [], [], [], []
    n0 = nv0 = 0
    n_all = sum(r["src"].shape[1] for r in rows); nv_all = sum(r["verts"].shape[1] for r in rows)
    for w, r in enumerate(rows):
        n, nv = r["src"].shape[1], r["verts"].shape[1]
        src.append(r["src"]); rgb.append(r["rgb"]); verts.append(r["verts"]); vrgb.append(r["vrgb"])
        with np.errstate(invalid="ignore"):
            uv.append(np.array([w % g, w // g]) / g + r["uv"] / g)
        f = r["faces"].astype(np.int64)
        faces.append(np.where(f < 0, f, np.where(f >= nv, nv_all + 7, f + nv0)))
        L = r["lists"].astype(np.int64)
        full = np.full((nv, 32), NOIDX, np.int64)
        full[:, :r["k"]] = np.where(L < n, L + n0, np.where(L == NOIDX, NOIDX, n_all + 5))
        lists.append(full.astype(np.uint32))
        n0 += n; nv0 += nv
    return dict(name="merged", src=np.concatenate(src, axis=1), rgb=np.concatenate(rgb), verts=np.concatenate(verts, axis=1), uv=np.concatenate(uv),
                vrgb=np.concatenate(vrgb), faces=np.concatenate(faces).astype(np.int32), lists=np.concatenate(lists), k=32)
