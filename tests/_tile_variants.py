"""Every compiled instantiation of the LDS tile kernel and how a query reaches it (shared by the CPU and GPU suites).

csrc/pt_knn_tile.hip, pt_launch_knn_tile, launches knn_tile_kernel<K, CAP, TWG, WIDE, BLEND, DBL, KC, BND>; csrc/pt_tile_route.h decides
K, CAP, TWG, WIDE and KC (expected_route below says the same in Python).  Which one runs depends on
  - k: K (the list width) and KC (the pass-1 chain) of the k bucket;
  - the geometry: small (512 threads, k <= 16), medium (384 threads, k in 17..24), large (768 threads), wide (512 threads, k in 25..32,
    whatever the geometry).  pt_set_param("tile", 2) asks for small / medium, ("tile", 3) for large;
  - BLEND: a fused query + blend (pt_query_blend_resident);
  - DBL: an fp64 cloud (fp32 shadow in LDS, exact records in pass 3);
  - BND: per-target bounds (pt_stream_query's chunks) and / or the max_dist cap.  A fused query takes the bounded variant through the
    cap only, and the bounded medium geometry is launched only under the cap (uncapped streamed chunks keep the large one).
A small or medium launch hands the blocks over its budget to a second launch of the LARGE instantiation with the same BLEND / DBL / BND
over a list of those blocks (the retry).  The table below has one row per instantiation; test_boundary checks it against the
instantiations the compiler emitted, test_gpu_tile_variants runs every row and checks that the row's instantiation answered."""

CAP_SMALL_8, CAP_SMALL_16, CAP_LARGE, CAP_WIDE = 4400, 3888, 8448, 8960           # PT_TILE_CAP_* (csrc/pt_tile_route.h)

# The launcher's geometry cells: (geometry, K, CAP, TWG, WIDE, KC, k values to run: first, middle, last of the bucket)
_SMALL = [("small", 8, CAP_SMALL_8, 512, False, 8, (1, 5, 8)), ("small", 16, CAP_SMALL_16, 512, False, 16, (9, 13, 16))]
_MEDIUM = [("medium", 32, CAP_SMALL_16, 384, False, 20, (17, 20)), ("medium", 32, CAP_SMALL_16, 384, False, 24, (21, 24))]
_LARGE = [("large", 8, CAP_LARGE, 768, False, 8, (1, 5, 8)), ("large", 16, CAP_LARGE, 768, False, 16, (9, 13, 16)),
          ("large", 32, CAP_LARGE, 768, False, 20, (17, 20)), ("large", 32, CAP_LARGE, 768, False, 24, (21, 24))]
_WIDE = [("wide", 32, CAP_WIDE, 512, True, 32, (25, 28, 32))]
_TILE_PARAM = {"small": 2, "medium": 2, "large": 3, "wide": 3}

# streamed chunks (per-target bounds) cost a build per chunk: those rows run the last k of their bucket (and 28 in the wide one)
_STREAM_KS = {8: (8,), 16: (16,), 20: (20,), 24: (24,), 32: (28, 32)}


def _rows():
    rows = []
    for bnd in (False, True):
        for geo, K, cap, twg, wide, kc, ks in _SMALL + _MEDIUM + _LARGE + _WIDE:
            for dbl in (False, True):
                for blend in (False, True):
                    if not bnd:
                        bound = "none"
                    elif blend or geo in ("small", "medium"):
                        bound = "cap"               # fused bounded variants: the cap only; bounded medium: the cap only; small: either
                    else:
                        bound = "stream"
                    rows.append(dict(K=K, CAP=cap, TWG=twg, WIDE=wide, BLEND=blend, DBL=dbl, KC=kc, BND=bnd, geometry=geo,
                                     tile=_TILE_PARAM[geo], ks=_STREAM_KS[kc] if bound == "stream" else ks,
                                     dtype="f64" if dbl else "f32", fused=blend, bound=bound, retry=geo in ("small", "medium")))
    for r in rows:
        r["id"] = "%s-K%d-KC%d-%s-%s-%s" % (r["geometry"], r["K"], r["KC"], r["dtype"], "blend" if r["BLEND"] else "plain", r["bound"])
    return rows


ROWS = _rows()


def expected_route(k, geometry, bound):
    """(K, CAP, TWG, WIDE, KC) of the launch that answers k neighbours when the caller asks for `geometry` ("large", "small", "medium")
    with bound "none", "stream" (per-target bounds without a cap) or "cap", read off ROWS: k in 25..32 runs the wide row whatever is
    asked for; the geometry asked for runs if it has a row for k; everything else runs the large one.  One exception: the BOUNDED
    medium geometry is launched only under a cap -- uncapped streamed chunks keep the large geometry they always had."""
    kc = min(r["KC"] for r in ROWS if k <= r["KC"])           # the k buckets end at the KC values: 8, 16, 20, 24, 32
    if geometry == "medium" and bound == "stream":
        geometry = "large"
    for geo in ("wide", geometry, "large"):
        for r in ROWS:
            if r["geometry"] == geo and r["KC"] == kc:
                return (r["K"], r["CAP"], r["TWG"], r["WIDE"], r["KC"])
    raise ValueError("no row for k = %d" % k)


def instantiation(row):
    """(K, CAP, TWG, WIDE, BLEND, DBL, KC, BND) -- the template arguments, in knn_tile_kernel's order"""
    return (row["K"], row["CAP"], row["TWG"], row["WIDE"], row["BLEND"], row["DBL"], row["KC"], row["BND"])


def code(K, TWG, WIDE, BLEND, DBL, KC, BND, listed=False):
    """pt_stats_t::tile_variant of a launch (pt_tile_code, csrc/pt_tile_route.h)"""
    return K | KC << 6 | (TWG // 64) << 12 | int(WIDE) << 16 | int(BLEND) << 17 | int(DBL) << 18 | int(BND) << 19 | int(listed) << 20


def row_code(row, listed=False):
    return code(row["K"], row["TWG"], row["WIDE"], row["BLEND"], row["DBL"], row["KC"], row["BND"], listed)


def retry_code(row):
    """the retry launch of a small / medium row: the large instantiation of its k bucket, over a block list"""
    K, KC = row["K"], row["KC"]
    return code(K, 768, False, row["BLEND"], row["DBL"], KC, row["BND"], listed=True)


def decode(c):
    return dict(K=c & 63, KC=(c >> 6) & 63, TWG=((c >> 12) & 15) * 64, WIDE=bool(c >> 16 & 1), BLEND=bool(c >> 17 & 1), DBL=bool(c >> 18 & 1),
                BND=bool(c >> 19 & 1), listed=bool(c >> 20 & 1))
