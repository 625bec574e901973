"""The oracle (CPU restatement, oracle/ort_oracle.c) against the golden vectors produced by
the reference's own code (tests/golden/make_golden.py).  Bit-exact everywhere: this is what
pins the oracle.  CPU only."""
import os

import numpy as np
import pytest

import ref_io
from conftest import GOLDEN, ROOT, assert_bits_equal

SCENES = ["testscene", "c2_analytic", "c3_bunny_room", "c4_dwarf_room", "letters", "glass_room", "rand_a", "rand_b"]
# + the 99 458-triangle decimation of BASELINE.json's synthetic-mesh config (generated, see conftest.load_scene)
SCENES_C5 = SCENES + ["c5_heightfield_224"]


@pytest.mark.parametrize("seed", [12345, 1, 4294967295, 2463534242])
def test_rng_streams(oracle, seed):
    """random.h:5-117: xorshift (13,17,>>5), rng_01, random_between (two steps), %, spherical."""
    want = open(os.path.join(GOLDEN, "rng_%d.bin" % seed), "rb").read()
    assert oracle.rng_table(seed, 64) == want


def test_rng_survey_crosscheck(oracle):
    """start_random_series(12345) -> 104278947, 3831047122, 3324124125, 2171811514."""
    tab = np.frombuffer(oracle.rng_table(12345, 4)[:32], dtype="<u4")
    assert list(tab[0::2]) == [104278947, 3831047122, 3324124125, 2171811514]


def test_unit_tables(oracle):
    """every intersector and BSDF function, input -> output, against the reference build."""
    z = np.load(os.path.join(GOLDEN, "unit_tables.npz"))
    recs = z["records"].view(ref_io.UNIT_REC_DTYPE).reshape(-1)
    got = oracle.unit_batch(recs)
    want = z["ref_det"]
    for op in np.unique(recs["op"]):
        sel = recs["op"] == op
        assert_bits_equal(got[sel], want[sel], "unit op %d" % op)


def test_unit_edges(oracle):
    """the corner sets of tests/unit_cases.py (+-0 and NaN slab products, tangent bands, radicands of exactly 0, normals
    in the 1e-4 band around +-z, quadrant boundaries, ...) for ops 1-11, against the reference build (unit_edges.npz).
    Bit for bit; a NaN matches any NaN."""
    import unit_cases
    z = np.load(os.path.join(GOLDEN, "unit_edges.npz"))
    recs = z["records"].view(ref_io.UNIT_REC_DTYPE).reshape(-1)
    assert sorted(np.unique(recs["op"])) == list(range(1, 12))
    got = oracle.unit_batch(recs)
    for op in range(1, 12):
        sel = recs["op"] == op
        unit_cases.assert_match(got[sel], z["ref_det"][sel], recs["a"][sel], "oracle op %d vs the reference" % op)


def test_unit_edges_are_the_generators_corner_sets():
    """unit_edges.npz holds exactly what tests/unit_cases.py makes today (a changed generator needs new fixtures:
    make_golden.py --only-unit-edges)"""
    import unit_cases
    z = np.load(os.path.join(GOLDEN, "unit_edges.npz"))
    recs = z["records"].view(ref_io.UNIT_REC_DTYPE).reshape(-1)
    want = np.concatenate([unit_cases.records(op, unit_cases.corners(op)) for op in range(1, 12)])
    assert recs.tobytes() == want.tobytes()


def test_libm_is_close_to_glibc():
    """the deterministic libm is within 1 ulp of glibc on the path's argument ranges (documents
    the distance between the bit-exact anchor and the as-shipped build)."""
    z = np.load(os.path.join(GOLDEN, "unit_tables.npz"))
    recs = z["records"].view(ref_io.UNIT_REC_DTYPE).reshape(-1)
    sel = recs["op"] == 9
    a, b = z["ref_det"][sel][:, :5], z["ref_glibc"][sel][:, :5]
    both_nan = np.isnan(a) & np.isnan(b)
    ia = a.view("<i4").astype(np.int64)
    ib = b.view("<i4").astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    ulp = np.abs(ia - ib)
    ulp[both_nan] = 0
    finite = np.isfinite(a) & np.isfinite(b)
    assert (np.isnan(a) == np.isnan(b)).all()
    assert ulp[finite].max() <= 1


@pytest.mark.parametrize("name", SCENES_C5)
def test_octree_matches_reference(oracle, manifest, name, load_scene):
    """the restated loose octree (ray.cpp:1468-2045) has the reference's node/leaf/byte counts."""
    flat = load_scene(name).flatten(64, 48)
    st = oracle.OracleScene(flat).tree_stats()
    want = manifest["scenes"][name]["octree"]
    assert st["nodes"] == want["octree_nodes"]
    assert st["nonempty_leaves"] == want["octree_leaves"]
    assert st["record_bytes"] == want["record_bytes"]


@pytest.mark.parametrize("name", SCENES_C5)
def test_renders_match_reference(oracle, manifest, name, load_scene):
    """full renders in every seeding policy: image bits, shapes-tested counter, final RNG state."""
    z = np.load(os.path.join(GOLDEN, "renders_%s.npz" % name))
    entries = [e for e in manifest["renders"] if e["scene"] == name]
    assert entries
    scene = load_scene(name)
    for e in entries:
        osc = oracle.OracleScene(scene.flatten(e["width"], e["height"]))
        img, st = osc.render(e["width"], e["height"], e["spp"], e["seed"], e["policy"], chunk=e["chunk"], threads=1)
        assert_bits_equal(img, z[e["key"]], "%s %s" % (name, e["key"]))
        assert st["shapes_tested"] == e["shapes_tested"], e["key"]
        if e["policy"] != "tile32":
            assert st["final_rng"] == e["final_rng"], e["key"]


def test_render_is_thread_count_independent(oracle, load_scene):
    osc = oracle.OracleScene(load_scene("c2_analytic").flatten(40, 30))
    a, _ = osc.render(40, 30, 4, 5, "chunk", chunk=2, threads=1)
    b, _ = osc.render(40, 30, 4, 5, "chunk", chunk=2, threads=7)
    assert_bits_equal(a, b)


@pytest.mark.parametrize("name", SCENES)
def test_raycast_matches_reference(oracle, name, load_scene):
    """raycast_top_most_node (ray.cpp:1165) closest hits for 400 rays: t, normal, material."""
    z = np.load(os.path.join(GOLDEN, "raycast_%s.npz" % name))
    osc = oracle.OracleScene(load_scene(name).flatten(64, 64))
    t, n, mat = osc.raycast(z["rays"][:, 0:3], z["rays"][:, 3:6])
    assert_bits_equal(t, z["t"], "t")
    assert_bits_equal(n, z["n"], "normal")
    assert (mat == z["mat"]).all()


@pytest.mark.parametrize("name", SCENES)
def test_raycast_edges_match_reference(oracle, name, load_scene):
    """the hostile rays of tests/raycast_cases.py (non-finite, zero, extreme and grazing; raycast_edges_<scene>.npz):
    t, normal, material bit for bit, a NaN where the reference has one"""
    import raycast_cases
    z = np.load(os.path.join(GOLDEN, "raycast_edges_%s.npz" % name))
    osc = oracle.OracleScene(load_scene(name).flatten(64, 64))
    t, n, mat = osc.raycast(z["rays"][:, 0:3], z["rays"][:, 3:6])
    raycast_cases.assert_same_answers(t, n, mat, z["t"], z["n"], z["mat"], name + " oracle vs the reference")


@pytest.mark.parametrize("name", SCENES)
def test_raycast_edges_are_the_generators_rays(oracle, name, load_scene):
    """raycast_edges_<scene>.npz holds exactly what tests/raycast_cases.py makes today (a changed generator needs new
    fixtures: make_golden.py --only-raycast-edges)"""
    import raycast_cases
    z = np.load(os.path.join(GOLDEN, "raycast_edges_%s.npz" % name))
    flat = load_scene(name).flatten(64, 64)
    osc = oracle.OracleScene(flat)
    rays, cat = raycast_cases.cases(flat, lambda r: osc.raycast(r[:, 0:3], r[:, 3:6])[0])
    assert rays.tobytes() == z["rays"].tobytes()
    assert (cat == z["category"]).all()


@pytest.mark.parametrize("name", SCENES)
def test_raycast_edges_are_not_all_misses(name):
    """every category is there, and the reference hits something with non-finite, extreme, grazing and far rays: a
    fixture of misses alone would pin nothing but the miss record"""
    import raycast_cases
    z = np.load(os.path.join(GOLDEN, "raycast_edges_%s.npz" % name))
    assert len(z["rays"]) <= 2000 and len(z["t"]) == len(z["rays"])
    bits = z["rays"].view("<u4")
    hit = z["t"] < raycast_cases.FLT_MAX
    for c, what in enumerate(raycast_cases.CATEGORIES):
        sel = z["category"] == c
        assert sel.sum() >= 100, what
        if what != "zero":
            assert hit[sel].sum() >= 20, what
    nonfinite = z["category"] == raycast_cases.CATEGORIES.index("nonfinite")
    # qNaN, the negative NaN and both infinities in every component, hit or not
    for comp in range(6):
        for v in (raycast_cases.QNAN, raycast_cases.NEG_NAN, np.float32(np.inf), np.float32(-np.inf)):
            assert (bits[nonfinite, comp] == np.float32(v).view("<u4")).sum() >= 6, (comp, v)
    assert hit[nonfinite & np.isnan(z["rays"][:, 0:6]).any(axis=1)].any()
    # the zero rays: all eight sign patterns of (+-0, +-0, +-0)
    zero = z["rays"][z["category"] == raycast_cases.CATEGORIES.index("zero")]
    patterns = {tuple(r) for r in zero[:, 3:6].view("<u4") if not (r & 0x7FFFFFFF).any()}
    assert len(patterns) == 8


def test_glibc_distance_is_recorded_and_small(manifest):
    """reference + glibc libm vs reference + deterministic libm on the same seeds: almost all
    pixels bit-equal; the rest are single decorrelated paths (1/spp-sized) -- see DESIGN.md."""
    seen = 0
    for e in manifest["renders"]:
        if "glibc_distance" in e:
            d = e["glibc_distance"]
            assert d["bit_equal_fraction"] > 0.97, e["key"]
            seen += 1
    assert seen >= 6


def test_survey_crosscheck_recorded(manifest):
    """SURVEY App. C.3 values for testscene 64x64x4 seed 12345 (whole image, glibc build)."""
    c = manifest["survey_crosscheck"]
    assert c["shapes_tested"] == 8463155
    assert c["final_rng"] == 507954640
    assert c["sha256"] == "07f48b563f8d92ec10f003e607e2a98076460331fc9bdac00ea9e77e543135b4"


def test_glibc_distance_at_baseline_scale(manifest):
    """north_star's tolerance is per-pixel L2 < 1e-4 against the CPU reference.  The parity anchor is the reference with
    a deterministic libm; this pins how far that is from the reference AS SHIPPED (glibc libm) at BASELINE scale: a
    128x72 window of the 1920x1080 frame, 1024 spp in 64-sample jobs, same seeds (tools/glibc_distance_baseline.py,
    both sides = the reference's own sources compiled here).  Stated bounds: bunny room (the headline scene) and dwarf
    room: every pixel within 1e-6, > 99 % bit-equal; the analytic scene (glass, mirrors: a flipped comparison
    decorrelates a whole 64-sample job) >= 99.9 % of the pixels within 1e-4 and none beyond 1e-2."""
    b = manifest["glibc_distance_baseline"]
    for scene in ("c3_bunny_room", "c4_dwarf_room"):
        d = b[scene]
        assert (d["width"], d["height"], d["spp"], d["chunk"]) == (1920, 1080, 1024, 64) and d["pixels"] == 128 * 72
        assert d["fraction_below_1e4"] == 1.0 and d["max_l2"] < 1e-6 and d["bit_equal_fraction"] > 0.99, scene
    d = b["c2_analytic"]
    assert d["fraction_below_1e4"] >= 0.999 and d["max_l2"] < 1e-2 and d["bit_equal_fraction"] > 0.99


def _detscene(tmp_path_factory):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_detscene
    d = str(tmp_path_factory.mktemp("detscene")) + "/"
    scn, nv, nf = make_detscene.write_scene(d)
    return scn, d, nv, nf


def test_oracle_on_the_determinant_threshold_scene(api, oracle, manifest, tmp_path_factory):
    """tiny triangles whose |e1 x e2| straddles ray.cpp:95's 1e-6 and a strip seen edge-on (tools/make_detscene.py):
    the oracle equals the reference's own pixels (tests/golden/make_det_golden.py), bit for bit"""
    import hashlib
    scn, d, nv, nf = _detscene(tmp_path_factory)
    meta = manifest["detscene"]
    assert (nv, nf) == (meta["vertices"], meta["triangles"])
    assert hashlib.sha256(open(os.path.join(d, "detscene.ply"), "rb").read()).hexdigest() == meta["ply_sha256"]
    scene = api.Scene.load_scn(scn).commit()
    W, H = meta["width"], meta["height"]
    osc = oracle.OracleScene(scene.flatten(W, H))
    z = np.load(os.path.join(GOLDEN, "renders_detscene.npz"))
    for c in meta["cases"]:
        x0, y0, x1, y1 = meta["windows"][c["window"]]
        img, st = osc.render(W, H, c["spp"], c["seed"], c["policy"], chunk=c["chunk"], rect=(x0, y0, x1, y1), threads=8)
        assert_bits_equal(img[y0:y1, x0:x1], z[c["key"]], c["key"])
        assert st["shapes_tested"] == c["reference"]["shapes_tested"]


def test_oracle_equals_the_reference_at_baseline_scale(api, oracle, manifest):
    """the oracle against the reference's own pixels at BASELINE parameters (1920x1080, 1024 spp, 64-sample jobs): a 16x8
    corner of each fixture window (tests/golden/baseline_windows.npz; the GPU tests compare the whole 128x72 window)"""
    z = np.load(os.path.join(GOLDEN, "baseline_windows.npz"))
    for name in ("c3_bunny_room", "c4_dwarf_room", "c2_analytic"):
        meta = manifest["glibc_distance_baseline"][name]
        x0, y0, x1, y1 = meta["window"]
        scene = api.Scene.load_scn(os.path.join(ROOT, "data", name + ".scn")).commit()
        rect = (x0, y0, x0 + 16, y0 + 8)
        img, _ = oracle.OracleScene(scene.flatten(1920, 1080)).render(1920, 1080, 1024, meta["seed"], "chunk", chunk=64, rect=rect, threads=8)
        assert_bits_equal(img[rect[1]:rect[3], rect[0]:rect[2]], z[name + "__det"][:8, :16], name)


@pytest.mark.parametrize("variant", ["at_caps", "mats_over", "lights_over", "ref_limits"])
def test_oracle_on_the_scenes_at_and_past_the_table_caps(api, oracle, manifest, tmp_path_factory, variant):
    """tools/make_tablescene.py: 48 / 49 materials, 64 / 65 lights, and the most the reference's loader holds (100 materials,
    100 lights).  The loader agrees with the reference's on every count and array, and the oracle equals the reference's own
    pixels (renders_tables_<variant>.npz) and closest hits (raycast_tables_<variant>.npz), bit for bit; the conditions that
    make the scene tell a wrong table index (table_scenes.assert_conditions) hold."""
    import hashlib
    import table_scenes
    d = tmp_path_factory.mktemp("tables_" + variant)
    scene, counts, csg = table_scenes.build(api, variant, d)
    meta = manifest["tablescenes"][variant]
    assert hashlib.sha256(open(os.path.join(str(d), variant + ".scn"), "rb").read()).hexdigest() == meta["scn_sha256"]
    si = scene.info()
    for kind, n in (("materials", si.material_count), ("spheres", si.sphere_count), ("boxes", si.box_count), ("cylinders", si.cylinder_count),
                    ("lights", si.light_count), ("meshes", si.mesh_count)):
        assert n == meta["octree"][kind] == counts[kind], kind
    assert si.triangle_count == counts["triangles"]
    scene.commit()
    flat = scene.flatten(table_scenes.W, table_scenes.H)
    dg = ref_io.scene_digest(flat)
    for k in ("materials_sha256", "spheres_sha256", "boxes_sha256", "cylinders_sha256", "lights"):
        assert dg[k] == meta[k], k
    osc = oracle.OracleScene(flat, with_reference_csg=csg)
    table_scenes.assert_conditions(variant, scene, osc, flat)
    st = osc.tree_stats()
    assert (st["nodes"], st["nonempty_leaves"], st["record_bytes"]) == (meta["octree"]["octree_nodes"], meta["octree"]["octree_leaves"], meta["octree"]["record_bytes"])
    z = np.load(os.path.join(GOLDEN, "renders_tables_%s.npz" % variant))
    assert len(meta["renders"]) == 4
    for e in meta["renders"]:
        o2 = oracle.OracleScene(scene.flatten(e["width"], e["height"]), with_reference_csg=csg)
        img, rs = o2.render(e["width"], e["height"], e["spp"], e["seed"], e["policy"], chunk=e["chunk"], threads=1)
        assert_bits_equal(img, z[e["key"]], "%s %s" % (variant, e["key"]))
        assert rs["shapes_tested"] == e["shapes_tested"], e["key"]
        if e["policy"] != "tile32":
            assert rs["final_rng"] == e["final_rng"], e["key"]
    r = np.load(os.path.join(GOLDEN, "raycast_tables_%s.npz" % variant))
    t, n, mat = oracle.OracleScene(scene.flatten(64, 64), with_reference_csg=csg).raycast(r["rays"][:, 0:3], r["rays"][:, 3:6])
    assert_bits_equal(t, r["t"], "t")
    assert_bits_equal(n, r["n"], "normal")
    assert (mat == r["mat"]).all() and (r["mat"] >= 7).sum() >= 40  # the fixture sees the grid's materials, not the walls alone
