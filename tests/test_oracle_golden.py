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


# ---- the generated scenes that the other tests hold against the oracle alone (make_golden.py --only-generated) ---------------------
DIGEST_KEYS = ("counts", "camera_bits", "ambient_bits", "materials_sha256", "spheres_sha256", "boxes_sha256", "cylinders_sha256", "lights", "meshes", "sha256")


def _loaded(api, scn, meta, w, h):
    """the file has the manifest's hash and the product's loader gives the reference loader's arrays -> (scene, flat)"""
    import reference_goldens as rg
    assert rg.sha256(scn) == meta["scn_sha256"], scn
    scene = api.Scene.load_scn(scn).commit()
    flat = scene.flatten(w, h)
    dg = ref_io.scene_digest(flat)
    for k in DIGEST_KEYS:
        assert dg[k] == meta[k], (scn, k)
    return scene, flat


def _same_tree(osc, meta):
    st = osc.tree_stats()
    assert (st["nodes"], st["nonempty_leaves"], st["record_bytes"]) == (meta["octree"]["octree_nodes"], meta["octree"]["octree_leaves"], meta["octree"]["record_bytes"])


def _pixel_planes_match(oracle, osc, w, h, spp, seed, frame, states, meta, what):
    """the oracle's PIXEL render, its counters and (states given) every pixel's final series state against the reference's"""
    import reference_goldens as rg
    if states is None:
        img, st = osc.render(w, h, spp, seed, "pixel", threads=1)
    else:
        img, st, got = rg.oracle_pixel_planes(oracle, osc, w, h, spp, seed)
        rg.assert_words_equal(got, states, what + ": final states")
    assert_bits_equal(img, frame, what)
    assert (st["shapes_tested"], st["final_rng"]) == (meta["shapes_tested"], meta["final_rng"]), what


@pytest.fixture(scope="module")
def deep(api, manifest, tmp_path_factory):
    """the deep scene's files, regenerated: (scn, graze_scn, layout, the manifest's entry, {which: the committed scene of the file})"""
    import deep_scenes
    import reference_goldens as rg
    d = tmp_path_factory.mktemp("golden_deepscene")
    scn, graze_scn, layout = rg.deep_files(d)
    meta = manifest["generated"]["deepscene"]
    for k in ("inner", "outer"):
        assert rg.sha256(os.path.join(str(d), k + ".ply")) == meta["ply_sha256"][k]
    w, h = deep_scenes.GPU_RENDER[:2]
    scenes = {"cone": _loaded(api, scn, meta, w, h)[0], "graze": _loaded(api, graze_scn, meta["graze"], w, h)[0]}
    return scn, graze_scn, layout, meta, scenes


def test_deep_scene_is_the_references(api, oracle, deep):
    """coordinates out to 1.2e18: the loader's arrays, the arrays the deep-stack tests build without a file (make_deepscene.arrays,
    what deep_scenes.world commits) and the oracle's octree are the reference's"""
    import deep_scenes
    from deep_scenes import make_deepscene
    scn, graze_scn, layout, meta, scenes = deep
    w, h = deep_scenes.GPU_RENDER[:2]
    args, _ = make_deepscene.arrays()
    flat = api.Scene.from_arrays(**args).commit().flatten(w, h)
    dg = ref_io.scene_digest(flat)
    for k in DIGEST_KEYS:
        assert dg[k] == meta[k], k
    _same_tree(oracle.OracleScene(flat, with_reference_csg=True), meta)
    assert meta["octree"] == dict(meta["graze"]["octree"])   # the grazing scene differs by its camera alone
    assert meta["camera_bits"] != meta["graze"]["camera_bits"]


def test_deep_scene_renders_match_reference(oracle, deep):
    """the reference's own frames of the deep scene in four seeding policies, and of the grazing camera's scene: image bits,
    shapes-tested counter, final RNG state"""
    import deep_scenes
    import reference_goldens as rg
    _, _, _, meta, scenes = deep
    z = rg.load("renders_deepscene.npz")
    assert sorted(z.files) == sorted(k for *_, k in rg.deep_renders()) == sorted(meta["renders"])
    for cam, policy, w, h, spp, chunk, key in rg.deep_renders():
        osc = oracle.OracleScene(scenes[cam].flatten(w, h), with_reference_csg=True)
        img, st = osc.render(w, h, spp, deep_scenes.SEED, policy, chunk=max(chunk, 1), threads=1)
        assert_bits_equal(img, z[key], key)
        assert st["shapes_tested"] == meta["renders"][key]["shapes_tested"], key
        if policy != "tile32":
            assert st["final_rng"] == meta["renders"][key]["final_rng"], key
        assert (z[key] != 0).any()


def test_deep_scene_raycasts_match_reference(oracle, deep):
    """the 4 000 cone rays and the 4 000 grazing rays of deep_scenes.world: the rays regenerate bit for bit, and the oracle's t,
    normal and material are the reference's"""
    import deep_scenes
    import reference_goldens as rg
    _, _, layout, meta, scenes = deep
    z = rg.load("raycast_deepscene.npz")
    rays, graze, _ = deep_scenes.ray_sets(layout)
    osc = oracle.OracleScene(scenes["cone"].flatten(64, 64), with_reference_csg=True)
    import hashlib
    for name, rr in (("cone", rays), ("graze", graze)):
        assert hashlib.sha256(np.ascontiguousarray(rr, "<f4").tobytes()).hexdigest() == meta["rays_sha256"][name], name
        t, n, mat = osc.raycast(rr[:, 0:3], rr[:, 3:6])
        assert_bits_equal(t, z[name + "__t"], name + " t")
        assert_bits_equal(n, z[name + "__n"], name + " normals")
        assert (mat == z[name + "__mat"]).all(), name
        assert (z[name + "__mat"] != 0).all()   # the room is closed


def test_light_pick_rooms_match_reference(api, oracle, manifest, tmp_path_factory):
    """the rooms of 1, 1, 2 and 3 lights of tests/test_gpu_light_pick.py in both flavours: the oracle's PIXEL image and every
    pixel's final RandomSeries state -- what that test holds the device against -- are the reference's"""
    import reference_goldens as rg
    import test_gpu_light_pick as pick
    d = tmp_path_factory.mktemp("golden_light_pick")
    z = rg.load("renders_light_pick.npz")
    rooms = rg.pick_rooms()
    assert len(rooms) == 8 and len(z.files) == 16
    for flavour, lights, key, text in rooms:
        meta = manifest["generated"]["light_pick"][key]
        scene, flat = _loaded(api, rg.write_text(d, "pick_" + key, text), meta, pick.W, pick.H)
        assert flat.lights["type"].tolist() == pick.LIGHTS[lights][1]
        osc = oracle.OracleScene(flat)
        _same_tree(osc, meta)
        _pixel_planes_match(oracle, osc, pick.W, pick.H, pick.SPP, pick.SEED, z[key + "__pixel"], z[key + "__states"], meta["render"], key)


@pytest.mark.parametrize("name", ["room_all_lobes", "room_diffuse"])
def test_rooms_and_their_twins_match_reference(api, oracle, manifest, tmp_path_factory, name):
    """the rooms of the light-group and feature renders, their three dark twins and their white twin.  Both ways: the oracle on
    the twin written as a file (every other `light` line 0 0 0; every `brdf` and `light` line `light 1 1 1`) and the oracle on
    the patched material arrays that light_groups_cases.dark_twin and feature_cases.twin(white=True) build give the reference's
    frames of the files, so the construction the other tests use is the reference's"""
    import feature_cases as fc
    import light_groups_cases as lg
    import reference_goldens as rg
    d = tmp_path_factory.mktemp("golden_" + name)
    z = rg.load("renders_rooms.npz")
    metas = manifest["generated"]["rooms"][name]
    flats = {}
    for variant, text in rg.room_variants(name):
        meta = metas[variant]
        _, flats[variant] = _loaded(api, rg.write_text(d, "%s_%s" % (name, variant), text), meta, lg.W, lg.H)
        osc = oracle.OracleScene(flats[variant])
        _same_tree(osc, meta)
        for spp in lg.SPPS:
            key = "%s__%s__%dspp" % (name, variant, spp)
            states = None if variant.startswith("dark") else z[key + "__states"]
            _pixel_planes_match(oracle, osc, lg.W, lg.H, spp, lg.SEED, z[key], states, meta["renders"][key], key + ", the file")
    own = flats["own"]
    lights = [int(m) for m in np.nonzero(own.materials["is_light"])[0]]
    assert len(lights) == 3
    for g, m in enumerate(lights):
        emit = flats["dark%d" % g].materials["emit"].view("<u4")
        assert (flats["dark%d" % g].materials["is_light"] == own.materials["is_light"]).all()
        assert emit[m].any() and not emit[[k for k in lights if k != m]].any()   # all-zero bits: +0, the value dark_twin writes
        twin = lg.dark_twin(oracle, own, frozenset([m]))
        for spp in lg.SPPS:
            key = "%s__dark%d__%dspp" % (name, g, spp)
            img, _ = twin.render(lg.W, lg.H, spp, lg.SEED, "pixel", rr=lg.RR, threads=1)
            assert_bits_equal(img, z[key], key + ", the patched arrays")
            assert (z[key] != 0).any() and (z[key].view("<u4") != z["%s__own__%dspp" % (name, spp)].view("<u4")).any()
    white = fc.twin(oracle, own, white=True)
    for spp in lg.SPPS:
        key = "%s__white__%dspp" % (name, spp)
        img, states = fc.twin_planes(white, own.camera, lg.W, lg.H, lg.SEED, spp)
        assert_bits_equal(img, z[key], key + ", the patched arrays")
        rg.assert_words_equal(states, z[key + "__states"], key + ", the patched arrays: final states")


@pytest.mark.parametrize("name", ["room_all_lobes", "glass_room"])
def test_pixel_chains_match_reference(api, oracle, manifest, tmp_path_factory, name):
    """render_adaptive_cases.chains -- one sample per call, the series threaded through, what the adaptive and sample-map
    expectations are cut from -- against the reference called the same way (ref_driver's chain): every call's colour and the
    state after it, 64 calls a pixel"""
    import reference_goldens as rg
    import render_adaptive_cases as rac
    scn, _ = rg.chain_scene(tmp_path_factory.mktemp("golden_chain_" + name), name)
    meta = manifest["generated"]["chains"][name]
    assert rg.sha256(scn) == meta["scn_sha256"]
    assert (meta["samples"], meta["seed"], meta["width"], meta["height"]) == (rg.CHAIN_SAMPLES, rac.SEED, rac.W, rac.H) and rg.CHAIN_SAMPLES == rac.MAX_SPP
    want = rg.chains_from(rg.load("chains_rooms.npz"), name)
    scene = api.Scene.load_scn(scn).commit()
    osc = oracle.OracleScene(scene.flatten(rac.W, rac.H))
    got = rac.chains(osc, rac.W, rac.H, rac.SEED, rac.RR)
    assert sorted(got) == sorted(want)
    tested, img = 0, np.zeros((rac.H, rac.W, 3), "<f4")
    for (x, y), (_, states) in got.items():   # the same calls once more, for the counter the chains do not keep
        for s in [oracle.job_seed(rac.SEED, y * rac.W + x)] + states[:-1].tolist():
            tested += osc.tiled_raytrace(img, x, y, x + 1, y + 1, int(s), 1, rac.RR)[0]
    assert tested == meta["shapes_tested"]
    cols = np.stack([got[k][0] for k in sorted(got)])
    assert_bits_equal(cols, np.stack([want[k][0] for k in sorted(got)]), name + " colours")
    rg.assert_words_equal(np.stack([got[k][1] for k in sorted(got)]), np.stack([want[k][1] for k in sorted(got)]), name + " states")
    assert (cols != 0).any(axis=(1, 2)).mean() > 0.5   # most pixels see light within 64 samples
