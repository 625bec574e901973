"""The tree's shape cannot change a bit -- on the host.  Every hit comes out of traverse() (csrc/ort_lane.h) walking the tree
build_tree (csrc/ort_tree.cpp) made, and that tree's shape is a matter of four commit-time knobs: ORT_LEAF_TRI, ORT_LEAF_OTHER,
ORT_TREE_SPLIT_KINDS, ORT_ANALYTIC_PROLOGUE.  tests/tree_shapes.py names six settings of them and lists, per scene, those that
change its tree; here

  * tools/host_sim --tree-check verifies, for every scene the repository has or generates and every setting, what the lanes take
    for granted about a tree (coverage, slot tables, boxes, SPHERE_BELOW_BIT, depths, the breadth-first top, the wide tree);
  * tools/host_sim runs the lane code on every listed (scene, variant) -- renders in both seeding policies with the plain
    loop, the wide tree, the LDS tables' image, the wavefront schedule and the five-waves split of the stack, every ray
    query, the feature render and a batch of views -- bit for bit against the oracle, whose answers know no variant, and on
    the cluster scene (tools/make_clusterscene.py: full 16-primitive leaves of every kind, duplicates, coplanar faces) against
    the reference's own pixels and hits (tests/golden/*_cluster.npz) as well.

SIM_WAVEFRONT's value is the slot count of the schedule: 100, as in the other host tests."""
import glob
import hashlib
import os

import numpy as np
import pytest

import accumulate_cases as acs
import ao_cases
import deep_scenes
import feature_cases
import follow_cases as fw
import host_sim_tool as hs
import irradiance_cases
import light_groups_cases as lg
import occluded_cases
import radiance_cases
import sample_map_cases as sm
import table_scenes
import tree_shapes as ts
from conftest import DATA, assert_bits_equal

TABS = {"SIM_TABS": "1"}
SOME_EXACT = {"SIM_FORCE_FALLBACK": "0xf"}
RENDER_RUNS = [("host_sim", {}), ("host_sim", {"SIM_WIDE": "1"}), ("host_sim", TABS), ("host_sim", {"SIM_WAVEFRONT": "100"}), ("host_sim_w5", {})]
ids = lambda e: ("+".join(sorted(e)) or "plain") if isinstance(e, dict) else str(e)
pairs = pytest.mark.parametrize("name,variant", ts.PAIRS, ids=ts.PAIR_IDS)


@pytest.fixture()
def world(api, oracle, load_scene, tmp_path_factory):
    return lambda name: ts.world(api, oracle, load_scene, tmp_path_factory, name)


def _env(variant, extra=None):
    return dict(ts.VARIANTS[variant], **(extra or {}))


# ---- the listing -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ts.SCENES)
def test_every_listed_variant_changes_the_tree(world, monkeypatch, name):
    """no listed case is vacuous, none that would change the tree is left out, and each variant shows what it is for"""
    w = world(name)
    info = {v: ts.variant_scene(w, v, monkeypatch).tree_info() for v in ts.VARIANTS}
    base = info["default"]
    for v in ts.VARIANTS:
        if v != "default":
            assert (ts.tree_tuple(info[v]) != ts.tree_tuple(base)) == (v in ts.LISTED[name]), (name, v, info[v], base)
    if "leaf1" in ts.LISTED[name]:
        assert info["leaf1"]["max_leaf_prims"] == 1
    assert info["no_prologue"]["prologue_prims"] == 0 and info["mixed_root"]["prologue_prims"] == 0
    if name in ts.HAS_TRIANGLES_AND_ANALYTIC:
        assert info["mixed_root"]["node_count"] != info["no_prologue"]["node_count"]
    assert 0 < info["small_prologue"]["prologue_prims"] < base["prologue_prims"]
    print("\n".join("%s %s: %r" % (name, v, ts.tree_tuple(info[v])) for v in ts.VARIANTS))


def test_the_cluster_scene_builds_full_leaves_of_every_kind(world, manifest):
    """committed under leaf16 the cluster scene has a 16-primitive leaf of triangles, of spheres, of boxes and of cylinders: the
    top bits of the leaf word's count field are set; and the scene stays within the kernels' LDS tables"""
    w = world("cluster")
    assert hashlib.sha256(open(w.scn, "rb").read()).hexdigest() == manifest["clusterscene"]["scn_sha256"], "the fixtures are this scene's"
    line, r = ts.tree_check(w.scn, w.base, "leaf16")
    assert line is not None, r.stderr
    assert line["max_leaf"] == {"triangle": 16, "sphere": 16, "box": 16, "cylinder": 16}, line
    line, _ = ts.tree_check(w.scn, w.base, "default")
    assert max(line["max_leaf"].values()) <= 4 and line["prologue"] > 0
    si = w.scene.info()
    caps = table_scenes.caps()
    assert si.material_count <= min(47 + 1, caps["materials"]) and si.light_count <= caps["lights"]
    assert si.material_count <= 99 and si.sphere_count <= 100 and si.cylinder_count <= 100   # what the reference's loader holds
    assert min(si.sphere_count, si.box_count, si.cylinder_count, si.triangle_count) >= 18
    ts.assert_cluster_conditions(w)


def test_the_cluster_scene_as_arrays_is_the_same_layout(api, world):
    """make_clusterscene.arrays(): the shapes, materials and lights of the .scn in the same order, every number within the six
    decimals the text holds (the loaders scale decimals their own way, so not to the bit: the tests use the .scn throughout)"""
    args, _ = ts.make_clusterscene.arrays()
    a, b = api.Scene.from_arrays(**args).commit().flatten(*ts.RENDER[:2]), world("cluster").flat
    assert a.lights.tobytes() == b.lights.tobytes()
    for k in ("materials", "spheres", "boxes", "cylinders"):
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape
        for f in x.dtype.names:
            assert np.allclose(x[f], y[f], rtol=0, atol=4e-6), (k, f)
    assert [len(m["vertices"]) for m in a.meshes] == [len(m["vertices"]) for m in b.meshes] == [3 * 18, 3 * 2]
    assert all(np.allclose(m["vertices"], n["vertices"], rtol=0, atol=4e-6) and m["mat"] == n["mat"] for m, n in zip(a.meshes, b.meshes))


# ---- the tree check ------------------------------------------------------------------------------------------------------------
def _check_all_variants(scn, base):
    for variant in ts.VARIANTS:
        line, r = ts.tree_check(scn, base, variant)
        assert line is not None, "%s under %s: %s" % (os.path.basename(scn), variant, r.stderr[-600:])
        if variant == "leaf1":
            assert max(line["max_leaf"].values()) <= 1
        if variant in ("no_prologue", "mixed_root"):
            assert line["prologue"] == 0


@pytest.mark.parametrize("name", sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(DATA, "*.scn"))))
def test_tree_check_on_the_repository_scenes(name):
    _check_all_variants(os.path.join(DATA, name + ".scn"), DATA + "/")


@pytest.mark.parametrize("name", ["cluster", "deep", "c5_heightfield_224"] + ["tables_" + v for v in table_scenes.make_tablescene.variants() if v != "beyond_ref"])
def test_tree_check_on_the_generated_scenes(api, oracle, world, tmp_path, name):
    """(beyond_ref exists as arrays alone: no .scn for the tool to load)"""
    if name == "cluster":
        w = world(name)
        scn, base = w.scn, w.base
    elif name == "deep":
        scn, _ = deep_scenes.make_deepscene.write_scene(str(tmp_path))
        base = str(tmp_path) + "/"
    elif name.startswith("c5_"):
        import make_heightfield
        scn, _, _ = make_heightfield.write_scene(224, str(tmp_path))
        base = str(tmp_path) + "/"
    else:
        v = name[len("tables_"):]
        scn, _ = table_scenes.make_tablescene.write_scene(str(tmp_path), stem=v, **table_scenes.variants()[v])
        base = str(tmp_path) + "/"
    _check_all_variants(scn, base)


# ---- the lanes, per (scene, variant) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tool,env", RENDER_RUNS, ids=lambda v: v if isinstance(v, str) else ids(v))
@pytest.mark.parametrize("policy", ["chunk", "pixel"])
@pairs
def test_render(world, tmp_path, name, variant, policy, tool, env):
    w = world(name)
    width, height, spp, chunk = ts.RENDER
    chunk = chunk if policy == "chunk" else 0
    ref, ost = ts.oracle_render(w, width, height, spp, policy, chunk)
    args, outs = hs.render_args(str(tmp_path), w.scn, width, height, spp, ts.SEED, policy, chunk, w.base)
    r = hs.run(hs.built(tool), args, env=_env(variant, env), threads=1 if "SIM_WAVEFRONT" in env else 8)
    got = np.fromfile(outs[0], "<f4").reshape(height, width, 3)
    assert_bits_equal(got, ref, "%s %s %s %s %r vs the oracle" % (name, variant, policy, tool, env))
    c = hs.counters(r)
    assert c["paths"] == ost["paths"] == width * height * spp and c["rays"] == ost["rays"], (c, ost)
    if name == "cluster":
        z = ts.golden("renders_cluster.npz")
        assert_bits_equal(got, z["%s_%dx%d_%dspp_c%d_s%d" % (policy, width, height, spp, max(chunk, 1), ts.SEED)], "%s %s vs the reference" % (variant, policy))


@pytest.mark.parametrize("env", [{}, TABS, SOME_EXACT, {"SIM_FORCE_FALLBACK": "0"}], ids=ids)
@pairs
def test_raycast(world, tmp_path, name, variant, env):
    w = world(name)
    rays, t, n, mat = ts.rays_of(w)
    if name == "cluster":
        ts.assert_cluster_conditions(w)
    hits, r = hs.raycast(hs.built("host_sim"), tmp_path, w.scn, rays, base=w.base, env=_env(variant, env), threads=8)
    what = "%s %s %r" % (name, variant, env)
    assert_bits_equal(hits["t"], t, what + " t")
    assert_bits_equal(hits["n"], n, what + " normals")
    assert (hits["mat"] == mat).all(), "%s: %d materials differ" % (what, (hits["mat"] != mat).sum())
    # holds because no shape of these scenes carries material 0; tests/test_void_material_host.py has the scenes where a hit with
    # mat == 0 names a shape
    assert ((hits["prim"] == hs.NO_PRIM) == (mat == 0)).all()
    c = hs.counters(r)
    assert c["rays"] == len(rays)
    # the fast walk is what is tested.  Half of the mixed set is the exact walk's by design (raycast_needs_exact, ort_lane.h: origins
    # far outside, directions that are not unit vectors), and resolve_hit hands it what it cannot settle (more of it where walls
    # are in the tree and not in the prologue: 851 rays of testscene's set under the default tree, 1 016 with no prologue); of
    # the other half, at least half must be the fast walk's own
    assert c["fallback"] == len(rays) if env.get("SIM_FORCE_FALLBACK") == "0" else (0 < c["fallback"] < len(rays) if env == SOME_EXACT else c["fallback"] * 4 <= 3 * len(rays)), c
    if name == "cluster":
        z = ts.golden("raycast_cluster.npz")
        assert z["rays"].tobytes() == rays.tobytes(), "the fixture's rays are this set"
        assert_bits_equal(hits["t"], z["t"], what + " t vs the reference")
        assert_bits_equal(hits["n"], z["n"], what + " normals vs the reference")
        assert (hits["mat"] == z["mat"]).all()


@pytest.mark.parametrize("env", [{}, SOME_EXACT], ids=ids)
@pairs
def test_occluded_at_and_one_ulp_either_side_of_the_hit(world, tmp_path, name, variant, env):
    w = world(name)
    rays, t, _, mat = ts.rays_of(w)
    tmax = ts.occluded_limits(t)
    want = occluded_cases.expected(t, mat, tmax)
    assert want.mean() > 0.2 and (~want).mean() > 0.5
    got = hs.occluded(hs.built("host_sim"), tmp_path, w.scn, rays, tmax, w.base, env=_env(variant, env), threads=8)
    assert (got == want.astype(np.uint8)).all(), "%s %s: %d bytes differ" % (name, variant, (got != want.astype(np.uint8)).sum())
    got = hs.occluded(hs.built("host_sim"), tmp_path, w.scn, rays, None, w.base, env=_env(variant, env), threads=8)
    assert (got == (mat != 0).astype(np.uint8)).all()


@pytest.mark.parametrize("env", [{}, TABS], ids=ids)
@pairs
def test_radiance(world, tmp_path, name, variant, env):
    w = world(name)
    cases = ts.radiance_cases_of(w)
    want_rgb, want_states = ts.radiance_expected(w)
    rgb, states = hs.radiance(hs.built("host_sim"), tmp_path, w.scn, cases.rays, cases.seeds, ts.RADIANCE_SPP, 0.8, w.base, env=_env(variant, env), threads=8)
    radiance_cases.assert_same(rgb, states, want_rgb, want_states, "%s %s %r" % (name, variant, env))


@pairs
def test_irradiance(world, tmp_path, name, variant):
    w = world(name)
    pts = ts.points_of(w, ts.N_POINTS_HOST)
    want_rgb, want_states = ts.irradiance_expected(w, ts.N_POINTS_HOST)
    rgb, states, _ = irradiance_cases.host_sim(hs.built("host_sim"), tmp_path, w.scn, pts.points, pts.seeds, ts.IRR_SPP, 0.0, w.base, env=_env(variant), threads=8)
    radiance_cases.assert_same(rgb, states, want_rgb, want_states, "%s %s" % (name, variant))


@pytest.mark.parametrize("radius", ["none", "per point"])
@pairs
def test_ambient_occlusion(world, tmp_path, name, variant, radius):
    w = world(name)
    pts = ts.points_of(w, ts.N_POINTS_HOST)
    radius = None if radius == "none" else ts.ao_radius(w)
    want = ts.ao_expected(w, radius, ts.N_POINTS_HOST)
    got = ao_cases.host_sim(hs.built("host_sim"), tmp_path, w.scn, pts.points, pts.seeds, None if radius is None else radius[:ts.N_POINTS_HOST], ts.AO_SPP,
                            base=w.base, env=_env(variant), threads=8)
    ao_cases.assert_same(got[:3], want, "%s %s" % (name, variant))


@pairs
def test_features(world, tmp_path, name, variant):
    w = world(name)
    width, height, spp = ts.FEATURES
    got, _ = feature_cases.host_sim(hs.built("host_sim"), tmp_path, w.scn, width, height, None, spp, seed=ts.SEED, base=w.base, env=_env(variant), threads=8)
    feature_cases.assert_same({k: v[0] for k, v in got.items()}, ts.features_expected(w), "%s %s" % (name, variant))


def _follow(w, tmp_path, variant, env=None):
    width, height, spp = ts.FEATURES
    got, r = fw.host_sim(hs.built("host_sim"), tmp_path, w.scn, width, height, None, spp, ts.FOLLOW[0], ts.FOLLOW[1], seed=ts.SEED, base=w.base,
                         env=_env(variant, env), threads=8)
    return {k: v[0] for k, v in got.items()}, hs.counters(r)


@pytest.mark.parametrize("env", [{}, TABS], ids=ids)
@pairs
def test_follow(world, tmp_path, name, variant, env):
    """--follow at FEATURES' frame, rr 0.5, cap 64, against follow_cases' chain from the oracle, which knows no variant: all seven
    planes, the ids' shapes through --raycast of the chain's last rays under the same variant, and every plane but ids byte for
    byte what the first variant of the scene gave.  The followed bounce rays start on a surface, so they are the fast walk's own:
    on glass_room, whose default tree is one leaf, they walk a tree only under no_prologue, mixed_root and small_prologue --
    asserted through the node tests per ray, which under no_prologue exceed the default tree's on every scene"""
    w = world(name)
    ts.assert_follow_conditions(w)
    c = ts.follow_chain(w)
    got, counted = _follow(w, tmp_path, variant, env)
    what = "%s %s %r follow" % (name, variant, env)
    fw.assert_same(got, ts.follow_expected(w), what)
    assert counted["rays"] == c.rays and counted["paths"] == 0
    prims = hs.raycast(hs.built("host_sim"), tmp_path, w.scn, c.last, base=w.base, env=_env(variant), threads=8)[0]["prim"]
    fw.assert_prims(got["ids"][None], [c], prims, what)
    as_bytes = lambda p: [np.ascontiguousarray(p[k]).tobytes() for k in fw.PLANES if k != "ids"]
    first = ts.cached(w, ("follow on the host, the default tree", ids(env)), lambda: as_bytes(_follow(w, tmp_path, "default", env)[0]))
    assert as_bytes(got) == first, "%s: a plane differs from the one under the default tree" % what
    if variant == "no_prologue":
        _, default = _follow(w, tmp_path, "default", env)
        print("%s: node tests per ray %.2f under no_prologue, %.2f under the default tree" % (name, counted["node_tests"] / counted["rays"], default["node_tests"] / default["rays"]))
        assert default["rays"] == counted["rays"] and counted["node_tests"] > default["node_tests"]


@pytest.mark.parametrize("policy", ["chunk", "pixel"])
@pairs
def test_views(world, tmp_path, name, variant, policy):
    w = world(name)
    width, height, spp, chunk = ts.VIEWS
    chunk = chunk if policy == "chunk" else 0
    cams = ts.view_cams(w)
    frames = hs.views(hs.built("host_sim"), tmp_path, w.scn, cams, ts.VIEW_SEEDS, width, height, spp, policy, chunk, w.base, env=_env(variant), threads=8)
    for v, (cam, seed) in enumerate(zip(cams, ts.VIEW_SEEDS)):
        ref, _ = ts.oracle_render(w, width, height, spp, policy, chunk, cam=cam, seed=seed)
        assert_bits_equal(frames[v], ref, "%s %s %s view %d" % (name, variant, policy, v))


@pytest.mark.parametrize("env", [{}, TABS], ids=ids)
@pairs
def test_light_groups_and_sample_map(world, tmp_path, name, variant, env):
    """the lanes of pt_groups and pt_sample_map at VIEWS' frame: one group per light material against the dark twins of the
    world's flattened scene, and the mixed map at cap 4 against the oracle's chains; the lanes of pt_accumulate under the same
    map in two passes (caps 1 and 3) against those chains folded, every plane byte for byte the default tree's"""
    w = world(name)
    width, height, spp, _ = ts.VIEWS
    assert (lg.W, lg.H) == (width, height)
    ref = lg.SceneRef(w.scn, w.base)
    _, G = ts.light_groups_of(w)
    frames, rgb, states = lg.host_light_groups(hs.built("host_sim"), tmp_path, ref, ts.group_table(w), G, spp, seed=ts.SEED, env=_env(variant, env), threads=8)
    want = ts.light_groups_expected(w)
    assert (want[0] != 0).any()
    for got, w_, label in zip((frames[0], rgb[0], states[0]), want, ("group frames", "out_rgb", "final states")):
        lg.assert_plane(got, w_, None, lg.GUARD_F, "%s %s %r light groups: %s" % (name, variant, env, label))
    smap, want = ts.sample_map_expected(w)
    got, _ = sm.host_sample_map(hs.built("host_sim"), tmp_path, ref, smap, ts.MAP_CAP, seed=ts.SEED, env=_env(variant, env), threads=8)
    sm.assert_planes(tuple(p[0] for p in got), want, "%s %s %r sample map" % (name, variant, env))
    # the lanes of pt_accumulate: a continued job reloads its sums and state and walks the variant's tree from there
    passes = lambda v: [np.ascontiguousarray(a).tobytes() for a in
                        ts.accumulate_passes(w, acs.host_call(hs.built("host_sim"), tmp_path, ref, env=_env(v, env), threads=8), "%s %s %r" % (name, v, env)).all()]
    first = ts.cached(w, ("accumulate on the host, the default tree", ids(env)), lambda: passes("default"))
    assert passes(variant) == first, "%s %s %r accumulate: a plane differs from the one under the default tree" % (name, variant, env)
