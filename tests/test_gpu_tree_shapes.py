"""The tree's shape cannot change a bit -- on the device.  tests/test_tree_shapes_host.py pins that on the host, where one lane
runs at a time; here the wave-level parts run: the descend loop's break-outs and the refill exits (a lane that leaves
traverse() mid-descent and resumes must carry cur and sp across), announce_winner, the ray exchange, the treelet in LDS.  One
scene handle per listed (scene, variant) of tests/tree_shapes.py, committed under the variant's knobs and uploaded; every
render call and ray query on it, under the launch knobs that pick another kernel or another schedule, bit for bit against the
oracle (whose answers know no variant), against the first variant's own output (which says sooner which shape is off), and on the
cluster scene against the reference's own pixels and hits (tests/golden/*_cluster.npz)."""
import numpy as np
import pytest

import accumulate_cases as acs
import ao_cases
import adaptive_cases
import feature_cases
import follow_cases as fw
import light_groups_cases as lg
import occluded_cases
import radiance_cases
import render_adaptive_cases as rac
import sample_map_cases as sm
import tree_shapes as ts
from conftest import assert_bits_equal
from test_gpu_raycast import assert_same_hits

pytestmark = pytest.mark.gpu

KNOBS = ("ORT_EXCHANGE", "ORT_WAVES5", "ORT_WIDE", "ORT_MODE", "ORT_KERNEL", "ORT_LDS_TABLES", "ORT_DEBUG_FORCE_FALLBACK", "ORT_CACHE_RESIDENT",
         "ORT_REFILL_BELOW", "ORT_DESCEND_BELOW")
RENDER_KNOBS = {
    "default": {},
    "exchange": {"ORT_EXCHANGE": "1"},
    "waves5": {"ORT_EXCHANGE": "0", "ORT_WAVES5": "1"},
    "plain": {"ORT_EXCHANGE": "0", "ORT_WAVES5": "0"},
    "wide": {"ORT_WIDE": "1"},
    "tables_in_hbm": {"ORT_LDS_TABLES": "0"},
    "wavefront": {"ORT_MODE": "wavefront"},
    "general": {"ORT_KERNEL": "general"},
    "some_exact": {"ORT_DEBUG_FORCE_FALLBACK": "0xf"},
}
# the large-tree policy (refill 32, descend 16, five waves) on these small trees, and the loop exits at their extremes: every
# ray leaves the descend loop at once and refills at every step, or none ever does
LARGE_TREE = [{"ORT_CACHE_RESIDENT": "0"}] + [dict(e, ORT_REFILL_BELOW=r, ORT_DESCEND_BELOW=d) for r in ("1", "64") for d in ("0", "64")
                                             for e in ({}, {"ORT_EXCHANGE": "1"})]
pairs = pytest.mark.parametrize("name,variant", ts.PAIRS, ids=ts.PAIR_IDS)
_handles = {}
_first = {}


@pytest.fixture()
def handle(api, oracle, load_scene, tmp_path_factory, monkeypatch):
    """(scene name, variant) -> (the scene's world, a handle committed under the variant and uploaded); cached for the module"""
    def get(name, variant):
        w = ts.world(api, oracle, load_scene, tmp_path_factory, name)
        if (name, variant) not in _handles:
            scene = ts.variant_scene(w, variant, monkeypatch)
            if scene.device is None:
                assert api.device_count() >= 1
                scene.upload(0)
            if variant != "default":
                assert ts.tree_tuple(scene.tree_info()) != ts.tree_tuple(w.scene.tree_info())
            _handles[(name, variant)] = scene
        return w, _handles[(name, variant)]
    return get


@pytest.fixture()
def knobs(monkeypatch):
    def set_(env):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    return set_


def same_as_first(name, variant, key, *arrays):
    """what the first variant of this scene that got here answered for key, the other variants answer too, byte for byte"""
    got = [np.ascontiguousarray(a).tobytes() for a in arrays]
    first_variant, first = _first.setdefault((name, key), (variant, got))
    for i, (a, b) in enumerate(zip(got, first)):
        assert a == b, "%s %s: output %d under %s differs from the one under %s" % (name, key, i, variant, first_variant)


@pairs
def test_renders(handle, knobs, name, variant):
    """CHUNK and PIXEL under every knob set, TILE32 once; once with counters: paths and rays are the oracle's"""
    w, scene = handle(name, variant)
    width, height, spp, chunk = ts.GPU_RENDER
    for policy, ch in (("chunk", chunk), ("pixel", 0)):
        ref, ost = ts.oracle_render(w, width, height, spp, policy, ch)
        for label, env in RENDER_KNOBS.items():
            knobs(env)
            img, _ = scene.render(width, height, spp, ts.SEED, policy, chunk=ch)
            assert_bits_equal(img, ref, "%s %s %s %s" % (name, variant, policy, label))
            same_as_first(name, variant, ("render", policy, label), img)
        knobs({})
        img, st = scene.render(width, height, spp, ts.SEED, policy, chunk=ch, counters=True)
        assert_bits_equal(img, ref, "%s %s %s counters" % (name, variant, policy))
        assert st["paths"] == width * height * spp == ost["paths"] and st["rays"] == ost["rays"]
    knobs({})
    ref, _ = ts.oracle_render(w, width, height, 2, "tile32", 0)
    img, _ = scene.render(width, height, 2, ts.SEED, "tile32")
    assert_bits_equal(img, ref, "%s %s tile32" % (name, variant))
    if name == "cluster":   # the reference's own pixels, at the size they were recorded at
        z = ts.golden("renders_cluster.npz")
        gw, gh, gspp, gchunk = ts.RENDER
        for policy, ch in ts.GOLDEN_RENDERS:
            img, _ = scene.render(gw, gh, gspp, ts.SEED, policy, chunk=ch if policy == "chunk" else 0)
            assert_bits_equal(img, z["%s_%dx%d_%dspp_c%d_s%d" % (policy, gw, gh, gspp, ch, ts.SEED)], "%s %s vs the reference" % (variant, policy))


@pytest.mark.parametrize("name,variant", [p for p in ts.PAIRS if p[0] in ("testscene", "cluster")],
                         ids=["%s-%s" % p for p in ts.PAIRS if p[0] in ("testscene", "cluster")])
def test_large_tree_policy_and_loop_exit_extremes(handle, knobs, name, variant):
    w, scene = handle(name, variant)
    width, height, spp, chunk = ts.GPU_RENDER
    for policy, ch in (("chunk", chunk), ("pixel", 0)):
        ref, _ = ts.oracle_render(w, width, height, spp, policy, ch)
        for env in LARGE_TREE if policy == "chunk" else LARGE_TREE[:1]:
            knobs(env)
            img, _ = scene.render(width, height, spp, ts.SEED, policy, chunk=ch)
            assert_bits_equal(img, ref, "%s %s %s %r" % (name, variant, policy, env))


@pytest.mark.parametrize("tables", ["lds", "hbm"])
@pairs
def test_ray_queries(handle, knobs, name, variant, tables):
    """ort_raycast, ort_occluded (limits at and one float either side of the hit), ort_radiance, ort_radiance_adaptive,
    ort_irradiance and ort_ambient_occlusion, with the tables in LDS and in HBM"""
    w, scene = handle(name, variant)
    knobs({} if tables == "lds" else {"ORT_LDS_TABLES": "0"})
    what = "%s %s tables in %s" % (name, variant, tables)
    rays, t, n, mat = ts.rays_of(w)
    if name == "cluster":
        ts.assert_cluster_conditions(w)
    hits, _ = scene.raycast(rays)
    assert_same_hits(hits, t, n, mat, what)
    counted, st = scene.raycast(rays, counters=True)
    assert st["rays"] == len(rays) and counted.tobytes() == hits.tobytes()
    same_as_first(name, variant, "raycast", hits["t"], hits["n"], hits["mat"])
    if name == "cluster":
        z = ts.golden("raycast_cluster.npz")
        assert z["rays"].tobytes() == rays.tobytes()
        assert_same_hits(hits, z["t"], z["n"], z["mat"], what + " vs the reference")
    tmax = ts.occluded_limits(t)
    got, _ = scene.occluded(rays, tmax)
    want = occluded_cases.expected(t, mat, tmax)
    assert (np.asarray(got).astype(bool) == want).all(), "%s: %d occlusion bytes differ" % (what, (np.asarray(got).astype(bool) != want).sum())
    got, _ = scene.occluded(rays, None)
    assert (np.asarray(got).astype(bool) == (mat != 0)).all()

    cases = ts.radiance_cases_of(w)
    rgb, states, _ = scene.radiance(cases.rays, cases.seeds, ts.RADIANCE_SPP, 0.8, want_states=True)
    radiance_cases.assert_same(rgb, states, *ts.radiance_expected(w), what + " radiance")
    ad = ts.RADIANCE_AD
    got = scene.radiance_adaptive(cases.rays, cases.seeds, ad.min_spp, ad.max_spp, ad.tolerance, ad.floor, ad.check_every, 0.8, want_states=True)
    adaptive_cases.assert_same(got[:4], ts.radiance_adaptive_expected(w), what + " adaptive radiance")
    same_as_first(name, variant, "radiance", rgb, states, got[1])

    pts = ts.points_of(w)
    rgb, states, _ = scene.irradiance(pts.points, pts.seeds, ts.IRR_SPP, 0.0, want_states=True)
    radiance_cases.assert_same(rgb, states, *ts.irradiance_expected(w), what + " irradiance")
    for radius in (None, ts.ao_radius(w)):
        got = scene.ambient_occlusion(pts.points, pts.seeds, ts.AO_SPP, radius, want_bent=True, want_states=True)
        ao_cases.assert_same(got[:3], ts.ao_expected(w, radius), what + " ambient occlusion")


@pytest.mark.parametrize("tables", ["lds", "hbm"])
@pairs
def test_camera_queries(api, handle, knobs, name, variant, tables):
    """ort_render_features, ort_render_follow (against follow_cases' chain; under no_prologue the counters build's node tests
    exceed the default tree's for the same rays), ort_render_views, ort_render_adaptive, ort_render_light_groups (one group per
    light material, against the dark twins of the world's flattened scene), ort_render_sample_map (the mixed map) and
    ort_render_accumulate (that map in two passes) on the small frames, with the tables in LDS and in HBM"""
    w, scene = handle(name, variant)
    knobs({} if tables == "lds" else {"ORT_LDS_TABLES": "0"})
    what = "%s %s tables in %s" % (name, variant, tables)
    width, height, spp = ts.FEATURES
    planes, _ = scene.render_features(width, height, spp, ts.SEED, want=feature_cases.PLANES)
    feature_cases.assert_same(planes, ts.features_expected(w), what + " features")
    same_as_first(name, variant, "features", *[planes[k] for k in ("albedo", "normal", "depth", "hits", "states")])
    # follow: the bounce rays start on a surface, so they are the fast walk's own and walk the variant's tree (glass_room's
    # default tree is one leaf: there they walk one only under the variants without, or with a small, prologue)
    ts.assert_follow_conditions(w)
    c = ts.follow_chain(w)
    followed, st = scene.render_follow(width, height, spp, ts.SEED, ts.FOLLOW[1], ts.FOLLOW[0], want=fw.PLANES, counters=True)
    fw.assert_same(followed, ts.follow_expected(w), what + " follow")
    fw.assert_prims(followed["ids"][None], [c], scene.raycast(c.last)[0]["prim"], what + " follow")
    assert st["rays"] == c.rays and st["paths"] == 0
    same_as_first(name, variant, "follow", *[followed[k] for k in fw.PLANES if k != "ids"])
    plain, _ = scene.render_follow(width, height, spp, ts.SEED, ts.FOLLOW[1], ts.FOLLOW[0], want=fw.PLANES)
    for k in fw.PLANES:
        assert np.ascontiguousarray(plain[k]).tobytes() == np.ascontiguousarray(followed[k]).tobytes(), "%s follow: %s with and without counters" % (what, k)
    if variant == "no_prologue":
        _, default = handle(name, "default")[1].render_follow(width, height, spp, ts.SEED, ts.FOLLOW[1], ts.FOLLOW[0], want=("hits",), counters=True)
        assert default["rays"] == st["rays"] and st["node_tests"] > default["node_tests"], (st["node_tests"], default["node_tests"])
    width, height, spp, chunk = ts.VIEWS
    cams = ts.view_cams(w)
    for policy, ch in (("chunk", chunk), ("pixel", 0)):
        frames, _ = scene.render_views(cams, ts.VIEW_SEEDS, width, height, spp, policy, chunk=ch)
        for v, (cam, seed) in enumerate(zip(cams, ts.VIEW_SEEDS)):
            ref, _ = ts.oracle_render(w, width, height, spp, policy, ch, cam=cam, seed=seed)
            assert_bits_equal(frames[v], ref, "%s views %s view %d" % (what, policy, v))
    ad = ts.RENDER_AD
    rgb, n, m2, fin, _ = scene.render_adaptive(width, height, ad.min_spp, ad.max_spp, ad.tolerance, ad.floor, ad.check_every, seed=ts.SEED, rr=rac.RR,
                                               want_states=True)
    rac.assert_same((rgb, n, m2, fin), ts.render_adaptive_expected(w), what + " adaptive render")
    same_as_first(name, variant, "render adaptive", rgb, n, m2, fin)
    groups, G = ts.light_groups_of(w)
    out = [np.full((G, height, width, 3), lg.GUARD_F, "<f4"), np.full((height, width, 3), lg.GUARD_F, "<f4"), np.full((height, width), lg.GUARD_STATE, "<u4")]
    frames, rgb, states, _ = scene.render_light_groups(width, height, spp, ts.SEED, ts.group_table(w), True, True, group_count=G, rr=lg.RR, out=out)
    for got, want, label in zip((frames, rgb, states), ts.light_groups_expected(w), ("group frames", "out_rgb", "final states")):
        lg.assert_plane(got, want, None, lg.GUARD_F, "%s light groups: %s" % (what, label))
    same_as_first(name, variant, "light groups", frames, rgb, states)
    smap, want = ts.sample_map_expected(w)
    got = scene.render_sample_map(width, height, smap, ts.MAP_CAP, ts.SEED, True, True, rr=sm.RR, out=sm.guards())[:3]
    sm.assert_planes(got, want, what + " sample map")
    same_as_first(name, variant, "sample map", *got)
    acc = ts.accumulate_passes(w, acs.library_call(api, ts.AccumulateCase(w, scene), counters=False), what)   # two passes, caps 1 and 3, against the chains folded
    same_as_first(name, variant, "accumulate", acc.sum, acc.m2, acc.count, acc.states)


@pairs
def test_accumulate_device_forms_and_views(api, handle, knobs, name, variant):
    """passes of 1 + 3 samples through the _device forms on a non-default stream, guard words around every plane and no
    synchronisation between them, against the oracle's chains folded; and ort_render_views_accumulate on the two views of
    tree_shapes.view_cams in the same passes against the oracle's chains from each camera"""
    w, scene = handle(name, variant)
    knobs({})
    c = ts.AccumulateCase(w, scene)
    what = "%s %s accumulate" % (name, variant)
    want = acs.Planes()
    for n in ts.ACCUMULATE_CAPS:
        acs.model(want, 0, ts.pixel_chains(w), None, n, None)
    got = acs.stream_split(c, ts.ACCUMULATE_CAPS, seed=ts.SEED)
    acs.assert_planes(got, want, what + ", the device forms on a stream")
    views = acs.views_split(acs.library_call(api, c), c, ts.view_cams(w), ts.VIEW_SEEDS, ts.ACCUMULATE_CAPS, what + ", views")
    same_as_first(name, variant, "accumulate on a stream and views", got.sum, got.m2, got.count, got.states, views.sum, views.m2, views.count, views.states)
