"""The traversal stack past its LDS entries, on the host: every kernel walks the fast tree with a per-lane stack whose first
entries live in LDS and whose tail lives in scratch (csrc/ort_lane.h: 24 + 40 entries in the four-waves units, 20 + 44 in
ort_kernels_w5.hip, 16 + 48 in the wavefront trace, four LDS entries fewer in resolve_hit's re-traversal, up to three
entries a level in the wide tree).  The repository's scenes never get past entry 10; the scene of tools/make_deepscene.py
(tests/deep_scenes.py) takes nearly every ray into the tail, six entries at the deepest, and its cylinders send rays through the re-traversal.

tools/host_sim (the four-waves split) and tools/host_sim_w5 (the same sources with the five-waves unit's split) run the
lane code on that scene: ray queries, radiance, renders, a batch of views, the wavefront schedule and the wide tree, with
the tables from their arrays and from the LDS image, and with one ray in sixteen re-cast exactly -- all bit for bit against
the oracle.  One-off mutation checks of this file are recorded in profiles/r15_deep_stack.md."""
import numpy as np
import pytest

import ao_cases
import deep_scenes as ds
import host_sim_tool as hs
import irradiance_cases
import occluded_cases
import radiance_cases
from conftest import assert_bits_equal

TABS = {"SIM_TABS": "1"}
SOME_EXACT = {"SIM_FORCE_FALLBACK": "0xf"}
ENVS = [{}, TABS, SOME_EXACT]
ids = lambda e: "+".join(sorted(e)) or "plain" if isinstance(e, dict) else str(e)


@pytest.fixture(scope="module")
def w(api, oracle, tmp_path_factory):
    return ds.world(api, oracle, tmp_path_factory)


def test_text_and_arrays_are_one_scene(api, w):
    """what host_sim loads (.scn + PLY) is what the library gets as arrays, bit for bit: the oracle's scene is both"""
    flat = api.Scene.load_scn(w.scn).flatten(*ds.GPU_RENDER[:2])
    for k in ("materials", "spheres", "boxes", "cylinders", "lights", "camera", "ambient"):
        assert getattr(flat, k).tobytes() == getattr(w.flat, k).tobytes(), k
    assert len(flat.meshes) == len(w.flat.meshes) == 2
    for a, b in zip(flat.meshes, w.flat.meshes):
        assert a["mat"] == b["mat"] and all(a[k].tobytes() == b[k].tobytes() for k in ("vertices", "indices", "aabb_min", "aabb_max"))


def test_the_scene_reaches_the_scratch_tail(w):
    ds.assert_conditions(w)


@pytest.mark.parametrize("env", ENVS, ids=ids)
@pytest.mark.parametrize("rays", ["cone", "grazing"])
@pytest.mark.parametrize("tool", ds.TOOLS)
def test_raycast(w, tool, rays, env):
    """grazing: rays at the cylinders' silhouettes, a few hundred of which resolve_hit traverses a second time"""
    rr, (t, n, mat) = (w.rays, (w.t, w.n, w.mat)) if rays == "cone" else (w.graze, w.graze_hits)
    hits, r = hs.raycast(hs.built(tool), w.dir, w.scn, rr, base=w.base, env=env, threads=8)
    assert_bits_equal(hits["t"], t, "t")
    assert_bits_equal(hits["n"], n, "normals")
    assert (hits["mat"] == mat).all()
    c = hs.counters(r)
    assert c["rays"] == len(rr) and (0 < c["fallback"] < c["rays"] if env == SOME_EXACT else c["fallback"] * 20 <= c["rays"])


@pytest.mark.parametrize("env", ENVS, ids=ids)
@pytest.mark.parametrize("tool", ds.TOOLS)
def test_occluded_at_and_one_ulp_either_side_of_the_hit(w, tool, env):
    k = np.arange(len(w.t)) % 3
    tmax = np.where(k == 0, w.t, np.where(k == 1, np.nextafter(w.t, np.float32(-np.inf)), np.nextafter(w.t, np.float32(np.inf)))).astype("<f4")
    want = occluded_cases.expected(w.t, w.mat, tmax)
    assert want.mean() > 0.3 and (~want).mean() > 0.6
    got = hs.occluded(hs.built(tool), w.dir, w.scn, w.rays, tmax, w.base, env=env, threads=8)
    assert (got == want.astype(np.uint8)).all(), "%d bytes differ" % (got != want.astype(np.uint8)).sum()
    got = hs.occluded(hs.built(tool), w.dir, w.scn, w.rays, None, w.base, env=env, threads=8)
    assert (got == 1).all()


@pytest.mark.parametrize("env", ENVS, ids=ids)
@pytest.mark.parametrize("tool", ds.TOOLS)
def test_radiance(w, tool, env):
    want_rgb, want_states = ds.radiance_expected(w, 2)
    assert (want_rgb != 0).any(axis=1).mean() >= 0.10
    rgb, states = hs.radiance(hs.built(tool), w.dir, w.scn, w.prays, w.pseeds, 2, 0.8, w.base, env=env, threads=8)
    radiance_cases.assert_same(rgb, states, want_rgb, want_states, "%s %r" % (tool, env))


@pytest.mark.parametrize("env", ENVS, ids=ids)
@pytest.mark.parametrize("tool", ds.TOOLS)
def test_irradiance(w, tool, env):
    want_rgb, want_states = ds.irradiance_expected(w, 2)
    rgb, states, _ = irradiance_cases.host_sim(hs.built(tool), w.dir, w.scn, w.points.points, w.points.seeds, 2, 0.8, w.base, env=env, threads=8)
    radiance_cases.assert_same(rgb, states, want_rgb, want_states, "%s %r" % (tool, env))


@pytest.mark.parametrize("env", ENVS, ids=ids)
@pytest.mark.parametrize("radius", ["none", "per point"])
@pytest.mark.parametrize("tool", ds.TOOLS)
def test_ambient_occlusion(w, tool, radius, env):
    radius = None if radius == "none" else ds.ao_radius(w)
    want = ds.ao_expected(w, radius)
    occluded = 1 - want[0].mean() / ds.AO_SPP
    assert occluded == 1 if radius is None else 0.1 < occluded < 0.9, occluded   # the room is closed; within a radius some of each
    got = ao_cases.host_sim(hs.built(tool), w.dir, w.scn, w.points.points, w.points.seeds, radius, ds.AO_SPP, base=w.base, env=env, threads=8)
    ao_cases.assert_same(got[:3], want, "%s %r" % (tool, env))


# SIM_WIDE: the 4-wide tree, up to three stacked entries a level; SIM_WAVEFRONT: the wavefront trace's own split, 16 + 48,
# whichever tool runs it, so only the first tool does
RENDER_ENVS = [(t, e) for t in ds.TOOLS for e in ENVS + [{"SIM_WIDE": "1"}, dict(TABS, SIM_WIDE="1")]] + [(ds.TOOLS[0], {"SIM_WAVEFRONT": "100"})]


@pytest.mark.parametrize("tool,env", RENDER_ENVS, ids=lambda v: v if isinstance(v, str) else ids(v))
@pytest.mark.parametrize("policy", ["pixel", "chunk"])
@pytest.mark.parametrize("camera", ["cone", "grazing"])
def test_render(w, camera, policy, tool, env):
    """cone: the scene's own camera.  grazing: the same scene under a camera that looks at a cylinder's silhouette, so that the
    frame's rays are re-traversed by resolve_hit by the hundred, with the re-traversal's stack past its LDS entries"""
    width, height, spp, chunk = ds.RENDER
    chunk = chunk if policy == "chunk" else 0
    scn = w.scn if camera == "cone" else w.graze_scn
    ref, _ = ds.oracle_render(w, width, height, spp, policy, chunk, cam=None if camera == "cone" else ds.graze_cam(w, width, height))
    args, outs = hs.render_args(w.dir, scn, width, height, spp, ds.SEED, policy, chunk, w.base)
    r = hs.run(hs.built(tool), args, env=env, threads=1 if "SIM_WAVEFRONT" in env else 8)
    got = np.fromfile(outs[0], "<f4").reshape(height, width, 3)
    assert_bits_equal(got, ref, "%s %s %s %r" % (camera, tool, policy, env))
    probe = hs.stack_probe(r)
    assert probe[0]["deepest"] > probe[0]["lds"] and probe[0]["scratch_pops"] > 0, probe   # this run, too, was in the tail
    if camera == "grazing":
        assert probe[1]["lds"] == probe[0]["lds"] - 4 and probe[1]["above"] >= 100, probe   # and its re-traversals


@pytest.mark.parametrize("policy", ["pixel", "chunk"])
@pytest.mark.parametrize("tool", ds.TOOLS)
def test_views(api, w, tool, policy):
    width, height, spp, chunk = ds.RENDER
    chunk = chunk if policy == "chunk" else 0
    cams = ds.view_cams(api, w, width, height)
    frames = hs.views(hs.built(tool), w.dir, w.scn, cams, ds.VIEW_SEEDS, width, height, spp, policy, chunk, w.base, threads=8)
    for v, (cam, seed) in enumerate(zip(cams, ds.VIEW_SEEDS)):
        ref, _ = ds.oracle_render(w, width, height, spp, policy, chunk, cam=cam, seed=seed)
        assert_bits_equal(frames[v], ref, "%s %s view %d" % (tool, policy, v))


def test_the_culling_slack_bounds_how_early_a_triangle_hit_may_be(api, oracle, w, tmp_path):
    """A LIMIT OF THE FAST WALK, stated: it skips a node whose box the ray enters at or beyond 1.0002 x the best distance so far
    (kCullSlack), which allows the distance the reference's triangle test computes to precede the
    triangle's own plane by 2e-4 of itself.  The same scene with every wedge listed from its far tip (two long, nearly parallel
    edges: the computed distance is off by up to 1e-3) goes past that.  Closest hits still agree with the oracle on every ray
    (an unbounded walk meets the box before it has a nearer best), and so does ort_occluded's exact walk.  Its bounded walk, with
    the limit one float past the hit, misses hits -- and exactly among the rays whose hit is that early, never another one, and
    never by reporting a hit that is not there."""
    tool = hs.built(ds.TOOLS[0])
    scn, L = ds.make_deepscene.write_scene(str(tmp_path), tip_first=True)
    base = str(tmp_path) + "/"
    scene = api.Scene.load_scn(scn)
    osc = oracle.OracleScene(scene.flatten(8, 8), with_reference_csg=True)
    t, n, mat = osc.raycast(w.rays[:, 0:3], w.rays[:, 3:6])
    hits, _ = hs.raycast(tool, tmp_path, scn, w.rays, base=base, threads=8)
    assert_bits_equal(hits["t"], t, "t")
    assert_bits_equal(hits["n"], n, "normals")
    assert (hits["mat"] == mat).all()
    kind, index = api.decode_prim(hits["prim"])
    inner = (mat == ds.make_deepscene.MAT_INNER) & (kind == api.HIT_TRIANGLE) & (index < len(L["xs_inner"]))
    assert inner.sum() == (mat == ds.make_deepscene.MAT_INNER).sum() > 1000
    plane = np.where(inner, (L["xs_inner"][np.where(inner, index, 0)] - w.rays[:, 0].astype(np.float64)) / w.rays[:, 3].astype(np.float64), t)
    early = (plane - t) / plane                      # by how much of itself the computed distance precedes the plane
    assert (early > 2.1e-4).sum() >= 20 and early.max() < 2e-3, (np.sort(early)[-25:],)
    tmax = np.nextafter(t, np.float32(np.inf))
    want = occluded_cases.expected(t, mat, tmax).astype(np.uint8)
    assert want.all()
    exact = hs.occluded(tool, tmp_path, scn, w.rays, tmax, base, env={"SIM_FORCE_FALLBACK": "0"}, threads=8)
    assert (exact == want).all()
    fast = hs.occluded(tool, tmp_path, scn, w.rays, tmax, base, threads=8)
    missed = fast != want
    assert (early[missed] > 1.9e-4).all(), "a hit no earlier than the slack allows was missed: %r" % (np.sort(early[missed])[:5],)
    print("bounded walk: %d of %d hits missed, all among the %d rays whose hit precedes its plane by more than 1.9e-4" %
          (missed.sum(), len(missed), (early > 1.9e-4).sum()))


# the light-group and sample-map lanes (pt_groups, pt_sample_map): a unit of their own on the device
@pytest.mark.parametrize("env", ENVS, ids=ids)
@pytest.mark.parametrize("tool", ds.TOOLS)
def test_light_groups(w, tmp_path, tool, env):
    """the scene's one light material in group 5 of 8: frame 5, out_rgb and the states are the oracle's PIXEL render, the other
    seven frames +0 in every word"""
    import light_groups_cases as lg
    width, height, spp, _ = ds.RENDER
    assert (lg.W, lg.H) == (width, height)
    frames, rgb, states = lg.host_light_groups(hs.built(tool), tmp_path, lg.SceneRef(w.scn, w.base), ds.group_table(w), ds.LIGHT_GROUPS[0], spp,
                                               seed=ds.SEED, env=env, threads=8)
    want = ds.light_groups_expected(w)
    assert (want[1] != 0).any()
    for got, w_, label in zip((frames[0], rgb[0], states[0]), want, ("group frames", "out_rgb", "final states")):
        lg.assert_plane(got, w_, None, lg.GUARD_F, "%s %r: %s" % (tool, env, label))


@pytest.mark.parametrize("env", ENVS, ids=ids)
@pytest.mark.parametrize("tool", ds.TOOLS)
def test_sample_map(w, tmp_path, tool, env):
    import light_groups_cases as lg
    import sample_map_cases as sm
    smap, want = ds.sample_map_expected(w)
    got, _ = sm.host_sample_map(hs.built(tool), tmp_path, lg.SceneRef(w.scn, w.base), smap, ds.MAP_CAP, seed=ds.SEED, env=env, threads=8)
    sm.assert_planes(tuple(p[0] for p in got), want, "%s %r" % (tool, env))
    assert (sm.counts(smap, ds.MAP_CAP) == ds.MAP_CAP).any() and (want[0] != sm.GUARD_RGB).any()
