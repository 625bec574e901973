"""The render kernels added after the plain render, with more jobs than resident lanes: batches of views (loop_views),
pt_adaptive, pt_groups, pt_sample_map, feature_pixels, and the point queries' units (irradiance_points, ao_points), at
1024 x 768 -- 786 432 one-pixel jobs, three per resident lane of a 256-unit device.  Their own tests render 384 to 1 152 jobs:
there no lane runs a second job, no wave holds lanes on different jobs, and every ORT_JOB_BATCH plans what the unbatched run
plans (tests/test_many_jobs_host.py).  Here the persistent loop's job-to-job step runs -- the reset of AdaptState, the zeroing
of the group sums, the focal-point cache, the feature accumulators, draw_job called by part of a wave, a sample-map lane that
drops an empty job and draws a real one -- in the code objects of these families' own units.

Every comparison is bit for bit.  (a) Three 24 x 16 windows of the frame against the oracle (tests/many_jobs_cases.py).  (b) The
whole frame by identity against OTHER kernels: the plain PIXEL render, render_adaptive at min == max, the one-view batch,
ort_raycast.  Nothing is compared with the kernel under test's own output except the knob sweep, against the default run that
(a) and (b) have pinned.  That the frame is large enough is asserted from tools/launch_plan for this device's unit count
(planned()), never assumed."""
import numpy as np
import pytest

import ao_cases as ao
import feature_cases as fc
import irradiance_cases as ic
import light_groups_cases as lg
import many_jobs_cases as mj
import sample_map_cases as sm
from test_gpu_ao import torch_form as torch_ao
from test_gpu_irradiance import torch_irradiance
from test_launch_plan import tool  # noqa: F401 -- the fixture: tools/launch_plan, built as tests/test_launch_plan.py builds it

pytestmark = pytest.mark.gpu

W, H, SPP, CAP, SEED, RR, AD = mj.W, mj.H, mj.SPP, mj.CAP, mj.SEED, mj.RR, mj.AD
SCENES = mj.ROOMS + (mj.MESH,)
_plans, _default, _fixed = {}, {}, {}


@pytest.fixture()
def planned(tool):  # noqa: F811
    """the launch plans of every family on this device's unit count, asserted once: two jobs a lane, batches that batch"""
    import torch
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    if cu not in _plans:
        _plans[cu] = mj.plans(tool, cu)
        print("\n%d units, %d resident lanes\n%s" % (cu, mj.lanes(cu), mj.plans_report(_plans[cu])))
    return cu, _plans[cu]


@pytest.fixture()
def case(api, oracle, tmp_path_factory):
    def get(name):
        c = lg.case(api, oracle, name, tmp_path_factory)
        if c.scene.device is None:
            assert api.device_count() >= 1, "GPU test on a machine without a HIP device (the render path has no CPU fallback)"
            c.scene.upload(0)
        return c
    return get


@pytest.fixture()
def knobs(monkeypatch):
    def set_(env):
        for k in mj.KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    return set_


def sweep(knobs, family, run, default, samples):
    """every knob set: every plane byte-equal to the default run's; then counters: the same planes, paths the samples asked for"""
    for label, env in mj.KNOB_SETS.items():
        knobs(env)
        got, _ = run(False)
        for i, (g, d) in enumerate(zip(got, default)):
            mj.assert_same(g, d, "%s under %s %r: plane %d against the default run" % (family, label, env, i))
    knobs({})
    got, st = run(True)
    for i, (g, d) in enumerate(zip(got, default)):
        mj.assert_same(g, d, "%s with counters: plane %d against the default run" % (family, i))
    assert st["paths"] == samples, "%s with counters: %d paths, %d samples asked for" % (family, st["paths"], samples)


def fixed(c, k):
    """(rgb, m2, states) of k samples a pixel over the whole frame from the OTHER kernels: the plain PIXEL render's colours and,
    from k = 2 on, render_adaptive's planes at min_spp == max_spp == k (whose colours must be the render's); once per scene"""
    key = (c.name, k)
    if key not in _fixed:
        img, _ = c.scene.render(W, H, k, SEED, "pixel", rr=RR)
        m2 = states = None
        if k >= 2:
            rgb, n, m2, states, _ = c.scene.render_adaptive(W, H, k, k, 0.3, seed=SEED, rr=RR, want_states=True)
            assert (n == k).all()
            mj.assert_same(rgb, img, "%s: render_adaptive at min == max == %d against the PIXEL render" % (c.name, k))
        _fixed[key] = (img, m2, states)
    return _fixed[key]


def test_the_frame_is_large_enough_on_this_device(planned):
    cu, seen = planned
    assert seen[("light groups", "default")][0] >= 2 * 4 * cu * 256


# ---- light groups ----------------------------------------------------------------------------------------------------------------
def run_groups(c, groups, G, counters=False, cams=None, seeds=None):
    if cams is None:
        out = c.scene.render_light_groups(W, H, SPP, SEED, c.table(groups), True, True, group_count=G, rr=RR, counters=counters)
    else:
        out = c.scene.render_views_light_groups(cams, seeds, W, H, SPP, c.table(groups), True, True, group_count=G, rr=RR, counters=counters)
    return out[:3], out[3]


def default_groups(c):
    if ("groups", c.name) not in _default:
        _default[("groups", c.name)] = run_groups(c, c.per_light(), len(c.lights))[0]
    return _default[("groups", c.name)]


@pytest.mark.parametrize("name", SCENES)
def test_light_groups(planned, case, name):
    c = case(name)
    frames, rgb, states = default_groups(c)
    what = "light groups, %s" % name
    # (b) out_rgb is the PIXEL render; the states are render_adaptive's at min == max == 4
    img, _, fin = fixed(c, SPP)
    mj.assert_same(rgb, img, what + ": out_rgb against the PIXEL render")
    mj.assert_same(states, fin, what + ": final states against render_adaptive at min == max == 4")
    # ... all lights in one group: frame 0 is the render too
    (one, rgb1, _), _ = run_groups(c, {m: 0 for m in c.lights}, 1)
    mj.assert_same(one[0], img, what + ": every light in group 0, frame 0 against the PIXEL render")
    mj.assert_same(rgb1, img, what + ": every light in group 0, out_rgb")
    # ... one group per light: frame g is frame 0 of the call whose table holds that light alone
    for g, m in enumerate(c.lights):
        (alone, _, _), _ = run_groups(c, {m: 0}, 1)
        mj.assert_same(frames[g], alone[0], what + ": frame %d against frame 0 of the call with light %d alone" % (g, m))
    assert (frames != 0).any(axis=(1, 2, 3)).all()
    # (a) the windows: the oracle's renders of the dark twins and of the scene, and its chains' states
    for win in mj.WINDOWS:
        for g, m in enumerate(c.lights):
            mj.assert_window(frames[g], mj.window_frame(c, [m], SPP, win), win, what + ": frame %d against the dark twin" % g)
        mj.assert_window(rgb, mj.window_frame(c, None, SPP, win), win, what + ": out_rgb against the oracle")
        mj.assert_window(states, mj.window_planes(c, win, mj.Adaptive(SPP, SPP, 1, 0, 0))[3], win, what + ": final states against the oracle")


@pytest.mark.parametrize("name", ["room_all_lobes", mj.MESH])
def test_light_groups_knobs(planned, case, knobs, name):
    c = case(name)
    sweep(knobs, "light groups, %s" % name, lambda counters: run_groups(c, c.per_light(), len(c.lights), counters), default_groups(c), W * H * SPP)


# ---- the sample map ----------------------------------------------------------------------------------------------------------------
MAPS = {"full": mj.full_map, "sparse": mj.sparse_map}


def run_map(c, smap, counters=False, cams=None, seeds=None):
    """host form on guard-filled planes -> (rgb, m2, states), stats"""
    if cams is None:
        out = c.scene.render_sample_map(W, H, smap, CAP, SEED, True, True, rr=RR, counters=counters, out=sm.guards(None, size=mj.SIZE))
    else:
        out = c.scene.render_views_sample_map(cams, seeds, W, H, smap, CAP, True, True, rr=RR, counters=counters, out=sm.guards(len(cams), size=mj.SIZE))
    return out[:3], out[3]


def assert_map_planes(c, got, smap, what, whole_frame=fixed):
    """(b) over all 786 432 pixels: a pixel with n = k is the PIXEL render's at spp = k in colour and render_adaptive's at
    min == max == k in m2 and state (k = 1: the colour alone); every word where n == 0 holds its guard"""
    n = sm.counts(smap, CAP)
    rgb, m2, states = got
    classes = [0]
    for k in (1, 2, 4, 8):
        img, q, fin = whole_frame(c, k)
        at = n == k
        assert at.any()
        mj.assert_same(rgb, img, "%s: colour of the pixels with n = %d against the PIXEL render at spp = %d" % (what, k, k), at)
        if k >= 2:
            mj.assert_same(m2, q, "%s: m2 of the pixels with n = %d against render_adaptive at min == max == %d" % (what, k, k), at)
            mj.assert_same(states, fin, "%s: state of the pixels with n = %d against render_adaptive at min == max == %d" % (what, k, k), at)
        classes.append(k)
    assert set(np.unique(n).tolist()) == set(classes)
    empty = n == 0
    for plane, guard in zip(got, sm.guards(None, size=mj.SIZE)):
        mj.assert_same(plane, guard, what + ": the guard words where n == 0", empty)


@pytest.mark.parametrize("which", list(MAPS))
@pytest.mark.parametrize("name", SCENES)
def test_sample_map(planned, case, name, which):
    c = case(name)
    smap = MAPS[which]()
    mj.assert_full_map(smap) if which == "full" else mj.assert_sparse_map(smap)
    before = smap.copy()
    got, _ = run_map(c, smap)
    assert (smap == before).all(), "the host map was written"
    what = "sample map (%s), %s" % (which, name)
    _default[("map", which, name)] = got
    assert_map_planes(c, got, smap, what)
    n = sm.counts(smap, CAP)
    for win in mj.WINDOWS:   # (a) the oracle's chains cut at the map's counts, the guards where n == 0
        want = mj.window_planes(c, win, n)
        for plane, w_, label in zip(got, (want[0], want[2], want[3]), ("colours", "second moments", "final states")):
            mj.assert_window(plane, w_, win, "%s: %s against the oracle's chains" % (what, label))


@pytest.mark.parametrize("name,which", [("room_diffuse", "full"), (mj.MESH, "sparse")])
def test_sample_map_knobs(planned, case, knobs, name, which):
    c = case(name)
    smap = MAPS[which]()
    if ("map", which, name) not in _default:
        _default[("map", which, name)] = run_map(c, smap)[0]
    sweep(knobs, "sample map (%s), %s" % (which, name), lambda counters: run_map(c, smap, counters), _default[("map", which, name)],
          int(sm.counts(smap, CAP).sum(dtype=np.int64)))


# ---- the adaptive render -------------------------------------------------------------------------------------------------------------
def run_adaptive(c, counters=False):
    out = c.scene.render_adaptive(W, H, AD.min_spp, AD.max_spp, AD.tolerance, AD.floor, AD.check_every, seed=SEED, rr=RR, want_states=True, counters=counters)
    return out[:4], out[4]


@pytest.mark.parametrize("name", SCENES)
def test_adaptive(planned, case, name):
    c = case(name)
    mj.assert_adaptive_windows(c)   # from the oracle's chains: the rule cuts some pixels of every window and not others
    (rgb, spp, m2, states), _ = run_adaptive(c)
    _default[("adaptive", name)] = (rgb, spp, m2, states)
    what = "adaptive render, %s" % name
    assert set(np.unique(spp).tolist()) == {2, 4, 6, 8}, np.unique(spp)
    for k in (2, 4, 6, 8):   # (b) by selection: a pixel that stopped at k is the PIXEL render's at spp = k
        mj.assert_same(rgb, fixed(c, k)[0], "%s: colour of the pixels that stopped at %d against the PIXEL render at spp = %d" % (what, k, k), spp == k)
    # ... and its counts fed to the sample-map render give its planes back
    got, _ = run_map(c, spp)
    for plane, w_, label in zip(got, (rgb, m2, states), ("out_rgb", "out_m2", "final states")):
        mj.assert_same(plane, w_, "%s: %s against render_sample_map of its out_spp" % (what, label))
    for win in mj.ADAPTIVE_WINDOWS[name]:   # (a)
        for plane, w_, label in zip((rgb, spp, m2, states), mj.window_planes(c, win, AD), ("colours", "sample counts", "second moments", "final states")):
            mj.assert_window(plane, w_, win, "%s: %s against the rule on the oracle's chains" % (what, label))


@pytest.mark.parametrize("name", ["room_all_lobes", mj.MESH])
def test_adaptive_knobs(planned, case, knobs, name):
    c = case(name)
    if ("adaptive", name) not in _default:
        _default[("adaptive", name)] = run_adaptive(c)[0]
    default = _default[("adaptive", name)]
    sweep(knobs, "adaptive render, %s" % name, lambda counters: run_adaptive(c, counters), default, int(default[1].sum(dtype=np.int64)))


# ---- batches of views ------------------------------------------------------------------------------------------------------------------
POLICIES = {"pixel": ("pixel", 0), "chunk": ("chunk", 2)}


@pytest.mark.parametrize("policy", list(POLICIES))
@pytest.mark.parametrize("name", SCENES)
def test_views(api, planned, case, knobs, name, policy):
    """V = 2, the scene's own camera and batch_cameras' second on two seeds: each frame is the one-view batch of that camera,
    and its windows are the oracle's"""
    c = case(name)
    cams, seeds = mj.view_cameras(api, c), list(mj.VIEW_SEEDS)
    pol, chunk = POLICIES[policy]
    what = "views %s, %s" % (policy, name)
    frames, _ = c.scene.render_views(cams, seeds, W, H, SPP, pol, chunk=chunk, rr=RR)
    for v in range(2):
        one, _ = c.scene.render_views(cams[v:v + 1], seeds[v:v + 1], W, H, SPP, pol, chunk=chunk, rr=RR)
        mj.assert_same(frames[v], one[0], "%s: view %d against its one-view batch" % (what, v))
        for win in mj.WINDOWS:
            want = mj.window_frame(c, None, SPP, win, seeds[v], cams[v]) if pol == "pixel" else mj.window_chunk_frame(c, SPP, chunk, win, seeds[v], cams[v])
            mj.assert_window(frames[v], want, win, "%s: view %d against the oracle" % (what, v))
    assert frames[0].tobytes() != frames[1].tobytes()
    if name != "room_diffuse":
        def run(counters):
            out, st = c.scene.render_views(cams, seeds, W, H, SPP, pol, chunk=chunk, rr=RR, counters=counters)
            return (out,), st
        sweep(knobs, what, run, (frames,), 2 * W * H * SPP)


@pytest.mark.parametrize("name", ["room_all_lobes", mj.MESH])
def test_views_of_light_groups_and_sample_maps(api, planned, case, name):
    """V = 2 for the light-group and the sample-map forms, a map per view: view v is the single-view call's and the oracle's"""
    c = case(name)
    cams, seeds = mj.view_cameras(api, c), list(mj.VIEW_SEEDS)
    groups, G = c.per_light(), len(c.lights)
    (frames, rgb, states), _ = run_groups(c, groups, G, cams=cams, seeds=seeds)
    for v in range(2):
        what = "light groups, %s, view %d of 2" % (name, v)
        (f1, r1, s1), _ = run_groups(c, groups, G, cams=cams[v:v + 1], seeds=seeds[v:v + 1])
        for got, want, label in ((frames[v], f1[0], "group frames"), (rgb[v], r1[0], "out_rgb"), (states[v], s1[0], "final states")):
            mj.assert_same(got, want, "%s: %s against the one-view batch" % (what, label))
        for win in mj.WINDOWS:
            for g, m in enumerate(c.lights):
                mj.assert_window(frames[v][g], mj.window_frame(c, [m], SPP, win, seeds[v], cams[v]), win, what + ": frame %d against the dark twin" % g)
            mj.assert_window(rgb[v], mj.window_frame(c, None, SPP, win, seeds[v], cams[v]), win, what + ": out_rgb against the oracle")
    mj.assert_same(frames[0], default_groups(c)[0], "light groups, %s: view 0, the scene's own camera, against the single-frame call" % name)
    del frames, rgb, states
    maps = np.stack([mj.full_map(), mj.sparse_map(5)])
    before = maps.copy()
    got, _ = run_map(c, maps, cams=cams, seeds=seeds)
    assert (maps == before).all(), "the host maps were written"
    for v in range(2):
        what = "sample map, %s, view %d of 2" % (name, v)
        one, _ = run_map(c, maps[v:v + 1], cams=cams[v:v + 1], seeds=seeds[v:v + 1])
        n = sm.counts(maps[v], CAP)
        for plane, p1, label in zip(got, one, ("colours", "second moments", "final states")):
            mj.assert_same(plane[v], p1[0], "%s: %s against the one-view batch" % (what, label))
        for win in mj.WINDOWS:
            want = mj.window_planes(c, win, n, seeds[v], cams[v])
            for plane, w_, label in zip(got, (want[0], want[2], want[3]), ("colours", "second moments", "final states")):
                mj.assert_window(plane[v], w_, win, "%s: %s against the oracle's chains" % (what, label))
    assert_map_planes(c, tuple(p[0] for p in got), maps[0], "sample map, %s, view 0 of 2" % name)   # the scene's own camera and SEED


# ---- features ----------------------------------------------------------------------------------------------------------------------------
def run_features(c, spp, counters=False):
    planes, st = c.scene.render_features(W, H, spp, SEED, want=fc.PLANES, counters=counters)
    return planes, st


@pytest.mark.parametrize("name", ["room_all_lobes", mj.MESH])
def test_features(api, oracle, planned, case, knobs, name):
    """spp = 1: every plane is ort_raycast's record of the pixel's first camera ray, over the whole frame (identity 1 of
    tests/test_gpu_features.py, the rays from feature_cases.camera_rays); spp = 2: the windows are feature_cases' references"""
    import torch
    c = case(name)
    what = "features, %s" % name
    cam = c.camera(mj.SIZE)
    planes, _ = run_features(c, 1)
    rays, after = mj.first_rays(oracle, cam, SEED)
    dev = torch.device("cuda", 0)
    d_rays = torch.from_numpy(rays).to(dev)
    d_hits = torch.full((len(rays) * 24,), 0xAB, dtype=torch.uint8, device=dev)
    c.scene.raycast_device(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), want_stats=True)
    hits = d_hits.cpu().numpy().view(api.HIT_DTYPE).reshape(H, W)
    del d_rays, d_hits
    hit = hits["mat"] != 0
    assert hit.any()
    alb = fc.albedo_table(c.flat)
    mj.assert_same(planes["ids"][..., 0], hits["mat"], what + " spp 1: ids.mat against ort_raycast")
    mj.assert_same(planes["ids"][..., 1], hits["prim"], what + " spp 1: ids.prim against ort_raycast")
    # (the planes are sums that start at +0, divided by spp: a -0 component of ort_raycast's normal comes out +0, as include/ort.h's
    # "N starts at +0, N += h.n" and feature_cases.expected have it)
    mj.assert_same(planes["normal"], (np.zeros((H, W, 3), "<f4") + hits["n"]).astype("<f4"), what + " spp 1: normal against ort_raycast")
    mj.assert_same(planes["depth"], np.where(hit, hits["t"], np.float32(0)).astype("<f4"), what + " spp 1: depth against ort_raycast")
    mj.assert_same(planes["hits"], hit.astype("<u4"), what + " spp 1: hits against ort_raycast")
    mj.assert_same(planes["albedo"], np.where(hit[..., None], alb[hits["mat"]], np.float32(0)).astype("<f4"), what + " spp 1: albedo of ort_raycast's material")
    mj.assert_same(planes["states"], after.reshape(H, W), what + " spp 1: final states against the oracle's streams")
    assert len(np.unique(hits["mat"])) >= 4
    two, _ = run_features(c, 2)
    for win in mj.WINDOWS:
        f = fc.frame(oracle, c.twin(None), c.flat, cam, W, H, SEED, 2, win)
        for spp, got in ((1, planes), (2, two)):
            want = fc.expected(f, spp)
            fc.assert_same({k: mj.crop(v, win) for k, v in got.items()}, {k: mj.crop(v, win) for k, v in want.items()},
                           "%s spp %d, window %r (indices within the window)" % (what, spp, win))
    keys = list(fc.PLANES)
    for label, env in mj.KNOB_SETS.items():
        knobs(env)
        got, _ = run_features(c, 2)
        for k in keys:
            mj.assert_same(got[k], two[k], "%s spp 2 under %s %r: %s against the default run" % (what, label, env, k))
    knobs({})
    got, st = run_features(c, 2, counters=True)
    for k in keys:
        mj.assert_same(got[k], two[k], "%s spp 2 with counters: %s against the default run" % (what, k))
    assert st["rays"] == W * H * 2 and st["paths"] == 0, st


# ---- the point queries: a unit of their own ---------------------------------------------------------------------------------------------
_points = {}


def points_world(oracle, gpu_scene):
    """c3_bunny_room: 1 024 base points (the ambient-occlusion tests' world: the irradiance tests' point set and four axis
    points), their radii, the oracle's table and its closed form at rr = 0"""
    if "w" not in _points:
        scene = gpu_scene("c3_bunny_room")
        flat = scene.flatten(1, 1)
        w = ao.build("many jobs c3_bunny_room", scene, flat, oracle.OracleScene(flat, with_reference_csg=True), oracle, mj.POINTS - ao.AXIS_POINTS)
        assert len(w.pts.points) == mj.POINTS
        w.closed = ic.chain_closed_form(oracle, w.osc, flat, w.pts, AD.max_spp)
        _points["w"] = w
    return _points["w"]


def tiles_equal_the_first(planes, n, what):
    """every tile of 1 024 answers, the partial last one too, equals the first byte for byte"""
    for i, a in enumerate(planes):
        a = np.ascontiguousarray(a)
        first = a[:mj.POINTS]
        whole = (n // mj.POINTS) * mj.POINTS
        ne = (bits_rows(a[:whole]).reshape(n // mj.POINTS, mj.POINTS, -1) != bits_rows(first)[None]).any(axis=2)
        assert not ne.any(), "%s: output %d: tile %d differs from the first at its point %d" % ((what, i) + tuple(int(x) for x in np.argwhere(ne)[0]))
        ne = (bits_rows(a[whole:]) != bits_rows(first[:n - whole])).any(axis=1)
        assert not ne.any(), "%s: output %d: the last, partial tile differs from the first at its point %d" % (what, i, int(np.argwhere(ne)[0][0]))


def bits_rows(a):
    return np.ascontiguousarray(a).view("<u4").reshape(len(a), -1)


def test_point_queries(oracle, planned, gpu_scene, knobs):
    """irradiance_points, irradiance_adaptive_points and ao_points, the device forms, one launch each over 1 024 points tiled to
    three per resident lane and 257 more: the first tile is the oracle's, every other tile the first"""
    cu, seen = planned
    w = points_world(oracle, gpu_scene)
    n = mj.point_count(cu)
    assert seen[("irradiance points", "default")][0] == n
    idx = np.arange(n) % mj.POINTS
    pts, seeds, radii = w.pts.points[idx], w.pts.seeds[idx], w.radii[idx]
    ok = int(w.pts.ok[idx].sum())

    def irradiance(counters=False):
        got, st = torch_irradiance(w.scene, pts, seeds, mj.IRR_SPP, 0.0, counters=counters, want_stats=counters)
        return (got[0], got[3]), st

    def adaptive(counters=False):
        return torch_irradiance(w.scene, pts, seeds, 0, 0.0, ad=AD, counters=counters, want_stats=counters)

    def occlusion(counters=False):
        return torch_ao(w.scene, pts, seeds, radii, mj.AO_SPP, counters=counters, want_stats=counters)

    (rgb, fin), _ = irradiance()
    want = ic.expected_from(w.closed, w.pts, mj.IRR_SPP)
    ic.rc.assert_same(rgb[:mj.POINTS], fin[:mj.POINTS], *want, "irradiance points: the first tile against the oracle's closed form")
    tiles_equal_the_first((rgb, fin), n, "irradiance points")
    got, _ = adaptive()
    want = ic.expected_adaptive(w.closed, w.pts, AD)
    assert len(set(want[1][w.pts.ok].tolist())) >= 2
    ic.ac.assert_same(tuple(a[:mj.POINTS] for a in got), want, "adaptive irradiance points: the first tile against the rule on the closed form")
    tiles_equal_the_first(got, n, "adaptive irradiance points")
    occ, _ = occlusion()
    ao.assert_same(tuple(a[:mj.POINTS] for a in occ), ao.expected(w, w.radii, mj.AO_SPP), "ao points: the first tile against the oracle")
    tiles_equal_the_first(occ, n, "ao points")
    mixed = ao.bits(w, w.radii, mj.AO_SPP)[w.pts.ok]
    assert mixed.any() and not mixed.all()
    sweep(knobs, "irradiance points", irradiance, (rgb, fin), ok * mj.IRR_SPP)
    sweep(knobs, "adaptive irradiance points", adaptive, got, int(got[1].sum(dtype=np.int64)))
    for label, env in mj.KNOB_SETS.items():
        knobs(env)
        again, _ = occlusion()
        for i, (g, d) in enumerate(zip(again, occ)):
            assert bits_rows(g).tobytes() == bits_rows(d).tobytes(), "ao points under %s %r: output %d differs from the default run's" % (label, env, i)
    knobs({})
    again, st = occlusion(True)
    assert all(bits_rows(g).tobytes() == bits_rows(d).tobytes() for g, d in zip(again, occ)) and st["rays"] == ok * mj.AO_SPP, st
