"""Ambient-occlusion queries (ort_ambient_occlusion and its device form), host side: the point sets and radii shown not to be
vacuous from the oracle alone, the C ABI surface and its errors in the order include/ort.h gives them, and the lane code run on
host threads (tools/host_sim --ambient-occlusion, ao_lane with and without the LDS table, plain and under ASan + UBSan) against
the oracle, all bits (tests/ao_cases.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ao_cases as ao
import host_sim_tool as hs
import irradiance_cases as ic
import occluded_cases as oc
import radiance_cases as rc
from conftest import DATA
from host_cases import aligned as _aligned, scene as _scene

NAMES = {"ort_ambient_occlusion", "ort_ambient_occlusion_device"}
SCENES = {"testscene": 128, "c2_analytic": 128, "c3_bunny_room": 64}
TABS = [{}, {"SIM_TABS": "1"}]
_worlds = {}


@pytest.fixture(scope="module")
def host_sim():
    return hs.built("host_sim")


@pytest.fixture()
def world(oracle, load_scene):
    """name -> the scene's points, radii and the oracle's table of 8 samples per point; computed once"""
    def get(name):
        if name not in _worlds:
            scene = load_scene(name)
            flat = scene.flatten(1, 1)
            _worlds[name] = ao.build(name, scene, flat, oracle.OracleScene(flat), oracle, SCENES[name])
        return _worlds[name]
    return get


# ---- 1. the point sets and the radii, from the oracle alone -------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_point_sets_are_not_vacuous(world, name):
    """8 samples at radius R = 0.1 x the diagonal, of the point_set's points inside the domain: at least 0.25 have both an open and
    an occluded sample, at least 0.10 are all open, at least 0.05 all occluded; the radius array holds every kind it promises; the
    axis points' first direction has a +-0 component"""
    w = world(name)
    p = w.pts
    mixed, all_open, all_occ = ao.classes(w, w.R)
    print("%s: %d points in the set, mixed %.3f, all open %.3f, all occluded %.3f; without a radius all occluded %.3f"
          % (name, w.base, mixed, all_open, all_occ, ao.classes(w, None)[2]))
    assert mixed >= 0.25 and all_open >= 0.10 and all_occ >= 0.05
    assert w.R == np.float32(0.1 * np.linalg.norm(np.asarray(w.hi, np.float64) - np.asarray(w.lo, np.float64)))
    r = w.radii
    assert (r == w.R).sum() > len(r) // 2
    for v in (np.inf, 0.0, -1.0, oc.FLT_MAX, np.float32(0.4 * w.diag)):
        assert (r == np.float32(v)).sum() >= 2, v
    assert np.isnan(r).sum() >= 2
    # the points at their own hit distances: inside the domain, and each of the three rungs flips or keeps exactly that sample
    assert len(w.own) >= 16 and p.ok[w.own].all()
    at = below = above = 0
    for i in w.own:
        hit = w.mat[i] != 0
        with np.errstate(over="ignore"):
            up = np.nextafter(w.t[i], np.float32(np.inf))
        at += int(((w.t[i] == r[i]) & hit).any())
        below += int(((np.nextafter(w.t[i], np.float32(0)) == r[i]) & hit).any())
        above += int(((up == r[i]) & hit).any())
    assert at >= 5 and below >= 5 and above >= 5
    open_at, open_r = ao.expected(w, r, 8)[0][w.own], ao.expected(w, w.R, 8)[0][w.own]
    assert (open_at != open_r).any()
    # the axis points: d_0 is the normal itself, so two of its components are +-0
    axis = np.arange(w.base, len(p.points))
    assert len(axis) >= 4 and p.ok[axis].all() and not p.far[axis].any()
    assert (p.seeds[axis] == rc.unstep(0xFFFFFFFF)).all() and (np.abs(p.points[axis, 5]) == 1).all() and (p.points[axis, 3:5] == 0).all()
    assert ((w.d[axis, 0] == 0).sum(axis=1) == 2).all() and (w.d[axis, 0, 2] == p.points[axis, 5]).all()
    assert not (w.d[:w.base][p.ok[:w.base]] == 0).any()   # no drawn direction of the point_set itself has a zero component


# ---- 2. the C ABI -----------------------------------------------------------------------------------------------------------------
def test_entry_points_have_c_linkage(api):
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NAMES <= names
    assert NAMES <= set(api.EXPORTS)
    hdr = open(os.path.join(os.path.dirname(DATA), "include", "ort.h")).read()
    assert all(n + "(" in hdr for n in NAMES)
    assert "#define ORT_AO_INVALID 0xffffffffu" in hdr and api.AO_INVALID == 0xFFFFFFFF
    assert api.lib().ort_abi_version() == 3   # additive: the ABI version stands


def _caller(api, device_form):
    L = api.lib()

    def call(handle, pts, seeds, radius, n, spp, out, bent, states, flags=0, stats=None):
        if device_form:
            return L.ort_ambient_occlusion_device(handle, pts, seeds, radius, n, spp, out, bent, states, flags, None, stats)
        return L.ort_ambient_occlusion(handle, pts, seeds, radius, n, spp, out, bent, states, flags, stats)
    return call


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("committed", [True, False])
def test_errors_come_in_order(api, device_form, committed):
    """INVALID (nulls, then misaligned pointers, then spp == 0), then STATE before NO_DEVICE, on a scene that is not uploaded"""
    s = _scene(api, committed)
    L = api.lib()
    call = _caller(api, device_form)
    keep = [_aligned(4 * 24), _aligned(16), _aligned(16), _aligned(16), _aligned(48), _aligned(16)]
    pts, seeds, rad, out, bent, fin = (k[1] for k in keep)
    state = api.ERR_NO_DEVICE if committed else api.ERR_STATE
    assert call(None, pts, seeds, rad, 4, 1, out, bent, fin) == api.ERR_INVALID
    assert call(s.handle, None, seeds, rad, 4, 1, out, bent, fin) == api.ERR_INVALID
    assert b"points" in L.ort_last_error()
    assert call(s.handle, pts, None, rad, 4, 1, out, bent, fin) == api.ERR_INVALID
    assert call(s.handle, pts, seeds, rad, 4, 1, None, bent, fin) == api.ERR_INVALID
    assert call(s.handle, pts + 4, seeds, rad, 4, 0, None, bent, fin) == api.ERR_INVALID     # a null comes before a misaligned pointer
    assert b"null" in L.ort_last_error()
    for p_, sd, r_, o, b, f in ((pts + 4, seeds, rad, out, bent, fin), (pts, seeds + 2, rad, out, bent, fin), (pts, seeds, rad + 1, out, bent, fin),
                                (pts, seeds, rad, out + 2, bent, fin), (pts, seeds, rad, out, bent + 1, fin), (pts, seeds, rad, out, bent, fin + 2),
                                (pts + 2, seeds, None, out, None, None)):
        assert call(s.handle, p_, sd, r_, 4, 0, o, b, f) == api.ERR_INVALID                   # a misaligned pointer comes before spp
        assert b"aligned" in L.ort_last_error()
    assert call(s.handle, pts, seeds, rad, 4, 0, out, bent, fin) == api.ERR_INVALID
    assert b"spp" in L.ort_last_error()                                                       # ... and spp before the scene's state
    assert call(s.handle, pts + 8, seeds + 4, None, 4, 3, out + 4, None, None) == state
    assert call(s.handle, pts, seeds, rad, 4, 1, out, bent, fin, api.RENDER_COUNTERS) == state
    assert (b"commit" if not committed else b"upload") in L.ort_last_error()


@pytest.mark.parametrize("device_form", [False, True])
def test_empty_batch_is_ok(api, device_form):
    """count == 0: ORT_OK without a launch, with every other argument bad"""
    call = _caller(api, device_form)
    keep_r, p = _aligned(24)
    for s in (_scene(api), _scene(api, committed=False)):
        assert call(s.handle, None, None, None, 0, 0, None, None, None) == api.OK
        assert call(s.handle, p + 1, p + 1, p + 1, 0, 0, p + 1, p + 1, p + 1) == api.OK
    assert call(None, None, None, None, 0, 0, None, None, None) == api.OK
    st = api.Stats()
    st.rays = 7
    assert call(_scene(api).handle, None, None, None, 0, 1, None, None, None, 0, ctypes.byref(st)) == api.OK
    assert st.rays == 0


def test_python_shapes(api):
    s = _scene(api)
    pts = np.zeros((3, 6), "<f4")
    for bad in (np.zeros((3, 5), "<f4"), np.zeros(6, "<f4")):
        with pytest.raises(ValueError):
            s.ambient_occlusion(bad, np.ones(len(bad), "<u4"), 1)
    with pytest.raises(ValueError):
        s.ambient_occlusion(pts, np.ones(2, "<u4"), 1)
    with pytest.raises(ValueError):
        s.ambient_occlusion(pts, np.ones(3, "<u4"), 1, radius=np.ones(2, "<f4"))
    for kw in ({}, {"radius": 0.5}, {"radius": np.ones(3), "want_bent": True, "want_states": True}):
        with pytest.raises(api.OrtError) as e:
            s.ambient_occlusion(pts, np.ones(3, "<u4"), 2, **kw)
        assert e.value.code == api.ERR_NO_DEVICE
    with pytest.raises(api.OrtError) as e:
        s.ambient_occlusion(pts, np.ones(3, "<u4"), 0)
    assert e.value.code == api.ERR_INVALID
    out, bent, states, st = s.ambient_occlusion(np.zeros((0, 6), "<f4"), np.zeros(0, "<u4"), 4, want_bent=True, want_states=True)
    assert out.shape == (0,) and out.dtype == np.dtype("<u4") and bent.shape == (0, 3) and states.shape == (0,) and st["rays"] == 0
    assert len(s.ambient_occlusion(np.zeros((0, 6), "<f4"), np.zeros(0, "<u4"), 4)) == 2
    with pytest.raises(api.OrtError) as e:
        s.ambient_occlusion_device(64, 64, 0, 4, 1, 64)
    assert e.value.code == api.ERR_NO_DEVICE


# ---- 3. the lane code on host threads -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_host_sim_is_the_oracles_answer(host_sim, world, tmp_path, name):
    """spp 1 and 8; the radius array, all-R and no radius; the prologue's shapes from the LDS table's image and from their array;
    each optional output absent in turn; the counters' rays; the axis points' first sample takes the exact walk where the tree
    holds boxes"""
    w = world(name)
    p = w.pts
    inside = int(p.ok.sum())
    for spp in (1, 8):
        for what, radius in (("radii", w.radii), ("all R", np.full(len(p.points), w.R, "<f4")), ("no radius", None)):
            want = ao.expected(w, radius, spp)
            for k, env in enumerate(TABS):
                got = ao.host_sim(host_sim, tmp_path, name, p.points, p.seeds, radius, spp, env=env, threads=8 if k == 0 else 3)
                ao.assert_same(got[:3], want, "%s %s spp %d %r" % (name, what, spp, env))
                c = hs.counters(got[3])
                assert c["rays"] == inside * spp and c["paths"] == 0
        assert (want[0][p.ok] <= spp).all() and (want[0][~p.ok] == ao.AO_INVALID).all()
    want = ao.expected(w, w.radii, 8)
    for bent, states in ((False, True), (True, False), (False, False)):
        got = ao.host_sim(host_sim, tmp_path, name, p.points, p.seeds, w.radii, 8, want_bent=bent, want_states=states, threads=8)
        assert (got[1] is None) == (not bent) and (got[2] is None) == (not states)
        ao.assert_same(got[:3], want, "%s without %s" % (name, "both" if not (bent or states) else "bent" if not bent else "states"))
    # one thread, the points in another order: a point's answer is its own
    perm = np.random.default_rng(4).permutation(len(p.points))
    got = ao.host_sim(host_sim, tmp_path, name, p.points[perm], p.seeds[perm], w.radii[perm], 8, threads=1)
    ao.assert_same(got[:3], tuple(a[perm] for a in want), name + " permuted")
    # the axis points alone, one sample at radius R: d_0 has two +-0 components
    axis = np.arange(w.base, len(p.points))
    got = ao.host_sim(host_sim, tmp_path, name, p.points[axis], p.seeds[axis], np.full(len(axis), w.R, "<f4"), 1)
    ao.assert_same(got[:3], ao.expected(w, w.R, 1, axis), name + " axis points")


def test_axis_samples_fall_back_with_boxes_in_the_tree(host_sim, api, world, tmp_path):
    """c2_analytic: a +-0 component of d_0 sends that sample to the exact walk when the fast tree holds boxes.  As the scene commits
    by itself all nine boxes sit in the analytic prologue (the cheapest kind goes first), so the rule does not apply; committed under
    ORT_ANALYTIC_PROLOGUE=0 every box is in the tree, and fallback counts the sample.  The bits are the oracle's both ways"""
    w = world("c2_analytic")
    p = w.pts
    assert w.scene.tree_info()["prologue_prims"] >= w.scene.info().box_count > 0
    axis = np.arange(w.base, len(p.points))
    radius = np.full(len(axis), w.R, "<f4")
    want = ao.expected(w, w.R, 1, axis)
    assert ((w.d[axis, 0] == 0).sum(axis=1) == 2).all()
    for tabs in TABS:
        got = ao.host_sim(host_sim, tmp_path, "c2_analytic", p.points[axis], p.seeds[axis], radius, 1, env=dict(tabs, ORT_ANALYTIC_PROLOGUE="0"))
        ao.assert_same(got[:3], want, "axis points, boxes in the tree %r" % tabs)
        c = hs.counters(got[3])
        assert c["rays"] == len(axis) and c["fallback"] >= len(axis)
    got = ao.host_sim(host_sim, tmp_path, "c2_analytic", p.points, p.seeds, w.radii, 8, env={"ORT_ANALYTIC_PROLOGUE": "0"}, threads=8)
    ao.assert_same(got[:3], ao.expected(w, w.radii, 8), "all points, boxes in the tree")
    with np.errstate(invalid="ignore"):
        live = w.radii > 0   # a point whose radius is NaN or <= 0 traverses nothing, so it cannot fall back
    assert hs.counters(got[3])["fallback"] >= int(live[axis].sum()) + 8 * int((p.far & live).sum()) > 0


def test_final_states_do_not_depend_on_the_scene(host_sim, world, tmp_path):
    """testscene's points and seeds run in c2_analytic: other counts, the same final states -- two steps per sample, whatever is hit"""
    w = world("testscene")
    p = w.pts
    got = ao.host_sim(host_sim, tmp_path, "c2_analytic", p.points, p.seeds, w.radii, 8, want_bent=False, threads=8)
    want = ao.expected(w, w.radii, 8)
    ao.assert_same((None, None, got[2]), want, "testscene's points in c2_analytic")
    assert (got[0] != want[0]).any() and ((got[0] == ao.AO_INVALID) == (want[0] == ao.AO_INVALID)).all()
    steps = np.array([int(s) or 1 for s in p.seeds], np.uint64)
    for _ in range(16):
        steps = np.array([rc.step(int(x)) for x in steps], np.uint64)
    assert (got[2][p.ok] == steps[p.ok].astype("<u4")).all()


def test_far_points_fall_back(host_sim, world, tmp_path):
    """c2_analytic holds quadrics in its tree: every sample of a point outside the scene's box takes the exact walk, the near ones
    do not"""
    w = world("c2_analytic")
    p = w.pts
    far = np.flatnonzero(p.far)
    assert len(far) == 8
    for radius in (np.full(len(far), w.R, "<f4"), None):
        got = ao.host_sim(host_sim, tmp_path, "c2_analytic", p.points[far], p.seeds[far], radius, 8, threads=4)
        ao.assert_same(got[:3], ao.expected(w, None if radius is None else w.R, 8, far), "far points")
        c = hs.counters(got[3])
        assert c["rays"] == 8 * len(far) and c["fallback"] >= 8 * len(far)
    near = np.flatnonzero(p.ok & ~p.far)[:64]
    got = ao.host_sim(host_sim, tmp_path, "c2_analytic", p.points[near], p.seeds[near], np.full(len(near), w.R, "<f4"), 8, threads=4)
    assert hs.counters(got[3])["fallback"] < 8 * len(near)


def test_radius_ladder(host_sim, oracle, load_scene, tmp_path):
    """ao_cases.radius_ladder on testscene, one sample per point: at a radius one float below the sample's own hit distance and at
    that distance the sample is open, one float above it is occluded -- by the bounded walk, with the LDS table, and with every
    sample re-cast exactly (SIM_FORCE_FALLBACK=0: there the closest hit is found at t itself and the comparison alone decides)"""
    flat = load_scene("testscene").flatten(1, 1)
    points, seeds, radii, want, left_out = ao.radius_ladder(oracle, oracle.OracleScene(flat), flat)
    print("radius ladder: %d of %d points left out (their sample hits nothing), %d rungs" % (left_out, ao.LADDER_POINTS, len(points)))
    assert 4 * left_out <= ao.LADDER_POINTS and 0 < len(points) <= 3 * ao.LADDER_POINTS
    for env in ({}, {"SIM_TABS": "1"}, {"SIM_FORCE_FALLBACK": "0"}):
        got = ao.host_sim(host_sim, tmp_path, "testscene", points, seeds, radii, 1, want_bent=False, want_states=False, env=env, threads=8)
        bad = np.flatnonzero(got[0] != want)
        assert len(bad) == 0, "%r: %d open counts differ, first at point %d rung %s: %d" % (env, len(bad), bad[0] // 3, ("prev(t)", "t", "next(t)")[bad[0] % 3], got[0][bad[0]])
        if "SIM_FORCE_FALLBACK" in env:
            assert hs.counters(got[3])["fallback"] >= len(points)


# ---- 4. under the sanitizers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["testscene", "c2_analytic"])
def test_host_sim_under_sanitizers(world, tmp_path, name):
    """tools/host_sim_san (the stand-alone ASan + UBSan binary, run directly) at spp 8: ends clean, with the same bits"""
    san = hs.built("host_sim_san")
    w = world(name)
    p = w.pts
    want = ao.expected(w, w.radii, 8)
    for env in TABS:
        got = ao.host_sim(san, tmp_path, name, p.points, p.seeds, w.radii, 8, env=env, threads=4)
        ao.assert_same(got[:3], want, "sanitized %s %r" % (name, env))
    got = ao.host_sim(san, tmp_path, name, p.points, p.seeds, None, 8, want_bent=False, want_states=False, threads=4)
    ao.assert_same(got[:3], ao.expected(w, None, 8), "sanitized %s, no radius, no optional output" % name)
