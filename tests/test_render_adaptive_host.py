"""The adaptive camera render (ort_render_adaptive, ort_render_views_adaptive and their device forms), host side: the helper that
turns the oracle into their reference (tests/render_adaptive_cases.py) pinned against the oracle's own PIXEL render, the frame
set shown not to be vacuous, the C ABI surface and its errors in the order include/ort.h gives them, the launch plan, and the lane
code with the stopping rule run on host threads (tools/host_sim --render-adaptive), plain and under ASan + UBSan, against that
reference bit for bit."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import host_sim_tool as hs
import render_adaptive_cases as rac
import table_scenes
from adaptive_cases import Adaptive
from conftest import DATA, ROOT
from host_cases import adaptive_params as _params, aligned as _aligned, scene as _scene

NAMES = {"ort_render_adaptive", "ort_render_adaptive_device", "ort_render_views_adaptive", "ort_render_views_adaptive_device"}
_worlds = {}


class World:
    pass


@pytest.fixture()
def world(api, oracle, load_scene, tmp_path_factory):
    """name -> scene, oracle scene with the scene's own camera at 24 x 16, and the oracle's chains of 64 samples per pixel at
    seed 2024, rr 0.8; computed once"""
    def get(name):
        if name not in _worlds:
            w = World()
            if name.startswith("tables_"):
                d = tmp_path_factory.mktemp("ra_" + name)
                scene, _, csg = table_scenes.build(api, name[len("tables_"):], d)
                w.scene, w.scn, w.base = scene.commit(), str(d / (name[len("tables_"):] + ".scn")), str(d) + "/"
            else:
                w.scene, w.scn, w.base, csg = load_scene(name), name, None, True
            w.osc = oracle.OracleScene(w.scene.flatten(rac.W, rac.H), with_reference_csg=csg)
            w.chain = rac.chains(w.osc, rac.W, rac.H, rac.SEED, rac.RR)
            _worlds[name] = w
        return _worlds[name]
    return get


@pytest.fixture(scope="module")
def host_sim():
    return hs.built("host_sim")


# ---- 1. the helper against the oracle alone ---------------------------------------------------------------------------------
def test_helper_without_checks_is_the_pixel_render(world):
    """min == max == n: no check runs, and the expectation is the oracle's PIXEL render at spp = n, every pixel taking n samples"""
    w = world("c2_analytic")
    for n in (2, 8, 17):
        rgb, spp, m2, fin = rac.expected_from(w.chain, rac.W, rac.H, Adaptive(n, n, 3, 0.3, 0.05))
        want, _ = w.osc.render(rac.W, rac.H, n, rac.SEED, "pixel", rr=rac.RR)
        rac.assert_same((rgb, None, None, None), (want, None, None, None), "min = max = %d" % n)
        assert (spp == n).all() and (m2 >= 0).all() and ((m2 > 0) == (rgb != 0).any(axis=2)).all()
        assert (fin == np.array([[w.chain[(x, y)][1][n - 1] for x in range(rac.W)] for y in range(rac.H)])).all()


# ---- 2. the frame set is not vacuous ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["testscene", "c2_analytic", "c3_bunny_room"])
def test_frame_set_is_not_vacuous(world, name):
    """from the oracle alone, the scene's own camera at 24 x 16, seed 2024, rr 0.8, under FRAME: each of the three classes
    (stopped at min_spp, strictly between, ran to max_spp) holds at least 5 % of the pixels; at least 10 % of the early-stopped
    pixels are not black"""
    w = world(name)
    assert tuple(rac.FRAME) == (8, 64, 8, 0.3, 0.05) and (rac.W, rac.H, rac.SEED, rac.RR) == (24, 16, 2024, 0.8)
    rgb, spp, m2, fin = rac.expected_from(w.chain, rac.W, rac.H, rac.FRAME)
    at_min, between, at_max, lit = rac.classes(spp, rgb, rac.FRAME)
    print("%s: at min %.3f, between %.3f, at max %.3f; early and lit %.3f" % (name, at_min, between, at_max, lit))
    assert at_min >= 0.05 and between >= 0.05 and at_max >= 0.05 and lit >= 0.10


# ---- 3. the C ABI -----------------------------------------------------------------------------------------------------------
def test_entry_points_have_c_linkage(api):
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NAMES <= names
    assert NAMES <= set(api.EXPORTS)
    hdr = open(os.path.join(os.path.dirname(DATA), "include", "ort.h")).read()
    assert all(n + "(" in hdr for n in NAMES)
    assert api.lib().ort_abi_version() == 3   # additive: the ABI version stands
    # the header states the order of the errors, and the semantics operation by operation
    section = hdr[hdr.index("the adaptive camera render"):hdr.index("int ort_render_adaptive(")]
    for word in ("in ort_render_views' order with the ad checks directly after the params checks", "ORT_ERR_INVALID", "ORT_ERR_UNSUPPORTED",
                 "ORT_ERR_STATE", "ORT_ERR_NO_DEVICE", "ray.cpp:1232", "job_seed(seed, y*W + x)", "(n - min_spp) % check_every == 0",
                 "C / (float)n", "left untouched in every plane", "Two identities"):
        assert word in section, word
    order = [section.rindex(k) for k in ("ORT_ERR_INVALID (", "ORT_ERR_UNSUPPORTED (policy", "ORT_ERR_STATE (", "ORT_ERR_NO_DEVICE (")]
    assert order == sorted(order)


GOOD = tuple(rac.FRAME)   # any valid set: the errors do not depend on it


def _caller(api, views_form, device_form):
    """call(handle, params, ad, out, spp, m2, states[, views, count]) through one of the four entry points"""
    L = api.lib()
    cam = api.View()

    def call(handle, p, ad, out, spp, m2, states, views="own", count=1, stats=None):
        adp = ctypes.byref(api.Adaptive(*ad)) if ad is not None else None
        pp = ctypes.byref(p) if p is not None else None
        if views_form:
            v = ctypes.addressof(cam) if isinstance(views, str) else views
            if device_form:
                return L.ort_render_views_adaptive_device(handle, pp, adp, v, count, out, spp, m2, states, None, stats)
            return L.ort_render_views_adaptive(handle, pp, adp, v, count, out, spp, m2, states, stats)
        if device_form:
            return L.ort_render_adaptive_device(handle, pp, adp, out, spp, m2, states, None, stats)
        return L.ort_render_adaptive(handle, pp, adp, out, spp, m2, states, stats)
    return call, cam


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("views_form", [False, True])
@pytest.mark.parametrize("committed", [True, False])
def test_errors_come_in_order(api, views_form, device_form, committed):
    """INVALID (nulls, the view cap, the params with max_spp for spp, then the stopping rule's parameters), UNSUPPORTED (policy,
    shard, packed, a camera outside the box), then the scene's state: STATE before NO_DEVICE.  On a committed-but-not-uploaded
    scene and on an uncommitted one, so every error comes before any device work"""
    s = _scene(api, committed)
    L = api.lib()
    call, view = _caller(api, views_form, device_form)
    cam = s.camera(8, 8)
    for k, name in enumerate(("p", "x_axis", "y_axis", "z_axis")):
        setattr(view.camera, name, api.V3(*[float(c) for c in cam[k]]))
    keep = [_aligned(8 * 8 * 12), _aligned(256), _aligned(256), _aligned(256)]
    out, spp, m2, fin = (k[1] for k in keep)
    state = api.ERR_NO_DEVICE if committed else api.ERR_STATE
    nan, inf = float("nan"), float("inf")
    bad_ad = (1, 64, 4, 0.3, 0.05)
    # nulls first: before bad params and a bad ad
    assert call(s.handle, _params(api, width=0), bad_ad, None, spp, m2, fin) == api.ERR_INVALID
    assert b"framebuffer" in L.ort_last_error()
    if views_form:
        assert call(s.handle, _params(api, width=0), bad_ad, out, spp, m2, fin, views=None) == api.ERR_INVALID
        assert b"views" in L.ort_last_error()
        assert call(s.handle, _params(api, width=0), bad_ad, out, spp, m2, fin, count=api.MAX_VIEWS + 1) == api.ERR_INVALID
        assert b"ORT_MAX_VIEWS" in L.ort_last_error()
    assert call(None, _params(api), GOOD, out, spp, m2, fin) == api.ERR_INVALID
    assert call(s.handle, None, GOOD, out, spp, m2, fin) == api.ERR_INVALID
    # the params, as the render call judges them, before ad; spp and chunk are ignored
    for p, word in ((_params(api, width=0), b"image size"), (_params(api, rect=(4, 4, 4, 8)), b"rect"), (_params(api, rect=(0, 0, 9, 8)), b"rect"),
                    (_params(api, rr=-0.5), b"rr"), (_params(api, rr=nan), b"rr"), (_params(api, policy=7), b"policy"),
                    (_params(api, shard=(3, 2)), b"shard index")):
        assert call(s.handle, p, bad_ad, out, spp, m2, fin) == api.ERR_INVALID, word
        assert word in L.ort_last_error(), (word, L.ort_last_error())
    assert call(s.handle, _params(api, width=70000, height=1), bad_ad, out, spp, m2, fin) == api.ERR_UNSUPPORTED   # as the render call: 16-bit coordinates
    # ad, as ort_radiance_adaptive judges it, before what the call does not do
    chunky = _params(api, policy="chunk", spp=7, chunk=3, shard=(0, 2), packed=True)
    assert call(s.handle, chunky, None, out, spp, m2, fin) == api.ERR_INVALID
    assert b"null ad" in L.ort_last_error()
    for bad, word in ((bad_ad, b"min_spp"), ((0, 0, 4, 0.3, 0.05), b"min_spp"), ((8, 7, 4, 0.3, 0.05), b"max_spp"),
                      ((4, (1 << 24) + 1, 4, 0.3, 0.05), b"1 << 24"), ((4, 64, 0, 0.3, 0.05), b"check_every"),
                      ((4, 64, 4, nan, 0.05), b"tolerance"), ((4, 64, 4, inf, 0.05), b"tolerance"), ((4, 64, 4, -0.5, 0.05), b"tolerance"),
                      ((4, 64, 4, 0.3, nan), b"floor"), ((4, 64, 4, 0.3, inf), b"floor"), ((4, 64, 4, 0.3, -1.0), b"floor")):
        assert call(s.handle, chunky, bad, out, spp, m2, fin) == api.ERR_INVALID, bad
        assert word in L.ort_last_error(), (bad, L.ort_last_error())
    # what the call does not do: any policy but PIXEL, shards, a packed framebuffer
    for policy in ("tile32", "whole", "chunk"):
        assert call(s.handle, _params(api, policy=policy, shard=(0, 2) if policy == "chunk" else (0, 1)), GOOD, out, spp, m2, fin) == api.ERR_UNSUPPORTED
        assert b"PIXEL" in L.ort_last_error()
    assert call(s.handle, _params(api, shard=(1, 2), packed=True), GOOD, out, spp, m2, fin) == api.ERR_UNSUPPORTED
    assert b"shard" in L.ort_last_error()
    assert call(s.handle, _params(api, packed=True), GOOD, out, spp, m2, fin) == api.ERR_UNSUPPORTED
    assert b"packed" in L.ort_last_error()
    if views_form:   # a camera outside the box, naming the view
        two = (api.View * 2)(view, view)
        two[1].camera.p = api.V3(1e6, 0.0, 0.0)
        assert call(s.handle, _params(api), GOOD, out, spp, m2, fin, views=ctypes.addressof(two), count=2) == api.ERR_UNSUPPORTED
        assert b"view 1" in L.ort_last_error()
    # all of these come before the scene's state; good arguments reach it, the optional planes NULL and the limits included
    assert call(s.handle, _params(api, spp=0, chunk=5), (2, 2, 1, 0.0, 0.0), out, None, None, None) == state
    assert call(s.handle, _params(api, rr=7.5), (2, 1 << 24, 0xFFFFFFFF, 1e30, 3e38), out, spp, m2, fin) == state
    assert (b"commit" if not committed else b"upload") in L.ort_last_error()


@pytest.mark.parametrize("device_form", [False, True])
def test_empty_batch_is_ok(api, device_form):
    """view_count == 0: ORT_OK without a launch, whatever the other arguments"""
    call, _ = _caller(api, True, device_form)
    for s in (_scene(api), _scene(api, committed=False)):
        assert call(s.handle, None, None, None, None, None, None, views=None, count=0) == api.OK
        assert call(s.handle, _params(api, width=0, policy="whole"), (0, 0, 0, -1.0, -1.0), None, None, None, None, count=0) == api.OK
    assert call(None, None, GOOD, None, None, None, None, views=None, count=0) == api.OK
    st = api.Stats()
    st.rays = 7
    assert call(_scene(api).handle, None, GOOD, None, None, None, None, views=None, count=0, stats=ctypes.byref(st)) == api.OK
    assert st.rays == 0


def test_python_shapes(api):
    s = _scene(api)
    with pytest.raises(api.OrtError) as e:
        s.render_adaptive(8, 6, 8, 64, 0.3, seed=3, want_states=True)
    assert e.value.code == api.ERR_NO_DEVICE
    with pytest.raises(api.OrtError) as e:
        s.render_adaptive(8, 6, 1, 64, 0.3)
    assert e.value.code == api.ERR_INVALID
    for bad in ((-1, 64), (4, 1 << 32)):
        with pytest.raises(ValueError):
            s.render_adaptive(8, 6, bad[0], bad[1], 0.3)
    planes = [np.zeros((6, 8, 3), "<f4"), np.zeros((6, 8), "<u4"), np.zeros((6, 8), "<f4")]
    for bad in (planes[:2], [planes[0], planes[1].astype("<i8"), planes[2]], [planes[0][:, ::2], planes[1], planes[2]],
                [np.zeros((8, 6, 3), "<f4"), planes[1], planes[2]], planes + [np.zeros((6, 8), "<u4")]):
        with pytest.raises(ValueError):
            s.render_adaptive(8, 6, 8, 64, 0.3, out=bad)
    with pytest.raises(ValueError):
        s.render_adaptive(8, 6, 8, 64, 0.3, want_states=True, out=planes)
    cams = np.stack([s.camera(8, 6)] * 2)
    for bad_cams, bad_seeds in ((cams[:, :3], [1, 2]), (cams, [1]), (cams[0], [1, 2])):
        with pytest.raises(ValueError):
            s.render_views_adaptive(bad_cams, bad_seeds, 8, 6, 8, 64, 0.3)
    with pytest.raises(ValueError):
        s.render_views_adaptive(cams, [1, 2], 8, 6, 8, 64, 0.3, out=planes)   # one frame's planes for two views
    with pytest.raises(api.OrtError) as e:
        s.render_views_adaptive(cams, [1, 2], 8, 6, 8, 64, 0.3)
    assert e.value.code == api.ERR_NO_DEVICE
    rgb, spp, m2, states, st = s.render_views_adaptive(np.zeros((0, 4, 3), "<f4"), [], 8, 6, 8, 64, 0.3, want_states=True)
    assert rgb.shape == (0, 6, 8, 3) and spp.shape == m2.shape == states.shape == (0, 6, 8) and st["paths"] == 0
    assert spp.dtype == states.dtype == np.dtype("<u4") and rgb.dtype == m2.dtype == np.dtype("<f4")
    p = s.params(8, 6, 1, 1, "pixel")
    for call in (lambda: s.render_adaptive_device(p, 8, 64, 0.3, 0.05, 4, 64), lambda: s.render_views_adaptive_device(p, cams, [1, 2], 8, 64, 0.3, 0.05, 4, 64)):
        with pytest.raises(api.OrtError) as e:
            call()
        assert e.value.code == api.ERR_NO_DEVICE


# ---- 4. the launch plan -----------------------------------------------------------------------------------------------------------
def test_launch_plan_prints_the_adaptive_plan():
    """plan_pixel_jobs, RK_ADAPTIVE: always the plain loop over implicit one-pixel jobs of a batch of views, both BSDF flavours with
    counters, the job space the blocks under the rect times the views; no exchange, no five waves, no wide tree, no wavefront,
    whatever the knobs say"""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "launch_plan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    tool = os.path.join(ROOT, "tools", "launch_plan")

    def plan(env=None, **kw):
        e = {k: v for k, v in os.environ.items() if not k.startswith("ORT_")}
        e.update(env or {})
        return json.loads(subprocess.check_output([tool] + ["%s=%s" % kv for kv in kw.items()], env=e))
    base = dict(adaptive=1, policy="pixel", width=1920, height=1080, x1=1920, y1=1080, materials=8, lights=2, diffuse_only=1, sah_cost=0.5)
    forced = {"ORT_EXCHANGE": "1", "ORT_WAVES5": "1", "ORT_WIDE": "1", "ORT_MODE": "wavefront", "ORT_DEBUG_UTIL": "1"}
    for env in ({}, forced):
        for counters in (0, 1):
            pl = plan(env, counters=counters, has_wide=1, **base)
            assert pl["adaptive"] == 1 and pl["views"] == 1 and pl["view_count"] == 1 and pl["implicit"] == 1 and pl["mode"] == 1
            assert not (pl["exchange"] or pl["five"] or pl["wide"] or pl["wavefront"] or pl["util"])
            assert pl["counters"] == counters and pl["diffuse"] == 1 and pl["tabs"] == 1
            assert pl["job_count"] == pl["view_jobs"] == 240 * 135 * 64 and pl["grid"] == pl["max_blocks"] == 1024
            assert pl["partial_bytes"] == pl["stash_bytes"] == pl["drain_bytes"] == 0
    pl = plan({"ORT_KERNEL": "general", "ORT_LDS_TABLES": "0"}, views=3, x0=5, y0=9, **{**base, "x1": 20, "y1": 17, "width": 27, "height": 19})
    assert pl["diffuse"] == 0 and pl["tabs"] == 0 and pl["view_count"] == 3
    assert pl["view_jobs"] == 3 * 2 * 64 and pl["job_count"] == 3 * pl["view_jobs"] and pl["grid"] == 5   # blocks x 0..2, y 1..2
    assert plan(**{**base, "materials": 60})["tabs"] == 0
    assert subprocess.run([tool, "adaptive=1", "policy=chunk", "width=8", "height=8", "x1=8", "y1=8"], capture_output=True).returncode == 2


# ---- 5. the lane code on host threads ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,envs", [("c2_analytic", [{}, {"SIM_TABS": "1"}]),
                                       ("c3_bunny_room", [{"SIM_DIFFUSE": "1"}, {"SIM_TABS": "1", "SIM_DIFFUSE": "1"}, {}]),
                                       ("tables_mats_over", [{}])])
def test_host_sim_is_the_reference(host_sim, world, tmp_path, name, envs):
    """all four planes, all bits: both BSDF flavours, the tables in LDS form and from their arrays; one thread and eight; a
    check_every so large that the next check's count passes 2^32"""
    w = world(name)
    once = Adaptive(8, 64, 0xFFFFFFFC, 0.3, 0.05)
    want = {ad: rac.expected_from(w.chain, rac.W, rac.H, ad) for ad in rac.SETS + (once,)}
    assert ((want[once][1] == 8) | (want[once][1] == 64)).all() and (want[once][1] == 64).any() and (want[once][1] == 8).any()
    for k, env in enumerate(envs):
        for ad, threads in ((rac.FRAME, 8), (rac.EVERY, 1), (rac.FIXED, 8), (once, 8)):
            if k and ad is not rac.FRAME:
                continue
            got = rac.host_sim(host_sim, tmp_path, w.scn, rac.W, rac.H, None, rac.SEED, ad, rac.RR, w.base, env=env, threads=threads)
            rac.assert_same(got, want[ad], "%s %r %r, %d threads" % (name, ad, env, threads))
    r = hs.run(host_sim, rac.host_sim_args(str(tmp_path), w.scn, rac.W, rac.H, None, rac.SEED, rac.FRAME, rac.RR, w.base)[0])
    assert hs.counters(r)["paths"] == int(want[rac.FRAME][1].sum())   # the counters' paths: the samples taken


def test_host_sim_rect_inside_a_frame(host_sim, oracle, load_scene, tmp_path):
    """a rect that cuts 8 x 8 blocks inside a 27 x 19 frame (partial blocks at the frame's edges too): the rect's pixels are the
    reference's in all four planes, the pixels outside it keep their guard values; 1 thread and 8"""
    w, h, rect = 27, 19, (5, 9, 26, 17)
    scene = load_scene("c2_analytic")
    osc = oracle.OracleScene(scene.flatten(w, h))
    want = rac.expected_from(rac.chains(osc, w, h, 77, rac.RR, rect), w, h, rac.FRAME, rac.GUARDS)
    inside = np.zeros((h, w), bool)
    inside[rect[1]:rect[3], rect[0]:rect[2]] = True
    assert (want[1][~inside] == rac.GUARDS[1]).all() and (want[1][inside] <= 64).all() and len(set(want[1][inside])) > 2
    for threads in (1, 8):
        got = rac.host_sim(host_sim, tmp_path, "c2_analytic", w, h, rect, 77, rac.FRAME, rac.RR, threads=threads)
        rac.assert_same(got, want, "rect %r of %d x %d, %d threads" % (rect, w, h, threads))


# ---- 6. under the sanitizers --------------------------------------------------------------------------------------------------
def test_host_sim_under_sanitizers(oracle, load_scene, tmp_path):
    """tools/host_sim_san (the stand-alone ASan + UBSan binary, run directly) on one 16 x 12 frame: ends clean, with the
    reference's planes"""
    san = hs.built("host_sim_san")
    w, h = 16, 12
    osc = oracle.OracleScene(load_scene("c2_analytic").flatten(w, h))
    want = rac.expected_from(rac.chains(osc, w, h, 5, rac.RR), w, h, rac.FRAME)
    for env in ({}, {"SIM_TABS": "1"}):
        got = rac.host_sim(san, tmp_path, "c2_analytic", w, h, None, 5, rac.FRAME, rac.RR, env=env, threads=2)
        rac.assert_same(got, want, "sanitized %r" % env)
