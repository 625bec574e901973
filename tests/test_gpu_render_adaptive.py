"""The adaptive camera render on the device (ort_render_adaptive, ort_render_views_adaptive and their device forms; kernels
pt_adaptive): colours, sample counts, second moments and final stream states, bit for bit what the stopping rule of include/ort.h
gives on the oracle's own camera samples (tests/render_adaptive_cases.py).  Frames are at most 27 x 19, max_spp at most 64."""
import numpy as np
import pytest

import render_adaptive_cases as rac
import table_scenes
import views_cases
from adaptive_cases import Adaptive
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

SCENES = ["testscene", "c2_analytic", "glass_room", "c3_bunny_room", "tables_mats_over"]
RRS = (0.8, 0.0)
W, H, SEED = rac.W, rac.H, rac.SEED
_worlds = {}


class World:
    pass


@pytest.fixture()
def world(api, oracle, gpu_scene, tmp_path_factory):
    """name -> the uploaded scene and the oracle's chains of 64 samples per pixel of the 24 x 16 frame at seed 2024 ({rr:
    chain}, each computed once, when first asked for)"""
    def get(name):
        if name not in _worlds:
            w = World()
            if name.startswith("tables_"):
                scene, _, csg = table_scenes.build(api, name[len("tables_"):], tmp_path_factory.mktemp(name))
                w.scene = scene.commit().upload(0)
            else:
                w.scene, csg = gpu_scene(name), True
            w.csg = csg
            w.osc = oracle.OracleScene(w.scene.flatten(W, H), with_reference_csg=csg)
            w.chain = {}

            def want(ad, rr=rac.RR, w=w):
                if rr not in w.chain:
                    w.osc.set_camera(w.scene.camera(W, H))
                    w.chain[rr] = rac.chains(w.osc, W, H, SEED, rr)
                return rac.expected_from(w.chain[rr], W, H, ad)
            w.want = want
            _worlds[name] = w
        return _worlds[name]
    return get


def run(scene, ad, rr=rac.RR, w=W, h=H, seed=SEED, **kw):
    """the host form -> (rgb, spp, m2, states), stats"""
    rgb, spp, m2, fin, st = scene.render_adaptive(w, h, ad.min_spp, ad.max_spp, ad.tolerance, ad.floor, ad.check_every, seed=seed, rr=rr,
                                                  want_states=True, **kw)
    return (rgb, spp, m2, fin), st


def torch_planes(shape, fills=(-7.0, 0x5A5A5A5A, -7.0, 0x5A5A5A5A), pad=0):
    """four device tensors (flat, `pad` guard words at both ends) for planes of `shape` pixels"""
    import torch
    dev = torch.device("cuda", 0)
    n = int(np.prod(shape))
    return [torch.full((k * n + 2 * pad,), f, dtype=t, device=dev)
            for k, f, t in zip((3, 1, 1, 1), fills, (torch.float32, torch.int32, torch.float32, torch.int32))]


def torch_run(scene, ad, rr=rac.RR, skip=(), counters=False, want_stats=False, rect=None, w=W, h=H, seed=SEED, views=None):
    """the device form, with torch tensors on a non-default stream; without stats the call does not wait: synchronise.
    skip: which of "spp", "m2", "states" to pass as NULL -> (rgb, spp, m2, states) with the fillers where nothing was asked for"""
    import torch
    shape = (h, w) if views is None else (len(views[0]), h, w)
    t = torch_planes(shape)
    ptr = [x.data_ptr() for x in t]
    for k, name in enumerate(("spp", "m2", "states")):
        if name in skip:
            ptr[k + 1] = 0
    p = scene.params(w, h, 0, seed, "pixel", 0, rect, rr, counters)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        if views is None:
            st = scene.render_adaptive_device(p, ad.min_spp, ad.max_spp, ad.tolerance, ad.floor, ad.check_every, *ptr, stream=stream.cuda_stream,
                                              want_stats=want_stats)
        else:
            st = scene.render_views_adaptive_device(p, views[0], views[1], ad.min_spp, ad.max_spp, ad.tolerance, ad.floor, ad.check_every, *ptr,
                                                    stream=stream.cuda_stream, want_stats=want_stats)
    stream.synchronize()
    h_ = [x.cpu().numpy() for x in t]
    return (h_[0].reshape(shape + (3,)), h_[1].view("<u4").reshape(shape), h_[2].reshape(shape), h_[3].view("<u4").reshape(shape)), st


# ---- 1. against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rr", RRS)
@pytest.mark.parametrize("ad", rac.SETS, ids=["frame", "every", "fixed"])
@pytest.mark.parametrize("name", SCENES)
def test_frame_is_the_rule_on_the_oracles_samples(world, name, ad, rr):
    w = world(name)
    want = w.want(ad, rr)
    got, st = run(w.scene, ad, rr)
    rac.assert_same(got, want, "%s %r rr %g, host form" % (name, ad, rr))
    assert st["kernel_ms"] > 0 and st["paths"] == 0   # counters only on request


# ---- 2. the two identities, against the PIXEL render in the same process -----------------------------------------------------------
@pytest.mark.parametrize("name", ["c2_analytic", "glass_room", "c3_bunny_room"])
def test_identities_against_the_pixel_render(world, name):
    w = world(name)
    for n in (2, 7):
        img, _ = w.scene.render(W, H, n, SEED, "pixel", rr=rac.RR)
        got, _ = run(w.scene, Adaptive(n, n, 1, 0.3, 0.05))
        assert_bits_equal(got[0], img, "%s min = max = %d" % (name, n))
        assert (got[1] == n).all()
    img, _ = w.scene.render(W, H, 8, SEED, "pixel", rr=rac.RR)
    got, _ = run(w.scene, rac.HUGE)
    assert np.isfinite(got[2]).all()
    assert_bits_equal(got[0], img, name + " huge tolerance")
    assert (got[1] == 8).all()
    rac.assert_same(got, w.want(rac.HUGE), name + " huge tolerance against the rule")


# ---- 3. frame, rect, guard words ----------------------------------------------------------------------------------------------------
_rect_ref = {}


def rect_reference(oracle, scene, w, h, rect, seed):
    key = (w, h, rect, seed)
    if key not in _rect_ref:
        osc = oracle.OracleScene(scene.flatten(w, h))
        _rect_ref[key] = rac.chains(osc, w, h, seed, rac.RR, rect)
    return _rect_ref[key]


@pytest.mark.parametrize("w,h,rect", [(27, 19, (5, 9, 26, 17)), (1, 1, None), (9, 1, None)])
def test_frame_rect_and_guard_words(api, oracle, gpu_scene, w, h, rect):
    """a rect that cuts 8 x 8 blocks inside a 27 x 19 frame, a 1 x 1 and a 9 x 1 frame: guard words before and after every plane
    and the pixels outside the rect keep what they held, host form and device form"""
    scene = gpu_scene("c2_analytic")
    G = 8
    fills = (np.float32(-3.5), 0xC3C3C3C3, np.float32(-3.5), 0xC3C3C3C3)
    want = rac.expected_from(rect_reference(oracle, scene, w, h, rect, 77), w, h, rac.FRAME, fills)
    L = api.lib()
    ad = api.Adaptive(*rac.FRAME)
    p = scene.params(w, h, 0, 77, "pixel", 0, rect, rac.RR)
    n = w * h

    def check(planes, what):
        inner = [x[k * G: x.size - k * G] for x, k in zip(planes, (1, 1, 1, 1))]
        got = (inner[0].reshape(h, w, 3), inner[1].view("<u4").reshape(h, w), inner[2].reshape(h, w), inner[3].view("<u4").reshape(h, w))
        rac.assert_same(got, want, what)
        for x, fill in zip(planes, fills):
            x = x.view("<u4") if x.dtype.kind in "iu" else x
            assert (x[:G] == fill).all() and (x[-G:] == fill).all(), what + ": a guard word was written"
    planes = [np.full(k * n + 2 * G, f, dt) for k, f, dt in zip((3, 1, 1, 1), fills, ("<f4", "<u4", "<f4", "<u4"))]
    assert L.ort_render_adaptive(scene.handle, api.C.byref(p), api.C.byref(ad), *[x.ctypes.data + 4 * G for x in planes], None) == api.OK
    check(planes, "host form %d x %d %r" % (w, h, rect))
    # the device form: the same guards at both ends of each tensor
    t = torch_planes((h, w), (-3.5, 0xC3C3C3C3 - (1 << 32), -3.5, 0xC3C3C3C3 - (1 << 32)), pad=G)
    st = scene.render_adaptive_device(p, *rac.FRAME[:2], rac.FRAME.tolerance, rac.FRAME.floor, rac.FRAME.check_every,
                                      *[x.data_ptr() + 4 * G for x in t], want_stats=True)
    assert st["kernel_ms"] > 0
    check([x.cpu().numpy() for x in t], "device form %d x %d %r" % (w, h, rect))


# ---- 4. NULL outputs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip", ["spp", "m2", "states"])
def test_null_optional_outputs(api, world, skip):
    """each optional plane passed as NULL in turn, both forms: the others are the rule's, and nothing is written for it"""
    w = world("c2_analytic")
    want = w.want(rac.FRAME)
    got, st = torch_run(w.scene, rac.FRAME, skip=(skip,))
    assert st is None
    k = {"spp": 1, "m2": 2, "states": 3}[skip]
    filler = np.float32(-7.0) if skip == "m2" else 0x5A5A5A5A
    assert (got[k] == filler).all()
    rac.assert_same(tuple(None if i == k else g for i, g in enumerate(got)), want, "device form without " + skip)
    out, spp, m2, fin = np.zeros((H, W, 3), "<f4"), np.zeros((H, W), "<u4"), np.zeros((H, W), "<f4"), np.zeros((H, W), "<u4")
    ptr = {"spp": spp.ctypes.data, "m2": m2.ctypes.data, "states": fin.ctypes.data}
    ptr[skip] = None
    p = w.scene.params(W, H, 0, SEED, "pixel", 0, None, rac.RR)
    assert api.lib().ort_render_adaptive(w.scene.handle, api.C.byref(p), api.C.byref(api.Adaptive(*rac.FRAME)), out.ctypes.data, ptr["spp"],
                                         ptr["m2"], ptr["states"], None) == api.OK
    got = (out, spp, m2, fin)
    assert not got[k].any()
    rac.assert_same(tuple(None if i == k else g for i, g in enumerate(got)), want, "host form without " + skip)


# ---- 5. the device form; counters -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["testscene", "c3_bunny_room"])
def test_device_form_on_a_stream_and_counters(world, name):
    w = world(name)
    for ad, rr in ((rac.FRAME, 0.8), (rac.EVERY, 0.0)):
        want = w.want(ad, rr)
        got, st = torch_run(w.scene, ad, rr)          # stats == NULL: enqueued, then synchronised
        assert st is None
        rac.assert_same(got, want, "%s device form %r rr %g" % (name, ad, rr))
    got, st = torch_run(w.scene, rac.FRAME, counters=True, want_stats=True)
    rac.assert_same(got, w.want(rac.FRAME), name + " device form with counters")
    assert st["paths"] == int(got[1].sum()) and st["paths"] > 8 * W * H
    assert st["rays"] >= st["paths"] and st["node_tests"] > 0 and st["kernel_ms"] > 0
    _, st_host = run(w.scene, rac.FRAME, counters=True)
    assert {k: st_host[k] for k in ("paths", "rays", "node_tests", "tri_tests", "analytic_tests")} == \
           {k: st[k] for k in ("paths", "rays", "node_tests", "tri_tests", "analytic_tests")}


# ---- 6. every kernel of the family ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c3_bunny_room", "glass_room"])
def test_every_kernel_of_the_family(world, monkeypatch, name):
    """pt_adaptive<counters, diffuse, tabs>: the bunny room is diffuse only, ORT_KERNEL=general takes its all-lobes flavour (the
    glass room's own), ORT_LDS_TABLES=0 the tables in HBM.  One answer."""
    w = world(name)
    want = w.want(rac.FRAME)
    for env in ({}, {"ORT_LDS_TABLES": "0"}, {"ORT_KERNEL": "general"}, {"ORT_KERNEL": "general", "ORT_LDS_TABLES": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for counters in (False, True):
            got, st = run(w.scene, rac.FRAME, counters=counters)
            rac.assert_same(got, want, "%s %s counters=%s" % (name, env, counters))
            assert st["paths"] == (int(want[1].sum()) if counters else 0)
        for k in env:
            monkeypatch.delenv(k)


# ---- 7. knobs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c2_analytic", "c3_bunny_room", "tables_mats_over"])
def test_independent_of_batches_and_walk(world, monkeypatch, name):
    w = world(name)
    want = w.want(rac.FRAME)
    for batch in ("0", "7", "128"):
        monkeypatch.setenv("ORT_JOB_BATCH", batch)
        got, _ = run(w.scene, rac.FRAME)
        rac.assert_same(got, want, name + " ORT_JOB_BATCH=" + batch)
    monkeypatch.delenv("ORT_JOB_BATCH")
    _, st_fast = run(w.scene, rac.FRAME, counters=True)
    monkeypatch.setenv("ORT_DEBUG_FORCE_FALLBACK", "0")
    got, st = run(w.scene, rac.FRAME, counters=True)
    monkeypatch.delenv("ORT_DEBUG_FORCE_FALLBACK")
    rac.assert_same(got, want, name + " every ray re-cast exactly")
    assert st["fallback_rays"] == st["rays"] == st_fast["rays"] > st_fast["fallback_rays"]
    assert st["paths"] == st_fast["paths"] == int(want[1].sum())


# ---- 8. views --------------------------------------------------------------------------------------------------------------------------
VW, VH = 16, 12
_views_ref = {}


def views_reference(api, oracle, scene, name):
    """three poses (tests/views_cases.py) with three seeds at 16 x 12: (cameras, the reference's planes per view), once"""
    if name not in _views_ref:
        flat = scene.flatten(VW, VH)
        cams = np.stack([api.camera_from_pose(p, q, r, VW, VH) for p, q, r in views_cases.poses(scene, flat)])
        osc = oracle.OracleScene(flat)
        want = []
        for cam, seed in zip(cams, views_cases.SEEDS):
            osc.set_camera(cam)
            want.append(rac.expected_from(rac.chains(osc, VW, VH, seed, rac.RR), VW, VH, rac.FRAME))
        _views_ref[name] = (cams, tuple(np.stack([v[k] for v in want]) for k in range(4)))
    return _views_ref[name]


def run_views(scene, cams, seeds, ad=rac.FRAME, **kw):
    out = scene.render_views_adaptive(cams, seeds, VW, VH, ad.min_spp, ad.max_spp, ad.tolerance, ad.floor, ad.check_every, rr=rac.RR,
                                      want_states=True, **kw)
    return out[:4], out[4]


@pytest.mark.parametrize("name", ["c2_analytic", "c3_bunny_room"])
def test_views_are_the_reference_from_each_pose(api, oracle, gpu_scene, name):
    scene = gpu_scene(name)
    cams, want = views_reference(api, oracle, scene, name)
    seeds = views_cases.SEEDS
    got, st = run_views(scene, cams, seeds, counters=True)
    rac.assert_same(got, want, name + " three views")
    assert st["paths"] == int(want[1].sum())
    assert len({int(want[1][v].sum()) for v in range(3)}) == 3   # three different frames
    # the batch is its views one call each, in any order
    for order in ([2, 0, 1], [1], [0, 0]):
        part, _ = run_views(scene, cams[order], [seeds[v] for v in order])
        rac.assert_same(part, tuple(x[order] for x in want), "%s views %r" % (name, order))
    # the device form
    dev, st = torch_run(scene, rac.FRAME, w=VW, h=VH, views=(cams, seeds))
    assert st is None
    rac.assert_same(dev, want, name + " three views, device form")


def test_one_view_batch_of_the_scenes_camera_is_the_frame_call(gpu_scene):
    scene = gpu_scene("glass_room")
    own = scene.camera(VW, VH)
    for seed in (2024, 99):
        one, _ = run_views(scene, own[None], [seed])
        frame, _ = run(scene, rac.FRAME, w=VW, h=VH, seed=seed)
        rac.assert_same(tuple(x[0] for x in one), frame, "own camera, seed %d" % seed)
        assert len(set(frame[1].ravel())) > 2
    # a rect applies to every view; pixels outside it keep what the planes held
    rect = (3, 2, 13, 9)
    planes = [np.full((2, VH, VW, 3), -2.0, "<f4"), np.full((2, VH, VW), 7, "<u4"), np.full((2, VH, VW), -2.0, "<f4"), np.full((2, VH, VW), 7, "<u4")]
    scene.render_views_adaptive(np.stack([own, own]), [2024, 99], VW, VH, *rac.FRAME[:2], rac.FRAME.tolerance, rac.FRAME.floor, rac.FRAME.check_every,
                                rect=rect, rr=rac.RR, want_states=True, out=planes)
    inside = np.zeros((VH, VW), bool)
    inside[rect[1]:rect[3], rect[0]:rect[2]] = True
    for v, seed in enumerate((2024, 99)):
        frame, _ = run(scene, rac.FRAME, w=VW, h=VH, seed=seed)
        for k in range(4):
            assert planes[k][v][inside].tobytes() == frame[k][inside].tobytes(), (v, k)
            assert (planes[k][v][~inside] == (7 if k in (1, 3) else -2.0)).all(), (v, k)


def test_a_camera_outside_the_box_is_refused(api, gpu_scene):
    scene = gpu_scene("c2_analytic")
    cams = np.stack([scene.camera(VW, VH)] * 3)
    cams[2, 0] += np.float32(1e4)
    with pytest.raises(api.OrtError) as e:
        run_views(scene, cams, [1, 2, 3])
    assert e.value.code == api.ERR_UNSUPPORTED and "view 2" in str(e.value)
