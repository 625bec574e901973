"""A batch of camera views in one launch (ort_render_views / ort_render_views_device), host side: the C ABI surface, the pose
helper against the oracle's, the argument and state errors in the order include/ort.h gives them -- all reported before any
device work, so they are the same on a machine without a GPU --, the workspace rule, the launch plan of a batch through
tools/launch_plan, and the shapes Scene.render_views accepts."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
import table_scenes
from conftest import DATA, GOLDEN, assert_bits_equal
from host_cases import scene as _scene
from test_launch_plan import KNOBS

NAMES = {"ort_camera_from_pose", "ort_render_views", "ort_render_views_device", "ort_render_views_workspace_bytes"}
FORCE_ALL = {"ORT_EXCHANGE": "1", "ORT_WAVES5": "1", "ORT_WIDE": "1"}


def test_views_entry_points_have_c_linkage(api):
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NAMES <= names
    assert NAMES <= set(api.EXPORTS)
    hdr = open(os.path.join(os.path.dirname(DATA), "include", "ort.h")).read()
    assert "ort_view;" in hdr   # the fifth symbol is the struct
    assert ctypes.sizeof(api.View) == 52
    assert api.lib().ort_abi_version() == 3   # additive: the ABI version stands


# ---- the pose helper ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", [(1920, 1080), (64, 64), (37, 23)])
def test_camera_from_pose_is_the_oracles(api, width, height):
    rng = np.random.default_rng(width * 1000 + height)
    for _ in range(200):
        p = (rng.standard_normal(3) * 10).astype("<f4")
        q = rng.standard_normal(4).astype("<f4")
        if rng.random() < 0.7:
            q = (q / np.linalg.norm(q)).astype("<f4")   # the reference does not normalise: both kinds
        ratio = np.float32(rng.uniform(0.05, 1.5))
        assert_bits_equal(api.camera_from_pose(p, q, ratio, width, height), oracle_lib.camera(p, q, ratio, width, height),
                          "pose %s %s %s" % (p, q, ratio))


@pytest.mark.parametrize("name", ["c2_analytic", "c3_bunny_room", "testscene"])
def test_camera_from_pose_of_the_scenes_own_pose(api, load_scene, name):
    s = load_scene(name)
    si = s.info()
    p = [si.camera_p.x, si.camera_p.y, si.camera_p.z]
    for w, h in [(1920, 1080), (20, 13), (64, 64)]:
        assert_bits_equal(api.camera_from_pose(p, list(si.camera_quat_xyzw), si.camera_height_ratio, w, h), s.camera(w, h), name)


def test_camera_from_pose_argument_errors(api):
    L = api.lib()
    p = np.zeros(3, "<f4")
    q = np.array([0, 0, 0, 1], "<f4")
    cam = api.Camera()
    ok = (p.ctypes.data, q.ctypes.data, 0.2, 8, 8, ctypes.byref(cam))
    assert L.ort_camera_from_pose(*ok) == api.OK
    for i, bad in ((0, None), (1, None), (5, None), (3, 0), (3, -4), (4, 0), (4, -1)):
        args = list(ok)
        args[i] = bad
        assert L.ort_camera_from_pose(*args) == api.ERR_INVALID, (i, bad)
    for bad_p, bad_q in ((np.zeros(2), q), (p, np.zeros(3)), (np.zeros((1, 3)), q)):
        with pytest.raises(ValueError):
            api.camera_from_pose(bad_p, bad_q, 0.2, 8, 8)


# ---- errors, in order --------------------------------------------------------------------------------------------------
def _caller(api, device_form):
    L = api.lib()

    def call(handle, params, views, count, out, stats=None):
        p = ctypes.byref(params) if params is not None else None
        v = views.ctypes.data if views is not None else None
        if device_form:
            return L.ort_render_views_device(handle, p, v, count, out, None, stats)
        return L.ort_render_views(handle, p, v, count, out, stats)
    return call


def _origin_box(flat):
    """the box of every shape and the scene's own camera_p (what the tree was built for), from Scene.flatten's arrays"""
    pts = [flat.camera[0][None, :]]
    r = np.abs(flat.spheres["r"])[:, None]
    pts += [flat.spheres["center"] - r, flat.spheres["center"] + r, flat.boxes["min"], flat.boxes["max"]]
    r = np.abs(flat.cylinders["r"])[:, None]
    for end in (flat.cylinders["base"], flat.cylinders["base"] + flat.cylinders["axis"]):
        pts += [end - r, end + r]
    pts += [np.asarray(m["vertices"], "<f4").reshape(-1, 3) for m in flat.meshes]
    pts = np.concatenate([np.asarray(q, "<f4").reshape(-1, 3) for q in pts])
    return pts.min(axis=0), pts.max(axis=0)


def _good_views(api, s, w, h, n=3):
    views = np.zeros(n, api.VIEW_DTYPE)
    views["camera"] = s.camera(w, h)
    views["seed"] = np.arange(1, n + 1)
    return views


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("committed", [True, False])
def test_views_errors_come_in_order(api, device_form, committed):
    """INVALID (nulls, bad params, the view cap), then UNSUPPORTED (policy, shard, packed, camera outside the box or not finite),
    then the scene's state: STATE on an uncommitted scene, NO_DEVICE on a committed one that is not uploaded"""
    s = _scene(api, committed)
    L = api.lib()
    call = _caller(api, device_form)
    w, h = 20, 13
    state = api.ERR_NO_DEVICE if committed else api.ERR_STATE
    views = _good_views(api, s, w, h)
    buf = np.full((3, h, w, 3), 7.0, "<f4")
    out = buf.ctypes.data
    good = api.Scene.params(w, h, 4, 0, "chunk", chunk=2)
    assert call(s.handle, good, views, 3, out) == state
    assert (b"commit" if not committed else b"upload") in L.ort_last_error()
    # 1. INVALID
    assert call(None, good, views, 3, out) == api.ERR_INVALID
    assert call(s.handle, None, views, 3, out) == api.ERR_INVALID
    assert call(s.handle, good, None, 3, out) == api.ERR_INVALID
    assert call(s.handle, good, views, 3, None) == api.ERR_INVALID
    for kw in (dict(width=0, height=h, spp=1), dict(width=w, height=h, spp=0), dict(width=w, height=h, spp=6, chunk=4),
               dict(width=w, height=h, spp=1, rect=(5, 5, 5, 9)), dict(width=w, height=h, spp=1, rect=(0, 0, w + 1, h)),
               dict(width=w, height=h, spp=1, rr=float("nan"))):
        assert call(s.handle, api.Scene.params(seed=0, **kw), views, 3, out) == api.ERR_INVALID, kw
    many = np.zeros(api.MAX_VIEWS + 1, api.VIEW_DTYPE)
    many["camera"] = views["camera"][0]
    assert api.MAX_VIEWS >= 1024
    assert call(s.handle, good, many, api.MAX_VIEWS + 1, out) == api.ERR_INVALID
    assert b"views" in L.ort_last_error()
    # ... before UNSUPPORTED: a bad rect with an unsupported policy is the rect's error
    assert call(s.handle, api.Scene.params(w, h, 1, 0, "tile32", rect=(5, 5, 5, 9)), views, 3, out) == api.ERR_INVALID
    # 2. UNSUPPORTED
    for policy in ("tile32", "whole"):
        assert call(s.handle, api.Scene.params(w, h, 2, 0, policy), views, 3, out) == api.ERR_UNSUPPORTED, policy
    assert call(s.handle, api.Scene.params(w, h, 4, 0, "chunk", chunk=2, shard=(0, 2)), views, 3, out) == api.ERR_UNSUPPORTED
    assert call(s.handle, api.Scene.params(w, h, 4, 0, "pixel", shard=(1, 2)), views, 3, out) == api.ERR_UNSUPPORTED
    assert call(s.handle, api.Scene.params(w, h, 4, 0, "chunk", chunk=2, packed=True), views, 3, out) == api.ERR_UNSUPPORTED
    lo, hi = _origin_box(s.flatten(w, h))
    for axis in range(3):
        for far in (hi[axis] + 10.0, lo[axis] - 10.0):
            bad = views.copy()
            bad["camera"][1][0][axis] = far
            assert call(s.handle, good, bad, 3, out) == api.ERR_UNSUPPORTED
            assert b"view 1" in L.ort_last_error()
    for row in range(4):
        for value in (np.nan, np.inf, -np.inf):
            bad = views.copy()
            bad["camera"][2][row][1] = value
            assert call(s.handle, good, bad, 3, out) == api.ERR_UNSUPPORTED, (row, value)
            assert b"view 2" in L.ort_last_error()
    bad = views.copy()
    bad["camera"][0][0][0] = np.nan
    bad["camera"][1][0][0] = np.nan
    assert call(s.handle, good, bad, 3, out) == api.ERR_UNSUPPORTED and b"view 0" in L.ort_last_error()   # the first offender
    # nothing was written anywhere
    assert (buf == 7.0).all()


@pytest.mark.parametrize("device_form", [False, True])
def test_views_empty_batch_is_ok(api, device_form):
    """view_count == 0: ORT_OK without a launch, whatever the other arguments"""
    call = _caller(api, device_form)
    good = api.Scene.params(8, 8, 1, 0, "pixel")
    for s in (_scene(api), _scene(api, committed=False)):
        assert call(s.handle, None, None, 0, None) == api.OK
        assert call(s.handle, good, None, 0, None) == api.OK
        assert call(s.handle, api.Scene.params(8, 8, 0, 0, "tile32", shard=(3, 2)), None, 0, None) == api.OK
    assert call(None, None, None, 0, None) == api.OK
    st = api.Stats()
    st.rays = 7
    assert call(_scene(api).handle, good, None, 0, None, ctypes.byref(st)) == api.OK
    assert st.rays == 0


def test_views_aperture_box_rule(api):
    """the aperture's bounding box, p - 0.1 z +- 0.1 |x| +- 0.1 |y| per component, against the scene's box grown by 0.25"""
    s = _scene(api)
    L = api.lib()
    w, h = 16, 16
    lo, hi = _origin_box(s.flatten(w, h))
    good = api.Scene.params(w, h, 1, 0, "pixel")
    out = np.zeros((1, h, w, 3), "<f4")
    view = np.zeros(1, api.VIEW_DTYPE)
    cam = np.zeros((4, 3), "<f4")
    cam[1] = (0.5, 0, 0)   # x axis: aperture reaches +-0.05 in x
    cam[2] = (0, 0.2, 0)   # y axis: +-0.02 in y
    cam[3] = (0, 0, 1)     # z axis: centre 0.1 below p in z
    for axis, reach in ((0, 0.05), (1, 0.02), (2, -0.1)):
        for delta, want in ((-0.01, api.ERR_NO_DEVICE), (0.01, api.ERR_UNSUPPORTED)):
            cam[0] = (hi - 1.0)
            cam[0][axis] = hi[axis] + 0.25 - reach + delta
            view["camera"][0] = cam
            assert L.ort_render_views(s.handle, ctypes.byref(good), view.ctypes.data, 1, out.ctypes.data, None) == want, (axis, delta)


# ---- workspace -----------------------------------------------------------------------------------------------------------
def test_views_workspace_is_per_view(api):
    for spp, chunk in ((64, 16), (4, 2), (3, 1)):
        p = api.Scene.params(93, 61, spp, 0, "chunk", chunk=chunk)
        one = api.workspace_bytes(p)
        assert one == (spp // chunk) * 12 * 8 * 64 * 12
        for v in (0, 1, 5, 1024):
            assert api.views_workspace_bytes(p, v) == v * one
    assert api.views_workspace_bytes(api.Scene.params(93, 61, 8, 0, "pixel"), 7) == 0
    n = ctypes.c_uint64(0)
    assert api.lib().ort_render_views_workspace_bytes(None, 3, ctypes.byref(n)) == api.ERR_INVALID
    assert api.lib().ort_render_views_workspace_bytes(ctypes.byref(api.Scene.params(8, 8, 1, 0)), 3, None) == api.ERR_INVALID


# ---- the plan of a batch ---------------------------------------------------------------------------------------------------
def _plan(env=None, defaults=True, **kw):
    args = dict(cu_count=256, diffuse_only=1, fast_tree_bytes=6 << 20, sah_cost=0.05) if defaults else {}
    args.update(kw)
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(env or {})
    r = subprocess.run([table_scenes.launch_plan_tool()] + ["%s=%s" % kv for kv in args.items()], env=e, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return r.stdout


SHAPES = [dict(width=128, height=128, spp=64, chunk=16), dict(width=20, height=13, spp=3, chunk=1, x0=3, y0=2, x1=17, y1=9),
          dict(width=1920, height=1080, spp=1024, chunk=64), dict(width=256, height=256, spp=8, policy="pixel")]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("traits", [dict(), dict(diffuse_only=0), dict(sah_cost=0.2), dict(fast_tree_bytes=86 << 20, diffuse_only=0, has_wide=1),
                                    dict(materials=60), dict(counters=1)])
def test_views_plan(shape, traits):
    """V = 5: five times the jobs and the partial planes, the view's job count stated; always the plain loop at four waves --
    no exchange, no five-waves unit, no wide tree, no wavefront mode -- with diffuse and tabs as the single view has them,
    whatever the knobs say; batch and refill rules applied to the enlarged job count"""
    kw = dict(tab_flags=11)
    kw.update(shape)
    kw.update(traits)
    if "materials" in kw:
        del kw["tab_flags"]
    one = json.loads(_plan(env={"ORT_EXCHANGE": "0", "ORT_WAVES5": "0"}, **kw))
    for env in ({}, FORCE_ALL, dict(FORCE_ALL, ORT_MODE="wavefront", ORT_DEBUG_UTIL="1")):
        p = json.loads(_plan(env=env, views=5, **kw))
        assert (p["views"], p["view_count"], p["view_jobs"]) == (1, 5, one["job_count"])
        assert p["job_count"] == 5 * one["job_count"] and p["partial_bytes"] == 5 * one["partial_bytes"]
        assert (p["exchange"], p["five"], p["wide"], p["wavefront"], p["util"]) == (0, 0, 0, 0, 0)
        assert (p["diffuse"], p["tabs"], p["counters"]) == (one["diffuse"], one["tabs"], one["counters"])
        assert p["implicit"] == (1 if p["tabs"] and not p["counters"] else 0)
        assert (p["mode"], p["nchunks"], p["my_blocks"], p["block_major"]) == (one["mode"], one["nchunks"], one["my_blocks"], one["block_major"])
        assert (p["stash_bytes"], p["capL"], p["endgame_from"]) == (0, 0, 0)
        lanes = p["grid"] * 256
        assert p["grid"] == min(1024, (p["job_count"] + 255) // 256)
        assert p["job_batch"] == (128 if p["job_count"] >= 96 * lanes else 64)
        assert p["batch_until"] == max(0, p["job_count"] - 8 * ((p["job_batch"] + 63) // 64) * lanes)
        assert (p["refill_below"], p["descend_below"]) == (one["refill_below"], one["descend_below"])
    # views=1 is the render call as it was, knobs and all
    for env in ({}, FORCE_ALL):
        a, b = json.loads(_plan(env=env, views=1, **kw)), json.loads(_plan(env=env, **kw))
        assert (a.pop("views"), a.pop("view_count"), a.pop("view_jobs")) == (0, 1, b["job_count"])
        assert a == b


def test_plan_without_views_is_what_it_was():
    """without the views argument the tool prints what it printed before it knew of views, byte for byte: the SHA-256 of the
    line the parent revision printed for every configuration tests/test_launch_plan.py asks about (arguments and knobs as that
    module passed them)"""
    cases = json.load(open(os.path.join(GOLDEN, "launch_plan_before_views.json")))
    assert len(cases) >= 500
    for c in cases:
        line = _plan(env=c["env"], defaults=False, **c["args"])
        assert hashlib.sha256(line.encode()).hexdigest() == c["sha256"], (c["args"], c["env"], line)


# ---- Python shapes -----------------------------------------------------------------------------------------------------------
def test_python_render_views_shapes(api):
    s = _scene(api)
    raw = _scene(api, committed=False)
    cam = s.camera(8, 8)
    cams = np.stack([cam, cam])
    for bad_c, bad_s in ((cam, [1]), (cams[:, :3], [1, 2]), (cams.reshape(2, 12), [1, 2]), (cams, [1]), (cams, [1, 2, 3]), (cams, 5),
                         (cams, [[1, 2]]), (np.zeros((api.MAX_VIEWS + 1, 4, 3), "<f4"), np.zeros(api.MAX_VIEWS + 1, "<u4"))):
        for scene in (s, raw):   # a bad shape is rejected before the library is called: a ValueError whatever the scene's state
            with pytest.raises(ValueError):
                scene.render_views(bad_c, bad_s, 8, 8, 1)
            with pytest.raises(ValueError):
                scene.render_views_device(64, api.Scene.params(8, 8, 1, 0), bad_c, bad_s)
    with pytest.raises(ValueError):
        s.render_views(cams, [1, 2], 8, 8, 1, out=np.zeros((2, 8, 9, 3), "<f4"))
    with pytest.raises(ValueError):
        s.render_views(cams, [1, 2], 8, 8, 1, out=np.zeros((2, 8, 8, 3), "<f8"))
    # good shapes reach the library, which has no device to run on
    for seeds in ([1, 2], np.array([1, 0xFFFFFFFF], "<u4"), (3, 4)):
        with pytest.raises(api.OrtError) as e:
            s.render_views(cams, seeds, 8, 8, 2, policy="pixel")
        assert e.value.code == api.ERR_NO_DEVICE
        with pytest.raises(api.OrtError) as e:
            s.render_views_device(64, api.Scene.params(8, 8, 2, 0, "chunk", chunk=1), cams, seeds)
        assert e.value.code == api.ERR_NO_DEVICE
    with pytest.raises(api.OrtError) as e:
        raw.render_views(cams, [1, 2], 8, 8, 2)
    assert e.value.code == api.ERR_STATE
    frames, st = s.render_views(np.zeros((0, 4, 3), "<f4"), np.zeros(0, "<u4"), 8, 8, 1)
    assert frames.shape == (0, 8, 8, 3) and st["paths"] == 0
