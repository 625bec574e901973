"""Feature renders that follow mirrors and glass (ort_render_follow, ort_render_views_follow and their device forms), host side:
the helper that turns the oracle into their reference (tests/follow_cases.py) pinned against the oracle's own PIXEL render of the
diffuse twin, the conditions the inputs are held to, the C ABI surface and its errors in the order include/ort.h gives them, the
launch plan, and the lane code run on host threads (tools/host_sim --follow), plain and as the stand-alone ASan + UBSan binary,
against that reference bit for bit; identities 1 and 2 against tools/host_sim --features."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import feature_cases as fc
import follow_cases as fw
import host_sim_tool as hs
from conftest import DATA, ROOT
from host_cases import aligned as _aligned, params as _params, scene as _scene

NAMES = {"ort_render_follow", "ort_render_follow_device", "ort_render_views_follow", "ort_render_views_follow_device"}


@pytest.fixture()
def world(api, oracle, load_scene, tmp_path_factory):
    return lambda name: fw.world(api, oracle, load_scene, tmp_path_factory, name)


@pytest.fixture(scope="module")
def host_sim():
    return hs.built("host_sim")


def _single(got):
    return {k: v[0] for k, v in got.items()}


# ---- 1. the helper against the oracle alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fw.SCENES)
def test_helper_is_the_twins_render(oracle, world, name):
    """the final states the numpy chain predicts are, on every pixel of the single frame and of the batch's three, the states
    the oracle's own PIXEL jobs return on the diffuse twin, at spp 1 and 5, rr 0.5 and 0.8: every draw of every followed sample
    is the render's.  No restated arithmetic on the twin's side"""
    w = world(name)
    tw = fw.twin(oracle, w.flat)
    for spp, rr in ((1, 0.5), (5, 0.5), (5, 0.8)):
        for c in fw.chains(w, spp, rr, 64):
            assert c.at_cap == 0
            want = fw.expected(c)["states"]
            got = fw.twin_states(tw, c.cam, c.w, c.h, c.seed, spp, rr)
            ne = got != want
            assert not ne.any(), "%s seed %d spp %d rr %g: %d states differ, first at %s" % (name, c.seed, spp, rr, ne.sum(), tuple(np.argwhere(ne)[0]))


def test_helper_rect_is_the_twins(oracle, world):
    w = world("glass_room")
    tw = fw.twin(oracle, w.flat)
    c = fw.chains(w, 5, 0.5, 64, fw.RECT)[0]
    got = fw.twin_states(tw, c.cam, c.w, c.h, c.seed, 5, 0.5, rect=fw.RECT)
    assert (got == fw.expected(c)["states"]).all()
    assert len(c.xs) == (fw.RECT[2] - fw.RECT[0]) * (fw.RECT[3] - fw.RECT[1])


# ---- 2. the conditions --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fw.SPECULAR_SCENES)
def test_conditions(world, name):
    """the scene's own camera, seed 2024, spp 5.  rr 0.5, cap 64: at least 10 % of the samples are followed, at least 50 roulette
    deaths, at least 50 refractions, some sample with b >= 2, at least 5 % of the pixels have 0 < hits < spp, no sample at the cap.
    rr 0.8, cap 2: at least 5 samples are recorded at the cap on a specular-only surface"""
    w = world(name)
    fw.check_conditions(fw.chains(w, 5, 0.5, 64)[0], fw.chains(w, 5, 0.8, 2)[0], name)
    for c in fw.chains(w, 5, 0.5, 64)[1:3]:   # the batch's two frames from the scene's own camera see the specular shapes on their own seeds
        assert c.followed >= 0.10 * c.samples


# ---- 3. the C ABI -----------------------------------------------------------------------------------------------------------
def test_entry_points_have_c_linkage(api):
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NAMES <= names
    assert NAMES <= set(api.EXPORTS)
    hdr = open(os.path.join(os.path.dirname(DATA), "include", "ort.h")).read()
    assert all(n + "(" in hdr for n in NAMES)
    assert api.lib().ort_abi_version() == 3   # additive: the ABI version stands
    assert ctypes.sizeof(api.FollowPlanes) == 56
    assert api.MAX_FOLLOW_BOUNCES == 64 and "#define ORT_MAX_FOLLOW_BOUNCES 64u" in hdr
    section = hdr[hdr.index("feature renders that follow mirrors and glass"):hdr.index("int ort_render_follow(")]
    for word in ("ray.cpp:1247-1426", "ray.cpp:1262 / :1411", "ray.cpp:1267", "ray.cpp:537-601", "ray.cpp:1100-1161", "ray.cpp:1345-1348", "ray.cpp:1428",
                 "job_seed(seed, y*W + x)", "wo = -normalize(d)", "b == max_bounces", "!(u < rr)", "0, ORT_NO_PRIM", "2.0f * 1e-4f", "not re-normalised",
                 "No pdf, BSDF value or path weight is evaluated", "A / (float)spp", "times spp / hits", "left untouched in every plane",
                 "Six identities", "diffuse twin", "in ort_render_views_features' order", "ORT_ERR_INVALID", "ORT_ERR_UNSUPPORTED", "ORT_ERR_STATE",
                 "ORT_ERR_NO_DEVICE", "camera rays plus bounce rays", "paths = 0", "At least one of the first six"):
        assert word in section, word
    order = [section.rindex(k) for k in ("ORT_ERR_INVALID (", "ORT_ERR_UNSUPPORTED (policy", "ORT_ERR_STATE (", "ORT_ERR_NO_DEVICE (")]
    assert order == sorted(order)
    order = [section.index(k) for k in ("spp above 1 << 24", "max_bounces above ORT_MAX_FOLLOW_BOUNCES", "a plane not 4-byte aligned")]
    assert order == sorted(order)


def _caller(api, views_form, device_form):
    """call(handle, params, planes[, views, count], cap) through one of the four entry points; planes: a FollowPlanes or None"""
    L = api.lib()
    cam = api.View()

    def call(handle, p, planes, views="own", count=1, stats=None, cap=8):
        fp = ctypes.byref(planes) if planes is not None else None
        pp = ctypes.byref(p) if p is not None else None
        if views_form:
            v = ctypes.addressof(cam) if isinstance(views, str) else views
            if device_form:
                return L.ort_render_views_follow_device(handle, pp, v, count, cap, fp, None, stats)
            return L.ort_render_views_follow(handle, pp, v, count, cap, fp, stats)
        if device_form:
            return L.ort_render_follow_device(handle, pp, cap, fp, None, stats)
        return L.ort_render_follow(handle, pp, cap, fp, stats)
    return call, cam


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("views_form", [False, True])
@pytest.mark.parametrize("committed", [True, False])
def test_errors_come_in_order(api, views_form, device_form, committed):
    """INVALID (the null planes struct, all of the first six planes null, null views, the view cap, the params -- rr among them --,
    then spp above 1 << 24, max_bounces above 64 and a misaligned plane), UNSUPPORTED (policy, shard, packed, a camera outside the
    box), then the scene's state: STATE before NO_DEVICE.  On a committed-but-not-uploaded scene and on an uncommitted one, so
    every error comes before any device work"""
    s = _scene(api, committed)
    L = api.lib()
    call, view = _caller(api, views_form, device_form)
    cam = s.camera(8, 8)
    for k, name in enumerate(("p", "x_axis", "y_axis", "z_axis")):
        setattr(view.camera, name, api.V3(*[float(c) for c in cam[k]]))
    fields = ("albedo", "normal", "depth", "hits", "ids", "bounces", "final_states")
    keep = [_aligned(8 * 8 * 12) for _ in fields]
    ptr = dict(zip(fields, (k[1] for k in keep)))
    full = api.FollowPlanes(**ptr)
    state = api.ERR_NO_DEVICE if committed else api.ERR_STATE
    bad_p = _params(api, width=0)
    # nulls first: before bad params and a bad cap
    assert call(s.handle, bad_p, None, cap=65) == api.ERR_INVALID
    assert b"planes" in L.ort_last_error()
    assert call(s.handle, bad_p, api.FollowPlanes(), cap=65) == api.ERR_INVALID
    assert b"no plane" in L.ort_last_error()
    assert call(s.handle, bad_p, api.FollowPlanes(final_states=ptr["final_states"])) == api.ERR_INVALID   # the states are not one of the six
    assert b"no plane" in L.ort_last_error()
    if views_form:
        assert call(s.handle, bad_p, full, views=None) == api.ERR_INVALID
        assert b"views" in L.ort_last_error()
        assert call(s.handle, bad_p, full, count=api.MAX_VIEWS + 1) == api.ERR_INVALID
        assert b"ORT_MAX_VIEWS" in L.ort_last_error()
    assert call(None, _params(api), full) == api.ERR_INVALID
    assert call(s.handle, None, full) == api.ERR_INVALID
    # the params, as the render call judges them (rr too: it is used here), before the cap and the planes' alignment
    odd = api.FollowPlanes(**{**ptr, "depth": ptr["depth"] + 2})
    for p, word in ((bad_p, b"image size"), (_params(api, rect=(4, 4, 4, 8)), b"rect"), (_params(api, rect=(0, 0, 9, 8)), b"rect"),
                    (_params(api, spp=0), b"spp"), (_params(api, rr=-3.0), b"rr"), (_params(api, rr=float("nan")), b"rr"),
                    (_params(api, policy=7), b"policy"), (_params(api, shard=(3, 2)), b"shard index")):
        assert call(s.handle, p, odd, cap=65) == api.ERR_INVALID, word
        assert word in L.ort_last_error(), (word, L.ort_last_error())
    assert call(s.handle, _params(api, width=70000, height=1), odd) == api.ERR_UNSUPPORTED   # as the render call: 16-bit coordinates
    # spp above 1 << 24, then the cap, then the alignment, before what the call does not do
    chunky = _params(api, policy="chunk", spp=(1 << 24) + 1, shard=(0, 2), packed=True)
    assert call(s.handle, chunky, odd, cap=65) == api.ERR_INVALID
    assert b"1 << 24" in L.ort_last_error()
    chunky.spp = 1 << 24
    for cap in (65, 0xFFFFFFFF):
        assert call(s.handle, chunky, odd, cap=cap) == api.ERR_INVALID
        assert b"max_bounces" in L.ort_last_error()
    for name in ptr:
        assert call(s.handle, chunky, api.FollowPlanes(**{**ptr, name: ptr[name] + (1 if name == "ids" else 2)}), cap=64) == api.ERR_INVALID, name
        assert b"4-byte aligned" in L.ort_last_error()
    # what the call does not do: any policy but PIXEL, shards, a packed plane
    for policy in ("tile32", "whole", "chunk"):
        assert call(s.handle, _params(api, policy=policy, shard=(0, 2) if policy == "chunk" else (0, 1)), full) == api.ERR_UNSUPPORTED
        assert b"PIXEL" in L.ort_last_error()
    assert call(s.handle, _params(api, shard=(1, 2), packed=True), full) == api.ERR_UNSUPPORTED
    assert b"shard" in L.ort_last_error()
    assert call(s.handle, _params(api, packed=True), full) == api.ERR_UNSUPPORTED
    assert b"packed" in L.ort_last_error()
    if views_form:   # a camera outside the box, naming the view
        two = (api.View * 2)(view, view)
        two[1].camera.p = api.V3(1e6, 0.0, 0.0)
        assert call(s.handle, _params(api), full, views=ctypes.addressof(two), count=2) == api.ERR_UNSUPPORTED
        assert b"view 1" in L.ort_last_error()
    # all of these come before the scene's state; good arguments reach it: one plane alone, the limits, chunk as it comes
    for planes in (api.FollowPlanes(hits=ptr["hits"]), api.FollowPlanes(bounces=ptr["bounces"])):
        assert call(s.handle, _params(api, spp=1, chunk=5, rr=0.0), planes, cap=0) == state
    assert call(s.handle, _params(api, spp=1 << 24, rr=float("inf")), full, cap=64) == state
    assert (b"commit" if not committed else b"upload") in L.ort_last_error()


@pytest.mark.parametrize("device_form", [False, True])
def test_empty_batch_is_ok(api, device_form):
    """view_count == 0: ORT_OK without a launch, whatever the other arguments"""
    call, _ = _caller(api, True, device_form)
    for s in (_scene(api), _scene(api, committed=False)):
        assert call(s.handle, None, None, views=None, count=0, cap=99) == api.OK
        assert call(s.handle, _params(api, width=0, policy="whole"), api.FollowPlanes(), count=0) == api.OK
    assert call(None, None, None, views=None, count=0) == api.OK
    st = api.Stats()
    st.rays = 7
    assert call(_scene(api).handle, None, None, views=None, count=0, stats=ctypes.byref(st)) == api.OK
    assert st.rays == 0


def test_python_shapes(api):
    s = _scene(api)
    with pytest.raises(api.OrtError) as e:
        s.render_follow(8, 6, 4, 3, want=("depth", "bounces", "states"))
    assert e.value.code == api.ERR_NO_DEVICE
    with pytest.raises(api.OrtError) as e:
        s.render_follow(8, 6, 4, 3, max_bounces=65)
    assert e.value.code == api.ERR_INVALID
    for bad in ((), ("depth", "depth"), ("colour",)):
        with pytest.raises(ValueError):
            s.render_follow(8, 6, 4, 3, want=bad)
    good = fw.guard_planes((6, 8), ("depth", "bounces"))
    for bad in ({"depth": good["depth"]}, {**good, "depth": good["depth"].astype("<f8")}, {**good, "bounces": np.zeros((6, 8, 1), "<u4")}):
        with pytest.raises(ValueError):
            s.render_follow(8, 6, 4, 3, want=("depth", "bounces"), out=bad)
    cams = np.stack([s.camera(8, 6)] * 2)
    with pytest.raises(ValueError):
        s.render_views_follow(cams, [1], 8, 6, 4)
    with pytest.raises(api.OrtError) as e:
        s.render_views_follow(cams, [1, 2], 8, 6, 4)
    assert e.value.code == api.ERR_NO_DEVICE
    planes, st = s.render_views_follow(np.zeros((0, 4, 3), "<f4"), [], 8, 6, 4, want=fw.PLANES)
    assert planes["albedo"].shape == (0, 6, 8, 3) and planes["ids"].shape == (0, 6, 8, 2) and planes["bounces"].shape == (0, 6, 8) and st["rays"] == 0
    assert all(planes[k].dtype == np.dtype(fw.DTYPES[k]) for k in fw.PLANES)
    p = s.params(8, 6, 4, 1, "pixel")
    with pytest.raises(ValueError):
        s.render_follow_device(p, colour=64)
    for call in (lambda: s.render_follow_device(p, 3, depth=64, bounces=128), lambda: s.render_views_follow_device(p, cams, [1, 2], hits=64)):
        with pytest.raises(api.OrtError) as e:
            call()
        assert e.value.code == api.ERR_NO_DEVICE


def test_over_hits(api):
    """the mean over the recorded samples: plane * spp / hits in float32, 0 where nothing was recorded"""
    plane = np.array([[[0.5, 1.0, 0.25], [0.0, 0.0, 0.0]]], "<f4")
    hits = np.array([[2, 0]], "<u4")
    got = api.over_hits(plane, hits, 4)
    assert got.dtype == np.dtype("<f4") and got.shape == plane.shape
    assert (got[0, 0] == np.array([1.0, 2.0, 0.5], "<f4")).all() and (got[0, 1] == 0).all()
    assert (api.over_hits(np.array([[0.75, 0.0]], "<f4"), hits, 4) == np.array([[1.5, 0.0]], "<f4")).all()


# ---- 4. the launch plan -----------------------------------------------------------------------------------------------------------
def test_launch_plan_prints_the_follow_plan():
    """plan_follow: plan_features' grid, thresholds and batches over the same job space; tabs asks for the lights' table too;
    follow_view is features_view with the roulette's rr"""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "launch_plan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    tool = os.path.join(ROOT, "tools", "launch_plan")

    def plan(query="follow", env=None, **kw):
        e = {k: v for k, v in os.environ.items() if not k.startswith("ORT_")}
        e.update(env or {})
        out = subprocess.check_output([tool, "query=" + query] + ["%s=%s" % kv for kv in kw.items()], env=e).decode().splitlines()
        return json.loads(out[0]), dict(l.split(" = ") for l in out[1:])
    hd = dict(width=1920, height=1080, x1=1920, y1=1080, materials=8)
    for counters in (0, 1):
        pl, _ = plan(counters=counters, **hd)
        ft, _ = plan("features", counters=counters, **hd)
        assert pl.pop("query") == "follow" and ft.pop("query") == "features"
        assert pl == ft and pl["tabs"] == 1 and pl["count"] == 240 * 135 * 64 and pl["job_batch"] == 64 and pl["counters"] == counters
    assert plan(**{**hd, "materials": 60})[0]["tabs"] == 0 and plan(**{**hd, "pro_boxes": 30})[0]["tabs"] == 0
    assert plan(**{**hd, "lights": 70})[0]["tabs"] == 0 and plan("features", **{**hd, "lights": 70})[0]["tabs"] == 1   # these lanes read the lights
    pl, _ = plan(env={"ORT_JOB_BATCH": "7", "ORT_BATCH_TAIL": "1"}, **hd)
    assert pl["job_batch"] == 7 and pl["batch_until"] == pl["count"] - pl["grid"] * 256
    small = {**hd, "width": 24, "height": 16, "x1": 21, "y1": 13}
    pl, fill = plan(views=3, x0=3, y0=2, fill=1, spp=5, rr=0.5, **small)
    _, ffill = plan("features", views=3, x0=3, y0=2, fill=1, spp=5, rr=0.5, **small)
    assert pl["view_jobs"] == 6 * 64 and pl["count"] == 3 * 6 * 64 and pl["grid"] == 5
    assert float(fill["rr"]) == 0.5 and float(ffill["rr"]) == 0.0
    assert {k: v for k, v in fill.items() if k != "rr"} == {k: v for k, v in ffill.items() if k != "rr"}
    assert subprocess.run([tool, "query=follow", "width=8", "height=8", "x1=9", "y1=8"], capture_output=True).returncode == 2


# ---- 5. the lane code on host threads ---------------------------------------------------------------------------------------
def _prims(host_sim, tmp_path, w, chains, env=None):
    rays = np.concatenate([c.last for c in chains])
    hits, _ = hs.raycast(host_sim, tmp_path, w.scn, rays, base=w.base, env=env or {})
    return hits


@pytest.mark.parametrize("name,envs", [("glass_room", [{}, {"SIM_TABS": "1"}]), ("c2_analytic", [{}, {"SIM_TABS": "1"}]), ("c3_bunny_room", [{}]),
                                       ("open", [{"SIM_TABS": "1"}]), ("tables_mats_over", [{}])])
def test_host_sim_is_the_reference(host_sim, world, tmp_path, name, envs):
    """all seven planes, all bits, the single frame and the batch of three, spp 1 and 5 at rr 0.5, cap 64, the tables in LDS form
    and from their arrays, one thread and eight; rays is the helper's count of camera and bounce rays; the shapes of the ids are
    tools/host_sim --raycast's for the helper's last rays, and at spp 1 so are depth's last leg, the normal and the material
    (identity 6)"""
    w = world(name)
    for k, env in enumerate(envs):
        for spp in fw.SPPS:
            one, batch, ch = fw.expected_set(w, spp, 0.5, 64)
            got, r = fw.host_sim(host_sim, tmp_path, w.scn, fw.W, fw.H, None, spp, 0.5, 64, seed=fw.SEED, base=w.base, env=env, threads=1 if k else 8)
            fw.assert_same(_single(got), one, "%s single spp %d %r" % (name, spp, env))
            assert hs.counters(r)["rays"] == ch[0].rays and hs.counters(r)["paths"] == 0
            gotb, r = fw.host_sim(host_sim, tmp_path, w.scn, fw.W, fw.H, None, spp, 0.5, 64, cams=w.fcams, seeds=w.fseeds, base=w.base, env=env, threads=8)
            fw.assert_same(gotb, batch, "%s batch spp %d %r" % (name, spp, env))
            assert hs.counters(r)["rays"] == sum(c.rays for c in ch[1:])
            if not k:
                hits = _prims(host_sim, tmp_path, w, ch, env)
                ids = np.concatenate([got["ids"], gotb["ids"]])
                fw.assert_prims(ids, ch, hits["prim"], "%s spp %d" % (name, spp))
                if spp == 1:
                    rec = np.concatenate([got["hits"].reshape(-1), gotb["hits"].reshape(-1)]) == 1
                    normal = np.concatenate([got["normal"].reshape(-1, 3), gotb["normal"].reshape(-1, 3)])
                    assert rec.any() and (ids.reshape(-1, 2)[rec, 0] == hits["mat"][rec]).all()
                    assert (normal[rec].view("<u4") == hits["n"][rec].view("<u4")).all() and (normal[~rec] == 0).all()


def test_host_sim_cap_and_no_roulette(host_sim, world, tmp_path):
    """cap 2 at rr 0.8: capped samples record the specular surface with its zero albedo; rr 0: no bounce, specular-only pixels
    have hits == 0 and their sums are +0"""
    w = world("glass_room")
    one, batch, ch = fw.expected_set(w, 5, 0.8, 2)
    assert ch[0].capped_specular >= 5
    got, _ = fw.host_sim(host_sim, tmp_path, w.scn, fw.W, fw.H, None, 5, 0.8, 2, seed=fw.SEED, base=w.base, threads=8)
    fw.assert_same(_single(got), one, "cap 2")
    gotb, _ = fw.host_sim(host_sim, tmp_path, w.scn, fw.W, fw.H, None, 5, 0.8, 2, cams=w.fcams, seeds=w.fseeds, base=w.base, threads=8)
    fw.assert_same(gotb, batch, "cap 2, batch")
    one, _, ch = fw.expected_set(w, 5, 0.0, 64)
    got, r = fw.host_sim(host_sim, tmp_path, w.scn, fw.W, fw.H, None, 5, 0.0, 64, seed=fw.SEED, base=w.base, threads=8)
    fw.assert_same(_single(got), one, "rr 0")
    assert hs.counters(r)["rays"] == fw.W * fw.H * 5 and (got["bounces"] == 0).all()
    first = fc.expected(fc.frames(w)[0], 5)
    spec = fw.specular_only(w.flat)[fc.frames(w)[0].mat].all(axis=1).reshape(fw.H, fw.W)   # every sample lands on a specular-only surface
    assert spec.sum() >= 5 and (got["hits"][0][spec] == 0).all()
    for k in ("albedo", "normal", "depth"):
        assert (got[k][0][spec].view("<u4") == 0).all(), k
    assert (first["hits"][spec] == 5).all()   # the first-hit render counts them all


@pytest.mark.parametrize("name", ["glass_room", "open"])
def test_identity_1_cap_0_is_the_first_hit_render(host_sim, world, tmp_path, name):
    """max_bounces == 0: ort_render_features' six planes for any rr, bit for bit; bounces all zero"""
    w = world(name)
    want, _ = fc.host_sim(host_sim, tmp_path, w.scn, fw.W, fw.H, fw.RECT, 5, cams=w.fcams, seeds=w.fseeds, base=w.base, threads=8)
    for rr in (0.0, 0.8, 7.0):
        got, _ = fw.host_sim(host_sim, tmp_path, w.scn, fw.W, fw.H, fw.RECT, 5, rr, 0, cams=w.fcams, seeds=w.fseeds, base=w.base, threads=8)
        for k in fc.PLANES:
            assert (got[k].view("<u4") == want[k].view("<u4")).all(), (rr, k)
        inside = got["bounces"] != fw.GUARDS["bounces"]
        assert inside.sum() == 3 * (fw.RECT[2] - fw.RECT[0]) * (fw.RECT[3] - fw.RECT[1]) and (got["bounces"][inside] == 0).all()


def test_identity_2_all_diffuse_scene(host_sim, world, tmp_path):
    """a scene whose non-light materials all have a diffuse part gives ort_render_features' planes for every cap and rr"""
    w = world("c3_bunny_room")
    assert not fw.specular_only(w.flat).any()
    want, _ = fc.host_sim(host_sim, tmp_path, w.scn, fw.W, fw.H, None, 5, seed=fw.SEED, base=w.base, threads=8)
    for rr, cap in ((0.5, 64), (0.8, 3), (4.0, 64)):
        got, _ = fw.host_sim(host_sim, tmp_path, w.scn, fw.W, fw.H, None, 5, rr, cap, seed=fw.SEED, base=w.base, threads=8)
        for k in fc.PLANES:
            assert (got[k].view("<u4") == want[k].view("<u4")).all(), (rr, cap, k)
        assert (got["bounces"] == 0).all()


def test_host_sim_rect_planes_alone_and_forced_walk(host_sim, world, tmp_path):
    """the rect (3, 2, 21, 13) cuts blocks on all four sides: its pixels are the reference's in every plane, those outside keep
    their guard words; each plane asked for alone has the bits it has with all seven; the exact walk forced on the rays whose
    direction's low bits are zero changes no bit"""
    w = world("glass_room")
    _, batch, _ = fw.expected_set(w, 5, 0.5, 64, fw.RECT, fw.GUARDS)
    inside = np.zeros((fw.H, fw.W), bool)
    inside[fw.RECT[1]:fw.RECT[3], fw.RECT[0]:fw.RECT[2]] = True
    args = (w.scn, fw.W, fw.H, fw.RECT, 5, 0.5, 64)
    got, _ = fw.host_sim(host_sim, tmp_path, *args, cams=w.fcams, seeds=w.fseeds, base=w.base, threads=8)
    fw.assert_same(got, batch, "rect, batch")
    for k in fw.PLANES:
        assert (got[k][:, ~inside].view("<u4") == np.asarray(fw.GUARDS[k], fw.DTYPES[k]).view("<u4")).all(), k
    for k in fw.PLANES[:6]:
        alone, _ = fw.host_sim(host_sim, tmp_path, *args, cams=w.fcams, seeds=w.fseeds, want=(k,), base=w.base, threads=8)
        assert set(alone) == {k} and (alone[k].view("<u4") == got[k].view("<u4")).all(), k
    forced, r = fw.host_sim(host_sim, tmp_path, *args, cams=w.fcams, seeds=w.fseeds, base=w.base, threads=8, env={"SIM_FORCE_FALLBACK": "0xf"})
    assert hs.counters(r)["fallback"] > 0
    for k in fw.PLANES:
        assert (forced[k].view("<u4") == got[k].view("<u4")).all(), k


# ---- 6. under the sanitizers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fw.SPECULAR_SCENES)
def test_host_sim_under_sanitizers(world, tmp_path, name):
    """tools/host_sim_san (the stand-alone ASan + UBSan binary, run directly): the single frame and the batch at spp 5, the cap
    reached, a rect that cuts blocks, planes left out: ends clean, with the reference's planes"""
    san = hs.built("host_sim_san")
    w = world(name)
    one, batch, _ = fw.expected_set(w, 5, 0.5, 64)
    for env in ({}, {"SIM_TABS": "1"}):
        got, _ = fw.host_sim(san, tmp_path, w.scn, fw.W, fw.H, None, 5, 0.5, 64, seed=fw.SEED, base=w.base, env=env, threads=2)
        fw.assert_same(_single(got), one, "sanitized %s %r" % (name, env))
    got, _ = fw.host_sim(san, tmp_path, w.scn, fw.W, fw.H, None, 5, 0.5, 64, cams=w.fcams, seeds=w.fseeds, want=("normal", "ids", "bounces", "states"), base=w.base, threads=2)
    fw.assert_same(got, batch, "sanitized %s batch" % name)
    _, capped, _ = fw.expected_set(w, 5, 0.8, 2, fw.RECT, fw.GUARDS)
    got, _ = fw.host_sim(san, tmp_path, w.scn, fw.W, fw.H, fw.RECT, 5, 0.8, 2, cams=w.fcams, seeds=w.fseeds, base=w.base, threads=2)
    fw.assert_same(got, capped, "sanitized %s rect, cap 2" % name)
