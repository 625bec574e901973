"""First-hit feature renders (ort_render_features, ort_render_views_features and their device forms), host side: the helper that
turns the oracle into their reference (tests/feature_cases.py) pinned against the oracle's own PIXEL render of the emissive twin,
the input set shown to earn its keep, the C ABI surface and its errors in the order include/ort.h gives them, the launch plan, and
the lane code run on host threads (tools/host_sim --features), plain and under ASan + UBSan, against that reference bit for bit."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import feature_cases as fc
import host_sim_tool as hs
from conftest import DATA, ROOT
from host_cases import aligned as _aligned, params as _params, scene as _scene

NAMES = {"ort_render_features", "ort_render_features_device", "ort_render_views_features", "ort_render_views_features_device"}
SCENES = ["c2_analytic", "c3_bunny_room", "open"]


@pytest.fixture()
def world(api, oracle, load_scene, tmp_path_factory):
    return lambda name: fc.world(api, oracle, load_scene, tmp_path_factory, name)


@pytest.fixture(scope="module")
def host_sim():
    return hs.built("host_sim")


# ---- 1. the helper against the oracle alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_helper_is_the_twins_render(oracle, world, name):
    """the albedo and the final states the numpy restatement of the camera sample predicts are, on every pixel of the single
    frame and of the three posed views, the oracle's own PIXEL render of the emissive twin and the states its jobs return; the
    white twin's render is hits / spp.  No restated arithmetic on the twin's side"""
    w = world(name)
    tw, white = fc.twin(oracle, w.flat), fc.twin(oracle, w.flat, white=True)
    for f in fc.frames(w):
        for spp in fc.SPPS:
            want = fc.expected(f, spp)
            img, states = fc.twin_planes(tw, f.cam, f.w, f.h, f.seed, spp)
            fc.assert_same({"albedo": img, "states": states}, want, "%s seed %d spp %d: helper vs twin" % (name, f.seed, spp))
            cov, _ = fc.twin_planes(white, f.cam, f.w, f.h, f.seed, spp, with_states=False)
            ratio = (want["hits"].astype("<f4") / np.float32(spp)).astype("<f4")
            assert (cov.view("<u4") == np.repeat(ratio[..., None], 3, axis=2).view("<u4")).all()


def test_helper_rect_is_the_twins(oracle, world):
    w = world("open")
    tw = fc.twin(oracle, w.flat)
    f = fc.frames(w, fc.RECT)[2]
    want = fc.expected(f, 5)
    img, states = fc.twin_planes(tw, f.cam, f.w, f.h, f.seed, 5, rect=fc.RECT)
    fc.assert_same({"albedo": img, "states": states}, want, "rect: helper vs twin")
    inside = np.zeros((fc.H, fc.W), bool)
    inside[fc.RECT[1]:fc.RECT[3], fc.RECT[0]:fc.RECT[2]] = True
    assert (want["hits"][~inside] == 0).all() and len(f.xs) == inside.sum()


# ---- 2. the inputs earn their keep ------------------------------------------------------------------------------------------
def test_inputs_earn_their_keep(world):
    """from the oracle alone, over the set the GPU tests render (three scenes, the single frame and the three views each, spp 5):
    at least 5 % of the samples miss, at least 5 % of the pixels have 0 < hits < spp, a pixel sees a light, and the first hits
    carry materials that only spheres, only boxes, only cylinders and only triangles carry"""
    fr = [f for name in SCENES for f in fc.frames(world(name))]
    miss, partial, lights = fc.stats_of(fr, 5)
    print("misses %.3f of the samples, partial coverage %.3f of the pixels, %d pixels see a light first" % (miss, partial, lights))
    assert miss >= 0.05 and partial >= 0.05 and lights >= 1
    kinds = set()
    for name in SCENES:
        w = world(name)
        flat = w.flat
        carriers = {"sphere": set(flat.spheres["mat"]), "box": set(flat.boxes["mat"]), "cylinder": set(flat.cylinders["mat"]),
                    "triangle": {m["mat"] for m in flat.meshes}}
        seen = set(np.unique(np.concatenate([f.mat.reshape(-1) for f in fc.frames(w)]))) - {0}
        for kind, mats in carriers.items():
            others = set().union(*[v for k, v in carriers.items() if k != kind])
            if seen & (mats - others):
                kinds.add(kind)
    assert kinds == {"sphere", "box", "cylinder", "triangle"}, kinds


# ---- 3. the C ABI -----------------------------------------------------------------------------------------------------------
def test_entry_points_have_c_linkage(api):
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NAMES <= names
    assert NAMES <= set(api.EXPORTS)
    hdr = open(os.path.join(os.path.dirname(DATA), "include", "ort.h")).read()
    assert all(n + "(" in hdr for n in NAMES)
    assert api.lib().ort_abi_version() == 3   # additive: the ABI version stands
    assert ctypes.sizeof(api.FeaturePlanes) == 48
    section = hdr[hdr.index("first-hit feature renders"):hdr.index("int ort_render_features(")]
    for word in ("in ort_render_views_adaptive's order with the planes where ad stands", "ORT_ERR_INVALID", "ORT_ERR_UNSUPPORTED", "ORT_ERR_STATE",
                 "ORT_ERR_NO_DEVICE", "job_seed(seed, y*W + x)", "TWO steps", "ray.cpp:1233-1234", "ray.cpp:1237", "A / (float)spp",
                 "left untouched in every plane", "Four identities", "0, ORT_NO_PRIM", "exactly 2*spp steps", "not re-normalised"):
        assert word in section, word
    order = [section.rindex(k) for k in ("ORT_ERR_INVALID (", "ORT_ERR_UNSUPPORTED (policy", "ORT_ERR_STATE (", "ORT_ERR_NO_DEVICE (")]
    assert order == sorted(order)


def _caller(api, views_form, device_form):
    """call(handle, params, planes[, views, count]) through one of the four entry points; planes: a FeaturePlanes or None"""
    L = api.lib()
    cam = api.View()

    def call(handle, p, planes, views="own", count=1, stats=None):
        fp = ctypes.byref(planes) if planes is not None else None
        pp = ctypes.byref(p) if p is not None else None
        if views_form:
            v = ctypes.addressof(cam) if isinstance(views, str) else views
            if device_form:
                return L.ort_render_views_features_device(handle, pp, v, count, fp, None, stats)
            return L.ort_render_views_features(handle, pp, v, count, fp, stats)
        if device_form:
            return L.ort_render_features_device(handle, pp, fp, None, stats)
        return L.ort_render_features(handle, pp, fp, stats)
    return call, cam


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("views_form", [False, True])
@pytest.mark.parametrize("committed", [True, False])
def test_errors_come_in_order(api, views_form, device_form, committed):
    """INVALID (the null planes struct, no feature plane, null views, the view cap, the params, then spp above 1 << 24 and a
    misaligned plane), UNSUPPORTED (policy, shard, packed, a camera outside the box), then the scene's state: STATE before
    NO_DEVICE.  On a committed-but-not-uploaded scene and on an uncommitted one, so every error comes before any device work"""
    s = _scene(api, committed)
    L = api.lib()
    call, view = _caller(api, views_form, device_form)
    cam = s.camera(8, 8)
    for k, name in enumerate(("p", "x_axis", "y_axis", "z_axis")):
        setattr(view.camera, name, api.V3(*[float(c) for c in cam[k]]))
    keep = [_aligned(8 * 8 * 12) for _ in range(6)]
    ptr = dict(zip(("albedo", "normal", "depth", "hits", "ids", "final_states"), (k[1] for k in keep)))
    full = api.FeaturePlanes(**ptr)
    state = api.ERR_NO_DEVICE if committed else api.ERR_STATE
    bad_p = _params(api, width=0)
    # nulls first: before bad params
    assert call(s.handle, bad_p, None) == api.ERR_INVALID
    assert b"planes" in L.ort_last_error()
    assert call(s.handle, bad_p, api.FeaturePlanes()) == api.ERR_INVALID
    assert b"no feature plane" in L.ort_last_error()
    assert call(s.handle, bad_p, api.FeaturePlanes(final_states=ptr["final_states"])) == api.ERR_INVALID   # the states are no feature plane
    assert b"no feature plane" in L.ort_last_error()
    if views_form:
        assert call(s.handle, bad_p, full, views=None) == api.ERR_INVALID
        assert b"views" in L.ort_last_error()
        assert call(s.handle, bad_p, full, count=api.MAX_VIEWS + 1) == api.ERR_INVALID
        assert b"ORT_MAX_VIEWS" in L.ort_last_error()
    assert call(None, _params(api), full) == api.ERR_INVALID
    assert call(s.handle, None, full) == api.ERR_INVALID
    # the params, as the render call judges them, before the planes' alignment; chunk and rr are ignored
    odd = api.FeaturePlanes(**{**ptr, "depth": ptr["depth"] + 2})
    for p, word in ((bad_p, b"image size"), (_params(api, rect=(4, 4, 4, 8)), b"rect"), (_params(api, rect=(0, 0, 9, 8)), b"rect"),
                    (_params(api, spp=0), b"spp"), (_params(api, policy=7), b"policy"), (_params(api, shard=(3, 2)), b"shard index")):
        assert call(s.handle, p, odd) == api.ERR_INVALID, word
        assert word in L.ort_last_error(), (word, L.ort_last_error())
    assert call(s.handle, _params(api, width=70000, height=1), odd) == api.ERR_UNSUPPORTED   # as the render call: 16-bit coordinates
    # spp above 1 << 24 and the alignment, before what the call does not do
    chunky = _params(api, policy="chunk", spp=(1 << 24) + 1, shard=(0, 2), packed=True)
    assert call(s.handle, chunky, odd) == api.ERR_INVALID
    assert b"1 << 24" in L.ort_last_error()
    chunky.spp = 1 << 24
    for name in ptr:
        assert call(s.handle, chunky, api.FeaturePlanes(**{**ptr, name: ptr[name] + (1 if name == "ids" else 2)})) == api.ERR_INVALID, name
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
    # all of these come before the scene's state; good arguments reach it: one plane alone, the limits, chunk and rr as they come
    assert call(s.handle, _params(api, spp=1, chunk=5, rr=-3.0), api.FeaturePlanes(hits=ptr["hits"])) == state
    assert call(s.handle, _params(api, spp=1 << 24, rr=float("nan")), full) == state
    assert (b"commit" if not committed else b"upload") in L.ort_last_error()


@pytest.mark.parametrize("device_form", [False, True])
def test_empty_batch_is_ok(api, device_form):
    """view_count == 0: ORT_OK without a launch, whatever the other arguments"""
    call, _ = _caller(api, True, device_form)
    for s in (_scene(api), _scene(api, committed=False)):
        assert call(s.handle, None, None, views=None, count=0) == api.OK
        assert call(s.handle, _params(api, width=0, policy="whole"), api.FeaturePlanes(), count=0) == api.OK
    assert call(None, None, None, views=None, count=0) == api.OK
    st = api.Stats()
    st.rays = 7
    assert call(_scene(api).handle, None, None, views=None, count=0, stats=ctypes.byref(st)) == api.OK
    assert st.rays == 0


def test_python_shapes(api):
    s = _scene(api)
    with pytest.raises(api.OrtError) as e:
        s.render_features(8, 6, 4, 3, want=("depth", "states"))
    assert e.value.code == api.ERR_NO_DEVICE
    with pytest.raises(api.OrtError) as e:
        s.render_features(8, 6, 0, 3)
    assert e.value.code == api.ERR_INVALID
    for bad in ((), ("depth", "depth"), ("colour",)):
        with pytest.raises(ValueError):
            s.render_features(8, 6, 4, 3, want=bad)
    good = fc.guard_planes((6, 8), ("depth", "ids"))
    for bad in ({"depth": good["depth"]}, {**good, "depth": good["depth"].astype("<f8")}, {**good, "ids": good["ids"][:, ::2]},
                {**good, "ids": np.zeros((6, 8), "<u4")}, {**good, "hits": np.zeros((6, 8), "<u4")}):
        with pytest.raises(ValueError):
            s.render_features(8, 6, 4, 3, want=("depth", "ids"), out=bad)
    cams = np.stack([s.camera(8, 6)] * 2)
    for bad_cams, bad_seeds in ((cams[:, :3], [1, 2]), (cams, [1]), (cams[0], [1, 2])):
        with pytest.raises(ValueError):
            s.render_views_features(bad_cams, bad_seeds, 8, 6, 4)
    with pytest.raises(ValueError):
        s.render_views_features(cams, [1, 2], 8, 6, 4, want=("depth", "ids"), out=good)   # one frame's planes for two views
    with pytest.raises(api.OrtError) as e:
        s.render_views_features(cams, [1, 2], 8, 6, 4)
    assert e.value.code == api.ERR_NO_DEVICE
    planes, st = s.render_views_features(np.zeros((0, 4, 3), "<f4"), [], 8, 6, 4, want=fc.PLANES)
    assert planes["albedo"].shape == planes["normal"].shape == (0, 6, 8, 3) and planes["ids"].shape == (0, 6, 8, 2)
    assert planes["depth"].shape == planes["hits"].shape == planes["states"].shape == (0, 6, 8) and st["rays"] == 0
    assert all(planes[k].dtype == np.dtype(fc.DTYPES[k]) for k in fc.PLANES)
    p = s.params(8, 6, 4, 1, "pixel")
    with pytest.raises(ValueError):
        s.render_features_device(p, colour=64)
    for call in (lambda: s.render_features_device(p, depth=64, ids=128), lambda: s.render_views_features_device(p, cams, [1, 2], hits=64)):
        with pytest.raises(api.OrtError) as e:
            call()
        assert e.value.code == api.ERR_NO_DEVICE


# ---- 4. the launch plan -----------------------------------------------------------------------------------------------------------
def test_launch_plan_prints_the_feature_plan():
    """plan_features: plan_ray_query's grid and thresholds over [view][block under the rect][pixel in block]; tabs asks for the
    prologue's table and the materials'; the batches are the render's, and read their knobs"""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "launch_plan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    tool = os.path.join(ROOT, "tools", "launch_plan")

    def plan(env=None, **kw):
        e = {k: v for k, v in os.environ.items() if not k.startswith("ORT_")}
        e.update(env or {})
        out = subprocess.check_output([tool, "query=features"] + ["%s=%s" % kv for kv in kw.items()], env=e).decode().splitlines()
        return json.loads(out[0]), dict(l.split(" = ") for l in out[1:])
    hd = dict(width=1920, height=1080, x1=1920, y1=1080, materials=8)
    ray = json.loads(subprocess.check_output([tool, "query=raycast", "count=%d" % (240 * 135 * 64), "materials=8"]))
    for counters in (0, 1):
        pl, _ = plan(counters=counters, **hd)
        assert pl["count"] == pl["view_jobs"] == 240 * 135 * 64 and pl["view_count"] == 1 and pl["counters"] == counters and pl["tabs"] == 1
        assert all(pl[k] == ray[k] for k in ("grid", "refill_below", "descend_below", "diffuse"))
        assert pl["job_batch"] == 64
    assert plan(**{**hd, "materials": 60})[0]["tabs"] == 0 and plan(**{**hd, "pro_boxes": 30})[0]["tabs"] == 0
    assert json.loads(subprocess.check_output([tool, "query=raycast", "count=9", "materials=60"]))["tabs"] == 1   # that query reads no materials
    pl, _ = plan({"ORT_JOB_BATCH": "7", "ORT_BATCH_TAIL": "1"}, **hd)
    assert pl["job_batch"] == 7 and pl["batch_until"] == pl["count"] - pl["grid"] * 256
    pl, fill = plan(views=3, x0=3, y0=2, fill=1, spp=5, **{**hd, "width": 24, "height": 16, "x1": 21, "y1": 13})
    assert pl["view_jobs"] == 6 * 64 and pl["count"] == 3 * 6 * 64 and pl["grid"] == 5
    want = dict(mode=1, W=24, H=16, x0=3, y0=2, x1=21, y1=13, spp=5, job_count=1152, view_jobs=384, view_count=3, blocks_w=3, block_x0=0, block_y0=0,
                my_blocks=6, shard_count=1, refill_below=pl["refill_below"], job_batch=pl["job_batch"])
    assert {k: int(fill[k]) for k in want} == want
    assert subprocess.run([tool, "query=features", "width=8", "height=8", "x1=9", "y1=8"], capture_output=True).returncode == 2


# ---- 5. the lane code on host threads ---------------------------------------------------------------------------------------
def _single(got):
    return {k: v[0] for k, v in got.items()}


@pytest.mark.parametrize("name,envs", [("c2_analytic", [{}, {"SIM_TABS": "1"}]), ("c3_bunny_room", [{}, {"SIM_TABS": "1"}]), ("open", [{}, {"SIM_TABS": "1"}]),
                                       ("tables_mats_over", [{}])])
def test_host_sim_is_the_reference(host_sim, world, tmp_path, name, envs):
    """all six planes, all bits, the single frame and the batch of three views, spp 1 and 5, the tables in LDS form and from their
    arrays, one thread and eight; the shapes of the ids are tools/host_sim --raycast's for the helper's rays (identity 1)"""
    w = world(name)
    for k, env in enumerate(envs):
        for spp in fc.SPPS:
            one, batch = fc.expected_set(w, spp)
            got, r = fc.host_sim(host_sim, tmp_path, w.scn, fc.W, fc.H, None, spp, seed=fc.SEED, base=w.base, env=env, threads=1 if k else 8)
            fc.assert_same(_single(got), one, "%s single spp %d %r" % (name, spp, env))
            assert hs.counters(r)["rays"] == fc.W * fc.H * spp and hs.counters(r)["paths"] == 0
            gotb, _ = fc.host_sim(host_sim, tmp_path, w.scn, fc.W, fc.H, None, spp, cams=w.cams, seeds=w.seeds, base=w.base, env=env, threads=8)
            fc.assert_same(gotb, batch, "%s batch spp %d %r" % (name, spp, env))
            if spp == 1 and not k:
                fr = fc.frames(w)
                rays = np.concatenate([f.rays[:, 0] for f in fr])
                hits, _ = hs.raycast(host_sim, tmp_path, w.scn, rays, base=w.base, env=env)
                ids = np.concatenate([got["ids"].reshape(-1, 2), gotb["ids"].reshape(-1, 2)])
                depth = np.concatenate([got["depth"].reshape(-1), gotb["depth"].reshape(-1)])
                normal = np.concatenate([got["normal"].reshape(-1, 3), gotb["normal"].reshape(-1, 3)])
                hit = hits["mat"] != 0
                assert (ids[:, 0] == hits["mat"]).all() and (ids[:, 1] == hits["prim"]).all()
                assert (depth[hit].view("<u4") == hits["t"][hit].view("<u4")).all() and (depth[~hit] == 0).all()
                assert (normal.view("<u4") == hits["n"].view("<u4")).all()


def test_host_sim_rect_planes_alone_and_forced_walk(host_sim, world, tmp_path):
    """the rect (3, 2, 21, 13) cuts blocks on all four sides: its pixels are the reference's in every plane, those outside keep
    their guard words; each plane asked for alone has the bits it has with all six; the exact walk forced on the rays whose
    direction's low bits are zero changes no bit"""
    w = world("open")
    one, batch = fc.expected_set(w, 5, fc.RECT, fc.GUARDS)
    inside = np.zeros((fc.H, fc.W), bool)
    inside[fc.RECT[1]:fc.RECT[3], fc.RECT[0]:fc.RECT[2]] = True
    assert (one["hits"][~inside] == fc.GUARDS["hits"]).all() and (one["hits"][inside] <= 5).all()
    got, _ = fc.host_sim(host_sim, tmp_path, w.scn, fc.W, fc.H, fc.RECT, 5, cams=w.cams, seeds=w.seeds, base=w.base, threads=8)
    fc.assert_same(got, batch, "rect, batch")
    for k in ("ids", "albedo"):   # the guards outside the rect, the hits' shapes included
        assert (got[k][:, ~inside].view("<u4") == np.asarray(fc.GUARDS[k], fc.DTYPES[k]).view("<u4")).all()
    for k in fc.PLANES[:5]:
        alone, _ = fc.host_sim(host_sim, tmp_path, w.scn, fc.W, fc.H, fc.RECT, 5, cams=w.cams, seeds=w.seeds, want=(k,), base=w.base, threads=8)
        assert set(alone) == {k} and (alone[k].view("<u4") == got[k].view("<u4")).all(), k
    forced, r = fc.host_sim(host_sim, tmp_path, w.scn, fc.W, fc.H, fc.RECT, 5, cams=w.cams, seeds=w.seeds, base=w.base, threads=8, env={"SIM_FORCE_FALLBACK": "0xf"})
    assert hs.counters(r)["fallback"] > 0
    for k in fc.PLANES:
        assert (forced[k].view("<u4") == got[k].view("<u4")).all(), k


# ---- 6. under the sanitizers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c2_analytic", "c3_bunny_room"])
def test_host_sim_under_sanitizers(world, tmp_path, name):
    """tools/host_sim_san (the stand-alone ASan + UBSan binary, run directly): the single frame and the batch at spp 5, a rect that
    cuts blocks, planes left out: ends clean, with the reference's planes"""
    san = hs.built("host_sim_san")
    w = world(name)
    one, batch = fc.expected_set(w, 5)
    for env in ({}, {"SIM_TABS": "1"}):
        got, _ = fc.host_sim(san, tmp_path, w.scn, fc.W, fc.H, None, 5, seed=fc.SEED, base=w.base, env=env, threads=2)
        fc.assert_same(_single(got), one, "sanitized %s %r" % (name, env))
    got, _ = fc.host_sim(san, tmp_path, w.scn, fc.W, fc.H, None, 5, cams=w.cams, seeds=w.seeds, want=("normal", "ids", "states"), base=w.base, threads=2)
    fc.assert_same(got, batch, "sanitized %s batch" % name)
    _, rect = fc.expected_set(w, 5, fc.RECT, fc.GUARDS)
    got, _ = fc.host_sim(san, tmp_path, w.scn, fc.W, fc.H, fc.RECT, 5, cams=w.cams, seeds=w.seeds, base=w.base, threads=2)
    fc.assert_same(got, rect, "sanitized %s rect" % name)
