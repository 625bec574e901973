"""Path-depth renders (ort_render_depths, ort_render_views_depths and their device forms), host side: the helper that turns the
oracle into their reference (tests/depths_cases.py: the fold over chains of one-sample calls) pinned against the oracle's own
PIXEL render, the scenes shown not to be vacuous, the C ABI surface and its errors in the order include/ort.h gives them, the
launch plan, and the lane code with the bin sums run on host threads (tools/host_sim --depths), plain and under ASan + UBSan,
against the fold bit for bit."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import depths_cases as dc
import host_sim_tool as hs
from conftest import DATA, ROOT
from host_cases import aligned as _aligned, params as _params, scene as _scene

NAMES = {"ort_render_depths", "ort_render_depths_device", "ort_render_views_depths", "ort_render_views_depths_device"}
_bits = dc.bits


@pytest.fixture()
def case(api, oracle, tmp_path_factory):
    return lambda name: dc.case(api, oracle, name, tmp_path_factory)


@pytest.fixture(scope="module")
def host_sim():
    return hs.built("host_sim")


# ---- 1. the helper against the oracle alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.SCENES)
def test_one_bin_is_the_pixel_render(case, name):
    """the G = 1 fold is the oracle's PIXEL frame in every bit, its states are the jobs' states and its lengths are spp, at both
    sample counts, whole frame and rect"""
    c = case(name)
    for spp in dc.SPPS:
        B, N, rgb, st = dc.expected(c, 1, spp)
        for rect in (None, dc.RECT):
            m = dc.inside(rect)
            assert (_bits(B[0])[m] == _bits(c.frame(None, spp, rect=rect))[m]).all()
            assert (st[m] == c.states(spp, rect=rect)[m]).all()
        assert (_bits(B[0]) == _bits(rgb)).all() and (N == spp).all()


@pytest.mark.parametrize("name", dc.SCENES)
def test_identities_hold_on_the_fold(case, name):
    """identity 3: below the last bin, a frame and a length plane do not depend on G; the lengths of a pixel add up to spp;
    identity 4: without the roulette no path bounces, and everything lies in bin 0"""
    c = case(name)
    for spp in dc.SPPS:
        folds = {G: dc.expected(c, G, spp) for G in dc.BINS}
        for G in dc.BINS:
            assert (folds[G][1].sum(axis=0) == spp).all()
            assert (_bits(folds[G][2]) == _bits(folds[1][2])).all() and (folds[G][3] == folds[1][3]).all()
        for g in range(2):
            assert (_bits(folds[3][0][g]) == _bits(folds[8][0][g])).all() and (folds[3][1][g] == folds[8][1][g]).all()
        assert (folds[3][1][2] == folds[8][1][2:].sum(axis=0)).all()
    ch0 = dc.chains(c, n=4, rr=0.0)
    assert (ch0.depth == 0).all()
    B, N, rgb, _ = dc.fold(ch0, 3, 4)
    assert (_bits(B[1:]) == 0).all() and (N[0] == 4).all() and (N[1:] == 0).all() and (_bits(B[0]) == _bits(rgb)).all()
    assert name not in dc.ANALYTIC or (B[0] != 0).any()   # lights seen directly


# ---- 2. not vacuous, as conditions -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.ANALYTIC)
def test_bins_are_not_vacuous(case, name):
    """from the oracle alone on the whole 24 x 16 frame at 16 spp, seed 2024, rr 0.8, the scene's own camera, G = 8: every bin's
    frame is non-zero on at least 0.02 of the pixels, at least 0.25 of the pixels are non-zero in two or more bins, at least 600
    of the 6144 samples are clamped into bin 7, and the float32 sum of the bins differs from the full frame in some pixel but by at
    most 1e-5"""
    assert (dc.W, dc.H, dc.SEED, dc.RR, dc.SPPS[0]) == (24, 16, 2024, 0.8, 16)
    c = case(name)
    ch = dc.chains(c)
    B, N, rgb, _ = dc.fold(ch, 8, 16)
    lit = (B != 0).any(axis=3)
    shares = lit.reshape(8, -1).mean(axis=1)
    several = (lit.sum(axis=0) >= 2).mean()
    clamped = int(N[7].sum())   # the samples whose last ray has depth 7 or more
    s = np.zeros_like(rgb)
    for g in range(8):
        s = (s + B[g]).astype("<f4")
    differ = (_bits(s) != _bits(rgb)).any(axis=2).mean()
    err = float(np.abs(s - rgb).max())
    print("%s: lit share per bin %s, by two or more %.3f, clamped into bin 7 %d of %d, deepest %d, sum differs on %.3f of the pixels by at most %.3g"
          % (name, " ".join("%.3f" % x for x in shares), several, clamped, ch.depth.size, int(ch.depth.max()), differ, err))
    assert ch.depth.size == 6144
    assert (shares >= 0.02).all() and several >= 0.25 and clamped >= 600
    assert differ > 0 and err <= 1e-5


# ---- 3. the C ABI ------------------------------------------------------------------------------------------------------------
def test_entry_points_have_c_linkage(api):
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NAMES <= names
    assert NAMES <= set(api.EXPORTS)
    hdr = open(os.path.join(os.path.dirname(DATA), "include", "ort.h")).read()
    assert all(n + "(" in hdr for n in NAMES)
    assert api.lib().ort_abi_version() == 3   # additive: the ABI version stands
    assert (api.MAX_DEPTH_BINS, api.DEPTH_EMISSION, api.DEPTH_DIRECT, api.DEPTH_INDIRECT) == (8, 0, 1, 2)
    for line in ("#define ORT_MAX_DEPTH_BINS 8u", "#define ORT_DEPTH_EMISSION 0u", "#define ORT_DEPTH_DIRECT   1u", "#define ORT_DEPTH_INDIRECT 2u"):
        assert line in hdr, line
    section = hdr[hdr.index("path-depth renders"):hdr.index("int ort_render_depths(")]
    for word in ("in ort_render_light_groups' order with the bin count where the groups stand", "ORT_ERR_INVALID", "ORT_ERR_UNSUPPORTED", "ORT_ERR_STATE",
                 "ORT_ERR_NO_DEVICE", "job_seed(seed, y*W + x)", "min(d, G - 1)", "B_bin(d) = B_bin(d) + e", "N_bin(d) = N_bin(d) + 1", "B_g / (float)spp",
                 "((v*G + g) * height*width*3)", "((v*G + g) * height*width)", "left untouched in every plane", "Six identities", "add up to spp",
                 "is not a new depth", "paths = view_count x rect pixels x spp"):
        assert word in section, word
    order = [section.rindex(k) for k in ("ORT_ERR_INVALID (", "ORT_ERR_UNSUPPORTED (policy", "ORT_ERR_STATE (", "ORT_ERR_NO_DEVICE (")]
    assert order == sorted(order)


def _caller(api, views_form, device_form):
    """call(handle, params, G, out_bins, out_rgb, out_lengths, states[, views, count]) through one of the four entry points"""
    L = api.lib()
    cam = api.View()

    def call(handle, p, G, out, rgb, lengths, states, views="own", count=1, stats=None):
        pp = ctypes.byref(p) if p is not None else None
        if views_form:
            v = ctypes.addressof(cam) if isinstance(views, str) else views
            if device_form:
                return L.ort_render_views_depths_device(handle, pp, G, v, count, out, rgb, lengths, states, None, stats)
            return L.ort_render_views_depths(handle, pp, G, v, count, out, rgb, lengths, states, stats)
        if device_form:
            return L.ort_render_depths_device(handle, pp, G, out, rgb, lengths, states, None, stats)
        return L.ort_render_depths(handle, pp, G, out, rgb, lengths, states, stats)
    return call, cam


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("views_form", [False, True])
@pytest.mark.parametrize("committed", [True, False])
def test_errors_come_in_order(api, views_form, device_form, committed):
    """INVALID (nulls, the view cap, the params, spp above 1 << 24, then the bin count and the planes' alignment), UNSUPPORTED
    (policy, shard, packed, a camera outside the box), then the scene's state: STATE before NO_DEVICE.  On a committed-but-not-
    uploaded scene and on an uncommitted one, so every error comes before any device work"""
    s = _scene(api, committed)
    L = api.lib()
    call, view = _caller(api, views_form, device_form)
    cam = s.camera(8, 8)
    for k, name in enumerate(("p", "x_axis", "y_axis", "z_axis")):
        setattr(view.camera, name, api.V3(*[float(c) for c in cam[k]]))
    keep = [_aligned(8 * 8 * 8 * 12), _aligned(8 * 8 * 12), _aligned(8 * 8 * 8 * 4), _aligned(256)]
    out, rgb, lens, fin = (k[1] for k in keep)
    state = api.ERR_NO_DEVICE if committed else api.ERR_STATE
    nan = float("nan")
    BAD_G = 0
    # nulls first: before bad params and a bad bin count
    assert call(s.handle, _params(api, width=0), BAD_G, None, rgb, lens, fin) == api.ERR_INVALID
    assert b"bin frames" in L.ort_last_error()
    if views_form:
        assert call(s.handle, _params(api, width=0), BAD_G, out, rgb, lens, fin, views=None) == api.ERR_INVALID
        assert b"views" in L.ort_last_error()
        assert call(s.handle, _params(api, width=0), BAD_G, out, rgb, lens, fin, count=api.MAX_VIEWS + 1) == api.ERR_INVALID
        assert b"ORT_MAX_VIEWS" in L.ort_last_error()
    assert call(None, _params(api), 3, out, rgb, lens, fin) == api.ERR_INVALID
    assert call(s.handle, None, 3, out, rgb, lens, fin) == api.ERR_INVALID
    # the params, as the render call judges them, before the bin count; chunk is ignored
    for p, word in ((_params(api, width=0), b"image size"), (_params(api, rect=(4, 4, 4, 8)), b"rect"), (_params(api, rect=(0, 0, 9, 8)), b"rect"),
                    (_params(api, spp=0), b"spp"), (_params(api, rr=-0.5), b"rr"), (_params(api, rr=nan), b"rr"), (_params(api, policy=7), b"policy"),
                    (_params(api, shard=(3, 2)), b"shard index")):
        assert call(s.handle, p, BAD_G, out, rgb, lens, fin) == api.ERR_INVALID, word
        assert word in L.ort_last_error(), (word, L.ort_last_error())
    assert call(s.handle, _params(api, width=70000, height=1), BAD_G, out, rgb, lens, fin) == api.ERR_UNSUPPORTED   # as the render call: 16-bit coordinates
    assert call(s.handle, _params(api, spp=(1 << 24) + 1), BAD_G, out, rgb, lens, fin) == api.ERR_INVALID
    assert b"1 << 24" in L.ort_last_error()
    # the bin count, then the alignment, before what the call does not do
    chunky = _params(api, policy="chunk", spp=7, chunk=3, shard=(0, 2), packed=True)
    for G in (0, api.MAX_DEPTH_BINS + 1, 0xFFFFFFFF):
        assert call(s.handle, chunky, G, out + 2, rgb, lens, fin) == api.ERR_INVALID
        assert b"bin_count" in L.ort_last_error()
    for planes in ((out + 2, rgb, lens, fin), (out, rgb + 1, lens, fin), (out, rgb, lens + 3, fin), (out, rgb, lens, fin + 2)):
        assert call(s.handle, chunky, 3, *planes) == api.ERR_INVALID
        assert b"4-byte aligned" in L.ort_last_error()
    # what the call does not do: any policy but PIXEL, shards, a packed framebuffer
    for policy in ("tile32", "whole", "chunk"):
        assert call(s.handle, _params(api, policy=policy, shard=(0, 2) if policy == "chunk" else (0, 1)), 3, out, rgb, lens, fin) == api.ERR_UNSUPPORTED
        assert b"PIXEL" in L.ort_last_error()
    assert call(s.handle, _params(api, shard=(1, 2), packed=True), 3, out, rgb, lens, fin) == api.ERR_UNSUPPORTED
    assert b"shard" in L.ort_last_error()
    assert call(s.handle, _params(api, packed=True), 3, out, rgb, lens, fin) == api.ERR_UNSUPPORTED
    assert b"packed" in L.ort_last_error()
    if views_form:   # a camera outside the box, naming the view
        two = (api.View * 2)(view, view)
        two[1].camera.p = api.V3(1e6, 0.0, 0.0)
        assert call(s.handle, _params(api), 3, out, rgb, lens, fin, views=ctypes.addressof(two), count=2) == api.ERR_UNSUPPORTED
        assert b"view 1" in L.ort_last_error()
    # all of these come before the scene's state; good arguments reach it: the optional planes NULL, the limits
    assert call(s.handle, _params(api, spp=1 << 24, chunk=5, rr=7.5), api.MAX_DEPTH_BINS, out, None, None, None) == state
    for G in (1, 3, 8):
        assert call(s.handle, _params(api), G, out, rgb, lens, fin) == state
    assert (b"commit" if not committed else b"upload") in L.ort_last_error()


@pytest.mark.parametrize("device_form", [False, True])
def test_empty_batch_is_ok(api, device_form):
    """view_count == 0: ORT_OK without a launch, whatever the other arguments"""
    call, _ = _caller(api, True, device_form)
    for s in (_scene(api), _scene(api, committed=False)):
        assert call(s.handle, None, 0, None, None, None, None, views=None, count=0) == api.OK
        assert call(s.handle, _params(api, width=0, policy="whole"), 99, None, None, None, None, count=0) == api.OK
    assert call(None, None, 0, None, None, None, None, views=None, count=0) == api.OK
    st = api.Stats()
    st.rays = 7
    assert call(_scene(api).handle, None, 0, None, None, None, None, views=None, count=0, stats=ctypes.byref(st)) == api.OK
    assert st.rays == 0


def test_python_shapes(api):
    s = _scene(api)
    with pytest.raises(api.OrtError) as e:
        s.render_depths(8, 6, 4, 3)
    assert e.value.code == api.ERR_NO_DEVICE
    for G in (0, 9):
        with pytest.raises(api.OrtError) as e:
            s.render_depths(8, 6, 4, 3, bins=G)
        assert e.value.code == api.ERR_INVALID
    for bad in (("rgb", "rgb"), ("m2",), ("bins",)):
        with pytest.raises(ValueError):
            s.render_depths(8, 6, 4, 3, want=bad)
    planes = {"bins": np.zeros((3, 6, 8, 3), "<f4"), "rgb": np.zeros((6, 8, 3), "<f4"), "lengths": np.zeros((3, 6, 8), "<u4")}
    for bad in ({"bins": planes["bins"]}, dict(planes, lengths=planes["lengths"].astype("<i8")), dict(planes, bins=np.zeros((2, 6, 8, 3), "<f4")),
                [planes["bins"], planes["rgb"], planes["lengths"]]):
        with pytest.raises(ValueError):
            s.render_depths(8, 6, 4, 3, want=("rgb", "lengths"), out=bad)
    with pytest.raises(api.OrtError) as e:
        s.render_depths(8, 6, 4, 3, want=("lengths", "rgb"), out=planes)
    assert e.value.code == api.ERR_NO_DEVICE
    cams = np.stack([s.camera(8, 6)] * 2)
    for bad_cams, bad_seeds in ((cams[:, :3], [1, 2]), (cams, [1]), (cams[0], [1, 2])):
        with pytest.raises(ValueError):
            s.render_views_depths(bad_cams, bad_seeds, 8, 6, 4)
    with pytest.raises(ValueError):
        s.render_views_depths(cams, [1, 2], 8, 6, 4, want=("rgb", "lengths"), out=planes)   # one frame's planes for two views
    with pytest.raises(api.OrtError) as e:
        s.render_views_depths(cams, [1, 2], 8, 6, 4)
    assert e.value.code == api.ERR_NO_DEVICE
    fr, others, st = s.render_views_depths(np.zeros((0, 4, 3), "<f4"), [], 8, 6, 4, bins=8, want=("rgb", "lengths", "states"))
    assert fr.shape == (0, 8, 6, 8, 3) and fr.dtype == np.dtype("<f4") and st["paths"] == 0
    assert {k: v.shape for k, v in others.items()} == {"rgb": (0, 6, 8, 3), "lengths": (0, 8, 6, 8), "states": (0, 6, 8)}
    fr, others, st = s.render_views_depths(np.zeros((0, 4, 3), "<f4"), [], 8, 6, 4, want=())
    assert fr.shape == (0, 3, 6, 8, 3) and others == {}
    p = s.params(8, 6, 4, 1, "pixel")
    for call in (lambda: s.render_depths_device(p, 3, 64), lambda: s.render_views_depths_device(p, cams, [1, 2], 3, 64)):
        with pytest.raises(api.OrtError) as e:
            call()
        assert e.value.code == api.ERR_NO_DEVICE


# ---- 4. the launch plan ------------------------------------------------------------------------------------------------------
def test_launch_plan_names_the_depths_kernels():
    """plan_pixel_jobs, RK_DEPTHS: the plain loop over implicit one-pixel jobs of a batch of views, both BSDF flavours with counters,
    whatever the knobs say; its variant is depths<...> and is built; in every other field the light-group render's launch; the
    plans of the other calls name what they named"""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "launch_plan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    tool = os.path.join(ROOT, "tools", "launch_plan")

    def plan(env=None, **kw):
        e = {k: v for k, v in os.environ.items() if not k.startswith("ORT_")}
        e.update(env or {})
        return json.loads(subprocess.check_output([tool] + ["%s=%s" % kv for kv in kw.items()], env=e))
    frame = dict(policy="pixel", width=1920, height=1080, x1=1920, y1=1080, materials=8, lights=2, diffuse_only=1, sah_cost=0.5, spp=16)
    forced = {"ORT_EXCHANGE": "1", "ORT_WAVES5": "1", "ORT_WIDE": "1", "ORT_MODE": "wavefront", "ORT_DEBUG_UTIL": "1"}
    for env in ({}, forced):
        for counters in (0, 1):
            pl = plan(env, depths=1, variant=1, counters=counters, has_wide=1, **frame)
            assert pl["depths"] == 1 and pl["views"] == 1 and pl["view_count"] == 1 and pl["implicit"] == 1 and pl["mode"] == 1
            assert not (pl["exchange"] or pl["five"] or pl["wide"] or pl["wavefront"] or pl["util"])
            assert pl["variant"] == "depths<%d, 1, 1, 1, 0>" % counters and pl["built"] == 1
            assert pl["job_count"] == pl["view_jobs"] == 240 * 135 * 64 and pl["grid"] == pl["max_blocks"] == 1024
            assert pl["partial_bytes"] == pl["stash_bytes"] == pl["drain_bytes"] == 0
            same = plan(env, groups=1, counters=counters, has_wide=1, **frame)   # the light-group render's launch in every other field
            assert {k: v for k, v in pl.items() if k not in ("depths", "variant", "built")} == {k: v for k, v in same.items() if k != "groups"}
    pl = plan({"ORT_KERNEL": "general", "ORT_LDS_TABLES": "0"}, depths=1, variant=1, views=3, x0=5, y0=9, **{**frame, "x1": 20, "y1": 17, "width": 27, "height": 19})
    assert pl["variant"] == "depths<0, 0, 0, 1, 0>" and pl["built"] == 1 and pl["view_count"] == 3
    assert pl["view_jobs"] == 3 * 2 * 64 and pl["job_count"] == 3 * pl["view_jobs"] and pl["grid"] == 5
    assert plan(depths=1, variant=1, **{**frame, "materials": 60})["variant"] == "depths<0, 1, 0, 1, 0>"
    # the other calls' plans name what they named
    assert plan(variant=1, **frame)["variant"].startswith(("loop<", "exchange<", "five<"))
    assert plan(variant=1, groups=1, **frame)["variant"] == "groups<0, 1, 1, 1, 0>"
    assert plan(variant=1, accumulate=1, **frame)["variant"] == "accumulate<0, 1, 1, 1, 0>"
    for bad in (["depths=1", "policy=chunk"], ["depths=1", "groups=1", "policy=pixel"], ["depths=1", "policy=pixel", "shard_count=2"]):
        assert subprocess.run([tool, "width=8", "height=8", "x1=8", "y1=8"] + bad, capture_output=True).returncode == 2
    sweep = json.loads(subprocess.check_output([tool, "sweep=1"], env={k: v for k, v in os.environ.items() if not k.startswith("ORT_")}))
    assert sweep["plans"] > 0 and (sweep["unbuilt"], sweep["first"]) == (0, [])


# ---- 5. the lane code on host threads ----------------------------------------------------------------------------------------
def _check(c, got, G, spp, rect, what, seed=dc.SEED, cams=None, seeds=None):
    for v in range(len(got[0])):
        cam, sd = (None, seed) if cams is None else (cams[v], int(seeds[v]))
        dc.assert_planes([None if p is None else p[v] for p in got], dc.expected(c, G, spp, sd, cam), rect, "%s: view %d" % (what, v))


@pytest.mark.parametrize("name", dc.SCENES)
def test_host_sim_is_the_fold(host_sim, case, tmp_path, name):
    """every scene, every bin count, 16 spp and 1, the rect: every plane bit for bit, guards outside the rect intact; the tables in
    LDS form and from their arrays, both BSDF flavours where the scene allows, one thread and eight"""
    c = case(name)
    envs = [{}, {"SIM_TABS": "1"}] if name != dc.lg.TABLE_SCENE else [{}]
    if name == "room_diffuse":
        envs = [{"SIM_DIFFUSE": "1"}, {"SIM_DIFFUSE": "1", "SIM_TABS": "1"}, {}]
    for spp in dc.SPPS:
        for k, env in enumerate(envs):
            for G in (dc.BINS if k == 0 else (3,)):
                for threads in ((8, 1) if k == 0 and spp == 16 and G == 3 else (8,)):
                    got, _ = dc.host_depths(host_sim, tmp_path, c, G, spp, rect=dc.RECT, env=env, threads=threads)
                    _check(c, got, G, spp, dc.RECT, "%s G = %d, %d spp %r, %d threads" % (name, G, spp, env, threads))
    # the whole frame, and the counters' paths: a path per sample
    got, r = dc.host_depths(host_sim, tmp_path, c, 8, 16, threads=8)
    assert hs.counters(r)["paths"] == dc.W * dc.H * 16
    _check(c, got, 8, 16, None, name + ": whole frame")


@pytest.mark.parametrize("name", ["room_all_lobes", "c2_analytic"])
def test_host_sim_optional_planes(host_sim, case, tmp_path, name):
    """NULL optional planes change no bit of the others"""
    c = case(name)
    for want in ((), ("lengths",), ("rgb",), ("states",), ("rgb", "states")):
        got, _ = dc.host_depths(host_sim, tmp_path, c, 3, 16, rect=dc.RECT, want=want, threads=8)
        assert [p is not None for p in got[1:]] == [n in want for n in ("rgb", "lengths", "states")]
        _check(c, got, 3, 16, dc.RECT, "%s: want %r" % (name, want))


@pytest.mark.parametrize("name", dc.lg.ROOMS)
def test_host_sim_batch_of_views(host_sim, api, case, tmp_path, name):
    """three views on three seeds, two of them the same camera: planes (v, .) are the single frame's for that camera and seed"""
    c = case(name)
    cams, seeds = dc.batch_cameras(api, c), dc.BATCH_SEEDS
    assert (cams[0] == cams[2]).all() and (cams[0] != cams[1]).any() and len(set(seeds)) == 3
    for spp, rect, G in ((16, dc.RECT, 3), (1, None, 8)):
        got, _ = dc.host_depths(host_sim, tmp_path, c, G, spp, rect=rect, cams=cams, seeds=seeds, threads=8)
        _check(c, got, G, spp, rect, "%s: batch, %d spp" % (name, spp), cams=cams, seeds=seeds)
        assert (_bits(got[0][0]) != _bits(got[0][2])).any() and (_bits(got[0][0]) != _bits(got[0][1])).any()
    one, _ = dc.host_depths(host_sim, tmp_path, c, 3, 16, rect=dc.RECT, cams=cams[1:2], seeds=seeds[1:2], threads=8)
    _check(c, one, 3, 16, dc.RECT, name + ": batch of one", cams=cams[1:2], seeds=seeds[1:2])


# ---- 6. under the sanitizers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["room_all_lobes", "c2_analytic"])
def test_host_sim_under_sanitizers(case, tmp_path, name):
    """tools/host_sim_san (the stand-alone ASan + UBSan binary, run directly): ends clean, with the fold's planes; the planes are
    exactly as long as the frames, so a write past a plane's end is a write past the block"""
    san = hs.built("host_sim_san")
    c = case(name)
    env = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}
    for extra, spp, rect, G in (({}, 16, dc.RECT, 3), ({"SIM_TABS": "1"}, 1, None, 8)):
        got, _ = dc.host_depths(san, tmp_path, c, G, spp, rect=rect, env=dict(env, **extra), threads=2)
        _check(c, got, G, spp, rect, "%s sanitized %r" % (name, extra))
    got, _ = dc.host_depths(san, tmp_path, c, 1, 1, rect=dc.RECT, want=(), env=env, threads=2)
    _check(c, got, 1, 1, dc.RECT, name + " sanitized, G = 1, no optional plane")
