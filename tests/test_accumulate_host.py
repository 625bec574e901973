"""Accumulating renders (ort_render_accumulate, ort_render_views_accumulate and their device forms), host side: the lane code
pt_lane<..., LF_SPPMAP | LF_ACCUM> run on host threads (tools/host_sim --accumulate, plain and under ASan + UBSan, its planes
chained through files) against the oracle's and the reference's chains folded into undivided sums (tests/accumulate_cases.py),
the launch plan, the C ABI surface with its errors in the order include/ort.h gives them, and the Python Accumulator."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import accumulate_cases as acs
import host_sim_tool as hs
import light_groups_cases as lg
import reference_goldens as rg
import sample_map_cases as sm
from conftest import DATA, ROOT
from host_cases import aligned as _aligned, params as _params, scene as _scene

NAMES = {"ort_render_accumulate", "ort_render_accumulate_device", "ort_render_views_accumulate", "ort_render_views_accumulate_device"}
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}


@pytest.fixture()
def case(api, oracle, tmp_path_factory):
    return lambda name: lg.case(api, oracle, name, tmp_path_factory)


@pytest.fixture(scope="module")
def host_sim():
    return hs.built("host_sim")


# ---- 1. the reference, from the oracle alone ----------------------------------------------------------------------------------
def test_the_fold_is_the_cut_undivided(case):
    """fold() against adaptive_cases.cut on the oracle's chains: the same Q and state, and C / n the same colour; a split fold is
    the whole fold; the model's single call is sample_map_cases.expected"""
    c = case("room_all_lobes")
    chain = sm.chains(c)
    for (x, y) in ((5, 5), (12, 3), (20, 12)):
        cols, states = chain[(x, y)]
        for n in (1, 5, 16):
            C, Q = acs.fold(cols, np.zeros(3, "<f4"), 0, 0, n)
            rgb, took, q, state = acs.ac.cut(cols, states, acs.ac.Adaptive(n, n, 1, 0, 0))
            assert took == n and ((C / np.float32(n)).astype("<f4").view("<u4") == rgb.view("<u4")).all() and Q == q
            C2, Q2 = acs.fold(cols, *acs.fold(cols, np.zeros(3, "<f4"), 0, 0, n // 2), n // 2, n)
            assert (C2.view("<u4") == C.view("<u4")).all() and Q2 == Q
    p = acs.Planes()
    acs.model(p, 0, chain, sm.mixed_map(), acs.CAP, acs.RECT)
    sm.assert_planes((p.rgb[0], p.m2[0], p.states[0]), sm.expected(c, sm.mixed_map(), rect=acs.RECT), "the model's first call")
    assert (p.sum[0][p.count[0] > 1] * np.float32(1) != p.rgb[0][p.count[0] > 1]).any()   # the sums are not the means


# ---- 2. the lane code on host threads -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sm.SCENES)
def test_identity_1_one_call_is_the_sample_map_render(host_sim, case, tmp_path, name):
    c = case(name)
    envs = [{}, {"SIM_TABS": "1"}] if name != lg.TABLE_SCENE else [{}]
    if name == "room_diffuse":
        envs = [{"SIM_DIFFUSE": "1"}, {"SIM_DIFFUSE": "1", "SIM_TABS": "1"}, {}]
    for env in envs:
        got, _ = sm.host_sample_map(host_sim, tmp_path, c, sm.mixed_map(), rect=acs.RECT, env=env, threads=8)
        acs.identity_1(acs.host_call(host_sim, tmp_path, c, env=env, threads=8), c, tuple(g[0] for g in got), "%s %r" % (name, env))


@pytest.mark.parametrize("name", ["room_all_lobes", "c4_dwarf_room"])
def test_identity_2_uniform_split(host_sim, case, tmp_path, name):
    c = case(name)
    img = hs.render(host_sim, tmp_path, c.scn, acs.W, acs.H, 16, acs.SEED, "pixel", 0, base=c.base, threads=8)
    frame = np.where(sm.inside(acs.RECT)[..., None], img.reshape(acs.H, acs.W, 3), acs.GUARD_RGB).astype("<f4")
    for threads in (8, 1):
        acs.identity_2_uniform(acs.host_call(host_sim, tmp_path, c, threads=threads), c, frame, "%s, %d threads" % (name, threads))


def test_identity_2_per_pixel_split(host_sim, case, tmp_path):
    c = case("room_all_lobes")
    for env in ({}, {"SIM_TABS": "1"}):
        acs.identity_2_per_pixel(acs.host_call(host_sim, tmp_path, c, env=env, threads=8), c, "room_all_lobes %r" % (env,))


@pytest.mark.parametrize("name", rg.CHAIN_SCENES)
def test_against_the_references_chains(host_sim, case, tmp_path, name):
    """64 samples as 1 + 3 + 12 + 48 against the fold of chains_rooms.npz: no oracle in between"""
    assert (acs.W, acs.H, acs.SEED, acs.RR) == (rg.rac.W, rg.rac.H, rg.rac.SEED, rg.rac.RR) and sum(acs.REF_SPLIT) == rg.CHAIN_SAMPLES
    c = case(name)
    acs.reference_split(acs.host_call(host_sim, tmp_path, c, threads=8), rg.chains_from(rg.load("chains_rooms.npz"), name), name)


def test_identity_3_hostile_planes_saturation_and_null_map(host_sim, case, tmp_path):
    c = case("room_all_lobes")
    call = acs.host_call(host_sim, tmp_path, c, threads=8)
    acs.identity_3(call, c, "hostile planes")
    acs.saturation(call, c, "saturation")
    acs.null_map(call, c, "no map")


def test_identity_4_optional_planes(host_sim, case, tmp_path):
    c = case("room_diffuse")
    acs.identity_4(acs.host_call(host_sim, tmp_path, c, threads=8), c, "room_diffuse")


def test_identity_5_batch_of_views(host_sim, api, case, tmp_path):
    c = case("room_all_lobes")
    acs.identity_5(acs.host_call(host_sim, tmp_path, c, threads=8), api, c, "room_all_lobes")


def test_host_sim_under_sanitizers(api, case, tmp_path):
    """tools/host_sim_san (the stand-alone ASan + UBSan binary, run directly): every scenario's reads and writes of the caller's
    planes, which are exactly as long as the frames, so an access past a plane's end is one past the block"""
    san = hs.built("host_sim_san")
    c = case("room_all_lobes")
    call = acs.host_call(san, tmp_path, c, env=SAN_ENV, threads=2)
    acs.identity_2_per_pixel(call, c, "sanitized")
    acs.identity_3(call, c, "sanitized, hostile planes")
    acs.saturation(call, c, "sanitized, saturation")
    acs.identity_4(acs.host_call(san, tmp_path, c, env=dict(SAN_ENV, SIM_TABS="1"), threads=2), c, "sanitized, optional planes")
    acs.identity_5(call, api, c, "sanitized, views")


# ---- 3. the launch plan ---------------------------------------------------------------------------------------------------------
def test_launch_plan_names_the_accumulate_kernels():
    """plan_pixel_jobs, RK_ACCUMULATE: the sample-map render's launch in every other field, whatever the knobs say; its variant is
    accumulate<...> and is built"""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "launch_plan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    tool = os.path.join(ROOT, "tools", "launch_plan")

    def plan(env=None, **kw):
        e = {k: v for k, v in os.environ.items() if not k.startswith("ORT_")}
        e.update(env or {})
        return json.loads(subprocess.check_output([tool] + ["%s=%s" % kv for kv in kw.items()], env=e, text=True).splitlines()[0])
    frame = dict(policy="pixel", width=1920, height=1080, x1=1920, y1=1080, materials=8, lights=2, diffuse_only=1, sah_cost=0.5, spp=16)
    forced = {"ORT_EXCHANGE": "1", "ORT_WAVES5": "1", "ORT_WIDE": "1", "ORT_MODE": "wavefront", "ORT_DEBUG_UTIL": "1"}
    for env in ({}, forced):
        for counters in (0, 1):
            pl = plan(env, accumulate=1, variant=1, counters=counters, has_wide=1, **frame)
            assert pl["accumulate"] == 1 and pl["views"] == 1 and pl["implicit"] == 1 and pl["mode"] == 1
            assert pl["variant"] == "accumulate<%d, 1, 1, 1, 0>" % counters and pl["built"] == 1
            same = plan(env, sample_map=1, counters=counters, has_wide=1, **frame)
            assert {k: v for k, v in pl.items() if k not in ("accumulate", "variant", "built")} == {k: v for k, v in same.items() if k != "sample_map"}
    small = {**frame, "x1": 20, "y1": 17, "width": 27, "height": 19}
    pl = plan({"ORT_KERNEL": "general", "ORT_LDS_TABLES": "0"}, accumulate=1, variant=1, views=3, x0=5, y0=9, **small)
    assert pl["variant"] == "accumulate<0, 0, 0, 1, 0>" and pl["built"] == 1 and pl["view_count"] == 3 and pl["job_count"] == 3 * 3 * 2 * 64
    assert plan(variant=1, sample_map=1, **frame)["variant"] == "sample_map<0, 1, 1, 1, 0>"
    for bad in (["accumulate=1", "policy=chunk"], ["accumulate=1", "sample_map=1", "policy=pixel"], ["accumulate=1", "policy=pixel", "shard_count=2"]):
        assert subprocess.run([tool, "width=8", "height=8", "x1=8", "y1=8"] + bad, capture_output=True).returncode == 2


# ---- 4. the C ABI -------------------------------------------------------------------------------------------------------------------
def test_entry_points_have_c_linkage(api):
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NAMES <= names and NAMES <= set(api.EXPORTS)
    hdr = open(os.path.join(os.path.dirname(DATA), "include", "ort.h")).read()
    assert all(n + "(" in hdr for n in NAMES) and "} ort_accum_planes;" in hdr
    assert api.lib().ort_abi_version() == 3   # additive: the ABI version stands
    assert ctypes.sizeof(api.AccumPlanes) == 4 * ctypes.sizeof(ctypes.c_void_p)
    section = hdr[hdr.index("accumulating renders"):hdr.index("int ort_render_accumulate(")]
    for word in ("ORT_ERR_INVALID", "ORT_ERR_UNSUPPORTED", "ORT_ERR_STATE", "ORT_ERR_NO_DEVICE", "job_seed(seed, y*W + x)", "n0    = count[i]",
                 "min(asked, params->spp, (1 << 24) - min(n0, 1 << 24))", "0 TAKEN AS 1", "NOT read", "Five identities", "Split invariance",
                 "UNDIVIDED", "C / (float)(n0 + add)", "only when stats != NULL"):
        assert word in section, word
    assert "Not offered: resuming" not in hdr


def _caller(api, views_form, device_form):
    """call(handle, params, acc, map, rgb[, views, count]) through one of the four entry points"""
    L = api.lib()
    cam = api.View()

    def call(handle, p, acc, smap, rgb, views="own", count=1, stats=None):
        pp = ctypes.byref(p) if p is not None else None
        pa = ctypes.byref(acc) if acc is not None else None
        tail = (pa, smap, rgb) + ((None,) if device_form else ()) + (stats,)
        name = "ort_render_%saccumulate%s" % ("views_" if views_form else "", "_device" if device_form else "")
        if views_form:
            return getattr(L, name)(handle, pp, ctypes.addressof(cam) if isinstance(views, str) else views, count, *tail)
        return getattr(L, name)(handle, pp, *tail)
    return call, cam


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("views_form", [False, True])
@pytest.mark.parametrize("committed", [True, False])
def test_errors_come_in_order(api, views_form, device_form, committed):
    """ort_render_sample_map's order with acc where the map stands: INVALID (null views, the view cap, null scene or params, the
    params, the cap above 1 << 24, then a null acc or required plane, then the alignment of every given plane and of the map),
    UNSUPPORTED (policy, shard, packed, a camera outside the box), then the scene's state: STATE before NO_DEVICE.  On a
    committed-but-not-uploaded scene and on an uncommitted one, so every error comes before any device work"""
    s = _scene(api, committed)
    L = api.lib()
    call, view = _caller(api, views_form, device_form)
    cam = s.camera(8, 8)
    for k, name in enumerate(("p", "x_axis", "y_axis", "z_axis")):
        setattr(view.camera, name, api.V3(*[float(c) for c in cam[k]]))
    keep = [_aligned(8 * 8 * 12), _aligned(8 * 8 * 4), _aligned(8 * 8 * 4), _aligned(8 * 8 * 4), _aligned(8 * 8 * 4), _aligned(8 * 8 * 12)]
    d_sum, m2, count, states, smap, rgb = (k[1] for k in keep)
    acc = api.AccumPlanes(d_sum, m2, count, states)
    state = api.ERR_NO_DEVICE if committed else api.ERR_STATE
    if views_form:   # nulls first: before bad params and a null acc
        assert call(s.handle, _params(api, width=0), None, None, None, views=None) == api.ERR_INVALID
        assert b"views" in L.ort_last_error()
        assert call(s.handle, _params(api, width=0), None, None, None, count=api.MAX_VIEWS + 1) == api.ERR_INVALID
        assert b"ORT_MAX_VIEWS" in L.ort_last_error()
    assert call(None, _params(api), acc, smap, rgb) == api.ERR_INVALID
    assert call(s.handle, None, acc, smap, rgb) == api.ERR_INVALID
    # the params, as the render call judges them, before acc; chunk is ignored
    for p, word in ((_params(api, width=0), b"image size"), (_params(api, rect=(4, 4, 4, 8)), b"rect"), (_params(api, spp=0), b"spp"),
                    (_params(api, rr=-0.5), b"rr"), (_params(api, rr=float("nan")), b"rr"), (_params(api, policy=7), b"policy"),
                    (_params(api, shard=(3, 2)), b"shard index")):
        assert call(s.handle, p, None, smap, rgb) == api.ERR_INVALID, word
        assert word in L.ort_last_error(), (word, L.ort_last_error())
    assert call(s.handle, _params(api, spp=(1 << 24) + 1), None, smap, rgb) == api.ERR_INVALID
    assert b"1 << 24" in L.ort_last_error()
    # acc and its required planes, then the alignment, before what the call does not do
    chunky = _params(api, policy="chunk", spp=7, chunk=3, shard=(0, 2), packed=True)
    assert call(s.handle, chunky, None, smap, rgb) == api.ERR_INVALID
    assert b"null acc" in L.ort_last_error()
    for planes in ((None, m2, count, states), (d_sum, m2, None, states), (d_sum, m2, count, None)):
        assert call(s.handle, chunky, api.AccumPlanes(*planes), smap + 2, rgb) == api.ERR_INVALID   # a null plane before a misaligned map
        assert b"null" in L.ort_last_error() and b"plane" in L.ort_last_error()
    for planes, mp, out in (((d_sum + 2, m2, count, states), smap, rgb), ((d_sum, m2 + 1, count, states), smap, rgb), ((d_sum, m2, count + 3, states), smap, rgb),
                            ((d_sum, m2, count, states + 2), smap, rgb), ((d_sum, m2, count, states), smap + 2, rgb), ((d_sum, m2, count, states), smap, rgb + 1)):
        assert call(s.handle, chunky, api.AccumPlanes(*planes), mp, out) == api.ERR_INVALID
        assert b"4-byte aligned" in L.ort_last_error()
    # what the call does not do: any policy but PIXEL, shards, a packed framebuffer
    for policy in ("tile32", "whole", "chunk"):
        assert call(s.handle, _params(api, policy=policy, shard=(0, 2) if policy == "chunk" else (0, 1)), acc, smap, rgb) == api.ERR_UNSUPPORTED
        assert b"PIXEL" in L.ort_last_error()
    assert call(s.handle, _params(api, shard=(1, 2), packed=True), acc, smap, rgb) == api.ERR_UNSUPPORTED
    assert b"shard" in L.ort_last_error()
    assert call(s.handle, _params(api, packed=True), acc, smap, rgb) == api.ERR_UNSUPPORTED
    assert b"packed" in L.ort_last_error()
    if views_form:   # a camera outside the box, naming the view
        two = (api.View * 2)(view, view)
        two[1].camera.p = api.V3(1e6, 0.0, 0.0)
        assert call(s.handle, _params(api), acc, smap, rgb, views=ctypes.addressof(two), count=2) == api.ERR_UNSUPPORTED
        assert b"view 1" in L.ort_last_error()
    # all of these come before the scene's state; good arguments reach it: the optional planes and the map NULL, the limits
    assert call(s.handle, _params(api, spp=1 << 24, chunk=5, rr=7.5), api.AccumPlanes(d_sum, None, count, states), None, None) == state
    assert call(s.handle, _params(api, spp=1), acc, smap, rgb) == state
    assert (b"commit" if not committed else b"upload") in L.ort_last_error()


@pytest.mark.parametrize("device_form", [False, True])
def test_empty_batch_is_ok(api, device_form):
    """view_count == 0: ORT_OK without a launch, whatever the other arguments"""
    call, _ = _caller(api, True, device_form)
    for s in (_scene(api), _scene(api, committed=False)):
        assert call(s.handle, None, None, None, None, views=None, count=0) == api.OK
        assert call(s.handle, _params(api, width=0, policy="whole"), None, None, None, count=0) == api.OK
    st = api.Stats()
    st.rays = 7
    assert call(_scene(api).handle, None, None, None, None, views=None, count=0, stats=ctypes.byref(st)) == api.OK
    assert st.rays == 0


# ---- 5. the Python surface --------------------------------------------------------------------------------------------------------
def test_accumulator_and_python_shapes(api, tmp_path):
    s = _scene(api)
    acc = api.Accumulator(8, 6)
    assert acc.sum_rgb.shape == (6, 8, 3) and acc.m2.shape == acc.count.shape == acc.states.shape == (6, 8) and not acc.count.any()
    assert (acc.rgb(fill=-2.0) == -2.0).all()
    acc.count[1, 2], acc.sum_rgb[1, 2] = 3, (1.0, 2.0, 0.5)
    acc.states[4, 4], acc.m2[0, 7] = 0xDEADBEEF, 0.25
    want = (np.array([1.0, 2.0, 0.5], "<f4") / np.float32(3)).astype("<f4")
    assert (acc.rgb()[1, 2].view("<u4") == want.view("<u4")).all() and acc.rgb().dtype == np.dtype("<f4") and (acc.rgb()[0, 0] == 0).all()
    path = str(tmp_path / "frame.npz")
    acc.save(path)
    back = api.Accumulator.load(path)
    assert (back.width, back.height, back.views) == (8, 6, None)
    for name in ("sum_rgb", "m2", "count", "states"):
        a, b = getattr(acc, name), getattr(back, name)
        assert a.dtype == b.dtype and (a.view("<u4") == b.view("<u4")).all() and b.flags.c_contiguous
    batch = api.Accumulator(8, 6, views=2)
    batch.save(path)
    assert api.Accumulator.load(path).sum_rgb.shape == (2, 6, 8, 3)
    # the calls: shapes are judged here, everything else by the library
    for call in (lambda: s.render_accumulate(acc, 4, 3), lambda: s.render_accumulate(acc, np.full((6, 8), 3), 3, use_m2=False, out=np.zeros((6, 8, 3), "<f4"))):
        with pytest.raises(api.OrtError) as e:
            call()
        assert e.value.code == api.ERR_NO_DEVICE
    for bad in (lambda: s.render_accumulate(batch, 4, 3), lambda: s.render_accumulate(acc, np.zeros((8, 6)), 3),
                lambda: s.render_accumulate(acc, 4, 3, out=np.zeros((6, 8, 3), "<f8")), lambda: s.render_accumulate("acc", 4, 3)):
        with pytest.raises(ValueError):
            bad()
    cams = np.stack([s.camera(8, 6)] * 2)
    with pytest.raises(ValueError):
        s.render_views_accumulate(cams, [1, 2], acc, 4)
    with pytest.raises(api.OrtError) as e:
        s.render_views_accumulate(cams, [1, 2], batch, np.full((2, 6, 8), 2))
    assert e.value.code == api.ERR_NO_DEVICE
    assert s.render_views_accumulate(np.zeros((0, 4, 3), "<f4"), [], api.Accumulator(8, 6, views=0), 4)["paths"] == 0
    p = s.params(8, 6, 4, 1, "pixel")
    for call in (lambda: s.render_accumulate_device(p, 64, 128, 256), lambda: s.render_views_accumulate_device(p, cams, [1, 2], 64, 128, 256, d_m2=512)):
        with pytest.raises(api.OrtError) as e:
            call()
        assert e.value.code == api.ERR_NO_DEVICE
    acc.count = acc.count.astype("<i8")
    with pytest.raises(ValueError):
        s.render_accumulate(acc, 4, 3)
