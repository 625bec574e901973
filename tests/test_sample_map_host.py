"""Sample-map renders (ort_render_sample_map, ort_render_views_sample_map and their device forms), host side: the mixed map and
the reference shown not to be vacuous from the oracle alone, the lane code with the map run on host threads (tools/host_sim
--sample-map) against the oracle's planes bit for bit, the launch plan, and the C ABI surface with its errors in the order
include/ort.h gives them."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import host_sim_tool as hs
import light_groups_cases as lg
import sample_map_cases as sm
from conftest import DATA, ROOT
from host_cases import aligned as _aligned, params as _params, scene as _scene

NAMES = {"ort_render_sample_map", "ort_render_sample_map_device", "ort_render_views_sample_map", "ort_render_views_sample_map_device"}


@pytest.fixture()
def case(api, oracle, tmp_path_factory):
    return lambda name: lg.case(api, oracle, name, tmp_path_factory)


@pytest.fixture(scope="module")
def host_sim():
    return hs.built("host_sim")


# ---- 1. the map and the reference, from the oracle alone ------------------------------------------------------------------------
def test_the_mixed_map_is_what_the_tests_need():
    """every value, neighbours that differ, a whole block of zeros, a row of zeros, zeros and samples on the rect's border"""
    assert (sm.W, sm.H, sm.CAP, sm.SEED, sm.RR, sm.RECT) == (24, 16, 16, 2024, 0.8, (3, 2, 21, 13))
    base = sm.base_map()
    assert set(base.reshape(-1).tolist()) == set(sm.VALUES) == {0, 1, 2, 3, 5, 16, 17, 0xFFFFFFFF}
    assert (base[:, 1:] != base[:, :-1]).all() and (base[1:, :] != base[:-1, :]).all()
    m = sm.mixed_map()
    inside = sm.inside(sm.RECT)
    for region in (np.ones((sm.H, sm.W), bool), inside):
        assert set(m[region].tolist()) == set(sm.VALUES)            # every value survives the zeros, in the rect too
    bx, by = sm.ZERO_BLOCK
    assert bx % 8 == 0 and by % 8 == 0 and (m[by:by + 8, bx:bx + 8] == 0).all() and inside[by:by + 8, bx:bx + 8].any()
    assert (m[sm.ZERO_ROW] == 0).all() and inside[sm.ZERO_ROW].any()
    ring = sm.border(sm.RECT)
    assert (m[ring] == 0).any() and (m[ring] != 0).any()
    assert sm.counts(m).max() == sm.CAP and (sm.counts(m)[m >= 16] == 16).all()
    assert (sm.mixed_map(3) != m).any()


@pytest.mark.parametrize("name", sm.SCENES)
def test_every_class_of_the_map_shows_light(case, name):
    """the condition on the reference alone: for every distinct n >= 1 in the map (every map value, so the clamped ones on their
    own too), whole frame and rect, at least one pixel of that class has a non-zero colour and at least one a non-zero Q"""
    c = case(name)
    m = sm.mixed_map()
    for rect in (None, sm.RECT):
        rgb, m2, fin = sm.expected(c, m, rect=rect)
        live = sm.inside(rect) & (m != 0)
        assert (fin[live] != sm.GUARD_STATE).all() and (fin[~live] == sm.GUARD_STATE).all()
        for v in sorted(set(m[live].tolist())):
            at = live & (m == v)
            lit = int((rgb[at] != 0).any(axis=1).sum())
            print("%s rect %r: map value %d (n = %d): %d pixels, %d lit, %d with Q != 0" % (name, rect, v, min(v, sm.CAP), int(at.sum()), lit, int((m2[at] != 0).sum())))
            assert lit >= 1 and (m2[at] != 0).any(), (name, rect, v)


def test_a_constant_map_is_the_pixel_render(case):
    """the reference against the oracle's own PIXEL render: constant maps 1 and 16, and 0xffffffff under the cap"""
    c = case("room_all_lobes")
    for v, n in ((1, 1), (16, 16), (0xFFFFFFFF, 16)):
        rgb, _, fin = sm.expected(c, np.full((sm.H, sm.W), v, "<u4"), rect=sm.RECT)
        m = sm.inside(sm.RECT)
        assert (rgb[m].view("<u4") == c.frame(None, n, rect=sm.RECT)[m].view("<u4")).all()
        assert (fin[m] == c.states(n, rect=sm.RECT)[m]).all()


# ---- 2. the lane code on host threads ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sm.SCENES)
def test_host_sim_is_the_oracle(host_sim, case, tmp_path, name):
    """the mixed map with and without the rect: every plane bit for bit, the guards intact where n == 0 and outside the rect; the
    tables in LDS form and from their arrays, both BSDF flavours where the scene allows, one thread and eight; the counters'
    paths are the samples asked for"""
    c = case(name)
    m = sm.mixed_map()
    envs = [{}, {"SIM_TABS": "1"}] if name != lg.TABLE_SCENE else [{}]
    if name == "room_diffuse":
        envs = [{"SIM_DIFFUSE": "1"}, {"SIM_DIFFUSE": "1", "SIM_TABS": "1"}, {}]
    for rect in (sm.RECT, None):
        want = sm.expected(c, m, rect=rect)
        for k, env in enumerate(envs):
            for threads in ((8, 1) if k == 0 and rect else (8,)):
                got, r = sm.host_sample_map(host_sim, tmp_path, c, m, rect=rect, env=env, threads=threads)
                sm.assert_planes(tuple(g[0] for g in got), want, "%s rect %r %r, %d threads" % (name, rect, env, threads))
                assert hs.counters(r)["paths"] == int(sm.counts(m)[sm.inside(rect)].sum())


def test_host_sim_optional_planes_and_maps(host_sim, case, tmp_path):
    """dropping out_m2, final_states or both moves no bit of the rest; an all-zero map writes nothing; a map at or above the cap
    is the constant map"""
    c = case("room_diffuse")
    m = sm.mixed_map()
    want = sm.expected(c, m, rect=sm.RECT)
    for want_m2, want_states in ((False, True), (True, False), (False, False)):
        got, _ = sm.host_sample_map(host_sim, tmp_path, c, m, rect=sm.RECT, want_m2=want_m2, want_states=want_states, threads=8)
        sm.assert_planes(tuple(g[0] if g is not None else None for g in got), want, "m2 %d states %d" % (want_m2, want_states))
    zero = np.zeros((sm.H, sm.W), "<u4")
    got, r = sm.host_sample_map(host_sim, tmp_path, c, zero, threads=8)
    sm.assert_planes(tuple(g[0] for g in got), sm.expected(c, zero), "all-zero map")
    assert hs.counters(r)["paths"] == 0 and hs.counters(r)["rays"] == 0
    above = np.where(sm.base_map() % 2 == 0, 5, 0xFFFFFFFF).astype("<u4")
    got, _ = sm.host_sample_map(host_sim, tmp_path, c, above, cap=5, rect=sm.RECT, threads=8)
    sm.assert_planes(tuple(g[0] for g in got), sm.expected(c, np.full((sm.H, sm.W), 5, "<u4"), cap=5, rect=sm.RECT), "a map at or above the cap")


@pytest.mark.parametrize("name", ["room_all_lobes"])
def test_host_sim_batch_of_views(host_sim, api, case, tmp_path, name):
    """two views, another camera, seed and map each: frame v is the single frame's for that camera, seed and map frame"""
    c = case(name)
    cams, seeds = sm.batch_cameras(api, c)[:2], sm.BATCH_SEEDS[:2]
    maps = np.stack([sm.mixed_map(), sm.mixed_map(3)])
    assert (cams[0] != cams[1]).any() and seeds[0] != seeds[1] and (maps[0] != maps[1]).any()
    got, r = sm.host_sample_map(host_sim, tmp_path, c, maps, rect=sm.RECT, cams=cams, seeds=seeds, threads=8)
    for v in range(2):
        sm.assert_planes(tuple(g[v] for g in got), sm.expected(c, maps[v], seed=seeds[v], cam=cams[v], rect=sm.RECT), "%s: view %d" % (name, v))
    assert hs.counters(r)["paths"] == int(sm.counts(maps)[:, sm.inside(sm.RECT)].sum())
    one, _ = sm.host_sample_map(host_sim, tmp_path, c, maps[1:2], cams=cams[1:2], seeds=seeds[1:2], threads=8)
    sm.assert_planes(tuple(g[0] for g in one), sm.expected(c, maps[1], seed=seeds[1], cam=cams[1]), name + ": batch of one")


def test_host_sim_under_sanitizers(case, tmp_path):
    """tools/host_sim_san (the stand-alone ASan + UBSan binary, run directly): ends clean, with the oracle's planes; the map and
    the planes are exactly as long as the frames, so a read or write past a plane's end is one past the block"""
    san = hs.built("host_sim_san")
    c = case("room_all_lobes")
    m = sm.mixed_map()
    env = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}
    for extra, rect in (({}, sm.RECT), ({"SIM_TABS": "1"}, None)):
        got, _ = sm.host_sample_map(san, tmp_path, c, m, rect=rect, env=dict(env, **extra), threads=2)
        sm.assert_planes(tuple(g[0] for g in got), sm.expected(c, m, rect=rect), "sanitized %r" % (extra,))
    got, _ = sm.host_sample_map(san, tmp_path, c, m, rect=sm.RECT, want_m2=False, want_states=False, env=env, threads=2)
    sm.assert_planes((got[0][0], None, None), sm.expected(c, m, rect=sm.RECT), "sanitized, the colours alone")


# ---- 3. the launch plan -----------------------------------------------------------------------------------------------------------
def test_launch_plan_names_the_sample_map_kernels():
    """plan_pixel_jobs, RK_SAMPLE_MAP: the adaptive render's launch in every other field, whatever the knobs say; its variant is
    sample_map<...> and is built; the fill of the call: spp is the cap, the job space every pixel under the rect"""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "launch_plan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    tool = os.path.join(ROOT, "tools", "launch_plan")

    def run(env=None, **kw):
        e = {k: v for k, v in os.environ.items() if not k.startswith("ORT_")}
        e.update(env or {})
        return subprocess.check_output([tool] + ["%s=%s" % kv for kv in kw.items()], env=e, text=True).splitlines()

    def plan(env=None, **kw):
        return json.loads(run(env, **kw)[0])
    frame = dict(policy="pixel", width=1920, height=1080, x1=1920, y1=1080, materials=8, lights=2, diffuse_only=1, sah_cost=0.5, spp=16)
    forced = {"ORT_EXCHANGE": "1", "ORT_WAVES5": "1", "ORT_WIDE": "1", "ORT_MODE": "wavefront", "ORT_DEBUG_UTIL": "1"}
    for env in ({}, forced):
        for counters in (0, 1):
            pl = plan(env, sample_map=1, variant=1, counters=counters, has_wide=1, **frame)
            assert pl["sample_map"] == 1 and pl["views"] == 1 and pl["view_count"] == 1 and pl["implicit"] == 1 and pl["mode"] == 1
            assert not (pl["exchange"] or pl["five"] or pl["wide"] or pl["wavefront"] or pl["util"])
            assert pl["variant"] == "sample_map<%d, 1, 1, 1, 0>" % counters and pl["built"] == 1
            assert pl["job_count"] == pl["view_jobs"] == 240 * 135 * 64 and pl["grid"] == pl["max_blocks"] == 1024
            assert pl["partial_bytes"] == pl["stash_bytes"] == pl["drain_bytes"] == 0
            same = plan(env, adaptive=1, counters=counters, has_wide=1, **frame)
            assert {k: v for k, v in pl.items() if k not in ("sample_map", "variant", "built")} == {k: v for k, v in same.items() if k != "adaptive"}
    small = {**frame, "x1": 20, "y1": 17, "width": 27, "height": 19}
    pl = plan({"ORT_KERNEL": "general", "ORT_LDS_TABLES": "0"}, sample_map=1, variant=1, views=3, x0=5, y0=9, **small)
    assert pl["variant"] == "sample_map<0, 0, 0, 1, 0>" and pl["built"] == 1 and pl["view_count"] == 3
    assert pl["view_jobs"] == 3 * 2 * 64 and pl["job_count"] == 3 * pl["view_jobs"] and pl["grid"] == 5
    assert plan(sample_map=1, variant=1, **{**frame, "materials": 60})["variant"] == "sample_map<0, 1, 0, 1, 0>"
    # the fill of the call
    lines = run(sample_map=1, fill=1, views=3, x0=5, y0=9, rr=0.75, view_seed=40, **small)[1:]
    fill = dict(l.split(" = ") for l in lines)
    assert (fill["mode"], fill["spp"], fill["view_count"], fill["W"], fill["H"]) == ("1", "16", "3", "27", "19")
    assert (fill["x0"], fill["y0"], fill["x1"], fill["y1"]) == ("5", "9", "20", "17") and float(fill["rr"]) == 0.75
    assert int(fill["job_count"]) == 3 * int(fill["view_jobs"]) == 3 * 3 * 2 * 64 and fill["nchunks"] == "1" and fill["packed_out"] == "0"
    # the other calls' plans name what they named
    assert plan(variant=1, adaptive=1, **frame)["variant"] == "adaptive<0, 1, 1, 1, 0>"
    assert plan(variant=1, groups=1, **frame)["variant"] == "groups<0, 1, 1, 1, 0>"
    assert plan(variant=1, views=3, **frame)["variant"] == "loop_views<0, 1, 1, 1, 0>"
    for bad in (["sample_map=1", "policy=chunk"], ["sample_map=1", "adaptive=1", "policy=pixel"], ["sample_map=1", "groups=1", "policy=pixel"],
                ["sample_map=1", "policy=pixel", "shard_count=2"]):
        assert subprocess.run([tool, "width=8", "height=8", "x1=8", "y1=8"] + bad, capture_output=True).returncode == 2
    sweep = json.loads(subprocess.check_output([tool, "sweep=1"], env={k: v for k, v in os.environ.items() if not k.startswith("ORT_")}))
    assert sweep["plans"] > 0 and (sweep["unbuilt"], sweep["first"]) == (0, [])


# ---- 4. the C ABI -----------------------------------------------------------------------------------------------------------------
def test_entry_points_have_c_linkage(api):
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NAMES <= names
    assert NAMES <= set(api.EXPORTS)
    hdr = open(os.path.join(os.path.dirname(DATA), "include", "ort.h")).read()
    assert all(n + "(" in hdr for n in NAMES)
    assert api.lib().ort_abi_version() == 3   # additive: the ABI version stands
    section = hdr[hdr.index("sample-map renders"):hdr.index("int ort_render_sample_map(")]
    for word in ("ORT_ERR_INVALID", "ORT_ERR_UNSUPPORTED", "ORT_ERR_STATE", "ORT_ERR_NO_DEVICE", "job_seed(seed, y*W + x)",
                 "min(sample_map[i], params->spp)", "0xffffffff", "stay untouched", "Four identities", "out_spp", "DEVICE pointer"):
        assert word in section, word
    order = [section.rindex(k) for k in ("ORT_ERR_INVALID (", "ORT_ERR_UNSUPPORTED (policy", "ORT_ERR_STATE (", "ORT_ERR_NO_DEVICE")]
    assert order == sorted(order)


def _caller(api, views_form, device_form):
    """call(handle, params, map, rgb, m2, states[, views, count]) through one of the four entry points"""
    L = api.lib()
    cam = api.View()

    def call(handle, p, smap, rgb, m2, states, views="own", count=1, stats=None):
        pp = ctypes.byref(p) if p is not None else None
        if views_form:
            v = ctypes.addressof(cam) if isinstance(views, str) else views
            if device_form:
                return L.ort_render_views_sample_map_device(handle, pp, v, count, smap, rgb, m2, states, None, stats)
            return L.ort_render_views_sample_map(handle, pp, v, count, smap, rgb, m2, states, stats)
        if device_form:
            return L.ort_render_sample_map_device(handle, pp, smap, rgb, m2, states, None, stats)
        return L.ort_render_sample_map(handle, pp, smap, rgb, m2, states, stats)
    return call, cam


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("views_form", [False, True])
@pytest.mark.parametrize("committed", [True, False])
def test_errors_come_in_order(api, views_form, device_form, committed):
    """INVALID (nulls, the view cap, the params, the cap above 1 << 24, then the null map and the alignment of the map and the
    planes), UNSUPPORTED (policy, shard, packed, a camera outside the box), then the scene's state: STATE before NO_DEVICE.  On
    a committed-but-not-uploaded scene and on an uncommitted one, so every error comes before any device work.  The map's
    values are never judged: a map of 0xffffffff reaches the scene's state like any other"""
    s = _scene(api, committed)
    L = api.lib()
    call, view = _caller(api, views_form, device_form)
    cam = s.camera(8, 8)
    for k, name in enumerate(("p", "x_axis", "y_axis", "z_axis")):
        setattr(view.camera, name, api.V3(*[float(c) for c in cam[k]]))
    keep = [_aligned(8 * 8 * 4), _aligned(8 * 8 * 12), _aligned(8 * 8 * 4), _aligned(8 * 8 * 4)]
    smap, rgb, m2, fin = (k[1] for k in keep)
    keep[0][0][:] = 0xFF   # every word of the map 0xffffffff
    state = api.ERR_NO_DEVICE if committed else api.ERR_STATE
    nan = float("nan")
    # nulls first: before bad params and a null map
    assert call(s.handle, _params(api, width=0), None, None, m2, fin) == api.ERR_INVALID
    assert b"framebuffer" in L.ort_last_error()
    if views_form:
        assert call(s.handle, _params(api, width=0), None, rgb, m2, fin, views=None) == api.ERR_INVALID
        assert b"views" in L.ort_last_error()
        assert call(s.handle, _params(api, width=0), None, rgb, m2, fin, count=api.MAX_VIEWS + 1) == api.ERR_INVALID
        assert b"ORT_MAX_VIEWS" in L.ort_last_error()
    assert call(None, _params(api), smap, rgb, m2, fin) == api.ERR_INVALID
    assert call(s.handle, None, smap, rgb, m2, fin) == api.ERR_INVALID
    # the params, as the render call judges them, before the map; chunk is ignored
    for p, word in ((_params(api, width=0), b"image size"), (_params(api, rect=(4, 4, 4, 8)), b"rect"), (_params(api, rect=(0, 0, 9, 8)), b"rect"),
                    (_params(api, spp=0), b"spp"), (_params(api, rr=-0.5), b"rr"), (_params(api, rr=nan), b"rr"), (_params(api, policy=7), b"policy"),
                    (_params(api, shard=(3, 2)), b"shard index")):
        assert call(s.handle, p, None, rgb, m2, fin) == api.ERR_INVALID, word
        assert word in L.ort_last_error(), (word, L.ort_last_error())
    assert call(s.handle, _params(api, width=70000, height=1), None, rgb, m2, fin) == api.ERR_UNSUPPORTED   # as the render call: 16-bit coordinates
    assert call(s.handle, _params(api, spp=(1 << 24) + 1), None, rgb, m2, fin) == api.ERR_INVALID
    assert b"1 << 24" in L.ort_last_error()
    # the map and the alignment, before what the call does not do
    chunky = _params(api, policy="chunk", spp=7, chunk=3, shard=(0, 2), packed=True)
    assert call(s.handle, chunky, None, rgb, m2, fin) == api.ERR_INVALID
    assert b"null" in L.ort_last_error() and b"sample_map" in L.ort_last_error()
    for args in ((smap + 2, rgb, m2, fin), (smap, rgb + 1, m2, fin), (smap, rgb, m2 + 2, fin), (smap, rgb, m2, fin + 3)):
        assert call(s.handle, chunky, *args) == api.ERR_INVALID
        assert b"4-byte aligned" in L.ort_last_error()
    # what the call does not do: any policy but PIXEL, shards, a packed framebuffer
    for policy in ("tile32", "whole", "chunk"):
        assert call(s.handle, _params(api, policy=policy, shard=(0, 2) if policy == "chunk" else (0, 1)), smap, rgb, m2, fin) == api.ERR_UNSUPPORTED
        assert b"PIXEL" in L.ort_last_error()
    assert call(s.handle, _params(api, shard=(1, 2), packed=True), smap, rgb, m2, fin) == api.ERR_UNSUPPORTED
    assert b"shard" in L.ort_last_error()
    assert call(s.handle, _params(api, packed=True), smap, rgb, m2, fin) == api.ERR_UNSUPPORTED
    assert b"packed" in L.ort_last_error()
    if views_form:   # a camera outside the box, naming the view
        two = (api.View * 2)(view, view)
        two[1].camera.p = api.V3(1e6, 0.0, 0.0)
        assert call(s.handle, _params(api), smap, rgb, m2, fin, views=ctypes.addressof(two), count=2) == api.ERR_UNSUPPORTED
        assert b"view 1" in L.ort_last_error()
    # all of these come before the scene's state; good arguments reach it: the optional planes NULL, the limits, any map value
    assert call(s.handle, _params(api, spp=1 << 24, chunk=5, rr=7.5), smap, rgb, None, None) == state
    assert call(s.handle, _params(api, spp=1), smap, rgb, m2, fin) == state
    assert (b"commit" if not committed else b"upload") in L.ort_last_error()


@pytest.mark.parametrize("device_form", [False, True])
def test_empty_batch_is_ok(api, device_form):
    """view_count == 0: ORT_OK without a launch, whatever the other arguments"""
    call, _ = _caller(api, True, device_form)
    for s in (_scene(api), _scene(api, committed=False)):
        assert call(s.handle, None, None, None, None, None, views=None, count=0) == api.OK
        assert call(s.handle, _params(api, width=0, policy="whole"), None, None, None, None, count=0) == api.OK
    st = api.Stats()
    st.rays = 7
    assert call(_scene(api).handle, None, None, None, None, None, views=None, count=0, stats=ctypes.byref(st)) == api.OK
    assert st.rays == 0


def test_python_shapes(api):
    s = _scene(api)
    m = np.full((6, 8), 3, "<u4")
    with pytest.raises(api.OrtError) as e:
        s.render_sample_map(8, 6, m, 4, 3, want_states=True)
    assert e.value.code == api.ERR_NO_DEVICE
    with pytest.raises(api.OrtError) as e:
        s.render_sample_map(8, 6, m.astype("<i8"), 4, 3)   # any integers
    assert e.value.code == api.ERR_NO_DEVICE
    assert s._sample_map(np.array([[-1, 1 << 32]]), (1, 2)).tolist() == [[0xFFFFFFFF, 0]]
    for bad in (np.zeros((8, 6), "<u4"), np.zeros(48, "<u4"), np.zeros((1, 6, 8), "<u4")):
        with pytest.raises(ValueError):
            s.render_sample_map(8, 6, bad, 4, 3)
    planes = [np.zeros((6, 8, 3), "<f4"), np.zeros((6, 8), "<f4"), np.zeros((6, 8), "<u4")]
    for bad in (planes[:2], [planes[0], planes[1], planes[2].astype("<i8")], [planes[0][:, ::2], planes[1], planes[2]]):
        with pytest.raises(ValueError):
            s.render_sample_map(8, 6, m, 4, 3, want_states=True, out=bad)
    cams = np.stack([s.camera(8, 6)] * 2)
    with pytest.raises(ValueError):
        s.render_views_sample_map(cams, [1, 2], 8, 6, m, 4)   # one frame's map for two views
    with pytest.raises(ValueError):
        s.render_views_sample_map(cams, [1], 8, 6, np.stack([m, m]), 4)
    with pytest.raises(api.OrtError) as e:
        s.render_views_sample_map(cams, [1, 2], 8, 6, np.stack([m, m]), 4)
    assert e.value.code == api.ERR_NO_DEVICE
    rgb, m2, states, st = s.render_views_sample_map(np.zeros((0, 4, 3), "<f4"), [], 8, 6, np.zeros((0, 6, 8), "<u4"), 4, want_states=True)
    assert rgb.shape == (0, 6, 8, 3) and m2.shape == (0, 6, 8) and states.shape == (0, 6, 8) and st["paths"] == 0
    p = s.params(8, 6, 4, 1, "pixel")
    for call in (lambda: s.render_sample_map_device(p, 64, 128), lambda: s.render_views_sample_map_device(p, cams, [1, 2], 64, 128)):
        with pytest.raises(api.OrtError) as e:
            call()
        assert e.value.code == api.ERR_NO_DEVICE
