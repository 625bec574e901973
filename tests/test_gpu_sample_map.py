"""Sample-map renders on the device (ort_render_sample_map, ort_render_views_sample_map and their device forms; kernels
pt_sample_map): colours, sums of squared sample luminance and final stream states, bit for bit the oracle's chains cut at the
map's counts (tests/sample_map_cases.py), on guard-filled planes.  Frames are 24 x 16, the cap 16; one uploaded scene per case."""
import numpy as np
import pytest

import light_groups_cases as lg
import sample_map_cases as sm

pytestmark = pytest.mark.gpu

W, H, CAP = sm.W, sm.H, sm.CAP


@pytest.fixture()
def case(api, oracle, tmp_path_factory):
    def get(name):
        c = lg.case(api, oracle, name, tmp_path_factory)
        if c.scene.device is None:
            assert api.device_count() >= 1, "GPU test on a machine without a HIP device (the render path has no CPU fallback)"
            c.scene.upload(0)
        return c
    return get


def run(c, smap, cap=CAP, rect=None, seed=sm.SEED, want_m2=True, want_states=True, **kw):
    """the single-frame host form on guard-filled planes -> (rgb, m2 or None, states or None), stats"""
    out = c.scene.render_sample_map(W, H, smap, cap, seed, want_m2, want_states, rect=rect, rr=sm.RR, out=sm.guards(None, want_m2, want_states), **kw)
    return (out[0], out[1] if want_m2 else None, out[-2] if want_states else None), out[-1]


def bits(a):
    return np.ascontiguousarray(a).view("<u4")


# ---- 1. against the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sm.SCENES)
def test_the_mixed_map_is_the_oracle(case, name):
    """both BSDF flavours, tables in LDS and past its caps: the mixed map with the rect and over the whole frame, every plane bit
    for bit, every guard intact where n == 0 and outside the rect"""
    c = case(name)
    m = sm.mixed_map()
    for rect in (sm.RECT, None):
        got, st = run(c, m, rect=rect)
        sm.assert_planes(got, sm.expected(c, m, rect=rect), "%s rect %r" % (name, rect))
        assert st["kernel_ms"] > 0 and st["paths"] == 0   # counters only on request


# ---- 2. identity 1: a constant map is the PIXEL render and the adaptive render that never checks ------------------------------------
@pytest.mark.parametrize("name", ["room_all_lobes", "c4_dwarf_room"])
def test_constant_maps_are_the_other_renders(case, name):
    """constant maps 1, 2, 5 and 16 and a map of 0xffffffff (cap 16): out_rgb is scene.render(..., "pixel") at spp = n; all three
    planes are render_adaptive's at min_spp == max_spp == n.  (That call refuses min_spp < 2 -- a variance needs two samples --
    so n = 1 is held against the PIXEL render alone, and n = 2 stands beside it for the adaptive render.)"""
    c = case(name)
    for v, n in ((1, 1), (2, 2), (5, 5), (16, 16), (0xFFFFFFFF, 16)):
        got, _ = run(c, np.full((H, W), v, "<u4"), rect=sm.RECT)
        img, _ = c.scene.render(W, H, n, sm.SEED, "pixel", rect=sm.RECT, rr=sm.RR, out=np.full((H, W, 3), sm.GUARD_RGB, "<f4"))
        assert (bits(got[0]) == bits(img)).all(), (name, v, "PIXEL render")
        if n >= 2:
            rgb, spp, m2, states, _ = c.scene.render_adaptive(W, H, n, n, 0.3, seed=sm.SEED, rect=sm.RECT, rr=sm.RR, want_states=True,
                                                              out=[np.full((H, W, 3), sm.GUARD_RGB, "<f4"), np.zeros((H, W), "<u4"),
                                                                   np.full((H, W), sm.GUARD_M2, "<f4"), np.full((H, W), sm.GUARD_STATE, "<u4")])
            assert (spp[sm.inside(sm.RECT)] == n).all()
            sm.assert_planes(got, (rgb, m2, states), "%s: constant map %d against render_adaptive" % (name, v))
    # any map at or above a cap n is the constant map n
    above = np.where(sm.base_map() % 2 == 0, 5, 0xFFFFFFFF).astype("<u4")
    got, _ = run(c, above, cap=5)
    want, _ = run(c, np.full((H, W), 5, "<u4"), cap=5)
    sm.assert_planes(got, want, name + ": a map at or above the cap")


# ---- 3. identity 3: the adaptive render's sample counts fed back -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["room_diffuse", "room_all_lobes"])
def test_the_adaptive_renders_counts_fed_back(case, name):
    """render_adaptive(min 4, every 4, max 16, tolerance 0.3, floor 0.05)'s out_spp as the map, the same seed, cap 16 and cap 64:
    that call's out_rgb, out_m2 and final_states"""
    c = case(name)
    for rect in (sm.RECT, None):
        rgb, spp, m2, states, _ = c.scene.render_adaptive(W, H, 4, 16, 0.3, 0.05, 4, seed=sm.SEED, rect=rect, rr=sm.RR, want_states=True,
                                                          out=[np.full((H, W, 3), sm.GUARD_RGB, "<f4"), np.zeros((H, W), "<u4"),
                                                               np.full((H, W), sm.GUARD_M2, "<f4"), np.full((H, W), sm.GUARD_STATE, "<u4")])
        inside = sm.inside(rect)
        assert len(set(spp[inside].tolist())) >= 2 and (spp[~inside] == 0).all()   # the rule cut some pixels and not others
        for cap in (16, 64):
            got, _ = run(c, spp, cap=cap, rect=rect)
            sm.assert_planes(got, (rgb, m2, states), "%s rect %r cap %d" % (name, rect, cap))


# ---- 4. identity 2 and the optional planes -------------------------------------------------------------------------------------------
def test_a_pixel_depends_on_its_own_count_alone(case):
    """the map changed everywhere but at a probe set: the probe pixels do not move; out_m2, final_states or both dropped: the
    kept planes do not move"""
    c = case("room_all_lobes")
    m = sm.mixed_map()
    full, _ = run(c, m, rect=sm.RECT)
    y, x = np.mgrid[0:H, 0:W]
    probe = ((x * 7 + y * 5) % 11 == 0) & (m != 0) & sm.inside(sm.RECT)
    assert probe.sum() >= 8
    other = np.where(probe, m, sm.mixed_map(5)[::-1, ::-1]).astype("<u4")
    assert (other[~probe] != m[~probe]).mean() > 0.5
    got, _ = run(c, other, rect=sm.RECT)
    for g, f in zip(got, full):
        assert (bits(g)[probe] == bits(f)[probe]).all()
    sm.assert_planes(got, sm.expected(c, other, rect=sm.RECT), "the other map")
    for want_m2, want_states in ((False, True), (True, False), (False, False)):
        got, _ = run(c, m, rect=sm.RECT, want_m2=want_m2, want_states=want_states)
        sm.assert_planes(got, full, "m2 %d states %d" % (want_m2, want_states))


# ---- 5. and 6. the all-zero map and the counters ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["room_diffuse", lg.TABLE_SCENE])
def test_zero_map_and_counters(case, name):
    """an all-zero map: ORT_OK, every guard intact, paths == 0 under counters; the mixed map: paths == the sum of min(map, cap)
    over the rect, and the planes are the planes without counters"""
    c = case(name)
    zero = np.zeros((H, W), "<u4")
    for counters in (False, True):
        got, st = run(c, zero, counters=counters)
        sm.assert_planes(got, sm.guards(), "all-zero map")
        assert st["paths"] == 0 and st["rays"] == 0
    m = sm.mixed_map()
    for rect, cap in ((sm.RECT, CAP), (None, CAP), (sm.RECT, 3)):
        got, st = run(c, m, cap=cap, rect=rect, counters=True)
        assert st["paths"] == int(sm.counts(m, cap)[sm.inside(rect)].sum()) and st["rays"] >= st["paths"]
        sm.assert_planes(got, sm.expected(c, m, cap=cap, rect=rect), "%s with counters, rect %r cap %d" % (name, rect, cap))


# ---- 7. a batch of views --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["room_diffuse", "room_all_lobes"])
def test_views_are_the_single_frames(api, case, name):
    """three views, each with its own map: frame v is the single-frame call's for that camera, seed and map frame -- and the
    oracle's"""
    c = case(name)
    cams, seeds = sm.batch_cameras(api, c), sm.BATCH_SEEDS
    maps = np.stack([sm.mixed_map(), sm.mixed_map(3), sm.mixed_map(6)[::-1].copy()])
    out = c.scene.render_views_sample_map(cams, seeds, W, H, maps, CAP, True, True, rect=sm.RECT, rr=sm.RR, counters=True, out=sm.guards(3))
    assert out[3]["paths"] == int(sm.counts(maps)[:, sm.inside(sm.RECT)].sum())
    for v in range(3):
        sm.assert_planes(tuple(p[v] for p in out[:3]), sm.expected(c, maps[v], seed=seeds[v], cam=cams[v], rect=sm.RECT), "%s: view %d" % (name, v))
    # the single-frame call is the one-view batch of the scene's own camera
    single, _ = run(c, maps[0], rect=sm.RECT, seed=seeds[0])
    sm.assert_planes(single, tuple(p[0] for p in out[:3]), name + ": view 0 against the single-frame call")
    assert (bits(out[0][0]) != bits(out[0][2])).any()


# ---- 8. the device forms, on torch tensors on a stream of their own ----------------------------------------------------------------
def torch_run(c, smap, cap=CAP, rect=None, cams=None, seeds=None, want_m2=True, want_states=True, want_stats=False, counters=False, pad=16):
    """-> (rgb, m2 or None, states or None) as numpy, stats; the map is a device tensor; every tensor has `pad` guard words at
    both ends, which are checked here, and guard values throughout"""
    import torch
    dev = torch.device("cuda", 0)
    V = 1 if cams is None else len(cams)
    n = V * H * W
    fills = (float(sm.GUARD_RGB), float(sm.GUARD_M2), sm.GUARD_STATE - (1 << 32))
    t = [torch.full((k + 2 * pad,), f, dtype=dt, device=dev) for k, f, dt in zip((3 * n, n, n), fills, (torch.float32, torch.float32, torch.int32))]
    ptr = [x.data_ptr() + 4 * pad for x in t]
    p = c.scene.params(W, H, cap, sm.SEED, "pixel", 0, rect, sm.RR, counters)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        d_map = torch.from_numpy(np.ascontiguousarray(smap, "<u4").view("<i4").reshape(-1)).to(dev, non_blocking=False)   # the same words
        assert d_map.is_cuda and d_map.numel() == n
        args = (d_map.data_ptr(), ptr[0], ptr[1] if want_m2 else 0, ptr[2] if want_states else 0)
        if cams is None:
            st = c.scene.render_sample_map_device(p, *args, stream=stream.cuda_stream, want_stats=want_stats)
        else:
            st = c.scene.render_views_sample_map_device(p, cams, seeds, *args, stream=stream.cuda_stream, want_stats=want_stats)
    stream.synchronize()
    assert (d_map.cpu().numpy().view("<u4") == np.ascontiguousarray(smap, "<u4").reshape(-1)).all(), "the map was written"
    h = [x.cpu().numpy() for x in t]
    for x, f in zip(h, (sm.GUARD_RGB, sm.GUARD_M2, sm.GUARD_STATE)):
        g = np.array(f, x.dtype if x.dtype.kind == "f" else "<u4").reshape(1).view("<u4")[0]
        assert (x[:pad].view("<u4") == g).all() and (x[-pad:].view("<u4") == g).all(), "a guard word around a plane was written"
    lead = () if cams is None else (V,)
    rgb = h[0][pad:-pad].reshape(lead + (H, W, 3))
    m2 = h[1][pad:-pad].reshape(lead + (H, W))
    states = h[2][pad:-pad].view("<u4").reshape(lead + (H, W))
    if not want_m2:
        assert (m2 == sm.GUARD_M2).all()
    if not want_states:
        assert (states == sm.GUARD_STATE).all()
    return (rgb, m2 if want_m2 else None, states if want_states else None), st


@pytest.mark.parametrize("name", ["room_all_lobes", lg.TABLE_SCENE])
def test_device_form_on_a_stream(case, name):
    c = case(name)
    m = sm.mixed_map()
    got, st = torch_run(c, m, rect=sm.RECT)          # stats == NULL: enqueued, then synchronised
    assert st is None
    sm.assert_planes(got, sm.expected(c, m, rect=sm.RECT), name + ": device form")
    got, st = torch_run(c, m, want_m2=False, want_states=False, want_stats=True, counters=True)
    sm.assert_planes(got, sm.expected(c, m), name + ": device form, the colours alone")
    assert st["paths"] == int(sm.counts(m).sum()) and st["kernel_ms"] > 0


def test_device_form_of_a_batch(api, case):
    c = case("room_diffuse")
    cams, seeds = sm.batch_cameras(api, c), sm.BATCH_SEEDS
    maps = np.stack([sm.mixed_map(), sm.mixed_map(3), sm.mixed_map(6)[::-1].copy()])
    got, st = torch_run(c, maps, rect=sm.RECT, cams=cams, seeds=seeds)
    assert st is None
    for v in range(3):
        sm.assert_planes(tuple(x[v] for x in got), sm.expected(c, maps[v], seed=seeds[v], cam=cams[v], rect=sm.RECT), "device form, view %d" % v)


# ---- 9. every kernel of the family; job batches; the exact walk ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["room_diffuse", "c2_analytic", lg.TABLE_SCENE])
def test_every_kernel_of_the_family(case, monkeypatch, name):
    """pt_sample_map<counters, diffuse, tabs>: the diffuse room takes the diffuse flavour, ORT_KERNEL=general its all-lobes one (the
    analytic scene's own); ORT_LDS_TABLES=0 reads the tables from HBM, as the table scene always does -- with it, ORT_KERNEL=general
    launches the all-lobes flavour with tabs = false, with and without counters, which nothing else does.  One answer; with
    counters, paths = the sum of min(map, cap) over the rect"""
    c = case(name)
    m = sm.mixed_map()
    want = sm.expected(c, m, rect=sm.RECT)
    asked = int(sm.counts(m)[sm.inside(sm.RECT)].sum())
    for env in ({}, {"ORT_LDS_TABLES": "0"}, {"ORT_KERNEL": "general"}, {"ORT_KERNEL": "general", "ORT_LDS_TABLES": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for counters in (False, True):
            got, st = run(c, m, rect=sm.RECT, counters=counters)
            sm.assert_planes(got, want, "%s %s counters=%s" % (name, env, counters))
            assert st["paths"] == (asked if counters else 0)
        for k in env:
            monkeypatch.delenv(k)


def test_independent_of_batches_and_walk(case, monkeypatch):
    c = case("room_all_lobes")
    m = sm.mixed_map()
    want = sm.expected(c, m, rect=sm.RECT)
    for batch in ("0", "7", "128"):
        monkeypatch.setenv("ORT_JOB_BATCH", batch)
        got, _ = run(c, m, rect=sm.RECT)
        sm.assert_planes(got, want, "ORT_JOB_BATCH=" + batch)
    monkeypatch.delenv("ORT_JOB_BATCH")
    monkeypatch.setenv("ORT_DEBUG_FORCE_FALLBACK", "0")
    got, st = run(c, m, rect=sm.RECT, counters=True)
    monkeypatch.delenv("ORT_DEBUG_FORCE_FALLBACK")
    sm.assert_planes(got, want, "every ray re-cast exactly")
    assert st["fallback_rays"] == st["rays"] > 0
