"""Path-depth renders on the device (ort_render_depths, ort_render_views_depths and their device forms; kernels pt_depths): the bin
frames, the length planes, the unsplit frame and the final stream states, bit for bit the fold over the oracle's chains of
one-sample calls (tests/depths_cases.py).  Frames are 24 x 16, at most 16 spp, but for the one many-jobs case; one uploaded scene
per case."""
import numpy as np
import pytest

import depths_cases as dc
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

W, H = dc.W, dc.H
ALL = ("rgb", "lengths", "states")


def _uploaded(api, c):
    if c.scene.device is None:
        assert api.device_count() >= 1, "GPU test on a machine without a HIP device (the render path has no CPU fallback)"
        c.scene.upload(0)
    return c


@pytest.fixture()
def case(api, oracle, tmp_path_factory):
    return lambda name: _uploaded(api, dc.case(api, oracle, name, tmp_path_factory))


def guards(V, G, want=ALL, size=None):
    """the host planes of a call, every word a guard value"""
    w, h = size if size else (W, H)
    lead = () if V is None else (V,)
    planes = {"bins": np.full(lead + (G, h, w, 3), dc.GUARD_F, "<f4"), "rgb": np.full(lead + (h, w, 3), dc.GUARD_F, "<f4"),
              "lengths": np.full(lead + (G, h, w), dc.GUARD_LEN, "<u4"), "states": np.full(lead + (h, w), dc.GUARD_STATE, "<u4")}
    return {k: v for k, v in planes.items() if k == "bins" or k in want}


def run(c, G, spp, rect=None, seed=dc.SEED, want=ALL, rr=dc.RR, size=None, **kw):
    """the single-frame host form on guard-filled planes -> (bins, rgb or None, lengths or None, states or None), stats"""
    w, h = size if size else (W, H)
    bins, others, st = c.scene.render_depths(w, h, spp, seed, bins=G, rr=rr, want=want, rect=rect, out=guards(None, G, want, size), **kw)
    return (bins, others.get("rgb"), others.get("lengths"), others.get("states")), st


def run_views(c, cams, seeds, G, spp, rect=None, want=ALL, **kw):
    bins, others, st = c.scene.render_views_depths(cams, seeds, W, H, spp, bins=G, rr=dc.RR, want=want, rect=rect, out=guards(len(cams), G, want), **kw)
    return (bins, others.get("rgb"), others.get("lengths"), others.get("states")), st


def check(c, got, G, spp, rect, what, seed=dc.SEED, cam=None):
    dc.assert_planes(got, dc.expected(c, G, spp, seed, cam), rect, what)


def same(a, b, what):
    for x, y in zip(a, b):
        assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()), what


# ---- 1. against the fold -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.SCENES)
def test_planes_are_the_fold(case, name):
    """every scene, every bin count, 16 spp and 1, the rect and the whole frame: every plane bit for bit, the pixels outside the
    rect keep their guard values"""
    c = case(name)
    for G in dc.BINS:
        for spp, rect in ((16, dc.RECT), (1, dc.RECT), (16, None)):
            got, st = run(c, G, spp, rect)
            check(c, got, G, spp, rect, "%s G = %d, %d spp %r" % (name, G, spp, rect))
            assert st["kernel_ms"] > 0 and st["paths"] == 0   # counters only on request
    assert name not in dc.ANALYTIC or (got[0] != 0).any(axis=(1, 2, 3)).all()   # G = 8, whole frame: no bin's frame is black


# ---- 2. the identities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["room_diffuse", "c2_analytic"])
def test_identities_1_to_4(case, name):
    c = case(name)
    for spp in dc.SPPS:
        img, _ = c.scene.render(W, H, spp, dc.SEED, "pixel", rr=dc.RR)
        one, _ = run(c, 1, spp)
        three, _ = run(c, 3, spp)
        eight, _ = run(c, 8, spp)
        assert_bits_equal(one[1], img, "%s %d spp: identity 1, out_rgb against ort_render_image" % (name, spp))
        assert one[3].tobytes() == c.states(spp).tobytes(), "identity 1: the states"
        for got in (three, eight):
            assert got[1].tobytes() == one[1].tobytes() and got[3].tobytes() == one[3].tobytes()
            assert (got[2].sum(axis=0) == spp).all()
        assert one[0][0].tobytes() == one[1].tobytes() and (one[2] == spp).all(), "identity 2"
        assert three[0][:2].tobytes() == eight[0][:2].tobytes() and three[2][:2].tobytes() == eight[2][:2].tobytes(), "identity 3"
    # identity 3, the other half: NULL optional planes change no bit of the others
    base, _ = run(c, 3, 16, dc.RECT)
    for want in ((), ("lengths",), ("rgb", "states")):
        got, _ = run(c, 3, 16, dc.RECT, want=want)
        check(c, got, 3, 16, dc.RECT, "%s: want %r" % (name, want))
        assert got[0].tobytes() == base[0].tobytes()
    # identity 4: without the roulette nothing bounces
    got, _ = run(c, 3, 4, rr=0.0)
    assert (dc.bits(got[0][1:]) == 0).all() and (got[2][0] == 4).all() and not got[2][1:].any()
    assert got[0][0].tobytes() == got[1].tobytes() and got[0][0].any()
    want = dc.fold(dc.chains(c, n=4, rr=0.0), 3, 4)
    dc.assert_planes(got, want, None, name + ": rr = 0")


@pytest.mark.parametrize("name", dc.lg.ROOMS)
def test_batch_of_views(api, case, name):
    """identity 6: three views on three seeds, two of them the same camera: against the fold from each camera, and against the
    single-frame calls and one-view batches; with counters, paths = views x rect pixels x spp"""
    c = case(name)
    cams, seeds = dc.batch_cameras(api, c), dc.BATCH_SEEDS
    for spp, rect, G in ((16, dc.RECT, 3), (1, None, 8)):
        got, st = run_views(c, cams, seeds, G, spp, rect, counters=True)
        for v in range(3):
            check(c, tuple(x[v] for x in got), G, spp, rect, "%s: view %d of the batch, %d spp" % (name, v, spp), seeds[v], cams[v])
        x0, y0, x1, y1 = rect if rect else (0, 0, W, H)
        assert st["paths"] == 3 * (x1 - x0) * (y1 - y0) * spp
        for v in (0, 2):   # the scene's own camera: the single-frame call on that seed
            one, _ = run(c, G, spp, rect, seed=seeds[v])
            same(one, tuple(x[v] for x in got), (name, v))
        for order in ([1], [2, 1, 0]):
            part, _ = run_views(c, cams[order], [seeds[v] for v in order], G, spp, rect)
            same(part, tuple(x[order] for x in got), (name, order))
    assert got[0][0].tobytes() != got[0][2].tobytes() and got[0][0].tobytes() != got[0][1].tobytes()


# ---- 3. the device forms, on torch tensors on a stream of their own ----------------------------------------------------------------
def torch_run(c, G, spp, rect=None, cams=None, seeds=None, want=ALL, want_stats=False, counters=False, pad=16):
    """-> (bins, rgb or None, lengths or None, states or None) as numpy, stats; every tensor has `pad` guard words at both ends,
    which are checked here, and guard values throughout"""
    import torch
    dev = torch.device("cuda", 0)
    V = 1 if cams is None else len(cams)
    n = V * H * W
    names = ("bins", "rgb", "lengths", "states")
    sizes = (3 * n * G, 3 * n, n * G, n)
    guard = (dc.GUARD_F, dc.GUARD_F, dc.GUARD_LEN, dc.GUARD_STATE)
    fills = (float(dc.GUARD_F), float(dc.GUARD_F), dc.GUARD_LEN - (1 << 32), dc.GUARD_STATE - (1 << 32))
    t = [torch.full((k + 2 * pad,), f, dtype=dt, device=dev) for k, f, dt in zip(sizes, fills, (torch.float32, torch.float32, torch.int32, torch.int32))]
    ptr = [x.data_ptr() + 4 * pad if name == "bins" or name in want else 0 for x, name in zip(t, names)]
    p = c.scene.params(W, H, spp, dc.SEED, "pixel", 0, rect, dc.RR, counters)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        if cams is None:
            st = c.scene.render_depths_device(p, G, *ptr, stream=stream.cuda_stream, want_stats=want_stats)
        else:
            st = c.scene.render_views_depths_device(p, cams, seeds, G, *ptr, stream=stream.cuda_stream, want_stats=want_stats)
    stream.synchronize()
    h = [x.cpu().numpy() for x in t]
    for x, f in zip(h, guard):
        g = np.array(f, x.dtype if x.dtype.kind == "f" else "<u4").reshape(1).view("<u4")[0]
        assert (x[:pad].view("<u4") == g).all() and (x[-pad:].view("<u4") == g).all(), "a guard word around a plane was written"
    lead = () if cams is None else (V,)
    shapes = (lead + (G, H, W, 3), lead + (H, W, 3), lead + (G, H, W), lead + (H, W))
    planes = [x[pad:-pad].reshape(s) if x.dtype.kind == "f" else x[pad:-pad].view("<u4").reshape(s) for x, s in zip(h, shapes)]
    for name, x, f in zip(names[1:], planes[1:], guard[1:]):
        if name not in want:
            assert (x == f).all(), "the %s plane was not passed and was written" % name
    return (planes[0],) + tuple(x if name in want else None for name, x in zip(names[1:], planes[1:])), st


@pytest.mark.parametrize("name", dc.SCENES)
def test_device_form_on_a_stream(case, name):
    c = case(name)
    got, st = torch_run(c, 3, 16, dc.RECT)          # stats == NULL: enqueued, then synchronised
    assert st is None
    check(c, got, 3, 16, dc.RECT, name + ": device form")
    got, st = torch_run(c, 8, 1, None, want=(), want_stats=True, counters=True)
    check(c, got, 8, 1, None, name + ": device form, the bin frames alone")
    assert st["paths"] == W * H and st["rays"] >= st["paths"] and st["kernel_ms"] > 0


def test_device_form_of_a_batch(api, case):
    c = case("room_diffuse")
    cams, seeds = dc.batch_cameras(api, c), dc.BATCH_SEEDS
    got, st = torch_run(c, 3, 16, dc.RECT, cams=cams, seeds=seeds)
    assert st is None
    for v in range(3):
        check(c, tuple(x[v] for x in got), 3, 16, dc.RECT, "device form, view %d" % v, seeds[v], cams[v])


# ---- 4. every kernel of the family; counters ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["room_diffuse", "c2_analytic", dc.lg.TABLE_SCENE])
def test_every_kernel_of_the_family(case, monkeypatch, name):
    """pt_depths<counters, diffuse, tabs>: the diffuse room takes the diffuse flavour, ORT_KERNEL=general its all-lobes one (the
    analytic scene's own); ORT_LDS_TABLES=0 reads the tables from HBM, as the table scene always does.  One answer;
    ORT_RENDER_COUNTERS changes no plane and gives paths = rect pixels x spp"""
    c = case(name)
    x0, y0, x1, y1 = dc.RECT
    for env in ({}, {"ORT_LDS_TABLES": "0"}, {"ORT_KERNEL": "general"}, {"ORT_KERNEL": "general", "ORT_LDS_TABLES": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for counters in (False, True):
            got, st = run(c, 3, 16, dc.RECT, counters=counters)
            check(c, got, 3, 16, dc.RECT, "%s %s counters=%s" % (name, env, counters))
            assert st["paths"] == ((x1 - x0) * (y1 - y0) * 16 if counters else 0)
        for k in env:
            monkeypatch.delenv(k)


def test_independent_of_batches_and_walk(case, monkeypatch):
    """the job batches change nothing, and a re-cast of the same ray on the exact octree walk is not a new depth"""
    c = case("room_all_lobes")
    for batch in ("0", "7", "128"):
        monkeypatch.setenv("ORT_JOB_BATCH", batch)
        got, _ = run(c, 3, 16, dc.RECT)
        check(c, got, 3, 16, dc.RECT, "ORT_JOB_BATCH=" + batch)
    monkeypatch.delenv("ORT_JOB_BATCH")
    monkeypatch.setenv("ORT_DEBUG_FORCE_FALLBACK", "0")
    got, st = run(c, 8, 16, dc.RECT, counters=True)
    monkeypatch.delenv("ORT_DEBUG_FORCE_FALLBACK")
    check(c, got, 8, 16, dc.RECT, "every ray re-cast exactly")
    assert st["fallback_rays"] == st["rays"] > 0


# ---- 5. a hostile light, seen directly -----------------------------------------------------------------------------------------------
def test_non_finite_light_seen_directly(api, oracle):
    """hostile_materials' emission scene: lights whose emit holds inf and NaN, seen directly (unguarded, so bin 0 and the frame
    hold them) and after bounces (dropped where the product is not finite).  Against the oracle's fold, NaN by position"""
    import hostile_materials as hm
    c = _uploaded(api, hm.emission_case(api, oracle))
    ch = dc.record(oracle, c.twin(None), c.cam, (W, H), (0, 0, W, H), dc.SEED, 16)
    want = dc.fold(ch, 3, 16)
    assert np.isnan(want[0][0]).any() and np.isinf(want[0][0]).any(), "no non-finite light is seen directly"
    assert (want[0][1:] != 0).any()   # and after bounces
    got, _ = run(c, 3, 16, dc.RECT)
    dc.assert_planes(got, want, dc.RECT, "hostile emission", nan_by_position=True)
    assert np.isnan(got[0][0]).any()


# ---- 6. more jobs than resident lanes ------------------------------------------------------------------------------------------------
BIG = (1024, 768)
WINDOW = (501, 371, 533, 403)   # 32 x 32, aligned to 8 in neither x nor y


def test_many_jobs(case):
    """1024 x 768 at 1 spp, G = 3: three jobs per resident lane of a 256-unit device, with a batch of jobs straddling the end.
    Without the oracle: out_rgb against ort_render_image PIXEL on the device, the G = 1 call's bins against out_rgb, frames 0 and
    1 against the G = 8 call's, the lengths summing to 1; and a 32 x 32 window of the frame against the fold"""
    c = case("room_all_lobes")
    w, h = BIG
    img, _ = c.scene.render(w, h, 1, dc.SEED, "pixel", rr=dc.RR)
    three, _ = run(c, 3, 1, size=BIG)
    assert_bits_equal(three[1], img, "out_rgb against ort_render_image")
    assert (three[2].sum(axis=0) == 1).all() and three[2].max() == 1
    assert (three[2].reshape(3, -1).sum(axis=1) > 0).all() and (three[0] != 0).any(axis=(1, 2, 3)).all()
    one, _ = run(c, 1, 1, size=BIG, want=("rgb",))
    assert one[0][0].tobytes() == one[1].tobytes() == img.tobytes()
    eight, _ = run(c, 8, 1, size=BIG, want=("lengths",))
    assert eight[0][:2].tobytes() == three[0][:2].tobytes() and eight[2][:2].tobytes() == three[2][:2].tobytes()
    assert (eight[2][2:].sum(axis=0) == three[2][2]).all()
    want = dc.expected(c, 3, 1, size=BIG, window=WINDOW)
    x0, y0, x1, y1 = WINDOW   # the rest of the frame was rendered too: the window's words alone
    for name, g, wnt in zip(("bins", "lengths", "rgb", "states"), (three[0], three[2], three[1], three[3]), want):
        cut = (Ellipsis, slice(y0, y1), slice(x0, x1)) + ((slice(None),) if name in ("bins", "rgb") else ())
        assert dc.bits(g[cut]).tobytes() == dc.bits(wnt[cut]).tobytes(), "the window against the fold: " + name
