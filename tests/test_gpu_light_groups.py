"""Light-group renders on the device (ort_render_light_groups, ort_render_views_light_groups and their device forms; kernels
pt_groups): the group frames, the unsplit frame and the final stream states, bit for bit the oracle's PIXEL renders of the dark
twins and of the scene itself (tests/light_groups_cases.py).  Frames are 24 x 16, at most 16 spp; one uploaded scene per case."""
import numpy as np
import pytest

import light_groups_cases as lg
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

W, H = lg.W, lg.H


@pytest.fixture()
def case(api, oracle, tmp_path_factory):
    def get(name):
        c = lg.case(api, oracle, name, tmp_path_factory)
        if c.scene.device is None:
            assert api.device_count() >= 1, "GPU test on a machine without a HIP device (the render path has no CPU fallback)"
            c.scene.upload(0)
        return c
    return get


def guards(V, G, want_rgb=True, want_states=True):
    """the host planes of a call, every word a guard value"""
    lead = () if V is None else (V,)
    return ([np.full(lead + (G, H, W, 3), lg.GUARD_F, "<f4")] + ([np.full(lead + (H, W, 3), lg.GUARD_F, "<f4")] if want_rgb else []) +
            ([np.full(lead + (H, W), lg.GUARD_STATE, "<u4")] if want_states else []))


def run(c, groups, G, spp, rect=None, seed=lg.SEED, want_rgb=True, want_states=True, filler=0x5A, **kw):
    """the single-frame host form on guard-filled planes -> (frames (G, H, W, 3), rgb or None, states or None), stats"""
    out = c.scene.render_light_groups(W, H, spp, seed, c.table(groups, filler), want_rgb, want_states, group_count=G, rect=rect, rr=lg.RR,
                                      out=guards(None, G, want_rgb, want_states), **kw)
    return (out[0], out[1] if want_rgb else None, out[-2] if want_states else None), out[-1]


def run_views(c, cams, seeds, groups, G, spp, rect=None, **kw):
    out = c.scene.render_views_light_groups(cams, seeds, W, H, spp, c.table(groups), True, True, group_count=G, rect=rect, rr=lg.RR,
                                            out=guards(len(cams), G), **kw)
    return out[:3], out[3]


def check(c, got, groups, G, spp, rect, what, seed=lg.SEED, cam=None):
    frames, rgb, states = got
    lg.assert_plane(frames, c.expected(groups, G, spp, seed, cam, rect), rect, lg.GUARD_F, what + ": group frames")
    if rgb is not None:
        lg.assert_plane(rgb, c.frame(None, spp, seed, cam, rect), rect, lg.GUARD_F, what + ": rgb")
    if states is not None:
        lg.assert_plane(states, c.states(spp, seed, cam, rect), rect, lg.GUARD_STATE, what + ": states")


def scene_groups(c):
    """one group per light; the table scene: its lights past the LDS cap share the last group"""
    return c.per_light() if c.name != lg.TABLE_SCENE else {m: min(g, 2) for g, m in enumerate(c.lights)}


# ---- 1. against the twins --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lg.SCENES)
def test_frames_are_the_twins(case, name):
    """every scene, one group per light, 16 spp and 1, the rect and the whole frame: every plane bit for bit, the pixels outside
    the rect keep their guard values"""
    c = case(name)
    groups = scene_groups(c)
    G = max(groups.values()) + 1
    for spp, rect in ((16, lg.RECT), (1, lg.RECT), (16, None)):
        got, st = run(c, groups, G, spp, rect)
        check(c, got, groups, G, spp, rect, "%s %d spp %r" % (name, spp, rect))
        assert st["kernel_ms"] > 0 and st["paths"] == 0   # counters only on request
    assert (got[0] != 0).any(axis=(1, 2, 3)).all()   # no group's frame is black


@pytest.mark.parametrize("name", ["room_all_lobes", "testscene"])
def test_group_tables(case, name):
    """G = 1, G = 8 with empty groups, a light in no group, two lights sharing a group against the twin that keeps both"""
    c = case(name)
    a, b, rest = c.lights[0], c.lights[1], c.lights[2:]
    tables = {
        "G = 1, every light": ({m: 0 for m in c.lights}, 1),
        "G = 1, one light in no group": ({m: 0 for m in c.lights[1:]}, 1),
        "G = 8, empty groups": ({a: 6, b: 2, **{m: 7 for m in rest}}, 8),
        "two lights share a group": ({a: 1, b: 1, **{m: 0 for m in rest}}, 2),
    }
    for what, (groups, G) in tables.items():
        got, _ = run(c, groups, G, 16, lg.RECT)
        check(c, got, groups, G, 16, lg.RECT, "%s: %s" % (name, what))
    got, _ = run(c, *tables["G = 8, empty groups"], 16, None)
    assert not got[0][[0, 1, 3, 4, 5]].any() and got[0][[2, 6, 7]].any(axis=(1, 2, 3)).all()


# ---- 2. identity 1: against the render call in the same process -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["room_diffuse", "c4_dwarf_room"])
def test_rgb_is_the_pixel_render(case, name):
    c = case(name)
    for spp in lg.SPPS:
        img, _ = c.scene.render(W, H, spp, lg.SEED, "pixel", rr=lg.RR)
        got, _ = run(c, c.per_light(), len(c.lights), spp)
        assert_bits_equal(got[1], img, "%s %d spp: out_rgb against ort_render_image" % (name, spp))


# ---- 3. identity 3: a group's frame depends only on which lights are in it --------------------------------------------------------
@pytest.mark.parametrize("name", ["room_all_lobes", "c2_analytic"])
def test_frame_depends_only_on_its_group(case, name):
    c = case(name)
    a, others = c.lights[0], c.lights[1:]
    base, _ = run(c, c.per_light(), len(c.lights), 16, lg.RECT)
    want = c.frame([a], 16, rect=lg.RECT)
    lg.assert_plane(base[0][0], want, lg.RECT, lg.GUARD_F, name)
    variants = {
        "the other lights in one group": ({a: 0, **{m: 1 for m in others}}, 2, 0, True, True),
        "the other lights in no group, G = 1": ({a: 0}, 1, 0, True, True),
        "another G, another index": ({a: 2, **{m: 7 - k for k, m in enumerate(others)}}, 8, 2, True, True),
        "no rgb": (c.per_light(), len(c.lights), 0, False, True),
        "no states": (c.per_light(), len(c.lights), 0, True, False),
        "neither": (c.per_light(), len(c.lights), 0, False, False),
    }
    for what, (groups, G, g, want_rgb, want_states) in variants.items():
        for filler in (0x5A, 0):   # and not on the entries of the materials that are no light
            got, _ = run(c, groups, G, 16, lg.RECT, want_rgb=want_rgb, want_states=want_states, filler=filler)
            assert got[0][g].tobytes() == base[0][0].tobytes(), "%s: %s" % (name, what)
            check(c, got, groups, G, 16, lg.RECT, "%s: %s" % (name, what))


# ---- 4. identity 4: a batch is its views -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lg.ROOMS)
def test_batch_of_views(api, case, name):
    """three views on three seeds, two of them the same camera: against the twins from each camera, and against the single-frame
    calls and one-view batches"""
    c = case(name)
    cams, seeds = lg.batch_cameras(api, c), lg.BATCH_SEEDS
    groups = c.per_light()
    for spp, rect in ((16, lg.RECT), (1, None)):
        got, st = run_views(c, cams, seeds, groups, 3, spp, rect, counters=True)
        for v in range(3):
            check(c, tuple(x[v] for x in got), groups, 3, spp, rect, "%s: view %d of the batch, %d spp" % (name, v, spp), seeds[v], cams[v])
        x0, y0, x1, y1 = rect if rect else (0, 0, W, H)
        assert st["paths"] == 3 * (x1 - x0) * (y1 - y0) * spp
        for v in (0, 2):   # the scene's own camera: the single-frame call on that seed
            one, _ = run(c, groups, 3, spp, rect, seed=seeds[v])
            for a, b in zip(one, got):
                assert a.tobytes() == b[v].tobytes(), (name, v)
        for order in ([1], [2, 1, 0]):
            part, _ = run_views(c, cams[order], [seeds[v] for v in order], groups, 3, spp, rect)
            for a, b in zip(part, got):
                assert a.tobytes() == b[order].tobytes(), (name, order)
    assert got[0][0].tobytes() != got[0][2].tobytes() and got[0][0].tobytes() != got[0][1].tobytes()


# ---- 5. the device forms, on torch tensors on a stream of their own ----------------------------------------------------------------
def torch_run(c, groups, G, spp, rect=None, cams=None, seeds=None, want_rgb=True, want_states=True, want_stats=False, counters=False, pad=16):
    """-> (frames, rgb or None, states or None) as numpy, stats; every tensor has `pad` guard words at both ends, which are
    checked here, and guard values throughout"""
    import torch
    dev = torch.device("cuda", 0)
    V = 1 if cams is None else len(cams)
    n = V * H * W
    sizes = (3 * n * G, 3 * n, n)
    fills = (float(lg.GUARD_F), float(lg.GUARD_F), lg.GUARD_STATE - (1 << 32))
    t = [torch.full((k + 2 * pad,), f, dtype=dt, device=dev) for k, f, dt in zip(sizes, fills, (torch.float32, torch.float32, torch.int32))]
    ptr = [x.data_ptr() + 4 * pad for x in t]
    p = c.scene.params(W, H, spp, lg.SEED, "pixel", 0, rect, lg.RR, counters)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        args = (c.table(groups), ptr[0], ptr[1] if want_rgb else 0, ptr[2] if want_states else 0)
        if cams is None:
            st = c.scene.render_light_groups_device(p, *args, group_count=G, stream=stream.cuda_stream, want_stats=want_stats)
        else:
            st = c.scene.render_views_light_groups_device(p, cams, seeds, *args, group_count=G, stream=stream.cuda_stream, want_stats=want_stats)
    stream.synchronize()
    h = [x.cpu().numpy() for x in t]
    for x, f in zip(h, (lg.GUARD_F, lg.GUARD_F, lg.GUARD_STATE)):
        g = np.array(f, x.dtype if x.dtype.kind == "f" else "<u4").reshape(1).view("<u4")[0]
        assert (x[:pad].view("<u4") == g).all() and (x[-pad:].view("<u4") == g).all(), "a guard word around a plane was written"
    lead = () if cams is None else (V,)
    frames = h[0][pad:-pad].reshape(lead + (G, H, W, 3))
    rgb = h[1][pad:-pad].reshape(lead + (H, W, 3))
    states = h[2][pad:-pad].view("<u4").reshape(lead + (H, W))
    if not want_rgb:
        assert (rgb == lg.GUARD_F).all()
    if not want_states:
        assert (states == lg.GUARD_STATE).all()
    return (frames, rgb if want_rgb else None, states if want_states else None), st


@pytest.mark.parametrize("name", ["room_all_lobes", "c4_dwarf_room", lg.TABLE_SCENE])
def test_device_form_on_a_stream(case, name):
    c = case(name)
    groups = scene_groups(c)
    G = max(groups.values()) + 1
    got, st = torch_run(c, groups, G, 16, lg.RECT)          # stats == NULL: enqueued, then synchronised
    assert st is None
    check(c, got, groups, G, 16, lg.RECT, name + ": device form")
    got, st = torch_run(c, groups, G, 1, None, want_rgb=False, want_states=False, want_stats=True, counters=True)
    check(c, got, groups, G, 1, None, name + ": device form, the group frames alone")
    assert st["paths"] == W * H and st["rays"] >= st["paths"] and st["kernel_ms"] > 0


def test_device_form_of_a_batch(api, case):
    c = case("room_diffuse")
    cams, seeds = lg.batch_cameras(api, c), lg.BATCH_SEEDS
    got, st = torch_run(c, c.per_light(), 3, 16, lg.RECT, cams=cams, seeds=seeds)
    assert st is None
    for v in range(3):
        check(c, tuple(x[v] for x in got), c.per_light(), 3, 16, lg.RECT, "device form, view %d" % v, seeds[v], cams[v])


# ---- 6. every kernel of the family; counters ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["room_diffuse", "c2_analytic", lg.TABLE_SCENE])
def test_every_kernel_of_the_family(case, monkeypatch, name):
    """pt_groups<counters, diffuse, tabs>: the diffuse room takes the diffuse flavour, ORT_KERNEL=general its all-lobes one (the
    analytic scene's own); ORT_LDS_TABLES=0 reads the tables from HBM, as the table scene always does.  One answer; with
    counters, paths = rect pixels x spp"""
    c = case(name)
    groups = scene_groups(c)
    G = max(groups.values()) + 1
    x0, y0, x1, y1 = lg.RECT
    for env in ({}, {"ORT_LDS_TABLES": "0"}, {"ORT_KERNEL": "general"}, {"ORT_KERNEL": "general", "ORT_LDS_TABLES": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for counters in (False, True):
            got, st = run(c, groups, G, 16, lg.RECT, counters=counters)
            check(c, got, groups, G, 16, lg.RECT, "%s %s counters=%s" % (name, env, counters))
            assert st["paths"] == ((x1 - x0) * (y1 - y0) * 16 if counters else 0)
        for k in env:
            monkeypatch.delenv(k)


def test_independent_of_batches_and_walk(case, monkeypatch):
    c = case("room_all_lobes")
    groups = c.per_light()
    for batch in ("0", "7", "128"):
        monkeypatch.setenv("ORT_JOB_BATCH", batch)
        got, _ = run(c, groups, 3, 16, lg.RECT)
        check(c, got, groups, 3, 16, lg.RECT, "ORT_JOB_BATCH=" + batch)
    monkeypatch.delenv("ORT_JOB_BATCH")
    monkeypatch.setenv("ORT_DEBUG_FORCE_FALLBACK", "0")
    got, st = run(c, groups, 3, 16, lg.RECT, counters=True)
    monkeypatch.delenv("ORT_DEBUG_FORCE_FALLBACK")
    check(c, got, groups, 3, 16, lg.RECT, "every ray re-cast exactly")
    assert st["fallback_rays"] == st["rays"] > 0
