"""Accumulating renders on the device (ort_render_accumulate, ort_render_views_accumulate and their device forms; kernels
pt_accumulate): the scenarios of tests/accumulate_cases.py, which the host tests run through tools/host_sim, through the library
-- every plane bit for bit the oracle's or the reference's chains folded into undivided sums -- and what only a device shows:
passes chained on a stream with no synchronisation between them, more jobs than resident lanes, a continued job whose traversal
stack reaches its scratch tail, and the checkpoint of a frame.  Frames are 24 x 16 unless said otherwise."""
import numpy as np
import pytest

import accumulate_cases as acs
import deep_scenes as ds
import light_groups_cases as lg
import many_jobs_cases as mj
import reference_goldens as rg
import sample_map_cases as sm

pytestmark = pytest.mark.gpu

W, H = acs.W, acs.H


@pytest.fixture()
def case(api, oracle, tmp_path_factory):
    def get(name):
        c = lg.case(api, oracle, name, tmp_path_factory)
        if c.scene.device is None:
            assert api.device_count() >= 1, "GPU test on a machine without a HIP device (the render path has no CPU fallback)"
            c.scene.upload(0)
        return c
    return get


def bits(a):
    return np.ascontiguousarray(a).view("<u4")


# ---- 1. the shared scenarios ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counters", [False, True])
@pytest.mark.parametrize("name", sm.SCENES)
def test_identity_1_one_call_is_the_sample_map_render(api, case, name, counters):
    c = case(name)
    out = c.scene.render_sample_map(W, H, sm.mixed_map(), acs.CAP, acs.SEED, True, True, rect=acs.RECT, rr=acs.RR, out=sm.guards())
    acs.identity_1(acs.library_call(api, c, counters=counters), c, out[:3], "%s counters=%s" % (name, counters))


@pytest.mark.parametrize("name", ["room_all_lobes", "c4_dwarf_room"])
def test_identity_2_uniform_split(api, case, name):
    c = case(name)
    img, _ = c.scene.render(W, H, 16, acs.SEED, "pixel", rect=acs.RECT, rr=acs.RR, out=np.full((H, W, 3), acs.GUARD_RGB, "<f4"))
    acs.identity_2_uniform(acs.library_call(api, c), c, img, name)
    rgb, spp, m2, states, _ = c.scene.render_adaptive(W, H, 16, 16, 0.3, seed=acs.SEED, rect=acs.RECT, rr=acs.RR, want_states=True)
    split = acs.Planes()
    for k in acs.SPLIT:
        acs.library_call(api, c, counters=False)(split, None, k, acs.RECT)
    at = sm.inside(acs.RECT)
    assert (bits(split.m2[0])[at] == bits(m2)[at]).all() and (split.states[0][at] == states[at]).all() and (split.count[0][at] == spp[at]).all()


@pytest.mark.parametrize("env", [{}, {"ORT_LDS_TABLES": "0"}, {"ORT_KERNEL": "general"}, {"ORT_KERNEL": "general", "ORT_LDS_TABLES": "0"}], ids=str)
def test_identity_2_per_pixel_split_on_every_kernel(api, case, monkeypatch, env):
    """pt_accumulate<counters, diffuse, tabs>: the diffuse room takes the diffuse flavour, ORT_KERNEL=general its all-lobes one,
    ORT_LDS_TABLES=0 reads the tables from HBM; with and without counters"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = case("room_diffuse")
    for counters in (False, True):
        acs.identity_2_per_pixel(acs.library_call(api, c, counters=counters), c, "room_diffuse %r counters=%s" % (env, counters))


@pytest.mark.parametrize("name", rg.CHAIN_SCENES)
def test_against_the_references_chains(api, case, name):
    """64 samples as 1 + 3 + 12 + 48 against the fold of chains_rooms.npz: no oracle in between"""
    assert sum(acs.REF_SPLIT) == rg.CHAIN_SAMPLES
    acs.reference_split(acs.library_call(api, case(name)), rg.chains_from(rg.load("chains_rooms.npz"), name), name)


def test_identity_3_hostile_planes_saturation_and_null_map(api, case):
    c = case("room_all_lobes")
    for counters in (True, False):
        call = acs.library_call(api, c, counters=counters)
        acs.identity_3(call, c, "hostile planes, counters=%s" % counters)
        acs.saturation(call, c, "saturation, counters=%s" % counters)
    acs.null_map(acs.library_call(api, c), c, "no map")


def test_identity_4_optional_planes(api, case):
    c = case("room_diffuse")
    acs.identity_4(acs.library_call(api, c), c, "room_diffuse")


@pytest.mark.parametrize("name", ["room_all_lobes", lg.TABLE_SCENE])
def test_identity_5_batch_of_views(api, case, name):
    c = case(name)
    acs.identity_5(acs.library_call(api, c), api, c, name)


# ---- 2. the Accumulator: a checkpoint ---------------------------------------------------------------------------------------------
def test_accumulator_checkpoint(api, case, tmp_path):
    """two passes, save, load, one more pass: the uninterrupted run's planes; .rgb() is out_rgb where the last call sampled, and
    the PIXEL render at the total"""
    c = case("room_all_lobes")
    whole, parts = api.Accumulator(W, H), api.Accumulator(W, H)
    out_whole, out = np.full((H, W, 3), acs.GUARD_RGB, "<f4"), np.full((H, W, 3), acs.GUARD_RGB, "<f4")
    c.scene.render_accumulate(whole, 12, acs.SEED, rr=acs.RR, out=out_whole)
    c.scene.render_accumulate(parts, 4, acs.SEED, rr=acs.RR)
    c.scene.render_accumulate(parts, sm.mixed_map(), acs.SEED, cap=5, rr=acs.RR)
    parts.save(str(tmp_path / "frame.npz"))
    back = api.Accumulator.load(str(tmp_path / "frame.npz"))
    assert (back.count == 4 + sm.counts(sm.mixed_map(), 5)).all()
    c.scene.render_accumulate(back, 12 - back.count, acs.SEED, rr=acs.RR, out=out)
    for name in ("sum_rgb", "m2", "count", "states"):
        assert (bits(getattr(back, name)) == bits(getattr(whole, name))).all(), name
    assert len(np.unique(back.count)) == 1 and (bits(out) == bits(out_whole)).all()   # every pixel took samples in the last call
    assert (bits(back.rgb()) == bits(out_whole)).all()
    img, _ = c.scene.render(W, H, 12, acs.SEED, "pixel", rr=acs.RR)
    assert (bits(back.rgb()) == bits(img)).all()


# ---- 3. the device forms: passes chained on a stream ------------------------------------------------------------------------------
def test_four_passes_on_a_stream_without_synchronisation(api, case):
    """torch tensors on a non-default stream, guard words around every plane: four passes (the mixed map, no map, a batch of one
    view through the views form, the shifted map on the rect) enqueued with stats == NULL and no synchronisation between them,
    one torch.cuda.synchronize() at the end: the host form's planes after the same four calls, and the oracle's"""
    import torch
    c = case("room_all_lobes")
    dev = torch.device("cuda", 0)
    n = H * W
    host = acs.Planes()
    stream = torch.cuda.Stream(dev)
    passes = ((sm.mixed_map(), acs.CAP, None, False), (None, 3, None, False), (None, 2, acs.SMALL_RECT, True), (sm.mixed_map(3), 7, acs.RECT, False))
    with torch.cuda.stream(stream):
        d = acs.DevicePlanes(host)
        ptr = d.ptr
        maps = [None if m is None else torch.from_numpy(np.ascontiguousarray(m, "<u4").view("<i4").reshape(-1)).to(dev) for m, _, _, _ in passes]
        for (m, cap, rect, views_form), d_map in zip(passes, maps):
            p = c.scene.params(W, H, cap, acs.SEED, "pixel", 0, rect, acs.RR)
            args = dict(d_m2=ptr[1], d_map=d_map.data_ptr() if d_map is not None else 0, d_rgb=ptr[4], stream=stream.cuda_stream)
            if views_form:
                st = c.scene.render_views_accumulate_device(p, c.camera()[None], [acs.SEED], ptr[0], ptr[2], ptr[3], **args)
            else:
                st = c.scene.render_accumulate_device(p, ptr[0], ptr[2], ptr[3], **args)
            assert st is None
    torch.cuda.synchronize()
    call = acs.library_call(api, c, counters=False)
    want = acs.Planes()
    chain = sm.chains(c, cap=acs.CAP + 3 + 2 + 7)
    for m, cap, rect, _ in passes:
        call(host, m, cap, rect)
        acs.model(want, 0, chain, m, cap, rect)
    acs.assert_planes(host, want, "the host form against the oracle")
    acs.assert_planes(d.download(), host, "four passes on a stream against the host form")
    for m, d_map in zip((p[0] for p in passes), maps):
        assert d_map is None or (d_map.cpu().numpy().view("<u4") == m.reshape(-1)).all(), "the map was written"
    # one pass of the same total through the device form with stats: the same sums, the paths counted
    one = [torch.zeros(k, dtype=dt, device=dev) for k, dt in ((3 * n, torch.float32), (n, torch.float32), (n, torch.int32), (n, torch.int32))]
    total = torch.from_numpy(np.ascontiguousarray(want.count[0]).view("<i4").reshape(-1)).to(dev)
    p = c.scene.params(W, H, int(want.count.max()), acs.SEED, "pixel", 0, None, acs.RR, True)
    st = c.scene.render_accumulate_device(p, one[0].data_ptr(), one[2].data_ptr(), one[3].data_ptr(), d_m2=one[1].data_ptr(), d_map=total.data_ptr(), want_stats=True)
    assert st["paths"] == int(want.count.sum()) and st["kernel_ms"] > 0
    sampled = want.count[0] > 0
    for x, w_ in zip(one, (want.sum[0], want.m2[0], want.count[0], want.states[0])):
        assert (x.cpu().numpy().view("<u4").reshape(bits(w_).shape)[sampled] == bits(w_)[sampled]).all()


# ---- 4. more jobs than resident lanes ---------------------------------------------------------------------------------------------
def test_many_jobs_two_passes(api, case):
    """1024 x 768, three jobs per resident lane of a 256-unit device: two passes of 2 + 2 samples against one pass of 4 and the
    PIXEL render at spp = 4 over the whole frame, and window by window against the oracle's chains folded"""
    c = case("room_all_lobes")
    split, one = api.Accumulator(mj.W, mj.H), api.Accumulator(mj.W, mj.H)
    out = np.full((mj.H, mj.W, 3), acs.GUARD_RGB, "<f4")
    st = c.scene.render_accumulate(split, 2, mj.SEED, rr=mj.RR, counters=True)
    assert st["paths"] == 2 * mj.W * mj.H
    c.scene.render_accumulate(split, 2, mj.SEED, rr=mj.RR, out=out)
    c.scene.render_accumulate(one, 4, mj.SEED, rr=mj.RR)
    for name in ("sum_rgb", "m2", "count", "states"):
        mj.assert_same(getattr(split, name), getattr(one, name), "2 + 2 against 4: " + name)
    img, _ = c.scene.render(mj.W, mj.H, 4, mj.SEED, "pixel", rr=mj.RR)
    mj.assert_same(out, img, "out_rgb against the PIXEL render at spp = 4")
    assert (split.count == 4).all()
    for win in mj.WINDOWS:
        x0, y0, x1, y1 = win
        want = acs.Planes(size=mj.SIZE)
        for k in (2, 2):
            acs.model(want, 0, mj.window_chains(c, win), None, k, win, size=mj.SIZE)
        for got, w_, label in zip((split.sum_rgb, split.m2, split.count, split.states, out), want.all(), acs.NAMES):
            mj.assert_window(got, np.ascontiguousarray(w_[0, y0:y1, x0:x1]), win, "2 + 2 against the oracle's chains: " + label)


# ---- 5. the deep-stack scene ------------------------------------------------------------------------------------------------------
def test_a_continued_job_with_its_stack_in_the_scratch_tail(api, oracle, tmp_path_factory):
    """the scene of tests/deep_scenes.py, where nearly every ray's traversal stack goes past its LDS entries: 1 + 3 samples
    against the oracle's chains of four"""
    w = ds.world(api, oracle, tmp_path_factory)
    if w.scene.device is None:
        w.scene.upload(0)
    width, height, spp, _ = ds.RENDER
    assert (width, height, spp) == (W, H, 4)
    chain = ds.pixel_chains(w)
    for counters in (False, True):
        call = acs.library_call(api, w, counters=counters)
        got, want = acs.Planes(), acs.Planes()
        for k in (1, 3):
            paths = call(got, None, k, None, seed=ds.SEED)
            assert paths in (None, k * W * H)
            acs.model(want, 0, chain, None, k, None)
            acs.assert_planes(got, want, "deep scene, counters=%s, after the pass of %d" % (counters, k))
