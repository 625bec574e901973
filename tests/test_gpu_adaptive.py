"""Adaptive radiance queries on the device (ort_radiance_adaptive / ort_radiance_adaptive_device, kernels
radiance_adaptive_rays): colours, sample counts, second moments and final stream states, bit for bit what the stopping rule of
include/ort.h gives on the oracle's own samples (tests/adaptive_cases.py).  NaN outputs compare by position."""
import numpy as np
import pytest

import adaptive_cases as ac
import radiance_cases as rc
import table_scenes
from adaptive_cases import Adaptive

pytestmark = pytest.mark.gpu

# rays per scene (at most 256); max_spp is at most 64 everywhere
SCENES = {"testscene": 256, "c2_analytic": 256, "glass_room": 192, "c3_bunny_room": 128, "tables_mats_over": 192}
RRS = (0.8, 0.0)
_worlds = {}


class World:
    pass


@pytest.fixture()
def world(api, oracle, gpu_scene, tmp_path_factory):
    """name -> the uploaded scene, its rays and the oracle's chains of 64 samples per ray ({rr: chain}); computed once"""
    def get(name):
        if name not in _worlds:
            w = World()
            if name.startswith("tables_"):
                scene, _, csg = table_scenes.build(api, name[len("tables_"):], tmp_path_factory.mktemp(name))
                w.scene = scene.commit().upload(0)
            else:
                w.scene, csg = gpu_scene(name), True
            flat = w.scene.flatten(1, 1)
            w.osc = oracle.OracleScene(flat, with_reference_csg=csg)
            w.cases = ac.cases_for(name, flat, w.osc, SCENES[name])
            w.chain = {rr: ac.chains(w.osc, w.cases, 64, rr) for rr in RRS}
            w.want = lambda ad, rr=ac.RR, w=w: ac.expected_from(w.chain[rr], w.cases, ad)
            _worlds[name] = w
        return _worlds[name]
    return get


def run(scene, c, ad, rr=ac.RR, **kw):
    """the host form -> (rgb, spp, m2, states), stats"""
    rgb, spp, m2, fin, st = scene.radiance_adaptive(c.rays, c.seeds, ad.min_spp, ad.max_spp, ad.tolerance, ad.floor, ad.check_every, rr,
                                                    want_states=True, **kw)
    return (rgb, spp, m2, fin), st


def torch_run(scene, c, ad, rr=ac.RR, skip=(), counters=False, want_stats=False):
    """the device form, with torch tensors on a non-default stream; without stats the call does not wait: synchronise.
    skip: which of "spp", "m2", "states" to pass as NULL -> (rgb, spp, m2, states) with the fillers where nothing was asked for"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(c.rays)
    d_rays = torch.from_numpy(np.ascontiguousarray(c.rays, "<f4")).to(dev)
    d_seeds = torch.from_numpy(np.ascontiguousarray(c.seeds, "<u4").view("<i4")).to(dev)
    d_out = torch.full((n, 3), -7.0, dtype=torch.float32, device=dev)
    d_spp = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_m2 = torch.full((n,), -7.0, dtype=torch.float32, device=dev)
    d_fin = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        st = scene.radiance_adaptive_device(d_rays.data_ptr(), d_seeds.data_ptr(), n, ad.min_spp, ad.max_spp, ad.tolerance, ad.floor, ad.check_every,
                                            rr, d_out.data_ptr(), 0 if "spp" in skip else d_spp.data_ptr(), 0 if "m2" in skip else d_m2.data_ptr(),
                                            0 if "states" in skip else d_fin.data_ptr(), stream=stream.cuda_stream, counters=counters,
                                            want_stats=want_stats)
    stream.synchronize()
    return (d_out.cpu().numpy(), d_spp.cpu().numpy().view("<u4"), d_m2.cpu().numpy(), d_fin.cpu().numpy().view("<u4")), st


# ---- 1. against the oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rr", RRS)
@pytest.mark.parametrize("ad", ac.SETS, ids=["main", "every", "fixed"])
@pytest.mark.parametrize("name", list(SCENES))
def test_adaptive_is_the_rule_on_the_oracles_samples(world, name, ad, rr):
    w = world(name)
    got, st = run(w.scene, w.cases, ad, rr)
    ac.assert_same(got, w.want(ad, rr), "%s %r rr %g, host form" % (name, ad, rr))
    assert st["kernel_ms"] > 0 and st["paths"] == 0   # counters only on request


# ---- 2. the two identities, against ort_radiance in the same process -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["c2_analytic", "glass_room", "c3_bunny_room"])
def test_identities_against_radiance(world, name):
    w = world(name)
    c = w.cases
    for n in (2, 7):
        rgb, fin, _ = w.scene.radiance(c.rays, c.seeds, n, ac.RR, want_states=True)
        got, _ = run(w.scene, c, Adaptive(n, n, 1, 0.3, 0.05))
        rc.assert_same(got[0], got[3], rgb, fin, "%s min = max = %d" % (name, n))
        assert (got[1][c.ok] == n).all() and (got[1][~c.ok] == 0).all()
    rgb, fin, _ = w.scene.radiance(c.rays, c.seeds, 4, ac.RR, want_states=True)
    got, _ = run(w.scene, c, ac.HUGE)
    assert np.isfinite(got[2]).all()
    rc.assert_same(got[0], got[3], rgb, fin, name + " huge tolerance")
    assert (got[1][c.ok] == 4).all()
    ac.assert_same(got, w.want(ac.HUGE), name + " huge tolerance against the rule")


# ---- 3. counts and guard words; NULL outputs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 63, 65, 513])
def test_counts_and_guard_words(api, world, count):
    w = world("testscene")
    idx = np.arange(count) % len(w.cases.rays)
    c = w.cases.take(idx)
    want = tuple(x[idx] for x in w.want(ac.MAIN))
    L = api.lib()
    ad = api.Adaptive(*ac.MAIN)
    G = 8   # guard words before and after each output array: the call is given the address of word G

    def inner(x, words):
        return x[G: G + words]

    def guards_hold(x, words, fill):
        return (x[:G] == fill).all() and (x[G + words:] == fill).all() and len(x) == words + 2 * G
    out = np.full(3 * count + 2 * G, -3.5, "<f4")
    spp = np.full(count + 2 * G, 0xC3C3C3C3, "<u4")
    m2 = np.full(count + 2 * G, -3.5, "<f4")
    fin = np.full(count + 2 * G, 0xC3C3C3C3, "<u4")
    rays, seeds = np.ascontiguousarray(c.rays), np.ascontiguousarray(c.seeds)
    assert L.ort_radiance_adaptive(w.scene.handle, rays.ctypes.data, seeds.ctypes.data, count, api.C.byref(ad), ac.RR, out.ctypes.data + 4 * G,
                                   spp.ctypes.data + 4 * G, m2.ctypes.data + 4 * G, fin.ctypes.data + 4 * G, 0, None) == api.OK
    ac.assert_same((inner(out, 3 * count).reshape(-1, 3), inner(spp, count), inner(m2, count), inner(fin, count)), want, "host form, %d rays" % count)
    assert guards_hold(out, 3 * count, np.float32(-3.5)) and guards_hold(spp, count, 0xC3C3C3C3)
    assert guards_hold(m2, count, np.float32(-3.5)) and guards_hold(fin, count, 0xC3C3C3C3)
    # the device form: the same guards at both ends of each tensor
    import torch
    dev = torch.device("cuda", 0)
    d_rays = torch.from_numpy(rays).to(dev)
    d_seeds = torch.from_numpy(seeds.view("<i4")).to(dev)
    d_out = torch.full((3 * count + 2 * G,), -3.5, dtype=torch.float32, device=dev)
    d_spp = torch.full((count + 2 * G,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
    d_m2 = torch.full((count + 2 * G,), -3.5, dtype=torch.float32, device=dev)
    d_fin = torch.full((count + 2 * G,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
    st = w.scene.radiance_adaptive_device(d_rays.data_ptr(), d_seeds.data_ptr(), count, *ac.MAIN[:2], ac.MAIN.tolerance, ac.MAIN.floor,
                                          ac.MAIN.check_every, ac.RR, d_out.data_ptr() + 4 * G, d_spp.data_ptr() + 4 * G, d_m2.data_ptr() + 4 * G,
                                          d_fin.data_ptr() + 4 * G, want_stats=True)
    assert st["kernel_ms"] > 0
    h = [t.cpu().numpy() for t in (d_out, d_spp, d_m2, d_fin)]
    ac.assert_same((inner(h[0], 3 * count).reshape(-1, 3), inner(h[1], count).view("<u4"), inner(h[2], count), inner(h[3], count).view("<u4")), want,
                   "device form, %d rays" % count)
    assert guards_hold(h[0], 3 * count, np.float32(-3.5)) and guards_hold(h[1], count, 0x3C3C3C3C)
    assert guards_hold(h[2], count, np.float32(-3.5)) and guards_hold(h[3], count, 0x3C3C3C3C)


@pytest.mark.parametrize("skip", ["spp", "m2", "states"])
def test_null_optional_outputs(api, world, skip):
    """each optional output passed as NULL in turn, both forms: the others are the rule's, and nothing is written for it"""
    w = world("c2_analytic")
    c, want = w.cases, w.want(ac.MAIN)
    got, st = torch_run(w.scene, c, ac.MAIN, skip=(skip,))
    assert st is None
    k = {"spp": 1, "m2": 2, "states": 3}[skip]
    filler = np.float32(-7.0) if skip == "m2" else 0x5A5A5A5A
    assert (got[k] == filler).all()
    ac.assert_same(tuple(None if i == k else g for i, g in enumerate(got)), want, "device form without " + skip)
    n = len(c.rays)
    out, spp, m2, fin = np.zeros((n, 3), "<f4"), np.zeros(n, "<u4"), np.zeros(n, "<f4"), np.zeros(n, "<u4")
    ptr = {"spp": spp.ctypes.data, "m2": m2.ctypes.data, "states": fin.ctypes.data}
    ptr[skip] = None
    rays, seeds = np.ascontiguousarray(c.rays), np.ascontiguousarray(c.seeds)
    assert api.lib().ort_radiance_adaptive(w.scene.handle, rays.ctypes.data, seeds.ctypes.data, n, api.C.byref(api.Adaptive(*ac.MAIN)), ac.RR,
                                           out.ctypes.data, ptr["spp"], ptr["m2"], ptr["states"], 0, None) == api.OK
    got = (out, spp, m2, fin)
    assert not got[k].any()
    ac.assert_same(tuple(None if i == k else g for i, g in enumerate(got)), want, "host form without " + skip)


# ---- 4. rays outside the domain ------------------------------------------------------------------------------------------------------------
def test_bad_rays_leave_their_neighbours_alone(world):
    w = world("glass_room")
    good = np.flatnonzero(w.cases.ok)[:128]
    c = w.cases.take(good)
    want = [x[good].copy() for x in w.want(ac.MAIN)]
    rays, seeds = c.rays.copy(), c.seeds.copy()
    bad = np.arange(2, len(good), 5)   # every fifth ray of two waves, seeds 0 among them
    lo, hi = rc.origin_box(w.scene.flatten(1, 1))
    rays[bad] = rc.out_of_domain(np.random.default_rng(9), lo, hi, len(bad))
    seeds[bad[::2]] = 0
    want[0][bad], want[1][bad], want[2][bad], want[3][bad] = np.nan, 0, 0, seeds[bad]
    got, st = run(w.scene, rc.Cases(rays, seeds, c.cams, c.ok), ac.MAIN, counters=True)
    ac.assert_same(got, want, "bad rays among good ones")
    assert st["paths"] == int(want[1].sum()) and (want[1] > 4).any()


# ---- 5. order, slicing, batches, the exact walk ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c2_analytic", "c3_bunny_room", "tables_mats_over"])
def test_independent_of_order_cut_batches_and_walk(world, monkeypatch, name):
    w = world(name)
    c, want = w.cases, w.want(ac.MAIN)
    n = len(c.rays)
    perm = np.random.default_rng(3).permutation(n)
    got, _ = run(w.scene, c.take(perm), ac.MAIN)
    ac.assert_same(got, tuple(x[perm] for x in want), name + " permuted")
    for part in (slice(0, n // 3), slice(n // 3, n)):
        got, _ = run(w.scene, c.take(part), ac.MAIN)
        ac.assert_same(got, tuple(x[part] for x in want), name + " part")
    for batch in ("0", "7", "128"):
        monkeypatch.setenv("ORT_JOB_BATCH", batch)
        got, _ = run(w.scene, c, ac.MAIN)
        ac.assert_same(got, want, name + " ORT_JOB_BATCH=" + batch)
    monkeypatch.delenv("ORT_JOB_BATCH")
    _, st_fast = run(w.scene, c, ac.MAIN, counters=True)
    monkeypatch.setenv("ORT_DEBUG_FORCE_FALLBACK", "0")
    got, st = run(w.scene, c, ac.MAIN, counters=True)
    monkeypatch.delenv("ORT_DEBUG_FORCE_FALLBACK")
    ac.assert_same(got, want, name + " every ray re-cast exactly")
    assert st["fallback_rays"] == st["rays"] == st_fast["rays"] > st_fast["fallback_rays"]
    assert st["paths"] == st_fast["paths"] == int(want[1].sum())


# ---- 6. the device form; counters ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["testscene", "c3_bunny_room"])
def test_device_form_on_a_stream_and_counters(world, name):
    w = world(name)
    c = w.cases
    for ad, rr in ((ac.MAIN, 0.8), (ac.EVERY, 0.0)):
        got, st = torch_run(w.scene, c, ad, rr)          # stats == NULL: enqueued, then synchronised
        assert st is None
        ac.assert_same(got, w.want(ad, rr), "%s device form %r rr %g" % (name, ad, rr))
    got, st = torch_run(w.scene, c, ac.MAIN, counters=True, want_stats=True)
    ac.assert_same(got, w.want(ac.MAIN), name + " device form with counters")
    assert st["paths"] == int(got[1].sum()) and st["paths"] > 4 * int(c.ok.sum())
    assert st["rays"] >= st["paths"] and st["node_tests"] > 0 and st["kernel_ms"] > 0
    _, st_host = run(w.scene, c, ac.MAIN, counters=True)
    assert {k: st_host[k] for k in ("paths", "rays", "node_tests", "tri_tests", "analytic_tests")} == \
           {k: st[k] for k in ("paths", "rays", "node_tests", "tri_tests", "analytic_tests")}


# ---- 7. every kernel of the family ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c3_bunny_room", "glass_room"])
def test_every_kernel_of_the_family(world, monkeypatch, name):
    """radiance_adaptive_rays<counters, diffuse, tabs>, forced as tests/test_gpu_radiance.py forces radiance_rays'.  One answer."""
    w = world(name)
    c, want = w.cases, w.want(ac.MAIN)
    for env in ({}, {"ORT_LDS_TABLES": "0"}, {"ORT_KERNEL": "general"}, {"ORT_KERNEL": "general", "ORT_LDS_TABLES": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for counters in (False, True):
            got, st = run(w.scene, c, ac.MAIN, counters=counters)
            ac.assert_same(got, want, "%s %s counters=%s" % (name, env, counters))
            assert st["paths"] == (int(want[1].sum()) if counters else 0)
        for k in env:
            monkeypatch.delenv(k)


# ---- 8. the host form across a staging slice ------------------------------------------------------------------------------------------------------
def test_host_form_crosses_a_staging_slice(world):
    """the host form stages through per-scene buffers in slices of 2^20 rays: 2^20 + 65 rays are the device form's answers for the
    4096 distinct rays they repeat (min 2, max 3, a check after the second sample).  rr is 0.8, as everywhere else: at rr 0 a
    sample is the first hit's emission alone, the same every time, and every ray stops at 2; with bounces about one in nine of
    these rays sees light in only one of its first two samples and goes on to a third (counted with the oracle)"""
    w = world("c2_analytic")
    rng = np.random.default_rng(77)
    lo, hi = rc.origin_box(w.scene.flatten(1, 1))
    cams = np.concatenate([rc.inside(rng, lo, hi, 2048), rc.at_lights(rng, w.scene.flatten(1, 1), lo, hi, 2048)])
    base = np.array([np.concatenate(rc.pinhole(p, z)) for p, z in cams], "<f4")
    seeds = rng.integers(0, 1 << 32, len(base), dtype=np.uint64).astype("<u4")
    ad = Adaptive(2, 3, 1, 0.3, 0.05)
    cb = rc.Cases(base, seeds, cams, np.ones(len(base), bool))
    ref, _ = torch_run(w.scene, cb, ad, ac.RR)
    some = np.arange(0, 4096, 64)
    ac.assert_same(tuple(x[some] for x in ref), ac.expected(w.osc, cb.take(some), ad, ac.RR), "every 64th of the base rays")
    assert (ref[1] == 2).any() and (ref[1] == 3).any()
    n = (1 << 20) + 65
    idx = np.arange(n) % len(base)
    got, st = run(w.scene, rc.Cases(base[idx], seeds[idx], None, None), ad, ac.RR, counters=True)
    for g, r in zip(got, ref):
        assert g.tobytes() == r[idx].tobytes()
    assert st["paths"] == int(ref[1][idx].astype(np.int64).sum())   # the counters of both slices
