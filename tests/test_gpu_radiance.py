"""Radiance queries on the device (ort_radiance / ort_radiance_device, kernels radiance_rays): the path-traced light along a
caller's ray, bit for bit the oracle's pixel of a pinhole camera whose every sample starts at that ray (tests/radiance_cases.py:
how the oracle is driven, and the rays).  All bits of the colours and of the final stream states; NaN outputs compare by
position."""
import ctypes

import numpy as np
import pytest

import radiance_cases as rc
import table_scenes

pytestmark = pytest.mark.gpu

# rays per scene: all generators mixed; the mesh scene costs the oracle most and gets fewest
SCENES = {"testscene": 520, "c2_analytic": 384, "glass_room": 384, "c3_bunny_room": 192, "tables_mats_over": 256}
SPPS = (1, 3)
RRS = (0.8, 0.0)
_worlds = {}


class World:
    pass


@pytest.fixture()
def world(api, oracle, gpu_scene, tmp_path_factory):
    """name -> the uploaded scene, its rays and what the oracle says of them ({rr: {spp: (rgb, states)}}); computed once"""
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
            w.cases = rc.mixed(name, flat, w.osc, SCENES[name])
            w.want = {rr: rc.expected_of(w.osc, w.cases, SPPS, rr) for rr in RRS}
            _worlds[name] = w
        return _worlds[name]
    return get


def torch_radiance(scene, rays, seeds, spp, rr, states=True, counters=False, want_stats=False):
    """the device form, with torch tensors on a non-default stream; without stats the call does not wait: synchronise"""
    import torch
    dev = torch.device("cuda", 0)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays, "<f4")).to(dev)
    d_seeds = torch.from_numpy(np.ascontiguousarray(seeds, "<u4").view("<i4")).to(dev)
    d_out = torch.full((len(rays), 3), -7.0, dtype=torch.float32, device=dev)
    d_fin = torch.full((len(rays),), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        st = scene.radiance_device(d_rays.data_ptr(), d_seeds.data_ptr(), len(rays), spp, rr, d_out.data_ptr(),
                                   d_fin.data_ptr() if states else 0, stream=stream.cuda_stream, counters=counters, want_stats=want_stats)
    stream.synchronize()
    return d_out.cpu().numpy(), d_fin.cpu().numpy().view("<u4"), st


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rr", RRS)
@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("name", list(SCENES))
def test_radiance_is_the_oracles(world, name, spp, rr):
    w = world(name)
    rgb, fin, st = w.scene.radiance(w.cases.rays, w.cases.seeds, spp, rr, want_states=True)
    rc.assert_same(rgb, fin, *w.want[rr][spp], "%s spp %d rr %g, host form" % (name, spp, rr))
    assert st["kernel_ms"] > 0 and st["paths"] == 0   # counters only on request


# ---- 2. the inputs cannot pass on black ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_the_oracles_values_are_not_black(world, name):
    """on the oracle's values (spp 3, rr 0.8 for the light; spp 1, rr 0.8 for the states): at least a tenth of the rays inside
    the domain carry radiance, at least a quarter bounce at their primary hit; every generator is present"""
    w = world(name)
    ok = w.cases.ok
    rgb3, _ = w.want[0.8][3]
    _, fin1 = w.want[0.8][1]
    assert (rgb3[ok] != 0).any(axis=1).mean() >= 0.10
    assert rc.survives_primary(w.cases.seeds, fin1)[ok].mean() >= 0.25
    d = w.cases.rays[ok, 3:6]
    assert ((d == 0).sum(axis=1) == 2).sum() >= ok.sum() // 10          # axis-aligned
    lo, hi = rc.origin_box(w.scene.flatten(1, 1))
    o = w.cases.rays[ok, 0:3]
    assert ((o < lo) | (o > hi)).any(axis=1).sum() >= ok.sum() // 10    # from outside the box
    assert (~ok).sum() == 8 and np.isnan(w.want[0.8][1][0][~ok]).all()


# ---- 3. counts, guard words, slices, no states -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 63, 65, 513])
def test_counts_and_guard_words(api, world, count):
    w = world("testscene")
    c = w.cases.take(np.arange(count))
    want_rgb, want_fin = w.want[0.8][3][0][:count], w.want[0.8][3][1][:count]
    L = api.lib()
    out = np.full(3 * count + 8, -3.5, "<f4")
    fin = np.full(count + 8, 0xC3C3C3C3, "<u4")
    rays, seeds = np.ascontiguousarray(c.rays), np.ascontiguousarray(c.seeds)
    assert L.ort_radiance(w.scene.handle, rays.ctypes.data, seeds.ctypes.data, count, 3, 0.8, out.ctypes.data, fin.ctypes.data, 0, None) == api.OK
    rc.assert_same(out[: 3 * count].reshape(-1, 3), fin[:count], want_rgb, want_fin, "host form, %d rays" % count)
    assert (out[3 * count:] == np.float32(-3.5)).all() and (fin[count:] == 0xC3C3C3C3).all()
    # final_states == NULL
    out[:] = -3.5
    assert L.ort_radiance(w.scene.handle, rays.ctypes.data, seeds.ctypes.data, count, 3, 0.8, out.ctypes.data, None, 0, None) == api.OK
    rc.assert_same(out[: 3 * count].reshape(-1, 3), None, want_rgb, None, "host form without states, %d rays" % count)
    assert (out[3 * count:] == np.float32(-3.5)).all()
    # the device form: the tensors' own ends are the guards (the allocations are larger than what the call may write)
    import torch
    dev = torch.device("cuda", 0)
    d_rays = torch.from_numpy(rays).to(dev)
    d_seeds = torch.from_numpy(seeds.view("<i4")).to(dev)
    d_out = torch.full((3 * count + 8,), -3.5, dtype=torch.float32, device=dev)
    d_fin = torch.full((count + 8,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
    st = w.scene.radiance_device(d_rays.data_ptr(), d_seeds.data_ptr(), count, 3, 0.8, d_out.data_ptr(), d_fin.data_ptr(), want_stats=True)
    assert st["kernel_ms"] > 0
    h_out, h_fin = d_out.cpu().numpy(), d_fin.cpu().numpy().view("<u4")
    rc.assert_same(h_out[: 3 * count].reshape(-1, 3), h_fin[:count], want_rgb, want_fin, "device form, %d rays" % count)
    assert (h_out[3 * count:] == np.float32(-3.5)).all() and (h_fin[count:] == 0x3C3C3C3C).all()


def test_host_form_crosses_a_staging_slice(world):
    """the host form stages through per-scene buffers in slices of 2^20 rays: 2^20 + 65 rays, one sample each, are the device
    form's answers for the 4096 distinct rays they repeat"""
    w = world("c2_analytic")
    rng = np.random.default_rng(77)
    lo, hi = rc.origin_box(w.scene.flatten(1, 1))
    cams = rc.inside(rng, lo, hi, 4096)
    base = np.array([np.concatenate(rc.pinhole(p, z)) for p, z in cams], "<f4")
    seeds = rng.integers(0, 1 << 32, len(base), dtype=np.uint64).astype("<u4")
    ref_rgb, ref_fin, _ = torch_radiance(w.scene, base, seeds, 1, 0.8)
    some = np.arange(0, 4096, 64)
    rc.assert_same(ref_rgb[some], ref_fin[some], *rc.expected(w.osc, cams[some], seeds[some], 1, 0.8), "every 64th of the base rays")
    n = (1 << 20) + 65
    idx = np.arange(n) % len(base)
    rgb, fin, st = w.scene.radiance(base[idx], seeds[idx], 1, 0.8, want_states=True, counters=True)
    assert rgb.view("<u4").tobytes() == ref_rgb[idx].view("<u4").tobytes()
    assert fin.tobytes() == ref_fin[idx].tobytes()
    assert st["paths"] == n   # the counters of both slices


# ---- 4. order, slicing, batches, the exact walk ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c2_analytic", "c3_bunny_room", "tables_mats_over"])
def test_independent_of_order_cut_batches_and_walk(world, monkeypatch, name):
    w = world(name)
    c, (want_rgb, want_fin) = w.cases, w.want[0.8][3]
    n = len(c.rays)
    perm = np.random.default_rng(3).permutation(n)
    rgb, fin, _ = w.scene.radiance(c.rays[perm], c.seeds[perm], 3, 0.8, want_states=True)
    rc.assert_same(rgb, fin, want_rgb[perm], want_fin[perm], name + " permuted")
    for part in (slice(0, n // 2), slice(n // 2, n)):
        rgb, fin, _ = w.scene.radiance(c.rays[part], c.seeds[part], 3, 0.8, want_states=True)
        rc.assert_same(rgb, fin, want_rgb[part], want_fin[part], name + " half")
    for batch in ("0", "7", "128"):
        monkeypatch.setenv("ORT_JOB_BATCH", batch)
        rgb, fin, _ = w.scene.radiance(c.rays, c.seeds, 3, 0.8, want_states=True)
        rc.assert_same(rgb, fin, want_rgb, want_fin, name + " ORT_JOB_BATCH=" + batch)
    monkeypatch.delenv("ORT_JOB_BATCH")
    _, st_fast = w.scene.radiance(c.rays, c.seeds, 3, 0.8, counters=True)
    monkeypatch.setenv("ORT_DEBUG_FORCE_FALLBACK", "0")
    rgb, fin, st = w.scene.radiance(c.rays, c.seeds, 3, 0.8, want_states=True, counters=True)
    monkeypatch.delenv("ORT_DEBUG_FORCE_FALLBACK")
    rc.assert_same(rgb, fin, want_rgb, want_fin, name + " every ray re-cast exactly")
    assert st["fallback_rays"] == st["rays"] == st_fast["rays"] > st_fast["fallback_rays"]
    if name == "c2_analytic":   # boxes and quadrics in its tree: the axis-aligned and the far primary rays took the walk unasked
        assert st_fast["fallback_rays"] > 0


# ---- 5. seed 0, rays outside the domain ----------------------------------------------------------------------------------------------------
def test_seed_zero_is_seed_one_and_bad_rays_leave_their_neighbours_alone(world):
    w = world("glass_room")
    good = np.flatnonzero(w.cases.ok)[:128]
    c = w.cases.take(good)
    ones = np.ones(len(good), "<u4")
    rgb1, fin1, _ = w.scene.radiance(c.rays, ones, 3, 0.8, want_states=True)
    rc.assert_same(rgb1, fin1, *rc.expected(w.osc, c.cams, ones, 3, 0.8), "seed 1")
    rgb0, fin0, _ = w.scene.radiance(c.rays, np.zeros(len(good), "<u4"), 3, 0.8, want_states=True)
    rc.assert_same(rgb0, fin0, rgb1, fin1, "seed 0 against seed 1")
    assert (rgb1 != 0).any()
    # every fifth ray of two waves replaced by one outside the domain, seeds 0 among them
    want_rgb, want_fin = w.want[0.8][3][0][good].copy(), w.want[0.8][3][1][good].copy()
    rays, seeds = c.rays.copy(), c.seeds.copy()
    bad = np.arange(2, len(good), 5)
    lo, hi = rc.origin_box(w.scene.flatten(1, 1))
    rays[bad] = rc.out_of_domain(np.random.default_rng(9), lo, hi, len(bad))
    seeds[bad[::2]] = 0
    want_rgb[bad], want_fin[bad] = np.nan, seeds[bad]
    rgb, fin, st = w.scene.radiance(rays, seeds, 3, 0.8, want_states=True, counters=True)
    rc.assert_same(rgb, fin, want_rgb, want_fin, "bad rays among good ones")
    assert st["paths"] == 3 * (len(good) - len(bad))


# ---- 6. the device form; counters -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["testscene", "c3_bunny_room"])
def test_device_form_on_a_stream_and_counters(world, name):
    w = world(name)
    c = w.cases
    for spp, rr in ((3, 0.8), (1, 0.0)):
        rgb, fin, st = torch_radiance(w.scene, c.rays, c.seeds, spp, rr)          # stats == NULL: enqueued, then synchronised
        assert st is None
        rc.assert_same(rgb, fin, *w.want[rr][spp], "%s device form spp %d rr %g" % (name, spp, rr))
    rgb, fin, _ = torch_radiance(w.scene, c.rays, c.seeds, 3, 0.8, states=False)
    rc.assert_same(rgb, None, w.want[0.8][3][0], None, name + " device form without states")
    assert (fin == 0x5A5A5A5A).all()
    rgb, fin, st = torch_radiance(w.scene, c.rays, c.seeds, 3, 0.8, counters=True, want_stats=True)
    rc.assert_same(rgb, fin, *w.want[0.8][3], name + " device form with counters")
    assert st["paths"] == 3 * int(c.ok.sum())
    assert st["rays"] >= st["paths"] and st["node_tests"] > 0 and st["analytic_tests"] > 0 and st["kernel_ms"] > 0
    _, st_host = w.scene.radiance(c.rays, c.seeds, 3, 0.8, counters=True)
    assert {k: st_host[k] for k in ("paths", "rays", "node_tests", "tri_tests", "analytic_tests")} == \
           {k: st[k] for k in ("paths", "rays", "node_tests", "tri_tests", "analytic_tests")}


# ---- every kernel of the family ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c3_bunny_room", "glass_room"])
def test_every_kernel_of_the_family(world, monkeypatch, name):
    """radiance_rays<counters, diffuse, tabs>: the bunny room has no specular or transmissive material (diffuse flavour), the
    glass room has (all lobes; ORT_KERNEL=general gives the bunny room that flavour too); ORT_LDS_TABLES=0 reads the tables
    from HBM; counters on request.  One answer."""
    w = world(name)
    c, (want_rgb, want_fin) = w.cases, w.want[0.8][3]
    for env in ({}, {"ORT_LDS_TABLES": "0"}, {"ORT_KERNEL": "general"}, {"ORT_KERNEL": "general", "ORT_LDS_TABLES": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for counters in (False, True):
            rgb, fin, st = w.scene.radiance(c.rays, c.seeds, 3, 0.8, want_states=True, counters=counters)
            rc.assert_same(rgb, fin, want_rgb, want_fin, "%s %s counters=%s" % (name, env, counters))
            assert st["paths"] == (3 * int(c.ok.sum()) if counters else 0)
        for k in env:
            monkeypatch.delenv(k)
