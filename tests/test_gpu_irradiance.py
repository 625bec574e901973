"""Irradiance queries on the device (ort_irradiance, ort_irradiance_adaptive and their device forms; kernels irradiance_points,
irradiance_adaptive_points): cosine-weighted hemisphere gathers at points, held against what exists (tests/irradiance_cases.py) --
identity I2 (rr = 0: the oracle's closed form), identity I1 (rr = 0.8: a chain of ort_radiance calls at spp = 1 along directions
composed from the oracle), adaptive_cases.cut over that chain.  All bits of every output; NaN outputs compare by position."""
import ctypes
import zlib

import numpy as np
import pytest

import adaptive_cases as ac
import irradiance_cases as ic
import radiance_cases as rc
import ref_io
import table_scenes
from adaptive_cases import Adaptive

pytestmark = pytest.mark.gpu

# points per scene; c2_analytic: all lobes, boxes in the tree; c3_bunny_room: a mesh; tables_mats_over: the table-less kernels
SCENES = {"testscene": 256, "c2_analytic": 256, "glass_room": 192, "c3_bunny_room": 128, "tables_mats_over": 128}
ADAPTIVE_SCENES = ("testscene", "c2_analytic")
RR = ic.RR
_worlds = {}


class World:
    pass


@pytest.fixture()
def world(api, oracle, gpu_scene, tmp_path_factory):
    """name -> the uploaded scene, its points, the oracle's closed form of 8 samples at rr = 0 and (filled on demand) the chain of
    ort_radiance calls at rr = 0.8; computed once"""
    def get(name):
        if name not in _worlds:
            w = World()
            if name.startswith("tables_"):
                scene, _, csg = table_scenes.build(api, name[len("tables_"):], tmp_path_factory.mktemp(name))
                w.scene = scene.commit().upload(0)
            else:
                w.scene, csg = gpu_scene(name), True
            w.name = name
            w.flat = w.scene.flatten(1, 1)
            w.osc = oracle.OracleScene(w.flat, with_reference_csg=csg)
            w.pts = ic.point_set(name, w.flat, w.osc, SCENES[name])
            w.closed = ic.chain_closed_form(oracle, w.osc, w.flat, w.pts, 8)
            w.chain = None
            _worlds[name] = w
        return _worlds[name]
    return get


def radiance_chain(w, oracle):
    """identity I1's reference: 8 chained ort_radiance calls at spp = 1 (17 on the scenes of the adaptive tests)"""
    if w.chain is None:
        def one(rays, seeds):
            rgb, fin, _ = w.scene.radiance(rays, seeds, 1, RR, want_states=True)
            return rgb, fin
        w.chain = ic.chain_by_radiance(oracle, w.pts, 17 if w.name in ADAPTIVE_SCENES else 8, one)
    return w.chain


def torch_irradiance(scene, points, seeds, spp, rr, ad=None, skip=(), counters=False, want_stats=False):
    """the device forms, with torch tensors on a non-default stream; without stats the call does not wait: synchronise.
    -> ((rgb, spp, m2, states), stats); the planes in `skip` are not passed and keep their fill"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(points)
    d_pts = torch.from_numpy(np.ascontiguousarray(points, "<f4")).to(dev)
    d_seeds = torch.from_numpy(np.ascontiguousarray(seeds, "<u4").view("<i4")).to(dev)
    d_out = torch.full((n, 3), -7.0, dtype=torch.float32, device=dev)
    d_spp = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_m2 = torch.full((n,), -7.0, dtype=torch.float32, device=dev)
    d_fin = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    ptr = lambda t, what: 0 if what in skip else t.data_ptr()
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        if ad is None:
            st = scene.irradiance_device(d_pts.data_ptr(), d_seeds.data_ptr(), n, spp, rr, d_out.data_ptr(), ptr(d_fin, "states"),
                                         stream=stream.cuda_stream, counters=counters, want_stats=want_stats)
        else:
            st = scene.irradiance_adaptive_device(d_pts.data_ptr(), d_seeds.data_ptr(), n, ad.min_spp, ad.max_spp, ad.tolerance, ad.floor,
                                                  ad.check_every, rr, d_out.data_ptr(), ptr(d_spp, "spp"), ptr(d_m2, "m2"), ptr(d_fin, "states"),
                                                  stream=stream.cuda_stream, counters=counters, want_stats=want_stats)
    stream.synchronize()
    return (d_out.cpu().numpy(), d_spp.cpu().numpy().view("<u4"), d_m2.cpu().numpy(), d_fin.cpu().numpy().view("<u4")), st


# ---- 1. identity I2: without bounces, the oracle's closed form -----------------------------------------------------------------
@pytest.mark.parametrize("spp", [1, 8])
@pytest.mark.parametrize("name", list(SCENES))
def test_without_bounces_is_the_oracles_closed_form(world, name, spp):
    w = world(name)
    rgb, fin, st = w.scene.irradiance(w.pts.points, w.pts.seeds, spp, 0.0, want_states=True)
    rc.assert_same(rgb, fin, *ic.expected_from(w.closed, w.pts, spp), "%s rr 0 spp %d, host form" % (name, spp))
    assert st["kernel_ms"] > 0 and st["paths"] == 0   # counters only on request
    if spp == 8:
        lit, mixed = ic.lit_shares(w.closed)
        assert lit >= 0.10 and mixed >= 0.10, "the point set is vacuous: lit %.3f, mixed %.3f" % (lit, mixed)


# ---- 2. identity I1: a chain of ort_radiance samples ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_is_a_chain_of_radiance_samples(world, oracle, name):
    w = world(name)
    chain = radiance_chain(w, oracle)
    want = ic.expected_from(chain, w.pts, 8)
    assert (want[0][w.pts.ok] != 0).any(axis=1).mean() >= 0.10
    rgb, fin, _ = w.scene.irradiance(w.pts.points, w.pts.seeds, 8, RR, want_states=True)
    rc.assert_same(rgb, fin, *want, name + " rr 0.8 spp 8, host form")
    got, st = torch_irradiance(w.scene, w.pts.points, w.pts.seeds, 8, RR)
    assert st is None
    rc.assert_same(got[0], got[3], *want, name + " rr 0.8 spp 8, device form on a stream")
    assert (got[1] == 0x5A5A5A5A).all() and (got[2] == np.float32(-7.0)).all()   # the uniform form has no such planes


# ---- 3. the adaptive form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ad", ic.SETS, ids=["main", "every"])
@pytest.mark.parametrize("name", ADAPTIVE_SCENES)
def test_adaptive_is_the_rule_over_the_chain(api, world, oracle, name, ad):
    w = world(name)
    p = w.pts
    want = ic.expected_adaptive(radiance_chain(w, oracle), p, ad)
    assert len(set(want[1][p.ok])) >= 3   # points stop at several counts
    rgb, spp, m2, fin, st = w.scene.irradiance_adaptive(p.points, p.seeds, ad.min_spp, ad.max_spp, ad.tolerance, ad.floor, ad.check_every, RR,
                                                        want_states=True, counters=True)
    ac.assert_same((rgb, spp, m2, fin), want, "%s %r, host form" % (name, ad))
    assert st["paths"] == int(want[1].sum())
    got, _ = torch_irradiance(w.scene, p.points, p.seeds, 0, RR, ad=ad)
    ac.assert_same(got, want, "%s %r, device form on a stream" % (name, ad))
    # each optional plane NULL in turn: the others are unchanged, and nothing is written where nothing was asked for
    pts, seeds = np.ascontiguousarray(p.points), np.ascontiguousarray(p.seeds)
    n = len(pts)
    for k, what in enumerate(("spp", "m2", "states")):
        host = [np.zeros((n, 3), "<f4"), np.full(n, 0xC3C3C3C3, "<u4"), np.full(n, -3.5, "<f4"), np.full(n, 0xC3C3C3C3, "<u4")]
        ptrs = [a.ctypes.data if j != k + 1 else None for j, a in enumerate(host)]
        assert api.lib().ort_irradiance_adaptive(w.scene.handle, pts.ctypes.data, seeds.ctypes.data, n, ctypes.byref(api.Adaptive(*ad)), RR, *ptrs,
                                                 0, None) == api.OK
        ac.assert_same(tuple(None if j == k + 1 else a for j, a in enumerate(host)), want, "%s %r, host form without %s" % (name, ad, what))
        assert (host[k + 1] == (np.float32(-3.5) if what == "m2" else 0xC3C3C3C3)).all()
        got, _ = torch_irradiance(w.scene, pts, seeds, 0, RR, ad=ad, skip=(what,))
        ac.assert_same(tuple(None if j == k + 1 else a for j, a in enumerate(got)), want, "%s %r, device form without %s" % (name, ad, what))
        assert (got[k + 1] == (np.float32(-7.0) if what == "m2" else 0x5A5A5A5A)).all()


@pytest.mark.parametrize("name", ADAPTIVE_SCENES)
def test_adaptive_without_checks_is_the_uniform_query(world, name):
    """min_spp == max_spp == n: ort_irradiance's bits at spp = n"""
    w = world(name)
    p = w.pts
    for n in (2, 8):
        rgb, fin, _ = w.scene.irradiance(p.points, p.seeds, n, RR, want_states=True)
        a_rgb, a_spp, a_m2, a_fin, _ = w.scene.irradiance_adaptive(p.points, p.seeds, n, n, 0.3, 0.05, 3, RR, want_states=True)
        rc.assert_same(a_rgb, a_fin, rgb, fin, "%s min = max = %d" % (name, n))
        assert (a_spp[p.ok] == n).all() and (a_spp[~p.ok] == 0).all() and (a_m2[~p.ok] == 0).all()
        assert ((a_m2[p.ok] > 0) == (rgb[p.ok] != 0).any(axis=1)).all()


# ---- 4. the hemisphere draw as the kernels compose it ------------------------------------------------------------------------------
def test_op20_on_the_device_is_the_oracles_composition(api, world, oracle):
    rng = np.random.default_rng(20)
    p = world("c2_analytic").pts
    normals = np.concatenate([rc._units(rng, 256), p.points[p.ok, 3:6]]).astype("<f4")
    seeds = np.concatenate([rng.integers(0, 1 << 32, 256, dtype=np.uint64).astype("<u4"), p.seeds[p.ok]])
    assert (seeds == 0).any() and (seeds == 0xFFFFFFFF).any() and (seeds == rc.unstep(0xFFFFFFFF)).any()
    got = api.unit_eval_device(ref_io.make_unit_records(20, ic.op20_rows(seeds, normals)))
    ic.assert_op20(got, ic.op20_expected(oracle, seeds, normals), "op 20 on the device")


# ---- 5. counts and guard words ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 63, 65, 513])
def test_counts_and_guard_words(api, world, count):
    """rr = 0, against the closed form: guard words after every output array of the host forms, final_states == NULL, and the
    device forms writing no further than count"""
    w = world("testscene")
    idx = np.arange(count) % len(w.pts.points)
    p = w.pts.take(idx)
    closed = {j: w.closed[int(i)] for j, i in enumerate(idx) if int(i) in w.closed}
    want_rgb, want_fin = ic.expected_from(closed, p, 8)
    ad = Adaptive(2, 8, 2, 0.6, 0.05)
    want_ad = ic.expected_adaptive(closed, p, ad)
    L = api.lib()
    pts, seeds = np.ascontiguousarray(p.points), np.ascontiguousarray(p.seeds)
    out, fin = np.full(3 * count + 8, -3.5, "<f4"), np.full(count + 8, 0xC3C3C3C3, "<u4")
    assert L.ort_irradiance(w.scene.handle, pts.ctypes.data, seeds.ctypes.data, count, 8, 0.0, out.ctypes.data, fin.ctypes.data, 0, None) == api.OK
    rc.assert_same(out[: 3 * count].reshape(-1, 3), fin[:count], want_rgb, want_fin, "host form, %d points" % count)
    assert (out[3 * count:] == np.float32(-3.5)).all() and (fin[count:] == 0xC3C3C3C3).all()
    out[:] = -3.5   # final_states == NULL
    assert L.ort_irradiance(w.scene.handle, pts.ctypes.data, seeds.ctypes.data, count, 8, 0.0, out.ctypes.data, None, 0, None) == api.OK
    rc.assert_same(out[: 3 * count].reshape(-1, 3), None, want_rgb, None, "host form without states, %d points" % count)
    assert (out[3 * count:] == np.float32(-3.5)).all()
    # the adaptive host form: four arrays, four guards
    out[:] = -3.5
    fin[:] = 0xC3C3C3C3
    spp, m2 = np.full(count + 8, 0xC3C3C3C3, "<u4"), np.full(count + 8, -3.5, "<f4")
    assert L.ort_irradiance_adaptive(w.scene.handle, pts.ctypes.data, seeds.ctypes.data, count, ctypes.byref(api.Adaptive(*ad)), 0.0, out.ctypes.data,
                                     spp.ctypes.data, m2.ctypes.data, fin.ctypes.data, 0, None) == api.OK
    ac.assert_same((out[: 3 * count].reshape(-1, 3), spp[:count], m2[:count], fin[:count]), want_ad, "adaptive host form, %d points" % count)
    assert (out[3 * count:] == np.float32(-3.5)).all() and (fin[count:] == 0xC3C3C3C3).all()
    assert (spp[count:] == 0xC3C3C3C3).all() and (m2[count:] == np.float32(-3.5)).all()
    # the device forms: the tensors' own ends are the guards (the allocations are larger than what the call may write)
    import torch
    dev = torch.device("cuda", 0)
    d_pts, d_seeds = torch.from_numpy(pts).to(dev), torch.from_numpy(seeds.view("<i4")).to(dev)
    d_out = torch.full((3 * count + 8,), -3.5, dtype=torch.float32, device=dev)
    d_fin = torch.full((count + 8,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
    st = w.scene.irradiance_device(d_pts.data_ptr(), d_seeds.data_ptr(), count, 8, 0.0, d_out.data_ptr(), d_fin.data_ptr(), want_stats=True)
    assert st["kernel_ms"] > 0
    h_out, h_fin = d_out.cpu().numpy(), d_fin.cpu().numpy().view("<u4")
    rc.assert_same(h_out[: 3 * count].reshape(-1, 3), h_fin[:count], want_rgb, want_fin, "device form, %d points" % count)
    assert (h_out[3 * count:] == np.float32(-3.5)).all() and (h_fin[count:] == 0x3C3C3C3C).all()
    d_out.fill_(-3.5)
    d_fin.fill_(0x3C3C3C3C)
    d_spp = torch.full((count + 8,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
    d_m2 = torch.full((count + 8,), -3.5, dtype=torch.float32, device=dev)
    w.scene.irradiance_adaptive_device(d_pts.data_ptr(), d_seeds.data_ptr(), count, ad.min_spp, ad.max_spp, ad.tolerance, ad.floor, ad.check_every, 0.0,
                                       d_out.data_ptr(), d_spp.data_ptr(), d_m2.data_ptr(), d_fin.data_ptr(), want_stats=True)
    h = d_out.cpu().numpy(), d_spp.cpu().numpy().view("<u4"), d_m2.cpu().numpy(), d_fin.cpu().numpy().view("<u4")
    ac.assert_same((h[0][: 3 * count].reshape(-1, 3), h[1][:count], h[2][:count], h[3][:count]), want_ad, "adaptive device form, %d points" % count)
    assert (h[0][3 * count:] == np.float32(-3.5)).all() and (h[1][count:] == 0x3C3C3C3C).all()
    assert (h[2][count:] == np.float32(-3.5)).all() and (h[3][count:] == 0x3C3C3C3C).all()


# ---- 6. counters ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["testscene", "c3_bunny_room"])
def test_counters_count_the_samples(world, name):
    w = world(name)
    p = w.pts
    inside = int(p.ok.sum())
    for spp in (1, 8):
        _, st = w.scene.irradiance(p.points, p.seeds, spp, RR, counters=True)
        assert st["paths"] == inside * spp
        assert st["rays"] >= st["paths"] and st["node_tests"] > 0 and st["kernel_ms"] > 0
    got, st = torch_irradiance(w.scene, p.points, p.seeds, 8, RR, counters=True, want_stats=True)
    assert st["paths"] == inside * 8
    ad = ic.MAIN
    rgb, spp, m2, st = w.scene.irradiance_adaptive(p.points, p.seeds, ad.min_spp, ad.max_spp, ad.tolerance, ad.floor, ad.check_every, RR, counters=True)
    assert st["paths"] == int(spp.sum()) and inside * ad.min_spp < st["paths"] < inside * ad.max_spp
    got, st = torch_irradiance(w.scene, p.points, p.seeds, 0, RR, ad=ad, counters=True, want_stats=True)
    assert st["paths"] == int(got[1].sum()) == int(spp.sum())


# ---- 7. across a staging slice ---------------------------------------------------------------------------------------------------------
SLICE_COUNT = (1 << 20) + 257   # kRadianceSlice of offline_raytracer_amd/csrc/ort_kernels.hip and a ragged remainder
BASE = 4096


def slice_base(w):
    """-> points (BASE, 6), seeds (BASE,): half near a light, the rest anywhere inside the box with any normal, and 16 points
    outside the domain (they answer NaN)"""
    rng = np.random.default_rng(zlib.crc32(b"slice boundary irradiance"))
    lo, hi = rc.origin_box(w.flat)
    k = (BASE - 16) // 2
    anywhere = np.concatenate([rng.uniform(lo, hi, size=(BASE - 16 - k, 3)), rc._units(rng, BASE - 16 - k)], axis=1)
    pts = np.concatenate([ic.near_lights(rng, w.flat, lo, hi, k), anywhere, ic.out_of_domain(rng, lo, hi, 16)]).astype("<f4")
    return pts[rng.permutation(BASE)], rng.integers(0, 1 << 32, BASE, dtype=np.uint64).astype("<u4")


def same_bytes(host, device, what):
    host, device = np.ascontiguousarray(host), np.ascontiguousarray(device)
    assert host.shape == device.shape and host.dtype.itemsize == device.dtype.itemsize, what
    if host.tobytes() != device.tobytes():
        a, b = host.reshape(len(host), -1).view(np.uint8), device.reshape(len(device), -1).view(np.uint8)
        bad = np.flatnonzero((a != b).any(axis=1))
        raise AssertionError("%s: the forms differ for %d of %d points, first %d" % (what, len(bad), len(host), bad[0]))


def test_host_forms_cross_a_staging_slice(world):
    """(1 << 20) + 257 points tiled from 4 096, one sample each (two to four under the rule): the host form, staged in two
    slices, equals the device form's one launch in every output"""
    w = world("c2_analytic")
    pts, seeds = slice_base(w)
    idx = np.arange(SLICE_COUNT) % BASE
    pts, seeds = np.ascontiguousarray(pts[idx]), np.ascontiguousarray(seeds[idx])
    rgb, fin, st = w.scene.irradiance(pts, seeds, 1, RR, want_states=True, counters=True)
    dev, _ = torch_irradiance(w.scene, pts, seeds, 1, RR)
    same_bytes(rgb, dev[0], "rgb")
    same_bytes(fin, dev[3], "final states")
    assert np.isnan(rgb).any() and (rgb > 0).any()
    assert st["paths"] == int((~np.isnan(rgb[:, 0])).sum())   # the counters of both slices
    ad = Adaptive(2, 4, 1, 0.6, 0.05)
    host = w.scene.irradiance_adaptive(pts, seeds, ad.min_spp, ad.max_spp, ad.tolerance, ad.floor, ad.check_every, RR, want_states=True)
    dev, _ = torch_irradiance(w.scene, pts, seeds, 0, RR, ad=ad)
    for h, d, what in zip(host[:4], dev, ("rgb", "spp", "m2", "final states")):
        same_bytes(h, d, "adaptive " + what)
    assert set(np.unique(host[1])) == {0, 2, 3, 4}   # 0: the points outside the domain


# ---- 8. far points: the exact walk --------------------------------------------------------------------------------------------------
def test_far_points_take_the_exact_walk(world):
    """c2_analytic holds quadrics in its tree: every primary sample of a point outside the scene's box is re-cast exactly, and
    its bits are the closed form's"""
    w = world("c2_analytic")
    far = np.flatnonzero(w.pts.far)
    p = w.pts.take(far)
    closed = {j: w.closed[int(i)] for j, i in enumerate(far)}
    rgb, fin, st = w.scene.irradiance(p.points, p.seeds, 8, 0.0, want_states=True, counters=True)
    rc.assert_same(rgb, fin, *ic.expected_from(closed, p, 8), "far points, rr 0 spp 8")
    assert st["fallback_rays"] >= 8 * len(far) > 0 and st["paths"] == 8 * len(far)
    near = np.flatnonzero(w.pts.ok & ~w.pts.far)[:64]
    _, st_near = w.scene.irradiance(w.pts.points[near], w.pts.seeds[near], 8, 0.0, counters=True)
    assert st_near["fallback_rays"] < 8 * len(near)
