"""Ambient-occlusion queries on the device (ort_ambient_occlusion and its device form; kernels ao_points): hemisphere
visibility gathers at points, held against the oracle alone (tests/ao_cases.py) -- irradiance_cases.directions for d_k and the
states, OracleScene.raycast for t and mat, occluded_cases.expected for the bit, a numpy float32 sum for the bent sum.  All bits of
every output; NaN outputs compare by position."""
import zlib

import numpy as np
import pytest

import ao_cases as ao
import irradiance_cases as ic
import radiance_cases as rc
from test_gpu_tables import table_scene  # noqa: F401 -- the fixture: pro_over committed under ORT_ANALYTIC_PROLOGUE=40

pytestmark = pytest.mark.gpu

SCENES = {"testscene": 256, "c2_analytic": 256, "glass_room": 192, "c3_bunny_room": 128}
_worlds = {}


@pytest.fixture()
def world(oracle, gpu_scene):
    """name -> the uploaded scene, its points, radii and the oracle's table of 8 samples per point; computed once"""
    def get(name):
        if name not in _worlds:
            scene = gpu_scene(name)
            flat = scene.flatten(1, 1)
            _worlds[name] = ao.build(name, scene, flat, oracle.OracleScene(flat, with_reference_csg=True), oracle, SCENES[name])
        return _worlds[name]
    return get


def host_form(scene, points, seeds, radius, spp, counters=False):
    out, bent, fin, st = scene.ambient_occlusion(points, seeds, spp, radius=radius, want_bent=True, want_states=True, counters=counters)
    return (out, bent, fin), st


def torch_form(scene, points, seeds, radius, spp, skip=(), counters=False, want_stats=False, pad=0):
    """the device form, with torch tensors on a non-default stream; without stats the call does not wait: synchronise.
    -> ((open, bent, states), stats); the outputs in `skip` are not passed and keep their fill; pad: guard words after each output"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(points)
    d_pts = torch.from_numpy(np.ascontiguousarray(points, "<f4")).to(dev)
    d_seeds = torch.from_numpy(np.ascontiguousarray(seeds, "<u4").view("<i4")).to(dev)
    d_rad = torch.from_numpy(np.ascontiguousarray(radius, "<f4")).to(dev) if radius is not None else None
    d_open = torch.full((n + pad,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_bent = torch.full((3 * (n + pad),), -7.0, dtype=torch.float32, device=dev)
    d_fin = torch.full((n + pad,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        st = scene.ambient_occlusion_device(d_pts.data_ptr(), d_seeds.data_ptr(), d_rad.data_ptr() if d_rad is not None else None, n, spp,
                                            d_open.data_ptr(), 0 if "bent" in skip else d_bent.data_ptr(), 0 if "states" in skip else d_fin.data_ptr(),
                                            stream=stream.cuda_stream, counters=counters, want_stats=want_stats)
    stream.synchronize()
    return (d_open.cpu().numpy().view("<u4"), d_bent.cpu().numpy().reshape(-1, 3), d_fin.cpu().numpy().view("<u4")), st


# ---- 1. against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", [1, 8])
@pytest.mark.parametrize("name", list(SCENES))
def test_is_the_oracles_answer(world, name, spp):
    """the radius array (R, +inf, NaN, 0, -1, FLT_MAX, 0.4 x the diagonal, the points' own hit distances and their neighbours):
    the host form, and the device form on a non-default torch stream"""
    w = world(name)
    p = w.pts
    want = ao.expected(w, w.radii, spp)
    got, st = host_form(w.scene, p.points, p.seeds, w.radii, spp)
    ao.assert_same(got, want, "%s spp %d, host form" % (name, spp))
    assert st["kernel_ms"] > 0 and st["rays"] == 0 and st["paths"] == 0   # counters only on request
    got, st = torch_form(w.scene, p.points, p.seeds, w.radii, spp)
    assert st is None
    ao.assert_same(got, want, "%s spp %d, device form on a stream" % (name, spp))
    occ = ao.bits(w, w.radii, spp)[p.ok]
    assert occ.any() and not occ.all()


@pytest.mark.parametrize("name", list(SCENES))
def test_without_a_radius_and_at_one_radius(world, name):
    w = world(name)
    p = w.pts
    got, _ = host_form(w.scene, p.points, p.seeds, None, 8)
    ao.assert_same(got, ao.expected(w, None, 8), name + " no radius")
    got, _ = torch_form(w.scene, p.points, p.seeds, None, 8)
    ao.assert_same(got, ao.expected(w, None, 8), name + " no radius, device form")
    got, _ = host_form(w.scene, p.points, p.seeds, float(w.R), 8)       # a scalar: broadcast by the binding
    ao.assert_same(got, ao.expected(w, w.R, 8), name + " all R")


# ---- 2. the table-less kernels ----------------------------------------------------------------------------------------------------
def test_prologue_past_its_cap(oracle, table_scene):  # noqa: F811
    """40 boxes in the prologue, twice what its LDS slot holds: ao_points<*, false> reads them from HBM, with and without counters"""
    scene, osc_at = table_scene("pro_over", 40)
    flat = scene.flatten(1, 1)
    w = ao.build("tables pro_over/40", scene, flat, osc_at(1, 1), oracle, 124)
    p = w.pts
    assert len(p.points) == 128
    want = ao.expected(w, w.radii, 8)
    got, _ = host_form(scene, p.points, p.seeds, w.radii, 8)
    ao.assert_same(got, want, "pro_over/40")
    got, st = host_form(scene, p.points, p.seeds, w.radii, 8, counters=True)
    ao.assert_same(got, want, "pro_over/40 with counters")
    assert st["rays"] == 8 * int(p.ok.sum())
    occ = ao.bits(w, w.radii, 8)[p.ok]
    assert occ.any() and not occ.all()


# ---- 3. sample k is ort_occluded's ------------------------------------------------------------------------------------------------
def test_a_sample_is_an_occlusion_query(world):
    """c2_analytic: out_open at spp 8 equals spp minus the sum of ort_occluded's bytes over the eight rays (p, d_k) with the same
    limits, both run on the device"""
    w = world("c2_analytic")
    p = w.pts
    idx = np.flatnonzero(p.ok)
    rays = np.concatenate([np.repeat(p.points[idx, 0:3], 8, axis=0), w.d[idx].reshape(-1, 3)], axis=1).astype("<f4")
    occ, _ = w.scene.occluded(rays, np.repeat(w.radii[idx], 8))
    out, _ = w.scene.ambient_occlusion(p.points, p.seeds, 8, radius=w.radii)
    assert (out[idx] == 8 - occ.reshape(-1, 8).sum(axis=1)).all()
    assert 0 < occ.mean() < 1


def test_radius_ladder(oracle, gpu_scene):
    """ao_cases.radius_ladder's arrays (tests/test_ao_host.py runs them through the lane code on the host), one launch at one sample
    per point: open one float below the sample's own hit distance and at it, occluded one float above.  What this pins on the device
    is the bound: a bounded walk that accepted a hit at or beyond its bound, or cut one below it, fails here.  It does not pin the
    verdict's strict <: the bounded walk never accepts a hit at t == bound, so with <= these samples are still open; only a sample
    that takes the exact walk shows it, and that is the host test's run under SIM_FORCE_FALLBACK=0 (the device reads its knob at
    upload, and this is one launch at the defaults)"""
    scene = gpu_scene("testscene")
    flat = scene.flatten(1, 1)
    points, seeds, radii, want, left_out = ao.radius_ladder(oracle, oracle.OracleScene(flat), flat)
    assert 4 * left_out <= ao.LADDER_POINTS and 0 < len(points) <= 192
    out, _ = scene.ambient_occlusion(points, seeds, 1, radius=radii)
    bad = np.flatnonzero(out != want)
    assert len(bad) == 0, "%d open counts differ, first at point %d rung %s: %d" % (len(bad), bad[0] // 3, ("prev(t)", "t", "next(t)")[bad[0] % 3], out[bad[0]])


# ---- 4. counts and guard words ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 63, 65, 513])
def test_counts_and_guard_words(api, world, count):
    """guard words after every output array of the host form; the device form writes no further than count; with each optional
    output NULL in turn the others are unchanged, and nothing is written where nothing was asked for"""
    w = world("testscene")
    idx = np.arange(count) % len(w.pts.points)
    p = w.pts.take(idx)
    radii = np.ascontiguousarray(w.radii[idx])
    want = ao.expected(w, w.radii, 8, idx)
    L = api.lib()
    pts, seeds = np.ascontiguousarray(p.points), np.ascontiguousarray(p.seeds)
    for skip in ((), ("bent",), ("states",), ("bent", "states")):
        out, bent, fin = np.full(count + 8, 0xC3C3C3C3, "<u4"), np.full(3 * count + 8, -3.5, "<f4"), np.full(count + 8, 0xC3C3C3C3, "<u4")
        assert L.ort_ambient_occlusion(w.scene.handle, pts.ctypes.data, seeds.ctypes.data, radii.ctypes.data, count, 8, out.ctypes.data,
                                       None if "bent" in skip else bent.ctypes.data, None if "states" in skip else fin.ctypes.data, 0, None) == api.OK
        ao.assert_same((out[:count], None if "bent" in skip else bent[:3 * count], None if "states" in skip else fin[:count]), want,
                       "host form, %d points, without %r" % (count, skip))
        assert (out[count:] == 0xC3C3C3C3).all() and (bent[3 * count:] == np.float32(-3.5)).all() and (fin[count:] == 0xC3C3C3C3).all()
        assert "bent" not in skip or (bent == np.float32(-3.5)).all()
        assert "states" not in skip or (fin == 0xC3C3C3C3).all()
        got, _ = torch_form(w.scene, pts, seeds, radii, 8, skip=skip, pad=8)
        ao.assert_same((got[0][:count], None if "bent" in skip else got[1][:count], None if "states" in skip else got[2][:count]), want,
                       "device form, %d points, without %r" % (count, skip))
        assert (got[0][count:] == 0x5A5A5A5A).all() and (got[1][count:] == np.float32(-7.0)).all() and (got[2][count:] == 0x5A5A5A5A).all()
        assert "bent" not in skip or (got[1] == np.float32(-7.0)).all()
        assert "states" not in skip or (got[2] == 0x5A5A5A5A).all()


# ---- 5. independence ---------------------------------------------------------------------------------------------------------------
def test_a_points_answer_is_its_own(world):
    """512 points permuted, and cut into calls of 1, 63 and the rest: the same per-point words"""
    w = world("c2_analytic")
    idx = np.arange(512) % len(w.pts.points)
    p = w.pts.take(idx)
    radii = w.radii[idx]
    want = ao.expected(w, w.radii, 8, idx)
    got, _ = host_form(w.scene, p.points, p.seeds, radii, 8)
    ao.assert_same(got, want, "512 points")
    perm = np.random.default_rng(7).permutation(512)
    got, _ = host_form(w.scene, p.points[perm], p.seeds[perm], radii[perm], 8)
    ao.assert_same(got, tuple(a[perm] for a in want), "512 points permuted")
    parts = [host_form(w.scene, p.points[a:b], p.seeds[a:b], radii[a:b], 8)[0] for a, b in ((0, 1), (1, 64), (64, 512))]
    ao.assert_same(tuple(np.concatenate([part[k] for part in parts]) for k in range(3)), want, "512 points in three calls")


# ---- 6. counters ---------------------------------------------------------------------------------------------------------------------
def test_counters_count_the_samples(world):
    """rays = (points inside the domain) * spp, whatever the radius (a sample is counted before its radius is looked at); paths = 0;
    the far points of c2_analytic fall back on every sample, the near ones on fewer; the axis points' first sample falls back"""
    w = world("c2_analytic")
    p = w.pts
    inside = int(p.ok.sum())
    for spp in (1, 8):
        for radius in (w.radii, None):
            got, st = host_form(w.scene, p.points, p.seeds, radius, spp, counters=True)
            ao.assert_same(got, ao.expected(w, radius, spp), "with counters")
            assert st["rays"] == inside * spp and st["paths"] == 0 and st["node_tests"] > 0 and st["kernel_ms"] > 0
    got, st = torch_form(w.scene, p.points, p.seeds, w.radii, 8, counters=True, want_stats=True)
    assert st["rays"] == inside * 8 and st["paths"] == 0
    far = np.flatnonzero(p.far)
    R = np.float32(w.R)
    _, st = host_form(w.scene, p.points[far], p.seeds[far], np.full(len(far), R, "<f4"), 8, counters=True)
    assert st["fallback_rays"] >= 8 * len(far) > 0 and st["rays"] == 8 * len(far)
    near = np.flatnonzero(p.ok[:w.base] & ~p.far[:w.base])[:64]
    _, st_near = host_form(w.scene, p.points[near], p.seeds[near], np.full(len(near), R, "<f4"), 8, counters=True)
    assert st_near["fallback_rays"] < 8 * len(near)


def test_axis_samples_fall_back_with_boxes_in_the_tree(api, world, monkeypatch):
    """c2_analytic: a +-0 component of d_0 sends that sample to the exact walk when the fast tree holds boxes.  As the scene commits
    by itself all nine boxes sit in the analytic prologue, so the rule does not apply; committed under ORT_ANALYTIC_PROLOGUE=0
    every box is in the tree, and fallback_rays counts the sample.  The bits are the oracle's both ways"""
    import os
    from conftest import DATA
    w = world("c2_analytic")
    p = w.pts
    assert w.scene.tree_info()["prologue_prims"] >= w.scene.info().box_count > 0
    axis = np.arange(w.base, len(p.points))
    assert ((w.d[axis, 0] == 0).sum(axis=1) == 2).all()   # d_0 has +-0 components
    R = np.float32(w.R)
    want = ao.expected(w, R, 1, axis)
    got, st = host_form(w.scene, p.points[axis], p.seeds[axis], np.full(len(axis), R, "<f4"), 1, counters=True)
    ao.assert_same(got, want, "axis points, boxes in the prologue")
    scene = api.Scene.load_scn(os.path.join(DATA, "c2_analytic.scn"))
    monkeypatch.setenv("ORT_ANALYTIC_PROLOGUE", "0")   # read by build_tree at commit
    scene.commit()
    monkeypatch.delenv("ORT_ANALYTIC_PROLOGUE")
    assert scene.tree_info()["prologue_prims"] == 0
    scene.upload(0)
    for counters in (True, False):
        got, st = host_form(scene, p.points[axis], p.seeds[axis], np.full(len(axis), R, "<f4"), 1, counters=counters)
        ao.assert_same(got, want, "axis points, boxes in the tree")
        assert st["fallback_rays"] >= len(axis)
    got, st = host_form(scene, p.points, p.seeds, w.radii, 8, counters=True)
    ao.assert_same(got, ao.expected(w, w.radii, 8), "all points, boxes in the tree")
    with np.errstate(invalid="ignore"):
        live = w.radii > 0   # a point whose radius is NaN or <= 0 traverses nothing, so it cannot fall back
    assert st["fallback_rays"] >= int(live[axis].sum()) + 8 * int((p.far & live).sum()) > 0


# ---- 7. across a staging slice ---------------------------------------------------------------------------------------------------------
SLICE_COUNT = (1 << 20) + 257   # kRadianceSlice of offline_raytracer_amd/csrc/ort_kernels.hip and a ragged remainder
BASE = 4096


def test_host_form_crosses_a_staging_slice(world):
    """(1 << 20) + 257 points tiled from 4 096, one sample each: the host form, staged in two slices, equals the device form's one
    launch in every output; invalid points are present"""
    w = world("c2_analytic")
    rng = np.random.default_rng(zlib.crc32(b"slice boundary ao"))
    anywhere = np.concatenate([rng.uniform(w.lo, w.hi, size=(BASE - 16, 3)), rc._units(rng, BASE - 16)], axis=1)
    base = np.concatenate([anywhere, ic.out_of_domain(rng, w.lo, w.hi, 16)]).astype("<f4")[rng.permutation(BASE)]
    seeds = rng.integers(0, 1 << 32, BASE, dtype=np.uint64).astype("<u4")
    radii = np.where(rng.random(BASE) < 0.1, np.float32(np.nan), (w.diag * rng.uniform(0.0, 0.5, BASE))).astype("<f4")
    idx = np.arange(SLICE_COUNT) % BASE
    pts, seeds, radii = np.ascontiguousarray(base[idx]), np.ascontiguousarray(seeds[idx]), np.ascontiguousarray(radii[idx])
    host, st = host_form(w.scene, pts, seeds, radii, 1, counters=True)
    dev, _ = torch_form(w.scene, pts, seeds, radii, 1)
    for h, d, what in zip(host, dev, ("open", "bent", "final states")):
        assert h.shape == d.shape and h.tobytes() == d.tobytes(), what
    out = host[0]
    bad = ~ic.in_domain(base)
    assert bad.sum() == 16 and ((out == ao.AO_INVALID) == bad[idx]).all()
    assert (out == 0).any() and (out == 1).any() and np.isnan(host[1]).any()
    assert (out[:BASE] == out[BASE:2 * BASE]).all() and (out[-257:] == out[:257]).all()
    assert st["rays"] == int((out != ao.AO_INVALID).sum())   # the counters of both slices


# ---- 8. the bound cuts the work --------------------------------------------------------------------------------------------------------
def test_the_radius_bounds_the_walk(world):
    """c3_bunny_room with counters: fewer node tests at a radius of 0.02 x the diagonal than without one, on the same points and seeds.
    The tree holds no spheres there, so a point farther than its radius from the root's two boxes costs one test of them (counted
    as two node tests) and none of its samples visits the tree; without a radius every sample that is not ended early visits it"""
    w = world("c3_bunny_room")
    p = w.pts
    _, near = host_form(w.scene, p.points, p.seeds, float(np.float32(0.02 * w.diag)), 8, counters=True)
    _, free = host_form(w.scene, p.points, p.seeds, None, 8, counters=True)
    print("node_tests: %d at 0.02 x the diagonal, %d without a radius" % (near["node_tests"], free["node_tests"]))
    assert near["rays"] == free["rays"] and 0 < near["node_tests"] < free["node_tests"]
