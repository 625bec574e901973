"""Occlusion ray queries on the device (ort_occluded / ort_occluded_device, kernel occluded_rays).  The contract
(include/ort.h): occluded[i] = (h.mat != 0 && h.t < tmax[i]) with h the reference's closest hit of rays[i], the IEEE
comparison, one byte per ray.  There is no tolerance: every byte equals the value worked out in numpy from the
reference's own answers (tests/golden/raycast_*.npz, raycast_edges_*.npz, raycast_tables_*.npz), from the oracle at scale
and on the hostile rays, and from the closest-hit kernel on the same tensors.  The limits that matter most sit one ulp
either side of the hit: a traversal cut at tmax has not seen what lies beyond it, and must not let that decide."""
import os
import zlib

import numpy as np
import pytest

import raycast_cases
from occluded_cases import RUNGS, drawn_limits, expected, ladder, laddered  # noqa: F401
import table_scenes
from conftest import GOLDEN
from test_gpu_raycast import SCENES, golden_like, mixed_rays, torch_raycast
from test_gpu_tables import table_scene  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

F32 = np.float32
FLT_MAX = F32(3.4028235e38)
INF = F32(np.inf)
KINDS = ["golden distribution", "start on a surface", "axis-aligned / non-unit", "outside, missing"]


def assert_bytes(got, want, what, groups=None, names=None):
    got = np.asarray(got)
    assert got.shape == want.shape, "%s: %s vs %s" % (what, got.shape, want.shape)
    raw = got.view(np.uint8)
    assert ((raw == 0) | (raw == 1)).all(), "%s: a byte that is neither 0 nor 1" % what
    bad = np.flatnonzero(raw != want.astype(np.uint8))
    if len(bad):
        where = ""
        if groups is not None:
            g = groups[bad]
            where = "; by group: " + ", ".join("%s %d" % (names[i], (g == i).sum()) for i in np.unique(g))
        raise AssertionError("%s: %d of %d bytes differ, first at %d (got %d, want %d)%s"
                             % (what, len(bad), len(want), bad[0], raw[bad[0]], int(want[bad[0]]), where))


def torch_occluded(scene, rays, tmax, counters=False, want_stats=False):
    """the device form: torch tensors on a non-default stream, the output prefilled with 0xAB and followed by 64 guard
    bytes, which must come back untouched"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(rays)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays, "<f4")).to(dev)
    d_tmax = None if tmax is None else torch.from_numpy(np.ascontiguousarray(tmax, "<f4")).to(dev)
    d_out = torch.full((n + 64,), 0xAB, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        st = scene.occluded_device(d_rays.data_ptr(), None if d_tmax is None else d_tmax.data_ptr(), n, d_out.data_ptr(),
                                   stream=stream.cuda_stream, counters=counters, want_stats=want_stats)
    stream.synchronize()
    out = d_out.cpu().numpy()
    assert (out[n:] == 0xAB).all(), "guard bytes after the output were written"
    assert ((out[:n] == 0) | (out[:n] == 1)).all(), "an output byte that is neither 0 nor 1"
    return out[:n].view(np.bool_), st


def check_ladder(scene, rays, t, mat, what, device_form=True):
    assert not np.isnan(t).any()
    rr, tm, want, rung = laddered(rays, t, mat)
    # neither answer can be had from a constant
    assert (~want).mean() >= 0.10 and want.mean() >= 0.10, (what, want.mean())
    got, st = scene.occluded(rr, tm)
    assert got.dtype == np.bool_
    assert_bytes(got, want, what + ", host form", rung, RUNGS)
    assert st["paths"] == 0 and st["kernel_ms"] > 0
    if device_form:
        dg, _ = torch_occluded(scene, rr, tm)
        assert_bytes(dg, want, what + ", device form", rung, RUNGS)
    # no limit == the +inf rung
    inf_rung = expected(t, mat, np.full(len(t), INF, "<f4"))
    none, _ = scene.occluded(rays)
    assert_bytes(none, inf_rung, what + ", tmax=None, host form")
    if device_form:
        dn, _ = torch_occluded(scene, rays, None)
        assert_bytes(dn, inf_rung, what + ", tmax=None, device form")
    scalar, _ = scene.occluded(rays, np.inf)
    assert_bytes(scalar, inf_rung, what + ", scalar +inf")
    return rr, tm, want


# ---- 1. the reference's own answers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("prefix", ["raycast", "raycast_edges"])
def test_reference_fixtures_through_the_ladder(api, gpu_scene, prefix, name):
    z = np.load(os.path.join(GOLDEN, "%s_%s.npz" % (prefix, name)))
    check_ladder(gpu_scene(name), z["rays"], z["t"], z["mat"], "%s_%s" % (prefix, name))


# ---- 2. the oracle at scale --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [(s, 20000) for s in SCENES] + [("c5_heightfield_224", 4000)])
def test_against_oracle_at_scale(api, oracle, gpu_scene, name, n):
    scene = gpu_scene(name)
    rays, kinds = mixed_rays(scene, name, n)
    t, _, mat = oracle.OracleScene(scene.flatten(64, 64)).raycast(rays[:, 0:3], rays[:, 3:6])
    rng = np.random.default_rng(zlib.crc32(("occluded " + name).encode()))
    tm = drawn_limits(rng, t)
    want = expected(t, mat, tm)
    got, _ = scene.occluded(rays, tm)
    for k, what in enumerate(KINDS):
        sel = kinds == k
        assert_bytes(got[sel], want[sel], "%s: %s" % (name, what))
    assert not got[kinds == 3].any()          # misses, whatever the limit
    assert 0.1 < want[kinds == 0].mean() < 0.9
    dg, _ = torch_occluded(scene, rays, tm)
    assert_bytes(dg, want, name + ", device form", kinds, KINDS)


# ---- 3. agreement with the closest-hit kernel --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c3_bunny_room", "c2_analytic"])
def test_agrees_with_closest_hit_kernel(api, gpu_scene, name):
    scene = gpu_scene(name)
    rng = np.random.default_rng(zlib.crc32(("agree " + name).encode()))
    n = 1 << 20
    rays = golden_like(rng, n)
    hits, _ = torch_raycast(scene, rays)
    t, mat = hits["t"], hits["mat"]
    assert (mat != 0).sum() > n // 2
    with np.errstate(over="ignore"):
        limits = {"t/2": t * F32(0.5), "next(t)": np.nextafter(t, INF), "t permuted across rays": t[rng.permutation(n)]}
    for what, tm in limits.items():
        tm = np.ascontiguousarray(tm, "<f4")
        got, _ = torch_occluded(scene, rays, tm)
        assert_bytes(got, expected(t, mat, tm), "%s, tmax = %s" % (name, what))
    perm_want = expected(t, mat, limits["t permuted across rays"])
    assert 0.2 < perm_want.mean() < 0.8


# ---- 4. hostile rays ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_hostile_rays_through_the_ladder(api, oracle, gpu_scene, name):
    scene = gpu_scene(name)
    flat = scene.flatten(64, 64)
    osc = oracle.OracleScene(flat)
    rays, cat = raycast_cases.cases(flat, lambda r: osc.raycast(r[:, 0:3], r[:, 3:6])[0], scale=4)
    t, _, mat = osc.raycast(rays[:, 0:3], rays[:, 3:6])
    rr, tm, want, _ = laddered(rays, t, mat)
    got, _ = scene.occluded(rr, tm)
    k = len(RUNGS)
    cats = np.repeat(cat, k)
    for c, what in enumerate(raycast_cases.CATEGORIES):
        sel = cats == c
        assert sel.any()
        assert_bytes(got[sel], want[sel], "%s, %s rays" % (name, what), np.tile(np.arange(k), len(t))[sel], RUNGS)


# ---- 5. the exact walk, and the tables in HBM ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c2_analytic", "c3_bunny_room", "letters", "glass_room"])
def test_forced_exact_walk_and_hbm_tables(api, gpu_scene, monkeypatch, name):
    z = np.load(os.path.join(GOLDEN, "raycast_%s.npz" % name))
    e = np.load(os.path.join(GOLDEN, "raycast_edges_%s.npz" % name))
    scene = gpu_scene(name)
    rays = np.concatenate([z["rays"], e["rays"][::4]])
    t, mat = np.concatenate([z["t"], e["t"][::4]]), np.concatenate([z["mat"], e["mat"][::4]])
    rr, tm, want, rung = laddered(rays, t, mat)
    fast, st_fast = scene.occluded(rr, tm)
    assert_bytes(fast, want, name + " default", rung, RUNGS)
    monkeypatch.setenv("ORT_DEBUG_FORCE_FALLBACK", "0")
    exact, st = scene.occluded(rr, tm)
    none_exact, st_none = scene.occluded(rays)
    monkeypatch.delenv("ORT_DEBUG_FORCE_FALLBACK")
    assert st["fallback_rays"] == len(rr) > st_fast["fallback_rays"]
    assert st_none["fallback_rays"] == len(rays)
    assert exact.tobytes() == fast.tobytes()
    assert_bytes(none_exact, expected(t, mat, np.full(len(t), INF, "<f4")), name + " forced walk, no limit")
    monkeypatch.setenv("ORT_LDS_TABLES", "0")
    hbm, st_hbm = scene.occluded(rr, tm)
    counted, st_c = scene.occluded(rr, tm, counters=True)
    monkeypatch.delenv("ORT_LDS_TABLES")
    assert hbm.tobytes() == fast.tobytes() and counted.tobytes() == fast.tobytes()
    assert st_hbm["fallback_rays"] == st_fast["fallback_rays"] and st_c["rays"] == len(rr)


# ---- 6. scenes past the caps of the LDS tables ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", table_scenes.GOLDEN_VARIANTS)
def test_table_scenes_through_the_ladder(api, table_scene, variant):  # noqa: F811
    scene, _ = table_scene(variant)
    r = np.load(os.path.join(GOLDEN, "raycast_tables_%s.npz" % variant))
    rr, tm, want, rung = laddered(r["rays"], r["t"], r["mat"])
    got, _ = scene.occluded(rr, tm)
    assert_bytes(got, want, variant + ", host form", rung, RUNGS)
    dg, _ = torch_occluded(scene, rr, tm)
    assert_bytes(dg, want, variant + ", device form", rung, RUNGS)
    assert want.any() and not want.all()


def test_prologue_past_its_cap(api, table_scene):  # noqa: F811
    """40 boxes in the prologue, twice what its LDS slot holds: occluded_rays<*, false> reads them from HBM"""
    scene, osc_at = table_scene("pro_over", 40)
    osc = osc_at(64, 64)
    rays, _ = mixed_rays(scene, "tables pro_over/40 occluded", 4000)
    t, _, mat = osc.raycast(rays[:, 0:3], rays[:, 3:6])
    rr, tm, want, rung = laddered(rays, t, mat)
    got, _ = scene.occluded(rr, tm)
    assert_bytes(got, want, "pro_over/40", rung, RUNGS)
    counted, st = scene.occluded(rr, tm, counters=True)
    assert counted.tobytes() == got.tobytes() and st["rays"] == len(rr)
    assert want.any() and not want.all()


# ---- 7. slicing and order ------------------------------------------------------------------------------------------------
def test_independent_of_batch_order_and_slicing(api, gpu_scene):
    scene = gpu_scene("c3_bunny_room")
    rng = np.random.default_rng(77)
    n = 200003
    rays = golden_like(rng, n)
    hits, _ = scene.raycast(rays)
    tm = drawn_limits(rng, hits["t"])
    ref, _ = torch_occluded(scene, rays, tm)
    assert_bytes(ref, expected(hits["t"], hits["mat"], tm), "whole batch")
    perm = rng.permutation(n)
    shuffled, _ = scene.occluded(rays[perm], tm[perm])
    assert shuffled.tobytes() == ref[perm].tobytes()
    at, parts = 0, []
    for size in (1, 63, 65, 1025, n - (1 + 63 + 65 + 1025)):
        part, _ = scene.occluded(rays[at:at + size], tm[at:at + size])
        parts.append(part)
        at += size
    assert at == n and np.concatenate(parts).tobytes() == ref.tobytes()
    again, _ = torch_occluded(scene, rays, tm)
    assert again.tobytes() == ref.tobytes()


def test_host_form_across_its_slice_boundary(api, gpu_scene):
    """2^22 + 65 rays with a limit each: the host form stages rays, limits and bytes through the scene's buffers in slices of
    2^22 rays, so this is two launches, the second of 65 rays from an offset into all three arrays.  Every byte equals the
    device form's for the same rays in one launch, and the host form's for the two halves given separately (one slice each)."""
    scene = gpu_scene("c3_bunny_room")
    rng = np.random.default_rng(zlib.crc32(b"occluded slices"))
    n = (1 << 22) + 65
    rays = golden_like(rng, n)
    hits, _ = torch_raycast(scene, rays)
    tm = drawn_limits(rng, hits["t"])
    ref, st_dev = torch_occluded(scene, rays, tm, counters=True, want_stats=True)
    assert_bytes(ref, expected(hits["t"], hits["mat"], tm), "device form, one launch")
    assert 0.1 < ref.mean() < 0.9 and ref[-65:].any() and not ref[-65:].all()  # neither slice can be had from a constant
    got, st = scene.occluded(rays, tm, counters=True)
    assert_bytes(got, ref, "host form, two slices")
    assert st["rays"] == n == st_dev["rays"] and st["paths"] == 0
    half = n // 2
    a, st_a = scene.occluded(rays[:half], tm[:half], counters=True)
    b, st_b = scene.occluded(rays[half:], tm[half:], counters=True)
    assert np.concatenate([a, b]).tobytes() == ref.tobytes()
    assert (st_a["rays"], st_b["rays"]) == (half, n - half)


# ---- 8. the bound is used ------------------------------------------------------------------------------------------------
def test_the_bound_cuts_the_traversal(api, gpu_scene):
    scene = gpu_scene("c3_bunny_room")
    cand = golden_like(np.random.default_rng(8), 60000)
    first, _ = scene.raycast(cand)
    sel = np.flatnonzero(first["mat"] != 0)[:20000]
    assert len(sel) == 20000
    rays, t = cand[sel], first["t"][sel]
    _, st_closest = scene.raycast(rays, counters=True)
    got, st = scene.occluded(rays, t * F32(0.5), counters=True)
    assert not got.any()
    assert st["rays"] == len(rays) == st_closest["rays"]
    assert st["node_tests"] + st["tri_tests"] < st_closest["node_tests"] + st_closest["tri_tests"]
    # and a limit that asks for no traversal at all does none
    got, st0 = scene.occluded(rays, np.zeros(len(rays), "<f4"), counters=True)
    assert not got.any() and st0["rays"] == len(rays) and st0["node_tests"] == 0 and st0["tri_tests"] == 0
