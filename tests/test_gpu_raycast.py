"""Closest-hit ray queries on the device (ort_raycast / ort_raycast_device, kernel raycast_rays): bit for bit the
reference's raycast_top_most_node (ray.cpp:1165-1176) -- its own outputs (tests/golden/raycast_*.npz) and, at scale
and on the hard cases (rays that start on a surface, axis-aligned and non-unit directions, misses), the oracle."""
import os

import numpy as np
import pytest

import raycast_cases
import ref_io
from conftest import DATA, GOLDEN, assert_bits_equal
from raycast_cases import golden_like, unit_vectors  # noqa: F401  (other test files import them from here)
from raycast_cases import needs_exact as _needs_exact, scene_box as _scene_box, threshold_rays as _threshold_rays  # noqa: F401
from raycast_cases import threshold_scene as _threshold_scene  # noqa: F401

pytestmark = pytest.mark.gpu

SCENES = ["testscene", "c2_analytic", "c3_bunny_room", "c4_dwarf_room", "letters", "glass_room", "rand_a", "rand_b"]
FLT_MAX = np.float32(3.4028235e38)


def hits_of(hits):
    return hits["t"], hits["n"], hits["mat"]


def assert_same_hits(hits, t, n, mat, what):
    assert_bits_equal(hits["t"], t, what + " t")
    assert_bits_equal(hits["n"], n, what + " normal")
    bad = np.flatnonzero(hits["mat"] != mat)
    assert len(bad) == 0, "%s: material differs for %d rays, first %d: %d vs %d" % (what, len(bad), bad[0], hits["mat"][bad[0]], mat[bad[0]])


def torch_raycast(scene, rays, counters=False, want_stats=False):
    """the device form, with torch tensors on a non-default stream"""
    import torch
    dev = torch.device("cuda", 0)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays, "<f4")).to(dev)
    d_hits = torch.full((len(rays) * 24,), 0xAB, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        st = scene.raycast_device(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), stream=stream.cuda_stream,
                                  counters=counters, want_stats=want_stats)
    stream.synchronize()
    from offline_raytracer_amd import api
    return d_hits.cpu().numpy().view(api.HIT_DTYPE), st


@pytest.mark.parametrize("name", SCENES)
def test_reference_goldens(api, gpu_scene, name):
    """the reference's own closest hits for 400 rays per scene: host form and device form (torch, non-default stream)"""
    z = np.load(os.path.join(GOLDEN, "raycast_%s.npz" % name))
    scene = gpu_scene(name)
    hits, st = scene.raycast(z["rays"])
    assert_same_hits(hits, z["t"], z["n"], z["mat"], name + " host form")
    assert st["paths"] == 0 and st["kernel_ms"] > 0
    dh, _ = torch_raycast(scene, z["rays"])
    assert_same_hits(dh, z["t"], z["n"], z["mat"], name + " device form")
    assert (dh["prim"] == hits["prim"]).all()


def mixed_rays(scene, name, n):
    """raycast_cases.mixed_rays with the device's own first cast placing the surface starts"""
    return raycast_cases.mixed_rays(lambda rays: scene.raycast(rays)[0]["t"], name, n)


@pytest.mark.parametrize("name,n", [(s, 20000) for s in SCENES] + [("c5_heightfield_224", 4000)])
def test_against_oracle_at_scale(api, oracle, gpu_scene, name, n):
    scene = gpu_scene(name)
    rays, kinds = mixed_rays(scene, name, n)
    hits, _ = scene.raycast(rays)
    osc = oracle.OracleScene(scene.flatten(64, 64))
    t, nrm, mat = osc.raycast(rays[:, 0:3], rays[:, 3:6])
    for k, what in enumerate(["golden distribution", "start on a surface", "axis-aligned / non-unit", "outside, missing"]):
        sel = kinds == k
        assert_same_hits(hits[sel], t[sel], nrm[sel], mat[sel], "%s: %s" % (name, what))
    assert (kinds == 1).sum() > n // 8  # enough surface starts
    # a miss is what the reference returns: Flt_Max, zero normal, material 0; and no shape
    out = hits[kinds == 3]
    assert (out["t"].view("<u4") == FLT_MAX.view("<u4")).all() and (out["n"] == 0).all() and (out["mat"] == 0).all()
    assert (out["prim"] == api.NO_PRIM).all()
    missed = hits["t"] == FLT_MAX
    assert ((hits["prim"] == api.NO_PRIM) == missed).all()
    assert (hits["mat"][~missed] != 0).all()


@pytest.mark.parametrize("name", ["c2_analytic", "c3_bunny_room", "letters", "glass_room"])
def test_forced_exact_walk(api, gpu_scene, monkeypatch, name):
    """every ray re-cast on the reference-compatible octree (the exact fallback): the same bits"""
    z = np.load(os.path.join(GOLDEN, "raycast_%s.npz" % name))
    scene = gpu_scene(name)
    rays = np.concatenate([z["rays"], golden_like(np.random.default_rng(7), 3000)])
    fast, st_fast = scene.raycast(rays)
    monkeypatch.setenv("ORT_DEBUG_FORCE_FALLBACK", "0")
    exact, st = scene.raycast(rays)
    monkeypatch.delenv("ORT_DEBUG_FORCE_FALLBACK")
    assert st["fallback_rays"] == len(rays) > st_fast["fallback_rays"]
    assert_same_hits(exact[: len(z["t"])], z["t"], z["n"], z["mat"], name + " forced fallback, goldens")
    assert exact.tobytes() == fast.tobytes()


UNIT_OPS = {0: 1, 4: 2, 2: 3, 3: 4}  # hit kind -> unit_eval op (triangle, sphere, aab, cylinder)


@pytest.mark.parametrize("name", SCENES + ["c5_heightfield_224"])
def test_prim_is_the_shape_that_was_hit(api, gpu_scene, name):
    """re-intersect every hit ray with the reported shape alone (unit_eval_device ops 1-4): same t, same normal, and
    the shape's material is the hit's"""
    scene = gpu_scene(name)
    rays, kinds = mixed_rays(scene, name, 6000)
    hits, _ = scene.raycast(rays)
    sel = np.flatnonzero(hits["prim"] != api.NO_PRIM)
    assert len(sel) > 1000
    kind, index = api.decode_prim(hits["prim"][sel])
    flat = scene.flatten(64, 64)
    rows = np.zeros((len(sel), 24), "<f4")
    mat = np.zeros(len(sel), "<u4")
    o, d = rays[sel, 0:3], rays[sel, 3:6]
    k = kind == api.HIT_TRIANGLE
    if k.any():
        mesh, local = scene.triangle_of(index[k])
        for m in np.unique(mesh):
            mm = flat.meshes[m]
            w = np.flatnonzero(k)[mesh == m]
            ix = mm["indices"].reshape(-1, 3)[local[mesh == m]]
            rows[w, 0:3], rows[w, 3:6], rows[w, 6:9] = mm["vertices"][ix[:, 0]], mm["vertices"][ix[:, 1]], mm["vertices"][ix[:, 2]]
            rows[w, 9:12], rows[w, 12:15] = o[w], d[w]
            mat[w] = mm["mat"]
    k = kind == api.HIT_SPHERE
    sp = flat.spheres[index[k]]
    rows[k, 0:3], rows[k, 3], rows[k, 4:7], rows[k, 7:10], mat[k] = sp["center"], sp["r"], o[k], d[k], sp["mat"]
    k = kind == api.HIT_BOX
    bx = flat.boxes[index[k]]
    rows[k, 0:3], rows[k, 3:6], rows[k, 6:9], rows[k, 9:12], mat[k] = bx["min"], bx["max"], o[k], d[k], bx["mat"]
    k = kind == api.HIT_CYLINDER
    cy = flat.cylinders[index[k]]
    rows[k, 0:3], rows[k, 3:6], rows[k, 6], rows[k, 7:10], rows[k, 10:13], mat[k] = cy["base"], cy["axis"], cy["r"], o[k], d[k], cy["mat"]
    ops = np.vectorize(UNIT_OPS.get)(kind)
    recs = np.zeros(len(sel), dtype=ref_io.UNIT_REC_DTYPE)
    recs["op"] = ops
    recs["a"] = rows
    got = api.unit_eval_device(recs)
    assert_bits_equal(got[:, 0], hits["t"][sel], name + " t of the reported shape")
    # raycast_bvh returns the normal normalised (ray.cpp:817): the device's normalize (op 10, math.h:298-310)
    nrm = np.zeros((len(sel), 24), "<f4")
    nrm[:, 0:3] = got[:, 1:4]
    unit = api.unit_eval_device(ref_io.make_unit_records(10, nrm))
    assert_bits_equal(unit[:, 0:3], hits["n"][sel], name + " normal of the reported shape")
    assert (mat == hits["mat"][sel]).all()


def test_independent_of_batch_order_and_slicing(api, gpu_scene):
    scene = gpu_scene("c3_bunny_room")
    rng = np.random.default_rng(2024)
    n = (1 << 20) + 7
    rays = golden_like(rng, n)
    ref, _ = torch_raycast(scene, rays)
    assert (ref["t"] < FLT_MAX).sum() > n // 2
    for count in (1, 63, 64, 65):
        part, _ = scene.raycast(rays[:count])
        assert part.tobytes() == ref[:count].tobytes(), count
        part, _ = scene.raycast(rays[n - count:])
        assert part.tobytes() == ref[n - count:].tobytes(), count
    perm = rng.permutation(n)
    shuffled, _ = scene.raycast(rays[perm])
    assert shuffled.tobytes() == ref[perm].tobytes()
    again, _ = torch_raycast(scene, rays)
    assert again.tobytes() == ref.tobytes()
    # the host form cuts more than 4M rays into slices of 4M: same answers
    big = np.concatenate([rays[perm], rays, rays[perm], rays, rays[:9]])
    assert len(big) > (1 << 22)
    hb, _ = scene.raycast(big)
    assert hb.tobytes() == np.concatenate([ref[perm], ref, ref[perm], ref, ref[:9]]).tobytes()


def test_counters(api, gpu_scene):
    scene = gpu_scene("c3_bunny_room")
    rays = golden_like(np.random.default_rng(5), 100000)
    plain, st0 = scene.raycast(rays)
    hits, st = scene.raycast(rays, counters=True)
    assert hits.tobytes() == plain.tobytes()
    assert st["rays"] == len(rays) and st["paths"] == 0
    assert st["node_tests"] > 0 and st["tri_tests"] > 0 and st["analytic_tests"] > 0
    assert st["kernel_ms"] > 0 and st0["kernel_ms"] > 0
    assert st0["rays"] == 0 and st0["node_tests"] == 0  # counters only on request
    _, sd = torch_raycast(scene, rays, counters=True, want_stats=True)
    assert sd["rays"] == len(rays) and sd["node_tests"] == st["node_tests"] and sd["kernel_ms"] > 0
    empty, s_empty = scene.raycast(np.zeros((0, 6), "<f4"), counters=True)
    assert len(empty) == 0 and s_empty["rays"] == 0


def test_renders_unchanged_by_raycasts(api, oracle):
    """a fresh upload renders, builds its query tables at the first raycast, renders again: both renders bit-equal to
    the oracle"""
    scene = api.Scene.load_scn(os.path.join(DATA, "c3_bunny_room.scn")).commit().upload(0)
    W = H = 40
    before, _ = scene.render(W, H, 8, 99, "chunk", chunk=4)
    z = np.load(os.path.join(GOLDEN, "raycast_c3_bunny_room.npz"))
    hits, _ = scene.raycast(z["rays"])
    assert_same_hits(hits, z["t"], z["n"], z["mat"], "raycast between renders")
    torch_raycast(scene, golden_like(np.random.default_rng(3), 50000))
    after, _ = scene.render(W, H, 8, 99, "chunk", chunk=4)
    assert_bits_equal(after, before, "render after raycasts")
    ref, _ = oracle.OracleScene(scene.flatten(W, H)).render(W, H, 8, 99, "chunk", chunk=4, threads=4)
    assert_bits_equal(after, ref, "render after raycasts vs oracle")
    scene.close()


# ---- rays at the exact walk's thresholds (raycast_needs_exact, ort_lane.h) -------------------------------------------
# raycast_needs_exact sends a ray to the exact octree walk when |d|^2 < 0.999 with spheres in the fast tree (< 1e-30
# with cylinders alone), or when its origin lies outside the scene box with quadrics in it.  Rays with |d|^2 in
# [0.999, 1) stay in the fast tree, whose sphere boxes (ort_tree.cpp) must then hold every tangent-band "hit"
# (|b^2 - a c| < 1e-5: a band that widens as 1e-5 / |d|^2), and rays from exactly the scene box's faces count as inside.
@pytest.mark.parametrize("small", [False, True], ids=["room", "small"])
def test_exact_walk_thresholds(api, oracle, monkeypatch, small):
    """tangent rays across the sphere band at |d|^2 around 0.999 and 1, origins on the scene box's faces and one ulp
    either side, every quadric in the fast tree (no analytic prologue): t, normal and material bit-equal to the
    oracle, the reported shape consistent, at least the rays raycast_needs_exact selects counted as exact walks, and
    the same answers with every ray forced to the exact walk"""
    monkeypatch.setenv("ORT_ANALYTIC_PROLOGUE", "0")
    scene = _threshold_scene(api, small).commit()
    monkeypatch.delenv("ORT_ANALYTIC_PROLOGUE")
    scene.upload(0)
    flat = scene.flatten(64, 48)
    cam = np.array([scene.info().camera_p.x, scene.info().camera_p.y, scene.info().camera_p.z], "<f4")
    lo, hi = _scene_box(flat, cam)
    if small:
        assert float(np.linalg.norm((hi - lo).astype(np.float64))) < 1.0
    rays = _threshold_rays(flat, cam, np.random.default_rng(99 + small), (0.03, 0.08) if small else (0.4, 2.5))
    hits, st = scene.raycast(rays)
    t, nrm, mat = oracle.OracleScene(flat, with_reference_csg=False).raycast(rays[:, 0:3], rays[:, 3:6])
    assert_same_hits(hits, t, nrm, mat, "thresholds (%s)" % ("small" if small else "room"))
    # the reported shape: none exactly for the misses, else one whose material is the hit's
    missed = hits["t"] == FLT_MAX
    assert ((hits["prim"] == api.NO_PRIM) == missed).all()
    kind, index = api.decode_prim(hits["prim"][~missed])
    table = {api.HIT_SPHERE: flat.spheres, api.HIT_BOX: flat.boxes, api.HIT_CYLINDER: flat.cylinders}
    for k, arr in table.items():
        sel = kind == k
        assert (arr["mat"][index[sel]] == hits["mat"][~missed][sel]).all()
    assert (kind != api.HIT_TRIANGLE).all()
    need = _needs_exact(rays, lo, hi, len(flat.spheres) > 0, len(flat.spheres) + len(flat.cylinders) > 0)
    assert 0 < need.sum() < len(rays)
    assert st["fallback_rays"] >= need.sum(), (st["fallback_rays"], int(need.sum()))
    # the fast tree really answers the rays at |d|^2 >= 0.999 from inside the box
    assert (~need).sum() > len(rays) // 3
    monkeypatch.setenv("ORT_DEBUG_FORCE_FALLBACK", "0")
    exact, st_x = scene.raycast(rays)
    monkeypatch.delenv("ORT_DEBUG_FORCE_FALLBACK")
    assert st_x["fallback_rays"] == len(rays)
    assert exact.tobytes() == hits.tobytes()
    scene.close()
