"""Closest-hit ray queries on rays no render casts (tests/raycast_cases.py): non-finite, zero, extreme and grazing
directions, far origins.  The device must give the reference's answer for every IEEE-754 ray (include/ort.h): every
non-NaN output bit for bit, a NaN where the reference has one.  The goldens (raycast_edges_<scene>.npz) are the
reference's own answers; at scale the oracle stands in for it."""
import os

import numpy as np
import pytest

import raycast_cases
import ref_io
from conftest import GOLDEN
from raycast_cases import FLT_MAX, assert_same_answers
from test_gpu_raycast import SCENES, UNIT_OPS, _threshold_scene, golden_like, torch_raycast

pytestmark = pytest.mark.gpu

NONFINITE, ZERO = raycast_cases.CATEGORIES.index("nonfinite"), raycast_cases.CATEGORIES.index("zero")


def golden(name):
    return np.load(os.path.join(GOLDEN, "raycast_edges_%s.npz" % name))


def check_records(api, scene, flat, rays, hits, what):
    """a miss is exactly FLT_MAX / 0 / 0 / NO_PRIM; a hit's shape, intersected alone by the device's generic
    intersectors (unit_eval_device ops 1-4), gives the same t and (normalised, op 10) normal, and has the hit's
    material"""
    missed = hits["t"].view("<u4") == FLT_MAX.view("<u4")
    assert (hits["n"][missed].view("<u4") == 0).all() and (hits["mat"][missed] == 0).all(), what
    assert (hits["prim"][missed] == api.NO_PRIM).all(), what
    assert (hits["prim"][~missed] != api.NO_PRIM).all(), what
    sel = np.flatnonzero(~missed)
    if len(sel) == 0:
        return
    kind, index = api.decode_prim(hits["prim"][sel])
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
    recs = np.zeros(len(sel), dtype=ref_io.UNIT_REC_DTYPE)
    recs["op"] = np.vectorize(UNIT_OPS.get)(kind)
    recs["a"] = rows
    got = api.unit_eval_device(recs)
    nrm = np.zeros((len(sel), 24), "<f4")
    nrm[:, 0:3] = got[:, 1:4]
    unit = api.unit_eval_device(ref_io.make_unit_records(10, nrm))
    assert_same_answers(got[:, 0], unit[:, 0:3], mat, hits["t"][sel], hits["n"][sel], hits["mat"][sel],
                        what + ", the reported shape alone")


@pytest.mark.parametrize("name", SCENES)
def test_edge_goldens(api, gpu_scene, name):
    """the reference's own answers for ~1 500 hostile rays per scene: host form and device form (torch, non-default
    stream), the same records from both, and every record consistent with the shape it names"""
    z = golden(name)
    scene = gpu_scene(name)
    hits, _ = scene.raycast(z["rays"])
    for c, what in enumerate(raycast_cases.CATEGORIES):
        sel = z["category"] == c
        assert_same_answers(hits["t"][sel], hits["n"][sel], hits["mat"][sel], z["t"][sel], z["n"][sel], z["mat"][sel],
                            "%s host form, %s rays" % (name, what))
    dh, _ = torch_raycast(scene, z["rays"])
    assert dh.tobytes() == hits.tobytes()
    check_records(api, scene, scene.flatten(64, 64), z["rays"], hits, name)


def _scale_case(api, gpu_scene, monkeypatch, name):
    if name.startswith("threshold_"):
        monkeypatch.setenv("ORT_ANALYTIC_PROLOGUE", "0")  # every quadric in the fast tree
        scene = _threshold_scene(api, name == "threshold_small").commit()
        monkeypatch.delenv("ORT_ANALYTIC_PROLOGUE")
        scene.upload(0)
        return scene, scene.flatten(64, 48), False
    return gpu_scene(name), gpu_scene(name).flatten(64, 64), True


@pytest.mark.parametrize("name,scale", [(s, 13) for s in SCENES] + [("c5_heightfield_224", 3), ("threshold_room", 13),
                                                                     ("threshold_small", 13)])
def test_edges_against_oracle_at_scale(api, oracle, gpu_scene, monkeypatch, name, scale):
    """~20 000 seeded hostile rays per scene (~4 500 on the 99 458-triangle height field) against the oracle, which is
    bit-equal to the reference on these rays (test_oracle_golden.py); also the two threshold scenes with every quadric
    in the fast tree"""
    scene, flat, cached = _scale_case(api, gpu_scene, monkeypatch, name)
    osc = oracle.OracleScene(flat, with_reference_csg=cached)
    rays, cat = raycast_cases.cases(flat, lambda r: osc.raycast(r[:, 0:3], r[:, 3:6])[0], seed=1, scale=scale)
    hits, _ = scene.raycast(rays)
    t, n, mat = osc.raycast(rays[:, 0:3], rays[:, 3:6])
    for c, what in enumerate(raycast_cases.CATEGORIES):
        sel = cat == c
        assert_same_answers(hits["t"][sel], hits["n"][sel], hits["mat"][sel], t[sel], n[sel], mat[sel],
                            "%s, %s rays" % (name, what))
    check_records(api, scene, flat, rays, hits, name)
    if not cached:
        scene.close()


def test_routes_and_forced_exact_walk(api, gpu_scene, monkeypatch):
    """which walk the non-finite and zero rays take (stats fallback_rays counts the exact walks): in the scenes with
    quadrics in the fast tree every ray with d = (+-0, +-0, +-0) or a NaN takes the exact walk (raycast_needs_exact:
    |d|^2 short of the tree's threshold or NaN, or an origin not inside the scene's box); others take the fast tree
    (infinite direction components, whose 1/d is 0; single-axis directions and NaN or infinite origins where the tree
    holds no quadrics or boxes), so both walks are exercised.  Every ray forced to the exact walk gives the same records."""
    routes = {}
    for name in SCENES:
        z = golden(name)
        scene = gpu_scene(name)
        cat, rays = z["category"], z["rays"]
        null_dir = (rays[:, 3:6] == 0).all(axis=1)
        zero_or_nan = ((cat == ZERO) & null_dir) | ((cat == NONFINITE) & np.isnan(rays).any(axis=1))
        either = (cat == ZERO) | (cat == NONFINITE)
        _, st_a = scene.raycast(rays[zero_or_nan])
        _, st_b = scene.raycast(rays[either])
        routes[name] = ((st_a["fallback_rays"], int(zero_or_nan.sum())), (st_b["fallback_rays"], int(either.sum())))
        monkeypatch.setenv("ORT_DEBUG_FORCE_FALLBACK", "0")
        exact, st_x = scene.raycast(rays)
        monkeypatch.delenv("ORT_DEBUG_FORCE_FALLBACK")
        assert st_x["fallback_rays"] == len(rays)
        fast, _ = scene.raycast(rays)
        assert exact.tobytes() == fast.tobytes(), name
    print("exact walks (null-direction or NaN rays; non-finite and zero rays), per scene:", routes)
    assert any(a[0] == a[1] for a, _ in routes.values()), routes
    assert all(b[0] < b[1] for _, b in routes.values()), routes


def axis_rays(rng, n):
    """golden_like origins along +-x, +-y or +-z, the other two components +0 or -0 (height probes, orthographic
    views)"""
    rays = golden_like(rng, n)
    axis = rng.integers(0, 3, n)
    d = np.where(rng.random((n, 3)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype("<f4")
    d[np.arange(n), axis] = np.where(rng.random(n) < 0.5, np.float32(-1), np.float32(1))
    rays[:, 3:6] = d
    return rays


@pytest.mark.parametrize("name", ["c3_bunny_room", "c4_dwarf_room", "letters", "c5_heightfield_224"])
def test_axis_aligned_rays_take_the_fast_tree(api, oracle, gpu_scene, monkeypatch, name):
    """unit directions along an axis, +-0 elsewhere (1/d infinite in two components), in scenes whose boxes are all in
    the analytic prologue: the fast tree answers them (raycast_needs_exact routes such rays only when the fast tree
    holds boxes), with the reference's answers, the same as the exact walk's; origins exactly on the shapes' planes
    (box faces, cylinder ends, the height field's vertex coordinates) among them"""
    scene = gpu_scene(name)
    rng = np.random.default_rng(len(name) * 7)
    n = 1 << 16
    rays = axis_rays(rng, n)
    flat = scene.flatten(64, 64)
    planes = raycast_cases._planes(flat)  # a quarter of the origins on a box face / cylinder end / vertex coordinate
    for i in range(n // 4):
        a, v = planes[rng.integers(0, len(planes))]
        rays[i, a] = v
        rays[i, 3:6] = 0
        rays[i, 3 + (a + 1 + rng.integers(0, 2)) % 3] = np.float32(1) if rng.random() < 0.5 else np.float32(-1)
        if rng.random() < 0.5:
            rays[i, 3 + a] = np.float32(-0.0)
    hits, st = scene.raycast(rays)
    assert st["fallback_rays"] * 100 < n, (st["fallback_rays"], n)
    monkeypatch.setenv("ORT_DEBUG_FORCE_FALLBACK", "0")
    exact, _ = scene.raycast(rays)
    monkeypatch.delenv("ORT_DEBUG_FORCE_FALLBACK")
    assert exact.tobytes() == hits.tobytes()
    sel = np.concatenate([np.arange(3000), rng.choice(np.arange(3000, n), 3000, replace=False)])
    t, nrm, mat = oracle.OracleScene(flat).raycast(rays[sel, 0:3], rays[sel, 3:6])
    assert_same_answers(hits["t"][sel], hits["n"][sel], hits["mat"][sel], t, nrm, mat, name + " axis-aligned rays")


@pytest.mark.parametrize("name", ["testscene", "c3_bunny_room"])
def test_no_cross_lane_effects(api, gpu_scene, name):
    """hostile rays at lanes 0, 63, 64, 65, the last index and random places among 2^20 ordinary rays: every ordinary
    record byte-identical to the run without them, every hostile record the one it gets when cast alone"""
    z = golden(name)
    scene = gpu_scene(name)
    rng = np.random.default_rng(31 + len(name))
    n = 1 << 20
    plain = golden_like(rng, n)
    ref, _ = torch_raycast(scene, plain)
    hostile = z["rays"]
    alone = np.zeros(len(hostile), api.HIT_DTYPE)
    pick = np.concatenate([np.arange(8), rng.choice(len(hostile), 56, replace=False)])
    for i in pick:
        alone[i] = scene.raycast(hostile[i:i + 1])[0][0]
    batch, _ = scene.raycast(hostile)
    assert batch[pick].tobytes() == alone[pick].tobytes()
    places = np.concatenate([[0, 63, 64, 65, n - 1], rng.choice(np.arange(66, n - 1), len(hostile) - 5, replace=False)])
    mixed = plain.copy()
    mixed[places] = hostile
    got, _ = torch_raycast(scene, mixed)
    ordinary = np.ones(n, bool)
    ordinary[places] = False
    assert got[ordinary].tobytes() == ref[ordinary].tobytes()
    assert got[places].tobytes() == batch.tobytes()
    assert_same_answers(got["t"][places], got["n"][places], got["mat"][places], z["t"], z["n"], z["mat"],
                        name + " hostile rays among ordinary ones")
    # the hostile rays packed together at the front, every lane of the first waves hostile
    front = plain.copy()
    front[: len(hostile)] = hostile
    got, _ = scene.raycast(front)
    assert got[: len(hostile)].tobytes() == batch.tobytes()
    assert got[len(hostile):].tobytes() == ref[len(hostile):].tobytes()


@pytest.mark.parametrize("name", ["testscene", "c3_bunny_room", "rand_b"])
def test_edges_with_counters(api, gpu_scene, name):
    z = golden(name)
    scene = gpu_scene(name)
    plain, _ = scene.raycast(z["rays"])
    hits, st = scene.raycast(z["rays"], counters=True)
    assert hits.tobytes() == plain.tobytes()
    assert st["rays"] == len(z["rays"])
