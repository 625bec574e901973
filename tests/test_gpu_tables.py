"""The kernels that read the small tables (materials, light types, prologue shapes, the tree's top) from HBM instead of LDS
-- every render and ray-query kernel has such a TABS = false form -- and the scenes at and past the caps of those tables
(48 materials with index 0, 64 lights, 40 float4 of prologue shapes: csrc/ort_plan.h, table_fit_flags).  Two ways in: the
knob ORT_LDS_TABLES=0 on the repository's scenes, and scenes that leave the tables by themselves (tools/make_tablescene.py;
their counts are cap and cap + 1 of the numbers tests/test_launch_plan.py pins, which also shows what each one selects).
Everything bit for bit: the reference's own pixels and hits (tests/golden/*_tables_*.npz) and the oracle."""
import os

import numpy as np
import pytest

import raycast_cases
import table_scenes
from conftest import GOLDEN, assert_bits_equal
from test_gpu_raycast import assert_same_hits, mixed_rays
from test_gpu_raycast_edges import check_records
from test_oracle_golden import SCENES_C5

pytestmark = pytest.mark.gpu

FORCE_ALL = {"ORT_EXCHANGE": "1", "ORT_WAVES5": "1", "ORT_WIDE": "1"}
SIZES = [("chunk", 93, 61, 8, 4), ("pixel", 45, 35, 5, 0)]   # both with ragged 8x8 edge blocks
ALL = ["at_caps", "mats_over", "mats_over_diffuse", "lights_over", "ref_limits", "beyond_ref"]


# ---- ORT_LDS_TABLES=0 on the repository's scenes -------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES_C5)
def test_hbm_form_matches_reference_goldens(api, manifest, gpu_scene, monkeypatch, name):
    """ORT_LDS_TABLES=0: pt_persistent<false, false, false> (all lobes) or pt_persistent<false, true, false> (scenes without a
    specular or transmissive material, such as the bunny and dwarf rooms), implicit job spaces (PIXEL, CHUNK) and explicit jobs (TILE32, WHOLE),
    == the reference's own image, every seeding policy"""
    z = np.load(os.path.join(GOLDEN, "renders_%s.npz" % name))
    scene = gpu_scene(name)
    monkeypatch.setenv("ORT_LDS_TABLES", "0")
    entries = [e for e in manifest["renders"] if e["scene"] == name]
    assert entries
    for e in entries:
        policy = "chunk" if e["policy"] == "sample" else e["policy"]
        img, _ = scene.render(e["width"], e["height"], e["spp"], e["seed"], policy, chunk=e["chunk"])
        assert_bits_equal(img, z[e["key"]], "%s %s" % (name, e["key"]))


@pytest.mark.parametrize("name", SCENES_C5)
@pytest.mark.parametrize("policy,w,h,spp,chunk", [("chunk", 96, 64, 16, 4), ("pixel", 80, 50, 6, 0)])
def test_hbm_form_matches_oracle_and_lds_form(api, oracle, gpu_scene, monkeypatch, name, policy, w, h, spp, chunk):
    """ORT_LDS_TABLES=0, counters off: pt_persistent<false, false, false> / <false, true, false>; counters on: the counters
    kernel pt_persistent<true, false, false>.  Same image as the oracle and as the same render with the tables in LDS; same
    rays, paths and exact re-casts in both forms."""
    scene = gpu_scene(name)
    ref, ost = oracle.OracleScene(scene.flatten(w, h)).render(w, h, spp, 4242, policy, chunk=max(chunk, 1), threads=16)
    for counters in (False, True):
        monkeypatch.delenv("ORT_LDS_TABLES", raising=False)
        lds, st_lds = scene.render(w, h, spp, 4242, policy, chunk=chunk, counters=counters)
        monkeypatch.setenv("ORT_LDS_TABLES", "0")
        hbm, st = scene.render(w, h, spp, 4242, policy, chunk=chunk, counters=counters)
        assert_bits_equal(hbm, ref, "%s %s counters=%s, tables in HBM vs the oracle" % (name, policy, counters))
        assert_bits_equal(hbm, lds, "%s %s counters=%s, tables in HBM vs in LDS" % (name, policy, counters))
        assert st["fallback_rays"] == st_lds["fallback_rays"]
        if counters:
            assert st["paths"] == st_lds["paths"] == w * h * spp == ost["paths"]
            assert st["rays"] == st_lds["rays"] == ost["rays"]


@pytest.mark.parametrize("name", ["testscene", "c3_bunny_room"])
def test_hbm_form_through_the_reference_order_walk(api, oracle, gpu_scene, monkeypatch, name):
    """ORT_LDS_TABLES=0 with ORT_DEBUG_FORCE_FALLBACK=0 (every ray re-cast exactly) and 0xf (1/16, both walks inside a wave):
    resolve_hit's re-traversals (the prologue with HAS_EXCL, the un-cached treelet) and the exact walk inside
    pt_persistent<true, false, false> and pt_persistent<false, *, false>"""
    scene = gpu_scene(name)
    w, h, spp = 64, 40, 4
    ref, ost = oracle.OracleScene(scene.flatten(w, h)).render(w, h, spp, 77, "chunk", chunk=2, threads=16)
    monkeypatch.setenv("ORT_LDS_TABLES", "0")
    monkeypatch.setenv("ORT_DEBUG_FORCE_FALLBACK", "0")
    img, st = scene.render(w, h, spp, 77, "chunk", chunk=2, counters=True)
    assert st["fallback_rays"] == st["rays"] == ost["rays"]
    assert_bits_equal(img, ref, "all rays re-cast, counters")
    img, _ = scene.render(w, h, spp, 77, "chunk", chunk=2)
    assert_bits_equal(img, ref, "all rays re-cast")
    monkeypatch.setenv("ORT_DEBUG_FORCE_FALLBACK", "0xf")
    img, st = scene.render(w, h, spp, 77, "chunk", chunk=2, counters=True)
    assert 0 < st["fallback_rays"] < st["rays"]
    assert_bits_equal(img, ref, "1/16 of the rays re-cast, counters")
    img, _ = scene.render(w, h, spp, 77, "pixel")
    ref_p, _ = oracle.OracleScene(scene.flatten(w, h)).render(w, h, spp, 77, "pixel", threads=16)
    assert_bits_equal(img, ref_p, "1/16 of the rays re-cast, PIXEL")


@pytest.mark.parametrize("name", ["glass_room", "c4_dwarf_room"])
def test_hbm_form_explicit_jobs(api, oracle, gpu_scene, monkeypatch, name):
    """ORT_LDS_TABLES=0, explicit jobs (ort_tiled_raytrace_batch, and TILE32 as main() schedules it): the explicit-job mode of
    pt_persistent<false, false, false> (glass room) and <false, true, false> (dwarf room); images and every job's final
    RandomSeries state against the oracle"""
    scene = gpu_scene(name)
    monkeypatch.setenv("ORT_LDS_TABLES", "0")
    w, h = 40, 30
    jobs = np.zeros(5, api.JOB_DTYPE)
    jobs[0] = (0, 0, 8, 8, 11, 2)
    jobs[1] = (8, 0, 40, 3, 12, 1)
    jobs[2] = (5, 10, 5, 20, 13, 4)      # empty rect
    jobs[3] = (39, 29, 40, 30, 0xFFFFFFFF, 7)
    jobs[4] = (0, 29, 39, 30, 1, 3)
    out = np.zeros((h, w, 3), "<f4")
    finals, _ = scene.tiled_raytrace_batch(out, jobs)
    ref = np.zeros((h, w, 3), "<f4")
    osc = oracle.OracleScene(scene.flatten(w, h))
    for i, j in enumerate(jobs):
        _, s = osc.tiled_raytrace(ref, int(j["x0"]), int(j["y0"]), int(j["x1"]), int(j["y1"]), int(j["rng_state"]), int(j["spp"]))
        assert finals[i] == s, i
    assert_bits_equal(out, ref, name + " batch")
    img, _ = scene.render(70, 45, 2, 12345, "tile32")
    want, _ = oracle.OracleScene(scene.flatten(70, 45)).render(70, 45, 2, 12345, "tile32", threads=16)
    assert_bits_equal(img, want, name + " tile32")


# ---- scenes that leave the tables by themselves ---------------------------------------------------------------------------
_cache = {}


@pytest.fixture()
def table_scene(api, oracle, tmp_path_factory, monkeypatch):
    """(variant, prologue budget or None) -> (uploaded scene, oracle-scene factory); cached for the module"""
    def get(variant, prologue=None):
        key = (variant, prologue)
        if key not in _cache:
            scene, _, csg = table_scenes.build(api, variant, tmp_path_factory.mktemp("tables_" + variant))
            if prologue is not None:
                monkeypatch.setenv("ORT_ANALYTIC_PROLOGUE", str(prologue))   # read by build_tree at commit
            scene.commit()
            monkeypatch.delenv("ORT_ANALYTIC_PROLOGUE", raising=False)
            assert api.device_count() >= 1
            scene.upload(0)
            _cache[key] = (scene, csg)
        scene, csg = _cache[key]
        return scene, (lambda w, h: oracle.OracleScene(scene.flatten(w, h), with_reference_csg=csg))
    return get


@pytest.mark.parametrize("variant", table_scenes.GOLDEN_VARIANTS)
def test_table_scenes_match_reference_goldens(api, manifest, table_scene, variant):
    """at_caps (48 materials, 64 lights: the last float4 of the material and light slots in use) runs the table kernels;
    mats_over (49), lights_over (65) and ref_limits (100 / 100) run pt_persistent<false, false, false> by themselves: the
    reference's own pixels in every seeding policy, and its closest hits"""
    scene, _ = table_scene(variant)
    z = np.load(os.path.join(GOLDEN, "renders_tables_%s.npz" % variant))
    entries = manifest["tablescenes"][variant]["renders"]
    assert len(entries) == 4
    for e in entries:
        img, _ = scene.render(e["width"], e["height"], e["spp"], e["seed"], e["policy"], chunk=e["chunk"])
        assert_bits_equal(img, z[e["key"]], "%s %s" % (variant, e["key"]))
    r = np.load(os.path.join(GOLDEN, "raycast_tables_%s.npz" % variant))
    hits, _ = scene.raycast(r["rays"])
    assert_same_hits(hits, r["t"], r["n"], r["mat"], variant + " raycast goldens")


@pytest.mark.parametrize("variant", ALL)
def test_table_scenes_match_oracle(api, oracle, table_scene, variant):
    """Past a cap the default plan takes pt_persistent<false, false, false> (mats_over, lights_over, ref_limits, beyond_ref:
    300 materials, 200 lights), pt_persistent<false, true, false> (mats_over_diffuse: 49 diffuse materials) and, with
    counters, pt_persistent<true, false, false>; at_caps stays on the table kernels.  PIXEL and CHUNK at sizes with ragged
    edge blocks, counters on and off, the union of three shards, and three packed shards un-permuted.  The scene's
    conditions (a quarter of the primary hits past material 48, the last material seen, the light types) are asserted
    from the oracle first."""
    import torch
    scene, osc_at = table_scene(variant)
    flat = scene.flatten(table_scenes.W, table_scenes.H)
    table_scenes.assert_conditions(variant, scene, osc_at(table_scenes.W, table_scenes.H), flat)
    for policy, w, h, spp, chunk in SIZES:
        ref, ost = osc_at(w, h).render(w, h, spp, 4242, policy, chunk=max(chunk, 1), threads=16)
        img, _ = scene.render(w, h, spp, 4242, policy, chunk=chunk)
        assert_bits_equal(img, ref, "%s %s" % (variant, policy))
        img, st = scene.render(w, h, spp, 4242, policy, chunk=chunk, counters=True)
        assert_bits_equal(img, ref, "%s %s counters" % (variant, policy))
        assert st["paths"] == w * h * spp == ost["paths"] and st["rays"] == ost["rays"]
        acc = np.zeros_like(ref)
        full = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        for r in range(3):
            part, _ = scene.render(w, h, spp, 4242, policy, chunk=chunk, shard=(r, 3))
            assert not ((part != 0).any(axis=2) & (acc != 0).any(axis=2)).any(), "shards overlap"
            acc += part
            n = api.shard_block_count(w, h, r, 3)
            packed = torch.full((max(1, n), 64, 3), -1.0, dtype=torch.float32, device="cuda")
            scene.render_device(packed.data_ptr(), api.Scene.params(w, h, spp, 4242, policy, chunk=chunk, shard=(r, 3), packed=True), want_stats=True)
            api.unpack_blocks_device(packed.data_ptr(), w, h, r, 3, full.data_ptr())
        torch.cuda.synchronize()
        assert_bits_equal(acc, ref, "%s %s union of 3 shards" % (variant, policy))
        assert_bits_equal(full.cpu().numpy(), ref, "%s %s 3 packed shards un-permuted" % (variant, policy))


def test_at_the_caps_every_family_reads_the_last_slot(api, table_scene, monkeypatch):
    """at_caps: material 47 is the last record of the LDS material slot (the tree's top nodes follow it), light 63 the last flag
    of the light slot (the materials follow).  LDS form == HBM form (ORT_LDS_TABLES=0), == the ray exchange (tables next to
    the stashes), == the five-waves build (tables next to a shorter stack), == the four-waves plain loop"""
    scene, osc_at = table_scene("at_caps")
    for policy, w, h, spp, chunk in SIZES:
        ref, _ = osc_at(w, h).render(w, h, spp, 99, policy, chunk=max(chunk, 1), threads=16)
        for env in ({}, {"ORT_LDS_TABLES": "0"}, {"ORT_EXCHANGE": "1"}, {"ORT_EXCHANGE": "0", "ORT_WAVES5": "1"}, {"ORT_EXCHANGE": "0", "ORT_WAVES5": "0"},
                    {"ORT_WIDE": "1"}):
            for k in FORCE_ALL.keys() | {"ORT_LDS_TABLES"}:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            img, _ = scene.render(w, h, spp, 99, policy, chunk=chunk)
            assert_bits_equal(img, ref, "at_caps %s %s" % (policy, env))


@pytest.mark.parametrize("variant", ALL[1:])
def test_requests_past_the_caps_fall_back_to_the_plain_loop(api, table_scene, monkeypatch, variant):
    """ORT_EXCHANGE=1, ORT_WAVES5=1, ORT_WIDE=1 on a scene past a cap: none of them has a TABS = false build, the plan stays
    with pt_persistent<false, *, false> (test_launch_plan.py) and the image is still the oracle's"""
    scene, osc_at = table_scene(variant)
    policy, w, h, spp, chunk = SIZES[0]
    ref, _ = osc_at(w, h).render(w, h, spp, 5, policy, chunk=chunk, threads=16)
    for k, v in FORCE_ALL.items():
        monkeypatch.setenv(k, v)
    img, _ = scene.render(w, h, spp, 5, policy, chunk=chunk)
    assert_bits_equal(img, ref, variant)


# ---- ray queries --------------------------------------------------------------------------------------------------------
def _check_rays(api, scene, osc, flat, name, n=20000):
    rays, _ = mixed_rays(scene, "tables " + name, n)
    edge, _ = raycast_cases.cases(flat, lambda r: osc.raycast(r[:, 0:3], r[:, 3:6])[0])
    for what, rr in (("mixed rays", rays), ("edge rays", edge)):
        t, nrm, mat = osc.raycast(rr[:, 0:3], rr[:, 3:6])
        plain, st0 = scene.raycast(rr)
        counted, st1 = scene.raycast(rr, counters=True)
        raycast_cases.assert_same_answers(plain["t"], plain["n"], plain["mat"], t, nrm, mat, "%s, %s" % (name, what))
        assert counted.tobytes() == plain.tobytes() and st1["rays"] == len(rr) and st0["fallback_rays"] == st1["fallback_rays"]
        check_records(api, scene, flat, rr, plain, "%s, %s" % (name, what))
    return rays


@pytest.mark.parametrize("variant", ALL)
def test_ray_queries_on_the_table_scenes(api, table_scene, variant):
    """20 000 rays drawn as test_gpu_raycast.test_against_oracle_at_scale draws them and the hostile rays of raycast_cases.py:
    t, normal and material against the oracle, the reported shape re-intersected alone, counters on and off.  (These scenes
    keep their prologue in LDS -- raycast_rays<*, true>; the materials of the hits come from the shapes, past index 48.)"""
    scene, osc_at = table_scene(variant)
    flat = scene.flatten(64, 64)
    rays = _check_rays(api, scene, osc_at(64, 64), flat, variant)
    hits, _ = scene.raycast(rays)
    if variant in table_scenes.OVER_MATS:
        assert (hits["mat"] >= table_scenes.caps()["materials"]).sum() > 200


@pytest.mark.parametrize("budget,slots_fit", [(40, False), (21, False), (20, True)])
def test_prologue_past_its_cap(api, table_scene, monkeypatch, budget, slots_fit):
    """pro_over committed under ORT_ANALYTIC_PROLOGUE=40 and 21: 40 resp. 21 boxes in the prologue, 80 / 42 float4 where
    the LDS slot holds 40, so TAB_PRO is missing: the ray queries run raycast_rays<false, false> and, with counters,
    raycast_rays<true, false>; the renders pt_persistent<false, false, false> / <true, false, false> with the prologue read
    from HBM (prologue_tests<*, false>; its HAS_EXCL form in the re-traversals that ORT_DEBUG_FORCE_FALLBACK=0xf provokes).
    Under ORT_ANALYTIC_PROLOGUE=20 the prologue's 20 boxes fill the slot to its last float4 and everything stays in LDS."""
    scene, osc_at = table_scene("pro_over", budget)
    si = scene.info()
    assert scene.tree_info()["prologue_prims"] == budget <= si.box_count   # boxes are the cheapest kind: the prologue holds boxes alone
    assert (2 * budget <= table_scenes.caps()["pro_slots"]) == slots_fit
    flat = scene.flatten(64, 64)
    osc = osc_at(64, 64)
    rays = _check_rays(api, scene, osc, flat, "pro_over/%d" % budget, n=20000 if budget == 40 else 6000)
    fast, st_fast = scene.raycast(rays)
    monkeypatch.setenv("ORT_DEBUG_FORCE_FALLBACK", "0")
    exact, st = scene.raycast(rays, counters=True)
    assert st["fallback_rays"] == len(rays) >= st_fast["fallback_rays"]
    assert exact.tobytes() == fast.tobytes()
    for mask in (None, "0xf"):
        if mask:
            monkeypatch.setenv("ORT_DEBUG_FORCE_FALLBACK", mask)
        else:
            monkeypatch.delenv("ORT_DEBUG_FORCE_FALLBACK")
        for policy, w, h, spp, chunk in SIZES:
            ref, ost = osc_at(w, h).render(w, h, spp, 31, policy, chunk=max(chunk, 1), threads=16)
            img, _ = scene.render(w, h, spp, 31, policy, chunk=chunk)
            assert_bits_equal(img, ref, "pro_over/%d %s mask %s" % (budget, policy, mask))
            img, st = scene.render(w, h, spp, 31, policy, chunk=chunk, counters=True)
            assert_bits_equal(img, ref, "pro_over/%d %s mask %s counters" % (budget, policy, mask))
            assert st["rays"] == ost["rays"] and (mask is None or 0 < st["fallback_rays"] < st["rays"])
