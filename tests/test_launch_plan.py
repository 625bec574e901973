"""The launch policy of the render call and of the ray queries (csrc/ort_plan.h: plan_render, plan_ray_query, plan_radiance)
without a device, through tools/launch_plan: which kernel, which grid, which thresholds.  Expected values are the defaults and crossovers of DESIGN.md sections 5-6 as the code states
them: SAH cost 0.09, 24 and 96 jobs per lane, 16 MB of fast tree, five waves for the all-lobes flavour and trees that leave the
L2.  The GPU tests compare images of forced variants (ORT_WAVES5, ORT_EXCHANGE, ORT_WIDE, ...); the tests here are what says
that each forcing really selects the kernel its test names, and which requests fall back silently."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

TOOL = os.path.join(ROOT, "tools", "launch_plan")
CU = 256
LANES = CU * 4 * 256  # four workgroups of 256 lanes per compute unit
KNOBS = ("ORT_DEBUG_FORCE_FALLBACK ORT_DEBUG_UTIL ORT_DEBUG_FALLBACK ORT_DEBUG_DRAIN ORT_CACHE_RESIDENT ORT_REFILL_BELOW ORT_DESCEND_BELOW "
         "ORT_MODE ORT_KERNEL ORT_LDS_TABLES ORT_EXCHANGE ORT_LONG_MIN ORT_LONG_REFILL ORT_INFLIGHT_CAP ORT_PARK_MIN ORT_LPT ORT_WIDE ORT_WAVES5 "
         "ORT_ENDGAME_JOBS ORT_BLOCKS_PER_CU ORT_JOB_BATCH ORT_BATCH_TAIL").split()


@pytest.fixture(scope="module")
def tool():
    src = [os.path.join(ROOT, "tools", "launch_plan.cpp"), os.path.join(ROOT, "include", "ort.h")]
    src += [os.path.join(ROOT, "offline_raytracer_amd", "csrc", h) for h in ("ort_plan.h", "ort_setup.h", "ort_scene.h")]
    if not os.path.exists(TOOL) or any(os.path.getmtime(s) > os.path.getmtime(TOOL) for s in src):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or (hipcc if os.path.exists(hipcc) else None)
        if cxx is None:
            pytest.skip("tools/launch_plan is not built and there is no C++ compiler to build it with")
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tools"), "launch_plan", "CXX=" + cxx])
    return TOOL


def plan(tool, env=None, **kw):
    """the plan for a 256-unit device; by default a diffuse scene with all tables, a 6 MB tree and a cheap one (SAH cost 0.05)"""
    args = dict(cu_count=CU, diffuse_only=1, fast_tree_bytes=6 << 20, sah_cost=0.05)
    args.update(kw)
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(env or {})
    r = subprocess.run([tool] + ["%s=%s" % kv for kv in args.items()], env=e, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def fill(tool, **kw):
    """-> (the plan, the fields of the RenderView that are not pointers as the shared fill sets them for it: fill=1)"""
    args = dict(cu_count=CU, diffuse_only=1, fast_tree_bytes=6 << 20, sah_cost=0.05, fill=1)
    args.update(kw)
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run([tool] + ["%s=%s" % kv for kv in args.items()], env=e, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    fields = dict(line.split(" = ") for line in lines[1:])
    assert len(fields) == len(lines) - 1 == 39
    return json.loads(lines[0]), {k: float(v) if k in ("rr", "ad_tolerance", "ad_floor") else int(v) for k, v in fields.items()}


def qplan(tool, query, count, env=None, **kw):
    """the QueryPlan of a ray query over count rays on the same device; by default the scene of plan()"""
    return plan(tool, env, query=query, count=count, **kw)


def kernel(p):
    """the plan's kernel in words"""
    if p["wavefront"]:
        return "wavefront"
    name = "five" if p["five"] else "exchange" if p["exchange"] else "wide" if p["wide"] else "plain"
    return name + "".join("+" + f for f in ("counters", "diffuse", "tabs", "implicit") if p[f])


HD = dict(width=1920, height=1080, chunk=64)   # 32 400 blocks of 8x8
UHD = dict(width=3840, height=2160, chunk=64)  # 129 600
SMALL = dict(width=256, height=256, spp=16, chunk=4)  # what the GPU parity tests render


# ---- the five BASELINE configurations ---------------------------------------------------------------------------------
def test_c3_headline_frame_runs_the_plain_loop_at_four_waves(tool):
    p = plan(tool, sah_cost=0.076, spp=1024, **HD)
    jobs = 32400 * 64 * 16
    assert kernel(p) == "plain+diffuse+tabs+implicit"
    assert (p["grid"], p["refill_below"], p["descend_below"], p["block_major"], p["job_batch"]) == (1024, 16, 8, 1, 128)
    assert p["job_count"] == jobs and jobs >= 96 * LANES
    assert p["batch_until"] == jobs - 16 * LANES  # batches of 128 stop 16 jobs per lane before the end
    assert p["partial_bytes"] == jobs * 12 and p["stash_bytes"] == 0 and p["drain_bytes"] == 0


def test_c3_eight_way_shard_draws_batches_of_64(tool):
    p = plan(tool, sah_cost=0.076, spp=1024, shard_index=0, shard_count=8, **HD)
    jobs = 4050 * 64 * 16  # 15.8 jobs per lane
    assert kernel(p) == "plain+diffuse+tabs+implicit" and p["grid"] == 1024
    assert (p["job_count"], p["job_batch"], p["batch_until"]) == (jobs, 64, jobs - 8 * LANES)


def test_c4_dwarf_room_takes_the_ray_exchange(tool):
    p = plan(tool, sah_cost=0.11, spp=512, **UHD)
    jobs = 129600 * 64 * 8
    assert kernel(p).startswith("exchange+diffuse") and p["grid"] == 1024
    assert (p["refill_below"], p["descend_below"], p["job_batch"]) == (24, 8, 128)
    assert p["endgame_from"] == jobs - 4 * LANES  # the stashes drain over the last four jobs per lane
    assert (p["capL"], p["capR"], p["long_min"], p["long_refill"], p["inflight_cap"], p["park_min"]) == (128, 192, 64, 32, 64, 1)
    # per wave: L records of 9 float4 and L stacks of 24 / 4 float4 for 128 paths, R records of 9 float4 for 192
    assert p["stash_wave_f4"] == (9 + 24 // 4) * 128 + 9 * 192
    assert p["stash_bytes"] == 1024 * 4 * p["stash_wave_f4"] * 16


def test_c2_all_lobes_scene_runs_five_waves(tool):
    p = plan(tool, diffuse_only=0, spp=1024, **HD)
    assert kernel(p) == "five+tabs+implicit" and p["grid"] == 5 * CU
    assert (p["refill_below"], p["descend_below"]) == (16, 8)


def test_c5_tree_out_of_the_l2_runs_five_waves_with_later_exits(tool):
    p = plan(tool, fast_tree_bytes=86 << 20, sah_cost=0.5, spp=4096, **UHD)  # SAH cost and launch length would earn the exchange
    assert kernel(p) == "five+diffuse+tabs+implicit" and p["grid"] == 5 * CU
    assert (p["refill_below"], p["descend_below"]) == (32, 16)


# ---- the crossovers, one step either side ----------------------------------------------------------------------------
def test_exchange_from_an_sah_cost_of_0_09(tool):
    assert plan(tool, sah_cost=0.09, spp=512, **UHD)["exchange"] == 1
    assert kernel(plan(tool, sah_cost=0.0899, spp=512, **UHD)) == "plain+diffuse+tabs+implicit"


def test_exchange_from_24_jobs_per_lane(tool):
    at = plan(tool, sah_cost=0.2, policy="pixel", width=3072, height=2048, spp=4)
    below = plan(tool, sah_cost=0.2, policy="pixel", width=3072, height=2040, spp=4)
    assert at["job_count"] == 24 * LANES and at["exchange"] == 1
    assert below["job_count"] == 24 * LANES - 384 * 64 and below["exchange"] == 0


def test_batches_of_128_from_96_jobs_per_lane(tool):
    at = plan(tool, width=3072, height=2048, spp=4, chunk=1)
    below = plan(tool, width=3072, height=2040, spp=4, chunk=1)
    assert at["job_count"] == 96 * LANES and (at["job_batch"], at["batch_until"]) == (128, 80 * LANES)
    assert (below["job_batch"], below["batch_until"]) == (64, below["job_count"] - 8 * LANES)


def test_cache_residency_ends_at_16_mb(tool):
    at = plan(tool, fast_tree_bytes=16 << 20, spp=1024, **HD)
    over = plan(tool, fast_tree_bytes=(16 << 20) + 1, spp=1024, **HD)
    assert (kernel(at), at["refill_below"], at["descend_below"]) == ("plain+diffuse+tabs+implicit", 16, 8)
    assert (kernel(over), over["refill_below"], over["descend_below"]) == ("five+diffuse+tabs+implicit", 32, 16)
    forced = plan(tool, {"ORT_CACHE_RESIDENT": "0"}, spp=1024, **HD)  # A/B runs
    assert (kernel(forced), forced["refill_below"], forced["descend_below"]) == ("five+diffuse+tabs+implicit", 32, 16)
    assert kernel(plan(tool, {"ORT_CACHE_RESIDENT": "1"}, fast_tree_bytes=86 << 20, spp=1024, **HD)) == "plain+diffuse+tabs+implicit"


# ---- what the GPU tests force is what they get ---------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["chunk", "pixel"])
def test_waves5_forces_the_five_waves_build(tool, policy):
    a = plan(tool, {"ORT_EXCHANGE": "0", "ORT_WAVES5": "0"}, policy=policy, **SMALL)
    b = plan(tool, {"ORT_EXCHANGE": "0", "ORT_WAVES5": "1"}, policy=policy, **SMALL)
    assert kernel(a) == "plain+diffuse+tabs+implicit" and kernel(b) == "five+diffuse+tabs+implicit"
    assert a["grid"] == b["grid"] == 1024 * (4 if policy == "chunk" else 1) * 64 // 256  # fewer jobs than resident lanes


def test_wide_needs_the_wide_tree(tool):
    assert kernel(plan(tool, {"ORT_WIDE": "1"}, has_wide=1, **SMALL)) == "wide+diffuse+tabs+implicit"
    assert kernel(plan(tool, {"ORT_WIDE": "1"}, has_wide=1, diffuse_only=0, **SMALL)) == "wide+tabs+implicit"
    assert kernel(plan(tool, {"ORT_WIDE": "1"}, has_wide=1, counters=1, **SMALL)) == "wide+counters+tabs"
    assert kernel(plan(tool, {"ORT_WIDE": "1"}, has_wide=0, **SMALL)) == "plain+diffuse+tabs+implicit"
    assert kernel(plan(tool, {"ORT_WIDE": "0"}, has_wide=1, **SMALL)) == "plain+diffuse+tabs+implicit"
    assert kernel(plan(tool, has_wide=1, **SMALL)) == "plain+diffuse+tabs+implicit"  # never by itself


def test_exchange_forced_needs_all_tables_and_an_implicit_job_space(tool):
    assert kernel(plan(tool, {"ORT_EXCHANGE": "1"}, **SMALL)).startswith("exchange+diffuse")
    assert kernel(plan(tool, {"ORT_EXCHANGE": "1"}, policy="pixel", **SMALL)).startswith("exchange+diffuse")
    assert kernel(plan(tool, {"ORT_EXCHANGE": "1"}, diffuse_only=0, **SMALL)).startswith("exchange+tabs")  # all lobes, when asked
    assert plan(tool, {"ORT_EXCHANGE": "1"}, **SMALL)["refill_below"] == 24
    assert plan(tool, {"ORT_EXCHANGE": "1", "ORT_REFILL_BELOW": "16"}, **SMALL)["refill_below"] == 16
    for missing in (1, 2, 8):  # TAB_PRO, TAB_LIGHTS, TAB_MATS
        assert kernel(plan(tool, {"ORT_EXCHANGE": "1"}, tab_flags=11 & ~missing, **SMALL)) == "plain+diffuse"
    assert kernel(plan(tool, {"ORT_EXCHANGE": "1", "ORT_LDS_TABLES": "0"}, **SMALL)) == "plain+diffuse"
    assert kernel(plan(tool, {"ORT_EXCHANGE": "1"}, explicit_jobs=1, job_count=1024)) == "plain+diffuse+tabs"
    assert kernel(plan(tool, {"ORT_EXCHANGE": "0"}, sah_cost=0.11, spp=512, **UHD)) == "plain+diffuse+tabs+implicit"
    # counters: only the diffuse flavour with the ORT_DEBUG_UTIL probes has an exchange build
    assert kernel(plan(tool, {"ORT_EXCHANGE": "1"}, counters=1, **SMALL)) == "plain+counters+tabs"
    assert kernel(plan(tool, {"ORT_EXCHANGE": "1", "ORT_DEBUG_UTIL": "1"}, counters=1, **SMALL)) == "exchange+counters+diffuse+tabs"


def test_the_other_forcings(tool):
    assert kernel(plan(tool, {"ORT_KERNEL": "general"}, **SMALL)) == "five+tabs+implicit"  # all lobes: five waves by itself
    assert kernel(plan(tool, {"ORT_KERNEL": "general", "ORT_WAVES5": "0"}, **SMALL)) == "plain+tabs+implicit"
    assert kernel(plan(tool, {"ORT_LDS_TABLES": "0"}, **SMALL)) == "plain+diffuse"
    assert kernel(plan(tool, {"ORT_LDS_TABLES": "0"}, diffuse_only=0, **SMALL)) == "plain"
    assert kernel(plan(tool, {"ORT_MODE": "wavefront"}, **SMALL)) == "wavefront"
    assert kernel(plan(tool, {"ORT_MODE": "persistent"}, **SMALL)) == "plain+diffuse+tabs+implicit"
    assert plan(tool, **SMALL)["block_major"] == 1 and plan(tool, {"ORT_LPT": "0"}, **SMALL)["block_major"] == 0
    assert plan(tool, policy="pixel", **SMALL)["block_major"] == 0 and plan(tool, width=256, height=256, spp=4, chunk=4)["block_major"] == 0
    p = plan(tool, {"ORT_JOB_BATCH": "0"}, **SMALL)
    assert (p["job_batch"], p["batch_until"]) == (0, p["job_count"])  # no tail to hold back: every draw goes to the counter anyway
    p = plan(tool, {"ORT_JOB_BATCH": "7", "ORT_BATCH_TAIL": "1"}, spp=1024, **HD)
    assert (p["job_batch"], p["batch_until"]) == (7, p["job_count"] - LANES)
    assert plan(tool, {"ORT_ENDGAME_JOBS": "0", "ORT_EXCHANGE": "1"}, **SMALL)["endgame_from"] == 1024 * 64 * 4


# ---- the silent fall-backs, stated as such -------------------------------------------------------------------------------
def test_no_five_waves_when_the_two_units_disagree_on_the_argument_layout(tool):
    for env in ({"ORT_EXCHANGE": "0", "ORT_WAVES5": "1"}, {}):
        assert kernel(plan(tool, env, diffuse_only=0, w5_layout_ok=0, **SMALL)) == "plain+tabs+implicit"
    assert plan(tool, fast_tree_bytes=86 << 20, w5_layout_ok=0, **SMALL)["five"] == 0


def test_no_five_waves_next_to_a_wide_or_exchange_request_or_without_tables(tool):
    for env in ({"ORT_WIDE": "1"}, {"ORT_EXCHANGE": "1"}, {"ORT_LDS_TABLES": "0"}, {"ORT_MODE": "wavefront"}):
        assert plan(tool, dict(env, ORT_WAVES5="1"), **SMALL)["five"] == 0, env
    assert plan(tool, {"ORT_WAVES5": "1"}, tab_flags=3, **SMALL)["five"] == 0


def test_counters_never_run_five_waves_or_the_implicit_variant(tool):
    for env in ({}, {"ORT_WAVES5": "1", "ORT_EXCHANGE": "0"}, {"ORT_DEBUG_UTIL": "1"}, {"ORT_KERNEL": "general"}):
        for diffuse_only in (0, 1):
            p = plan(tool, env, counters=1, diffuse_only=diffuse_only, **SMALL)
            assert (p["five"], p["implicit"], p["counters"]) == (0, 0, 1), env
    # the diffuse flavour with counters is the one with the probes
    assert kernel(plan(tool, counters=1, **SMALL)) == "plain+counters+tabs"
    assert kernel(plan(tool, {"ORT_DEBUG_UTIL": "1"}, counters=1, **SMALL)) == "plain+counters+diffuse+tabs"
    assert kernel(plan(tool, {"ORT_LDS_TABLES": "0"}, counters=1, **SMALL)) == "plain+counters"


def test_explicit_jobs_run_neither_exchange_nor_five_waves_nor_the_implicit_variant(tool):
    for env in ({}, {"ORT_EXCHANGE": "1"}, {"ORT_WAVES5": "1", "ORT_EXCHANGE": "0"}, {"ORT_WIDE": "1"}):
        for diffuse_only in (0, 1):
            p = plan(tool, env, explicit_jobs=1, job_count=100 * LANES, diffuse_only=diffuse_only, sah_cost=0.5, has_wide=1)
            assert kernel(p) == ("plain+diffuse+tabs" if diffuse_only else "plain+tabs"), env
            assert p["block_major"] == 0 and p["partial_bytes"] == 0
    assert kernel(plan(tool, {"ORT_WIDE": "1"}, explicit_jobs=1, job_count=1024, has_wide=1, counters=1)) == "wide+counters+tabs"


# ---- the caps of the LDS tables (table_fit_flags): what fits, and what a scene past a cap runs ---------------------------
FORCE_ALL = {"ORT_EXCHANGE": "1", "ORT_WAVES5": "1", "ORT_WIDE": "1"}
PLAIN_HBM = {(0, 1): "plain+diffuse", (0, 0): "plain", (1, 0): "plain+counters", (1, 1): "plain+counters"}  # (counters, diffuse_only)


def _at_and_over(tool, at, over, missing):
    """`at` fits its table and runs the table kernels; `over` loses the one table `missing` and with it the whole family:
    pt_persistent<false, true, false> / <false, false, false> / <true, false, false>, whatever is asked for"""
    for policy in ("chunk", "pixel"):
        a = plan(tool, policy=policy, has_wide=1, **at, **SMALL)
        assert a["tab_flags"] == 11 and kernel(a) == "plain+diffuse+tabs+implicit", at
        assert kernel(plan(tool, policy=policy, diffuse_only=0, **at, **SMALL)) == "five+tabs+implicit"
        assert kernel(plan(tool, {"ORT_EXCHANGE": "1"}, policy=policy, **at, **SMALL)).startswith("exchange+diffuse")
        assert plan(tool, {"ORT_WAVES5": "1", "ORT_EXCHANGE": "0"}, policy=policy, **at, **SMALL)["five"] == 1
        for env in ({}, FORCE_ALL):
            for (counters, diffuse_only), name in PLAIN_HBM.items():
                p = plan(tool, env, policy=policy, has_wide=1, counters=counters, diffuse_only=diffuse_only, **over, **SMALL)
                assert p["tab_flags"] == 11 & ~missing, over
                assert kernel(p) == name, (over, env, counters, diffuse_only)
                assert (p["exchange"], p["five"], p["wide"], p["implicit"], p["tabs"]) == (0, 0, 0, 0, 0)
    p = plan(tool, FORCE_ALL, explicit_jobs=1, job_count=4096, has_wide=1, **over)
    assert kernel(p) == "plain+diffuse" and kernel(plan(tool, explicit_jobs=1, job_count=4096, **at)) == "plain+diffuse+tabs"


def test_table_caps_are_the_lane_codes(tool):
    """the numbers the scenes of tests/table_scenes.py are built from (ort_kernels.hip asserts them equal to kTabMatCap, kTabLightCap, kTabProCap)"""
    assert plan(tool, **SMALL)["tab_caps"] == {"materials": 48, "lights": 64, "pro_slots": 40}
    assert plan(tool, **SMALL)["tab_flags"] == 11  # an empty scene fits everywhere


def test_48_materials_fit_and_49_do_not(tool):
    _at_and_over(tool, dict(materials=48), dict(materials=49), 8)


def test_64_lights_fit_and_65_do_not(tool):
    _at_and_over(tool, dict(lights=64), dict(lights=65), 2)


def test_40_prologue_slots_fit_and_41_do_not(tool):
    _at_and_over(tool, dict(pro_boxes=20), dict(pro_boxes=21), 1)            # boxes alone: two float4 each
    _at_and_over(tool, dict(pro_boxes=10, pro_spheres=4, pro_cyls=4), dict(pro_boxes=10, pro_spheres=5, pro_cyls=4), 1)  # 40, and 41 with an odd sphere count
    assert plan(tool, pro_boxes=10, pro_spheres=3, pro_cyls=4, **SMALL)["tab_flags"] == 11   # 39
    assert plan(tool, pro_cyls=10, **SMALL)["tab_flags"] == 11 and plan(tool, pro_cyls=10, pro_spheres=1, **SMALL)["tab_flags"] == 10
    assert plan(tool, pro_spheres=40, **SMALL)["tab_flags"] == 11 and plan(tool, pro_spheres=41, **SMALL)["tab_flags"] == 10


def test_each_table_is_judged_alone_and_an_explicit_tab_flags_wins(tool):
    assert plan(tool, materials=49, lights=65, pro_boxes=21, **SMALL)["tab_flags"] == 0
    assert plan(tool, materials=48, lights=64, pro_boxes=20, **SMALL)["tab_flags"] == 11
    assert plan(tool, materials=300, lights=200, **SMALL)["tab_flags"] == 1
    assert plan(tool, materials=300, tab_flags=11, **SMALL)["tab_flags"] == 11


def test_the_scenes_of_the_gpu_table_tests_select_what_their_docstrings_name(tool):
    """tests/test_gpu_tables.py: the variants of tools/make_tablescene.py (counts relative to the caps the tool prints) and the
    kernels they take by themselves; ORT_LDS_TABLES=0 on the repository's own scenes.  The ray queries read TAB_PRO alone
    (plan_ray_query): raycast_rays<*, false> and occluded_rays<*, false> where bit 1 of tab_flags is missing."""
    import table_scenes
    v = table_scenes.variants()
    for query in ("raycast", "occluded"):
        for name in ("mats_over", "mats_over_diffuse", "lights_over", "ref_limits", "beyond_ref"):  # past a cap the queries do not read
            q = qplan(tool, query, 4000, materials=v[name]["materials"], lights=v[name]["lights"])
            assert q["tab_flags"] & 1 and q["tab_flags"] != 11 and q["tabs"] == 1, (query, name)
        for pro_boxes, tabs in ((40, 0), (21, 0), (20, 1)):
            q = qplan(tool, query, 4000, materials=v["pro_over"]["materials"], lights=v["pro_over"]["lights"], pro_boxes=pro_boxes)
            assert (q["tab_flags"] & 1, q["tabs"]) == (tabs, tabs), (query, pro_boxes)
    def names(kw, **more):
        args = dict(materials=kw["materials"], lights=kw["lights"], **more)
        return (kernel(plan(tool, FORCE_ALL, diffuse_only=0, **args, **SMALL)), kernel(plan(tool, FORCE_ALL, diffuse_only=1, **args, **SMALL)),
                kernel(plan(tool, FORCE_ALL, diffuse_only=0, counters=1, **args, **SMALL)), plan(tool, **args, **SMALL)["tab_flags"])
    assert names(v["at_caps"])[3] == 11 and names(v["at_caps"])[1].startswith("exchange+diffuse")
    assert kernel(plan(tool, diffuse_only=0, materials=v["at_caps"]["materials"], lights=v["at_caps"]["lights"], **SMALL)) == "five+tabs+implicit"
    assert names(v["mats_over"]) == ("plain", "plain+diffuse", "plain+counters", 3)          # pt_persistent<false, false, false>, <true, false, false>
    assert names(v["mats_over_diffuse"]) == ("plain", "plain+diffuse", "plain+counters", 3)  # <false, true, false>: the scene is diffuse_only
    assert names(v["lights_over"]) == ("plain", "plain+diffuse", "plain+counters", 9)
    assert names(v["ref_limits"]) == names(v["beyond_ref"]) == ("plain", "plain+diffuse", "plain+counters", 1)
    # pro_over: 40 boxes in the prologue under ORT_ANALYTIC_PROLOGUE=40, 21 under 21, 20 (the cap) under 20
    assert names(v["pro_over"], pro_boxes=40) == names(v["pro_over"], pro_boxes=21) == ("plain", "plain+diffuse", "plain+counters", 10)
    assert names(v["pro_over"], pro_boxes=20)[3] == 11
    for counters in (0, 1):  # the knob, on scenes that fit
        assert kernel(plan(tool, {"ORT_LDS_TABLES": "0"}, counters=counters, diffuse_only=0, **SMALL)) == ("plain+counters" if counters else "plain")
    assert kernel(plan(tool, {"ORT_LDS_TABLES": "0"}, explicit_jobs=1, job_count=1024, diffuse_only=0)) == "plain"


# ---- clamps ---------------------------------------------------------------------------------------------------------
VALUES = ["0", "1", "5", "63", "64", "65", "128", "129", "1000", "100000"]


@pytest.mark.parametrize("long_min", VALUES)
def test_exchange_knobs_cannot_stall_a_wave(tool, long_min):
    for cap in VALUES:
        for refill in ("0", "64", "1000"):
            p = plan(tool, {"ORT_EXCHANGE": "1", "ORT_LONG_MIN": long_min, "ORT_INFLIGHT_CAP": cap, "ORT_LONG_REFILL": refill}, **SMALL)
            assert p["exchange"] == 1
            assert p["inflight_cap"] >= p["long_min"] >= 1 and p["long_min"] <= p["capL"] == 128
            assert p["long_min"] == min(max(int(long_min), 1), 128) and p["inflight_cap"] == max(int(cap), p["long_min"])
            assert p["long_refill"] == min(int(refill), 64)


@pytest.mark.parametrize("exchange", ["0", "1"])
def test_loop_exit_thresholds_stay_in_range(tool, exchange):
    for v in VALUES:
        p = plan(tool, {"ORT_EXCHANGE": exchange, "ORT_REFILL_BELOW": v, "ORT_DESCEND_BELOW": v}, **SMALL)
        assert p["refill_below"] == min(max(int(v), 1), 64) and p["descend_below"] == min(int(v), 64)


# ---- the grid -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jobs", [0, 1, 255, 256, 257, 1000, 256 * 1024 - 1, 256 * 1024, 256 * 1280 + 1, 10**9])
def test_at_least_one_workgroup_and_never_more_lanes_than_jobs(tool, jobs):
    for env, kw in (({}, {}), ({"ORT_MODE": "wavefront"}, {}), ({}, {"counters": 1}), ({"ORT_BLOCKS_PER_CU": "8"}, {}), ({"ORT_BLOCKS_PER_CU": "9"}, {})):
        p = plan(tool, env, explicit_jobs=1, job_count=jobs, **kw)
        per_cu = 8 if env.get("ORT_BLOCKS_PER_CU") == "8" else 4  # 1..8, anything else: 4
        assert p["max_blocks"] == CU * per_cu
        assert p["grid"] == min(max((jobs + 255) // 256, 1), CU * per_cu)
        assert p["batch_until"] <= p["job_count"] == jobs


@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (9, 8), (64, 64), (1920, 1080)])
def test_implicit_job_spaces_fill_the_grid_they_need(tool, w, h):
    blocks = ((w + 7) // 8) * ((h + 7) // 8)
    for env, per_cu in (({"ORT_WAVES5": "0"}, 4), ({"ORT_WAVES5": "1"}, 5), ({"ORT_EXCHANGE": "1"}, 4)):
        for policy, per_block in (("pixel", 64), ("chunk", 128)):
            p = plan(tool, env, policy=policy, width=w, height=h, spp=8, chunk=4)
            assert p["job_count"] == blocks * per_block and p["five"] == (per_cu == 5)
            assert p["grid"] == min((p["job_count"] + 255) // 256, CU * per_cu) >= 1
            assert p["endgame_from"] <= p["job_count"] and p["batch_until"] <= p["job_count"]
    # a shard that owns no block at all
    p = plan(tool, width=8, height=8, spp=8, chunk=4, shard_index=3, shard_count=8)
    assert (p["job_count"], p["grid"]) == (0, 1)
    # five waves under ORT_BLOCKS_PER_CU keep the grid the upload fixed
    assert plan(tool, {"ORT_WAVES5": "1", "ORT_BLOCKS_PER_CU": "6"}, spp=1024, **HD)["grid"] == CU * 6


# ---- the ray queries (plan_ray_query, plan_radiance): the job space is the ray array ---------------------------------------
QUERY_KNOBS = ({"ORT_CACHE_RESIDENT": "0"}, {"ORT_CACHE_RESIDENT": "1"}, {"ORT_DESCEND_BELOW": "3"}, {"ORT_REFILL_BELOW": "5"}, {"ORT_JOB_BATCH": "7"},
               {"ORT_BATCH_TAIL": "1"})
CLOSEST = ["raycast", "occluded"]


@pytest.mark.parametrize("query", CLOSEST)
def test_ray_query_grid_and_batches(tool, query):
    a, b, c = qplan(tool, query, 1), qplan(tool, query, 1000), qplan(tool, query, 10_000_000)
    assert (a["grid"], a["batch_until"]) == (1, 0)
    assert (b["grid"], b["batch_until"]) == (4, 0)
    assert (c["grid"], c["job_batch"], c["batch_until"], c["refill_below"]) == (1024, 1024, 10_000_000 - 4 * LANES, 32)
    for p in (a, b, c):
        assert (p["job_batch"], p["refill_below"], p["diffuse"], p["counters"]) == (1024, 32, 0, 0)
    assert qplan(tool, query, 1000, counters=1)["counters"] == 1
    assert qplan(tool, query, 4 * LANES)["batch_until"] == 0 and qplan(tool, query, 4 * LANES + 1)["batch_until"] == 1
    assert qplan(tool, query, 256 * 1024 + 1)["grid"] == 1024 and qplan(tool, query, 256 * 1023 + 1)["grid"] == 1024
    assert qplan(tool, query, 256 * 1023)["grid"] == 1023


@pytest.mark.parametrize("query", CLOSEST)
def test_ray_query_descends_by_the_16_mb_line_and_reads_no_knob(tool, query):
    for count in (1000, 10_000_000):
        small, large = qplan(tool, query, count), qplan(tool, query, count, fast_tree_bytes=86 << 20)
        assert small["descend_below"] == 8 and large["descend_below"] == 16
        assert qplan(tool, query, count, fast_tree_bytes=16 << 20)["descend_below"] == 8
        assert qplan(tool, query, count, fast_tree_bytes=(16 << 20) + 1)["descend_below"] == 16
        for env in QUERY_KNOBS:
            assert qplan(tool, query, count, env) == small, env
            assert qplan(tool, query, count, env, fast_tree_bytes=86 << 20) == large, env


@pytest.mark.parametrize("query", CLOSEST)
def test_ray_query_tabs_is_the_prologues_table_alone(tool, query):
    assert qplan(tool, query, 1000)["tabs"] == 1
    for over in (dict(materials=49), dict(lights=65), dict(materials=300, lights=200)):  # past a cap, the prologue fits
        q = qplan(tool, query, 1000, **over)
        assert q["tab_flags"] & 1 and q["tab_flags"] != 11 and q["tabs"] == 1, over
    q = qplan(tool, query, 1000, pro_boxes=21)
    assert (q["tab_flags"], q["tabs"]) == (10, 0)
    for flags in range(12):
        if flags & 4 == 0:
            assert qplan(tool, query, 1000, tab_flags=flags)["tabs"] == (flags & 1), flags
    assert qplan(tool, query, 1000, {"ORT_LDS_TABLES": "0"})["tabs"] == 1
    assert qplan(tool, query, 1000, {"ORT_LDS_TABLES": "0"}, pro_boxes=21)["tabs"] == 0
    assert qplan(tool, query, 1000, {"ORT_KERNEL": "general"}, diffuse_only=1)["diffuse"] == 0  # no BSDF in these lanes


def test_radiance_loop_exits_follow_the_tree_and_both_knobs(tool):
    small, large = qplan(tool, "radiance", 1000), qplan(tool, "radiance", 1000, fast_tree_bytes=86 << 20)
    assert (small["refill_below"], small["descend_below"]) == (16, 8)
    assert (large["refill_below"], large["descend_below"]) == (32, 16)
    forced = qplan(tool, "radiance", 1000, {"ORT_CACHE_RESIDENT": "0"})
    assert (forced["refill_below"], forced["descend_below"]) == (32, 16)
    forced = qplan(tool, "radiance", 1000, {"ORT_CACHE_RESIDENT": "1"}, fast_tree_bytes=86 << 20)
    assert (forced["refill_below"], forced["descend_below"]) == (16, 8)
    for v in VALUES:
        p = qplan(tool, "radiance", 1000, {"ORT_REFILL_BELOW": v, "ORT_DESCEND_BELOW": v})
        assert p["refill_below"] == min(max(int(v), 1), 64) and p["descend_below"] == min(int(v), 64)


def test_radiance_batches_of_128_from_96_rays_per_lane(tool):
    at, below = qplan(tool, "radiance", 96 * LANES), qplan(tool, "radiance", 96 * LANES - 1)
    assert (at["grid"], at["job_batch"], at["batch_until"]) == (1024, 128, 80 * LANES)
    assert (below["job_batch"], below["batch_until"]) == (64, 96 * LANES - 1 - 8 * LANES)
    few = qplan(tool, "radiance", 1000)  # four workgroups, one ray per lane: nothing to batch
    assert (few["grid"], few["job_batch"], few["batch_until"]) == (4, 64, 0)
    assert qplan(tool, "radiance", 1)["grid"] == 1
    p = qplan(tool, "radiance", 10_000_000, {"ORT_JOB_BATCH": "7", "ORT_BATCH_TAIL": "1"})
    assert (p["job_batch"], p["batch_until"]) == (7, 10_000_000 - LANES)
    p = qplan(tool, "radiance", 10_000_000, {"ORT_JOB_BATCH": "0"})
    assert (p["job_batch"], p["batch_until"]) == (0, 10_000_000)
    p = qplan(tool, "radiance", 10_000_000, {"ORT_JOB_BATCH": "256"})
    assert (p["job_batch"], p["batch_until"]) == (256, 10_000_000 - 32 * LANES)


def test_radiance_flavours(tool):
    for counters in (0, 1):  # both BSDF flavours exist with counters
        assert (qplan(tool, "radiance", 1000, counters=counters, diffuse_only=1)["diffuse"], qplan(tool, "radiance", 1000, counters=counters, diffuse_only=0)["diffuse"]) == (1, 0)
        assert qplan(tool, "radiance", 1000, {"ORT_KERNEL": "general"}, counters=counters, diffuse_only=1)["diffuse"] == 0
        assert qplan(tool, "radiance", 1000, counters=counters)["counters"] == counters
    assert qplan(tool, "radiance", 1000)["tabs"] == 1
    for missing in (1, 2, 8):  # all three tables, or none
        assert qplan(tool, "radiance", 1000, tab_flags=11 & ~missing)["tabs"] == 0
    assert qplan(tool, "radiance", 1000, materials=49)["tabs"] == 0 and qplan(tool, "radiance", 1000, lights=65)["tabs"] == 0
    assert qplan(tool, "radiance", 1000, pro_boxes=21)["tabs"] == 0
    assert qplan(tool, "radiance", 1000, {"ORT_LDS_TABLES": "0"})["tabs"] == 0


def test_radiance_has_no_other_kernel_to_force(tool):
    for count in (1000, 100 * LANES):
        base = qplan(tool, "radiance", count, has_wide=1, sah_cost=0.5)
        for env in ({"ORT_EXCHANGE": "1"}, {"ORT_WAVES5": "1"}, {"ORT_WIDE": "1"}, {"ORT_MODE": "wavefront"}, FORCE_ALL):
            assert qplan(tool, "radiance", count, env, has_wide=1, sah_cost=0.5) == base, env


# ---- the RenderView a plan is turned into (render_view, csrc/ort_setup.h): what device_render uploads besides pointers -------
FRAME = dict(width=20, height=13, x0=3, y0=2, x1=17, y1=9, seed=9, rr=0.5)   # 3 x 2 blocks under the rect
EXCHANGE_FIELDS = ("capL", "capR", "long_min", "long_refill", "inflight_cap", "park_min", "stash_wave_f4")


def test_fill_of_the_adaptive_call(tool):
    """spp is max_spp whatever params->spp says; seed and chunk stay unset (the lanes read the seed from the camera table, and a
    job's length is the rule's), and so do the exchange fields and endgame_from"""
    for views in ({}, dict(views=3, view_seed=40)):
        p, rv = fill(tool, policy="pixel", adaptive=1, spp=5, chunk=5, min_spp=8, max_spp=64, check_every=4, tolerance=0.25, floor=0.5, **FRAME, **views)
        n = views.get("views", 1)
        assert (rv["seed"], rv["chunk"], rv["spp"], rv["endgame_from"], rv["block_major"], rv["packed_out"]) == (0, 0, 64, 0, 0, 0)
        assert [rv[k] for k in EXCHANGE_FIELDS] == [0] * 7
        assert (rv["ad_min_spp"], rv["ad_check_every"], rv["ad_tolerance"], rv["ad_floor"], rv["rr"]) == (8, 4, 0.25, 0.5, 0.5)
        assert (rv["mode"], rv["nchunks"], rv["my_blocks"], rv["view_jobs"], rv["view_count"], rv["job_count"]) == (1, 1, 6, 384, n, 384 * n)
        assert (rv["W"], rv["H"], rv["x0"], rv["y0"], rv["x1"], rv["y1"]) == (20, 13, 3, 2, 17, 9)
        assert (rv["blocks_w"], rv["block_x0"], rv["block_y0"], rv["shard_index"], rv["shard_count"]) == (3, 0, 0, 0, 1)
        assert (rv["refill_below"], rv["descend_below"], rv["job_batch"], rv["batch_until"]) == (16, 8, 64, 0)
        assert (rv["job_batch"], rv["batch_until"], rv["refill_below"]) == (p["job_batch"], p["batch_until"], p["refill_below"])


def test_fill_of_a_one_view_batch_is_the_single_frame_call_with_that_views_seed(tool):
    """view_count and view_jobs stay unset: the launch is the single-frame kernel's"""
    _, one = fill(tool, policy="chunk", spp=4, chunk=2, views=1, view_seed=77, **FRAME)
    _, single = fill(tool, policy="chunk", spp=4, chunk=2, **FRAME)
    assert (one["view_count"], one["view_jobs"], one["seed"], single["seed"]) == (0, 0, 77, 9)
    assert (one["mode"], one["nchunks"], one["job_count"], one["my_blocks"], one["block_major"], one["spp"], one["chunk"]) == (2, 2, 768, 6, 1, 4, 2)
    assert dict(one, seed=9) == single


def test_fill_of_a_three_view_chunk_batch(tool):
    """the job space is three times the view's, the seed params->seed (unread: the lanes take theirs from the camera table)"""
    p, rv = fill(tool, policy="chunk", spp=4, chunk=2, views=3, view_seed=77, **FRAME)
    assert (rv["view_count"], rv["view_jobs"], rv["job_count"], rv["seed"]) == (3, 768, 2304, 9)
    assert rv["job_count"] == 3 * rv["view_jobs"] == p["job_count"]
    assert (rv["mode"], rv["nchunks"], rv["block_major"], rv["endgame_from"]) == (2, 2, 1, 0)
    assert [rv[k] for k in EXCHANGE_FIELDS] == [0] * 7


# ---- every plan names a kernel that is built (plan_variant, kBuiltKernels: csrc/ort_plan.h) ----------------------------------
def test_every_plan_of_the_sweep_names_a_built_kernel(tool):
    """tools/launch_plan sweep=1: plan_render and plan_pixel_jobs over traits, job spaces, frames and the knobs that choose
    kernels, each plan's variant looked up in the list ort_kernels.hip's table of launchers is held against at compile time:
    what would be an ORT_ERR_INTERNAL on the device is found here"""
    r = subprocess.run([tool, "sweep=1"], env={k: v for k, v in os.environ.items() if k not in KNOBS}, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    s = json.loads(r.stdout)
    assert s["plans"] > 0 and (s["unbuilt"], s["first"]) == (0, []), s
    # the variant of a plan, by name: what the forcings of the GPU tests launch
    assert (plan(tool, variant=1, **SMALL)["variant"], plan(tool, variant=1, **SMALL)["built"]) == ("loop<0, 1, 1, 1, 0>", 1)
    assert plan(tool, {"ORT_EXCHANGE": "1", "ORT_DEBUG_UTIL": "1"}, counters=1, variant=1, **SMALL)["variant"] == "exchange<1, 1, 1, 1, 0>"
    assert plan(tool, {"ORT_WAVES5": "1", "ORT_EXCHANGE": "0"}, variant=1, **SMALL)["variant"] == "five<0, 1, 1, 1, 0>"
    assert plan(tool, views=3, counters=1, variant=1, **SMALL)["variant"] == "loop_views<1, 0, 1, 0, 0>"
    assert plan(tool, policy="pixel", adaptive=1, variant=1, **SMALL)["variant"] == "adaptive<0, 1, 1, 1, 0>"
    assert "variant" not in plan(tool, **SMALL)
