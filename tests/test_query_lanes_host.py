"""The ray-query lanes (raycast_lane, occluded_lane, radiance_lane), the batch-of-views flavour of pt_lane and the TABS = true
lane code, run without a GPU: tools/host_sim compiles ort_lane.h for the host, one simulated lane per thread, on the tables the
product's own host code packs (ort_setup.h: the shape table behind `prim`, the scene box, the image of the LDS tables, the
camera table of a batch of views).  Everything is compared bit for bit -- NaNs by position -- with the reference's own answers
(tests/golden/raycast_*.npz) and with the oracle.  SIM_TABS=1 selects the TABS = true instantiations, the tables read from a heap
block of exactly kTabF4 float4; SIM_FORCE_FALLBACK=0 sends every ray through the exact walk.

Shown to fail on a scratch copy (never committed), one change at a time; everything not named stayed green:
  occluded_lane's `h.best_t < bound` as `<=`: test_occlusion_ladder and test_occlusion_ladder_table_scenes go red in every case
  (the rung tmax == t).
  raycast_lane reading io.prim_src[info_index(...) + 1]: test_reference_answers, test_reference_answers_at_and_past_the_table_caps,
  test_mixed_and_hostile_rays_against_the_oracle and test_exact_walk_thresholds go red in every case (the reported shape's material).
  load_view_camera's view index pinned to 0: all six cases of test_views_match_the_oracle go red (views 1 and 2).
  pack_lds_tables writing the material records one float4 early: the SIM_TABS=1 runs of test_render_modes_with_tables (all four,
  at_caps with the last float4 of the slot in use among them), test_radiance and test_views_match_the_oracle go red."""
import os

import numpy as np
import pytest

import host_sim_tool as hs
import occluded_cases
import radiance_cases
import raycast_cases
import table_scenes
from conftest import GOLDEN, assert_bits_equal
from raycast_cases import needs_exact, scene_box, threshold_rays, threshold_scene
from views_cases import SEEDS, poses

SCENES = ["testscene", "c2_analytic", "c3_bunny_room", "c4_dwarf_room", "letters", "glass_room", "rand_a", "rand_b"]   # test_gpu_raycast.SCENES

FLT_MAX = np.float32(3.4028235e38)
TABS = {"SIM_TABS": "1"}
EXACT = {"SIM_FORCE_FALLBACK": "0"}


@pytest.fixture(scope="module")
def host_sim():
    return hs.built("host_sim")


@pytest.fixture(scope="module")
def table_scn(api, tmp_path_factory):
    """variant -> (committed product scene, .scn path, its directory, with_reference_csg)"""
    made = {}

    def get(variant):
        if variant not in made:
            d = tmp_path_factory.mktemp("q_" + variant)
            scene, _, csg = table_scenes.build(api, variant, d)
            made[variant] = (scene.commit(), str(d / (variant + ".scn")), str(d) + "/", csg)
        return made[variant]
    return get


def _same_hits(hits, z, what):
    raycast_cases.assert_same_answers(hits["t"], hits["n"], hits["mat"], z["t"], z["n"], z["mat"], what)


def _assert_prims(api, scene, flat, hits, what):
    """prim is NO_PRIM exactly for the misses; otherwise it names a shape whose material is the hit's"""
    missed = hits["mat"] == 0
    assert ((hits["prim"] == hs.NO_PRIM) == missed).all(), what
    sel = np.flatnonzero(~missed)
    kind, index = api.decode_prim(hits["prim"][sel])
    mat = np.zeros(len(sel), "<u4")
    k = kind == api.HIT_TRIANGLE
    if k.any():
        mesh, _ = scene.triangle_of(index[k])
        mat[k] = np.array([flat.meshes[m]["mat"] for m in mesh], "<u4")
    for code, arr in ((api.HIT_SPHERE, flat.spheres), (api.HIT_BOX, flat.boxes), (api.HIT_CYLINDER, flat.cylinders)):
        k = kind == code
        mat[k] = arr["mat"][index[k]]
    assert (mat == hits["mat"][sel]).all(), what + ": the reported shape's material is not the hit's"


def _all_ways(host_sim, d, scene, rays, base=None, tabs=True, commit_env=None):
    """tables off / on, fast / exact walk, each on 8 threads and on 1: the same bytes every time -> the hits"""
    first = None
    for env in [{}, TABS, EXACT, dict(TABS, **EXACT)] if tabs else [{}, EXACT]:
        for threads in (8, 1):   # the single lane takes every third ray: a third of the work, the same scene load
            sub = slice(None) if threads == 8 else slice(0, None, 3)
            hits, r = hs.raycast(host_sim, d, scene, rays[sub], base, env=dict(commit_env or {}, **env), threads=threads)
            c = hs.counters(r)
            assert c["rays"] == len(rays[sub]) and c["overflow"] == 0
            if "SIM_FORCE_FALLBACK" in env:
                assert c["fallback"] == len(rays[sub])
            if first is None:
                first = hits
            assert hits.tobytes() == first[sub].tobytes(), (env, threads)
    return first


# ---- closest hit: the reference's own answers -------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_reference_answers(host_sim, api, load_scene, tmp_path, name):
    scene = load_scene(name)
    flat = scene.flatten(64, 64)
    zs = [np.load(os.path.join(GOLDEN, "%s_%s.npz" % (prefix, name))) for prefix in ("raycast", "raycast_edges")]
    z = {k: np.concatenate([zs[0][k], zs[1][k][::2]]) for k in ("rays", "t", "n", "mat")}   # one array (a run costs a scene load): 400 + 756 rays
    hits = _all_ways(host_sim, tmp_path, name, z["rays"])
    _same_hits(hits, z, "raycast_%s and raycast_edges_%s" % (name, name))
    _assert_prims(api, scene, flat, hits, name)
    # every ray is answered on its own: a cut of the array gives that cut of the answers
    for count, env in ((1, {}), (63, TABS), (64, {}), (65, TABS)) if name in ("c2_analytic", "c3_bunny_room") else ():   # a prologue-only scene and a mesh
        cut = slice(0, count) if count & 1 else slice(len(hits) - count, len(hits))
        part, _ = hs.raycast(host_sim, tmp_path, name, z["rays"][cut], env=env, threads=2)
        assert part.tobytes() == hits[cut].tobytes(), count


@pytest.mark.parametrize("variant", table_scenes.GOLDEN_VARIANTS)
def test_reference_answers_at_and_past_the_table_caps(host_sim, api, table_scn, tmp_path, variant):
    scene, scn, base, _ = table_scn(variant)
    z = np.load(os.path.join(GOLDEN, "raycast_tables_%s.npz" % variant))
    hits = _all_ways(host_sim, tmp_path, scn, z["rays"], base)   # the prologue fits in every variant: TAB_PRO is all a query needs
    _same_hits(hits, z, "raycast_tables_" + variant)
    _assert_prims(api, scene, scene.flatten(64, 64), hits, variant)


# ---- closest hit: the oracle ----------------------------------------------------------------------------------------------
N_MIXED = 800   # drawn as the GPU tests draw their 20 000: a run's cost here is the scene's load, and the hostile rays come on top


@pytest.fixture(scope="module")
def oracle_cast(oracle, load_scene):
    """name -> (flat, cast(rays) -> (t, n, mat)), one oracle scene per data scene"""
    made = {}

    def get(name):
        if name not in made:
            flat = load_scene(name).flatten(64, 64)
            osc = oracle.OracleScene(flat)
            made[name] = (flat, lambda rays: osc.raycast(np.ascontiguousarray(rays[:, 0:3]), np.ascontiguousarray(rays[:, 3:6])))
        return made[name]
    return get


@pytest.mark.parametrize("name", SCENES)
def test_mixed_and_hostile_rays_against_the_oracle(host_sim, api, load_scene, oracle_cast, tmp_path, name):
    """800 mixed rays drawn as the GPU tests draw them (the surface starts from the oracle's own first cast) and the hostile
    rays of raycast_cases.cases"""
    flat, cast = oracle_cast(name)
    rays, kinds = raycast_cases.mixed_rays(lambda r: cast(r)[0], name, N_MIXED)
    edge, _ = raycast_cases.cases(flat, lambda r: cast(r)[0])
    rays = np.concatenate([rays, edge])
    t, n, mat = cast(rays)
    want = {"t": t, "n": n, "mat": mat}
    for env, threads in (({}, 8), (TABS, 1), (dict(TABS, **EXACT), 8)):
        hits, _ = hs.raycast(host_sim, tmp_path, name, rays, env=env, threads=threads)
        _same_hits(hits, want, "%s %r" % (name, env))
    assert (kinds == 1).sum() > N_MIXED // 8
    out = hits[:N_MIXED][kinds == 3]
    assert (out["t"].view("<u4") == FLT_MAX.view("<u4")).all() and (out["n"] == 0).all() and (out["prim"] == hs.NO_PRIM).all()
    _assert_prims(api, load_scene(name), flat, hits, name)


def _write_scn(flat, path):
    """a scene of analytic shapes in the .scn grammar, as tools/make_tablescene.py writes one: every shape after a brdf line of
    its own material (a shape takes the last material read)"""
    f3 = "%.6f %.6f %.6f"
    cam = flat.camera[0]
    L = ["screen 64 48", ("camera " + f3 + " b 0.3 q 1.000000 0.000000 0.000000 0.000000") % tuple(float(x) for x in cam)]

    def brdf(m):
        m = flat.materials[m]
        L.append(("brdf " + f3 + " " + f3 + " 10 " + f3 + " %.6f") % (tuple(m["diffuse"]) + tuple(m["specular"][:3]) + tuple(m["transmission"]) + (m["ior"],)))
    for sp in flat.spheres:
        brdf(sp["mat"])
        L.append(("sphere " + f3 + " %.6f") % (tuple(sp["center"]) + (sp["r"],)))
    for b in flat.boxes:
        brdf(b["mat"])
        L.append(("box " + f3 + " " + f3) % (tuple(b["min"]) + tuple(np.asarray(b["max"], "<f4") - np.asarray(b["min"], "<f4"))))
    for c in flat.cylinders:
        brdf(c["mat"])
        L.append(("cylinder " + f3 + " " + f3 + " %.6f") % (tuple(c["base"]) + tuple(c["axis"]) + (c["r"],)))
    with open(path, "w") as f:
        f.write("\n".join(L) + "\n")
    return path


@pytest.mark.parametrize("small", [False, True], ids=["room", "small"])
def test_exact_walk_thresholds(host_sim, api, oracle, monkeypatch, tmp_path, small):
    """the threshold scenes of the GPU test, committed under ORT_ANALYTIC_PROLOGUE=0 (every quadric in the fast tree), written
    out as .scn: the oracle's answers, and at least the rays raycast_needs_exact selects counted as exact walks"""
    flat = threshold_scene(api, small).flatten(64, 48)
    scn = _write_scn(flat, str(tmp_path / "threshold.scn"))
    loaded = api.Scene.load_scn(scn)
    monkeypatch.setenv("ORT_ANALYTIC_PROLOGUE", "0")
    loaded.commit()
    monkeypatch.delenv("ORT_ANALYTIC_PROLOGUE")
    lflat = loaded.flatten(64, 48)   # the scene as the text gives it (six decimals): rays and expectations are made from this one
    assert (len(lflat.spheres), len(lflat.boxes), len(lflat.cylinders)) == (len(flat.spheres), len(flat.boxes), len(flat.cylinders))
    assert loaded.tree_info()["prologue_prims"] == 0
    if small:
        assert float(np.linalg.norm(np.subtract(*scene_box(lflat, lflat.camera[0])[::-1]).astype(np.float64))) < 1.0
    cam = np.asarray(lflat.camera[0], "<f4")
    lo, hi = scene_box(lflat, cam)
    rays = threshold_rays(lflat, cam, np.random.default_rng(99 + small), (0.03, 0.08) if small else (0.4, 2.5))
    t, n, mat = oracle.OracleScene(lflat, with_reference_csg=True).raycast(rays[:, 0:3], rays[:, 3:6])
    env = {"ORT_ANALYTIC_PROLOGUE": "0"}
    hits, r = hs.raycast(host_sim, tmp_path, scn, rays, str(tmp_path) + "/", env=env, threads=8)
    _same_hits(hits, {"t": t, "n": n, "mat": mat}, "thresholds")
    _assert_prims(api, loaded, lflat, hits, "thresholds")
    need = needs_exact(rays, lo, hi, len(lflat.spheres) > 0, len(lflat.spheres) + len(lflat.cylinders) > 0)
    assert 0 < need.sum() < len(rays) and (~need).sum() > len(rays) // 3
    assert hs.counters(r)["fallback"] >= need.sum(), (hs.counters(r)["fallback"], int(need.sum()))
    exact, rx = hs.raycast(host_sim, tmp_path, scn, rays, str(tmp_path) + "/", env=dict(env, **EXACT), threads=8)
    assert hs.counters(rx)["fallback"] == len(rays) and exact.tobytes() == hits.tobytes()


@pytest.mark.parametrize("budget,fits", [(40, False), (21, False), (20, True)])
def test_prologue_past_its_slot(host_sim, api, oracle, table_scn, monkeypatch, tmp_path, budget, fits):
    """pro_over under ORT_ANALYTIC_PROLOGUE=40 and 21: the prologue's boxes do not fit the LDS slot, SIM_TABS is refused and
    prologue_tests reads them from their array; under 20 they fill the slot to its last float4"""
    _, scn, base, csg = table_scn("pro_over")
    scene = api.Scene.load_scn(scn)
    monkeypatch.setenv("ORT_ANALYTIC_PROLOGUE", str(budget))
    scene.commit()
    monkeypatch.delenv("ORT_ANALYTIC_PROLOGUE")
    assert scene.tree_info()["prologue_prims"] == budget
    flat = scene.flatten(64, 64)
    osc = oracle.OracleScene(flat, with_reference_csg=csg)
    rays = np.load(os.path.join(GOLDEN, "raycast_tables_at_caps.npz"))["rays"]
    t, n, mat = osc.raycast(rays[:, 0:3], rays[:, 3:6])
    env = {"ORT_ANALYTIC_PROLOGUE": str(budget)}
    hits = _all_ways(host_sim, tmp_path, scn, rays, base, tabs=fits, commit_env=env)
    _same_hits(hits, {"t": t, "n": n, "mat": mat}, "pro_over %d" % budget)
    if not fits:
        args, _ = hs.raycast_args(str(tmp_path), scn, rays, base)
        r = hs.run(host_sim, args, env=dict(env, **TABS), check=False)
        assert r.returncode == 1 and "SIM_TABS" in r.stderr


# ---- occlusion ------------------------------------------------------------------------------------------------------------
def _check_ladder(host_sim, d, scene, rays, t, mat, what, base=None):
    """the limits of the GPU tests: none, a scalar, and per ray -inf, -1, -0.0, 0, t/2, prev(t), t, next(t), 2t, FLT_MAX, +inf, NaN"""
    ok = ~np.isnan(t)
    rays, t, mat = rays[ok], t[ok], mat[ok]
    rr, tm, want, rung = occluded_cases.laddered(rays, t, mat)
    assert (~want).mean() >= 0.10 and want.mean() >= 0.10
    for env, threads in (({}, 8), (TABS, 1), (EXACT, 8)):
        got = hs.occluded(host_sim, d, scene, rr, tm, base, env=env, threads=threads)
        bad = np.flatnonzero(got != want.astype(np.uint8))
        assert len(bad) == 0, "%s %r: %d bytes differ, first at rung %s" % (what, env, len(bad), occluded_cases.RUNGS[rung[bad[0]]])
    inf_rung = occluded_cases.expected(t, mat, np.full(len(t), np.inf, "<f4")).astype(np.uint8)
    assert (hs.occluded(host_sim, d, scene, rays, None, base, env=TABS, threads=8) == inf_rung).all(), what + ": no limit"
    scalar = occluded_cases.expected(t, mat, np.full(len(t), 2.5, "<f4")).astype(np.uint8)
    assert (hs.occluded(host_sim, d, scene, rays, np.full(len(t), 2.5, "<f4"), base, threads=8) == scalar).all(), what + ": scalar limit"


@pytest.mark.parametrize("name", SCENES)
def test_occlusion_ladder(host_sim, tmp_path, name):
    zs = [np.load(os.path.join(GOLDEN, "%s_%s.npz" % (prefix, name))) for prefix in ("raycast", "raycast_edges")]
    z = {k: np.concatenate([zs[0][k][::4], zs[1][k][::9]]) for k in ("rays", "t", "mat")}   # 100 + 168 rays, twelve limits each
    _check_ladder(host_sim, tmp_path, name, z["rays"], z["t"], z["mat"], "raycast_%s and raycast_edges_%s" % (name, name))


@pytest.mark.parametrize("variant", ["at_caps", "mats_over"])
def test_occlusion_ladder_table_scenes(host_sim, table_scn, tmp_path, variant):
    _, scn, base, _ = table_scn(variant)
    z = np.load(os.path.join(GOLDEN, "raycast_tables_%s.npz" % variant))
    _check_ladder(host_sim, tmp_path, scn, z["rays"], z["t"], z["mat"], variant, base)


# ---- radiance ---------------------------------------------------------------------------------------------------------------
N_RADIANCE = 120


@pytest.mark.parametrize("name,envs", [("testscene", [{}, TABS]), ("c2_analytic", [{}, TABS]),
                                       ("c3_bunny_room", [{"SIM_DIFFUSE": "1"}, dict(TABS, SIM_DIFFUSE="1"), {}]),
                                       ("tables_mats_over", [{}])])
def test_radiance(host_sim, oracle, load_scene, table_scn, tmp_path, name, envs):
    """radiance_cases.mixed with its out-of-domain rays: colours and final stream states for spp 1 and 3; a ray outside the
    domain gives NaN NaN NaN and its seed back, and its neighbours are untouched (they equal the oracle's)"""
    if name.startswith("tables_"):
        scene, scn, base, csg = table_scn(name[len("tables_"):])
    else:
        scene, scn, base, csg = load_scene(name), name, None, True
    flat = scene.flatten(64, 64)
    osc = oracle.OracleScene(flat, with_reference_csg=csg)
    cases = radiance_cases.mixed(name, flat, osc, N_RADIANCE)
    want = radiance_cases.expected_of(osc, cases, (1, 3), 0.8)
    assert (~cases.ok).sum() == 8 and np.isnan(want[1][0][~cases.ok]).all() and (want[3][1][~cases.ok] == cases.seeds[~cases.ok]).all()
    for env in envs:
        for spp, threads in ((1, 8), (3, 1)):
            rgb, states = hs.radiance(host_sim, tmp_path, scn, cases.rays, cases.seeds, spp, 0.8, base, env=env, threads=threads)
            radiance_cases.assert_same(rgb, states, want[spp][0], want[spp][1], "%s spp %d %r" % (name, spp, env))
    if name.startswith("tables_"):   # past the material cap the TABS lanes are not available
        args, _ = hs.radiance_args(str(tmp_path), scn, cases.rays, cases.seeds, 1, 0.8, base)
        assert hs.run(host_sim, args, env=TABS, check=False).returncode == 1


# ---- a batch of views ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,spp,policy,chunk", [(24, 16, 4, "chunk", 2), (19, 13, 3, "pixel", 0)])
@pytest.mark.parametrize("name", ["testscene", "c3_bunny_room", "tables_mats_over"])
def test_views_match_the_oracle(host_sim, api, oracle, load_scene, table_scn, tmp_path, name, w, h, spp, policy, chunk):
    """three views, one of them the scene's own pose: frame v is the oracle's render with set_camera of that view and that
    view's seed; a batch of one view is the single-view render"""
    if name.startswith("tables_"):
        scene, scn, base, csg = table_scn(name[len("tables_"):])
    else:
        scene, scn, base, csg = load_scene(name), name, None, True
    flat = scene.flatten(w, h)
    cams = np.stack([api.camera_from_pose(p, q, r, w, h) for p, q, r in poses(scene, flat)])
    assert_bits_equal(cams[0], scene.camera(w, h), "view 0 is the scene's own camera")
    osc = oracle.OracleScene(flat, with_reference_csg=csg)
    want = []
    for cam, seed in zip(cams, SEEDS):
        osc.set_camera(cam)
        want.append(osc.render(w, h, spp, seed, policy, chunk=max(chunk, 1), threads=8)[0])
    for env in ({}, TABS) if base is None else ({},):
        frames = hs.views(host_sim, tmp_path, scn, cams, SEEDS, w, h, spp, policy, chunk, base, env=env, threads=8)
        for v in range(3):
            assert_bits_equal(frames[v], want[v], "%s %s view %d %r" % (name, policy, v, env))
    one = hs.views(host_sim, tmp_path, scn, cams[:1], SEEDS[:1], w, h, spp, policy, chunk, base, threads=1)
    single = hs.render(host_sim, tmp_path, scn, w, h, spp, SEEDS[0], policy, chunk, base, threads=8)
    assert_bits_equal(one[0], single, "a batch of one view vs the single-view render")


# ---- the old render modes with the tables in their LDS layout ---------------------------------------------------------------------
@pytest.mark.parametrize("scene,w,h,spp,policy,chunk,extra", [
    ("c2_analytic", 93, 61, 6, "chunk", 2, {}),            # ragged edge blocks, all lobes
    ("c3_bunny_room", 96, 64, 4, "pixel", 0, {"SIM_DIFFUSE": "1"}),
    ("c3_bunny_room", 96, 64, 4, "chunk", 2, {"SIM_WIDE": "1"}),  # the 4-wide tree
    ("tables_at_caps", 45, 35, 5, "pixel", 0, {}),         # the last float4 of the material and the light slot in use
])
def test_render_modes_with_tables(host_sim, oracle, load_scene, table_scn, tmp_path, scene, w, h, spp, policy, chunk, extra):
    """the parametrisations of test_cpu_tile_queue.test_worker_pool_matches_the_oracle, and at_caps, under SIM_TABS=1"""
    if scene.startswith("tables_"):
        sc, scn, base, csg = table_scn(scene[len("tables_"):])
    else:
        sc, scn, base, csg = load_scene(scene), scene, None, True
    got = hs.render(host_sim, tmp_path, scn, w, h, spp, 77, policy, chunk, base, env=dict(TABS, **extra), threads=8)
    ref, _ = oracle.OracleScene(sc.flatten(w, h), with_reference_csg=csg).render(w, h, spp, 77, policy, chunk=max(chunk, 1), threads=8)
    assert_bits_equal(got, ref, "%s %s with the tables' image vs the oracle" % (scene, policy))
