"""Hostile materials on the CPU (tests/hostile_materials.py): the loader, the oracle and the host-compiled lane code against the
REFERENCE'S OWN frames, final states and chains of scenes whose coefficients are NaN, inf, negative, huge and vanishing
(tests/golden/renders_hostile.npz, chains_hostile.npz; make_golden.py --only-hostile), and the conditions that keep those scenes
from going quiet.  All of this runs before anything goes to a GPU (tests/test_gpu_hostile_materials.py): it is what lets the
oracle stand in for the reference where a call has no golden, and what says that a divergence on the device is the device's.

Everything is bit-exact, or NaN by position (hostile_materials.same_words); no pixel is skipped."""
import os
import re

import numpy as np
import pytest

import accumulate_cases as acs
import adaptive_cases as ac
import feature_cases as fc
import follow_cases as fw
import host_sim_tool as hs
import hostile_materials as hm
import irradiance_cases as ic
import light_groups_cases as lg
import radiance_cases as rc
import ref_io
import reference_goldens as rg
import render_adaptive_cases as rac
import sample_map_cases as sm
import test_launch_plan as tlp
from test_launch_plan import tool as launch_plan_tool  # noqa: F401  (the fixture that builds tools/launch_plan)

DIGEST_KEYS = ("counts", "camera_bits", "ambient_bits", "spheres_sha256", "boxes_sha256", "cylinders_sha256", "lights", "meshes")
POLICIES = (("pixel", 0), ("chunk", 4), ("whole", 0), ("tile32", 0))


@pytest.fixture(scope="module")
def frames():
    return rg.load("renders_hostile.npz")


@pytest.fixture(scope="module")
def chain_file():
    return rg.load("chains_hostile.npz")


@pytest.fixture()
def case(api, oracle, manifest, tmp_path_factory):
    def get(name):
        c = hm.case(api, oracle, name, tmp_path_factory)
        assert rg.sha256(c.scn) == manifest["generated"]["hostile"]["scenes"][name]["scn_sha256"], name
        return c
    return get


# ---- the loader --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hm.SCENES)
def test_loader_reads_the_references_coefficients(case, manifest, frames, name):
    """ort_scene_get_materials gives inf and NaN where hostile_materials.MATERIALS says so, and every word of the material array
    is the reference loader's (scene-dump), NaN by position; every other array has the reference's digest"""
    c = case(name)
    m = c.flat.materials
    meta = manifest["generated"]["hostile"]["scenes"][name]
    dg = ref_io.scene_digest(c.flat)
    for k in DIGEST_KEYS:
        assert dg[k] == meta[k], (name, k)
    got = np.frombuffer(np.ascontiguousarray(m).tobytes(), "<f4").reshape(len(m), -1)
    want = frames[name + "__materials"].view("<f4")
    nans = hm.same_words(got, want, name + ": materials")
    I = hm.INDEX
    assert np.isnan(m["diffuse"][I["nan"], 0]) and np.isinf(m["diffuse"][I["inf"], 0]) and m["diffuse"][I["inf"], 0] > 0
    # the lexer's own arithmetic: -0.500000 reads as -0.50000006, so the plain values are held to the reference's words above alone
    assert np.isclose(m["diffuse"][I["neg"], 0], -0.5) and np.allclose(m["diffuse"][I["kdgt1"]], 3)
    assert m["diffuse"][I["tiny"], 0] > 0 and np.float32(m["diffuse"][I["tiny"], 0]) ** 2 == 0      # |Kd|^2 underflows
    assert np.isclose(m["diffuse"][I["big"], 0], 1e30, rtol=1e-5)
    if name == "hostile":
        assert np.isnan(m["specular"][I["ksnan"], 0]) and np.isinf(m["specular"][I["ksinf"], 0])
        assert np.isnan(m["ior"][I["iornan"]]) and np.isinf(m["transmission"][I["ktinf"], 0])
        assert m["ior"][I["ior0"]] == 0 and np.isclose(m["ior"][I["iorhalf"]], 0.5)
        assert nans == 3 and int(np.isinf(want).sum()) == 3
    else:
        assert nans == 1 and int(np.isinf(want).sum()) == 1
        assert not m["specular"][1:, :3].any() and not m["transmission"].any()
    assert [int(i) for i in np.nonzero(m["is_light"])[0]] == list(hm.LIGHT_MATERIALS)
    assert m["emit"][list(hm.LIGHT_MATERIALS)].tolist() == [[3, 0, 2], [2, 1, 1], [0, 0, 0]]


def test_the_dark_twins_are_files_of_one_light(api, manifest, tmp_path):
    for g in range(3):
        scn, _ = hm.write(tmp_path, "hostile_dark%d" % g, hm.dark(g))
        assert rg.sha256(scn) == manifest["generated"]["hostile"]["scenes"]["hostile_dark%d" % g]["scn_sha256"]
        emit = api.Scene.load_scn(scn).commit().flatten(hm.W, hm.H).materials["emit"][list(hm.LIGHT_MATERIALS)]
        assert not emit[[k for k in range(3) if k != g]].view("<u4").any()   # all-zero bits: +0, the value light_groups_cases.dark_twin writes


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
def test_oracle_renders_match_reference(api, oracle, case, manifest, frames, tmp_path):
    """every frame of renders_hostile.npz: four policies at 24 x 16 with the PIXEL final states, PIXEL and CHUNK at 96 x 64, the
    diffuse twin, the three dark twins as files and as light_groups_cases.dark_twin's patched arrays; counters and final RNG too"""
    meta = manifest["generated"]["hostile"]["renders"]
    assert sorted(meta) == sorted(hm.key(s, p, ch, size) for s, p, ch, size, _ in hm.RENDERS)
    scenes = {n: case(n).scene for n in hm.SCENES}
    for g in range(3):
        scenes["hostile_dark%d" % g] = api.Scene.load_scn(hm.write(tmp_path, "hostile_dark%d" % g, hm.dark(g))[0]).commit()
    for scene, policy, chunk, (w, h), states in hm.RENDERS:
        key = hm.key(scene, policy, chunk, (w, h))
        osc = oracle.OracleScene(scenes[scene].flatten(w, h))
        if states:
            img, st, fin = rg.oracle_pixel_planes(oracle, osc, w, h, hm.SPP, hm.SEED, hm.RR)
            rg.assert_words_equal(fin, frames[key + "__states"], key + ": final states")
        else:
            img, st = osc.render(w, h, hm.SPP, hm.SEED, policy, chunk=max(chunk, 1), rr=hm.RR, threads=1)
        hm.same_words(img, frames[key], key)
        assert st["shapes_tested"] == meta[key]["shapes_tested"], key
        if policy != "tile32":
            assert st["final_rng"] == meta[key]["final_rng"], key
    c = case("hostile")
    for g, m in enumerate(c.lights):
        img, _ = c.twin([m]).render(hm.W, hm.H, hm.SPP, hm.SEED, "pixel", rr=hm.RR, threads=1)
        hm.same_words(img, frames[hm.key("hostile_dark%d" % g, "pixel", 0, (hm.W, hm.H))], "dark twin %d, the patched arrays" % g)


@pytest.mark.parametrize("name", hm.SCENES)
def test_oracle_chains_match_reference(oracle, case, manifest, chain_file, name):
    """render_adaptive_cases.chains against the reference called the same way: 64 one-sample calls a pixel, colours and states"""
    meta = manifest["generated"]["hostile"]["chains"][name]
    assert (meta["samples"], meta["seed"], meta["width"], meta["height"]) == (hm.CHAIN_SAMPLES, hm.SEED, hm.W, hm.H) and hm.CHAIN_SAMPLES == rac.MAX_SPP
    c = case(name)
    got = hm.chains_of(c)
    hm.same_words(np.stack([got[(x, y)][0] for y in range(hm.H) for x in range(hm.W)]).reshape(hm.H, hm.W, hm.CHAIN_SAMPLES, 3),
                  chain_file[name + "__colours"], name + " chain colours")
    rg.assert_words_equal(np.stack([got[(x, y)][1] for y in range(hm.H) for x in range(hm.W)]).reshape(hm.H, hm.W, hm.CHAIN_SAMPLES),
                          chain_file[name + "__states"], name + " chain states")


# ---- the conditions, on the reference's data ----------------------------------------------------------------------------------------
def test_conditions_hold_on_the_references_data(api, oracle, frames, chain_file, tmp_path):
    """what keeps the scene from going quiet; floors below what the committed layout measures (printed):
    non-zero pixels 175 of 384 (floor 128); pixels a material's swap for grey changes 6 (neg) to 117 (ksnan) (floor 5); the 96 x 64
    frame holds 36 finite words above 1e20 and 76 negative words (floor 1 each); 6 pixels' running Q goes non-finite within 64
    samples (floor 3) and none within min_spp = 16; no NaN word in any rendered colour frame: the bounce guard drops every
    non-finite emission, so a NaN in a frame would be a finding"""
    own = frames[hm.key("hostile", "pixel", 0, (hm.W, hm.H))]
    nonzero = int((own != 0).any(axis=2).sum())
    big = frames[hm.key("hostile", "pixel", 0, hm.BIG)]
    huge, negative = int((np.isfinite(big) & (big > 1e20)).sum()), int((big < 0).sum())
    print("non-zero pixels %d of %d; 96 x 64: %d finite words above 1e20, %d negative words" % (nonzero, hm.W * hm.H, huge, negative))
    assert nonzero >= 128 and huge >= 1 and negative >= 1
    for scene, policy, chunk, size, _ in hm.RENDERS:
        assert not np.isnan(frames[hm.key(scene, policy, chunk, size)]).any(), (scene, policy)
    ad = hm.adaptive_set()
    for name in hm.SCENES:
        q = np.stack([hm.luminance_q(chain_file[name + "__colours"][y, x]) for y in range(hm.H) for x in range(hm.W)])
        late, early = int((~np.isfinite(q[:, -1])).sum()), int((~np.isfinite(q[:, ad.min_spp - 1])).sum())
        print("%s: Q non-finite within 64 samples on %d pixels, within %d on %d" % (name, late, ad.min_spp, early))
        if name == "hostile":
            assert late >= 3 and early == 0
    changed = {}
    for n in hm.NAMES:
        scn, _ = hm.write(tmp_path, "swap_" + n, hm.swap(n))
        img, _ = oracle.OracleScene(api.Scene.load_scn(scn).commit().flatten(hm.W, hm.H)).render(hm.W, hm.H, hm.SPP, hm.SEED, "pixel", rr=hm.RR, threads=8)
        changed[n] = int((img.view("<u4") != own.view("<u4")).any(axis=2).sum())
    print("pixels a swap changes:", changed)
    assert min(changed.values()) >= 5, changed


def test_adaptive_render_keeps_sampling_on_a_non_finite_q(chain_file):
    """adaptive_stop with Q = inf: v = inf - inf = NaN, which the header defines as keep sampling.  Under the main set (min 16, a
    check every 16) the six pixels of `hostile` whose Q overflows are black for their first 16 samples and stop there -- the
    condition that none overflows within min_spp and a first check that stops a black pixel leave nothing else in this layout --
    so the pixels that reach a check with Q = inf are hostile_diffuse's under the main set (4 of them, measured) and hostile's
    under hostile_materials.adaptive_late (min 32: pixel (14, 11) overflows at sample 27).  Every such pixel runs to max_spp"""
    for name, ad, floor in (("hostile_diffuse", hm.adaptive_set(), 3), ("hostile", hm.adaptive_late(), 1)):
        chain = hm.chains_from(chain_file, name)
        _, spp, m2, _ = rac.expected_from(chain, hm.W, hm.H, ad)
        print("%s %r: %d pixels end with a non-finite m2" % (name, ad, (~np.isfinite(m2)).sum()))
        assert (~np.isfinite(m2)).sum() >= floor and (spp[~np.isfinite(m2)] == ad.max_spp).all()
        assert len(np.unique(spp)) > 1
    _, spp, m2, _ = rac.expected_from(hm.chains_from(chain_file, "hostile"), hm.W, hm.H, hm.adaptive_set())
    assert np.isfinite(m2).all() and len(np.unique(spp)) == 3


# ---- which flavour an upload picks ---------------------------------------------------------------------------------------------------
def test_the_upload_guard_picks_the_diffuse_flavour_by_itself(case, launch_plan_tool):
    """ort_setup.h's materials_diffuse_only -- the guard ort_scene_upload picks the DIFFUSE kernels with -- as tools/host_sim reports
    it of the loaded scene, handed to tools/launch_plan: hostile_diffuse (NaN, inf and all-zero materials: pd_c = NaN) takes the
    DIFFUSE flavour by itself, hostile the all-lobes one, and ORT_KERNEL=general forces the all-lobes one.  Without this the GPU
    tests of the diffuse twin would not be running what they claim"""
    tool = hs.built("host_sim")
    got = {}
    for name in hm.SCENES:
        c = case(name)
        r = hs.run(tool, hs.render_args(os.path.dirname(c.scn), c.scn, 8, 8, 1, 3, "pixel", 0, c.base)[0])
        got[name] = int(re.search(r"^materials: \d+, diffuse_only (\d)$", r.stderr, re.M).group(1))
    assert got == {"hostile": 0, "hostile_diffuse": 1}
    size = dict(width=hm.W, height=hm.H, spp=hm.SPP, chunk=4)
    assert "+diffuse" in tlp.kernel(tlp.plan(launch_plan_tool, diffuse_only=got["hostile_diffuse"], **size))
    assert "+diffuse" not in tlp.kernel(tlp.plan(launch_plan_tool, diffuse_only=got["hostile"], **size))
    assert "+diffuse" not in tlp.kernel(tlp.plan(launch_plan_tool, {"ORT_KERNEL": "general"}, diffuse_only=got["hostile_diffuse"], **size))


# ---- the lane code on the host --------------------------------------------------------------------------------------------------------
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}


@pytest.fixture(scope="module", params=["host_sim", "host_sim_w5", "host_sim_san"])
def tool(request):
    t = hs.built(request.param)
    env = dict(SAN_ENV) if request.param == "host_sim_san" else {}

    def run_env(extra=None):
        return dict(env, **(extra or {}))
    return t, run_env


def _clean(r):
    assert "runtime error:" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]


@pytest.mark.parametrize("name", hm.SCENES)
def test_lanes_render_the_references_frames(tool, case, frames, tmp_path, name):
    """the four policies, also through the tables image, the forced fallback, the wide tree, the wavefront trace and, on the diffuse twin, the
    DIFFUSE flavour (SIM_DIFFUSE=1; without it the all-lobes flavour runs, which is ORT_KERNEL=general there)"""
    t, env = tool
    c = case(name)
    sets = [{}, {"SIM_TABS": "1"}, {"SIM_FORCE_FALLBACK": "0xf"}]
    if name == "hostile_diffuse":
        sets += [{"SIM_DIFFUSE": "1"}, {"SIM_DIFFUSE": "1", "SIM_TABS": "1"}, {"ORT_KERNEL": "general"}]
    for policy, chunk in POLICIES:
        key = hm.key(name, policy, chunk, (hm.W, hm.H))
        if key not in frames.files:
            continue
        for e in sets + ([{"SIM_WIDE": "1"}, {"SIM_WAVEFRONT": "100"}] if policy == "chunk" else []):
            img = hs.render(t, tmp_path, c.scn, hm.W, hm.H, hm.SPP, hm.SEED, policy, chunk, c.base, env=env(e), threads=1 if "SIM_WAVEFRONT" in e else 2)
            hm.same_words(img, frames[key], "%s %s %r" % (name, policy, e))
    if name == "hostile":
        for policy, chunk in POLICIES[:2]:
            img = hs.render(t, tmp_path, c.scn, hm.BIG[0], hm.BIG[1], hm.SPP, hm.SEED, policy, chunk, c.base, env=env(), threads=4)
            hm.same_words(img, frames[hm.key(name, policy, chunk, hm.BIG)], "%s %s 96 x 64" % (name, policy))


def _diffuse_sets(name):
    return [{}, {"SIM_DIFFUSE": "1"}] if name == "hostile_diffuse" else [{}]


@pytest.mark.parametrize("name", hm.SCENES)
def test_lanes_views_adaptive_groups_and_sample_map(api, tool, case, frames, chain_file, tmp_path, name):
    """--views against the oracle with set_camera; --render-adaptive and --sample-map against the reference's chains;
    --light-groups against the reference's dark twins (the diffuse twin: the oracle's)"""
    t, env = tool
    c = case(name)
    chain = hm.chains_from(chain_file, name)
    cams = hm.view_cameras(api, c)
    smap = sm.mixed_map()
    for e in _diffuse_sets(name):
        for policy, chunk in POLICIES[:2]:
            got = hs.views(t, tmp_path, c.scn, cams, hm.VIEW_SEEDS, hm.W, hm.H, hm.SPP, policy, chunk, c.base, env=env(e), threads=2)
            hm.same_words(got, hm.view_frames(c, cams, hm.VIEW_SEEDS, policy, chunk), "%s views %s %r" % (name, policy, e))
        for ad in hm.ADAPTIVE_SETS:
            got = rac.host_sim(t, tmp_path, c.scn, hm.W, hm.H, None, hm.SEED, ad, hm.RR, c.base, env=env(e), threads=2)
            for g, w_, what in zip(got, rac.expected_from(chain, hm.W, hm.H, ad), ("colours", "sample counts", "second moments", "final states")):
                hm.same_words(g, w_, "%s adaptive %r %s %r" % (name, ad, what, e))
        (rgb, m2, fin), r = sm.host_sample_map(t, tmp_path, c, smap, sm.CAP, hm.SEED, env=env(e), threads=2)
        _clean(r)
        for g, w_, what in zip((rgb[0], m2[0], fin[0]), sm.expected_from(chain, smap, sm.CAP), ("colours", "second moments", "final states")):
            hm.same_words(g, w_, "%s sample map %s %r" % (name, what, e))
        own, states = hm.pixel_planes(c)
        if name == "hostile":
            hm.same_words(own, frames[hm.key(name, "pixel", 0, (hm.W, hm.H))], "the oracle's own frame")
        for groups, G in ((c.per_light(), 3), ({m: 0 for m in c.lights}, 1)):
            fr, rgb, st = lg.host_light_groups(t, tmp_path, c, c.table(groups), G, hm.SPP, hm.SEED, env=env(e), threads=2)
            for g in range(G):
                if G == 1:
                    want = own
                elif name == "hostile":
                    want = frames[hm.key("hostile_dark%d" % g, "pixel", 0, (hm.W, hm.H))]
                else:
                    want = c.twin([c.lights[g]]).render(hm.W, hm.H, hm.SPP, hm.SEED, "pixel", rr=hm.RR, threads=8)[0]
                hm.same_words(fr[0, g], want, "%s light groups G = %d, group %d %r" % (name, G, g, e))
            hm.same_words(rgb[0], own, "%s light groups: the unsplit frame" % name)
            hm.same_words(st[0], states, "%s light groups: final states" % name)


@pytest.mark.parametrize("name", hm.SCENES)
def test_lanes_features_and_queries(api, tool, case, tmp_path, name):
    """--features (single frame and a batch whose third view sees the inf wall and the negative ceiling), --radiance,
    --radiance-adaptive, --irradiance and --irradiance-adaptive on hostile_materials.ray_cases (radiance_cases.mixed's rays and 16
    aimed ones), adaptive_cases.cases_for's noisy rays and irradiance_cases' points"""
    t, env = tool
    c = case(name)
    cams = hm.view_cameras(api, c)
    want = hm.feature_expected(c, cams, hm.VIEW_SEEDS)
    alb = np.stack([w_["albedo"] for w_ in want])
    assert np.isnan(alb).any() and np.isinf(alb).any() and (alb < 0).any()
    cases, pts = hm.ray_cases(c), hm.point_set(c)
    exp, exp_ad, exp_noisy = hm.radiance_expected(c)
    noisy = hm.noisy_ray_cases(c)
    assert min(ac.classes(exp_noisy[1], exp_noisy[0], noisy.ok, ac.MAIN)[:3]) >= 0.1   # stopped at min_spp, between, ran to max_spp
    one = lambda rays, seeds: hs.radiance(hs.built("host_sim"), tmp_path, c.scn, rays, seeds, 1, hm.RR, c.base, threads=2)
    chain = ic.chain_by_radiance(c.oracle, pts, 17, one)
    for e in _diffuse_sets(name):
        got, r = fc.host_sim(t, tmp_path, c.scn, hm.W, hm.H, None, hm.FEATURE_SPP, seed=hm.SEED, base=c.base, env=env(e), threads=2)
        _clean(r)
        assert hm.assert_features({k: v[0] for k, v in got.items()}, want[0], "%s features %r" % (name, e)) > 0
        got, r = fc.host_sim(t, tmp_path, c.scn, hm.W, hm.H, None, hm.FEATURE_SPP, cams=cams, seeds=hm.VIEW_SEEDS, base=c.base, env=env(e), threads=2)
        for v in range(3):
            hm.assert_features({k: a[v] for k, a in got.items()}, want[v], "%s features, view %d %r" % (name, v, e))
        rgb, fin = hs.radiance(t, tmp_path, c.scn, cases.rays, cases.seeds, hm.QUERY_SPP, hm.RR, c.base, env=env(e), threads=2)
        rc.assert_same(rgb, fin, exp[0], exp[1], "%s radiance %r" % (name, e))
        ac.assert_same(ac.host_sim(t, tmp_path, c.scn, cases.rays, cases.seeds, ac.MAIN, hm.RR, c.base, env=env(e), threads=2), exp_ad,
                       "%s adaptive radiance %r" % (name, e))
        ac.assert_same(ac.host_sim(t, tmp_path, c.scn, noisy.rays, noisy.seeds, ac.MAIN, hm.RR, c.base, env=env(e), threads=2), exp_noisy,
                       "%s adaptive radiance, the noisy rays %r" % (name, e))
        rgb, fin, r = ic.host_sim(t, tmp_path, c.scn, pts.points, pts.seeds, 8, hm.RR, c.base, env=env(e), threads=2)
        _clean(r)
        w_rgb, w_fin = ic.expected_from(chain, pts, 8)
        rc.assert_same(rgb, fin, w_rgb, w_fin, "%s irradiance %r" % (name, e))
        got, r = ic.host_sim_adaptive(t, tmp_path, c.scn, pts.points, pts.seeds, ic.EVERY, hm.RR, c.base, env=env(e), threads=2)
        ac.assert_same(got, ic.expected_adaptive(chain, pts, ic.EVERY), "%s adaptive irradiance %r" % (name, e))


@pytest.mark.parametrize("which", ["host_sim", "host_sim_w5"])
@pytest.mark.parametrize("name", hm.SCENES)
def test_lanes_follow(oracle, case, tmp_path, name, which):
    """--follow, the single frame and a batch of three views (the scene's own camera, hostile_materials.WALL_CAM at the nan and the
    zero wall, UP_CAM at neg and inf), from the arrays, from the tables image and with the exact walk forced, at (spp 5, rr 0.5,
    cap 64) and (rr 0.8, cap 2), against follow_cases' chain.  follow_lane's terminal test `is_light || |Kd|^2 > 0 || b == cap`
    meets every hostile Kd here: NaN (false: followed), 1e-30 (its square underflows: followed), the all-zero material (followed),
    inf and -0.5 (recorded; an infinite and a negative albedo sum), and the three followed ones draw sample_brdf with no lobe.
    At cap 64 the chain's final states are first pinned against the diffuse twin's PIXEL states from the oracle on every frame.
    hostile_materials.follow_conditions states what the frames exercise.  No view of either scene gives a bounce ray with a
    non-finite direction -- the oracle's count over the four frames and both settings is 0: sample_brdf without a lobe still
    returns a finite direction -- so the NaN words the planes hold are the recorded Kd of the nan wall at the cap"""
    t = hs.built(which)
    c = case(name)
    w = hm.follow_world(c)
    fw.pin_on_twin(oracle, w, hm.FEATURE_SPP, hm.FOLLOW_SETTINGS[0][0], c.csg)
    assert hm.follow_conditions(c) == 0
    cast = lambda rays: hs.raycast(hs.built("host_sim"), tmp_path, c.scn, rays, base=c.base, threads=2)[0]["prim"]
    for e in ({}, {"SIM_TABS": "1"}, {"SIM_FORCE_FALLBACK": "0xf"}):
        def render(batch, rr, cap):
            kw = dict(cams=w.fcams, seeds=w.fseeds) if batch else dict(seed=hm.SEED)
            got, r = fw.host_sim(t, tmp_path, c.scn, hm.W, hm.H, None, hm.FEATURE_SPP, rr, cap, base=c.base, env=e, threads=2, **kw)
            _clean(r)
            return got
        nans = fw.assert_renders(render, cast, w, hm.FEATURE_SPP, hm.FOLLOW_SETTINGS, "%s follow %r" % (name, e), nan=True)
        assert (nans > 0) == (name == "hostile")


@pytest.mark.parametrize("which", ["host_sim", "host_sim_w5"])
@pytest.mark.parametrize("name", hm.SCENES)
def test_lanes_accumulate(api, case, chain_file, tmp_path, name, which):
    """--accumulate: 64 samples as 1 + 3 + 12 + 48 and as 26 + 1 + 37 -- a pass ends just before, and a pass of one sample takes,
    the sample at which a pixel of `hostile` overflows its Q -- against the fold of the REFERENCE's chains (chains_hostile.npz, no
    oracle in between); accumulate_cases.identity_2_per_pixel (maps, caps and rects that differ between the calls) against the
    oracle's chains, which test_oracle_chains_match_reference holds against the reference's; a batch of three views in two
    passes against the oracle's chains from each camera.  A continued job reloads sum, m2, count and state from the planes:
    here those words are huge, negative and infinite"""
    c = case(name)
    chain = hm.chains_from(chain_file, name)
    hm.accumulate_expected(chain, name)
    cams = hm.view_cameras(api, c)
    for e in _diffuse_sets(name) + [{"SIM_TABS": "1"}]:
        call = acs.host_call(hs.built(which), tmp_path, c, env=e, threads=2)
        for split in hm.accumulate_splits():
            acs.reference_split(call, chain, "%s accumulate %r %r" % (name, split, e), split, nan=True)
        acs.identity_2_per_pixel(call, c, "%s accumulate, per-pixel calls %r" % (name, e), chain=hm.chains_of(c), nan=True)
    single = acs.Planes()
    for n in (1, 3):
        call(single, None, n)
    acs.views_split(call, c, cams, hm.VIEW_SEEDS, (1, 3), name + " accumulate, views", nan=True, single=single)


# ---- part B on the CPU: the oracle alone meets the floors ----------------------------------------------------------------------------
def test_emission_scene_holds_nan_and_inf_pixels(api, oracle):
    """the oracle's 64 x 48 frame of hostile_materials.emission_scene: at least 8 NaN pixels, 8 inf pixels and 128 finite non-zero
    ones (measured: 68, 508 and 798 under PIXEL), so the GPU test that holds the device against the oracle there is not vacuous"""
    e = hm.emission_case(api, oracle)
    m = e.flat.materials
    assert np.isinf(m["emit"][5, 0]) and np.isnan(m["emit"][6, 0]) and m["emit"][7].tolist() == [-1, np.float32(3e38), np.float32(3e38)]
    for policy, chunk in POLICIES[:2]:
        img, _ = e.big().render(hm.EMIT_W, hm.EMIT_H, hm.SPP, hm.EMIT_SEED, policy, chunk=max(chunk, 1), rr=hm.RR, threads=8)
        nan = np.isnan(img).any(axis=2)
        inf = np.isinf(img).any(axis=2) & ~nan
        lit = np.isfinite(img).all(axis=2) & (img != 0).any(axis=2)
        print("%s: %d NaN pixels, %d inf pixels, %d finite non-zero pixels" % (policy, nan.sum(), inf.sum(), lit.sum()))
        assert nan.sum() >= 8 and inf.sum() >= 8 and lit.sum() >= 128
    cases = hm.ray_cases(e)
    exp, exp_ad, _ = hm.radiance_expected(e)   # what the GPU test of the queries relies on
    assert np.isnan(exp[0][cases.ok]).any() and np.isinf(exp[0][cases.ok]).any() and (~np.isfinite(exp_ad[2])).any()
    own, _ = hm.pixel_planes(e)
    assert np.isnan(own).any() and np.isinf(own).any()
