"""The device on hostile materials (tests/hostile_materials.py): every path-tracing kernel on scenes whose coefficients are NaN,
inf, negative, huge and vanishing, and (part B) on lights whose emission is.  A GPU build can differ from x86 exactly here -- NaN
through selects, inf and 0 products -- and the host checks (tests/test_hostile_materials_host.py: the loader, the oracle and the
host-compiled lane code against the same fixtures) cannot see that.

The plain renders are held against the REFERENCE'S OWN frames with no oracle in between (tests/golden/renders_hostile.npz,
make_golden.py --only-hostile), the adaptive and sample-map renders against the reference's chains (chains_hostile.npz), the
light groups against its dark twins; views, features and the ray and point queries against the oracle, which the host tests hold
against the reference on these very scenes.  Which kernel flavour each scene takes by itself is asserted on the CPU
(test_the_upload_guard_picks_the_diffuse_flavour_by_itself).  Everything is bit-exact, or NaN by position
(hostile_materials.same_words: the device's NaN need not carry x86's sign and payload); no pixel is skipped.  Frames are 24 x 16
unless said otherwise."""
import numpy as np
import pytest

import accumulate_cases as acs
import adaptive_cases as ac
import follow_cases as fw
import hostile_materials as hm
import irradiance_cases as ic
import light_groups_cases as lg
import radiance_cases as rc
import reference_goldens as rg
import render_adaptive_cases as rac
import sample_map_cases as sm
from test_follow_gpu import device_call as follow_device, host_call as follow_host
from test_gpu_adaptive import torch_run as adaptive_radiance_device
from test_gpu_features import device_call as features_device
from test_gpu_irradiance import torch_irradiance
from test_gpu_light_groups import torch_run as light_groups_device
from test_gpu_radiance import torch_radiance
from test_gpu_reference_goldens import KNOBS, knobs, uploaded  # noqa: F401  (knobs is a fixture)
from test_gpu_render_adaptive import torch_run as render_adaptive_device
from test_gpu_sample_map import torch_run as sample_map_device

pytestmark = pytest.mark.gpu

W, H = hm.W, hm.H
POLICIES = (("pixel", 0), ("chunk", 4), ("whole", 0), ("tile32", 0))
# name -> (environment, counters, the scenes it runs on)
KNOB_SETS = {
    "default": ({}, False, hm.SCENES),
    "exchange": ({"ORT_EXCHANGE": "1"}, False, hm.SCENES),
    "plain": ({"ORT_EXCHANGE": "0", "ORT_WAVES5": "0"}, False, hm.SCENES),
    "five": ({"ORT_EXCHANGE": "0", "ORT_WAVES5": "1"}, False, hm.SCENES),
    "wide": ({"ORT_WIDE": "1"}, False, hm.SCENES),
    "wavefront": ({"ORT_MODE": "wavefront"}, False, hm.SCENES),
    "hbm_tables": ({"ORT_LDS_TABLES": "0"}, False, hm.SCENES),
    "general": ({"ORT_KERNEL": "general"}, False, ("hostile_diffuse",)),
    "fallback": ({"ORT_DEBUG_FORCE_FALLBACK": "0xf"}, False, hm.SCENES),
    "counters": ({}, True, hm.SCENES),
}
assert {k for env, _, _ in KNOB_SETS.values() for k in env} <= set(KNOBS)


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
        uploaded(api, c.scene)
        return c
    return get


# ---- the plain render against the reference's frames --------------------------------------------------------------------------------
def test_plain_pixel_render_of_hostile(case, knobs, frames):
    """the narrowest case: `hostile`, PIXEL, the default plan"""
    knobs({})
    img, _ = case("hostile").scene.render(W, H, hm.SPP, hm.SEED, "pixel", rr=hm.RR)
    assert hm.same_words(img, frames[hm.key("hostile", "pixel", 0, (W, H))], "hostile PIXEL") == 0   # the guard drops every non-finite emission


@pytest.mark.parametrize("name,which", [(n, k) for n in hm.SCENES for k, v in KNOB_SETS.items() if n in v[2]])
def test_renders_match_reference(case, knobs, frames, name, which):
    """every policy the reference rendered the scene under (four for `hostile`, PIXEL and CHUNK for the diffuse twin), under
    every kernel the knobs reach; ORT_WIDE=1 asks for the wide tree where the scene has one and is the default plan elsewhere"""
    env, counters, _ = KNOB_SETS[which]
    c = case(name)
    knobs(env)
    done = 0
    for policy, chunk in POLICIES:
        key = hm.key(name, policy, chunk, (W, H))
        if key not in frames.files:
            continue
        img, st = c.scene.render(W, H, hm.SPP, hm.SEED, policy, chunk=chunk, rr=hm.RR, counters=counters)
        assert hm.same_words(img, frames[key], "%s %s, %s" % (name, policy, which)) == 0
        if counters:
            assert st["rays"] > 0 and st["paths"] > 0
        if which == "fallback":
            assert c.scene.render(W, H, hm.SPP, hm.SEED, policy, chunk=chunk, rr=hm.RR, counters=True)[1]["fallback_rays"] > 0
        done += 1
    assert done == (4 if name == "hostile" else 2)


@pytest.mark.parametrize("policy,chunk", POLICIES[:2])
def test_the_96_x_64_frame(case, knobs, frames, policy, chunk):
    """24 waves of mixed hostile and grey lanes, finite words above 1e20 and negative words among them"""
    knobs({})
    want = frames[hm.key("hostile", policy, chunk, hm.BIG)]
    img, _ = case("hostile").scene.render(hm.BIG[0], hm.BIG[1], hm.SPP, hm.SEED, policy, chunk=chunk, rr=hm.RR)
    assert hm.same_words(img, want, "hostile %s 96 x 64" % policy) == 0
    assert (np.isfinite(want) & (want > 1e20)).any() and (want < 0).any()


def test_render_device_form(api, case, knobs, frames):
    import torch
    knobs({})
    for name in hm.SCENES:
        d = torch.full((H, W, 3), -7.0, dtype=torch.float32, device="cuda")
        case(name).scene.render_device(d.data_ptr(), api.Scene.params(W, H, hm.SPP, hm.SEED, "chunk", 4, None, hm.RR), want_stats=True)
        hm.same_words(d.cpu().numpy(), frames[hm.key(name, "chunk", 4, (W, H))], name + " render_device")


# ---- views ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy,chunk", POLICIES[:2])
@pytest.mark.parametrize("name", hm.SCENES)
def test_render_views(api, case, knobs, name, policy, chunk):
    """three views -- the scene's own, light_groups_cases' second pose, and one up at the negative ceiling and the inf wall --
    against the oracle with set_camera; the host form and the device form"""
    import torch
    knobs({})
    c = case(name)
    cams = hm.view_cameras(api, c)
    want = hm.view_frames(c, cams, hm.VIEW_SEEDS, policy, chunk)
    got, _ = c.scene.render_views(cams, list(hm.VIEW_SEEDS), W, H, hm.SPP, policy, chunk=chunk, rr=hm.RR)
    hm.same_words(got, want, "%s views %s" % (name, policy))
    d = torch.full((3, H, W, 3), -7.0, dtype=torch.float32, device="cuda")
    c.scene.render_views_device(d.data_ptr(), api.Scene.params(W, H, hm.SPP, 0, policy, chunk, None, hm.RR), cams, list(hm.VIEW_SEEDS), want_stats=True)
    hm.same_words(d.cpu().numpy(), want, "%s views %s, the device form" % (name, policy))


# ---- the adaptive and the sample-map render, on the reference's chains ---------------------------------------------------------------
@pytest.mark.parametrize("ad", hm.ADAPTIVE_SETS, ids=["main", "late"])
@pytest.mark.parametrize("name", hm.SCENES)
def test_render_adaptive(case, knobs, chain_file, name, ad):
    """all four planes: min 16 (late: 32), max 64, a check every 16, render_adaptive_cases.FRAME's tolerance.  A pixel that reaches
    a check with Q = inf has v = inf - inf = NaN, which include/ort.h defines as keep sampling: it runs to max_spp and its m2 is
    inf (the diffuse twin under the main set, `hostile` under the late one; the host tests say why)"""
    knobs({})
    c = case(name)
    want = rac.expected_from(hm.chains_from(chain_file, name), W, H, ad)
    if (name, ad.min_spp) in (("hostile_diffuse", 16), ("hostile", 32)):
        assert (~np.isfinite(want[2])).any() and (want[1][~np.isfinite(want[2])] == ad.max_spp).all()
    got = c.scene.render_adaptive(W, H, ad.min_spp, ad.max_spp, ad.tolerance, ad.floor, ad.check_every, seed=hm.SEED, rr=hm.RR, want_states=True)[:4]
    dev, _ = render_adaptive_device(c.scene, ad, rr=hm.RR, seed=hm.SEED)
    for form, planes in (("host", got), ("device", dev)):
        for g, w_, what in zip(planes, want, ("colours", "sample counts", "second moments", "final states")):
            hm.same_words(g, w_, "%s adaptive %s, the %s form" % (name, what, form))
    x0, y0, x1, y1 = hm.RECT   # the device form on RECT: the planes' fill words stay outside it
    inside = {k: v for k, v in hm.chains_from(chain_file, name).items() if x0 <= k[0] < x1 and y0 <= k[1] < y1}
    dev, _ = render_adaptive_device(c.scene, ad, rr=hm.RR, seed=hm.SEED, rect=hm.RECT)
    for g, w_, what in zip(dev, rac.expected_from(inside, W, H, ad, guards=(-7.0, 0x5A5A5A5A, -7.0, 0x5A5A5A5A)), ("colours", "sample counts", "second moments", "final states")):
        hm.same_words(g, w_, "%s adaptive %s, the device form on a rect" % (name, what))


@pytest.mark.parametrize("name", hm.SCENES)
def test_render_sample_map(case, knobs, chain_file, name):
    """colours, m2 and states under sample_map_cases.mixed_map at cap 16, on guard-filled planes"""
    assert (sm.W, sm.H, sm.SEED, sm.RR, sm.RECT) == (W, H, hm.SEED, hm.RR, hm.RECT)
    knobs({})
    c = case(name)
    smap = sm.mixed_map()
    want = sm.expected_from(hm.chains_from(chain_file, name), smap, sm.CAP)
    got = c.scene.render_sample_map(W, H, smap, sm.CAP, hm.SEED, True, True, rr=hm.RR, out=sm.guards())[:3]
    dev, _ = sample_map_device(c, smap)
    for form, planes in (("host", got), ("device", dev)):
        for g, w_, what in zip(planes, want, ("colours", "second moments", "final states")):
            hm.same_words(g, w_, "%s sample map %s, the %s form" % (name, what, form))
    dev, _ = sample_map_device(c, smap, rect=hm.RECT)
    for g, w_, what in zip(dev, sm.expected_from(hm.chains_from(chain_file, name), smap, sm.CAP, rect=hm.RECT), ("colours", "second moments", "final states")):
        hm.same_words(g, w_, "%s sample map %s, the device form on a rect" % (name, what))


# ---- light groups, on the reference's dark twins ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hm.SCENES)
def test_render_light_groups(case, knobs, frames, name):
    """one group per light (G = 3) and all lights in one (G = 1): group frames, the unsplit frame and the final states.  The dark
    twins of `hostile` are the reference's frames of the files; the diffuse twin's are the oracle's"""
    assert (lg.W, lg.H, lg.SEED, lg.RR) == (W, H, hm.SEED, hm.RR)
    knobs({})
    c = case(name)
    if name == "hostile":
        own, states = frames[hm.key(name, "pixel", 0, (W, H))], frames[hm.key(name, "pixel", 0, (W, H)) + "__states"]
        twins = [frames[hm.key("hostile_dark%d" % g, "pixel", 0, (W, H))] for g in range(3)]
    else:
        own, states = hm.pixel_planes(c)
        twins = [c.twin([m]).render(W, H, hm.SPP, hm.SEED, "pixel", rr=hm.RR, threads=8)[0] for m in c.lights]
        hm.same_words(own, frames[hm.key(name, "pixel", 0, (W, H))], "the oracle's own frame")
    for groups, G in ((c.per_light(), 3), ({m: 0 for m in c.lights}, 1)):
        out = [np.full((G, H, W, 3), lg.GUARD_F, "<f4"), np.full((H, W, 3), lg.GUARD_F, "<f4"), np.full((H, W), lg.GUARD_STATE, "<u4")]
        host = c.scene.render_light_groups(W, H, hm.SPP, hm.SEED, c.table(groups), True, True, group_count=G, rr=hm.RR, out=out)[:3]
        dev, _ = light_groups_device(c, groups, G, hm.SPP)
        for form, (fr, rgb, st) in (("host", host), ("device", dev)):
            for g in range(G):
                hm.same_words(fr[g], twins[g] if G == 3 else own, "%s light groups G = %d, group %d, the %s form" % (name, G, g, form))
            hm.same_words(rgb, own, "%s light groups: the unsplit frame, the %s form" % (name, form))
            hm.same_words(st, states, "%s light groups: final states, the %s form" % (name, form))


# ---- features ---------------------------------------------------------------------------------------------------------------------------
class _Views:
    pass


@pytest.mark.parametrize("name", hm.SCENES)
def test_render_features(api, case, knobs, name):
    """all planes against feature_cases' oracle planes, the single frame and a batch of three views.  The albedo plane holds NaN
    (the scene's own view: the nan wall), inf and negative sums (the view up at the inf wall and the neg ceiling)"""
    knobs({})
    c = case(name)
    cams = hm.view_cameras(api, c)
    want = hm.feature_expected(c, cams, hm.VIEW_SEEDS)
    alb = np.stack([w_["albedo"] for w_ in want])
    assert np.isnan(alb).any() and np.isinf(alb).any() and (alb < 0).any()
    planes = ("albedo", "normal", "depth", "hits", "ids", "states")
    got, _ = c.scene.render_features(W, H, hm.FEATURE_SPP, hm.SEED, want=planes)
    assert hm.assert_features(got, want[0], name + " features") > 0
    got, _ = c.scene.render_views_features(cams, list(hm.VIEW_SEEDS), W, H, hm.FEATURE_SPP, want=planes)
    for v in range(3):
        hm.assert_features({k: a[v] for k, a in got.items()}, want[v], "%s features, view %d" % (name, v))
    w = _Views()
    w.scene, w.size, w.cams, w.seeds = c.scene, (W, H), cams, list(hm.VIEW_SEEDS)
    dev, _ = features_device(api, w, hm.FEATURE_SPP, True)
    for v in range(3):
        hm.assert_features({k: a[v] for k, a in dev.items()}, want[v], "%s features, view %d, the device form" % (name, v))
    dev, _ = features_device(api, w, hm.FEATURE_SPP, False)
    hm.assert_features({k: a[0] for k, a in dev.items()}, want[0], name + " features, the device form")


# ---- the accumulating renders, on the reference's chains ------------------------------------------------------------------------------
ACCUMULATE_KNOBS = ("default", "hbm_tables", "general", "fallback", "counters")


@pytest.mark.parametrize("name,which", [(n, k) for n in hm.SCENES for k in ACCUMULATE_KNOBS if n in KNOB_SETS[k][2]])
def test_render_accumulate(api, case, knobs, chain_file, name, which):
    """ort_render_accumulate: 64 samples as 1 + 3 + 12 + 48 and as 26 + 1 + 37 -- a pass ends just before, and a pass of one sample
    takes, the sample at which a pixel of `hostile` overflows its Q -- against the fold of the REFERENCE's chains with no oracle
    in between, every plane after every pass.  A continued job reloads sum, m2, count and state from memory: huge, negative and
    infinite words here.  Under the default plan also accumulate_cases.identity_2_per_pixel against the oracle's chains"""
    env, counters, _ = KNOB_SETS[which]
    c = case(name)
    chain = hm.chains_from(chain_file, name)
    hm.accumulate_expected(chain, name)
    knobs(env)
    call = acs.library_call(api, c, counters=counters)
    for split in hm.accumulate_splits():
        acs.reference_split(call, chain, "%s accumulate %r, %s" % (name, split, which), split, nan=True)
    if which == "default":
        acs.identity_2_per_pixel(call, c, name + " accumulate, per-pixel calls", chain=hm.chains_of(c), nan=True)


@pytest.mark.parametrize("name", hm.SCENES)
def test_render_accumulate_device_forms_and_views(api, case, knobs, chain_file, name):
    """the 26 + 1 + 37 split through the _device forms on a non-default stream, guard words around every plane and no
    synchronisation between the passes, against the fold of the reference's chains; and ort_render_views_accumulate on the
    file's three views in passes of 1 + 3 against the oracle's chains from each camera, frame 0 the single-frame form's"""
    knobs({})
    c = case(name)
    chain = hm.chains_from(chain_file, name)
    want = acs.Planes()
    for k in hm.OVERFLOW_SPLIT:
        acs.model(want, 0, chain, None, k, None)
    acs.assert_planes(acs.stream_split(c, hm.OVERFLOW_SPLIT), want, name + " accumulate, the device forms on a stream", nan=True)
    call = acs.library_call(api, c)
    single = acs.Planes()
    for n in (1, 3):
        call(single, None, n)
    acs.views_split(call, c, hm.view_cameras(api, c), hm.VIEW_SEEDS, (1, 3), name + " accumulate, views", nan=True, single=single)


FOLLOW_KNOBS = ("default", "hbm_tables", "general", "fallback", "counters")


@pytest.mark.parametrize("name,which", [(n, k) for n in hm.SCENES for k in FOLLOW_KNOBS if n in KNOB_SETS[k][2]])
def test_render_follow(api, case, knobs, name, which):
    """ort_render_follow and ort_render_views_follow against follow_cases' chain, which tests/test_hostile_materials_host.py pins
    against the oracle's diffuse twin on these very frames: the single frame and a batch of three views (the scene's own camera,
    WALL_CAM at the nan and the zero wall, UP_CAM at neg and inf) at (spp 5, rr 0.5, cap 64) and (rr 0.8, cap 2), all seven planes,
    ids' shapes through ort_raycast of the chains' last rays.  The terminal test meets NaN, 1e-30, all-zero, inf and negative Kd;
    the followed ones draw sample_brdf without a lobe, their records come from LDS (default) or from HBM (hbm_tables), the burn
    reads the lights' table in LDS, and `fallback` hands the bounce rays to the exact walk.  Under the default plan the device
    forms too, on a non-default stream over guard words.  No bounce ray of these frames has a non-finite direction (the oracle's
    count is 0): the NaN words are the nan wall's Kd recorded at the cap"""
    env, counters, _ = KNOB_SETS[which]
    c = case(name)
    assert hm.follow_conditions(c) == 0
    w = hm.follow_world(c)
    knobs(env)
    cast = lambda rays: c.scene.raycast(rays)[0]["prim"]
    rays = {}

    def host(batch, rr, cap):
        got, st = follow_host(w, hm.FEATURE_SPP, batch, rr=rr, cap=cap, counters=counters)
        rays[(batch, rr, cap)] = st["rays"]
        return got
    nans = fw.assert_renders(host, cast, w, hm.FEATURE_SPP, hm.FOLLOW_SETTINGS, "%s follow, %s" % (name, which), nan=True)
    assert (nans > 0) == (name == "hostile")
    if counters:
        for rr, cap in hm.FOLLOW_SETTINGS:
            ch = fw.chains(w, hm.FEATURE_SPP, rr, cap)
            assert rays[(False, rr, cap)] == ch[0].rays and rays[(True, rr, cap)] == sum(k.rays for k in ch[1:])
    if which == "fallback":
        assert follow_host(w, hm.FEATURE_SPP, True, counters=True)[1]["fallback_rays"] > 0
    if which == "default":
        device = lambda batch, rr, cap: follow_device(api, w, hm.FEATURE_SPP, batch, rr=rr, cap=cap)[0]
        fw.assert_renders(device, cast, w, hm.FEATURE_SPP, hm.FOLLOW_SETTINGS, "%s follow, the device forms" % name, nan=True)


# ---- the ray and point queries -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hm.SCENES)
def test_radiance_and_adaptive_radiance(case, knobs, name):
    """radiance_cases.mixed's 64 rays (8 outside the domain) and 16 aimed at the sphere under the light: colours and states at
    4 spp, and colours, states, spp and m2 under adaptive_cases.MAIN, there and on adaptive_cases.cases_for's rays, which hold
    all three classes of the stopping rule; host and device forms"""
    knobs({})
    c = case(name)
    cases = hm.ray_cases(c)
    exp, exp_ad, exp_noisy = hm.radiance_expected(c)
    rgb, fin, _ = c.scene.radiance(cases.rays, cases.seeds, hm.QUERY_SPP, hm.RR, want_states=True)
    rc.assert_same(rgb, fin, exp[0], exp[1], name + " radiance")
    rgb, fin, _ = torch_radiance(c.scene, cases.rays, cases.seeds, hm.QUERY_SPP, hm.RR)
    rc.assert_same(rgb, fin, exp[0], exp[1], name + " radiance, the device form")
    m = ac.MAIN
    got = c.scene.radiance_adaptive(cases.rays, cases.seeds, m.min_spp, m.max_spp, m.tolerance, m.floor, m.check_every, hm.RR, want_states=True)[:4]
    ac.assert_same(got, exp_ad, name + " adaptive radiance")
    ac.assert_same(adaptive_radiance_device(c.scene, cases, m, hm.RR)[0], exp_ad, name + " adaptive radiance, the device form")
    noisy = hm.noisy_ray_cases(c)
    assert min(ac.classes(exp_noisy[1], exp_noisy[0], noisy.ok, m)[:3]) >= 0.1   # stopped at min_spp, between, ran to max_spp
    got = c.scene.radiance_adaptive(noisy.rays, noisy.seeds, m.min_spp, m.max_spp, m.tolerance, m.floor, m.check_every, hm.RR, want_states=True)[:4]
    ac.assert_same(got, exp_noisy, name + " adaptive radiance, the noisy rays")
    ac.assert_same(adaptive_radiance_device(c.scene, noisy, m, hm.RR)[0], exp_noisy, name + " adaptive radiance, the noisy rays, the device form")


@pytest.mark.parametrize("name", hm.SCENES)
def test_irradiance_and_adaptive_irradiance(case, knobs, name):
    """irradiance_cases' 64 points: identity I1 -- sample k is the radiance query (held above) at spp = 1 along the direction the
    oracle draws -- for 8 samples, and adaptive_cases.cut over 17 under irradiance_cases.EVERY; host and device forms"""
    knobs({})
    c = case(name)
    pts = hm.point_set(c)
    one = lambda rays, seeds: c.scene.radiance(rays, seeds, 1, hm.RR, want_states=True)[:2]
    chain = ic.chain_by_radiance(c.oracle, pts, 17, one)
    w_rgb, w_fin = ic.expected_from(chain, pts, 8)
    rgb, fin, _ = c.scene.irradiance(pts.points, pts.seeds, 8, hm.RR, want_states=True)
    rc.assert_same(rgb, fin, w_rgb, w_fin, name + " irradiance")
    (rgb, _, _, fin), _ = torch_irradiance(c.scene, pts.points, pts.seeds, 8, hm.RR)
    rc.assert_same(rgb, fin, w_rgb, w_fin, name + " irradiance, the device form")
    e = ic.EVERY
    want = ic.expected_adaptive(chain, pts, e)
    got = c.scene.irradiance_adaptive(pts.points, pts.seeds, e.min_spp, e.max_spp, e.tolerance, e.floor, e.check_every, hm.RR, want_states=True)[:4]
    ac.assert_same(got, want, name + " adaptive irradiance")
    ac.assert_same(torch_irradiance(c.scene, pts.points, pts.seeds, 0, hm.RR, ad=e)[0], want, name + " adaptive irradiance, the device form")


# ---- part B: non-finite emission, which a file cannot say --------------------------------------------------------------------------------
@pytest.fixture()
def emission(api, oracle):
    e = hm.emission_case(api, oracle)
    uploaded(api, e.scene)
    return e


@pytest.mark.parametrize("policy,chunk", POLICIES[:2])
def test_non_finite_emission_plain_render(emission, knobs, policy, chunk):
    """hostile_materials.emission_scene at 64 x 48 against the oracle (with_reference_csg=False).  The reference cannot read this
    scene -- its `light` statement takes integers -- so the oracle alone answers; its emission code is pinned against the
    reference on the file scenes above.  A primary hit on such a light is unguarded: the frame DOES hold NaN and inf pixels"""
    knobs({})
    e = emission
    want, _ = e.big().render(hm.EMIT_W, hm.EMIT_H, hm.SPP, hm.EMIT_SEED, policy, chunk=max(chunk, 1), rr=hm.RR, threads=8)
    nan = np.isnan(want).any(axis=2)
    assert nan.sum() >= 8 and (np.isinf(want).any(axis=2) & ~nan).sum() >= 8 and (np.isfinite(want).all(axis=2) & (want != 0).any(axis=2)).sum() >= 128
    img, _ = e.scene.render(hm.EMIT_W, hm.EMIT_H, hm.SPP, hm.EMIT_SEED, policy, chunk=chunk, rr=hm.RR)
    assert hm.same_words(img, want, "non-finite emission, %s" % policy) >= 8


def test_non_finite_emission_groups_features_adaptive_and_radiance(api, emission, knobs):
    """the light-group (one group per light, G = 4), feature and adaptive renders at 24 x 16 and the radiance query, against the
    oracle: the group sums, the albedo plane and m2 all carry inf and NaN here"""
    knobs({})
    e = emission
    own, states = hm.pixel_planes(e)
    assert np.isnan(own).any() and np.isinf(own).any()
    groups = e.per_light()
    fr, rgb, st, _ = e.scene.render_light_groups(W, H, hm.SPP, hm.SEED, e.table(groups), True, True, group_count=4, rr=hm.RR)
    for g, m in enumerate(e.lights):
        hm.same_words(fr[g], e.twin([m]).render(W, H, hm.SPP, hm.SEED, "pixel", rr=hm.RR, threads=8)[0], "non-finite emission: group %d" % g)
    assert hm.same_words(rgb, own, "non-finite emission: the unsplit frame") > 0
    hm.same_words(st, states, "non-finite emission: final states")
    want = hm.feature_expected(e, [e.cam], [hm.SEED])[0]
    assert np.isnan(want["albedo"]).any() and np.isinf(want["albedo"]).any() and (want["albedo"] < 0).any()
    got, _ = e.scene.render_features(W, H, hm.FEATURE_SPP, hm.SEED, want=("albedo", "normal", "depth", "hits", "ids", "states"))
    hm.assert_features(got, want, "non-finite emission: features")
    ad = hm.adaptive_set()
    want = rac.expected_from(hm.chains_of(e), W, H, ad)
    assert np.isnan(want[2]).any() or np.isinf(want[2]).any()
    got = e.scene.render_adaptive(W, H, ad.min_spp, ad.max_spp, ad.tolerance, ad.floor, ad.check_every, seed=hm.SEED, rr=hm.RR, want_states=True)[:4]
    for g, w_, what in zip(got, want, ("colours", "sample counts", "second moments", "final states")):
        hm.same_words(g, w_, "non-finite emission: adaptive " + what)
    cases = hm.ray_cases(e)
    exp, exp_ad, _ = hm.radiance_expected(e)
    assert np.isnan(exp[0][cases.ok]).any() and np.isinf(exp[0][cases.ok]).any() and (~np.isfinite(exp_ad[2])).any()
    rgb, fin, _ = e.scene.radiance(cases.rays, cases.seeds, hm.QUERY_SPP, hm.RR, want_states=True)
    rc.assert_same(rgb, fin, exp[0], exp[1], "non-finite emission: radiance")
    m = ac.MAIN
    got = e.scene.radiance_adaptive(cases.rays, cases.seeds, m.min_spp, m.max_spp, m.tolerance, m.floor, m.check_every, hm.RR, want_states=True)[:4]
    ac.assert_same(got, exp_ad, "non-finite emission: adaptive radiance")
