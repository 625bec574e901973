"""The device on hostile shapes (tests/hostile_shapes.py): spheres of radius -0.5, 0 and 1e-20, boxes with max < min, cylinders
with a zero axis, a negative or a zero radius, meshes scaled by 0, -0.6 and 1e-20, lights made of such shapes, and single shapes of
size 1e12, 1e6 and 1e8.  A GPU build can differ from x86 exactly here -- NaN through min and max, 0/0, denormal products, a
division by a zero length in light sampling --, and the host checks (tests/test_hostile_shapes_host.py: the loader, the oracle
and the host-compiled lane code on the same fixtures) cannot see what it makes of it.

Everything is held against the REFERENCE'S OWN output (tests/golden/raycast_shapes.npz, renders_shapes.npz, chains_shapes.npz;
make_golden.py --only-shapes) where the reference has a form for it, and against the oracle, which the host tests hold against
the reference on these scenes, elsewhere (views, features, ray and point queries, the exact walk at 4 spp, the scene of arrays).
hostile_materials.same_words compares: bit for bit, NaN matching NaN; no pixel, ray or point is skipped.  Frames are 24 x 16 at
16 spp unless said otherwise."""
import numpy as np
import pytest

import accumulate_cases as acs
import adaptive_cases as ac
import ao_cases as ao
import feature_cases as fc
import follow_cases as fw
import hostile_materials as hm
import hostile_shapes as hsh
import irradiance_cases as ic
import light_groups_cases as lg
import occluded_cases as oc
import radiance_cases as rc
import reference_goldens as rg
import render_adaptive_cases as rac
import sample_map_cases as sm
from raycast_cases import assert_same_answers
from test_follow_gpu import device_call as follow_device, host_call as follow_host
from test_gpu_adaptive import torch_run as adaptive_radiance_device
from test_gpu_ao import torch_form as ao_device
from test_gpu_features import device_call as features_device
from test_gpu_irradiance import torch_irradiance
from test_gpu_light_groups import torch_run as light_groups_device
from test_gpu_occluded import torch_occluded
from test_gpu_radiance import torch_radiance
from test_gpu_raycast import torch_raycast
from test_gpu_raycast_edges import check_records
from test_gpu_reference_goldens import KNOBS, knobs, uploaded  # noqa: F401  (knobs is a fixture)
from test_gpu_render_adaptive import torch_run as render_adaptive_device
from test_gpu_sample_map import torch_run as sample_map_device
from test_gpu_void_material import VARIANTS

pytestmark = pytest.mark.gpu

W, H = hsh.W, hsh.H
same = hsh.same_words
EVERYWHERE = ["default", "hbm_tables", "fallback", "exact", "wide", "counters"]
# for the other calls: their tests pass no counters flag, and up to 64 samples a pixel with every ray on the exact walk take too long
PLANS = [k for k in EVERYWHERE if k not in ("counters", "exact")]
assert {k for w in EVERYWHERE for k in VARIANTS[w][0]} <= set(KNOBS)
EXACT_SPP = 4


@pytest.fixture(scope="module")
def frames():
    return rg.load("renders_shapes.npz")


@pytest.fixture(scope="module")
def chain_file():
    return rg.load("chains_shapes.npz")


@pytest.fixture(scope="module")
def hits_file():
    return rg.load("raycast_shapes.npz")


@pytest.fixture()
def case(api, oracle, manifest, tmp_path_factory, monkeypatch):
    def get(name, commit=""):
        if name in hsh.ARRAYS:
            c = hsh.arrays_case(api, oracle, name)
        else:
            if commit:
                for k, v in hsh.PROLOGUE_WIDE.items():
                    monkeypatch.setenv(k, v)
            c = hsh.case(api, oracle, name, tmp_path_factory, commit)
            for k in hsh.PROLOGUE_WIDE:
                monkeypatch.delenv(k, raising=False)
            if name not in hsh.SPECULAR:   # those are written for the follow renders alone: the reference has no fixture of them
                assert rg.sha256(c.scn) == manifest["generated"]["shapes"]["scenes"][name]["scn_sha256"], name
            if name in ("shapes_seen", "shapes_seen_specular"):   # 11 boxes and 2 spheres; every box and sphere and one cylinder
                assert c.scene.tree_info()["prologue_prims"] == (17 if commit else 13)
        uploaded(api, c.scene)
        return c
    return get


# ---- closest hits ----------------------------------------------------------------------------------------------------------------------
def test_plain_closest_hits_on_shapes_seen(case, knobs, manifest, hits_file):
    """the narrowest case: the default plan, the host form, the reference's records.  The rays are regenerated (the manifest
    holds their SHA-256)"""
    knobs({})
    c = case("shapes_seen")
    rays, kind = hsh.rays_of(c)
    assert hsh.rays_sha256(rays) == manifest["generated"]["shapes"]["raycast"]["rays_sha256"]
    hits, _ = c.scene.raycast(rays)
    z = hits_file
    assert_same_answers(hits["t"], hits["n"], hits["mat"], z["t"], z["n"], z["mat"], "shapes_seen, the host form")


@pytest.mark.parametrize("name", ("shapes_seen", "shapes_seen@prologue24", "shapes_leaves"))
@pytest.mark.parametrize("which", EVERYWHERE)
def test_closest_hits_and_occlusion(api, case, knobs, hits_file, which, name):
    """shapes_seen (hostile boxes and a sphere in the prologue), its commit with a hostile cylinder in the prologue, and
    shapes_leaves (every hostile shape in a tree leaf), the same rays on each: host and device forms against the reference's
    t, n and mat, per kind of ray; every record's prim against the shape that
    its t and n belong to (test_gpu_raycast_edges.check_records: the reported shape, intersected alone by the device's generic
    intersectors, gives the same record -- a hostile shape too).  Then ort_occluded over occluded_cases' ladder on the reference's
    t -- tmax one ulp either side of each hit --, without limits and with the scalar +inf; host and device forms"""
    env, counters = VARIANTS[which]
    name, _, commit = name.partition("@")
    commit = "@" + commit if commit else ""
    c = case(name, commit)
    rays, kind = hsh.rays_of(case("shapes_seen"))
    z = dict(zip(("t", "n", "mat"), hsh.records(hits_file, name)))
    sel = hsh.exact_subset(kind) if which == "exact" else np.ones(len(rays), bool)
    r = rays[sel]
    knobs(env)
    hits, st = c.scene.raycast(r, counters=counters)
    for k, what in enumerate(hsh.RAY_KINDS):
        s = kind[sel] == k
        assert_same_answers(hits["t"][s], hits["n"][s], hits["mat"][s], z["t"][sel][s], z["n"][sel][s], z["mat"][sel][s], "%s%s %s, rays at %s" % (name, commit, which, what))
    if counters:
        assert st["rays"] == len(r)
    if which in ("fallback", "exact"):
        assert st["fallback_rays"] > 0
    dh, _ = torch_raycast(c.scene, r, counters=counters)
    assert dh.tobytes() == hits.tobytes()
    assert hsh.hostile_hit(hits["mat"]).sum() >= 0.1 * len(r)
    for n in hsh.HIT:
        assert (hits["mat"] == hsh.MAT[n]).any(), n
    finite = np.isfinite(r).all(axis=1) & ~np.isnan(hits["t"])
    check_records(api, c.scene, c.flat, r[finite], hits[finite], "%s%s %s" % (name, commit, which))
    t, mat = z["t"][sel], z["mat"][sel]
    ok = ~np.isnan(t)
    rr, tm, want = hsh.one_ulp_ladder(r[ok], t[ok], mat[ok])
    assert want.mean() >= 0.1 and (~want).mean() >= 0.1
    got, st = c.scene.occluded(rr, tm, counters=counters)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "%s, host form: %d of %d bytes differ, first %d (tmax %r)" % (which, len(bad), len(want), bad[0], tm[bad[0]])
    if counters:
        assert st["rays"] == len(rr)
    assert (torch_occluded(c.scene, rr, tm, counters=counters)[0] == want).all(), which + ", device form"
    unlimited = (mat[ok] != 0) & (t[ok] < np.inf)
    for limit in (None, np.float32(np.inf)):
        assert (c.scene.occluded(r[ok], limit)[0] == unlimited).all(), (which, limit)
    assert (torch_occluded(c.scene, r[ok], None)[0] == unlimited).all()


@pytest.mark.parametrize("which", EVERYWHERE)
def test_closest_hits_and_occlusion_on_the_scene_of_arrays(api, case, knobs, which):
    """a radius of -0.0 and a denormal one, a box with min == max, a repeated vertex index, hostile shapes that carry material 0:
    2 000 rays against the oracle's t, n and mat, each record's prim against the shape it names, the occlusion ladder over the
    oracle's t; host and device forms"""
    env, counters = VARIANTS[which]
    c = case("arrays_shapes")
    rays = hsh.arrays_rays(c)
    if which == "exact":
        rays = np.ascontiguousarray(rays[::2])
    t, n, mat = c.twin(None).raycast(rays[:, 0:3], rays[:, 3:6])
    knobs(env)
    hits, st = c.scene.raycast(rays, counters=counters)
    assert_same_answers(hits["t"], hits["n"], hits["mat"], t, n, mat, "arrays_shapes %s" % which)
    if which in ("fallback", "exact"):
        assert st["fallback_rays"] > 0
    check_records(api, c.scene, c.flat, rays, hits, "arrays_shapes %s" % which)
    assert torch_raycast(c.scene, rays, counters=counters)[0].tobytes() == hits.tobytes()
    rr, tm, want, _ = oc.laddered(rays, t, mat)
    assert want.mean() >= 0.1 and (~want).mean() >= 0.1
    got, _ = c.scene.occluded(rr, tm, counters=counters)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "arrays_shapes %s: %d of %d bytes differ, first %d" % (which, len(bad), len(want), bad[0])
    assert (torch_occluded(c.scene, rr, tm, counters=counters)[0] == want).all()


# ---- ambient occlusion ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", EVERYWHERE)
def test_ambient_occlusion(case, knobs, hits_file, which):
    """192 points lifted off the hostile shapes' hit points (every shape of hostile_shapes.HIT has some) at
    ao_cases.radius_array's radii and without a radius; host and device forms"""
    env, counters = VARIANTS[which]
    c = case("shapes_seen")
    pts = hsh.points_of(c, hits_file)
    assert set(pts[2].tolist()) == {hsh.MAT[n] for n in hsh.HIT}
    w = hsh.ao_world(c, pts[:2])
    knobs(env)
    for radius in (w.radii, None):
        want = ao.expected(w, radius, 8)
        out, bent, fin, st = c.scene.ambient_occlusion(w.pts.points, w.pts.seeds, 8, radius=radius, want_bent=True, want_states=True, counters=counters)
        ao.assert_same((out, bent, fin), want, "shapes_seen AO %s" % which)
        if counters:
            assert st["rays"] == 8 * len(w.pts.points)
        got, _ = ao_device(c.scene, w.pts.points, w.pts.seeds, radius, 8)
        ao.assert_same(got, want, "shapes_seen AO %s, the device form" % which)


# ---- the plain renders ---------------------------------------------------------------------------------------------------------------------
def test_plain_pixel_render_of_shapes_seen(case, knobs, frames):
    """the narrowest render: shapes_seen, PIXEL, the default plan, the reference's frame"""
    knobs({})
    img, _ = case("shapes_seen").scene.render(W, H, hsh.SPP, hsh.SEED, "pixel", rr=hsh.RR)
    same(img, frames[hsh.key("shapes_seen", "pixel", 0, (W, H))], "shapes_seen PIXEL")


@pytest.mark.parametrize("which", EVERYWHERE)
@pytest.mark.parametrize("name", hsh.SCENES + ("shapes_seen@prologue24",))
def test_renders_match_reference(api, case, knobs, frames, name, which):
    """the four policies under every kernel the knobs reach, against the reference's frames.  Under ORT_DEBUG_FORCE_FALLBACK=0
    (every ray on the exact walk) 4 spp, against the oracle.  Under the default plan also a rect, the union of three shards and
    the device form (PIXEL and CHUNK)"""
    import torch
    env, counters = VARIANTS[which]
    name, _, commit = name.partition("@")
    c = case(name, "@" + commit if commit else "")
    knobs(env)
    for policy, chunk in hsh.POLICIES:
        if which == "exact":
            want = hsh.oracle_frame(c, (W, H), policy, chunk, spp=EXACT_SPP)
            img, st = c.scene.render(W, H, EXACT_SPP, hsh.SEED, policy, chunk=chunk, rr=hsh.RR, counters=True)
            assert st["fallback_rays"] == st["rays"] > 0
        else:
            want = frames[hsh.key(name, policy, chunk, (W, H))]
            img, st = c.scene.render(W, H, hsh.SPP, hsh.SEED, policy, chunk=chunk, rr=hsh.RR, counters=counters)
        same(img, want, "%s %s, %s" % (name + commit, policy, which))
        if counters:
            ost = c.twin(None).render(W, H, hsh.SPP, hsh.SEED, policy, chunk=max(chunk, 1), rr=hsh.RR, threads=8)[1]
            assert (st["rays"], st["paths"]) == (ost["rays"], ost["paths"]), policy
        if which != "default" or policy not in ("pixel", "chunk"):
            continue
        got, _ = c.scene.render(W, H, hsh.SPP, hsh.SEED, policy, chunk=chunk, rect=hsh.RECT, rr=hsh.RR)
        x0, y0, x1, y1 = hsh.RECT
        if policy == "pixel":     # a pixel's job is its own: the rect's pixels are the frame's
            same(got[y0:y1, x0:x1], want[y0:y1, x0:x1], "%s %s, a rect" % (name, policy))
        else:
            same(got[y0:y1, x0:x1], hsh.oracle_frame(c, (W, H), policy, chunk, rect=hsh.RECT)[y0:y1, x0:x1], "%s %s, a rect" % (name, policy))
        union = np.zeros((H, W, 3), "<f4")
        for k in range(3):
            part, _ = c.scene.render(W, H, hsh.SPP, hsh.SEED, policy, chunk=chunk, rr=hsh.RR, shard=(k, 3))
            union = np.where(part.view("<u4") != 0, part, union)
        same(union, want, "%s %s, the union of three shards" % (name, policy))
        d = torch.full((H, W, 3), -7.0, dtype=torch.float32, device="cuda")
        c.scene.render_device(d.data_ptr(), api.Scene.params(W, H, hsh.SPP, hsh.SEED, policy, chunk, None, hsh.RR), want_stats=True)
        same(d.cpu().numpy(), want, "%s %s, the device form" % (name, policy))


@pytest.mark.parametrize("which", EVERYWHERE)
def test_renders_of_the_scene_of_arrays(case, knobs, which):
    """the four policies on the scene of arrays -- a radius of -0.0 and a denormal one, a box with min == max, a repeated vertex
    index, hostile shapes that carry material 0 -- against the oracle; under the exact walk 4 spp"""
    env, counters = VARIANTS[which]
    c = case("arrays_shapes")
    spp = EXACT_SPP if which == "exact" else hsh.SPP
    knobs(env)
    for policy, chunk in hsh.POLICIES:
        want = hsh.oracle_frame(c, (W, H), policy, chunk, spp=spp)
        img, st = c.scene.render(W, H, spp, hsh.SEED, policy, chunk=chunk, rr=hsh.RR, counters=counters or which == "exact")
        same(img, want, "arrays_shapes %s, %s" % (policy, which))
        assert bool(want.view("<u4").any())
        if which == "exact":
            assert st["fallback_rays"] == st["rays"] > 0


@pytest.mark.parametrize("policy,chunk", hsh.POLICIES[:2])
@pytest.mark.parametrize("name", hsh.SCENES)
def test_the_96_x_64_frames(case, knobs, frames, name, policy, chunk):
    """24 waves of lanes that meet hostile and ordinary shapes side by side, against the reference's frames"""
    knobs({})
    img, _ = case(name).scene.render(hsh.BIG[0], hsh.BIG[1], hsh.SPP, hsh.SEED, policy, chunk=chunk, rr=hsh.RR)
    same(img, frames[hsh.key(name, policy, chunk, hsh.BIG)], "%s %s 96 x 64" % (name, policy))


# ---- views -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", PLANS)
@pytest.mark.parametrize("policy,chunk", hsh.POLICIES[:2])
@pytest.mark.parametrize("name", ("shapes_seen", "shapes_lights", "shapes_leaves") + hsh.ARRAYS)
def test_render_views_one_inside_the_negative_sphere(api, case, knobs, name, policy, chunk, which):
    """three views: the scene's own, light_groups_cases' second pose, and one standing at the centre of the sphere of radius -0.5
    (shapes_lights, the arrays: a step nearer the table); host and device forms, and under PIXEL view 0 of the adaptive batch
    against the single-frame adaptive call, which the test below holds against the reference's chains"""
    import torch
    knobs(VARIANTS[which][0])
    c = case(name)
    cams = hsh.view_cameras(api, c)
    spp = hsh.SPP
    want = np.stack([hsh.oracle_frame(c, (W, H), policy, chunk, cam=cam, seed=s, spp=spp) for cam, s in zip(cams, hsh.VIEW_SEEDS)])
    assert all(w_.view("<u4").any() for w_ in want)
    got, _ = c.scene.render_views(cams, list(hsh.VIEW_SEEDS), W, H, spp, policy, chunk=chunk, rr=hsh.RR)
    same(got, want, "%s views %s" % (name, policy))
    d = torch.full((3, H, W, 3), -7.0, dtype=torch.float32, device="cuda")
    c.scene.render_views_device(d.data_ptr(), api.Scene.params(W, H, spp, 0, policy, chunk, None, hsh.RR), cams, list(hsh.VIEW_SEEDS), want_stats=True)
    same(d.cpu().numpy(), want, "%s views %s, the device form" % (name, policy))
    if policy == "pixel":
        ad = hm.adaptive_set()
        rgb, spp, m2, fin = c.scene.render_views_adaptive(cams, list(hsh.VIEW_SEEDS), W, H, ad.min_spp, ad.max_spp, ad.tolerance, ad.floor, ad.check_every,
                                                          rr=hsh.RR, want_states=True)[:4]
        own = c.scene.render_adaptive(W, H, ad.min_spp, ad.max_spp, ad.tolerance, ad.floor, ad.check_every, seed=hsh.VIEW_SEEDS[0], rr=hsh.RR, want_states=True)[:4]
        for g, w_, what in zip((rgb[0], spp[0], m2[0], fin[0]), own, ("colours", "sample counts", "second moments", "final states")):
            same(g, w_, "%s view 0 of the adaptive batch: %s" % (name, what))


@pytest.mark.parametrize("which", PLANS)
# ---- the adaptive and the sample-map render ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hsh.CHAINS + hsh.ARRAYS)
def test_render_adaptive_and_sample_map(case, knobs, chain_file, name, which):
    """all four planes of the adaptive render (min 16, max 64, a check every 16) on the reference's chains (the oracle's for the
    scene of arrays), then the sample-map render fed that call's counts.  Host and device forms, the device form on a rect"""
    knobs(VARIANTS[which][0])
    c = case(name)
    chain = hsh.chains_from(chain_file, name) if name in hsh.CHAINS else hsh.chains_of(c)
    ad = hm.adaptive_set()
    want = rac.expected_from(chain, W, H, ad)
    got = c.scene.render_adaptive(W, H, ad.min_spp, ad.max_spp, ad.tolerance, ad.floor, ad.check_every, seed=hsh.SEED, rr=hsh.RR, want_states=True)[:4]
    dev, _ = render_adaptive_device(c.scene, ad, rr=hsh.RR, seed=hsh.SEED)
    for form, planes in (("host", got), ("device", dev)):
        for g, w_, what in zip(planes, want, ("colours", "sample counts", "second moments", "final states")):
            same(g, w_, "%s adaptive %s, the %s form" % (name, what, form))
    x0, y0, x1, y1 = hsh.RECT
    inside = {k: v for k, v in chain.items() if x0 <= k[0] < x1 and y0 <= k[1] < y1}
    dev, _ = render_adaptive_device(c.scene, ad, rr=hsh.RR, seed=hsh.SEED, rect=hsh.RECT)
    for g, w_, what in zip(dev, rac.expected_from(inside, W, H, ad, guards=(-7.0, 0x5A5A5A5A, -7.0, 0x5A5A5A5A)), ("colours", "sample counts", "second moments", "final states")):
        same(g, w_, "%s adaptive %s, the device form on a rect" % (name, what))
    assert (sm.W, sm.H, sm.SEED, sm.RR, sm.RECT) == (W, H, hsh.SEED, hsh.RR, hsh.RECT)
    smap = np.asarray(got[1], "<u4")
    assert smap.max() > sm.CAP      # some counts are cut at the cap
    want = sm.expected_from(chain, smap, sm.CAP)
    host = c.scene.render_sample_map(W, H, smap, sm.CAP, hsh.SEED, True, True, rr=hsh.RR, out=sm.guards())[:3]
    dev, _ = sample_map_device(c, smap)
    for form, planes in (("host", host), ("device", dev)):
        for g, w_, what in zip(planes, want, ("colours", "second moments", "final states")):
            same(g, w_, "%s sample map %s, the %s form" % (name, what, form))


@pytest.mark.parametrize("which", PLANS)
# ---- light groups --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(hsh.N_LIGHTS) + hsh.ARRAYS)
def test_render_light_groups(case, knobs, frames, name, which):
    """one group per light and all lights in one: the group frames match the reference's dark twins, the unsplit frame its plain
    frame, the states its PIXEL final states.  In shapes_lights the sphere light of radius 0, the zero-axis cylinder light and
    the cylinder light of radius 0 give frames of +0 and still take their turn in the bounce's light pick -- the other groups'
    frames are the dark twins', whose light list keeps them.  The scene of arrays is held against the oracle's twins"""
    assert (lg.W, lg.H, lg.SEED, lg.RR) == (W, H, hsh.SEED, hsh.RR)
    knobs(VARIANTS[which][0])
    c = case(name)
    n = len(c.lights)
    if name in hsh.N_LIGHTS:
        own, states = frames[hsh.key(name, "pixel", 0, (W, H))], frames[hsh.key(name, "pixel", 0, (W, H)) + "__states"]
        twins = [frames[hsh.key("%s_dark%d" % (name, g), "pixel", 0, (W, H))] for g in range(n)]
        assert n == hsh.N_LIGHTS[name]
    else:
        own, states = hsh.pixel_planes(c)
        twins = [c.twin([m]).render(W, H, hsh.SPP, hsh.SEED, "pixel", rr=hsh.RR, threads=8)[0] for m in c.lights]
    if name == "shapes_lights":
        assert [bool(t.view("<u4").any()) for t in twins] == [True, False, False, True, False, True]
    for groups, G in ((c.per_light(), n), ({m: 0 for m in c.lights}, 1)):
        table = c.table(groups)
        out = [np.full((G, H, W, 3), lg.GUARD_F, "<f4"), np.full((H, W, 3), lg.GUARD_F, "<f4"), np.full((H, W), lg.GUARD_STATE, "<u4")]
        host = c.scene.render_light_groups(W, H, hsh.SPP, hsh.SEED, table, True, True, group_count=G, rr=hsh.RR, out=out)[:3]
        dev, _ = light_groups_device(c, groups, G, hsh.SPP)
        for form, (fr, rgb, st) in (("host", host), ("device", dev)):
            for g in range(G):
                same(fr[g], twins[g] if G == n else own, "%s light groups G = %d, group %d, the %s form" % (name, G, g, form))
            same(rgb, own, "%s light groups: the unsplit frame, the %s form" % (name, form))
            same(st, states, "%s light groups: final states, the %s form" % (name, form))


# ---- features ----------------------------------------------------------------------------------------------------------------------------------
class _Views:
    pass


@pytest.mark.parametrize("which", PLANS)
@pytest.mark.parametrize("name", ("shapes_seen", "shapes_leaves") + hsh.ARRAYS)
def test_render_features(api, oracle, case, knobs, name, which):
    """albedo, normal, depth, hits and ids of first hits on hostile shapes; ids of sample 0 names the shape -- ort_raycast's prim
    for that sample's ray, whose record check_records holds against the shape alone.  The single frame and a batch of views, host
    and device forms"""
    knobs(VARIANTS[which][0])
    c = case(name)
    cams = hsh.view_cameras(api, c)
    seeds = list(hsh.VIEW_SEEDS)
    planes = ("albedo", "normal", "depth", "hits", "ids", "states")
    wants = [hsh.feature_expected(c, cam, s) for cam, s in zip(cams, seeds)]
    prims = []
    for v, (_, f) in enumerate(wants):
        hits, _ = c.scene.raycast(f.rays[:, 0])
        assert_same_answers(hits["t"], hits["n"], hits["mat"], f.t[:, 0], f.nrm[:, 0], f.mat[:, 0], "%s, sample 0's rays of view %d" % (name, v))
        check_records(api, c.scene, c.flat, np.ascontiguousarray(f.rays[:, 0]), hits, "%s, sample 0's rays of view %d" % (name, v))
        prims.append(hits["prim"])
    if name != "arrays_shapes":
        assert hsh.hostile_hit(wants[0][1].mat[:, 0]).mean() >= 0.1
    got, _ = c.scene.render_features(W, H, hsh.FEATURE_SPP, hsh.SEED, want=planes)
    hsh.assert_features(got, wants[0][0], wants[0][1], prims[0], name + " features")
    got, _ = c.scene.render_views_features(cams, seeds, W, H, hsh.FEATURE_SPP, want=planes)
    w = _Views()
    w.scene, w.size, w.cams, w.seeds = c.scene, (W, H), cams, seeds
    dev, _ = features_device(api, w, hsh.FEATURE_SPP, True)
    for v in range(len(cams)):
        for form, p in (("host", got), ("device", dev)):
            hsh.assert_features({k: a[v] for k, a in p.items()}, wants[v][0], wants[v][1], prims[v], "%s features, view %d, the %s form" % (name, v, form))
    assert fc.SEED == hsh.SEED
    dev, _ = features_device(api, w, hsh.FEATURE_SPP, False)
    hsh.assert_features({k: a[0] for k, a in dev.items()}, wants[0][0], wants[0][1], prims[0], name + " features, the device form")


@pytest.mark.parametrize("which", ["default", "hbm_tables", "fallback", "counters"])
@pytest.mark.parametrize("name", hsh.FOLLOW_SCENES + ("shapes_seen@prologue24", "shapes_seen_specular@prologue24") + hsh.ARRAYS)
def test_render_follow(api, case, knobs, name, which):
    """ort_render_follow and ort_render_views_follow against follow_cases' chain, which tests/test_hostile_shapes_host.py pins
    against the oracle's diffuse twin on these frames: the single frame and the batch of hostile_shapes.view_cameras at (spp 5,
    rr 0.5, cap 64) and (rr 0.8, cap 2), all seven planes, ids' shapes through ort_raycast of the chains' last rays; the device
    forms under the default plan.  shapes_seen, shapes_leaves and the scene of arrays have no specular-only material: there the
    six planes are ort_render_views_features' and bounces is zero (identity 2).  Their SPECULAR twins make the hostile shapes
    that rays meet mirrors and glass, so the bounce rays start ON hostile shapes: 45 % of the own frame's samples are followed
    where the hostile sphere and boxes sit in the prologue (shapes_seen_specular; committed with a wider prologue, a hostile
    cylinder sits there too), 27 % where every hostile shape sits in a leaf (shapes_leaves_specular), paths 7 and 9 bounces deep
    (tests/test_hostile_shapes_host.py asserts the placement).  The far scenes follow 12 %"""
    env, counters = VARIANTS[which]
    name, _, commit = name.partition("@")
    c = case(name, "@" + commit if commit else "")
    follows = hsh.follow_conditions(api, c)
    assert follows == (name in hsh.FOLLOWING)
    w = hsh.follow_world(api, c)
    knobs(env)
    cast = lambda rays: c.scene.raycast(rays)[0]["prim"]
    last = {}

    def host(batch, rr, cap):
        last[batch], last["stats"] = follow_host(w, hsh.FEATURE_SPP, batch, rr=rr, cap=cap, counters=counters)
        return last[batch]
    fw.assert_renders(host, cast, w, hsh.FEATURE_SPP, hsh.FOLLOW_SETTINGS, "%s follow, %s" % (name, which))
    if counters:
        assert last["stats"]["rays"] == sum(k.rays for k in fw.chains(w, hsh.FEATURE_SPP, *hsh.FOLLOW_SETTINGS[-1])[1:])
    if not follows:
        first, _ = c.scene.render_views_features(w.fcams, w.fseeds, W, H, hsh.FEATURE_SPP, want=fc.PLANES)
        for k in fc.PLANES:
            same(last[True][k], first[k], "%s, %s: %s against ort_render_views_features" % (name, which, k))
        assert not last[True]["bounces"].any()
    if which == "default":
        device = lambda batch, rr, cap: follow_device(api, w, hsh.FEATURE_SPP, batch, rr=rr, cap=cap)[0]
        fw.assert_renders(device, cast, w, hsh.FEATURE_SPP, hsh.FOLLOW_SETTINGS, "%s follow, the device forms" % name)


# ---- the accumulating renders -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", PLANS + ["counters"])
@pytest.mark.parametrize("name", hsh.CHAINS + hsh.ARRAYS)
def test_render_accumulate(api, case, knobs, chain_file, name, which):
    """ort_render_accumulate: 64 samples as 1 + 3 + 12 + 48 against the fold of the REFERENCE's chains (the oracle's for the scene
    of arrays), every plane after every pass: a continued job reloads its sums and its state and walks on among the hostile shapes"""
    knobs(VARIANTS[which][0])
    c = case(name)
    chain = hsh.chains_from(chain_file, name) if name in hsh.CHAINS else hsh.chains_of(c)
    acs.reference_split(acs.library_call(api, c, counters=VARIANTS[which][1]), chain, "%s accumulate, %s" % (name, which), nan=name not in hsh.NO_NONFINITE)


@pytest.mark.parametrize("name", hsh.CHAINS)
def test_render_accumulate_device_forms_and_views(api, case, knobs, chain_file, name):
    """the 1 + 3 + 12 + 48 split through the _device forms on a non-default stream, guard words around every plane and no
    synchronisation between the passes, against the fold of the reference's chains; ort_render_views_accumulate on
    hostile_shapes.view_cameras in passes of 1 + 3 against the oracle's chains from each camera, frame 0 the single-frame form's"""
    knobs({})
    c = case(name)
    chain, nan = hsh.chains_from(chain_file, name), name not in hsh.NO_NONFINITE
    want = acs.Planes()
    for k in acs.REF_SPLIT:
        acs.model(want, 0, chain, None, k, None)
    acs.assert_planes(acs.stream_split(c, acs.REF_SPLIT), want, name + " accumulate, the device forms on a stream", nan=nan)
    call = acs.library_call(api, c)
    single = acs.Planes()
    for n in (1, 3):
        call(single, None, n)
    acs.views_split(call, c, hsh.view_cameras(api, c), hsh.VIEW_SEEDS, (1, 3), name + " accumulate, views", nan=nan, single=single)


@pytest.mark.parametrize("which", PLANS)
# ---- the ray and point queries ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("shapes_seen", "shapes_lights", "shapes_leaves") + hsh.ARRAYS)
def test_radiance_and_adaptive_radiance(case, knobs, name, which):
    """radiance_cases.mixed's 64 rays (8 outside the domain) and 16 aimed at the scene's first sphere (the one of radius -0.5 in
    shapes_seen and shapes_leaves), and adaptive_cases.cases_for's noisy rays: colours and states at 4 spp, and colours, states,
    spp and m2 under adaptive_cases.MAIN, against the oracle; host and device forms"""
    knobs(VARIANTS[which][0])
    c = case(name)
    cases = hm.ray_cases(c)
    exp, exp_ad, exp_noisy = hm.radiance_expected(c)
    rgb, fin, _ = c.scene.radiance(cases.rays, cases.seeds, hsh.QUERY_SPP, hsh.RR, want_states=True)
    rc.assert_same(rgb, fin, exp[0], exp[1], name + " radiance")
    rgb, fin, _ = torch_radiance(c.scene, cases.rays, cases.seeds, hsh.QUERY_SPP, hsh.RR)
    rc.assert_same(rgb, fin, exp[0], exp[1], name + " radiance, the device form")
    m = ac.MAIN
    for cs_, want, what in ((cases, exp_ad, ""), (hm.noisy_ray_cases(c), exp_noisy, ", the noisy rays")):
        got = c.scene.radiance_adaptive(cs_.rays, cs_.seeds, m.min_spp, m.max_spp, m.tolerance, m.floor, m.check_every, hsh.RR, want_states=True)[:4]
        ac.assert_same(got, want, name + " adaptive radiance" + what)
        ac.assert_same(adaptive_radiance_device(c.scene, cs_, m, hsh.RR)[0], want, name + " adaptive radiance, the device form" + what)


@pytest.mark.parametrize("which", PLANS)
def test_irradiance_and_adaptive_irradiance(case, knobs, hits_file, which):
    """the 192 points lifted off the hostile shapes of shapes_seen: identity I1 -- sample k is the radiance query (held above) at
    spp = 1 along the direction the oracle draws -- for 8 samples, and adaptive_cases.cut over 17 under irradiance_cases.EVERY;
    host and device forms"""
    knobs(VARIANTS[which][0])
    c = case("shapes_seen")
    p_, s_, _ = hsh.points_of(c, hits_file)
    pts = ic.Points(p_, s_, np.ones(len(p_), bool), np.zeros(len(p_), bool))
    one = lambda rays, seeds: c.scene.radiance(rays, seeds, 1, hsh.RR, want_states=True)[:2]
    chain = ic.chain_by_radiance(c.oracle, pts, 17, one)
    w_rgb, w_fin = ic.expected_from(chain, pts, 8)
    rgb, fin, _ = c.scene.irradiance(pts.points, pts.seeds, 8, hsh.RR, want_states=True)
    rc.assert_same(rgb, fin, w_rgb, w_fin, "irradiance")
    (rgb, _, _, fin), _ = torch_irradiance(c.scene, pts.points, pts.seeds, 8, hsh.RR)
    rc.assert_same(rgb, fin, w_rgb, w_fin, "irradiance, the device form")
    e = ic.EVERY
    want = ic.expected_adaptive(chain, pts, e)
    got = c.scene.irradiance_adaptive(pts.points, pts.seeds, e.min_spp, e.max_spp, e.tolerance, e.floor, e.check_every, hsh.RR, want_states=True)[:4]
    ac.assert_same(got, want, "adaptive irradiance")
    ac.assert_same(torch_irradiance(c.scene, pts.points, pts.seeds, 0, hsh.RR, ad=e)[0], want, "adaptive irradiance, the device form")
