"""The device on shapes that carry material 0, the no-hit material (tests/void_material.py).  Such a shape is real geometry that
every caller of the hit treats as a miss, and several kernels hold code for exactly that: the occlusion and ambient-occlusion
lanes switch their early end off (mats_nonzero), the shading step ends the path, the feature lane does not count the sample,
resolve_hit and the wavefront shade derive the material from the shape.  The host checks (tests/test_void_material_host.py: the
loader, the oracle and the host-compiled lane code on the same fixtures) cannot see what a GPU build makes of it.

Closest hits on void_seen are held against the REFERENCE'S OWN records (tests/golden/raycast_void.npz) and the renders of
void_hidden against its frames, states and chains (renders_void.npz, chains_void.npz; make_golden.py --only-void).  void_seen,
all_void and the scene of arrays have primary hits on void shapes, where the reference dereferences a null material: they are
held against the oracle, which the host tests hold against the reference wherever it can go.  Everything is bit for bit; no
pixel, ray or point is skipped.  Frames are 24 x 16 at 16 spp unless said otherwise."""
import numpy as np
import pytest

import accumulate_cases as acs
import adaptive_cases as ac
import ao_cases as ao
import feature_cases as fc
import follow_cases as fw
import hostile_materials as hm
import irradiance_cases as ic
import light_groups_cases as lg
import occluded_cases as oc
import radiance_cases as rc
import reference_goldens as rg
import render_adaptive_cases as rac
import sample_map_cases as sm
import void_material as vm
from raycast_cases import FLT_MAX, assert_same_answers
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

pytestmark = pytest.mark.gpu

W, H = vm.W, vm.H
POLICIES = (("pixel", 0), ("chunk", 4), ("whole", 0), ("tile32", 0))
# name -> (environment, counters)
VARIANTS = {
    "default": ({}, False),
    "hbm_tables": ({"ORT_LDS_TABLES": "0"}, False),
    "fallback": ({"ORT_DEBUG_FORCE_FALLBACK": "0xf"}, False),
    "exact": ({"ORT_DEBUG_FORCE_FALLBACK": "0"}, False),          # every ray on the exact walk: 24 x 16 x 4 spp, 2 000 rays
    "wide": ({"ORT_WIDE": "1"}, False),
    "wavefront": ({"ORT_MODE": "wavefront"}, False),
    "five": ({"ORT_EXCHANGE": "0", "ORT_WAVES5": "1"}, False),
    "exchange": ({"ORT_EXCHANGE": "1"}, False),
    "counters": ({}, True),
    "general": ({"ORT_KERNEL": "general"}, False),                # the all-lobes kernels on a scene that takes the DIFFUSE ones by itself
}
EVERYWHERE = [k for k in VARIANTS if k != "general"]
assert {k for env, _ in VARIANTS.values() for k in env} <= set(KNOBS)
EXACT_SPP = 4


@pytest.fixture(scope="module")
def frames():
    return rg.load("renders_void.npz")


@pytest.fixture(scope="module")
def chain_file():
    return rg.load("chains_void.npz")


@pytest.fixture(scope="module")
def hits_file():
    return rg.load("raycast_void.npz")


@pytest.fixture()
def case(api, oracle, manifest, tmp_path_factory):
    def get(name):
        if name in vm.ARRAYS:
            c = vm.arrays_case(api, oracle, name)
        else:
            c = vm.case(api, oracle, name, tmp_path_factory)
            assert rg.sha256(c.scn) == manifest["generated"]["void"]["scenes"][name]["scn_sha256"], name
        uploaded(api, c.scene)
        return c
    return get


# ---- closest hits ----------------------------------------------------------------------------------------------------------------------
def test_plain_closest_hits_on_void_seen(case, knobs, manifest, hits_file):
    """the narrowest case: the default plan, the host form, the reference's records.  The rays are regenerated (the manifest
    holds their SHA-256)"""
    knobs({})
    c = case("void_seen")
    rays, kind = vm.rays_of(c)
    assert vm.rays_sha256(rays) == manifest["generated"]["void"]["raycast"]["rays_sha256"]
    hits, _ = c.scene.raycast(rays)
    z = hits_file
    assert_same_answers(hits["t"], hits["n"], hits["mat"], z["t"], z["n"], z["mat"], "void_seen, the host form")


@pytest.mark.parametrize("which", EVERYWHERE)
def test_closest_hits(api, case, knobs, hits_file, which):
    """host and device forms against the reference's t, n and mat and against the oracle; every record's prim against the shape
    that its t and n belong to (test_gpu_raycast_edges.check_records: a hit names a shape, a void one too); against the `solid`
    twin t, n and prim are equal in every bit and mat is 0 exactly on the void shapes"""
    env, counters = VARIANTS[which]
    c, cs = case("void_seen"), case("void_seen_solid")
    rays, kind = vm.rays_of(c)
    z = hits_file
    sel = vm.exact_subset(kind) if which == "exact" else np.ones(len(rays), bool)
    r = rays[sel]
    knobs(env)
    hits, st = c.scene.raycast(r, counters=counters)
    for k, what in enumerate(vm.KINDS):
        s = kind[sel] == k
        assert_same_answers(hits["t"][s], hits["n"][s], hits["mat"][s], z["t"][sel][s], z["n"][sel][s], z["mat"][sel][s], "void_seen %s, %s rays" % (which, what))
    t, n, mat = c.twin(None).raycast(r[:, 0:3], r[:, 3:6])
    assert_same_answers(hits["t"], hits["n"], hits["mat"], t, n, mat, "void_seen %s against the oracle" % which)
    if counters:
        assert st["rays"] == len(r)
    if which in ("fallback", "exact"):
        assert st["fallback_rays"] > 0
    dh, _ = torch_raycast(c.scene, r, counters=counters)
    assert dh.tobytes() == hits.tobytes()
    missed = hits["t"].view("<u4") == FLT_MAX.view("<u4")
    void = ~missed & (hits["mat"] == 0)
    assert (hits["prim"][void] != api.NO_PRIM).all() and void.sum() >= 0.05 * len(r)
    finite = np.isfinite(r).all(axis=1) & ~np.isnan(hits["t"])
    check_records(api, c.scene, c.flat, r[finite], hits[finite], "void_seen " + which)
    solid, _ = cs.scene.raycast(r, counters=counters)
    for k in ("t", "n", "prim"):
        assert hits[k].tobytes() == solid[k].tobytes(), (k, which)
    assert ((hits["mat"] == 0) == (missed | (solid["mat"] == 1))).all()
    assert (hits["mat"][~void] == np.where(missed, 0, solid["mat"].astype(np.int64) - 1)[~void]).all()


@pytest.mark.parametrize("which", ["default", "hbm_tables", "fallback", "exact", "wide", "counters"])
@pytest.mark.parametrize("name", vm.ARRAYS)
def test_closest_hits_and_occlusion_on_the_scene_of_arrays(api, case, knobs, name, which):
    """void shapes in the middle and at the end of every array, a void mesh between two solid ones and the coincident pairs in
    both orders, asked directly: 256 rays at the pairs, 1 000 from inside the room and 500 aimed at the void shapes, against the
    oracle's t, n and mat, each record's prim against the shape it names; the occlusion ladder over the oracle's t; host and device
    forms.  Each pair's tie goes where the oracle's goes, and both outcomes occur for spheres and for boxes"""
    env, counters = VARIANTS[which]
    c = case(name)
    rays, kind = vm.arrays_rays(c)
    t, n, mat = c.twin(None).raycast(rays[:, 0:3], rays[:, 3:6])
    void = (t < FLT_MAX) & (mat == 0)
    assert 0.2 <= void[kind == 2].mean() <= 0.8 and void[kind == 1].any()
    for i, (shape, order) in enumerate((s, o) for s in ("spheres", "boxes") for o in (0, 1)):
        m = mat[i * vm.PAIR_RAYS:(i + 1) * vm.PAIR_RAYS]
        solid = vm.pair_rays(c, shape, order)[1]
        assert np.isin(m, (0, solid)).all() and (m == (0 if order == 0 else solid)).mean() >= 0.9, (shape, order)
    knobs(env)
    hits, st = c.scene.raycast(rays, counters=counters)
    assert_same_answers(hits["t"], hits["n"], hits["mat"], t, n, mat, "%s %s" % (name, which))
    if which in ("fallback", "exact"):
        assert st["fallback_rays"] > 0
    assert (hits["prim"][void] != api.NO_PRIM).all()
    check_records(api, c.scene, c.flat, rays, hits, "%s %s" % (name, which))
    assert torch_raycast(c.scene, rays, counters=counters)[0].tobytes() == hits.tobytes()
    rr, tm, want, _ = oc.laddered(rays, t, mat)
    assert want.mean() >= 0.1 and (~want).mean() >= 0.1
    got, _ = c.scene.occluded(rr, tm, counters=counters)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "%s %s: %d of %d bytes differ, first %d" % (name, which, len(bad), len(want), bad[0])
    assert (torch_occluded(c.scene, rr, tm, counters=counters)[0] == want).all()
    assert (c.scene.occluded(rays, None)[0] == (mat != 0)).all()


def test_conditions_on_the_rays(case, hits_file):
    """the shares that keep the closest-hit and occlusion tests from passing on an empty case, on the reference's records: of the
    aimed, surface and pair rays 20 % to 80 % have a void closest hit; at least 500 rays a void hit in front of a solid surface
    that the `removed` twin reports"""
    c = case("void_seen")
    rays, kind = vm.rays_of(c)
    t, mat = hits_file["t"], hits_file["mat"]
    void = (t < FLT_MAX) & (mat == 0)
    aimed = np.isin(kind, [vm.KINDS.index(k) for k in ("aimed", "surface", "pair")])
    assert 0.2 <= void[aimed].mean() <= 0.8
    hr, _ = case("void_seen_removed").scene.raycast(rays)
    assert int((void & (hr["mat"] != 0)).sum()) >= 500


# ---- occlusion -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", EVERYWHERE)
def test_occlusion(case, knobs, hits_file, which):
    """occluded_cases' ladder over the reference's t and, for every ray whose closest hit is void, three more rungs at prev, at and
    next of the `removed` twin's distance (byte 0 on all three: a solid surface behind a void shape, below tmax, does not
    occlude); tmax = None and the scalar +inf; host and device forms.  The same rays on the `solid` twin, where mats_nonzero is 1
    and the early end is taken, against its own expectation"""
    env, counters = VARIANTS[which]
    c, cs, cr = case("void_seen"), case("void_seen_solid"), case("void_seen_removed")
    rays, kind = vm.rays_of(c)
    t, mat = hits_file["t"], hits_file["mat"]
    sel = ~np.isnan(t) & (vm.exact_subset(kind) if which == "exact" else True)
    r, t, mat = rays[sel], t[sel], mat[sel]
    tr = cr.twin(None).raycast(r[:, 0:3], r[:, 3:6])[0]
    rr, tm, want = vm.occlusion_ladder(r, t, mat, tr)
    assert want.mean() >= 0.1 and (~want).mean() >= 0.1
    knobs(env)
    got, st = c.scene.occluded(rr, tm, counters=counters)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "%s, host form: %d of %d bytes differ, first %d (tmax %r)" % (which, len(bad), len(want), bad[0], tm[bad[0]])
    if counters:
        assert st["rays"] == len(rr)
    dg, _ = torch_occluded(c.scene, rr, tm, counters=counters)
    assert (dg == want).all(), which + ", device form"
    unlimited = (mat != 0) & (t < np.inf)
    assert 0.1 < unlimited.mean() < 0.9
    for limit in (None, np.float32(np.inf)):
        assert (c.scene.occluded(r, limit)[0] == unlimited).all(), (which, limit)
    assert (torch_occluded(c.scene, r, None)[0] == unlimited).all()
    ts, _, ms = cs.twin(None).raycast(r[:, 0:3], r[:, 3:6])
    rr, tm, want, _ = oc.laddered(r, ts, ms)
    got, _ = cs.scene.occluded(rr, tm, counters=counters)
    assert (got == want).all(), which + ", the solid twin"
    assert (torch_occluded(cs.scene, rr, tm)[0] == want).all(), which + ", the solid twin, device form"


# ---- ambient occlusion ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["default", "hbm_tables", "fallback", "exact", "counters"])
def test_ambient_occlusion(case, knobs, which):
    """the 256 points at ao_cases.radius_array's radii and without a radius: a sample whose closest hit is void is open and its
    direction enters the bent sum; host and device forms; and the `solid` twin"""
    env, counters = VARIANTS[which]
    pts = vm.points_of(case("void_seen"))
    for name in ("void_seen", "void_seen_solid"):
        c = case(name)
        w = vm.ao_world(c, pts)
        sampled = ((w.mat[:, :8] == 0) & (w.t[:, :8] < FLT_MAX)).any(axis=1).mean()
        assert (sampled >= 0.25) if name == "void_seen" else sampled == 0
        knobs(env)
        for radius in (w.radii, None):
            want = ao.expected(w, radius, 8)
            out, bent, fin, st = c.scene.ambient_occlusion(w.pts.points, w.pts.seeds, 8, radius=radius, want_bent=True, want_states=True, counters=counters)
            ao.assert_same((out, bent, fin), want, "%s AO %s" % (name, which))
            if counters:
                assert st["rays"] == 8 * len(w.pts.points)
            got, _ = ao_device(c.scene, w.pts.points, w.pts.seeds, radius, 8)
            ao.assert_same(got, want, "%s AO %s, the device form" % (name, which))


def test_conditions_on_the_points(case):
    """at least 10 % of the points differ from BOTH twins in the open count, and half of them stand within R of a void shape"""
    c = case("void_seen")
    pts = vm.points_of(c)
    w = vm.ao_world(c, pts)
    own = ao.expected(w, w.radii, 8)[0]
    differs = np.ones(len(own), bool)
    for t in vm.TWINS:
        differs &= ao.expected(vm.ao_world(case("void_seen_" + t), pts), w.radii, 8)[0] != own
    assert differs.mean() >= 0.1 and (vm.void_distance(c.flat, pts[0][:, 0:3]) < w.R).mean() >= 0.5


# ---- the plain renders ---------------------------------------------------------------------------------------------------------------------
def test_plain_pixel_render_of_void_hidden(case, knobs, frames):
    """the narrowest render: void_hidden, PIXEL, the default plan, the reference's frame"""
    knobs({})
    img, _ = case("void_hidden").scene.render(W, H, vm.SPP, vm.SEED, "pixel", rr=vm.RR)
    rg.assert_words_equal(img, frames[vm.key("void_hidden", "pixel", 0, (W, H))], "void_hidden PIXEL")


@pytest.mark.parametrize("which", EVERYWHERE)
def test_renders_of_void_hidden_match_reference(case, knobs, frames, oracle, which):
    """the four policies under every kernel the knobs reach; paths meet the void shapes at bounces only, which is the reference's
    own else branch.  Under ORT_DEBUG_FORCE_FALLBACK=0 (every ray on the exact walk) 4 spp, against the oracle"""
    env, counters = VARIANTS[which]
    c = case("void_hidden")
    knobs(env)
    for policy, chunk in POLICIES:
        if which == "exact":
            want, ost = c.twin(None).render(W, H, EXACT_SPP, vm.SEED, policy, chunk=max(chunk, 1), rr=vm.RR, threads=8)
            img, st = c.scene.render(W, H, EXACT_SPP, vm.SEED, policy, chunk=chunk, rr=vm.RR, counters=True)
            assert st["fallback_rays"] == st["rays"] > 0
        else:
            want = frames[vm.key("void_hidden", policy, chunk, (W, H))]
            img, st = c.scene.render(W, H, vm.SPP, vm.SEED, policy, chunk=chunk, rr=vm.RR, counters=counters)
        rg.assert_words_equal(img, want, "void_hidden %s, %s" % (policy, which))
        if counters:
            ost = c.twin(None).render(W, H, vm.SPP, vm.SEED, policy, chunk=max(chunk, 1), rr=vm.RR, threads=8)[1]
            assert (st["rays"], st["paths"]) == (ost["rays"], ost["paths"]), policy


@pytest.mark.parametrize("policy,chunk", POLICIES[:2])
def test_the_96_x_64_frames(case, knobs, frames, policy, chunk):
    """24 waves: void_hidden against the reference, void_seen against the oracle; in void_seen at least 10 % of the pixels have a
    void first hit for sample 0 and at least 10 % of the others differ from each twin (bounce hits on void shapes decide pixels);
    the same 10 % for void_hidden against its twins"""
    knobs({})
    c = case("void_hidden")
    img, _ = c.scene.render(vm.BIG[0], vm.BIG[1], vm.SPP, vm.SEED, policy, chunk=chunk, rr=vm.RR)
    rg.assert_words_equal(img, frames[vm.key("void_hidden", policy, chunk, vm.BIG)], "void_hidden %s 96 x 64" % policy)
    for name in vm.SCENES:
        c = case(name)
        own, _ = c.scene.render(vm.BIG[0], vm.BIG[1], vm.SPP, vm.SEED, policy, chunk=chunk, rr=vm.RR)
        rg.assert_words_equal(own, vm.oracle_frame(c, vm.BIG, policy, chunk), "%s %s 96 x 64" % (name, policy))
        f = vm.first_hits(c, vm.BIG)
        void = np.zeros(vm.BIG[::-1], bool)
        void[f.ys, f.xs] = f.mat[:, 0] == 0
        assert (void.mean() >= 0.1) if name == "void_seen" else not void.any()
        for t in vm.TWINS:
            twin, _ = case(name + "_" + t).scene.render(vm.BIG[0], vm.BIG[1], vm.SPP, vm.SEED, policy, chunk=chunk, rr=vm.RR)
            assert (twin.view("<u4") != own.view("<u4")).any(axis=2)[~void].mean() >= 0.1, (name, t)


@pytest.mark.parametrize("name,which", [(n, k) for n in ("void_seen", "all_void") + vm.ARRAYS for k in EVERYWHERE] + [("arrays_diffuse", "general")])
def test_renders_with_primary_void_hits(api, case, knobs, name, which):
    """void_seen, all_void and both flavours of the scene of arrays against the oracle: a path ends with no contribution where it
    meets a void shape, at the primary hit too, and the stream advances exactly as the oracle's does (CHUNK carries one stream
    across a chunk's samples).  PIXEL and CHUNK, a rect, the union of three shards, and the device form"""
    import torch
    env, counters = VARIANTS[which]
    c = case(name)
    spp = EXACT_SPP if which == "exact" else vm.SPP
    knobs(env)
    for policy, chunk in POLICIES[:2]:
        want = vm.oracle_frame(c, (W, H), policy, chunk, spp=spp)
        img, st = c.scene.render(W, H, spp, vm.SEED, policy, chunk=chunk, rr=vm.RR, counters=counters or which == "exact")
        rg.assert_words_equal(img, want, "%s %s, %s" % (name, policy, which))
        if which == "exact":
            assert st["fallback_rays"] == st["rays"] > 0      # the knob was read: every ray took the exact walk
        if name == "all_void":
            assert not img.view("<u4").any()
        if counters:
            osc = c.twin(None)
            ost = osc.render(W, H, spp, vm.SEED, policy, chunk=max(chunk, 1), rr=vm.RR, threads=8)[1]
            assert (st["rays"], st["paths"]) == (ost["rays"], ost["paths"]), policy
        if which != "default":
            continue
        got, _ = c.scene.render(W, H, spp, vm.SEED, policy, chunk=chunk, rect=vm.RECT, rr=vm.RR)
        x0, y0, x1, y1 = vm.RECT
        rg.assert_words_equal(got[y0:y1, x0:x1], vm.oracle_frame(c, (W, H), policy, chunk, rect=vm.RECT)[y0:y1, x0:x1], "%s %s, a rect" % (name, policy))
        union = np.zeros((H, W, 3), "<f4")
        for k in range(3):
            part, _ = c.scene.render(W, H, spp, vm.SEED, policy, chunk=chunk, rr=vm.RR, shard=(k, 3))
            assert not (union.view("<u4") != 0)[part.view("<u4") != 0].any()
            union = np.where(part.view("<u4") != 0, part, union)
        rg.assert_words_equal(union, want, "%s %s, the union of three shards" % (name, policy))
        d = torch.full((H, W, 3), -7.0, dtype=torch.float32, device="cuda")
        c.scene.render_device(d.data_ptr(), api.Scene.params(W, H, spp, vm.SEED, policy, chunk, None, vm.RR), want_stats=True)
        rg.assert_words_equal(d.cpu().numpy(), want, "%s %s, the device form" % (name, policy))


# ---- views -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy,chunk", POLICIES[:2])
@pytest.mark.parametrize("name", ("void_seen", "all_void") + vm.ARRAYS)
def test_render_views_one_inside_a_void_sphere(api, oracle, case, knobs, name, policy, chunk):
    """three views of void_seen, all_void and both scenes of arrays: the scene's own, light_groups_cases' second pose, and one
    standing inside the scene's first void sphere.  Its frame is all +0 -- every path ends on its primary hit -- and, under PIXEL,
    a pixel's final state is its seed advanced two steps per sample (the aperture draw alone), which the adaptive batch returns.
    In all_void that holds for all three views, and every plane of every call is +0 (spp: min_spp)"""
    import torch
    knobs({})
    c = case(name)
    cams = vm.view_cameras(api, c)
    f = vm.first_hits(c, (W, H), seed=vm.VIEW_SEEDS[2], cam=cams[2])
    assert (f.mat[:, 0] == 0).all() and (f.t[:, 0] < FLT_MAX).all()
    want = np.stack([vm.oracle_frame(c, (W, H), policy, chunk, cam=cam, seed=s) for cam, s in zip(cams, vm.VIEW_SEEDS)])
    assert not want[2].view("<u4").any() and bool(want[0].view("<u4").any()) == (name != "all_void")
    got, _ = c.scene.render_views(cams, list(vm.VIEW_SEEDS), W, H, vm.SPP, policy, chunk=chunk, rr=vm.RR)
    rg.assert_words_equal(got, want, "%s views %s" % (name, policy))
    d = torch.full((3, H, W, 3), -7.0, dtype=torch.float32, device="cuda")
    c.scene.render_views_device(d.data_ptr(), api.Scene.params(W, H, vm.SPP, 0, policy, chunk, None, vm.RR), cams, list(vm.VIEW_SEEDS), want_stats=True)
    rg.assert_words_equal(d.cpu().numpy(), want, "%s views %s, the device form" % (name, policy))
    if policy == "pixel":
        ad = hm.adaptive_set()
        rgb, spp, m2, fin = c.scene.render_views_adaptive(cams, list(vm.VIEW_SEEDS), W, H, ad.min_spp, ad.max_spp, ad.tolerance, ad.floor, ad.check_every,
                                                          rr=vm.RR, want_states=True)[:4]
        for v in ((0, 1, 2) if name == "all_void" else (2,)):
            assert not rgb[v].view("<u4").any() and not m2[v].view("<u4").any() and (spp[v] == ad.min_spp).all(), (name, v)
            states = np.array([vm.advance(oracle, oracle.job_seed(vm.VIEW_SEEDS[v], j), 2 * ad.min_spp) for j in range(W * H)], "<u4").reshape(H, W)
            rg.assert_words_equal(fin[v], states, "%s view %d, every first hit void: final states" % (name, v))
        if name != "all_void":      # the scene's own view is the single-frame call's, held against the chains below
            own = c.scene.render_adaptive(W, H, ad.min_spp, ad.max_spp, ad.tolerance, ad.floor, ad.check_every, seed=vm.VIEW_SEEDS[0], rr=vm.RR, want_states=True)[:4]
            for g, w_, what in zip((rgb[0], spp[0], m2[0], fin[0]), own, ("colours", "sample counts", "second moments", "final states")):
                rg.assert_words_equal(g, w_, "%s view 0 of the adaptive batch: %s" % (name, what))


# ---- the adaptive and the sample-map render ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vm.SCENES + ("all_void",) + vm.ARRAYS)
def test_render_adaptive_and_sample_map(case, knobs, chain_file, name):
    """all four planes of the adaptive render (min 16, max 64, a check every 16), on the reference's chains for void_hidden and
    the oracle's elsewhere; a zero-variance pixel -- every pixel of all_void, every pixel whose samples all end on a void shape
    -- stops at min_spp.  Then the sample-map render fed that call's counts.  Host and device forms, the device form on a rect"""
    knobs({})
    c = case(name)
    chain = vm.chains_from(chain_file, name) if name == "void_hidden" else vm.chains_of(c)
    ad = hm.adaptive_set()
    want = rac.expected_from(chain, W, H, ad)
    zero = ~np.asarray(want[0]).view("<u4").any(axis=2) & (want[2] == 0)
    assert zero.any() and (want[1][zero] == ad.min_spp).all() and (zero.all() == (name == "all_void"))
    got = c.scene.render_adaptive(W, H, ad.min_spp, ad.max_spp, ad.tolerance, ad.floor, ad.check_every, seed=vm.SEED, rr=vm.RR, want_states=True)[:4]
    dev, _ = render_adaptive_device(c.scene, ad, rr=vm.RR, seed=vm.SEED)
    for form, planes in (("host", got), ("device", dev)):
        for g, w_, what in zip(planes, want, ("colours", "sample counts", "second moments", "final states")):
            rg.assert_words_equal(g, w_, "%s adaptive %s, the %s form" % (name, what, form))
    x0, y0, x1, y1 = vm.RECT
    inside = {k: v for k, v in chain.items() if x0 <= k[0] < x1 and y0 <= k[1] < y1}
    dev, _ = render_adaptive_device(c.scene, ad, rr=vm.RR, seed=vm.SEED, rect=vm.RECT)
    for g, w_, what in zip(dev, rac.expected_from(inside, W, H, ad, guards=(-7.0, 0x5A5A5A5A, -7.0, 0x5A5A5A5A)), ("colours", "sample counts", "second moments", "final states")):
        rg.assert_words_equal(g, w_, "%s adaptive %s, the device form on a rect" % (name, what))
    assert (sm.W, sm.H, sm.SEED, sm.RR, sm.RECT) == (W, H, vm.SEED, vm.RR, vm.RECT)
    smap = np.asarray(got[1], "<u4")
    assert smap.max() > sm.CAP or name == "all_void"      # some counts are cut at the cap
    want = sm.expected_from(chain, smap, sm.CAP)
    host = c.scene.render_sample_map(W, H, smap, sm.CAP, vm.SEED, True, True, rr=vm.RR, out=sm.guards())[:3]
    dev, _ = sample_map_device(c, smap)
    for form, planes in (("host", host), ("device", dev)):
        for g, w_, what in zip(planes, want, ("colours", "second moments", "final states")):
            rg.assert_words_equal(g, w_, "%s sample map %s, the %s form" % (name, what, form))


# ---- light groups --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vm.SCENES + ("all_void",) + vm.ARRAYS)
def test_render_light_groups(case, knobs, frames, name):
    """one group per light and all lights in one: the group frames match the dark twins (the reference's files for void_hidden),
    the unsplit frame the plain render, the states the PIXEL jobs'.  group_of_material[0] holds a filler (0x5A, no group) that no
    lane may read: a void hit indexes nothing.  The light a void sphere encloses contributes a frame of +0 and still takes its turn
    in the bounce's light pick -- the other groups' frames are the dark twins', whose light list keeps it.  all_void has no light:
    one group that no material names, its frame and the unsplit frame +0, the states the PIXEL jobs'"""
    assert (lg.W, lg.H, lg.SEED, lg.RR) == (W, H, vm.SEED, vm.RR)
    knobs({})
    c = case(name)
    own, states = vm.pixel_planes(c)
    if name == "void_hidden":
        rg.assert_words_equal(own, frames[vm.key(name, "pixel", 0, (W, H))], "the oracle's own frame")
        twins = [frames[vm.key("void_hidden_dark%d" % g, "pixel", 0, (W, H))] for g in range(3)]
    else:
        twins = [c.twin([m]).render(W, H, vm.SPP, vm.SEED, "pixel", rr=vm.RR, threads=8)[0] for m in c.lights]
    n = len(c.lights)
    enclosed = {"void_seen": vm.ENCLOSED_LIGHT, "arrays_diffuse": 1, "arrays_all_lobes": 1}.get(name)
    for g in range(n):
        assert bool(twins[g].view("<u4").any()) == (g != enclosed), (name, g)
    for groups, G in (((c.per_light(), n), ({m: 0 for m in c.lights}, 1)) if n else (({}, 1),)):
        table = c.table(groups)
        assert table[0] == 0x5A
        out = [np.full((G, H, W, 3), lg.GUARD_F, "<f4"), np.full((H, W, 3), lg.GUARD_F, "<f4"), np.full((H, W), lg.GUARD_STATE, "<u4")]
        host = c.scene.render_light_groups(W, H, vm.SPP, vm.SEED, table, True, True, group_count=G, rr=vm.RR, out=out)[:3]
        dev, _ = light_groups_device(c, groups, G, vm.SPP)
        for form, (fr, rgb, st) in (("host", host), ("device", dev)):
            for g in range(G):
                rg.assert_words_equal(fr[g], twins[g] if G == n and n > 1 else own, "%s light groups G = %d, group %d, the %s form" % (name, G, g, form))
            rg.assert_words_equal(rgb, own, "%s light groups: the unsplit frame, the %s form" % (name, form))
            rg.assert_words_equal(st, states, "%s light groups: final states, the %s form" % (name, form))
    plain, _ = c.scene.render(W, H, vm.SPP, vm.SEED, "pixel", rr=vm.RR)
    rg.assert_words_equal(plain, own, name + ": the plain PIXEL render")
    assert bool(own.view("<u4").any()) == (name != "all_void")


# ---- features ----------------------------------------------------------------------------------------------------------------------------------
class _Views:
    pass


@pytest.mark.parametrize("name", ("void_seen", "all_void") + vm.ARRAYS)
def test_render_features(api, oracle, case, knobs, name):
    """a void first hit does not count in hits and adds nothing to albedo, normal or depth; ids of sample 0 holds material 0 with
    the shape's prim -- ort_raycast's for that sample's ray, which the tests above hold against the reference.  The single frame
    and a batch of views, host and device forms.  all_void: every plane asserted -- colours +0, hits 0, ids 0 with a prim.
    feature_cases' albedo twin leaves material 0 as it is (its white twin of all_void is +0)"""
    knobs({})
    c = case(name)
    if name == "all_void":
        img, _ = fc.twin_planes(fc.twin(oracle, c.flat, white=True), c.cam, W, H, vm.SEED, 4, with_states=False)
        assert not img.view("<u4").any()
    cams = vm.view_cameras(api, c) if name == "void_seen" else np.stack([c.cam, c.cam])
    seeds = list(vm.VIEW_SEEDS[:len(cams)])
    planes = ("albedo", "normal", "depth", "hits", "ids", "states")
    wants = [vm.feature_expected(c, cam, s) for cam, s in zip(cams, seeds)]
    prims = []
    for v, (_, f) in enumerate(wants):      # the closest-hit records behind ids: the oracle's t, n and mat, and the shape each names
        hits, _ = c.scene.raycast(f.rays[:, 0])
        assert_same_answers(hits["t"], hits["n"], hits["mat"], f.t[:, 0], f.nrm[:, 0], f.mat[:, 0], "%s, sample 0's rays of view %d" % (name, v))
        check_records(api, c.scene, c.flat, np.ascontiguousarray(f.rays[:, 0]), hits, "%s, sample 0's rays of view %d" % (name, v))
        prims.append(hits["prim"])
    got, _ = c.scene.render_features(W, H, vm.FEATURE_SPP, vm.SEED, want=planes)
    void = vm.assert_features(got, wants[0][0], wants[0][1], prims[0], name + " features")
    assert void >= (W * H if name == "all_void" else W * H // 10)
    if name == "all_void":
        for k in ("albedo", "normal", "depth", "hits"):
            assert not np.ascontiguousarray(got[k]).view("<u4").any(), k
        assert not got["ids"][..., 0].any() and (got["ids"][..., 1] != fc.NO_PRIM).all()
    else:
        assert ((wants[0][0]["hits"] > 0) & (wants[0][0]["hits"] < vm.FEATURE_SPP)).any()
    got, _ = c.scene.render_views_features(cams, seeds, W, H, vm.FEATURE_SPP, want=planes)
    w = _Views()
    w.scene, w.size, w.cams, w.seeds = c.scene, (W, H), cams, seeds
    dev, _ = features_device(api, w, vm.FEATURE_SPP, True)
    for v in range(len(cams)):
        for form, p in (("host", got), ("device", dev)):
            vm.assert_features({k: a[v] for k, a in p.items()}, wants[v][0], wants[v][1], prims[v], "%s features, view %d, the %s form" % (name, v, form))
    if name == "void_seen":
        assert not got["hits"][2].any() and (got["ids"][2][..., 1] != fc.NO_PRIM).all()   # inside the void sphere
    assert fc.SEED == vm.SEED
    dev, _ = features_device(api, w, vm.FEATURE_SPP, False)
    vm.assert_features({k: a[0] for k, a in dev.items()}, wants[0][0], wants[0][1], prims[0], name + " features, the device form")


@pytest.mark.parametrize("which", ["default", "hbm_tables", "fallback", "counters"])
@pytest.mark.parametrize("name", vm.SCENES + ("all_void",))
def test_render_follow(api, case, knobs, name, which):
    """ort_render_follow and ort_render_views_follow against follow_cases' chain, which tests/test_void_material_host.py pins
    against the oracle's diffuse twin on these very frames: the single frame and a batch of four views (one inside a void sphere,
    GLASS_CAM looking at void shapes through the glass sphere) at (spp 5, rr 0.5, cap 64) and (rr 0.8, cap 2), all seven planes.
    A camera ray or a bounce ray that ends on a void shape records nothing; as sample 0 it leaves ids {0, that shape} -- the shape
    ort_raycast names for the chain's last ray -- and NO_PRIM stays for a miss and for a sample 0 the roulette ended.  Under the
    default plan the device forms too.  all_void: every plane +0, hits 0, and the final states are ort_render_views_features'"""
    env, counters = VARIANTS[which]
    c = case(name)
    vm.follow_conditions(api, c)
    w = vm.follow_world(api, c)
    knobs(env)
    cast = lambda rays: c.scene.raycast(rays)[0]["prim"]
    last = {}

    def host(batch, rr, cap):
        last[batch], last["stats"] = follow_host(w, vm.FEATURE_SPP, batch, rr=rr, cap=cap, counters=counters)
        return last[batch]
    assert fw.assert_renders(host, cast, w, vm.FEATURE_SPP, vm.FOLLOW_SETTINGS, "%s follow, %s" % (name, which)) == 0
    if counters:
        assert last["stats"]["rays"] == sum(k.rays for k in fw.chains(w, vm.FEATURE_SPP, *vm.FOLLOW_SETTINGS[-1])[1:])
    if which == "fallback" and name != "all_void":
        assert follow_host(w, vm.FEATURE_SPP, True, counters=True)[1]["fallback_rays"] > 0
    if which == "default":
        device = lambda batch, rr, cap: follow_device(api, w, vm.FEATURE_SPP, batch, rr=rr, cap=cap)[0]
        fw.assert_renders(device, cast, w, vm.FEATURE_SPP, vm.FOLLOW_SETTINGS, "%s follow, the device forms" % name)
    if name == "all_void":
        got = last[True]
        for k in ("albedo", "normal", "depth", "hits", "bounces"):
            assert not np.ascontiguousarray(got[k]).view("<u4").any(), k
        assert not got["ids"][..., 0].any() and (got["ids"][..., 1] != fc.NO_PRIM).any()
        first, _ = c.scene.render_views_features(w.fcams, w.fseeds, W, H, vm.FEATURE_SPP, want=("hits", "states"))
        rg.assert_words_equal(got["states"], first["states"], "all_void: the final states are the first-hit render's")


# ---- the accumulating renders -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["default", "hbm_tables", "fallback", "counters"])
def test_render_accumulate(api, case, knobs, chain_file, which):
    """ort_render_accumulate.  void_hidden: 64 samples as 1 + 3 + 12 + 48 against the fold of the REFERENCE's chains
    (chains_void.npz: paths that meet void shapes at bounces).  void_seen: accumulate_cases.identity_2_per_pixel against the
    oracle's chains, and a pixel whose every camera sample ends on a void shape keeps sum, m2 and out_rgb at +0 while its count
    and state advance"""
    env, counters = VARIANTS[which]
    knobs(env)
    c = case("void_hidden")
    acs.reference_split(acs.library_call(api, c, counters=counters), vm.chains_from(chain_file, "void_hidden"), "void_hidden accumulate, " + which)
    c = case("void_seen")
    call = acs.library_call(api, c, counters=counters)
    acs.identity_2_per_pixel(call, c, "void_seen accumulate, " + which, chain=vm.chains_of(c))
    assert vm.accumulate_primary_void_pixels(call, c, "void_seen accumulate, " + which) >= 50


def test_render_accumulate_device_forms_and_views(api, case, knobs, chain_file):
    """void_hidden's 1 + 3 + 12 + 48 through the _device forms on a non-default stream, guard words around every plane and no
    synchronisation between the passes, against the fold of the reference's chains; ort_render_views_accumulate on void_seen's
    three views -- one inside a void sphere, whose frame stays +0 with its counts advanced -- in passes of 1 + 3 against the
    oracle's chains from each camera, frame 0 the single-frame form's"""
    knobs({})
    c = case("void_hidden")
    chain = vm.chains_from(chain_file, "void_hidden")
    want = acs.Planes()
    for k in acs.REF_SPLIT:
        acs.model(want, 0, chain, None, k, None)
    acs.assert_planes(acs.stream_split(c, acs.REF_SPLIT), want, "void_hidden accumulate, the device forms on a stream")
    c = case("void_seen")
    call = acs.library_call(api, c)
    single = acs.Planes()
    for n in (1, 3):
        call(single, None, n)
    got = acs.views_split(call, c, vm.view_cameras(api, c), vm.VIEW_SEEDS, (1, 3), "void_seen accumulate, views", single=single)
    assert not got.sum[2].view("<u4").any() and not got.m2[2].view("<u4").any() and (got.count[2] == 4).all()   # inside the void sphere


# ---- the ray and point queries ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("void_seen",) + vm.ARRAYS)
def test_radiance_and_adaptive_radiance(case, knobs, name):
    """radiance_cases.mixed's 64 rays (8 outside the domain) and 16 aimed at the scene's first sphere (void in void_seen), and
    adaptive_cases.cases_for's noisy rays: colours and states at 4 spp, and colours, states, spp and m2 under adaptive_cases.MAIN,
    against the oracle; host and device forms"""
    knobs({})
    c = case(name)
    cases = hm.ray_cases(c)
    exp, exp_ad, exp_noisy = hm.radiance_expected(c)
    rgb, fin, _ = c.scene.radiance(cases.rays, cases.seeds, vm.QUERY_SPP, vm.RR, want_states=True)
    rc.assert_same(rgb, fin, exp[0], exp[1], name + " radiance")
    rgb, fin, _ = torch_radiance(c.scene, cases.rays, cases.seeds, vm.QUERY_SPP, vm.RR)
    rc.assert_same(rgb, fin, exp[0], exp[1], name + " radiance, the device form")
    m = ac.MAIN
    for cs_, want, what in ((cases, exp_ad, ""), (hm.noisy_ray_cases(c), exp_noisy, ", the noisy rays")):
        got = c.scene.radiance_adaptive(cs_.rays, cs_.seeds, m.min_spp, m.max_spp, m.tolerance, m.floor, m.check_every, vm.RR, want_states=True)[:4]
        ac.assert_same(got, want, name + " adaptive radiance" + what)
        ac.assert_same(adaptive_radiance_device(c.scene, cs_, m, vm.RR)[0], want, name + " adaptive radiance, the device form" + what)


def test_irradiance_and_adaptive_irradiance(case, knobs):
    """the 256 points of void_seen: identity I1 -- sample k is the radiance query (held above) at spp = 1 along the direction the
    oracle draws -- for 8 samples, and adaptive_cases.cut over 17 under irradiance_cases.EVERY; host and device forms.  At least
    10 % of the points differ from both twins in the 8-sample colour"""
    knobs({})
    c = case("void_seen")
    p_, s_ = vm.points_of(c)
    pts = ic.Points(p_, s_, np.ones(len(p_), bool), np.zeros(len(p_), bool))
    one = lambda k: (lambda rays, seeds: k.scene.radiance(rays, seeds, 1, vm.RR, want_states=True)[:2])
    chain = ic.chain_by_radiance(c.oracle, pts, 17, one(c))
    w_rgb, w_fin = ic.expected_from(chain, pts, 8)
    rgb, fin, _ = c.scene.irradiance(pts.points, pts.seeds, 8, vm.RR, want_states=True)
    rc.assert_same(rgb, fin, w_rgb, w_fin, "irradiance")
    (rgb, _, _, fin), _ = torch_irradiance(c.scene, pts.points, pts.seeds, 8, vm.RR)
    rc.assert_same(rgb, fin, w_rgb, w_fin, "irradiance, the device form")
    e = ic.EVERY
    want = ic.expected_adaptive(chain, pts, e)
    got = c.scene.irradiance_adaptive(pts.points, pts.seeds, e.min_spp, e.max_spp, e.tolerance, e.floor, e.check_every, vm.RR, want_states=True)[:4]
    ac.assert_same(got, want, "adaptive irradiance")
    ac.assert_same(torch_irradiance(c.scene, pts.points, pts.seeds, 0, vm.RR, ad=e)[0], want, "adaptive irradiance, the device form")
    differs = np.ones(len(p_), bool)
    for t in vm.TWINS:
        ct = case("void_seen_" + t)
        other = ct.scene.irradiance(pts.points, pts.seeds, 8, vm.RR)[0]
        differs &= (other.view("<u4") != w_rgb.view("<u4")).any(axis=1)
    assert differs.mean() >= 0.1
