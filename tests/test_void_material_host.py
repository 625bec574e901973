"""Material 0 on shapes, on the CPU (tests/void_material.py): the loader, the oracle and the host-compiled lane code against the
REFERENCE'S OWN closest hits on void_seen and its frames, final states and chains of void_hidden (tests/golden/raycast_void.npz,
renders_void.npz, chains_void.npz; make_golden.py --only-void), and the conditions that keep the cases from being empty.  All of
this runs before anything goes to a GPU (tests/test_gpu_void_material.py): it is what lets the oracle stand in for the reference
where the reference cannot go -- a primary hit on a void shape dereferences a null material there -- and what says that a
divergence on the device is the device's.

Everything is bit for bit; no pixel, ray or point is skipped."""
import re

import numpy as np
import pytest

import accumulate_cases as acs
import adaptive_cases as ac
import ao_cases as ao
import feature_cases as fc
import follow_cases as fw
import host_sim_tool as hs
import hostile_materials as hm
import irradiance_cases as ic
import light_groups_cases as lg
import occluded_cases as oc
import radiance_cases as rc
import ref_io
import reference_goldens as rg
import render_adaptive_cases as rac
import sample_map_cases as sm
import void_material as vm
from raycast_cases import FLT_MAX, assert_same_answers

DIGEST_KEYS = ("counts", "camera_bits", "ambient_bits", "materials_sha256", "spheres_sha256", "boxes_sha256", "cylinders_sha256", "lights", "meshes")
POLICIES = (("pixel", 0), ("chunk", 4), ("whole", 0), ("tile32", 0))
W, H = vm.W, vm.H


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
        c = vm.case(api, oracle, name, tmp_path_factory)
        assert rg.sha256(c.scn) == manifest["generated"]["void"]["scenes"][name]["scn_sha256"], name
        return c
    return get


def _mats_nonzero(c):
    r = hs.run(hs.built("host_sim"), hs.render_args(c.base, c.scn, 8, 8, 1, 3, "pixel", 0, c.base)[0])
    return int(re.search(r"^shapes: mats_nonzero (\d)$", r.stderr, re.M).group(1))


# ---- the loader --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vm.STEMS)
def test_loader_gives_shapes_before_the_first_brdf_material_0(case, manifest, name):
    """every array has the reference loader's digest; the shapes written before the first `brdf` carry material 0 and are the
    first of their arrays; the light list is the reference's and lacks the void cylinder (a `solid` twin's has it); and
    all_mats_nonzero, as tools/host_sim prints it, is 0 exactly where a shape carries material 0"""
    c = case(name)
    meta = manifest["generated"]["void"]["scenes"][name]
    dg = ref_io.scene_digest(c.flat)
    for k in DIGEST_KEYS:
        assert dg[k] == meta[k], (name, k)
    f = c.flat
    mats = {"sphere": f.spheres["mat"], "box": f.boxes["mat"], "cylinder": f.cylinders["mat"], "mesh": np.array([m["mat"] for m in f.meshes], "<u4")}
    base = name.split("_")[0] + "_" + name.split("_")[1]
    lights = [[int(t), int(i)] for t, i in zip(f.lights["type"], f.lights["index"])]
    if name == "all_void":
        assert len(f.materials) == 1 and len(f.lights) == 0 and all((m == 0).all() and len(m) for m in mats.values())
    elif name.endswith("_removed"):
        assert all((m != 0).all() for m in mats.values()) and lights == [[1, 3], [1, 4], [2, 0]]
    else:
        n = vm.void_counts(base)
        want = 1 if name.endswith("_solid") else 0
        for k, m in mats.items():
            assert (m[:n[k]] == want).all() and (m[n[k]:] > want).all(), (name, k)
        # in file order; spheres 6 and 7 are the two light spheres, cylinder 1 the light cylinder, cylinder 0 the void one
        assert lights == ([[2, 0], [1, 6], [1, 7], [2, 1]] if want else [[1, 6], [1, 7], [2, 1]])
    assert _mats_nonzero(c) == (0 if name == "all_void" or not name.endswith(("_solid", "_removed")) else 1)


def test_the_coincident_spheres_are_bit_identical(case):
    s = case("void_seen").flat.spheres
    assert s[1]["mat"] == 0 and s[4]["mat"] != 0
    assert s[1]["center"].tobytes() == s[4]["center"].tobytes() and s[1]["r"].tobytes() == s[4]["r"].tobytes()
    assert s[2]["mat"] == 0 and s[7]["mat"] != 0 and s[2]["center"].tobytes() == s[7]["center"].tobytes() and s[2]["r"] > s[7]["r"]   # encloses the second light


# ---- the oracle against the reference ------------------------------------------------------------------------------------------------
def test_oracle_closest_hits_match_reference(case, manifest, hits_file):
    """void_material.ray_sets placed by the oracle's casts are the bytes the reference's casts placed (the manifest's SHA-256), and
    t, n and mat of all 8 512 rays are the reference's raycast_top_most_node: a void shape's t and n with mat 0, the tie of the
    coincident spheres to the void one (first in the file)"""
    c = case("void_seen")
    rays, kind = vm.rays_of(c)
    meta = manifest["generated"]["void"]["raycast"]
    assert vm.rays_sha256(rays) == meta["rays_sha256"] and len(rays) == meta["count"] and (kind == hits_file["kind"]).all()
    t, n, mat = c.twin(None).raycast(rays[:, 0:3], rays[:, 3:6])
    for k, what in enumerate(vm.KINDS):
        s = kind == k
        assert_same_answers(t[s], n[s], mat[s], hits_file["t"][s], hits_file["n"][s], hits_file["mat"][s], "oracle, %s rays" % what)


def test_the_surface_rays_start_on_void_shapes(case, hits_file):
    """all 500 `surface` rays start at o + t d of a ray whose closest hit -- the oracle's and, through the manifest's SHA-256 of the
    rays, the reference's -- carries material 0, and that point lies on a void shape's bounding box to within rounding"""
    c = case("void_seen")
    rays, kind = vm.rays_of(c)
    parents, t, mat = vm.surface_parents(c)
    assert len(parents) == vm.N_SURFACE and (mat == 0).all() and (t < FLT_MAX).all()
    start = rays[kind == vm.KINDS.index("surface"), 0:3]
    assert start.tobytes() == (parents[:, 0:3] + t[:, None] * parents[:, 3:6]).astype("<f4").tobytes()
    assert (vm.void_distance(c.flat, start) < 1e-4).all()
    only = c.oracle.OracleScene(api_scene(c, vm.void_only_text()).flatten(W, H))
    tv, _, mv = only.raycast(parents[:, 0:3], parents[:, 3:6])
    assert (mv != 0).all() and tv.tobytes() == t.tobytes()      # the void shapes alone give the same distance


def api_scene(c, text):
    from offline_raytracer_amd import api
    return api.Scene.parse_scn(text, c.base).commit()


def test_oracle_renders_and_chains_match_reference(api, oracle, case, manifest, frames, chain_file):
    """every frame of renders_void.npz -- void_hidden in four policies at 24 x 16 with the PIXEL final states, PIXEL and CHUNK at
    96 x 64, the three dark twins -- with counters and final RNG, and the 64-sample chains"""
    meta = manifest["generated"]["void"]["renders"]
    assert sorted(meta) == sorted(vm.key(s, p, ch, size) for s, p, ch, size, _ in vm.RENDERS)
    for scene, policy, chunk, (w, h), states in vm.RENDERS:
        key = vm.key(scene, policy, chunk, (w, h))
        osc = oracle.OracleScene(case(scene).scene.flatten(w, h))
        if states:
            img, st, fin = rg.oracle_pixel_planes(oracle, osc, w, h, vm.SPP, vm.SEED, vm.RR)
            rg.assert_words_equal(fin, frames[key + "__states"], key + ": final states")
        else:
            img, st = osc.render(w, h, vm.SPP, vm.SEED, policy, chunk=max(chunk, 1), rr=vm.RR, threads=1)
        rg.assert_words_equal(img, frames[key], key)
        assert st["shapes_tested"] == meta[key]["shapes_tested"], key
        if policy != "tile32":
            assert st["final_rng"] == meta[key]["final_rng"], key
    c = case("void_hidden")
    for g, m in enumerate(c.lights):
        img, _ = c.twin([m]).render(W, H, vm.SPP, vm.SEED, "pixel", rr=vm.RR, threads=1)
        rg.assert_words_equal(img, frames[vm.key("void_hidden_dark%d" % g, "pixel", 0, (W, H))], "dark twin %d, the patched arrays" % g)
    got = vm.chains_of(c)
    rg.assert_words_equal(np.stack([got[(x, y)][0] for y in range(H) for x in range(W)]).reshape(H, W, vm.CHAIN_SAMPLES, 3),
                          chain_file["void_hidden__colours"], "chain colours")
    rg.assert_words_equal(np.stack([got[(x, y)][1] for y in range(H) for x in range(W)]).reshape(H, W, vm.CHAIN_SAMPLES),
                          chain_file["void_hidden__states"], "chain states")


def test_the_albedo_twin_leaves_material_0_alone(oracle, case):
    """feature_cases.twin turns every material m >= 1 into a light; were material 0 one too, all_void's white twin would shine"""
    c = case("all_void")
    img, _ = fc.twin_planes(fc.twin(oracle, c.flat, white=True), c.cam, W, H, vm.SEED, 4, with_states=False)
    assert not img.view("<u4").any()
    c = case("void_seen")
    f = vm.first_hits(c, (W, H))
    img, _ = fc.twin_planes(fc.twin(oracle, c.flat, white=True), c.cam, W, H, vm.SEED, 1, with_states=False)
    void = np.zeros((H, W), bool)
    void[f.ys, f.xs] = f.mat[:, 0] == 0
    assert void.any() and not img[void].view("<u4").any() and (img[~void] == 1).all()


# ---- the conditions: no case is empty -------------------------------------------------------------------------------------------------
def test_conditions_on_the_rays_and_limits(api, oracle, case, hits_file, tmp_path):
    """measured (printed): of the aimed, surface and pair rays 75.8 % have a void closest hit (20 % to 80 %); 2 576 rays have a
    void hit in front of a solid surface that the `removed` twin reports (500); 246 a solid hit with a void shape behind it
    (200); of the ladder's 109 872 bytes 18.8 % are 1 (10 % each way)"""
    c = case("void_seen")
    rays, kind = vm.rays_of(c)
    t, mat = hits_file["t"], hits_file["mat"]
    hit = t < FLT_MAX
    void = hit & (mat == 0)
    aimed = np.isin(kind, [vm.KINDS.index(k) for k in ("aimed", "surface", "pair")])
    tr, _, mr = case("void_seen_removed").twin(None).raycast(rays[:, 0:3], rays[:, 3:6])
    in_front = int((void & (mr != 0)).sum())
    only = oracle.OracleScene(api.Scene.parse_scn(vm.void_only_text(), c.base).commit().flatten(W, H))
    with np.errstate(all="ignore"):
        tv, _, mv = only.raycast(rays[:, 0:3], rays[:, 3:6])
        behind = int((hit & (mat != 0) & (mv != 0) & (tv > t)).sum())
    _, _, want = vm.occlusion_ladder(rays, t, mat, tr)
    print("void share of the aimed rays %.3f; void in front of solid %d; solid in front of void %d; ladder: %d bytes, %.3f ones"
          % (void[aimed].mean(), in_front, behind, len(want), want.mean()))
    assert 0.2 <= void[aimed].mean() <= 0.8
    assert in_front >= 500 and behind >= 200
    assert want.mean() >= 0.1 and (~want).mean() >= 0.1


def test_conditions_on_the_frames(case):
    """96 x 64, 16 spp, measured (printed): void_seen has a void first hit for sample 0 on 54.4 % of the pixels; of the others
    86.1 % differ from the `solid` twin and 53.3 % from the `removed` one (bounce hits on void shapes decide pixels); void_hidden
    has none, and 74.6 % and 35.2 % of its pixels differ.  Floors: 10 % each"""
    for name in vm.SCENES:
        c = case(name)
        f = vm.first_hits(c, vm.BIG)
        assert (f.t[:, 0] < FLT_MAX).all()
        void = np.zeros(vm.BIG[::-1], bool)
        void[f.ys, f.xs] = f.mat[:, 0] == 0
        own = vm.oracle_frame(c, vm.BIG, "pixel", 0)
        shares = [((vm.oracle_frame(case(name + "_" + t), vm.BIG, "pixel", 0).view("<u4") != own.view("<u4")).any(axis=2))[~void].mean() for t in vm.TWINS]
        print("%s: void first hits %.3f; other pixels that differ from solid %.3f, from removed %.3f" % (name, void.mean(), shares[0], shares[1]))
        assert (void.mean() >= 0.1) if name == "void_seen" else not void.any()
        assert min(shares) >= 0.1


def test_conditions_on_the_points(case, tmp_path):
    """the 256 points: measured (printed) shares that differ from BOTH twins in the open count at ao_cases' radii and in the
    8-sample irradiance colour; floor 10 %"""
    c = case("void_seen")
    pts = vm.points_of(c)
    worlds = {t: vm.ao_world(case("void_seen" + ("_" + t if t else "")), pts) for t in (None,) + vm.TWINS}
    own = ao.expected(worlds[None], worlds[None].radii, 8)[0]
    differs = np.ones(len(own), bool)
    for t in vm.TWINS:
        differs &= ao.expected(worlds[t], worlds[None].radii, 8)[0] != own
    w = worlds[None]
    near = vm.void_distance(c.flat, pts[0][:, 0:3]) < w.R          # R = 0.1 x the diagonal, the radius most points get
    sampled = ((w.mat[:, :8] == 0) & (w.t[:, :8] < FLT_MAX)).any(axis=1)
    print("open counts differ from both twins on %.3f of the points; a void shape within R of %.3f; one of 8 samples meets a void shape on %.3f"
          % (differs.mean(), near.mean(), sampled.mean()))
    assert differs.mean() >= 0.1 and near.mean() >= 0.5 and sampled.mean() >= 0.25
    cols = {}
    for t in (None,) + vm.TWINS:
        ct = case("void_seen" + ("_" + t if t else ""))
        p = ic.Points(pts[0], pts[1], np.ones(len(pts[0]), bool), np.zeros(len(pts[0]), bool))
        cols[t] = ic.expected_from(ic.chain_by_radiance(ct.oracle, p, 8, _one(ct, tmp_path)), p, 8)[0]
    d = np.ones(len(pts[0]), bool)
    for t in vm.TWINS:
        d &= (cols[t].view("<u4") != cols[None].view("<u4")).any(axis=1)
    print("irradiance colours differ from both twins on %.3f of the points" % d.mean())
    assert d.mean() >= 0.1


def _one(c, d):
    """identity I1's radiance call: tools/host_sim --radiance at one sample, which test_lanes_radiance_and_irradiance holds against
    the oracle on this scene"""
    return lambda rays, seeds: hs.radiance(hs.built("host_sim"), d, c.scn, rays, seeds, 1, vm.RR, c.base, threads=4)


# ---- the lane code on the host -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["host_sim", "host_sim_w5"])
def tool(request):
    return hs.built(request.param)


QUERY_SETS = ({}, {"SIM_TABS": "1"}, {"SIM_FORCE_FALLBACK": "0xf"}, {"SIM_WIDE": "1"})


def test_lanes_closest_hits(tool, case, hits_file, tmp_path):
    """--raycast on void_seen against the reference's records: the default walk, the tables image, the forced fallback and the wide
    tree on all rays, the exact walk for every ray (SIM_FORCE_FALLBACK=0) on void_material.exact_subset's 2 000.  A void hit names its shape;
    against the `solid` twin t, n and prim are equal in every bit and mat is 0 exactly on the void shapes"""
    c, cs = case("void_seen"), case("void_seen_solid")
    rays, kind = vm.rays_of(c)
    z = hits_file
    for e in QUERY_SETS + ({"SIM_FORCE_FALLBACK": "0"},):
        sel = vm.exact_subset(kind) if e.get("SIM_FORCE_FALLBACK") == "0" else np.ones(len(rays), bool)
        hits, _ = hs.raycast(tool, tmp_path, c.scn, rays[sel], c.base, env=e, threads=4)
        assert_same_answers(hits["t"], hits["n"], hits["mat"], z["t"][sel], z["n"][sel], z["mat"][sel], "void_seen %r" % (e,))
        missed = hits["t"].view("<u4") == FLT_MAX.view("<u4")
        assert ((hits["prim"] == hs.NO_PRIM) == missed).all(), e
        void = ~missed & (hits["mat"] == 0)
        assert void.sum() >= 0.2 * sel.sum()
        solid, _ = hs.raycast(tool, tmp_path, cs.scn, rays[sel], cs.base, env=e, threads=4)
        for k in ("t", "n", "prim"):
            assert hits[k].tobytes() == solid[k].tobytes(), (k, e)
        assert ((hits["mat"] == 0) == (missed | (solid["mat"] == 1))).all() and (hits["mat"][~void] == np.where(missed, 0, solid["mat"] - 1)[~void]).all()


def test_lanes_occlusion(tool, case, hits_file, tmp_path):
    """--occluded: occluded_cases' ladder over the reference's t with three more rungs at the `removed` twin's distance for every
    void hit (byte 0 on all three: a solid surface behind a void shape below tmax does not occlude), without limits (tmax NULL),
    and the same rays on the `solid` twin, whose early end is taken, against its own expectation"""
    c, cs = case("void_seen"), case("void_seen_solid")
    rays, kind = vm.rays_of(c)
    t, mat = hits_file["t"], hits_file["mat"]
    finite = ~np.isnan(t)
    tr = case("void_seen_removed").twin(None).raycast(rays[:, 0:3], rays[:, 3:6])[0]
    rr, tm, want = vm.occlusion_ladder(rays[finite], t[finite], mat[finite], tr[finite])
    assert want.mean() >= 0.1 and (~want).mean() >= 0.1
    few = vm.exact_subset(kind)[finite]
    for e in QUERY_SETS + ({"SIM_FORCE_FALLBACK": "0"},):
        if e.get("SIM_FORCE_FALLBACK") == "0":
            rr_, tm_, want_ = vm.occlusion_ladder(rays[finite][few], t[finite][few], mat[finite][few], tr[finite][few])
            assert want_.mean() >= 0.1 and (~want_).mean() >= 0.1
        else:
            rr_, tm_, want_ = rr, tm, want
        got = hs.occluded(tool, tmp_path, c.scn, rr_, tm_, c.base, env=e, threads=4)
        bad = np.flatnonzero(got != want_.astype(np.uint8))
        assert len(bad) == 0, "%r: %d of %d bytes differ, first %d" % (e, len(bad), len(want_), bad[0])
    got = hs.occluded(tool, tmp_path, c.scn, rays, None, c.base, threads=4)
    assert (got == ((mat != 0) & (t < np.inf)).astype(np.uint8)).all() and 0.1 < got.mean() < 0.9
    ts, _, ms = cs.twin(None).raycast(rays[:, 0:3], rays[:, 3:6])
    assert (ms[finite] != 0).sum() > (mat[finite] != 0).sum()
    rr, tm, want, _ = oc.laddered(rays[finite], ts[finite], ms[finite])
    got = hs.occluded(tool, tmp_path, cs.scn, rr, tm, cs.base, threads=4)
    assert (got == want.astype(np.uint8)).all()


def test_lanes_ambient_occlusion(tool, case, tmp_path):
    """--ambient-occlusion on the 256 points: a sample whose closest hit is void is open and its direction enters the bent sum;
    ao_cases.radius_array's radii, no radius, and the `solid` twin"""
    pts = vm.points_of(case("void_seen"))
    for name in ("void_seen", "void_seen_solid"):
        c = case(name)
        w = vm.ao_world(c, pts)
        void_open = ((w.mat[:, :8] == 0) & (w.t[:, :8] < FLT_MAX)).any(axis=1).mean()
        assert (void_open >= 0.25) if name == "void_seen" else void_open == 0
        for e in ({}, {"SIM_TABS": "1"}, {"SIM_FORCE_FALLBACK": "0xf"}):
            for radius in (w.radii, None):
                got = ao.host_sim(tool, tmp_path, c.scn, w.pts.points, w.pts.seeds, radius, 8, base=c.base, env=e, threads=4)[:3]
                ao.assert_same(got, ao.expected(w, radius, 8), "%s AO %r" % (name, e))


RENDER_SETS = ({}, {"SIM_TABS": "1"}, {"SIM_FORCE_FALLBACK": "0xf"})


def test_lanes_render_the_references_frames_of_void_hidden(tool, case, frames, tmp_path):
    """the four policies, also through the tables image, the forced fallback, the wide tree and the wavefront trace; 96 x 64"""
    c = case("void_hidden")
    for policy, chunk in POLICIES:
        key = vm.key("void_hidden", policy, chunk, (W, H))
        for e in RENDER_SETS + (({"SIM_WIDE": "1"}, {"SIM_WAVEFRONT": "100"}) if policy == "chunk" else ()):
            img = hs.render(tool, tmp_path, c.scn, W, H, vm.SPP, vm.SEED, policy, chunk, c.base, env=e, threads=1 if "SIM_WAVEFRONT" in e else 2)
            rg.assert_words_equal(img, frames[key], "void_hidden %s %r" % (policy, e))
    for policy, chunk in POLICIES[:2]:
        img = hs.render(tool, tmp_path, c.scn, vm.BIG[0], vm.BIG[1], vm.SPP, vm.SEED, policy, chunk, c.base, threads=4)
        rg.assert_words_equal(img, frames[vm.key("void_hidden", policy, chunk, vm.BIG)], "void_hidden %s 96 x 64" % policy)


@pytest.mark.parametrize("name", ("void_seen", "void_hidden", "all_void"))
def test_lanes_render_with_every_ray_on_the_exact_walk(tool, case, tmp_path, name):
    """SIM_FORCE_FALLBACK=0: every ray of the render is re-cast by the exact walk, whose resolve_hit derives the material from the
    shape; 24 x 16 at 4 spp, PIXEL and CHUNK, against the oracle"""
    c = case(name)
    for policy, chunk in POLICIES[:2]:
        want = vm.oracle_frame(c, (W, H), policy, chunk, spp=4)
        img = hs.render(tool, tmp_path, c.scn, W, H, 4, vm.SEED, policy, chunk, c.base, env={"SIM_FORCE_FALLBACK": "0"}, threads=4)
        rg.assert_words_equal(img, want, "%s %s, the exact walk" % (name, policy))


@pytest.mark.parametrize("name", ("void_seen", "all_void"))
def test_lanes_render_primary_void_hits(tool, case, tmp_path, name):
    """void_seen and all_void against the oracle: a path ends with no contribution at a void shape, at the primary hit too, and
    the stream advances as the oracle's does (CHUNK and WHOLE carry one stream across pixels).  all_void: every word +0"""
    c = case(name)
    for policy, chunk in POLICIES:
        want = vm.oracle_frame(c, (W, H), policy, chunk)
        for e in RENDER_SETS + (({"SIM_WIDE": "1"}, {"SIM_WAVEFRONT": "100"}) if policy == "chunk" else ()):
            img = hs.render(tool, tmp_path, c.scn, W, H, vm.SPP, vm.SEED, policy, chunk, c.base, env=e, threads=1 if "SIM_WAVEFRONT" in e else 2)
            rg.assert_words_equal(img, want, "%s %s %r" % (name, policy, e))
        if name == "all_void":
            assert not want.view("<u4").any()
    if name == "void_seen":
        for policy, chunk in POLICIES[:2]:
            img = hs.render(tool, tmp_path, c.scn, vm.BIG[0], vm.BIG[1], vm.SPP, vm.SEED, policy, chunk, c.base, threads=4)
            rg.assert_words_equal(img, vm.oracle_frame(c, vm.BIG, policy, chunk), "void_seen %s 96 x 64" % policy)


def _views_expected(api, oracle, c):
    """-> (cameras, the oracle's PIXEL frames of the three views, the final state of every pixel of the view inside the void sphere)"""
    cams = vm.view_cameras(api, c)
    want = np.stack([vm.oracle_frame(c, (W, H), "pixel", 0, cam=cam, seed=s) for cam, s in zip(cams, vm.VIEW_SEEDS)])
    f = vm.first_hits(c, (W, H), seed=vm.VIEW_SEEDS[2], cam=cams[2])
    assert (f.mat[:, 0] == 0).all() and (f.t[:, 0] < FLT_MAX).all() and not want[2].view("<u4").any()
    return cams, want


@pytest.mark.parametrize("name", vm.SCENES + ("all_void",))
def test_lanes_views_adaptive_groups_and_sample_map(api, oracle, tool, case, frames, chain_file, tmp_path, name):
    """--views (the third view stands inside a void sphere: its frame is +0), --render-adaptive and --sample-map on the
    reference's chains (void_hidden) or the oracle's, --light-groups against the dark twins: the light a void sphere encloses
    gives a frame of +0 in void_seen, and group_of_material[0] holds a filler no lane may read.  all_void takes every call too:
    three views of +0, and the light-group call with one group that nothing names"""
    c = case(name)
    cams, want = (hm.view_cameras(api, c), None) if name == "void_hidden" else _views_expected(api, oracle, c)
    if want is None:
        want = np.stack([vm.oracle_frame(c, (W, H), "pixel", 0, cam=cam, seed=s) for cam, s in zip(cams, vm.VIEW_SEEDS)])
    got = hs.views(tool, tmp_path, c.scn, cams, vm.VIEW_SEEDS, W, H, vm.SPP, "pixel", 0, c.base, threads=2)
    rg.assert_words_equal(got, want, name + " views")
    assert bool(want.view("<u4").any()) == (name != "all_void")
    chain = vm.chains_from(chain_file, name) if name == "void_hidden" else vm.chains_of(c)
    ad = hm.adaptive_set()
    got = rac.host_sim(tool, tmp_path, c.scn, W, H, None, vm.SEED, ad, vm.RR, c.base, threads=2)
    want = rac.expected_from(chain, W, H, ad)
    for g, w_, what in zip(got, want, ("colours", "sample counts", "second moments", "final states")):
        rg.assert_words_equal(g, w_, "%s adaptive %s" % (name, what))
    zero = ~np.asarray(want[0]).view("<u4").any(axis=2) & (want[2] == 0)
    assert (want[1][zero] == ad.min_spp).all() and zero.any()        # a zero-variance pixel stops at min_spp
    smap = np.minimum(want[1], sm.CAP).astype("<u4")                 # the sample map fed the adaptive call's counts
    (rgb, m2, fin), _ = sm.host_sample_map(tool, tmp_path, c, smap, sm.CAP, vm.SEED, threads=2)
    for g, w_, what in zip((rgb[0], m2[0], fin[0]), sm.expected_from(chain, smap, sm.CAP), ("colours", "second moments", "final states")):
        rg.assert_words_equal(g, w_, "%s sample map %s" % (name, what))
    own, states = vm.pixel_planes(c)
    # all_void has no light: one group that no material names, its frame and the unsplit frame +0, the states the PIXEL jobs'
    for groups, G in (((c.per_light(), 3), ({m: 0 for m in c.lights}, 1)) if name != "all_void" else (({}, 1),)):
        table = c.table(groups)
        assert table[0] == 0x5A
        fr, rgb, st = lg.host_light_groups(tool, tmp_path, c, table, G, vm.SPP, vm.SEED, threads=2)
        for g in range(G):
            if G == 1:
                want_g = own
            elif name == "void_hidden":
                want_g = frames[vm.key("void_hidden_dark%d" % g, "pixel", 0, (W, H))]
            else:
                want_g = c.twin([c.lights[g]]).render(W, H, vm.SPP, vm.SEED, "pixel", rr=vm.RR, threads=8)[0]
            rg.assert_words_equal(fr[0, g], want_g, "%s light groups G = %d, group %d" % (name, G, g))
            if name == "void_seen" and G == 3:
                assert bool(fr[0, g].view("<u4").any()) == (g != vm.ENCLOSED_LIGHT)
        rg.assert_words_equal(rgb[0], own, name + " light groups: the unsplit frame")
        rg.assert_words_equal(st[0], states, name + " light groups: final states")


@pytest.mark.parametrize("name", ("void_seen", "all_void"))
def test_lanes_features(api, oracle, tool, case, tmp_path, name):
    """--features: a void first hit does not count in hits and adds nothing to albedo, normal or depth; ids of sample 0 holds
    material 0 with the shape's prim, which is --raycast's for that sample's ray.  all_void: colours +0, hits 0, ids 0 with a prim"""
    c = case(name)
    want, f = vm.feature_expected(c, c.cam, vm.SEED)
    prims = hs.raycast(hs.built("host_sim"), tmp_path, c.scn, f.rays[:, 0], c.base, threads=2)[0]["prim"]
    got, _ = fc.host_sim(tool, tmp_path, c.scn, W, H, None, vm.FEATURE_SPP, seed=vm.SEED, base=c.base, threads=2)
    void = vm.assert_features({k: v[0] for k, v in got.items()}, want, f, prims, name + " features")
    assert void >= (W * H if name == "all_void" else W * H // 10)
    if name == "all_void":
        for k in ("albedo", "normal", "depth", "hits"):
            assert not np.ascontiguousarray(got[k]).view("<u4").any(), k
        assert not got["ids"][0, ..., 0].any() and (got["ids"][0, ..., 1] != fc.NO_PRIM).all()
    else:
        partial = (want["hits"] > 0) & (want["hits"] < vm.FEATURE_SPP)
        assert partial.any()


@pytest.mark.parametrize("name", vm.SCENES + ("all_void",))
def test_lanes_follow(api, oracle, tool, case, tmp_path, name):
    """--follow, the single frame and a batch of four views (void_material.view_cameras, one of them inside a void sphere, and
    GLASS_CAM, which looks at void shapes through the glass sphere), from the arrays, from the tables image and with the exact
    walk forced, at (spp 5, rr 0.5, cap 64) and (rr 0.8, cap 2), against follow_cases' chain.  A sample that ends on a void shape
    -- a camera ray or a bounce ray -- records nothing; as sample 0 it leaves ids {0, that shape}, the shape --raycast names for
    the chain's last ray, and not NO_PRIM, which stays for a miss and for a sample 0 the roulette ended.  At cap 64 the chain's
    final states are first pinned against the diffuse twin's PIXEL states from the oracle (void_hidden, void_seen: every pixel
    of every frame).  all_void: every plane +0, hits 0, ids {0, a shape} or {0, NO_PRIM}, and the final states are --features'
    at the same spp: nothing can be followed"""
    c = case(name)
    w = vm.follow_world(api, c)
    fw.pin_on_twin(oracle, w, vm.FEATURE_SPP, vm.FOLLOW_SETTINGS[0][0], c.csg)
    vm.follow_conditions(api, c)
    cast = lambda rays: hs.raycast(hs.built("host_sim"), tmp_path, c.scn, rays, c.base, threads=2)[0]["prim"]
    for e in RENDER_SETS:
        last = {}

        def render(batch, rr, cap):
            kw = dict(cams=w.fcams, seeds=w.fseeds) if batch else dict(seed=vm.SEED)
            last[batch] = fw.host_sim(tool, tmp_path, c.scn, W, H, None, vm.FEATURE_SPP, rr, cap, base=c.base, env=e, threads=2, **kw)[0]
            return last[batch]
        assert fw.assert_renders(render, cast, w, vm.FEATURE_SPP, vm.FOLLOW_SETTINGS, "%s follow %r" % (name, e)) == 0
        if name == "all_void":
            first, _ = fc.host_sim(tool, tmp_path, c.scn, W, H, None, vm.FEATURE_SPP, cams=w.fcams, seeds=w.fseeds, base=c.base, env=e, threads=2)
            got = last[True]
            for k in ("albedo", "normal", "depth", "hits", "bounces"):
                assert not np.ascontiguousarray(got[k]).view("<u4").any(), k
            assert not got["ids"][..., 0].any() and (got["ids"][..., 1] != fc.NO_PRIM).any()
            rg.assert_words_equal(got["states"], first["states"], "all_void: the final states are the first-hit render's")


def test_lanes_accumulate(api, tool, case, chain_file, tmp_path):
    """--accumulate.  void_hidden: 64 samples as 1 + 3 + 12 + 48 against the fold of the REFERENCE's chains (chains_void.npz: paths
    that meet void shapes at bounces).  void_seen: accumulate_cases.identity_2_per_pixel against the oracle's chains; a pixel
    whose every camera sample ends on a void shape keeps sum, m2 and out_rgb at +0 while its count and state advance; and a
    batch of void_material.view_cameras -- one inside a void sphere -- in passes of 1 + 3 against the oracle's chains"""
    for e in RENDER_SETS[:2]:
        c = case("void_hidden")
        acs.reference_split(acs.host_call(tool, tmp_path, c, env=e, threads=2), vm.chains_from(chain_file, "void_hidden"), "void_hidden accumulate %r" % (e,))
        c = case("void_seen")
        call = acs.host_call(tool, tmp_path, c, env=e, threads=2)
        acs.identity_2_per_pixel(call, c, "void_seen accumulate %r" % (e,), chain=vm.chains_of(c))
        assert vm.accumulate_primary_void_pixels(call, c, "void_seen accumulate %r" % (e,)) >= 50
    single = acs.Planes()
    for n in (1, 3):
        call(single, None, n)
    got = acs.views_split(call, c, vm.view_cameras(api, c), vm.VIEW_SEEDS, (1, 3), "void_seen accumulate, views", single=single)
    assert not got.sum[2].view("<u4").any() and not got.m2[2].view("<u4").any() and (got.count[2] == 4).all()   # inside the void sphere


def test_lanes_radiance_and_irradiance(api, tool, case, tmp_path):
    """--radiance, --radiance-adaptive on hostile_materials.ray_cases (radiance_cases.mixed's rays and 16 aimed at the first
    sphere, which is void here), --irradiance and --irradiance-adaptive on the 256 points (identity I1: sample k is the
    radiance query at spp = 1 along the direction the oracle draws), against the oracle"""
    c = case("void_seen")
    cases = hm.ray_cases(c)
    exp, exp_ad, _ = hm.radiance_expected(c)
    pts_, seeds_ = vm.points_of(c)
    pts = ic.Points(pts_, seeds_, np.ones(len(pts_), bool), np.zeros(len(pts_), bool))
    chain = ic.chain_by_radiance(c.oracle, pts, 17, _one(c, tmp_path))
    for e in ({}, {"SIM_TABS": "1"}):
        rgb, fin = hs.radiance(tool, tmp_path, c.scn, cases.rays, cases.seeds, vm.QUERY_SPP, vm.RR, c.base, env=e, threads=2)
        rc.assert_same(rgb, fin, exp[0], exp[1], "radiance %r" % (e,))
        ac.assert_same(ac.host_sim(tool, tmp_path, c.scn, cases.rays, cases.seeds, ac.MAIN, vm.RR, c.base, env=e, threads=2), exp_ad, "adaptive radiance %r" % (e,))
        rgb, fin, _ = ic.host_sim(tool, tmp_path, c.scn, pts.points, pts.seeds, 8, vm.RR, c.base, env=e, threads=4)
        w_rgb, w_fin = ic.expected_from(chain, pts, 8)
        rc.assert_same(rgb, fin, w_rgb, w_fin, "irradiance %r" % (e,))
        got, _ = ic.host_sim_adaptive(tool, tmp_path, c.scn, pts.points, pts.seeds, ic.EVERY, vm.RR, c.base, env=e, threads=4)
        ac.assert_same(got, ic.expected_adaptive(chain, pts, ic.EVERY), "adaptive irradiance %r" % (e,))


# ---- the scene of arrays, on the CPU: the loader and the oracle (tools/host_sim reads files only) -------------------------------------
@pytest.mark.parametrize("name", vm.ARRAYS)
def test_arrays_scene_holds_both_orders_of_the_tie(api, oracle, name):
    """ort_scene_create keeps mat = 0 where the caller put it -- in the middle and at the end of every array -- and the oracle's
    closest hit on a coincident pair carries the material of the shape the reference's test order meets first -- the earlier of
    the array for at least nine rays in ten; the octree's visiting order may give a ray to the other -- so both outcomes of the
    tie occur, for spheres and for boxes"""
    c = vm.arrays_case(api, oracle, name)
    f = c.flat
    for arr in (f.spheres, f.boxes, f.cylinders):
        m = arr["mat"]
        assert m[-1] == 0 and (m[1:-1] == 0).any() and m[0] != 0
    assert [m["mat"] for m in f.meshes] == [3, 0, 6]
    osc = c.twin(None)
    for kind, arr in (("spheres", f.spheres), ("boxes", f.boxes)):
        for order in (0, 1):
            rays, solid = vm.pair_rays(c, kind, order)
            t, _, mat = osc.raycast(rays[:, 0:3], rays[:, 3:6])
            want = 0 if order == 0 else solid
            print(kind, order, "rays to the earlier shape: %d of %d" % ((mat == want).sum(), len(mat)))
            assert (t < 1.6).all() and np.isin(mat, (0, solid)).all() and (mat == want).mean() >= 0.9, (kind, order, mat)
