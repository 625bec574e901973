"""Hostile shapes, on the CPU (tests/hostile_shapes.py): the loader, the oracle and the host-compiled lane code against the
REFERENCE'S OWN closest hits, frames, final states and chains of scenes whose shapes have zero, negative and inverted sizes, zero
axes, vanishing and huge scales (tests/golden/raycast_shapes.npz, renders_shapes.npz, chains_shapes.npz; make_golden.py
--only-shapes), the conditions that keep the cases from being empty, where the commit puts the hostile shapes (prologue or
leaf), and the scenes the commit refuses.  All of this runs before anything goes to a GPU
(tests/test_gpu_hostile_shapes.py): it is what says that a divergence on the device is the device's.

Everything is compared with hostile_materials.same_words: bit for bit, NaN matching NaN; no pixel, ray or point is skipped."""
import numpy as np
import pytest

import accumulate_cases as acs
import adaptive_cases as ac
import ao_cases as ao
import feature_cases as fc
import follow_cases as fw
import host_sim_tool as hs
import hostile_materials as hm
import hostile_shapes as hsh
import irradiance_cases as ic
import light_groups_cases as lg
import radiance_cases as rc
import ref_io
import reference_goldens as rg
import render_adaptive_cases as rac
import sample_map_cases as sm
from raycast_cases import FLT_MAX, assert_same_answers

DIGEST_KEYS = ("counts", "camera_bits", "ambient_bits", "materials_sha256", "spheres_sha256", "boxes_sha256", "cylinders_sha256", "lights", "meshes")
W, H = hsh.W, hsh.H
same = hsh.same_words


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
def case(api, oracle, manifest, tmp_path_factory):
    def get(name):
        c = hsh.case(api, oracle, name, tmp_path_factory)
        if name not in hsh.SPECULAR:   # those are written for the follow renders alone: the reference has no fixture of them
            assert rg.sha256(c.scn) == manifest["generated"]["shapes"]["scenes"][name]["scn_sha256"], name
        return c
    return get


# ---- the loader --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hsh.STEMS)
def test_loader_keeps_the_hostile_sizes_as_written(case, manifest, name):
    """every array has the reference loader's digest: a negative or zero radius stays as written, a box written with a negative
    extent has max < min, a zero axis stays zero, a mesh scaled by 0 has every vertex at its place, and every cylinder with a
    material -- the zero-axis one too -- is on the light list"""
    c = case(name)
    meta = manifest["generated"]["shapes"]["scenes"][name]
    dg = ref_io.scene_digest(c.flat)
    for k in DIGEST_KEYS:
        assert dg[k] == meta[k], (name, k)
    f = c.flat
    if name in ("shapes_seen", "shapes_leaves"):
        at = hsh.shape_index(f)
        assert f.spheres[at["sphere_neg"][1]]["r"] == np.float32(-0.5) and f.spheres[at["sphere_zero"][1]]["r"] == 0
        assert f.spheres[at["sphere_tiny"][1]]["r"] == np.float32(1e-20)
        b = f.boxes[at["box_inv1"][1]]
        assert b["max"][0] < b["min"][0] and b["max"][1] > b["min"][1]
        b = f.boxes[at["box_inv3"][1]]
        assert (b["max"] < b["min"]).all()
        b = f.boxes[at["box_flat"][1]]
        assert b["max"][2] == b["min"][2]
        assert not f.cylinders[at["cyl_axis0"][1]]["axis"].any() and f.cylinders[at["cyl_neg"][1]]["r"] == np.float32(-0.25)
        assert f.cylinders[at["cyl_zero"][1]]["r"] == 0
        m = f.meshes[at["mesh_zero"][1]]
        assert (m["vertices"] == m["vertices"][0]).all() and (m["aabb_min"] == m["aabb_max"]).all()
        cyl_lights = sorted(int(i) for t, i in zip(f.lights["type"], f.lights["index"]) if t == 2)
        assert cyl_lights == list(range(len(f.cylinders)))
    if name == "shapes_lights":
        assert abs(f.spheres["r"][3] + 0.9) < 1e-6 and f.spheres["r"][4] == 0 and f.spheres["r"][5] == 0.5 and len(f.lights) == 6
        assert not f.cylinders[0]["axis"].any() and f.cylinders[1]["r"] == np.float32(-0.3) and f.cylinders[2]["r"] == 0


# ---- where the commit puts the hostile shapes ----------------------------------------------------------------------------------------
def test_hostile_shapes_of_every_kind_in_the_prologue_and_in_leaves(case):
    """tools/host_sim --tree-check walks the committed tree and names the prologue's shapes (every other shape lies in exactly one
    leaf, or the check fails).  shapes_leaves: seven slabs and the room fill the prologue, every hostile shape -- one of each kind at
    least -- lies in a leaf.  shapes_seen: the default commit's prologue (a budget of 14 box tests: boxes first, then spheres)
    holds the four hostile boxes and the sphere of radius -0.5 and no cylinder; committed with ORT_ANALYTIC_PROLOGUE=24 it holds a
    hostile cylinder too.  Both commits are rendered and queried below and on the device"""
    c = case("shapes_leaves")
    pro, line = hsh.prologue_of(c)
    where = hsh.in_prologue(c)
    print("shapes_leaves:", line, pro)
    assert line["prologue"] == 14 and not any(where.values())
    for kind in hsh.KINDS_OF_SHAPE:
        assert any(hsh.KIND[n] == kind for n in hsh.NAMES if not where[n])
    c = case("shapes_seen")
    where = hsh.in_prologue(c)
    print("shapes_seen:", {n: v for n, v in where.items() if v})
    assert where["box_inv1"] and where["box_inv3"] and where["box_flat"] and where["box_point"] and where["sphere_neg"]
    assert not any(where[n] for n in hsh.NAMES if hsh.KIND[n] == "cylinder")
    wide = hsh.in_prologue(c, hsh.PROLOGUE_WIDE)
    print("shapes_seen, ORT_ANALYTIC_PROLOGUE=24:", {n: v for n, v in wide.items() if v})
    for kind in ("sphere", "box", "cylinder"):
        assert any(wide[n] for n in hsh.NAMES if hsh.KIND[n] == kind), kind
    assert all(wide[n] for n in hsh.NAMES if hsh.KIND[n] == "sphere")


# ---- the oracle against the reference ------------------------------------------------------------------------------------------------
def test_oracle_closest_hits_match_reference(case, manifest, hits_file):
    """hostile_shapes.ray_sets placed by the oracle's casts are the bytes the reference's casts placed (the manifest's SHA-256),
    and t, n and mat of all rays are the reference's raycast_top_most_node, on shapes_seen and on shapes_leaves"""
    rays, kind = hsh.rays_of(case("shapes_seen"))
    meta = manifest["generated"]["shapes"]["raycast"]
    assert hsh.rays_sha256(rays) == meta["rays_sha256"] and len(rays) == meta["count"] and (kind == hits_file["kind"]).all()
    for name in hsh.RAYCAST_SCENES:
        t, n, mat = case(name).twin(None).raycast(rays[:, 0:3], rays[:, 3:6])
        zt, zn, zmat = hsh.records(hits_file, name)
        for k, what in enumerate(hsh.RAY_KINDS):
            s = kind == k
            assert_same_answers(t[s], n[s], mat[s], zt[s], zn[s], zmat[s], "oracle on %s, rays at %s" % (name, what))


def test_oracle_renders_and_chains_match_reference(api, oracle, case, manifest, frames, chain_file):
    """every frame of renders_shapes.npz -- six scenes in four policies at 24 x 16 with the PIXEL final states, PIXEL and CHUNK at
    96 x 64, the scenes without their hostile shapes, the nine dark twins -- with counters and final RNG, and the 64-sample chains"""
    meta = manifest["generated"]["shapes"]["renders"]
    assert sorted(meta) == sorted(hsh.key(s, p, ch, size) for s, p, ch, size, _ in hsh.RENDERS)
    for scene, policy, chunk, (w, h), states in hsh.RENDERS:
        key = hsh.key(scene, policy, chunk, (w, h))
        osc = oracle.OracleScene(case(scene).scene.flatten(w, h))
        if states:
            img, st, fin = rg.oracle_pixel_planes(oracle, osc, w, h, hsh.SPP, hsh.SEED, hsh.RR)
            same(fin, frames[key + "__states"], key + ": final states")
        else:
            img, st = osc.render(w, h, hsh.SPP, hsh.SEED, policy, chunk=max(chunk, 1), rr=hsh.RR, threads=1)
        same(img, frames[key], key)
        assert st["shapes_tested"] == meta[key]["shapes_tested"], key
        if policy != "tile32":
            assert st["final_rng"] == meta[key]["final_rng"], key
    for name in hsh.N_LIGHTS:
        c = case(name)
        assert len(c.lights) == hsh.N_LIGHTS[name]
        for g, m in enumerate(c.lights):
            img, _ = c.twin([m]).render(W, H, hsh.SPP, hsh.SEED, "pixel", rr=hsh.RR, threads=1)
            same(img, frames[hsh.key("%s_dark%d" % (name, g), "pixel", 0, (W, H))], "%s dark twin %d, the patched arrays" % (name, g))
    for name in hsh.CHAINS:
        got = hsh.chains_of(case(name))
        same(np.stack([got[(x, y)][0] for y in range(H) for x in range(W)]).reshape(H, W, hsh.CHAIN_SAMPLES, 3), chain_file[name + "__colours"], name + " chain colours")
        same(np.stack([got[(x, y)][1] for y in range(H) for x in range(W)]).reshape(H, W, hsh.CHAIN_SAMPLES), chain_file[name + "__states"], name + " chain states")


# ---- the conditions: no case is empty -------------------------------------------------------------------------------------------------
def test_every_hostile_shape_is_hit_or_never_hit(hits_file):
    """of the rays that start inside the room (those aimed at the shapes and those in any direction), the reference's closest-hit
    record names each hostile shape on at least 32, or on none: hostile_shapes.HIT and NEVER say which, eight and seven.  Printed:
    the counts, and what raycast_cases' extreme rays add (from 1e8 and further away the float32 quadratic reports the spheres of
    radius 0 and 1e-20 on seven rays; nothing is claimed of those but the bits, which every other test here compares)"""
    mat, kind = hits_file["mat"], hits_file["kind"]
    inside = kind != hsh.RAY_KINDS.index("edges")
    counts = {n: int((mat[inside] == hsh.MAT[n]).sum()) for n in hsh.NAMES}
    print("rays from inside the room that name each shape:", counts)
    print("raycast_cases' rays that name each shape:", {n: int((mat[~inside] == hsh.MAT[n]).sum()) for n in hsh.NAMES})
    assert set(hsh.HIT) | set(hsh.NEVER) == set(hsh.NAMES) and len(hsh.HIT) >= 6
    for n in hsh.HIT:
        assert counts[n] >= 32, (n, counts[n])
    for n in hsh.NEVER:
        assert counts[n] == 0, (n, counts[n])
    assert {"sphere_neg", "cyl_neg", "mesh_neg", "mesh_q0"} <= set(hsh.HIT)


def test_the_hostile_shapes_change_the_frames(frames):
    """every 24 x 16 PIXEL reference frame of a scene whose hostile shapes stand in the room differs in at least 16 words from the
    frame of the scene without them.  The sphere of radius 1e12, the sphere at x = 1e12 and the box at x = 1e6 lie outside the
    closed room, where no path of the reference ever gets: their frames ARE the plain scene's, in every word -- what the far shape
    changes is the product's quadric slack, so the product has to give that same frame from other boxes.  No frame of
    shapes_seen, shapes_leaves or shapes_far holds a non-finite word; those of shapes_lights may, and hold none"""
    outside = ("shapes_far_sphere_r", "shapes_far_sphere_c", "shapes_far_box")
    for name in hsh.SCENES:
        own = frames[hsh.key(name, "pixel", 0, (W, H))]
        plain = frames[hsh.key(name + "_plain", "pixel", 0, (W, H))]
        differ = int((own.view("<u4") != plain.view("<u4")).sum())
        print("%s: %d of %d words differ from the frame without the hostile shapes" % (name, differ, own.size))
        assert (differ == 0) if name in outside else (differ >= 16), name
    nonfinite = {}
    for scene, policy, chunk, size, _ in hsh.RENDERS:
        k = hsh.key(scene, policy, chunk, size)
        nonfinite[k] = int((~np.isfinite(frames[k])).sum())
        if scene.startswith(hsh.NO_NONFINITE):
            assert nonfinite[k] == 0, k
    print("non-finite words in the frames of shapes_lights:", {k: v for k, v in nonfinite.items() if k.startswith("shapes_lights")})
    dark = [int(frames[hsh.key("shapes_lights_dark%d" % g, "pixel", 0, (W, H))].view("<u4").any()) for g in range(6)]
    print("shapes_lights: which light alone lights anything:", dict(zip(hsh.LIGHT_NAMES, dark)))
    assert dark[0] and dark[3] and dark[5]      # the spheres of radius -0.9 and 0.5 and the cylinder of radius -0.3 shine


# ---- the lane code on the host -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["host_sim", "host_sim_w5"])
def tool(request):
    return hs.built(request.param)


QUERY_SETS = ({}, {"SIM_TABS": "1"}, {"SIM_FORCE_FALLBACK": "0xf"}, {"SIM_WIDE": "1"}, hsh.PROLOGUE_WIDE)
RENDER_SETS = ({}, {"SIM_TABS": "1"}, {"SIM_FORCE_FALLBACK": "0xf"})


@pytest.mark.parametrize("name", hsh.RAYCAST_SCENES)
def test_lanes_closest_hits(tool, case, hits_file, tmp_path, name):
    """--raycast on shapes_seen (hostile boxes and a sphere in the prologue) and shapes_leaves (every hostile shape in a leaf)
    against the reference's records: the default walk, the tables image, the forced fallback, the wide tree and (shapes_seen) the
    commit with a hostile cylinder in its prologue on all rays, the exact walk for every ray (SIM_FORCE_FALLBACK=0) on
    hostile_shapes.exact_subset's 2 000; a hit names a shape"""
    c = case(name)
    rays, kind = hsh.rays_of(case("shapes_seen"))
    zt, zn, zmat = hsh.records(hits_file, name)
    for e in QUERY_SETS[:4 if name == "shapes_leaves" else 5] + ({"SIM_FORCE_FALLBACK": "0"},):
        sel = hsh.exact_subset(kind) if e.get("SIM_FORCE_FALLBACK") == "0" else np.ones(len(rays), bool)
        hits, r = hs.raycast(tool, tmp_path, c.scn, rays[sel], c.base, env=e, threads=4)
        assert_same_answers(hits["t"], hits["n"], hits["mat"], zt[sel], zn[sel], zmat[sel], "%s %r" % (name, e))
        missed = hits["t"].view("<u4") == FLT_MAX.view("<u4")
        assert ((hits["prim"] == hs.NO_PRIM) == (missed | np.isnan(hits["t"]))).all(), e
        assert hsh.hostile_hit(hits["mat"]).sum() >= 0.1 * sel.sum()


def test_lanes_occlusion(tool, case, hits_file, tmp_path):
    """--occluded: occluded_cases' ladder over the reference's t (tmax one ulp either side of each hit), and without limits"""
    c = case("shapes_seen")
    rays, kind = hsh.rays_of(c)
    t, mat = hits_file["t"], hits_file["mat"]
    finite = ~np.isnan(t)
    rr, tm, want = hsh.one_ulp_ladder(rays[finite], t[finite], mat[finite])
    assert want.mean() >= 0.1 and (~want).mean() >= 0.1
    few = hsh.exact_subset(kind)[finite]
    for e in QUERY_SETS + ({"SIM_FORCE_FALLBACK": "0"},):
        rr_, tm_, want_ = (hsh.one_ulp_ladder(rays[finite][few], t[finite][few], mat[finite][few]) if e.get("SIM_FORCE_FALLBACK") == "0" else (rr, tm, want))
        got = hs.occluded(tool, tmp_path, c.scn, rr_, tm_, c.base, env=e, threads=4)
        bad = np.flatnonzero(got != want_.astype(np.uint8))
        assert len(bad) == 0, "%r: %d of %d bytes differ, first %d" % (e, len(bad), len(want_), bad[0])
    got = hs.occluded(tool, tmp_path, c.scn, rays, None, c.base, threads=4)
    assert (got == ((mat != 0) & (t < np.inf)).astype(np.uint8)).all()


def test_lanes_ambient_occlusion(tool, case, hits_file, tmp_path):
    """--ambient-occlusion on 192 points lifted off the hostile shapes' hit points, at ao_cases.radius_array's radii and without a
    radius"""
    c = case("shapes_seen")
    pts = hsh.points_of(c, hits_file)
    assert set(pts[2].tolist()) == {hsh.MAT[n] for n in hsh.HIT}
    w = hsh.ao_world(c, pts[:2])
    for e in ({}, {"SIM_TABS": "1"}, {"SIM_FORCE_FALLBACK": "0xf"}):
        for radius in (w.radii, None):
            got = ao.host_sim(tool, tmp_path, c.scn, w.pts.points, w.pts.seeds, radius, 8, base=c.base, env=e, threads=4)[:3]
            ao.assert_same(got, ao.expected(w, radius, 8), "shapes_seen AO %r" % (e,))


_shares = {}


@pytest.mark.parametrize("name", hsh.SCENES)
def test_lanes_render_the_references_frames(tool, case, frames, tmp_path, name):
    """the four policies, also through the tables image, the forced fallback, the wide tree, the wavefront trace and (shapes_seen)
    the commit with a hostile cylinder in its prologue; 96 x 64.  Printed, not capped: the share of rays that took the exact walk
    (host_sim's fallback counter) in the 96 x 64 PIXEL frame"""
    c = case(name)
    for policy, chunk in hsh.POLICIES:
        key = hsh.key(name, policy, chunk, (W, H))
        sets = RENDER_SETS + (({"SIM_WIDE": "1"}, {"SIM_WAVEFRONT": "100"}) if policy == "chunk" else ())
        sets += (hsh.PROLOGUE_WIDE,) if name == "shapes_seen" else ()
        for e in sets:
            img = hs.render(tool, tmp_path, c.scn, W, H, hsh.SPP, hsh.SEED, policy, chunk, c.base, env=e, threads=1 if "SIM_WAVEFRONT" in e else 2)
            same(img, frames[key], "%s %s %r" % (name, policy, e))
    for policy, chunk in hsh.POLICIES[:2]:
        args, outs = hs.render_args(str(tmp_path), c.scn, hsh.BIG[0], hsh.BIG[1], hsh.SPP, hsh.SEED, policy, chunk, c.base)
        r = hs.run(tool, args, threads=4)
        same(np.fromfile(outs[0], "<f4").reshape(hsh.BIG[1], hsh.BIG[0], 3), frames[hsh.key(name, policy, chunk, hsh.BIG)], "%s %s 96 x 64" % (name, policy))
        if policy == "pixel":
            k = hs.counters(r)
            print("%s: exact-walk share of the 96 x 64 PIXEL frame: %d of %d rays, %.4f" % (name, k["fallback"], k["rays"], k["fallback"] / k["rays"]))


@pytest.mark.parametrize("name", ("shapes_seen", "shapes_lights", "shapes_leaves"))
def test_lanes_render_with_every_ray_on_the_exact_walk(tool, case, tmp_path, name):
    """SIM_FORCE_FALLBACK=0: every ray of the render is re-cast by the exact walk; 24 x 16 at 4 spp, PIXEL and CHUNK, against the
    oracle (which the test above holds against the reference)"""
    c = case(name)
    for policy, chunk in hsh.POLICIES[:2]:
        want = hsh.oracle_frame(c, (W, H), policy, chunk, spp=4)
        img = hs.render(tool, tmp_path, c.scn, W, H, 4, hsh.SEED, policy, chunk, c.base, env={"SIM_FORCE_FALLBACK": "0"}, threads=4)
        same(img, want, "%s %s, the exact walk" % (name, policy))


def test_exact_walk_share_of_the_closest_hit_rays(case, hits_file, tmp_path):
    """printed, not capped: per kind of ray, the share that the default walk hands to the exact walk, on shapes_seen and on the
    scene without the hostile shapes -- which shape sends rays there that never come near it is a finding for
    profiles/r27_hostile_shapes.md"""
    c, cp = case("shapes_seen"), case("shapes_seen_plain")
    rays, kind = hsh.rays_of(c)
    for k, what in enumerate(hsh.RAY_KINDS):
        r = rays[kind == k]
        out = []
        for cc in (c, cp):
            _, run = hs.raycast(hs.built("host_sim"), tmp_path, cc.scn, r, cc.base, threads=4)
            out.append(hs.counters(run)["fallback"])
        print("rays at %-12s %5d rays: exact walk %5d (%.3f); without the hostile shapes %5d (%.3f)" % (what, len(r), out[0], out[0] / len(r), out[1], out[1] / len(r)))


@pytest.mark.parametrize("name", ("shapes_seen", "shapes_lights", "shapes_leaves"))
def test_lanes_views_adaptive_groups_and_sample_map(api, oracle, tool, case, frames, chain_file, tmp_path, name):
    """--views (the third view stands inside the sphere of radius -0.5), --render-adaptive and --sample-map on the reference's
    chains, --light-groups against the reference's dark twins: the lights of radius 0 and the zero-axis cylinder light give frames
    of +0 and still take their turn in the light pick"""
    c = case(name)
    cams = hsh.view_cameras(api, c)
    want = np.stack([hsh.oracle_frame(c, (W, H), "pixel", 0, cam=cam, seed=s) for cam, s in zip(cams, hsh.VIEW_SEEDS)])
    got = hs.views(tool, tmp_path, c.scn, cams, hsh.VIEW_SEEDS, W, H, hsh.SPP, "pixel", 0, c.base, threads=2)
    same(got, want, name + " views")
    if name != "shapes_lights":
        f = hsh.first_hits(c, (W, H), seed=hsh.VIEW_SEEDS[2], cam=cams[2])
        # measured: 0.  From inside, the reference's test does not report a sphere of negative radius: the view sees through it
        print("%s: first hits of the view inside the sphere of radius -0.5 that name it: %.3f" % (name, (f.mat[:, 0] == hsh.MAT["sphere_neg"]).mean()))
        assert (f.t[:, 0] < FLT_MAX).all() and bool(want[2].view("<u4").any())
    chain = hsh.chains_from(chain_file, name)
    ad = hm.adaptive_set()
    got = rac.host_sim(tool, tmp_path, c.scn, W, H, None, hsh.SEED, ad, hsh.RR, c.base, threads=2)
    want = rac.expected_from(chain, W, H, ad)
    for g, w_, what in zip(got, want, ("colours", "sample counts", "second moments", "final states")):
        same(g, w_, "%s adaptive %s" % (name, what))
    smap = np.minimum(want[1], sm.CAP).astype("<u4")
    (rgb, m2, fin), _ = sm.host_sample_map(tool, tmp_path, c, smap, sm.CAP, hsh.SEED, threads=2)
    for g, w_, what in zip((rgb[0], m2[0], fin[0]), sm.expected_from(chain, smap, sm.CAP), ("colours", "second moments", "final states")):
        same(g, w_, "%s sample map %s" % (name, what))
    if name not in hsh.N_LIGHTS:
        return
    own, states = frames[hsh.key(name, "pixel", 0, (W, H))], frames[hsh.key(name, "pixel", 0, (W, H)) + "__states"]
    n = len(c.lights)
    for groups, G in ((c.per_light(), n), ({m: 0 for m in c.lights}, 1)):
        fr, rgb, st = lg.host_light_groups(tool, tmp_path, c, c.table(groups), G, hsh.SPP, hsh.SEED, threads=2)
        for g in range(G):
            same(fr[0, g], frames[hsh.key("%s_dark%d" % (name, g), "pixel", 0, (W, H))] if G == n else own, "%s light groups G = %d, group %d" % (name, G, g))
        same(rgb[0], own, name + " light groups: the unsplit frame")
        same(st[0], states, name + " light groups: final states")


@pytest.mark.parametrize("name", ("shapes_seen", "shapes_leaves"))
def test_lanes_features(api, oracle, tool, case, tmp_path, name):
    """--features: albedo, normal, depth, hits and ids of first hits on hostile shapes; ids of sample 0 names the shape, which is
    --raycast's prim for that sample's ray"""
    c = case(name)
    want, f = hsh.feature_expected(c, c.cam, hsh.SEED)
    assert hsh.hostile_hit(f.mat[:, 0]).mean() >= 0.1
    prims = hs.raycast(hs.built("host_sim"), tmp_path, c.scn, f.rays[:, 0], c.base, threads=2)[0]["prim"]
    got, _ = fc.host_sim(tool, tmp_path, c.scn, W, H, None, hsh.FEATURE_SPP, seed=hsh.SEED, base=c.base, threads=2)
    hsh.assert_features({k: v[0] for k, v in got.items()}, want, f, prims, name + " features")


@pytest.mark.parametrize("name", hsh.FOLLOW_SCENES)
def test_lanes_follow(api, oracle, tool, case, tmp_path, name):
    """--follow, the single frame and the batch of hostile_shapes.view_cameras, from the arrays, from the tables image and with
    the exact walk forced, at (spp 5, rr 0.5, cap 64) and (rr 0.8, cap 2), against follow_cases' chain, whose final states are
    first pinned against the diffuse twin's PIXEL states from the oracle.  shapes_seen and shapes_leaves have no specular-only
    material -- printed: nothing is followed from any view -- so there the six planes are --features' and bounces is zero, for
    both settings (identity 2).  Their SPECULAR twins make the hostile shapes that rays meet mirrors and glass, so bounce rays
    start ON a sphere of radius -0.5, inverted and flat boxes, cylinders of radius -0.25 and 0 and meshes scaled by -0.6 or
    turned by a zero quaternion: 45 % of the own frame's samples are followed where those spheres and boxes sit in the prologue
    (shapes_seen_specular; tools/host_sim --tree-check says so here), 27 % where every hostile shape sits in a leaf
    (shapes_leaves_specular), paths 7 and 9 bounces deep.  The far scenes keep the room's glass and mirror: 12 %"""
    c = case(name)
    w = hsh.follow_world(api, c)
    fw.pin_on_twin(oracle, w, hsh.FEATURE_SPP, hsh.FOLLOW_SETTINGS[0][0], c.csg)
    follows = hsh.follow_conditions(api, c)
    assert follows == (name in hsh.FOLLOWING)
    if name in hsh.SPECULAR:   # where the commit puts the shapes the samples are followed through
        where = hsh.in_prologue(c)
        followed = fw.chains(w, hsh.FEATURE_SPP, *hsh.FOLLOW_SETTINGS[0])[0].followed_by_mat
        inside = [n for n in hsh.FOLLOW_SPECULAR if where[n] and followed[hsh.MAT[n]]]
        print("%s: followed through prologue shapes %s" % (name, inside))
        if name == "shapes_seen_specular":
            assert {"sphere_neg", "box_inv1", "box_inv3", "box_flat"} <= set(inside) and not where["cyl_neg"] and followed[hsh.MAT["cyl_neg"]]
        else:
            assert not any(where.values())
    cast = lambda rays: hs.raycast(hs.built("host_sim"), tmp_path, c.scn, rays, c.base, threads=2)[0]["prim"]
    for e in RENDER_SETS:
        last = {}

        def render(batch, rr, cap):
            kw = dict(cams=w.fcams, seeds=w.fseeds) if batch else dict(seed=hsh.SEED)
            last[batch] = fw.host_sim(tool, tmp_path, c.scn, W, H, None, hsh.FEATURE_SPP, rr, cap, base=c.base, env=e, threads=2, **kw)[0]
            if not follows:
                first, _ = fc.host_sim(tool, tmp_path, c.scn, W, H, None, hsh.FEATURE_SPP, base=c.base, env=e, threads=2, **kw)
                for k in fc.PLANES:
                    same(last[batch][k], first[k], "%s %r rr %g cap %d: %s against --features" % (name, e, rr, cap, k))
                assert not last[batch]["bounces"].any()
            return last[batch]
        fw.assert_renders(render, cast, w, hsh.FEATURE_SPP, hsh.FOLLOW_SETTINGS, "%s follow %r" % (name, e))


@pytest.mark.parametrize("name", hsh.CHAINS)
def test_lanes_accumulate(api, tool, case, chain_file, tmp_path, name):
    """--accumulate: 64 samples as 1 + 3 + 12 + 48 against the fold of the REFERENCE's chains (chains_shapes.npz), from the arrays
    and from the tables image: a continued job reloads its sums and its state and walks on among the hostile shapes (and, in
    shapes_lights, towards the hostile lights); a batch of hostile_shapes.view_cameras in passes of 1 + 3 against the oracle's
    chains from each camera"""
    c = case(name)
    for e in RENDER_SETS[:2]:
        call = acs.host_call(tool, tmp_path, c, env=e, threads=2)
        acs.reference_split(call, hsh.chains_from(chain_file, name), "%s accumulate %r" % (name, e), nan=name not in hsh.NO_NONFINITE)
    single = acs.Planes()
    for n in (1, 3):
        call(single, None, n)
    acs.views_split(call, c, hsh.view_cameras(api, c), hsh.VIEW_SEEDS, (1, 3), name + " accumulate, views", nan=name not in hsh.NO_NONFINITE, single=single)


def _one(c, d):
    return lambda rays, seeds: hs.radiance(hs.built("host_sim"), d, c.scn, rays, seeds, 1, hsh.RR, c.base, threads=4)


def test_lanes_radiance_and_irradiance(api, tool, case, hits_file, tmp_path):
    """--radiance, --radiance-adaptive on hostile_materials.ray_cases (radiance_cases.mixed's rays and 16 aimed at the scene's first
    sphere, the one of radius -0.5), --irradiance and --irradiance-adaptive on the 192 points lifted off the hostile shapes
    (identity I1: sample k is the radiance query at spp = 1 along the direction the oracle draws), against the oracle"""
    c = case("shapes_seen")
    assert c.flat.spheres[hm.AIM_SPHERE[0]]["r"] == np.float32(-0.5)
    cases = hm.ray_cases(c)
    exp, exp_ad, _ = hm.radiance_expected(c)
    p_, s_, _ = hsh.points_of(c, hits_file)
    pts = ic.Points(p_, s_, np.ones(len(p_), bool), np.zeros(len(p_), bool))
    chain = ic.chain_by_radiance(c.oracle, pts, 17, _one(c, tmp_path))
    for e in ({}, {"SIM_TABS": "1"}):
        rgb, fin = hs.radiance(tool, tmp_path, c.scn, cases.rays, cases.seeds, hsh.QUERY_SPP, hsh.RR, c.base, env=e, threads=2)
        rc.assert_same(rgb, fin, exp[0], exp[1], "radiance %r" % (e,))
        ac.assert_same(ac.host_sim(tool, tmp_path, c.scn, cases.rays, cases.seeds, ac.MAIN, hsh.RR, c.base, env=e, threads=2), exp_ad, "adaptive radiance %r" % (e,))
        rgb, fin, _ = ic.host_sim(tool, tmp_path, c.scn, pts.points, pts.seeds, 8, hsh.RR, c.base, env=e, threads=4)
        w_rgb, w_fin = ic.expected_from(chain, pts, 8)
        rc.assert_same(rgb, fin, w_rgb, w_fin, "irradiance %r" % (e,))
        got, _ = ic.host_sim_adaptive(tool, tmp_path, c.scn, pts.points, pts.seeds, ic.EVERY, hsh.RR, c.base, env=e, threads=4)
        ac.assert_same(got, ic.expected_adaptive(chain, pts, ic.EVERY), "adaptive irradiance %r" % (e,))


# ---- the scene of arrays, on the CPU: the loader and the oracle (tools/host_sim reads files only) -------------------------------------
def test_arrays_scene_keeps_what_a_file_cannot_say(api, oracle):
    """ort_scene_create keeps a radius of -0.0 and a denormal one bit for bit, a box with min == max, an index buffer that repeats
    a vertex, and material 0 on hostile shapes; the oracle's closest hits name the hostile solid shapes and the void ones"""
    c = hsh.arrays_case(api, oracle)
    f = c.flat
    assert f.spheres[2]["r"].tobytes() == np.float32(-0.0).tobytes() and f.spheres[3]["r"].tobytes() == np.float32(1e-40).tobytes()
    assert (f.boxes[3]["min"] == f.boxes[3]["max"]).all() and f.boxes[7]["mat"] == 0 and f.spheres[4]["mat"] == 0 and f.cylinders[1]["mat"] == 0
    ix = np.asarray(f.meshes[0]["indices"]).reshape(-1)
    assert ix[0] == ix[1] == ix[2] and ix[3] == ix[4] == ix[5]
    rays = hsh.arrays_rays(c)
    t, _, mat = c.twin(None).raycast(rays[:, 0:3], rays[:, 3:6])
    aimed = slice(1000, 2000)
    void = (t[aimed] < FLT_MAX) & (mat[aimed] == 0)
    print("arrays_shapes: void closest hits on %.3f of the aimed rays; materials hit %r" % (void.mean(), sorted(set(mat.tolist()))))
    assert void.mean() >= 0.05 and not np.isnan(t).any() and set(mat.tolist()) >= {0, 1, 2, 3, 6}


# ---- the scenes the commit refuses -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,line", hsh.REFUSED)
def test_commit_refuses_nonfinite_and_oversized_shapes(api, what, line, tmp_path):
    """ort_scene_commit returns ORT_ERR_INVALID with the stated message for a NaN centre, an infinite radius and a radius of 1e20
    (bounds beyond 1e30 after the slack), through the loader and through ort_scene_create; the scene stays usable -- it still
    answers ort_scene_info, refuses again in the same way, and is destroyed cleanly"""
    scene = api.Scene.parse_scn(hsh.refused_text(line), str(tmp_path) + "/")
    flat = scene.flatten(W, H)
    sph = flat.spheres.copy()
    assert not np.isfinite(sph["center"]).all() or not np.isfinite(sph["r"]).all() or (np.abs(sph["r"]) >= 1e20).any()
    for s in (scene, api.Scene.from_arrays(flat.materials, sph, flat.boxes, flat.cylinders, flat.lights, [], camera_p=hsh.vm.CAMERA_P,
                                           camera_quat_xyzw=(0.416981, 0.279589, 0.480987, 0.718247), camera_height_ratio=0.2, screen=(W, H))):
        for _ in range(2):
            with pytest.raises(api.OrtError) as e:
                s.commit()
            assert e.value.code == api.ERR_INVALID and hsh.REFUSED_MESSAGE in str(e.value), (what, str(e.value))
            assert s.info().sphere_count == len(sph) and len(s.flatten(W, H).spheres) == len(sph)
            with pytest.raises(api.OrtError) as e:      # not committed: nothing renders it
                s.tree_info()
            assert e.value.code == api.ERR_STATE
        s.close()


@pytest.mark.parametrize("what,line", hsh.ACCEPTED)
def test_commit_accepts_a_radius_of_1e12(api, what, line, tmp_path):
    scene = api.Scene.parse_scn(hsh.refused_text(line), str(tmp_path) + "/").commit()
    assert scene.tree_info()["node_count"] >= 1
