"""SH light-probe queries (ort_probe_sh) against what exists: the points, and what they must give.

Nothing of the path is restated here.  A sample of a point (p, n) is a direction drawn over the whole sphere about the pole n and
then a radiance query's sample along it; what the sample adds to the colour sum it also adds, times the SH basis at that
direction, to nine more sums (include/ort.h):

  the direction   from the oracle alone, exactly as irradiance_cases.directions composes it, with c = 1 - 2 e0 where that has
                  sqrt(e0): the draws from oracle.rng_table, c and phi as IEEE float32 operations in numpy, sample_lobe from the
                  oracle's unit op 8, normalize from op 10;
  the basis       numpy float32, one rounding per operation, in the header's order (basis);
  rr = 0          identity I2: the sample's colour from OracleScene.raycast along the direction and the material table alone;
  rr > 0          identity I1: sample k is the existing radiance query at spp = 1 for the ray (p, d_k) with seed s'_k -- K chained
                  calls through the returned states (tools/host_sim --radiance on the CPU, ort_radiance on the GPU);
  the fold        a sample adds one vector e to the colour sum or none (a path ends at the light it reaches), and a spp = 1
                  radiance call returns (+0 + e) / 1.0f: the sample's colour IS what it added, up to the sign of a zero, which no
                  sum that starts at +0 keeps.  So S[j] = S[j] + b_j(d_k) * colour_k over all samples, in float32, is the
                  kernels' S bit for bit (a sample that added nothing adds +-0), and the mean is S / float32(spp).
"""
import os
import zlib

import numpy as np

import host_sim_tool as hs
import irradiance_cases as ic
import radiance_cases as rc
import ref_io
import unit_cases as U

F = np.float32
RR = 0.8
SPP = 8
SCENES = {"testscene": 128, "c2_analytic": 128}   # points per scene; c2_analytic: specular materials, boxes and quadrics in the tree
TILTED = np.array([0.48, -0.6, 0.64], "<f4")       # a pole off every axis, |n|^2 = 1 in float32


# ---- the sphere draw, from the oracle ------------------------------------------------------------------------------------------
def directions(oracle, normals, states):
    """-> (d float32[n, 3], wo = -normalize(d), the states after the two draws): include/ort.h's composition for ort_probe_sh"""
    e0, e1, after = ic.draws(oracle, states)
    with np.errstate(all="ignore"):
        c = (F(1.0) - (F(2.0) * e0).astype("<f4")).astype("<f4")
        phi = (U.TWO_PI * e1).astype("<f4")
    rows = np.concatenate([np.asarray(normals, "<f4"), c[:, None], phi[:, None]], axis=1)
    m = oracle.unit_batch(ref_io.make_unit_records(8, rows))[:, :3]
    d = oracle.unit_batch(ref_io.make_unit_records(10, m))[:, :3]
    wo = -oracle.unit_batch(ref_io.make_unit_records(10, d))[:, :3]
    return np.ascontiguousarray(d, "<f4"), np.ascontiguousarray(wo, "<f4"), after


def op21_expected(oracle, seeds, normals):
    """-> float32[n, 8]: d.xyz wo.xyz rng(bits) 0, the seed a stream state as it stands (rows: irradiance_cases.op20_rows)"""
    d, wo, after = directions(oracle, normals, seeds)
    return np.concatenate([d, wo, after.view("<f4").reshape(-1, 1), np.zeros((len(d), 1), "<f4")], axis=1)


def basis(d):
    """the nine basis values at d (n, 3), float32 per operation, in the header's order -> float32[n, 9]"""
    d = np.asarray(d, "<f4")
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all="ignore"):
        xy, yz, xz = (x * y).astype("<f4"), (y * z).astype("<f4"), (x * z).astype("<f4")
        zz, xx, yy = (z * z).astype("<f4"), (x * x).astype("<f4"), (y * y).astype("<f4")
        b = [np.full(len(d), F(0.282094792), "<f4"),
             (F(0.488602512) * y).astype("<f4"), (F(0.488602512) * z).astype("<f4"), (F(0.488602512) * x).astype("<f4"),
             (F(1.092548431) * xy).astype("<f4"), (F(1.092548431) * yz).astype("<f4"),
             (F(0.315391565) * ((F(3.0) * zz).astype("<f4") - F(1.0)).astype("<f4")).astype("<f4"),
             (F(1.092548431) * xz).astype("<f4"), (F(0.546274215) * (xx - yy).astype("<f4")).astype("<f4")]
    return np.stack(b, axis=1).astype("<f4")


def op22_directions():
    """directions for the basis: the axes, +-0 components, a subnormal component, and 256 random unit vectors"""
    rng = np.random.default_rng(22)
    sub = np.array([1e-42], "<f4")[0]
    fixed = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (-0.0, 0.0, 1), (0.0, -0.0, -1), (1, -0.0, -0.0), (-0.0, -1, 0.0),
             (sub, 0.6, 0.8), (0.6, -sub, 0.8), (0.8, 0.6, sub), (-sub, -sub, 1), tuple(TILTED), (0.57735026, 0.57735026, 0.57735026)]
    return np.concatenate([np.array(fixed, "<f4"), rc._units(rng, 256).astype("<f4")])


def assert_bits(got, want, what):
    """all bits, the sign of a zero included"""
    ic.assert_op20(got, want, what)


# ---- the points ----------------------------------------------------------------------------------------------------------------
def point_set(name, flat, osc, n, bad=8, far=8):
    """irradiance_cases.point_set's recipe -- half near a light, the eight lobe normals (exactly +-z and either side of
    sample_lobe's 1e-4 switch among them), far points, points outside the domain, the rest on surfaces, the seeds 0, 0xffffffff
    and the one whose first draw is 1.0 (here c = -1: d is the pole's opposite) -- with the POLES of the points near a light set in
    turn to the one the recipe gave (tilted towards the light), +z, -z and a fixed tilted one: the draw covers the sphere whatever
    the pole, so which points see light does not depend on it"""
    rng = np.random.default_rng(zlib.crc32(("probe " + name).encode()))
    lo, hi = rc.origin_box(flat)
    near = ic.near_lights(rng, flat, lo, hi, n // 2)
    for k, pole in ((1, (0, 0, 1)), (2, (0, 0, -1)), (3, TILTED)):
        near[k::4, 3:6] = np.asarray(pole, "<f4")
    lobes = ic.lobe_normals()
    surf = ic.on_surfaces(rng, osc, lo, hi, n - n // 2 - far - bad)
    lobe_pts = np.concatenate([surf[:len(lobes), 0:3], lobes], axis=1)
    pts = np.concatenate([near, lobe_pts, surf[len(lobes):], ic.far_points(rng, lo, hi, far), ic.out_of_domain(rng, lo, hi, bad)]).astype("<f4")
    assert len(pts) == n
    seeds = rng.integers(1, 1 << 32, size=n, dtype=np.uint64).astype("<u4")
    seeds[0], seeds[1], seeds[2] = 0, 0xFFFFFFFF, rc.unstep(0xFFFFFFFF)
    is_far = np.zeros(n, bool)
    is_far[n - far - bad:n - bad] = True
    ok = ic.in_domain(pts)
    assert (~ok).sum() == bad and not ok[n - bad:].any()
    perm = rng.permutation(n)
    return ic.Points(pts[perm], seeds[perm], ok[perm], is_far[perm])


# ---- what a query must give ------------------------------------------------------------------------------------------------------
def chain_closed_form(oracle, osc, flat, pts, spp):
    """identity I2 (rr = 0), from the oracle alone: {point index: (colours float32[spp, 3], the state after each sample, the
    directions float32[spp, 3])}"""
    idx = np.flatnonzero(pts.ok)
    p, nrm = pts.points[idx, 0:3], pts.points[idx, 3:6]
    s = np.where(pts.seeds[idx] == 0, 1, pts.seeds[idx]).astype("<u4")
    cols, states, dirs = np.zeros((len(idx), spp, 3), "<f4"), np.zeros((len(idx), spp), "<u4"), np.zeros((len(idx), spp, 3), "<f4")
    for k in range(spp):
        d, _, after = directions(oracle, nrm, s)
        _, _, mat = osc.raycast(p, d)
        for j in range(len(idx)):
            m = flat.materials[mat[j]]
            if mat[j] != 0 and m["is_light"]:
                cols[j, k] = m["emit"]
            s[j] = rc.step(int(after[j])) if (mat[j] != 0 and not m["is_light"]) else after[j]
        states[:, k], dirs[:, k] = s, d
    return {int(i): (cols[j], states[j], dirs[j]) for j, i in enumerate(idx)}


def chain_by_radiance(oracle, pts, spp, radiance):
    """identity I1: radiance(rays (n, 6), seeds (n,)) -> (rgb, final states) is the existing radiance query at spp = 1; call k
    gets the rays (p_i, d_ik) and the seeds s'_ik.  -> {point index: (colours, states, directions)}"""
    idx = np.flatnonzero(pts.ok)
    p, nrm = pts.points[idx, 0:3], pts.points[idx, 3:6]
    s = np.where(pts.seeds[idx] == 0, 1, pts.seeds[idx]).astype("<u4")
    cols, states, dirs = np.zeros((len(idx), spp, 3), "<f4"), np.zeros((len(idx), spp), "<u4"), np.zeros((len(idx), spp, 3), "<f4")
    for k in range(spp):
        d, _, after = directions(oracle, nrm, s)
        assert (after != 0).all()
        rgb, fin = radiance(np.concatenate([p, d], axis=1).astype("<f4"), after)
        cols[:, k], s = rgb, np.asarray(fin, "<u4").copy()
        states[:, k], dirs[:, k] = s, d
    return {int(i): (cols[j], states[j], dirs[j]) for j, i in enumerate(idx)}


def fold(cols, dirs):
    """-> S float32[9, 3] and C float32[3]: the nine sums and the colour sum over the samples in order, float32 per operation"""
    S, C = np.zeros((9, 3), "<f4"), np.zeros(3, "<f4")
    b = basis(dirs)
    with np.errstate(all="ignore"):
        for k in range(len(cols)):
            S = (S + (b[k][:, None] * cols[k][None, :]).astype("<f4")).astype("<f4")
            C = (C + cols[k]).astype("<f4")
    return S, C


def expected_from(chain, pts, spp):
    """-> (sh float32[N, 9, 3], rgb float32[N, 3], final states uint32[N]) at spp samples: the fold's means inside the domain; NaN
    in all 30 words and the seed outside"""
    n = len(pts.points)
    sh, rgb, fin = np.full((n, 9, 3), np.nan, "<f4"), np.full((n, 3), np.nan, "<f4"), pts.seeds.copy()
    for i, (cols, states, dirs) in chain.items():
        S, C = fold(cols[:spp], dirs[:spp])
        with np.errstate(all="ignore"):
            sh[i], rgb[i], fin[i] = (S / F(spp)).astype("<f4"), (C / F(spp)).astype("<f4"), states[spp - 1]
    return sh, rgb, fin


def assert_same(got, want, what):
    """got, want: (sh, rgb or None, states or None).  All bits; a NaN matches by position"""
    rc.assert_same(np.asarray(got[0]).reshape(-1, 27), got[2], np.asarray(want[0]).reshape(-1, 27), want[2], what + ", sh")
    if got[1] is not None:
        rc.assert_same(got[1], None, want[1], None, what + ", rgb")


def mixed_share(chain):
    """of the points of a chain: the share with both a sample that adds light and one that does not"""
    lit = np.array([(cols != 0).any(axis=1) for cols, _, _ in chain.values()])
    return (lit.any(axis=1) & ~lit.all(axis=1)).mean()


def lit_at_a_bounce(chain, osc, flat, pts):
    """the points with a sample that added light although its primary hit (the oracle's closest hit along the sample's direction)
    is no light: the light was reached after a bounce, where the primary direction is no longer the path's"""
    out = []
    for i, (cols, _, dirs) in chain.items():
        lit = np.flatnonzero((cols != 0).any(axis=1))
        if not len(lit):
            continue
        _, _, mat = osc.raycast(np.repeat(pts.points[i:i + 1, 0:3], len(lit), axis=0), dirs[lit])
        if any(m == 0 or not flat.materials[m]["is_light"] for m in mat):
            out.append(i)
    return out


# ---- tools/host_sim --probe-sh ---------------------------------------------------------------------------------------------------
def host_sim(tool, d, scene, points, seeds, spp, rr, want_rgb=True, want_states=True, base=None, **kw):
    """-> ((sh (n, 9, 3), rgb (n, 3) or None, final states (n,) or None), CompletedProcess)"""
    d = str(d)
    np.ascontiguousarray(points, "<f4").tofile(os.path.join(d, "probes.f32"))
    np.ascontiguousarray(seeds, "<u4").tofile(os.path.join(d, "probe_seeds.u32"))
    outs = [os.path.join(d, f) for f in ("probe_sh.f32", "probe_rgb.f32", "probe_states.u32")]
    r = hs.run(tool, ["--probe-sh"] + hs.scene_args(scene, base) + [os.path.join(d, "probes.f32"), os.path.join(d, "probe_seeds.u32"), spp, repr(float(rr)),
                                                                    outs[0], outs[1] if want_rgb else "-", outs[2] if want_states else "-"], **kw)
    sh = np.fromfile(outs[0], "<f4").reshape(-1, 9, 3)
    assert len(sh) == len(points)
    return (sh, np.fromfile(outs[1], "<f4").reshape(-1, 3) if want_rgb else None, np.fromfile(outs[2], "<u4") if want_states else None), r
