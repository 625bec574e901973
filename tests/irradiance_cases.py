"""Irradiance queries (ort_irradiance, ort_irradiance_adaptive) against what exists: the points, and what they must give.

Nothing of the path is restated here.  A sample of a point (p, n) is a direction drawn about n and then a radiance query's
sample along it (include/ort.h):

  the direction   from the oracle alone -- the two draws and the stream's state after them from oracle.rng_table (rng_01,
                  random.h), c = sqrt(e0) and phi = (2 pi) * e1 as IEEE float32 operations (numpy: correctly rounded, as the
                  library's separately rounded f32 operations), sample_lobe from the oracle's unit op 8, normalize from op 10;
  rr = 0          identity I2: the whole answer from the oracle -- OracleScene.raycast along the direction plus the material
                  table: a light's emission or nothing, one more draw exactly when a surface that is not a light is hit;
  rr > 0          identity I1: sample k is the existing radiance query at spp = 1 for the ray (p, d_k) with seed s'_k, the
                  state after the two draws -- K chained calls through the returned states (tools/host_sim --radiance on the
                  CPU, ort_radiance on the GPU), radiance_cases.mean_of for the mean, adaptive_cases.cut for the stopping rule.
"""
import os
import zlib

import numpy as np

import adaptive_cases as ac
import host_sim_tool as hs
import radiance_cases as rc
import ref_io
import unit_cases as U
from adaptive_cases import Adaptive

F = np.float32

# The parameter sets of the adaptive tests (max_spp <= 17: a chain is one radiance call per sample): adaptive_cases.MAIN cut to 16
# samples and adaptive_cases.EVERY, each with its tolerance moved.  Seven points in ten see no light in their first samples and
# stop black at min_spp; a point near a light sees it directly in a fraction of its samples, so its samples are all-or-nothing
# and the standard error falls slowly: at the tolerance of 0.3 nearly all of the others run to max_spp.  Shares of the points
# inside the domain on the composed chain at rr 0.8 (stopped at min_spp / strictly between / ran to max_spp), 128 points per
# scene (tests/test_irradiance_host.py::test_adaptive_classes_are_present holds at least 5 % each under the chosen values):
#     tolerance   (4, 16, 4) testscene     c2_analytic         (2, 17, 1) testscene     c2_analytic
#     0.3         .675 .033 .292           .775 .008 .217      .883 .025 .092           .875 .008 .117
#     0.5         .708 .050 .242           .783 .025 .192      .883 .042 .075           .875 .050 .075
#     0.6         .742 .067 .192           .800 .067 .133      .883 .067 .050           .883 .058 .058     <- EVERY
#     0.7         .775 .108 .117           .825 .100 .075      .892 .083 .025           .883 .083 .033     <- MAIN
#     0.8         .783 .125 .092           .825 .142 .033      .892 .083 .025           .883 .108 .008
MAIN = Adaptive(4, 16, 4, 0.7, 0.05)
EVERY = Adaptive(2, 17, 1, 0.6, 0.05)
SETS = (MAIN, EVERY)
RR = 0.8


# ---- the hemisphere draw, from the oracle --------------------------------------------------------------------------------------
def draws(oracle, states):
    """per stream state: two rng_01 -> (e0, e1 float32[n], the state after them uint32[n])"""
    n = len(states)
    e0, e1, after = np.zeros(n, "<f4"), np.zeros(n, "<f4"), np.zeros(n, "<u4")
    for i, s in enumerate(states):
        tab = np.frombuffer(oracle.rng_table(int(s), 2)[:16], "<u4")    # state, value bits, state, value bits
        e0[i], e1[i] = tab[1:2].view("<f4")[0], tab[3:4].view("<f4")[0]
        after[i] = tab[2]
    return e0, e1, after


def directions(oracle, normals, states):
    """-> (d float32[n, 3], wo = -normalize(d), the states after the two draws): the composition of include/ort.h"""
    e0, e1, after = draws(oracle, states)
    with np.errstate(all="ignore"):
        c = np.sqrt(e0).astype("<f4")
        phi = (U.TWO_PI * e1).astype("<f4")
    rows = np.concatenate([np.asarray(normals, "<f4"), c[:, None], phi[:, None]], axis=1)
    m = oracle.unit_batch(ref_io.make_unit_records(8, rows))[:, :3]
    d = oracle.unit_batch(ref_io.make_unit_records(10, m))[:, :3]
    wo = -oracle.unit_batch(ref_io.make_unit_records(10, d))[:, :3]
    return np.ascontiguousarray(d, "<f4"), np.ascontiguousarray(wo, "<f4"), after


def op20_rows(seeds, normals):
    """the unit records' rows of op 20: seed(bits) n.xyz"""
    return np.concatenate([np.asarray(seeds, "<u4").view("<f4").reshape(-1, 1), np.asarray(normals, "<f4")], axis=1)


def op20_expected(oracle, seeds, normals):
    """-> float32[n, 8]: d.xyz wo.xyz rng(bits) 0, the seed a stream state as it stands"""
    d, wo, after = directions(oracle, normals, seeds)
    return np.concatenate([d, wo, after.view("<f4").reshape(-1, 1), np.zeros((len(d), 1), "<f4")], axis=1)


def assert_op20(got, want, what):
    """all bits, the sign of a zero included"""
    g, w = np.ascontiguousarray(got, "<f4").view("<u4"), np.ascontiguousarray(want, "<f4").view("<u4")
    ne = g != w
    if ne.any():
        i = np.argwhere(ne)[0]
        raise AssertionError("%s: %d of %d words differ; first at %s: %#x vs %#x" % (what, ne.sum(), ne.size, tuple(i), g[tuple(i)], w[tuple(i)]))


# ---- the points ----------------------------------------------------------------------------------------------------------------
LOBE_Z = (1.0, -1.0, 1 - 5e-5, -(1 - 5e-5), 1 - 2e-4, -(1 - 2e-4))   # exactly +-z; either side of sample_lobe's 1e-4 switch


def len2(n):
    """|n|^2 as the domain test computes it: x*x + y*y + z*z, float32 per operation"""
    n = np.asarray(n, "<f4")
    return ((n[..., 0] * n[..., 0]).astype("<f4") + (n[..., 1] * n[..., 1]).astype("<f4")).astype("<f4") + (n[..., 2] * n[..., 2]).astype("<f4")


def in_domain(points):
    with np.errstate(all="ignore"):
        l2 = len2(points[:, 3:6])
        return np.isfinite(points).all(axis=1) & (l2 >= F(0.999)) & (l2 <= F(1.001))


def lobe_normals():
    """-> (8, 3): (0,0,1), (0,0,-1), n.z at +-(1 - 5e-5) and +-(1 - 2e-4) with n.x making |n|^2 about 1, and two normals whose
    |n|^2 is the first float32 inside the domain from below 0.999 and from above 1.001"""
    out = []
    for z in LOBE_Z:
        z = F(z)
        out.append([F(np.sqrt(F(1) - z * z)), F(0), z])
    u = np.array([0.48, -0.6, 0.64], "<f4")
    for edge, up in ((0.999, True), (1.001, False)):
        s = F(np.sqrt(edge))
        while True:   # walk into the domain
            n = (u * s).astype("<f4")
            l2 = len2(n)
            if l2 >= F(0.999) and l2 <= F(1.001):
                break
            s = np.nextafter(s, F(np.inf) if up else F(0))
        while True:   # and back to its edge
            t = np.nextafter(s, F(0) if up else F(np.inf))
            l2 = len2((u * t).astype("<f4"))
            if not (l2 >= F(0.999) and l2 <= F(1.001)):
                break
            s = t
        out.append((u * s).astype("<f4"))
    return np.array(out, "<f4")


def _lights(flat):
    """-> [(centre, radius)]: a sphere's own, a cylinder's middle and the larger of its radius and half its length"""
    out = []
    for kind, index in zip(flat.lights["type"], flat.lights["index"]):
        if kind == 1:
            out.append((flat.spheres["center"][index], abs(float(flat.spheres["r"][index]))))
        else:
            c = flat.cylinders[index]
            out.append((c["base"] + F(0.5) * c["axis"], max(abs(float(c["r"])), 0.5 * float(np.linalg.norm(c["axis"])))))
    return out


def near_lights(rng, flat, lo, hi, n):
    """points that face a light from 1.3 to 3 of its radii, the normal (towards the light) jittered by 0.3; inside the scene's
    box.  Without lights: anywhere inside"""
    lights = _lights(flat)
    out = []
    while len(out) < n:
        if not lights:
            p, nn = rng.uniform(lo, hi), rc._units(rng, 1)[0]
        else:
            centre, radius = lights[rng.integers(0, len(lights))]
            u = rc._units(rng, 1)[0]
            p = centre + u * F(radius * rng.uniform(1.3, 3.0))
            nn = -u + rng.normal(size=3) * 0.3
            nn = nn / np.linalg.norm(nn)
        if (p > lo).all() and (p < hi).all():
            out.append(np.concatenate([p, nn]))
    return np.array(out, "<f4")


def on_surfaces(rng, osc, lo, hi, n):
    """points found with oracle.raycast from inside the box, lifted by 1e-3 along the hit normal on the side the ray came from"""
    out = []
    while len(out) < n:
        od = [rc.pinhole(p, z) for p, z in rc.inside(rng, lo, hi, 2 * n + 8)]
        o, d = np.array([a for a, _ in od]), np.array([b for _, b in od])
        t, nrm, mat = osc.raycast(o, d)
        for oi, di, ti, ni, mi in zip(o, d, t, nrm, mat):
            if mi == 0 or len(out) >= n:
                continue
            nn = ni if np.dot(ni, di) < 0 else -ni
            out.append(np.concatenate([oi + ti * di + F(1e-3) * nn, nn]))
    return np.array(out, "<f4")


def far_points(rng, lo, hi, n):
    """points 1 to 3 box diagonals outside the scene's box, facing a point inside it: with quadrics in the tree every primary
    sample takes the exact walk"""
    cams = rc.outside(rng, lo, hi, n)
    return np.concatenate([cams[:, 0], -cams[:, 1]], axis=1).astype("<f4")


def out_of_domain(rng, lo, hi, n):
    """-> (n, 6) points outside the per-point domain: a NaN in p, an infinity in p, a NaN in n, |n| of 0, 0.5 and 2"""
    pts = np.concatenate([rng.uniform(lo, hi, size=(n, 3)), rc._units(rng, n)], axis=1).astype("<f4")
    for i in range(n):
        kind = i % 6
        if kind == 0:
            pts[i, i % 3] = F(np.nan)
        elif kind == 1:
            pts[i, (i // 6 + 1) % 3] = F(np.inf) if (i // 6) % 2 == 0 else F(-np.inf)
        elif kind == 2:
            pts[i, 3 + i % 3] = F(np.nan)
        else:
            pts[i, 3:6] *= F((0.0, 0.5, 2.0)[kind - 3])
    return pts


class Points:
    """points (N, 6) p.xyz n.xyz, seeds (N,), ok (N,) bool: inside the domain, far (N,) bool: outside the scene's box"""

    def __init__(self, points, seeds, ok, far):
        self.points, self.seeds, self.ok, self.far = points, seeds, ok, far

    def take(self, idx):
        return Points(self.points[idx], self.seeds[idx], self.ok[idx], self.far[idx])


def point_set(name, flat, osc, n, bad=8, far=8):
    """n points, seeded by the scene's name, shuffled: half near a light, eight lobe normals, `far` far points, `bad` outside the
    domain, the rest on surfaces.  Seeds are arbitrary words; among the points near a light one is 0, one 0xffffffff and one
    a state whose first draw is state 0xffffffff: rng_01 == 1.0, so c = 1"""
    rng = np.random.default_rng(zlib.crc32(("irradiance " + name).encode()))
    lo, hi = rc.origin_box(flat)
    near = near_lights(rng, flat, lo, hi, n // 2)
    lobes = lobe_normals()
    surf = on_surfaces(rng, osc, lo, hi, n - n // 2 - far - bad)
    lobe_pts = np.concatenate([surf[:len(lobes), 0:3], lobes], axis=1)   # where a surface point stands, with the normal swapped
    pts = np.concatenate([near, lobe_pts, surf[len(lobes):], far_points(rng, lo, hi, far), out_of_domain(rng, lo, hi, bad)]).astype("<f4")
    assert len(pts) == n
    seeds = rng.integers(1, 1 << 32, size=n, dtype=np.uint64).astype("<u4")
    seeds[0], seeds[1], seeds[2] = 0, 0xFFFFFFFF, rc.unstep(0xFFFFFFFF)
    is_far = np.zeros(n, bool)
    is_far[n - far - bad:n - bad] = True
    ok = in_domain(pts)
    assert (~ok).sum() == bad and not ok[n - bad:].any()
    perm = rng.permutation(n)
    return Points(pts[perm], seeds[perm], ok[perm], is_far[perm])


# ---- what a query must give ------------------------------------------------------------------------------------------------------
def chain_closed_form(oracle, osc, flat, pts, spp):
    """identity I2 (rr = 0), from the oracle alone: {point index: (colours float32[spp, 3], the state after each sample)}"""
    idx = np.flatnonzero(pts.ok)
    p, nrm = pts.points[idx, 0:3], pts.points[idx, 3:6]
    s = np.where(pts.seeds[idx] == 0, 1, pts.seeds[idx]).astype("<u4")
    cols = np.zeros((len(idx), spp, 3), "<f4")
    states = np.zeros((len(idx), spp), "<u4")
    for k in range(spp):
        d, _, after = directions(oracle, nrm, s)
        _, _, mat = osc.raycast(p, d)
        for j in range(len(idx)):
            m = flat.materials[mat[j]]
            if mat[j] != 0 and m["is_light"]:
                cols[j, k] = m["emit"]
            s[j] = rc.step(int(after[j])) if (mat[j] != 0 and not m["is_light"]) else after[j]
        states[:, k] = s
    return {int(i): (cols[j], states[j]) for j, i in enumerate(idx)}


def chain_by_radiance(oracle, pts, spp, radiance):
    """identity I1: radiance(rays (n, 6), seeds (n,)) -> (rgb, final states) is the existing radiance query at spp = 1; call k
    gets the rays (p_i, d_ik) and the seeds s'_ik.  -> {point index: (colours, states)}"""
    idx = np.flatnonzero(pts.ok)
    p, nrm = pts.points[idx, 0:3], pts.points[idx, 3:6]
    s = np.where(pts.seeds[idx] == 0, 1, pts.seeds[idx]).astype("<u4")
    cols = np.zeros((len(idx), spp, 3), "<f4")
    states = np.zeros((len(idx), spp), "<u4")
    for k in range(spp):
        d, _, after = directions(oracle, nrm, s)
        assert (after != 0).all()
        rgb, fin = radiance(np.concatenate([p, d], axis=1).astype("<f4"), after)
        cols[:, k], s = rgb, np.asarray(fin, "<u4").copy()
        states[:, k] = s
    return {int(i): (cols[j], states[j]) for j, i in enumerate(idx)}


def expected_from(chain, pts, spp):
    """-> (rgb float32[N, 3], final states uint32[N]) at spp samples: the chain's mean inside the domain, NaN and the seed outside"""
    rgb = np.full((len(pts.points), 3), np.nan, "<f4")
    fin = pts.seeds.copy()
    for i, (cols, states) in chain.items():
        rgb[i], fin[i] = rc.mean_of(cols[:spp]), states[spp - 1]
    return rgb, fin


def expected_adaptive(chain, pts, ad):
    """-> (rgb, spp, m2, states): adaptive_cases.cut over the chain; outside the domain NaN, 0, 0 and the seed"""
    n = len(pts.points)
    rgb, spp, m2, fin = np.full((n, 3), np.nan, "<f4"), np.zeros(n, "<u4"), np.zeros(n, "<f4"), pts.seeds.copy()
    for i, (cols, states) in chain.items():
        rgb[i], spp[i], m2[i], fin[i] = ac.cut(cols, states, ad)
    return rgb, spp, m2, fin


def lit_shares(chain):
    """of the points of a chain: the share that is not black, and the share with a sample that adds light and one that does not"""
    lit = np.array([(cols != 0).any(axis=1) for cols, _ in chain.values()])
    return lit.any(axis=1).mean(), (lit.any(axis=1) & ~lit.all(axis=1)).mean()


# ---- tools/host_sim --irradiance, --irradiance-adaptive --------------------------------------------------------------------------
def host_sim_args(d, scene, points, seeds, spp, rr, base=None):
    np.ascontiguousarray(points, "<f4").tofile(os.path.join(d, "points.f32"))
    np.ascontiguousarray(seeds, "<u4").tofile(os.path.join(d, "pseeds.u32"))
    outs = [os.path.join(d, "irr.f32"), os.path.join(d, "irr_states.u32")]
    return ["--irradiance"] + hs.scene_args(scene, base) + [os.path.join(d, "points.f32"), os.path.join(d, "pseeds.u32"), spp, repr(float(rr))] + outs, outs


def host_sim(tool, d, scene, points, seeds, spp, rr, base=None, **kw):
    """-> (rgb (n, 3) float32, final states (n,) uint32, CompletedProcess)"""
    args, outs = host_sim_args(str(d), scene, points, seeds, spp, rr, base)
    r = hs.run(tool, args, **kw)
    return np.fromfile(outs[0], "<f4").reshape(-1, 3), np.fromfile(outs[1], "<u4"), r


def host_sim_adaptive(tool, d, scene, points, seeds, ad, rr, base=None, **kw):
    """-> ((rgb, spp, m2, final states), CompletedProcess)"""
    d = str(d)
    np.ascontiguousarray(points, "<f4").tofile(os.path.join(d, "points.f32"))
    np.ascontiguousarray(seeds, "<u4").tofile(os.path.join(d, "pseeds.u32"))
    outs = [os.path.join(d, f) for f in ("irr_ad.f32", "irr_spp.u32", "irr_m2.f32", "irr_ad_states.u32")]
    r = hs.run(tool, ["--irradiance-adaptive"] + hs.scene_args(scene, base) +
               [os.path.join(d, "points.f32"), os.path.join(d, "pseeds.u32"), ad.min_spp, ad.max_spp, ad.check_every, ac._bits(ad.tolerance),
                ac._bits(ad.floor), repr(float(rr))] + outs, **kw)
    return (np.fromfile(outs[0], "<f4").reshape(-1, 3), np.fromfile(outs[1], "<u4"), np.fromfile(outs[2], "<f4"), np.fromfile(outs[3], "<u4")), r
