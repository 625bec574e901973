"""Radiance queries (ort_radiance) against the oracle as it stands: the rays, and what they must give.

oracle_tiled_raytrace with a pinhole camera (x_axis = y_axis = 0) traces every sample of its one pixel from one fixed point in
one fixed direction: ap = p - 0.1 z and dir0 = normalize(focal - ap), whatever aperture angle it draws.  That draw costs the
stream two steps (rng_between), so a sample of a radiance query that starts with state s is the oracle's spp = 1 call with
state unstep(unstep(s)), and an spp = n query is n such calls chained through the returned state.  pinhole() restates the
oracle's arithmetic for ap and dir0 in numpy float32, operation by operation, so that the ray handed to the device is the
oracle's primary ray bit for bit (tests/test_radiance_host.py pins that)."""
import zlib

import numpy as np

F = np.float32


# ---- the xorshift step (random.h:5-12: << 13, >> 17, >> 5) and its inverse ---------------------------------------------------
def step(x):
    x &= 0xFFFFFFFF
    x ^= (x << 13) & 0xFFFFFFFF
    x ^= x >> 17
    x ^= x >> 5
    return x


def unstep(x):
    x &= 0xFFFFFFFF
    for shift, left in ((5, False), (17, False), (13, True)):
        r = x
        for _ in range(32 // shift + 1):
            r = x ^ (((r << shift) & 0xFFFFFFFF) if left else (r >> shift))
        x = r
    return x


# ---- the oracle's primary ray of a pinhole camera ----------------------------------------------------------------------------
def _len(a):
    return np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])   # v_len: left to right, f32 per operation


def _normalize(a):
    l = _len(a)
    d = l - F(0)
    if not (d >= F(-0.000001) and d < F(0.000001)):            # o_ceq(l, 0)
        return np.array([a[0] / l, a[1] / l, a[2] / l], "<f4")
    return np.zeros(3, "<f4")


def pinhole(p, z):
    """camera [p, 0, 0, z] on a 1 x 1 image -> (o, d) float32[3]: the origin and direction of every sample's primary ray, in
    the oracle's own order of operations (oracle_tiled_raytrace: focal_length, to_pixel, focal, ap, dir0).  p must have no
    zero component (p + (+-0) is then p whatever the aperture angle's sign)."""
    p = np.asarray(p, "<f4")
    z = np.asarray(z, "<f4")
    assert (p != 0).all()
    with np.errstate(all="ignore"):
        fl = _len(np.array([p[0] - F(0), p[1] - F(0), p[2] - F(0.2)], "<f4"))
        t = np.array([(F(-0.0) + F(-0.0)) - z[k] for k in range(3)], "<f4")          # px X + py Y - Z with X = Y = 0, px = py = -1
        to_pixel = _normalize(t)
        focal = np.array([p[k] + fl * to_pixel[k] for k in range(3)], "<f4")
        ap = np.array([p[k] - F(0.1) * z[k] for k in range(3)], "<f4")
        d = _normalize(np.array([focal[k] - ap[k] for k in range(3)], "<f4"))
    return ap, d


def camera_of(p, z):
    return np.array([p, [0, 0, 0], [0, 0, 0], z], "<f4")


# ---- what a query must give ----------------------------------------------------------------------------------------------------
def sample_chain(osc, p, z, seed, spp, rr):
    """-> (colours float32[spp, 3], states after each sample): spp chained spp = 1 calls of the oracle on one stream"""
    osc.set_camera(camera_of(p, z))
    s = (int(seed) & 0xFFFFFFFF) or 1
    cols = np.zeros((spp, 3), "<f4")
    states = []
    img = np.zeros((1, 1, 3), "<f4")
    for k in range(spp):
        _, s = osc.tiled_raytrace(img, 0, 0, 1, 1, unstep(unstep(s)), 1, rr)
        cols[k] = img[0, 0]
        states.append(s)
    return cols, states


def mean_of(cols):
    """the samples' colours summed in float32 in sample order, divided by float32(spp)"""
    acc = np.zeros(3, "<f4")
    for c in cols:
        acc = (acc + c).astype("<f4")
    return (acc / F(len(cols))).astype("<f4")


def expected(osc, cams, seeds, spp, rr):
    """cams: (N, 2, 3) p, z.  -> (rgb float32[N, 3], final states uint32[N])"""
    rgb = np.zeros((len(cams), 3), "<f4")
    fin = np.zeros(len(cams), "<u4")
    for i, (p, z) in enumerate(cams):
        cols, states = sample_chain(osc, p, z, seeds[i], spp, rr)
        rgb[i] = mean_of(cols)
        fin[i] = states[-1]
    return rgb, fin


def expected_prefixes(osc, cams, seeds, spps, rr):
    """the same for several sample counts at once (one chain of max(spps) samples per ray): {spp: (rgb, final states)}"""
    out = {n: (np.zeros((len(cams), 3), "<f4"), np.zeros(len(cams), "<u4")) for n in spps}
    for i, (p, z) in enumerate(cams):
        cols, states = sample_chain(osc, p, z, seeds[i], max(spps), rr)
        for n in spps:
            out[n][0][i] = mean_of(cols[:n])
            out[n][1][i] = states[n - 1]
    return out


# ---- generators: cameras (N, 2, 3) of p, z --------------------------------------------------------------------------------------
def origin_box(flat):
    """the box of every shape and the scene's own camera_p (what the tree was built for), from Scene.flatten's arrays"""
    pts = [np.asarray(flat.camera[0], "<f4")[None, :]]
    r = np.abs(flat.spheres["r"])[:, None]
    pts += [flat.spheres["center"] - r, flat.spheres["center"] + r, flat.boxes["min"], flat.boxes["max"]]
    r = np.abs(flat.cylinders["r"])[:, None]
    for end in (flat.cylinders["base"], flat.cylinders["base"] + flat.cylinders["axis"]):
        pts += [end - r, end + r]
    pts += [np.asarray(m["vertices"], "<f4").reshape(-1, 3) for m in flat.meshes]
    pts = np.concatenate([np.asarray(q, "<f4").reshape(-1, 3) for q in pts])
    return pts.min(axis=0), pts.max(axis=0)


def _units(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype("<f4")


def _nonzero(p):
    p = np.asarray(p, "<f4").copy()
    p[p == 0] = F(1e-3)
    return p


def inside(rng, lo, hi, n, margin=0.15):
    """random pinholes whose aperture point lies inside the origin box"""
    span = hi - lo
    p = rng.uniform(lo + margin * span + 0.1, hi - margin * span - 0.1, size=(n, 3)).astype("<f4")
    return np.stack([_nonzero(p), _units(rng, n)], axis=1)


def at_lights(rng, flat, lo, hi, n):
    """pinholes inside the box that look at a light (its centre, jittered by a tenth of the box): most see it directly, which
    is what keeps a set of rays from being black in a room whose lights are small"""
    cams = inside(rng, lo, hi, n)
    centres = []
    for kind, index in zip(flat.lights["type"], flat.lights["index"]):
        if kind == 1:
            centres.append(flat.spheres["center"][index])
        else:
            centres.append(flat.cylinders["base"][index] + F(0.5) * flat.cylinders["axis"][index])
    if not centres:
        return cams
    centres = np.asarray(centres, "<f4")
    target = centres[rng.integers(0, len(centres), n)] + rng.normal(size=(n, 3)) * 0.03 * (hi - lo)
    z = cams[:, 0] - target
    cams[:, 1] = (z / np.linalg.norm(z, axis=1, keepdims=True)).astype("<f4")
    return cams


AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], "<f4")


def axis_aligned(rng, lo, hi, n):
    """z = +-x, +-y, +-z: a direction with two zero components"""
    cams = inside(rng, lo, hi, n)
    cams[:, 1] = AXES[np.arange(n) % 6]
    return cams


def outside(rng, lo, hi, n):
    """origins 1 to 3 box diagonals outside the box, looking at a point inside it"""
    centre, diag = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    p = (centre + _units(rng, n) * (diag * rng.uniform(1.0, 3.0, size=(n, 1)) + diag / 2)).astype("<f4")
    target = rng.uniform(lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo), size=(n, 3))
    z = p - target
    z = (z / np.linalg.norm(z, axis=1, keepdims=True)).astype("<f4")
    return np.stack([_nonzero(p), z], axis=1)


def probes(rng, osc, lo, hi, n):
    """rays that start 1e-3 above a surface found with oracle.raycast, into the hemisphere of its normal"""
    out = []
    while len(out) < n:
        c = inside(rng, lo, hi, 2 * n)
        od = [pinhole(p, z) for p, z in c]
        t, nrm, mat = osc.raycast(np.array([o for o, _ in od]), np.array([d for _, d in od]))
        for (o, d), ti, ni, mi in zip(od, t, nrm, mat):
            if mi == 0 or len(out) >= n:
                continue
            nn = ni if np.dot(ni, d) < 0 else -ni      # the side the ray came from
            start = o + ti * d + F(1e-3) * nn
            u = _units(rng, 1)[0]
            if np.dot(u, nn) < 0:
                u = -u
            z = -u
            out.append(np.stack([_nonzero(start + F(0.1) * z), z]))
    return np.array(out, "<f4")


def out_of_domain(rng, lo, hi, n):
    """-> (n, 6) rays outside the per-ray domain: a NaN or infinite component, |d| = 0, 0.5, 2"""
    rays = np.zeros((n, 6), "<f4")
    for i, (p, z) in enumerate(inside(rng, lo, hi, n)):
        o, d = pinhole(p, z)
        kind = i % 6
        if kind == 0:
            d = d * F(0)
        elif kind == 1:
            d = d * F(0.5)
        elif kind == 2:
            d = d * F(2)
        elif kind == 3:
            d[i % 3] = F(np.nan)
        elif kind == 4:
            o[i % 3] = F(np.inf) if i % 2 else F(-np.inf)
        else:
            o[(i // 6) % 3] = F(np.nan)
        rays[i, 0:3], rays[i, 3:6] = o, d
    return rays


class Cases:
    """rays (N, 6), seeds (N,), cams (N, 2, 3) (rows of out-of-domain rays unused), ok (N,) bool: inside the domain"""

    def __init__(self, rays, seeds, cams, ok):
        self.rays, self.seeds, self.cams, self.ok = rays, seeds, cams, ok

    def take(self, idx):
        return Cases(self.rays[idx], self.seeds[idx], self.cams[idx], self.ok[idx])


def mixed(name, flat, osc, n, bad=8, salt=""):
    """n rays mixing all generators, shuffled: three eighths anywhere inside the box, a quarter inside it looking at a light,
    the rest axis-aligned, from outside and probes, and `bad` rays outside the domain.  Seeds are arbitrary 32-bit words (job_seed of the ray's number), one of them 0."""
    rng = np.random.default_rng(zlib.crc32(("radiance " + name + salt).encode()))
    lo, hi = origin_box(flat)
    good = n - bad
    k = good // 8
    cams = np.concatenate([inside(rng, lo, hi, good - 7 * k), at_lights(rng, flat, lo, hi, 2 * k), axis_aligned(rng, lo, hi, k),
                           outside(rng, lo, hi, k), probes(rng, osc, lo, hi, 3 * k)])
    rays = np.zeros((n, 6), "<f4")
    for i, (p, z) in enumerate(cams):
        rays[i, 0:3], rays[i, 3:6] = pinhole(p, z)
    rays[good:] = out_of_domain(rng, lo, hi, bad)
    cams = np.concatenate([cams, np.ones((bad, 2, 3), "<f4")])
    ok = np.arange(n) < good
    seeds = rng.integers(1, 1 << 32, size=n, dtype=np.uint64).astype("<u4")
    perm = rng.permutation(n)
    return Cases(rays[perm], seeds[perm], cams[perm], ok[perm])


def expected_of(osc, cases, spps, rr):
    """{spp: (rgb, states)} for all rays of a case set: the oracle's values inside the domain, NaN and the seed outside"""
    idx = np.flatnonzero(cases.ok)
    part = expected_prefixes(osc, cases.cams[idx], cases.seeds[idx], spps, rr)
    out = {}
    for n in spps:
        rgb = np.full((len(cases.rays), 3), np.nan, "<f4")
        fin = cases.seeds.copy()
        rgb[idx], fin[idx] = part[n]
        out[n] = (rgb, fin)
    return out


def assert_same(rgb, states, want_rgb, want_states, what):
    """all bits; NaN outputs compare by position"""
    rgb = np.ascontiguousarray(rgb, "<f4")
    nan_w, nan_g = np.isnan(want_rgb), np.isnan(rgb)
    assert (nan_w == nan_g).all(), "%s: NaN in other places: %d vs %d" % (what, nan_g.sum(), nan_w.sum())
    ne = (rgb.view("<u4") != np.ascontiguousarray(want_rgb, "<f4").view("<u4")) & ~nan_w
    if ne.any():
        i = np.argwhere(ne)[0]
        raise AssertionError("%s: %d of %d colour values differ bitwise; first at %s: %r vs %r" % (what, ne.sum(), ne.size, tuple(i), rgb[tuple(i)], want_rgb[tuple(i)]))
    if states is not None:
        bad = np.flatnonzero(np.asarray(states) != np.asarray(want_states))
        assert len(bad) == 0, "%s: %d final states differ, first ray %d: %#x vs %#x" % (what, len(bad), bad[0], states[bad[0]], want_states[bad[0]])


def survives_primary(seeds, states):
    """per ray: its final state differs from the state after one rng_01 draw (a path that ends at its primary hit without a
    roulette draw leaves the seed itself, one that loses the first draw leaves step(seed))"""
    one = np.array([step(int(s) or 1) for s in seeds], "<u4")
    return (np.asarray(states) != one) & (np.asarray(states) != np.where(seeds == 0, 1, seeds))
