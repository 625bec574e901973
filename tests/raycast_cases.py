"""Hostile rays for the closest-hit queries (test infrastructure, next to unit_cases.py).

A render only casts rays it makes itself: finite, unit length, from inside the scene.  A caller of ort_raycast can
send any 24 bytes.  This module makes, from a scene's flattened arrays (api.Scene.flatten), the rays at which the
device's fast tree, its box tests and its routing to the exact walk (raycast_needs_exact, ort_lane.h) are most likely
to part from the reference's raycast_top_most_node.  Five categories:

  nonfinite   one component of o or d set to qNaN, to a negative NaN with a payload, to +inf or to -inf; all-NaN
              origins; all-inf directions
  zero        d = (+-0, +-0, +-0), and single-axis directions whose other two components are +-0, cast from free space,
              from inside shapes and from surface points (a first cast's o + t d)
  magnitude   |d| from 1.4e-45 through 1e-20 and 1e-3, and from 1e18 across the |d|^2 overflow edge up to 3e38;
              single subnormal components
  grazing     an origin coordinate exactly on a box's face, a cylinder's end point or a mesh vertex's coordinate, or one
              ulp either side, with the direction's component on that axis +0 or -0
  far         origins 1e3 - 1e9 away, aimed at shape centres; origins with one coordinate at +-FLT_MAX

  cases(flat, cast, seed=0, scale=1) -> (rays (n, 6) float32, category index per ray)

`cast(rays) -> t` is the closest-hit distance of any reference-exact implementation (the oracle, the reference): it
places the surface points.  Seeded numpy, float32 throughout: the same call gives the same rays on every machine.
scale = 1 gives 1 512 rays per scene (the goldens, tests/golden/raycast_edges_<scene>.npz); a larger scale draws
proportionally more of each kind.
"""
import zlib

import numpy as np

F32 = np.float32
FLT_MAX = F32(3.4028235e38)
CATEGORIES = ["nonfinite", "zero", "magnitude", "grazing", "far"]
QNAN = np.array([0x7FC00000], "<u4").view("<f4")[0]
NEG_NAN = np.array([0xFFC1A5E3], "<u4").view("<f4")[0]  # sign set, quiet, a payload
POS_ZERO, NEG_ZERO = F32(0.0), F32(-0.0)
# |d| for the magnitude category: the smallest subnormal up to 1e-3, then around and past the |d|^2 overflow edge
# (|d|^2 = inf from |d| ~ 1.8447e19)
SMALL_LENGTHS = [1.4e-45, 1e-44, 1e-42, 1e-39, 1.1754942e-38, 1e-30, 1e-23, 1e-20, 1e-10, 1e-3]
LARGE_LENGTHS = [1e18, 1e19, 1.8e19, 1.8446743e19, 1.8446746e19, 1.85e19, 1.9e19, 1e20, 1e30, 3e38]
SUBNORMALS = [1.4e-45, -1.4e-45, 1e-42, -1e-41, 1.1754942e-38, -5e-39]
FAR = [1e3, 3e4, 1e6, 5e7, 1e9]


def f32(a):
    return np.asarray(a, dtype=F32)


def _unit(v):
    v = np.asarray(v, np.float64)
    n = np.linalg.norm(v, axis=-1, keepdims=True)
    n[n == 0] = 1
    return (v / n).astype(F32)


def scene_bounds(flat):
    """the box of every shape (spheres and cylinder ends +- r, boxes, mesh boxes) and the camera, in float32"""
    pts = [f32(flat.camera[0]).reshape(1, 3)]
    for s in flat.spheres:
        pts += [f32(s["center"]) - abs(s["r"]), f32(s["center"]) + abs(s["r"])]
    for b in flat.boxes:
        pts += [f32(b["min"]), f32(b["max"])]
    for c in flat.cylinders:
        for p in (f32(c["base"]), f32(c["base"]) + f32(c["axis"])):
            pts += [p - abs(c["r"]), p + abs(c["r"])]
    for m in flat.meshes:
        pts += [f32(m["aabb_min"]), f32(m["aabb_max"])]
    pts = np.concatenate([f32(p).reshape(-1, 3) for p in pts])
    return pts.min(axis=0), pts.max(axis=0)


def centres(flat):
    """a point inside (or at) every shape: sphere centres, box centres, cylinder mid-points, mesh vertices"""
    out = [f32(flat.spheres["center"]).reshape(-1, 3),
           ((f32(flat.boxes["min"]) + f32(flat.boxes["max"])) * F32(0.5)).reshape(-1, 3),
           (f32(flat.cylinders["base"]) + f32(flat.cylinders["axis"]) * F32(0.5)).reshape(-1, 3)]
    for m in flat.meshes:
        v = f32(m["vertices"])
        out.append(v[:: max(1, len(v) // 64)])
    return np.concatenate(out)


def _aimed(rng, flat, n):
    """n ordinary rays: origins within the scene's box, unit directions at shape centres (most of them hit)"""
    lo, hi = scene_bounds(flat)
    pad = (hi - lo) * F32(0.05)
    o = (lo + pad + (hi - lo - 2 * pad) * rng.uniform(0, 1, (n, 3))).astype(F32)
    c = centres(flat)
    t = c[rng.integers(0, len(c), n)]
    d = _unit(t.astype(np.float64) - o)
    bad = ~(np.abs(d).sum(axis=1) > 0)
    d[bad] = (1, 0, 0)
    return o, d


def _nonfinite(rng, flat, k):
    o, d = _aimed(rng, flat, 6 * k)
    rays = np.concatenate([o, d], axis=1)
    vals = f32([QNAN, NEG_NAN, np.inf, -np.inf])
    out = []
    for comp in range(6):
        for v in vals:
            r = rays[rng.integers(0, len(rays), k)].copy()
            r[:, comp] = v
            out.append(r)
    r = rays[rng.integers(0, len(rays), 2 * k)].copy()  # all-NaN origins, both NaN kinds
    r[:, 0:3] = np.where(rng.integers(0, 2, (len(r), 1)) == 1, NEG_NAN, QNAN)
    out.append(r)
    r = rays[rng.integers(0, len(rays), 2 * k)].copy()  # all-inf directions, every sign pattern
    r[:, 3:6] = np.where(rng.integers(0, 2, (len(r), 3)) == 1, F32(np.inf), F32(-np.inf))
    out.append(r)
    return np.concatenate(out)


def _surface_points(rng, flat, cast, n):
    o, d = _aimed(rng, flat, 2 * n)
    t = f32(cast(np.concatenate([o, d], axis=1)))
    hit = t < FLT_MAX
    p = (o[hit] + t[hit, None] * d[hit]).astype(F32)  # float32 arithmetic, rounded per operation
    return p[:n]


def _zero_dirs(rng, n):
    """+-0 in all three components (every sign pattern), or one non-zero axis with +-0 in the other two"""
    signs = rng.integers(0, 2, (n, 3)) == 1
    d = np.where(signs, NEG_ZERO, POS_ZERO).astype(F32)
    single = rng.random(n) < 0.6
    axis = rng.integers(0, 3, n)
    mag = f32([1.0, 0.5, 2.0, 1e-3, 37.5])[rng.integers(0, 5, n)] * np.where(rng.random(n) < 0.5, F32(-1), F32(1))
    rows = np.flatnonzero(single)
    d[rows, axis[rows]] = mag[rows]
    # the eight sign patterns of (+-0, +-0, +-0) at least once each
    for i in range(min(8, n)):
        d[i] = [NEG_ZERO if (i >> b) & 1 else POS_ZERO for b in range(3)]
    return d


def _zero(rng, flat, cast, k):
    lo, hi = scene_bounds(flat)
    free = (lo + (hi - lo) * rng.uniform(0, 1, (3 * k, 3))).astype(F32)
    c = centres(flat)
    inside = c[rng.integers(0, len(c), 3 * k)]
    surf = _surface_points(rng, flat, cast, 3 * k)
    o = np.concatenate([free, inside, surf]).astype(F32)
    return np.concatenate([o, _zero_dirs(rng, len(o))], axis=1)


def _magnitude(rng, flat, k):
    out = []
    for L in SMALL_LENGTHS + LARGE_LENGTHS:
        o, d = _aimed(rng, flat, k)
        out.append(np.concatenate([o, (d.astype(np.float64) * L).astype(F32)], axis=1))
    # one subnormal component; the others of an axis-aligned or a general unit direction
    o, d = _aimed(rng, flat, 6 * k)
    axis = rng.integers(0, 3, len(d))
    half = rng.random(len(d)) < 0.5
    d[half] = np.eye(3, dtype=F32)[axis[half]] * np.where(rng.random((int(half.sum()), 1)) < 0.5, F32(-1), F32(1))
    which = (axis + 1 + rng.integers(0, 2, len(d))) % 3
    d[np.arange(len(d)), which] = f32(SUBNORMALS)[rng.integers(0, len(SUBNORMALS), len(d))]
    out.append(np.concatenate([o, d], axis=1))
    return np.concatenate(out).astype(F32)


def _planes(flat):
    """(axis, coordinate) pairs a ray can graze: box faces, cylinder ends, mesh vertex coordinates"""
    out = []
    for b in flat.boxes:
        for a in range(3):
            out += [(a, f32(b["min"])[a]), (a, f32(b["max"])[a])]
    for c in flat.cylinders:
        a = int(np.argmax(np.abs(f32(c["axis"]))))
        out += [(a, f32(c["base"])[a]), (a, (f32(c["base"]) + f32(c["axis"]))[a])]
    for m in flat.meshes:
        v = f32(m["vertices"])
        for row in v[:: max(1, len(v) // 24)]:
            out += [(a, row[a]) for a in range(3)]
    return out


def _grazing(rng, flat, k):
    planes = _planes(flat)
    lo, hi = scene_bounds(flat)
    c = centres(flat)
    n = 30 * k
    pick = rng.integers(0, len(planes), n)
    o = (lo + (hi - lo) * rng.uniform(0, 1, (n, 3))).astype(F32)
    t = c[rng.integers(0, len(c), n)]
    step = rng.integers(-1, 2, n)  # on the plane, or one ulp below / above it
    axes = np.zeros(n, int)
    for i in range(n):
        a, v = planes[pick[i]]
        axes[i] = a
        o[i, a] = v if step[i] == 0 else np.nextafter(v, F32(np.inf) if step[i] > 0 else F32(-np.inf))
    d = (t.astype(np.float64) - o)
    d[np.arange(n), axes] = 0
    d = _unit(d)
    flat_dir = ~(np.abs(d).sum(axis=1) > 0)
    d[flat_dir, (axes[flat_dir] + 1) % 3] = 1
    d[np.arange(n), axes] = np.where(rng.random(n) < 0.5, NEG_ZERO, POS_ZERO)
    return np.concatenate([o, d], axis=1).astype(F32)


def _far(rng, flat, k):
    c = centres(flat)
    n = 20 * k
    t = c[rng.integers(0, len(c), n)]
    u = _unit(rng.normal(size=(n, 3)))
    dist = f32(FAR)[rng.integers(0, len(FAR), n)] * f32(rng.uniform(1, 3, n))
    o = (t + u * dist[:, None]).astype(F32)
    d = _unit(t.astype(np.float64) - o.astype(np.float64))
    rays = [np.concatenate([o, d], axis=1)]
    # one coordinate at +-FLT_MAX, the others at a shape centre, pointing back (or slightly off)
    m = 4 * k
    t = c[rng.integers(0, len(c), m)]
    axis = rng.integers(0, 3, m)
    sign = np.where(rng.random(m) < 0.5, F32(-1), F32(1))
    o = t.copy()
    o[np.arange(m), axis] = sign * FLT_MAX
    d = np.zeros((m, 3), F32)
    d[np.arange(m), axis] = -sign
    off = rng.random(m) < 0.5
    d[off] = _unit(d[off] + rng.normal(size=(int(off.sum()), 3)) * 1e-3)
    rays.append(np.concatenate([o, d], axis=1))
    return np.concatenate(rays).astype(F32)


def cases(flat, cast, seed=0, scale=1):
    """(rays, category) for one scene: 1 512 * scale rays, CATEGORIES[category[i]] names ray i's kind"""
    rng = np.random.default_rng(20261016 + seed)
    k = 12 * scale
    with np.errstate(all="ignore"):
        parts = [_nonfinite(rng, flat, k), _zero(rng, flat, cast, 2 * k), _magnitude(rng, flat, k),
                 _grazing(rng, flat, k), _far(rng, flat, k)]
    rays = np.concatenate(parts).astype("<f4")
    cat = np.repeat(np.arange(len(parts)), [len(p) for p in parts]).astype(np.int32)
    return np.ascontiguousarray(rays), cat


# ---- comparing answers: NaN by position ----------------------------------------------------------------------------
CANON_NAN = np.uint32(0x7FC00000)


def canonical_bits(a):
    """float32 bits with every NaN mapped to one pattern (x86 and gfx950 make different default NaNs; which NaN is not
    part of the contract, where one is)"""
    a = np.ascontiguousarray(a, dtype="<f4")
    return np.where(np.isnan(a), CANON_NAN, a.view("<u4"))


def assert_same_answers(t, n, mat, want_t, want_n, want_mat, what):
    """t, normal and material equal bit for bit, a NaN anywhere equal to a NaN at the same place"""
    for got, want, field in ((t, want_t, "t"), (n, want_n, "normal")):
        g, w = canonical_bits(got), canonical_bits(want)
        assert g.shape == w.shape, "%s %s: shape %s vs %s" % (what, field, g.shape, w.shape)
        ne = g != w
        if ne.any():
            idx = np.argwhere(ne)[0]
            raise AssertionError("%s %s: %d of %d values differ; first at %s: %r vs %r"
                                 % (what, field, int(ne.sum()), ne.size, tuple(idx), np.float32(got[tuple(idx)]),
                                    np.float32(want[tuple(idx)])))
    bad = np.flatnonzero(np.asarray(mat) != np.asarray(want_mat))
    assert len(bad) == 0, "%s: material differs for %d rays, first %d: %d vs %d" % (what, len(bad), bad[0], mat[bad[0]], want_mat[bad[0]])


# ---- ordinary rays at scale (the GPU tests and tests/test_query_lanes_host.py draw the same ones) ----------------------
def unit_vectors(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype("<f4")


def golden_like(rng, n):
    """the goldens' distribution (tests/golden/make_golden.py): origins in and around the room, uniform directions"""
    o = np.stack([rng.uniform(-2.5, 14.5, n), rng.uniform(-2.5, 14.5, n), rng.uniform(0.05, 8.8, n)], axis=1)
    h = n // 2
    o[:h] = np.stack([rng.uniform(-1.5, 1.5, h), rng.uniform(-1.8, 1.5, h), rng.uniform(0.05, 2.5, h)], axis=1)
    return np.concatenate([o.astype("<f4"), unit_vectors(rng, n)], axis=1)


def mixed_rays(cast, name, n):
    """the four kinds of ray, n in all: golden distribution, rays that start on a surface (a first cast's o + t d, new
    directions), axis-aligned / zero-component / non-unit directions, rays from outside that miss.  cast(rays) -> t is the first
    cast: the device's in the GPU tests, the oracle's where there is no device"""
    rng = np.random.default_rng(zlib.crc32(("mixed " + name).encode()))
    q = n // 4
    a = golden_like(rng, q)
    first_t = np.asarray(cast(golden_like(rng, 2 * q)), "<f4")
    base = golden_like(rng, 2 * q)
    hit = first_t < FLT_MAX
    o = base[hit, 0:3] + first_t[hit, None] * base[hit, 3:6]  # float32 arithmetic, rounded per operation
    o = o[:q].astype("<f4")
    b = np.concatenate([o, unit_vectors(rng, len(o))], axis=1)
    # axis-aligned and zero-component directions, non-unit lengths
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],
                     [1, 1, 0], [0, -1, 1], [1, 0, -1], [-1, 1, 1]], "<f4")
    d = axes[rng.integers(0, len(axes), q)] * rng.choice(np.array([1e-3, 0.1, 0.5, 1, 2, 37.5], "<f4"), q)[:, None]
    mix = rng.random(q) < 0.3  # some non-unit random directions too
    d[mix] = unit_vectors(rng, int(mix.sum())) * rng.uniform(0.01, 50, int(mix.sum()))[:, None].astype("<f4")
    c = np.concatenate([golden_like(rng, q)[:, 0:3], d.astype("<f4")], axis=1)
    # from far outside, pointing away from the scene
    u = unit_vectors(rng, n - 3 * q)
    e = np.concatenate([(u * np.float32(1000.0) + np.float32(6.0)).astype("<f4"), u * rng.uniform(0.5, 2, len(u))[:, None].astype("<f4")], axis=1)
    rays = np.concatenate([a, b, c, e]).astype("<f4")
    kinds = np.repeat(np.arange(4), [len(a), len(b), len(c), len(e)])
    return rays, kinds


# ---- rays at the exact walk's thresholds (raycast_needs_exact, ort_lane.h): shared by the GPU and the host-lane tests -------
LEN2 = [np.float32(0.998), np.nextafter(np.float32(0.999), np.float32(0)), np.float32(0.999),
        np.nextafter(np.float32(0.999), np.float32(2)), np.float32(0.9995), np.float32(1 - 2.0 ** -24), np.float32(1),
        np.float32(1.01)]


def threshold_scene(api, small):
    """small = False: a room (six slabs), 30 spheres (r 0, 1e-3, 2e-3 and 0.05 among them) and four cylinders;
    small = True: a handful of the same shapes within a box of diagonal < 1, so that the boxes' scene-size slack is
    at its least"""
    rng = np.random.default_rng(424242 + small)
    mats = np.zeros(4, api.MATERIAL_DTYPE)
    mats["diffuse"][1] = (0.7, 0.7, 0.7)
    mats["specular"][2, :3] = 1
    mats["transmission"][3] = 1; mats["ior"][1:] = (1.0, 1.0, 1.4)
    tiny = [0.0, 1e-3, 2e-3, 0.05]
    if small:
        sph = np.zeros(8, api.SPHERE_DTYPE)
        for i in range(8):
            sph[i] = (rng.uniform(0.1, 0.4, 3), tiny[i % 4] if i < 6 else 0.03, 1 + i % 3)
        cyl = np.zeros(2, api.CYLINDER_DTYPE)
        cyl[0] = ((0.05, 0.05, 0.05), (0, 0, 0.3), 0.02, 1)
        cyl[1] = ((0.45, 0.1, 0.2), (-0.1, 0.2, 0.05), 1e-3, 2)
        box = np.zeros(1, api.BOX_DTYPE)
        box[0] = ((0.2, 0.3, 0.0), (0.3, 0.35, 0.08), 1)
        cam = (0.25, 0.0, 0.25)
    else:
        sph = np.zeros(30, api.SPHERE_DTYPE)
        for i in range(30):
            r = tiny[i % 4] if i < 16 else rng.uniform(0.1, 0.8)
            sph[i] = (rng.uniform(-3, 3, 3) * (1, 1, 0) + (0, 0, rng.uniform(0.3, 4)), r, 1 + i % 3)
        cyl = np.zeros(4, api.CYLINDER_DTYPE)
        for i in range(4):
            cyl[i] = (rng.uniform(-2.5, 2.5, 3) * (1, 1, 0) + (0, 0, 0.5), (0, 0, 1.5) if i == 0 else rng.normal(size=3),
                      (0.2, 1e-3, 0.05, 0.3)[i], 1 + i % 3)
        box = np.zeros(6, api.BOX_DTYPE)
        room = [((-4, -4, -0.2), (4, 4, 0)), ((-4, -4, 5), (4, 4, 5.2)), ((-4.2, -4, -0.2), (-4, 4, 5.2)),
                ((4, -4, -0.2), (4.2, 4, 5.2)), ((-4, -4.2, -0.2), (4, -4, 5.2)), ((-4, 4, -0.2), (4, 4.2, 5.2))]
        for i, (lo, hi) in enumerate(room):
            box[i] = (lo, hi, 1)
        cam = (3.3, 2.0, 2.6)
    return api.Scene.from_arrays(mats, sph, box, cyl, None, camera_p=cam, camera_height_ratio=0.3, screen=(64, 48))


def scene_box(flat, cam):
    """the box ort_kernels.hip (the query tables, "the box of everything ort_tree.cpp sized the quadric boxes for")
    computes, in f32: the camera, spheres and cylinder ends +- |r|, box corners"""
    lo = np.array(cam, "<f4").copy()
    hi = lo.copy()

    def grow(p, r):
        p = np.asarray(p, "<f4")
        r = np.float32(abs(r))
        np.minimum(lo, p - r, out=lo)
        np.maximum(hi, p + r, out=hi)
    for s in flat.spheres:
        grow(s["center"], s["r"])
    for b in flat.boxes:
        grow(b["min"], 0)
        grow(b["max"], 0)
    for c in flat.cylinders:
        grow(c["base"], c["r"])
        grow(np.asarray(c["base"], "<f4") + np.asarray(c["axis"], "<f4"), c["r"])
    return lo, hi


def _dir_of_len2(u, target):
    """a multiple of the unit vector u whose |d|^2, summed in f32 as the kernel does, is target (or the nearest)"""
    s = np.float32(np.sqrt(np.float64(target)))
    best = None
    for k in range(-6, 7):
        sk = s
        for _ in range(abs(k)):
            sk = np.nextafter(sk, np.float32(np.inf if k > 0 else 0))
        d = (u * sk).astype("<f4")
        l2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        err = abs(float(l2) - float(target))
        if best is None or err < best[0]:
            best = (err, d)
        if err == 0:
            break
    return best[1]


def threshold_rays(flat, cam, rng, dists):
    rays = []
    axes = np.eye(3, dtype="<f4")
    for s in flat.spheres:
        c, r = np.asarray(s["center"], "<f4"), float(s["r"])
        for l2 in LEN2:
            for j in range(3):
                u = [axes[j], -axes[j], (axes[j] + axes[(j + 1) % 3] * 0.37) / np.float32(np.linalg.norm([1, 0.37]))][j].astype("<f4")
                w = np.cross(u, axes[(j + 2) % 3]).astype("<f4")
                w /= np.float32(np.linalg.norm(w))
                d = _dir_of_len2(u, l2)
                # perpendicular offsets across both edges of the tangent band: D^2 = r^2 +- 1e-5 / |d|^2
                offs = []
                for sign in (1, -1):
                    e2 = r * r + sign * 1e-5 / float(l2)
                    if e2 > 0:
                        D = np.sqrt(e2)
                        offs += [D * (1 + k * 2e-7) for k in range(-6, 7)] + [D * (1 + k * 1e-5) for k in (-3, -1, 1, 3)]
                offs += [r, 0.5 * r]
                for D in offs:
                    for L in dists:
                        o = (c - np.float32(L) * u + np.float32(D) * w).astype("<f4")
                        rays.append(np.concatenate([o, d]))
    # origins exactly on the faces of the scene box, one ulp inside and outside, pointed at the shapes
    lo, hi = scene_box(flat, cam)
    targets = np.concatenate([np.asarray(flat.spheres["center"], "<f4"), np.asarray(flat.cylinders["base"], "<f4")])
    for k in range(3):
        for face in (lo[k], hi[k]):
            for step in (None, 0, np.inf):
                for _ in range(24):
                    o = (lo + (hi - lo) * rng.uniform(0, 1, 3).astype("<f4")).astype("<f4")
                    o[k] = face if step is None else np.nextafter(face, np.float32(step) if step else np.float32(-np.inf))
                    t = targets[rng.integers(0, len(targets))]
                    u = (t - o).astype(np.float64)
                    n = np.linalg.norm(u)
                    u = (u / n if n > 0 else np.array([1.0, 0, 0])).astype("<f4")
                    rays.append(np.concatenate([o, _dir_of_len2(u, LEN2[rng.integers(0, len(LEN2))])]))
        # on an edge and a corner of the box
        rays.append(np.concatenate([lo, _dir_of_len2(np.full(3, 1 / np.sqrt(3), "<f4"), 1)]))
        rays.append(np.concatenate([hi, _dir_of_len2(np.full(3, -1 / np.sqrt(3), "<f4"), 0.999)]))
    return np.array(rays, "<f4")


def needs_exact(rays, lo, hi, tree_spheres, tree_quadrics):
    """raycastneeds_exact (ort_lane.h) restated in f32"""
    d = rays[:, 3:6]
    l2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    o = rays[:, 0:3]
    inside = ((o >= lo) & (o <= hi)).all(axis=1)
    short = ~(l2 >= np.float32(0.999 if tree_spheres else 1e-30))
    return (tree_quadrics & short) | (tree_quadrics & ~inside)
