"""Adversarial inputs for the per-function parity tests (test infrastructure, next to ref_io.py).

For every op of ort_unit_eval_device (include/ort.h) this module makes a CORNER set -- the inputs at which a restated or
specialised function is most likely to part from the reference: +-0 and NaN slab products, a radicand of exactly 0,
wi = +-wo, normals in the 1e-4 band around +-z, arguments next to quadrant boundaries, roughness other than 0.01,
zero-weight materials -- and a seeded BULK set of realistic inputs.  Seeded numpy, float32 throughout: the same call
gives the same records on every machine.

  corners(op)         -> (n, k) float32 rows, op's input layout
  bulk(op, n, seed)   -> (n, k) float32 rows
  records(op, rows)   -> packed {u32 op; f32 in[24]} records (ref_io.make_unit_records)

Ops 14-19 (the kernels' specialised forms) take the inputs of the generic op they stand in for; GENERIC_OF names it.
The inputs of the box forms and the diffuse forms are filtered to what their callers feed them (finite_box_rows,
diffuse_rows).
"""
import numpy as np

import ref_io

F32 = np.float32
PI = F32(3.14159265358979323846)
TWO_PI = F32(2.0) * PI                      # 2 * kPi in f32, as sample_brdf_draw computes the azimuth's range
# the generic op whose inputs (and answer) a kernel form shares
GENERIC_OF = {14: 3, 15: 6, 16: 6, 17: 5, 18: 5, 19: 9}


def f32(a):
    return np.asarray(a, dtype=F32)


def ulps(x, k):
    """x moved k ulps (k < 0: towards -inf), elementwise, in float32"""
    x = f32(x).copy()
    step = np.inf if k > 0 else -np.inf
    for _ in range(abs(int(k))):
        x = np.nextafter(x, F32(step)).astype(F32)
    return x


def around(x, k):
    """x and its 2k neighbours in float32 (-k .. +k ulps)"""
    return np.concatenate([ulps(x, j).reshape(-1) for j in range(-k, k + 1)])


def records(op, rows):
    return ref_io.make_unit_records(op, rows)


def _unit(v):
    v = f32(v)
    with np.errstate(all="ignore"):
        return (v / np.linalg.norm(v.astype(np.float64), axis=-1, keepdims=True)).astype(F32)


def _rand_unit(rng, n):
    return _unit(rng.normal(size=(n, 3)))


def _pick(rng, pool, n):
    pool = f32(pool)
    return pool[rng.integers(0, len(pool), size=n)]


# ---- f32 restatements (numpy float32 operations are separately rounded, as the path's) ----------------------------
def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize3(v):
    """math.h:298-310 in f32: v / |v| unless |v| is within 1e-6 of 0"""
    v = f32(v)
    with np.errstate(all="ignore"):
        ln = np.sqrt(dot3(v, v)).astype(F32)
        d = ln - F32(0)
        zero = (d >= F32(-1e-6)) & (d < F32(1e-6))
        out = v / ln[..., None]
    out[zero] = 0
    return out.astype(F32)


def mat_weights(kd, ks, kt):
    """make_mat's lobe weights (ort_device.h): |K| / (|Kd| + |Ks| + |Kt|), in f32"""
    with np.errstate(all="ignore"):
        a, b, c = (np.sqrt(dot3(f32(k), f32(k))).astype(F32) for k in (kd, ks, kt))
        s = a + b + c
        return a / s, b / s, c / s


def is_diffuse_material(kd, ks, kt):
    """the upload-time guard of the diffuse kernels (offline_raytracer_amd/csrc/ort_kernels.hip:191-197) in f32: a material
    is diffuse when |Ks|^2 > 0, |Kt|^2 > 0, ps_c > 0 and pt_c > 0 are all false (ps_c, pt_c as make_mat derives them)"""
    ks, kt = f32(ks), f32(kt)
    ks2 = ks[..., 0] * ks[..., 0] + ks[..., 1] * ks[..., 1] + ks[..., 2] * ks[..., 2]
    kt2 = kt[..., 0] * kt[..., 0] + kt[..., 1] * kt[..., 1] + kt[..., 2] * kt[..., 2]
    _, ps_c, pt_c = mat_weights(kd, ks, kt)
    with np.errstate(invalid="ignore"):
        return ~((ks2 > 0) | (kt2 > 0) | (ps_c > 0) | (pt_c > 0))


def radicand(N, wi, wo, ior):
    """ray.cpp:899-933 as eval_scattering / pdf_brdf evaluate it, in f32"""
    N, wi, wo, ior = f32(N), f32(wi), f32(wo), f32(ior)
    front = dot3(N, wo) >= 0
    ni = np.where(front, F32(1), ior).astype(F32)
    no = np.where(front, ior, F32(1)).astype(F32)
    n = ni / no
    m = normalize3(-(ni[..., None] * wi + no[..., None] * wo))
    d = dot3(wo, m)
    return F32(1) - (n * n) * (F32(1) - d * d)


# ---- intersectors -----------------------------------------------------------------------------------------------
def _triangle_corners(rng):
    rows = []
    v0, e1, e2 = f32([0, 0, 0]), f32([1, 0, 0]), f32([0, 1, 0])
    # det = -d.z exactly for e1 = x, e2 = y: det at +-1e-6 and a few ulps either side (ray.cpp:71 rejects |det| < 1e-6)
    for det in around(F32(1e-6), 3).tolist() + around(F32(-1e-6), 3).tolist():
        for p in ([0.25, 0.25], [0.6, 0.3]):
            d = f32([0.3, -0.2, -det])
            o = f32([p[0], p[1], 0]) - d                       # reaches p at t ~ 1
            rows.append(np.concatenate([v0, v0 + e1, v0 + e2, o, d]))
    # u = x, v = y exactly for this triangle and d = -z: the edges u = 0, v = 0, u + v = 1, +-0 and one ulp either side
    edge = [0.0, -0.0, 1e-45, -1e-45, 1e-7, -1e-7]
    pts = [(u, v) for u in edge for v in (0.3, 0.0, -0.0, 1e-45)]
    pts += [(v, u) for u, v in pts]
    for s in (0.25, 0.5, 0.1, 0.7, 1.0 / 3.0):
        u = F32(s)
        for k in (-2, -1, 0, 1, 2):
            pts.append((float(u), float(ulps(F32(1) - u, k))))
    pts += [(1.0, 0.0), (0.0, 1.0), (float(ulps(F32(1), 1)), 0.0), (0.0, float(ulps(F32(1), -1)))]
    for u, v in pts:
        for base in (f32([0, 0, 0]), f32([2, -3, 0.5])):
            rows.append(np.concatenate([base, base + e1, base + e2, base + f32([u, v, 1]), f32([0, 0, -1])]))
    # origin on the plane (t = 0 < 1e-6), on a vertex, behind; degenerate (collapsed, colinear) and duplicated triangles
    tri = f32([[0.1, 0.2, 0.3], [1.3, 0.1, -0.2], [0.4, 1.5, 0.2]])
    cen = tri.mean(axis=0).astype(F32)
    for o, d in ((cen, _unit([0.2, 0.1, 1])[None][0]), (tri[0], _unit(cen - tri[0])), (tri[1], f32([0, 0, 1])),
                 (cen + f32([0, 0, 2]), f32([0, 0, -1])), (cen + f32([0, 0, 2]), f32([0, 0, 1])),
                 (cen + f32([0, 0, 2]), _unit(tri[2] - (cen + f32([0, 0, 2]))))):
        for t in (tri, tri[[0, 0, 2]], tri[[0, 1, 1]], f32([tri[0], tri[1], 2 * tri[1] - tri[0]]), tri[[1, 2, 0]], tri[[0, 2, 1]]):
            rows.append(np.concatenate([t.reshape(-1), o, d]))
    return f32(rows)


def _sphere_root(c, r, o, d):
    rel = o - c
    a, b = dot3(d, d), dot3(d, rel)
    cc = dot3(rel, rel) - r * r
    return b * b - a * cc


def _sphere_corners(rng):
    rows = []
    tol = F32(1e-5)
    # roots across the tangent band |b^2 - a c| < 1e-5 (ray.cpp:150,174): for each |d|, scan the offset h of a ray that
    # passes the sphere sideways and keep the h whose root lands nearest -1e-5, 0 and +1e-5 on either side
    for s2 in (1.0, 0.999, 0.998, 0.5, 4.0, 1e-2):
        s = F32(np.sqrt(s2))
        for rad in (F32(1), F32(2e-3), F32(0.05)):
            c = f32([0.5, -0.25, 0.125])
            d = f32([s, 0, 0])
            x0 = F32(-3) * rad - F32(1)
            for target in (tol, F32(0), -tol):
                h0 = np.sqrt(max(1e-30, float(rad) ** 2 - float(target) / float(s) ** 2))
                span = np.linspace(h0 * (1 - 2e-3), h0 * (1 + 2e-3), 8192).astype(F32)
                span = np.unique(np.concatenate([span, around(F32(h0), 16)]))
                o = np.stack([np.full_like(span, x0), span, np.zeros_like(span)], axis=1) + c
                o = f32(o)
                root = _sphere_root(c, rad, o, d)
                for lo_side in (True, False):
                    sel = (root < target) if lo_side else (root >= target)
                    if sel.any():
                        idx = np.argsort(np.abs(root - target) + np.where(sel, 0, np.inf))[:3]
                        for i in idx:
                            if np.isfinite(root[i]):
                                rows.append(np.concatenate([c, [rad], o[i], d]))
    # zero and negative radius, origin on the surface and at the centre, |d| != 1, zero direction
    c = f32([0.3, -0.7, 1.1])
    for rad in (0.0, -0.0, -0.5, 0.5, 1e-3):
        for o in (c, c + f32([abs(rad), 0, 0]), c + f32([0, 0, -abs(rad)]), c + f32([-3, 0.01, 0])):
            for d in (f32([1, 0, 0]), f32([0, 0, 1]), f32([0.5, 0, 0]), f32([3, 0.2, 0]), f32([0, 0, 0]), _unit([1, 1, 1])):
                rows.append(np.concatenate([c, [rad], o, d]))
    return f32(rows)


def _box_corners(rng):
    rows = []
    lo, hi = f32([-1, -1, -1]), f32([1, 1, 1])
    # per axis: origin on a face (lo - o = +0 or -0 products), inside, outside; d component +-0 (1/d = +-inf: 0 * inf = NaN)
    opool = f32([-2, -1, -0.0, 0.0, 0.5, 1, 2])
    dpool = f32([1, -1, 0.0, -0.0, 0.5, -0.25, 1e-30, -1e-30, 3e38, 1e-40])
    for _ in range(140):
        o, d = _pick(rng, opool, 3), _pick(rng, dpool, 3)
        rows.append(np.concatenate([lo, hi, o, d]))
    # on an edge / a corner, looking along the faces
    for o in (f32([1, 1, 0]), f32([-1, 1, -1]), f32([1, -0.0, 1])):
        for d in (f32([0, 0, 1]), f32([-0.0, 1, 0]), f32([-1, -0.0, 0.0]), _unit([-1, -1, -1])):
            rows.append(np.concatenate([lo, hi, o, d]))
    # flat boxes (lo = hi on an axis), inverted boxes (lo > hi), huge and denormal coordinates
    for b_lo, b_hi in ((f32([-1, 0, -1]), f32([1, 0, 1])), (f32([1, 1, 1]), f32([-1, -1, -1])), (f32([0, 0, 0]), f32([0, 0, 0])),
                       (f32([-3e38, -3e38, -3e38]), f32([3e38, 3e38, 3e38])), (f32([-1e-40, -1e-40, -1e-40]), f32([1e-40, 1e-40, 1e-40])),
                       (f32([1e30, -1, -1]), f32([2e30, 1, 1]))):
        for _ in range(10):
            o = _pick(rng, f32([-2, -1e-40, 0.0, -0.0, 1e-40, 2, 1e30, -3e38]), 3)
            d = _pick(rng, f32([1, -1, 0.0, -0.0, 0.7, 1e-30]), 3)
            rows.append(np.concatenate([b_lo, b_hi, o, d]))
    return f32(rows)


def _cylinder_corners(rng):
    rows = []
    axes = [[0, 0, 1], [0, 0, -1], [0, 0, 0.4], [0, 0, -2.5], [1e-4, 0, 1], [0, -1e-4, -1], [1e-7, 1e-7, 1], [-1e-7, 0, -1],
            [1e-3, 0, 1], [1, 0, 0], [0, -2, 0], [1, 1, 1]]
    for ax in axes:
        ax = f32(ax)
        u = _unit(ax.astype(np.float64))
        side = _unit(np.cross(u, [0.3, 0.7, 0.1]) if abs(u[2]) < 0.9 else np.cross(u, [1, 0, 0]))
        base = f32([0.25, -0.5, 0.125])
        for rad in (F32(0.5), F32(0), F32(-0.5), F32(1e-3)):
            on_side = base + F32(0.5) * ax + abs(rad) * side
            for o in (base, base + ax, base + F32(0.5) * ax, on_side, base + abs(rad) * side, base - F32(2) * ax + F32(0.1) * side,
                      base + F32(3) * side):
                for d in (u, -u, side, -side, _unit(u + side)):
                    if rng.uniform() < 0.45:
                        rows.append(np.concatenate([base, ax, [rad], o, f32(d)]))
    return f32(rows)


# ---- BSDF ---------------------------------------------------------------------------------------------------------
MATERIALS = f32([                                   # Kd Ks Kt ior
    [0.6, 0.6, 0.6, 0, 0, 0, 0, 0, 0, 1.0],        # diffuse
    [0.2, 0.2, 0.2, 1, 1, 1, 0, 0, 0, 1.0],        # diffuse + specular
    [0, 0, 0, 1, 1, 1, 0, 0, 0, 1.0],              # mirror
    [0, 0, 0, 0, 0, 0, 1, 1, 1, 1.4],              # glass
    [0, 0, 0, 0.2, 0, 0, 1, 0, 0, 1.2],            # red glass: logf(0) on two channels
    [0, 0, 0, 0, 0.5, 0, 0, 0.7, 0, 1.5],          # zero channels in Ks and Kt
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 1.0],              # all zero: 0/0 lobe weights
    [0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.4, 0.4, 0.4, 1.33],
    [0, 0, 0, 0, 0, 0, 1, 1, 1, 1.0],              # ior = 1
    [0.5, 0.1, 0.0, 0, 0, 0, 0, 0, 0, 1.0],        # diffuse, a zero channel
    [0.8, 0.8, 0.8, 1e-22, 0, 0, 0, 0, 0, 1.0],    # |Ks|^2 denormal
    [1e-30, 0, 0, 0, 0, 0, 0, 0, 0, 1.0],          # |Kd|^2 = 0, |Kd| > 0
    [0.1, 0.1, 0.1, 0, 0, 0, 1e-3, 1e-3, 1e-3, 2.4],
])
ROUGH = f32([0.01, 1e-4, 0.05, 0.1, 0.3, 0.5, 0.8, 1.0, 1e-20])


def _bsdf_dict(n):
    return dict(N=np.zeros((n, 3), F32), wi=np.zeros((n, 3), F32), wo=np.zeros((n, 3), F32), m=np.zeros((n, 10), F32),
                rough=np.full(n, 0.01, F32), dist=np.ones(n, F32), rr=np.ones(n, F32),
                seed=np.ones(n, np.uint32))


def _band_normals():
    """normals exactly +-z, inside and just outside sample_lobe_n's 1e-4 band around +-z, and in (1e-4, 1e-3)"""
    out = [[0, 0, 1], [0, 0, -1]]
    for dz in (1e-6, 5e-5, 9.9e-5, 1e-4, 1.01e-4, 3e-4, 5e-4, 9.9e-4, 1.1e-3):
        z = 1.0 - dz
        s = np.sqrt(1 - z * z)
        for sgn in (1, -1):
            out.append([s * 0.6, s * 0.8, sgn * z])
            v = f32([s, 0, sgn * z])
            out.append(v.tolist())
    return normalize3(f32(out))


def _tir_pairs(rng, count, ior):
    """(N, wi, wo) with the radicand 1 - n^2 (1 - (wo.m)^2) at exactly 0 and one representable step either side"""
    N = f32([0, 0, 1])
    ior = F32(ior)
    found = {}
    for trial in range(8):
        th = rng.uniform(0.5, 1.3)
        ph = rng.uniform(0, 2 * np.pi)
        wo = f32([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), -np.cos(th)])   # inside: ni = ior, no = 1, n = ior
        n = float(ior)
        crit = np.sqrt(1 - 1 / n ** 2) * (1 if trial % 2 else -1)
        # a unit m with wo.m = +-crit, tilted towards N (so that D(N, m) > 0), then wi with m ~ -(ior wi + wo)
        w64 = wo.astype(np.float64)
        perp = _unit(N - np.dot(N, w64) * w64).astype(np.float64)
        m = _unit(crit * w64 + np.sqrt(1 - crit ** 2) * perp).astype(np.float64)
        k = -np.dot(m, w64) + np.sqrt(np.dot(m, w64) ** 2 + n ** 2 - 1)
        wi0 = _unit(-(k * m + w64) / n)
        cand = f32(wi0[None, :] + rng.normal(scale=3e-7, size=(200000, 3)))
        r = radicand(np.broadcast_to(N, cand.shape), cand, np.broadcast_to(wo, cand.shape), np.full(len(cand), ior, F32))
        for i in np.flatnonzero(r == 0)[:2]:
            found.setdefault("zero", []).append((wo, cand[i]))
        pos = np.where(r > 0, r, np.inf)
        neg = np.where(r < 0, -r, np.inf)
        for arr, name in ((pos, "pos"), (neg, "neg")):
            i = int(np.argmin(arr))
            if np.isfinite(arr[i]):
                found.setdefault(name, []).append((wo, cand[i]))
    out = []
    for name in ("zero", "pos", "neg"):
        out += found.get(name, [])[:count]
    return [(N, wi, wo, ior) for wo, wi in out]


def _bsdf_corner_dict(rng):
    geo = []                                            # (N, wi, wo)
    Ns = _band_normals()
    for N in Ns:
        t = _unit(np.cross(N, [0.3, 0.5, 0.7]))
        wo = _unit(N * 0.6 + t * 0.8)
        refl = f32(2 * dot3(wo, N) * N - wo)
        for wi in (wo, -wo, t, -t, refl, _unit(refl + f32([1e-3, 0, 0])), _unit(-N * 0.3 + t), N, -N):
            geo.append((N, f32(wi), wo, None))
        geo.append((N, t, -t, None))                    # wi.N = 0 and wo.N = 0
        geo.append((N, _unit(N + t), t, None))          # wo.N = 0
        geo.append((N, -wo, -N, None))
    for ior in (1.4, 1.5, 1.33, 2.0):
        geo += _tir_pairs(rng, 3, ior)
    mats = MATERIALS
    n = len(geo) * 3
    B = _bsdf_dict(n)
    # materials: every geometry with three materials; the radicand rows get transmitting ones with the ior they were made for
    B["m"] = mats[rng.integers(0, len(mats), size=n)]
    B["m"][: len(mats)] = mats
    for i in range(n):
        N, wi, wo, ior = geo[i % len(geo)]
        B["N"][i], B["wi"][i], B["wo"][i] = N, wi, wo
        if ior is not None:
            B["m"][i] = [[0, 0, 0, 0.3, 0.3, 0.3, 0.9, 0.8, 0.0, ior], [0, 0, 0, 0, 0, 0, 1, 1, 1, ior],
                         [0.2, 0.2, 0.2, 0, 0, 0, 0.5, 0, 0.5, ior]][i // len(geo)]
    B["rough"] = _pick(rng, ROUGH, n)
    B["dist"] = _pick(rng, f32([0, 1e-3, 0.5, 7.5, 1e3, 1e30]), n)
    B["rr"] = _pick(rng, f32([1, 0.5, 0.8, 1e-30]), n)
    B["seed"] = rng.integers(1, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    return B


def straddle_rr(rows, p0):
    """op 15 / 16 rows with rr set so that p = p0 * rr lands one step below, at and above the 1e-6 guard (p0: op 6's
    answer on the same rows)"""
    out = []
    with np.errstate(all="ignore"):
        rr0 = F32(1e-6) / f32(p0)
    ok = np.isfinite(rr0) & (rr0 > 0) & (rr0 <= 1)
    for k in (-1, 0, 1):
        r = f32(rows[ok]).copy()
        r[:, 21] = ulps(rr0[ok], k)
        out.append(r)
    return np.concatenate(out)


def bsdf_rows(op, B):
    """the dict of BSDF inputs in op's layout"""
    m, n = B["m"], len(B["N"])
    col = lambda v: f32(v).reshape(n, 1)
    seed = B["seed"].astype("<u4").view("<f4").reshape(n, 1)
    if op in (5, 17, 18):
        return np.concatenate([seed, B["N"], B["wo"], col(B["rough"]), m], axis=1)
    if op == 6:
        return np.concatenate([B["N"], B["wi"], B["wo"], col(B["rough"]), m], axis=1)
    if op == 7:
        return np.concatenate([B["N"], B["wi"], B["wo"], m, col(B["rough"]), col(B["dist"])], axis=1)
    if op in (15, 16):
        return np.concatenate([B["N"], B["wi"], B["wo"], m, col(B["rough"]), col(B["dist"]), col(B["rr"])], axis=1)
    raise ValueError(op)


def variant_to_generic(op, rows):
    """rows of a kernel form -> the rows of its generic op (GENERIC_OF)"""
    rows = f32(rows)
    if op in (14, 17, 18, 19):
        return rows
    if op in (15, 16):   # N wi wo Kd Ks Kt ior rough dist rr -> op 6: N wi wo rough Kd Ks Kt ior
        return np.concatenate([rows[:, 0:9], rows[:, 19:20], rows[:, 9:19]], axis=1)
    raise ValueError(op)


def variant_to_eval(rows):
    """rows of op 15 / 16 -> op 7 (N wi wo Kd Ks Kt ior rough dist)"""
    return f32(rows)[:, :21]


def diffuse_rows(rows, op):
    """the rows of op (16 / 18 layouts) whose material passes the diffuse kernels' upload guard"""
    off = 8 if op in (5, 17, 18) else 9
    return rows[is_diffuse_material(rows[:, off:off + 3], rows[:, off + 3:off + 6], rows[:, off + 6:off + 9])]


def finite_box_rows(rows):
    """op 3 / 14 rows whose origin and 1/d are all finite (all_finite6: what test_prim<FINITE_RAY> and the prologue get)"""
    with np.errstate(all="ignore"):
        inv = F32(1) / rows[:, 9:12]
    return rows[np.isfinite(rows[:, 6:9]).all(axis=1) & np.isfinite(inv).all(axis=1)]


# ---- libm and the rest ----------------------------------------------------------------------------------------------
def quadrant_args():
    """every f32 within 4 ulps of k pi / 4, k = -8 .. 8 (sin / cos quadrant boundaries)"""
    base = f32([k * np.pi / 4 for k in range(-8, 9)])
    return np.unique(around(base, 4))


def _libm_corners(rng):
    x = quadrant_args()
    n = len(x)
    y = _pick(rng, f32([5, 4, 0.5, -1, 2]), n)
    rows = [np.stack([x, y], axis=1)]
    special = f32([0, -0.0, 1, -1, np.inf, -np.inf, np.nan, 1e-45, 1e-40, 1.1754944e-38, ulps(F32(1), -1), ulps(F32(1), 1), 2.7182817, 0.5])
    ys = f32([5, 4, 0, -0.0, -1e-45, -1, -np.inf, np.inf, 1e-40, -88.7, -103.9, -104, -150])
    g = np.array(np.meshgrid(special, ys)).reshape(2, -1).T
    rows.append(f32(g))
    e = F32(np.e)
    rows.append(np.stack([np.full(len(ys), e, F32), ys], axis=1))
    # atan2f(rough sqrt(e0), sqrt(1 - e0)) at e0 = 0 and 1: x = 0 or y = 0
    e0 = f32([0, 1e-45, 0.5, ulps(F32(1), -1), 1])
    for rough in (0.01, 1.0, 1e-4):
        yy = F32(rough) * np.sqrt(e0).astype(F32)
        xx = np.sqrt(F32(1) - e0).astype(F32)
        rows.append(np.stack([xx, yy], axis=1))
    return np.concatenate(rows).astype(F32)


def _lobe_corners(rng):
    Ns = _band_normals()
    rows = []
    cs = f32([0, 1, ulps(F32(1), -1), 0.5, 1e-4])
    phis = quadrant_args()
    for N in Ns:
        for c in cs:
            for phi in _pick(rng, phis, 3):
                rows.append([N[0], N[1], N[2], c, phi])
        rows.append([N[0] * 3, N[1] * 3, N[2] * 3, 0.5, 1.0])   # unnormalised N: normalised inside
    rows.append([0, 0, 0, 0.5, 1.0])
    return f32(rows)


def _normalize_corners(rng):
    ln = around(F32(1e-6), 4)
    rows = [np.stack([ln, np.zeros_like(ln), np.zeros_like(ln)], axis=1)]
    rows.append(np.stack([-ln, np.zeros_like(ln), np.zeros_like(ln)], axis=1))
    u = _unit([0.48, 0.6, 0.64])
    rows.append(f32(ln[:, None] * u[None, :]))
    rows.append(f32([[0, 0, 0], [-0.0, 0, -0.0], [1e-40, 0, 0], [3e38, 3e38, 0], [1e20, 1e20, 1e20], [np.inf, 0, 0], [np.nan, 1, 0]]))
    return np.concatenate(rows).astype(F32)


def _fgg_corners(rng):
    rows = []
    ldh = f32([0, -0.0, 1, -1, ulps(F32(1), -1), -ulps(F32(1), -1), 1e-45, 0.5, 1.0000001, -1.0000001])
    Ns = _band_normals()
    for i in range(120):
        N = Ns[i % len(Ns)]
        t = _unit(np.cross(N, [0.3, 0.5, 0.7]))
        H = [N, _unit(N + f32([1e-3, 0, 0])), t, _unit(N + t), -N, _unit(t + f32(1e-7) * N)][i % 6]
        w = [N, t, _unit(N + t), f32([0, 0, 0]), -N][(i // 6) % 5]
        rows.append(np.concatenate([_pick(rng, MATERIALS[:, 3:6].reshape(-1), 3), [ldh[i % len(ldh)]], N, H,
                                    [ROUGH[i % len(ROUGH)]], w]))
    return f32(rows)


_CORNERS = {1: _triangle_corners, 2: _sphere_corners, 3: _box_corners, 4: _cylinder_corners, 8: _lobe_corners,
            9: _libm_corners, 10: _normalize_corners, 11: _fgg_corners}


def corners(op, seed=20261016):
    """the corner rows of op (the generic ops' own; a kernel form's are those of its generic op, filtered to its callers'
    inputs)"""
    rng = np.random.default_rng(seed + op)
    if op in _CORNERS:
        return _CORNERS[op](rng)
    if op in (5, 6, 7, 15, 16, 17, 18):
        rows = bsdf_rows(op, _bsdf_corner_dict(np.random.default_rng(seed)))
        return diffuse_rows(rows, op) if op in (16, 18) else rows
    if op == 14:
        return corners(3, seed)
    if op == 19:
        return quadrant_args().reshape(-1, 1)
    raise ValueError(op)


# ---- bulk -------------------------------------------------------------------------------------------------------
def _bsdf_bulk_dict(rng, n):
    B = _bsdf_dict(n)
    B["N"] = _rand_unit(rng, n)
    near_z = rng.uniform(size=n) < 0.1               # a tenth of the normals near +-z
    B["N"][near_z] = normalize3(f32(np.stack([rng.normal(scale=1e-3, size=near_z.sum()), rng.normal(scale=1e-3, size=near_z.sum()),
                                              np.sign(rng.uniform(-1, 1, size=near_z.sum()))], axis=1)))
    B["wo"] = _rand_unit(rng, n)
    B["wi"] = _rand_unit(rng, n)
    flip = (dot3(B["wo"], B["N"]) < 0) & (rng.uniform(size=n) < 0.7)
    B["wo"][flip] = -B["wo"][flip]
    spec = rng.uniform(size=n) < 0.4                 # wi near the mirror direction: the GGX lobe
    refl = f32(2 * dot3(B["wo"], B["N"])[:, None] * B["N"] - B["wo"])
    B["wi"][spec] = _unit(refl[spec] + rng.normal(scale=rng.uniform(1e-3, 0.2, size=(spec.sum(), 1)), size=(spec.sum(), 3)))
    m = MATERIALS[rng.integers(0, len(MATERIALS), size=n)].copy()
    free = rng.uniform(size=n) < 0.5                  # half the materials: random coefficients, random zero channels
    k = free.sum()
    mm = f32(rng.uniform(0, 1, size=(k, 10)) * (rng.uniform(size=(k, 10)) < 0.6))
    mm[:, 9] = f32(rng.uniform(1, 2.5, size=k))
    m[free] = mm
    B["m"] = m
    B["rough"] = f32(np.where(rng.uniform(size=n) < 0.3, 0.01, rng.uniform(0, 1, size=n)))
    B["rough"][B["rough"] == 0] = F32(0.01)
    B["dist"] = f32(rng.exponential(2.0, size=n))
    B["rr"] = f32(np.where(rng.uniform(size=n) < 0.5, 0.8, rng.uniform(0, 1, size=n)))
    B["seed"] = rng.integers(1, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    return B


def _diffuse_bulk_dict(rng, n):
    B = _bsdf_bulk_dict(rng, n)
    B["m"][:, 3:9] = 0
    B["m"][: n // 64, 0:3] = 0                       # zero-weight materials (0/0 lobe weights) pass the guard too
    return B


def bulk(op, n, seed=1):
    """n seeded realistic rows for op"""
    rng = np.random.default_rng(seed * 1000 + op)
    if op == 1:
        v = f32(rng.uniform(-2, 2, size=(n, 9)))
        o = f32(rng.uniform(-4, 4, size=(n, 3)))
        cen = (v[:, 0:3] + v[:, 3:6] + v[:, 6:9]) / F32(3)
        d = _unit(cen + f32(rng.normal(scale=0.6, size=(n, 3))) - o)
        return np.concatenate([v, o, d], axis=1).astype(F32)
    if op == 2:
        c = f32(rng.uniform(-2, 2, size=(n, 3)))
        r = f32(rng.uniform(0.001, 1.5, size=(n, 1)))
        o = f32(rng.uniform(-4, 4, size=(n, 3)))
        d = _unit(c + f32(rng.normal(scale=0.8, size=(n, 3))) * r - o)
        d *= f32(np.where(rng.uniform(size=(n, 1)) < 0.2, rng.uniform(0.3, 1.5, size=(n, 1)), 1.0))
        return np.concatenate([c, r, o, d], axis=1).astype(F32)
    if op in (3, 14):
        lo = f32(rng.uniform(-3, 0, size=(n, 3)))
        hi = lo + f32(rng.uniform(0.0, 3, size=(n, 3)))
        o = f32(rng.uniform(-5, 5, size=(n, 3)))
        d = _unit((lo + hi) / F32(2) + f32(rng.normal(scale=1.0, size=(n, 3))) - o)
        ax = rng.uniform(size=(n, 3)) < 0.05         # axis-parallel components: 1/d = +-inf
        d[ax] = _pick(rng, [0.0, -0.0], ax.sum())
        on = rng.uniform(size=(n, 3)) < 0.05         # origins on a face plane
        o[on] = np.where(rng.uniform(size=on.sum()) < 0.5, lo[on], hi[on])
        rows = np.concatenate([lo, hi, o, d], axis=1).astype(F32)
        return rows
    if op == 4:
        base = f32(rng.uniform(-2, 2, size=(n, 3)))
        axis = f32(rng.normal(size=(n, 3)) * rng.uniform(0.2, 3, size=(n, 1)))
        z = rng.uniform(size=n) < 0.1
        axis[z] = f32(np.stack([rng.normal(scale=1e-4, size=z.sum()), rng.normal(scale=1e-4, size=z.sum()),
                                np.sign(rng.uniform(-1, 1, size=z.sum()))], axis=1))
        r = f32(rng.uniform(0.001, 0.8, size=(n, 1)))
        o = f32(rng.uniform(-4, 4, size=(n, 3)))
        d = _unit(base + axis * f32(rng.uniform(0, 1, size=(n, 1))) + f32(rng.normal(scale=0.5, size=(n, 3))) - o)
        return np.concatenate([base, axis, r, o, d], axis=1).astype(F32)
    if op in (5, 6, 7, 15, 17):
        return bsdf_rows(op, _bsdf_bulk_dict(rng, n))
    if op in (16, 18):
        return diffuse_rows(bsdf_rows(op, _diffuse_bulk_dict(rng, n)), op)
    if op == 8:
        N = _rand_unit(rng, n) * f32(rng.uniform(0.5, 2, size=(n, 1)))
        z = rng.uniform(size=n) < 0.2
        N[z] = f32(np.stack([rng.normal(scale=3e-3, size=z.sum()), rng.normal(scale=3e-3, size=z.sum()),
                             np.sign(rng.uniform(-1, 1, size=z.sum()))], axis=1))
        return np.concatenate([N, f32(rng.uniform(0, 1, size=(n, 1))), f32(rng.uniform(0, 1, size=(n, 1))) * TWO_PI], axis=1).astype(F32)
    if op == 9:
        x = f32(rng.uniform(-7, 7, size=n))
        y = f32(rng.uniform(-6, 6, size=n))
        h = n // 2
        x[h:] = f32(rng.uniform(0, 1, size=n - h))
        y[h:] = _pick(rng, [4, 5], n - h)
        return np.stack([x, y], axis=1)
    if op == 10:
        return f32(rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-8, 4, size=(n, 1)))
    if op == 11:
        B = _bsdf_bulk_dict(rng, n)
        H = _unit(B["N"] + f32(rng.normal(scale=rng.uniform(1e-3, 0.5, size=(n, 1)), size=(n, 3))))
        ldh = f32(rng.uniform(-1.05, 1.05, size=(n, 1)))
        return np.concatenate([B["m"][:, 3:6], ldh, B["N"], H, B["rough"].reshape(n, 1), B["wo"]], axis=1).astype(F32)
    if op == 19:
        return f32(rng.uniform(0, 1, size=(n, 1))) * TWO_PI
    raise ValueError(op)


def libm_sweeps(n, seed=7):
    """op 9 rows over the path's argument ranges, n per function (generator of chunks):
    sin / cos / sincos on [0, 2 pi); atan2f(rough sqrt(e0), sqrt(1 - e0)); powf(x, 5), powf(x, 4), logf on [0, 1];
    powf(e, y) for y <= 0 down to -inf (dist * logf(Kt))"""
    rng = np.random.default_rng(seed)
    chunk = 1 << 20
    e = F32(np.e)
    for name in ("sincos", "atan2", "pow5", "pow4", "exp"):
        for k in range(0, n, chunk):
            m = min(chunk, n - k)
            if name == "sincos":
                x = f32(rng.uniform(0, 1, size=m)) * TWO_PI
                y = np.full(m, 5, F32)
            elif name == "atan2":
                e0 = f32(rng.uniform(0, 1, size=m))
                rough = f32(np.where(rng.uniform(size=m) < 0.5, 0.01, rng.uniform(0, 1, size=m)))
                x, y = np.sqrt(F32(1) - e0).astype(F32), (rough * np.sqrt(e0)).astype(F32)
            elif name in ("pow5", "pow4"):
                x = f32(rng.uniform(0, 1, size=m))
                x[: m // 16] = f32(10.0 ** rng.uniform(-45, 0, size=m // 16))
                y = np.full(m, 5 if name == "pow5" else 4, F32)
            else:
                x = np.full(m, e, F32)
                y = -f32(rng.exponential(3.0, size=m) * (10.0 ** rng.uniform(-6, 2, size=m)))
                y[: 64] = -np.inf
            yield name, np.stack([x, y], axis=1).astype(F32)


# ---- comparison --------------------------------------------------------------------------------------------------
def mismatches(got, want, zero_sign=False):
    """False where got == want bit for bit or both are NaN (any NaN matches any NaN); zero_sign: +0 also matches -0"""
    a = np.ascontiguousarray(got, dtype=F32)
    b = np.ascontiguousarray(want, dtype=F32)
    ok = (a.view("<u4") == b.view("<u4")) | (np.isnan(a) & np.isnan(b))
    if zero_sign:
        ok |= (a == 0) & (b == 0)
    return ~ok


def assert_match(got, want, rows, what, zero_sign=False):
    bad = mismatches(got, want, zero_sign)
    if bad.ndim > 1:
        bad = bad.any(axis=tuple(range(1, bad.ndim)))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError("%s: %d of %d records differ; first: in %s -> %r, want %r"
                             % (what, int(bad.sum()), len(bad), f32(rows[i]).tolist(), f32(got[i]).tolist(), f32(want[i]).tolist()))


def check_kernel_form(op, rows, got, generic, what=""):
    """got = the outputs of kernel form op (14-19) on rows; generic(records) -> outputs of the generic ops (the oracle's
    unit_batch, or the device's own ops).  Asserts that the form gives its generic function's answer:
      14  hit_aab_finite == op 3 (t up to the sign of a zero, normal exact) and hit_aab_t_finite == op 3's t, both where
          all_finite6(o, 1/d); hit_aab_t == op 3's t everywhere
      15  p == op 6 * rr (in f32); f == op 7 where p > 1e-6, else 0
      16  pdf_brdf<true> * rr == op 6 * rr; eval_scattering<true> == op 7
      17, 18  == op 5 (wi, is_trans, RNG state)
      19  == op 9's sinf, cosf"""
    rows, got = f32(rows), f32(got)
    what = "%s op %d" % (what, op)
    if op == 14:
        want = generic(records(3, rows))
        with np.errstate(all="ignore"):
            fin = np.isfinite(rows[:, 6:9]).all(axis=1) & np.isfinite(F32(1) / rows[:, 9:12]).all(axis=1)
        assert_match(got[fin, 0], want[fin, 0], rows[fin], what + " hit_aab_finite t", zero_sign=True)
        assert_match(got[fin, 1:4], want[fin, 1:4], rows[fin], what + " hit_aab_finite n")
        assert_match(got[fin, 4], want[fin, 0], rows[fin], what + " hit_aab_t_finite", zero_sign=True)
        assert_match(got[:, 5], want[:, 0], rows, what + " hit_aab_t")
    elif op in (15, 16):
        rr = rows[:, 21]
        p = generic(records(6, variant_to_generic(op, rows)))[:, 0] * rr
        f = generic(records(7, variant_to_eval(rows)))[:, 0:3]
        assert_match(got[:, 0], p, rows, what + " p")
        if op == 15:
            big = got[:, 0] > F32(1e-6)
            f = np.where(big[:, None], f, F32(0))
        assert_match(got[:, 1:4], f, rows, what + " f")
    elif op in (17, 18):
        assert_match(got[:, 0:5], generic(records(5, rows))[:, 0:5], rows, what + " wi, is_trans, rng")
    elif op == 19:
        want = generic(records(9, np.concatenate([rows[:, :1], np.zeros_like(rows[:, :1])], axis=1)))
        assert_match(got[:, 0:2], want[:, 0:2], rows, what + " sin, cos")
    else:
        raise ValueError(op)
    assert got[:, 6:].view("<u4").max(initial=0) == 0, what + ": unused outputs are not 0"


KERNEL_FORMS = (14, 15, 16, 17, 18, 19)


def kernel_form_rows(op, rows, p0=None):
    """rows for kernel form op from the corner or bulk rows of the same op; with p0 (op 6's answer on op 15 / 16 rows),
    rows whose p straddles the 1e-6 guard are added"""
    if op in (15, 16) and p0 is not None:
        rows = np.concatenate([rows, straddle_rr(rows, p0)])
    return f32(rows)
