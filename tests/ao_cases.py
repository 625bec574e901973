"""Ambient-occlusion queries (ort_ambient_occlusion and its device form) against what exists: the points, the radii, and what
they must give (test infrastructure, next to irradiance_cases.py).

Nothing of the query is restated here.  Sample k of a point (p, n) is irradiance_cases.directions' d_k (the oracle's rng_table,
unit ops 8 and 10, numpy float32 for the square root and the product), OracleScene.raycast(p, d_k) for t and mat,
occluded_cases.expected for the bit at the point's radius, and a numpy float32 sum in sample order for the bent sum."""
import os
import zlib

import numpy as np

import host_sim_tool as hs
import irradiance_cases as ic
import occluded_cases as oc
import radiance_cases as rc

F = np.float32
AO_INVALID = 0xFFFFFFFF
SAMPLES = 8   # samples per point of the oracle's table: the largest spp of the tests
AXIS_POINTS = 4


class World:
    """pts: irradiance_cases.Points, the scene's point_set and AXIS_POINTS more; base: how many of them are the point_set's;
    d (N, SAMPLES, 3), t, mat (N, SAMPLES), after (N, SAMPLES): the oracle's table (rows of points outside the domain unused);
    diag, R; radii: the scene's radius array"""


def with_axis_points(pts, rng):
    """AXIS_POINTS more points whose first sample's direction is exactly the normal: where points of the set stand (inside the
    domain and the scene's box), the normal exactly (0, 0, +-1), the seed a state whose first draw is 1.0, so c = 1 and d_0 = n"""
    at = rng.choice(np.flatnonzero(pts.ok & ~pts.far), AXIS_POINTS, replace=False)
    extra = pts.points[at].copy()
    extra[:, 3:6] = [(0, 0, 1 if k % 2 == 0 else -1) for k in range(AXIS_POINTS)]
    seeds = np.full(AXIS_POINTS, rc.unstep(0xFFFFFFFF), "<u4")
    return ic.Points(np.concatenate([pts.points, extra]).astype("<f4"), np.concatenate([pts.seeds, seeds]).astype("<u4"),
                     np.concatenate([pts.ok, np.ones(AXIS_POINTS, bool)]), np.concatenate([pts.far, np.zeros(AXIS_POINTS, bool)]))


def sample_table(oracle, osc, pts, spp=SAMPLES):
    """-> d (N, spp, 3), t (N, spp), mat (N, spp), after (N, spp): per point inside the domain and sample, the drawn direction,
    the oracle's closest hit along it and the stream's state after the sample's two draws"""
    n = len(pts.points)
    idx = np.flatnonzero(pts.ok)
    p, nrm = pts.points[idx, 0:3], pts.points[idx, 3:6]
    s = np.where(pts.seeds[idx] == 0, 1, pts.seeds[idx]).astype("<u4")
    d, t, mat, after = np.zeros((n, spp, 3), "<f4"), np.zeros((n, spp), "<f4"), np.zeros((n, spp), "<u4"), np.zeros((n, spp), "<u4")
    for k in range(spp):
        dk, _, s = ic.directions(oracle, nrm, s)
        s = np.asarray(s, "<u4").copy()
        tk, _, mk = osc.raycast(p, dk)
        d[idx, k], t[idx, k], mat[idx, k], after[idx, k] = dk, tk, mk, s
    return d, t, mat, after


def radius_array(name, w):
    """One radius per point, from a draw seeded by the scene's name: R for most; +inf, NaN, 0, -1, FLT_MAX and 0.4 x the diagonal
    for four points each (two each in a set of fewer than 100, so that R stays the most); and for 18 points inside the domain (16
    in such a set) the hit distance of one of that point's own first 8 samples, in turn as it is, one float below and one float
    above (the strict < inside the lane).  -> (radii float32[N], those points)"""
    rng = np.random.default_rng(zlib.crc32(("ao radii " + name).encode()))
    n = len(w.pts.points)
    radii = np.full(n, w.R, "<f4")
    hits = np.flatnonzero(w.pts.ok & (w.mat[:, :SAMPLES] != 0).any(axis=1))
    few, n_own = (4, 18) if n >= 100 else (2, 16)
    own = rng.choice(hits, n_own, replace=False)
    for j, i in enumerate(own):
        k = rng.choice(np.flatnonzero(w.mat[i, :SAMPLES] != 0))
        t = w.t[i, k]
        with np.errstate(over="ignore"):
            radii[i] = (t, np.nextafter(t, F(0)), np.nextafter(t, F(np.inf)))[j % 3]
    rest = rng.permutation(np.setdiff1d(np.arange(n), own))
    for j, v in enumerate((np.inf, np.nan, 0.0, -1.0, oc.FLT_MAX, 0.4 * w.diag)):
        radii[rest[few * j:few * j + few]] = F(v)
    return radii, own


def build(name, scene, flat, osc, oracle, n):
    """the world of a scene: computed once by the tests that share it, and left unchanged"""
    w = World()
    w.name, w.scene, w.flat, w.osc = name, scene, flat, osc
    base = ic.point_set(name, flat, osc, n)
    w.base = n
    w.pts = with_axis_points(base, np.random.default_rng(zlib.crc32(("ao axis " + name).encode())))
    w.d, w.t, w.mat, w.after = sample_table(oracle, osc, w.pts)
    lo, hi = rc.origin_box(flat)
    w.lo, w.hi = lo, hi
    w.diag = float(np.linalg.norm(np.asarray(hi, np.float64) - np.asarray(lo, np.float64)))
    w.R = F(0.1 * w.diag)
    w.radii, w.own = radius_array(name, w)
    return w


def bits(w, radius, spp):
    """-> bool (N, spp): sample k of point i is occluded (occluded_cases.expected); radius: None, a scalar or (N,)"""
    n = len(w.pts.points)
    r = np.full(n, np.inf, "<f4") if radius is None else np.broadcast_to(np.asarray(radius, "<f4"), (n,))
    return oc.expected(w.t[:, :spp], w.mat[:, :spp], r[:, None])


def expected(w, radius, spp, idx=None):
    """-> (open uint32[N], bent float32[N, 3], final states uint32[N]) for all points of the world, or those of idx: the oracle's
    answer inside the domain; AO_INVALID, NaN and the seed outside"""
    p = w.pts
    n = len(p.points)
    occ = bits(w, radius, spp)
    out = np.full(n, AO_INVALID, "<u4")
    bent = np.full((n, 3), np.nan, "<f4")
    fin = p.seeds.copy()
    for i in np.flatnonzero(p.ok):
        b = np.zeros(3, "<f4")
        for k in range(spp):
            if not occ[i, k]:
                b = (b + w.d[i, k]).astype("<f4")   # a separately rounded float32 add per component
        out[i], bent[i], fin[i] = spp - int(occ[i].sum()), b, w.after[i, spp - 1]
    if idx is not None:
        return out[idx], bent[idx], fin[idx]
    return out, bent, fin


def classes(w, radius, spp=SAMPLES):
    """of the point_set's points inside the domain: the shares that are mixed, all open, all occluded"""
    ok = w.pts.ok[:w.base]
    occ = bits(w, radius, spp)[:w.base][ok].sum(axis=1)
    return ((occ > 0) & (occ < spp)).mean(), (occ == 0).mean(), (occ == spp).mean()


LADDER_POINTS = 64
LADDER_SEED = 20   # of the draw below: with it 64 of testscene's 64 first samples hit a surface (the test asserts at least 48)


def radius_ladder(oracle, osc, flat, n=LADDER_POINTS):
    """The strict < of a sample's verdict, at one sample per point: n surface points (irradiance_cases.on_surfaces) with arbitrary
    seeds; t = the oracle's distance along sample 0's direction; each point whose sample hits a surface three times, at radius
    prev(t), t and next(t), the neighbouring floats: open counts 1, 1, 0.  Points whose sample hits nothing are left out.
    -> (points (3m, 6), seeds (3m,), radii (3m,), open uint32 (3m,), how many of the n points were left out)"""
    rng = np.random.default_rng(LADDER_SEED)
    lo, hi = rc.origin_box(flat)
    pts = ic.on_surfaces(rng, osc, lo, hi, n)
    seeds = rng.integers(1, 1 << 32, size=n, dtype=np.uint64).astype("<u4")
    assert ic.in_domain(pts).all()
    d0, _, _ = ic.directions(oracle, pts[:, 3:6], seeds)
    t, _, mat = osc.raycast(pts[:, 0:3], d0)
    hit = np.flatnonzero(np.asarray(mat) != 0)
    t = np.asarray(t, "<f4")[hit]
    assert np.isfinite(t).all() and (t > 0).all()
    radii = np.stack([np.nextafter(t, F(0)), t, np.nextafter(t, F(np.inf))], axis=1).astype("<f4")
    assert (radii[:, 0] < t).all() and (t < radii[:, 2]).all() and np.isfinite(radii).all()
    return (np.repeat(pts[hit], 3, axis=0).astype("<f4"), np.repeat(seeds[hit], 3), radii.reshape(-1),
            np.tile(np.array([1, 1, 0], "<u4"), len(hit)), n - len(hit))


def assert_same(got, want, what):
    """(open, bent, states) against (open, bent, states): all bits, NaN by position; a None on either side is not compared"""
    for g, w_, label in zip(got, want, ("open", "bent", "final states")):
        if g is None or w_ is None:
            continue
        if label == "bent":
            g, w_ = np.ascontiguousarray(g, "<f4").reshape(-1, 3), np.ascontiguousarray(w_, "<f4").reshape(-1, 3)
            assert g.shape == w_.shape, "%s %s: shape %s vs %s" % (what, label, g.shape, w_.shape)
            nan_g, nan_w = np.isnan(g), np.isnan(w_)
            assert (nan_g == nan_w).all(), "%s %s: NaN at other places, first point %d" % (what, label, np.argwhere(nan_g != nan_w)[0][0])
            ne = (g.view("<u4") != w_.view("<u4")) & ~nan_w
        else:
            g, w_ = np.ascontiguousarray(g, "<u4"), np.ascontiguousarray(w_, "<u4")
            assert g.shape == w_.shape, "%s %s: shape %s vs %s" % (what, label, g.shape, w_.shape)
            ne = g != w_
        if ne.any():
            i = np.argwhere(ne)[0]
            raise AssertionError("%s %s: %d of %d words differ; first at %s: %r vs %r" % (what, label, ne.sum(), ne.size, tuple(i), g[tuple(i)], w_[tuple(i)]))


# ---- tools/host_sim --ambient-occlusion ----------------------------------------------------------------------------------------
def host_sim(tool, d, scene, points, seeds, radius, spp, want_bent=True, want_states=True, base=None, **kw):
    """radius: None or (n,).  -> (open, bent or None, final states or None, CompletedProcess)"""
    d = str(d)
    path = lambda f: os.path.join(d, f)
    np.ascontiguousarray(points, "<f4").tofile(path("ao_points.f32"))
    np.ascontiguousarray(seeds, "<u4").tofile(path("ao_seeds.u32"))
    if radius is not None:
        np.ascontiguousarray(radius, "<f4").tofile(path("ao_radius.f32"))
    for f in ("ao_open.u32", "ao_bent.f32", "ao_states.u32"):
        if os.path.exists(path(f)):
            os.remove(path(f))
    r = hs.run(tool, ["--ambient-occlusion"] + hs.scene_args(scene, base) +
               [path("ao_points.f32"), path("ao_seeds.u32"), path("ao_radius.f32") if radius is not None else "-", spp, path("ao_open.u32"),
                path("ao_bent.f32") if want_bent else "-", path("ao_states.u32") if want_states else "-"], **kw)
    assert os.path.exists(path("ao_bent.f32")) == want_bent and os.path.exists(path("ao_states.u32")) == want_states
    out = np.fromfile(path("ao_open.u32"), "<u4")
    assert len(out) == len(points)
    return (out, np.fromfile(path("ao_bent.f32"), "<f4").reshape(-1, 3) if want_bent else None,
            np.fromfile(path("ao_states.u32"), "<u4") if want_states else None, r)
