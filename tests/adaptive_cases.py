"""Adaptive radiance queries (ort_radiance_adaptive) against the oracle as it stands: the stopping rule of include/ort.h restated
in numpy float32, operation by operation, and what a query must give -- one chain of max_spp oracle samples per ray
(radiance_cases.sample_chain), cut where the rule stops.  Every value is a numpy float32 scalar, so every operation rounds on its
own, as the library's separately rounded f32 operations do."""
import os
import zlib
from collections import namedtuple

import numpy as np

import host_sim_tool as hs
import radiance_cases as rc

F = np.float32

Adaptive = namedtuple("Adaptive", "min_spp max_spp check_every tolerance floor")

# The parameter sets of the GPU tests.  MAIN is min 4, every 4, max 64, floor 0.05 with the tolerance at 0.3 (at 0.25 too few of
# these rays stop strictly between min_spp and max_spp); tests/test_adaptive_host.py::test_case_sets_are_not_vacuous holds the
# three classes of rays under it from the oracle alone.  EVERY checks after every sample, the last check at 16; FIXED never checks.
MAIN = Adaptive(4, 64, 4, 0.3, 0.05)
EVERY = Adaptive(2, 17, 1, 0.3, 0.05)
FIXED = Adaptive(8, 8, 3, 0.3, 0.05)
SETS = (MAIN, EVERY, FIXED)
RR = 0.8
HUGE = Adaptive(4, 64, 4, 1e30, 1.0)   # thr * thr = +inf: every ray with finite Q stops at min_spp


def luminance(e):
    return (F(0.2126) * F(e[0]) + F(0.7152) * F(e[1])) + F(0.0722) * F(e[2])


def stop(C, Q, n, tolerance, floor):
    """the check after n samples with colour sum C (float32[3]) and sum of squared sample luminance Q"""
    with np.errstate(all="ignore"):
        fn = F(n)
        Y = luminance(C)
        m = Y / fn
        v = Q / fn - m * m
        if v < F(0):
            v = F(0)                       # a NaN stays a NaN
        vm = v / (fn - F(1.0))
        a = -m if m < F(0) else m
        b = a if a > F(floor) else F(floor)
        thr = F(tolerance) * b
        return bool(vm <= thr * thr)       # false with a NaN anywhere: keep sampling


def cut(cols, states, ad):
    """one ray: its samples' colours (>= max_spp rows) and the stream's state after each -> (rgb, n, Q, state) under the rule"""
    C = np.zeros(3, "<f4")
    Q = F(0)
    n = 0
    with np.errstate(all="ignore"):
        for k in range(ad.max_spp):
            e = cols[k]
            C = (C + e).astype("<f4")
            y = luminance(e)
            Q = F(Q + y * y)               # a sample that added nothing has e = 0: Q + 0 = Q
            n = k + 1
            if n >= ad.min_spp and n < ad.max_spp and (n - ad.min_spp) % ad.check_every == 0 and stop(C, Q, n, ad.tolerance, ad.floor):
                break
        return (C / F(n)).astype("<f4"), n, Q, states[n - 1]


def chains(osc, cases, spp, rr):
    """the oracle's part, computed once per scene and rr: {ray index: (colours float32[spp, 3], states)} for the rays inside
    the domain"""
    return {int(i): rc.sample_chain(osc, cases.cams[i][0], cases.cams[i][1], cases.seeds[i], spp, rr) for i in np.flatnonzero(cases.ok)}


def expected_from(chain, cases, ad):
    """-> (rgb float32[N, 3], spp uint32[N], m2 float32[N], states uint32[N]); a ray outside the domain: NaN NaN NaN, 0, 0 and
    its seed as given"""
    n = len(cases.rays)
    rgb = np.full((n, 3), np.nan, "<f4")
    spp = np.zeros(n, "<u4")
    m2 = np.zeros(n, "<f4")
    fin = cases.seeds.copy()
    for i, (cols, states) in chain.items():
        assert len(cols) >= ad.max_spp
        rgb[i], spp[i], m2[i], fin[i] = cut(cols, states, ad)
    return rgb, spp, m2, fin


def expected(osc, cases, ad, rr):
    return expected_from(chains(osc, cases, ad.max_spp, rr), cases, ad)


def near_lights(rng, flat, lo, hi, n, spread=0.2):
    """radiance_cases.at_lights with the aim widened: the direction jittered by `spread`, so that most of these rays land on a
    surface near a light and see it after one bounce every few samples -- the rays a stopping rule has to work on"""
    cams = rc.at_lights(rng, flat, lo, hi, n)
    z = cams[:, 1] + rng.normal(size=(n, 3)) * spread
    cams[:, 1] = (z / np.linalg.norm(z, axis=1, keepdims=True)).astype("<f4")
    return cams


def noisy(rng, flat, osc, lo, hi, n, trial=32):
    """-> (cams, seeds): rays near the lights chosen with the oracle, on the streams they are then traced with: of the first
    `trial` samples (rr 0.8) more than five and fewer than all carry light, one of the first four among them.  Such a ray does
    not stop black at a min_spp of four, and its mean takes tens of samples to settle: what runs on past min_spp"""
    out, seeds = [], []
    while len(out) < n:
        cams = np.concatenate([near_lights(rng, flat, lo, hi, n, s) for s in (0.1, 0.2, 0.3)])
        for (p, z), seed in zip(cams, rng.integers(1, 1 << 32, size=len(cams), dtype=np.uint64)):
            lit = (rc.sample_chain(osc, p, z, seed, trial, 0.8)[0] != 0).any(axis=1)
            if 5 < lit.sum() < trial and lit[:4].any() and len(out) < n:
                out.append(np.stack([p, z]))
                seeds.append(seed)
    return np.array(out, "<f4"), np.array(seeds, "<u4")


def cases_for(name, flat, osc, n, bad=8):
    """the rays of the adaptive tests: radiance_cases.mixed (all generators, `bad` rays outside the domain, one seed 0) for a
    quarter, then rays at the lights, probes just above a surface, and for half of the set noisy().  In these rooms the lights are
    small: a ray from anywhere is black in its first four samples nine times in ten and stops there, so the set leans on the
    rays that are not"""
    k = n // 8
    base = rc.mixed(name, flat, osc, n - 6 * k, bad=bad, salt=" adaptive")
    rng = np.random.default_rng(zlib.crc32(("adaptive " + name).encode()))
    lo, hi = rc.origin_box(flat)
    hard, hard_seeds = noisy(rng, flat, osc, lo, hi, 4 * k)
    cams = np.concatenate([rc.at_lights(rng, flat, lo, hi, k), rc.probes(rng, osc, lo, hi, k), hard])
    rays = np.array([np.concatenate(rc.pinhole(p, z)) for p, z in cams], "<f4")
    seeds = np.concatenate([rng.integers(1, 1 << 32, size=2 * k, dtype=np.uint64).astype("<u4"), hard_seeds])
    return rc.Cases(np.concatenate([base.rays, rays]), np.concatenate([base.seeds, seeds]), np.concatenate([base.cams, cams]),
                    np.concatenate([base.ok, np.ones(len(cams), bool)]))


def classes(spp, rgb, ok, ad):
    """fractions of the rays inside the domain: stopped at min_spp, strictly between, ran to max_spp; and, of those that stopped
    early, the fraction that is not black"""
    s = spp[ok]
    early = s < ad.max_spp
    lit = (rgb[ok][early] != 0).any(axis=1)
    return (s == ad.min_spp).mean(), ((s > ad.min_spp) & (s < ad.max_spp)).mean(), (s == ad.max_spp).mean(), lit.mean() if early.any() else 0.0


def assert_same(got, want, what):
    """got, want: (rgb, spp, m2, states), any of got's last three None (not asked for).  All bits; NaN outputs compare by
    position"""
    rc.assert_same(got[0], got[3], want[0], want[3], what)
    if got[1] is not None:
        bad = np.flatnonzero(np.asarray(got[1]) != want[1])
        assert len(bad) == 0, "%s: %d sample counts differ, first ray %d: %d vs %d" % (what, len(bad), bad[0], got[1][bad[0]], want[1][bad[0]])
    if got[2] is not None:
        g, w = np.ascontiguousarray(got[2], "<f4"), np.ascontiguousarray(want[2], "<f4")
        assert (np.isnan(g) == np.isnan(w)).all(), what + ": NaN second moments in other places"
        bad = np.flatnonzero((g.view("<u4") != w.view("<u4")) & ~np.isnan(w))
        assert len(bad) == 0, "%s: %d second moments differ bitwise, first ray %d: %r vs %r" % (what, len(bad), bad[0], g[bad[0]], w[bad[0]])


# ---- tools/host_sim --radiance-adaptive -------------------------------------------------------------------------------------------
def _bits(x):
    return "0x%08x" % int(np.array([x], "<f4").view("<u4")[0])


def host_sim_args(d, scene, rays, seeds, ad, rr, base=None):
    np.ascontiguousarray(rays, "<f4").tofile(os.path.join(d, "rays.f32"))
    np.ascontiguousarray(seeds, "<u4").tofile(os.path.join(d, "seeds.u32"))
    outs = [os.path.join(d, f) for f in ("ad_rgb.f32", "ad_spp.u32", "ad_m2.f32", "ad_states.u32")]
    return (["--radiance-adaptive"] + hs.scene_args(scene, base) + [os.path.join(d, "rays.f32"), os.path.join(d, "seeds.u32"), ad.min_spp, ad.max_spp,
                                                                     ad.check_every, _bits(ad.tolerance), _bits(ad.floor), repr(float(rr))] + outs, outs)


def host_sim(tool, d, scene, rays, seeds, ad, rr=RR, base=None, **kw):
    """-> (rgb (n, 3) float32, spp (n,) uint32, m2 (n,) float32, final states (n,) uint32)"""
    args, outs = host_sim_args(str(d), scene, rays, seeds, ad, rr, base)
    hs.run(tool, args, **kw)
    return np.fromfile(outs[0], "<f4").reshape(-1, 3), np.fromfile(outs[1], "<u4"), np.fromfile(outs[2], "<f4"), np.fromfile(outs[3], "<u4")
