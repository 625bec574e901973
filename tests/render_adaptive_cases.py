"""The adaptive camera render (ort_render_adaptive, ort_render_views_adaptive) against the oracle as it stands (test
infrastructure).  Per pixel, oracle_tiled_raytrace on the rect (x, y, x+1, y+1) with spp = 1, chained through the returned
stream state from job_seed(seed, y*W + x), gives each camera sample's colour and the state after it; adaptive_cases.cut -- the
stopping rule of include/ort.h restated in numpy float32 -- cuts the chain.  A chain of the largest max_spp serves every
parameter set: a set with a smaller max_spp reads a prefix of it."""
import os

import numpy as np

import adaptive_cases as ac
import host_sim_tool as hs
import oracle_lib
from adaptive_cases import Adaptive

# FRAME: the main set of the frame tests (tests/test_render_adaptive_host.py holds its three classes of pixels from the oracle
# alone); EVERY checks after every sample, the last check at 16; FIXED never checks
FRAME = Adaptive(8, 64, 8, 0.3, 0.05)
EVERY = ac.EVERY
FIXED = ac.FIXED
SETS = (FRAME, EVERY, FIXED)
HUGE = Adaptive(8, 64, 8, 1e30, 1.0)   # thr * thr = +inf: every pixel with finite Q stops at min_spp
W, H, SEED, RR = 24, 16, 2024, 0.8
MAX_SPP = 64
# what a plane holds where nothing was written: tools/host_sim --render-adaptive starts its planes at these
GUARDS = (np.float32(-7.0), 0xEEEEEEEE, np.float32(-1.0), 0xDDDDDDDD)


def pixel_chain(osc, w, h, x, y, seed, spp, rr):
    """-> (colours float32[spp, 3], states after each sample) of pixel (x, y): spp chained spp = 1 calls on the pixel's stream"""
    s = oracle_lib.job_seed(seed, y * w + x)
    img = np.zeros((h, w, 3), "<f4")
    cols = np.zeros((spp, 3), "<f4")
    states = np.zeros(spp, "<u4")
    for k in range(spp):
        _, s = osc.tiled_raytrace(img, x, y, x + 1, y + 1, s, 1, rr)
        cols[k] = img[y, x]
        states[k] = s
    return cols, states


def chains(osc, w, h, seed, rr, rect=None, spp=MAX_SPP):
    """{(x, y): (colours, states)} for the pixels of rect (the whole frame by default), with the oracle's camera as it is set"""
    x0, y0, x1, y1 = rect if rect else (0, 0, w, h)
    return {(x, y): pixel_chain(osc, w, h, x, y, seed, spp, rr) for y in range(y0, y1) for x in range(x0, x1)}


def expected_from(chain, w, h, ad, guards=(0, 0, 0, 0)):
    """-> (rgb (h, w, 3) float32, spp (h, w) uint32, m2 (h, w) float32, states (h, w) uint32); pixels without a chain (outside
    the rect) hold `guards`"""
    rgb = np.full((h, w, 3), guards[0], "<f4")
    spp = np.full((h, w), guards[1], "<u4")
    m2 = np.full((h, w), guards[2], "<f4")
    fin = np.full((h, w), guards[3], "<u4")
    for (x, y), (cols, states) in chain.items():
        assert len(cols) >= ad.max_spp
        rgb[y, x], spp[y, x], m2[y, x], fin[y, x] = ac.cut(cols, states, ad)
    return rgb, spp, m2, fin


def classes(spp, rgb, ad):
    """fractions of the pixels: stopped at min_spp, strictly between, ran to max_spp; and, of the early-stopped, not black"""
    s = spp.reshape(-1)
    early = s < ad.max_spp
    lit = (rgb.reshape(-1, 3)[early] != 0).any(axis=1)
    return (s == ad.min_spp).mean(), ((s > ad.min_spp) & (s < ad.max_spp)).mean(), (s == ad.max_spp).mean(), lit.mean() if early.any() else 0.0


def assert_same(got, want, what):
    """got, want: (rgb, spp, m2, states) planes of one shape, any of got's last three None (not asked for).  All bits."""
    names = ("colours", "sample counts", "second moments", "final states")
    for g, w_, name in zip(got, want, names):
        if g is None:
            continue
        g, w_ = np.ascontiguousarray(g), np.ascontiguousarray(w_)
        assert g.shape == w_.shape and g.dtype.itemsize == 4 and w_.dtype.itemsize == 4, "%s: %s %s vs %s" % (what, name, g.shape, w_.shape)
        ne = g.view("<u4") != w_.view("<u4")
        if ne.any():
            at = tuple(np.argwhere(ne)[0])
            raise AssertionError("%s: %d of %d %s differ bitwise; first at %s: %r vs %r" % (what, int(ne.sum()), ne.size, name, at, g[at], w_[at]))


# ---- tools/host_sim --render-adaptive ---------------------------------------------------------------------------------------
def host_sim_args(d, scene, w, h, rect, seed, ad, rr, base=None):
    outs = [os.path.join(d, f) for f in ("ra_rgb.f32", "ra_spp.u32", "ra_m2.f32", "ra_states.u32")]
    x0, y0, x1, y1 = rect if rect else (0, 0, w, h)
    return (["--render-adaptive"] + hs.scene_args(scene, base) + [w, h, x0, y0, x1, y1, seed, ad.min_spp, ad.max_spp, ad.check_every,
                                                                  ac._bits(ad.tolerance), ac._bits(ad.floor), repr(float(rr))] + outs, outs)


def host_sim(tool, d, scene, w, h, rect, seed, ad, rr=RR, base=None, **kw):
    """-> the four planes as the tool wrote them (GUARDS where it wrote nothing)"""
    args, outs = host_sim_args(str(d), scene, w, h, rect, seed, ad, rr, base)
    hs.run(tool, args, **kw)
    return (np.fromfile(outs[0], "<f4").reshape(h, w, 3), np.fromfile(outs[1], "<u4").reshape(h, w), np.fromfile(outs[2], "<f4").reshape(h, w),
            np.fromfile(outs[3], "<u4").reshape(h, w))
