"""Sample-map renders (ort_render_sample_map, ort_render_views_sample_map and their device forms) against the oracle as it
stands: the maps, the reference and the guard values (test infrastructure, next to render_adaptive_cases.py).

THE REFERENCE is render_adaptive_cases.chains: per pixel, spp = 1 oracle calls chained on the pixel's own stream.  Pixel i's
planes are adaptive_cases.cut(cols, states, Adaptive(n_i, n_i, 1, 0, 0)) with n_i = min(map_i, cap): a rule that never checks,
so the chain's first n_i samples, their mean, their sum of squared luminance and the state after them.  A pixel with n_i = 0, or
outside the rect, keeps its guard words.  Nothing of the call is restated.  The scenes are light_groups_cases' (its Case holds
the committed scene and the oracle's scene); a chain of CAP samples per pixel and (scene, camera, seed) is computed once."""
import os

import numpy as np

import adaptive_cases as ac
import host_sim_tool as hs
import light_groups_cases as lg
import render_adaptive_cases as rac
from adaptive_cases import Adaptive

W, H = 24, 16            # 3 x 2 blocks of 8 x 8: partial in both directions
CAP = 16
SEED = 2024
RR = 0.8
RECT = (3, 2, 21, 13)
VALUES = (0, 1, 2, 3, 5, 16, 17, 0xFFFFFFFF)
SCENES = ("room_diffuse", "room_all_lobes", "c4_dwarf_room", lg.TABLE_SCENE)
# what a plane holds where nothing was written: tools/host_sim --sample-map starts its planes at these, and the GPU tests too
GUARD_RGB, GUARD_M2, GUARD_STATE = np.float32(-7.0), np.float32(-1.0), 0xDDDDDDDD
ZERO_BLOCK = (8, 0)      # the 8 x 8 block at x 8..15, y 0..7: six of its rows lie inside RECT
ZERO_ROW = 10
BATCH_SEEDS = lg.BATCH_SEEDS
assert (lg.W, lg.H, lg.RR) == (W, H, RR)


def base_map(shift=0):
    """every value of VALUES, laid out so that horizontal and vertical neighbours differ: the index steps by 1 along x and by
    3 along y, modulo 8"""
    y, x = np.mgrid[0:H, 0:W]
    return np.array(VALUES, "<u4")[(x + 3 * y + shift) % len(VALUES)]


def border(rect):
    """the pixels of rect's outermost ring"""
    x0, y0, x1, y1 = rect
    m = np.zeros((H, W), bool)
    m[y0:y1, x0:x1] = True
    m[y0 + 1:y1 - 1, x0 + 1:x1 - 1] = False
    return m


def mixed_map(shift=0):
    """base_map with one whole 8 x 8 block of zeros, one row of zeros, and a zero on every other pixel of RECT's border"""
    m = base_map(shift)
    bx, by = ZERO_BLOCK
    m[by:by + 8, bx:bx + 8] = 0
    m[ZERO_ROW, :] = 0
    y, x = np.mgrid[0:H, 0:W]
    m[border(RECT) & ((x + y) % 2 == 0)] = 0
    return m


def counts(smap, cap=CAP):
    """n = min(map, cap), as the lanes cut it"""
    return np.minimum(np.asarray(smap, "<u4"), np.uint32(cap)).astype("<u4")


def inside(rect):
    return lg.inside(rect)


_chains = {}


def chains(c, seed=SEED, cam=None):
    """{(x, y): (colours float32[CAP, 3], states)} of case c's whole frame from cam (the scene's own by default), once"""
    cam = c.cam if cam is None else np.asarray(cam, "<f4").reshape(4, 3)
    key = (c.name, seed, cam.tobytes())
    if key not in _chains:
        osc = c.twin(None)
        osc.set_camera(cam)
        _chains[key] = rac.chains(osc, W, H, seed, RR, None, CAP)
    return _chains[key]


def expected(c, smap, cap=CAP, seed=SEED, cam=None, rect=None):
    """-> (rgb (H, W, 3) float32, m2 (H, W) float32, states (H, W) uint32): the oracle's planes where n >= 1 inside rect, the
    guards elsewhere"""
    n = counts(smap, cap)
    rgb = np.full((H, W, 3), GUARD_RGB, "<f4")
    m2 = np.full((H, W), GUARD_M2, "<f4")
    fin = np.full((H, W), GUARD_STATE, "<u4")
    m = inside(rect)
    for (x, y), (cols, states) in chains(c, seed, cam).items():
        k = int(n[y, x])
        if k == 0 or not m[y, x]:
            continue
        rgb[y, x], took, m2[y, x], fin[y, x] = ac.cut(cols, states, Adaptive(k, k, 1, 0, 0))
        assert took == k
    return rgb, m2, fin


def assert_planes(got, want, what):
    """got: (rgb, m2 or None, states or None), want: expected()'s three; every word, so the guards where nothing may be written too"""
    for g, w_, name in zip(got, want, ("colours", "second moments", "final states")):
        if g is None:
            continue
        g, w_ = np.ascontiguousarray(g), np.ascontiguousarray(w_)
        assert g.shape == w_.shape and g.dtype.itemsize == 4, "%s: %s %s vs %s" % (what, name, g.shape, w_.shape)
        ne = g.view("<u4") != w_.view("<u4")
        if ne.any():
            at = tuple(np.argwhere(ne)[0])
            raise AssertionError("%s: %d of %d %s differ bitwise; first at %s: %r vs %r" % (what, int(ne.sum()), ne.size, name, at, g[at], w_[at]))


def guards(V=None, want_m2=True, want_states=True):
    """the host planes of a call, every word a guard value"""
    lead = () if V is None else (V,)
    return ([np.full(lead + (H, W, 3), GUARD_RGB, "<f4")] + ([np.full(lead + (H, W), GUARD_M2, "<f4")] if want_m2 else []) +
            ([np.full(lead + (H, W), GUARD_STATE, "<u4")] if want_states else []))


def batch_cameras(api, c):
    return lg.batch_cameras(api, c)


# ---- tools/host_sim --sample-map --------------------------------------------------------------------------------------------
def host_sample_map(tool, d, c, smap, cap=CAP, seed=SEED, rect=None, cams=None, seeds=None, want_m2=True, want_states=True, **kw):
    """-> ((rgb (V, H, W, 3), m2 (V, H, W) or None, states (V, H, W) or None), the run); cams None: the single-frame form (V = 1)"""
    d = str(d)
    np.ascontiguousarray(smap, "<u4").tofile(os.path.join(d, "map.u32"))
    if cams is not None:
        np.ascontiguousarray(cams, "<f4").tofile(os.path.join(d, "cams.f32"))
        np.ascontiguousarray(seeds, "<u4").tofile(os.path.join(d, "vseeds.u32"))
    V = 1 if cams is None else len(cams)
    x0, y0, x1, y1 = rect if rect else (0, 0, W, H)
    outs = [os.path.join(d, n) for n in ("sm_rgb.f32", "sm_m2.f32", "sm_states.u32")]
    for o in outs:
        if os.path.exists(o):
            os.remove(o)
    args = ["--sample-map"] + c.hs_args() + [os.path.join(d, "cams.f32") if cams is not None else "-",
                                              os.path.join(d, "vseeds.u32") if cams is not None else seed,
                                              W, H, x0, y0, x1, y1, cap, repr(float(RR)), os.path.join(d, "map.u32"),
                                              outs[0], outs[1] if want_m2 else "-", outs[2] if want_states else "-"]
    r = hs.run(tool, args, **kw)
    return (np.fromfile(outs[0], "<f4").reshape(V, H, W, 3),
            np.fromfile(outs[1], "<f4").reshape(V, H, W) if want_m2 else None,
            np.fromfile(outs[2], "<u4").reshape(V, H, W) if want_states else None), r
