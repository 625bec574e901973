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


def base_map(shift=0, size=None, values=VALUES):
    """every value of `values`, laid out so that horizontal and vertical neighbours differ: the index steps by 1 along x and by
    3 along y, modulo their number (8 for VALUES); size: (w, h), the module's 24 x 16 by default"""
    w, h = size if size else (W, H)
    y, x = np.mgrid[0:h, 0:w]
    return np.array(values, "<u4")[(x + 3 * y + shift) % len(values)]


def border(rect, size=None):
    """the pixels of rect's outermost ring"""
    w, h = size if size else (W, H)
    x0, y0, x1, y1 = rect
    m = np.zeros((h, w), bool)
    m[y0:y1, x0:x1] = True
    m[y0 + 1:y1 - 1, x0 + 1:x1 - 1] = False
    return m


def mixed_map(shift=0, size=None, values=VALUES, rect=RECT, zero_block=ZERO_BLOCK, zero_row=ZERO_ROW):
    """base_map with one whole 8 x 8 block of zeros, one row of zeros, and a zero on every other pixel of rect's border"""
    w, h = size if size else (W, H)
    m = base_map(shift, size, values)
    bx, by = zero_block
    m[by:by + 8, bx:bx + 8] = 0
    m[zero_row, :] = 0
    y, x = np.mgrid[0:h, 0:w]
    m[border(rect, size) & ((x + y) % 2 == 0)] = 0
    return m


def counts(smap, cap=CAP):
    """n = min(map, cap), as the lanes cut it"""
    return np.minimum(np.asarray(smap, "<u4"), np.uint32(cap)).astype("<u4")


def inside(rect, size=None):
    return lg.inside(rect, size)


_chains = {}


def chains(c, seed=SEED, cam=None, size=None, window=None, cap=CAP):
    """{(x, y): (colours float32[cap, 3], states)} of case c's frame from cam (the scene's own by default), once; size: (w, h),
    the module's 24 x 16 by default; window: the pixels that get a chain, the whole frame by default"""
    w, h = size if size else (W, H)
    cam = c.camera(size) if cam is None else np.asarray(cam, "<f4").reshape(4, 3)
    key = (c.name, seed, cam.tobytes(), (w, h), window, cap)
    if key not in _chains:
        osc = c.twin(None)
        osc.set_camera(cam)
        _chains[key] = rac.chains(osc, w, h, seed, RR, window, cap)
    return _chains[key]


def expected_from(chain, smap, cap=CAP, rect=None, size=None):
    """{(x, y): (colours, states)} of the pixels the oracle answers for, each at least min(cap, its count) samples long -> (rgb
    (h, w, 3) float32, m2 (h, w) float32, states (h, w) uint32): the chain cut at n = min(map, cap) where n >= 1 inside rect,
    the guards elsewhere"""
    w, h = size if size else (W, H)
    n = counts(smap, cap)
    rgb = np.full((h, w, 3), GUARD_RGB, "<f4")
    m2 = np.full((h, w), GUARD_M2, "<f4")
    fin = np.full((h, w), GUARD_STATE, "<u4")
    m = inside(rect, size)
    for (x, y), (cols, states) in chain.items():
        k = int(n[y, x])
        if k == 0 or not m[y, x]:
            continue
        rgb[y, x], took, m2[y, x], fin[y, x] = ac.cut(cols, states, Adaptive(k, k, 1, 0, 0))
        assert took == k
    return rgb, m2, fin


def expected(c, smap, cap=CAP, seed=SEED, cam=None, rect=None, size=None, window=None, chain=CAP):
    """-> (rgb (h, w, 3) float32, m2 (h, w) float32, states (h, w) uint32): the oracle's planes where n >= 1 inside rect, the
    guards elsewhere; with a window, the oracle's planes inside it alone (a large frame is held against it window by window);
    chain: the samples a pixel's chain holds, at least min(cap, the map's largest count)"""
    return expected_from(chains(c, seed, cam, size, window, chain), smap, cap, rect, size)


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


def guards(V=None, want_m2=True, want_states=True, size=None):
    """the host planes of a call, every word a guard value"""
    w, h = size if size else (W, H)
    lead = () if V is None else (V,)
    return ([np.full(lead + (h, w, 3), GUARD_RGB, "<f4")] + ([np.full(lead + (h, w), GUARD_M2, "<f4")] if want_m2 else []) +
            ([np.full(lead + (h, w), GUARD_STATE, "<u4")] if want_states else []))


def batch_cameras(api, c, size=None):
    return lg.batch_cameras(api, c, size)


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
