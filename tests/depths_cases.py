"""Path-depth renders (ort_render_depths, ort_render_views_depths and their device forms) against the oracle as it stands: the
reference, the scenes and the guard values (test infrastructure, next to light_groups_cases.py, whose scenes and cameras these
are).

THE FOLD is the reference.  oracle_tiled_raytrace on a 1 x 1 rect at spp = 1 with an o_render_stats returns one sample's colour,
the stream's next state and `rays`, the sample's ray count: its last ray's depth + 1.  A pixel's job is the chain of such calls
from job_seed(seed, y*W + x); the sample's colour is what it added to the pixel's sum (or +0, which changes no bit of a sum), on
its last ray.  So, in float32 and in sample order,  B[bin(rays_k - 1)] += colour_k  and  N[bin(rays_k - 1)] += 1,  then B / spp.
Nothing of the call is restated: the chains come from the oracle, the fold is three lines.  A chain is recorded once per (scene,
camera, seed, frame size, window) at the largest sample count; a shorter job is its first samples, a rect is a part of it and
every bin count folds the same records."""
import ctypes as C
import os

import numpy as np

import host_sim_tool as hs
import light_groups_cases as lg

F = np.float32
W, H, RECT, SPPS, SEED, RR = lg.W, lg.H, lg.RECT, lg.SPPS, lg.SEED, lg.RR
BINS = (1, 3, 8)
MAX_BINS = 8
SCENES = ("room_all_lobes", "room_diffuse", "c2_analytic", lg.TABLE_SCENE)   # the table scene selects the kernels without LDS tables
ANALYTIC = SCENES[:3]
GUARD_F, GUARD_LEN, GUARD_STATE = F(-7.0), 0xEEEEEEEE, 0xDDDDDDDD   # what host_sim's planes start with, and the GPU tests' too
BATCH_SEEDS = lg.BATCH_SEEDS
batch_cameras, inside = lg.batch_cameras, lg.inside


def case(api, oracle, name, tmp_path_factory):
    """light_groups_cases' Case of the scene: the committed scene, its flattened arrays, its oracle scene and cameras"""
    return lg.case(api, oracle, name, tmp_path_factory)


class Chains:
    """the one-sample calls of every pixel of a window: colour (h, w, n, 3) float32, depth (h, w, n) of the sample's last ray,
    state (h, w, n) after the sample; h, w the window's"""

    def __init__(self, colour, depth, state):
        self.colour, self.depth, self.state = colour, depth, state
        for a in (colour, depth, state):
            a.setflags(write=False)


_chains = {}


def record(oracle, osc, cam, size, window, seed, n, rr=RR):
    """Chains of n samples a pixel, for the pixels of window (x0, y0, x1, y1) of a frame of size (w, h) from cam"""
    L = oracle.lib()
    w, h = size
    x0, y0, x1, y1 = window
    osc.set_camera(cam)
    colour = np.zeros((y1 - y0, x1 - x0, n, 3), "<f4")
    depth = np.zeros((y1 - y0, x1 - x0, n), np.int64)
    state = np.zeros((y1 - y0, x1 - x0, n), "<u4")
    one = np.zeros((h, w, 3), "<f4")
    for y in range(y0, y1):
        for x in range(x0, x1):
            s = C.c_uint32(oracle.job_seed(seed, y * w + x))
            for k in range(n):
                st = oracle.RenderStats()
                L.oracle_tiled_raytrace(osc.handle, C.byref(osc.camera), one.ctypes.data, w, h, x, y, x + 1, y + 1, C.byref(s), 1, rr, C.byref(st))
                assert st.paths == 1 and st.rays >= 1   # every call casts at least one ray
                colour[y - y0, x - x0, k] = one[y, x]
                depth[y - y0, x - x0, k] = st.rays - 1
                state[y - y0, x - x0, k] = s.value
    return Chains(colour, depth, state)


def chains(c, seed=SEED, cam=None, size=None, window=None, n=None, rr=RR):
    """the Chains of case c, recorded once: the scene's own camera, the module's frame, the whole frame and the largest sample
    count by default"""
    size = tuple(size) if size else (W, H)
    cam = c.camera(size) if cam is None else np.asarray(cam, "<f4").reshape(4, 3)
    window = tuple(window) if window else (0, 0) + size
    n = n if n else max(SPPS)
    key = (c.name, seed, cam.tobytes(), size, window, n, rr)
    if key not in _chains:
        _chains[key] = record(c.oracle, c.twin(None), cam, size, window, seed, n, rr)
    return _chains[key]


def fold(ch, G, spp):
    """-> (bins (G, h, w, 3) float32, lengths (G, h, w) uint32, rgb (h, w, 3) float32, states (h, w) uint32) of the jobs that are
    the chains' first spp samples; rgb is the G = 1 fold"""
    assert 1 <= G <= MAX_BINS and 1 <= spp <= ch.depth.shape[2]
    h, w = ch.depth.shape[:2]
    B, N, Cs = np.zeros((G, h, w, 3), "<f4"), np.zeros((G, h, w), "<u4"), np.zeros((h, w, 3), "<f4")
    with np.errstate(all="ignore"):
        for k in range(spp):
            b = np.minimum(ch.depth[:, :, k], G - 1)
            for g in range(G):
                m = b == g
                B[g][m] = B[g][m] + ch.colour[:, :, k][m]
                N[g][m] += 1
            Cs = Cs + ch.colour[:, :, k]
        return B / F(spp), N, Cs / F(spp), ch.state[:, :, spp - 1].copy()


def expected(c, G, spp, seed=SEED, cam=None, size=None, window=None):
    """-> [bins, lengths, rgb, states]: the fold of case c's chains laid into whole planes of the frame, zeros outside the window.
    A rect is a part of them: assert_plane reads nothing outside it"""
    size = tuple(size) if size else (W, H)
    w, h = size
    x0, y0, x1, y1 = window if window else (0, 0, w, h)
    B, N, rgb, st = fold(chains(c, seed, cam, size, window), G, spp)
    full = [np.zeros((G, h, w, 3), "<f4"), np.zeros((G, h, w), "<u4"), np.zeros((h, w, 3), "<f4"), np.zeros((h, w), "<u4")]
    full[0][:, y0:y1, x0:x1], full[1][:, y0:y1, x0:x1], full[2][y0:y1, x0:x1], full[3][y0:y1, x0:x1] = B, N, rgb, st
    return full


def bits(a):
    return np.ascontiguousarray(a).view("<u4")


def assert_plane(got, want, rect, guard, what, size=None, nan_by_position=False):
    """got (..., h, w[, 3]) equals want bit for bit inside rect and still holds guard outside it.  nan_by_position: a NaN of want
    is matched by any NaN of got (a NaN's payload is not part of any contract), every other word bit for bit"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    w, h = size if size else (W, H)
    m = inside(rect, (w, h))
    colour = got.ndim >= 3 and got.shape[-1] == 3 and got.shape[-3:-1] == (h, w)
    g, wt = bits(got), bits(want)
    gi, wi, go = (g[..., m, :], wt[..., m, :], g[..., ~m, :]) if colour else (g[..., m], wt[..., m], g[..., ~m])
    bad = gi != wi
    if nan_by_position:
        gf, wf = (got[..., m, :], want[..., m, :]) if colour else (got[..., m], want[..., m])
        bad &= ~(np.isnan(gf) & np.isnan(wf))
    assert not bad.any(), "%s: %d of %d words inside the rect differ; first %r" % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))
    gw = np.array(guard, got.dtype).reshape(1).view("<u4")[0]
    assert (go == gw).all(), "%s: %d words outside the rect were written" % (what, int((go != gw).sum()))


def assert_planes(got, want, rect, what, size=None, nan_by_position=False):
    """got: (bins, rgb or None, lengths or None, states or None) of one view; want: expected()'s four planes"""
    names, guards = ("bins", "lengths", "rgb", "states"), (GUARD_F, GUARD_LEN, GUARD_F, GUARD_STATE)
    bins_, rgb, lengths, states = got
    for name, guard, g, w in zip(names, guards, (bins_, lengths, rgb, states), want):
        if g is not None:
            assert_plane(g, w, rect, guard, "%s: %s" % (what, name), size, nan_by_position and name in ("bins", "rgb"))


# ---- tools/host_sim --depths -------------------------------------------------------------------------------------------------
def host_depths(tool, d, c, G, spp, seed=SEED, rect=None, cams=None, seeds=None, want=("rgb", "lengths", "states"), **kw):
    """-> (bins (V, G, H, W, 3), rgb (V, H, W, 3) or None, lengths (V, G, H, W) or None, states (V, H, W) or None); cams None: the
    single-frame form (V = 1)"""
    d = str(d)
    if cams is not None:
        np.ascontiguousarray(cams, "<f4").tofile(os.path.join(d, "cams.f32"))
        np.ascontiguousarray(seeds, "<u4").tofile(os.path.join(d, "vseeds.u32"))
    V = 1 if cams is None else len(cams)
    x0, y0, x1, y1 = rect if rect else (0, 0, W, H)
    outs = [os.path.join(d, n) for n in ("bins.f32", "rgb.f32", "lengths.u32", "states.u32")]
    for o in outs:
        if os.path.exists(o):
            os.remove(o)
    args = ["--depths"] + c.hs_args() + [os.path.join(d, "cams.f32") if cams is not None else "-",
                                         os.path.join(d, "vseeds.u32") if cams is not None else seed,
                                         W, H, x0, y0, x1, y1, spp, repr(float(RR)), G, outs[0]]
    args += [o if n in want else "-" for n, o in zip(("rgb", "lengths", "states"), outs[1:])]
    r = hs.run(tool, args, **kw)
    return (np.fromfile(outs[0], "<f4").reshape(V, G, H, W, 3),
            np.fromfile(outs[1], "<f4").reshape(V, H, W, 3) if "rgb" in want else None,
            np.fromfile(outs[2], "<u4").reshape(V, G, H, W) if "lengths" in want else None,
            np.fromfile(outs[3], "<u4").reshape(V, H, W) if "states" in want else None), r
