"""Accumulating renders (ort_render_accumulate, ort_render_views_accumulate and their device forms): the planes, the reference
and the scenarios that the host tests (tools/host_sim --accumulate) and the GPU tests share (test infrastructure, next to
sample_map_cases.py).

THE REFERENCE is never the code under test: per pixel, spp = 1 oracle calls chained on the pixel's own stream
(sample_map_cases.chains, which is render_adaptive_cases.chains), or the reference's own chains (tests/golden/chains_rooms.npz),
FOLDED with separately rounded float32 adds into the undivided sum: fold() is adaptive_cases.cut's sibling that returns C where
cut returns C / n.  model() applies include/ort.h's contract for a sequence of calls to such chains and gives all five planes.

A scenario takes `call`, which runs ONE accumulating call on a Planes in place -- through the lane code on host threads or
through the library on a device -- and is the same for both.  Every comparison is on every 32-bit word of every plane."""
import os

import numpy as np

import adaptive_cases as ac
import host_sim_tool as hs
import sample_map_cases as sm
from hostile_materials import same_words

F = np.float32
W, H, CAP, SEED, RR, RECT = sm.W, sm.H, sm.CAP, sm.SEED, sm.RR, sm.RECT
SMALL_RECT = (5, 4, 17, 11)
LIMIT = 1 << 24
SPLIT = (1, 2, 5, 8)          # 16 samples
REF_SPLIT = (1, 3, 12, 48)    # 64 samples: the whole of a reference chain
# what a plane holds where nothing was written.  count has no guard: a caller starts it at zero, and the call reads it
GUARD_SUM = np.array([0x7FC00123], "<u4").view("<f4")[0]   # a NaN: a fresh pixel's sum is not read
GUARD_M2, GUARD_STATE, GUARD_RGB = sm.GUARD_M2, sm.GUARD_STATE, sm.GUARD_RGB
NAMES = ("sum_rgb", "m2", "count", "states", "out_rgb")


class Planes:
    """the four planes of the caller's and the frame, V frames each: sum (V, H, W, 3), m2, count, states (V, H, W), rgb (V, H, W, 3)"""

    def __init__(self, V=1, size=None):
        w, h = size if size else (W, H)
        self.sum = np.full((V, h, w, 3), GUARD_SUM, "<f4")
        self.m2 = np.full((V, h, w), GUARD_M2, "<f4")
        self.count = np.zeros((V, h, w), "<u4")
        self.states = np.full((V, h, w), GUARD_STATE, "<u4")
        self.rgb = np.full((V, h, w, 3), GUARD_RGB, "<f4")

    def all(self):
        return (self.sum, self.m2, self.count, self.states, self.rgb)

    def copy(self):
        p = Planes.__new__(Planes)
        p.sum, p.m2, p.count, p.states, p.rgb = (a.copy() for a in self.all())
        return p


def assert_planes(got, want, what, skip=(), nan=False):
    """every word of the five planes; skip: names of planes the call was not given (the caller holds those against their guards).
    nan: the chains hold NaN (hostile materials), so the float planes go through hostile_materials.same_words -- equal bits, or a
    NaN in both -> the NaN words expected in sum_rgb, m2 and out_rgb (0 without nan)"""
    nans = 0
    for g, w_, name in zip(got.all(), want.all(), NAMES):
        if name in skip:
            continue
        assert g.shape == w_.shape and g.dtype == w_.dtype, "%s: %s %s vs %s" % (what, name, g.shape, w_.shape)
        if nan:
            nans += same_words(g, w_, "%s: %s" % (what, name))
            continue
        ne = np.ascontiguousarray(g).view("<u4") != np.ascontiguousarray(w_).view("<u4")
        if ne.any():
            at = tuple(np.argwhere(ne)[0])
            raise AssertionError("%s: %d of %d words of %s differ; first at %s: %r vs %r" % (what, int(ne.sum()), ne.size, name, at, g[at], w_[at]))
    return nans


# ---- the reference ---------------------------------------------------------------------------------------------------------
def fold(cols, C, Q, k0, k1):
    """samples k0 .. k1 - 1 of a chain added to (C float32[3], Q float32), each add rounded on its own -> (C, Q)"""
    C = np.array(C, "<f4")
    Q = F(Q)
    with np.errstate(all="ignore"):
        for k in range(k0, k1):
            e = cols[k]
            C = (C + e).astype("<f4")
            y = ac.luminance(e)
            Q = F(Q + y * y)
    return C, Q


def adds(count, smap, cap, rect, size=None):
    """the contract's add for every pixel of one frame: min(asked, cap, LIMIT - min(n0, LIMIT)) inside rect, 0 outside"""
    asked = np.full(count.shape, cap, np.int64) if smap is None else np.asarray(smap, "<u4").astype(np.int64)
    room = LIMIT - np.minimum(count.astype(np.int64), LIMIT)
    return np.where(sm.inside(rect, size), np.minimum(np.minimum(asked, cap), room), 0)


def model(planes, v, chain, smap, cap, rect, use_m2=True, want_rgb=True, offset=None, size=None):
    """one call applied to frame v of planes, in place, by the contract and the chain {(x, y): (colours, states)}: a fresh pixel's
    samples are the chain's first, a continued pixel's those after count - offset[y, x] (offset: the count a hostile pixel
    started with, whose chain starts at its own state; 0 by default).  use_m2 False: Q is not carried"""
    add = adds(planes.count[v], smap, cap, rect, size)
    for (x, y), (cols, states) in chain.items():
        a = int(add[y, x])
        if a == 0:
            continue
        n0 = int(planes.count[v, y, x])
        k0 = n0 - (int(offset[y, x]) if offset is not None else 0)
        C0, Q0 = (planes.sum[v, y, x], planes.m2[v, y, x]) if n0 else (np.zeros(3, "<f4"), F(0))
        if not use_m2:
            Q0 = F(0)
        assert k0 + a <= len(cols), "the chain of pixel %r is %d samples long, %d asked for" % ((x, y), len(cols), k0 + a)
        C, Q = fold(cols, C0, Q0, k0, k0 + a)
        planes.sum[v, y, x] = C
        if use_m2:
            planes.m2[v, y, x] = Q
        planes.count[v, y, x] = n0 + a
        planes.states[v, y, x] = states[k0 + a - 1]
        if want_rgb:
            with np.errstate(all="ignore"):
                planes.rgb[v, y, x] = (C / F(n0 + a)).astype("<f4")
    assert int(add.sum()) == sum(int(add[y, x]) for (x, y) in chain), "a pixel that takes samples has no chain"
    return int(add.sum())


def chain_from_state(c, x, y, state, n, cam=None, size=None):
    """n oracle calls of one sample each on pixel (x, y), chained from `state` -> (colours float32[n, 3], states)"""
    w, h = size if size else (W, H)
    osc = c.twin(None)
    osc.set_camera(c.camera(size) if cam is None else np.asarray(cam, "<f4").reshape(4, 3))
    img = np.zeros((h, w, 3), "<f4")
    cols, states, s = np.zeros((n, 3), "<f4"), np.zeros(n, "<u4"), int(state)
    for k in range(n):
        _, s = osc.tiled_raytrace(img, x, y, x + 1, y + 1, s, 1, RR)
        cols[k], states[k] = img[y, x], s
    return cols, states


# ---- tools/host_sim --accumulate --------------------------------------------------------------------------------------------
def host_call(tool, d, c, size=None, **run_kw):
    """-> call(planes, smap, cap, rect=None, seed=SEED, cams=None, seeds=None, use_m2=True, want_rgb=True), which runs one
    accumulating call on planes in place and returns the paths it counted (a call that does not count returns None)"""
    d = str(d)
    w, h = size if size else (W, H)

    def call(planes, smap, cap, rect=None, seed=SEED, cams=None, seeds=None, use_m2=True, want_rgb=True):
        files = [os.path.join(d, n) for n in ("acc_sum.f32", "acc_m2.f32", "acc_count.u32", "acc_states.u32", "acc_rgb.f32", "acc_map.u32")]
        for a, f in zip(planes.all(), files):
            np.ascontiguousarray(a).tofile(f)
        if smap is not None:
            np.ascontiguousarray(smap, "<u4").tofile(files[5])
        if cams is not None:
            np.ascontiguousarray(cams, "<f4").tofile(os.path.join(d, "cams.f32"))
            np.ascontiguousarray(seeds, "<u4").tofile(os.path.join(d, "vseeds.u32"))
        x0, y0, x1, y1 = rect if rect else (0, 0, w, h)
        args = ["--accumulate"] + c.hs_args() + [os.path.join(d, "cams.f32") if cams is not None else "-",
                                                 os.path.join(d, "vseeds.u32") if cams is not None else seed, w, h, x0, y0, x1, y1, cap,
                                                 repr(float(RR)), files[5] if smap is not None else "-", files[0], files[1] if use_m2 else "-",
                                                 files[2], files[3], files[4] if want_rgb else "-"]
        r = hs.run(tool, args, **run_kw)
        for a, f in zip(planes.all(), files):
            a[...] = np.fromfile(f, a.dtype).reshape(a.shape)
        return hs.counters(r)["paths"]
    return call


# ---- the library, host form ----------------------------------------------------------------------------------------------------
def library_call(api, c, size=None, counters=True):
    """the same call through Scene.render_accumulate / render_views_accumulate on an uploaded scene; without counters the
    call returns None where the others return the paths counted"""
    w, h = size if size else (W, H)

    def call(planes, smap, cap, rect=None, seed=SEED, cams=None, seeds=None, use_m2=True, want_rgb=True):
        V = planes.count.shape[0]
        acc = api.Accumulator(w, h, None if cams is None else V)
        lead = (lambda a: a[0]) if cams is None else (lambda a: a)
        acc.sum_rgb, acc.m2, acc.count, acc.states = (np.ascontiguousarray(lead(a)) for a in (planes.sum, planes.m2, planes.count, planes.states))
        out = np.ascontiguousarray(lead(planes.rgb)) if want_rgb else None
        add = cap if smap is None else np.asarray(smap, "<u4").reshape(acc.count.shape)
        if cams is None:
            st = c.scene.render_accumulate(acc, add, seed, cap, rect, RR, counters, use_m2, out)
        else:
            st = c.scene.render_views_accumulate(cams, seeds, acc, add, cap, rect, RR, counters, use_m2, out)
        for mine, theirs in zip(planes.all(), (acc.sum_rgb, acc.m2, acc.count, acc.states, out)):
            if theirs is not None:
                lead(mine)[...] = theirs
        return st["paths"] if counters else None
    return call


# ---- the library, device forms: planes in device memory with guard words around them ---------------------------------------------
PAD, PAD_WORD = 16, 0xABABABAB


class DevicePlanes:
    """the five planes of a Planes as torch tensors on device 0, PAD guard words before and after each; ptr: the planes' device
    addresses in Planes.all()'s order.  Made inside the caller's stream context, so the uploads are ordered with its launches"""

    def __init__(self, planes):
        import torch
        self.shape_of = planes
        self.t = []
        for a in planes.all():
            words = np.ascontiguousarray(a).view("<u4").reshape(-1)
            whole = np.concatenate([np.full(PAD, PAD_WORD, "<u4"), words, np.full(PAD, PAD_WORD, "<u4")]).view("<i4")
            self.t.append(torch.from_numpy(whole).to(torch.device("cuda", 0)))
        self.ptr = [x.data_ptr() + 4 * PAD for x in self.t]

    def download(self):
        """-> Planes; asserts that no guard word around a plane was written.  The caller has synchronised"""
        got = self.shape_of.copy()
        for x, g in zip(self.t, got.all()):
            words = x.cpu().numpy().view("<u4")
            assert (words[:PAD] == PAD_WORD).all() and (words[-PAD:] == PAD_WORD).all(), "a guard word around a plane was written"
            g[...] = words[PAD:-PAD].view(g.dtype).reshape(g.shape)
        return got


def stream_split(c, split, seed=SEED, size=None):
    """the passes of `split` -- no map, the whole frame, from count == 0 -- through ort_render_accumulate_device (every second pass
    through ort_render_views_accumulate_device as a batch of one view, the scene's own camera) on a non-default stream, stats ==
    NULL, no synchronisation between the passes and one at the end -> Planes.  A continued pass reads the sums, m2, counts and
    states the pass before it wrote, in stream order"""
    import torch
    w, h = size if size else (W, H)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    with torch.cuda.stream(stream):
        d = DevicePlanes(Planes(size=size))
        for k, n in enumerate(split):
            p = c.scene.params(w, h, n, seed, "pixel", 0, None, RR)
            args = dict(d_m2=d.ptr[1], d_map=0, d_rgb=d.ptr[4], stream=stream.cuda_stream)
            if k % 2:
                st = c.scene.render_views_accumulate_device(p, np.asarray(c.camera(size), "<f4")[None], [seed], d.ptr[0], d.ptr[2], d.ptr[3], **args)
            else:
                st = c.scene.render_accumulate_device(p, d.ptr[0], d.ptr[2], d.ptr[3], **args)
            assert st is None
    torch.cuda.synchronize()
    return d.download()


def views_split(call, c, cams, seeds, split, what, nan=False, single=None):
    """the passes of `split` through the views form on a batch: frame v against the oracle's chains from that camera and seed,
    folded by model(); single: the planes of the single-frame form after the same passes, which a frame from the scene's own
    camera on SEED must equal (frame 0 of the matrices' batches)"""
    got, want = Planes(len(cams)), Planes(len(cams))
    for n in split:
        call(got, None, n, cams=cams, seeds=seeds)
        for v in range(len(cams)):
            model(want, v, sm.chains(c, int(seeds[v]), cams[v], cap=sum(split)), None, n, None)
    assert_planes(got, want, what + ": against the oracle, view by view", nan=nan)
    if single is not None:
        for g, s_, name in zip(got.all(), single.all(), NAMES):
            assert (np.ascontiguousarray(g[0]).view("<u4") == np.ascontiguousarray(s_[0]).view("<u4")).all(), "%s: view 0 against the single-frame form, %s" % (what, name)
    return got


# ---- the scenarios -----------------------------------------------------------------------------------------------------------
def identity_1(call, c, sample_map_planes, what):
    """one call from count == 0 with the mixed map at cap 16 on the rect: the sample-map render's planes (sample_map_planes: its
    (rgb, m2, states) for that map, cap and rect on guard-filled planes, from the same implementation) and the oracle's"""
    m = sm.mixed_map()
    got = Planes()
    paths = call(got, m, CAP, RECT)
    want = Planes()
    asked = model(want, 0, sm.chains(c), m, CAP, RECT)
    assert asked == int(sm.counts(m)[sm.inside(RECT)].sum()) and paths in (None, asked)
    assert_planes(got, want, what + ": against the oracle")
    rgb, m2, states = sm.expected(c, m, rect=RECT)
    sm.assert_planes((got.rgb[0], got.m2[0], got.states[0]), (rgb, m2, states), what + ": against the oracle's sample-map planes")
    sm.assert_planes((got.rgb[0], got.m2[0], got.states[0]), sample_map_planes, what + ": against ort_render_sample_map")
    assert (got.count[0] == np.where(sm.inside(RECT), sm.counts(m), 0)).all()


def identity_2_uniform(call, c, pixel_frame, what):
    """passes of 1, 2, 5 and 8 samples (no map) against one pass of 16 and against the PIXEL render at spp = 16 (pixel_frame:
    ort_render_image's, the rect rendered into a frame of GUARD_RGB)"""
    one = Planes()
    assert call(one, None, 16, RECT) in (None, 16 * int(sm.inside(RECT).sum()))
    split = Planes()
    for k in SPLIT:
        call(split, None, k, RECT)
    assert_planes(split, one, what + ": 1 + 2 + 5 + 8 against 16")
    assert (np.ascontiguousarray(one.rgb[0]).view("<u4") == np.ascontiguousarray(pixel_frame).view("<u4")).all(), what + ": against the PIXEL render"
    want = Planes()
    model(want, 0, sm.chains(c), None, 16, RECT)
    assert_planes(one, want, what + ": against the oracle")


def per_pixel_calls():
    return ((sm.mixed_map(0), CAP, RECT), (sm.mixed_map(3), 7, None), (None, 3, SMALL_RECT))


def identity_2_per_pixel(call, c, what, chain=None, nan=False):
    """three calls -- the mixed map on the rect, the shifted mixed map at cap 7 on the whole frame, a constant 3 through a smaller
    rect -- against the chains cut at the cumulative counts.  A pixel no call sampled holds its guards; one that some but not
    all calls sampled holds the earlier call's out_rgb.  chain: the oracle's of c by default; nan: as assert_planes
    -> the planes after the third call"""
    chain = sm.chains(c, cap=CAP + 7 + 3) if chain is None else chain
    got, want = Planes(), Planes()
    took = []
    for k, (m, cap, rect) in enumerate(per_pixel_calls()):
        before = want.count[0].copy()
        paths = call(got, m, cap, rect)
        assert paths in (None, model(want, 0, chain, m, cap, rect))
        took.append(want.count[0] != before)
        assert_planes(got, want, "%s: after call %d" % (what, k), nan=nan)
    never = ~(took[0] | took[1] | took[2])
    earlier = took[0] & ~took[1] & ~took[2]
    assert never.any() and earlier.any() and (took[0] & took[1] & took[2]).any()
    assert (got.count[0][never] == 0).all() and (got.states[0][never] == GUARD_STATE).all() and (got.rgb[0][never] == GUARD_RGB).all()
    first = Planes()
    model(first, 0, chain, *per_pixel_calls()[0])
    if nan:
        same_words(got.rgb[0][earlier], first.rgb[0][earlier], what + ": the earlier call's out_rgb")
    else:
        assert (got.rgb[0][earlier].view("<u4") == first.rgb[0][earlier].view("<u4")).all()
    return got


def reference_split(call, chain, what, split=REF_SPLIT, nan=False):
    """64 samples as 1 + 3 + 12 + 48 (or as `split`) over the whole frame against the fold of the REFERENCE's chains
    (chains_rooms.npz; chains_hostile.npz with nan, as assert_planes takes it) -> the expected planes after the last pass"""
    got, want = Planes(), Planes()
    for k in split:
        call(got, None, k)
        model(want, 0, chain, None, k, None)
        assert_planes(got, want, "%s: after the pass of %d" % (what, k), nan=nan)
    assert (got.count == sum(split)).all()
    return want


HOSTILE = (   # (x, y): count, state, sum, m2 -- pixels of RECT
    ((4, 3), 5, 0, (1e30, -0.0, float("nan")), 2.5),
    ((9, 9), 5, 1, (0.25, 0.5, 0.75), float("inf")),
    ((12, 5), 5, 0xFFFFFFFF, (-0.0, 1e30, -3.0), -0.0),
    ((18, 12), 5, 0x9E3779B9, (1.0, 2.0, 3.0), 0.125),
)


def identity_3(call, c, what):
    """a handful of pixels start with count = 5, states 0 (which must behave as 1), 1, 0xffffffff and an ordinary one, sums with
    1e30, -0 and NaN in them: against oracle calls chained from exactly those states, folded from exactly those sums.  Beside
    them fresh pixels, NaN and 0xdddddddd in their unread words"""
    add = 4
    got = Planes()
    offset = np.zeros((H, W), np.int64)
    chain = dict(sm.chains(c))
    for (x, y), n, state, C, Q in HOSTILE:
        got.count[0, y, x], got.states[0, y, x], got.sum[0, y, x], got.m2[0, y, x] = n, state, np.array(C, "<f4"), F(Q)
        offset[y, x] = n
        chain[(x, y)] = chain_from_state(c, x, y, state if state else 1, add)
    want = got.copy()
    paths = call(got, None, add, RECT)
    asked = model(want, 0, chain, None, add, RECT, offset=offset)
    assert asked == add * int(sm.inside(RECT).sum()) and paths in (None, asked)
    assert_planes(got, want, what)
    zero = HOSTILE[0][0]
    assert got.states[0, zero[1], zero[0]] == chain_from_state(c, zero[0], zero[1], 1, add)[1][-1]
    assert np.isnan(got.sum[0, zero[1], zero[0], 2]) and (got.count[0][offset > 0] == 5 + add).all()


def saturation(call, c, what):
    """count = (1 << 24) - 3 with 16 asked takes 3 samples and leaves 1 << 24; the next call writes no word for that pixel.  A
    count above 1 << 24 takes none"""
    got = Planes()
    at, over = (7, 6), (8, 6)
    state = 0x1234567
    got.count[0, at[1], at[0]], got.states[0, at[1], at[0]], got.sum[0, at[1], at[0]], got.m2[0, at[1], at[0]] = LIMIT - 3, state, (2.0, 4.0, 8.0), F(1.5)
    got.count[0, over[1], over[0]] = 0xEEEEEEEE
    chain = dict(sm.chains(c))
    chain[at] = chain_from_state(c, at[0], at[1], state, 3)
    offset = np.zeros((H, W), np.int64)
    offset[at[1], at[0]] = LIMIT - 3
    want = got.copy()
    paths = call(got, None, 16, RECT)
    asked = model(want, 0, chain, None, 16, RECT, offset=offset)
    assert asked == 16 * (int(sm.inside(RECT).sum()) - 2) + 3 and paths in (None, asked)
    assert_planes(got, want, what + ": the call that saturates")
    assert got.count[0, at[1], at[0]] == LIMIT and got.count[0, over[1], over[0]] == 0xEEEEEEEE and got.states[0, over[1], over[0]] == GUARD_STATE
    only = np.zeros((H, W), "<u4")
    only[at[1], at[0]] = only[over[1], over[0]] = 16
    want = got.copy()
    assert call(got, only, 16, RECT) in (None, 0)
    assert_planes(got, want, what + ": the call after")


def null_map(call, c, what):
    """no map equals the constant map at the cap"""
    a, b = Planes(), Planes()
    call(a, None, 5, RECT)
    call(b, np.full((H, W), 5, "<u4"), 5, RECT)
    assert_planes(a, b, what)
    call(a, None, 3, None)
    call(b, np.full((H, W), 0xFFFFFFFF, "<u4"), 3, None)
    assert_planes(a, b, what + ", continued")


def identity_4(call, c, what):
    """m2 NULL and out_rgb NULL, separately and together, over two calls: no bit of the other planes moves, and the plane that
    was not passed keeps every word"""
    full = Planes()
    call(full, sm.mixed_map(), CAP, RECT)
    call(full, sm.mixed_map(3), 7, None)
    for use_m2, want_rgb in ((False, True), (True, False), (False, False)):
        got = Planes()
        call(got, sm.mixed_map(), CAP, RECT, use_m2=use_m2, want_rgb=want_rgb)
        call(got, sm.mixed_map(3), 7, None, use_m2=use_m2, want_rgb=want_rgb)
        skip = (() if use_m2 else ("m2",)) + (() if want_rgb else ("out_rgb",))
        assert_planes(got, full, "%s: m2 %d out_rgb %d" % (what, use_m2, want_rgb), skip)
        if not use_m2:
            assert (got.m2 == GUARD_M2).all()
        if not want_rgb:
            assert (got.rgb == GUARD_RGB).all()


def identity_5(call, api, c, what):
    """a batch of three views, a map per view, per-view seeds, two calls: frame v is the single-frame call's for that camera and
    seed (the oracle's chains from that camera); view 0 is the single-frame form itself"""
    cams, seeds = sm.batch_cameras(api, c), sm.BATCH_SEEDS
    maps = (np.stack([sm.mixed_map(), sm.mixed_map(3), sm.mixed_map(6)[::-1].copy()]), np.stack([sm.mixed_map(1), sm.mixed_map(), sm.mixed_map(2)]))
    got, want = Planes(3), Planes(3)
    total = 0
    for m, cap, rect in ((maps[0], CAP, RECT), (maps[1], 6, None)):
        paths = call(got, m, cap, rect, cams=cams, seeds=seeds)
        asked = sum(model(want, v, sm.chains(c, seeds[v], cams[v], cap=CAP + 6), m[v], cap, rect) for v in range(3))
        assert paths in (None, asked)
        total += asked
    assert_planes(got, want, what + ": against the oracle, view by view")
    single = Planes()
    call(single, maps[0][0], CAP, RECT, seed=seeds[0])
    call(single, maps[1][0], 6, None, seed=seeds[0])
    for g, s in zip(got.all(), single.all()):
        assert (np.ascontiguousarray(g[0]).view("<u4") == np.ascontiguousarray(s[0]).view("<u4")).all(), what + ": view 0 against the single-frame form"
    assert (got.sum[0].view("<u4") != got.sum[2].view("<u4")).any() and total > 0
