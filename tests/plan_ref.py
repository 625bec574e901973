"""The sample planner's contract (include/ort.h, ort_plan_samples) restated in numpy, written from the header's text and from
nothing else: whole planes at a time, a window being shifted views of the e plane.  Every f32 step is one numpy float32
operation, so it rounds once, as the contract says; the sums and the budget scaling are integers (uint64; the one product that
passes 2^63 in no legal call, want * budget, is at most 2^24 * 2^39).  The tests compare the library's and the host simulator's
maps and totals with this one, word for word."""
import numpy as np

F = np.float32
MAX_COUNT = 1 << 24
DEFAULTS = dict(floor=0.05, radius=1, pilot=4, min_add=1, cap=4096, rgb_is_sum=False, budget=None)


def lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def errors(rgb, m2, count, tolerance, floor, rgb_is_sum):
    """one frame -> (e (H, W) float32 with +0 for unknown and invalid pixels, unknown, invalid, unconverged: bool planes, tol2)"""
    rgb, m2 = np.asarray(rgb, "<f4"), np.asarray(m2, "<f4")
    n = np.asarray(count, "<u4")
    tol2 = F(tolerance) * F(tolerance)
    floor = F(floor)
    with np.errstate(all="ignore"):
        fn = n.astype(F)
        m = lum(rgb) / fn if rgb_is_sum else lum(rgb)
        v = m2 / fn - m * m
        v = np.where(v < 0, F(0), v)
        vm = v / (fn - F(1.0))
        a = np.abs(m)
        b = np.where(a > floor, a, floor)
        e = (vm / (b * b)).astype(F)
    unknown = n < 2
    invalid = ~unknown & ((n > MAX_COUNT) | ~np.isfinite(e))
    valid = ~unknown & ~invalid
    with np.errstate(all="ignore"):
        e = np.where(valid & (e > 0), e, F(0)).astype(F)
    unconverged = valid & (e > tol2)
    return e, unknown, invalid, unconverged, tol2


def window_max(e, radius):
    h, w = e.shape
    d = e.copy()
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if abs(dx) >= w or abs(dy) >= h:
                continue
            ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
            xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
            d[yd, xd] = np.maximum(d[yd, xd], e[ys, xs])
    return d


def wants(rgb, m2, count, tolerance, floor, radius, pilot, min_add, cap, rgb_is_sum):
    """one frame -> (want (H, W) uint32, room (H, W) uint32, e, unknown, invalid, unconverged)"""
    e, unknown, invalid, unconverged, tol2 = errors(rgb, m2, count, tolerance, floor, rgb_is_sum)
    n = np.asarray(count, "<u4").astype(np.uint64)
    room = np.minimum(np.uint64(cap), np.uint64(MAX_COUNT) - np.minimum(n, np.uint64(MAX_COUNT)))
    d = window_max(e, radius)
    with np.errstate(all="ignore"):
        fn = np.asarray(count, "<u4").astype(F)
        need = fn * (d / tol2) - fn
        small = np.where((need > 0) & (need < F(16777216.0)), need, F(0))       # what the cast may be handed
        k = np.where(need >= F(16777216.0), np.uint64(MAX_COUNT), small.astype(np.uint64))
    k = np.maximum(k, np.uint64(min_add))
    want = np.where(unknown, np.minimum(np.uint64(pilot), room), np.where(d > tol2, np.minimum(k, room), np.uint64(0)))
    return want.astype("<u4"), room.astype("<u4"), e, unknown, invalid, unconverged


def plan_frame(rgb, m2, count, tolerance, floor=0.05, radius=1, pilot=4, min_add=1, cap=4096, rgb_is_sum=False, budget=None):
    """one frame -> (map (H, W) uint32, totals dict)"""
    want, _, e, unknown, invalid, unconverged = wants(rgb, m2, count, tolerance, floor, radius, pilot, min_add, cap, rgb_is_sum)
    wanted = int(want.astype(np.uint64).sum(dtype=np.uint64))
    budget = int(budget or 0)
    if budget == 0 or wanted <= budget:
        add = want
    else:
        add = (want.astype(np.uint64) * np.uint64(budget) // np.uint64(wanted)).astype("<u4")
    totals = dict(wanted=wanted, planned=int(add.astype(np.uint64).sum(dtype=np.uint64)), unconverged=int(unconverged.sum()), unknown=int(unknown.sum()),
                  invalid=int(invalid.sum()), worst=F(e.max()))
    return add, totals


def plan(rgb, m2, count, tolerance, **kw):
    """(H, W[, 3]) planes -> (map, totals dict), or (V, H, W[, 3]) -> (maps, list of dicts): every frame on its own"""
    if np.ndim(count) == 2:
        return plan_frame(rgb, m2, count, tolerance, **kw)
    frames = [plan_frame(rgb[v], m2[v], count[v], tolerance, **kw) for v in range(len(count))]
    return np.stack([f[0] for f in frames]), [f[1] for f in frames]
