"""The newer render kernels with more jobs than resident lanes (tests/test_gpu_many_jobs.py, tests/test_many_jobs_host.py): the
frame, the windows the oracle answers for, the sample maps, the knob sets, and the launch plans that say the frame is large
enough (test infrastructure, next to light_groups_cases.py and sample_map_cases.py, whose scenes and oracle these are).

1024 x 768 is 12 288 blocks of 8 x 8 and 786 432 one-pixel jobs: three per resident lane of a 256-unit device (units x 4
workgroups x 256 lanes).  A lane of pt_adaptive, pt_groups, pt_sample_map, the VIEWS loop and feature_pixels then runs a second
and a third job, lanes of one wave hold different jobs (and views), and ORT_JOB_BATCH has a tail to hold back -- none of which
happens at the 24 x 16 of the families' own tests.  tools/launch_plan says so without a device (plans() below): no test here
takes it for granted.

Two references.  (a) Three 24 x 16 windows of the frame against the oracle, used as the small tests use it: the oracle's PIXEL
render of the scene and of its dark twins with rect = the window, render_adaptive_cases.chains over the window, feature_cases'
frame of the window.  (b) The whole frame by identity against other kernels (the tests' own business)."""
import numpy as np

import adaptive_cases as ac
import light_groups_cases as lg
import sample_map_cases as sm
import test_launch_plan as tlp
from adaptive_cases import Adaptive

W, H = 1024, 768
SIZE = (W, H)
SPP, CAP = 4, 8                        # fixed-length renders; the cap of the adaptive and sample-map renders
SEED, RR = lg.SEED, lg.RR
VIEW_SEEDS = (lg.SEED, 7)              # V = 2: the scene's own camera and batch_cameras' second
AD = Adaptive(2, 8, 2, 0.3, 0.05)      # checks after 2, 4 and 6 samples: a pixel stops at 2, 4, 6 or 8
FEATURE_SPP = (1, 2)
ROOMS = lg.ROOMS
MESH = "c4_dwarf_room"                 # where a triangle tree matters
# at the origin; aligned to 8 in neither x nor y; touching the last column and the last row
WINDOWS = ((0, 0, 24, 16), (501, 371, 525, 387), (1000, 752, 1024, 768))
# the adaptive render's windows, per scene: WINDOWS wherever the oracle's chains meet assert_adaptive_windows' condition there
# (they do in all three scenes: 77 to 89 % of a window's pixels stop at 2, 9 to 23 % run to 8); a window that does not is moved
ADAPTIVE_WINDOWS = {name: WINDOWS for name in lg.ROOMS + ("c4_dwarf_room",)}
POINTS, IRR_SPP, AO_SPP = 1024, 2, 4

KNOBS = ("ORT_JOB_BATCH", "ORT_BATCH_TAIL", "ORT_CACHE_RESIDENT", "ORT_REFILL_BELOW", "ORT_DESCEND_BELOW", "ORT_LDS_TABLES", "ORT_KERNEL")
KNOB_SETS = {
    "no batches": {"ORT_JOB_BATCH": "0"},
    "batches of 7 to the end": {"ORT_JOB_BATCH": "7", "ORT_BATCH_TAIL": "0"},
    "batches of 128, tail 1": {"ORT_JOB_BATCH": "128", "ORT_BATCH_TAIL": "1"},
    "large-tree policy": {"ORT_CACHE_RESIDENT": "0"},
    "refill 1 descend 0": {"ORT_REFILL_BELOW": "1", "ORT_DESCEND_BELOW": "0"},
    "refill 1 descend 64": {"ORT_REFILL_BELOW": "1", "ORT_DESCEND_BELOW": "64"},
    "refill 64 descend 0": {"ORT_REFILL_BELOW": "64", "ORT_DESCEND_BELOW": "0"},
    "refill 64 descend 64": {"ORT_REFILL_BELOW": "64", "ORT_DESCEND_BELOW": "64"},
    "tables in HBM": {"ORT_LDS_TABLES": "0"},
    "general kernel": {"ORT_KERNEL": "general"},
}
BATCHING = ("batches of 7 to the end", "batches of 128, tail 1")   # the sets that claim to batch


# ---- the launches, as tools/launch_plan plans them ---------------------------------------------------------------------------
def lanes(cu_count):
    return cu_count * 4 * 256


def point_count(cu_count):
    """1 024 base points tiled to three per resident lane and 257 more: the last tile is partial, the last wave too"""
    return 3 * lanes(cu_count) + 257


def launches(cu_count):
    """{family: launch_plan's arguments} of every launch the GPU tests make at the large size"""
    frame = dict(width=W, height=H)
    out = {
        "views pixel": dict(frame, policy="pixel", spp=SPP, views=2),
        "views chunk": dict(frame, policy="chunk", spp=SPP, chunk=2, views=2),
        "adaptive": dict(frame, policy="pixel", adaptive=1, min_spp=AD.min_spp, max_spp=AD.max_spp, check_every=AD.check_every),
        "light groups": dict(frame, policy="pixel", groups=1, spp=SPP),
        "light groups, two views": dict(frame, policy="pixel", groups=1, spp=SPP, views=2),
        "sample map": dict(frame, policy="pixel", sample_map=1, spp=CAP),
        "sample map, two views": dict(frame, policy="pixel", sample_map=1, spp=CAP, views=2),
        "irradiance points": dict(query="radiance", count=point_count(cu_count)),
        "ao points": dict(query="raycast", count=point_count(cu_count)),
    }
    for spp in FEATURE_SPP:
        out["features spp %d" % spp] = dict(frame, query="features", x1=W, y1=H, spp=spp)
    return out


READS_NO_KNOB = ("ao points",)   # plan_ray_query: its batches are constants, and at three jobs a lane it deals one by one


def plans(tool, cu_count):
    """-> {(family, knob set or "default"): (jobs, grid, job_batch, batch_until)} of every launch under every knob set, each
    held to what makes the tests mean something: at least two jobs per resident lane of the launch's own grid, and under
    the sets that claim to batch a tail that is really held back, in batches of more than one.  Fails, never skips"""
    seen = {}
    for family, args in launches(cu_count).items():
        for label, env in [("default", {})] + list(KNOB_SETS.items()):
            p = tlp.plan(tool, env, cu_count=cu_count, **args)
            jobs = p["job_count"] if "job_count" in p else p["count"]
            what = "%s under %s on %d units" % (family, label, cu_count)
            assert p["grid"] == 4 * cu_count, "%s: grid %d" % (what, p["grid"])
            assert jobs >= 2 * p["grid"] * 256, "%s: %d jobs for %d lanes: no lane is sure of a second job" % (what, jobs, p["grid"] * 256)
            if label in BATCHING and family not in READS_NO_KNOB:
                assert p["batch_until"] > 0 and p["job_batch"] > 1, "%s: job_batch %d until %d: nothing is batched" % (what, p["job_batch"], p["batch_until"])
                assert p["job_batch"] == int(env["ORT_JOB_BATCH"])
            if label == "no batches" and family not in READS_NO_KNOB:
                assert p["job_batch"] == 0
            seen[(family, label)] = (jobs, p["grid"], p["job_batch"], p["batch_until"])
    return seen


def plans_report(seen):
    """what the plan assertions saw, one line a family: jobs per lane at the default, batch_until under the batching sets"""
    lines = []
    for (family, label), (jobs, grid, _, _) in seen.items():
        if label == "default":
            lines.append("%s: %d jobs, %.2f per lane; batch_until %s" % (family, jobs, jobs / (grid * 256.0), ", ".join(
                "%d (%s)" % (seen[(family, b)][3], b) for b in BATCHING)))
    return "\n".join(lines)


# ---- the sample maps -----------------------------------------------------------------------------------------------------------
MAP_VALUES = (0, 1, 2, 4, 8, 0xFFFFFFFF)
ZERO_BLOCKS = ((8, 0), (504, 376), (1008, 752), (512, 384), (0, 760))   # whole 8 x 8 blocks of zeros: one in every window
ZERO_ROWS = (10, 380, 761)                                             # whole rows of zeros: one through every window


def full_map(shift=0):
    """every value of MAP_VALUES over the whole frame, laid out as sample_map_cases.base_map lays its own out -- the index
    steps by 1 along x and by 3 along y, modulo 6, so that neighbours differ -- with whole zero blocks and zero rows"""
    m = sm.base_map(shift, SIZE, MAP_VALUES)
    for bx, by in ZERO_BLOCKS:
        m[by:by + 8, bx:bx + 8] = 0
    for y in ZERO_ROWS:
        m[y, :] = 0
    return m


def sparse_map(seed=20240607):
    """about one pixel in sixteen non-zero, value and place from a fixed-seed generator: most jobs a lane draws are empty.
    Inside the oracle's windows one pixel in five, so that the oracle has more than a handful of pixels to answer for"""
    rng = np.random.default_rng(seed)
    density = np.full((H, W), 1.0 / 16.0)
    for x0, y0, x1, y1 in WINDOWS:
        density[y0:y1, x0:x1] = 0.2
    m = np.zeros((H, W), "<u4")
    on = rng.random((H, W)) < density
    m[on] = np.array(MAP_VALUES[1:], "<u4")[rng.integers(0, len(MAP_VALUES) - 1, int(on.sum()))]
    return m


def crop(a, window):
    x0, y0, x1, y1 = window
    return a[..., y0:y1, x0:x1, :] if a.ndim >= 3 and a.shape[-1] in (2, 3) and a.shape[-2] == W else a[..., y0:y1, x0:x1]


def assert_full_map(m, cap=CAP):
    """from the map alone: every value class on at least 2 % of the frame; each oracle window with at least 50 pixels of
    n >= 1 and at least 50 of n == 0"""
    assert m.shape == (H, W) and m.dtype == np.dtype("<u4")
    for v in MAP_VALUES:
        assert (m == v).mean() >= 0.02, "value %#x covers %.4f of the frame" % (v, (m == v).mean())
    assert set(np.unique(m).tolist()) == set(MAP_VALUES)
    assert_map_windows(m, cap)
    assert (m[:, 1:] != m[:, :-1]).mean() > 0.9 and (m[1:] != m[:-1]).mean() > 0.9   # neighbours differ


def assert_map_windows(m, cap=CAP, windows=WINDOWS):
    n = sm.counts(m, cap)
    for win in windows:
        k = crop(n, win)
        assert (k >= 1).sum() >= 50 and (k == 0).sum() >= 50, "window %r: %d pixels with samples, %d without" % (win, (k >= 1).sum(), (k == 0).sum())


def assert_sparse_map(m, cap=CAP):
    """at least 90 % of the pixels empty (and no fewer than one in twenty-four taken); the windows as for the full map"""
    assert m.shape == (H, W) and m.dtype == np.dtype("<u4")
    assert 0.90 <= (m == 0).mean() <= 1.0 - 1.0 / 24.0, (m == 0).mean()
    assert set(np.unique(m).tolist()) == set(MAP_VALUES)
    assert_map_windows(m, cap)


# ---- cameras -------------------------------------------------------------------------------------------------------------------
def view_cameras(api, c):
    """(2, 4, 3): the scene's own camera at 1024 x 768, and light_groups_cases.batch_cameras' second"""
    return np.ascontiguousarray(lg.batch_cameras(api, c, SIZE)[:2])


# ---- (a) the oracle on a window ------------------------------------------------------------------------------------------------
_cache = {}


def _cam(c, cam):
    return c.camera(SIZE) if cam is None else np.asarray(cam, "<f4").reshape(4, 3)


def window_frame(c, keep, spp, window, seed=SEED, cam=None):
    """(16, 24, 3): the window of the oracle's PIXEL render of case c's twin(keep) -- keep = None: the scene itself -- at
    1024 x 768 with rect = window"""
    cam = _cam(c, cam)
    key = ("frame", c.name, None if keep is None else frozenset(keep), spp, window, seed, cam.tobytes())
    if key not in _cache:
        osc = c.twin(keep)
        osc.set_camera(cam)
        img, _ = osc.render(W, H, spp, seed, "pixel", rect=window, rr=RR, threads=8)
        _cache[key] = np.ascontiguousarray(crop(img, window))
        _cache[key].setflags(write=False)
    return _cache[key]


def window_chunk_frame(c, spp, chunk, window, seed=SEED, cam=None):
    """the same of the CHUNK render of the scene itself"""
    cam = _cam(c, cam)
    key = ("chunk", c.name, spp, chunk, window, seed, cam.tobytes())
    if key not in _cache:
        osc = c.twin(None)
        osc.set_camera(cam)
        img, _ = osc.render(W, H, spp, seed, "chunk", chunk=chunk, rect=window, rr=RR, threads=8)
        _cache[key] = np.ascontiguousarray(crop(img, window))
    return _cache[key]


def window_chains(c, window, seed=SEED, cam=None):
    """render_adaptive_cases.chains(osc, 1024, 768, seed, rr, window, CAP) of the scene itself, once"""
    return sm.chains(c, seed, _cam(c, cam), SIZE, window, CAP)


def window_planes(c, window, rule, seed=SEED, cam=None):
    """-> (rgb (16, 24, 3), n (16, 24), m2 (16, 24), states (16, 24)): the chains of the window cut by rule -- an Adaptive, or
    a map of counts (h, w) over the whole frame, pixel i cut by the rule that never checks at n_i; a pixel with n_i = 0 holds
    sample_map_cases' guards"""
    x0, y0, x1, y1 = window
    rgb = np.full((y1 - y0, x1 - x0, 3), sm.GUARD_RGB, "<f4")
    n = np.zeros((y1 - y0, x1 - x0), "<u4")
    m2 = np.full((y1 - y0, x1 - x0), sm.GUARD_M2, "<f4")
    fin = np.full((y1 - y0, x1 - x0), sm.GUARD_STATE, "<u4")
    for (x, y), (cols, states) in window_chains(c, window, seed, cam).items():
        ad = rule
        if not isinstance(rule, Adaptive):
            k = int(rule[y, x])
            if k == 0:
                continue
            ad = Adaptive(k, k, 1, 0, 0)
        rgb[y - y0, x - x0], n[y - y0, x - x0], m2[y - y0, x - x0], fin[y - y0, x - x0] = ac.cut(cols, states, ad)
    return rgb, n, m2, fin


def adaptive_window_shares(c, window):
    """{count: share of the window's pixels that AD stops there}, from the oracle's chains"""
    n = window_planes(c, window, AD)[1]
    return {int(k): float((n == k).mean()) for k in np.unique(n)}


def assert_adaptive_windows(c):
    """in every window of the scene at least two distinct counts occur, each on at least 5 % of its pixels: the rule cuts some
    pixels and not others where the oracle is looked at"""
    for window in ADAPTIVE_WINDOWS[c.name]:
        shares = adaptive_window_shares(c, window)
        assert set(shares) <= {2, 4, 6, 8}
        assert sum(s >= 0.05 for s in shares.values()) >= 2, "%s window %r: %r" % (c.name, window, shares)


# ---- comparing -------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).view("<u4")


def first_difference(got, want, where=None, origin=(0, 0)):
    """None, or "n of m words differ; first at pixel (x, y) ..." over the words where `where` (a mask over the leading axes,
    by default all of them) holds; got, want: (..., rows, columns[, k]) planes of the frame or of a window at origin"""
    g, w_ = bits(got), bits(want)
    assert g.shape == w_.shape, "shape %s vs %s" % (g.shape, w_.shape)
    ne = g != w_
    if where is not None:
        ne &= where.reshape(where.shape + (1,) * (ne.ndim - where.ndim))
    if not ne.any():
        return None
    at = tuple(int(i) for i in np.argwhere(ne)[0])
    rows = [k for k in range(g.ndim - 1) if g.shape[k:k + 2] in ((H, W), (16, 24))]
    pixel = "pixel (x %d, y %d), " % (origin[0] + at[rows[0] + 1], origin[1] + at[rows[0]]) if rows else ""
    return "%d of %d words differ; first at %sindex %r: %r vs %r" % (int(ne.sum()), ne.size, pixel, at, np.ascontiguousarray(got)[at], np.ascontiguousarray(want)[at])


def assert_same(got, want, what, where=None):
    d = first_difference(got, want, where)
    assert d is None, "%s: %s" % (what, d)


def assert_window(got, want, window, what):
    """the window of the full-frame plane got (..., h, w[, k]) equals the oracle's crop want; a difference is reported in the
    frame's own coordinates"""
    d = first_difference(crop(np.ascontiguousarray(got), window), want, origin=window[:2])
    assert d is None, "%s, window %r: %s" % (what, window, d)


# ---- the first camera ray of every pixel of the frame ----------------------------------------------------------------------------
# feature_cases.camera_rays asks the oracle twice per pixel (oracle_job_seed, oracle_rng_table): seven seconds for this frame.
# The two steps in numpy -- integer arithmetic and one float32 product -- are what it is given here instead;
# tests/test_many_jobs_host.py holds them against the oracle's own on the windows and on 4 096 pixels picked across the frame.
def numpy_streams(oracle, seed, pix):
    """oracle_job_seed(seed, pix) for an array of pixels: fmix32(seed ^ pix * 2654435761), 0 taken as 1"""
    h = np.uint32(seed & 0xFFFFFFFF) ^ (np.asarray(pix).astype(np.uint32) * np.uint32(2654435761))
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return np.where(h == 0, np.uint32(1), h).astype("<u4")


def numpy_draw(oracle, state):
    """random_between(0, 2 pi): two steps of the stream, the second one's word as a float32 over 2^32, times float32(2 pi)"""
    x = np.array(state, dtype=np.uint32)
    for _ in range(2):
        x ^= x << np.uint32(13)
        x ^= x >> np.uint32(17)
        x ^= x >> np.uint32(5)
    v = x.astype("<f4") / np.float32(4294967296.0)
    return x.astype("<u4"), (np.float32(0.0) + (np.float32(2.0) * np.float32(np.pi) - np.float32(0.0)) * v).astype("<f4")


def first_rays(oracle, cam, seed, rect=None, fast=True):
    """-> (rays (n, 6), states after the sample (n,)) of sample 0 of the pixels of rect (the whole frame by default), row-major"""
    import feature_cases as fc
    kw = dict(streams=numpy_streams, draw=numpy_draw) if fast else {}
    ap, d, after, _, _ = fc.camera_rays(oracle, cam, W, H, seed, 1, rect, **kw)
    return np.ascontiguousarray(np.concatenate([ap[:, 0], d[:, 0]], axis=1), "<f4"), after[:, 0]
