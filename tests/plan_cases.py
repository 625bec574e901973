"""The sample planner's shared test cases: the seeded synthetic frames of tests/denoise_cases.py (exponential sample noise with
m2 from the actual samples), each with its colour in both forms -- the mean (rgb) and the undivided sum (sum_rgb = rgb * count) --
the frame sizes, the budgets, the big sums, the hostile frame and the parameter corners that tests/test_plan_host.py (CPU) and
tests/test_gpu_plan.py run, and the host simulator's driver (tools/sampleplan_sim).  Each case's reference plan
(tests/plan_ref.py) is computed once per session and shared.

A case is (planes, kw): planes a dict rgb, sum_rgb, m2, count; kw the keyword arguments of plan_ref.plan after the planes
(tolerance, floor, radius, pilot, min_add, cap, rgb_is_sum, budget).  With rgb_is_sum the colour plane is planes["sum_rgb"]."""
import os
import subprocess

import numpy as np
import pytest

import denoise_cases
import plan_ref
from conftest import ROOT

TOOLS = os.path.join(ROOT, "tools")
DEFAULTS = dict(tolerance=0.25, floor=0.05, radius=1, pilot=4, min_add=1, cap=4096, rgb_is_sum=False, budget=None)
TOTALS_DTYPE = np.dtype([("wanted", "<u8"), ("planned", "<u8"), ("unconverged", "<u4"), ("unknown", "<u4"), ("invalid", "<u4"), ("worst", "<f4")])
FIELDS = ("wanted", "planned", "unconverged", "unknown", "invalid")


def _with_sum(p):
    """a denoise_cases frame -> the planner's planes; the sum is one f32 multiply, exact where count is a power of two"""
    with np.errstate(all="ignore"):
        s = (p["rgb"] * p["count"].astype("<f4")[..., None]).astype("<f4")
    return dict(rgb=p["rgb"], sum_rgb=s, m2=p["m2"], count=p["count"])


def frame(w, h, seed, spp=16):
    return _with_sum(denoise_cases.frame(w, h, seed, spp=spp)[0])


def colour(planes, kw):
    return planes["sum_rgb" if kw["rgb_is_sum"] else "rgb"]


def hostile(seed=5):
    """67 x 45 with every hostile pixel of the list, each among ordinary neighbours: ordinary floats, nothing that faults.  Both
    colour forms carry the same hostile words"""
    p = denoise_cases.frame(67, 45, seed)[0]
    rgb, m2, count = p["rgb"], p["m2"], p["count"]
    lum = plan_ref.lum(rgb)
    m2[34:44, 45:60] = (np.float32(16) * lum * lum)[34:44, 45:60]   # a converged region: no variance to speak of ...
    rgb[38, 50] = np.nan                                            # ... with a NaN pixel inside it (its window carries nothing)
    m2[36, 59] = 1e6                                                # ... and a huge finite error on its edge (the windows around carry it)
    rgb[36, 44] = np.inf                                            # ... and an inf pixel just outside
    rgb[0, 0] = np.nan                                              # a hostile pixel in each frame corner
    rgb[0, 66] = (1e30, 1e30, 1e30)                                 # finite, its square is not
    rgb[44, 0, 1] = -np.inf
    count[44, 66] = 0xFFFFFFFF
    rgb[3, 9, 1] = np.inf
    m2[10, 10] = 1e38
    m2[13, 40] = 3e38                                               # with two samples: the error overflows
    count[13, 40] = 2
    m2[10, 30] = 0
    m2[11, 31] = -3.0
    m2[11, 33] = np.nan
    m2[12, 35] = np.float32(-0.0)
    rgb[12, 35] = 0
    count[20:30, 30:40] = 0                                         # a block no pass has touched
    count[5, 20] = 0
    count[5, 22] = 1
    count[5, 24] = 2
    count[6, 21] = (1 << 24) - 1
    count[6, 23] = 1 << 24
    count[6, 25] = (1 << 24) + 1
    count[40, 2] = 0xFFFFFFFF
    rgb[40, 2] = 0.5
    return _with_sum(p)


def batch(seed=21):
    """three different 23 x 19 frames with different spp, view-major: three different totals"""
    frames = [denoise_cases.frame(23, 19, seed + i, spp=8 + 4 * i)[0] for i in range(3)]
    frames[1]["count"][4:7, 3:9] = 0
    frames[2]["rgb"][18, 22] = np.nan       # the last pixel of the last frame, and the first of the one before it
    frames[1]["rgb"][0, 0] = np.nan
    return _with_sum({k: np.stack([f[k] for f in frames]) for k in ("rgb", "m2", "count")})


def _cases():
    c = {}
    for name, (w, h) in (("1x1", (1, 1)), ("7x1", (7, 1)), ("1x9", (1, 9)), ("5x3", (5, 3)), ("64x4", (64, 4)), ("67x45", (67, 45)), ("130x9", (130, 9))):
        c[name] = (frame(w, h, 100 + w), dict(DEFAULTS))
    main = c["67x45"][0]
    c["67x45_sum"] = (main, dict(DEFAULTS, rgb_is_sum=True))
    c["67x45_tol0.1"] = (main, dict(DEFAULTS, tolerance=0.1))
    c["67x45_tol0.5"] = (main, dict(DEFAULTS, tolerance=0.5))
    c["batch3_23x19"] = (batch(), dict(DEFAULTS))
    c["batch3_23x19_sum_budget"] = (batch(), dict(DEFAULTS, rgb_is_sum=True, budget=2000))   # scales two of the three frames
    for r in (0, 2, 3):
        c["radius%d" % r] = (main, dict(DEFAULTS, radius=r))
    # budgets, from the reference's own wanted of the default case
    want = plan_ref.wants(main["rgb"], main["m2"], main["count"], **{k: v for k, v in DEFAULTS.items() if k != "budget"})[0]
    wanted, wanting = int(want.astype(np.uint64).sum()), int((want > 0).sum())
    for name, b in (("third", wanted // 3), ("exact", wanted), ("plus1", wanted + 1), ("one", 1), ("below_wanting", wanting - 1), ("max", 1 << 39)):
        c["budget_" + name] = (main, dict(DEFAULTS, budget=b))
    small = frame(33, 17, 9)
    small["count"][3:6, 4:9] = 0            # some unknown pixels, for the pilot corners
    small = _with_sum(small)
    for name, kw in (("cap1", dict(cap=1)), ("cap_max", dict(cap=1 << 24)), ("min_add_over_cap", dict(min_add=5000)), ("pilot0", dict(pilot=0)),
                     ("pilot_over_cap", dict(pilot=100000)), ("tol1e-18", dict(tolerance=1e-18)), ("tol1e3", dict(tolerance=1e3)),
                     ("floor1e-30", dict(floor=1e-30)), ("floor1e30", dict(floor=1e30))):
        c["corner_" + name] = (small, dict(DEFAULTS, **kw))
    # the big sums: every pixel unknown and asking for 2^24
    big = dict(DEFAULTS, pilot=1 << 24, cap=1 << 24)
    for name, (w, h), b in (("bigsum_64x4", (64, 4), None), ("bigsum_67x45_max", (67, 45), 1 << 39), ("bigsum_67x45_scaled", (67, 45), 1 << 33)):
        p = frame(w, h, 7)
        p["count"][...] = 0
        c[name] = (p, dict(big, budget=b))
    c["hostile"] = (hostile(), dict(DEFAULTS))
    c["hostile_sum_r3"] = (hostile(6), dict(DEFAULTS, rgb_is_sum=True, radius=3, budget=20000))
    return c


CASES = _cases()
NAMES = list(CASES)
BUDGETED = [n for n in NAMES if CASES[n][1]["budget"]]
SMALL_HOSTILE_AND_BIG = [n for n in NAMES if n.startswith(("hostile", "1x", "7x", "5x", "64x4", "batch", "bigsum"))]
VS_HOST_BUILD = [n for n in NAMES if n.startswith(("hostile", "batch", "bigsum", "130x9", "67x45"))]
_ref = {}


def reference(name):
    """the contract's plan of a case, (map, totals), computed once; read-only"""
    if name not in _ref:
        planes, kw = CASES[name]
        smap, totals = plan_ref.plan(colour(planes, kw), planes["m2"], planes["count"], **kw)
        smap.setflags(write=False)
        _ref[name] = (smap, totals)
    return _ref[name]


def assert_same_plan(got_map, got_totals, want_map, want_totals, what):
    """the map's words and every field of the totals equal, worst by its bits"""
    got_map, want_map = np.ascontiguousarray(got_map, "<u4"), np.ascontiguousarray(want_map, "<u4")
    assert got_map.shape == want_map.shape, "%s: shape %s vs %s" % (what, got_map.shape, want_map.shape)
    ne = got_map != want_map
    if ne.any():
        i = tuple(np.argwhere(ne)[0])
        raise AssertionError("%s: %d of %d map words differ; first at %s: %d vs %d" % (what, int(ne.sum()), ne.size, i, got_map[i], want_map[i]))
    g, w = (t if isinstance(t, list) else [t] for t in (got_totals, want_totals))
    assert len(g) == len(w), "%s: %d totals vs %d" % (what, len(g), len(w))
    for f, (a, b) in enumerate(zip(g, w)):
        for k in FIELDS:
            assert int(a[k]) == int(b[k]), "%s: frame %d %s %d vs %d" % (what, f, k, a[k], b[k])
        ab, bb = (int(np.array(t["worst"], "<f4").view("<u4")) for t in (a, b))
        assert ab == bb, "%s: frame %d worst %r (0x%08x) vs %r (0x%08x)" % (what, f, a["worst"], ab, b["worst"], bb)


def built(target):
    """tools/<target> (sampleplan_sim or sampleplan_sim_san), made when it is missing or older than its sources"""
    tool = os.path.join(TOOLS, target)
    src = [os.path.join(TOOLS, "sampleplan_sim.cpp"), os.path.join(TOOLS, "Makefile"), os.path.join(ROOT, "offline_raytracer_amd", "csrc", "ort_sampleplan.h")]
    if not os.path.exists(tool) or any(os.path.getmtime(s) > os.path.getmtime(tool) for s in src):
        if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
            pytest.skip("tools/%s is not built and there is no hipcc to build it with" % target)
        r = subprocess.run(["make", "-s", "-B", "-C", TOOLS, target], capture_output=True, text=True)
        assert r.returncode == 0, "make %s failed (exit %d)\n%s" % (target, r.returncode, (r.stdout + r.stderr)[-4000:])
    return tool


def run_sim(tool, planes, kw, tmp, env=None):
    """the planes through tools/<tool> -> (CompletedProcess, map or None, totals (dict, or list of dicts for a batch) or None)"""
    count = planes["count"]
    frames = 1 if count.ndim == 2 else len(count)
    h, w = count.shape[-2:]
    paths = []
    for k, a, dt in (("rgb", colour(planes, kw), "<f4"), ("m2", planes["m2"], "<f4"), ("count", count, "<u4")):
        path = os.path.join(str(tmp), k + ".bin")
        np.ascontiguousarray(a, dt).tofile(path)
        paths.append(path)
    outs = [os.path.join(str(tmp), "map.bin"), os.path.join(str(tmp), "totals.bin")]
    for o in outs:
        if os.path.exists(o):
            os.remove(o)
    args = [tool, w, h, frames, repr(float(np.float32(kw["tolerance"]))), repr(float(np.float32(kw["floor"]))), kw["radius"], kw["pilot"], kw["min_add"], kw["cap"],
            int(bool(kw["rgb_is_sum"])), int(kw["budget"] or 0)] + paths + outs
    r = subprocess.run([str(a) for a in args], env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=300)
    if r.returncode != 0 or not all(os.path.exists(o) for o in outs):
        return r, None, None
    smap = np.fromfile(outs[0], "<u4").reshape(count.shape)
    rec = np.fromfile(outs[1], TOTALS_DTYPE)
    totals = [dict({k: int(t[k]) for k in FIELDS}, worst=np.float32(t["worst"])) for t in rec]
    return r, smap, totals[0] if count.ndim == 2 else totals
