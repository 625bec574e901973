"""The denoiser's shared test cases: seeded synthetic frames -- two or three surfaces with different normals, depth ramps, a
textured albedo, exponential sample noise with m2 from the actual samples -- the frame sizes, the hostile set and the parameter
corners that tests/test_denoise_host.py (CPU) and tests/test_gpu_denoise.py run, and the host simulator's driver
(tools/denoise_sim).  Each case's reference frame (tests/denoise_ref.py) is computed once per session and shared."""
import os
import subprocess

import numpy as np
import pytest

import denoise_ref
from conftest import ROOT

TOOLS = os.path.join(ROOT, "tools")
PLANES = ("rgb", "m2", "count", "albedo", "normal", "depth")
DEFAULTS = dict(iterations=5, normal_squarings=5, sigma_l=4.0, sigma_z=0.05)


def _lum(c):
    return (np.float32(0.2126) * c[..., 0] + np.float32(0.7152) * c[..., 1]) + np.float32(0.0722) * c[..., 2]


def frame(w, h, seed, spp=16, surfaces=3):
    """-> (planes dict, truth (h, w, 3)): surface k covers the pixels on its side of two slanted lines; each has its own unit
    normal, a depth ramp and a brightness; the albedo is a checker with a gradient across it; every pixel has spp samples
    truth * e, e exponential with mean 1, whose mean is rgb and whose squared luminances add up to m2"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype("<f4")
    u, v = x / np.float32(max(w - 1, 1)), y / np.float32(max(h - 1, 1))
    which = np.zeros((h, w), int)
    which[u + np.float32(0.3) * v > np.float32(0.55)] = 1
    if surfaces > 2:
        which[(v - np.float32(0.4) * u > np.float32(0.6))] = 2
    normals = np.array([[0, 0, 1], [0.6, 0, 0.8], [0, -0.8, 0.6]], "<f4")
    light = np.array([1.0, 0.45, 0.7], "<f4")
    normal = normals[which]
    depth = (np.array([4.0, 5.5, 3.0], "<f4")[which] + np.array([0.8, -1.1, 0.5], "<f4")[which] * u + np.array([0.3, 0.6, -0.9], "<f4")[which] * v).astype("<f4")
    check = ((x.astype(int) // 5 + y.astype(int) // 4) % 2).astype("<f4")
    albedo = np.stack([np.float32(0.2) + np.float32(0.6) * check, np.float32(0.3) + np.float32(0.5) * u, np.float32(0.75) - np.float32(0.5) * check * v], -1).astype("<f4")
    truth = (albedo * light[which][..., None]).astype("<f4")
    e = rng.exponential(1.0, (spp, h, w)).astype("<f4")
    samples = truth[None] * e[..., None]
    rgb = (samples.sum(0, dtype="<f4") / np.float32(spp)).astype("<f4")
    m2 = (_lum(samples) ** 2).sum(0, dtype="<f4").astype("<f4")
    planes = dict(rgb=rgb, m2=m2, count=np.full((h, w), spp, "<u4"), albedo=albedo, normal=normal.astype("<f4"), depth=depth)
    return planes, truth


def hostile(seed=5):
    """67 x 45 with every hostile pixel of the issue's list, each among ordinary neighbours: ordinary floats, nothing that faults"""
    p, _ = frame(67, 45, seed)
    rgb, m2, count, albedo, normal, depth = (p[k] for k in PLANES)
    rgb[3, 4] = np.nan                      # NaN and inf colours
    rgb[3, 9, 1] = np.inf
    rgb[8, 60] = (-np.inf, 1, 1)
    count[20:30, 30:40] = 0                 # a block no sample map touched ...
    rgb[20:30, 30:40] = 7.5                 # ... whose colour must come back as it stands
    count[5, 20] = 1                        # one sample: the variance is Y*Y
    count[6, 21] = 1 << 24
    count[40, 2] = 0xFFFFFFFF
    albedo[12, 12] = 0                      # zero and negative albedo: floored
    albedo[12, 14] = (-0.5, 0.4, 0.0)
    albedo[13, 50] = np.nan
    normal[30:34, 5:12] = 0                 # misses: zero normals
    depth[30:34, 5:12] = 0
    normal[15, 40:44] *= np.float32(2)      # normals of length 2
    normal[2, 30] = np.inf
    depth[36, 20:24] = 0                    # depth 0 next to ordinary depths, and negative depth
    depth[38, 20:24] *= np.float32(-1)
    depth[41, 41] = np.nan
    m2[10, 10] = 1e38                       # the variance overflows: unusable
    m2[10, 30] = 0                          # v clamps at 0
    m2[11, 31] = -3.0
    m2[11, 33] = np.nan
    m2[44, 66] = np.float32(-0.0)
    rgb[44, 66] = 0
    rgb[0, 0] = 1e30                        # finite, its squares are not
    return p


def batch(seed=21):
    """three different 23 x 19 frames, view-major"""
    frames = [frame(23, 19, seed + i, spp=8 + 4 * i, surfaces=2 + i % 2)[0] for i in range(3)]
    frames[1]["count"][4:7, 3:9] = 0
    frames[2]["rgb"][18, 22] = np.nan       # the last pixel of the last frame, and the first of the one before it
    frames[1]["rgb"][0, 0] = np.nan
    return {k: np.stack([f[k] for f in frames]) for k in PLANES}


def _cases():
    c = {}
    for name, (w, h), kw in (("1x1", (1, 1), {}), ("7x1", (7, 1), {}), ("1x9", (1, 9), {}), ("5x3", (5, 3), {}),
                             ("33x17_it6", (33, 17), dict(iterations=6)), ("67x45", (67, 45), {})):
        c[name] = (frame(w, h, 100 + w)[0], dict(DEFAULTS, **kw))
    c["batch3_23x19"] = (batch(), dict(DEFAULTS))
    c["hostile"] = (hostile(), dict(DEFAULTS))
    c["hostile_it8_sq0"] = (hostile(6), dict(DEFAULTS, iterations=8, normal_squarings=0))
    small = frame(33, 17, 9)[0]
    for name, kw in (("it1", dict(iterations=1)), ("it8", dict(iterations=8)), ("sq0", dict(normal_squarings=0)), ("sq8", dict(normal_squarings=8)),
                     ("sl1e-20", dict(sigma_l=1e-20)), ("sl1e20", dict(sigma_l=1e20)), ("sz_wide", dict(sigma_z=0.1, sigma_l=8.0))):
        c["corner_" + name] = (small, dict(DEFAULTS, **kw))
    return c


CASES = _cases()
NAMES = list(CASES)
SMALL_AND_HOSTILE = [n for n in NAMES if n.startswith(("hostile", "1x", "7x", "5x", "batch"))]
_ref = {}


def reference(name):
    """the contract's frame of a case, computed once; read-only"""
    if name not in _ref:
        planes, kw = CASES[name]
        _ref[name] = denoise_ref.denoise(*[planes[k] for k in PLANES], **kw)
        _ref[name].setflags(write=False)
    return _ref[name]


def assert_same_frame(got, want, what):
    """bit for bit, a NaN by position"""
    got, want = np.ascontiguousarray(got, "<f4"), np.ascontiguousarray(want, "<f4")
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert (gn == wn).all(), "%s: %d NaNs out of place" % (what, int((gn != wn).sum()))
    from conftest import assert_bits_equal
    assert_bits_equal(np.where(gn, np.float32(0), got), np.where(wn, np.float32(0), want), what)


def built(target):
    """tools/<target> (denoise_sim or denoise_sim_san), made when it is missing or older than its sources"""
    tool = os.path.join(TOOLS, target)
    src = [os.path.join(TOOLS, "denoise_sim.cpp"), os.path.join(TOOLS, "Makefile"), os.path.join(ROOT, "offline_raytracer_amd", "csrc", "ort_denoise.h")]
    if not os.path.exists(tool) or any(os.path.getmtime(s) > os.path.getmtime(tool) for s in src):
        if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
            pytest.skip("tools/%s is not built and there is no hipcc to build it with" % target)
        r = subprocess.run(["make", "-s", "-B", "-C", TOOLS, target], capture_output=True, text=True)
        assert r.returncode == 0, "make %s failed (exit %d)\n%s" % (target, r.returncode, (r.stdout + r.stderr)[-4000:])
    return tool


def run_sim(tool, planes, kw, tmp, env=None, in_place=False):
    """the planes through tools/<tool> -> (CompletedProcess, the frame it wrote or None)"""
    count = planes["count"]
    frames = 1 if count.ndim == 2 else len(count)
    h, w = count.shape[-2:]
    paths = []
    for k in PLANES:
        path = os.path.join(str(tmp), k + ".bin")
        np.ascontiguousarray(planes[k], "<u4" if k == "count" else "<f4").tofile(path)
        paths.append(path)
    out = paths[0] if in_place else os.path.join(str(tmp), "out.bin")
    if not in_place and os.path.exists(out):
        os.remove(out)
    args = [tool, w, h, frames, kw["iterations"], kw["normal_squarings"], repr(float(kw["sigma_l"])), repr(float(kw["sigma_z"]))] + paths + [out]
    r = subprocess.run([str(a) for a in args], env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=300)
    got = np.fromfile(out, "<f4").reshape(count.shape + (3,)) if r.returncode == 0 and os.path.exists(out) else None
    return r, got
