"""tools/host_sim from the tests: building the plain and the sanitized binary, and running one of its modes on arrays
(test infrastructure for test_query_lanes_host.py and test_host_sanitizers.py; raw little-endian files in a scratch
directory, as the tool reads and writes them)."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import DATA, ROOT

TOOLS = os.path.join(ROOT, "tools")
CSRC = os.path.join(ROOT, "offline_raytracer_amd", "csrc")
HIT_DTYPE = np.dtype([("t", "<f4"), ("n", "<f4", 3), ("mat", "<u4"), ("prim", "<u4")])
NO_PRIM = 0xFFFFFFFF
_KNOBS = ("SIM_", "ORT_", "ASAN_OPTIONS", "UBSAN_OPTIONS", "LSAN_OPTIONS")


def built(target):
    """the path of tools/<target> (host_sim, host_sim_w5 or host_sim_san), made when it is missing or older than its sources"""
    tool = os.path.join(TOOLS, target)
    src = [os.path.join(TOOLS, f) for f in ("host_sim.cpp", "host_sim_stubs.cpp", "Makefile")]
    src += [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".cpp"))]
    if not os.path.exists(tool) or any(os.path.getmtime(s) > os.path.getmtime(tool) for s in src):
        if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
            pytest.skip("tools/%s is not built and there is no hipcc to build it with" % target)
        r = subprocess.run(["make", "-s", "-B", "-C", TOOLS, target], capture_output=True, text=True)
        assert r.returncode == 0, "make %s failed (exit %d)\n%s" % (target, r.returncode, (r.stdout + r.stderr)[-4000:])
    return tool


def scene_args(scene, base=None):
    """the name of a scene under data/, or with base (its directory) the path of a .scn -> [scn, base]"""
    return [scene, base] if base else [os.path.join(DATA, scene + ".scn"), DATA + "/"]


def run(tool, args, env=None, threads=1, check=True):
    """-> CompletedProcess; env: the SIM_* / ORT_* knobs of this run (none is inherited)"""
    e = {k: v for k, v in os.environ.items() if not k.startswith(_KNOBS)}
    e["SIM_THREADS"] = str(threads)
    e.update(env or {})
    r = subprocess.run([tool] + [str(a) for a in args], env=e, capture_output=True, text=True, timeout=600)
    if check:
        assert r.returncode == 0, "%s %s: exit %d\n%s" % (os.path.basename(tool), " ".join(map(str, args[:1])), r.returncode, r.stderr[-1500:])
    return r


def counters(r):
    """the work counters of a run's last stderr line -> {"rays": ..., "fallback": ...}"""
    line = [l for l in r.stderr.splitlines() if l.startswith("sim:")][-1]
    return {k: int(v) for k, v in re.findall(r"(\w+) (\d+)(?= |$)", line)}


def stack_probe(r):
    """the stack probe's lines of a run's stderr, one per instantiation of traverse -> [{"lds": its LDS entries, "deepest": the
    deepest stack, "traversals", "above": traversals that went past the LDS entries, "steps_above", "scratch_pops"}], the
    instantiation with the most LDS entries (the main traversal) first; the re-traversal of resolve_hit has four fewer"""
    return [{k: int(v) for k, v in re.findall(r"(\w+) (\d+)", l[len("stack:"):])} for l in r.stderr.splitlines() if l.startswith("stack:")]


def raycast_args(d, scene, rays, base=None):
    np.ascontiguousarray(rays, "<f4").tofile(os.path.join(d, "rays.f32"))
    return ["--raycast"] + scene_args(scene, base) + [os.path.join(d, "rays.f32"), os.path.join(d, "hits.bin")], [os.path.join(d, "hits.bin")]


def raycast(tool, d, scene, rays, base=None, **kw):
    """-> (hits as HIT_DTYPE records, CompletedProcess)"""
    args, outs = raycast_args(str(d), scene, rays, base)
    r = run(tool, args, **kw)
    hits = np.fromfile(outs[0], HIT_DTYPE)
    assert len(hits) == len(rays)
    return hits, r


def occluded_args(d, scene, rays, tmax, base=None):
    np.ascontiguousarray(rays, "<f4").tofile(os.path.join(d, "rays.f32"))
    if tmax is not None:
        np.ascontiguousarray(tmax, "<f4").tofile(os.path.join(d, "tmax.f32"))
    return (["--occluded"] + scene_args(scene, base) + [os.path.join(d, "rays.f32"), os.path.join(d, "tmax.f32") if tmax is not None else "-",
                                                        os.path.join(d, "occ.u8")], [os.path.join(d, "occ.u8")])


def occluded(tool, d, scene, rays, tmax, base=None, **kw):
    """-> bytes (uint8), one per ray"""
    args, outs = occluded_args(str(d), scene, rays, tmax, base)
    run(tool, args, **kw)
    out = np.fromfile(outs[0], np.uint8)
    assert len(out) == len(rays)
    return out


def radiance_args(d, scene, rays, seeds, spp, rr, base=None):
    np.ascontiguousarray(rays, "<f4").tofile(os.path.join(d, "rays.f32"))
    np.ascontiguousarray(seeds, "<u4").tofile(os.path.join(d, "seeds.u32"))
    outs = [os.path.join(d, "rad.f32"), os.path.join(d, "states.u32")]
    return ["--radiance"] + scene_args(scene, base) + [os.path.join(d, "rays.f32"), os.path.join(d, "seeds.u32"), spp, repr(float(rr))] + outs, outs


def radiance(tool, d, scene, rays, seeds, spp, rr=0.8, base=None, **kw):
    """-> (rgb (n, 3) float32, final states (n,) uint32)"""
    args, outs = radiance_args(str(d), scene, rays, seeds, spp, rr, base)
    run(tool, args, **kw)
    return np.fromfile(outs[0], "<f4").reshape(-1, 3), np.fromfile(outs[1], "<u4")


def views_args(d, scene, cams, seeds, w, h, spp, policy, chunk, base=None):
    np.ascontiguousarray(cams, "<f4").tofile(os.path.join(d, "cams.f32"))
    np.ascontiguousarray(seeds, "<u4").tofile(os.path.join(d, "vseeds.u32"))
    out = os.path.join(d, "views.f32")
    return ["--views"] + scene_args(scene, base) + [os.path.join(d, "cams.f32"), os.path.join(d, "vseeds.u32"), w, h, spp, policy, chunk, out], [out]


def views(tool, d, scene, cams, seeds, w, h, spp, policy, chunk, base=None, **kw):
    """cams (n, 4, 3): p and the three axes -> frames (n, h, w, 3)"""
    args, outs = views_args(str(d), scene, cams, seeds, w, h, spp, policy, chunk, base)
    run(tool, args, **kw)
    return np.fromfile(outs[0], "<f4").reshape(len(cams), h, w, 3)


def render_args(d, scene, w, h, spp, seed, policy, chunk, base=None, shard=None):
    out = os.path.join(d, "frame.f32")
    return scene_args(scene, base) + [w, h, spp, seed, policy, chunk, out] + (list(shard) if shard else []), [out]


def render(tool, d, scene, w, h, spp, seed, policy, chunk, base=None, **kw):
    args, outs = render_args(str(d), scene, w, h, spp, seed, policy, chunk, base)
    run(tool, args, **kw)
    return np.fromfile(outs[0], "<f4").reshape(h, w, 3)
