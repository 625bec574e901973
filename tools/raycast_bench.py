"""Throughput of the closest-hit ray queries (ort_raycast_device, kernel raycast_rays) on one GPU.

Per scene: 2^24 rays per call (the golden tables' distribution -- origins in and around the room, uniform unit
directions -- drawn on the device from a fixed seed), warm-up calls, then calls until at least --seconds of timed work;
the rate comes from HIP events around the calls.  One more call with ORT_RENDER_COUNTERS gives the work per ray.
host_us_per_call is the wall time of a call on the host, enqueued and with want_stats (quartiles of --host-calls calls each):
at a small --rays-log2 it is the library's per-call overhead.
Prints one JSON line per scene.  For the kernel time alone run it under rocprofv3 --kernel-trace --stats.
--dirs axis casts the same origins along the six axis directions (+-x, +-y, +-z with +-0 in the other components,
e.g. height probes): the directions whose 1/d has infinite components.
usage: python3 tools/raycast_bench.py [--scenes c2_analytic,c3_bunny_room,...] [--rays-log2 24] [--warmup 5] [--seconds 1]
                                      [--dirs uniform|axis]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SCENES = "c2_analytic,c3_bunny_room,c4_dwarf_room,c5_heightfield_708"


def scene_path(name):
    if name.startswith("c5_heightfield_"):
        import make_heightfield
        path, _, _ = make_heightfield.write_scene(int(name.rsplit("_", 1)[1]), tempfile.mkdtemp(prefix="c5_"))
        return path
    return os.path.join(ROOT, "data", name + ".scn")


def make_rays(torch, n, seed, dev, dirs="uniform"):
    """tests/golden/make_golden.py's distribution: half the origins near the middle of the room, half anywhere in it"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    u = torch.rand((n, 3), generator=g, device=dev)
    lo = torch.tensor([-2.5, -2.5, 0.05], device=dev)
    hi = torch.tensor([14.5, 14.5, 8.8], device=dev)
    o = lo + u * (hi - lo)
    h = n // 2
    lo2 = torch.tensor([-1.5, -1.8, 0.05], device=dev)
    hi2 = torch.tensor([1.5, 1.5, 2.5], device=dev)
    o[:h] = lo2 + u[:h] * (hi2 - lo2)
    d = torch.randn((n, 3), generator=g, device=dev)
    d = d / d.norm(dim=1, keepdim=True)
    if dirs == "axis":  # the largest component's axis and sign, the other two +0 or -0 (their signs kept)
        k = d.abs().argmax(dim=1, keepdim=True)
        d = torch.where(torch.arange(3, device=dev)[None, :] == k, torch.sign(d), d * 0)
    return torch.cat([o, d], dim=1).float().contiguous()


def host_us_per_call(call, sync, calls):
    """{"enqueue" | "want_stats": [first quartile, median, third quartile]} of the wall time of call(), in microseconds"""
    out = {}
    for key, kw in (("enqueue", {}), ("want_stats", {"want_stats": True})):
        sync()
        us = []
        for _ in range(calls):
            t0 = time.perf_counter()
            call(**kw)
            us.append((time.perf_counter() - t0) * 1e6)
        us.sort()
        out[key] = [round(us[len(us) * q // 4], 2) for q in (1, 2, 3)]
    sync()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=SCENES)
    ap.add_argument("--host-calls", type=int, default=400)
    ap.add_argument("--rays-log2", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=20261016)
    ap.add_argument("--dirs", choices=["uniform", "axis"], default="uniform")
    args = ap.parse_args()
    import torch
    from offline_raytracer_amd import api
    dev = torch.device("cuda", 0)
    n = 1 << args.rays_log2
    stream = torch.cuda.Stream(dev)
    for name in args.scenes.split(","):
        t0 = time.time()
        scene = api.Scene.load_scn(scene_path(name)).commit().upload(0)
        load_s = time.time() - t0
        rays = make_rays(torch, n, args.seed, dev, args.dirs)
        hits = torch.empty(n * 24, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        call = lambda **kw: scene.raycast_device(rays.data_ptr(), n, hits.data_ptr(), stream=stream.cuda_stream, **kw)  # noqa: E731
        for _ in range(args.warmup):
            call()
        stream.synchronize()
        ev = []
        total_ms, calls = 0.0, 0
        while total_ms < args.seconds * 1e3:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(8):
                call()
            b.record(stream)
            b.synchronize()
            total_ms += a.elapsed_time(b)
            calls += 8
            ev.append(a.elapsed_time(b) / 8)
        st = call(want_stats=True)  # kernel time of one call by the library's own events
        sc = call(counters=True, want_stats=True)
        h = hits.view(torch.float32).view(-1, 6)[:, 0]
        hit_fraction = float((h < 3.4e38).float().mean().item())
        out = {"tool": "raycast_bench", "scene": name, "dirs": args.dirs, "rays_per_call": n, "calls": calls, "timed_ms": round(total_ms, 3),
               "grays_per_s": n * calls / (total_ms * 1e-3) / 1e9,
               "ms_per_call_median": sorted(ev)[len(ev) // 2], "kernel_ms": st["kernel_ms"],
               "grays_per_s_kernel_ms": n / (st["kernel_ms"] * 1e-3) / 1e9,
               "node_tests_per_ray": sc["node_tests"] / n, "tri_tests_per_ray": sc["tri_tests"] / n,
               "analytic_tests_per_ray": sc["analytic_tests"] / n, "fallback_rays": sc["fallback_rays"],
               "host_us_per_call": host_us_per_call(call, stream.synchronize, args.host_calls), "counted_rays": sc["rays"], "hit_fraction": hit_fraction, "tree": scene.tree_info(), "load_s": round(load_s, 2),
               "lib": os.path.relpath(api.LIB_PATH, ROOT)}
        print(json.dumps(out), flush=True)
        scene.close()
        del rays, hits
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
