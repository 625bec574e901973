"""Throughput of the SH light-probe query (ort_probe_sh_device, kernels probe_sh_points) against the irradiance query on as many
paths and against the route it replaces, in the same process, one GPU.

Per scene (bunny room, analytic scene, dwarf room) and case (--cases: points x samples, 2^18 x 64 and 2^20 x 16 by default):
  points      probe positions anywhere inside the scene's box with a random unit pole (tools/radiance_bench.py's box_rays: the
              origin is the position, the direction the pole), rr 0.8.
  query       ort_probe_sh_device: the 27 coefficients per point; the plain mean and the states are not asked for.
  irradiance  the comparator on as many paths: ort_irradiance_device on the same points, seeds and sample count (the pole as the
              normal: the same loop, a hemisphere where the query has the sphere, 3 words out where it has 27).
Both get --warmup calls, then --calls timed calls, one pair of HIP events per call, alternating call by call in the same rounds so
that clocks and cache state drift alike.  Then, once per case and whole (wall clock, from the points on the host to the
coefficients on the host):
  route       what a baker does without the query: points * spp uniform directions drawn with numpy, as many 24-byte rays and
              seeds materialised and uploaded, one ort_radiance_device call at spp = 1, a colour per sample downloaded, the
              projection onto api.sh_basis and the mean per point in numpy (in blocks of 2^20 samples).
  query_whole the query's own whole: points and seeds uploaded, the call, the coefficients downloaded.
One JSON line per scene and case: M paths/s of query and irradiance from the median call, ratio = query / irradiance, each side's
spread s = (max - min) / median, the per-path ray and test counts of both (a counted call each), the route's stages in ms, its
ratio to the query's whole, and the bytes each moves across the bus.  No figure is required: the lines record.
usage: python3 tools/probe_bench.py [--scenes ...] [--cases 18x64,20x16] [--warmup 3] [--calls 7]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import occluded_bench  # noqa: E402
import radiance_bench  # noqa: E402
import raycast_bench  # noqa: E402

SCENES = "c3_bunny_room,c2_analytic,c4_dwarf_room"
BLOCK = 1 << 20   # samples per block of the route's numpy projection


def route(torch, api, scene, points_host, n, spp, rr, seed, dev):
    """the replaced route, whole -> (stages in ms, sh float32[n, 9, 3])"""
    rng = np.random.default_rng(seed)
    t = [time.perf_counter()]
    d = rng.standard_normal((n * spp, 3), dtype=np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.empty((n * spp, 6), "<f4")
    rays[:, 0:3] = np.repeat(points_host[:, 0:3], spp, axis=0)
    rays[:, 3:6] = d
    seeds = rng.integers(1, 1 << 31, n * spp, dtype=np.int32)
    t.append(time.perf_counter())
    d_rays, d_seeds = torch.from_numpy(rays).to(dev), torch.from_numpy(seeds).to(dev)
    d_rgb = torch.empty((n * spp, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    t.append(time.perf_counter())
    st = scene.radiance_device(d_rays.data_ptr(), d_seeds.data_ptr(), n * spp, 1, rr, d_rgb.data_ptr(), want_stats=True)
    t.append(time.perf_counter())
    rgb = d_rgb.cpu().numpy()
    t.append(time.perf_counter())
    sums = np.zeros((n, 9, 3), np.float32)
    per = max(1, BLOCK // spp) * spp   # whole points per block
    for at in range(0, n * spp, per):
        b = api.sh_basis(d[at:at + per])
        sums[at // spp:(at + per) // spp] = np.einsum("ksj,ksc->kjc", b.reshape(-1, spp, 9), rgb[at:at + per].reshape(-1, spp, 3))
    sh = sums / np.float32(spp)
    t.append(time.perf_counter())
    ms = {k: (b - a) * 1e3 for k, a, b in zip(("make_rays", "upload", "call", "download", "project"), t, t[1:])}
    ms["kernel"] = st["kernel_ms"]
    ms["whole"] = (t[-1] - t[0]) * 1e3
    return ms, sh


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=SCENES)
    ap.add_argument("--cases", default="18x64,20x16", help="log2(points) x samples, comma-separated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--no-route", action="store_true", help="leave the replaced route out")
    args = ap.parse_args()
    assert args.calls >= 5 and args.warmup >= 2
    import torch
    from offline_raytracer_amd import api
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    rr = 0.8
    cases = [tuple(int(x) for x in c.split("x")) for c in args.cases.split(",")]
    for name in args.scenes.split(","):
        scene = api.Scene.load_scn(raycast_bench.scene_path(name)).commit().upload(0)
        lo, hi = occluded_bench.scene_box(scene.flatten(1, 1))
        for log2n, spp in cases:
            n = 1 << log2n
            points = radiance_bench.box_rays(torch, lo, hi, n, args.seed, dev)
            seeds_host = api.job_seeds(args.seed, n)
            seeds = torch.from_numpy(seeds_host.view("<i4")).to(dev)
            d_sh = torch.empty((n, 27), dtype=torch.float32, device=dev)
            d_rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)

            def query(**kw):
                return scene.probe_sh_device(points.data_ptr(), seeds.data_ptr(), n, spp, rr, d_sh.data_ptr(), stream=stream.cuda_stream, **kw)

            def irradiance(**kw):
                return scene.irradiance_device(points.data_ptr(), seeds.data_ptr(), n, spp, rr, d_rgb.data_ptr(), stream=stream.cuda_stream, **kw)
            calls = (("query", query), ("irradiance", irradiance))
            for _ in range(args.warmup):
                for _, fn in calls:
                    fn()
            stream.synchronize()
            ms = {k: [] for k, _ in calls}
            for _ in range(args.calls):
                for key, fn in calls:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    fn()
                    b.record(stream)
                    b.synchronize()
                    ms[key].append(a.elapsed_time(b))
            st = {k: fn(counters=True, want_stats=True) for k, fn in calls}
            med = {k: float(np.median(v)) for k, v in ms.items()}
            s = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
            ratio = med["irradiance"] / med["query"]
            paths = n * spp
            out = {"tool": "probe_bench", "scene": name, "points": n, "spp": spp, "rr": rr, "warmup": args.warmup, "calls": args.calls,
                   "mpaths_per_s": {k: paths / (v * 1e-3) / 1e6 for k, v in med.items()},
                   "ratio": ratio, "s": s, "ratio_within_spreads": bool(abs(ratio - 1.0) <= s["query"] + s["irradiance"]),
                   "ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                   "rays_per_path": {k: v["rays"] / max(1, v["paths"]) for k, v in st.items()},
                   "tests_per_path": {k: (v["node_tests"] + v["tri_tests"] + v["analytic_tests"]) / max(1, v["paths"]) for k, v in st.items()},
                   "fallback_rays": {k: v["fallback_rays"] for k, v in st.items()},
                   "bytes_query": int(n * (24 + 4 + 108)), "bytes_irradiance": int(n * (24 + 4 + 12)), "bytes_route": int(paths * (24 + 4 + 12)),
                   "lib": os.path.relpath(api.LIB_PATH, ROOT)}
            if not args.no_route:
                points_host = points.cpu().numpy()
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                p2, s2 = torch.from_numpy(points_host).to(dev), torch.from_numpy(seeds_host.view("<i4")).to(dev)
                sh2 = torch.empty((n, 27), dtype=torch.float32, device=dev)
                scene.probe_sh_device(p2.data_ptr(), s2.data_ptr(), n, spp, rr, sh2.data_ptr())
                sh_query = sh2.cpu().numpy().reshape(n, 9, 3)
                whole = (time.perf_counter() - t0) * 1e3
                route_ms, sh_route = route(torch, api, scene, points_host, n, spp, rr, args.seed, dev)
                out["query_whole_ms"] = whole
                out["route_ms"] = route_ms
                out["route_over_query_whole"] = route_ms["whole"] / whole
                # two Monte-Carlo estimates of the same coefficients: their means over the points agree to the noise
                out["mean_sh0"] = {"query": [float(x) for x in sh_query[:, 0].mean(axis=0)], "route": [float(x) for x in sh_route[:, 0].mean(axis=0)]}
                del p2, s2, sh2, sh_query, sh_route
            print(json.dumps(out), flush=True)
            del points, seeds, d_sh, d_rgb
            torch.cuda.empty_cache()
        scene.close()


if __name__ == "__main__":
    main()
