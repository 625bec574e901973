"""Overhead and payoff of the adaptive radiance queries (ort_radiance_adaptive_device, kernels radiance_adaptive_rays) against
ort_radiance_device on the same rays in the same process, one GPU.

Per scene, the rays are the primary rays of a --size x --size pinhole frame from the scene's own camera (radiance_bench.frame_rays).
  overhead  the adaptive query with min_spp == max_spp == --spp (no check ever runs) against ort_radiance at spp = --spp: --warmup
            calls, then --calls timed calls of each, alternating, one pair of HIP events per call (as tools/radiance_bench.py).
            ratio = samples per second adaptive / uniform from the median calls; s = (max - min) / median of the uniform call's
            own timings: a ratio within 1 - s of 1 is inside the yardstick's noise.
  payoff    at max_spp = --max-spp (min_spp 16, a check every 16, floor 0.05) and each of --tolerances: the samples taken against
            count x max_spp, the kernel time against the uniform call at max_spp, and the RMSE (over rgb, of the rays finite in
            all three) of both -- the uniform call given the same total samples, rounded up per ray -- against ort_radiance at
            --ref-spp on another stream of seeds.
One JSON line per scene.  Nothing is required of the numbers: the line records.
usage: python3 tools/adaptive_bench.py [--scenes ...] [--size 512] [--spp 256] [--max-spp 1024] [--tolerances 0.1,0.05]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import radiance_bench  # noqa: E402
import raycast_bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c3_bunny_room,c2_analytic,c4_dwarf_room")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--max-spp", type=int, default=1024)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--tolerances", default="0.1,0.05")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261018)
    args = ap.parse_args()
    assert args.calls >= 5 and args.warmup >= 2
    import torch
    from offline_raytracer_amd import api
    dev = torch.device("cuda", 0)
    size, n = args.size, args.size * args.size
    stream = torch.cuda.Stream(dev)
    for name in args.scenes.split(","):
        scene = api.Scene.load_scn(raycast_bench.scene_path(name)).commit().upload(0)
        rays = radiance_bench.frame_rays(torch, scene.flatten(size, size).camera, size, dev)
        seeds = torch.from_numpy(api.job_seeds(args.seed, n).view("<i4")).to(dev)
        ref_seeds = torch.from_numpy(api.job_seeds(args.seed + 1, n).view("<i4")).to(dev)
        rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
        spp = torch.empty((n,), dtype=torch.int32, device=dev)
        m2 = torch.empty((n,), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)

        def uniform(k, sd=seeds, **kw):
            return scene.radiance_device(rays.data_ptr(), sd.data_ptr(), n, k, 0.8, rgb.data_ptr(), stream=stream.cuda_stream, **kw)

        def adaptive(lo, hi, tol, every=16, **kw):
            return scene.radiance_adaptive_device(rays.data_ptr(), seeds.data_ptr(), n, lo, hi, tol, 0.05, every, 0.8, rgb.data_ptr(), spp.data_ptr(),
                                                  m2.data_ptr(), stream=stream.cuda_stream, **kw)
        calls = (("uniform", lambda: uniform(args.spp)), ("adaptive", lambda: adaptive(args.spp, args.spp, 0.1)))
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
        med = {k: float(np.median(v)) for k, v in ms.items()}
        out = {"tool": "adaptive_bench", "scene": name, "size": size, "rays_per_call": n, "warmup": args.warmup, "calls": args.calls,
               "overhead": {"spp": args.spp, "msamples_per_s_uniform": n * args.spp / (med["uniform"] * 1e-3) / 1e6,
                            "msamples_per_s_adaptive": n * args.spp / (med["adaptive"] * 1e-3) / 1e6,
                            "ratio": med["uniform"] / med["adaptive"], "s": (max(ms["uniform"]) - min(ms["uniform"])) / med["uniform"],
                            "s_adaptive": (max(ms["adaptive"]) - min(ms["adaptive"])) / med["adaptive"],
                            "ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}},
               "payoff": [], "lib": os.path.relpath(api.LIB_PATH, ROOT)}
        uniform(args.ref_spp, ref_seeds, want_stats=True)
        ref = rgb.clone()
        st_full = uniform(args.max_spp, want_stats=True)

        def rmse(x):
            ok = torch.isfinite(x).all(dim=1) & torch.isfinite(ref).all(dim=1)
            return float(((x[ok].double() - ref[ok].double()) ** 2).mean().sqrt())
        rmse_full = rmse(rgb)
        for tol in (float(t) for t in args.tolerances.split(",")):
            st = adaptive(16, args.max_spp, tol, want_stats=True)
            taken = int(spp.long().sum())
            e_ad = rmse(rgb)
            same = -(-taken // n)   # the uniform call with the same total, rounded up per ray
            st_same = uniform(same, want_stats=True)
            out["payoff"].append({"tolerance": tol, "min_spp": 16, "check_every": 16, "floor": 0.05, "max_spp": args.max_spp,
                                  "samples_taken": taken, "samples_uniform": n * args.max_spp, "fraction": taken / (n * args.max_spp),
                                  "kernel_ms_adaptive": st["kernel_ms"], "kernel_ms_uniform_max_spp": st_full["kernel_ms"],
                                  "uniform_same_total_spp": same, "kernel_ms_uniform_same_total": st_same["kernel_ms"],
                                  "rmse_adaptive": e_ad, "rmse_uniform_same_total": rmse(rgb), "rmse_uniform_max_spp": rmse_full,
                                  "rays_at_min_spp": int((spp == 16).sum()), "rays_at_max_spp": int((spp == args.max_spp).sum())})
        print(json.dumps(out), flush=True)
        scene.close()
        del rays, seeds, ref_seeds, rgb, spp, m2, ref
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
