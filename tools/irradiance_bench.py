"""Throughput of the irradiance queries (ort_irradiance_device, kernels irradiance_points) against the radiance queries
(ort_radiance_device) on as many paths in the same process, one GPU, in paths per second.

Per scene (those of tools/raycast_bench.py):
  points      --points surface points found with ort_raycast (rays of radiance_bench.py's incoherent family; the hits on a
              surface, lifted by 1e-3 along the normal on the side the ray came from), --spp samples each, rr 0.8.
  rays        the comparator: ort_radiance on as many rays (p, one cosine-weighted direction about n), the same spp: the same
              number of paths, each ray's samples all along its one direction -- round 9's incoherent family.
Both get --warmup calls, then --calls timed calls, one pair of HIP events per call, alternating call by call so that clocks and
cache state drift alike.  One JSON line per scene: M paths/s of each from the median call, ratio = irradiance / radiance, each
side's spread s = (max - min) / median, whether the ratio lies within the two spreads, and the per-path ray and test counts of
both (a counted call each).  Then, once each:
  today       the route a caller takes without the query: points * spp rays made in torch (a cosine direction per sample), one
              ort_radiance call at spp = 1 over all of them, the mean per point in torch; its time (torch's part and the
              call's) and the bytes of rays and seeds it makes.
  adaptive    ort_irradiance_adaptive_device at min_spp 16, max_spp --max-spp, tolerance 0.1 (floor 0.05, a check every 4)
              against the uniform call at --max-spp: its share of the samples and of the kernel time.
No figure is required: the lines record.
usage: python3 tools/irradiance_bench.py [--scenes ...] [--points 262144] [--spp 64] [--max-spp 1024] [--warmup 3] [--calls 7]"""
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


def surface_points(torch, api, scene, lo, hi, n, seed, dev):
    """-> (n, 6) float32 on the device: p lifted off its surface, n the unit normal on the side the finding ray came from"""
    out, have, k = [], 0, 0
    while have < n:
        rays = radiance_bench.box_rays(torch, lo, hi, 2 * n, seed + k, dev)
        hits = torch.empty((2 * n, 6), dtype=torch.float32, device=dev)
        scene.raycast_device(rays.data_ptr(), 2 * n, hits.data_ptr(), want_stats=True)
        mat = hits.view(torch.int32)[:, 4]
        t, nrm = hits[:, 0:1], hits[:, 1:4]
        o, d = rays[:, 0:3], rays[:, 3:6]
        nrm = torch.where((nrm * d).sum(dim=1, keepdim=True) < 0, nrm, -nrm)
        nrm = nrm / nrm.norm(dim=1, keepdim=True)
        p = o + t * d + 1e-3 * nrm
        keep = (mat != 0) & torch.isfinite(p).all(dim=1) & torch.isfinite(nrm).all(dim=1)
        out.append(torch.cat([p, nrm], dim=1)[keep])
        have += int(keep.sum())
        k += 1
        assert k < 64, "the scene's box holds too few surfaces"
    return torch.cat(out)[:n].float().contiguous()


def cosine_dirs(torch, normals, g):
    """one cosine-weighted direction about each unit normal: normalize(n + a uniform unit vector)"""
    u = torch.randn(normals.shape, generator=g, device=normals.device)
    u = u / u.norm(dim=1, keepdim=True)
    d = normals + u
    length = d.norm(dim=1, keepdim=True)
    d = torch.where(length > 1e-3, d / length, normals)
    return d.float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=raycast_bench.SCENES)
    ap.add_argument("--points", type=int, default=1 << 18)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--max-spp", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--seed", type=int, default=20261019)
    args = ap.parse_args()
    assert args.calls >= 5 and args.warmup >= 2
    import torch
    from offline_raytracer_amd import api
    dev = torch.device("cuda", 0)
    n, spp, rr = args.points, args.spp, 0.8
    stream = torch.cuda.Stream(dev)
    for name in args.scenes.split(","):
        scene = api.Scene.load_scn(raycast_bench.scene_path(name)).commit().upload(0)
        lo, hi = occluded_bench.scene_box(scene.flatten(1, 1))
        points = surface_points(torch, api, scene, lo, hi, n, args.seed, dev)
        g = torch.Generator(device=dev)
        g.manual_seed(args.seed)
        rays = torch.cat([points[:, 0:3], cosine_dirs(torch, points[:, 3:6], g)], dim=1).contiguous()
        seeds = torch.from_numpy(api.job_seeds(args.seed, n).view("<i4")).to(dev)
        rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)

        def irradiance(s=spp, **kw):
            return scene.irradiance_device(points.data_ptr(), seeds.data_ptr(), n, s, rr, rgb.data_ptr(), stream=stream.cuda_stream, **kw)

        def radiance(**kw):
            return scene.radiance_device(rays.data_ptr(), seeds.data_ptr(), n, spp, rr, rgb.data_ptr(), stream=stream.cuda_stream, **kw)
        calls = (("irradiance", irradiance), ("radiance", radiance))
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
        st = {"irradiance": irradiance(counters=True, want_stats=True), "radiance": radiance(counters=True, want_stats=True)}
        med = {k: float(np.median(v)) for k, v in ms.items()}
        s = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
        ratio = med["radiance"] / med["irradiance"]

        # today's route, once: a ray per sample made in torch, one call at spp = 1, the mean in torch
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        p_all = points[:, None, 0:3].expand(n, spp, 3).reshape(-1, 3)
        d_all = cosine_dirs(torch, points[:, None, 3:6].expand(n, spp, 3).reshape(-1, 3), g)
        rays_all = torch.cat([p_all, d_all], dim=1).contiguous()
        seeds_all = torch.randint(1, 1 << 31, (n * spp,), generator=g, device=dev, dtype=torch.int32)
        rgb_all = torch.empty((n * spp, 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        st_today = scene.radiance_device(rays_all.data_ptr(), seeds_all.data_ptr(), n * spp, 1, rr, rgb_all.data_ptr(), want_stats=True)
        mean = rgb_all.reshape(n, spp, 3).mean(dim=1)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        today = {"ms_make_rays": (t1 - t0) * 1e3, "ms_call_and_mean": (t2 - t1) * 1e3, "kernel_ms": st_today["kernel_ms"],
                 "bytes_rays_and_seeds": int(rays_all.numel() * 4 + seeds_all.numel() * 4), "bytes_colours": int(rgb_all.numel() * 4),
                 "mean_luminance": float(mean.mean())}
        del p_all, d_all, rays_all, seeds_all, rgb_all, mean

        # the adaptive form against the uniform call at max_spp
        spp_out = torch.zeros((n,), dtype=torch.int32, device=dev)
        st_uni = irradiance(args.max_spp, want_stats=True)
        st_ad = scene.irradiance_adaptive_device(points.data_ptr(), seeds.data_ptr(), n, 16, args.max_spp, 0.1, 0.05, 4, rr, rgb.data_ptr(),
                                                 d_spp=spp_out.data_ptr(), stream=stream.cuda_stream, want_stats=True)
        taken = int(spp_out.to(torch.int64).sum())
        adaptive = {"min_spp": 16, "max_spp": args.max_spp, "tolerance": 0.1, "floor": 0.05, "check_every": 4,
                    "kernel_ms_uniform": st_uni["kernel_ms"], "kernel_ms_adaptive": st_ad["kernel_ms"],
                    "share_of_samples": taken / float(n * args.max_spp), "share_of_kernel_time": st_ad["kernel_ms"] / st_uni["kernel_ms"]}

        out = {"tool": "irradiance_bench", "scene": name, "points": n, "spp": spp, "rr": rr, "warmup": args.warmup, "calls": args.calls,
               "mpaths_per_s_irradiance": n * spp / (med["irradiance"] * 1e-3) / 1e6,
               "mpaths_per_s_radiance": n * spp / (med["radiance"] * 1e-3) / 1e6,
               "ratio": ratio, "s_irradiance": s["irradiance"], "s_radiance": s["radiance"],
               "ratio_within_spreads": bool(abs(ratio - 1.0) <= s["irradiance"] + s["radiance"]),
               "ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
               "rays_per_path": {k: v["rays"] / max(1, v["paths"]) for k, v in st.items()},
               "tests_per_path": {k: (v["node_tests"] + v["tri_tests"] + v["analytic_tests"]) / max(1, v["paths"]) for k, v in st.items()},
               "fallback_rays": {k: v["fallback_rays"] for k, v in st.items()},
               "today": today, "adaptive": adaptive, "lib": os.path.relpath(api.LIB_PATH, ROOT)}
        print(json.dumps(out), flush=True)
        scene.close()
        del points, rays, seeds, rgb, spp_out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
