"""Throughput of the ambient-occlusion queries (ort_ambient_occlusion_device, kernels ao_points) against today's route -- the
occlusion ray query (ort_occluded_device) over as many materialised rays -- in the same process, one GPU, in rays per second.

Per scene (those of tools/raycast_bench.py), case (--cases: points x samples, 2^18 x 64 and 2^20 x 16 by default) and radius
(5 % of the scene box's diagonal: the ambient family of tools/occluded_bench.py; and none):
  query       ort_ambient_occlusion_device over surface points found with ort_raycast (tools/irradiance_bench.py's), spp samples
              each, the open counts and the bent sums asked for.
  occluded    the comparator: ort_occluded_device over points * spp rays (p, a cosine-weighted direction about n drawn with
              torch: for timing any unit directions about the same normals do), tmax the same radius.
  irradiance  ort_irradiance_device at rr = 0 on the same points and sample counts (the same draw, an unbounded closest hit and a
              material lookup); with the unbounded radius only.
All get --warmup calls, then --calls timed calls, one pair of HIP events per call, alternating call by call so that clocks and
cache state drift alike.  One JSON line per scene, case and radius: G rays/s of each from the median call, ratio = query /
occluded, each side's spread s = (max - min) / median, ok = ratio >= 1 - s of the comparator, the bytes each route moves (24 B
of ray, 4 B of limit and 1 B of answer per ray against at most 52 B per point), the node tests per ray of both (a counted call
each) and the visibility both report.  No figure is required: the lines record.
usage: python3 tools/ao_bench.py [--scenes ...] [--cases 18x64,20x16] [--warmup 3] [--calls 7]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import irradiance_bench  # noqa: E402
import occluded_bench  # noqa: E402
import raycast_bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=raycast_bench.SCENES)
    ap.add_argument("--cases", default="18x64,20x16", help="log2(points) x samples, comma-separated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--seed", type=int, default=20261019)
    args = ap.parse_args()
    assert args.calls >= 5 and args.warmup >= 2
    import torch
    from offline_raytracer_amd import api
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    cases = [tuple(int(x) for x in c.split("x")) for c in args.cases.split(",")]
    for name in args.scenes.split(","):
        scene = api.Scene.load_scn(raycast_bench.scene_path(name)).commit().upload(0)
        lo, hi = occluded_bench.scene_box(scene.flatten(1, 1))
        r05 = float(0.05 * np.linalg.norm((hi - lo).astype(np.float64)))
        for log2n, spp in cases:
            n = 1 << log2n
            points = irradiance_bench.surface_points(torch, api, scene, lo, hi, n, args.seed, dev)
            g = torch.Generator(device=dev)
            g.manual_seed(args.seed)
            seeds = torch.from_numpy(api.job_seeds(args.seed, n).view("<i4")).to(dev)
            rays = torch.cat([points[:, None, 0:3].expand(n, spp, 3).reshape(-1, 3),
                              irradiance_bench.cosine_dirs(torch, points[:, None, 3:6].expand(n, spp, 3).reshape(-1, 3), g)], dim=1).contiguous()
            d_open = torch.empty((n,), dtype=torch.int32, device=dev)
            d_bent = torch.empty((n, 3), dtype=torch.float32, device=dev)
            d_rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
            d_occ = torch.empty((n * spp,), dtype=torch.uint8, device=dev)
            for radius in (r05, None):
                d_rad = torch.full((n,), radius, dtype=torch.float32, device=dev) if radius is not None else None
                d_tmax = torch.full((n * spp,), radius, dtype=torch.float32, device=dev) if radius is not None else None
                torch.cuda.synchronize(dev)

                def query(**kw):
                    return scene.ambient_occlusion_device(points.data_ptr(), seeds.data_ptr(), d_rad.data_ptr() if d_rad is not None else None, n, spp,
                                                          d_open.data_ptr(), d_bent=d_bent.data_ptr(), stream=stream.cuda_stream, **kw)

                def occluded(**kw):
                    return scene.occluded_device(rays.data_ptr(), d_tmax.data_ptr() if d_tmax is not None else None, n * spp, d_occ.data_ptr(),
                                                 stream=stream.cuda_stream, **kw)

                def irradiance(**kw):
                    return scene.irradiance_device(points.data_ptr(), seeds.data_ptr(), n, spp, 0.0, d_rgb.data_ptr(), stream=stream.cuda_stream, **kw)
                calls = [("query", query), ("occluded", occluded)] + ([("irradiance", irradiance)] if radius is None else [])
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
                ratio = med["occluded"] / med["query"]
                total = n * spp
                out = {"tool": "ao_bench", "scene": name, "points": n, "spp": spp, "radius": radius, "warmup": args.warmup, "calls": args.calls,
                       "grays_per_s": {k: total / (v * 1e-3) / 1e9 for k, v in med.items()},
                       "ratio": ratio, "s": s, "ok": bool(ratio >= 1 - s["occluded"]),
                       "ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                       "bytes_query": int(n * (24 + 4 + (4 if radius is not None else 0) + 4 + 12)),
                       "bytes_occluded": int(total * (24 + (4 if radius is not None else 0) + 1)),
                       "node_tests_per_ray": {k: v["node_tests"] / total for k, v in st.items()},
                       "tests_per_ray": {k: (v["node_tests"] + v["tri_tests"] + v["analytic_tests"]) / total for k, v in st.items()},
                       "rays": {k: v["rays"] for k, v in st.items()}, "fallback_rays": {k: v["fallback_rays"] for k, v in st.items()},
                       "visibility_query": float(d_open.to(torch.float64).sum().item() / total),
                       "visibility_occluded": float(1.0 - d_occ.to(torch.float64).mean().item()),
                       "lib": os.path.relpath(api.LIB_PATH, ROOT)}
                if "irradiance" in med:
                    out["ratio_to_irradiance"] = med["irradiance"] / med["query"]
                print(json.dumps(out), flush=True)
                del d_rad, d_tmax
            del points, seeds, rays, d_open, d_bent, d_rgb, d_occ
            torch.cuda.empty_cache()
        scene.close()


if __name__ == "__main__":
    main()
