"""Throughput of the radiance queries (ort_radiance_device, kernels radiance_rays) against the PIXEL render
(ort_render_image_device) of the same frame and sample count in the same process, one GPU, in paths per second.

Per scene (those of tools/raycast_bench.py), --spp samples per ray:
  frame       the primary rays of a --size x --size frame from the scene's own camera, one per pixel, without the aperture: from
              p - 0.1 z towards the pixel's point on the focal plane (ray.cpp:1215-1240 with the aperture's radius 0), unit
              length.  The comparator renders the same frame with the PIXEL policy and the same spp: the same number of paths
              from (almost) the same rays, its primary rays spread over the aperture.
  incoherent  as many rays with origins uniform in the scene's box (shrunk by 2 % so that none starts outside) and uniform
              directions: no two lanes of a wave start alike.  No render compares; the frame family's comparator stands.
Each gets --warmup calls, then --calls timed calls, one pair of HIP events per call, the three alternating call by call so
that clocks and cache state drift alike.  One JSON line per scene: M paths/s of each from the median call, ratio_frame =
radiance / render on the frame, s = (max - min) / median of the render's timings.  No ratio is required: the line records.
host_us_per_call is raycast_bench.py's, for the frame family's call: at a small --size and --spp, the library's per-call overhead.
usage: python3 tools/radiance_bench.py [--scenes ...] [--size 512] [--spp 64] [--warmup 3] [--calls 7]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import occluded_bench  # noqa: E402
import raycast_bench  # noqa: E402


def frame_rays(torch, cam, size, dev):
    """cam: (4, 3) p, x_axis, y_axis, z_axis -> (size * size, 6) float32, row-major pixels"""
    p, x, y, z = (torch.from_numpy(np.asarray(c, "<f4")).to(dev) for c in cam)
    k = torch.arange(size, device=dev, dtype=torch.float32)
    f = 2.0 * k / float(size) - 1.0
    to_pixel = f[None, :, None] * x + f[:, None, None] * y - z
    to_pixel = to_pixel / to_pixel.norm(dim=2, keepdim=True)
    focal = p + (p - torch.tensor([0.0, 0.0, 0.2], device=dev)).norm() * to_pixel
    o = (p - 0.1 * z).expand(size, size, 3)
    d = focal - o
    d = d / d.norm(dim=2, keepdim=True)
    return torch.cat([o, d], dim=2).reshape(-1, 6).float().contiguous()


def box_rays(torch, lo, hi, n, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    lo, hi = torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev)
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * 0.98
    o = mid + (torch.rand((n, 3), generator=g, device=dev) * 2 - 1) * half
    d = torch.randn((n, 3), generator=g, device=dev)
    d = d / d.norm(dim=1, keepdim=True)
    return torch.cat([o, d], dim=1).float().contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=raycast_bench.SCENES)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--seed", type=int, default=20261017)
    ap.add_argument("--host-calls", type=int, default=400)
    args = ap.parse_args()
    assert args.calls >= 5 and args.warmup >= 2
    import torch
    from offline_raytracer_amd import api
    dev = torch.device("cuda", 0)
    size, spp = args.size, args.spp
    n = size * size
    stream = torch.cuda.Stream(dev)
    for name in args.scenes.split(","):
        scene = api.Scene.load_scn(raycast_bench.scene_path(name)).commit().upload(0)
        flat = scene.flatten(size, size)
        lo, hi = occluded_bench.scene_box(flat)
        families = {"frame": frame_rays(torch, flat.camera, size, dev), "incoherent": box_rays(torch, lo, hi, n, args.seed, dev)}
        seeds = torch.from_numpy(api.job_seeds(args.seed, n).view("<i4")).to(dev)
        rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
        image = torch.empty((size, size, 3), dtype=torch.float32, device=dev)
        params = api.Scene.params(size, size, spp, args.seed, policy="pixel")
        counted = api.Scene.params(size, size, spp, args.seed, policy="pixel", counters=True)
        torch.cuda.synchronize(dev)

        def render(p=params, **kw):
            return scene.render_device(image.data_ptr(), p, stream=stream.cuda_stream, **kw)

        def radiance(fam, **kw):
            return scene.radiance_device(families[fam].data_ptr(), seeds.data_ptr(), n, spp, 0.8, rgb.data_ptr(), stream=stream.cuda_stream, **kw)
        calls = (("render", render), ("frame", lambda **kw: radiance("frame", **kw)), ("incoherent", lambda **kw: radiance("incoherent", **kw)))
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
        st = {"render": render(counted, want_stats=True), "frame": radiance("frame", counters=True, want_stats=True),
              "incoherent": radiance("incoherent", counters=True, want_stats=True)}
        med = {k: float(np.median(v)) for k, v in ms.items()}
        out = {"tool": "radiance_bench", "scene": name, "size": size, "spp": spp, "rays_per_call": n, "warmup": args.warmup, "calls": args.calls,
               "mpaths_per_s_render_pixel": n * spp / (med["render"] * 1e-3) / 1e6,
               "mpaths_per_s_radiance_frame": n * spp / (med["frame"] * 1e-3) / 1e6,
               "mpaths_per_s_radiance_incoherent": n * spp / (med["incoherent"] * 1e-3) / 1e6,
               "ratio_frame": med["render"] / med["frame"], "ratio_incoherent": med["render"] / med["incoherent"],
               "s": (max(ms["render"]) - min(ms["render"])) / med["render"],
               "s_frame": (max(ms["frame"]) - min(ms["frame"])) / med["frame"],
               "s_incoherent": (max(ms["incoherent"]) - min(ms["incoherent"])) / med["incoherent"],
               "ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
               "rays_per_path": {k: v["rays"] / max(1, v["paths"]) for k, v in st.items()},
               "tests_per_path": {k: (v["node_tests"] + v["tri_tests"] + v["analytic_tests"]) / max(1, v["paths"]) for k, v in st.items()},
               "fallback_rays": {k: v["fallback_rays"] for k, v in st.items()},
               "host_us_per_call": raycast_bench.host_us_per_call(calls[1][1], stream.synchronize, args.host_calls),
               "lib": os.path.relpath(api.LIB_PATH, ROOT)}
        print(json.dumps(out), flush=True)
        scene.close()
        del families, seeds, rgb, image
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
