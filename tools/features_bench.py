"""Throughput of the first-hit feature render (ort_render_features_device, kernels feature_pixels) against the route it replaces
and against the render of the same frame, in the same process, one GPU.

Per scene (c2_analytic, c3_bunny_room, c4_dwarf_room by default), at --size (1920x1080) and --spp (16), the scene's own camera:
  features  (a) ort_render_features_device, all five feature planes and the final states asked for.
  raycast   (b) today's route minus its host gather: ort_raycast_device over as many materialised camera rays through the same
            pixels (the aperture angle drawn with torch: for timing any angle does; not bit-exact).
  render    (c) ort_render_image_device, PIXEL policy, the same spp, rr = 0: the same primary rays plus shading.
  --variants: (a) again under other batch knobs (NAME:ENV=V+ENV=V,...; the library reads them at every call under
            ORT_KNOBS_LIVE=1), e.g. the ray queries' own rule rq:ORT_JOB_BATCH=1024+ORT_BATCH_TAIL=4.
All get --warmup calls, then --calls timed calls, alternating call by call so that clocks and cache state drift alike; a call's
time is the library's own kernel_ms (one pair of HIP events around its kernel).  One JSON line per scene: G rays/s of each from the
median call (pixels x spp / kernel_ms), a/b and a/c, each side's spread s = (max - min) / median, ok = a/b >= 1 - s of (b), the bytes
each route moves (24 B of ray up and 24 B of hit down per sample against 40 B of planes per pixel), node tests per ray of (a) and
(b) from a counted call each, and the coverage both report.  No figure is required: the lines record.
usage: python3 tools/features_bench.py [--scenes ...] [--size 1920x1080] [--spp 16] [--warmup 3] [--calls 7] [--variants ...]"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def camera_rays(torch, cam, w, h, spp, seed, dev):
    """(h * w * spp, 6) float32: the render's camera sample through every pixel centre, the aperture angle from torch's generator"""
    p, X, Y, Z = [torch.tensor(c, dtype=torch.float32, device=dev) for c in np.asarray(cam, "<f4")]
    fl = torch.linalg.norm(p - torch.tensor([0.0, 0.0, 0.2], device=dev))
    ys, xs = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32), indexing="ij")
    to_pixel = (2 * xs / w - 1)[..., None] * X + (2 * ys / h - 1)[..., None] * Y - Z
    focal = p + fl * to_pixel / torch.linalg.norm(to_pixel, dim=-1, keepdim=True)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rad = torch.rand((h, w, spp), generator=g, device=dev) * (2 * math.pi)
    ap = p + 0.1 * torch.cos(rad)[..., None] * X + 0.1 * torch.sin(rad)[..., None] * Y - 0.1 * Z
    d = focal[:, :, None, :] - ap
    d = d / torch.linalg.norm(d, dim=-1, keepdim=True)
    return torch.cat([ap, d], dim=-1).reshape(-1, 6).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c2_analytic,c3_bunny_room,c4_dwarf_room")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--variants", default="", help="NAME:ENV=V+ENV=V,... : the feature call again under these knobs")
    args = ap.parse_args()
    assert args.calls >= 5 and args.warmup >= 2
    os.environ.setdefault("ORT_KNOBS_LIVE", "1")
    import torch
    from offline_raytracer_amd import api
    dev = torch.device("cuda", 0)
    w, h = (int(v) for v in args.size.split("x"))
    spp, n = args.spp, w * h
    variants = {}
    for v in filter(None, args.variants.split(",")):
        name, envs = v.split(":")
        variants[name] = dict(e.split("=") for e in envs.split("+"))
    for name in args.scenes.split(","):
        scene = api.Scene.load_scn(os.path.join(ROOT, "data", name + ".scn")).commit().upload(0)
        rays = camera_rays(torch, scene.camera(w, h), w, h, spp, args.seed, dev)
        d_hits = torch.empty((n * spp * 24,), dtype=torch.uint8, device=dev)
        planes = {"albedo": torch.empty((h, w, 3), dtype=torch.float32, device=dev), "normal": torch.empty((h, w, 3), dtype=torch.float32, device=dev),
                  "depth": torch.empty((h, w), dtype=torch.float32, device=dev), "hits": torch.empty((h, w), dtype=torch.int32, device=dev),
                  "ids": torch.empty((h, w, 2), dtype=torch.int32, device=dev), "states": torch.empty((h, w), dtype=torch.int32, device=dev)}
        d_rgb = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        ptrs = {k: t.data_ptr() for k, t in planes.items()}
        torch.cuda.synchronize(dev)

        def features(env=None, counters=False):
            for k, v in (env or {}).items():
                os.environ[k] = v
            try:
                return scene.render_features_device(api.Scene.params(w, h, spp, args.seed, "pixel", counters=counters), want_stats=True, **ptrs)
            finally:
                for k in env or {}:
                    del os.environ[k]

        def raycast(counters=False):
            return scene.raycast_device(rays.data_ptr(), n * spp, d_hits.data_ptr(), counters=counters, want_stats=True)

        def render(counters=False):
            return scene.render_device(d_rgb.data_ptr(), api.Scene.params(w, h, spp, args.seed, "pixel", rr=0.0, counters=counters), want_stats=True)
        calls = [("features", features), ("raycast", raycast), ("render", render)]
        calls += [(k, (lambda env: lambda counters=False: features(env, counters))(env)) for k, env in variants.items()]
        for _ in range(args.warmup):
            for _, fn in calls:
                fn()
        ms = {k: [] for k, _ in calls}
        for _ in range(args.calls):
            for key, fn in calls:
                ms[key].append(fn()["kernel_ms"])
        st = {k: fn(counters=True) for k, fn in calls if k != "render"}
        med = {k: float(np.median(v)) for k, v in ms.items()}
        s = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
        total = n * spp
        hit_records = d_hits.cpu().numpy().view(api.HIT_DTYPE)
        out = {"tool": "features_bench", "scene": name, "width": w, "height": h, "spp": spp, "warmup": args.warmup, "calls": args.calls,
               "grays_per_s": {k: total / (v * 1e-3) / 1e9 for k, v in med.items()},
               "a_over_b": med["raycast"] / med["features"], "a_over_c": med["render"] / med["features"], "s": s,
               "ok": bool(med["raycast"] / med["features"] >= 1 - s["raycast"]),
               "ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
               "bytes_features": int(n * 40), "bytes_raycast": int(total * 48), "bytes_render": int(n * 12),
               "node_tests_per_ray": {k: v["node_tests"] / total for k, v in st.items()},
               "rays": {k: v["rays"] for k, v in st.items()}, "fallback_rays": {k: v["fallback_rays"] for k, v in st.items()},
               "coverage_features": float(planes["hits"].to(torch.float64).sum().item() / total),
               "coverage_raycast": float((hit_records["mat"] != 0).mean()),
               "variants": variants, "lib": os.path.relpath(api.LIB_PATH, ROOT)}
        print(json.dumps(out), flush=True)
        del rays, d_hits, planes, d_rgb, hit_records
        torch.cuda.empty_cache()
        scene.close()


if __name__ == "__main__":
    main()
