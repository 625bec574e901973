"""Time, quality and the default parameters of the denoiser (ort_denoise_device; kernels denoise_pack and denoise_atrous of
ort_denoise.h), one GPU, one process.  Per scene, a --width x --height frame from the scene's own camera, three parts in one run:
  time      kernel_ms of the device form (one pair of HIP events around the pack and the passes) at iterations = 1 .. --iterations
            on the --time-spp frame, and of a device-to-device copy of the workspace's bytes (48 per pixel: torch's copy_ between two
            tensors, timed by events on the same stream).  --warmup rounds, then --calls timed rounds, the legs alternating within a
            round.  A call at k iterations is the pack, k - 1 passes that write a (c, var) plane and one that writes out_rgb; the
            pack and the passes apart come from a kernel trace in a run of its own (profiles/r25_denoise.md).  ratio = the whole
            call at --iterations over the copy, from the medians; s = (max - min) / median of each leg.  The copy reads and writes
            48 bytes a pixel once: the floor that ONE memory-bound pass over the workspace could approach, so the call's floor is
            several of them.  bytes_per_call counts what the call must move if every plane is read and written once per kernel.
  quality   RMSE over rgb against a PIXEL render at --ref-spp on another seed: the frame at each of --spp (render_adaptive with
            min == max, which gives the m2 and count planes; guides from render_features at the same count) before and after the
            denoiser at the defaults, and the undenoised frame at --plain-spp beside them.
  grid      the denoised RMSE of every (sigma_l, sigma_z, normal_squarings, iterations) of the grid, per --spp.
One JSON line per scene, and a last line with the grid summed over the scenes and its best entry.  Nothing is required of the
numbers: the lines record.
usage: python3 tools/denoise_bench.py [--scenes c3_bunny_room,c2_analytic] [--width 1920] [--height 1080] [--spp 64,256]
           [--plain-spp 1024] [--ref-spp 16384] [--parts time,quality,grid]"""
import argparse
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID = dict(sigma_l=(2.0, 4.0, 8.0), sigma_z=(0.02, 0.05, 0.1), normal_squarings=(5, 7), iterations=(4, 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c3_bunny_room,c2_analytic")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", default="64,256")
    ap.add_argument("--time-spp", type=int, default=64)
    ap.add_argument("--plain-spp", type=int, default=1024)
    ap.add_argument("--ref-spp", type=int, default=16384)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--parts", default="time,quality,grid")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--seed", type=int, default=2024)
    a = ap.parse_args()
    assert a.calls >= 5 and a.warmup >= 2
    parts = a.parts.split(",")
    import torch
    from offline_raytracer_amd import api
    if api.device_count() < 1:
        raise SystemExit("denoise_bench: no HIP device; nothing here is measured without one")
    dev = torch.device("cuda", 0)
    W, H, n = a.width, a.height, a.width * a.height
    spps = [int(s) for s in a.spp.split(",")]
    defaults = dict(api.DENOISE_DEFAULTS)
    ws_bytes = api.denoise_workspace_bytes(W, H)
    total = {}
    for name in a.scenes.split(","):
        scene = api.Scene.load_scn(os.path.join(ROOT, "data", name + ".scn")).commit().upload(0)
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        rgb, m2, albedo, normal, depth, out = f32(H, W, 3), f32(H, W), f32(H, W, 3), f32(H, W, 3), f32(H, W), f32(H, W, 3)
        count = torch.zeros((H, W), dtype=torch.int32, device=dev)
        ws, ws2 = (torch.zeros(ws_bytes, dtype=torch.uint8, device=dev) for _ in range(2))
        torch.cuda.synchronize(dev)

        def sample(spp):
            """the frame at spp samples a pixel, with its m2 and count planes and its guides"""
            scene.render_adaptive_device(scene.params(W, H, 0, a.seed, "pixel"), spp, spp, 0.3, 0.05, 1, rgb.data_ptr(), count.data_ptr(), m2.data_ptr(),
                                         want_stats=True)
            scene.render_features_device(scene.params(W, H, spp, a.seed, "pixel"), want_stats=True, albedo=albedo.data_ptr(), normal=normal.data_ptr(),
                                         depth=depth.data_ptr())

        def denoise(**kw):
            return api.denoise_device(rgb.data_ptr(), m2.data_ptr(), count.data_ptr(), albedo.data_ptr(), normal.data_ptr(), depth.data_ptr(), W, H,
                                      out.data_ptr(), ws.data_ptr(), ws_bytes, want_stats=True, **dict(defaults, **kw))["kernel_ms"]

        def copy():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ws2.copy_(ws)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        line = {"tool": "denoise_bench", "scene": name, "width": W, "height": H, "defaults": defaults, "workspace_bytes": ws_bytes,
                "lib": os.path.relpath(api.LIB_PATH, ROOT)}
        if "time" in parts:
            sample(a.time_spp)
            legs = [("copy", copy)] + [("iterations_%d" % k, (lambda k=k: denoise(iterations=k))) for k in range(1, a.iterations + 1)]
            ms = {k: [] for k, _ in legs}
            for r in range(a.warmup + a.calls):
                for k, f in legs:
                    t = f()
                    if r >= a.warmup:
                        ms[k].append(t)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            whole = "iterations_%d" % a.iterations
            # what a call must move: the pack reads 48 and writes 32 bytes a pixel, a pass reads 32 (its own entries of both planes)
            # and writes 16, the last pass reads 12 more (albedo) and writes 12
            must = n * (80 + 48 * (a.iterations - 1) + 56)
            line["time"] = {"spp": a.time_spp, "warmup": a.warmup, "calls": a.calls, "median_ms": med,
                            "s": {k: (max(v) - min(v)) / med[k] for k, v in ms.items()},
                            "increment_ms": {"iterations_%d" % k: med["iterations_%d" % k] - med["iterations_%d" % (k - 1)] for k in range(2, a.iterations + 1)},
                            "ratio_call_over_copy": med[whole] / med["copy"],
                            "ratio_range": [min(ms[whole]) / max(ms["copy"]), max(ms[whole]) / min(ms["copy"])],
                            "copy_gb_per_s": 2 * ws_bytes / (med["copy"] * 1e-3) / 1e9, "bytes_per_call": must,
                            "call_gb_per_s": must / (med[whole] * 1e-3) / 1e9, "kernel_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}}
        if "quality" in parts or "grid" in parts:
            ref = f32(H, W, 3)
            scene.render_device(ref.data_ptr(), scene.params(W, H, a.ref_spp, a.seed + 1, "pixel"), want_stats=True)
            rmse = lambda x: float(((x.double() - ref.double()) ** 2).mean().sqrt())
            line["quality"] = {"ref_spp": a.ref_spp}
            scene.render_device(out.data_ptr(), scene.params(W, H, a.plain_spp, a.seed, "pixel"), want_stats=True)
            line["quality"]["rmse_plain_%d" % a.plain_spp] = rmse(out)
            grid = {}
            for spp in spps:
                sample(spp)
                before = rmse(rgb)
                denoise()
                after = rmse(out)
                usable_changed = float((out != rgb).any(dim=2).double().mean())
                line["quality"]["spp_%d" % spp] = {"rmse_before": before, "rmse_after": after, "pixels_changed": usable_changed}
                if "grid" in parts:
                    for sl, sz, sq, it in itertools.product(*[GRID[k] for k in ("sigma_l", "sigma_z", "normal_squarings", "iterations")]):
                        denoise(sigma_l=sl, sigma_z=sz, normal_squarings=sq, iterations=it)
                        key = "sl%g_sz%g_sq%d_it%d" % (sl, sz, sq, it)
                        grid.setdefault(key, {})["spp_%d" % spp] = rmse(out)
            if grid:
                line["grid"] = grid
                for key, v in grid.items():
                    total[key] = total.get(key, 0.0) + sum(v.values())
            del ref
        print(json.dumps(line), flush=True)
        del scene
    if total:
        best = min(total, key=total.get)
        print(json.dumps({"tool": "denoise_bench", "grid_sum_over_scenes_and_spp": total, "best": best, "best_sum": total[best],
                          "defaults_key": "sl%g_sz%g_sq%d_it%d" % (defaults["sigma_l"], defaults["sigma_z"], defaults["normal_squarings"], defaults["iterations"])}),
              flush=True)


if __name__ == "__main__":
    main()
