"""What the accumulating render (ort_render_accumulate_device; kernels pt_accumulate) costs against the sample-map render it
extends, and what splitting a frame's samples into passes costs, same process, one GPU.

Per scene, a --width x --height frame from the scene's own camera, two parts in one run.  Every leg runs --warmup rounds and then
--calls timed rounds, the legs of a part alternating within a round; a leg reports its median and s = (max - min) / median of
its own timings.
  fresh   one pass of --spp samples from count == 0 (no map, m2 and out_rgb given) against ort_render_sample_map_device with a
          constant map of --spp: kernel_ms of each call (one pair of HIP events around the launch).  out_rgb, m2 and the states of
          the two are compared bit for bit first.
  split   --total samples as 1 x total, 4 x total/4, 16 x total/16 and 64 x total/64 on one stream, count zeroed before every
          round: "kernel" is the sum of the passes' kernel_ms (every call asked for stats, so every call waits), "wall" the host's
          clock around the same passes enqueued with stats == NULL and one synchronisation at the end.  fixed_ms_per_pass is
          (t(P passes) - t(1 pass)) / (P - 1).  The four planes after every split are compared bit for bit with the single pass's.
  bytes   what a pass moves per pixel by the contract (no map): 4 read where the job is drawn, 20 more for a continued pixel
          (state, sum, m2), 24 written (sum, m2, count, state) and 12 more with out_rgb.
One JSON line per scene.  Nothing is required of the numbers: the line records.
usage: python3 tools/accumulate_bench.py [--scenes c3_bunny_room,c2_analytic] [--width 1920] [--height 1080] [--spp 256] [--total 1024]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(v):
    return {"median_ms": float(np.median(v)), "s": (max(v) - min(v)) / float(np.median(v)), "all_ms": [round(x, 4) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c3_bunny_room,c2_analytic")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--total", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2024)
    a = ap.parse_args()
    assert a.calls >= 3 and a.warmup >= 1 and a.total % 64 == 0
    import torch
    from offline_raytracer_amd import api
    dev = torch.device("cuda", 0)
    W, H, n = a.width, a.height, a.width * a.height
    stream = torch.cuda.Stream(dev)
    for name in a.scenes.split(","):
        scene = api.Scene.load_scn(os.path.join(ROOT, "data", name + ".scn")).commit().upload(0)
        with torch.cuda.stream(stream):
            rgb = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
            acc_sum = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
            m2 = torch.zeros((H, W), dtype=torch.float32, device=dev)
            count = torch.zeros((H, W), dtype=torch.int32, device=dev)
            states = torch.zeros((H, W), dtype=torch.int32, device=dev)
            smap = torch.full((H, W), a.spp, dtype=torch.int32, device=dev)
        stream.synchronize()

        def accumulate(k, want_stats):
            return scene.render_accumulate_device(scene.params(W, H, k, a.seed, "pixel"), acc_sum.data_ptr(), count.data_ptr(), states.data_ptr(),
                                                  d_m2=m2.data_ptr(), d_rgb=rgb.data_ptr(), stream=stream.cuda_stream, want_stats=want_stats)

        def fresh():
            with torch.cuda.stream(stream):
                count.zero_()
            return accumulate(a.spp, True)["kernel_ms"]

        def mapped():
            return scene.render_sample_map_device(scene.params(W, H, a.spp, a.seed, "pixel"), smap.data_ptr(), rgb.data_ptr(), m2.data_ptr(),
                                                  states.data_ptr(), stream=stream.cuda_stream, want_stats=True)["kernel_ms"]

        def planes():
            stream.synchronize()
            return [x.clone().view(torch.int32) for x in (rgb, m2, states)]
        out = {"tool": "accumulate_bench", "scene": name, "width": W, "height": H, "warmup": a.warmup, "calls": a.calls,
               "lib": os.path.relpath(api.LIB_PATH, ROOT)}
        # ---- one fresh pass against the sample-map render ----
        ms = {"accumulate": [], "sample_map": []}
        for r in range(a.warmup + a.calls):
            for k, f in (("sample_map", mapped), ("accumulate", fresh)):
                t = f()
                if r == 0:
                    ms[k + "_planes"] = planes()
                if r >= a.warmup:
                    ms[k].append(t)
        same = all(bool(torch.equal(x, y)) for x, y in zip(ms.pop("accumulate_planes"), ms.pop("sample_map_planes")))
        legs = {k: summary(v) for k, v in ms.items()}
        out["fresh"] = {"spp": a.spp, "planes_identical": same, "legs": legs,
                        "accumulate_over_sample_map": legs["accumulate"]["median_ms"] / legs["sample_map"]["median_ms"],
                        "mpaths_per_s": {k: n * a.spp / (v["median_ms"] * 1e-3) / 1e6 for k, v in legs.items()}}
        # ---- the same total in 1, 4, 16 and 64 passes ----
        splits = (1, 4, 16, 64)
        kernel, wall, identical, single = {p: [] for p in splits}, {p: [] for p in splits}, {}, None
        for r in range(a.warmup + a.calls):
            for p in splits:
                with torch.cuda.stream(stream):
                    count.zero_()
                stream.synchronize()
                t = sum(accumulate(a.total // p, True)["kernel_ms"] for _ in range(p))
                with torch.cuda.stream(stream):
                    count.zero_()
                stream.synchronize()
                t0 = time.perf_counter()
                for _ in range(p):
                    accumulate(a.total // p, False)
                stream.synchronize()
                w = (time.perf_counter() - t0) * 1e3
                if r == 0:
                    now = [x.clone().view(torch.int32) for x in (acc_sum, m2, count, states, rgb)]
                    single = now if p == 1 else single
                    identical[p] = all(bool(torch.equal(x, y)) for x, y in zip(now, single))
                if r >= a.warmup:
                    kernel[p].append(t)
                    wall[p].append(w)
        k1, w1 = float(np.median(kernel[1])), float(np.median(wall[1]))
        out["split"] = {"total": a.total, "passes": {str(p): {"spp_per_pass": a.total // p, "planes_identical_to_one_pass": identical[p],
                                                             "kernel": summary(kernel[p]), "wall": summary(wall[p]),
                                                             "kernel_over_one_pass": float(np.median(kernel[p])) / k1,
                                                             "wall_over_one_pass": float(np.median(wall[p])) / w1,
                                                             **({"fixed_kernel_ms_per_pass": (float(np.median(kernel[p])) - k1) / (p - 1),
                                                                 "fixed_wall_ms_per_pass": (float(np.median(wall[p])) - w1) / (p - 1)} if p > 1 else {})}
                                               for p in splits}}
        out["bytes"] = {"per_pixel_read_fresh": 4, "per_pixel_read_continued": 24, "per_pixel_written": 24, "per_pixel_written_with_out_rgb": 36,
                        "per_pass_mib_fresh": n * (4 + 36) / 2 ** 20, "per_pass_mib_continued": n * (24 + 36) / 2 ** 20}
        print(json.dumps(out), flush=True)
        scene.close()
        del rgb, acc_sum, m2, count, states, smap
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
