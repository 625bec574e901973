"""Cost of the feature render that follows mirrors and glass (ort_render_follow_device, kernels follow_pixels) against the
first-hit feature render (ort_render_features_device, kernels feature_pixels), and whether its guides pay in the denoiser.  One
GPU, one process, the scene's own camera.

  cost     per scene of --scenes at --size x --spp, rr --rr, cap --cap: --warmup rounds, then --calls timed rounds, the two calls
           alternating within a round so that clocks and cache state drift alike; a call's time is the library's own kernel_ms.  Per
           scene: the median of each, each side's spread s = (max - min) / median, ratio = follow / features, the rays each casts (a
           counted call each) and its G rays/s, and within = ratio <= 1 + s of the comparator.  On a scene whose materials all have a
           diffuse part every path ends at its first vertex and the ratio is the lane's overhead alone.
  quality  tools/denoise_bench.py's procedure (its steps sit in its main(), so they are repeated here one by one, with the same
           calls and api.DENOISE_DEFAULTS): RMSE over rgb against a PIXEL render at --ref-spp on another seed (rendered in --strips
           horizontal strips, a line of progress after each) of the frame at each of --quality-spp (render_adaptive with min == max),
           undenoised and denoised with each of
             a  the first-hit guides (render_features' albedo, normal, depth);
             b  the followed albedo, normal and depth, as means over the recorded samples (plane * spp / hits, 0 where hits is 0);
             c  the followed albedo (likewise) with the first-hit normal and depth.
One JSON line per scene and part; --md writes the same figures as tables (with --resources, a file of tools/kernel_resources.sh's
lines, the kernels' registers, scratch and LDS before them).  Nothing is required of the numbers: the lines record.
usage: python3 tools/follow_bench.py [--parts cost,quality] [--scenes c2_analytic,glass_room,c3_bunny_room]
           [--quality-scenes c2_analytic,c3_bunny_room] [--size 1920x1080] [--spp 16] [--rr 0.8] [--cap 8] [--md FILE]"""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def resource_rows(path):
    """tools/kernel_resources.sh's lines of the two families -> [(kernel, VGPRs, VGPR spill, SGPR spill, scratch, LDS, occupancy)]"""
    rows = []
    for line in open(path):
        m = re.match(r"((?:feature|follow)_pixels<[01],[01]>) .*?VGPRs=(\d+) .*?ScratchSize \[bytes/lane\]=(\d+) .*?Occupancy \[waves/SIMD\]=(\d+) "
                     r"SGPRs Spill=(\d+) VGPRs Spill=(\d+) LDS Size \[bytes/block\]=(\d+)", line)
        if m:
            rows.append((m.group(1), m.group(2), m.group(6), m.group(5), m.group(3), m.group(7), m.group(4)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="cost,quality")
    ap.add_argument("--scenes", default="c2_analytic,glass_room,c3_bunny_room")
    ap.add_argument("--quality-scenes", default="c2_analytic,c3_bunny_room")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--rr", type=float, default=0.8)
    ap.add_argument("--cap", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--quality-spp", default="64,256")
    ap.add_argument("--ref-spp", type=int, default=16384)
    ap.add_argument("--strips", type=int, default=8)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--md", default="")
    ap.add_argument("--resources", default="")
    a = ap.parse_args()
    assert a.calls >= 5 and a.warmup >= 2
    parts = a.parts.split(",")
    import torch
    from offline_raytracer_amd import api
    if api.device_count() < 1:
        raise SystemExit("follow_bench: no HIP device; nothing here is measured without one")
    dev = torch.device("cuda", 0)
    W, H = (int(v) for v in a.size.split("x"))
    n = W * H
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    if "cost" in parts:
        for name in a.scenes.split(","):
            scene = api.Scene.load_scn(os.path.join(ROOT, "data", name + ".scn")).commit().upload(0)
            first = {"albedo": f32(H, W, 3), "normal": f32(H, W, 3), "depth": f32(H, W), "hits": i32(H, W), "ids": i32(H, W, 2), "states": i32(H, W)}
            followed = dict({k: torch.zeros_like(t) for k, t in first.items()}, bounces=i32(H, W))
            p1, p2 = {k: t.data_ptr() for k, t in first.items()}, {k: t.data_ptr() for k, t in followed.items()}
            torch.cuda.synchronize(dev)
            params = lambda counters=False: api.Scene.params(W, H, a.spp, a.seed, "pixel", 0, None, a.rr, counters)
            calls = [("features", lambda counters=False: scene.render_features_device(params(counters), want_stats=True, **p1)),
                     ("follow", lambda counters=False: scene.render_follow_device(params(counters), a.cap, want_stats=True, **p2))]
            for _ in range(a.warmup):
                for _, fn in calls:
                    fn()
            ms = {k: [] for k, _ in calls}
            for _ in range(a.calls):
                for k, fn in calls:
                    ms[k].append(fn()["kernel_ms"])
            st = {k: fn(counters=True) for k, fn in calls}
            med = {k: float(np.median(v)) for k, v in ms.items()}
            s = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
            ratio = med["follow"] / med["features"]
            emit({"tool": "follow_bench", "part": "cost", "scene": name, "width": W, "height": H, "spp": a.spp, "rr": a.rr, "cap": a.cap,
                  "warmup": a.warmup, "calls": a.calls, "median_ms": med, "s": s, "ratio": ratio, "within": bool(ratio <= 1 + s["features"]),
                  "rays": {k: v["rays"] for k, v in st.items()}, "grays_per_s": {k: st[k]["rays"] / (med[k] * 1e-3) / 1e9 for k in med},
                  "node_tests_per_ray": {k: v["node_tests"] / max(v["rays"], 1) for k, v in st.items()},
                  "recorded_share": float(followed["hits"].double().sum().item() / (n * a.spp)),
                  "bounces_per_recorded": float(followed["bounces"].double().sum().item() / max(followed["hits"].double().sum().item(), 1.0)),
                  "first_hit_planes_equal_where_nothing_is_followed": bool(name != "c3_bunny_room" or all((first[k] == followed[k]).all().item() for k in first)),
                  "ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "lib": os.path.relpath(api.LIB_PATH, ROOT)})
            del first, followed
            torch.cuda.empty_cache()
            scene.close()

    if "quality" in parts:
        defaults = dict(api.DENOISE_DEFAULTS)
        ws_bytes = api.denoise_workspace_bytes(W, H)
        for name in a.quality_scenes.split(","):
            scene = api.Scene.load_scn(os.path.join(ROOT, "data", name + ".scn")).commit().upload(0)
            rgb, m2, out, ref = f32(H, W, 3), f32(H, W), f32(H, W, 3), f32(H, W, 3)
            count, hits = i32(H, W), i32(H, W)
            g1 = {"albedo": f32(H, W, 3), "normal": f32(H, W, 3), "depth": f32(H, W)}
            g2 = {k: torch.zeros_like(t) for k, t in g1.items()}
            ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            for k in range(a.strips):   # the reference, a strip at a time: every pixel is its own job on its own stream
                y0, y1 = H * k // a.strips, H * (k + 1) // a.strips
                st = scene.render_device(ref.data_ptr(), scene.params(W, H, a.ref_spp, a.seed + 1, "pixel", 0, (0, y0, W, y1)), want_stats=True)
                print("follow_bench: %s reference rows %d..%d in %.0f ms" % (name, y0, y1, st["kernel_ms"]), file=sys.stderr, flush=True)
            rmse = lambda x: float(((x.double() - ref.double()) ** 2).mean().sqrt())

            def denoise(albedo, normal, depth):
                api.denoise_device(rgb.data_ptr(), m2.data_ptr(), count.data_ptr(), albedo.data_ptr(), normal.data_ptr(), depth.data_ptr(), W, H,
                                   out.data_ptr(), ws.data_ptr(), ws_bytes, want_stats=True, **defaults)
                return rmse(out)
            line = {"tool": "follow_bench", "part": "quality", "scene": name, "width": W, "height": H, "ref_spp": a.ref_spp, "rr": a.rr, "cap": a.cap,
                    "defaults": defaults}
            for spp in (int(v) for v in a.quality_spp.split(",")):
                scene.render_adaptive_device(scene.params(W, H, 0, a.seed, "pixel"), spp, spp, 0.3, 0.05, 1, rgb.data_ptr(), count.data_ptr(), m2.data_ptr(),
                                             want_stats=True)
                scene.render_features_device(scene.params(W, H, spp, a.seed, "pixel"), want_stats=True, **{k: t.data_ptr() for k, t in g1.items()})
                scene.render_follow_device(api.Scene.params(W, H, spp, a.seed, "pixel", 0, None, a.rr), a.cap, want_stats=True, hits=hits.data_ptr(),
                                           **{k: t.data_ptr() for k, t in g2.items()})
                h = hits.float()
                over = {k: torch.where((h > 0)[(...,) + (None,) * (t.dim() - 2)], t * float(spp) / h.clamp(min=1.0)[(...,) + (None,) * (t.dim() - 2)],
                                       torch.zeros_like(t)).contiguous() for k, t in g2.items()}
                line["spp_%d" % spp] = {"rmse_before": rmse(rgb), "a_first_hit": denoise(g1["albedo"], g1["normal"], g1["depth"]),
                                        "b_followed": denoise(over["albedo"], over["normal"], over["depth"]),
                                        "c_followed_albedo": denoise(over["albedo"], g1["normal"], g1["depth"]),
                                        "recorded_share": float(h.double().sum().item() / (n * spp)),
                                        "pixels_nothing_recorded": float((h == 0).double().mean().item())}
                del over
            emit(line)
            del rgb, m2, out, ref, count, hits, g1, g2, ws
            torch.cuda.empty_cache()
            scene.close()

    if a.md:
        with open(a.md, "w") as f:
            f.write("# Feature renders that follow mirrors and glass: resources, cost, and whether the guides pay\n\n")
            if a.resources:
                f.write("## Resources (tools/kernel_resources.sh; <counters, tabs>)\n\n| kernel | VGPRs | VGPR spill | SGPR spill | scratch B/lane | LDS B/block | waves/SIMD |\n|---|---|---|---|---|---|---|\n")
                for r in resource_rows(a.resources):
                    f.write("| `%s` | %s |\n" % (r[0], " | ".join(r[1:])))
                f.write("\n")
            cost = [l for l in lines if l["part"] == "cost"]
            if cost:
                c0 = cost[0]
                f.write("## Cost: %d x %d x %d spp, rr %g, cap %d; %d warm-up rounds, %d timed rounds, the calls alternating\n\n" %
                        (c0["width"], c0["height"], c0["spp"], c0["rr"], c0["cap"], c0["warmup"], c0["calls"]))
                f.write("| scene | features ms (s) | follow ms (s) | ratio | within 1 + s | rays features | rays follow | G rays/s features | G rays/s follow | recorded | bounces / recorded |\n"
                        "|---|---|---|---|---|---|---|---|---|---|---|\n")
                for l in cost:
                    f.write("| %s | %.3f (%.3f) | %.3f (%.3f) | %.3f | %s | %d | %d | %.2f | %.2f | %.3f | %.3f |\n" %
                            (l["scene"], l["median_ms"]["features"], l["s"]["features"], l["median_ms"]["follow"], l["s"]["follow"], l["ratio"],
                             "yes" if l["within"] else "no", l["rays"]["features"], l["rays"]["follow"], l["grays_per_s"]["features"], l["grays_per_s"]["follow"],
                             l["recorded_share"], l["bounces_per_recorded"]))
                f.write("\n")
            qual = [l for l in lines if l["part"] == "quality"]
            if qual:
                f.write("## Whether it pays: RMSE against %d spp on another seed, the denoiser at its defaults\n\n" % qual[0]["ref_spp"])
                f.write("| scene | spp | not denoised | (a) first-hit guides | (b) followed albedo, normal, depth | (c) followed albedo, first-hit normal and depth |\n|---|---|---|---|---|---|\n")
                for l in qual:
                    for k in sorted((k for k in l if k.startswith("spp_")), key=lambda k: int(k[4:])):
                        v = l[k]
                        f.write("| %s | %s | %.5f | %.5f | %.5f | %.5f |\n" % (l["scene"], k[4:], v["rmse_before"], v["a_first_hit"], v["b_followed"], v["c_followed_albedo"]))
                f.write("\n")


if __name__ == "__main__":
    main()
