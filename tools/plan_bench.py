"""Time and use of the sample planner (ort_plan_samples_device; kernels sampleplan_error, sampleplan_want and sampleplan_scale of
ort_sampleplan.h), one GPU, one process.  Per scene, a --width x --height frame from the scene's own camera, three parts in one
run; the frame's planes are those of an accumulating pilot of --pilot samples a pixel (ort_render_accumulate_device).
  time      kernel_ms of the device form (one pair of HIP events around the zeroing of the totals and the three kernels) at radius
            0 .. 3, unscaled (no budget: sampleplan_scale reads the totals and ends) and scaled (a budget of half of what is
            wanted: it rewrites the map), with the window as the call takes it and forced to direct loads and to the LDS tile
            (ORT_PLAN_TILE=0 / 1), and of a device-to-device copy that moves the bytes the unscaled plan moves (36 a pixel:
            20 read and 4 written by the error step, 8 read and 4 written by the want step, so the copy is of 18 bytes a pixel;
            torch's copy_, timed by events on the same stream).  --warmup rounds, then --calls timed rounds, the legs alternating
            within a round; ratio = the plan over the copy, from the medians; s = (max - min) / median of each leg.  The three
            kernels apart come from a kernel trace in a run of its own (profiles/r26_sample_plan.md).
  two_pass  the two-pass scheme of tools/sample_map_bench.py on the accumulating render -- a pilot, a map for B more samples, a
            second pass that continues the pilot's streams -- with the map planned on the device (plan, one read of 32 bytes) and
            built on the host as that tool builds it (the sum and m2 planes downloaded, numpy, the map uploaded).  B = the in-lane
            adaptive call's total samples minus the pilot's.  Wall time of the whole leg (host clock around it, the device idle
            before and after) and the kernel time of its calls.
  quality   RMSE over rgb against a PIXEL render at --ref-spp on another seed: render_converge_device under a total budget of the
            adaptive call's samples (--passes passes), the in-lane adaptive call itself, the uniform frame of equal total (the same
            mean count, rounded up), the two-pass frames of the part above (device map and host map, both continued accumulation)
            and, for the host map, the r23 scheme: the second pass as an independent estimate on another seed, blended by counts.
One JSON line per scene.  Nothing is required of the numbers: the line records.
usage: python3 tools/plan_bench.py [--scenes c3_bunny_room,c2_analytic] [--width 1920] [--height 1080] [--pilot 128]
           [--max-spp 1024] [--tolerance 0.3] [--passes 4] [--ref-spp 16384] [--parts time,two_pass,quality]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOOR = 0.05


def luminance(rgb):
    return (np.float32(0.2126) * rgb[..., 0] + np.float32(0.7152) * rgb[..., 1]) + np.float32(0.0722) * rgb[..., 2]


def max3x3(a):
    p = np.pad(a, 1, mode="edge")
    h, w = a.shape
    return np.max(np.stack([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)]), axis=0)


def host_map(h_sum, h_q, n1, budget):
    """tools/sample_map_bench.py's map (lines 190-204 there), from the pilot's planes"""
    with np.errstate(all="ignore"):
        m = luminance(h_sum / np.float32(n1)).astype(np.float64)
        var = np.maximum(h_q.astype(np.float64) / n1 - m * m, 0.0)
        rel = np.sqrt(var / (n1 - 1)) / np.maximum(np.abs(m), FLOOR)
    rel = np.where(np.isfinite(rel), rel, 0.0)
    wgt = max3x3(rel) ** 2
    n2 = np.floor(budget * wgt / wgt.sum()).astype(np.int64)
    return np.minimum(n2, 1 << 24).astype("<u4")


def spread(v):
    med = float(np.median(v))
    return {"median": med, "s": (max(v) - min(v)) / med if med else 0.0, "all": [round(x, 4) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c3_bunny_room,c2_analytic")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--pilot", type=int, default=128)
    ap.add_argument("--max-spp", type=int, default=1024)
    ap.add_argument("--tolerance", type=float, default=0.3)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--ref-spp", type=int, default=16384)
    ap.add_argument("--parts", default="time,two_pass,quality")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--pass-calls", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    a = ap.parse_args()
    assert a.calls >= 5 and a.warmup >= 2 and a.pass_calls >= 3
    parts = a.parts.split(",")
    import torch
    from offline_raytracer_amd import api
    if api.device_count() < 1:
        raise SystemExit("plan_bench: no HIP device; nothing here is measured without one")
    dev = torch.device("cuda", 0)
    W, H, n, N1 = a.width, a.height, a.width * a.height, a.pilot
    ws_bytes = api.plan_workspace_bytes(W, H)
    for name in a.scenes.split(","):
        scene = api.Scene.load_scn(os.path.join(ROOT, "data", name + ".scn")).commit().upload(0)
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        d_sum, d_m2, d_count, d_states, d_map = f32(H, W, 3), f32(H, W), i32(H, W), i32(H, W), i32(H, W)
        rgb, spp_plane, q_plane = f32(H, W, 3), i32(H, W), f32(H, W)
        d_totals = torch.zeros(4, dtype=torch.int64, device=dev)
        ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
        c0, c1 = (torch.zeros(18 * n, dtype=torch.uint8, device=dev) for _ in range(2))
        torch.cuda.synchronize(dev)
        plan_kw = dict(floor=FLOOR, radius=1, pilot=N1, min_add=1, cap=a.max_spp, rgb_is_sum=True)

        def fresh():
            for t in (d_sum, d_m2, d_count, d_states):
                t.zero_()

        def accumulate(cap, d_map_ptr=0, seed=a.seed):
            return scene.render_accumulate_device(scene.params(W, H, cap, seed, "pixel"), d_sum.data_ptr(), d_count.data_ptr(), d_states.data_ptr(), d_m2.data_ptr(),
                                                  d_map_ptr, want_stats=True)["kernel_ms"]

        def plan(**kw):
            return api.plan_samples_device(d_sum.data_ptr(), d_m2.data_ptr(), d_count.data_ptr(), W, H, d_map.data_ptr(), d_totals.data_ptr(), ws.data_ptr(), ws_bytes,
                                           a.tolerance, want_stats=True, **dict(plan_kw, **kw))["kernel_ms"]

        def totals():
            return api._totals_dicts(np.frombuffer(d_totals.cpu().numpy().tobytes(), api.PLAN_TOTALS_DTYPE))[0]

        def copy():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c1.copy_(c0)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        def frame():
            return d_sum / d_count.to(torch.float32).clamp(min=1).unsqueeze(-1)

        line = {"tool": "plan_bench", "scene": name, "width": W, "height": H, "pilot": N1, "tolerance": a.tolerance, "floor": FLOOR, "cap": a.max_spp,
                "lib": os.path.relpath(api.LIB_PATH, ROOT)}
        fresh()
        pilot_ms = accumulate(N1)
        plan()
        t_pilot = totals()
        line["after_pilot"] = {k: (float(v) if k == "worst" else v) for k, v in t_pilot.items()}
        if "time" in parts:
            half = max(t_pilot["wanted"] // 2, 1)
            def forced(value, f):
                os.environ["ORT_PLAN_TILE"] = value
                try:
                    return f()
                finally:
                    del os.environ["ORT_PLAN_TILE"]
            legs = [("copy", copy)] + [("radius_%d" % r, (lambda r=r: plan(radius=r))) for r in range(4)] + \
                   [("radius_%d_direct" % r, (lambda r=r: forced("0", lambda: plan(radius=r)))) for r in range(4)] + \
                   [("radius_%d_tile" % r, (lambda r=r: forced("1", lambda: plan(radius=r)))) for r in range(4)] + \
                   [("radius_%d_scaled" % r, (lambda r=r: plan(radius=r, budget=half))) for r in range(4)]
            ms = {k: [] for k, _ in legs}
            for r in range(a.warmup + a.calls):
                for k, f in legs:
                    t = f()
                    if r >= a.warmup:
                        ms[k].append(t)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            line["time"] = {"warmup": a.warmup, "calls": a.calls, "median_ms": med, "s": {k: (max(v) - min(v)) / med[k] for k, v in ms.items()},
                            "ratio_plan_over_copy": {k: med[k] / med["copy"] for k in med if k != "copy"},
                            "ratio_range_radius_1": [min(ms["radius_1"]) / max(ms["copy"]), max(ms["radius_1"]) / min(ms["copy"])],
                            "copy_gb_per_s": 36 * n / (med["copy"] * 1e-3) / 1e9, "plan_gb_per_s_radius_1": 36 * n / (med["radius_1"] * 1e-3) / 1e9,
                            "kernel_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}}
        if "two_pass" in parts or "quality" in parts:
            ad_ms = scene.render_adaptive_device(scene.params(W, H, 0, a.seed, "pixel"), N1, a.max_spp, a.tolerance, FLOOR, N1, rgb.data_ptr(), spp_plane.data_ptr(),
                                                 q_plane.data_ptr(), want_stats=True)["kernel_ms"]
            taken = int(spp_plane.long().sum())
            ad_frame = rgb.clone()
            B = taken - N1 * n
            line["adaptive"] = {"min_spp": N1, "max_spp": a.max_spp, "check_every": N1, "samples": taken, "kernel_ms": ad_ms, "second_pass_budget": B}
        frames = {}
        if ("two_pass" in parts or "quality" in parts) and B > 0:
            def device_leg():
                fresh()
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                k = accumulate(N1)
                k += plan(budget=B)
                t = totals()
                k += accumulate(a.max_spp, d_map.data_ptr())
                torch.cuda.synchronize(dev)
                return (time.perf_counter() - t0) * 1e3, k, t["planned"]

            def host_leg():
                fresh()
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                k = accumulate(N1)
                n2 = host_map(d_sum.cpu().numpy(), d_m2.cpu().numpy(), N1, B)
                d_map.copy_(torch.from_numpy(n2.view("<i4")))
                k += accumulate(int(max(int(n2.max()), 1)), d_map.data_ptr())
                torch.cuda.synchronize(dev)
                return (time.perf_counter() - t0) * 1e3, k, int(n2.astype(np.int64).sum())
            res = {"device_map": [], "host_map": []}
            for r in range(1 + a.pass_calls):
                for k, f in (("device_map", device_leg), ("host_map", host_leg)):
                    out = f()
                    if r >= 1:
                        res[k].append(out)
                    if r == 0:
                        frames["two_pass_" + k] = frame().clone()
                        if k == "host_map":
                            host_n2 = d_map.clone()
            line["two_pass"] = {k: {"wall_ms": spread([x[0] for x in v]), "kernel_ms": spread([x[1] for x in v]), "second_pass_samples": v[0][2],
                                    "total_samples": v[0][2] + N1 * n} for k, v in res.items()}
            line["two_pass"]["pilot_kernel_ms"] = pilot_ms
        if "quality" in parts:
            ref = f32(H, W, 3)
            scene.render_device(ref.data_ptr(), scene.params(W, H, a.ref_spp, a.seed + 1, "pixel"), want_stats=True)
            rmse = lambda x: float(((x.double() - ref.double()) ** 2).mean().sqrt())
            q = {"ref_spp": a.ref_spp, "rmse_adaptive": rmse(ad_frame), "adaptive_samples": taken}
            for k, f in frames.items():
                q["rmse_" + k] = rmse(f)
            mean = -(-taken // n)
            scene.render_device(rgb.data_ptr(), scene.params(W, H, mean, a.seed, "pixel"), want_stats=True)
            q.update({"uniform_spp": mean, "rmse_uniform_same_total": rmse(rgb)})
            if frames:   # r23's scheme with the host map: an independent second estimate on another seed, blended by counts
                fresh()
                accumulate(N1)
                pilot = frame().clone()
                cap = int(max(int(host_n2.max()), 1))
                scene.render_sample_map_device(scene.params(W, H, cap, a.seed + 7, "pixel"), host_n2.data_ptr(), rgb.data_ptr(), want_stats=True)
                f2 = host_n2.to(torch.float32).unsqueeze(-1)
                q["rmse_two_pass_host_map_blended"] = rmse(torch.where(f2 > 0, (N1 * pilot + f2 * rgb) / (N1 + f2), pilot))
                q["rmse_pilot_alone"] = rmse(pilot)
            fresh()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            # the budget of the loop is per frame: the adaptive call's total
            history = scene.render_converge_device(W, H, d_sum, d_m2, d_count, d_states, d_map, d_totals, ws, a.tolerance, a.seed, passes=a.passes, budget=taken,
                                                   pilot=N1, cap=a.max_spp, floor=FLOOR, radius=1, min_add=1)
            torch.cuda.synchronize(dev)
            q["converge"] = {"passes": a.passes, "budget": taken, "wall_ms": (time.perf_counter() - t0) * 1e3, "samples": int(d_count.long().sum()),
                             "rmse": rmse(frame()), "history": [{k: (float(v) if k == "worst" else v) for k, v in t.items()} for t in history]}
            line["quality"] = q
            del ref
        print(json.dumps(line), flush=True)
        scene.close()
        del d_sum, d_m2, d_count, d_states, d_map, rgb, spp_plane, q_plane, ws, c0, c1, frames
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
