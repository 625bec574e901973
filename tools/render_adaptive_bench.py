"""Overhead, payoff, error and the views form of the adaptive camera render (ort_render_adaptive_device,
ort_render_views_adaptive_device; kernels pt_adaptive) against ort_render_image_device at the PIXEL policy, same process, one GPU.

Per scene, a --width x --height frame from the scene's own camera, four parts in one run:
  overhead  the adaptive call with min_spp == max_spp == --spp (no check ever runs) against the PIXEL render at spp = --spp, as
            the launch policy runs it ("uniform": ray exchange and five-waves unit allowed) and held to the same plain loop
            ("uniform_plain": ORT_EXCHANGE=0 ORT_WAVES5=0).  --warmup rounds, then --calls timed rounds, the three alternating
            within a round; kernel_ms of each call (one pair of HIP events around the launch).  ratio = uniform / adaptive from
            the medians, s = (max - min) / median of the uniform render's own timings: a ratio within 1 - s of 1 is inside the
            yardstick's noise.
  payoff    with checks firing (min_spp --min-spp, a check every --min-spp, max_spp --max-spp, tolerance --tolerance, floor
            0.05: the tests' FRAME set scaled): the samples taken as a share of pixels x max_spp; the kernel time as a share of
            the uniform render's at max_spp, and against a uniform render at the mean sample count (rounded up).
  error     RMSE over rgb against a PIXEL render at --ref-spp on another seed: the adaptive frame, the uniform frame of equal
            total samples (the same mean count, rounded up), the uniform frame at max_spp.  Pixels that stopped black at
            min_spp are counted: the rule's known weakness is part of the figure.
  views     one batch of --views views of --view-size x --view-size (the scene's pose moved toward the scene's centre and yawed,
            a seed each) against its views one call each (one-view batches: the single-frame call knows the scene's own camera only):
            host time from before the first call to after one final
            synchronise, alternating, median of --calls; the planes are compared bit for bit first.
One JSON line per scene.  Nothing is required of the numbers: the line records.
usage: python3 tools/render_adaptive_bench.py [--scenes c3_bunny_room,c2_analytic] [--width 1920] [--height 1080] [--spp 256]
           [--min-spp 128] [--max-spp 1024] [--tolerance 0.3] [--ref-spp 16384] [--views 8] [--view-size 256]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["ORT_KNOBS_LIVE"] = "1"   # the uniform legs differ in knobs: read them at every call

PLAIN = {"ORT_EXCHANGE": "0", "ORT_WAVES5": "0"}


def with_env(env, f):
    old = {k: os.environ.get(k) for k in PLAIN}
    for k in PLAIN:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return f()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c3_bunny_room,c2_analytic")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--min-spp", type=int, default=128)
    ap.add_argument("--max-spp", type=int, default=1024)
    ap.add_argument("--tolerance", type=float, default=0.3)
    ap.add_argument("--ref-spp", type=int, default=16384)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--view-size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2024)
    a = ap.parse_args()
    assert a.calls >= 5 and a.warmup >= 2
    import torch
    from offline_raytracer_amd import api
    import views_cases
    dev = torch.device("cuda", 0)
    W, H, n = a.width, a.height, a.width * a.height
    FLOOR = 0.05
    for name in a.scenes.split(","):
        scene = api.Scene.load_scn(os.path.join(ROOT, "data", name + ".scn")).commit().upload(0)
        rgb = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        spp = torch.zeros((H, W), dtype=torch.int32, device=dev)
        m2 = torch.zeros((H, W), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)

        def uniform(k, seed=a.seed):
            return scene.render_device(rgb.data_ptr(), scene.params(W, H, k, seed, "pixel"), want_stats=True)["kernel_ms"]

        def adaptive(lo, hi, every, tol=a.tolerance):
            return scene.render_adaptive_device(scene.params(W, H, 0, a.seed, "pixel"), lo, hi, tol, FLOOR, every, rgb.data_ptr(), spp.data_ptr(),
                                                m2.data_ptr(), want_stats=True)["kernel_ms"]
        # ---- overhead: no check ever runs ----
        legs = (("uniform", {}, lambda: uniform(a.spp)), ("uniform_plain", PLAIN, lambda: uniform(a.spp)),
                ("adaptive", {}, lambda: adaptive(a.spp, a.spp, 1)))
        ms = {k: [] for k, _, _ in legs}
        frames = {}
        for r in range(a.warmup + a.calls):
            for k, env, f in legs:
                t = with_env(env, f)
                if r >= a.warmup:
                    ms[k].append(t)
                if r == 0:
                    frames[k] = rgb.clone()
        same = bool(torch.equal(frames["uniform"].view(torch.int32), frames["adaptive"].view(torch.int32)) and
                    torch.equal(frames["uniform_plain"].view(torch.int32), frames["adaptive"].view(torch.int32)))
        del frames
        med = {k: float(np.median(v)) for k, v in ms.items()}
        out = {"tool": "render_adaptive_bench", "scene": name, "width": W, "height": H, "warmup": a.warmup, "calls": a.calls,
               "overhead": {"spp": a.spp, "frames_identical": same,
                            "mpaths_per_s": {k: n * a.spp / (v * 1e-3) / 1e6 for k, v in med.items()},
                            "ratio": med["uniform"] / med["adaptive"], "ratio_plain": med["uniform_plain"] / med["adaptive"],
                            "s": (max(ms["uniform"]) - min(ms["uniform"])) / med["uniform"],
                            "s_plain": (max(ms["uniform_plain"]) - min(ms["uniform_plain"])) / med["uniform_plain"],
                            "s_adaptive": (max(ms["adaptive"]) - min(ms["adaptive"])) / med["adaptive"],
                            "kernel_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}},
               "lib": os.path.relpath(api.LIB_PATH, ROOT)}
        # ---- payoff and error ----
        uniform(a.ref_spp, a.seed + 1)
        ref = rgb.clone()

        def rmse():
            return float(((rgb.double() - ref.double()) ** 2).mean().sqrt())
        adaptive(a.min_spp, a.max_spp, a.min_spp)   # warm
        t_ad = [adaptive(a.min_spp, a.max_spp, a.min_spp) for _ in range(3)]
        e_ad = rmse()
        taken = int(spp.long().sum())
        black_at_min = int(((spp == a.min_spp) & (rgb == 0).all(dim=2)).sum())
        mean = -(-taken // n)   # the uniform render with the same total, rounded up per pixel
        t_full = [uniform(a.max_spp) for _ in range(3)]
        e_full = rmse()
        t_mean = [uniform(mean) for _ in range(3)]
        e_mean = rmse()
        out["payoff"] = {"min_spp": a.min_spp, "max_spp": a.max_spp, "check_every": a.min_spp, "tolerance": a.tolerance, "floor": FLOOR,
                         "samples_taken": taken, "samples_uniform": n * a.max_spp, "fraction_of_samples": taken / (n * a.max_spp),
                         "pixels_at_min_spp": int((spp == a.min_spp).sum()), "pixels_at_max_spp": int((spp == a.max_spp).sum()),
                         "pixels_black_at_min_spp": black_at_min,
                         "kernel_ms_adaptive": float(np.median(t_ad)), "kernel_ms_uniform_max_spp": float(np.median(t_full)),
                         "fraction_of_time": float(np.median(t_ad) / np.median(t_full)),
                         "uniform_mean_spp": mean, "kernel_ms_uniform_mean_spp": float(np.median(t_mean)),
                         "time_against_uniform_mean_spp": float(np.median(t_ad) / np.median(t_mean)),
                         "kernel_ms_all": {"adaptive": t_ad, "uniform_max_spp": t_full, "uniform_mean_spp": t_mean}}
        out["error"] = {"ref_spp": a.ref_spp, "rmse_adaptive": e_ad, "rmse_uniform_same_total": e_mean, "rmse_uniform_max_spp": e_full}
        del ref
        # ---- the views form ----
        V, S = a.views, a.view_size
        si = scene.info()
        p0 = np.array([si.camera_p.x, si.camera_p.y, si.camera_p.z], "<f4")
        q0 = np.array(list(si.camera_quat_xyzw), dtype=np.float64)
        lo, hi = views_cases.scene_box(scene.flatten(S, S))
        centre = (lo.astype(np.float64) + hi) / 2
        cams = []
        for v in range(V):
            f, yaw = 0.5 * v / max(V - 1, 1), np.radians(-40.0 + 80.0 * v / max(V - 1, 1)) / 2
            q = views_cases.quat_mul(np.array([0.0, 0.0, np.sin(yaw), np.cos(yaw)]), q0).astype("<f4")
            cams.append(api.camera_from_pose((p0 + f * (centre - p0)).astype("<f4"), q, si.camera_height_ratio, S, S))
        cams = np.stack(cams)
        seeds = [a.seed + v for v in range(V)]
        pb = [torch.zeros((V, S, S, k), dtype=t, device=dev) for k, t in ((3, torch.float32), (1, torch.int32), (1, torch.float32))]
        ps = [torch.zeros_like(x) for x in pb]
        pv = scene.params(S, S, 0, 0, "pixel")
        rule = (a.min_spp, a.max_spp, a.tolerance, FLOOR, a.min_spp)

        def batch():
            scene.render_views_adaptive_device(pv, cams, seeds, *rule, *[x.data_ptr() for x in pb])

        def sequence():
            for v in range(V):
                # the single-frame call renders the scene's own camera: a view of its own goes through a one-view batch
                scene.render_views_adaptive_device(pv, cams[v:v + 1], seeds[v:v + 1], *rule, *[x[v].data_ptr() for x in ps])

        def timed(f):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        tv = {"batch": [], "sequence": []}
        for r in range(a.warmup + a.calls):
            for k, f in (("batch", batch), ("sequence", sequence)):
                t = timed(f)
                if r >= a.warmup:
                    tv[k].append(t)
        same = all(bool(torch.equal(x.view(torch.int32), y.view(torch.int32))) for x, y in zip(pb, ps))
        mb, msq = float(np.median(tv["batch"])), float(np.median(tv["sequence"]))
        out["views"] = {"views": V, "size": S, "planes_identical": same, "samples_taken": int(pb[1].long().sum()), "batch_ms": mb, "sequence_ms": msq,
                        "speedup": msq / mb, "s": (max(tv["sequence"]) - min(tv["sequence"])) / msq,
                        "batch_all_ms": [round(x, 3) for x in tv["batch"]], "sequence_all_ms": [round(x, 3) for x in tv["sequence"]]}
        print(json.dumps(out), flush=True)
        scene.close()
        del rgb, spp, m2, pb, ps
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
