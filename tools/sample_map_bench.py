"""Overhead, the fed-back map, sparse maps and a two-pass scheme of the sample-map render (ort_render_sample_map_device; kernels
pt_sample_map) against ort_render_image_device at the PIXEL policy and ort_render_adaptive_device, same process, one GPU.

Per scene, a --width x --height frame from the scene's own camera, four parts in one run.  Every timing is kernel_ms of a call (one
pair of HIP events around the launch); every leg runs --warmup rounds and then --calls timed rounds, the legs of a part alternating
within a round; a leg reports its median and s = (max - min) / median of its own timings.
  overhead  a constant map at --spp (cap --spp) against the PIXEL render at spp = --spp, as the launch policy runs it ("uniform") and
            held to the same plain loop ("uniform_plain": ORT_EXCHANGE=0 ORT_WAVES5=0), and against the adaptive call with
            min_spp == max_spp == --spp (pt_adaptive; no check ever runs).  The four frames are compared bit for bit first.
  fed_back  the adaptive call with checks firing (min_spp --min-spp, a check every --min-spp, max_spp --max-spp, tolerance
            --tolerance, floor 0.05) against the sample-map call fed that call's out_spp, same seed, cap --max-spp; the three
            planes are compared bit for bit first.
  sparse    maps that are --spp on 1 % and on 10 % of the pixels and 0 elsewhere, once scattered (pixels drawn at random) and once
            as one compact rectangle in the frame's middle, and the all-zero map: kernel time, and time per rendered sample
            against the dense constant map's.  The all-zero map's time over the pixel count is what an empty job costs.
  two_pass  a pilot of --min-spp samples a pixel (the adaptive call at min_spp == max_spp, for its out_m2); on the HOST the relative
            standard error of every pixel's mean luminance (floor 0.05 under the mean, as the stopping rule), its 3 x 3 maximum
            r, and a map n2 = floor(B r^2 / sum r^2) with B = the fed_back adaptive run's total samples minus the pilot's; a second
            pass with that map on another seed; the two passes combined by their counts.  RMSE over rgb against a PIXEL render
            at --ref-spp on a third seed: the combined frame, the adaptive call's frame and the uniform frame of equal total
            (the same mean count, rounded up).
One JSON line per scene.  Nothing is required of the numbers: the line records.
usage: python3 tools/sample_map_bench.py [--scenes c3_bunny_room,c2_analytic] [--width 1920] [--height 1080] [--spp 256]
           [--min-spp 128] [--max-spp 1024] [--tolerance 0.3] [--ref-spp 16384]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["ORT_KNOBS_LIVE"] = "1"   # the uniform legs differ in knobs: read them at every call

PLAIN = {"ORT_EXCHANGE": "0", "ORT_WAVES5": "0"}
FLOOR = 0.05


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


def rounds(legs, warmup, calls, after_first=None):
    """legs: (name, env, f -> kernel ms) -> {name: [ms of the timed rounds]}; after_first(name) runs once per leg, in round 0"""
    ms = {k: [] for k, _, _ in legs}
    for r in range(warmup + calls):
        for k, env, f in legs:
            t = with_env(env, f)
            if r >= warmup:
                ms[k].append(t)
            if r == 0 and after_first:
                after_first(k)
    return ms


def summary(ms):
    return {k: {"median_ms": float(np.median(v)), "s": (max(v) - min(v)) / float(np.median(v)), "all_ms": [round(x, 4) for x in v]} for k, v in ms.items()}


def luminance(rgb):
    return (np.float32(0.2126) * rgb[..., 0] + np.float32(0.7152) * rgb[..., 1]) + np.float32(0.0722) * rgb[..., 2]


def max3x3(a):
    p = np.pad(a, 1, mode="edge")
    h, w = a.shape
    return np.max(np.stack([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)]), axis=0)


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
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2024)
    a = ap.parse_args()
    assert a.calls >= 3 and a.warmup >= 1
    import torch
    from offline_raytracer_amd import api
    dev = torch.device("cuda", 0)
    W, H, n = a.width, a.height, a.width * a.height
    for name in a.scenes.split(","):
        scene = api.Scene.load_scn(os.path.join(ROOT, "data", name + ".scn")).commit().upload(0)
        rgb = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        spp = torch.zeros((H, W), dtype=torch.int32, device=dev)
        m2 = torch.zeros((H, W), dtype=torch.float32, device=dev)
        states = torch.zeros((H, W), dtype=torch.int32, device=dev)
        smap = torch.zeros((H, W), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)

        def uniform(k, seed=a.seed):
            return scene.render_device(rgb.data_ptr(), scene.params(W, H, k, seed, "pixel"), want_stats=True)["kernel_ms"]

        def adaptive(lo, hi, every, seed=a.seed):
            return scene.render_adaptive_device(scene.params(W, H, 0, seed, "pixel"), lo, hi, a.tolerance, FLOOR, every, rgb.data_ptr(), spp.data_ptr(),
                                                m2.data_ptr(), states.data_ptr(), want_stats=True)["kernel_ms"]

        def mapped(cap, seed=a.seed, d_map=None):
            return scene.render_sample_map_device(scene.params(W, H, cap, seed, "pixel"), (smap if d_map is None else d_map).data_ptr(), rgb.data_ptr(),
                                                  m2.data_ptr(), states.data_ptr(), want_stats=True)["kernel_ms"]
        out = {"tool": "sample_map_bench", "scene": name, "width": W, "height": H, "warmup": a.warmup, "calls": a.calls,
               "lib": os.path.relpath(api.LIB_PATH, ROOT)}
        # ---- overhead: a constant map ----
        smap.fill_(a.spp)
        frames = {}
        ms = rounds((("uniform", {}, lambda: uniform(a.spp)), ("uniform_plain", PLAIN, lambda: uniform(a.spp)),
                     ("adaptive_fixed", {}, lambda: adaptive(a.spp, a.spp, 1)), ("sample_map", {}, lambda: mapped(a.spp))),
                    a.warmup, a.calls, lambda k: frames.__setitem__(k, rgb.clone()))
        same = all(bool(torch.equal(frames["sample_map"].view(torch.int32), f.view(torch.int32))) for f in frames.values())
        del frames
        legs = summary(ms)
        dense_ms = legs["sample_map"]["median_ms"]
        out["overhead"] = {"spp": a.spp, "frames_identical": same, "legs": legs,
                           "mpaths_per_s": {k: n * a.spp / (v["median_ms"] * 1e-3) / 1e6 for k, v in legs.items()},
                           "sample_map_over": {k: dense_ms / v["median_ms"] for k, v in legs.items() if k != "sample_map"}}
        # ---- the adaptive call's counts fed back ----
        adaptive(a.min_spp, a.max_spp, a.min_spp)
        want = [x.clone() for x in (rgb, m2, states)]
        counts = spp.clone()
        taken = int(counts.long().sum())
        mapped(a.max_spp, d_map=counts)
        same = all(bool(torch.equal(x.view(torch.int32), y.view(torch.int32))) for x, y in zip(want, (rgb, m2, states)))
        ad_frame = want[0]
        del want
        ms = rounds((("adaptive", {}, lambda: adaptive(a.min_spp, a.max_spp, a.min_spp)), ("sample_map", {}, lambda: mapped(a.max_spp, d_map=counts))),
                    a.warmup, a.calls)
        legs = summary(ms)
        out["fed_back"] = {"min_spp": a.min_spp, "max_spp": a.max_spp, "check_every": a.min_spp, "tolerance": a.tolerance, "floor": FLOOR,
                           "planes_identical": same, "samples_taken": taken, "fraction_of_samples": taken / (n * a.max_spp), "legs": legs,
                           "sample_map_over_adaptive": legs["sample_map"]["median_ms"] / legs["adaptive"]["median_ms"]}
        # ---- sparse maps ----
        gen = torch.Generator(device="cpu").manual_seed(a.seed)
        maps = {"zero": torch.zeros((H, W), dtype=torch.int32)}
        for share in (0.01, 0.10):
            k = int(round(n * share))
            scattered = torch.zeros(n, dtype=torch.int32)
            scattered[torch.randperm(n, generator=gen)[:k]] = a.spp
            maps["scattered_%g" % share] = scattered.reshape(H, W)
            h = max(1, int(round((k * H / W) ** 0.5)))   # a rectangle of the frame's proportions
            w = max(1, int(round(k / h)))
            compact = torch.zeros((H, W), dtype=torch.int32)
            compact[(H - h) // 2:(H - h) // 2 + h, (W - w) // 2:(W - w) // 2 + w] = a.spp
            maps["compact_%g" % share] = compact
        maps = {k: v.to(dev) for k, v in maps.items()}
        ms = rounds(tuple((k, {}, (lambda m: lambda: mapped(a.spp, d_map=m))(v)) for k, v in maps.items()), a.warmup, a.calls)
        legs = summary(ms)
        dense_ns = dense_ms * 1e6 / (n * a.spp)
        out["sparse"] = {"spp": a.spp, "dense_ns_per_sample": dense_ns, "maps": {}}
        for k, v in legs.items():
            samples = int(maps[k].long().sum())
            v.update({"pixels": int((maps[k] != 0).sum()), "samples": samples})
            if samples:
                v["ns_per_sample"] = v["median_ms"] * 1e6 / samples
                v["per_sample_over_dense"] = v["ns_per_sample"] / dense_ns
            else:
                v["ns_per_empty_job"] = v["median_ms"] * 1e6 / n
            out["sparse"]["maps"][k] = v
        del maps
        # ---- two passes: a pilot, a host-built map, a second pass on another seed ----
        uniform(a.ref_spp, a.seed + 1)
        ref = rgb.clone()

        def rmse(x):
            return float(((x.double() - ref.double()) ** 2).mean().sqrt())
        e_ad = rmse(ad_frame)
        mean = -(-taken // n)
        N1 = a.min_spp
        ms = rounds((("uniform_mean_spp", {}, lambda: uniform(mean)), ("pilot", {}, lambda: adaptive(N1, N1, 1))), a.warmup, a.calls)
        uniform(mean)
        e_mean = rmse(rgb)
        adaptive(N1, N1, 1)
        pilot = rgb.clone()
        h_rgb, h_q = pilot.cpu().numpy(), m2.cpu().numpy()
        with np.errstate(all="ignore"):
            m = luminance(h_rgb).astype(np.float64)
            var = np.maximum(h_q.astype(np.float64) / N1 - m * m, 0.0)
            rel = np.sqrt(var / (N1 - 1)) / np.maximum(np.abs(m), FLOOR)
        rel = np.where(np.isfinite(rel), rel, 0.0)
        r = max3x3(rel)
        budget = taken - N1 * n
        two = {"pilot_spp": N1, "budget_second_pass": budget}
        if budget > 0 and (r > 0).any():
            wgt = r * r
            n2 = np.floor(budget * wgt / wgt.sum()).astype(np.int64)
            cap = int(min(max(int(n2.max()), 1), 1 << 24))
            n2 = np.minimum(n2, cap).astype("<u4")
            d_n2 = torch.from_numpy(n2.view("<i4")).to(dev)
            ms.update(rounds((("second_pass", {}, lambda: mapped(cap, seed=a.seed + 7, d_map=d_n2)),), a.warmup, a.calls))
            f2 = d_n2.to(torch.float32).unsqueeze(-1)
            combined = torch.where(f2 > 0, (N1 * pilot + f2 * rgb) / (N1 + f2), pilot)
            two.update({"second_pass_samples": int(n2.astype(np.int64).sum()), "second_pass_pixels": int((n2 != 0).sum()), "second_pass_max": int(n2.max()),
                        "total_samples": int(n2.astype(np.int64).sum()) + N1 * n,
                        "rmse_two_pass": rmse(combined), "rmse_pilot_alone": rmse(pilot)})
            del combined, d_n2
        two.update({"ref_spp": a.ref_spp, "adaptive_total_samples": taken, "rmse_adaptive": e_ad, "uniform_mean_spp": mean,
                    "rmse_uniform_same_total": e_mean, "legs": dict(summary(ms), adaptive=out["fed_back"]["legs"]["adaptive"])})
        out["two_pass"] = two
        print(json.dumps(out), flush=True)
        scene.close()
        del rgb, spp, m2, states, smap, ref, pilot, ad_frame, counts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
