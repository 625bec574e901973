"""Overhead and payoff of the light-group render (ort_render_light_groups_device; kernels pt_groups) against
ort_render_image_device at the PIXEL policy, same process, one GPU.

Per scene (c2_analytic, testscene, c4_dwarf_room by default), a --width x --height frame from the scene's own camera at --spp,
one group per light material (G = the scene's light materials), the unsplit frame asked for as well:
  overhead  the call's kernel time against the PIXEL render of the same frame, as the launch policy runs that ("pixel": ray
            exchange and five-waves unit allowed) and held to the same plain loop ("pixel_plain": ORT_EXCHANGE=0 ORT_WAVES5=0).
            --warmup rounds, then --calls timed rounds, the legs alternating within a round; kernel_ms of each call (one pair
            of HIP events around the launch).  ratio = groups / pixel from the medians, with the spread s = (max - min) / median
            of each leg: a ratio within s of 1 is inside the noise.
  route     the route the call replaces: G PIXEL renders.  A scene cannot be re-lit in place, so the G renders are of the scene
            itself (the dark twins trace the same paths: same cost); "g_renders" is the sum of G calls' kernel_ms, per round.
            speedup = g_renders / groups.
  bytes     of planes the call writes: (G + 1) x width x height x 12; the G sums are read and written in place per emission.
The frames are checked first: the unsplit frame bit for bit the PIXEL render's, and the G frames adding up to it to rounding.
One JSON line per scene.  Nothing is required of the numbers: the line records.
usage: python3 tools/light_groups_bench.py [--scenes c2_analytic,testscene,c4_dwarf_room] [--width 1920] [--height 1080] [--spp 256]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["ORT_KNOBS_LIVE"] = "1"   # the pixel legs differ in knobs: read them at every call

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
    ap.add_argument("--scenes", default="c2_analytic,testscene,c4_dwarf_room")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2024)
    a = ap.parse_args()
    assert a.calls >= 5 and a.warmup >= 2
    import torch
    from offline_raytracer_amd import api
    dev = torch.device("cuda", 0)
    W, H, n = a.width, a.height, a.width * a.height
    for name in a.scenes.split(","):
        scene = api.Scene.load_scn(os.path.join(ROOT, "data", name + ".scn")).commit().upload(0)
        lights = scene.light_materials()
        G = len(lights)
        groups = {m: g for g, m in enumerate(lights)}
        frames = torch.zeros((G, H, W, 3), dtype=torch.float32, device=dev)
        rgb = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        ref = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        p = scene.params(W, H, a.spp, a.seed, "pixel")

        def split():
            return scene.render_light_groups_device(p, groups, frames.data_ptr(), rgb.data_ptr(), want_stats=True)["kernel_ms"]

        def pixel():
            return scene.render_device(ref.data_ptr(), p, want_stats=True)["kernel_ms"]

        def g_renders():
            return sum(pixel() for _ in range(G))
        legs = (("groups", {}, split), ("pixel", {}, pixel), ("pixel_plain", PLAIN, pixel), ("g_renders", {}, g_renders))
        ms = {k: [] for k, _, _ in legs}
        for r in range(a.warmup + a.calls):
            for k, env, f in legs:
                t = with_env(env, f)
                if r >= a.warmup:
                    ms[k].append(t)
        same = bool(torch.equal(rgb.view(torch.int32), ref.view(torch.int32)))
        total = frames.sum(dim=0)
        scale = float(ref.abs().max())
        sum_err = float((total - ref).abs().max())
        med = {k: float(np.median(v)) for k, v in ms.items()}
        s = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
        out = {"tool": "light_groups_bench", "scene": name, "width": W, "height": H, "spp": a.spp, "groups": G, "light_materials": lights,
               "warmup": a.warmup, "calls": a.calls, "rgb_is_the_pixel_render": same, "sum_of_groups_max_abs_diff": sum_err, "frame_max": scale,
               "lit_share_per_group": [float((frames[g] != 0).any(dim=2).double().mean()) for g in range(G)],
               "overhead": {"ratio": med["groups"] / med["pixel"], "ratio_plain": med["groups"] / med["pixel_plain"]},
               "route": {"speedup": med["g_renders"] / med["groups"]},
               "median_ms": med, "s": s, "mpaths_per_s": {k: n * a.spp * (G if k == "g_renders" else 1) / (v * 1e-3) / 1e6 for k, v in med.items()},
               "bytes_of_planes": int((G + 1) * n * 12),
               "kernel_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "lib": os.path.relpath(api.LIB_PATH, ROOT)}
        print(json.dumps(out), flush=True)
        scene.close()
        del frames, rgb, ref, total
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
