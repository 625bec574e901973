"""Overhead of the path-depth render (ort_render_depths_device; kernels pt_depths) against the light-group render
(ort_render_light_groups_device; pt_groups), whose machinery it shares, and against ort_render_image_device at the PIXEL policy,
same process, one GPU.

Per scene (c2_analytic, testscene, c4_dwarf_room by default), a --width x --height frame from the scene's own camera at --spp, the
unsplit frame asked for as well.  --warmup rounds, then --calls timed rounds, the legs alternating within a round; kernel_ms of
each call (one pair of HIP events around the launch):
  depths3, depths8          the call at G = 3 and G = 8, without out_lengths: the depth word in LDS and the bin sums alone
  depths3_len, depths8_len  the same with out_lengths: one more read-modify-write of a word per sample
  groups                    ort_render_light_groups, one group per light material: the comparator
  pixel_plain, pixel        the PIXEL render held to the plain four-waves loop (ORT_EXCHANGE=0 ORT_WAVES5=0), and as the launch
                            policy runs it
Every ratio is a quotient of medians and stands beside the comparator's own spread s = (max - min) / median: a ratio within s
of 1 is inside the noise.  depths*_len / depths* is what the length words cost; depths* / groups what the counter and the bin
choice cost.
The frames are checked first: the unsplit frame bit for bit the PIXEL render's, the bins adding up to it to rounding, the
lengths adding up to spp.  energy_share_per_bin: the share of the frame's summed luminance that each of the 8 bins carries.
One JSON line per scene.  Nothing is required of the numbers: the line records.
usage: python3 tools/depths_bench.py [--scenes c2_analytic,testscene,c4_dwarf_room] [--width 1920] [--height 1080] [--spp 256]"""
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
    lum = torch.tensor([0.2126, 0.7152, 0.0722], dtype=torch.float64, device=dev)
    for name in a.scenes.split(","):
        scene = api.Scene.load_scn(os.path.join(ROOT, "data", name + ".scn")).commit().upload(0)
        lights = scene.light_materials()
        groups = {m: g for g, m in enumerate(lights)}
        bins = torch.zeros((8, H, W, 3), dtype=torch.float32, device=dev)
        lengths = torch.zeros((8, H, W), dtype=torch.int32, device=dev)
        frames = torch.zeros((len(lights), H, W, 3), dtype=torch.float32, device=dev)
        rgb = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        ref = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        p = scene.params(W, H, a.spp, a.seed, "pixel")

        def depths(G, with_lengths):
            return lambda: scene.render_depths_device(p, G, bins.data_ptr(), rgb.data_ptr(), lengths.data_ptr() if with_lengths else 0, want_stats=True)["kernel_ms"]

        def split():
            return scene.render_light_groups_device(p, groups, frames.data_ptr(), rgb.data_ptr(), want_stats=True)["kernel_ms"]

        def pixel():
            return scene.render_device(ref.data_ptr(), p, want_stats=True)["kernel_ms"]
        legs = (("depths3", {}, depths(3, False)), ("depths3_len", {}, depths(3, True)), ("groups", {}, split), ("pixel_plain", PLAIN, pixel),
                ("depths8", {}, depths(8, False)), ("pixel", {}, pixel), ("depths8_len", {}, depths(8, True)))
        ms = {k: [] for k, _, _ in legs}
        for r in range(a.warmup + a.calls):
            for k, env, f in legs:
                t = with_env(env, f)
                if r >= a.warmup:
                    ms[k].append(t)
        # the last depths call was G = 8 with lengths: bins, lengths and rgb are its planes
        same = bool(torch.equal(rgb.view(torch.int32), ref.view(torch.int32)))
        sum_err = float((bins.sum(dim=0) - ref).abs().max())
        lengths_ok = bool((lengths.sum(dim=0) == a.spp).all())
        energy = [(bins[g].double() @ lum).sum() for g in range(8)]
        whole = float(sum(energy))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        s = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
        ratio = {"%s/%s" % (x, y): med[x] / med[y] for x in ("depths3", "depths3_len", "depths8", "depths8_len") for y in ("groups", "pixel_plain", "pixel")}
        ratio.update({"depths3_len/depths3": med["depths3_len"] / med["depths3"], "depths8_len/depths8": med["depths8_len"] / med["depths8"],
                      "groups/pixel_plain": med["groups"] / med["pixel_plain"]})
        out = {"tool": "depths_bench", "scene": name, "width": W, "height": H, "spp": a.spp, "light_groups": len(lights), "warmup": a.warmup, "calls": a.calls,
               "rgb_is_the_pixel_render": same, "sum_of_bins_max_abs_diff": sum_err, "frame_max": float(ref.abs().max()), "lengths_add_up_to_spp": lengths_ok,
               "energy_share_per_bin": [float(e) / whole if whole else 0.0 for e in energy],
               "sample_share_per_bin": [float(lengths[g].double().sum()) / (n * a.spp) for g in range(8)],
               "lit_share_per_bin": [float((bins[g] != 0).any(dim=2).double().mean()) for g in range(8)],
               "ratio": ratio, "median_ms": med, "s": s, "mpaths_per_s": {k: n * a.spp / (v * 1e-3) / 1e6 for k, v in med.items()},
               "kernel_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "lib": os.path.relpath(api.LIB_PATH, ROOT)}
        print(json.dumps(out), flush=True)
        scene.close()
        del bins, lengths, frames, rgb, ref
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
