"""Cost of the ID-matte render (ort_render_matte_device, kernels matte_pixels) against the first-hit feature render of the same
samples and against the route it replaces, and of ort_matte_mask_device against a copy, in the same process, one GPU.

Per scene (c3_bunny_room, c2_analytic, c4_dwarf_room by default), at --size (1920x1080) and --spp (16), the scene's own camera:
  features   the comparator: ort_render_features_device with the hits and ids planes, the parent's kernel on the same rays.
  matte      (a) ort_render_matte_device with all five planes, per mode (material, object, prim) and K in --slots (1, 4, 8).
  All get --warmup calls, then --calls timed calls, alternating call by call so that clocks and cache state drift alike; a call's
  time is the library's own kernel_ms (one pair of HIP events around its kernel).  ratio = median matte / median features, with
  each side's spread s = (max - min) / median; above = ratio > 1 + s of the comparator.
  route      (b) the route it replaces, whole, --route-calls times on the host clock: ort_raycast_device over materialised camera
             rays (the aperture angle drawn with torch: for timing any angle does), the hits brought to the host, and a numpy
             histogram per pixel (a sort of each pixel's ids and the run lengths), by material.  Its three parts are given apart.
  bytes      (c) what each route moves: the matte's planes (8 K + 12 B a pixel) against 24 B of ray up and 24 B of hit down per
             sample, and the hits again over the bus.
  shares     (d) the share of pixels with more than one id and with other > 0, per mode and K.
  mask       (e) ort_matte_mask_device on the K = 8 object slots, selecting every object of the most common material, against a
             device-to-device copy of as many bytes as it reads and writes, --mask-calls each, alternating, torch events on one stream.
One JSON line per scene.  No figure is required: the lines record.
usage: python3 tools/matte_bench.py [--scenes ...] [--size 1920x1080] [--spp 16] [--slots 1,4,8] [--warmup 3] [--calls 7]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

EMPTY = 0xFFFFFFFF


def host_histogram(mat, spp):
    """(pixels * spp,) materials -> per pixel the sorted ids and where a run starts: numpy's part of the route the call replaces"""
    ids = np.sort(mat.reshape(-1, spp), axis=1)
    starts = np.ones(ids.shape, bool)
    starts[:, 1:] = ids[:, 1:] != ids[:, :-1]
    return ids, starts, (starts & (ids != 0)).sum(axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c3_bunny_room,c2_analytic,c4_dwarf_room")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--slots", default="1,4,8")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--route-calls", type=int, default=2)
    ap.add_argument("--mask-calls", type=int, default=21)
    ap.add_argument("--seed", type=int, default=20261021)
    args = ap.parse_args()
    assert args.calls >= 5 and args.warmup >= 2
    os.environ.setdefault("ORT_KNOBS_LIVE", "1")
    import torch
    from features_bench import camera_rays
    from offline_raytracer_amd import api
    if api.device_count() < 1:
        raise SystemExit("matte_bench needs a HIP device: nothing here is measured without one")
    dev = torch.device("cuda", 0)
    w, h = (int(v) for v in args.size.split("x"))
    spp, n = args.spp, w * h
    ks = [int(k) for k in args.slots.split(",")]
    kmax = max(ks)
    for name in args.scenes.split(","):
        scene = api.Scene.load_scn(os.path.join(ROOT, "data", name + ".scn")).commit().upload(0)
        u32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        f_planes = {"hits": u32(h, w), "ids": u32(h, w, 2)}
        m_planes = {"ids": u32(h, w, kmax), "counts": u32(h, w, kmax), "other": u32(h, w), "hits": u32(h, w), "states": u32(h, w)}
        f_ptrs, m_ptrs = {k: t.data_ptr() for k, t in f_planes.items()}, {k: t.data_ptr() for k, t in m_planes.items()}
        params = lambda counters=False: api.Scene.params(w, h, spp, args.seed, "pixel", counters=counters)
        torch.cuda.synchronize(dev)

        def features(counters=False):
            return scene.render_features_device(params(counters), want_stats=True, **f_ptrs)

        def matte(by, k):
            return lambda counters=False: scene.render_matte_device(params(counters), by, k, want_stats=True, **m_ptrs)
        calls = [("features", features)] + [("%s_%d" % (by, k), matte(by, k)) for by in ("material", "object", "prim") for k in ks]
        for _ in range(args.warmup):
            for _, fn in calls:
                fn()
        ms = {k: [] for k, _ in calls}
        for _ in range(args.calls):
            for key, fn in calls:
                ms[key].append(fn()["kernel_ms"])
        med = {k: float(np.median(v)) for k, v in ms.items()}
        s = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
        shares, node_tests = {}, {}
        for key, fn in calls:
            st = fn(counters=True)
            node_tests[key] = st["node_tests"] / (n * spp)
            assert st["rays"] == n * spp
            if key != "features":
                k = int(key.rsplit("_", 1)[1])
                # a K-slot render writes K words a pixel at the front of the buffer: pixel-major, K wide
                ids = m_planes["ids"].reshape(-1)[: n * k].view(h, w, k)
                shares[key] = {"several_ids": float((ids[..., 1] != -1).double().mean().item()) if k > 1 else None,
                               "other": float((m_planes["other"] != 0).double().mean().item())}
        # (b) the route it replaces, whole
        rays = camera_rays(torch, scene.camera(w, h), w, h, spp, args.seed, dev)
        d_hits = torch.empty((n * spp * 24,), dtype=torch.uint8, device=dev)
        route = []
        for _ in range(args.route_calls + 1):   # the first is the warm-up
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            st = scene.raycast_device(rays.data_ptr(), n * spp, d_hits.data_ptr(), want_stats=True)
            t1 = time.perf_counter()
            hits = d_hits.cpu().numpy().view(api.HIT_DTYPE)
            t2 = time.perf_counter()
            _, _, several = host_histogram(hits["mat"], spp)
            t3 = time.perf_counter()
            route.append({"kernel_ms": st["kernel_ms"], "call_ms": (t1 - t0) * 1e3, "download_ms": (t2 - t1) * 1e3, "histogram_ms": (t3 - t2) * 1e3,
                          "whole_ms": (t3 - t0) * 1e3})
        route = route[1:]
        # (e) the mask against a copy of its bytes
        scene.render_matte_device(params(), "object", kmax, **m_ptrs)
        ids, mats = scene.object_ids()
        select = ids[mats == np.argmax(np.bincount(mats))][:api.MAX_MATTE_SELECT]
        d_mask = torch.empty((h, w), dtype=torch.float32, device=dev)
        nbytes = n * (8 * kmax + 4)
        src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev), torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        ev = lambda: torch.cuda.Event(enable_timing=True)
        mask_ms, copy_ms = [], []
        for i in range(args.mask_calls + 3):
            a, b, c = ev(), ev(), ev()
            a.record(stream)
            api.matte_mask_device(m_ptrs["ids"], m_ptrs["counts"], kmax, spp, select, w, h, d_mask.data_ptr(), stream=stream.cuda_stream)
            b.record(stream)
            dst.copy_(src)   # reads nbytes / 2, writes nbytes / 2: as many bytes as the mask call moves
            c.record(stream)
            c.synchronize()
            if i >= 3:
                mask_ms.append(a.elapsed_time(b))
                copy_ms.append(b.elapsed_time(c))
        out = {"tool": "matte_bench", "scene": name, "width": w, "height": h, "spp": spp, "warmup": args.warmup, "calls": args.calls,
               "median_ms": med, "s": s, "ratio": {k: med[k] / med["features"] for k in med if k != "features"},
               "above": {k: bool(med[k] / med["features"] > 1 + s["features"]) for k in med if k != "features"},
               "ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "node_tests_per_ray": node_tests, "shares": shares,
               "route": route, "route_over_matte_material_%d" % kmax: float(np.median([r["whole_ms"] for r in route])) / med["material_%d" % kmax],
               "bytes_matte": {str(k): int(n * (8 * k + 12)) for k in ks}, "bytes_features": int(n * 12), "bytes_route_device": int(n * spp * 48),
               "bytes_route_bus": int(n * spp * 24),
               "mask": {"select": int(len(select)), "bytes": int(nbytes), "mask_ms": float(np.median(mask_ms)), "copy_ms": float(np.median(copy_ms)),
                        "mask_s": (max(mask_ms) - min(mask_ms)) / float(np.median(mask_ms)), "copy_s": (max(copy_ms) - min(copy_ms)) / float(np.median(copy_ms)),
                        "coverage": float(d_mask.double().mean().item())},
               "lib": os.path.relpath(api.LIB_PATH, ROOT)}
        print(json.dumps(out), flush=True)
        del rays, d_hits, hits, f_planes, m_planes, d_mask, src, dst
        torch.cuda.empty_cache()
        scene.close()


if __name__ == "__main__":
    main()
