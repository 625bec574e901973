"""ID-matte renders (ort_render_matte, ort_render_views_matte and their device forms) and the mask call (ort_matte_mask): the
reference, and what the planes must give (test infrastructure, next to feature_cases.py).

The reference restates nothing of the render but a histogram.  The per-sample ids come from elsewhere:
 - BY_MATERIAL: feature_cases.frame(...).mat, the oracle's closest hits of the camera samples' rays, which
   tests/test_features_host.py pins against the oracle's own render of the emissive twin;
 - BY_PRIM: the prims of the same rays through ort_raycast -- tools/host_sim --raycast on the CPU side, Scene.raycast on the GPU
   side --, which tests/test_query_lanes_host.py and tests/test_gpu_raycast.py hold to the reference;
 - BY_OBJECT: those prims with a triangle's replaced by HIT_MESH << 28 | its mesh, the mesh from the scene's triangle counts.
A sample is recorded where the oracle's material is not 0.  slots() is include/ort.h's slot rule and final order in plain Python
over those ids, one pixel at a time."""
import os

import numpy as np

import feature_cases as fc
import host_sim_tool as hs

W, H, SPPS, RECT, SEED = fc.W, fc.H, fc.SPPS, fc.RECT, fc.SEED
EMPTY = 0xFFFFFFFF
HIT_MESH = 1
BY = {"material": 0, "object": 1, "prim": 2}
KS = (1, 2, 8)
PLANES = ("ids", "counts", "other", "hits", "states")
GUARDS = {"ids": 0xEEEEEEEE, "counts": 0xEEEEEEEE, "other": 0xEEEEEEEE, "hits": 0xEEEEEEEE, "states": 0xDDDDDDDD}
SCENES = ["open", "c2_analytic", "c3_bunny_room"]


CLOSE_SEED = 31


def world(api, oracle, load_scene, tmp_path_factory, name):
    """feature_cases.world with the batch these tests render: mcams (V, 4, 3) and mseeds, feature_cases' three views and, in the
    bunny room, one more.  From the scene's own camera and from the three posed views the bunny stands in the focal plane, where a
    pixel's samples meet: no pixel of the reference sees more than two triangles.  The fourth view stands half way to the middle of
    the mesh's box, which puts the bunny well in front of the focal plane: pixels with up to four triangles (asserted on the
    reference in tests/test_matte_host.py)"""
    w = fc.world(api, oracle, load_scene, tmp_path_factory, name)
    if not hasattr(w, "mcams"):
        w.mcams, w.mseeds = w.cams, list(w.seeds)
        if name == "c3_bunny_room":
            si = w.scene.info()
            p0 = np.array([si.camera_p.x, si.camera_p.y, si.camera_p.z], "<f4")
            mesh = w.flat.meshes[0]
            p = (p0 + 0.5 * ((mesh["aabb_min"] + mesh["aabb_max"]) / 2 - p0)).astype("<f4")
            close = api.camera_from_pose(p, np.array(list(si.camera_quat_xyzw), "<f4"), si.camera_height_ratio, *w.size)
            assert (close.view("<u4") == oracle.camera(p, np.array(list(si.camera_quat_xyzw), "<f4"), si.camera_height_ratio, *w.size).view("<u4")).all()
            w.mcams, w.mseeds = np.concatenate([w.cams, close[None]]), w.mseeds + [CLOSE_SEED]
    return w


def frames(w, rect=None):
    """feature_cases.frames -- the single frame, then the batch's three --, then the frames of the views this file adds"""
    fr = fc.frames(w, rect)
    key = ("matte_frames", rect)
    if key not in w.cache:
        w.cache[key] = [fc.frame(w.oracle, w.osc, w.flat, cam, w.size[0], w.size[1], seed, fc.MAX_SPP, rect)
                        for cam, seed in list(zip(w.mcams, w.mseeds))[len(w.cams):]]
    return fr + w.cache[key]


# ---- the slot rule ------------------------------------------------------------------------------------------------------------------
def slots(sample_ids, recorded, k):
    """sample_ids, recorded (n, spp): every sample's id and whether it is recorded -> (ids (n, k), counts (n, k), other (n,), hits
    (n,), first (n, k): the kept ids in their order of first appearance, EMPTY behind them): the rule of include/ort.h"""
    n = len(sample_ids)
    ids, counts = np.full((n, k), EMPTY, "<u4"), np.zeros((n, k), "<u4")
    first = np.full((n, k), EMPTY, "<u4")
    other, hits = np.zeros(n, "<u4"), np.zeros(n, "<u4")
    for i in range(n):
        kept, cnt = [], []
        for x, rec in zip(sample_ids[i], recorded[i]):
            if not rec:
                continue
            hits[i] += 1
            x = int(x)
            if x in kept:
                cnt[kept.index(x)] += 1
            elif len(kept) < k:
                kept.append(x)
                cnt.append(1)
            else:
                other[i] += 1
        first[i, :len(kept)] = kept
        order = sorted(range(len(kept)), key=lambda j: (-cnt[j], kept[j]))   # count descending, then id ascending (unsigned)
        ids[i, :len(kept)] = [kept[j] for j in order]
        counts[i, :len(kept)] = [cnt[j] for j in order]
    return ids, counts, other, hits, first


def histogram(sample_ids, recorded):
    """per pixel: {id: count} over the recorded samples"""
    out = []
    for row, rec in zip(sample_ids, recorded):
        h = {}
        for x, r in zip(row, rec):
            if r:
                h[int(x)] = h.get(int(x), 0) + 1
        out.append(h)
    return out


# ---- the per-sample ids ---------------------------------------------------------------------------------------------------------------
def tri_counts(flat):
    return np.array([len(m["indices"]) // 3 for m in flat.meshes], np.int64)


def object_of_prim(flat, prims):
    """ort_raycast's prim words -> the object ids: a triangle's word becomes HIT_MESH << 28 | the mesh that holds that mesh-major
    triangle id; every other word stands"""
    prims = np.asarray(prims, "<u4")
    tri = (prims >> 28) == 0
    ends = np.cumsum(tri_counts(flat))
    mesh = np.searchsorted(ends, (prims & 0x0FFFFFFF).astype(np.int64), side="right")
    assert (mesh[tri] < len(ends)).all()
    return np.where(tri, (HIT_MESH << 28) | mesh.astype("<u4"), prims).astype("<u4")


def object_table(flat):
    """{object id: its material} of the flattened scene, as Scene.object_ids gives it"""
    t = {(HIT_MESH << 28) | i: int(m["mat"]) for i, m in enumerate(flat.meshes)}
    for kind, shapes in ((2, flat.boxes), (3, flat.cylinders), (4, flat.spheres)):
        t.update({(kind << 28) | i: int(m) for i, m in enumerate(shapes["mat"])})
    return t


def host_prims(tool, d, w):
    """rays (n, 6) -> prims, through tools/host_sim --raycast"""
    def prims(rays):
        hits, _ = hs.raycast(tool, d, w.scn, rays, base=w.base, threads=8)
        return hits["prim"], hits["mat"]
    return prims


def device_prims(w):
    """rays (n, 6) -> prims, through ort_raycast on the device"""
    def prims(rays):
        hits, _ = w.scene.raycast(rays)
        return hits["prim"], hits["mat"]
    return prims


def sample_ids(w, prims, by, rect=None):
    """[(ids (n, MAX_SPP), recorded (n, MAX_SPP))] for the single frame and the batch's views.  prims: host_prims or device_prims,
    called once per world and rect and kept; its materials must be the oracle's"""
    fr = frames(w, rect)
    key = ("matte_prims", rect)
    if by != "material" and key not in w.cache:
        got = []
        for f in fr:
            p, m = prims(f.rays.reshape(-1, 6))
            assert (m.reshape(f.mat.shape) == f.mat).all()   # ort_raycast names the oracle's material: the same hit
            got.append(p.reshape(f.mat.shape))
        w.cache[key] = got
    out = []
    for i, f in enumerate(fr):
        rec = f.mat != 0
        if by == "material":
            ids = f.mat.astype("<u4")
        elif by == "prim":
            ids = w.cache[key][i]
        else:
            ids = object_of_prim(w.flat, w.cache[key][i])
        out.append((ids, rec))
    return out


def expected(f, ids, rec, spp, k, guards=None):
    """{plane: array} of frame f: the slots of the first spp samples; pixels outside the rect hold the guards (zeros without)"""
    out = {p: np.full((f.h, f.w) + ((k,) if p in ("ids", "counts") else ()), guards[p] if guards else 0, "<u4") for p in PLANES}
    i, c, o, h, _ = slots(ids[:, :spp], rec[:, :spp], k)
    out["ids"][f.ys, f.xs], out["counts"][f.ys, f.xs], out["other"][f.ys, f.xs], out["hits"][f.ys, f.xs] = i, c, o, h
    out["states"][f.ys, f.xs] = f.after[:, spp - 1]
    return out


def expected_set(w, prims, by, spp, k, rect=None, guards=None):
    """-> (the single frame's planes, the batch's planes stacked (V, h, w, ...))"""
    fr = frames(w, rect)
    per = [expected(f, ids, rec, spp, k, guards) for f, (ids, rec) in zip(fr, sample_ids(w, prims, by, rect))]
    return per[0], {p: np.stack([q[p] for q in per[1:]]) for p in PLANES}


def same_bits(got, want, what):
    for p in got:
        g, w_ = np.ascontiguousarray(got[p]), np.ascontiguousarray(want[p])
        assert g.shape == w_.shape and g.dtype == w_.dtype, "%s %s: %s %s vs %s %s" % (what, p, g.shape, g.dtype, w_.shape, w_.dtype)
        ne = g != w_
        assert not ne.any(), "%s %s: %d of %d words differ; first at %s: %r vs %r" % (what, p, ne.sum(), ne.size, tuple(np.argwhere(ne)[0]),
                                                                                      g[tuple(np.argwhere(ne)[0])], w_[tuple(np.argwhere(ne)[0])])


def guard_planes(shape, k, want=PLANES):
    return {p: np.full(tuple(shape) + ((k,) if p in ("ids", "counts") else ()), GUARDS[p], "<u4") for p in want}


def check_order(ids, counts, other=None, hits=None):
    """what every pixel's slots must satisfy whatever was rendered: the used slots first, by count descending then id ascending;
    no id twice; unused slots (EMPTY, 0); used counts > 0; with other and hits, sum(counts) + other == hits"""
    ids, counts = ids.reshape(-1, ids.shape[-1]).astype(np.int64), counts.reshape(-1, counts.shape[-1]).astype(np.int64)
    used = ids != EMPTY
    assert (used[:, :-1] | ~used[:, 1:]).all() if ids.shape[1] > 1 else True          # no used slot behind an unused one
    assert (counts[~used] == 0).all() and (counts[used] > 0).all()
    if ids.shape[1] > 1:
        both = used[:, 1:]
        a_c, b_c, a_i, b_i = counts[:, :-1], counts[:, 1:], ids[:, :-1], ids[:, 1:]
        assert (~both | (a_c > b_c) | ((a_c == b_c) & (a_i < b_i))).all()             # strictly ordered: so no id twice among neighbours ...
        for j in range(ids.shape[1]):                                                  # ... nor anywhere
            for l in range(j + 1, ids.shape[1]):
                assert not (used[:, j] & used[:, l] & (ids[:, j] == ids[:, l])).any()
    if other is not None:
        assert (counts.sum(axis=1) + other.reshape(-1) == hits.reshape(-1)).all()


# ---- tools/host_sim --matte -------------------------------------------------------------------------------------------------------------
FILES = {"ids": "m_ids.u32", "counts": "m_counts.u32", "other": "m_other.u32", "hits": "m_hits.u32", "states": "m_states.u32"}


def host_sim(tool, d, scene, w, h, rect, spp, by, k, cams=None, seeds=None, seed=0, want=PLANES, base=None, **kw):
    """cams None: the single-frame form on seed; otherwise (V, 4, 3) cameras and (V,) seeds.  -> ({plane: (V, h, w[, k])}, run)"""
    d = str(d)
    path = lambda f: os.path.join(d, f)
    for f in FILES.values():
        if os.path.exists(path(f)):
            os.remove(path(f))
    if cams is None:
        cam_args, nv = ["-", seed], 1
    else:
        np.ascontiguousarray(cams, "<f4").tofile(path("m_cams.f32"))
        np.ascontiguousarray(seeds, "<u4").tofile(path("m_seeds.u32"))
        cam_args, nv = [path("m_cams.f32"), path("m_seeds.u32")], len(cams)
    x0, y0, x1, y1 = rect if rect else (0, 0, w, h)
    r = hs.run(tool, ["--matte"] + hs.scene_args(scene, base) + cam_args + [w, h, x0, y0, x1, y1, spp, BY[by], k] +
               [path(FILES[p]) if p in want else "-" for p in PLANES], **kw)
    out = {}
    for p in PLANES:
        assert os.path.exists(path(FILES[p])) == (p in want)
        if p in want:
            out[p] = np.fromfile(path(FILES[p]), "<u4").reshape((nv, h, w) + ((k,) if p in ("ids", "counts") else ()))
    return out, r


# ---- the mask ---------------------------------------------------------------------------------------------------------------------------
def mask(ids, counts, spp, select):
    """numpy's one line: the selected slots' counts summed as uint32 (wrapping), as float32, over float32(spp)"""
    with np.errstate(over="ignore"):
        return (np.where(np.isin(ids, np.asarray(select, "<u4")) & (ids != EMPTY), counts, 0).astype("<u4").sum(axis=-1, dtype="<u4").astype("<f4")
                / np.float32(spp)).astype("<f4")


def hostile_slots(rng, shape, k):
    """slots no render writes: random small ids with repeats inside a pixel, counts above any spp, 0xFFFFFFFF counts, pixels that are
    all EMPTY, EMPTY slots with counts in them"""
    ids = rng.integers(0, 12, size=tuple(shape) + (k,)).astype("<u4")
    ids[rng.random(ids.shape) < 0.2] = EMPTY
    ids[rng.random(shape) < 0.1] = EMPTY
    big = rng.integers(0, 1 << 32, size=ids.shape, dtype=np.uint64).astype("<u4")
    counts = np.where(rng.random(ids.shape) < 0.5, rng.integers(0, 9, size=ids.shape).astype("<u4"), big)
    counts[rng.random(ids.shape) < 0.1] = 0xFFFFFFFF
    return ids, counts
