"""First-hit feature renders (ort_render_features, ort_render_views_features and their device forms) against the oracle as it
stands: the references, and what the planes must give (test infrastructure, next to render_adaptive_cases.py).

Two references.
1. THE EMISSIVE TWIN.  A second OracleScene from the same flattened scene with only the materials changed: every material m >= 1
   becomes a light whose emit is albedo(m) (its own emit if it is a light, else its diffuse).  Geometry and tree are untouched,
   so every primary hit ends its sample without a roulette draw, and the oracle's own PIXEL render of the twin at the same seed and
   spp, any rr, IS the albedo plane; the state oracle_tiled_raytrace returns per pixel IS final_states.  A twin with emit (1, 1, 1)
   gives coverage.  Nothing of the query is restated for these planes.
2. THE CAMERA SAMPLE'S RAY in numpy float32 (camera_rays), for depth, normal and ids.mat: oracle_rng_table(state, 2) gives the
   state after random_between's two steps and its value, unit op 9 the sin/cos, unit op 10 both normalizes, numpy float32 the
   products and sums in oracle_tiled_raytrace's order (focal_length, px, py, to_pixel, focal, ap, dir0); then OracleScene.raycast
   and float32 sums in sample order.  tests/test_features_host.py pins this helper against the oracle through reference 1: the
   albedo and final states it predicts must equal the twin's render on every pixel."""
import os
import struct

import numpy as np

import host_sim_tool as hs
import ref_io

F = np.float32
W, H = 24, 16          # 3 x 2 blocks of 8 x 8: partial in both directions
SPPS = (1, 5)
RECT = (3, 2, 21, 13)
NO_PRIM = 0xFFFFFFFF
PLANES = ("albedo", "normal", "depth", "hits", "ids", "states")
GUARDS = {"albedo": F(-7.0), "normal": F(-7.0), "depth": F(-7.0), "hits": 0xEEEEEEEE, "ids": 0xEEEEEEEE, "states": 0xDDDDDDDD}
SHAPES = {"albedo": (3,), "normal": (3,), "depth": (), "hits": (), "ids": (2,), "states": ()}
DTYPES = {"albedo": "<f4", "normal": "<f4", "depth": "<f4", "hits": "<u4", "ids": "<u4", "states": "<u4"}


# ---- reference 1: the emissive twin ----------------------------------------------------------------------------------------------
def albedo_table(flat):
    """(materials, 3) float32: emit of a light, diffuse otherwise, as they stand"""
    m = flat.materials
    return np.where(np.asarray(m["is_light"]).reshape(-1, 1) != 0, m["emit"], m["diffuse"]).astype("<f4")


class _Twin:
    pass


def twin(oracle, flat, white=False, csg=True):
    """the oracle's scene of flat with every material m >= 1 a light of emit albedo(m), or with white of emit (1, 1, 1)"""
    t = _Twin()
    t.__dict__.update(flat.__dict__)
    mats = flat.materials.copy()
    alb = albedo_table(flat)
    mats["is_light"][1:] = 1
    mats["emit"][1:] = F(1.0) if white else alb[1:]
    t.materials = mats
    return oracle.OracleScene(t, with_reference_csg=csg)


def twin_planes(osc_twin, cam, w, h, seed, spp, rect=None, with_states=True):
    """-> (the twin's PIXEL render (h, w, 3), the per-pixel final states (h, w)) from camera cam; pixels outside rect: 0"""
    osc_twin.set_camera(cam)
    img, _ = osc_twin.render(w, h, spp, seed, "pixel", rect=rect, rr=0.5, threads=8)
    x0, y0, x1, y1 = rect if rect else (0, 0, w, h)
    states = np.zeros((h, w), "<u4")
    if with_states:
        one = np.zeros((h, w, 3), "<f4")
        for y in range(y0, y1):
            for x in range(x0, x1):
                _, states[y, x] = osc_twin.tiled_raytrace(one, x, y, x + 1, y + 1, job_seed(seed, y * w + x), spp, 0.5)
                assert (one[y, x].view("<u4") == img[y, x].view("<u4")).all()   # the PIXEL render is these jobs
    return img, states


def job_seed(master, job):
    import oracle_lib
    return oracle_lib.job_seed(master, job)


# ---- the scene with misses: the closed rooms of data/ have none ------------------------------------------------------------------
def open_scene_text():
    """a .scn of a few shapes over a small slab under an open sky, seen by c2_analytic's camera: 56 thin sticks (cylinders, r 0.012)
    and 20 small spheres strewn between the camera and the slab, most of them far from the focal plane, so that the aperture
    spreads them over several pixels (0 < hits < spp), and a light.  The sticks are more than the prologue's table holds: the rest
    stand in the fast tree.  Numbers from a 32-bit LCG: the same text wherever it is built"""
    state = [1234]

    def u(lo=0.0, hi=1.0):
        state[0] = (state[0] * 1664525 + 1013904223) & 0xFFFFFFFF
        return lo + (hi - lo) * (state[0] >> 8) / float(1 << 24)
    cam = np.array([5.553228, 2.942755, 2.900874])
    t = ["screen 400 300", "camera 5.553228 2.942755 2.900874 b 0.2 q 0.416981 0.279589 0.480987 0.718247",
         "ambient 0.125000 0.125000 0.125000", ""]
    brdf = "brdf %.6f %.6f %.6f %.6f %.6f %.6f %d %.6f %.6f %.6f %.1f"
    t += [brdf % (0.6, 0.6, 0.6, 0, 0, 0, 10, 0, 0, 0, 1.0), "box -1.500000 -1.500000 -0.100000 3.000000 3.000000 0.100000"]
    t += [brdf % (0.8, 0.3, 0.2, 0, 0, 0, 10, 0, 0, 0, 1.0), "box 0.600000 -0.900000 0.000000 0.500000 0.500000 0.900000",
          "sphere -0.400000 0.700000 0.450000 0.450000"]
    t += [brdf % (0.2, 0.4, 0.8, 1, 1, 1, 20, 0, 0, 0, 1.0)]
    for _ in range(56):
        f = u(0.05, 0.95)
        c = cam * f + np.array([u(-0.6, 0.6), u(-0.6, 0.6), u(-0.6, 0.6)]) * (0.3 + f)
        d = np.array([u(-1, 1), u(-1, 1), u(-1, 1)])
        d = d / max(np.linalg.norm(d), 0.1) * u(2.0, 4.0)
        t.append("cylinder %.6f %.6f %.6f %.6f %.6f %.6f 0.012000" % (tuple(c - d / 2) + tuple(d)))
    t += [brdf % (0.1, 0.7, 0.3, 0, 0, 0, 10, 0, 0, 0, 1.0)]
    for _ in range(20):
        f = u(0.05, 0.9)
        c = cam * f + np.array([u(-0.5, 0.5), u(-0.5, 0.5), u(-0.5, 0.5)]) * (0.3 + f)
        t.append("sphere %.6f %.6f %.6f 0.030000" % tuple(c))
    t += [brdf % (0, 0, 0, 0, 0, 0, 10, 1, 1, 1, 1.4), "sphere 1.300000 1.200000 0.350000 0.350000"]
    t += ["", "light 4 3 2", "sphere 0.200000 -0.200000 1.600000 0.250000"]
    return "\n".join(t) + "\n"


# ---- reference 2: the camera sample's ray -------------------------------------------------------------------------------------
def _normalize(oracle, v):
    return np.ascontiguousarray(oracle.unit_batch(ref_io.make_unit_records(10, np.asarray(v, "<f4").reshape(-1, 3)))[:, :3], "<f4")


def _scale(s, v):
    return (np.asarray(s, "<f4").reshape(-1, 1) * np.asarray(v, "<f4").reshape(1, 3)).astype("<f4")


def oracle_streams(oracle, seed, pix):
    """the pixels' stream seeds, one oracle_job_seed call each"""
    return np.array([job_seed(seed, int(i)) for i in pix], "<u4")


def oracle_draw(oracle, state):
    """the aperture angle's draw, one oracle_rng_table call a stream -> (the states after it, the angles)"""
    after, rad = np.zeros(len(state), "<u4"), np.zeros(len(state), "<f4")
    for i in range(len(state)):
        # n = 2: {state, value} x 2 of rng_01, then two chained random_between(0, 2 pi): the state after two steps sits
        # in the second rng_01 entry, the first random_between value behind the four words
        b = oracle.rng_table(int(state[i]), 2)
        after[i] = struct.unpack_from("<I", b, 8)[0]
        rad[i] = struct.unpack_from("<f", b, 16)[0]
    return after, rad


def camera_rays(oracle, cam, w, h, seed, spp, rect=None, streams=oracle_streams, draw=oracle_draw):
    """cam (4, 3): p, x_axis, y_axis, z_axis.  -> (ap (n, spp, 3), d (n, spp, 3), states after each sample (n, spp), xs, ys) for the
    n pixels of rect in row-major order: every sample's primary ray as oracle_tiled_raytrace composes it, operation by operation.
    streams, draw: the two steps that cost an oracle call a pixel, for a caller with a whole large frame to get through (and
    its own duty to pin what it passes against these)"""
    cam = np.asarray(cam, "<f4").reshape(4, 3)
    p, X, Y, Z = cam
    x0, y0, x1, y1 = rect if rect else (0, 0, w, h)
    ys, xs = [a.reshape(-1) for a in np.mgrid[y0:y1, x0:x1]]
    n = len(xs)
    with np.errstate(all="ignore"):
        v = np.array([p[0] - F(0), p[1] - F(0), p[2] - F(0.2)], "<f4")
        fl = np.sqrt(((v[0] * v[0]).astype("<f4") + (v[1] * v[1]).astype("<f4")).astype("<f4") + (v[2] * v[2]).astype("<f4"))   # v_len
        px = ((F(2.0) * xs.astype("<f4")).astype("<f4") / F(w)).astype("<f4") - F(1.0)
        py = ((F(2.0) * ys.astype("<f4")).astype("<f4") / F(h)).astype("<f4") - F(1.0)
        to_pixel = _normalize(oracle, ((_scale(px, X) + _scale(py, Y)).astype("<f4") - Z[None, :]).astype("<f4"))
        focal = (p[None, :] + (F(fl) * to_pixel).astype("<f4")).astype("<f4")
        state = streams(oracle, seed, ys.astype(np.int64) * w + xs)
        ap = np.zeros((n, spp, 3), "<f4")
        d = np.zeros((n, spp, 3), "<f4")
        after = np.zeros((n, spp), "<u4")
        for k in range(spp):
            state, rad = draw(oracle, state)
            sc = oracle.unit_batch(ref_io.make_unit_records(9, rad.reshape(-1, 1)))
            sn, cs = sc[:, 0].astype("<f4"), sc[:, 1].astype("<f4")
            a = (p[None, :] + _scale((F(0.1) * cs).astype("<f4"), X)).astype("<f4")
            a = (a + _scale((F(0.1) * sn).astype("<f4"), Y)).astype("<f4")
            a = (a - (F(0.1) * Z).astype("<f4")[None, :]).astype("<f4")
            ap[:, k] = a
            d[:, k] = _normalize(oracle, (focal - a).astype("<f4"))
            after[:, k] = state
    return ap, d, after, xs, ys


class Frame:
    """one frame's reference: rays (n, spp, 6) of the rect's pixels, t, mat (n, spp), nrm (n, spp, 3), after (n, spp), xs, ys, and
    the flattened scene's albedo table"""


def frame(oracle, osc, flat, cam, w, h, seed, spp, rect=None):
    """the oracle's first hits of every sample of every pixel of rect, at the largest spp a test uses"""
    f = Frame()
    f.w, f.h, f.seed, f.cam, f.rect = w, h, seed, np.asarray(cam, "<f4"), rect
    ap, d, f.after, f.xs, f.ys = camera_rays(oracle, cam, w, h, seed, spp, rect)
    f.rays = np.concatenate([ap, d], axis=2)
    t, nrm, mat = osc.raycast(ap.reshape(-1, 3), d.reshape(-1, 3))
    n = len(f.xs)
    f.t, f.nrm, f.mat = t.reshape(n, spp), nrm.reshape(n, spp, 3), mat.reshape(n, spp)
    f.albedo = albedo_table(flat)
    f.is_light = np.asarray(flat.materials["is_light"]).reshape(-1)
    return f


def expected(f, spp, guards=None):
    """{plane: array} of frame f at spp (a prefix of its samples): float32 sums in sample order over the samples that hit, divided
    by float32(spp); hits; sample 0's material (ids[..., 1], the shape, is not the oracle's to say: it stays at NO_PRIM for a miss
    and is otherwise compared through ort_raycast); the final states.  Pixels outside the rect hold the guards (zeros without)"""
    out = {k: np.full((f.h, f.w) + SHAPES[k], guards[k] if guards else 0, DTYPES[k]) for k in PLANES}
    n = len(f.xs)
    A, N, D = np.zeros((n, 3), "<f4"), np.zeros((n, 3), "<f4"), np.zeros(n, "<f4")
    hits = np.zeros(n, "<u4")
    with np.errstate(all="ignore"):
        for k in range(spp):
            hit = f.mat[:, k] != 0
            A[hit] = (A[hit] + f.albedo[f.mat[hit, k]]).astype("<f4")
            N[hit] = (N[hit] + f.nrm[hit, k]).astype("<f4")
            D[hit] = (D[hit] + f.t[hit, k]).astype("<f4")
            hits[hit] += 1
        out["albedo"][f.ys, f.xs] = (A / F(spp)).astype("<f4")
        out["normal"][f.ys, f.xs] = (N / F(spp)).astype("<f4")
        out["depth"][f.ys, f.xs] = (D / F(spp)).astype("<f4")
    out["hits"][f.ys, f.xs] = hits
    out["ids"][f.ys, f.xs, 0] = f.mat[:, 0]
    out["ids"][f.ys, f.xs, 1] = NO_PRIM
    out["states"][f.ys, f.xs] = f.after[:, spp - 1]
    return out


def assert_same(got, want, what, prims=True):
    """every plane of got that want has, all bits; ids: the material everywhere; the shape must be NO_PRIM exactly where the
    material is 0 and the sample missed (prims: the caller compares the shapes of hits through ort_raycast)"""
    for k in PLANES:
        if k not in got or got[k] is None:
            continue
        g, w_ = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w_.shape and g.dtype == w_.dtype, "%s %s: %s %s vs %s %s" % (what, k, g.shape, g.dtype, w_.shape, w_.dtype)
        gu, wu = g.view("<u4"), w_.view("<u4")
        ne = gu != wu
        if k == "ids":
            hit = w_[..., 0] != 0
            guard = (w_[..., 0] == GUARDS["ids"]) & (w_[..., 1] == GUARDS["ids"])
            ne[..., 1] &= ~(hit & ~guard)   # a hit's shape: any value but NO_PRIM
            ne[..., 1] |= hit & ~guard & (g[..., 1] == NO_PRIM)
        if ne.any():
            i = tuple(np.argwhere(ne)[0])
            raise AssertionError("%s %s: %d of %d words differ; first at %s: %r vs %r" % (what, k, ne.sum(), ne.size, i, g[i], w_[i]))


def stats_of(frames, spp):
    """over a set of frames at spp: (share of samples that miss, share of pixels with 0 < hits < spp, pixels whose sample 0 sees a
    light)"""
    miss = np.concatenate([(f.mat[:, :spp] == 0).reshape(-1) for f in frames])
    hits = np.concatenate([(f.mat[:, :spp] != 0).sum(axis=1) for f in frames])
    lights = sum(int((np.asarray(f.is_light)[f.mat[:, 0]] != 0).sum()) for f in frames)
    return miss.mean(), ((hits > 0) & (hits < spp)).mean(), lights


# ---- tools/host_sim --features ----------------------------------------------------------------------------------------------------
FILES = {"albedo": "f_albedo.f32", "normal": "f_normal.f32", "depth": "f_depth.f32", "hits": "f_hits.u32", "ids": "f_ids.u32", "states": "f_states.u32"}


def host_sim(tool, d, scene, w, h, rect, spp, cams=None, seeds=None, seed=0, want=PLANES, base=None, **kw):
    """cams None: the single-frame form on seed; otherwise (V, 4, 3) cameras and (V,) seeds.  -> ({plane: (V, h, w, ...)}, run)"""
    d = str(d)
    path = lambda f: os.path.join(d, f)
    for f in FILES.values():
        if os.path.exists(path(f)):
            os.remove(path(f))
    if cams is None:
        cam_args, nv = ["-", seed], 1
    else:
        np.ascontiguousarray(cams, "<f4").tofile(path("f_cams.f32"))
        np.ascontiguousarray(seeds, "<u4").tofile(path("f_seeds.u32"))
        cam_args, nv = [path("f_cams.f32"), path("f_seeds.u32")], len(cams)
    x0, y0, x1, y1 = rect if rect else (0, 0, w, h)
    r = hs.run(tool, ["--features"] + hs.scene_args(scene, base) + cam_args + [w, h, x0, y0, x1, y1, spp] +
               [path(FILES[k]) if k in want else "-" for k in PLANES], **kw)
    out = {}
    for k in PLANES:
        assert os.path.exists(path(FILES[k])) == (k in want)
        if k in want:
            out[k] = np.fromfile(path(FILES[k]), DTYPES[k]).reshape((nv, h, w) + SHAPES[k])
    return out, r


# ---- the worlds the CPU and the GPU tests share: computed once, left unchanged ---------------------------------------------------
SEED = 2024
VIEW_SEEDS = [7, 0xDEADBEEF, 99]   # the batch: poses 1 and 2 of views_cases.MOVES (moved and yawed), then pose 0 -- the single frame's camera -- on another seed
MAX_SPP = max(SPPS)
_worlds = {}


class World:
    """scene (committed), scn + base (what tools/host_sim loads), size, flat, osc, own (the scene's camera), cams (3, 4, 3), seeds"""


def world(api, oracle, load_scene, tmp_path_factory, name):
    """name: a scene of data/, "open" (open_scene_text), "tables_<variant>" (tools/make_tablescene.py) or "deep"
    (tools/make_deepscene.py, at 8 x 8)"""
    if name in _worlds:
        return _worlds[name]
    import views_cases
    w = World()
    w.name, w.size, csg = name, (W, H), True
    if name == "open":
        d = tmp_path_factory.mktemp("features_open")
        w.scn, w.base = str(d / "open.scn"), str(d) + "/"
        with open(w.scn, "w") as f:
            f.write(open_scene_text())
        w.scene = api.Scene.load_scn(w.scn).commit()
    elif name.startswith("tables_"):
        import table_scenes
        d = tmp_path_factory.mktemp("features_" + name)
        scene, _, csg = table_scenes.build(api, name[len("tables_"):], d)
        w.scene, w.scn, w.base = scene.commit(), str(d / (name[len("tables_"):] + ".scn")), str(d) + "/"
    elif name == "deep":
        import deep_scenes
        dw = deep_scenes.world(api, oracle, tmp_path_factory)
        w.scene, w.scn, w.base, w.size = dw.scene, dw.scn, dw.base, (8, 8)
    else:
        w.scene, w.scn, w.base = load_scene(name), name, None
    w.flat = w.scene.flatten(*w.size)
    w.osc = oracle.OracleScene(w.flat, with_reference_csg=csg)
    w.own = w.scene.camera(*w.size)
    if name == "deep":
        other = deep_scenes.view_cams(api, dw, *w.size)[1]
        w.cams = np.stack([other, other, w.own])
    else:
        ps = views_cases.poses(w.scene, w.flat)
        for p, q, r in ps:   # the product's pose helper is the oracle's
            assert (api.camera_from_pose(p, q, r, *w.size).view("<u4") == oracle.camera(p, q, r, *w.size).view("<u4")).all()
        c = [api.camera_from_pose(p, q, r, *w.size) for p, q, r in ps]
        w.cams = np.stack([c[1], c[2], c[0]])
    w.seeds = list(VIEW_SEEDS)
    w.oracle, w.cache = oracle, {}
    _worlds[name] = w
    return w


def frames(w, rect=None, spp=MAX_SPP):
    """[the single frame (the scene's own camera, SEED), the batch's three]: the oracle's first hits of spp samples a pixel"""
    key = ("frames", rect, spp)
    if key not in w.cache:
        w.cache[key] = [frame(w.oracle, w.osc, w.flat, cam, w.size[0], w.size[1], seed, spp, rect)
                        for cam, seed in [(w.own, SEED)] + list(zip(w.cams, w.seeds))]
    return w.cache[key]


def expected_set(w, spp, rect=None, guards=None, max_spp=MAX_SPP):
    """-> (the single frame's planes, the batch's planes stacked (3, h, w, ...))"""
    fr = frames(w, rect, max_spp)
    one = expected(fr[0], spp, guards)
    per = [expected(f, spp, guards) for f in fr[1:]]
    return one, {k: np.stack([p[k] for p in per]) for k in PLANES}


def guard_planes(shape, want=PLANES):
    """{plane: array of shape + the plane's own, filled with its guard}"""
    return {k: np.full(tuple(shape) + SHAPES[k], GUARDS[k], DTYPES[k]) for k in want}
