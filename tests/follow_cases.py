"""Feature renders that follow mirrors and glass (ort_render_follow, ort_render_views_follow and their device forms) against the
oracle as it stands: the references, and what the planes must give (test infrastructure, next to feature_cases.py).

Two references.
1. THE DIFFUSE TWIN, for final_states.  A second OracleScene from the same flattened scene with only the materials changed: every
   non-light material with |Kd|^2 > 0 becomes a light; everything else -- the specular-only materials, the geometry, the light
   list -- is untouched.  A path of the twin's own PIXEL render ends exactly where the followed sample records its vertex, and
   draws exactly what the followed sample draws on the way, so while no sample reaches the cap the state oracle_tiled_raytrace
   returns per pixel IS final_states.  Nothing of the contract is restated.
2. THE CHAIN in numpy float32, from the oracle alone (chain): feature_cases.camera_rays with its streams hook gives each sample's
   camera ray from the stream where the last sample left it, OracleScene.raycast the vertices, oracle_rng_table the roulette value
   and the burn's steps, unit op 5 sample_brdf and the state after it, unit op 10 wo, numpy float32 the origin updates and the
   sums.  tests/test_follow_host.py pins this helper against reference 1 on every pixel before anything else uses it."""
import os
import struct

import numpy as np

import feature_cases as fc
import host_sim_tool as hs
import ref_io
from hostile_materials import same_words

F = np.float32
W, H, SPPS, RECT, SEED, NO_PRIM = fc.W, fc.H, fc.SPPS, fc.RECT, fc.SEED, fc.NO_PRIM
MAX_SPP = max(SPPS)
PLANES = ("albedo", "normal", "depth", "hits", "ids", "bounces", "states")
GUARDS = dict(fc.GUARDS, bounces=0xEEEEEEEE)
SHAPES = dict(fc.SHAPES, bounces=())
DTYPES = dict(fc.DTYPES, bounces="<u4")
VIEW_SEEDS = [7, 0xDEADBEEF, 99]   # the batch: the scene's own camera on two more seeds, then pose 1 of views_cases.MOVES
EPS, ROUGH = F(0.0001), F(0.01)    # ray.cpp:1196, :1194
FLT_MAX = np.finfo("<f4").max     # the t of a cast that hit nothing
SCENES = ["glass_room", "c2_analytic", "c3_bunny_room", "open"]
SPECULAR_SCENES = ["glass_room", "c2_analytic"]


# ---- reference 1: the diffuse twin ---------------------------------------------------------------------------------------------
def diffuse_part(flat):
    """per material: |Kd|^2 > 0, the f32 x*x + y*y + z*z of ray.cpp:1267 (false for a NaN)"""
    kd = np.asarray(flat.materials["diffuse"], "<f4")
    with np.errstate(all="ignore"):
        return ((kd[:, 0] * kd[:, 0] + kd[:, 1] * kd[:, 1]).astype("<f4") + kd[:, 2] * kd[:, 2]).astype("<f4") > 0


def specular_only(flat):
    """per material: neither the no-hit material, a light, nor one with a diffuse part -- what a sample is followed through"""
    s = ~(np.asarray(flat.materials["is_light"]).reshape(-1) != 0) & ~diffuse_part(flat)
    s[0] = False
    return s


class _Twin:
    pass


def twin(oracle, flat, csg=True):
    """the oracle's scene of flat with every non-light material that has a diffuse part made a light"""
    t = _Twin()
    t.__dict__.update(flat.__dict__)
    mats = flat.materials.copy()
    sel = ~(np.asarray(mats["is_light"]).reshape(-1) != 0) & diffuse_part(flat)
    sel[0] = False
    mats["is_light"][sel] = 1
    mats["emit"][sel] = mats["diffuse"][sel]
    t.materials = mats
    return oracle.OracleScene(t, with_reference_csg=csg)


def twin_states(osc_twin, cam, w, h, seed, spp, rr, rect=None):
    """the final states of the twin's PIXEL jobs (h, w); pixels outside rect: 0"""
    osc_twin.set_camera(cam)
    x0, y0, x1, y1 = rect if rect else (0, 0, w, h)
    states = np.zeros((h, w), "<u4")
    one = np.zeros((h, w, 3), "<f4")
    for y in range(y0, y1):
        for x in range(x0, x1):
            _, states[y, x] = osc_twin.tiled_raytrace(one, x, y, x + 1, y + 1, fc.job_seed(seed, y * w + x), spp, rr)
    return states


# ---- reference 2: the chain ----------------------------------------------------------------------------------------------------
def _step(oracle, state, k=1):
    """the stream's state k steps after state"""
    return struct.unpack_from("<I", oracle.rng_table(int(state), k), 8 * (k - 1))[0]


def _rng_01(oracle, state):
    b = oracle.rng_table(int(state), 1)
    return struct.unpack_from("<I", b, 0)[0], F(struct.unpack_from("<f", b, 4)[0])


def _sample_brdf(oracle, state, n, wo, mats, mat):
    """unit op 5 per row -> (wi (k, 3), is_trans (k,), the states after the three draws)"""
    rows = np.zeros((len(state), 24), "<f4")
    rows[:, 0] = np.asarray(state, "<u4").view("<f4")
    rows[:, 1:4], rows[:, 4:7], rows[:, 7] = n, wo, ROUGH
    rows[:, 8:11], rows[:, 11:14] = mats["diffuse"][mat], mats["specular"][mat][:, :3]
    rows[:, 14:17], rows[:, 17] = mats["transmission"][mat], mats["ior"][mat]
    out = oracle.unit_batch(ref_io.make_unit_records(5, rows))
    return np.ascontiguousarray(out[:, :3], "<f4"), out[:, 3] != 0, np.ascontiguousarray(out[:, 4]).view("<u4").copy()


class Chain:
    """one frame's reference at one (spp, rr, cap): the sums A, N, D (n, ...), hits, B, ids_mat, died0 (sample 0 ended at the
    roulette), void0 (sample 0 ended on a void shape: material 0 WITH a hit, which the oracle's t tells from a miss; void0_bounces:
    the b it did so at), last (n, 6): sample 0's last ray, states (n,), xs, ys, and the counts the conditions are stated on --
    among them void_ends (samples that end on a void shape), void_bounce_ends (those with b >= 1), followed_by_mat (per material,
    the samples followed through it at b == 0) and nonfinite_dirs (bounce rays whose direction has a non-finite component)"""


def chain(oracle, osc, flat, cam, w, h, seed, spp, rr, cap, rect=None):
    mats = flat.materials
    is_light = np.asarray(mats["is_light"]).reshape(-1) != 0
    dif = diffuse_part(flat)
    alb = fc.albedo_table(flat)
    sphere_light = np.asarray(flat.lights["type"]).reshape(-1) == 1   # T_SPHERE
    nl = len(sphere_light)
    rr = F(rr)
    c = Chain()
    c.w, c.h, c.seed, c.cam, c.rect, c.spp, c.rr, c.cap = w, h, seed, np.asarray(cam, "<f4"), rect, spp, rr, cap
    x0, y0, x1, y1 = rect if rect else (0, 0, w, h)
    c.ys, c.xs = [a.reshape(-1) for a in np.mgrid[y0:y1, x0:x1]]
    n = len(c.xs)
    state = fc.oracle_streams(oracle, seed, c.ys.astype(np.int64) * w + c.xs)
    c.A, c.N, c.D = np.zeros((n, 3), "<f4"), np.zeros((n, 3), "<f4"), np.zeros(n, "<f4")
    c.hits, c.B, c.ids_mat = np.zeros(n, "<u4"), np.zeros(n, "<u4"), np.zeros(n, "<u4")
    c.died0, c.void0, c.void0_bounces, c.last = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, np.int64), np.zeros((n, 6), "<f4")
    c.void_ends, c.void_bounce_ends, c.nonfinite_dirs, c.followed_by_mat = 0, 0, 0, np.zeros(len(mats), np.int64)
    c.samples, c.rays, c.followed, c.deaths, c.refractions, c.max_b, c.at_cap, c.capped_specular = n * spp, 0, 0, 0, 0, 0, 0, 0
    with np.errstate(all="ignore"):
        for k in range(spp):
            now = state.copy()
            ap, d, after, _, _ = fc.camera_rays(oracle, cam, w, h, seed, 1, rect, streams=lambda o_, s_, p_: now)
            o, dr, state = ap[:, 0].copy(), d[:, 0].copy(), after[:, 0].copy()
            wo = (-fc._normalize(oracle, dr)).astype("<f4")   # ray.cpp:1241: normalised again (sic)
            L, b = np.zeros(n, "<f4"), np.zeros(n, np.int64)
            act = np.arange(n)
            while len(act):
                c.rays += len(act)
                c.max_b = max(c.max_b, int(b[act].max()))
                t, nrm, mat = osc.raycast(o[act], dr[act])
                void = (mat == 0) & (np.ascontiguousarray(t, "<f4").view("<u4") != FLT_MAX.view("<u4"))   # a void shape, not a miss
                c.void_ends += int(void.sum())
                c.void_bounce_ends += int((void & (b[act] >= 1)).sum())
                if k == 0:
                    c.last[act] = np.concatenate([o[act], dr[act]], axis=1)
                    c.ids_mat[act] = mat
                    c.void0[act] = void
                    c.void0_bounces[act] = np.where(void, b[act], 0)
                hit = mat != 0
                a, t, nrm, mat = act[hit], t[hit], nrm[hit], mat[hit]
                L[a] = (L[a] + t).astype("<f4")
                capped = b[a] == cap
                term = is_light[mat] | dif[mat] | capped
                c.at_cap += int(capped.sum())
                c.capped_specular += int((capped & ~is_light[mat] & ~dif[mat]).sum())
                ta = a[term]
                c.A[ta] = (c.A[ta] + alb[mat[term]]).astype("<f4")
                c.N[ta] = (c.N[ta] + nrm[term]).astype("<f4")
                c.D[ta] = (c.D[ta] + L[ta]).astype("<f4")
                c.B[ta] += b[ta].astype("<u4")
                c.hits[ta] += 1
                ba, tb, nb, mb = a[~term], t[~term], nrm[~term], mat[~term]
                c.followed += int((b[ba] == 0).sum())
                c.followed_by_mat += np.bincount(mb[b[ba] == 0], minlength=len(mats))
                o[ba] = (o[ba] + ((tb - EPS).astype("<f4")[:, None] * dr[ba]).astype("<f4")).astype("<f4")   # ray.cpp:1262 / :1411
                alive = np.zeros(len(ba), bool)
                for i, p in enumerate(ba):
                    state[p], u = _rng_01(oracle, state[p])   # the roulette, ray.cpp:1280
                    alive[i] = u < rr
                    if not alive[i]:
                        c.deaths += 1
                        if k == 0:
                            c.ids_mat[p], c.died0[p] = 0, True
                        continue
                    s = _step(oracle, state[p])   # sample_random_lights' burn, ray.cpp:537-601
                    if nl and sphere_light[s % nl]:
                        s = _step(oracle, s, 4)
                    state[p] = s
                sa = ba[alive]
                if len(sa):
                    wi, tr, state[sa] = _sample_brdf(oracle, state[sa], nb[alive], wo[sa], mats, mb[alive])
                    c.refractions += int(tr.sum())
                    c.nonfinite_dirs += int((~np.isfinite(wi)).any(axis=1).sum())
                    o[sa[tr]] = (o[sa[tr]] + ((F(2.0) * EPS) * dr[sa[tr]]).astype("<f4")).astype("<f4")   # ray.cpp:1345-1348
                    dr[sa], wo[sa] = wi, (-wi).astype("<f4")
                    b[sa] += 1
                act = sa
    c.states = state
    c.partial = int(((c.hits > 0) & (c.hits < spp)).sum())
    return c


def expected(c, guards=None):
    """{plane: array} of chain c: the sums divided by float32(spp), hits, bounces, sample 0's material (ids[..., 1], the shape,
    is not the oracle's to say: NO_PRIM here, compared through ort_raycast on c.last), the final states.  Pixels outside the
    rect hold the guards (zeros without).  Beside the planes, "void0" (h, w) bool: sample 0 ended on a void shape, whose ids are
    {0, that shape} -- what assert_same needs to tell such a pixel from a miss"""
    out = {k: np.full((c.h, c.w) + SHAPES[k], guards[k] if guards else 0, DTYPES[k]) for k in PLANES}
    with np.errstate(all="ignore"):
        out["albedo"][c.ys, c.xs] = (c.A / F(c.spp)).astype("<f4")
        out["normal"][c.ys, c.xs] = (c.N / F(c.spp)).astype("<f4")
        out["depth"][c.ys, c.xs] = (c.D / F(c.spp)).astype("<f4")
    out["hits"][c.ys, c.xs] = c.hits
    out["bounces"][c.ys, c.xs] = c.B
    out["ids"][c.ys, c.xs, 0] = c.ids_mat
    out["ids"][c.ys, c.xs, 1] = NO_PRIM
    out["states"][c.ys, c.xs] = c.states
    out["void0"] = np.zeros((c.h, c.w), bool)
    out["void0"][c.ys, c.xs] = c.void0
    return out


NAN_PLANES = ("albedo", "normal", "depth")


def assert_same(got, want, what, nan=False):
    """every plane of got that want has, all bits; ids as feature_cases.assert_same: the material everywhere, the shape NO_PRIM
    exactly where the material is 0 and nothing was hit.  Where sample 0 ended on a void shape (want["void0"]) the material is 0
    and the shape is NOT NO_PRIM: it is the void shape's, which assert_prims compares through the closest-hit query.
    nan: albedo, normal and depth may hold NaN sums; they go through hostile_materials.same_words (equal bits, or NaN in both)
    -> the number of NaN words expected in those planes (0 without nan)"""
    got = {k: v for k, v in got.items() if v is not None}
    nans = 0
    if nan:
        for k in NAN_PLANES:
            if k in got:
                nans += same_words(got[k], want[k], "%s %s" % (what, k))
        got = {k: v for k, v in got.items() if k not in NAN_PLANES}
    void = want.get("void0")
    if "ids" in got and void is not None and void.any():
        ids = np.ascontiguousarray(got["ids"])
        assert ids.shape == want["ids"].shape and ids.dtype == want["ids"].dtype, "%s ids: %s %s" % (what, ids.shape, ids.dtype)
        bad = void & ((ids[..., 0] != 0) | (ids[..., 1] == NO_PRIM))
        assert not bad.any(), "%s ids: %d void ends of sample 0 are not {0, a shape}; first at %s: %r" % (what, bad.sum(), tuple(np.argwhere(bad)[0]), ids[tuple(np.argwhere(bad)[0])])
        ids = ids.copy()
        ids[void, 1] = NO_PRIM   # held above; every other pixel goes through the shared rule
        got = dict(got, ids=ids)
    fc.assert_same({k: v for k, v in got.items() if k != "bounces"}, want, what)
    if got.get("bounces") is not None:
        ne = np.ascontiguousarray(got["bounces"]) != want["bounces"]
        assert got["bounces"].dtype == np.dtype("<u4") and not ne.any(), "%s bounces: %d words differ, first at %s" % (what, ne.sum(), tuple(np.argwhere(ne)[0]) if ne.any() else ())
    return nans


def assert_prims(got_ids, chains, prims, what):
    """got_ids (V, h, w, 2) against the shapes a raycast of the chains' last rays names (prims, concatenated in the chains' order):
    a sample 0 the roulette ended has NO_PRIM, every other one the record's shape -- the void shape's where it ended on one
    (material 0 with a shape), NO_PRIM where the last ray missed everything"""
    at = 0
    for v, c in enumerate(chains):
        p = np.asarray(prims[at:at + len(c.xs)], "<u4")
        at += len(c.xs)
        assert (p[c.void0] != NO_PRIM).all(), "%s view %d: the closest-hit query names no shape for a void end" % (what, v)
        assert (got_ids[v][c.ys, c.xs, 0][c.void0] == 0).all(), "%s view %d: ids.mat of a void end" % (what, v)
        want = np.where(c.died0, NO_PRIM, p).astype("<u4")
        ne = got_ids[v][c.ys, c.xs, 1] != want
        assert not ne.any(), "%s view %d: ids.prim, %d differ (%d of them void ends)" % (what, v, ne.sum(), (ne & c.void0).sum())


# ---- the conditions the inputs are held to ---------------------------------------------------------------------------------------
def check_conditions(open_chain, capped_chain, name):
    """open_chain: seed 2024, spp 5, rr 0.5, cap 64; capped_chain: rr 0.8, cap 2.  Conditions on the oracle's side, not measurements"""
    c = open_chain
    n = len(c.xs)
    print("%s rr 0.5 cap 64: followed %.3f of the samples, %d roulette deaths, %d refractions, deepest b %d, partial %.3f of the pixels, %d at the cap; "
          "rr 0.8 cap 2: %d recorded at the cap on a specular-only surface" % (name, c.followed / c.samples, c.deaths, c.refractions, c.max_b, c.partial / n,
                                                                            c.at_cap, capped_chain.capped_specular))
    assert c.followed >= 0.10 * c.samples
    assert c.deaths >= 50
    assert c.refractions >= 50
    assert c.max_b >= 2
    assert c.partial >= 0.05 * n
    assert c.at_cap == 0
    assert capped_chain.capped_specular >= 5


# ---- tools/host_sim --follow ------------------------------------------------------------------------------------------------------
FILES = dict(fc.FILES, bounces="f_bounces.u32")


def host_sim(tool, d, scene, w, h, rect, spp, rr, cap, cams=None, seeds=None, seed=0, want=PLANES, base=None, **kw):
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
    r = hs.run(tool, ["--follow"] + hs.scene_args(scene, base) + cam_args + [w, h, x0, y0, x1, y1, spp, repr(float(rr)), cap] +
               [path(FILES[k]) if k in want else "-" for k in PLANES], **kw)
    out = {}
    for k in PLANES:
        assert os.path.exists(path(FILES[k])) == (k in want)
        if k in want:
            out[k] = np.fromfile(path(FILES[k]), DTYPES[k]).reshape((nv, h, w) + SHAPES[k])
    return out, r


# ---- the worlds the CPU and the GPU tests share: computed once, left unchanged ---------------------------------------------------
def world(api, oracle, load_scene, tmp_path_factory, name):
    """feature_cases.world(name) with the batch this feature wants: every frame sees the specular shapes -- the scene's own camera
    on two more seeds, then pose 1 (fcams, fseeds: on the deep scene, feature_cases' own batch)"""
    w = fc.world(api, oracle, load_scene, tmp_path_factory, name)
    if not hasattr(w, "fcams"):
        w.fcams = w.cams if name == "deep" else np.stack([w.own, w.own, w.cams[0]])
        w.fseeds = list(VIEW_SEEDS)
    return w


class CaseWorld:
    """what world() gives, of a case of hostile_materials, void_material or hostile_shapes: scene, scn + base, size, flat, osc (the
    case's oracle scene), own (the case's camera: the single frame, on SEED), fcams and fseeds (the batch), oracle, cache"""


def case_world(c, cams, seeds, size=(W, H)):
    """the world of case c with the batch (cams (V, 4, 3), seeds); kept on the case, so chains are computed once a session"""
    key = (np.ascontiguousarray(cams, "<f4").tobytes(), tuple(int(s) for s in seeds), tuple(size))
    worlds = c.__dict__.setdefault("_follow_worlds", {})
    if key not in worlds:
        w = CaseWorld()
        w.name, w.scene, w.size, w.flat, w.oracle, w.cache = c.name, c.scene, tuple(size), c.flat, c.oracle, {}
        w.scn, w.base = getattr(c, "scn", None), getattr(c, "base", None)
        w.osc, w.own = c.twin(None), np.asarray(c.cam, "<f4").reshape(4, 3)
        w.fcams, w.fseeds = np.ascontiguousarray(cams, "<f4"), [int(s) for s in seeds]
        worlds[key] = w
    return worlds[key]


def chains(w, spp, rr, cap, rect=None):
    """[the single frame (the scene's own camera, SEED), the batch's three] at (spp, rr, cap), cached on the world"""
    key = ("chains", spp, float(rr), cap, rect)
    if key not in w.cache:
        w.cache[key] = [chain(w.oracle, w.osc, w.flat, cam, w.size[0], w.size[1], seed, spp, rr, cap, rect)
                        for cam, seed in [(w.own, SEED)] + list(zip(w.fcams, w.fseeds))]
    return w.cache[key]


def expected_set(w, spp, rr, cap, rect=None, guards=None):
    """-> (the single frame's planes, the batch's planes stacked (V, h, w, ...), the 1 + V chains)"""
    ch = chains(w, spp, rr, cap, rect)
    one = expected(ch[0], guards)
    per = [expected(c, guards) for c in ch[1:]]
    return one, {k: np.stack([p[k] for p in per]) for k in PLANES + ("void0",)}, ch


def pin_on_twin(oracle, w, spp, rr, csg=True):
    """reference 1 pins reference 2 on world w: while nothing reaches the cap, the chains' final states are, on every pixel of the
    single frame and of the batch, the states of the oracle's own PIXEL jobs on the diffuse twin.  The reference itself cannot
    render a followed plane; this is what ties the helper to it on the scene at hand"""
    key = ("pinned", spp, float(rr))
    if key in w.cache:
        return
    tw = twin(oracle, w.flat, csg)
    for v, c in enumerate(chains(w, spp, rr, 64)):
        assert c.at_cap == 0, (w.name, v, c.at_cap)
        ne = twin_states(tw, c.cam, c.w, c.h, c.seed, spp, rr) != expected(c)["states"]
        assert not ne.any(), "%s frame %d spp %d rr %g: %d states differ from the diffuse twin's, first at %s" % (w.name, v, spp, rr, ne.sum(), tuple(np.argwhere(ne)[0]))
    w.cache[key] = True


def assert_renders(render, raycast, w, spp, settings, what, nan=False):
    """the single frame and the batch of world w at every (rr, cap) of settings against reference 2, all planes, and ids[..., 1]
    against the closest-hit query on the chains' last rays.  render(batch, rr, cap) -> {plane: (V, h, w, ...)} (the single frame
    as a batch of one), raycast(rays (n, 6)) -> prims (n,): the implementation under test, on host threads or on the device
    -> the NaN words expected in albedo, normal and depth over all of it"""
    nans = 0
    for rr, cap in settings:
        one, batch, ch = expected_set(w, spp, rr, cap)
        got, gotb = render(False, rr, cap), render(True, rr, cap)
        nans += assert_same({k: v[0] for k, v in got.items()}, one, "%s single rr %g cap %d" % (what, rr, cap), nan)
        nans += assert_same(gotb, batch, "%s batch rr %g cap %d" % (what, rr, cap), nan)
        if "ids" in got:
            prims = raycast(np.ascontiguousarray(np.concatenate([c.last for c in ch]), "<f4"))
            assert_prims(np.concatenate([got["ids"], gotb["ids"]]), ch, prims, "%s rr %g cap %d" % (what, rr, cap))
    return nans


def guard_planes(shape, want=PLANES):
    """{plane: array of shape + the plane's own, filled with its guard}"""
    return {k: np.full(tuple(shape) + SHAPES[k], GUARDS[k], DTYPES[k]) for k in want}
