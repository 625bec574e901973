"""Hostile materials (test infrastructure, next to light_groups_cases.py): light_groups_cases' room with every coefficient a
`brdf` line can carry out of range -- Kd > 1, negative, NaN, inf, a Kd whose square underflows, huge, NaN and inf Ks, ior 0,
ior < 1, ior NaN, Kt inf -- under three lights of which one is black.  The .scn lexer reads `1.0e+39` as 1.0 * powf(10, 39) =
+inf and `0.0e+39` as 0 * inf = NaN, in the reference and in the product's loader alike, so the REFERENCE ITSELF renders these
scenes: tests/golden/make_golden.py --only-hostile writes its frames, final states, chains and scene-dumps
(renders_hostile.npz, chains_hostile.npz, manifest.json["generated"]["hostile"]), and the CPU tests
(tests/test_hostile_materials_host.py) and the GPU tests (tests/test_gpu_hostile_materials.py) build the files from here.

Everything is compared with same_words: a word matches when its 32 bits are equal or when both words are NaN (the device's NaN
need not carry x86's sign and payload).  No pixel is skipped and nothing has a tolerance."""
import numpy as np

import light_groups_cases as lg
import reference_goldens as rg

W, H = lg.W, lg.H          # 24 x 16
BIG = (96, 64)             # 24 waves of mixed hostile and grey lanes
SPP = 16
SEED = 2024
RR = 0.8
RECT = (3, 2, 21, 13)
CHAIN_SAMPLES = rg.CHAIN_SAMPLES
FILES = ("renders_hostile.npz", "chains_hostile.npz")
GREY = "0.600000 0.600000 0.600000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0"

# name -> (brdf line: Kd, Ks, shininess, Kt, ior; the shape it is on), in file order
MATERIALS = (
    ("kdgt1", "3.000000 3.000000 3.000000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0",
     "box -3.000000 -3.000000 -0.100000 18.000000 18.000000 0.100000"),                  # floor
    ("neg", "-0.500000 0.500000 0.500000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0",
     "box -3.000000 -3.000000 8.900000 18.000000 18.000000 0.100000"),                   # ceiling
    ("nan", "0.0e+39 0.500000 0.500000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0",
     "box -3.000000 -3.000000 -0.100000 0.100000 18.000000 9.000000"),                   # wall
    ("zero", "0.000000 0.000000 0.000000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0",
     "box 15.000000 -3.000000 -0.100000 0.100000 18.000000 9.000000"),                   # wall
    ("ksnan", "0.600000 0.600000 0.600000 0.0e+39 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0",
     "box -3.000000 -3.000000 -0.100000 18.000000 0.100000 9.000000"),                   # wall
    ("inf", "1.0e+39 0.500000 0.500000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0",
     "box -3.000000 15.000000 -0.100000 18.000000 0.100000 9.000000"),                   # wall
    ("tiny", "1.0e-30 0.000000 0.000000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0",
     "box -1.200000 -1.200000 0.390000 2.400000 2.400000 0.020000"),                     # table
    ("big", "1.0e+30 1.000000 0.000000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0",
     "sphere 0.000000 0.000000 0.870000 0.45"),                                          # under the light
    ("ksinf", "0.300000 0.300000 0.300000 1.0e+39 1.000000 1.000000 10 0.000000 0.000000 0.000000 1.0",
     "sphere -1.000000 -1.000000 0.870000 0.45"),
    ("ior0", "0.000000 0.000000 0.000000 0.000000 0.000000 0.000000 10 1.000000 1.000000 1.000000 0.0",
     "sphere 1.000000 -1.000000 0.870000 0.45"),
    ("iorhalf", "0.000000 0.000000 0.000000 0.200000 0.200000 0.200000 10 1.000000 0.000000 0.500000 0.5",
     "sphere -1.000000 1.000000 0.870000 0.45"),
    ("iornan", "0.100000 0.100000 0.100000 0.000000 0.000000 0.000000 10 1.000000 1.000000 1.000000 0.0e+39",
     "sphere 1.000000 1.000000 0.870000 0.45"),
    ("ktinf", "0.000000 0.000000 0.000000 0.000000 0.000000 0.000000 10 1.0e+39 1.000000 0.000000 1.4",
     "sphere 0.000000 -1.000000 0.870000 0.45"),
)
NAMES = tuple(m[0] for m in MATERIALS)
DIFFUSE_KEEPS = ("kdgt1", "neg", "nan", "zero", "inf", "tiny", "big")   # the diffuse twin: the other six are grey
# light_groups_cases.THREE_LIGHTS' shapes: one light without a red channel, one plain, one black
LIGHTS = """light 3 0 2
sphere 0.000000 0.000000 2.800000 0.9
light 2 1 1
sphere 3.000000 1.000000 2.000000 0.4
light 0 0 0
cylinder -1.200000 -1.200000 2.600000 2.400000 0.000000 0.000000 0.3
"""
HEAD = "\n".join(lg.ROOM.splitlines()[:3]) + "\n"   # screen, camera, ambient
SCENES = ("hostile", "hostile_diffuse")
# material index of a name: material 0 is the loader's default, the brdf lines follow in file order, then the lights
INDEX = {n: i + 1 for i, n in enumerate(NAMES)}
LIGHT_MATERIALS = tuple(range(len(NAMES) + 1, len(NAMES) + 4))


def text(grey=()):
    """the scene with the materials named in grey written as plain 0.6 grey"""
    assert set(grey) <= set(NAMES)
    return HEAD + "".join("brdf %s\n%s\n" % (GREY if n in grey else line, shape) for n, line, shape in MATERIALS) + LIGHTS


def hostile():
    return text()


def hostile_diffuse():
    return text([n for n in NAMES if n not in DIFFUSE_KEEPS])


def swap(name):
    """hostile with one material turned grey"""
    return text([name])


def dark(keep):
    """hostile with every `light` line but the keep-th reading light 0 0 0 (reference_goldens.dark_twin_text's rule)"""
    return rg.dark_text(hostile(), keep)


def scene_text(name):
    return {"hostile": hostile, "hostile_diffuse": hostile_diffuse}[name]()


def variants():
    """[(stem, text)] of every file the goldens are rendered from"""
    return [(n, scene_text(n)) for n in SCENES] + [("hostile_dark%d" % g, dark(g)) for g in range(3)]


# (scene, policy, chunk, (w, h), whether the final states are kept) of renders_hostile.npz, all at SPP and SEED
RENDERS = ([("hostile", p, c, (W, H), p == "pixel") for p, c in (("pixel", 0), ("chunk", 4), ("whole", 0), ("tile32", 0))] +
           [("hostile", p, c, BIG, False) for p, c in (("pixel", 0), ("chunk", 4))] +
           [("hostile_diffuse", p, c, (W, H), p == "pixel") for p, c in (("pixel", 0), ("chunk", 4))] +
           [("hostile_dark%d" % g, "pixel", 0, (W, H), False) for g in range(3)])


def key(scene, policy, chunk, size):
    return scene + "__" + rg.render_key(policy, size[0], size[1], SPP, chunk, SEED)


def write(directory, stem, txt=None):
    """-> (scn, base) of the scene's file in directory"""
    return rg.write_text(directory, stem, scene_text(stem) if txt is None else txt), str(directory) + "/"


def chains_from(z, name):
    """chains_hostile.npz -> {(x, y): (colours (CHAIN_SAMPLES, 3), states)} as render_adaptive_cases.chains gives them"""
    cols, states = z[name + "__colours"], z[name + "__states"]
    assert cols.shape == (H, W, CHAIN_SAMPLES, 3) and states.shape == (H, W, CHAIN_SAMPLES)
    return {(x, y): (cols[y, x], states[y, x]) for y in range(H) for x in range(W)}


def same_words(got, want, what):
    """every 32-bit word of got equals want's, or both are float32 NaNs (any sign, any payload) -> the number of NaN words in want"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == 4 and want.dtype.itemsize == 4, "%s: %s %s vs %s %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    g, w_ = got.view("<u4"), want.view("<u4")
    ne = g != w_
    if got.dtype.kind == "f" and want.dtype.kind == "f":
        nan = lambda v: ((v & 0x7F800000) == 0x7F800000) & ((v & 0x007FFFFF) != 0)
        ne &= ~(nan(g) & nan(w_))
        nans = int(nan(w_).sum())
    else:
        nans = 0
    if ne.any():
        at = tuple(np.argwhere(ne)[0])
        raise AssertionError("%s: %d of %d words differ (%d NaN words expected); first at %s: %r (0x%08x) vs %r (0x%08x)"
                             % (what, int(ne.sum()), ne.size, nans, at, got[at], int(g[at]), want[at], int(w_[at])))
    return nans


def luminance_q(cols):
    """the running sum of squared luminance after each sample of a chain (n, 3), in float32 as adaptive_cases.cut keeps it"""
    import adaptive_cases as ac
    q, out = np.float32(0), []
    with np.errstate(all="ignore"):
        for c in np.asarray(cols, "<f4"):
            l = ac.luminance(c)
            q = np.float32(q + np.float32(l * l))
            out.append(q)
    return np.array(out, "<f4")


class Case:
    """what light_groups_cases.host_light_groups, sample_map_cases.host_sample_map and sample_map_cases.chains take of a case:
    the scene file of `name` written into directory, its committed scene, flattened arrays and oracle scene"""

    write_scene = staticmethod(write)   # (directory, name) -> (scn, base); tests/void_material.py writes its own scenes

    def __init__(self, api, oracle, name, directory):
        self.name, self.oracle, self.csg = name, oracle, True
        self.scn, self.base = self.write_scene(directory, name)
        self.scene = api.Scene.load_scn(self.scn).commit()
        self.flat = self.scene.flatten(W, H)
        self.lights = [int(m) for m in np.nonzero(self.flat.materials["is_light"])[0]]
        self.cam = np.asarray(self.flat.camera, "<f4").reshape(4, 3)
        self._twins = {}

    def hs_args(self):
        return [self.scn, self.base]

    def camera(self, size=None):
        size = tuple(size) if size else (W, H)
        return self.cam if size == (W, H) else np.asarray(self.scene.flatten(*size).camera, "<f4").reshape(4, 3)

    def twin(self, keep):
        k = None if keep is None else frozenset(keep)
        if k not in self._twins:
            self._twins[k] = lg.dark_twin(self.oracle, self.flat, k, self.csg)
        return self._twins[k]

    def table(self, groups, filler=0x5A):
        t = np.full(len(self.flat.materials), filler, np.uint8)
        t[self.lights] = lg.NO_GROUP
        for m, g in groups.items():
            t[m] = g
        return t

    def per_light(self):
        return {m: g for g, m in enumerate(self.lights)}


_cases = {}


def case(api, oracle, name, tmp_path_factory):
    if name not in _cases:
        _cases[name] = Case(api, oracle, name, tmp_path_factory.mktemp("hostile_" + name))
    return _cases[name]


# ---- what the CPU and the GPU tests share: computed once, left unchanged ---------------------------------------------------------
def adaptive_set():
    """min 16, max 64, a check every 16 samples, render_adaptive_cases.FRAME's tolerance and floor"""
    import render_adaptive_cases as rac
    from adaptive_cases import Adaptive
    return Adaptive(16, 64, 16, rac.FRAME.tolerance, rac.FRAME.floor)


def adaptive_late():
    """min 32: the first check comes after the sample (27) at which a pixel of `hostile` overflows its Q"""
    a = adaptive_set()
    return a._replace(min_spp=32)


ADAPTIVE_SETS = (adaptive_set(), adaptive_late())


# a second view for the feature planes: from the table's side up at the ceiling (neg) and the wall at y = 15 (inf), which the
# scene's own camera has behind it.  p, x_axis, y_axis, z_axis as ort_view holds them; a sample looks along px X + py Y - Z
UP_CAM = np.array([[4.0, 3.0, 2.0], [0.3, -0.1, 0.0], [0.05, 0.15, -0.2], [-0.1, -0.75, -0.65]], "<f4")
VIEW_SEEDS = (SEED, 7, 99)
FEATURE_SPP = 5
QUERY_SPP = 4
N_RAYS = 64
N_POINTS = 64
N_AIMED = 16
AIM_SPHERE = (0, 1)   # the file scenes: `big`, the first sphere; part B: the inf light, the second
_shared = {}


def view_cameras(api, c):
    """three views: the scene's own camera, light_groups_cases' second pose, and UP_CAM"""
    return np.stack([c.cam, lg.batch_cameras(api, c)[1], UP_CAM])


# ---- the renders that follow mirrors and glass (follow_cases.py) ---------------------------------------------------------------------
# a view for them: from the middle of the room along -y, wide enough that the left edge of the frame is the wall at x = -3 (nan)
# and the right edge the wall at x = 15 (zero), the two materials with no lobe at all that a sample is followed through.  UP_CAM
# follows nothing (it faces neg and inf, which are recorded): it stays, as the view whose albedo sums are infinite and negative
WALL_CAM = np.array([[6.0, 10.0, 3.0], [1.5, 0.0, 0.0], [0.0, 0.0, -0.6], [0.0, 1.0, 0.0]], "<f4")
FOLLOW_SETTINGS = ((0.5, 64), (0.8, 2))   # (rr, cap): nothing reaches the cap; the cap records specular-only surfaces
SPECULAR_ONLY = ("nan", "zero", "tiny")   # in both scenes; `hostile` adds the Kd = 0 spheres
SPECULAR_SPHERES = ("ior0", "iorhalf", "ktinf")


def follow_world(c):
    """follow_cases' world of a case: the single frame from the scene's own camera on SEED; the batch is that camera, WALL_CAM and
    UP_CAM on VIEW_SEEDS"""
    import follow_cases as fw
    return fw.case_world(c, np.stack([c.cam, WALL_CAM, UP_CAM]), VIEW_SEEDS)


def follow_conditions(c):
    """what the follow frames of a case must exercise, from the oracle's side (follow_cases.chain), printed and asserted: on the
    scene's own camera at rr 0.5, cap 64 at least a tenth of the samples are followed, through each of nan, zero (WALL_CAM's frame:
    the own camera has that wall behind it) and tiny and, on `hostile`, through at least two of the three Kd = 0 spheres; at least
    50 roulette deaths and 50 refractions (hostile_diffuse, which has no transmission: 50 draws that sample_brdf answers with its
    transmission flag all the same); nothing at the cap.  At rr 0.8, cap 2 at least 5 samples are recorded at the cap on a
    specular-only surface and the own frame's albedo plane expects a NaN word -- the nan wall's Kd, recorded -- on `hostile`,
    whose spheres send paths that deep.  UP_CAM's frame holds infinite albedo sums.  -> the bounce rays with a non-finite direction, over all
    frames and both settings"""
    import follow_cases as fw
    w = follow_world(c)
    open_, capped = fw.chains(w, FEATURE_SPP, *FOLLOW_SETTINGS[0]), fw.chains(w, FEATURE_SPP, *FOLLOW_SETTINGS[1])
    o, k = open_[0], capped[0]
    by = lambda ch, n: int(ch.followed_by_mat[INDEX[n]])
    nan_words = int(np.isnan(fw.expected(k)["albedo"]).sum())   # the scene's own frame, the albedo plane alone
    nonfinite = sum(ch.nonfinite_dirs for ch in open_ + capped)
    print("%s rr 0.5 cap 64: followed %.3f of the samples (%s; WALL_CAM %.3f: %s), %d roulette deaths, %d refractions, deepest b %d, %d at the cap; "
          "rr 0.8 cap 2: %d recorded at the cap on a specular-only surface, %d NaN words expected in albedo; %d bounce rays with a non-finite direction"
          % (c.name, o.followed / o.samples, {n: by(o, n) for n in SPECULAR_ONLY + SPECULAR_SPHERES}, open_[2].followed / open_[2].samples,
             {n: by(open_[2], n) for n in SPECULAR_ONLY}, o.deaths, o.refractions, o.max_b, o.at_cap, k.capped_specular, nan_words, nonfinite))
    assert o.followed >= 0.10 * o.samples and o.deaths >= 50 and o.refractions >= 50
    assert all(ch.at_cap == 0 for ch in open_)
    assert by(o, "nan") > 0 and by(o, "tiny") > 0 and by(open_[2], "zero") > 0 and by(open_[2], "nan") > 0
    assert open_[3].followed == 0 and np.isinf(fw.expected(open_[3])["albedo"]).any()
    if c.name == "hostile":
        assert sum(by(o, n) > 0 for n in SPECULAR_SPHERES) >= 2
        assert k.capped_specular >= 5 and nan_words >= 1
    return nonfinite


# ---- the accumulating renders (accumulate_cases.py) -----------------------------------------------------------------------------------
# 64 samples, the whole of a reference chain: accumulate_cases.REF_SPLIT, and a split with a boundary on either side of sample 27
# (index 26), where pixel (14, 11) of `hostile` overflows its Q: one pass ends just before it, a pass of one sample takes it
OVERFLOW_SPLIT = (26, 1, 37)


def accumulate_splits():
    import accumulate_cases as acs
    return (acs.REF_SPLIT, OVERFLOW_SPLIT)


def accumulate_expected(chain, name):
    """the folds of the reference's chains under both splits, by accumulate_cases.model alone, and what they must hold: infinite m2
    words at the end (6 pixels of `hostile`, 8 of hostile_diffuse), and on `hostile` under OVERFLOW_SPLIT none after the first
    pass and one after the pass of one sample -- the continued job reloads a finite Q and leaves an infinite one, and the next
    reloads that.  The reference's chains hold no NaN word (its bounce guard drops every non-finite emission), so neither do the
    sums: the NaN-aware compare is there for the device's sake, not because a NaN is expected"""
    import accumulate_cases as acs
    for split in accumulate_splits():
        want, infs = acs.Planes(), []
        for k in split:
            acs.model(want, 0, chain, None, k, None)
            infs.append(int(np.isinf(want.m2).sum()))
        print("%s %r: infinite m2 words after each pass %r, NaN words %d" % (name, split, infs, sum(int(np.isnan(a).sum()) for a in (want.sum, want.m2, want.rgb))))
        assert infs[-1] >= 3 and np.isfinite(want.sum).all()
        if name == "hostile" and split == OVERFLOW_SPLIT:
            assert infs[:2] == [0, 1]


def ray_cases(c):
    """radiance_cases.mixed on the scene -- 64 rays, 8 of them outside the domain -- and 16 pinholes inside the room that look at
    the sphere under the light (`big`, Kd 1e30; part B: the inf light), whose bounces carry the huge, negative and non-finite terms"""
    import zlib
    import radiance_cases as rc
    k = ("rays", c.name)
    if k not in _shared:
        base = rc.mixed(c.name, c.flat, c.twin(None), N_RAYS, bad=8)
        rng = np.random.default_rng(zlib.crc32(("hostile aimed " + c.name).encode()))
        lo, hi = rc.origin_box(c.flat)
        cams = rc.inside(rng, lo, hi, N_AIMED)
        s = c.flat.spheres[AIM_SPHERE[c.name == "hostile_emission"]]
        z = cams[:, 0] - (s["center"] + rng.normal(size=(N_AIMED, 3)) * 0.4 * s["r"])
        cams[:, 1] = (z / np.linalg.norm(z, axis=1, keepdims=True)).astype("<f4")
        rays = np.array([np.concatenate(rc.pinhole(p, d)) for p, d in cams], "<f4")
        seeds = rng.integers(1, 1 << 32, size=N_AIMED, dtype=np.uint64).astype("<u4")
        _shared[k] = rc.Cases(np.concatenate([base.rays, rays]), np.concatenate([base.seeds, seeds]), np.concatenate([base.cams, cams]),
                              np.concatenate([base.ok, np.ones(N_AIMED, bool)]))
    return _shared[k]


def noisy_ray_cases(c):
    """adaptive_cases.cases_for on the scene: the rays a stopping rule has to work on (in these rooms a ray from anywhere is black
    in its first four samples nine times in ten), so that all three classes of rays are there"""
    import adaptive_cases as ac
    k = ("noisy rays", c.name)
    if k not in _shared:
        _shared[k] = ac.cases_for(c.name, c.flat, c.twin(None), N_RAYS)
    return _shared[k]


def point_set(c):
    """irradiance_cases.point_set on the scene: 64 points, 8 outside the domain, 8 far"""
    import irradiance_cases as ic
    k = ("points", c.name)
    if k not in _shared:
        _shared[k] = ic.point_set(c.name, c.flat, c.twin(None), N_POINTS)
    return _shared[k]


def radiance_expected(c):
    """-> (radiance_cases.expected_of at QUERY_SPP, adaptive_cases.expected under adaptive_cases.MAIN) of ray_cases, and
    adaptive_cases.expected under MAIN of noisy_ray_cases; from the oracle"""
    import adaptive_cases as ac
    import radiance_cases as rc
    k = ("radiance", c.name)
    if k not in _shared:
        cases, osc = ray_cases(c), c.twin(None)
        _shared[k] = (rc.expected_of(osc, cases, (QUERY_SPP,), RR)[QUERY_SPP], ac.expected(osc, cases, ac.MAIN, RR),
                      ac.expected(osc, noisy_ray_cases(c), ac.MAIN, RR))
        osc.set_camera(c.cam)
    return _shared[k]


def feature_expected(c, cams, seeds):
    """[feature_cases.expected of each (camera, seed)] at FEATURE_SPP, from the oracle's first hits"""
    import feature_cases as fc
    k = ("features", c.name, np.asarray(cams, "<f4").tobytes(), tuple(seeds))
    if k not in _shared:
        osc = c.twin(None)
        _shared[k] = [fc.expected(fc.frame(c.oracle, osc, c.flat, cam, W, H, int(s), FEATURE_SPP), FEATURE_SPP) for cam, s in zip(cams, seeds)]
    return _shared[k]


def assert_features(got, want, what):
    """feature_cases.assert_same for every plane but albedo, which holds NaN, inf and negative sums: same_words -> its NaN words"""
    import feature_cases as fc
    fc.assert_same({k: v for k, v in got.items() if k != "albedo"}, want, what)
    return same_words(got["albedo"], want["albedo"], what + " albedo")


def view_frames(c, cams, seeds, policy, chunk):
    """the oracle's frames of the views at SPP, set_camera each"""
    k = ("views", c.name, np.asarray(cams, "<f4").tobytes(), tuple(seeds), policy, chunk)
    if k not in _shared:
        osc, out = c.twin(None), []
        for cam, s in zip(cams, seeds):
            osc.set_camera(np.asarray(cam, "<f4").reshape(4, 3))
            out.append(osc.render(W, H, SPP, int(s), policy, chunk=max(chunk, 1), rr=RR, threads=8)[0])
        osc.set_camera(c.cam)
        _shared[k] = np.stack(out)
    return _shared[k]


# ---- part B: what a file cannot say -- non-finite emission, through Scene.from_arrays -----------------------------------------------
EMIT_W, EMIT_H = 64, 48
EMIT_SEED = 4100


def emission_scene(api):
    """test_gpu_parity._degenerate_scene's room and camera with four lights -- emit (inf, 1, 0), (NaN, 2, 2), (-1, 3e38, 3e38)
    whose sum overflows within 16 samples, and one whose diffuse, specular and transmission coefficients are non-zero too -- and
    three hostile surfaces of MATERIALS' table: the kdgt1 floor, a nan wall and a ktinf sphere.  The reference cannot read this
    scene (its `light` statement takes integers); the oracle's emission code is pinned on the file scenes above"""
    mats = np.zeros(10, api.MATERIAL_DTYPE)
    mats["ior"][:] = 1.0
    mats["diffuse"][1] = (0.7, 0.7, 0.7)
    mats["diffuse"][2] = (3, 3, 3)                                    # kdgt1
    mats["diffuse"][3] = (np.nan, 0.5, 0.5)                           # nan
    mats["transmission"][4] = (np.inf, 1, 0); mats["ior"][4] = 1.4    # ktinf
    mats["is_light"][5:9] = 1
    mats["emit"][5] = (np.inf, 1, 0)
    mats["emit"][6] = (np.nan, 2, 2)
    mats["emit"][7] = (-1, 3e38, 3e38)
    mats["emit"][8] = (4, 4, 4); mats["diffuse"][8] = (0.5, 0.5, 0.5); mats["specular"][8, :3] = 1; mats["transmission"][8] = 1; mats["ior"][8] = 1.5
    mats["diffuse"][9] = (0.2, 0.2, 0.8)
    room = [((-4, -4, -0.2), (4, 4, 0), 2), ((-4, -4, 5), (4, 4, 5.2), 1), ((-4.2, -4, -0.2), (-4, 4, 5.2), 3),
            ((4, -4, -0.2), (4.2, 4, 5.2), 1), ((-4, -4.2, -0.2), (4, -4, 5.2), 9), ((-4, 4, -0.2), (4, 4.2, 5.2), 1)]
    box = np.zeros(len(room), api.BOX_DTYPE)
    for i, v in enumerate(room):
        box[i] = v
    spheres = [((0, 0, 4.2), 0.7, 8), ((0.3, 0.2, 0.6), 0.5, 5), ((1.4, -1.0, 0.45), 0.4, 6), ((-1.0, 1.3, 0.5), 0.45, 7), ((1.5, 1.2, 0.4), 0.4, 4)]
    sph = np.zeros(len(spheres), api.SPHERE_DTYPE)
    for i, v in enumerate(spheres):
        sph[i] = v
    lights = np.array([(1, 0), (1, 1), (1, 2), (1, 3)], api.LIGHT_DTYPE)
    q = np.array([0.279589, 0.480987, 0.718247, 0.416981], "<f4")
    return api.Scene.from_arrays(mats, sph, box, np.zeros(0, api.CYLINDER_DTYPE), lights, [], camera_p=(3.3, 2.0, 2.6), camera_quat_xyzw=q,
                                 camera_height_ratio=0.3, screen=(EMIT_W, EMIT_H))


class EmissionCase:
    """emission_scene committed, its flattened arrays at 64 x 48 and 24 x 16 and the oracle's scenes of both (no reference CSG)"""

    def __init__(self, api, oracle):
        self.name, self.oracle, self.csg = "hostile_emission", oracle, False
        self.scene = emission_scene(api).commit()
        self.flat_big = self.scene.flatten(EMIT_W, EMIT_H)
        self.flat = self.scene.flatten(W, H)
        self.lights = [int(m) for m in np.nonzero(self.flat.materials["is_light"])[0]]
        self.cam = np.asarray(self.flat.camera, "<f4").reshape(4, 3)
        self._twins = {}
        self._big = None

    twin, table, per_light = Case.twin, Case.table, Case.per_light

    def big(self):
        if self._big is None:
            self._big = self.oracle.OracleScene(self.flat_big, with_reference_csg=False)
        return self._big


def emission_case(api, oracle):
    if "emission" not in _cases:
        _cases["emission"] = EmissionCase(api, oracle)
    return _cases["emission"]


def pixel_planes(c, spp=SPP, seed=SEED):
    """-> (the oracle's PIXEL frame at 24 x 16, the final states) of a case without goldens, once"""
    k = ("pixel", c.name, spp, seed)
    if k not in _shared:
        osc = c.twin(None)
        osc.set_camera(c.cam)
        img, _, states = rg.oracle_pixel_planes(c.oracle, osc, W, H, spp, seed, RR)
        _shared[k] = (img, states)
    return _shared[k]


def chains_of(c):
    """render_adaptive_cases.chains of a case without goldens: 64 one-sample calls a pixel, once"""
    import render_adaptive_cases as rac
    k = ("chains", c.name)
    if k not in _shared:
        osc = c.twin(None)
        osc.set_camera(c.cam)
        _shared[k] = rac.chains(osc, W, H, SEED, RR)
    return _shared[k]
