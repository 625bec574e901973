"""The shapes a scene's fast tree can take, for the CPU and the GPU tests that pin "the tree's shape cannot change a bit"
(tests/test_tree_shapes_host.py, tests/test_gpu_tree_shapes.py): the commit-time variants, stated once;
which variant changes which scene's tree; the scenes' worlds -- rays, points, frames and the oracle's answers for them,
computed once per scene and session and left unchanged, since the oracle walks no fast tree and so knows no variant -- and
the conditions that make the cluster scene's ray set meet its purpose, checked from the oracle's hits alone."""
import os
import sys
import zlib

import numpy as np

import ao_cases
import feature_cases
import host_sim_tool as hs
import irradiance_cases
import light_groups_cases as lg
import radiance_cases
import raycast_cases
import render_adaptive_cases as rac
import sample_map_cases as sm
import views_cases
from adaptive_cases import Adaptive
from conftest import DATA, GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_clusterscene  # noqa: E402

# what ort_scene_commit reads (csrc/ort_tree.cpp: build_tree)
COMMIT_KNOBS = ("ORT_LEAF_TRI", "ORT_LEAF_OTHER", "ORT_ANALYTIC_PROLOGUE", "ORT_TREE_SPLIT_KINDS")
VARIANTS = {
    "default": {},
    "leaf1": {"ORT_LEAF_TRI": "1", "ORT_LEAF_OTHER": "1"},
    "leaf16": {"ORT_LEAF_TRI": "16", "ORT_LEAF_OTHER": "16"},
    "no_prologue": {"ORT_ANALYTIC_PROLOGUE": "0"},
    "mixed_root": {"ORT_ANALYTIC_PROLOGUE": "0", "ORT_TREE_SPLIT_KINDS": "0", "ORT_LEAF_TRI": "16", "ORT_LEAF_OTHER": "16"},
    "small_prologue": {"ORT_ANALYTIC_PROLOGUE": "3", "ORT_LEAF_TRI": "2"},
}
# The variants that change each scene's tree (test_tree_shapes_host.py::test_every_listed_variant_changes_the_tree asserts it for
# every row, so none is vacuous).  Not listed: leaf1 on c2_analytic (every leaf of its default tree holds one shape already)
# and leaf1, leaf16 on glass_room (all its shapes but one cylinder are in the prologue: the tree is one leaf).
LISTED = {
    "testscene": ["leaf1", "leaf16", "no_prologue", "mixed_root", "small_prologue"],
    "c4_dwarf_room": ["leaf1", "leaf16", "no_prologue", "mixed_root", "small_prologue"],
    "c2_analytic": ["leaf16", "no_prologue", "mixed_root", "small_prologue"],
    "glass_room": ["no_prologue", "mixed_root", "small_prologue"],
    "cluster": ["leaf1", "leaf16", "no_prologue", "mixed_root", "small_prologue"],
}
SCENES = list(LISTED)
HAS_TRIANGLES_AND_ANALYTIC = ["testscene", "c4_dwarf_room", "cluster"]
# every (scene, variant) the lane tests run: the default tree, the control, first
PAIRS = [(s, v) for s in SCENES for v in ["default"] + LISTED[s]]
PAIR_IDS = ["%s-%s" % p for p in PAIRS]

SEED = 4242
N_RAYS = 2000
N_MIXED_CLUSTER = 600                 # of the cluster scene's 2 000: the mixed set; the other 1 400 are aimed
RENDER = (48, 32, 4, 2)               # the host's frame: w, h, spp, chunk
GPU_RENDER = (64, 48, 4, 2)
GOLDEN_RENDERS = [("chunk", 2), ("pixel", 1)]   # the reference's own renders of the cluster scene at RENDER, SEED
N_RADIANCE, RADIANCE_SPP = 200, 4
N_POINTS_HOST, N_POINTS = 200, 256
AO_SPP = 4
IRR_SPP = 2
FEATURES = (32, 24, 2)                # w, h, spp
VIEWS = (24, 16, 4, 2)                # w, h, spp, chunk
VIEW_SEEDS = [7, 0xDEADBEEF]
RADIANCE_AD = Adaptive(2, 6, 1, 0.3, 0.05)
RENDER_AD = Adaptive(2, 4, 1, 0.3, 0.05)


def tree_tuple(ti):
    """what of Scene.tree_info() the fast tree's shape decides (the reference octree's part does not depend on the knobs)"""
    return tuple(ti[k] for k in ("node_count", "leaf_count", "max_leaf_prims", "max_depth", "prim_bytes", "sah_cost", "prologue_prims",
                                 "wide_node_count", "wide_max_depth"))


def commit_under(scene, variant, monkeypatch):
    """commit with the variant's environment, and leave none of it behind"""
    for k in COMMIT_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    scene.commit()
    for k in COMMIT_KNOBS:
        monkeypatch.delenv(k, raising=False)
    return scene


def tree_check(scn, base, variant, tool="host_sim", extra_env=None):
    """tools/host_sim --tree-check under the variant's environment -> (its line as a dict, CompletedProcess); the line:
    nodes, leaves, depth, wide_nodes, wide_depth, prologue and max_leaf = {kind: the largest leaf of that kind}"""
    r = hs.run(hs.built(tool), ["--tree-check", scn, base], env=dict(VARIANTS[variant], **(extra_env or {})), check=False)
    if r.returncode != 0:
        return None, r
    words = r.stdout.split()
    assert words[:2] == ["tree-check", "ok:"], r.stdout
    at = words.index("max_leaf")
    out = {words[i]: int(words[i + 1]) for i in range(2, at, 2)}
    out["max_leaf"] = {words[i]: int(words[i + 1]) for i in range(at + 1, len(words), 2)}
    return out, r


# ---- the worlds ----------------------------------------------------------------------------------------------------------------
_worlds = {}


class World:
    """name, scn + base (what tools/host_sim and Scene.load_scn read), scene (committed under no knob), flat, osc, layout (the
    cluster scene's), cache"""


def world(api, oracle, load_scene, tmp_path_factory, name):
    if name in _worlds:
        return _worlds[name]
    assert not any(k in os.environ for k in COMMIT_KNOBS), "the default tree is built under no knob"
    w = World()
    w.name, w.layout = name, None
    if name == "cluster":
        d = tmp_path_factory.mktemp("cluster")
        w.scn, w.layout = make_clusterscene.write_scene(str(d))
        w.base = str(d) + "/"
        w.scene = api.Scene.load_scn(w.scn).commit()
    else:
        w.scn, w.base = os.path.join(DATA, name + ".scn"), DATA + "/"
        w.scene = load_scene(name)
    w.flat = w.scene.flatten(*RENDER[:2])
    w.osc = oracle.OracleScene(w.flat)
    w.oracle, w.api, w.cache = oracle, api, {}
    _worlds[name] = w
    return w


def cached(w, key, make):
    if key not in w.cache:
        w.cache[key] = make()
    return w.cache[key]


def variant_scene(w, variant, monkeypatch):
    """a second handle of the world's scene, committed under the variant (not uploaded); cached"""
    def make():
        return commit_under(w.api.Scene.load_scn(w.scn, w.base), variant, monkeypatch)
    return w.scene if variant == "default" else cached(w, ("scene", variant), make)


# ---- rays ----------------------------------------------------------------------------------------------------------------------
def _units(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _ball(rng, n, r):
    return _units(rng, n) * (r * rng.uniform(0, 1, (n, 1)) ** (1 / 3))


def _towards(o, target):
    d = target - o
    return np.concatenate([o, d / np.linalg.norm(d, axis=1, keepdims=True)], axis=1)


def aimed_rays(L, rng):
    """1 400 rays at what the cluster scene is for: 260 at the clusters' centres, 100 grazing its spheres, 160 along the cylinders' shared axis (half of
    them on it), 160 each at the duplicate spheres, the duplicate cylinders, the boxes' shared top face and the triangles' shared
    plane, 240 from inside the clusters"""
    cam = make_clusterscene.mt.CAM
    near_cam = lambda n: cam + rng.uniform(-1.5, 1.5, (n, 3))
    anywhere = lambda n: np.stack([rng.uniform(-2, 8, n), rng.uniform(-2, 6, n), rng.uniform(0.2, 5, n)], axis=1)
    out = []
    centres = [L["centres"][k] for k in ("sphere", "box", "cylinder", "triangle")]
    for c, n in zip(centres, (40, 100, 60, 60)):      # (the spheres get the grazing rays as well, the boxes are the most hidden)
        o = np.concatenate([near_cam(n // 2), anywhere(n // 2)])
        out.append(_towards(o, c + _ball(rng, n, 0.35)))
    # 100 rays that graze a sphere: they pass its centre at sqrt(r^2 + 1e-5 x [0, 1)), the window in which the reference's sphere
    # test reports the point of closest approach (ray.cpp:174-183), which the SPHERE_BELOW_BIT exemption of the node cull is for
    sph = [(c, r) for c, r, _ in L["spheres"]]
    o = np.concatenate([near_cam(50), anywhere(50)])
    target = np.zeros((100, 3))
    for i in range(100):
        c, r = sph[rng.integers(len(sph))]
        m = np.sqrt(r * r + 1e-5 * rng.uniform(0, 1))
        oc = c - o[i]
        D = np.linalg.norm(oc)
        e = np.cross(oc, _units(rng, 1)[0])
        target[i] = c + m * D / np.sqrt(D * D - m * m) * e / np.linalg.norm(e)
    out.append(_towards(o, target))
    base, axis = L["axis"]
    s = np.where(rng.random(160) < 0.5, rng.uniform(-1.5, -0.2, 160), rng.uniform(1.2, 2.5, 160))
    side = _units(rng, 160) * rng.uniform(0, 0.2, (160, 1))
    side[:80] = 0
    o = base + s[:, None] * axis + side
    out.append(np.concatenate([o, np.where(s[:, None] < 0, 1.0, -1.0) * axis / np.linalg.norm(axis)], axis=1))
    c, r = L["dup_sphere"]
    out.append(_towards(near_cam(100), c + _ball(rng, 100, r)))
    out.append(np.concatenate([c + _ball(rng, 60, 0.5 * r), _units(rng, 60)], axis=1))
    b, a, r = L["dup_cylinder"]
    on_axis = lambda n: b + rng.uniform(0.05, 0.95, (n, 1)) * a
    out.append(_towards(near_cam(120), on_axis(120) + _ball(rng, 120, r)))
    out.append(np.concatenate([on_axis(40) + _ball(rng, 40, 0.5 * r), _units(rng, 40)], axis=1))
    f = L["face"]
    xy = rng.uniform(f["lo"], f["hi"], (160, 2))
    xy[120:] = rng.uniform(f["lo"] - 0.03, f["hi"] + 0.03, (40, 2))      # and about its rim
    target = np.concatenate([xy, np.full((160, 1), f["z"])], axis=1)
    up = np.stack([rng.uniform(-0.4, 0.4, 160), rng.uniform(-0.4, 0.4, 160), rng.uniform(0.15, 0.6, 160)], axis=1)   # from below the light
    up[:40, 0:2] = 0                                  # straight down
    out.append(_towards(target + up, target))
    p = L["plane"]
    target = np.zeros((0, 3))
    while len(target) < 160:                          # points of the first triangle that the second one covers as well
        b = rng.dirichlet((1, 1, 1), 400)
        q = b @ np.asarray(p["t1"], np.float64)
        target = np.concatenate([target, q[_inside_triangle(q, p["t2"])]])[:160]
    out.append(_towards(near_cam(160), target))
    for k, c in enumerate(centres):                   # from inside; among the shells of the spheres, which are 0.40 to 0.46 from their centre
        o = c + (_units(rng, 60) * rng.uniform(0.38, 0.47, (60, 1)) if k == 0 else _ball(rng, 60, 0.3))
        out.append(np.concatenate([o, _units(rng, 60)], axis=1))
    rays = np.concatenate(out).astype("<f4")
    assert len(rays) == N_RAYS - N_MIXED_CLUSTER
    return rays


def ray_set(name, layout, cast):
    """a scene's 2 000 rays: the mixed set of tests/test_gpu_raycast.py, cast(rays) -> t placing its surface starts (the oracle in
    the tests, the reference where tests/golden/make_golden.py records the fixture); on the cluster scene 600 of those and the
    1 400 aimed ones"""
    if name == "cluster":
        mixed, _ = raycast_cases.mixed_rays(cast, "tree shapes cluster", N_MIXED_CLUSTER)
        rays = np.concatenate([mixed, aimed_rays(layout, np.random.default_rng(zlib.crc32(b"tree shapes aimed")))])
    else:
        rays, _ = raycast_cases.mixed_rays(cast, "tree shapes " + name, N_RAYS)
    assert rays.shape == (N_RAYS, 6)
    return rays


def rays_of(w):
    """the scene's rays and the oracle's closest hits -> (rays, t, n, mat)"""
    def make():
        rays = ray_set(w.name, w.layout, lambda r: w.osc.raycast(r[:, 0:3], r[:, 3:6])[0])
        return (rays,) + tuple(w.osc.raycast(rays[:, 0:3], rays[:, 3:6]))
    return cached(w, "rays", make)


def _inside_triangle(p, tri):
    a, b, c = [np.asarray(x, np.float64) for x in tri]
    n = np.cross(b - a, c - a)
    s = [np.einsum("ij,j->i", np.cross(q - r, p - r), n) for q, r in ((b, a), (c, b), (a, c))]
    return (s[0] >= 0) & (s[1] >= 0) & (s[2] >= 0)


def coplanar_hits(w):
    """-> (rays whose oracle hit lies on the two boxes' shared top face, where both have it; rays whose hit lies in the two
    triangles' shared plane, inside both)"""
    rays, t, _, mat = rays_of(w)
    L = w.layout
    hit = mat != 0
    p = rays[:, 0:3].astype(np.float64) + np.where(hit, t, 0).astype(np.float64)[:, None] * rays[:, 3:6]
    f = L["face"]
    on_face = hit & np.isin(mat, make_clusterscene.MAT_BOX_FACE) & (np.abs(p[:, 2] - f["z"]) < 1e-4) & \
        (p[:, 0:2] >= f["lo"]).all(axis=1) & (p[:, 0:2] <= f["hi"]).all(axis=1)
    pl = L["plane"]
    in_plane = hit & np.isin(mat, (make_clusterscene.MAT_MESH_A, make_clusterscene.MAT_MESH_B)) & (np.abs((p - pl["p"]) @ pl["n"]) < 1e-4) & \
        _inside_triangle(p, pl["t1"]) & _inside_triangle(p, pl["t2"])
    return on_face, in_plane


def assert_cluster_conditions(w):
    """The ray set cannot miss its purpose, from the oracle's hits alone: half of the rays end on a cluster shape, 50 on each
    pair of duplicates, 50 on each pair of coplanar faces."""
    assert w.name == "cluster"
    _, _, _, mat = rays_of(w)
    mc = make_clusterscene
    assert (mat >= mc.MAT_SPH_GLASS).sum() >= N_RAYS // 2, (mat >= mc.MAT_SPH_GLASS).sum()
    assert np.isin(mat, mc.MAT_SPH_DUP).sum() >= 50, np.bincount(mat, minlength=mc.N_MATERIALS)
    assert np.isin(mat, mc.MAT_CYL_DUP).sum() >= 50, np.bincount(mat, minlength=mc.N_MATERIALS)
    on_face, in_plane = coplanar_hits(w)
    assert on_face.sum() >= 50 and in_plane.sum() >= 50, (on_face.sum(), in_plane.sum())
    for kind_mats in ((mc.MAT_SPH_GLASS, mc.MAT_SPH_DIFF, mc.MAT_SPH_SPEC), (mc.MAT_BOX_GLASS, mc.MAT_BOX_DIFF), (mc.MAT_CYL_DIFF, mc.MAT_CYL_SPEC),
                      (mc.MAT_MESH_A,)):
        assert np.isin(mat, kind_mats).sum() >= 100, kind_mats   # every cluster is hit


def occluded_limits(t):
    """per ray the oracle's hit distance, in turn as it is, one float below and one float above"""
    k = np.arange(len(t)) % 3
    with np.errstate(over="ignore"):
        return np.where(k == 0, t, np.where(k == 1, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf)))).astype("<f4")


def golden(name):
    return np.load(os.path.join(GOLDEN, name))


# ---- the oracle's answers --------------------------------------------------------------------------------------------------------
def oracle_render(w, width, height, spp, policy, chunk, cam=None, seed=SEED):
    def make():
        w.osc.set_camera(cam if cam is not None else w.scene.camera(width, height))
        return w.osc.render(width, height, spp, seed, policy, chunk=max(chunk, 1), threads=16)
    return cached(w, ("render", width, height, spp, policy, chunk, seed, None if cam is None else np.asarray(cam).tobytes()), make)


def radiance_cases_of(w):
    return cached(w, "radiance cases", lambda: radiance_cases.mixed("tree shapes " + w.name, w.flat, w.osc, N_RADIANCE))


def radiance_expected(w):
    return cached(w, "radiance", lambda: radiance_cases.expected_of(w.osc, radiance_cases_of(w), [RADIANCE_SPP], 0.8)[RADIANCE_SPP])


def radiance_adaptive_expected(w):
    from adaptive_cases import expected
    return cached(w, "radiance adaptive", lambda: expected(w.osc, radiance_cases_of(w), RADIANCE_AD, 0.8))


def points_of(w, n=N_POINTS):
    """the scene's 256 points (p, n) with their seeds; the host's tests take the first 200 of them"""
    pts = cached(w, "points", lambda: irradiance_cases.point_set("tree shapes " + w.name, w.flat, w.osc, N_POINTS))
    return pts if n == N_POINTS else pts.take(np.arange(n))


def irradiance_expected(w, n=N_POINTS):
    """identity I2 of irradiance_cases (rr = 0), from the oracle alone"""
    def make():
        pts = points_of(w)
        return irradiance_cases.expected_from(irradiance_cases.chain_closed_form(w.oracle, w.osc, w.flat, pts, IRR_SPP), pts, IRR_SPP)
    rgb, fin = cached(w, "irradiance", make)
    return rgb[:n], fin[:n]


def _ao_table(w):
    def make():
        t = ao_cases.World()
        t.pts = points_of(w)
        t.d, t.t, t.mat, t.after = ao_cases.sample_table(w.oracle, w.osc, t.pts, AO_SPP)
        return t
    return cached(w, "ao table", make)


def ao_radius(w):
    """per point the oracle's hit distance of one of its own samples, in turn as it is, one float below and one float above"""
    t = _ao_table(w).t[np.arange(N_POINTS), np.arange(N_POINTS) % AO_SPP]
    return occluded_limits(t)


def ao_expected(w, radius, n=N_POINTS):
    return tuple(x[:n] for x in ao_cases.expected(_ao_table(w), radius, AO_SPP))


def features_expected(w):
    def make():
        width, height, spp = FEATURES
        cam = w.scene.camera(width, height)
        return feature_cases.expected(feature_cases.frame(w.oracle, w.osc, w.flat, cam, width, height, SEED, spp), spp)
    return cached(w, "features", make)


FOLLOW = (0.5, 64)                    # rr, cap of the follow render at FEATURES' frame: nothing reaches the cap
FOLLOWING_SCENES = ("glass_room", "c2_analytic")


def follow_chain(w):
    """follow_cases.chain of FEATURES' frame from the scene's own camera: the follow render's reference, which knows no variant"""
    import follow_cases
    def make():
        width, height, spp = FEATURES
        return follow_cases.chain(w.oracle, w.osc, w.flat, w.scene.camera(width, height), width, height, SEED, spp, FOLLOW[0], FOLLOW[1])
    return cached(w, "follow chain", make)


def follow_expected(w):
    import follow_cases
    return cached(w, "follow", lambda: follow_cases.expected(follow_chain(w)))


def assert_follow_conditions(w):
    """on the scenes with mirrors and glass at least a tenth of the samples are followed and some path bounces twice: the bounce
    rays, which start on a surface and so are the fast walk's own, are there to walk whatever tree the variant builds"""
    c = follow_chain(w)
    print("%s follow: followed %.3f of the samples, deepest b %d, %d rays for %d samples" % (w.name, c.followed / c.samples, c.max_b, c.rays, c.samples))
    assert c.at_cap == 0
    if w.name in FOLLOWING_SCENES:
        assert c.followed >= 0.10 * c.samples and c.max_b >= 2


def view_cams(w):
    """two cameras: the scene's own pose moved towards the middle of the scene and yawed (views_cases.MOVES 1 and 2)"""
    def make():
        width, height = VIEWS[:2]
        return np.stack([w.api.camera_from_pose(p, q, r, width, height) for p, q, r in views_cases.poses(w.scene, w.flat)[1:3]])
    return cached(w, "view cams", make)


def pixel_chains(w):
    """render_adaptive_cases.chains of the whole VIEWS frame from the scene's own camera, four samples a pixel"""
    def make():
        width, height = VIEWS[:2]
        w.osc.set_camera(w.scene.camera(width, height))
        return rac.chains(w.osc, width, height, SEED, rac.RR, spp=RENDER_AD.max_spp)
    return cached(w, "pixel chains", make)


def render_adaptive_expected(w):
    return cached(w, "render adaptive", lambda: rac.expected_from(pixel_chains(w), VIEWS[0], VIEWS[1], RENDER_AD))


MAP_CAP = 4   # the chains' length


def light_groups_of(w):
    """-> ({light material: group}, G): one group per light material, in material order; past eight they share the last"""
    lights = [int(m) for m in np.nonzero(w.flat.materials["is_light"])[0]]
    groups = {m: min(g, lg.MAX_GROUPS - 1) for g, m in enumerate(lights)}
    return groups, max(groups.values()) + 1


def group_table(w, filler=0x5A):
    t = np.full(len(w.flat.materials), filler, np.uint8)
    for m, g in light_groups_of(w)[0].items():
        t[m] = g
    return t


def light_groups_expected(w):
    """-> (frames (G, h, w, 3), rgb (h, w, 3), states (h, w)) at VIEWS' frame and spp: frame g is the oracle's PIXEL render of the
    dark twin that keeps group g (light_groups_cases.dark_twin of w.flat), rgb its render of the scene, the states its chains'"""
    def make():
        width, height, spp, _ = VIEWS
        groups, G = light_groups_of(w)
        cam = w.scene.camera(width, height)
        frames = []
        for g in range(G):
            twin = lg.dark_twin(w.oracle, w.flat, [m for m, k in groups.items() if k == g])
            twin.set_camera(cam)
            frames.append(twin.render(width, height, spp, SEED, "pixel", rr=lg.RR, threads=8)[0])
        rgb, _ = oracle_render(w, width, height, spp, "pixel", 0)
        states = np.zeros((height, width), "<u4")
        for (x, y), (_, st) in pixel_chains(w).items():
            states[y, x] = st[spp - 1]
        return np.stack(frames), rgb, states
    return cached(w, "light groups", make)


def sample_map_expected(w):
    """sample_map_cases.mixed_map() at cap 4 -> (the map, (rgb, m2, states)) from the oracle's chains"""
    assert (sm.W, sm.H) == VIEWS[:2]
    return cached(w, "sample map", lambda: (sm.mixed_map(), sm.expected_from(pixel_chains(w), sm.mixed_map(), MAP_CAP)))


class AccumulateCase:
    """what accumulate_cases' calls and sample_map_cases.chains take of a case, of a world and one of its scene handles"""

    def __init__(self, w, scene):
        self.name, self.scene, self.osc = "tree shapes " + w.name, scene, w.osc

    def twin(self, keep):
        assert keep is None
        return self.osc

    def camera(self, size=None):
        return self.scene.camera(*(size if size else VIEWS[:2]))


ACCUMULATE_CAPS = (1, 3)   # two passes under the mixed map: MAP_CAP = 4 is the chains' length


def accumulate_passes(w, call, what):
    """two accumulating passes under sample_map_cases.mixed_map(), caps 1 and 3, through `call` (accumulate_cases.host_call's or
    library_call's, at SEED) against pixel_chains folded by accumulate_cases.model, every plane after each pass -> the planes"""
    import accumulate_cases as acs
    assert sum(ACCUMULATE_CAPS) == MAP_CAP and (acs.W, acs.H) == VIEWS[:2]
    smap = sm.mixed_map()
    got, want = acs.Planes(), acs.Planes()
    for cap in ACCUMULATE_CAPS:
        paths = call(got, smap, cap, seed=SEED)
        asked = acs.model(want, 0, pixel_chains(w), smap, cap, None)
        assert paths in (None, asked) and asked > 0
        acs.assert_planes(got, want, "%s accumulate: after the pass at cap %d" % (what, cap))
    assert len(np.unique(got.count)) >= 4
    return got
