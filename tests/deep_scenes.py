"""The deep scene (tools/make_deepscene.py) for the CPU and the GPU tests of the traversal stack's scratch tail: the scene
both ways (arrays for the library, .scn + PLY for tools/host_sim), the ray sets, the oracle's answers -- computed once per
session and left unchanged -- and the conditions that make a wrong stack entry visible, checked from the oracle's hits and
the host probe alone (tools/host_sim prints, per instantiation of traverse, how deep its stack got)."""
import os
import sys

import numpy as np

import ao_cases
import host_sim_tool as hs
import irradiance_cases
import radiance_cases
from views_cases import quat_mul
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_deepscene  # noqa: E402
import make_tablescene  # noqa: E402

N_RAYS = 4000
N_RADIANCE = 500
N_POINTS = 500
AO_SPP = 4
GRAZE_B = 0.01   # the grazing camera's height ratio: the frame spans twice the outer tenth of the cylinder's silhouette
RENDER = (24, 16, 4, 2)       # the host's frame: w, h, spp, chunk
GPU_RENDER = (64, 48, 4, 2)
SEED = 4242
VIEW_SEEDS = [2024, 0xDEADBEEF]
TOOLS = ("host_sim", "host_sim_w5")   # the four-waves split of the stack (24 + 40) and the five-waves unit's (20 + 44)

_world = {}


class World:
    pass


def world(api, oracle, tmp_path_factory):
    """the scene, committed, with everything the tests share"""
    if "w" in _world:
        return _world["w"]
    w = World()
    d = tmp_path_factory.mktemp("deepscene")
    w.dir, w.base = str(d), str(d) + "/"
    w.scn, w.layout = make_deepscene.write_scene(w.dir)
    args, _ = make_deepscene.arrays()
    w.scene = api.Scene.from_arrays(**args).commit()
    w.flat = w.scene.flatten(GPU_RENDER[0], GPU_RENDER[1])
    w.osc = oracle.OracleScene(w.flat, with_reference_csg=True)
    w.rays, w.graze, rng = ray_sets(w.layout)
    w.t, w.n, w.mat = w.osc.raycast(w.rays[:, 0:3], w.rays[:, 3:6])
    w.graze_hits = w.osc.raycast(w.graze[:, 0:3], w.graze[:, 3:6])
    # pinholes for the radiance queries: in front of the inner stack, looking down the same cone
    p = np.concatenate([rng.uniform(1, 8, (N_RADIANCE, 1)), rng.uniform(0.5, 3, (N_RADIANCE, 2)) * rng.choice([-1, 1], (N_RADIANCE, 2))], axis=1)
    z = -np.concatenate([np.ones((N_RADIANCE, 1)), rng.uniform(-1, 1, (N_RADIANCE, 2)) * [1 / 3, 1 / 4]], axis=1)
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    w.cams = np.stack([p, z], axis=1).astype("<f4")
    w.prays = np.array([np.concatenate(radiance_cases.pinhole(p_, z_)) for p_, z_ in w.cams], "<f4")
    w.pseeds = rng.integers(1, 1 << 32, N_RADIANCE, dtype=np.uint64).astype("<u4")
    # points for the irradiance and ambient-occlusion queries: in front of the inner stack, their normals about +x
    pp = np.concatenate([rng.uniform(1, 8, (N_POINTS, 1)), rng.uniform(-3, 3, (N_POINTS, 2))], axis=1)
    nn = np.concatenate([np.ones((N_POINTS, 1)), rng.uniform(-0.3, 0.3, (N_POINTS, 2))], axis=1)
    nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    pts = np.concatenate([pp, nn], axis=1).astype("<f4")
    assert irradiance_cases.in_domain(pts).all()
    w.points = irradiance_cases.Points(pts, rng.integers(1, 1 << 32, N_POINTS, dtype=np.uint64).astype("<u4"), np.ones(N_POINTS, bool), np.zeros(N_POINTS, bool))
    w.oracle = oracle
    # the same scene under a camera that looks at the silhouette of the third cylinder (the one nearly along x) near its end,
    # where most rays that reach it draw a verdict other than CH_ADMIT: its frame's rays are re-traversed by resolve_hit
    w.graze_scn = write_graze_scene(w.scn, w.layout, w.dir)
    w.graze_scene = api.Scene.load_scn(w.graze_scn)   # for its camera, as the loader reads it
    w.cache = {}
    _world["w"] = w
    return w


def ray_sets(layout):
    """-> (the cone rays, the grazing rays, the generator as they leave it): what world() casts, from the layout alone"""
    rng = np.random.default_rng(5)
    slope = rng.uniform(-1, 1, (N_RAYS, 2)) * [1 / 3, 1 / 4]     # the 4:3 frame of the scene's camera
    rays = np.zeros((N_RAYS, 6), "<f4")
    rays[:, 1:3] = rng.uniform(-2, 2, (N_RAYS, 2))
    rays[:, 3], rays[:, 4:6] = 1, slope
    rays[:, 3:6] /= np.linalg.norm(rays[:, 3:6].astype(np.float64), axis=1, keepdims=True)   # the queries take unit directions
    return rays, grazing_rays(layout, rng, N_RAYS), rng


def write_graze_scene(scn, layout, directory):
    """the .scn next to scn with the grazing camera in place of the scene's own -> its path (the PLY files are shared)"""
    b, a, r = [np.asarray(v, np.float64) for v in layout["cylinders"][2]]
    c = b + 0.1 * a
    side = np.cross(a, c)
    d = c + 0.9 * float(r) * side / np.linalg.norm(side)
    z = -d / np.linalg.norm(d)
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    qw, qx, qy, qz = make_tablescene._quat_wxyz(np.stack([x, np.cross(z, x), z], axis=1))
    text = open(scn).read().splitlines()
    cam = [i for i, l in enumerate(text) if l.startswith("camera ")]
    assert len(cam) == 1
    text[cam[0]] = "camera 0. 0. 0. b %g q %.9f %.9f %.9f %.9f" % (GRAZE_B, qw, qx, qy, qz)
    path = os.path.join(directory, "deepscene_graze.scn")
    open(path, "w").write("\n".join(text) + "\n")
    return path


def grazing_rays(layout, rng, n):
    """rays from about the origin at the outer fifth of the silhouette of the third cylinder (the one nearly along x), near its two
    ends: the reference's boxes miss the cylinder they hold, most rays that reach it there draw a verdict other than CH_ADMIT
    and are traversed a second time by resolve_hit"""
    b, a, r = [np.asarray(v, np.float64) for v in layout["cylinders"][2]]
    out = np.zeros((n, 6), "<f4")
    for i in range(n):
        c = b + (rng.choice([0.1, 0.9]) + rng.uniform(-0.08, 0.08)) * a
        side = np.cross(a, c)
        p = c + float(r) * rng.uniform(0.8, 0.999) * side / np.linalg.norm(side)
        o = np.array([0.0, rng.uniform(-2, 2), rng.uniform(-2, 2)])
        out[i, 0:3], out[i, 3:6] = o, (p - o) / np.linalg.norm(p - o)
    return out


def cached(w, key, make):
    if key not in w.cache:
        w.cache[key] = make()
    return w.cache[key]


def oracle_render(w, width, height, spp, policy, chunk, cam=None, seed=SEED):
    def make():
        w.osc.set_camera(cam if cam is not None else w.scene.camera(width, height))
        return w.osc.render(width, height, spp, seed, policy, chunk=max(chunk, 1), threads=16)
    return cached(w, ("render", width, height, spp, policy, chunk, seed, None if cam is None else cam.tobytes()), make)


def view_cams(api, w, width, height):
    """the scene's own camera, and one that stands off the axis inside the cone, yawed by ten degrees"""
    qw, qx, qy, qz = make_deepscene.CAM_Q_WXYZ
    a = np.radians(10.0) / 2
    q = quat_mul(np.array([0.0, 0.0, np.sin(a), np.cos(a)]), np.array([qx, qy, qz, qw])).astype("<f4")
    return np.stack([w.scene.camera(width, height), api.camera_from_pose((2000.0, 500.0, -300.0), q, make_deepscene.CAM_RATIO, width, height)])


def radiance_expected(w, spp, rr=0.8):
    return cached(w, ("radiance", spp, rr), lambda: radiance_cases.expected(w.osc, w.cams, w.pseeds, spp, rr))


def host_render_counters(w, camera, width, height, spp, policy, chunk, env=None):
    """the work counters of tools/host_sim's render of that frame (camera: cone or grazing): rays, paths, fallback"""
    def make():
        args, _ = hs.render_args(w.dir, w.scn if camera == "cone" else w.graze_scn, width, height, spp, SEED, policy, chunk, w.base)
        return hs.counters(hs.run(hs.built(TOOLS[0]), args, env=env, threads=8))
    return cached(w, ("host render", camera, width, height, spp, policy, chunk, repr(env)), make)


def graze_cam(w, width, height):
    return w.graze_scene.camera(width, height)


def irradiance_expected(w, spp, rr=0.8):
    """identity I1 of irradiance_cases: a chain of host_sim's radiance samples (which test_deep_stack_host.py holds against the
    oracle) along the oracle's drawn directions"""
    def make():
        rad = lambda rays, seeds: hs.radiance(hs.built(TOOLS[0]), w.dir, w.scn, rays, seeds, 1, rr, w.base, threads=8)
        return irradiance_cases.expected_from(irradiance_cases.chain_by_radiance(w.oracle, w.points, spp, rad), w.points, spp)
    return cached(w, ("irradiance", spp, rr), make)


def _ao_table(w):
    def table():
        t = ao_cases.World()
        t.pts = w.points
        t.d, t.t, t.mat, t.after = ao_cases.sample_table(w.oracle, w.osc, w.points, AO_SPP)
        return t
    return cached(w, "ao table", table)


def ao_radius(w):
    """per point the oracle's hit distance of one of its own samples, in turn as it is, one float below and one float above: the
    strict < of the lane decides that sample, and about half of the others lie on either side"""
    t = _ao_table(w).t[np.arange(N_POINTS), np.arange(N_POINTS) % AO_SPP]
    k = np.arange(N_POINTS) % 3
    return np.where(k == 0, t, np.where(k == 1, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(np.inf)))).astype("<f4")


def ao_expected(w, radius):
    """ao_cases.expected over the oracle's closest hits along the drawn directions; radius: None or ao_radius(w)"""
    return ao_cases.expected(_ao_table(w), radius, AO_SPP)


def probes(w, rays="rays"):
    """{tool: (the stack probe of a --raycast run over the ray set (rays) or the grazing set (graze), its counters)}"""
    def make():
        out = {}
        for tool in TOOLS:
            _, r = hs.raycast(hs.built(tool), w.dir, w.scn, getattr(w, rays), base=w.base, threads=8)
            out[tool] = (hs.stack_probe(r), hs.counters(r))
        return out
    return cached(w, "probes " + rays, make)


def winners(w):
    """from the oracle's closest hits -> (inner, outer, far: bool per ray; the number of distinct winning triangles).  A sheet is
    told from its neighbours by where along x the hit is; far: on a cylinder, or past the nearest point of one"""
    L = w.layout
    px = w.rays[:, 0].astype(np.float64) + w.t.astype(np.float64) * w.rays[:, 3]
    inner, outer = w.mat == make_deepscene.MAT_INNER, w.mat == make_deepscene.MAT_OUTER
    near = min(float(min(b[0], b[0] + a[0]) - r) for b, a, r in L["cylinders"])
    far = (w.mat == make_deepscene.MAT_CYL) | (px >= near)
    sheets = set(np.rint(px[inner]).astype(np.int64).tolist())
    assert np.abs(px[inner] - np.rint(px[inner])).max() < 0.05 and sheets <= set(L["xs_inner"].tolist())
    plates = set(np.abs(np.log(px[outer][:, None] / L["xs_outer"][None, :])).argmin(axis=1).tolist())
    return inner, outer, far, len(sheets) + len(plates)


def assert_conditions(w):
    """What puts the tested code on the scratch half of the stack, and makes a wrong entry change an answer."""
    ti = w.scene.tree_info()
    assert ti["max_depth"] >= 30, ti
    assert ti["wide_node_count"] > 0 and 3 * ti["wide_max_depth"] > 24, ti
    assert (w.mat != 0).all(), "the room is closed: every ray has an answer"
    inner, outer, far, distinct = winners(w)
    assert inner.mean() >= 0.25 and outer.mean() >= 0.10 and far.mean() >= 0.02 and distinct >= 100, \
        (inner.mean(), outer.mean(), far.mean(), distinct)
    for tool, (probe, counters) in probes(w).items():
        main, again = probe[0], probe[1]
        assert again["lds"] == main["lds"] - 4, (tool, probe)           # resolve_hit's re-traversal
        assert main["traversals"] == counters["rays"] == len(w.rays)    # no ray is left out
        assert main["deepest"] >= main["lds"] + 4, (tool, probe)
        assert main["above"] >= len(w.rays) // 2 and main["scratch_pops"] >= len(w.rays), (tool, probe)
        assert again["above"] >= 32 and again["scratch_pops"] >= 32, (tool, probe)
        assert counters["fallback"] * 20 <= counters["rays"], (tool, counters)   # the fast path is what is tested
    assert probes(w)[TOOLS[0]][0][0]["lds"] > probes(w)[TOOLS[1]][0][0]["lds"]   # two splits of the stack
    for tool, (probe, counters) in probes(w, "graze").items():   # the grazing set: a quarter of it re-traversed, in scratch
        assert probe[1]["traversals"] >= len(w.graze) // 4 and probe[1]["above"] >= len(w.graze) // 4, (tool, probe)
        assert counters["fallback"] * 20 <= counters["rays"], (tool, counters)


# ---- the light-group and sample-map renders: the host's frame, 4 spp ---------------------------------------------------------------
LIGHT_GROUPS = (8, 5)   # G, and the group the scene's one light material is in: seven frames stay +0
MAP_CAP = 4


def light_material(w):
    lights = np.nonzero(w.flat.materials["is_light"])[0]
    assert len(lights) == 1
    return int(lights[0])


def group_table(w, filler=0x5A):
    """a byte per material: the light's group, a filler the call must not read for every other material"""
    t = np.full(len(w.flat.materials), filler, np.uint8)
    t[light_material(w)] = LIGHT_GROUPS[1]
    return t


def pixel_chains(w):
    """render_adaptive_cases.chains of the host's whole frame, four samples a pixel, from the scene's own camera"""
    import render_adaptive_cases as rac
    width, height, spp, _ = RENDER

    def make():
        w.osc.set_camera(w.scene.camera(width, height))
        return rac.chains(w.osc, width, height, SEED, rac.RR, spp=spp)
    return cached(w, "pixel chains", make)


def light_groups_expected(w):
    """-> (frames (8, h, w, 3), rgb (h, w, 3), states (h, w)): the light's frame and out_rgb are the oracle's PIXEL render of the
    scene, the states its one-pixel jobs', every other frame +0"""
    width, height, spp, _ = RENDER
    img, _ = oracle_render(w, width, height, spp, "pixel", 0)
    states = np.zeros((height, width), "<u4")
    for (x, y), (_, st) in pixel_chains(w).items():
        states[y, x] = st[spp - 1]
    frames = np.zeros((LIGHT_GROUPS[0], height, width, 3), "<f4")
    frames[LIGHT_GROUPS[1]] = img
    return frames, img, states


def sample_map_expected(w):
    """sample_map_cases.mixed_map() at cap 4 -> (the map, (rgb, m2, states)): the oracle's chains cut at the map's counts"""
    import sample_map_cases as sm
    assert (sm.W, sm.H) == RENDER[:2]
    smap = sm.mixed_map()
    return smap, sm.expected_from(pixel_chains(w), smap, MAP_CAP)
