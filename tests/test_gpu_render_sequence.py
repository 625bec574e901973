"""Camera render calls of every kind, one after another, on one uploaded scene: the plain render (CHUNK, PIXEL and the
explicit jobs of WHOLE), a batch of views, the adaptive frame and the adaptive batch, host and device forms, two frame sizes
and ray queries in between.  They share one call path (device_render), the scene's staging buffers, its RenderView,
camera table and job counter on the device, and with the ray queries the steps around a launch and the settling of a call that
did not wait; every step is held bit for bit against the oracle, so a call that leaves something behind for the next one shows.

20 x 13 is 3 x 2 blocks of 8 x 8, partial on two edges; the rect cuts blocks on every side.  The oracle's frames and its
chains of 64 samples per pixel of the rect are computed once per scene."""
import numpy as np
import pytest

import radiance_cases as rc
import raycast_cases
import render_adaptive_cases as rac
import test_gpu_views as tv
from conftest import assert_bits_equal
from test_gpu_raycast import assert_same_hits
from test_gpu_render_adaptive import torch_planes
from views_cases import SEEDS

pytestmark = pytest.mark.gpu

W, H, RECT = tv.W, tv.H, (3, 2, 17, 9)
SW, SH = 9, 5
SEED, RR, AD = SEEDS[0], rac.RR, rac.FRAME
FILL = np.float32(7.0)
_worlds = {}


def world(api, oracle, scene, name):
    """what the oracle says for every step, once per scene: its own scene object, the views and their frames
    (test_gpu_views.reference), and {view: chains} of the rect's pixels at 20 x 13 and of the whole 9 x 5 frame"""
    if name not in _worlds:
        cams, ref = tv.reference(api, oracle, scene, name)
        osc = oracle.OracleScene(scene.flatten(W, H))
        chain = []
        for cam, seed in zip(cams, SEEDS):
            osc.set_camera(cam)
            chain.append(rac.chains(osc, W, H, seed, RR, RECT))
        osc.set_camera(scene.camera(SW, SH))
        small_chain = rac.chains(osc, SW, SH, SEED, RR)
        small, _ = osc.render(SW, SH, 3, SEED, "pixel", rr=RR)
        osc.set_camera(cams[0])
        whole, _ = osc.render(W, H, 2, SEED, "whole", rr=RR)
        # 65 rays of all four kinds, one wave and one more, and their closest hits as test_gpu_raycast.py obtains them
        some, _ = raycast_cases.mixed_rays(lambda r: osc.raycast(r[:, 0:3], r[:, 3:6])[0], name + " sequence", 80)
        assert len(some) >= 65
        hit_rays = np.ascontiguousarray(some[np.round(np.linspace(0, len(some) - 1, 65)).astype(int)])
        hits = osc.raycast(hit_rays[:, 0:3], hit_rays[:, 3:6])
        cases = rc.mixed(name, scene.flatten(W, H), osc, 40, salt=" sequence")
        rad = rc.expected_of(osc, cases, (2,), RR)[2]   # (sets the oracle's camera to each ray's pinhole: nothing after it renders)
        _worlds[name] = dict(cams=cams, ref=ref, chain=chain, small_chain=small_chain, small=small, whole=whole, cases=cases, rad=rad,
                             hit_rays=hit_rays, hits=hits)
    return _worlds[name]


def inside_rect():
    m = np.zeros((H, W), bool)
    m[RECT[1]:RECT[3], RECT[0]:RECT[2]] = True
    return m


def adaptive_frame(scene, wd, what):
    """the adaptive frame with all four planes on the rect, into guard-filled planes: the rule on the oracle's samples inside,
    the guards outside"""
    planes = [np.full((H, W, 3), rac.GUARDS[0], "<f4"), np.full((H, W), rac.GUARDS[1], "<u4"), np.full((H, W), rac.GUARDS[2], "<f4"),
              np.full((H, W), rac.GUARDS[3], "<u4")]
    got = scene.render_adaptive(W, H, AD.min_spp, AD.max_spp, AD.tolerance, AD.floor, AD.check_every, seed=SEED, rect=RECT, rr=RR,
                                want_states=True, out=planes)
    rac.assert_same(got[:4], rac.expected_from(wd["chain"][0], W, H, AD, rac.GUARDS), what)


def plain_chunk(scene, wd, what):
    """the plain CHUNK render in host form, with a rect and a pre-filled out"""
    want, _ = wd["ref"]("chunk", 4, 2, RECT)
    out = np.full((H, W, 3), FILL, "<f4")
    img, _ = scene.render(W, H, 4, SEED, "chunk", chunk=2, rect=RECT, rr=RR, out=out)
    m = inside_rect()
    assert (img[~m] == FILL).all(), what + ": pixels outside the rect were touched"
    assert_bits_equal(img[m], want[0][m], what)


@pytest.mark.parametrize("name", ["glass_room", "c3_bunny_room"])
def test_calls_of_every_kind_in_sequence(api, oracle, gpu_scene, name):
    import torch
    scene = gpu_scene(name)
    wd = world(api, oracle, scene, name)
    cams, ref = wd["cams"], wd["ref"]
    # 1. a plain CHUNK render, host form, rect, pre-filled out
    plain_chunk(scene, wd, name + " 1: plain chunk render")
    # 2. a three-view PIXEL batch
    want, _ = ref("pixel", 3, 0)
    frames, _ = scene.render_views(cams, SEEDS, W, H, 3, "pixel", rr=RR)
    for v in range(3):
        assert_bits_equal(frames[v], want[v], "%s 2: pixel batch, view %d" % (name, v))
    # 3. an adaptive frame, four planes, rect, guard-filled planes
    adaptive_frame(scene, wd, name + " 3: adaptive frame")
    # 4. the WHOLE policy: explicit jobs
    img, _ = scene.render(W, H, 2, SEED, "whole", rr=RR)
    assert_bits_equal(img, wd["whole"], name + " 4: whole policy")
    # 5. an adaptive three-view batch without states
    planes = [np.full((3, H, W, 3), rac.GUARDS[0], "<f4"), np.full((3, H, W), rac.GUARDS[1], "<u4"), np.full((3, H, W), rac.GUARDS[2], "<f4")]
    got = scene.render_views_adaptive(cams, SEEDS, W, H, AD.min_spp, AD.max_spp, AD.tolerance, AD.floor, AD.check_every, rect=RECT, rr=RR, out=planes)
    for v in range(3):
        rac.assert_same(tuple(x[v] for x in got[:3]) + (None,), rac.expected_from(wd["chain"][v], W, H, AD, rac.GUARDS),
                        "%s 5: adaptive batch, view %d" % (name, v))
    # 6. a smaller frame, plain and adaptive
    img, _ = scene.render(SW, SH, 3, SEED, "pixel", rr=RR)
    assert_bits_equal(img, wd["small"], name + " 6: 9 x 5 pixel render")
    got = scene.render_adaptive(SW, SH, AD.min_spp, AD.max_spp, AD.tolerance, AD.floor, AD.check_every, seed=SEED, rr=RR, want_states=True)
    rac.assert_same(got[:4], rac.expected_from(wd["small_chain"], SW, SH, AD), name + " 6: 9 x 5 adaptive frame")
    # 7. the 20 x 13 plain render again
    plain_chunk(scene, wd, name + " 7: plain chunk render again")
    # 8. the device forms without stats, back to back on one stream: neither call waits, the second settles the first
    dev = torch.device("cuda", 0)
    d_img = torch.full((H * W * 3,), float(FILL), dtype=torch.float32, device=dev)
    t = torch_planes((H, W), (float(rac.GUARDS[0]), rac.GUARDS[1] - (1 << 32), float(rac.GUARDS[2]), rac.GUARDS[3] - (1 << 32)))
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        assert scene.render_device(d_img.data_ptr(), scene.params(W, H, 3, SEED, "pixel", rr=RR), stream=stream.cuda_stream) is None
        assert scene.render_adaptive_device(scene.params(W, H, 0, SEED, "pixel", 0, RECT, RR), AD.min_spp, AD.max_spp, AD.tolerance, AD.floor,
                                            AD.check_every, *[x.data_ptr() for x in t], stream=stream.cuda_stream) is None
    stream.synchronize()
    assert_bits_equal(d_img.cpu().numpy().reshape(H, W, 3), want[0], name + " 8: device form, plain")
    h = [x.cpu().numpy() for x in t]
    rac.assert_same((h[0].reshape(H, W, 3), h[1].view("<u4").reshape(H, W), h[2].reshape(H, W), h[3].view("<u4").reshape(H, W)),
                    rac.expected_from(wd["chain"][0], W, H, AD, rac.GUARDS), name + " 8: device form, adaptive")
    # 9. a radiance query between two renders (it stages where the adaptive planes do), then the adaptive frame again
    img, _ = scene.render(W, H, 3, SEED, "pixel", rr=RR)
    assert_bits_equal(img, want[0], name + " 9: pixel render")
    rgb, fin, _ = scene.radiance(wd["cases"].rays, wd["cases"].seeds, 2, RR, want_states=True)
    rc.assert_same(rgb, fin, wd["rad"][0], wd["rad"][1], name + " 9: radiance query")
    adaptive_frame(scene, wd, name + " 9: adaptive frame again")
    # 10. render, closest hits, radiance, render: four device forms without stats back to back on one stream.  No call waits;
    # each settles the one before it, and all share the scene's ctrl words, RenderView and events
    cases = wd["cases"]
    d_first, d_last = (torch.full((H * W * 3,), float(FILL), dtype=torch.float32, device=dev) for _ in range(2))
    d_hit_rays = torch.from_numpy(wd["hit_rays"]).to(dev)
    d_hits = torch.full((65 * 24,), 0xAB, dtype=torch.uint8, device=dev)
    d_rays = torch.from_numpy(np.ascontiguousarray(cases.rays, "<f4")).to(dev)
    d_seeds = torch.from_numpy(np.ascontiguousarray(cases.seeds, "<u4").view("<i4")).to(dev)
    d_rgb = torch.full((40 * 3,), float(FILL), dtype=torch.float32, device=dev)
    d_fin = torch.zeros(40, dtype=torch.int32, device=dev)
    pixel = scene.params(W, H, 3, SEED, "pixel", rr=RR)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        assert scene.render_device(d_first.data_ptr(), pixel, stream=stream.cuda_stream) is None
        assert scene.raycast_device(d_hit_rays.data_ptr(), 65, d_hits.data_ptr(), stream=stream.cuda_stream) is None
        assert scene.radiance_device(d_rays.data_ptr(), d_seeds.data_ptr(), 40, 2, RR, d_rgb.data_ptr(), d_fin.data_ptr(),
                                     stream=stream.cuda_stream) is None
        assert scene.render_device(d_last.data_ptr(), pixel, stream=stream.cuda_stream) is None
    stream.synchronize()
    assert_bits_equal(d_first.cpu().numpy().reshape(H, W, 3), want[0], name + " 10: first render")
    assert_same_hits(d_hits.cpu().numpy().view(api.HIT_DTYPE), *wd["hits"], name + " 10: closest hits")
    rc.assert_same(d_rgb.cpu().numpy().reshape(40, 3), d_fin.cpu().numpy().view("<u4"), wd["rad"][0], wd["rad"][1], name + " 10: radiance query")
    assert_bits_equal(d_last.cpu().numpy().reshape(H, W, 3), want[0], name + " 10: render again")


# ---- the light-group and sample-map calls among the others ---------------------------------------------------------------------------
# device_render stages the group frames through the ray queries' ray buffer (query_stage[0]) and the sample map through their
# output buffer (query_stage[1], read-only, never staged out), and keeps the group table on the host side of the scene: a call
# that leaves something of its own there, or finds something of another's, shows in the next step
GUARD_F, GUARD_M2, GUARD_STATE = np.float32(-7.0), np.float32(-1.0), 0xDDDDDDDD
GROUP_SPP, MAP_CAP = 4, 16


def masked(got, want, guard, what, rect=RECT):
    """got (..., H, W[, 3]) equals want bit for bit inside the rect and holds guard outside it"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    m = np.zeros((H, W), bool)
    m[rect[1]:rect[3], rect[0]:rect[2]] = True
    m = m if got.shape[-1] != 3 else m[..., None]
    ne = (got.view("<u4") != want.view("<u4")) & m
    assert not ne.any(), "%s: %d words inside the rect differ; first at %r" % (what, int(ne.sum()), tuple(np.argwhere(ne)[0]))
    g = np.array(guard, got.dtype).reshape(1).view("<u4")[0]
    out = (got.view("<u4") != g) & ~m
    assert not out.any(), "%s: %d words outside the rect were written; first at %r" % (what, int(out.sum()), tuple(np.argwhere(out)[0]))


def group_world(api, oracle, scene, name, wd):
    """the oracle's part of the light-group and sample-map steps, once per scene: its PIXEL renders of the dark twins (rect, 4
    spp, the scene's own camera and seed), the maps and the planes the chains give for them, the feature planes"""
    import feature_cases as fc
    import light_groups_cases as lg
    import sample_map_cases as sm
    if "groups" in wd:
        return wd["groups"]
    g = {}
    flat = scene.flatten(W, H)
    g["lights"] = [int(m) for m in np.nonzero(flat.materials["is_light"])[0]]
    twins = {}

    def frame(keep):
        """the rect of the PIXEL render of the twin that keeps the lights of `keep`, +0 elsewhere; keep None: the scene itself"""
        key = None if keep is None else frozenset(keep)
        if key not in twins:
            osc = lg.dark_twin(oracle, flat, key)
            osc.set_camera(wd["cams"][0])
            twins[key] = osc.render(W, H, GROUP_SPP, SEED, "pixel", rect=RECT, rr=RR, threads=8)[0]
        return twins[key]

    def frames(groups, G):
        return np.stack([frame([m for m, k in groups.items() if k == i]) for i in range(G)])
    g["frame"], g["frames"] = frame, frames
    g["table"] = lambda groups: np.array([groups.get(m, lg.NO_GROUP if m in g["lights"] else 0x5A) for m in range(len(flat.materials))], np.uint8)
    states = np.zeros((H, W), "<u4")
    for (x, y), (_, st) in wd["chain"][0].items():
        states[y, x] = st[GROUP_SPP - 1]
    g["states"] = states
    g["maps"] = np.stack([sm.mixed_map(s, (W, H), rect=RECT, zero_row=5) for s in (0, 3, 6)])
    assert all((sm.counts(m, MAP_CAP)[RECT[1]:RECT[3], RECT[0]:RECT[2]] == k).any() for m in g["maps"] for k in (0, 1, MAP_CAP))
    g["map_planes"] = [sm.expected_from(wd["chain"][v], g["maps"][v], MAP_CAP, RECT, (W, H)) for v in range(3)]
    osc = oracle.OracleScene(flat)
    g["features"] = fc.expected(fc.frame(oracle, osc, flat, wd["cams"][0], W, H, SEED, 2, RECT), 2, fc.GUARDS)
    wd["groups"] = g
    return g


def map_guards(V=None):
    lead = () if V is None else (V,)
    return [np.full(lead + (H, W, 3), GUARD_F, "<f4"), np.full(lead + (H, W), GUARD_M2, "<f4"), np.full(lead + (H, W), GUARD_STATE, "<u4")]


@pytest.mark.parametrize("name", ["glass_room", "c3_bunny_room"])
def test_light_groups_and_sample_maps_in_sequence(api, oracle, gpu_scene, name):
    import torch
    import feature_cases as fc
    import sample_map_cases as sm
    scene = gpu_scene(name)
    wd = world(api, oracle, scene, name)
    g = group_world(api, oracle, scene, name, wd)
    cams, lights = wd["cams"], g["lights"]
    inside = inside_rect()

    def raycast(what):
        hits, _ = scene.raycast(wd["hit_rays"])
        assert_same_hits(hits, *wd["hits"], what)

    def light_groups(groups, G, what):
        out = [np.full((G, H, W, 3), GUARD_F, "<f4"), np.full((H, W, 3), GUARD_F, "<f4"), np.full((H, W), GUARD_STATE, "<u4")]
        frames, rgb, states, _ = scene.render_light_groups(W, H, GROUP_SPP, SEED, g["table"](groups), True, True, group_count=G, rect=RECT, rr=RR, out=out)
        masked(frames, g["frames"](groups, G), GUARD_F, what + ": group frames")
        masked(rgb, g["frame"](None), GUARD_F, what + ": out_rgb")
        masked(states, g["states"], GUARD_STATE, what + ": final states")
        return frames

    # 1. a host raycast of 65 rays: it fills the ray queries' two staging buffers
    raycast(name + " 1: closest hits")
    # 2. light groups, G = 1, host form, guard-filled planes: the group frames are staged where the rays were
    light_groups({m: 0 for m in lights}, 1, name + " 2: light groups, G = 1")
    # 3. G = 8 with empty groups: eight frames grow that buffer
    eight = {m: (6, 2)[i % 2] for i, m in enumerate(lights)}
    frames = light_groups(eight, 8, name + " 3: light groups, G = 8")
    assert not frames[[0, 1, 3, 4, 5, 7]][:, inside].view("<u4").any() and frames[6][inside].any()
    # 4. a sample map in host form: the map is staged where the hits were
    maps = g["maps"].copy()
    got = scene.render_sample_map(W, H, maps[0], MAP_CAP, SEED, True, True, rect=RECT, rr=RR, out=map_guards())
    assert (maps == g["maps"]).all(), name + " 4: the host map was written"
    sm.assert_planes(got[:3], g["map_planes"][0], name + " 4: sample map")
    # 5. the raycast again
    raycast(name + " 5: closest hits again")
    # 6. a three-view sample-map batch, a map per view
    got = scene.render_views_sample_map(cams, SEEDS, W, H, maps, MAP_CAP, True, True, rect=RECT, rr=RR, out=map_guards(3))
    assert (maps == g["maps"]).all(), name + " 6: the host maps were written"
    for v in range(3):
        sm.assert_planes(tuple(p[v] for p in got[:3]), g["map_planes"][v], "%s 6: sample-map batch, view %d" % (name, v))
    # 7. a features render
    planes, _ = scene.render_features(W, H, 2, SEED, rect=RECT, want=fc.PLANES, out=fc.guard_planes((H, W)))
    fc.assert_same(planes, g["features"], name + " 7: features")
    # 8. the plain CHUNK render
    plain_chunk(scene, wd, name + " 8: plain chunk render")
    # 9. four device forms with stats == NULL back to back on one stream, no wait between them, each settling the one before:
    # light groups with table A, with table B (the lights' groups permuted: the table is the call's own), a sample map, a render
    G = len(lights) + 1
    table_a = {m: i for i, m in enumerate(lights)}
    table_b = {m: (i + 1) % G for i, m in enumerate(lights)}
    dev = torch.device("cuda", 0)
    n = H * W
    full = lambda k, fill, dt: torch.full((k,), fill, dtype=dt, device=dev)
    a, b = ([full(3 * n * G, float(GUARD_F), torch.float32), full(3 * n, float(GUARD_F), torch.float32), full(n, GUARD_STATE - (1 << 32), torch.int32)] for _ in range(2))
    m = [full(3 * n, float(GUARD_F), torch.float32), full(n, float(GUARD_M2), torch.float32), full(n, GUARD_STATE - (1 << 32), torch.int32)]
    d_map = torch.from_numpy(np.ascontiguousarray(maps[1]).view("<i4").reshape(-1)).to(dev)
    d_img = full(3 * n, float(FILL), torch.float32)
    p = scene.params(W, H, GROUP_SPP, SEED, "pixel", 0, RECT, RR)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        assert scene.render_light_groups_device(p, g["table"](table_a), *[x.data_ptr() for x in a], group_count=G, stream=stream.cuda_stream) is None
        assert scene.render_light_groups_device(p, g["table"](table_b), *[x.data_ptr() for x in b], group_count=G, stream=stream.cuda_stream) is None
        assert scene.render_sample_map_device(scene.params(W, H, MAP_CAP, SEED, "pixel", 0, RECT, RR), d_map.data_ptr(), *[x.data_ptr() for x in m],
                                              stream=stream.cuda_stream) is None
        assert scene.render_device(d_img.data_ptr(), scene.params(W, H, 3, SEED, "pixel", rr=RR), stream=stream.cuda_stream) is None
    stream.synchronize()
    for t, table, label in ((a, table_a, "table A"), (b, table_b, "table B")):
        h = [x.cpu().numpy() for x in t]
        masked(h[0].reshape(G, H, W, 3), g["frames"](table, G), GUARD_F, "%s 9: light groups with %s: group frames" % (name, label))
        masked(h[1].reshape(H, W, 3), g["frame"](None), GUARD_F, "%s 9: light groups with %s: out_rgb" % (name, label))
        masked(h[2].view("<u4").reshape(H, W), g["states"], GUARD_STATE, "%s 9: light groups with %s: final states" % (name, label))
    assert (d_map.cpu().numpy().view("<u4").reshape(H, W) == g["maps"][1]).all(), name + " 9: the map tensor was written"
    h = [x.cpu().numpy() for x in m]
    sm.assert_planes((h[0].reshape(H, W, 3), h[1].reshape(H, W), h[2].view("<u4").reshape(H, W)),
                     sm.expected_from(wd["chain"][0], g["maps"][1], MAP_CAP, RECT, (W, H)), name + " 9: sample map, device form")
    assert_bits_equal(d_img.cpu().numpy().reshape(H, W, 3), wd["ref"]("pixel", 3, 0)[0][0], name + " 9: plain render, device form")
    # 10. the adaptive frame
    adaptive_frame(scene, wd, name + " 10: adaptive frame")
