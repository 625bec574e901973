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
