"""First-hit feature renders on the device (ort_render_features, ort_render_views_features and their device forms; kernels
feature_pixels): all six planes bit for bit the references of tests/feature_cases.py -- the oracle's first hits of the camera
samples' rays, which tests/test_features_host.py pins against the oracle's own render of the emissive twin -- on frames of 24 x 16
(8 x 8 blocks partial in both directions) at spp 1 and 5; the identities of include/ort.h; the rect and the guard words; the
kernels without LDS tables; the stack in its scratch tail; the forced exact walk; job batches; counters."""
import numpy as np
import pytest

import feature_cases as fc
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

SCENES = ["c2_analytic", "c3_bunny_room", "open"]


@pytest.fixture()
def world(api, oracle, load_scene, tmp_path_factory):
    def get(name):
        w = fc.world(api, oracle, load_scene, tmp_path_factory, name)
        if w.scene.device is None:
            if api.device_count() < 1:
                pytest.fail("GPU test on a machine without a HIP device (the feature render has no CPU fallback)")
            w.scene.upload(0)
        return w
    return get


def host_call(w, spp, batch, rect=None, want=fc.PLANES, counters=False, out=None):
    """the host forms -> ({plane: (V, h, w, ...)}, stats): the single frame as a batch of one"""
    if batch:
        return w.scene.render_views_features(w.cams, w.seeds, w.size[0], w.size[1], spp, rect=rect, want=want, counters=counters, out=out)
    planes, st = w.scene.render_features(w.size[0], w.size[1], spp, fc.SEED, rect=rect, want=want, counters=counters,
                                         out=None if out is None else {k: v[0] for k, v in out.items()})
    return {k: v[None] for k, v in planes.items()}, st


def device_call(api, w, spp, batch, rect=None, want=fc.PLANES, counters=False, want_stats=False):
    """the device forms, with torch tensors that start as guard words, on a non-default stream"""
    import torch
    dev = torch.device("cuda", 0)
    nv = len(w.cams) if batch else 1
    guards = fc.guard_planes((nv, w.size[1], w.size[0]), want)
    d = {k: torch.from_numpy(v.view("<i4") if v.dtype == np.dtype("<u4") else v).to(dev) for k, v in guards.items()}
    p = api.Scene.params(w.size[0], w.size[1], spp, fc.SEED, "pixel", 0, rect, 0.8, counters)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        ptrs = {k: t.data_ptr() for k, t in d.items()}
        if batch:
            st = w.scene.render_views_features_device(p, w.cams, w.seeds, stream=stream.cuda_stream, want_stats=want_stats, **ptrs)
        else:
            st = w.scene.render_features_device(p, stream=stream.cuda_stream, want_stats=want_stats, **ptrs)
    stream.synchronize()
    return {k: t.cpu().numpy().view(fc.DTYPES[k]) for k, t in d.items()}, st


def same_bits(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        ne = np.ascontiguousarray(a[k]).view("<u4") != np.ascontiguousarray(b[k]).view("<u4")
        assert not ne.any(), "%s %s: %d of %d words differ, first at %s" % (what, k, ne.sum(), ne.size, tuple(np.argwhere(ne)[0]))


# ---- all six planes against the references ------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", fc.SPPS)
@pytest.mark.parametrize("name", SCENES)
def test_planes_are_the_references(api, world, name, spp):
    """the single frame and the batch of three posed views (the last the single frame's camera on another seed), host forms: every bit of albedo,
    normal, depth, hits, the ids' material and the final states; the ids' shapes are ort_raycast's for the helper's rays"""
    w = world(name)
    one, batch = fc.expected_set(w, spp)
    got, _ = host_call(w, spp, False)
    fc.assert_same({k: v[0] for k, v in got.items()}, one, "%s single spp %d" % (name, spp))
    gotb, _ = host_call(w, spp, True)
    fc.assert_same(gotb, batch, "%s batch spp %d" % (name, spp))
    assert (gotb["states"][2] != got["states"][0]).all() and (gotb["states"][2] != 0).all()   # the repeated camera, another seed
    rays = np.concatenate([f.rays[:, 0] for f in fc.frames(w)])
    hits, _ = w.scene.raycast(rays)
    ids = np.concatenate([got["ids"].reshape(-1, 2), gotb["ids"].reshape(-1, 2)])
    assert (ids[:, 0] == hits["mat"]).all() and (ids[:, 1] == hits["prim"]).all()


def test_inputs_earn_their_keep(api, world):
    """on the oracle's side, over the set above at spp 5: at least 5 % of the samples miss, at least 5 % of the pixels have
    0 < hits < spp, a pixel sees a light; and the ids (pinned to ort_raycast's above) name triangles, boxes, cylinders and spheres"""
    ws = [world(name) for name in SCENES]
    miss, partial, lights = fc.stats_of([f for w in ws for f in fc.frames(w)], 5)
    print("misses %.3f of the samples, partial coverage %.3f of the pixels, %d pixels see a light first" % (miss, partial, lights))
    assert miss >= 0.05 and partial >= 0.05 and lights >= 1
    kinds = set()
    for w in ws:
        ids = host_call(w, 1, True, want=("ids",))[0]["ids"].reshape(-1, 2)   # the bunny is seen from the scene's own pose: view 2
        kinds |= set((ids[ids[:, 0] != 0, 1] >> 28).tolist())
    assert kinds == {api.HIT_TRIANGLE, api.HIT_BOX, api.HIT_CYLINDER, api.HIT_SPHERE}, kinds


# ---- the identities of include/ort.h --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_identity_1_spp_1_is_the_raycast(api, world, name):
    """spp = 1: depth, normal and ids are ort_raycast_device's t, n, mat, prim for the pixel's first camera ray, bit for bit (a
    miss: the planes hold 0, 0 0 0 and 0, ORT_NO_PRIM where the record holds Flt_Max, 0 0 0, 0 and ORT_NO_PRIM)"""
    import torch
    w = world(name)
    got, _ = device_call(api, w, 1, True)
    rays = np.concatenate([f.rays[:, 0] for f in fc.frames(w)[1:]])
    dev = torch.device("cuda", 0)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays, "<f4")).to(dev)
    d_hits = torch.full((len(rays) * 24,), 0xAB, dtype=torch.uint8, device=dev)
    w.scene.raycast_device(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), want_stats=True)
    hits = d_hits.cpu().numpy().view(api.HIT_DTYPE)
    hit = hits["mat"] != 0
    assert hit.any() and (name != "open" or (~hit).any())
    ids = got["ids"].reshape(-1, 2)
    assert (ids[:, 0] == hits["mat"]).all() and (ids[:, 1] == hits["prim"]).all() and (ids[~hit, 1] == api.NO_PRIM).all()
    assert_bits_equal(got["normal"].reshape(-1, 3), hits["n"], name + " normal")
    assert_bits_equal(got["depth"].reshape(-1)[hit], hits["t"][hit], name + " depth")
    assert (got["depth"].reshape(-1)[~hit].view("<u4") == 0).all() and (got["hits"].reshape(-1) == hit).all()


@pytest.mark.parametrize("name", ["c2_analytic", "open"])
def test_identity_2_first_primary_ray_of_the_pixel_render(api, world, name):
    """ort_render_image, PIXEL, spp = 1, rr = 0: the pixel is emit of ids.mat if that material is a light, and 0 otherwise"""
    w = world(name)
    ids = host_call(w, 1, False, want=("ids",))[0]["ids"][0]
    img, _ = w.scene.render(w.size[0], w.size[1], 1, fc.SEED, "pixel", rr=0.0)
    mats = w.flat.materials
    want = np.where((mats["is_light"][ids[..., 0]] != 0)[..., None], mats["emit"][ids[..., 0]], np.float32(0)).astype("<f4")
    assert (want != 0).any()
    assert_bits_equal(img, want, name + ": the PIXEL render's first sample")


# ---- the rect, the guard words, the forms ---------------------------------------------------------------------------------------
def test_rect_guards_planes_alone_and_forms(api, world):
    """rect (3, 2, 21, 13) over guard words: outside untouched in every plane, host and device form; each plane asked for alone
    gives the bits it has with all six; host form equals device form; frame v of the batch equals the single call"""
    w = world("open")
    one, batch = fc.expected_set(w, 5, fc.RECT, fc.GUARDS)
    inside = np.zeros((fc.H, fc.W), bool)
    inside[fc.RECT[1]:fc.RECT[3], fc.RECT[0]:fc.RECT[2]] = True
    dev_b, _ = device_call(api, w, 5, True, fc.RECT)
    fc.assert_same(dev_b, batch, "rect, device form, batch")
    host_b, _ = host_call(w, 5, True, fc.RECT, out=fc.guard_planes((3, fc.H, fc.W)))
    same_bits(host_b, dev_b, "host form vs device form, batch")
    dev_1, _ = device_call(api, w, 5, False, fc.RECT)
    fc.assert_same({k: v[0] for k, v in dev_1.items()}, one, "rect, device form, single")
    host_1, _ = host_call(w, 5, False, fc.RECT, out=fc.guard_planes((1, fc.H, fc.W)))
    same_bits(host_1, dev_1, "host form vs device form, single")
    for k in fc.PLANES:   # the guards, bit for bit, the hits' shapes included
        assert (dev_b[k][:, ~inside].view("<u4") == np.asarray(fc.GUARDS[k], fc.DTYPES[k]).view("<u4")).all(), k
    for k in fc.PLANES[:5]:
        alone, _ = device_call(api, w, 5, True, fc.RECT, want=(k,))
        same_bits(alone, {k: dev_b[k]}, "plane %s alone" % k)
    for v in range(3):   # a batch is its views one call each; the scene's own camera in a batch is the single-frame call
        alone, _ = w.scene.render_views_features(w.cams[v:v + 1], w.seeds[v:v + 1], fc.W, fc.H, 5, rect=fc.RECT, want=fc.PLANES, out=fc.guard_planes((1, fc.H, fc.W)))
        same_bits(alone, {k: a[v:v + 1] for k, a in dev_b.items()}, "view %d alone" % v)
    own, _ = w.scene.render_views_features(np.stack([w.cams[0], w.own]), [1, fc.SEED], fc.W, fc.H, 5, rect=fc.RECT, want=fc.PLANES, out=fc.guard_planes((2, fc.H, fc.W)))
    same_bits({k: a[1:2] for k, a in own.items()}, dev_1, "the scene's own camera in a batch vs the single-frame call")


# ---- the other kernels and paths ----------------------------------------------------------------------------------------------
def test_past_the_lds_table_caps(api, world):
    """a scene past the material cap (the TABS = false kernels): the albedo read from HBM gives the references' planes"""
    w = world("tables_mats_over")
    assert len(w.flat.materials) > 48
    for counters in (False, True):
        one, batch = fc.expected_set(w, 5)
        got, _ = host_call(w, 5, False, counters=counters)
        fc.assert_same({k: v[0] for k, v in got.items()}, one, "tables_mats_over single, counters %d" % counters)
        gotb, _ = host_call(w, 5, True, counters=counters)
        fc.assert_same(gotb, batch, "tables_mats_over batch, counters %d" % counters)
    assert len(np.unique(one["ids"][..., 0])) > 8 and (one["ids"][..., 0] >= 48).any()   # many materials seen, some past the cap


def test_stack_in_its_scratch_tail(api, world):
    """the deep scene at 8 x 8, spp 2: walks that run the per-lane stack past its LDS entries give the references' planes"""
    w = world("deep")
    one, batch = fc.expected_set(w, 2, max_spp=2)
    got, _ = host_call(w, 2, False)
    fc.assert_same({k: v[0] for k, v in got.items()}, one, "deep single")
    gotb, _ = host_call(w, 2, True)
    fc.assert_same(gotb, batch, "deep batch")
    assert (one["hits"] > 0).any()


@pytest.mark.parametrize("name", ["c3_bunny_room", "open"])
def test_forced_exact_walk(api, world, monkeypatch, name):
    """ORT_DEBUG_FORCE_FALLBACK=0 (every ray) and 0xf (the rays whose direction's low bits are zero): the same bits, with
    fallback_rays > 0"""
    w = world(name)
    _, batch = fc.expected_set(w, 5)
    base, st = host_call(w, 5, True)
    fc.assert_same(base, batch, name)
    for mask in ("0", "0xf"):
        monkeypatch.setenv("ORT_DEBUG_FORCE_FALLBACK", mask)
        got, st = host_call(w, 5, True)
        same_bits(got, base, "%s ORT_DEBUG_FORCE_FALLBACK=%s" % (name, mask))
        assert st["fallback_rays"] > 0
    monkeypatch.delenv("ORT_DEBUG_FORCE_FALLBACK")


def test_job_batches(api, world, monkeypatch):
    """ORT_JOB_BATCH in {0, 7, 128}: which lane runs which pixel cannot change a bit"""
    w = world("c3_bunny_room")
    _, batch = fc.expected_set(w, 5)
    for n in ("0", "7", "128"):
        monkeypatch.setenv("ORT_JOB_BATCH", n)
        got, _ = host_call(w, 5, True)
        fc.assert_same(got, batch, "ORT_JOB_BATCH=" + n)
    monkeypatch.delenv("ORT_JOB_BATCH")


def test_counters(api, world):
    """with ORT_RENDER_COUNTERS: rays = frames x rect pixels x spp, paths = 0; fallback_rays and kernel_ms always filled; the
    counters kernels write the same planes"""
    w = world("open")
    _, batch = fc.expected_set(w, 5, fc.RECT, fc.GUARDS)
    got, st = device_call(api, w, 5, True, fc.RECT, counters=True, want_stats=True)
    fc.assert_same(got, batch, "counters")
    assert st["rays"] == 3 * (fc.RECT[2] - fc.RECT[0]) * (fc.RECT[3] - fc.RECT[1]) * 5 and st["paths"] == 0
    assert st["kernel_ms"] > 0 and st["node_tests"] > 0
    _, st = host_call(w, 1, False, counters=True)
    assert st["rays"] == fc.W * fc.H and st["paths"] == 0 and st["kernel_ms"] > 0
    _, st = host_call(w, 1, False)
    assert st["rays"] == 0 and st["kernel_ms"] > 0 and st["fallback_rays"] >= 0
