"""Feature renders that follow mirrors and glass on the device (ort_render_follow, ort_render_views_follow and their device forms;
kernels follow_pixels): all seven planes bit for bit the references of tests/follow_cases.py -- the numpy chain from the oracle
alone, which tests/test_follow_host.py pins against the oracle's own render of the diffuse twin -- on frames of 24 x 16 (8 x 8
blocks partial in both directions) at spp 1 and 5; the six identities of include/ort.h; the rect and the guard words; the cap and
the roulette's ends; the kernels without LDS tables; the stack in its scratch tail; the forced exact walk; job batches;
counters; more jobs than resident lanes."""
import numpy as np
import pytest

import feature_cases as fc
import follow_cases as fw

pytestmark = pytest.mark.gpu

RR, CAP = 0.5, 64


@pytest.fixture()
def world(api, oracle, load_scene, tmp_path_factory):
    def get(name):
        w = fw.world(api, oracle, load_scene, tmp_path_factory, name)
        if w.scene.device is None:
            if api.device_count() < 1:
                pytest.fail("GPU test on a machine without a HIP device (the follow render has no CPU fallback)")
            w.scene.upload(0)
        return w
    return get


def host_call(w, spp, batch, rr=RR, cap=CAP, rect=None, want=fw.PLANES, counters=False, out=None):
    """the host forms -> ({plane: (V, h, w, ...)}, stats): the single frame as a batch of one"""
    if batch:
        return w.scene.render_views_follow(w.fcams, w.fseeds, w.size[0], w.size[1], spp, cap, rr, want=want, rect=rect, counters=counters, out=out)
    planes, st = w.scene.render_follow(w.size[0], w.size[1], spp, fw.SEED, cap, rr, want=want, rect=rect, counters=counters,
                                       out=None if out is None else {k: v[0] for k, v in out.items()})
    return {k: v[None] for k, v in planes.items()}, st


def device_call(api, w, spp, batch, rr=RR, cap=CAP, rect=None, want=fw.PLANES, counters=False, want_stats=False):
    """the device forms, with torch tensors that start as guard words, on a non-default stream"""
    import torch
    dev = torch.device("cuda", 0)
    nv = len(w.fcams) if batch else 1
    guards = fw.guard_planes((nv, w.size[1], w.size[0]), want)
    d = {k: torch.from_numpy(v.view("<i4") if v.dtype == np.dtype("<u4") else v).to(dev) for k, v in guards.items()}
    p = api.Scene.params(w.size[0], w.size[1], spp, fw.SEED, "pixel", 0, rect, rr, counters)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        ptrs = {k: t.data_ptr() for k, t in d.items()}
        if batch:
            st = w.scene.render_views_follow_device(p, w.fcams, w.fseeds, cap, stream=stream.cuda_stream, want_stats=want_stats, **ptrs)
        else:
            st = w.scene.render_follow_device(p, cap, stream=stream.cuda_stream, want_stats=want_stats, **ptrs)
    stream.synchronize()
    return {k: t.cpu().numpy().view(fw.DTYPES[k]) for k, t in d.items()}, st


def same_bits(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        ne = np.ascontiguousarray(a[k]).view("<u4") != np.ascontiguousarray(b[k]).view("<u4")
        assert not ne.any(), "%s %s: %d of %d words differ, first at %s" % (what, k, ne.sum(), ne.size, tuple(np.argwhere(ne)[0]))


def _single(got):
    return {k: v[0] for k, v in got.items()}


# ---- all seven planes against reference 2 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", fw.SPPS)
@pytest.mark.parametrize("name", fw.SCENES)
def test_planes_are_the_references(api, world, name, spp):
    """the single frame and the batch of three (the scene's own camera on two more seeds, then pose 1), host forms and then device
    forms on a non-default stream over guard words: every bit of albedo, normal, depth, hits, bounces, the ids' material and the
    final states; the ids' shapes are ort_raycast's for the helper's last rays"""
    w = world(name)
    one, batch, ch = fw.expected_set(w, spp, RR, CAP)
    got, _ = host_call(w, spp, False)
    fw.assert_same(_single(got), one, "%s single spp %d" % (name, spp))
    gotb, _ = host_call(w, spp, True)
    fw.assert_same(gotb, batch, "%s batch spp %d" % (name, spp))
    hits, _ = w.scene.raycast(np.concatenate([c.last for c in ch]))
    fw.assert_prims(np.concatenate([got["ids"], gotb["ids"]]), ch, hits["prim"], "%s spp %d" % (name, spp))
    dev, _ = device_call(api, w, spp, False)
    same_bits(dev, got, "%s single spp %d: device form vs host form" % (name, spp))
    devb, _ = device_call(api, w, spp, True)
    same_bits(devb, gotb, "%s batch spp %d: device form vs host form" % (name, spp))


@pytest.mark.parametrize("name", fw.SPECULAR_SCENES)
def test_conditions(world, name):
    """the conditions of tests/test_follow_host.py, asserted here too from the oracle's side: what the frames above must exercise"""
    w = world(name)
    fw.check_conditions(fw.chains(w, 5, 0.5, 64)[0], fw.chains(w, 5, 0.8, 2)[0], name)


# ---- the identities of include/ort.h --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fw.SCENES)
def test_identity_1_cap_0_is_the_first_hit_render(api, world, name):
    """max_bounces == 0 gives ort_render_features' six planes for any rr, bit for bit; bounces is all zero"""
    w = world(name)
    want, _ = w.scene.render_views_features(w.fcams, w.fseeds, fw.W, fw.H, 5, want=fc.PLANES)
    for rr in (0.0, 0.8, 7.0):
        got, _ = host_call(w, 5, True, rr=rr, cap=0)
        assert (got.pop("bounces") == 0).all()
        same_bits(got, want, "%s cap 0 rr %g" % (name, rr))


def test_identity_2_all_diffuse_scene(api, world):
    """a scene whose non-light materials all have a diffuse part gives ort_render_features' planes for every cap and rr"""
    w = world("c3_bunny_room")
    assert not fw.specular_only(w.flat).any()
    want, _ = w.scene.render_views_features(w.fcams, w.fseeds, fw.W, fw.H, 5, want=fc.PLANES)
    for rr, cap in ((0.5, 64), (0.8, 3), (4.0, 64)):
        got, _ = host_call(w, 5, True, rr=rr, cap=cap)
        assert (got.pop("bounces") == 0).all()
        same_bits(got, want, "bunny room cap %d rr %g" % (cap, rr))


@pytest.mark.parametrize("name", fw.SPECULAR_SCENES)
def test_identity_3_final_states_are_the_diffuse_twins(api, oracle, world, name):
    """while no sample reaches the cap, final_states are the final states of the oracle's PIXEL jobs on the diffuse twin at the same
    seed, spp and rr"""
    w = world(name)
    tw = fw.twin(oracle, w.flat)
    for spp, rr in ((5, 0.5), (5, 0.8)):
        assert all(c.at_cap == 0 for c in fw.chains(w, spp, rr, 64))
        got, _ = host_call(w, spp, True, rr=rr, cap=64, want=("hits", "states"))
        for v, (cam, seed) in enumerate(zip(w.fcams, w.fseeds)):
            want = fw.twin_states(tw, cam, fw.W, fw.H, seed, spp, rr)
            assert (got["states"][v] == want).all(), (name, spp, rr, v)


@pytest.mark.parametrize("name", fw.SPECULAR_SCENES)
def test_identity_6_the_recorded_vertex_is_the_raycast_of_the_last_ray(api, world, name):
    """spp 1: where sample 0 recorded a vertex, normal and ids are ort_raycast's n, mat, prim for the last ray of the chain, and
    depth is the helper's path length, whose last leg is that record's t"""
    w = world(name)
    _, _, ch = fw.expected_set(w, 1, RR, CAP)
    got, _ = device_call(api, w, 1, True)
    hits, _ = w.scene.raycast(np.concatenate([c.last for c in ch[1:]]))
    rec = got["hits"].reshape(-1) == 1
    ids = got["ids"].reshape(-1, 2)
    bounced = got["bounces"].reshape(-1) > 0
    assert (rec & bounced).sum() >= 5
    assert (ids[rec, 0] == hits["mat"][rec]).all() and (ids[rec, 1] == hits["prim"][rec]).all()
    assert (got["normal"].reshape(-1, 3)[rec].view("<u4") == hits["n"][rec].view("<u4")).all()
    direct = rec & ~bounced   # no bounce: the whole path is that one ray
    assert (got["depth"].reshape(-1)[direct].view("<u4") == hits["t"][direct].view("<u4")).all()
    assert (got["depth"].reshape(-1)[rec & bounced] > hits["t"][rec & bounced]).all()


# ---- the rect, the guard words, the forms ---------------------------------------------------------------------------------------
def test_rect_guards_planes_alone_and_forms(api, world):
    """rect (3, 2, 21, 13) over guard words: outside untouched in every plane, host and device form; each plane asked for alone
    gives the bits it has with all seven; host form equals device form; frame v of the batch equals the single call"""
    w = world("glass_room")
    one, batch, _ = fw.expected_set(w, 5, RR, CAP, fw.RECT, fw.GUARDS)
    inside = np.zeros((fw.H, fw.W), bool)
    inside[fw.RECT[1]:fw.RECT[3], fw.RECT[0]:fw.RECT[2]] = True
    dev_b, _ = device_call(api, w, 5, True, rect=fw.RECT)
    fw.assert_same(dev_b, batch, "rect, device form, batch")
    host_b, _ = host_call(w, 5, True, rect=fw.RECT, out=fw.guard_planes((3, fw.H, fw.W)))
    same_bits(host_b, dev_b, "host form vs device form, batch")
    dev_1, _ = device_call(api, w, 5, False, rect=fw.RECT)
    fw.assert_same(_single(dev_1), one, "rect, device form, single")
    host_1, _ = host_call(w, 5, False, rect=fw.RECT, out=fw.guard_planes((1, fw.H, fw.W)))
    same_bits(host_1, dev_1, "host form vs device form, single")
    for k in fw.PLANES:   # the guards, bit for bit, the hits' shapes included
        assert (dev_b[k][:, ~inside].view("<u4") == np.asarray(fw.GUARDS[k], fw.DTYPES[k]).view("<u4")).all(), k
    for k in fw.PLANES[:6]:
        alone, _ = device_call(api, w, 5, True, rect=fw.RECT, want=(k,))
        same_bits(alone, {k: dev_b[k]}, "plane %s alone" % k)
    for v in range(3):   # a batch is its views one call each; the scene's own camera in a batch is the single-frame call
        alone, _ = w.scene.render_views_follow(w.fcams[v:v + 1], w.fseeds[v:v + 1], fw.W, fw.H, 5, CAP, RR, want=fw.PLANES, rect=fw.RECT,
                                               out=fw.guard_planes((1, fw.H, fw.W)))
        same_bits(alone, {k: a[v:v + 1] for k, a in dev_b.items()}, "view %d alone" % v)
    own, _ = w.scene.render_views_follow(np.stack([w.fcams[2], w.own]), [1, fw.SEED], fw.W, fw.H, 5, CAP, RR, want=fw.PLANES, rect=fw.RECT,
                                         out=fw.guard_planes((2, fw.H, fw.W)))
    same_bits({k: a[1:2] for k, a in own.items()}, dev_1, "the scene's own camera in a batch vs the single-frame call")


# ---- the cap and the roulette's ends ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fw.SPECULAR_SCENES)
def test_cap_2_records_the_specular_surface(api, world, name):
    """cap 2 at rr 0.8: capped samples record the specular surface with its zero albedo"""
    w = world(name)
    one, batch, ch = fw.expected_set(w, 5, 0.8, 2)
    assert ch[0].capped_specular >= 5
    got, _ = host_call(w, 5, False, rr=0.8, cap=2)
    fw.assert_same(_single(got), one, name + " cap 2")
    gotb, _ = host_call(w, 5, True, rr=0.8, cap=2)
    fw.assert_same(gotb, batch, name + " cap 2, batch")
    spec = fw.specular_only(w.flat)
    capped = (got["ids"][0][..., 0] != 0) & spec[got["ids"][0][..., 0]]   # sample 0 recorded on a specular-only surface: only the cap does that
    assert capped.any() and (got["bounces"][0][capped] >= 2).all() and (fc.albedo_table(w.flat)[got["ids"][0][capped, 0]] == 0).all()


def test_rr_0_follows_nothing(api, world):
    """rr 0: no bounce.  Specular-only pixels have hits == 0 and their sums are +0"""
    w = world("glass_room")
    one, _, ch = fw.expected_set(w, 5, 0.0, 64)
    got, st = host_call(w, 5, False, rr=0.0, counters=True)
    fw.assert_same(_single(got), one, "rr 0")
    assert st["rays"] == fw.W * fw.H * 5 and (got["bounces"] == 0).all()
    spec = fw.specular_only(w.flat)[fc.frames(w)[0].mat].all(axis=1).reshape(fw.H, fw.W)   # every sample lands on a specular-only surface
    assert spec.sum() >= 5 and (got["hits"][0][spec] == 0).all()
    for k in ("albedo", "normal", "depth"):
        assert (got[k][0][spec].view("<u4") == 0).all(), k


# ---- the other kernels and paths ----------------------------------------------------------------------------------------------
def test_past_the_lds_table_caps(api, world):
    """a scene past the material cap (the TABS = false kernels): the materials and the lights read from HBM give the references'
    planes"""
    w = world("tables_mats_over")
    assert len(w.flat.materials) > 48
    for counters in (False, True):
        one, batch, _ = fw.expected_set(w, 5, RR, CAP)
        got, _ = host_call(w, 5, False, counters=counters)
        fw.assert_same(_single(got), one, "tables_mats_over single, counters %d" % counters)
        gotb, _ = host_call(w, 5, True, counters=counters)
        fw.assert_same(gotb, batch, "tables_mats_over batch, counters %d" % counters)


def test_stack_in_its_scratch_tail(api, world):
    """the deep scene at 8 x 8, spp 2: walks that run the per-lane stack past its LDS entries give the references' planes"""
    w = world("deep")
    one, batch, _ = fw.expected_set(w, 2, RR, CAP)
    got, _ = host_call(w, 2, False)
    fw.assert_same(_single(got), one, "deep single")
    gotb, _ = host_call(w, 2, True)
    fw.assert_same(gotb, batch, "deep batch")
    assert (one["hits"] > 0).any()


@pytest.mark.parametrize("name", ["glass_room", "c3_bunny_room"])
def test_forced_exact_walk(api, world, monkeypatch, name):
    """ORT_DEBUG_FORCE_FALLBACK=0 (every ray) and 0xf (the rays whose direction's low bits are zero): the same bits, with
    fallback_rays > 0"""
    w = world(name)
    _, batch, _ = fw.expected_set(w, 5, RR, CAP)
    base, st = host_call(w, 5, True)
    fw.assert_same(base, batch, name)
    for mask in ("0", "0xf"):
        monkeypatch.setenv("ORT_DEBUG_FORCE_FALLBACK", mask)
        got, st = host_call(w, 5, True)
        same_bits(got, base, "%s ORT_DEBUG_FORCE_FALLBACK=%s" % (name, mask))
        assert st["fallback_rays"] > 0
    monkeypatch.delenv("ORT_DEBUG_FORCE_FALLBACK")


def test_job_batches(api, world, monkeypatch):
    """ORT_JOB_BATCH in {0, 7, 128}: which lane runs which pixel cannot change a bit"""
    w = world("glass_room")
    _, batch, _ = fw.expected_set(w, 5, RR, CAP)
    for n in ("0", "7", "128"):
        monkeypatch.setenv("ORT_JOB_BATCH", n)
        got, _ = host_call(w, 5, True)
        fw.assert_same(got, batch, "ORT_JOB_BATCH=" + n)
    monkeypatch.delenv("ORT_JOB_BATCH")


def test_counters(api, world):
    """with ORT_RENDER_COUNTERS: rays = the helper's count of camera and bounce rays, paths = 0; fallback_rays and kernel_ms always
    filled; the counters kernels write the same planes"""
    w = world("c2_analytic")
    _, batch, ch = fw.expected_set(w, 5, RR, CAP, fw.RECT, fw.GUARDS)
    got, st = device_call(api, w, 5, True, rect=fw.RECT, counters=True, want_stats=True)
    fw.assert_same(got, batch, "counters")
    pixels = (fw.RECT[2] - fw.RECT[0]) * (fw.RECT[3] - fw.RECT[1])
    assert st["rays"] == sum(c.rays for c in ch[1:]) > 3 * pixels * 5 and st["paths"] == 0
    assert st["kernel_ms"] > 0 and st["node_tests"] > 0
    _, _, ch = fw.expected_set(w, 1, RR, CAP)
    _, st = host_call(w, 1, False, counters=True)
    assert st["rays"] == ch[0].rays and st["paths"] == 0 and st["kernel_ms"] > 0
    _, st = host_call(w, 1, False)
    assert st["rays"] == 0 and st["kernel_ms"] > 0 and st["fallback_rays"] >= 0


# ---- more jobs than resident lanes ------------------------------------------------------------------------------------------------
def test_more_jobs_than_resident_lanes(api, oracle, world):
    """glass_room at 1024 x 768, spp 2, rr 0.8, cap 8: 786 432 jobs, several for every resident lane.  The frame equals the same
    frame rendered as its four quadrant rects, bit for bit in every plane; a 24 x 16 rect around the glass spheres equals
    reference 2"""
    w = world("glass_room")
    big_w, big_h, spp, rr, cap = 1024, 768, 2, 0.8, 8
    whole, _ = w.scene.render_follow(big_w, big_h, spp, fw.SEED, cap, rr, want=fw.PLANES)
    quads = fw.guard_planes((big_h, big_w))
    for rect in ((0, 0, 512, 384), (512, 0, 1024, 384), (0, 384, 512, 768), (512, 384, 1024, 768)):
        w.scene.render_follow(big_w, big_h, spp, fw.SEED, cap, rr, want=fw.PLANES, rect=rect, out=quads)
    same_bits(quads, whole, "the frame vs its four quadrants")
    # the pixel of the 24 x 16 frame whose first hits are specular-only most often: its centre in the large frame, from the oracle's side
    follows = fw.specular_only(w.flat)[fc.frames(w)[0].mat].sum(axis=1).reshape(fw.H, fw.W)
    cy, cx = np.unravel_index(np.argmax(follows), follows.shape)
    x0 = min(max(int((cx + 0.5) * big_w / fw.W) - 12, 0), big_w - 24)
    y0 = min(max(int((cy + 0.5) * big_h / fw.H) - 8, 0), big_h - 16)
    rect = (x0, y0, x0 + 24, y0 + 16)
    c = fw.chain(oracle, w.osc, w.flat, w.scene.camera(big_w, big_h), big_w, big_h, fw.SEED, spp, rr, cap, rect)
    assert c.followed >= 0.10 * c.samples, (rect, c.followed)
    want = fw.expected(c)
    for k in fw.PLANES:
        if k == "ids":
            assert (whole[k][y0:y0 + 16, x0:x0 + 24, 0] == want[k][y0:y0 + 16, x0:x0 + 24, 0]).all()
        else:
            assert (whole[k][y0:y0 + 16, x0:x0 + 24].view("<u4") == want[k][y0:y0 + 16, x0:x0 + 24].view("<u4")).all(), k
