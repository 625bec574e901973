"""ID-matte renders on the device (ort_render_matte, ort_render_views_matte and their device forms; kernels matte_pixels) and
ort_matte_mask: every word of the five planes against the reference of tests/matte_cases.py -- a histogram over the oracle's
materials and ort_raycast's prims for the camera samples' rays -- on frames of 24 x 16 (8 x 8 blocks partial in both directions)
at spp 1 and 5, K in {1, 2, 8}, all three modes; the identities of include/ort.h against ort_render_features and ort_raycast on
the device; the rect and the guard words; the kernels without LDS tables; the stack in its scratch tail; the forced exact walk;
job batches; counters; more jobs than resident lanes; the mask against numpy, its device form between guard words."""
import numpy as np
import pytest

import feature_cases as fc
import matte_cases as mc

pytestmark = pytest.mark.gpu

MODES = ("material", "object", "prim")
GUARD = 64   # words of 0xA5A5A5A5 either side of every device buffer the mask call may write


@pytest.fixture()
def world(api, oracle, load_scene, tmp_path_factory):
    def get(name):
        w = mc.world(api, oracle, load_scene, tmp_path_factory, name)
        if w.scene.device is None:
            if api.device_count() < 1:
                pytest.fail("GPU test on a machine without a HIP device (the matte render has no CPU fallback)")
            w.scene.upload(0)
        return w
    return get


def host_call(w, spp, batch, by, k, rect=None, want=mc.PLANES[2:], counters=False, out=None):
    """the host forms -> ({plane: (V, h, w[, k])}, stats): the single frame as a batch of one"""
    if batch:
        return w.scene.render_views_matte(w.mcams, w.mseeds, w.size[0], w.size[1], spp, by, k, rect=rect, want=want, counters=counters, out=out)
    planes, st = w.scene.render_matte(w.size[0], w.size[1], spp, mc.SEED, by, k, rect=rect, want=want, counters=counters,
                                      out=None if out is None else {p: v[0] for p, v in out.items()})
    return {p: v[None] for p, v in planes.items()}, st


def device_call(api, w, spp, batch, by, k, rect=None, want=mc.PLANES[2:], counters=False, want_stats=False):
    """the device forms, with torch tensors that start as guard words, on a non-default stream"""
    import torch
    dev = torch.device("cuda", 0)
    nv = len(w.mcams) if batch else 1
    guards = mc.guard_planes((nv, w.size[1], w.size[0]), k, ("ids", "counts") + tuple(want))
    d = {p: torch.from_numpy(v.view("<i4")).to(dev) for p, v in guards.items()}
    params = api.Scene.params(w.size[0], w.size[1], spp, mc.SEED, "pixel", 0, rect, 0.8, counters)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        ptrs = {p: t.data_ptr() for p, t in d.items()}
        if batch:
            st = w.scene.render_views_matte_device(params, w.mcams, w.mseeds, by, k, stream=stream.cuda_stream, want_stats=want_stats, **ptrs)
        else:
            st = w.scene.render_matte_device(params, by, k, stream=stream.cuda_stream, want_stats=want_stats, **ptrs)
    stream.synchronize()
    return {p: t.cpu().numpy().view("<u4") for p, t in d.items()}, st


def _single(got):
    return {p: v[0] for p, v in got.items()}


# ---- every word against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by", MODES)
@pytest.mark.parametrize("name", mc.SCENES)
def test_planes_are_the_references(api, world, name, by):
    """the single frame and the batch, host forms and then device forms on a non-default stream over guard words, K in {1, 2, 8},
    spp 1 and 5: every word of ids, counts, other, hits and the final states"""
    w = world(name)
    prims = mc.device_prims(w)
    for k in mc.KS:
        for spp in mc.SPPS:
            one, batch = mc.expected_set(w, prims, by, spp, k)
            got, _ = host_call(w, spp, False, by, k)
            mc.same_bits(_single(got), one, "%s %s K %d spp %d single" % (name, by, k, spp))
            gotb, _ = host_call(w, spp, True, by, k)
            mc.same_bits(gotb, batch, "%s %s K %d spp %d batch" % (name, by, k, spp))
            if k == 2 or spp == 5:
                dev, _ = device_call(api, w, spp, False, by, k)
                mc.same_bits(dev, got, "%s %s K %d spp %d: device form vs host form" % (name, by, k, spp))
                devb, _ = device_call(api, w, spp, True, by, k)
                mc.same_bits(devb, gotb, "%s %s K %d spp %d batch: device form vs host form" % (name, by, k, spp))


# ---- the identities of include/ort.h ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.SCENES)
def test_identities(api, world, name):
    """(1) sum(counts) + other == hits, and hits and final_states are ort_render_features' planes; (2) at spp 1 slot 0 is
    ort_render_features' ids.mat (BY_MATERIAL) or ids.prim (BY_PRIM) -- which is ort_raycast's prim of the pixel's ray -- where it hit
    and EMPTY where it did not; (3) where other == 0 under both modes the BY_OBJECT counts folded through object -> material are the
    BY_MATERIAL counts; (4) frame v of a batch is the single-frame call's frame"""
    w = world(name)
    feat5, _ = w.scene.render_views_features(w.mcams, w.mseeds, mc.W, mc.H, 5, want=("hits", "states"))
    feat1, _ = w.scene.render_views_features(w.mcams, w.mseeds, mc.W, mc.H, 1, want=("hits", "ids"))
    rays = np.concatenate([f.rays[:, 0] for f in mc.frames(w)[1:]])
    cast, _ = w.scene.raycast(rays)
    hit = feat1["hits"] == 1
    assert (feat1["ids"][..., 1].reshape(-1) == cast["prim"]).all() and hit.any()
    got = {}
    for by in MODES:
        for k in (2, 8):
            g, _ = host_call(w, 5, True, by, k, want=("other", "hits", "states"))
            mc.check_order(g["ids"], g["counts"], g["other"], g["hits"])
            assert (g["hits"] == feat5["hits"]).all() and (g["states"] == feat5["states"]).all()
            got[by, k] = g
        one, _ = host_call(w, 1, True, by, 2)
        assert ((one["ids"][..., 0] == mc.EMPTY) == ~hit).all() and (one["ids"][..., 1] == mc.EMPTY).all()
        want = {"material": feat1["ids"][..., 0], "prim": feat1["ids"][..., 1]}.get(by)
        if want is None:
            want = mc.object_of_prim(w.flat, feat1["ids"][..., 1])
        assert (one["ids"][..., 0][hit] == want[hit]).all()
    ids, mats = w.scene.object_ids()
    table = dict(zip(ids.tolist(), mats.tolist()))
    for k in (2, 8):
        o, m = got["object", k], got["material", k]
        exact = (o["other"] == 0) & (m["other"] == 0)
        assert exact.any()
        for oi, oc, mi, mcnt in zip(o["ids"][exact], o["counts"][exact], m["ids"][exact], m["counts"][exact]):
            h = {}
            for x, c in zip(oi, oc):
                if x != mc.EMPTY:
                    h[table[int(x)]] = h.get(table[int(x)], 0) + int(c)
            assert h == {int(x): int(c) for x, c in zip(mi, mcnt) if x != mc.EMPTY}
    for v in range(len(w.mcams)):
        alone, _ = w.scene.render_views_matte(w.mcams[v:v + 1], w.mseeds[v:v + 1], mc.W, mc.H, 5, "object", 2, want=("other", "hits", "states"))
        mc.same_bits(alone, {p: a[v:v + 1] for p, a in got["object", 2].items()}, "view %d alone" % v)
    own, _ = w.scene.render_views_matte(np.stack([w.mcams[0], w.own]), [1, mc.SEED], mc.W, mc.H, 5, "prim", 8, want=("other", "hits", "states"))
    single, _ = host_call(w, 5, False, "prim", 8, want=("other", "hits", "states"))
    mc.same_bits({p: a[1:2] for p, a in own.items()}, single, "the scene's own camera in a batch vs the single-frame call")


# ---- the rect, the guard words, the optional planes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("by", MODES)
def test_rect_guards_and_planes_alone(api, world, by):
    """rect (3, 2, 21, 13) over guard words: outside untouched in every plane, host and device form (identity 6); other, hits and
    final_states asked for or not change no word elsewhere (identity 5)"""
    w = world("open")
    prims = mc.device_prims(w)
    inside = np.zeros((mc.H, mc.W), bool)
    inside[mc.RECT[1]:mc.RECT[3], mc.RECT[0]:mc.RECT[2]] = True
    for k in (2, 8):
        one, batch = mc.expected_set(w, prims, by, 5, k, mc.RECT, mc.GUARDS)
        dev_b, _ = device_call(api, w, 5, True, by, k, rect=mc.RECT)
        mc.same_bits(dev_b, batch, "rect, device form, batch, K %d" % k)
        host_b, _ = host_call(w, 5, True, by, k, rect=mc.RECT, out=mc.guard_planes((len(w.mcams), mc.H, mc.W), k))
        mc.same_bits(host_b, dev_b, "host form vs device form, batch")
        dev_1, _ = device_call(api, w, 5, False, by, k, rect=mc.RECT)
        mc.same_bits(_single(dev_1), one, "rect, device form, single")
        for p in mc.PLANES:
            assert (dev_b[p][:, ~inside] == mc.GUARDS[p]).all(), p
        for want in ((), ("other",), ("hits",), ("states",)):
            alone, _ = device_call(api, w, 5, True, by, k, rect=mc.RECT, want=want)
            assert set(alone) == {"ids", "counts"} | set(want)
            mc.same_bits(alone, dev_b, "planes %r alone" % (want,))


# ---- the other kernels and paths ------------------------------------------------------------------------------------------------------------
def test_past_the_lds_table_caps(api, world):
    """a scene past the material cap (the TABS = false kernels), with and without counters: the references' planes"""
    w = world("tables_mats_over")
    assert len(w.flat.materials) > 48
    prims = mc.device_prims(w)
    for counters in (False, True):
        for by, k in (("material", 8), ("object", 2), ("prim", 1)):
            one, batch = mc.expected_set(w, prims, by, 5, k)
            got, _ = host_call(w, 5, False, by, k, counters=counters)
            mc.same_bits(_single(got), one, "tables_mats_over %s single, counters %d" % (by, counters))
            gotb, _ = host_call(w, 5, True, by, k, counters=counters)
            mc.same_bits(gotb, batch, "tables_mats_over %s batch, counters %d" % (by, counters))


def test_stack_in_its_scratch_tail(api, world):
    """the deep scene at 8 x 8, spp 2: walks that run the per-lane stack past its LDS entries give the references' planes"""
    w = world("deep")
    prims = mc.device_prims(w)
    for by in MODES:
        one, batch = mc.expected_set(w, prims, by, 2, 2)
        got, _ = host_call(w, 2, False, by, 2)
        mc.same_bits(_single(got), one, "deep %s single" % by)
        gotb, _ = host_call(w, 2, True, by, 2)
        mc.same_bits(gotb, batch, "deep %s batch" % by)
        assert (one["hits"] > 0).any()


@pytest.mark.parametrize("name", ["open", "c3_bunny_room"])
def test_forced_exact_walk(api, world, monkeypatch, name):
    """ORT_DEBUG_FORCE_FALLBACK=0 (every ray) and 0xf (the rays whose direction's low bits are zero): the same words, with
    fallback_rays > 0"""
    w = world(name)
    _, batch = mc.expected_set(w, mc.device_prims(w), "object", 5, 8)
    base, _ = host_call(w, 5, True, "object", 8)
    mc.same_bits(base, batch, name)
    for mask in ("0", "0xf"):
        monkeypatch.setenv("ORT_DEBUG_FORCE_FALLBACK", mask)
        got, st = host_call(w, 5, True, "object", 8)
        mc.same_bits(got, base, "%s ORT_DEBUG_FORCE_FALLBACK=%s" % (name, mask))
        assert st["fallback_rays"] > 0
    monkeypatch.delenv("ORT_DEBUG_FORCE_FALLBACK")


def test_job_batches(api, world, monkeypatch):
    """ORT_JOB_BATCH in {0, 7, 128}: which lane runs which pixel cannot change a word"""
    w = world("open")
    _, batch = mc.expected_set(w, mc.device_prims(w), "prim", 5, 2)
    for n in ("0", "7", "128"):
        monkeypatch.setenv("ORT_JOB_BATCH", n)
        got, _ = host_call(w, 5, True, "prim", 2)
        mc.same_bits(got, batch, "ORT_JOB_BATCH=" + n)
    monkeypatch.delenv("ORT_JOB_BATCH")


def test_counters(api, world):
    """with ORT_RENDER_COUNTERS: rays = frames x rect pixels x spp, paths = 0; fallback_rays and kernel_ms always filled; the counters
    kernels write the same planes"""
    w = world("c2_analytic")
    _, batch = mc.expected_set(w, mc.device_prims(w), "object", 5, 2, mc.RECT, mc.GUARDS)
    got, st = device_call(api, w, 5, True, "object", 2, rect=mc.RECT, counters=True, want_stats=True)
    mc.same_bits(got, batch, "counters")
    pixels = (mc.RECT[2] - mc.RECT[0]) * (mc.RECT[3] - mc.RECT[1])
    assert st["rays"] == len(w.mcams) * pixels * 5 and st["paths"] == 0 and st["kernel_ms"] > 0 and st["node_tests"] > 0
    _, st = host_call(w, 1, False, "material", 1, counters=True)
    assert st["rays"] == mc.W * mc.H and st["paths"] == 0 and st["kernel_ms"] > 0
    _, st = host_call(w, 1, False, "material", 1)
    assert st["rays"] == 0 and st["kernel_ms"] > 0 and st["fallback_rays"] >= 0


# ---- more jobs than resident lanes ------------------------------------------------------------------------------------------------------
def test_more_jobs_than_resident_lanes(api, world):
    """the bunny room at 1024 x 768, spp 2, K 2, BY_OBJECT: 786 432 jobs, three for every resident lane.  Identities (1) and (2)
    against ort_render_features at that size, the slots in the stated order, no id twice in a pixel"""
    w = world("c3_bunny_room")
    big_w, big_h = 1024, 768
    got, _ = w.scene.render_matte(big_w, big_h, 2, mc.SEED, "object", 2, want=("other", "hits", "states"))
    feat, _ = w.scene.render_features(big_w, big_h, 2, mc.SEED, want=("hits", "states"))
    mc.check_order(got["ids"], got["counts"], got["other"], got["hits"])
    assert (got["hits"] == feat["hits"]).all() and (got["states"] == feat["states"]).all() and (got["other"] == 0).all()
    assert ((got["ids"][..., 1] != mc.EMPTY).sum() > 1000)   # silhouettes and the aperture: pixels that see two objects
    one, _ = w.scene.render_matte(big_w, big_h, 1, mc.SEED, "prim", 2, want=("hits",))
    feat1, _ = w.scene.render_features(big_w, big_h, 1, mc.SEED, want=("hits", "ids"))
    hit = feat1["hits"] == 1
    assert (one["ids"][..., 0][hit] == feat1["ids"][..., 1][hit]).all() and (one["ids"][..., 0][~hit] == mc.EMPTY).all()
    assert (one["counts"][..., 0] == feat1["hits"]).all() and (one["ids"][..., 1] == mc.EMPTY).all()
    obj, _ = w.scene.render_matte(big_w, big_h, 1, mc.SEED, "object", 2, want=())
    assert (obj["ids"][..., 0][hit] == mc.object_of_prim(w.flat, feat1["ids"][..., 1][hit])).all()


# ---- the mask ---------------------------------------------------------------------------------------------------------------------------
def test_mask_is_numpy(api):
    """ort_matte_mask on hostile slots (all EMPTY, ids twice in a pixel, sums above spp that wrap, 0xFFFFFFFF counts), selections with
    duplicates, of one id, of 256, of ids no slot holds: numpy's one line, bit for bit.  A frame of more pixels than one launch's
    first stride covers, and odd sizes"""
    rng = np.random.default_rng(12)
    for k, shape in ((1, (5, 7)), (2, (2, 9, 11)), (8, (3, 16, 24)), (3, (301, 257))):
        ids, counts = mc.hostile_slots(rng, shape, k)
        for spp, select in ((1, [3]), (5, [3, 3, 7, 3, 0]), (1 << 24, list(range(256))), (7, [500, 600]), (16, [11, 0, 5, 0xFFFFFFFE])):
            got = api.matte_mask(ids, counts, spp, select)
            want = mc.mask(ids, counts, spp, select)
            assert got.shape == want.shape and (got.view("<u4") == want.view("<u4")).all(), (k, shape, spp, select)


def test_mask_device_form_between_guard_words(api, world):
    """the device form on a render's slots, on a non-default stream, every buffer between guard words: the mask is the host form's and
    numpy's, ids and counts are unchanged, no guard word is touched; a refused call writes nothing"""
    import torch
    w = world("open")
    got, _ = host_call(w, 5, True, "object", 8)
    ids, mats = w.scene.object_ids()
    select = ids[mats == np.argmax(np.bincount(mats))]   # every object of the most common material
    assert 1 < len(select) <= api.MAX_MATTE_SELECT
    want = mc.mask(got["ids"], got["counts"], 5, select)
    assert (want > 0).any() and ((want > 0) & (want < 1)).any()
    assert (api.matte_mask(got["ids"], got["counts"], 5, select).view("<u4") == want.view("<u4")).all()
    dev = torch.device("cuda", 0)

    def guarded(words):
        whole = np.full(len(words) + 2 * GUARD, 0xA5A5A5A5, "<u4")
        whole[GUARD:-GUARD] = words
        return torch.from_numpy(whole.view("<i4")).to(dev)
    t = {"ids": guarded(got["ids"].reshape(-1)), "counts": guarded(got["counts"].reshape(-1)), "out": guarded(np.full(want.size, 0x5EED5EED, "<u4"))}
    ptr = {p: v.data_ptr() + 4 * GUARD for p, v in t.items()}
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    nv = len(w.mcams)
    with torch.cuda.stream(stream):
        with pytest.raises(api.OrtError):
            api.matte_mask_device(ptr["ids"], ptr["counts"], 8, 5, [3, mc.EMPTY], mc.W, mc.H, ptr["out"], frame_count=nv, stream=stream.cuda_stream)
        stream.synchronize()
        assert (t["out"].cpu().numpy().view("<u4")[GUARD:-GUARD] == 0x5EED5EED).all(), "a refused call wrote"
        sel = np.array(select, "<u4")
        api.matte_mask_device(ptr["ids"], ptr["counts"], 8, 5, sel, mc.W, mc.H, ptr["out"], frame_count=nv, stream=stream.cuda_stream)
        sel[:] = 0   # select is read before the call returns
    stream.synchronize()
    back = {p: v.cpu().numpy().view("<u4") for p, v in t.items()}
    for p, v in back.items():
        assert (v[:GUARD] == 0xA5A5A5A5).all() and (v[-GUARD:] == 0xA5A5A5A5).all(), "guard words of %s overwritten" % p
    assert (back["out"][GUARD:-GUARD].reshape(want.shape) == want.view("<u4")).all()
    assert (back["ids"][GUARD:-GUARD] == got["ids"].reshape(-1)).all() and (back["counts"][GUARD:-GUARD] == got["counts"].reshape(-1)).all()
