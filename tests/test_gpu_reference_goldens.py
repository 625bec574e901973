"""The device against the REFERENCE'S OWN answers on the generated test scenes, with no oracle in between: the deep scene
(coordinates out to 1.2e18), the light-pick rooms, the rooms of the light-group and feature renders through their dark and white
twins written as files, and the per-pixel chains of one-sample calls behind the adaptive and sample-map renders.  Everything
expected is read from tests/golden/ (make_golden.py --only-generated; tests/reference_goldens.py rebuilds the scene files, and
tests/test_oracle_golden.py holds their hashes and the oracle against the same fixtures).  Frames are at most 64 x 48; all bits."""
import numpy as np
import pytest

import deep_scenes as ds
import light_groups_cases as lg
import occluded_cases
import reference_goldens as rg
import render_adaptive_cases as rac
import sample_map_cases as sm
import test_gpu_light_pick as pick
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

KNOBS = ("ORT_EXCHANGE", "ORT_WAVES5", "ORT_WIDE", "ORT_MODE", "ORT_KERNEL", "ORT_LDS_TABLES", "ORT_DEBUG_FORCE_FALLBACK")
TABLES = {"lds": {}, "hbm": {"ORT_LDS_TABLES": "0"}}   # the default plan; the kernels that read the scene's tables from HBM


@pytest.fixture()
def knobs(monkeypatch):
    def set_(env):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    return set_


def uploaded(api, scene):
    if scene.device is None:
        assert api.device_count() >= 1, "GPU test on a machine without a HIP device (the render path has no CPU fallback)"
        scene.upload(0)
    return scene


# ---- the deep scene -------------------------------------------------------------------------------------------------------------
class Deep:
    pass


@pytest.fixture(scope="module")
def deep(api, manifest, tmp_path_factory):
    """the deep scene loaded from its regenerated file and uploaded, the grazing scene for its camera, both ray sets"""
    d = Deep()
    scn, graze_scn, layout = rg.deep_files(tmp_path_factory.mktemp("gpu_golden_deepscene"))
    d.meta = manifest["generated"]["deepscene"]
    assert rg.sha256(scn) == d.meta["scn_sha256"] and rg.sha256(graze_scn) == d.meta["graze"]["scn_sha256"]
    d.scene = uploaded(api, api.Scene.load_scn(scn).commit())
    d.graze_scene = api.Scene.load_scn(graze_scn)
    d.rays = dict(zip(("cone", "graze"), ds.ray_sets(layout)[:2]))
    d.hits = rg.load("raycast_deepscene.npz")
    d.frames = rg.load("renders_deepscene.npz")
    return d


@pytest.mark.parametrize("tables", list(TABLES))
def test_deep_scene_renders(deep, knobs, tables):
    """every frame of renders_deepscene.npz: PIXEL and CHUNK at 64 x 48, all four policies at 24 x 16, and the grazing camera's
    PIXEL frame as a batch of one view (the render call itself with that camera)"""
    knobs(TABLES[tables])
    for cam, policy, w, h, spp, chunk, key in rg.deep_renders():
        if cam == "cone":
            img, _ = deep.scene.render(w, h, spp, ds.SEED, policy, chunk=chunk)
        else:
            frames, _ = deep.scene.render_views(deep.graze_scene.camera(w, h)[None], [ds.SEED], w, h, spp, policy, chunk=chunk)
            img = frames[0]
        assert_bits_equal(img, deep.frames[key], "%s, tables in %s" % (key, tables))


@pytest.mark.parametrize("tables", list(TABLES))
@pytest.mark.parametrize("rays", ["cone", "graze"])
def test_deep_scene_raycast(deep, knobs, rays, tables):
    knobs(TABLES[tables])
    hits, _ = deep.scene.raycast(deep.rays[rays])
    assert_bits_equal(hits["t"], deep.hits[rays + "__t"], "t")
    assert_bits_equal(hits["n"], deep.hits[rays + "__n"], "normals")
    assert (hits["mat"] == deep.hits[rays + "__mat"]).all()


@pytest.mark.parametrize("tables", list(TABLES))
@pytest.mark.parametrize("rays", ["cone", "graze"])
def test_deep_scene_occluded(deep, knobs, rays, tables):
    """tmax at the reference's t, one float below and one float above, in turn: the contract on the reference's t and material"""
    knobs(TABLES[tables])
    t, mat = deep.hits[rays + "__t"], deep.hits[rays + "__mat"]
    k = np.arange(len(t)) % 3
    tmax = np.where(k == 0, t, np.where(k == 1, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf)))).astype("<f4")
    got, _ = deep.scene.occluded(deep.rays[rays], tmax)
    want = occluded_cases.expected(t, mat, tmax)
    assert want[k == 2].all() and not want[k != 2].any()   # the closed room: every ray hits, the strict < decides
    assert (np.asarray(got).astype(bool) == want).all(), "%d bytes differ" % (np.asarray(got).astype(bool) != want).sum()


# ---- the light-pick rooms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour,lights,key,text", rg.pick_rooms(), ids=[r[2] for r in rg.pick_rooms()])
def test_light_pick_rooms(api, manifest, tmp_path_factory, flavour, lights, key, text):
    """the PIXEL render, and the same pixels as one-pixel explicit jobs with their final RandomSeries states"""
    scn = rg.write_text(tmp_path_factory.mktemp("gpu_golden_pick"), "pick_" + key, text)
    assert rg.sha256(scn) == manifest["generated"]["light_pick"][key]["scn_sha256"]
    scene = uploaded(api, api.Scene.load_scn(scn).commit())
    z = rg.load("renders_light_pick.npz")
    W, H = pick.W, pick.H
    img, _ = scene.render(W, H, pick.SPP, pick.SEED, "pixel")
    assert_bits_equal(img, z[key + "__pixel"], key + ": PIXEL render")
    jobs = np.zeros(W * H, api.JOB_DTYPE)
    ys, xs = [a.reshape(-1) for a in np.mgrid[0:H, 0:W]]
    jobs["x0"], jobs["y0"], jobs["x1"], jobs["y1"], jobs["rng_state"], jobs["spp"] = xs, ys, xs + 1, ys + 1, api.job_seeds(pick.SEED, W * H), pick.SPP
    out = np.zeros((H, W, 3), "<f4")
    finals, _ = scene.tiled_raytrace_batch(out, jobs)
    assert_bits_equal(out, z[key + "__pixel"], key + ": one-pixel jobs")
    rg.assert_words_equal(np.asarray(finals, "<u4").reshape(H, W), z[key + "__states"], key + ": final RandomSeries states")


# ---- the rooms: light groups and features -----------------------------------------------------------------------------------------
@pytest.fixture()
def room(api, oracle, manifest, tmp_path_factory):
    """name -> light_groups_cases' Case of the room (its uploaded scene and its group tables; the oracle it carries is not asked)"""
    def get(name):
        c = lg.case(api, oracle, name, tmp_path_factory)
        assert rg.sha256(c.scn) == manifest["generated"]["rooms"][name]["own"]["scn_sha256"]
        uploaded(api, c.scene)
        return c
    return get


@pytest.mark.parametrize("spp", lg.SPPS)
@pytest.mark.parametrize("name", lg.ROOMS)
def test_light_groups_are_the_dark_twins(room, name, spp):
    """one group per light: frame g is the reference's PIXEL render of the file whose other `light` lines read 0 0 0; out_rgb and
    the final states are its render of the room itself"""
    c = room(name)
    z = rg.load("renders_rooms.npz")
    groups = c.per_light()
    assert len(groups) == 3
    out = [np.full((3, lg.H, lg.W, 3), lg.GUARD_F, "<f4"), np.full((lg.H, lg.W, 3), lg.GUARD_F, "<f4"), np.full((lg.H, lg.W), lg.GUARD_STATE, "<u4")]
    frames, rgb, states, _ = c.scene.render_light_groups(lg.W, lg.H, spp, lg.SEED, c.table(groups), True, True, group_count=3, rr=lg.RR, out=out)
    for g in range(3):
        assert_bits_equal(frames[g], z["%s__dark%d__%dspp" % (name, g, spp)], "%s %d spp: group %d" % (name, spp, g))
    assert_bits_equal(rgb, z["%s__own__%dspp" % (name, spp)], "%s %d spp: out_rgb" % (name, spp))
    rg.assert_words_equal(states, z["%s__own__%dspp__states" % (name, spp)], "%s %d spp: final states" % (name, spp))


@pytest.mark.parametrize("spp", lg.SPPS)
@pytest.mark.parametrize("name", lg.ROOMS)
def test_feature_hits_and_states_are_the_white_twins(room, name, spp):
    """feature_cases' relation: the white twin's frame is hits / spp in every channel, its final states are final_states"""
    c = room(name)
    z = rg.load("renders_rooms.npz")
    planes, _ = c.scene.render_features(lg.W, lg.H, spp, lg.SEED, want=("hits", "states"))
    ratio = (planes["hits"].astype("<f4") / np.float32(spp)).astype("<f4")
    assert_bits_equal(np.repeat(ratio[..., None], 3, axis=2), z["%s__white__%dspp" % (name, spp)], "%s %d spp: hits / spp" % (name, spp))
    assert (planes["hits"] <= spp).all()
    rg.assert_words_equal(planes["states"], z["%s__white__%dspp__states" % (name, spp)], "%s %d spp: final states" % (name, spp))


# ---- the chains: adaptive and sample-map renders ----------------------------------------------------------------------------------
@pytest.fixture()
def chained(room, gpu_scene):
    """name -> (the uploaded scene, the reference's chains of 64 one-sample calls a pixel)"""
    def get(name):
        scene = room(name).scene if name in lg.ROOMS else gpu_scene(name)
        return scene, rg.chains_from(rg.load("chains_rooms.npz"), name)
    return get


@pytest.mark.parametrize("ad", rac.SETS, ids=["frame", "every", "fixed"])
@pytest.mark.parametrize("name", rg.CHAIN_SCENES)
def test_adaptive_render_is_the_rule_on_the_references_samples(chained, name, ad):
    scene, chain = chained(name)
    want = rac.expected_from(chain, rac.W, rac.H, ad)
    rgb, spp, m2, fin, _ = scene.render_adaptive(rac.W, rac.H, ad.min_spp, ad.max_spp, ad.tolerance, ad.floor, ad.check_every, seed=rac.SEED,
                                                 rr=rac.RR, want_states=True)
    rac.assert_same((rgb, spp, m2, fin), want, "%s %r" % (name, ad))
    assert ad.min_spp == ad.max_spp or len(np.unique(spp)) > 1


@pytest.mark.parametrize("name", rg.CHAIN_SCENES)
def test_sample_map_render_is_the_references_chains_cut(chained, name):
    """the mixed map at cap 16 on guard-filled planes: the chain's first min(map, cap) samples, the guards where the count is 0"""
    assert (sm.W, sm.H, sm.SEED, sm.RR) == (rac.W, rac.H, rac.SEED, rac.RR)
    scene, chain = chained(name)
    smap = sm.mixed_map()
    want = sm.expected_from(chain, smap, sm.CAP)
    out = scene.render_sample_map(sm.W, sm.H, smap, sm.CAP, sm.SEED, True, True, rr=sm.RR, out=sm.guards())
    sm.assert_planes(out[:3], want, name)
