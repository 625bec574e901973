"""The traversal stack past its LDS entries, on the device: the scene of tools/make_deepscene.py (tests/deep_scenes.py) takes
nearly every ray of every kernel into the scratch tail (six entries at the deepest) of its per-lane stack (the probe of tools/host_sim measures it,
tests/test_deep_stack_host.py asserts it), further in the five-waves unit (20 LDS entries), the wavefront trace (16), the
re-traversal of resolve_hit (four fewer each) and the wide tree (up to 44 entries deep).  One small launch per test, every
result bit for bit the oracle's."""
import numpy as np
import pytest

import ao_cases
import deep_scenes as ds
import occluded_cases
import radiance_cases
import render_adaptive_cases as rac
from adaptive_cases import Adaptive
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

KNOBS = ("ORT_EXCHANGE", "ORT_WAVES5", "ORT_WIDE", "ORT_MODE", "ORT_KERNEL", "ORT_LDS_TABLES", "ORT_DEBUG_FORCE_FALLBACK", "ORT_LONG_MIN",
         "ORT_INFLIGHT_CAP", "ORT_REFILL_BELOW", "ORT_LONG_REFILL")
PLAIN = {"ORT_EXCHANGE": "0", "ORT_WAVES5": "0"}
EXCHANGE = {"ORT_EXCHANGE": "1"}
# the plain loop; the five-waves unit; the ray exchange at its default and at the squeezed knob sets of
# test_gpu_parity.test_ray_exchange_equals_plain_loop (lanes with more than kLdsStack entries may not park, parked paths carry
# 20 and more stack words); the wavefront kernels; the wide tree; the all-lobes flavour; one ray in sixteen re-cast exactly
VARIANTS = {
    "plain": PLAIN,
    "waves5": {"ORT_EXCHANGE": "0", "ORT_WAVES5": "1"},
    "exchange": EXCHANGE,
    "exchange_16": dict(EXCHANGE, ORT_LONG_MIN="16", ORT_INFLIGHT_CAP="16", ORT_REFILL_BELOW="40"),
    "exchange_128": dict(EXCHANGE, ORT_LONG_MIN="128", ORT_INFLIGHT_CAP="128", ORT_LONG_REFILL="60"),
    "exchange_cap0": dict(EXCHANGE, ORT_INFLIGHT_CAP="0"),
    "exchange_long128": dict(EXCHANGE, ORT_LONG_MIN="128"),
    "wavefront": {"ORT_MODE": "wavefront"},
    "wide": {"ORT_WIDE": "1"},
    "general": {"ORT_KERNEL": "general"},
    "tables_in_hbm": {"ORT_LDS_TABLES": "0"},
    "some_exact": {"ORT_DEBUG_FORCE_FALLBACK": "0xf"},
    "plain_some_exact": dict(PLAIN, ORT_DEBUG_FORCE_FALLBACK="0xf"),
}


@pytest.fixture(scope="module")
def w(api, oracle, tmp_path_factory):
    w = ds.world(api, oracle, tmp_path_factory)
    if w.scene.device is None:
        assert api.device_count() >= 1
        w.scene.upload(0)
    return w


@pytest.fixture()
def knobs(monkeypatch):
    def set_(env):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    return set_


def test_conditions(w):
    ds.assert_conditions(w)


@pytest.mark.parametrize("counters", [False, True])
@pytest.mark.parametrize("tables", ["lds", "hbm"])
@pytest.mark.parametrize("rays", ["cone", "grazing"])
def test_raycast(w, knobs, rays, tables, counters):
    """grazing: rays at the cylinders' silhouettes, a few hundred of which resolve_hit traverses a second time"""
    rr, (t, n, mat) = (w.rays, (w.t, w.n, w.mat)) if rays == "cone" else (w.graze, w.graze_hits)
    knobs({} if tables == "lds" else {"ORT_LDS_TABLES": "0"})
    hits, st = w.scene.raycast(rr, counters=counters)
    assert_bits_equal(hits["t"], t, "t")
    assert_bits_equal(hits["n"], n, "normals")
    assert (hits["mat"] == mat).all()
    host = ds.probes(w, "rays" if rays == "cone" else "graze")[ds.TOOLS[0]][1]
    assert st["fallback_rays"] == host["fallback"]
    if counters:
        assert st["rays"] == host["rays"] == len(rr)


@pytest.mark.parametrize("counters", [False, True])
@pytest.mark.parametrize("tables", ["lds", "hbm"])
def test_occluded(w, knobs, tables, counters):
    knobs({} if tables == "lds" else {"ORT_LDS_TABLES": "0"})
    k = np.arange(len(w.t)) % 3
    tmax = np.where(k == 0, w.t, np.where(k == 1, np.nextafter(w.t, np.float32(-np.inf)), np.nextafter(w.t, np.float32(np.inf)))).astype("<f4")
    got, st = w.scene.occluded(w.rays, tmax, counters=counters)
    want = occluded_cases.expected(w.t, w.mat, tmax)
    assert (np.asarray(got).astype(bool) == want).all(), "%d bytes differ" % (np.asarray(got).astype(bool) != want).sum()
    got, _ = w.scene.occluded(w.rays, None, counters=counters)
    assert np.asarray(got).astype(bool).all()
    if counters:
        assert st["rays"] == len(w.rays)


@pytest.mark.parametrize("policy", ["chunk", "pixel"])
@pytest.mark.parametrize("variant", list(VARIANTS), ids=list(VARIANTS))
@pytest.mark.parametrize("camera", ["cone", "grazing"])
def test_render(w, knobs, camera, variant, policy):
    """cone: the scene's own camera.  grazing: a camera that looks at a cylinder's silhouette, given as a batch of one view,
    which is the render call itself with that camera: hundreds of the frame's rays are re-traversed by resolve_hit, with the
    re-traversal's stack past its LDS entries (tests/test_deep_stack_host.py asserts that from the probe).  Paths, rays and the
    rays in the exact fallback are those of tools/host_sim's render of the same frame"""
    width, height, spp, chunk = ds.GPU_RENDER
    chunk = chunk if policy == "chunk" else 0
    cam = None if camera == "cone" else ds.graze_cam(w, width, height)
    ref, ost = ds.oracle_render(w, width, height, spp, policy, chunk, cam=cam)
    knobs(VARIANTS[variant])

    def render(counters):
        if cam is None:
            return w.scene.render(width, height, spp, ds.SEED, policy, chunk=chunk, counters=counters)
        frames, st = w.scene.render_views(cam[None], [ds.SEED], width, height, spp, policy, chunk=chunk, counters=counters)
        return frames[0], st
    img, _ = render(False)
    assert_bits_equal(img, ref, "%s %s %s" % (camera, variant, policy))
    img, st = render(True)
    assert_bits_equal(img, ref, "%s %s %s, counters" % (camera, variant, policy))
    host = ds.host_render_counters(w, camera, width, height, spp, policy, chunk,
                                   {"SIM_FORCE_FALLBACK": "0xf"} if "some_exact" in variant else None)
    assert st["paths"] == width * height * spp == ost["paths"] == host["paths"] and st["rays"] == ost["rays"] == host["rays"]
    assert st["fallback_rays"] == host["fallback"]
    assert (0 < st["fallback_rays"] < st["rays"]) if "some_exact" in variant else st["fallback_rays"] * 20 <= st["rays"]


@pytest.mark.parametrize("policy", ["chunk", "pixel"])
@pytest.mark.parametrize("variant", ["default", "plain", "waves5", "exchange_16"])
def test_render_views(api, w, knobs, variant, policy):
    width, height, spp, chunk = ds.GPU_RENDER
    chunk = chunk if policy == "chunk" else 0
    cams = ds.view_cams(api, w, width, height)
    knobs(VARIANTS.get(variant, {}))
    frames, _ = w.scene.render_views(cams, ds.VIEW_SEEDS, width, height, spp, policy, chunk=chunk)
    for v, (cam, seed) in enumerate(zip(cams, ds.VIEW_SEEDS)):
        ref, _ = ds.oracle_render(w, width, height, spp, policy, chunk, cam=cam, seed=seed)
        assert_bits_equal(frames[v], ref, "%s %s view %d" % (variant, policy, v))


@pytest.mark.parametrize("variant", ["default", "tables_in_hbm", "general", "some_exact"])
def test_radiance(w, knobs, variant):
    want_rgb, want_states = ds.radiance_expected(w, 2)
    knobs(VARIANTS.get(variant, {}))
    for counters in (False, True):
        rgb, states, _ = w.scene.radiance(w.prays, w.pseeds, 2, 0.8, want_states=True, counters=counters)
        radiance_cases.assert_same(rgb, states, want_rgb, want_states, "%s counters=%s" % (variant, counters))


@pytest.mark.parametrize("variant", ["default", "tables_in_hbm", "general", "some_exact"])
def test_irradiance(w, knobs, variant):
    """the irradiance unit's kernels, a copy of the lane code of their own"""
    want_rgb, want_states = ds.irradiance_expected(w, 2)
    knobs(VARIANTS.get(variant, {}))
    for counters in (False, True):
        rgb, states, _ = w.scene.irradiance(w.points.points, w.points.seeds, 2, 0.8, want_states=True, counters=counters)
        radiance_cases.assert_same(rgb, states, want_rgb, want_states, "%s counters=%s" % (variant, counters))


@pytest.mark.parametrize("radius", ["none", "per point"])
@pytest.mark.parametrize("variant", ["default", "tables_in_hbm", "some_exact"])
def test_ambient_occlusion(w, knobs, variant, radius):
    radius = None if radius == "none" else ds.ao_radius(w)
    want = ds.ao_expected(w, radius)
    knobs(VARIANTS.get(variant, {}))
    for counters in (False, True):
        got = w.scene.ambient_occlusion(w.points.points, w.points.seeds, ds.AO_SPP, radius, want_bent=True, want_states=True, counters=counters)
        ao_cases.assert_same(got[:3], want, "%s counters=%s" % (variant, counters))


@pytest.mark.parametrize("variant", ["default", "tables_in_hbm", "general"])
def test_render_adaptive(w, knobs, variant):
    """pt_adaptive, a unit of its own: every pixel checked after every sample from the second on, four at the most"""
    ad = Adaptive(2, 4, 1, 0.3, 0.05)
    width, height = ds.RENDER[:2]

    def make():
        w.osc.set_camera(w.scene.camera(width, height))
        return rac.expected_from(rac.chains(w.osc, width, height, ds.SEED, rac.RR, spp=ad.max_spp), width, height, ad)
    want = ds.cached(w, "render_adaptive", make)
    knobs(VARIANTS.get(variant, {}))
    rgb, spp, m2, fin, _ = w.scene.render_adaptive(width, height, ad.min_spp, ad.max_spp, ad.tolerance, ad.floor, ad.check_every, seed=ds.SEED,
                                                   rr=rac.RR, want_states=True)
    rac.assert_same((rgb, spp, m2, fin), want, variant)
    assert len(np.unique(spp)) > 1


@pytest.mark.parametrize("variant", ["default", "tables_in_hbm", "general", "some_exact"])
def test_light_groups(w, knobs, variant):
    """pt_groups, built beside pt_adaptive: the scene's one light material in group 5 of 8, on guard-filled planes: frame 5,
    out_rgb and the states are the oracle's PIXEL render, the other seven frames +0 in every word"""
    import light_groups_cases as lg
    width, height, spp, _ = ds.RENDER
    G = ds.LIGHT_GROUPS[0]
    want = ds.light_groups_expected(w)
    knobs(VARIANTS.get(variant, {}))
    for counters in (False, True):
        out = [np.full((G, height, width, 3), lg.GUARD_F, "<f4"), np.full((height, width, 3), lg.GUARD_F, "<f4"), np.full((height, width), lg.GUARD_STATE, "<u4")]
        frames, rgb, states, st = w.scene.render_light_groups(width, height, spp, ds.SEED, ds.group_table(w), True, True, group_count=G, rr=lg.RR,
                                                              counters=counters, out=out)
        for got, w_, label in zip((frames, rgb, states), want, ("group frames", "out_rgb", "final states")):
            lg.assert_plane(got, w_, None, lg.GUARD_F, "%s counters=%s: %s" % (variant, counters, label))
        assert st["paths"] == (width * height * spp if counters else 0)


@pytest.mark.parametrize("variant", ["default", "tables_in_hbm", "general", "some_exact"])
def test_sample_map(w, knobs, variant):
    """pt_sample_map: the mixed map at cap 4 against the oracle's chains, the guards where a pixel has no samples"""
    import sample_map_cases as sm
    width, height = ds.RENDER[:2]
    smap, want = ds.sample_map_expected(w)
    knobs(VARIANTS.get(variant, {}))
    for counters in (False, True):
        out = w.scene.render_sample_map(width, height, smap, ds.MAP_CAP, ds.SEED, True, True, rr=sm.RR, counters=counters, out=sm.guards())
        sm.assert_planes(out[:3], want, "%s counters=%s" % (variant, counters))
        assert out[3]["paths"] == (int(sm.counts(smap, ds.MAP_CAP).sum()) if counters else 0)
