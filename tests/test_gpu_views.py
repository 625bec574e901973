"""A batch of camera views in one launch (ort_render_views) on the device: every frame bit for bit the oracle's render from that
view's camera with that view's seed, in the PIXEL and CHUNK policies, through every flavour of the VIEWS kernels (all lobes,
diffuse, counters, tables in LDS and in HBM); the ties to the single-view call; the rect; the device form; the rejected camera.

The views: the scene's own pose, moved toward the centre of the scene's box by 0, 0.3 and 0.6 of the way (inside the box by
convexity; the 0.2 height ratio of every data/*.scn keeps the aperture far within the 0.25 of slack) and yawed by 0, +25 and
-40 degrees; the same pose goes to api.camera_from_pose and to the oracle's camera()."""
import numpy as np
import pytest

import table_scenes
import views_cases
from conftest import assert_bits_equal
from views_cases import MOVES, SEEDS, quat_mul, scene_box  # noqa: F401

pytestmark = pytest.mark.gpu

W, H = 20, 13   # 3 x 2 blocks of 8 x 8: partial blocks on two edges
POLICIES = [("pixel", 3, 0), ("chunk", 4, 2), ("chunk", 3, 1)]
SCENES = ["c2_analytic", "c3_bunny_room", "glass_room", "c5_heightfield_224"]


def poses(scene, flat=None):
    """[(p, quat_xyzw, ratio)] for MOVES"""
    return views_cases.poses(scene, flat if flat is not None else scene.flatten(W, H))


_ref = {}


def reference(api, oracle, scene, name, csg=True):
    """name -> (cameras (3, 4, 3) as the product's pose helper gives them, {(policy, spp, chunk, rect): ((3, H, W, 3) frames, rays)}):
    the oracle's frames from each view's camera and seed, computed once per scene and policy and shared by the tests"""
    if name not in _ref:
        flat = scene.flatten(W, H)
        ps = poses(scene, flat)
        cams = np.stack([api.camera_from_pose(p, q, r, W, H) for p, q, r in ps])
        for cam, (p, q, r) in zip(cams, ps):
            assert_bits_equal(cam, oracle.camera(p, q, r, W, H), name + " pose")
        assert_bits_equal(cams[0], scene.camera(W, H), name + ": view 0 is the scene's own camera")
        _ref[name] = (cams, oracle.OracleScene(flat, with_reference_csg=csg), {})
    cams, osc, frames = _ref[name]

    def get(policy, spp, chunk, rect=None):
        key = (policy, spp, chunk, rect)
        if key not in frames:
            out, rays = [], 0
            for cam, seed in zip(cams, SEEDS):
                osc.set_camera(cam)
                img, st = osc.render(W, H, spp, seed, policy, chunk=max(chunk, 1), rect=rect, threads=16)
                out.append(img)
                rays += st["rays"]
            frames[key] = (np.stack(out), rays)
        return frames[key]
    return cams, get


@pytest.mark.parametrize("policy,spp,chunk", POLICIES)
@pytest.mark.parametrize("name", SCENES)
def test_views_match_the_oracle(api, oracle, gpu_scene, name, policy, spp, chunk):
    """three views, three seeds, one launch; without counters (the implicit VIEWS kernels: all lobes for c2_analytic -- prologue
    only -- and glass_room, diffuse for the bunny room and the height field) and with (the counters VIEWS kernel)"""
    scene = gpu_scene(name)
    cams, ref = reference(api, oracle, scene, name)
    want, rays = ref(policy, spp, chunk)
    frames, _ = scene.render_views(cams, SEEDS, W, H, spp, policy, chunk=chunk)
    assert frames.shape == (3, H, W, 3)
    for v in range(3):
        assert_bits_equal(frames[v], want[v], "%s %s view %d" % (name, policy, v))
    frames, st = scene.render_views(cams, SEEDS, W, H, spp, policy, chunk=chunk, counters=True)
    for v in range(3):
        assert_bits_equal(frames[v], want[v], "%s %s view %d, counters" % (name, policy, v))
    assert st["paths"] == 3 * W * H * spp
    assert st["rays"] == rays


@pytest.mark.parametrize("policy,spp,chunk", POLICIES)
def test_views_tie_to_the_single_view_call(api, oracle, gpu_scene, policy, spp, chunk):
    scene = gpu_scene("c3_bunny_room")
    cams, ref = reference(api, oracle, scene, "c3_bunny_room")
    want, _ = ref(policy, spp, chunk)
    # the scene's own camera with seed s is scene.render with seed s
    own = scene.camera(W, H)
    for seed in (SEEDS[0], 99):
        one, _ = scene.render_views(own[None], [seed], W, H, spp, policy, chunk=chunk)
        img, _ = scene.render(W, H, spp, seed, policy, chunk=chunk)
        assert_bits_equal(one[0], img, "own camera, seed %d" % seed)
    # ... and in a batch of two, where the table kernels run
    two, _ = scene.render_views(np.stack([own, own]), [SEEDS[0], 99], W, H, spp, policy, chunk=chunk)
    assert_bits_equal(two[1], img, "own camera in a batch")
    assert_bits_equal(two[0], want[0], "own camera in a batch vs the oracle")
    # a batch is its views one call each
    batch, _ = scene.render_views(cams, SEEDS, W, H, spp, policy, chunk=chunk)
    for v in range(3):
        one, _ = scene.render_views(cams[v:v + 1], SEEDS[v:v + 1], W, H, spp, policy, chunk=chunk)
        assert_bits_equal(one[0], batch[v], "view %d alone" % v)
        assert_bits_equal(one[0], want[v], "view %d alone vs the oracle" % v)
    # the same view twice: the same seed gives the same frame, another seed another
    rep, _ = scene.render_views(np.stack([cams[1], cams[1], cams[1]]), [SEEDS[1], SEEDS[1], SEEDS[1] + 1], W, H, spp, policy, chunk=chunk)
    assert_bits_equal(rep[0], want[1], "repeated view")
    assert_bits_equal(rep[1], rep[0], "repeated view, same seed")
    assert (rep[2].view("<u4") != rep[0].view("<u4")).any()


@pytest.mark.parametrize("policy,spp,chunk", POLICIES)
def test_views_rect(api, oracle, gpu_scene, policy, spp, chunk):
    scene = gpu_scene("glass_room")
    cams, ref = reference(api, oracle, scene, "glass_room")
    rect = (3, 2, 17, 9)
    want, _ = ref(policy, spp, chunk, rect)
    out = np.full((3, H, W, 3), 7.0, "<f4")
    frames, _ = scene.render_views(cams, SEEDS, W, H, spp, policy, chunk=chunk, rect=rect, out=out)
    assert frames is out
    inside = np.zeros((H, W), bool)
    inside[2:9, 3:17] = True
    for v in range(3):
        assert (frames[v][~inside] == 7.0).all(), "view %d: pixels outside the rect were touched" % v
        assert_bits_equal(frames[v][inside], want[v][inside], "view %d inside the rect" % v)


def _same_under(monkeypatch, scene, cams, want, env, what, policies=POLICIES):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for policy, spp, chunk in policies:
        frames, _ = scene.render_views(cams, SEEDS, W, H, spp, policy, chunk=chunk)
        for v in range(3):
            assert_bits_equal(frames[v], want(policy, spp, chunk)[0][v], "%s %s view %d" % (what, policy, v))
    for k in env:
        monkeypatch.delenv(k)


def test_views_general_kernel_on_a_diffuse_scene(api, oracle, gpu_scene, monkeypatch):
    scene = gpu_scene("c3_bunny_room")
    cams, ref = reference(api, oracle, scene, "c3_bunny_room")
    _same_under(monkeypatch, scene, cams, ref, {"ORT_KERNEL": "general"}, "ORT_KERNEL=general")


@pytest.mark.parametrize("name", ["c2_analytic", "c3_bunny_room"])
def test_views_tables_in_hbm(api, oracle, gpu_scene, monkeypatch, name):
    """ORT_LDS_TABLES=0: the VIEWS kernels without the LDS tables (all lobes; diffuse for the bunny room)"""
    scene = gpu_scene(name)
    cams, ref = reference(api, oracle, scene, name)
    _same_under(monkeypatch, scene, cams, ref, {"ORT_LDS_TABLES": "0"}, "ORT_LDS_TABLES=0")
    monkeypatch.setenv("ORT_LDS_TABLES", "0")
    frames, st = scene.render_views(cams, SEEDS, W, H, 4, "chunk", chunk=2, counters=True)
    want, rays = ref("chunk", 4, 2)
    assert_bits_equal(frames, want, "ORT_LDS_TABLES=0, counters")
    assert (st["paths"], st["rays"]) == (3 * W * H * 4, rays)


_table_cache = {}


def test_views_on_a_scene_past_the_table_caps(api, oracle, tmp_path_factory):
    """49 materials: the scene leaves the LDS tables by itself"""
    if "s" not in _table_cache:
        scene, _, csg = table_scenes.build(api, "mats_over", tmp_path_factory.mktemp("views_tables"))
        assert api.device_count() >= 1
        _table_cache["s"] = (scene.commit().upload(0), csg)
    scene, csg = _table_cache["s"]
    cams, ref = reference(api, oracle, scene, "tables:mats_over", csg)
    for policy, spp, chunk in POLICIES[:2]:
        frames, _ = scene.render_views(cams, SEEDS, W, H, spp, policy, chunk=chunk)
        assert_bits_equal(frames, ref(policy, spp, chunk)[0], "mats_over %s" % policy)


@pytest.mark.parametrize("batch", ["0", "7", "128"])
def test_views_job_batches_straddle_views(api, oracle, gpu_scene, monkeypatch, batch):
    """a view has 6 * 64 * nchunks jobs: batches of 7 and of 128 indices cross the view boundaries"""
    scene = gpu_scene("c3_bunny_room")
    cams, ref = reference(api, oracle, scene, "c3_bunny_room")
    _same_under(monkeypatch, scene, cams, ref, {"ORT_JOB_BATCH": batch}, "ORT_JOB_BATCH=" + batch)


def test_views_ignore_the_variants_they_do_not_have(api, oracle, gpu_scene, monkeypatch):
    scene = gpu_scene("c3_bunny_room")
    cams, ref = reference(api, oracle, scene, "c3_bunny_room")
    _same_under(monkeypatch, scene, cams, ref, {"ORT_EXCHANGE": "1", "ORT_WAVES5": "1"}, "ORT_EXCHANGE=1 ORT_WAVES5=1")
    scene = gpu_scene("c2_analytic")
    cams, ref = reference(api, oracle, scene, "c2_analytic")
    _same_under(monkeypatch, scene, cams, ref, {"ORT_EXCHANGE": "1", "ORT_WAVES5": "1", "ORT_WIDE": "1", "ORT_MODE": "wavefront"}, "every knob", POLICIES[:2])


def test_views_device_form(api, oracle, gpu_scene):
    import torch
    scene = gpu_scene("c3_bunny_room")
    cams, ref = reference(api, oracle, scene, "c3_bunny_room")
    stream = torch.cuda.Stream()
    for policy, spp, chunk in POLICIES[:2]:
        host, _ = scene.render_views(cams, SEEDS, W, H, spp, policy, chunk=chunk)
        p = api.Scene.params(W, H, spp, 12345, policy, chunk=chunk)   # params.seed is ignored
        assert api.views_workspace_bytes(p, 3) == 3 * api.workspace_bytes(p)
        a = torch.full((3, H, W, 3), -1.0, dtype=torch.float32, device="cuda")
        b = torch.full((3, H, W, 3), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert scene.render_views_device(a.data_ptr(), p, cams, SEEDS, stream=stream.cuda_stream) is None   # returns without waiting
        st = scene.render_views_device(b.data_ptr(), p, cams[::-1].copy(), SEEDS[::-1], stream=stream.cuda_stream, want_stats=True)   # settles the first
        assert st["kernel_ms"] > 0 and st["paths"] == 0
        stream.synchronize()
        assert_bits_equal(a.cpu().numpy(), host, "device form %s" % policy)
        assert_bits_equal(b.cpu().numpy(), host[::-1], "device form %s, views reversed" % policy)
        assert_bits_equal(host, ref(policy, spp, chunk)[0], "host form %s" % policy)


def test_views_rejected_camera(api, oracle, gpu_scene):
    """an argument check: nothing is launched, nothing written"""
    scene = gpu_scene("c2_analytic")
    cams, _ = reference(api, oracle, scene, "c2_analytic")
    lo, hi = scene_box(scene.flatten(W, H))
    bad = cams.copy()
    bad[2][0] = hi + 10.0
    out = np.full((3, H, W, 3), 7.0, "<f4")
    with pytest.raises(api.OrtError) as e:
        scene.render_views(bad, SEEDS, W, H, 2, "pixel", out=out)
    assert e.value.code == api.ERR_UNSUPPORTED and "view 2" in str(e.value)
    assert (out == 7.0).all()
    frames, _ = scene.render_views(cams, SEEDS, W, H, 2, "pixel", out=out)   # the scene is none the worse for it
    assert (frames != 7.0).any()
