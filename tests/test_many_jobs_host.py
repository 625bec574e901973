"""What makes tests/test_gpu_many_jobs.py mean something, checked without a device (tests/many_jobs_cases.py): the launch plans
of every family at 1024 x 768 on a 256-unit device -- at least two jobs per resident lane, and a tail really held back under the
knob sets that claim to batch --, the sample maps' value classes and windows from the maps alone, and from the oracle's chains
that the stopping rule cuts some pixels and not others in every window the oracle is asked about."""
import numpy as np
import pytest

import light_groups_cases as lg
import many_jobs_cases as mj
import sample_map_cases as sm
from test_launch_plan import tool  # noqa: F401 -- the fixture: tools/launch_plan, built as tests/test_launch_plan.py builds it

CU = 256


def test_every_launch_has_two_jobs_a_lane_and_the_batching_sets_batch(tool):  # noqa: F811
    seen = mj.plans(tool, CU)
    print(mj.plans_report(seen))
    lanes = mj.lanes(CU)
    assert lanes == 262144
    for family in ("adaptive", "light groups", "sample map", "features spp 1"):
        assert seen[(family, "default")][:2] == (mj.W * mj.H, 4 * CU) and mj.W * mj.H == 3 * lanes
        # what the small frames of the families' own tests get, and this frame does not: nothing held back by default is fine,
        # as long as the batching sets hold something back
        assert seen[(family, "batches of 7 to the end")][2:] == (7, 3 * lanes)
        assert seen[(family, "batches of 128, tail 1")][2:] == (128, 2 * lanes)
    assert seen[("views chunk", "default")][0] == 2 * 2 * 3 * lanes
    assert seen[("irradiance points", "default")][0] == 3 * lanes + 257


def test_the_small_frames_batch_nothing(tool):  # noqa: F811
    """the gap this closes, stated: at 24 x 16 every value of ORT_JOB_BATCH plans what the unbatched run plans"""
    import test_launch_plan as tlp
    for batch in ("0", "7", "128"):
        p = tlp.plan(tool, {"ORT_JOB_BATCH": batch}, cu_count=CU, width=24, height=16, policy="pixel", groups=1, spp=16)
        assert p["job_count"] == 384 and (p["batch_until"] == 0 or p["job_batch"] == 0), p


def test_the_maps_meet_their_conditions():
    for shift in (0, 3):
        mj.assert_full_map(mj.full_map(shift))
    assert (mj.full_map() != mj.full_map(3)).mean() > 0.5
    for seed in (20240607, 5):
        mj.assert_sparse_map(mj.sparse_map(seed))
    m = mj.full_map()
    for bx, by in mj.ZERO_BLOCKS:
        assert bx % 8 == 0 and by % 8 == 0 and not m[by:by + 8, bx:bx + 8].any()
    assert not m[list(mj.ZERO_ROWS)].any()
    n = sm.counts(m, mj.CAP)
    assert set(np.unique(n).tolist()) == {0, 1, 2, 4, 8}


def test_the_windows_are_what_they_are_for():
    (ax0, ay0, _, _), (bx0, by0, _, _), (_, _, cx1, cy1) = mj.WINDOWS
    assert (ax0, ay0) == (0, 0) and bx0 % 8 and by0 % 8 and (cx1, cy1) == (mj.W, mj.H)
    for x0, y0, x1, y1 in mj.WINDOWS:
        assert (x1 - x0, y1 - y0) == (24, 16) and 0 <= x0 and x1 <= mj.W and 0 <= y0 and y1 <= mj.H
    assert (mj.W // 8) * (mj.H // 8) == 12288


@pytest.mark.parametrize("name", list(mj.ADAPTIVE_WINDOWS))
def test_the_rule_cuts_some_pixels_of_every_window(api, oracle, tmp_path_factory, name):
    """from the oracle's chains, never from the device: in every window at least two counts on at least 5 % of its pixels each"""
    c = lg.case(api, oracle, name, tmp_path_factory)
    mj.assert_adaptive_windows(c)
    kinds = [w for w in mj.ADAPTIVE_WINDOWS[name]]
    assert len(kinds) == 3 and kinds[0][:2] == (0, 0) and kinds[1][0] % 8 and kinds[1][1] % 8 and kinds[2][2:] == (mj.W, mj.H)


def test_the_size_argument_defaults_to_the_small_frame(api, oracle, tmp_path_factory):
    """light_groups_cases and sample_map_cases at their own 24 x 16 are untouched by the size argument; at 1024 x 768 the camera
    is the one Scene.flatten(1024, 768) gives"""
    c = lg.case(api, oracle, "room_diffuse", tmp_path_factory)
    assert c.camera() is c.cam and c.camera((lg.W, lg.H)) is c.cam
    assert c.camera(mj.SIZE).tobytes() == np.asarray(c.scene.flatten(*mj.SIZE).camera, "<f4").tobytes() != c.cam.tobytes()
    assert (sm.mixed_map() == sm.mixed_map(size=(sm.W, sm.H))).all() and sm.base_map(size=mj.SIZE).shape == (mj.H, mj.W)
    assert lg.inside(lg.RECT).shape == (lg.H, lg.W) and lg.inside(mj.WINDOWS[1], mj.SIZE).sum() == 384
    cams = mj.view_cameras(api, c)
    assert cams.shape == (2, 4, 3) and cams[0].tobytes() == c.camera(mj.SIZE).tobytes() != cams[1].tobytes()


def test_the_whole_frames_camera_rays_are_the_oracles(api, oracle, load_scene):
    """many_jobs_cases' numpy stream seeding and aperture draw against the oracle's own, call by call: on every pixel of the
    three windows through feature_cases.camera_rays, and on 4 096 streams picked across the frame on two seeds"""
    import feature_cases as fc
    cam = load_scene("c4_dwarf_room").camera(*mj.SIZE)
    for win in mj.WINDOWS:
        slow, fast = mj.first_rays(oracle, cam, mj.SEED, win, fast=False), mj.first_rays(oracle, cam, mj.SEED, win)
        assert slow[0].tobytes() == fast[0].tobytes() and slow[1].tobytes() == fast[1].tobytes(), win
    pix = np.random.default_rng(1).integers(0, mj.W * mj.H, 4096)
    for seed in (mj.SEED, 0xDEADBEEF):
        streams = fc.oracle_streams(oracle, seed, pix)
        assert (streams == mj.numpy_streams(oracle, seed, pix)).all()
        (a, ra), (b, rb) = fc.oracle_draw(oracle, streams), mj.numpy_draw(oracle, streams)
        assert (a == b).all() and ra.tobytes() == rb.tobytes()
