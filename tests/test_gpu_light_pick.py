"""The light pick of a bounce (ort_lane.h, after the roulette draw: sample_random_lights' RNG steps, ray.cpp:537-601): one RNG
step, light index = state % light_count, four more steps if that light is a sphere.  With one light the index is 0 and the
kernels branch round the remainder; with more they take it.  Scenes of 1, 1, 2 and 3 lights, generated here -- a light is a
sphere under a `light` material (type 1) or any cylinder (type 2: the reference lists every cylinder, emitting or not); the
3-light scene has its sphere light between two cylinders, so the four extra steps depend on the index drawn.  16 x 16 pixels,
4 spp, PIXEL policy, the diffuse and the all-lobes flavour of the kernels: the image, and every pixel's final RandomSeries
state (the same pixels as one-pixel explicit jobs seeded as PIXEL seeds them), bit for bit against the oracle."""
import numpy as np
import pytest

from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

W = H = 16
SPP = 4
SEED = 20261019

ROOM = """screen 400 300
camera 5.553228 2.942755 2.900874 b 0.2 q 0.416981 0.279589 0.480987 0.718247
ambient 0.125000 0.125000 0.125000
brdf 0.600000 0.600000 0.600000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0
box -3.000000 -3.000000 -0.100000 18.000000 18.000000 0.100000
brdf 0.600000 0.600000 0.600000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0
box -3.000000 -3.000000 8.900000 18.000000 18.000000 0.100000
brdf 0.200000 0.900000 0.200000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0
box -3.000000 -3.000000 -0.100000 0.100000 18.000000 9.000000
brdf 0.900000 0.200000 0.900000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0
box 15.000000 -3.000000 -0.100000 0.100000 18.000000 9.000000
brdf 0.200000 0.200000 0.900000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0
box -3.000000 -3.000000 -0.100000 18.000000 0.100000 9.000000
brdf 0.900000 0.900000 0.200000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0
box -3.000000 15.000000 -0.100000 18.000000 0.100000 9.000000
brdf 0.595000 0.560000 0.210000 0.000000 0.000000 0.000000 200 0.000000 0.000000 0.000000 1.0
box -1.200000 -1.200000 0.390000 2.400000 2.400000 0.020000
"""
# three spheres on the table: glass, tinted glass with a specular lobe, a mirror (all lobes) / three diffuse ones (diffuse flavour)
SPHERES = {
    "all_lobes": """brdf 0.000000 0.000000 0.000000 0.000000 0.000000 0.000000 10 1.000000 1.000000 1.000000 1.4
sphere 0.000000 0.000000 0.900000 0.5
brdf 0.000000 0.000000 0.000000 0.200000 0.000000 0.000000 10 1.000000 0.000000 0.000000 1.2
sphere 1.000000 1.000000 0.800000 0.3
brdf 0.000000 0.000000 0.000000 1.000000 1.000000 1.000000 20 0.000000 0.000000 0.000000 1.0
sphere -1.000000 0.800000 0.700000 0.3
""",
    "diffuse": """brdf 0.800000 0.300000 0.300000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0
sphere 0.000000 0.000000 0.900000 0.5
brdf 0.300000 0.800000 0.300000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0
sphere 1.000000 1.000000 0.800000 0.3
brdf 0.300000 0.300000 0.800000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0
sphere -1.000000 0.800000 0.700000 0.3
""",
}
CYL_A = "cylinder 1.200000 -1.200000 0.400000 -0.000000 2.400000 0.000000 0.05\n"   # under the last sphere's material: a light that emits nothing
LIGHT = "light 3 3 2\n"
SPHERE_LIGHT = "sphere 0.000000 0.000000 2.800000 0.9\n"
CYL_B = "cylinder -1.200000 -1.200000 2.600000 2.400000 0.000000 0.000000 0.08\n"    # under the light material: it emits
# name -> (statements after the spheres, the light list's types in file order)
LIGHTS = {
    "one_sphere": (LIGHT + SPHERE_LIGHT, [1]),
    "one_cylinder": (LIGHT + CYL_B, [2]),
    "two": (CYL_A + LIGHT + SPHERE_LIGHT, [2, 1]),
    "three": (CYL_A + LIGHT + SPHERE_LIGHT + CYL_B, [2, 1, 2]),
}
# the default plan, the five-waves unit, the ray exchange, the kernels that read the light types from HBM
KNOBS = [{}, {"ORT_EXCHANGE": "0", "ORT_WAVES5": "1"}, {"ORT_EXCHANGE": "1"}, {"ORT_LDS_TABLES": "0"}]

_cache = {}


@pytest.fixture()
def pick_scene(api, oracle, tmp_path_factory):
    """(flavour, lights) -> (uploaded scene, its oracle scene, the oracle's PIXEL image, per-pixel jobs, the oracle's final states)"""
    def get(flavour, lights):
        key = (flavour, lights)
        if key not in _cache:
            tail, types = LIGHTS[lights]
            scn = tmp_path_factory.mktemp("light_pick") / ("%s_%s.scn" % (flavour, lights))
            scn.write_text(ROOM + SPHERES[flavour] + tail)
            scene = api.Scene.load_scn(str(scn)).commit()
            assert scene.info().light_count == len(types)
            flat = scene.flatten(W, H)
            assert flat.lights["type"].tolist() == types
            assert api.device_count() >= 1
            scene.upload(0)
            osc = oracle.OracleScene(flat)
            ref, _ = osc.render(W, H, SPP, SEED, "pixel", threads=4)
            jobs = np.zeros(W * H, api.JOB_DTYPE)
            states = np.zeros(W * H, "<u4")
            ref_jobs = np.zeros((H, W, 3), "<f4")
            for y in range(H):
                for x in range(W):
                    i = y * W + x
                    jobs[i] = (x, y, x + 1, y + 1, oracle.job_seed(SEED, i), SPP)
                    _, states[i] = osc.tiled_raytrace(ref_jobs, x, y, x + 1, y + 1, int(jobs[i]["rng_state"]), SPP)
            assert_bits_equal(ref_jobs, ref, "oracle: one-pixel jobs vs its PIXEL render")
            assert (ref != 0).any()
            _cache[key] = (scene, ref, jobs, states)
        return _cache[key]
    return get


@pytest.mark.parametrize("lights", list(LIGHTS))
@pytest.mark.parametrize("flavour", list(SPHERES))
def test_light_pick_matches_oracle(api, pick_scene, monkeypatch, flavour, lights):
    scene, ref, jobs, states = pick_scene(flavour, lights)
    for env in KNOBS:
        for k in ("ORT_EXCHANGE", "ORT_WAVES5", "ORT_LDS_TABLES"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        what = "%s, %s, %s" % (flavour, lights, env)
        img, _ = scene.render(W, H, SPP, SEED, "pixel")
        assert_bits_equal(img, ref, what + ": PIXEL render")
        out = np.zeros((H, W, 3), "<f4")
        finals, _ = scene.tiled_raytrace_batch(out, jobs)
        assert_bits_equal(out, ref, what + ": one-pixel jobs")
        assert finals.tolist() == states.tolist(), what + ": final RandomSeries states"
