"""The host form of the four ray queries across a staging slice: one full slice plus a ragged remainder, against the device
form of the same call (one launch over all rays).  The answers themselves are other tests' business (tests/test_gpu_raycast.py,
test_gpu_occluded.py, test_gpu_radiance.py, test_gpu_adaptive.py); here the two forms must agree bit for bit in every output
array, NaNs included, with every optional array passed and with none."""
import zlib

import numpy as np
import pytest

import radiance_cases as rc
from adaptive_cases import Adaptive
from occluded_cases import drawn_limits
from test_gpu_adaptive import torch_run
from test_gpu_occluded import torch_occluded
from test_gpu_radiance import torch_radiance
from test_gpu_raycast import mixed_rays, torch_raycast

pytestmark = pytest.mark.gpu

# kRaycastSlice and kRadianceSlice of offline_raytracer_amd/csrc/ort_kernels.hip, plus a remainder that is a multiple neither
# of the workgroup (256) nor of a wave (64): the smallest counts that run the slice loop twice and end on a ragged slice
RAYCAST_COUNT = (1 << 22) + 257
RADIANCE_COUNT = (1 << 20) + 257
BASE = 4096   # distinct rays, tiled up to the count
RR = 0.8
_base = {}


def same_bytes(host, device, what):
    host, device = np.ascontiguousarray(host), np.ascontiguousarray(device)
    assert host.shape == device.shape and host.dtype.itemsize == device.dtype.itemsize, what
    if host.tobytes() != device.tobytes():
        a, b = host.reshape(len(host), -1).view(np.uint8), device.reshape(len(device), -1).view(np.uint8)
        bad = np.flatnonzero((a != b).any(axis=1))
        raise AssertionError("%s: the forms differ for %d of %d rays, first %d (slice %d)"
                             % (what, len(bad), len(host), bad[0], bad[0] // (len(host) - 257)))


@pytest.fixture()
def scene(gpu_scene):
    return gpu_scene("c2_analytic")


def closest_hit_base(scene):
    """-> rays (BASE, 6), tmax (BASE,): the four kinds of tests/raycast_cases.py, limits drawn around their own hits"""
    if "hit" not in _base:
        rays, _ = mixed_rays(scene, "c2_analytic", BASE)
        rng = np.random.default_rng(zlib.crc32(b"slice boundary limits"))
        _base["hit"] = rays, drawn_limits(rng, scene.raycast(rays)[0]["t"])
    return _base["hit"]


def radiance_base(scene):
    """-> rays (BASE, 6), seeds (BASE,): pinholes inside the box, half of them looking at a light, and 16 rays outside the domain
    (they answer NaN)"""
    if "radiance" not in _base:
        rng = np.random.default_rng(zlib.crc32(b"slice boundary radiance"))
        flat = scene.flatten(1, 1)
        lo, hi = rc.origin_box(flat)
        k = (BASE - 16) // 2
        cams = np.concatenate([rc.inside(rng, lo, hi, k), rc.at_lights(rng, flat, lo, hi, k)])
        rays = np.array([np.concatenate(rc.pinhole(p, z)) for p, z in cams] + list(rc.out_of_domain(rng, lo, hi, 16)), "<f4")
        perm = rng.permutation(BASE)
        _base["radiance"] = rays[perm], rng.integers(0, 1 << 32, BASE, dtype=np.uint64).astype("<u4")
    return _base["radiance"]


def test_raycast_across_a_slice(scene):
    rays = closest_hit_base(scene)[0]
    rays = rays[np.arange(RAYCAST_COUNT) % len(rays)]
    host, _ = scene.raycast(rays)
    device, _ = torch_raycast(scene, rays)
    same_bytes(host, device, "hits")
    assert (host["mat"] != 0).any() and (host["mat"] == 0).any()


@pytest.mark.parametrize("limits", [True, False], ids=["tmax", "no tmax"])
def test_occluded_across_a_slice(scene, limits):
    rays, tmax = closest_hit_base(scene)
    idx = np.arange(RAYCAST_COUNT) % len(rays)
    rays, tmax = rays[idx], tmax[idx] if limits else None
    host, _ = scene.occluded(rays, tmax)
    device, _ = torch_occluded(scene, rays, tmax)
    same_bytes(host, device, "occlusion bytes")
    assert host.any() and not host.all()


@pytest.mark.parametrize("states", [True, False], ids=["states", "no states"])
def test_radiance_across_a_slice(scene, states):
    idx = np.arange(RADIANCE_COUNT) % BASE
    rays, seeds = radiance_base(scene)
    rays, seeds = rays[idx], seeds[idx]
    got = scene.radiance(rays, seeds, 1, RR, want_states=states)
    d_rgb, d_fin, _ = torch_radiance(scene, rays, seeds, 1, RR, states=states)
    same_bytes(got[0], d_rgb, "rgb")
    assert np.isnan(got[0]).any() and (got[0] > 0).any()
    if states:
        same_bytes(got[1], d_fin, "final states")
    else:
        assert (d_fin == 0x5A5A5A5A).all()   # nothing was written where nothing was asked for


@pytest.mark.parametrize("optional", [True, False], ids=["spp m2 states", "rgb alone"])
def test_adaptive_across_a_slice(api, scene, optional):
    idx = np.arange(RADIANCE_COUNT) % BASE
    rays, seeds = radiance_base(scene)
    rays, seeds = np.ascontiguousarray(rays[idx]), np.ascontiguousarray(seeds[idx])
    ad = Adaptive(2, 2, 1, 0.3, 0.05)
    device, _ = torch_run(scene, rc.Cases(rays, seeds, None, None), ad, RR, skip=() if optional else ("spp", "m2", "states"))
    n = len(rays)
    host = np.zeros((n, 3), "<f4"), np.zeros(n, "<u4"), np.zeros(n, "<f4"), np.zeros(n, "<u4")
    ptrs = [a.ctypes.data if optional or k == 0 else None for k, a in enumerate(host)]
    assert api.lib().ort_radiance_adaptive(scene.handle, rays.ctypes.data, seeds.ctypes.data, n, api.C.byref(api.Adaptive(*ad)), RR, *ptrs, 0,
                                           None) == api.OK
    same_bytes(host[0], device[0], "rgb")
    assert np.isnan(host[0]).any() and (host[0] > 0).any()
    if optional:
        for h, d, what in zip(host[1:], device[1:], ("spp", "m2", "final states")):
            same_bytes(h, d, what)
        assert set(np.unique(host[1])) == {0, 2}   # 0: the rays outside the domain
    else:
        assert not host[1].any() and not host[2].any() and not host[3].any()
        assert (device[1] == 0x5A5A5A5A).all() and (device[2] == np.float32(-7.0)).all() and (device[3] == 0x5A5A5A5A).all()
