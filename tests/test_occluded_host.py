"""Occlusion ray queries (ort_occluded / ort_occluded_device), host side: the C ABI surface, and the argument and state
errors in the order include/ort.h gives them -- all reported before any device work, so they are the same on a machine
without a GPU -- and the shapes Scene.occluded accepts."""
import subprocess

import numpy as np
import pytest

from host_cases import aligned as _aligned, scene as _scene

NAMES = {"ort_occluded", "ort_occluded_device"}


def test_occluded_entry_points_have_c_linkage(api):
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NAMES <= names
    assert NAMES <= set(api.EXPORTS)
    assert api.lib().ort_abi_version() == 3   # additive: the ABI version stands


def _caller(api, device_form):
    L = api.lib()

    def call(handle, rays, tmax, n, out, flags=0):
        if device_form:
            return L.ort_occluded_device(handle, rays, tmax, n, out, flags, None, None)
        return L.ort_occluded(handle, rays, tmax, n, out, flags, None)
    return call


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("committed", [True, False])
def test_occluded_argument_errors_come_first(api, device_form, committed):
    """null and misaligned pointers are ORT_ERR_INVALID on a committed-but-not-uploaded scene and on an uncommitted one:
    argument errors precede state errors"""
    s = _scene(api, committed)
    L = api.lib()
    call = _caller(api, device_form)
    keep_r, rays = _aligned(4 * 24)
    keep_t, tmax = _aligned(4 * 4)
    keep_o, out = _aligned(4)
    state = api.ERR_NO_DEVICE if committed else api.ERR_STATE
    assert call(None, rays, tmax, 4, out) == api.ERR_INVALID
    assert call(s.handle, None, tmax, 4, out) == api.ERR_INVALID
    assert call(s.handle, rays, tmax, 4, None) == api.ERR_INVALID
    assert call(s.handle, None, None, 4, None) == api.ERR_INVALID
    for r, t in ((rays + 4, tmax), (rays + 2, None), (rays, tmax + 2), (rays, tmax + 1), (rays + 4, tmax + 3)):
        assert call(s.handle, r, t, 4, out) == api.ERR_INVALID
        assert b"aligned" in L.ort_last_error()
    # rays 8-byte (not 16-byte) aligned, tmax 4-byte aligned, the bytes at any address, tmax null: fine as arguments go
    assert call(s.handle, rays + 8, tmax + 4, 4, out + 1) == state
    assert call(s.handle, rays, None, 4, out + 3) == state


@pytest.mark.parametrize("device_form", [False, True])
def test_occluded_state_errors(api, device_form):
    L = api.lib()
    call = _caller(api, device_form)
    keep_r, rays = _aligned(24)
    keep_t, tmax = _aligned(4)
    keep_o, out = _aligned(1)
    raw = _scene(api, committed=False)
    assert call(raw.handle, rays, tmax, 1, out, api.RENDER_COUNTERS) == api.ERR_STATE
    assert b"commit" in L.ort_last_error()
    committed = _scene(api)
    assert call(committed.handle, rays, tmax, 1, out, api.RENDER_COUNTERS) == api.ERR_NO_DEVICE
    assert b"upload" in L.ort_last_error()
    assert call(committed.handle, rays, None, 1, out) == api.ERR_NO_DEVICE


@pytest.mark.parametrize("device_form", [False, True])
def test_occluded_empty_batch_is_ok(api, device_form):
    """count == 0: ORT_OK without a launch, whatever the other arguments"""
    call = _caller(api, device_form)
    keep_r, rays = _aligned(24)
    for s in (_scene(api), _scene(api, committed=False)):
        assert call(s.handle, None, None, 0, None) == api.OK
        assert call(s.handle, rays + 1, rays + 1, 0, None) == api.OK
    assert call(None, None, None, 0, None) == api.OK
    L = api.lib()
    st = api.Stats()
    st.rays = 7
    s = _scene(api)
    import ctypes
    if device_form:
        assert L.ort_occluded_device(s.handle, None, None, 0, None, 0, None, ctypes.byref(st)) == api.OK
    else:
        assert L.ort_occluded(s.handle, None, None, 0, None, 0, ctypes.byref(st)) == api.OK
    assert st.rays == 0


def test_python_occluded_shapes_and_device(api):
    s = _scene(api)
    for bad in (np.zeros((3, 5), "<f4"), np.zeros(6, "<f4"), np.zeros((2, 3, 6), "<f4")):
        with pytest.raises(ValueError):
            s.occluded(bad)
    rays = np.zeros((3, 6), "<f4")
    for bad in (np.zeros(2, "<f4"), np.zeros(4, "<f4"), np.zeros((3, 1), "<f4"), np.zeros((1, 3), "<f4")):
        with pytest.raises(ValueError):
            s.occluded(rays, bad)
    # a bad shape is rejected before the library is called: on an uncommitted scene it is still a ValueError
    with pytest.raises(ValueError):
        _scene(api, committed=False).occluded(rays, np.zeros(2, "<f4"))
    # good shapes reach the library, which has no device to run on
    for tmax in (None, 1.5, np.float32(2), np.ones(3, "<f4"), [1.0, 2.0, 3.0]):
        with pytest.raises(api.OrtError) as e:
            s.occluded(rays, tmax)
        assert e.value.code == api.ERR_NO_DEVICE
    out, st = s.occluded(np.zeros((0, 6), "<f4"), 1.0)
    assert out.dtype == np.bool_ and out.shape == (0,) and st["rays"] == 0
    with pytest.raises(api.OrtError) as e:
        s.occluded_device(64, None, 4, 64)
    assert e.value.code == api.ERR_NO_DEVICE
