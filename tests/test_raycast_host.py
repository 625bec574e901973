"""Closest-hit ray queries (ort_raycast / ort_raycast_device), host side: the C ABI surface, the hit record layout,
argument and state errors (checked before any device work, so they are the same on a machine without a GPU), and
the helpers that decode a hit's shape."""
import ctypes
import subprocess

import numpy as np
import pytest

from host_cases import aligned as _aligned, scene as _scene


def test_raycast_entry_points_have_c_linkage(api):
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"ort_raycast", "ort_raycast_device"} <= names
    assert {"ort_raycast", "ort_raycast_device"} <= set(api.EXPORTS)


def test_hit_dtype_matches_ort_hit(api):
    assert api.HIT_DTYPE.itemsize == ctypes.sizeof(api.Hit) == 24
    for name in ("t", "n", "mat", "prim"):
        assert api.HIT_DTYPE.fields[name][1] == getattr(api.Hit, name).offset, name
    assert (api.HIT_DTYPE.fields["t"][1], api.HIT_DTYPE.fields["n"][1], api.HIT_DTYPE.fields["mat"][1],
            api.HIT_DTYPE.fields["prim"][1]) == (0, 4, 16, 20)
    assert (api.HIT_TRIANGLE, api.HIT_BOX, api.HIT_CYLINDER, api.HIT_SPHERE) == (0, 2, 3, 4)
    assert api.NO_PRIM == 0xFFFFFFFF


@pytest.mark.parametrize("device_form", [False, True])
def test_raycast_argument_errors(api, device_form):
    s = _scene(api)
    L = api.lib()
    keep_r, rays = _aligned(6 * 4 * 4)
    keep_h, hits = _aligned(4 * 24)

    def call(scene_handle, r, n, h):
        if device_form:
            return L.ort_raycast_device(scene_handle, r, n, h, 0, None, None)
        return L.ort_raycast(scene_handle, r, n, h, 0, None)

    assert call(None, rays, 4, hits) == api.ERR_INVALID
    assert call(s.handle, None, 4, hits) == api.ERR_INVALID
    assert call(s.handle, rays, 4, None) == api.ERR_INVALID
    # 8-byte alignment of both buffers (the kernel moves the 24-byte records as three 8-byte words)
    for r, h in ((rays + 4, hits), (rays, hits + 4), (rays + 2, hits + 6)):
        assert call(s.handle, r, 4, h) == api.ERR_INVALID
        assert b"aligned" in L.ort_last_error()
    # an 8-byte but not 16-byte aligned buffer is fine as far as the arguments go: the scene is not uploaded
    assert call(s.handle, rays + 8, 4, hits + 8) == api.ERR_NO_DEVICE


@pytest.mark.parametrize("device_form", [False, True])
def test_raycast_state_errors(api, device_form):
    L = api.lib()
    keep_r, rays = _aligned(24)
    keep_h, hits = _aligned(24)

    def call(s, r, n, h):
        if device_form:
            return L.ort_raycast_device(s.handle, r, n, h, api.RENDER_COUNTERS, None, None)
        return L.ort_raycast(s.handle, r, n, h, api.RENDER_COUNTERS, None)

    raw = _scene(api, committed=False)
    assert call(raw, rays, 1, hits) == api.ERR_STATE
    committed = _scene(api)
    assert call(committed, rays, 1, hits) == api.ERR_NO_DEVICE
    assert b"upload" in L.ort_last_error()
    # count == 0 needs no buffers, but the state is still checked
    assert call(committed, None, 0, None) == api.ERR_NO_DEVICE
    assert call(raw, None, 0, None) == api.ERR_STATE


def test_python_raycast_without_device_raises(api):
    s = _scene(api)
    with pytest.raises(api.OrtError) as e:
        s.raycast(np.zeros((3, 6), "<f4"))
    assert e.value.code == api.ERR_NO_DEVICE
    with pytest.raises(ValueError):
        s.raycast(np.zeros((3, 5), "<f4"))


def test_decode_prim_synthetic(api):
    assert api.decode_prim(api.NO_PRIM) == (None, None)
    assert api.decode_prim(0) == (api.HIT_TRIANGLE, 0)
    assert api.decode_prim((api.HIT_BOX << 28) | 5) == (api.HIT_BOX, 5)
    assert api.decode_prim((api.HIT_CYLINDER << 28) | 0x0FFFFFFF) == (api.HIT_CYLINDER, 0x0FFFFFFF)
    assert api.decode_prim(np.uint32((api.HIT_SPHERE << 28) | 12345)) == (api.HIT_SPHERE, 12345)
    prims = np.array([api.NO_PRIM, 7, (api.HIT_SPHERE << 28) | 3, (api.HIT_BOX << 28)], np.uint32)
    kind, index = api.decode_prim(prims)
    assert kind.tolist() == [-1, api.HIT_TRIANGLE, api.HIT_SPHERE, api.HIT_BOX]
    assert index.tolist() == [-1, 7, 3, 0]


def _mesh_triangle_counts(api, s):
    counts = []
    for i in range(s.info().mesh_count):
        m = api.Mesh()
        assert api.lib().ort_scene_get_mesh(s.handle, i, ctypes.byref(m)) == api.OK
        counts.append(m.index_count // 3)
    return counts


def test_triangle_of_synthetic(api):
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], "<f4")
    mats = np.zeros(2, api.MATERIAL_DTYPE)
    meshes = [dict(vertices=tri, indices=np.array([0, 1, 2], "<u4"), mat=1),
              dict(vertices=tri, indices=np.array([0, 1, 2, 1, 3, 2, 0, 3, 2], "<u4"), mat=1),
              dict(vertices=tri, indices=np.array([0, 1, 2, 1, 3, 2, 7], "<u4")[:6], mat=1)]
    s = api.Scene.from_arrays(mats, meshes=meshes)
    assert s.triangle_of(0) == (0, 0)
    assert s.triangle_of(1) == (1, 0)
    assert s.triangle_of(3) == (1, 2)
    assert s.triangle_of(4) == (2, 0)
    assert s.triangle_of(5) == (2, 1)
    mesh, local = s.triangle_of(np.arange(6))
    assert mesh.tolist() == [0, 1, 1, 1, 2, 2] and local.tolist() == [0, 0, 1, 2, 0, 1]
    with pytest.raises(IndexError):
        s.triangle_of(6)
    with pytest.raises(IndexError):
        s.triangle_of(-1)


@pytest.mark.parametrize("name", ["letters", "c3_bunny_room"])
def test_triangle_of_scene_meshes(api, load_scene, name):
    s = load_scene(name)
    counts = _mesh_triangle_counts(api, s)
    assert sum(counts) == s.info().triangle_count > 0
    first = np.concatenate([[0], np.cumsum(counts)])
    for m, c in enumerate(counts):
        if c == 0:
            continue
        assert s.triangle_of(int(first[m])) == (m, 0)
        assert s.triangle_of(int(first[m] + c - 1)) == (m, c - 1)
    ids = np.arange(sum(counts))
    mesh, local = s.triangle_of(ids)
    assert (first[mesh] + local == ids).all()
    assert (local < np.asarray(counts)[mesh]).all()
