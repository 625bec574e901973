"""The views of the batch-of-views tests (test infrastructure): shared by the GPU tests (tests/test_gpu_views.py) and the
host-compiled lane code's (tests/test_query_lanes_host.py).  The scene's own pose, moved toward the centre of the scene's box by
0, 0.3 and 0.6 of the way and yawed by 0, +25 and -40 degrees."""
import numpy as np

SEEDS = [2024, 7, 0xDEADBEEF]
MOVES = [(0.0, 0.0), (0.3, 25.0), (0.6, -40.0)]


def quat_mul(a, b):
    """Hamilton product of xyzw quaternions"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def scene_box(flat):
    pts = [np.asarray(flat.camera[0], "<f4")[None, :]]
    r = np.abs(flat.spheres["r"])[:, None]
    pts += [flat.spheres["center"] - r, flat.spheres["center"] + r, flat.boxes["min"], flat.boxes["max"]]
    r = np.abs(flat.cylinders["r"])[:, None]
    for end in (flat.cylinders["base"], flat.cylinders["base"] + flat.cylinders["axis"]):
        pts += [end - r, end + r]
    pts += [np.asarray(m["vertices"], "<f4").reshape(-1, 3) for m in flat.meshes]
    pts = np.concatenate([np.asarray(q, "<f4").reshape(-1, 3) for q in pts])
    return pts.min(axis=0), pts.max(axis=0)


def poses(scene, flat):
    """[(p, quat_xyzw, ratio)] for MOVES"""
    si = scene.info()
    p0 = np.array([si.camera_p.x, si.camera_p.y, si.camera_p.z], "<f4")
    q0 = np.array(list(si.camera_quat_xyzw), dtype=np.float64)
    lo, hi = scene_box(flat)
    centre = (lo.astype(np.float64) + hi) / 2
    out = []
    for f, yaw in MOVES:
        p = (p0 + f * (centre - p0)).astype("<f4")
        a = np.radians(yaw) / 2
        q = quat_mul(np.array([0.0, 0.0, np.sin(a), np.cos(a)]), q0).astype("<f4") if yaw else q0.astype("<f4")
        out.append((p, q, si.camera_height_ratio))
    return out
