"""Limits for the occlusion queries and what they must give (test infrastructure, next to raycast_cases.py): shared by the GPU
tests (tests/test_gpu_occluded.py) and the host-compiled lane code's (tests/test_query_lanes_host.py)."""
import numpy as np

F32 = np.float32
FLT_MAX = F32(3.4028235e38)
INF = F32(np.inf)
RUNGS = ["-inf", "-1", "-0.0", "0", "t/2", "prev(t)", "t", "next(t)", "2t", "FLT_MAX", "+inf", "NaN"]


def ladder(t):
    """(len(t), 12) limits: the rungs of RUNGS for every expected distance"""
    t = np.asarray(t, "<f4")
    with np.errstate(over="ignore", invalid="ignore"):
        cols = [np.full_like(t, -INF), np.full_like(t, -1), np.full_like(t, -0.0), np.zeros_like(t), t * F32(0.5),
                np.nextafter(t, -INF), t, np.nextafter(t, INF), t * F32(2), np.full_like(t, FLT_MAX), np.full_like(t, INF),
                np.full_like(t, np.nan)]
    out = np.stack(cols, axis=1).astype("<f4")
    assert out.shape[1] == len(RUNGS)
    return out


def expected(t, mat, tmax):
    """the contract, as it reads"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(mat) != 0) & (np.asarray(t, "<f4") < np.asarray(tmax, "<f4"))


def laddered(rays, t, mat):
    """every ray once per rung, all rungs in one batch -> (rays, tmax, expected, rung index)"""
    lad = ladder(t)
    k = lad.shape[1]
    rr = np.repeat(np.ascontiguousarray(rays, "<f4"), k, axis=0)
    tm = lad.reshape(-1)
    want = expected(np.repeat(t, k), np.repeat(mat, k), tm)
    return rr, tm, want, np.tile(np.arange(k), len(t))


def drawn_limits(rng, t):
    """per ray one of prev(t), t, next(t), t * U(0, 2), +inf"""
    t = np.asarray(t, "<f4")
    with np.errstate(over="ignore", invalid="ignore"):
        choice = np.stack([np.nextafter(t, -INF), t, np.nextafter(t, INF), (t * rng.uniform(0, 2, len(t)).astype("<f4")).astype("<f4"),
                           np.full_like(t, INF)], axis=1)
    return choice[np.arange(len(t)), rng.integers(0, 5, len(t))].astype("<f4")
