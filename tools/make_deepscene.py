#!/usr/bin/env python3
"""A scene whose fast tree is deep enough that the per-lane traversal stack leaves its LDS entries and runs in the
scratch tail (csrc/ort_lane.h: kLdsStack + kSpillStack, 24 + 40 in the four-waves units, 20 + 44 in the five-waves unit,
16 + 48 in the wavefront trace, the re-traversal of resolve_hit four LDS entries fewer).  A balanced tree cannot get
there (a million triangles give depth 23, and the stack is no deeper than the tree); what does is coordinate range plus
count.  Everything is perpendicular to x, seen from the origin looking down +x:

  * the inner stack: M thin sheets at x = inner_x + i, each ONE narrow wedge-shaped triangle inside the same square,
    along a line at a random angle through a random point near the axis, from edge to edge of the square.  Their boxes
    overlap in every way, the SAH builder (16 centroid bins on three axes) splits them unevenly, and nearly every ray of
    the cone pierces both children of nearly every node: the deepest stack is the number of far children put aside on
    the way down to the first leaf;
  * the outer plates: N such wedges at x = outer_x * ratio ** k in squares of half size 0.6 x.  Their centroids are in
    geometric progression, so the builder peels them off the top of the tree one or two at a time: more levels, and
    more far children, above the inner stack.  (Range alone buys a level per 0.65 to 1.2 decades, and float32 triangles
    and quadrics allow 18: the walls stand at 1e18.);
  * three short, fat, slightly oblique cylinders at the far end.  The reference's boxes around a cylinder are too small
    (DESIGN.md section 3, item 4), so rays that graze one are re-traversed by resolve_hit: the whole deep tree a second
    time, on the re-traversal's shorter LDS part;
  * two sphere lights (one far out, one behind the camera, which is what most lit paths end on) and a closed room of
    six wall boxes around everything, so that no ray goes unanswered.

No region of the cone is kept free of wedges (with every angle allowed the boxes are large, which is what keeps the stack
deep); instead a wedge covers little (inner_cover, outer_cover: its share of its square), so a third of the rays win on the
inner stack, a fifth on an outer plate, and half on a cylinder or a wall behind one.

EVERY COORDINATE IS AN INTEGER THAT float32 HOLDS EXACTLY, written as "N.": the .scn and PLY lexers of the product (and
of the reference) scale decimals by powers of (double)0.1f, which such a literal survives unchanged, so arrays() and
write_scene() describe the same scene bit for bit (tests/test_deep_stack_host.py asserts it).  The colours are 0.25 and
0.5, the camera's quaternion is (+-0.5)^4, for the same reason.  Edges are thousands of units long: every triangle's
determinant is far from the intersector's 1e-6 threshold.

usage: make_deepscene.py out_dir"""
import os
import sys

import numpy as np

INNER_X = 16384                      # the first inner sheet; sheets are one unit apart
OUTER_X = 65536                      # the first outer plate
CAM = (0.0, 0.0, 0.0)
CAM_Q_WXYZ = (0.5, -0.5, -0.5, 0.5)  # camera x -> +y, y -> -z, z -> -x: it looks down +x
CAM_RATIO = 0.25                     # 4:3 frame: slopes up to 1/3 x 1/4, corner 0.417
MAT_WALL, MAT_LIGHT, MAT_CYL, MAT_INNER, MAT_OUTER = 1, 7, 8, 9, 10   # MAT_WALL..6: the six walls

DEFAULT = dict(inner=4096, outer=23, ratio=4, inner_cover=0.00004, outer_cover=0.02, cylinders=3, seed=20251, inner_x=INNER_X, outer_x=OUTER_X, inner_angles=(0, 180), outer_angles=(0, 180), tip_first=False)


def _q(v):
    """-> float32 values that are integers (below 2**23 by rounding; float32 has no fractions from there on)"""
    v = np.asarray(v, np.float64)
    return np.where(np.abs(v) < 2.0 ** 23, np.rint(v), v.astype(np.float32).astype(np.float64)).astype(np.float32)


def _sliver(rng, x, half, cover, angles, tip_first=False):
    """one triangle in the plane at x, inside the square of this half size: a narrow wedge along a line at a random angle
    (degrees, drawn from `angles`) through a random point near the axis, from edge to edge of the square, with
    cover * (0.3 .. 1.7) of the square's area"""
    th = np.radians(rng.uniform(*angles))
    u, v = np.array([np.cos(th), np.sin(th)]), np.array([-np.sin(th), np.cos(th)])
    p = rng.uniform(-0.1, 0.1, 2) * half
    with np.errstate(divide="ignore"):
        t_hi = np.min(np.where(u > 0, (half - p) / u, np.where(u < 0, (-half - p) / u, np.inf)))
        t_lo = -np.min(np.where(u > 0, (half + p) / u, np.where(u < 0, (p - half) / u, np.inf)))
    w = max(1.0, 4.0 * cover * rng.uniform(0.3, 1.7) * half * half / (t_hi - t_lo))
    a, b = p + t_hi * u, p + t_lo * u
    if rng.integers(2):
        a, b = b, a
    c = np.clip([b - w * v, b + w * v], -half, half)
    # the first vertex is one of the two that lie close together: the triangle test's edges from it are one short and one long
    # one, which keeps its distance accurate.  tip_first: from the far tip they are two long, nearly parallel ones, and the
    # computed distance of so thin a triangle is then off by up to 1e-3 of itself, more than the tree walk's culling allows a
    # hit to precede its box (2e-4: DESIGN.md section 3, item 4; tests/test_deep_stack_host.py states that limit on such a scene)
    tri = [(x, c[0][0], c[0][1]), (x, c[1][0], c[1][1]), (x, a[0], a[1])]
    return tri[2:] + tri[:2] if tip_first else tri


def layout(inner, outer, ratio, inner_cover, outer_cover, cylinders, seed, inner_x, outer_x, inner_angles, outer_angles, tip_first):
    """-> dict: inner / outer vertex arrays ((3 n, 3) float32), the sheets' x, the analytic shapes"""
    rng = np.random.default_rng(seed)
    vin = [v for i in range(inner) for v in _sliver(rng, inner_x + i, 0.5 * (inner_x + inner), inner_cover, inner_angles, tip_first)]
    assert inner_x + inner < outer_x
    xs_out = [outer_x * ratio ** k for k in range(outer)]
    vout = [v for x in xs_out for v in _sliver(rng, x, 0.6 * x, outer_cover, outer_angles, tip_first)]
    X = float(xs_out[-1])
    T = X / 64                                                 # wall thickness
    lo, hi, side = -X / 16, 1.25 * X, 0.8 * X
    walls = [((lo - T, -side - T, -side - T), (T, 2 * side + 2 * T, 2 * side + 2 * T)),           # behind the camera
             ((hi, -side - T, -side - T), (T, 2 * side + 2 * T, 2 * side + 2 * T)),               # the far end
             ((lo, -side - T, -side), (hi - lo, T, 2 * side)), ((lo, side, -side), (hi - lo, T, 2 * side)),
             ((lo, -side - T, -side - T), (hi - lo, 2 * side + 2 * T, T)), ((lo, -side - T, side), (hi - lo, 2 * side + 2 * T, T))]
    # short, fat, slightly oblique cylinders off the axis, where the wedges (all through points near the axis) lie thin
    cyl = [((0.50 * X, -0.24 * X, 0.05 * X), (0.02 * X, 0.16 * X, 0.015 * X), 0.045 * X),
           ((0.62 * X, 0.12 * X, -0.09 * X), (0.025 * X, 0.02 * X, 0.17 * X), 0.05 * X),
           ((0.42 * X, 0.02 * X, -0.015 * X), (0.12 * X, 0.012 * X, 0.018 * X), 0.035 * X)][:cylinders]
    return dict(inner=_q(vin), outer=_q(vout), xs_inner=np.arange(inner_x, inner_x + inner), xs_outer=np.array(xs_out, np.float64),
                walls=[(_q(p), _q(s)) for p, s in walls], spheres=[(_q((0.5 * X, 0.58 * X, 0.58 * X)), _q(0.1 * X)), (_q((-0.036 * X, 0, 0)), _q(0.025 * X))],   # the second one behind the camera
                cylinders=[(_q(b), _q(a), _q(r)) for b, a, r in cyl], far=X)


WALL_KD = [(0.5, 0.5, 0.5), (0.5, 0.5, 0.25), (0.25, 0.5, 0.25), (0.5, 0.25, 0.5), (0.25, 0.25, 0.5), (0.5, 0.5, 0.25)]
KD = {MAT_CYL: (0.5, 0.5, 0.25), MAT_INNER: (0.5, 0.25, 0.25), MAT_OUTER: (0.25, 0.5, 0.5)}
LIGHT_RGB = (4, 4, 4)


def arrays(**kw):
    """-> (keyword arguments of offline_raytracer_amd.api.Scene.from_arrays, the layout)"""
    L = layout(**dict(DEFAULT, **kw))
    Z3, Z4 = (0, 0, 0), (0, 0, 0, 0)
    mats = [(Z3, Z4, Z3, 0.0, Z3, 0)]
    mats += [(kd, (0, 0, 0, 10.0), Z3, 1.0, Z3, 0) for kd in WALL_KD]
    mats += [(Z3, Z4, Z3, 0.0, tuple(float(c) for c in LIGHT_RGB), 1)]
    mats += [(KD[m], (0, 0, 0, 10.0), Z3, 1.0, Z3, 0) for m in (MAT_CYL, MAT_INNER, MAT_OUTER)]
    boxes = [(tuple(p), tuple(p + s), MAT_WALL + i) for i, (p, s) in enumerate(L["walls"])]
    sph = [(tuple(c), float(r), MAT_LIGHT) for c, r in L["spheres"]]
    cyl = [(tuple(b), tuple(a), float(rr), MAT_CYL) for b, a, rr in L["cylinders"]]
    lights = [(1, i) for i in range(len(sph))] + [(2, i) for i in range(len(cyl))]
    meshes = [dict(vertices=L[k], indices=np.arange(len(L[k]), dtype="<u4"), mat=m) for k, m in (("inner", MAT_INNER), ("outer", MAT_OUTER))]
    w, x, y, z = CAM_Q_WXYZ
    return dict(materials=mats, spheres=sph, boxes=boxes, cylinders=cyl, lights=lights, meshes=meshes, camera_p=CAM,
                camera_quat_xyzw=(x, y, z, w), camera_height_ratio=CAM_RATIO, screen=(400, 300), ambient=(0.25, 0.25, 0.25),
                with_reference_csg=True), L   # as every scene loaded from a .scn has it


def _n(v):
    v = float(v)
    assert v == int(v) and np.float32(v) == v, v
    return "%d." % int(v)


def _ply(path, v):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float32 x\nproperty float32 y\nproperty float32 z\n"
                "element face %d\nproperty list uint8 int32 vertex_index\nend_header\n" % (len(v), len(v) // 3))
        f.write("".join("%s %s %s\n" % (_n(a), _n(b), _n(c)) for a, b, c in v))
        f.write("".join("3 %d %d %d\n" % (i, i + 1, i + 2) for i in range(0, len(v), 3)))


def write_scene(directory, stem="deepscene", **kw):
    """-> (path of the .scn, the layout); inner.ply and outer.ply are written next to it"""
    L = layout(**dict(DEFAULT, **kw))
    brdf = lambda kd: "brdf %g %g %g 0. 0. 0. 10 0. 0. 0. 1." % kd
    v3 = lambda a: " ".join(_n(c) for c in a)
    S = ["screen 400 300", "camera %s b %g q %g %g %g %g" % ((v3(CAM), CAM_RATIO) + CAM_Q_WXYZ), "ambient 0.25 0.25 0.25"]
    for kd, (p, s) in zip(WALL_KD, L["walls"]):
        S += [brdf(kd), "box %s %s" % (v3(p), v3(s))]
    S += ["light %d %d %d" % LIGHT_RGB] + ["sphere %s %s" % (v3(c), _n(r)) for c, r in L["spheres"]] + [brdf(KD[MAT_CYL])]
    S += ["cylinder %s %s %s" % (v3(b), v3(a), _n(r)) for b, a, r in L["cylinders"]]
    for k, m in (("inner", MAT_INNER), ("outer", MAT_OUTER)):
        _ply(os.path.join(directory, k + ".ply"), L[k])
        S += [brdf(KD[m]), "mesh %s.ply 0. 0. 0. 1. q 1. 0. 0. 0." % k]
    scn = os.path.join(directory, stem + ".scn")
    with open(scn, "w") as f:
        f.write("\n".join(S) + "\n")
    return scn, L


if __name__ == "__main__":
    print(write_scene(sys.argv[1])[0])
