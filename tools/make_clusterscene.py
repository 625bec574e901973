#!/usr/bin/env python3
"""A scene whose fast tree can hold FULL leaves: the leaf word of csrc/ort_scene.h counts up to 16 primitives (MAX_LEAF_PRIMS),
the builder's defaults stop at 4 triangles and 2 analytic shapes, and the repository's other scenes never get past 6 under any
setting of ORT_LEAF_TRI / ORT_LEAF_OTHER.  Here, in the closed room of tools/make_tablescene.py and under its camera, four
clusters stand in the plane through the centre of the view, one per primitive kind, each of shapes that overlap heavily and
share a box centre, so that no split by centroid pays and the builder, allowed 16 to a leaf, puts 16 there:

  * spheres: 16 concentric shells, the outer ones transmissive (paths get inside), then diffuse and specular ones in turn;
  * boxes: 24 boxes about one centre, each a little wider and a little flatter than the last so that every one shows, every
    other one transmissive.  The default analytic prologue (14 box tests' worth: the six walls and the eight largest of these)
    leaves 16 of them to the tree;
  * cylinders: 16 coaxial cylinders on one slanted axis through one centre, the thinner the longer;
  * triangles: a "book" of 16 triangles that share one edge, the diagonal of a box, their third vertices inside that box: all
    sixteen have the same bounds exactly.

Next to each cluster, off its centre, the ties (what the reference decides by the order of its own walk, ray.cpp's strict <):

  * two spheres that are exact duplicates under different materials, and two such cylinders;
  * two boxes whose top faces lie in one plane and overlap, different materials;
  * two triangles in one plane that overlap, in two meshes of different materials (the second mesh holds these alone).

One large sphere light over the clusters; every cylinder is on the light list as well (the reference puts them there), 19
lights and 23 materials with index 0: within the kernels' LDS tables (48 and 64, csrc/ort_plan.h), so the table kernels,
the ray exchange and the wide tree all run on it, and within the .scn grammar's counts.

write_scene() writes cluster.scn, cluster_a.ply and cluster_b.ply (what tools/host_sim and Scene.load_scn read; the tests
use this form everywhere); arrays() gives the same layout as Scene.from_arrays arguments (the decimal text of the .scn
goes through the loaders' own scaling, so the two agree to the last digit written, not to the bit).
usage: make_clusterscene.py out_dir"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_tablescene as mt  # noqa: E402

N_LEAF = 16                      # MAX_LEAF_PRIMS
# material indices, in file order (0 is "no hit")
MAT_WALL0, MAT_LIGHT = 1, 7
MAT_SPH_GLASS, MAT_SPH_DIFF, MAT_SPH_SPEC, MAT_SPH_DUP = 8, 9, 10, (11, 12)
MAT_BOX_GLASS, MAT_BOX_DIFF, MAT_BOX_FACE = 13, 14, (15, 16)
MAT_CYL_DIFF, MAT_CYL_SPEC, MAT_CYL_DUP = 17, 18, (19, 20)
MAT_MESH_A, MAT_MESH_B = 21, 22
N_MATERIALS = 23
Z3 = (0.0, 0.0, 0.0)
BRDF = {
    MAT_SPH_GLASS: ((0.05, 0.05, 0.08), Z3, 10, (0.9, 0.9, 0.85), 1.5),
    MAT_SPH_DIFF: ((0.8, 0.3, 0.2), Z3, 10, Z3, 1.0),
    MAT_SPH_SPEC: ((0.2, 0.2, 0.2), (0.7, 0.7, 0.6), 40, Z3, 1.0),
    MAT_SPH_DUP[0]: ((0.1, 0.1, 0.1), Z3, 10, (0.8, 0.9, 0.8), 1.3),
    MAT_SPH_DUP[1]: ((0.2, 0.7, 0.3), Z3, 10, Z3, 1.0),
    MAT_BOX_GLASS: ((0.05, 0.08, 0.05), Z3, 10, (0.85, 0.9, 0.9), 1.4),
    MAT_BOX_DIFF: ((0.3, 0.4, 0.8), Z3, 10, Z3, 1.0),
    MAT_BOX_FACE[0]: ((0.8, 0.8, 0.2), Z3, 10, Z3, 1.0),
    MAT_BOX_FACE[1]: ((0.2, 0.8, 0.8), (0.3, 0.3, 0.3), 20, Z3, 1.0),
    MAT_CYL_DIFF: ((0.7, 0.5, 0.2), Z3, 10, Z3, 1.0),
    MAT_CYL_SPEC: ((0.2, 0.2, 0.3), (0.6, 0.6, 0.7), 60, Z3, 1.0),
    MAT_CYL_DUP[0]: ((0.9, 0.2, 0.6), Z3, 10, Z3, 1.0),
    MAT_CYL_DUP[1]: ((0.1, 0.1, 0.1), Z3, 10, (0.9, 0.8, 0.9), 1.6),
    MAT_MESH_A: ((0.6, 0.6, 0.6), Z3, 10, Z3, 1.0),
    MAT_MESH_B: ((0.9, 0.4, 0.1), Z3, 10, Z3, 1.0),
}
LIGHT_RGB = (2, 2, 2)


def _r6(v):
    """what the .scn holds: six decimals"""
    return np.round(np.asarray(v, np.float64), 6)


def layout():
    """-> dict: the centres of the four clusters, the shapes by kind as (fields..., material), in file order, the vertices of
    the two meshes ((3 n, 3), world space) and where the ties are"""
    u, v, w = mt._basis()
    centre = mt.CAM - mt.DIST * w
    c_sph, c_box = _r6(centre - 0.85 * u + 0.5 * v), _r6(centre + 0.85 * u + 0.5 * v)
    c_cyl, c_tri = _r6(centre - 0.85 * u - 0.5 * v), _r6(centre + 0.85 * u - 0.5 * v)
    L = dict(centres=dict(sphere=c_sph, box=c_box, cylinder=c_cyl, triangle=c_tri), light=(_r6(centre + np.array([0.0, 0.0, 2.3])), 1.1))

    # spheres: radii 0.46 down to 0.40, so close that no split of the sixteen by size beats one leaf (ort_tree.cpp: a leaf costs
    # 1.2 a primitive, a split 1 + 1.2 x the children's area-weighted counts); the four outermost are glass
    radii = _r6(0.46 - 0.004 * np.arange(N_LEAF))
    sph = [(c_sph, radii[k], MAT_SPH_GLASS) for k in range(4)]
    sph += [(c_sph, radii[k], MAT_SPH_DIFF) for k in range(4, N_LEAF, 2)] + [(c_sph, radii[k], MAT_SPH_SPEC) for k in range(5, N_LEAF, 2)]
    dup_c = _r6(c_sph + 0.34 * u - 0.3 * v + 0.1 * w)     # sticks out of the shells, towards the camera and the frame's centre
    sph += [(dup_c, 0.22, MAT_SPH_DUP[0]), (dup_c, 0.22, MAT_SPH_DUP[1])]
    L["spheres"], L["dup_sphere"] = sph, (dup_c, 0.22)

    # boxes: 24 about one centre, none inside another: from box to box the half size grows by 0.004 along x and shrinks by as much
    # along y (the reference's box test reports entries alone, so of nested boxes only the outermost would ever win; of these every
    # one shows a strip of two faces), and shrinks by 0.002 along z; glass and diffuse in turn
    box = []
    for mat, ks in ((MAT_BOX_GLASS, range(0, 24, 2)), (MAT_BOX_DIFF, range(1, 24, 2))):
        for k in ks:
            h = _r6(np.array([0.28 + 0.004 * k, 0.372 - 0.004 * k, 0.33 - 0.002 * k]))
            box.append((_r6(c_box - h), _r6(2 * h), mat))
    # two boxes on top of them, smaller than all of those, whose top faces lie in the plane z = top and overlap
    top = float(_r6(c_box[2] + 0.45))
    p0 = _r6([c_box[0] - 0.22, c_box[1] - 0.20, top - 0.10])
    p1 = _r6([c_box[0] - 0.06, c_box[1] - 0.08, top - 0.07])
    s0, s1 = _r6([0.30, 0.30, top - p0[2]]), _r6([0.30, 0.30, top - p1[2]])
    box += [(p0, s0, MAT_BOX_FACE[0]), (p1, s1, MAT_BOX_FACE[1])]
    L["boxes"] = box
    L["face"] = dict(z=top, lo=np.maximum(p0[:2], p1[:2]), hi=np.minimum(p0[:2] + s0[:2], p1[:2] + s1[:2]))

    # cylinders: one slanted axis through one centre, the thinner the longer (radii 0.220 down by 0.004, lengths up by 0.012: each
    # sticks out of the ends of the thicker ones)
    a1 = 0.55 * u + 0.35 * v + 0.2 * w
    a1 /= np.linalg.norm(a1)
    cyl = []
    for k in range(N_LEAF):
        axis = _r6((0.6 + 0.012 * k) * a1)
        cyl.append((_r6(c_cyl - 0.5 * axis), axis, float(_r6(0.22 - 0.004 * k)), MAT_CYL_DIFF if k % 2 == 0 else MAT_CYL_SPEC))
    base, axis = cyl[0][0], cyl[0][1]
    cyl.sort(key=lambda c: c[3])
    dup_b, dup_a = _r6(c_cyl + 0.1 * u + 0.05 * v + 0.3 * w), _r6(0.1 * u + 0.45 * v)
    cyl += [(dup_b, dup_a, 0.09, MAT_CYL_DUP[0]), (dup_b, dup_a, 0.09, MAT_CYL_DUP[1])]
    L["cylinders"], L["axis"], L["dup_cylinder"] = cyl, (base, axis), (dup_b, dup_a, 0.09)

    # triangles: the book.  lo and hi are the ends of the shared edge, page k turns about it
    lo, hi = _r6(c_tri - [0.4, 0.35, 0.38]), _r6(c_tri + [0.4, 0.35, 0.38])
    va = []
    for k in range(N_LEAF):
        a = 2 * np.pi * k / N_LEAF
        third = _r6(c_tri + np.array([0.37 * np.cos(a), 0.32 * np.sin(a), 0.3 * np.cos(2 * a + 0.4)]))
        va += [lo, hi, third]
    # the two triangles in one plane, facing the camera: the first and a third one in mesh A, the second in mesh B
    q = _r6(c_tri - 0.55 * u + 0.25 * v + 0.45 * w)
    t1 = [q, q + 0.5 * u, q + 0.45 * v]
    t2 = [q + 0.1 * u + 0.05 * v, q + 0.55 * u + 0.1 * v, q + 0.15 * u + 0.5 * v]
    t3 = [q - 0.3 * u - 0.1 * w, q - 0.05 * u - 0.1 * w, q - 0.3 * u + 0.3 * v - 0.1 * w]
    t4 = [q + 0.9 * u - 0.2 * w, q + 1.2 * u - 0.2 * w, q + 0.9 * u + 0.3 * v - 0.2 * w]
    va += [_r6(p) for p in t1 + t3]
    vb = [_r6(p) for p in t2 + t4]
    L["mesh_a"], L["mesh_b"] = np.array(va), np.array(vb)
    # the shared plane, for the tests: a point, the normal, and the two triangles as written
    L["plane"] = dict(p=q, n=w, t1=np.array(va[3 * N_LEAF:3 * N_LEAF + 3]), t2=np.array(vb[0:3]))
    return L


def _statements():
    """the scene in file order: ("brdf", material index) | ("light",) | ("sphere", c, r) | ("box", lo, size) | ("cylinder", base,
    axis, r) | ("mesh", "a" | "b")"""
    L = layout()
    st = []
    for i, (kd, b) in enumerate(mt.WALLS):
        st += [("wall", kd), ("box", np.array(b[:3]), np.array(b[3:]))]
    st += [("light",), ("sphere",) + L["light"]]
    cur = MAT_LIGHT
    for kind, key in (("sphere", "spheres"), ("box", "boxes"), ("cylinder", "cylinders")):
        for s in L[key]:
            assert s[-1] >= cur, "materials go up through the file"
            if s[-1] != cur:
                assert s[-1] == cur + 1
                cur = s[-1]
                st.append(("brdf", cur))
            st.append((kind,) + s[:-1])
    st += [("brdf", MAT_MESH_A), ("mesh", "a"), ("brdf", MAT_MESH_B), ("mesh", "b")]
    return st, L


def _ply(path, v):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float32 x\nproperty float32 y\nproperty float32 z\n"
                "element face %d\nproperty list uint8 int32 vertex_index\nend_header\n" % (len(v), len(v) // 3))
        f.write("".join("%.6f %.6f %.6f\n" % tuple(p) for p in v))
        f.write("".join("3 %d %d %d\n" % (i, i + 1, i + 2) for i in range(0, len(v), 3)))


def write_scene(directory, stem="cluster"):
    """-> (path of the .scn, the layout); <stem>_a.ply (18 triangles) and <stem>_b.ply (2) are written next to it"""
    st, L = _statements()
    f3 = "%.6f %.6f %.6f"
    brdf = lambda kd, ks, alpha, kt, ior: ("brdf " + f3 + " " + f3 + " %d " + f3 + " %.6f") % (tuple(kd) + tuple(ks) + (alpha,) + tuple(kt) + (ior,))
    S = [mt.HEADER.rstrip("\n")]
    for s in st:
        if s[0] == "wall":
            S.append(brdf(s[1], Z3, 10, Z3, 1.0))
        elif s[0] == "brdf":
            S.append(brdf(*BRDF[s[1]]))
        elif s[0] == "light":
            S.append("light %d %d %d" % LIGHT_RGB)
        elif s[0] == "sphere":
            S.append(("sphere " + f3 + " %.6f") % (tuple(s[1]) + (s[2],)))
        elif s[0] == "box":
            S.append(("box " + f3 + " " + f3) % (tuple(s[1]) + tuple(s[2])))
        elif s[0] == "cylinder":
            S.append(("cylinder " + f3 + " " + f3 + " %.6f") % (tuple(s[1]) + tuple(s[2]) + (s[3],)))
        else:
            _ply(os.path.join(directory, "%s_%s.ply" % (stem, s[1])), L["mesh_" + s[1]])
            S.append("mesh %s_%s.ply  0.000000 0.000000 0.000000 1.000000  q 1.000000 0.000000 0.000000 0.000000" % (stem, s[1]))
    scn = os.path.join(directory, stem + ".scn")
    with open(scn, "w") as f:
        f.write("\n".join(S) + "\n")
    return scn, L


def arrays():
    """-> (keyword arguments of offline_raytracer_amd.api.Scene.from_arrays, the layout)"""
    st, L = _statements()
    mats = [(Z3, (0, 0, 0, 0), Z3, 0.0, Z3, 0)]
    sph, box, cyl, lig, meshes = [], [], [], [], []
    for s in st:
        m = len(mats) - 1
        if s[0] == "wall":
            mats.append((s[1], (0, 0, 0, 10.0), Z3, 1.0, Z3, 0))
        elif s[0] == "brdf":
            kd, ks, alpha, kt, ior = BRDF[s[1]]
            mats.append((kd, tuple(ks) + (float(alpha),), kt, ior, Z3, 0))
        elif s[0] == "light":
            mats.append((Z3, (0, 0, 0, 0), Z3, 0.0, tuple(float(c) for c in LIGHT_RGB), 1))
        elif s[0] == "sphere":
            sph.append((tuple(s[1]), float(s[2]), m))
            if mats[m][5]:
                lig.append((1, len(sph) - 1))
        elif s[0] == "box":
            lo = np.asarray(s[1], "<f4")
            box.append((tuple(lo), tuple(lo + np.asarray(s[2], "<f4")), m))
        elif s[0] == "cylinder":
            cyl.append((tuple(s[1]), tuple(s[2]), float(s[3]), m))
            lig.append((2, len(cyl) - 1))
        else:
            v = L["mesh_" + s[1]].astype("<f4")
            meshes.append(dict(vertices=v, indices=np.arange(len(v), dtype="<u4"), mat=m))
    assert len(mats) == N_MATERIALS
    w_, x_, y_, z_ = mt.CAM_Q_WXYZ
    return dict(materials=mats, spheres=sph, boxes=box, cylinders=cyl, lights=lig, meshes=meshes, camera_p=tuple(mt.CAM),
                camera_quat_xyzw=(x_, y_, z_, w_), camera_height_ratio=0.2, screen=(400, 300), ambient=(0.125, 0.125, 0.125),
                with_reference_csg=True), L


if __name__ == "__main__":
    print(write_scene(sys.argv[1])[0])
