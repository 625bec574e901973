#!/usr/bin/env python3
"""Scenes that cross the caps of the kernels' LDS tables (csrc/ort_plan.h: table_fit_flags -- 48 materials with index 0,
64 lights, 40 float4 of prologue shapes), so that the TABS = false kernels, which read materials, light types and
prologue shapes from HBM, run by themselves, and the scenes AT the caps, which use the last float4 of every table slot.

The closed room of the other scenes; in front of the camera, in the plane through the centre of the view:

  * a grid of small shapes (spheres, boxes, cylinders, two copies of letterX.ply), EACH WITH ITS OWN MATERIAL.  The diffuse
    colour is a hash of the material's index; every third material is specular, every fifth transmissive with an ior of its
    own (lobes=False: all diffuse, the scene then runs the diffuse flavour of the kernels).  A material read at index
    m ^ 1, m & 47, m - 1 or m % 48 is visibly another one;
  * behind the grid one large sphere with the LAST material of the scene: it fills the gaps of the grid and the rim of
    the frame, so a scene of 49 materials has a quarter of its primary hits on index 48;
  * above and below the grid, one large sphere light and rows of small emitters -- spheres and cylinders under `light` materials -- which, together
    with the grid's cylinders, are the light list (the reference puts every cylinder on it, light or not).  The type of
    light i is a hash of i for i < 64 and the opposite of light i - 64 from there on: a flag read at a wrapped or
    shifted index is another flag, and it decides how many RNG steps a bounce takes.  (type[i] != type[i - 64]
    implies type[i] == type[i - 128]: the list is aperiodic for every power of two up to 64, which is the cap.);
  * big_boxes=N: N pillars along the two far walls, larger than every box of the grid, so that the analytic prologue
    (ORT_ANALYTIC_PROLOGUE, read when the scene is committed) takes walls and pillars first: 2 float4 each.

write_scene() writes a .scn in the reference's grammar (at most 100 materials with index 0, 100 spheres, 100 cylinders,
100 boxes: parser.h:195-208); arrays() gives the same layout as from_arrays() arguments for counts beyond that.
usage: make_tablescene.py out_dir [variant]"""
import os
import shutil
import sys

import numpy as np

DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data")
CAM = np.array([5.553228, 2.942755, 2.900874])
CAM_Q_WXYZ = (0.416981, 0.279589, 0.480987, 0.718247)
HEADER = ("screen 400 300\ncamera 5.553228 2.942755 2.900874 b 0.2 q 0.416981 0.279589 0.480987 0.718247\n"
          "ambient 0.125000 0.125000 0.125000\n")
WALLS = [((0.6, 0.6, 0.6), (-3, -3, -0.1, 18, 18, 0.1)), ((0.6, 0.6, 0.6), (-3, -3, 8.9, 18, 18, 0.1)),
         ((0.2, 0.9, 0.2), (-3, -3, -0.1, 0.1, 18, 9)), ((0.9, 0.2, 0.9), (15, -3, -0.1, 0.1, 18, 9)),
         ((0.2, 0.2, 0.9), (-3, -3, -0.1, 18, 0.1, 9)), ((0.9, 0.9, 0.2), (-3, 15, -0.1, 18, 0.1, 9))]
DIST = 6.0             # camera to the plane of the grid
HALF_U, HALF_V = 1.45, 0.78   # half extents of the grid in that plane (the 4:3 frame sees 1.6 x 1.2 there)

# the variants of tests/test_gpu_tables.py, relative to the caps (materials counts index 0)
CAP_MATS, CAP_LIGHTS = 48, 64


def variants(cap_mats=CAP_MATS, cap_lights=CAP_LIGHTS):
    return {
        "at_caps": dict(materials=cap_mats, lights=cap_lights),
        "mats_over": dict(materials=cap_mats + 1, lights=12),
        "mats_over_diffuse": dict(materials=cap_mats + 1, lights=12, lobes=False),
        "lights_over": dict(materials=20, lights=cap_lights + 1),
        "ref_limits": dict(materials=100, lights=100),             # the most the .scn loaders hold,
        "beyond_ref": dict(materials=300, lights=200),       # arrays() only
        "pro_over": dict(materials=20, lights=12, big_boxes=40),
    }


def hash32(i, salt=0):
    x = (int(i) * 2654435761 + salt * 40503 + 12345) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x45D9F3B) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x45D9F3B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def light_types(n, period=CAP_LIGHTS):
    """1 = sphere, 2 = cylinder (ort_light.type)"""
    t = []
    for i in range(n):
        t.append((1 if hash32(i, 7) & 0x100 else 2) if i < period else 3 - t[i - period])
    return t


def material_of(m, lobes=True):
    """(Kd, Ks, alpha, Kt, ior) of surface material m"""
    h = hash32(m, 1)
    kd = tuple(round(0.15 + 0.75 * ((h >> s) & 0xFF) / 255.0, 6) for s in (0, 8, 16))
    ks, kt, ior, alpha = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0, 10 + (h >> 24) % 90
    if lobes and m % 3 == 0:
        ks = tuple(round(0.2 + 0.8 * ((hash32(m, 2) >> s) & 0xFF) / 255.0, 6) for s in (0, 8, 16))
    if lobes and m % 5 == 0:
        kt = tuple(round(0.3 + 0.7 * ((hash32(m, 3) >> s) & 0xFF) / 255.0, 6) for s in (0, 8, 16))
        ior = round(1.05 + 0.6 * ((hash32(m, 4) & 0xFFFF) / 65535.0), 6)
        kd = tuple(round(0.3 * c, 6) for c in kd)
    return kd, ks, alpha, kt, ior


def _basis():
    w, x, y, z = CAM_Q_WXYZ
    ez = np.array([2 * x * z + 2 * w * y, 2 * y * z - 2 * w * x, 1 - 2 * x * x - 2 * y * y])   # the camera's z axis; it looks along -z
    ex = np.array([1 - 2 * y * y - 2 * z * z, 2 * x * y + 2 * w * z, 2 * x * z - 2 * w * y])
    ey = np.cross(ez, ex)
    return ex / np.linalg.norm(ex), ey / np.linalg.norm(ey), ez / np.linalg.norm(ez)


def _quat_wxyz(R):
    """quaternion of the rotation matrix R (columns = images of x, y, z)"""
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    if w > 1e-6:
        return w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)
    x = np.sqrt(max(0.0, 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2
    return (R[2, 1] - R[1, 2]) / (4 * x), x, (R[0, 1] + R[1, 0]) / (4 * x), (R[0, 2] + R[2, 0]) / (4 * x)


def layout(materials, lights, lobes=True, big_boxes=0):
    """The scene as a list of statements in file order: ("brdf", Kd, Ks, alpha, Kt, ior) | ("light", r, g, b) |
    ("sphere", c, r) | ("box", lo, size) | ("cylinder", base, axis, r) | ("mesh", translate, scale, quat_wxyz), and its counts.
    materials counts index 0, the "no hit" material, as the table cap does."""
    u, v, w = _basis()
    centre = CAM - DIST * w
    types = light_types(lights)
    nseg = min(4, max(1, lights // 4))
    n_grid = materials - 1 - len(WALLS) - nseg - 1 - (1 if big_boxes else 0)
    if n_grid < 4:
        raise ValueError("materials=%d leaves no material for the grid" % materials)
    st = []
    mat = [0]          # index of the current material

    def brdf():
        mat[0] += 1
        st.append(("brdf",) + material_of(mat[0], lobes))

    for kd, box in WALLS:
        mat[0] += 1
        st.append(("brdf", kd, (0.0, 0.0, 0.0), 10, (0.0, 0.0, 0.0), 1.0))
        st.append(("box", box[:3], box[3:]))
    if big_boxes:       # pillars along the far walls (x = -3 and y = -3), one material
        brdf()
        for k in range(big_boxes):
            t = -2.6 + 17.0 * (k // 2) / max(1, (big_boxes + 1) // 2)
            st.append(("box", (-2.9, t, 0.0, ) if k % 2 == 0 else (t, -2.9, 0.0), (0.35, 0.35, 8.0 - 0.05 * k)))

    cols = int(np.ceil(np.sqrt(n_grid * HALF_U / HALF_V)))
    rows = int(np.ceil(n_grid / cols))
    cell = min(2 * HALF_U / cols, 2 * HALF_V / rows)
    li = [0]
    n_emit = [0]
    per_row = 40

    def emitter():
        e = n_emit[0]
        n_emit[0] += 1
        row, col = e // per_row, e % per_row
        side = 1.0 if row % 2 == 0 else -1.0
        p = centre + (col - (per_row - 1) / 2) * (3.0 / per_row) * u + side * (HALF_V + 0.08 + 0.075 * (row // 2)) * v + 0.1 * w
        if types[li[0]] == 1 and not any(x[0] == "sphere" for x in st):
            st.append(("sphere", centre + np.array([0.0, 0.0, 2.3]), 1.1))   # the one large light, over the grid: what most paths end on
        elif types[li[0]] == 1:
            st.append(("sphere", p, 0.028))
        else:
            st.append(("cylinder", p - 0.03 * v, 0.06 * v, 0.02))
        li[0] += 1

    g = 0
    counts = dict(grid_spheres=0, grid_boxes=0, grid_cylinders=0, grid_meshes=0)
    for s in range(nseg):
        mat[0] += 1
        st.append(("light", 1 + (s + 1) % 2, 1 + s % 2, 1 + (s // 2) % 2))
        # this segment's share of the light list; it stops in front of a cylinder, which the grid's next cylinder then is.
        # The last segment takes all that is left: the grid shapes after it add no light
        target = lights if s == nseg - 1 else (lights * (s + 1)) // nseg
        while li[0] < target or (li[0] < lights and types[li[0]] != 2):
            emitter()
        g_end = n_grid * (s + 1) // nseg
        while g < g_end:
            brdf()
            r, c = g // cols, g % cols
            p = centre + (c - (cols - 1) / 2) * cell * u + (r - (rows - 1) / 2) * cell * v
            kind = ("sphere", "box", "cylinder", "sphere", "box")[g % 5]
            if g in (n_grid // 3, n_grid - 2):
                kind = "mesh"
            if kind == "cylinder" and not (li[0] < lights and types[li[0]] == 2):
                kind = "box"      # the light list has no cylinder at this place
            if kind == "sphere":
                st.append(("sphere", p, 0.36 * cell))
                counts["grid_spheres"] += 1
            elif kind == "box":
                h = 0.29 * cell
                st.append(("box", p - h, (2 * h, 2 * h, 2 * h)))
                counts["grid_boxes"] += 1
            elif kind == "cylinder":
                a = (0.7 * u + 0.7 * v if hash32(g, 5) & 1 else 0.7 * u - 0.7 * v) * 0.6 * cell
                st.append(("cylinder", p - a / 2, a, 0.17 * cell))
                counts["grid_cylinders"] += 1
                li[0] += 1
            else:               # letterX.ply lies in its x-y plane, 1.6 x 2.9: turned to face the camera
                st.append(("mesh", p + 0.02 * w, 0.3 * cell, _quat_wxyz(np.stack([u, v, w], 1))))
                counts["grid_meshes"] += 1
            g += 1
    assert li[0] == lights and g == n_grid, (li[0], lights, g, n_grid)
    brdf()                      # the last material: the large sphere behind everything
    st.append(("sphere", centre - 1.9 * w, 1.6))
    assert mat[0] + 1 == materials
    counts.update(materials=materials, lights=lights, light_types=types, spheres=sum(s_[0] == "sphere" for s_ in st),
                  boxes=sum(s_[0] == "box" for s_ in st), cylinders=sum(s_[0] == "cylinder" for s_ in st),
                  meshes=counts["grid_meshes"], sphere_lights=types.count(1), cyl_lights=types.count(2),
                  triangles=4 * counts["grid_meshes"])
    return st, counts


def write_scene(directory, stem="tablescene", materials=CAP_MATS, lights=CAP_LIGHTS, lobes=True, big_boxes=0):
    """-> (path of the .scn, counts); letterX.ply is copied next to it"""
    st, counts = layout(materials, lights, lobes, big_boxes)
    for kind, cap in (("materials", 100), ("spheres", 100), ("boxes", 100), ("cylinders", 100)):
        if counts[kind] > cap:
            raise ValueError("%d %s: the .scn grammar's loaders hold %d (use arrays())" % (counts[kind], kind, cap))
    f3 = "%.6f %.6f %.6f"
    L = [HEADER.rstrip("\n")]
    for s in st:
        if s[0] == "brdf":
            L.append(("brdf " + f3 + " " + f3 + " %d " + f3 + " %.6f") % (s[1] + s[2] + (s[3],) + s[4] + (s[5],)))
        elif s[0] == "light":
            L.append("light %d %d %d" % s[1:])
        elif s[0] == "sphere":
            L.append(("sphere " + f3 + " %.6f") % (tuple(s[1]) + (s[2],)))
        elif s[0] == "box":
            L.append(("box " + f3 + " " + f3) % (tuple(s[1]) + tuple(s[2])))
        elif s[0] == "cylinder":
            L.append(("cylinder " + f3 + " " + f3 + " %.6f") % (tuple(s[1]) + tuple(s[2]) + (s[3],)))
        else:
            L.append(("mesh letterX.ply  " + f3 + " %.6f  q %.6f %.6f %.6f %.6f") % (tuple(s[1]) + (s[2],) + tuple(s[3])))
    scn = os.path.join(directory, stem + ".scn")
    with open(scn, "w") as f:
        f.write("\n".join(L) + "\n")
    if counts["meshes"] and not os.path.exists(os.path.join(directory, "letterX.ply")):
        shutil.copy(os.path.join(DATA, "letterX.ply"), os.path.join(directory, "letterX.ply"))
    return scn, counts


def arrays(materials=300, lights=200, lobes=True, big_boxes=0):
    """-> (keyword arguments of offline_raytracer_amd.api.Scene.from_arrays, counts): the same layout without the .scn
    grammar's limits; the two meshes are plain quads of four triangles in place of letterX.ply"""
    st, counts = layout(materials, lights, lobes, big_boxes)
    u, v, _ = _basis()
    mats = [((0, 0, 0), (0, 0, 0, 0), (0, 0, 0), 0.0, (0, 0, 0), 0)]
    sph, box, cyl, lig, meshes = [], [], [], [], []
    for s in st:
        m = len(mats) - 1
        if s[0] == "brdf":
            mats.append((s[1], tuple(s[2]) + (float(s[3]),), s[4], s[5], (0, 0, 0), 0))
        elif s[0] == "light":
            mats.append(((0, 0, 0), (0, 0, 0, 0), (0, 0, 0), 0.0, tuple(float(c) for c in s[1:]), 1))
        elif s[0] == "sphere":
            sph.append((tuple(s[1]), s[2], m))
            if mats[m][5]:
                lig.append((1, len(sph) - 1))
        elif s[0] == "box":
            lo = np.asarray(s[1], "<f4")
            box.append((tuple(lo), tuple(lo + np.asarray(s[2], "<f4")), m))
        elif s[0] == "cylinder":
            cyl.append((tuple(s[1]), tuple(s[2]), s[3], m))
            lig.append((2, len(cyl) - 1))
        else:
            h = 1.2 * s[2]
            p = np.asarray(s[1])
            vs = np.array([p, p - h * u - h * v, p + h * u - h * v, p + h * u + h * v, p - h * u + h * v], "<f4")
            meshes.append(dict(vertices=vs, indices=np.array([0, 1, 2, 0, 2, 3, 0, 3, 4, 0, 4, 1], "<u4"), mat=m))
    w_, x_, y_, z_ = CAM_Q_WXYZ
    counts["triangles"] = 4 * len(meshes)
    return dict(materials=mats, spheres=sph, boxes=box, cylinders=cyl, lights=lig, meshes=meshes, camera_p=tuple(CAM),
                camera_quat_xyzw=(x_, y_, z_, w_), camera_height_ratio=0.2, screen=(400, 300), ambient=(0.125, 0.125, 0.125),
                with_reference_csg=False), counts


if __name__ == "__main__":
    kw = variants()[sys.argv[2]] if len(sys.argv) > 2 else {}
    print(write_scene(sys.argv[1], **kw))
