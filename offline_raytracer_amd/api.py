"""ctypes binding of libort.so -- the C ABI of include/ort.h.

Python here is plumbing (tests, bench.py, torch.distributed launch); the host side of the
product is C++ (offline_raytracer_amd/csrc) and the compute is HIP.  Every render entry
point raises unless the HIP library is built and the scene is resident on a GPU: there is
no CPU fallback for the render call.
"""
import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ORT_LIB", os.path.join(PKG_DIR, "lib", "libort.so"))  # ORT_LIB: tuning builds only
CSRC_DIR = os.path.join(PKG_DIR, "csrc")

OK, ERR_INVALID, ERR_IO, ERR_PARSE, ERR_NO_DEVICE, ERR_HIP, ERR_UNSUPPORTED, ERR_STATE, ERR_NO_MEMORY, ERR_INTERNAL = range(10)
POLICY_TILE32, POLICY_WHOLE, POLICY_PIXEL, POLICY_CHUNK = range(4)
POLICIES = {"tile32": POLICY_TILE32, "whole": POLICY_WHOLE, "pixel": POLICY_PIXEL, "chunk": POLICY_CHUNK}
RENDER_COUNTERS = 1
RENDER_PACKED = 2
COMM_ID_BYTES = 128
HIT_TRIANGLE, HIT_BOX, HIT_CYLINDER, HIT_SPHERE = 0, 2, 3, 4
NO_PRIM = 0xFFFFFFFF
AO_INVALID = 0xFFFFFFFF  # ORT_AO_INVALID: ambient_occlusion()'s open count of a point outside the domain
SH_COEFFS = 9            # ORT_SH_COEFFS: probe_sh()'s coefficients per point and colour channel, bands 0 to 2
MAX_VIEWS = 4096  # ORT_MAX_VIEWS
MAX_LIGHT_GROUPS = 8     # ORT_MAX_LIGHT_GROUPS
NO_LIGHT_GROUP = 0xFF    # ORT_NO_LIGHT_GROUP: a light that is in no group
MAX_DEPTH_BINS = 8       # ORT_MAX_DEPTH_BINS
DEPTH_EMISSION, DEPTH_DIRECT, DEPTH_INDIRECT = 0, 1, 2   # ORT_DEPTH_*: the bins of a three-bin path-depth render


class OrtError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("ort error %d: %s" % (code, message))
        self.code = code


class V3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


MATERIAL_DTYPE = np.dtype([("diffuse", "<f4", 3), ("specular", "<f4", 4), ("transmission", "<f4", 3),
                           ("ior", "<f4"), ("emit", "<f4", 3), ("is_light", "<i4")])
SPHERE_DTYPE = np.dtype([("center", "<f4", 3), ("r", "<f4"), ("mat", "<u4")])
BOX_DTYPE = np.dtype([("min", "<f4", 3), ("max", "<f4", 3), ("mat", "<u4")])
CYLINDER_DTYPE = np.dtype([("base", "<f4", 3), ("axis", "<f4", 3), ("r", "<f4"), ("mat", "<u4")])
LIGHT_DTYPE = np.dtype([("type", "<u4"), ("index", "<u4")])
JOB_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("rng_state", "<u4"),
                      ("spp", "<u4")])


class Mesh(C.Structure):
    _fields_ = [("vertices", C.c_void_p), ("vertex_count", C.c_uint32), ("indices", C.c_void_p),
                ("index_count", C.c_uint32), ("mat", C.c_uint32), ("aabb_min", V3), ("aabb_max", V3)]


class SceneDesc(C.Structure):
    _fields_ = [("materials", C.c_void_p), ("material_count", C.c_uint32),
                ("spheres", C.c_void_p), ("sphere_count", C.c_uint32),
                ("boxes", C.c_void_p), ("box_count", C.c_uint32),
                ("cylinders", C.c_void_p), ("cylinder_count", C.c_uint32),
                ("meshes", C.c_void_p), ("mesh_count", C.c_uint32),
                ("lights", C.c_void_p), ("light_count", C.c_uint32),
                ("camera_p", V3), ("camera_quat_xyzw", C.c_float * 4), ("camera_height_ratio", C.c_float),
                ("screen_width", C.c_int32), ("screen_height", C.c_int32), ("ambient", V3),
                ("with_reference_csg", C.c_int32)]


class SceneInfo(C.Structure):
    _fields_ = [("material_count", C.c_uint32), ("sphere_count", C.c_uint32), ("box_count", C.c_uint32),
                ("cylinder_count", C.c_uint32), ("mesh_count", C.c_uint32), ("light_count", C.c_uint32),
                ("triangle_count", C.c_uint32), ("screen_width", C.c_int32), ("screen_height", C.c_int32),
                ("ambient", V3), ("camera_p", V3), ("camera_quat_xyzw", C.c_float * 4),
                ("camera_height_ratio", C.c_float)]


class TreeInfo(C.Structure):
    _fields_ = [("node_count", C.c_uint32), ("leaf_count", C.c_uint32), ("max_leaf_prims", C.c_uint32),
                ("max_depth", C.c_uint32), ("node_bytes", C.c_uint64), ("prim_bytes", C.c_uint64),
                ("sah_cost", C.c_float), ("ref_node_count", C.c_uint32), ("ref_nonempty_leaves", C.c_uint32),
                ("ref_max_leaf_records", C.c_uint32), ("ref_bytes", C.c_uint64), ("prologue_prims", C.c_uint32),
                ("wide_node_count", C.c_uint32), ("wide_max_depth", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("paths", C.c_uint64), ("rays", C.c_uint64), ("node_tests", C.c_uint64), ("tri_tests", C.c_uint64),
                ("analytic_tests", C.c_uint64), ("fallback_rays", C.c_uint64), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Adaptive(C.Structure):
    """ort_adaptive: the stopping rule of an adaptive radiance query."""
    _fields_ = [("min_spp", C.c_uint32), ("max_spp", C.c_uint32), ("check_every", C.c_uint32), ("tolerance", C.c_float),
                ("floor", C.c_float)]


assert C.sizeof(Adaptive) == 20


class RenderParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32),
                ("x1", C.c_int32), ("y1", C.c_int32), ("policy", C.c_int32), ("seed", C.c_uint32),
                ("spp", C.c_uint32), ("chunk", C.c_uint32), ("rr", C.c_float), ("flags", C.c_uint32),
                ("shard_index", C.c_uint32), ("shard_count", C.c_uint32)]


class Camera(C.Structure):
    _fields_ = [("p", V3), ("x_axis", V3), ("y_axis", V3), ("z_axis", V3)]


class View(C.Structure):
    """ort_view: one frame of a batch (ort_render_views): its camera basis and its seed."""
    _fields_ = [("camera", Camera), ("seed", C.c_uint32)]


VIEW_DTYPE = np.dtype([("camera", "<f4", (4, 3)), ("seed", "<u4")])
assert VIEW_DTYPE.itemsize == C.sizeof(View) == 52


class FeaturePlanes(C.Structure):
    """ort_feature_planes: where a first-hit feature render writes (ort_render_features); a null pointer is a plane not asked for."""
    _fields_ = [("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("hits", C.c_void_p), ("ids", C.c_void_p),
                ("final_states", C.c_void_p)]


class FollowPlanes(C.Structure):
    """ort_follow_planes: where a feature render that follows mirrors and glass writes (ort_render_follow); a null pointer is a
    plane not asked for."""
    _fields_ = [("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("hits", C.c_void_p), ("ids", C.c_void_p),
                ("bounces", C.c_void_p), ("final_states", C.c_void_p)]


assert C.sizeof(FollowPlanes) == 56


class Matte(C.Structure):
    """ort_matte: what an ID-matte render names a hit by (MATTE_BY) and the slots per pixel"""
    _fields_ = [("by", C.c_uint32), ("slots", C.c_uint32)]


class MattePlanes(C.Structure):
    """ort_matte_planes: where an ID-matte render writes (ort_render_matte); ids and counts are required, a null pointer among the
    others is a plane not asked for."""
    _fields_ = [("ids", C.c_void_p), ("counts", C.c_void_p), ("other", C.c_void_p), ("hits", C.c_void_p), ("final_states", C.c_void_p)]


assert C.sizeof(MattePlanes) == 40 and C.sizeof(Matte) == 8


class LightGroups(C.Structure):
    _fields_ = [("group_of_material", C.c_void_p), ("material_count", C.c_uint32), ("group_count", C.c_uint32)]


class DenoiseParams(C.Structure):
    """ort_denoise_params"""
    _fields_ = [("iterations", C.c_uint32), ("normal_squarings", C.c_uint32), ("sigma_l", C.c_float), ("sigma_z", C.c_float)]


class DenoisePlanes(C.Structure):
    """ort_denoise_planes: the six planes a denoise call reads, all required"""
    _fields_ = [("rgb", C.c_void_p), ("m2", C.c_void_p), ("count", C.c_void_p), ("albedo", C.c_void_p), ("normal", C.c_void_p),
                ("depth", C.c_void_p)]


# denoise()'s defaults: the best of the grid of profiles/r25_denoise.md (RMSE against 16 384 spp, summed over two scenes at 64 and 256 spp)
DENOISE_DEFAULTS = dict(iterations=4, normal_squarings=7, sigma_l=8.0, sigma_z=0.02)


class PlanParams(C.Structure):
    """ort_plan_params"""
    _fields_ = [("tolerance", C.c_float), ("floor", C.c_float), ("radius", C.c_uint32), ("pilot", C.c_uint32), ("min_add", C.c_uint32),
                ("cap", C.c_uint32), ("rgb_is_sum", C.c_uint32), ("reserved", C.c_uint32), ("budget", C.c_uint64)]


class PlanPlanes(C.Structure):
    """ort_plan_planes: the three planes a plan reads, all required"""
    _fields_ = [("rgb", C.c_void_p), ("m2", C.c_void_p), ("count", C.c_void_p)]


class PlanTotals(C.Structure):
    """ort_plan_totals: 32 bytes per frame"""
    _fields_ = [("wanted", C.c_uint64), ("planned", C.c_uint64), ("unconverged", C.c_uint32), ("unknown", C.c_uint32), ("invalid", C.c_uint32),
                ("worst", C.c_float)]

    def as_dict(self):
        return dict(wanted=int(self.wanted), planned=int(self.planned), unconverged=int(self.unconverged), unknown=int(self.unknown),
                    invalid=int(self.invalid), worst=np.float32(self.worst))


PLAN_TOTALS_DTYPE = np.dtype([("wanted", "<u8"), ("planned", "<u8"), ("unconverged", "<u4"), ("unknown", "<u4"), ("invalid", "<u4"), ("worst", "<f4")])
# plan_samples()'s defaults: the floor of the adaptive calls, a 3 x 3 window as the measured two-pass scheme (profiles/r23_sample_map.md)
PLAN_DEFAULTS = dict(floor=0.05, radius=1, pilot=16, min_add=1, cap=1024)


class AccumPlanes(C.Structure):
    """ort_accum_planes: the caller's planes of an accumulating render (ort_render_accumulate), read and written; m2 may be null."""
    _fields_ = [("sum_rgb", C.c_void_p), ("m2", C.c_void_p), ("count", C.c_void_p), ("states", C.c_void_p)]


FEATURE_PLANES = ("albedo", "normal", "depth", "hits", "ids", "states")   # render_features()'s want=
FOLLOW_PLANES = ("albedo", "normal", "depth", "hits", "ids", "bounces", "states")   # render_follow()'s want=
MAX_FOLLOW_BOUNCES = 64   # ORT_MAX_FOLLOW_BOUNCES
MATTE_PLANES = ("ids", "counts", "other", "hits", "states")   # render_matte()'s planes; want= names the last three
MATTE_BY = {"material": 0, "object": 1, "prim": 2}   # ORT_MATTE_BY_*
MATTE_EMPTY = 0xFFFFFFFF   # ORT_MATTE_EMPTY
HIT_MESH = 1               # ORT_HIT_MESH: the kind of an object id that names a mesh
MAX_MATTE_SLOTS = 8        # ORT_MAX_MATTE_SLOTS
MAX_MATTE_SELECT = 256     # ORT_MAX_MATTE_SELECT


class Hit(C.Structure):
    """ort_hit: the closest hit of one ray (raycast_top_most_node's hit_t, hit_normal, hit_mat_index) and its shape."""
    _fields_ = [("t", C.c_float), ("n", V3), ("mat", C.c_uint32), ("prim", C.c_uint32)]


HIT_DTYPE = np.dtype([("t", "<f4"), ("n", "<f4", 3), ("mat", "<u4"), ("prim", "<u4")])
assert HIT_DTYPE.itemsize == C.sizeof(Hit) == 24


# every symbol include/ort.h declares
EXPORTS = [
    "ort_last_error", "ort_abi_version", "ort_scene_load_scn", "ort_scene_parse_scn", "ort_scene_create",
    "ort_scene_destroy", "ort_scene_get_info", "ort_scene_get_materials", "ort_scene_get_spheres",
    "ort_scene_get_boxes", "ort_scene_get_cylinders", "ort_scene_get_lights", "ort_scene_get_mesh",
    "ort_scene_get_camera", "ort_scene_commit", "ort_scene_get_tree_info", "ort_device_count", "ort_scene_upload",
    "ort_tiled_raytrace", "ort_tiled_raytrace_batch", "ort_render_image", "ort_render_image_device",
    "ort_render_workspace_bytes", "ort_unit_eval_device", "ort_rgbe", "ort_write_hdr",
    "ort_shard_block_count", "ort_pack_blocks_host", "ort_unpack_blocks_host", "ort_unpack_blocks_device",
    "ort_comm_unique_id", "ort_comm_create", "ort_comm_create_local", "ort_comm_destroy", "ort_gather_framebuffer",
    "ort_gather_framebuffer_local", "ort_raycast", "ort_raycast_device",
    "ort_occluded", "ort_occluded_device", "ort_ambient_occlusion", "ort_ambient_occlusion_device",
    "ort_radiance", "ort_radiance_device",
    "ort_radiance_adaptive", "ort_radiance_adaptive_device",
    "ort_irradiance", "ort_irradiance_device", "ort_irradiance_adaptive", "ort_irradiance_adaptive_device",
    "ort_probe_sh", "ort_probe_sh_device",
    "ort_camera_from_pose", "ort_render_views", "ort_render_views_device", "ort_render_views_workspace_bytes",
    "ort_render_adaptive", "ort_render_adaptive_device", "ort_render_views_adaptive", "ort_render_views_adaptive_device",
    "ort_render_features", "ort_render_features_device", "ort_render_views_features", "ort_render_views_features_device",
    "ort_render_follow", "ort_render_follow_device", "ort_render_views_follow", "ort_render_views_follow_device",
    "ort_render_matte", "ort_render_matte_device", "ort_render_views_matte", "ort_render_views_matte_device",
    "ort_matte_mask", "ort_matte_mask_device",
    "ort_render_light_groups", "ort_render_light_groups_device", "ort_render_views_light_groups",
    "ort_render_views_light_groups_device",
    "ort_render_depths", "ort_render_depths_device", "ort_render_views_depths", "ort_render_views_depths_device",
    "ort_render_sample_map", "ort_render_sample_map_device", "ort_render_views_sample_map", "ort_render_views_sample_map_device",
    "ort_render_accumulate", "ort_render_accumulate_device", "ort_render_views_accumulate", "ort_render_views_accumulate_device",
    "ort_denoise_workspace_bytes", "ort_denoise", "ort_denoise_device",
    "ort_plan_samples_workspace_bytes", "ort_plan_samples", "ort_plan_samples_device"]

_lib = None


def build_library():
    """Compile the HIP extension in-tree (hipcc --offload-arch=gfx950)."""
    subprocess.check_call(["make", "-s", "-j5", "-C", CSRC_DIR])   # five kernel units, one job each


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  libort.so needs libamdhip64.so.7 and finds the system's (/opt/rocm); PyTorch ships
    its own copy under torch/lib and asks for it by file name, so if libort.so is loaded BEFORE torch the process ends
    up with two runtimes and the second one to initialise finds "no ROCm-capable device".  Loading torch's copy first
    (without importing torch) makes both resolve to the same library whatever the import order.  Only where torch is
    installed and only for this Python binding; the C++ driver uses the system runtime.  ORT_SYSTEM_HIP=1 opts out."""
    if os.environ.get("ORT_SYSTEM_HIP") == "1":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(path):
            C.CDLL(path, mode=C.RTLD_GLOBAL)
    except Exception:  # noqa: BLE001 -- best effort: without it the import order decides, as before
        pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OrtError(ERR_STATE, "libort.so is not built (run offline_raytracer_amd.api.build_library() or "
                                      "make -C offline_raytracer_amd/csrc); there is no fallback implementation")
        _share_hip_runtime_with_torch()
        L = C.CDLL(LIB_PATH)
        L.ort_last_error.restype = C.c_char_p
        L.ort_scene_load_scn.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]
        L.ort_scene_parse_scn.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.POINTER(C.c_void_p)]
        L.ort_scene_create.argtypes = [C.POINTER(SceneDesc), C.POINTER(C.c_void_p)]
        L.ort_scene_destroy.argtypes = [C.c_void_p]
        L.ort_scene_destroy.restype = None
        L.ort_scene_get_info.argtypes = [C.c_void_p, C.POINTER(SceneInfo)]
        for name in ("materials", "spheres", "boxes", "cylinders", "lights"):
            getattr(L, "ort_scene_get_" + name).argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.ort_scene_get_mesh.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(Mesh)]
        L.ort_scene_get_camera.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(Camera)]
        L.ort_scene_commit.argtypes = [C.c_void_p]
        L.ort_scene_get_tree_info.argtypes = [C.c_void_p, C.POINTER(TreeInfo)]
        L.ort_device_count.argtypes = [C.POINTER(C.c_int)]
        L.ort_scene_upload.argtypes = [C.c_void_p, C.c_int]
        L.ort_tiled_raytrace.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_int32, C.POINTER(C.c_uint32), C.c_uint32, C.c_float,
                                         C.POINTER(C.c_uint64)]
        L.ort_tiled_raytrace_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_uint32,
                                               C.c_float, C.c_void_p, C.POINTER(Stats)]
        L.ort_render_workspace_bytes.argtypes = [C.POINTER(RenderParams), C.POINTER(C.c_uint64)]
        L.ort_unit_eval_device.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
        # host form / device form pairs: the device form takes the same arguments and a stream before the stats
        vp, stats = C.c_void_p, C.POINTER(Stats)
        for name, argtypes in (
                ("ort_render_image", [vp, C.POINTER(RenderParams), vp, stats]),
                ("ort_render_views", [vp, C.POINTER(RenderParams), vp, C.c_uint32, vp, stats]),
                ("ort_render_adaptive", [vp, C.POINTER(RenderParams), C.POINTER(Adaptive), vp, vp, vp, vp, stats]),
                ("ort_render_views_adaptive", [vp, C.POINTER(RenderParams), C.POINTER(Adaptive), vp, C.c_uint32, vp, vp, vp, vp, stats]),
                ("ort_render_light_groups", [vp, C.POINTER(RenderParams), C.POINTER(LightGroups), vp, vp, vp, stats]),
                ("ort_render_views_light_groups", [vp, C.POINTER(RenderParams), C.POINTER(LightGroups), vp, C.c_uint32, vp, vp, vp, stats]),
                ("ort_render_depths", [vp, C.POINTER(RenderParams), C.c_uint32, vp, vp, vp, vp, stats]),
                ("ort_render_views_depths", [vp, C.POINTER(RenderParams), C.c_uint32, vp, C.c_uint32, vp, vp, vp, vp, stats]),
                ("ort_render_sample_map", [vp, C.POINTER(RenderParams), vp, vp, vp, vp, stats]),
                ("ort_render_views_sample_map", [vp, C.POINTER(RenderParams), vp, C.c_uint32, vp, vp, vp, vp, stats]),
                ("ort_render_accumulate", [vp, C.POINTER(RenderParams), C.POINTER(AccumPlanes), vp, vp, stats]),
                ("ort_render_views_accumulate", [vp, C.POINTER(RenderParams), vp, C.c_uint32, C.POINTER(AccumPlanes), vp, vp, stats]),
                ("ort_render_features", [vp, C.POINTER(RenderParams), C.POINTER(FeaturePlanes), stats]),
                ("ort_render_views_features", [vp, C.POINTER(RenderParams), vp, C.c_uint32, C.POINTER(FeaturePlanes), stats]),
                ("ort_render_follow", [vp, C.POINTER(RenderParams), C.c_uint32, C.POINTER(FollowPlanes), stats]),
                ("ort_render_views_follow", [vp, C.POINTER(RenderParams), vp, C.c_uint32, C.c_uint32, C.POINTER(FollowPlanes), stats]),
                ("ort_render_matte", [vp, C.POINTER(RenderParams), C.POINTER(Matte), C.POINTER(MattePlanes), stats]),
                ("ort_render_views_matte", [vp, C.POINTER(RenderParams), vp, C.c_uint32, C.POINTER(Matte), C.POINTER(MattePlanes), stats]),
                ("ort_raycast", [vp, vp, C.c_uint64, vp, C.c_uint32, stats]),
                ("ort_occluded", [vp, vp, vp, C.c_uint64, vp, C.c_uint32, stats]),
                ("ort_ambient_occlusion", [vp, vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp, C.c_uint32, stats]),
                ("ort_radiance", [vp, vp, vp, C.c_uint64, C.c_uint32, C.c_float, vp, vp, C.c_uint32, stats]),
                ("ort_radiance_adaptive", [vp, vp, vp, C.c_uint64, C.POINTER(Adaptive), C.c_float, vp, vp, vp, vp, C.c_uint32, stats]),
                ("ort_irradiance", [vp, vp, vp, C.c_uint64, C.c_uint32, C.c_float, vp, vp, C.c_uint32, stats]),
                ("ort_irradiance_adaptive", [vp, vp, vp, C.c_uint64, C.POINTER(Adaptive), C.c_float, vp, vp, vp, vp, C.c_uint32, stats]),
                ("ort_probe_sh", [vp, vp, vp, C.c_uint64, C.c_uint32, C.c_float, vp, vp, vp, C.c_uint32, stats])):
            getattr(L, name).argtypes = argtypes
            getattr(L, name + "_device").argtypes = argtypes[:-1] + [vp, stats]
        L.ort_camera_from_pose.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.c_int32, C.POINTER(Camera)]
        L.ort_render_views_workspace_bytes.argtypes = [C.POINTER(RenderParams), C.c_uint32, C.POINTER(C.c_uint64)]
        L.ort_rgbe.restype = C.c_uint32
        L.ort_rgbe.argtypes = [C.c_float, C.c_float, C.c_float]
        L.ort_write_hdr.argtypes = [C.c_char_p, C.c_void_p, C.c_int32, C.c_int32]
        L.ort_shard_block_count.argtypes = [C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
        L.ort_pack_blocks_host.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p]
        L.ort_unpack_blocks_host.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p]
        L.ort_unpack_blocks_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.ort_denoise_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_uint32, C.POINTER(C.c_uint64)]
        L.ort_denoise.argtypes = [C.c_int, C.POINTER(DenoiseParams), C.POINTER(DenoisePlanes), C.c_int32, C.c_int32, C.c_uint32, vp, stats]
        L.ort_denoise_device.argtypes = [C.c_int, C.POINTER(DenoiseParams), C.POINTER(DenoisePlanes), C.c_int32, C.c_int32, C.c_uint32, vp, vp,
                                         C.c_uint64, vp, stats]
        L.ort_matte_mask.argtypes = [C.c_int, vp, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.c_int32, C.c_int32, C.c_uint32, vp]
        L.ort_matte_mask_device.argtypes = [C.c_int, vp, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.c_int32, C.c_int32, C.c_uint32, vp, vp]
        L.ort_plan_samples_workspace_bytes.argtypes =[C.c_int32, C.c_int32, C.c_uint32, C.POINTER(C.c_uint64)]
        L.ort_plan_samples.argtypes = [C.c_int, C.POINTER(PlanParams), C.POINTER(PlanPlanes), C.c_int32, C.c_int32, C.c_uint32, vp, vp, stats]
        L.ort_plan_samples_device.argtypes = [C.c_int, C.POINTER(PlanParams), C.POINTER(PlanPlanes), C.c_int32, C.c_int32, C.c_uint32, vp, vp, vp,
                                              C.c_uint64, vp, stats]
        L.ort_comm_unique_id.argtypes = [C.c_void_p]
        L.ort_comm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.ort_comm_create_local.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p)]
        L.ort_comm_destroy.argtypes = [C.c_void_p]
        L.ort_comm_destroy.restype = None
        L.ort_gather_framebuffer.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        L.ort_gather_framebuffer_local.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.c_int32,
                                                   C.c_int32, C.POINTER(C.c_void_p)]
        _lib = L
    return _lib


def _check(rc):
    if rc != OK:
        raise OrtError(rc, lib().ort_last_error().decode("utf-8", "replace"))


def device_count():
    n = C.c_int(0)
    rc = lib().ort_device_count(C.byref(n))
    return n.value if rc == OK else 0


def _v3(a):
    return V3(float(a[0]), float(a[1]), float(a[2]))


def camera_from_pose(p, quat_xyzw, ratio, width, height):
    """Camera basis of a pose for a width x height image (macos_main.mm:550-556): rows p, x_axis, y_axis, z_axis as
    Scene.camera returns them for the scene's own pose.  -> (4, 3) float32."""
    p = np.ascontiguousarray(p, dtype="<f4")
    q = np.ascontiguousarray(quat_xyzw, dtype="<f4")
    if p.shape != (3,) or q.shape != (4,):
        raise ValueError("p must have 3 components and quat_xyzw 4, got shapes %s and %s" % (p.shape, q.shape))
    cam = Camera()
    _check(lib().ort_camera_from_pose(p.ctypes.data, q.ctypes.data, float(ratio), int(width), int(height), C.byref(cam)))
    return np.array([[v.x, v.y, v.z] for v in (cam.p, cam.x_axis, cam.y_axis, cam.z_axis)], dtype="<f4")


def _rays(rays):
    """-> (N, 6) float32, C-contiguous; ValueError on any other shape"""
    rays = np.ascontiguousarray(rays, dtype="<f4")
    if rays.ndim != 2 or rays.shape[1] != 6:
        raise ValueError("rays must be an (N, 6) array of o.xyz d.xyz, got shape %s" % (rays.shape,))
    return rays


def _probe_points(points):
    """-> (N, 6) float32 p.xyz n.xyz, C-contiguous: as given, or (N, 3) positions with the pole +z filled in"""
    points = np.ascontiguousarray(points, dtype="<f4")
    if points.ndim == 2 and points.shape[1] == 3:
        pole = np.zeros((len(points), 3), "<f4")
        pole[:, 2] = 1.0
        return np.ascontiguousarray(np.concatenate([points, pole], axis=1))
    if points.ndim != 2 or points.shape[1] != 6:
        raise ValueError("points must be an (N, 3) array of p.xyz or an (N, 6) array of p.xyz n.xyz, got shape %s" % (points.shape,))
    return points


def _seeds(seeds, n):
    """-> uint32[n] (any integers, taken modulo 2^32); ValueError on any other shape"""
    seeds = np.asarray(seeds)
    if seeds.shape != (n,):
        raise ValueError("seeds must be an (N,) array with N = %d, got shape %s" % (n, seeds.shape))
    return np.ascontiguousarray(seeds.astype(np.int64) & 0xFFFFFFFF, dtype="<u4")


def _ptr(p):
    """a raw device pointer or a stream -> the ctypes argument; 0 and None are NULL"""
    return C.c_void_p(p) if p else None


def _flags(counters):
    return RENDER_COUNTERS if counters else 0


def _stats(want=True):
    """-> (the ort_stats * argument of a call, what to return after it): a fresh struct and its as_dict, or NULL and None"""
    st = Stats() if want else None
    return (C.byref(st), st.as_dict) if want else (None, lambda: None)


def _views(cameras, seeds):
    """(V, 4, 3) camera bases and (V,) seeds -> the ort_view array of a batch; ValueError on any other shape."""
    cameras = np.asarray(cameras, dtype="<f4")
    seeds = np.asarray(seeds)
    if cameras.ndim != 3 or cameras.shape[1:] != (4, 3):
        raise ValueError("cameras must be a (V, 4, 3) array of p, x_axis, y_axis, z_axis rows, got shape %s" % (cameras.shape,))
    if seeds.shape != (len(cameras),):
        raise ValueError("seeds must be a (V,) array with V = %d, got shape %s" % (len(cameras), seeds.shape))
    if len(cameras) > MAX_VIEWS:
        raise ValueError("at most %d views in one call, got %d" % (MAX_VIEWS, len(cameras)))
    views = np.zeros(len(cameras), VIEW_DTYPE)
    views["camera"] = cameras
    views["seed"] = seeds.astype(np.int64) & 0xFFFFFFFF
    return views


def _lead(views):
    """the leading axes of a render's planes: none for one frame (views None), (V,) for a batch"""
    return () if views is None else (len(views),)


def _is_plane(a, shape, dtype):
    return isinstance(a, np.ndarray) and a.shape == shape and a.dtype == np.dtype(dtype) and a.flags.c_contiguous


def _host_planes(specs, out, what):
    """The host planes of a render, as a list: zeros by specs [(shape, dtype), ...], or the caller's out checked against them.
    what: the planes' names, for the message about their number"""
    if out is None:
        return [np.zeros(sh, dt) for sh, dt in specs]
    if len(out) != len(specs):
        raise ValueError("out must hold %d planes (%s), got %d" % (len(specs), what, len(out)))
    for a, (sh, dt) in zip(out, specs):
        if not _is_plane(a, sh, dt):
            raise ValueError("out: every plane must be a C-contiguous array, expected shape %s dtype %s" % (sh, dt))
    return list(out)


class Scene:
    """Owning wrapper of an ort_scene handle."""

    def __init__(self, handle):
        self.handle = C.c_void_p(handle)
        self.device = None

    # -- construction ----------------------------------------------------------------
    @classmethod
    def load_scn(cls, path, base_dir=None):
        if base_dir is None:
            base_dir = os.path.dirname(os.path.abspath(path)) + "/"
        h = C.c_void_p()
        _check(lib().ort_scene_load_scn(os.fsencode(path), os.fsencode(base_dir), C.byref(h)))
        return cls(h.value)

    @classmethod
    def parse_scn(cls, text, base_dir=""):
        data = text if isinstance(text, bytes) else text.encode()
        h = C.c_void_p()
        _check(lib().ort_scene_parse_scn(data, len(data), os.fsencode(base_dir), C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_arrays(cls, materials, spheres=None, boxes=None, cylinders=None, lights=None, meshes=(),
                    camera_p=(0, 0, 0), camera_quat_xyzw=(0, 0, 0, 1), camera_height_ratio=0.2, screen=(0, 0),
                    ambient=(0, 0, 0), with_reference_csg=False):
        def arr(a, dt):
            return np.ascontiguousarray(a if a is not None else np.zeros(0, dt), dtype=dt)
        mats, sph, box = arr(materials, MATERIAL_DTYPE), arr(spheres, SPHERE_DTYPE), arr(boxes, BOX_DTYPE)
        cyl, lig = arr(cylinders, CYLINDER_DTYPE), arr(lights, LIGHT_DTYPE)
        keep = []
        ms = (Mesh * max(1, len(meshes)))()
        for i, m in enumerate(meshes):
            v = np.ascontiguousarray(m["vertices"], dtype="<f4").reshape(-1, 3)
            ix = np.ascontiguousarray(m["indices"], dtype="<u4")
            keep += [v, ix]
            lo = m.get("aabb_min", v.min(axis=0) if len(v) else (0, 0, 0))
            hi = m.get("aabb_max", v.max(axis=0) if len(v) else (0, 0, 0))
            ms[i] = Mesh(v.ctypes.data, len(v), ix.ctypes.data, len(ix), int(m["mat"]), _v3(lo), _v3(hi))
        d = SceneDesc(mats.ctypes.data, len(mats), sph.ctypes.data, len(sph), box.ctypes.data, len(box),
                      cyl.ctypes.data, len(cyl), C.addressof(ms), len(meshes), lig.ctypes.data, len(lig),
                      _v3(camera_p), (C.c_float * 4)(*[float(q) for q in camera_quat_xyzw]),
                      float(camera_height_ratio), int(screen[0]), int(screen[1]), _v3(ambient),
                      1 if with_reference_csg else 0)
        h = C.c_void_p()
        _check(lib().ort_scene_create(C.byref(d), C.byref(h)))
        return cls(h.value)

    def close(self):
        if self.handle:
            lib().ort_scene_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- inspection ------------------------------------------------------------------
    def info(self):
        si = SceneInfo()
        _check(lib().ort_scene_get_info(self.handle, C.byref(si)))
        return si

    def _get(self, name, dtype, count):
        out = np.zeros(count, dtype)
        _check(getattr(lib(), "ort_scene_get_" + name)(self.handle, out.ctypes.data, count))
        return out

    def flatten(self, width, height):
        """The scene as plain arrays (same field layout as tests/ref_io.SceneDump)."""
        si = self.info()

        class Flat:
            pass
        f = Flat()
        f.width, f.height = width, height
        f.ambient = np.array([si.ambient.x, si.ambient.y, si.ambient.z], "<f4")
        f.materials = self._get("materials", MATERIAL_DTYPE, si.material_count)
        f.spheres = self._get("spheres", SPHERE_DTYPE, si.sphere_count)
        f.boxes = self._get("boxes", BOX_DTYPE, si.box_count)
        f.cylinders = self._get("cylinders", CYLINDER_DTYPE, si.cylinder_count)
        f.lights = self._get("lights", LIGHT_DTYPE, si.light_count)
        f.meshes = []
        for i in range(si.mesh_count):
            m = Mesh()
            _check(lib().ort_scene_get_mesh(self.handle, i, C.byref(m)))
            v = np.ctypeslib.as_array(C.cast(m.vertices, C.POINTER(C.c_float)), shape=(m.vertex_count, 3)).copy() \
                if m.vertex_count else np.zeros((0, 3), "<f4")
            ix = np.ctypeslib.as_array(C.cast(m.indices, C.POINTER(C.c_uint32)), shape=(m.index_count,)).copy() \
                if m.index_count else np.zeros(0, "<u4")
            f.meshes.append(dict(vertices=v.astype("<f4"), indices=ix.astype("<u4"), mat=m.mat,
                                 aabb_min=np.array([m.aabb_min.x, m.aabb_min.y, m.aabb_min.z], "<f4"),
                                 aabb_max=np.array([m.aabb_max.x, m.aabb_max.y, m.aabb_max.z], "<f4")))
        f.camera = self.camera(width, height)
        return f

    def camera(self, width, height):
        cam = Camera()
        _check(lib().ort_scene_get_camera(self.handle, width, height, C.byref(cam)))
        return np.array([[v.x, v.y, v.z] for v in (cam.p, cam.x_axis, cam.y_axis, cam.z_axis)], dtype="<f4")

    # -- build / upload -----------------------------------------------------------------
    def commit(self):
        _check(lib().ort_scene_commit(self.handle))
        return self

    def tree_info(self):
        ti = TreeInfo()
        _check(lib().ort_scene_get_tree_info(self.handle, C.byref(ti)))
        return {k: getattr(ti, k) for k, _ in ti._fields_}

    def upload(self, device=0):
        _check(lib().ort_scene_upload(self.handle, device))
        self.device = device
        return self

    # -- render ---------------------------------------------------------------------------
    @staticmethod
    def params(width, height, spp, seed, policy="chunk", chunk=0, rect=None, rr=0.8, counters=False, shard=(0, 1), packed=False):
        x0, y0, x1, y1 = rect if rect else (0, 0, width, height)
        pol = POLICIES[policy] if isinstance(policy, str) else policy
        if pol == POLICY_CHUNK and not chunk:
            chunk = spp
        return RenderParams(width, height, x0, y0, x1, y1, pol, seed & 0xFFFFFFFF, spp, chunk, rr,
                            _flags(counters) | (RENDER_PACKED if packed else 0), shard[0], shard[1])

    def render(self, width, height, spp, seed, policy="chunk", chunk=0, rect=None, rr=0.8, counters=False,
               shard=(0, 1), out=None):
        """Host framebuffer in/out.  Returns (image[H,W,3] float32, stats dict)."""
        p = self.params(width, height, spp, seed, policy, chunk, rect, rr, counters, shard)
        if out is None:
            out = np.zeros((height, width, 3), dtype="<f4")
        st, stats = _stats()
        _check(lib().ort_render_image(self.handle, C.byref(p), out.ctypes.data, st))
        return out, stats()

    def render_device(self, d_out_ptr, params, stream=None, want_stats=False):
        """Device framebuffer (raw device pointer, e.g. torch_tensor.data_ptr())."""
        st, stats = _stats(want_stats)
        _check(lib().ort_render_image_device(self.handle, C.byref(params), _ptr(d_out_ptr), _ptr(stream), st))
        return stats()

    # -- a batch of camera views in one launch ----------------------------------------------
    def render_views(self, cameras, seeds, width, height, spp, policy="chunk", chunk=0, rect=None, rr=0.8, counters=False,
                     out=None):
        """One frame per view, in one launch.  cameras: (V, 4, 3) float32 bases (camera_from_pose, Scene.camera); seeds:
        (V,).  Frame v is what render() gives with seed seeds[v] if the scene's camera were cameras[v].  Host
        framebuffers in/out: returns (frames[V,H,W,3] float32, stats dict); pixels outside rect keep what out held."""
        views = _views(cameras, seeds)
        if out is None:
            out = np.zeros((len(views), height, width, 3), dtype="<f4")
        if out.shape != (len(views), height, width, 3) or out.dtype != np.dtype("<f4") or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous float32 array of shape %s" % ((len(views), height, width, 3),))
        p = self.params(width, height, spp, 0, policy, chunk, rect, rr, counters)
        st, stats = _stats()
        _check(lib().ort_render_views(self.handle, C.byref(p), views.ctypes.data, len(views), out.ctypes.data, st))
        return out, stats()

    def render_views_device(self, d_out_ptr, params, cameras, seeds, stream=None, want_stats=False):
        """The same into a device buffer of V frames (raw device pointer, e.g. a (V, H, W, 3) torch tensor's data_ptr()).
        Enqueued on stream; waits only when want_stats (returns the stats dict).  params.seed is ignored."""
        views = _views(cameras, seeds)
        st, stats = _stats(want_stats)
        _check(lib().ort_render_views_device(self.handle, C.byref(params), views.ctypes.data, len(views), _ptr(d_out_ptr), _ptr(stream), st))
        return stats()

    # -- the camera renders that cut one-pixel jobs: four kinds, each one frame or a batch of views, host or device form ----
    def _pixel_jobs(self, kind, views, device, params, head, tail, stream=None, want_stats=True):
        """One of a kind's four entry points: ort_render_[views_]<kind>[_device](scene, params, *head[, views, count], *tail[,
        stream], stats).  views: None for the single-frame form, or the ort_view array (_views).  -> the stats dict, or None"""
        name = "ort_render_%s%s%s" % ("" if views is None else "views_", kind, "_device" if device else "")
        args = list(head) + ([] if views is None else [views.ctypes.data, len(views)]) + list(tail) + ([_ptr(stream)] if device else [])
        st, stats = _stats(want_stats)
        _check(getattr(lib(), name)(self.handle, C.byref(params), *args, st))
        return stats()

    # -- the adaptive camera render: one frame, or a batch of views ----------------------------
    def _adaptive_host(self, views, width, height, ad, seed, rect, rr, want_states, counters, out):
        shape = _lead(views) + (height, width)
        specs = [(shape + (3,), "<f4"), (shape, "<u4"), (shape, "<f4")] + ([(shape, "<u4")] if want_states else [])
        planes = _host_planes(specs, out, "rgb, spp, m2" + (", states" if want_states else ""))
        p = self.params(width, height, 1, seed, "pixel", 0, rect, rr, counters)
        tail = [a.ctypes.data for a in planes] + ([] if want_states else [None])
        return tuple(planes) + (self._pixel_jobs("adaptive", views, False, p, [C.byref(ad)], tail),)

    def _adaptive_device(self, views, params, ad, d_planes, stream, want_stats):
        return self._pixel_jobs("adaptive", views, True, params, [C.byref(ad)], [_ptr(d) for d in d_planes], stream, want_stats)

    def render_adaptive(self, width, height, min_spp, max_spp, tolerance, floor=0.05, check_every=4, seed=0, rect=None, rr=0.8,
                        want_states=False, counters=False, out=None):
        """render(policy="pixel") with a sample count per pixel: each pixel is sampled until the estimated standard error of
        its mean luminance is at most tolerance times the mean's magnitude (floor standing in for it in the dark), checked
        after min_spp samples and then every check_every, at most max_spp times (include/ort.h gives the rule).  Returns (rgb
        (H, W, 3) float32, spp (H, W) uint32 samples taken, m2 (H, W) float32 sum of squared sample luminance, stats dict),
        with want_states (rgb, spp, m2, states (H, W) uint32, stats).  Pixels outside rect keep what out's planes held."""
        ad = _adaptive(min_spp, max_spp, check_every, tolerance, floor)
        return self._adaptive_host(None, width, height, ad, seed, rect, rr, want_states, counters, out)

    def render_adaptive_device(self, params, min_spp, max_spp, tolerance, floor, check_every, d_out, d_spp=0, d_m2=0, d_states=0,
                               stream=None, want_stats=False):
        """The same into device planes (raw device pointers, e.g. torch tensors' data_ptr(): (H, W, 3) float32 and, where a
        pointer is given, (H, W) uint32 / float32 / uint32).  params: Scene.params(..., policy="pixel"); its spp is ignored.
        Enqueued on stream; waits only when want_stats (returns the stats dict)."""
        ad = _adaptive(min_spp, max_spp, check_every, tolerance, floor)
        return self._adaptive_device(None, params, ad, (d_out, d_spp, d_m2, d_states), stream, want_stats)

    def render_views_adaptive(self, cameras, seeds, width, height, min_spp, max_spp, tolerance, floor=0.05, check_every=4, rect=None,
                              rr=0.8, want_states=False, counters=False, out=None):
        """render_adaptive for a batch of views in one launch (cameras, seeds as render_views): frame v is what
        render_adaptive gives with seed seeds[v] if the scene's camera were cameras[v].  Returns (rgb (V, H, W, 3), spp (V, H,
        W), m2 (V, H, W)[, states (V, H, W)], stats dict)."""
        views = _views(cameras, seeds)
        ad = _adaptive(min_spp, max_spp, check_every, tolerance, floor)
        return self._adaptive_host(views, width, height, ad, 0, rect, rr, want_states, counters, out)

    def render_views_adaptive_device(self, params, cameras, seeds, min_spp, max_spp, tolerance, floor, check_every, d_out, d_spp=0,
                                     d_m2=0, d_states=0, stream=None, want_stats=False):
        """The same into device planes of V frames each, view-major.  Enqueued on stream; waits only when want_stats (returns
        the stats dict).  params.seed and params.spp are ignored."""
        views = _views(cameras, seeds)
        ad = _adaptive(min_spp, max_spp, check_every, tolerance, floor)
        return self._adaptive_device(views, params, ad, (d_out, d_spp, d_m2, d_states), stream, want_stats)

    # -- light-group renders: one frame per group of lights, in one pass --------------------------
    def light_materials(self):
        """the indices of the materials that are lights, ascending"""
        return [int(m) for m in np.nonzero(self._get("materials", MATERIAL_DTYPE, self.info().material_count)["is_light"])[0]]

    def _light_groups(self, groups, group_count):
        """groups -> (the ort_light_groups struct, the table that it points into, G).  groups: a byte per material of the scene,
        or a dict {material index: group} with every other material NO_LIGHT_GROUP.  group_count: G, by default one more
        than the largest group named."""
        n = self.info().material_count
        if isinstance(groups, dict):
            table = np.full(n, NO_LIGHT_GROUP, np.uint8)
            for m, g in groups.items():
                if not 0 <= int(m) < n:
                    raise ValueError("groups: material %d is not one of the scene's %d" % (m, n))
                table[int(m)] = g
        else:
            table = np.ascontiguousarray(groups, dtype=np.uint8)
            if table.shape != (n,):
                raise ValueError("groups must hold a byte per material: shape (%d,), got %s" % (n, table.shape))
        if group_count is None:
            named = table[table != NO_LIGHT_GROUP] if isinstance(groups, dict) else table[self.light_materials()]
            named = named[named != NO_LIGHT_GROUP]
            group_count = int(named.max()) + 1 if len(named) else 1
        return LightGroups(table.ctypes.data, n, group_count), table, int(group_count)

    def _light_groups_host(self, views, width, height, spp, seed, groups, want_rgb, want_states, group_count, rect, rr, counters, out):
        lg, table, G = self._light_groups(groups, group_count)
        lead, hw = _lead(views), (height, width)
        specs = [(lead + (G,) + hw + (3,), "<f4")] + ([(lead + hw + (3,), "<f4")] if want_rgb else []) + ([(lead + hw, "<u4")] if want_states else [])
        planes = _host_planes(specs, out, "groups" + (", rgb" if want_rgb else "") + (", states" if want_states else ""))
        p = self.params(width, height, spp, seed, "pixel", 0, rect, rr, counters)
        tail = [planes[0].ctypes.data, planes[1].ctypes.data if want_rgb else None, planes[-1].ctypes.data if want_states else None]
        return tuple(planes) + (self._pixel_jobs("light_groups", views, False, p, [C.byref(lg)], tail),)

    def _light_groups_device(self, views, params, groups, d_planes, group_count, stream, want_stats):
        lg, table, _ = self._light_groups(groups, group_count)
        return self._pixel_jobs("light_groups", views, True, params, [C.byref(lg)], [_ptr(d) for d in d_planes], stream, want_stats)

    def render_light_groups(self, width, height, spp, seed, groups, want_rgb=True, want_states=False, group_count=None, rect=None,
                            rr=0.8, counters=False, out=None):
        """render(policy="pixel") split by which light the energy came from, in one pass: frame g holds what the lights of
        group g contribute and is, bit for bit, the render of the scene with every other light's emission set to zero
        (include/ort.h gives the contract).  groups: a length-material_count sequence of group indices (a light's entry below
        G or NO_LIGHT_GROUP; other materials' entries are not read), or a dict {material index: group}, e.g. {m: i for i, m
        in enumerate(scene.light_materials())}.  Returns (frames (G, H, W, 3) float32[, rgb (H, W, 3) float32 the unsplit
        frame][, states (H, W) uint32], stats dict).  Pixels outside rect keep what out's planes held."""
        return self._light_groups_host(None, width, height, spp, seed, groups, want_rgb, want_states, group_count, rect, rr, counters, out)

    def render_light_groups_device(self, params, groups, d_groups, d_rgb=0, d_states=0, group_count=None, stream=None, want_stats=False):
        """The same into device planes (raw device pointers, e.g. torch tensors' data_ptr(): (G, H, W, 3) float32 and, where a
        pointer is given, (H, W, 3) float32 / (H, W) uint32).  params: Scene.params(..., policy="pixel").  Enqueued on stream;
        waits only when want_stats (returns the stats dict)."""
        return self._light_groups_device(None, params, groups, (d_groups, d_rgb, d_states), group_count, stream, want_stats)

    def render_views_light_groups(self, cameras, seeds, width, height, spp, groups, want_rgb=True, want_states=False, group_count=None,
                                  rect=None, rr=0.8, counters=False, out=None):
        """render_light_groups for a batch of views in one launch (cameras, seeds as render_views): frames (v, .) are what
        render_light_groups gives with seed seeds[v] if the scene's camera were cameras[v].  Returns (frames (V, G, H, W, 3)[,
        rgb (V, H, W, 3)][, states (V, H, W)], stats dict)."""
        views = _views(cameras, seeds)
        return self._light_groups_host(views, width, height, spp, 0, groups, want_rgb, want_states, group_count, rect, rr, counters, out)

    def render_views_light_groups_device(self, params, cameras, seeds, groups, d_groups, d_rgb=0, d_states=0, group_count=None,
                                         stream=None, want_stats=False):
        """The same into device planes, view-major: (V, G, H, W, 3), (V, H, W, 3), (V, H, W).  Enqueued on stream; waits only
        when want_stats (returns the stats dict).  params.seed is ignored."""
        views = _views(cameras, seeds)
        return self._light_groups_device(views, params, groups, (d_groups, d_rgb, d_states), group_count, stream, want_stats)

    # -- path-depth renders: emission, direct, indirect -- one frame per bounce count, in one pass ------
    _DEPTH_PLANES = ("rgb", "lengths", "states")

    def _depths_host(self, views, width, height, spp, seed, bins, rect, rr, want, counters, out):
        want = tuple(want)
        if any(w not in self._DEPTH_PLANES for w in want) or len(set(want)) != len(want):
            raise ValueError("want names planes among %s, each once; got %r" % (self._DEPTH_PLANES, want))
        G = int(bins)
        lead, hw = _lead(views), (height, width)
        Ga = G if 1 <= G <= MAX_DEPTH_BINS else 1   # a bin count the call refuses: planes that are never written
        shapes = {"bins": (lead + (Ga,) + hw + (3,), "<f4"), "rgb": (lead + hw + (3,), "<f4"), "lengths": (lead + (Ga,) + hw, "<u4"),
                  "states": (lead + hw, "<u4")}
        names = ["bins"] + [n for n in self._DEPTH_PLANES if n in want]
        if out is not None and (not isinstance(out, dict) or set(out) != set(names)):
            raise ValueError("out must be a dict of the planes %s" % (names,))
        planes = dict(zip(names, _host_planes([shapes[n] for n in names], None if out is None else [out[n] for n in names], ", ".join(names))))
        p = self.params(width, height, spp, seed, "pixel", 0, rect, rr, counters)
        tail = [planes[n].ctypes.data if n in planes else None for n in ("bins",) + self._DEPTH_PLANES]
        st = self._pixel_jobs("depths", views, False, p, [C.c_uint32(G & 0xFFFFFFFF)], tail)
        return planes["bins"], {n: planes[n] for n in names[1:]}, st

    def render_depths(self, width, height, spp, seed, bins=3, rr=0.8, want=("rgb",), rect=None, counters=False, out=None):
        """render(policy="pixel") split by how many bounces the light took, in one pass: with bins=3 frame DEPTH_EMISSION holds the
        light sources seen directly, DEPTH_DIRECT the light that took one bounce and DEPTH_INDIRECT everything beyond; with more
        bins (up to MAX_DEPTH_BINS) frame g < bins - 1 holds the light that took exactly g bounces and the last frame the rest
        (include/ort.h gives the contract).  want: which other planes to return, among "rgb" (the unsplit frame), "lengths"
        ((bins, H, W) uint32: a pixel's samples counted by the depth of their last ray) and "states" ((H, W) uint32).  Returns
        (frames (bins, H, W, 3) float32, {name: plane for the planes asked for}, stats dict).  out: a dict of the caller's planes,
        "bins" and those of want; pixels outside rect keep what they held."""
        return self._depths_host(None, width, height, spp, seed, bins, rect, rr, want, counters, out)

    def render_depths_device(self, params, bins, d_bins, d_rgb=0, d_lengths=0, d_states=0, stream=None, want_stats=False):
        """The same into device planes (raw device pointers, e.g. torch tensors' data_ptr(): (bins, H, W, 3) float32 and, where a
        pointer is given, (H, W, 3) float32 / (bins, H, W) uint32 / (H, W) uint32).  params: Scene.params(..., policy="pixel").
        Enqueued on stream; waits only when want_stats (returns the stats dict)."""
        return self._pixel_jobs("depths", None, True, params, [C.c_uint32(int(bins) & 0xFFFFFFFF)], [_ptr(d) for d in (d_bins, d_rgb, d_lengths, d_states)],
                                stream, want_stats)

    def render_views_depths(self, cameras, seeds, width, height, spp, bins=3, rr=0.8, want=("rgb",), rect=None, counters=False, out=None):
        """render_depths for a batch of views in one launch (cameras, seeds as render_views): frames (v, .) are what render_depths
        gives with seed seeds[v] if the scene's camera were cameras[v].  Returns (frames (V, bins, H, W, 3), {"rgb": (V, H, W, 3),
        "lengths": (V, bins, H, W), "states": (V, H, W)} as asked for, stats dict)."""
        return self._depths_host(_views(cameras, seeds), width, height, spp, 0, bins, rect, rr, want, counters, out)

    def render_views_depths_device(self, params, cameras, seeds, bins, d_bins, d_rgb=0, d_lengths=0, d_states=0, stream=None, want_stats=False):
        """The same into device planes, view-major: (V, bins, H, W, 3), (V, H, W, 3), (V, bins, H, W), (V, H, W).  Enqueued on stream;
        waits only when want_stats (returns the stats dict).  params.seed is ignored."""
        return self._pixel_jobs("depths", _views(cameras, seeds), True, params, [C.c_uint32(int(bins) & 0xFFFFFFFF)],
                                [_ptr(d) for d in (d_bins, d_rgb, d_lengths, d_states)], stream, want_stats)

    # -- sample-map renders: the caller's sample count per pixel ----------------------------------
    @staticmethod
    def _sample_map(sample_map, shape):
        """the caller's map -> a C-contiguous uint32 array of that shape (integers, taken modulo 2^32: 0xffffffff stays itself)"""
        m = np.asarray(sample_map)
        if m.shape != shape:
            raise ValueError("sample_map must have shape %s, got %s" % (shape, m.shape))
        if m.dtype != np.dtype("<u4"):
            m = (m.astype(np.int64) & 0xFFFFFFFF).astype("<u4")
        return np.ascontiguousarray(m)

    def _sample_map_host(self, views, width, height, sample_map, cap, seed, want_m2, want_states, rect, rr, counters, out):
        shape = _lead(views) + (height, width)
        smap = self._sample_map(sample_map, shape)
        specs = [(shape + (3,), "<f4")] + ([(shape, "<f4")] if want_m2 else []) + ([(shape, "<u4")] if want_states else [])
        planes = _host_planes(specs, out, "rgb" + (", m2" if want_m2 else "") + (", states" if want_states else ""))
        p = self.params(width, height, cap, seed, "pixel", 0, rect, rr, counters)
        tail = [smap.ctypes.data, planes[0].ctypes.data, planes[1].ctypes.data if want_m2 else None, planes[-1].ctypes.data if want_states else None]
        return tuple(planes) + (self._pixel_jobs("sample_map", views, False, p, [], tail),)

    def _sample_map_device(self, views, params, d_planes, stream, want_stats):
        return self._pixel_jobs("sample_map", views, True, params, [], [_ptr(d) for d in d_planes], stream, want_stats)

    def render_sample_map(self, width, height, sample_map, cap, seed, want_m2=True, want_states=False, rect=None, rr=0.8, counters=False,
                          out=None):
        """render(policy="pixel") with the caller's sample count per pixel: pixel (x, y) gets min(sample_map[y, x], cap)
        samples of its own stream, and a pixel whose count is 0 is not rendered -- its words of every plane keep what out
        held, as the pixels outside rect do (include/ort.h gives the contract).  sample_map: (H, W) integers, row 0 at the
        bottom -- render_adaptive's spp plane can be passed as it stands.  Returns (rgb (H, W, 3) float32[, m2 (H, W) float32
        sum of squared sample luminance][, states (H, W) uint32], stats dict).  Passes taken with different seeds combine
        weighted by their counts: (n1 * rgb1 + n2 * rgb2) / (n1 + n2)."""
        return self._sample_map_host(None, width, height, sample_map, cap, seed, want_m2, want_states, rect, rr, counters, out)

    def render_sample_map_device(self, params, d_map, d_rgb, d_m2=0, d_states=0, stream=None, want_stats=False):
        """The same with the map and the planes on the device (raw device pointers, e.g. torch tensors' data_ptr(): the map
        (H, W) uint32 -- or int32 holding the same words --, (H, W, 3) float32 and, where a pointer is given, (H, W) float32 /
        uint32).  params: Scene.params(..., policy="pixel"), its spp the cap.  Enqueued on stream; waits only when
        want_stats (returns the stats dict)."""
        return self._sample_map_device(None, params, (d_map, d_rgb, d_m2, d_states), stream, want_stats)

    def render_views_sample_map(self, cameras, seeds, width, height, sample_map, cap, want_m2=True, want_states=False, rect=None,
                                rr=0.8, counters=False, out=None):
        """render_sample_map for a batch of views in one launch (cameras, seeds as render_views; sample_map (V, H, W), a map
        per view): frame v is what render_sample_map gives with seed seeds[v] and sample_map[v] if the scene's camera were
        cameras[v].  Returns (rgb (V, H, W, 3)[, m2 (V, H, W)][, states (V, H, W)], stats dict)."""
        views = _views(cameras, seeds)
        return self._sample_map_host(views, width, height, sample_map, cap, 0, want_m2, want_states, rect, rr, counters, out)

    def render_views_sample_map_device(self, params, cameras, seeds, d_map, d_rgb, d_m2=0, d_states=0, stream=None, want_stats=False):
        """The same with the maps and the planes on the device, V frames each, view-major.  Enqueued on stream; waits only
        when want_stats (returns the stats dict).  params.seed is ignored."""
        views = _views(cameras, seeds)
        return self._sample_map_device(views, params, (d_map, d_rgb, d_m2, d_states), stream, want_stats)

    # -- accumulating renders: a frame's samples continued across calls ---------------------------
    def _accumulate_host(self, views, acc, add, seed, cap, rect, rr, counters, use_m2, out):
        if not isinstance(acc, Accumulator) or acc.views != (None if views is None else len(views)):
            raise ValueError("acc must be an Accumulator of %s" % ("one frame (views=None)" if views is None else "%d views" % len(views)))
        shape = _lead(views) + (acc.height, acc.width)
        if np.ndim(add) == 0:   # the same count for every pixel: no map, the cap is the count
            smap, cap = None, int(add) if cap is None else cap
        else:
            smap = self._sample_map(add, shape)
            cap = min(max(int(smap.max()) if smap.size else 1, 1), 1 << 24) if cap is None else cap
        if out is not None and not _is_plane(out, shape + (3,), "<f4"):
            raise ValueError("out must be a C-contiguous float32 array of shape %s" % (shape + (3,),))
        p = self.params(acc.width, acc.height, cap, seed, "pixel", 0, rect, rr, counters)
        planes = acc._struct(use_m2)
        tail = [C.byref(planes), None if smap is None else smap.ctypes.data, None if out is None else out.ctypes.data]
        return self._pixel_jobs("accumulate", views, False, p, [], tail)

    def _accumulate_device(self, views, params, d_sum, d_count, d_states, d_m2, d_map, d_rgb, stream, want_stats):
        planes = AccumPlanes(d_sum or None, d_m2 or None, d_count or None, d_states or None)
        return self._pixel_jobs("accumulate", views, True, params, [], [C.byref(planes), _ptr(d_map), _ptr(d_rgb)], stream, want_stats)

    def render_accumulate(self, acc, add, seed, cap=None, rect=None, rr=0.8, counters=False, use_m2=True, out=None):
        """Continue the frame that acc (an Accumulator) holds: every pixel of rect takes up to `add` more samples of ITS OWN
        stream, from where its last call left it, and acc's planes -- the undivided colour sums, the sums of squared sample
        luminance, the sample counts, the streams' states -- are updated in place.  After any split into calls the planes hold
        the bits of the single call, so acc.rgb() is render(policy="pixel")'s frame at the total count (include/ort.h gives the
        contract).  add: an integer, the same for every pixel, or an (H, W) map of integers as render_sample_map takes it, cut
        at cap (by default the map's largest value); a pixel never passes 1 << 24 samples.  A fresh Accumulator starts the
        frame.  use_m2=False leaves acc.m2 out of the call; out: an (H, W, 3) float32 array that receives sum / count of the
        pixels that took samples in this call (the others keep what it held).  Returns the stats dict."""
        return self._accumulate_host(None, acc, add, seed, cap, rect, rr, counters, use_m2, out)

    def render_accumulate_device(self, params, d_sum, d_count, d_states, d_m2=0, d_map=0, d_rgb=0, stream=None, want_stats=False):
        """The same on the device's own planes (raw device pointers, e.g. torch tensors' data_ptr(): (H, W, 3) float32 sums,
        (H, W) uint32 counts -- or int32 holding the same words -- and states, and where a pointer is given (H, W) float32 m2, the
        (H, W) map and the (H, W, 3) frame).  params: Scene.params(..., policy="pixel"), its spp the cap on what this call adds.
        Enqueued on stream; waits only when want_stats (returns the stats dict), so successive calls on one stream chain
        passes on planes that never visit the host."""
        return self._accumulate_device(None, params, d_sum, d_count, d_states, d_m2, d_map, d_rgb, stream, want_stats)

    def render_views_accumulate(self, cameras, seeds, acc, add, cap=None, rect=None, rr=0.8, counters=False, use_m2=True, out=None):
        """render_accumulate for a batch of views in one launch (cameras, seeds as render_views; acc an Accumulator of V views,
        add an integer or a (V, H, W) map, out (V, H, W, 3)): frame v is what render_accumulate gives with seed seeds[v] if the
        scene's camera were cameras[v].  Returns the stats dict."""
        return self._accumulate_host(_views(cameras, seeds), acc, add, 0, cap, rect, rr, counters, use_m2, out)

    def render_views_accumulate_device(self, params, cameras, seeds, d_sum, d_count, d_states, d_m2=0, d_map=0, d_rgb=0, stream=None,
                                       want_stats=False):
        """The same with every plane on the device, V frames each, view-major.  params.seed is ignored."""
        return self._accumulate_device(_views(cameras, seeds), params, d_sum, d_count, d_states, d_m2, d_map, d_rgb, stream, want_stats)

    # -- the converge loop: plan on the device, accumulate the plan, until nothing is planned --------
    @staticmethod
    def _pass_budget(budget, spent, passes_left):
        """the per-frame budget of the next pass under a total of `budget` a frame: what is left, shared among the passes left;
        None without a total, 0 when nothing is left to share (the loop ends: 0 would mean "no budget" to the planner)"""
        return None if budget is None else max(int(budget) - spent, 0) // passes_left

    def render_converge(self, acc, tolerance, seed, passes=8, budget=None, pilot=PLAN_DEFAULTS["pilot"], cap=PLAN_DEFAULTS["cap"], keep_maps=False,
                        cameras=None, rr=0.8, **plan_kw):
        """Sample the frame acc (an Accumulator) holds until it has converged: up to `passes` times, plan the next pass from acc's
        own planes (Accumulator.plan: tolerance, pilot, cap and plan_kw -- floor, radius, min_add) and, unless every frame's plan
        is empty (planned == 0), render_accumulate exactly that map with cap as the pass's cap.  From a fresh Accumulator the first
        plan is the pilot.  budget: the most samples a FRAME gets over the whole loop; pass k plans with (what is left) //
        (passes left) as its budget, and the loop ends when that is 0.  cameras: (V, 4, 3) for an Accumulator of V views, seed then
        being the V seeds (render_views_accumulate); a frame's spending is counted as the largest of the batch.  Returns the list
        of every plan's totals -- one entry per plan made, each the dict (or, for views, the list of dicts) of plan_samples with
        "budget" added, the last one being the plan that ended the loop unless the passes ran out -- and, with keep_maps,
        (totals, maps)."""
        history, maps, spent = [], [], 0
        for k in range(int(passes)):
            b = self._pass_budget(budget, spent, int(passes) - k)
            if b == 0:
                break
            smap, totals = acc.plan(tolerance, pilot=pilot, cap=cap, budget=b, **plan_kw)
            per_frame = totals if isinstance(totals, list) else [totals]
            for t in per_frame:
                t["budget"] = b
            history.append(totals)
            if all(t["planned"] == 0 for t in per_frame):
                break
            if keep_maps:
                maps.append(smap)
            if cameras is None:
                self.render_accumulate(acc, smap, seed, cap=cap, rr=rr)
            else:
                self.render_views_accumulate(cameras, seed, acc, smap, cap=cap, rr=rr)
            spent += max(t["planned"] for t in per_frame)
        return (history, maps) if keep_maps else history

    def render_converge_device(self, width, height, d_sum, d_m2, d_count, d_states, d_map, d_totals, d_workspace, tolerance, seed, passes=8,
                               budget=None, pilot=PLAN_DEFAULTS["pilot"], cap=PLAN_DEFAULTS["cap"], cameras=None, rr=0.8, stream=None, device=0,
                               **plan_kw):
        """render_converge on the device's own planes, none of which visits the host: d_sum, d_m2, d_count, d_states (the planes of
        render_accumulate_device), the caller's map d_map (uint32 or int32, a word per pixel), d_totals (32 bytes per frame, e.g. 4
        int64 per frame) and d_workspace (plan_workspace_bytes) are torch tensors on the scene's device.  Plan and pass are
        enqueued on stream (a raw stream, as the other device forms take; None: the default stream); between them the host reads
        d_totals, 32 bytes per frame, and nothing else.  Returns the list of every plan's totals, as render_converge."""
        import torch
        frames = 1 if cameras is None else len(cameras)
        ws_bytes = d_workspace.numel() * d_workspace.element_size()
        if d_totals.numel() * d_totals.element_size() < 32 * frames:
            raise ValueError("d_totals must hold 32 bytes per frame")
        history, spent = [], 0
        ext = torch.cuda.ExternalStream(stream, device=d_totals.device) if stream else torch.cuda.current_stream(d_totals.device)
        for k in range(int(passes)):
            b = self._pass_budget(budget, spent, int(passes) - k)
            if b == 0:
                break
            plan_samples_device(d_sum.data_ptr(), d_m2.data_ptr(), d_count.data_ptr(), width, height, d_map.data_ptr(), d_totals.data_ptr(),
                                d_workspace.data_ptr(), ws_bytes, tolerance, frame_count=frames, pilot=pilot, cap=cap, rgb_is_sum=True, budget=b,
                                device=device, stream=stream, **plan_kw)
            with torch.cuda.stream(ext):
                raw = d_totals.reshape(-1).view(torch.uint8)[:32 * frames].cpu()   # the one read: ordered behind the plan on its stream
            per_frame = _totals_dicts(np.frombuffer(raw.numpy().tobytes(), PLAN_TOTALS_DTYPE))
            for t in per_frame:
                t["budget"] = b
            history.append(per_frame if cameras is not None else per_frame[0])
            if all(t["planned"] == 0 for t in per_frame):
                break
            params = self.params(width, height, cap, 0 if cameras is not None else seed, "pixel", 0, None, rr)
            if cameras is None:
                self.render_accumulate_device(params, d_sum.data_ptr(), d_count.data_ptr(), d_states.data_ptr(), d_m2.data_ptr(), d_map.data_ptr(), stream=stream)
            else:
                self.render_views_accumulate_device(params, cameras, seed, d_sum.data_ptr(), d_count.data_ptr(), d_states.data_ptr(), d_m2.data_ptr(),
                                                    d_map.data_ptr(), stream=stream)
            spent += max(t["planned"] for t in per_frame)
        return history

    # -- first-hit feature renders: albedo, normal, depth, coverage and id planes ---------------
    @staticmethod
    def _feature_planes(shape, want, out):
        """the host planes of a feature render, by name: zeros, or the caller's (out: a dict by the names of want, checked)"""
        specs = {"albedo": (shape + (3,), "<f4"), "normal": (shape + (3,), "<f4"), "depth": (shape, "<f4"), "hits": (shape, "<u4"),
                 "ids": (shape + (2,), "<u4"), "states": (shape, "<u4")}
        want = tuple(want)
        if not want or len(set(want)) != len(want) or not set(want) <= set(FEATURE_PLANES):
            raise ValueError("want must name planes of %s, each once, got %r" % (FEATURE_PLANES, want))
        if out is None:
            return {k: np.zeros(*specs[k]) for k in want}
        if set(out) != set(want):
            raise ValueError("out must hold exactly the planes of want %r, got %r" % (want, tuple(out)))
        for k in want:
            if not _is_plane(out[k], *specs[k]):
                raise ValueError("out[%r] must be a C-contiguous array of shape %s dtype %s" % ((k,) + specs[k]))
        return dict(out)

    @staticmethod
    def _feature_struct(ptrs):
        """name -> pointer (ints, ctypes pointers, None) -> FeaturePlanes"""
        unknown = set(ptrs) - set(FEATURE_PLANES)
        if unknown:
            raise ValueError("unknown feature planes %r: the planes are %s" % (sorted(unknown), FEATURE_PLANES))
        fp = FeaturePlanes()
        for k in FEATURE_PLANES:
            v = _ptr(ptrs.get(k))
            setattr(fp, "final_states" if k == "states" else k, v.value if isinstance(v, C.c_void_p) else v)
        return fp

    def _features_host(self, views, width, height, spp, seed, rect, want, counters, out):
        planes = self._feature_planes(_lead(views) + (height, width), want, out)
        p = self.params(width, height, spp, seed, "pixel", 0, rect, 0.0, counters)
        fp = self._feature_struct({k: a.ctypes.data for k, a in planes.items()})
        return planes, self._pixel_jobs("features", views, False, p, [], [C.byref(fp)])

    def _features_device(self, views, params, d_planes, stream, want_stats):
        fp = self._feature_struct(d_planes)
        return self._pixel_jobs("features", views, True, params, [], [C.byref(fp)], stream, want_stats)

    def render_features(self, width, height, spp, seed, rect=None, want=("albedo", "normal", "depth", "hits", "ids"), counters=False,
                        out=None):
        """What the camera's own samples see first, per pixel: the means over spp camera samples (the PIXEL render's aperture
        draw on the pixel's own stream, then raycast()'s closest hit) of the first hit's albedo (emit of a light, diffuse
        otherwise), unit normal and distance, the number of samples that hit a surface (coverage = hits / spp), sample 0's
        (mat, prim) and, with "states" in want, the stream's final state.  Returns (planes, stats dict), planes a dict by
        the names of want: albedo, normal (H, W, 3) float32, depth (H, W) float32, hits, states (H, W) uint32, ids (H, W, 2)
        uint32.  Pixels outside rect keep what out's planes held.  Which planes are asked for changes no bit of the others."""
        return self._features_host(None, width, height, spp, seed, rect, want, counters, out)

    def render_features_device(self, params, stream=None, want_stats=False, **d_planes):
        """The same into device planes: albedo=, normal=, depth=, hits=, ids=, states= raw device pointers (e.g. torch tensors'
        data_ptr()), those not given are not written.  params: Scene.params(..., policy="pixel"); its chunk and rr are ignored.
        Enqueued on stream; waits only when want_stats (returns the stats dict)."""
        return self._features_device(None, params, d_planes, stream, want_stats)

    def render_views_features(self, cameras, seeds, width, height, spp, rect=None, want=("albedo", "normal", "depth", "hits", "ids"),
                              counters=False, out=None):
        """render_features for a batch of views in one launch (cameras, seeds as render_views): frame v is what render_features
        gives with seed seeds[v] if the scene's camera were cameras[v].  Every plane has a leading axis of V frames."""
        views = _views(cameras, seeds)
        return self._features_host(views, width, height, spp, 0, rect, want, counters, out)

    def render_views_features_device(self, params, cameras, seeds, stream=None, want_stats=False, **d_planes):
        """The same into device planes of V frames each, view-major.  Enqueued on stream; waits only when want_stats (returns
        the stats dict).  params.seed is ignored."""
        views = _views(cameras, seeds)
        return self._features_device(views, params, d_planes, stream, want_stats)

    # -- feature renders that follow mirrors and glass: the planes of the first non-specular vertex ---
    @staticmethod
    def _follow_planes(shape, want, out):
        """the host planes of a follow render, by name: zeros, or the caller's (out: a dict by the names of want, checked)"""
        specs = {"albedo": (shape + (3,), "<f4"), "normal": (shape + (3,), "<f4"), "depth": (shape, "<f4"), "hits": (shape, "<u4"),
                 "ids": (shape + (2,), "<u4"), "bounces": (shape, "<u4"), "states": (shape, "<u4")}
        want = tuple(want)
        if not want or len(set(want)) != len(want) or not set(want) <= set(FOLLOW_PLANES):
            raise ValueError("want must name planes of %s, each once, got %r" % (FOLLOW_PLANES, want))
        if out is None:
            return {k: np.zeros(*specs[k]) for k in want}
        if set(out) != set(want):
            raise ValueError("out must hold exactly the planes of want %r, got %r" % (want, tuple(out)))
        for k in want:
            if not _is_plane(out[k], *specs[k]):
                raise ValueError("out[%r] must be a C-contiguous array of shape %s dtype %s" % ((k,) + specs[k]))
        return dict(out)

    @staticmethod
    def _follow_struct(ptrs):
        """name -> pointer (ints, ctypes pointers, None) -> FollowPlanes"""
        unknown = set(ptrs) - set(FOLLOW_PLANES)
        if unknown:
            raise ValueError("unknown follow planes %r: the planes are %s" % (sorted(unknown), FOLLOW_PLANES))
        fp = FollowPlanes()
        for k in FOLLOW_PLANES:
            v = _ptr(ptrs.get(k))
            setattr(fp, "final_states" if k == "states" else k, v.value if isinstance(v, C.c_void_p) else v)
        return fp

    def _follow_host(self, views, width, height, spp, seed, max_bounces, rr, rect, want, counters, out):
        planes = self._follow_planes(_lead(views) + (height, width), want, out)
        p = self.params(width, height, spp, seed, "pixel", 0, rect, rr, counters)
        fp = self._follow_struct({k: a.ctypes.data for k, a in planes.items()})
        return planes, self._pixel_jobs("follow", views, False, p, [], [C.c_uint32(max_bounces), C.byref(fp)])

    def _follow_device(self, views, params, max_bounces, d_planes, stream, want_stats):
        fp = self._follow_struct(d_planes)
        return self._pixel_jobs("follow", views, True, params, [], [C.c_uint32(max_bounces), C.byref(fp)], stream, want_stats)

    def render_follow(self, width, height, spp, seed, max_bounces=8, rr=0.8, want=("albedo", "normal", "depth", "hits", "ids", "bounces"),
                      rect=None, counters=False, out=None):
        """render_features with mirrors and glass followed: every camera sample goes on through surfaces that are neither a light
        nor have a diffuse part, as the render's own path does (roulette rr, the render's draws, at most max_bounces bounces,
        max_bounces <= MAX_FOLLOW_BOUNCES), and what is recorded is the vertex where it ends: albedo, unit normal (as it stands),
        the path's length from the aperture point, the samples that recorded a vertex (hits), sample 0's (mat, prim), the sum of
        the recorded samples' bounces and, with "states" in want, the stream's final state.  The sums are divided by spp: over_hits
        gives the mean over the recorded samples.  Returns (planes, stats dict) as render_features; bounces is (H, W) uint32.
        max_bounces = 0 is render_features, bit for bit."""
        return self._follow_host(None, width, height, spp, seed, max_bounces, rr, rect, want, counters, out)

    def render_follow_device(self, params, max_bounces=8, stream=None, want_stats=False, **d_planes):
        """The same into device planes: albedo=, normal=, depth=, hits=, ids=, bounces=, states= raw device pointers, those not given
        are not written.  params: Scene.params(..., policy="pixel"); its chunk is ignored, its rr is the roulette's.  Enqueued on
        stream; waits only when want_stats (returns the stats dict)."""
        return self._follow_device(None, params, max_bounces, d_planes, stream, want_stats)

    def render_views_follow(self, cameras, seeds, width, height, spp, max_bounces=8, rr=0.8,
                            want=("albedo", "normal", "depth", "hits", "ids", "bounces"), rect=None, counters=False, out=None):
        """render_follow for a batch of views in one launch (cameras, seeds as render_views): frame v is what render_follow gives
        with seed seeds[v] if the scene's camera were cameras[v].  Every plane has a leading axis of V frames."""
        views = _views(cameras, seeds)
        return self._follow_host(views, width, height, spp, 0, max_bounces, rr, rect, want, counters, out)

    def render_views_follow_device(self, params, cameras, seeds, max_bounces=8, stream=None, want_stats=False, **d_planes):
        """The same into device planes of V frames each, view-major.  Enqueued on stream; waits only when want_stats (returns
        the stats dict).  params.seed is ignored."""
        views = _views(cameras, seeds)
        return self._follow_device(views, params, max_bounces, d_planes, stream, want_stats)

    # -- ID-matte renders: per-pixel coverage per material, object or shape -------------------------
    def object_ids(self):
        """every object id an ID-matte render by="object" can give, with the material the object carries -> (ids (N,) uint32,
        mats (N,) uint32): HIT_MESH << 28 | i for mesh i, then kind << 28 | i for the boxes (2), cylinders (3) and spheres (4) in
        the scene's own order.  What selections for matte_mask are built from."""
        si = self.info()
        ids, mats = [], []
        for i in range(si.mesh_count):
            m = Mesh()
            _check(lib().ort_scene_get_mesh(self.handle, i, C.byref(m)))
            ids.append(HIT_MESH << 28 | i)
            mats.append(m.mat)
        for kind, name, dtype, n in ((2, "boxes", BOX_DTYPE, si.box_count), (3, "cylinders", CYLINDER_DTYPE, si.cylinder_count),
                                     (4, "spheres", SPHERE_DTYPE, si.sphere_count)):
            shapes = self._get(name, dtype, n)
            ids += [kind << 28 | i for i in range(n)]
            mats += [int(m) for m in shapes["mat"]]
        return np.array(ids, "<u4"), np.array(mats, "<u4")

    @staticmethod
    def _matte(by, slots):
        if by not in MATTE_BY:
            raise ValueError("by must be one of %s, got %r" % (tuple(MATTE_BY), by))
        if not 0 <= int(slots) <= 0xFFFFFFFF:
            raise ValueError("slots must fit an unsigned 32-bit word, got %r" % (slots,))
        return Matte(MATTE_BY[by], int(slots))

    @staticmethod
    def _matte_planes(shape, slots, want, out):
        """the host planes of a matte render, by name: ids and counts always, those of want besides; zeros, or the caller's (out: a
        dict by exactly those names, checked)"""
        k = max(1, min(int(slots), MAX_MATTE_SLOTS))   # a bad slots is the library's to name
        specs = {"ids": (shape + (k,), "<u4"), "counts": (shape + (k,), "<u4"), "other": (shape, "<u4"), "hits": (shape, "<u4"), "states": (shape, "<u4")}
        want = tuple(want)
        if len(set(want)) != len(want) or not set(want) <= set(MATTE_PLANES[2:]):
            raise ValueError("want must name planes of %s, each once, got %r" % (MATTE_PLANES[2:], want))
        names = MATTE_PLANES[:2] + want
        if out is None:
            return {n: np.zeros(*specs[n]) for n in names}
        if set(out) != set(names):
            raise ValueError("out must hold exactly the planes %r, got %r" % (names, tuple(out)))
        for n in names:
            if not _is_plane(out[n], *specs[n]):
                raise ValueError("out[%r] must be a C-contiguous array of shape %s dtype %s" % ((n,) + specs[n]))
        return dict(out)

    @staticmethod
    def _matte_struct(ptrs):
        """name -> pointer (ints, ctypes pointers, None) -> MattePlanes"""
        unknown = set(ptrs) - set(MATTE_PLANES)
        if unknown:
            raise ValueError("unknown matte planes %r: the planes are %s" % (sorted(unknown), MATTE_PLANES))
        mp = MattePlanes()
        for k in MATTE_PLANES:
            v = _ptr(ptrs.get(k))
            setattr(mp, "final_states" if k == "states" else k, v.value if isinstance(v, C.c_void_p) else v)
        return mp

    def _matte_host(self, views, width, height, spp, seed, by, slots, rect, want, counters, out):
        m = self._matte(by, slots)
        planes = self._matte_planes(_lead(views) + (height, width), slots, want, out)
        p = self.params(width, height, spp, seed, "pixel", 0, rect, 0.8, counters)
        mp = self._matte_struct({k: a.ctypes.data for k, a in planes.items()})
        return planes, self._pixel_jobs("matte", views, False, p, [], [C.byref(m), C.byref(mp)])

    def _matte_device(self, views, params, by, slots, d_planes, stream, want_stats):
        m = self._matte(by, slots)
        mp = self._matte_struct(d_planes)
        return self._pixel_jobs("matte", views, True, params, [], [C.byref(m), C.byref(mp)], stream, want_stats)

    def render_matte(self, width, height, spp, seed, by="object", slots=8, rect=None, want=("other", "hits"), counters=False, out=None):
        """ID mattes: per pixel, how many of the camera's spp samples (render_features' samples, bit for bit) saw which id --
        by="material" the hit's material, by="prim" its shape as raycast names it, by="object" the shape, or for a triangle
        HIT_MESH << 28 | its mesh (object_ids lists them).  Returns ({"ids": (H, W, slots) uint32, "counts": (H, W, slots) uint32,
        and those of want: "other", "hits", "states" (H, W) uint32}, stats dict).  A pixel's slots are ordered by count
        descending, then id ascending; unused slots hold (MATTE_EMPTY, 0).  While other is 0 the slots are the pixel's exact
        histogram; where other > 0 the kept ids are the first `slots` to appear, not the largest: render again with more slots.
        matte_mask turns a selection of ids into a coverage mask.  Pixels outside rect keep what out's planes held."""
        return self._matte_host(None, width, height, spp, seed, by, slots, rect, want, counters, out)

    def render_matte_device(self, params, by="object", slots=8, stream=None, want_stats=False, **d_planes):
        """The same into device planes: ids=, counts= (both required, slots words a pixel), other=, hits=, states= raw device
        pointers.  params: Scene.params(..., policy="pixel"); its chunk and rr are ignored.  Enqueued on stream; waits only when
        want_stats (returns the stats dict)."""
        return self._matte_device(None, params, by, slots, d_planes, stream, want_stats)

    def render_views_matte(self, cameras, seeds, width, height, spp, by="object", slots=8, rect=None, want=("other", "hits"), counters=False,
                           out=None):
        """render_matte for a batch of views in one launch (cameras, seeds as render_views): frame v is what render_matte gives
        with seed seeds[v] if the scene's camera were cameras[v].  Every plane has a leading axis of V frames."""
        views = _views(cameras, seeds)
        return self._matte_host(views, width, height, spp, 0, by, slots, rect, want, counters, out)

    def render_views_matte_device(self, params, cameras, seeds, by="object", slots=8, stream=None, want_stats=False, **d_planes):
        """The same into device planes of V frames each, view-major.  params.seed is ignored."""
        views = _views(cameras, seeds)
        return self._matte_device(views, params, by, slots, d_planes, stream, want_stats)

    # -- closest-hit ray queries -----------------------------------------------------------
    def raycast(self, rays, counters=False):
        """Closest hit of each ray (raycast_top_most_node, ray.cpp:1165).  rays: (N, 6) float32 o.xyz d.xyz (d need
        not be unit length).  Returns (hits: HIT_DTYPE[N], stats dict); synchronous."""
        rays = _rays(rays)
        hits = np.zeros(len(rays), HIT_DTYPE)
        st, stats = _stats()
        _check(lib().ort_raycast(self.handle, rays.ctypes.data, len(rays), hits.ctypes.data, _flags(counters), st))
        return hits, stats()

    def raycast_device(self, d_rays_ptr, count, d_hits_ptr, stream=None, counters=False, want_stats=False):
        """Device rays (count x 6 float32) -> device hits (count x 24 B, HIT_DTYPE), raw pointers on the scene's device,
        e.g. torch tensors' data_ptr().  Enqueued on stream; waits only when want_stats (returns the stats dict)."""
        st, stats = _stats(want_stats)
        _check(lib().ort_raycast_device(self.handle, _ptr(d_rays_ptr), count, _ptr(d_hits_ptr), _flags(counters), _ptr(stream), st))
        return stats()

    # -- occlusion ray queries -------------------------------------------------------------
    def occluded(self, rays, tmax=None, counters=False):
        """Is anything in the way before tmax?  occluded[i] = (hit.mat != 0 and hit.t < tmax[i]) with hit the closest hit
        raycast returns for rays[i]; the comparison is the IEEE one (NaN, zero and negative limits give False).  rays:
        (N, 6) float32 o.xyz d.xyz; tmax: None (no limit), a scalar (broadcast) or an (N,) array, in units of the ray
        parameter.  Returns (occluded: bool[N], stats dict); synchronous."""
        rays = _rays(rays)
        if tmax is not None:
            tmax = np.asarray(tmax, dtype="<f4")
            if tmax.ndim == 0:
                tmax = np.full(len(rays), tmax, dtype="<f4")
            if tmax.shape != (len(rays),):
                raise ValueError("tmax must be a scalar or an (N,) array with N = %d, got shape %s" % (len(rays), tmax.shape))
            tmax = np.ascontiguousarray(tmax)
        out = np.zeros(len(rays), np.bool_)
        st, stats = _stats()
        _check(lib().ort_occluded(self.handle, rays.ctypes.data, tmax.ctypes.data if tmax is not None else None, len(rays),
                                  out.ctypes.data, _flags(counters), st))
        return out, stats()

    def occluded_device(self, d_rays_ptr, d_tmax_ptr, count, d_out_ptr, stream=None, counters=False, want_stats=False):
        """Device rays (count x 6 float32) and limits (count float32, or None: no limit) -> device bytes (count, each 0 or
        1: a torch.bool tensor), raw pointers on the scene's device.  Enqueued on stream; waits only when want_stats."""
        st, stats = _stats(want_stats)
        _check(lib().ort_occluded_device(self.handle, _ptr(d_rays_ptr), _ptr(d_tmax_ptr), count, _ptr(d_out_ptr), _flags(counters),
                                         _ptr(stream), st))
        return stats()

    # -- radiance queries -----------------------------------------------------------------
    def radiance(self, rays, seeds, spp, rr=0.8, want_states=False, counters=False):
        """Path-traced radiance along each ray: spp samples of the reference's sample body from rays[i] on the xorshift
        stream that starts at seeds[i] (0 is taken as 1), no aperture.  rays: (N, 6) float32 o.xyz d.xyz, d of unit length
        (|d|^2 within [0.999, 1.001], all components finite; any other ray gives NaN NaN NaN and its seed back); seeds: (N,)
        uint32, e.g. job_seeds(master, N).  Returns (rgb: float32[N, 3], stats dict), with want_states (rgb, states:
        uint32[N], stats dict); synchronous."""
        return self._radiance(lib().ort_radiance, rays, seeds, spp, rr, want_states, counters)

    def _radiance(self, call, rays, seeds, spp, rr, want_states, counters):
        """The host form of a radiance or irradiance query: call is the library's function, rays the (N, 6) array."""
        rays = _rays(rays)
        seeds = _seeds(seeds, len(rays))
        out = np.zeros((len(rays), 3), "<f4")
        states = np.zeros(len(rays), "<u4") if want_states else None
        st, stats = _stats()
        _check(call(self.handle, rays.ctypes.data, seeds.ctypes.data, len(rays), int(spp), float(rr), out.ctypes.data,
                    states.ctypes.data if want_states else None, _flags(counters), st))
        return (out, states, stats()) if want_states else (out, stats())

    def radiance_device(self, d_rays, d_seeds, n, spp, rr, d_out, d_states=0, stream=0, counters=False, want_stats=False):
        """Device rays (n x 6 float32) and seeds (n uint32) -> device colours (n x 3 float32) and, if d_states, final states
        (n uint32): raw pointers on the scene's device, e.g. torch tensors' data_ptr().  Enqueued on stream; waits only when
        want_stats (returns the stats dict)."""
        st, stats = _stats(want_stats)
        _check(lib().ort_radiance_device(self.handle, _ptr(d_rays), _ptr(d_seeds), n, int(spp), float(rr), _ptr(d_out), _ptr(d_states),
                                         _flags(counters), _ptr(stream), st))
        return stats()

    # -- adaptive radiance queries ----------------------------------------------------------
    def radiance_adaptive(self, rays, seeds, min_spp, max_spp, tolerance, floor=0.05, check_every=4, rr=0.8, want_states=False,
                          counters=False):
        """radiance() with a sample count per ray: each ray is sampled until the estimated standard error of its mean
        luminance is at most tolerance times the mean's magnitude (floor standing in for the magnitude in the dark), checked
        after min_spp samples and then every check_every, and at most max_spp times (include/ort.h gives the rule operation
        by operation).  A ray that saw no light in its first min_spp samples stops black: pick min_spp for the scene.
        Returns (rgb: float32[N, 3], spp: uint32[N] samples taken, m2: float32[N] sum of squared sample luminance, stats
        dict), with want_states (rgb, spp, m2, states, stats); a ray outside the domain gives NaN, 0, 0 and its seed."""
        return self._radiance_adaptive(lib().ort_radiance_adaptive, rays, seeds, min_spp, max_spp, tolerance, floor, check_every, rr,
                                       want_states, counters)

    def _radiance_adaptive(self, call, rays, seeds, min_spp, max_spp, tolerance, floor, check_every, rr, want_states, counters):
        """The host form of an adaptive radiance or irradiance query, as _radiance."""
        rays = _rays(rays)
        seeds = _seeds(seeds, len(rays))
        ad = _adaptive(min_spp, max_spp, check_every, tolerance, floor)
        out = np.zeros((len(rays), 3), "<f4")
        spp = np.zeros(len(rays), "<u4")
        m2 = np.zeros(len(rays), "<f4")
        states = np.zeros(len(rays), "<u4") if want_states else None
        st, stats = _stats()
        _check(call(self.handle, rays.ctypes.data, seeds.ctypes.data, len(rays), C.byref(ad), float(rr),
                    out.ctypes.data, spp.ctypes.data, m2.ctypes.data,
                    states.ctypes.data if want_states else None, _flags(counters), st))
        return (out, spp, m2, states, stats()) if want_states else (out, spp, m2, stats())

    def radiance_adaptive_device(self, d_rays, d_seeds, n, min_spp, max_spp, tolerance, floor, check_every, rr, d_out, d_spp=0,
                                 d_m2=0, d_states=0, stream=0, counters=False, want_stats=False):
        """Device rays (n x 6 float32) and seeds (n uint32) -> device colours (n x 3 float32) and, where a pointer is given,
        samples taken (n uint32), sums of squared sample luminance (n float32) and final states (n uint32): raw pointers on
        the scene's device.  Enqueued on stream; waits only when want_stats (returns the stats dict)."""
        st, stats = _stats(want_stats)
        ad = _adaptive(min_spp, max_spp, check_every, tolerance, floor)
        _check(lib().ort_radiance_adaptive_device(self.handle, _ptr(d_rays), _ptr(d_seeds), n, C.byref(ad), float(rr), _ptr(d_out),
                                                  _ptr(d_spp), _ptr(d_m2), _ptr(d_states), _flags(counters), _ptr(stream), st))
        return stats()

    # -- irradiance queries: cosine-weighted hemisphere gathers at points -------------------------
    def irradiance(self, points, seeds, spp, rr=0.8, want_states=False, counters=False):
        """The cosine-weighted mean of the radiance arriving at each point over the hemisphere about its normal: spp samples,
        each a direction drawn about n with the reference's diffuse lobe and then radiance()'s sample along it, on the
        xorshift stream that starts at seeds[i] (0 is taken as 1).  points: (N, 6) float32 p.xyz n.xyz, n of unit length
        (|n|^2 within [0.999, 1.001], all components finite; any other point gives NaN NaN NaN and its seed back), p lifted
        off its surface by the caller (say p + 1e-3 n).  Irradiance is pi * rgb; a diffuse texel's radiosity is kd * rgb.
        Returns as radiance(); synchronous."""
        return self._radiance(lib().ort_irradiance, points, seeds, spp, rr, want_states, counters)

    def irradiance_device(self, d_points, d_seeds, n, spp, rr, d_out, d_states=0, stream=0, counters=False, want_stats=False):
        """Device points (n x 6 float32) and seeds (n uint32) -> device colours (n x 3 float32) and, if d_states, final
        states: raw pointers on the scene's device, as radiance_device()."""
        st, stats = _stats(want_stats)
        _check(lib().ort_irradiance_device(self.handle, _ptr(d_points), _ptr(d_seeds), n, int(spp), float(rr), _ptr(d_out), _ptr(d_states),
                                           _flags(counters), _ptr(stream), st))
        return stats()

    # -- SH light-probe queries: radiance over the sphere as 9 SH coefficients ------------------------
    def probe_sh(self, points, seeds, spp, rr=0.8, want_rgb=False, want_states=False, counters=False):
        """The radiance arriving at each point from all directions, projected onto the nine real spherical harmonics of bands
        0 to 2 (world axes): spp samples, each a direction drawn uniformly over the sphere and then radiance()'s sample along
        it, on the xorshift stream that starts at seeds[i] (0 is taken as 1).  points: (N, 3) float32 positions, or (N, 6)
        p.xyz n.xyz as irradiance() takes them -- n is only the pole of the sample pattern, +z where positions alone are
        given; a point outside irradiance()'s domain gives NaN in all 27 words and its seed back.  Returns (sh: float32[N, 9,
        3] [point][coefficient][rgb], the MEAN of basis times radiance: the field's SH coefficients are 4 pi * sh, and
        sh_irradiance() shades a normal from it), then rgb float32[N, 3] (the plain mean) with want_rgb, states uint32[N] with
        want_states, and the stats dict; synchronous."""
        points = _probe_points(points)
        seeds = _seeds(seeds, len(points))
        sh = np.zeros((len(points), SH_COEFFS, 3), "<f4")
        rgb = np.zeros((len(points), 3), "<f4") if want_rgb else None
        states = np.zeros(len(points), "<u4") if want_states else None
        st, stats = _stats()
        _check(lib().ort_probe_sh(self.handle, points.ctypes.data, seeds.ctypes.data, len(points), int(spp), float(rr), sh.ctypes.data,
                                  rgb.ctypes.data if want_rgb else None, states.ctypes.data if want_states else None, _flags(counters), st))
        return (sh,) + ((rgb,) if want_rgb else ()) + ((states,) if want_states else ()) + (stats(),)

    def probe_sh_device(self, d_points, d_seeds, n, spp, rr, d_sh, d_rgb=0, d_states=0, stream=0, counters=False, want_stats=False):
        """Device points (n x 6 float32) and seeds (n uint32) -> device coefficients (n x 27 float32) and, where a pointer is
        given, plain means (n x 3 float32) and final states (n uint32): raw pointers on the scene's device, as
        radiance_device()."""
        st, stats = _stats(want_stats)
        _check(lib().ort_probe_sh_device(self.handle, _ptr(d_points), _ptr(d_seeds), n, int(spp), float(rr), _ptr(d_sh), _ptr(d_rgb),
                                         _ptr(d_states), _flags(counters), _ptr(stream), st))
        return stats()

    def irradiance_adaptive(self, points, seeds, min_spp, max_spp, tolerance, floor=0.05, check_every=4, rr=0.8, want_states=False,
                            counters=False):
        """irradiance() with a sample count per point: radiance_adaptive()'s stopping rule, unchanged, over the point's
        samples.  Returns as radiance_adaptive(); a point outside the domain gives NaN, 0, 0 and its seed."""
        return self._radiance_adaptive(lib().ort_irradiance_adaptive, points, seeds, min_spp, max_spp, tolerance, floor, check_every,
                                       rr, want_states, counters)

    def irradiance_adaptive_device(self, d_points, d_seeds, n, min_spp, max_spp, tolerance, floor, check_every, rr, d_out, d_spp=0,
                                   d_m2=0, d_states=0, stream=0, counters=False, want_stats=False):
        """Device points and seeds -> device colours and, where a pointer is given, samples taken, sums of squared sample
        luminance and final states: as radiance_adaptive_device()."""
        st, stats = _stats(want_stats)
        ad = _adaptive(min_spp, max_spp, check_every, tolerance, floor)
        _check(lib().ort_irradiance_adaptive_device(self.handle, _ptr(d_points), _ptr(d_seeds), n, C.byref(ad), float(rr), _ptr(d_out),
                                                    _ptr(d_spp), _ptr(d_m2), _ptr(d_states), _flags(counters), _ptr(stream), st))
        return stats()

    # -- ambient-occlusion queries: hemisphere visibility gathers at points ------------------------
    def ambient_occlusion(self, points, seeds, spp, radius=None, want_bent=False, want_states=False, counters=False):
        """How much of the hemisphere about its normal each point sees within radius: spp samples, each irradiance()'s
        direction draw about n on the xorshift stream that starts at seeds[i] (0 is taken as 1) and then occluded()'s answer
        for the ray (p, d) with tmax = radius[i].  points: (N, 6) float32 p.xyz n.xyz as for irradiance(); radius: None (no
        limit), a scalar (broadcast) or an (N,) array, a distance; NaN or <= 0 leaves every sample open.  open[i] counts the
        samples with nothing in the way: visibility is open / spp, ambient occlusion one minus that.  bent[i] is the float32
        sum of the open samples' directions, in sample order, not normalised.  A point outside the domain gives AO_INVALID,
        NaN NaN NaN and its seed back.  Returns (open: uint32[N], [bent: float32[N, 3] if want_bent], [states: uint32[N] if
        want_states], stats dict); synchronous."""
        points = _rays(points)
        seeds = _seeds(seeds, len(points))
        if radius is not None:
            radius = np.asarray(radius, dtype="<f4")
            if radius.ndim == 0:
                radius = np.full(len(points), radius, dtype="<f4")
            if radius.shape != (len(points),):
                raise ValueError("radius must be a scalar or an (N,) array with N = %d, got shape %s" % (len(points), radius.shape))
            radius = np.ascontiguousarray(radius)
        out = np.zeros(len(points), "<u4")
        bent = np.zeros((len(points), 3), "<f4") if want_bent else None
        states = np.zeros(len(points), "<u4") if want_states else None
        st, stats = _stats()
        _check(lib().ort_ambient_occlusion(self.handle, points.ctypes.data, seeds.ctypes.data,
                                           radius.ctypes.data if radius is not None else None, len(points), int(spp), out.ctypes.data,
                                           bent.ctypes.data if want_bent else None, states.ctypes.data if want_states else None,
                                           _flags(counters), st))
        return (out,) + ((bent,) if want_bent else ()) + ((states,) if want_states else ()) + (stats(),)

    def ambient_occlusion_device(self, d_points, d_seeds, d_radius, n, spp, d_open, d_bent=0, d_states=0, stream=0, counters=False,
                                 want_stats=False):
        """Device points (n x 6 float32), seeds (n uint32) and radii (n float32, or None: no limit) -> device open counts (n
        uint32) and, where a pointer is given, bent sums (n x 3 float32) and final states (n uint32): raw pointers on the
        scene's device.  Enqueued on stream; waits only when want_stats (returns the stats dict)."""
        st, stats = _stats(want_stats)
        _check(lib().ort_ambient_occlusion_device(self.handle, _ptr(d_points), _ptr(d_seeds), _ptr(d_radius), n, int(spp), _ptr(d_open),
                                                  _ptr(d_bent), _ptr(d_states), _flags(counters), _ptr(stream), st))
        return stats()

    def triangle_of(self, index):
        """mesh-major triangle id (decode_prim of a triangle hit) -> (mesh, triangle within that mesh).  Accepts arrays."""
        first = getattr(self, "_tri_first", None)
        if first is None:
            counts = []
            for i in range(self.info().mesh_count):
                m = Mesh()
                _check(lib().ort_scene_get_mesh(self.handle, i, C.byref(m)))
                counts.append(m.index_count // 3)
            first = self._tri_first = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
        idx = np.asarray(index, dtype=np.int64)
        if (idx < 0).any() or (idx >= first[-1]).any():
            raise IndexError("triangle id out of range (the scene has %d triangles)" % first[-1])
        mesh = np.searchsorted(first, idx, side="right") - 1
        local = idx - first[mesh]
        if np.ndim(index) == 0:
            return int(mesh), int(local)
        return mesh, local

    def tiled_raytrace(self, out, x0, y0, x1, y1, rng_state, spp, rr=0.8):
        """Exact analogue of one reference call (ray.cpp:1178); returns (shape_tests, new_rng_state)."""
        height, width = out.shape[:2]
        st = C.c_uint32(rng_state)
        n = C.c_uint64(0)
        _check(lib().ort_tiled_raytrace(self.handle, out.ctypes.data, width, height, x0, y0, x1, y1, C.byref(st), spp,
                                        rr, C.byref(n)))
        return n.value, st.value

    def tiled_raytrace_batch(self, out, jobs, rr=0.8):
        height, width = out.shape[:2]
        jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
        finals = np.zeros(len(jobs), "<u4")
        st, stats = _stats()
        _check(lib().ort_tiled_raytrace_batch(self.handle, out.ctypes.data, width, height, jobs.ctypes.data, len(jobs),
                                              rr, finals.ctypes.data, st))
        return finals, stats()


class Accumulator:
    """The host planes of an accumulating render (Scene.render_accumulate): sum_rgb (H, W, 3) float32, the undivided colour
    sums; m2 (H, W) float32, the sums of squared sample luminance; count (H, W) uint32, the samples each pixel has had; states
    (H, W) uint32, the streams' states.  views=V: V frames of each, (V, H, W[, 3]).  A fresh one has count == 0 everywhere,
    which is all the call reads of a pixel that has had no sample.  save / load: the checkpoint of a frame."""

    def __init__(self, width, height, views=None):
        self.width, self.height, self.views = int(width), int(height), None if views is None else int(views)
        shape = (() if views is None else (self.views,)) + (self.height, self.width)
        self.sum_rgb = np.zeros(shape + (3,), "<f4")
        self.m2 = np.zeros(shape, "<f4")
        self.count = np.zeros(shape, "<u4")
        self.states = np.zeros(shape, "<u4")

    def _struct(self, use_m2=True):
        shape = self.count.shape
        for a, sh, dt in ((self.sum_rgb, shape + (3,), "<f4"), (self.m2, shape, "<f4"), (self.count, shape, "<u4"), (self.states, shape, "<u4")):
            if not _is_plane(a, sh, dt):
                raise ValueError("Accumulator: every plane must be a C-contiguous array, expected shape %s dtype %s" % (sh, dt))
        return AccumPlanes(self.sum_rgb.ctypes.data, self.m2.ctypes.data if use_m2 else None, self.count.ctypes.data, self.states.ctypes.data)

    def rgb(self, fill=0.0):
        """sum_rgb / count in float32, component by component -- the call's own out_rgb; fill where count == 0"""
        out = np.full(self.sum_rgb.shape, fill, "<f4")
        had = self.count != 0
        with np.errstate(all="ignore"):
            out[had] = self.sum_rgb[had] / self.count[had].astype("<f4")[:, None]
        return out

    def denoise(self, planes, **kw):
        """the frame as it stands, denoised (denoise()): its own rgb(), m2 and count with the albedo, normal and depth planes of a
        Scene.render_features dict of the same shape -> (out, stats)"""
        return denoise(self.rgb(), self.m2, self.count, planes["albedo"], planes["normal"], planes["depth"], **kw)

    def plan(self, tolerance, **kw):
        """where the frame's next samples should go (plan_samples()): its own sum_rgb (rgb_is_sum=True), m2 and count -> (map,
        totals); the map is what render_accumulate takes as add, with cap=cap"""
        return plan_samples(self.sum_rgb, self.m2, self.count, tolerance, rgb_is_sum=True, **kw)

    def save(self, path):
        """the frame as it stands, into one .npz file (np.savez): Accumulator.load(path) continues it"""
        with open(path, "wb") as f:
            np.savez(f, sum_rgb=self.sum_rgb, m2=self.m2, count=self.count, states=self.states)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            count = z["count"]
            if count.ndim not in (2, 3) or count.dtype != np.dtype("<u4"):
                raise ValueError("%s: count must be (H, W) or (V, H, W) uint32, got %s %s" % (path, count.shape, count.dtype))
            acc = cls(count.shape[-1], count.shape[-2], None if count.ndim == 2 else count.shape[0])
            for name in ("sum_rgb", "m2", "count", "states"):
                a = z[name]
                have = getattr(acc, name)
                if a.shape != have.shape or a.dtype != have.dtype:
                    raise ValueError("%s: %s must be %s %s, got %s %s" % (path, name, have.shape, have.dtype, a.shape, a.dtype))
                have[...] = a
        return acc


def _adaptive(min_spp, max_spp, check_every, tolerance, floor):
    """-> Adaptive; counts that do not fit 32 bits are a ValueError here, everything else is the library's to judge"""
    for name, v in (("min_spp", min_spp), ("max_spp", max_spp), ("check_every", check_every)):
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError("%s must fit an unsigned 32-bit word, got %r" % (name, v))
    return Adaptive(int(min_spp), int(max_spp), int(check_every), float(tolerance), float(floor))


def sh_basis(d):
    """The nine real SH basis values of bands 0 to 2 at directions d (..., 3), float32, operation for operation as the
    probe_sh() kernels form them (include/ort.h): every product and sum rounded to float32 on its own.  -> float32[..., 9]"""
    d = np.asarray(d, dtype="<f4")
    if d.shape[-1:] != (3,):
        raise ValueError("d must be an (..., 3) array of directions, got shape %s" % (d.shape,))
    F = np.float32
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    with np.errstate(all="ignore"):
        b = [np.full(x.shape, F(0.282094792), "<f4"),
             F(0.488602512) * y, F(0.488602512) * z, F(0.488602512) * x,
             F(1.092548431) * (x * y), F(1.092548431) * (y * z), F(0.315391565) * (F(3.0) * (z * z) - F(1.0)),
             F(1.092548431) * (x * z), F(0.546274215) * (x * x - y * y)]
    return np.stack([np.asarray(v, "<f4") for v in b], axis=-1)


SH_COSINE_LOBE = (np.pi, 2.0 * np.pi / 3.0, np.pi / 4.0)   # A_l of bands 0, 1, 2: the clamped cosine's zonal coefficients


def sh_irradiance(sh, normals):
    """The cosine-convolved irradiance a renderer evaluates per normal from probe_sh()'s coefficients:
    4 pi * sum_j A_l(j) * sh[:, j] * Y_j(n), with A = pi, 2 pi / 3, pi / 4 per band, in float64.  sh: (N, 9, 3) or (9, 3);
    normals: (N, 3) or (3,) unit vectors.  -> float64[N, 3] (or [3])"""
    sh = np.asarray(sh, dtype=np.float64)
    n = np.asarray(normals, dtype=np.float64)
    if sh.shape[-2:] != (SH_COEFFS, 3) or n.shape[-1:] != (3,):
        raise ValueError("sh must be (..., 9, 3) and normals (..., 3), got shapes %s and %s" % (sh.shape, n.shape))
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    Y = np.stack([np.full(x.shape, 0.282094792), 0.488602512 * y, 0.488602512 * z, 0.488602512 * x, 1.092548431 * (x * y), 1.092548431 * (y * z),
                  0.315391565 * (3.0 * (z * z) - 1.0), 1.092548431 * (x * z), 0.546274215 * (x * x - y * y)], axis=-1)
    A = np.array([SH_COSINE_LOBE[0]] + [SH_COSINE_LOBE[1]] * 3 + [SH_COSINE_LOBE[2]] * 5)
    return 4.0 * np.pi * np.sum((A * Y)[..., :, None] * sh, axis=-2)


def decode_prim(prim):
    """ort_hit.prim -> (kind, index): kind is HIT_TRIANGLE / HIT_BOX / HIT_CYLINDER / HIT_SPHERE, index the shape's
    position in the scene's own arrays (triangles: mesh-major id, see Scene.triangle_of).  A miss (NO_PRIM) gives
    (None, None); arrays give int64 arrays, -1 for misses."""
    if np.ndim(prim) == 0:
        p = int(prim)
        return (None, None) if p == NO_PRIM else (p >> 28, p & 0x0FFFFFFF)
    p = np.asarray(prim, dtype=np.uint32).astype(np.int64)
    miss = p == NO_PRIM
    return np.where(miss, -1, p >> 28), np.where(miss, -1, p & 0x0FFFFFFF)


def job_seeds(master, n):
    """job_seed(master, i) for i in range(n): the per-pixel seeding policies' seeds (fmix32 of master ^ i * 2654435761, 0
    replaced by 1), for ray i of a radiance query.  -> uint32[n]"""
    h = (np.uint64(int(master) & 0xFFFFFFFF) ^ ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)))
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h[h == 0] = 1
    return h.astype("<u4")


def unit_eval_device(records, device=0):
    """records: structured array {op: u4, a: f4[24]} -> (n, 8) float32, evaluated by the HIP device functions."""
    records = np.ascontiguousarray(records)
    assert records.dtype.itemsize == 100
    out = np.zeros((len(records), 8), "<f4")
    _check(lib().ort_unit_eval_device(device, records.ctypes.data, len(records), out.ctypes.data))
    return out


def rgbe(r, g, b):
    return lib().ort_rgbe(r, g, b)


def write_hdr(path, image):
    image = np.ascontiguousarray(image, dtype="<f4")
    h, w = image.shape[:2]
    _check(lib().ort_write_hdr(os.fsencode(path), image.ctypes.data, w, h))


def workspace_bytes(params):
    n = C.c_uint64(0)
    _check(lib().ort_render_workspace_bytes(C.byref(params), C.byref(n)))
    return n.value


def views_workspace_bytes(params, view_count):
    n = C.c_uint64(0)
    _check(lib().ort_render_views_workspace_bytes(C.byref(params), view_count, C.byref(n)))
    return n.value


# ---- denoising (ort_denoise.h) --------------------------------------------------------------------
def _denoise_params(iterations, normal_squarings, sigma_l, sigma_z):
    for name, v in (("iterations", iterations), ("normal_squarings", normal_squarings)):
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError("%s must fit an unsigned 32-bit word, got %r" % (name, v))
    return DenoiseParams(int(iterations), int(normal_squarings), float(sigma_l), float(sigma_z))


def over_hits(plane, hits, spp):
    """a plane of render_follow or render_features (a sum divided by spp) as the mean over the samples that recorded a vertex:
    plane * spp / hits in float32, and 0 where hits is 0.  plane (..., H, W) or (..., H, W, 3), hits (..., H, W)"""
    plane, hits = np.asarray(plane, "<f4"), np.asarray(hits)
    h = hits.reshape(hits.shape + (1,) * (plane.ndim - hits.ndim)).astype("<f4")
    with np.errstate(all="ignore"):
        return np.where(h > 0, plane * np.float32(spp) / h, np.float32(0)).astype("<f4")


def _select(select):
    select = np.ascontiguousarray(np.asarray(select).astype(np.int64).reshape(-1) & 0xFFFFFFFF, dtype="<u4")
    return select, (select.ctypes.data if len(select) else None)


def matte_mask(ids, counts, spp, select, device=0, out=None):
    """ort_matte_mask: the slots of render_matte -- ids and counts (H, W, K) uint32, or with a leading V -- and a selection of ids
    (1 .. MAX_MATTE_SELECT of them; a duplicate counts once) -> out (H, W) float32: the selected slots' counts, summed, over
    float32(spp)."""
    ids, counts = np.ascontiguousarray(ids, dtype="<u4"), np.ascontiguousarray(counts, dtype="<u4")
    if ids.ndim not in (3, 4) or ids.shape != counts.shape:
        raise ValueError("ids and counts must both be (H, W, K) or (V, H, W, K), got shapes %s and %s" % (ids.shape, counts.shape))
    shape = ids.shape[:-1]
    if out is None:
        out = np.empty(shape, "<f4")
    elif not _is_plane(out, shape, "<f4"):
        raise ValueError("out must be a C-contiguous float32 array of shape %s" % (shape,))
    select, sp = _select(select)
    _check(lib().ort_matte_mask(int(device), ids.ctypes.data, counts.ctypes.data, ids.shape[-1], int(spp), sp, len(select), shape[-1], shape[-2],
                                1 if ids.ndim == 3 else shape[0], out.ctypes.data))
    return out


def matte_mask_device(d_ids, d_counts, slots, spp, select, width, height, d_out, frame_count=1, device=0, stream=None):
    """ort_matte_mask_device: raw device pointers (torch data_ptr()) of ids and counts (slots words a pixel) and of out (a float a
    pixel); select is host memory, read before the call returns.  One kernel enqueued on stream; no wait, no allocation."""
    select, sp = _select(select)
    _check(lib().ort_matte_mask_device(int(device), _ptr(d_ids), _ptr(d_counts), int(slots), int(spp), sp, len(select), int(width), int(height),
                                       int(frame_count), _ptr(d_out), _ptr(stream)))


def denoise_workspace_bytes(width, height, frame_count=1):
    n = C.c_uint64(0)
    _check(lib().ort_denoise_workspace_bytes(int(width), int(height), int(frame_count), C.byref(n)))
    return n.value


def denoise(rgb, m2, count, albedo, normal, depth, iterations=DENOISE_DEFAULTS["iterations"], sigma_l=DENOISE_DEFAULTS["sigma_l"],
            sigma_z=DENOISE_DEFAULTS["sigma_z"], normal_squarings=DENOISE_DEFAULTS["normal_squarings"], device=0, out=None):
    """ort_denoise: the mean colour rgb (H, W, 3) with its sums of squared sample luminance m2 (H, W) and sample counts count
    (H, W) uint32 -- what render_adaptive, render_sample_map or an Accumulator give -- and render_features' albedo, normal and
    depth planes -> (out (H, W, 3) float32, stats).  A leading V on every array is a batch of V frames, each denoised on its
    own.  out may be rgb itself (in place)."""
    count = np.ascontiguousarray(count, dtype="<u4")
    if count.ndim not in (2, 3):
        raise ValueError("count must be (H, W) or (V, H, W), got shape %s" % (count.shape,))
    shape = count.shape
    planes = []
    for name, a, sh in (("rgb", rgb, shape + (3,)), ("m2", m2, shape), ("albedo", albedo, shape + (3,)), ("normal", normal, shape + (3,)),
                        ("depth", depth, shape)):
        a = np.ascontiguousarray(a, dtype="<f4")
        if a.shape != sh:
            raise ValueError("%s must have shape %s, got %s" % (name, sh, a.shape))
        planes.append(a)
    if out is None:
        out = np.empty(shape + (3,), "<f4")
    elif not _is_plane(out, shape + (3,), "<f4"):
        raise ValueError("out must be a C-contiguous float32 array of shape %s" % (shape + (3,),))
    frames = 1 if count.ndim == 2 else shape[0]
    p = _denoise_params(iterations, normal_squarings, sigma_l, sigma_z)
    pl = DenoisePlanes(planes[0].ctypes.data, planes[1].ctypes.data, count.ctypes.data, planes[2].ctypes.data, planes[3].ctypes.data,
                       planes[4].ctypes.data)
    st, stats = _stats()
    _check(lib().ort_denoise(int(device), C.byref(p), C.byref(pl), shape[-1], shape[-2], frames, out.ctypes.data, st))
    return out, stats()


def denoise_device(d_rgb, d_m2, d_count, d_albedo, d_normal, d_depth, width, height, d_out, d_workspace, workspace_bytes, frame_count=1,
                   iterations=DENOISE_DEFAULTS["iterations"], sigma_l=DENOISE_DEFAULTS["sigma_l"], sigma_z=DENOISE_DEFAULTS["sigma_z"],
                   normal_squarings=DENOISE_DEFAULTS["normal_squarings"], device=0, stream=None, want_stats=False):
    """ort_denoise_device: raw device pointers (torch data_ptr()) of the six planes, of out (may be d_rgb) and of a workspace of
    denoise_workspace_bytes; enqueued on stream, waits only for stats -> stats or None"""
    p = _denoise_params(iterations, normal_squarings, sigma_l, sigma_z)
    pl = DenoisePlanes(*[p_ if p_ else None for p_ in (d_rgb, d_m2, d_count, d_albedo, d_normal, d_depth)])
    st, stats = _stats(want_stats)
    _check(lib().ort_denoise_device(int(device), C.byref(p), C.byref(pl), int(width), int(height), int(frame_count), _ptr(d_out),
                                    _ptr(d_workspace), int(workspace_bytes), _ptr(stream), st))
    return stats()


# ---- planning the next pass's sample map (ort_sampleplan.h) -----------------------------------------
def _plan_params(tolerance, floor, radius, pilot, min_add, cap, rgb_is_sum, budget):
    for name, v in (("radius", radius), ("pilot", pilot), ("min_add", min_add), ("cap", cap)):
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError("%s must fit an unsigned 32-bit word, got %r" % (name, v))
    budget = 0 if budget is None else int(budget)
    if not 0 <= budget <= 0xFFFFFFFFFFFFFFFF:
        raise ValueError("budget must fit an unsigned 64-bit word, got %r" % (budget,))
    return PlanParams(float(tolerance), float(floor), int(radius), int(pilot), int(min_add), int(cap), 1 if rgb_is_sum else 0, 0, budget)


def _totals_dicts(records):
    """PLAN_TOTALS_DTYPE records -> a list of dicts"""
    return [dict(wanted=int(r["wanted"]), planned=int(r["planned"]), unconverged=int(r["unconverged"]), unknown=int(r["unknown"]),
                 invalid=int(r["invalid"]), worst=np.float32(r["worst"])) for r in records]


def plan_workspace_bytes(width, height, frames=1):
    n = C.c_uint64(0)
    _check(lib().ort_plan_samples_workspace_bytes(int(width), int(height), int(frames), C.byref(n)))
    return n.value


def plan_samples(rgb, m2, count, tolerance, floor=PLAN_DEFAULTS["floor"], radius=PLAN_DEFAULTS["radius"], pilot=PLAN_DEFAULTS["pilot"],
                 min_add=PLAN_DEFAULTS["min_add"], cap=PLAN_DEFAULTS["cap"], rgb_is_sum=False, budget=None, device=0, out=None, want_stats=False):
    """ort_plan_samples: the colour rgb (H, W, 3) -- the mean, or with rgb_is_sum the undivided sum --, the sums of squared sample
    luminance m2 (H, W) and the sample counts count (H, W) uint32 -> (map (H, W) uint32, totals dict): for every pixel the samples
    that bring the worst squared relative standard error within its (2 radius + 1)^2 window down to tolerance^2 at the variance
    measured so far, at least min_add and at most cap; pilot for a pixel that has had fewer than 2 samples; scaled down by integer
    division where the frame's sum passes budget (include/ort.h gives the rule operation by operation).  The map is what
    render_sample_map and render_accumulate take, with cap as their cap.  totals: wanted, planned, unconverged, unknown, invalid,
    worst.  A leading V on every array is a batch of V frames, each planned on its own with its own budget: totals is a list.
    want_stats: (map, totals, stats)."""
    count = np.ascontiguousarray(count, dtype="<u4")
    if count.ndim not in (2, 3):
        raise ValueError("count must be (H, W) or (V, H, W), got shape %s" % (count.shape,))
    shape = count.shape
    planes = []
    for name, a, sh in (("rgb", rgb, shape + (3,)), ("m2", m2, shape)):
        a = np.ascontiguousarray(a, dtype="<f4")
        if a.shape != sh:
            raise ValueError("%s must have shape %s, got %s" % (name, sh, a.shape))
        planes.append(a)
    if out is None:
        out = np.empty(shape, "<u4")
    elif not _is_plane(out, shape, "<u4"):
        raise ValueError("out must be a C-contiguous uint32 array of shape %s" % (shape,))
    frames = 1 if count.ndim == 2 else shape[0]
    p = _plan_params(tolerance, floor, radius, pilot, min_add, cap, rgb_is_sum, budget)
    pl = PlanPlanes(planes[0].ctypes.data, planes[1].ctypes.data, count.ctypes.data)
    totals = np.zeros(frames, PLAN_TOTALS_DTYPE)
    st, stats = _stats()
    _check(lib().ort_plan_samples(int(device), C.byref(p), C.byref(pl), shape[-1], shape[-2], frames, out.ctypes.data, totals.ctypes.data, st))
    t = _totals_dicts(totals)
    t = t[0] if count.ndim == 2 else t
    return (out, t, stats()) if want_stats else (out, t)


def plan_samples_device(d_rgb, d_m2, d_count, width, height, d_map, d_totals, d_workspace, workspace_bytes, tolerance, frame_count=1,
                        floor=PLAN_DEFAULTS["floor"], radius=PLAN_DEFAULTS["radius"], pilot=PLAN_DEFAULTS["pilot"], min_add=PLAN_DEFAULTS["min_add"],
                        cap=PLAN_DEFAULTS["cap"], rgb_is_sum=False, budget=None, device=0, stream=None, want_stats=False):
    """ort_plan_samples_device: raw device pointers (torch data_ptr()) of the three planes, of the map, of frame_count entries of
    totals (32 bytes each, PLAN_TOTALS_DTYPE; 8-byte aligned) and of a workspace of plan_workspace_bytes; the totals are zeroed
    and the kernels enqueued on stream, waits only for stats -> stats or None"""
    p = _plan_params(tolerance, floor, radius, pilot, min_add, cap, rgb_is_sum, budget)
    pl = PlanPlanes(*[p_ if p_ else None for p_ in (d_rgb, d_m2, d_count)])
    st, stats = _stats(want_stats)
    _check(lib().ort_plan_samples_device(int(device), C.byref(p), C.byref(pl), int(width), int(height), int(frame_count), _ptr(d_map),
                                         _ptr(d_totals), _ptr(d_workspace), int(workspace_bytes), _ptr(stream), st))
    return stats()


# ---- multi-GPU: block sharding and the one collective (ort_comm.cpp) -----------------------------
def shard_block_count(width, height, index, count):
    n = C.c_uint64(0)
    _check(lib().ort_shard_block_count(width, height, index, count, C.byref(n)))
    return n.value


def pack_blocks_host(image, index, count):
    """[H, W, 3] float32 -> this shard's packed blocks [n_blocks, 64, 3] (CPU)."""
    image = np.ascontiguousarray(image, dtype="<f4")
    h, w = image.shape[:2]
    out = np.zeros((shard_block_count(w, h, index, count), 64, 3), "<f4")
    _check(lib().ort_pack_blocks_host(image.ctypes.data, w, h, index, count, out.ctypes.data))
    return out


def unpack_blocks_host(packed, width, height, index, count, out=None):
    packed = np.ascontiguousarray(packed, dtype="<f4")
    if out is None:
        out = np.zeros((height, width, 3), "<f4")
    _check(lib().ort_unpack_blocks_host(packed.ctypes.data, width, height, index, count, out.ctypes.data))
    return out


def unpack_blocks_device(d_packed_ptr, width, height, index, count, d_full_ptr, stream=None):
    _check(lib().ort_unpack_blocks_device(_ptr(d_packed_ptr), width, height, index, count, _ptr(d_full_ptr), _ptr(stream)))


class Comm:
    """One rank's handle on the gather (RCCL underneath for world > 1, loaded on first use)."""

    def __init__(self, handle):
        self.handle = handle

    @staticmethod
    def unique_id():
        buf = (C.c_ubyte * COMM_ID_BYTES)()
        _check(lib().ort_comm_unique_id(buf))
        return bytes(buf)

    @classmethod
    def create(cls, unique_id, rank, world, device):
        h = C.c_void_p()
        buf = (C.c_ubyte * COMM_ID_BYTES).from_buffer_copy(unique_id) if unique_id else None
        _check(lib().ort_comm_create(buf, rank, world, device, C.byref(h)))
        return cls(h.value)

    def gather(self, d_packed_ptr, d_full_ptr, width, height, stream=None):
        _check(lib().ort_gather_framebuffer(self.handle, _ptr(d_packed_ptr), _ptr(d_full_ptr), width, height, _ptr(stream)))

    def close(self):
        if self.handle:
            lib().ort_comm_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
