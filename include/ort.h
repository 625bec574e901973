/*
 * include/ort.h -- C ABI of the MI355X-native render path (libort.so).
 *
 * Drop-in boundary for ONE path of gyuhyun-lee/offline_raytracer: the per-pixel path
 * trace `tiled_raytrace_bvh` (reference code/ray.cpp:1178-1466) and the host code on
 * either side of it that the reference keeps in main() (code/macos_main.mm).  The
 * reference has no FFI of its own; each entry point below names the reference
 * interface it replaces.  Plain pointers and sizes only.  The compute entry points
 * need a gfx950 device and fail with ORT_ERR_NO_DEVICE / ORT_ERR_HIP otherwise: there
 * is no CPU fallback for the render call.
 *
 * Framebuffer layout everywhere: packed f32 RGB, 12 B per pixel, row-major, row 0 =
 * BOTTOM of the image (ray.cpp:1215-1216; the HDR writer flips, macos_main.mm:686-704).
 */
#ifndef ORT_H
#define ORT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORT_ABI_VERSION 3

enum {
    ORT_OK = 0,
    ORT_ERR_INVALID = 1,     /* bad argument (null, empty rect, spp % chunk, ...) */
    ORT_ERR_IO = 2,          /* file cannot be opened / written */
    ORT_ERR_PARSE = 3,       /* where the reference would trip an assert (platform.h:16-20) */
    ORT_ERR_NO_DEVICE = 4,   /* no HIP device / scene not uploaded */
    ORT_ERR_HIP = 5,         /* a HIP call failed; see ort_last_error() */
    ORT_ERR_UNSUPPORTED = 6, /* e.g. OBJ v/vt faces (parser.cpp:921-923) */
    ORT_ERR_STATE = 7,       /* call order (render before commit/upload) */
    ORT_ERR_NO_MEMORY = 8,   /* a host allocation failed */
    ORT_ERR_INTERNAL = 9     /* an exception the C++ side did not expect; see ort_last_error() */
};

/* thread-local description of the last failure on this thread */
const char *ort_last_error(void);
int ort_abi_version(void);

/* ---- plain data mirrors of the reference structs ---------------------------------- */
typedef struct { float x, y, z; } ort_v3;

/* ray.h:30-40.  The coefficients are used as given: any IEEE-754 value is allowed in diffuse, specular, transmission, ior and
 * emit -- negative, above 1, denormal, +-inf, NaN (a .scn file can say them too: its lexer reads 1.0e+39 as +inf and 0.0e+39 as
 * NaN) -- and no call clamps, rejects or repairs one.  What a call returns is then the reference's own result on the same
 * numbers, in every bit, a NaN output where the reference has one (sign and payload are not promised).  What makes that hold:
 *   - a bounce adds a light's emission to a sample only when none of its components is NaN or inf (ray.cpp's guard); a primary
 *     hit on a light adds it as it stands, so a non-finite emit shows in the pixels that see the light directly and nowhere else;
 *   - a primary hit scales the path's weight by diffuse only if |diffuse|^2 > 0: false for a NaN and for a square that underflows;
 *   - the lobe weights |Kd|, |Ks|, |Kt| over their sum are NaN when the sum is 0, inf or NaN: every "choice < weight" is then
 *     false and the sample takes the specular draw and then refracts, whichever kernel flavour runs; a scene is "diffuse only"
 *     when no material passes |Ks|^2 > 0, |Kt|^2 > 0 or a specular or transmission weight > 0, the comparisons that guard the
 *     specular and transmission blocks themselves;
 *   - the stopping rule of the adaptive calls keeps sampling when its variance is NaN (a sum of squared luminance that overflowed).
 * The roulette probability rr of every call must lie in (0, 1): at rr >= 1 or NaN a path in a closed scene has no bound. */
typedef struct {
    ort_v3 diffuse;
    float specular[4]; /* .w ("alpha") is parsed but unused by the path */
    ort_v3 transmission;
    float ior;
    ort_v3 emit;
    int32_t is_light;
} ort_material;

typedef struct { ort_v3 center; float r; uint32_t mat; } ort_sphere;        /* ray.h:4-10 */
typedef struct { ort_v3 min, max; uint32_t mat; } ort_box;                  /* ray.h:12-18 */
typedef struct { ort_v3 base, axis; float r; uint32_t mat; } ort_cylinder;  /* ray.h:20-27 */
typedef struct { uint32_t type; uint32_t index; } ort_light;  /* light push buffer entry: 1 = sphere, 2 = cylinder (ray.h:97-106) */
typedef struct { ort_v3 p, x_axis, y_axis, z_axis; } ort_camera;            /* ray.h:42-49 */

/* ray.h:51-65: placed (world-space) vertices */
typedef struct {
    const float *vertices;
    uint32_t vertex_count;
    const uint32_t *indices;
    uint32_t index_count;
    uint32_t mat;
    ort_v3 aabb_min, aabb_max;
} ort_mesh;

typedef struct {
    const ort_material *materials; uint32_t material_count; /* index 0 = reserved "no hit" */
    const ort_sphere *spheres;     uint32_t sphere_count;
    const ort_box *boxes;          uint32_t box_count;
    const ort_cylinder *cylinders; uint32_t cylinder_count;
    const ort_mesh *meshes;        uint32_t mesh_count;
    const ort_light *lights;       uint32_t light_count;
    /* camera as parsed (parser.cpp:1208-1226) */
    ort_v3 camera_p;
    float camera_quat_xyzw[4];
    float camera_height_ratio;
    int32_t screen_width, screen_height;
    ort_v3 ambient;
    /* main() pushes one inert CSG shape into its octree (macos_main.mm:322-332,532-538).  It is
       never hit, but it shapes the octree node boxes, and those decide which shapes a ray that
       starts exactly on a node face can see (ray.cpp:788-803).  Non-zero: reproduce it, as
       ort_scene_load_scn always does. */
    int32_t with_reference_csg;
} ort_scene_desc;

typedef struct {
    uint32_t material_count, sphere_count, box_count, cylinder_count, mesh_count, light_count;
    uint32_t triangle_count;
    int32_t screen_width, screen_height; /* the .scn "screen" line */
    ort_v3 ambient;
    ort_v3 camera_p;
    float camera_quat_xyzw[4];
    float camera_height_ratio;
} ort_scene_info;

typedef struct {
    uint32_t node_count, leaf_count, max_leaf_prims, max_depth;
    uint64_t node_bytes, prim_bytes; /* resident in HBM after upload */
    float sah_cost;
    /* the reference-compatible loose octree kept beside it (visibility chains + fallback) */
    uint32_t ref_node_count, ref_nonempty_leaves, ref_max_leaf_records;
    uint64_t ref_bytes;
    /* analytic shapes kept out of the tree and tested outright by every ray (0: all shapes are in the tree) */
    uint32_t prologue_prims;
    /* the 4-wide form of the same tree (128-byte nodes, up to four children each), which renders of trees that do not
       fit the L2 traverse instead: half the dependent node fetches per ray */
    uint32_t wide_node_count, wide_max_depth;
} ort_tree_info;

/* work counters of one render call (device counters).  All zero unless
   ORT_RENDER_COUNTERS is passed. */
typedef struct {
    uint64_t paths, rays, node_tests, tri_tests, analytic_tests;
    uint64_t fallback_rays; /* rays re-cast on the reference-compatible octree (Exactness) */
    double kernel_ms; /* HIP-event time of the path-trace kernel(s), always filled */
} ort_stats;

typedef struct ort_scene ort_scene;

/* ---- scene ingestion (host) ---------------------------------------------------------
 * ort_scene_load_scn replaces parse_scene (parser.cpp:1184-1446) + the mesh loading and
 * placement loop of main() (macos_main.mm:342-414): .scn grammar, ASCII PLY
 * (parser.cpp:384-570) and OBJ (parser.cpp:687-982) with the reference's number lexer
 * (parser.cpp:158-250), fan triangulation and placement arithmetic, bit for bit.
 * base_dir is prepended to mesh file names exactly as given (parser.cpp:1436-1438). */
int ort_scene_load_scn(const char *scn_path, const char *base_dir, ort_scene **out);
/* the same from memory-resident text (scn_text need not be NUL-terminated) */
int ort_scene_parse_scn(const char *scn_text, size_t scn_size, const char *base_dir, ort_scene **out);
/* scene from flattened arrays (copied) */
int ort_scene_create(const ort_scene_desc *desc, ort_scene **out);
void ort_scene_destroy(ort_scene *scene);

int ort_scene_get_info(const ort_scene *scene, ort_scene_info *out);
/* copy-out accessors; cap = capacity of out in elements; returns ORT_ERR_INVALID if too small */
int ort_scene_get_materials(const ort_scene *scene, ort_material *out, uint32_t cap);
int ort_scene_get_spheres(const ort_scene *scene, ort_sphere *out, uint32_t cap);
int ort_scene_get_boxes(const ort_scene *scene, ort_box *out, uint32_t cap);
int ort_scene_get_cylinders(const ort_scene *scene, ort_cylinder *out, uint32_t cap);
int ort_scene_get_lights(const ort_scene *scene, ort_light *out, uint32_t cap);
/* borrowed pointers, valid until ort_scene_destroy */
int ort_scene_get_mesh(const ort_scene *scene, uint32_t mesh_index, ort_mesh *out);
/* camera basis for a W x H image: macos_main.mm:550-556 */
int ort_scene_get_camera(const ort_scene *scene, int32_t width, int32_t height, ort_camera *out);

/* ---- acceleration structure (host) --------------------------------------------------
 * Replaces the octree construction of main() (macos_main.mm:418-545 driving
 * ray.cpp:1799-2045).  Closest-hit results do not depend on the tree (SURVEY 8a note),
 * so this builds the GPU layout directly: a flat SoA tree with 16-byte-aligned node
 * records and triangle slabs.
 * What a shape may be.  Sizes need not be positive: a sphere or cylinder of negative or zero radius, a box with max < min or
 * max == min on any axis, a cylinder whose axis is (0, 0, 0), a mesh whose triangles have no area are all accepted, and every
 * call gives for them what the reference gives, bit for bit (a box is bounded by the min and max of its corners, a quadric by
 * |r|; where the reference's own octree, built from r * (1, 1, 1) or from 0/0, finds such a shape and where it does not is
 * reproduced by the tree kept for that purpose).
 * What is refused.  Every shape gets a bounding box, grown for spheres and cylinders by a slack that scales with the diagonal
 * of the box of ALL shapes and camera_p.  A scene in which any shape's box, after the slack, has a non-finite component or one
 * beyond 1e30 in magnitude is refused: ORT_ERR_INVALID, ort_last_error() "scene contains a non-finite or oversized primitive".
 * One huge shape is enough: with a sphere of radius 1e20 in the scene the slack of every other quadric overflows.  A NaN or
 * infinite centre, corner, radius, axis or vertex is refused for the same reason; 1e12 is accepted.  The reference renders
 * such scenes; this library does not.  A refused scene stays a valid, uncommitted handle: it still answers ort_scene_get_info and the
 * ort_scene_get_* calls, ort_scene_get_tree_info returns ORT_ERR_STATE, the next commit refuses it again in the same way, and
 * it is destroyed as any other. */
int ort_scene_commit(ort_scene *scene);
int ort_scene_get_tree_info(const ort_scene *scene, ort_tree_info *out);

/* ---- device ---------------------------------------------------------------------- */
int ort_device_count(int *count);
/* copies the committed scene into the HBM of HIP device <device> (hipSetDevice).  Also decided here, once per upload: which of
 * the scene's small read-only tables fit the slots the kernels keep in LDS -- up to 48 materials (material 0, "no hit",
 * included), up to 64 lights, up to 40 float4 of the commit's prologue shapes (a box takes 2, a sphere 1, a cylinder 4).  A
 * scene past any of the three (48 surface materials, 65 lights) renders the same image through the kernels that read all of
 * these tables from HBM, and without the ray exchange, the five-waves build, the implicit job spaces and the wide tree; ray
 * queries depend on the prologue's size alone.  The speed of that form has not been measured. */
int ort_scene_upload(ort_scene *scene, int device);

/* ---- the render call ---------------------------------------------------------------
 * One job == one call of the reference function
 *   u64 tiled_raytrace_bvh(World*, Camera*, BVHOctreeNode*, v3 *out, i32 W, i32 H,
 *                          i32 x0, i32 y0, i32 x1, i32 y1, RandomSeries*, u32 spp, f32 rr)
 * (ray.cpp:1178-1183): the pixels of [x0,x1) x [y0,y1) are rendered serially, row-major,
 * with ONE xorshift stream threaded through every pixel and sample of the rect. */
typedef struct {
    int32_t x0, y0, x1, y1;
    uint32_t rng_state; /* RandomSeries.next_random on entry (random.h:17-29) */
    uint32_t spp;
} ort_tile_job;

/* exact analogue of a single reference call; *rng_state is updated as the reference
   updates its RandomSeries.  out_rgb is a HOST buffer of width*height*3 floats; only the
   rect is written.  shape_tests (may be NULL) receives this tree's intersection-test
   count (the reference's return value is tree-dependent diagnostics). */
int ort_tiled_raytrace(ort_scene *scene, float *out_rgb, int32_t width, int32_t height, int32_t x0, int32_t y0,
                       int32_t x1, int32_t y1, uint32_t *rng_state, uint32_t spp, float rr, uint64_t *shape_tests);

/* many reference calls in one launch (one GPU lane per job).  rects must be disjoint.
   final_states (may be NULL) receives each job's final RNG state. */
int ort_tiled_raytrace_batch(ort_scene *scene, float *out_rgb, int32_t width, int32_t height,
                             const ort_tile_job *jobs, uint32_t job_count, float rr, uint32_t *final_states,
                             ort_stats *stats);

/* Seeding policies = the caller side of the reference call (main()'s tile loop,
 * macos_main.mm:602-662).  job_seed(m, j) = fmix32(m ^ (j * 2654435761u)), 0 -> 1.
 *  TILE32 : main()'s schedule: 32x32 tiles of ceil(W/32) x ceil(H/32) px, tile series =
 *           random_u32(&master) in row-major tile order, master state = seed.
 *  WHOLE  : one call over the rect, series = random_u32(&master).
 *  PIXEL  : one call per pixel (1x1 rect, all spp), series = job_seed(seed, y*W + x).
 *  CHUNK  : spp/chunk calls per pixel of <chunk> samples; call k of pixel i uses
 *           job_seed(seed, k*W*H + i); pixel = (sum_k call_k, in k order) / (spp/chunk).
 * Results are independent of how pixels are spread over lanes, workgroups or GPUs. */
enum { ORT_POLICY_TILE32 = 0, ORT_POLICY_WHOLE = 1, ORT_POLICY_PIXEL = 2, ORT_POLICY_CHUNK = 3 };

/* flags.  ORT_RENDER_PACKED (PIXEL / CHUNK policies): the output buffer holds only this shard's 8x8 blocks,
   [local block k][pixel in block, row-major 8x8][rgb] with k-th block = block id shard_index + k * shard_count of
   the row-major block grid (ceil(W/8) wide, row 0 = bottom); ort_shard_block_count blocks, 768 B each.  That is
   the layout ort_gather_framebuffer moves between GPUs. */
enum { ORT_RENDER_COUNTERS = 1, ORT_RENDER_PACKED = 2 };

typedef struct {
    int32_t width, height;
    int32_t x0, y0, x1, y1; /* pixels to render (clipped to the image) */
    int32_t policy;
    uint32_t seed;
    uint32_t spp;
    uint32_t chunk; /* ORT_POLICY_CHUNK only */
    float rr;       /* russian roulette continue probability; main() uses 0.8 */
    uint32_t flags;
    /* multi-GPU sharding of PIXEL / CHUNK renders: the image is cut into 8x8-pixel
       blocks numbered row-major; this call renders blocks with id % shard_count ==
       shard_index.  shard_count <= 1: everything. */
    uint32_t shard_index, shard_count;
} ort_render_params;

/* host framebuffer in, host framebuffer out (device staging is internal); synchronous */
int ort_render_image(ort_scene *scene, const ort_render_params *params, float *out_rgb, ort_stats *stats);

/* device framebuffer: d_out_rgb is a DEVICE pointer (width*height*3 floats) on the scene's
   device, e.g. a torch tensor's data_ptr.  Work is enqueued on hip_stream (a hipStream_t
   passed as void*, NULL = the default stream) and the call returns without waiting
   unless stats != NULL.  Pixels of other shards are left untouched. */
int ort_render_image_device(ort_scene *scene, const ort_render_params *params, void *d_out_rgb, void *hip_stream,
                            ort_stats *stats);

/* bytes of device workspace ort_render_image_device keeps for these params (CHUNK partial sums, held in the packed
   block layout: a shard keeps 1/shard_count of a frame per chunk) */
int ort_render_workspace_bytes(const ort_render_params *params, uint64_t *bytes);

/* ---- a batch of camera views in one launch ---------------------------------------------
 * The render call with the camera moved from the scene to the caller: view_count frames of one committed, uploaded
 * scene, each from a pose of its own, in ONE persistent launch over [view][block][chunk][pixel] -- a turntable, a camera
 * path, a stereo pair, many small probe views -- without re-creating the scene (tree, octree, upload) per pose and
 * without paying a launch's fixed cost per view.
 *
 * Frame identity: the output is view_count frames, view-major, each width*height*3 f32 with row 0 at the bottom.  Frame v
 * is, bit for bit, what ort_render_image would write for the same params with params.seed = views[v].seed if the scene's
 * camera basis (ort_scene_get_camera) were views[v].camera.  Seeds belong to jobs, so neither the order of the views nor
 * how the batch is cut into calls can change a bit of a frame.
 * Seed and rect: params->seed is ignored.  The rect applies to every view; pixels outside it are left untouched in every
 * frame.
 * views is a HOST array in both forms; it is copied before the call returns (as the explicit job list of
 * ort_tiled_raytrace_batch).
 * Policies: ORT_POLICY_PIXEL and ORT_POLICY_CHUNK only.  TILE32 and WHOLE, shard_count > 1 and ORT_RENDER_PACKED return
 * ORT_ERR_UNSUPPORTED: a multi-GPU caller deals views to GPUs, not blocks.
 * view_count == 0 returns ORT_OK without a launch, whatever the other arguments.  view_count above ORT_MAX_VIEWS is
 * ORT_ERR_INVALID.
 * Where a camera may stand: the fast tree's quadric boxes are sized for ray origins within the box of all shapes and the
 * scene's own camera_p, with 0.25 of slack per side (ort_scene_commit; DESIGN.md, render_views).  A view is accepted only
 * if its aperture's bounding box -- per component k, p_k - 0.1 z_k +- 0.1 |x_k| +- 0.1 |y_k| -- has finite components and
 * lies inside that box grown by 0.25 per side; otherwise the call returns ORT_ERR_UNSUPPORTED and ort_last_error() names
 * the first offending view.  Bounce rays start at hits and need no rule.  A caller who needs a camera further out creates
 * the scene with a camera_p out there.
 * Errors are reported before any device work, in this order: ORT_ERR_INVALID (nulls, empty or bad params exactly as
 * ort_render_image judges them, view cap exceeded), ORT_ERR_UNSUPPORTED (policy, shard, packed, camera outside the box),
 * ORT_ERR_STATE (scene not committed), ORT_ERR_NO_DEVICE (not uploaded).
 * stats as for the render call; with ORT_RENDER_COUNTERS paths = view_count * pixels * spp. */
typedef struct { ort_camera camera; uint32_t seed; } ort_view; /* 52 B */
#define ORT_MAX_VIEWS 4096u

/* macos_main.mm:550-556 for a caller's pose: what ort_scene_get_camera does for the scene's own */
int ort_camera_from_pose(const float p[3], const float quat_xyzw[4], float height_ratio, int32_t width, int32_t height,
                         ort_camera *out);

/* host views in, host frames out (view_count * width*height*3 floats; device staging is internal); synchronous */
int ort_render_views(ort_scene *scene, const ort_render_params *params, const ort_view *views, uint32_t view_count,
                     float *out_rgb, ort_stats *stats);
/* d_out_rgb is a DEVICE pointer (view_count * width*height*3 floats) on the scene's device; enqueued on hip_stream,
   returns without waiting unless stats != NULL -- as ort_render_image_device */
int ort_render_views_device(ort_scene *scene, const ort_render_params *params, const ort_view *views, uint32_t view_count,
                            void *d_out_rgb, void *hip_stream, ort_stats *stats);
/* view_count times ort_render_workspace_bytes: the CHUNK partial planes are per view */
int ort_render_views_workspace_bytes(const ort_render_params *params, uint32_t view_count, uint64_t *bytes);

/* ---- closest-hit ray queries ----------------------------------------------------------
 * Replaces raycast_top_most_node (reference code/ray.cpp:1165-1176): the closest hit of each of the caller's rays,
 * bit for bit the reference's hit_t, hit_normal and hit_mat_index (ties in the reference's test order, phantom
 * sphere hits and visibility chains included).  A miss is t = FLT_MAX, n = 0, mat = 0, prim = ORT_NO_PRIM.
 * A shape may itself carry material 0, the "no hit" material: in a .scn file every sphere, box, cylinder or mesh written
 * before the first `brdf` or `light` line does (parser.cpp:1260-1440), and ort_scene_create accepts mat = 0 on any shape.
 * Such a shape is geometry like any other and wins closest-hit contests: a hit on it returns the shape's t, n and prim
 * with mat = 0 -- never ORT_NO_PRIM with a finite t.  What a caller of the hit makes of mat = 0 is said per query below.
 * Rays: count x {o.xyz, d.xyz} f32, 24 B each; d need not be of unit length (the reference does not normalise it),
 * zero components are allowed.  Every IEEE-754 ray gets the reference's answer, NaN, infinite, zero, subnormal and
 * overflowing components included: every non-NaN output bit for bit, a NaN output NaN in the same field and component
 * (its sign and payload are not part of the contract: x86 and gfx950 make different default NaNs).  Rays the fast tree
 * cannot answer exactly take the exact octree walk, roughly 1 000x slower per ray: |d|^2 < 0.999 with spheres in the
 * tree, an origin outside the scene's box with quadrics in it, and a +-0 or NaN direction component (axis-aligned
 * rays) when boxes are in it (raycast_rays).  hits[i] answers rays[i];
 * results do not depend on count, order or how the batch is sliced.
 * prim = kind << 28 | index: index is the shape's position in the scene's own arrays (the get_spheres / get_boxes /
 * get_cylinders order), for triangles the mesh-major triangle id (triangles of the earlier meshes, then the
 * triangle within its mesh, index_count / 3 per mesh).
 * flags: ORT_RENDER_COUNTERS fills the work counters of stats (rays, node / triangle / analytic tests); stats (may be
 * NULL) always gets fallback_rays and kernel_ms, paths = 0.
 * Both pointers must be 8-byte aligned.  Errors are reported before any device work: ORT_ERR_INVALID (null or
 * misaligned pointer with count > 0), ORT_ERR_STATE (scene not committed), ORT_ERR_NO_DEVICE (not uploaded);
 * count == 0 returns ORT_OK without a launch. */
typedef struct { float t; ort_v3 n; uint32_t mat; uint32_t prim; } ort_hit; /* 24 B */
enum { ORT_HIT_TRIANGLE = 0, ORT_HIT_BOX = 2, ORT_HIT_CYLINDER = 3, ORT_HIT_SPHERE = 4 };
#define ORT_NO_PRIM 0xffffffffu

/* host rays in, host hits out; synchronous (staged through device buffers kept per scene, in bounded slices) */
int ort_raycast(ort_scene *scene, const float *rays, uint64_t count, ort_hit *hits, uint32_t flags, ort_stats *stats);
/* DEVICE rays and hits on the scene's device (e.g. torch tensors' data_ptr); enqueued on hip_stream (NULL = the
   default stream), returns without waiting unless stats != NULL -- as the device form of the render call */
int ort_raycast_device(ort_scene *scene, const void *d_rays, uint64_t count, void *d_hits, uint32_t flags,
                       void *hip_stream, ort_stats *stats);

/* ---- occlusion ray queries ------------------------------------------------------------
 * "Is anything in the way before tmax?" -- shadow rays, ambient occlusion, line of sight.  With h the closest hit
 * ort_raycast returns for rays[i] (the reference's raycast_top_most_node answer, bit for bit):
 *     occluded[i] = (h.mat != 0 && h.t < tmax[i]) ? 1 : 0
 * Rays as for ort_raycast (24 B each, d not normalised, any IEEE-754 bits); tmax[i] is in units of the ray parameter,
 * the same t as ort_hit.t.  The comparison is the IEEE one: a NaN tmax or a NaN h.t gives 0; tmax <= 0, -0.0 and
 * -inf give 0; a miss (t = FLT_MAX, mat = 0) gives 0 for every tmax, +inf included; tmax == h.t gives 0 (strict),
 * the next float above h.t gives 1.  A closest hit on a shape that carries material 0 (see ort_raycast) gives byte 0
 * for every tmax too, tmax == NULL included, even where a solid surface lies behind it below tmax: only the closest
 * hit is asked.  A solid shape in front of such a shape is the ordinary comparison.  tmax == NULL means no limit: the
 * answers of tmax[i] = +inf.  The output is one byte per ray, exactly 0 or 1 (the layout of a bool tensor).
 * occluded[i] answers rays[i]; results do not depend on count, order or how the batch is sliced.  There is no tmin:
 * the intersectors' own threshold (1e-6) stands.
 * The traversal never looks beyond tmax, writes one byte instead of 24 and needs no shape table; the rays that
 * ort_raycast sends to the exact octree walk take it here too (occluded_rays).
 * flags and stats as for ort_raycast.  rays must be 8-byte aligned, a non-NULL tmax 4-byte aligned.  count == 0 returns
 * ORT_OK without a launch, whatever the other arguments.  Otherwise errors are reported before any device work, in
 * this order: ORT_ERR_INVALID (null scene, rays or occluded; misaligned rays or tmax), ORT_ERR_STATE (scene not
 * committed), ORT_ERR_NO_DEVICE (not uploaded). */

/* host rays (and limits) in, host bytes out; synchronous (staged through device buffers kept per scene, in bounded slices) */
int ort_occluded(ort_scene *scene, const float *rays, const float *tmax, uint64_t count, uint8_t *occluded, uint32_t flags,
                 ort_stats *stats);
/* DEVICE rays, limits (may be NULL) and bytes on the scene's device; enqueued on hip_stream (NULL = the default
   stream), returns without waiting unless stats != NULL -- as ort_raycast_device */
int ort_occluded_device(ort_scene *scene, const void *d_rays, const void *d_tmax, uint64_t count, void *d_occluded,
                        uint32_t flags, void *hip_stream, ort_stats *stats);

/* ---- radiance queries -----------------------------------------------------------------
 * The path-traced light that arrives along a caller's own ray: light probes, irradiance and lightmap baking, sparse or
 * foveated pixel sets, "rays in, colours out" batches -- the path tracer without its camera.
 * out_rgb[i] is the reference's pixel value for a pixel whose every sample starts at o_i in direction d_i: the sample body
 * of tiled_raytrace_bvh (ray.cpp:1247-1426: closest hit, emission, roulette, BSDF sampling, bounces) with wo =
 * -normalize(d_i), run spp times on ONE xorshift stream that starts at seeds[i], WITHOUT the aperture draw of a camera
 * sample (ray.cpp:1232); the samples' colours are summed in sample order and divided by (float)spp, component by
 * component.  Bit for bit.  final_states[i] (final_states may be NULL) is the stream's state afterwards.  A seed of 0 is
 * taken as 1, as the per-pixel seeding policies never hand out 0: a zero xorshift state never leaves zero.
 * Rays as for ort_raycast: count x {o.xyz, d.xyz} f32, 24 B each, 8-byte aligned.  out_rgb is count x 3 f32, seeds and
 * final_states count x u32 (4-byte aligned).  out_rgb[i] answers rays[i] with seeds[i]; results do not depend on count,
 * order, how the batch is sliced or how rays fall on the GPU's lanes.
 * The per-ray domain: d must be what a primary direction is in the reference -- all six components of the ray finite and
 * |d|^2 (f32: x*x + y*y + z*z) within [0.999, 1.001].  A ray outside this domain gets out_rgb[i] = NaN NaN NaN and
 * final_states[i] = seeds[i] (as given, 0 included), and is not traced; the other rays of the call are unaffected.  Inside the domain
 * every ray gets the exact answer, axis-aligned directions and origins far outside the scene included: the primary rays
 * that ort_raycast sends to the exact octree walk (a +-0 direction component with boxes in the tree, an origin outside the
 * scene's box with quadrics in it) take it here too, roughly 1 000x slower per primary ray (radiance_rays).
 * Bounce rays start at hits and need no rule.
 * rr is the roulette's survival probability, as ort_render_params.rr, here within [0, 1): at 1 no path in a closed room ends.
 * flags: ORT_RENDER_COUNTERS fills the work counters of stats, paths = (rays inside the domain) * spp; stats (may be NULL)
 * always gets fallback_rays and kernel_ms.
 * count == 0 returns ORT_OK without a launch, whatever the other arguments.  Otherwise errors are reported before any
 * device work, in this order: ORT_ERR_INVALID (null scene, rays, seeds or out_rgb; misaligned pointer; spp == 0; rr
 * outside [0, 1) or NaN), ORT_ERR_STATE (scene not committed), ORT_ERR_NO_DEVICE (not uploaded). */

/* host rays and seeds in, host colours (and states) out; synchronous (staged through device buffers kept per scene, in
   bounded slices) */
int ort_radiance(ort_scene *scene, const float *rays, const uint32_t *seeds, uint64_t count, uint32_t spp, float rr,
                 float *out_rgb, uint32_t *final_states /* may be NULL */, uint32_t flags, ort_stats *stats);
/* DEVICE rays, seeds, colours and states (may be NULL) on the scene's device; enqueued on hip_stream (NULL = the default
   stream), returns without waiting unless stats != NULL -- as ort_raycast_device */
int ort_radiance_device(ort_scene *scene, const void *d_rays, const void *d_seeds, uint64_t count, uint32_t spp, float rr,
                        void *d_out_rgb, void *d_final_states, uint32_t flags, void *hip_stream, ort_stats *stats);

/* ---- adaptive radiance queries ----------------------------------------------------------
 * ort_radiance with a sample count per ray: every ray is sampled until the estimated standard error of its mean luminance is
 * small against the mean, between min_spp and max_spp samples.  A ray that looks at a light or into the dark stops at min_spp,
 * a ray that sees light only after bounces runs on -- decided in the lane that traces it, with no trip to the host.
 * Rays, seeds, the per-ray domain, rr, alignment, final_states, independence of count, order and slicing, and the host and the
 * device form are exactly as for ort_radiance.  Per ray, every operation a separately rounded f32 operation (no FMA):
 *  - Samples.  Samples are ort_radiance's samples.  Each is the reference's sample body from the ray, on one xorshift stream
 *    that starts at seeds[i] (0 is taken as 1).
 *  - Colour sum.  C is the running colour sum.  It starts at 0, and a sample adds at most one vector e to it: the emission term
 *    of ray.cpp:1254-1259 or :1358-1371.
 *  - Second moment.  Q is the running sum of squared sample luminance.  Whenever a vector e is added to C, compute
 *    y = (0.2126f*e.x + 0.7152f*e.y) + 0.0722f*e.z, then Q = Q + y*y.  A sample that adds nothing leaves Q unchanged.
 *  - When checks happen.  A check runs after sample n when n >= min_spp, n < max_spp and (n - min_spp) % check_every == 0.
 *  - The check.
 *        fn  = (float)n
 *        Y   = (0.2126f*C.x + 0.7152f*C.y) + 0.0722f*C.z
 *        m   = Y / fn
 *        v   = Q / fn - m*m;   if (v < 0) v = 0;          (NaN stays NaN)
 *        vm  = v / (fn - 1.0f)
 *        a   = m < 0 ? -m : m;   b = a > floor ? a : floor
 *        thr = tolerance * b
 *        stop iff vm <= thr*thr                            (false, NaN included: keep sampling)
 *  - Stopping.  The ray stops at the first check that says stop.  Otherwise it stops at n = max_spp.
 *  - Outputs.  out_rgb[i] = C / (float)n, component by component (ray.cpp:1428 with n in place of spp); out_spp[i] = n;
 *    out_m2[i] = Q; final_states[i] is the stream's state after sample n.  out_spp, out_m2 and final_states may each be NULL.
 * What the rule means: it compares the estimated standard error of the mean luminance, sqrt(vm), against tolerance times the
 * mean's magnitude, with floor standing in for the magnitude in the dark.  A caller rebuilds the estimate from the three
 * outputs: n = out_spp[i]; the mean luminance m = luminance(out_rgb[i]) (Y / n up to one rounding); the sample variance
 * v = max(0, out_m2[i] / n - m*m); the standard error of the mean sqrt(v / (n - 1)).  The sums themselves are C = out_rgb[i] * n
 * (up to one rounding) and Q = out_m2[i].
 * The known weakness: a ray that has seen no light in its first min_spp samples has v == 0 and stops black, though light might
 * have reached it later (a small or far light seen only after bounces).  Callers pick min_spp for their scene.
 * A ray outside the per-ray domain gets out_rgb = NaN NaN NaN, out_spp = 0, out_m2 = 0 and final_states[i] = seeds[i]; its
 * neighbours are unaffected.
 * Two identities: with min_spp == max_spp == n no check runs, and colours and final states are ort_radiance's at spp = n, bit for
 * bit; with a tolerance so large that thr*thr is +inf every ray with finite Q stops at min_spp with ort_radiance's results at
 * spp = min_spp.
 * flags and stats as for ort_radiance; with ORT_RENDER_COUNTERS, paths is the number of samples taken: the sum of out_spp.
 * count == 0 returns ORT_OK without a launch, whatever the other arguments.  Otherwise errors are reported before any device
 * work, in ort_radiance's order with ad in the place of spp: ORT_ERR_INVALID (null scene, rays, seeds or out_rgb; misaligned
 * rays (8 bytes), seeds, out_rgb, out_spp, out_m2 or final_states (4 bytes); ad == NULL, min_spp < 2, max_spp < min_spp, max_spp >
 * 1 << 24 -- (float)n must be exact --, check_every == 0, tolerance or floor NaN, infinite or negative; rr outside [0, 1) or
 * NaN), ORT_ERR_STATE (scene not committed), ORT_ERR_NO_DEVICE (not uploaded). */
typedef struct { uint32_t min_spp, max_spp, check_every; float tolerance, floor; } ort_adaptive; /* 20 B */

/* host rays and seeds in, host colours (and counts, second moments, states) out; synchronous, staged as ort_radiance */
int ort_radiance_adaptive(ort_scene *scene, const float *rays, const uint32_t *seeds, uint64_t count, const ort_adaptive *ad, float rr,
                          float *out_rgb, uint32_t *out_spp /* may be NULL */, float *out_m2 /* may be NULL */,
                          uint32_t *final_states /* may be NULL */, uint32_t flags, ort_stats *stats);
/* DEVICE pointers on the scene's device; enqueued on hip_stream (NULL = the default stream), returns without waiting unless
   stats != NULL -- as ort_radiance_device */
int ort_radiance_adaptive_device(ort_scene *scene, const void *d_rays, const void *d_seeds, uint64_t count, const ort_adaptive *ad, float rr,
                                 void *d_out_rgb, void *d_out_spp, void *d_out_m2, void *d_final_states, uint32_t flags, void *hip_stream,
                                 ort_stats *stats);

/* ---- irradiance queries: cosine-weighted hemisphere gathers at points -------------------------
 * Light probes, irradiance and lightmap baking from what a baker has: points and normals, not rays.  out_rgb[i] is the
 * cosine-weighted mean of the radiance that arrives at p_i over the hemisphere about n_i: spp samples, each a direction drawn
 * about n_i with the reference's own diffuse lobe and then ort_radiance's sample along it.  IRRADIANCE is pi * out_rgb; the
 * radiosity of a diffuse texel with reflectance kd is kd * out_rgb (component by component).  The mean is returned as it is,
 * C / (float)n, so that no rounding is added to it.
 * points is count x {p.xyz, n.xyz} f32, 24 B each, 8-byte aligned: the layout of a ray, staged, sliced and checked as
 * ort_radiance's rays.  p is used as given: a caller lifts it off its surface first (say p + 1e-3 n), or every sample starts
 * inside the surface's own intersection threshold.
 * The per-point domain is ort_radiance's per-ray test applied to (p, n): six finite components and |n|^2 (f32: x*x + y*y + z*z)
 * within [0.999, 1.001].  A point outside it gets out_rgb[i] = NaN NaN NaN and final_states[i] = seeds[i] (as given, 0
 * included) -- in the adaptive form also out_spp[i] = 0 and out_m2[i] = 0 --, is not traced, and leaves its neighbours alone.
 * A point's samples run on ONE xorshift stream that starts at seeds[i] (0 is taken as 1).  Per sample, every operation a
 * separately rounded f32 operation (no FMA):
 *        e0  = rng_01(s);  e1 = rng_01(s)               (random.h: two steps of the stream)
 *        c   = sqrtf(e0)                                 (ray.cpp:1123, the diffuse lobe)
 *        phi = (2.0f * kPi) * e1                         (sample_brdf's azimuth)
 *        m   = sample_lobe(n, c, phi)                    (ray.cpp:1065-1091: n normalised inside, cos/sin of the deterministic libm)
 *        d   = normalize(m)
 *   then ort_radiance's sample from the ray (p, d) on the same stream s: direction d as it stands, wo = -normalize(d), no aperture
 *   draw, the sample body of ray.cpp:1247-1426.  This is sample_brdf's diffuse draw without its lobe-choice draw.
 * The samples' colours are summed in sample order and divided by (float)spp, component by component; final_states[i] (may be
 * NULL) is the stream's state afterwards.
 * Two identities.  With s'_k the stream's state after sample k's two direction draws (never 0), sample k's colour and the state
 * after it are, bit for bit, ort_radiance's for the single ray (p, d_k) with seed s'_k at spp = 1.  With rr = 0 the roulette never
 * continues: with h the closest hit of (p, d_k), sample k adds the emission of h's material if that is a light and nothing
 * otherwise, and draws one more rng_01 exactly when h.mat != 0 and the material is not a light.
 * rr, flags, stats, count == 0, alignment, the order of the errors (before any device work) and independence of count, order and
 * slicing are ort_radiance's, with points where rays stand.  With ORT_RENDER_COUNTERS, paths = (points inside the domain) * spp.
 * A primary ray that ort_raycast would send to the exact octree walk takes it here too, per SAMPLE: p outside the scene's box
 * with quadrics in the tree (every sample of such a point), a +-0 component of d_k with boxes in it.  Such points cost about
 * 1 000x per sample (irradiance_points).
 * The adaptive form is ort_radiance_adaptive's rule, unchanged, over these samples: the same C, Q, checks, outputs (out_spp,
 * out_m2 and final_states may each be NULL), the same validation of ad, the same two identities -- with min_spp == max_spp == n it
 * gives ort_irradiance's bits at spp = n -- and, with ORT_RENDER_COUNTERS, paths = the sum of out_spp. */

/* host points and seeds in, host colours (and states) out; synchronous, staged as ort_radiance */
int ort_irradiance(ort_scene *scene, const float *points, const uint32_t *seeds, uint64_t count, uint32_t spp, float rr,
                   float *out_rgb, uint32_t *final_states /* may be NULL */, uint32_t flags, ort_stats *stats);
/* DEVICE pointers on the scene's device; enqueued on hip_stream (NULL = the default stream), returns without waiting unless
   stats != NULL -- as ort_radiance_device */
int ort_irradiance_device(ort_scene *scene, const void *d_points, const void *d_seeds, uint64_t count, uint32_t spp, float rr,
                          void *d_out_rgb, void *d_final_states, uint32_t flags, void *hip_stream, ort_stats *stats);
/* the adaptive form, host and device: as ort_radiance_adaptive and ort_radiance_adaptive_device */
int ort_irradiance_adaptive(ort_scene *scene, const float *points, const uint32_t *seeds, uint64_t count, const ort_adaptive *ad, float rr,
                            float *out_rgb, uint32_t *out_spp /* may be NULL */, float *out_m2 /* may be NULL */,
                            uint32_t *final_states /* may be NULL */, uint32_t flags, ort_stats *stats);
int ort_irradiance_adaptive_device(ort_scene *scene, const void *d_points, const void *d_seeds, uint64_t count, const ort_adaptive *ad, float rr,
                                   void *d_out_rgb, void *d_out_spp, void *d_out_m2, void *d_final_states, uint32_t flags, void *hip_stream,
                                   ort_stats *stats);

/* ---- SH light-probe queries: radiance over the sphere as 9 SH coefficients ---------------------
 * A light probe is not tied to a normal: it stores the radiance that arrives at a point from ALL directions, so that any normal can
 * be shaded from it later.  out_sh[i] holds, per colour channel, the means over spp uniformly drawn directions of the arriving
 * radiance times the nine real spherical harmonics of bands 0 to 2.  The mean is returned as it stands, S / (float)spp, so that no
 * rounding is added: the SH COEFFICIENTS of the radiance field are 4 pi * out_sh (the sphere's measure over the uniform density),
 * as irradiance is pi * ort_irradiance's mean.
 *  - Inputs.  points is ort_irradiance's array: count x {p.xyz, n.xyz} f32, 24 B each, 8-byte aligned; the per-point domain test is
 *    the same and p is used as given.  Here n is only the POLE of the sample pattern (c below is the cosine to it): a caller without
 *    a preference passes (0, 0, 1).  The SH basis is always in world axes, whatever n is.  seeds is count x u32.
 *  - One sample.  A point's samples run on ONE xorshift stream that starts at seeds[i] (0 is taken as 1).  Per sample, every
 *    operation a separately rounded f32 operation (no FMA):
 *        e0  = rng_01(s);  e1 = rng_01(s)
 *        c   = 1.0f - 2.0f * e0                          (uniform over the sphere; ort_irradiance has sqrtf(e0) here)
 *        phi = (2.0f * kPi) * e1
 *        m   = sample_lobe(n, c, phi);  d = normalize(m)
 *    then ort_radiance's sample from the ray (p, d) on the same stream: direction d as it stands, wo = -normalize(d), no aperture
 *    draw.  Whenever that sample adds a vector e to the colour sum C -- the primary hit's emission, or a bounce's emission that
 *    passed the finite check -- the basis is formed from x, y, z = d (the sample's PRIMARY direction, also at a bounce):
 *        b0 = 0.282094792f
 *        b1 = 0.488602512f*y          b2 = 0.488602512f*z          b3 = 0.488602512f*x
 *        b4 = 1.092548431f*(x*y)      b5 = 1.092548431f*(y*z)      b6 = 0.315391565f*(3.0f*(z*z) - 1.0f)
 *        b7 = 1.092548431f*(x*z)      b8 = 0.546274215f*(x*x - y*y)
 *        S[j] = S[j] + b_j * e        component by component, the product rounded and then the sum; S starts at +0
 *  - Outputs.  out_sh is count x ORT_SH_COEFFS x 3 f32, [point][coefficient][rgb], and holds S[j] / (float)spp.  out_rgb (may be
 *    NULL) is count x 3 f32, C / (float)spp: the plain mean, which is also out_sh[i][0] / b0 up to rounding.  final_states (may be
 *    NULL) is the stream's state after the last sample.
 *  - Outside the domain.  Such a point gets NaN in all 27 words of out_sh[i] and in out_rgb[i], and final_states[i] = seeds[i] (as
 *    given, 0 included); it is not traced, and its neighbours are unaffected.
 *  - Two identities, in ort_irradiance's form.  I1: with s'_k the stream's state after sample k's two direction draws, sample k's
 *    colour and the state after it are, bit for bit, ort_radiance's for the single ray (p, d_k) with seed s'_k at spp = 1; d_k is
 *    unit op 21's direction for the state before the sample, and b1 ... b8 are unit op 22's.  I2: with rr = 0 the roulette never
 *    continues: with h the closest hit of (p, d_k), sample k adds the emission of h's material if that is a light and nothing
 *    otherwise, and draws one more rng_01 exactly when h.mat != 0 and the material is not a light.
 *  - rr, flags, stats, count == 0, alignment and the order of the errors (before any device work) are ort_irradiance's, with out_sh
 *    where out_rgb stood as the required output: ORT_ERR_INVALID (null scene, points, seeds or out_sh; misaligned points (8 bytes),
 *    seeds, out_sh, out_rgb or final_states (4 bytes); spp == 0; rr outside [0, 1) or NaN), ORT_ERR_STATE, ORT_ERR_NO_DEVICE.
 *    With ORT_RENDER_COUNTERS, paths = (points inside the domain) * spp.  Results do not depend on count, order, how the batch is
 *    sliced or how points fall on the GPU's lanes.  Primary rays take the exact octree walk where ort_irradiance's do. */
#define ORT_SH_COEFFS 9u

/* host points and seeds in, host coefficients (and means, states) out; synchronous, staged as ort_radiance */
int ort_probe_sh(ort_scene *scene, const float *points, const uint32_t *seeds, uint64_t count, uint32_t spp, float rr,
                 float *out_sh, float *out_rgb /* may be NULL */, uint32_t *final_states /* may be NULL */, uint32_t flags,
                 ort_stats *stats);
/* DEVICE pointers on the scene's device; enqueued on hip_stream (NULL = the default stream), returns without waiting unless
   stats != NULL -- as ort_radiance_device */
int ort_probe_sh_device(ort_scene *scene, const void *d_points, const void *d_seeds, uint64_t count, uint32_t spp, float rr,
                        void *d_out_sh, void *d_out_rgb, void *d_final_states, uint32_t flags, void *hip_stream, ort_stats *stats);

/* ---- ambient-occlusion queries: hemisphere visibility gathers at points ------------------------
 * The visibility gather of a baker's texel or probe: ambient occlusion, a bent normal, "how much sky does this point see within
 * r".  ort_irradiance's points, seeds and direction draw; ort_occluded's answer along every drawn direction.
 *  - Inputs.  points is ort_irradiance's array: count x {p.xyz, n.xyz} f32, 24 B each, 8-byte aligned.  seeds is count x u32.  The
 *    per-point domain and the treatment of p are ort_irradiance's: six finite components, |n|^2 (f32: x*x + y*y + z*z) within
 *    [0.999, 1.001], p used as given (a caller lifts it off its surface first).
 *  - The radius.  radius is count x f32, 4-byte aligned, in units of the ray parameter; directions are unit vectors, so it is a
 *    distance.  It is ort_occluded's tmax, with that call's IEEE rules.  radius == NULL means no limit.  A NaN or <= 0 radius
 *    (-0.0 and -inf included) leaves every sample of that point open.
 *  - One sample.  A point's samples run on ONE xorshift stream that starts at seeds[i] (0 is taken as 1).  Sample k is
 *    ort_irradiance's direction draw, every operation a separately rounded f32 operation (no FMA):
 *        e0  = rng_01(s);  e1 = rng_01(s)
 *        c   = sqrtf(e0)
 *        phi = (2.0f * kPi) * e1
 *        m   = sample_lobe(n, c, phi)
 *        d_k = normalize(m)
 *    and then o_k, the byte ort_occluded returns for the ray (p, d_k) with tmax = radius[i]: (h.mat != 0 && h.t < radius[i]) of the
 *    reference's closest hit h.  Nothing else is drawn: the stream advances exactly two steps per sample, whatever is hit.
 *    A sample whose closest hit is on a shape that carries material 0 (see ort_raycast) is therefore an open sample, at every
 *    radius, and its direction enters the bent sum.
 *  - Outputs.  out_open[i] is the number of samples with o_k == 0: visibility is out_open / spp, ambient occlusion one minus that;
 *    the count is returned so that no rounding is added.  out_bent (may be NULL) is count x 3 f32: B starts at (+0, +0, +0) and,
 *    for every open sample in sample order, B = B + d_k component by component, each a separately rounded f32 add; B is returned as
 *    it stands -- the caller normalises it, and |B| / out_open measures the open cone.  final_states[i] (may be NULL) is the stream
 *    after 2 * spp steps.
 *  - Outside the domain.  Such a point gets out_open[i] = ORT_AO_INVALID, out_bent = NaN NaN NaN and final_states[i] = seeds[i] (as
 *    given, 0 included), is not traced, and leaves its neighbours alone.
 *  - Identities.  Sample k's bit is ort_occluded's for (p, d_k) at that radius; d_k is unit op 20's direction for the stream's
 *    state before the sample; final_states does not depend on the scene; results do not depend on count, order, how the batch is
 *    sliced or how points fall on the GPU's lanes.
 *  - Flags and statistics as for ort_occluded.  With ORT_RENDER_COUNTERS, rays = (points inside the domain) * spp -- a sample is
 *    counted before its radius is looked at --, paths = 0; fallback_rays and kernel_ms are always filled.  A sample that
 *    ort_occluded would send to the exact octree walk takes it here too: every sample of a point outside the scene's box with
 *    quadrics in the tree, a +-0 component of d_k with boxes in it.
 *  - Errors.  count == 0 returns ORT_OK without a launch, whatever the other arguments.  Otherwise errors are reported before any
 *    device work, in this order: ORT_ERR_INVALID (null scene, points, seeds or out_open; misaligned points (8 bytes) or any other
 *    array (4 bytes); spp == 0), ORT_ERR_STATE (scene not committed), ORT_ERR_NO_DEVICE (not uploaded). */
#define ORT_AO_INVALID 0xffffffffu

/* host arrays in, host counts (and bent sums, states) out; synchronous, staged as ort_radiance */
int ort_ambient_occlusion(ort_scene *scene, const float *points, const uint32_t *seeds, const float *radius /* may be NULL */,
                          uint64_t count, uint32_t spp, uint32_t *out_open, float *out_bent /* may be NULL */,
                          uint32_t *final_states /* may be NULL */, uint32_t flags, ort_stats *stats);
/* DEVICE pointers on the scene's device; enqueued on hip_stream (NULL = the default stream), returns without waiting unless
   stats != NULL -- as ort_occluded_device */
int ort_ambient_occlusion_device(ort_scene *scene, const void *d_points, const void *d_seeds, const void *d_radius, uint64_t count,
                                 uint32_t spp, void *d_out_open, void *d_out_bent, void *d_final_states, uint32_t flags,
                                 void *hip_stream, ort_stats *stats);

/* ---- the adaptive camera render: one frame, or a batch of views ---------------------------------
 * The camera render with a sample count per pixel: "this noise level, at most max_spp samples", and a sample-count map back.
 * A pixel job under ORT_POLICY_PIXEL is all samples of pixel (x, y) on the stream job_seed(seed, y*W + x); the adaptive render is
 * that job cut by the rule of ort_radiance_adaptive, unchanged.  Per pixel, every operation a separately rounded f32 operation:
 *  - Samples.  A sample is a CAMERA sample of the reference (ray.cpp:1215-1426): the aperture draw of ray.cpp:1232 is part of it,
 *    unlike in the radiance queries.  The pixel's samples run on one xorshift stream that starts at job_seed(seed, y*W + x).
 *  - Colour sum and second moment.  C, Q, y and the luminance weights are as defined for ort_radiance_adaptive: a sample adds at
 *    most one vector e to C, and then Q = Q + y*y with y = (0.2126f*e.x + 0.7152f*e.y) + 0.0722f*e.z.
 *  - When checks happen.  A check runs after sample n when n >= min_spp, n < max_spp and (n - min_spp) % check_every == 0.
 *  - The check.  As given for ort_radiance_adaptive, operation by operation (fn, Y, m, v, vm, a, b, thr; stop iff vm <= thr*thr).
 *  - Stopping.  The pixel stops at the first check that says stop, otherwise at n = max_spp.
 *  - Outputs.  pixel = C / (float)n, component by component (ray.cpp:1428 with n in place of spp).
 * Per-pixel outputs, each a plane of width*height entries per frame with row 0 at the bottom:
 *    out_rgb       3 f32 per pixel   the mean colour
 *    out_spp       u32               n, the samples taken                         (may be NULL)
 *    out_m2        f32               Q, the sum of squared sample luminance       (may be NULL)
 *    final_states  u32               the stream's state after sample n            (may be NULL)
 * Pixels outside the rect are left untouched in every plane.  A caller rebuilds the error estimate from the planes as described
 * for ort_radiance_adaptive; the known weakness is the same: a pixel that has seen no light in its first min_spp samples stops
 * black.
 * Two identities.  (1) With min_spp == max_spp == n no check runs and out_rgb is ort_render_image's at ORT_POLICY_PIXEL and
 * spp = n, bit for bit.  (2) With a tolerance so large that thr*thr is +inf, every pixel with finite Q stops at min_spp with that
 * call's bits at spp = min_spp.
 * Parameters.  params->policy must be ORT_POLICY_PIXEL; any other policy is ORT_ERR_UNSUPPORTED.  params->spp and params->chunk
 * are ignored: ad->max_spp takes the place of spp before the parameter checks the render call shares.  shard_count > 1 and
 * ORT_RENDER_PACKED return ORT_ERR_UNSUPPORTED.  ad is judged exactly as ort_radiance_adaptive judges it, rr as the render call
 * judges it (rr >= 0).
 * The views form follows ort_render_views: params->seed is ignored; the per-view seed and camera, the rule where a camera may
 * stand, ORT_MAX_VIEWS and view_count == 0 (ORT_OK without a launch, whatever the other arguments) are as there; the planes hold
 * view_count frames, view-major.  Frame v is, bit for bit and in every plane, what the single-frame call gives with params->seed
 * = views[v].seed on a scene whose camera basis is views[v].camera.  The single-frame call is the one-view batch of the scene's own
 * camera (ort_scene_get_camera) and params->seed.
 * Errors are reported before any device work, in ort_render_views' order with the ad checks directly after the params checks:
 * ORT_ERR_INVALID (null out_rgb or views, view cap exceeded, null scene or params, empty or bad params exactly as
 * ort_render_image judges them with max_spp for spp; then ad == NULL, min_spp < 2, max_spp < min_spp, max_spp > 1 << 24,
 * check_every == 0, tolerance or floor NaN, infinite or negative), ORT_ERR_UNSUPPORTED (policy, shard, packed, camera outside the
 * box), ORT_ERR_STATE (scene not committed), ORT_ERR_NO_DEVICE (not uploaded).
 * The device forms take DEVICE pointers on the scene's device, enqueue on hip_stream (NULL = the default stream) and wait only
 * when stats != NULL; views is a HOST array in both forms, copied before the call returns.  stats as for the render call; with
 * ORT_RENDER_COUNTERS, paths is the number of samples taken: the sum of out_spp over the rect of every frame.  No workspace is
 * needed: PIXEL jobs have no partial planes. */

/* host planes in, host planes out (device staging is internal); synchronous */
int ort_render_adaptive(ort_scene *scene, const ort_render_params *params, const ort_adaptive *ad, float *out_rgb,
                        uint32_t *out_spp /* may be NULL */, float *out_m2 /* may be NULL */, uint32_t *final_states /* may be NULL */,
                        ort_stats *stats);
int ort_render_adaptive_device(ort_scene *scene, const ort_render_params *params, const ort_adaptive *ad, void *d_out_rgb,
                               void *d_out_spp, void *d_out_m2, void *d_final_states, void *hip_stream, ort_stats *stats);
/* view_count frames per plane, view-major */
int ort_render_views_adaptive(ort_scene *scene, const ort_render_params *params, const ort_adaptive *ad, const ort_view *views,
                              uint32_t view_count, float *out_rgb, uint32_t *out_spp /* may be NULL */, float *out_m2 /* may be NULL */,
                              uint32_t *final_states /* may be NULL */, ort_stats *stats);
int ort_render_views_adaptive_device(ort_scene *scene, const ort_render_params *params, const ort_adaptive *ad, const ort_view *views,
                                     uint32_t view_count, void *d_out_rgb, void *d_out_spp, void *d_out_m2, void *d_final_states,
                                     void *hip_stream, ort_stats *stats);

/* ---- light-group renders: one frame per group of lights, in one pass ------------------------------
 * The frame split by which light the energy came from, so that a compositor can re-tint, dim or switch off a light after the
 * render: G frames, and if asked for the unsplit frame, for about the price of one render instead of G renders of G scenes.
 * Job.  The job is the ORT_POLICY_PIXEL job of pixel (x, y): all spp camera samples on the stream job_seed(seed, y*W + x)
 * (views[v].seed in the views form).  The samples are ort_render_image's samples, unchanged, the aperture draw included.
 * Sums, every operation a separately rounded f32 operation:
 *  - C is the render's sum.  C_g, for g in [0, G), starts at (+0, +0, +0).
 *  - Whenever a sample adds a vector e to C -- a light was hit: at the primary hit unguarded (ray.cpp:1254-1259), at a bounce only
 *    if e is finite (ray.cpp:1358-1371) -- let m be the material that was hit and g = group_of_material[m].  If g < G then
 *    C_g = C_g + e, component by component: the same e under the same conditions.
 *  - Entries of materials that are not lights are never read and may hold any byte.  A light whose entry is ORT_NO_LIGHT_GROUP
 *    is in no group.
 * Outputs, each plane with row 0 at the bottom:
 *    out_groups    view_count x G frames of width*height*3 f32; frame (v, g) starts at ((v*G + g) * height*width*3) floats
 *                  and holds C_g / (float)spp
 *    out_rgb       view_count frames, view-major: C / (float)spp                        (may be NULL)
 *    final_states  width*height u32 per view: the stream's state after the job          (may be NULL)
 * Pixels outside the rect are left untouched in every plane.
 * Five identities.  (1) out_rgb and final_states are ort_render_image's ORT_POLICY_PIXEL frame and its jobs' final states, bit for
 * bit.  (2) Frame g is, bit for bit, ort_render_image's ORT_POLICY_PIXEL frame of the scene whose light materials outside group g
 * have emit = +0 (is_light untouched): that scene has the same geometry and tree, so every path takes the same turns and draws the
 * same numbers, and its dark lights add +-0, or a NaN that the bounce guard drops, to a sum that started at +0 -- which never
 * changes it.  (3) Frame g depends only on which materials are in group g: moving other lights between groups, another G, or NULL
 * for out_rgb or final_states changes no bit of it.  (4) Frame (v, .) of a batch is the single-frame call's for that camera and
 * seed; the single-frame call is the one-view batch of the scene's own camera (ort_scene_get_camera) and params->seed.  (5) The
 * frames of a partition of the lights add up to out_rgb only up to rounding, not bit for bit (f32 addition is not associative):
 * that is why the call offers out_rgb from the same pass.
 * Parameters.  params->policy must be ORT_POLICY_PIXEL; any other policy is ORT_ERR_UNSUPPORTED.  params->spp is within
 * [1, 1 << 24], so that (float)spp is exact.  shard_count > 1 and ORT_RENDER_PACKED return ORT_ERR_UNSUPPORTED.  params->chunk is
 * ignored; rr is judged as the render call judges it (rr >= 0).  The views form follows ort_render_views: params->seed is ignored;
 * the per-view seed and camera, the rule where a camera may stand, ORT_MAX_VIEWS and view_count == 0 (ORT_OK without a launch,
 * whatever the other arguments) are as there.
 * Errors are reported before any device work, in ort_render_views_adaptive's order with the groups where ad stands:
 * ORT_ERR_INVALID (null out_groups or views, view cap exceeded, null scene or params, empty or bad params exactly as
 * ort_render_image judges them; then spp above 1 << 24; then groups == NULL, a null table, material_count not the scene's,
 * group_count 0 or above ORT_MAX_LIGHT_GROUPS, a LIGHT material's entry that is neither < group_count nor ORT_NO_LIGHT_GROUP, a
 * plane not 4-byte aligned), ORT_ERR_UNSUPPORTED (policy, shard, packed, camera outside the box), ORT_ERR_STATE (scene not
 * committed), ORT_ERR_NO_DEVICE (not uploaded).
 * The device forms take DEVICE pointers for the planes on the scene's device, enqueue on hip_stream (NULL = the default stream)
 * and wait only when stats != NULL; views, the groups struct and its table are HOST memory in every form, copied before the call
 * returns.  stats as for the render call; with ORT_RENDER_COUNTERS, paths = view_count x rect pixels x spp.  No workspace is
 * needed: the group sums of a pixel live in its words of out_groups while its job runs. */
#define ORT_MAX_LIGHT_GROUPS 8u
#define ORT_NO_LIGHT_GROUP   0xffu
typedef struct {
    const uint8_t *group_of_material; /* HOST array in every form, copied before the call returns; material_count entries */
    uint32_t material_count;          /* must equal the scene's material_count (index 0 included) */
    uint32_t group_count;             /* G, 1 .. ORT_MAX_LIGHT_GROUPS */
} ort_light_groups;

/* host planes in, host planes out (device staging is internal); synchronous */
int ort_render_light_groups(ort_scene *scene, const ort_render_params *params, const ort_light_groups *groups, float *out_groups,
                            float *out_rgb /* may be NULL */, uint32_t *final_states /* may be NULL */, ort_stats *stats);
int ort_render_light_groups_device(ort_scene *scene, const ort_render_params *params, const ort_light_groups *groups,
                                   void *d_out_groups, void *d_out_rgb, void *d_final_states, void *hip_stream, ort_stats *stats);
/* view_count x G group frames, view_count frames per other plane, view-major */
int ort_render_views_light_groups(ort_scene *scene, const ort_render_params *params, const ort_light_groups *groups,
                                  const ort_view *views, uint32_t view_count, float *out_groups, float *out_rgb /* may be NULL */,
                                  uint32_t *final_states /* may be NULL */, ort_stats *stats);
int ort_render_views_light_groups_device(ort_scene *scene, const ort_render_params *params, const ort_light_groups *groups,
                                         const ort_view *views, uint32_t view_count, void *d_out_groups, void *d_out_rgb,
                                         void *d_final_states, void *hip_stream, ort_stats *stats);

/* ---- path-depth renders: emission, direct, indirect -- one frame per bounce count, in one pass ----
 * The frame split by how many bounces the light took: the "emission / direct / indirect" triple of compositors and denoisers,
 * and with more bins a per-bounce breakdown.  No depth cap exists to render it with, so G renders of G scenes cannot give it.
 * Job.  The job is the ORT_POLICY_PIXEL job of pixel (x, y): all spp camera samples on the stream job_seed(seed, y*W + x)
 * (views[v].seed in the views form).  The samples are ort_render_image's samples, unchanged, the aperture draw included.
 * Depth.  Every ray of a sample has a depth d: 0 for the camera ray, one more with each sample_brdf draw, that is each bounce ray
 * (ray.cpp:1335-1353).  A re-cast of the same ray on the exact octree walk is not a new depth.
 * Bins.  G = bin_count bins, 1 <= G <= ORT_MAX_DEPTH_BINS; the bin of a depth is min(d, G - 1).  With G = 3, bin 0
 * (ORT_DEPTH_EMISSION) is light sources seen directly, bin 1 (ORT_DEPTH_DIRECT) light that took one bounce, bin 2
 * (ORT_DEPTH_INDIRECT) everything beyond.
 * Sums, every operation a separately rounded f32 operation:
 *  - C is the render's sum.  B_g, for g in [0, G), starts at (+0, +0, +0).
 *  - Whenever a sample adds a vector e to C -- a light was hit: at the primary hit unguarded (ray.cpp:1254-1259), at a bounce only
 *    if e is finite (ray.cpp:1358-1371) -- on a ray of depth d, then B_bin(d) = B_bin(d) + e, component by component: the same e
 *    under the same conditions.
 * Lengths.  N_g, for g in [0, G), starts at 0.  When a sample ends, for any reason -- a light was hit, nothing was hit, a shape of
 * material 0 was hit, or the roulette said so -- with d the depth of the last ray it cast, N_bin(d) = N_bin(d) + 1.  The N_g of
 * a pixel add up to spp.
 * Outputs, each plane with row 0 at the bottom, plane-major as out_groups is:
 *    out_bins      view_count x G frames of width*height*3 f32; frame (v, g) starts at ((v*G + g) * height*width*3) floats
 *                  and holds B_g / (float)spp
 *    out_rgb       view_count frames, view-major: C / (float)spp                        (may be NULL)
 *    out_lengths   view_count x G planes of width*height u32; plane (v, g) starts at ((v*G + g) * height*width) words
 *                  and holds N_g                                                        (may be NULL)
 *    final_states  width*height u32 per view: the stream's state after the job          (may be NULL)
 * Pixels outside the rect are left untouched in every plane.
 * Six identities.  (1) out_rgb and final_states are ort_render_image's ORT_POLICY_PIXEL frame and its jobs' final states, bit for
 * bit.  (2) With G = 1, out_bins is out_rgb bit for bit and out_lengths is spp: the additions are the same, in the same order.
 * (3) For g < G - 1, frame g and length plane g do not depend on G; nor does any plane depend on which optional planes are NULL.
 * (4) With rr = 0 no path bounces: every bin but bin 0 is +0 and every length lies in bin 0.  (5) The bins add up to out_rgb only
 * up to rounding, not bit for bit (f32 addition is not associative): that is why the call offers out_rgb from the same pass.
 * (6) Frame (v, .) of a batch is the single-frame call's for that camera and seed; the single-frame call is the one-view batch of
 * the scene's own camera (ort_scene_get_camera) and params->seed.
 * Parameters.  params->policy must be ORT_POLICY_PIXEL; any other policy is ORT_ERR_UNSUPPORTED.  params->spp is within
 * [1, 1 << 24], so that (float)spp is exact.  shard_count > 1 and ORT_RENDER_PACKED return ORT_ERR_UNSUPPORTED.  params->chunk is
 * ignored; rr is judged as the render call judges it (rr >= 0).  The views form follows ort_render_views_light_groups:
 * params->seed is ignored; the per-view seed and camera, the rule where a camera may stand, ORT_MAX_VIEWS and view_count == 0
 * (ORT_OK without a launch, whatever the other arguments) are as there.
 * Errors are reported before any device work, in ort_render_light_groups' order with the bin count where the groups stand:
 * ORT_ERR_INVALID (null out_bins or views, view cap exceeded, null scene or params, empty or bad params exactly as
 * ort_render_image judges them; then spp above 1 << 24; then bin_count 0 or above ORT_MAX_DEPTH_BINS; then a plane not 4-byte
 * aligned), ORT_ERR_UNSUPPORTED (policy, shard, packed, camera outside the box), ORT_ERR_STATE (scene not committed),
 * ORT_ERR_NO_DEVICE (not uploaded).
 * The device forms take DEVICE pointers for the planes on the scene's device, enqueue on hip_stream (NULL = the default stream)
 * and wait only when stats != NULL; views is HOST memory in every form, copied before the call returns.  stats as for the render
 * call; with ORT_RENDER_COUNTERS, paths = view_count x rect pixels x spp.  No workspace is needed: the bin sums and the length
 * counts of a pixel live in its words of out_bins and out_lengths while its job runs. */
#define ORT_MAX_DEPTH_BINS 8u
#define ORT_DEPTH_EMISSION 0u
#define ORT_DEPTH_DIRECT   1u
#define ORT_DEPTH_INDIRECT 2u

/* host planes in, host planes out (device staging is internal); synchronous */
int ort_render_depths(ort_scene *scene, const ort_render_params *params, uint32_t bin_count, float *out_bins,
                      float *out_rgb /* may be NULL */, uint32_t *out_lengths /* may be NULL */, uint32_t *final_states /* may be NULL */,
                      ort_stats *stats);
int ort_render_depths_device(ort_scene *scene, const ort_render_params *params, uint32_t bin_count, void *d_out_bins, void *d_out_rgb,
                             void *d_out_lengths, void *d_final_states, void *hip_stream, ort_stats *stats);
/* view_count x G bin frames and length planes, view_count frames per other plane, view-major */
int ort_render_views_depths(ort_scene *scene, const ort_render_params *params, uint32_t bin_count, const ort_view *views,
                            uint32_t view_count, float *out_bins, float *out_rgb /* may be NULL */, uint32_t *out_lengths /* may be NULL */,
                            uint32_t *final_states /* may be NULL */, ort_stats *stats);
int ort_render_views_depths_device(ort_scene *scene, const ort_render_params *params, uint32_t bin_count, const ort_view *views,
                                   uint32_t view_count, void *d_out_bins, void *d_out_rgb, void *d_out_lengths, void *d_final_states,
                                   void *hip_stream, ort_stats *stats);

/* ---- sample-map renders: the caller's sample count per pixel -------------------------------------
 * The camera render with a job length of the caller's choosing for every pixel: the second pass of a two-pass scheme (a pilot
 * frame, a map built from its out_m2 and guide planes, the samples spent where the map says), a foveated frame, or -- a map that
 * is zero outside a pixel set -- the sparse camera render of just that set, aperture draw included.
 * The map.  sample_map holds view_count frames of width*height u32, view-major, row 0 at the bottom: the layout of
 * ort_render_adaptive's out_spp, which can be fed back as it stands.  HOST memory in the host forms, a DEVICE pointer on the
 * scene's device in the _device forms (a map built on the GPU never visits the host).  It must be 4-byte aligned and must not
 * overlap an output plane (not checked).  It is read, never written.
 * Job.  The job is the ORT_POLICY_PIXEL job of pixel (x, y): camera samples, the aperture draw included, on the stream
 * job_seed(seed, y*W + x) (views[v].seed in the views form), cut after n = min(sample_map[i], params->spp) samples.  params->spp
 * is the cap and lies within [1, 1 << 24], so that (float)n is exact.  The map's values are never judged: a value above the cap
 * is clamped, 0xffffffff included, identically in all four forms (the device forms cannot see the values before the launch).
 * n == 0: the pixel is not rendered -- its stream is never started and its words in every output plane stay untouched, exactly as
 * the pixels outside the rect.  An all-zero map returns ORT_OK after a launch that writes nothing.
 * Outputs for n >= 1, each plane view_count frames, view-major, row 0 at the bottom:
 *    out_rgb       C / (float)n, component by component, C the render's sum of the n samples
 *    out_m2        Q, the sum of squared sample luminance, accumulated operation by operation as ort_radiance_adaptive
 *                  defines it                                                             (may be NULL)
 *    final_states  the stream's state after sample n                                      (may be NULL)
 * Which optional planes are asked for changes no bit of the others.
 * Four identities, all bit for bit.  (1) A constant map n, or any map at or above a cap n, gives ort_render_image's
 * ORT_POLICY_PIXEL frame at spp = n, and ort_render_adaptive's planes at min_spp == max_spp == n.  (2) The planes of pixel i
 * depend only on n_i, the seed and the camera, not on the rest of the map.  (3) ort_render_adaptive's out_spp as the map, the same
 * seed and a cap >= max_spp give that call's out_rgb, out_m2 and final_states.  (4) Frame v of a batch is the single-frame call's
 * for that camera, seed and map frame; the single-frame call is the one-view batch of the scene's own camera
 * (ort_scene_get_camera) and params->seed.
 * This call starts every pixel's stream anew; a pixel's stream and sums are resumed from an earlier call through
 * ort_render_accumulate (below), which takes the same map.  Passes taken with DIFFERENT seeds are independent
 * estimates and combine weighted by their counts: rgb = (n1 * rgb1 + n2 * rgb2) / (n1 + n2) where n1 + n2 > 0.
 * Parameters.  params->policy must be ORT_POLICY_PIXEL; any other policy is ORT_ERR_UNSUPPORTED.  shard_count > 1 and
 * ORT_RENDER_PACKED return ORT_ERR_UNSUPPORTED.  params->chunk is ignored; rr is judged as the render call judges it (rr >= 0).
 * The views form follows ort_render_views: params->seed is ignored; the per-view seed and camera, the rule where a camera may
 * stand, ORT_MAX_VIEWS and view_count == 0 (ORT_OK without a launch, whatever the other arguments) are as there.
 * Errors are reported before any device work, in ort_render_light_groups' order with the map where the groups stand:
 * ORT_ERR_INVALID (null out_rgb or views, view cap exceeded, null scene or params, empty or bad params exactly as
 * ort_render_image judges them; then spp above 1 << 24; then a null sample_map, a map or plane not 4-byte aligned),
 * ORT_ERR_UNSUPPORTED (policy, shard, packed, camera outside the box), ORT_ERR_STATE (scene not committed), ORT_ERR_NO_DEVICE
 * (not uploaded).
 * The device forms take DEVICE pointers for the map and the planes, enqueue on hip_stream (NULL = the default stream) and wait
 * only when stats != NULL; views is HOST memory in every form, copied before the call returns.  stats as for the render call; with
 * ORT_RENDER_COUNTERS, paths = the sum of n over the rect of every frame.  No workspace is needed. */
/* host map and planes (device staging is internal); synchronous */
int ort_render_sample_map(ort_scene *scene, const ort_render_params *params, const uint32_t *sample_map, float *out_rgb,
                          float *out_m2 /* may be NULL */, uint32_t *final_states /* may be NULL */, ort_stats *stats);
int ort_render_sample_map_device(ort_scene *scene, const ort_render_params *params, const void *d_sample_map, void *d_out_rgb,
                                 void *d_out_m2, void *d_final_states, void *hip_stream, ort_stats *stats);
/* view_count frames of the map and of every plane, view-major */
int ort_render_views_sample_map(ort_scene *scene, const ort_render_params *params, const ort_view *views, uint32_t view_count,
                                const uint32_t *sample_map, float *out_rgb, float *out_m2 /* may be NULL */,
                                uint32_t *final_states /* may be NULL */, ort_stats *stats);
int ort_render_views_sample_map_device(ort_scene *scene, const ort_render_params *params, const ort_view *views, uint32_t view_count,
                                       const void *d_sample_map, void *d_out_rgb, void *d_out_m2, void *d_final_states,
                                       void *hip_stream, ort_stats *stats);

/* ---- accumulating renders: a frame's samples continued across calls ------------------------------
 * The sample-map render on planes that carry a pixel's state from call to call: render 64 samples, look, continue to 1024; render
 * until a time budget runs out; checkpoint the planes and pick the frame up after a restart; refine the pixels of a pilot pass
 * instead of blending an independent estimate.  After any split of a pixel's samples over calls the planes hold the bits of the
 * single call.
 * The planes (ort_accum_planes) belong to the caller and are read AND written; each holds view_count frames of width*height
 * entries, view-major, row 0 at the bottom -- the layout of ort_render_adaptive's planes:
 *    sum_rgb   3 f32 per pixel   C, the UNDIVIDED colour sum.  (out_rgb * n is not C: the division rounds once, which is why
 *                                a mean cannot serve as state)
 *    m2        f32               Q, the sum of squared sample luminance, as ort_radiance_adaptive defines it   (may be NULL)
 *    count     u32               n, the samples this pixel has had so far
 *    states    u32               the stream's state after sample n
 * HOST pointers in the host forms, DEVICE pointers on the scene's device in the _device forms; the struct itself is host memory in
 * every form and is read before the call returns.  Every given plane and the map must be 4-byte aligned.  Planes and the map must
 * not overlap one another (not checked).  A caller starts a frame by setting count to zero and nothing else.
 * sample_map (may be NULL) is ort_render_sample_map's map, read and never written; out_rgb (may be NULL) is a frame of
 * view_count * width * height * 3 f32, written and never read.
 * Contract for pixel i inside the rect, operation by operation:
 *    n0    = count[i]
 *    asked = sample_map ? sample_map[i] : params->spp
 *    add   = min(asked, params->spp, (1 << 24) - min(n0, 1 << 24))
 * params->spp is the cap on what ONE call adds and lies within [1, 1 << 24]; the total never passes 1 << 24, so (float)n stays
 * exact.  Neither the map's nor the planes' values are ever judged, identically in all four forms.
 * add == 0: no word of any plane is read (count[i] and the map word apart) or written for this pixel and its stream is not touched
 * -- exactly the sample-map render's empty job and the pixels outside the rect.
 * n0 == 0, a fresh pixel: the stream starts at job_seed(seed, y*W + x) (views[v].seed in the views form), C = (+0, +0, +0),
 * Q = +0; sum_rgb[i], m2[i] and states[i] are NOT read, whatever they hold.
 * n0 > 0, a continued pixel: the stream starts at states[i], WITH 0 TAKEN AS 1 (a zero xorshift state never leaves zero, the
 * roulette would then never end a path in a closed room: the rule is the contract's, not the caller's duty); C = sum_rgb[i] and,
 * if m2 is given, Q = m2[i] (Q = +0 otherwise) -- used as they stand, NaN and infinities included, as a hostile material is.  A
 * sample that reaches no light adds the colour +0, so a stored -0 is +0 afterwards: the sums start as stored + (+0).
 * Then add camera samples run, the aperture draw included: ort_render_image's ORT_POLICY_PIXEL samples, unchanged, each adding
 * at most one vector to C component by component and its squared luminance to Q.  Written afterwards:
 *    sum_rgb[i] = C;  m2[i] = Q if m2 is given;  count[i] = n0 + add;  states[i] = the stream's state;
 *    out_rgb[i] = C / (float)(n0 + add), component by component, if out_rgb is given.
 * out_rgb is written only for pixels that took samples in THIS call; every other pixel keeps what it held.
 * Five identities, all bit for bit.  (1) From count == 0 one call gives in out_rgb, m2 and states what ort_render_sample_map
 * gives for the same map and cap, and count equals that call's n; with a constant add = n that is ort_render_image's
 * ORT_POLICY_PIXEL frame at spp = n and ort_render_adaptive's planes at min_spp == max_spp == n.  (2) Split invariance: for any
 * split of a pixel's samples over any number of calls -- other maps, caps and rects per call, other pixels doing anything -- the
 * four planes after the last call depend only on the pixel's total n, the seed and the camera, so sum_rgb / (float)count is the
 * single call's pixel.  (3) From the caller's own planes the call is add chained spp = 1 renders from that state: C receives each
 * one's colour in order, starting from the given C.  (4) Whether m2 or out_rgb is NULL changes no bit of the other planes.
 * (5) Frame v of a batch is the single-frame call's for that camera and seed; the single-frame call is the one-view batch of the
 * scene's own camera (ort_scene_get_camera) and params->seed.
 * Parameters.  params->policy must be ORT_POLICY_PIXEL; any other policy, shard_count > 1 and ORT_RENDER_PACKED return
 * ORT_ERR_UNSUPPORTED.  params->chunk is ignored; rr is judged as the render call judges it.  The views form follows
 * ort_render_views: params->seed is ignored, and view_count == 0 is ORT_OK without a launch, whatever the other arguments.
 * Errors are reported before any device work, in ort_render_sample_map's order with acc where the map stands: ORT_ERR_INVALID
 * (null views, view cap exceeded, null scene or params, empty or bad params exactly as ort_render_image judges them; then spp
 * above 1 << 24; then a null acc, acc->sum_rgb, acc->count or acc->states; then a given plane or map not 4-byte aligned),
 * ORT_ERR_UNSUPPORTED (policy, shard, packed, camera outside the box), ORT_ERR_STATE (scene not committed), ORT_ERR_NO_DEVICE
 * (not uploaded).
 * The device forms enqueue on hip_stream (NULL = the default stream) and wait for the launch only when stats != NULL.  Successive
 * calls on one stream therefore chain passes on planes that never leave the device: no plane visits the host between them, and
 * the order of the stream is the order of the passes.  (As every call on a scene, a call first waits until the scene's previous
 * launch has finished: a scene runs one launch at a time.)  views is HOST memory in every form, copied before the call returns.
 * stats as for the render call; with ORT_RENDER_COUNTERS, paths = the sum of add over the rect of every frame.  No workspace is
 * needed. */
typedef struct {
    float    *sum_rgb;  /* 3 f32 per pixel: C, the undivided colour sum        in and out */
    float    *m2;       /* f32: Q, the sum of squared sample luminance         in and out, may be NULL */
    uint32_t *count;    /* u32: n, the samples this pixel has had so far       in and out */
    uint32_t *states;   /* u32: the stream's state after sample n              in and out */
} ort_accum_planes;     /* HOST pointers in the host forms, DEVICE pointers in the _device forms; the struct itself is host memory */
/* host planes, map and frame (device staging is internal); synchronous */
int ort_render_accumulate(ort_scene *scene, const ort_render_params *params, const ort_accum_planes *acc,
                          const uint32_t *sample_map /* may be NULL */, float *out_rgb /* may be NULL */, ort_stats *stats);
int ort_render_accumulate_device(ort_scene *scene, const ort_render_params *params, const ort_accum_planes *acc,
                                 const void *d_sample_map, void *d_out_rgb, void *hip_stream, ort_stats *stats);
/* view_count frames of every plane, of the map and of out_rgb, view-major */
int ort_render_views_accumulate(ort_scene *scene, const ort_render_params *params, const ort_view *views, uint32_t view_count,
                                const ort_accum_planes *acc, const uint32_t *sample_map /* may be NULL */,
                                float *out_rgb /* may be NULL */, ort_stats *stats);
int ort_render_views_accumulate_device(ort_scene *scene, const ort_render_params *params, const ort_view *views, uint32_t view_count,
                                       const ort_accum_planes *acc, const void *d_sample_map, void *d_out_rgb, void *hip_stream,
                                       ort_stats *stats);

/* ---- first-hit feature renders: albedo, normal, depth, coverage and id planes of the camera -----
 * The noise-free guide planes a denoiser wants next to the colour: what the camera's own samples see FIRST.  A pass of its own on
 * the pixel's own stream, a raycast per sample instead of a path; through the aperture the planes have the distribution of the
 * render's samples.
 * Planes.  Each holds width*height entries per frame with row 0 at the bottom, view_count frames view-major:
 *    albedo        3 f32 per pixel   mean over spp of the first hit's albedo           (may be NULL)
 *    normal        3 f32 per pixel   mean over spp of the first hit's unit normal      (may be NULL)
 *    depth         f32               mean over spp of the first hit's distance         (may be NULL)
 *    hits          u32               samples that hit a surface; coverage = hits/spp   (may be NULL)
 *    ids           2 u32: mat, prim  of sample 0                                       (may be NULL)
 *    final_states  u32               the stream's state after the last sample          (may be NULL)
 * Pixels outside the rect are left untouched in every plane.
 * The job.  A job is pixel (x, y) of a frame; its stream starts at job_seed(seed, y*W + x), the ORT_POLICY_PIXEL stream of that
 * pixel (views[v].seed in the views form).  Sample k = 0 .. spp-1, every operation a separately rounded f32 operation (no FMA):
 *  - rad = random_between(s, 0, 2 pi): TWO steps of the stream (random.h:47-53);
 *  - ap, the aperture point of ray.cpp:1233-1234, and d = normalize(focal - ap) of ray.cpp:1237 with focal of ray.cpp:1198 and
 *    :1215-1221 for that pixel and camera: the render's own expressions in the render's own order;
 *  - h, the closest hit of the ray (ap, d), exactly the record ort_raycast returns for it: t, the normalised n, mat, prim.  Whatever
 *    ray comes out gets that query's answer, exact-walk rays included.
 * Nothing else is drawn: the stream advances exactly 2*spp steps whatever is hit, so final_states does not depend on the scene.
 * Sums.  A, N and D start at +0.  For every sample with h.mat != 0, in sample order: hits++, A += albedo(h.mat), N += h.n,
 * D += h.t, each component a separately rounded f32 add.  albedo(m) is materials[m].emit if is_light, else materials[m].diffuse,
 * as it stands: a mirror or glass surface has its (often zero) diffuse colour.
 * Outputs.  albedo = A / (float)spp, normal = N / (float)spp, depth = D / (float)spp, component by component (ray.cpp:1428's
 * division).  hits is the count; a caller who wants the mean over hits divides by coverage.  normal is not re-normalised.  ids =
 * {h.mat, h.prim} of sample 0; a miss gives 0, ORT_NO_PRIM; ids do not average.  A sample whose closest hit is on a shape that
 * carries material 0 (see ort_raycast) does not count in hits and adds nothing to A, N or D; as sample 0 it gives ids = {0, the
 * shape's prim}.  d is a unit vector, so depth is a distance from the aperture point.
 * Parameters.  params->policy must be ORT_POLICY_PIXEL; any other policy is ORT_ERR_UNSUPPORTED.  params->spp is within
 * [1, 1 << 24], so that (float)spp is exact.  params->chunk and params->rr are ignored.  shard_count > 1 and ORT_RENDER_PACKED
 * return ORT_ERR_UNSUPPORTED.
 * The views form follows ort_render_views: params->seed is ignored; the per-view seed and camera, the rule where a camera may
 * stand, ORT_MAX_VIEWS and view_count == 0 (ORT_OK without a launch, whatever the other arguments) are as there.  The single-frame
 * call is the one-view batch of the scene's own camera (ort_scene_get_camera) and params->seed.
 * Four identities.  (1) At spp = 1, depth, normal and ids are ort_raycast's t, n, mat, prim for the pixel's first camera ray.
 * (2) That ray is the first primary ray of the ORT_POLICY_PIXEL render: with rr = 0 and spp = 1, ort_render_image's pixel is emit
 * of ids.mat if that material is a light, and 0 otherwise.  (3) Frame v of a batch is, in every plane, the single-frame call's
 * frame for that camera and seed.  (4) Which planes are asked for changes no bit of the others.
 * Errors are reported before any device work, in ort_render_views_adaptive's order with the planes where ad stands:
 * ORT_ERR_INVALID (null planes struct, all of the five feature planes NULL, null views, view cap exceeded, null scene or params,
 * empty or bad params exactly as ort_render_image judges them; then spp above 1 << 24, a plane not 4-byte aligned),
 * ORT_ERR_UNSUPPORTED (policy, shard, packed, camera outside the box), ORT_ERR_STATE (scene not committed), ORT_ERR_NO_DEVICE (not
 * uploaded).
 * The device forms take DEVICE pointers on the scene's device, enqueue on hip_stream (NULL = the default stream) and wait only
 * when stats != NULL; views and the planes struct are HOST memory in both forms, read before the call returns.  stats follow the
 * ray queries: with ORT_RENDER_COUNTERS, rays = frames x rect pixels x spp and paths = 0; fallback_rays and kernel_ms are always
 * filled. */
typedef struct {
    float    *albedo;        /* 3 f32 per pixel   may be NULL */
    float    *normal;        /* 3 f32 per pixel   may be NULL */
    float    *depth;         /* f32               may be NULL */
    uint32_t *hits;          /* u32               may be NULL */
    uint32_t *ids;           /* 2 u32: mat, prim  may be NULL */
    uint32_t *final_states;  /* u32               may be NULL */
} ort_feature_planes;        /* HOST pointers in the host forms, DEVICE pointers in the _device forms */

/* host planes in, host planes out (device staging is internal); synchronous */
int ort_render_features(ort_scene *scene, const ort_render_params *params, const ort_feature_planes *planes, ort_stats *stats);
int ort_render_features_device(ort_scene *scene, const ort_render_params *params, const ort_feature_planes *planes, void *hip_stream,
                               ort_stats *stats);
/* view_count frames per plane, view-major */
int ort_render_views_features(ort_scene *scene, const ort_render_params *params, const ort_view *views, uint32_t view_count,
                              const ort_feature_planes *planes, ort_stats *stats);
int ort_render_views_features_device(ort_scene *scene, const ort_render_params *params, const ort_view *views, uint32_t view_count,
                                     const ort_feature_planes *planes, void *hip_stream, ort_stats *stats);

/* ---- feature renders that follow mirrors and glass: the planes of the first non-specular vertex -----
 * ort_render_features stops at the first hit: what is seen in a mirror or through glass gets the guides of the mirror or the glass
 * itself.  These calls follow the path the renderer itself would take through specular-only surfaces and record albedo, normal,
 * distance and ids where the path first meets a light or a surface with a diffuse part.  The contract is the reference's sample
 * body (ray.cpp:1247-1426) cut at that vertex.
 * Planes.  Each holds width*height entries per frame with row 0 at the bottom, view_count frames view-major:
 *    albedo        3 f32 per pixel   mean over spp of the recorded vertex's albedo                                  (may be NULL)
 *    normal        3 f32 per pixel   mean over spp of the recorded vertex's unit normal, as it stands: not mirrored
 *                                    back into the first surface's frame, not re-normalised                         (may be NULL)
 *    depth         f32               mean over spp of the path length from the aperture point to the recorded vertex (may be NULL)
 *    hits          u32               samples that recorded a vertex                                                 (may be NULL)
 *    ids           2 u32: mat, prim  of sample 0's last vertex                                                      (may be NULL)
 *    bounces       u32               sum over the recorded samples of the bounces followed                          (may be NULL)
 *    final_states  u32               the stream's state after the last sample                                       (may be NULL)
 * At least one of the first six must be given.  Pixels outside the rect are left untouched in every plane.
 * The job.  A job is pixel (x, y) of a frame; its stream s starts at job_seed(seed, y*W + x), the ORT_POLICY_PIXEL stream of that
 * pixel (views[v].seed in the views form).  Sample k = 0 .. spp-1, every operation a separately rounded f32 operation (no FMA):
 *  1. The camera sample: exactly ort_render_features' sample -- rad (two steps of the stream), ap, d = normalize(focal - ap).
 *     Then o = ap, dir = d, wo = -normalize(d) (ray.cpp:1241, sic), L = +0, b = 0.
 *  2. The vertex: h, the closest hit of the ray (o, dir), the record ort_raycast returns for it: t, the normalised n, mat, prim.  A
 *     primary ray that ort_raycast would send to the exact walk takes it here too; bounce rays start at hits and are traced as
 *     the render traces its bounce rays.
 *      - h.mat == 0 (a miss, or a shape that carries material 0): the sample ends without a record; as sample 0 it gives
 *        ids = {0, h.prim}, h.prim being ORT_NO_PRIM for a miss.
 *      - Otherwise L = L + h.t.  With m = materials[h.mat], the vertex is TERMINAL iff m.is_light, or |m.diffuse|^2 > 0 -- the f32
 *        x*x + y*y + z*z of ray.cpp:1267, the render's own test, so false for a NaN --, or b == max_bounces.
 *      - Terminal: hits++, A += albedo(m) (emit of a light, diffuse otherwise, as it stands), N += h.n, D += L, B += b, each
 *        component a separately rounded f32 add; as sample 0 it gives ids = {h.mat, h.prim}.  The sample ends.
 *  3. The bounce: otherwise exactly what the render does at a live non-light vertex:
 *      - o = o + (h.t - 1e-4f) * dir (ray.cpp:1262 / :1411);
 *      - the roulette: u = rng_01(s); if !(u < rr) the sample ends without a record, and as sample 0 it gives ids = {0, ORT_NO_PRIM};
 *      - sample_random_lights' burn (ray.cpp:537-601): one step, the light of index state % light_count, and four more steps if that
 *        light is a sphere; with no lights the one step;
 *      - wi = sample_brdf(s, h.n, wo, 0.01, Kd, Ks, Kt, ior, &is_trans): three draws, ray.cpp:1100-1161;
 *      - if is_trans, o = o + (2.0f * 1e-4f) * dir, dir still being the arriving direction (ray.cpp:1345-1348);
 *      - then dir = wi, wo = -wi, b++, and back to step 2.
 * No pdf, BSDF value or path weight is evaluated, and none of them advances the stream.
 * Outputs.  albedo = A / (float)spp, normal = N / (float)spp, depth = D / (float)spp, component by component (ray.cpp:1428's
 * division); hits; bounces = B; final_states; ids as given above.  A mean over the RECORDED samples is the plane times spp / hits.
 * Parameters.  params->policy must be ORT_POLICY_PIXEL.  params->spp is within [1, 1 << 24].  params->chunk is ignored.  params->rr
 * is used, and is judged as the render call judges it.  max_bounces is within [0, ORT_MAX_FOLLOW_BOUNCES]; the cap bounds every path,
 * so any rr the render call accepts is safe here.  shard_count > 1 and ORT_RENDER_PACKED return ORT_ERR_UNSUPPORTED.  The views form,
 * the rule where a camera may stand, ORT_MAX_VIEWS and view_count == 0 are as in ort_render_views_features; the single-frame call is
 * the one-view batch of the scene's own camera and params->seed.
 * Six identities, all bit for bit.  (1) max_bounces == 0 gives ort_render_features' six planes for any scene and rr; bounces is all
 * zero.  (2) A scene in which every non-light material has |Kd|^2 > 0 gives those planes for every max_bounces and rr.  (3) Take the
 * diffuse twin of the scene: every non-light material with |Kd|^2 > 0 made a light, everything else untouched.  While no sample
 * reaches the cap, final_states equals the final states of the twin's ort_render_image ORT_POLICY_PIXEL jobs at the same seed, spp
 * and rr.  (4) Frame v of a batch is, in every plane, the single-frame call's frame for that camera and seed.  (5) Which planes are
 * asked for changes no bit of the others.  (6) The recorded vertex of sample 0 at spp 1 is ort_raycast's record for the last ray of
 * the chain.
 * Errors are reported before any device work, in ort_render_views_features' order: ORT_ERR_INVALID (null planes struct, all of the
 * first six planes NULL, null views, view cap exceeded, null scene or params, empty or bad params exactly as ort_render_image judges
 * them, rr included; then spp above 1 << 24, max_bounces above ORT_MAX_FOLLOW_BOUNCES, a plane not 4-byte aligned),
 * ORT_ERR_UNSUPPORTED (policy, shard, packed, camera outside the box), ORT_ERR_STATE (scene not committed), ORT_ERR_NO_DEVICE (not
 * uploaded).
 * The device forms are as ort_render_features_device's.  stats follow the ray queries: with ORT_RENDER_COUNTERS, rays is every ray
 * cast (camera rays plus bounce rays) and paths = 0; fallback_rays and kernel_ms are always filled. */
#define ORT_MAX_FOLLOW_BOUNCES 64u
typedef struct {
    float    *albedo;        /* 3 f32 per pixel   may be NULL */
    float    *normal;        /* 3 f32 per pixel   may be NULL */
    float    *depth;         /* f32               may be NULL */
    uint32_t *hits;          /* u32               may be NULL */
    uint32_t *ids;           /* 2 u32: mat, prim  may be NULL */
    uint32_t *bounces;       /* u32               may be NULL */
    uint32_t *final_states;  /* u32               may be NULL */
} ort_follow_planes;         /* HOST pointers in the host forms, DEVICE pointers in the _device forms; the struct itself is host memory */

/* host planes in, host planes out (device staging is internal); synchronous */
int ort_render_follow(ort_scene *scene, const ort_render_params *params, uint32_t max_bounces, const ort_follow_planes *planes, ort_stats *stats);
int ort_render_follow_device(ort_scene *scene, const ort_render_params *params, uint32_t max_bounces, const ort_follow_planes *planes,
                             void *hip_stream, ort_stats *stats);
/* view_count frames per plane, view-major */
int ort_render_views_follow(ort_scene *scene, const ort_render_params *params, const ort_view *views, uint32_t view_count,
                            uint32_t max_bounces, const ort_follow_planes *planes, ort_stats *stats);
int ort_render_views_follow_device(ort_scene *scene, const ort_render_params *params, const ort_view *views, uint32_t view_count,
                                   uint32_t max_bounces, const ort_follow_planes *planes, void *hip_stream, ort_stats *stats);

/* ---- ID-matte renders: per-pixel coverage per material, object or shape, for compositing -----
 * ort_render_features' ids are those of sample 0 and do not average: through the aperture a pixel at a silhouette, or any pixel off
 * the focal plane, sees several shapes.  These calls count, per pixel, how many of the camera's samples saw which id: an
 * anti-aliased matte per material, object or shape is counts / spp (ort_matte_mask below).
 * Planes.  width*height entries per frame with row 0 at the bottom, view_count frames view-major; K = m->slots:
 *    ids           K u32 per pixel   [frame][pixel][slot]: the ids kept, ORT_MATTE_EMPTY in an unused slot      (REQUIRED)
 *    counts        K u32 per pixel   [frame][pixel][slot]: the samples that saw ids' id, 0 in an unused slot     (REQUIRED)
 *    other         u32               recorded samples that found no slot                                        (may be NULL)
 *    hits          u32               recorded samples                                                           (may be NULL)
 *    final_states  u32               the stream's state after the last sample                                   (may be NULL)
 * Pixels outside the rect are left untouched in every plane.
 * The job.  The job, its stream, the camera sample and the closest hit h are ort_render_features', word for word.  The stream
 * advances 2*spp steps whatever is hit.
 * The id of a sample.  h.mat == 0 (a miss, or a shape that carries material 0) records nothing: this is the rule by which such a
 * sample "does not count in hits".  Otherwise the sample is recorded with the id
 *    ORT_MATTE_BY_MATERIAL  h.mat;
 *    ORT_MATTE_BY_PRIM      h.prim as ort_raycast returns it;
 *    ORT_MATTE_BY_OBJECT    h.prim for a box, cylinder or sphere; for a triangle ORT_HIT_MESH << 28 | mesh index, the index being the
 *                           position in the scene's mesh order, as ort_scene_get_mesh takes it.
 * The slots.  K slots start empty, with used = 0 and other = 0.  For every recorded sample, in sample order, with id x: if a used
 * slot holds x, its count goes up by one; else if used < K, slot `used` becomes (x, 1) and used++; else other++.  At the job's end
 * the used slots are ordered by count descending, with ties broken by ascending id (unsigned compare), and written to
 * ids[at*K + j] and counts[at*K + j], at being the pixel's index in its plane; unused slots get (ORT_MATTE_EMPTY, 0).  hits is the
 * number of recorded samples.
 * Lossy slots.  While other == 0 the slots are the pixel's exact histogram.  Where other > 0 the kept ids are the first K to
 * appear, not the K largest.  A lane cannot know the largest without holding them all.  The caller sees which pixels are affected
 * and renders again with a larger K.
 * Six identities, all bit for bit.  (1) sum(counts) + other == hits, and hits and final_states are ort_render_features' planes.
 * (2) At spp == 1, ids[at*K] is ort_render_features' ids.mat (BY_MATERIAL) or ids.prim (BY_PRIM) where it hit, and ORT_MATTE_EMPTY
 * where it did not.  (3) Where other == 0 under both modes, the BY_OBJECT counts folded through "object -> its material" are the
 * BY_MATERIAL counts.  (4) Frame v of a batch is the single-frame call's frame.  (5) other, hits and final_states being asked for
 * or not changes no bit elsewhere.  (6) Pixels outside the rect are untouched in every plane.
 * Parameters, the error order, stats and the device-form rules are ort_render_views_features'.  Added to its ORT_ERR_INVALID
 * list, after "a plane not 4-byte aligned" and in this order: m NULL; by above 2; slots 0 or above ORT_MAX_MATTE_SLOTS; ids or
 * counts NULL.  (A NULL planes struct stands where ort_render_views_features has it; no "all planes NULL" error exists here.)
 * During a call the words of ids and counts inside the rect are working memory: their contents before the call are not read. */
#define ORT_MATTE_BY_MATERIAL 0u
#define ORT_MATTE_BY_OBJECT 1u
#define ORT_MATTE_BY_PRIM 2u
#define ORT_MAX_MATTE_SLOTS 8u
#define ORT_MATTE_EMPTY 0xffffffffu
#define ORT_HIT_MESH 1   /* kind of an object id that names a mesh; ort_raycast never returns it */
typedef struct {
    uint32_t by;     /* ORT_MATTE_BY_MATERIAL, ORT_MATTE_BY_OBJECT or ORT_MATTE_BY_PRIM */
    uint32_t slots;  /* K, within [1, ORT_MAX_MATTE_SLOTS] */
} ort_matte;
typedef struct {
    uint32_t *ids;           /* K u32 per pixel   required */
    uint32_t *counts;        /* K u32 per pixel   required */
    uint32_t *other;         /* u32               may be NULL */
    uint32_t *hits;          /* u32               may be NULL */
    uint32_t *final_states;  /* u32               may be NULL */
} ort_matte_planes;          /* HOST pointers in the host forms, DEVICE pointers in the _device forms; the struct itself is host memory */

/* host planes in, host planes out (device staging is internal); synchronous */
int ort_render_matte(ort_scene *scene, const ort_render_params *params, const ort_matte *m, const ort_matte_planes *planes, ort_stats *stats);
int ort_render_matte_device(ort_scene *scene, const ort_render_params *params, const ort_matte *m, const ort_matte_planes *planes, void *hip_stream,
                            ort_stats *stats);
/* view_count frames per plane, view-major */
int ort_render_views_matte(ort_scene *scene, const ort_render_params *params, const ort_view *views, uint32_t view_count, const ort_matte *m,
                           const ort_matte_planes *planes, ort_stats *stats);
int ort_render_views_matte_device(ort_scene *scene, const ort_render_params *params, const ort_view *views, uint32_t view_count, const ort_matte *m,
                                  const ort_matte_planes *planes, void *hip_stream, ort_stats *stats);

/* ---- a mask from matte slots: the coverage of a selection of ids -----
 * out_mask[p] = (float)(the sum of counts[p][j] over the slots j whose ids[p][j] is in select) / (float)spp: a u32 sum that wraps
 * as u32 sums do, one conversion and one f32 division.  ids and counts hold `slots` words per pixel as ort_render_matte writes them
 * ([frame][pixel][slot]), out_mask one f32 per pixel; a duplicate in select counts once; slots that hold ORT_MATTE_EMPTY are never
 * selected.  No scene and no allocation: the call names its device, as ort_denoise does, and the device form enqueues one kernel on
 * hip_stream and does not wait.  select is HOST memory in both forms, copied before the call returns.
 * frame_count == 0 is ORT_OK without a launch.  ORT_ERR_INVALID, in this order: a null ids, counts, select or out_mask; one of ids,
 * counts, out_mask not 4-byte aligned; slots 0 or above ORT_MAX_MATTE_SLOTS; width or height < 1 or
 * frame_count*width*height*slots >= 1 << 31; spp outside [1, 1 << 24]; select_count outside [1, ORT_MAX_MATTE_SELECT]; ORT_MATTE_EMPTY in select.
 * ORT_ERR_NO_DEVICE: no such device. */
#define ORT_MAX_MATTE_SELECT 256u
int ort_matte_mask(int device, const uint32_t *ids, const uint32_t *counts, uint32_t slots, uint32_t spp, const uint32_t *select,
                   uint32_t select_count, int32_t width, int32_t height, uint32_t frame_count, float *out_mask);
int ort_matte_mask_device(int device, const void *d_ids, const void *d_counts, uint32_t slots, uint32_t spp, const uint32_t *select,
                          uint32_t select_count, int32_t width, int32_t height, uint32_t frame_count, void *d_out_mask, void *hip_stream);

/* ---- denoising: a variance-guided, edge-avoiding a-trous filter over rendered frames -----------
 * What uses the planes above: the mean colour with its sample count n and its sum of squared sample luminance Q (ort_render_adaptive,
 * ort_render_sample_map, ort_render_accumulate) and the guide planes of ort_render_features.  `iterations` passes of 5 x 5 taps at
 * stride 1, 2, 4, ... over the albedo-demodulated colour; a tap's weight falls with the angle between the normals, with the depth
 * difference and with the luminance difference measured in standard deviations of the pixel's own noise.  The calls take no scene
 * handle -- a frame loaded from a checkpoint can be denoised -- and `device` is used as ort_unit_eval_device uses it.
 * Planes.  All six are required; each holds frame_count frames of width*height entries, view-major, row 0 at the bottom; out_rgb is
 * 3 f32 per pixel likewise.  No tap ever crosses from one frame into another: frame f of a batch is the single-frame call's result
 * for that frame's planes.  out_rgb may be in->rgb itself (in place); any other overlap is the caller's error and is not checked.
 * Every operation below is a separately rounded f32 operation (no FMA), and no weight uses a transcendental function, so the
 * result is defined bit for bit.  lum(c) = (0.2126f*c.x + 0.7152f*c.y) + 0.0722f*c.z.  fall(x): r = 1.0f / (1.0f + x); r = r*r;
 * r = r*r.
 * Prologue, per pixel.  n = count, fn = (float)n; a_k = albedo_k > 1e-3f ? albedo_k : 1e-3f; c_k = rgb_k / a_k; Y = lum(rgb);
 * v = m2 / fn - Y*Y; if (v < 0) v = 0; vm = n > 1 ? v / (fn - 1.0f) : Y*Y; la = lum(a); var = vm / (la*la).
 * The pixel is USABLE iff n >= 1 and all of rgb, m2, albedo, normal, depth, c and var are finite.  Usability is decided here and
 * never judged again.  An unusable pixel is never a tap, and its output is out_rgb = rgb, the input's bits: a pixel with
 * count == 0 (what a sample map left out), a NaN pixel, a pixel whose variance overflows.
 * Iteration j = 0 .. iterations-1, stride s = 1 << j, for each usable pixel p; inputs are the c and var planes of the previous
 * iteration (two planes, used in turn):
 *  - variance prefilter.  G = GW = 0; for dy = -1..1 (outer), dx = -1..1 (inner), q = p + (dx, dy): skip q outside the frame or
 *    unusable; w3 = k3[|dx|] * k3[|dy|] with k3 = {0.5, 0.25}; G = G + w3*var_q; GW = GW + w3.  Then g = G / GW.
 *  - l_p = lum(c_p); den = (sigma_l*sigma_l)*g + 1e-10f.
 *  - taps.  S = (0, 0, 0), V = 0, W = 0; for dy = -2..2 (outer), dx = -2..2 (inner), q = p + s*(dx, dy): skip q outside the frame
 *    or unusable; h = k[|dx|] * k[|dy|] with k = {0.375, 0.25, 0.0625}.  The centre tap has w = h.  Any other tap:
 *       d  = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z
 *       wn = d > 0 ? d : 0, then wn = wn*wn, normal_squarings times
 *       dz = z_p - z_q;  zm = max(|z_p|, |z_q|)
 *       xz = (dz*dz) / (((zm*zm) * (float)(s*s*(dx*dx + dy*dy))) * (sigma_z*sigma_z))
 *       dl = l_p - lum(c_q);  xl = (dl*dl) / den
 *       w  = ((h*wn) * fall(xz)) * fall(xl);  if w is not finite, w = 0
 *    then, for every tap: S_k = S_k + w*c_q,k;  V = V + (w*w)*var_q;  W = W + w.
 *  - result.  c'_p = S / W component by component, var'_p = V / (W*W).  Unusable pixels keep their entries.
 * After the last iteration out_rgb_k = c'_k * a_k.
 * Consequences.  A pixel with a zero normal (a miss) has wn = 0 with every neighbour and keeps its own value up to (rgb/a)*a.
 * Mirrors and glass are not followed by the feature planes: what is seen in them is filtered by the guides of the surface itself;
 * ort_render_follow's planes follow them.
 * Values that become non-finite during the iterations propagate by IEEE rules; a NaN output matches the contract by position, not
 * by sign or payload, as elsewhere in this library.  Results do not depend on frame_count, on the tile shape, or on how pixels
 * fall on the GPU's lanes.
 * frame_count == 0 returns ORT_OK without a launch, whatever the other arguments.  Otherwise errors are reported before any device
 * work, in this order: ORT_ERR_INVALID (a null params struct, planes struct, plane or out_rgb; then a plane or out_rgb not 4-byte
 * aligned; then width or height < 1 or frame_count*width*height >= 2^31; then iterations outside [1, 8]; then normal_squarings > 8;
 * then sigma_l or sigma_z NaN, infinite or <= 0; then, in the device form, a workspace that is null, not 16-byte aligned or shorter
 * than ort_denoise_workspace_bytes), then ORT_ERR_NO_DEVICE (no such device).
 * The host form stages the planes, allocates and frees its own workspace and is synchronous.  The device form takes DEVICE pointers
 * on `device` (the two structs are host memory, read before the call returns), enqueues on hip_stream (NULL = the default stream)
 * and waits only when stats != NULL; it never allocates: the caller passes a workspace of ort_denoise_workspace_bytes = 48 bytes per
 * pixel and frame (two planes of (c, var), one of (normal, depth)), 16-byte aligned, whose contents are lost.  stats (may be NULL)
 * gets kernel_ms, the HIP-event time of the pack and the passes; every other field is 0. */
typedef struct {
    uint32_t iterations;        /* 1 .. 8 passes, strides 1 .. 1 << (iterations-1) */
    uint32_t normal_squarings;  /* 0 .. 8: the normal weight is max(0, n_p . n_q) ^ (2 ^ normal_squarings) */
    float sigma_l;              /* luminance tolerance, in standard deviations */
    float sigma_z;              /* relative depth tolerance per pixel of tap distance */
} ort_denoise_params;
typedef struct {            /* HOST pointers in the host form, DEVICE pointers in the device form; the struct is host memory */
    const float    *rgb;    /* 3 f32 / pixel: the MEAN colour (out_rgb of any render call, or sum / count) */
    const float    *m2;     /* f32: Q, the sum of squared sample luminance */
    const uint32_t *count;  /* u32: n, the samples the pixel has had */
    const float    *albedo; /* 3 f32 / pixel   ort_render_features' planes */
    const float    *normal; /* 3 f32 / pixel */
    const float    *depth;  /* f32 */
} ort_denoise_planes;
int ort_denoise_workspace_bytes(int32_t width, int32_t height, uint32_t frame_count, uint64_t *bytes);
int ort_denoise(int device, const ort_denoise_params *p, const ort_denoise_planes *in, int32_t width, int32_t height,
                uint32_t frame_count, float *out_rgb, ort_stats *stats);
int ort_denoise_device(int device, const ort_denoise_params *p, const ort_denoise_planes *in, int32_t width, int32_t height,
                       uint32_t frame_count, void *d_out_rgb, void *d_workspace, uint64_t workspace_bytes, void *hip_stream,
                       ort_stats *stats);

/* ---- planning the next pass: where a frame's next samples go (csrc/ort_sampleplan.h) -----------
 * The step between two passes of ort_render_accumulate: from a frame's colour, its sum of squared sample luminance Q and its
 * sample counts n, a sample map -- the layout ort_render_sample_map and ort_render_accumulate read -- that asks, for every pixel,
 * for the samples that bring the worst error of its neighbourhood down to a tolerance at the variance measured so far; and per
 * frame 32 bytes of totals, which are all a caller needs to read to decide whether to go on.  The calls take no scene handle -- a
 * checkpoint can be planned -- and `device` is used as ort_unit_eval_device uses it.
 * Planes.  rgb, m2 and count hold frame_count frames of width*height entries, view-major, row 0 at the bottom; sample_map is one
 * u32 per pixel likewise and totals is frame_count entries.  No window crosses from one frame into another and a budget is per
 * frame: frame f of a batch is the single-frame call's result for that frame's planes.  Every pixel of every frame of the map is
 * written.  The map may not overlap a plane (not checked).
 * Every f32 operation below is rounded on its own (no FMA, correctly rounded divides); nothing uses a transcendental function, and
 * the allocation uses the SQUARED relative error, so no square root is taken.  Everything that is summed is an integer.  The result
 * is defined bit for bit.  lum(c) = (0.2126f*c.x + 0.7152f*c.y) + 0.0722f*c.z.  tol2 = tolerance*tolerance, taken once.
 * Per pixel, its error e (the terms of the adaptive calls' stopping rule):
 *    n = count; fn = (float)n; m = rgb_is_sum ? lum(rgb) / fn : lum(rgb);
 *    v = m2 / fn - m*m; if (v < 0) v = 0; vm = v / (fn - 1.0f);
 *    a = |m|; b = a > floor ? a : floor; e = vm / (b*b).
 *    The pixel is UNKNOWN if n < 2.  It is INVALID if it is not unknown and either n > 1<<24 or e is not finite.  Unknown and
 *    invalid pixels have e = +0.  A valid e that is not > 0 is +0 (a -0 never reaches a comparison of bits).  The pixel is
 *    UNCONVERGED if it is valid and e > tol2.  This is decided once; the later steps read e alone.
 * Window.  d = the maximum of e over the (2*radius+1)^2 pixels around the pixel that lie inside its own frame: a maximum of
 * non-negative finite floats, independent of order.
 * What the pixel wants.  room = min(cap, (1<<24) - min(n, 1<<24)).
 *    unknown pixel:       want = min(pilot, room)
 *    otherwise, d > tol2: need = fn * (d / tol2) - fn;
 *                         k = need >= 16777216.0f ? 1<<24 : (need > 0 ? (uint32_t)need : 0);  if (k < min_add) k = min_add;
 *                         want = min(k, room)
 *    otherwise:           want = 0
 *    An invalid pixel wants nothing of its own error but is planned from its neighbours' like any other: a NaN pixel cannot eat
 *    a budget for ever.
 * Per frame.  wanted = the sum of want, in 64 bits.  If budget == 0 or wanted <= budget, add = want; otherwise
 * add = (uint32_t)((uint64_t)want * budget / wanted), an integer division.  sample_map = add.  planned = the sum of add.
 * worst = the maximum e.  unconverged, unknown and invalid count pixels.
 * Consequences.  planned <= budget wherever a budget is given.  A scaled frame has planned > budget - (its pixels with want > 0).
 * A scaled plan can be all zero while pixels are unconverged: the budget is exhausted.  planned == 0 and unconverged == 0 together
 * mean converged (with pilot > 0 an unknown pixel with room keeps planned above 0).  add <= want <= room <= cap: the pass that
 * follows, with params->spp = cap, takes exactly the map.  Results do not depend on frame_count, on the tile shape, or on which
 * lane or workgroup added what.
 * frame_count == 0 returns ORT_OK without a launch, whatever the other arguments.  Otherwise errors are reported before any device
 * work, in this order: ORT_ERR_INVALID (a null params struct, planes struct, plane, sample_map or totals; then a plane or the map
 * not 4-byte aligned or totals not 8-byte aligned; then width or height < 1 or frame_count*width*height >= 2^31; then, in the
 * struct's order: tolerance NaN, infinite, <= 0 or with tolerance*tolerance (f32) == 0; floor NaN, infinite or <= 0; radius > 3;
 * min_add == 0; cap outside [1, 1<<24]; rgb_is_sum > 1; reserved != 0; budget > 1<<39; then, in the device form, a workspace that is
 * null, not 4-byte aligned or shorter than ort_plan_samples_workspace_bytes), then ORT_ERR_NO_DEVICE (no such device).
 * The host form stages the planes, allocates and frees its own workspace and is synchronous.  The device form takes DEVICE pointers
 * on `device` (the two structs are host memory, read before the call returns), zeroes d_totals on hip_stream itself, enqueues there
 * (NULL = the default stream) and waits only when stats != NULL; it never allocates: the caller passes a workspace of
 * ort_plan_samples_workspace_bytes = 4 bytes per pixel and frame (the e plane), whose contents are lost.  stats (may be NULL) gets
 * kernel_ms, the HIP-event time of the three kernels; every other field is 0. */
typedef struct {
    float    tolerance;   /* target relative standard error of a pixel's mean luminance; finite, > 0, and tolerance*tolerance (f32) > 0 */
    float    floor;       /* stands in for |mean luminance| in the dark, as ort_adaptive's floor; finite, > 0 */
    uint32_t radius;      /* 0..3: a pixel plans for the worst error within (2r+1) x (2r+1) */
    uint32_t pilot;       /* samples asked for a pixel that has had fewer than 2 (no estimate yet); may be 0 */
    uint32_t min_add;     /* >= 1: the least an unconverged pixel asks for */
    uint32_t cap;         /* 1 .. 1<<24: the most any pixel gets in one pass (params->spp of the pass that follows) */
    uint32_t rgb_is_sum;  /* 0: rgb is the MEAN colour; 1: rgb is ort_accum_planes.sum_rgb, the undivided sum */
    uint32_t reserved;    /* must be 0 */
    uint64_t budget;      /* 0: no budget; else 1 .. 1<<39: the most samples one FRAME gets in this pass */
} ort_plan_params;
typedef struct {            /* HOST pointers in the host form, DEVICE pointers in the device form; the struct is host memory */
    const float    *rgb;    /* 3 f32 / pixel: the mean colour, or with rgb_is_sum the undivided sum */
    const float    *m2;     /* f32: Q, the sum of squared sample luminance */
    const uint32_t *count;  /* u32: n, the samples the pixel has had */
} ort_plan_planes;
typedef struct {
    uint64_t wanted, planned;                 /* the sums of want and of add over the frame */
    uint32_t unconverged, unknown, invalid;   /* pixels */
    float    worst;                           /* the largest e of the frame: a squared relative standard error */
} ort_plan_totals; /* 32 bytes */
int ort_plan_samples_workspace_bytes(int32_t width, int32_t height, uint32_t frame_count, uint64_t *bytes);
int ort_plan_samples(int device, const ort_plan_params *p, const ort_plan_planes *in, int32_t width, int32_t height,
                     uint32_t frame_count, uint32_t *sample_map, ort_plan_totals *totals, ort_stats *stats);
int ort_plan_samples_device(int device, const ort_plan_params *p, const ort_plan_planes *in, int32_t width, int32_t height,
                            uint32_t frame_count, void *d_sample_map, void *d_totals, void *d_workspace, uint64_t workspace_bytes,
                            void *hip_stream, ort_stats *stats);

/* ---- multi-GPU: block sharding and the one collective -------------------------------------
 * Replaces main()'s shared-memory tile pool (macos_main.mm:565-671: eight pthreads, one queue, one framebuffer)
 * across the GPUs of a node: scene replicated, 8x8 blocks dealt round-robin, every rank renders its blocks into a
 * packed buffer (ORT_RENDER_PACKED) and ONE gather brings them to rank 0 -- grouped ncclSend / ncclRecv over RCCL
 * (xGMI), then an un-permute kernel on rank 0.  Seeds are per pixel, so the assembled image is bit-identical to a
 * one-GPU render.  librccl.so is loaded on first use. */
int ort_shard_block_count(int32_t width, int32_t height, uint32_t shard_index, uint32_t shard_count, uint64_t *blocks);
/* host-side (CPU) packing, for callers that move the blocks themselves */
int ort_pack_blocks_host(const float *full_rgb, int32_t width, int32_t height, uint32_t shard_index, uint32_t shard_count, float *packed);
int ort_unpack_blocks_host(const float *packed, int32_t width, int32_t height, uint32_t shard_index, uint32_t shard_count, float *full_rgb);
/* device-side un-permute of one shard's packed blocks into a full frame (both DEVICE pointers) */
int ort_unpack_blocks_device(const void *d_packed, int32_t width, int32_t height, uint32_t shard_index, uint32_t shard_count,
                             void *d_full_rgb, void *hip_stream);

typedef struct ort_comm ort_comm;
#define ORT_COMM_ID_BYTES 128
/* one process per GPU: rank 0 draws an id (ncclGetUniqueId), hands it to the other ranks by any means, then every
   rank creates its communicator on its device.  world == 1 needs no id and never touches RCCL. */
int ort_comm_unique_id(void *id /* ORT_COMM_ID_BYTES */);
int ort_comm_create(const void *id, int rank, int world, int device, ort_comm **out);
/* one process driving all GPUs (ncclCommInitAll): fills out[0 .. world) */
int ort_comm_create_local(int world, const int *devices, ort_comm **out);
void ort_comm_destroy(ort_comm *comm);
/* the collective: every rank passes its packed blocks (device pointer, same width/height/world as rendered with);
   rank 0 also passes the full frame to assemble (device pointer, width*height*3 floats), others NULL.  Enqueued on
   hip_stream of the communicator's device; returns without waiting. */
int ort_gather_framebuffer(ort_comm *comm, const void *d_packed, void *d_full_rgb, int32_t width, int32_t height, void *hip_stream);
/* the same for ort_comm_create_local's communicators, all ranks in one call (streams may be NULL) */
int ort_gather_framebuffer_local(ort_comm **comms, int world, const void *const *d_packed, void *d_full_rgb_rank0, int32_t width,
                                 int32_t height, void *const *hip_streams);

/* ---- diagnostics: per-function evaluation ON THE DEVICE (parity tests) -----------------
 * records: count x {u32 op; f32 in[24]}; out: count x f32[8].  Ops (reference file:line):
 *  1 triangle  ray.cpp:63-115   in v0 v1 v2 o d              out t n.xyz
 *  2 sphere    ray.cpp:132-190  in c r o d                   out t n.xyz
 *  3 aab       ray.cpp:206-283  in min max o d               out t n.xyz
 *  4 cylinder  ray.cpp:286-352  in base axis r o d           out t n.xyz
 *  5 sample_brdf ray.cpp:1100   in seed(bits) N wo rough Kd Ks Kt ior   out wi.xyz is_transmission rng(bits)
 *  6 pdf_brdf  ray.cpp:1007     in N wi wo rough Kd Ks Kt ior           out p
 *  7 eval_scattering ray.cpp:936 in N wi wo Kd Ks Kt ior rough dist     out f.xyz
 *  8 sample_lobe ray.cpp:1065   in N c phi                   out v.xyz
 *  9 libm      (deterministic)  in x y                       out sinf(x) cosf(x) atan2f(y,x) powf(x,y) logf(x)
 * 10 normalize math.h:298-310   in v                         out v.xyz
 * 11 fresnel/ggx/geometry ray.cpp:825-897 in Ks l_dot_h N H rough w     out F.xyz D G
 * 12 rng       random.h:5-53    in seed(bits) job(bits)      out step(bits) rng_01 rng_between(0,2pi) state(bits) job_seed(bits)
 * 13 IEEE ops                   in a b c                     out a/b sqrt(a) a*b a+b a-b (f32)bits(a) a*b+c
 * Ops 14-20 run the specialised forms the render and raycast kernels call in place of the functions above, composed
 * as those kernels compose them; each must give its generic function's answer (diagnostics for the parity tests):
 * 14 aab forms  (op 3's inputs, 1/d as op 3)                 out hit_aab_finite t n.xyz, hit_aab_t_finite t, hit_aab_t t
 *               (the _finite forms only for finite o and 1/d: all_finite6)
 * 15 pdf_eval_scattering in N wi wo Kd Ks Kt ior rough dist rr      out p f.xyz (f = 0 unless p > 1e-6)
 * 16 diffuse pdf/eval    (op 15's inputs)                    out pdf_brdf<true> * rr, eval_scattering<true> f.xyz
 *               (only for materials with |Ks|^2, |Kt|^2, ps_c, pt_c all 0)
 * 17 BSDF sample as the all-lobes kernels draw it (op 5's inputs and outputs): sample_brdf_draw, ort_sincosf of phi,
 *               sample_brdf_finish<NORMALIZED = false>, normalize
 * 18 the same as the diffuse kernels draw it (sample_brdf_draw<true>, sample_brdf_finish<false, true>; diffuse materials)
 * 19 sincos     in x                                         out ort_sincosf of x: sin cos
 * 20 hemisphere draw as the irradiance kernels compose it    in seed(bits) n.xyz     out d.xyz wo.xyz rng(bits)
 *               (two rng_01, sqrt, ort_sincosf of 2 pi e1, sample_lobe_n about normalize(n), normalize; wo = -normalize(d); the
 *               stream after the two draws; the seed is a stream state as it stands, 0 not taken as 1)
 * 21 sphere draw as the SH light-probe kernels compose it     in seed(bits) n.xyz     out d.xyz wo.xyz rng(bits)
 *               (op 20 with c = 1 - 2 e0 where that has sqrt(e0))
 * 22 SH basis   in d.xyz                                     out b1 b2 b3 b4 b5 b6 b7 b8 of ort_probe_sh (b0 is a constant) */
int ort_unit_eval_device(int device, const void *records, uint32_t count, float *out);

/* ---- output ------------------------------------------------------------------------
 * v3_to_rgbe (macos_main.mm:242-261) and the .hdr writer (macos_main.mm:263-287,683-707) */
uint32_t ort_rgbe(float r, float g, float b);
int ort_write_hdr(const char *path, const float *rgb, int32_t width, int32_t height);

#ifdef __cplusplus
}
#endif
#endif /* ORT_H */
