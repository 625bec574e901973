/*
 * ort_scene.h -- host-side scene object behind the opaque ort_scene handle.
 */
#ifndef ORT_SCENE_H
#define ORT_SCENE_H

#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/ort.h"
#include "ort_plan.h" /* RenderKind */

namespace ort {

struct HostMesh {
    std::vector<float> vertices;   // 3 * n, world space after placement
    std::vector<uint32_t> indices; // 3 * triangles
    uint32_t mat = 0;
    ort_v3 aabb_min = {0, 0, 0}, aabb_max = {0, 0, 0};
};

/* ---- device-resident layout (mirrored on the host before upload) -----------------------
 * All records are 16-byte multiples so one lane fetches a record with dwordx4 loads.
 *
 * Node (64 B): a binary node carrying BOTH children's boxes, so one fetch decides both.
 *   lo0.xyz hi0.xyz lo1.xyz hi1.xyz child0 child1 pad pad
 * child word: bit31 = leaf.  interior: [29:0] node index, bit30 = a sphere lives below.
 *   leaf: [30:28] primitive kind, [27:24] count-1, [23:0] first index within that kind's array.
 */
struct DevNode {
    float lo0[3], hi0[3], lo1[3], hi1[3];
    uint32_t child0, child1, pad0, pad1;
};
static_assert(sizeof(DevNode) == 64, "node record must be 64 B");

/* kind codes: SPHERE = 4 so that bit 30 of a leaf word means "sphere leaf"; interior child
   words reuse bit 30 as "a sphere lives below".  Such children are exempt from the
   closer-than-best cull: ray_intersect_with_sphere's tangent branch (ray.cpp:174-183) reports
   t = -b/(2a), a point OUTSIDE the sphere's box and nearer than its entry distance. */
enum : uint32_t { PRIM_TRI = 0, PRIM_BOX = 2, PRIM_CYL = 3, PRIM_SPHERE = 4 };
constexpr uint32_t LEAF_BIT = 0x80000000u;
constexpr uint32_t SPHERE_BELOW_BIT = 0x40000000u;
constexpr uint32_t NODE_INDEX_MASK = 0x3fffffffu;
constexpr uint32_t EMPTY_CHILD = 0xffffffffu; /* leaf, kind 7: never visited (box is inverted) */
constexpr uint32_t MAX_LEAF_PRIMS = 16;
/* depth of the fast tree = what a traversal stack must hold at most.  ONE constant: ort_tree.cpp builds within it
   (and refuses a tree that exceeds it), ort_lane.h static_asserts that its smallest stack (the re-traversal of
   resolve_hit: LDS entries minus the four it borrows, plus the scratch tail) holds it */
constexpr uint32_t kTreeDepthBudget = 60;
#ifndef ORT_TREELET_NODES
#define ORT_TREELET_NODES 32
#endif
constexpr uint32_t kTreeletNodes = ORT_TREELET_NODES; /* the breadth-first top of the fast tree has indices [0, 32): kept in LDS by the kernel */

/* Wide node (128 B): the same tree with every other level folded away -- up to FOUR children per node, their boxes
 * stored by coordinate (lo.x of the four children in one 16-byte word, ...) and the four child words; child words as in
 * DevNode, unused slots = EMPTY_CHILD with an inverted box.  A ray then makes half the dependent node fetches on its
 * way down, which is what bounds deep trees (the 1M-triangle scene: ~10 binary visits per ray; profiles/r02_tuning.md).
 * Built from the binary tree by ort_tree.cpp (collapse_to_wide); used by the kernel variant for trees that leave the L2. */
struct DevNode4 {
    float lox[4], loy[4], loz[4], hix[4], hiy[4], hiz[4];
    uint32_t child[4];
    uint32_t pad[4];
};
static_assert(sizeof(DevNode4) == 128, "wide node record must be 128 B");

inline uint32_t make_leaf(uint32_t kind, uint32_t first, uint32_t count) {
    return LEAF_BIT | (kind << 28) | ((count - 1u) << 24) | (first & 0x00ffffffu);
}

/* Triangle slab (48 B): v0, e1 = v1 - v0, e2 = v2 - v0, n = cross(e1, e2).  e1/e2/n are the
   reference's own f32 expressions (ray.cpp:87-88,110) evaluated once on the host: same
   bits as evaluating them per test. */
struct DevTri { float v0[3], e1[3], e2[3], n[3]; };
static_assert(sizeof(DevTri) == 48, "triangle slab must be 48 B");

struct DevSphere { float c[3]; float r; };                     /* 16 B */
struct DevBox { float lo[3]; float pad0; float hi[3]; float pad1; }; /* 32 B */
/* cylinder: base, radius, the row-major rotation of rotation_matrix_along_z(axis)
   (ray.cpp:8-33) and |axis| (ray.cpp:302), all precomputed with the reference's f32
   expressions; 64 B */
struct DevCyl { float base[3]; float r; float rot[9]; float len; float pad[2]; };
static_assert(sizeof(DevCyl) == 64, "cylinder record must be 64 B");

/* material as the path reads it (ray.h:30-40 minus specular.w) plus the per-material values that
   sample_brdf / pdf_brdf / eval_scattering recompute on every call (ray.cpp:939,1010-1018,
   1105-1113): lobe weights |K|/(|Kd|+|Ks|+|Kt|) and Kd/pi, evaluated once on the host with the
   reference's f32 expressions (same bits); 80 B */
struct DevMaterial {
    float diffuse[3]; float ior;
    float specular[3]; uint32_t is_light;
    float transmission[3]; float pd_c;
    float emit[3]; float ps_c;
    float ed[3]; float pt_c;
};
static_assert(sizeof(DevMaterial) == 80, "material record must be 80 B");
DevMaterial make_dev_material(const ort_material &m); /* ort_tree.cpp */

struct Tree {
    std::vector<DevNode> nodes;
    std::vector<DevNode4> nodes4; /* the 4-wide form of the same tree (empty if it was not built) */
    uint32_t max_depth4 = 0;      /* levels of the wide tree: a traversal stacks at most 3 entries per level */
    std::vector<DevTri> tris;
    std::vector<uint32_t> tri_mat;
    std::vector<DevSphere> spheres;
    std::vector<uint32_t> sphere_mat;
    std::vector<DevBox> boxes;
    std::vector<uint32_t> box_mat;
    std::vector<DevCyl> cyls;
    std::vector<uint32_t> cyl_mat;
    /* source index -> slot in the reordered arrays above (triangles: mesh-major triangle id) */
    std::vector<uint32_t> tri_slot, sphere_slot, box_slot, cyl_slot;
    uint32_t leaf_count = 0, max_leaf_prims = 0, max_depth = 0;
    float sah_cost = 0;
    /* the scene's few analytic shapes are not in the tree: every ray tests all of them up front, the
       whole wave in step (ort_lane.h: prologue_tests); the tree then holds the triangles only */
    bool analytic_prologue = false;
    uint32_t pro_boxes = 0, pro_spheres = 0, pro_cyls = 0; /* shapes [0, n) of each kind form the prologue */
    bool built = false;
};

/* ---- the reference-compatible loose octree (ort_reftree.cpp) ---------------------------
 * Node (48 B): lo.xyz first_child | hi.xyz rec_first | rec_count flags pad pad
 * flags: bit0 = is_leaf, bit1 = the reference's push buffer is non-empty.
 * recs: kind << 28 | slot (same slots as the fast tree's primitive arrays).
 * chain_boxes: per record-holding node, the boxes of that node and its ancestors up to,
 * not including, the root (2 x F4 each); *_chain[slot] = len << 28 | first pair index. */
struct F4 { float x, y, z, w; };
struct DevRefNode {
    float lo[3]; int32_t first_child;
    float hi[3]; uint32_t rec_first;
    uint32_t rec_count, flags, pad0, pad1;
};
static_assert(sizeof(DevRefNode) == 48, "reference octree node must be 48 B");

struct RefTree {
    std::vector<DevRefNode> nodes;
    std::vector<uint32_t> recs;
    std::vector<F4> chain_boxes;
    std::vector<uint32_t> tri_chain, sphere_chain, box_chain, cyl_chain;
    /* position of each primitive in the reference's test order: raycast_bvh walks breadth-first
       (children in slot order) and a node's records in push order, and among bit-equal hit
       distances the first one tested wins (strict <, ray.cpp:653,670,686,708) */
    std::vector<uint32_t> tri_order, sphere_order, box_order, cyl_order;
    uint32_t nonempty_leaves = 0, max_leaf_records = 0;
    uint32_t unnested_chains = 0; /* chains whose boxes are not nested (expected 0; those take the full walk) */
    bool built = false;
};

/* What shading asks about a ray's winner, one record per primitive (SceneView::prim_info, ort_lane.h; build_prim_info,
   ort_setup.h).  chain: len << 28 | kChainNested | first pair of chain_boxes (RefTree's *_chain word); mat: material index */
struct PrimInfo { uint32_t chain, mat; };

struct DeviceScene; /* ort_kernels.hip */

struct Scene {
    std::vector<ort_material> materials;
    std::vector<ort_sphere> spheres;
    std::vector<ort_box> boxes;
    std::vector<ort_cylinder> cylinders;
    std::vector<ort_light> lights;
    std::vector<HostMesh> meshes;
    ort_v3 ambient = {0, 0, 0};
    ort_v3 camera_p = {0, 0, 0};
    float camera_quat[4] = {0, 0, 0, 1}; /* xyzw */
    float camera_height_ratio = 0;
    int32_t screen_width = 0, screen_height = 0;

    /* main() inserts one inert CSG shape into its octree (macos_main.mm:322-332,532-538); it can
       never be hit but it shapes the node boxes, so scenes loaded from .scn carry it */
    bool reference_csg = false;

    Tree tree;
    RefTree ref;
    DeviceScene *dev = nullptr;
};

/* ort_parse.cpp */
int parse_scn_text(const char *text, size_t size, const char *base_dir, Scene *scene, std::string *err);
int read_file(const char *path, std::vector<char> *out);
void camera_basis(const Scene &s, int32_t width, int32_t height, ort_camera *out);
/* the same for any pose (macos_main.mm:550-556) */
void camera_from_pose(const ort_v3 &p, const float quat_xyzw[4], float height_ratio, int32_t width, int32_t height, ort_camera *out);

/* The box of everything ort_tree.cpp sized the quadric boxes for: all shapes and the scene's own camera_p.  Ray origins within
   it, with the 0.25 of slack per side the tree allows (build_tree: e = hi - lo + 0.5), get the reference's answers from the fast
   tree: what the ray queries test a caller's origin against (raycast_needs_exact) and ort_render_views a caller's camera. */
inline void scene_origin_box(const Scene &s, float lo[3], float hi[3]) {
    lo[0] = hi[0] = s.camera_p.x; lo[1] = hi[1] = s.camera_p.y; lo[2] = hi[2] = s.camera_p.z;
    auto grow = [&](float x, float y, float z, float r) {
        const float p[3] = {x, y, z};
        for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], p[k] - r); hi[k] = std::max(hi[k], p[k] + r); }
    };
    for (const ort_sphere &q : s.spheres) grow(q.center.x, q.center.y, q.center.z, fabsf(q.r));
    for (const ort_box &q : s.boxes) { grow(q.min.x, q.min.y, q.min.z, 0.0f); grow(q.max.x, q.max.y, q.max.z, 0.0f); }
    for (const ort_cylinder &q : s.cylinders) {
        grow(q.base.x, q.base.y, q.base.z, fabsf(q.r));
        grow(q.base.x + q.axis.x, q.base.y + q.axis.y, q.base.z + q.axis.z, fabsf(q.r));
    }
    for (const HostMesh &m : s.meshes)
        for (size_t i = 0; i + 2 < m.vertices.size(); i += 3) grow(m.vertices[i], m.vertices[i + 1], m.vertices[i + 2], 0.0f);
}

/* ort_tree.cpp */
int build_tree(Scene *scene, std::string *err);
/* ort_reftree.cpp */
int build_ref_tree(Scene *scene, std::string *err);

/* ort_hdr.cpp */
uint32_t rgbe_pack(float r, float g, float b);

/* ort_kernels.hip */
int device_count(int *n, std::string *err);
int device_upload(Scene *scene, int device, std::string *err);
void device_release(Scene *scene);
/* One camera render call.  host: the planes are the caller's memory, staged whole both ways so that pixels outside the rect keep
   what they held, and the call returns when they are back; otherwise they are device pointers and the call is one launch
   enqueued on stream (it waits only for stats or job_states).  Every plane is passed once, whichever form it is */
struct RenderCall {
    bool host;
    void *stream;
    ort_stats *stats;         /* may be null */
    const ort_tile_job *jobs; /* explicit jobs (the TILE32 / WHOLE policies, ort_tiled_raytrace_batch); null: the PIXEL / CHUNK job space of p */
    uint32_t job_count;
    uint32_t *job_states;     /* ... and where their final states go (may be null): always the caller's memory, read back before the call returns */
    const ort_view *views;    /* view_count frames, each from views[v].camera with views[v].seed; null: the scene's own camera and p->seed */
    uint32_t view_count;
    RenderKind kind;          /* what the render is (ort_plan.h); the fields below are the arguments of the kinds that are not plain, each null where the kind does not take it */
    const ort_adaptive *ad;   /* RK_ADAPTIVE: the stopping rule (checked by the caller) that cuts every pixel of views (not null then) */
    const ort_light_groups *groups; /* the light-group render's table (checked by the caller; views not null then, ad null); null: no group frames */
    void *out_groups;         /* ... and its view_count x group_count frames, as the call's form has them; out_rgb and states may then be null */
    const void *sample_map;   /* the sample-map render's map, view_count planes of a word a pixel, as the call's form has them (checked by the caller; views not null then, ad and groups null); null: every job is p->spp long */
    void *acc_sum;            /* the accumulating render's plane of undivided colour sums, as the call's form has it (checked by the caller; views not null then, ad and groups null; sample_map may be null); its count, m2 and states planes travel as out_spp, out_m2 and states, all four read and written; null: no accumulation */
    uint32_t depth_bins;      /* RK_DEPTHS: the bin count G (checked by the caller; views not null then, ad, groups, sample_map and acc_sum null); its view_count x G bin frames travel as out_groups and its view_count x G length planes (may be null) as out_spp; out_rgb and states may be null; 0: no depth bins */
};
/* out_rgb: view_count frames, view-major (or, ORT_RENDER_PACKED, this shard's blocks).  The adaptive render's other planes (each
   may be null, and is for a plain render): samples taken, sums of squared sample luminance and final states, a word a pixel */
int device_render(Scene *scene, const ort_render_params *p, const RenderCall &c, void *out_rgb, void *out_spp, void *out_m2, void *states, std::string *err);
int device_unit_eval(int device, const void *records, uint32_t n, float *out, std::string *err);
/* One ray query call.  host: the arrays are the caller's memory, staged to the device in bounded slices, and the call returns
   when the answers are back; otherwise they are device pointers and the call is one launch enqueued on stream (it waits only
   for stats).  Every array is passed once, whichever form it is */
struct QueryCall {
    bool host;
    uint64_t count;
    uint32_t flags;
    void *stream;
    ort_stats *stats; /* may be null */
};
/* closest hits: count rays -> count ort_hit */
int device_raycast(Scene *scene, const QueryCall &q, const void *rays, void *hits, std::string *err);
/* occlusion: count rays and their limits (tmax may be null: no limit) -> count bytes */
int device_occluded(Scene *scene, const QueryCall &q, const void *rays, const void *tmax, void *out, std::string *err);
/* ambient occlusion: count points (p, n), seeds and radii (radius may be null: no limit), spp samples each -> count open counts
   and, where asked for (null otherwise), bent sums (3 floats a point) and final states */
int device_ambient_occlusion(Scene *scene, const QueryCall &q, const void *points, const void *seeds, const void *radius, uint32_t spp, void *out_open,
                             void *out_bent, void *states, std::string *err);
/* radiance: count rays and seeds -> colours and, where asked for (null otherwise), final states.  ad == null: exactly spp samples
   per ray; otherwise the adaptive query (spp unread): the stopping rule's parameters, and two more optional outputs (samples
   taken, sum of squared sample luminance).  points: the irradiance queries -- the array holds count points (p, n) in the rays'
   place, and every sample's direction is drawn about n.  out_sh (with points, without ad; null otherwise): the SH light-probe
   query -- the direction is drawn over the whole sphere, out_sh gets 27 floats a point and out may be null */
int device_radiance(Scene *scene, const QueryCall &q, const void *rays, const void *seeds, uint32_t spp, float rr, const ort_adaptive *ad, void *out,
                    void *out_spp, void *out_m2, void *states, bool points, void *out_sh, std::string *err);
/* first-hit feature renders: view_count frames of p's rect (checked by the caller: PIXEL, no shards, not packed), view v from
   views[v].camera on views[v].seed, p->spp camera samples a pixel -> the planes asked for (null otherwise), view-major.  q.count is
   unread.  The host form stages every plane whole both ways, as device_render does, so that pixels outside the rect keep what they
   held */
int device_render_features(Scene *scene, const ort_render_params *p, const ort_view *views, uint32_t view_count, const QueryCall &q,
                           const ort_feature_planes &planes, std::string *err);
/* feature renders that follow mirrors and glass: device_render_features' frames, forms and staging with the seven planes of
   ort_render_follow; p->rr is the roulette's, max_bounces (checked by the caller) the cap on every path */
int device_render_follow(Scene *scene, const ort_render_params *p, const ort_view *views, uint32_t view_count, uint32_t max_bounces, const QueryCall &q,
                         const ort_follow_planes &planes, std::string *err);
/* ID-matte renders: device_render_features' frames, forms and staging with the five planes of ort_render_matte; m (checked by the
   caller) names the mode and the slots per pixel */
int device_render_matte(Scene *scene, const ort_render_params *p, const ort_view *views, uint32_t view_count, const ort_matte &m, const QueryCall &q,
                        const ort_matte_planes &planes, std::string *err);
/* a mask from matte slots (include/ort.h: ort_matte_mask), on `device` and without a scene.  host: ids, counts and out_mask are the
   caller's memory, staged whole; otherwise they are device pointers, nothing is allocated and the kernel is enqueued on stream
   without a wait.  select is host memory in both forms and travels in the launch.  The arguments are checked by the caller */
int device_matte_mask(int device, bool host, const void *ids, const void *counts, uint32_t slots, uint32_t spp, const uint32_t *select, uint32_t select_count,
                      int32_t w, int32_t h, uint32_t frames, void *out_mask, void *stream, std::string *err);
/* the denoiser (include/ort.h: ort_denoise), on `device` and without a scene.  host: every plane and out_rgb are the caller's
   memory, staged whole, and the workspace is the call's own (workspace unread); otherwise all are device pointers, the workspace is
   the caller's and the passes are enqueued on stream.  The arguments are checked by the caller */
int device_denoise(int device, bool host, const ort_denoise_params &p, const ort_denoise_planes &in, int32_t w, int32_t h, uint32_t frames, void *out_rgb,
                   void *workspace, void *stream, ort_stats *stats, std::string *err);
/* the sample planner (include/ort.h: ort_plan_samples), on `device` and without a scene.  host: the planes, the map and the totals
   are the caller's memory, staged whole, and the workspace is the call's own (workspace unread); otherwise all are device pointers,
   the workspace is the caller's and the kernels are enqueued on stream.  The arguments are checked by the caller */
int device_plan_samples(int device, bool host, const ort_plan_params &p, const ort_plan_planes &in, int32_t w, int32_t h, uint32_t frames, void *sample_map,
                        void *totals, void *workspace, void *stream, ort_stats *stats, std::string *err);
/* ort_comm.cpp */
struct Comm;
uint64_t comm_shard_blocks(int32_t w, int32_t h, uint32_t index, uint32_t count);
void pack_blocks_host(const float *full, int32_t w, int32_t h, uint32_t index, uint32_t count, float *packed);
void unpack_blocks_host(const float *packed, int32_t w, int32_t h, uint32_t index, uint32_t count, float *full);
int unpack_blocks_device(const void *d_packed, int32_t w, int32_t h, uint32_t index, uint32_t count, void *d_full, void *stream, std::string *err);
int comm_unique_id(void *id, std::string *err);
int comm_create(const void *id, int rank, int world, int device, Comm **out, std::string *err);
int comm_create_local(int world, const int *devices, Comm **out, std::string *err);
void comm_destroy(Comm *c);
int gather_framebuffer(Comm *c, const void *d_packed, void *d_full, int32_t w, int32_t h, void *stream, std::string *err);
int gather_framebuffer_local(Comm **cs, int world, const void *const *d_packed, void *d_full_root, int32_t w, int32_t h,
                             void *const *streams, std::string *err);
/* ort_tree.cpp: rotation_matrix_along_z(axis) rows + |axis| as the kernel receives them */
void cylinder_frame_for(const ort_cylinder &c, float rot[9], float *len);

} // namespace ort

struct ort_scene : public ort::Scene {};
struct ort_comm; /* = ort::Comm behind the C ABI */

#endif
