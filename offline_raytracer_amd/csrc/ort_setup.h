/*
 * ort_setup.h -- what the host works out from a committed scene before a kernel can run, as plain functions of their
 * inputs: the layout and the image of the small LDS tables, the PrimInfo array, the shape table of the ray queries (the inverse
 * of the tree's slot maps), what raycast_needs_exact reads, the camera table of a batch of views, and every field of a call's
 * RenderView that is not a pointer.  No HIP in here: ort_kernels.hip calls these and keeps the uploads and launches; tools/host_sim.cpp calls the
 * same functions to run the lane code on host threads, so the CPU tests exercise the product's own tables and launch set-up
 * (tests/test_query_lanes_host.py), and tools/launch_plan prints the fill of a plan (tests/test_launch_plan.py).
 */
#ifndef ORT_SETUP_H
#define ORT_SETUP_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "ort_plan.h"
#include "ort_scene.h"

namespace ort {

/* Small read-only tables every ray touches live in LDS, copied there once per workgroup: ~100 cycles of latency
   instead of a trip to L1 / L2 on the critical path of every ray (the kernel is latency-bound: DESIGN.md).
   Layout in float4 units; a table that does not fit its slot stays in HBM (SceneView::tab_flags). */
constexpr int kTabRoot = 0;                      /* node 0 of the fast tree (4) */
constexpr int kTabPro = 4;                       /* the analytic prologue's shapes: boxes (2 each), spheres (1), cylinders (4) */
constexpr int kTabProCap = 40;
constexpr int kTabLights = kTabPro + kTabProCap; /* light_is_sphere[64] as u32 */
constexpr int kTabLightCap = 64;
constexpr int kTabMats = kTabLights + kTabLightCap / 4; /* DevMaterial records, 5 each */
constexpr int kTabMatCap = 48;
constexpr int kTabTreelet = kTabMats + 5 * kTabMatCap; /* nodes [0, kTreeletNodes) of the fast tree, breadth-first top (ort_tree.cpp) */
constexpr int kTabF4 = kTabTreelet + 4 * (int)kTreeletNodes; /* 428 float4 = 6848 B */
enum : uint32_t { TAB_PRO = 1u, TAB_LIGHTS = 2u, TAB_MATS = 8u };

static_assert(kPlanAllTabs == (TAB_PRO | TAB_LIGHTS | TAB_MATS) && kPlanTabPro == TAB_PRO && kPlanTabLights == TAB_LIGHTS && kPlanTabMats == TAB_MATS &&
              kPlanTabMatCap == (uint32_t)kTabMatCap && kPlanTabLightCap == (uint32_t)kTabLightCap && kPlanTabProCap == (uint32_t)kTabProCap,
              "ort_plan.h counts with the table layout's caps");
static_assert(sizeof(F4) == 16 && sizeof(DevNode) == 4 * sizeof(F4) && sizeof(DevBox) == 2 * sizeof(F4) && sizeof(DevSphere) == sizeof(F4) &&
              sizeof(DevCyl) == 4 * sizeof(F4) && sizeof(DevMaterial) == 5 * sizeof(F4), "the table layout counts records in 16-byte units");

/* the materials and the lights' kinds as the kernels read them */
inline std::vector<DevMaterial> dev_materials(const Scene &scene) {
    std::vector<DevMaterial> mats(scene.materials.size());
    for (size_t i = 0; i < mats.size(); ++i) mats[i] = make_dev_material(scene.materials[i]);
    return mats;
}
/* whether no surface material can enter the specular / transmission blocks: the four guards of eval_scattering / pdf_brdf, for
   every material a path can scatter on.  This picks the DIFFUSE kernel flavour.  Every comparison with a NaN is false, so a scene
   whose materials are NaN, inf-diffuse or all-zero (pd_c = ps_c = pt_c = NaN) counts as diffuse-only: the blocks' own guards are
   the same comparisons, and skip them for such a material too (tests/hostile_materials.py) */
inline bool materials_diffuse_only(const std::vector<DevMaterial> &mats) {
    for (size_t i = 1; i < mats.size(); ++i) {
        const DevMaterial &dm = mats[i];
        if (dm.is_light) continue;
        const float ks2 = dm.specular[0] * dm.specular[0] + dm.specular[1] * dm.specular[1] + dm.specular[2] * dm.specular[2];
        const float kt2 = dm.transmission[0] * dm.transmission[0] + dm.transmission[1] * dm.transmission[1] + dm.transmission[2] * dm.transmission[2];
        if (ks2 > 0.0f || kt2 > 0.0f || dm.ps_c > 0.0f || dm.pt_c > 0.0f) return false;
    }
    return true;
}
inline std::vector<uint32_t> light_sphere_flags(const Scene &scene) {
    std::vector<uint32_t> lis(scene.lights.size());
    for (size_t i = 0; i < lis.size(); ++i) lis[i] = (scene.lights[i].type == 1u) ? 1u : 0u;
    return lis;
}

/* the image of the LDS tables (kTabF4 records of 16 bytes): root node, prologue shapes, light flags, materials, the tree's top.
   Returns which tables fit their slot (table_fit_flags); one that does not is left zero and read from its own array */
inline uint32_t pack_lds_tables(const Tree &t, const std::vector<DevMaterial> &mats, const std::vector<uint32_t> &lis, std::vector<F4> &tab) {
    tab.assign((size_t)kTabF4, F4{0, 0, 0, 0});
    const uint32_t flags = table_fit_flags(mats.size(), lis.size(), t.pro_boxes, t.pro_spheres, t.pro_cyls);
    if (!t.nodes.empty()) memcpy(&tab[kTabRoot], &t.nodes[0], sizeof(DevNode));
    {
        /* the top of the fast tree; slots beyond the tree's size are never addressed */
        const size_t nt = t.nodes.size() < (size_t)kTreeletNodes ? t.nodes.size() : (size_t)kTreeletNodes;
        if (nt) memcpy(&tab[kTabTreelet], t.nodes.data(), nt * sizeof(DevNode));
    }
    if (flags & TAB_PRO) {
        F4 *q = &tab[kTabPro];
        if (t.pro_boxes) memcpy(q, t.boxes.data(), (size_t)t.pro_boxes * sizeof(DevBox));
        q += 2u * t.pro_boxes;
        if (t.pro_spheres) memcpy(q, t.spheres.data(), (size_t)t.pro_spheres * sizeof(DevSphere));
        q += t.pro_spheres;
        if (t.pro_cyls) memcpy(q, t.cyls.data(), (size_t)t.pro_cyls * sizeof(DevCyl));
    }
    if ((flags & TAB_LIGHTS) && !lis.empty()) memcpy(&tab[kTabLights], lis.data(), lis.size() * 4u);
    if ((flags & TAB_MATS) && !mats.empty()) memcpy(&tab[kTabMats], mats.data(), mats.size() * sizeof(DevMaterial));
    return flags;
}

/* the PrimInfo array of a committed scene (SceneView::prim_info), triangles | boxes | cylinders | spheres */
inline void build_prim_info(const Tree &t, const RefTree &rt, std::vector<PrimInfo> &out, uint32_t &info_box, uint32_t &info_cyl, uint32_t &info_sphere) {
    info_box = (uint32_t)t.tri_mat.size();
    info_cyl = info_box + (uint32_t)t.box_mat.size();
    info_sphere = info_cyl + (uint32_t)t.cyl_mat.size();
    out.assign((size_t)info_sphere + t.sphere_mat.size(), PrimInfo{0u, 0u});
    auto fill = [&out](uint32_t base, const std::vector<uint32_t> &chain, const std::vector<uint32_t> &mat) {
        for (size_t i = 0; i < mat.size(); ++i) out[base + i] = PrimInfo{i < chain.size() ? chain[i] : 0u, mat[i]};
    };
    fill(0u, rt.tri_chain, t.tri_mat);
    fill(info_box, rt.box_chain, t.box_mat);
    fill(info_cyl, rt.cyl_chain, t.cyl_mat);
    fill(info_sphere, rt.sphere_chain, t.sphere_mat);
}

/* ray queries: the inverse of the tree's slot maps, in PrimInfo order (triangles | boxes | cylinders | spheres; info_* are
   build_prim_info's): slot -> kind << 28 | the shape's index in the scene's own arrays.  False when the maps are no bijection
   onto the shape arrays */
inline bool invert_prim_slots(const Tree &t, uint32_t info_box, uint32_t info_cyl, uint32_t info_sphere, std::vector<uint32_t> &src) {
    const uint32_t none = 0xffffffffu; /* kNoPrim */
    src.assign((size_t)info_sphere + t.spheres.size(), none);
    bool bijective = src.size() == t.tri_slot.size() + t.box_slot.size() + t.cyl_slot.size() + t.sphere_slot.size();
    auto invert = [&](uint32_t kind, uint32_t base, const std::vector<uint32_t> &slot, size_t slots) {
        bijective = bijective && slot.size() == slots && (size_t)base + slots <= src.size();
        for (size_t i = 0; i < slot.size() && bijective; ++i) {
            bijective = slot[i] < slots && src[base + slot[i]] == none && i < 0x10000000u;
            if (bijective) src[base + slot[i]] = (kind << 28) | (uint32_t)i;
        }
    };
    invert(PRIM_TRI, 0u, t.tri_slot, t.tris.size());
    invert(PRIM_BOX, info_box, t.box_slot, t.boxes.size());
    invert(PRIM_CYL, info_cyl, t.cyl_slot, t.cyls.size());
    invert(PRIM_SPHERE, info_sphere, t.sphere_slot, t.spheres.size());
    for (uint32_t v : src) bijective = bijective && v != none;
    return bijective;
}

/* what raycast_needs_exact reads (IO: ort::RaycastIO, ort_lane.h): which kinds of shape the fast tree holds, and the scene's box
   (scene_origin_box) */
template <typename IO>
inline void ray_query_io(const Scene &scene, const float lo[3], const float hi[3], IO *io) {
    io->tree_spheres = scene.tree.spheres.size() > scene.tree.pro_spheres;
    io->tree_quadrics = io->tree_spheres || scene.tree.cyls.size() > scene.tree.pro_cyls;
    io->tree_boxes = scene.tree.boxes.size() > scene.tree.pro_boxes;
    memcpy(io->lo, lo, 3 * sizeof(float));
    memcpy(io->hi, hi, 3 * sizeof(float));
}

/* radiance queries: what radiance_lane reads behind hot.c besides the launch policy (View: ort::RenderView, ort_lane.h -- the one
   definition every kernel unit shares -- or tools/launch_plan's pointer-free FillView) -- the
   job space is one PIXEL-style job per ray; q is the query's ray_query_io with its rays set.  All pointers are the lanes' */
template <typename View, typename IO>
inline void radiance_view(const IO &q, const void *seeds, uint32_t spp, float rr, void *out, void *final_states, View *rv) {
    rv->mode = PLAN_JOBS_PIXEL;
    rv->spp = spp; rv->rr = rr;
    rv->out = (float *)out;
    rv->final_states = (uint32_t *)final_states;
    rv->rays = q.rays;
    rv->seeds = (const uint32_t *)seeds;
    rv->ray_tree_spheres = q.tree_spheres; rv->ray_tree_quadrics = q.tree_quadrics; rv->ray_tree_boxes = q.tree_boxes;
    memcpy(rv->ray_lo, q.lo, sizeof(rv->ray_lo));
    memcpy(rv->ray_hi, q.hi, sizeof(rv->ray_hi));
}

/* adaptive radiance queries: radiance_view with max_spp for spp, then what the stopping rule reads and where a ray's sample
   count and sum of squared luminance go (either may be null) */
template <typename View, typename IO>
inline void radiance_adaptive_view(const IO &q, const void *seeds, const ort_adaptive &ad, float rr, void *out, void *out_spp, void *out_m2,
                                   void *final_states, View *rv) {
    radiance_view(q, seeds, ad.max_spp, rr, out, final_states, rv);
    rv->ad_min_spp = ad.min_spp; rv->ad_check_every = ad.check_every;
    rv->ad_tolerance = ad.tolerance; rv->ad_floor = ad.floor;
    rv->ad_spp = (uint32_t *)out_spp;
    rv->ad_m2 = (float *)out_m2;
}

/* camera renders: everything in the RenderView (View) that is not a pointer -- what the call says and what its plan says
   (plan_render, or plan_pixel_jobs: with a stopping rule ad, RK_ADAPTIVE's).  views: the batch's, null for the scene's own camera and
   p.seed.  A batch of one view of the plain render is the single-frame call with that view's seed (and camera: the caller's to
   set); the lanes of a larger batch, and of every adaptive render, read both from the camera table.  With ad, spp is max_spp and
   seed and chunk stay unset: a job's length is the rule's.  A field the plan leaves at zero stays zero */
template <typename View>
inline void render_view(const ort_render_params &p, const LaunchPlan &pl, const ort_view *views, const ort_adaptive *ad, View *rv) {
    rv->W = p.width; rv->H = p.height;
    rv->x0 = p.x0; rv->y0 = p.y0; rv->x1 = p.x1; rv->y1 = p.y1;
    rv->rr = p.rr;
    if (ad) {
        rv->spp = ad->max_spp;
        rv->ad_min_spp = ad->min_spp; rv->ad_check_every = ad->check_every;
        rv->ad_tolerance = ad->tolerance; rv->ad_floor = ad->floor;
    } else {
        rv->seed = views && !pl.views ? views[0].seed : p.seed; rv->spp = p.spp; rv->chunk = p.chunk;
    }
    rv->packed_out = (p.flags & ORT_RENDER_PACKED) != 0 && pl.mode != PLAN_JOBS_EXPLICIT;
    rv->mode = pl.mode; rv->nchunks = pl.nchunks; rv->job_count = pl.job_count;
    rv->shard_count = pl.blocks.shard_count; rv->shard_index = pl.blocks.shard_index;
    rv->blocks_w = pl.blocks.blocks_w; rv->block_x0 = pl.blocks.block_x0; rv->block_y0 = pl.blocks.block_y0;
    rv->my_blocks = pl.blocks.my_blocks;
    if (pl.views) { rv->view_jobs = pl.view_jobs; rv->view_count = pl.view_count; }
    rv->refill_below = pl.refill_below; rv->descend_below = pl.descend_below;
    rv->capL = pl.capL; rv->capR = pl.capR;
    rv->long_min = pl.long_min; rv->long_refill = pl.long_refill; rv->inflight_cap = pl.inflight_cap; rv->park_min = pl.park_min;
    rv->endgame_from = pl.endgame_from;
    rv->stash_wave_f4 = pl.stash_wave_f4;
    rv->block_major = pl.block_major;
    rv->job_batch = pl.job_batch; rv->batch_until = pl.batch_until;
}

/* first-hit feature renders: what feature_lane reads behind hot.c besides the launch policy and the camera table's pointer -- the
   frame, the rect, the 8x8 blocks under it, spp, and the job space [view][block][pixel in block] (plan_features, ort_plan.h) */
template <typename View>
inline void features_view(const ort_render_params &p, uint32_t view_count, View *rv) {
    const BlockGrid g = block_grid_for(&p);
    rv->mode = PLAN_JOBS_PIXEL;
    rv->W = p.width; rv->H = p.height;
    rv->x0 = p.x0; rv->y0 = p.y0; rv->x1 = p.x1; rv->y1 = p.y1;
    rv->spp = p.spp;
    rv->shard_count = g.shard_count; rv->shard_index = g.shard_index;
    rv->blocks_w = g.blocks_w; rv->block_x0 = g.block_x0; rv->block_y0 = g.block_y0;
    rv->my_blocks = g.my_blocks;
    rv->view_jobs = feature_view_jobs(p); rv->view_count = view_count;
    rv->job_count = rv->view_jobs * view_count;
}

/* feature renders that follow mirrors and glass (follow_lane): features_view, and the roulette's rr, which these lanes read */
template <typename View>
inline void follow_view(const ort_render_params &p, uint32_t view_count, View *rv) {
    features_view(p, view_count, rv);
    rv->rr = p.rr;
}

/* ID-matte renders (matte_lane): features_view as it stands; by and slots travel in the kernels' third argument */
template <typename View>
inline void matte_view(const ort_render_params &p, uint32_t view_count, View *rv) {
    features_view(p, view_count, rv);
}

/* ID-matte renders BY_OBJECT: invert_prim_slots' table with a triangle's word replaced by ORT_HIT_MESH << 28 | its mesh's index.
   A triangle's index in the scene's own arrays is mesh-major, so tri_counts (the triangles of every mesh, in the scene's mesh
   order) names its mesh.  False when a triangle lies beyond the meshes or a mesh index does not fit below bit 28 */
inline bool object_ids_from_prim_src(const std::vector<uint32_t> &src, const std::vector<uint32_t> &tri_counts, std::vector<uint32_t> &obj) {
    std::vector<uint64_t> end(tri_counts.size()); /* end[m]: the first triangle id past mesh m */
    uint64_t sum = 0;
    for (size_t m = 0; m < tri_counts.size(); ++m) end[m] = sum += tri_counts[m];
    obj = src;
    for (uint32_t &w : obj) {
        if ((w >> 28) != PRIM_TRI) continue;
        const size_t m = (size_t)(std::upper_bound(end.begin(), end.end(), (uint64_t)(w & 0x0fffffffu)) - end.begin());
        if (m >= end.size() || m >= 0x10000000u) return false;
        w = (1u /* ORT_HIT_MESH */ << 28) | (uint32_t)m;
    }
    return true;
}
/* ... for a scene: tri_counts from its meshes, as ort_scene_get_mesh orders them */
inline bool object_ids_from_prim_src(const Scene &scene, const std::vector<uint32_t> &src, std::vector<uint32_t> &obj) {
    std::vector<uint32_t> tri_counts;
    for (const HostMesh &m : scene.meshes) tri_counts.push_back((uint32_t)(m.indices.size() / 3));
    return object_ids_from_prim_src(src, tri_counts, obj);
}

/* runtime bools to template arguments: f(std::bool_constant...) with one constant per bool, true first at every level */
template <typename F>
inline void with_bools(F f) { f(); }
template <typename F, typename... Rest>
inline void with_bools(F f, bool b, Rest... rest) {
    if (b) with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

/* the kernels' by-value argument (Hot: ort::RenderHot, ort_lane.h): the few fields of rv every ray reads, and where the lanes find
   the rest -- rv itself on the host, its copy in HBM on the device */
template <typename Hot, typename View>
inline Hot render_hot(const View &rv, const void *where) {
    Hot hot{};
    hot.mode = rv.mode; hot.W = rv.W; hot.H = rv.H; hot.rr = rv.rr;
    hot.refill_below = rv.refill_below; hot.descend_below = rv.descend_below;
    hot.c = (decltype(hot.c))where;
    return hot;
}

/* occlusion queries: no shape of the scene carries material 0 (the early end of occluded_lane) */
inline uint32_t all_mats_nonzero(const Tree &t) {
    for (const std::vector<uint32_t> *m : {&t.tri_mat, &t.box_mat, &t.cyl_mat, &t.sphere_mat})
        for (uint32_t v : *m) if (v == 0u) return 0u;
    return 1u;
}

/* a batch of views: the camera table load_view_camera reads, 4 records of 16 bytes per view: p.xyz and the seed's bits, then
   the three axes */
inline void pack_view_table(const ort_view *views, uint32_t view_count, std::vector<float> &tab) {
    tab.assign((size_t)view_count * 16u, 0.0f);
    for (uint32_t v = 0; v < view_count; ++v) {
        float *q = &tab[(size_t)v * 16u];
        const ort_camera &c = views[v].camera;
        const float rows[4][3] = {{c.p.x, c.p.y, c.p.z}, {c.x_axis.x, c.x_axis.y, c.x_axis.z}, {c.y_axis.x, c.y_axis.y, c.y_axis.z}, {c.z_axis.x, c.z_axis.y, c.z_axis.z}};
        for (int r = 0; r < 4; ++r) memcpy(q + 4 * r, rows[r], sizeof(rows[r]));
        memcpy(q + 3, &views[v].seed, sizeof(uint32_t));
    }
}

} // namespace ort

#endif
