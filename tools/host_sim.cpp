/*
 * tools/host_sim.cpp -- DEVELOPER HARNESS, not part of the product: the kernel's lane code on host threads.
 *
 * The dev container has no GPU.  This tool compiles the kernel's lane function
 * (ort_lane.h: pt_lane) as ordinary host C++ (-DORT_HOST_SIM) and runs one simulated
 * lane per host thread (SIM_THREADS, default 1) over the job space, so kernel logic can be debugged
 * against the oracle before spending GPU-box time.  With policy tile32 and SIM_THREADS = cores it is
 * the Linux counterpart of the reference's own driver: main()'s 1 024 tiles
 * (macos_main.mm:602-662) handed out by one job counter to a pool of worker threads
 * (macos_main.mm:565-598 starts eight pthreads on a work queue), every worker a lane of the
 * kernel.  The library never loads, links or runs it: the render call has no CPU fallback
 * (tests/test_host.py holds its image against the oracle; nothing else uses it).
 *
 * The ray-query lanes (raycast_lane, occluded_lane, ao_lane, radiance_lane with and without its adaptive rule), the batch-of-views flavour of pt_lane, its adaptive one, its light-group one, its sample-map one and its accumulating one run here too, on
 * the tables the product's own host code packs, and the camera modes on the launch plan and RenderView fill of the product's own render call (ort_plan.h, ort_setup.h): tests/test_query_lanes_host.py holds them against the
 * reference's answers and the oracle, tests/test_host_sanitizers.py runs the same binary built with ASan + UBSan
 * (make host_sim_san).
 *
 * build: see tools/Makefile     run: [SIM_THREADS=n] host_sim <scn> <base> W H spp seed policy chunk out.f32
 *   or: host_sim --unit records.bin out.f32   (ort_unit_eval_device on the host)
 *   or: host_sim --raycast scn base rays.f32 hits.bin                        (ort_hit records)
 *   or: host_sim --occluded scn base rays.f32 tmax.f32|- out.u8
 *   or: host_sim --ambient-occlusion scn base points.f32 seeds.u32 radius.f32|- spp open.u32 bent.f32|- states.u32|-   (ao_lane)
 *   or: host_sim --radiance scn base rays.f32 seeds.u32 spp rr out.f32 states.u32
 *   or: host_sim --radiance-adaptive scn base rays.f32 seeds.u32 min_spp max_spp check_every tolerance floor rr out.f32 spp.u32 m2.f32 states.u32
 *   or: host_sim --irradiance scn base points.f32 seeds.u32 spp rr out.f32 states.u32            (points: p, n, 6 floats each)
 *   or: host_sim --irradiance-adaptive scn base points.f32 seeds.u32 min_spp max_spp check_every tolerance floor rr out.f32 spp.u32 m2.f32 states.u32
 *       (the irradiance queries: the two modes above over points, radiance_lane with LF_HEMI)
 *   or: host_sim --probe-sh scn base points.f32 seeds.u32 spp rr sh.f32 out.f32|- states.u32|-      (sh: 27 floats a point)
 *       (the SH light-probe query: --irradiance with LF_SH and one more output file; out and states given as - are not passed)
 *   or: host_sim --views scn base cams.f32 seeds.u32 W H spp policy chunk out.f32   (cams: p, x, y, z axes, 12 floats a view)
 *       (as on the device, one view is the single-frame lane with that view's camera and seed: the VIEWS lanes run from two views on)
 *   or: host_sim --render-adaptive scn base W H x0 y0 x1 y1 seed min_spp max_spp check_every tolerance floor rr out.f32 spp.u32 m2.f32 states.u32
 *       (the adaptive camera render of the scene's own camera: pt_lane with LF_IMPLICIT | LF_VIEWS | LF_ADAPT over a one-view batch; the planes start
 *       at the guard values -7.0f, 0xeeeeeeee, -1.0f, 0xdddddddd, which pixels outside the rect keep)
 *   or: host_sim --features scn base cams.f32|- seeds.u32|seed W H x0 y0 x1 y1 spp albedo.f32|- normal.f32|- depth.f32|- hits.u32|- ids.u32|- states.u32|-
 *   or: host_sim --follow scn base cams.f32|- seeds.u32|seed W H x0 y0 x1 y1 spp rr max_bounces albedo.f32|- normal.f32|- depth.f32|- hits.u32|- ids.u32|- bounces.u32|- states.u32|-
 *       (the feature render that follows mirrors and glass, follow_lane: --features' arguments with rr, the cap and the bounces plane)
 *   or: host_sim --matte scn base cams.f32|- seeds.u32|seed W H x0 y0 x1 y1 spp by slots ids.u32 counts.u32 other.u32|- hits.u32|- states.u32|-
 *       (the ID-matte render, matte_lane: --features' arguments with by -- 0 material, 1 object, 2 prim -- and slots, and the five planes
 *       of ort_render_matte; the planes start at 0xeeeeeeee and, the states, 0xdddddddd)
 *       (the first-hit feature render, feature_lane: a batch of views, or with cams - the scene's own camera on the seed given; a
 *       plane given as - is not passed; the planes start at -7.0f, 0xeeeeeeee and, the states, 0xdddddddd)
 *   or: host_sim --light-groups scn base cams.f32|- seeds.u32|seed W H x0 y0 x1 y1 spp rr groups.u8 G groups.f32 rgb.f32|- states.u32|-
 *       (the light-group render, pt_lane with LF_IMPLICIT | LF_VIEWS | LF_GROUPS: a batch of views, or with cams - the scene's own camera on the seed
 *       given; groups.u8 holds a byte per material of the scene, G is the group count; the planes start at -7.0f and, the states,
 *       0xdddddddd; rgb and states given as - are not passed)
 *   or: host_sim --depths scn base cams.f32|- seeds.u32|seed W H x0 y0 x1 y1 spp rr G bins.f32 rgb.f32|- lengths.u32|- states.u32|-
 *       (the path-depth render, pt_lane<..., VIEWS, DEPTHS>: a batch of views, or with cams - the scene's own camera on the seed
 *       given; G is the bin count; the frames start at -7.0f, the lengths at 0xeeeeeeee and the states at 0xdddddddd; rgb, lengths
 *       and states given as - are not passed)
 *   or: host_sim --sample-map scn base cams.f32|- seeds.u32|seed W H x0 y0 x1 y1 cap rr map.u32 rgb.f32 m2.f32|- states.u32|-
 *       (the sample-map render, pt_lane<..., VIEWS, SPPMAP>: a batch of views, or with cams - the scene's own camera on the seed
 *       given; map.u32 holds views x W x H sample counts, cap is the most a pixel gets; the planes start at -7.0f, the sums at
 *       -1.0f and the states at 0xdddddddd; m2 and states given as - are not passed)
 *   or: host_sim --accumulate scn base cams.f32|- seeds.u32|seed W H x0 y0 x1 y1 cap rr map.u32|- sum.f32 m2.f32|- count.u32 states.u32 rgb.f32|-
 *       (the accumulating render, pt_lane<..., VIEWS, SPPMAP, ACCUM>: as --sample-map, the map given as - is not passed; every
 *       plane file holds views x W x H entries, is READ before the lanes run and WRITTEN after them, so that runs chain; m2 and rgb
 *       given as - are not passed)
 *   or: host_sim --tree-check scn base
 *       (no lane runs: the fast tree, binary and 4-wide, as build_tree made it under the environment's ORT_LEAF_TRI, ORT_LEAF_OTHER,
 *       ORT_TREE_SPLIT_KINDS and ORT_ANALYTIC_PROLOGUE, checked for everything the lanes take for granted -- see TreeCheck; one line
 *       on stdout when it is sound, the first violation on stderr and status 1 when it is not)
 * Every mode prints, per instantiation of traverse, how deep the per-lane stack got ("stack: lds 24 deepest ..."; tests/host_sim_tool.py
 * stack_probe reads it); make host_sim_w5 builds the same tool with the five-waves unit's split of that stack (20 + 44 entries).
 * All files raw little-endian.  SIM_TABS=1: the LF_TABS lane code, on a heap copy of the LDS tables' image.
 */
#define ORT_HOST_SIM 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
static uint32_t *g_pixel_rng; static int g_W;
static int g_dbg_x = -1, g_dbg_y = -1; static FILE *g_ray_log;
#define ORT_SIM_RAY_HOOK(PX_, PY_, O_, D_, T_, N_, M_) do { if ((PX_) == g_dbg_x && (PY_) == g_dbg_y && g_ray_log) { float r_[11] = {O_.x, O_.y, O_.z, D_.x, D_.y, D_.z, T_, N_.x, N_.y, N_.z, 0}; unsigned m_ = (M_); fwrite(r_, 4, 10, g_ray_log); fwrite(&m_, 4, 1, g_ray_log); } } while (0)
/* the stack probe: how deep traverse's per-lane stack gets, per instantiation (its LDS_ENTRIES: the main traversal's kLdsStack, the
   re-traversal's kLdsStack - 4, the wavefront trace's 16 and 12).  Entries from LDS_ENTRIES on are the scratch tail (spill[]).  A
   thread counts for itself and adds its counts to the totals when it is done (probe_flush); print_counters prints the totals */
struct StackProbe { int lds; int deepest; int prev; bool above; unsigned long long rays, rays_above, steps_above, scratch_pops; };
static thread_local StackProbe t_probe[4];
static inline void stack_probe(int lds, int sp, bool fresh) {
    StackProbe *s = t_probe;
    while (s->lds != lds && s->lds != 0 && s != t_probe + 3) ++s;
    s->lds = lds;
    if (fresh) { s->rays++; s->above = false; s->prev = 0; }
    if (sp > lds) { s->steps_above++; if (!s->above) { s->above = true; s->rays_above++; } }
    if (!fresh && sp == s->prev - 1 && sp >= lds) s->scratch_pops++; /* the entry popped, index sp, was in scratch */
    if (sp > s->deepest) s->deepest = sp;
    s->prev = sp;
}
#define ORT_SIM_STACK_HOOK(LDS_, SP_, FRESH_) stack_probe((LDS_), (SP_), (FRESH_))
#define ORT_SIM_PIXEL_HOOK(x, y, rng) do { if (g_pixel_rng) g_pixel_rng[(y) * g_W + (x)] = (rng); } while (0)
#include "../offline_raytracer_amd/csrc/ort_lane.h"

#include <float.h>
#include <stdarg.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <thread>

using namespace ort;
#ifdef ORT_CHAIN_STATS
namespace ort { unsigned long long g_cs[4][16]; }
static void cs_dump() { static const char *nm[4] = {"chain len:", "first-outside depth from top (15 = none):", "re-cast reasons [1 phantom first, 2 unknown + hit in gap, 6 unknown + phantom in gap, 3 reject + phantom, 4 reject + second verdict]:", "first verdict [0 reject, 1 unknown; 4 + kind of W]:"};
    for (int k = 0; k < 4; ++k) { fprintf(stderr, "%s", nm[k]); for (int i = 0; i < 16; ++i) fprintf(stderr, " %llu", g_cs[k][i]); fprintf(stderr, "\n"); } }
#endif

/* --unit IN OUT: the per-function records of ort_unit_eval_device ({u32 op; f32 in[24]} -> f32 out[8]) through the lane
   code's own dispatch (unit_eval_op), compiled for the host; op 4's frame is filled in as ort_unit_eval_device does */
static int unit_mode(const char *in_path, const char *out_path) {
    FILE *f = fopen(in_path, "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", in_path); return 1; }
    std::vector<unsigned char> rec;
    unsigned char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) rec.insert(rec.end(), buf, buf + got);
    fclose(f);
    if (rec.size() % 100u) { fprintf(stderr, "%s: not a whole number of 100-byte records\n", in_path); return 1; }
    const size_t n = rec.size() / 100u;
    std::vector<float> out(8 * n);
    for (size_t i = 0; i < n; ++i) {
        uint32_t op;
        float a[24];
        memcpy(&op, &rec[100 * i], 4);
        memcpy(a, &rec[100 * i + 4], 96);
        if (op == 4u) {
            ort_cylinder c{{a[0], a[1], a[2]}, {a[3], a[4], a[5]}, a[6], 0};
            cylinder_frame_for(c, a + 13, a + 22);
        }
        unit_eval_op(op, a, &out[8 * i]);
    }
    FILE *g = fopen(out_path, "wb");
    if (!g || fwrite(out.data(), 4, out.size(), g) != out.size()) { fprintf(stderr, "cannot write %s\n", out_path); return 1; }
    fclose(g);
    return 0;
}

static bool read_bytes(const char *path, std::vector<unsigned char> &out) {
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", path); return false; }
    unsigned char buf[1 << 16];
    size_t got;
    out.clear();
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + got);
    fclose(f);
    return true;
}
static bool write_bytes(const char *path, const void *p, size_t bytes) {
    FILE *f = fopen(path, "wb");
    const bool ok = f && (bytes == 0 || fwrite(p, 1, bytes, f) == bytes);
    if (f) fclose(f);
    if (!ok) fprintf(stderr, "cannot write %s\n", path);
    return ok;
}

/* a committed scene as the lanes see it: what device_upload builds, in host memory, through the same functions (ort_setup.h) */
struct Sim {
    ort_scene *scene = nullptr;
    SceneView sv{};
    SceneCold cold{};
    std::vector<DevMaterial> mats;
    std::vector<uint32_t> lis;
    std::vector<PrimInfo> prim_info;
    uint32_t tab_flags = 0;
    float4 *tab = nullptr; /* SIM_TABS: exactly kTabF4 float4 on the heap, so that a read past a slot's end is a read past the block */
    unsigned long long ctrl[128] = {0}; /* as DeviceScene::ctrl_buf: [0] next_job, [1..5] counters, [6..7] fallback, diagnostics up to [6 + kDiagFallback + 2] */
    int n_threads = 1;
    ~Sim() { delete[] tab; if (scene) ort_scene_destroy(scene); }
};

/* need: the tables the mode's TABS kernel keeps in LDS (all three for the path tracers, TAB_PRO for the ray queries) */
static int sim_open(Sim &S, const char *scn, const char *base, uint32_t need) {
    if (ort_scene_load_scn(scn, base, &S.scene) != ORT_OK || ort_scene_commit(S.scene) != ORT_OK) {
        fprintf(stderr, "scene: %s\n", ort_last_error());
        return 1;
    }
    const Tree &t = S.scene->tree;
    const RefTree &rt = S.scene->ref;
    ort_tree_info ti;
    ort_scene_get_tree_info(S.scene, &ti);
    fprintf(stderr, "tree: %u nodes, %u leaves, max leaf %u, depth %u, sah %.2f\n", ti.node_count, ti.leaf_count, ti.max_leaf_prims, ti.max_depth, ti.sah_cost);
    S.mats = dev_materials(*S.scene);
    fprintf(stderr, "materials: %zu, diffuse_only %d\n", S.mats.size(), (int)materials_diffuse_only(S.mats)); /* the flavour an upload picks */
    fprintf(stderr, "shapes: mats_nonzero %u\n", all_mats_nonzero(t)); /* whether the occlusion lanes may take their early end */
    S.lis = light_sphere_flags(*S.scene);
    SceneView &sv = S.sv;
    sv.nodes = (const float4 *)t.nodes.data(); sv.tris = (const float4 *)t.tris.data();
    sv.spheres = (const float4 *)t.spheres.data(); sv.boxes = (const float4 *)t.boxes.data(); sv.cyls = (const float4 *)t.cyls.data();
    build_prim_info(t, rt, S.prim_info, sv.info_box, sv.info_cyl, sv.info_sphere);
    sv.prim_info = S.prim_info.data();
    sv.materials = (const float4 *)S.mats.data();
    sv.light_is_sphere = S.lis.data(); sv.light_count = (uint32_t)S.lis.size();
    sv.pro_boxes = t.pro_boxes; sv.pro_spheres = t.pro_spheres; sv.pro_cyls = t.pro_cyls;
    {
        std::vector<F4> img;
        S.tab_flags = pack_lds_tables(t, S.mats, S.lis, img);
        sv.tab_flags = S.tab_flags;
        if (getenv("SIM_TABS") && atoi(getenv("SIM_TABS"))) {
            if ((S.tab_flags & need) != need) {
                fprintf(stderr, "SIM_TABS: the scene's tables do not fit their LDS slots (fit flags %u, needed %u)\n", S.tab_flags, need);
                return 1;
            }
            S.tab = new float4[kTabF4];
            memcpy(S.tab, img.data(), (size_t)kTabF4 * sizeof(float4));
            sv.tab_src = S.tab;
        }
    }
    sv.cold = &S.cold;
    S.cold.ref_nodes = (const float4 *)rt.nodes.data(); S.cold.ref_recs = rt.recs.data(); sv.chain_boxes = (const float4 *)rt.chain_boxes.data();
    S.cold.tri_order = rt.tri_order.data(); S.cold.sphere_order = rt.sphere_order.data(); S.cold.box_order = rt.box_order.data(); S.cold.cyl_order = rt.cyl_order.data();
    S.cold.fallback_counters = S.ctrl + 6;
    fprintf(stderr, "ref octree: %zu nodes, %u leaves, max leaf %u, chain boxes %zu\n", rt.nodes.size(), rt.nonempty_leaves, rt.max_leaf_records, rt.chain_boxes.size() / 2);
    sv.force_fallback_mask = getenv("SIM_FORCE_FALLBACK") ? (uint32_t)strtoul(getenv("SIM_FORCE_FALLBACK"), 0, 0) : 0xffffffffu;
    S.n_threads = getenv("SIM_THREADS") ? std::max(1, atoi(getenv("SIM_THREADS"))) : 1;
    return 0;
}

static StackProbe g_probe[4];
static std::mutex g_probe_lock;
static void probe_flush() {
    std::lock_guard<std::mutex> hold(g_probe_lock);
    for (StackProbe &t : t_probe) {
        if (!t.lds) continue;
        StackProbe *g = g_probe;
        while (g->lds != t.lds && g->lds != 0 && g != g_probe + 3) ++g;
        g->lds = t.lds;
        g->deepest = std::max(g->deepest, t.deepest);
        g->rays += t.rays; g->rays_above += t.rays_above; g->steps_above += t.steps_above; g->scratch_pops += t.scratch_pops;
        t = StackProbe{};
    }
}

/* a pool of workers on one job counter: every worker owns what a GPU lane owns (traversal stack, focal-point cache, its
   queue of the exact fallback), shares what the lanes share (scene, tables, job counter, work counters, outputs) */
template <typename Fn>
static void run_lanes(const Sim &S, Fn lane) {
    auto worker = [&](int w) {
        SceneView svw = S.sv;
        SceneCold coldw = S.cold;
        std::vector<uint32_t> q(S.scene->ref.nodes.size() + 8), lock(1, 0u), stack(kLdsStack * kBlock);
        std::vector<float> focal(4 * kBlock); /* the fourth row: the path-depth render's depth word */
        coldw.bfs_pool = q.data(); coldw.bfs_locks = lock.data(); coldw.bfs_queue_cap = (uint32_t)q.size(); coldw.bfs_queue_count = 1;
        svw.cold = &coldw;
        lane(svw, stack.data(), focal.data(), (uint32_t)w);
        probe_flush();
    };
    if (S.n_threads <= 1) { worker(0); return; }
    std::vector<std::thread> pool;
    for (int w = 0; w < S.n_threads; ++w) pool.emplace_back(worker, w);
    for (auto &th : pool) th.join();
}

static void print_counters(const Sim &S, double sec, const char *tail = "") {
    const unsigned long long *c = S.ctrl;
    probe_flush();
    std::sort(g_probe, g_probe + 4, [](const StackProbe &a, const StackProbe &b) { return a.lds > b.lds; });
    for (const StackProbe &g : g_probe)
        if (g.lds) fprintf(stderr, "stack: lds %d deepest %d traversals %llu above %llu steps_above %llu scratch_pops %llu\n", g.lds, g.deepest, g.rays, g.rays_above, g.steps_above, g.scratch_pops);
    fprintf(stderr, "sim: %.2fs paths %llu rays %llu node_tests %llu tri_tests %llu analytic %llu fallback %llu overflow %llu%s\n", sec, c[1], c[2], c[3], c[4], c[5], c[6], c[7], tail);
}

/* the rays of a query: count x 6 floats, as 8-byte words (the lanes read them as three float2) */
static bool read_rays(const char *path, std::vector<float2> &rays, size_t *count) {
    std::vector<unsigned char> b;
    if (!read_bytes(path, b)) return false;
    if (b.size() % 24u) { fprintf(stderr, "%s: not a whole number of 24-byte rays\n", path); return false; }
    *count = b.size() / 24u;
    rays.resize(3 * *count); /* exactly: a read of ray `count` is a read past the block */
    if (!b.empty()) memcpy(rays.data(), b.data(), b.size());
    return true;
}
template <typename T>
static bool read_array(const char *path, std::vector<T> &v, size_t want, const char *what) {
    std::vector<unsigned char> b;
    if (!read_bytes(path, b)) return false;
    if (b.size() != want * sizeof(T)) { fprintf(stderr, "%s: %zu bytes, expected %zu %s\n", path, b.size(), want, what); return false; }
    v.resize(want);
    if (!b.empty()) memcpy(v.data(), b.data(), b.size());
    return true;
}

/* the job space and thresholds launch_query (ort_kernels.hip) takes from its plan, chosen here for one simulated lane per
   thread: no batches */
static RenderHot query_hot(Sim &S, RenderView &rv, size_t count) {
    rv.job_count = count;
    rv.next_job = S.ctrl;
    rv.counters = S.ctrl + 1;
    rv.refill_below = 32;
    rv.descend_below = getenv("SIM_DESCEND_BELOW") ? atoi(getenv("SIM_DESCEND_BELOW")) : 8;
    return render_hot<RenderHot>(rv, &rv);
}

/* what the ray queries' lanes ask of the scene (ray_query_io, ort_setup.h), and the caller's rays or points */
static RaycastIO sim_query_io(const Sim &S, const float2 *rays = nullptr) {
    float lo[3], hi[3];
    scene_origin_box(*S.scene, lo, hi);
    RaycastIO q{};
    ray_query_io(*S.scene, lo, hi, &q);
    q.rays = rays;
    return q;
}

static int raycast_mode(char **a) { /* scn base rays.f32 hits.bin */
    Sim S;
    if (int rc = sim_open(S, a[0], a[1], TAB_PRO)) return rc;
    size_t n = 0;
    std::vector<float2> rays;
    if (!read_rays(a[2], rays, &n)) return 1;
    std::vector<uint2> hits(3 * n);
    std::vector<uint32_t> src;
    if (!invert_prim_slots(S.scene->tree, S.sv.info_box, S.sv.info_cyl, S.sv.info_sphere, src)) { fprintf(stderr, "the tree's slot maps are not a bijection onto its shape arrays\n"); return 1; }
    RaycastIO io = sim_query_io(S, rays.data());
    io.hits = hits.data(); io.prim_src = src.data();
    RenderView rv{};
    const RenderHot hot = query_hot(S, rv, n);
    auto t0 = std::chrono::steady_clock::now();
    run_lanes(S, [&](const SceneView &sv, uint32_t *stack, float *, uint32_t w) {
        with_bools([&](auto T) { raycast_lane<LF_COUNTERS | lf_if(decltype(T)::value, LF_TABS)>(sv, hot, io, S.tab, stack, 0, w, nullptr); }, S.tab != nullptr);
    });
    print_counters(S, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    static_assert(sizeof(ort_hit) == 3 * sizeof(uint2), "ort_hit is three 8-byte words");
    return write_bytes(a[3], hits.data(), n * sizeof(ort_hit)) ? 0 : 1;
}

static int occluded_mode(char **a) { /* scn base rays.f32 tmax.f32|- out.u8 */
    Sim S;
    if (int rc = sim_open(S, a[0], a[1], TAB_PRO)) return rc;
    size_t n = 0;
    std::vector<float2> rays;
    if (!read_rays(a[2], rays, &n)) return 1;
    std::vector<float> tmax;
    const bool limits = std::string(a[3]) != "-";
    if (limits && !read_array(a[3], tmax, n, "limits")) return 1;
    std::vector<uint8_t> out(n, (uint8_t)0xee); /* every byte is written: one that is not stays neither 0 nor 1 */
    OccludedIO io{};
    io.q = sim_query_io(S, rays.data());
    io.tmax = limits ? tmax.data() : nullptr;
    io.out = out.data();
    io.mats_nonzero = all_mats_nonzero(S.scene->tree);
    RenderView rv{};
    const RenderHot hot = query_hot(S, rv, n);
    auto t0 = std::chrono::steady_clock::now();
    run_lanes(S, [&](const SceneView &sv, uint32_t *stack, float *, uint32_t w) {
        with_bools([&](auto T) { occluded_lane<LF_COUNTERS | lf_if(decltype(T)::value, LF_TABS)>(sv, hot, io, S.tab, stack, 0, w, nullptr); }, S.tab != nullptr);
    });
    print_counters(S, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return write_bytes(a[4], out.data(), n) ? 0 : 1;
}

/* the ambient-occlusion query's lanes (ao_lane); an output given as - is an optional array the caller did not pass */
static int ao_mode(char **a) { /* scn base points.f32 seeds.u32 radius.f32|- spp open.u32 bent.f32|- states.u32|- */
    Sim S;
    if (int rc = sim_open(S, a[0], a[1], TAB_PRO)) return rc;
    size_t n = 0;
    std::vector<float2> points;
    std::vector<uint32_t> seeds;
    if (!read_rays(a[2], points, &n) || !read_array(a[3], seeds, n, "seeds")) return 1;
    std::vector<float> radius;
    const bool limits = std::string(a[4]) != "-", want_bent = std::string(a[7]) != "-", want_states = std::string(a[8]) != "-";
    if (limits && !read_array(a[4], radius, n, "radii")) return 1;
    const uint32_t spp = (uint32_t)strtoul(a[5], 0, 10);
    if (spp == 0u) { fprintf(stderr, "spp must be >= 1\n"); return 1; }
    std::vector<uint32_t> open(n, 0xeeeeeeeeu), states(want_states ? n : 0, 0xddddddddu); /* every word is written: one that is not keeps its filler */
    std::vector<float> bent(want_bent ? 3 * n : 0, -7.0f);
    AoIO io{};
    io.q = sim_query_io(S, points.data());
    io.seeds = seeds.data();
    io.radius = limits ? radius.data() : nullptr;
    io.open = open.data();
    io.bent = want_bent ? bent.data() : nullptr;
    io.states = want_states ? states.data() : nullptr;
    io.spp = spp;
    io.mats_nonzero = all_mats_nonzero(S.scene->tree);
    RenderView rv{};
    const RenderHot hot = query_hot(S, rv, n);
    auto t0 = std::chrono::steady_clock::now();
    run_lanes(S, [&](const SceneView &sv, uint32_t *stack, float *, uint32_t w) {
        std::vector<float> job((kAoCacheWords - 1) * kBlock + 1); /* exactly: a word beyond the lane's six is a write past the block */
        with_bools([&](auto T) { ao_lane<LF_COUNTERS | lf_if(decltype(T)::value, LF_TABS)>(sv, hot, io, S.tab, stack, job.data(), 0, w, nullptr); }, S.tab != nullptr);
    });
    print_counters(S, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return write_bytes(a[6], open.data(), 4 * n) && (!want_bent || write_bytes(a[7], bent.data(), 12 * n)) &&
           (!want_states || write_bytes(a[8], states.data(), 4 * n)) ? 0 : 1;
}

/* HEMI: the irradiance query's lanes (--irradiance): the rays file holds points */
template <bool HEMI>
static int radiance_mode(char **a) { /* scn base rays.f32 seeds.u32 spp rr out.f32 states.u32 */
    Sim S;
    if (int rc = sim_open(S, a[0], a[1], TAB_PRO | TAB_LIGHTS | TAB_MATS)) return rc;
    size_t n = 0;
    std::vector<float2> rays;
    std::vector<uint32_t> seeds;
    if (!read_rays(a[2], rays, &n) || !read_array(a[3], seeds, n, "seeds")) return 1;
    std::vector<float> out(3 * n, 0.0f);
    std::vector<uint32_t> states(n, 0u);
    const RaycastIO q = sim_query_io(S, rays.data());
    RenderView rv{};
    radiance_view(q, seeds.data(), (uint32_t)strtoul(a[4], 0, 10), (float)atof(a[5]), out.data(), states.data(), &rv);
    const RenderHot hot = query_hot(S, rv, n);
    const bool diffuse_only = getenv("SIM_DIFFUSE") != nullptr; /* caller vouches for Ks = Kt = 0 */
    auto t0 = std::chrono::steady_clock::now();
    run_lanes(S, [&](const SceneView &sv, uint32_t *stack, float *, uint32_t w) {
        with_bools([&](auto D, auto T) {
            radiance_lane<LF_COUNTERS | lf_if(decltype(D)::value, LF_DIFFUSE) | lf_if(decltype(T)::value, LF_TABS) | lf_if(HEMI, LF_HEMI)>(sv, hot, S.tab, stack, 0, w, nullptr);
        }, diffuse_only, S.tab != nullptr);
    });
    print_counters(S, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return write_bytes(a[6], out.data(), 12 * n) && write_bytes(a[7], states.data(), 4 * n) ? 0 : 1;
}

/* the SH light-probe query's lanes (--probe-sh): radiance_lane with LF_HEMI | LF_SH; the lane's direction words are the worker's
   focal cache, as the camera lanes use it */
static int probe_sh_mode(char **a) { /* scn base points.f32 seeds.u32 spp rr sh.f32 out.f32|- states.u32|- */
    Sim S;
    if (int rc = sim_open(S, a[0], a[1], TAB_PRO | TAB_LIGHTS | TAB_MATS)) return rc;
    size_t n = 0;
    std::vector<float2> points;
    std::vector<uint32_t> seeds;
    if (!read_rays(a[2], points, &n) || !read_array(a[3], seeds, n, "seeds")) return 1;
    const bool want_out = std::string(a[7]) != "-", want_states = std::string(a[8]) != "-";
    std::vector<float> sh(27 * n, -7.0f), out(want_out ? 3 * n : 0, -7.0f); /* every word is written: one that is not keeps its filler */
    std::vector<uint32_t> states(want_states ? n : 0, 0xddddddddu);
    const RaycastIO q = sim_query_io(S, points.data());
    RenderView rv{};
    radiance_view(q, seeds.data(), (uint32_t)strtoul(a[4], 0, 10), (float)atof(a[5]), want_out ? out.data() : nullptr, want_states ? states.data() : nullptr, &rv);
    rv.sh_out = sh.data();
    const RenderHot hot = query_hot(S, rv, n);
    const bool diffuse_only = getenv("SIM_DIFFUSE") != nullptr; /* caller vouches for Ks = Kt = 0 */
    auto t0 = std::chrono::steady_clock::now();
    run_lanes(S, [&](const SceneView &sv, uint32_t *stack, float *focal, uint32_t w) {
        with_bools([&](auto D, auto T) {
            radiance_lane<LF_COUNTERS | lf_if(decltype(D)::value, LF_DIFFUSE) | lf_if(decltype(T)::value, LF_TABS) | LF_HEMI | LF_SH>(sv, hot, S.tab, stack, 0, w, nullptr, focal);
        }, diffuse_only, S.tab != nullptr);
    });
    print_counters(S, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return write_bytes(a[6], sh.data(), 108 * n) && (!want_out || write_bytes(a[7], out.data(), 12 * n)) &&
           (!want_states || write_bytes(a[8], states.data(), 4 * n)) ? 0 : 1;
}

/* the adaptive query: radiance_lane with LF_ADAPT; tolerance and floor are read as float bits when written 0x........ (a test can
   pass any float exactly), as decimals otherwise */
static float float_arg(const char *s) {
    if (s[0] == '0' && (s[1] == 'x' || s[1] == 'X')) { const uint32_t b = (uint32_t)strtoul(s, 0, 16); float f; memcpy(&f, &b, 4); return f; }
    return (float)atof(s);
}
template <bool HEMI> /* as radiance_mode's */
static int radiance_adaptive_mode(char **a) { /* scn base rays.f32 seeds.u32 min_spp max_spp check_every tolerance floor rr out.f32 spp.u32 m2.f32 states.u32 */
    Sim S;
    if (int rc = sim_open(S, a[0], a[1], TAB_PRO | TAB_LIGHTS | TAB_MATS)) return rc;
    size_t n = 0;
    std::vector<float2> rays;
    std::vector<uint32_t> seeds;
    if (!read_rays(a[2], rays, &n) || !read_array(a[3], seeds, n, "seeds")) return 1;
    ort_adaptive ad{(uint32_t)strtoul(a[4], 0, 10), (uint32_t)strtoul(a[5], 0, 10), (uint32_t)strtoul(a[6], 0, 10), float_arg(a[7]), float_arg(a[8])};
    if (ad.min_spp < 2u || ad.max_spp < ad.min_spp || ad.max_spp > (1u << 24) || ad.check_every == 0u) { fprintf(stderr, "bad adaptive parameters\n"); return 1; }
    std::vector<float> out(3 * n, 0.0f), m2(n, -1.0f);
    std::vector<uint32_t> spp(n, 0xeeeeeeeeu), states(n, 0u); /* every word is written: one that is not keeps its filler */
    const RaycastIO q = sim_query_io(S, rays.data());
    RenderView rv{};
    radiance_adaptive_view(q, seeds.data(), ad, (float)atof(a[9]), out.data(), spp.data(), m2.data(), states.data(), &rv);
    const RenderHot hot = query_hot(S, rv, n);
    const bool diffuse_only = getenv("SIM_DIFFUSE") != nullptr; /* caller vouches for Ks = Kt = 0 */
    auto t0 = std::chrono::steady_clock::now();
    run_lanes(S, [&](const SceneView &sv, uint32_t *stack, float *, uint32_t w) {
        with_bools([&](auto D, auto T) {
            radiance_lane<LF_COUNTERS | lf_if(decltype(D)::value, LF_DIFFUSE) | lf_if(decltype(T)::value, LF_TABS) | LF_ADAPT | lf_if(HEMI, LF_HEMI)>(sv, hot, S.tab, stack, 0, w, nullptr);
        }, diffuse_only, S.tab != nullptr);
    });
    print_counters(S, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return write_bytes(a[10], out.data(), 12 * n) && write_bytes(a[11], spp.data(), 4 * n) && write_bytes(a[12], m2.data(), 4 * n) &&
           write_bytes(a[13], states.data(), 4 * n) ? 0 : 1;
}

/* The camera modes set their launch up as device_render does: a plan (plan_render, plan_pixel_jobs) and render_view's fill of
   it, for traits the simulation states itself and knobs that keep its schedule -- one simulated lane per thread: no batches, jobs
   in chunk-major order, the plain loop -- whatever the environment says; the modes add their pointers */
static SceneTraits sim_traits(const Sim &S) {
    SceneTraits t;
    t.diffuse_only = getenv("SIM_DIFFUSE") != nullptr; /* caller vouches for Ks = Kt = 0 */
    t.tab_flags = S.tab_flags;
    t.fast_tree_bytes = S.scene->tree.nodes.size() * sizeof(DevNode) + S.scene->tree.tris.size() * sizeof(DevTri);
    t.sah_cost = S.scene->tree.sah_cost;
    t.has_wide = !S.scene->tree.nodes4.empty();
    t.max_blocks = 1;
    return t;
}
static Knobs sim_knobs() {
    Knobs kn;
    kn.refill_below = 12;
    kn.descend_below = getenv("SIM_DESCEND_BELOW") ? atoi(getenv("SIM_DESCEND_BELOW")) : 8;
    kn.job_batch = 0; /* draw_job then never reads batch_until (want < need takes need) */
    kn.exchange = kn.waves5 = kn.wide = kn.lpt = 0;
    return kn;
}
static ort_render_params sim_params(int W, int H, uint32_t spp, uint32_t seed, const std::string &policy, uint32_t chunk) {
    ort_render_params p{};
    p.width = W; p.height = H; p.x1 = W; p.y1 = H;
    p.spp = spp; p.seed = seed; p.chunk = chunk; p.rr = getenv("SIM_RR") ? (float)atof(getenv("SIM_RR")) : 0.8f;
    p.policy = policy == "pixel" ? ORT_POLICY_PIXEL : policy == "chunk" ? ORT_POLICY_CHUNK : ORT_POLICY_WHOLE;
    return p;
}
/* What the camera modes open with: the views and their packed table, and for the modes that take a rect the PIXEL params of it */
struct SimCameras {
    std::vector<ort_view> views;
    uint32_t nv = 0;
    std::vector<float4> view_tab; /* the camera table, 16-byte aligned for the lanes' float4 reads */
    ort_render_params p{};        /* the frame and the rect under the PIXEL policy; spp, rr and the rest are the mode's to set */
    size_t n = 0;                 /* the words of a one-word plane, nv * W * H exactly: an access past a plane's end is one past the block */
};
/* the views of cams.f32 and seeds.u32, and their table */
static bool read_cameras(const char *cams, const char *seeds_path, SimCameras *c) {
    static_assert(sizeof(ort_camera) == 48, "a camera is twelve floats");
    if (cams) {
        std::vector<unsigned char> cb;
        if (!read_bytes(cams, cb)) return false;
        if (cb.empty() || cb.size() % 48u) { fprintf(stderr, "%s: not a whole, positive number of 48-byte cameras\n", cams); return false; }
        std::vector<uint32_t> seeds;
        if (!read_array(seeds_path, seeds, cb.size() / 48u, "seeds")) return false;
        c->views.resize(seeds.size());
        for (size_t v = 0; v < c->views.size(); ++v) { memcpy(&c->views[v].camera, &cb[48u * v], 48); c->views[v].seed = seeds[v]; }
    }
    c->nv = (uint32_t)c->views.size();
    std::vector<float> tab_host;
    pack_view_table(c->views.data(), c->nv, tab_host);
    c->view_tab.resize(4u * c->nv);
    memcpy(c->view_tab.data(), tab_host.data(), tab_host.size() * sizeof(float));
    return true;
}
/* ... of a mode with a rect: frame = W H x0 y0 x1 y1; cams "-" is the single-frame form, the scene's own camera on the seed given
   where the seeds file stands.  S.sv.cam becomes the first view's, unread by the VIEWS lanes */
static bool sim_cameras(Sim &S, const char *cams, const char *seeds, char **frame, SimCameras *c) {
    ort_render_params &p = c->p;
    p.width = atoi(frame[0]); p.height = atoi(frame[1]); p.x0 = atoi(frame[2]); p.y0 = atoi(frame[3]); p.x1 = atoi(frame[4]); p.y1 = atoi(frame[5]);
    p.policy = ORT_POLICY_PIXEL;
    if (p.width <= 0 || p.height <= 0 || p.width > 65535 || p.height > 65535 || p.x0 < 0 || p.y0 < 0 || p.x1 > p.width || p.y1 > p.height || p.x0 >= p.x1 || p.y0 >= p.y1) {
        fprintf(stderr, "bad frame size or rect\n");
        return false;
    }
    const bool own = std::string(cams) == "-";
    if (own) {
        c->views.resize(1);
        camera_basis(*S.scene, p.width, p.height, &c->views[0].camera);
        c->views[0].seed = (uint32_t)strtoul(seeds, 0, 10);
    }
    if (!read_cameras(own ? nullptr : cams, seeds, c)) return false;
    c->n = (size_t)c->nv * p.width * p.height;
    memcpy(S.sv.cam, &c->views[0].camera, sizeof(ort_camera));
    return true;
}

/* the plain loop's lanes over the job space of rv: pt_lane with explicit jobs (no LF_IMPLICIT), and LF_WIDE or LF_VIEWS or
   neither.  SIM_DIFFUSE: the caller vouches for Ks = Kt = 0; the wide lanes run in the all-lobes flavour whatever it says.  TABS =
   false: the small tables are read from their arrays; SIM_TABS: from the packed image */
static void run_pt_lanes(const Sim &S, const RenderHot &hot, bool wide, bool views) {
    run_lanes(S, [&](const SceneView &sv, uint32_t *stack, float *focal, uint32_t w) {
        with_bools([&](auto D, auto T) {
            constexpr uint32_t F = LF_COUNTERS | lf_if(decltype(D)::value, LF_DIFFUSE) | lf_if(decltype(T)::value, LF_TABS);
            if (views) pt_lane<F | LF_VIEWS>(sv, hot, S.tab, stack, focal, 0, w);
            else if (!wide) pt_lane<F>(sv, hot, S.tab, stack, focal, 0, w);
            else if constexpr (!(F & LF_DIFFUSE)) pt_lane<F | LF_WIDE>(sv, hot, S.tab, stack, focal, 0, w);
        }, getenv("SIM_DIFFUSE") != nullptr && !wide, S.tab != nullptr);
    });
}

static int views_mode(char **a) { /* scn base cams.f32 seeds.u32 W H spp policy chunk out.f32 */
    Sim S;
    if (int rc = sim_open(S, a[0], a[1], TAB_PRO | TAB_LIGHTS | TAB_MATS)) return rc;
    SimCameras c; /* no rect, and the policy is the caller's: the views and their table alone */
    if (!read_cameras(a[2], a[3], &c)) return 1;
    const std::vector<ort_view> &views = c.views;
    const uint32_t nv = c.nv;
    const int W = atoi(a[4]), H = atoi(a[5]);
    const uint32_t spp = (uint32_t)strtoul(a[6], 0, 10), chunk = (uint32_t)strtoul(a[8], 0, 10);
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535) { fprintf(stderr, "bad frame size\n"); return 1; }
    const std::string policy = a[7];
    if (policy != "pixel" && policy != "chunk") { fprintf(stderr, "a batch of views renders under the pixel or the chunk policy\n"); return 1; }
    if (policy == "chunk" && (!chunk || spp % chunk)) { fprintf(stderr, "chunk must divide spp\n"); return 1; }
    const ort_render_params p = sim_params(W, H, spp, 0, policy, chunk);
    const LaunchPlan pl = plan_render(sim_traits(S), p, false, 0, false, sim_knobs(), nv);
    ort_camera cam; /* the scene's (unread by the VIEWS lanes), or as on the device the one view's of a batch of one */
    camera_basis(*S.scene, W, H, &cam);
    if (!pl.views) cam = views[0].camera;
    memcpy(S.sv.cam, &cam, sizeof(cam));
    RenderView rv{};
    render_view(p, pl, views.data(), nullptr, &rv);
    std::vector<float> out((size_t)nv * W * H * 3, 0.0f), partial(pl.partial_bytes / sizeof(float), 0.0f);
    rv.out = out.data(); rv.partial = partial.data(); rv.views = c.view_tab.data();
    rv.next_job = S.ctrl; rv.counters = S.ctrl + 1;
    const RenderHot hot = render_hot<RenderHot>(rv, &rv);
    auto t0 = std::chrono::steady_clock::now();
    run_pt_lanes(S, hot, false, pl.views);
    if (rv.mode == JOBS_CHUNK)
        for (uint32_t v = 0; v < nv; ++v)
            for (unsigned long long i = 0; i < (unsigned long long)rv.my_blocks * 64; ++i) combine_pixel(hot, i, v);
    print_counters(S, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return write_bytes(a[9], out.data(), out.size() * sizeof(float)) ? 0 : 1;
}

/* the adaptive camera render (ort_render_adaptive): what device_render sets up for it, for one simulated lane per thread */
static int render_adaptive_mode(char **a) { /* scn base W H x0 y0 x1 y1 seed min_spp max_spp check_every tolerance floor rr out.f32 spp.u32 m2.f32 states.u32 */
    Sim S;
    if (int rc = sim_open(S, a[0], a[1], TAB_PRO | TAB_LIGHTS | TAB_MATS)) return rc;
    SimCameras c; /* no cameras on this command line: the single-frame form */
    if (!sim_cameras(S, "-", a[8], a + 2, &c)) return 1;
    ort_adaptive ad{(uint32_t)strtoul(a[9], 0, 10), (uint32_t)strtoul(a[10], 0, 10), (uint32_t)strtoul(a[11], 0, 10), float_arg(a[12]), float_arg(a[13])};
    if (ad.min_spp < 2u || ad.max_spp < ad.min_spp || ad.max_spp > (1u << 24) || ad.check_every == 0u) { fprintf(stderr, "bad adaptive parameters\n"); return 1; }
    const size_t n = c.n;
    std::vector<float> out(3 * n, -7.0f), m2(n, -1.0f);
    std::vector<uint32_t> spp(n, 0xeeeeeeeeu), states(n, 0xddddddddu);
    ort_render_params &p = c.p;
    p.rr = (float)atof(a[14]);
    RenderView rv{};
    render_view(p, plan_pixel_jobs(RK_ADAPTIVE, sim_traits(S), p, sim_knobs(), 1), c.views.data(), &ad, &rv);
    rv.out = out.data(); rv.ad_spp = spp.data(); rv.ad_m2 = m2.data(); rv.final_states = states.data();
    rv.views = c.view_tab.data();
    rv.next_job = S.ctrl; rv.counters = S.ctrl + 1;
    const RenderHot hot = render_hot<RenderHot>(rv, &rv);
    auto t0 = std::chrono::steady_clock::now();
    run_lanes(S, [&](const SceneView &sv, uint32_t *stack, float *focal, uint32_t w) {
        AdaptState A; /* the lane's own, as pt_adaptive's slot of LDS */
        with_bools([&](auto D, auto T) {
            pt_lane<LF_COUNTERS | lf_if(decltype(D)::value, LF_DIFFUSE) | lf_if(decltype(T)::value, LF_TABS) | LF_IMPLICIT | LF_VIEWS | LF_ADAPT>(sv, hot, S.tab, stack, focal, 0, w, false, nullptr, &A);
        }, getenv("SIM_DIFFUSE") != nullptr, S.tab != nullptr);
    });
    print_counters(S, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return write_bytes(a[15], out.data(), 12 * n) && write_bytes(a[16], spp.data(), 4 * n) && write_bytes(a[17], m2.data(), 4 * n) &&
           write_bytes(a[18], states.data(), 4 * n) ? 0 : 1;
}

/* the light-group render (ort_render_light_groups and its views form): what device_render sets up for it, for one simulated lane
   per thread.  cams - : the single-frame form, the scene's own camera on the seed given where the seeds file stands */
static int light_groups_mode(char **a) { /* scn base cams.f32|- seeds.u32|seed W H x0 y0 x1 y1 spp rr groups.u8 G groups.f32 rgb.f32|- states.u32|- */
    Sim S;
    if (int rc = sim_open(S, a[0], a[1], TAB_PRO | TAB_LIGHTS | TAB_MATS)) return rc;
    SimCameras c;
    if (!sim_cameras(S, a[2], a[3], a + 4, &c)) return 1;
    const uint32_t spp = (uint32_t)strtoul(a[10], 0, 10), G = (uint32_t)strtoul(a[13], 0, 10);
    if (spp == 0u || spp > (1u << 24)) { fprintf(stderr, "spp must be within [1, 1 << 24]\n"); return 1; }
    if (G == 0u || G > ORT_MAX_LIGHT_GROUPS) { fprintf(stderr, "G must be within [1, ORT_MAX_LIGHT_GROUPS]\n"); return 1; }
    std::vector<unsigned char> table;
    if (!read_bytes(a[12], table)) return 1;
    if (table.size() != S.scene->materials.size()) { fprintf(stderr, "%s: %zu bytes, the scene has %zu materials\n", a[12], table.size(), S.scene->materials.size()); return 1; }
    for (size_t m = 0; m < table.size(); ++m)
        if (S.scene->materials[m].is_light && table[m] >= G && table[m] != ORT_NO_LIGHT_GROUP) { fprintf(stderr, "light material %zu names no group\n", m); return 1; }
    const bool want_rgb = std::string(a[15]) != "-", want_states = std::string(a[16]) != "-";
    const size_t n = c.n;
    std::vector<float> groups(3 * n * G, -7.0f), rgb(want_rgb ? 3 * n : 0, -7.0f);
    std::vector<uint32_t> states(want_states ? n : 0, 0xddddddddu);
    ort_render_params &p = c.p;
    p.spp = spp; p.rr = (float)atof(a[11]);
    RenderView rv{};
    render_view(p, plan_pixel_jobs(RK_GROUPS, sim_traits(S), p, sim_knobs(), c.nv), c.views.data(), nullptr, &rv);
    rv.out = want_rgb ? rgb.data() : nullptr; rv.final_states = want_states ? states.data() : nullptr;
    rv.group_of_material = table.data(); rv.group_count = G; rv.group_out = groups.data();
    rv.views = c.view_tab.data();
    rv.next_job = S.ctrl; rv.counters = S.ctrl + 1;
    const RenderHot hot = render_hot<RenderHot>(rv, &rv);
    auto t0 = std::chrono::steady_clock::now();
    run_lanes(S, [&](const SceneView &sv, uint32_t *stack, float *focal, uint32_t w) {
        with_bools([&](auto D, auto T) {
            pt_lane<LF_COUNTERS | lf_if(decltype(D)::value, LF_DIFFUSE) | lf_if(decltype(T)::value, LF_TABS) | LF_IMPLICIT | LF_VIEWS | LF_GROUPS>(sv, hot, S.tab, stack, focal, 0, w);
        }, getenv("SIM_DIFFUSE") != nullptr, S.tab != nullptr);
    });
    print_counters(S, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return write_bytes(a[14], groups.data(), 12 * n * G) && (!want_rgb || write_bytes(a[15], rgb.data(), 12 * n)) &&
           (!want_states || write_bytes(a[16], states.data(), 4 * n)) ? 0 : 1;
}

/* the path-depth render (ort_render_depths and its views form): what device_render sets up for it, for one simulated lane per
   thread.  cams - : the single-frame form, the scene's own camera on the seed given where the seeds file stands */
static int depths_mode(char **a) { /* scn base cams.f32|- seeds.u32|seed W H x0 y0 x1 y1 spp rr G bins.f32 rgb.f32|- lengths.u32|- states.u32|- */
    Sim S;
    if (int rc = sim_open(S, a[0], a[1], TAB_PRO | TAB_LIGHTS | TAB_MATS)) return rc;
    SimCameras c;
    if (!sim_cameras(S, a[2], a[3], a + 4, &c)) return 1;
    const uint32_t spp = (uint32_t)strtoul(a[10], 0, 10), G = (uint32_t)strtoul(a[12], 0, 10);
    if (spp == 0u || spp > (1u << 24)) { fprintf(stderr, "spp must be within [1, 1 << 24]\n"); return 1; }
    if (G == 0u || G > ORT_MAX_DEPTH_BINS) { fprintf(stderr, "G must be within [1, ORT_MAX_DEPTH_BINS]\n"); return 1; }
    const bool want_rgb = std::string(a[14]) != "-", want_len = std::string(a[15]) != "-", want_states = std::string(a[16]) != "-";
    const size_t n = c.n;
    std::vector<float> bins(3 * n * G, -7.0f), rgb(want_rgb ? 3 * n : 0, -7.0f);
    std::vector<uint32_t> lengths(want_len ? n * G : 0, 0xeeeeeeeeu), states(want_states ? n : 0, 0xddddddddu);
    ort_render_params &p = c.p;
    p.spp = spp; p.rr = (float)atof(a[11]);
    RenderView rv{};
    render_view(p, plan_pixel_jobs(RK_DEPTHS, sim_traits(S), p, sim_knobs(), c.nv), c.views.data(), nullptr, &rv);
    rv.out = want_rgb ? rgb.data() : nullptr; rv.final_states = want_states ? states.data() : nullptr;
    rv.depth_bins = G; rv.depth_out = bins.data(); rv.depth_len = want_len ? lengths.data() : nullptr;
    rv.views = c.view_tab.data();
    rv.next_job = S.ctrl; rv.counters = S.ctrl + 1;
    const RenderHot hot = render_hot<RenderHot>(rv, &rv);
    auto t0 = std::chrono::steady_clock::now();
    run_lanes(S, [&](const SceneView &sv, uint32_t *stack, float *focal, uint32_t w) {
        with_bools([&](auto D, auto T) {
            pt_lane<LF_COUNTERS | lf_if(decltype(D)::value, LF_DIFFUSE) | lf_if(decltype(T)::value, LF_TABS) | LF_IMPLICIT | LF_VIEWS | LF_DEPTHS>(sv, hot, S.tab, stack, focal, 0, w);
        }, getenv("SIM_DIFFUSE") != nullptr, S.tab != nullptr);
    });
    print_counters(S, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return write_bytes(a[13], bins.data(), 12 * n * G) && (!want_rgb || write_bytes(a[14], rgb.data(), 12 * n)) &&
           (!want_len || write_bytes(a[15], lengths.data(), 4 * n * G)) && (!want_states || write_bytes(a[16], states.data(), 4 * n)) ? 0 : 1;
}

/* the sample-map render (ort_render_sample_map and its views form): what device_render sets up for it, for one simulated lane
   per thread.  cams - : the single-frame form, the scene's own camera on the seed given where the seeds file stands */
static int sample_map_mode(char **a) { /* scn base cams.f32|- seeds.u32|seed W H x0 y0 x1 y1 cap rr map.u32 rgb.f32 m2.f32|- states.u32|- */
    Sim S;
    if (int rc = sim_open(S, a[0], a[1], TAB_PRO | TAB_LIGHTS | TAB_MATS)) return rc;
    SimCameras c;
    if (!sim_cameras(S, a[2], a[3], a + 4, &c)) return 1;
    const uint32_t cap = (uint32_t)strtoul(a[10], 0, 10);
    if (cap == 0u || cap > (1u << 24)) { fprintf(stderr, "cap must be within [1, 1 << 24]\n"); return 1; }
    const size_t n = c.n;
    std::vector<uint32_t> map;
    if (!read_array(a[12], map, n, "map words (views x W x H)")) return 1;
    const bool want_m2 = std::string(a[14]) != "-", want_states = std::string(a[15]) != "-";
    std::vector<float> rgb(3 * n, -7.0f), m2(want_m2 ? n : 0, -1.0f);
    std::vector<uint32_t> states(want_states ? n : 0, 0xddddddddu);
    ort_render_params &p = c.p;
    p.spp = cap; p.rr = (float)atof(a[11]);
    RenderView rv{};
    render_view(p, plan_pixel_jobs(RK_SAMPLE_MAP, sim_traits(S), p, sim_knobs(), c.nv), c.views.data(), nullptr, &rv);
    rv.out = rgb.data(); rv.ad_m2 = want_m2 ? m2.data() : nullptr; rv.final_states = want_states ? states.data() : nullptr;
    rv.sample_map = map.data();
    rv.views = c.view_tab.data();
    rv.next_job = S.ctrl; rv.counters = S.ctrl + 1;
    const RenderHot hot = render_hot<RenderHot>(rv, &rv);
    auto t0 = std::chrono::steady_clock::now();
    run_lanes(S, [&](const SceneView &sv, uint32_t *stack, float *focal, uint32_t w) {
        AdaptState A; /* the lane's own, as pt_sample_map's slot of LDS */
        with_bools([&](auto D, auto T) {
            pt_lane<LF_COUNTERS | lf_if(decltype(D)::value, LF_DIFFUSE) | lf_if(decltype(T)::value, LF_TABS) | LF_IMPLICIT | LF_VIEWS | LF_SPPMAP>(sv, hot, S.tab, stack, focal, 0, w, false, nullptr, &A);
        }, getenv("SIM_DIFFUSE") != nullptr, S.tab != nullptr);
    });
    print_counters(S, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return write_bytes(a[13], rgb.data(), 12 * n) && (!want_m2 || write_bytes(a[14], m2.data(), 4 * n)) &&
           (!want_states || write_bytes(a[15], states.data(), 4 * n)) ? 0 : 1;
}

/* the accumulating render (ort_render_accumulate and its views form): what device_render sets up for it, for one simulated lane
   per thread.  The planes are the files' words, in and out */
static int accumulate_mode(char **a) { /* scn base cams.f32|- seeds.u32|seed W H x0 y0 x1 y1 cap rr map.u32|- sum.f32 m2.f32|- count.u32 states.u32 rgb.f32|- */
    Sim S;
    if (int rc = sim_open(S, a[0], a[1], TAB_PRO | TAB_LIGHTS | TAB_MATS)) return rc;
    SimCameras c;
    if (!sim_cameras(S, a[2], a[3], a + 4, &c)) return 1;
    const uint32_t cap = (uint32_t)strtoul(a[10], 0, 10);
    if (cap == 0u || cap > (1u << 24)) { fprintf(stderr, "cap must be within [1, 1 << 24]\n"); return 1; }
    const size_t n = c.n;
    const bool want_map = std::string(a[12]) != "-", want_m2 = std::string(a[14]) != "-", want_rgb = std::string(a[17]) != "-";
    std::vector<uint32_t> map, count, states;
    std::vector<float> sum, m2, rgb;
    if (want_map && !read_array(a[12], map, n, "map words (views x W x H)")) return 1;
    if (!read_array(a[13], sum, 3 * n, "sum floats (views x W x H x 3)")) return 1;
    if (want_m2 && !read_array(a[14], m2, n, "m2 floats (views x W x H)")) return 1;
    if (!read_array(a[15], count, n, "count words (views x W x H)")) return 1;
    if (!read_array(a[16], states, n, "state words (views x W x H)")) return 1;
    if (want_rgb && !read_array(a[17], rgb, 3 * n, "rgb floats (views x W x H x 3)")) return 1;
    ort_render_params &p = c.p;
    p.spp = cap; p.rr = (float)atof(a[11]);
    RenderView rv{};
    render_view(p, plan_pixel_jobs(RK_ACCUMULATE, sim_traits(S), p, sim_knobs(), c.nv), c.views.data(), nullptr, &rv);
    rv.out = want_rgb ? rgb.data() : nullptr; rv.ad_m2 = want_m2 ? m2.data() : nullptr;
    rv.sample_map = want_map ? map.data() : nullptr;
    rv.acc_sum = sum.data(); rv.ad_spp = count.data(); rv.final_states = states.data();
    rv.views = c.view_tab.data();
    rv.next_job = S.ctrl; rv.counters = S.ctrl + 1;
    const RenderHot hot = render_hot<RenderHot>(rv, &rv);
    auto t0 = std::chrono::steady_clock::now();
    run_lanes(S, [&](const SceneView &sv, uint32_t *stack, float *focal, uint32_t w) {
        AdaptState A; /* the lane's own, as pt_accumulate's slot of LDS */
        with_bools([&](auto D, auto T) {
            pt_lane<LF_COUNTERS | lf_if(decltype(D)::value, LF_DIFFUSE) | lf_if(decltype(T)::value, LF_TABS) | LF_IMPLICIT | LF_VIEWS | LF_SPPMAP | LF_ACCUM>(sv, hot, S.tab, stack, focal, 0, w, false, nullptr, &A);
        }, getenv("SIM_DIFFUSE") != nullptr, S.tab != nullptr);
    });
    print_counters(S, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return write_bytes(a[13], sum.data(), 12 * n) && (!want_m2 || write_bytes(a[14], m2.data(), 4 * n)) && write_bytes(a[15], count.data(), 4 * n) &&
           write_bytes(a[16], states.data(), 4 * n) && (!want_rgb || write_bytes(a[17], rgb.data(), 12 * n)) ? 0 : 1;
}

/* the first-hit feature render (ort_render_features and its views form): what device_render_features sets up for it, for one
   simulated lane per thread.  cams - : the single-frame form, the scene's own camera on the seed given where the seeds file stands.
   A plane given as - is one the caller did not pass; every word of a plane starts as a filler that a pixel outside the rect keeps */
static int features_mode(char **a) { /* scn base cams.f32|- seeds.u32|seed W H x0 y0 x1 y1 spp albedo.f32|- normal.f32|- depth.f32|- hits.u32|- ids.u32|- states.u32|- */
    Sim S;
    if (int rc = sim_open(S, a[0], a[1], TAB_PRO | TAB_MATS)) return rc;
    SimCameras c;
    if (!sim_cameras(S, a[2], a[3], a + 4, &c)) return 1;
    const uint32_t spp = (uint32_t)strtoul(a[10], 0, 10);
    if (spp == 0u || spp > (1u << 24)) { fprintf(stderr, "spp must be within [1, 1 << 24]\n"); return 1; }
    std::vector<uint32_t> src;
    if (!invert_prim_slots(S.scene->tree, S.sv.info_box, S.sv.info_cyl, S.sv.info_sphere, src)) { fprintf(stderr, "the tree's slot maps are not a bijection onto its shape arrays\n"); return 1; }
    bool want[6];
    for (int k = 0; k < 6; ++k) want[k] = std::string(a[11 + k]) != "-";
    const size_t n = c.n;
    std::vector<float> albedo(want[0] ? 3 * n : 0, -7.0f), normal(want[1] ? 3 * n : 0, -7.0f), depth(want[2] ? n : 0, -7.0f);
    std::vector<uint32_t> hits(want[3] ? n : 0, 0xeeeeeeeeu), ids(want[4] ? 2 * n : 0, 0xeeeeeeeeu), states(want[5] ? n : 0, 0xddddddddu);
    ort_render_params &p = c.p;
    p.spp = spp;
    FeatureIO io{};
    io.q = sim_query_io(S);
    io.q.prim_src = src.data();
    io.albedo = want[0] ? albedo.data() : nullptr; io.normal = want[1] ? normal.data() : nullptr; io.depth = want[2] ? depth.data() : nullptr;
    io.hits = want[3] ? hits.data() : nullptr; io.ids = want[4] ? ids.data() : nullptr; io.states = want[5] ? states.data() : nullptr;
    RenderView rv{};
    features_view(p, c.nv, &rv);
    rv.views = c.view_tab.data();
    const RenderHot hot = query_hot(S, rv, (size_t)rv.job_count);
    auto t0 = std::chrono::steady_clock::now();
    run_lanes(S, [&](const SceneView &sv, uint32_t *stack, float *, uint32_t w) {
        std::vector<float> job((kFeatureCacheWords - 1) * kBlock + 1); /* exactly: a word beyond the lane's seven is a write past the block */
        with_bools([&](auto T) { feature_lane<LF_COUNTERS | lf_if(decltype(T)::value, LF_TABS)>(sv, hot, io, S.tab, stack, job.data(), 0, w, nullptr); }, S.tab != nullptr);
    });
    print_counters(S, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return (!want[0] || write_bytes(a[11], albedo.data(), 12 * n)) && (!want[1] || write_bytes(a[12], normal.data(), 12 * n)) &&
           (!want[2] || write_bytes(a[13], depth.data(), 4 * n)) && (!want[3] || write_bytes(a[14], hits.data(), 4 * n)) &&
           (!want[4] || write_bytes(a[15], ids.data(), 8 * n)) && (!want[5] || write_bytes(a[16], states.data(), 4 * n)) ? 0 : 1;
}

/* the ID-matte render (ort_render_matte and its views form): what device_render_matte sets up for it, for one simulated lane per
   thread; features_mode's arguments with by (0 material, 1 object, 2 prim) and slots behind spp, and the five planes of the call.
   ids and counts are always written; every word of a plane starts as 0xeeeeeeee (the states: 0xdddddddd) */
static int matte_mode(char **a) { /* scn base cams.f32|- seeds.u32|seed W H x0 y0 x1 y1 spp by slots ids.u32 counts.u32 other.u32|- hits.u32|- states.u32|- */
    Sim S;
    if (int rc = sim_open(S, a[0], a[1], TAB_PRO | TAB_MATS)) return rc;
    SimCameras c;
    if (!sim_cameras(S, a[2], a[3], a + 4, &c)) return 1;
    const uint32_t spp = (uint32_t)strtoul(a[10], 0, 10), by = (uint32_t)strtoul(a[11], 0, 10), slots = (uint32_t)strtoul(a[12], 0, 10);
    if (spp == 0u || spp > (1u << 24)) { fprintf(stderr, "spp must be within [1, 1 << 24]\n"); return 1; }
    if (by > ORT_MATTE_BY_PRIM) { fprintf(stderr, "by must be 0 (material), 1 (object) or 2 (prim)\n"); return 1; }
    if (slots == 0u || slots > ORT_MAX_MATTE_SLOTS) { fprintf(stderr, "slots must be within [1, %u]\n", ORT_MAX_MATTE_SLOTS); return 1; }
    if (std::string(a[13]) == "-" || std::string(a[14]) == "-") { fprintf(stderr, "ids and counts are required\n"); return 1; }
    std::vector<uint32_t> src, table;
    if (!invert_prim_slots(S.scene->tree, S.sv.info_box, S.sv.info_cyl, S.sv.info_sphere, src)) { fprintf(stderr, "the tree's slot maps are not a bijection onto its shape arrays\n"); return 1; }
    if (by == ORT_MATTE_BY_OBJECT && !object_ids_from_prim_src(*S.scene, src, table)) { fprintf(stderr, "a triangle lies beyond the scene's meshes\n"); return 1; }
    if (by == ORT_MATTE_BY_PRIM) table = src;
    bool want[3];
    for (int k = 0; k < 3; ++k) want[k] = std::string(a[15 + k]) != "-";
    const size_t n = c.n;
    std::vector<uint32_t> ids(n * slots, 0xeeeeeeeeu), counts(n * slots, 0xeeeeeeeeu), other(want[0] ? n : 0, 0xeeeeeeeeu), hits(want[1] ? n : 0, 0xeeeeeeeeu),
        states(want[2] ? n : 0, 0xddddddddu);
    ort_render_params &p = c.p;
    p.spp = spp;
    MatteIO io{};
    io.q = sim_query_io(S);
    io.q.prim_src = by == ORT_MATTE_BY_MATERIAL ? nullptr : table.data();
    io.ids = ids.data(); io.counts = counts.data();
    io.other = want[0] ? other.data() : nullptr; io.hits = want[1] ? hits.data() : nullptr; io.states = want[2] ? states.data() : nullptr;
    io.by = by; io.slots = slots;
    RenderView rv{};
    matte_view(p, c.nv, &rv);
    rv.views = c.view_tab.data();
    const RenderHot hot = query_hot(S, rv, (size_t)rv.job_count);
    auto t0 = std::chrono::steady_clock::now();
    run_lanes(S, [&](const SceneView &sv, uint32_t *stack, float *, uint32_t w) {
        with_bools([&](auto T) { matte_lane<LF_COUNTERS | lf_if(decltype(T)::value, LF_TABS)>(sv, hot, io, S.tab, stack, 0, w, nullptr); }, S.tab != nullptr);
    });
    print_counters(S, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return write_bytes(a[13], ids.data(), 4 * n * slots) && write_bytes(a[14], counts.data(), 4 * n * slots) && (!want[0] || write_bytes(a[15], other.data(), 4 * n)) &&
           (!want[1] || write_bytes(a[16], hits.data(), 4 * n)) && (!want[2] || write_bytes(a[17], states.data(), 4 * n)) ? 0 : 1;
}

/* the feature render that follows mirrors and glass (ort_render_follow and its views form): what device_render_follow sets up for
   it, for one simulated lane per thread; features_mode's arguments with rr and the cap behind spp and the bounces plane before
   the states */
static int follow_mode(char **a) { /* scn base cams.f32|- seeds.u32|seed W H x0 y0 x1 y1 spp rr max_bounces albedo.f32|- normal.f32|- depth.f32|- hits.u32|- ids.u32|- bounces.u32|- states.u32|- */
    Sim S;
    if (int rc = sim_open(S, a[0], a[1], TAB_PRO | TAB_LIGHTS | TAB_MATS)) return rc;
    SimCameras c;
    if (!sim_cameras(S, a[2], a[3], a + 4, &c)) return 1;
    const uint32_t spp = (uint32_t)strtoul(a[10], 0, 10), cap = (uint32_t)strtoul(a[12], 0, 10);
    if (spp == 0u || spp > (1u << 24)) { fprintf(stderr, "spp must be within [1, 1 << 24]\n"); return 1; }
    if (cap > ORT_MAX_FOLLOW_BOUNCES) { fprintf(stderr, "max_bounces must be within [0, %u]\n", ORT_MAX_FOLLOW_BOUNCES); return 1; }
    std::vector<uint32_t> src;
    if (!invert_prim_slots(S.scene->tree, S.sv.info_box, S.sv.info_cyl, S.sv.info_sphere, src)) { fprintf(stderr, "the tree's slot maps are not a bijection onto its shape arrays\n"); return 1; }
    bool want[7];
    for (int k = 0; k < 7; ++k) want[k] = std::string(a[13 + k]) != "-";
    const size_t n = c.n;
    std::vector<float> albedo(want[0] ? 3 * n : 0, -7.0f), normal(want[1] ? 3 * n : 0, -7.0f), depth(want[2] ? n : 0, -7.0f);
    std::vector<uint32_t> hits(want[3] ? n : 0, 0xeeeeeeeeu), ids(want[4] ? 2 * n : 0, 0xeeeeeeeeu), bounces(want[5] ? n : 0, 0xeeeeeeeeu),
        states(want[6] ? n : 0, 0xddddddddu);
    ort_render_params &p = c.p;
    p.spp = spp; p.rr = (float)atof(a[11]);
    FollowIO io{};
    io.q = sim_query_io(S);
    io.q.prim_src = src.data();
    io.albedo = want[0] ? albedo.data() : nullptr; io.normal = want[1] ? normal.data() : nullptr; io.depth = want[2] ? depth.data() : nullptr;
    io.hits = want[3] ? hits.data() : nullptr; io.ids = want[4] ? ids.data() : nullptr; io.bounces = want[5] ? bounces.data() : nullptr;
    io.states = want[6] ? states.data() : nullptr;
    io.max_bounces = cap;
    RenderView rv{};
    follow_view(p, c.nv, &rv);
    rv.views = c.view_tab.data();
    const RenderHot hot = query_hot(S, rv, (size_t)rv.job_count);
    auto t0 = std::chrono::steady_clock::now();
    run_lanes(S, [&](const SceneView &sv, uint32_t *stack, float *, uint32_t w) {
        std::vector<float> job((kFollowCacheWords - 1) * kBlock + 1); /* exactly: a word beyond the lane's eight is a write past the block */
        with_bools([&](auto T) { follow_lane<LF_COUNTERS | lf_if(decltype(T)::value, LF_TABS)>(sv, hot, io, S.tab, stack, job.data(), 0, w, nullptr); }, S.tab != nullptr);
    });
    print_counters(S, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return (!want[0] || write_bytes(a[13], albedo.data(), 12 * n)) && (!want[1] || write_bytes(a[14], normal.data(), 12 * n)) &&
           (!want[2] || write_bytes(a[15], depth.data(), 4 * n)) && (!want[3] || write_bytes(a[16], hits.data(), 4 * n)) &&
           (!want[4] || write_bytes(a[17], ids.data(), 8 * n)) && (!want[5] || write_bytes(a[18], bounces.data(), 4 * n)) &&
           (!want[6] || write_bytes(a[19], states.data(), 4 * n)) ? 0 : 1;
}

/* --tree-check scn base: the scene committed under the environment's knobs (ORT_LEAF_TRI, ORT_LEAF_OTHER, ORT_TREE_SPLIT_KINDS,
   ORT_ANALYTIC_PROLOGUE), and everything the lanes take for granted about what build_tree hands them, verified from the finished
   arrays alone: nothing of the builder's own bookkeeping is trusted but the scene's source shapes.  The first violation is
   printed and ends the run with status 1; a sound tree prints one line (tests/test_tree_shapes_host.py reads it). */
struct TreeCheck {
    const Scene &sc;
    const Tree &t;
    std::vector<uint32_t> covered[5];      /* per kind code: how many leaves (or the prologue) hold each slot */
    std::vector<double> tight[5];          /* per kind code: 6 doubles a slot, the box of the shape itself */
    std::vector<uint32_t> leaves2, leaves4; /* the leaf words the two walks reach */
    uint32_t max_leaf[5] = {0, 0, 0, 0, 0}, leaf_count = 0, depth = 0, depth4 = 0, root_kinds[2] = {0, 0};
    std::vector<uint8_t> seen2, seen4;
    std::string err;
    struct Sub { double lo[3], hi[3]; bool sphere; uint32_t kinds; };

    explicit TreeCheck(const Scene &s) : sc(s), t(s.tree) {}
    bool fail(const char *fmt, ...) {
        if (!err.empty()) return false;
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        err = buf;
        return false;
    }
    size_t kind_size(uint32_t k) const { return k == PRIM_TRI ? t.tris.size() : k == PRIM_SPHERE ? t.spheres.size() : k == PRIM_BOX ? t.boxes.size() : t.cyls.size(); }
    static const char *kind_name(uint32_t k) { return k == PRIM_TRI ? "triangle" : k == PRIM_SPHERE ? "sphere" : k == PRIM_BOX ? "box" : k == PRIM_CYL ? "cylinder" : "?"; }
    void set_tight(uint32_t k, uint32_t slot, const double lo[3], const double hi[3]) {
        for (int c = 0; c < 3; ++c) { tight[k][6 * (size_t)slot + c] = lo[c]; tight[k][6 * (size_t)slot + 3 + c] = hi[c]; }
    }
    /* the slot tables against the source shapes: a bijection source -> slot, the record at the slot is that shape's, bit for bit */
    bool slots() {
        for (uint32_t k : {(uint32_t)PRIM_TRI, (uint32_t)PRIM_BOX, (uint32_t)PRIM_CYL, (uint32_t)PRIM_SPHERE}) {
            covered[k].assign(kind_size(k), 0u);
            tight[k].assign(6 * kind_size(k), 0.0);
        }
        std::vector<uint8_t> taken;
        auto claim = [&](uint32_t k, const std::vector<uint32_t> &slot, size_t i) {
            if (slot[i] >= kind_size(k)) return fail("%s %zu: slot %u outside the %zu records of its kind", kind_name(k), i, slot[i], kind_size(k));
            if (taken[slot[i]]) return fail("%s %zu: slot %u is taken twice", kind_name(k), i, slot[i]);
            taken[slot[i]] = 1;
            return true;
        };
        size_t n_tri = 0;
        for (const HostMesh &m : sc.meshes) n_tri += m.indices.size() / 3;
        if (t.tri_slot.size() != n_tri || t.tris.size() != n_tri || t.tri_mat.size() != n_tri) return fail("%zu triangles, %zu slots, %zu records", n_tri, t.tri_slot.size(), t.tris.size());
        taken.assign(n_tri, 0);
        size_t g = 0;
        for (const HostMesh &m : sc.meshes)
            for (size_t k = 0; k + 2 < m.indices.size(); k += 3, ++g) {
                if (!claim(PRIM_TRI, t.tri_slot, g)) return false;
                const DevTri &d = t.tris[t.tri_slot[g]];
                const float *v[3] = {&m.vertices[3 * (size_t)m.indices[k]], &m.vertices[3 * (size_t)m.indices[k + 1]], &m.vertices[3 * (size_t)m.indices[k + 2]]};
                if (memcmp(d.v0, v[0], 12) != 0 || t.tri_mat[t.tri_slot[g]] != m.mat) return fail("triangle %zu: the record at slot %u is another triangle's", g, t.tri_slot[g]);
                double lo[3], hi[3];
                for (int c = 0; c < 3; ++c) { lo[c] = std::min({v[0][c], v[1][c], v[2][c]}); hi[c] = std::max({v[0][c], v[1][c], v[2][c]}); }
                set_tight(PRIM_TRI, t.tri_slot[g], lo, hi);
            }
        if (t.sphere_slot.size() != sc.spheres.size() || t.spheres.size() != sc.spheres.size() || t.sphere_mat.size() != sc.spheres.size()) return fail("sphere counts disagree");
        taken.assign(sc.spheres.size(), 0);
        for (size_t i = 0; i < sc.spheres.size(); ++i) {
            if (!claim(PRIM_SPHERE, t.sphere_slot, i)) return false;
            const ort_sphere &s = sc.spheres[i];
            const DevSphere &d = t.spheres[t.sphere_slot[i]];
            const float want[4] = {s.center.x, s.center.y, s.center.z, s.r};
            if (memcmp(&d, want, 16) != 0 || t.sphere_mat[t.sphere_slot[i]] != s.mat) return fail("sphere %zu: the record at slot %u is another sphere's", i, t.sphere_slot[i]);
            double lo[3], hi[3];
            for (int c = 0; c < 3; ++c) { lo[c] = (double)want[c] - fabs((double)s.r); hi[c] = (double)want[c] + fabs((double)s.r); }
            set_tight(PRIM_SPHERE, t.sphere_slot[i], lo, hi);
        }
        if (t.box_slot.size() != sc.boxes.size() || t.boxes.size() != sc.boxes.size() || t.box_mat.size() != sc.boxes.size()) return fail("box counts disagree");
        taken.assign(sc.boxes.size(), 0);
        for (size_t i = 0; i < sc.boxes.size(); ++i) {
            if (!claim(PRIM_BOX, t.box_slot, i)) return false;
            const ort_box &b = sc.boxes[i];
            const DevBox &d = t.boxes[t.box_slot[i]];
            const float mn[3] = {b.min.x, b.min.y, b.min.z}, mx[3] = {b.max.x, b.max.y, b.max.z};
            if (memcmp(d.lo, mn, 12) != 0 || memcmp(d.hi, mx, 12) != 0 || t.box_mat[t.box_slot[i]] != b.mat) return fail("box %zu: the record at slot %u is another box's", i, t.box_slot[i]);
            double lo[3], hi[3];
            for (int c = 0; c < 3; ++c) { lo[c] = std::min(mn[c], mx[c]); hi[c] = std::max(mn[c], mx[c]); }
            set_tight(PRIM_BOX, t.box_slot[i], lo, hi);
        }
        if (t.cyl_slot.size() != sc.cylinders.size() || t.cyls.size() != sc.cylinders.size() || t.cyl_mat.size() != sc.cylinders.size()) return fail("cylinder counts disagree");
        taken.assign(sc.cylinders.size(), 0);
        for (size_t i = 0; i < sc.cylinders.size(); ++i) {
            if (!claim(PRIM_CYL, t.cyl_slot, i)) return false;
            const ort_cylinder &c = sc.cylinders[i];
            const DevCyl &d = t.cyls[t.cyl_slot[i]];
            float rot[9], len;
            cylinder_frame_for(c, rot, &len);
            const float base[3] = {c.base.x, c.base.y, c.base.z};
            if (memcmp(d.base, base, 12) != 0 || memcmp(&d.r, &c.r, 4) != 0 || memcmp(d.rot, rot, 36) != 0 || memcmp(&d.len, &len, 4) != 0 || t.cyl_mat[t.cyl_slot[i]] != c.mat)
                return fail("cylinder %zu: the record at slot %u is another cylinder's", i, t.cyl_slot[i]);
            /* the segment the intersector tests, base .. base + len * a, and a disc of radius r about each end */
            double lo[3], hi[3];
            for (int k = 0; k < 3; ++k) {
                const double a = rot[6 + k], p0 = base[k], p1 = (double)base[k] + (double)len * a, e = fabs((double)c.r) * sqrt(std::max(0.0, 1.0 - a * a));
                lo[k] = std::min(p0, p1) - e; hi[k] = std::max(p0, p1) + e;
            }
            set_tight(PRIM_CYL, t.cyl_slot[i], lo, hi);
        }
        /* the prologue's shapes are the first of their kind's array */
        if (t.pro_boxes > t.boxes.size() || t.pro_spheres > t.spheres.size() || t.pro_cyls > t.cyls.size()) return fail("the prologue is longer than a shape array");
        if (t.analytic_prologue != (t.pro_boxes + t.pro_spheres + t.pro_cyls > 0)) return fail("analytic_prologue disagrees with the prologue's counts");
        for (uint32_t i = 0; i < t.pro_boxes; ++i) covered[PRIM_BOX][i]++;
        for (uint32_t i = 0; i < t.pro_spheres; ++i) covered[PRIM_SPHERE][i]++;
        for (uint32_t i = 0; i < t.pro_cyls; ++i) covered[PRIM_CYL][i]++;
        return true;
    }
    /* a child word and its box -> what lies below it; wide: the word is the 4-wide tree's */
    bool below(uint32_t word, const float lo[3], const float hi[3], uint32_t level, bool wide, Sub *out, const char *where, uint32_t at) {
        for (int c = 0; c < 3; ++c) { out->lo[c] = DBL_MAX; out->hi[c] = -DBL_MAX; }
        out->sphere = false;
        out->kinds = 0;
        if (word & LEAF_BIT) {
            const uint32_t kind = (word >> 28) & 7u, count = ((word >> 24) & 15u) + 1u, first = word & 0x00ffffffu;
            if (kind != PRIM_TRI && kind != PRIM_BOX && kind != PRIM_CYL && kind != PRIM_SPHERE) return fail("%s node %u: leaf word %08x has kind %u", where, at, word, kind);
            if (count < 1u || count > MAX_LEAF_PRIMS) return fail("%s node %u: leaf word %08x holds %u primitives", where, at, word, count);
            if ((size_t)first + count > kind_size(kind)) return fail("%s node %u: leaf %08x runs to %u of %zu %ss", where, at, word, first + count, kind_size(kind), kind_name(kind));
            for (uint32_t i = first; i < first + count; ++i) {
                if (!wide) covered[kind][i]++;
                for (int c = 0; c < 3; ++c) { out->lo[c] = std::min(out->lo[c], tight[kind][6 * (size_t)i + c]); out->hi[c] = std::max(out->hi[c], tight[kind][6 * (size_t)i + 3 + c]); }
            }
            out->sphere = kind == PRIM_SPHERE;
            out->kinds = 1u << kind;
            (wide ? leaves4 : leaves2).push_back(word);
            if (!wide) { leaf_count++; max_leaf[kind] = std::max(max_leaf[kind], count); depth = std::max(depth, level); }
        } else {
            const uint32_t i = word & NODE_INDEX_MASK;
            std::vector<uint8_t> &seen = wide ? seen4 : seen2;
            if (i >= seen.size()) return fail("%s node %u: child index %u of %zu nodes", where, at, i, seen.size());
            if (seen[i]) return fail("%s node %u is reached twice", where, i);
            seen[i] = 1;
            if (!wide) depth = std::max(depth, level);
            else depth4 = std::max(depth4, level + 1u);
            const uint32_t n = wide ? 4u : 2u;
            for (uint32_t k = 0; k < n; ++k) {
                uint32_t cw;
                float clo[3], chi[3];
                if (wide) {
                    const DevNode4 &w = t.nodes4[i];
                    cw = w.child[k];
                    clo[0] = w.lox[k]; clo[1] = w.loy[k]; clo[2] = w.loz[k]; chi[0] = w.hix[k]; chi[1] = w.hiy[k]; chi[2] = w.hiz[k];
                } else {
                    const DevNode &b = t.nodes[i];
                    cw = k ? b.child1 : b.child0;
                    memcpy(clo, k ? b.lo1 : b.lo0, 12); memcpy(chi, k ? b.hi1 : b.hi0, 12);
                }
                if (cw == EMPTY_CHILD) {
                    if (!(clo[0] > chi[0] && clo[1] > chi[1] && clo[2] > chi[2])) return fail("%s node %u: the box of empty child %u is not inverted", where, i, k);
                    continue;
                }
                Sub s;
                if (!below(cw, clo, chi, level + 1u, wide, &s, where, i)) return false;
                for (int c = 0; c < 3; ++c) { out->lo[c] = std::min(out->lo[c], s.lo[c]); out->hi[c] = std::max(out->hi[c], s.hi[c]); }
                out->sphere |= s.sphere;
                out->kinds |= s.kinds;
                if (!wide && i == 0 && level == 0) root_kinds[k] = s.kinds;
            }
            if (out->kinds == 0 && !(i == 0 && level == 0)) return fail("%s node %u has nothing below it", where, i);
            if (((word & SPHERE_BELOW_BIT) != 0) != out->sphere && !(i == 0 && level == 0))
                return fail("%s node %u: child word %08x, SPHERE_BELOW_BIT %s but %s below it", where, at, word, (word & SPHERE_BELOW_BIT) ? "set" : "clear", out->sphere ? "a sphere leaf" : "no sphere leaf");
        }
        if (!(word == 0u && level == 0))
            for (int c = 0; c < 3; ++c)
                if (out->kinds && !((double)lo[c] <= out->lo[c] && (double)hi[c] >= out->hi[c]))
                    return fail("%s node %u: the box of child %08x, [%.9g, %.9g] on axis %d, does not contain what is below it, [%.17g, %.17g]", where, at, word, lo[c], hi[c], c, out->lo[c], out->hi[c]);
        return true;
    }
    /* interior nodes in breadth-first order, children in slot order */
    std::vector<uint32_t> breadth_first(bool wide) const {
        std::vector<uint32_t> order(1, 0u);
        for (size_t h = 0; h < order.size(); ++h)
            for (uint32_t k = 0; k < (wide ? 4u : 2u); ++k) {
                const uint32_t cw = wide ? t.nodes4[order[h]].child[k] : (k ? t.nodes[order[h]].child1 : t.nodes[order[h]].child0);
                if (!(cw & LEAF_BIT)) order.push_back(cw & NODE_INDEX_MASK);
            }
        return order;
    }
    bool run() {
        if (!slots()) return false;
        if (t.nodes.empty()) return fail("no node 0");
        seen2.assign(t.nodes.size(), 0);
        seen4.assign(t.nodes4.size(), 0);
        const float none[3] = {0, 0, 0};
        Sub all;
        if (!below(0u, none, none, 0u, false, &all, "binary", 0u)) return false; /* node 0: no child word points at it, no box holds it */
        for (size_t i = 0; i < seen2.size(); ++i)
            if (!seen2[i]) return fail("binary node %zu is not reached from node 0", i);
        for (uint32_t k : {(uint32_t)PRIM_TRI, (uint32_t)PRIM_BOX, (uint32_t)PRIM_CYL, (uint32_t)PRIM_SPHERE})
            for (size_t i = 0; i < covered[k].size(); ++i)
                if (covered[k][i] != 1u) return fail("%s slot %zu is in %u leaves (the prologue counted as one)", kind_name(k), i, covered[k][i]);
        /* the special roots */
        const DevNode &root = t.nodes[0];
        const bool single = root.child1 == EMPTY_CHILD && root.child0 != EMPTY_CHILD;
        if (root.child0 == EMPTY_CHILD && (root.child1 != EMPTY_CHILD || t.nodes.size() != 1 || leaf_count != 0)) return fail("an empty root with something under it");
        if (single && (!(root.child0 & LEAF_BIT) || t.nodes.size() != 1)) return fail("a root with one child that is not a single leaf");
        if (single) depth = 0; /* the builder counts the leaf where it made it, before it wrapped it in node 0 */
        const char *split_env = getenv("ORT_TREE_SPLIT_KINDS");
        const uint32_t analytic = (1u << PRIM_BOX) | (1u << PRIM_CYL) | (1u << PRIM_SPHERE), tri = 1u << PRIM_TRI;
        if ((!split_env || atoi(split_env) != 0) && (all.kinds & tri) && (all.kinds & analytic)) /* analytic shapes left, triangles right */
            if ((root_kinds[0] & tri) || (root_kinds[1] & analytic)) return fail("the kind-split root has kinds %x left and %x right", root_kinds[0], root_kinds[1]);
        ort_tree_info ti;
        if (ort_scene_get_tree_info(&static_cast<const ort_scene &>(sc), &ti) != ORT_OK) return fail("ort_scene_get_tree_info: %s", ort_last_error());
        const uint32_t biggest = std::max({max_leaf[PRIM_TRI], max_leaf[PRIM_BOX], max_leaf[PRIM_CYL], max_leaf[PRIM_SPHERE]});
        if (depth > kTreeDepthBudget) return fail("depth %u is past the budget of %u", depth, kTreeDepthBudget);
        if (ti.node_count != t.nodes.size() || ti.leaf_count != leaf_count || ti.max_leaf_prims != biggest || ti.max_depth != depth)
            return fail("tree info says %u nodes, %u leaves, max leaf %u, depth %u; the walk finds %zu, %u, %u, %u", ti.node_count, ti.leaf_count, ti.max_leaf_prims, ti.max_depth,
                        t.nodes.size(), leaf_count, biggest, depth);
        /* the top of the tree has the lowest indices, breadth-first */
        const std::vector<uint32_t> bfs = breadth_first(false);
        for (uint32_t k = 0; k < std::min<size_t>(kTreeletNodes, bfs.size()); ++k)
            if (bfs[k] != k) return fail("binary node %u is number %u in breadth-first order: [0, %u) is not the top of the tree", bfs[k], k, kTreeletNodes);
        /* the 4-wide tree (a scene that is all prologue has none: nothing would walk it) */
        if (t.nodes4.empty() && (leaf_count != 0 || ti.wide_node_count != 0 || ti.wide_max_depth != 0)) return fail("no wide tree");
        Sub all4;
        if (!t.nodes4.empty() && !below(0u, none, none, 0u, true, &all4, "wide", 0u)) return false;
        for (size_t i = 0; i < seen4.size(); ++i)
            if (!seen4[i]) return fail("wide node %zu is not reached from node 0", i);
        const std::vector<uint32_t> bfs4 = t.nodes4.empty() ? std::vector<uint32_t>() : breadth_first(true);
        for (uint32_t k = 0; k < bfs4.size(); ++k)
            if (bfs4[k] != k) return fail("wide node %u is number %u in breadth-first order", bfs4[k], k);
        if (ti.wide_node_count != t.nodes4.size() || ti.wide_max_depth != depth4) return fail("tree info says %u wide nodes, depth %u; the walk finds %zu, %u", ti.wide_node_count, ti.wide_max_depth, t.nodes4.size(), depth4);
        std::sort(leaves2.begin(), leaves2.end());
        std::sort(leaves4.begin(), leaves4.end());
        if (leaves2 != leaves4) return fail("the binary tree reaches %zu leaf words, the wide tree %zu, or other ones", leaves2.size(), leaves4.size());
        printf("tree-check ok: nodes %zu leaves %u depth %u wide_nodes %zu wide_depth %u prologue %u max_leaf triangle %u sphere %u box %u cylinder %u\n", t.nodes.size(), leaf_count, depth,
               t.nodes4.size(), depth4, t.pro_boxes + t.pro_spheres + t.pro_cyls, max_leaf[PRIM_TRI], max_leaf[PRIM_SPHERE], max_leaf[PRIM_BOX], max_leaf[PRIM_CYL]);
        /* which source shapes the prologue holds (stderr: the line above is all of stdout); every other shape is in exactly one leaf */
        fprintf(stderr, "prologue: box");
        for (size_t i = 0; i < sc.boxes.size(); ++i) if (t.box_slot[i] < t.pro_boxes) fprintf(stderr, " %zu", i);
        fprintf(stderr, " sphere");
        for (size_t i = 0; i < sc.spheres.size(); ++i) if (t.sphere_slot[i] < t.pro_spheres) fprintf(stderr, " %zu", i);
        fprintf(stderr, " cylinder");
        for (size_t i = 0; i < sc.cylinders.size(); ++i) if (t.cyl_slot[i] < t.pro_cyls) fprintf(stderr, " %zu", i);
        fprintf(stderr, "\n");
        return true;
    }
};

static int tree_check_mode(char **a) { /* scn base */
    ort_scene *scene = nullptr;
    if (ort_scene_load_scn(a[0], a[1], &scene) != ORT_OK || ort_scene_commit(scene) != ORT_OK) {
        fprintf(stderr, "scene: %s\n", ort_last_error());
        if (scene) ort_scene_destroy(scene);
        return 1;
    }
    int rc = 0;
    {
        TreeCheck tc(*scene);
        if (!tc.run()) { fprintf(stderr, "tree-check: %s\n", tc.err.c_str()); rc = 1; }
    }
    ort_scene_destroy(scene);
    return rc;
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (argc == 4 && mode == "--tree-check") return tree_check_mode(argv + 2);
    if (argc == 19 && mode == "--features") return features_mode(argv + 2);
    if (argc == 22 && mode == "--follow") return follow_mode(argv + 2);
    if (argc == 20 && mode == "--matte") return matte_mode(argv + 2);
    if (argc == 4 && mode == "--unit") return unit_mode(argv[2], argv[3]);
    if (argc == 6 && mode == "--raycast") return raycast_mode(argv + 2);
    if (argc == 7 && mode == "--occluded") return occluded_mode(argv + 2);
    if (argc == 11 && mode == "--ambient-occlusion") return ao_mode(argv + 2);
    if (argc == 10 && mode == "--radiance") return radiance_mode<false>(argv + 2);
    if (argc == 16 && mode == "--radiance-adaptive") return radiance_adaptive_mode<false>(argv + 2);
    if (argc == 10 && mode == "--irradiance") return radiance_mode<true>(argv + 2);
    if (argc == 16 && mode == "--irradiance-adaptive") return radiance_adaptive_mode<true>(argv + 2);
    if (argc == 11 && mode == "--probe-sh") return probe_sh_mode(argv + 2);
    if (argc == 12 && mode == "--views") return views_mode(argv + 2);
    if (argc == 21 && mode == "--render-adaptive") return render_adaptive_mode(argv + 2);
    if (argc == 19 && mode == "--light-groups") return light_groups_mode(argv + 2);
    if (argc == 19 && mode == "--depths") return depths_mode(argv + 2);
    if (argc == 18 && mode == "--sample-map") return sample_map_mode(argv + 2);
    if (argc == 20 && mode == "--accumulate") return accumulate_mode(argv + 2);
    if (argc < 10 || mode.rfind("--", 0) == 0) {
        fprintf(stderr, "usage: host_sim scn base W H spp seed policy chunk out.f32 [shard_index shard_count]\n"
                        "       host_sim --unit records.bin out.f32\n"
                        "       host_sim --tree-check scn base\n"
                        "       host_sim --raycast scn base rays.f32 hits.bin\n"
                        "       host_sim --occluded scn base rays.f32 tmax.f32|- out.u8\n"
                        "       host_sim --ambient-occlusion scn base points.f32 seeds.u32 radius.f32|- spp open.u32 bent.f32|- states.u32|-\n"
                        "       host_sim --radiance scn base rays.f32 seeds.u32 spp rr out.f32 states.u32\n"
                        "       host_sim --radiance-adaptive scn base rays.f32 seeds.u32 min_spp max_spp check_every tolerance floor rr out.f32 spp.u32 m2.f32 states.u32\n"
                        "       host_sim --irradiance scn base points.f32 seeds.u32 spp rr out.f32 states.u32\n"
                        "       host_sim --irradiance-adaptive scn base points.f32 seeds.u32 min_spp max_spp check_every tolerance floor rr out.f32 spp.u32 m2.f32 states.u32\n"
                        "       host_sim --probe-sh scn base points.f32 seeds.u32 spp rr sh.f32 out.f32|- states.u32|-\n"
                        "       host_sim --views scn base cams.f32 seeds.u32 W H spp policy chunk out.f32\n"
                        "       host_sim --render-adaptive scn base W H x0 y0 x1 y1 seed min_spp max_spp check_every tolerance floor rr out.f32 spp.u32 m2.f32 states.u32\n"
                        "       host_sim --features scn base cams.f32|- seeds.u32|seed W H x0 y0 x1 y1 spp albedo.f32|- normal.f32|- depth.f32|- hits.u32|- ids.u32|- states.u32|-\n"
                        "       host_sim --follow scn base cams.f32|- seeds.u32|seed W H x0 y0 x1 y1 spp rr max_bounces albedo.f32|- normal.f32|- depth.f32|- hits.u32|- ids.u32|- bounces.u32|- states.u32|-\n"
                        "       host_sim --matte scn base cams.f32|- seeds.u32|seed W H x0 y0 x1 y1 spp by slots ids.u32 counts.u32 other.u32|- hits.u32|- states.u32|-\n"
                        "       host_sim --light-groups scn base cams.f32|- seeds.u32|seed W H x0 y0 x1 y1 spp rr groups.u8 G groups.f32 rgb.f32|- states.u32|-\n"
                        "       host_sim --depths scn base cams.f32|- seeds.u32|seed W H x0 y0 x1 y1 spp rr G bins.f32 rgb.f32|- lengths.u32|- states.u32|-\n"
                        "       host_sim --sample-map scn base cams.f32|- seeds.u32|seed W H x0 y0 x1 y1 cap rr map.u32 rgb.f32 m2.f32|- states.u32|-\n"
                        "       host_sim --accumulate scn base cams.f32|- seeds.u32|seed W H x0 y0 x1 y1 cap rr map.u32|- sum.f32 m2.f32|- count.u32 states.u32 rgb.f32|-\n");
        return 2;
    }
    int W = atoi(argv[3]), H = atoi(argv[4]);
    uint32_t spp = (uint32_t)strtoul(argv[5], 0, 10), seed = (uint32_t)strtoul(argv[6], 0, 10);
    std::string policy = argv[7];
    uint32_t chunk = (uint32_t)strtoul(argv[8], 0, 10);
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535) { fprintf(stderr, "bad frame size\n"); return 1; }
    Sim S;
    if (int rc = sim_open(S, argv[1], argv[2], TAB_PRO | TAB_LIGHTS | TAB_MATS)) return rc;
    ort_scene *scene = S.scene;
    const Tree &t = scene->tree;
    SceneView &sv = S.sv;
    unsigned long long *ctrl = S.ctrl;
    ort_camera cam;
    camera_basis(*scene, W, H, &cam);
    memcpy(sv.cam, &cam, sizeof(cam));

    ort_render_params p = sim_params(W, H, spp, seed, policy, chunk);
    p.shard_count = argc > 11 ? (uint32_t)atoi(argv[11]) : 1; p.shard_index = argc > 11 ? (uint32_t)atoi(argv[10]) : 0;
    if (!p.shard_count || p.shard_index >= p.shard_count) { fprintf(stderr, "bad shard\n"); return 1; }
    if (policy == "chunk" && (!chunk || spp % chunk)) { fprintf(stderr, "chunk must divide spp\n"); return 1; }
    std::vector<ort_tile_job> jobs;
    if (policy != "pixel" && policy != "chunk") {
        uint32_t master = seed;
        auto xs = [&]() { master ^= master << 13; master ^= master >> 17; master ^= master >> 5; return master; };
        if (policy == "whole") jobs.push_back(ort_tile_job{0, 0, W, H, xs(), spp});
        else {
            int tw = (int)ceilf(W / 32.0f), th = (int)ceilf(H / 32.0f);
            for (int ty = 0; ty < 32; ++ty) for (int tx = 0; tx < 32; ++tx) {
                ort_tile_job j{tx * tw, ty * th, std::min(W, tx * tw + tw), std::min(H, ty * th + th), xs(), spp};
                if (j.x0 < j.x1 && j.y0 < j.y1) jobs.push_back(j);
            }
        }
    }
    const LaunchPlan pl = plan_render(sim_traits(S), p, !jobs.empty(), jobs.size(), false, sim_knobs());
    RenderView rv{};
    render_view(p, pl, nullptr, nullptr, &rv);
    std::vector<float> out((size_t)W * H * 3, 0.0f), partial(pl.partial_bytes / sizeof(float), 0.0f); /* packed block layout: edge blocks are whole */
    std::vector<uint32_t> finals(jobs.size());
    rv.out = out.data(); rv.partial = partial.data(); rv.next_job = ctrl; rv.counters = ctrl + 1;
    if (!jobs.empty()) { rv.jobs = jobs.data(); rv.final_states = finals.data(); }
    std::vector<uint32_t> pix_rng((size_t)W * H, 0);
    const RenderHot hot = render_hot<RenderHot>(rv, &rv);
    if (getenv("SIM_RAY_LOG")) { g_ray_log = fopen(getenv("SIM_RAY_LOG"), "wb"); g_dbg_x = atoi(getenv("SIM_X")); g_dbg_y = atoi(getenv("SIM_Y")); }
    if (getenv("SIM_DUMP_RNG")) { g_pixel_rng = pix_rng.data(); g_W = W; }
    auto t0 = std::chrono::steady_clock::now();
    const bool wide = getenv("SIM_WIDE") != nullptr;
    if (getenv("SIM_WAVEFRONT")) {
        /* the wavefront schedule with a small slot pool: shade all slots, trace all slots, repeat */
        if (S.tab) { fprintf(stderr, "SIM_TABS: the wavefront kernels read the tables from their arrays\n"); return 1; }
        std::vector<uint32_t> bfsq(scene->ref.nodes.size() + 8), bfs_lock(1, 0u);
        S.cold.bfs_pool = bfsq.data(); S.cold.bfs_locks = bfs_lock.data(); S.cold.bfs_queue_cap = (uint32_t)bfsq.size(); S.cold.bfs_queue_count = 1;
        uint32_t slots = (uint32_t)atoi(getenv("SIM_WAVEFRONT"));
        if (slots > rv.job_count) slots = (uint32_t)rv.job_count;
        std::vector<float4> od0(slots), hit0(slots), p0(slots), p1(slots), p2(slots);
        std::vector<float2> od1(slots);
        std::vector<uint4> p3(slots);
        std::vector<uint32_t> hitp(slots), flags(slots, (uint32_t)PS_NEED_JOB);
        unsigned long long active = 0;
        WfView wf{slots, od0.data(), od1.data(), hit0.data(), hitp.data(), p0.data(), p1.data(), p2.data(), p3.data(), flags.data(), &active};
        std::vector<uint32_t> wlds(kWfLdsStack * kBlock), wspill(kWfSpill);
        Counters c;
        for (;;) {
            unsigned long long produced = 0;
            for (uint32_t i = 0; i < slots; ++i) produced += wf_shade_slot<LF_COUNTERS>(sv, hot, nullptr, wf, i, c) ? 1 : 0;
            if (!produced) break;
            for (uint32_t i = 0; i < slots; ++i) wf_trace_slot<LF_COUNTERS>(sv, nullptr, wf, i, 0, wlds.data(), wspill.data(), 0, c);
        }
        flush_counters(hot, c, true);
    } else {
        if (wide) { /* the 4-wide form of the tree (DevNode4, visit_node4) */
            if (t.nodes4.empty()) { fprintf(stderr, "no wide tree\n"); return 1; }
            fprintf(stderr, "wide tree: %zu nodes, depth %u\n", t.nodes4.size(), t.max_depth4);
            sv.nodes = (const float4 *)t.nodes4.data();
        }
        run_pt_lanes(S, hot, wide, false);
    }
    if (rv.mode == JOBS_CHUNK)
        for (unsigned long long i = 0; i < (unsigned long long)rv.my_blocks * 64; ++i) combine_pixel(hot, i);
    double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

#ifdef ORT_CHAIN_STATS
    cs_dump();
#endif
    print_counters(S, sec, finals.empty() ? "" : (" final_rng " + std::to_string(finals.back())).c_str());
#ifdef ORT_CHAIN_CROSSCHECK
    fprintf(stderr, "chain shortcut == full walk on %llu rays; unnested chains %u\n", g_chain_crosschecks, scene->ref.unnested_chains);
#endif
    if (g_ray_log) fclose(g_ray_log);
    if (g_pixel_rng && !write_bytes(getenv("SIM_DUMP_RNG"), pix_rng.data(), pix_rng.size() * 4)) return 1;
    return write_bytes(argv[9], out.data(), out.size() * sizeof(float)) ? 0 : 1;
}
