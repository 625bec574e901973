/*
 * ort_plan.h -- the launch policy of the render call, of a batch of views and of the three ray queries, as arithmetic: what
 * ort_kernels.hip launches, with which grid and which thresholds, decided from a few facts about the uploaded scene
 * (SceneTraits), the render parameters or the ray count, and the developer knobs: plan_render for ort_render_image and
 * ort_render_views; plan_pixel_jobs, given the RenderKind, for the renders that cut one-pixel jobs over a batch of views
 * (ort_render_adaptive, ort_render_light_groups, ort_render_sample_map, ort_render_accumulate and the views form of each);
 * plan_ray_query for ort_raycast and ort_occluded, plan_radiance for ort_radiance.  Host-only and free of HIP,
 * so that tools/launch_plan.cpp and tests/test_launch_plan.py can hold the measured crossovers without a device.
 * ort_kernels.hip turns a LaunchPlan or a QueryPlan into launches and decides nothing.
 */
#ifndef ORT_PLAN_H
#define ORT_PLAN_H

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/ort.h"

namespace ort {

/* Developer knobs (none changes a result).  The environment is read ONCE, when the scene is uploaded
   (ort_scene_upload); ORT_KNOBS_LIVE=1 -- tests and tuning sweeps that flip a knob between two renders of one uploaded
   scene -- reads it again at every render.  -1 = not set: the launch policy decides. */
struct Knobs {
    uint32_t force_fallback_mask = 0xffffffffu; /* ORT_DEBUG_FORCE_FALLBACK */
    bool debug_util = false, debug_fallback = false, debug_drain = false; /* ORT_DEBUG_UTIL, ORT_DEBUG_FALLBACK, ORT_DEBUG_DRAIN */
    int cache_resident = -1;   /* ORT_CACHE_RESIDENT */
    int refill_below = -1, descend_below = -1; /* ORT_REFILL_BELOW, ORT_DESCEND_BELOW */
    bool wavefront = false;    /* ORT_MODE=wavefront */
    bool general_kernel = false; /* ORT_KERNEL=general */
    int lds_tables = -1;       /* ORT_LDS_TABLES */
    int exchange = -1;         /* ORT_EXCHANGE */
    int long_min = -1, long_refill = -1, inflight_cap = -1, park_min = -1; /* ORT_LONG_MIN, ORT_LONG_REFILL, ORT_INFLIGHT_CAP, ORT_PARK_MIN */
    int lpt = -1;              /* ORT_LPT=0: CHUNK jobs issued chunk-major (rounds 1-2) instead of block-major */
    int wide = -1;             /* ORT_WIDE=1: traverse the 4-wide form of the tree (default: never) */
    int waves5 = -1;           /* ORT_WAVES5=0 / 1: the plain loop's five-waves-per-SIMD build (default: all-lobes flavour, trees that leave the L2) */
    int endgame_jobs = -1;     /* ORT_ENDGAME_JOBS: the ray exchange drains its stashes over the last n/4 jobs per lane (default 16 = four jobs) */
    int blocks_per_cu = -1;    /* ORT_BLOCKS_PER_CU (takes effect at upload) */
    int job_batch = -1, batch_tail = -1; /* ORT_JOB_BATCH: job indices a wave draws at a time (0: one draw per job); ORT_BATCH_TAIL: ... until this many jobs per lane are left */
};
inline int env_int(const char *name, int unset = -1) {
    const char *e = getenv(name);
    return e ? atoi(e) : unset;
}
inline Knobs read_knobs() {
    Knobs k;
    const char *e;
    if ((e = getenv("ORT_DEBUG_FORCE_FALLBACK"))) k.force_fallback_mask = (uint32_t)strtoul(e, nullptr, 0);
    k.debug_util = getenv("ORT_DEBUG_UTIL") != nullptr;
    k.debug_fallback = getenv("ORT_DEBUG_FALLBACK") != nullptr;
    k.debug_drain = getenv("ORT_DEBUG_DRAIN") != nullptr;
    k.cache_resident = env_int("ORT_CACHE_RESIDENT");
    k.refill_below = env_int("ORT_REFILL_BELOW");
    k.descend_below = env_int("ORT_DESCEND_BELOW");
    k.wavefront = (e = getenv("ORT_MODE")) && strcmp(e, "wavefront") == 0;
    k.general_kernel = (e = getenv("ORT_KERNEL")) && strcmp(e, "general") == 0;
    k.lds_tables = env_int("ORT_LDS_TABLES");
    k.exchange = env_int("ORT_EXCHANGE");
    k.long_min = env_int("ORT_LONG_MIN");
    k.long_refill = env_int("ORT_LONG_REFILL");
    k.inflight_cap = env_int("ORT_INFLIGHT_CAP");
    k.park_min = env_int("ORT_PARK_MIN");
    k.lpt = env_int("ORT_LPT");
    k.wide = env_int("ORT_WIDE");
    k.waves5 = env_int("ORT_WAVES5");
    k.endgame_jobs = env_int("ORT_ENDGAME_JOBS");
    k.blocks_per_cu = env_int("ORT_BLOCKS_PER_CU");
    k.job_batch = env_int("ORT_JOB_BATCH");
    k.batch_tail = env_int("ORT_BATCH_TAIL");
    return k;
}

/* The lane code's limits the policy counts with (ort_lane.h, which only a HIP unit can include: ort_kernels.hip asserts every
   one of them equal to its original) */
constexpr uint32_t kPlanBlock = 256;     /* kBlock: lanes per workgroup */
constexpr uint32_t kPlanLdsStack = 24;   /* kLdsStack of the four-waves unit, the one with the ray exchange */
constexpr uint32_t kPlanStashVecs = 9, kPlanCapL = 128, kPlanCapR = 192; /* kStashVecs, kCapL, kCapR */
constexpr uint32_t kPlanTabPro = 1u, kPlanTabLights = 2u, kPlanTabMats = 8u; /* TAB_PRO, TAB_LIGHTS, TAB_MATS */
constexpr uint32_t kPlanAllTabs = kPlanTabPro | kPlanTabLights | kPlanTabMats;
constexpr uint32_t kPlanTabMatCap = 48, kPlanTabLightCap = 64, kPlanTabProCap = 40; /* kTabMatCap, kTabLightCap, kTabProCap */
enum : int { PLAN_JOBS_EXPLICIT = 0, PLAN_JOBS_PIXEL = 1, PLAN_JOBS_CHUNK = 2 }; /* JOBS_* */

/* the resident workgroups of a persistent launch: per_cu for each compute unit (256 units where the device reports none) */
inline unsigned int persistent_blocks(int cu_count, unsigned int per_cu) { return (unsigned int)(cu_count > 0 ? cu_count : 256) * per_cu; }
/* ... as fixed at upload: 4 workgroups of 256 lanes per CU (4 = one wave per SIMD each), or ORT_BLOCKS_PER_CU */
inline unsigned int upload_max_blocks(int cu_count, const Knobs &kn) {
    unsigned int per_cu = kn.blocks_per_cu > 0 ? (unsigned int)kn.blocks_per_cu : 4u;
    if (per_cu < 1u || per_cu > 8u) per_cu = 4u;
    return persistent_blocks(cu_count, per_cu);
}

/* the one cache-residency line: trees up to 16 MB stay in the 8 x 4 MB of L2.  knob = ORT_CACHE_RESIDENT (A/B runs: treat
   the tree as (not) cache-resident), -1: not set */
inline bool tree_is_cache_resident(size_t fast_tree_bytes, int knob) {
    return knob >= 0 ? knob != 0 : fast_tree_bytes <= (size_t)(16u << 20);
}

/* the 8x8 blocks a PIXEL / CHUNK render enumerates: the whole grid in its global numbering when sharded (that is
   what block_id % world == rank refers to), only the blocks under the rect on one GPU */
struct BlockGrid { uint32_t blocks_w, block_x0, block_y0, my_blocks, shard_index, shard_count; };
inline BlockGrid block_grid_for(const ort_render_params *p) {
    BlockGrid g;
    g.shard_count = p->shard_count > 1 ? p->shard_count : 1;
    g.shard_index = p->shard_count > 1 ? p->shard_index : 0;
    g.blocks_w = (uint32_t)((p->width + 7) / 8);
    uint32_t total = g.blocks_w * (uint32_t)((p->height + 7) / 8);
    g.block_x0 = g.block_y0 = 0;
    if (g.shard_count == 1 && p->x1 > p->x0 && p->y1 > p->y0) {
        g.block_x0 = (uint32_t)(p->x0 / 8);
        g.block_y0 = (uint32_t)(p->y0 / 8);
        g.blocks_w = (uint32_t)((p->x1 + 7) / 8) - g.block_x0;
        total = g.blocks_w * ((uint32_t)((p->y1 + 7) / 8) - g.block_y0);
    }
    g.my_blocks = (total > g.shard_index) ? (total - g.shard_index + g.shard_count - 1) / g.shard_count : 0;
    return g;
}

inline uint64_t shard_block_count(const ort_render_params *p) { return block_grid_for(p).my_blocks; }

inline uint64_t render_workspace_bytes(const ort_render_params *p) {
    if (p->policy != ORT_POLICY_CHUNK || p->chunk == 0) return 0;
    uint64_t nch = p->spp / p->chunk;
    return nch * (uint64_t)block_grid_for(p).my_blocks * 64ull * 12ull; /* partial planes hold this shard's blocks only */
}
/* a batch of views (ort_render_views): every view has partial planes of its own */
inline uint64_t render_views_workspace_bytes(const ort_render_params *p, uint32_t view_count) { return (uint64_t)view_count * render_workspace_bytes(p); }

/* Which of the scene's small read-only tables fit their LDS slots (TAB_* bits), decided once at upload: the materials, index 0
   included, up to 48 records; the light types up to 64 lights; the analytic prologue's shapes up to 40 float4 (a box takes two, a
   sphere one, a cylinder four).  A table at its cap uses the last float4 of its slot.  The render kernels keep the tables in LDS
   only if all three fit, the ray queries look at the prologue alone; a scene past a cap -- 48 surface materials, 65 lights --
   is read from HBM by the TABS = false kernels and runs neither the ray exchange, the five-waves build, the implicit job
   spaces nor the wide tree (plan_render below). */
inline uint32_t table_fit_flags(size_t material_count, size_t light_count, uint32_t pro_boxes, uint32_t pro_spheres, uint32_t pro_cyls) {
    uint32_t flags = 0;
    if (2ull * pro_boxes + pro_spheres + 4ull * pro_cyls <= kPlanTabProCap) flags |= kPlanTabPro;
    if (light_count <= kPlanTabLightCap) flags |= kPlanTabLights;
    if (material_count <= kPlanTabMatCap) flags |= kPlanTabMats;
    return flags;
}

/* what the policy reads from an uploaded scene, and nothing else */
struct SceneTraits {
    bool diffuse_only = false;   /* no surface material can enter the specular / transmission blocks */
    uint32_t tab_flags = 0;      /* which small tables fit their LDS slots (TAB_*) */
    size_t fast_tree_bytes = 0;  /* nodes and triangles of the fast tree */
    float sah_cost = 0;          /* expected node visits of a random ray through the scene box (ort_tree.cpp) */
    bool has_wide = false;       /* the 4-wide form of the tree is uploaded */
    int cu_count = 0;
    unsigned int max_blocks = 0; /* resident workgroups of a persistent launch, fixed at upload */
};

/* when a wave leaves its loops: the traversal loop (to start new rays) when fewer lanes than refill_below are still tracing, the
   descend loop when fewer than descend_below still walk interior nodes.  ORT_REFILL_BELOW / ORT_DESCEND_BELOW, clamped; by
   default tuned on MI355X (profiles/r01_tuning.md) separately for trees that stay in L2 and trees that do not */
inline void plan_loop_exits(bool cache_resident_tree, const Knobs &kn, int *refill_below, int *descend_below) {
    *refill_below = kn.refill_below >= 0 ? kn.refill_below : (cache_resident_tree ? 16 : 32); /* 12 until the block-major issue (round 3: 8-way shard 64.4 -> 63.8 ms) */
    if (*refill_below < 1) *refill_below = 1;
    if (*refill_below > 64) *refill_below = 64;
    /* cache-resident trees (bunny room: 6 MB): 8, worth +10 %.  Trees that leave the 8 x 4 MB of L2 (the 1M-triangle
       scene, 86 MB): 16 and a later refill (32): the waits are longer there, so leaving the loops costs more
       (3840x2160, 256 spp: 1 272 Mpaths/s; with the small-tree values 1 100; profiles/r02_tuning.md) */
    *descend_below = kn.descend_below >= 0 ? kn.descend_below : (cache_resident_tree ? 8 : 16);
    if (*descend_below < 0) *descend_below = 0;
    if (*descend_below > 64) *descend_below = 64;
}

/* a wave draws its job indices in batches (ort_lane.h: draw_job) until ORT_BATCH_TAIL jobs per lane are left in the job
   space, then one by one: the end of a launch is dealt as finely as before.
   64 indices at a time, 128 on launches of 96 jobs per lane and more; what a wave holds back is at most two jobs per lane of
   its own, of up to eight average job lengths each in the expensive blocks: batches stop 8 (16) jobs per lane before the
   end.  Whole headline frame / its 8-way shard, ms: no batches 422.5 / 63.7, 32: 418.9 / 63.1, 64: 414.3 / 62.0, 128: 411.3 /
   74.4 (with the tail of 64), 256: 419.9 / 113 (profiles/r03_tuning.md) */
inline void plan_job_batches(unsigned long long job_count, unsigned long long lanes, const Knobs &kn, uint32_t *job_batch, unsigned long long *batch_until) {
    *job_batch = kn.job_batch >= 0 ? (uint32_t)kn.job_batch : (job_count >= 96ull * lanes ? 128u : 64u);
    const unsigned long long per_lane = kn.batch_tail >= 0 ? (unsigned long long)kn.batch_tail : 8ull * ((*job_batch + 63u) / 64u);
    const unsigned long long tail = per_lane * lanes;
    *batch_until = job_count > tail ? job_count - tail : 0ull;
}

/* What a camera render is: the plain one (plan_render), or one of the kinds that cut one-pixel jobs over a batch of views
   (plan_pixel_jobs), each with a kernel family of its own (kind_family).  The caller of device_render states it (RenderCall::kind),
   the plan carries it, and plan_variant turns it into the family: nobody infers it */
enum RenderKind : int { RK_PLAIN = 0, RK_ADAPTIVE, RK_GROUPS, RK_SAMPLE_MAP, RK_ACCUMULATE, RK_DEPTHS };

/* everything device_render decides before it touches the device */
struct LaunchPlan {
    /* the kernel: wavefront <counters> | five waves <diffuse> | exchange <counters, diffuse> | plain loop <counters, diffuse, tabs,
       implicit, wide>.  diffuse / tabs / implicit are the kernel's template arguments: under counters the diffuse flavour only
       exists with the ORT_DEBUG_UTIL probes, and the exchange kernels know no other job space than the implicit ones */
    bool wavefront = false, exchange = false, five = false, wide = false, counters = false, diffuse = false, tabs = false, implicit = false;
    bool util = false; /* ORT_DEBUG_UTIL probes (counters builds) */
    /* a batch of views (ort_render_views, view_count > 1): the plain loop's VIEWS kernels, whose lanes read their camera from a
       per-view table; the job space is view_count times the single view's, the view outermost */
    bool views = false;
    RenderKind kind = RK_PLAIN; /* other than plain (plan_pixel_jobs): that kind's kernels <counters, diffuse, tabs> */
    uint32_t view_count = 1;
    unsigned long long view_jobs = 0; /* jobs of one view (job_count / view_count) */
    unsigned int grid = 1;
    /* the job space */
    int mode = PLAN_JOBS_EXPLICIT;
    uint32_t nchunks = 0;
    unsigned long long job_count = 0;
    BlockGrid blocks{};
    /* the RenderView fields that are policy */
    int refill_below = 0, descend_below = 0;
    uint32_t capL = 0, capR = 0, long_min = 0, long_refill = 0, inflight_cap = 0, park_min = 0;
    unsigned long long endgame_from = 0;
    uint32_t stash_wave_f4 = 0;
    uint32_t block_major = 0;
    uint32_t job_batch = 0;
    unsigned long long batch_until = 0;
    /* the buffers that follow: CHUNK partial planes (= render_workspace_bytes), the waves' stashes, ORT_DEBUG_DRAIN end times
       (allocated only by calls that read stats back) */
    size_t partial_bytes = 0, stash_bytes = 0, drain_bytes = 0;
};

/* job_count: the number of explicit jobs (explicit_jobs; ignored otherwise: PIXEL / CHUNK job spaces follow from p).
   w5_layout_ok: a planner switch, false = never the five-waves unit (the units share one definition of the argument structs, so
   device_render passes true; tools/launch_plan and its tests keep the input).
   view_count: the views of an ort_render_views batch (PIXEL / CHUNK job spaces only).  1 is the render call as it always was: a
   batch of one view is that call with the view's camera and seed.  More than one: the job space is [view][block][chunk][pixel]
   -- the view outermost, so the lanes of a wave almost always share a camera and the launch ends on the last view's last blocks --
   and the launch is always the plain persistent loop at four waves: no ray exchange, no five-waves unit, no wide tree, no
   wavefront mode and no ORT_DEBUG_UTIL probes, whatever the knobs say (those variants are not built with a camera table).
   diffuse and tabs are decided as ever; the batch and refill rules count with the enlarged job space. */
inline LaunchPlan plan_render(const SceneTraits &t, const ort_render_params &p, bool explicit_jobs, uint64_t job_count, bool w5_layout_ok,
                              const Knobs &kn, uint32_t view_count = 1) {
    LaunchPlan pl;
    const bool views = view_count > 1u && !explicit_jobs;
    const bool want_util = kn.debug_util && !views; /* developer diagnostics, counters build only */
    /* tuning knobs; results do not depend on them */
    const bool cache_resident_tree = tree_is_cache_resident(t.fast_tree_bytes, kn.cache_resident);
    plan_loop_exits(cache_resident_tree, kn, &pl.refill_below, &pl.descend_below);

    pl.blocks = block_grid_for(&p);
    if (explicit_jobs) {
        pl.mode = PLAN_JOBS_EXPLICIT;
        pl.job_count = job_count;
    } else if (p.policy == ORT_POLICY_PIXEL) {
        pl.mode = PLAN_JOBS_PIXEL;
        pl.nchunks = 1;
        pl.job_count = (unsigned long long)pl.blocks.my_blocks * 64ull;
    } else {
        pl.mode = PLAN_JOBS_CHUNK;
        pl.nchunks = p.spp / p.chunk;
        pl.job_count = (unsigned long long)pl.blocks.my_blocks * 64ull * pl.nchunks;
        pl.partial_bytes = (size_t)pl.nchunks * (size_t)pl.blocks.my_blocks * 64u * 12u; /* = render_workspace_bytes(p) */
    }
    pl.view_jobs = pl.job_count;
    if (views) {
        pl.views = true;
        pl.view_count = view_count;
        pl.job_count *= view_count;
        pl.partial_bytes *= view_count; /* = render_views_workspace_bytes(p, view_count) */
    }

    const bool counters = (p.flags & ORT_RENDER_COUNTERS) != 0;
    const bool wavefront = kn.wavefront && !views; /* ORT_MODE=wavefront; results are identical */
    const bool diffuse = t.diffuse_only && !kn.general_kernel; /* ORT_KERNEL=general forces the all-lobes kernel (A/B runs; same results) */
    /* TABS: the scene's small tables all fit their LDS slots (table_fit_flags); otherwise every one of them is read from HBM */
    const bool tabs = (t.tab_flags & kPlanAllTabs) == kPlanAllTabs && kn.lds_tables != 0; /* ORT_LDS_TABLES=0: read them from HBM anyway (A/B runs; same results) */
    /* the plain loop of implicit job spaces exists at FIVE waves per SIMD as well (ort_kernels_w5.hip: 96 registers, 20 LDS stack
       entries, machine LICM off).  Same call, four / five waves: analytic scene 3 302 / 3 514 Mpaths/s, glass room 3 625 / 3 848,
       testscene 2 790 / 2 885, 1M-triangle scene 1 401 / 1 500 -- the all-lobes flavour and trees that leave the L2 take it.  The
       diffuse flavour on a cache-resident tree does not: bunny room whole frame 4 729 / 4 712, its 4- / 8-way shards 117.0 / 119.2 and
       63.5 / 65.9 ms (a quarter more lanes, a quarter fewer jobs per lane: the tail weighs more); nor the ray exchange (5 053 / 4 949).
       ORT_WAVES5=0 / 1 forces. */
    const bool can_five = !views && !wavefront && !counters && tabs && pl.mode != PLAN_JOBS_EXPLICIT && kn.wide <= 0 && kn.exchange <= 0 && w5_layout_ok;
    /* persistent grid: 4 blocks of 256 lanes per CU (5 for the five-waves kernels, decided below), never more lanes than jobs */
    unsigned long long lanes_wanted = pl.job_count;
    unsigned int max_blocks = t.max_blocks;
    unsigned int grid = (unsigned int)((lanes_wanted + kPlanBlock - 1) / kPlanBlock);
    if (grid > max_blocks) grid = max_blocks;
    if (grid == 0) grid = 1;
    bool exch = false;
    if (!wavefront) {
        /* ray exchange (pt_lane_x): bit-identical; 60 of 64 lanes in the shading pass instead of 53 and leaf
           visits four times better filled, against the parking traffic.  On by itself where it is a gain
           (profiles/r02_tuning.md): the diffuse flavour (the all-lobes one spills too much around the exchange) on
           launches of at least 24 jobs per lane -- every parked path is a job in progress, so a wave's tail grows with
           what it has parked, which short launches cannot amortise (round 3, stashes drained over the last four jobs per
           lane: 2- / 4- / 8-way shard of the headline frame, 63 / 32 / 16 jobs per lane: 216.2 / 115.5 / 65.2 ms with the exchange,
           228.6 / 117.0 / 63.5 plain).  ORT_EXCHANGE=0 / 1 forces it. */
        /* ... and not for trees that leave the L2: the 1M-triangle scene runs 1 392 Mpaths/s with it and 1 393 without (round 2:
           1 268 / 1 272), and its stashes would move 3 TB/s through the fabric for that */
        /* ... and only where rays spend their time in the tree: since a wave draws its jobs in batches of like jobs (draw_job) the
           plain loop keeps its lanes together by itself, and the exchange pays from an SAH cost of the tree (expected node visits of a
           random ray through the scene box, ort_tree.cpp) of about 0.09 -- 1080p / 512 spp, exchange / plain loop, Mpaths/s: bunny at
           scale 3 / 5 / 8 / 12 (SAH cost 0.027 / 0.076 / 0.19 / 0.44) 5 428 / 5 844, 5 143 / 5 151, 3 904 / 3 728, 3 173 / 2 946; dwarf at
           scale 0.008 / 0.012 / 0.02 / 0.03 (0.018 / 0.040 / 0.11 / 0.25) 5 335 / 5 666, 4 921 / 5 143, 4 454 / 4 276, 3 626 / 3 483 */
        const bool worth_it = diffuse && cache_resident_tree && t.sah_cost >= 0.09f && pl.job_count >= 24ull * (unsigned long long)grid * kPlanBlock;
        exch = !views && tabs && pl.mode != PLAN_JOBS_EXPLICIT && (kn.exchange >= 0 ? kn.exchange != 0 : worth_it) && (!counters || (want_util && diffuse));
        if (exch && kn.refill_below < 0) pl.refill_below = 24; /* stragglers park instead of idling: leave the loop a little earlier (dwarf room 4K, 16 / 24 / 48: 4 466 / 4 536 / 4 536 Mpaths/s) */
        if (exch) {
            pl.capL = kPlanCapL; pl.capR = kPlanCapR;
            pl.long_min = kn.long_min >= 0 ? (uint32_t)kn.long_min : 64u;
            pl.long_refill = kn.long_refill >= 0 ? (uint32_t)kn.long_refill : 32u;
            pl.inflight_cap = kn.inflight_cap >= 0 ? (uint32_t)kn.inflight_cap : 64u;
            pl.park_min = kn.park_min >= 0 ? (uint32_t)kn.park_min : 1u;
            if (pl.long_min < 1u) pl.long_min = 1u;
            if (pl.long_min > pl.capL) pl.long_min = pl.capL;
            if (pl.long_refill > 64u) pl.long_refill = 64u;
            /* a wave whose lanes all hold off new jobs (parked paths >= inflight_cap) must be able to start a traversal phase
               on what it has parked (parked + tracing >= long_min), or nothing in it could ever move again */
            if (pl.inflight_cap < pl.long_min) pl.inflight_cap = pl.long_min;
            if (pl.inflight_cap < 1u) pl.inflight_cap = 1u;
            {
                /* the last FOUR jobs per lane (round 3, whole frame / 2- / 4- / 8-way shard: 0 jobs 431.5 / 224.4 / 122.3 / 71.6 ms, two
                   426.3 / 219.8 / 117.5 / 66.1, four 426.4 / 218.8 / 116.6 / 64.6) */
                const unsigned long long quarter_jobs = kn.endgame_jobs >= 0 ? (unsigned long long)kn.endgame_jobs : 16ull;
                const unsigned long long tail_jobs = quarter_jobs * (unsigned long long)grid * kPlanBlock / 4ull;
                pl.endgame_from = pl.job_count > tail_jobs ? pl.job_count - tail_jobs : 0ull;
            }
            pl.stash_wave_f4 = (kPlanStashVecs + kPlanLdsStack / 4u) * pl.capL + kPlanStashVecs * pl.capR;
            pl.stash_bytes = (size_t)t.max_blocks * (kPlanBlock / 64) * pl.stash_wave_f4 * 16u; /* float4 units */
        }
    }
    const bool five = can_five && !exch && (kn.waves5 >= 0 ? kn.waves5 != 0 : (!diffuse || !cache_resident_tree));
    if (five && kn.blocks_per_cu <= 0) {
        max_blocks = persistent_blocks(t.cu_count, 5u);
        grid = (unsigned int)((lanes_wanted + kPlanBlock - 1) / kPlanBlock);
        if (grid > max_blocks) grid = max_blocks;
        if (grid == 0) grid = 1;
    }
    /* CHUNK renders issue their jobs block-major (see "the order in which a CHUNK render issues its jobs"); ORT_LPT=0:
       chunk-major as in rounds 1-2 (A/B runs; same image either way) */
    if (pl.mode == PLAN_JOBS_CHUNK && pl.nchunks >= 2u && kn.lpt != 0) pl.block_major = 1u;
    if (!wavefront) plan_job_batches(pl.job_count, (unsigned long long)grid * kPlanBlock, kn, &pl.job_batch, &pl.batch_until);
    if (kn.debug_drain && !wavefront) pl.drain_bytes = (size_t)max_blocks * (kPlanBlock / 64) * sizeof(unsigned long long);
    /* 4-wide tree (DevNode4): half the dependent node fetches per ray -- and twice the vector instructions per visit, in a
       kernel that is issue-bound at a third of its lanes on the trees it was meant for: 1 218 against 1 368 Mpaths/s on the
       1M-triangle scene (profiles/r03_tuning.md).  Off unless ORT_WIDE=1 asks for it (same image either way). */
    const bool wide = !views && t.has_wide && !exch && tabs && (counters || pl.mode != PLAN_JOBS_EXPLICIT) && !(counters && diffuse && want_util) && kn.wide > 0;

    pl.wavefront = wavefront;
    pl.counters = counters;
    pl.util = want_util;
    pl.exchange = exch;
    pl.five = five;
    pl.wide = wide && !wavefront;
    pl.diffuse = diffuse && (!counters || want_util);
    pl.tabs = tabs;
    /* IMPLICIT job spaces (PIXEL / CHUNK policies): the variant whose lanes carry no job rect / count / index */
    pl.implicit = !wavefront && !counters && tabs && pl.mode != PLAN_JOBS_EXPLICIT;
    pl.grid = grid;
    return pl;
}

/* The launch of a camera render that cuts one-pixel jobs over view_count >= 1 frames, of the kind given (not RK_PLAIN): always
   the plain persistent loop at four waves, over the implicit one-pixel jobs of the PIXEL policy, with the camera read from the
   view table -- the single frame is the one-view batch of the scene's own camera.  The job space is plan_render's for a batch of
   views, [view][block][pixel], and so are the grid, the refill and descend thresholds and the batch rules; p.chunk is not read.
   The ray exchange, the five-waves unit, the wide tree and wavefront mode are not built for these kinds and their knobs are not
   looked at; ORT_DEBUG_UTIL and ORT_DEBUG_DRAIN have no probes here.  Both BSDF flavours exist with counters, as for the radiance
   queries; every variant is IMPLICIT.  No partial planes, no stashes: no workspace.  The kinds have every field but `kind` in
   common (tests/test_launch_plan.py and the kinds' *_host.py tests hold them to it); what a job is differs:
   - RK_ADAPTIVE (ort_render_adaptive, ort_render_views_adaptive; the pt_adaptive kernels): p.spp is not read either -- a job's
     length is the stopping rule's to decide, at most max_spp;
   - RK_GROUPS (ort_render_light_groups, ort_render_views_light_groups; pt_groups): the group sums where the stopping rule
     stands.  A job is p.spp samples long (render_view's to say);
   - RK_SAMPLE_MAP (ort_render_sample_map, ort_render_views_sample_map; pt_sample_map): the caller's map where the stopping rule
     stands.  The job space holds every pixel under the rect, whatever its word of the map says: the plan cannot read a map that
     may live on the device, and a job of no samples ends where it is drawn.  p.spp is the cap on a job's length (render_view's to
     say);
   - RK_ACCUMULATE (ort_render_accumulate, ort_render_views_accumulate; pt_accumulate): the sample-map render's launch, for
     kernels that start a pixel from the caller's planes.  Neither the map nor the planes' counts can be read here, so the job
     space again holds every pixel under the rect;
   - RK_DEPTHS (ort_render_depths, ort_render_views_depths; pt_depths): the light-group render's launch, the sums chosen by the
     depth of the ray an emission arrived on.  A job is p.spp samples long (render_view's to say) */
inline LaunchPlan plan_pixel_jobs(RenderKind kind, const SceneTraits &t, const ort_render_params &p, const Knobs &kn, uint32_t view_count = 1) {
    LaunchPlan pl;
    plan_loop_exits(tree_is_cache_resident(t.fast_tree_bytes, kn.cache_resident), kn, &pl.refill_below, &pl.descend_below);
    pl.blocks = block_grid_for(&p); /* the caller has refused shards: the blocks under the rect */
    pl.mode = PLAN_JOBS_PIXEL;
    pl.nchunks = 1;
    pl.view_jobs = (unsigned long long)pl.blocks.my_blocks * 64ull;
    pl.views = true;
    pl.view_count = view_count;
    pl.job_count = pl.view_jobs * view_count;
    pl.kind = kind;
    pl.counters = (p.flags & ORT_RENDER_COUNTERS) != 0;
    pl.diffuse = t.diffuse_only && !kn.general_kernel;
    pl.tabs = (t.tab_flags & kPlanAllTabs) == kPlanAllTabs && kn.lds_tables != 0;
    pl.implicit = true;
    unsigned long long blocks = (pl.job_count + kPlanBlock - 1) / kPlanBlock;
    pl.grid = (unsigned int)(blocks < t.max_blocks ? blocks : t.max_blocks);
    if (pl.grid == 0) pl.grid = 1;
    plan_job_batches(pl.job_count, (unsigned long long)pl.grid * kPlanBlock, kn, &pl.job_batch, &pl.batch_until);
    return pl;
}

/* ---- the kernels that are built ------------------------------------------------------------------------------------------ */
/* A render kernel by name: its family and its template arguments.  A bool its family's kernels do not take is stated as what
   they are compiled with (the ray exchange and the five-waves build: tabs and implicit; wavefront mode: none of the four) */
enum KernelFamily : int { KF_NONE = 0, KF_WAVEFRONT, KF_LOOP, KF_LOOP_VIEWS, KF_EXCHANGE, KF_FIVE, KF_ADAPTIVE, KF_GROUPS, KF_SAMPLE_MAP, KF_ACCUM, KF_DEPTHS };
struct KernelVariant {
    KernelFamily family;
    bool counters, diffuse, tabs, implicit, wide;
};
constexpr bool operator==(const KernelVariant &a, const KernelVariant &b) {
    return a.family == b.family && a.counters == b.counters && a.diffuse == b.diffuse && a.tabs == b.tabs && a.implicit == b.implicit && a.wide == b.wide;
}
/* the pixel-job kinds' families stand in the kinds' order, KF_ADAPTIVE to KF_DEPTHS */
constexpr KernelFamily kind_family(RenderKind k) { return (KernelFamily)((int)KF_ADAPTIVE + ((int)k - (int)RK_ADAPTIVE)); }
constexpr bool pixel_job_family(KernelFamily f) { return f >= KF_ADAPTIVE && f <= KF_DEPTHS; }
static_assert(kind_family(RK_GROUPS) == KF_GROUPS && kind_family(RK_SAMPLE_MAP) == KF_SAMPLE_MAP && kind_family(RK_ACCUMULATE) == KF_ACCUM && kind_family(RK_DEPTHS) == KF_DEPTHS,
              "a pixel-job kind and its kernel family are added at the same place of their enums");

/* the variant a plan asks for.  A plan that claims two families at once, or a pixel-job kind outside a PIXEL batch of views,
   names none */
inline KernelVariant plan_variant(const LaunchPlan &pl) {
    if ((int)pl.wavefront + (int)pl.exchange + (int)pl.five + (int)pl.views > 1 || (pl.kind != RK_PLAIN && !(pl.views && pl.mode == PLAN_JOBS_PIXEL)))
        return {KF_NONE, false, false, false, false, false};
    if (pl.wavefront) return {KF_WAVEFRONT, pl.counters, false, false, false, false};
    if (pl.exchange) return {KF_EXCHANGE, pl.counters, pl.diffuse, true, true, false};
    if (pl.five) return {KF_FIVE, false, pl.diffuse, true, true, false};
    return {pl.kind != RK_PLAIN ? kind_family(pl.kind) : pl.views ? KF_LOOP_VIEWS : KF_LOOP, pl.counters, pl.diffuse, pl.tabs, pl.implicit, pl.wide};
}

/* All that is built of the families that are built in part, and every one of them costs its share of minutes of compile time:
   ort_kernels.hip instantiates the first four families (its table of launchers is held against this list at compile time),
   ort_kernels_w5.hip the fifth.  The pixel-job kinds' families (ort_kernels_render_adaptive.hip) are built in full -- every
   <counters, diffuse, tabs>, implicit, not wide -- and, like the ray queries' families, need no list: variant_built states the
   rule.  plan_render and plan_pixel_jobs produce nothing that is not built (tools/launch_plan sweep=1 and
   tests/test_launch_plan.py hold them to it); a plan that did would be an error, not a fallback */
constexpr KernelVariant kBuiltKernels[] = {
    /* family, counters, diffuse, tabs, implicit, wide */
    {KF_WAVEFRONT, false, false, false, false, false}, {KF_WAVEFRONT, true, false, false, false, false},
    /* the plain loop: implicit job spaces exist with tables and without counters; under counters the wide tree knows one flavour */
    {KF_LOOP, false, false, false, false, false}, {KF_LOOP, false, false, true, false, false}, {KF_LOOP, false, false, true, true, false},
    {KF_LOOP, false, true, false, false, false}, {KF_LOOP, false, true, true, false, false}, {KF_LOOP, false, true, true, true, false},
    {KF_LOOP, true, false, false, false, false}, {KF_LOOP, true, false, true, false, false},
    {KF_LOOP, true, true, false, false, false}, {KF_LOOP, true, true, true, false, false}, /* diffuse under counters: the ORT_DEBUG_UTIL probes */
    {KF_LOOP, false, false, true, true, true}, {KF_LOOP, false, true, true, true, true}, {KF_LOOP, true, false, true, false, true},
    /* ... with the camera table: counters | diffuse, tabs; implicit follows from both */
    {KF_LOOP_VIEWS, false, false, false, false, false}, {KF_LOOP_VIEWS, false, false, true, true, false},
    {KF_LOOP_VIEWS, false, true, false, false, false}, {KF_LOOP_VIEWS, false, true, true, true, false},
    {KF_LOOP_VIEWS, true, false, false, false, false}, {KF_LOOP_VIEWS, true, false, true, false, false},
    {KF_EXCHANGE, false, false, true, true, false}, {KF_EXCHANGE, false, true, true, true, false},
    {KF_EXCHANGE, true, true, true, true, false}, /* diagnostics: probes of the diffuse flavour */
    {KF_FIVE, false, false, true, true, false}, {KF_FIVE, false, true, true, true, false},
};
constexpr size_t kBuiltKernelCount = sizeof(kBuiltKernels) / sizeof(kBuiltKernels[0]);

/* the place of v in the list, kBuiltKernelCount where it is not listed */
constexpr size_t built_index(const KernelVariant &v) {
    size_t i = 0;
    while (i < kBuiltKernelCount && !(kBuiltKernels[i] == v)) ++i;
    return i;
}
constexpr bool variant_built(const KernelVariant &v) { return pixel_job_family(v.family) ? v.implicit && !v.wide : built_index(v) < kBuiltKernelCount; }

/* ---- the ray queries: the job space is the caller's ray array -------------------------------------------------------- */
/* what ort_kernels.hip launches for a query over count rays: <counters, tabs> of raycast_rays / occluded_rays, <counters,
   diffuse, tabs> of radiance_rays, and the RenderView fields that are policy */
struct QueryPlan {
    bool counters = false, diffuse = false, tabs = false;
    unsigned int grid = 1;
    int refill_below = 0, descend_below = 0;
    uint32_t job_batch = 0;
    unsigned long long batch_until = 0;
};

/* the persistent grid of a query: a lane per ray up to the resident workgroups */
inline unsigned int query_grid(const SceneTraits &t, uint64_t count) {
    const uint64_t blocks = (count + kPlanBlock - 1) / kPlanBlock;
    return (unsigned int)(blocks < t.max_blocks ? blocks : t.max_blocks);
}

/* Closest-hit and occlusion queries.  Fixed by a measured sweep (profiles/r04_raycast_tuning.md); the -D forms exist for such
   sweeps (tools/build_variant.sh) */
#ifndef ORT_RAYCAST_REFILL
#define ORT_RAYCAST_REFILL 32 /* leave the traversal loop, and start new rays, when fewer lanes than this are still tracing */
#endif
#ifndef ORT_RAYCAST_BATCH
#define ORT_RAYCAST_BATCH 1024 /* ray indices a wave draws per atomic */
#endif
#ifndef ORT_RAYCAST_TAIL
#define ORT_RAYCAST_TAIL 4 /* ... until this many rays per lane are left: then exactly as many as it needs */
#endif
/* The launch of ort_raycast and ort_occluded over count rays (count >= 1; raycast_rays, occluded_rays).  It takes no knobs,
   and that is where it parts from plan_radiance below, each difference as the kernels were measured and shipped:
   - refill_below, the batch and its tail are the three constants above: ORT_REFILL_BELOW, ORT_JOB_BATCH and ORT_BATCH_TAIL are
     not read, and there is no 64 / 128 rule;
   - descend_below is 8 or 16 by the 16 MB line, as the renders': ORT_DESCEND_BELOW is not read, and neither is
     ORT_CACHE_RESIDENT;
   - tabs is the prologue's table alone (TAB_PRO: these lanes read neither materials nor lights), whatever ORT_LDS_TABLES says;
   - there is one BSDF-free flavour: diffuse stays false.
   ort_ambient_occlusion (ao_points) launches by this plan too, over count points: a job there is spp draws and bounded walks, not
   one ray, and nothing of the plan has been tuned for that. */
inline QueryPlan plan_ray_query(const SceneTraits &t, uint64_t count, bool counters) {
    QueryPlan pl;
    pl.counters = counters;
    pl.tabs = (t.tab_flags & kPlanTabPro) != 0;
    pl.grid = query_grid(t, count);
    const unsigned long long lanes = (unsigned long long)pl.grid * kPlanBlock;
    pl.refill_below = ORT_RAYCAST_REFILL;
    pl.descend_below = tree_is_cache_resident(t.fast_tree_bytes, -1) ? 8 : 16;
    pl.job_batch = ORT_RAYCAST_BATCH;
    pl.batch_until = count > ORT_RAYCAST_TAIL * lanes ? count - ORT_RAYCAST_TAIL * lanes : 0ull;
    return pl;
}

/* The launch of a first-hit feature render (ort_render_features and its views forms; the feature_pixels kernels): the job space
   is [view][8x8 block under the rect][pixel in block], a job is spp camera samples of one pixel, each one ray of ort_raycast.
   plan_ray_query over those jobs (the grid, the refill and descend thresholds: the walk is that query's), with two differences:
   - these lanes read the materials too, so tabs asks for both the prologue's table and the materials' (TAB_PRO and TAB_MATS); a
     scene past either cap reads both from HBM;
   - a job is a PIXEL job of the render, spp samples long and one of an 8x8 block's 64, not one ray of a long array: the batches
     are the render's (plan_job_batches: a block at a time, ORT_JOB_BATCH and ORT_BATCH_TAIL read).  plan_ray_query's 1024 indices
     per draw hand a full HD frame -- eight jobs per lane -- to the first quarter of the waves, sixteen jobs a lane, before its
     tail rule starts: measured at 1920 x 1080 x 16 spp, 3.5 / 10.8 / 11.0 ms against 1.4 / 4.0 / 2.8 ms on the analytic scene, the
     bunny room and the dwarf room (profiles/r18_features.md). */
inline unsigned long long feature_view_jobs(const ort_render_params &p) { return (unsigned long long)block_grid_for(&p).my_blocks * 64ull; }
inline QueryPlan plan_features(const SceneTraits &t, const ort_render_params &p, uint32_t view_count, bool counters, const Knobs &kn) {
    const unsigned long long count = feature_view_jobs(p) * view_count;
    QueryPlan pl = plan_ray_query(t, count, counters);
    pl.tabs = (t.tab_flags & (kPlanTabPro | kPlanTabMats)) == (kPlanTabPro | kPlanTabMats);
    plan_job_batches(count, (unsigned long long)pl.grid * kPlanBlock, kn, &pl.job_batch, &pl.batch_until);
    return pl;
}

/* The launch of a feature render that follows mirrors and glass (ort_render_follow and its views forms; the follow_pixels
   kernels): plan_features' rules over the same job space, with one difference: these lanes read the lights' table too
   (sample_random_lights' burn at every bounce), so tabs asks for all three small tables (TAB_PRO, TAB_MATS and TAB_LIGHTS); a scene
   past any of the three caps reads all of them from HBM.  Nothing of the plan has been tuned for paths longer than one ray. */
inline QueryPlan plan_follow(const SceneTraits &t, const ort_render_params &p, uint32_t view_count, bool counters, const Knobs &kn) {
    QueryPlan pl = plan_features(t, p, view_count, counters, kn);
    pl.tabs = (t.tab_flags & kPlanAllTabs) == kPlanAllTabs;
    return pl;
}

/* The launch of an ID-matte render (ort_render_matte and its views forms; the matte_pixels kernels): plan_features, every rule
   unchanged -- the job space, the walk and the batches are that render's.  tabs stays plan_features' condition although these lanes
   read no material: one condition for both first-hit kinds, so that their plans are the same line for line. */
inline QueryPlan plan_matte(const SceneTraits &t, const ort_render_params &p, uint32_t view_count, bool counters, const Knobs &kn) {
    return plan_features(t, p, view_count, counters, kn);
}

/* The launch of a radiance query over count rays (ort_radiance; the radiance_rays kernels): always the plain persistent loop at
   four waves.  The ray exchange, the five-waves unit, the wide tree and wavefront mode are not built with a ray job space and
   their knobs are not looked at; ORT_DEBUG_UTIL has no probes here.  diffuse, tabs, the refill and descend thresholds and the
   batch rules are decided as plan_render decides them for the plain loop, with one difference: both BSDF flavours exist with
   counters.  Nothing of this has been tuned for ray batches yet. */
inline QueryPlan plan_radiance(const SceneTraits &t, uint64_t count, bool counters, const Knobs &kn) {
    QueryPlan pl;
    plan_loop_exits(tree_is_cache_resident(t.fast_tree_bytes, kn.cache_resident), kn, &pl.refill_below, &pl.descend_below);
    pl.counters = counters;
    pl.diffuse = t.diffuse_only && !kn.general_kernel;
    pl.tabs = (t.tab_flags & kPlanAllTabs) == kPlanAllTabs && kn.lds_tables != 0;
    pl.grid = query_grid(t, count);
    if (pl.grid == 0) pl.grid = 1;
    plan_job_batches(count, (unsigned long long)pl.grid * kPlanBlock, kn, &pl.job_batch, &pl.batch_until);
    return pl;
}

} // namespace ort

#endif
