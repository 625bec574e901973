/*
 * ort_lane.h -- the lane code of the path tracer and its kernels (gfx950), without a host side.
 *
 * One GPU lane executes one JOB at a time; a job is one call of the reference function
 * tiled_raytrace_bvh (code/ray.cpp:1178-1466): a pixel rect rendered serially with one
 * xorshift stream.  The lane is a small state machine (new job -> pixel -> sample ->
 * bounce) that alternates "produce the next ray" with an interruptible closest-hit
 * traversal; a lane whose path ends immediately starts its next sample / pixel / job.
 *
 * Traversal replaces raycast_bvh (ray.cpp:624-822): ordered depth-first walk of the
 * 2-wide tree of ort_tree.cpp with a per-lane stack whose first entries live in LDS
 * (column-per-lane, conflict-free) and whose tail spills to scratch.
 *
 * Included by five translation units: ort_kernels.hip (the library's kernels at four waves per SIMD, and the host side),
 * ort_kernels_w5.hip (the plain-loop kernels at FIVE: 96 registers, 20 LDS stack entries, built with machine LICM off),
 * ort_kernels_adaptive.hip (the adaptive radiance queries' kernels, at the first unit's limits: a unit of their own so that they
 * compile beside it), ort_kernels_render_adaptive.hip (the adaptive camera render's, the light-group render's and the sample-map render's, likewise) and ort_kernels_irradiance.hip (the
 * irradiance queries', likewise).  Same lane code, other limits
 * (ORT_WAVES_PER_EU, ORT_LDS_STACK, ORT_SPILL_STACK); each unit compiles it in a namespace of its own, which it names beside
 * its limits (ORT_NS; `ort` when it names none), so that two builds of one template are two symbols.  What does not depend on a
 * limit -- the argument structs and the sibling units' launchers -- is defined once, in namespace ort, ahead of that namespace;
 * the kernels that are no templates are compiled for the unit that asks (ORT_LIBRARY_KERNELS: ort_kernels.hip).
 * tools/host_sim.cpp compiles the lane code for the host (ORT_HOST_SIM: one simulated lane).
 */
#ifndef ORT_LANE_H
#define ORT_LANE_H

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ort_device.h"
#include "ort_scene.h"
#include "ort_setup.h"

/* ---- what passes between the host and the kernels: the argument structs, once for all units ------------------------------
 * None of them depends on a unit's limits, so the host side (ort_kernels.hip) and every unit's kernels share these very types:
 * a sibling unit's launcher takes the host's SceneView and RenderHot as they are.  (PrimInfo, plain integers: ort_scene.h.) */
namespace ort {

#ifdef ORT_HOST_SIM
#define ORT_CONSTANT_AS
#else
/* the structs behind these pointers are written by the host before the launch and never by a kernel: the constant
   address space tells the compiler so, and wave-uniform reads of them become scalar loads (s_load_dwordx8 ...)
   instead of per-lane vector loads of one address */
#define ORT_CONSTANT_AS __attribute__((address_space(4)))
#endif
/* The part of the scene view that only rare paths read -- the reference test order (bit-equal hit distances) and
   the exact breadth-first fallback -- lives behind one pointer in HBM: as by-value kernel arguments these twenty
   scalar registers were spilled to vector lanes and back all through the shading code. */
struct SceneCold {
    const float4 *ref_nodes;   /* reference-compatible octree: 3 per node */
    const uint32_t *ref_recs;
    const uint32_t *tri_order, *sphere_order, *box_order, *cyl_order; /* reference test order (ties) */
    /* exact fallback: a pool of queues in HBM, each long enough for every node of the reference tree
       (a ray enqueues a node at most once), taken with a try-lock for the duration of one re-cast */
    uint32_t *bfs_pool;
    uint32_t *bfs_locks;
    uint32_t bfs_queue_cap, bfs_queue_count;
    unsigned long long *fallback_counters; /* [0] rays re-cast exactly, [1] queue overflows (cannot happen: kept as a tripwire);
                                              diagnostics at [kDiagFallback]: octree nodes enqueued, rays traversed again, busy queues met */
};

struct SceneView {
    const float4 *tab_src;    /* kTabF4 float4, the image of the LDS tables */
    uint32_t tab_flags;
    const float4 *nodes;      /* 4 per node (DevNode), or -- WIDE kernel variants -- 8 per node (DevNode4) */
    const float4 *tris;       /* 3 per triangle: v0 e1 e2 n (12 floats) */
    const float4 *spheres;    /* 1 per sphere: c.xyz r */
    const float4 *boxes;      /* 2 per box */
    const float4 *cyls;       /* 4 per cylinder */
    /* what shading needs to know about a ray's winner: its visibility-chain word and its material index, ONE array
       over all kinds (triangles first; info_index()) so that a lane can ask for both the moment its ray is finished */
    const PrimInfo *prim_info;
    uint32_t info_box, info_cyl, info_sphere; /* first entry of each analytic kind */
    const float4 *materials;  /* 5 per material (DevMaterial) */
    const uint32_t *light_is_sphere;
    uint32_t light_count;
    uint32_t pro_boxes, pro_spheres, pro_cyls; /* analytic prologue: every ray tests shapes [0, n) of each kind outright */
    float cam[12];            /* p, x_axis, y_axis, z_axis */
    /* reference-compatible octree (ort_reftree.cpp): visibility chains */
    const float4 *chain_boxes; /* 2 per chain entry */
    const ORT_CONSTANT_AS SceneCold *cold; /* what only the rare paths read (ties, the exact fallback) */
    unsigned long long *util; /* diagnostics (ORT_DEBUG_UTIL=1, counters build): per-phase wave-iteration and active-lane sums */
    uint32_t force_fallback_mask; /* tests (ORT_DEBUG_FORCE_FALLBACK): also re-cast rays with (bits(dir.x) & mask) == 0; ~0u = off */
};

enum : int { JOBS_EXPLICIT = 0, JOBS_PIXEL = 1, JOBS_CHUNK = 2 };

struct RenderView {
    int mode;
    const ort_tile_job *jobs;
    uint32_t *final_states;
    unsigned long long job_count; /* size of the job index space */
    int W, H, x0, y0, x1, y1;
    uint32_t seed, spp, chunk, nchunks;
    float rr;
    int refill_below; /* leave the traversal loop when fewer lanes than this are still tracing */
    int descend_below; /* leave the descend loop (to process the leaves already reached, and perhaps refill) when
                          fewer lanes than this are still walking interior nodes */
    uint32_t shard_index, shard_count, blocks_w, my_blocks;
    uint32_t block_x0, block_y0; /* unsharded renders enumerate only the 8x8 blocks that touch the rect */
    float *out;      /* W*H*3, or (packed_out) this shard's blocks: my_blocks * 64 * 3 */
    float *partial;  /* CHUNK: nchunks planes of this shard's blocks, my_blocks * 64 * 3 floats each */
    int packed_out;  /* ORT_RENDER_PACKED: out holds only this shard's 8x8 blocks, [local block][pixel in block][rgb] */
    unsigned long long *next_job;
    unsigned long long *counters; /* paths rays node_tests tri_tests analytic_tests fallback_rays */
    /* ray exchange (pt_lane_x): every wave owns two LIFO stashes in HBM, L for parked paths whose ray is still
       being traversed and R for parked paths whose ray is finished; float4 units */
    float4 *stash;
    uint32_t stash_wave_f4; /* per wave: L records kStashVecs * capL, L stacks kLdsStack / 4 * capL, R records kStashVecs * capR (device_render sizes it) */
    uint32_t capL, capR;
    uint32_t long_min;   /* start a traversal phase on parked rays when tracing lanes + parked rays reach this */
    uint32_t long_refill; /* within such a phase, take more parked rays when fewer lanes than this are tracing */
    uint32_t park_min;   /* stragglers are parked only when there are at least this many of them (fewer: they idle through one shading pass, cheaper than an exchange step) */
    uint32_t inflight_cap; /* a lane without a path starts a new job only while the wave holds fewer parked paths than this
                              (every parked path is a job in progress: the more a wave holds, the longer its tail) */
    uint32_t block_major; /* CHUNK policy: the job space is [block][chunk][pixel] (see below) instead of [chunk][block][pixel] */
    unsigned long long endgame_from; /* ray exchange: job index from which waves stop parking and drain their stashes (pt_lane_x) */
    uint32_t job_batch;  /* a wave draws this many job indices from next_job at a time and hands them to its lanes one by one (0 / 1: every draw goes to next_job) */
    unsigned long long batch_until; /* ... while the job counter, as the wave last saw it, is below this index; after it: exactly as many as it needs */
    unsigned long long *drain; /* diagnostics (ORT_DEBUG_DRAIN): when each wave ran out of work (s_memrealtime), [workgroup * 4 + wave] */
    /* a batch of views (ort_render_views; the VIEWS kernels): the job space is [view][the single view's job space], out holds
       view_count frames and partial view_count sets of planes, view-major */
    const float4 *views;          /* 4 per view: p.xyz seed(bits) | x_axis | y_axis | z_axis */
    unsigned long long view_jobs; /* jobs of one view */
    uint32_t view_count;
    /* radiance queries (ort_radiance; the radiance_rays kernels): the job space is the caller's ray array, job j is ray j with spp
       samples on the stream that starts at seeds[j]; out holds job_count x 3 floats, final_states (may be null) job_count states */
    const float2 *rays;           /* job_count x 3: o.x o.y | o.z d.x | d.y d.z */
    const uint32_t *seeds;
    uint32_t ray_tree_spheres, ray_tree_quadrics, ray_tree_boxes; /* what raycast_needs_exact reads (RaycastIO), for the primary rays */
    float ray_lo[3], ray_hi[3];
    /* adaptive radiance queries (ort_radiance_adaptive; the radiance_adaptive_rays kernels): spp above is max_spp; a ray's sample
       count and its sum of squared sample luminance go to ad_spp and ad_m2 (either may be null), job_count words each.  The
       adaptive camera render (pt_adaptive): the same fields; ad_spp, ad_m2 and final_states (each may be null) are planes of
       view_count * W * H words, a pixel's word where its colour is in out */
    uint32_t ad_min_spp, ad_check_every;
    float ad_tolerance, ad_floor;
    uint32_t *ad_spp;
    float *ad_m2;
    /* light-group renders (ort_render_light_groups; the pt_groups kernels): group_of_material holds a byte per material of the
       scene, read only for a light that was hit; group_out holds view_count x group_count frames of W * H * 3 floats, frame
       (v, g) at (v * group_count + g) * W * H * 3, and its words ARE the pixel's group sums while its job runs.  out and
       final_states (a plane of view_count * W * H words, as the adaptive render's) may each be null */
    const uint8_t *group_of_material;
    uint32_t group_count;
    float *group_out;
    /* sample-map renders (ort_render_sample_map; the pt_sample_map kernels): a plane of view_count * W * H words, a pixel's word
       where its colour is in out: the caller's sample count for that pixel, read once where its job is drawn and cut at spp
       above, the cap.  ad_m2 and final_states (each may be null) are planes as the adaptive render's */
    const uint32_t *sample_map;
    /* accumulating renders (ort_render_accumulate; the pt_accumulate kernels): the sample-map render's fields, sample_map null
       where every pixel is asked for the cap, and four planes of the caller's that are read AND written: acc_sum, three floats a
       pixel, the undivided colour sum; ad_spp, the samples a pixel has had; ad_m2 (may be null) and final_states as above.  out
       (may be null) is written alone */
    float *acc_sum;
    /* SH light-probe queries (ort_probe_sh; the probe_sh_points kernels): the irradiance queries' fields, and sh_out, job_count x 27
       floats, [point][coefficient][rgb]: a point's words ARE its 27 sums while its job runs, as group_out's are a pixel's.  out
       (may be null here) holds the plain means */
    float *sh_out;
    /* path-depth renders (ort_render_depths; the pt_depths kernels): depth_out holds view_count x depth_bins frames of W * H * 3
       floats, frame (v, g) at (v * depth_bins + g) * W * H * 3, and its words ARE the pixel's bin sums while its job runs, as
       group_out's are; depth_len (may be null) holds view_count x depth_bins planes of W * H words, plane (v, g) at
       (v * depth_bins + g) * W * H: the pixel's counts of samples by the depth of their last ray.  out and final_states (a plane
       of view_count * W * H words) may each be null */
    uint32_t depth_bins;
    float *depth_out;
    uint32_t *depth_len;
};

/* ---- the order in which a CHUNK render issues its jobs ----------------------------------------------------------
 * A job is a serial stream of `chunk` samples that only one lane can advance.  The policy defines the job SET -- chunk k
 * of pixel i, seeded by (k, i) -- not an order, and seeds belong to jobs, so the order of issue cannot change a bit of
 * the image.  Issued chunk-major ([chunk][block][pixel], rounds 1-2) a launch ended with a sweep over the whole image in
 * which the last lanes to draw an expensive job (a bunny pixel costs eight wall pixels) finished it alone: 12-19 ms on
 * the 57 ms an 8-way shard of the headline frame needs (profiles/r03_scaling_proxy.json, r03_tuning.md).  Now
 * BLOCK-major, [block][chunk][pixel]: all chunks of an 8x8 block are issued together, so the lanes of a wave work on the
 * same few pixels with different seeds -- like rays, like costs, jobs that end together -- and the launch ends on its last
 * BLOCKS, not on a last pass over everything: 8-way shard 70.8 -> 64.6 ms, plain loop on the whole frame 496 -> 461 ms.
 * Issuing the blocks most expensive first on top of that (longest processing time first) was built twice and bought
 * nothing: measured and sorted inside the launch, the lists are never ready in time (the expensive blocks are exactly the
 * ones whose measuring jobs end last); measured by one render and used by the next, an 8-way shard took 65.6 ms against
 * 65.2 in natural block order (profiles/r03_tuning.md).  Natural block order it is: no state, no atomics. */

/* What the kernels receive by value: the handful of render parameters every ray reads; everything else stays in the
   RenderView in HBM behind `c` (job decoding, pixel addresses, stashes: read once per job or per pixel).  By value the
   whole RenderView cost ~45 scalar registers, spilled to vector lanes and back all through the lane code. */
struct RenderHot {
    int mode, W, H;
    float rr;
    int refill_below, descend_below;
    const ORT_CONSTANT_AS RenderView *c;
};

/* wavefront mode: per-slot path state in HBM, structure-of-arrays so that a wave's loads and
   stores are coalesced (consecutive lanes = consecutive slots); 112 B per slot */
struct WfView {
    uint32_t slots;
    float4 *od0;     /* org.xyz dir.x            (shade -> trace) */
    float2 *od1;     /* dir.y dir.z */
    float4 *hit0;    /* best_t hit_n.xyz         (trace -> shade) */
    uint32_t *hitp;  /* hit_prim */
    float4 *p0;      /* weight.xyz color.x       (shade -> shade) */
    float4 *p1;      /* color.yz wo.xy */
    float4 *p2;      /* wo.z rng sample spp */
    uint4 *p3;       /* job_index  px|py<<16  jx0|jx1<<16  jy1|plane<<16 */
    uint32_t *flags; /* bits 0-2 ps, bit 3 primary, bit 4 has a ray to trace */
    unsigned long long *active; /* rays produced by the last counted shade launch */
};

/* a path's state, as the lanes and WfView::flags hold it */
enum : int { PS_NEED_JOB = 0, PS_PIXEL = 1, PS_SAMPLE = 2, PS_HIT = 3, PS_DONE = 4 };

/* the third argument of the ray queries' kernels (raycast_rays, occluded_rays, ao_points; their lanes are described below) */
struct RaycastIO {
    const float2 *rays;        /* count x 3: o.x o.y | o.z d.x | d.y d.z */
    uint2 *hits;               /* count x 3: t n.x | n.y n.z | mat prim (ort_hit) */
    const uint32_t *prim_src;  /* info_index order -> kind << 28 | the shape's index in the scene's own arrays */
    /* The fast tree's quadric boxes hold every hit the reference's intersectors can report for the rays a render casts
       (ort_tree.cpp): unit directions, origins within the scene's box (shapes and camera).  A caller's ray need not be
       either.  A sphere's tangent branch (|b^2 - a c| < 1e-5, ray.cpp:174) widens as 1e-5 / |d|^2 when |d| < 1 -- a
       "hit" far outside the sphere's box -- and the f32 cancellation of both quadrics grows with the origin's distance.
       A cylinder's quadric degrades once |d|^2 nears the subnormal range (a = dx^2 + dy^2 is 0 below |d| ~ 1e-19).
       A direction component of +-0 (or NaN, or one whose reciprocal overflows) makes 1/d non-finite: box shapes in the
       fast tree then part from the reference for rays from exactly a box's face plane (grazing a room's wall).
       Such rays take the exact walk of the reference octree instead (resolve_hit: a phantom that could win). */
    uint32_t tree_spheres;     /* the fast tree holds spheres (those of the analytic prologue are tested outright) */
    uint32_t tree_quadrics;    /* ... spheres or cylinders */
    uint32_t tree_boxes;       /* ... boxes */
    float lo[3], hi[3];        /* the scene's box as ort_tree.cpp sized the quadric boxes for */
};

struct OccludedIO {
    RaycastIO q;            /* the rays and what raycast_needs_exact reads; hits and prim_src are null */
    const float *tmax;      /* count limits, or null: none */
    uint8_t *out;           /* count bytes, each 0 or 1 */
    uint32_t mats_nonzero;  /* no shape of the scene carries material 0 */
};

struct AoIO {
    RaycastIO q;            /* q.rays: the points (p, n); and what raycast_needs_exact reads.  hits and prim_src are null */
    const uint32_t *seeds;  /* count stream seeds (0 is taken as 1) */
    const float *radius;    /* count limits, or null: none */
    uint32_t *open;         /* count: samples with nothing in the way, or ORT_AO_INVALID */
    float *bent;            /* count x 3, or null: the sum of the open samples' directions, in sample order */
    uint32_t *states;       /* count, or null: the stream after 2 * spp steps */
    uint32_t spp;           /* >= 1 */
    uint32_t mats_nonzero;  /* no shape of the scene carries material 0 (the early end, as occluded_lane's) */
};

/* the third argument of feature_pixels: the planes of ort_render_features, view_count frames of W * H entries each, view-major.
   The job space, the rect, spp and the camera table are the RenderView's (features_view, ort_setup.h) */
struct FeatureIO {
    RaycastIO q;            /* q.prim_src, and what raycast_needs_exact reads.  rays and hits are null */
    float *albedo;          /* 3 per pixel, or null */
    float *normal;          /* 3 per pixel, or null */
    float *depth;           /* 1 per pixel, or null */
    uint32_t *hits;         /* 1 per pixel, or null: samples that hit a surface */
    uint32_t *ids;          /* 2 per pixel, or null: mat, prim of sample 0 */
    uint32_t *states;       /* 1 per pixel, or null: the stream after 2 * spp steps */
};

/* the third argument of follow_pixels: the planes of ort_render_follow, laid out as FeatureIO's.  rr is the RenderView's
   (follow_view, ort_setup.h) */
struct FollowIO {
    RaycastIO q;            /* q.prim_src, and what raycast_needs_exact reads.  rays and hits are null */
    float *albedo;          /* 3 per pixel, or null */
    float *normal;          /* 3 per pixel, or null */
    float *depth;           /* 1 per pixel, or null: the path's length from the aperture point to the recorded vertex */
    uint32_t *hits;         /* 1 per pixel, or null: samples that recorded a vertex */
    uint32_t *ids;          /* 2 per pixel, or null: mat, prim of sample 0's last vertex */
    uint32_t *bounces;      /* 1 per pixel, or null: the bounces followed, summed over the recorded samples */
    uint32_t *states;       /* 1 per pixel, or null: the stream after the last sample */
    uint32_t max_bounces;   /* <= ORT_MAX_FOLLOW_BOUNCES: a vertex reached after this many bounces is recorded whatever it is */
};

/* the third argument of matte_pixels: the planes of ort_render_matte, view_count frames view-major; ids and counts hold `slots`
   words per pixel and are the lanes' working memory for the length of a job (matte_lane) */
struct MatteIO {
    RaycastIO q;            /* what raycast_needs_exact reads; q.prim_src is the table the mode names a hit by: the shape table
                               (ORT_MATTE_BY_PRIM), the object table (ORT_MATTE_BY_OBJECT), null (ORT_MATTE_BY_MATERIAL).  rays and hits are null */
    uint32_t *ids;          /* slots per pixel */
    uint32_t *counts;       /* slots per pixel */
    uint32_t *other;        /* 1 per pixel, or null: recorded samples that found no slot */
    uint32_t *hits;         /* 1 per pixel, or null: recorded samples */
    uint32_t *states;       /* 1 per pixel, or null: the stream after 2 * spp steps */
    uint32_t by;            /* ORT_MATTE_BY_* */
    uint32_t slots;         /* K, within [1, ORT_MAX_MATTE_SLOTS] */
};

} // namespace ort

#ifndef ORT_HOST_SIM
/* The sibling units' entry points, declared here alone: each is defined by the unit that holds its kernels and called by
   ort_kernels.hip.  The flavour comes as named fields: a render kernel's KernelVariant (plan_variant, ort_plan.h), a query's
   QueryPlan; every other bool of the kernels is fixed by the family. */
void ort_launch_w5(const ort::KernelVariant &v, unsigned int grid, hipStream_t stream, const ort::SceneView &sv, const ort::RenderHot &hot);              /* KF_FIVE: ort_kernels_w5.hip */
void ort_launch_pixel_jobs(const ort::KernelVariant &v, unsigned int grid, hipStream_t stream, const ort::SceneView &sv, const ort::RenderHot &hot);      /* KF_ADAPTIVE to KF_DEPTHS: ort_kernels_render_adaptive.hip */
void ort_launch_radiance_adaptive(const ort::QueryPlan &pl, hipStream_t stream, const ort::SceneView &sv, const ort::RenderHot &hot);                    /* ort_kernels_adaptive.hip */
void ort_launch_irradiance(const ort::QueryPlan &pl, bool adaptive, hipStream_t stream, const ort::SceneView &sv, const ort::RenderHot &hot);            /* ort_kernels_irradiance.hip */
void ort_launch_probe_sh(const ort::QueryPlan &pl, hipStream_t stream, const ort::SceneView &sv, const ort::RenderHot &hot);                             /* ort_kernels_irradiance.hip */
#endif

/* The lane code and the limits it is built for: a unit that compiles them at limits of its own, or beside ort_kernels.hip's,
   names its namespace (ORT_NS) where it states them, so that two builds of one template are two symbols */
#ifndef ORT_NS
#define ORT_NS ort
#endif

namespace ORT_NS {

using namespace ort;
using namespace ortd;

constexpr int kBlock = 256;      /* 4 waves */
#ifndef ORT_LDS_STACK
#define ORT_LDS_STACK 24
#endif
constexpr int kLdsStack = ORT_LDS_STACK; /* entries per lane in LDS: 24 * 256 * 4 B = 24 KB per block */
#ifndef ORT_SPILL_STACK
#define ORT_SPILL_STACK 40
#endif
constexpr int kSpillStack = ORT_SPILL_STACK;  /* scratch tail */
static_assert(kLdsStack - 4 + kSpillStack >= (int)kTreeDepthBudget, "the re-traversal of resolve_hit must hold a tree of kTreeDepthBudget levels");
constexpr uint32_t kBfsPoolQueues = 1024;     /* queues of the breadth-first fallback, shared by all lanes */
constexpr size_t kBfsPoolBytes = 1024u << 20; /* at most; a queue holds one entry per reference-tree node */
constexpr int kDiagFallback = 106;            /* fallback_counters = ctrl + 6: the diagnostics sit at ctrl[112..114] */
constexpr uint32_t kBfsLockStride = 32;       /* u32 units: every lock word has a 128-byte line to itself */

/* the layout of the small LDS tables (kTabRoot ... kTabF4, TAB_*): ort_setup.h, with the host code that fills them */

/* ---- kernel ---------------------------------------------------------------------------- */
#ifdef ORT_HOST_SIM /* one simulated lane per host thread: tools/host_sim.cpp (job draws and counters are atomic: its threads share them) */
#define ORT_BALLOT(p) ((p) ? 1ull : 0ull)
#define ORT_POPC64(m) __builtin_popcountll(m)
#define ORT_NEXT_JOB(p) __atomic_fetch_add((p), 1ull, __ATOMIC_RELAXED)
#define ORT_COUNT(p, v) ((void)__atomic_fetch_add((p), (v), __ATOMIC_RELAXED))
#define ORT_TRY_LOCK(p) (*(p) == 0u ? (*(p) = 1u, true) : false)
#define ORT_PEEK(p) (*(p))
#define ORT_BACKOFF()
#define ORT_UNLOCK(p) (*(p) = 0u)
#define ORT_FENCE()
#define ORT_FFS64(m) __builtin_ffsll((long long)(m))
#define ORT_LANE() 0
#define ORT_UTIL(sv, k, pred)
#define ORT_PHASE(pr, sv, k, pred)
#ifndef ORT_SIM_PIXEL_HOOK
#define ORT_SIM_PIXEL_HOOK(x, y, rng)
#endif
#ifndef ORT_SIM_RAY_HOOK
#define ORT_SIM_RAY_HOOK(x, y, o, d, t, n, m)
#endif
#ifndef ORT_SIM_STACK_HOOK /* traverse's stack depth after every visit and pop (fresh: the traversal starts at the root); tools/host_sim.cpp's probe */
#define ORT_SIM_STACK_HOOK(lds_entries, sp, fresh)
#endif
#else
#define ORT_SIM_PIXEL_HOOK(x, y, rng)
#define ORT_SIM_RAY_HOOK(x, y, o, d, t, n, m)
#define ORT_SIM_STACK_HOOK(lds_entries, sp, fresh)
#define ORT_BALLOT(p) __ballot(p)
#define ORT_POPC64(m) __popcll(m)
#define ORT_NEXT_JOB(p) atomicAdd((p), 1ull)
#define ORT_COUNT(p, v) atomicAdd((p), (v))
#define ORT_TRY_LOCK(p) (atomicCAS((p), 0u, 1u) == 0u)
#define ORT_PEEK(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define ORT_BACKOFF() __builtin_amdgcn_s_sleep(64) /* 64 x 64 clocks, ~2 us */
#define ORT_UNLOCK(p) ((void)atomicExch((p), 0u))
#define ORT_FENCE() __threadfence()
#define ORT_FFS64(m) __ffsll((unsigned long long)(m))
#define ORT_LANE() ((int)__lane_id())
/* lane-utilisation probe: event k happened in this wave with popc(pred) lanes taking part.  Diagnostics build only
   (COUNTERS, ORT_DEBUG_UTIL=1); the waves of the first 32 workgroups record, into LDS (global atomics here would
   keep every following load waiting behind them), flushed to memory when the workgroup ends */
#define ORT_UTIL(sv, k, pred)                                                                        \
    do {                                                                                             \
        if (COUNTERS && (sv).util && blockIdx.x < 32u) {                                             \
            unsigned long long m_ = __ballot(pred);                                                  \
            if (m_ && (int)__lane_id() == __ffsll(m_) - 1) {                                         \
                atomicAdd(&g_lds_prof[2 * (k)], 1ull);                                               \
                atomicAdd(&g_lds_prof[2 * (k) + 1], (unsigned long long)__popcll(m_));               \
            }                                                                                        \
        }                                                                                            \
    } while (0)
/* phase timer (same diagnostics build): the shader cycles since the wave's previous mark are charged to phase k,
   with the number of lanes for which pred holds */
#define ORT_PHASE(pr, sv, k, pred)                                                                   \
    do {                                                                                             \
        if (COUNTERS && (pr).on) {                                                                   \
            const unsigned long long now_ = __builtin_amdgcn_s_memtime();                            \
            const unsigned long long m_ = __ballot(pred), a_ = __ballot(true);                       \
            /* the wave's previous mark lives in LDS: a register would only be updated in the lanes active there */ \
            unsigned long long *last_ = &g_lds_prof[96 + (threadIdx.x >> 6)];                        \
            if ((int)__lane_id() == __ffsll(a_) - 1) {                                               \
                atomicAdd(&g_lds_prof[32 + 3 * (k)], now_ - *last_);                                 \
                atomicAdd(&g_lds_prof[32 + 3 * (k) + 1], 1ull);                                      \
                atomicAdd(&g_lds_prof[32 + 3 * (k) + 2], (unsigned long long)__popcll(m_));          \
                *last_ = __builtin_amdgcn_s_memtime();                                               \
            }                                                                                        \
        }                                                                                            \
    } while (0)
#endif

#ifndef ORT_HOST_SIM
__shared__ unsigned long long g_lds_prof[96 + 4]; /* + the four waves' previous marks */ /* diagnostics build only: [0,32) event probes, [32,96) phase timers */
#endif

struct Prof { unsigned long long t = 0; bool on = false; };

#ifndef ORT_DESCEND_SHIFT
#define ORT_DESCEND_SHIFT 2
#endif

/* Branch-frequency hints on the exactness machinery of resolve_hit (chain walk of odd chains, phantom hits, re-traversals,
   the exact fallback): the register allocator weighs spill code by block frequency and this kernel lives at its
   128-register cap, so telling it that these paths are rare moves the spills there: +4.4 % on the bunny room.  (Hints on
   ties, deep stacks and the once-per-job blocks were neutral or harmful and are not kept.) */
#define ORT_RARE(x) __builtin_expect(!!(x), 0)
#if defined(ORT_HOST_SIM) && defined(ORT_CHAIN_STATS) /* tools/host_sim: why rays leave the fast path */
extern unsigned long long g_cs[4][16];
#define ORT_STAT(row, col) (g_cs[row][col]++)
#else
#define ORT_STAT(row, col) ((void)0)
#endif
constexpr uint32_t kNoPrim = 0xffffffffu;
constexpr uint32_t kTraversalDone = 0xffffffffu; /* == EMPTY_CHILD: a leaf word no tree contains */

/* ---- the compile-time flavours of the lane code, by name -----------------------------------------------------------------
 * Every lane function below is a template over ONE flag word F (and, where it owns a stack, the ints LDS_ENTRIES and BLOCK): a
 * set of the names defined here, read back into constexpr bools of the same names at the function's top.  A caller derives its
 * callee's word from its own by name (F | LF_RAYS, F & ~LF_WIDE, walk_of(F)); a __global__ wrapper builds its lane's from its
 * bools with lf_if.  A word holds only names its function reads (LF_OF_*): two kernels that need the same walk then share one
 * instantiation of it, as they always have -- and which instantiations are shared moves the compiler's code (a word that carried
 * its caller's other names along changed the treelet's address arithmetic in every TABS kernel).  flavour_ok states the legal
 * sets once, and every function asserts it.  A new flavour is one name here, its place in the LF_OF_* of the functions that
 * read it, one line in flavour_ok, and the callers that turn it on. */
constexpr uint32_t LF_COUNTERS = 1u << 0; /* the diagnostics build: paths, rays and tests are counted (Counters), the probes are live */
constexpr uint32_t LF_DIFFUSE = 1u << 1;  /* every surface material of the scene has Ks = Kt = 0 (see at pt_persistent) */
constexpr uint32_t LF_TABS = 1u << 2;     /* the small read-only tables are in LDS (fill_tab): prologue shapes, materials, lights, treelet */
/* IMPLICIT: the caller vouches for an implicit job space (PIXEL / CHUNK policies: every job is one pixel, spp_u
   samples): the job's rect, its sample count and its index then need no registers of their own */
constexpr uint32_t LF_IMPLICIT = 1u << 3;
constexpr uint32_t LF_WIDE = 1u << 4;     /* the fast tree is the 4-wide one (DevNode4; visit_node4): the plain loop of a single frame only */
/* VIEWS: a batch of views (ort_render_views): the job index names the view first, and the view's camera and seed come from
   the table behind rv.c->views instead of sv.cam and rv.c->seed -- the same expressions on the same operands, so the same bits */
constexpr uint32_t LF_VIEWS = 1u << 5;
/* RAYS: radiance queries (ort_radiance; with IMPLICIT): the job space is the caller's ray array (rv.c->rays), a job is ONE ray with
   spp_u samples on the stream that starts at rv.c->seeds[j].  Every sample starts at the ray's origin in the ray's direction,
   with wo = -normalize(d) (ray.cpp:1240-1246 for a camera without an aperture), and no aperture angle is drawn; the job ends
   with 12 bytes at out + 3 j and its stream's state.  The ray is read again for every sample (24 bytes from L2 per path of
   hundreds of node tests) instead of held in six registers through the traversal loop; P.job_index | P.pxy << 32 is the ray index */
constexpr uint32_t LF_RAYS = 1u << 6;
/* ADAPT: adaptive radiance queries (ort_radiance_adaptive; with RAYS) and the adaptive camera render (ort_render_adaptive,
   ort_render_views_adaptive; with VIEWS, one-pixel jobs in JOBS_PIXEL mode): spp_u is max_spp, and the job also ends at the first
   check of the stopping rule (adaptive_stop) that says so.  A (the lane's AdaptState) holds the sum of squared sample
   luminance and the sample count of the next check; the job writes its sample count and that sum besides the mean, which
   divides by the samples taken -- per ray for a query, per pixel of its view's planes for a render, with the stream's state.
   Everything of it sits under if constexpr (ADAPT): the other kernels compile as without it */
constexpr uint32_t LF_ADAPT = 1u << 7;
/* HEMI: irradiance queries (ort_irradiance, ort_irradiance_adaptive; with RAYS): the caller's array holds points (p, n) where RAYS
   reads rays (o, d) -- the same 24 bytes, the same domain test, read again for every sample -- and a sample's primary direction is
   drawn in the lane, on the job's stream: sample_brdf's diffuse draw without the lobe choice (e0, e1; c = sqrt(e0), ray.cpp:1123;
   phi = 2 pi e1), sample_lobe about n (ray.cpp:1065-1091) and normalize for d.  phi is the angle of the one converged sin/cos below;
   from d on the sample is RAYS' for the ray (p, d): direction d as it stands, wo = -normalize(d).  Everything of it sits under
   if constexpr (HEMI) */
constexpr uint32_t LF_HEMI = 1u << 8;
/* GROUPS: light-group renders (ort_render_light_groups; with VIEWS, one-pixel jobs in JOBS_PIXEL mode): whenever a sample adds an
   emission e to the pixel's sum, the same e is added to the sum of the hit light's group (rv.c->group_of_material, a byte per
   material in HBM, read here alone; a group at or above group_count is no group).  The G sums are the pixel's own words of the G
   output frames: the job belongs to this lane from start to end, so it zeroes them at the pixel's start, loads, adds and stores one
   triple per emission and divides them in place at the job's end -- no registers, no LDS, no atomics.  The render's own frame and
   the final states are optional planes.  Everything of it sits under if constexpr (GROUPS) */
constexpr uint32_t LF_GROUPS = 1u << 9;
/* SPPMAP: sample-map renders (ort_render_sample_map; with VIEWS, one-pixel jobs in JOBS_PIXEL mode): the job of pixel i is
   n = min(rv.c->sample_map[i], spp_u) samples long, spp_u being the cap; the lane that draws the job reads the word once, and a
   job of no samples is dropped right there, as a pixel outside the rect is: nothing written, the stream never started, the next job
   drawn in the same pass.  A (the lane's AdaptState) holds n in `next` and the sum of squared sample luminance in q; the job
   writes the mean over n and, where asked for, that sum and the stream's state.  Everything of it sits under
   if constexpr (SPPMAP) */
constexpr uint32_t LF_SPPMAP = 1u << 16;
/* ACCUM: accumulating renders (ort_render_accumulate; with SPPMAP, whose job draw and job end it extends): a pixel's samples
   continue across calls.  The caller's planes hold, per pixel, the UNDIVIDED colour sum C (rv.c->acc_sum), the sum of squared
   sample luminance Q (ad_m2, may be null), the samples taken so far n0 (ad_spp) and the stream's state after sample n0
   (final_states).  The lane that draws the job reads n0 beside the map word (a null map: the cap stands in for it) and forms
   add = min(asked, spp_u, (1 << 24) - min(n0, 1 << 24)); add == 0 is SPPMAP's empty job.  n0 == 0: the job_seed start, C = Q = +0,
   nothing else of the planes read.  n0 > 0: the stream starts at the stored state (0 taken as 1: a zero xorshift state never
   leaves zero), C and Q at the stored sums + (+0), which is what the first added colour makes of them.  The job's end stores
   C, Q, n0 + add, the state and, where asked for (out), C / (float)(n0 + add); n0 is read again there, so it is not live
   through the traversal loop.  A pixel's words are one lane's for the length of its job: no atomics.  Everything of it sits
   under if constexpr (ACCUM) */
constexpr uint32_t LF_ACCUM = 1u << 17;
/* SH: SH light-probe queries (ort_probe_sh; with RAYS and HEMI, never ADAPT): the irradiance query's job with the direction's cosine
   drawn uniformly, c = 1 - 2 e0 (the whole sphere about the pole n), and, whenever a sample adds an emission e to the point's sum,
   b_j(d) * e added to the point's nine SH sums, d being the sample's PRIMARY direction and b_j the real SH basis of bands 0 to 2 in
   world axes (sh_basis_add).  d is not in P.dir once the path has bounced, so the lane keeps it in three words of LDS
   (produce_ray's focal_cache, unused under RAYS): written where the primary ray is composed, read only when an emission is added
   -- no registers through the traversal loop, no second sin/cos.  The 27 sums are the point's own words of rv.c->sh_out, as GROUPS
   keeps its sums: zeroed at the job's start, one load, add and store per word and emission, divided in place at the job's end.
   rv.c->out is an optional array here.  Everything of it sits under if constexpr (SH) */
constexpr uint32_t LF_SH = 1u << 18;
/* DEPTHS: path-depth renders (ort_render_depths; with VIEWS, one-pixel jobs in JOBS_PIXEL mode): every ray of a sample has a depth
   d, 0 for the camera ray and one more with each sample_brdf draw.  Whenever a sample adds an emission e to the pixel's sum, on a
   ray of depth d, the same e is added to the sum of bin min(d, depth_bins - 1); when a sample ends, the length count of the bin
   of its last ray's depth rises by one.  The bin sums are the pixel's own words of the G output frames, kept as GROUPS keeps its
   sums (zeroed at the pixel's start, one load, add and store per triple and emission, divided in place at the job's end), and the
   length counts are the pixel's own words of the G length planes where the caller asks for them.  The one new piece of state is
   d, and it is not a register: it lives in a fourth row of the lane's focal cache (a word of LDS per lane, as pt_persistent_x
   keeps its late flag), zeroed where a pixel starts and where a sample ends, read where an emission is added or a sample ends,
   bumped where a bounce is drawn -- once per RAY, hundreds of node tests, while a register would be live through the whole
   traversal loop of kernels that sit at their 128-register cap.  Everything of it sits under if constexpr (DEPTHS) */
constexpr uint32_t LF_DEPTHS = 1u << 19;
/* the walk's own options */
constexpr uint32_t LF_TREELET = 1u << 10;     /* traverse: the top of the binary tree is read from the LDS tables (with TABS, never WIDE) */
constexpr uint32_t LF_ANNOUNCE = 1u << 11;    /* traverse asks for a finished ray's PrimInfo (announce_winner); resolve_hit then finds it ANNOUNCED */
constexpr uint32_t LF_EXACT_ORDER = 1u << 12; /* test_prim: the exact walk's records, in the reference's order: no exclusion, phantoms, ties or runner-up */
constexpr uint32_t LF_FINITE_RAY = 1u << 13;  /* test_prim: origin and 1/d are finite, a box takes hit_aab_finite */
constexpr uint32_t LF_FROM_TAB = 1u << 14;    /* test_prim: the shape's record comes from the LDS tables (rec) */
constexpr uint32_t LF_HAS_EXCL = 1u << 15;    /* prologue_tests: the re-traversals of resolve_hit ignore one shape (excl); a ray's first traversal ignores none */

constexpr uint32_t lf_if(bool on, uint32_t names) { return on ? names : 0u; }

/* the names each function reads */
constexpr uint32_t LF_OF_TEST_PRIM = LF_COUNTERS | LF_EXACT_ORDER | LF_FINITE_RAY | LF_FROM_TAB;
constexpr uint32_t LF_OF_PROLOGUE = LF_COUNTERS | LF_TABS | LF_HAS_EXCL;
constexpr uint32_t LF_OF_BEGIN_RAY = LF_COUNTERS | LF_TABS;
constexpr uint32_t LF_OF_TRAVERSE = LF_COUNTERS | LF_TREELET | LF_ANNOUNCE | LF_WIDE;
constexpr uint32_t LF_OF_RESOLVE_HIT = LF_COUNTERS | LF_TABS | LF_ANNOUNCE | LF_WIDE;
constexpr uint32_t LF_OF_PRODUCE_RAY = LF_COUNTERS | LF_DIFFUSE | LF_TABS | LF_IMPLICIT | LF_VIEWS | LF_RAYS | LF_ADAPT | LF_HEMI | LF_GROUPS | LF_SPPMAP | LF_ACCUM | LF_SH | LF_DEPTHS;
constexpr uint32_t LF_OF_LANE = LF_OF_PRODUCE_RAY | LF_WIDE; /* pt_lane ... radiance_lane: a job's flavour */
/* ... and, from a lane's flavour f, the words of the three steps of its loop: begin_ray (and a prologue in its place); traverse,
   where finished rays announce their winners and the top of the binary tree comes from the LDS tables if there are any; and the
   resolve_hit that follows such a walk */
constexpr uint32_t begin_of(uint32_t f) { return f & LF_OF_BEGIN_RAY; }
constexpr uint32_t walk_of(uint32_t f) { return (f & (LF_COUNTERS | LF_WIDE)) | LF_ANNOUNCE | lf_if((f & LF_TABS) && !(f & LF_WIDE), LF_TREELET); }
constexpr uint32_t resolve_of(uint32_t f) { return (f & (LF_COUNTERS | LF_TABS | LF_WIDE)) | LF_ANNOUNCE; }

/* the sets that are built: f holds none but the names its function reads, and what each flavour needs beside it or cannot stand beside */
constexpr bool flavour_ok(uint32_t f, uint32_t reads) {
    const bool IMPLICIT = f & LF_IMPLICIT, WIDE = f & LF_WIDE, VIEWS = f & LF_VIEWS, RAYS = f & LF_RAYS, ADAPT = f & LF_ADAPT;
    const bool HEMI = f & LF_HEMI, GROUPS = f & LF_GROUPS, TREELET = f & LF_TREELET, EXACT_ORDER = f & LF_EXACT_ORDER;
    const bool SPPMAP = f & LF_SPPMAP, ACCUM = f & LF_ACCUM, SH = f & LF_SH, DEPTHS = f & LF_DEPTHS;
    return (f & ~reads) == 0u
        && (!RAYS || (IMPLICIT && !VIEWS))                        /* a caller's ray array is an implicit job space of its own */
        && (!ADAPT || (IMPLICIT && (RAYS || VIEWS)))              /* the adaptive rule is built for the radiance queries and for one-pixel jobs of a batch of views */
        && (!HEMI || RAYS)                                        /* the hemisphere draw starts a sample of a radiance query's job */
        && (!GROUPS || (IMPLICIT && VIEWS && !RAYS && !ADAPT))    /* the group sums are built for plain one-pixel jobs of a batch of views */
        && (!SPPMAP || (IMPLICIT && VIEWS && !RAYS && !ADAPT && !GROUPS)) /* the sample map cuts plain one-pixel jobs of a batch of views */
        && (!ACCUM || SPPMAP)                                     /* accumulation continues the sample map's jobs */
        && (!SH || (HEMI && !ADAPT))                              /* the SH sums are built for the plain job of points */
        && (!DEPTHS || (IMPLICIT && VIEWS && !RAYS && !ADAPT && !GROUPS && !SPPMAP)) /* the depth bins are built for plain one-pixel jobs of a batch of views */
        && (!WIDE || !(VIEWS || RAYS || ADAPT || HEMI || GROUPS || SPPMAP || TREELET)) /* the 4-wide tree serves the single frame's plain loop, and has no treelet */
        && (!EXACT_ORDER || !(f & (LF_FINITE_RAY | LF_FROM_TAB))); /* the exact walk reads HBM */
}

ORT_D uint32_t prim_order(const SceneView &sv, uint32_t kind, uint32_t slot) {
    return (kind == PRIM_TRI) ? sv.cold->tri_order[slot] : (kind == PRIM_SPHERE) ? sv.cold->sphere_order[slot]
         : (kind == PRIM_BOX) ? sv.cold->box_order[slot] : sv.cold->cyl_order[slot];
}

/* one primitive against the ray, exactly as raycast_bvh does per record (ray.cpp:647-716):
   accept when hit_t >= 1e-6 and strictly closer than the best so far */
template <uint32_t F>
ORT_D void test_prim(const SceneView &sv, uint32_t kind, uint32_t slot, V3 org, V3 dir, V3 inv_d, float &best_t, V3 &hit_n,
                     uint32_t &hit_prim, float &phantom_t, float &runner_t, unsigned long long &c_tris, unsigned long long &c_analytic,
                     uint32_t excl = 0xffffffffu, const float4 *rec = nullptr /* FROM_TAB: the shape's record in the LDS tables */) {
    static_assert(flavour_ok(F, LF_OF_TEST_PRIM), "see flavour_ok");
    constexpr bool COUNTERS = F & LF_COUNTERS, EXACT_ORDER = F & LF_EXACT_ORDER, FINITE_RAY = F & LF_FINITE_RAY, FROM_TAB = F & LF_FROM_TAB;
    float t;
    V3 n = mk(0, 0, 0);
    bool tangent = false;
    if (!EXACT_ORDER && ((kind << 28) | slot) == excl) return;
    if (kind == PRIM_TRI) {
        const float4 *tp = sv.tris + 3u * slot;
        float4 a = tp[0], b = tp[1], c = tp[2];
        if (COUNTERS) c_tris++;
        t = hit_triangle(mk(a.x, a.y, a.z), mk(a.w, b.x, b.y), mk(b.z, b.w, c.x), org, dir);
        n = mk(c.y, c.z, c.w);
    } else if (kind == PRIM_SPHERE) {
        float4 s;
        if (FROM_TAB) s = rec[0]; else s = sv.spheres[slot];
        if (COUNTERS) c_analytic++;
        t = hit_sphere(mk(s.x, s.y, s.z), s.w, org, dir, n, tangent);
    } else if (kind == PRIM_BOX) {
        float4 lo, hi;
        if (FROM_TAB) { lo = rec[0]; hi = rec[1]; } else { lo = sv.boxes[2u * slot]; hi = sv.boxes[2u * slot + 1u]; }
        if (COUNTERS) c_analytic++;
        t = FINITE_RAY ? hit_aab_finite(mk(lo.x, lo.y, lo.z), mk(hi.x, hi.y, hi.z), org, inv_d, n)
                       : hit_aab(mk(lo.x, lo.y, lo.z), mk(hi.x, hi.y, hi.z), org, inv_d, n);
    } else {
        float4 a, b, c, d;
        if (FROM_TAB) { a = rec[0]; b = rec[1]; c = rec[2]; d = rec[3]; }
        else { const float4 *cp = sv.cyls + 4u * slot; a = cp[0]; b = cp[1]; c = cp[2]; d = cp[3]; }
        if (COUNTERS) c_analytic++;
        t = hit_cylinder(mk(a.x, a.y, a.z), a.w, mk(b.x, b.y, b.z), mk(b.w, c.x, c.y), mk(c.z, c.w, d.x), d.y, org, dir, n);
    }
    if (!EXACT_ORDER && tangent) {
        /* a phantom hit outside its box: whether the reference sees it depends on its visiting
           order, so it never competes here; the caller re-casts the ray exactly if it could win */
        phantom_t = fminf(phantom_t, t);
        return;
    }
    bool take = (t >= kHitTMin && t < best_t);
    if (!EXACT_ORDER && t == best_t && t >= kHitTMin && hit_prim != kNoPrim) {
        /* bit-equal distance (e.g. the shared diagonal of a fan-triangulated quad): the reference
           keeps whichever it tested first */
        take = prim_order(sv, kind, slot) < prim_order(sv, hit_prim >> 28, hit_prim & 0x00ffffffu);
    }
    /* the nearest hit that does NOT win (fast traversal only): resolve_hit needs to know that nothing
       else lies between the winner and the entry of its node boxes */
    if (!EXACT_ORDER && t >= kHitTMin) runner_t = fminf(runner_t, take ? best_t : t);
    if (take) {
        best_t = t;
        hit_n = n;
        hit_prim = (kind << 28) | slot;
    }
}

/* the reference's child test (ray.cpp:788-803) as far as it can be decided after the fact: origin
   inside the box (half-open), or the slab test enters at 1e-6 <= t <= t_hit, t_hit being the distance of
   the winner W of the fast traversal (the minimum over ALL primitives, ties to the lower test rank).
   The reference's clause is "t < best at that moment"; every primitive it tested before this node has a
   lower rank than W, hence a strictly larger distance, so best > t_hit and an entry at t <= t_hit
   passes.  An entry BEYOND t_hit (a hit in front of its own node box: cylinder and sphere boxes are
   not conservative to the last ulp, and a flat box around an axis-aligned triangle rounds either way)
   passes or not depending on what was found earlier -- unless nothing else CAN have been found below it:
   t_other is the nearest other hit (runner-up or phantom), exact within 2e-4 of t_hit because the fast
   traversal tests everything in that window; an entry below t_other (and inside the window) is below
   any best the reference can have held.  Otherwise undecidable here: the caller re-casts exactly. */
enum : int { CH_ADMIT = 0, CH_REJECT = 1, CH_UNKNOWN = 2 };

ORT_D uint32_t info_index(const SceneView &sv, uint32_t prim) {
    const uint32_t kind = prim >> 28, slot = prim & 0x00ffffffu;
    return slot + ((kind == PRIM_TRI) ? 0u : (kind == PRIM_BOX) ? sv.info_box : (kind == PRIM_CYL) ? sv.info_cyl : sv.info_sphere);
}

/* A lane whose ray is finished knows its winner long before the wave gets to shade it (the other lanes are still
   traversing): it asks for the winner's PrimInfo right away, with two loads that have no register destination
   (LDS-DMA, global_load_lds_dword) and land in entries 0 and 1 of the lane's own, now idle, traversal stack.
   resolve_hit picks them up after an s_waitcnt vmcnt(0): two dependent round trips (chain word, material index)
   less on the critical path of every shading pass.  hipcc does not count these loads; its own waits only become
   conservative by them (memory returns in order). */
template <int BLOCK>
ORT_D void announce_winner(const SceneView &sv, uint32_t prim, uint32_t *lds_stack, int tid) {
    if (prim == kNoPrim) return;
    const PrimInfo *p = sv.prim_info + info_index(sv, prim);
#ifdef ORT_HOST_SIM
    lds_stack[tid] = p->chain;
    lds_stack[BLOCK + tid] = p->mat;
#else
    /* M0 = LDS byte address of the wave's 64 consecutive words of one stack entry; lane i lands at M0 + 4 i */
    const uint32_t dst = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)(lds_stack + (tid & ~63)));
    const uint32_t *q = &p->mat;
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\t"
                 "s_add_u32 m0, %3, %4\n\ts_nop 0\n\tglobal_load_lds_dword %2, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(p), "v"(q), "s"(dst), "n"(BLOCK * 4) : "scc");
#endif
}

/* the announced words of this lane (see announce_winner) */
template <int BLOCK>
ORT_D void announced_info(const uint32_t *lds_stack, int tid, uint32_t &chain, uint32_t &mat) {
#ifndef ORT_HOST_SIM
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    chain = lds_stack[tid];
    mat = lds_stack[BLOCK + tid];
}
/* CH_REJECT: never admitted whatever was found before (the ray misses the box or enters below 1e-6 from
   outside): the shapes below are invisible to this ray.  CH_UNKNOWN: enters at t_entry > t_hit with another
   hit possibly in between; t_entry is handed back in gap */
ORT_D int ref_node_verdict(V3 lo, V3 hi, V3 org, V3 inv_d, float t_hit, float t_other, float &gap) {
    if ((org.x >= lo.x && org.x < hi.x) && (org.y >= lo.y && org.y < hi.y) && (org.z >= lo.z && org.z < hi.z)) return CH_ADMIT;
    const float t = hit_aab_t(lo, hi, org, inv_d);
    if (!(t >= kHitTMin)) return CH_REJECT;
    if (t <= t_hit || (t < t_other && t < t_hit * 1.0001f)) return CH_ADMIT;
    gap = fmaxf(gap, t);
    return CH_UNKNOWN;
}

/* would the reference have reached this primitive?  Every node box on the way down must admit the
   ray (origin inside, half-open; or entered at t >= 1e-6).  Entries run from the primitive's own node
   (entry 0, the smallest box) up to the root's child.  chain_verdict_full tests them all, four at a
   time so the (divergent, L2-latency-bound) loads overlap. */
ORT_D int chain_verdict_full(const SceneView &sv, uint32_t first, uint32_t len, V3 org, V3 inv_d, float t_hit, float t_other, float &gap) {
    int verdict = CH_ADMIT;
    for (uint32_t base = 0; base < len; base += 4u) {
        float4 lo[4], hi[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            uint32_t i = base + k;
            i = (i < len) ? i : (len - 1u); /* clamp: re-tests the last entry, harmless */
            lo[k] = sv.chain_boxes[2u * (first + i)];
            hi[k] = sv.chain_boxes[2u * (first + i) + 1u];
        }
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const int v = ref_node_verdict(mk(lo[k].x, lo[k].y, lo[k].z), mk(hi[k].x, hi[k].y, hi[k].z), org, inv_d, t_hit, t_other, gap);
            verdict = (v == CH_REJECT || verdict == CH_REJECT) ? CH_REJECT : (v == CH_UNKNOWN ? CH_UNKNOWN : verdict);
        }
        if (verdict == CH_REJECT) break;
    }
    return verdict;
}

ORT_D bool in_rect_half_open(float4 lo, float4 hi, V3 org) { /* math.h:1156-1169 */
    return (org.x >= lo.x && org.x < hi.x) && (org.y >= lo.y && org.y < hi.y) && (org.z >= lo.z && org.z < hi.z);
}

/* The octree's boxes are nested (a shape grows every node it is pushed through, ray.cpp:1799-1948;
   ort_reftree.cpp verifies it per chain and sets kChainNested).  With nested boxes B_top >= ... >= B_0
   and a finite 1/d the admission tests are monotone: "origin inside" can only turn false going down, the
   entry distance max_a min(t_lo, t_hi) can only grow (each per-axis near distance is a monotone float
   function of the box bound) and the exit distance can only shrink.  So with B_j the first box from the
   top that does not contain the origin, the whole chain admits the ray  <=>  B_j and B_0 do: boxes above
   B_j contain the origin; boxes between are entered no earlier than B_j and are hit if B_0 is.
   Two slab tests instead of one per level. */
constexpr uint32_t kChainNested = 0x08000000u;
#if defined(ORT_HOST_SIM) && defined(ORT_CHAIN_CROSSCHECK)
static unsigned long long g_chain_crosschecks = 0;
#endif
ORT_D int chain_verdict(const SceneView &sv, uint32_t word, V3 org, V3 inv_d, float t_hit, float t_other, float &gap) {
#ifdef ORT_MEASURE_NO_CHAIN /* developer measurement only (wrong images): what the visibility-chain check costs, by leaving it out */
    gap = 0.0f;
    return CH_ADMIT;
#endif
    const uint32_t len = word >> 28, first = word & 0x07ffffffu;
    gap = 0.0f;
    if (len == 0u) return CH_ADMIT;
    const bool finite = (om_f32_bits(inv_d.x) & 0x7fffffffu) < 0x7f800000u && (om_f32_bits(inv_d.y) & 0x7fffffffu) < 0x7f800000u &&
                        (om_f32_bits(inv_d.z) & 0x7fffffffu) < 0x7f800000u;
    if (ORT_RARE(!(word & kChainNested) || !finite)) return chain_verdict_full(sv, first, len, org, inv_d, t_hit, t_other, gap);
    const float4 dlo = sv.chain_boxes[2u * first], dhi = sv.chain_boxes[2u * first + 1u];
    float4 jlo = dlo, jhi = dhi;
    bool found = false;
#ifndef ORT_CHAIN_ROUND
#define ORT_CHAIN_ROUND 2 /* boxes fetched per step of the (rare) scan below */
#endif
    if (len >= 2u) {
        /* ONE round of loads settles nearly every chain: the leaf box (above), its parent (entry 1), the top two
           ancestors (entries len-1, len-2).  Origin inside the parent: inside every ancestor (nested), none to enter.
           Otherwise the first box from the top that does not contain it is the top one, the next, or -- a long chain
           with the origin inside its top two boxes -- found by scanning on down; the parent at the latest. */
        const uint32_t it = len - 1u, it1 = (len >= 3u) ? len - 2u : 1u;
        const float4 plo = sv.chain_boxes[2u * (first + 1u)], phi = sv.chain_boxes[2u * (first + 1u) + 1u];
        const float4 tlo = sv.chain_boxes[2u * (first + it)], thi = sv.chain_boxes[2u * (first + it) + 1u];
        const float4 ulo = sv.chain_boxes[2u * (first + it1)], uhi = sv.chain_boxes[2u * (first + it1) + 1u];
        if (!in_rect_half_open(plo, phi, org)) {
            found = true;
            if (!in_rect_half_open(tlo, thi, org)) { jlo = tlo; jhi = thi; }
            else if (!in_rect_half_open(ulo, uhi, org)) { jlo = ulo; jhi = uhi; }
            else {
                jlo = plo; jhi = phi;
                bool hit = false;
                for (int32_t top = (int32_t)len - 3; ORT_RARE(!hit && top >= 2); top -= ORT_CHAIN_ROUND) {
                    float4 lo[ORT_CHAIN_ROUND], hi[ORT_CHAIN_ROUND];
#pragma unroll
                    for (int32_t k = 0; k < ORT_CHAIN_ROUND; ++k) {
                        int32_t i = top - k;
                        i = (i > 2) ? i : 2; /* clamp: re-tests entry 2, harmless */
                        lo[k] = sv.chain_boxes[2u * (first + (uint32_t)i)];
                        hi[k] = sv.chain_boxes[2u * (first + (uint32_t)i) + 1u];
                    }
#pragma unroll
                    for (int32_t k = 0; k < ORT_CHAIN_ROUND; ++k) {
                        const bool outside = !in_rect_half_open(lo[k], hi[k], org);
                        if (!hit && outside) { jlo = lo[k]; jhi = hi[k]; hit = true; }
                    }
                }
            }
        }
    }
#if defined(ORT_HOST_SIM) && defined(ORT_CHAIN_STATS)
    { int jj = -1; for (int32_t i = (int32_t)len - 1; i >= 1; --i) if (!in_rect_half_open(sv.chain_boxes[2u*(first+i)], sv.chain_boxes[2u*(first+i)+1u], org)) { jj = (int)len - 1 - i; break; }
      g_cs[0][len]++; g_cs[1][jj < 0 ? 15 : jj]++; }
#endif
    /* found: an ancestor that does not contain the origin must be entered at t >= 1e-6.  Then, and when every
       ancestor contains the origin, the leaf box decides the rest (origin inside it, or the bounds on its entry
       distance): the entry distance only grows down the chain */
    int verdict = CH_ADMIT;
    if (found && !(hit_aab_t(mk(jlo.x, jlo.y, jlo.z), mk(jhi.x, jhi.y, jhi.z), org, inv_d) >= kHitTMin)) verdict = CH_REJECT;
    else verdict = ref_node_verdict(mk(dlo.x, dlo.y, dlo.z), mk(dhi.x, dhi.y, dhi.z), org, inv_d, t_hit, t_other, gap);
#if defined(ORT_HOST_SIM) && defined(ORT_CHAIN_CROSSCHECK) /* tools/host_sim: the shortcut against the full walk, every ray */
    {
        float g2 = 0.0f;
        if (verdict != chain_verdict_full(sv, first, len, org, inv_d, t_hit, t_other, g2)) { fprintf(stderr, "chain shortcut disagrees with the full walk\n"); abort(); }
        g_chain_crosschecks++;
    }
#endif
    return verdict;
}

/* exact fallback: raycast_bvh (ray.cpp:624-822) emulated literally on the reference-compatible
   octree -- breadth-first, children in slot order, records in push order, a child admitted when
   the origin is inside it or 1e-6 <= t_entry < best AT THAT MOMENT.  The reference never reuses
   queue memory within a ray; the emulation appends to one queue of the pool in HBM (a ray enqueues a node
   at most once, so ref_node_count entries are enough).
   Returns false if the queue overflowed (the render call then fails). */
template <bool COUNTERS>
ORT_D bool ref_raycast_bfs(const SceneView &sv, V3 org, V3 dir, V3 inv_d, uint32_t *queue, float &best_t, V3 &hit_n,
                           uint32_t &hit_prim, unsigned long long &c_nodes, unsigned long long &c_tris,
                           unsigned long long &c_analytic) {
    best_t = 3.402823466e+38f;
    hit_n = mk(0, 0, 0);
    hit_prim = kNoPrim;
    float unused = 0;
    uint32_t head = 0, tail = 0;
    bool ok = true;
    const uint32_t cap = sv.cold->bfs_queue_cap;
    queue[tail++] = 0;
    while (head != tail) {
        uint32_t node = queue[head++];
        const float4 *np = sv.cold->ref_nodes + 3u * node;
        float4 a = np[0], b = np[1], c = np[2];
        int32_t first_child = (int32_t)om_f32_bits(a.w);
        uint32_t rec_first = om_f32_bits(b.w), rec_count = om_f32_bits(c.x);
        for (uint32_t r = 0; r < rec_count; ++r) {
            uint32_t rec = sv.cold->ref_recs[rec_first + r];
            test_prim<lf_if(COUNTERS, LF_COUNTERS) | LF_EXACT_ORDER>(sv, rec >> 28, rec & 0x00ffffffu, org, dir, inv_d, best_t, hit_n, hit_prim, unused, unused, c_tris, c_analytic);
        }
        if (first_child >= 0) {
            for (uint32_t k = 0; k < 8u; ++k) {
                uint32_t ci = (uint32_t)first_child + k;
                const float4 *cp = sv.cold->ref_nodes + 3u * ci;
                float4 ca = cp[0], cb = cp[1], cc = cp[2];
                uint32_t flags = om_f32_bits(cc.y);
                bool leaf_with_records = (flags & 3u) == 3u;
                bool has_children = (int32_t)om_f32_bits(ca.w) >= 0;
                if (!(leaf_with_records || has_children)) continue;
                V3 lo = mk(ca.x, ca.y, ca.z), hi = mk(cb.x, cb.y, cb.z);
                bool add = (org.x >= lo.x && org.x < hi.x) && (org.y >= lo.y && org.y < hi.y) && (org.z >= lo.z && org.z < hi.z);
                if (!add) {
                    float t = hit_aab_t(lo, hi, org, inv_d);
                    if (COUNTERS) c_nodes++;
                    add = (t >= kHitTMin && t < best_t);
                }
                if (add) {
                    if (tail >= cap) { ok = false; continue; }
                    queue[tail++] = ci;
                }
            }
        }
    }
    ORT_COUNT(sv.cold->fallback_counters + kDiagFallback, (unsigned long long)tail); /* diagnostics (ORT_DEBUG_FALLBACK): nodes enqueued */
    return ok;
}

/* ---- the lane: path state, hit resolution, ray production, traversal ------------------------
 * Shared by the two execution modes:
 *   persistent: one kernel, every lane loops  produce_ray <-> traverse  (pt_persistent)
 *   wavefront : path state lives in HBM; wf_shade runs produce_ray once per slot, wf_trace
 *               runs traverse + resolve_hit once per slot, alternating over all slots. */
struct Counters {
    unsigned long long paths = 0, rays = 0, nodes = 0, tris = 0, analytic = 0;
};

/* job bookkeeping is packed (image sizes and chunk counts fit 16 bits; checked on the host) so that
   few registers stay live across the traversal loop */
struct PathState {
    int ps = PS_NEED_JOB;
    uint32_t rng = 0, job_index = 0; /* job_index: the explicit job; in a batch of views (the VIEWS kernels, implicit job spaces) the view:
                                        whose camera, seed and frame the job belongs to */
    uint32_t pxy = 0;  /* px | py << 16: the pixel being rendered */
    uint32_t jxx = 0;  /* jx0 | jx1 << 16: the job rect's x range */
    uint32_t jyp = 0;  /* jy1 | plane << 16: the rect's end row; CHUNK policy: which partial plane */
    uint32_t spp = 0, sample = 0;
    V3 color, org, dir, wo, weight;
    bool primary = true;
};

/* what a lane of an adaptive radiance query or an adaptive camera render keeps besides its PathState (produce_ray's ADAPT flag):
   no other kernel has these.  radiance_adaptive_rays holds it in registers, pt_adaptive in LDS beside the focal cache */
struct AdaptState {
    float q = 0;       /* Q: the running sum of squared sample luminance */
    uint32_t next = 0; /* the sample count after which the next check runs; 0: a check has said stop */
};

struct HitState {
    float best_t = 0;
    V3 hit_n;
    uint32_t hit_prim = kNoPrim;
    float phantom_t = 0;
    float runner_t = 0; /* nearest hit other than the winner, exact below best_t * 1.0002 (kCullSlack) */
    uint32_t hit_mat = 0; /* material index of hit_prim, 0 = no hit: set by resolve_hit */
};

/* position of pixel (x, y) in this shard's packed block layout [local block][pixel in block]: blocks are numbered
   row-major over the block grid and dealt round-robin, so the shard's k-th block is block shard_index + k * shard_count */
ORT_D size_t packed_index(const RenderHot &rv, uint32_t x, uint32_t y) {
    const uint32_t blk = ((y >> 3) - rv.c->block_y0) * rv.c->blocks_w + ((x >> 3) - rv.c->block_x0);
    return (size_t)((blk - rv.c->shard_index) / rv.c->shard_count) * 64u + ((y & 7u) << 3) + (x & 7u);
}
/* where a job writes pixel (x, y): its partial plane (CHUNK; packed, so a shard keeps 1/N of a frame per plane) or
   the output image (full frame, or packed on request) */
ORT_D float *pixel_ptr(const RenderHot &rv, uint32_t plane, uint32_t x, uint32_t y) {
    if (rv.mode == JOBS_CHUNK) return rv.c->partial + ((size_t)plane * rv.c->my_blocks * 64u + packed_index(rv, x, y)) * 3u;
    if (rv.c->packed_out) return rv.c->out + packed_index(rv, x, y) * 3u;
    return rv.c->out + 3u * ((size_t)y * (size_t)rv.W + (size_t)x);
}

/* the same in a batch of views (the VIEWS kernels): set `view` of the partial planes, frame `view` of the output; never packed,
   never sharded */
ORT_D float *view_pixel_ptr(const RenderHot &rv, uint32_t view, uint32_t plane, uint32_t x, uint32_t y) {
    if (rv.mode == JOBS_CHUNK) return rv.c->partial + (((size_t)view * rv.c->nchunks + plane) * rv.c->my_blocks * 64u + packed_index(rv, x, y)) * 3u;
    return rv.c->out + 3u * (((size_t)view * (size_t)rv.H + (size_t)y) * (size_t)rv.W + (size_t)x);
}

/* traversal state of one ray on the fast tree */
struct Trav {
    uint32_t cur = 0;
    int sp = 0;
    V3 inv_d;
};

ORT_D void reset_hit(HitState &h, float best_t) {
    h.best_t = best_t;
    h.hit_n = mk(0, 0, 0);
    h.hit_prim = kNoPrim;
    h.phantom_t = __builtin_inff(); /* none yet; compared with <= against best_t (<= FLT_MAX) */
    h.runner_t = __builtin_inff();
}

/* the analytic prologue (ort_tree.cpp): the lanes that start a ray now all test the same shape at the same
   time -- uniform addresses, no divergence -- and enter the tree with best_t already set */
template <uint32_t F>
ORT_D void prologue_tests(const SceneView &sv, const float4 *tab, V3 org, V3 dir, V3 inv_d, HitState &h, Counters &c, uint32_t excl = kNoPrim) {
    static_assert(flavour_ok(F, LF_OF_PROLOGUE), "see flavour_ok");
    constexpr bool COUNTERS = F & LF_COUNTERS, TABS = F & LF_TABS, HAS_EXCL = F & LF_HAS_EXCL;
    constexpr uint32_t SHAPE = (F & LF_COUNTERS) | lf_if(TABS, LF_FROM_TAB); /* test_prim's flavour for a prologue shape */
    /* TABS: the shapes' records come from the LDS tables */
    const float4 *pb = nullptr, *ps = nullptr, *pc = nullptr; /* formed under TABS only: tab is null without them */
    if (TABS) { pb = tab + kTabPro; ps = pb + 2u * sv.pro_boxes; pc = ps + sv.pro_spheres; }
    /* boxes: when every lane's origin and 1/d are finite (all but a handful of rays), the slab test runs on the
       hardware's min / max (hit_aab_finite: same values); wave-uniform choice, so no lane waits for the other form */
#ifndef ORT_PROLOGUE_DEFER
#define ORT_PROLOGUE_DEFER 1 /* 0: every box test works out its normal (A/B builds; same results) */
#endif
    if (!ORT_PROLOGUE_DEFER && ORT_BALLOT(!all_finite6(org, inv_d)) == 0ull) {
        for (uint32_t i = 0; i < sv.pro_boxes; ++i)
            test_prim<SHAPE | LF_FINITE_RAY>(sv, PRIM_BOX, i, org, dir, inv_d, h.best_t, h.hit_n, h.hit_prim, h.phantom_t, h.runner_t, c.tris, c.analytic, excl, TABS ? pb + 2u * i : nullptr);
    } else
    if (ORT_BALLOT(!all_finite6(org, inv_d)) == 0ull) {
        /* distances only while the boxes compete (test_prim's rule: accept 1e-6 <= t < best, equal distances by reference
           test order, the runner-up kept); the entering face's normal is worked out once, below, for the box that won */
        for (uint32_t i = 0; i < sv.pro_boxes; ++i) {
            float4 lo, hi;
            if (TABS) { lo = pb[2u * i]; hi = pb[2u * i + 1u]; } else { lo = sv.boxes[2u * i]; hi = sv.boxes[2u * i + 1u]; }
            const uint32_t prim = ((uint32_t)PRIM_BOX << 28) | i;
            if (COUNTERS && (!HAS_EXCL || prim != excl)) c.analytic++;
            float t = hit_aab_t_finite(mk(lo.x, lo.y, lo.z), mk(hi.x, hi.y, hi.z), org, inv_d);
            if (HAS_EXCL && ORT_RARE(prim == excl)) t = -1.0f;
            bool take = (t >= kHitTMin && t < h.best_t);
            if (ORT_RARE(t == h.best_t && t >= kHitTMin && h.hit_prim != kNoPrim))
                take = prim_order(sv, PRIM_BOX, i) < prim_order(sv, h.hit_prim >> 28, h.hit_prim & 0x00ffffffu);
            if (t >= kHitTMin) h.runner_t = fminf(h.runner_t, take ? h.best_t : t);
            if (take) { h.best_t = t; h.hit_prim = prim; }
        }
        if ((h.hit_prim >> 28) == PRIM_BOX && h.hit_prim != kNoPrim) { /* reset_hit precedes every prologue: a box winner here is one of these */
            const uint32_t i = h.hit_prim & 0x00ffffffu;
            float4 lo, hi;
            if (TABS) { lo = pb[2u * i]; hi = pb[2u * i + 1u]; } else { lo = sv.boxes[2u * i]; hi = sv.boxes[2u * i + 1u]; }
            V3 n = mk(0, 0, 0);
            (void)hit_aab_finite(mk(lo.x, lo.y, lo.z), mk(hi.x, hi.y, hi.z), org, inv_d, n);
            h.hit_n = n;
        }
    } else {
        for (uint32_t i = 0; i < sv.pro_boxes; ++i)
            test_prim<SHAPE>(sv, PRIM_BOX, i, org, dir, inv_d, h.best_t, h.hit_n, h.hit_prim, h.phantom_t, h.runner_t, c.tris, c.analytic, excl, TABS ? pb + 2u * i : nullptr);
    }
    for (uint32_t i = 0; i < sv.pro_spheres; ++i)
        test_prim<SHAPE>(sv, PRIM_SPHERE, i, org, dir, inv_d, h.best_t, h.hit_n, h.hit_prim, h.phantom_t, h.runner_t, c.tris, c.analytic, excl, TABS ? ps + i : nullptr);
    for (uint32_t i = 0; i < sv.pro_cyls; ++i)
        test_prim<SHAPE>(sv, PRIM_CYL, i, org, dir, inv_d, h.best_t, h.hit_n, h.hit_prim, h.phantom_t, h.runner_t, c.tris, c.analytic, excl, TABS ? pc + 4u * i : nullptr);
}

#ifndef ORT_HOST_SIM
/* ---- the same walk, by the wave -------------------------------------------------------------------------------
 * One lane's ray (lane `leader`), walked by all the lanes that are active with it (the others of resolve_hit's callers:
 * any subset, at least the leader).  The order-dependent part of raycast_bvh is "best at that moment": a node's records
 * are tested against the best so far, its children are admitted against the best after its records, nodes are taken in
 * queue order.  Nodes are still taken one at a time, in order; what the lanes share is the work inside a node:
 *   records: one per lane, each against the best so far; the sequential rule (take when t < best, strictly) ends with
 *            the smallest t, the earliest record among equals -- picked here from the lanes that would take theirs;
 *   children: one per lane, all eight against the same best (nothing changes it between them); the admitted ones are
 *            appended in slot order by the leader lane, which is also the only lane that reads the queue (program
 *            order of ONE thread keeps its stores and loads of the queue coherent).
 * A node then costs about four dependent round trips instead of one per record and per child: on the 1M-triangle
 * scene the walks took 10 % of the launch (one lane walking, 63 waiting) before this. */
ORT_D float wave_bcast(float v, int lane) { return om_bits_f32((uint32_t)__builtin_amdgcn_readlane((int)om_f32_bits(v), lane)); }
ORT_D uint32_t wave_bcast(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }
ORT_D uint32_t lane_rank(unsigned long long mask) { /* set bits of mask below this lane */
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

template <bool COUNTERS>
ORT_D bool ref_raycast_bfs_wave(const SceneView &sv, const int leader, V3 org_l, V3 dir_l, V3 inv_l, uint32_t *queue, float &out_t, V3 &out_n,
                                uint32_t &out_prim, unsigned long long &c_nodes, unsigned long long &c_tris, unsigned long long &c_analytic) {
    /* the leader's ray, in VECTOR registers of every lane (the empty asm hides their uniformity: as scalars they would
       crowd the scalar register file, whose spills land in the hot code around this rare region) */
    V3 org = mk(wave_bcast(org_l.x, leader), wave_bcast(org_l.y, leader), wave_bcast(org_l.z, leader));
    V3 dir = mk(wave_bcast(dir_l.x, leader), wave_bcast(dir_l.y, leader), wave_bcast(dir_l.z, leader));
    V3 inv_d = mk(wave_bcast(inv_l.x, leader), wave_bcast(inv_l.y, leader), wave_bcast(inv_l.z, leader));
    asm volatile("" : "+v"(org.x), "+v"(org.y), "+v"(org.z), "+v"(dir.x), "+v"(dir.y), "+v"(dir.z), "+v"(inv_d.x), "+v"(inv_d.y), "+v"(inv_d.z));
    const unsigned long long active = __ballot(true);
    const uint32_t n_active = (uint32_t)__popcll(active), rank = lane_rank(active);
    const bool is_leader = ORT_LANE() == leader;
    /* wave-uniform state of the walk */
    float best_t = 3.402823466e+38f;
    int win_lane = -1;            /* the lane that holds the best hit's normal and primitive (keep_*) */
    V3 keep_n = mk(0, 0, 0);
    uint32_t keep_prim = kNoPrim;
    uint32_t head = 0, tail = 1;
    bool ok = true;
    const uint32_t cap = sv.cold->bfs_queue_cap;
    if (is_leader) queue[0] = 0;
    while (head != tail) {
        uint32_t node_v = 0;
        if (is_leader) node_v = queue[head];
        const uint32_t node = wave_bcast(node_v, leader);
        head++;
        const float4 *np = sv.cold->ref_nodes + 3u * node;
        const float4 a = np[0], b = np[1], c = np[2];
        const int32_t first_child = (int32_t)om_f32_bits(a.w);
        const uint32_t rec_first = om_f32_bits(b.w), rec_count = om_f32_bits(c.x);
        for (uint32_t r0 = 0; r0 < rec_count; r0 += n_active) {
            float t = best_t, unused = 0;
            V3 n = mk(0, 0, 0);
            uint32_t prim = kNoPrim;
            if (r0 + rank < rec_count) {
                const uint32_t rec = sv.cold->ref_recs[rec_first + r0 + rank];
                test_prim<lf_if(COUNTERS, LF_COUNTERS) | LF_EXACT_ORDER>(sv, rec >> 28, rec & 0x00ffffffu, org, dir, inv_d, t, n, prim, unused, unused, c_tris, c_analytic);
            }
            /* the lanes that would take their record: the smallest distance wins, the lowest lane (= earliest record) among equals */
            unsigned long long takers = __ballot(prim != kNoPrim);
            if (takers != 0ull) {
                int w = -1;
                float m = 0.0f;
                while (takers != 0ull) {
                    const int j = __ffsll(takers) - 1;
                    takers &= takers - 1ull;
                    const float tj = wave_bcast(t, j);
                    if (w < 0 || tj < m) { m = tj; w = j; }
                }
                best_t = m;
                win_lane = w;
                if (ORT_LANE() == w) { keep_n = n; keep_prim = prim; }
            }
        }
        if (first_child >= 0) {
            for (uint32_t k0 = 0; k0 < 8u; k0 += n_active) {
                const uint32_t k = k0 + rank;
                bool add = false;
                if (k < 8u) {
                    const float4 *cp = sv.cold->ref_nodes + 3u * ((uint32_t)first_child + k);
                    const float4 ca = cp[0], cb = cp[1], cc = cp[2];
                    const uint32_t flags = om_f32_bits(cc.y);
                    const bool leaf_with_records = (flags & 3u) == 3u;
                    const bool has_children = (int32_t)om_f32_bits(ca.w) >= 0;
                    if (leaf_with_records || has_children) {
                        const V3 lo = mk(ca.x, ca.y, ca.z), hi = mk(cb.x, cb.y, cb.z);
                        add = (org.x >= lo.x && org.x < hi.x) && (org.y >= lo.y && org.y < hi.y) && (org.z >= lo.z && org.z < hi.z);
                        if (!add) {
                            const float t = hit_aab_t(lo, hi, org, inv_d);
                            if (COUNTERS) c_nodes++;
                            add = (t >= kHitTMin && t < best_t);
                        }
                    }
                }
                const unsigned long long admitted = __ballot(add);
                const uint32_t n_add = (uint32_t)__popcll(admitted);
                if (is_leader) { /* in lane order = slot order */
                    unsigned long long m2 = admitted;
                    uint32_t at = tail;
                    while (m2 != 0ull) {
                        const int j = __ffsll(m2) - 1;
                        m2 &= m2 - 1ull;
                        const uint32_t kk = k0 + (uint32_t)__popcll(active & ((1ull << j) - 1ull));
                        if (at < cap) queue[at++] = (uint32_t)first_child + kk;
                    }
                }
                if (tail + n_add > cap) { ok = false; tail = cap; } else tail += n_add;
            }
        }
    }
    V3 hit_n = mk(0, 0, 0);
    uint32_t hit_prim = kNoPrim;
    if (win_lane >= 0) {
        hit_n = mk(wave_bcast(keep_n.x, win_lane), wave_bcast(keep_n.y, win_lane), wave_bcast(keep_n.z, win_lane));
        hit_prim = wave_bcast(keep_prim, win_lane);
    }
    if (is_leader) {
        ORT_COUNT(sv.cold->fallback_counters + kDiagFallback, (unsigned long long)tail);
        out_t = best_t; out_n = hit_n; out_prim = hit_prim;
    }
    return ok;
}
#endif /* !ORT_HOST_SIM */

/* the exact answer: raycast_bvh emulated literally on the reference-compatible octree.  Rare.  The lanes of a
   wave that need it take turns (wave-uniform loop over the ballot), so a wave never has more than one lane
   holding or waiting for a queue of the pool: a waiting lane can only wait for holders in other waves, which
   are running, never for a lane of its own wave parked at a reconvergence point.  The fences order the queue's
   contents across holders on different XCDs (each XCD has its own L2). */
template <bool COUNTERS>
ORT_D void recast_exactly(const SceneView &sv, bool need, V3 org, V3 dir, V3 inv_d, uint32_t lane_id, HitState &h, Counters &c) {
#ifdef ORT_MEASURE_NO_RECAST /* developer measurement only (wrong images): what the exact fallback costs, by leaving it out */
    return;
#endif
    unsigned long long pending = ORT_BALLOT(need);
    while (ORT_RARE(pending != 0ull)) {
        const int leader = ORT_FFS64(pending) - 1;
        uint32_t slot = 0;
        if (ORT_LANE() == leader) {
            ORT_COUNT(sv.cold->fallback_counters, 1ull); /* straight to memory, no register kept across the loop */
            /* a queue of the pool: look before trying (a plain load does not serialise in L2 the way an atomic on a
               contended line does) and back off between looks.  Without the back-off the lanes that wait slow the
               breadth-first walks that hold the queues down (every load of theirs queues up behind the atomics), which
               makes more lanes wait: on a long launch over a 1M-triangle scene that feedback halved the throughput */
            slot = ((lane_id * 2654435761u) >> 8) % sv.cold->bfs_queue_count;
            while (ORT_PEEK(sv.cold->bfs_locks + slot * kBfsLockStride) != 0u || !ORT_TRY_LOCK(sv.cold->bfs_locks + slot * kBfsLockStride)) {
                ORT_COUNT(sv.cold->fallback_counters + kDiagFallback + 2, 1ull); /* diagnostics (ORT_DEBUG_FALLBACK): busy queues met */
                slot = (slot + 1u) % sv.cold->bfs_queue_count;
                ORT_BACKOFF();
            }
        }
        ORT_FENCE();
#ifdef ORT_HOST_SIM
        const bool ok = ref_raycast_bfs<COUNTERS>(sv, org, dir, inv_d, sv.cold->bfs_pool + (size_t)slot * sv.cold->bfs_queue_cap, h.best_t, h.hit_n,
                                                  h.hit_prim, c.nodes, c.tris, c.analytic);
#else
        /* the lanes that are here with the leader walk its ray together (ref_raycast_bfs_wave) */
        slot = wave_bcast(slot, leader);
        const bool ok = ref_raycast_bfs_wave<COUNTERS>(sv, leader, org, dir, inv_d, sv.cold->bfs_pool + (size_t)slot * sv.cold->bfs_queue_cap, h.best_t, h.hit_n,
                                                       h.hit_prim, c.nodes, c.tris, c.analytic);
#endif
        ORT_FENCE();
        if (ORT_LANE() == leader) {
            if (!ok) ORT_COUNT(sv.cold->fallback_counters + 1, 1ull);
            ORT_UNLOCK(sv.cold->bfs_locks + slot * kBfsLockStride);
        }
        pending &= pending - 1ull;
    }
}

/* ray.cpp:1215-1221: the point on the focal plane through the centre of pixel pxy = x | y << 16 */
ORT_D V3 focal_point(const RenderHot &rv, uint32_t pxy, V3 cam_p, V3 cam_x, V3 cam_y, V3 cam_z, float focal_length) {
    float fx = (2.0f * (int)(pxy & 0xffffu) / (float)rv.W) - 1.0f; /* i32 -> f32, as the reference's x, y */
    float fy = (2.0f * (int)(pxy >> 16) / (float)rv.H) - 1.0f;
    V3 to_pixel = normalize(sub(add(scale(fx, cam_x), scale(fy, cam_y)), cam_z));
    return add(cam_p, scale(focal_length, to_pixel));
}

/* VIEWS: the camera of view v as the table holds it (RenderView::views).  Read where it is needed -- once per pixel for the
   focal point, once per camera sample for the aperture point -- instead of held in twelve registers through the traversal loop:
   64 bytes that every lane of a wave almost always shares, from L1 / L2, per path of hundreds of node tests */
struct ViewCamera { V3 p, x, y, z; };
ORT_D ViewCamera load_view_camera(const RenderHot &rv, uint32_t v) {
    const float4 *q = rv.c->views + 4u * (size_t)v;
    const float4 a = q[0], b = q[1], c = q[2], d = q[3];
    ViewCamera cam;
    cam.p = mk(a.x, a.y, a.z);
    cam.x = mk(b.x, b.y, b.z);
    cam.y = mk(c.x, c.y, c.z);
    cam.z = mk(d.x, d.y, d.z);
    return cam;
}
/* ... and what produce_ray computes from sv.cam, from it: the pixel's focal point (ray.cpp:1198, :1215-1221) and the point on
   the aperture (ray.cpp:1233-1239), the same expressions in the same order */
ORT_D V3 view_focal_point(const RenderHot &rv, uint32_t pxy, const ViewCamera &cam) {
    return focal_point(rv, pxy, cam.p, cam.x, cam.y, cam.z, len(sub(cam.p, mk(0, 0, 0.2f))));
}
ORT_D V3 view_aperture_point(const ViewCamera &cam, float aperture, float cs, float sn) {
    return sub(add(add(cam.p, scale(aperture * cs, cam.x)), scale(aperture * sn, cam.y)), scale(0.1f, cam.z));
}

#ifndef ORT_HOST_SIM
/* Job indices for the lanes of this wave that need one now (the active lanes).  The wave draws them from next_job in
   batches -- one returned device-scope atomic, a few microseconds that the whole wave waits for, per job_batch jobs
   instead of one in every pass in which some lane ends a job -- and keeps the unissued part of its last batch in two
   words of LDS: pool[0] = next index, pool[1] = end of the batch.  What the batches are really for: consecutive
   indices are like jobs (block-major order: the 64 pixels of one 8x8 block under one chunk seed), so the lanes of a
   wave trace like paths and end their jobs together -- plain loop on the headline frame 4 728 -> 5 204 Mpaths/s,
   analytic scene 3 567 -> 3 886 (profiles/r03_tuning.md).  Near the end of the job space (batch_until) a wave asks
   for exactly what it needs, so that no wave sits on indices that idle lanes elsewhere could take.  Which lane runs
   which job cannot change a bit of the image (seeds belong to jobs).  No pool (wave_job_pool): one atomic per lane and draw. */
ORT_D unsigned long long draw_job(const RenderHot &rv, unsigned long long *pool) {
    if (!pool) return ORT_NEXT_JOB(rv.c->next_job);
    const unsigned long long mask = __ballot(true);
    const uint32_t n = (uint32_t)__popcll(mask);
    const uint32_t rank = lane_rank(mask);
    const unsigned long long next = ((volatile unsigned long long *)pool)[0], end = ((volatile unsigned long long *)pool)[1];
    const uint32_t avail = (uint32_t)(end - next);
    unsigned long long j = next + rank;
    if (n > avail) { /* wave-uniform */
        const uint32_t need = n - avail;
        uint32_t want = rv.c->job_batch;
        if (want < need || end >= rv.c->batch_until) want = need;
        unsigned long long base = 0ull;
        if (rank == 0u) base = atomicAdd(rv.c->next_job, (unsigned long long)want);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
        base = ((unsigned long long)hi << 32) | lo;
        if (rank >= avail) j = base + (rank - avail);
        if (rank == 0u) { ((volatile unsigned long long *)pool)[0] = base + need; ((volatile unsigned long long *)pool)[1] = base + want; }
    } else if (rank == 0u) {
        ((volatile unsigned long long *)pool)[0] = next + n;
    }
    return j;
}
/* this wave's two words of the workgroup's pool array, emptied; nullptr when draws are not batched */
ORT_D unsigned long long *wave_job_pool(const RenderHot &rv, unsigned long long *lds_pool) {
    unsigned long long *pool = lds_pool + 2u * (threadIdx.x >> 6);
    if ((threadIdx.x & 63u) == 0u) { ((volatile unsigned long long *)pool)[0] = 0ull; ((volatile unsigned long long *)pool)[1] = 0ull; }
    return rv.c->job_batch > 1u ? pool : nullptr;
}
#else
/* one simulated lane draws one index at a time (tools/host_sim.cpp passes no pool) */
ORT_D unsigned long long draw_job(const RenderHot &rv, unsigned long long *) { return ORT_NEXT_JOB(rv.c->next_job); }
#endif

/* entry j of a caller's array of 24-byte rays (o, d) or points (p, n), as three 8-byte loads (the host checks the alignment) */
struct Ray6 { V3 o, d; };
ORT_D Ray6 load_ray(const float2 *rays, unsigned long long j) {
    const float2 *r = rays + 3ull * j;
    const float2 a = r[0], b = r[1], e = r[2];
    return Ray6{mk(a.x, a.y, b.x), mk(b.y, e.x, e.y)};
}
/* the per-ray / per-point domain (include/ort.h): six finite components, |d|^2 within [0.999, 1.001]: what a primary direction
   is in the reference (for a point, n stands for d) */
ORT_D bool in_query_domain(V3 o, V3 d) {
    const float l2 = len2(d);
    return all_finite6(o, d) && l2 >= 0.999f && l2 <= 1.001f;
}
/* pixel (x, y) of a view's frame: its word index in a view-major plane, view_count frames of W * H each */
ORT_D size_t plane_index(const RenderHot &rv, uint32_t view, uint32_t x, uint32_t y) { return ((size_t)view * (size_t)rv.H + (size_t)y) * (size_t)rv.W + (size_t)x; }
/* light-group renders: pixel pxy's three words of frame (view, g) of rv.c->group_out */
ORT_D float *group_pixel_ptr(const RenderHot &rv, uint32_t view, uint32_t g, uint32_t pxy) {
    return rv.c->group_out + 3u * plane_index(rv, view * rv.c->group_count + g, pxy & 0xffffu, pxy >> 16);
}
/* path-depth renders: pixel pxy's three words of frame (view, g) of rv.c->depth_out, its word of plane (view, g) of rv.c->depth_len,
   and the bin of a depth */
ORT_D float *depth_pixel_ptr(const RenderHot &rv, uint32_t view, uint32_t g, uint32_t pxy) {
    return rv.c->depth_out + 3u * plane_index(rv, view * rv.c->depth_bins + g, pxy & 0xffffu, pxy >> 16);
}
ORT_D uint32_t *depth_len_ptr(const RenderHot &rv, uint32_t view, uint32_t g, uint32_t pxy) {
    return rv.c->depth_len + plane_index(rv, view * rv.c->depth_bins + g, pxy & 0xffffu, pxy >> 16);
}
ORT_D uint32_t depth_bin(const RenderHot &rv, uint32_t d) { const uint32_t last = rv.c->depth_bins - 1u; return d < last ? d : last; }
/* ... and the lane's depth word: the fourth row of its focal cache */
ORT_D uint32_t *depth_word(float *focal_cache, int focal_stride) { return (uint32_t *)(focal_cache + 3 * focal_stride); }
/* 8x8 block blk of the rect's block grid and pixel-in-block pin -> (x, y); outside: a pixel of an edge block that the rect does not hold */
struct BlockPixel { int x, y; bool outside; };
ORT_D BlockPixel block_pixel(const RenderHot &rv, uint32_t blk, uint32_t pin) {
    const int x = (int)((rv.c->block_x0 + blk % rv.c->blocks_w) * 8u + (pin & 7u));
    const int y = (int)((rv.c->block_y0 + blk / rv.c->blocks_w) * 8u + (pin >> 3));
    return BlockPixel{x, y, x < rv.c->x0 || x >= rv.c->x1 || y < rv.c->y0 || y >= rv.c->y1};
}
/* tests (ORT_DEBUG_FORCE_FALLBACK): this ray is re-cast exactly whatever the fast traversal found */
ORT_D bool forced_fallback(const SceneView &sv, V3 dir) {
    return sv.force_fallback_mask != 0xffffffffu && (om_f32_bits(dir.x) & sv.force_fallback_mask) == 0u;
}

/* adaptive radiance queries: the luminance of a colour, and the stopping rule after n samples with colour sum C and sum of
   squared sample luminance Q, operation by operation as include/ort.h defines them (every operation rounded on its own: the
   build contracts nothing).  The estimated standard error of the mean luminance against tolerance times the mean's magnitude,
   lum_floor standing in for the magnitude in the dark; a NaN anywhere says "keep sampling" */
ORT_D float adaptive_luminance(V3 e) { return (0.2126f * e.x + 0.7152f * e.y) + 0.0722f * e.z; }
ORT_D bool adaptive_stop(V3 C, float Q, uint32_t n, float tolerance, float lum_floor) {
    const float fn = (float)n;
    const float m = adaptive_luminance(C) / fn;
    float v = Q / fn - m * m;
    if (v < 0.0f) v = 0.0f;
    const float vm = v / (fn - 1.0f);
    const float a = m < 0.0f ? -m : m;
    const float b = a > lum_floor ? a : lum_floor;
    const float thr = tolerance * b;
    return vm <= thr * thr;
}

/* ---- produce_ray's steps ---------------------------------------------------------------------------------------------
 * One pass of the lane state machine, cut where its concerns meet: shade the hit that arrived (shade_arrival), end a job
 * (end_job), draw the next one (take_job), start a pixel (begin_pixel), draw what a new sample starts from (primary_sample) and
 * compose the next ray (compose_ray_diffuse, compose_ray_all_lobes).  Every step is a template over produce_ray's flag word and
 * reads back only the bits it uses; produce_ray (below them) keeps the loop and the control flow. */

/* the frame's one camera (sv.cam) in the form of a view's, and its focal length.  VIEWS: unused; every lane reads its view's
   camera where it needs it (load_view_camera) */
struct SceneCamera { ViewCamera v; float focal_length; };
ORT_D SceneCamera scene_camera(const SceneView &sv) {
    SceneCamera cam;
    cam.v.p = mk(sv.cam[0], sv.cam[1], sv.cam[2]);
    cam.v.x = mk(sv.cam[3], sv.cam[4], sv.cam[5]);
    cam.v.y = mk(sv.cam[6], sv.cam[7], sv.cam[8]);
    cam.v.z = mk(sv.cam[9], sv.cam[10], sv.cam[11]);
    cam.focal_length = len(sub(cam.v.p, mk(0, 0, 0.2f))); /* ray.cpp:1198 */
    return cam;
}
constexpr float kAperture = 0.1f; /* ray.cpp:1199 */

/* what one pass hands from step to step */
struct RayPass {
    bool bounce = false;
    float angle = 0.0f; /* the pass's one angle: the lobe's azimuth (bounce), the aperture angle or HEMI's azimuth (a new sample) */
    BrdfDraw draw;
    Mat m;
    V3 n, focal;
    V3 ray_o = {0, 0, 0}, ray_d = {0, 0, 0}; /* RAYS: the sample's ray as the caller gave it (HEMI: the point and its normal) */
    float hemi_c = 0.0f;                     /* HEMI: the drawn direction's cosine to the normal */
};

/* what a lane that asked for a job got */
enum JobTake { JOB_TAKEN, JOB_SKIPPED /* nothing to run in it: ask again */, JOB_NONE_LEFT, JOB_PARKED /* ray exchange: a parked path comes first */ };

/* SH: the real spherical-harmonic basis of bands 0 to 2 at the direction d = (x, y, z), in world axes and in include/ort.h's order
   and operations (ort_probe_sh), every one a separately rounded f32 operation: b[0] is b1 ... b[7] is b8; b0 is the constant kShB0 */
constexpr float kShB0 = 0.282094792f;
struct ShBasis { float b1, b2, b3, b4, b5, b6, b7, b8; };
ORT_D ShBasis sh_basis(V3 d) {
    const float x = d.x, y = d.y, z = d.z;
    ShBasis b;
    b.b1 = 0.488602512f * y; b.b2 = 0.488602512f * z; b.b3 = 0.488602512f * x;
    b.b4 = 1.092548431f * (x * y); b.b5 = 1.092548431f * (y * z); b.b6 = 0.315391565f * (3.0f * (z * z) - 1.0f);
    b.b7 = 1.092548431f * (x * z); b.b8 = 0.546274215f * (x * x - y * y);
    return b;
}
/* ... and S[j] = S[j] + b_j * e for the nine triples at q: the product rounded, then the sum; one load, add and store per word */
ORT_D void sh_add1(float *q, float b, V3 e) { q[0] = q[0] + b * e.x; q[1] = q[1] + b * e.y; q[2] = q[2] + b * e.z; }
ORT_D void sh_basis_add(float *q, V3 d, V3 e) {
    const ShBasis b = sh_basis(d);
    sh_add1(q, kShB0, e); sh_add1(q + 3, b.b1, e); sh_add1(q + 6, b.b2, e); sh_add1(q + 9, b.b3, e); sh_add1(q + 12, b.b4, e);
    sh_add1(q + 15, b.b5, e); sh_add1(q + 18, b.b6, e); sh_add1(q + 21, b.b7, e); sh_add1(q + 24, b.b8, e);
}
constexpr uint32_t kShWords = 27u; /* ORT_SH_COEFFS x rgb */
/* the point's 27 words of rv.c->sh_out; the point's index as write_ray_record forms it */
ORT_D float *sh_point_ptr(const RenderHot &rv, const PathState &P) { return rv.c->sh_out + kShWords * (((size_t)P.pxy << 32) | P.job_index); }

/* PS_HIT, a traversal has finished: ray.cpp:817 then :1251-1277 (primary) or :1355-1421 (bounce).  Returns whether the path
   bounces: then s.n, s.m, s.draw and s.angle are the bounce's.  Otherwise the sample has ended: P.sample counts it and (ADAPT) the
   stopping rule has been asked where a check is due */
template <uint32_t F>
ORT_D bool shade_arrival(const SceneView &sv, const RenderHot &rv, const float4 *tab, PathState &P, const HitState &h, Counters &c, uint32_t spp_u,
                         AdaptState *A, RayPass &s, [[maybe_unused]] const float *dir_cache = nullptr, [[maybe_unused]] int dir_stride = 0,
                         [[maybe_unused]] uint32_t *depth = nullptr /* DEPTHS: the lane's depth word */) {
    constexpr bool COUNTERS = F & LF_COUNTERS, DIFFUSE = F & LF_DIFFUSE, TABS = F & LF_TABS;
    constexpr bool ADAPT = F & LF_ADAPT, GROUPS = F & LF_GROUPS, SPPMAP = F & LF_SPPMAP, SH = F & LF_SH, DEPTHS = F & LF_DEPTHS;
    bool alive = true;
    const uint32_t hit_mat = h.hit_mat; /* resolve_hit: 0 = nothing hit */
    s.n = normalize(h.hit_n);
    ORT_SIM_RAY_HOOK((int)(P.pxy & 0xffffu), (int)(P.pxy >> 16), P.org, P.dir, h.best_t, s.n, hit_mat);
    if (COUNTERS && P.primary) c.paths++;
    if (hit_mat) {
        if (TABS) s.m = load_mat(tab + kTabMats, hit_mat);
        else s.m = load_mat(sv.materials, hit_mat);
    }
    if (!hit_mat) {
        alive = false; /* bounce miss: ray.cpp:1418-1421; primary miss: undefined in the reference, defined: terminate */
    } else if (s.m.is_light) {
        /* ray.cpp:1254-1259 (primary: unweighted, unchecked) / :1358-1371 (bounce: dropped if not finite) */
        V3 e = P.primary ? s.m.emit : had(P.weight, s.m.emit);
        if (P.primary || (!isnan3(e) && !isinf3(e))) {
            P.color = add(P.color, e);
            if constexpr (ADAPT || SPPMAP) { const float y = adaptive_luminance(e); A->q = A->q + y * y; }
            if constexpr (GROUPS) {
                const uint32_t g = rv.c->group_of_material[hit_mat];
                if (g < rv.c->group_count) {
                    float *q = group_pixel_ptr(rv, P.job_index, g, P.pxy);
                    q[0] = q[0] + e.x; q[1] = q[1] + e.y; q[2] = q[2] + e.z;
                }
            }
            if constexpr (DEPTHS) { /* the bin of the arriving ray's depth */
                float *q = depth_pixel_ptr(rv, P.job_index, depth_bin(rv, *depth), P.pxy);
                q[0] = q[0] + e.x; q[1] = q[1] + e.y; q[2] = q[2] + e.z;
            }
            if constexpr (SH) /* the sample's primary direction, from the lane's three words (produce_ray wrote them) */
                sh_basis_add(sh_point_ptr(rv, P), mk(dir_cache[0], dir_cache[dir_stride], dir_cache[2 * dir_stride]), e);
        }
        alive = false;
    } else {
        if (P.primary) {
            if (len2(s.m.kd) > 0.0f) P.weight = had(P.weight, s.m.kd); /* ray.cpp:1267-1270 */
        } else {
            /* ray.cpp:1374-1405: pdf and BSDF with the NEW surface's normal and material, the OLD wo (sic) */
            if (DIFFUSE) {
                float p = pdf_brdf<true>(s.n, P.dir, P.wo, kRoughness, s.m) * rv.rr;
                if (p > 0.000001f) {
                    V3 f = eval_scattering<true>(s.n, P.dir, P.wo, s.m, kRoughness, h.best_t);
                    P.weight = had(divs(f, p), P.weight);
                }
            } else { /* all lobes: the two calls fused, their common terms evaluated once (ort_device.h) */
                V3 f = mk(0, 0, 0);
                const float p = pdf_eval_scattering(s.n, P.dir, P.wo, s.m, kRoughness, h.best_t, rv.rr, f);
                if (p > 0.000001f) P.weight = had(divs(f, p), P.weight);
            }
            P.wo = neg(P.dir);
        }
        P.org = add(P.org, scale(h.best_t - kEps, P.dir)); /* ray.cpp:1262,1411 */
    }
    P.primary = false;
    /* ray.cpp:1280: the roulette draw happens only while the path is alive */
    const bool bounce = alive && rng_01(P.rng) < rv.rr;
    if (bounce) {
        /* sample_random_lights (ray.cpp:537-601): result unused, RNG advances */
        rng_step(P.rng);
        if (sv.light_count) {
            /* one light: x % 1 == 0.  The count is wave-uniform, so this is a scalar branch around the per-lane remainder */
            uint32_t li = 0u;
            if (sv.light_count != 1u) li = P.rng % sv.light_count;
            uint32_t is_sphere;
            if (TABS) is_sphere = ((const uint32_t *)tab)[4 * kTabLights + li];
            else is_sphere = sv.light_is_sphere[li];
            if (is_sphere) { rng_step(P.rng); rng_step(P.rng); rng_step(P.rng); rng_step(P.rng); }
        }
        ORT_UTIL(sv, 6, true);
        s.draw = sample_brdf_draw<DIFFUSE>(P.rng, kRoughness, s.m);
        s.angle = s.draw.phi;
        if constexpr (DEPTHS) *depth = *depth + 1u; /* the bounce ray is one deeper */
    } else {
        P.sample++;
        P.ps = PS_SAMPLE;
        if constexpr (DEPTHS) { /* the sample's last ray was the one that arrived; the next sample starts at the camera */
            if (rv.c->depth_len) { uint32_t *n = depth_len_ptr(rv, P.job_index, depth_bin(rv, *depth), P.pxy); *n = *n + 1u; }
            *depth = 0u;
        }
        if constexpr (ADAPT) {
            /* a check runs after sample n when n >= min_spp, n < max_spp and (n - min_spp) % check_every == 0: A->next
               counts up to it, so nothing is divided per sample */
            if (P.sample == A->next && P.sample < spp_u) {
                const uint32_t after = A->next + rv.c->ad_check_every;
                A->next = after < A->next ? 0xffffffffu : after; /* beyond 2^32: never again */
                if (adaptive_stop(P.color, A->q, P.sample, rv.c->ad_tolerance, rv.c->ad_floor)) A->next = 0u;
            }
        }
    }
    return bounce;
}

/* the samples of the job in hand, and whether the sample that just ended was its last */
template <uint32_t F>
ORT_D uint32_t job_length(const PathState &P, uint32_t spp_u, const AdaptState *A) {
    if constexpr (F & LF_SPPMAP) return A->next; /* the n of the job in hand; with none in hand (P.ps is not PS_SAMPLE) whatever the word holds decides nothing */
    else return (F & LF_IMPLICIT) ? spp_u : P.spp;
}
template <uint32_t F>
ORT_D bool job_over(const PathState &P, uint32_t job_spp, const AdaptState *A) {
    if constexpr (F & LF_ADAPT) return P.ps == PS_SAMPLE && (P.sample == job_spp || A->next == 0u); /* ... or the rule said stop */
    else return P.ps == PS_SAMPLE && P.sample == job_spp;
}

/* end_job's write-backs.  First what the job leaves (ray.cpp:1428), the mean of its samples.  ACCUM: the pixel's words, sums
   first; the mean over all its samples, this call's and the earlier ones' */
template <uint32_t F>
ORT_D V3 job_mean(const RenderHot &rv, const PathState &P, uint32_t job_spp) {
    if constexpr (F & LF_ACCUM) {
        const size_t at = plane_index(rv, P.job_index, P.pxy & 0xffffu, P.pxy >> 16);
        const uint32_t total = rv.c->ad_spp[at] + job_spp; /* n0 + add <= 1 << 24: exact in float */
        float *q = rv.c->acc_sum + 3u * at;
        q[0] = P.color.x; q[1] = P.color.y; q[2] = P.color.z;
        rv.c->ad_spp[at] = total;
        return divs(P.color, (float)total);
    } else {
        return divs(P.color, (float)((F & LF_ADAPT) ? P.sample : job_spp));
    }
}
/* RAYS: the ray's record */
template <uint32_t F>
ORT_D void write_ray_record(const RenderHot &rv, const PathState &P, const AdaptState *A, V3 o) {
    const size_t ray = ((size_t)P.pxy << 32) | P.job_index;
    if constexpr (F & LF_SH) { /* the 27 sums become means where they stand; the plain mean if asked for */
        const float fs = (float)rv.c->spp;
        float *q = sh_point_ptr(rv, P);
        for (uint32_t k = 0; k < kShWords; ++k) q[k] = q[k] / fs;
        if (rv.c->out) { float *p = rv.c->out + 3u * ray; p[0] = o.x; p[1] = o.y; p[2] = o.z; }
    } else {
        float *p = rv.c->out + 3u * ray;
        p[0] = o.x; p[1] = o.y; p[2] = o.z;
    }
    if (rv.c->final_states) rv.c->final_states[ray] = P.rng;
    if constexpr (F & LF_ADAPT) {
        if (rv.c->ad_spp) rv.c->ad_spp[ray] = P.sample;
        if (rv.c->ad_m2) rv.c->ad_m2[ray] = A->q;
    }
}
/* the pixel kinds: the pixel's colour where its kind keeps it */
template <uint32_t F>
ORT_D void write_pixel(const RenderHot &rv, const PathState &P, uint32_t job_spp, V3 o) {
    const uint32_t px = P.pxy & 0xffffu, py = P.pxy >> 16;
    if constexpr (F & LF_GROUPS) { /* JOBS_PIXEL: the G sums become means where they stand; the frame and the states if asked for */
        const float fs = (float)job_spp;
        for (uint32_t g = 0; g < rv.c->group_count; ++g) {
            float *q = group_pixel_ptr(rv, P.job_index, g, P.pxy);
            q[0] = q[0] / fs; q[1] = q[1] / fs; q[2] = q[2] / fs;
        }
        if (rv.c->out) { float *p = view_pixel_ptr(rv, P.job_index, 0u, px, py); p[0] = o.x; p[1] = o.y; p[2] = o.z; }
        if (rv.c->final_states) rv.c->final_states[plane_index(rv, P.job_index, px, py)] = P.rng;
    } else if constexpr (F & LF_DEPTHS) { /* likewise the G bin sums; the length counts stand as they are */
        const float fs = (float)job_spp;
        for (uint32_t g = 0; g < rv.c->depth_bins; ++g) {
            float *q = depth_pixel_ptr(rv, P.job_index, g, P.pxy);
            q[0] = q[0] / fs; q[1] = q[1] / fs; q[2] = q[2] / fs;
        }
        if (rv.c->out) { float *p = view_pixel_ptr(rv, P.job_index, 0u, px, py); p[0] = o.x; p[1] = o.y; p[2] = o.z; }
        if (rv.c->final_states) rv.c->final_states[plane_index(rv, P.job_index, px, py)] = P.rng;
    } else if constexpr (F & LF_ACCUM) { /* the frame is an optional plane here */
        if (rv.c->out) { float *p = view_pixel_ptr(rv, P.job_index, 0u, px, py); p[0] = o.x; p[1] = o.y; p[2] = o.z; }
    } else {
        float *p;
        if constexpr (F & LF_VIEWS) p = view_pixel_ptr(rv, P.job_index, P.jyp >> 16, px, py);
        else p = pixel_ptr(rv, P.jyp >> 16, px, py);
        p[0] = o.x; p[1] = o.y; p[2] = o.z;
    }
}
/* ADAPT, SPPMAP: the pixel's words of its view's planes, view_count frames of W * H each (JOBS_PIXEL) */
template <uint32_t F>
ORT_D void write_pixel_planes(const RenderHot &rv, const PathState &P, const AdaptState *A) {
    if constexpr (F & LF_ADAPT) {
        const size_t at = plane_index(rv, P.job_index, P.pxy & 0xffffu, P.pxy >> 16);
        if (rv.c->ad_spp) rv.c->ad_spp[at] = P.sample;
        if (rv.c->ad_m2) rv.c->ad_m2[at] = A->q;
        if (rv.c->final_states) rv.c->final_states[at] = P.rng;
    }
    if constexpr (F & LF_SPPMAP) { /* likewise, without the sample count: the caller holds it */
        const size_t at = plane_index(rv, P.job_index, P.pxy & 0xffffu, P.pxy >> 16);
        if (rv.c->ad_m2) rv.c->ad_m2[at] = A->q;
        if ((F & LF_ACCUM) || rv.c->final_states) rv.c->final_states[at] = P.rng; /* ACCUM: the state is a required plane */
    }
}
/* a tile job: on to the rect's next pixel, or the job has ended with its last */
ORT_D void next_tile_pixel(const RenderHot &rv, PathState &P) {
    uint32_t px = P.pxy & 0xffffu, py = P.pxy >> 16;
    px++;
    if (px == (P.jxx >> 16)) { px = P.jxx & 0xffffu; py++; }
    P.pxy = px | (py << 16);
    if (py == (P.jyp & 0xffffu)) {
        if (rv.mode == JOBS_EXPLICIT && rv.c->final_states) rv.c->final_states[P.job_index] = P.rng;
        P.ps = PS_NEED_JOB;
    } else {
        P.ps = PS_PIXEL;
    }
}

/* PS_SAMPLE with the job's last sample behind it: what the job computed goes where its kind keeps it, and the lane asks for a
   new job or (a tile job) goes on to its next pixel */
template <uint32_t F>
ORT_D void end_job(const RenderHot &rv, PathState &P, uint32_t job_spp, const AdaptState *A) {
    const V3 o = job_mean<F>(rv, P, job_spp);
    if constexpr (F & LF_RAYS) {
        write_ray_record<F>(rv, P, A, o);
        P.ps = PS_NEED_JOB;
    } else {
        write_pixel<F>(rv, P, job_spp, o);
        write_pixel_planes<F>(rv, P, A);
        if (F & LF_IMPLICIT) P.ps = PS_NEED_JOB; /* a one-pixel job ends with its pixel */
        else next_tile_pixel(rv, P);
    }
}

/* take_job's decodes, one per job space; false: the job holds nothing to run.
   RAYS: job j is entry j of the caller's rays.  A ray outside the per-ray domain (in_query_domain) is answered here, NaN and its
   seed, without a traversal */
template <uint32_t F>
ORT_D bool decode_ray_job(const RenderHot &rv, PathState &P, unsigned long long j) {
    const Ray6 r = load_ray(rv.c->rays, j);
    const uint32_t seed = rv.c->seeds[j];
    if (!in_query_domain(r.o, r.d)) {
        if constexpr (F & LF_SH) { /* all 27 words, and the optional mean */
            float *q = rv.c->sh_out + kShWords * (size_t)j;
            for (uint32_t k = 0; k < kShWords; ++k) q[k] = om_bits_f32(0x7fc00000u);
            if (rv.c->out) { float *p = rv.c->out + 3u * (size_t)j; p[0] = p[1] = p[2] = om_bits_f32(0x7fc00000u); }
        } else {
            float *p = rv.c->out + 3u * (size_t)j;
            p[0] = p[1] = p[2] = om_bits_f32(0x7fc00000u);
        }
        if (rv.c->final_states) rv.c->final_states[j] = seed;
        if constexpr (F & LF_ADAPT) {
            if (rv.c->ad_spp) rv.c->ad_spp[j] = 0u;
            if (rv.c->ad_m2) rv.c->ad_m2[j] = 0.0f;
        }
        return false;
    }
    P.job_index = (uint32_t)j;
    P.pxy = (uint32_t)(j >> 32);
    P.rng = seed ? seed : 1u; /* as job_seed: a zero xorshift state never leaves zero */
    return true;
}
/* JOBS_EXPLICIT: job j is the caller's tile j */
ORT_D bool decode_tile_job(const RenderHot &rv, PathState &P, unsigned long long j) {
    ort_tile_job jb = rv.c->jobs[j];
    P.job_index = (uint32_t)j;
    P.jxx = (uint32_t)jb.x0 | ((uint32_t)jb.x1 << 16);
    P.jyp = (uint32_t)jb.y1;
    P.pxy = (uint32_t)jb.x0 | ((uint32_t)jb.y0 << 16);
    P.rng = jb.rng_state; P.spp = jb.spp;
    if (jb.x1 <= jb.x0 || jb.y1 <= jb.y0) { /* empty rect: the reference loops zero times */
        if (rv.c->final_states) rv.c->final_states[P.job_index] = P.rng;
        return false;
    }
    return true;
}
/* the implicit job space: [chunk k][my 8x8 block b][pixel-in-block p], one pixel a job.  VIEWS: [view][the view's job space].
   SPPMAP, ACCUM: the job's length goes to A->next (no samples: no job), the samples the pixel has had to acc_n0 */
template <uint32_t F>
ORT_D bool decode_pixel_job(const RenderHot &rv, PathState &P, unsigned long long j, uint32_t spp_u, AdaptState *A, uint32_t &acc_n0) {
    constexpr bool IMPLICIT = F & LF_IMPLICIT, VIEWS = F & LF_VIEWS, SPPMAP = F & LF_SPPMAP, ACCUM = F & LF_ACCUM;
    [[maybe_unused]] uint32_t view_seed = 0u;
    if constexpr (VIEWS) { /* the view's seed sits in the fourth word of its table entry */
        P.job_index = (uint32_t)(j / rv.c->view_jobs);
        j = j % rv.c->view_jobs;
        view_seed = om_f32_bits(rv.c->views[4u * (size_t)P.job_index].w);
    }
    unsigned long long per_chunk = (unsigned long long)rv.c->my_blocks * 64ull;
    uint32_t k, lb, pin; /* chunk, local block, pixel in block */
    if (rv.c->block_major) {
        const uint32_t per_block = rv.c->nchunks * 64u;
        const uint32_t within = (uint32_t)(j % per_block);
        lb = (uint32_t)(j / per_block);
        k = within >> 6;
        pin = within & 63u;
    } else {
        k = (uint32_t)(j / per_chunk);
        const uint32_t rem = (uint32_t)(j % per_chunk);
        lb = rem >> 6;
        pin = rem & 63u;
    }
    const BlockPixel bp = block_pixel(rv, rv.c->shard_index + lb * rv.c->shard_count, pin);
    if (bp.outside) return false;
    const int x = bp.x, y = bp.y;
    if constexpr (SPPMAP) { /* the job's length, one word of the caller's map, cut at the cap */
        const size_t at = plane_index(rv, P.job_index, (uint32_t)x, (uint32_t)y);
        uint32_t asked;
        if constexpr (ACCUM) asked = rv.c->sample_map ? rv.c->sample_map[at] : spp_u;
        else asked = rv.c->sample_map[at];
        uint32_t n = asked < spp_u ? asked : spp_u;
        if constexpr (ACCUM) { /* ... and at what keeps the pixel's total within 1 << 24 */
            acc_n0 = rv.c->ad_spp[at];
            const uint32_t room = (1u << 24) - (acc_n0 < (1u << 24) ? acc_n0 : (1u << 24));
            n = n < room ? n : room;
        }
        if (n == 0u) return false;
        A->next = n;
    }
    uint32_t pix = (uint32_t)(y * rv.W + x), seed;
    if constexpr (VIEWS) seed = view_seed;
    else seed = rv.c->seed;
    if (!IMPLICIT) P.jxx = (uint32_t)x | ((uint32_t)(x + 1) << 16);
    P.pxy = (uint32_t)x | ((uint32_t)y << 16);
    if (rv.mode == JOBS_PIXEL) {
        P.rng = job_seed(seed, pix);
        if (!IMPLICIT) P.spp = rv.c->spp;
        P.jyp = (uint32_t)(y + 1);
    } else {
        P.rng = job_seed(seed, k * (uint32_t)(rv.W * rv.H) + pix);
        if (!IMPLICIT) P.spp = rv.c->chunk;
        P.jyp = (uint32_t)(y + 1) | (k << 16);
    }
    return true;
}

/* PS_NEED_JOB: draw_job and the decode of what it drew.  JOB_TAKEN leaves the lane at PS_PIXEL, JOB_NONE_LEFT at PS_DONE */
template <uint32_t F>
ORT_D JobTake take_job(const RenderHot &rv, PathState &P, uint32_t spp_u, uint32_t *late_flag, bool no_new_job, unsigned long long *pool, AdaptState *A,
                       uint32_t &acc_n0) {
    constexpr bool IMPLICIT = F & LF_IMPLICIT;
    if (no_new_job) return JOB_PARKED; /* ray exchange, end of the launch: this lane takes a parked path first (pt_lane_x) */
    const unsigned long long j = draw_job(rv, pool);
    if (j >= rv.c->job_count) { P.ps = PS_DONE; return JOB_NONE_LEFT; }
    if (IMPLICIT && late_flag && j >= rv.c->endgame_from) *late_flag = 1u; /* ray exchange: the launch is near its end (pt_lane_x) */
    bool taken;
    if constexpr (F & LF_RAYS) {
        taken = decode_ray_job<F>(rv, P, j);
    } else {
        if (!IMPLICIT && rv.mode == JOBS_EXPLICIT) taken = decode_tile_job(rv, P, j);
        else taken = decode_pixel_job<F>(rv, P, j, spp_u, A, acc_n0);
    }
    if (!taken) return JOB_SKIPPED;
    P.ps = PS_PIXEL;
    return JOB_TAKEN;
}

/* PS_PIXEL: the pixel's sums and counts at zero (ray.cpp:1211), or (ACCUM, a pixel that has had acc_n0 samples) as the planes hold
   them; the pixel's focal point into the lane's cache */
template <uint32_t F>
ORT_D void begin_pixel(const RenderHot &rv, PathState &P, const SceneCamera &cam, AdaptState *A, uint32_t acc_n0, float *focal_cache, int focal_stride) {
    ORT_SIM_PIXEL_HOOK((int)(P.pxy & 0xffffu), (int)(P.pxy >> 16), P.rng);
    P.color = mk(0, 0, 0); /* ray.cpp:1211 */
    P.sample = 0;
    P.ps = PS_SAMPLE;
    if constexpr (F & LF_ADAPT) { A->q = 0.0f; A->next = rv.c->ad_min_spp; }
    if constexpr (F & LF_SPPMAP) A->q = 0.0f;
    if constexpr (F & LF_ACCUM) {
        if (acc_n0) { /* a continued pixel: its stream and its sums as the planes hold them, judged no more than a material is */
            const size_t at = plane_index(rv, P.job_index, P.pxy & 0xffffu, P.pxy >> 16);
            const uint32_t state = rv.c->final_states[at];
            P.rng = state ? state : 1u; /* as job_seed: a zero xorshift state never leaves zero */
            /* + (+0): the call is chained one-sample renders whose colours are added to C, and a colour is never -0,
               so a -0 the caller stored is +0 after the first of them whatever it holds; every other value stands */
            const float *q = rv.c->acc_sum + 3u * at;
            P.color = mk(q[0] + 0.0f, q[1] + 0.0f, q[2] + 0.0f);
            if (rv.c->ad_m2) A->q = rv.c->ad_m2[at] + 0.0f;
        }
    }
    if constexpr (F & LF_GROUPS) {
        for (uint32_t g = 0; g < rv.c->group_count; ++g) {
            float *q = group_pixel_ptr(rv, P.job_index, g, P.pxy);
            q[0] = 0.0f; q[1] = 0.0f; q[2] = 0.0f;
        }
    }
    if constexpr (F & LF_DEPTHS) { /* the bin sums and, where asked for, the length counts start at zero where they stand; the first ray is the camera's */
        for (uint32_t g = 0; g < rv.c->depth_bins; ++g) {
            float *q = depth_pixel_ptr(rv, P.job_index, g, P.pxy);
            q[0] = 0.0f; q[1] = 0.0f; q[2] = 0.0f;
            if (rv.c->depth_len) *depth_len_ptr(rv, P.job_index, g, P.pxy) = 0u;
        }
        *depth_word(focal_cache, focal_stride) = 0u;
    }
    if constexpr (F & LF_SH) { /* the point's 27 sums start at +0 where they stand; focal_cache is the lane's direction words */
        float *q = sh_point_ptr(rv, P);
        for (uint32_t k = 0; k < kShWords; ++k) q[k] = 0.0f;
    } else if (focal_cache) { /* the pixel's focal point, once per pixel (persistent kernel: three floats of LDS per lane) */
        V3 f;
        if constexpr (F & LF_VIEWS) f = view_focal_point(rv, P.pxy, load_view_camera(rv, P.job_index));
        else f = focal_point(rv, P.pxy, cam.v.p, cam.v.x, cam.v.y, cam.v.z, cam.focal_length);
        focal_cache[0] = f.x; focal_cache[focal_stride] = f.y; focal_cache[2 * focal_stride] = f.z;
    }
}

/* what a lane that starts a sample draws before the pass's one sin/cos: the aperture angle (ray.cpp:1232), beside the pixel's
   focal point; RAYS: the caller's ray, and no angle; HEMI: the direction's cosine and azimuth */
template <uint32_t F>
ORT_D void primary_sample(const RenderHot &rv, PathState &P, const SceneCamera &cam, const float *focal_cache, int focal_stride, RayPass &s) {
    if constexpr (F & LF_RAYS) { /* the caller's ray; no aperture, so no angle is drawn */
        const Ray6 r = load_ray(rv.c->rays, ((unsigned long long)P.pxy << 32) | P.job_index);
        s.ray_o = r.o;
        s.ray_d = r.d;
        if constexpr (F & LF_HEMI) { /* the diffuse lobe's draw (sample_brdf_draw without the choice); its azimuth is the pass's one angle */
            const float e0 = rng_01(P.rng), e1 = rng_01(P.rng);
            if constexpr (F & LF_SH) s.hemi_c = 1.0f - 2.0f * e0; /* uniform over the sphere about the pole */
            else s.hemi_c = __builtin_sqrtf(e0); /* ray.cpp:1123 */
            s.angle = 2.0f * kPi * e1;
        }
    } else {
        /* ray.cpp:1215-1221: point on the focal plane through the pixel centre: a function of the pixel alone,
           read back from the per-lane cache or (wavefront mode) recomputed -- same expressions, same bits */
        if constexpr (F & LF_VIEWS) {
            s.focal = focal_cache ? mk(focal_cache[0], focal_cache[focal_stride], focal_cache[2 * focal_stride])
                                  : view_focal_point(rv, P.pxy, load_view_camera(rv, P.job_index));
        } else {
            s.focal = focal_cache ? mk(focal_cache[0], focal_cache[focal_stride], focal_cache[2 * focal_stride])
                                  : focal_point(rv, P.pxy, cam.v.p, cam.v.x, cam.v.y, cam.v.z, cam.focal_length);
        }
        s.angle = rng_between(P.rng, 0.0f, 2 * kPi); /* ray.cpp:1232 */
    }
}

/* where a new sample's ray starts, ray.cpp:1233-1239: the caller's origin (RAYS), or the point of the aperture at the pass's angle */
template <uint32_t F>
ORT_D V3 sample_origin(const RenderHot &rv, const PathState &P, const SceneCamera &cam, const RayPass &s, float cs, float sn) {
    if constexpr (F & LF_RAYS) {
        return s.ray_o;
    } else {
        if constexpr (F & LF_VIEWS) return view_aperture_point(load_view_camera(rv, P.job_index), kAperture, cs, sn);
        else return view_aperture_point(cam.v, kAperture, cs, sn);
    }
}
/* a new sample's ray is composed: the path starts */
ORT_D void begin_path(PathState &P, V3 ap) {
    P.org = ap;
    P.weight = mk(1, 1, 1);
    P.primary = true;
    P.ps = PS_HIT;
}

/* The next ray, from cos/sin of the pass's angle.  DIFFUSE: the leaner flavour has the registers for the wider merge; the
   all-lobes one spills on it.  Bounce lanes normalise twice here (the surface normal again, ray.cpp:1069, and the sampled
   direction, :1158) and so do camera lanes (the ray direction, :1240, and -- sic -- the direction again for wo, :1241): two
   converged evaluations instead of four divergent ones */
template <uint32_t F>
ORT_D void compose_ray_diffuse(const RenderHot &rv, PathState &P, const SceneCamera &cam, const RayPass &s, float cs, float sn) {
    constexpr bool RAYS = F & LF_RAYS, HEMI = F & LF_HEMI;
    V3 ap = mk(0, 0, 0);
    if (!s.bounce) ap = sample_origin<F>(rv, P, cam, s, cs, sn); /* ray.cpp:1233-1239 */
    const V3 unit1 = normalize(s.bounce ? s.n : (RAYS ? s.ray_d : sub(s.focal, ap)));
    bool is_trans = false;
    V3 raw = unit1;
    if (s.bounce) raw = sample_brdf_finish<false, true>(s.n, unit1, P.wo, s.m, s.draw, cs, sn, is_trans);
    if constexpr (HEMI) { if (!s.bounce) raw = sample_lobe_n(unit1, s.hemi_c, cs, sn); } /* unit1 = normalize(n), as sample_lobe's */
    const V3 unit2 = normalize(raw);
    if (s.bounce) {
        if (is_trans) P.org = add(P.org, scale(2.0f * kEps, P.dir)); /* ray.cpp:1345-1348: dir is still the arriving direction */
        P.dir = unit2;
    } else {
        if constexpr (HEMI) { /* d; wo = -normalize(d), as RAYS for the ray (p, d) */
            P.dir = unit2;
            P.wo = neg(normalize(unit2));
        } else if constexpr (RAYS) { /* the direction as given; wo = -normalize(d) */
            P.dir = s.ray_d;
            P.wo = neg(unit1);
        } else {
            P.dir = unit1;
            P.wo = neg(unit2);
        }
        begin_path(P, ap);
    }
}
/* all lobes: both branches end by normalising a direction (ray.cpp:1158 / :1240): one converged evaluation */
template <uint32_t F>
ORT_D void compose_ray_all_lobes(const RenderHot &rv, PathState &P, const SceneCamera &cam, const RayPass &s, float cs, float sn) {
    constexpr bool RAYS = F & LF_RAYS, HEMI = F & LF_HEMI;
    V3 raw, ap = mk(0, 0, 0);
    bool is_trans = false;
    if (s.bounce) {
        raw = sample_brdf_finish<false>(s.n, normalize(s.n), P.wo, s.m, s.draw, cs, sn, is_trans);
    } else {
        /* ray.cpp:1233-1246 */
        ap = sample_origin<F>(rv, P, cam, s, cs, sn);
        if constexpr (HEMI) raw = sample_lobe_n(normalize(s.ray_d), s.hemi_c, cs, sn);
        else if constexpr (RAYS) raw = s.ray_d;
        else raw = sub(s.focal, ap);
    }
    const V3 unit = normalize(raw);
    if (s.bounce) {
        if (is_trans) P.org = add(P.org, scale(2.0f * kEps, P.dir)); /* ray.cpp:1345-1348: dir is still the arriving direction */
        P.dir = unit;
    } else {
        if constexpr (RAYS && !HEMI) { /* the direction as given; wo = -normalize(d) */
            P.dir = raw;
            P.wo = neg(unit);
        } else { /* HEMI: d = unit, and wo = -normalize(d) as RAYS for the ray (p, d) */
            P.dir = unit;
            P.wo = neg(normalize(P.dir)); /* normalised again (sic) */
        }
        begin_path(P, ap);
    }
}

/* Advance the lane's path state machine until it has produced the next ray (returns true; the ray
   is P.org / P.dir) or has run out of work (returns false).  On entry with P.ps == PS_HIT, h holds
   the resolved closest hit of the ray produced by the previous call. */
template <uint32_t F> /* IMPLICIT ... ACCUM: at their names, LF_IMPLICIT ... LF_ACCUM */
ORT_D bool produce_ray(const SceneView &sv, const RenderHot &rv, const float4 *tab, PathState &P, const HitState &h, Counters &c, Prof &pr,
                       float *focal_cache = nullptr, int focal_stride = 0, uint32_t spp_u = 0, uint32_t *late_flag = nullptr, bool no_new_job = false,
                       unsigned long long *pool = nullptr, AdaptState *A = nullptr) {
    static_assert(flavour_ok(F, LF_OF_PRODUCE_RAY), "see flavour_ok");
    constexpr bool COUNTERS = F & LF_COUNTERS, DIFFUSE = F & LF_DIFFUSE, SPPMAP = F & LF_SPPMAP;
    const SceneCamera cam = scene_camera(sv);
    while (P.ps != PS_DONE) {
        ORT_UTIL(sv, 5, true);
        ORT_PHASE(pr, sv, 8, true);
        RayPass s;
        if (P.ps == PS_HIT) {
            if constexpr (F & LF_SH) s.bounce = shade_arrival<F>(sv, rv, tab, P, h, c, spp_u, A, s, focal_cache, focal_stride);
            else if constexpr (F & LF_DEPTHS) s.bounce = shade_arrival<F>(sv, rv, tab, P, h, c, spp_u, A, s, nullptr, 0, depth_word(focal_cache, focal_stride));
            else s.bounce = shade_arrival<F>(sv, rv, tab, P, h, c, spp_u, A, s);
            ORT_PHASE(pr, sv, 1, true);
        }
        if (!s.bounce) {
            /* a lane arrives here after its sample ended (PS_SAMPLE), or with nothing yet (PS_NEED_JOB).
               Pixel write-back, next pixel / next job and the new camera ray all happen in this same
               pass, so the rest of the wave does not wait through a second trip round the loop. */
            const uint32_t job_spp = job_length<F>(P, spp_u, A);
            if (job_over<F>(P, job_spp, A)) end_job<F>(rv, P, job_spp, A);
            [[maybe_unused]] uint32_t acc_n0 = 0u; /* ACCUM: the samples the pixel drawn in this pass has had; a pixel starts in the pass that draws its job */
            if (P.ps == PS_NEED_JOB) {
                const JobTake t = take_job<F>(rv, P, spp_u, late_flag, no_new_job, pool, A, acc_n0);
                if (t == JOB_PARKED) return false;
                if (t == JOB_NONE_LEFT) break;
                if (t == JOB_SKIPPED) continue;
            }
            if (P.ps == PS_PIXEL) begin_pixel<F>(rv, P, cam, A, acc_n0, focal_cache, focal_stride);
            if constexpr (!SPPMAP) { /* SPPMAP: a job in hand has n >= 1 samples and P.sample < n here: nothing to skip */
                if (P.sample == job_spp) continue; /* spp == 0: the reference's sample loop runs zero times */
            }
            primary_sample<F>(rv, P, cam, focal_cache, focal_stride, s);
            ORT_PHASE(pr, sv, 2, true);
        }
        /* lanes that bounce and lanes that start a new camera sample both need cos/sin of one angle
           (lobe azimuth / aperture angle): the double-precision evaluation happens here once,
           converged, instead of once in each branch (same operand, same bits) */
        ORT_UTIL(sv, 7, true);
        float cs, sn;
        ort_sincosf(s.angle, &sn, &cs);
        if (DIFFUSE) compose_ray_diffuse<F>(rv, P, cam, s, cs, sn);
        else compose_ray_all_lobes<F>(rv, P, cam, s, cs, sn);
        if constexpr (F & LF_SH) { /* the sample's primary direction d, for the emissions its path adds after it has bounced */
            if (!s.bounce) { focal_cache[0] = P.dir.x; focal_cache[focal_stride] = P.dir.y; focal_cache[2 * focal_stride] = P.dir.z; }
        }
        ORT_PHASE(pr, sv, 3, true);
        return true;
    }
    return false;
}


/* a child is skipped only when its entry distance (less the slab test's rounding margin, 0.9999996)
   is beyond best_t * 1.0002: every primitive hit within 2e-4 of the final winner is therefore tested,
   which is what makes HitState::runner_t exact in that window */
constexpr float kCullSlack = 0.9997996f; /* <= 0.9999996 / 1.0002 */

/* One interior node of the fast tree (record a b cc d) against the ray: both child boxes in the reference's own
   (p - o) * (1/d) form (ray.cpp:215-222) with ulp margins, conservative; fminf/fmaxf drop the NaN of 0 * inf, i.e. that
   axis is ignored.  Continues with the nearer child, stacks the farther one, or pops. */
template <bool COUNTERS, int LDS_ENTRIES, int BLOCK>
ORT_D void visit_node(float4 a, float4 b, float4 cc, float4 d, V3 org, V3 inv_d, float best_t, uint32_t &cur, int &sp, uint32_t *lds_stack,
                      uint32_t *spill, int tid, Counters &c) {
    uint32_t c0 = om_f32_bits(d.x), c1 = om_f32_bits(d.y);
    if (COUNTERS) c.nodes += 2;
    /* child 0: lo = a.xyz, hi = (a.w, b.x, b.y); child 1: lo = (b.z, b.w, cc.x), hi = cc.yzw */
    float t0x = (a.x - org.x) * inv_d.x, t1x = (a.w - org.x) * inv_d.x;
    float t0y = (a.y - org.y) * inv_d.y, t1y = (b.x - org.y) * inv_d.y;
    float t0z = (a.z - org.z) * inv_d.z, t1z = (b.y - org.z) * inv_d.z;
    float n0 = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
    float f0 = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
    float u0x = (b.z - org.x) * inv_d.x, u1x = (cc.y - org.x) * inv_d.x;
    float u0y = (b.w - org.y) * inv_d.y, u1y = (cc.z - org.y) * inv_d.y;
    float u0z = (cc.x - org.z) * inv_d.z, u1z = (cc.w - org.z) * inv_d.z;
    float n1 = fmaxf(fmaxf(fminf(u0x, u1x), fminf(u0y, u1y)), fminf(u0z, u1z));
    float f1 = fminf(fminf(fmaxf(u0x, u1x), fmaxf(u0y, u1y)), fmaxf(u0z, u1z));
    /* children with a sphere below are not culled by distance (phantom tangent hits) */
    bool h0 = (f0 * 1.0000004f >= n0) && (f0 >= 0.0f) && ((n0 * kCullSlack < best_t) || (c0 & SPHERE_BELOW_BIT));
    bool h1 = (f1 * 1.0000004f >= n1) && (f1 >= 0.0f) && ((n1 * kCullSlack < best_t) || (c1 & SPHERE_BELOW_BIT)) && (c1 != EMPTY_CHILD);
    if (h0 && h1) {
        bool swap = n1 < n0;
        uint32_t farc = swap ? c0 : c1;
        cur = swap ? c1 : c0;
        if (sp < LDS_ENTRIES) lds_stack[sp * BLOCK + tid] = farc;
        else spill[sp - LDS_ENTRIES] = farc;
        sp++;
    } else if (h0) {
        cur = c0;
    } else if (h1) {
        cur = c1;
    } else if (sp == 0) {
        cur = kTraversalDone;
    } else {
        sp--;
        /* two loads behind a branch (the volatile is meant to keep the compiler from merging them into one flat_load of a
           selected generic pointer, so that the LDS side is a plain ds_read: it does in the pt_persistent kernels; raycast_rays
           and wf_trace read the tail with flat_load all the same, profiles/r15_deep_stack.md) */
        if (sp < LDS_ENTRIES) cur = lds_stack[sp * BLOCK + tid];
        else cur = ((volatile uint32_t *)spill)[sp - LDS_ENTRIES];
    }
}

/* One interior node of the 4-wide tree (DevNode4: lo.x, lo.y, lo.z, hi.x, hi.y, hi.z of four children, four child words)
   against the ray: the same conservative slab test as visit_node per child, then the children that are hit are visited
   nearest first -- the nearest becomes the current node, the others are stacked farthest first.  Half the dependent
   fetches of the binary tree on the way down. */
template <bool COUNTERS, int LDS_ENTRIES, int BLOCK>
ORT_D void visit_node4(float4 lx, float4 ly, float4 lz, float4 hx, float4 hy, float4 hz, float4 cw, V3 org, V3 inv_d, float best_t, uint32_t &cur, int &sp,
                       uint32_t *lds_stack, uint32_t *spill, int tid, Counters &c) {
    if (COUNTERS) c.nodes += 4;
    float key0, key1, key2, key3;
    uint32_t w0, w1, w2, w3;
#define ORT_SLAB4(K, W, LX, LY, LZ, HX, HY, HZ, CW)                                                                        \
    {                                                                                                                      \
        const float t0x = ((LX) - org.x) * inv_d.x, t1x = ((HX) - org.x) * inv_d.x;                                        \
        const float t0y = ((LY) - org.y) * inv_d.y, t1y = ((HY) - org.y) * inv_d.y;                                        \
        const float t0z = ((LZ) - org.z) * inv_d.z, t1z = ((HZ) - org.z) * inv_d.z;                                        \
        const float n_ = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));                                  \
        const float f_ = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));                                  \
        const uint32_t cw_ = om_f32_bits(CW);                                                                              \
        const bool hit_ = (f_ * 1.0000004f >= n_) && (f_ >= 0.0f) && ((n_ * kCullSlack < best_t) || (cw_ & SPHERE_BELOW_BIT)) && (cw_ != EMPTY_CHILD); \
        K = hit_ ? fminf(n_, 3.402823466e+38f) : __builtin_inff(); /* a hit sorts strictly before every miss */             \
        W = hit_ ? cw_ : EMPTY_CHILD;                                                                                      \
    }
    ORT_SLAB4(key0, w0, lx.x, ly.x, lz.x, hx.x, hy.x, hz.x, cw.x)
    ORT_SLAB4(key1, w1, lx.y, ly.y, lz.y, hx.y, hy.y, hz.y, cw.y)
    ORT_SLAB4(key2, w2, lx.z, ly.z, lz.z, hx.z, hy.z, hz.z, cw.z)
    ORT_SLAB4(key3, w3, lx.w, ly.w, lz.w, hx.w, hy.w, hz.w, cw.w)
#undef ORT_SLAB4
    /* ascending by entry distance: five compare-exchanges */
#define ORT_CX(KA, WA, KB, WB)                                                                                             \
    {                                                                                                                      \
        const bool sw_ = KB < KA;                                                                                          \
        const float ka_ = sw_ ? KB : KA, kb_ = sw_ ? KA : KB;                                                              \
        const uint32_t wa_ = sw_ ? WB : WA, wb_ = sw_ ? WA : WB;                                                           \
        KA = ka_; KB = kb_; WA = wa_; WB = wb_;                                                                            \
    }
    ORT_CX(key0, w0, key1, w1)
    ORT_CX(key2, w2, key3, w3)
    ORT_CX(key0, w0, key2, w2)
    ORT_CX(key1, w1, key3, w3)
    ORT_CX(key1, w1, key2, w2)
#undef ORT_CX
    if (w0 == EMPTY_CHILD) { /* nothing hit: pop */
        if (sp == 0) {
            cur = kTraversalDone;
        } else {
            sp--;
            if (sp < LDS_ENTRIES) cur = lds_stack[sp * BLOCK + tid];
            else cur = ((volatile uint32_t *)spill)[sp - LDS_ENTRIES];
        }
        return;
    }
    cur = w0;
    if (w3 != EMPTY_CHILD) { if (sp < LDS_ENTRIES) lds_stack[sp * BLOCK + tid] = w3; else spill[sp - LDS_ENTRIES] = w3; sp++; }
    if (w2 != EMPTY_CHILD) { if (sp < LDS_ENTRIES) lds_stack[sp * BLOCK + tid] = w2; else spill[sp - LDS_ENTRIES] = w2; sp++; }
    if (w1 != EMPTY_CHILD) { if (sp < LDS_ENTRIES) lds_stack[sp * BLOCK + tid] = w1; else spill[sp - LDS_ENTRIES] = w1; sp++; }
}

/* raycast_top_most_node (ray.cpp:1165-1176): start at the root.  The lanes that start a ray now are converged: they
   test the analytic prologue together and visit the root node together, its record read from the LDS tables, before
   they join the traversal loop (whose other lanes are at arbitrary depths) */
template <uint32_t F, int LDS_ENTRIES, int BLOCK>
ORT_D void begin_ray(const SceneView &sv, const float4 *tab, const PathState &P, Trav &T, HitState &h, Counters &c, Prof &pr,
                     uint32_t *lds_stack, uint32_t *spill, int tid) {
    static_assert(flavour_ok(F, LF_OF_BEGIN_RAY), "see flavour_ok");
    [[maybe_unused]] constexpr bool COUNTERS = F & LF_COUNTERS; /* the probes' */
    T.cur = 0;
    T.sp = 0;
    T.inv_d = mk(1.0f / P.dir.x, 1.0f / P.dir.y, 1.0f / P.dir.z); /* ray.cpp:210, once per ray */
    reset_hit(h, 3.402823466e+38f); /* Flt_Max, ray.cpp:627 */
    prologue_tests<F>(sv, tab, P.org, P.dir, T.inv_d, h, c);
    ORT_PHASE(pr, sv, 4, true);
}

/* Closest hit: interruptible ordered DFS, replaces raycast_bvh (ray.cpp:624-822) on the fast tree.
 * while-while: a lane first descends interior nodes until it holds a leaf (or runs out of stack),
 * then the wave processes leaves together, so the cheap box code and the expensive primitive code
 * are not serialised against each other in every iteration.
 * Slab test: the reference's own (p - o) * (1/d) form (ray.cpp:215-222) with ulp margins,
 * conservative; fminf/fmaxf drop the NaN of 0 * inf, i.e. that axis is ignored.
 * Returns when this lane's ray is finished, or -- refill_below > 0 -- as soon as fewer than
 * refill_below lanes of the wave are still traversing (the caller resumes later: all state is in T/h). */
template <uint32_t F, int LDS_ENTRIES, int BLOCK>
ORT_D bool traverse(const SceneView &sv, V3 org, V3 dir, Trav &T, HitState &h, uint32_t *lds_stack, uint32_t *spill, int tid,
                    int refill_below, int descend_below, Counters &c, Prof &pr, uint32_t excl = kNoPrim, const float4 *tab = nullptr) {
    static_assert(flavour_ok(F, LF_OF_TRAVERSE), "see flavour_ok");
    constexpr bool COUNTERS = F & LF_COUNTERS, TREELET = F & LF_TREELET, ANNOUNCE = F & LF_ANNOUNCE, WIDE = F & LF_WIDE;
    bool tracing = true;
    uint32_t cur = T.cur;
    int sp = T.sp;
    const V3 inv_d = T.inv_d;
    ORT_SIM_STACK_HOOK(LDS_ENTRIES, sp, cur == 0u);
    while (tracing) {
        ORT_UTIL(sv, 2, true);
        ORT_PHASE(pr, sv, 9, true);
        /* the straggler threshold of this round: descend_below, but never more than a quarter of the lanes
           that start descending now (a wave that enters with 20 such lanes should not stop at 8) */
        const int entering = ORT_POPC64(ORT_BALLOT((cur & LEAF_BIT) == 0u));
        const int stragglers = descend_below < (entering >> ORT_DESCEND_SHIFT) ? descend_below : (entering >> ORT_DESCEND_SHIFT);
        while (!(cur & LEAF_BIT)) {
            ORT_UTIL(sv, 0, true);
            const uint32_t ni = cur & NODE_INDEX_MASK;
            if (WIDE) { /* sv.nodes holds the 4-wide form (DevNode4, 8 float4 each): seven 16-byte loads in flight together */
                const float4 *np = sv.nodes + 8u * ni;
                const float4 lx = np[0], ly = np[1], lz = np[2], hx = np[3], hy = np[4], hz = np[5], cw = np[6];
                visit_node4<COUNTERS, LDS_ENTRIES, BLOCK>(lx, ly, lz, hx, hy, hz, cw, org, inv_d, h.best_t, cur, sp, lds_stack, spill, tid, c);
            } else {
            float4 na, nb, nc, nd;
            if (TREELET && ni < kTreeletNodes) { /* the top of the tree: LDS */
                const float4 *np = tab + kTabTreelet + 4u * ni;
                na = np[0]; nb = np[1]; nc = np[2]; nd = np[3];
            } else {
                const float4 *np = sv.nodes + 4u * ni;
                na = np[0]; nb = np[1]; nc = np[2]; nd = np[3];
            }
            visit_node<COUNTERS, LDS_ENTRIES, BLOCK>(na, nb, nc, nd, org, inv_d, h.best_t, cur, sp, lds_stack, spill, tid, c);
            }
            ORT_SIM_STACK_HOOK(LDS_ENTRIES, sp, false);
            /* the stragglers of the descend loop would keep the rest of the wave waiting: break out
               and come back for them (their cur / sp carry over) */
            if (ORT_POPC64(ORT_BALLOT(true)) < stragglers) break;
        }
        ORT_PHASE(pr, sv, 5, true);
        if (!(cur & LEAF_BIT)) {
            /* still on an interior node after the early exit above: nothing to do this round */
        } else if (cur == kTraversalDone) {
            tracing = false;
        } else {
            ORT_UTIL(sv, 1, true);
            uint32_t kind = (cur >> 28) & 7u, count = ((cur >> 24) & 15u) + 1u, first = cur & 0x00ffffffu;
            for (uint32_t i = 0; i < count; ++i)
                test_prim<F & LF_COUNTERS>(sv, kind, first + i, org, dir, inv_d, h.best_t, h.hit_n, h.hit_prim, h.phantom_t, h.runner_t, c.tris, c.analytic, excl);
            if (sp == 0) {
                cur = kTraversalDone;
                tracing = false;
            } else {
                sp--;
                /* two loads behind a branch: see visit_node */
                if (sp < LDS_ENTRIES) cur = lds_stack[sp * BLOCK + tid];
                else cur = ((volatile uint32_t *)spill)[sp - LDS_ENTRIES];
            }
            ORT_SIM_STACK_HOOK(LDS_ENTRIES, sp, false);
            ORT_PHASE(pr, sv, 6, true);
        }
        /* finished: the winner's chain word and material are wanted next (resolve_hit), ask for them now */
        if (ANNOUNCE && !tracing) announce_winner<BLOCK>(sv, h.hit_prim, lds_stack, tid);
        /* when most of the wave has finished its ray, let the finished lanes shade and refill */
        if (refill_below > 0 && ORT_POPC64(ORT_BALLOT(tracing)) < refill_below) break;
    }
    T.cur = cur;
    T.sp = sp;
    return tracing;
}

/* After a traversal: is the winner W of the fast traversal what the reference returns (ray.cpp:788-803)?

   - W's chain admits the ray (chain_verdict): done.
   - A box of W's chain can never be entered (CH_REJECT: missed, or entered below 1e-6 from outside --
     the reference's cylinder boxes do not contain their cylinders): W is invisible to this ray whatever the
     visiting order, so the answer is the best of the OTHER shapes: one more fast traversal with W ignored,
     whose winner is checked the same way.
   - W's leaf box is entered beyond W's own distance with room for another hit in between (CH_UNKNOWN): one
     more fast traversal, limited to that entry distance and ignoring W, settles whether such a hit exists;
     if not, W stands.
   - Anything else (a phantom that could win, a second complication on the same ray): the literal
     breadth-first emulation.
   The extra traversals run here, to completion, for the lanes that need them (1e-5 of the rays of the
   reference's scenes, 1e-2 with slanted cylinders) while the rest of the wave waits: the shape to ignore is
   a local of this rare branch, not a register carried through every ray's traversal. */
template <uint32_t F, int LDS_ENTRIES, int BLOCK>
ORT_D void resolve_hit(const SceneView &sv, const float4 *tab, V3 org, V3 dir, V3 inv_d, uint32_t lane_id, HitState &h, Counters &c, Prof &pr,
                       uint32_t *lds_stack, uint32_t *spill, int tid) {
    static_assert(flavour_ok(F, LF_OF_RESOLVE_HIT), "see flavour_ok");
    constexpr bool COUNTERS = F & LF_COUNTERS, ANNOUNCED = F & LF_ANNOUNCE;
    /* the winner's chain word and material index: announced by the traversal (in the lane's stack entries 0 and 1),
       or fetched here */
    uint32_t word = 0, mat = 0;
    if (ANNOUNCED) {
        announced_info<BLOCK>(lds_stack, tid, word, mat);
    } else if (h.hit_prim != kNoPrim) {
        const PrimInfo pi = sv.prim_info[info_index(sv, h.hit_prim)];
        word = pi.chain; mat = pi.mat;
    }
    bool stale = false; /* the winner has changed since */
    bool recast = forced_fallback(sv, dir);
    if (!ORT_RARE(recast)) {
        if (ORT_RARE(h.phantom_t <= h.best_t)) {
            recast = true;
            ORT_STAT(2, 1);
        } else if (h.hit_prim != kNoPrim) {
            float gap = 0.0f;
            const int verdict = chain_verdict(sv, word, org, inv_d, h.best_t, fminf(h.runner_t, h.phantom_t), gap);
            if (ORT_RARE(verdict != CH_ADMIT)) {
                stale = true;
                ORT_STAT(3, verdict == CH_REJECT ? 0 : 1); ORT_STAT(3, 4 + (int)(h.hit_prim >> 28));
                ORT_COUNT(sv.cold->fallback_counters + kDiagFallback + 1, 1ull); /* diagnostics (ORT_DEBUG_FALLBACK): re-traversals */
                /* W waits in the lane's (idle) traversal-stack slots of LDS, not in registers */
                const uint32_t w_prim = h.hit_prim;
                uint32_t *save = lds_stack + tid;
                save[(LDS_ENTRIES - 1) * BLOCK] = om_f32_bits(h.best_t);
                save[(LDS_ENTRIES - 2) * BLOCK] = om_f32_bits(h.hit_n.x);
                save[(LDS_ENTRIES - 3) * BLOCK] = om_f32_bits(h.hit_n.y);
                save[(LDS_ENTRIES - 4) * BLOCK] = om_f32_bits(h.hit_n.z);
                Trav t2;
                t2.cur = 0; t2.sp = 0; t2.inv_d = inv_d;
                /* CH_UNKNOWN: only hits at or before the leaf box's entry matter (the hit tests' "<" must accept t == gap) */
                reset_hit(h, verdict == CH_REJECT ? 3.402823466e+38f : om_bits_f32(om_f32_bits(gap) + 1u));
                prologue_tests<(F & LF_OF_PROLOGUE) | LF_HAS_EXCL>(sv, tab, org, dir, inv_d, h, c, w_prim);
                (void)traverse<F & LF_OF_TRAVERSE & ~LF_ANNOUNCE, LDS_ENTRIES - 4, BLOCK>(sv, org, dir, t2, h, lds_stack, spill, tid, 0, 0, c, pr, w_prim);
                if (verdict == CH_UNKNOWN) {
                    if (h.hit_prim != kNoPrim || h.phantom_t <= gap) {
                        recast = true; /* something is there: order decides */
                        ORT_STAT(2, h.hit_prim != kNoPrim ? 2 : 6);
                    } else {           /* nothing there: W stands */
                        h.best_t = om_bits_f32(save[(LDS_ENTRIES - 1) * BLOCK]);
                        h.hit_n = mk(om_bits_f32(save[(LDS_ENTRIES - 2) * BLOCK]), om_bits_f32(save[(LDS_ENTRIES - 3) * BLOCK]),
                                     om_bits_f32(save[(LDS_ENTRIES - 4) * BLOCK]));
                        h.hit_prim = w_prim;
                    }
                } else if (h.phantom_t <= h.best_t) {
                    recast = true;
                    ORT_STAT(2, 3);
                } else if (h.hit_prim != kNoPrim) {
                    float gap2 = 0.0f;
                    if (chain_verdict(sv, sv.prim_info[info_index(sv, h.hit_prim)].chain, org, inv_d, h.best_t, fminf(h.runner_t, h.phantom_t), gap2) != CH_ADMIT) { recast = true; ORT_STAT(2, 4); }
                }
            }
        }
    }
    recast_exactly<COUNTERS>(sv, recast, org, dir, inv_d, lane_id, h, c);
    if (ORT_RARE(stale || recast)) mat = (h.hit_prim != kNoPrim) ? sv.prim_info[info_index(sv, h.hit_prim)].mat : 0u;
    h.hit_mat = (h.hit_prim != kNoPrim) ? mat : 0u;
}

ORT_D void flush_counters(const RenderHot &rv, const Counters &c, bool all) {
    if (all) {
        ORT_COUNT(rv.c->counters + 0, c.paths);
        ORT_COUNT(rv.c->counters + 1, c.rays);
        ORT_COUNT(rv.c->counters + 2, c.nodes);
        ORT_COUNT(rv.c->counters + 3, c.tris);
        ORT_COUNT(rv.c->counters + 4, c.analytic);
    }
}

/* persistent mode: one lane runs jobs until the job space is empty */
/* ADAPT: the adaptive camera render (pt_adaptive): the same loop, a pixel ending where produce_ray's stopping rule says; A is the
   lane's AdaptState, wherever the caller keeps it */
/* GROUPS: the light-group render (pt_groups): the same loop, produce_ray keeping the group sums in the output frames */
/* SPPMAP: the sample-map render (pt_sample_map): the same loop, produce_ray cutting every job at its word of the caller's map; A
   as for ADAPT */
/* ACCUM: the accumulating render (pt_accumulate): SPPMAP's loop, produce_ray starting a pixel from the caller's planes */
/* DEPTHS: the path-depth render (pt_depths): the same loop, produce_ray keeping the bin sums and the length counts in the output
   planes and the ray's depth in a fourth row of lds_focal, which the caller sizes for it */
template <uint32_t F>
ORT_D void pt_lane(const SceneView &sv, const RenderHot &rv, const float4 *tab, uint32_t *lds_stack, float *lds_focal, const int tid,
                   const uint32_t lane_id, bool prof_on = false, unsigned long long *pool = nullptr, AdaptState *A = nullptr) {
    static_assert(flavour_ok(F, LF_OF_LANE), "see flavour_ok");
    constexpr bool COUNTERS = F & LF_COUNTERS, IMPLICIT = F & LF_IMPLICIT;
    uint32_t spill[kSpillStack];
    const uint32_t spp_u = IMPLICIT ? ((rv.mode == JOBS_PIXEL) ? rv.c->spp : rv.c->chunk) : 0u; /* samples per (one-pixel) job */
    Prof pr;
    pr.on = prof_on;
#ifndef ORT_HOST_SIM
    if (COUNTERS && prof_on) pr.t = __builtin_amdgcn_s_memtime();
#endif
    PathState P;
    HitState h;
    Trav T;
    Counters c;
    bool tracing = false;
    for (;;) {
        if (!tracing) {
            ORT_UTIL(sv, 3, true);
            ORT_UTIL(sv, 4, P.ps == PS_HIT);
            ORT_PHASE(pr, sv, 7, true);
            if (P.ps == PS_HIT) resolve_hit<resolve_of(F), kLdsStack, kBlock>(sv, tab, P.org, P.dir, T.inv_d, lane_id, h, c, pr, lds_stack, spill, tid);
            ORT_PHASE(pr, sv, 0, P.ps == PS_HIT);
            tracing = produce_ray<F & ~LF_WIDE>(sv, rv, tab, P, h, c, pr, lds_focal + tid, kBlock, spp_u, nullptr, false, pool, A);
            if (tracing) {
                begin_ray<begin_of(F), kLdsStack, kBlock>(sv, tab, P, T, h, c, pr, lds_stack, spill, tid);
                if (COUNTERS) c.rays++;
            }
        }
        if (ORT_BALLOT(P.ps != PS_DONE) == 0ull) break;
        if (tracing) tracing = traverse<walk_of(F), kLdsStack, kBlock>(sv, P.org, P.dir, T, h, lds_stack, spill, tid, rv.refill_below, rv.descend_below, c, pr, kNoPrim, tab);
    }
    flush_counters(rv, c, COUNTERS);
}


#ifndef ORT_HOST_SIM
/* ---- ray exchange: whole waves shade, whole waves traverse --------------------------------------------------
 * The plain loop (pt_lane) leaves the traversal loop when fewer than refill_below lanes are still tracing; those
 * stragglers then sit idle through the whole shading pass, and the next traversal loop runs for them and the few
 * new rays that need more than the root.  Here the stragglers are PARKED instead: path, hit and traversal state
 * (kStashVecs float4 = 36 dwords) plus the used part of the LDS stack go to the wave's own L stash in HBM, and the lane takes a parked
 * path whose ray is finished (R stash) or a new job, so that the shading pass runs with all 64 lanes.  When enough
 * rays are parked, the wave parks its finished paths in R, fills ALL lanes from L and traverses -- 64 rays of the
 * expensive kind together, topping up from L as they finish.  Path state travels with the ray, seeds belong to
 * jobs, so which lane or in which order a path is advanced cannot change a bit of the result.
 * Both stashes are private to the wave (wave-uniform tops, ballot-prefix slots): no atomics, no barriers. */
struct Stash {
    float4 *rec;    /* [kStashVecs][cap] */
    uint32_t *stk;  /* [kLdsStack][cap], L only */
    uint32_t cap;
};

constexpr uint32_t kStashVecs = 9u; /* float4 per parked path */
/* compile-time constants, so that the nine plane offsets of a parked record are literals instead of scalar registers (which were spilled) */
constexpr uint32_t kCapL = 128u, kCapR = 192u; /* parked paths per wave: unfinished rays / finished rays */
static_assert(kLdsStack % 4 == 0, "the L stash carves its stack words out of float4 units (kLdsStack / 4 per parked path)");
ORT_D void stash_store(const Stash &st, uint32_t slot, const PathState &P, const HitState &h, uint32_t cur, int sp, V3 inv_d, const float *focal_cache,
                       uint32_t info_chain = 0u, uint32_t info_mat = 0u) {
    float4 *r = st.rec + slot;
    const uint32_t cap = st.cap;
    r[0] = make_float4(P.org.x, P.org.y, P.org.z, P.dir.x);
    r[cap] = make_float4(P.dir.y, P.dir.z, h.best_t, om_bits_f32(h.hit_prim));
    r[2u * cap] = make_float4(h.hit_n.x, h.hit_n.y, h.hit_n.z, h.phantom_t);
    r[3u * cap] = make_float4(h.runner_t, om_bits_f32(cur), om_bits_f32((uint32_t)sp), om_bits_f32(P.rng));
    r[4u * cap] = make_float4(P.color.x, P.color.y, P.color.z, P.weight.x);
    r[5u * cap] = make_float4(P.weight.y, P.weight.z, P.wo.x, P.wo.y);
    r[6u * cap] = make_float4(P.wo.z, om_bits_f32(P.pxy), om_bits_f32(P.jyp), om_bits_f32(P.sample | (P.primary ? 0x80000000u : 0u)));
    /* 1/d and the pixel's focal point travel too: recomputing them costs more than two more stores and loads */
    r[7u * cap] = make_float4(inv_d.x, inv_d.y, inv_d.z, focal_cache[0]);
    /* a finished ray's announced winner info (R stash; announce_winner) */
    r[8u * cap] = make_float4(focal_cache[kBlock], focal_cache[2 * kBlock], om_bits_f32(info_chain), om_bits_f32(info_mat));
}

ORT_D void stash_load(const Stash &st, uint32_t slot, const RenderHot &rv, PathState &P, HitState &h, Trav &T, float *focal_cache, uint32_t *lds_info) {
    const float4 *r = st.rec + slot;
    const uint32_t cap = st.cap;
    const float4 a = r[0], b = r[cap], c = r[2u * cap], d = r[3u * cap], e = r[4u * cap], f = r[5u * cap], g = r[6u * cap];
    const float4 i = r[7u * cap], j = r[8u * cap];
    P.org = mk(a.x, a.y, a.z); P.dir = mk(a.w, b.x, b.y);
    h.best_t = b.z; h.hit_prim = om_f32_bits(b.w);
    h.hit_n = mk(c.x, c.y, c.z); h.phantom_t = c.w;
    h.runner_t = d.x; T.cur = om_f32_bits(d.y); T.sp = (int)om_f32_bits(d.z); P.rng = om_f32_bits(d.w);
    P.color = mk(e.x, e.y, e.z); P.weight = mk(e.w, f.x, f.y); P.wo = mk(f.z, f.w, g.x);
    P.pxy = om_f32_bits(g.y); P.jyp = om_f32_bits(g.z);
    const uint32_t sm = om_f32_bits(g.w);
    P.sample = sm & 0x7fffffffu; P.primary = (sm >> 31) != 0u;
    P.ps = PS_HIT;
    T.inv_d = mk(i.x, i.y, i.z);
    focal_cache[0] = i.w; focal_cache[kBlock] = j.x; focal_cache[2 * kBlock] = j.y;
    /* where resolve_hit looks for them (an L path refills its stack over them: it has not finished yet) */
    lds_info[0] = om_f32_bits(j.z); lds_info[kBlock] = om_f32_bits(j.w);
}

template <uint32_t F>
ORT_D void pt_lane_x(const SceneView &sv, const RenderHot &rv, const float4 *tab, uint32_t *lds_stack, float *lds_focal, const int tid,
                     const uint32_t lane_id, bool prof_on, unsigned long long *pool) {
    static_assert(flavour_ok(F, LF_OF_LANE), "see flavour_ok");
    constexpr bool COUNTERS = F & LF_COUNTERS;
    uint32_t spill[kSpillStack];
    Prof pr;
    pr.on = prof_on;
    if (COUNTERS && prof_on) pr.t = __builtin_amdgcn_s_memtime();
    PathState P;
    HitState h;
    Trav T;
    Counters c;
    bool tracing = false;

    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(lane_id >> 6)); /* wave-uniform: the stash addresses stay in scalar registers */
    const uint32_t spp_u = (rv.mode == JOBS_PIXEL) ? rv.c->spp : rv.c->chunk;                /* samples per (one-pixel) job */
    float4 *wbase = rv.c->stash + (size_t)wave * rv.c->stash_wave_f4;
    Stash L, R;
    L.rec = wbase; L.cap = kCapL;
    L.stk = (uint32_t *)(wbase + kStashVecs * kCapL);
    R.rec = wbase + (kStashVecs + (uint32_t)kLdsStack / 4u) * kCapL; R.cap = kCapR; R.stk = nullptr;
    uint32_t ltop = 0, rtop = 0; /* wave-uniform */
    float *focal_cache = lds_focal + tid;
    /* the wave stops parking, and hands its parked paths to free lanes before new jobs, as soon as one of its lanes has
       drawn a job beyond endgame_from: every parked path is a job in progress, and the oldest ones lie at the bottom of the
       LIFO stashes until something drains them -- left to the very end they are a second tail after the job space is empty.
       The lane that draws such a job raises a word of its own in LDS (produce_ray); the wave looks at the 64 words once per
       exchange step.  (Looking at the job counter itself, one lane every 16th step, halved the kernel's speed: 4 096 waves
       reading the one line every job draw of the chip goes through.) */
    uint32_t *late_flag = (uint32_t *)lds_focal + 3 * kBlock + tid;
    *late_flag = 0u;
    bool early_end = false;

    for (;;) {
        if (!early_end) early_end = __ballot(*(volatile uint32_t *)late_flag != 0u) != 0ull;
        /* ---- exchange: every lane is tracing (unfinished ray), done (finished ray, PS_HIT) or free (no path) ---- */
        const unsigned long long m_tr = __ballot(tracing);
        const unsigned long long m_done = __ballot(!tracing && P.ps == PS_HIT);
        const unsigned long long m_free = ~(m_tr | m_done);
        const uint32_t n_tr = (uint32_t)__popcll(m_tr), n_free = (uint32_t)__popcll(m_free);
        /* nothing left but parked rays: traverse them however few */
        const bool drain = m_tr == 0ull && m_done == 0ull && rtop == 0u && __ballot(P.ps != PS_DONE) == 0ull;
        /* once the job space is empty nothing is parked any more (every parked path is a job some lane still has to
           finish): lanes without a path take parked ones, finished rays first, and everything else carries on */
        const bool endgame = early_end || __ballot(P.ps == PS_DONE) != 0ull;
        bool long_phase = !endgame && ltop > 0u && (n_tr + ltop >= rv.c->long_min || drain);
        if (endgame) {
            const bool is_free = !tracing && P.ps != PS_HIT;
            const unsigned long long m_recv = __ballot(is_free);
            const uint32_t rrank = lane_rank(m_recv);
            const bool take_r = is_free && rrank < rtop;
            const bool take_l = is_free && !take_r && rrank - rtop < ltop;
            if (take_r) stash_load(R, rtop - 1u - rrank, rv, P, h, T, focal_cache, lds_stack + tid);
            if (take_l) {
                const uint32_t slot = ltop - 1u - (rrank - rtop);
                stash_load(L, slot, rv, P, h, T, focal_cache, lds_stack + tid);
                for (int lv = 0; lv < T.sp; ++lv) lds_stack[lv * kBlock + tid] = L.stk[(uint32_t)lv * L.cap + slot];
                tracing = true;
            }
            uint32_t n_recv = (uint32_t)__popcll(m_recv);
            const uint32_t from_r = n_recv < rtop ? n_recv : rtop;
            rtop -= from_r;
            n_recv -= from_r;
            ltop -= n_recv < ltop ? n_recv : ltop;
        } else if (long_phase) {
            /* fill the lanes that are not tracing with parked rays; finished paths make room by parking in R */
            uint32_t want = 64u - n_tr;
            if (want > ltop) want = ltop;
            uint32_t need_done = want > n_free ? want - n_free : 0u;
            if (need_done > R.cap - rtop) need_done = R.cap - rtop;
            const bool is_done = !tracing && P.ps == PS_HIT;
            const uint32_t drank = lane_rank(m_done);
            const bool park = is_done && drank < need_done;
            if (park) {
                uint32_t info_chain, info_mat;
                announced_info<kBlock>(lds_stack, tid, info_chain, info_mat);
                stash_store(R, rtop + drank, P, h, 0u, 0, T.inv_d, focal_cache, info_chain, info_mat);
                P.ps = PS_NEED_JOB;
            }
            rtop += need_done < (uint32_t)__popcll(m_done) ? need_done : (uint32_t)__popcll(m_done);
            const bool is_free = !tracing && P.ps != PS_HIT; /* includes the lanes that parked just now */
            const unsigned long long m_recv = __ballot(is_free);
            const uint32_t rrank = lane_rank(m_recv);
            const bool take = is_free && rrank < ltop;
            if (take) {
                const uint32_t slot = ltop - 1u - rrank;
                stash_load(L, slot, rv, P, h, T, focal_cache, lds_stack + tid);
                for (int lv = 0; lv < T.sp; ++lv) lds_stack[lv * kBlock + tid] = L.stk[(uint32_t)lv * L.cap + slot];
                tracing = true;
            }
            const uint32_t n_recv = (uint32_t)__popcll(m_recv);
            ltop -= n_recv < ltop ? n_recv : ltop;
            /* no lane could take a ray (R full, so no finished path could make room) and none is tracing: shade
               instead, which frees lanes */
            if (n_tr == 0u && __ballot(take) == 0ull) long_phase = false;
        } else {
            /* park the stragglers (their stack tail must be in LDS), then hand the free lanes parked finished paths */
            const bool can_park = tracing && T.sp <= kLdsStack && n_tr >= rv.c->park_min;
            const unsigned long long m_park = __ballot(can_park);
            const uint32_t prank = lane_rank(m_park);
            const bool park = can_park && ltop + prank < L.cap;
            if (park) {
                const uint32_t slot = ltop + prank;
                stash_store(L, slot, P, h, T.cur, T.sp, T.inv_d, focal_cache);
                for (int lv = 0; lv < T.sp; ++lv) L.stk[(uint32_t)lv * L.cap + slot] = lds_stack[lv * kBlock + tid];
                tracing = false;
                P.ps = PS_NEED_JOB;
            }
            {
                const uint32_t n_park = (uint32_t)__popcll(m_park), room = L.cap - ltop;
                ltop += n_park < room ? n_park : room;
            }
            const bool is_free = !tracing && P.ps != PS_HIT;
            const unsigned long long m_recv = __ballot(is_free);
            const uint32_t rrank = lane_rank(m_recv);
            const bool take = is_free && rrank < rtop;
            if (take) {
                stash_load(R, rtop - 1u - rrank, rv, P, h, T, focal_cache, lds_stack + tid);
            }
            const uint32_t n_recv = (uint32_t)__popcll(m_recv);
            rtop -= n_recv < rtop ? n_recv : rtop;
        }
        /* ---- shade: only outside a traversal phase, so that it runs with (nearly) all lanes ---- */
        const bool hold = P.ps == PS_NEED_JOB && ltop + rtop >= rv.c->inflight_cap; /* no new job for now */
        if (!long_phase && !tracing && !hold) {
            ORT_UTIL(sv, 3, true);
            ORT_UTIL(sv, 4, P.ps == PS_HIT);
            ORT_PHASE(pr, sv, 7, true);
            if (P.ps == PS_HIT) resolve_hit<resolve_of(F), kLdsStack, kBlock>(sv, tab, P.org, P.dir, T.inv_d, lane_id, h, c, pr, lds_stack, spill, tid);
            ORT_PHASE(pr, sv, 0, P.ps == PS_HIT);
            /* near the end of the launch a lane whose job ends draws no new one while the wave still holds parked paths: the
               next exchange step hands it one of those (endgame branch above), so that the stashes are empty when the job
               space is */
            tracing = produce_ray<F | LF_IMPLICIT>(sv, rv, tab, P, h, c, pr, focal_cache, kBlock, spp_u, late_flag, early_end && ltop + rtop > 0u, pool);
            if (tracing) {
                begin_ray<begin_of(F), kLdsStack, kBlock>(sv, tab, P, T, h, c, pr, lds_stack, spill, tid);
                if (COUNTERS) c.rays++;
            }
        }
        if (__ballot(P.ps != PS_DONE || tracing) == 0ull && ltop == 0u && rtop == 0u) break;
        /* in a traversal phase come back for more parked rays when half the lanes have finished; otherwise (and once
           L is empty) when only stragglers are left, which then park */
        const int below = (long_phase && ltop > 0u) ? (int)rv.c->long_refill : rv.refill_below;
        if (tracing) tracing = traverse<walk_of(F), kLdsStack, kBlock>(sv, P.org, P.dir, T, h, lds_stack, spill, tid, below, rv.descend_below, c, pr, kNoPrim, tab);
    }
    flush_counters(rv, c, COUNTERS);
}
#endif /* !ORT_HOST_SIM */

/* ---- wavefront mode -------------------------------------------------------------------------- */
constexpr uint32_t WF_PRIMARY = 8u, WF_HAS_RAY = 16u;
constexpr int kWfLdsStack = 16; /* trace kernel: 16 LDS entries per lane (16 KB per 256-lane block), tail in scratch */
constexpr int kWfSpill = 48;
static_assert(kWfLdsStack - 4 + kWfSpill >= (int)kTreeDepthBudget, "wavefront trace stack must hold a tree of kTreeDepthBudget levels");

/* one slot: resume its path, produce the next ray, store everything back; returns true if a ray was produced */
template <uint32_t F>
ORT_D bool wf_shade_slot(const SceneView &sv, const RenderHot &rv, const float4 *tab, const WfView &wf, uint32_t i, Counters &c) {
    constexpr bool COUNTERS = F & LF_COUNTERS;
    uint32_t fl = wf.flags[i];
    PathState P;
    P.ps = (int)(fl & 7u);
    if (P.ps == PS_DONE) return false;
    HitState h;
    if (P.ps != PS_NEED_JOB) {
        float4 a = wf.od0[i];
        float2 b = wf.od1[i];
        float4 q0 = wf.p0[i], q1 = wf.p1[i], q2 = wf.p2[i];
        uint4 q3 = wf.p3[i];
        float4 hh = wf.hit0[i];
        P.org = mk(a.x, a.y, a.z); P.dir = mk(a.w, b.x, b.y);
        P.weight = mk(q0.x, q0.y, q0.z); P.color = mk(q0.w, q1.x, q1.y); P.wo = mk(q1.z, q1.w, q2.x);
        P.rng = om_f32_bits(q2.y); P.sample = om_f32_bits(q2.z); P.spp = om_f32_bits(q2.w);
        P.job_index = q3.x; P.pxy = q3.y; P.jxx = q3.z; P.jyp = q3.w;
        P.primary = (fl & WF_PRIMARY) != 0;
        h.best_t = hh.x; h.hit_n = mk(hh.y, hh.z, hh.w); h.hit_prim = wf.hitp[i];
        h.hit_mat = (P.ps == PS_HIT && h.hit_prim != kNoPrim) ? sv.prim_info[info_index(sv, h.hit_prim)].mat : 0u;
    }
    Prof pr;
    bool tracing = produce_ray<F>(sv, rv, tab, P, h, c, pr);
    if (tracing) {
        wf.od0[i] = make_float4(P.org.x, P.org.y, P.org.z, P.dir.x);
        wf.od1[i] = make_float2(P.dir.y, P.dir.z);
        wf.p0[i] = make_float4(P.weight.x, P.weight.y, P.weight.z, P.color.x);
        wf.p1[i] = make_float4(P.color.y, P.color.z, P.wo.x, P.wo.y);
        wf.p2[i] = make_float4(P.wo.z, om_bits_f32(P.rng), om_bits_f32(P.sample), om_bits_f32(P.spp));
        wf.p3[i] = make_uint4(P.job_index, P.pxy, P.jxx, P.jyp);
        if (COUNTERS) c.rays++;
    }
    wf.flags[i] = (uint32_t)P.ps | (P.primary ? WF_PRIMARY : 0u) | (tracing ? WF_HAS_RAY : 0u);
    return tracing;
}

/* one slot: closest hit of its ray, resolved to the reference's answer */
template <uint32_t F>
ORT_D void wf_trace_slot(const SceneView &sv, const float4 *tab, const WfView &wf, uint32_t i, uint32_t lane_id, uint32_t *lds_stack,
                         uint32_t *spill, int tid, Counters &c) {
    if (!(wf.flags[i] & WF_HAS_RAY)) return;
    float4 a = wf.od0[i];
    float2 b = wf.od1[i];
    PathState P;
    P.org = mk(a.x, a.y, a.z); P.dir = mk(a.w, b.x, b.y);
    HitState h;
    Trav T;
    Prof pr;
    begin_ray<F, kWfLdsStack, kBlock>(sv, tab, P, T, h, c, pr, lds_stack, spill, tid);
    traverse<F, kWfLdsStack, kBlock>(sv, P.org, P.dir, T, h, lds_stack, spill, tid, 0, 0, c, pr);
    resolve_hit<F, kWfLdsStack, kBlock>(sv, tab, P.org, P.dir, T.inv_d, lane_id, h, c, pr, lds_stack, spill, tid);
    wf.hit0[i] = make_float4(h.best_t, h.hit_n.x, h.hit_n.y, h.hit_n.z);
    wf.hitp[i] = h.hit_prim;
}

/* pixel = (sum over k of partial[k], in k order) / nchunks for one pixel (CHUNK policy) */
/* view: which frame of the output and which set of partial planes (ort_render_views; 0 otherwise) */
ORT_D void combine_pixel(const RenderHot &rv, unsigned long long idx, uint32_t view = 0) {
    uint32_t blk = rv.c->shard_index + (uint32_t)(idx >> 6) * rv.c->shard_count;
    uint32_t pin = (uint32_t)(idx & 63ull);
    int x = (int)((rv.c->block_x0 + blk % rv.c->blocks_w) * 8u + (pin & 7u));
    int y = (int)((rv.c->block_y0 + blk / rv.c->blocks_w) * 8u + (pin >> 3));
    if (x < rv.c->x0 || x >= rv.c->x1 || y < rv.c->y0 || y >= rv.c->y1) return;
    const size_t plane = (size_t)rv.c->my_blocks * 64u * 3u; /* partial planes are packed: idx is the pixel's place in each */
    V3 acc = mk(0, 0, 0);
    for (uint32_t k = 0; k < rv.c->nchunks; ++k) {
        const float *p = rv.c->partial + ((size_t)view * rv.c->nchunks + k) * plane + 3u * (size_t)idx;
        acc = add(acc, mk(p[0], p[1], p[2]));
    }
    acc = divs(acc, (float)rv.c->nchunks);
    float *o = rv.c->packed_out ? rv.c->out + 3u * (size_t)idx : rv.c->out + 3u * (((size_t)view * (size_t)rv.H + (size_t)y) * (size_t)rv.W + (size_t)x);
    o[0] = acc.x; o[1] = acc.y; o[2] = acc.z;
}

/* one record of the parity tests' per-function evaluation (unit_eval on the device, tools/host_sim --unit on the host):
   op and in[24] -> out[8], op codes and layouts as documented in include/ort.h (ort_unit_eval_device).  Ops 1-13 call
   the reference-shaped functions; ops 14 and up call the specialised forms the render and raycast kernels run instead,
   composed as those kernels compose them, so that each can be held against the generic function's answer. */
ORT_D void unit_eval_op(uint32_t op, const float *a, float *o) {
    for (int k = 0; k < 8; ++k) o[k] = 0.0f;
    auto in3 = [&](int k) { return mk(a[k], a[k + 1], a[k + 2]); };
    V3 n3 = mk(0, 0, 0);
    switch (op) {
    case 1: {
        V3 v0 = in3(0), e1 = sub(in3(3), v0), e2 = sub(in3(6), v0);
        float t = hit_triangle(v0, e1, e2, in3(9), in3(12));
        o[0] = t;
        if (t >= 0.0f) { V3 c = cross(e1, e2); o[1] = c.x; o[2] = c.y; o[3] = c.z; }
    } break;
    case 2: { bool tg; float t = hit_sphere(in3(0), a[3], in3(4), in3(7), n3, tg); o[0] = t; o[1] = n3.x; o[2] = n3.y; o[3] = n3.z; } break;
    case 3: { V3 dd = in3(9); float t = hit_aab(in3(0), in3(3), in3(6), mk(1.0f / dd.x, 1.0f / dd.y, 1.0f / dd.z), n3); o[0] = t; o[1] = n3.x; o[2] = n3.y; o[3] = n3.z; } break;
    case 4: {
        /* host-precomputed frame arrives in a[13..22]: rot rows (9) + |axis| */
        float t = hit_cylinder(in3(0), a[6], in3(13), in3(16), in3(19), a[22], in3(7), in3(10), n3);
        o[0] = t; o[1] = n3.x; o[2] = n3.y; o[3] = n3.z;
    } break;
    case 5: {
        uint32_t seed = om_f32_bits(a[0]);
        Mat m = make_mat(in3(8), in3(11), in3(14), a[17]);
        bool tr;
        V3 wi = sample_brdf(seed, in3(1), in3(4), a[7], m, tr);
        o[0] = wi.x; o[1] = wi.y; o[2] = wi.z; o[3] = tr ? 1.0f : 0.0f; o[4] = om_bits_f32(seed);
    } break;
    case 6: {
        Mat m = make_mat(in3(10), in3(13), in3(16), a[19]);
        o[0] = pdf_brdf(in3(0), in3(3), in3(6), a[9], m);
    } break;
    case 7: {
        Mat m = make_mat(in3(9), in3(12), in3(15), a[18]);
        V3 f = eval_scattering(in3(0), in3(3), in3(6), m, a[19], a[20]);
        o[0] = f.x; o[1] = f.y; o[2] = f.z;
    } break;
    case 8: { V3 r = sample_lobe(in3(0), a[3], a[4]); o[0] = r.x; o[1] = r.y; o[2] = r.z; } break;
    case 9:
        o[0] = ort_sinf(a[0]); o[1] = ort_cosf(a[0]); o[2] = ort_atan2f(a[1], a[0]); o[3] = ort_powf(a[0], a[1]); o[4] = ort_logf(a[0]);
        break;
    case 10: { V3 r = normalize(in3(0)); o[0] = r.x; o[1] = r.y; o[2] = r.z; } break;
    case 11: {
        V3 F = fresnel(in3(0), a[3]);
        o[0] = F.x; o[1] = F.y; o[2] = F.z;
        o[3] = ggx_d(in3(4), in3(7), a[10]);
        o[4] = geom(in3(11), in3(4), in3(7), a[10]);
    } break;
    case 12: { /* RNG: seed -> state after one step, rng_01, rng_between(0, 2pi) from the same seed */
        uint32_t s0 = om_f32_bits(a[0]), s1 = s0, s2 = s0;
        rng_step(s0);
        o[0] = om_bits_f32(s0);
        o[1] = rng_01(s1);
        o[2] = rng_between(s2, 0.0f, 2 * kPi);
        o[3] = om_bits_f32(s2);
        o[4] = om_bits_f32(job_seed(om_f32_bits(a[0]), om_f32_bits(a[1])));
    } break;
    case 13: { /* raw IEEE f32 arithmetic: the bit-exactness premise (div, sqrt, mul, add, sub, u32->f32) */
        o[0] = a[0] / a[1]; o[1] = __builtin_sqrtf(a[0]); o[2] = a[0] * a[1]; o[3] = a[0] + a[1]; o[4] = a[0] - a[1];
        o[5] = (float)om_f32_bits(a[0]); o[6] = a[0] * a[1] + a[2];
    } break;
    case 14: { /* the box forms of the fast paths (op 3's inputs): test_prim<FINITE_RAY> and the analytic prologue; node admission */
        V3 dd = in3(9), inv = mk(1.0f / dd.x, 1.0f / dd.y, 1.0f / dd.z);
        float t = hit_aab_finite(in3(0), in3(3), in3(6), inv, n3);
        o[0] = t; o[1] = n3.x; o[2] = n3.y; o[3] = n3.z;
        o[4] = hit_aab_t_finite(in3(0), in3(3), in3(6), inv);
        o[5] = hit_aab_t(in3(0), in3(3), in3(6), inv);
    } break;
    case 15: { /* pdf_eval_scattering, as produce_ray's all-lobes flavour calls it: f stays 0 unless p > 1e-6 */
        Mat m = make_mat(in3(9), in3(12), in3(15), a[18]);
        V3 f = mk(0, 0, 0);
        o[0] = pdf_eval_scattering(in3(0), in3(3), in3(6), m, a[19], a[20], a[21], f);
        o[1] = f.x; o[2] = f.y; o[3] = f.z;
    } break;
    case 16: { /* the diffuse flavour's pdf and BSDF (op 15's inputs; only for materials the upload guard calls diffuse) */
        Mat m = make_mat(in3(9), in3(12), in3(15), a[18]);
        o[0] = pdf_brdf<true>(in3(0), in3(3), in3(6), a[19], m) * a[21];
        V3 f = eval_scattering<true>(in3(0), in3(3), in3(6), m, a[19], a[20]);
        o[1] = f.x; o[2] = f.y; o[3] = f.z;
    } break;
    case 17: case 18: { /* produce_ray's BSDF sample (op 5's inputs): 17 the all-lobes flavour, 18 the diffuse one */
        uint32_t seed = om_f32_bits(a[0]);
        Mat m = make_mat(in3(8), in3(11), in3(14), a[17]);
        const V3 n = in3(1), wo = in3(4);
        bool tr = false;
        float sn, cs;
        V3 wi;
        if (op == 17) {
            BrdfDraw draw = sample_brdf_draw<false>(seed, a[7], m);
            ort_sincosf(draw.phi, &sn, &cs);
            wi = normalize(sample_brdf_finish<false>(n, normalize(n), wo, m, draw, cs, sn, tr));
        } else {
            BrdfDraw draw = sample_brdf_draw<true>(seed, a[7], m);
            ort_sincosf(draw.phi, &sn, &cs);
            const V3 unit1 = normalize(n);
            wi = normalize(sample_brdf_finish<false, true>(n, unit1, wo, m, draw, cs, sn, tr));
        }
        o[0] = wi.x; o[1] = wi.y; o[2] = wi.z; o[3] = tr ? 1.0f : 0.0f; o[4] = om_bits_f32(seed);
    } break;
    case 19: { float sn, cs; ort_sincosf(a[0], &sn, &cs); o[0] = sn; o[1] = cs; } break;
    case 20: { /* produce_ray's hemisphere draw (HEMI): seed(bits) n.xyz -> d, wo = -normalize(d), the stream after the two draws */
        uint32_t seed = om_f32_bits(a[0]);
        const float e0 = rng_01(seed), e1 = rng_01(seed);
        float sn, cs;
        ort_sincosf(2.0f * kPi * e1, &sn, &cs);
        const V3 d = normalize(sample_lobe_n(normalize(in3(1)), __builtin_sqrtf(e0), cs, sn));
        const V3 wo = neg(normalize(d));
        o[0] = d.x; o[1] = d.y; o[2] = d.z; o[3] = wo.x; o[4] = wo.y; o[5] = wo.z; o[6] = om_bits_f32(seed);
    } break;
    case 21: { /* produce_ray's sphere draw (SH): op 20 with c = 1 - 2 e0 */
        uint32_t seed = om_f32_bits(a[0]);
        const float e0 = rng_01(seed), e1 = rng_01(seed);
        float sn, cs;
        ort_sincosf(2.0f * kPi * e1, &sn, &cs);
        const V3 d = normalize(sample_lobe_n(normalize(in3(1)), 1.0f - 2.0f * e0, cs, sn));
        const V3 wo = neg(normalize(d));
        o[0] = d.x; o[1] = d.y; o[2] = d.z; o[3] = wo.x; o[4] = wo.y; o[5] = wo.z; o[6] = om_bits_f32(seed);
    } break;
    case 22: { /* the SH basis (SH): d.xyz -> b1 ... b8 (b0 is a constant) */
        const ShBasis b = sh_basis(in3(0));
        o[0] = b.b1; o[1] = b.b2; o[2] = b.b3; o[3] = b.b4; o[4] = b.b5; o[5] = b.b6; o[6] = b.b7; o[7] = b.b8;
    } break;
    default: break;
    }
}

#ifndef ORT_HOST_SIM
#ifndef ORT_WAVES_PER_EU
#define ORT_WAVES_PER_EU 4 /* VGPR budget: 4 waves/SIMD = 128 registers, 7 (diffuse flavour) / 26 (general) spilled; tuned on MI355X: profiles/r01_tuning.md */
#endif
/* DIFFUSE: every surface material of the uploaded scene has Ks = Kt = 0, so the evaluation and pdf
   of the specular / transmission lobes are compiled out (sampling keeps all three lobes: a draw of
   exactly 1.0 still takes the reference's transmission branch).  Same values, fewer registers. */
/* the workgroup's copy of the small read-only tables (SceneView::tab_src -> LDS) */
__device__ __forceinline__ void fill_tab(const SceneView &sv, float4 *lds_tab) {
    for (int i = (int)threadIdx.x; i < kTabF4; i += (int)blockDim.x) lds_tab[i] = sv.tab_src[i];
    __syncthreads();
}

/* VIEWS: the kernels of ort_render_views (the plain loop only; SceneView::cam is not read) */
template <bool COUNTERS, bool DIFFUSE, bool TABS, bool IMPLICIT = false, bool WIDE = false, bool VIEWS = false>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_WAVES_PER_EU, ORT_WAVES_PER_EU)))
pt_persistent(SceneView sv, RenderHot rv) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    __shared__ float lds_focal[3 * kBlock]; /* focal[component][lane] */
    __shared__ unsigned long long lds_pool[2 * (kBlock / 64)]; /* per wave: the unissued part of its last batch of job indices (draw_job) */
    __shared__ float4 lds_tab[TABS ? kTabF4 : 1];
    if (TABS) fill_tab(sv, lds_tab);
    const bool prof = COUNTERS && sv.util != nullptr && blockIdx.x < 32u;
    if (prof) {
        if (threadIdx.x < 96) g_lds_prof[threadIdx.x] = 0ull;
        if (threadIdx.x < 4) g_lds_prof[96 + threadIdx.x] = __builtin_amdgcn_s_memtime();
        __syncthreads();
    }
    pt_lane<lf_if(COUNTERS, LF_COUNTERS) | lf_if(DIFFUSE, LF_DIFFUSE) | lf_if(TABS, LF_TABS) | lf_if(IMPLICIT, LF_IMPLICIT) | lf_if(WIDE, LF_WIDE) | lf_if(VIEWS, LF_VIEWS)>(sv, rv, lds_tab, lds_stack, lds_focal, (int)threadIdx.x, blockIdx.x * (uint32_t)kBlock + threadIdx.x, prof,
                                                    wave_job_pool(rv, lds_pool));
    if ((threadIdx.x & 63u) == 0u && rv.c->drain) rv.c->drain[blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)] = __builtin_amdgcn_s_memrealtime();
    if (prof) {
        __syncthreads();
        if (threadIdx.x < 96 && g_lds_prof[threadIdx.x]) atomicAdd(sv.util + threadIdx.x, g_lds_prof[threadIdx.x]);
    }
}

/* The adaptive camera render (ort_render_adaptive, ort_render_views_adaptive): the plain loop over the implicit one-pixel jobs of a
   batch of views (JOBS_PIXEL; the single frame is the one-view batch of the scene's own camera), every pixel cut by the stopping
   rule.  Built in ort_kernels_render_adaptive.hip alone.  The lane's AdaptState (Q and the next check's sample count) lives in LDS
   beside the focal cache, not in registers: it is touched once per SAMPLE -- hundreds of node tests -- while two more registers
   would be live through the whole traversal loop of a kernel that sits at its 128-register cap and spills already; 2 KB of LDS
   per workgroup leaves the four workgroups per CU their room.  No probes, no drain times */
template <bool COUNTERS, bool DIFFUSE, bool TABS>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_WAVES_PER_EU, ORT_WAVES_PER_EU)))
pt_adaptive(SceneView sv, RenderHot rv) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    __shared__ float lds_focal[3 * kBlock]; /* focal[component][lane] */
    __shared__ unsigned long long lds_pool[2 * (kBlock / 64)]; /* as pt_persistent */
    __shared__ float4 lds_tab[TABS ? kTabF4 : 1];
#ifdef ORT_ADAPT_IN_REGISTERS /* A/B builds: the resource figures of the other choice (profiles/r12_render_adaptive.md) */
    AdaptState adapt, *const A = &adapt;
#else
    static_assert(sizeof(AdaptState) == sizeof(uint2), "a lane's AdaptState is two words of LDS");
    __shared__ uint2 lds_adapt[kBlock]; /* raw words: produce_ray sets both at every pixel's start, before it reads them */
    AdaptState *const A = reinterpret_cast<AdaptState *>(lds_adapt) + threadIdx.x;
#endif
    if (TABS) fill_tab(sv, lds_tab);
    pt_lane<lf_if(COUNTERS, LF_COUNTERS) | lf_if(DIFFUSE, LF_DIFFUSE) | lf_if(TABS, LF_TABS) | LF_IMPLICIT | LF_VIEWS | LF_ADAPT>(sv, rv, lds_tab, lds_stack, lds_focal, (int)threadIdx.x, blockIdx.x * (uint32_t)kBlock + threadIdx.x, false,
                                                              wave_job_pool(rv, lds_pool), A);
}

/* The light-group render (ort_render_light_groups, ort_render_views_light_groups): the plain loop over the implicit one-pixel jobs
   of a batch of views (JOBS_PIXEL; the single frame is the one-view batch of the scene's own camera), every emission added to its
   light's group as well (produce_ray's GROUPS flag).  Built beside pt_adaptive, in ort_kernels_render_adaptive.hip alone.  The
   group sums live in the output frames, so the kernel holds what pt_persistent holds and nothing more.  No probes, no drain times */
template <bool COUNTERS, bool DIFFUSE, bool TABS>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_WAVES_PER_EU, ORT_WAVES_PER_EU)))
pt_groups(SceneView sv, RenderHot rv) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    __shared__ float lds_focal[3 * kBlock]; /* focal[component][lane] */
    __shared__ unsigned long long lds_pool[2 * (kBlock / 64)]; /* as pt_persistent */
    __shared__ float4 lds_tab[TABS ? kTabF4 : 1];
    if (TABS) fill_tab(sv, lds_tab);
    pt_lane<lf_if(COUNTERS, LF_COUNTERS) | lf_if(DIFFUSE, LF_DIFFUSE) | lf_if(TABS, LF_TABS) | LF_IMPLICIT | LF_VIEWS | LF_GROUPS>(sv, rv, lds_tab, lds_stack, lds_focal, (int)threadIdx.x, blockIdx.x * (uint32_t)kBlock + threadIdx.x, false,
                                                                     wave_job_pool(rv, lds_pool));
}

/* The path-depth render (ort_render_depths, ort_render_views_depths): pt_groups' loop with the emission's bin chosen by the depth of
   the ray it arrived on (produce_ray's DEPTHS flag) instead of by the light that was hit, and a count of the samples by the depth
   of their last ray.  Built beside pt_groups, in ort_kernels_render_adaptive.hip alone.  The sums and the counts live in the
   output planes; the depth of the ray in flight is the fourth row of lds_focal, one more word of LDS per lane (1 KB per
   workgroup).  No probes, no drain times */
template <bool COUNTERS, bool DIFFUSE, bool TABS>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_WAVES_PER_EU, ORT_WAVES_PER_EU)))
pt_depths(SceneView sv, RenderHot rv) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    __shared__ float lds_focal[4 * kBlock]; /* rows 0-2 focal[component][lane], row 3 the depth of the lane's ray in flight (u32) */
    __shared__ unsigned long long lds_pool[2 * (kBlock / 64)]; /* as pt_persistent */
    __shared__ float4 lds_tab[TABS ? kTabF4 : 1];
    if (TABS) fill_tab(sv, lds_tab);
    pt_lane<lf_if(COUNTERS, LF_COUNTERS) | lf_if(DIFFUSE, LF_DIFFUSE) | lf_if(TABS, LF_TABS) | LF_IMPLICIT | LF_VIEWS | LF_DEPTHS>(sv, rv, lds_tab, lds_stack, lds_focal, (int)threadIdx.x, blockIdx.x * (uint32_t)kBlock + threadIdx.x, false,
                                                                     wave_job_pool(rv, lds_pool));
}

/* The sample-map render (ort_render_sample_map, ort_render_views_sample_map): the plain loop over the implicit one-pixel jobs of a
   batch of views (JOBS_PIXEL; the single frame is the one-view batch of the scene's own camera), every job as long as the caller's
   map says (produce_ray's SPPMAP flag).  Built beside pt_adaptive, in ort_kernels_render_adaptive.hip alone.  The job's length and
   its sum of squared sample luminance are the two LDS words per lane that pt_adaptive keeps its AdaptState in, for that
   kernel's reason: touched once per sample, not worth two registers through the traversal loop.  No probes, no drain times */
template <bool COUNTERS, bool DIFFUSE, bool TABS>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_WAVES_PER_EU, ORT_WAVES_PER_EU)))
pt_sample_map(SceneView sv, RenderHot rv) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    __shared__ float lds_focal[3 * kBlock]; /* focal[component][lane] */
    __shared__ unsigned long long lds_pool[2 * (kBlock / 64)]; /* as pt_persistent */
    __shared__ float4 lds_tab[TABS ? kTabF4 : 1];
    static_assert(sizeof(AdaptState) == sizeof(uint2), "a lane's AdaptState is two words of LDS");
    __shared__ uint2 lds_adapt[kBlock]; /* raw words: produce_ray sets n where it draws a job and Q at the pixel's start; before a lane's first job n is read and not used */
    AdaptState *const A = reinterpret_cast<AdaptState *>(lds_adapt) + threadIdx.x;
    if (TABS) fill_tab(sv, lds_tab);
    pt_lane<lf_if(COUNTERS, LF_COUNTERS) | lf_if(DIFFUSE, LF_DIFFUSE) | lf_if(TABS, LF_TABS) | LF_IMPLICIT | LF_VIEWS | LF_SPPMAP>(sv, rv, lds_tab, lds_stack, lds_focal, (int)threadIdx.x, blockIdx.x * (uint32_t)kBlock + threadIdx.x, false,
                                                                     wave_job_pool(rv, lds_pool), A);
}

/* The accumulating render (ort_render_accumulate, ort_render_views_accumulate): pt_sample_map's loop and its LDS, word for word,
   with produce_ray's ACCUM flag on top of SPPMAP: a job starts from the pixel's words of the caller's planes and ends by storing
   them.  The map may be null.  Built beside pt_sample_map, in ort_kernels_render_adaptive.hip alone */
template <bool COUNTERS, bool DIFFUSE, bool TABS>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_WAVES_PER_EU, ORT_WAVES_PER_EU)))
pt_accumulate(SceneView sv, RenderHot rv) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    __shared__ float lds_focal[3 * kBlock]; /* focal[component][lane] */
    __shared__ unsigned long long lds_pool[2 * (kBlock / 64)]; /* as pt_persistent */
    __shared__ float4 lds_tab[TABS ? kTabF4 : 1];
    static_assert(sizeof(AdaptState) == sizeof(uint2), "a lane's AdaptState is two words of LDS");
    __shared__ uint2 lds_adapt[kBlock]; /* as pt_sample_map: add where a job is drawn, Q at the pixel's start */
    AdaptState *const A = reinterpret_cast<AdaptState *>(lds_adapt) + threadIdx.x;
    if (TABS) fill_tab(sv, lds_tab);
    pt_lane<lf_if(COUNTERS, LF_COUNTERS) | lf_if(DIFFUSE, LF_DIFFUSE) | lf_if(TABS, LF_TABS) | LF_IMPLICIT | LF_VIEWS | LF_SPPMAP | LF_ACCUM>(sv, rv, lds_tab, lds_stack, lds_focal, (int)threadIdx.x, blockIdx.x * (uint32_t)kBlock + threadIdx.x, false,
                                                                     wave_job_pool(rv, lds_pool), A);
}

/* the same with the ray exchange (pt_lane_x): implicit job spaces only, LDS tables required */
template <bool COUNTERS, bool DIFFUSE>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_WAVES_PER_EU, ORT_WAVES_PER_EU)))
pt_persistent_x(SceneView sv, RenderHot rv) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    __shared__ float lds_focal[4 * kBlock]; /* rows 0-2 focal point, row 3 "this lane drew a job near the end of the launch" (u32) */
    __shared__ unsigned long long lds_pool[2 * (kBlock / 64)]; /* per wave: the unissued part of its last batch of job indices (draw_job) */
    __shared__ float4 lds_tab[kTabF4];
    fill_tab(sv, lds_tab);
    const bool prof = COUNTERS && sv.util != nullptr && blockIdx.x < 32u;
    if (prof) {
        if (threadIdx.x < 96) g_lds_prof[threadIdx.x] = 0ull;
        if (threadIdx.x < 4) g_lds_prof[96 + threadIdx.x] = __builtin_amdgcn_s_memtime();
        __syncthreads();
    }
    pt_lane_x<lf_if(COUNTERS, LF_COUNTERS) | lf_if(DIFFUSE, LF_DIFFUSE) | LF_TABS>(sv, rv, lds_tab, lds_stack, lds_focal, (int)threadIdx.x, blockIdx.x * (uint32_t)kBlock + threadIdx.x, prof,
                                       wave_job_pool(rv, lds_pool));
    if ((threadIdx.x & 63u) == 0u && rv.c->drain) rv.c->drain[blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)] = __builtin_amdgcn_s_memrealtime();
    if (prof) {
        __syncthreads();
        if (threadIdx.x < 96 && g_lds_prof[threadIdx.x]) atomicAdd(sv.util + threadIdx.x, g_lds_prof[threadIdx.x]);
    }
}

#ifdef ORT_LIBRARY_KERNELS /* the kernels that are no templates would be compiled by every unit that includes this: ort_kernels.hip alone asks for them */
/* wavefront kernels: fixed-size grids, grid-stride over the slots */
template <bool COUNTERS>
__global__ void __launch_bounds__(kBlock) wf_shade(SceneView sv, RenderHot rv, WfView wf, int count_active) {
    const float4 *lds_tab = nullptr; /* the wavefront kernels read the tables from HBM */
    Counters c;
    unsigned long long produced = 0;
    const uint32_t stride = gridDim.x * (uint32_t)kBlock;
    for (uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x; i < wf.slots; i += stride)
        if (wf_shade_slot<lf_if(COUNTERS, LF_COUNTERS)>(sv, rv, lds_tab, wf, i, c)) produced++;
    if (count_active && produced) atomicAdd(wf.active, produced);
    flush_counters(rv, c, COUNTERS);
}

template <bool COUNTERS>
__global__ void __launch_bounds__(kBlock) wf_trace(SceneView sv, RenderHot rv, WfView wf) {
    __shared__ uint32_t lds_stack[kWfLdsStack * kBlock];
    const float4 *lds_tab = nullptr;
    uint32_t spill[kWfSpill];
    Counters c;
    const uint32_t stride = gridDim.x * (uint32_t)kBlock;
    const uint32_t lane_id = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    for (uint32_t i = lane_id; i < wf.slots; i += stride)
        wf_trace_slot<lf_if(COUNTERS, LF_COUNTERS)>(sv, lds_tab, wf, i, lane_id, lds_stack, spill, (int)threadIdx.x, c);
    flush_counters(rv, c, COUNTERS);
}

__global__ void wf_init(WfView wf) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < wf.slots) wf.flags[i] = (uint32_t)PS_NEED_JOB;
    if (i == 0) *wf.active = 0ull;
}

/* per-function evaluation on the device, for the parity tests: records of {u32 op; f32 in[24]}
   -> f32 out[8], op codes as documented in include/ort.h (ort_unit_eval_device) */
__global__ void unit_eval(const uint32_t *records, uint32_t n, float *out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *rec = records + 25u * i;
    float a[24];
    for (int k = 0; k < 24; ++k) a[k] = om_bits_f32(rec[1 + k]);
    float o[8];
    unit_eval_op(rec[0], a, o);
    for (int k = 0; k < 8; ++k) out[8u * i + k] = o[k];
}

__global__ void combine_chunks(RenderHot rv) {
    unsigned long long idx = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (unsigned long long)rv.c->my_blocks * 64ull) return;
    combine_pixel(rv, idx);
}
/* the same over the frames of a batch of views: [view][this view's pixels] */
__global__ void combine_chunks_views(RenderHot rv) {
    const unsigned long long idx = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x, per_view = (unsigned long long)rv.c->my_blocks * 64ull;
    if (idx >= per_view * rv.c->view_count) return;
    combine_pixel(rv, idx % per_view, (uint32_t)(idx / per_view));
}

#endif /* ORT_LIBRARY_KERNELS */
#endif /* !ORT_HOST_SIM */

/* ---- closest-hit ray queries (ort_raycast): raycast_top_most_node, ray.cpp:1165-1176 --------------------------------
 * The path-trace loop without shading: a lane without a ray takes the next ray index from its wave's batch (draw_job:
 * the job space is the ray array, job_count rays), starts it (begin_ray: analytic prologue from the LDS tables),
 * traverses with refill_below -- so the finished lanes of a wave fetch new rays while the rest are still in the tree --
 * and, once the ray is finished, resolves its hit to the reference's answer (resolve_hit: chains, ties, phantoms, the
 * exact fallback) and writes the record, the normal normalised as raycast_bvh returns it.  A wave's ray indices are contiguous, so its 24-byte loads and stores
 * coalesce; both are done as three 8-byte accesses (the host checks the alignment). */
ORT_D bool raycast_needs_exact(const RaycastIO &io, V3 org, V3 dir, V3 inv_d) {
    const bool short_dir = io.tree_quadrics && !(len2(dir) >= (io.tree_spheres ? 0.999f : 1e-30f));
    const bool inv_nonfinite = io.tree_boxes && !(((inv_d.x - inv_d.x) + (inv_d.y - inv_d.y)) + (inv_d.z - inv_d.z) == 0.0f);
    const bool far = io.tree_quadrics && !(org.x >= io.lo[0] && org.x <= io.hi[0] && org.y >= io.lo[1] && org.y <= io.hi[1] &&
                                          org.z >= io.lo[2] && org.z <= io.hi[2]);
    return short_dir || far || inv_nonfinite;
}
/* no fast traversal for a ray that has just been started: resolve_hit re-casts it exactly (a phantom that could win) */
ORT_D void skip_fast_walk(Trav &T, HitState &h) {
    T.cur = kTraversalDone;
    h.phantom_t = 0.0f;
}
ORT_D float ray_bound(float tm) { return (tm > 0.0f) ? fminf(tm, 3.402823466e+38f) : 0.0f; } /* THE BOUND (at occluded_lane, which keeps a twin of this line); 0 for NaN or <= 0 */
/* three of a lane's LDS words (job_cache: word k at job_cache[k * kBlock]) as a V3: read, and accumulated by separately rounded adds */
ORT_D V3 cache_v3(const float *w) { return mk(w[0], w[kBlock], w[2 * kBlock]); }
ORT_D void cache_add_v3(float *w, V3 v) { w[0] = w[0] + v.x; w[kBlock] = w[kBlock] + v.y; w[2 * kBlock] = w[2 * kBlock] + v.z; }

template <uint32_t F>
ORT_D void raycast_lane(const SceneView &sv, const RenderHot &rv, const RaycastIO &io, const float4 *tab, uint32_t *lds_stack, const int tid,
                        const uint32_t lane_id, unsigned long long *pool) {
    static_assert(flavour_ok(F, LF_OF_LANE), "see flavour_ok");
    constexpr bool COUNTERS = F & LF_COUNTERS;
    uint32_t spill[kSpillStack];
    PathState P;
    HitState h;
    Trav T;
    Counters c;
    Prof pr;
    unsigned long long ray = 0;
    bool tracing = false, held = false, more = true; /* held: this lane's ray is finished but its hit is not written yet */
    for (;;) {
        if (!tracing) {
            if (held) {
                resolve_hit<resolve_of(F), kLdsStack, kBlock>(sv, tab, P.org, P.dir, T.inv_d, lane_id, h, c, pr, lds_stack, spill, tid);
                const uint32_t src = h.hit_prim != kNoPrim ? io.prim_src[info_index(sv, h.hit_prim)] : kNoPrim;
                const V3 n = normalize(h.hit_n); /* ray.cpp:817: the normal leaves raycast_bvh normalised (a miss's stays 0) */
                uint2 *o = io.hits + 3ull * ray;
                o[0] = make_uint2(om_f32_bits(h.best_t), om_f32_bits(n.x));
                o[1] = make_uint2(om_f32_bits(n.y), om_f32_bits(n.z));
                o[2] = make_uint2(h.hit_mat, src);
                held = false;
            }
            if (more) {
                const unsigned long long j = draw_job(rv, pool);
                if (j < rv.c->job_count) {
                    const Ray6 r = load_ray(io.rays, j);
                    P.org = r.o;
                    P.dir = r.d;
                    ray = j;
                    begin_ray<begin_of(F), kLdsStack, kBlock>(sv, tab, P, T, h, c, pr, lds_stack, spill, tid);
                    if (ORT_RARE(raycast_needs_exact(io, P.org, P.dir, T.inv_d))) skip_fast_walk(T, h);
                    if (COUNTERS) c.rays++;
                    tracing = held = true;
                } else {
                    more = false;
                }
            }
        }
        /* a lane that is not tracing now has no ray and will get none */
        if (ORT_BALLOT(tracing) == 0ull) break;
        if (tracing) tracing = traverse<walk_of(F), kLdsStack, kBlock>(sv, P.org, P.dir, T, h, lds_stack, spill, tid, rv.refill_below, rv.descend_below, c, pr, kNoPrim, tab);
    }
    flush_counters(rv, c, COUNTERS);
}

/* TABS: the prologue shapes fit their LDS slot (TAB_PRO: at most kTabProCap float4, ort_plan.h table_fit_flags); otherwise they
   are read from HBM */
#ifndef ORT_HOST_SIM
template <bool COUNTERS, bool TABS>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_WAVES_PER_EU, ORT_WAVES_PER_EU)))
raycast_rays(SceneView sv, RenderHot rv, RaycastIO io) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    __shared__ unsigned long long lds_pool[2 * (kBlock / 64)]; /* per wave: the unissued part of its last batch of ray indices (draw_job) */
    __shared__ float4 lds_tab[TABS ? kTabF4 : 1];
    if (TABS) fill_tab(sv, lds_tab);
    raycast_lane<lf_if(COUNTERS, LF_COUNTERS) | lf_if(TABS, LF_TABS)>(sv, rv, io, lds_tab, lds_stack, (int)threadIdx.x, blockIdx.x * (uint32_t)kBlock + threadIdx.x, wave_job_pool(rv, lds_pool));
}
#endif

/* ---- occlusion ray queries (ort_occluded): is anything in the way before tmax? ---------------------------------------
 * occluded = (h.mat != 0 && h.t < tmax), h the closest hit raycast_rays returns.  The loop of raycast_lane with three
 * differences.
 * THE BOUND.  A ray starts with best_t = B = min(tmax, FLT_MAX) instead of FLT_MAX, so the prologue and the tree walk accept
 * and descend only below B, from the first node on.  What that traversal knows afterwards:
 *   - no winner: no shape is hit below B.  The reference's answer is some shape's distance or a phantom's, so it is >= B unless
 *     a phantom lies at or below B (phantoms are never culled by distance: phantom_t is complete) -- resolve_hit's own
 *     "phantom_t <= best_t" test, with best_t still B, sends exactly those to the exact walk.  Otherwise the answer is 0.
 *   - a winner W: it is the nearest of ALL shapes (every other one is at or beyond B > t_W), which is chain_verdict's premise.
 *     Its other premise -- t_other is the nearest other hit, exact inside the 2e-4 window above t_W -- no longer holds as it
 *     stands: the walk has not seen runners-up at or beyond B.  Everything it has not seen is at or beyond B, so
 *     min(runner_t, B) bounds the nearest other hit from below, and a smaller t_other only turns CH_ADMIT into CH_UNKNOWN.
 *     The bound is therefore handed to resolve_hit as a runner-up; the re-traversals of resolve_hit start afresh (bounded by
 *     the leaf box's entry, or unbounded) and owe nothing to B.  After resolve_hit, h is the reference's closest hit whenever
 *     that lies below B, and the byte is the contract's comparison.
 * tmax <= 0 or NaN: 0 without a traversal (a hit has t >= 1e-6).  B is 0 for them, which matters only to the forced walk below.
 * EARLY END.  The reference's best distance only ever decreases, and it tests every record of every node it visits.  So
 * if a candidate C with t_C < tmax is in a node the reference is certain to visit, its answer is at most t_C: occluded,
 * whatever else the scene holds -- provided no shape carries material 0 (mats_nonzero), since the contract also asks
 * mat != 0 of the final winner.  "Certain to visit" is decidable without knowing the nearest hit (chain_verdict's other
 * clauses are not: they compare entry distances with the best at that moment): C lies in the root (chain length 0), or
 * the ray's origin is inside every box of C's chain -- inside the smallest of them when the chain is nested
 * (kChainNested) -- because a child that contains the origin is admitted unconditionally (ray.cpp:788-803).  The test is made
 * once, on the prologue's winner, where the wave is converged; a candidate met inside the tree is not tested (a chain
 * fetch per leaf hit costs more than the rest of the bounded walk) and goes through resolve_hit like every other ray.
 * EXACT WALK.  The rays raycast_needs_exact names, and those ORT_DEBUG_FORCE_FALLBACK selects, skip the fast traversal
 * and the early end; resolve_hit re-casts them exactly and their closest hit is compared with tmax.
 * One byte out per ray, a plain byte store: a wave's ray indices are contiguous, 64 adjacent bytes. */
template <uint32_t F>
ORT_D void occluded_lane(const SceneView &sv, const RenderHot &rv, const OccludedIO &io, const float4 *tab, uint32_t *lds_stack, const int tid,
                         const uint32_t lane_id, unsigned long long *pool) {
    static_assert(flavour_ok(F, LF_OF_LANE), "see flavour_ok");
    constexpr bool COUNTERS = F & LF_COUNTERS;
    uint32_t spill[kSpillStack];
    PathState P;
    HitState h;
    Trav T;
    Counters c;
    Prof pr;
    unsigned long long ray = 0;
    float bound = 0.0f;
    bool tracing = false, held = false, more = true; /* held: this lane's ray is finished but its byte is not written yet */
    for (;;) {
        if (!tracing) {
            if (held) {
                h.runner_t = fminf(h.runner_t, bound); /* the bound is a runner-up the walk may not have seen */
                resolve_hit<resolve_of(F), kLdsStack, kBlock>(sv, tab, P.org, P.dir, T.inv_d, lane_id, h, c, pr, lds_stack, spill, tid);
                io.out[ray] = (h.hit_mat != 0u && h.best_t < bound) ? (uint8_t)1 : (uint8_t)0;
                held = false;
            }
            if (more) {
                const unsigned long long j = draw_job(rv, pool);
                if (j < rv.c->job_count) {
                    const Ray6 r = load_ray(io.q.rays, j);
                    const float tm = io.tmax ? io.tmax[j] : __builtin_inff();
                    P.org = r.o;
                    P.dir = r.d;
                    ray = j;
                    if (COUNTERS) c.rays++;
                    /* forced_fallback's and ray_bound's twins, kept in this form: through either helper occluded_rays' code moves */
                    const bool forced = sv.force_fallback_mask != 0xffffffffu && (om_f32_bits(P.dir.x) & sv.force_fallback_mask) == 0u;
                    bound = (tm > 0.0f) ? fminf(tm, 3.402823466e+38f) : 0.0f;
                    if (!(tm > 0.0f) && !forced) {
                        io.out[j] = (uint8_t)0; /* nothing is hit below 1e-6 */
                    } else {
                        T.cur = 0;
                        T.sp = 0;
                        T.inv_d = mk(1.0f / P.dir.x, 1.0f / P.dir.y, 1.0f / P.dir.z); /* as begin_ray, with the bound for Flt_Max */
                        reset_hit(h, bound);
                        prologue_tests<begin_of(F)>(sv, tab, P.org, P.dir, T.inv_d, h, c);
                        bool seen = false; /* the prologue's winner is one the reference is certain to test */
                        if (ORT_RARE(forced || raycast_needs_exact(io.q, P.org, P.dir, T.inv_d))) {
                            skip_fast_walk(T, h);
                        } else if (io.mats_nonzero && h.hit_prim != kNoPrim) {
                            const uint32_t word = sv.prim_info[info_index(sv, h.hit_prim)].chain;
                            const uint32_t first = word & 0x07ffffffu;
                            seen = (word >> 28) == 0u;
                            if (!seen && (word & kChainNested)) seen = in_rect_half_open(sv.chain_boxes[2u * first], sv.chain_boxes[2u * first + 1u], P.org);
                        }
                        if (seen) io.out[j] = (uint8_t)1;
                        else tracing = held = true;
                    }
                } else {
                    more = false;
                }
            }
        }
        /* a lane that is neither tracing nor entitled to another draw has no ray and will get none */
        if (ORT_BALLOT(tracing || more) == 0ull) break;
        if (tracing) tracing = traverse<walk_of(F), kLdsStack, kBlock>(sv, P.org, P.dir, T, h, lds_stack, spill, tid, rv.refill_below, rv.descend_below, c, pr, kNoPrim, tab);
    }
    flush_counters(rv, c, COUNTERS);
}

#ifndef ORT_HOST_SIM
template <bool COUNTERS, bool TABS>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_WAVES_PER_EU, ORT_WAVES_PER_EU)))
occluded_rays(SceneView sv, RenderHot rv, OccludedIO io) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    __shared__ unsigned long long lds_pool[2 * (kBlock / 64)]; /* as raycast_rays */
    __shared__ float4 lds_tab[TABS ? kTabF4 : 1];
    if (TABS) fill_tab(sv, lds_tab);
    occluded_lane<lf_if(COUNTERS, LF_COUNTERS) | lf_if(TABS, LF_TABS)>(sv, rv, io, lds_tab, lds_stack, (int)threadIdx.x, blockIdx.x * (uint32_t)kBlock + threadIdx.x, wave_job_pool(rv, lds_pool));
}
#endif

/* ---- ambient-occlusion queries (ort_ambient_occlusion): hemisphere visibility gathers at points --------------------------
 * A job is a point (p, n) with a seed and a radius; its spp samples run on one xorshift stream.  A sample is unit op 20's
 * direction draw about n (two rng_01, sqrt, the deterministic sin/cos, sample_lobe_n about normalize(n), normalize) and then
 * occluded_lane's ray (p, d) at tmax = radius: the bound, the prologue, raycast_needs_exact on (p, d), the early end on the
 * prologue's winner, the bounded walk, resolve_hit with the bound for a runner-up and the same comparison.  The lane keeps
 * the point, normalize(n), the stream, the sample count, the open count, the bent sum and the bound across samples, and
 * writes 4 to 20 bytes per point at the job's end.  A point outside the domain (produce_ray's RAYS test, on n for d) is
 * answered where it is drawn: ORT_AO_INVALID, NaN, its seed as given.
 * WHERE A SAMPLE STARTS.  occluded_lane fetches a ray wherever a lane is idle; here that place holds the binary64 sin/cos.  So
 * the idle lanes first settle what needs no arithmetic -- the finished sample's verdict, the job's end, the next point (a
 * loop: an invalid point takes another) -- and then meet at ONE draw, produce_ray's structure: one converged ort_sincosf per
 * pass of the outer loop for every lane that starts a sample, whether the point's first or a later one.
 * A radius that is NaN or <= 0 (bound 0) traverses nothing -- nothing is hit below 1e-6 -- but still draws, counts a ray and
 * adds d to the bent sum.  The stream advances exactly two steps per sample, whatever is hit.
 * WHERE THE JOB'S STATE LIVES.  With all of it in registers the kernels spill 8 to 34 VGPRs where occluded_rays spills none
 * (profiles/r14_ao.md).  What is touched once per sample and never inside the walk -- the bent sum and normalize(n) -- sits in
 * six per-lane LDS words instead (job_cache: word k of a lane at job_cache[k * kBlock], conflict-free), as pt_adaptive keeps its
 * AdaptState: 6 KB per block, which leaves four blocks per CU.
 * WHAT THE RADIUS SAVES PER POINT.  The bound is the job's, not the ray's, and every direction has unit length: when p lies
 * farther than the bound from both child boxes of the fast tree's root, no sample of the point can hit anything of the tree
 * below the bound, and none visits it (T.cur = kTraversalDone after the prologue; resolve_hit sees a walk that found nothing,
 * with the bound for a runner-up as ever).  One distance test of the root's record per point -- counted as its two box tests --
 * instead of a root visit per sample.  Not with spheres in the tree: a sphere's tangent branch reports hits outside its box and
 * nearer than the box's entry (ort_scene.h), so there every sample walks.  The distance is compared with 0.2 % to spare, far
 * more than the rounding of |d_k| and of a hit's distance. */
ORT_D bool ao_box_within(float4 lo_xyz_hi_x, float hi_y, float hi_z, V3 p, float bound) {
    const float dx = fmaxf(fmaxf(lo_xyz_hi_x.x - p.x, p.x - lo_xyz_hi_x.w), 0.0f);
    const float dy = fmaxf(fmaxf(lo_xyz_hi_x.y - p.y, p.y - hi_y), 0.0f);
    const float dz = fmaxf(fmaxf(lo_xyz_hi_x.z - p.z, p.z - hi_z), 0.0f);
    return !(((dx * dx + dy * dy) + dz * dz) * 0.998f > bound * bound); /* NaN or overflow: within */
}
constexpr int kAoCacheWords = 6; /* bent.xyz, normalize(n).xyz */

template <uint32_t F>
ORT_D void ao_lane(const SceneView &sv, const RenderHot &rv, const AoIO &io, const float4 *tab, uint32_t *lds_stack, float *job_cache, const int tid,
                   const uint32_t lane_id, unsigned long long *pool) {
    static_assert(flavour_ok(F, LF_OF_LANE), "see flavour_ok");
    constexpr bool COUNTERS = F & LF_COUNTERS, TABS = F & LF_TABS;
    uint32_t spill[kSpillStack];
    HitState h;
    Trav T;
    Counters c;
    Prof pr;
    unsigned long long point = 0;
    V3 org = mk(0, 0, 0), dir = mk(0, 0, 0);
    float *const bent = job_cache, *const unit_n = job_cache + 3 * kBlock; /* per-lane words, stride kBlock */
    uint32_t rng = 1u, sample = 0, open = 0; /* sample: the samples of this point started so far */
    float bound = 0.0f;
    bool tracing = false, held = false, busy = false, more = true; /* held: as occluded_lane's; busy: this lane owns a point */
    bool reach = true; /* something of the fast tree may lie within the bound of this point */
    for (;;) {
        if (!tracing) {
            if (held) { /* the finished sample's verdict */
                h.runner_t = fminf(h.runner_t, bound); /* the bound is a runner-up the walk may not have seen */
                resolve_hit<resolve_of(F), kLdsStack, kBlock>(sv, tab, org, dir, T.inv_d, lane_id, h, c, pr, lds_stack, spill, tid);
                if (!(h.hit_mat != 0u && h.best_t < bound)) { open++; cache_add_v3(bent, dir); }
                held = false;
            }
            bool start = false;
            for (;;) { /* the job's end and the next point */
                if (busy) {
                    if (sample < io.spp) { start = true; break; }
                    io.open[point] = open;
                    if (io.bent) { float *b = io.bent + 3ull * point; const V3 s = cache_v3(bent); b[0] = s.x; b[1] = s.y; b[2] = s.z; }
                    if (io.states) io.states[point] = rng;
                    busy = false;
                }
                if (!more) break;
                const unsigned long long j = draw_job(rv, pool);
                if (!(j < rv.c->job_count)) { more = false; break; }
                const float2 *r = io.q.rays + 3ull * j; /* load_ray's twin, kept in this form: through the helper ao_points' code moves */
                const float2 a = r[0], b = r[1], e = r[2];
                const uint32_t seed = io.seeds[j];
                const V3 p = mk(a.x, a.y, b.x), n = mk(b.y, e.x, e.y);
                if (!in_query_domain(p, n)) { /* the per-point domain (include/ort.h) */
                    io.open[j] = 0xffffffffu;
                    if (io.bent) { float *o = io.bent + 3ull * j; o[0] = o[1] = o[2] = om_bits_f32(0x7fc00000u); }
                    if (io.states) io.states[j] = seed;
                    continue;
                }
                const float tm = io.radius ? io.radius[j] : __builtin_inff();
                bound = ray_bound(tm);
                reach = true;
                if (io.radius && bound > 0.0f && bound < 3.402823466e+38f && !io.q.tree_spheres) {
                    /* the root's record as traverse reads it: child 0 lo = a.xyz, hi = (a.w, b.x, b.y); child 1 lo = (b.z, b.w, cc.x), hi = cc.yzw */
                    const float4 *np = TABS ? tab + kTabTreelet : sv.nodes;
                    const float4 ra = np[0], rb = np[1], rc = np[2], rd = np[3];
                    const bool in0 = om_f32_bits(rd.x) != EMPTY_CHILD && ao_box_within(ra, rb.x, rb.y, p, bound);
                    const bool in1 = om_f32_bits(rd.y) != EMPTY_CHILD && ao_box_within(make_float4(rb.z, rb.w, rc.x, rc.y), rc.z, rc.w, p, bound);
                    reach = in0 || in1;
                    if (COUNTERS) c.nodes += 2;
                }
                point = j;
                org = p;
                const V3 un = normalize(n);
                unit_n[0] = un.x; unit_n[kBlock] = un.y; unit_n[2 * kBlock] = un.z;
                rng = seed ? seed : 1u; /* as job_seed: a zero xorshift state never leaves zero */
                bent[0] = bent[kBlock] = bent[2 * kBlock] = 0.0f;
                sample = 0; open = 0;
                busy = true;
            }
            if (start) { /* the draw, as unit op 20 composes it: one converged sin/cos for the lanes that start a sample */
                const float e0 = rng_01(rng), e1 = rng_01(rng);
                float sn, cs;
                ort_sincosf(2.0f * kPi * e1, &sn, &cs);
                dir = normalize(sample_lobe_n(cache_v3(unit_n), __builtin_sqrtf(e0), cs, sn));
                sample++;
                if (COUNTERS) c.rays++;
                if (!(bound > 0.0f)) { /* nothing is hit below 1e-6 */
                    open++; cache_add_v3(bent, dir);
                } else {
                    const bool forced = forced_fallback(sv, dir);
                    T.cur = 0;
                    T.sp = 0;
                    T.inv_d = mk(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z); /* as begin_ray, with the bound for Flt_Max */
                    reset_hit(h, bound);
                    prologue_tests<begin_of(F)>(sv, tab, org, dir, T.inv_d, h, c);
                    bool seen = false; /* the prologue's winner is one the reference is certain to test */
                    if (ORT_RARE(forced || raycast_needs_exact(io.q, org, dir, T.inv_d))) {
                        skip_fast_walk(T, h);
                    } else if (io.mats_nonzero && h.hit_prim != kNoPrim) {
                        const uint32_t word = sv.prim_info[info_index(sv, h.hit_prim)].chain;
                        const uint32_t first = word & 0x07ffffffu;
                        seen = (word >> 28) == 0u;
                        if (!seen && (word & kChainNested)) seen = in_rect_half_open(sv.chain_boxes[2u * first], sv.chain_boxes[2u * first + 1u], org);
                    }
                    if (!seen) {
                        if (!reach) T.cur = kTraversalDone; /* nothing of the tree below the bound: no walk, resolve_hit as after one */
                        tracing = held = true;
                    } /* seen: occluded, nothing to add */
                }
            }
        }
        /* a lane that neither traces, owns a point nor is entitled to another draw has none and will get none */
        if (ORT_BALLOT(tracing || busy || more) == 0ull) break;
        if (tracing) tracing = traverse<walk_of(F), kLdsStack, kBlock>(sv, org, dir, T, h, lds_stack, spill, tid, rv.refill_below, rv.descend_below, c, pr, kNoPrim, tab);
    }
    flush_counters(rv, c, COUNTERS);
}

#ifndef ORT_HOST_SIM
template <bool COUNTERS, bool TABS>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_WAVES_PER_EU, ORT_WAVES_PER_EU)))
ao_points(SceneView sv, RenderHot rv, AoIO io) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    __shared__ unsigned long long lds_pool[2 * (kBlock / 64)]; /* as raycast_rays */
    __shared__ float4 lds_tab[TABS ? kTabF4 : 1];
    __shared__ float lds_job[kAoCacheWords * kBlock]; /* the job's state that is touched once per sample (ao_lane) */
    if (TABS) fill_tab(sv, lds_tab);
    ao_lane<lf_if(COUNTERS, LF_COUNTERS) | lf_if(TABS, LF_TABS)>(sv, rv, io, lds_tab, lds_stack, lds_job + threadIdx.x, (int)threadIdx.x, blockIdx.x * (uint32_t)kBlock + threadIdx.x, wave_job_pool(rv, lds_pool));
}
#endif

/* ---- first-hit feature renders (ort_render_features): albedo, normal, depth, coverage and id planes of the camera ---------
 * A job is pixel (x, y) of a frame of the batch; its spp samples run on the PIXEL policy's stream of that pixel, job_seed(the
 * view's seed, y * W + x).  A sample is the render's own camera sample (produce_ray: rng_between for the aperture angle -- two
 * steps of the stream --, the deterministic sin/cos, view_aperture_point, normalize(focal - ap)) and then raycast_lane's ray
 * (ap, d): begin_ray, raycast_needs_exact, the walk with refill_below, resolve_hit, normalize(n), prim_src.  A sample that hits
 * a surface (mat != 0) counts and adds the material's albedo (emit of a light, diffuse otherwise), n and t to the job's sums,
 * each component a separately rounded add in sample order; the job ends with the sums divided by (float)spp.  Sample 0 also
 * names the pixel's ids.  Nothing else is drawn: the stream advances 2 * spp steps whatever is hit.
 * THE JOB SPACE is [view][8x8 block of the rect][pixel in block], as the PIXEL render's implicit one (produce_ray; block_pixel decodes it here): a wave's
 * jobs are one block -- coherent primary rays, and plane stores that coalesce.  A pixel of an edge block outside the rect is
 * a job that ends where it is drawn.
 * WHERE A SAMPLE STARTS is ao_lane's answer: the idle lanes first settle the finished sample's sums, the job's end and the
 * next pixel, and then meet at ONE converged ort_sincosf per pass of the outer loop.
 * WHERE THE JOB'S STATE LIVES.  The seven sums are touched once per sample and never inside the walk: seven per-lane LDS words
 * (job_cache: word k of a lane at job_cache[k * kBlock]), as ao_lane keeps its six.  The hit count, the stream, the pixel and
 * the view stay in registers.  The view's camera is read from the table at every sample's start (load_view_camera) and the
 * focal point recomputed there -- the render's expressions in the render's order, so the same bits -- instead of either being
 * held through the walk.  The ids go straight to memory at sample 0 (profiles/r18_features.md). */
constexpr int kFeatureCacheWords = 7; /* albedo.xyz, normal.xyz, depth */

/* the pixel lanes' shared steps (feature_lane, follow_lane, matte_lane).
   A job of the [view][8x8 block of the rect][pixel in block] space is drawn: the lane's view, pixel and stream, no sample started
   (follow_lane holds the same lines in place, see there) */
ORT_D JobTake take_pixel_job(const RenderHot &rv, PathState &P, unsigned long long *pool) {
    const unsigned long long j = draw_job(rv, pool);
    if (!(j < rv.c->job_count)) return JOB_NONE_LEFT;
    const uint32_t view = (uint32_t)(j / rv.c->view_jobs), within = (uint32_t)(j % rv.c->view_jobs);
    const BlockPixel bp = block_pixel(rv, within >> 6, within & 63u);
    if (bp.outside) return JOB_SKIPPED;
    const int x = bp.x, y = bp.y;
    P.job_index = view;
    P.pxy = (uint32_t)x | ((uint32_t)y << 16);
    P.rng = job_seed(om_f32_bits(rv.c->views[4u * (size_t)view].w), (uint32_t)(y * rv.W + x));
    P.sample = 0;
    return JOB_TAKEN;
}
/* the camera sample into P.org / P.dir, as produce_ray's steps compose it (primary_sample, compose_ray_*): one converged sin/cos
   for the lanes that start a sample */
ORT_D void view_camera_sample(const RenderHot &rv, PathState &P) {
    const ViewCamera cam = load_view_camera(rv, P.job_index);
    const V3 focal = view_focal_point(rv, P.pxy, cam);
    const float angle = rng_between(P.rng, 0.0f, 2 * kPi); /* ray.cpp:1232 */
    float sn, cs;
    ort_sincosf(angle, &sn, &cs);
    P.org = view_aperture_point(cam, kAperture, cs, sn); /* ray.cpp:1199, :1233-1234 */
    P.dir = normalize(sub(focal, P.org));                /* ray.cpp:1237 */
}
/* the job's end: the means of the albedo, normal and depth sums (job_cache's first seven words) into the planes asked for */
template <class IO>
ORT_D void write_feature_means(const IO &io, size_t at, const float *job_cache, uint32_t spp) {
    const float fs = (float)spp; /* ray.cpp:1428's division, component by component */
    if (io.albedo) { float *o = io.albedo + 3u * at; const V3 s = cache_v3(job_cache); o[0] = s.x / fs; o[1] = s.y / fs; o[2] = s.z / fs; }
    if (io.normal) { float *o = io.normal + 3u * at; const V3 s = cache_v3(job_cache + 3 * kBlock); o[0] = s.x / fs; o[1] = s.y / fs; o[2] = s.z / fs; }
    if (io.depth) io.depth[at] = job_cache[6 * kBlock] / fs;
}

template <uint32_t F>
ORT_D void feature_lane(const SceneView &sv, const RenderHot &rv, const FeatureIO &io, const float4 *tab, uint32_t *lds_stack, float *job_cache, const int tid,
                        const uint32_t lane_id, unsigned long long *pool) {
    static_assert(flavour_ok(F, LF_OF_LANE), "see flavour_ok");
    constexpr bool COUNTERS = F & LF_COUNTERS, TABS = F & LF_TABS;
    uint32_t spill[kSpillStack];
    PathState P; /* org, dir; rng; pxy; job_index: the view; sample: the samples of this pixel started so far */
    HitState h;
    Trav T;
    Counters c;
    Prof pr;
    const uint32_t spp = rv.c->spp;
    uint32_t hits = 0;
    bool tracing = false, held = false, busy = false, more = true; /* held: as raycast_lane's; busy: this lane owns a pixel */
    for (;;) {
        if (!tracing) {
            if (held) { /* the finished sample: raycast_lane's record, into the sums */
                resolve_hit<resolve_of(F), kLdsStack, kBlock>(sv, tab, P.org, P.dir, T.inv_d, lane_id, h, c, pr, lds_stack, spill, tid);
                if (P.sample == 1u && io.ids) {
                    const uint32_t src = h.hit_prim != kNoPrim ? io.q.prim_src[info_index(sv, h.hit_prim)] : kNoPrim;
                    const size_t at = plane_index(rv, P.job_index, P.pxy & 0xffffu, P.pxy >> 16);
                    io.ids[2u * at] = h.hit_mat;
                    io.ids[2u * at + 1u] = src;
                }
                if (h.hit_mat != 0u) {
                    Mat m;
                    if (TABS) m = load_mat(tab + kTabMats, h.hit_mat);
                    else m = load_mat(sv.materials, h.hit_mat);
                    const V3 a = m.is_light ? m.emit : m.kd;
                    const V3 n = normalize(h.hit_n); /* ray.cpp:817, as raycast_lane returns it */
                    hits++;
                    cache_add_v3(job_cache, a);
                    cache_add_v3(job_cache + 3 * kBlock, n);
                    job_cache[6 * kBlock] = job_cache[6 * kBlock] + h.best_t;
                }
                held = false;
            }
            bool start = false;
            for (;;) { /* the job's end and the next pixel */
                if (busy) {
                    if (P.sample < spp) { start = true; break; }
                    const size_t at = plane_index(rv, P.job_index, P.pxy & 0xffffu, P.pxy >> 16);
                    write_feature_means(io, at, job_cache, spp);
                    if (io.hits) io.hits[at] = hits;
                    if (io.states) io.states[at] = P.rng;
                    busy = false;
                }
                if (!more) break;
                const JobTake t = take_pixel_job(rv, P, pool);
                if (t == JOB_NONE_LEFT) { more = false; break; }
                if (t == JOB_SKIPPED) continue;
                hits = 0;
                for (int k = 0; k < kFeatureCacheWords; ++k) job_cache[k * kBlock] = 0.0f;
                busy = true;
            }
            if (start) {
                view_camera_sample(rv, P);
                P.sample++;
                begin_ray<begin_of(F), kLdsStack, kBlock>(sv, tab, P, T, h, c, pr, lds_stack, spill, tid);
                if (ORT_RARE(raycast_needs_exact(io.q, P.org, P.dir, T.inv_d))) skip_fast_walk(T, h);
                if (COUNTERS) c.rays++;
                tracing = held = true;
            }
        }
        /* a lane that neither traces, owns a pixel nor is entitled to another draw has none and will get none */
        if (ORT_BALLOT(tracing || busy || more) == 0ull) break;
        if (tracing) tracing = traverse<walk_of(F), kLdsStack, kBlock>(sv, P.org, P.dir, T, h, lds_stack, spill, tid, rv.refill_below, rv.descend_below, c, pr, kNoPrim, tab);
    }
    flush_counters(rv, c, COUNTERS);
}

/* TABS: the prologue shapes AND the materials fit their LDS slots (TAB_PRO, TAB_MATS: plan_features, ort_plan.h); otherwise both
   are read from HBM */
#ifndef ORT_HOST_SIM
template <bool COUNTERS, bool TABS>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_WAVES_PER_EU, ORT_WAVES_PER_EU)))
feature_pixels(SceneView sv, RenderHot rv, FeatureIO io) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    __shared__ unsigned long long lds_pool[2 * (kBlock / 64)]; /* as raycast_rays */
    __shared__ float4 lds_tab[TABS ? kTabF4 : 1];
    __shared__ float lds_job[kFeatureCacheWords * kBlock]; /* the job's sums (feature_lane) */
    if (TABS) fill_tab(sv, lds_tab);
    feature_lane<lf_if(COUNTERS, LF_COUNTERS) | lf_if(TABS, LF_TABS)>(sv, rv, io, lds_tab, lds_stack, lds_job + threadIdx.x, (int)threadIdx.x, blockIdx.x * (uint32_t)kBlock + threadIdx.x, wave_job_pool(rv, lds_pool));
}
#endif

/* ---- feature renders that follow mirrors and glass (ort_render_follow): the planes of the first non-specular vertex ----------
 * feature_lane's job, job space and camera sample; but a sample whose vertex is neither a light nor has a diffuse part goes on
 * as the render's own path does at a live non-light vertex (produce_ray: ray.cpp:1262, the roulette, sample_random_lights'
 * burn, sample_brdf's three draws, the 2 eps step through a refracting surface) until it meets a vertex that is one of the two,
 * or has bounced max_bounces times: THAT vertex is recorded.  No pdf, BSDF value or weight is evaluated; none advances the stream.
 * A separate lane, not a flavour of feature_lane: the first-hit kernels' code stays as it is (profiles/r28_isa_diff.txt).
 * WHERE A SAMPLE STARTS AND WHERE IT BOUNCES.  The idle lanes settle the finished vertex; those that bounce hold draw.phi, the
 * others end the sample (and perhaps the job, and draw the next pixel) and hold the aperture angle: both meet at ONE converged
 * ort_sincosf per pass of the outer loop, as pt_lane's two kinds of lanes do, and at one normalize behind it (ray.cpp:1158 / :1237).
 * WHERE THE JOB'S STATE LIVES.  feature_lane's seven sums and the path's length so far (L) are touched once per vertex and never
 * inside the walk: eight per-lane LDS words.  A ninth, for the sum of the recorded samples' bounces (B), is 544 bytes more than
 * the counters build with tables has at four blocks a CU (profiles/r28_follow.md), so B is a register, and the bounces of the path
 * in hand (b <= 64) share one with the hit count (<= 1 << 24): hb = hits | b << 25.  wo is not held: it is -dir at a bounce vertex
 * and -normalize(dir) at the primary one (ray.cpp:1241, sic).  The material is loaded once after resolve_hit, for the terminal
 * test and the draw alike. */
constexpr int kFollowCacheWords = 8; /* albedo.xyz, normal.xyz, depth; L */
constexpr uint32_t kFollowHitsMask = (1u << 25) - 1u, kFollowBounce = 1u << 25; /* hb: the hit count below, b above */

template <uint32_t F>
ORT_D void follow_lane(const SceneView &sv, const RenderHot &rv, const FollowIO &io, const float4 *tab, uint32_t *lds_stack, float *job_cache, const int tid,
                       const uint32_t lane_id, unsigned long long *pool) {
    static_assert(flavour_ok(F, LF_OF_LANE), "see flavour_ok");
    constexpr bool COUNTERS = F & LF_COUNTERS, TABS = F & LF_TABS;
    uint32_t spill[kSpillStack];
    PathState P; /* org, dir; rng; pxy; job_index: the view; sample: the samples of this pixel started so far */
    HitState h;
    Trav T;
    Counters c;
    Prof pr;
    const uint32_t spp = rv.c->spp;
    uint32_t hb = 0, B = 0;
    bool tracing = false, held = false, busy = false, more = true; /* as feature_lane's */
    for (;;) {
        if (!tracing) {
            bool bounce = false;
            float angle = 0.0f;
            BrdfDraw draw;
            Mat m;
            V3 n = mk(0, 0, 0);
            if (held) { /* the finished vertex: raycast_lane's record */
                resolve_hit<resolve_of(F), kLdsStack, kBlock>(sv, tab, P.org, P.dir, T.inv_d, lane_id, h, c, pr, lds_stack, spill, tid);
                uint32_t id_mat = h.hit_mat;
                bool died = false;
                if (h.hit_mat != 0u) {
                    if (TABS) m = load_mat(tab + kTabMats, h.hit_mat);
                    else m = load_mat(sv.materials, h.hit_mat);
                    n = normalize(h.hit_n); /* ray.cpp:817, as raycast_lane returns it */
                    const float L = job_cache[7 * kBlock] + h.best_t;
                    job_cache[7 * kBlock] = L;
                    if (m.is_light || len2(m.kd) > 0.0f || (hb >> 25) == io.max_bounces) { /* ray.cpp:1254, :1267; the cap */
                        const V3 a = m.is_light ? m.emit : m.kd;
                        hb++;
                        cache_add_v3(job_cache, a);
                        cache_add_v3(job_cache + 3 * kBlock, n);
                        job_cache[6 * kBlock] = job_cache[6 * kBlock] + L;
                        B += hb >> 25;
                    } else {
                        P.org = add(P.org, scale(h.best_t - kEps, P.dir)); /* ray.cpp:1262,1411 */
                        bounce = rng_01(P.rng) < rv.rr;                    /* ray.cpp:1280 */
                        if (bounce) {
                            /* sample_random_lights (ray.cpp:537-601): result unused, RNG advances; as produce_ray's */
                            rng_step(P.rng);
                            if (sv.light_count) {
                                uint32_t li = 0u;
                                if (sv.light_count != 1u) li = P.rng % sv.light_count;
                                uint32_t is_sphere;
                                if (TABS) is_sphere = ((const uint32_t *)tab)[4 * kTabLights + li];
                                else is_sphere = sv.light_is_sphere[li];
                                if (is_sphere) { rng_step(P.rng); rng_step(P.rng); rng_step(P.rng); rng_step(P.rng); }
                            }
                            draw = sample_brdf_draw<false>(P.rng, kRoughness, m);
                            angle = draw.phi;
                        } else {
                            died = true;
                            id_mat = 0u;
                        }
                    }
                }
                if (!bounce && P.sample == 1u && io.ids) { /* sample 0's last vertex; a path the roulette ended has none */
                    const uint32_t src = !died && h.hit_prim != kNoPrim ? io.q.prim_src[info_index(sv, h.hit_prim)] : kNoPrim;
                    const size_t at = plane_index(rv, P.job_index, P.pxy & 0xffffu, P.pxy >> 16);
                    io.ids[2u * at] = id_mat;
                    io.ids[2u * at + 1u] = src;
                }
                held = false;
            }
            bool start = false;
            if (!bounce) for (;;) { /* the job's end and the next pixel */
                if (busy) {
                    if (P.sample < spp) { start = true; break; }
                    const size_t at = plane_index(rv, P.job_index, P.pxy & 0xffffu, P.pxy >> 16);
                    write_feature_means(io, at, job_cache, spp);
                    if (io.hits) io.hits[at] = hb & kFollowHitsMask;
                    if (io.bounces) io.bounces[at] = B;
                    if (io.states) io.states[at] = P.rng;
                    busy = false;
                }
                if (!more) break;
                /* take_pixel_job's lines, in place: through the helper, in each of seven forms tried, these kernels' register
                   counts change (profiles/r30_lane_steps.md) */
                const unsigned long long j = draw_job(rv, pool);
                if (!(j < rv.c->job_count)) { more = false; break; }
                const uint32_t view = (uint32_t)(j / rv.c->view_jobs), within = (uint32_t)(j % rv.c->view_jobs);
                const BlockPixel bp = block_pixel(rv, within >> 6, within & 63u);
                if (bp.outside) continue;
                const int x = bp.x, y = bp.y;
                P.job_index = view;
                P.pxy = (uint32_t)x | ((uint32_t)y << 16);
                P.rng = job_seed(om_f32_bits(rv.c->views[4u * (size_t)view].w), (uint32_t)(y * rv.W + x));
                P.sample = 0;
                hb = 0;
                B = 0;
                for (int k = 0; k < kFollowCacheWords; ++k) job_cache[k * kBlock] = 0.0f;
                busy = true;
            }
            if (start || bounce) {
                /* the lanes that start a camera sample (as produce_ray composes it) and the lanes that bounce: one converged
                   sin/cos of the aperture angle / the lobe's azimuth, and one converged normalize of what comes out */
                ViewCamera cam;
                V3 focal = mk(0, 0, 0);
                if (start) {
                    cam = load_view_camera(rv, P.job_index);
                    focal = view_focal_point(rv, P.pxy, cam);
                    angle = rng_between(P.rng, 0.0f, 2 * kPi); /* ray.cpp:1232 */
                }
                float sn, cs;
                ort_sincosf(angle, &sn, &cs);
                V3 raw, ap = mk(0, 0, 0);
                bool is_trans = false;
                if (bounce) {
                    const V3 wo = (hb >> 25) == 0u ? neg(normalize(P.dir)) : neg(P.dir); /* ray.cpp:1241 (sic) / :1408 */
                    raw = sample_brdf_finish<false>(n, normalize(n), wo, m, draw, cs, sn, is_trans);
                } else {
                    ap = view_aperture_point(cam, kAperture, cs, sn); /* ray.cpp:1199, :1233-1234 */
                    raw = sub(focal, ap);                             /* ray.cpp:1237 */
                }
                const V3 unit = normalize(raw);
                if (bounce) {
                    if (is_trans) P.org = add(P.org, scale(2.0f * kEps, P.dir)); /* ray.cpp:1345-1348: dir is still the arriving direction */
                    P.dir = unit;
                    hb += kFollowBounce;
                } else {
                    P.org = ap;
                    P.dir = unit;
                    P.sample++;
                    hb &= kFollowHitsMask;
                    job_cache[7 * kBlock] = 0.0f;
                }
                begin_ray<begin_of(F), kLdsStack, kBlock>(sv, tab, P, T, h, c, pr, lds_stack, spill, tid);
                /* a primary ray is ort_raycast's; a bounce ray starts at a hit and needs no rule, as in the render */
                if (!bounce && ORT_RARE(raycast_needs_exact(io.q, P.org, P.dir, T.inv_d))) skip_fast_walk(T, h);
                if (COUNTERS) c.rays++;
                tracing = held = true;
            }
        }
        /* a lane that neither traces, owns a pixel nor is entitled to another draw has none and will get none */
        if (ORT_BALLOT(tracing || busy || more) == 0ull) break;
        if (tracing) tracing = traverse<walk_of(F), kLdsStack, kBlock>(sv, P.org, P.dir, T, h, lds_stack, spill, tid, rv.refill_below, rv.descend_below, c, pr, kNoPrim, tab);
    }
    flush_counters(rv, c, COUNTERS);
}

/* TABS: the prologue shapes, the materials AND the lights fit their LDS slots (plan_follow, ort_plan.h); otherwise all three are
   read from HBM */
#ifndef ORT_HOST_SIM
template <bool COUNTERS, bool TABS>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_WAVES_PER_EU, ORT_WAVES_PER_EU)))
follow_pixels(SceneView sv, RenderHot rv, FollowIO io) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    __shared__ unsigned long long lds_pool[2 * (kBlock / 64)]; /* as raycast_rays */
    __shared__ float4 lds_tab[TABS ? kTabF4 : 1];
    __shared__ float lds_job[kFollowCacheWords * kBlock]; /* the job's sums and L (follow_lane) */
    if (TABS) fill_tab(sv, lds_tab);
    follow_lane<lf_if(COUNTERS, LF_COUNTERS) | lf_if(TABS, LF_TABS)>(sv, rv, io, lds_tab, lds_stack, lds_job + threadIdx.x, (int)threadIdx.x, blockIdx.x * (uint32_t)kBlock + threadIdx.x, wave_job_pool(rv, lds_pool));
}
#endif

/* ---- ID-matte renders (ort_render_matte): per-pixel coverage per material, object or shape ----------------------------------
 * feature_lane's job, job space, camera sample and closest hit, word for word; what a sample leaves is not a sum but an id (the
 * hit's material, its shape as ort_raycast names it, or its object: io.q.prim_src is the table the mode reads, null BY_MATERIAL),
 * binned into the pixel's K slots by include/ort.h's rule.  A separate lane, not a flavour of feature_lane: every existing
 * kernel's code stays as it is (profiles/r29_isa_diff.txt).
 * WHERE THE SLOTS LIVE.  Sixteen words a lane do not fit in LDS beside the stack and the tables (feature_pixels' largest variant
 * holds 39 456 of the 40 960 bytes that four blocks a CU allow), and sixteen dynamically indexed registers are scratch.  So the
 * slots live where they end up: in the pixel's own K words of io.ids and io.counts, which belong to this lane alone for the length
 * of the job (as pt_groups keeps its G sums in the pixel's own output words).  The current run (id, length) is held in registers,
 * and only a sample whose id differs from the run's merges the run into the slots: slot assignment depends on the order of first
 * appearance alone, so merging runs in order gives the slots of the per-sample rule, and a pixel that sees one id touches memory
 * once, at its job's end.  used, other and the hit count are registers; no LDS word is the job's.  Plain vector loads and
 * stores, no atomics: a pixel has one owner, and a lane reads back only what it wrote itself. */
ORT_D void matte_merge(uint32_t *ids, uint32_t *counts, uint32_t slots, uint32_t &used, uint32_t &other, uint32_t id, uint32_t len) {
    for (uint32_t j = 0; j < used; ++j)
        if (ids[j] == id) { counts[j] = counts[j] + len; return; }
    if (used < slots) { ids[used] = id; counts[used] = len; used++; }
    else other += len;
}

/* the job's end: the used slots by count descending, ties by ascending id (a selection sort in place over at most
   ORT_MAX_MATTE_SLOTS entries), and (ORT_MATTE_EMPTY, 0) in the others */
ORT_D void matte_finish(uint32_t *ids, uint32_t *counts, uint32_t slots, uint32_t used) {
    for (uint32_t j = 0; j + 1u < used; ++j) {
        uint32_t best = j, bi = ids[j], bc = counts[j];
        const uint32_t ji = bi, jc = bc;
        for (uint32_t k = j + 1u; k < used; ++k) {
            const uint32_t ki = ids[k], kc = counts[k];
            if (kc > bc || (kc == bc && ki < bi)) { best = k; bi = ki; bc = kc; }
        }
        if (best != j) { ids[best] = ji; counts[best] = jc; ids[j] = bi; counts[j] = bc; }
    }
    for (uint32_t j = used; j < slots; ++j) { ids[j] = 0xffffffffu; counts[j] = 0u; }
}

template <uint32_t F>
ORT_D void matte_lane(const SceneView &sv, const RenderHot &rv, const MatteIO &io, const float4 *tab, uint32_t *lds_stack, const int tid, const uint32_t lane_id,
                      unsigned long long *pool) {
    static_assert(flavour_ok(F, LF_OF_LANE), "see flavour_ok");
    constexpr bool COUNTERS = F & LF_COUNTERS;
    uint32_t spill[kSpillStack];
    PathState P; /* org, dir; rng; pxy; job_index: the view; sample: the samples of this pixel started so far */
    HitState h;
    Trav T;
    Counters c;
    Prof pr;
    const uint32_t spp = rv.c->spp, slots = io.slots;
    uint32_t hits = 0, used = 0, other = 0, run_id = 0, run_len = 0; /* run_len == 0: no run yet */
    bool tracing = false, held = false, busy = false, more = true;   /* as feature_lane's */
    for (;;) {
        if (!tracing) {
            if (held) { /* the finished sample: raycast_lane's record, into the run or the slots */
                resolve_hit<resolve_of(F), kLdsStack, kBlock>(sv, tab, P.org, P.dir, T.inv_d, lane_id, h, c, pr, lds_stack, spill, tid);
                if (h.hit_mat != 0u) {
                    const uint32_t x = io.by == 0u ? h.hit_mat : io.q.prim_src[info_index(sv, h.hit_prim)];
                    hits++;
                    if (run_len != 0u && x == run_id) run_len++;
                    else {
                        if (run_len != 0u) {
                            const size_t at = plane_index(rv, P.job_index, P.pxy & 0xffffu, P.pxy >> 16) * slots;
                            matte_merge(io.ids + at, io.counts + at, slots, used, other, run_id, run_len);
                        }
                        run_id = x;
                        run_len = 1u;
                    }
                }
                held = false;
            }
            bool start = false;
            for (;;) { /* the job's end and the next pixel */
                if (busy) {
                    if (P.sample < spp) { start = true; break; }
                    const size_t px = plane_index(rv, P.job_index, P.pxy & 0xffffu, P.pxy >> 16), at = px * slots;
                    if (run_len != 0u) matte_merge(io.ids + at, io.counts + at, slots, used, other, run_id, run_len);
                    matte_finish(io.ids + at, io.counts + at, slots, used);
                    if (io.other) io.other[px] = other;
                    if (io.hits) io.hits[px] = hits;
                    if (io.states) io.states[px] = P.rng;
                    busy = false;
                }
                if (!more) break;
                const JobTake t = take_pixel_job(rv, P, pool);
                if (t == JOB_NONE_LEFT) { more = false; break; }
                if (t == JOB_SKIPPED) continue;
                hits = used = other = run_len = 0u;
                busy = true;
            }
            if (start) {
                view_camera_sample(rv, P);
                P.sample++;
                begin_ray<begin_of(F), kLdsStack, kBlock>(sv, tab, P, T, h, c, pr, lds_stack, spill, tid);
                if (ORT_RARE(raycast_needs_exact(io.q, P.org, P.dir, T.inv_d))) skip_fast_walk(T, h);
                if (COUNTERS) c.rays++;
                tracing = held = true;
            }
        }
        /* a lane that neither traces, owns a pixel nor is entitled to another draw has none and will get none */
        if (ORT_BALLOT(tracing || busy || more) == 0ull) break;
        if (tracing) tracing = traverse<walk_of(F), kLdsStack, kBlock>(sv, P.org, P.dir, T, h, lds_stack, spill, tid, rv.refill_below, rv.descend_below, c, pr, kNoPrim, tab);
    }
    flush_counters(rv, c, COUNTERS);
}

/* TABS: the prologue shapes fit their LDS slot and so do the materials (plan_matte is plan_features: TAB_PRO and TAB_MATS), though
   these lanes read no material; otherwise the shapes are read from HBM */
#ifndef ORT_HOST_SIM
template <bool COUNTERS, bool TABS>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_WAVES_PER_EU, ORT_WAVES_PER_EU)))
matte_pixels(SceneView sv, RenderHot rv, MatteIO io) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    __shared__ unsigned long long lds_pool[2 * (kBlock / 64)]; /* as raycast_rays */
    __shared__ float4 lds_tab[TABS ? kTabF4 : 1];
    if (TABS) fill_tab(sv, lds_tab);
    matte_lane<lf_if(COUNTERS, LF_COUNTERS) | lf_if(TABS, LF_TABS)>(sv, rv, io, lds_tab, lds_stack, (int)threadIdx.x, blockIdx.x * (uint32_t)kBlock + threadIdx.x, wave_job_pool(rv, lds_pool));
}
#endif

/* ---- radiance queries (ort_radiance): the path-traced light that arrives along a caller's ray ---------------------------
 * The plain path-trace loop (pt_lane) with the ray array for a job space (produce_ray's RAYS flag): a lane draws a ray index from
 * its wave's batch, runs spp samples of the reference's sample body (ray.cpp:1247-1426) from that ray on one xorshift stream,
 * and writes the mean and the stream's state.  Primary rays are a caller's, so they pass raycast_needs_exact as the rays of
 * ort_raycast do (inside the per-ray domain: an axis-aligned direction with boxes in the tree, an origin outside the scene's
 * box with quadrics in it) and then skip the fast traversal: resolve_hit re-casts them exactly.  Bounce rays start at hits and
 * need no rule, as in the render.  No ray exchange, no five-waves build, no wide tree, no wavefront mode (ort_plan.h). */
/* ADAPT: the adaptive query (ort_radiance_adaptive): the same loop, the job ending where produce_ray's stopping rule says */
/* HEMI: the irradiance queries (ort_irradiance, ort_irradiance_adaptive): the same loop over points, every sample's primary
   direction drawn in the lane (produce_ray's HEMI flag); the drawn direction passes raycast_needs_exact like a caller's */
/* SH: the SH light-probe query (ort_probe_sh): HEMI's loop with the direction drawn over the whole sphere and the nine SH sums
   beside the colour's (produce_ray's SH flag); dir_cache is where the lane keeps a sample's primary direction */
template <uint32_t F>
ORT_D void radiance_lane(const SceneView &sv, const RenderHot &rv, const float4 *tab, uint32_t *lds_stack, const int tid, const uint32_t lane_id,
                         unsigned long long *pool, float *dir_cache = nullptr /* SH: the lane's own three words, kBlock apart */) {
    constexpr uint32_t JOB = F | LF_IMPLICIT | LF_RAYS; /* the caller names what varies: COUNTERS, DIFFUSE, TABS, ADAPT, HEMI, SH */
    static_assert(flavour_ok(JOB, LF_OF_LANE), "see flavour_ok");
    constexpr bool COUNTERS = F & LF_COUNTERS;
    uint32_t spill[kSpillStack];
    const uint32_t spp_u = rv.c->spp;
    Prof pr;
    PathState P;
    AdaptState A; /* ADAPT only */
    HitState h;
    Trav T;
    Counters c;
    bool tracing = false;
    for (;;) {
        if (!tracing) {
            if (P.ps == PS_HIT) resolve_hit<resolve_of(F), kLdsStack, kBlock>(sv, tab, P.org, P.dir, T.inv_d, lane_id, h, c, pr, lds_stack, spill, tid);
            if constexpr (F & LF_SH) tracing = produce_ray<JOB>(sv, rv, tab, P, h, c, pr, dir_cache, kBlock, spp_u, nullptr, false, pool, &A);
            else tracing = produce_ray<JOB>(sv, rv, tab, P, h, c, pr, nullptr, 0, spp_u, nullptr, false, pool, &A);
            if (tracing) {
                begin_ray<begin_of(F), kLdsStack, kBlock>(sv, tab, P, T, h, c, pr, lds_stack, spill, tid);
                if (P.primary) { /* the facts raycast_needs_exact asks for, from the launch's copy (kept in this form: in a helper the radiance kernels' code moves) */
                    RaycastIO q{};
                    q.tree_spheres = rv.c->ray_tree_spheres; q.tree_quadrics = rv.c->ray_tree_quadrics; q.tree_boxes = rv.c->ray_tree_boxes;
                    for (int k = 0; k < 3; ++k) { q.lo[k] = rv.c->ray_lo[k]; q.hi[k] = rv.c->ray_hi[k]; }
                    if (ORT_RARE(raycast_needs_exact(q, P.org, P.dir, T.inv_d))) skip_fast_walk(T, h);
                }
                if (COUNTERS) c.rays++;
            }
        }
        if (ORT_BALLOT(P.ps != PS_DONE) == 0ull) break;
        if (tracing) tracing = traverse<walk_of(F), kLdsStack, kBlock>(sv, P.org, P.dir, T, h, lds_stack, spill, tid, rv.refill_below, rv.descend_below, c, pr, kNoPrim, tab);
    }
    flush_counters(rv, c, COUNTERS);
}

/* DIFFUSE and TABS as pt_persistent's: the BSDF flavour, and all three small tables in LDS or all of them in HBM */
#ifndef ORT_HOST_SIM
template <bool COUNTERS, bool DIFFUSE, bool TABS>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_WAVES_PER_EU, ORT_WAVES_PER_EU)))
radiance_rays(SceneView sv, RenderHot rv) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    __shared__ unsigned long long lds_pool[2 * (kBlock / 64)]; /* as raycast_rays */
    __shared__ float4 lds_tab[TABS ? kTabF4 : 1];
    if (TABS) fill_tab(sv, lds_tab);
    radiance_lane<lf_if(COUNTERS, LF_COUNTERS) | lf_if(DIFFUSE, LF_DIFFUSE) | lf_if(TABS, LF_TABS)>(sv, rv, lds_tab, lds_stack, (int)threadIdx.x, blockIdx.x * (uint32_t)kBlock + threadIdx.x, wave_job_pool(rv, lds_pool));
}

/* the adaptive query's eight, as radiance_rays */
template <bool COUNTERS, bool DIFFUSE, bool TABS>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_WAVES_PER_EU, ORT_WAVES_PER_EU)))
radiance_adaptive_rays(SceneView sv, RenderHot rv) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    __shared__ unsigned long long lds_pool[2 * (kBlock / 64)]; /* as raycast_rays */
    __shared__ float4 lds_tab[TABS ? kTabF4 : 1];
    if (TABS) fill_tab(sv, lds_tab);
    radiance_lane<lf_if(COUNTERS, LF_COUNTERS) | lf_if(DIFFUSE, LF_DIFFUSE) | lf_if(TABS, LF_TABS) | LF_ADAPT>(sv, rv, lds_tab, lds_stack, (int)threadIdx.x, blockIdx.x * (uint32_t)kBlock + threadIdx.x, wave_job_pool(rv, lds_pool));
}

/* the irradiance queries' sixteen (ort_kernels_irradiance.hip), as radiance_rays and radiance_adaptive_rays: rv.c->rays holds points */
template <bool COUNTERS, bool DIFFUSE, bool TABS>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_WAVES_PER_EU, ORT_WAVES_PER_EU)))
irradiance_points(SceneView sv, RenderHot rv) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    __shared__ unsigned long long lds_pool[2 * (kBlock / 64)]; /* as raycast_rays */
    __shared__ float4 lds_tab[TABS ? kTabF4 : 1];
    if (TABS) fill_tab(sv, lds_tab);
    radiance_lane<lf_if(COUNTERS, LF_COUNTERS) | lf_if(DIFFUSE, LF_DIFFUSE) | lf_if(TABS, LF_TABS) | LF_HEMI>(sv, rv, lds_tab, lds_stack, (int)threadIdx.x, blockIdx.x * (uint32_t)kBlock + threadIdx.x, wave_job_pool(rv, lds_pool));
}
template <bool COUNTERS, bool DIFFUSE, bool TABS>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_WAVES_PER_EU, ORT_WAVES_PER_EU)))
irradiance_adaptive_points(SceneView sv, RenderHot rv) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    __shared__ unsigned long long lds_pool[2 * (kBlock / 64)]; /* as raycast_rays */
    __shared__ float4 lds_tab[TABS ? kTabF4 : 1];
    if (TABS) fill_tab(sv, lds_tab);
    radiance_lane<lf_if(COUNTERS, LF_COUNTERS) | lf_if(DIFFUSE, LF_DIFFUSE) | lf_if(TABS, LF_TABS) | LF_ADAPT | LF_HEMI>(sv, rv, lds_tab, lds_stack, (int)threadIdx.x, blockIdx.x * (uint32_t)kBlock + threadIdx.x, wave_job_pool(rv, lds_pool));
}
/* the SH light-probe query's eight (ort_kernels_irradiance.hip), as irradiance_points; lds_dir holds every lane's primary direction,
   dir[component][lane] as the pt_* kernels' lds_focal: 3 KB beside the stack's 24, so four blocks a CU still fit */
template <bool COUNTERS, bool DIFFUSE, bool TABS>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_WAVES_PER_EU, ORT_WAVES_PER_EU)))
probe_sh_points(SceneView sv, RenderHot rv) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    __shared__ float lds_dir[3 * kBlock];
    __shared__ unsigned long long lds_pool[2 * (kBlock / 64)]; /* as raycast_rays */
    __shared__ float4 lds_tab[TABS ? kTabF4 : 1];
    if (TABS) fill_tab(sv, lds_tab);
    radiance_lane<lf_if(COUNTERS, LF_COUNTERS) | lf_if(DIFFUSE, LF_DIFFUSE) | lf_if(TABS, LF_TABS) | LF_HEMI | LF_SH>(sv, rv, lds_tab, lds_stack, (int)threadIdx.x, blockIdx.x * (uint32_t)kBlock + threadIdx.x, wave_job_pool(rv, lds_pool),
                                                                                                                     lds_dir + threadIdx.x);
}
#endif

} // namespace ORT_NS

#endif /* ORT_LANE_H */
