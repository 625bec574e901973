/*
 * ort_kernels.hip -- host side of the path-trace kernels: scene upload and the render and ray-query calls as HIP plumbing
 * (device_render turns the LaunchPlan of ort_plan.h, where the launch policy lives, into buffers and launches), and the
 * kernels' four-waves-per-SIMD build (the lane code itself is ort_lane.h).  A plan becomes a launch by its KernelVariant
 * (plan_variant, ort_plan.h): a variant of a pixel-job kind's family, built in full, goes to the sibling unit's one entry point
 * (ort_launch_pixel_jobs); for the others kLaunchers below pairs every entry of that header's list of built kernels with this
 * unit's kernel, which that instantiates, or a sibling unit's launcher.  A render and a ray query share the steps around their kernels.
 * The denoiser's kernels (ort_denoise.h) are launched from here too (device_denoise): they need no scene and no plan.
 * So are the sample planner's (ort_sampleplan.h, device_plan_samples) and the matte mask's (ort_mattemask.h, device_matte_mask).
 */
#include <algorithm>
#include <memory>
#include <type_traits>

#define ORT_LIBRARY_KERNELS 1 /* this unit also holds the kernels that are no templates: wf_*, unit_eval, combine_chunks* */
#include "ort_lane.h" /* in namespace ort, at the header's own limits; it declares the sibling units' launchers */
#include "ort_plan.h"
#include "ort_setup.h"
#include "ort_denoise.h" /* the denoiser's pixel functions and kernels (namespace ortdn); device_denoise below launches them */
#include "ort_sampleplan.h" /* the sample planner's (namespace ortsp); device_plan_samples below launches them */
#include "ort_mattemask.h" /* the matte mask's (namespace ortmm); device_matte_mask below launches it */

#ifndef ORT_HOST_SIM /* tools/host_sim.cpp drives the lane code itself and has no device */
namespace ort {

using namespace ortd;

static_assert(kPlanBlock == (uint32_t)kBlock && kPlanLdsStack == (uint32_t)kLdsStack && kPlanStashVecs == kStashVecs && kPlanCapL == kCapL &&
              kPlanCapR == kCapR && (int)PLAN_JOBS_EXPLICIT == (int)JOBS_EXPLICIT && /* the table caps: ort_setup.h */
              (int)PLAN_JOBS_PIXEL == (int)JOBS_PIXEL && (int)PLAN_JOBS_CHUNK == (int)JOBS_CHUNK,
              "ort_plan.h counts with the lane code's limits");

/* ---- host side --------------------------------------------------------------------------- */
#define ORT_HIP(call)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            *err = std::string(#call) + ": " + hipGetErrorString(e_);                          \
            return ORT_ERR_HIP;                                                                \
        }                                                                                      \
    } while (0)

/* a device allocation that frees itself (on the device that is current then: ~DeviceScene sets it); move-only */
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); return *this; }
    ~DevBuf() { if (p) (void)hipFree(p); }
    /* at least `need` bytes; what it held is lost when it has to grow */
    int ensure(size_t need, std::string *err) {
        if (bytes >= need && p) return ORT_OK;
        if (p) ORT_HIP(hipFree(p));
        p = nullptr;
        bytes = 0;
        ORT_HIP(hipMalloc(&p, need ? need : 16));
        bytes = need;
        return ORT_OK;
    }
    template <typename T> T *as() const { return (T *)p; }
};

/* what an upload creates on its device, and owns: the buffers free themselves, the rest goes here */
struct DeviceScene {
    explicit DeviceScene(int device_index) : device(device_index) {}
    ~DeviceScene() { /* the members' destructors run after this body: on this device */
        (void)hipSetDevice(device);
        if (h_active) (void)hipHostFree(h_active);
        for (hipEvent_t ev : {ev0, ev1, ev_done})
            if (ev) (void)hipEventDestroy(ev);
    }
    const int device;
    Knobs knobs;
    DevBuf nodes, tris, spheres, boxes, cyls, materials;
    DevBuf nodes4; /* the 4-wide form of the tree (uploaded when it exists and its depth fits the traversal stacks) */
    DevBuf prim_info;
    uint32_t info_box = 0, info_cyl = 0, info_sphere = 0;
    DevBuf light_is_sphere;
    DevBuf tab; /* image of the LDS tables (kTabF4 float4) */
    DevBuf cold; /* SceneCold */
    DevBuf rv_dev; /* the RenderView of the render in flight (RenderHot::c) */
    DevBuf view_tab; /* ... and, for a batch of views, its camera table (RenderView::views) */
    std::vector<float> view_tab_host; /* the source of that upload: the scene's, so that it outlives a call that does not wait */
    DevBuf group_tab; /* ... and, for a light-group render, its group table (RenderView::group_of_material), uploaded per call */
    std::vector<uint8_t> group_tab_host; /* likewise its source */
    uint32_t tab_flags = 0;
    uint32_t light_count = 0;
    bool diffuse_only = false; /* no surface material can enter the specular / transmission blocks */
    DevBuf ref_nodes, ref_recs, chain_boxes;
    DevBuf tri_order, sphere_order, box_order, cyl_order;
    DevBuf bfs_pool, bfs_locks;
    uint32_t bfs_queue_cap = 0, bfs_queue_count = 0;
    unsigned int max_blocks = 0;
    DevBuf ctrl_buf; /* 128 x u64: [0] next_job, [1..5] counters */
    unsigned long long *ctrl() const { return ctrl_buf.as<unsigned long long>(); }
    DevBuf partial, staging, jobs, states;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_done = nullptr; /* end of the last render enqueued on this scene */
    bool inflight = false;        /* that render was returned from without waiting (device form, stats == NULL) */
    int cu_count = 0;
    DevBuf stash; /* ray exchange: the waves' stashes */
    DevBuf drain; /* ORT_DEBUG_DRAIN: per-wave end times */
    DevBuf wf_mem; /* wavefront state, carved into the WfView arrays */
    unsigned long long *h_active = nullptr; /* pinned */
    /* ray queries (device_raycast): the shape table, built at the first query on this upload, and the host path's staging */
    DevBuf prim_src;
    DevBuf obj_src; /* ID-matte renders BY_OBJECT (device_render_matte): prim_src with a triangle's word naming its mesh, built at the first such render */
    float scene_lo[3] = {0, 0, 0}, scene_hi[3] = {0, 0, 0}; /* shapes and camera (raycast_needs_exact) */
    bool scene_box_known = false;
    DevBuf query_stage[7]; /* the i-th array of the host form in flight (run_query); seven: the radiance queries' six and the SH light-probe query's sums */
};

int device_count(int *n, std::string *err) {
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *n = 0; *err = std::string("hipGetDeviceCount: ") + hipGetErrorString(e); return ORT_ERR_NO_DEVICE; }
    *n = c;
    return ORT_OK;
}

template <typename T>
static int upload_vec(const std::vector<T> &v, DevBuf *dst, std::string *err) {
    size_t bytes = v.size() * sizeof(T);
    int rc = dst->ensure(bytes, err);
    if (rc) return rc;
    if (bytes) ORT_HIP(hipMemcpy(dst->p, v.data(), bytes, hipMemcpyHostToDevice));
    return ORT_OK;
}

void device_release(Scene *scene) {
    delete scene->dev;
    scene->dev = nullptr;
}

int device_upload(Scene *scene, int device, std::string *err) {
    int n = 0;
    int rc = device_count(&n, err);
    if (rc != ORT_OK) return rc;
    if (n <= 0) { *err = "no HIP device visible"; return ORT_ERR_NO_DEVICE; }
    if (device < 0 || device >= n) { *err = "device index out of range"; return ORT_ERR_INVALID; }
    device_release(scene);
    ORT_HIP(hipSetDevice(device));
    /* the scene becomes resident (check_resident) once everything is there: a failure on the way frees what was built */
    std::unique_ptr<DeviceScene> owner(new DeviceScene(device));
    DeviceScene *d = owner.get();
    const Tree &t = scene->tree;
    if ((rc = upload_vec(t.nodes, &d->nodes, err))) return rc;
    /* a traversal of the wide tree stacks at most three entries per level; the smallest stack is resolve_hit's re-traversal */
    if (!t.nodes4.empty() && 3u * t.max_depth4 <= (uint32_t)(kLdsStack - 4 + kSpillStack))
        if ((rc = upload_vec(t.nodes4, &d->nodes4, err))) return rc;
    if ((rc = upload_vec(t.tris, &d->tris, err))) return rc;
    if ((rc = upload_vec(t.spheres, &d->spheres, err))) return rc;
    if ((rc = upload_vec(t.boxes, &d->boxes, err))) return rc;
    if ((rc = upload_vec(t.cyls, &d->cyls, err))) return rc;
    {
        std::vector<PrimInfo> info;
        build_prim_info(t, scene->ref, info, d->info_box, d->info_cyl, d->info_sphere);
        if ((rc = upload_vec(info, &d->prim_info, err))) return rc;
    }
    const std::vector<DevMaterial> mats = dev_materials(*scene);
    if ((rc = upload_vec(mats, &d->materials, err))) return rc;
    d->diffuse_only = materials_diffuse_only(mats);
    const std::vector<uint32_t> lis = light_sphere_flags(*scene);
    d->light_count = (uint32_t)lis.size();
    if ((rc = upload_vec(lis, &d->light_is_sphere, err))) return rc;
    {
        std::vector<F4> tab; /* the image of the LDS tables (pack_lds_tables) */
        d->tab_flags = pack_lds_tables(t, mats, lis, tab);
        if ((rc = upload_vec(tab, &d->tab, err))) return rc;
    }
    const RefTree &rt = scene->ref;
    if ((rc = upload_vec(rt.nodes, &d->ref_nodes, err))) return rc;
    if ((rc = upload_vec(rt.recs, &d->ref_recs, err))) return rc;
    if ((rc = upload_vec(rt.chain_boxes, &d->chain_boxes, err))) return rc;
    if ((rc = upload_vec(rt.tri_order, &d->tri_order, err))) return rc;
    if ((rc = upload_vec(rt.sphere_order, &d->sphere_order, err))) return rc;
    if ((rc = upload_vec(rt.box_order, &d->box_order, err))) return rc;
    if ((rc = upload_vec(rt.cyl_order, &d->cyl_order, err))) return rc;
    if ((rc = d->ctrl_buf.ensure(128 * sizeof(unsigned long long), err))) return rc;
    ORT_HIP(hipMemset(d->ctrl(), 0, 128 * sizeof(unsigned long long)));
    ORT_HIP(hipEventCreate(&d->ev0));
    ORT_HIP(hipEventCreate(&d->ev1));
    ORT_HIP(hipEventCreateWithFlags(&d->ev_done, hipEventDisableTiming));
    hipDeviceProp_t prop;
    ORT_HIP(hipGetDeviceProperties(&prop, device));
    d->cu_count = prop.multiProcessorCount;
    d->knobs = read_knobs();
    d->max_blocks = upload_max_blocks(d->cu_count, d->knobs); /* persistent grid: 4 workgroups of 256 lanes per CU */
    /* fallback queues: one entry per reference-tree node each, as many as fit the budget */
    d->bfs_queue_cap = (uint32_t)rt.nodes.size() + 8u;
    size_t fit = kBfsPoolBytes / ((size_t)d->bfs_queue_cap * sizeof(uint32_t));
    d->bfs_queue_count = (uint32_t)(fit < 16 ? 16 : (fit > kBfsPoolQueues ? kBfsPoolQueues : fit));
    if ((rc = d->bfs_pool.ensure((size_t)d->bfs_queue_count * d->bfs_queue_cap * sizeof(uint32_t), err))) return rc;
    if ((rc = d->bfs_locks.ensure((size_t)d->bfs_queue_count * kBfsLockStride * sizeof(uint32_t), err))) return rc;
    ORT_HIP(hipMemset(d->bfs_locks.p, 0, d->bfs_locks.bytes));
    ORT_HIP(hipHostMalloc((void **)&d->h_active, sizeof(unsigned long long)));
    {
        SceneCold cold{};
        cold.ref_nodes = d->ref_nodes.as<const float4>(); cold.ref_recs = d->ref_recs.as<const uint32_t>();
        cold.tri_order = d->tri_order.as<const uint32_t>(); cold.sphere_order = d->sphere_order.as<const uint32_t>();
        cold.box_order = d->box_order.as<const uint32_t>(); cold.cyl_order = d->cyl_order.as<const uint32_t>();
        cold.bfs_pool = d->bfs_pool.as<uint32_t>(); cold.bfs_locks = d->bfs_locks.as<uint32_t>();
        cold.bfs_queue_cap = d->bfs_queue_cap; cold.bfs_queue_count = d->bfs_queue_count;
        cold.fallback_counters = d->ctrl() + 6;
        if ((rc = d->rv_dev.ensure(sizeof(RenderView), err))) return rc;
        if ((rc = d->cold.ensure(sizeof(SceneCold), err))) return rc;
        ORT_HIP(hipMemcpy(d->cold.p, &cold, sizeof(SceneCold), hipMemcpyHostToDevice));
    }
    scene->dev = owner.release();
    return ORT_OK;
}

int device_unit_eval(int device, const void *records, uint32_t n, float *out, std::string *err) {
    int count = 0;
    int rc = device_count(&count, err);
    if (rc != ORT_OK) return rc;
    if (device < 0 || device >= count) { *err = "no such HIP device"; return ORT_ERR_NO_DEVICE; }
    ORT_HIP(hipSetDevice(device));
    DevBuf d_rec, d_out;
    if ((rc = d_rec.ensure((size_t)n * 100u + 16, err)) || (rc = d_out.ensure((size_t)n * 32u + 16, err))) return rc;
    ORT_HIP(hipMemcpy(d_rec.p, records, (size_t)n * 100u, hipMemcpyHostToDevice));
    if (n) hipLaunchKernelGGL(unit_eval, dim3((n + 63) / 64), dim3(64), 0, 0, d_rec.as<const uint32_t>(), n, d_out.as<float>());
    ORT_HIP(hipGetLastError());
    ORT_HIP(hipMemcpy(out, d_out.p, (size_t)n * 32u, hipMemcpyDeviceToHost));
    return ORT_OK;
}

/* wavefront mode: all slots alternate between wf_shade (produce the next ray) and wf_trace (closest
   hit) until no slot produces a ray any more.  The host only learns "finished" by reading a
   counter, so it launches iterations in batches and checks after each batch. */
template <bool COUNTERS>
static int launch_wavefront(DeviceScene *d, const LaunchPlan &, const SceneView &sv, const RenderView &rvf, const RenderHot &rv, hipStream_t stream, std::string *err) {
    const uint32_t kMaxSlots = 1u << 21;
    unsigned long long want = rvf.job_count < kMaxSlots ? rvf.job_count : kMaxSlots;
    uint32_t S = (uint32_t)((want + kBlock - 1) / kBlock) * kBlock;
    if (S == 0) S = kBlock;
    const size_t per_slot = 16 + 8 + 16 + 4 + 16 + 16 + 16 + 16 + 4;
    size_t need = (size_t)S * per_slot + 4096;
    int rc = d->wf_mem.ensure(need, err);
    if (rc) return rc;
    WfView wf{};
    wf.slots = S;
    char *base = d->wf_mem.as<char>();
    auto carve = [&](size_t bytes) { char *p = base; base += (bytes + 255) & ~(size_t)255; return p; };
    wf.active = (unsigned long long *)carve(256);
    wf.od0 = (float4 *)carve((size_t)S * 16); wf.hit0 = (float4 *)carve((size_t)S * 16);
    wf.p0 = (float4 *)carve((size_t)S * 16); wf.p1 = (float4 *)carve((size_t)S * 16); wf.p2 = (float4 *)carve((size_t)S * 16);
    wf.p3 = (uint4 *)carve((size_t)S * 16);
    wf.od1 = (float2 *)carve((size_t)S * 8);
    wf.hitp = (uint32_t *)carve((size_t)S * 4); wf.flags = (uint32_t *)carve((size_t)S * 4);
    if ((size_t)(base - d->wf_mem.as<char>()) > d->wf_mem.bytes) { *err = "internal: wavefront state carve overflow"; return ORT_ERR_INVALID; }

    unsigned int blocks = S / kBlock;
    unsigned int grid = blocks < d->max_blocks * 2u ? blocks : d->max_blocks * 2u;
    hipLaunchKernelGGL(wf_init, dim3(blocks), dim3(kBlock), 0, stream, wf);
    ORT_HIP(hipGetLastError());
    const int batch = 32;
    for (;;) {
        for (int it = 0; it < batch; ++it) {
            int last = (it == batch - 1);
            if (last) ORT_HIP(hipMemsetAsync(wf.active, 0, sizeof(unsigned long long), stream));
            hipLaunchKernelGGL(wf_shade<COUNTERS>, dim3(grid), dim3(kBlock), 0, stream, sv, rv, wf, last);
            hipLaunchKernelGGL(wf_trace<COUNTERS>, dim3(grid), dim3(kBlock), 0, stream, sv, rv, wf);
        }
        ORT_HIP(hipGetLastError());
        ORT_HIP(hipMemcpyAsync(d->h_active, wf.active, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        ORT_HIP(hipStreamSynchronize(stream));
        if (*d->h_active == 0ull) break;
    }
    return ORT_OK;
}

/* the five-waves unit's kernels, as a launcher of launch_wavefront's kind */
static int launch_five_waves(DeviceScene *, const LaunchPlan &pl, const SceneView &sv, const RenderView &, const RenderHot &hot, hipStream_t stream, std::string *) {
    ort_launch_w5(plan_variant(pl), pl.grid, stream, sv, hot);
    return ORT_OK;
}

/* What launches each of the listed kernels (kBuiltKernels, ort_plan.h), in that list's order: a kernel of this unit, which its
   entry here instantiates, or the host function that launches what another family is made of */
struct Launcher {
    KernelVariant variant;
    void (*kernel)(SceneView, RenderHot);
    int (*host)(DeviceScene *, const LaunchPlan &, const SceneView &, const RenderView &, const RenderHot &, hipStream_t, std::string *);
};
template <bool C, bool D, bool T, bool I = false, bool W = false>
constexpr Launcher loop() { return {{KF_LOOP, C, D, T, I, W}, pt_persistent<C, D, T, I, W>, nullptr}; }
template <bool C, bool D, bool T, bool I = false>
constexpr Launcher views() { return {{KF_LOOP_VIEWS, C, D, T, I, false}, pt_persistent<C, D, T, I, false, true>, nullptr}; }
template <bool C, bool D>
constexpr Launcher exchange() { return {{KF_EXCHANGE, C, D, true, true, false}, pt_persistent_x<C, D>, nullptr}; }
constexpr Launcher five(bool d) { return {{KF_FIVE, false, d, true, true, false}, nullptr, launch_five_waves}; }
constexpr Launcher kLaunchers[] = {
    {{KF_WAVEFRONT, false, false, false, false, false}, nullptr, launch_wavefront<false>},
    {{KF_WAVEFRONT, true, false, false, false, false}, nullptr, launch_wavefront<true>},
    loop<false, false, false>(), loop<false, false, true>(), loop<false, false, true, true>(),
    loop<false, true, false>(), loop<false, true, true>(), loop<false, true, true, true>(),
    loop<true, false, false>(), loop<true, false, true>(), loop<true, true, false>(), loop<true, true, true>(),
    loop<false, false, true, true, true>(), loop<false, true, true, true, true>(), loop<true, false, true, false, true>(),
    views<false, false, false>(), views<false, false, true, true>(), views<false, true, false>(), views<false, true, true, true>(),
    views<true, false, false>(), views<true, false, true>(),
    exchange<false, false>(), exchange<false, true>(), exchange<true, true>(),
    five(false), five(true),
};
constexpr bool launchers_match(size_t i = 0) { return i == kBuiltKernelCount || (kLaunchers[i].variant == kBuiltKernels[i] && launchers_match(i + 1)); }
static_assert(sizeof(kLaunchers) / sizeof(kLaunchers[0]) == kBuiltKernelCount && launchers_match(),
              "kLaunchers holds the entries of kBuiltKernels (ort_plan.h), all of them, in its order");

/* the kernel a plan names, launched: a pixel-job kind's by the sibling unit that builds those families in full, any other by its
   place in the list; a plan that names one nobody built is an error, not a fallback */
static int launch_path_tracer(DeviceScene *d, const LaunchPlan &pl, const SceneView &sv, const RenderView &rv, const RenderHot &hot, hipStream_t stream, std::string *err) {
    const KernelVariant v = plan_variant(pl);
    if (!variant_built(v)) { *err = "internal: no kernel is built for this launch plan"; return ORT_ERR_INTERNAL; }
    if (pixel_job_family(v.family)) { ort_launch_pixel_jobs(v, pl.grid, stream, sv, hot); return ORT_OK; }
    const size_t i = built_index(v);
    if (kLaunchers[i].host) return kLaunchers[i].host(d, pl, sv, rv, hot, stream, err);
    hipLaunchKernelGGL(kLaunchers[i].kernel, dim3(pl.grid), dim3(kBlock), 0, stream, sv, hot);
    return ORT_OK;
}

/* a render or ray query that was returned from without waiting: waited for, and its tripwire checked (one call at a time
   per scene: the job counter and the work counters in ctrl, and the RenderView in rv_dev, belong to the scene).  A fallback
   queue overflow cannot happen by construction, and must not go unnoticed if it does. */
static int settle_inflight(DeviceScene *d, std::string *err, const char *what = "the previous render on this scene overflowed a reference-order fallback queue") {
    if (!d->inflight) return ORT_OK;
    ORT_HIP(hipEventSynchronize(d->ev_done));
    d->inflight = false;
    unsigned long long ovf = 0;
    ORT_HIP(hipMemcpy(&ovf, d->ctrl() + 7, sizeof(ovf), hipMemcpyDeviceToHost));
    if (ovf) { *err = what; return ORT_ERR_UNSUPPORTED; }
    return ORT_OK;
}

/* ---- the steps of every launch on a scene, render or ray query, around its kernels -------------------------------------------- */
/* it starts from a zeroed ctrl, and its RenderView points into it: the job counter and the work counters */
static int reset_ctrl(DeviceScene *d, RenderView *rv, hipStream_t stream, std::string *err) {
    rv->next_job = d->ctrl();
    rv->counters = d->ctrl() + 1;
    ORT_HIP(hipMemsetAsync(d->ctrl(), 0, 128 * sizeof(unsigned long long), stream));
    return ORT_OK;
}
/* ... and from its RenderView in HBM (pageable source: the copy is staged before the call returns); the kernels get the few
   fields every ray reads by value and a pointer to the rest.  timed: the launch's time is asked for */
static int upload_view(DeviceScene *d, const RenderView &rv, bool timed, hipStream_t stream, RenderHot *hot, std::string *err) {
    ORT_HIP(hipMemcpyAsync(d->rv_dev.p, &rv, sizeof(RenderView), hipMemcpyHostToDevice, stream));
    *hot = render_hot<RenderHot>(rv, d->rv_dev.p);
    if (timed) ORT_HIP(hipEventRecord(d->ev0, stream));
    return ORT_OK;
}
/* after the last kernel: what the launches said, and the end of the time */
static int end_kernels(DeviceScene *d, bool timed, hipStream_t stream, std::string *err) {
    ORT_HIP(hipGetLastError());
    if (timed) ORT_HIP(hipEventRecord(d->ev1, stream));
    return ORT_OK;
}
/* after everything the call enqueues on the scene's buffers: the next call on the scene settles this one (settle_inflight) */
static int mark_inflight(DeviceScene *d, hipStream_t stream, std::string *err) {
    ORT_HIP(hipEventRecord(d->ev_done, stream));
    d->inflight = true;
    return ORT_OK;
}
/* A frame-sized plane of a render call as the lanes see it (dev): the caller's device pointer, or in the host form one of the
   scene's staging buffers holding the caller's words -- staged whole, both ways.  A plane that is not asked for stays null */
struct Plane { void *caller; DevBuf *stage; size_t bytes; void *dev; };
static int stage_planes_in(Plane *planes, size_t n, bool host, hipStream_t stream, std::string *err) {
    for (Plane *pn = planes; pn != planes + n; ++pn) {
        pn->dev = pn->caller;
        if (!host || !pn->caller) continue;
        if (int rc = pn->stage->ensure(pn->bytes, err)) return rc;
        pn->dev = pn->stage->p;
        ORT_HIP(hipMemcpyAsync(pn->dev, pn->caller, pn->bytes, hipMemcpyHostToDevice, stream));
    }
    return ORT_OK;
}
static int stage_planes_out(const Plane *planes, size_t n, bool host, hipStream_t stream, std::string *err) {
    for (const Plane *pn = planes; host && pn != planes + n; ++pn)
        if (pn->caller) ORT_HIP(hipMemcpyAsync(pn->caller, pn->dev, pn->bytes, hipMemcpyDeviceToHost, stream));
    return ORT_OK;
}
/* the camera table of a batch of views, packed and on its way to d->view_tab.  Both copies of it are the previous call's until
   that has finished (the caller has settled it); the caller's array is read here and not again */
static int upload_view_table(DeviceScene *d, const ort_view *views, uint32_t n, hipStream_t stream, std::string *err) {
    std::vector<float> &tab = d->view_tab_host;
    pack_view_table(views, n, tab);
    if (int rc = d->view_tab.ensure(tab.size() * sizeof(float), err)) return rc;
    ORT_HIP(hipMemcpyAsync(d->view_tab.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, stream));
    return ORT_OK;
}

/* a settled, timed launch's time and counters, added to stats (paths: its kernels count paths) */
static int add_launch_stats(const DeviceScene *d, bool counters, bool paths, ort_stats *stats, std::string *err) {
    float ms = 0;
    ORT_HIP(hipEventElapsedTime(&ms, d->ev0, d->ev1));
    unsigned long long c[6];
    ORT_HIP(hipMemcpy(c, d->ctrl() + 1, sizeof(c), hipMemcpyDeviceToHost));
    stats->kernel_ms += ms;
    stats->fallback_rays += c[5]; /* counted by every kernel flavour (straight to memory, rare) */
    if (counters) { stats->rays += c[1]; stats->node_tests += c[2]; stats->tri_tests += c[3]; stats->analytic_tests += c[4]; }
    if (counters && paths) stats->paths += c[0];
    return ORT_OK;
}

/* the scene as every kernel sees it (camera and diagnostics are the render's to add); re-reads the knobs under ORT_KNOBS_LIVE */
static SceneView scene_view(Scene *scene, DeviceScene *d) {
    SceneView sv{};
    sv.nodes = d->nodes.as<const float4>(); sv.tris = d->tris.as<const float4>();
    sv.spheres = d->spheres.as<const float4>(); sv.boxes = d->boxes.as<const float4>(); sv.cyls = d->cyls.as<const float4>();
    sv.prim_info = d->prim_info.as<const PrimInfo>();
    sv.info_box = d->info_box; sv.info_cyl = d->info_cyl; sv.info_sphere = d->info_sphere;
    sv.materials = d->materials.as<const float4>();
    sv.light_is_sphere = d->light_is_sphere.as<const uint32_t>();
    sv.tab_src = d->tab.as<const float4>();
    sv.tab_flags = d->tab_flags;
    sv.light_count = d->light_count;
    sv.pro_boxes = scene->tree.pro_boxes;
    sv.pro_spheres = scene->tree.pro_spheres;
    sv.pro_cyls = scene->tree.pro_cyls;
    sv.chain_boxes = d->chain_boxes.as<const float4>();
    if (getenv("ORT_KNOBS_LIVE")) { const int keep = d->knobs.blocks_per_cu; d->knobs = read_knobs(); d->knobs.blocks_per_cu = keep; }
    sv.force_fallback_mask = d->knobs.force_fallback_mask;
    sv.cold = (const ORT_CONSTANT_AS SceneCold *)d->cold.p;
    return sv;
}

static size_t fast_tree_bytes(const Scene *scene) { return scene->tree.nodes.size() * sizeof(DevNode) + scene->tree.tris.size() * sizeof(DevTri); }

/* what the launch policy may know about the uploaded scene */
static SceneTraits scene_traits(const Scene *scene, const DeviceScene *d) {
    SceneTraits t;
    t.diffuse_only = d->diffuse_only;
    t.tab_flags = d->tab_flags;
    t.fast_tree_bytes = fast_tree_bytes(scene);
    t.sah_cost = scene->tree.sah_cost;
    t.has_wide = d->nodes4.p != nullptr;
    t.cu_count = d->cu_count;
    t.max_blocks = d->max_blocks;
    return t;
}

/* ---- developer diagnostics of a finished render (stderr; tools/util_run.py and the tuning logs read these lines) ---- */
static int print_fallback_diag(const DeviceScene *d, const LaunchPlan &pl, std::string *err) {
    unsigned long long fb[2], dg[3];
    ORT_HIP(hipMemcpy(fb, d->ctrl() + 6, sizeof(fb), hipMemcpyDeviceToHost));
    ORT_HIP(hipMemcpy(dg, d->ctrl() + 6 + kDiagFallback, sizeof(dg), hipMemcpyDeviceToHost));
    fprintf(stderr, "fallback: %llu rays traversed again without their first winner, %llu re-cast exactly (%llu octree nodes enqueued, %llu busy queues met)\n",
            dg[1], fb[0], dg[0], dg[2]);
    fprintf(stderr, "issue order: %s\n", pl.block_major ? "block-major" : "chunk-major");
    return ORT_OK;
}

/* how the launch drains */
static int print_drain_diag(const DeviceScene *d, const LaunchPlan &pl, std::string *err) {
    std::vector<unsigned long long> t((size_t)pl.grid * (kBlock / 64));
    ORT_HIP(hipMemcpy(t.data(), d->drain.p, t.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    unsigned long long last = 0;
    for (unsigned long long v : t) last = v > last ? v : last;
    const double tick_ms = 1e-5; /* s_memrealtime: 100 MHz */
    const double marks[] = {0.25, 0.5, 1, 2, 3, 5, 8, 12, 20};
    fprintf(stderr, "drain: of %zu waves, still running before the end of the launch:", t.size());
    for (double m : marks) {
        size_t n = 0;
        for (unsigned long long v : t) n += (double)(last - v) * tick_ms < m ? 1 : 0;
        fprintf(stderr, "  %g ms: %zu", m, n);
    }
    fprintf(stderr, "\n");
    return ORT_OK;
}

static int print_util_diag(const DeviceScene *d, std::string *err) {
    static const char *names[8] = {"node visit", "leaf visit", "traverse outer iteration", "shade call", "  of which lanes with a finished ray",
                                   "produce_ray pass", "  bounce draw", "  sin/cos + ray setup"};
    unsigned long long u[16];
    ORT_HIP(hipMemcpy(u, d->ctrl() + 8, sizeof(u), hipMemcpyDeviceToHost));
    for (int k = 0; k < 8; ++k)
        fprintf(stderr, "util %-40s wave-events %14llu  mean active lanes %6.2f\n", names[k], u[2 * k],
                u[2 * k] ? (double)u[2 * k + 1] / (double)u[2 * k] : 0.0);
    static const char *pnames[10] = {"resolve_hit (chain check)", "hit processing + bounce draw", "pixel / job / new sample", "sin/cos + normalise + ray setup",
                                    "1/d + analytic prologue", "descend loop", "leaf", "pt_lane loop top (after traverse)",
                                    "produce_ray entry (after resolve)", "traverse loop top"};
    unsigned long long ph[30];
    ORT_HIP(hipMemcpy(ph, d->ctrl() + 8 + 32, sizeof(ph), hipMemcpyDeviceToHost));
    double total = 0;
    for (int k = 0; k < 10; ++k) total += (double)ph[3 * k];
    for (int k = 0; k < 10; ++k)
        fprintf(stderr, "phase %-36s share %5.1f %%  cycles/mark %8.1f  marks %12llu  lanes at mark %5.1f\n", pnames[k],
                total > 0 ? 100.0 * (double)ph[3 * k] / total : 0.0, ph[3 * k + 1] ? (double)ph[3 * k] / (double)ph[3 * k + 1] : 0.0,
                ph[3 * k + 1], ph[3 * k + 1] ? (double)ph[3 * k + 2] / (double)ph[3 * k + 1] : 0.0);
    return ORT_OK;
}

/* The camera render call, of the kind the caller states (c.kind): plain, adaptive (c.ad), split by light group (c.groups), cut
   by the caller's map (c.sample_map), continued from the caller's planes (c.acc_sum, with or without a map) or split by path
   depth (c.depth_bins).  What runs, on
   which grid and with which thresholds is plan_render's or, for a pixel-job kind, plan_pixel_jobs' decision (ort_plan.h), and
   what the RenderView says besides pointers is render_view's (ort_setup.h); this is the plumbing around them: settle the previous call, plan, staging, views, buffers, launch, combine, finish */
int device_render(Scene *scene, const ort_render_params *p, const RenderCall &c, void *out_rgb, void *out_spp, void *out_m2, void *states, std::string *err) {
    DeviceScene *d = scene->dev;
    if (!d) { *err = "scene is not uploaded to a device (ort_scene_upload)"; return ORT_ERR_NO_DEVICE; }
    ORT_HIP(hipSetDevice(d->device));
    hipStream_t stream = (hipStream_t)c.stream;
    const uint32_t view_count = c.views ? c.view_count : 1u;
    int rc;
    /* One render at a time per scene: the job counter, the work counters, the partial planes and the stashes belong
       to the scene.  A render that was returned from without waiting is waited for here, and its tripwire checked. */
    if ((rc = settle_inflight(d, err))) return rc;

    SceneView sv = scene_view(scene, d);
    const SceneTraits traits = scene_traits(scene, d);
    const LaunchPlan pl = c.kind != RK_PLAIN ? plan_pixel_jobs(c.kind, traits, *p, d->knobs, view_count)
                                             : plan_render(traits, *p, c.jobs != nullptr, c.job_count, /* w5_layout_ok */ true, d->knobs, view_count);
    sv.util = pl.util ? d->ctrl() + 8 : nullptr;
    if (pl.wide) sv.nodes = d->nodes4.as<const float4>();
    /* the camera: the scene's own; a batch of one view is the same call with that view's camera and seed; the lanes of a larger
       batch read theirs from the table (the VIEWS kernels: sv.cam stays the scene's, unread) */
    ort_camera cam;
    camera_basis(*scene, p->width, p->height, &cam);
    if (c.views && !pl.views) cam = c.views[0].camera;
    memcpy(sv.cam, &cam, sizeof(cam));

    RenderView rv{};
    render_view(*p, pl, c.views, c.ad, &rv);
    /* the planes as the lanes see them: the caller's device pointers, or the scene's staging buffers holding the caller's words.
       view_count frames, view-major, or the packed framebuffer; the 4-byte planes stage where the radiance queries' do */
    const size_t pixels = (size_t)view_count * (size_t)p->width * (size_t)p->height;
    const size_t bins = c.depth_bins ? c.depth_bins : 1u; /* the path-depth render's length planes: a plane per bin where the others have one */
    Plane planes[7] = {{out_rgb, &d->staging, rv.packed_out ? (size_t)rv.my_blocks * 768u : pixels * 12u, nullptr}, {out_spp, &d->query_stage[3], pixels * 4u * bins, nullptr},
                       {out_m2, &d->query_stage[4], pixels * 4u, nullptr}, {states, &d->query_stage[5], pixels * 4u, nullptr},
                       {c.out_groups, &d->query_stage[0], pixels * 12u * (c.groups ? c.groups->group_count : c.depth_bins), nullptr},
                       /* the one plane that is read and not written: staged in with the others, never out */
                       {const_cast<void *>(c.sample_map), &d->query_stage[1], pixels * 4u, nullptr},
                       /* the accumulating render's colour sums, staged both ways as its count (out_spp), m2 and states are */
                       {c.acc_sum, &d->query_stage[2], pixels * 12u, nullptr}};
    if ((rc = stage_planes_in(planes, 7, c.host, stream, err))) return rc;
    rv.out = (float *)planes[0].dev;
    rv.ad_spp = (uint32_t *)planes[1].dev;
    rv.ad_m2 = (float *)planes[2].dev;
    rv.final_states = (uint32_t *)planes[3].dev;
    rv.sample_map = (const uint32_t *)planes[5].dev;
    rv.acc_sum = (float *)planes[6].dev;
    if (c.groups) { /* the group table, the scene's copy of it on its way to the device; the previous call was settled above */
        d->group_tab_host.assign(c.groups->group_of_material, c.groups->group_of_material + c.groups->material_count);
        if ((rc = d->group_tab.ensure(d->group_tab_host.size(), err))) return rc;
        ORT_HIP(hipMemcpyAsync(d->group_tab.p, d->group_tab_host.data(), d->group_tab_host.size(), hipMemcpyHostToDevice, stream));
        rv.group_of_material = d->group_tab.as<const uint8_t>();
        rv.group_count = c.groups->group_count;
        rv.group_out = (float *)planes[4].dev;
    }
    if (c.depth_bins) { /* the bin frames where the group frames travel, the length planes where the sample counts do */
        rv.depth_bins = c.depth_bins;
        rv.depth_out = (float *)planes[4].dev;
        rv.depth_len = (uint32_t *)planes[1].dev;
    }
    if (c.jobs) {
        if ((rc = d->jobs.ensure((size_t)c.job_count * sizeof(ort_tile_job), err))) return rc;
        /* synchronous: the caller's job list may be gone when this call returns */
        ORT_HIP(hipStreamSynchronize(stream));
        ORT_HIP(hipMemcpy(d->jobs.p, c.jobs, (size_t)c.job_count * sizeof(ort_tile_job), hipMemcpyHostToDevice));
        rv.jobs = d->jobs.as<const ort_tile_job>();
        if (c.job_states) {
            if ((rc = d->states.ensure((size_t)c.job_count * 4u, err))) return rc;
            rv.final_states = d->states.as<uint32_t>();
        }
    }
    if (pl.views) { /* the camera table; the previous call was settled above */
        if ((rc = upload_view_table(d, c.views, view_count, stream, err))) return rc;
        rv.views = d->view_tab.as<const float4>();
    }
    if (pl.mode == PLAN_JOBS_CHUNK) {
        if ((rc = d->partial.ensure(pl.partial_bytes, err))) return rc;
        rv.partial = d->partial.as<float>();
    }
    if (pl.exchange) {
        if ((rc = d->stash.ensure(pl.stash_bytes, err))) return rc;
        rv.stash = d->stash.as<float4>();
    }
    if ((rc = reset_ctrl(d, &rv, stream, err))) return rc;
    if (pl.drain_bytes && c.stats) {
        if ((rc = d->drain.ensure(pl.drain_bytes, err))) return rc;
        ORT_HIP(hipMemsetAsync(d->drain.p, 0, pl.drain_bytes, stream));
        rv.drain = d->drain.as<unsigned long long>();
    }
    RenderHot hot;
    if ((rc = upload_view(d, rv, c.stats != nullptr, stream, &hot, err)) || (rc = launch_path_tracer(d, pl, sv, rv, hot, stream, err))) return rc;
    if (rv.mode == JOBS_CHUNK) {
        ORT_HIP(hipGetLastError());
        unsigned long long total = (unsigned long long)rv.my_blocks * 64ull;
        unsigned int cgrid = (unsigned int)((total + 255) / 256);
        if (pl.views) {
            cgrid = (unsigned int)((total * pl.view_count + 255) / 256);
            if (cgrid) hipLaunchKernelGGL(combine_chunks_views, dim3(cgrid), dim3(256), 0, stream, hot);
        } else if (cgrid) hipLaunchKernelGGL(combine_chunks, dim3(cgrid), dim3(256), 0, stream, hot);
    }
    if ((rc = end_kernels(d, c.stats != nullptr, stream, err))) return rc;

    if ((rc = stage_planes_out(planes, 5, c.host, stream, err)) || (rc = stage_planes_out(planes + 6, 1, c.host, stream, err))) return rc;
    if (c.job_states) ORT_HIP(hipMemcpyAsync(c.job_states, d->states.p, (size_t)c.job_count * 4u, hipMemcpyDeviceToHost, stream));
    /* every synchronous form of the call checks the tripwire before it returns (the fire-and-forget device form, stats == NULL,
       cannot without a sync: the next call on the scene does; bench.py asks for stats) */
    if ((rc = mark_inflight(d, stream, err))) return rc;
    if (c.stats || c.host || c.job_states)
        if ((rc = settle_inflight(d, err, "reference-order fallback queue overflowed"))) return rc;
    if (c.stats && d->knobs.debug_fallback && (rc = print_fallback_diag(d, pl, err))) return rc;
    if (c.stats && rv.drain && (rc = print_drain_diag(d, pl, err))) return rc;
    if (c.stats) memset(c.stats, 0, sizeof(*c.stats));
    if (c.stats && (rc = add_launch_stats(d, pl.counters, true, c.stats, err))) return rc;
    if (c.stats && pl.counters && pl.util && (rc = print_util_diag(d, err))) return rc;
    return ORT_OK;
}

/* ---- the ray queries (ort_raycast*, ort_occluded*, ort_ambient_occlusion*, ort_radiance*) -------------------------------------------------------- */
/* What is launched, on which grid and with which thresholds is plan_ray_query's and plan_radiance's decision (ort_plan.h); this
   is the plumbing around them: one launch path (launch_query) and one host-form loop (run_sliced) for the three */
constexpr uint64_t kRaycastSlice = 1ull << 22;  /* rays per launch of the host form of ort_raycast and ort_occluded (2 x 96 MB of staging) */
constexpr uint64_t kRadianceSlice = 1ull << 20; /* ... of ort_radiance and ort_radiance_adaptive: a ray is spp paths; 44 and 52 MB of staging */
constexpr uint64_t kProbeShSlice = 1ull << 18;  /* ... of ort_probe_sh: a point is spp paths and 148 bytes; 39 MB of staging */
/* tests/test_gpu_slice_boundary.py mirrors both: it runs every query over one slice and a ragged remainder */

/* the inverse of the tree's slot maps, in PrimInfo order (triangles | boxes | cylinders | spheres): slot -> kind << 28 |
   the shape's index in the scene's own arrays.  Built and uploaded at the first query, so that render-only users pay nothing */
static int ensure_prim_src(Scene *scene, DeviceScene *d, std::string *err) {
    if (d->prim_src.p) return ORT_OK;
    std::vector<uint32_t> src;
    const bool bijective = invert_prim_slots(scene->tree, d->info_box, d->info_cyl, d->info_sphere, src);
    if (!bijective) { *err = "internal: the tree's slot maps are not a bijection onto its shape arrays"; return ORT_ERR_INTERNAL; }
    return upload_vec(src, &d->prim_src, err);
}

/* the same table with a triangle's word naming its mesh (object_ids_from_prim_src, ort_setup.h): the ids of ORT_MATTE_BY_OBJECT.
   Built from the scene's mesh triangle counts and uploaded at the first matte render that asks for it */
static int ensure_obj_src(Scene *scene, DeviceScene *d, std::string *err) {
    if (d->obj_src.p) return ORT_OK;
    std::vector<uint32_t> src, obj;
    const bool ok = invert_prim_slots(scene->tree, d->info_box, d->info_cyl, d->info_sphere, src) && object_ids_from_prim_src(*scene, src, obj);
    if (!ok) { *err = "internal: the tree's slot maps are not a bijection onto its shape arrays, or a triangle lies beyond the scene's meshes"; return ORT_ERR_INTERNAL; }
    return upload_vec(obj, &d->obj_src, err);
}

/* what raycast_needs_exact reads, and the rays (a device pointer) */
static RaycastIO ray_query_io(Scene *scene, DeviceScene *d, const void *rays) {
    RaycastIO io{};
    io.rays = (const float2 *)rays;
    ort::ray_query_io(*scene, d->scene_lo, d->scene_hi, &io);
    return io;
}

/* One launch of a ray query over count rays.  rv holds what the query's lanes read behind hot.c besides the policy (nothing for
   raycast_rays and occluded_rays, radiance_view for radiance_rays); issue(sv, hot, plan) enqueues the kernel the plan names.
   stats (may be NULL): synchronous, the launch's time and counters added (radiance: the primary rays traced as paths) */
template <typename Plan, typename Issue>
static int launch_planned(Scene *scene, DeviceScene *d, RenderView rv, uint64_t count, Plan plan, bool radiance, hipStream_t stream, ort_stats *stats,
                          std::string *err, Issue issue) {
    int rc;
    if ((rc = settle_inflight(d, err))) return rc;
    const SceneView sv = scene_view(scene, d);
    const QueryPlan pl = plan(scene_traits(scene, d), d->knobs); /* after scene_view: under ORT_KNOBS_LIVE it reads the knobs again */
    const bool counters = pl.counters;
    rv.job_count = count; /* the job space: the ray array, drawn in batches */
    rv.job_batch = pl.job_batch; rv.batch_until = pl.batch_until;
    rv.refill_below = pl.refill_below; rv.descend_below = pl.descend_below;
    RenderHot hot;
    if ((rc = reset_ctrl(d, &rv, stream, err)) || (rc = upload_view(d, rv, stats != nullptr, stream, &hot, err))) return rc;
    issue(sv, hot, pl);
    if ((rc = end_kernels(d, stats != nullptr, stream, err)) || (rc = mark_inflight(d, stream, err))) return rc;
    /* with stats, wait for it and add its time and counters */
    if (stats && ((rc = settle_inflight(d, err)) || (rc = add_launch_stats(d, counters, radiance, stats, err)))) return rc;
    return ORT_OK;
}
/* ... by the plan of the ray queries (plan_ray_query) or the radiance queries (plan_radiance) over count rays.  launch_planned
   takes the plan as a function of the traits and the knobs, to call once the knobs are this call's */
template <typename Issue>
static int launch_query(Scene *scene, DeviceScene *d, const RenderView &rv, uint64_t count, bool radiance, bool counters, hipStream_t stream, ort_stats *stats,
                        std::string *err, Issue issue) {
    return launch_planned(scene, d, rv, count, [&](const SceneTraits &t, const Knobs &kn) { return radiance ? plan_radiance(t, count, counters, kn) : plan_ray_query(t, count, counters); },
                          radiance, stream, stats, err, issue);
}

/* One array of the host form of a query: `bytes` per ray between the caller's memory and a staging buffer of the scene, towards
   the device or (out) back.  host == NULL: an optional array the caller did not pass; it does not travel, and dev() is null */
struct QueryStream {
    void *host;
    DevBuf *stage;
    size_t bytes;
    bool out;
    void *dev() const { return host ? stage->p : nullptr; }
};

/* The host form: bounded slices through the scene's staging buffers, launch(n) over the first n rays staged.  Every ray is
   answered on its own (and on its own random stream), so the slicing cannot change a result */
template <size_t N, typename Launch>
static int run_sliced(DeviceScene *d, uint64_t count, uint64_t slice_cap, const QueryStream (&streams)[N], hipStream_t stream, std::string *err, Launch launch) {
    int rc;
    const uint64_t slice = count < slice_cap ? count : slice_cap;
    for (const QueryStream &s : streams)
        if (s.host && (rc = s.stage->ensure((size_t)slice * s.bytes, err))) return rc;
    for (uint64_t at = 0; at < count; at += slice) {
        const uint64_t n = count - at < slice ? count - at : slice;
        if ((rc = settle_inflight(d, err))) return rc; /* the staging buffers are the previous slice's until it is done */
        for (const QueryStream &s : streams)
            if (s.host && !s.out) ORT_HIP(hipMemcpyAsync(s.stage->p, (const char *)s.host + at * s.bytes, (size_t)n * s.bytes, hipMemcpyHostToDevice, stream));
        if ((rc = launch(n))) return rc;
        for (const QueryStream &s : streams)
            if (s.host && s.out) ORT_HIP(hipMemcpyAsync((char *)s.host + at * s.bytes, s.stage->p, (size_t)n * s.bytes, hipMemcpyDeviceToHost, stream));
        ORT_HIP(hipStreamSynchronize(stream));
    }
    return settle_inflight(d, err);
}

/* what every query call starts with: the scene's device made current, the stats zeroed, and, from the first query of any kind
   on, the box of everything ort_tree.cpp sized the quadric boxes for (shapes and camera: raycast_needs_exact) */
static int begin_query(Scene *scene, ort_stats *stats, DeviceScene **d_out, std::string *err) {
    DeviceScene *d = *d_out = scene->dev;
    if (!d) { *err = "scene is not uploaded to a device (ort_scene_upload)"; return ORT_ERR_NO_DEVICE; }
    ORT_HIP(hipSetDevice(d->device));
    if (!d->scene_box_known) scene_origin_box(*scene, d->scene_lo, d->scene_hi);
    d->scene_box_known = true;
    if (stats) memset(stats, 0, sizeof(*stats));
    return ORT_OK;
}

/* One array of a query call: `bytes` per ray, read by the kernel or (out) written.  p == NULL: an optional array the caller did
   not pass */
struct QueryArray {
    const void *p;
    size_t bytes;
    bool out;
};

/* A query over its arrays, launch(p, n) running the first n rays at the device pointers p[i].  The device form: the caller's
   pointers, one launch.  The host form: run_sliced, array i staged through the scene's i-th staging buffer */
template <size_t N, typename Launch>
static int run_query(DeviceScene *d, const QueryCall &q, uint64_t slice_cap, const QueryArray (&arrays)[N], std::string *err, Launch launch) {
    static_assert(N <= sizeof(d->query_stage) / sizeof(d->query_stage[0]), "one staging buffer per array");
    void *p[N];
    if (!q.host) {
        for (size_t i = 0; i < N; ++i) p[i] = (void *)arrays[i].p;
        return launch(p, q.count);
    }
    QueryStream s[N];
    for (size_t i = 0; i < N; ++i) s[i] = QueryStream{(void *)arrays[i].p, &d->query_stage[i], arrays[i].bytes, arrays[i].out};
    return run_sliced(d, q.count, slice_cap, s, (hipStream_t)q.stream, err, [&](uint64_t n) {
        for (size_t i = 0; i < N; ++i) p[i] = s[i].dev();
        return launch(p, n);
    });
}

/* closest hits: count rays -> count hits */
int device_raycast(Scene *scene, const QueryCall &q, const void *rays, void *hits, std::string *err) {
    static_assert(sizeof(ort_hit) == 24, "ort_hit is three 8-byte words");
    DeviceScene *d;
    int rc;
    if ((rc = begin_query(scene, q.stats, &d, err)) || (rc = ensure_prim_src(scene, d, err))) return rc;
    hipStream_t stream = (hipStream_t)q.stream;
    const bool counters = (q.flags & ORT_RENDER_COUNTERS) != 0;
    const QueryArray arrays[] = {{rays, 24u, false}, {hits, sizeof(ort_hit), true}};
    return run_query(d, q, kRaycastSlice, arrays, err, [&](void *const *p, uint64_t n) {
        RaycastIO io = ray_query_io(scene, d, p[0]);
        io.hits = (uint2 *)p[1];
        io.prim_src = d->prim_src.as<const uint32_t>();
        return launch_query(scene, d, RenderView{}, n, false, counters, stream, q.stats, err, [&](const SceneView &sv, const RenderHot &hot, const QueryPlan &pl) {
            with_bools([&](auto C, auto T) {
                hipLaunchKernelGGL((raycast_rays<decltype(C)::value, decltype(T)::value>), dim3(pl.grid), dim3(kBlock), 0, stream, sv, hot, io);
            }, pl.counters, pl.tabs);
        });
    });
}

/* occlusion: the same for count rays and their limits at tmax (may be null) -> count bytes.  No shape table: a byte names no
   shape */
int device_occluded(Scene *scene, const QueryCall &q, const void *rays, const void *tmax, void *out, std::string *err) {
    DeviceScene *d;
    int rc;
    if ((rc = begin_query(scene, q.stats, &d, err))) return rc;
    hipStream_t stream = (hipStream_t)q.stream;
    const bool counters = (q.flags & ORT_RENDER_COUNTERS) != 0;
    const QueryArray arrays[] = {{rays, 24u, false}, {tmax, sizeof(float), false}, {out, 1u, true}};
    return run_query(d, q, kRaycastSlice, arrays, err, [&](void *const *p, uint64_t n) {
        OccludedIO io{};
        io.q = ray_query_io(scene, d, p[0]);
        io.tmax = (const float *)p[1];
        io.out = (uint8_t *)p[2];
        io.mats_nonzero = all_mats_nonzero(scene->tree);
        return launch_query(scene, d, RenderView{}, n, false, counters, stream, q.stats, err, [&](const SceneView &sv, const RenderHot &hot, const QueryPlan &pl) {
            with_bools([&](auto C, auto T) {
                hipLaunchKernelGGL((occluded_rays<decltype(C)::value, decltype(T)::value>), dim3(pl.grid), dim3(kBlock), 0, stream, sv, hot, io);
            }, pl.counters, pl.tabs);
        });
    });
}

/* ambient occlusion: count points with their seeds and radii (may be null) -> an open count each and, where asked for, the bent
   sums and the final states.  The six arrays fill the six staging buffers; a point is spp rays, so the host form's slice is the
   radiance queries'.  plan_ray_query over the points, as it stands: untuned for this job space (a job is spp traversals and
   draws, not one) -- no constant departs from it, so none needs a measurement of its own */
int device_ambient_occlusion(Scene *scene, const QueryCall &q, const void *points, const void *seeds, const void *radius, uint32_t spp, void *out_open,
                             void *out_bent, void *states, std::string *err) {
    DeviceScene *d;
    int rc;
    if ((rc = begin_query(scene, q.stats, &d, err))) return rc;
    hipStream_t stream = (hipStream_t)q.stream;
    const bool counters = (q.flags & ORT_RENDER_COUNTERS) != 0;
    const QueryArray arrays[] = {{points, 24u, false}, {seeds, 4u, false}, {radius, sizeof(float), false}, {out_open, 4u, true}, {out_bent, 12u, true}, {states, 4u, true}};
    return run_query(d, q, kRadianceSlice, arrays, err, [&](void *const *p, uint64_t n) {
        AoIO io{};
        io.q = ray_query_io(scene, d, p[0]);
        io.seeds = (const uint32_t *)p[1];
        io.radius = (const float *)p[2];
        io.open = (uint32_t *)p[3];
        io.bent = (float *)p[4];
        io.states = (uint32_t *)p[5];
        io.spp = spp;
        io.mats_nonzero = all_mats_nonzero(scene->tree);
        return launch_query(scene, d, RenderView{}, n, false, counters, stream, q.stats, err, [&](const SceneView &sv, const RenderHot &hot, const QueryPlan &pl) {
            with_bools([&](auto C, auto T) {
                hipLaunchKernelGGL((ao_points<decltype(C)::value, decltype(T)::value>), dim3(pl.grid), dim3(kBlock), 0, stream, sv, hot, io);
            }, pl.counters, pl.tabs);
        });
    });
}

/* first-hit feature renders: view_count frames of p's rect -> the planes asked for.  The planes are frames, not arrays over the
   jobs, so the host form stages them as device_render stages its own (stage_planes_in / _out) -- plane i through the scene's i-th
   query staging buffer -- and the launch is one; the camera table is device_render's too (upload_view_table).  The
   launch goes through the queries' one path by plan_features (ort_plan.h) */
int device_render_features(Scene *scene, const ort_render_params *p, const ort_view *views, uint32_t view_count, const QueryCall &q,
                           const ort_feature_planes &planes, std::string *err) {
    DeviceScene *d;
    int rc;
    if ((rc = begin_query(scene, q.stats, &d, err)) || (rc = ensure_prim_src(scene, d, err))) return rc;
    hipStream_t stream = (hipStream_t)q.stream;
    /* the staging buffers and both copies of the camera table are the previous call's until that has finished */
    if ((rc = settle_inflight(d, err))) return rc;
    const size_t pixels = (size_t)view_count * (size_t)p->width * (size_t)p->height;
    DevBuf *const st = d->query_stage;
    Plane pn[6] = {{planes.albedo, st, pixels * 12u, nullptr}, {planes.normal, st + 1, pixels * 12u, nullptr}, {planes.depth, st + 2, pixels * 4u, nullptr},
                   {planes.hits, st + 3, pixels * 4u, nullptr}, {planes.ids, st + 4, pixels * 8u, nullptr}, {planes.final_states, st + 5, pixels * 4u, nullptr}};
    static_assert(sizeof(pn) / sizeof(pn[0]) <= sizeof(d->query_stage) / sizeof(d->query_stage[0]), "one staging buffer per plane");
    if ((rc = stage_planes_in(pn, 6, q.host, stream, err)) || (rc = upload_view_table(d, views, view_count, stream, err))) return rc;
    RenderView rv{};
    features_view(*p, view_count, &rv);
    rv.views = d->view_tab.as<const float4>();
    FeatureIO io{};
    io.q = ray_query_io(scene, d, nullptr);
    io.q.prim_src = d->prim_src.as<const uint32_t>();
    io.albedo = (float *)pn[0].dev; io.normal = (float *)pn[1].dev; io.depth = (float *)pn[2].dev;
    io.hits = (uint32_t *)pn[3].dev; io.ids = (uint32_t *)pn[4].dev; io.states = (uint32_t *)pn[5].dev;
    const bool counters = (q.flags & ORT_RENDER_COUNTERS) != 0;
    auto planner = [&](const SceneTraits &t, const Knobs &kn) { return plan_features(t, *p, view_count, counters, kn); };
    rc = launch_planned(scene, d, rv, rv.job_count, planner, false, stream, q.stats, err, [&](const SceneView &sv, const RenderHot &hot, const QueryPlan &plan) {
        with_bools([&](auto C, auto T) {
            hipLaunchKernelGGL((feature_pixels<decltype(C)::value, decltype(T)::value>), dim3(plan.grid), dim3(kBlock), 0, stream, sv, hot, io);
        }, plan.counters, plan.tabs);
    });
    if (rc || (rc = stage_planes_out(pn, 6, q.host, stream, err)) || !q.host) return rc;
    ORT_HIP(hipStreamSynchronize(stream));
    return settle_inflight(d, err);
}

/* feature renders that follow mirrors and glass: device_render_features with the seven planes of ort_render_follow -- the seventh
   stages through the render's frame buffer (d->staging), which no query uses --, follow_view's rr, the cap in the kernels' third
   argument and plan_follow's plan */
int device_render_follow(Scene *scene, const ort_render_params *p, const ort_view *views, uint32_t view_count, uint32_t max_bounces, const QueryCall &q,
                         const ort_follow_planes &planes, std::string *err) {
    DeviceScene *d;
    int rc;
    if ((rc = begin_query(scene, q.stats, &d, err)) || (rc = ensure_prim_src(scene, d, err))) return rc;
    hipStream_t stream = (hipStream_t)q.stream;
    /* the staging buffers and both copies of the camera table are the previous call's until that has finished */
    if ((rc = settle_inflight(d, err))) return rc;
    const size_t pixels = (size_t)view_count * (size_t)p->width * (size_t)p->height;
    DevBuf *const st = d->query_stage;
    Plane pn[7] = {{planes.albedo, st, pixels * 12u, nullptr}, {planes.normal, st + 1, pixels * 12u, nullptr}, {planes.depth, st + 2, pixels * 4u, nullptr},
                   {planes.hits, st + 3, pixels * 4u, nullptr}, {planes.ids, st + 4, pixels * 8u, nullptr}, {planes.final_states, st + 5, pixels * 4u, nullptr},
                   {planes.bounces, &d->staging, pixels * 4u, nullptr}};
    static_assert(sizeof(pn) / sizeof(pn[0]) <= sizeof(d->query_stage) / sizeof(d->query_stage[0]) + 1, "one staging buffer per plane");
    if ((rc = stage_planes_in(pn, 7, q.host, stream, err)) || (rc = upload_view_table(d, views, view_count, stream, err))) return rc;
    RenderView rv{};
    follow_view(*p, view_count, &rv);
    rv.views = d->view_tab.as<const float4>();
    FollowIO io{};
    io.q = ray_query_io(scene, d, nullptr);
    io.q.prim_src = d->prim_src.as<const uint32_t>();
    io.albedo = (float *)pn[0].dev; io.normal = (float *)pn[1].dev; io.depth = (float *)pn[2].dev;
    io.hits = (uint32_t *)pn[3].dev; io.ids = (uint32_t *)pn[4].dev; io.states = (uint32_t *)pn[5].dev; io.bounces = (uint32_t *)pn[6].dev;
    io.max_bounces = max_bounces;
    const bool counters = (q.flags & ORT_RENDER_COUNTERS) != 0;
    auto planner = [&](const SceneTraits &t, const Knobs &kn) { return plan_follow(t, *p, view_count, counters, kn); };
    rc = launch_planned(scene, d, rv, rv.job_count, planner, false, stream, q.stats, err, [&](const SceneView &sv, const RenderHot &hot, const QueryPlan &plan) {
        with_bools([&](auto C, auto T) {
            hipLaunchKernelGGL((follow_pixels<decltype(C)::value, decltype(T)::value>), dim3(plan.grid), dim3(kBlock), 0, stream, sv, hot, io);
        }, plan.counters, plan.tabs);
    });
    if (rc || (rc = stage_planes_out(pn, 7, q.host, stream, err)) || !q.host) return rc;
    ORT_HIP(hipStreamSynchronize(stream));
    return settle_inflight(d, err);
}

/* ID-matte renders: device_render_features with the five planes of ort_render_matte -- ids and counts hold m.slots words a pixel
   --, the table the mode names a hit by (the shape table, the object table, none) and plan_matte's plan.  The host form stages
   ids and counts whole both ways like every other plane, so that pixels outside the rect keep what they held */
int device_render_matte(Scene *scene, const ort_render_params *p, const ort_view *views, uint32_t view_count, const ort_matte &m, const QueryCall &q,
                        const ort_matte_planes &planes, std::string *err) {
    DeviceScene *d;
    int rc;
    if ((rc = begin_query(scene, q.stats, &d, err))) return rc;
    if (m.by == ORT_MATTE_BY_PRIM && (rc = ensure_prim_src(scene, d, err))) return rc;
    if (m.by == ORT_MATTE_BY_OBJECT && (rc = ensure_obj_src(scene, d, err))) return rc;
    hipStream_t stream = (hipStream_t)q.stream;
    /* the staging buffers and both copies of the camera table are the previous call's until that has finished */
    if ((rc = settle_inflight(d, err))) return rc;
    const size_t pixels = (size_t)view_count * (size_t)p->width * (size_t)p->height;
    DevBuf *const st = d->query_stage;
    Plane pn[5] = {{planes.ids, st, pixels * 4u * m.slots, nullptr}, {planes.counts, st + 1, pixels * 4u * m.slots, nullptr}, {planes.other, st + 2, pixels * 4u, nullptr},
                   {planes.hits, st + 3, pixels * 4u, nullptr}, {planes.final_states, st + 4, pixels * 4u, nullptr}};
    static_assert(sizeof(pn) / sizeof(pn[0]) <= sizeof(d->query_stage) / sizeof(d->query_stage[0]), "one staging buffer per plane");
    if ((rc = stage_planes_in(pn, 5, q.host, stream, err)) || (rc = upload_view_table(d, views, view_count, stream, err))) return rc;
    RenderView rv{};
    matte_view(*p, view_count, &rv);
    rv.views = d->view_tab.as<const float4>();
    MatteIO io{};
    io.q = ray_query_io(scene, d, nullptr);
    io.q.prim_src = m.by == ORT_MATTE_BY_PRIM ? d->prim_src.as<const uint32_t>() : m.by == ORT_MATTE_BY_OBJECT ? d->obj_src.as<const uint32_t>() : nullptr;
    io.ids = (uint32_t *)pn[0].dev; io.counts = (uint32_t *)pn[1].dev; io.other = (uint32_t *)pn[2].dev;
    io.hits = (uint32_t *)pn[3].dev; io.states = (uint32_t *)pn[4].dev;
    io.by = m.by; io.slots = m.slots;
    const bool counters = (q.flags & ORT_RENDER_COUNTERS) != 0;
    auto planner = [&](const SceneTraits &t, const Knobs &kn) { return plan_matte(t, *p, view_count, counters, kn); };
    rc = launch_planned(scene, d, rv, rv.job_count, planner, false, stream, q.stats, err, [&](const SceneView &sv, const RenderHot &hot, const QueryPlan &plan) {
        with_bools([&](auto C, auto T) {
            hipLaunchKernelGGL((matte_pixels<decltype(C)::value, decltype(T)::value>), dim3(plan.grid), dim3(kBlock), 0, stream, sv, hot, io);
        }, plan.counters, plan.tabs);
    });
    if (rc || (rc = stage_planes_out(pn, 5, q.host, stream, err)) || !q.host) return rc;
    ORT_HIP(hipStreamSynchronize(stream));
    return settle_inflight(d, err);
}

/* radiance: count rays with their seeds -> 3 floats each and, where asked for (states may be null), the final states.  No shape
   table: a colour names no shape.  With ad (checked by the caller) the adaptive query: the stopping rule's parameters where spp
   stands, and, where asked for, every ray's sample count and its sum of squared sample luminance; plan_radiance's plan as it
   is, the kernels ort_kernels_adaptive.hip's.  With points the irradiance queries: the array holds (p, n) where a ray's (o, d)
   stand -- the same bytes, staging and view -- and the kernels, plain or adaptive, are ort_kernels_irradiance.hip's.  With out_sh
   (points then, and no ad) the SH light-probe query: one more array of 27 floats a point, which the view gets as sh_out; out may
   then be null */
int device_radiance(Scene *scene, const QueryCall &q, const void *rays, const void *seeds, uint32_t spp, float rr, const ort_adaptive *ad, void *out,
                    void *out_spp, void *out_m2, void *states, bool points, void *out_sh, std::string *err) {
    DeviceScene *d;
    int rc;
    if ((rc = begin_query(scene, q.stats, &d, err))) return rc;
    hipStream_t stream = (hipStream_t)q.stream;
    const bool counters = (q.flags & ORT_RENDER_COUNTERS) != 0;
    const QueryArray arrays[] = {{rays, 24u, false}, {seeds, 4u, false}, {out, 12u, true}, {out_spp, 4u, true}, {out_m2, 4u, true}, {states, 4u, true}, {out_sh, 108u, true}};
    return run_query(d, q, out_sh ? kProbeShSlice : kRadianceSlice, arrays, err, [&](void *const *p, uint64_t n) {
        RenderView rv{};
        if (ad) radiance_adaptive_view(ray_query_io(scene, d, p[0]), p[1], *ad, rr, p[2], p[3], p[4], p[5], &rv);
        else radiance_view(ray_query_io(scene, d, p[0]), p[1], spp, rr, p[2], p[5], &rv);
        rv.sh_out = (float *)p[6];
        return launch_query(scene, d, rv, n, true, counters, stream, q.stats, err, [&](const SceneView &sv, const RenderHot &hot, const QueryPlan &pl) {
            if (out_sh) ort_launch_probe_sh(pl, stream, sv, hot);
            else if (points) ort_launch_irradiance(pl, ad != nullptr, stream, sv, hot);
            else if (ad) ort_launch_radiance_adaptive(pl, stream, sv, hot);
            else with_bools([&](auto C, auto D, auto T) {
                hipLaunchKernelGGL((radiance_rays<decltype(C)::value, decltype(D)::value, decltype(T)::value>), dim3(pl.grid), dim3(kBlock), 0, stream, sv, hot);
            }, pl.counters, pl.diffuse, pl.tabs);
        });
    });
}

/* ---- the denoiser (ort_denoise.h): a pack, then `iterations` a-trous passes that ping-pong between the workspace's two CV planes.
   No scene: the call names its device.  host: the caller's planes are staged whole, the passes run in place on the staged colour
   and the workspace is this call's own; otherwise every pointer is the device's, nothing is allocated and the passes are enqueued
   on stream (the call waits only for stats).  The arguments are checked by the caller (ort_api.cpp: denoise_common). */
int device_denoise(int device, bool host, const ort_denoise_params &p, const ort_denoise_planes &in, int32_t w, int32_t h, uint32_t frames, void *out_rgb,
                   void *workspace, void *stream_, ort_stats *stats, std::string *err) {
    int count = 0;
    int rc = device_count(&count, err);
    if (rc != ORT_OK) return rc;
    if (device < 0 || device >= count) { *err = "no such HIP device"; return ORT_ERR_NO_DEVICE; }
    ORT_HIP(hipSetDevice(device));
    hipStream_t stream = host ? nullptr : (hipStream_t)stream_;
    const size_t n = (size_t)frames * (size_t)w * (size_t)h;
    DevBuf d_rgb, d_m2, d_count, d_albedo, d_normal, d_depth, d_ws;
    const void *rgb = in.rgb, *m2 = in.m2, *cnt = in.count, *albedo = in.albedo, *normal = in.normal, *depth = in.depth;
    if (host) {
        struct { DevBuf *buf; const void **src; size_t bytes; } stage[] = {{&d_rgb, &rgb, 12 * n},       {&d_m2, &m2, 4 * n},         {&d_count, &cnt, 4 * n},
                                                                           {&d_albedo, &albedo, 12 * n}, {&d_normal, &normal, 12 * n}, {&d_depth, &depth, 4 * n}};
        for (auto &s : stage) {
            if ((rc = s.buf->ensure(s.bytes, err))) return rc;
            ORT_HIP(hipMemcpy(s.buf->p, *s.src, s.bytes, hipMemcpyHostToDevice));
            *s.src = s.buf->p;
        }
        if ((rc = d_ws.ensure(ortdn::kWorkspaceBytesPerPixel * n, err))) return rc;
        workspace = d_ws.p;
    }
    float *d_out = host ? d_rgb.as<float>() : (float *)out_rgb;
    ortdn::F4 *cv[2] = {(ortdn::F4 *)workspace, (ortdn::F4 *)workspace + n};
    ortdn::F4 *gd = (ortdn::F4 *)workspace + 2 * n;
    const ortdn::Params prm{p.iterations, p.normal_squarings, p.sigma_l * p.sigma_l, p.sigma_z * p.sigma_z};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    struct EventGuard { hipEvent_t &a, &b; ~EventGuard() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } guard{ev0, ev1};
    if (stats) {
        ORT_HIP(hipEventCreate(&ev0));
        ORT_HIP(hipEventCreate(&ev1));
        ORT_HIP(hipEventRecord(ev0, stream));
    }
    constexpr uint64_t kMaxGrid = 1u << 20; /* workgroups of one launch; the kernels stride over what is beyond */
    const uint64_t pack_groups = (n + 255u) / 256u;
    hipLaunchKernelGGL(ortdn::denoise_pack, dim3((uint32_t)std::min(pack_groups, kMaxGrid)), dim3(256), 0, stream, (const float *)rgb, (const float *)m2,
                       (const uint32_t *)cnt, (const float *)albedo, (const float *)normal, (const float *)depth, cv[0], gd, (uint32_t)n);
    ORT_HIP(hipGetLastError());
    const uint32_t tiles_x = ((uint32_t)w + ortdn::kTileW - 1u) / ortdn::kTileW, tiles_y = ((uint32_t)h + ortdn::kTileH - 1u) / ortdn::kTileH;
    const uint64_t tiles = (uint64_t)tiles_x * tiles_y * frames;
    const dim3 grid((uint32_t)std::min(tiles, kMaxGrid));
    for (uint32_t j = 0; j < p.iterations; ++j) {
        const int s = 1 << j;
        const ortdn::F4 *src = cv[j & 1u];
        if (j + 1u == p.iterations)
            hipLaunchKernelGGL(ortdn::denoise_atrous<true>, grid, dim3(256), 0, stream, src, gd, (ortdn::F4 *)nullptr, (const float *)rgb, (const float *)albedo, d_out, w, h,
                               tiles_x, tiles_y, tiles, s, prm);
        else
            hipLaunchKernelGGL(ortdn::denoise_atrous<false>, grid, dim3(256), 0, stream, src, gd, cv[(j & 1u) ^ 1u], (const float *)nullptr, (const float *)nullptr,
                               (float *)nullptr, w, h, tiles_x, tiles_y, tiles, s, prm);
        ORT_HIP(hipGetLastError());
    }
    if (stats) {
        ORT_HIP(hipEventRecord(ev1, stream));
        ORT_HIP(hipEventSynchronize(ev1));
        float ms = 0.0f;
        ORT_HIP(hipEventElapsedTime(&ms, ev0, ev1));
        *stats = ort_stats{};
        stats->kernel_ms = ms;
    }
    if (host) ORT_HIP(hipMemcpy(out_rgb, d_out, 12 * n, hipMemcpyDeviceToHost));
    return ORT_OK;
}

/* ---- the sample planner (ort_sampleplan.h): error, want, scale, one after the other on one stream; the device decides whether a
   frame is scaled, so nothing comes back to the host between them.  No scene: the call names its device.  host: the caller's
   planes are staged whole, the map, the totals and the workspace are this call's own and are copied back; otherwise every pointer
   is the device's, nothing is allocated and the kernels are enqueued on stream behind the zeroing of the totals (the call waits
   only for stats).  The arguments are checked by the caller (ort_api.cpp: plan_common). */
int device_plan_samples(int device, bool host, const ort_plan_params &p, const ort_plan_planes &in, int32_t w, int32_t h, uint32_t frames, void *sample_map,
                        void *totals, void *workspace, void *stream_, ort_stats *stats, std::string *err) {
    static_assert(sizeof(ort_plan_totals) == sizeof(ortsp::Totals) && offsetof(ort_plan_totals, worst) == offsetof(ortsp::Totals, worst_bits) &&
                      offsetof(ort_plan_totals, unconverged) == offsetof(ortsp::Totals, unconverged), "ortsp::Totals is ort_plan_totals");
    int count = 0;
    int rc = device_count(&count, err);
    if (rc != ORT_OK) return rc;
    if (device < 0 || device >= count) { *err = "no such HIP device"; return ORT_ERR_NO_DEVICE; }
    ORT_HIP(hipSetDevice(device));
    hipStream_t stream = host ? nullptr : (hipStream_t)stream_;
    const size_t n = (size_t)frames * (size_t)w * (size_t)h;
    const size_t totals_bytes = sizeof(ortsp::Totals) * (size_t)frames;
    DevBuf d_rgb, d_m2, d_count, d_map, d_totals, d_ws;
    const void *rgb = in.rgb, *m2 = in.m2, *cnt = in.count;
    void *d_sample_map = sample_map, *d_tot = totals;
    if (host) {
        struct { DevBuf *buf; const void **src; size_t bytes; } stage[] = {{&d_rgb, &rgb, 12 * n}, {&d_m2, &m2, 4 * n}, {&d_count, &cnt, 4 * n}};
        for (auto &s : stage) {
            if ((rc = s.buf->ensure(s.bytes, err))) return rc;
            ORT_HIP(hipMemcpy(s.buf->p, *s.src, s.bytes, hipMemcpyHostToDevice));
            *s.src = s.buf->p;
        }
        if ((rc = d_map.ensure(4 * n, err)) || (rc = d_totals.ensure(totals_bytes, err)) || (rc = d_ws.ensure(ortsp::kWorkspaceBytesPerPixel * n, err))) return rc;
        d_sample_map = d_map.p;
        d_tot = d_totals.p;
        workspace = d_ws.p;
    }
    const ortsp::Params prm{p.tolerance * p.tolerance, p.floor, p.radius, p.pilot, p.min_add, p.cap, p.rgb_is_sum, p.budget};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    struct EventGuard { hipEvent_t &a, &b; ~EventGuard() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } guard{ev0, ev1};
    if (stats) {
        ORT_HIP(hipEventCreate(&ev0));
        ORT_HIP(hipEventCreate(&ev1));
        ORT_HIP(hipEventRecord(ev0, stream));
    }
    ORT_HIP(hipMemsetAsync(d_tot, 0, totals_bytes, stream));
    /* a workgroup issues its atomics once per frame it touched, and they all meet on the frame's 32 bytes: the grid is the measured
       balance between that queue (about 10 ns a workgroup and total) and the lanes the window's loads want in flight -- at 1080p
       256 .. 4096 workgroups give 0.147, 0.099, 0.087, 0.107, 0.168 ms at radius 1 (profiles/r26_sample_plan.md).  The tiles beyond
       the grid are reached by stride */
    constexpr uint64_t kMaxGrid = 1024;
    const uint32_t tiles_x = ((uint32_t)w + ortsp::kTileW - 1u) / ortsp::kTileW, tiles_y = ((uint32_t)h + ortsp::kTileH - 1u) / ortsp::kTileH;
    const uint64_t tiles = (uint64_t)tiles_x * tiles_y * frames;
    const dim3 grid((uint32_t)std::min(tiles, kMaxGrid));
    float *e_plane = (float *)workspace;
    ortsp::Totals *tot = (ortsp::Totals *)d_tot;
    hipLaunchKernelGGL(ortsp::sampleplan_error, grid, dim3(256), 0, stream, (const float *)rgb, (const float *)m2, (const uint32_t *)cnt, e_plane, tot, w, h, tiles_x,
                       tiles_y, tiles, prm);
    ORT_HIP(hipGetLastError());
    /* the window from an LDS tile with halo wherever there is a window; ORT_PLAN_TILE=0 / 1 (a developer knob, read at every call)
       forces the direct loads / the tile at every radius.  The map is the same either way */
    const char *knob = getenv("ORT_PLAN_TILE");
    const bool tile = knob && (knob[0] == '0' || knob[0] == '1') ? knob[0] == '1' : p.radius >= 1;
    hipLaunchKernelGGL(tile ? ortsp::sampleplan_want<true> : ortsp::sampleplan_want<false>, grid, dim3(256), 0, stream, (const float *)e_plane, (const uint32_t *)cnt,
                       (uint32_t *)d_sample_map, tot, w, h, tiles_x, tiles_y, tiles, prm);
    ORT_HIP(hipGetLastError());
    hipLaunchKernelGGL(ortsp::sampleplan_scale, grid, dim3(256), 0, stream, (uint32_t *)d_sample_map, tot, w, h, tiles_x, tiles_y, tiles, prm);
    ORT_HIP(hipGetLastError());
    if (stats) {
        ORT_HIP(hipEventRecord(ev1, stream));
        ORT_HIP(hipEventSynchronize(ev1));
        float ms = 0.0f;
        ORT_HIP(hipEventElapsedTime(&ms, ev0, ev1));
        *stats = ort_stats{};
        stats->kernel_ms = ms;
    }
    if (host) {
        ORT_HIP(hipMemcpy(sample_map, d_sample_map, 4 * n, hipMemcpyDeviceToHost));
        ORT_HIP(hipMemcpy(totals, d_tot, totals_bytes, hipMemcpyDeviceToHost));
    }
    return ORT_OK;
}

/* ---- a mask from matte slots (ort_mattemask.h): one kernel, one lane a pixel by grid stride.  No scene: the call names its device.
   The selection is sorted and freed of duplicates here and travels in the launch's arguments, so the device form allocates
   nothing and has read the caller's select when it returns; it does not wait.  host: ids, counts and the mask are staged whole
   through buffers of this call's own.  The arguments are checked by the caller (ort_api.cpp: matte_mask_common). */
int device_matte_mask(int device, bool host, const void *ids, const void *counts, uint32_t slots, uint32_t spp, const uint32_t *select, uint32_t select_count,
                      int32_t w, int32_t h, uint32_t frames, void *out_mask, void *stream_, std::string *err) {
    int count = 0;
    int rc = device_count(&count, err);
    if (rc != ORT_OK) return rc;
    if (device < 0 || device >= count) { *err = "no such HIP device"; return ORT_ERR_NO_DEVICE; }
    ORT_HIP(hipSetDevice(device));
    hipStream_t stream = host ? nullptr : (hipStream_t)stream_;
    const size_t n = (size_t)frames * (size_t)w * (size_t)h;
    DevBuf d_ids, d_counts, d_mask;
    if (host) {
        if ((rc = d_ids.ensure(4 * n * slots, err)) || (rc = d_counts.ensure(4 * n * slots, err)) || (rc = d_mask.ensure(4 * n, err))) return rc;
        ORT_HIP(hipMemcpy(d_ids.p, ids, 4 * n * slots, hipMemcpyHostToDevice));
        ORT_HIP(hipMemcpy(d_counts.p, counts, 4 * n * slots, hipMemcpyHostToDevice));
        ids = d_ids.p; counts = d_counts.p;
    }
    float *d_out = host ? d_mask.as<float>() : (float *)out_mask;
    ortmm::Select sel;
    ortmm::prepare_select(select, select_count, &sel);
    constexpr uint64_t kMaxGrid = 1u << 16; /* workgroups of one launch; the kernel strides over what is beyond */
    const uint64_t groups = (n + 255u) / 256u;
    hipLaunchKernelGGL(ortmm::matte_mask, dim3((uint32_t)std::min(groups, kMaxGrid)), dim3(256), 0, stream, (const uint32_t *)ids, (const uint32_t *)counts, d_out, slots,
                       (float)spp, (uint32_t)n, sel);
    ORT_HIP(hipGetLastError());
    if (host) ORT_HIP(hipMemcpy(out_mask, d_out, 4 * n, hipMemcpyDeviceToHost));
    return ORT_OK;
}

} // namespace ort

#endif /* !ORT_HOST_SIM */
