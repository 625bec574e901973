/*
 * ort_kernels_adaptive.hip -- the kernels of the adaptive radiance queries (ort_radiance_adaptive): radiance_adaptive_rays.
 *
 * The lane code (ort_lane.h) compiled a third time, at the limits of ort_kernels.hip proper (four waves per SIMD, 24 LDS stack
 * entries), for the eight variants of radiance_lane<..., ADAPT = true> only.  A unit of its own because eight more path-trace
 * kernels are a quarter more compile time: here they compile beside the others (under make -j3 the three units build at once)
 * and the library builds no slower than before them (profiles/r10_adaptive.md).  device_radiance_adaptive (ort_kernels.hip)
 * launches them through ort_launch_radiance_adaptive.
 */
#define ORT_ADAPTIVE_TU 1
#include "ort_lane.h"

/* The argument structs are the same declarations compiled in this unit's namespace: passed as bytes, and the caller checks the
   sizes (the RenderView's too: the lanes read it behind hot.c) */
void ort_launch_radiance_adaptive(int counters, int diffuse, int tabs, unsigned int grid, void *stream, const void *sv_bytes, const void *hot_bytes) {
    using namespace ort_ad;
    SceneView sv;
    RenderHot hot;
    memcpy(&sv, sv_bytes, sizeof(sv));
    memcpy(&hot, hot_bytes, sizeof(hot));
#define ORT_RA(C, D, T)                                                                                                          \
    if ((counters != 0) == C && (diffuse != 0) == D && (tabs != 0) == T) {                                                       \
        hipLaunchKernelGGL((radiance_adaptive_rays<C, D, T>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, sv, hot);      \
        return;                                                                                                                  \
    }
    ORT_RA(true, true, true) ORT_RA(true, true, false) ORT_RA(true, false, true) ORT_RA(true, false, false)
    ORT_RA(false, true, true) ORT_RA(false, true, false) ORT_RA(false, false, true) ORT_RA(false, false, false)
#undef ORT_RA
}
size_t ort_adaptive_sizeof_scene_view() { return sizeof(ort_ad::SceneView); }
size_t ort_adaptive_sizeof_render_hot() { return sizeof(ort_ad::RenderHot); }
size_t ort_adaptive_sizeof_render_view() { return sizeof(ort_ad::RenderView); }
