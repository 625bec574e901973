/*
 * ort_kernels_render_adaptive.hip -- the kernels of the adaptive camera render (ort_render_adaptive, ort_render_views_adaptive):
 * pt_adaptive.
 *
 * The lane code (ort_lane.h) compiled a fourth time, at the limits of ort_kernels.hip proper (four waves per SIMD, 24 LDS stack
 * entries), for the eight variants of pt_lane<..., VIEWS = true, ADAPT = true> only.  A unit of its own for the reason
 * ort_kernels_adaptive.hip is one: eight more path-trace kernels are compile time that ort_kernels.hip, the unit that sets the
 * build's wall time, should not carry; here they compile beside the others (under make -j4 the four units build at once;
 * profiles/r12_render_adaptive.md).  device_render_adaptive (ort_kernels.hip) launches them through ort_launch_render_adaptive.
 */
#define ORT_RENDER_ADAPTIVE_TU 1
#include "ort_lane.h"

/* The argument structs are the same declarations compiled in this unit's namespace: passed as bytes, and the caller checks the
   sizes (the RenderView's too: the lanes read it behind hot.c) */
void ort_launch_render_adaptive(int counters, int diffuse, int tabs, unsigned int grid, void *stream, const void *sv_bytes, const void *hot_bytes) {
    using namespace ort_ra;
    SceneView sv;
    RenderHot hot;
    memcpy(&sv, sv_bytes, sizeof(sv));
    memcpy(&hot, hot_bytes, sizeof(hot));
#define ORT_PA(C, D, T)                                                                                                          \
    if ((counters != 0) == C && (diffuse != 0) == D && (tabs != 0) == T) {                                                       \
        hipLaunchKernelGGL((pt_adaptive<C, D, T>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, sv, hot);                  \
        return;                                                                                                                  \
    }
    ORT_PA(true, true, true) ORT_PA(true, true, false) ORT_PA(true, false, true) ORT_PA(true, false, false)
    ORT_PA(false, true, true) ORT_PA(false, true, false) ORT_PA(false, false, true) ORT_PA(false, false, false)
#undef ORT_PA
}
size_t ort_render_adaptive_sizeof_scene_view() { return sizeof(ort_ra::SceneView); }
size_t ort_render_adaptive_sizeof_render_hot() { return sizeof(ort_ra::RenderHot); }
size_t ort_render_adaptive_sizeof_render_view() { return sizeof(ort_ra::RenderView); }
