/*
 * ort_kernels_render_adaptive.hip -- the kernels of the adaptive camera render (ort_render_adaptive, ort_render_views_adaptive):
 * pt_adaptive.
 *
 * The lane code (ort_lane.h) compiled a fourth time, at the limits of ort_kernels.hip proper (four waves per SIMD, 24 LDS stack
 * entries), for the eight variants of pt_lane<..., VIEWS = true, ADAPT = true> only.  A unit of its own for the reason
 * ort_kernels_adaptive.hip is one: eight more path-trace kernels are compile time that ort_kernels.hip, the unit that sets the
 * build's wall time, should not carry; here they compile beside the others (under make -j4 the four units build at once;
 * profiles/r12_render_adaptive.md).  device_render (ort_kernels.hip), given a stopping rule, launches them through
 * ort_launch_render_adaptive.
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
    ort::with_bools([&](auto C, auto D, auto T) {
        hipLaunchKernelGGL((pt_adaptive<decltype(C)::value, decltype(D)::value, decltype(T)::value>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, sv, hot);
    }, counters != 0, diffuse != 0, tabs != 0);
}
void ort_render_adaptive_layout(size_t sizes[3]) { sizes[0] = sizeof(ort_ra::SceneView); sizes[1] = sizeof(ort_ra::RenderHot); sizes[2] = sizeof(ort_ra::RenderView); }
