/*
 * ort_kernels_adaptive.hip -- the kernels of the adaptive radiance queries (ort_radiance_adaptive): radiance_adaptive_rays.
 *
 * The lane code (ort_lane.h) compiled a third time, at the limits of ort_kernels.hip proper (four waves per SIMD, 24 LDS stack
 * entries), for the eight variants of radiance_lane<..., ADAPT = true> only.  A unit of its own because eight more path-trace
 * kernels are a quarter more compile time: here they compile beside the others (under make -j3 the three units build at once)
 * and the library builds no slower than before them (profiles/r10_adaptive.md).  device_radiance (ort_kernels.hip), given
 * a stopping rule, launches them through ort_launch_radiance_adaptive.
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
    ort::with_bools([&](auto C, auto D, auto T) {
        hipLaunchKernelGGL((radiance_adaptive_rays<decltype(C)::value, decltype(D)::value, decltype(T)::value>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, sv, hot);
    }, counters != 0, diffuse != 0, tabs != 0);
}
void ort_adaptive_layout(size_t sizes[3]) { sizes[0] = sizeof(ort_ad::SceneView); sizes[1] = sizeof(ort_ad::RenderHot); sizes[2] = sizeof(ort_ad::RenderView); }
