/*
 * ort_kernels_irradiance.hip -- the kernels of the irradiance queries (ort_irradiance, ort_irradiance_adaptive):
 * irradiance_points and irradiance_adaptive_points.
 *
 * The lane code (ort_lane.h) compiled a fifth time, at the limits of ort_kernels.hip proper (four waves per SIMD, 24 LDS stack
 * entries), for the sixteen variants of radiance_lane<..., HEMI = true> only: the radiance queries' loop over points, every
 * sample's primary direction drawn in the lane (produce_ray's HEMI flag).  A unit of its own for ort_kernels_adaptive.hip's
 * reason: sixteen more path-trace kernels compile here beside the others (under make -j5 the five units build at once).
 * device_radiance (ort_kernels.hip), given points, launches them through ort_launch_irradiance.
 */
#define ORT_IRRADIANCE_TU 1
#include "ort_lane.h"

/* The argument structs are the same declarations compiled in this unit's namespace: passed as bytes, and the caller checks the
   sizes (the RenderView's too: the lanes read it behind hot.c) */
void ort_launch_irradiance(int adaptive, int counters, int diffuse, int tabs, unsigned int grid, void *stream, const void *sv_bytes, const void *hot_bytes) {
    using namespace ort_ir;
    SceneView sv;
    RenderHot hot;
    memcpy(&sv, sv_bytes, sizeof(sv));
    memcpy(&hot, hot_bytes, sizeof(hot));
    ort::with_bools([&](auto C, auto D, auto T) {
        if (adaptive)
            hipLaunchKernelGGL((irradiance_adaptive_points<decltype(C)::value, decltype(D)::value, decltype(T)::value>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, sv, hot);
        else
            hipLaunchKernelGGL((irradiance_points<decltype(C)::value, decltype(D)::value, decltype(T)::value>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, sv, hot);
    }, counters != 0, diffuse != 0, tabs != 0);
}
void ort_irradiance_layout(size_t sizes[3]) { sizes[0] = sizeof(ort_ir::SceneView); sizes[1] = sizeof(ort_ir::RenderHot); sizes[2] = sizeof(ort_ir::RenderView); }
