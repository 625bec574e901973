/*
 * ort_kernels_irradiance.hip -- the kernels of the irradiance queries (ort_irradiance, ort_irradiance_adaptive):
 * irradiance_points and irradiance_adaptive_points; and of the SH light-probe query (ort_probe_sh): probe_sh_points.
 *
 * The lane code (ort_lane.h) compiled a fifth time, at the limits of ort_kernels.hip proper (four waves per SIMD, 24 LDS stack
 * entries), for the sixteen variants of radiance_lane with LF_HEMI only: the radiance queries' loop over points, every
 * sample's primary direction drawn in the lane (produce_ray's HEMI).  A unit of its own for ort_kernels_adaptive.hip's
 * reason: sixteen more path-trace kernels compile here beside the others (under make -j5 the five units build at once).
 * device_radiance (ort_kernels.hip), given points, launches them through ort_launch_irradiance.
 * The SH light-probe query's eight (LF_HEMI | LF_SH: the same loop, the direction drawn over the whole sphere, nine SH sums per
 * point) make it twenty-four; device_radiance, given an SH array, launches them through ort_launch_probe_sh.
 */
#define ORT_NS ort_ir /* the limits: ort_lane.h's defaults */
#include "ort_lane.h"

/* adaptive: with the stopping rule (irradiance_adaptive_points).  The caller's own SceneView and RenderHot: the argument structs
   are ort_lane.h's one definition */
void ort_launch_irradiance(const ort::QueryPlan &pl, bool adaptive, hipStream_t stream, const ort::SceneView &sv, const ort::RenderHot &hot) {
    using namespace ort_ir;
    ort::with_bools([&](auto C, auto D, auto T) {
        if (adaptive)
            hipLaunchKernelGGL((irradiance_adaptive_points<decltype(C)::value, decltype(D)::value, decltype(T)::value>), dim3(pl.grid), dim3(kBlock), 0, stream, sv, hot);
        else
            hipLaunchKernelGGL((irradiance_points<decltype(C)::value, decltype(D)::value, decltype(T)::value>), dim3(pl.grid), dim3(kBlock), 0, stream, sv, hot);
    }, pl.counters, pl.diffuse, pl.tabs);
}

/* the SH light-probe query's kernels (probe_sh_points), likewise */
void ort_launch_probe_sh(const ort::QueryPlan &pl, hipStream_t stream, const ort::SceneView &sv, const ort::RenderHot &hot) {
    using namespace ort_ir;
    ort::with_bools([&](auto C, auto D, auto T) {
        hipLaunchKernelGGL((probe_sh_points<decltype(C)::value, decltype(D)::value, decltype(T)::value>), dim3(pl.grid), dim3(kBlock), 0, stream, sv, hot);
    }, pl.counters, pl.diffuse, pl.tabs);
}
