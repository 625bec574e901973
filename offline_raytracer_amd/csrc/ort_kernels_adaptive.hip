/*
 * ort_kernels_adaptive.hip -- the kernels of the adaptive radiance queries (ort_radiance_adaptive): radiance_adaptive_rays.
 *
 * The lane code (ort_lane.h) compiled a third time, at the limits of ort_kernels.hip proper (four waves per SIMD, 24 LDS stack
 * entries), for the eight variants of radiance_lane with LF_ADAPT only.  A unit of its own because eight more path-trace
 * kernels are a quarter more compile time: here they compile beside the others (under make -j3 the three units build at once)
 * and the library builds no slower than before them (profiles/r10_adaptive.md).  device_radiance (ort_kernels.hip), given
 * a stopping rule, launches them through ort_launch_radiance_adaptive.
 */
#define ORT_NS ort_ad /* the limits: ort_lane.h's defaults */
#include "ort_lane.h"

/* the caller's own SceneView and RenderHot: the argument structs are ort_lane.h's one definition */
void ort_launch_radiance_adaptive(const ort::QueryPlan &pl, hipStream_t stream, const ort::SceneView &sv, const ort::RenderHot &hot) {
    using namespace ort_ad;
    ort::with_bools([&](auto C, auto D, auto T) {
        hipLaunchKernelGGL((radiance_adaptive_rays<decltype(C)::value, decltype(D)::value, decltype(T)::value>), dim3(pl.grid), dim3(kBlock), 0, stream, sv, hot);
    }, pl.counters, pl.diffuse, pl.tabs);
}
