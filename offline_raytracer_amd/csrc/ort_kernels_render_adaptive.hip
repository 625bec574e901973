/*
 * ort_kernels_render_adaptive.hip -- the kernels of the camera renders that run one-pixel jobs over a batch of views with something
 * added to the plain loop: the adaptive render (ort_render_adaptive, ort_render_views_adaptive: pt_adaptive), the light-group
 * render (ort_render_light_groups, ort_render_views_light_groups: pt_groups), the sample-map render (ort_render_sample_map,
 * ort_render_views_sample_map: pt_sample_map) and the accumulating render (ort_render_accumulate, ort_render_views_accumulate:
 * pt_accumulate).
 *
 * The lane code (ort_lane.h) compiled a fourth time, at the limits of ort_kernels.hip proper (four waves per SIMD, 24 LDS stack
 * entries), for the eight variants of pt_lane with LF_IMPLICIT | LF_VIEWS | LF_ADAPT, the eight with LF_IMPLICIT | LF_VIEWS |
 * LF_GROUPS and the eight with LF_IMPLICIT | LF_VIEWS | LF_SPPMAP only.  A unit of its own for the reason ort_kernels_adaptive.hip is one: more path-trace kernels are compile
 * time that ort_kernels.hip, the unit that sets the build's wall time, should not carry; here they compile beside the others
 * (profiles/r12_render_adaptive.md, profiles/r21_light_groups.md).  The light-group kernels share this unit, sixteen kernels as
 * the irradiance unit holds, instead of adding a sixth.  The sample-map kernels make it twenty-four: measured, the unit then
 * compiles in about half the time ort_kernels.hip takes beside it, so the build's wall time is still that unit's
 * (profiles/r23_sample_map.md).  The eight pt_accumulate kernels (LF_SPPMAP | LF_ACCUM) make it thirty-two: the unit then
 * takes three quarters of ort_kernels.hip's time (profiles/r24_accumulate.md), launched through ort_launch_render_accumulate.
 * device_render (ort_kernels.hip), given a stopping rule, a group table or a sample map, launches
 * them through ort_launch_render_adaptive, ort_launch_render_groups or ort_launch_render_sample_map.
 */
#define ORT_NS ort_ra /* the limits: ort_lane.h's defaults */
#include "ort_lane.h"

/* KF_ADAPTIVE: implicit jobs over a batch of views.  The caller's own SceneView and RenderHot: the argument structs are
   ort_lane.h's one definition */
void ort_launch_render_adaptive(const ort::KernelVariant &v, unsigned int grid, hipStream_t stream, const ort::SceneView &sv, const ort::RenderHot &hot) {
    using namespace ort_ra;
    ort::with_bools([&](auto C, auto D, auto T) {
        hipLaunchKernelGGL((pt_adaptive<decltype(C)::value, decltype(D)::value, decltype(T)::value>), dim3(grid), dim3(kBlock), 0, stream, sv, hot);
    }, v.counters, v.diffuse, v.tabs);
}

/* KF_GROUPS: likewise */
void ort_launch_render_groups(const ort::KernelVariant &v, unsigned int grid, hipStream_t stream, const ort::SceneView &sv, const ort::RenderHot &hot) {
    using namespace ort_ra;
    ort::with_bools([&](auto C, auto D, auto T) {
        hipLaunchKernelGGL((pt_groups<decltype(C)::value, decltype(D)::value, decltype(T)::value>), dim3(grid), dim3(kBlock), 0, stream, sv, hot);
    }, v.counters, v.diffuse, v.tabs);
}

/* KF_SAMPLE_MAP: likewise */
void ort_launch_render_sample_map(const ort::KernelVariant &v, unsigned int grid, hipStream_t stream, const ort::SceneView &sv, const ort::RenderHot &hot) {
    using namespace ort_ra;
    ort::with_bools([&](auto C, auto D, auto T) {
        hipLaunchKernelGGL((pt_sample_map<decltype(C)::value, decltype(D)::value, decltype(T)::value>), dim3(grid), dim3(kBlock), 0, stream, sv, hot);
    }, v.counters, v.diffuse, v.tabs);
}

/* KF_ACCUM: likewise */
void ort_launch_render_accumulate(const ort::KernelVariant &v, unsigned int grid, hipStream_t stream, const ort::SceneView &sv, const ort::RenderHot &hot) {
    using namespace ort_ra;
    ort::with_bools([&](auto C, auto D, auto T) {
        hipLaunchKernelGGL((pt_accumulate<decltype(C)::value, decltype(D)::value, decltype(T)::value>), dim3(grid), dim3(kBlock), 0, stream, sv, hot);
    }, v.counters, v.diffuse, v.tabs);
}
