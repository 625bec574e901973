/*
 * ort_kernels_render_adaptive.hip -- the kernels of the camera renders that run one-pixel jobs over a batch of views with something
 * added to the plain loop: the adaptive render (ort_render_adaptive, ort_render_views_adaptive: pt_adaptive), the light-group
 * render (ort_render_light_groups, ort_render_views_light_groups: pt_groups), the sample-map render (ort_render_sample_map,
 * ort_render_views_sample_map: pt_sample_map) and the accumulating render (ort_render_accumulate, ort_render_views_accumulate:
 * pt_accumulate).  The path-depth render (ort_render_depths, ort_render_views_depths: pt_depths) is the fifth.
 *
 * The lane code (ort_lane.h) compiled a fourth time, at the limits of ort_kernels.hip proper (four waves per SIMD, 24 LDS stack
 * entries), for the eight variants of pt_lane with LF_IMPLICIT | LF_VIEWS | LF_ADAPT, the eight with LF_IMPLICIT | LF_VIEWS |
 * LF_GROUPS and the eight with LF_IMPLICIT | LF_VIEWS | LF_SPPMAP only.  A unit of its own for the reason ort_kernels_adaptive.hip is one: more path-trace kernels are compile
 * time that ort_kernels.hip, the unit that sets the build's wall time, should not carry; here they compile beside the others
 * (profiles/r12_render_adaptive.md, profiles/r21_light_groups.md).  The light-group kernels share this unit, sixteen kernels as
 * the irradiance unit holds, instead of adding a sixth.  The sample-map kernels make it twenty-four: measured, the unit then
 * compiles in about half the time ort_kernels.hip takes beside it, so the build's wall time is still that unit's
 * (profiles/r23_sample_map.md).  The eight pt_accumulate kernels (LF_SPPMAP | LF_ACCUM) make it thirty-two: the unit then
 * takes three quarters of ort_kernels.hip's time (profiles/r24_accumulate.md).  The eight pt_depths kernels (LF_DEPTHS) make it
 * forty: compiled side by side on eight cores, 61 s against ort_kernels.hip's 79 s, which still sets the wall time
 * (profiles/r32_depths.md).
 * All five families are built in full, every <counters, diffuse, tabs>, so that nothing lists them (variant_built, ort_plan.h):
 * device_render (ort_kernels.hip), for a render of a kind that is not plain, launches them through the one entry point below.
 */
#define ORT_NS ort_ra /* the limits: ort_lane.h's defaults */
#include "ort_lane.h"

/* A variant of a pixel-job kind's family (KF_ADAPTIVE to KF_DEPTHS): implicit jobs over a batch of views.  The caller's own
   SceneView and RenderHot: the argument structs are ort_lane.h's one definition.  A new kind is one more case */
void ort_launch_pixel_jobs(const ort::KernelVariant &v, unsigned int grid, hipStream_t stream, const ort::SceneView &sv, const ort::RenderHot &hot) {
    using namespace ort_ra;
    ort::with_bools([&](auto C, auto D, auto T) {
        constexpr bool c = decltype(C)::value, d = decltype(D)::value, t = decltype(T)::value;
        switch (v.family) {
        case ort::KF_ADAPTIVE: hipLaunchKernelGGL((pt_adaptive<c, d, t>), dim3(grid), dim3(kBlock), 0, stream, sv, hot); break;
        case ort::KF_GROUPS: hipLaunchKernelGGL((pt_groups<c, d, t>), dim3(grid), dim3(kBlock), 0, stream, sv, hot); break;
        case ort::KF_SAMPLE_MAP: hipLaunchKernelGGL((pt_sample_map<c, d, t>), dim3(grid), dim3(kBlock), 0, stream, sv, hot); break;
        case ort::KF_ACCUM: hipLaunchKernelGGL((pt_accumulate<c, d, t>), dim3(grid), dim3(kBlock), 0, stream, sv, hot); break;
        case ort::KF_DEPTHS: hipLaunchKernelGGL((pt_depths<c, d, t>), dim3(grid), dim3(kBlock), 0, stream, sv, hot); break;
        default: break; /* launch_path_tracer sends no other family here */
        }
    }, v.counters, v.diffuse, v.tabs);
}
