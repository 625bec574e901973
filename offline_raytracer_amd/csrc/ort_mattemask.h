/*
 * ort_mattemask.h -- a mask from matte slots (include/ort.h: ort_matte_mask): its pixel function, and its kernel.
 *
 * Host-and-device, as ort_denoise.h is: ort_kernels.hip includes it for the kernel (gfx950) and its plumbing
 * (device_matte_mask), tools/mattemask_sim.cpp compiles the same pixel function for the host and walks it over every pixel.
 * A pixel's result is a u32 sum over its own slots, one conversion and one correctly rounded f32 division: no shared state,
 * so neither the grid nor the lane a pixel falls on can change a bit.
 *
 * The selection.  The host sorts the caller's ids and drops the duplicates (prepare_select), so "a duplicate counts once" is a
 * property of the table, and membership is a binary search: at most 8 probes of at most 256 words.  The table travels as a kernel
 * argument -- 1028 bytes, copied by the launch itself, so the device form neither allocates nor reads the caller's memory after
 * it returns -- and every workgroup copies it into LDS once; one lane a pixel from there on, by grid stride.
 */
#ifndef ORT_MATTEMASK_H
#define ORT_MATTEMASK_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ORT_MM __host__ __device__ __forceinline__
#else
#define ORT_MM static inline
#endif

namespace ortmm {

constexpr uint32_t kMaxSelect = 256; /* ORT_MAX_MATTE_SELECT */
constexpr uint32_t kEmpty = 0xffffffffu; /* ORT_MATTE_EMPTY */

/* the selection as the kernel takes it: n ids, ascending, each once */
struct Select {
    uint32_t n;
    uint32_t id[kMaxSelect];
};

/* the caller's select_count <= kMaxSelect ids -> the sorted table without duplicates (an insertion sort: host only, 256 at most) */
static inline void prepare_select(const uint32_t *select, uint32_t select_count, Select *out) {
    out->n = 0;
    for (uint32_t i = 0; i < select_count && i < kMaxSelect; ++i) {
        const uint32_t v = select[i];
        uint32_t at = 0;
        while (at < out->n && out->id[at] < v) ++at;
        if (at < out->n && out->id[at] == v) continue;
        for (uint32_t k = out->n; k > at; --k) out->id[k] = out->id[k - 1u];
        out->id[at] = v;
        out->n++;
    }
    for (uint32_t i = out->n; i < kMaxSelect; ++i) out->id[i] = kEmpty;
}

/* is id one of sel[0 .. n), ascending and unique? */
ORT_MM bool selected(const uint32_t *sel, uint32_t n, uint32_t id) {
    uint32_t lo = 0, hi = n; /* the answer, if any, is in [lo, hi) */
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t v = sel[mid];
        if (v == id) return true;
        if (v < id) lo = mid + 1u;
        else hi = mid;
    }
    return false;
}

/* pixel p: the u32 sum of the selected slots' counts over (float)spp */
ORT_MM float mask_pixel(const uint32_t *ids, const uint32_t *counts, uint32_t slots, const uint32_t *sel, uint32_t n, float fspp, size_t p) {
    uint32_t sum = 0;
    for (uint32_t j = 0; j < slots; ++j) {
        const uint32_t id = ids[p * slots + j];
        if (id != kEmpty && selected(sel, n, id)) sum += counts[p * slots + j];
    }
    return (float)sum / fspp;
}

#if defined(__HIP__) || defined(__HIPCC__)
__global__ void __launch_bounds__(256) matte_mask(const uint32_t *ids, const uint32_t *counts, float *out_mask, uint32_t slots, float fspp, uint32_t pixels, Select s) {
    __shared__ uint32_t sel[kMaxSelect];
    for (uint32_t i = threadIdx.x; i < kMaxSelect; i += 256u) sel[i] = s.id[i];
    __syncthreads();
    const uint32_t n = s.n;
    for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < pixels; p += (uint64_t)gridDim.x * 256u)
        out_mask[p] = mask_pixel(ids, counts, slots, sel, n, fspp, (size_t)p);
}
#endif

} // namespace ortmm

#endif
