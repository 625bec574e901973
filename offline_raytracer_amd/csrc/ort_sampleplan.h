/*
 * ort_sampleplan.h -- the sample planner of include/ort.h (ort_plan_samples): its pixel functions, and their kernels.
 *
 * Host-and-device, as ort_denoise.h is: ort_kernels.hip includes it for the kernels (gfx950) and their plumbing
 * (device_plan_samples), tools/sampleplan_sim.cpp compiles the same pixel functions for the host and walks them over every pixel.
 * Every f32 operation is separately rounded in the order include/ort.h states (-ffp-contract=off, correctly rounded divides); no
 * transcendental function.  Everything that is summed is an integer, and the one maximum that crosses lanes is taken over
 * non-negative floats through their bits, so neither the tile shape, the grid nor the order in which workgroups arrive can change
 * a bit of the map or of the totals.
 *
 * Three steps, each a kernel:
 *    error   the three planes -> the E plane (the workspace: one f32 per pixel), the squared relative standard error of the
 *            pixel's mean luminance; +0 for a pixel that is unknown (fewer than 2 samples) or invalid (a count past 2^24, an
 *            error that is not finite).  Validity is decided here and never judged again: what is not > 0 is stored as +0, so
 *            every later comparison is one of non-negative finite floats.  The frame's counters and its worst error.
 *    want    the maximum of E over the pixel's window -> what the pixel wants, into the map; the frame's sum of wants.
 *    scale   where the frame's sum is over the budget, want * budget / wanted by integer division, in place; the frame's sum
 *            of what is planned.  A frame that is within its budget is not read again: its first tile adds wanted to planned.
 */
#ifndef ORT_SAMPLEPLAN_H
#define ORT_SAMPLEPLAN_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ORT_SP __host__ __device__ __forceinline__
#else
#define ORT_SP static inline
#endif

namespace ortsp {

/* the call's parameters as the kernels use them: tol2 = tolerance*tolerance is taken once, on the host */
struct Params {
    float tol2, floor;
    uint32_t radius, pilot, min_add, cap, rgb_is_sum;
    uint64_t budget;
};

/* ort_plan_totals as the kernels write it: worst through its bits (an e is never below +0, so the order of the bits is the
   order of the floats) */
struct Totals {
    unsigned long long wanted, planned;
    uint32_t unconverged, unknown, invalid, worst_bits;
};
static_assert(sizeof(Totals) == 32, "ort_plan_totals is 32 bytes");

constexpr uint64_t kWorkspaceBytesPerPixel = 4; /* the E plane */
constexpr uint32_t kMaxCount = 1u << 24;        /* a pixel never passes 2^24 samples (ort_render_accumulate) */
constexpr uint32_t kUnconverged = 1u, kUnknown = 2u, kInvalid = 4u; /* what error_pixel says of a pixel; 0: valid and converged */

ORT_SP bool finite1(float v) {
    uint32_t b;
    __builtin_memcpy(&b, &v, 4);
    return (b & 0x7f800000u) != 0x7f800000u;
}
ORT_SP uint32_t bits_of(float v) {
    uint32_t b;
    __builtin_memcpy(&b, &v, 4);
    return b;
}
ORT_SP float lum(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }

/* step 1 of one pixel: entry i of the three planes -> entry i of E; returns kUnknown, kInvalid, kUnconverged or 0 */
ORT_SP uint32_t error_pixel(const float *rgb, const float *m2, const uint32_t *count, float *e_plane, size_t i, const Params &prm) {
    const uint32_t n = count[i];
    const float fn = (float)n;
    const float l = lum(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
    const float m = prm.rgb_is_sum ? l / fn : l;
    float v = m2[i] / fn - m * m;
    if (v < 0.0f) v = 0.0f;
    const float vm = v / (fn - 1.0f);
    const float a = __builtin_fabsf(m);
    const float b = a > prm.floor ? a : prm.floor;
    float e = vm / (b * b);
    uint32_t what;
    if (n < 2u) {
        what = kUnknown;
        e = 0.0f;
    } else if (n > kMaxCount || !finite1(e)) {
        what = kInvalid;
        e = 0.0f;
    } else {
        if (!(e > 0.0f)) e = 0.0f; /* -0 becomes +0 */
        what = e > prm.tol2 ? kUnconverged : 0u;
    }
    e_plane[i] = e;
    return what;
}

/* step 2 of one pixel, in two halves: the maximum of E over the window of (x, y) in the frame whose first entry is `base` ... */
ORT_SP float window_max(const float *e_plane, size_t base, int W, int H, int x, int y, int r) {
    float d = 0.0f;
    for (int dy = -r; dy <= r; ++dy) {
        const long long qy = (long long)y + dy; /* 64-bit: a width or height may be near 2^31 */
        if (qy < 0 || qy >= H) continue;
        for (int dx = -r; dx <= r; ++dx) {
            const long long qx = (long long)x + dx;
            if (qx < 0 || qx >= W) continue;
            const float e = e_plane[base + (size_t)qy * (size_t)W + (size_t)qx];
            d = e > d ? e : d;
        }
    }
    return d;
}
/* ... and what a pixel with n samples and that maximum d wants; d is not read for an unknown pixel */
ORT_SP uint32_t want_of(uint32_t n, float d, const Params &prm) {
    const uint32_t left = kMaxCount - (n < kMaxCount ? n : kMaxCount);
    const uint32_t room = prm.cap < left ? prm.cap : left;
    if (n < 2u) return prm.pilot < room ? prm.pilot : room;
    if (!(d > prm.tol2)) return 0u;
    const float fn = (float)n;
    const float need = fn * (d / prm.tol2) - fn;
    uint32_t k = need >= 16777216.0f ? kMaxCount : (need > 0.0f ? (uint32_t)need : 0u);
    if (k < prm.min_add) k = prm.min_add;
    return k < room ? k : room;
}
ORT_SP uint32_t want_pixel(const float *e_plane, const uint32_t *count, size_t base, int W, int H, int x, int y, const Params &prm) {
    const uint32_t n = count[base + (size_t)y * (size_t)W + (size_t)x];
    return want_of(n, n < 2u ? 0.0f : window_max(e_plane, base, W, H, x, y, (int)prm.radius), prm);
}

/* step 3: is the frame over its budget, and what a pixel of such a frame gets.  want <= 2^24 and budget <= 2^39: the product
   fits 64 bits */
ORT_SP bool over_budget(uint64_t wanted, uint64_t budget) { return budget != 0u && wanted > budget; }
ORT_SP uint32_t scaled_want(uint32_t want, uint64_t wanted, uint64_t budget) { return (uint32_t)((uint64_t)want * budget / wanted); }

#if (defined(__HIP__) || defined(__HIPCC__)) && !defined(ORT_HOST_SIM)
/* ---- the kernels: one lane per pixel, the denoiser's tiles ------------------------------------------------------------------
   Tiles [0, tiles) of kTileW x kTileH pixels, frame-major then row-major, a grid-stride loop over tiles: the frame of a
   workgroup's tiles never decreases, so a workgroup keeps its lanes' partial sums in registers while the frame stays the same
   and reduces them -- across each wave, then across the four waves through LDS -- when the frame changes and at its end: one
   atomic per total, workgroup and frame it touched.  Every atomic is an integer one */
constexpr int kTileW = 64, kTileH = 4;
constexpr unsigned long long kNoFrame = ~0ull;

struct Add { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };
struct Max { template <typename T> __device__ T operator()(T a, T b) const { return a > b ? a : b; } };

/* every lane of the workgroup calls it (the callers' conditions are uniform); lane 0 of wave 0 gets the whole */
template <typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, T *lds, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, (T)__shfl_down(v, o));
    __syncthreads(); /* the previous use of lds is over */
    if ((threadIdx.x & 63u) == 0u) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return op(op(lds[0], lds[1]), op(lds[2], lds[3]));
}

struct TilePos { unsigned long long f; long long x, y; bool first; };
__device__ __forceinline__ TilePos tile_pos(uint64_t t, uint32_t tiles_x, uint32_t tiles_y) {
    const uint64_t row = t / tiles_x, f = row / tiles_y;
    const uint32_t tx = (uint32_t)(t - row * tiles_x), ty = (uint32_t)(row - f * tiles_y);
    return TilePos{f, (long long)tx * kTileW + (long long)(threadIdx.x & (kTileW - 1)), (long long)ty * kTileH + (long long)(threadIdx.x / kTileW),
                   tx == 0u && ty == 0u};
}

__global__ __launch_bounds__(256) void sampleplan_error(const float *rgb, const float *m2, const uint32_t *count, float *e_plane, Totals *totals,
                                                        int W, int H, uint32_t tiles_x, uint32_t tiles_y, uint64_t tiles, Params prm) {
    __shared__ uint32_t lds[4];
    uint32_t unconverged = 0u, unknown = 0u, invalid = 0u, worst = 0u;
    unsigned long long cur = kNoFrame;
    auto flush = [&]() {
        const uint32_t a = block_reduce(unconverged, lds, Add()), b = block_reduce(unknown, lds, Add()), c = block_reduce(invalid, lds, Add());
        const uint32_t w = block_reduce(worst, lds, Max());
        if (threadIdx.x == 0u) {
            if (a) atomicAdd(&totals[cur].unconverged, a);
            if (b) atomicAdd(&totals[cur].unknown, b);
            if (c) atomicAdd(&totals[cur].invalid, c);
            if (w) atomicMax(&totals[cur].worst_bits, w);
        }
        unconverged = unknown = invalid = worst = 0u;
    };
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const TilePos tp = tile_pos(t, tiles_x, tiles_y);
        if (tp.f != cur) { /* uniform over the workgroup */
            if (cur != kNoFrame) flush();
            cur = tp.f;
        }
        if (tp.x < W && tp.y < H) {
            const size_t i = (size_t)tp.f * (size_t)W * (size_t)H + (size_t)tp.y * (size_t)W + (size_t)tp.x;
            const uint32_t what = error_pixel(rgb, m2, count, e_plane, i, prm);
            unconverged += what & kUnconverged ? 1u : 0u;
            unknown += what & kUnknown ? 1u : 0u;
            invalid += what & kInvalid ? 1u : 0u;
            const uint32_t eb = bits_of(e_plane[i]);
            worst = eb > worst ? eb : worst;
        }
    }
    if (cur != kNoFrame) flush();
}

/* TILE: the window is read from LDS.  The workgroup first copies its tile of E with a halo of `radius` pixels -- (64 + 2r) x (4 + 2r)
   floats, at most 70 x 10 -- into LDS, +0 standing for what lies outside the frame: +0 is the identity of a maximum over
   non-negative floats, so the window needs no bounds and gives the bits of window_max.  Without TILE every tap is a load through
   L1 / L2 (window_max itself).  Same map either way; which one a call takes is device_plan_samples' choice */
constexpr int kMaxRadius = 3, kHaloW = kTileW + 2 * kMaxRadius, kHaloH = kTileH + 2 * kMaxRadius;
template <bool TILE>
__global__ __launch_bounds__(256) void sampleplan_want(const float *e_plane, const uint32_t *count, uint32_t *sample_map, Totals *totals, int W, int H,
                                                       uint32_t tiles_x, uint32_t tiles_y, uint64_t tiles, Params prm) {
    __shared__ unsigned long long lds[4];
    __shared__ float halo[TILE ? kHaloW * kHaloH : 1];
    const int r = (int)prm.radius < kMaxRadius ? (int)prm.radius : kMaxRadius, lw = kTileW + 2 * r, lh = kTileH + 2 * r;
    unsigned long long wanted = 0ull; /* 64 bits from the first add: one tile's wants can sum to exactly 2^32 */
    unsigned long long cur = kNoFrame;
    auto flush = [&]() {
        const unsigned long long s = block_reduce(wanted, lds, Add());
        if (threadIdx.x == 0u && s) atomicAdd(&totals[cur].wanted, s);
        wanted = 0ull;
    };
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const TilePos tp = tile_pos(t, tiles_x, tiles_y);
        if (tp.f != cur) {
            if (cur != kNoFrame) flush();
            cur = tp.f;
        }
        const size_t base = (size_t)tp.f * (size_t)W * (size_t)H;
        if constexpr (TILE) {
            const long long x0 = tp.x - (long long)(threadIdx.x & (kTileW - 1)) - r, y0 = tp.y - (long long)(threadIdx.x / kTileW) - r; /* the halo's corner */
            __syncthreads(); /* the previous tile's windows are read */
            for (int i = (int)threadIdx.x; i < lw * lh; i += 256) {
                const long long gx = x0 + i % lw, gy = y0 + i / lw;
                halo[i] = gx >= 0 && gx < W && gy >= 0 && gy < H ? e_plane[base + (size_t)gy * (size_t)W + (size_t)gx] : 0.0f;
            }
            __syncthreads();
        }
        if (tp.x < W && tp.y < H) {
            uint32_t k;
            if constexpr (TILE) {
                const uint32_t n = count[base + (size_t)tp.y * (size_t)W + (size_t)tp.x];
                float d = 0.0f;
                if (n >= 2u) {
                    const float *row = halo + (threadIdx.x / kTileW) * lw + (threadIdx.x & (kTileW - 1));
                    for (int dy = 0; dy <= 2 * r; ++dy, row += lw)
                        for (int dx = 0; dx <= 2 * r; ++dx) d = row[dx] > d ? row[dx] : d;
                }
                k = want_of(n, d, prm);
            } else {
                k = want_pixel(e_plane, count, base, W, H, (int)tp.x, (int)tp.y, prm);
            }
            sample_map[base + (size_t)tp.y * (size_t)W + (size_t)tp.x] = k;
            wanted += k;
        }
    }
    if (cur != kNoFrame) flush();
}

__global__ __launch_bounds__(256) void sampleplan_scale(uint32_t *sample_map, Totals *totals, int W, int H, uint32_t tiles_x, uint32_t tiles_y,
                                                        uint64_t tiles, Params prm) {
    __shared__ unsigned long long lds[4];
    unsigned long long planned = 0ull;
    unsigned long long cur = kNoFrame;
    auto flush = [&]() {
        const unsigned long long s = block_reduce(planned, lds, Add());
        if (threadIdx.x == 0u && s) atomicAdd(&totals[cur].planned, s);
        planned = 0ull;
    };
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const TilePos tp = tile_pos(t, tiles_x, tiles_y);
        if (tp.f != cur) {
            if (cur != kNoFrame) flush();
            cur = tp.f;
        }
        const unsigned long long wanted = totals[tp.f].wanted; /* complete: sampleplan_want has ended */
        if (!over_budget(wanted, prm.budget)) { /* the map stands as it is: this lane's share of planned is the frame's, once */
            if (tp.first && threadIdx.x == 0u) planned += wanted;
            continue;
        }
        if (tp.x < W && tp.y < H) {
            const size_t i = (size_t)tp.f * (size_t)W * (size_t)H + (size_t)tp.y * (size_t)W + (size_t)tp.x;
            const uint32_t k = scaled_want(sample_map[i], wanted, prm.budget);
            sample_map[i] = k;
            planned += k;
        }
    }
    if (cur != kNoFrame) flush();
}
#endif

} // namespace ortsp
#endif /* ORT_SAMPLEPLAN_H */
