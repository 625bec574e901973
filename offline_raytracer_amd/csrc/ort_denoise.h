/*
 * ort_denoise.h -- the edge-avoiding a-trous denoiser of include/ort.h (ort_denoise): its pixel functions, and their kernels.
 *
 * Host-and-device, as ort_lane.h is: ort_kernels.hip includes it for the kernels (gfx950) and their plumbing
 * (device_denoise), tools/denoise_sim.cpp compiles the same pixel functions for the host and walks them over every pixel.
 * Every operation is a separately rounded f32 operation in the order include/ort.h states (-ffp-contract=off, correctly
 * rounded divides); no transcendental function, no atomics, no shared state: a pixel's result depends on the planes of the
 * previous pass alone, so neither the tile shape nor the lane a pixel falls on can change a bit.
 *
 * Planes.  denoise_pack reads the caller's six planes once and writes two planes of 16 bytes per pixel:
 *    CV = (c.xyz, var)     the albedo-demodulated colour and the variance of its luminance; var = -1 marks an UNUSABLE pixel
 *    GD = (n.xyz, depth)   the guides
 * so that a tap is one 16-byte load of each, and lanes adjacent in x read adjacent addresses at every stride.  A usable pixel's
 * variance is never below -0 (a clamped difference over squares, then sums of squares times such values), and a NaN is not
 * below zero either, so `var < 0` is the mark and nothing else: usability is decided by the pack and never judged again.
 * The passes ping-pong between two CV planes; the last one remodulates from the albedo plane and writes out_rgb.
 */
#ifndef ORT_DENOISE_H
#define ORT_DENOISE_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ORT_DN __host__ __device__ __forceinline__
#else
#define ORT_DN static inline
#endif

namespace ortdn {

struct alignas(16) F4 { float x, y, z, w; };

/* the call's parameters as the passes use them: the two squares are taken once, on the host */
struct Params {
    uint32_t iterations, normal_squarings;
    float sl2, sz2; /* sigma_l*sigma_l, sigma_z*sigma_z */
};

constexpr uint64_t kWorkspaceBytesPerPixel = 48; /* two CV planes and one GD plane */
constexpr float kAlbedoFloor = 1e-3f;

ORT_DN bool finite1(float v) {
    uint32_t b;
    __builtin_memcpy(&b, &v, 4);
    return (b & 0x7f800000u) != 0x7f800000u;
}
ORT_DN bool finite3(float x, float y, float z) { return finite1(x) && finite1(y) && finite1(z); }
ORT_DN float lum(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }
ORT_DN float fall(float x) {
    float r = 1.0f / (1.0f + x);
    r = r * r;
    r = r * r;
    return r;
}
ORT_DN float floor_albedo(float a) { return a > kAlbedoFloor ? a : kAlbedoFloor; }
ORT_DN float absf(float v) { return __builtin_fabsf(v); }

/* the prologue of one pixel: entry i of the six planes -> entry i of CV and GD */
ORT_DN void pack_pixel(const float *rgb, const float *m2, const uint32_t *count, const float *albedo, const float *normal,
                       const float *depth, F4 *cv, F4 *gd, size_t i) {
    const uint32_t n = count[i];
    const float fn = (float)n;
    const float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2], q = m2[i];
    const float al0 = albedo[3 * i], al1 = albedo[3 * i + 1], al2 = albedo[3 * i + 2];
    const float a0 = floor_albedo(al0), a1 = floor_albedo(al1), a2 = floor_albedo(al2);
    const float c0 = r / a0, c1 = g / a1, c2 = b / a2;
    const float Y = lum(r, g, b);
    float v = q / fn - Y * Y;
    if (v < 0.0f) v = 0.0f;
    const float vm = n > 1u ? v / (fn - 1.0f) : Y * Y;
    const float la = lum(a0, a1, a2);
    const float var = vm / (la * la);
    const float nx = normal[3 * i], ny = normal[3 * i + 1], nz = normal[3 * i + 2], z = depth[i];
    const bool usable = n >= 1u && finite3(r, g, b) && finite1(q) && finite3(al0, al1, al2) && finite3(nx, ny, nz) && finite1(z) &&
                        finite3(c0, c1, c2) && finite1(var);
    F4 o;
    o.x = c0; o.y = c1; o.z = c2; o.w = usable ? var : -1.0f;
    cv[i] = o;
    o.x = nx; o.y = ny; o.z = nz; o.w = z;
    gd[i] = o;
}

/* one pass of one pixel: (x, y) of the frame whose first entry is `base`, taps at stride s.  cv_in and gd are read at the taps,
   only this pixel's entry of cv_out (or, LAST, of out_rgb) is written; LAST reads this pixel's own rgb and albedo, and nothing
   else of those planes, so out_rgb may be rgb itself. */
template <bool LAST>
ORT_DN void atrous_pixel(const F4 *cv_in, const F4 *gd, F4 *cv_out, const float *rgb, const float *albedo, float *out_rgb,
                         size_t base, int W, int H, int x, int y, int s, const Params &prm) {
    const size_t p = base + (size_t)y * (size_t)W + (size_t)x;
    const F4 cp = cv_in[p];
    if (cp.w < 0.0f) { /* unusable: never a tap, and its output is its input, bit for bit */
        if (LAST) {
            const uint32_t *src = (const uint32_t *)rgb + 3 * p;
            uint32_t *dst = (uint32_t *)out_rgb + 3 * p;
            const uint32_t b0 = src[0], b1 = src[1], b2 = src[2];
            dst[0] = b0; dst[1] = b1; dst[2] = b2;
        } else {
            cv_out[p] = cp;
        }
        return;
    }
    /* the variance prefilter: 3 x 3 at stride 1, only .w of a tap is read */
    float G = 0.0f, GW = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const float vq = cv_in[base + (size_t)qy * (size_t)W + (size_t)qx].w;
            if (vq < 0.0f) continue;
            const float w3 = (dx ? 0.25f : 0.5f) * (dy ? 0.25f : 0.5f);
            G = G + w3 * vq;
            GW = GW + w3;
        }
    }
    const float g = G / GW;
    const float lp = lum(cp.x, cp.y, cp.z);
    const float den = prm.sl2 * g + 1e-10f;
    const F4 gp = gd[p];
    float S0 = 0.0f, S1 = 0.0f, S2 = 0.0f, V = 0.0f, Wt = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
            const float h = (ax == 0 ? 0.375f : ax == 1 ? 0.25f : 0.0625f) * (ay == 0 ? 0.375f : ay == 1 ? 0.25f : 0.0625f);
            F4 cq;
            float w;
            if (dx == 0 && dy == 0) {
                cq = cp;
                w = h;
            } else {
                /* 64-bit: s*dx reaches 256 beyond a width that may itself be near 2^31 */
                const long long qx = (long long)x + (long long)s * dx, qy = (long long)y + (long long)s * dy;
                if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                const size_t q = base + (size_t)qy * (size_t)W + (size_t)qx;
                cq = cv_in[q];
                if (cq.w < 0.0f) continue;
                const F4 gq = gd[q];
                const float d = (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z;
                float wn = d > 0.0f ? d : 0.0f;
                for (uint32_t k = 0; k < prm.normal_squarings; ++k) wn = wn * wn;
                const float dz = gp.w - gq.w;
                const float zp = absf(gp.w), zq = absf(gq.w);
                const float zm = zp > zq ? zp : zq;
                const float xz = (dz * dz) / (((zm * zm) * (float)(s * s * (dx * dx + dy * dy))) * prm.sz2);
                const float dl = lp - lum(cq.x, cq.y, cq.z);
                const float xl = (dl * dl) / den;
                w = ((h * wn) * fall(xz)) * fall(xl);
                if (!finite1(w)) w = 0.0f;
            }
            S0 = S0 + w * cq.x;
            S1 = S1 + w * cq.y;
            S2 = S2 + w * cq.z;
            V = V + (w * w) * cq.w;
            Wt = Wt + w;
        }
    }
    const float o0 = S0 / Wt, o1 = S1 / Wt, o2 = S2 / Wt;
    if (LAST) {
        out_rgb[3 * p] = o0 * floor_albedo(albedo[3 * p]);
        out_rgb[3 * p + 1] = o1 * floor_albedo(albedo[3 * p + 1]);
        out_rgb[3 * p + 2] = o2 * floor_albedo(albedo[3 * p + 2]);
    } else {
        F4 o;
        o.x = o0; o.y = o1; o.z = o2; o.w = V / (Wt * Wt);
        cv_out[p] = o;
    }
}

#if (defined(__HIP__) || defined(__HIPCC__)) && !defined(ORT_HOST_SIM)
/* ---- the kernels: one lane per pixel --------------------------------------------------------------------------------------- */
constexpr int kTileW = 64, kTileH = 4; /* a workgroup of 256 lanes: each wave is 64 pixels of one row, 1 KiB per tap and plane */

/* entries [0, total) of the six planes, a grid-stride loop (total < 2^31) */
__global__ __launch_bounds__(256) void denoise_pack(const float *rgb, const float *m2, const uint32_t *count, const float *albedo,
                                                    const float *normal, const float *depth, F4 *cv, F4 *gd, uint32_t total) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256u)
        pack_pixel(rgb, m2, count, albedo, normal, depth, cv, gd, (size_t)i);
}

/* tiles [0, tiles) of kTileW x kTileH pixels, frame-major then row-major, a grid-stride loop over tiles: a frame of one column
   and 2^30 rows has more tiles than a grid has workgroups */
template <bool LAST>
__global__ __launch_bounds__(256) void denoise_atrous(const F4 *cv_in, const F4 *gd, F4 *cv_out, const float *rgb, const float *albedo,
                                                      float *out_rgb, int W, int H, uint32_t tiles_x, uint32_t tiles_y, uint64_t tiles,
                                                      int s, Params prm) {
    const int lx = (int)(threadIdx.x & (kTileW - 1)), ly = (int)(threadIdx.x / kTileW);
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t row = t / tiles_x, f = row / tiles_y;
        const uint32_t tx = (uint32_t)(t - row * tiles_x), ty = (uint32_t)(row - f * tiles_y);
        const long long x = (long long)tx * kTileW + lx, y = (long long)ty * kTileH + ly;
        if (x >= W || y >= H) continue;
        atrous_pixel<LAST>(cv_in, gd, cv_out, rgb, albedo, out_rgb, (size_t)f * (size_t)W * (size_t)H, W, H, (int)x, (int)y, s, prm);
    }
}
#endif

} // namespace ortdn
#endif /* ORT_DENOISE_H */
