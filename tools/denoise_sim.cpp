/*
 * denoise_sim -- the denoiser's pixel functions (offline_raytracer_amd/csrc/ort_denoise.h) compiled for the host: the pack and
 * the a-trous passes over every pixel, one after the other, as device_denoise (ort_kernels.hip) launches them.  No device, no HIP:
 * what the kernels compute, under a host compiler and, as denoise_sim_san, under AddressSanitizer and
 * UndefinedBehaviorSanitizer (tests/test_denoise_host.py).
 *
 *   denoise_sim W H FRAMES ITERATIONS NORMAL_SQUARINGS SIGMA_L SIGMA_Z rgb m2 count albedo normal depth out
 *
 * The six inputs and the output are raw little-endian plane files as include/ort.h lays them out (FRAMES frames, view-major, row
 * 0 first): rgb, albedo, normal and out 3 f32 per pixel, m2 and depth one f32, count one u32.  out may name the rgb file.
 * The arguments are judged as ort_denoise judges them; exit status 2 for a bad argument, 1 for a file that cannot be read or
 * written.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../offline_raytracer_amd/csrc/ort_denoise.h"

using namespace ortdn;

template <typename T>
static bool read_plane(const char *path, size_t n, std::vector<T> *v) {
    v->resize(n);
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "denoise_sim: cannot open %s\n", path); return false; }
    const size_t got = fread(v->data(), sizeof(T), n, f);
    const bool at_end = fgetc(f) == EOF;
    fclose(f);
    if (got != n || !at_end) { fprintf(stderr, "denoise_sim: %s does not hold %zu entries of %zu bytes\n", path, n, sizeof(T)); return false; }
    return true;
}

int main(int argc, char **argv) {
    if (argc != 15) {
        fprintf(stderr, "usage: denoise_sim W H FRAMES ITERATIONS NORMAL_SQUARINGS SIGMA_L SIGMA_Z rgb m2 count albedo normal depth out\n");
        return 2;
    }
    const long long W = atoll(argv[1]), H = atoll(argv[2]), F = atoll(argv[3]), iterations = atoll(argv[4]), squarings = atoll(argv[5]);
    const float sigma_l = strtof(argv[6], nullptr), sigma_z = strtof(argv[7], nullptr);
    if (W < 1 || H < 1 || F < 1 || W * H * F >= (1ll << 31) || W >= (1ll << 31) || H >= (1ll << 31) || iterations < 1 || iterations > 8 || squarings < 0 ||
        squarings > 8 || !(sigma_l > 0.0f) || !finite1(sigma_l) || !(sigma_z > 0.0f) || !finite1(sigma_z)) {
        fprintf(stderr, "denoise_sim: bad argument\n");
        return 2;
    }
    const size_t n = (size_t)(W * H * F);
    std::vector<float> rgb, m2, albedo, normal, depth;
    std::vector<uint32_t> count;
    if (!read_plane(argv[8], 3 * n, &rgb) || !read_plane(argv[9], n, &m2) || !read_plane(argv[10], n, &count) || !read_plane(argv[11], 3 * n, &albedo) ||
        !read_plane(argv[12], 3 * n, &normal) || !read_plane(argv[13], n, &depth))
        return 1;
    std::vector<F4> cv[2] = {std::vector<F4>(n), std::vector<F4>(n)}, gd(n);
    std::vector<float> out(3 * n);
    for (size_t i = 0; i < n; ++i) pack_pixel(rgb.data(), m2.data(), count.data(), albedo.data(), normal.data(), depth.data(), cv[0].data(), gd.data(), i);
    const Params prm{(uint32_t)iterations, (uint32_t)squarings, sigma_l * sigma_l, sigma_z * sigma_z};
    for (uint32_t j = 0; j < prm.iterations; ++j) {
        const int s = 1 << j;
        const bool last = j + 1u == prm.iterations;
        const F4 *src = cv[j & 1u].data();
        F4 *dst = cv[(j & 1u) ^ 1u].data();
        for (long long f = 0; f < F; ++f)
            for (long long y = 0; y < H; ++y)
                for (long long x = 0; x < W; ++x) {
                    const size_t base = (size_t)(f * W * H);
                    if (last) atrous_pixel<true>(src, gd.data(), nullptr, rgb.data(), albedo.data(), out.data(), base, (int)W, (int)H, (int)x, (int)y, s, prm);
                    else atrous_pixel<false>(src, gd.data(), dst, nullptr, nullptr, nullptr, base, (int)W, (int)H, (int)x, (int)y, s, prm);
                }
    }
    FILE *f = fopen(argv[14], "wb");
    if (!f || fwrite(out.data(), 4, 3 * n, f) != 3 * n || fclose(f) != 0) { fprintf(stderr, "denoise_sim: cannot write %s\n", argv[14]); return 1; }
    return 0;
}
