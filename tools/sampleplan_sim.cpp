/*
 * sampleplan_sim -- the sample planner's pixel functions (offline_raytracer_amd/csrc/ort_sampleplan.h) compiled for the host: the
 * error, want and scale steps over every pixel, one after the other, as device_plan_samples (ort_kernels.hip) launches them, the
 * sums taken in a plain loop.  No device, no HIP: what the kernels compute, under a host compiler and, as sampleplan_sim_san,
 * under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_plan_host.py).
 *
 *   sampleplan_sim W H FRAMES TOLERANCE FLOOR RADIUS PILOT MIN_ADD CAP RGB_IS_SUM BUDGET rgb m2 count map totals
 *
 * The three inputs and the map are raw little-endian plane files as include/ort.h lays them out (FRAMES frames, view-major, row 0
 * first): rgb 3 f32 per pixel, m2 one f32, count and map one u32; totals is FRAMES entries of ort_plan_totals, 32 bytes each.
 * TOLERANCE and FLOOR are read as f32 from their decimal text.  The arguments are judged as ort_plan_samples judges them; exit
 * status 2 for a bad argument, 1 for a file that cannot be read or written.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../offline_raytracer_amd/csrc/ort_sampleplan.h"

using namespace ortsp;

template <typename T>
static bool read_plane(const char *path, size_t n, std::vector<T> *v) {
    v->resize(n);
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "sampleplan_sim: cannot open %s\n", path); return false; }
    const size_t got = fread(v->data(), sizeof(T), n, f);
    const bool at_end = fgetc(f) == EOF;
    fclose(f);
    if (got != n || !at_end) { fprintf(stderr, "sampleplan_sim: %s does not hold %zu entries of %zu bytes\n", path, n, sizeof(T)); return false; }
    return true;
}

static bool write_file(const char *path, const void *data, size_t bytes) {
    FILE *f = fopen(path, "wb");
    if (!f) { fprintf(stderr, "sampleplan_sim: cannot write %s\n", path); return false; }
    const bool ok = fwrite(data, 1, bytes, f) == bytes;
    if (fclose(f) != 0 || !ok) { fprintf(stderr, "sampleplan_sim: cannot write %s\n", path); return false; }
    return true;
}

int main(int argc, char **argv) {
    if (argc != 17) {
        fprintf(stderr, "usage: sampleplan_sim W H FRAMES TOLERANCE FLOOR RADIUS PILOT MIN_ADD CAP RGB_IS_SUM BUDGET rgb m2 count map totals\n");
        return 2;
    }
    const long long W = atoll(argv[1]), H = atoll(argv[2]), F = atoll(argv[3]);
    const float tolerance = strtof(argv[4], nullptr), floor = strtof(argv[5], nullptr);
    const long long radius = atoll(argv[6]), pilot = atoll(argv[7]), min_add = atoll(argv[8]), cap = atoll(argv[9]), is_sum = atoll(argv[10]);
    const unsigned long long budget = strtoull(argv[11], nullptr, 10);
    if (W < 1 || H < 1 || F < 1 || W >= (1ll << 31) || H >= (1ll << 31) || F >= (1ll << 31) || W * H >= (1ll << 31) || W * H * F >= (1ll << 31) ||
        !(tolerance > 0.0f) || !finite1(tolerance) || !(tolerance * tolerance > 0.0f) || !(floor > 0.0f) || !finite1(floor) || radius < 0 || radius > 3 ||
        pilot < 0 || pilot > 0xFFFFFFFFll || min_add < 1 || min_add > 0xFFFFFFFFll || cap < 1 || cap > (1ll << 24) || is_sum < 0 || is_sum > 1 ||
        argv[11][0] == '-' || budget > (1ull << 39)) {
        fprintf(stderr, "sampleplan_sim: bad argument\n");
        return 2;
    }
    const size_t per_frame = (size_t)(W * H), n = per_frame * (size_t)F;
    std::vector<float> rgb, m2;
    std::vector<uint32_t> count;
    if (!read_plane(argv[12], 3 * n, &rgb) || !read_plane(argv[13], n, &m2) || !read_plane(argv[14], n, &count)) return 1;
    const Params prm{tolerance * tolerance, floor, (uint32_t)radius, (uint32_t)pilot, (uint32_t)min_add, (uint32_t)cap, (uint32_t)is_sum, (uint64_t)budget};
    std::vector<float> e_plane(n);
    std::vector<uint32_t> map(n);
    std::vector<Totals> totals((size_t)F);
    memset(totals.data(), 0, sizeof(Totals) * totals.size());
    for (long long f = 0; f < F; ++f) {
        Totals &t = totals[(size_t)f];
        const size_t base = (size_t)f * per_frame;
        for (size_t i = base; i < base + per_frame; ++i) {
            const uint32_t what = error_pixel(rgb.data(), m2.data(), count.data(), e_plane.data(), i, prm);
            t.unconverged += what & kUnconverged ? 1u : 0u;
            t.unknown += what & kUnknown ? 1u : 0u;
            t.invalid += what & kInvalid ? 1u : 0u;
            const uint32_t eb = bits_of(e_plane[i]);
            t.worst_bits = eb > t.worst_bits ? eb : t.worst_bits;
        }
        for (long long y = 0; y < H; ++y)
            for (long long x = 0; x < W; ++x) {
                const uint32_t k = want_pixel(e_plane.data(), count.data(), base, (int)W, (int)H, (int)x, (int)y, prm);
                map[base + (size_t)(y * W + x)] = k;
                t.wanted += k;
            }
        if (over_budget(t.wanted, prm.budget)) {
            for (size_t i = base; i < base + per_frame; ++i) {
                map[i] = scaled_want(map[i], t.wanted, prm.budget);
                t.planned += map[i];
            }
        } else {
            t.planned = t.wanted;
        }
    }
    if (!write_file(argv[15], map.data(), 4 * n) || !write_file(argv[16], totals.data(), sizeof(Totals) * totals.size())) return 1;
    return 0;
}
