/*
 * mattemask_sim -- the matte mask's pixel function (offline_raytracer_amd/csrc/ort_mattemask.h) compiled for the host and walked
 * over every pixel, with the selection prepared as device_matte_mask (ort_kernels.hip) prepares it.  No device, no HIP: what the
 * kernel computes, under a host compiler and, as mattemask_sim_san, under AddressSanitizer and UndefinedBehaviorSanitizer
 * (tests/test_matte_host.py).
 *
 *   mattemask_sim W H FRAMES SLOTS SPP ids counts select out
 *
 * Raw little-endian files: ids and counts FRAMES x H x W x SLOTS u32 as ort_render_matte lays them out, select 1 .. 256 u32, out
 * FRAMES x H x W f32.  The arguments are judged as ort_matte_mask judges them; exit status 2 for a bad argument, 1 for a file that
 * cannot be read or written.
 */
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../offline_raytracer_amd/csrc/ort_mattemask.h"

using namespace ortmm;

/* the whole file as u32 words; n != 0: exactly n words */
static bool read_words(const char *path, size_t n, std::vector<uint32_t> *v) {
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "mattemask_sim: cannot open %s\n", path); return false; }
    uint32_t w;
    v->clear();
    while (fread(&w, 4, 1, f) == 1) v->push_back(w);
    const bool at_end = feof(f) && ftell(f) == (long)(4 * v->size());
    fclose(f);
    if (!at_end || (n && v->size() != n)) { fprintf(stderr, "mattemask_sim: %s does not hold the %zu words expected\n", path, n); return false; }
    return true;
}

int main(int argc, char **argv) {
    if (argc != 10) {
        fprintf(stderr, "usage: mattemask_sim W H FRAMES SLOTS SPP ids counts select out\n");
        return 2;
    }
    const long long W = atoll(argv[1]), H = atoll(argv[2]), F = atoll(argv[3]), slots = atoll(argv[4]), spp = atoll(argv[5]);
    if (slots < 1 || slots > 8 || W < 1 || H < 1 || F < 1 || W >= (1ll << 31) || H >= (1ll << 31) || F >= (1ll << 31) || W * H >= (1ll << 31) ||
        W * H * F * slots >= (1ll << 31) || spp < 1 || spp > (1ll << 24)) {
        fprintf(stderr, "mattemask_sim: bad argument\n");
        return 2;
    }
    const size_t n = (size_t)(W * H * F);
    std::vector<uint32_t> ids, counts, select;
    if (!read_words(argv[6], n * (size_t)slots, &ids) || !read_words(argv[7], n * (size_t)slots, &counts) || !read_words(argv[8], 0, &select)) return 1;
    if (select.empty() || select.size() > kMaxSelect) { fprintf(stderr, "mattemask_sim: select must hold 1 .. %u ids\n", kMaxSelect); return 2; }
    for (uint32_t v : select)
        if (v == kEmpty) { fprintf(stderr, "mattemask_sim: ORT_MATTE_EMPTY in select\n"); return 2; }
    Select sel;
    prepare_select(select.data(), (uint32_t)select.size(), &sel);
    /* exactly sel.n words, as a heap block of their own: a probe past the selection is a read past the block */
    std::vector<uint32_t> table(sel.id, sel.id + sel.n);
    std::vector<float> out(n);
    for (size_t p = 0; p < n; ++p) out[p] = mask_pixel(ids.data(), counts.data(), (uint32_t)slots, table.data(), sel.n, (float)spp, p);
    FILE *f = fopen(argv[9], "wb");
    if (!f || fwrite(out.data(), 4, n, f) != n || fclose(f) != 0) { fprintf(stderr, "mattemask_sim: cannot write %s\n", argv[9]); return 1; }
    return 0;
}
