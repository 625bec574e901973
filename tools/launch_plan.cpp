/* Developer tool: what device_render or a ray query would launch.  The launch policy (csrc/ort_plan.h) is arithmetic on a few
   facts about the uploaded scene, the render parameters or the ray count and the knobs, so it runs without a device:
     [ORT_... knobs] tools/launch_plan key=value ...   ->   the plan, one JSON line
   query=raycast|occluded|radiance count=N [counters=1]: the QueryPlan of that ray query over N rays (plan_ray_query,
   plan_radiance) instead of a render's LaunchPlan.  query=features width= height= x1= y1= [x0= y0= views=N spp= counters=1 fill=1]:
   the QueryPlan of ort_render_features, or with views=N of ort_render_views_features (plan_features), its job count and, with
   fill=1, features_view's fill of the RenderView.  query=follow with the same arguments and rr=: ort_render_follow's (plan_follow,
   follow_view); query=matte with features' arguments: ort_render_matte's (plan_matte, matte_view).  Otherwise
   keys: the SceneTraits and ort_render_params fields by name, policy=pixel|chunk, counters=1, explicit_jobs=1 job_count=N,
   w5_layout_ok=0, views=N (the plan of an ort_render_views batch of N views; its fields are appended to the line), one of
   adaptive=1, groups=1, sample_map=1, accumulate=1, depths=1 (plan_pixel_jobs for that kind: the plan of ort_render_adaptive,
   ort_render_light_groups, ort_render_sample_map, ort_render_accumulate or ort_render_depths, or with views=N of its views form; the key and the
   views fields are appended); fill=1: after the plan, every field of the RenderView that is not a pointer as the shared fill
   (render_view, csrc/ort_setup.h) sets it for that plan, "name = value" one per line -- seed=, rr= are the call's, view_seed=S
   gives view v of views=N the seed S + v, min_spp= max_spp= check_every= tolerance= floor= are the stopping rule's; max_blocks
   defaults to what an upload on cu_count units fixes.  tab_flags, where not given, follows from
   materials= (index 0 included), lights=, pro_boxes=, pro_spheres=, pro_cyls= as at upload (table_fit_flags; all 0 by default).  tests/test_launch_plan.py holds the measured
   crossovers and the knobs the GPU tests force kernels with against it.
   variant=1: the kernel the plan names (plan_variant) and whether it is built (variant_built) are appended to the line.
   sweep=1, and nothing else: every plan of a grid over traits, calls and knobs (sweep() below) held against the built kernels; one
   JSON line with the number of plans, how many name no built kernel, and the first of those. */
#include <stdio.h>

#include <type_traits>
#include <vector>

#include "../include/ort.h"
#include "../offline_raytracer_amd/csrc/ort_plan.h"
#include "../offline_raytracer_amd/csrc/ort_setup.h"

/* ort::RenderView (csrc/ort_lane.h, which only a HIP compiler reads: the one definition all kernel units and the host side share)
   without its pointers: the fields render_view fills.  This stand-in is why the set-up functions of ort_setup.h are templates.  Kept
   by hand in step with ort_lane.h: a field render_view assigns and this list lacks does not compile, but one added to RenderView and
   forgotten in render_view does not show here */
#define FILL_FIELDS(F) F(mode) F(W) F(H) F(x0) F(y0) F(x1) F(y1) F(seed) F(spp) F(chunk) F(rr) F(packed_out) F(nchunks) F(job_count) F(shard_index) \
    F(shard_count) F(blocks_w) F(block_x0) F(block_y0) F(my_blocks) F(view_jobs) F(view_count) F(refill_below) F(descend_below) F(capL) F(capR) F(long_min) \
    F(long_refill) F(inflight_cap) F(park_min) F(endgame_from) F(stash_wave_f4) F(block_major) F(job_batch) F(batch_until) F(ad_min_spp) F(ad_check_every) \
    F(ad_tolerance) F(ad_floor)
struct FillView {
    int mode, W, H, x0, y0, x1, y1, refill_below, descend_below, packed_out;
    uint32_t seed, spp, chunk, nchunks, shard_index, shard_count, blocks_w, block_x0, block_y0, my_blocks, view_count, capL, capR, long_min, long_refill,
        inflight_cap, park_min, stash_wave_f4, block_major, job_batch, ad_min_spp, ad_check_every;
    unsigned long long job_count, view_jobs, endgame_from, batch_until;
    float rr, ad_tolerance, ad_floor;
};

/* the pixel-job kinds, in the order of their enum, by their key on the command line, which is also their field of the output and
   the name of their kernel family */
struct PixelJobKey { const char *key; ort::RenderKind kind; };
static const PixelJobKey kPixelJobKeys[] = {{"adaptive", ort::RK_ADAPTIVE}, {"groups", ort::RK_GROUPS}, {"sample_map", ort::RK_SAMPLE_MAP}, {"accumulate", ort::RK_ACCUMULATE}, {"depths", ort::RK_DEPTHS}};

/* "family<counters, diffuse, tabs, implicit, wide>" */
static std::string variant_name(const ort::KernelVariant &v) {
    static const char *family[] = {"none", "wavefront", "loop", "loop_views", "exchange", "five"};
    char b[64];
    snprintf(b, sizeof(b), "%s<%d, %d, %d, %d, %d>", ort::pixel_job_family(v.family) ? kPixelJobKeys[v.family - ort::KF_ADAPTIVE].key : family[v.family], v.counters,
             v.diffuse, v.tabs, v.implicit, v.wide);
    return b;
}

/* every plan the policy gives over: both BSDF flavours; all tables, the prologue's alone, none; a tree inside and outside the L2; a
   cheap and a dear one; with and without the wide form; PIXEL, CHUNK and explicit jobs (the WHOLE policy); counters; one view and
   three (implicit job spaces); a frame smaller than the grid and a long launch; both answers of the five-waves layout check; and
   the knobs that choose kernels, unset and forced either way.  plan_pixel_jobs, every kind, for the single PIXEL frames */
static int sweep() {
    unsigned long long plans = 0, unbuilt = 0;
    std::string first;
    auto hold = [&](const ort::LaunchPlan &l) {
        ++plans;
        const ort::KernelVariant v = ort::plan_variant(l);
        if (ort::variant_built(v)) return;
        if (unbuilt++ < 5) first += (first.empty() ? "\"" : ", \"") + variant_name(v) + "\"";
    };
    const uint32_t tab_flags[] = {ort::kPlanAllTabs, ort::kPlanTabPro, 0u};
    const int policies[] = {ORT_POLICY_PIXEL, ORT_POLICY_CHUNK, ORT_POLICY_WHOLE};
    const int tri[] = {-1, 0, 1};
    ort::Knobs kn;
    ort::SceneTraits t;
    t.cu_count = 256;
    t.max_blocks = ort::upload_max_blocks(t.cu_count, kn);
    for (int diffuse_only = 0; diffuse_only < 2; ++diffuse_only) for (uint32_t flags : tab_flags) for (size_t mb : {1u, 64u})
    for (float sah : {0.02f, 0.3f}) for (int has_wide = 0; has_wide < 2; ++has_wide) {
        t.diffuse_only = diffuse_only != 0; t.tab_flags = flags; t.fast_tree_bytes = mb << 20; t.sah_cost = sah; t.has_wide = has_wide != 0;
        for (int policy : policies) for (int counters = 0; counters < 2; ++counters) for (int big = 0; big < 2; ++big)
        for (uint32_t views : {1u, 3u}) for (int w5 = 0; w5 < 2; ++w5) {
            const bool explicit_jobs = policy == ORT_POLICY_WHOLE;
            if (explicit_jobs && views > 1u) continue;
            ort_render_params p{};
            p.width = big ? 1920 : 45; p.height = big ? 1080 : 35; p.spp = big ? 512u : 8u; p.chunk = big ? 64u : 4u;
            p.policy = policy; p.rr = 0.8f; p.flags = counters ? ORT_RENDER_COUNTERS : 0;
            const uint64_t jobs = explicit_jobs ? ort::shard_block_count(&p) : 0; /* a job per 8 x 8 block */
            for (int exchange : tri) for (int wide : tri) for (int waves5 : tri) for (int wavefront = 0; wavefront < 2; ++wavefront)
            for (int general = 0; general < 2; ++general) for (int lds_tables : {-1, 0}) for (int util = 0; util < 2; ++util) {
                kn.exchange = exchange; kn.wide = wide; kn.waves5 = waves5; kn.wavefront = wavefront != 0;
                kn.general_kernel = general != 0; kn.lds_tables = lds_tables; kn.debug_util = util != 0;
                hold(ort::plan_render(t, p, explicit_jobs, jobs, w5 != 0, kn, views));
                if (policy == ORT_POLICY_PIXEL && views == 1u)
                    for (const PixelJobKey &k : kPixelJobKeys) hold(ort::plan_pixel_jobs(k.kind, t, p, kn, 1));
            }
        }
    }
    printf("{\"sweep\": 1, \"plans\": %llu, \"unbuilt\": %llu, \"first\": [%s]}\n", plans, unbuilt, first.c_str());
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && strcmp(argv[1], "sweep=1") == 0) return sweep();
    const ort::Knobs kn = ort::read_knobs();
    ort::SceneTraits t;
    t.tab_flags = ort::kPlanAllTabs;
    t.cu_count = 256;
    ort_render_params p{};
    p.policy = ORT_POLICY_CHUNK;
    p.chunk = 1;
    p.rr = 0.8f;
    bool explicit_jobs = false, w5_layout_ok = true, tab_flags_given = false;
    unsigned long materials = 0, lights = 0, pro_boxes = 0, pro_spheres = 0, pro_cyls = 0;
    unsigned long long job_count = 0;
    unsigned long view_count = 1;
    bool views_given = false, fill = false, variant = false;
    unsigned asked = 0; /* bit k: kPixelJobKeys[k] was given as 1; at most one may be, and that one is the call's kind (key, below) */
    unsigned long view_seed = 0;
    ort_adaptive ad{};
    const char *query = nullptr;
    unsigned long long count = 0;
    for (int i = 1; i < argc; ++i) {
        const char *eq = strchr(argv[i], '=');
        const size_t n = eq ? (size_t)(eq - argv[i]) : 0;
        const char *v = eq ? eq + 1 : "";
        auto is = [&](const char *key) { return strlen(key) == n && strncmp(argv[i], key, n) == 0; };
        auto kind_bit = [&]() { /* of a pixel-job kind's key, 0 for any other argument */
            unsigned bit = 1u;
            for (const PixelJobKey &k : kPixelJobKeys) { if (is(k.key)) return bit; bit <<= 1; }
            return 0u;
        };
        if (is("diffuse_only")) t.diffuse_only = atoi(v) != 0;
        else if (is("tab_flags")) { t.tab_flags = (uint32_t)strtoul(v, nullptr, 0); tab_flags_given = true; }
        else if (is("materials")) materials = strtoul(v, nullptr, 0);
        else if (is("lights")) lights = strtoul(v, nullptr, 0);
        else if (is("pro_boxes")) pro_boxes = strtoul(v, nullptr, 0);
        else if (is("pro_spheres")) pro_spheres = strtoul(v, nullptr, 0);
        else if (is("pro_cyls")) pro_cyls = strtoul(v, nullptr, 0);
        else if (is("fast_tree_bytes")) t.fast_tree_bytes = (size_t)strtoull(v, nullptr, 0);
        else if (is("sah_cost")) t.sah_cost = strtof(v, nullptr);
        else if (is("has_wide")) t.has_wide = atoi(v) != 0;
        else if (is("cu_count")) t.cu_count = atoi(v);
        else if (is("max_blocks")) t.max_blocks = (unsigned int)strtoul(v, nullptr, 0);
        else if (is("width")) p.width = atoi(v);
        else if (is("height")) p.height = atoi(v);
        else if (is("x0")) p.x0 = atoi(v);
        else if (is("y0")) p.y0 = atoi(v);
        else if (is("x1")) p.x1 = atoi(v);
        else if (is("y1")) p.y1 = atoi(v);
        else if (is("policy")) p.policy = strcmp(v, "pixel") == 0 ? ORT_POLICY_PIXEL : ORT_POLICY_CHUNK;
        else if (is("spp")) p.spp = (uint32_t)strtoul(v, nullptr, 0);
        else if (is("chunk")) p.chunk = (uint32_t)strtoul(v, nullptr, 0);
        else if (is("counters")) p.flags |= atoi(v) ? ORT_RENDER_COUNTERS : 0;
        else if (is("shard_index")) p.shard_index = (uint32_t)strtoul(v, nullptr, 0);
        else if (is("shard_count")) p.shard_count = (uint32_t)strtoul(v, nullptr, 0);
        else if (is("explicit_jobs")) explicit_jobs = atoi(v) != 0;
        else if (is("job_count")) job_count = strtoull(v, nullptr, 0);
        else if (is("w5_layout_ok")) w5_layout_ok = atoi(v) != 0;
        else if (is("query")) query = v;
        else if (is("count")) count = strtoull(v, nullptr, 0);
        else if (is("views")) { view_count = strtoul(v, nullptr, 0); views_given = true; }
        else if (const unsigned bit = kind_bit()) asked = atoi(v) ? asked | bit : asked & ~bit;
        else if (is("fill")) fill = atoi(v) != 0;
        else if (is("variant")) variant = atoi(v) != 0;
        else if (is("seed")) p.seed = (uint32_t)strtoul(v, nullptr, 0);
        else if (is("rr")) p.rr = strtof(v, nullptr);
        else if (is("view_seed")) view_seed = strtoul(v, nullptr, 0);
        else if (is("min_spp")) ad.min_spp = (uint32_t)strtoul(v, nullptr, 0);
        else if (is("max_spp")) ad.max_spp = (uint32_t)strtoul(v, nullptr, 0);
        else if (is("check_every")) ad.check_every = (uint32_t)strtoul(v, nullptr, 0);
        else if (is("tolerance")) ad.tolerance = strtof(v, nullptr);
        else if (is("floor")) ad.floor = strtof(v, nullptr);
        else { fprintf(stderr, "launch_plan: unknown argument %s\n", argv[i]); return 2; }
    }
    if (!tab_flags_given) t.tab_flags = ort::table_fit_flags(materials, lights, (uint32_t)pro_boxes, (uint32_t)pro_spheres, (uint32_t)pro_cyls);
    if (!t.max_blocks) t.max_blocks = ort::upload_max_blocks(t.cu_count, kn);
    if (query) {
        const bool radiance = strcmp(query, "radiance") == 0, counters = (p.flags & ORT_RENDER_COUNTERS) != 0;
        const bool follow = strcmp(query, "follow") == 0; /* plan_follow and follow_view where features has plan_features and features_view */
        const bool matte = strcmp(query, "matte") == 0;   /* plan_matte and matte_view */
        if (follow || matte || strcmp(query, "features") == 0) { /* plan_features over [view][block under the rect][pixel in block]; fill=1: features_view's fill */
            if (p.width <= 0 || p.height <= 0 || p.x0 < 0 || p.y0 < 0 || p.x1 > p.width || p.y1 > p.height || p.x0 >= p.x1 || p.y0 >= p.y1 || view_count < 1 ||
                view_count > ORT_MAX_VIEWS || p.shard_count > 1) { fprintf(stderr, "launch_plan: query=features|follow|matte width= height= x1= y1= [x0= y0= views=1..%u spp= rr=], no shards\n", ORT_MAX_VIEWS); return 2; }
            const ort::QueryPlan q = follow  ? ort::plan_follow(t, p, (uint32_t)view_count, counters, kn)
                                     : matte ? ort::plan_matte(t, p, (uint32_t)view_count, counters, kn)
                                             : ort::plan_features(t, p, (uint32_t)view_count, counters, kn);
            printf("{\"query\": \"%s\", \"count\": %llu, \"view_jobs\": %llu, \"view_count\": %lu, \"counters\": %d, \"diffuse\": %d, \"tabs\": %d, \"grid\": %u, "
                   "\"refill_below\": %d, \"descend_below\": %d, \"job_batch\": %u, \"batch_until\": %llu, \"max_blocks\": %u, \"tab_flags\": %u}\n",
                   query, ort::feature_view_jobs(p) * view_count, ort::feature_view_jobs(p), view_count, q.counters, q.diffuse, q.tabs, q.grid, q.refill_below, q.descend_below,
                   q.job_batch, q.batch_until, t.max_blocks, t.tab_flags);
            if (fill) {
                FillView rv{};
                if (follow) ort::follow_view(p, (uint32_t)view_count, &rv);
                else if (matte) ort::matte_view(p, (uint32_t)view_count, &rv);
                else ort::features_view(p, (uint32_t)view_count, &rv);
                rv.job_batch = q.job_batch; rv.batch_until = q.batch_until; rv.refill_below = q.refill_below; rv.descend_below = q.descend_below; /* as launch_planned sets them */
                auto print = [](const char *name, auto v) {
                    if constexpr (std::is_floating_point<decltype(v)>::value) printf("%s = %.9g\n", name, (double)v);
                    else printf("%s = %lld\n", name, (long long)v);
                };
#define FEATURE_FILL_PRINT(f) print(#f, rv.f);
                FILL_FIELDS(FEATURE_FILL_PRINT)
            }
            return 0;
        }
        if ((!radiance && strcmp(query, "raycast") && strcmp(query, "occluded")) || count < 1) { fprintf(stderr, "launch_plan: query=raycast|occluded|radiance count=1...\n"); return 2; }
        const ort::QueryPlan q = radiance ? ort::plan_radiance(t, count, counters, kn) : ort::plan_ray_query(t, count, counters);
        printf("{\"query\": \"%s\", \"count\": %llu, \"counters\": %d, \"diffuse\": %d, \"tabs\": %d, \"grid\": %u, \"refill_below\": %d, \"descend_below\": %d, "
               "\"job_batch\": %u, \"batch_until\": %llu, \"max_blocks\": %u, \"tab_flags\": %u}\n",
               query, count, q.counters, q.diffuse, q.tabs, q.grid, q.refill_below, q.descend_below, q.job_batch, q.batch_until, t.max_blocks, t.tab_flags);
        return 0;
    }
    if (!explicit_jobs && p.policy == ORT_POLICY_CHUNK && p.chunk == 0) { fprintf(stderr, "launch_plan: chunk=0\n"); return 2; }
    if (views_given && (view_count < 1 || view_count > ORT_MAX_VIEWS || explicit_jobs)) { fprintf(stderr, "launch_plan: views=1..%u, implicit job spaces only\n", ORT_MAX_VIEWS); return 2; }
    if (asked && (explicit_jobs || p.policy != ORT_POLICY_PIXEL || p.shard_count > 1 || (asked & (asked - 1u)))) { fprintf(stderr, "launch_plan: adaptive=1, groups=1, sample_map=1 or accumulate=1 (one of them) needs policy=pixel, implicit jobs and no shards\n"); return 2; }
    const PixelJobKey *key = nullptr; /* null: the plain render */
    for (const PixelJobKey &k : kPixelJobKeys)
        if (asked == 1u << (&k - kPixelJobKeys)) key = &k;
    const ort::LaunchPlan l = key ? ort::plan_pixel_jobs(key->kind, t, p, kn, (uint32_t)view_count)
                                  : ort::plan_render(t, p, explicit_jobs, job_count, w5_layout_ok, kn, (uint32_t)view_count);
    printf("{\"wavefront\": %d, \"exchange\": %d, \"five\": %d, \"wide\": %d, \"counters\": %d, \"diffuse\": %d, \"tabs\": %d, \"implicit\": %d, \"util\": %d, "
           "\"grid\": %u, \"mode\": %d, \"nchunks\": %u, \"job_count\": %llu, \"my_blocks\": %u, \"refill_below\": %d, \"descend_below\": %d, "
           "\"capL\": %u, \"capR\": %u, \"long_min\": %u, \"long_refill\": %u, \"inflight_cap\": %u, \"park_min\": %u, \"endgame_from\": %llu, "
           "\"stash_wave_f4\": %u, \"block_major\": %u, \"job_batch\": %u, \"batch_until\": %llu, \"partial_bytes\": %zu, \"stash_bytes\": %zu, "
           "\"drain_bytes\": %zu, \"max_blocks\": %u, \"tab_flags\": %u, \"tab_caps\": {\"materials\": %u, \"lights\": %u, \"pro_slots\": %u}",
           l.wavefront, l.exchange, l.five, l.wide, l.counters, l.diffuse, l.tabs, l.implicit, l.util, l.grid, l.mode, l.nchunks, l.job_count,
           l.blocks.my_blocks, l.refill_below, l.descend_below, l.capL, l.capR, l.long_min, l.long_refill, l.inflight_cap, l.park_min,
           l.endgame_from, l.stash_wave_f4, l.block_major, l.job_batch, l.batch_until, l.partial_bytes, l.stash_bytes, l.drain_bytes, t.max_blocks,
           t.tab_flags, ort::kPlanTabMatCap, ort::kPlanTabLightCap, ort::kPlanTabProCap);
    if (key) printf(", \"%s\": %d", key->key, l.kind == key->kind);
    if (views_given || key) printf(", \"views\": %d, \"view_count\": %u, \"view_jobs\": %llu", l.views, l.view_count, l.view_jobs);
    if (variant) printf(", \"variant\": \"%s\", \"built\": %d", variant_name(ort::plan_variant(l)).c_str(), ort::variant_built(ort::plan_variant(l)));
    printf("}\n");
    if (fill) { /* as device_render calls it: a batch's views, the single adaptive frame's one view, or none */
        std::vector<ort_view> views(views_given || key ? view_count : 0);
        for (size_t v = 0; v < views.size(); ++v) views[v].seed = (uint32_t)(view_seed + v);
        FillView rv{};
        ort::render_view(p, l, views.empty() ? nullptr : views.data(), key && key->kind == ort::RK_ADAPTIVE ? &ad : nullptr, &rv);
        auto print = [](const char *name, auto v) {
            if constexpr (std::is_floating_point<decltype(v)>::value) printf("%s = %.9g\n", name, (double)v);
            else printf("%s = %lld\n", name, (long long)v);
        };
#define FILL_PRINT(f) print(#f, rv.f);
        FILL_FIELDS(FILL_PRINT)
    }
    return 0;
}
