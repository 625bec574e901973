/*
 * ort_api.cpp -- the C ABI declared in include/ort.h.  Host-side plumbing only: argument
 * checks, the caller-side seeding policies (code/macos_main.mm:602-662) expressed as job
 * lists, and dispatch to the HIP path in ort_kernels.hip.  There is no CPU render path:
 * every render entry point fails unless the scene is resident on a HIP device.
 */
#include <float.h>
#include <math.h>
#include <string.h>

#include <exception>
#include <initializer_list>
#include <new>
#include <memory>
#include <string>
#include <vector>

#include "ort_plan.h" /* shard_block_count, render_workspace_bytes */
#include "ort_scene.h"

namespace {

thread_local std::string g_error;

int fail(int code, const std::string &msg) {
    g_error = msg;
    return code;
}

/* random_u32 (random.h:83-89) on the master series: used for the per-tile seeds */
uint32_t xorshift(uint32_t *s) {
    uint32_t x = *s;
    x ^= x << 13;
    x ^= x >> 17;
    x ^= x >> 5; /* sic: third shift is right (random.h:10-12) */
    *s = x;
    return x;
}

/* the render parameters by themselves (everything check_params says before it looks at the scene's state) */
int check_param_values(const ort_scene *scene, const ort_render_params *p) {
    if (!scene || !p) return fail(ORT_ERR_INVALID, "null scene or params");
    if (p->width <= 0 || p->height <= 0) return fail(ORT_ERR_INVALID, "image size must be positive");
    if ((uint64_t)p->width * (uint64_t)p->height > 0x7fffffffull / 3) return fail(ORT_ERR_INVALID, "image too large");
    if (p->width > 65535 || p->height > 65535) return fail(ORT_ERR_UNSUPPORTED, "image side above 65535 (lane state packs coordinates in 16 bits)");
    if (p->policy == ORT_POLICY_CHUNK && p->chunk && p->spp / p->chunk > 65535u) return fail(ORT_ERR_UNSUPPORTED, "more than 65535 chunks");
    if (p->x0 < 0 || p->y0 < 0 || p->x1 > p->width || p->y1 > p->height || p->x0 >= p->x1 || p->y0 >= p->y1)
        return fail(ORT_ERR_INVALID, "render rect is empty or outside the image");
    if (p->spp == 0) return fail(ORT_ERR_INVALID, "spp must be >= 1");
    if (!(p->rr >= 0.0f)) return fail(ORT_ERR_INVALID, "rr must be >= 0");
    if (p->policy == ORT_POLICY_CHUNK && (p->chunk == 0 || p->spp % p->chunk))
        return fail(ORT_ERR_INVALID, "spp must be a multiple of chunk");
    if (p->policy < ORT_POLICY_TILE32 || p->policy > ORT_POLICY_CHUNK) return fail(ORT_ERR_INVALID, "unknown policy");
    if (p->shard_count > 1 && p->shard_index >= p->shard_count) return fail(ORT_ERR_INVALID, "shard index out of range");
    if (p->shard_count > 1 && (p->policy == ORT_POLICY_TILE32 || p->policy == ORT_POLICY_WHOLE))
        return fail(ORT_ERR_UNSUPPORTED, "sharding needs a per-pixel seeding policy (PIXEL or CHUNK)");
    if (p->flags & ORT_RENDER_PACKED) {
        if (p->policy == ORT_POLICY_TILE32 || p->policy == ORT_POLICY_WHOLE)
            return fail(ORT_ERR_UNSUPPORTED, "a packed framebuffer needs a per-pixel seeding policy (PIXEL or CHUNK)");
        if (p->x0 != 0 || p->y0 != 0 || p->x1 != p->width || p->y1 != p->height)
            return fail(ORT_ERR_INVALID, "a packed framebuffer covers the whole image: the rect must be the full frame");
    }
    return ORT_OK;
}

/* the scene's state, which every call that launches looks at last: committed, and resident on a device */
int check_resident(const ort_scene *scene) {
    if (!scene->tree.built) return fail(ORT_ERR_STATE, "ort_scene_commit has not been called");
    if (!scene->dev) return fail(ORT_ERR_NO_DEVICE, "scene is not resident on a HIP device: call ort_scene_upload (no CPU fallback)");
    return ORT_OK;
}

int check_params(const ort_scene *scene, const ort_render_params *p) {
    int rc = check_param_values(scene, p);
    return rc != ORT_OK ? rc : check_resident(scene);
}

/* a call over nothing: OK, and no work was done */
int nothing_to_do(ort_stats *stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    return ORT_OK;
}

/* main()'s tile schedule (macos_main.mm:602-662) as explicit jobs: every one of the 1024
   tiles draws its seed, rendered or not; only tiles wholly inside the rect are rendered */
void tile32_jobs(const ort_render_params *p, std::vector<ort_tile_job> *jobs) {
    uint32_t master = p->seed;
    int32_t tw = (int32_t)ceilf(p->width / (float)32), th = (int32_t)ceilf(p->height / (float)32);
    for (int32_t ty = 0; ty < 32; ++ty)
        for (int32_t tx = 0; tx < 32; ++tx) {
            ort_tile_job j;
            j.x0 = tx * tw; j.y0 = ty * th;
            j.x1 = j.x0 + tw; j.y1 = j.y0 + th;
            if (j.x1 > p->width) j.x1 = p->width;
            if (j.y1 > p->height) j.y1 = p->height;
            j.rng_state = xorshift(&master);
            j.spp = p->spp;
            if (j.x0 >= p->x0 && j.y0 >= p->y0 && j.x1 <= p->x1 && j.y1 <= p->y1 && j.x0 < j.x1 && j.y0 < j.y1)
                jobs->push_back(j);
        }
}

/* one camera render on the device: out_rgb and the adaptive render's three other planes as the call's form has them */
int run_render(ort_scene *scene, const ort_render_params *p, const ort::RenderCall &c, void *out_rgb, void *out_spp = nullptr, void *out_m2 = nullptr,
               void *states = nullptr) {
    std::string err;
    const int rc = ort::device_render(scene, p, c, out_rgb, out_spp, out_m2, states, &err);
    return rc == ORT_OK ? ORT_OK : fail(rc, err);
}

/* out: the caller's memory (host) or a device pointer */
int render_common(ort_scene *scene, const ort_render_params *p, bool host, void *out, void *stream, ort_stats *stats) {
    int rc = check_params(scene, p);
    if (rc != ORT_OK) return rc;
    std::vector<ort_tile_job> jobs;
    if (p->policy == ORT_POLICY_TILE32 || p->policy == ORT_POLICY_WHOLE) {
        if (p->policy == ORT_POLICY_TILE32) {
            tile32_jobs(p, &jobs);
        } else {
            uint32_t master = p->seed;
            ort_tile_job j{p->x0, p->y0, p->x1, p->y1, xorshift(&master), p->spp};
            jobs.push_back(j);
        }
        if (jobs.empty()) return ORT_OK;
    }
    ort::RenderCall c{host, stream, stats}; /* the fields not named stay null / zero: no jobs, the scene's camera, no stopping rule */
    if (!jobs.empty()) { c.jobs = jobs.data(); c.job_count = (uint32_t)jobs.size(); }
    return run_render(scene, p, c, out);
}

template <typename T>
int copy_out(const std::vector<T> &v, T *out, uint32_t cap) {
    if (v.size() > cap || (!out && !v.empty())) return fail(ORT_ERR_INVALID, "output capacity too small");
    if (!v.empty()) memcpy(out, v.data(), v.size() * sizeof(T));
    return ORT_OK;
}

} // namespace


/* No exception crosses the C boundary: an allocation failure on hostile input (or anything else the C++ side
   throws) becomes an error code with a message instead of std::terminate under the caller's feet. */
template <typename F>
int guarded(F f) {
    try {
        return f();
    } catch (const std::bad_alloc &) {
        return fail(ORT_ERR_NO_MEMORY, "out of memory");
    } catch (const std::exception &e) {
        return fail(ORT_ERR_INTERNAL, std::string("internal error: ") + e.what());
    } catch (...) {
        return fail(ORT_ERR_INTERNAL, "internal error");
    }
}

extern "C" {

const char *ort_last_error(void) { return g_error.c_str(); }
static int ort_abi_version_impl(void) { return ORT_ABI_VERSION; }

static int ort_scene_parse_scn_impl(const char *text, size_t size, const char *base_dir, ort_scene **out) {
    if (!text || !out) return fail(ORT_ERR_INVALID, "null argument");
    *out = nullptr;
    std::unique_ptr<ort_scene> s(new (std::nothrow) ort_scene()); /* owned here until handed out: the parser may throw (bad_alloc on hostile input) */
    if (!s) return fail(ORT_ERR_NO_MEMORY, "out of memory");
    std::string err;
    int rc = ort::parse_scn_text(text, size, base_dir, s.get(), &err);
    if (rc != ORT_OK) return fail(rc, err);
    s->reference_csg = true; /* as main() does for every scene it loads (macos_main.mm:322-332) */
    *out = s.release();
    return ORT_OK;
}

static int ort_scene_load_scn_impl(const char *scn_path, const char *base_dir, ort_scene **out) {
    if (!scn_path || !out) return fail(ORT_ERR_INVALID, "null argument");
    std::vector<char> text;
    if (ort::read_file(scn_path, &text) != ORT_OK) return fail(ORT_ERR_IO, std::string("cannot read ") + scn_path);
    return ort_scene_parse_scn_impl(text.data(), text.size(), base_dir, out);
}

static int ort_scene_create_impl(const ort_scene_desc *d, ort_scene **out) {
    if (!d || !out) return fail(ORT_ERR_INVALID, "null argument");
    *out = nullptr;
    if (d->material_count == 0) return fail(ORT_ERR_INVALID, "material 0 (the reserved no-hit material) is required");
    ort_scene *s = new (std::nothrow) ort_scene();
    if (!s) return fail(ORT_ERR_NO_MEMORY, "out of memory");
    s->materials.assign(d->materials, d->materials + d->material_count);
    if (d->sphere_count) s->spheres.assign(d->spheres, d->spheres + d->sphere_count);
    if (d->box_count) s->boxes.assign(d->boxes, d->boxes + d->box_count);
    if (d->cylinder_count) s->cylinders.assign(d->cylinders, d->cylinders + d->cylinder_count);
    if (d->light_count) s->lights.assign(d->lights, d->lights + d->light_count);
    auto bad_mat = [&](uint32_t m) { return m >= d->material_count; };
    bool bad = false;
    for (auto &x : s->spheres) bad |= bad_mat(x.mat);
    for (auto &x : s->boxes) bad |= bad_mat(x.mat);
    for (auto &x : s->cylinders) bad |= bad_mat(x.mat);
    for (auto &l : s->lights) {
        if (l.type == 1u) bad |= (l.index >= d->sphere_count);
        else if (l.type == 2u) bad |= (l.index >= d->cylinder_count);
        else bad = true;
    }
    for (uint32_t i = 0; i < d->mesh_count && !bad; ++i) {
        const ort_mesh &m = d->meshes[i];
        ort::HostMesh hm;
        hm.vertices.assign(m.vertices, m.vertices + 3 * (size_t)m.vertex_count);
        hm.indices.assign(m.indices, m.indices + m.index_count);
        hm.mat = m.mat;
        hm.aabb_min = m.aabb_min;
        hm.aabb_max = m.aabb_max;
        bad |= bad_mat(m.mat);
        for (uint32_t ix : hm.indices) bad |= (ix >= m.vertex_count);
        s->meshes.push_back(std::move(hm));
    }
    if (bad) {
        delete s;
        return fail(ORT_ERR_INVALID, "material, light or vertex index out of range");
    }
    s->ambient = d->ambient;
    s->camera_p = d->camera_p;
    memcpy(s->camera_quat, d->camera_quat_xyzw, sizeof(s->camera_quat));
    s->camera_height_ratio = d->camera_height_ratio;
    s->screen_width = d->screen_width;
    s->screen_height = d->screen_height;
    s->reference_csg = d->with_reference_csg != 0;
    *out = s;
    return ORT_OK;
}

void ort_scene_destroy(ort_scene *scene) {
    if (!scene) return;
    ort::device_release(scene);
    delete scene;
}

static int ort_scene_get_info_impl(const ort_scene *s, ort_scene_info *out) {
    if (!s || !out) return fail(ORT_ERR_INVALID, "null argument");
    memset(out, 0, sizeof(*out));
    out->material_count = (uint32_t)s->materials.size();
    out->sphere_count = (uint32_t)s->spheres.size();
    out->box_count = (uint32_t)s->boxes.size();
    out->cylinder_count = (uint32_t)s->cylinders.size();
    out->mesh_count = (uint32_t)s->meshes.size();
    out->light_count = (uint32_t)s->lights.size();
    for (const auto &m : s->meshes) out->triangle_count += (uint32_t)(m.indices.size() / 3);
    out->screen_width = s->screen_width;
    out->screen_height = s->screen_height;
    out->ambient = s->ambient;
    out->camera_p = s->camera_p;
    memcpy(out->camera_quat_xyzw, s->camera_quat, sizeof(s->camera_quat));
    out->camera_height_ratio = s->camera_height_ratio;
    return ORT_OK;
}

static int ort_scene_get_materials_impl(const ort_scene *s, ort_material *out, uint32_t cap) { return s ? copy_out(s->materials, out, cap) : fail(ORT_ERR_INVALID, "null scene"); }
static int ort_scene_get_spheres_impl(const ort_scene *s, ort_sphere *out, uint32_t cap) { return s ? copy_out(s->spheres, out, cap) : fail(ORT_ERR_INVALID, "null scene"); }
static int ort_scene_get_boxes_impl(const ort_scene *s, ort_box *out, uint32_t cap) { return s ? copy_out(s->boxes, out, cap) : fail(ORT_ERR_INVALID, "null scene"); }
static int ort_scene_get_cylinders_impl(const ort_scene *s, ort_cylinder *out, uint32_t cap) { return s ? copy_out(s->cylinders, out, cap) : fail(ORT_ERR_INVALID, "null scene"); }
static int ort_scene_get_lights_impl(const ort_scene *s, ort_light *out, uint32_t cap) { return s ? copy_out(s->lights, out, cap) : fail(ORT_ERR_INVALID, "null scene"); }

static int ort_scene_get_mesh_impl(const ort_scene *s, uint32_t i, ort_mesh *out) {
    if (!s || !out) return fail(ORT_ERR_INVALID, "null argument");
    if (i >= s->meshes.size()) return fail(ORT_ERR_INVALID, "mesh index out of range");
    const ort::HostMesh &m = s->meshes[i];
    out->vertices = m.vertices.data();
    out->vertex_count = (uint32_t)(m.vertices.size() / 3);
    out->indices = m.indices.data();
    out->index_count = (uint32_t)m.indices.size();
    out->mat = m.mat;
    out->aabb_min = m.aabb_min;
    out->aabb_max = m.aabb_max;
    return ORT_OK;
}

static int ort_scene_get_camera_impl(const ort_scene *s, int32_t width, int32_t height, ort_camera *out) {
    if (!s || !out || width <= 0 || height <= 0) return fail(ORT_ERR_INVALID, "bad argument");
    ort::camera_basis(*s, width, height, out);
    return ORT_OK;
}

static int ort_scene_commit_impl(ort_scene *s) {
    if (!s) return fail(ORT_ERR_INVALID, "null scene");
    std::string err;
    int rc = ort::build_tree(s, &err);
    if (rc == ORT_OK) rc = ort::build_ref_tree(s, &err);
    return rc == ORT_OK ? ORT_OK : fail(rc, err);
}

static int ort_scene_get_tree_info_impl(const ort_scene *s, ort_tree_info *out) {
    if (!s || !out) return fail(ORT_ERR_INVALID, "null argument");
    if (!s->tree.built) return fail(ORT_ERR_STATE, "ort_scene_commit has not been called");
    const ort::Tree &t = s->tree;
    memset(out, 0, sizeof(*out));
    out->node_count = (uint32_t)t.nodes.size();
    out->leaf_count = t.leaf_count;
    out->max_leaf_prims = t.max_leaf_prims;
    out->max_depth = t.max_depth;
    out->node_bytes = t.nodes.size() * sizeof(ort::DevNode);
    out->prim_bytes = t.tris.size() * (sizeof(ort::DevTri) + 4) + t.spheres.size() * (sizeof(ort::DevSphere) + 4) +
                      t.boxes.size() * (sizeof(ort::DevBox) + 4) + t.cyls.size() * (sizeof(ort::DevCyl) + 4);
    out->sah_cost = t.sah_cost;
    const ort::RefTree &r = s->ref;
    out->ref_node_count = (uint32_t)r.nodes.size();
    out->ref_nonempty_leaves = r.nonempty_leaves;
    out->ref_max_leaf_records = r.max_leaf_records;
    out->ref_bytes = r.nodes.size() * sizeof(ort::DevRefNode) + r.recs.size() * 4 + r.chain_boxes.size() * 16 +
                     (r.tri_chain.size() + r.sphere_chain.size() + r.box_chain.size() + r.cyl_chain.size()) * 8;
    out->prologue_prims = t.pro_boxes + t.pro_spheres + t.pro_cyls;
    out->wide_node_count = (uint32_t)t.nodes4.size();
    out->wide_max_depth = t.max_depth4;
    return ORT_OK;
}

static int ort_device_count_impl(int *count) {
    if (!count) return fail(ORT_ERR_INVALID, "null argument");
    std::string err;
    int rc = ort::device_count(count, &err);
    return rc == ORT_OK ? ORT_OK : fail(rc, err);
}

static int ort_scene_upload_impl(ort_scene *s, int device) {
    if (!s) return fail(ORT_ERR_INVALID, "null scene");
    if (!s->tree.built) return fail(ORT_ERR_STATE, "ort_scene_commit has not been called");
    std::string err;
    int rc = ort::device_upload(s, device, &err);
    return rc == ORT_OK ? ORT_OK : fail(rc, err);
}

static int ort_tiled_raytrace_batch_impl(ort_scene *s, float *out_rgb, int32_t width, int32_t height, const ort_tile_job *jobs,
                             uint32_t job_count, float rr, uint32_t *final_states, ort_stats *stats) {
    if (!s || !out_rgb || (!jobs && job_count)) return fail(ORT_ERR_INVALID, "null argument");
    ort_render_params p{};
    p.width = width; p.height = height;
    p.x0 = 0; p.y0 = 0; p.x1 = width; p.y1 = height;
    p.policy = ORT_POLICY_WHOLE;
    p.spp = 1; p.rr = rr;
    if (stats) p.flags = ORT_RENDER_COUNTERS;
    int rc = check_params(s, &p);
    if (rc != ORT_OK) return rc;
    for (uint32_t i = 0; i < job_count; ++i) {
        const ort_tile_job &j = jobs[i];
        if (j.x0 < 0 || j.y0 < 0 || j.x1 > width || j.y1 > height) return fail(ORT_ERR_INVALID, "job rect outside the image");
        if (j.spp == 0) return fail(ORT_ERR_INVALID, "job spp must be >= 1");
    }
    if (job_count == 0) return ORT_OK;
    ort::RenderCall c{true, nullptr, stats};
    c.jobs = jobs; c.job_count = job_count; c.job_states = final_states;
    return run_render(s, &p, c, out_rgb);
}

static int ort_tiled_raytrace_impl(ort_scene *s, float *out_rgb, int32_t width, int32_t height, int32_t x0, int32_t y0, int32_t x1,
                       int32_t y1, uint32_t *rng_state, uint32_t spp, float rr, uint64_t *shape_tests) {
    if (!rng_state) return fail(ORT_ERR_INVALID, "null rng_state");
    ort_tile_job j{x0, y0, x1, y1, *rng_state, spp};
    uint32_t final_state = *rng_state;
    ort_stats st{};
    int rc = ort_tiled_raytrace_batch_impl(s, out_rgb, width, height, &j, 1, rr, &final_state, &st);
    if (rc != ORT_OK) return rc;
    *rng_state = final_state;
    if (shape_tests) *shape_tests = st.tri_tests + st.analytic_tests;
    return ORT_OK;
}

static int ort_render_image_impl(ort_scene *s, const ort_render_params *p, float *out_rgb, ort_stats *stats) {
    if (!out_rgb) return fail(ORT_ERR_INVALID, "null framebuffer");
    return render_common(s, p, true, out_rgb, nullptr, stats);
}

static int ort_render_image_device_impl(ort_scene *s, const ort_render_params *p, void *d_out_rgb, void *hip_stream, ort_stats *stats) {
    if (!d_out_rgb) return fail(ORT_ERR_INVALID, "null device framebuffer");
    return render_common(s, p, false, d_out_rgb, hip_stream, stats);
}

static int ort_unit_eval_device_impl(int device, const void *records, uint32_t count, float *out) {
    if ((!records || !out) && count) return fail(ORT_ERR_INVALID, "null argument");
    /* op 4 (cylinder): the kernel consumes the host-precomputed frame; fill it in a copy */
    std::vector<unsigned char> copy((const unsigned char *)records, (const unsigned char *)records + (size_t)count * 100u);
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t op;
        float a[24];
        memcpy(&op, &copy[(size_t)i * 100u], 4);
        if (op != 4u) continue;
        memcpy(a, &copy[(size_t)i * 100u + 4], 96);
        ort_cylinder c{{a[0], a[1], a[2]}, {a[3], a[4], a[5]}, a[6], 0};
        ort::cylinder_frame_for(c, a + 13, a + 22);
        memcpy(&copy[(size_t)i * 100u + 4], a, 96);
    }
    std::string err;
    int rc = ort::device_unit_eval(device, copy.data(), count, out, &err);
    return rc == ORT_OK ? ORT_OK : fail(rc, err);
}

/* The ray queries.  Each call has a host form (the caller's memory, staged in slices) and a device form (device pointers,
   enqueued on the caller's stream); both pass each array once, and the QueryCall says which form it is.  The order of the
   checks is each call's contract (include/ort.h). */
/* one pointer argument: whether the call needs it, and the alignment it must have (8, 4 or 1: none) */
struct PtrArg {
    const void *p;
    bool required;
    unsigned align;
};

/* a required pointer that is null, then a pointer that is not 8-byte aligned, then one that is not 4-byte aligned */
static int check_ptrs(std::initializer_list<PtrArg> args, const char *null_msg, const char *align8_msg, const char *align4_msg) {
    for (const PtrArg &a : args)
        if (a.required && !a.p) return fail(ORT_ERR_INVALID, null_msg);
    for (unsigned align : {8u, 4u})
        for (const PtrArg &a : args)
            if (a.align == align && ((uintptr_t)a.p & (align - 1u))) return fail(ORT_ERR_INVALID, align == 8u ? align8_msg : align4_msg);
    return ORT_OK;
}

/* closest hits: argument and state errors first, so that they are the same on a machine without a device; then count == 0 */
static int raycast_common(ort_scene *s, const ort::QueryCall &q, const void *rays, void *hits) {
    if (!s) return fail(ORT_ERR_INVALID, "null scene");
    int rc = q.count ? check_ptrs({{rays, true, 8}, {hits, true, 8}}, "null rays or hits", "rays and hits must be 8-byte aligned", "") : ORT_OK;
    if (rc != ORT_OK || (rc = check_resident(s)) != ORT_OK) return rc;
    if (q.count == 0) return nothing_to_do(q.stats);
    std::string err;
    rc = ort::device_raycast(s, q, rays, hits, &err);
    return rc == ORT_OK ? ORT_OK : fail(rc, err);
}

/* occlusion queries: count == 0 is OK whatever else is passed; then argument errors, then state errors */
static int occluded_common(ort_scene *s, const ort::QueryCall &q, const void *rays, const void *tmax, void *out) {
    if (q.count == 0) return nothing_to_do(q.stats);
    if (!s) return fail(ORT_ERR_INVALID, "null scene");
    int rc = check_ptrs({{rays, true, 8}, {tmax, false, 4}, {out, true, 1}}, "null rays or occluded", "rays must be 8-byte aligned", "tmax must be 4-byte aligned");
    if (rc != ORT_OK || (rc = check_resident(s)) != ORT_OK) return rc;
    std::string err;
    rc = ort::device_occluded(s, q, rays, tmax, out, &err);
    return rc == ORT_OK ? ORT_OK : fail(rc, err);
}

/* ambient-occlusion queries: count == 0 is OK whatever else is passed; then argument errors, then state errors */
static int ao_common(ort_scene *s, const ort::QueryCall &q, const void *points, const void *seeds, const void *radius, uint32_t spp, void *out_open,
                     void *out_bent, void *final_states) {
    if (q.count == 0) return nothing_to_do(q.stats);
    if (!s) return fail(ORT_ERR_INVALID, "null scene");
    int rc = check_ptrs({{points, true, 8}, {seeds, true, 4}, {radius, false, 4}, {out_open, true, 4}, {out_bent, false, 4}, {final_states, false, 4}},
                        "null points, seeds or out_open", "points must be 8-byte aligned", "seeds, radius, out_open, out_bent and final_states must be 4-byte aligned");
    if (rc != ORT_OK) return rc;
    if (spp == 0) return fail(ORT_ERR_INVALID, "spp must be >= 1");
    if ((rc = check_resident(s)) != ORT_OK) return rc;
    std::string err;
    rc = ort::device_ambient_occlusion(s, q, points, seeds, radius, spp, out_open, out_bent, final_states, &err);
    return rc == ORT_OK ? ORT_OK : fail(rc, err);
}

/* the stopping rule's parameters by themselves */
static int check_adaptive(const ort_adaptive *ad) {
    if (!ad) return fail(ORT_ERR_INVALID, "null ad (the adaptive parameters)");
    if (ad->min_spp < 2u) return fail(ORT_ERR_INVALID, "min_spp must be >= 2: a variance needs two samples");
    if (ad->max_spp < ad->min_spp) return fail(ORT_ERR_INVALID, "max_spp must be >= min_spp");
    if (ad->max_spp > (1u << 24)) return fail(ORT_ERR_INVALID, "max_spp must be <= 1 << 24: a sample count must be exact in float");
    if (ad->check_every == 0u) return fail(ORT_ERR_INVALID, "check_every must be >= 1");
    if (!(ad->tolerance >= 0.0f && ad->tolerance <= FLT_MAX)) return fail(ORT_ERR_INVALID, "tolerance must be finite and >= 0");
    if (!(ad->floor >= 0.0f && ad->floor <= FLT_MAX)) return fail(ORT_ERR_INVALID, "floor must be finite and >= 0");
    return ORT_OK;
}

/* radiance queries: count == 0 is OK whatever else is passed; then argument errors, then state errors.  adaptive: the same
   call with the stopping rule's parameters (ad, checked after the pointers) where spp stands, and out_spp and out_m2.  points: the
   irradiance queries -- the same call with points (p, n) where the rays stand, the same checks in the same order.  sh: the SH
   light-probe query (points, not adaptive) -- out_sh is the required output in out_rgb's place, and out_rgb is optional */
static int radiance_common(ort_scene *s, const ort::QueryCall &q, const void *rays, const void *seeds, uint32_t spp, float rr, bool adaptive,
                           const ort_adaptive *ad, void *out_rgb, void *out_spp, void *out_m2, void *final_states, bool points = false, bool sh = false,
                           void *out_sh = nullptr) {
    if (q.count == 0) return nothing_to_do(q.stats);
    if (!s) return fail(ORT_ERR_INVALID, "null scene");
    int rc = sh ? check_ptrs({{rays, true, 8}, {seeds, true, 4}, {out_sh, true, 4}, {out_rgb, false, 4}, {final_states, false, 4}}, "null points, seeds or out_sh",
                             "points must be 8-byte aligned", "seeds, out_sh, out_rgb and final_states must be 4-byte aligned")
                : check_ptrs({{rays, true, 8}, {seeds, true, 4}, {out_rgb, true, 4}, {out_spp, false, 4}, {out_m2, false, 4}, {final_states, false, 4}},
                        points ? "null points, seeds or out_rgb" : "null rays, seeds or out_rgb", points ? "points must be 8-byte aligned" : "rays must be 8-byte aligned",
                        adaptive ? "seeds, out_rgb, out_spp, out_m2 and final_states must be 4-byte aligned" : "seeds, out_rgb and final_states must be 4-byte aligned");
    if (rc != ORT_OK) return rc;
    if (adaptive && (rc = check_adaptive(ad)) != ORT_OK) return rc;
    if (!adaptive && spp == 0) return fail(ORT_ERR_INVALID, "spp must be >= 1");
    if (!(rr >= 0.0f && rr < 1.0f)) return fail(ORT_ERR_INVALID, "rr must be in [0, 1): at 1 a path in a closed room never ends");
    if ((rc = check_resident(s)) != ORT_OK) return rc;
    std::string err;
    rc = ort::device_radiance(s, q, rays, seeds, spp, rr, adaptive ? ad : nullptr, out_rgb, out_spp, out_m2, final_states, points, sh ? out_sh : nullptr, &err);
    return rc == ORT_OK ? ORT_OK : fail(rc, err);
}

/* ---- a batch of views ---- */
static int ort_camera_from_pose_impl(const float *p, const float *quat_xyzw, float height_ratio, int32_t width, int32_t height, ort_camera *out) {
    if (!p || !quat_xyzw || !out || width <= 0 || height <= 0) return fail(ORT_ERR_INVALID, "bad argument");
    ort::camera_from_pose(ort_v3{p[0], p[1], p[2]}, quat_xyzw, height_ratio, width, height, out);
    return ORT_OK;
}

/* Where a camera may stand: camera rays start on the aperture (ray.cpp:1233-1239: p + 0.1 cos(a) x + 0.1 sin(a) y - 0.1 z), and the
   fast tree answers for origins within the scene's box grown by the 0.25 per side build_tree allows (scene_origin_box).  The
   aperture's bounding box must lie inside it; a non-finite component fails every comparison. */
static bool view_in_box(const ort_camera &c, const float lo[3], const float hi[3]) {
    const float p[3] = {c.p.x, c.p.y, c.p.z}, x[3] = {c.x_axis.x, c.x_axis.y, c.x_axis.z}, y[3] = {c.y_axis.x, c.y_axis.y, c.y_axis.z},
                z[3] = {c.z_axis.x, c.z_axis.y, c.z_axis.z};
    for (int k = 0; k < 3; ++k) {
        const float mid = p[k] - 0.1f * z[k], ext = 0.1f * fabsf(x[k]) + 0.1f * fabsf(y[k]);
        const float a = mid - ext, b = mid + ext;
        if (!(fabsf(a) <= 3.0e38f) || !(fabsf(b) <= 3.0e38f)) return false;
        if (!(a >= lo[k] - 0.25f) || !(b <= hi[k] + 0.25f)) return false;
    }
    return true;
}

/* every view's aperture lies in the scene's box */
static int check_views_in_box(const ort_scene *s, const ort_view *views, uint32_t view_count) {
    float lo[3], hi[3];
    ort::scene_origin_box(*s, lo, hi);
    for (uint32_t v = 0; v < view_count; ++v)
        if (!view_in_box(views[v].camera, lo, hi))
            return fail(ORT_ERR_UNSUPPORTED, "view " + std::to_string(v) + ": the camera's aperture is not finite or leaves the box of the scene's shapes and its own "
                                             "camera_p (+ 0.25 per side) that the tree was built for; create the scene with a camera_p out there");
    return ORT_OK;
}

static int check_view_cap(uint32_t view_count) {
    static_assert(sizeof(ort_view) == 52, "ort_view is a camera and a seed");
    if (view_count > ORT_MAX_VIEWS) return fail(ORT_ERR_INVALID, "more than ORT_MAX_VIEWS (4096) views in one call");
    return ORT_OK;
}

/* no call that takes views renders a shard of a frame or into a packed framebuffer; each says so in its own words */
static int refuse_shards_and_packed(const ort_render_params &p, const char *sharded, const char *packed) {
    if (p.shard_count > 1) return fail(ORT_ERR_UNSUPPORTED, sharded);
    if (p.flags & ORT_RENDER_PACKED) return fail(ORT_ERR_UNSUPPORTED, packed);
    return ORT_OK;
}

/* view_count == 0 is OK whatever else is passed; then argument errors, what the call does not do, and the scene's state.  Always a
   batch, so there is no own-view form here; unlike the pixel-job renders below it allows CHUNK */
static int render_views_common(ort_scene *s, const ort_render_params *p, const ort_view *views, uint32_t view_count, bool host, void *out,
                               void *stream, ort_stats *stats) {
    if (view_count == 0) return nothing_to_do(stats);
    if (!views || !out) return fail(ORT_ERR_INVALID, "null views or framebuffer");
    int rc = check_view_cap(view_count);
    if (rc != ORT_OK || (rc = check_param_values(s, p)) != ORT_OK) return rc;
    if (p->policy != ORT_POLICY_PIXEL && p->policy != ORT_POLICY_CHUNK)
        return fail(ORT_ERR_UNSUPPORTED, "a batch of views needs a per-pixel seeding policy (PIXEL or CHUNK)");
    rc = refuse_shards_and_packed(*p, "a batch of views is not sharded: deal views to GPUs, not blocks", "a batch of views has no packed framebuffer");
    if (rc != ORT_OK || (rc = check_views_in_box(s, views, view_count)) != ORT_OK || (rc = check_resident(s)) != ORT_OK) return rc;
    ort::RenderCall c{host, stream, stats};
    c.views = views; c.view_count = view_count;
    return run_render(s, p, c, out);
}

/* The camera renders that cut one-pixel jobs -- adaptive, light groups, sample map, first-hit features -- each one frame or a batch
   of views, host or device form.  A kind is the words of its three refusals and four steps of its own; the order of the checks,
   which is every one of these calls' contract (include/ort.h), is this function:
     1. view_count == 0 is OK whatever else is passed (the views form);
     2. the kind's null arguments (nulls), the view cap, a null scene or params;
     3. the params as the render call judges them, after the kind has overwritten what is not the caller's to set here (adjust;
        chunk never is: one job per pixel);
     4. the kind's own argument checks (checks);
     5. what the call does not do: any policy but PIXEL, shards, packed planes, a camera outside the scene's box;
     6. the scene's state; then the launch (launch), with the params as adjusted and a RenderCall that holds the form and the views.
   !batch is the single-frame form: views is not read, and the call renders the one-view batch of the scene's own camera and
   params->seed. */
struct PixelJobKind {
    const char *not_pixel, *sharded, *packed;
};

extern "C++" { /* a template, in the middle of the C entry points */
template <typename Nulls, typename Adjust, typename Checks, typename Launch>
static int render_pixel_jobs(const PixelJobKind &kind, ort_scene *s, const ort_render_params *p, const ort_view *views, uint32_t view_count, bool batch,
                             bool host, void *stream, ort_stats *stats, Nulls nulls, Adjust adjust, Checks checks, Launch launch) {
    if (batch && view_count == 0) return nothing_to_do(stats);
    int rc = nulls();
    if (rc != ORT_OK || (rc = check_view_cap(view_count)) != ORT_OK) return rc;
    if (!s || !p) return fail(ORT_ERR_INVALID, "null scene or params");
    ort_render_params q = *p;
    adjust(&q);
    q.chunk = q.spp;
    if ((rc = check_param_values(s, &q)) != ORT_OK || (rc = checks(q)) != ORT_OK) return rc;
    if (q.policy != ORT_POLICY_PIXEL) return fail(ORT_ERR_UNSUPPORTED, kind.not_pixel);
    if ((rc = refuse_shards_and_packed(q, kind.sharded, kind.packed)) != ORT_OK) return rc;
    ort_view own;
    if (batch) {
        if ((rc = check_views_in_box(s, views, view_count)) != ORT_OK) return rc;
    } else {
        ort::camera_basis(*s, q.width, q.height, &own.camera);
        own.seed = q.seed;
        views = &own;
    }
    if ((rc = check_resident(s)) != ORT_OK) return rc;
    ort::RenderCall c{host, stream, stats};
    c.views = views; c.view_count = view_count;
    return launch(q, c);
}
} // extern "C++"

/* the nulls of a kind whose first plane is required: the views or the plane (the views form), the plane by the form's name */
static int check_first_plane(bool batch, bool host, const ort_view *views, const void *plane, const char *in_batch, const char *in_host, const char *in_device) {
    if (!plane || (batch && !views)) return fail(ORT_ERR_INVALID, batch ? in_batch : host ? in_host : in_device);
    return ORT_OK;
}

/* The adaptive camera render: spp is not the caller's to set either -- the params are judged with ad->max_spp where it stands --
   and its own check is ad, as ort_radiance_adaptive judges it */
static int render_adaptive_common(ort_scene *s, const ort_render_params *p, const ort_adaptive *ad, const ort_view *views, uint32_t view_count, bool batch,
                                  bool host, void *out_rgb, void *out_spp, void *out_m2, void *states, void *stream, ort_stats *stats) {
    static const PixelJobKind kind = {"the adaptive render cuts one-pixel jobs: it needs the PIXEL policy", "the adaptive render is not sharded",
                                      "the adaptive render has no packed framebuffer"};
    return render_pixel_jobs(
        kind, s, p, views, view_count, batch, host, stream, stats,
        [&] { return check_first_plane(batch, host, views, out_rgb, "null views or framebuffer", "null framebuffer", "null device framebuffer"); },
        [&](ort_render_params *q) { q->spp = ad && ad->max_spp ? ad->max_spp : 1u; }, /* a null ad or a max_spp of 0 is check_adaptive's to name */
        [&](const ort_render_params &) { return check_adaptive(ad); },
        [&](const ort_render_params &q, ort::RenderCall c) { c.kind = ort::RK_ADAPTIVE; c.ad = ad; return run_render(s, &q, c, out_rgb, out_spp, out_m2, states); });
}

/* Light-group renders.  Own checks: spp above 1 << 24, the groups (a null struct or table, another material count than the scene's,
   a group count outside [1, ORT_MAX_LIGHT_GROUPS], a light's entry that names no group and is not ORT_NO_LIGHT_GROUP; other
   materials' entries are not read), the planes' alignment */
static int render_groups_common(ort_scene *s, const ort_render_params *p, const ort_light_groups *groups, const ort_view *views, uint32_t view_count,
                                bool batch, bool host, void *out_groups, void *out_rgb, void *states, void *stream, ort_stats *stats) {
    static const PixelJobKind kind = {"the light-group render splits one-pixel jobs: it needs the PIXEL policy", "the light-group render is not sharded",
                                      "the light-group render has no packed framebuffer"};
    return render_pixel_jobs(
        kind, s, p, views, view_count, batch, host, stream, stats,
        [&] { return check_first_plane(batch, host, views, out_groups, "null views or group frames", "null group frames", "null device group frames"); },
        [](ort_render_params *) {},
        [&](const ort_render_params &q) {
            if (q.spp > (1u << 24)) return fail(ORT_ERR_INVALID, "spp must be <= 1 << 24: a sample count must be exact in float");
            if (!groups) return fail(ORT_ERR_INVALID, "null groups (the light-group table)");
            if (!groups->group_of_material) return fail(ORT_ERR_INVALID, "null group_of_material");
            if (groups->material_count != s->materials.size()) return fail(ORT_ERR_INVALID, "groups->material_count is not the scene's material count");
            if (groups->group_count == 0 || groups->group_count > ORT_MAX_LIGHT_GROUPS) return fail(ORT_ERR_INVALID, "group_count must be within [1, ORT_MAX_LIGHT_GROUPS]");
            for (size_t m = 0; m < s->materials.size(); ++m)
                if (s->materials[m].is_light && groups->group_of_material[m] >= groups->group_count && groups->group_of_material[m] != ORT_NO_LIGHT_GROUP)
                    return fail(ORT_ERR_INVALID, "light material " + std::to_string(m) + ": its group is neither below group_count nor ORT_NO_LIGHT_GROUP");
            return check_ptrs({{out_groups, true, 4}, {out_rgb, false, 4}, {states, false, 4}}, "", "", "out_groups, out_rgb and final_states must be 4-byte aligned");
        },
        [&](const ort_render_params &q, ort::RenderCall c) {
            c.kind = ort::RK_GROUPS; c.groups = groups; c.out_groups = out_groups;
            return run_render(s, &q, c, out_rgb, nullptr, nullptr, states);
        });
}

/* Path-depth renders: render_groups_common's order with the bin count where the groups stand.  Own checks: spp above 1 << 24, a bin
   count outside [1, ORT_MAX_DEPTH_BINS], the planes' alignment */
static int render_depths_common(ort_scene *s, const ort_render_params *p, uint32_t bin_count, const ort_view *views, uint32_t view_count, bool batch, bool host,
                                void *out_bins, void *out_rgb, void *out_lengths, void *states, void *stream, ort_stats *stats) {
    static const PixelJobKind kind = {"the path-depth render splits one-pixel jobs: it needs the PIXEL policy", "the path-depth render is not sharded",
                                      "the path-depth render has no packed framebuffer"};
    return render_pixel_jobs(
        kind, s, p, views, view_count, batch, host, stream, stats,
        [&] { return check_first_plane(batch, host, views, out_bins, "null views or bin frames", "null bin frames", "null device bin frames"); },
        [](ort_render_params *) {},
        [&](const ort_render_params &q) {
            if (q.spp > (1u << 24)) return fail(ORT_ERR_INVALID, "spp must be <= 1 << 24: a sample count must be exact in float");
            if (bin_count == 0 || bin_count > ORT_MAX_DEPTH_BINS) return fail(ORT_ERR_INVALID, "bin_count must be within [1, ORT_MAX_DEPTH_BINS]");
            return check_ptrs({{out_bins, true, 4}, {out_rgb, false, 4}, {out_lengths, false, 4}, {states, false, 4}}, "", "",
                              "out_bins, out_rgb, out_lengths and final_states must be 4-byte aligned");
        },
        [&](const ort_render_params &q, ort::RenderCall c) {
            c.kind = ort::RK_DEPTHS; c.depth_bins = bin_count; c.out_groups = out_bins;
            return run_render(s, &q, c, out_rgb, out_lengths, nullptr, states);
        });
}

/* Sample-map renders.  Own checks: spp -- the cap -- above 1 << 24, a null map, the map's and the planes' alignment.  The map's
   VALUES are never judged, in any form: the device forms cannot see them before the launch, so the lanes cut every one at the cap */
static int render_sample_map_common(ort_scene *s, const ort_render_params *p, const ort_view *views, uint32_t view_count, bool batch, bool host,
                                    const void *sample_map, void *out_rgb, void *out_m2, void *states, void *stream, ort_stats *stats) {
    static const PixelJobKind kind = {"the sample-map render cuts one-pixel jobs: it needs the PIXEL policy", "the sample-map render is not sharded",
                                      "the sample-map render has no packed framebuffer"};
    return render_pixel_jobs(
        kind, s, p, views, view_count, batch, host, stream, stats,
        [&] { return check_first_plane(batch, host, views, out_rgb, "null views or framebuffer", "null framebuffer", "null device framebuffer"); },
        [](ort_render_params *) {},
        [&](const ort_render_params &q) {
            if (q.spp > (1u << 24)) return fail(ORT_ERR_INVALID, "spp (the cap on a pixel's samples) must be <= 1 << 24: a sample count must be exact in float");
            if (!sample_map) return fail(ORT_ERR_INVALID, host ? "null sample_map" : "null device sample_map");
            return check_ptrs({{sample_map, true, 4}, {out_rgb, true, 4}, {out_m2, false, 4}, {states, false, 4}}, "", "",
                              "sample_map, out_rgb, out_m2 and final_states must be 4-byte aligned");
        },
        [&](const ort_render_params &q, ort::RenderCall c) { c.kind = ort::RK_SAMPLE_MAP; c.sample_map = sample_map; return run_render(s, &q, c, out_rgb, nullptr, out_m2, states); });
}

/* Accumulating renders: render_sample_map_common's order with acc where the map stands.  Nulls: the views (the views form); no plane
   is required before the params are judged, out_rgb being optional.  Own checks: spp -- the cap on what one call adds -- above
   1 << 24, a null acc or a null sum_rgb, count or states plane in it, the alignment of every plane and of the map.  Neither the map's
   values nor the planes' are ever judged: the lanes cut every count and take every sum and state as it stands */
static int render_accumulate_common(ort_scene *s, const ort_render_params *p, const ort_view *views, uint32_t view_count, bool batch, bool host,
                                    const ort_accum_planes *acc, const void *sample_map, void *out_rgb, void *stream, ort_stats *stats) {
    static const PixelJobKind kind = {"the accumulating render continues one-pixel jobs: it needs the PIXEL policy", "the accumulating render is not sharded",
                                      "the accumulating render has no packed framebuffer"};
    return render_pixel_jobs(
        kind, s, p, views, view_count, batch, host, stream, stats,
        [&] { return batch && !views ? fail(ORT_ERR_INVALID, "null views") : ORT_OK; },
        [](ort_render_params *) {},
        [&](const ort_render_params &q) {
            if (q.spp > (1u << 24)) return fail(ORT_ERR_INVALID, "spp (the cap on the samples a call adds to a pixel) must be <= 1 << 24: a sample count must be exact in float");
            if (!acc) return fail(ORT_ERR_INVALID, "null acc (the accumulation planes)");
            if (!acc->sum_rgb || !acc->count || !acc->states) return fail(ORT_ERR_INVALID, host ? "null sum_rgb, count or states plane" : "null device sum_rgb, count or states plane");
            return check_ptrs({{acc->sum_rgb, true, 4}, {acc->m2, false, 4}, {acc->count, true, 4}, {acc->states, true, 4}, {sample_map, false, 4}, {out_rgb, false, 4}}, "", "",
                              "sum_rgb, m2, count, states, sample_map and out_rgb must be 4-byte aligned");
        },
        [&](const ort_render_params &q, ort::RenderCall c) {
            c.kind = ort::RK_ACCUMULATE; c.sample_map = sample_map; c.acc_sum = acc->sum_rgb;
            return run_render(s, &q, c, out_rgb, acc->count, acc->m2, acc->states);
        });
}

/* First-hit feature renders.  Nulls: the planes struct, all five feature planes, the views.  rr is not the caller's to set either.  Own
   checks: spp above 1 << 24, the planes' alignment.  The launch is device_render_features, not run_render */
static int render_features_common(ort_scene *s, const ort_render_params *p, const ort_view *views, uint32_t view_count, bool batch, bool host,
                                  const ort_feature_planes *planes, void *stream, ort_stats *stats) {
    static const PixelJobKind kind = {"the feature render cuts one-pixel jobs: it needs the PIXEL policy", "the feature render is not sharded",
                                      "the feature render has no packed planes"};
    return render_pixel_jobs(
        kind, s, p, views, view_count, batch, host, stream, stats,
        [&] {
            if (!planes) return fail(ORT_ERR_INVALID, "null planes");
            if (!planes->albedo && !planes->normal && !planes->depth && !planes->hits && !planes->ids)
                return fail(ORT_ERR_INVALID, "no feature plane is asked for: albedo, normal, depth, hits and ids are all null");
            return batch && !views ? fail(ORT_ERR_INVALID, "null views") : ORT_OK;
        },
        [](ort_render_params *q) { q->rr = 0.0f; },
        [&](const ort_render_params &q) {
            if (q.spp > (1u << 24)) return fail(ORT_ERR_INVALID, "spp must be <= 1 << 24: a sample count must be exact in float");
            return check_ptrs({{planes->albedo, false, 4}, {planes->normal, false, 4}, {planes->depth, false, 4}, {planes->hits, false, 4}, {planes->ids, false, 4},
                               {planes->final_states, false, 4}}, "", "", "albedo, normal, depth, hits, ids and final_states must be 4-byte aligned");
        },
        [&](const ort_render_params &q, const ort::RenderCall &c) {
            std::string err;
            const int rc = ort::device_render_features(s, &q, c.views, c.view_count, {host, 0, q.flags, stream, stats}, *planes, &err);
            return rc == ORT_OK ? ORT_OK : fail(rc, err);
        });
}

/* Feature renders that follow mirrors and glass: render_features_common's order.  Nulls: the planes struct, all of the first six
   planes, the views.  rr IS the caller's here, judged with the params.  Own checks: spp above 1 << 24, max_bounces above
   ORT_MAX_FOLLOW_BOUNCES, the planes' alignment.  The launch is device_render_follow */
static int render_follow_common(ort_scene *s, const ort_render_params *p, const ort_view *views, uint32_t view_count, bool batch, bool host,
                                uint32_t max_bounces, const ort_follow_planes *planes, void *stream, ort_stats *stats) {
    static const PixelJobKind kind = {"the follow render cuts one-pixel jobs: it needs the PIXEL policy", "the follow render is not sharded",
                                      "the follow render has no packed planes"};
    return render_pixel_jobs(
        kind, s, p, views, view_count, batch, host, stream, stats,
        [&] {
            if (!planes) return fail(ORT_ERR_INVALID, "null planes");
            if (!planes->albedo && !planes->normal && !planes->depth && !planes->hits && !planes->ids && !planes->bounces)
                return fail(ORT_ERR_INVALID, "no plane is asked for: albedo, normal, depth, hits, ids and bounces are all null");
            return batch && !views ? fail(ORT_ERR_INVALID, "null views") : ORT_OK;
        },
        [](ort_render_params *) {},
        [&](const ort_render_params &q) {
            if (q.spp > (1u << 24)) return fail(ORT_ERR_INVALID, "spp must be <= 1 << 24: a sample count must be exact in float");
            if (max_bounces > ORT_MAX_FOLLOW_BOUNCES) return fail(ORT_ERR_INVALID, "max_bounces must be <= ORT_MAX_FOLLOW_BOUNCES");
            return check_ptrs({{planes->albedo, false, 4}, {planes->normal, false, 4}, {planes->depth, false, 4}, {planes->hits, false, 4}, {planes->ids, false, 4},
                               {planes->bounces, false, 4}, {planes->final_states, false, 4}}, "", "",
                              "albedo, normal, depth, hits, ids, bounces and final_states must be 4-byte aligned");
        },
        [&](const ort_render_params &q, const ort::RenderCall &c) {
            std::string err;
            const int rc = ort::device_render_follow(s, &q, c.views, c.view_count, max_bounces, {host, 0, q.flags, stream, stats}, *planes, &err);
            return rc == ORT_OK ? ORT_OK : fail(rc, err);
        });
}

/* ID-matte renders: render_features_common's order.  Nulls: the planes struct, the views; no plane is required before the params
   are judged.  rr is not the caller's to set, as there.  Own checks: spp above 1 << 24, the planes' alignment, then m, by, slots and
   the two required planes, in that order.  The launch is device_render_matte */
static int render_matte_common(ort_scene *s, const ort_render_params *p, const ort_view *views, uint32_t view_count, bool batch, bool host,
                               const ort_matte *m, const ort_matte_planes *planes, void *stream, ort_stats *stats) {
    static const PixelJobKind kind = {"the matte render cuts one-pixel jobs: it needs the PIXEL policy", "the matte render is not sharded",
                                      "the matte render has no packed planes"};
    return render_pixel_jobs(
        kind, s, p, views, view_count, batch, host, stream, stats,
        [&] {
            if (!planes) return fail(ORT_ERR_INVALID, "null planes");
            return batch && !views ? fail(ORT_ERR_INVALID, "null views") : ORT_OK;
        },
        [](ort_render_params *q) { q->rr = 0.0f; },
        [&](const ort_render_params &q) {
            if (q.spp > (1u << 24)) return fail(ORT_ERR_INVALID, "spp must be <= 1 << 24: a sample count must be exact in float");
            if (int rc = check_ptrs({{planes->ids, false, 4}, {planes->counts, false, 4}, {planes->other, false, 4}, {planes->hits, false, 4},
                                     {planes->final_states, false, 4}}, "", "", "ids, counts, other, hits and final_states must be 4-byte aligned"))
                return rc;
            if (!m) return fail(ORT_ERR_INVALID, "null m (the matte's mode and slots)");
            if (m->by > ORT_MATTE_BY_PRIM) return fail(ORT_ERR_INVALID, "by must be ORT_MATTE_BY_MATERIAL, ORT_MATTE_BY_OBJECT or ORT_MATTE_BY_PRIM");
            if (m->slots == 0 || m->slots > ORT_MAX_MATTE_SLOTS) return fail(ORT_ERR_INVALID, "slots must be within [1, ORT_MAX_MATTE_SLOTS]");
            if (!planes->ids || !planes->counts) return fail(ORT_ERR_INVALID, host ? "null ids or counts plane" : "null device ids or counts plane");
            return (int)ORT_OK;
        },
        [&](const ort_render_params &q, const ort::RenderCall &c) {
            std::string err;
            const int rc = ort::device_render_matte(s, &q, c.views, c.view_count, *m, {host, 0, q.flags, stream, stats}, *planes, &err);
            return rc == ORT_OK ? ORT_OK : fail(rc, err);
        });
}

/* ---- a mask from matte slots (ort_mattemask.h, device_matte_mask): no scene, the order of the checks is the call's contract (include/ort.h) ---- */
static int matte_mask_common(int device, bool host, const void *ids, const void *counts, uint32_t slots, uint32_t spp, const uint32_t *select, uint32_t select_count,
                             int32_t width, int32_t height, uint32_t frame_count, void *out_mask, void *hip_stream) {
    if (frame_count == 0) return ORT_OK;
    if (!ids || !counts || !select || !out_mask) return fail(ORT_ERR_INVALID, "null ids, counts, select or out_mask");
    for (const void *q : {ids, counts, (const void *)out_mask})
        if ((uintptr_t)q & 3u) return fail(ORT_ERR_INVALID, "ids, counts or out_mask not 4-byte aligned");
    if (slots == 0 || slots > ORT_MAX_MATTE_SLOTS) return fail(ORT_ERR_INVALID, "slots must be within [1, ORT_MAX_MATTE_SLOTS]");
    if (width < 1 || height < 1 || (uint64_t)frame_count * (uint64_t)width * (uint64_t)height * slots >= (1ull << 31)) return fail(ORT_ERR_INVALID, "bad frame size");
    if (spp < 1 || spp > (1u << 24)) return fail(ORT_ERR_INVALID, "spp must be within [1, 1 << 24]");
    if (select_count < 1 || select_count > ORT_MAX_MATTE_SELECT) return fail(ORT_ERR_INVALID, "select_count must be within [1, ORT_MAX_MATTE_SELECT]");
    for (uint32_t i = 0; i < select_count; ++i)
        if (select[i] == ORT_MATTE_EMPTY) return fail(ORT_ERR_INVALID, "ORT_MATTE_EMPTY in select");
    std::string err;
    int rc = ort::device_matte_mask(device, host, ids, counts, slots, spp, select, select_count, width, height, frame_count, out_mask, hip_stream, &err);
    return rc == ORT_OK ? ORT_OK : fail(rc, err);
}

static int ort_render_views_workspace_bytes_impl(const ort_render_params *p, uint32_t view_count, uint64_t *bytes) {
    if (!p || !bytes) return fail(ORT_ERR_INVALID, "null argument");
    *bytes = ort::render_views_workspace_bytes(p, view_count);
    return ORT_OK;
}

static int ort_render_workspace_bytes_impl(const ort_render_params *p, uint64_t *bytes) {
    if (!p || !bytes) return fail(ORT_ERR_INVALID, "null argument");
    *bytes = ort::render_workspace_bytes(p);
    return ORT_OK;
}


/* ---- multi-GPU (ort_comm.cpp) ---- */
static int ort_shard_block_count_impl(int32_t width, int32_t height, uint32_t shard_index, uint32_t shard_count, uint64_t *blocks) {
    if (!blocks || width <= 0 || height <= 0 || (shard_count > 1 && shard_index >= shard_count)) return fail(ORT_ERR_INVALID, "bad argument");
    *blocks = ort::comm_shard_blocks(width, height, shard_count > 1 ? shard_index : 0, shard_count > 1 ? shard_count : 1);
    return ORT_OK;
}
static int check_shard(const void *a, const void *b, int32_t w, int32_t h, uint32_t index, uint32_t count) {
    if (!a || !b || w <= 0 || h <= 0 || count == 0 || index >= count) return fail(ORT_ERR_INVALID, "bad argument");
    return ORT_OK;
}
static int ort_pack_blocks_host_impl(const float *full_rgb, int32_t width, int32_t height, uint32_t shard_index, uint32_t shard_count, float *packed) {
    int rc = check_shard(full_rgb, packed, width, height, shard_index, shard_count);
    if (rc == ORT_OK) ort::pack_blocks_host(full_rgb, width, height, shard_index, shard_count, packed);
    return rc;
}
static int ort_unpack_blocks_host_impl(const float *packed, int32_t width, int32_t height, uint32_t shard_index, uint32_t shard_count, float *full_rgb) {
    int rc = check_shard(full_rgb, packed, width, height, shard_index, shard_count);
    if (rc == ORT_OK) ort::unpack_blocks_host(packed, width, height, shard_index, shard_count, full_rgb);
    return rc;
}
static int ort_unpack_blocks_device_impl(const void *d_packed, int32_t width, int32_t height, uint32_t shard_index, uint32_t shard_count,
                                         void *d_full_rgb, void *hip_stream) {
    int rc = check_shard(d_full_rgb, d_packed, width, height, shard_index, shard_count);
    if (rc != ORT_OK) return rc;
    std::string err;
    rc = ort::unpack_blocks_device(d_packed, width, height, shard_index, shard_count, d_full_rgb, hip_stream, &err);
    return rc == ORT_OK ? ORT_OK : fail(rc, err);
}

/* ---- the denoiser (ort_denoise.h, device_denoise): no scene, the order of the checks is the call's contract (include/ort.h) ---- */
static int ort_denoise_workspace_bytes_impl(int32_t width, int32_t height, uint32_t frame_count, uint64_t *bytes) {
    if (!bytes) return fail(ORT_ERR_INVALID, "null argument");
    *bytes = 0;
    if (frame_count == 0) return ORT_OK;
    if (width < 1 || height < 1 || (uint64_t)frame_count * (uint64_t)width * (uint64_t)height >= (1ull << 31)) return fail(ORT_ERR_INVALID, "bad frame size");
    *bytes = 48ull * ((uint64_t)frame_count * (uint64_t)width * (uint64_t)height);
    return ORT_OK;
}
static int denoise_common(int device, bool host, const ort_denoise_params *p, const ort_denoise_planes *in, int32_t width, int32_t height, uint32_t frame_count,
                          void *out_rgb, void *workspace, uint64_t workspace_bytes, void *hip_stream, ort_stats *stats) {
    if (frame_count == 0) return ORT_OK;
    if (!p || !in) return fail(ORT_ERR_INVALID, "null params or planes struct");
    const void *ptrs[] = {in->rgb, in->m2, in->count, in->albedo, in->normal, in->depth, out_rgb};
    for (const void *q : ptrs)
        if (!q) return fail(ORT_ERR_INVALID, "null plane (all six planes and out_rgb are required)");
    for (const void *q : ptrs)
        if ((uintptr_t)q & 3u) return fail(ORT_ERR_INVALID, "plane not 4-byte aligned");
    if (width < 1 || height < 1 || (uint64_t)frame_count * (uint64_t)width * (uint64_t)height >= (1ull << 31)) return fail(ORT_ERR_INVALID, "bad frame size");
    if (p->iterations < 1 || p->iterations > 8) return fail(ORT_ERR_INVALID, "iterations must be within [1, 8]");
    if (p->normal_squarings > 8) return fail(ORT_ERR_INVALID, "normal_squarings must be at most 8");
    for (float sigma : {p->sigma_l, p->sigma_z})
        if (!(sigma > 0.0f) || !(sigma <= FLT_MAX)) return fail(ORT_ERR_INVALID, "sigma_l and sigma_z must be finite and > 0");
    if (!host) {
        const uint64_t need = 48ull * ((uint64_t)frame_count * (uint64_t)width * (uint64_t)height);
        if (!workspace || ((uintptr_t)workspace & 15u) || workspace_bytes < need) return fail(ORT_ERR_INVALID, "null, misaligned or short workspace (ort_denoise_workspace_bytes)");
    }
    std::string err;
    int rc = ort::device_denoise(device, host, *p, *in, width, height, frame_count, out_rgb, workspace, hip_stream, stats, &err);
    return rc == ORT_OK ? ORT_OK : fail(rc, err);
}
/* ---- the sample planner (ort_sampleplan.h, device_plan_samples): no scene, the order of the checks is the call's contract (include/ort.h) ---- */
static int ort_plan_samples_workspace_bytes_impl(int32_t width, int32_t height, uint32_t frame_count, uint64_t *bytes) {
    if (!bytes) return fail(ORT_ERR_INVALID, "null argument");
    *bytes = 0;
    if (frame_count == 0) return ORT_OK;
    if (width < 1 || height < 1 || (uint64_t)frame_count * (uint64_t)width * (uint64_t)height >= (1ull << 31)) return fail(ORT_ERR_INVALID, "bad frame size");
    *bytes = 4ull * ((uint64_t)frame_count * (uint64_t)width * (uint64_t)height);
    return ORT_OK;
}
static int plan_common(int device, bool host, const ort_plan_params *p, const ort_plan_planes *in, int32_t width, int32_t height, uint32_t frame_count,
                       void *sample_map, void *totals, void *workspace, uint64_t workspace_bytes, void *hip_stream, ort_stats *stats) {
    if (frame_count == 0) return ORT_OK;
    if (!p || !in) return fail(ORT_ERR_INVALID, "null params or planes struct");
    const void *ptrs[] = {in->rgb, in->m2, in->count, sample_map};
    for (const void *q : ptrs)
        if (!q) return fail(ORT_ERR_INVALID, "null plane (rgb, m2, count and sample_map are required)");
    if (!totals) return fail(ORT_ERR_INVALID, "null totals");
    for (const void *q : ptrs)
        if ((uintptr_t)q & 3u) return fail(ORT_ERR_INVALID, "plane or sample_map not 4-byte aligned");
    if ((uintptr_t)totals & 7u) return fail(ORT_ERR_INVALID, "totals not 8-byte aligned");
    if (width < 1 || height < 1 || (uint64_t)frame_count * (uint64_t)width * (uint64_t)height >= (1ull << 31)) return fail(ORT_ERR_INVALID, "bad frame size");
    if (!(p->tolerance > 0.0f) || !(p->tolerance <= FLT_MAX) || !(p->tolerance * p->tolerance > 0.0f)) return fail(ORT_ERR_INVALID, "tolerance must be finite and > 0, and so must its square");
    if (!(p->floor > 0.0f) || !(p->floor <= FLT_MAX)) return fail(ORT_ERR_INVALID, "floor must be finite and > 0");
    if (p->radius > 3) return fail(ORT_ERR_INVALID, "radius must be at most 3");
    if (p->min_add < 1) return fail(ORT_ERR_INVALID, "min_add must be at least 1");
    if (p->cap < 1 || p->cap > (1u << 24)) return fail(ORT_ERR_INVALID, "cap must be within [1, 1 << 24]");
    if (p->rgb_is_sum > 1) return fail(ORT_ERR_INVALID, "rgb_is_sum must be 0 or 1");
    if (p->reserved != 0) return fail(ORT_ERR_INVALID, "reserved must be 0");
    if (p->budget > (1ull << 39)) return fail(ORT_ERR_INVALID, "budget must be at most 1 << 39");
    if (!host) {
        const uint64_t need = 4ull * ((uint64_t)frame_count * (uint64_t)width * (uint64_t)height);
        if (!workspace || ((uintptr_t)workspace & 3u) || workspace_bytes < need) return fail(ORT_ERR_INVALID, "null, misaligned or short workspace (ort_plan_samples_workspace_bytes)");
    }
    std::string err;
    int rc = ort::device_plan_samples(device, host, *p, *in, width, height, frame_count, sample_map, totals, workspace, hip_stream, stats, &err);
    return rc == ORT_OK ? ORT_OK : fail(rc, err);
}
static int ort_comm_unique_id_impl(void *id) {
    if (!id) return fail(ORT_ERR_INVALID, "null argument");
    std::string err;
    int rc = ort::comm_unique_id(id, &err);
    return rc == ORT_OK ? ORT_OK : fail(rc, err);
}
static int ort_comm_create_impl(const void *id, int rank, int world, int device, ort_comm **out) {
    if (!out) return fail(ORT_ERR_INVALID, "null argument");
    std::string err;
    ort::Comm *c = nullptr;
    int rc = ort::comm_create(id, rank, world, device, &c, &err);
    *out = (ort_comm *)c;
    return rc == ORT_OK ? ORT_OK : fail(rc, err);
}
static int ort_comm_create_local_impl(int world, const int *devices, ort_comm **out) {
    if (!out || world < 1) return fail(ORT_ERR_INVALID, "bad argument");
    std::string err;
    int rc = ort::comm_create_local(world, devices, (ort::Comm **)out, &err);
    return rc == ORT_OK ? ORT_OK : fail(rc, err);
}
static int ort_gather_framebuffer_impl(ort_comm *comm, const void *d_packed, void *d_full_rgb, int32_t width, int32_t height, void *hip_stream) {
    if (!comm || !d_packed || width <= 0 || height <= 0) return fail(ORT_ERR_INVALID, "bad argument");
    std::string err;
    int rc = ort::gather_framebuffer((ort::Comm *)comm, d_packed, d_full_rgb, width, height, hip_stream, &err);
    return rc == ORT_OK ? ORT_OK : fail(rc, err);
}
static int ort_gather_framebuffer_local_impl(ort_comm **comms, int world, const void *const *d_packed, void *d_full_rgb_rank0, int32_t width,
                                             int32_t height, void *const *hip_streams) {
    if (!comms || !d_packed || !d_full_rgb_rank0 || world < 1 || width <= 0 || height <= 0) return fail(ORT_ERR_INVALID, "bad argument");
    std::string err;
    int rc = ort::gather_framebuffer_local((ort::Comm **)comms, world, d_packed, d_full_rgb_rank0, width, height, hip_streams, &err);
    return rc == ORT_OK ? ORT_OK : fail(rc, err);
}

/* ---- the exported entry points: every one behind guarded() ---- */
int ort_abi_version(void) { return guarded([&]() { return ort_abi_version_impl(); }); }
int ort_scene_parse_scn(const char *text, size_t size, const char *base_dir, ort_scene **out) { return guarded([&]() { return ort_scene_parse_scn_impl(text, size, base_dir, out); }); }
int ort_scene_load_scn(const char *scn_path, const char *base_dir, ort_scene **out) { return guarded([&]() { return ort_scene_load_scn_impl(scn_path, base_dir, out); }); }
int ort_scene_create(const ort_scene_desc *d, ort_scene **out) { return guarded([&]() { return ort_scene_create_impl(d, out); }); }
int ort_scene_get_info(const ort_scene *s, ort_scene_info *out) { return guarded([&]() { return ort_scene_get_info_impl(s, out); }); }
int ort_scene_get_materials(const ort_scene *s, ort_material *out, uint32_t cap) { return guarded([&]() { return ort_scene_get_materials_impl(s, out, cap); }); }
int ort_scene_get_spheres(const ort_scene *s, ort_sphere *out, uint32_t cap) { return guarded([&]() { return ort_scene_get_spheres_impl(s, out, cap); }); }
int ort_scene_get_boxes(const ort_scene *s, ort_box *out, uint32_t cap) { return guarded([&]() { return ort_scene_get_boxes_impl(s, out, cap); }); }
int ort_scene_get_cylinders(const ort_scene *s, ort_cylinder *out, uint32_t cap) { return guarded([&]() { return ort_scene_get_cylinders_impl(s, out, cap); }); }
int ort_scene_get_lights(const ort_scene *s, ort_light *out, uint32_t cap) { return guarded([&]() { return ort_scene_get_lights_impl(s, out, cap); }); }
int ort_scene_get_mesh(const ort_scene *s, uint32_t i, ort_mesh *out) { return guarded([&]() { return ort_scene_get_mesh_impl(s, i, out); }); }
int ort_scene_get_camera(const ort_scene *s, int32_t width, int32_t height, ort_camera *out) { return guarded([&]() { return ort_scene_get_camera_impl(s, width, height, out); }); }
int ort_scene_commit(ort_scene *s) { return guarded([&]() { return ort_scene_commit_impl(s); }); }
int ort_scene_get_tree_info(const ort_scene *s, ort_tree_info *out) { return guarded([&]() { return ort_scene_get_tree_info_impl(s, out); }); }
int ort_device_count(int *count) { return guarded([&]() { return ort_device_count_impl(count); }); }
int ort_scene_upload(ort_scene *s, int device) { return guarded([&]() { return ort_scene_upload_impl(s, device); }); }
int ort_tiled_raytrace_batch(ort_scene *s, float *out_rgb, int32_t width, int32_t height, const ort_tile_job *jobs, uint32_t job_count, float rr, uint32_t *final_states, ort_stats *stats) { return guarded([&]() { return ort_tiled_raytrace_batch_impl(s, out_rgb, width, height, jobs, job_count, rr, final_states, stats); }); }
int ort_tiled_raytrace(ort_scene *s, float *out_rgb, int32_t width, int32_t height, int32_t x0, int32_t y0, int32_t x1, int32_t y1, uint32_t *rng_state, uint32_t spp, float rr, uint64_t *shape_tests) { return guarded([&]() { return ort_tiled_raytrace_impl(s, out_rgb, width, height, x0, y0, x1, y1, rng_state, spp, rr, shape_tests); }); }
int ort_render_image(ort_scene *s, const ort_render_params *p, float *out_rgb, ort_stats *stats) { return guarded([&]() { return ort_render_image_impl(s, p, out_rgb, stats); }); }
int ort_render_image_device(ort_scene *s, const ort_render_params *p, void *d_out_rgb, void *hip_stream, ort_stats *stats) { return guarded([&]() { return ort_render_image_device_impl(s, p, d_out_rgb, hip_stream, stats); }); }
int ort_unit_eval_device(int device, const void *records, uint32_t count, float *out) { return guarded([&]() { return ort_unit_eval_device_impl(device, records, count, out); }); }
int ort_raycast(ort_scene *s, const float *rays, uint64_t count, ort_hit *hits, uint32_t flags, ort_stats *stats) { return guarded([&]() { return raycast_common(s, {true, count, flags, nullptr, stats}, rays, hits); }); }
int ort_raycast_device(ort_scene *s, const void *d_rays, uint64_t count, void *d_hits, uint32_t flags, void *hip_stream, ort_stats *stats) { return guarded([&]() { return raycast_common(s, {false, count, flags, hip_stream, stats}, d_rays, d_hits); }); }
int ort_occluded(ort_scene *s, const float *rays, const float *tmax, uint64_t count, uint8_t *occluded, uint32_t flags, ort_stats *stats) { return guarded([&]() { return occluded_common(s, {true, count, flags, nullptr, stats}, rays, tmax, occluded); }); }
int ort_occluded_device(ort_scene *s, const void *d_rays, const void *d_tmax, uint64_t count, void *d_occluded, uint32_t flags, void *hip_stream, ort_stats *stats) { return guarded([&]() { return occluded_common(s, {false, count, flags, hip_stream, stats}, d_rays, d_tmax, d_occluded); }); }
int ort_ambient_occlusion(ort_scene *s, const float *points, const uint32_t *seeds, const float *radius, uint64_t count, uint32_t spp, uint32_t *out_open, float *out_bent, uint32_t *final_states, uint32_t flags, ort_stats *stats) { return guarded([&]() { return ao_common(s, {true, count, flags, nullptr, stats}, points, seeds, radius, spp, out_open, out_bent, final_states); }); }
int ort_ambient_occlusion_device(ort_scene *s, const void *d_points, const void *d_seeds, const void *d_radius, uint64_t count, uint32_t spp, void *d_out_open, void *d_out_bent, void *d_final_states, uint32_t flags, void *hip_stream, ort_stats *stats) { return guarded([&]() { return ao_common(s, {false, count, flags, hip_stream, stats}, d_points, d_seeds, d_radius, spp, d_out_open, d_out_bent, d_final_states); }); }
int ort_radiance(ort_scene *s, const float *rays, const uint32_t *seeds, uint64_t count, uint32_t spp, float rr, float *out_rgb, uint32_t *final_states, uint32_t flags, ort_stats *stats) { return guarded([&]() { return radiance_common(s, {true, count, flags, nullptr, stats}, rays, seeds, spp, rr, false, nullptr, out_rgb, nullptr, nullptr, final_states); }); }
int ort_radiance_device(ort_scene *s, const void *d_rays, const void *d_seeds, uint64_t count, uint32_t spp, float rr, void *d_out_rgb, void *d_final_states, uint32_t flags, void *hip_stream, ort_stats *stats) { return guarded([&]() { return radiance_common(s, {false, count, flags, hip_stream, stats}, d_rays, d_seeds, spp, rr, false, nullptr, d_out_rgb, nullptr, nullptr, d_final_states); }); }
int ort_radiance_adaptive(ort_scene *s, const float *rays, const uint32_t *seeds, uint64_t count, const ort_adaptive *ad, float rr, float *out_rgb, uint32_t *out_spp, float *out_m2, uint32_t *final_states, uint32_t flags, ort_stats *stats) { return guarded([&]() { return radiance_common(s, {true, count, flags, nullptr, stats}, rays, seeds, 0, rr, true, ad, out_rgb, out_spp, out_m2, final_states); }); }
int ort_irradiance(ort_scene *s, const float *points, const uint32_t *seeds, uint64_t count, uint32_t spp, float rr, float *out_rgb, uint32_t *final_states, uint32_t flags, ort_stats *stats) { return guarded([&]() { return radiance_common(s, {true, count, flags, nullptr, stats}, points, seeds, spp, rr, false, nullptr, out_rgb, nullptr, nullptr, final_states, true); }); }
int ort_irradiance_device(ort_scene *s, const void *d_points, const void *d_seeds, uint64_t count, uint32_t spp, float rr, void *d_out_rgb, void *d_final_states, uint32_t flags, void *hip_stream, ort_stats *stats) { return guarded([&]() { return radiance_common(s, {false, count, flags, hip_stream, stats}, d_points, d_seeds, spp, rr, false, nullptr, d_out_rgb, nullptr, nullptr, d_final_states, true); }); }
int ort_probe_sh(ort_scene *s, const float *points, const uint32_t *seeds, uint64_t count, uint32_t spp, float rr, float *out_sh, float *out_rgb, uint32_t *final_states, uint32_t flags, ort_stats *stats) { return guarded([&]() { return radiance_common(s, {true, count, flags, nullptr, stats}, points, seeds, spp, rr, false, nullptr, out_rgb, nullptr, nullptr, final_states, true, true, out_sh); }); }
int ort_probe_sh_device(ort_scene *s, const void *d_points, const void *d_seeds, uint64_t count, uint32_t spp, float rr, void *d_out_sh, void *d_out_rgb, void *d_final_states, uint32_t flags, void *hip_stream, ort_stats *stats) { return guarded([&]() { return radiance_common(s, {false, count, flags, hip_stream, stats}, d_points, d_seeds, spp, rr, false, nullptr, d_out_rgb, nullptr, nullptr, d_final_states, true, true, d_out_sh); }); }
int ort_irradiance_adaptive(ort_scene *s, const float *points, const uint32_t *seeds, uint64_t count, const ort_adaptive *ad, float rr, float *out_rgb, uint32_t *out_spp, float *out_m2, uint32_t *final_states, uint32_t flags, ort_stats *stats) { return guarded([&]() { return radiance_common(s, {true, count, flags, nullptr, stats}, points, seeds, 0, rr, true, ad, out_rgb, out_spp, out_m2, final_states, true); }); }
int ort_irradiance_adaptive_device(ort_scene *s, const void *d_points, const void *d_seeds, uint64_t count, const ort_adaptive *ad, float rr, void *d_out_rgb, void *d_out_spp, void *d_out_m2, void *d_final_states, uint32_t flags, void *hip_stream, ort_stats *stats) { return guarded([&]() { return radiance_common(s, {false, count, flags, hip_stream, stats}, d_points, d_seeds, 0, rr, true, ad, d_out_rgb, d_out_spp, d_out_m2, d_final_states, true); }); }
int ort_radiance_adaptive_device(ort_scene *s, const void *d_rays, const void *d_seeds, uint64_t count, const ort_adaptive *ad, float rr, void *d_out_rgb, void *d_out_spp, void *d_out_m2, void *d_final_states, uint32_t flags, void *hip_stream, ort_stats *stats) { return guarded([&]() { return radiance_common(s, {false, count, flags, hip_stream, stats}, d_rays, d_seeds, 0, rr, true, ad, d_out_rgb, d_out_spp, d_out_m2, d_final_states); }); }
int ort_render_workspace_bytes(const ort_render_params *p, uint64_t *bytes) { return guarded([&]() { return ort_render_workspace_bytes_impl(p, bytes); }); }
int ort_camera_from_pose(const float p[3], const float quat_xyzw[4], float height_ratio, int32_t width, int32_t height, ort_camera *out) { return guarded([&]() { return ort_camera_from_pose_impl(p, quat_xyzw, height_ratio, width, height, out); }); }
int ort_render_views(ort_scene *s, const ort_render_params *p, const ort_view *views, uint32_t view_count, float *out_rgb, ort_stats *stats) { return guarded([&]() { return render_views_common(s, p, views, view_count, true, out_rgb, nullptr, stats); }); }
int ort_render_views_device(ort_scene *s, const ort_render_params *p, const ort_view *views, uint32_t view_count, void *d_out_rgb, void *hip_stream, ort_stats *stats) { return guarded([&]() { return render_views_common(s, p, views, view_count, false, d_out_rgb, hip_stream, stats); }); }
int ort_render_adaptive(ort_scene *s, const ort_render_params *p, const ort_adaptive *ad, float *out_rgb, uint32_t *out_spp, float *out_m2, uint32_t *final_states, ort_stats *stats) { return guarded([&]() { return render_adaptive_common(s, p, ad, nullptr, 1, false, true, out_rgb, out_spp, out_m2, final_states, nullptr, stats); }); }
int ort_render_adaptive_device(ort_scene *s, const ort_render_params *p, const ort_adaptive *ad, void *d_out_rgb, void *d_out_spp, void *d_out_m2, void *d_final_states, void *hip_stream, ort_stats *stats) { return guarded([&]() { return render_adaptive_common(s, p, ad, nullptr, 1, false, false, d_out_rgb, d_out_spp, d_out_m2, d_final_states, hip_stream, stats); }); }
int ort_render_views_adaptive(ort_scene *s, const ort_render_params *p, const ort_adaptive *ad, const ort_view *views, uint32_t view_count, float *out_rgb, uint32_t *out_spp, float *out_m2, uint32_t *final_states, ort_stats *stats) { return guarded([&]() { return render_adaptive_common(s, p, ad, views, view_count, true, true, out_rgb, out_spp, out_m2, final_states, nullptr, stats); }); }
int ort_render_depths(ort_scene *s, const ort_render_params *p, uint32_t bin_count, float *out_bins, float *out_rgb, uint32_t *out_lengths, uint32_t *final_states, ort_stats *stats) { return guarded([&]() { return render_depths_common(s, p, bin_count, nullptr, 1, false, true, out_bins, out_rgb, out_lengths, final_states, nullptr, stats); }); }
int ort_render_depths_device(ort_scene *s, const ort_render_params *p, uint32_t bin_count, void *d_out_bins, void *d_out_rgb, void *d_out_lengths, void *d_final_states, void *hip_stream, ort_stats *stats) { return guarded([&]() { return render_depths_common(s, p, bin_count, nullptr, 1, false, false, d_out_bins, d_out_rgb, d_out_lengths, d_final_states, hip_stream, stats); }); }
int ort_render_views_depths(ort_scene *s, const ort_render_params *p, uint32_t bin_count, const ort_view *views, uint32_t view_count, float *out_bins, float *out_rgb, uint32_t *out_lengths, uint32_t *final_states, ort_stats *stats) { return guarded([&]() { return render_depths_common(s, p, bin_count, views, view_count, true, true, out_bins, out_rgb, out_lengths, final_states, nullptr, stats); }); }
int ort_render_views_depths_device(ort_scene *s, const ort_render_params *p, uint32_t bin_count, const ort_view *views, uint32_t view_count, void *d_out_bins, void *d_out_rgb, void *d_out_lengths, void *d_final_states, void *hip_stream, ort_stats *stats) { return guarded([&]() { return render_depths_common(s, p, bin_count, views, view_count, true, false, d_out_bins, d_out_rgb, d_out_lengths, d_final_states, hip_stream, stats); }); }
int ort_render_light_groups(ort_scene *s, const ort_render_params *p, const ort_light_groups *groups, float *out_groups, float *out_rgb, uint32_t *final_states, ort_stats *stats) { return guarded([&]() { return render_groups_common(s, p, groups, nullptr, 1, false, true, out_groups, out_rgb, final_states, nullptr, stats); }); }
int ort_render_light_groups_device(ort_scene *s, const ort_render_params *p, const ort_light_groups *groups, void *d_out_groups, void *d_out_rgb, void *d_final_states, void *hip_stream, ort_stats *stats) { return guarded([&]() { return render_groups_common(s, p, groups, nullptr, 1, false, false, d_out_groups, d_out_rgb, d_final_states, hip_stream, stats); }); }
int ort_render_views_light_groups(ort_scene *s, const ort_render_params *p, const ort_light_groups *groups, const ort_view *views, uint32_t view_count, float *out_groups, float *out_rgb, uint32_t *final_states, ort_stats *stats) { return guarded([&]() { return render_groups_common(s, p, groups, views, view_count, true, true, out_groups, out_rgb, final_states, nullptr, stats); }); }
int ort_render_views_light_groups_device(ort_scene *s, const ort_render_params *p, const ort_light_groups *groups, const ort_view *views, uint32_t view_count, void *d_out_groups, void *d_out_rgb, void *d_final_states, void *hip_stream, ort_stats *stats) { return guarded([&]() { return render_groups_common(s, p, groups, views, view_count, true, false, d_out_groups, d_out_rgb, d_final_states, hip_stream, stats); }); }
int ort_render_views_adaptive_device(ort_scene *s, const ort_render_params *p, const ort_adaptive *ad, const ort_view *views, uint32_t view_count, void *d_out_rgb, void *d_out_spp, void *d_out_m2, void *d_final_states, void *hip_stream, ort_stats *stats) { return guarded([&]() { return render_adaptive_common(s, p, ad, views, view_count, true, false, d_out_rgb, d_out_spp, d_out_m2, d_final_states, hip_stream, stats); }); }
int ort_render_sample_map(ort_scene *s, const ort_render_params *p, const uint32_t *sample_map, float *out_rgb, float *out_m2, uint32_t *final_states, ort_stats *stats) { return guarded([&]() { return render_sample_map_common(s, p, nullptr, 1, false, true, sample_map, out_rgb, out_m2, final_states, nullptr, stats); }); }
int ort_render_sample_map_device(ort_scene *s, const ort_render_params *p, const void *d_sample_map, void *d_out_rgb, void *d_out_m2, void *d_final_states, void *hip_stream, ort_stats *stats) { return guarded([&]() { return render_sample_map_common(s, p, nullptr, 1, false, false, d_sample_map, d_out_rgb, d_out_m2, d_final_states, hip_stream, stats); }); }
int ort_render_views_sample_map(ort_scene *s, const ort_render_params *p, const ort_view *views, uint32_t view_count, const uint32_t *sample_map, float *out_rgb, float *out_m2, uint32_t *final_states, ort_stats *stats) { return guarded([&]() { return render_sample_map_common(s, p, views, view_count, true, true, sample_map, out_rgb, out_m2, final_states, nullptr, stats); }); }
int ort_render_views_sample_map_device(ort_scene *s, const ort_render_params *p, const ort_view *views, uint32_t view_count, const void *d_sample_map, void *d_out_rgb, void *d_out_m2, void *d_final_states, void *hip_stream, ort_stats *stats) { return guarded([&]() { return render_sample_map_common(s, p, views, view_count, true, false, d_sample_map, d_out_rgb, d_out_m2, d_final_states, hip_stream, stats); }); }
int ort_render_accumulate(ort_scene *s, const ort_render_params *p, const ort_accum_planes *acc, const uint32_t *sample_map, float *out_rgb, ort_stats *stats) { return guarded([&]() { return render_accumulate_common(s, p, nullptr, 1, false, true, acc, sample_map, out_rgb, nullptr, stats); }); }
int ort_render_accumulate_device(ort_scene *s, const ort_render_params *p, const ort_accum_planes *acc, const void *d_sample_map, void *d_out_rgb, void *hip_stream, ort_stats *stats) { return guarded([&]() { return render_accumulate_common(s, p, nullptr, 1, false, false, acc, d_sample_map, d_out_rgb, hip_stream, stats); }); }
int ort_render_views_accumulate(ort_scene *s, const ort_render_params *p, const ort_view *views, uint32_t view_count, const ort_accum_planes *acc, const uint32_t *sample_map, float *out_rgb, ort_stats *stats) { return guarded([&]() { return render_accumulate_common(s, p, views, view_count, true, true, acc, sample_map, out_rgb, nullptr, stats); }); }
int ort_render_views_accumulate_device(ort_scene *s, const ort_render_params *p, const ort_view *views, uint32_t view_count, const ort_accum_planes *acc, const void *d_sample_map, void *d_out_rgb, void *hip_stream, ort_stats *stats) { return guarded([&]() { return render_accumulate_common(s, p, views, view_count, true, false, acc, d_sample_map, d_out_rgb, hip_stream, stats); }); }
int ort_render_features(ort_scene *s, const ort_render_params *p, const ort_feature_planes *planes, ort_stats *stats) { return guarded([&]() { return render_features_common(s, p, nullptr, 1, false, true, planes, nullptr, stats); }); }
int ort_render_features_device(ort_scene *s, const ort_render_params *p, const ort_feature_planes *planes, void *hip_stream, ort_stats *stats) { return guarded([&]() { return render_features_common(s, p, nullptr, 1, false, false, planes, hip_stream, stats); }); }
int ort_render_views_features(ort_scene *s, const ort_render_params *p, const ort_view *views, uint32_t view_count, const ort_feature_planes *planes, ort_stats *stats) { return guarded([&]() { return render_features_common(s, p, views, view_count, true, true, planes, nullptr, stats); }); }
int ort_render_views_features_device(ort_scene *s, const ort_render_params *p, const ort_view *views, uint32_t view_count, const ort_feature_planes *planes, void *hip_stream, ort_stats *stats) { return guarded([&]() { return render_features_common(s, p, views, view_count, true, false, planes, hip_stream, stats); }); }
int ort_render_follow(ort_scene *s, const ort_render_params *p, uint32_t max_bounces, const ort_follow_planes *planes, ort_stats *stats) { return guarded([&]() { return render_follow_common(s, p, nullptr, 1, false, true, max_bounces, planes, nullptr, stats); }); }
int ort_render_follow_device(ort_scene *s, const ort_render_params *p, uint32_t max_bounces, const ort_follow_planes *planes, void *hip_stream, ort_stats *stats) { return guarded([&]() { return render_follow_common(s, p, nullptr, 1, false, false, max_bounces, planes, hip_stream, stats); }); }
int ort_render_views_follow(ort_scene *s, const ort_render_params *p, const ort_view *views, uint32_t view_count, uint32_t max_bounces, const ort_follow_planes *planes, ort_stats *stats) { return guarded([&]() { return render_follow_common(s, p, views, view_count, true, true, max_bounces, planes, nullptr, stats); }); }
int ort_render_views_follow_device(ort_scene *s, const ort_render_params *p, const ort_view *views, uint32_t view_count, uint32_t max_bounces, const ort_follow_planes *planes, void *hip_stream, ort_stats *stats) { return guarded([&]() { return render_follow_common(s, p, views, view_count, true, false, max_bounces, planes, hip_stream, stats); }); }
int ort_render_matte(ort_scene *s, const ort_render_params *p, const ort_matte *m, const ort_matte_planes *planes, ort_stats *stats) { return guarded([&]() { return render_matte_common(s, p, nullptr, 1, false, true, m, planes, nullptr, stats); }); }
int ort_render_matte_device(ort_scene *s, const ort_render_params *p, const ort_matte *m, const ort_matte_planes *planes, void *hip_stream, ort_stats *stats) { return guarded([&]() { return render_matte_common(s, p, nullptr, 1, false, false, m, planes, hip_stream, stats); }); }
int ort_render_views_matte(ort_scene *s, const ort_render_params *p, const ort_view *views, uint32_t view_count, const ort_matte *m, const ort_matte_planes *planes, ort_stats *stats) { return guarded([&]() { return render_matte_common(s, p, views, view_count, true, true, m, planes, nullptr, stats); }); }
int ort_render_views_matte_device(ort_scene *s, const ort_render_params *p, const ort_view *views, uint32_t view_count, const ort_matte *m, const ort_matte_planes *planes, void *hip_stream, ort_stats *stats) { return guarded([&]() { return render_matte_common(s, p, views, view_count, true, false, m, planes, hip_stream, stats); }); }
int ort_matte_mask(int device, const uint32_t *ids, const uint32_t *counts, uint32_t slots, uint32_t spp, const uint32_t *select, uint32_t select_count, int32_t width, int32_t height, uint32_t frame_count, float *out_mask) { return guarded([&]() { return matte_mask_common(device, true, ids, counts, slots, spp, select, select_count, width, height, frame_count, out_mask, nullptr); }); }
int ort_matte_mask_device(int device, const void *d_ids, const void *d_counts, uint32_t slots, uint32_t spp, const uint32_t *select, uint32_t select_count, int32_t width, int32_t height, uint32_t frame_count, void *d_out_mask, void *hip_stream) { return guarded([&]() { return matte_mask_common(device, false, d_ids, d_counts, slots, spp, select, select_count, width, height, frame_count, d_out_mask, hip_stream); }); }
int ort_render_views_workspace_bytes(const ort_render_params *p, uint32_t view_count, uint64_t *bytes) { return guarded([&]() { return ort_render_views_workspace_bytes_impl(p, view_count, bytes); }); }
int ort_shard_block_count(int32_t width, int32_t height, uint32_t shard_index, uint32_t shard_count, uint64_t *blocks) { return guarded([&]() { return ort_shard_block_count_impl(width, height, shard_index, shard_count, blocks); }); }
int ort_pack_blocks_host(const float *full_rgb, int32_t width, int32_t height, uint32_t shard_index, uint32_t shard_count, float *packed) { return guarded([&]() { return ort_pack_blocks_host_impl(full_rgb, width, height, shard_index, shard_count, packed); }); }
int ort_unpack_blocks_host(const float *packed, int32_t width, int32_t height, uint32_t shard_index, uint32_t shard_count, float *full_rgb) { return guarded([&]() { return ort_unpack_blocks_host_impl(packed, width, height, shard_index, shard_count, full_rgb); }); }
int ort_unpack_blocks_device(const void *d_packed, int32_t width, int32_t height, uint32_t shard_index, uint32_t shard_count, void *d_full_rgb, void *hip_stream) { return guarded([&]() { return ort_unpack_blocks_device_impl(d_packed, width, height, shard_index, shard_count, d_full_rgb, hip_stream); }); }
int ort_denoise_workspace_bytes(int32_t width, int32_t height, uint32_t frame_count, uint64_t *bytes) { return guarded([&]() { return ort_denoise_workspace_bytes_impl(width, height, frame_count, bytes); }); }
int ort_denoise(int device, const ort_denoise_params *p, const ort_denoise_planes *in, int32_t width, int32_t height, uint32_t frame_count, float *out_rgb, ort_stats *stats) { return guarded([&]() { return denoise_common(device, true, p, in, width, height, frame_count, out_rgb, nullptr, 0, nullptr, stats); }); }
int ort_denoise_device(int device, const ort_denoise_params *p, const ort_denoise_planes *in, int32_t width, int32_t height, uint32_t frame_count, void *d_out_rgb, void *d_workspace, uint64_t workspace_bytes, void *hip_stream, ort_stats *stats) { return guarded([&]() { return denoise_common(device, false, p, in, width, height, frame_count, d_out_rgb, d_workspace, workspace_bytes, hip_stream, stats); }); }
int ort_plan_samples_workspace_bytes(int32_t width, int32_t height, uint32_t frame_count, uint64_t *bytes) { return guarded([&]() { return ort_plan_samples_workspace_bytes_impl(width, height, frame_count, bytes); }); }
int ort_plan_samples(int device, const ort_plan_params *p, const ort_plan_planes *in, int32_t width, int32_t height, uint32_t frame_count, uint32_t *sample_map, ort_plan_totals *totals, ort_stats *stats) { return guarded([&]() { return plan_common(device, true, p, in, width, height, frame_count, sample_map, totals, nullptr, 0, nullptr, stats); }); }
int ort_plan_samples_device(int device, const ort_plan_params *p, const ort_plan_planes *in, int32_t width, int32_t height, uint32_t frame_count, void *d_sample_map, void *d_totals, void *d_workspace, uint64_t workspace_bytes, void *hip_stream, ort_stats *stats) { return guarded([&]() { return plan_common(device, false, p, in, width, height, frame_count, d_sample_map, d_totals, d_workspace, workspace_bytes, hip_stream, stats); }); }
int ort_comm_unique_id(void *id) { return guarded([&]() { return ort_comm_unique_id_impl(id); }); }
int ort_comm_create(const void *id, int rank, int world, int device, ort_comm **out) { return guarded([&]() { return ort_comm_create_impl(id, rank, world, device, out); }); }
int ort_comm_create_local(int world, const int *devices, ort_comm **out) { return guarded([&]() { return ort_comm_create_local_impl(world, devices, out); }); }
int ort_gather_framebuffer(ort_comm *comm, const void *d_packed, void *d_full_rgb, int32_t width, int32_t height, void *hip_stream) { return guarded([&]() { return ort_gather_framebuffer_impl(comm, d_packed, d_full_rgb, width, height, hip_stream); }); }
int ort_gather_framebuffer_local(ort_comm **comms, int world, const void *const *d_packed, void *d_full_rgb_rank0, int32_t width, int32_t height, void *const *hip_streams) { return guarded([&]() { return ort_gather_framebuffer_local_impl(comms, world, d_packed, d_full_rgb_rank0, width, height, hip_streams); }); }
void ort_comm_destroy(ort_comm *comm) { try { ort::comm_destroy((ort::Comm *)comm); } catch (...) {} }

} // extern "C"
