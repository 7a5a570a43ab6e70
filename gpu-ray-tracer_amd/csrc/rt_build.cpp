// rt_build.cpp — the C ABI's entries that make, describe and change a scene without launching a
// kernel: loading and creation, the SceneBuilder calls, info and exports, the camera, the
// environment and the atlas.  Host code only (rt_internal.h).
#include <cstring>
#include <fstream>
#include <memory>

#include "rt_internal.h"

using namespace rtm;
using namespace rtd;
using namespace rti;
using rt::DCamera;

namespace {

rt::Material mat_from(const float* m) {
    rt::Material r;
    r.Ke = v4(m[0], m[1], m[2], m[3]); r.Ka = v4(m[4], m[5], m[6], m[7]); r.Kd = v4(m[8], m[9], m[10], m[11]);
    r.Ks = v4(m[12], m[13], m[14], m[15]); r.Kt = v4(m[16], m[17], m[18], m[19]); r.Kr = v4(m[20], m[21], m[22], m[23]);
    r.alpha = m[24]; r.eta = m[25];
    return r;
}

// (ABI 3) hit_tri indexes the triangles in flattened mesh order, so the meshes must list every
// triangle exactly once: a bitmap of the triangles seen, failing on a repeat or on one left out
// (a count alone would pass a list that repeats one triangle and omits another).
bool meshes_cover_tris_once(const rt::Scene& h) {
    std::vector<unsigned char> seen(h.tris.size(), 0);
    size_t n = 0;
    for (auto& m : h.meshes)
        for (int i : m.tris) {
            if (i < 0 || (size_t)i >= seen.size() || seen[i]) return false;
            seen[i] = 1;
            n++;
        }
    return n == h.tris.size();
}

// RT_EXPORT_BVH_* (test hook): the arrays the most recent BVH build wrote into its frame slot,
// copied to the host once that slot's work is done.  Copies only: no launch, no state change.
int export_built_bvh(const rt_scene* s, int what, void* dst, int64_t cap) {
    const rt_scene::Built& b = s->built;
    if (!s->uploaded || b.slot < 0) return fail(RT_ERR_STATE, "no BVH built yet (render a frame first)");
    const FrameSlot& f = s->slots[b.slot];
    const size_t n = (size_t)s->n_leaf;
    const int32_t info[8] = {s->n_leaf, (int32_t)s->h.d_insts.size(), b.n_real, b.fdepth,
                             ordered_tree_usable(b.n_real, b.fdepth) ? 1 : 0, b.form, b.slot, 0};
    const void* src = nullptr;
    size_t bytes = 0;
    switch (what) {
        case RT_EXPORT_BVH_INFO: bytes = sizeof info; break;
        case RT_EXPORT_BVH_PAIRS: src = f.d_node_pair; bytes = 12 * n * sizeof(float); break;
        case RT_EXPORT_BVH_LEAF_INST: src = f.d_leaf; bytes = n * sizeof(int32_t); break;
        default: src = f.d_fnode; bytes = 16 * (size_t)std::max(b.n_real - 1, 0) * sizeof(float); break;
    }
    if ((bytes && !dst) || cap < (int64_t)bytes) return fail(RT_ERR_ARG, "destination too small");
    if (what == RT_EXPORT_BVH_INFO) { memcpy(dst, info, sizeof info); return RT_OK; }
    if (!bytes) return RT_OK;
    HIPCHK(hipSetDevice(s->device));
    if (f.pending) HIPCHK(hipEventSynchronize(f.done));
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_spp_offset(int k, float* dx, float* dy) {
    if (k < 0 || !dx || !dy) return fail(RT_ERR_ARG, "bad arguments");
    rt::spp_offset(k, dx, dy);
    return RT_OK;
}

int rt_scene_load_json(const char* path, int width, int height, rt_scene** out) {
    if (!path || !out) return fail(RT_ERR_ARG, "null argument");
    std::unique_ptr<rt_scene> s(new rt_scene);
    std::string err;
    int r = rt::load_cube_world(path, width, height, &s->h, &err);
    if (r == -2) return fail(RT_ERR_IO, err);
    if (r != 0) return fail(RT_ERR_PARSE, err);
    s->finished = true;
    s->canvas.assign((size_t)s->h.cam.W * s->h.cam.H, 0u);
    (void)warm_scene(s.get());
    *out = s.release();
    return RT_OK;
}

int rt_scene_create(const char* atlas, rt_scene** out) {
    if (!out) return fail(RT_ERR_ARG, "null argument");
    rt_scene* s = new rt_scene;
    s->h.atlas = atlas ? atlas : "";
    *out = s;
    return RT_OK;
}

int rt_scene_free(rt_scene* s) { delete s; return RT_OK; }

int rt_builder_add_vertex(rt_scene* s, float x, float y, float z, int* idx) {
    CHECK_BUILDING(s);
    int i = s->h.add_vertex(v3(x, y, z));
    if (idx) *idx = i;
    return RT_OK;
}
int rt_builder_create_mesh(rt_scene* s, const float* pos, const float* q, int* mesh) {
    CHECK_BUILDING(s);
    int m = s->h.create_mesh(pos ? v3(pos[0], pos[1], pos[2]) : v3(0, 0, 0), q ? Q{q[0], q[1], q[2], q[3]} : Q{0, 0, 0, 1});
    if (mesh) *mesh = m;
    return RT_OK;
}
int rt_builder_add_triangle(rt_scene* s, int mesh, int i0, int i1, int i2, const float* mat) {
    CHECK_BUILDING(s);
    if (!mat) return fail(RT_ERR_ARG, "null material");
    if (mesh < 0 || mesh >= (int)s->h.meshes.size()) return fail(RT_ERR_ARG, "mesh index out of range");
    int nv = (int)s->h.verts.size();
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) return fail(RT_ERR_ARG, "vertex index out of range");
    s->h.add_triangle(mesh, i0, i1, i2, s->h.add_material(mat_from(mat)));
    return RT_OK;
}
int rt_builder_add_triangle_tex(rt_scene* s, int mesh, int i0, int i1, int i2, const float* mat, const float* tex) {
    CHECK_BUILDING(s);
    if (!mat || !tex) return fail(RT_ERR_ARG, "null argument");
    if (mesh < 0 || mesh >= (int)s->h.meshes.size()) return fail(RT_ERR_ARG, "mesh index out of range");
    int nv = (int)s->h.verts.size();
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) return fail(RT_ERR_ARG, "vertex index out of range");
    rt::TexDesc t;
    t.has = 1; t.tx = tex[0]; t.ty = tex[1]; t.ux = tex[2]; t.uy = tex[3]; t.vx = tex[4]; t.vy = tex[5];
    s->h.add_triangle(mesh, i0, i1, i2, s->h.add_material(mat_from(mat)), t);
    return RT_OK;
}
int rt_builder_add_trans(rt_scene* s, int mesh, int* trans) {
    CHECK_BUILDING(s);
    if (mesh < 0 || mesh >= (int)s->h.meshes.size()) return fail(RT_ERR_ARG, "mesh index out of range");
    int t = s->h.add_trans(mesh);
    if (trans) *trans = t;
    return RT_OK;
}
int rt_builder_set_trans(rt_scene* s, int t, const float* pos, const float* q) {
    CHECK_SCENE(s);
    if (t < 0 || t >= (int)s->h.insts.size()) return fail(RT_ERR_ARG, "transformation index out of range");
    if (pos) s->h.insts[t].pos = v3(pos[0], pos[1], pos[2]);
    if (q) s->h.insts[t].rot = Q{q[0], q[1], q[2], q[3]};
    if (s->finished) {   // instances moved after finishing: refresh the flat copy
        // Device copies are per frame slot and are refreshed, stream-ordered, by the next frame
        // of each slot (sync_slot_insts): frames in flight keep the poses they were built from.
        s->h.d_insts[t].pose = make_pose(s->h.insts[t].rot, s->h.insts[t].pos);
        s->inst_gen++;
        invalidate(s);
    }
    return RT_OK;
}
int rt_builder_build_cube(rt_scene* s, float scale, const float* mat, int* mesh) {
    CHECK_BUILDING(s);
    if (!mat) return fail(RT_ERR_ARG, "null material");
    int m = s->h.build_cube(scale, mat_from(mat));
    if (mesh) *mesh = m;
    return RT_OK;
}
int rt_builder_build_cube_tex(rt_scene* s, float scale, const float* mat, const float* tile, int* mesh) {
    CHECK_BUILDING(s);
    if (!mat || !tile) return fail(RT_ERR_ARG, "null argument");
    int m = s->h.build_cube(scale, mat_from(mat), tile);
    if (mesh) *mesh = m;
    return RT_OK;
}
int rt_builder_add_point_light(rt_scene* s, const float* pos, const float* col) {
    CHECK_BUILDING(s);
    if (!pos || !col) return fail(RT_ERR_ARG, "null argument");
    s->h.add_point_light(v3(pos[0], pos[1], pos[2]), v4(col[0], col[1], col[2], col[3]));
    return RT_OK;
}
int rt_builder_add_directional_light(rt_scene* s, const float* dir, const float* col) {
    CHECK_BUILDING(s);
    if (!dir || !col) return fail(RT_ERR_ARG, "null argument");
    s->h.add_directional_light(v3(dir[0], dir[1], dir[2]), v4(col[0], col[1], col[2], col[3]));
    return RT_OK;
}
int rt_builder_finish(rt_scene* s, int W, int H, float fov, float unit, const float* cpos, const float* cq,
                      const float* da, const float* amb, int depth) {
    CHECK_BUILDING(s);
    if (W <= 0 || H <= 0 || !(unit > 0)) return fail(RT_ERR_ARG, "bad canvas/camera parameters");
    s->h.set_camera(W, H, fov, unit);
    if (cpos) s->h.cam.pos = v3(cpos[0], cpos[1], cpos[2]);
    if (cq) s->h.cam.rot = Q{cq[0], cq[1], cq[2], cq[3]};
    if (da) s->h.dist_atten = v3(da[0], da[1], da[2]);
    if (amb) s->h.ambience = v4(amb[0], amb[1], amb[2], amb[3]);
    s->h.depth = depth;
    std::string err;
    if (s->h.flatten(&err) != 0) return fail(RT_ERR_PARSE, err);
    s->finished = true;
    s->canvas.assign((size_t)W * H, 0u);
    (void)warm_scene(s);
    return RT_OK;
}

int rt_scene_info(const rt_scene* s, int32_t* c) {
    CHECK_FINISHED(s);
    if (!c) return fail(RT_ERR_ARG, "null argument");
    const rt::Scene& h = s->h;
    c[0] = h.cam.W; c[1] = h.cam.H; c[2] = (int)h.verts.size(); c[3] = (int)h.tris.size(); c[4] = (int)h.meshes.size();
    c[5] = (int)h.insts.size(); c[6] = (int)h.d_lights.size(); c[7] = (int)h.points.size(); c[8] = h.depth;
    c[9] = (int)h.mats.size();
    return RT_OK;
}

int rt_scene_export(const rt_scene* s, int what, void* dst, int64_t cap) {
    CHECK_FINISHED(s);
    if (what >= RT_EXPORT_BVH_INFO && what <= RT_EXPORT_BVH_FNODE) return export_built_bvh(s, what, dst, cap);
    const rt::Scene& h = s->h;
    if ((what == RT_EXPORT_TRIS || what == RT_EXPORT_TEXCOORDS) && !meshes_cover_tris_once(h))
        return fail(RT_ERR_STATE, "meshes do not cover every triangle once");
    std::vector<float> f;
    std::vector<int32_t> iv;
    switch (what) {
        case RT_EXPORT_VERTICES: for (auto& v : h.verts) { f.push_back(v.x); f.push_back(v.y); f.push_back(v.z); } break;
        case RT_EXPORT_NORMALS: f = h.verts_norm; break;
        case RT_EXPORT_TRIS:                                   // flattened (mesh) order: hit_tri indexes it
            for (auto& m : h.meshes)
                for (int i : m.tris) { const auto& t = h.tris[i]; iv.insert(iv.end(), {t.i0, t.i1, t.i2, t.mat}); }
            break;
        case RT_EXPORT_MATERIALS:
            for (auto& m : h.mats) {
                for (const V4* v : {&m.Ke, &m.Ka, &m.Kd, &m.Ks, &m.Kt, &m.Kr}) { f.push_back(v->x); f.push_back(v->y); f.push_back(v->z); f.push_back(v->w); }
                f.push_back(m.alpha); f.push_back(m.eta);
            }
            break;
        case RT_EXPORT_INSTANCES:
            for (auto& t : h.insts) { f.insert(f.end(), {t.rot.i, t.rot.j, t.rot.k, t.rot.r, t.pos.x, t.pos.y, t.pos.z}); }
            break;
        case RT_EXPORT_INST_MESH: for (auto& t : h.insts) iv.push_back(t.mesh); break;
        case RT_EXPORT_LIGHTS:
            for (auto& l : h.d_lights) f.insert(f.end(), {l.v.x, l.v.y, l.v.z, (float)l.type, l.col.x, l.col.y, l.col.z, l.col.w});
            break;
        case RT_EXPORT_CAMERA: {
            const DCamera& c = h.d_cam;
            f = {c.pos.x, c.pos.y, c.pos.z, h.cam.rot.i, h.cam.rot.j, h.cam.rot.k, h.cam.rot.r, c.near_, c.unit, c.W, c.H,
                 c.r.x, c.r.y, c.r.z, c.u.x, c.u.y, c.u.z, c.f.x, c.f.y, c.f.z, 0.0f};
            break;
        }
        case RT_EXPORT_ENV:
            f = {h.dist_atten.x, h.dist_atten.y, h.dist_atten.z, h.ambience.x, h.ambience.y, h.ambience.z, h.ambience.w};
            break;
        case RT_EXPORT_TEXCOORDS:
            for (auto& m : h.meshes)
                for (int i : m.tris) {
                    const auto& t = h.tris[i];
                    f.insert(f.end(), {(float)t.tex.has, t.tex.tx, t.tex.ty, t.tex.ux, t.tex.uy, t.tex.vx, t.tex.vy});
                }
            break;
        case RT_EXPORT_ATLAS: {
            const size_t n = h.atlas_rgba.size();
            if (!dst || cap < (int64_t)n) return fail(RT_ERR_ARG, "destination too small");
            if (n) memcpy(dst, h.atlas_rgba.data(), n);
            return RT_OK;
        }
        default: return fail(RT_ERR_ARG, "unknown export");
    }
    size_t bytes = f.size() * 4 + iv.size() * 4;
    if (!dst || cap < (int64_t)bytes) return fail(RT_ERR_ARG, "destination too small");
    if (!f.empty()) memcpy(dst, f.data(), f.size() * 4);
    if (!iv.empty()) memcpy(dst, iv.data(), iv.size() * 4);
    return RT_OK;
}

int rt_camera_get(const rt_scene* s, float* pos, float* q) {
    CHECK_SCENE(s);
    if (pos) { pos[0] = s->h.cam.pos.x; pos[1] = s->h.cam.pos.y; pos[2] = s->h.cam.pos.z; }
    if (q) { q[0] = s->h.cam.rot.i; q[1] = s->h.cam.rot.j; q[2] = s->h.cam.rot.k; q[3] = s->h.cam.rot.r; }
    return RT_OK;
}
int rt_camera_set(rt_scene* s, const float* pos, const float* q) {
    CHECK_FINISHED(s);
    if (pos) s->h.cam.pos = v3(pos[0], pos[1], pos[2]);
    if (q) s->h.cam.rot = Q{q[0], q[1], q[2], q[3]};
    s->h.update_camera_basis();
    s->cam_gen++;
    return RT_OK;
}
int rt_camera_translate(rt_scene* s, const float* d) {           // entity.h:53-56: translate_global(vec_to_local(dp))
    CHECK_FINISHED(s);
    if (!d) return fail(RT_ERR_ARG, "null argument");
    s->h.cam.pos = s->h.cam.pos + qrot(s->h.cam.rot, v3(d[0], d[1], d[2]));
    s->h.update_camera_basis();
    s->cam_gen++;
    return RT_OK;
}
int rt_camera_rotate(rt_scene* s, const float* dq) {             // entity.h:63-65: o = dr * o
    CHECK_FINISHED(s);
    if (!dq) return fail(RT_ERR_ARG, "null argument");
    s->h.cam.rot = qmul(Q{dq[0], dq[1], dq[2], dq[3]}, s->h.cam.rot);
    s->h.update_camera_basis();
    s->cam_gen++;
    return RT_OK;
}
int rt_camera_axes(const rt_scene* s, float* r, float* u, float* f) {
    CHECK_FINISHED(s);
    const DCamera& c = s->h.d_cam;
    if (r) { r[0] = c.r.x; r[1] = c.r.y; r[2] = c.r.z; }
    if (u) { u[0] = c.u.x; u[1] = c.u.y; u[2] = c.u.z; }
    if (f) { f[0] = c.f.x; f[1] = c.f.y; f[2] = c.f.z; }
    return RT_OK;
}
int rt_env_set(rt_scene* s, const float* amb, const float* da, int depth) {
    CHECK_FINISHED(s);
    if (depth < 0 || depth >= MAX_FRAMES) return fail(RT_ERR_ARG, "depth must be in [0, 9]");
    if (amb) s->h.ambience = v4(amb[0], amb[1], amb[2], amb[3]);
    if (da) s->h.dist_atten = v3(da[0], da[1], da[2]);
    s->h.depth = depth;
    s->env_gen++;
    return RT_OK;
}

int rt_scene_set_atlas(rt_scene* s, const uint8_t* rgba8, int w, int h) {
    if (!s) return fail(RT_ERR_ARG, "null scene");
    if (!rgba8 || w <= 0 || h <= 0 || w > 16384 || h > 16384) return fail(RT_ERR_ARG, "bad atlas image");
    s->h.atlas_rgba.assign(rgba8, rgba8 + (size_t)w * h * 4);
    s->h.atlas_w = w; s->h.atlas_h = h;
    s->atlas_dirty = true;
    s->atlas_gen++;
    return RT_OK;
}
int rt_scene_load_atlas(rt_scene* s, const char* path) {
    if (!s) return fail(RT_ERR_ARG, "null scene");
    std::vector<std::string> tries;
    if (path) tries.push_back(path);
    else {
        if (s->h.atlas.empty()) return fail(RT_ERR_STATE, "the scene names no atlas");
        if (s->h.atlas[0] != '/' && !s->h.base_dir.empty()) tries.push_back(s->h.base_dir + "/" + s->h.atlas);
        tries.push_back(s->h.atlas);
    }
    std::string err;
    for (const std::string& p : tries) {
        std::ifstream probe(p, std::ios::binary);
        if (!probe) { err = p + ": cannot open"; continue; }
        std::vector<uint8_t> px;
        int w = 0, h = 0;
        if (rt::load_png_rgba8(p, &px, &w, &h, &err) != 0) return fail(RT_ERR_PARSE, err);
        return rt_scene_set_atlas(s, px.data(), w, h);
    }
    return fail(RT_ERR_IO, err);
}
int rt_scene_atlas_info(const rt_scene* s, int32_t* a) {
    if (!s || !a) return fail(RT_ERR_ARG, "null argument");
    a[0] = s->h.atlas_w; a[1] = s->h.atlas_h; a[2] = s->h.atlas_rgba.empty() ? 0 : 1;
    return RT_OK;
}

}  // extern "C"
