// rt_runtime.cpp — the frame path of the host runtime: the scene object's upload (rt_internal.h),
// the frame slots, the per-frame BVH build and trace launch set-up, rt_render / rt_update_scene
// with the slot, overlap, timing, canvas and device entries, and the error text.  The other
// entry families of the C ABI (rt_amd.h) build on it from files of their own: rt_build.cpp,
// rt_accumulate.cpp, rt_occlusion.cpp, rt_query.cpp, rt_hooks.cpp, rt_multi.cpp, rt_copy.cpp.
// Host code only: kernels are reached through the launch layer of rt_device.h
// (rt_kernels.hip).  The host float code here (ordered_tree_shape, tri_axis_records, view_of's
// pruning slack) decides kernel variants and bounds: it is built with the kernels' float rules.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "rt_accum.h"
#include "rt_internal.h"

using namespace rtm;
using namespace rtb;
using namespace rtd;
using namespace rti;
using rt::DInst;
using rt::DMesh;
using rt::DTri;

namespace rti {
thread_local int g_device = 0;
namespace {
thread_local std::string g_err;
}
int fail(int code, const std::string& msg) { g_err = msg; return code; }
}  // namespace rti

namespace {
constexpr int BVH_MAX_LEAVES = 1 << 24;  // padded leaves (int indexing of the 12n-float pair records)

int padded(int n_t) {   // raytracer.cu:79: 1 << ceil(log2(n))
    if (n_t <= 0) return 0;
    int n = 1;
    while (n < n_t) n <<= 1;
    return n;
}

int upload_inst4(rt_scene* s);
int ensure_other_slot(rt_scene* s);
int mirror_slot_caps(rt_scene* s);

// TriAx records (rt_math.h) of the axis-plane triangle path: axis, plane coordinate,
// shared-plane flag and the in-plane reject box with its host-checked error bound.
std::vector<TriAx> tri_axis_records(const rt::Scene& h) {
    const double u = 0x1p-24;
    std::vector<TriAx> out(h.d_tris.size());
    auto c3 = [](V3 v, int a) { return a == 0 ? v.x : a == 1 ? v.y : v.z; };
    for (size_t i = 0; i < h.d_tris.size(); i++) {
        const DTri& T = h.d_tris[i];
        TriAx x{};
        x.code = 3;
        int ax = -1, zeros = 0;
        for (int a = 0; a < 3; a++) {
            const float c = c3(T.pn, a);
            if (c == 0.0f) zeros++;                          // +0 or -0
            else if (c == 1.0f || c == -1.0f) ax = a;
        }
        if (zeros == 2 && ax >= 0 && c3(T.b, ax) == c3(T.a, ax) && c3(T.c, ax) == c3(T.a, ax)) {
            x.code = ax;
            x.a_ax = c3(T.a, ax);
            const int au = (ax + 1) % 3, av = (ax + 2) % 3;
            const V3 P[3] = {T.a, T.b, T.c};
            double D = 0, lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
            for (int k = 0; k < 3; k++) {
                const V3 p = P[k], q = P[(k + 1) % 3];
                const double dx = (double)p.x - q.x, dy = (double)p.y - q.y, dz = (double)p.z - q.z;
                D = std::max(D, std::sqrt(dx * dx + dy * dy + dz * dz));
                const double pc[2] = {c3(p, au), c3(p, av)};
                for (int j = 0; j < 2; j++) { lo[j] = std::min(lo[j], pc[j]); hi[j] = std::max(hi[j], pc[j]); }
            }
            // exact (double) doubled area vs the stored float area
            const double e1[3] = {(double)T.b.x - T.a.x, (double)T.b.y - T.a.y, (double)T.b.z - T.a.z};
            const double e2[3] = {(double)T.c.x - T.a.x, (double)T.c.y - T.a.y, (double)T.c.z - T.a.z};
            const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
            const double A = std::sqrt(cx * cx + cy * cy + cz * cz);
            const double m = 1e-4 * D, win = 1e3 * D, off = m;
            bool ok = A > 0 && D > 0 && std::isfinite(A) && std::isfinite(D) && std::isfinite(win);
            if (ok) {
                const double eta = std::fabs((double)T.area - A) / A + 1e-12;
                auto margin = [&](double e) {
                    return (e / D) * (1 - 5.6 * u - eta) - (5.6 * u + eta) - 41.8 * u * (D + e + off) * (D + e + off) / A - 1.01e-5;
                };
                ok = margin(m) > 0 && margin(win) > 0;
            }
            if (ok) {
                // bounds rounded outwards to float
                x.ulo = std::nextafter((float)(lo[0] - m), -INFINITY); x.uhi = std::nextafter((float)(hi[0] + m), INFINITY);
                x.vlo = std::nextafter((float)(lo[1] - m), -INFINITY); x.vhi = std::nextafter((float)(hi[1] + m), INFINITY);
                x.win = std::nextafter((float)win, 0.0f);
                x.off = std::nextafter((float)off, 0.0f);
                x.code |= 8;
            }
        }
        out[i] = x;
    }
    // shared plane with the next triangle of the same mesh
    for (const DMesh& M : h.d_meshes)
        for (int t = M.tri_begin; t + 1 < M.tri_begin + M.tri_count; t++) {
            const TriAx &x = out[t], &y = out[t + 1];
            if ((x.code & 3) != 3 && (x.code & 3) == (y.code & 3)) {
                uint32_t bx, by;
                memcpy(&bx, &x.a_ax, 4); memcpy(&by, &y.a_ax, 4);
                if (bx == by) out[t].code |= 4;
            }
        }
    return out;
}

}  // namespace

// Mesh boxes: Trimesh::compute_bounding_box (trimesh.cu:21-32, sequential fit order) and
// the mesh pose.  They depend only on the immutable mesh data, so they are computed once
// here; the per-frame build (bvh_build_kernel) redoes everything per instance.
std::vector<Box> rti::mesh_boxes(const rt::Scene& h) {
    std::vector<Box> mbox(h.d_meshes.size());
    for (size_t m = 0; m < h.d_meshes.size(); m++) {
        Box b; b.nd = 0; b.mn = b.mx = v3(0, 0, 0);
        const DMesh& mesh = h.d_meshes[m];
        for (int t = mesh.tri_begin; t < mesh.tri_begin + mesh.tri_count; t++) {
            fit_vertex(b, h.d_tris[t].a); fit_vertex(b, h.d_tris[t].b); fit_vertex(b, h.d_tris[t].c);
        }
        mbox[m] = from_local(b, mesh.pose);
    }
    return mbox;
}

namespace {

// Leaf count and depth (internal nodes on the longest root-leaf path) of the ordered
// LBVH bvh_build_kernel will build: the same box, Morton and sort arithmetic on the
// host (RT_HD functions).  The fast traversal's stack holds <= FT_MAX_DEPTH entries (rt_plan.h).
// n_real and the deepest internal node's depth (root = 1).
void ordered_tree_shape(const rt::Scene& h, int* n_real, int* depth) {
    const std::vector<Box> mbox = mesh_boxes(h);
    std::vector<std::pair<unsigned long long, int>> kv;
    bool ordered = true;                                      // every real box finite with mn <= mx
    for (size_t i = 0; i < h.d_insts.size(); i++) {
        const Box b = from_local(mbox[h.d_insts[i].mesh], h.d_insts[i].pose);
        if (b.nd) {
            kv.push_back({z_order(neg(box_center(b))), (int)i});
            const float c[6] = {b.mn.x, b.mn.y, b.mn.z, b.mx.x, b.mx.y, b.mx.z};
            for (float x : c) ordered = ordered && std::isfinite(x);
            ordered = ordered && b.mn.x <= b.mx.x && b.mn.y <= b.mx.y && b.mn.z <= b.mx.z;
        }
    }
    std::stable_sort(kv.begin(), kv.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    const int nr = (int)kv.size();
    *n_real = nr;
    *depth = 0;
    // The fast traversal takes every record of the ordered tree as a proper box (no
    // degenerate / NaN test per child, pair_hit_tt): a pose that makes a box non-finite
    // leaves the frame to the heap kernels.
    if (!ordered) { *depth = 1 << 20; return; }
    if (nr < 2) return;
    std::vector<unsigned long long> keys(nr);
    for (int i = 0; i < nr; i++) keys[i] = kv[i].first;
    std::vector<int> child(2 * (nr - 1));                   // internal children (-1: leaf)
    for (int i = 0; i < nr - 1; i++) {
        int first, last, gamma;
        fnode_split(keys.data(), nr, i, first, last, gamma);
        child[2 * i] = gamma + 1 == last ? -1 : gamma + 1;
        child[2 * i + 1] = gamma == first ? -1 : gamma;
    }
    std::vector<std::pair<int, int>> todo{{0, 1}};
    while (!todo.empty()) {
        const auto [node, d] = todo.back();
        todo.pop_back();
        *depth = std::max(*depth, d);
        if (d > nr) { *depth = 1 << 20; return; }          // malformed: disable the fast tree
        for (int c = 0; c < 2; c++) if (child[2 * node + c] >= 0) todo.push_back({child[2 * node + c], d + 1});
    }
}

}  // namespace

// The scene's own stream, created on first use: a caller passing its own streams (frame
// pipelining) keeps every HIP stream of the process on a hardware queue of its own
// (GPU_MAX_HW_QUEUES = 4; streams beyond that share queues and serialise).
hipStream_t rti::sstream(rt_scene* s) {
    if (!s->stream) (void)hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    return s->stream;
}

int rti::upload(rt_scene* s) {
    if (s->uploaded) return RT_OK;
    FrameSlot& f = s->cur();
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(RT_ERR_NODEV, "no HIP device available");
    s->device = g_device;
    HIPCHK(hipSetDevice(s->device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, s->device));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
        return fail(RT_ERR_NODEV, std::string("device is ") + prop.gcnArchName + ", this build targets gfx950");
    for (auto& e : s->ev) HIPCHK(hipEventCreate(&e));
    const rt::Scene& h = s->h;
    auto up = [&](auto*& dst, const auto& vec) -> int {
        using T = typename std::remove_reference<decltype(vec)>::type::value_type;
        size_t bytes = std::max<size_t>(1, vec.size()) * sizeof(T);
        HIPCHK(hipMalloc((void**)&dst, bytes));
        if (!vec.empty()) HIPCHK(hipMemcpy(dst, vec.data(), vec.size() * sizeof(T), hipMemcpyHostToDevice));
        return RT_OK;
    };
    int r;
    if ((r = up(s->d_tris, h.d_tris)) || (r = up(s->d_meshes, h.d_meshes)) || (r = up(f.d_insts, h.d_insts)) ||
        (r = up(s->d_mats, h.d_mats)) || (r = up(s->d_lights, h.d_lights)))
        return r;
    s->n_leaf = padded((int)h.d_insts.size());
    if (s->n_leaf > BVH_MAX_LEAVES) return fail(RT_ERR_LIMIT, "more than 2^24 padded instances");
    s->n_cu = prop.multiProcessorCount;
    size_t nl = std::max(1, s->n_leaf);
    HIPCHK(hipMalloc((void**)&f.d_node_pair, 3 * nl * sizeof(float4)));
    ordered_tree_shape(h, &s->n_real, &s->fdepth);
    s->shape_gen = s->inst_gen;
    HIPCHK(hipMalloc((void**)&f.d_fnode, 4 * (size_t)std::max(1, s->n_real - 1) * sizeof(float4)));
    HIPCHK(hipMalloc((void**)&f.d_leaf, nl * sizeof(int)));
    HIPCHK(hipMalloc((void**)&f.d_inst4, std::max<size_t>(1, h.d_insts.size()) * sizeof(float4)));
    HIPCHK(hipMalloc((void**)&f.d_work, WORK_INTS * sizeof(int)));
    if ((r = upload_inst4(s)) != RT_OK) return r;
    if ((r = up(s->d_tri_ax, tri_axis_records(h))) != RT_OK) return r;
    if ((r = up(s->d_mesh_box, mesh_boxes(h))) != RT_OK) return r;
    HIPCHK(hipMalloc((void**)&f.d_tree, 2 * nl * sizeof(Box)));
    if (s->n_leaf > BVH_WG_LEAVES) HIPCHK(hipMalloc(&f.d_bscratch, bvh_large_scratch_bytes(s->n_leaf)));
    HIPCHK(hipMalloc((void**)&s->d_stats, STATS_N * sizeof(unsigned long long)));
    // the occluder hint table (rt_plan.h: hint_*), empty; scenes of the grid-wide BVH build get none.
    // The instance set is fixed once the scene is finished: moved instances leave stale entries,
    // which the kernels check, replace and clear themselves.
    if (s->n_leaf <= BVH_WG_LEAVES && !h.d_insts.empty()) {
        HIPCHK(hipMalloc((void**)&s->d_hint, hint_bytes((int)h.d_insts.size())));
        HIPCHK(hipMemset(s->d_hint, 0, hint_bytes((int)h.d_insts.size())));
    }
    HIPCHK(hipMalloc((void**)&s->d_canvas, (size_t)h.cam.W * h.cam.H * sizeof(uint32_t)));
    HIPCHK(hipMalloc((void**)&s->d_dbg, 4096 * sizeof(int)));
    for (auto& o : s->slots) if (!o.done) HIPCHK(hipEventCreateWithFlags(&o.done, hipEventDisableTiming));
    f.inst_gen = s->inst_gen;
    s->uploaded = true;
    if (s->n_slots > 1) return ensure_other_slot(s);
    return RT_OK;
}

namespace {

// compact instance records for the trace kernel: (p, mesh | 0x80000000 when the pose is not identity)
void fill_inst4(const rt::Scene& h, float4* v) {
    for (size_t i = 0; i < h.d_insts.size(); i++) {
        const DInst& d = h.d_insts[i];
        uint32_t w = (uint32_t)d.mesh | (d.pose.identity ? 0u : 0x80000000u);
        float fw; memcpy(&fw, &w, 4);
        v[i] = make_float4(d.pose.p.x, d.pose.p.y, d.pose.p.z, fw);
    }
}
int upload_inst4(rt_scene* s) {
    std::vector<float4> v(s->h.d_insts.size());
    fill_inst4(s->h, v.data());
    if (!v.empty()) HIPCHK(hipMemcpy(s->cur().d_inst4, v.data(), v.size() * sizeof(float4), hipMemcpyHostToDevice));
    return RT_OK;
}

// Bring the current slot's instance arrays to the host's generation, stream-ordered on `st`
// (after the slot's previous frame, which the caller has made `st` wait for).  The pinned
// staging is rewritten only once the copy that last read it has run (the slot's last frame,
// recorded after that copy).
int sync_slot_insts(rt_scene* s, hipStream_t st) {
    FrameSlot& f = s->cur();
    if (f.inst_gen == s->inst_gen) return RT_OK;
    const size_t n = s->h.d_insts.size();
    if (n) {
        if (!f.h_insts_pin) {
            HIPCHK(hipHostMalloc((void**)&f.h_insts_pin, n * sizeof(DInst), hipHostMallocDefault));
            HIPCHK(hipHostMalloc((void**)&f.h_inst4_pin, n * sizeof(float4), hipHostMallocDefault));
            int r;
            if (s->n_slots > 1 && (r = mirror_slot_caps(s)) != RT_OK) return r;
        } else if (f.pending) {
            HIPCHK(hipEventSynchronize(f.done));
        }
        memcpy(f.h_insts_pin, s->h.d_insts.data(), n * sizeof(DInst));
        fill_inst4(s->h, f.h_inst4_pin);
        HIPCHK(hipMemcpyAsync(f.d_insts, f.h_insts_pin, n * sizeof(DInst), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(f.d_inst4, f.h_inst4_pin, n * sizeof(float4), hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(f.done, st));   // covers the staging until the frame records it again
        f.pending = true;
    }
    f.inst_gen = s->inst_gen;
    return RT_OK;
}

// Ordered-LBVH shape (leaf count, depth) for the current host poses: instances that moved
// change the Morton order and with it the tree depth the fast traversal's stack must hold.
void refresh_shape(rt_scene* s) {
    if (s->shape_gen == s->inst_gen) return;
    int nr = 0;
    ordered_tree_shape(s->h, &nr, &s->fdepth);
    s->shape_gen = s->inst_gen;
}

// Begin a frame on the current slot: `st` waits for the slot's previous frame (all slots'
// last frames for side entries that do not rotate slots), then the slot's instances are
// brought up to date.  end_frame records the slot's completion.
int begin_frame(rt_scene* s, hipStream_t st, bool all_slots) {
    for (int i = 0; i < rt_scene::MAX_SLOTS; i++)
        if (s->slots[i].pending && (all_slots || i == s->cur_slot)) HIPCHK(hipStreamWaitEvent(st, s->slots[i].done, 0));
    refresh_shape(s);
    return sync_slot_insts(s, st);
}

// Buffers of the frame slots other than the current one (sizes as in upload), slot events.
int ensure_other_slot(rt_scene* s) {
    const size_t nl = std::max(1, s->n_leaf);
    for (int i = 0; i < s->n_slots; i++) {
        FrameSlot& o = s->slots[i];
        if (i == s->cur_slot || o.d_work) continue;
        HIPCHK(hipMalloc((void**)&o.d_node_pair, 3 * nl * sizeof(float4)));
        HIPCHK(hipMalloc((void**)&o.d_fnode, 4 * (size_t)std::max(1, s->n_real - 1) * sizeof(float4)));
        HIPCHK(hipMalloc((void**)&o.d_leaf, nl * sizeof(int)));
        HIPCHK(hipMalloc((void**)&o.d_tree, 2 * nl * sizeof(Box)));
        HIPCHK(hipMalloc((void**)&o.d_work, WORK_INTS * sizeof(int)));
        HIPCHK(hipMalloc((void**)&o.d_insts, std::max<size_t>(1, s->h.d_insts.size()) * sizeof(DInst)));
        HIPCHK(hipMalloc((void**)&o.d_inst4, std::max<size_t>(1, s->h.d_insts.size()) * sizeof(float4)));
        // the grid-wide build's sort buffers now, not at the slot's first frame inside a pipeline
        if (s->n_leaf > BVH_WG_LEAVES && !o.d_bscratch) HIPCHK(hipMalloc(&o.d_bscratch, bvh_large_scratch_bytes(s->n_leaf)));
        // the current poses now (blocking copies, here rather than at the slot's first frame: an
        // asynchronous copy on a frame's stream may start a new SDMA engine, ~7 ms of host time
        // the first time, profiles/r06/rblog/); later pose changes reach the slot through
        // sync_slot_insts, stream-ordered
        const size_t n = s->h.d_insts.size();
        if (n) {
            std::vector<float4> v4(n);
            fill_inst4(s->h, v4.data());
            HIPCHK(hipMemcpy(o.d_insts, s->h.d_insts.data(), n * sizeof(DInst), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(o.d_inst4, v4.data(), n * sizeof(float4), hipMemcpyHostToDevice));
        }
        o.inst_gen = s->inst_gen;
        o.work_zeroed = false; o.bvh_valid = false;
    }
    return mirror_slot_caps(s);                              // the current slot's grown buffers too
}

// Slot f's sky flags, live lists and scheduling history brought to at least the given
// capacities (0: that buffer is not wanted).  `synced` (another slot's buffers, which a frame in
// flight may be using): the device is waited for once per call, *synced, before a smaller
// buffer is freed.  A regrown history is reset at the slot's next use (the key).  *grew
// (optional) is set when a buffer grew.
int grow_slot(FrameSlot& f, int gsky_cap, int live_cap, int hist_cap, bool* synced, bool* grew) {
    auto quiesce = [&](const void* old) -> hipError_t {
        if (!old || !synced || *synced) return hipSuccess;
        *synced = true;
        return hipDeviceSynchronize();
    };
    if (gsky_cap > f.gsky_cap) {
        HIPCHK(quiesce(f.d_gsky));
        dfree(f.d_gsky);
        HIPCHK(hipMalloc((void**)&f.d_gsky, gsky_cap));
        f.gsky_cap = gsky_cap; if (grew) *grew = true;
    }
    if (live_cap > f.live_cap) {
        HIPCHK(quiesce(f.d_live));
        dfree(f.d_live);
        HIPCHK(hipMalloc((void**)&f.d_live, (size_t)live_cap * sizeof(int)));
        f.live_cap = live_cap; if (grew) *grew = true;
    }
    if (hist_cap > f.hist_cap) {
        HIPCHK(quiesce(f.d_hctl));
        for (int p = 0; p < 2; p++) { dfree(f.d_hlist[p]); dfree(f.d_hflag[p]); }
        dfree(f.d_hctl);
        for (int p = 0; p < 2; p++) {
            HIPCHK(hipMalloc((void**)&f.d_hlist[p], (size_t)hist_cap * sizeof(int)));
            HIPCHK(hipMalloc((void**)&f.d_hflag[p], hist_cap));
        }
        HIPCHK(hipMalloc((void**)&f.d_hctl, 4 * sizeof(unsigned long long)));
        f.hist_cap = hist_cap;
        f.hist_key[0] = -1;
        if (grew) *grew = true;
    }
    return RT_OK;
}

// The current slot grew a per-frame buffer (sky flags, live lists, history, pinned instance
// staging) at its first frame of a new layout: give every other allocated slot the same
// capacity now, so that their first frames -- possibly inside a steady pipeline -- allocate
// nothing (an allocation there cost the first 8 frames of a run up to ~1 ms: hipFree waits for
// the device, pinned allocations take milliseconds).  The slots' contents are reset on first
// use as before (history key, instance generation).  Only growth reaches here: waiting for the
// device before freeing a smaller buffer is a one-time cost per layout.
int mirror_slot_caps(rt_scene* s) {
    const FrameSlot& c = s->cur();
    const size_t n = s->h.d_insts.size();
    bool synced = false;
    for (int i = 0; i < s->n_slots; i++) {
        FrameSlot& o = s->slots[i];
        if (i == s->cur_slot || !o.d_work) continue;          // itself; not allocated (ensure_other_slot)
        int r;
        if ((r = grow_slot(o, c.gsky_cap, c.live_cap, c.hist_cap, &synced, nullptr)) != RT_OK) return r;
        if (c.h_insts_pin && !o.h_insts_pin && n) {
            HIPCHK(hipHostMalloc((void**)&o.h_insts_pin, n * sizeof(DInst), hipHostMallocDefault));
            HIPCHK(hipHostMalloc((void**)&o.h_inst4_pin, n * sizeof(float4), hipHostMallocDefault));
        }
    }
    return RT_OK;
}

// The current slot's layout buffers for n_groups pixel groups (sky: flags and live lists; hist:
// the scheduling history), and on growth every other allocated slot's (mirror_slot_caps).
int ensure_layout(rt_scene* s, int n_groups, bool sky, bool hist) {
    const Layout l = layout_of(n_groups);
    bool grew = false;
    int r = grow_slot(s->cur(), sky ? l.flags : 0, sky ? l.live : 0, hist ? l.flags : 0, nullptr, &grew);
    if (r != RT_OK) return r;
    return (grew && s->n_slots > 1) ? mirror_slot_caps(s) : RT_OK;
}

// Atlas -> float4 texels (byte / 255, as assets.cc:61-81) in HBM; the reference's CUDA
// texture (gputils TextureBuffer4D, alloc.h:24-80: point sampling, clamp) is sampled
// explicitly by hit_kd, since gfx950 has no texture units.
void free_atlas(rt_scene* s) {
    if (s->d_atlas) (void)hipFree(s->d_atlas);
    s->d_atlas = nullptr;
}
int ensure_atlas(rt_scene* s) {
    const rt::Scene& h = s->h;
    if (h.atlas_rgba.empty()) return fail(RT_ERR_STATE, "textured rendering needs an atlas: rt_scene_load_atlas / rt_scene_set_atlas");
    if (!s->atlas_dirty && s->d_atlas) return RT_OK;
    free_atlas(s);
    const size_t n = (size_t)h.atlas_w * h.atlas_h;
    std::vector<float4> texels(n);
    for (size_t i = 0; i < n; i++)
        texels[i] = make_float4((float)h.atlas_rgba[4 * i] / 255, (float)h.atlas_rgba[4 * i + 1] / 255,
                                (float)h.atlas_rgba[4 * i + 2] / 255, (float)h.atlas_rgba[4 * i + 3] / 255);
    HIPCHK(hipMalloc((void**)&s->d_atlas, n * sizeof(float4)));
    HIPCHK(hipMemcpy(s->d_atlas, texels.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    s->atlas_dirty = false;
    return RT_OK;
}

// (Re)allocate / reset the current slot's scheduling history when the launch layout changes.
int ensure_history(rt_scene* s, int n_groups, const long long* key, hipStream_t st) {
    int r;
    if ((r = ensure_layout(s, n_groups, false, true)) != RT_OK) return r;
    FrameSlot& f = s->cur();
    if (memcmp(key, f.hist_key, sizeof f.hist_key) != 0) {
        for (int p = 0; p < 2; p++) HIPCHK(hipMemsetAsync(f.d_hflag[p], 0, f.hist_cap, st));
        HIPCHK(hipMemsetAsync(f.d_hctl, 0, 4 * sizeof(unsigned long long), st));
        memcpy(f.hist_key, key, sizeof f.hist_key);
        f.hist_parity = 0;
    }
    return RT_OK;
}

// Per-frame buffers (sky flags, live lists, scheduling history) sized for a layout of n_groups
// pixel groups in the current slot and every allocated one, ahead of the first frame that needs
// them (warm_scene: the whole frame at 2-8 pixels per wave, the layouts of spp 8-32).  Contents
// are reset at first use as before (the history key); only capacity is reserved here.
int reserve_layout(rt_scene* s, int n_groups) { return ensure_layout(s, n_groups, true, true); }

int ensure_spp(rt_scene* s, int spp) {
    if (spp <= s->spp_cap) return RT_OK;
    int cap = std::max(spp, 64);
    std::vector<float2> tab(cap);
    for (int k = 0; k < cap; k++) rt::spp_offset(k, &tab[k].x, &tab[k].y);
    dfree(s->d_spp);
    HIPCHK(hipMalloc((void**)&s->d_spp, cap * sizeof(float2)));
    HIPCHK(hipMemcpy(s->d_spp, tab.data(), cap * sizeof(float2), hipMemcpyHostToDevice));
    s->spp_cap = cap;
    return RT_OK;
}

// The pruning slack (closest_hit) for rays starting within origin_amax (largest |coordinate|) of
// the world's origin, or -1 when the boxes do not provably contain their triangles: that holds
// only for pure translations with zero mesh offsets (the BVH boxes ignore the mesh pose,
// raytracer.cu:54-89).  Slack: 4e-4 x mesh size + 2^-14 x scene radius.
float prune_slack(const rt_scene* s, float origin_amax) {
    bool prune_ok = true;
    for (const auto& i : s->h.d_insts) prune_ok = prune_ok && i.pose.identity;
    for (const auto& m : s->h.d_meshes) prune_ok = prune_ok && m.pose.identity;
    float vmax = 0.0f, pmax = 0.0f;
    for (const auto& m : s->h.d_meshes) prune_ok = prune_ok && m.pose.p.x == 0 && m.pose.p.y == 0 && m.pose.p.z == 0;
    auto amax = [](rtm::V3 a) { return std::max(std::fabs(a.x), std::max(std::fabs(a.y), std::fabs(a.z))); };
    for (const auto& t : s->h.d_tris) vmax = std::max(vmax, std::max(amax(t.a), std::max(amax(t.b), amax(t.c))));
    for (const auto& i : s->h.d_insts) pmax = std::max(pmax, amax(i.pose.p));
    const float radius = pmax + vmax + origin_amax + 1.0f;
    prune_ok = prune_ok && std::isfinite(radius);
    return prune_ok ? 4e-4f * vmax + 0x1p-14f * radius : -1.0f;
}

// Bind the slot's scheduling history for a frame of mode `hist` (history_mode: 1 or 2): the
// previous frame's buffers to read, the other parity's to record into.  Returns that parity,
// which is the slot's from now on.
int bind_history(TraceParams& P, FrameSlot& f, int hist, int heavy_q) {
    const int prev = f.hist_parity, next = 1 - prev;
    P.hist = hist;
    P.heavy_q = heavy_q;
    P.hl_prev = f.d_hlist[prev]; P.hl_next = f.d_hlist[next];
    P.hf_prev = f.d_hflag[prev]; P.hf_next = f.d_hflag[next];
    P.hctl_prev = f.d_hctl + 2 * prev; P.hctl_next = f.d_hctl + 2 * next;
    f.hist_parity = next;
    return next;
}

}  // namespace

// What the other host files call (declared in rt_internal.h) from here on.

int rti::end_frame(rt_scene* s, hipStream_t st) {
    HIPCHK(hipEventRecord(s->cur().done, st));
    s->cur().pending = true;
    return RT_OK;
}

Layout rti::layout_of(int n_groups) {
    Layout l;
    l.sky_blocks = (n_groups + 63) / 64;                       // sky_kernel's blocks, 64 groups each
    l.flags = (std::max(n_groups, 1024) + 3) & ~3;             // sky and history flags: whole dwords (scalar loads)
    l.live_q = (l.sky_blocks + NQ - 1) / NQ * 64;                  // most groups of the blocks b = q mod NQ
    l.live = l.live_q * NQ + n_groups;                         // + the heavy live list (hist = 2)
    return l;
}

// Device staging of host_outputs frames (rgba, radiance, hit_inst, hit_tri), whole-frame sized.
int rti::ensure_out_staging(rt_scene* s) {
    const size_t px = (size_t)s->h.cam.W * s->h.cam.H;
    if (s->d_out_px >= px) return RT_OK;
    for (auto& p : s->d_out) dfree(p);
    s->d_out_px = 0;
    HIPCHK(hipMalloc(&s->d_out[0], px * 4)); HIPCHK(hipMalloc(&s->d_out[1], px * 16));
    HIPCHK(hipMalloc(&s->d_out[2], px * 4)); HIPCHK(hipMalloc(&s->d_out[3], px * 4));
    s->d_out_px = px;
    return RT_OK;
}

int rti::build_bvh(rt_scene* s, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    FrameSlot& f = s->cur();
    if (s->n_leaf == 0) {
        if (e0) { HIPCHK(hipEventRecord(e0, st)); HIPCHK(hipEventRecord(e1, st)); }
        f.bvh_valid = true;
        return RT_OK;
    }
    BvhArgs A;
    A.insts = f.d_insts; A.n_inst = (int)s->h.d_insts.size();
    A.mesh_box = s->d_mesh_box; A.n = s->n_leaf;
    A.tree = f.d_tree;
    A.node_pair = reinterpret_cast<float*>(f.d_node_pair); A.leaf_inst = f.d_leaf;
    A.fnode = f.d_fnode; A.n_real = s->n_real;
    A.work = f.d_work; A.n_work = WORK_INTS;
    // the slot the next fast frame records its heavy list into (launch_trace skips its memset)
    A.hctl = f.d_hctl ? f.d_hctl + 2 * (1 - f.hist_parity) : nullptr;
    f.hctl_zeroed = f.d_hctl ? 1 - f.hist_parity : -1;
    const int form = bvh_form(A.n, A.n_inst, BVH_WG_LEAVES);
    if (form == BVH_FORM_GRID) {                              // above one workgroup's LDS: the grid-wide build
        if (!f.d_bscratch) HIPCHK(hipMalloc(&f.d_bscratch, bvh_large_scratch_bytes(A.n)));
        HIPCHK(bvh_build_large(A, f.d_bscratch, st, e0, e1));
    } else {
        const bool lds_tree = form != BVH_FORM_HBM;                         // n <= 2048
        const size_t lds = bvh_lds_bytes(A.n, lds_tree);
        if (lds > BVH_LDS_MAX) return fail(RT_ERR_LIMIT, "BVH build needs more LDS than one CU has");
        HIPCHK(launch_bvh_build(A, lds_tree, lds, st, e0, e1));
        HIPCHK(hipGetLastError());
    }
    f.bvh_valid = true;
    f.work_zeroed = true;
    // what RT_EXPORT_BVH_* reads back (host state): the slot, and the shape this build was given
    s->built = {s->cur_slot, s->n_real, s->fdepth, form};
    return RT_OK;
}

SceneView rti::view_of(const rt_scene* s, bool use_bvh) {
    const FrameSlot& f = s->cur();
    SceneView v;
    v.tris = s->d_tris; v.meshes = s->d_meshes; v.insts = f.d_insts; v.mats = s->d_mats; v.lights = s->d_lights;
    v.node_pair = f.d_node_pair; v.leaf_inst = f.d_leaf;
    v.fnode = f.d_fnode; v.n_real = s->n_real;
    v.ftree = ordered_tree_usable(s->n_real, s->fdepth) ? 1 : 0; v.inst4 = f.d_inst4;
    v.n_leaf = s->n_leaf; v.n_inst = (int)s->h.d_insts.size();
    v.n_lights = (int)s->h.d_lights.size(); v.use_bvh = use_bvh ? 1 : 0;
    v.n_mats = (int)s->h.d_mats.size(); v.n_tris = (int)s->h.d_tris.size(); v.n_meshes = (int)s->h.d_meshes.size();
    v.ident_all = 1;
    for (const auto& i : s->h.d_insts) v.ident_all &= i.pose.identity ? 1 : 0;
    for (const auto& m : s->h.d_meshes) v.ident_all &= m.pose.identity ? 1 : 0;
    // Distance pruning (closest_hit): the camera's rays
    const rtm::V3 cp = s->h.d_cam.pos;
    v.prune_abs = prune_slack(s, std::max(std::fabs(cp.x), std::max(std::fabs(cp.y), std::fabs(cp.z))));
    v.tri_ax = (v.ident_all && !s->h.d_tris.empty()) ? s->d_tri_ax : nullptr;
    v.hint = nullptr;                                          // (launch_trace binds the table)
    v.nf_ctr = nullptr; v.near_first = NF_OFF; v.nf_pad = 0;   // (and the near-first mode and counters)
    return v;
}

// The view for rays a caller supplies (rt_query, rt_occlusion) with the two floats their kernels
// take.  The camera-ray shortcuts are off: view_of's pruning slack folds |cam.pos| in and the
// axis-plane path's error bound is checked for rays from there; a caller's origin is anywhere.
// The zero-axis cut alone stays, with the origin's term added per ray on the device.  The
// occlusion early exit's margin: one rescaling per instance at most, each < 1 + 2^-20.
CallerView rti::caller_ray_view(const rt_scene* s, bool use_bvh) {
    CallerView c{view_of(s, use_bvh), prune_slack(s, 0.0f), 0.0f};
    c.S.prune_abs = -1.0f; c.S.tri_ax = nullptr;
    const float margin = (float)c.S.n_inst * 0x1p-19f;
    c.any_margin = margin <= 0.125f ? margin : -1.0f;
    return c;
}

int rti::scene_atlas(rt_scene* s) { return ensure_atlas(s); }

// Fill TraceParams from the launch plan (rt_plan.h), ensure the slot's buffers, launch.
int rti::launch_trace(rt_scene* s, const rt_render_opts& o, const TraceRequest& q) {
    hipStream_t st = q.stream;
    FrameSlot& f = s->cur();
    const rt::Scene& h = s->h;
    const FrameGeometry g = frame_geometry(h.cam.W, h.cam.H, o.row0, o.row_step, o.spp);
    if (g.n_rows <= 0) {
        if (q.e0) { HIPCHK(hipEventRecord(q.e0, st)); HIPCHK(hipEventRecord(q.e1, st)); }
        return RT_OK;
    }
    TraceParams P{};
    P.gdur = q.gdur;
    P.cam = h.d_cam; P.dist_atten = h.dist_atten; P.ambience = h.ambience;
    P.W = h.cam.W; P.H = h.cam.H; P.row0 = o.row0; P.row_step = o.row_step; P.n_rows = g.n_rows;
    P.compact = o.compact; P.spp = o.spp; P.depth = h.depth;
    P.spp_recip = rta::mean_recip(o.spp);
    if (q.k0 != 0 && (o.spp != 1 || q.dbg)) return fail(RT_ERR_ARG, "a sample base needs a 1-spp launch without a debug pixel");
    P.k0 = q.k0;
    P.spp_off = s->d_spp;
    P.rgba = q.rgba; P.radiance = reinterpret_cast<float4*>(o.radiance); P.hit_inst = o.hit_inst; P.hit_tri = o.hit_tri;
    P.stats = (q.want_stats || q.prof) ? s->d_stats : nullptr; P.dbg_log = q.dbg; P.dbg_x = q.dbg_x; P.dbg_y = q.dbg_y;
    if (o.textures) {
        int r;
        if ((r = ensure_atlas(s)) != RT_OK) return r;
        P.atlas = s->d_atlas; P.atlas_w = s->h.atlas_w; P.atlas_h = s->h.atlas_h;
    }
    SceneView S = view_of(s, o.use_bvh != 0);
    S.hint = s->shadow_hints ? s->d_hint : nullptr;
    // nearer child first: only where the pruning claim holds (closest_hit); counted in the hint block's stripes
    S.near_first = S.prune_abs >= 0.0f ? s->near_first : NF_OFF;
    S.nf_ctr = s->d_hint ? reinterpret_cast<unsigned long long*>(s->d_hint + hint_table_ints(S.n_inst)) : nullptr;
    P.lanes_per_px = g.lanes_per_px; P.px_per_wave = g.px_per_wave; P.gw = g.gw; P.gh = g.gh;
    P.l_shift = g.l_shift; P.gw_shift = g.gw_shift; P.n_gx = g.n_gx; P.n_groups = g.n_groups;
    if (q.geo) { q.geo[0] = g.n_groups; q.geo[1] = g.gw; q.geo[2] = g.gh; q.geo[3] = g.n_gx; }
    P.scramble = g.scramble; P.scramble_small = g.scramble_small;
    P.div_ngx = g.div_ngx; P.div_perq = g.div_perq;
    P.work = f.d_work; P.tpc = TPC;
    const ShadeShortcuts sc = shade_shortcuts(h, q.want_stats, q.dbg != nullptr, q.occl_force);
    P.unlit_skip = sc.unlit_skip; P.occl_exit = sc.occl_exit;
    if (!q.lists && !f.work_zeroed) HIPCHK(hipMemsetAsync(f.d_work, 0, WORK_INTS * sizeof(int), st));
    const TraceVariant V = choose_trace_variant(S, o.spp, o.textures != 0, q.want_stats, q.prof, sc.ns);
    if (!V.fn)
        return fail(RT_ERR_STATE, "no trace kernel <" + std::to_string(V.ns_bucket) + ", " + std::to_string((int)V.lds) + ", " +
                                      std::to_string(V.mode) + ">");
    const bool listed = q.lists && V.sky;
    if (q.listed) *q.listed = listed;
    if (listed) HIPCHK(hipMemcpyAsync(f.d_work, q.lists_work, WORK_INTS * sizeof(int), hipMemcpyDeviceToDevice, st));
    else if (q.lists && !f.work_zeroed) HIPCHK(hipMemsetAsync(f.d_work, 0, WORK_INTS * sizeof(int), st));
    // another frame of the scene still in flight (grid_policy)
    bool other_running = false;
    for (int i = 1; i < s->n_slots && !other_running; i++) {
        const int sl = (s->cur_slot + s->n_slots - i) % s->n_slots;
        other_running = s->slots[sl].pending && hipEventQuery(s->slots[sl].done) == hipErrorNotReady;
    }
    const GridPlan grid = grid_policy(s->n_cu, V.per_cu, (listed && q.lists_n > 0) ? q.lists_n : g.n_groups, s->n_slots, s->overlap, other_running, s->ranks_per_device);
    P.grid_waves = grid.grid_waves; P.heavy_static = grid.heavy_static; P.heavy_cap = grid.heavy_cap;
    static const int heavy_q = [] { const char* e = getenv("RT_HEAVY_Q"); return e ? atoi(e) : RT_HEAVY_Q_DEFAULT; }();
    const long long full_waves = (long long)s->n_cu * V.per_cu * (TRACE_BLOCK_P / 64);
    const int hist = listed ? 0 : history_mode(q.want_stats, q.dbg != nullptr, V.sky, q.prof, heavy_q, g.n_groups, full_waves);
    if (hist) {
        const long long key[8] = {P.W, P.H, P.row0, P.row_step, P.n_rows, P.spp, P.n_groups, (long long)o.textures | hist << 8};
        int r;
        if ((r = ensure_history(s, P.n_groups, key, st)) != RT_OK) return r;
        const int next = bind_history(P, f, hist, heavy_q);
        if (hist == 1 && f.hctl_zeroed != next) HIPCHK(hipMemsetAsync(f.d_hctl + 2 * next, 0, 2 * sizeof(unsigned long long), st));
    }
    f.work_zeroed = false;                                    // this launch consumes the counters
    if (!listed) f.hctl_zeroed = -1;
    if (listed) {
        P.live = q.lists; P.live_cap = q.lists_cap;
        P.tpc = RT_TPC_LIVE;
    } else if (V.sky) {
        int r;
        if ((r = ensure_layout(s, P.n_groups, true, false)) != RT_OK) return r;
        const Layout l = layout_of(P.n_groups);
        P.gsky = f.d_gsky;
        P.live = f.d_live; P.live_cap = l.live_q;
        P.tpc = (V.part_k && P.lanes_per_px == 64) ? RT_TPC_WIDE : RT_TPC_LIVE;
        // (brute-force frames: the grown boxes' slack)
        HIPCHK(launch_sky(V.sky_brute, l.sky_blocks, P, S, f.d_gsky, f.d_live, s->d_mesh_box, S.prune_abs, 0x1p-12f, st, q.e0));
    }
    HIPCHK(launch_trace_kernel(V, grid.blocks, P, S, st, (V.sky && !listed) ? nullptr : q.e0, q.e1));
    HIPCHK(hipGetLastError());
    s->last_key = V; s->last_ftree = S.ftree; s->has_last_trace = true;   // rt_scene_last_trace
    return RT_OK;
}

// The side entries' prologue (debug_cast, experiments, profiles; they do not rotate slots): the
// scene on its device, the sample offsets, the scene's stream waiting for every frame in flight
// (any slot), and with `bvh` the current slot's BVH rebuilt.
int rti::begin_side_entry(rt_scene* s, int spp, bool bvh) {
    int r;
    if ((r = upload(s)) != RT_OK) return r;
    HIPCHK(hipSetDevice(s->device));
    if ((r = ensure_spp(s, spp)) != RT_OK) return r;
    if ((r = begin_frame(s, sstream(s), true)) != RT_OK) return r;   // nothing else in flight on this slot
    return bvh ? build_bvh(s, sstream(s)) : RT_OK;
}

// Zero the counters; the two minima (slots 15 and 19: the waves' earliest start and earliest end,
// trace_kernel) start at all ones.
int rti::clear_stats(rt_scene* s, hipStream_t st) {
    HIPCHK(hipMemsetAsync(s->d_stats, 0, STATS_N * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(s->d_stats + 15, 0xff, sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(s->d_stats + 19, 0xff, sizeof(unsigned long long), st));
    return RT_OK;
}

// A counted frame's epilogue (rt_render, rt_query), after the stream's sync: the four counters,
// and the BVH and trace times between ev[0], ev[1] and ev[2].
int rti::read_frame_stats(rt_scene* s, rt_stats* stats) {
    unsigned long long v[4];
    HIPCHK(hipMemcpy(v, s->d_stats, sizeof v, hipMemcpyDeviceToHost));
    stats->rays = v[0]; stats->nodes = v[1]; stats->leaves = v[2]; stats->tri_tests = v[3];
    float a = 0, b = 0;
    HIPCHK(hipEventElapsedTime(&a, s->ev[0], s->ev[1]));
    HIPCHK(hipEventElapsedTime(&b, s->ev[1], s->ev[2]));
    stats->bvh_ms = a; stats->trace_ms = b;
    return RT_OK;
}

// procedural::gpu::generate / SceneBuilder::build_gpu_scene put the scene on the device when it
// is made (cube_world.cc:195-207, scene_builder.cu:29-81); the first update_scene then only
// renders.  Here the upload is lazy (host-only scenes must load without a GPU), so a finished
// scene on a machine with a gfx950 device is uploaded at once and one untimed 1-spp frame is
// rendered into the device canvas: the code object, the scene's stream and the frame layout's
// buffers (sky flags, live lists, scheduling history) are then in place before the caller's
// first frame.  Without a usable device nothing happens (render calls report RT_ERR_NODEV as
// before); a failure here is left for the first render to report.  RT_NO_WARM=1 turns it off.
int rti::warm_scene(rt_scene* s) {
    static const bool off = [] { const char* e = getenv("RT_NO_WARM"); return e && atoi(e) != 0; }();
    int n = 0;
    if (off || hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); return RT_OK; }
    const std::string saved = g_err;
    // update_scene's own path: a 1-spp frame and its copy into the pinned canvas (the copy starts
    // the copy engine's queue for device-to-host transfers, ~7 ms the first time)
    if (s->h.cam.W > 0 && s->h.cam.H > 0 && rt_update_scene(s, 16, 1) != RT_OK) {
        g_err = saved;                                    // left for the caller's first render to report
        (void)hipGetLastError();
        return RT_OK;
    }
    // capacity for the whole frame at 8 pixels per wave (4 x 2 groups: 8-32 spp, the bench's layout)
    const long long groups = (long long)((s->h.cam.W + 3) / 4) * ((s->h.cam.H + 1) / 2);
    if (groups < (1ll << 26) && reserve_layout(s, (int)groups) != RT_OK) { g_err = saved; (void)hipGetLastError(); }
    return RT_OK;
}

void rti::invalidate(rt_scene* s) {
    for (auto& f : s->slots) f.bvh_valid = false;
}

rt_scene::~rt_scene() {
    free_multi(this);
    if (uploaded) (void)hipSetDevice(device);
    free_atlas(this);
    dfree(d_tris); dfree(d_meshes); dfree(d_mats); dfree(d_lights); dfree(d_tri_ax);
    dfree(d_mesh_box); dfree(d_spp); dfree(d_stats); dfree(d_hint); dfree(d_canvas); dfree(d_dbg);
    for (auto& p : d_out) dfree(p);
    query.release();
    shade.release();
    accum.release();
    occl.release();
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : tev) (void)hipEventDestroy(e);
    for (auto& f : slots) f.release();
    if (stream) (void)hipStreamDestroy(stream);
}

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }
const char* rt_last_error(void) { return g_err.c_str(); }

int rt_device_count(int* count) {
    if (!count) return fail(RT_ERR_ARG, "null count");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return RT_OK;
}

int rt_set_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(RT_ERR_NODEV, "no HIP device available");
    if (device < 0 || device >= n) return fail(RT_ERR_ARG, "device index out of range");
    g_device = device;
    HIPCHK(hipSetDevice(device));
    return RT_OK;
}

void rt_render_opts_default(rt_render_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->spp = 1; o->use_bvh = 1; o->rebuild_bvh = 1; o->row0 = 0; o->row_step = 1; o->kernel_dim = 16; o->sync = 1;
}

int rt_render(rt_scene* s, const rt_render_opts* o, rt_stats* stats) {
    CHECK_FINISHED(s);
    if (!o) return fail(RT_ERR_ARG, "null options");
    if (o->spp < 1 || o->row_step < 1 || o->row0 < 0) return fail(RT_ERR_ARG, "spp >= 1, row_step >= 1, row0 >= 0 required");
    int r;
    if ((r = upload(s)) != RT_OK) return r;
    HIPCHK(hipSetDevice(s->device));
    if ((size_t)s->h.cam.W * s->h.cam.H > (size_t)INT32_MAX) return fail(RT_ERR_LIMIT, "frame larger than 2^31 pixels");
    if (s->multi && o->row0 == 0 && o->row_step == 1) return render_multi(s, o, stats);   // whole frames: split
    if ((r = ensure_spp(s, o->spp)) != RT_OK) return r;
    hipStream_t st = o->stream ? (hipStream_t)o->stream : sstream(s);
    const bool timed = stats != nullptr;
    hipEvent_t* te = nullptr;
    if (o->timing) {
        if (s->tev_used + 4 > s->tev.size()) {
            if (s->tev.size() >= 4 * 4096) return fail(RT_ERR_STATE, "too many timed frames pending: call rt_timing_collect");
            for (int i = 0; i < 4 * 64; i++) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); s->tev.push_back(e); }
        }
        te = &s->tev[s->tev_used];
        s->tev_used += 4;
    }
    if (s->n_slots > 1) {                                    // rotate frame slots (rt_scene_set_frame_slots)
        if ((r = ensure_other_slot(s)) != RT_OK) return r;
        s->cur_slot = (s->cur_slot + 1) % s->n_slots;
    }
    if ((r = begin_frame(s, st, false)) != RT_OK) return r;  // after the slot's previous frame, current poses
    if (timed) { HIPCHK(hipMemsetAsync(s->d_stats, 0, STATS_N * sizeof(unsigned long long), st)); HIPCHK(hipEventRecord(s->ev[0], st)); }
    if (s->builds_bvh(o->use_bvh, o->rebuild_bvh)) {
        if ((r = build_bvh(s, st, te ? te[0] : nullptr, te ? te[1] : nullptr)) != RT_OK) {
            if (te) s->tev_used -= 4;                            // the frame's events stay unrecorded
            return r;
        }
    } else if (te) {
        HIPCHK(hipEventRecord(te[0], st)); HIPCHK(hipEventRecord(te[1], st));
    }
    if (timed) HIPCHK(hipEventRecord(s->ev[1], st));
    rt_render_opts oo = *o;
    const size_t W = s->h.cam.W, H = s->h.cam.H;
    const size_t n_rows = (H > (size_t)o->row0) ? (H - o->row0 + o->row_step - 1) / o->row_step : 0;
    const size_t out_px = o->compact ? n_rows * W : W * H;
    if (o->host_outputs) {                                   // stage through device buffers
        if ((r = ensure_out_staging(s)) != RT_OK) return r;
        oo.rgba = o->rgba ? (uint32_t*)s->d_out[0] : nullptr;
        oo.radiance = o->radiance ? (float*)s->d_out[1] : nullptr;
        oo.hit_inst = o->hit_inst ? (int32_t*)s->d_out[2] : nullptr;
        oo.hit_tri = o->hit_tri ? (int32_t*)s->d_out[3] : nullptr;
    }
    TraceRequest q;
    q.stream = st; q.rgba = oo.rgba ? oo.rgba : s->d_canvas; q.want_stats = timed;
    if (te) { q.e0 = te[2]; q.e1 = te[3]; }
    if ((r = launch_trace(s, oo, q)) != RT_OK) {
        if (te) s->tev_used -= 4;
        return r;
    }
    if (timed) HIPCHK(hipEventRecord(s->ev[2], st));
    if ((r = end_frame(s, st)) != RT_OK) return r;           // the slot is free again once this frame is done
    if (o->sync || timed || o->host_outputs) HIPCHK(hipStreamSynchronize(st));
    if (o->host_outputs) {
        if (o->rgba) HIPCHK(hipMemcpy(o->rgba, oo.rgba, out_px * 4, hipMemcpyDeviceToHost));
        if (o->radiance) HIPCHK(hipMemcpy(o->radiance, oo.radiance, out_px * 16, hipMemcpyDeviceToHost));
        if (o->hit_inst) HIPCHK(hipMemcpy(o->hit_inst, oo.hit_inst, out_px * 4, hipMemcpyDeviceToHost));
        if (o->hit_tri) HIPCHK(hipMemcpy(o->hit_tri, oo.hit_tri, out_px * 4, hipMemcpyDeviceToHost));
    }
    return timed ? read_frame_stats(s, stats) : RT_OK;
}

int rt_scene_set_frame_slots(rt_scene* s, int n) {
    CHECK_FINISHED(s);
    if (n < 1 || n > rt_scene::MAX_SLOTS) return fail(RT_ERR_ARG, "frame slots: 1 to " + std::to_string(rt_scene::MAX_SLOTS));
    if (n == s->n_slots) return RT_OK;
    if (s->uploaded) { HIPCHK(hipSetDevice(s->device)); HIPCHK(hipDeviceSynchronize()); }   // nothing in flight
    s->cur_slot = 0;
    for (auto& f : s->slots) f.pending = false;
    s->n_slots = n;
    return (n > 1 && s->uploaded) ? ensure_other_slot(s) : RT_OK;
}

int rt_scene_set_overlap(rt_scene* s, int policy) {
    CHECK_SCENE(s);
    if (policy != RT_OVERLAP_HALF && policy != RT_OVERLAP_FULL && policy != RT_OVERLAP_STREAM)
        return fail(RT_ERR_ARG, "overlap policy: RT_OVERLAP_HALF, RT_OVERLAP_FULL or RT_OVERLAP_STREAM");
    s->overlap = policy;
    if (s->multi) set_multi_overlap(s, policy);               // the replicas of rt_scene_set_devices too
    return RT_OK;
}

int rt_timing_collect(rt_scene* s, double* bvh_ms, double* trace_ms, int* n) {
    CHECK_FINISHED(s);
    double a = 0, b = 0;
    for (size_t i = 0; i + 4 <= s->tev_used; i += 4) {
        HIPCHK(hipEventSynchronize(s->tev[i + 3]));
        float x = 0, y = 0;
        HIPCHK(hipEventElapsedTime(&x, s->tev[i], s->tev[i + 1]));
        HIPCHK(hipEventElapsedTime(&y, s->tev[i + 2], s->tev[i + 3]));
        a += x; b += y;
    }
    if (bvh_ms) *bvh_ms = a;
    if (trace_ms) *trace_ms = b;
    if (n) *n = (int)(s->tev_used / 4);
    s->tev_used = 0;
    return RT_OK;
}

int rt_update_scene(rt_scene* s, int kernel_dim, int optimize) {    // raytracer.cu:102-120
    CHECK_FINISHED(s);
    if (kernel_dim <= 0) return fail(RT_ERR_ARG, "kernel_dim must be positive");
    rt_render_opts o;
    rt_render_opts_default(&o);
    o.use_bvh = optimize ? 1 : 0; o.rebuild_bvh = 1; o.kernel_dim = kernel_dim;
    o.sync = s->multi ? 1 : 0;                                // split frames end on the slot's streams
    int r = rt_render(s, &o, nullptr);
    if (r != RT_OK) return r;
    // the canvas is host-readable on return (canvas.cu:23-29): one copy-engine transfer into the
    // pinned host canvas on the frame's stream, then wait for that stream only
    hipStream_t st = sstream(s);
    if (s->canvas.pinned)
        HIPCHK(hipMemcpyAsync(s->canvas.data(), s->d_canvas, s->canvas.size() * sizeof(uint32_t), hipMemcpyDeviceToDeviceNoCU, st));
    else
        HIPCHK(hipMemcpyAsync(s->canvas.data(), s->d_canvas, s->canvas.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return RT_OK;
}


int rt_canvas_read(const rt_scene* s, uint32_t* dst, int64_t n) {
    CHECK_FINISHED(s);
    if (!dst || n < (int64_t)s->canvas.size()) return fail(RT_ERR_ARG, "destination too small");
    memcpy(dst, s->canvas.data(), s->canvas.size() * sizeof(uint32_t));
    return RT_OK;
}
const uint32_t* rt_canvas_host_ptr(const rt_scene* s) { return s ? s->canvas.data() : nullptr; }
int rt_canvas_get_color(const rt_scene* s, int x, int y, uint8_t* c) {
    CHECK_FINISHED(s);
    if (!c || x < 0 || y < 0 || x >= s->h.cam.W || y >= s->h.cam.H) return fail(RT_ERR_ARG, "pixel out of range");
    uint32_t e = s->canvas[(size_t)y * s->h.cam.W + x];                  // Color::from_encoding (color.cu:28-34)
    c[0] = (uint8_t)(e >> 24); c[1] = (uint8_t)(e >> 16); c[2] = (uint8_t)(e >> 8); c[3] = (uint8_t)e;
    return RT_OK;
}

}  // extern "C"
