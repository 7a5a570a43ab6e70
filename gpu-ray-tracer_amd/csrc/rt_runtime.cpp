// rt_runtime.cpp — the host runtime of the ray-tracing core: the scene object (rt_internal.h),
// its upload, the frame slots, the per-frame BVH build and trace launch set-up, and the C ABI
// (rt_amd.h) except the multi-device entries (rt_multi.cpp) and the copy-engine entries
// (rt_copy.cpp).  Host code only: kernels are reached through the launch layer of rt_device.h
// (rt_kernels.hip).  The host float code here (ordered_tree_shape, tri_axis_records, view_of's
// pruning slack) decides kernel variants and bounds: it is built with the kernels' float rules.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "rt_accum.h"
#include "rt_internal.h"

using namespace rtm;
using namespace rtb;
using namespace rtd;
using namespace rti;
using rt::DCamera;
using rt::DInst;
using rt::DLight;
using rt::DMat;
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

// Leaf count and depth (internal nodes on the longest root-leaf path) of the ordered
// LBVH bvh_build_kernel will build: the same box, Morton and sort arithmetic on the
// host (RT_HD functions).  The fast traversal's stack holds <= FT_MAX_DEPTH entries (rt_plan.h).
// Mesh boxes: Trimesh::compute_bounding_box (trimesh.cu:21-32, sequential fit order) and
// the mesh pose.  They depend only on the immutable mesh data, so they are computed once
// here; the per-frame build (bvh_build_kernel) redoes everything per instance.
std::vector<Box> mesh_boxes(const rt::Scene& h) {
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
void free_atlas(rt_scene* s);
int ensure_atlas(rt_scene* s);

// The scene's own stream, created on first use: a caller passing its own streams (frame
// pipelining) keeps every HIP stream of the process on a hardware queue of its own
// (GPU_MAX_HW_QUEUES = 4; streams beyond that share queues and serialise).
hipStream_t sstream(rt_scene* s) {
    if (!s->stream) (void)hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    return s->stream;
}

}  // namespace

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
int end_frame(rt_scene* s, hipStream_t st) {
    HIPCHK(hipEventRecord(s->cur().done, st));
    s->cur().pending = true;
    return RT_OK;
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

// Capacities of the per-frame layout buffers for n_groups pixel groups.
struct Layout { int flags, sky_blocks, live_q, live; };
Layout layout_of(int n_groups) {
    Layout l;
    l.sky_blocks = (n_groups + 63) / 64;                       // sky_kernel's blocks, 64 groups each
    l.flags = (std::max(n_groups, 1024) + 3) & ~3;             // sky and history flags: whole dwords (scalar loads)
    l.live_q = (l.sky_blocks + NQ - 1) / NQ * 64;                  // most groups of the blocks b = q mod NQ
    l.live = l.live_q * NQ + n_groups;                         // + the heavy live list (hist = 2)
    return l;
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

// Device staging of host_outputs frames (rgba, radiance, hit_inst, hit_tri), whole-frame sized.
int ensure_out_staging(rt_scene* s) {
    const size_t px = (size_t)s->h.cam.W * s->h.cam.H;
    if (s->d_out_px >= px) return RT_OK;
    for (auto& p : s->d_out) dfree(p);
    s->d_out_px = 0;
    HIPCHK(hipMalloc(&s->d_out[0], px * 4)); HIPCHK(hipMalloc(&s->d_out[1], px * 16));
    HIPCHK(hipMalloc(&s->d_out[2], px * 4)); HIPCHK(hipMalloc(&s->d_out[3], px * 4));
    s->d_out_px = px;
    return RT_OK;
}

int build_bvh(rt_scene* s, hipStream_t st, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr) {
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

SceneView view_of(const rt_scene* s, bool use_bvh) {
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
    return v;
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

// What a trace launch is asked for beside the render options (each caller sets what it uses).
struct TraceRequest {
    hipStream_t stream = nullptr;
    uint32_t* rgba = nullptr;
    int* dbg = nullptr; int dbg_x = -1, dbg_y = -1;           // debug_cast's event log and its pixel
    bool want_stats = false;                                   // the counted kernel (d_stats)
    int occl_force = -1;                                       // shade_shortcuts
    hipEvent_t e0 = nullptr, e1 = nullptr;                     // timestamps taken by the dispatches themselves
    bool prof = false;                                         // the fast kernel's profiling variant (M_PROF)
    unsigned* gdur = nullptr;                                  // per-group durations (rt_profile_groups)
    int k0 = 0;                                                // sample base (rt_accumulate; TraceParams::k0)
    int* geo = nullptr;                                        // out: {n_groups, gw, gh, n_gx}
    // rt_accumulate's refinement passes (adaptive mode): trace only the groups of these live-group
    // lists ([NQ][lists_cap], sky_kernel's form), starting from lists_work, an image of the work
    // counters with the lists' lengths set.  No sky pre-pass, no scheduling history read or recorded.
    // Only a kernel that runs from live lists today takes them (TraceKey::sky); *listed (out) says so,
    // and a launch that does not traces every group as without them.  lists_n: the groups listed,
    // when known (> 0: the grid is sized by it).
    const int* lists = nullptr; int lists_cap = 0; const int* lists_work = nullptr; int lists_n = 0;
    bool* listed = nullptr;
};

// Fill TraceParams from the launch plan (rt_plan.h), ensure the slot's buffers, launch.
int launch_trace(rt_scene* s, const rt_render_opts& o, const TraceRequest& q) {
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
int begin_side_entry(rt_scene* s, int spp, bool bvh) {
    int r;
    if ((r = upload(s)) != RT_OK) return r;
    HIPCHK(hipSetDevice(s->device));
    if ((r = ensure_spp(s, spp)) != RT_OK) return r;
    if ((r = begin_frame(s, sstream(s), true)) != RT_OK) return r;   // nothing else in flight on this slot
    return bvh ? build_bvh(s, sstream(s)) : RT_OK;
}

// The quantisation box of rt_query's coherence keys (rt_raykey.h): the instances' world boxes
// (bvh_inst_box's arithmetic: the mesh box moved by the instance pose) merged, on the host,
// for the current poses; the same box with and without the BVH.  Degenerate and non-finite
// boxes are left out (no box at all: zeros, every origin in cell 0).
void refresh_query_box(rt_scene* s) {
    if (s->q_box_gen == s->inst_gen) return;
    const std::vector<Box> mbox = mesh_boxes(s->h);
    rtk::KeyBox kb{v3(INFINITY, INFINITY, INFINITY), v3(-INFINITY, -INFINITY, -INFINITY)};
    bool any = false;
    for (const DInst& in : s->h.d_insts) {
        const Box b = from_local(mbox[in.mesh], in.pose);
        if (!b.nd || !rtk::finite3(b.mn) || !rtk::finite3(b.mx)) continue;
        kb.mn = v3(std::min(kb.mn.x, b.mn.x), std::min(kb.mn.y, b.mn.y), std::min(kb.mn.z, b.mn.z));
        kb.mx = v3(std::max(kb.mx.x, b.mx.x), std::max(kb.mx.y, b.mx.y), std::max(kb.mx.z, b.mx.z));
        any = true;
    }
    s->q_box = any ? kb : rtk::KeyBox{v3(0, 0, 0), v3(0, 0, 0)};
    s->q_box_gen = s->inst_gen;
}

// The sorted mode's scratch for a batch of n rays (query_order_plan's layout at the capacity,
// then hipCUB's temporary storage, whose size is asked once per capacity).  A failed allocation
// leaves the scene without scratch, otherwise as it was.
int ensure_order_scratch(rt_scene* s, long long n) {
    if (n <= s->qo_rays) return RT_OK;
    const long long cap = std::min<long long>(std::max(n, 2 * s->qo_rays), INT32_MAX);
    const QueryOrderPlan P = query_order_plan(cap, QUERY_ORDER_SORTED, false);
    const size_t temp = (ray_sort_temp_bytes(cap, P.key_bits) + 255) & ~(size_t)255;
    dfree(s->qo_dev); s->qo_rays = 0; s->qo_temp = 0;
    s->last_query_order = nullptr;                             // (rt_query_last: the last order went with the buffer)
    if (hipMalloc((void**)&s->qo_dev, P.scratch_bytes + temp) != hipSuccess) {
        s->qo_dev = nullptr;
        return fail(RT_ERR_HIP, std::string("rt_query: no memory for the sort of ") + std::to_string(n) + " rays: " +
                                    hipGetErrorString(hipGetLastError()));
    }
    s->qo_rays = cap; s->qo_temp = temp;
    return RT_OK;
}

// Zero the counters; the two minima (slots 15 and 19: the waves' earliest start and earliest end,
// trace_kernel) start at all ones.
int clear_stats(rt_scene* s, hipStream_t st) {
    HIPCHK(hipMemsetAsync(s->d_stats, 0, STATS_N * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(s->d_stats + 15, 0xff, sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(s->d_stats + 19, 0xff, sizeof(unsigned long long), st));
    return RT_OK;
}

rt::Material mat_from(const float* m) {
    rt::Material r;
    r.Ke = v4(m[0], m[1], m[2], m[3]); r.Ka = v4(m[4], m[5], m[6], m[7]); r.Kd = v4(m[8], m[9], m[10], m[11]);
    r.Ks = v4(m[12], m[13], m[14], m[15]); r.Kt = v4(m[16], m[17], m[18], m[19]); r.Kr = v4(m[20], m[21], m[22], m[23]);
    r.alpha = m[24]; r.eta = m[25];
    return r;
}

// procedural::gpu::generate / SceneBuilder::build_gpu_scene put the scene on the device when it
// is made (cube_world.cc:195-207, scene_builder.cu:29-81); the first update_scene then only
// renders.  Here the upload is lazy (host-only scenes must load without a GPU), so a finished
// scene on a machine with a gfx950 device is uploaded at once and one untimed 1-spp frame is
// rendered into the device canvas: the code object, the scene's stream and the frame layout's
// buffers (sky flags, live lists, scheduling history) are then in place before the caller's
// first frame.  Without a usable device nothing happens (render calls report RT_ERR_NODEV as
// before); a failure here is left for the first render to report.  RT_NO_WARM=1 turns it off.
int warm_scene(rt_scene* s) {
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

}  // namespace

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
    dfree(q_dev); hfree(q_host); dfree(qo_dev);
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

// (ABI 3) hit_tri indexes the triangles in flattened mesh order, so the meshes must list every
// triangle exactly once: a bitmap of the triangles seen, failing on a repeat or on one left out
// (a count alone would pass a list that repeats one triangle and omits another).
static bool meshes_cover_tris_once(const rt::Scene& h) {
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
static int export_built_bvh(const rt_scene* s, int what, void* dst, int64_t cap) {
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
    if (o->use_bvh && (o->rebuild_bvh || !s->cur().bvh_valid)) {
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
    if (timed) {
        unsigned long long v[4];
        HIPCHK(hipMemcpy(v, s->d_stats, sizeof v, hipMemcpyDeviceToHost));
        stats->rays = v[0]; stats->nodes = v[1]; stats->leaves = v[2]; stats->tri_tests = v[3];
        float a = 0, b = 0;
        HIPCHK(hipEventElapsedTime(&a, s->ev[0], s->ev[1]));
        HIPCHK(hipEventElapsedTime(&b, s->ev[1], s->ev[2]));
        stats->bvh_ms = a; stats->trace_ms = b;
    }
    return RT_OK;
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

int rt_debug_cast(rt_scene* s, int x, int y, char* buf, int64_t cap) {   // raytracer.cu:91-100
    CHECK_FINISHED(s);
    if (x < 0 || y < 0 || x >= s->h.cam.W || y >= s->h.cam.H) return fail(RT_ERR_ARG, "pixel out of range");
    int r;
    // rebuilds the current slot's BVH: first wait for every frame in flight (any slot)
    if ((r = begin_side_entry(s, 1, true)) != RT_OK) return r;
    HIPCHK(hipMemsetAsync(s->d_dbg, 0, 4096 * sizeof(int), sstream(s)));
    rt_render_opts o;
    rt_render_opts_default(&o);
    o.row0 = y; o.row_step = s->h.cam.H;                                  // just the row of (x, y)
    TraceRequest q;
    q.stream = sstream(s); q.rgba = s->d_canvas; q.dbg = s->d_dbg; q.dbg_x = x; q.dbg_y = y; q.want_stats = true;
    if ((r = launch_trace(s, o, q)) != RT_OK) return r;
    if ((r = end_frame(s, sstream(s))) != RT_OK) return r;
    std::vector<int> log(4096);
    HIPCHK(hipStreamSynchronize(sstream(s)));
    HIPCHK(hipMemcpy(log.data(), s->d_dbg, log.size() * sizeof(int), hipMemcpyDeviceToHost));
    static const char* names[] = {"", "shooting a ray", "preparing to shoot a reflection ray",
                                  "preparing to shoot a refraction ray", "shooting shadow ray"};
    std::string out;
    int n = std::min(log[0], 4094);
    for (int i = 0; i < n; i++) { int e = log[2 + i]; if (e >= 1 && e <= 4) { out += names[e]; out += '\n'; } }
    if (buf && cap > 0) { size_t m = std::min<size_t>(out.size(), (size_t)cap - 1); memcpy(buf, out.data(), m); buf[m] = 0; }
    return RT_OK;
}

// Profiling aid (not part of rt_amd.h's stable surface): run experiment `which` `reps`
// times -- 4: the counted kernel with the occlusion early exit, 5: the counted kernel,
// 6: the fast kernel's PROF variant (wave step counts, cycle split, and the queries the
// fast kernel issues) -- and return the mean kernel ms and the counters.
int rt_experiment(rt_scene* s, int which, int spp, int reps, double* ms, uint64_t* counters) {
    CHECK_FINISHED(s);
    int r;
    if (which == 4 || which == 5 || which == 6) {             // full frame: counted kernel (4: occlusion exit on),
                                                              // 6: the fast kernel's profiling variant (M_PROF)
        if ((r = begin_side_entry(s, spp, true)) != RT_OK) return r;
        rt_render_opts o; rt_render_opts_default(&o); o.spp = spp;
        TraceRequest q;
        q.stream = sstream(s); q.rgba = s->d_canvas;
        if (which == 6) q.prof = true;
        else { q.want_stats = true; q.occl_force = which == 4 ? 1 : 0; }
        float total = 0;
        for (int i = 0; i < reps; i++) {
            if ((r = clear_stats(s, sstream(s))) != RT_OK) return r;
            HIPCHK(hipEventRecord(s->ev[0], sstream(s)));
            if ((r = launch_trace(s, o, q)) != RT_OK) return r;
            HIPCHK(hipEventRecord(s->ev[1], sstream(s)));
            HIPCHK(hipEventSynchronize(s->ev[1]));
            float t = 0; HIPCHK(hipEventElapsedTime(&t, s->ev[0], s->ev[1]));
            if (i > 0 || reps == 1) total += t;
        }
        if ((r = end_frame(s, sstream(s))) != RT_OK) return r;
        unsigned long long v[22];
        HIPCHK(hipMemcpy(v, s->d_stats, sizeof v, hipMemcpyDeviceToHost));
        if (counters) for (int i = 0; i < 22; i++) counters[i] = v[i];
        if (ms) *ms = total / (reps > 1 ? reps - 1 : 1);
        return RT_OK;
    }
    return fail(RT_ERR_ARG, "experiment: 4 (counted, occlusion exit), 5 (counted), 6 (fast kernel, PROF counters)");
}

int rt_frame_work(rt_scene* s, const rt_render_opts* o, rt_work* w) {
    CHECK_FINISHED(s);
    if (!o || !w) return fail(RT_ERR_ARG, "null argument");
    if (o->spp < 1 || o->spp > 64 || o->row_step < 1 || o->row0 < 0 || !o->use_bvh || o->textures)
        return fail(RT_ERR_ARG, "rt_frame_work: BVH frames, 1 <= spp <= 64, untextured");
    int r;
    if ((r = begin_side_entry(s, o->spp, true)) != RT_OK) return r;
    const size_t rows = (s->h.cam.H > o->row0) ? (size_t)(s->h.cam.H - o->row0 + o->row_step - 1) / o->row_step : 0;
    // the frame: the caller's device buffer, or a private one (dropped, or copied to the caller's host buffer)
    const size_t out_px = (o->compact ? rows : (size_t)s->h.cam.H) * s->h.cam.W;
    const bool to_caller = o->rgba && !o->host_outputs;
    DevBuf<uint32_t> d_rgba;
    if (!to_caller) HIPCHK(d_rgba.alloc(std::max<size_t>(1, out_px)));
    hipStream_t st = sstream(s);
    if ((r = clear_stats(s, st)) != RT_OK) return r;
    rt_render_opts oo = *o;
    oo.radiance = nullptr; oo.hit_inst = oo.hit_tri = nullptr;
    TraceRequest q;
    q.stream = st; q.rgba = to_caller ? o->rgba : d_rgba.p; q.prof = true;
    if ((r = launch_trace(s, oo, q)) != RT_OK) return r;
    if ((r = end_frame(s, st)) != RT_OK) return r;
    unsigned long long v[STATS_N] = {};
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(v, s->d_stats, sizeof v, hipMemcpyDeviceToHost));
    if (v[4] == 0 && rows > 0) return fail(RT_ERR_STATE, "no profiling variant of the fast kernel for this scene");
    if (o->rgba && o->host_outputs && out_px) HIPCHK(hipMemcpy(o->rgba, d_rgba.p, out_px * 4, hipMemcpyDeviceToHost));
    w->queries = v[0]; w->wave_queries = v[4]; w->pair_steps = v[5]; w->leaf_visits = v[6]; w->tri_iters = v[7];
    w->leaf_lanes = v[2];
    w->scene_bytes = scene_image_bytes(view_of(s, true));
    w->lanes_primary = v[PROF_LANES_PRIMARY]; w->lanes_secondary = v[PROF_LANES_SECONDARY];
    w->lanes_shadow = v[PROF_LANES_SHADOW]; w->lanes_unlit = v[PROF_LANES_UNLIT];
    w->live_wave_queries = v[PROF_LIVE_WQ]; w->live_lanes = v[PROF_LIVE_LANES];
    for (int i = 0; i < 8; i++) {
        w->hist_wave_queries[i] = v[PROF_HIST_WQ + i];
        w->hist_pair_steps[i] = v[PROF_HIST_PAIR + i];
        w->hist_leaf_visits[i] = v[PROF_HIST_LEAF + i];
    }
    return RT_OK;
}

void rt_accum_opts_default(rt_accum_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->samples = 1; o->use_bvh = 1; o->rebuild_bvh = 1;
}

namespace {
constexpr int ACCUM_MAX_SAMPLES = 65536;

// Has anything that decides a sample changed since the accumulation's first one?
bool accum_stale(const rt_scene* s, int textures) {
    const rt_scene::Accum& a = s->accum;
    return a.n > 0 && (a.inst_gen != s->inst_gen || a.cam_gen != s->cam_gen || a.env_gen != s->env_gen ||
                       a.atlas_gen != s->atlas_gen || a.textures != textures);
}
void accum_drop(rt_scene* s) {
    if (s->accum.n > 0) s->accum.restarts++;
    s->accum.n = 0;
    s->accum.have_mask = false; s->accum.needed = -1; s->accum.count_pending = false;   // the mask goes with the sums
}
// The tiles of the scene's canvas: the pixel groups of a whole-frame 1-spp launch.
rtad::TileGrid accum_tiles(const rt_scene* s) {
    const FrameGeometry g = frame_geometry(s->h.cam.W, s->h.cam.H, 0, 1, 1);
    return rtad::tile_grid(s->h.cam.W, s->h.cam.H, g.gw, g.gh);
}
// Adaptive mode's buffers for the canvas's tiles; a failed allocation leaves none of them.
int ensure_adaptive(rt_scene* s) {
    rt_scene::Accum& a = s->accum;
    const int n = std::max(1, rtad::n_tiles(accum_tiles(s)));
    if (a.tile_cap >= n) return RT_OK;
    a.release_adaptive();
    if (hipMalloc((void**)&a.d_need, ((size_t)n + 3) & ~(size_t)3) != hipSuccess ||
        hipMalloc((void**)&a.d_live, (size_t)NQ * layout_of(n).live_q * sizeof(int)) != hipSuccess ||
        hipMalloc((void**)&a.d_image, WORK_INTS * sizeof(int)) != hipSuccess) {
        const std::string why = hipGetErrorString(hipGetLastError());
        a.release_adaptive();
        return fail(RT_ERR_HIP, "rt_accumulate: no memory for the mask and lists of " + std::to_string(n) + " tiles: " + why);
    }
    a.tile_cap = n;
    return RT_OK;
}
// The scene-owned buffers for the canvas; a failed allocation leaves none of them (and no samples).
int ensure_accum(rt_scene* s) {
    rt_scene::Accum& a = s->accum;
    const size_t px = std::max<size_t>(1, (size_t)s->h.cam.W * s->h.cam.H);
    if (a.px >= px) return RT_OK;
    a.release(); a.n = 0;
    if (hipMalloc((void**)&a.d_sum_r, px * sizeof(float4)) != hipSuccess || hipMalloc((void**)&a.d_sum_c, px * sizeof(float4)) != hipSuccess ||
        hipMalloc((void**)&a.d_pass, px * sizeof(float4)) != hipSuccess || hipMalloc((void**)&a.d_hit_inst, px * sizeof(int32_t)) != hipSuccess ||
        hipMalloc((void**)&a.d_hit_tri, px * sizeof(int32_t)) != hipSuccess) {
        const std::string why = hipGetErrorString(hipGetLastError());
        a.release();
        return fail(RT_ERR_HIP, "rt_accumulate: no memory for the sums of " + std::to_string(px) + " pixels: " + why);
    }
    a.px = px;
    return RT_OK;
}
}  // namespace

// Progressive refinement (rt_amd.h): a side entry like rt_frame_work.  Sample k of the
// accumulation is a 1-spp trace launch with sample base k into the pass buffer, then one fold
// (accum_fold_kernel); the call's last fold resolves the frame.
int rt_accumulate(rt_scene* s, const rt_accum_opts* o, int* n_samples) {
    CHECK_FINISHED(s);
    if (!o) return fail(RT_ERR_ARG, "null options");
    if (o->samples < 1) return fail(RT_ERR_ARG, "rt_accumulate: samples >= 1 required");
    if (!(o->rgba || o->radiance || o->hit_inst || o->hit_tri)) return fail(RT_ERR_ARG, "rt_accumulate: no output requested");
    const int textures = o->textures ? 1 : 0;
    const bool fresh = o->restart || accum_stale(s, textures);
    if ((long long)(fresh ? 0 : s->accum.n) + o->samples > ACCUM_MAX_SAMPLES)
        return fail(RT_ERR_LIMIT, "rt_accumulate: more than 65536 samples held (rt_accumulate_reset starts again)");
    if (s->multi) return fail(RT_ERR_STATE, "rt_accumulate: not on a scene split by rt_scene_set_devices");
    int r;
    if ((r = upload(s)) != RT_OK) return r;
    HIPCHK(hipSetDevice(s->device));
    const size_t px = (size_t)s->h.cam.W * s->h.cam.H;
    if (px > (size_t)INT32_MAX) return fail(RT_ERR_LIMIT, "frame larger than 2^31 pixels");
    if (textures && s->h.atlas_rgba.empty())
        return fail(RT_ERR_STATE, "textured rendering needs an atlas: rt_scene_load_atlas / rt_scene_set_atlas");
    if (fresh) accum_drop(s);
    if ((r = ensure_accum(s)) != RT_OK) return r;
    if (o->host_outputs && (r = ensure_out_staging(s)) != RT_OK) return r;
    rt_scene::Accum& a = s->accum;
    // frames in flight (any slot) first; the BVH at most once, for every sample of the call
    if ((r = begin_side_entry(s, 1, o->use_bvh && (o->rebuild_bvh || !s->cur().bvh_valid))) != RT_OK) return r;
    hipStream_t st = sstream(s);
    uint32_t* d_rgba = !o->rgba ? nullptr : o->host_outputs ? (uint32_t*)s->d_out[0] : o->rgba;
    float4* d_rad = !o->radiance ? nullptr : o->host_outputs ? (float4*)s->d_out[1] : reinterpret_cast<float4*>(o->radiance);
    rt_render_opts ro;
    rt_render_opts_default(&ro);
    ro.use_bvh = o->use_bvh; ro.textures = textures;
    ro.radiance = reinterpret_cast<float*>(a.d_pass);
    // Adaptive mode (rt_adapt.h): sample 0 everywhere, then the mask and the needed tiles' lists,
    // once; every later sample is traced and folded for the needed tiles only.
    const bool adaptive = a.mode == 1;
    for (int i = 0; i < o->samples; i++) {
        if (a.n == 0) {                                       // what this accumulation's samples see
            a.inst_gen = s->inst_gen; a.cam_gen = s->cam_gen; a.env_gen = s->env_gen; a.atlas_gen = s->atlas_gen;
            a.textures = textures;
        }
        const bool last = i == o->samples - 1;
        const int before = a.n;
        const bool refine = adaptive && before > 0;           // (a mask exists: sample 0 of this mode made it)
        if (refine && a.needed == 0) {                        // no tile has an edge: nothing to trace or fold
            a.traced = 0;
            if (last) HIPCHK(launch_accum_fold_tiles(a.d_pass, a.d_sum_r, a.d_sum_c, a.d_need, a.tiles, before, true, d_rgba, d_rad, st, nullptr, nullptr));
            a.n = before + 1;
            continue;
        }
        ro.hit_inst = a.n == 0 ? a.d_hit_inst : nullptr;      // sample 0's primary hit, kept
        ro.hit_tri = a.n == 0 ? a.d_hit_tri : nullptr;
        TraceRequest q;
        q.stream = st; q.k0 = a.n;                            // (no RGBA8 of the pass: the fold resolves)
        int geo[4] = {0, 0, 0, 0};
        bool listed = false;
        q.geo = geo; q.listed = &listed;
        if (refine) {
            q.lists = a.d_live; q.lists_cap = layout_of(rtad::n_tiles(a.tiles)).live_q; q.lists_work = a.d_image;
            q.lists_n = a.needed;
        }
        a.n = 0;                                              // a failed launch leaves no samples, not stale sums
        if ((r = launch_trace(s, ro, q)) != RT_OK) return r;
        if (!refine) {
            HIPCHK(launch_accum_fold(a.d_pass, a.d_sum_r, a.d_sum_c, (int)px, before, last, d_rgba, d_rad, st, nullptr, nullptr));
            if (adaptive && before == 0) {
                if ((r = ensure_adaptive(s)) != RT_OK) return r;
                a.tiles = rtad::tile_grid(s->h.cam.W, s->h.cam.H, geo[1], geo[2]);   // the launch's own geometry
                const int nt = rtad::n_tiles(a.tiles);
                if (nt != geo[0] || a.tiles.n_tx != geo[3] || nt > a.tile_cap || geo[1] * geo[2] > 64)
                    return fail(RT_ERR_STATE, "rt_accumulate: the 1-spp launch's groups are not the canvas's tiles");
                HIPCHK(launch_accum_edge(a.d_sum_c, a.tiles, a.threshold, a.d_need, st, nullptr, nullptr));
                HIPCHK(hipMemsetAsync(a.d_image, 0, WORK_INTS * sizeof(int), st));
                HIPCHK(launch_accum_lists(a.d_need, nt, a.d_live, layout_of(nt).live_q, a.d_image, st, nullptr, nullptr));
                a.have_mask = true; a.needed = -1;
                a.count_pending = true;                       // read at the next sync that ends a call
            }
            a.traced = adaptive ? geo[0] : 0;
        } else {
            HIPCHK(launch_accum_fold_tiles(a.d_pass, a.d_sum_r, a.d_sum_c, a.d_need, a.tiles, before, last, d_rgba, d_rad, st, nullptr, nullptr));
            a.traced = listed ? -1 : geo[0];                  // -1: the needed tiles (their count may still be pending)
        }
        a.n = before + 1;
    }
    const bool host = o->host_outputs != 0;
    const hipMemcpyKind kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (!host) {                                              // the kept hit ids into the caller's device arrays
        if (o->hit_inst) HIPCHK(hipMemcpyAsync(o->hit_inst, a.d_hit_inst, px * 4, kind, st));
        if (o->hit_tri) HIPCHK(hipMemcpyAsync(o->hit_tri, a.d_hit_tri, px * 4, kind, st));
    }
    if ((r = end_frame(s, st)) != RT_OK) return r;
    HIPCHK(hipStreamSynchronize(st));
    if (a.count_pending) {                                    // the lists' lengths, one copy; their sum is the count
        int len[16 * NQ];
        HIPCHK(hipMemcpy(len, a.d_image + 16 * (NQ + 1), sizeof len, hipMemcpyDeviceToHost));
        a.needed = 0;
        for (int q = 0; q < NQ; q++) a.needed += len[16 * q];
        a.count_pending = false;
    }
    if (a.traced == -1) a.traced = a.needed;
    if (host) {
        if (o->rgba) HIPCHK(hipMemcpy(o->rgba, d_rgba, px * 4, kind));
        if (o->radiance) HIPCHK(hipMemcpy(o->radiance, d_rad, px * 16, kind));
        if (o->hit_inst) HIPCHK(hipMemcpy(o->hit_inst, a.d_hit_inst, px * 4, kind));
        if (o->hit_tri) HIPCHK(hipMemcpy(o->hit_tri, a.d_hit_tri, px * 4, kind));
    }
    if (n_samples) *n_samples = a.n;
    return RT_OK;
}

int rt_accumulate_reset(rt_scene* s) {
    CHECK_SCENE(s);
    accum_drop(s);
    return RT_OK;
}

int rt_accumulate_info(const rt_scene* s, int32_t* out4) {
    CHECK_SCENE(s);
    if (!out4) return fail(RT_ERR_ARG, "null argument");
    out4[0] = s->accum.n; out4[1] = s->h.cam.W; out4[2] = s->h.cam.H; out4[3] = s->accum.restarts;
    return RT_OK;
}

int rt_accumulate_set_adaptive(rt_scene* s, int mode, float threshold) {
    CHECK_SCENE(s);
    if (mode != 0 && mode != 1) return fail(RT_ERR_ARG, "rt_accumulate_set_adaptive: mode 0 (uniform) or 1 (adaptive)");
    if (mode == 1 && !(threshold >= 0.0f && std::isfinite(threshold)))
        return fail(RT_ERR_ARG, "rt_accumulate_set_adaptive: threshold must be finite and >= 0");
    rt_scene::Accum& a = s->accum;
    if (mode == a.mode && (mode == 0 || threshold == a.threshold)) return RT_OK;   // nothing changes
    accum_drop(s);
    a.mode = mode;
    if (mode == 1) a.threshold = threshold;
    return RT_OK;
}

int rt_accumulate_adaptive_info(const rt_scene* s, int32_t* out8, float* threshold, uint8_t* need, int64_t need_cap) {
    CHECK_FINISHED(s);
    if (!out8) return fail(RT_ERR_ARG, "null argument");
    const rt_scene::Accum& a = s->accum;
    const rtad::TileGrid t = a.have_mask ? a.tiles : accum_tiles(s);
    const int nt = rtad::n_tiles(t);
    if (need && need_cap < nt) return fail(RT_ERR_ARG, "rt_accumulate_adaptive_info: need_cap below the number of tiles");
    if (need && !(a.have_mask && a.n > 0)) return fail(RT_ERR_STATE, "rt_accumulate_adaptive_info: no mask yet (adaptive mode, after rt_accumulate)");
    out8[0] = a.mode; out8[1] = t.gw; out8[2] = t.gh; out8[3] = t.n_tx; out8[4] = t.n_ty;
    out8[5] = (a.have_mask && a.n > 0) ? a.needed : -1;
    out8[6] = a.n > 0 ? (a.traced == -1 ? a.needed : a.traced) : 0; out8[7] = 0;   // (-1: the needed tiles, a call that failed before its sync)
    if (threshold) *threshold = a.threshold;
    if (need) {
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(hipMemcpy(need, a.d_need, (size_t)nt, hipMemcpyDeviceToHost));
    }
    return RT_OK;
}

// Test hook: the current frame slot's scheduling-history state as the host holds it.
int rt_scene_history_info(const rt_scene* s, int32_t* out12) {
    CHECK_FINISHED(s);
    if (!out12) return fail(RT_ERR_ARG, "null argument");
    const FrameSlot& f = s->cur();
    out12[0] = f.hist_parity; out12[1] = f.hctl_zeroed; out12[2] = f.hist_cap; out12[3] = s->cur_slot;
    for (int i = 0; i < 8; i++) out12[4 + i] = (int32_t)f.hist_key[i];
    return RT_OK;
}

// Test hooks: the scene's pass buffer (the 1-sample frame a pass is traced into) filled with a
// 32-bit pattern / copied out, after every frame in flight.
int rt_accumulate_pass_fill(rt_scene* s, uint32_t bits) {
    CHECK_FINISHED(s);
    if (!s->accum.d_pass) return fail(RT_ERR_STATE, "rt_accumulate_pass_fill: no pass buffer before the first rt_accumulate");
    int r;
    if ((r = begin_side_entry(s, 1, false)) != RT_OK) return r;
    const size_t px = (size_t)s->h.cam.W * s->h.cam.H;
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)s->accum.d_pass, (int)bits, px * 4, sstream(s)));
    HIPCHK(hipStreamSynchronize(sstream(s)));
    return RT_OK;
}

int rt_accumulate_pass_read(rt_scene* s, float* dst, int64_t cap_floats) {
    CHECK_FINISHED(s);
    if (!dst) return fail(RT_ERR_ARG, "null argument");
    if (!s->accum.d_pass) return fail(RT_ERR_STATE, "rt_accumulate_pass_read: no pass buffer before the first rt_accumulate");
    const size_t px = (size_t)s->h.cam.W * s->h.cam.H;
    if (cap_floats < (int64_t)(px * 4)) return fail(RT_ERR_ARG, "rt_accumulate_pass_read: buffer below W * H float4");
    int r;
    if ((r = begin_side_entry(s, 1, false)) != RT_OK) return r;
    HIPCHK(hipStreamSynchronize(sstream(s)));
    HIPCHK(hipMemcpy(dst, s->accum.d_pass, px * 16, hipMemcpyDeviceToHost));
    return RT_OK;
}

// Profiling aid (tools/accum_bench.py, not part of rt_amd.h's stable surface): the fold kernel
// alone over buffers of the scene's canvas size, `reps` launches timed by the dispatches' own
// events; *ms = the mean of all but the first.  The scene's accumulation is not touched.
int rt_accum_fold_time(rt_scene* s, int reps, int resolve, double* ms) {
    CHECK_FINISHED(s);
    if (reps < 1 || !ms) return fail(RT_ERR_ARG, "bad arguments");
    int r;
    if ((r = begin_side_entry(s, 1, false)) != RT_OK) return r;
    const size_t px = (size_t)s->h.cam.W * s->h.cam.H;
    if (px == 0 || px > (size_t)INT32_MAX) return fail(RT_ERR_LIMIT, "frame of no pixels, or of more than 2^31");
    DevBuf<float4> pass, sr, sc, rad;
    DevBuf<uint32_t> rgba;
    HIPCHK(pass.alloc(px)); HIPCHK(sr.alloc(px)); HIPCHK(sc.alloc(px)); HIPCHK(rad.alloc(px)); HIPCHK(rgba.alloc(px));
    hipStream_t st = sstream(s);
    HIPCHK(hipMemsetAsync(pass.p, 0, px * sizeof(float4), st));
    float total = 0;
    for (int i = 0; i < reps; i++) {
        HIPCHK(launch_accum_fold(pass.p, sr.p, sc.p, (int)px, i, resolve != 0, rgba.p, rad.p, st, s->ev[0], s->ev[1]));
        HIPCHK(hipEventSynchronize(s->ev[1]));
        float t = 0; HIPCHK(hipEventElapsedTime(&t, s->ev[0], s->ev[1]));
        if (i > 0 || reps == 1) total += t;
    }
    *ms = total / (reps > 1 ? reps - 1 : 1);
    return RT_OK;
}

// The same for adaptive mode's kernels, over the mask the scene's accumulation holds (RT_ERR_STATE
// without one): ms4 = {accum_edge_kernel, accum_lists_kernel, accum_fold_tiles_kernel folding only,
// the same resolving}.  The edge kernel reads the scene's sums and writes a scratch mask; lists,
// sums and pass are scratch too: the accumulation is not touched.
int rt_accum_adaptive_time(rt_scene* s, int reps, double* ms4) {
    CHECK_FINISHED(s);
    if (reps < 1 || !ms4) return fail(RT_ERR_ARG, "bad arguments");
    rt_scene::Accum& a = s->accum;
    if (!(a.have_mask && a.n > 0)) return fail(RT_ERR_STATE, "no mask (adaptive mode, after rt_accumulate)");
    int r;
    if ((r = begin_side_entry(s, 1, false)) != RT_OK) return r;
    const size_t px = (size_t)s->h.cam.W * s->h.cam.H;
    const int nt = rtad::n_tiles(a.tiles), live_q = layout_of(nt).live_q;
    DevBuf<float4> pass, sr, sc, rad;
    DevBuf<uint32_t> rgba;
    DevBuf<unsigned char> need;
    DevBuf<int> live, image;
    HIPCHK(pass.alloc(px)); HIPCHK(sr.alloc(px)); HIPCHK(sc.alloc(px)); HIPCHK(rad.alloc(px)); HIPCHK(rgba.alloc(px));
    HIPCHK(need.alloc(((size_t)nt + 3) & ~(size_t)3)); HIPCHK(live.alloc((size_t)NQ * live_q)); HIPCHK(image.alloc(WORK_INTS));
    hipStream_t st = sstream(s);
    HIPCHK(hipMemsetAsync(pass.p, 0, px * sizeof(float4), st));
    HIPCHK(hipMemsetAsync(sr.p, 0, px * sizeof(float4), st));
    HIPCHK(hipMemsetAsync(sc.p, 0, px * sizeof(float4), st));
    for (int k = 0; k < 4; k++) {
        float total = 0;
        for (int i = 0; i < reps; i++) {
            if (k == 0) HIPCHK(launch_accum_edge(a.d_sum_c, a.tiles, a.threshold, need.p, st, s->ev[0], s->ev[1]));
            if (k == 1) {
                HIPCHK(hipMemsetAsync(image.p, 0, WORK_INTS * sizeof(int), st));
                HIPCHK(launch_accum_lists(a.d_need, nt, live.p, live_q, image.p, st, s->ev[0], s->ev[1]));
            }
            if (k >= 2) HIPCHK(launch_accum_fold_tiles(pass.p, sr.p, sc.p, a.d_need, a.tiles, 1 + i, k == 3, rgba.p, rad.p, st, s->ev[0], s->ev[1]));
            HIPCHK(hipEventSynchronize(s->ev[1]));
            float t = 0; HIPCHK(hipEventElapsedTime(&t, s->ev[0], s->ev[1]));
            if (i > 0 || reps == 1) total += t;
        }
        ms4[k] = total / (reps > 1 ? reps - 1 : 1);
    }
    return RT_OK;
}

// Where a pass's time goes (tools/accum_bench.py; tool-only, not in rt_amd.h): `reps` refinement
// passes over the tile lists and as many uniform passes, each traced into the pass buffer and
// folded into scratch sums (the accumulation's sums, mask and lists are not touched; its mask is
// needed: RT_ERR_STATE without one.  The pass buffer is overwritten, and the uniform passes are
// ordinary launches: they record scheduling history and advance the slot's parity, as any
// rt_render does; only the listed passes leave the history alone).  Per pass four spans from events on the scene's stream: ms8 = {listed:
// pre-trace gap (a marker before launch_trace to the trace dispatch's own start: the counter image's
// copy), the trace kernel, the tiles fold, marker to fold end; uniform: the same with the gap to
// the sky pre-pass's start, sky + trace, accum_fold_kernel}.  Means of all but the first pass.
int rt_accum_pass_timeline(rt_scene* s, int reps, double* ms8) {
    CHECK_FINISHED(s);
    if (reps < 1 || !ms8) return fail(RT_ERR_ARG, "bad arguments");
    rt_scene::Accum& a = s->accum;
    if (!(a.have_mask && a.n > 0 && a.needed > 0)) return fail(RT_ERR_STATE, "no mask with a needed tile (adaptive mode, after rt_accumulate)");
    int r;
    if ((r = begin_side_entry(s, 1, true)) != RT_OK) return r;
    const size_t px = (size_t)s->h.cam.W * s->h.cam.H;
    DevBuf<float4> sr, sc;
    HIPCHK(sr.alloc(px)); HIPCHK(sc.alloc(px));
    hipStream_t st = sstream(s);
    HIPCHK(hipMemsetAsync(sr.p, 0, px * sizeof(float4), st));
    HIPCHK(hipMemsetAsync(sc.p, 0, px * sizeof(float4), st));
    struct Events {
        hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        ~Events() { for (auto& x : e) if (x) (void)hipEventDestroy(x); }
    } ev;
    for (auto& x : ev.e) HIPCHK(hipEventCreate(&x));
    rt_render_opts ro;
    rt_render_opts_default(&ro);
    ro.textures = a.textures;
    ro.radiance = reinterpret_cast<float*>(a.d_pass);
    for (int k = 0; k < 8; k++) ms8[k] = 0;
    for (int kind = 0; kind < 2; kind++)
        for (int i = 0; i < reps; i++) {
            TraceRequest q;
            bool listed = false;
            q.stream = st; q.k0 = 1; q.e0 = ev.e[1]; q.e1 = ev.e[2]; q.listed = &listed;
            if (kind == 0) {
                q.lists = a.d_live; q.lists_cap = layout_of(rtad::n_tiles(a.tiles)).live_q; q.lists_work = a.d_image;
                q.lists_n = a.needed;
            }
            HIPCHK(hipEventRecord(ev.e[0], st));
            if ((r = launch_trace(s, ro, q)) != RT_OK) return r;
            if (kind == 0 && !listed) return fail(RT_ERR_STATE, "this scene's kernel takes no tile lists");
            if (kind == 0) HIPCHK(launch_accum_fold_tiles(a.d_pass, sr.p, sc.p, a.d_need, a.tiles, 1 + i, false, nullptr, nullptr, st, ev.e[3], ev.e[4]));
            else HIPCHK(launch_accum_fold(a.d_pass, sr.p, sc.p, (int)px, 1 + i, false, nullptr, nullptr, st, ev.e[3], ev.e[4]));
            HIPCHK(hipEventSynchronize(ev.e[4]));
            if (i == 0 && reps > 1) continue;
            const int pairs[4][2] = {{0, 1}, {1, 2}, {3, 4}, {0, 4}};
            for (int k = 0; k < 4; k++) {
                float t = 0;
                HIPCHK(hipEventElapsedTime(&t, ev.e[pairs[k][0]], ev.e[pairs[k][1]]));
                ms8[4 * kind + k] += t / (reps > 1 ? reps - 1 : 1);
            }
        }
    return RT_OK;
}

void rt_occlusion_opts_default(rt_occlusion_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->samples = 1; o->radius = INFINITY; o->bias = RT_AO_BIAS_DEFAULT; o->use_bvh = 1; o->rebuild_bvh = 1;
}

namespace {
static_assert(RT_AO_MAX_SAMPLES == rto::AO_MAX_SAMPLES, "the direction table's length");

// Has anything that decides an occlusion sample changed since the accumulation's first one?
bool occl_stale(const rt_scene* s, float radius, float bias) {
    const rt_scene::Occl& a = s->occl;
    return a.n > 0 && (a.inst_gen != s->inst_gen || a.cam_gen != s->cam_gen || a.radius != radius || a.bias != bias);
}
void occl_drop(rt_scene* s) {
    if (s->occl.n > 0) s->occl.restarts++;
    s->occl.n = 0;
}
// The scene-owned buffers for the canvas and the direction table; a failed allocation leaves none
// of them (and no samples).
int ensure_occl(rt_scene* s) {
    rt_scene::Occl& a = s->occl;
    const size_t px = std::max<size_t>(1, (size_t)s->h.cam.W * s->h.cam.H);
    if (a.px >= px) return RT_OK;
    a.release();
    if (hipMalloc((void**)&a.d_table, rto::AO_MAX_SAMPLES * sizeof(rtm::V3)) != hipSuccess ||
        hipMalloc((void**)&a.d_surf, 2 * px * sizeof(float4)) != hipSuccess ||
        hipMalloc((void**)&a.d_count, px * sizeof(int32_t)) != hipSuccess) {
        const std::string why = hipGetErrorString(hipGetLastError());
        a.release();
        return fail(RT_ERR_HIP, "rt_occlusion: no memory for the surface record and counts of " + std::to_string(px) + " pixels: " + why);
    }
    std::vector<rtm::V3> tab(rto::AO_MAX_SAMPLES);
    for (int k = 0; k < rto::AO_MAX_SAMPLES; k++) rto::ao_direction(k, &tab[k].x);
    if (hipMemcpy(a.d_table, tab.data(), tab.size() * sizeof(rtm::V3), hipMemcpyHostToDevice) != hipSuccess) {
        const std::string why = hipGetErrorString(hipGetLastError());
        a.release();
        return fail(RT_ERR_HIP, "rt_occlusion: the direction table's copy: " + why);
    }
    a.px = px;
    return RT_OK;
}
// The kernels' arguments and scene view for the current slot: rt_query's view (camera-ray
// shortcuts off, the zero-axis cut's scene term, the early-exit margin).
void occl_launch_setup(rt_scene* s, bool use_bvh, OcclParams& P, SceneView& S, OcclPlan& plan) {
    const rt_scene::Occl& a = s->occl;
    S = view_of(s, use_bvh);
    S.prune_abs = -1.0f; S.tri_ax = nullptr;
    P = OcclParams{};
    P.cam = s->h.d_cam; P.W = s->h.cam.W; P.H = s->h.cam.H;
    P.radius = a.radius; P.bias = a.bias;
    P.zcut_scene = prune_slack(s, 0.0f);
    const float margin = (float)S.n_inst * 0x1p-19f;           // (rt_query's)
    P.any_margin = margin <= 0.125f ? margin : -1.0f;
    P.table = a.d_table; P.surf = a.d_surf; P.count = a.d_count;
    int map = -1;                                              // RT_OCCL_MAP (measurements): row / tile
    if (const char* e = getenv("RT_OCCL_MAP")) map = !strcmp(e, "row") ? OCCL_MAP_ROW : !strcmp(e, "tile") ? OCCL_MAP_TILE : -1;
    plan = occlusion_plan(P.W, P.H, S, map);
    P.map = plan.map; P.n_waves = plan.n_waves;
}
}  // namespace

// Ambient occlusion (rt_amd.h): a side entry like rt_query.  Its kernels are the occlusion kernels,
// not a trace kernel: the scene's last trace launch and the slots' scheduling history stay as they were.
int rt_occlusion(rt_scene* s, const rt_occlusion_opts* o, int* n_samples) {
    CHECK_FINISHED(s);
    if (!o) return fail(RT_ERR_ARG, "null options");
    if (o->samples < 1) return fail(RT_ERR_ARG, "rt_occlusion: samples >= 1 required");
    if (!(o->radius > 0.0f)) return fail(RT_ERR_ARG, "rt_occlusion: radius > 0 required (+inf: sky visibility)");
    if (!(o->bias >= 0.0f && std::isfinite(o->bias))) return fail(RT_ERR_ARG, "rt_occlusion: bias must be finite and >= 0");
    if (!(o->visibility || o->occluded || o->rgba)) return fail(RT_ERR_ARG, "rt_occlusion: no output requested");
    const bool fresh = o->restart || occl_stale(s, o->radius, o->bias);
    if ((long long)(fresh ? 0 : s->occl.n) + o->samples > RT_AO_MAX_SAMPLES)
        return fail(RT_ERR_LIMIT, "rt_occlusion: more than 1024 samples held (rt_occlusion_reset starts again)");
    if (s->multi) return fail(RT_ERR_STATE, "rt_occlusion: not on a scene split by rt_scene_set_devices");
    int r;
    if ((r = upload(s)) != RT_OK) return r;
    HIPCHK(hipSetDevice(s->device));
    const size_t px = (size_t)s->h.cam.W * s->h.cam.H;
    if (px > (size_t)INT32_MAX / 8) return fail(RT_ERR_LIMIT, "rt_occlusion: frame larger than 2^28 pixels");
    if (fresh) occl_drop(s);
    if ((r = ensure_occl(s)) != RT_OK) return r;
    if (o->host_outputs && (r = ensure_out_staging(s)) != RT_OK) return r;
    rt_scene::Occl& a = s->occl;
    // frames in flight (any slot) first; the BVH at most once, for every sample of the call
    if ((r = begin_side_entry(s, 1, o->use_bvh && (o->rebuild_bvh || !s->cur().bvh_valid))) != RT_OK) return r;
    hipStream_t st = sstream(s);
    const int before = a.n;
    if (before == 0) {                                        // what this accumulation's samples see
        a.inst_gen = s->inst_gen; a.cam_gen = s->cam_gen; a.radius = o->radius; a.bias = o->bias;
    }
    OcclParams P;
    SceneView S;
    OcclPlan plan;
    occl_launch_setup(s, o->use_bvh != 0, P, S, plan);
    const bool host = o->host_outputs != 0;
    P.visibility = !o->visibility ? nullptr : host ? (float*)s->d_out[1] : o->visibility;
    P.occluded = !o->occluded ? nullptr : host ? (int*)s->d_out[2] : o->occluded;
    P.rgba = !o->rgba ? nullptr : host ? (uint32_t*)s->d_out[0] : o->rgba;
    a.n = 0;                                                  // a failed launch leaves no samples, not stale counts
    if (px > 0) {
        if (before == 0) HIPCHK(launch_occl_surface(plan, P, S, st, nullptr, nullptr));
        for (int done = 0; done < o->samples; done += OCCL_LAUNCH_SAMPLES) {
            P.k0 = before + done;
            P.samples = std::min(OCCL_LAUNCH_SAMPLES, o->samples - done);
            P.resolve = done + P.samples == o->samples ? 1 : 0;
            P.n_total = before + o->samples;
            HIPCHK(launch_occlusion(plan, P, S, st, nullptr, nullptr));
        }
        HIPCHK(hipGetLastError());
    }
    if ((r = end_frame(s, st)) != RT_OK) return r;
    HIPCHK(hipStreamSynchronize(st));
    a.n = before + o->samples;
    if (host) {
        if (o->visibility) HIPCHK(hipMemcpy(o->visibility, P.visibility, px * 4, hipMemcpyDeviceToHost));
        if (o->occluded) HIPCHK(hipMemcpy(o->occluded, P.occluded, px * 4, hipMemcpyDeviceToHost));
        if (o->rgba) HIPCHK(hipMemcpy(o->rgba, P.rgba, px * 4, hipMemcpyDeviceToHost));
    }
    if (n_samples) *n_samples = a.n;
    return RT_OK;
}

int rt_occlusion_reset(rt_scene* s) {
    CHECK_SCENE(s);
    occl_drop(s);
    return RT_OK;
}

int rt_occlusion_info(const rt_scene* s, int32_t* out4) {
    CHECK_SCENE(s);
    if (!out4) return fail(RT_ERR_ARG, "null argument");
    out4[0] = s->occl.n; out4[1] = s->h.cam.W; out4[2] = s->h.cam.H; out4[3] = s->occl.restarts;
    return RT_OK;
}

int rt_ao_direction(int k, float* out3) {
    if (k < 0 || k >= RT_AO_MAX_SAMPLES || !out3) return fail(RT_ERR_ARG, "rt_ao_direction: 0 <= k < 1024 and a destination");
    rto::ao_direction(k, out3);
    return RT_OK;
}

// Test hook: the rays sample k traces, formed by occlusion_kernel's own code from the surface
// record of the current accumulation (its camera, poses and bias), without tracing.
int rt_occlusion_rays(rt_scene* s, int k, float* dst, int64_t cap_floats) {
    CHECK_FINISHED(s);
    if (!dst || k < 0 || k >= RT_AO_MAX_SAMPLES) return fail(RT_ERR_ARG, "rt_occlusion_rays: 0 <= k < 1024 and a destination");
    const size_t px = (size_t)s->h.cam.W * s->h.cam.H;
    if (cap_floats < (int64_t)(px * 6)) return fail(RT_ERR_ARG, "rt_occlusion_rays: buffer below W * H * 6 floats");
    if (s->occl.n <= 0) return fail(RT_ERR_STATE, "rt_occlusion_rays: no accumulation (after rt_occlusion)");
    int r;
    if ((r = begin_side_entry(s, 1, false)) != RT_OK) return r;
    if (px == 0) return RT_OK;
    DevBuf<float> rays;
    HIPCHK(rays.alloc(px * 6));
    OcclParams P;
    SceneView S;
    OcclPlan plan;
    occl_launch_setup(s, true, P, S, plan);
    P.k0 = k; P.rays = rays.p;
    HIPCHK(launch_occl_rays(P, sstream(s)));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(sstream(s)));
    HIPCHK(hipMemcpy(dst, rays.p, px * 6 * sizeof(float), hipMemcpyDeviceToHost));
    return RT_OK;
}

void rt_query_opts_default(rt_query_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->use_bvh = 1; o->rebuild_bvh = 1;
}

// Ray queries (rt_amd.h): a side entry like rt_debug_cast, but its kernel is query_kernel, not a
// trace kernel: the scene's last trace launch and the slots' scheduling history stay as they were.
int rt_query(rt_scene* s, const rt_query_opts* o, rt_stats* stats) {
    CHECK_FINISHED(s);
    if (!o) return fail(RT_ERR_ARG, "null options");
    if (o->n < 0) return fail(RT_ERR_ARG, "rt_query: n >= 0 required");
    if (o->n == 0) return RT_OK;
    const bool by_pixel = o->pixel != nullptr;
    if (by_pixel ? (o->origin || o->dir) : !(o->origin && o->dir))
        return fail(RT_ERR_ARG, "rt_query: give either pixel, or both origin and dir");
    const bool any = o->any_hit != 0;
    if (any ? !o->hit : !(o->t || o->inst || o->tri || o->uv || o->normal || o->hit || o->rays_out))
        return fail(RT_ERR_ARG, any ? "rt_query: an occlusion query writes `hit`" : "rt_query: no output requested");
    const size_t n = (size_t)o->n;
    if (s->query_order == RT_QUERY_ORDER_SORTED && o->n > (int64_t)INT32_MAX)
        return fail(RT_ERR_LIMIT, "rt_query: RT_QUERY_ORDER_SORTED takes at most 2^31 - 1 rays (32-bit ray indices)");
    if (o->host && by_pixel)
        for (size_t i = 0; i < n; i++) {
            const int x = o->pixel[2 * i], y = o->pixel[2 * i + 1];
            if (x < 0 || y < 0 || x >= s->h.cam.W || y >= s->h.cam.H)
                return fail(RT_ERR_ARG, "rt_query: pixel " + std::to_string(i) + " is outside the canvas");
        }
    int r;
    if ((r = begin_side_entry(s, 1, false)) != RT_OK) return r;   // upload, frames in flight, current poses
    hipStream_t st = sstream(s);
    const bool counted = stats != nullptr;
    // the sorted mode's scratch, before anything of this call is in flight
    const QueryOrderPlan OP = query_order_plan(o->n, s->query_order, counted);
    if (OP.sort && (r = ensure_order_scratch(s, o->n)) != RT_OK) return r;
    if (counted) { HIPCHK(hipMemsetAsync(s->d_stats, 0, STATS_N * sizeof(unsigned long long), st)); HIPCHK(hipEventRecord(s->ev[0], st)); }
    if (o->use_bvh && (o->rebuild_bvh || !s->cur().bvh_valid) && (r = build_bvh(s, st)) != RT_OK) return r;
    if (counted) HIPCHK(hipEventRecord(s->ev[1], st));

    QueryParams Q{};
    Q.cam = s->h.d_cam; Q.n = o->n;
    Q.origin = o->origin; Q.dir = o->dir; Q.tmax = o->tmax; Q.pixel = o->pixel;
    Q.t = any ? nullptr : o->t; Q.inst = any ? nullptr : o->inst; Q.tri = any ? nullptr : o->tri;
    Q.uv = any ? nullptr : o->uv; Q.normal = any ? nullptr : o->normal;
    Q.hit = o->hit; Q.rays_out = o->rays_out;
    Q.stats = counted ? s->d_stats : nullptr;
    // host pointers: the batch as one pinned image (inputs, then outputs) and its device copy
    struct Part { const void* src; void* dst; size_t bytes, off; };
    Part in[4] = {{o->origin, nullptr, 12 * n, 0}, {o->dir, nullptr, 12 * n, 0}, {o->tmax, nullptr, 4 * n, 0}, {o->pixel, nullptr, 8 * n, 0}};
    Part out[7] = {{nullptr, Q.t, 4 * n, 0}, {nullptr, Q.inst, 4 * n, 0}, {nullptr, Q.tri, 4 * n, 0}, {nullptr, Q.uv, 8 * n, 0},
                   {nullptr, Q.normal, 12 * n, 0}, {nullptr, Q.hit, n, 0}, {nullptr, Q.rays_out, 24 * n, 0}};
    size_t in_bytes = 0, total = 0;
    if (o->host) {
        for (Part& p : in) if (p.src) { p.off = total; total += a16(p.bytes); }
        in_bytes = total;
        for (Part& p : out) if (p.dst) { p.off = total; total += a16(p.bytes); }
        if (total > s->q_cap) {
            const size_t cap = std::max(total, 2 * s->q_cap);
            dfree(s->q_dev); hfree(s->q_host); s->q_cap = 0;
            HIPCHK(hipMalloc((void**)&s->q_dev, cap));
            HIPCHK(hipHostMalloc((void**)&s->q_host, cap, hipHostMallocDefault));
            s->q_cap = cap;
        }
        for (const Part& p : in) if (p.src) memcpy(s->q_host + p.off, p.src, p.bytes);
        HIPCHK(hipMemcpyAsync(s->q_dev, s->q_host, in_bytes, hipMemcpyHostToDevice, st));
        auto dev = [&](const Part& p) { return (void*)(s->q_dev + p.off); };
        if (o->origin) { Q.origin = (const float*)dev(in[0]); Q.dir = (const float*)dev(in[1]); }
        if (o->tmax) Q.tmax = (const float*)dev(in[2]);
        if (o->pixel) Q.pixel = (const int*)dev(in[3]);
        if (Q.t) Q.t = (float*)dev(out[0]);
        if (Q.inst) Q.inst = (int*)dev(out[1]);
        if (Q.tri) Q.tri = (int*)dev(out[2]);
        if (Q.uv) Q.uv = (float*)dev(out[3]);
        if (Q.normal) Q.normal = (float*)dev(out[4]);
        if (Q.hit) Q.hit = (unsigned char*)dev(out[5]);
        if (Q.rays_out) Q.rays_out = (float*)dev(out[6]);
    }
    // The camera-ray shortcuts off (query_kernel): view_of's pruning slack folds |cam.pos| in and
    // the axis-plane path's error bound is checked for rays from there; a caller's origin is anywhere.
    SceneView S = view_of(s, o->use_bvh != 0);
    S.prune_abs = -1.0f; S.tri_ax = nullptr;
    // The zero-axis cut alone stays, with the origin's term added per ray on the device
    Q.zcut_scene = prune_slack(s, 0.0f);
    // occlusion early exit (query_kernel): one rescaling per instance at most, each < 1 + 2^-20
    const float margin = (float)S.n_inst * 0x1p-19f;
    Q.any_margin = margin <= 0.125f ? margin : -1.0f;
    int form = -1;                                             // RT_QUERY_FORM (measurements): small / persistent
    if (const char* e = getenv("RT_QUERY_FORM")) form = !strcmp(e, "small") ? 0 : !strcmp(e, "persistent") ? 1 : -1;
    const QueryVariant V = choose_query_variant(o->n, S, any, counted, s->n_cu, form, OP.sort);
    if (!V.fn)
        return fail(RT_ERR_STATE, "no query kernel <" + std::to_string(V.tree) + ", " + std::to_string((int)V.lds) + ", " +
                                      std::to_string((int)V.any_hit) + ", " + std::to_string((int)V.counted) + ", " +
                                      std::to_string((int)V.ordered) + ">");
    bool trace = true;
    if (OP.sort) {
        // key, sort, trace: stream-ordered, no host synchronisation between them.  The buffers
        // are laid out for the scratch's capacity; the sort looks at the key bits in use only.
        refresh_query_box(s);
        const QueryOrderPlan CP = query_order_plan(s->qo_rays, QUERY_ORDER_SORTED, false);
        unsigned char* p = s->qo_dev;
        unsigned long long* k_in = (unsigned long long*)p; p += CP.keys_bytes;
        unsigned long long* k_out = (unsigned long long*)p; p += CP.keys_bytes;
        uint32_t* v_in = (uint32_t*)p; p += CP.idx_bytes;
        uint32_t* v_out = (uint32_t*)p; p += CP.idx_bytes;
        HIPCHK(launch_ray_keys(Q, s->q_box, k_in, v_in, st));
        HIPCHK(ray_sort_pairs(p, s->qo_temp, k_in, k_out, v_in, v_out, o->n, OP.key_bits, st));
        Q.order = v_out;
        // RT_QUERY_SORT_ONLY (measurements, tools/query_bench.py): stop after the sort; no output is written
        if (const char* e = getenv("RT_QUERY_SORT_ONLY")) trace = atoi(e) == 0;
    }
    if (trace) HIPCHK(launch_query_kernel(V, Q, S, st));
    HIPCHK(hipGetLastError());
    s->last_query = V; s->has_last_query = true;               // rt_query_last
    s->last_query_sorted = OP.sort; s->last_query_n = o->n; s->last_query_order = Q.order;
    if (counted) HIPCHK(hipEventRecord(s->ev[2], st));
    if (o->host && total > in_bytes)
        HIPCHK(hipMemcpyAsync(s->q_host + in_bytes, s->q_dev + in_bytes, total - in_bytes, hipMemcpyDeviceToHost, st));
    if ((r = end_frame(s, st)) != RT_OK) return r;
    HIPCHK(hipStreamSynchronize(st));
    if (o->host)
        for (const Part& p : out) if (p.dst) memcpy(p.dst, s->q_host + p.off, p.bytes);   // (dst: the caller's arrays)
    if (counted) {
        unsigned long long v[4];
        HIPCHK(hipMemcpy(v, s->d_stats, sizeof v, hipMemcpyDeviceToHost));
        stats->rays = v[0]; stats->nodes = v[1]; stats->leaves = v[2]; stats->tri_tests = v[3];
        float a = 0, b = 0;
        HIPCHK(hipEventElapsedTime(&a, s->ev[0], s->ev[1]));
        HIPCHK(hipEventElapsedTime(&b, s->ev[1], s->ev[2]));
        stats->bvh_ms = a; stats->trace_ms = b;
    }
    return RT_OK;
}

int rt_query_set_order(rt_scene* s, int mode) {
    CHECK_SCENE(s);
    if (mode != RT_QUERY_ORDER_CALLER && mode != RT_QUERY_ORDER_SORTED)
        return fail(RT_ERR_ARG, "query order: RT_QUERY_ORDER_CALLER or RT_QUERY_ORDER_SORTED");
    s->query_order = mode;
    return RT_OK;
}

int rt_query_last(const rt_scene* s, int32_t* out8, float* bounds6, uint32_t* order, int64_t order_cap) {
    CHECK_FINISHED(s);
    if (!s->has_last_query) return fail(RT_ERR_STATE, "no rt_query yet");
    const QueryVariant& k = s->last_query;
    const bool sorted = s->last_query_sorted;
    if (order && sorted && order_cap < s->last_query_n) return fail(RT_ERR_ARG, "rt_query_last: order_cap is below the batch's n");
    if (out8) {
        const int32_t v[8] = {k.tree, (int32_t)k.lds, (int32_t)k.any_hit, (int32_t)k.counted, (int32_t)k.ordered,
                              (int32_t)k.persistent, k.blocks, (int32_t)sorted};
        std::copy(v, v + 8, out8);
    }
    if (bounds6) {
        const rtk::KeyBox b = sorted ? s->q_box : rtk::KeyBox{v3(0, 0, 0), v3(0, 0, 0)};
        const float v[6] = {b.mn.x, b.mn.y, b.mn.z, b.mx.x, b.mx.y, b.mx.z};
        std::copy(v, v + 6, bounds6);
    }
    if (order && sorted) {
        if (!s->last_query_order) return fail(RT_ERR_STATE, "rt_query_last: the last order's buffer was released");
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(hipMemcpy(order, s->last_query_order, (size_t)s->last_query_n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return RT_OK;
}

int rt_scene_last_trace(const rt_scene* s, int32_t* out8) {
    CHECK_FINISHED(s);
    if (!out8) return fail(RT_ERR_ARG, "null argument");
    if (!s->has_last_trace) return fail(RT_ERR_STATE, "no trace launch yet");
    const TraceKey& k = s->last_key;
    const int32_t v[8] = {k.ns_bucket, (int32_t)k.lds, k.mode, (int32_t)k.shm, (int32_t)k.part_k, (int32_t)k.sky,
                          (int32_t)k.sky_brute, s->last_ftree};
    std::copy(v, v + 8, out8);
    return RT_OK;
}

int rt_scene_set_shadow_hints(rt_scene* s, int on) {
    CHECK_SCENE(s);
    s->shadow_hints = on != 0;
    if (s->multi) set_multi_shadow_hints(s, on != 0);         // the replicas of rt_scene_set_devices too
    return RT_OK;
}

// the test hooks' prologue: the scene's device, every frame in flight done
static int hints_quiesce(rt_scene* s) {
    CHECK_FINISHED(s);
    if (!s->uploaded) return fail(RT_ERR_STATE, "scene is not on a device");
    HIPCHK(hipSetDevice(s->device));
    for (auto& f : s->slots) if (f.pending) HIPCHK(hipEventSynchronize(f.done));
    return RT_OK;
}

int rt_scene_shadow_hints_fill(rt_scene* s, int32_t value) {
    int r;
    if ((r = hints_quiesce(s)) != RT_OK) return r;
    if (!s->d_hint) return RT_OK;
    const int n_inst = (int)s->h.d_insts.size();
    std::vector<int32_t> v(hint_bytes(n_inst) / sizeof(int32_t), 0);   // the counters' words stay zero
    std::fill(v.begin(), v.begin() + hint_table_ints(n_inst), value);
    HIPCHK(hipMemcpy(s->d_hint, v.data(), v.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return RT_OK;
}

int rt_scene_shadow_hint_code(rt_scene* s, int inst, int32_t* code) {
    int r;
    if ((r = hints_quiesce(s)) != RT_OK) return r;
    if (!code || inst < 0 || inst >= (int)s->h.d_insts.size()) return fail(RT_ERR_ARG, "instance out of range or null argument");
    *code = 0;
    const rt_scene::Built& b = s->built;
    if (b.slot < 0 || !ordered_tree_usable(b.n_real, b.fdepth)) return RT_OK;
    std::vector<float4> rec(4 * (size_t)(b.n_real - 1));
    HIPCHK(hipMemcpy(rec.data(), s->slots[b.slot].d_fnode, rec.size() * sizeof(float4), hipMemcpyDeviceToHost));
    for (int k = 0; k < b.n_real - 1; k++) {                  // a record's child references: -1 - instance for a leaf
        int32_t ref[2];
        memcpy(ref, &rec[4 * (size_t)k + 3], sizeof ref);
        for (int side = 0; side < 2; side++)
            if (ref[side] == -1 - inst) *code = hint_code(k, side);
    }
    return RT_OK;
}

int rt_scene_shadow_hints_read(rt_scene* s, int32_t* dst, int64_t cap) {
    int r;
    if ((r = hints_quiesce(s)) != RT_OK) return r;
    const size_t n = s->d_hint ? hint_table_ints((int)s->h.d_insts.size()) : 0;
    if ((n && !dst) || cap < (int64_t)n) return fail(RT_ERR_ARG, "destination too small");
    if (n) HIPCHK(hipMemcpy(dst, s->d_hint, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_scene_shadow_hint_counters(rt_scene* s, uint64_t* out4) {
    int r;
    if ((r = hints_quiesce(s)) != RT_OK) return r;
    if (!out4) return fail(RT_ERR_ARG, "null argument");
    std::fill(out4, out4 + 4, 0);
    if (!s->d_hint) return RT_OK;
    const int n_inst = (int)s->h.d_insts.size();
    static_assert(HINT_COUNTERS == 3 && HINT_COUNTERS <= HINT_STRIPE_WORDS, "out4 = three counters and the entry count");
    uint64_t c[HINT_STRIPES * HINT_STRIPE_WORDS];
    HIPCHK(hipMemcpy(c, s->d_hint + hint_table_ints(n_inst), sizeof c, hipMemcpyDeviceToHost));
    for (int k = 0; k < HINT_STRIPES; k++)
        for (int i = 0; i < HINT_COUNTERS; i++) out4[i] += c[k * HINT_STRIPE_WORDS + i];
    out4[3] = hint_table_ints(n_inst);
    return RT_OK;
}

// Profiling aid (tools/group_profile.py, not on the product path): per-group durations
// (100 MHz ticks) of the fast frame kernel over rows row0, row0 + row_step, ... (compact),
// as bench.py's rank row0 of row_step renders them.  `reps` frames, each with the per-frame
// BVH rebuild; the last one (scheduled from the previous frame's history) is recorded.
// geo = {n_groups, gw, gh, n_gx}; *ms = the last frame's kernel time.  prof = 1: the recorded
// frame runs the PROF variant (when the scene has one) and out[n_groups + 12 g ..] holds group
// g's wave queries, child-pair steps, leaf visits, triangle iterations, then shader cycles in
// queries, in leaf visits, in trace_sample, after queries (state machine), and in the group; then
// (slots 9-11) cycles in the light step (ST_LIGHT), in the hit normal of a query's step, and in
// parking (writes before the query, reads after it; the reads also count in the query's cycles).
int rt_profile_groups(rt_scene* s, int spp, int row0, int row_step, int reps, int prof, uint32_t* out, int64_t cap,
                      int* geo, double* ms) {
    CHECK_FINISHED(s);
    if (!out || !geo || cap <= 0 || reps < 1 || row_step < 1 || row0 < 0) return fail(RT_ERR_ARG, "bad arguments");
    int r;
    if ((r = begin_side_entry(s, spp, false)) != RT_OK) return r;   // (the BVH: per repetition, below)
    const int rows = (s->h.cam.H - row0 + row_step - 1) / row_step;
    if (rows <= 0) return fail(RT_ERR_ARG, "no rows in the slice");
    rt_render_opts o; rt_render_opts_default(&o);
    o.spp = spp; o.row0 = row0; o.row_step = row_step; o.compact = 1;
    DevBuf<uint32_t> d_rgba;
    DevBuf<unsigned> d_g;
    HIPCHK(d_rgba.alloc((size_t)s->h.cam.W * rows));
    geo[0] = geo[1] = geo[2] = geo[3] = 0;
    reps = std::max(reps, 2);                                 // frame 0 sizes the buffer and seeds the history
    const int nw = prof ? 13 : 1;                             // prof: + 12 counters per group (PROF kernel)
    TraceRequest q;
    q.stream = sstream(s); q.rgba = d_rgba.p; q.e0 = s->ev[0]; q.e1 = s->ev[1]; q.geo = geo;
    for (int i = 0; i < reps; i++) {
        if (i == reps - 1) {                                  // the recorded frame
            if (geo[0] <= 0 || (int64_t)geo[0] * nw > cap) return fail(RT_ERR_LIMIT, "group buffer too small");
            HIPCHK(d_g.alloc((size_t)geo[0] * nw));
            HIPCHK(hipMemsetAsync(d_g.p, 0, (size_t)geo[0] * nw * sizeof(unsigned), sstream(s)));
            q.prof = prof != 0; q.gdur = d_g.p;
        }
        if ((r = build_bvh(s, sstream(s))) != RT_OK) return r;
        if ((r = launch_trace(s, o, q)) != RT_OK) return r;
    }
    if ((r = end_frame(s, sstream(s))) != RT_OK) return r;
    HIPCHK(hipEventSynchronize(s->ev[1]));
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, s->ev[0], s->ev[1]));
    if (ms) *ms = t;
    HIPCHK(hipMemcpy(out, d_g.p, (size_t)geo[0] * nw * sizeof(unsigned), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_kat_device(const char* op, int n, const float* in0, const float* in1, const float* in2, float* of, int32_t* oi,
                  uint64_t* ou) {
    static const char* ops[] = {"normalize3", "cross", "reflect", "refract", "quat_rotate", "quat_inverse", "quat_mul",
                                "tri_hit", "ray_ctor", "zorder", "to_mat3", "box_hit", "pow", "tri_hit_f", "box_hit_f",
                                "box_pair", "rcp_cr", "sqrt_cr", "box_from_local", "box_merge", "entity", "ray_key",
                                "normalized_unit", "unit_len_rcp", "reflect_unit", "reflect_pre_unit"};
    // per-op sizes (floats): in0, in1, in2, out_f, out_i, out_u per element
    static const int sz[][6] = {{3, 0, 0, 3, 0, 0}, {3, 3, 0, 3, 0, 0}, {3, 3, 0, 3, 0, 0}, {3, 3, 2, 3, 1, 0},
                                {4, 3, 0, 3, 0, 0}, {4, 0, 0, 4, 0, 0}, {4, 4, 0, 4, 0, 0}, {9, 6, 0, 3, 1, 0},
                                {6, 0, 0, 6, 0, 0}, {3, 0, 0, 0, 0, 1}, {4, 0, 0, 9, 0, 0}, {7, 6, 0, 0, 1, 0},
                                {1, 1, 0, 1, 0, 0}, {9, 6, 0, 3, 1, 0}, {7, 6, 0, 0, 1, 0}, {14, 6, 0, 0, 2, 0},
                                {1, 0, 0, 1, 0, 0}, {1, 0, 0, 1, 0, 0}, {7, 7, 0, 6, 1, 0}, {7, 7, 0, 6, 1, 0},
                                {7, 3, 0, 12, 0, 0}, {6, 6, 0, 0, 0, 1}, {3, 0, 0, 3, 0, 0}, {3, 0, 0, 2, 0, 0},
                                {3, 3, 0, 3, 0, 0}, {3, 3, 1, 3, 0, 0}};
    static_assert(sizeof ops / sizeof *ops == sizeof sz / sizeof *sz, "one size row per op");
    if (!op || n <= 0) return fail(RT_ERR_ARG, "bad arguments");
    int k = -1;
    for (int i = 0; i < (int)(sizeof ops / sizeof *ops); i++) if (!strcmp(op, ops[i])) k = i;
    if (k < 0) return fail(RT_ERR_ARG, std::string("unknown op ") + op);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(RT_ERR_NODEV, "no HIP device available");
    HIPCHK(hipSetDevice(g_device));
    const float* hin[3] = {in0, in1, in2};
    DevBuf<float> din[3], dof;
    DevBuf<int> doi;
    DevBuf<unsigned long long> dou;
    for (int i = 0; i < 3; i++)
        if (sz[k][i]) {
            if (!hin[i]) return fail(RT_ERR_ARG, "missing input");
            HIPCHK(din[i].alloc((size_t)n * sz[k][i]));
            HIPCHK(hipMemcpy(din[i].p, hin[i], (size_t)n * sz[k][i] * 4, hipMemcpyHostToDevice));
        }
    if (sz[k][3]) HIPCHK(dof.alloc((size_t)n * sz[k][3]));
    if (sz[k][4]) HIPCHK(doi.alloc((size_t)n * sz[k][4]));
    if (sz[k][5]) HIPCHK(dou.alloc((size_t)n));
    launch_kat(k, n, din[0].p, din[1].p, din[2].p, dof.p, doi.p, dou.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    if (sz[k][3] && of) HIPCHK(hipMemcpy(of, dof.p, (size_t)n * sz[k][3] * 4, hipMemcpyDeviceToHost));
    if (sz[k][4] && oi) HIPCHK(hipMemcpy(oi, doi.p, (size_t)n * sz[k][4] * 4, hipMemcpyDeviceToHost));
    if (sz[k][5] && ou) HIPCHK(hipMemcpy(ou, dou.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    return RT_OK;
}

}  // extern "C"
