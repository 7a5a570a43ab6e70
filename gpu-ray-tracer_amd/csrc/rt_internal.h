// rt_internal.h — the scene object and what the host translation units share: rt_runtime.cpp
// (upload, frame slots, BVH build and trace launch, rt_render), rt_build.cpp (scene creation,
// exports, camera), rt_accumulate.cpp, rt_occlusion.cpp, rt_query.cpp, rt_shade.cpp (one entry family each),
// rt_hooks.cpp (debugging, profiling and test hooks), rt_multi.cpp (multi-device frames) and
// rt_copy.cpp (copy-engine entries).  What rt_query and rt_shade share is written once here: the
// staging of a batch with host pointers (BatchStage, stage_inputs, fetch_outputs, copy_outputs), the argument
// checks (check_ray_inputs, check_host_pixels, check_sorted_limit) and the sort (sort_rays).
// Internal functions live in namespace rti: the library's rt_* C symbols (rt_amd.h) stay its only
// interface.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rt_device.h"
#include "../../include/rt_amd.h"

struct MultiDev;   // rt_multi.cpp

namespace rti {

int fail(int code, const std::string& msg);   // records the thread's error text (rt_last_error)
extern thread_local int g_device;             // rt_set_device: the device new scenes upload to

template <class T> void dfree(T*& p) { if (p) { (void)hipFree(p); p = nullptr; } }
template <class T> void hfree(T*& p) { if (p) { (void)hipHostFree(p); p = nullptr; } }
// A device allocation that lives as long as its scope (the side entries' temporary buffers):
// freed on every return path, HIPCHK's early ones included.
template <class T> struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { dfree(p); }
    hipError_t alloc(size_t n) { return hipMalloc((void**)&p, n * sizeof(T)); }   // n elements
};
// The staging of an entry that takes a batch with host pointers (rt_query, rt_shade: one each): a
// pinned host image of the batch (rtd::batch_plan: inputs, then outputs) and its device copy.  They
// grow and are kept, so a warm call allocates nothing; a failed growth leaves the entry without
// staging, otherwise as it was.  `who` names the entry and n the batch in the error text.
struct BatchStage {
    unsigned char* host = nullptr; unsigned char* dev = nullptr; size_t cap = 0;
    rtd::BatchPlan plan{};                       // the layout of the batch it holds (stage_inputs)
    void release() { dfree(dev); hfree(host); cap = 0; }
    int ensure(size_t total, const char* who, long long n) {
        if (total <= cap) return RT_OK;
        const size_t grown = std::max(total, 2 * cap);
        release();
        if (hipMalloc((void**)&dev, grown) != hipSuccess || hipHostMalloc((void**)&host, grown, hipHostMallocDefault) != hipSuccess) {
            const std::string why = hipGetErrorString(hipGetLastError());
            release();
            return fail(RT_ERR_HIP, std::string(who) + ": no memory to stage " + std::to_string(n) + " rays: " + why);
        }
        cap = grown;
        return RT_OK;
    }
};

// Host framebuffer in pinned memory: rt_update_scene's device-to-host copy of the frame (the
// reference's post-condition, raytracer.cu:102-120) is then one direct transfer; into pageable
// memory HIP stages it in chunks through a bounce buffer.  Pageable fallback when pinning fails
// (no HIP device: the scene is still built and exported, nothing is rendered).
struct HostCanvas {
    uint32_t* p = nullptr;
    size_t n = 0;
    bool pinned = false;
    HostCanvas() = default;
    HostCanvas(const HostCanvas&) = delete;
    HostCanvas& operator=(const HostCanvas&) = delete;
    ~HostCanvas() { release(); }
    void release() {
        if (p) { if (pinned) (void)hipHostFree(p); else free(p); }
        p = nullptr; n = 0; pinned = false;
    }
    void assign(size_t m, uint32_t v) {
        release();
        if (!m) return;
        if (hipHostMalloc((void**)&p, m * sizeof(uint32_t), hipHostMallocDefault) == hipSuccess) {
            pinned = true;
        } else {
            (void)hipGetLastError();
            p = static_cast<uint32_t*>(malloc(m * sizeof(uint32_t)));
            if (!p) return;
        }
        n = m;
        std::fill(p, p + m, v);
    }
    uint32_t* data() { return p; }
    const uint32_t* data() const { return p; }
    size_t size() const { return n; }
    uint32_t operator[](size_t i) const { return p[i]; }
};

// The per-frame state, one record per frame slot (rt_scene_set_frame_slots): with n > 1 slots,
// consecutive frames rotate through n of these (BVH, work counters, scheduling history), so a
// frame on another stream can start on CUs freed by the previous frames' tails.
// Instance arrays are per-slot state too (rt_builder_set_trans after finish): a frame in
// flight keeps the poses its BVH was built from, and the next frame of a slot receives the
// current poses by a stream-ordered copy (sync_slot_insts) from the slot's pinned staging.
struct FrameSlot {
    rtm::Box* d_tree = nullptr; float4* d_node_pair = nullptr; int* d_leaf = nullptr;
    float4* d_fnode = nullptr;                   // ordered LBVH (fast kernel)
    void* d_bscratch = nullptr;                  // bvh_build_large's sort buffers (scenes above BVH_WG_LEAVES)
    int* d_work = nullptr;                       // null: the slot is not allocated yet
    bool work_zeroed = false;                    // bvh_build_kernel zeroed d_work for the next trace launch
    bool bvh_valid = false;
    // longest-first scheduling history (TraceParams::hist): double-buffered by frame parity
    int* d_hlist[2] = {nullptr, nullptr};
    unsigned char* d_hflag[2] = {nullptr, nullptr};
    unsigned long long* d_hctl = nullptr;        // [2][count, sum]
    int hist_cap = 0, hist_parity = 0;
    int hctl_zeroed = -1;                        // heavy-list slot the pending bvh_build_kernel zeroes (-1: none)
    long long hist_key[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    unsigned char* d_gsky = nullptr; int gsky_cap = 0;   // sky pre-pass flags (TraceParams::gsky)
    int* d_live = nullptr; int live_cap = 0;             // sky pre-pass live-group lists [NQ][live_cap]
    rt::DInst* d_insts = nullptr; float4* d_inst4 = nullptr;
    rt::DInst* h_insts_pin = nullptr; float4* h_inst4_pin = nullptr;   // pinned staging of the two
    unsigned inst_gen = 0;                       // instance generation the slot's arrays hold
    // Last frame of the slot (recorded on its stream, also with one slot): the next frame of
    // the slot, and side entries (debug_cast, experiments), wait for it stream-ordered.
    hipEvent_t done = nullptr;
    bool pending = false;

    void release() {
        dfree(d_tree); dfree(d_node_pair); dfree(d_leaf); dfree(d_fnode); dfree(d_bscratch); dfree(d_work);
        for (int p = 0; p < 2; p++) { dfree(d_hlist[p]); dfree(d_hflag[p]); }
        dfree(d_hctl); dfree(d_gsky); dfree(d_live);
        dfree(d_insts); dfree(d_inst4);
        hfree(h_insts_pin); hfree(h_inst4_pin);
        if (done) { (void)hipEventDestroy(done); done = nullptr; }
    }
};

}  // namespace rti

#ifndef RT_OVERLAP_DEFAULT
#define RT_OVERLAP_DEFAULT RT_OVERLAP_HALF   // (RT_OVERLAP_FULL: the A/B arm of round 3's policy)
#endif
#ifndef RT_MAX_SLOTS
#define RT_MAX_SLOTS 8
#endif

inline bool hints_default() { const char* e = getenv("RT_SHADOW_HINTS"); return !e || atoi(e) != 0; }
// RT_NEAR_FIRST in the environment: 0 off (the A/B arm), 2 the profiling variant too; default on
inline int near_first_default() {
    const char* e = getenv("RT_NEAR_FIRST");
    const int m = e ? atoi(e) : rtd::NF_ON;
    return m == rtd::NF_OFF || m == rtd::NF_PROFILE ? m : rtd::NF_ON;
}

struct rt_scene {
    rt::Scene h;
    MultiDev* multi = nullptr;                   // rt_scene_set_devices: frames split over several GPUs
    bool finished = false;
    int device = -1;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // device buffers shared by every frame slot
    rt::DTri* d_tris = nullptr; rt::DMesh* d_meshes = nullptr; rt::DMat* d_mats = nullptr;
    rt::DLight* d_lights = nullptr; rtm::Box* d_mesh_box = nullptr;
    int n_real = 0, fdepth = 0;                  // ordered LBVH (fast kernel): leaves, depth
    rtm::TriAx* d_tri_ax = nullptr;              // axis-plane triangle records (tri_axis_records)
    int n_cu = 0;
    float2* d_spp = nullptr; int spp_cap = 0;
    unsigned long long* d_stats = nullptr;
    // Shadow-query occluder hints (SceneView::hint): the scene's table and counters, shared by
    // every frame slot (frames in flight race on it benignly: aligned word stores of a hint);
    // null for scenes of the grid-wide BVH build.  shadow_hints: rt_scene_set_shadow_hints.
    int* d_hint = nullptr;
    bool shadow_hints = hints_default();         // (RT_SHADOW_HINTS=0 in the environment: off, the A/B arm)
    int near_first = near_first_default();       // rtd::NF_* (rt_plan.h): rt_scene_set_near_first
    uint32_t* d_canvas = nullptr;
    int* d_dbg = nullptr;
    float4* d_atlas = nullptr;                   // atlas texels (float4, byte / 255)
    bool atlas_dirty = false;
    void* d_out[4] = {nullptr, nullptr, nullptr, nullptr};   // staging for host_outputs
    struct Query {
        rti::BatchStage stage;                   // rt_query with host pointers
        // rt_query_set_order: the mode (host state), and the sorted mode's scratch for qo_rays rays
        // (query_order_plan: keys and ray indices, double-buffered, then hipCUB's qo_temp bytes); it
        // grows like the staging and is kept.  box: the keys' quantisation box, for the poses of box_gen.
        int order = RT_QUERY_ORDER_CALLER;
        unsigned char* qo_dev = nullptr; long long qo_rays = 0; size_t qo_temp = 0;
        rtk::KeyBox box{{0, 0, 0}, {0, 0, 0}};
        unsigned box_gen = 0;
        // the most recent rt_query (rt_query_last): its kernel and launch, whether the batch was
        // sorted, its size, the box its keys used and the device array of its order; host state
        rtd::QueryVariant last{};
        bool has_last = false, last_sorted = false;
        long long last_n = 0;
        const uint32_t* last_order = nullptr;
        void release() { stage.release(); rti::dfree(qo_dev); qo_rays = 0; qo_temp = 0; last_order = nullptr; }
    } query;
    struct Shade {
        rti::BatchStage stage;                   // rt_shade with host pointers: its own, not Query's
        // the most recent rt_shade (rt_shade_last): its kernel and launch, whether the batch was sorted, its size
        rtd::ShadeVariant last{};
        bool has_last = false, last_sorted = false;
        long long last_n = 0;
        void release() { stage.release(); }
    } shade;
    std::vector<hipEvent_t> tev;    // timing=1 events, 4 per frame: bvh start/stop, trace start/stop (pool)
    size_t tev_used = 0;
    size_t d_out_px = 0;
    int n_leaf = 0;
    bool uploaded = false;
    rti::HostCanvas canvas;          // host framebuffer (Canvas buffer, canvas.cu:7), pinned
    int overlap = RT_OVERLAP_DEFAULT;            // rt_scene_set_overlap
    int ranks_per_device = 1;                    // > 1: virtual ranks of rt_scene_set_devices share this device
    unsigned inst_gen = 1;                       // generation of the host instance array (set_trans bumps it)
    unsigned shape_gen = 0;                      // generation n_real / fdepth were computed for
    // generations of what else decides a sample (rt_accumulate's staleness test): the camera
    // (rt_camera_*), the environment (rt_env_set) and the atlas (rt_scene_set_atlas)
    unsigned cam_gen = 1, env_gen = 1, atlas_gen = 1;
    // rt_accumulate: the scene-owned running sums of `n` samples (raw and clamped per sample), the
    // pass buffer a sample is traced into, sample 0's kept hit ids, and what the first sample saw
    // (generations, the textures flag).  Allocated on first use (px pixels), freed with the scene;
    // rt_render and rt_update_scene never touch them.
    struct Accum {
        float4 *d_sum_r = nullptr, *d_sum_c = nullptr, *d_pass = nullptr;
        int32_t *d_hit_inst = nullptr, *d_hit_tri = nullptr;
        size_t px = 0;
        int n = 0, restarts = 0;
        unsigned inst_gen = 0, cam_gen = 0, env_gen = 0, atlas_gen = 0;
        int textures = 0;
        // Adaptive mode (rt_accumulate_set_adaptive, rt_adapt.h): the switch and its threshold (host
        // state); the mask of needed tiles, their live-group lists [NQ][live_q] and the image of the
        // work counters a refinement pass starts from (WORK_INTS ints),
        // for tile_cap tiles: allocated on first adaptive use, freed with the scene, owned by the
        // accumulation and not by a frame slot.  have_mask: decided for the samples held (dropped
        // with them); needed: its count, read back once; traced: the tiles the last pass's trace
        // launch was given.
        int mode = 0;
        float threshold = 8.0f / 255.0f;
        unsigned char* d_need = nullptr;
        int *d_live = nullptr, *d_image = nullptr;
        int tile_cap = 0;
        rtad::TileGrid tiles{};
        bool have_mask = false;
        bool count_pending = false;              // needed not read back yet (a call that failed before its sync leaves it so)
        int needed = -1, traced = 0;
        void release_adaptive() { rti::dfree(d_need); rti::dfree(d_live); rti::dfree(d_image); tile_cap = 0; have_mask = false; count_pending = false; needed = -1; }
        void release() {
            rti::dfree(d_sum_r); rti::dfree(d_sum_c); rti::dfree(d_pass); rti::dfree(d_hit_inst); rti::dfree(d_hit_tri); px = 0;
            release_adaptive();
        }
    } accum;
    // rt_occlusion: the scene-owned direction table, the surface record of every pixel's primary hit
    // (2 float4 a pixel, built with sample 0) and the counts of occluded samples, `n` samples held;
    // what sample 0 saw (generations, radius, bias).  Allocated on first use, freed with the scene.
    struct Occl {
        rtm::V3* d_table = nullptr;
        float4* d_surf = nullptr;
        int32_t* d_count = nullptr;
        size_t px = 0;
        int n = 0, restarts = 0;
        unsigned inst_gen = 0, cam_gen = 0;
        float radius = 0.0f, bias = 0.0f;
        // rt_occlusion_set_pattern / _set_filter: the direction pattern (what the samples held were
        // traced with: a change drops them) and the filtered resolve (outputs only); the lane
        // mapping the last call used (rt_occlusion_config)
        int pattern = RT_AO_PATTERN_SHARED, filter = 0, last_map = -1;
        float normal_min = RT_AO_FILTER_NORMAL_DEFAULT, plane_tol = RT_AO_FILTER_PLANE_DEFAULT;
        // rt_occlusion_filter_timing (measurements): start/stop events on occl_filter_kernel's dispatch
        bool time_filter = false;
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        float filter_ms = -1.0f;
        // rt_occlusion_set_history: the settings; the camera of the accumulation held;
        // the sample cursor (samples traced since the last drop, across moves), the moves so far and
        // whether a move since the last drop has seeded the weights.  d_weight: the history weights
        // n_h of the accumulation held (zeros before a move); d_prev_*: the frame a move left, the
        // pointers swapped with the current ones at a move.  Allocated on first use with history on
        // (hist_px: the pixels they hold).
        int hist_on = 0, max_history = RT_AO_HISTORY_DEFAULT, moves = 0;
        long long cursor = 0;
        bool weighted = false;
        float hist_normal_min = RT_AO_FILTER_NORMAL_DEFAULT, hist_plane_tol = RT_AO_FILTER_PLANE_DEFAULT;
        rt::DCamera acc_cam{};
        int32_t* d_weight = nullptr;
        float4* d_prev_surf = nullptr;
        int32_t *d_prev_count = nullptr, *d_prev_weight = nullptr;
        size_t hist_px = 0;
        // rt_occlusion_history_timing (measurements): events on the reproject and resolve dispatches
        bool time_history = false;
        hipEvent_t hev[4] = {nullptr, nullptr, nullptr, nullptr};
        float reproject_ms = -1.0f, resolve_ms = -1.0f;
        void drop_history() { cursor = 0; weighted = false; }
        void release_history() {
            rti::dfree(d_weight); rti::dfree(d_prev_surf); rti::dfree(d_prev_count); rti::dfree(d_prev_weight);
            hist_px = 0;
        }
        void release() {
            rti::dfree(d_table); rti::dfree(d_surf); rti::dfree(d_count); px = 0; n = 0;
            release_history();
            drop_history();
            if (ev0) (void)hipEventDestroy(ev0);
            if (ev1) (void)hipEventDestroy(ev1);
            ev0 = ev1 = nullptr;
            for (hipEvent_t& e : hev) {
                if (e) (void)hipEventDestroy(e);
                e = nullptr;
            }
        }
    } occl;
    static constexpr int MAX_SLOTS = RT_MAX_SLOTS;
    rti::FrameSlot slots[MAX_SLOTS];             // slots[0, n_slots) are in rotation (FrameSlot)
    int n_slots = 1, cur_slot = 0;
    // the most recent trace launch (rt_scene_last_trace): the key launch_trace launched with and
    // the SceneView::ftree it saw; host state only
    rtd::TraceKey last_key{};
    int last_ftree = 0;
    bool has_last_trace = false;
    // the most recent BVH build (RT_EXPORT_BVH_*): its frame slot (-1: none yet), the ordered
    // tree's shape it was launched with and which build ran (rtb::bvh_form); host state only
    struct Built { int slot = -1, n_real = 0, fdepth = 0, form = 0; } built;
    rti::FrameSlot& cur() { return slots[cur_slot]; }
    const rti::FrameSlot& cur() const { return slots[cur_slot]; }
    // does a call with these options build the current slot's BVH?
    bool builds_bvh(int use_bvh, int rebuild_bvh) const { return use_bvh && (rebuild_bvh || !cur().bvh_valid); }
    ~rt_scene();
};

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return rti::fail(RT_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)
#define CHECK_SCENE(s) do { if (!(s)) return rti::fail(RT_ERR_ARG, "null scene"); } while (0)
#define CHECK_BUILDING(s) do { CHECK_SCENE(s); if ((s)->finished) return rti::fail(RT_ERR_STATE, "scene already finished"); } while (0)
#define CHECK_FINISHED(s) do { CHECK_SCENE(s); if (!(s)->finished) return rti::fail(RT_ERR_STATE, "scene not finished (call rt_builder_finish)"); } while (0)

namespace rti {

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
// Capacities of the per-frame layout buffers for n_groups pixel groups.
struct Layout { int flags, sky_blocks, live_q, live; };
// A scene view for a caller's rays, the zero-axis cut's scene term and the early-exit margin.
struct CallerView { rtd::SceneView S; float zcut_scene, any_margin; };

// rt_runtime.cpp
int upload(rt_scene* s);          // device buffers of a finished scene on g_device (once)
void invalidate(rt_scene* s);     // every slot's BVH is stale (instances moved)
hipStream_t sstream(rt_scene* s);
int begin_side_entry(rt_scene* s, int spp, bool bvh);
int end_frame(rt_scene* s, hipStream_t st);
int build_bvh(rt_scene* s, hipStream_t st, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
int launch_trace(rt_scene* s, const rt_render_opts& o, const TraceRequest& q);
rtd::SceneView view_of(const rt_scene* s, bool use_bvh);
CallerView caller_ray_view(const rt_scene* s, bool use_bvh);
Layout layout_of(int n_groups);
int ensure_out_staging(rt_scene* s);
int clear_stats(rt_scene* s, hipStream_t st);
int read_frame_stats(rt_scene* s, rt_stats* stats);
std::vector<rtm::Box> mesh_boxes(const rt::Scene& h);
int warm_scene(rt_scene* s);
int scene_atlas(rt_scene* s);     // the atlas texels on the device, as a textured trace launch ensures them (RT_ERR_STATE without an atlas)
// rt_query.cpp: the coherence sort's pieces, shared with rt_shade.cpp.  refresh_query_box: the keys'
// quantisation box (rt_scene::Query::box) for the current poses.  ensure_order_scratch: the scene's
// sort scratch for a batch of n rays (query_order_plan's layout at the capacity, then hipCUB's
// temporary storage); `who` names the entry in the error text.  sort_rays: key, sort, index on `st`
// for the batch B describes; the device array of the batch's order (in the scene's scratch).
void refresh_query_box(rt_scene* s);
int ensure_order_scratch(rt_scene* s, long long n, const char* who);
int sort_rays(rt_scene* s, const rtd::RayBatch& B, int key_bits, hipStream_t st, const uint32_t** order);

// ---- What rt_query and rt_shade share; `who` names the entry in the error texts.
// The argument checks, each entry in its own order: a batch comes by pixel, or by origin and dir;
// pixels in host memory lie on the W x H canvas; the sorted order's ray indices are 32-bit.
inline int check_ray_inputs(const char* who, const void* origin, const void* dir, const void* pixel) {
    if (pixel ? (origin || dir) : !(origin && dir)) return fail(RT_ERR_ARG, std::string(who) + ": give either pixel, or both origin and dir");
    return RT_OK;
}
inline int check_host_pixels(const char* who, const int32_t* pixel, size_t n, int W, int H) {
    for (size_t i = 0; i < n; i++)
        if (pixel[2 * i] < 0 || pixel[2 * i + 1] < 0 || pixel[2 * i] >= W || pixel[2 * i + 1] >= H)
            return fail(RT_ERR_ARG, std::string(who) + ": pixel " + std::to_string(i) + " is outside the canvas");
    return RT_OK;
}
inline int check_sorted_limit(const char* who, int order, int64_t n) {
    if (order == RT_QUERY_ORDER_SORTED && n > (int64_t)INT32_MAX)
        return fail(RT_ERR_LIMIT, std::string(who) + ": RT_QUERY_ORDER_SORTED takes at most 2^31 - 1 rays (32-bit ray indices)");
    return RT_OK;
}
// A batch with host pointers through the staging g.  stage_inputs: the parts laid out (g.plan), g
// grown to hold them, the inputs copied into the image, its host-to-device copy issued and every
// present part's parameter field pointed at the part's device copy.  fetch_outputs, after the
// kernel: the outputs' device-to-host copy issued.  copy_outputs, after the stream's
// synchronisation: the outputs into the caller's arrays.
inline int stage_inputs(BatchStage& g, rtd::BatchPart* parts, size_t n_parts, const char* who, long long n, hipStream_t st) {
    g.plan = rtd::batch_plan(parts, n_parts);
    if (int r = g.ensure(g.plan.total, who, n)) return r;
    for (const rtd::BatchPart* p = parts; p < parts + n_parts; p++) {
        if (p->present && !p->output) memcpy(g.host + p->off, p->host, p->bytes);
        if (p->present) p->bind(p->field, g.dev + p->off);
    }
    HIPCHK(hipMemcpyAsync(g.dev, g.host, g.plan.in_bytes, hipMemcpyHostToDevice, st));
    return RT_OK;
}
inline int fetch_outputs(BatchStage& g, hipStream_t st) {
    const size_t in = g.plan.in_bytes;
    if (g.plan.total > in) HIPCHK(hipMemcpyAsync(g.host + in, g.dev + in, g.plan.total - in, hipMemcpyDeviceToHost, st));
    return RT_OK;
}
inline void copy_outputs(const BatchStage& g, const rtd::BatchPart* parts, size_t n_parts) {
    for (const rtd::BatchPart* p = parts; p < parts + n_parts; p++)
        if (p->present && p->output) memcpy(p->host, g.host + p->off, p->bytes);
}
// rt_multi.cpp
int render_multi(rt_scene* s, const rt_render_opts* o, rt_stats* stats);
void free_multi(rt_scene* s);
void set_multi_overlap(rt_scene* s, int policy);   // the replicas of rt_scene_set_devices
void set_multi_shadow_hints(rt_scene* s, bool on);
void set_multi_near_first(rt_scene* s, int mode);

// Mean kernel time (*ms) over `reps` runs of launch(i), which puts its work between ev[0] and
// ev[1] on the scene's stream; with more than one run the first is left out.
template <class F> int mean_ms(rt_scene* s, int reps, double* ms, F launch) {
    float total = 0;
    for (int i = 0; i < reps; i++) {
        int r;
        if ((r = launch(i)) != RT_OK) return r;
        HIPCHK(hipEventSynchronize(s->ev[1]));
        float t = 0; HIPCHK(hipEventElapsedTime(&t, s->ev[0], s->ev[1]));
        if (i > 0 || reps == 1) total += t;
    }
    *ms = total / (reps > 1 ? reps - 1 : 1);
    return RT_OK;
}

}  // namespace rti
