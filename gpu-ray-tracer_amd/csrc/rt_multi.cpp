// rt_multi.cpp — multi-GPU frames from one host process (rt_scene_set_devices):
// the RCCL loader, the replicas with their per-slot streams and buffers (MultiDev), and the
// render / gather / un-permute sequence.  Host code only (rt_internal.h).  The frame is
// split row-cyclically into n_ranks slices (slice r = rows r, r + N, ...), the BVH and scene
// replicated on every device (each replica rebuilds the same tree from the same instance
// array, raytracer.cu:103-119), so the one exchange is the gather of the RGBA8 slices:
//   1. device i renders ranks [i k, (i+1) k) (k = n_ranks / n_devices) into its slice buffer
//      sbuf[i] = k slices of rows_max x W (compact rows; rows_max = ceil(H / N)), on its stream;
//   2. ncclGroupStart; per device ncclGather(sbuf[i], gbuf on device 0, k rows_max W uint32,
//      root 0, comm[i], stream[i]); ncclGroupEnd -- one communicator per device from
//      ncclCommInitAll, so rank order = device order = slice order;
//   3. device 0 un-permutes gbuf into the frame (unpermute_kernel).
// Several ranks per device ("virtual" ranks: n_ranks > n_devices) keep the same sequence, so a
// one-GPU box runs the whole call sequence with a one-rank communicator.  RCCL is opened
// with dlopen at the first multi-device frame (the copy torch loaded, if any): the library
// has no link-time RCCL dependency.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types only: RCCL is opened at run time (MultiDev), never linked

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "rt_internal.h"

using namespace rti;

namespace {

struct Rccl {
    void* lib = nullptr;
    ncclResult_t (*comm_init_all)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
    ncclResult_t (*gather)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*group_start)() = nullptr;
    ncclResult_t (*group_end)() = nullptr;
    const char* (*err)(ncclResult_t) = nullptr;
};
Rccl* rccl(std::string* why) {
    static Rccl R;
    static std::string reason;
    static bool tried = false;
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (!tried) {
        tried = true;
        for (const char* n : {"librccl.so", "librccl.so.1"})                 // the copy already loaded (torch's)
            if (!R.lib) R.lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
        for (const char* n : {"librccl.so.1", "/opt/rocm/lib/librccl.so.1"})
            if (!R.lib) R.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (!R.lib) { reason = std::string("cannot load RCCL: ") + dlerror(); }
        else {
            auto sym = [&](const char* n) { void* f = dlsym(R.lib, n); if (!f && reason.empty()) reason = std::string("RCCL lacks ") + n; return f; };
            R.comm_init_all = (decltype(R.comm_init_all))sym("ncclCommInitAll");
            R.comm_destroy = (decltype(R.comm_destroy))sym("ncclCommDestroy");
            R.gather = (decltype(R.gather))sym("ncclGather");
            R.group_start = (decltype(R.group_start))sym("ncclGroupStart");
            R.group_end = (decltype(R.group_end))sym("ncclGroupEnd");
            R.err = (decltype(R.err))sym("ncclGetErrorString");
        }
    }
    if (!reason.empty()) { if (why) *why = reason; return nullptr; }
    return &R;
}
}  // namespace

struct MultiDev {
    std::vector<int> devices;
    int n_ranks = 1, per_dev = 1, rows_max = 0, W = 0, H = 0;
    std::vector<rt_scene*> reps;                 // reps[0] = the scene itself; reps[i > 0] owned replicas
    std::vector<unsigned> inst_gen;              // host instance generation each replica holds
    std::vector<ncclComm_t> comms;               // one per device (ncclCommInitAll: rank = device order)
    // Frames in flight: the scene's frame slots (rt_scene_set_frame_slots) give `depth`; frame f
    // uses slot k = f % depth -- its own stream per device, slice buffers and gather buffer -- so
    // frame f + 1 renders while frame f gathers and un-permutes.  A slot's stream orders frame f
    // after frame f - depth, the last user of the slot's buffers.
    int depth = 0;
    long long frame = 0;
    std::vector<std::vector<hipStream_t>> streams;   // [device][slot]
    std::vector<std::vector<uint32_t*>> sbuf;        // [device][slot]: per_dev slices of rows_max x W
    std::vector<uint32_t*> gbuf;                     // [slot], device 0: n_ranks slices
    hipEvent_t ev_in = nullptr, ev_out = nullptr;    // device 0: caller's stream -> frame -> caller's stream
    // per device: the last frame's gather; the next frame's gather (another slot's stream) waits
    // for it, so operations on a communicator run in issue order whatever RCCL does across streams
    std::vector<hipEvent_t> gdone;
    bool gdone_pending = false;
};

namespace {
// The per-slot streams and buffers (and their device work) released; the replicas and the
// communicators stay.
void free_multi_slots(MultiDev* m) {
    for (size_t i = 0; i < m->streams.size(); i++) {
        (void)hipSetDevice(m->devices[i]);
        for (hipStream_t st : m->streams[i]) if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
        if (i < m->sbuf.size()) for (uint32_t* b : m->sbuf[i]) if (b) (void)hipFree(b);
    }
    (void)hipSetDevice(m->devices[0]);
    for (uint32_t* b : m->gbuf) if (b) (void)hipFree(b);
    m->streams.clear(); m->sbuf.clear(); m->gbuf.clear();
    m->depth = 0;
}
}  // namespace

void rti::free_multi(rt_scene* s) {
    MultiDev* m = s->multi;
    if (!m) return;
    s->multi = nullptr;
    s->ranks_per_device = 1;
    free_multi_slots(m);
    Rccl* R = rccl(nullptr);
    for (size_t i = 0; i < m->comms.size(); i++) {
        (void)hipSetDevice(m->devices[i]);
        if (R && m->comms[i]) (void)R->comm_destroy(m->comms[i]);
    }
    for (size_t i = 0; i < m->gdone.size(); i++) {
        (void)hipSetDevice(m->devices[i]);
        if (m->gdone[i]) (void)hipEventDestroy(m->gdone[i]);
    }
    (void)hipSetDevice(m->devices[0]);
    if (m->ev_in) (void)hipEventDestroy(m->ev_in);
    if (m->ev_out) (void)hipEventDestroy(m->ev_out);
    for (size_t i = 1; i < m->reps.size(); i++) delete m->reps[i];
    if (s->uploaded) (void)hipSetDevice(s->device);
    delete m;
}

namespace {
// Replica i's host scene brought up to the primary's: camera, environment, instance poses,
// atlas (the device copies follow at its next frame, as for any scene).
void sync_replica(rt_scene* s, MultiDev* m, size_t i) {
    rt_scene* r = m->reps[i];
    r->h.cam = s->h.cam; r->h.d_cam = s->h.d_cam;
    r->h.dist_atten = s->h.dist_atten; r->h.ambience = s->h.ambience; r->h.depth = s->h.depth;
    r->overlap = s->overlap;
    if (m->inst_gen[i] != s->inst_gen) {
        r->h.insts = s->h.insts; r->h.d_insts = s->h.d_insts;
        r->inst_gen++;
        invalidate(r);
        m->inst_gen[i] = s->inst_gen;
    }
    if (r->h.atlas_rgba.size() != s->h.atlas_rgba.size() || (s->atlas_dirty && !s->h.atlas_rgba.empty())) {
        r->h.atlas_rgba = s->h.atlas_rgba; r->h.atlas_w = s->h.atlas_w; r->h.atlas_h = s->h.atlas_h;
        r->atlas_dirty = true;
    }
}

// Replicas and communicators on first use; per-slot streams and buffers whenever the frame
// slots changed (the work in flight is waited for first).
int setup_multi(rt_scene* s, MultiDev* m, Rccl* R) {
    const int nd = (int)m->devices.size(), W = m->W;
    int r;
    for (int i = (int)m->reps.size(); i < nd; i++) {
        HIPCHK(hipSetDevice(m->devices[i]));
        rt_scene* rp = new rt_scene;
        rp->h = s->h; rp->finished = true;
        rp->h.atlas_rgba.clear();
        rp->overlap = s->overlap;
        rp->near_first = s->near_first;                        // (a mode set before the split holds on the replicas)
        rp->ranks_per_device = m->per_dev;
        m->reps.push_back(rp);
        m->inst_gen.push_back(0);
        const int saved = g_device;
        g_device = m->devices[i];
        r = upload(rp);
        g_device = saved;
        if (r != RT_OK) return r;
    }
    if (m->gdone.empty()) {
        m->gdone.assign(nd, nullptr);
        for (int i = 0; i < nd; i++) {
            HIPCHK(hipSetDevice(m->devices[i]));
            HIPCHK(hipEventCreateWithFlags(&m->gdone[i], hipEventDisableTiming));
        }
    }
    if (m->comms.empty()) {
        m->comms.assign(nd, nullptr);
        ncclResult_t e = R->comm_init_all(m->comms.data(), nd, m->devices.data());
        if (e != ncclSuccess) { m->comms.clear(); return fail(RT_ERR_HIP, std::string("ncclCommInitAll: ") + R->err(e)); }
    }
    HIPCHK(hipSetDevice(m->devices[0]));
    if (!m->ev_in) HIPCHK(hipEventCreateWithFlags(&m->ev_in, hipEventDisableTiming));
    if (!m->ev_out) HIPCHK(hipEventCreateWithFlags(&m->ev_out, hipEventDisableTiming));
    const int D = s->n_slots;
    if (m->depth == D) return RT_OK;
    free_multi_slots(m);
    for (int i = 1; i < nd; i++) {                             // replicas rotate as many frame slots
        m->reps[i]->overlap = s->overlap;
        if ((r = rt_scene_set_frame_slots(m->reps[i], D)) != RT_OK) return r;
    }
    m->streams.assign(nd, std::vector<hipStream_t>(D, nullptr));
    m->sbuf.assign(nd, std::vector<uint32_t*>(D, nullptr));
    m->gbuf.assign(D, nullptr);
    for (int i = 0; i < nd; i++) {
        HIPCHK(hipSetDevice(m->devices[i]));
        for (int k = 0; k < D; k++) {
            HIPCHK(hipStreamCreateWithFlags(&m->streams[i][k], hipStreamNonBlocking));
            HIPCHK(hipMalloc((void**)&m->sbuf[i][k], (size_t)m->per_dev * m->rows_max * W * 4));
        }
    }
    HIPCHK(hipSetDevice(m->devices[0]));
    for (int k = 0; k < D; k++) HIPCHK(hipMalloc((void**)&m->gbuf[k], (size_t)m->n_ranks * m->rows_max * W * 4));
    m->depth = D;
    m->frame = 0;
    m->gdone_pending = false;
    return RT_OK;
}

}  // namespace

void rti::set_multi_overlap(rt_scene* s, int policy) {
    for (rt_scene* rp : s->multi->reps) rp->overlap = policy;
}
void rti::set_multi_near_first(rt_scene* s, int mode) {
    for (rt_scene* rp : s->multi->reps) rp->near_first = mode;
}
void rti::set_multi_shadow_hints(rt_scene* s, bool on) {
    for (rt_scene* rp : s->multi->reps) rp->shadow_hints = on;
}

int rti::render_multi(rt_scene* s, const rt_render_opts* o, rt_stats* stats) {
    MultiDev* m = s->multi;
    if (o->radiance || o->hit_inst || o->hit_tri) return fail(RT_ERR_ARG, "multi-device frames write RGBA8 only");
    std::string why;
    Rccl* R = rccl(&why);
    if (!R) return fail(RT_ERR_STATE, why);
    const int nd = (int)m->devices.size(), N = m->n_ranks, W = s->h.cam.W, H = s->h.cam.H;
    int r;
    if (m->W != W || m->H != H) return fail(RT_ERR_STATE, "canvas size changed after rt_scene_set_devices");
    if ((r = setup_multi(s, m, R)) != RT_OK) return r;
    for (int i = 1; i < nd; i++) sync_replica(s, m, i);
    const int k = (int)(m->frame % m->depth);
    hipStream_t caller = o->stream ? (hipStream_t)o->stream : nullptr;
    if (caller) {                                          // the caller's work before this frame (its output buffer)
        HIPCHK(hipSetDevice(m->devices[0]));
        HIPCHK(hipEventRecord(m->ev_in, caller));
    }
    unsigned long long tot[4] = {0, 0, 0, 0};
    double bvh_ms = 0, trace_ms = 0;
    // 1. every rank's slice, on its device's stream of this slot.  Event timing (o->timing)
    // covers the first device's ranks (the scene's own rt_timing_collect); replicas untimed.
    for (int i = 0; i < nd; i++) {
        double dev_bvh = 0, dev_trace = 0;
        for (int j = 0; j < m->per_dev; j++) {
            rt_render_opts so = *o;
            so.row0 = i * m->per_dev + j; so.row_step = N; so.compact = 1;
            so.rgba = m->sbuf[i][k] + (size_t)j * m->rows_max * W;
            so.stream = m->streams[i][k]; so.host_outputs = 0; so.sync = 0;
            if (i > 0) so.timing = 0;
            rt_stats st{};
            if ((r = rt_render(m->reps[i], &so, stats ? &st : nullptr)) != RT_OK) return r;
            if (stats) {
                tot[0] += st.rays; tot[1] += st.nodes; tot[2] += st.leaves; tot[3] += st.tri_tests;
                dev_bvh += st.bvh_ms; dev_trace += st.trace_ms;
            }
        }
        bvh_ms = std::max(bvh_ms, dev_bvh); trace_ms = std::max(trace_ms, dev_trace);
    }
    // 2. the gather to device 0 (one communicator per device, grouped)
    const size_t cnt = (size_t)m->per_dev * m->rows_max * W;
    if (m->gdone_pending)                                  // after the previous frame's gather (issue order)
        for (int i = 0; i < nd; i++) {
            HIPCHK(hipSetDevice(m->devices[i]));
            HIPCHK(hipStreamWaitEvent(m->streams[i][k], m->gdone[i], 0));
        }
    ncclResult_t e = R->group_start();
    for (int i = 0; i < nd && e == ncclSuccess; i++) {
        HIPCHK(hipSetDevice(m->devices[i]));
        e = R->gather(m->sbuf[i][k], i == 0 ? m->gbuf[k] : nullptr, cnt, ncclUint32, 0, m->comms[i], m->streams[i][k]);
    }
    ncclResult_t e2 = R->group_end();
    if (e == ncclSuccess) e = e2;
    if (e != ncclSuccess) return fail(RT_ERR_HIP, std::string("ncclGather: ") + R->err(e));
    for (int i = 0; i < nd; i++) {
        HIPCHK(hipSetDevice(m->devices[i]));
        HIPCHK(hipEventRecord(m->gdone[i], m->streams[i][k]));
    }
    m->gdone_pending = true;
    // 3. un-permute on device 0 into the caller's buffer (after the caller's earlier work on it)
    // or the canvas
    HIPCHK(hipSetDevice(m->devices[0]));
    hipStream_t s0 = m->streams[0][k];
    if (caller) HIPCHK(hipStreamWaitEvent(s0, m->ev_in, 0));
    uint32_t* out = (o->rgba && !o->host_outputs) ? o->rgba : s->d_canvas;
    const long long px = (long long)W * H;
    rtd::launch_unpermute(m->gbuf[k], out, W, H, N, m->rows_max, s0);
    HIPCHK(hipGetLastError());
    if (caller) {                                          // the caller's stream continues after the frame
        HIPCHK(hipEventRecord(m->ev_out, s0));
        HIPCHK(hipStreamWaitEvent(caller, m->ev_out, 0));
    }
    m->frame++;
    if (o->sync || o->host_outputs || stats)               // this frame only: the other slots keep running
        for (int i = 0; i < nd; i++) { HIPCHK(hipSetDevice(m->devices[i])); HIPCHK(hipStreamSynchronize(m->streams[i][k])); }
    HIPCHK(hipSetDevice(m->devices[0]));
    if (o->host_outputs && o->rgba) HIPCHK(hipMemcpy(o->rgba, out, (size_t)px * 4, hipMemcpyDeviceToHost));
    if (stats) {
        // counters summed over ranks; bvh_ms / trace_ms: the slowest device's summed kernel times
        // (its ranks run one after another on its stream), the frame's parallel kernel time
        stats->rays = tot[0]; stats->nodes = tot[1]; stats->leaves = tot[2]; stats->tri_tests = tot[3];
        stats->bvh_ms = bvh_ms; stats->trace_ms = trace_ms;
    }
    return RT_OK;
}

extern "C" int rt_scene_set_devices(rt_scene* s, const int* devices, int n_devices, int n_ranks) {
    CHECK_FINISHED(s);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(RT_ERR_NODEV, "no HIP device available");
    if (!devices || n_devices < 1 || n_ranks < n_devices || n_ranks % n_devices != 0)
        return fail(RT_ERR_ARG, "n_devices >= 1 device indices, n_ranks a multiple of n_devices");
    for (int i = 0; i < n_devices; i++) {
        if (devices[i] < 0 || devices[i] >= ndev) return fail(RT_ERR_ARG, "device index out of range");
        for (int j = 0; j < i; j++) if (devices[j] == devices[i]) return fail(RT_ERR_ARG, "a device listed twice");
    }
    if (n_ranks > s->h.cam.H) return fail(RT_ERR_ARG, "more ranks than canvas rows");
    int r;
    if (s->uploaded && s->device != devices[0]) return fail(RT_ERR_STATE, "devices[0] must be the scene's device");
    if (!s->uploaded) {
        const int saved = g_device;
        g_device = devices[0];
        r = upload(s);
        g_device = saved;
        if (r != RT_OK) return r;
    }
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());
    free_multi(s);
    if (n_devices == 1 && n_ranks == 1) return RT_OK;       // back to single-device frames
    MultiDev* m = new MultiDev;
    m->devices.assign(devices, devices + n_devices);
    m->n_ranks = n_ranks; m->per_dev = n_ranks / n_devices;
    m->W = s->h.cam.W; m->H = s->h.cam.H;
    m->rows_max = (m->H + n_ranks - 1) / n_ranks;
    m->reps.push_back(s);
    m->inst_gen.push_back(s->inst_gen);
    s->multi = m;
    s->ranks_per_device = m->per_dev;
    return RT_OK;
}
