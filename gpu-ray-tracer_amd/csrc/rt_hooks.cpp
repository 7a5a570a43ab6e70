// rt_hooks.cpp — debugging, profiling and test hooks built on launch_trace (rt_runtime.cpp):
// rt_debug_cast, rt_experiment, rt_frame_work, rt_profile_groups, the device KATs, the
// scheduling-history and last-trace reports, and the shadow-hint switch with its test hooks.
// Host code only (rt_internal.h).
#include <cstring>

#include "rt_internal.h"

using namespace rtd;
using namespace rti;

extern "C" {

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
        double mean = 0;
        r = mean_ms(s, reps, &mean, [&](int) -> int {
            int e;
            if ((e = clear_stats(s, sstream(s))) != RT_OK) return e;
            HIPCHK(hipEventRecord(s->ev[0], sstream(s)));
            if ((e = launch_trace(s, o, q)) != RT_OK) return e;
            HIPCHK(hipEventRecord(s->ev[1], sstream(s)));
            return RT_OK;
        });
        if (r != RT_OK) return r;
        if ((r = end_frame(s, sstream(s))) != RT_OK) return r;
        unsigned long long v[22];
        HIPCHK(hipMemcpy(v, s->d_stats, sizeof v, hipMemcpyDeviceToHost));
        if (counters) for (int i = 0; i < 22; i++) counters[i] = v[i];
        if (ms) *ms = mean;
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

// Test hook: the current frame slot's scheduling-history state as the host holds it.
int rt_scene_history_info(const rt_scene* s, int32_t* out12) {
    CHECK_FINISHED(s);
    if (!out12) return fail(RT_ERR_ARG, "null argument");
    const FrameSlot& f = s->cur();
    out12[0] = f.hist_parity; out12[1] = f.hctl_zeroed; out12[2] = f.hist_cap; out12[3] = s->cur_slot;
    for (int i = 0; i < 8; i++) out12[4 + i] = (int32_t)f.hist_key[i];
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

int rt_scene_set_near_first(rt_scene* s, int mode) {
    CHECK_SCENE(s);
    if (mode != NF_OFF && mode != NF_ON && mode != NF_PROFILE) return fail(RT_ERR_ARG, "near-first mode: 0, 1 or 2");
    s->near_first = mode;
    if (s->multi) set_multi_near_first(s, mode);
    return RT_OK;
}

int rt_scene_near_first_counters(rt_scene* s, uint64_t* out3) {
    int r;
    if ((r = hints_quiesce(s)) != RT_OK) return r;
    if (!out3) return fail(RT_ERR_ARG, "null argument");
    std::fill(out3, out3 + NF_COUNTERS, 0);
    if (!s->d_hint) return RT_OK;
    static_assert(NF_COUNTER0 >= HINT_COUNTERS && NF_COUNTER0 + NF_COUNTERS <= HINT_STRIPE_WORDS, "one stripe holds both sets");
    uint64_t c[HINT_STRIPES * HINT_STRIPE_WORDS];
    HIPCHK(hipMemcpy(c, s->d_hint + hint_table_ints((int)s->h.d_insts.size()), sizeof c, hipMemcpyDeviceToHost));
    for (int k = 0; k < HINT_STRIPES; k++)
        for (int i = 0; i < NF_COUNTERS; i++) out3[i] += c[k * HINT_STRIPE_WORDS + NF_COUNTER0 + i];
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
