// rt_occlusion.cpp — the ambient occlusion pass (rt_occlusion): the scene-owned direction table,
// surface record and counts, the reset / info entries and the rays' test hook; the history across
// camera moves (rt_occlusion_set_history): the previous frame's buffers, the move.  Host code only
// (rt_internal.h); its kernels are the occlusion kernels, reached through rt_device.h.
#include <cmath>
#include <cstring>

#include "rt_internal.h"

using namespace rtd;
using namespace rti;

namespace {
static_assert(RT_AO_MAX_SAMPLES == rto::AO_MAX_SAMPLES, "the direction table's length");
static_assert(RT_AO_INTERLEAVED_MAX_SAMPLES == rto::AO_INTERLEAVED_MAX_SAMPLES, "the interleaved pattern's samples");
static_assert(RT_AO_PATTERN_SHARED == OCCL_PATTERN_SHARED && RT_AO_PATTERN_INTERLEAVED == OCCL_PATTERN_INTERLEAVED, "the patterns");

// Has anything that decides an occlusion sample changed since the accumulation's first one?
bool occl_stale(const rt_scene* s, float radius, float bias) {
    const rt_scene::Occl& a = s->occl;
    return a.n > 0 && (a.inst_gen != s->inst_gen || a.cam_gen != s->cam_gen || a.radius != radius || a.bias != bias);
}
void occl_drop(rt_scene* s) {
    if (s->occl.n > 0) s->occl.restarts++;
    s->occl.n = 0;
    s->occl.drop_history();
}
// With history on: does this call find samples held whose camera alone changed?  It moves them
// (reprojection) where occl_stale alone would drop them.
bool occl_moves(const rt_scene* s, const rt_occlusion_opts* o) {
    const rt_scene::Occl& a = s->occl;
    return a.hist_on && !o->restart && a.n > 0 && a.cam_gen != s->cam_gen && a.inst_gen == s->inst_gen && a.radius == o->radius &&
           a.bias == o->bias && a.acc_cam.W == s->h.d_cam.W && a.acc_cam.H == s->h.d_cam.H;
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
// The history's buffers beside them: the weights of the accumulation held and the previous frame's
// record, counts and weights.  A failed allocation leaves none of the set.
int ensure_occl_history(rt_scene* s) {
    rt_scene::Occl& a = s->occl;
    if (a.hist_px >= a.px) return RT_OK;
    a.release_history();
    if (hipMalloc((void**)&a.d_weight, a.px * sizeof(int32_t)) != hipSuccess ||
        hipMalloc((void**)&a.d_prev_surf, 2 * a.px * sizeof(float4)) != hipSuccess ||
        hipMalloc((void**)&a.d_prev_count, a.px * sizeof(int32_t)) != hipSuccess ||
        hipMalloc((void**)&a.d_prev_weight, a.px * sizeof(int32_t)) != hipSuccess) {
        const std::string why = hipGetErrorString(hipGetLastError());
        a.release_history();
        return fail(RT_ERR_HIP, "rt_occlusion: no memory for the history of " + std::to_string(a.px) + " pixels: " + why);
    }
    a.hist_px = a.px;
    return RT_OK;
}
// The kernels' arguments and scene view for the current slot: the occlusion rays start on the
// surfaces, not at the camera, so the view is the one for a caller's rays (caller_ray_view).
void occl_launch_setup(rt_scene* s, bool use_bvh, OcclParams& P, SceneView& S, OcclPlan& plan) {
    const rt_scene::Occl& a = s->occl;
    const CallerView v = caller_ray_view(s, use_bvh);
    S = v.S;
    P = OcclParams{};
    P.cam = s->h.d_cam; P.W = s->h.cam.W; P.H = s->h.cam.H;
    P.radius = a.radius; P.bias = a.bias;
    P.zcut_scene = v.zcut_scene; P.any_margin = v.any_margin;
    P.table = a.d_table; P.surf = a.d_surf; P.count = a.d_count;
    P.pattern = a.pattern; P.normal_min = a.normal_min; P.plane_tol = a.plane_tol;
    P.weight = a.d_weight;
    int map = -1;                                              // RT_OCCL_MAP (measurements): row / tile / class (interleaved only)
    if (const char* e = getenv("RT_OCCL_MAP"))
        map = !strcmp(e, "row") ? OCCL_MAP_ROW : !strcmp(e, "tile") ? OCCL_MAP_TILE : !strcmp(e, "class") ? OCCL_MAP_CLASS : -1;
    plan = occlusion_plan(P.W, P.H, S, map, a.pattern);
    P.map = plan.map; P.n_waves = plan.n_waves;
}
// The surface record is built under the shared pattern's plan whatever the pattern (occl_surface_kernel
// knows the shared maps only; no result depends on the map).
hipError_t launch_surface_record(const OcclPlan& plan, OcclParams P, SceneView& S, hipStream_t st) {
    OcclPlan sp = plan;
    if (plan.map == OCCL_MAP_CLASS) {
        sp = occlusion_plan(P.W, P.H, S, -1, OCCL_PATTERN_SHARED);
        P.map = sp.map; P.n_waves = sp.n_waves;
    }
    return launch_occl_surface(sp, P, S, st, nullptr, nullptr);
}
int pattern_capacity(int pattern) { return pattern == RT_AO_PATTERN_INTERLEAVED ? RT_AO_INTERLEAVED_MAX_SAMPLES : RT_AO_MAX_SAMPLES; }
}  // namespace

extern "C" {

void rt_occlusion_opts_default(rt_occlusion_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->samples = 1; o->radius = INFINITY; o->bias = RT_AO_BIAS_DEFAULT; o->use_bvh = 1; o->rebuild_bvh = 1;
}

// Ambient occlusion (rt_amd.h): a side entry like rt_query.  Its kernels are the occlusion kernels,
// not a trace kernel: the scene's last trace launch and the slots' scheduling history stay as they were.
int rt_occlusion(rt_scene* s, const rt_occlusion_opts* o, int* n_samples) {
    CHECK_FINISHED(s);
    if (!o) return fail(RT_ERR_ARG, "null options");
    if (o->samples < 1) return fail(RT_ERR_ARG, "rt_occlusion: samples >= 1 required");
    if (!(o->radius > 0.0f)) return fail(RT_ERR_ARG, "rt_occlusion: radius > 0 required (+inf: sky visibility)");
    if (!(o->bias >= 0.0f && std::isfinite(o->bias))) return fail(RT_ERR_ARG, "rt_occlusion: bias must be finite and >= 0");
    if (!(o->visibility || o->occluded || o->rgba)) return fail(RT_ERR_ARG, "rt_occlusion: no output requested");
    const bool move = occl_moves(s, o);                       // history on: only the camera changed
    const bool fresh = !move && (o->restart || occl_stale(s, o->radius, o->bias));
    if ((long long)(fresh || move ? 0 : s->occl.n) + o->samples > pattern_capacity(s->occl.pattern))
        return fail(RT_ERR_LIMIT, s->occl.pattern == RT_AO_PATTERN_INTERLEAVED
                                      ? "rt_occlusion: more than 64 samples held in the interleaved pattern (rt_occlusion_reset starts again)"
                                      : "rt_occlusion: more than 1024 samples held (rt_occlusion_reset starts again)");
    if (s->multi) return fail(RT_ERR_STATE, "rt_occlusion: not on a scene split by rt_scene_set_devices");
    int r;
    if ((r = upload(s)) != RT_OK) return r;
    HIPCHK(hipSetDevice(s->device));
    const size_t px = (size_t)s->h.cam.W * s->h.cam.H;
    if (px > (size_t)INT32_MAX / 8) return fail(RT_ERR_LIMIT, "rt_occlusion: frame larger than 2^28 pixels");
    if (fresh) occl_drop(s);
    if ((r = ensure_occl(s)) != RT_OK) return r;
    if (s->occl.hist_on && (r = ensure_occl_history(s)) != RT_OK) return r;
    if (o->host_outputs && (r = ensure_out_staging(s)) != RT_OK) return r;
    rt_scene::Occl& a = s->occl;
    // frames in flight (any slot) first; the BVH at most once, for every sample of the call
    if ((r = begin_side_entry(s, 1, s->builds_bvh(o->use_bvh, o->rebuild_bvh))) != RT_OK) return r;
    hipStream_t st = sstream(s);
    const int cap = pattern_capacity(a.pattern);
    const int before = move ? 0 : a.n;                        // samples held since the last move or drop
    const long long cursor = a.hist_on ? a.cursor : before;   // this call's first sample is number `cursor`
    const int n_prev = a.n;                                   // a move: the samples of the frame being left
    const rt::DCamera prev_cam = a.acc_cam;
    if (before == 0 && !move) {                               // what this accumulation's samples see
        a.inst_gen = s->inst_gen; a.radius = o->radius; a.bias = o->bias;
    }
    if (before == 0) { a.cam_gen = s->cam_gen; a.acc_cam = s->h.d_cam; }
    if (move) {                                               // the accumulation being left becomes the previous frame
        std::swap(a.d_surf, a.d_prev_surf); std::swap(a.d_count, a.d_prev_count); std::swap(a.d_weight, a.d_prev_weight);
    }
    const bool weighted = a.hist_on && (a.weighted || move);  // per-pixel totals: a move since the last drop
    OcclParams P;
    SceneView S;
    OcclPlan plan;
    occl_launch_setup(s, o->use_bvh != 0, P, S, plan);
    const bool host = o->host_outputs != 0;
    P.visibility = !o->visibility ? nullptr : host ? (float*)s->d_out[1] : o->visibility;
    P.occluded = !o->occluded ? nullptr : host ? (int*)s->d_out[2] : o->occluded;
    P.rgba = !o->rgba ? nullptr : host ? (uint32_t*)s->d_out[0] : o->rgba;
    // the filtered resolve: the last launch resolves `occluded` only, occl_filter_kernel the other two;
    // with per-pixel totals no counting launch resolves: occl_resolve_kernel / occl_filter_kernel<true> do
    OcclParams F = P;
    const bool filter = a.filter != 0 && (P.visibility || P.rgba);
    if (filter || weighted) { P.visibility = nullptr; P.rgba = nullptr; }
    a.last_map = plan.map;
    a.n = 0;                                                  // a failed launch leaves no samples, not stale counts
    a.drop_history();
    const bool held = a.hist_on && n_prev > 0;                // ... and, with history, counts as a restart (taken back below)
    if (held) a.restarts++;
    bool timed = false, timed_h = false, timed_r = false;
    if (px > 0) {
        if (a.time_history && !a.hev[0])
            for (hipEvent_t& e : a.hev) HIPCHK(hipEventCreate(&e));
        if (before == 0) HIPCHK(launch_surface_record(plan, P, S, st));
        if (move) {                                           // every pixel's seed from the frame just left
            OcclReprojParams R{};
            R.prev_cam = prev_cam; R.W = P.W; R.H = P.H; R.n_prev = n_prev; R.max_history = a.max_history;
            R.normal_min = a.hist_normal_min; R.plane_tol = a.hist_plane_tol;
            R.surf = a.d_surf; R.prev_surf = a.d_prev_surf; R.prev_count = a.d_prev_count; R.prev_weight = a.d_prev_weight;
            R.count = a.d_count; R.weight = a.d_weight;
            timed_r = a.time_history;
            HIPCHK(launch_occl_reproject(R, st, timed_r ? a.hev[0] : nullptr, timed_r ? a.hev[1] : nullptr));
        } else if (a.hist_on && before == 0) {
            HIPCHK(hipMemsetAsync(a.d_weight, 0, px * sizeof(int32_t), st));   // no move yet: every n_h is 0
        }
        // sample number K uses the pattern's index K mod capacity: launches of at most
        // OCCL_LAUNCH_SAMPLES, none across the table's wrap (at most one: the limit above)
        for (int done = 0; done < o->samples;) {
            P.k0 = (int)((cursor + done) % cap);
            P.samples = std::min(std::min(OCCL_LAUNCH_SAMPLES, o->samples - done), cap - P.k0);
            done += P.samples;
            P.accumulate = (move || before + done - P.samples > 0) ? 1 : 0;
            P.resolve = (done == o->samples && !weighted) ? 1 : 0;
            P.n_total = before + o->samples;
            HIPCHK(launch_occlusion(plan, P, S, st, nullptr, nullptr));
        }
        F.n_total = before + o->samples;
        if (weighted && (F.occluded || !filter)) {
            OcclParams E = F;
            if (filter) { E.visibility = nullptr; E.rgba = nullptr; }
            timed_h = a.time_history && !filter;
            HIPCHK(launch_occl_resolve(E, st, timed_h ? a.hev[2] : nullptr, timed_h ? a.hev[3] : nullptr));
        }
        if (filter) {                                         // (a dispatch takes one pair of events: the history's first)
            timed_h = weighted && a.time_history;
            timed = a.time_filter && !timed_h;
            if (timed && !a.ev0) { HIPCHK(hipEventCreate(&a.ev0)); HIPCHK(hipEventCreate(&a.ev1)); }
            hipEvent_t e0 = timed_h ? a.hev[2] : timed ? a.ev0 : nullptr, e1 = timed_h ? a.hev[3] : timed ? a.ev1 : nullptr;
            HIPCHK(weighted ? launch_occl_filter_history(plan, F, st, e0, e1) : launch_occl_filter(plan, F, st, e0, e1));
        }
        HIPCHK(hipGetLastError());
    }
    if ((r = end_frame(s, st)) != RT_OK) return r;
    HIPCHK(hipStreamSynchronize(st));
    a.n = before + o->samples;
    if (held) a.restarts--;
    if (a.hist_on) {
        a.cursor = cursor + o->samples;
        a.weighted = weighted;
        if (move) a.moves++;
    }
    if (timed) HIPCHK(hipEventElapsedTime(&a.filter_ms, a.ev0, a.ev1));
    if (timed_r) HIPCHK(hipEventElapsedTime(&a.reproject_ms, a.hev[0], a.hev[1]));
    if (timed_h) {
        HIPCHK(hipEventElapsedTime(&a.resolve_ms, a.hev[2], a.hev[3]));
        if (filter && a.time_filter) a.filter_ms = a.resolve_ms;
    }
    if (host) {
        if (o->visibility) HIPCHK(hipMemcpy(o->visibility, F.visibility, px * 4, hipMemcpyDeviceToHost));
        if (o->occluded) HIPCHK(hipMemcpy(o->occluded, F.occluded, px * 4, hipMemcpyDeviceToHost));
        if (o->rgba) HIPCHK(hipMemcpy(o->rgba, F.rgba, px * 4, hipMemcpyDeviceToHost));
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

// The direction pattern (rt_amd.h): part of what an accumulation was started with.
int rt_occlusion_set_pattern(rt_scene* s, int pattern) {
    CHECK_SCENE(s);
    if (pattern != RT_AO_PATTERN_SHARED && pattern != RT_AO_PATTERN_INTERLEAVED)
        return fail(RT_ERR_ARG, "rt_occlusion_set_pattern: RT_AO_PATTERN_SHARED or RT_AO_PATTERN_INTERLEAVED");
    if (pattern == s->occl.pattern) return RT_OK;
    occl_drop(s);
    s->occl.pattern = pattern;
    return RT_OK;
}

// The filtered resolve (rt_amd.h): outputs only, the counts do not depend on it.
int rt_occlusion_set_filter(rt_scene* s, int on, float normal_min, float plane_tol) {
    CHECK_SCENE(s);
    if (on != 0 && on != 1) return fail(RT_ERR_ARG, "rt_occlusion_set_filter: on is 0 or 1");
    if (!(normal_min >= -1.0f && normal_min <= 1.0f)) return fail(RT_ERR_ARG, "rt_occlusion_set_filter: normal_min in [-1, 1] required");
    if (!(plane_tol >= 0.0f && std::isfinite(plane_tol))) return fail(RT_ERR_ARG, "rt_occlusion_set_filter: plane_tol must be finite and >= 0");
    s->occl.filter = on;
    if (on) { s->occl.normal_min = normal_min; s->occl.plane_tol = plane_tol; }
    return RT_OK;
}

// History across camera moves (rt_amd.h): part of what an accumulation was started with, the two
// thresholds excepted (they are read at the next move).
int rt_occlusion_set_history(rt_scene* s, int on, int max_history, float normal_min, float plane_tol) {
    CHECK_SCENE(s);
    if (on != 0 && on != 1) return fail(RT_ERR_ARG, "rt_occlusion_set_history: on is 0 or 1");
    if (max_history < 1 || max_history > RT_AO_MAX_SAMPLES) return fail(RT_ERR_ARG, "rt_occlusion_set_history: 1 <= max_history <= 1024 required");
    if (!(normal_min >= -1.0f && normal_min <= 1.0f)) return fail(RT_ERR_ARG, "rt_occlusion_set_history: normal_min in [-1, 1] required");
    if (!(plane_tol >= 0.0f && std::isfinite(plane_tol))) return fail(RT_ERR_ARG, "rt_occlusion_set_history: plane_tol must be finite and >= 0");
    rt_scene::Occl& a = s->occl;
    if (on != a.hist_on || max_history != a.max_history) occl_drop(s);
    a.hist_on = on; a.max_history = max_history;
    a.hist_normal_min = normal_min; a.hist_plane_tol = plane_tol;
    return RT_OK;
}

int rt_occlusion_history_info(const rt_scene* s, int32_t* out8, float* f2) {
    CHECK_SCENE(s);
    const rt_scene::Occl& a = s->occl;
    if (out8) {
        out8[0] = a.hist_on; out8[1] = a.max_history; out8[2] = a.moves;
        out8[3] = (int32_t)std::min<long long>(a.cursor, INT32_MAX);
        out8[4] = a.n; out8[5] = a.weighted ? 1 : 0; out8[6] = 0; out8[7] = 0;
    }
    if (f2) { f2[0] = a.hist_normal_min; f2[1] = a.hist_plane_tol; }
    return RT_OK;
}

// Test hook: the history weights of the accumulation held (zeros while no move has seeded them).
int rt_occlusion_history_weights(rt_scene* s, int32_t* dst, int64_t cap) {
    CHECK_FINISHED(s);
    const size_t px = (size_t)s->h.cam.W * s->h.cam.H;
    if (!dst || cap < (int64_t)px) return fail(RT_ERR_ARG, "rt_occlusion_history_weights: a destination of W * H int32");
    if (s->occl.n <= 0) return fail(RT_ERR_STATE, "rt_occlusion_history_weights: no accumulation (after rt_occlusion)");
    if (!s->occl.weighted || px == 0) { memset(dst, 0, px * sizeof(int32_t)); return RT_OK; }
    HIPCHK(hipSetDevice(s->device));                          // (rt_occlusion returned after its stream's sync)
    HIPCHK(hipMemcpy(dst, s->occl.d_weight, px * sizeof(int32_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

// Measurement hook: the times of occl_reproject_kernel and of the kernel that resolves with
// per-pixel totals (occl_resolve_kernel, or occl_filter_kernel<true>), by events on their dispatches.
int rt_occlusion_history_timing(rt_scene* s, int on, float* ms2) {
    CHECK_SCENE(s);
    s->occl.time_history = on != 0;
    if (ms2) { ms2[0] = s->occl.reproject_ms; ms2[1] = s->occl.resolve_ms; }
    return RT_OK;
}

// Measurement hook: occl_filter_kernel's own time, by start/stop events on its dispatch.
int rt_occlusion_filter_timing(rt_scene* s, int on, float* ms) {
    CHECK_SCENE(s);
    s->occl.time_filter = on != 0;
    if (ms) *ms = s->occl.filter_ms;
    return RT_OK;
}

int rt_occlusion_config(const rt_scene* s, int32_t* out4, float* f2) {
    CHECK_SCENE(s);
    const rt_scene::Occl& a = s->occl;
    if (out4) { out4[0] = a.pattern; out4[1] = a.filter; out4[2] = pattern_capacity(a.pattern); out4[3] = a.last_map; }
    if (f2) { f2[0] = a.normal_min; f2[1] = a.plane_tol; }
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
    if (k >= pattern_capacity(s->occl.pattern)) return fail(RT_ERR_ARG, "rt_occlusion_rays: 0 <= k < 64 in the interleaved pattern");
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

}  // extern "C"
