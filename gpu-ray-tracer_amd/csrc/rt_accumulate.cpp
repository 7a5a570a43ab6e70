// rt_accumulate.cpp — progressive refinement (rt_accumulate): the scene-owned sums, adaptive
// mode's tile mask and lists, the reset / info entries, the pass buffer's test hooks and the
// timing aids of tools/accum_bench.py.  Host code only (rt_internal.h); the trace launches go
// through launch_trace (rt_runtime.cpp).
#include <cmath>
#include <cstring>

#include "rt_internal.h"

using namespace rtd;
using namespace rti;

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

extern "C" {

void rt_accum_opts_default(rt_accum_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->samples = 1; o->use_bvh = 1; o->rebuild_bvh = 1;
}

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
    if ((r = begin_side_entry(s, 1, s->builds_bvh(o->use_bvh, o->rebuild_bvh))) != RT_OK) return r;
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
    return mean_ms(s, reps, ms, [&](int i) -> int {
        HIPCHK(launch_accum_fold(pass.p, sr.p, sc.p, (int)px, i, resolve != 0, rgba.p, rad.p, st, s->ev[0], s->ev[1]));
        return RT_OK;
    });
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
        r = mean_ms(s, reps, &ms4[k], [&](int i) -> int {
            if (k == 0) HIPCHK(launch_accum_edge(a.d_sum_c, a.tiles, a.threshold, need.p, st, s->ev[0], s->ev[1]));
            if (k == 1) {
                HIPCHK(hipMemsetAsync(image.p, 0, WORK_INTS * sizeof(int), st));
                HIPCHK(launch_accum_lists(a.d_need, nt, live.p, live_q, image.p, st, s->ev[0], s->ev[1]));
            }
            if (k >= 2) HIPCHK(launch_accum_fold_tiles(pass.p, sr.p, sc.p, a.d_need, a.tiles, 1 + i, k == 3, rgba.p, rad.p, st, s->ev[0], s->ev[1]));
            return RT_OK;
        });
        if (r != RT_OK) return r;
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

}  // extern "C"
