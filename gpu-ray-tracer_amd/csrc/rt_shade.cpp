// rt_shade.cpp — shading caller-supplied rays (rt_shade): the integrator's radiance for rays the
// caller forms or for the camera's rays of one sample of given pixels, and rt_shade_last.
// Host code only (rt_internal.h); the state lives in rt_scene::Shade, the sort's scratch and key
// box in rt_scene::Query (rt_query.cpp's helpers).
#include <cstring>
#include <iterator>

#include "rt_internal.h"

using namespace rtm;
using namespace rtd;
using namespace rti;

extern "C" {

void rt_shade_opts_default(rt_shade_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->use_bvh = 1; o->rebuild_bvh = 1;
}

// A side entry like rt_query (rt_amd.h): its kernel is shade_kernel, not a trace kernel, so the
// scene's last trace launch, the slots' scheduling history, the hint table and every counter stay
// as they were.
int rt_shade(rt_scene* s, const rt_shade_opts* o) {
    CHECK_FINISHED(s);
    if (!o) return fail(RT_ERR_ARG, "null options");
    if (o->n < 0) return fail(RT_ERR_ARG, "rt_shade: n >= 0 required");
    int r;
    if ((r = check_ray_inputs("rt_shade", o->origin, o->dir, o->pixel)) != RT_OK) return r;
    if (o->sample < 0) return fail(RT_ERR_ARG, "rt_shade: sample >= 0 required");
    if (!(o->radiance || o->rgba || o->rays_out)) return fail(RT_ERR_ARG, "rt_shade: no output requested");
    if (o->order != RT_QUERY_ORDER_CALLER && o->order != RT_QUERY_ORDER_SORTED)
        return fail(RT_ERR_ARG, "rt_shade: order is RT_QUERY_ORDER_CALLER or RT_QUERY_ORDER_SORTED");
    const size_t n = (size_t)o->n;
    if (o->host && o->pixel && (r = check_host_pixels("rt_shade", o->pixel, n, s->h.cam.W, s->h.cam.H)) != RT_OK) return r;
    if (o->sample >= 65536) return fail(RT_ERR_LIMIT, "rt_shade: sample < 65536 required");
    if ((r = check_sorted_limit("rt_shade", o->order, o->n)) != RT_OK) return r;
    // one block per 256 rays, no stride loop: the grid's 2^31 - 1 blocks bound the batch (shade_plan)
    if (o->n > (int64_t)SHADE_BLOCK * INT32_MAX)
        return fail(RT_ERR_LIMIT, "rt_shade: at most 256 (2^31 - 1) rays a call");
    if (o->textures && s->h.atlas_rgba.empty())
        return fail(RT_ERR_STATE, "textured shading needs an atlas: rt_scene_load_atlas / rt_scene_set_atlas");
    if (o->n == 0) return RT_OK;
    if ((r = begin_side_entry(s, 1, false)) != RT_OK) return r;   // upload, frames in flight, current poses
    hipStream_t st = sstream(s);
    rt_scene::Shade& ss = s->shade;
    // the sorted order's scratch (the scene's, shared with rt_query), before anything of this call is in flight
    const QueryOrderPlan OP = query_order_plan(o->n, o->order, false);
    if (OP.sort && (r = ensure_order_scratch(s, o->n, "rt_shade")) != RT_OK) return r;
    if (o->textures && (r = scene_atlas(s)) != RT_OK) return r;
    if (s->builds_bvh(o->use_bvh, o->rebuild_bvh) && (r = build_bvh(s, st)) != RT_OK) return r;

    ShadeParams Q{};
    Q.cam = s->h.d_cam; Q.n = o->n;
    Q.origin = o->origin; Q.dir = o->dir; Q.pixel = o->pixel; Q.sample = o->sample;
    Q.radiance = reinterpret_cast<float4*>(o->radiance); Q.rgba = o->rgba; Q.rays_out = o->rays_out;
    // host pointers: the batch staged (inputs, then outputs) and these fields pointed at its device copy
    BatchPart parts[] = {in_part(Q.origin, 12 * n), in_part(Q.dir, 12 * n), in_part(Q.pixel, 8 * n),
                         out_part(Q.radiance, 16 * n), out_part(Q.rgba, 4 * n), out_part(Q.rays_out, 24 * n)};
    if (o->host && (r = stage_inputs(ss.stage, parts, std::size(parts), "rt_shade", o->n, st)) != RT_OK) return r;
    // The scene for rays from anywhere: camera-ray shortcuts off; view_of leaves the hint table and
    // the counters unbound and near-first off (only launch_trace binds them), so the hint and
    // near-first counters do not move because of this call.
    CallerView cv = caller_ray_view(s, o->use_bvh != 0);
    SceneView& S = cv.S;
    // The launch's TraceParams: zeros, then exactly what trace_sample, hit_kd and dbg read --
    //   depth, dist_atten, ambience              the environment as rt_env_set left it
    //   unlit_skip, occl_exit                    shade_shortcuts of an uncounted frame without a debug pixel
    //   atlas, atlas_w, atlas_h                  the textured kernels' hit_kd
    //   hit_inst, hit_tri, stats, dbg_log        null: no hit ids, no counters, no event log
    //   dbg_x, dbg_y                             -1: no debug pixel
    // A field trace_sample comes to read later must be set here too.
    const rt::Scene& h = s->h;
    const ShadeShortcuts sc = shade_shortcuts(h, false, false, -1);
    TraceParams P{};
    P.depth = h.depth; P.dist_atten = h.dist_atten; P.ambience = h.ambience;
    P.unlit_skip = sc.unlit_skip; P.occl_exit = sc.occl_exit;
    if (o->textures) { P.atlas = s->d_atlas; P.atlas_w = h.atlas_w; P.atlas_h = h.atlas_h; }
    P.hit_inst = nullptr; P.hit_tri = nullptr; P.stats = nullptr; P.dbg_log = nullptr;
    P.dbg_x = -1; P.dbg_y = -1;
    const ShadeVariant V = choose_shade_variant(o->n, S, sc.ns, o->textures != 0);
    if (!V.fn)
        return fail(RT_ERR_STATE, "no shade kernel <" + std::to_string(V.ns_bucket) + ", " + std::to_string(V.tree) + ", " +
                                      std::to_string((int)V.tex) + ">");
    if (OP.sort) {
        // key, sort and index as rt_query: the keys of the same inputs (pixel mode: the pixels'
        // sample-0 rays, whose order is every sample's).  The order lives in the scene's sort
        // scratch, which rt_query's last order may share: that order is gone (rt_query_last).
        s->query.last_order = nullptr;
        if ((r = sort_rays(s, RayBatch{Q.cam, Q.n, Q.origin, Q.dir, Q.pixel}, OP.key_bits, st, &Q.order)) != RT_OK) return r;
    }
    HIPCHK(launch_shade_kernel(V, P, S, Q, st));
    HIPCHK(hipGetLastError());
    ss.last = V; ss.has_last = true; ss.last_sorted = OP.sort; ss.last_n = o->n;   // rt_shade_last
    if (o->host && (r = fetch_outputs(ss.stage, st)) != RT_OK) return r;
    if ((r = end_frame(s, st)) != RT_OK) return r;
    HIPCHK(hipStreamSynchronize(st));
    if (o->host) copy_outputs(ss.stage, parts, std::size(parts));
    return RT_OK;
}

int rt_shade_last(const rt_scene* s, int32_t* out8) {
    CHECK_FINISHED(s);
    const rt_scene::Shade& ss = s->shade;
    if (!ss.has_last) return fail(RT_ERR_STATE, "no rt_shade yet");
    if (out8) {
        const int32_t v[8] = {ss.last.ns_bucket, ss.last.tree, (int32_t)ss.last.tex, (int32_t)ss.last_sorted, ss.last.blocks,
                              (int32_t)(ss.last_n & 0x7fffffff), 0, 0};
        std::copy(v, v + 8, out8);
    }
    return RT_OK;
}

}  // extern "C"
