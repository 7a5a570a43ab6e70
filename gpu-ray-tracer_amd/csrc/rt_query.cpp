// rt_query.cpp — ray queries (rt_query): caller-supplied rays cast for the closest hit or for
// occlusion, the coherence sort's scratch and key box, rt_query_set_order and rt_query_last.
// Host code only (rt_internal.h); the state lives in rt_scene::Query.
#include <cmath>
#include <cstring>
#include <iterator>

#include "rt_internal.h"

using namespace rtm;
using namespace rtb;
using namespace rtd;
using namespace rti;
using rt::DInst;

// The quantisation box of rt_query's coherence keys (rt_raykey.h): the instances' world boxes
// (bvh_inst_box's arithmetic: the mesh box moved by the instance pose) merged, on the host,
// for the current poses; the same box with and without the BVH.  Degenerate and non-finite
// boxes are left out (no box at all: zeros, every origin in cell 0).
void rti::refresh_query_box(rt_scene* s) {
    rt_scene::Query& qs = s->query;
    if (qs.box_gen == s->inst_gen) return;
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
    qs.box = any ? kb : rtk::KeyBox{v3(0, 0, 0), v3(0, 0, 0)};
    qs.box_gen = s->inst_gen;
}

// The sorted mode's scratch for a batch of n rays (query_order_plan's layout at the capacity,
// then hipCUB's temporary storage, whose size is asked once per capacity).  A failed allocation
// leaves the scene without scratch, otherwise as it was.
int rti::ensure_order_scratch(rt_scene* s, long long n, const char* who) {
    rt_scene::Query& qs = s->query;
    if (n <= qs.qo_rays) return RT_OK;
    const long long cap = std::min<long long>(std::max(n, 2 * qs.qo_rays), INT32_MAX);
    const QueryOrderPlan P = query_order_plan(cap, QUERY_ORDER_SORTED, false);
    const size_t temp = (ray_sort_temp_bytes(cap, P.key_bits) + 255) & ~(size_t)255;
    dfree(qs.qo_dev); qs.qo_rays = 0; qs.qo_temp = 0;
    qs.last_order = nullptr;                                   // (rt_query_last: the last order went with the buffer)
    if (hipMalloc((void**)&qs.qo_dev, P.scratch_bytes + temp) != hipSuccess) {
        qs.qo_dev = nullptr;
        return fail(RT_ERR_HIP, std::string(who) + ": no memory for the sort of " + std::to_string(n) + " rays: " +
                                    hipGetErrorString(hipGetLastError()));
    }
    qs.qo_rays = cap; qs.qo_temp = temp;
    return RT_OK;
}

// Key, sort, index: stream-ordered, no host synchronisation between them.  The buffers are laid out
// for the scratch's capacity (ensure_order_scratch came first); the sort looks at the key bits in
// use only.
int rti::sort_rays(rt_scene* s, const RayBatch& B, int key_bits, hipStream_t st, const uint32_t** order) {
    rt_scene::Query& qs = s->query;
    refresh_query_box(s);
    const QueryOrderPlan CP = query_order_plan(qs.qo_rays, QUERY_ORDER_SORTED, false);
    unsigned char* p = qs.qo_dev;
    unsigned long long* k_in = (unsigned long long*)p; p += CP.keys_bytes;
    unsigned long long* k_out = (unsigned long long*)p; p += CP.keys_bytes;
    uint32_t* v_in = (uint32_t*)p; p += CP.idx_bytes;
    uint32_t* v_out = (uint32_t*)p; p += CP.idx_bytes;
    HIPCHK(launch_ray_keys(B, qs.box, k_in, v_in, st));
    HIPCHK(ray_sort_pairs(p, qs.qo_temp, k_in, k_out, v_in, v_out, B.n, key_bits, st));
    *order = v_out;
    return RT_OK;
}

extern "C" {

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
    int r;
    if ((r = check_ray_inputs("rt_query", o->origin, o->dir, o->pixel)) != RT_OK) return r;
    const bool any = o->any_hit != 0;
    if (any ? !o->hit : !(o->t || o->inst || o->tri || o->uv || o->normal || o->hit || o->rays_out))
        return fail(RT_ERR_ARG, any ? "rt_query: an occlusion query writes `hit`" : "rt_query: no output requested");
    const size_t n = (size_t)o->n;
    rt_scene::Query& qs = s->query;
    if ((r = check_sorted_limit("rt_query", qs.order, o->n)) != RT_OK) return r;
    if (o->host && o->pixel && (r = check_host_pixels("rt_query", o->pixel, n, s->h.cam.W, s->h.cam.H)) != RT_OK) return r;
    if ((r = begin_side_entry(s, 1, false)) != RT_OK) return r;   // upload, frames in flight, current poses
    hipStream_t st = sstream(s);
    const bool counted = stats != nullptr;
    // the sorted mode's scratch, before anything of this call is in flight
    const QueryOrderPlan OP = query_order_plan(o->n, qs.order, counted);
    if (OP.sort && (r = ensure_order_scratch(s, o->n, "rt_query")) != RT_OK) return r;
    if (counted) { HIPCHK(hipMemsetAsync(s->d_stats, 0, STATS_N * sizeof(unsigned long long), st)); HIPCHK(hipEventRecord(s->ev[0], st)); }
    if (s->builds_bvh(o->use_bvh, o->rebuild_bvh) && (r = build_bvh(s, st)) != RT_OK) return r;
    if (counted) HIPCHK(hipEventRecord(s->ev[1], st));

    QueryParams Q{};
    Q.cam = s->h.d_cam; Q.n = o->n;
    Q.origin = o->origin; Q.dir = o->dir; Q.tmax = o->tmax; Q.pixel = o->pixel;
    Q.t = any ? nullptr : o->t; Q.inst = any ? nullptr : o->inst; Q.tri = any ? nullptr : o->tri;
    Q.uv = any ? nullptr : o->uv; Q.normal = any ? nullptr : o->normal;
    Q.hit = o->hit; Q.rays_out = o->rays_out;
    Q.stats = counted ? s->d_stats : nullptr;
    // host pointers: the batch staged (inputs, then outputs) and these fields pointed at its device copy
    BatchPart parts[] = {in_part(Q.origin, 12 * n), in_part(Q.dir, 12 * n), in_part(Q.tmax, 4 * n), in_part(Q.pixel, 8 * n),
                         out_part(Q.t, 4 * n), out_part(Q.inst, 4 * n), out_part(Q.tri, 4 * n), out_part(Q.uv, 8 * n),
                         out_part(Q.normal, 12 * n), out_part(Q.hit, n), out_part(Q.rays_out, 24 * n)};
    if (o->host && (r = stage_inputs(qs.stage, parts, std::size(parts), "rt_query", o->n, st)) != RT_OK) return r;
    CallerView cv = caller_ray_view(s, o->use_bvh != 0);          // a caller's origin is anywhere
    SceneView& S = cv.S;
    Q.zcut_scene = cv.zcut_scene; Q.any_margin = cv.any_margin;
    int form = -1;                                             // RT_QUERY_FORM (measurements): small / persistent
    if (const char* e = getenv("RT_QUERY_FORM")) form = !strcmp(e, "small") ? 0 : !strcmp(e, "persistent") ? 1 : -1;
    const QueryVariant V = choose_query_variant(o->n, S, any, counted, s->n_cu, form, OP.sort);
    if (!V.fn)
        return fail(RT_ERR_STATE, "no query kernel <" + std::to_string(V.tree) + ", " + std::to_string((int)V.lds) + ", " +
                                      std::to_string((int)V.any_hit) + ", " + std::to_string((int)V.counted) + ", " +
                                      std::to_string((int)V.ordered) + ">");
    bool trace = true;
    if (OP.sort) {
        // key, sort, trace: stream-ordered, no host synchronisation between them
        if ((r = sort_rays(s, RayBatch{Q.cam, Q.n, Q.origin, Q.dir, Q.pixel}, OP.key_bits, st, &Q.order)) != RT_OK) return r;
        // RT_QUERY_SORT_ONLY (measurements, tools/query_bench.py): stop after the sort; no output is written
        if (const char* e = getenv("RT_QUERY_SORT_ONLY")) trace = atoi(e) == 0;
    }
    if (trace) HIPCHK(launch_query_kernel(V, Q, S, st));
    HIPCHK(hipGetLastError());
    qs.last = V; qs.has_last = true;                           // rt_query_last
    qs.last_sorted = OP.sort; qs.last_n = o->n; qs.last_order = Q.order;
    if (counted) HIPCHK(hipEventRecord(s->ev[2], st));
    if (o->host && (r = fetch_outputs(qs.stage, st)) != RT_OK) return r;
    if ((r = end_frame(s, st)) != RT_OK) return r;
    HIPCHK(hipStreamSynchronize(st));
    if (o->host) copy_outputs(qs.stage, parts, std::size(parts));
    return counted ? read_frame_stats(s, stats) : RT_OK;
}

int rt_query_set_order(rt_scene* s, int mode) {
    CHECK_SCENE(s);
    if (mode != RT_QUERY_ORDER_CALLER && mode != RT_QUERY_ORDER_SORTED)
        return fail(RT_ERR_ARG, "query order: RT_QUERY_ORDER_CALLER or RT_QUERY_ORDER_SORTED");
    s->query.order = mode;
    return RT_OK;
}

int rt_query_last(const rt_scene* s, int32_t* out8, float* bounds6, uint32_t* order, int64_t order_cap) {
    CHECK_FINISHED(s);
    const rt_scene::Query& qs = s->query;
    if (!qs.has_last) return fail(RT_ERR_STATE, "no rt_query yet");
    const QueryVariant& k = qs.last;
    const bool sorted = qs.last_sorted;
    if (order && sorted && order_cap < qs.last_n) return fail(RT_ERR_ARG, "rt_query_last: order_cap is below the batch's n");
    if (out8) {
        const int32_t v[8] = {k.tree, (int32_t)k.lds, (int32_t)k.any_hit, (int32_t)k.counted, (int32_t)k.ordered,
                              (int32_t)k.persistent, k.blocks, (int32_t)sorted};
        std::copy(v, v + 8, out8);
    }
    if (bounds6) {
        const rtk::KeyBox b = sorted ? qs.box : rtk::KeyBox{v3(0, 0, 0), v3(0, 0, 0)};
        const float v[6] = {b.mn.x, b.mn.y, b.mn.z, b.mx.x, b.mx.y, b.mx.z};
        std::copy(v, v + 6, bounds6);
    }
    if (order && sorted) {
        if (!qs.last_order) return fail(RT_ERR_STATE, "rt_query_last: the last order's buffer was released");
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(hipMemcpy(order, qs.last_order, (size_t)qs.last_n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return RT_OK;
}

}  // extern "C"
