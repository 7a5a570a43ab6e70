// rt_kernels.hip — gfx950 kernels of the ray-tracing core and their launch layer (rt_device.h).
// Device code only: the scene object, the frame slots and the C ABI are rt_runtime.cpp and
// the host files beside it (rt_build, rt_accumulate, rt_occlusion, rt_query, rt_hooks, ...).
//
// Hot path (BASELINE.json north_star): rtracer::gpu::update_scene
// (src/raytracer.cu:102-120) = per-frame BVH build + the per-pixel `trace`
// megakernel running renv::gpu::propagate_ray (src/rayenv/scene.cu:92-188).
//
// MI355X design:
//  * bvh_build_kernel: ONE workgroup of 1024 threads per frame builds the reference's Morton
//    BVH (boxes -> 64-bit z-order keys -> an LDS rank sort equal to thrust's stable
//    sort_by_key -> pairwise level merges, bvh.cu:11-91) in the reference's heap layout (child
//    pairs as three float4) and, from the same sorted leaves, an ordered LBVH for the fast
//    kernels (64-B records, leaves met in the heap's DFS order).  Above 8192 padded leaves the
//    grid-wide build of rt_bvh_large.hip takes over.
//  * sky_kernel: a pre-pass over pixel groups (8 pixels x 8 samples at 8 spp): a group none of
//    whose primary rays enters the tree's root is written here (zeros, -1 hit ids) and the
//    live groups go onto per-queue lists (and, hist = 2, the previous frame's heavy groups onto
//    a heavy list run first).
//  * trace_kernel: persistent 1024-thread blocks, one per CU, with the scene (ordered tree,
//    instances, shading records) staged in LDS.  A wave takes live groups from work queues;
//    lane = (pixel, sample).  Each lane runs propagate_ray (scene.cu:92-188) as a state machine
//    whose only wave-collective step is the closest-hit query: a packet traversal with the node
//    index wave-uniform (SGPR), 16-B broadcast LDS record reads, a filtered slab test with the
//    exact reference test as fallback, and ballots for descend / push / pop.  Integrator state
//    the traversal does not read is parked in LDS during the query.  Every filter and pruning
//    is exact: hit ids equal the reference's single-ray semantics and
//    radiance its float32 operations.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rt_accum.h"
#include "rt_adapt.h"
#include "rt_bvh.h"
#include "rt_device.h"
#include "rt_math.h"
#include "rt_scene.h"

using namespace rtm;
using namespace rtb;
using namespace rtd;
using rt::DCamera;
using rt::DInst;
using rt::DLight;
using rt::DMat;
using rt::DMesh;
using rt::DNode;
using rt::DTri;

namespace {

// (launch geometry, tuning macros and the kernel argument structs the host shares: rt_device.h;
// the LDS layout -- LDS limits, lds_bytes, parked fields, PROF slots -- and the MODE bits: rt_plan.h)
// (work counter layout: WORK_INTS, rt_device.h)
constexpr int WORK_HEAVY_LEN = 16 * (2 * NQ + 1);

enum : int { F_NORMAL = 0, F_REFLECT = 1, F_REFRACT = 2 };
enum : int { PH_NORMAL = 1, PH_SHADOW = 2, PH_DONE = 3 };

__device__ __forceinline__ float max_std(float a, float b) { return (a < b) ? b : a; }   // std::max
// powf of the reference (nvcc pow(float,float)); evaluated in double and rounded:
// agrees with glibc powf except for 1-ulp cases.  pow_pos (rt_math.h)
// answers x > 0 with |y ln x| <= 700 in about 40 double operations; the rest (x <= 0, inf,
// nan, overflow and underflow far outside float range) take the library's double pow.
__device__ __forceinline__ float pow_lib(float x, float y) { return (float)pow((double)x, (double)y); }
__device__ __noinline__ float pow_ref(float x, float y) {   // rare: kept out of line
    float o;
    return pow_pos(x, y, o) ? o : pow_lib(x, y);
}
// pow_ref with the C99 / IEEE special cases that dominate the shading calls answered
// inline (every powf and pow agree on them bit for bit, F.9.4.4): pow(x, +-0) = 1 (the
// materials without "alpha"), pow(1, y) = 1, pow(+-0, y > 0) = +0 except -0 for odd integer
// y (lights behind the surface give max(dot, 0) = +-0).  A wave skips the double-precision
// call when none of its lanes needs it.
__device__ __forceinline__ float pow_fast(float x, float y) {
    if (y == 0.0f || x == 1.0f) return 1.0f;
    if (x == 0.0f && y > 0.0f) {
        const bool odd = y == rintf(y) && rintf(0.5f * y) != 0.5f * y;
        return (odd && signbit(x)) ? -0.0f : 0.0f;
    }
    return pow_ref(x, y);
}



// UDiv (rt_device.h): unsigned division by a launch constant through host-computed magic numbers
__device__ __forceinline__ unsigned udiv(unsigned n, const UDiv& D) {
    if (D.d <= 1) return n;
    const unsigned t = __umulhi(n, D.m);
    return (t + ((n - t) >> 1)) >> D.s;
}

// Parts of a DTri (rt_scene.h): the plane filter's 32-B head and the rest of the test.
struct TriHot { V3 pn, a; float b_x, b_y; };
struct TriRest { V3 b, c; float area, inv_area; };
static_assert(sizeof(TriHot) == 32 && offsetof(DTri, b) == 24 && offsetof(DTri, inv_area) == 52, "DTri layout");

// Wave-uniform read-only records in global memory are read through the
// constant address space so that uniform indices compile to scalar (SMEM) loads.
template <class T> __device__ __forceinline__ T ldc(const T* p, int i) {
    static_assert(sizeof(T) % 4 == 0, "4-byte granular records");
    T r;
    uint32_t* d = reinterpret_cast<uint32_t*>(&r);
#if defined(__HIP_DEVICE_COMPILE__)
    const __attribute__((address_space(4))) uint32_t* s = (const __attribute__((address_space(4))) uint32_t*)(p + i);
#else
    const uint32_t* s = reinterpret_cast<const uint32_t*>(p + i);
#endif
#pragma unroll
    for (int w = 0; w < (int)(sizeof(T) / 4); w++) d[w] = s[w];
    return r;
}

__device__ __forceinline__ TriHot ld_hot(const DTri* T, int t) { return ldc(reinterpret_cast<const TriHot*>(T + t), 0); }
__device__ __forceinline__ TriRest ld_rest(const DTri* T, int t) {
    return ldc(reinterpret_cast<const TriRest*>(reinterpret_cast<const char*>(T + t) + 24), 0);
}

// BVH nodes and instance records as the trace kernel reads them: from LDS (staged
// once per persistent block) or, for scenes too large for LDS, from global memory.
// Nodes are stored by child pair: pair k holds heap nodes 2k (.x lanes) and 2k+1 (.y
// lanes) as three float4 = (mnx, mnx' , mny, mny'), (mnz, mnz', mxx, mxx'),
// (mxy, mxy', mxz, mxz'), so one pair test is three 16-B broadcast reads and packed
// (v_pk_*) slab arithmetic.  Pair 0 = (unused node 0, root).  Degenerate boxes are
// stored as min=+inf, max=-inf.
struct BvhRefs {
    const float4* fnode;    // ordered LBVH records (fast kernel): [4 (n_real - 1)]
    const float4* pair;     // [3n]
    const int* leaf;        // [n]  instance of leaf node n+i (bvh.cu ordering[])
    const float4* inst;     // [n_inst] (px, py, pz, mesh | 0x80000000 if the pose is not identity)
    // shading-side records (materials, lights, triangles, meshes): the scene's arrays, or
    // their LDS copies in M_SHADE kernels (hit normal, lighting and frame transitions read
    // them per lane after every query)
    const DMat* mats;
    const DLight* lights;
    const DTri* tris;
    const DMesh* meshes;
};

// One child box's slab interval [lo, hi] against a ray through its reciprocals (ray_inv):
// fma(m - o, 1/d, -+bias) per face, the bias carrying the zero-direction skip (ray_inv).
__device__ __forceinline__ void slab(const Ray& r, const RayInv& ri, float mnx, float mny, float mnz, float mxx,
                                     float mxy, float mxz, float& lo, float& hi) {
    const float qx0 = fmaf(mnx - r.o.x, ri.ix, -ri.bx), qx1 = fmaf(mxx - r.o.x, ri.ix, ri.bx);
    const float qy0 = fmaf(mny - r.o.y, ri.iy, -ri.by), qy1 = fmaf(mxy - r.o.y, ri.iy, ri.by);
    const float qz0 = fmaf(mnz - r.o.z, ri.iz, -ri.bz), qz1 = fmaf(mxz - r.o.z, ri.iz, ri.bz);
    lo = fmaxf(fmaxf(fminf(qx0, qx1), fminf(qy0, qy1)), fminf(qz0, qz1));
    hi = fminf(fminf(fmaxf(qx0, qx1), fmaxf(qy0, qy1)), fmaxf(qz0, qz1));
}

// BoundingBox::intersects (bounding_box.cu:62-104) for both children of pair k.
// Filtered like box_hit_f (rt_math.h), with the bound taken from the slab results
// themselves: every quotient q' = fl(e * r'), r' = v_rcp_f32(d) (ray_inv), is within
// 4.02u |q'| of the reference's fl(e / d), min and max keep a relative bound (|max a' -
// max a| <= 4.05u max(|a|, |a'|)), so |lo' - lo| <= 8.2u |lo'| and the same for hi; the
// test uses 16u plus an absolute floor.  Zero direction components are skipped through
// the RayInv bias (see ray_inv); rays with a non-finite reciprocal (ri.exact) and
// boxes near a tie take the exact reference test.
// tlo (pruning) is a lower bound of the exact entry distance, -inf if undecided.
__device__ __forceinline__ void pair_hit_at(const float4* rec, const Ray& r, const RayInv& ri, bool active,
                                            bool& h0, bool& h1, float& t0, float& t1) {
    const float4 A = rec[0], B = rec[1], C = rec[2];
    const bool nd0 = A.x <= B.z, nd1 = A.y <= B.w;            // nondegenerate (bounding_box.cu:63-65)
    float lo0, hi0, lo1, hi1;
    slab(r, ri, A.x, A.z, B.x, B.z, C.x, C.z, lo0, hi0);
    slab(r, ri, A.y, A.w, B.y, B.w, C.y, C.w, lo1, hi1);
    // Certain outcomes (the exact reference result known): with el, eh the error margins of
    // lo, hi, c = lo + el and a = hi - eh bound the reference's tmin from above and its tmax
    // from below, so max(c, 1e-5) <= a is certainly a hit; with d = lo - el, b = hi + eh,
    // max(d, 1e-5) > b is certainly a miss (bounding_box.cu:98: tmin > tmax || tmax < 1e-5).
    // For filtered rays lo and hi are finite (ray_inv sends a direction without a nonzero
    // component to the exact test), so the max forms equal the pairs of comparisons.
    // Lanes in between run the exact reference test; one uniform branch for both children.
    const float el0 = fmaf(fabsf(lo0), FILT_BOX, FILT_ABS), el1 = fmaf(fabsf(lo1), FILT_BOX, FILT_ABS);
    const float eh0 = fmaf(fabsf(hi0), FILT_BOX, FILT_ABS), eh1 = fmaf(fabsf(hi1), FILT_BOX, FILT_ABS);
    const float d0 = lo0 - el0, d1 = lo1 - el1;
    const bool fx = active && !ri.exact;
    const bool c0 = fx && nd0 && fmaxf(lo0 + el0, THRESH) <= hi0 - eh0;
    const bool c1 = fx && nd1 && fmaxf(lo1 + el1, THRESH) <= hi1 - eh1;
    const bool m0 = !nd0 || (fx && fmaxf(d0, THRESH) > hi0 + eh0);
    const bool m1 = !nd1 || (fx && fmaxf(d1, THRESH) > hi1 + eh1);
    h0 = c0; h1 = c1;
    t0 = c0 ? d0 : -INFINITY;
    t1 = c1 ? d1 : -INFINITY;
    const bool x0 = active && !m0 && !c0, x1 = active && !m1 && !c1;
    if (__builtin_expect(__ballot(x0 || x1) != 0, 0)) {
        if (x0) h0 = box_hit(v3(A.x, A.z, B.x), v3(B.z, C.x, C.z), r);
        if (x1) h1 = box_hit(v3(A.y, A.w, B.y), v3(B.w, C.y, C.w), r);
    }
}
// 0/1 in an SGPR from a wave mask, opaque to the optimizer (a boolean taken from a ballot is
// otherwise rebuilt through a VGPR: v_cndmask + v_cmp per use)
__device__ __forceinline__ unsigned any_lane(unsigned long long m) {
    unsigned h;
    asm("s_cmp_lg_u64 %1, 0\n\ts_cselect_b32 %0, 1, 0" : "=s"(h) : "s"(m) : "scc");
    return h;
}
// pair_hit_at for the fast traversal step, with each child's result as one float: the entry
// lower bound (lo - el, or -inf after the exact test) for a hit, NaN for a miss.  Every record
// of the ordered tree is a proper finite box (the host leaves a frame with a degenerate or
// non-finite real box to the heap kernels: ordered_tree_shape), so there is no per-child
// degenerate test; a ray that needs the exact test everywhere (ri.exact) enters with NaN
// reciprocals (closest_hit), so both its slab results are NaN and both outcome tests are
// false: it takes the exact test with no filtered-ray mask.  ta/tb carry no activity mask: an
// inactive lane's cut is NaN, so t <= cut is false for it.
__device__ __forceinline__ void pair_hit_tt2(const float4* rec, const Ray& r, const RayInv& ri, bool active,
                                             float& ta, float& tb) {
    const float4 A = rec[0], B = rec[1], C = rec[2];
    float lo0, hi0, lo1, hi1;
    slab(r, ri, A.x, A.z, B.x, B.z, C.x, C.z, lo0, hi0);
    slab(r, ri, A.y, A.w, B.y, B.w, C.y, C.w, lo1, hi1);
    const float el0 = fmaf(fabsf(lo0), FILT_BOX, FILT_ABS), eh0 = fmaf(fabsf(hi0), FILT_BOX, FILT_ABS);
    const float el1 = fmaf(fabsf(lo1), FILT_BOX, FILT_ABS), eh1 = fmaf(fabsf(hi1), FILT_BOX, FILT_ABS);
    const float d0 = lo0 - el0, d1 = lo1 - el1;
    const bool hc0 = fmaxf(lo0 + el0, THRESH) <= hi0 - eh0, hc1 = fmaxf(lo1 + el1, THRESH) <= hi1 - eh1;
    const bool mc0 = fmaxf(d0, THRESH) > hi0 + eh0, mc1 = fmaxf(d1, THRESH) > hi1 + eh1;
    const float QNAN = __builtin_nanf("");
    ta = hc0 ? d0 : QNAN;
    tb = hc1 ? d1 : QNAN;
    const bool k0 = hc0 || mc0, k1 = hc1 || mc1;               // outcome certain
    if (__builtin_expect(any_lane(__ballot(active && !(k0 && k1))), 0)) {
        if (active && !k0) ta = box_hit(v3(A.x, A.z, B.x), v3(B.z, C.x, C.z), r) ? -INFINITY : QNAN;
        if (active && !k1) tb = box_hit(v3(A.y, A.w, B.y), v3(B.w, C.y, C.w), r) ? -INFINITY : QNAN;
    }
}
// pair_hit_tt2 with the lane's activity as its cut ct (active: ct == ct) and the outcome tests
// issued as four v_cmp into SGPR masks, combined on the scalar unit: the compiler's form of
// `__ballot(active && !(k0 && k1))` rebuilt the combined mask through a VGPR (v_cndmask 0/1 +
// v_cmp_ne) before the branch, two VALU and a dependent hand-off per traversal step.
#ifndef RT_ASM_OUTCOME
#define RT_ASM_OUTCOME 1
#endif
__device__ __forceinline__ void pair_hit_tt2c(const float4* rec, const Ray& r, const RayInv& ri, float ct,
                                              float& ta, float& tb) {
#if RT_ASM_OUTCOME
    const float4 A = rec[0], B = rec[1], C = rec[2];
    float lo0, hi0, lo1, hi1;
    slab(r, ri, A.x, A.z, B.x, B.z, C.x, C.z, lo0, hi0);
    slab(r, ri, A.y, A.w, B.y, B.w, C.y, C.w, lo1, hi1);
    const float el0 = fmaf(fabsf(lo0), FILT_BOX, FILT_ABS), eh0 = fmaf(fabsf(hi0), FILT_BOX, FILT_ABS);
    const float el1 = fmaf(fabsf(lo1), FILT_BOX, FILT_ABS), eh1 = fmaf(fabsf(hi1), FILT_BOX, FILT_ABS);
    const float d0 = lo0 - el0, d1 = lo1 - el1;
    // certain hit: a <= b; certain miss: c > e (pair_hit_at)
    const float a0 = fmaxf(lo0 + el0, THRESH), b0 = hi0 - eh0, a1 = fmaxf(lo1 + el1, THRESH), b1 = hi1 - eh1;
    const float c0 = fmaxf(d0, THRESH), e0 = hi0 + eh0, c1 = fmaxf(d1, THRESH), e1 = hi1 + eh1;
    const float QNAN = __builtin_nanf("");
    unsigned long long h0, h1, m0, m1;
    asm("v_cmp_le_f32 %[h0], %[a0], %[b0]\n\t"
        "v_cmp_le_f32 %[h1], %[a1], %[b1]\n\t"
        "v_cmp_gt_f32 %[m0], %[c0], %[e0]\n\t"
        "v_cmp_gt_f32 %[m1], %[c1], %[e1]\n\t"
        "v_cndmask_b32 %[ta], %[nan], %[d0], %[h0]\n\t"
        "v_cndmask_b32 %[tb], %[nan], %[d1], %[h1]\n\t"
        "s_or_b64 %[m0], %[m0], %[h0]\n\t"                  // outcome of child A certain
        "s_or_b64 %[m1], %[m1], %[h1]\n\t"                  // ... of child B
        "s_and_b64 %[m0], %[m0], %[m1]\n\t"
        "v_cmp_o_f32 %[m1], %[ct], %[ct]\n\t"               // active lanes
        "s_andn2_b64 %[m0], %[m1], %[m0]"                   // active, some outcome uncertain
        : [h0] "=&s"(h0), [h1] "=&s"(h1), [m0] "=&s"(m0), [m1] "=&s"(m1), [ta] "=&v"(ta), [tb] "=&v"(tb)
        : [a0] "v"(a0), [b0] "v"(b0), [a1] "v"(a1), [b1] "v"(b1), [c0] "v"(c0), [e0] "v"(e0), [c1] "v"(c1),
          [e1] "v"(e1), [d0] "v"(d0), [d1] "v"(d1), [nan] "v"(QNAN), [ct] "v"(ct)
        : "scc");
    if (__builtin_expect(m0 != 0, 0)) {
        const bool active = ct == ct;
        const bool k0 = a0 <= b0 || c0 > e0, k1 = a1 <= b1 || c1 > e1;
        if (active && !k0) ta = box_hit(v3(A.x, A.z, B.x), v3(B.z, C.x, C.z), r) ? -INFINITY : QNAN;
        if (active && !k1) tb = box_hit(v3(A.y, A.w, B.y), v3(B.w, C.y, C.w), r) ? -INFINITY : QNAN;
    }
#else
    pair_hit_tt2(rec, r, ri, ct == ct, ta, tb);
#endif
}
__device__ __forceinline__ void pair_hit(const float4* np, int k, const Ray& r, const RayInv& ri, bool active,
                                         bool& h0, bool& h1, float& t0, float& t1) {
    pair_hit_at(np + 3 * k, r, ri, active, h0, h1, t0, t1);
}

struct Best { float time; int inst, tri; float u, v; };     // closest accepted triangle so far
// Per-lane work counters (rays/nodes/leaves/triangle tests, the reference's units) plus
// wave-level step counts for the profiling experiment (query iterations, child-pair
// steps, leaf visits, triangle-loop iterations -- SIMD work regardless of active lanes).
struct WaveCounters { unsigned long long rays, nodes, leaves, tris, wq, wpair, wleaf, wtri, cyc_q, cyc_leaf, cyc_all, cyc_sample, cyc_post, wbary, lbary, live,
                      cyc_light, cyc_normal, cyc_park,      // PROF: light step, hit normal, parking
                      hint,                                 // occluder hints: the wave's three counts (HINT_FIELD_BITS each)
                      nf;                                   // near-first: the wave's three counts (NF_FIELD_BITS each)
                      unsigned long long* pc; };            // PROF: this wave's occupancy counters in LDS

__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }   // value known wave-uniform
__device__ __forceinline__ Pose inst_pose(const SceneView& S, const BvhRefs& bv, int ti, int& mesh) {
    const float4 I = bv.inst[ti];
    const int w = __float_as_int(I.w);
    mesh = w & 0x7fffffff;
    if (w < 0) return ldc(S.insts, ti).pose;                  // general pose (precomputed quaternions)
    Pose e;
    e.p = v3(I.x, I.y, I.z); e.identity = 1;
    return e;
}

// Closest hit against one instance: renv::gpu::cast_local (scene.cu:27-40) ->
// Hitable::hit (hitable.cu:29-38) -> Trimesh::hit_local (trimesh.cu:11-19) with a
// wave-uniform instance; times are rescaled here exactly as in the reference
// (later comparisons depend on them); the normal is formed after traversal.
// With identity rotations everywhere (S.ident_all), the direction half of cast_local's
// two pose changes depends on the ray only: it is computed once per query by the same
// operations (qrot_identity, len, the Ray ctor's normalisation), so every leaf sees
// the same bits it would compute itself; only the origin chain is per leaf.
// `inv` (axis-plane triangles, axis_plane_t): fl(1/mrd_a), NaN where |mrd_a| < 1e-5.
struct DirPre { V3 mrd, inv; float scale, dir_len; };
__device__ __forceinline__ float axis_inv(float d) { return fabsf(d) < THRESH ? __builtin_nanf("") : rcp_cr(d); }
// keep_arm: passes an arm's operand through an empty asm statement, so that the arm stays an arm.
// Both arms of a vote are plain arithmetic, which the compiler otherwise hoists out of the branch
// (and out of the traversal loop) and runs one after the other with selects on the vote -- the
// generic chain on every query again.
__device__ __forceinline__ V3 keep_arm(V3 v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z)); return v; }
__device__ __forceinline__ float keep_arm(float s) { asm volatile("" : "+v"(s)); return s; }
// A traced direction is unit to a few ulps and every stage maps unit to unit, so the four
// length / reciprocal pairs take their closed forms (rt_math.h, unit_len_rcp: the same bits).
// One wave vote on the chain's head (unit_head): when a lane with a query (`active`) fails it,
// the whole wave runs the generic chain.
template <bool AXIS = false>
__device__ __forceinline__ DirPre dir_pre(V3 d, bool active) {
    DirPre p;
    if (!__ballot(active && !unit_head(dot(d, d)))) {
        d = keep_arm(d);
        const V3 lrd = normalized_unit(qrot_identity_unit(d), p.dir_len);
        p.mrd = normalized_unit(qrot_identity_unit(lrd), p.scale);
    } else {
        d = keep_arm(d);
        const V3 ld = qrot_identity(d);                      // Entity::vec_to_local, identity pose
        p.dir_len = len(ld);
        const V3 lrd = normalized(ld);                       // Ray ctor (geometry.h:216)
        const V3 md = qrot_identity(lrd);                    // HitHandle::get_local_ray, identity mesh pose
        p.scale = len(md);
        p.mrd = normalized(md);
    }
    if (AXIS) p.inv = v3(axis_inv(p.mrd.x), axis_inv(p.mrd.y), axis_inv(p.mrd.z));
    return p;
}

// The shading steps' chains (trace_sample: the hit's unit normal, the light step, the reflection
// step) in the same manner: one vote per chain of the lanes in that step, on the chain's first
// squared length(s); a failing lane sends the wave to the generic chain, unchanged.
// (len, 1 / len) of a vector from its squared length s
__device__ __forceinline__ void len_rcp_vote(float s, float& l, float& r) {
    if (!__ballot(!unit_head(s))) {
        unit_len_rcp(keep_arm(s), l, r);
    } else {
        l = sqrt_cr(keep_arm(s));
        r = rcp_cr(l);
    }
}
// normalized(v)
__device__ __forceinline__ V3 normalized_vote(V3 v) {
    const float s = dot(v, v);
    if (!__ballot(!unit_head(s))) {
        float l, r;
        unit_len_rcp(keep_arm(s), l, r);
        return r * v;
    }
    const float l = sqrt_cr(keep_arm(s));
    if (l > THRESH) return rcp_cr(l) * v;
    return v3(0.0f, 0.0f, 0.0f);
}
// reflect(dir, nrm): both heads vote, the mirrored direction's length follows them (rt_math.h)
__device__ __forceinline__ V3 reflect_vote(V3 dir, V3 nrm) {
    if (!__ballot(!(unit_head(dot(dir, dir)) && unit_head(dot(nrm, nrm)))))
        return reflect_unit(keep_arm(dir), keep_arm(nrm));
    return reflect(keep_arm(dir), keep_arm(nrm));
}

// An axis-plane triangle's step for the wave, on the record's axis AX (cast_local dispatches on the
// wave-uniform axis bits, so no component is picked by a select): the exact plane time tt from the
// per-query reciprocal (axis_plane_t) and its window test, then, where some lane passed (`plane`)
// and the record allows it, the exact in-plane reject (TriAx); `cand`: some lane is left.
// The wave tests stay `__ballot(..) != 0`: here the compiler branches on the compare masks
// themselves, while any_lane() made it rebuild each mask through a VGPR first (measured slower,
// DESIGN.md §3.2 item 35).
template <int AX>
__device__ __forceinline__ void axis_step(const TriAx& x, const Ray& mr, V3 inv, float lo, float t_best, float& tt,
                                          bool& pass, bool& plane, bool& cand) {
    pass = axis_plane_pass<AX>(x, mr.o, inv, lo, t_best, tt);
    plane = cand = __ballot(pass) != 0;
    if (plane && (x.code & 8)) {
        pass = pass && !axis_inplane_reject<AX>(x, mr, tt);
        cand = __ballot(pass) != 0;
    }
}

// t_lo: lower bound of any acceptable local time (-inf if none): the leaf box's entry
// distance minus the pruning slack M (closest_hit).  A triangle whose plane crossing is
// certainly below it lies outside the box, so its inside test is skipped.
// AXIS: the axis-plane triangle path (S.tri_ax, pre.inv set; identity rotations only).
// NEAR, `nf` (wave-uniform): a leaf visit of a near-first walk (closest_hit).  While the
// lane has accepted nothing in this leaf, the plane tests compare against the entry best widened by
// NF_W (nf_pass_bound, rt_math.h: `t_best` holds that comparand; the entry best itself stays in
// b.time), a triangle is still accepted only below the entry best, and one that passes the inside
// test within NF_W of it (nf_near_tie) sets `flag`: the result could depend on the order in which
// the leaves were met.  After the first accept t_best is the accepted time, as without NEAR.
template <bool STATS, bool AXIS = false, bool PROF = false, bool NEAR = false>
__device__ __forceinline__ bool cast_local(const SceneView& S, const BvhRefs& bv, int ti, const Ray& r, Best& b,
                                           const DirPre& pre, WaveCounters& wc, float t_lo, bool nf, int& flag) {
    int mesh_id;
    const Pose ip = inst_pose(S, bv, ti, mesh_id);
    mesh_id = uni(mesh_id);
    const DMesh mesh = ldc(S.meshes, mesh_id);
    float dir_len, scale;
    Ray mr;
    // AXIS kernels run only with identity rotations everywhere (choose_trace_variant checks it), so
    // the general-pose arm is not compiled into them.  Elsewhere its direction chain is plain
    // arithmetic on the query's ray, which the compiler would hoist out of the leaf and traversal
    // loops and run on every query whatever S.ident_all says: keep_arm holds it in its arm.
    if (AXIS || S.ident_all) {
        dir_len = pre.dir_len; scale = pre.scale;
        mr.o = qrot_identity(qrot_identity(r.o - ip.p) - mesh.pose.p);
        mr.d = pre.mrd;
    } else {
        V3 ld = vec_to_local(ip, keep_arm(r.d));
        dir_len = len(ld);
        Ray lr = make_ray(point_to_local(ip, r.o), ld);
        V3 md = vec_to_local(mesh.pose, lr.d);               // HitHandle::get_local_ray
        scale = len(md);
        mr = make_ray(point_to_local(mesh.pose, lr.o), md);
    }
    int best = -1;
    float bu = 0.0f, bv_ = 0.0f, t_best = b.time;
    if (NEAR && nf) t_best = nf_pass_bound(b.time);
    // the accept of a triangle that passed the inside test at `time` (< t_best)
    auto accept = [&](float time) {
        if (NEAR && nf && best < 0) {
            if (nf_near_tie(time, b.time)) flag = 1;
            return time < b.time;
        }
        return true;
    };
    if (AXIS) {
        // Axis-plane path (fast kernel, identity rotations): exact plane time from the
        // per-query reciprocal (axis_plane_t), then the exact in-plane reject (TriAx);
        // general triangles take the filtered test below.  Same decisions, same order.
        // One structured body per triangle: every path reaches the one latch, the twin skip is a
        // scalar step there, and the accepted state (t_best, best, bu, bv_) is the loop's only
        // vector state -- written in place by the accept and by nothing else.  (With `continue`s
        // and `t++` inside a branch the compiler carried that state and the accept's temporaries
        // through a second register set: 14 v_mov on an iteration that tests a plane and leaves.)
        const float lo = fmaxf(THRESH, t_lo);
        const int t_end = mesh.tri_begin + mesh.tri_count;
        int t = mesh.tri_begin;
        while (t < t_end) {
            const TriAx x = ldc(S.tri_ax, t);
            const int ax = x.code & 3;
            int step = 1;
            float tt;                                         // candidate lanes: the exact plane time
            bool pass;
            bool cand;                                        // some lane takes the inside test
            if (PROF) wc.wtri++;
            if (ax == 3) {                                    // general triangle: filtered plane test
                const TriHot h = ld_hot(S.tris, t);
                float denom, num;
                pass = tri_plane_f(h.a, h.pn, mr, t_best, t_lo, denom, num);
                cand = __ballot(pass) != 0;
                if (cand) pass = pass && tri_time_f(t_best, denom, num, tt);
            } else {
                bool plane;                                   // some lane passed the plane time
                if (ax == 0) axis_step<0>(x, mr, pre.inv, lo, t_best, tt, pass, plane, cand);
                else if (ax == 1) axis_step<1>(x, mr, pre.inv, lo, t_best, tt, pass, plane, cand);
                else axis_step<2>(x, mr, pre.inv, lo, t_best, tt, pass, plane, cand);
                if (!plane) step += (x.code >> 2) & 1;        // same plane, same t, same best: the twin is rejected too
                if (PROF && cand) { wc.wbary++; wc.lbary += __popcll(__ballot(pass)); }
            }
            if (cand) {                                       // the one inside test, for both kinds
                const TriHot h = ld_hot(S.tris, t);
                const TriRest q = ld_rest(S.tris, t);
                if (pass) {
                    float time, u, v;
                    if (tri_inside_t(h.a, q.b, q.c, q.area, q.inv_area, mr, tt, time, u, v) && accept(time)) {
                        t_best = time; best = t; bu = u; bv_ = v;
                    }
                }
            }
            t += step;
        }
    } else
    // The plane filter needs only the 32-B head (pn, a) of each record (one batch of
    // scalar loads); the rest is read only for triangles that pass it.
    for (int t = mesh.tri_begin; t < mesh.tri_begin + mesh.tri_count; t++) {
        const TriHot h = ld_hot(S.tris, t);
        float denom, num, time, u, v;
        const bool pass = tri_plane_f(h.a, h.pn, mr, t_best, t_lo, denom, num);
        if (STATS) {
            const unsigned long long pm = __ballot(pass);
            wc.wbary += pm != 0;
            wc.lbary += __popcll(pm);
        }
        if (!pass) continue;
        const TriRest q = ld_rest(S.tris, t);
        if (tri_inside_f(h.a, q.b, q.c, q.area, q.inv_area, mr, t_best, denom, num, time, u, v) && accept(time)) {
            t_best = time; best = t; bu = u; bv_ = v;
        }
    }
    if (best < 0) return false;
    b.time = (t_best * scale) * dir_len;                      // fix_isect, then cast_local
    b.inst = ti; b.tri = best; b.u = bu; b.v = bv_;
    return true;
}
template <bool STATS, bool AXIS = false, bool PROF = false>
__device__ __forceinline__ bool cast_local(const SceneView& S, const BvhRefs& bv, int ti, const Ray& r, Best& b,
                                           const DirPre& pre, WaveCounters& wc, float t_lo) {
    int flag = 0;
    return cast_local<STATS, AXIS, PROF, false>(S, bv, ti, r, b, pre, wc, t_lo, false, flag);
}

// World-space normal of the accepted hit (trimesh.cu:58-65, hitable.cu:20-23, scene.cu:35-37).
__device__ __forceinline__ V3 hit_normal(const SceneView& S, const BvhRefs& bv, const Best& b, int& mat) {
    int mesh_id;
    const Pose ip = inst_pose(S, bv, b.inst, mesh_id);
    const Pose mp = bv.meshes[mesh_id].pose;
    const DTri& T = bv.tris[b.tri];
    mat = T.mat;
    float b0 = 1.0f - b.u - b.v;
    V3 ni = (b0 * T.n0 + b.u * T.n1) + b.v * T.n2;
    // Equal unit vertex normals (every cube face) under identity poses: four unit-length stages
    // (unit_len_rcp).  One vote of the lanes that hit, on the chain's head: an interpolated normal
    // off unit length, or a general pose, sends the wave to the generic chain.
    if (!__ballot(!(mp.identity && ip.identity && unit_head(dot(ni, ni))))) {
        float l;
        const V3 un = normalized_unit(qrot_identity_unit(normalized_unit(ni, l)), l);
        return qrot_identity_unit(un);
    }
    ni = keep_arm(ni);
    V3 n = normalized(ni);
    n = normalized(vec_from_local(mp, n));
    return vec_from_local(ip, n);
}

// Zero direction components (box bound, see closest_hit).  The reference's slab test
// skips an axis with d_a == 0 (bounding_box.cu:62-104), so such a ray "hits" every
// box its other coordinates cross, whatever o_a: the shadow rays of the directional
// light (0, -1, 1) and the primary rays of the centre column/row sweep whole rows
// of leaves.  Along the ray the coordinate stays o_a exactly (world and local:
// d_a and the local direction's component are 0), so an accepted hit lies within
// the slack of the leaf box on that axis: a node whose a-range excludes o_a by more
// than prune_abs has no acceptable hit below it (node boxes contain their leaves').
// The slab then becomes [K (mn - o - M), K (mx - o + M)] through the same fma and
// bias as a nonzero axis (pair_hit_at): both ends > 0 or < 0 exactly when o_a is
// outside [mn - M, mx + M] (a certain miss), else lo_a <= 0 < 1e-5 <= hi_a never
// binds (every nonzero axis bounds t by ~1e3; lo <= 0 is below any acceptable
// time, so entry bounds stay valid).  closest_hit's `im` keeps the nonzero axes only.
// Fast (ordered-LBVH) kernels only.
// `slack`: the scene's prune_abs (camera rays: |cam.pos| is folded into it), or a caller ray's own
// (query_kernel: the same bound with the ray's origin in the camera's place; < 0 for a lane: off).
__device__ __forceinline__ void zero_axis_cut(float slack, const Ray& r, RayInv& ri) {
    if (!(slack >= 0.0f)) return;
    constexpr float K = 0x1p32f;
    if (r.d.x == 0.0f) { ri.ix = K; ri.bx = K * slack; }
    if (r.d.y == 0.0f) { ri.iy = K; ri.by = K * slack; }
    if (r.d.z == 0.0f) { ri.iz = K; ri.bz = K * slack; }
}
__device__ __forceinline__ void zero_axis_cut(const SceneView& S, const Ray& r, RayInv& ri) { zero_axis_cut(S.prune_abs, r, ri); }

// First step of the fast traversal for a ray (closest_hit, FT path, node 0 with an empty
// closest hit): whether it hits either child of the ordered LBVH's root.  A lane for which
// this is false visits nothing, and its query returns no hit.
__device__ __forceinline__ bool ft_root_hit(const SceneView& S, const BvhRefs& bv, bool active, const Ray& r) {
    RayInv ri = ray_inv(r);
    zero_axis_cut(S, r, ri);
    bool h0, h1;
    float t0, t1;
    pair_hit_at(bv.fnode, r, ri, active, h0, h1, t0, t1);     // the root record
    return h0 || h1;
}

// renv::gpu::cast_ray (scene.cu:42-73) for the whole wave.  Packet traversal of
// the reference's implicit heap: at an internal node hit by some lane, both
// children (2k, 2k+1: adjacent records) are tested; the wave descends into 2k
// first and keeps 2k+1 pending in a per-depth bit trail (wave-uniform, SGPR).
// Each lane processes exactly the leaves its own ray hits, in the reference's
// DFS order, so results equal the single-ray semantics; counters are the
// single-ray node tests (1 + 2 per internal node hit).
// `occl_t` >= 0 enables the occlusion early exit (shadow rays, all-opaque scenes): a
// lane stops once it has accepted a hit with time <= occl_t = max_t * (1 - 8u).
// The reference's closest hit is then also <= max_t and opaque (every later accept
// is < that time up to the instance/mesh rescaling, |scale - 1| <= 4u), so
// Light::attenuate returns 0 either way (light.cu:39-45).  Counters then count
// the work done, so it is only used when statistics are not requested.
//
// Box bound on acceptable times (S.prune_abs >= 0).  Claim: a triangle of a leaf can
// only be accepted at a local time t >= tmin(box) - M(t).  The accepted point lies
// within eps of its triangle (the barycentric-sum tolerance 1e-5 of geometry.h:
// 281-286 allows ~1e-5 x triangle size in its plane), the triangle lies in the leaf
// box when every pose is a pure translation and mesh offsets are zero (the host
// checks; the boxes ignore the mesh pose, raytracer.cu:54-89), and the local ray
// differs from the world ray by O(u (|coords| + t)).  So the world ray is within
// eps + delta of the box at time t, i.e. inside the box grown by that distance,
// whose slab entry is >= tmin - (eps + delta) * max_a |1/d_a| (a zero component is
// no constraint, a subnormal one gives an infinite bound).  The slack used is
// M(t) = (prune_abs + 2^-14 |t|) * im + 2^-14 |t|, im = max_a |1/d_a|, prune_abs =
// 4e-4 x max vertex coordinate + 2^-14 x scene radius: >= 20x the tolerance terms.
// Uses (both exact):
//  * distance pruning (frames without statistics): a lane skips a subtree whose box
//    entry bound tlo exceeds c + M(c), c = min(b.time, lim).  Its leaves would be
//    processed with b.time <= c and nothing in them can be accepted (a nested box is
//    entered no earlier).  `lim` = max_t for shadow segments: hits beyond it never
//    change Light::attenuate (light.cu:35-58).
//  * triangle skip (cast_local's t_lo): a triangle whose plane crossing is certainly
//    before tlo(leaf) - M cannot be accepted, so its inside test is not run.
//
// Occluder hint (HINT: the fast NS = 0 trace kernels; `hslot` non-null: a shadow wave query of an
// all-opaque scene with the scene's hint table).  `seed` (hint_code, 0: none,
// its node checked by the caller) names a leaf by its parent's record and side.  The loop's first
// iteration is then that record's pair test for that child alone -- the popped-leaf-B form -- and
// the one leaf site, with the root next.  The visit is one the walk itself can make (same pair test,
// same cut, same entry bound), only early: a lane it occludes (b.time <= occl_t) is done by the
// criterion above, every other lane's Best is put back to "no hit" and its walk is the unseeded
// one, bit for bit.  A side that is no leaf in this frame's tree (a stale code) visits nothing.  An occluded
// lane's b.tri is replaced by the code of the leaf visit that occluded it (nothing reads a shadow
// hit's triangle in an opaque scene), and after the walk lane 0 stores at most one word to *hslot:
// the code of a lane the walk occluded and the seed did not, or 0 when a seed decided no lane.
//
// Nearer child first (NEAR: the hinted kernels and their profiling twin; `nf_in`, wave-uniform: this
// query walks near-first -- no shadow lane, pruning on).  At a step where
// some lane hits each child, the lanes that hit both vote with the entry bounds the step already
// has: B is visited first when more of them enter B first (ties and empty votes: A first).  The
// two children then change places before the step's one set of arms: a pending internal A is
// pushed as B is, a pending leaf A as NF_LEAF_A + its parent, popped as the "that child alone" form
// (bonly 4), and two leaves reach the leaf site B first.  A step that hits one child or none runs
// what it ran, after one scalar test.  The order can only matter between near-tied leaves:
// cast_local flags the lane that meets one, and a walk that ends with a flagged lane puts every
// lane's Best back to "no hit" and runs again from the root in DFS order (nf off), so the result
// is the DFS walk's bit for bit.  wc.nf: the wave's near-first queries, reruns and swapped steps
// (NF_FIELD_BITS each).
//
// Query kind (KIND).  The live lanes of an NS = 0 kernel run in lockstep, so a
// wave query there is all normal lanes or all shadow lanes, and the two features belong to one kind
// each: the caller picks the walk once per wave query, and neither kind carries the other's code.
//  QK_ANY     neither feature (every kernel outside the class, and the caller-ray queries);
//  QK_SHADOW  hints, with the occlusion exit and `lim`; no vote, no swap, no pending leaf A, no
//             near-tie flag and no rerun.  A normal lane in it (occl_t < 0, lim = inf) walks in DFS order;
//  QK_NORMAL  near-first (`nf_in` still a run-time value: the rerun and the switch need it); no seed,
//             no occlusion exit, `occl_t` and `lim` not read (the cut is the closest hit's alone);
//  QK_NEAR    near-first with the occlusion exit and `lim`, no hints: the profiling twin's one walk.
enum QueryKind { QK_ANY = 0, QK_SHADOW, QK_NORMAL, QK_NEAR };
constexpr int NF_LEAF_A = 1 << 30;                            // stack entry -2 - (NF_LEAF_A + node): pending leaf A of node
__device__ __forceinline__ int lane_id_fresh();               // (defined with the launch-parameter helpers below)
template <bool NOLEAF, bool STATS, bool FT = false, bool AXIS = false, bool PROF = false, bool BRUTE = false,
          int KIND = QK_ANY>
__device__ __forceinline__ bool closest_hit(const SceneView& S, const BvhRefs& bv, bool active_in, const Ray& r,
                                            Best& b, WaveCounters& wc, float occl_t = -1.0f,
                                            float lim = INFINITY, float zcut = -1.0f, int seed = 0,
                                            int* hslot = nullptr, bool nf_in = false) {
    constexpr bool HINT = KIND == QK_SHADOW, NEAR = KIND == QK_NORMAL || KIND == QK_NEAR;
    constexpr bool OCCL = KIND != QK_NORMAL;                   // the occlusion exit and `lim` are compiled in
    static_assert(!HINT || (FT && !STATS && !PROF && !BRUTE && !NOLEAF), "hints: the fast kernels' ordered walk");
    static_assert(!NEAR || (FT && !STATS && !BRUTE && !NOLEAF), "near-first: the fast kernels' ordered walk");
    const bool prune = !STATS && S.prune_abs >= 0.0f;
    float im = 0.0f;                                           // max_a |1/d_a| (set below)
    auto slack = [&](float t) { return (S.prune_abs + 0x1p-14f * fabsf(t)) * im + 0x1p-14f * fabsf(t); };
    auto cut = [&]() {
        const float c = OCCL ? fminf(b.time, lim) : b.time;
        return c + slack(c);
    };
    bool active = active_in;
    const unsigned long long am = __ballot(active);
    if (STATS || PROF) { wc.rays += __popcll(am); wc.wq++; }
    bool hit = false;
    if (BRUTE) {
        // Brute-force kernels (M_BRUTE; the reference's -r, scene.cu:48-52): every instance in
        // ascending order, strict < on time, with no tree code compiled in (the traversal's
        // registers and its second copy of the leaf code made config 2's kernel spill).  The
        // triangles take the axis-plane path (AXIS: identity rotations) with no entry bound;
        // a lane that found an occluding hit (occl_t, all-opaque scenes) stops.
        DirPre pre{};
        if (AXIS) pre = dir_pre<true>(r.d, active);
        else if (S.ident_all) pre = dir_pre(r.d, active);
        bool live = active;
        for (int i = 0; i < S.n_inst; i++) {
            if (!__ballot(live)) break;
            if (live && cast_local<false, AXIS, PROF>(S, bv, i, r, b, pre, wc, -INFINITY)) {
                hit = true;
                if (b.time <= occl_t) live = false;
            }
        }
        return hit;
    }
    if (!FT && (!S.use_bvh || S.n_leaf == 0)) {               // brute force (scene.cu:48-52)
        DirPre pre{};
        if (S.ident_all) pre = dir_pre(r.d, active);
        for (int i = 0; i < S.n_inst; i++) {
            if (STATS) {
                wc.leaves += __popcll(am);
                wc.tris += (unsigned long long)__popcll(am) * ldc(S.meshes, uni(__float_as_int(bv.inst[i].w) & 0x7fffffff)).tri_count;
            }
            if (active && cast_local<STATS>(S, bv, i, r, b, pre, wc, -INFINITY)) hit = true;
        }
        return hit;
    }
    const int n = S.n_leaf;
    RayInv ri = ray_inv(r);
    im = ri.exact ? INFINITY : fmaxf(fabsf(ri.ix), fmaxf(fabsf(ri.iy), fabsf(ri.iz)));
    if (FT) zero_axis_cut(S, r, ri);
    if (FT) zero_axis_cut(zcut, r, ri);                       // (caller rays, per lane: query_kernel)
    if (FT) {
        // Ordered LBVH (fast kernel, S.ftree): same leaves and leaf order as the heap, so
        // each lane meets exactly the leaves its ray hits, in the heap's DFS order (a
        // hit leaf's ancestors contain it and are hit: the slab test is monotone in the
        // box).  Wave-uniform stack of pending B children in lanes 0..31 of one VGPR
        // (tree depth <= 31 is checked on the host): an internal node as its index, a
        // leaf B as -2 - parent, whose pair test is re-run when it is popped (fresh hit
        // and entry bound under the current cut).  Pruning and triangle skip as above.
        // The per-query direction chain (dir_pre) is formed at the wave's first leaf visit:
        // most queries (sky rays) reach no leaf, and it depends on the ray only.
        DirPre pre{};
        bool pre_ok = false;                                   // wave-uniform
        const bool box_bound = S.prune_abs >= 0.0f;
        auto t_low = [&](float tl) { return box_bound ? tl - slack(tl) : -INFINITY; };
        // One pair-test site and one leaf site (the leaf code is the bulk of the kernel):
        // an iteration tests a node's pair -- or, for a popped pending leaf B, re-tests its
        // parent's pair for child B only -- then runs at most one leaf; when both children
        // are leaves, B waits in registers (h2, t2, inst2) for the next iteration.
        // Per-lane state as floats, not booleans (a boolean live across the loop's blocks
        // costs scalar mask updates on every edge): a child's test result is its entry bound
        // t, or NaN for a miss; the lane's cut ct (the pruning bound, +inf without pruning)
        // is NaN once the lane is inactive (no query, or occluded), so "hit and not pruned"
        // is the one comparison t <= ct, false for every NaN.  The cut changes only when a
        // leaf improves the closest hit: recomputed after each leaf visit, not every step.
        const float QNAN = __builtin_nanf("");
        float ct = !active_in ? QNAN : prune ? cut() : INFINITY;
        // Compact step (same visits, same order), one loop latch: a step either descends into
        // A (B pushed when hit) or runs up to two leaves at the single leaf site (A then B) and
        // continues at an internal B or pops.  A popped "leaf B of node X" re-runs X's pair test
        // and goes straight to the leaf site.  A leaf A before an internal B no longer pushes B
        // (the stack holds no more than before).  Pushes are v_writelane into the stack VGPR.
        // Same-box A/B (profiles/r02/ab_trav2.log): frame 0.833 -> 0.810 ms, trace 0.973 -> 0.952.
        if (ri.exact) ri.ix = ri.iy = ri.iz = QNAN;           // every box: the exact test (pair_hit_tt2)
        // bonly: 1 a popped leaf B of `node`; 2 / 3 (HINT) the seed, leaf A / B of `node`.  The seed's
        // iteration is the only one whose next node is the root (next == 0), and everything it adds sits
        // on the popped-leaf and leaf-visit paths: a descending step runs what it ran without hints.
        // (NEAR) 4: a popped pending leaf A of `node`.
        int node = 0, sp = 0, stk = 0, bonly = 0;
        if (HINT && seed > 0) { node = hint_node(seed); bonly = 2 + hint_side(seed); }
        unsigned nf = NEAR && nf_in;                           // (uniform, 0 / 1) this walk orders by the vote
        int flag = 0;                                          // the lane met a near-tie between leaves (cast_local)
        int nsw = 0, nrr = 0;                                  // (uniform) swapped steps, reruns
        // (the entry through readfirstlane: a no-op where the compiler knows it uniform, which it does in
        // every kernel but the profiling variant once that orders its walk)
        auto push = [&](int e) { asm("v_writelane_b32 %0, %1, m0" : "+v"(stk) : "s"(uni(e)), "{m0}"(sp)); sp++; };
        for (;;) {
            const float4* rec = bv.fnode + 4 * node;
            if (PROF) wc.wpair++;
            const float2 rf = *reinterpret_cast<const float2*>(rec + 3);
            int ra = uni(__float_as_int(rf.x)), rb = uni(__float_as_int(rf.y));
            float ta, tb;
            pair_hit_tt2c(rec, r, ri, ct, ta, tb);
            float lt = QNAN, t2 = QNAN;                        // leaf entry bounds (NaN: missed)
            int linst = -1, inst2 = -1, next = -1;             // their instances, the next node (uniform; -1: pop)
            int lcode = 0;                                     // hint_code of leaf `linst` (HINT)
            if (bonly) {                                       // popped: leaf B of this node
                if (NEAR && bonly == 4) {                      // a pending leaf A: that child alone
                    lt = ta; linst = -1 - ra; lcode = hint_code(node, 0);
                } else
                if (HINT && bonly > 1) {                       // the seed: that child alone if it is a leaf, then the root
                    next = 0;
                    const int rs = bonly == 2 ? ra : rb;
                    if (rs < 0) { lt = bonly == 2 ? ta : tb; linst = -1 - rs; lcode = seed; }
                } else {
                    lt = tb; linst = -1 - rb; lcode = hint_code(node, 1);
                }
                bonly = 0;
            } else {
                const unsigned hA = any_lane(__ballot(ta <= ct)), hB = any_lane(__ballot(tb <= ct));
                int sw = 0;                                    // NF_LEAF_A: the children changed places for this step
                if (NEAR && (nf & hA & hB)) {                  // the vote of the lanes that hit both children
                    const unsigned long long both = __ballot(ta <= ct && tb <= ct);
                    if (__popcll(__ballot(tb < ta) & both) > __popcll(__ballot(ta < tb) & both)) {
                        // more of them enter B first: B plays A from here on (a pending leaf "B" is then leaf
                        // A of the node; lcode names the other side, and nothing reads it: no shadow lane)
                        const int rs = ra; ra = rb; rb = rs;
                        const float ts = ta; ta = tb; tb = ts;
                        sw = NF_LEAF_A;
                        nsw++;
                    }
                }
                if (ra >= 0 && hA) {                           // descend into A, B after A's subtree
                    next = ra;
                    if (hB) push(rb >= 0 ? rb : -2 - node - sw);
                } else {
                    if (hA) { lt = ta; linst = -1 - ra; lcode = hint_code(node, 0); }   // leaf A (ra < 0 here)
                    if (hB) {
                        if (rb >= 0) next = rb;                // after leaf A, if any
                        else if (linst >= 0) { t2 = tb; inst2 = -1 - rb; }
                        else { lt = tb; linst = -1 - rb; lcode = hint_code(node, 1); }
                    }
                }
            }
            if (linst >= 0) {
                for (;;) {                                     // the leaf site: one or two leaves
                    const bool lh = lt <= ct;                  // (ct only decreases: fresh for the second leaf)
                    if (__ballot(lh)) {
                        if (!pre_ok) {
                            if (AXIS) pre = dir_pre<true>(r.d, active_in);    // S.tri_ax set: identity rotations
                            else if (S.ident_all) pre = dir_pre(r.d, active_in);
                            pre_ok = true;
                        }
                        const unsigned long long cl0 = PROF ? __builtin_amdgcn_s_memtime() : 0;
                        if (PROF) { wc.wleaf++; wc.leaves += __popcll(__ballot(lh)); }
                        if (lh && cast_local<false, AXIS, PROF, NEAR>(S, bv, linst, r, b, pre, wc, t_low(lt), nf != 0, flag))
                            if (OCCL && b.time <= occl_t) {    // occluded: this lane is done
                                ct = QNAN;
                                if (HINT) b.tri = lcode;
                            }
                        if (prune && ct == ct) ct = cut();
                        if (PROF) wc.cyc_leaf += __builtin_amdgcn_s_memtime() - cl0;
                        if (!__ballot(ct == ct)) { next = -1; sp = 0; break; }   // every lane occluded: done
                    }
                    if (inst2 < 0) break;
                    lt = t2; linst = inst2; inst2 = -1; lcode++;   // (leaf B after leaf A)
                }
                if (HINT && next == 0 && ct == ct) {           // after the seed visit: undecided lanes start clean
                    b.time = INFINITY; b.inst = -1; b.tri = -1; b.u = 0.0f; b.v = 0.0f;
                    ct = prune ? cut() : INFINITY;
                }
            }
            if (next >= 0) { node = next; continue; }
            if (sp == 0) {
                if (!(NEAR && nf && __ballot(flag != 0))) break;
                // a near-tie between leaves: every lane starts clean, in DFS order
                nf = 0; nrr = 1;
                b.time = INFINITY; b.inst = -1; b.tri = -1; b.u = 0.0f; b.v = 0.0f;
                ct = !active_in ? QNAN : prune ? cut() : INFINITY;
                node = 0;
                continue;
            }
            sp--;                                              // an internal node, or leaf B of node -2 - e
            const int e = __builtin_amdgcn_readlane(stk, sp);
            if (e < 0) {
                node = -2 - e; bonly = 1;
                if (NEAR && node >= NF_LEAF_A) { node -= NF_LEAF_A; bonly = 4; }
            }
            else node = e;
        }
        if (NEAR && nf_in)
            wc.nf += 1ull + ((unsigned long long)nrr << NF_FIELD_BITS) + ((unsigned long long)nsw << 2 * NF_FIELD_BITS);
        if (HINT && hslot) {                                   // (uniform) at most one word, not waited for
            // A lane the seed visit occluded holds the seed as its code; a lane the walk occluded holds
            // another (the walk's visit of the seed's leaf decides what the seed visit decided).
            const unsigned long long oc = __ballot(b.time <= occl_t), sd = oc & __ballot(b.tri == seed);
            const unsigned long long od = oc & ~sd;
            wc.hint += 1ull + (seed > 0 ? 1ull << HINT_FIELD_BITS : 0ull) +
                       (sd && sd == __ballot(active_in) ? 1ull << 2 * HINT_FIELD_BITS : 0ull);
            if (od || (seed > 0 && !sd)) {
                const int code = od ? __builtin_amdgcn_readlane(b.tri, __builtin_ctzll(od)) : 0;
                if (lane_id_fresh() == 0) *hslot = code;
            }
        }
        return active_in && b.time < INFINITY;                 // an accepted triangle has a finite time
    }
    if (STATS) wc.nodes += __popcll(am);                       // root test
    bool hr, hdummy;
    float tdummy, troot;
    pair_hit(bv.pair, 0, r, ri, active, hdummy, hr, tdummy, troot);   // pair 0 = (unused, root)
    const unsigned long long br = __ballot(hr);
    if (!br) return false;
    DirPre pre{};
    if (S.ident_all) pre = dir_pre(r.d, active);
    // lower bound of acceptable local times in a leaf entered at >= tl (see distance pruning)
    const bool box_bound = !STATS && S.prune_abs >= 0.0f;   // counted kernel: plain reference path
    auto t_low = [&](float tl) { return box_bound ? tl - slack(tl) : -INFINITY; };
    auto leaf = [&](bool h, int li, float tl) {
        const unsigned long long m = __ballot(h);
        if (!m) return;
        const int ti = uni(bv.leaf[li]);                       // leaf instance: wave-uniform
        if (STATS) {
            const int tc = ldc(S.meshes, uni(__float_as_int(bv.inst[ti].w) & 0x7fffffff)).tri_count;
            wc.leaves += __popcll(m);
            wc.tris += (unsigned long long)__popcll(m) * tc;
            wc.wleaf++;
            wc.wtri += tc;
        }
        const unsigned long long c0 = STATS ? __builtin_amdgcn_s_memtime() : 0;
        if (NOLEAF) { if (h) { hit = true; b.inst = ti; } }
        else if (h && cast_local<STATS>(S, bv, ti, r, b, pre, wc, t_low(tl))) {
            hit = true;
            if (b.time <= occl_t) active = false;             // occluded: this lane is done
        }
        if (STATS) wc.cyc_leaf += __builtin_amdgcn_s_memtime() - c0;
    };
    if (n == 1) { leaf(hr, 0, troot); return hit; }
    // one copy of the leaf code for both children (keeps the kernel small)
    if (STATS) wc.nodes += 2ull * __popcll(br);
    int k = 1;
    unsigned pending = 0;
    for (;;) {
        const int c0 = 2 * k;
        bool h0, h1;
        float t0, t1;
        pair_hit(bv.pair, k, r, ri, active, h0, h1, t0, t1);  // children 2k, 2k+1
        if (prune) {
            const float ct = cut();
            h0 = h0 && !(t0 > ct);
            h1 = h1 && !(t1 > ct);
        }
        if (STATS) wc.wpair++;
        if (c0 >= n) {                                         // children are leaves: DFS order 2k, 2k+1
#pragma nounroll
            for (int c = 0; c < 2; c++) leaf(c == 0 ? h0 : (h1 && !(prune && t1 > cut())), c0 + c - n, c == 0 ? t0 : t1);
            if (!__ballot(active)) break;                      // every lane occluded
        } else {
            const unsigned long long b0 = __ballot(h0), b1 = __ballot(h1);
            if (STATS) wc.nodes += 2ull * (__popcll(b0) + __popcll(b1));
            if (b0) {
                if (b1) pending |= 1u << (31 - __clz(c0));
                k = c0;
                continue;
            }
            if (b1) { k = c0 + 1; continue; }
        }
        if (!pending) break;
        const int d = 31 - __clz(pending);                     // deepest pending right sibling
        pending &= ~(1u << d);
        k = (k >> ((31 - __clz(k)) - d)) + 1;
    }
    return hit;
}

// ---------------------------------------------------------------------------
// Shading: phong.cu:14-53, light.cu:11-77, scene.cu:14-22
// ---------------------------------------------------------------------------
// kd: the material's Kd (the reference), or the atlas texel in the textured mode
// diffuse + specular: phong's factor of the incoming light
// tl_len = len(to_light), tl_neg_unit = normalized(neg(to_light)) (the shadow ray's direction
// negated: the light step has them)
__device__ __forceinline__ V4 phong_factor(const DMat& m, V4 kd, V3 nrm, V3 nrm_unit, V3 ray_dir, V3 to_light,
                                           float tl_len, V3 tl_neg_unit) {
    float nd = max_std(dot(to_light, nrm), 0.0f);
    V4 diffuse = nd * kd;
    // reflect(neg(to_light), nrm) = reflect_pre(tl_len, tl_neg_unit, nrm_unit), its one normalisation voted
    V3 reflected = tl_len * normalized_vote(reflect_w(tl_neg_unit, nrm_unit));
    float rd = dot(neg(reflected), ray_dir);
    V4 specular = pow_fast(max_std(rd, 0.0f), m.alpha) * m.Ks;
    return diffuse + specular;
}
// phong(m, kd, nrm, incoming, ...) = phong_factor(m, kd, nrm, normalized(nrm), ...) * incoming (trace_sample's
// light step)

// RayFrame (scene.cu:81-90).  The top frame's hit point and normal are not kept in
// registers: while the frame is being lit they equal at(ray, is_time) and is_norm
// (the reference assigns them from exactly those, scene.cu:117-120), and a frame
// resumed from the stack reads them from its saved copy.
struct Frame {
    Ray ray;
    V4 atten;
    int last_mat, type, depth, in_obj;
};
struct SavedFrame { Frame f; V3 hit_pt, norm; };   // suspended under its reflection child

// The launch's TraceParams read in place from the kernel-argument segment (constant address
// space: scalar loads) through a pointer made fresh at each use site.  Passed by value and
// used directly, its ~80 dwords were loaded once and held in SGPRs for the whole persistent
// kernel; the scalar register file overflowed into VGPR lanes, and every group and every
// state-machine step re-read them with v_readlane (VALU issue slots).  Fresh per scope, a
// field is loaded (s_load) where it is needed and its SGPRs are free elsewhere.
typedef __attribute__((address_space(4))) const TraceParams KTP;
// a struct field of the in-place parameters, copied to registers word by word (scalar loads)
template <class T> __device__ __forceinline__ T kld(const __attribute__((address_space(4))) T& x) {
    static_assert(sizeof(T) % 4 == 0, "4-byte granular");
    T r;
    const __attribute__((address_space(4))) uint32_t* src = (const __attribute__((address_space(4))) uint32_t*)&x;
    uint32_t* d = reinterpret_cast<uint32_t*>(&r);
#pragma unroll
    for (int w = 0; w < (int)(sizeof(T) / 4); w++) d[w] = src[w];
    return r;
}
__device__ __forceinline__ KTP& kparams() {
    KTP* p = (KTP*)__builtin_amdgcn_kernarg_segment_ptr();     // the first kernel argument
    asm volatile("" : "+s"(p));
    return *p;
}
// The trace kernel's SceneView (its second argument, right after TraceParams) read the same way:
// a fresh copy per scope (the state loop's iteration, the group) is loaded where it is used
// instead of being held in SGPRs across the persistent loops.  RT_FRESH_SCENE=0: the by-value
// argument throughout (the A/B arm).
#ifndef RT_FRESH_SCENE
#define RT_FRESH_SCENE 1
#endif
typedef __attribute__((address_space(4))) const SceneView KSV;
static_assert(sizeof(TraceParams) % alignof(SceneView) == 0, "SceneView follows TraceParams in the kernarg segment");
static_assert(sizeof(TraceParams) == 400 && sizeof(SceneView) == 152 && offsetof(SceneView, hint) == 128 &&
                  offsetof(SceneView, nf_ctr) == 136,
              "kernarg layout (the kernels read it in place; the hint table after the 128 bytes every variant had, "
              "the near-first fields after it)");
__device__ __forceinline__ SceneView kscene() {
    const __attribute__((address_space(4))) char* p =
        (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return kld(*(KSV*)(p + sizeof(TraceParams)));
}
#if RT_FRESH_SCENE
#define SV() kscene()
#else
#define SV() S
#endif

// Textured mode (build-defined; phong.cu:18-23 leaves texture mapping a TODO): the
// diffuse colour of a hit on a triangle with TextureCoords is the atlas texel at
// (tx, ty) + u (ux, uy) + v (vx, vy), clamped to the atlas and truncated to a texel
// index (point sampling, clamp addressing: the reference's texture setup); other hits
// keep the material's Kd.  gfx950 has no image/sampler instructions (HIP marks tex2D
// unavailable there), so the atlas is a plain float4 array in HBM.
template <class PT>
__device__ __forceinline__ V4 hit_kd(const PT& P, const BvhRefs& bv, const Best& b, int mat) {
    const DTri& T = bv.tris[b.tri];
    if (!T.tex) return bv.mats[mat].Kd;
    const float x = (T.tx + b.u * T.ux) + b.v * T.vx;
    const float y = (T.ty + b.u * T.uy) + b.v * T.vy;
    const int ix = (int)fminf(fmaxf(x, 0.0f), (float)(P.atlas_w - 1));
    const int iy = (int)fminf(fmaxf(y, 0.0f), (float)(P.atlas_h - 1));
    const float4 c = P.atlas[(size_t)iy * P.atlas_w + ix];
    return v4(c.x, c.y, c.z, c.w);
}

// Opaque to the optimiser: values derived from x (64-bit output addresses) are formed
// here instead of being hoisted to the group start and spilled across the trace.
__device__ __forceinline__ void opaque(int& x) { asm volatile("" : "+v"(x)); }
// Build-defined sample offset k (rt_scene.cpp spp_offset: R2 sequence in double), computed
// with the same correctly rounded double operations as the host table (no memory access in
// the group loop: a vector load there waits, in order, for the previous group's stores and
// for the work-ticket atomic in flight).
__device__ __forceinline__ float2 spp_offset_dev(int k) {
    const double u = (double)k * 0.7548776662466927, v = (double)k * 0.5698402909980532;
    return make_float2((float)(u - floor(u)), (float)(v - floor(v)));
}

// A wave-uniform value made loop-variant where it is used: per-group constants derived from
// it (camera terms of the kernel arguments) are recomputed there instead of being hoisted out
// of the persistent group loop, held in VGPRs across the trace and spilled (the spill reloads
// were long-latency scratch misses at every group start).
template <class T> __device__ __forceinline__ T fresh_s(T x) { asm volatile("" : "+s"(x)); return x; }
// This lane's index, recomputed where it is used (two VALU) rather than held across the
// persistent loop (it was spilled and reloaded from scratch at every group).
__device__ __forceinline__ int lane_id_fresh() {
    const unsigned m = fresh_s(~0u);
    return (int)__builtin_amdgcn_mbcnt_hi(m, __builtin_amdgcn_mbcnt_lo(m, 0u));
}

// Lane -> (pixel, sample) of pixel group g, from the launch parameters (shifts for powers of
// two).  Recomputed where each term is used (camera ray, hit-id and output stores) rather than
// held in registers across the trace: the output pixel's index held across it was spilled to
// scratch (a store per group and lane; brute-force frames at spp = 1 wrote ~12 B per pixel).
struct GroupLane { int px, py, sub, base, pix; bool valid; };
__device__ __forceinline__ GroupLane group_lane(int g) {
    KTP& P = kparams();
    const int L = P.lanes_per_px;
    const int gy = (int)udiv((unsigned)g, kld(P.div_ngx)), gx = g - gy * P.n_gx;
    const int ln = lane_id_fresh();
    const int pix_g = P.l_shift >= 0 ? ln >> P.l_shift : ln / L;
    const int pxo = P.gw_shift >= 0 ? pix_g & (P.gw - 1) : pix_g % P.gw;
    const int pyo = P.gw_shift >= 0 ? pix_g >> P.gw_shift : pix_g / P.gw;
    GroupLane o;
    o.sub = P.l_shift >= 0 ? ln & (L - 1) : ln - pix_g * L;
    o.base = ln - o.sub;
    o.px = gx * P.gw + pxo;
    const int pr = gy * P.gh + pyo;
    o.valid = pix_g < P.px_per_wave && o.px < P.W && pr < P.n_rows;
    o.py = P.row0 + pr * P.row_step;
    o.pix = P.compact ? pr * P.W + o.px : o.py * P.W + o.px;   // < 2^31 (checked on the host)
    return o;
}



template <class PT>
__device__ __forceinline__ void dbg(const PT& P, bool me, int ev) {
    if (P.dbg_log && me) {
        int i = atomicAdd(P.dbg_log, 1);
        if (i < 4094) P.dbg_log[2 + i] = ev;
    }
}

// Camera::at (camera.cu:33-42), basis hoisted (bitwise identical, computed on the host)
__device__ __forceinline__ Ray camera_at(const DCamera& c, float cx, float cy) {
    float gx = (cx - (0.5f * c.W)) / c.unit;
    float gy = (0.5f * c.H - cy) / c.unit;
    V3 dir = (c.near_ * c.f + gx * c.r) + gy * c.u;
    return make_ray(c.pos, dir);
}

// One camera sample per lane through renv::gpu::propagate_ray (scene.cu:92-188),
// run as an explicit state machine whose only wave-collective step is the
// closest-hit query.  Each piece of the reference's control flow appears once:
//   ST_ADVANCE     REFLECT / REFRACT frame transitions until a NORMAL frame needs a ray
//   ST_WAIT_NORMAL waiting for the frame's closest hit (scene.cu:101-127)
//   ST_LIGHT       illuminate(): set up the shadow ray of light `li` (phong.cu:42-53)
//   ST_WAIT_SHADOW waiting for a shadow segment (Light::attenuate, light.cu:29-61)
// The top frame lives in registers; frames suspended under a reflection child (at
// most `depth`) in the private array `stk`.  rec_ids: this lane carries the pixel's
// sample 0 and records the primary hit ids of its pixel in group g.
enum : int { ST_DONE = 0, ST_ADVANCE = 1, ST_WAIT_NORMAL = 2, ST_LIGHT = 3, ST_WAIT_SHADOW = 4 };

// Parking (PARK): integrator state the traversal never reads is written to this lane's
// LDS column before each query and read back after it, so the query runs with those
// registers free (instead of the allocator spilling to scratch, whose working set is
// larger than L2: measured ~0.9 GB of write-back per frame).  The memory clobbers
// stop the compiler from forwarding the stored values and keeping them live.
// The light's phong factor (phong.cu:14-53 without the incoming light) is formed once, when the
// shadow query is set up, and parked: the light's term after the query is factor x incoming,
// the same operations in the same order as the reference's phong.  NS = 0 kernels park 4 fields
// fewer (park_fields, rt_plan.h; partial parking: PART_FIELDS there).
// Parked kernels also park normalized(hit normal), formed once per hit for phong's reflect
// (every light) and the reflection ray, instead of once per use (same value: frame -1.8%,
// profiles/r04/ab_nn.log).
template <int NS, bool STATS, bool PARK, bool TEX, bool FT, bool AXIS, bool PROF = false, bool BRUTE = false,
          bool PART = false>
__device__ __forceinline__ V4 trace_sample(const SceneView& S, const BvhRefs& bv, bool valid,
                                           Ray r0, bool me, bool rec_ids, int g, WaveCounters& wc, float* park, int& nq) {
    constexpr bool OPQ = NS == 0;                               // no refractive material in the scene
    constexpr bool NN = PARK;                                   // is_nn parked across the queries
    // occluder hints (closest_hit): the fast, fully parked or unparked, lockstep (NS = 0) kernels
    constexpr bool HINT = FT && OPQ && !STATS && !PROF && !BRUTE && !PART;
    // nearer child first (closest_hit): the same kernels, and their profiling twin on request
    constexpr bool NEAR = FT && OPQ && !STATS && !BRUTE && !PART;
    int hkey = -1;                                              // hint_key of the wave's last normal hit (uniform)
    KTP& P0 = kparams();
    Frame cur;
    SavedFrame stk[NS > 0 ? NS : 1];
    int top = -1, st = ST_DONE;
    // bit 0: primary ray not yet answered; bit 1: pop after illumination (depth 0);
    // bit 2: `cur` was resumed from stk[top] (hit point / normal live there);
    // bit 3: this lane records the pixel's primary hit ids (sample 0)
    int fl = rec_ids ? 9 : 1;
    V4 acc = v4(0, 0, 0, 0);
    float is_time = INFINITY;                                   // the sample's shared Isect
    V3 is_norm = v3(0, 0, 0);
    V3 is_nn = v3(0, 0, 0);                                     // normalized(is_norm) (parked kernels)
    int is_mat = 0;
    V4 is_kd = v4(0, 0, 0, 0);                                  // textured mode: the hit's diffuse colour
    int li = 0;
    V4 summed = v4(0, 0, 0, 0), rv = v4(0, 0, 0, 0);
    V4 fct = v4(0, 0, 0, 0);                                    // the light's phong factor
    float da = 1.0f, max_t = 0.0f;
    Ray q = r0;
    if (valid) {
        cur.ray = r0;
        cur.atten = v4(1.0f, 1.0f, 1.0f, 1.0f); cur.last_mat = -1;
        cur.type = F_NORMAL; cur.depth = P0.depth; cur.in_obj = 0;
        top = 0; st = ST_ADVANCE;
    }
    auto pop = [&]() {
        top--;
        if (NS > 0 && top >= 0) { cur = stk[top].f; fl |= 4; }
    };
    unsigned long long c_post = 0;
    for (;;) {
        KTP& P = kparams();
        if ((STATS || PROF) && c_post) { wc.cyc_post += __builtin_amdgcn_s_memtime() - c_post; c_post = 0; }
        // ---- local transitions until this lane waits for a query or is done ----
        // ST_LIGHT
        auto light_step = [&]() {
            const unsigned long long cl = PROF ? __builtin_amdgcn_s_memtime() : 0;
            if (li < SV().n_lights) {
                const DLight L = bv.lights[li];
                const V3 hpos = at(cur.ray, is_time);          // org_ray.at(isect.time) (phong.cu:48)
                V3 dtl;
                if (L.type == 0) {                             // PointLight::shine (light.cu:63-70)
                    V3 disp = L.v - hpos;
                    float dist = len(disp);
                    float quad = P.dist_atten.x + P.dist_atten.y * dist + P.dist_atten.z * dist * dist;
                    da = quad < 1.0f ? 1.0f : 1.0f / quad;
                    dtl = normalized(disp);
                    max_t = dist;
                } else {                                       // DirLight::shine (light.cu:72-77)
                    dtl = neg(L.v);
                    max_t = INFINITY;
                }
                // to = make_ray(hpos, dtl): normalized(dtl) formed here once; phong's
                // reflect(neg(dtl), n) takes |neg(dtl)| = |dtl| (the same squares) and
                // normalized(neg(dtl)) = neg(normalized(dtl)) (the same magnitudes, RNE is
                // sign-symmetric; +0s below THRESH in both)
                // (a point light's dtl is unit: closed forms on one vote of the lanes in this
                // step; a directional light's |dtl|^2 is the light's own, and fails it)
                float tl, tr;
                len_rcp_vote(dot(dtl, dtl), tl, tr);
                const bool tl_ok = tl > THRESH;
                const Ray to{hpos, tl_ok ? tr * dtl : v3(0.0f, 0.0f, 0.0f)};
                const V3 tn = tl_ok ? tr * neg(dtl) : v3(0.0f, 0.0f, 0.0f);
                rv = L.col;                                    // Light::attenuate (light.cu:30-31)
                // Unlit skip: when phong's factor (diffuse + specular) is zero in every
                // channel -- the light behind the surface, no specular lobe -- the light's
                // term (factor x incoming) is that signed zero for every incoming light
                // >= +0, which the host guarantees (unlit_skip: light colours >= +0 and
                // finite, transmission Kt in [+0, 1], so every attenuation is >= +0 and
                // finite).  The shadow segments cannot change the sum: none is traced.
                // The lane still takes the wait-for-shadow step, with no query (max_t = -inf
                // marks it): no hit, so the light's term is phong's with the unshadowed
                // light, the same signed zeros.
                const DMat& mm = bv.mats[is_mat];
                fct = phong_factor(mm, TEX ? is_kd : mm.Kd, is_norm, NN ? is_nn : normalized(is_norm), cur.ray.d,
                                   dtl, tl, tn);
                if (P.unlit_skip && fct.x == 0.0f && fct.y == 0.0f && fct.z == 0.0f && fct.w == 0.0f)
                    max_t = -INFINITY;
                q = Ray{at(to, THRESH), normalized_vote(to.d)};  // make_ray: to.d is unit already
                dbg(P, me, 4);
                st = ST_WAIT_SHADOW;
            } else {
                acc = acc + cur.atten * summed;                 // scene.cu:127
                if (fl & 2) { fl &= ~2; pop(); }
                st = top < 0 ? ST_DONE : ST_ADVANCE;
            }
            if (PROF) wc.cyc_light += __builtin_amdgcn_s_memtime() - cl;
        };
        // ST_ADVANCE, a NORMAL frame (scene.cu:100-103)
        auto normal_step = [&]() {
            is_time = INFINITY;
            dbg(P, me, 1);
            q = cur.ray;
            st = ST_WAIT_NORMAL;
        };
        // ST_ADVANCE, a REFLECT frame (scene.cu:129-148: the frame's own hit)
        auto reflect_step = [&]() {
            const DMat& m = bv.mats[is_mat];
            cur.type = F_REFRACT;
            if (m.reflective) {
                dbg(P, me, 2);
                const V3 hp = at(cur.ray, is_time);
                // NS = 0 with depth > 0: the host picks it only when no material is refractive.
                // The suspended frame would then only be popped when resumed (its REFRACT step
                // pops: the material of the shared Isect is never refractive, scene.cu:149-184),
                // and so would every frame under it, so the child replaces it (a tail call):
                // no stack, no scratch writes.
                if (NS > 0) {
                    stk[top].f = cur; stk[top].hit_pt = hp; stk[top].norm = is_norm;
                    top++;
                }
                cur.type = F_NORMAL;                           // the child: last_mat, in_obj inherited
                cur.atten = cur.atten * m.Kr;
                cur.depth = cur.depth - 1;
                // reflect's three lengths (the ray's, the normal's, the mirrored direction's) on one
                // vote of the reflecting lanes; the normal is taken inside this arm (reflect
                // re-normalises it: formed outside, that chain ran on every query).  Reflect of
                // unit vectors is unit: the Ray ctor's normalisation by unit_len_rcp, on a second vote.
                const V3 rd = reflect_vote(cur.ray.d, NN ? is_nn : normalized(is_norm));
                float rl;
                V3 rn;
                if (!__ballot(!unit_head(dot(rd, rd)))) rn = normalized_unit(rd, rl);
                else rn = normalized(keep_arm(rd));
                cur.ray = Ray{hp, rn};
            }
        };
        // Without a frame stack (NS = 0: no refractive material) a lane makes at most one pass of
        // LIGHT (the light step, or the frame's end), REFLECT, REFRACT (a pop: the sample is done),
        // NORMAL between two queries: the same steps in the same order as the loop below, as
        // predicated blocks, so that the integrator's state is not copied around a loop's back edge.
        if (NS == 0) {
            if (st == ST_LIGHT) light_step();
            if (st == ST_ADVANCE && cur.type == F_REFLECT) reflect_step();
            if (st == ST_ADVANCE && cur.type == F_REFRACT) { pop(); if (top < 0) st = ST_DONE; }
            if (st == ST_ADVANCE && cur.type == F_NORMAL) normal_step();
        } else
        while (st == ST_ADVANCE || st == ST_LIGHT) {
            if (st == ST_LIGHT) { light_step(); continue; }
            if (cur.type == F_NORMAL) { normal_step(); continue; }
            const DMat& m = bv.mats[is_mat];
            bool do_pop = false;
            if (cur.type == F_REFLECT) {
                reflect_step();
            } else if (!OPQ && m.refractive) {                    // F_REFRACT (scene.cu:149-184)
                dbg(P, me, 3);
                cur.type = F_NORMAL;
                float n1, n2;
                if (cur.in_obj) { n1 = bv.mats[cur.last_mat].eta; n2 = 1.0f; }
                else { n1 = 1.0f; n2 = bv.mats[cur.last_mat].eta; }
                V3 hp, nn;
                if (fl & 4) { hp = stk[top].hit_pt; nn = stk[top].norm; }
                else { hp = at(cur.ray, is_time); nn = is_norm; }
                bool tir;
                V3 rd = refract(cur.ray.d, normalized(nn), n1, n2, tir);
                if (tir) do_pop = true;
                else { cur.ray = make_ray(hp, rd); cur.in_obj = !cur.in_obj; cur.depth--; }
            } else {
                do_pop = true;
            }
            if (do_pop) { pop(); if (top < 0) st = ST_DONE; }
        }
        // ---- the wave-collective closest-hit query ----
        const bool need = (st == ST_WAIT_NORMAL || st == ST_WAIT_SHADOW);
        if (!__ballot(need)) break;
        nq++;                                                  // a wave query (uniform)
        Best b;
        b.time = INFINITY; b.inst = -1; b.tri = -1; b.u = 0.0f; b.v = 0.0f;
        float occl = -1.0f;
        if (P.occl_exit && st == ST_WAIT_SHADOW) occl = max_t * (1.0f - 0x1p-21f);
        const float lim = st == ST_WAIT_SHADOW ? max_t : INFINITY;
        // Occluder hint of a shadow wave query (closest_hit): the entry of the surface the wave
        // shades (hkey) and its light -- the live lanes of an NS = 0 kernel are on the same light --
        // read with one scalar load, issued here and used after the parking stores.
        int seed = 0;
        int* hslot = nullptr;
        if (HINT && hkey >= 0 && P.occl_exit) {
            const unsigned long long sm = __ballot(st == ST_WAIT_SHADOW && max_t >= 0.0f);
            int* const tab = SV().hint;
            if (sm && tab) {
                hslot = tab + hkey + (__builtin_amdgcn_readlane(li, __builtin_ctzll(sm)) & 3);
                seed = ldc(hslot, 0);
            }
        }
        const unsigned long long cpk0 = PROF ? __builtin_amdgcn_s_memtime() : 0;
        if (PARK) {
            float* pk = park;
            int f = 0;
            auto put = [&](float v) { if (!PART || f < PART_FIELDS) pk[f * TRACE_BLOCK_P] = v; f++; };
            put(cur.ray.o.x); put(cur.ray.o.y); put(cur.ray.o.z); put(cur.ray.d.x); put(cur.ray.d.y); put(cur.ray.d.z);
            put(cur.atten.x); put(cur.atten.y); put(cur.atten.z); put(cur.atten.w);
            put(acc.x); put(acc.y); put(acc.z); put(acc.w);
            put(summed.x); put(summed.y); put(summed.z); put(summed.w);
            put(fct.x); put(fct.y); put(fct.z); put(fct.w);
            if (NN) { put(is_nn.x); put(is_nn.y); put(is_nn.z); }
            if (!OPQ) { put(rv.x); put(rv.y); put(rv.z); put(rv.w); }
            asm volatile("" ::: "memory");
        }
        const unsigned long long c0 = (STATS || PROF) ? __builtin_amdgcn_s_memtime() : 0;
        if (PROF) wc.cyc_park += c0 - cpk0;
        // (an unlit-skipped shadow step, max_t = -inf, takes no query)
        const bool qa = st == ST_WAIT_NORMAL || (st == ST_WAIT_SHADOW && max_t >= 0.0f);
        const unsigned long long prof_p0 = wc.wpair, prof_l0 = wc.wleaf;
        if (HINT && seed != 0 && !hint_node_ok(seed, SV().n_real)) seed = 0;   // any table contents: a record of this tree, or none
        // Near-first: a wave query with an active lane, none of them a shadow lane (the host clears
        // the mode where the pruning claim does not hold; the profiling variant wants NF_PROFILE).
        const bool shq = NEAR && __ballot(st == ST_WAIT_SHADOW && qa);   // (uniform) a shadow wave query
        bool nfq = false;
        if (NEAR) {
            const int nm = SV().near_first;
            if (PROF ? nm == NF_PROFILE : nm != NF_OFF) nfq = __ballot(qa) && !shq;
        }
        // One walk per query kind (closest_hit): any shadow lane sends the wave to the shadow walk.
        bool hit;
        if constexpr (HINT) {
            if (shq) hit = closest_hit<false, STATS, FT, AXIS, PROF, BRUTE, QK_SHADOW>(SV(), bv, qa, q, b, wc, occl, lim,
                                                                                     -1.0f, seed, hslot);
            else hit = closest_hit<false, STATS, FT, AXIS, PROF, BRUTE, QK_NORMAL>(SV(), bv, qa, q, b, wc, -1.0f, INFINITY,
                                                                                   -1.0f, 0, nullptr, nfq);
        } else
            hit = closest_hit<false, STATS, FT, AXIS, PROF, BRUTE, NEAR ? QK_NEAR : QK_ANY>(SV(), bv, qa, q, b, wc, occl, lim,
                                                                                            -1.0f, 0, nullptr, nfq);
        if (HINT) {                                            // a normal query's first hit keys the wave's shadow queries
            const unsigned long long hm = __ballot(hit && st == ST_WAIT_NORMAL);
            if (hm) {
                const int hl = __builtin_ctzll(hm);
                hkey = hint_key(__builtin_amdgcn_readlane(b.inst, hl), __builtin_amdgcn_readlane(b.tri, hl));
            }
        }
        if (PROF && P.stats) {                                 // query occupancy (rt_frame_work)
            const unsigned long long mp = __ballot(st == ST_WAIT_NORMAL && (fl & 1));
            const unsigned long long mn = __ballot(st == ST_WAIT_NORMAL);
            const unsigned long long ms = __ballot(st == ST_WAIT_SHADOW && qa);
            const unsigned long long mu = __ballot(st == ST_WAIT_SHADOW && !qa);
            const int na = __popcll(mn | ms);
            if (lane_id_fresh() == 0) {
                unsigned long long* pc = wc.pc - PROF_LANES_PRIMARY;     // index by the d_stats slot
                pc[PROF_LANES_PRIMARY] += (unsigned long long)__popcll(mp);
                pc[PROF_LANES_SECONDARY] += (unsigned long long)__popcll(mn & ~mp);
                pc[PROF_LANES_SHADOW] += (unsigned long long)__popcll(ms);
                pc[PROF_LANES_UNLIT] += (unsigned long long)__popcll(mu);
                if (wc.live && na > 0) {
                    const int bk = (na - 1) >> 3;
                    pc[PROF_LIVE_WQ] += 1ull;
                    pc[PROF_LIVE_LANES] += (unsigned long long)na;
                    pc[PROF_HIST_WQ + bk] += 1ull;
                    pc[PROF_HIST_PAIR + bk] += wc.wpair - prof_p0;
                    pc[PROF_HIST_LEAF + bk] += wc.wleaf - prof_l0;
                }
            }
        }
        const unsigned long long cq1 = PROF ? __builtin_amdgcn_s_memtime() : 0;
        if (PARK) {
            asm volatile("" ::: "memory");
            const float* pk = park;
            int f = 0;
            auto get = [&](float& x) { if (!PART || f < PART_FIELDS) x = pk[f * TRACE_BLOCK_P]; f++; };
            get(cur.ray.o.x); get(cur.ray.o.y); get(cur.ray.o.z);
            get(cur.ray.d.x); get(cur.ray.d.y); get(cur.ray.d.z);
            get(cur.atten.x); get(cur.atten.y); get(cur.atten.z); get(cur.atten.w);
            get(acc.x); get(acc.y); get(acc.z); get(acc.w);
            get(summed.x); get(summed.y); get(summed.z); get(summed.w);
            get(fct.x); get(fct.y); get(fct.z); get(fct.w);
            if (NN) { get(is_nn.x); get(is_nn.y); get(is_nn.z); }
            if (!OPQ) { get(rv.x); get(rv.y); get(rv.z); get(rv.w); }
            if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); wc.cyc_park += __builtin_amdgcn_s_memtime() - cq1; }
        }
        unsigned long long c1 = 0;
        if (STATS || PROF) { c1 = __builtin_amdgcn_s_memtime(); wc.cyc_q += c1 - c0; c_post = c1; }
        if (!need) continue;
        int hmat = 0;
        V3 hn = v3(0, 0, 0);
        // (opaque scenes: a shadow segment needs neither the normal nor the material -- any hit
        // before the light is opaque, light.cu:44-46)
        const unsigned long long cn0 = PROF ? __builtin_amdgcn_s_memtime() : 0;
        if (hit && (!OPQ || st == ST_WAIT_NORMAL)) hn = hit_normal(SV(), bv, b, hmat);
        if (PROF) wc.cyc_normal += __builtin_amdgcn_s_memtime() - cn0;
        if (st == ST_WAIT_NORMAL) {
            if (fl & 1) {
                fl &= ~1;
                if (fl & 8) {                                  // the pixel of group g, recomputed here
                    const int op = group_lane(g).pix;
                    if (P.hit_inst) P.hit_inst[op] = hit ? b.inst : -1;
                    if (P.hit_tri) P.hit_tri[op] = hit ? b.tri : -1;
                }
            }
            if (!hit) {                                            // scene.cu:124-126
                is_time = INFINITY;
                pop();
                st = top >= 0 ? ST_ADVANCE : ST_DONE;
                continue;
            }
            is_time = b.time; is_norm = hn; is_mat = hmat;
            if (NN) is_nn = normalized_vote(hn);                   // hit_normal's fast arm returns a unit vector
            if (TEX) is_kd = hit_kd(P, bv, b, hmat);
            fl &= ~4;                                              // hit point / normal = at(ray, is_time), is_norm
            if (cur.depth > 0) {                                   // scene.cu:109-121
                if (!OPQ && cur.in_obj) {
                    const V4 kt = bv.mats[is_mat].Kt;               // trans_atten (scene.cu:14-22): time^Kt
                    cur.atten = cur.atten * v4(pow_fast(is_time, kt.x), pow_fast(is_time, kt.y),
                                               pow_fast(is_time, kt.z), pow_fast(is_time, kt.w));
                }
                cur.type = F_REFLECT;
                cur.last_mat = is_mat;
            } else {
                fl |= 2;                                           // popped after illumination (frame still needed)
            }
            const DMat& m = bv.mats[is_mat];                       // org_light (phong.cu:36-39)
            summed = m.Ke + m.Ka * kld(P.ambience);
            li = 0;
            st = ST_LIGHT;
            continue;
        }
        // ST_WAIT_SHADOW: one shadow segment (light.cu:35-58)
        bool light_done = true;
        if (OPQ && PARK) {                                     // not parked: the light's own colour
            rv = bv.lights[li].col;
        }
        V4 att = rv;
        if (hit && !(b.time > max_t)) {
            const DMat& m = bv.mats[hmat];
            if (OPQ || !m.refractive) {
                att = v4(0, 0, 0, 0);
            } else {
                if (dot(hn, q.d) > 0) {                            // calc_shadow_atten (light.cu:18-25)
                    rv = rv * v4(pow_fast(m.Kt.x, b.time), pow_fast(m.Kt.y, b.time), pow_fast(m.Kt.z, b.time),
                                 pow_fast(m.Kt.w, b.time));
                }
                q = make_ray(at(q, b.time), q.d);
                max_t -= b.time;
                dbg(P, me, 4);
                light_done = false;
            }
        }
        if (light_done) {
            // An unlit light's term is its factor's signed zeros times the light: adding it leaves
            // `summed` as it is unless `summed` is -0, which the host rules out (unlit_skip = 2:
            // no material's Ke + Ka * ambience has a -0 channel, and x + y is -0 only for two -0).
            if (!(max_t == -INFINITY && kparams().unlit_skip == 2)) {
                const V4 inc = (bv.lights[li].type == 0) ? da * att : att;  // PointLight: dist_atten * attenuate()
                summed = summed + fct * inc;                   // phong(): factor x incoming (phong.cu:50-52)
            }
            li++;
            st = ST_LIGHT;
        }
    }
    return acc;
}

// (stage_bvh's LDS image sizes: a16, shade_bytes, lds_bytes, rt_plan.h)
// word copy of n records of T into LDS at `dst` (block-cooperative)
template <class T> __device__ __forceinline__ const T* stage_words(unsigned char* dst, const T* src, int n) {
    static_assert(sizeof(T) % 4 == 0 && alignof(T) <= 16, "word-granular records");
    const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
    const int w = (int)(sizeof(T) / 4) * n;
    for (int i = threadIdx.x; i < w; i += blockDim.x) d32[i] = s32[i];
    return reinterpret_cast<const T*>(dst);
}

// LDS image of a persistent block: node pairs [3n float4] | leaf_inst [n] | inst4 [n_inst]
// (16-B aligned); lds_bytes() on the host must match.
template <bool LDS, bool FT = false, bool SHADE = false, bool BRUTE = false, bool PART = false>
__device__ __forceinline__ BvhRefs stage_bvh(const SceneView& S, unsigned char* smem) {
    BvhRefs bv;
    bv.fnode = S.fnode;
    bv.pair = S.node_pair; bv.leaf = S.leaf_inst; bv.inst = S.inst4;
    bv.mats = S.mats; bv.lights = S.lights; bv.tris = S.tris; bv.meshes = S.meshes;
    if (LDS && SHADE) {                                    // after the BVH image (lds_bytes without the cache)
        unsigned char* p = smem + lds_bytes(S, FT, false, BRUTE, PART);
        bv.mats = stage_words(p, S.mats, S.n_mats);       p += a16(sizeof(DMat) * (size_t)S.n_mats);
        bv.lights = stage_words(p, S.lights, S.n_lights); p += a16(sizeof(DLight) * (size_t)S.n_lights);
        bv.tris = stage_words(p, S.tris, S.n_tris);       p += a16(sizeof(DTri) * (size_t)S.n_tris);
        bv.meshes = stage_words(p, S.meshes, S.n_meshes);
    }
    if (LDS && BRUTE) {                                    // inst4 (no tree)
        float4* in = reinterpret_cast<float4*>(smem);
        for (int i = threadIdx.x; i < S.n_inst; i += blockDim.x) in[i] = S.inst4[i];
        __syncthreads();
        bv.inst = in;
    } else if (LDS && FT && PART) {                        // ordered LBVH (inst4 stays in global memory)
        const int nf = 4 * (S.n_real - 1);
        const float4* src = S.fnode;
        float4* fn = reinterpret_cast<float4*>(smem);
        for (int i = threadIdx.x; i < nf; i += blockDim.x) fn[i] = src[i];
        __syncthreads();
        bv.fnode = fn;
    } else if (LDS && FT) {                                // ordered LBVH | inst4
        const int nf = 4 * (S.n_real - 1);
        const float4* src = S.fnode;
        float4* fn = reinterpret_cast<float4*>(smem);
        float4* in = fn + nf;
        for (int i = threadIdx.x; i < nf; i += blockDim.x) fn[i] = src[i];
        for (int i = threadIdx.x; i < S.n_inst; i += blockDim.x) in[i] = S.inst4[i];
        __syncthreads();
        bv.fnode = fn; bv.inst = in;
    } else if (LDS) {
        const int n3 = 3 * S.n_leaf;
        float4* np = reinterpret_cast<float4*>(smem);
        int* lf = reinterpret_cast<int*>(smem + 16 * (size_t)n3);
        float4* in = reinterpret_cast<float4*>(smem + ((16 * (size_t)n3 + 4 * (size_t)S.n_leaf + 15) & ~(size_t)15));
        for (int i = threadIdx.x; i < n3; i += blockDim.x) np[i] = S.node_pair[i];
        for (int i = threadIdx.x; i < S.n_leaf; i += blockDim.x) lf[i] = S.leaf_inst[i];
        for (int i = threadIdx.x; i < S.n_inst; i += blockDim.x) in[i] = S.inst4[i];
        __syncthreads();
        bv.pair = np; bv.leaf = lf; bv.inst = in;
    }
    return bv;
}

__device__ __forceinline__ V4 shfl4(V4 v, int src) {
    return v4(__shfl(v.x, src), __shfl(v.y, src), __shfl(v.z, src), __shfl(v.w, src));
}

// Persistent blocks (one per CU): the BVH and the instance records are staged in
// LDS once, then every wave repeatedly takes a pixel group from the work counter.
// A group = `px_per_wave` pixels x `lanes_per_px` samples; lane (pixel p, sub s)
// traces samples k = round*L + s and the group leader sums the clamped sample
// radiance in k order (build-defined spp extension).
// MODE: the M_* bits (rt_plan.h, each described there).
template <int NS, bool LDS, int MODE>
__global__ __launch_bounds__(TRACE_BLOCK_P) void trace_kernel(TraceParams P_arg, SceneView S) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    (void)P_arg;                                               // read in place: kparams()
    KTP& P = kparams();
    constexpr bool FT = (MODE & M_FT) != 0, AXIS = (MODE & M_AXIS) != 0;
    constexpr bool SHADE = (MODE & M_SHADE) != 0, BRUTE = (MODE & M_BRUTE) != 0, PART = (MODE & M_PART) != 0;
    static_assert(!(BRUTE && FT), "a brute-force kernel has no tree");
    static_assert(!PART || (FT && (MODE & M_PARK)), "partial parking is a parked ordered-tree kernel");
    const BvhRefs bv = stage_bvh<LDS, FT, SHADE, BRUTE, PART>(S, smem);
    // LDS-staged sample sums (spp >= 16) in the partially parked kernels (config 5's world16 at
    // 64 spp); compiled out of the fully parked headline kernel, whose registers it would crowd
    constexpr bool LSUM = RT_LDS_SUM && PART;
    const int lane = threadIdx.x & 63;
    const int L = P.lanes_per_px;
    constexpr bool MULTI = (MODE & M_MULTI) != 0, STATS = (MODE & M_STATS) != 0, PARK = (MODE & M_PARK) != 0;
    constexpr bool PROF = (MODE & M_PROF) != 0, CYC = STATS || PROF;
    constexpr bool TEX = (MODE & M_TEX) != 0;
    float* park = PARK ? reinterpret_cast<float*>(smem + lds_bytes(S, FT, SHADE, BRUTE, PART)) + threadIdx.x : nullptr;
    const int rounds = MULTI ? (P.spp + L - 1) / L : 1;
    WaveCounters wc{0, 0, 0, 0};
    if (PROF) {                                                // this wave's occupancy counters (zeroed)
        wc.pc = reinterpret_cast<unsigned long long*>(smem + lds_bytes(S, FT, SHADE, BRUTE, PART) +
                                                       (PARK ? (size_t)park_fields(NS) * 4 * TRACE_BLOCK_P : 0)) +
                (threadIdx.x >> 6) * PROF_WAVE_SLOTS;
        if (lane < PROF_WAVE_SLOTS) wc.pc[lane] = 0;
    }
    // Dynamic group assignment over NQ interleaved queues (queue c owns groups g = c + NQ*j):
    // a wave drains its own queue (c = block % NQ, i.e. one per XCD dispatch slot) then the
    // others.  The next ticket is requested one group ahead so the atomic's latency hides
    // behind the current group; a single global counter serialised ~260k atomics (~2.5 ms,
    // measured) and a static split left a 1.5x load-imbalance tail (measured).
    const int q0 = blockIdx.x % NQ;
    const int per_q = (P.n_groups + NQ - 1) / NQ;
    int n_heavy = 0;
    unsigned long long thr = ~0ull, wave_sum = 0;
    if (P.hist == 2) {
        n_heavy = ldc(P.work, WORK_HEAVY_LEN);                 // this frame's heavy live list (sky_kernel)
    } else if (P.hist) {
        n_heavy = (int)min(P.hctl_prev[0], (unsigned long long)P.heavy_cap);
        // heavy: over 4x the previous frame's mean group and over 20 us (2000 ticks of the 100 MHz
        // clock) -- in a frame of uniformly cheap groups the mean-relative test alone flags
        // timing noise, and a long heavy list (one atomic per group) is slower than none
        if (P.hctl_prev[1]) thr = max(4 * P.hctl_prev[1] / (unsigned long long)P.n_groups, 2000ull);
    }
    int qi = n_heavy > 0 ? -1 : 0;                           // -1: the previous frame's heavy groups first
    // Lane 0 holds the raw result of the pending ticket request.  A ticket claims TPC
    // consecutive work indices of its queue (one index in the heavy list); the next one is
    // requested when the batch's last group starts, after that group's own global loads
    // (vmcnt retires in order, so an earlier atomic would hold them up), and read when the
    // batch is used up.  Fewer, batched device-scope atomics: the counters sustain ~100 M
    // atomics/s each, which alone bounded a TPC = 1 frame at 0.75 ms (measured, group
    // loop without tracing).
    int pend = 0, inflight = 0;
    auto step_of = [&](int q) { return q < 0 ? 1 : kparams().tpc; };
#if RT_HEAVY_STATIC
    // A frame issued alone (heavy_static: every block starts at once) deals the heavy list out
    // statically, wave w taking tickets w, w + W, w + 2W, ... with no atomic: otherwise the
    // grid's 4096 waves all queue on the one heavy counter before their first group (~100 M
    // atomics/s: ~40 us).  Lone trace 0.768 -> 0.702 ms (profiles/r04/ab_hs2.log).  Frames that
    // overlap others keep the counter: their blocks start as CUs free up, and a late block's
    // static share became the tail (pipelined frame +1.9% with it; profiles/r04/ab_hs.log).
    int hnext = (int)blockIdx.x * (TRACE_BLOCK_P / 64) + (int)(threadIdx.x >> 6);   // this wave's next heavy ticket
#endif
    // live lists: tickets [0, 2^k) of a list of n <= 2^k groups visit (t * odd) mod 2^k, a
    // bijection that spreads consecutive tickets over the list (arrival order is roughly
    // raster order, where expensive regions cluster); indices >= n are skipped
    auto live_n = [&](int q) { return ldc(kparams().work, 16 * (NQ + 1 + (q0 + q) % NQ)); };
    auto live_span = [&](int q) { const int n = live_n(q); return n <= 1 ? n : 1 << (32 - __builtin_clz((unsigned)n - 1)); };
    auto pow2_span = [](int n) { return n <= 1 ? n : 1 << (32 - __builtin_clz((unsigned)n - 1)); };
    auto request = [&](int q) {
        KTP& Pq = kparams();
        // The address goes through a VGPR so the atomic optimizer leaves the atomic alone:
        // its rewrite waits for the returned value right after issuing it, while the value is
        // needed only when the batch is used up (resolve), groups later.
        unsigned long long a = (unsigned long long)(q < 0 ? &Pq.work[16 * NQ] : &Pq.work[16 * ((q0 + q) % NQ)]);
        asm volatile("" : "+v"(a));
        typedef __attribute__((address_space(1))) int gint;   // keep the global (not flat) atomic
#if RT_HEAVY_STATIC
        if (q < 0 && kparams().heavy_static) { pend = hnext; hnext += kparams().grid_waves; inflight = 1; return; }
#endif
        if (lane == 0) pend = __hip_atomic_fetch_add((gint*)a, step_of(q), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        inflight = 1;
    };
    auto resolve = [&]() { inflight = 0; return __builtin_amdgcn_readfirstlane(pend); };   // all lanes active here
    // one-pixel groups (LSUM kernels, spp >= 64): RGBA results of consecutive pixels buffered one
    // per lane (wbuf), stored as one piece when the run breaks: a 4-B store per pixel-wave left
    // as its own memory-side write (config 5 wrote 20x its frame)
    unsigned wbuf = 0;
    int wbase = 0, wn = 0;                                     // (uniform) first pixel, count
    auto wflush = [&]() {
        if (wn > 0) {
            if (lane_id_fresh() < wn) kparams().rgba[wbase + lane_id_fresh()] = wbuf;
            wn = 0;
        }
    };
    request(qi);
    int tbase = resolve(), j = 0;
    const unsigned long long c_start = CYC ? __builtin_amdgcn_s_memtime() : 0;
    const unsigned long long rt_start = CYC ? __builtin_amdgcn_s_memrealtime() : 0;   // global 100 MHz clock
    for (;;) {
        KTP& P = kparams();                                    // this group's reads of the launch parameters
        for (;;) {                                             // next work index tbase + j of queue qi
            if (qi >= NQ) break;
            const int lim = qi < 0 ? (kparams().hist == 2 ? pow2_span(n_heavy) : n_heavy) : kparams().live ? live_span(qi) : per_q;
            if (tbase + j >= lim) {                             // queue drained (a pending batch is past it too)
                if (inflight) (void)resolve();
                qi++; j = 0;
                if (qi < NQ) { request(qi); tbase = resolve(); }
                continue;
            }
            if (j < step_of(qi)) break;
            if (!inflight) request(qi);                        // batch used up
            tbase = resolve(); j = 0;
        }
        if (qi >= NQ) break;
        const int ticket = tbase + j++;
        const bool last_of_batch = j == step_of(qi);
        // tickets visit the queue's groups in a scrambled order (t * scramble mod per_q, a
        // bijection): expensive image regions are spread over the frame instead of all
        // starting last and leaving a long tail of idle CUs (measured: first wave done at
        // 69% of the kernel span with row order)
        // The scheduling history is read with scalar loads: a vector load here would wait
        // (vmcnt is in order) for the previous group's output stores to be acknowledged.
        auto umod = [&](unsigned n) { return n - udiv(n, kld(P.div_perq)) * (unsigned)per_q; };
        // (the long modulo below is the rare arm: per_q made opaque there, so that the division's
        // float reciprocal of it -- a VGPR -- is formed in that arm, not held across the group loop)
        auto per_q_cold = [&]() { int v = per_q; asm volatile("" : "+s"(v)); return v; };
        auto live_g = [&]() {
            const int n = live_n(qi);
            int i;
            if (LSUM && kparams().tpc > 1) {
                // a ticket's tpc (a power of two) consecutive indices stay consecutive list entries
                // -- neighbouring pixels of one sky block -- and the runs are scrambled, so that a
                // wave stores their results as one wide piece (wstore below)
                const int rl = 31 - __builtin_clz((unsigned)kparams().tpc), span = live_span(qi);
                if (span <= (1 << rl)) i = ticket;
                else i = (int)((((((unsigned)ticket >> rl) * 0x9E3779B1u) & (unsigned)((span >> rl) - 1)) << rl) |
                               ((unsigned)ticket & ((1u << rl) - 1u)));
            } else {
                i = (int)(((unsigned)ticket * 0x9E3779B1u) & (unsigned)(live_span(qi) - 1));
            }
            return i < n ? ldc(P.live, ((q0 + qi) % NQ) * P.live_cap + i) : P.n_groups;
        };
        auto heavy_g = [&]() {                                 // hist = 2: the heavy live list, scrambled
            const int i = (int)(((unsigned)ticket * 0x9E3779B1u) & (unsigned)(pow2_span(n_heavy) - 1));
            return i < n_heavy ? ldc(P.live, NQ * P.live_cap + i) : P.n_groups;
        };
        const int g = qi < 0 ? (P.hist == 2 ? heavy_g() : ldc(P.hl_prev, ticket))
                             : P.live ? live_g()
                             : ((q0 + qi) % NQ) + NQ * (P.scramble_small ? (int)umod((unsigned)ticket * (unsigned)P.scramble)
                                                                         : (int)(((long long)ticket * P.scramble) % per_q_cold()));
        auto flag = [&](const unsigned char* f) { return (ldc(reinterpret_cast<const uint32_t*>(f), g >> 2) >> (8 * (g & 3))) & 0xffu; };
        if (g >= P.n_groups || (qi < 0 && P.hist == 1 && P.gsky && flag(P.gsky)) ||    // sky group: done by sky_kernel
            (qi >= 0 && P.hist == 1 && flag(P.hf_prev)))
            continue;
        const unsigned long long g_start = P.hist == 1 ? __builtin_amdgcn_s_memrealtime() : 0;
        int nq = 0;                                            // wave queries of this group (hist = 2)
        const GroupLane gl = group_lane(g);
        const int sub_g = gl.sub, px = gl.px, py = gl.py;
        const bool valid = gl.valid;
        const bool me = valid && sub_g == 0 && px == P.dbg_x && py == P.dbg_y;   // (no debug pixel with a sample base: launch_trace)
        V4 sum_c = v4(0, 0, 0, 0), sum_r = v4(0, 0, 0, 0);
        float acc = 0.0f;                                      // RT_LDS_SUM: this lane's (pixel, channel) sum
        const unsigned long long g_t0 = CYC ? __builtin_amdgcn_s_memrealtime() : 0, g_q0 = wc.wq;
        const unsigned long long g_p0 = wc.wpair, g_l0 = wc.wleaf, g_r0 = wc.wtri;
        const unsigned long long g_c0 = wc.cyc_q, g_c1 = wc.cyc_leaf, g_c2 = wc.cyc_sample, g_c3 = wc.cyc_post;
        const unsigned long long g_c4 = wc.cyc_light, g_c5 = wc.cyc_normal, g_c6 = wc.cyc_park;
        const unsigned long long g_m0 = CYC ? __builtin_amdgcn_s_memtime() : 0;
        for (int rd = 0; rd < rounds; rd++) {
            const int k = rd * L + sub_g;
            const bool act = valid && k < P.spp;
            Ray r0{v3(0, 0, 0), v3(0, 0, 1)};
            // The frame's sample: k, and in 1-spp launches (L = 1: k = 0) the sample base, which
            // rt_accumulate's passes set.  Read under the uniform branch only (the asm keeps it
            // there): launches of more samples, the headline's among them, pay a scalar compare.
            int kg = k;
            if (L == 1) { kg = kparams().k0; asm volatile("" : "+v"(kg)); }
            if (act) {
                const float2 o = spp_offset_dev(kg);
                DCamera cam = kld(P.cam);
                cam.W = fresh_s(cam.W); cam.H = fresh_s(cam.H); cam.near_ = fresh_s(cam.near_);
                r0 = camera_at(cam, (float)px + o.x, (float)py + o.y);
            }
            if (rd == 0 && last_of_batch) request(qi);         // next ticket, in flight during the trace
            // Whole-group miss (fast kernels): when no lane's primary ray hits a child of the
            // tree's root -- the traversal's first step, same test -- every sample misses, its
            // radiance is the integrator's initial zero (scene.cu:124-126) and the group's
            // outputs are zeros (and -1 hit ids).  Most groups of the reference scenes are sky.
            if (FT && !STATS && !PROF && !MULTI && SV().use_bvh && SV().n_leaf > 0 && !kparams().gsky && !__ballot(ft_root_hit(SV(), bv, act, r0))) {
                if (act && kg == 0) {
                    int gq = g;                                // (the pixel recomputed here: its two store
                    asm volatile("" : "+s"(gq));               // addresses are not held in VGPRs over the group)
                    const int op = group_lane(gq).pix;
                    if (P.hit_inst) P.hit_inst[op] = -1;
                    if (P.hit_tri) P.hit_tri[op] = -1;
                }
                break;                                         // sum_c = sum_r = 0
            }
            // PROF: the group is live when some primary enters the tree's root (the sky pre-pass's
            // test); occupancy counters are taken over live groups' queries only
            if (PROF && FT) wc.live = __ballot(ft_root_hit(SV(), bv, act, r0)) != 0;
            const unsigned long long cs = CYC ? __builtin_amdgcn_s_memtime() : 0;
            V4 c = trace_sample<NS, STATS, PARK, TEX, FT, AXIS, PROF, BRUTE, PART>(S, bv, act, r0, me && rd == 0, act && kg == 0, g, wc,
                                                 park, nq);
            if (CYC) wc.cyc_sample += __builtin_amdgcn_s_memtime() - cs;
            // in-order reduction over samples (ds_bpermute: the LDS pipe has room, the VALU
            // does not -- a DPP row-shift form measured 4% slower).  Each lane clamps its own
            // sample before the exchange (the same bits the leader would compute), and the raw
            // sum is formed only when the radiance output is requested.
            // (lane addresses and sample bounds formed here, after the trace: hoisted above it,
            // they were held across the trace and spilled)
            KTP& Pr = kparams();
            const bool want_r = Pr.radiance != nullptr;
            const int spp_n = Pr.spp;
            const GroupLane ga = group_lane(g);                // after the trace (not held across it)
            const int bb = ga.base, sub_a = ga.sub;
            const V4 cc = rta::clamp1(c);                      // raytracer.cu:37-40 (rt_accum.h)
            if (L == 8) {                               // spp = 8: all permutes in one LDS round trip
                V4 v[8];
#pragma unroll
                for (int s = 0; s < 8; s++) v[s] = shfl4(cc, bb + s);
                if (sub_a == 0)
#pragma unroll
                    for (int s = 0; s < 8; s++)
                        if (rd * L + s < spp_n) sum_c = sum_c + v[s];
                if (want_r) {
#pragma unroll
                    for (int s = 0; s < 8; s++) v[s] = shfl4(c, bb + s);
                    if (sub_a == 0)
#pragma unroll
                        for (int s = 0; s < 8; s++)
                            if (rd * L + s < spp_n) sum_r = sum_r + v[s];
                }
            } else if (LSUM && L >= 16) {
                // spp >= 16 (whole waves, or 16-32 lanes, per pixel): the in-order sums run one per
                // lane and channel through the wave's own parking columns (free between queries),
                // a ds_read and an add per sample, instead of four ds_bpermutes, four adds and the
                // leader's select per sample.  Lane j = (pixel p, channel f): channels 0-3 the
                // clamped colour, 4-7 the raw radiance when requested; the same adds in k order.
                const int ln = lane_id_fresh();                // (not held across the group loop)
                float* wcol = park - ln;                       // the wave's column 0, field 0
                float* mine = park;
                mine[0] = cc.x; mine[TRACE_BLOCK_P] = cc.y; mine[2 * TRACE_BLOCK_P] = cc.z; mine[3 * TRACE_BLOCK_P] = cc.w;
                if (want_r) {
                    mine[4 * TRACE_BLOCK_P] = c.x; mine[5 * TRACE_BLOCK_P] = c.y;
                    mine[6 * TRACE_BLOCK_P] = c.z; mine[7 * TRACE_BLOCK_P] = c.w;
                }
                __builtin_amdgcn_wave_barrier();
                const int nsh = want_r ? 3 : 2;                // log2 of the channels per pixel
                const int pj = ln >> nsh, fj = ln & ((1 << nsh) - 1);
                const int n_s = min(L, spp_n - rd * L);        // samples of this round (uniform)
                if (pj < kparams().px_per_wave) {
                    const float* src = wcol + fj * TRACE_BLOCK_P + pj * L;
                    int s = 0;
                    for (; s + 4 <= n_s; s += 4) {             // 16-B reads (pj * L: a multiple of 16 floats)
                        const float4 v = *reinterpret_cast<const float4*>(src + s);
                        acc = acc + v.x; acc = acc + v.y; acc = acc + v.z; acc = acc + v.w;
                    }
                    for (; s < n_s; s++) acc = acc + src[s];
                }
                __builtin_amdgcn_wave_barrier();
            } else {
                for (int s = 0; s < L; s++) {
                    const V4 v = shfl4(cc, bb + s);
                    if (sub_a == 0 && rd * L + s < spp_n) sum_c = sum_c + v;
                }
                if (want_r)
                    for (int s = 0; s < L; s++) {
                        const V4 v = shfl4(c, bb + s);
                        if (sub_a == 0 && rd * L + s < spp_n) sum_r = sum_r + v;
                    }
            }
        }
        if (LSUM && L >= 16) {                 // the channel sums to their pixel's leader
            const int ln = lane_id_fresh();
            float* wcol = park - ln;
            const int nsh = kparams().radiance != nullptr ? 3 : 2;
            const int pj = ln >> nsh, fj = ln & ((1 << nsh) - 1);
            if (pj < kparams().px_per_wave) wcol[fj * TRACE_BLOCK_P + pj * L] = acc;
            __builtin_amdgcn_wave_barrier();
            const float* mine = park;
            sum_c = v4(mine[0], mine[TRACE_BLOCK_P], mine[2 * TRACE_BLOCK_P], mine[3 * TRACE_BLOCK_P]);
            if (nsh == 3) sum_r = v4(mine[4 * TRACE_BLOCK_P], mine[5 * TRACE_BLOCK_P], mine[6 * TRACE_BLOCK_P], mine[7 * TRACE_BLOCK_P]);
            __builtin_amdgcn_wave_barrier();
        }
        const GroupLane go = group_lane(g);                    // the output pixel, recomputed here
        const bool wide = LSUM && L == 64 && kparams().rgba != nullptr;   // (uniform) buffered RGBA stores
        uint32_t w_enc = 0;
        int w_pix = -1;
        if (go.valid && go.sub == 0) {
            KTP& P = kparams();
            const int p = go.pix;
            const float inv = (float)P.spp;
            // mean = sum / spp and Color's truncation to bytes: rt_accum.h, shared with the fold
            // kernel of rt_accumulate
            auto mean = [&](float x) { return rta::mean(x, P.spp_recip, inv); };
            const uint32_t enc = rta::pack(v4(mean(sum_c.x), mean(sum_c.y), mean(sum_c.z), mean(sum_c.w)));
            if (wide) { w_enc = enc; w_pix = p; }
            else if (P.rgba) P.rgba[p] = enc;
            if (P.radiance) P.radiance[p] = make_float4(mean(sum_r.x), mean(sum_r.y), mean(sum_r.z), mean(sum_r.w));
        }
        if (wide) {                                            // lane 0 is the pixel's leader (L = 64)
            const int pu = __builtin_amdgcn_readlane(w_pix, 0);
            const unsigned eu = (unsigned)__builtin_amdgcn_readlane((int)w_enc, 0);
            if (pu >= 0) {
                if (wn > 0 && (pu != wbase + wn || wn == 64)) wflush();
                if (wn == 0) wbase = pu;
                asm("v_writelane_b32 %0, %1, m0" : "+v"(wbuf) : "s"(eu), "{m0}"(wn));
                wn++;
            }
        }
        if (STATS && P.stats && lane == 0) {                 // profiling: heaviest group (PROF: rt_profile_groups)
            atomicMax(&P.stats[20], __builtin_amdgcn_s_memrealtime() - g_t0);
            atomicMax(&P.stats[21], wc.wq - g_q0);
        }
        if (kparams().hist == 2) {            // heavy by work: the next frame's pre-pass runs it first
            KTP& P = kparams();
            if (nq >= P.heavy_q && lane_id_fresh() == 0) P.hf_next[g] = 1;
        } else if (kparams().hist) {          // record for the next frame's order
            KTP& P = kparams();
            const unsigned long long dur = __builtin_amdgcn_s_memrealtime() - g_start;   // wave-uniform (scalar)
            const bool heavy = dur > thr;
            wave_sum += dur;
            if (lane_id_fresh() == 0) {
            // at most heavy_cap recorded (a few per wave: the list is there to start the frame's
            // longest groups first); a group flagged in hf_next is always in hl_next
            int slot = -1;
            if (heavy) slot = atomicAdd(reinterpret_cast<int*>(P.hctl_next), 1);
            const bool rec = heavy && slot < P.heavy_cap;
            P.hf_next[g] = rec ? 1 : 0;
            if (rec) P.hl_next[slot] = g;
            if (P.gdur) {
                P.gdur[g] = (unsigned)dur;
                if (PROF) {                                    // wave step counts and cycle split of the group
                    unsigned* c = P.gdur + P.n_groups + 12 * (size_t)g;
                    c[0] = (unsigned)(wc.wq - g_q0); c[1] = (unsigned)(wc.wpair - g_p0);
                    c[2] = (unsigned)(wc.wleaf - g_l0); c[3] = (unsigned)(wc.wtri - g_r0);
                    c[4] = (unsigned)(wc.cyc_q - g_c0); c[5] = (unsigned)(wc.cyc_leaf - g_c1);
                    c[6] = (unsigned)(wc.cyc_sample - g_c2); c[7] = (unsigned)(wc.cyc_post - g_c3);
                    c[9] = (unsigned)(wc.cyc_light - g_c4); c[10] = (unsigned)(wc.cyc_normal - g_c5);
                    c[11] = (unsigned)(wc.cyc_park - g_c6);
                    c[8] = (unsigned)(__builtin_amdgcn_s_memtime() - g_m0);
                }
            }
            }
        }
    }
    if (LSUM) wflush();
    if (P.hist == 1 && lane == 0 && wave_sum) atomicAdd(&P.hctl_next[1], wave_sum);
    if (wc.hint && lane == 0) {                                // occluder hints: the wave's counts, after the table
        // (one of HINT_STRIPES copies by block: every wave adding to the same three words queued
        // ~12 k same-address atomics at the kernel's end, +5% on a lone frame's trace)
        unsigned long long* hc = reinterpret_cast<unsigned long long*>(SV().hint + hint_table_ints(SV().n_inst)) +
                                 (blockIdx.x % HINT_STRIPES) * HINT_STRIPE_WORDS;
        for (int i = 0; i < HINT_COUNTERS; i++) {
            const unsigned long long v = (wc.hint >> i * HINT_FIELD_BITS) & ((1ull << HINT_FIELD_BITS) - 1);
            if (v) atomicAdd(&hc[i], v);
        }
    }
    if (wc.nf && lane == 0) {                                  // near-first: the wave's counts, in the same stripes
        unsigned long long* const nc = SV().nf_ctr;
        if (nc)
            for (int i = 0; i < NF_COUNTERS; i++) {
                const unsigned long long v = (wc.nf >> i * NF_FIELD_BITS) & (i == 2 ? ~0ull : (1ull << NF_FIELD_BITS) - 1);
                if (v) atomicAdd(&nc[(blockIdx.x % HINT_STRIPES) * HINT_STRIPE_WORDS + NF_COUNTER0 + i], v);
            }
    }
    if (CYC && P.stats && lane == 0) {
        if (wc.rays) atomicAdd(&P.stats[0], wc.rays);
        if (wc.nodes) atomicAdd(&P.stats[1], wc.nodes);
        if (wc.leaves) atomicAdd(&P.stats[2], wc.leaves);
        if (wc.tris) atomicAdd(&P.stats[3], wc.tris);
        atomicAdd(&P.stats[4], wc.wq); atomicAdd(&P.stats[5], wc.wpair);
        atomicAdd(&P.stats[6], wc.wleaf); atomicAdd(&P.stats[7], wc.wtri);
        atomicAdd(&P.stats[8], wc.cyc_q); atomicAdd(&P.stats[9], wc.cyc_leaf);
        atomicAdd(&P.stats[10], __builtin_amdgcn_s_memtime() - c_start);
        atomicAdd(&P.stats[11], wc.cyc_sample); atomicAdd(&P.stats[12], wc.cyc_post);
        atomicAdd(&P.stats[13], wc.wbary); atomicAdd(&P.stats[14], wc.lbary);
        const unsigned long long rt_end = __builtin_amdgcn_s_memrealtime();
        atomicMin(&P.stats[15], rt_start);                      // kernel span (earliest start, latest end)
        atomicMax(&P.stats[16], rt_end);
        atomicAdd(&P.stats[17], rt_end - rt_start);             // summed wave lifetimes (same clock)
        atomicMax(&P.stats[18], rt_start);                      // latest start / earliest end
        atomicMin(&P.stats[19], rt_end);
        if (PROF)
            for (int i = 0; i < PROF_END - PROF_LANES_PRIMARY; i++)
                if (wc.pc[i]) atomicAdd(&P.stats[PROF_LANES_PRIMARY + i], wc.pc[i]);
    }
}


// Sky pre-pass of the fast frames: one wave per pixel group, the trace kernel's lane mapping
// (lane = pixel x sample), the primary ray of each lane (camera_at, camera.cu:33-42) and the
// traversal's first step on it (ft_root_hit: the same ray_inv, zero-axis cut and pair test on
// the root's children as closest_hit's first iteration).  A group none of whose primaries
// enters the root is a sky group: every sample's query returns no hit, its radiance is the
// integrator's initial zero (scene.cu:124-126), so the group's outputs are written here --
// rgba = the encoding of a zero mean (0), radiance 0, hit ids -1 -- exactly what the trace
// kernel's own whole-group miss test writes, and gsky[g] = 1 tells the trace kernel to skip
// the group.  84% of world8_stress's 1080p groups are sky: in the persistent trace kernel
// each one cost the group loop's whole prologue (ticket, parameter loads, register spills
// and restores around the integrator) -- a lean, high-occupancy kernel does the test
// instead.  The root records are read from global memory (all lanes the same address).
// Group-level sky test: the rays of a group leave the camera position through its pixel
// rectangle [x0, x1] x [y0, y1] (pixels and sample offsets in [0, 1); rows row_step apart
// are covered by their hull), i.e. they lie in the convex cone spanned by the four corner
// directions D(cx, cy) = near f + ((cx - W/2) / unit) r + ((H/2 - cy) / unit) u.  A box
// outside one of the cone's four side half-spaces {x : n . (x - pos) >= 0} meets no ray of
// the group.  Conservative margins: the rectangle grown by 1/64 pixel (the computed rays'
// direction rounding is ~1e-6 rad, 1/64 pixel ~1e-5 rad), the box grown by 1e-4 of its
// coordinate scale, a separation required beyond 1e-5 relative; and the test is only
// trusted when no direction component comes near zero over the rectangle (|D_a| >= 2^-40
// |D|), so every ray of the group takes the geometric slab test (no zero-axis skip and
// no exact-path fallback for tiny components: ray_inv).  A group it does not decide gets
// the exact per-ray root test.
// Brute-force sky test.  In frames without a tree (the reference's -r,
// scene.cu:48-52) every primary ray runs cast_local on every instance, and no box is tested.
// With pure translations and zero mesh offsets (S.prune_abs >= 0) the distance-pruning claim
// (closest_hit) bounds where an accepted hit can lie: a triangle of instance k is accepted at
// world time t only at a point within prune_abs + 2^-13 t of its box (the claim's spatial
// slack plus its time slack).  So when no t >= 0 puts the ray inside the box grown by A + B t
// with A = 2 prune_abs, B = 2^-12 (twice that), no triangle of the instance is accepted.  The
// interval of such t is formed in float: each bound's rounding (a few ulps of the scene radius
// R and of t) is far below what the doubling adds (prune_abs >= 2^-14 R, and 2^-13 t), so an
// interval found empty here is empty under the claim's slack.  Answers "maybe" unless empty.
__device__ __forceinline__ bool grown_box_maybe(float4 lo, float4 hi, float A, float B, const Ray& r) {
    float tl = 0.0f, th = INFINITY;
    auto axis = [&](float l, float h, float o, float d) {
        const float c1 = (l - A) - o, k1 = d + B;            // (d + B) t >= l - A - o
        if (k1 > 0.0f) tl = fmaxf(tl, c1 / k1);
        else if (k1 < 0.0f) th = fminf(th, c1 / k1);
        else if (c1 > 0.0f) tl = INFINITY;
        const float c2 = (h + A) - o, k2 = d - B;            // (d - B) t <= h + A - o
        if (k2 > 0.0f) th = fminf(th, c2 / k2);
        else if (k2 < 0.0f) tl = fmaxf(tl, c2 / k2);
        else if (c2 < 0.0f) tl = INFINITY;
    };
    axis(lo.x, hi.x, r.o.x, r.d.x);
    axis(lo.y, hi.y, r.o.y, r.d.y);
    axis(lo.z, hi.z, r.o.z, r.d.z);
    return !(tl > th);
}

// Brute-force frames (item 30): cone_misses_root's group cone and box test, factored so that
// one cone can be tested against several boxes (cone_misses_root keeps its own inline form: the
// headline's sky kernel measured 1.8% slower in a pipelined frame with this one).  GroupCone:
// the four corner directions, the side planes' normals (pointing inward), the largest
// direction component; ok = 0 when a direction component may come near zero (nothing decided).
struct GroupCone { V3 k[4], n[4]; float dmax; int ok; };
__device__ __forceinline__ GroupCone group_cone(const TraceParams& P, int g) {
    GroupCone gc;
    gc.ok = 0;
    const DCamera& c = P.cam;
    if (!(c.near_ > 0.0f)) return gc;
    const int gy = (int)udiv((unsigned)g, P.div_ngx), gx = g - gy * P.n_gx;
    const int pr0 = gy * P.gh;
    const float e = 1.0f / 64.0f;
    const float x0 = (float)(gx * P.gw) - e, x1 = (float)(gx * P.gw + P.gw) + e;
    const float y0 = (float)(P.row0 + pr0 * P.row_step) - e;
    const float y1 = (float)(P.row0 + (pr0 + P.gh - 1) * P.row_step + 1) + e;
    auto D = [&](float cx, float cy) {
        const float a = (cx - 0.5f * c.W) / c.unit, b = (0.5f * c.H - cy) / c.unit;
        return (c.near_ * c.f + a * c.r) + b * c.u;
    };
    gc.k[0] = D(x0, y0); gc.k[1] = D(x1, y0); gc.k[2] = D(x1, y1); gc.k[3] = D(x0, y1);
    const V3 mid = D(0.5f * (x0 + x1), 0.5f * (y0 + y1));
    auto amax = [](V3 v) { return fmaxf(fabsf(v.x), fmaxf(fabsf(v.y), fabsf(v.z))); };
    gc.dmax = fmaxf(fmaxf(amax(gc.k[0]), amax(gc.k[1])), fmaxf(amax(gc.k[2]), amax(gc.k[3])));
    const float tiny = 0x1p-40f * gc.dmax;
    auto near0 = [&](float a, float b, float cc, float d) {
        return fminf(fminf(a, b), fminf(cc, d)) <= tiny && fmaxf(fmaxf(a, b), fmaxf(cc, d)) >= -tiny;
    };
    const V3* k = gc.k;
    if (near0(k[0].x, k[1].x, k[2].x, k[3].x) || near0(k[0].y, k[1].y, k[2].y, k[3].y) || near0(k[0].z, k[1].z, k[2].z, k[3].z))
        return gc;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        gc.n[i] = cross(k[i], k[(i + 1) & 3]);
        if (dot(gc.n[i], mid) < 0.0f) gc.n[i] = neg(gc.n[i]);
    }
    gc.ok = 1;
    return gc;
}
// Whether no ray of the cone meets box [mn, mx] (nd = 0: a degenerate box, never hit), with
// conservative margins: the box grown by 1e-4 of its coordinate scale, separations beyond the
// rays' rounding (1e-5 relative).
__device__ __forceinline__ bool cone_outside(const GroupCone& gc, V3 pos, V3 mn, V3 mx, bool nd) {
    if (!nd) return true;
    auto amax = [](V3 v) { return fmaxf(fabsf(v.x), fmaxf(fabsf(v.y), fabsf(v.z))); };
    const float m = 1e-4f * (fmaxf(amax(mn), amax(mx)) + amax(pos)) + 1e-30f;
    mn = mn - v3(m, m, m); mx = mx + v3(m, m, m);
    // a box face plane: the apex beyond it and every direction pointing away from it by
    // more than the rounding of the computed rays (1e-5 relative)
    const float away = 1e-5f * gc.dmax;
    const V3* k = gc.k;
    auto face = [&](float o, float lo, float hi, float a0, float a1, float a2, float a3) {
        return (o > hi && fminf(fminf(a0, a1), fminf(a2, a3)) >= away) || (o < lo && fmaxf(fmaxf(a0, a1), fmaxf(a2, a3)) <= -away);
    };
    bool sep = face(pos.x, mn.x, mx.x, k[0].x, k[1].x, k[2].x, k[3].x) || face(pos.y, mn.y, mx.y, k[0].y, k[1].y, k[2].y, k[3].y) ||
               face(pos.z, mn.z, mx.z, k[0].z, k[1].z, k[2].z, k[3].z);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const V3 nn = gc.n[i];
        const V3 q = v3(nn.x >= 0.0f ? mx.x : mn.x, nn.y >= 0.0f ? mx.y : mn.y, nn.z >= 0.0f ? mx.z : mn.z) - pos;
        const float sv = dot(nn, q);
        const float tol = 1e-5f * (fabsf(nn.x) + fabsf(nn.y) + fabsf(nn.z)) * (fabsf(q.x) + fabsf(q.y) + fabsf(q.z));
        sep = sep || sv < -tol;
    }
    return sep;
}
__device__ __forceinline__ bool cone_misses_root(const TraceParams& P, const SceneView& S, int g) {
    const DCamera& c = P.cam;
    if (!(c.near_ > 0.0f) || S.n_real < 2) return false;
    const int gy = (int)udiv((unsigned)g, P.div_ngx), gx = g - gy * P.n_gx;
    const int pr0 = gy * P.gh;
    const float e = 1.0f / 64.0f;
    const float x0 = (float)(gx * P.gw) - e, x1 = (float)(gx * P.gw + P.gw) + e;
    const float y0 = (float)(P.row0 + pr0 * P.row_step) - e;
    const float y1 = (float)(P.row0 + (pr0 + P.gh - 1) * P.row_step + 1) + e;
    auto D = [&](float cx, float cy) {
        const float a = (cx - 0.5f * c.W) / c.unit, b = (0.5f * c.H - cy) / c.unit;
        return (c.near_ * c.f + a * c.r) + b * c.u;
    };
    const V3 k0 = D(x0, y0), k1 = D(x1, y0), k2 = D(x1, y1), k3 = D(x0, y1);
    const V3 mid = D(0.5f * (x0 + x1), 0.5f * (y0 + y1));
    auto amax = [](V3 v) { return fmaxf(fabsf(v.x), fmaxf(fabsf(v.y), fabsf(v.z))); };
    const float dmax = fmaxf(fmaxf(amax(k0), amax(k1)), fmaxf(amax(k2), amax(k3)));
    const float tiny = 0x1p-40f * dmax;
    auto near0 = [&](float a, float b, float cc, float d) {
        return fminf(fminf(a, b), fminf(cc, d)) <= tiny && fmaxf(fmaxf(a, b), fmaxf(cc, d)) >= -tiny;
    };
    if (near0(k0.x, k1.x, k2.x, k3.x) || near0(k0.y, k1.y, k2.y, k3.y) || near0(k0.z, k1.z, k2.z, k3.z)) return false;
    V3 n[4] = {cross(k0, k1), cross(k1, k2), cross(k2, k3), cross(k3, k0)};
#pragma unroll
    for (int i = 0; i < 4; i++) if (dot(n[i], mid) < 0.0f) n[i] = neg(n[i]);
    const float4* rec = S.fnode;                               // the root's two children (pair_hit_at)
    const float4 A = rec[0], B = rec[1], C = rec[2];
    auto outside = [&](V3 mn, V3 mx, bool nd) {
        if (!nd) return true;                                  // degenerate: never hit
        const float m = 1e-4f * (fmaxf(amax(mn), amax(mx)) + amax(c.pos)) + 1e-30f;
        mn = mn - v3(m, m, m); mx = mx + v3(m, m, m);
        // a box face plane: the apex beyond it and every direction pointing away from it by
        // more than the rounding of the computed rays (1e-5 relative)
        const float away = 1e-5f * dmax;
        auto face = [&](float o, float lo, float hi, float a0, float a1, float a2, float a3) {
            return (o > hi && fminf(fminf(a0, a1), fminf(a2, a3)) >= away) || (o < lo && fmaxf(fmaxf(a0, a1), fmaxf(a2, a3)) <= -away);
        };
        bool sep = face(c.pos.x, mn.x, mx.x, k0.x, k1.x, k2.x, k3.x) || face(c.pos.y, mn.y, mx.y, k0.y, k1.y, k2.y, k3.y) ||
                   face(c.pos.z, mn.z, mx.z, k0.z, k1.z, k2.z, k3.z);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const V3 q = v3(n[i].x >= 0.0f ? mx.x : mn.x, n[i].y >= 0.0f ? mx.y : mn.y, n[i].z >= 0.0f ? mx.z : mn.z) - c.pos;
            const float sv = dot(n[i], q);
            const float tol = 1e-5f * (fabsf(n[i].x) + fabsf(n[i].y) + fabsf(n[i].z)) * (fabsf(q.x) + fabsf(q.y) + fabsf(q.z));
            sep = sep || sv < -tol;
        }
        return sep;
    };
    return outside(v3(A.x, A.z, B.x), v3(B.z, C.x, C.z), A.x <= B.z) && outside(v3(A.y, A.w, B.y), v3(B.w, C.y, C.w), A.y <= B.w);
}
// Brute-force frames (item 30): whether no ray of the cone comes within the grown slack of
// any instance box.  A ray meets box k grown by A + B t only at times t <= (F + A) / (1 - B), F the
// distance from the camera to the box's farthest corner, so growing the box by
// G = A + B (F + A) / (1 - B), doubled for rounding, covers every such t.
__device__ __forceinline__ bool cone_misses_boxes(const TraceParams& P, int g, const float4* lo, const float4* hi, int nb,
                                                  float A, float B) {
    const GroupCone gc = group_cone(P, g);
    if (!gc.ok) return false;
    const V3 pos = P.cam.pos;
    for (int k = 0; k < nb; k++) {
        const float4 l = lo[k], h = hi[k];
        if (!(l.x <= h.x)) continue;                           // an empty mesh: never hit
        const V3 far = v3(fmaxf(fabsf(l.x - pos.x), fabsf(h.x - pos.x)), fmaxf(fabsf(l.y - pos.y), fabsf(h.y - pos.y)),
                          fmaxf(fabsf(l.z - pos.z), fabsf(h.z - pos.z)));
        const float F = (far.x + far.y) + far.z;               // >= the farthest corner's distance
        const float G = 2.0f * (A + B * (F + A) / (1.0f - B));
        if (!cone_outside(gc, pos, v3(l.x - G, l.y - G, l.z - G), v3(h.x + G, h.y + G, h.z + G), true)) return false;
    }
    return true;
}

// One block of 4 waves per 64 consecutive groups: wave 0 runs the cone test, one group per
// lane; the block writes the outputs of the groups it decided; the 4 waves share the groups it
// left undecided (exact per-ray test, one group per wave step); the block's live groups are
// appended to list (block % NQ) with one atomic.  Small blocks keep ~8 per CU resident: the
// per-ray tests are latency-bound chains (measured: 1024-group blocks, 102 -> 71 us per
// 1080p frame; per-ray tests of every group, 108 us).
// the heavy-list append runs on threads 64..127 beside the live list's 0..63 (one wave: after it)
constexpr int SKY_HOFF = SKY_THREADS >= 128 ? 64 : 0;
template <bool BRUTE>
// BRUTE: brute-force frames test the instance boxes (mesh box `mbox` + position) grown by
// sky_A + sky_B t instead of a tree's root (grown_box_maybe, cone_misses_boxes)
__global__ __launch_bounds__(SKY_THREADS) void sky_kernel(TraceParams P, SceneView S, unsigned char* gsky, int* live,
                                                          const Box* mbox, float sky_A, float sky_B) {
    __shared__ unsigned long long s_sky, s_todo;
    __shared__ int s_cnt, s_base, s_list[64];
    __shared__ int s_hcnt, s_hbase, s_hlist[64];               // hist = 2: last frame's heavy groups
    // sky_brute: the instance boxes (2 KB); the tree's pass keeps its LDS footprint without them
    struct Boxes { float4 lo[BRUTE ? 64 : 1], hi[BRUTE ? 64 : 1]; };
    __shared__ Boxes s_bx;
    float4* const s_blo = s_bx.lo;
    float4* const s_bhi = s_bx.hi;
    const bool h2 = P.hist == 2;
    constexpr bool brute = BRUTE;
    int nb = 0;
    if (brute) {                                               // (uniform) instance k's box: mesh box + position
        nb = S.n_inst;
        if ((int)threadIdx.x < nb) {
            const float4 I = S.inst4[threadIdx.x];
            const Box mb = mbox[__float_as_int(I.w) & 0x7fffffff];
            s_blo[threadIdx.x] = mb.nd ? make_float4(mb.mn.x + I.x, mb.mn.y + I.y, mb.mn.z + I.z, 0.0f)
                                       : make_float4(INFINITY, INFINITY, INFINITY, 0.0f);   // empty mesh: no hit
            s_bhi[threadIdx.x] = mb.nd ? make_float4(mb.mx.x + I.x, mb.mx.y + I.y, mb.mx.z + I.z, 0.0f)
                                       : make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
        }
        __syncthreads();
    }
    // does ray r (when act) possibly hit anything: the tree's root (the traversal's first step)
    // or, in brute-force frames, some instance's grown box
    auto root_hit = [&](bool act, const Ray& r) {
        if constexpr (!BRUTE) {
            BvhRefs bv{};
            bv.fnode = S.fnode;
            return ft_root_hit(S, bv, act, r);
        }
        if (!act) return false;
        const float A = 2.0f * sky_A, B = sky_B;
        for (int k = 0; k < nb; k++)
            if (s_blo[k].x <= s_bhi[k].x && grown_box_maybe(s_blo[k], s_bhi[k], A, B, r)) return true;
        return false;
    };
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, L = P.lanes_per_px;
    const int base = blockIdx.x * 64;
    const int n_in = min(64, P.n_groups - base);
    if (wv == 0) {
        const int gl = base + lane;
        const bool in = lane < n_in;
        const bool csky = in && (brute ? cone_misses_boxes(P, gl, s_blo, s_bhi, nb, 2.0f * sky_A, sky_B)
                                       : cone_misses_root(P, S, gl));
        // Representative ray: a group the cone test leaves undecided is live as
        // soon as one of its primaries enters the root -- lane 0's (pixel 0, sample 0), the
        // trace kernel's own ray and test -- so only the groups whose representative misses
        // need the 64-ray test below.  One group per lane here.
        bool rlive = false;
        if (in && !csky) {
            const int gy = (int)udiv((unsigned)gl, P.div_ngx), gx = gl - gy * P.n_gx;
            const float2 o = spp_offset_dev(P.k0);
            const Ray rr = camera_at(P.cam, (float)(gx * P.gw) + o.x, (float)(P.row0 + gy * P.gh * P.row_step) + o.y);
            rlive = root_hit(true, rr);
        }
        const unsigned long long m = __ballot(csky), t = __ballot(in && !csky && !rlive);
        if (csky) {
            gsky[gl] = 1;
            // the trace kernel records (hf_next) only the groups it runs: a sky group's entry
            // must not keep a heavy flag from the frame that last wrote this buffer
            if (P.hist == 1) P.hf_next[gl] = 0;
        }
        if (lane == 0) { s_sky = m; s_todo = t; s_cnt = 0; s_hcnt = 0; }
        if (rlive) gsky[gl] = 0;
        // hist = 2: a live group the previous frame found heavy goes on the heavy list instead
        const bool hv = rlive && h2 && P.hf_prev[gl];
        const unsigned long long rl = __ballot(rlive && !hv), hl = __ballot(hv);
        if (rl) {                                              // live already: into the block's list
            const int pos = __popcll(rl & ((1ull << lane) - 1ull));
            if (rlive && !hv) s_list[pos] = gl;
            if (lane == 0) s_cnt = __popcll(rl);
        }
        if (hl) {
            const int pos = __popcll(hl & ((1ull << lane) - 1ull));
            if (hv) s_hlist[pos] = gl;
            if (lane == 0) s_hcnt = __popcll(hl);
        }
    }
    __syncthreads();
    if (h2 && (int)threadIdx.x < n_in) P.hf_next[base + threadIdx.x] = 0;   // this frame records afresh
    auto sky_pixel = [&](int g, int pix) {                     // pixel pix of sky group g: zeros, -1 hit ids
        const int gy = (int)udiv((unsigned)g, P.div_ngx), gx = g - gy * P.n_gx;
        const int qx = P.gw_shift >= 0 ? pix & (P.gw - 1) : pix % P.gw;
        const int qy = P.gw_shift >= 0 ? pix >> P.gw_shift : pix / P.gw;
        const int px = gx * P.gw + qx, pr = gy * P.gh + qy;
        if (!(px < P.W && pr < P.n_rows)) return;
        const int pix_index = P.compact ? pr * P.W + px : (P.row0 + pr * P.row_step) * P.W + px;
        if (P.hit_inst && P.k0 == 0) P.hit_inst[pix_index] = -1;   // (sample 0's hit ids)
        if (P.hit_tri && P.k0 == 0) P.hit_tri[pix_index] = -1;
        if (P.rgba) P.rgba[pix_index] = 0u;                   // to_encoding of Color(0, 0, 0, 0)
        if (P.radiance) P.radiance[pix_index] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    };
    const unsigned long long skym = s_sky;
    if (skym)
        for (int i = threadIdx.x; i < 64 * P.px_per_wave; i += SKY_THREADS) {
            const int gi = i / P.px_per_wave;
            if ((skym >> gi) & 1) sky_pixel(base + gi, i - gi * P.px_per_wave);
        }
    // undecided groups: the exact per-ray root test, waves taking every 4th
    const int pix_g = P.l_shift >= 0 ? lane >> P.l_shift : lane / L;
    const int sub_g = lane - pix_g * L;
    const int pxo = P.gw_shift >= 0 ? pix_g & (P.gw - 1) : pix_g % P.gw;
    const int pyo = P.gw_shift >= 0 ? pix_g >> P.gw_shift : pix_g / P.gw;
    const bool lane_ok = pix_g < P.px_per_wave && sub_g < P.spp;   // k = sub_g (spp <= 64: one round)
    unsigned long long todo = s_todo;
    for (int k = 0; todo; k++) {
        const int bit = __builtin_ctzll(todo);
        todo &= todo - 1;
        if ((k % RT_SKY_WAVES) != wv) continue;
        const int g = base + bit;
        const int gy = (int)udiv((unsigned)g, P.div_ngx), gx = g - gy * P.n_gx;
        const int px = gx * P.gw + pxo, pr = gy * P.gh + pyo;
        const bool valid = pix_g < P.px_per_wave && px < P.W && pr < P.n_rows;
        const int py = P.row0 + pr * P.row_step;
        const bool act = valid && lane_ok;
        Ray r0{v3(0, 0, 0), v3(0, 0, 1)};
        if (act) {
            const float2 o = spp_offset_dev(P.k0 + sub_g);     // the trace kernel's own offsets
            r0 = camera_at(P.cam, (float)px + o.x, (float)py + o.y);
        }
        const bool sky = __ballot(root_hit(act, r0)) == 0;
        if (lane == 0) {
            gsky[g] = sky ? 1 : 0;
            if (sky && P.hist == 1) P.hf_next[g] = 0;
            if (!sky) {
                if (h2 && P.hf_prev[g]) s_hlist[atomicAdd(&s_hcnt, 1)] = g;
                else s_list[atomicAdd(&s_cnt, 1)] = g;
            }
        }
        if (sky && valid && sub_g == 0) sky_pixel(g, pix_g);
    }
    __syncthreads();
    const int q = blockIdx.x % NQ, n = s_cnt, nh = s_hcnt;
    if (n == 0 && nh == 0) return;
    if (threadIdx.x == 0 && n) s_base = atomicAdd(&P.work[16 * (NQ + 1 + q)], n);
    if ((int)threadIdx.x == SKY_HOFF + (SKY_HOFF ? 0 : 1) && nh) s_hbase = atomicAdd(&P.work[WORK_HEAVY_LEN], nh);
    __syncthreads();
    if ((int)threadIdx.x < n) live[q * P.live_cap + s_base + threadIdx.x] = s_list[threadIdx.x];
    if ((int)threadIdx.x >= SKY_HOFF && (int)threadIdx.x < SKY_HOFF + nh)   // heavy list after the NQ lists
        live[NQ * P.live_cap + s_hbase + threadIdx.x - SKY_HOFF] = s_hlist[threadIdx.x - SKY_HOFF];
}

// ---------------------------------------------------------------------------
// Ray queries (rt_query): renv::gpu::cast_ray (scene.cu:42-73) for caller-supplied rays.
// One ray per lane, one wave per 64 consecutive rays (a chunk), the tail lanes of the last
// chunk inactive; waves stride statically over the chunks (small form: one chunk per wave).
// TREE: QT_ORDERED (the ordered LBVH, closest_hit's FT path), QT_HEAP (the reference heap
// walk) or QT_BRUTE (the instance loop).  LDS: the tree and inst4 staged once per block
// (persistent form).  ANY: occlusion query with the early exit.  STATS: the counted reference
// walk (heap, or the instance loop when there is no tree): rt_stats' four counters.
// The scene comes with the camera-ray shortcuts off (prune_abs < 0: no distance pruning, no
// triangle skip; never the axis-plane triangle path): their bounds fold the camera position
// in, and a caller's origin is anywhere.  What stays on is exact for every
// ray: the filtered slab and plane tests with their exact fallbacks, the per-query direction
// chain of identity-pose scenes (dir_pre: a function of the direction only), and the zero-axis
// cut with a slack formed per ray from its own origin (ray_zcut_slack).
// A ray with a non-finite component, or whose direction normalises to zero (rmath::Ray:
// shorter than 1e-5, or too long for its length to be finite), is inactive from the start: it
// reports a miss and takes no part in the wave's ballots.  That test is rtk::caller_ray /
// rtk::ray_traceable (rt_raykey.h), shared with the coherence key.
// ORD (RT_QUERY_ORDER_SORTED, uncounted kernels): lane l of chunk c traces ray order[64 c + l]
// instead of ray 64 c + l, and writes every output at that ray's own index; otherwise the same code.
// ---------------------------------------------------------------------------

// The batch's QueryParams read in place from the kernel-argument segment, through a pointer made
// fresh at each use (kparams' reason: by value, its pointers and the camera were loaded once and
// held in SGPRs across the traversal, and the scalar file overflowed into VGPR lanes).
typedef __attribute__((address_space(4))) const QueryParams KQP;
__device__ __forceinline__ KQP& qparams() {
    KQP* p = (KQP*)__builtin_amdgcn_kernarg_segment_ptr();     // the first kernel argument
    asm volatile("" : "+s"(p));
    return *p;
}

// The zero-axis cut's slack for a ray from `o` (zero_axis_cut; ordered tree, pure translations: zcut_scene >= 0, the
// scene's term), or -1: no cut.  The bound is the camera rays' with this origin in the camera's place: on an axis where
// d_a = 0 the ray keeps its coordinate o_a exactly, world and local, so an accepted point is within the triangle
// tolerance and the origin's rounding of the leaf box there; 4e-4 x the largest vertex coordinate + 2^-14 x (scene
// radius + |o|) is 20x that.  Without it one axis-parallel ray (a frame's centre column, a line of sight along an axis)
// visits every leaf of its row: the 1024-ray batch holding the centre column's end measured 333 us without the cut, 92 us
// with it.  Origins beyond 2^64 (where K x slack leaves the float range) go without.  PARAMS is the
// kernel's accessor, qparams or oparams (plain functions, so each can be a template argument), not zcut_scene by value:
// the term is read in place at each of its two uses as before; with one read the occlusion kernels compiled to other code.
template <auto PARAMS>
__device__ __forceinline__ float ray_zcut_slack(V3 o) {
    float zc = -1.0f;
    if (PARAMS().zcut_scene >= 0.0f) {
        const float oa = fmaxf(fabsf(o.x), fmaxf(fabsf(o.y), fabsf(o.z)));
        if (oa <= 0x1p64f) zc = PARAMS().zcut_scene + 0x1p-14f * oa;
    }
    return zc;
}

template <int TREE, bool LDS, bool ANY, bool STATS, bool ORD = false>
__global__ __launch_bounds__(TRACE_BLOCK_P) void query_kernel(QueryParams Q_arg, SceneView S) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    (void)Q_arg;                                               // read in place: qparams()
    constexpr bool FT = TREE == QT_ORDERED, BRUTE = TREE == QT_BRUTE;
    static_assert(!(STATS && (FT || ANY)), "a counted query is the whole reference walk");
    static_assert(!(STATS && ORD), "a counted query runs in caller order");
    const BvhRefs bv = stage_bvh<LDS, FT, false, BRUTE>(S, smem);
    const int lane = threadIdx.x & 63;
    const int block_waves = (int)(blockDim.x >> 6);
    const long long chunks = (qparams().n + 63) >> 6;
    const long long stride = (long long)gridDim.x * block_waves;
    WaveCounters wc{0, 0, 0, 0};
    for (long long c = (long long)blockIdx.x * block_waves + (long long)(threadIdx.x >> 6); c < chunks; c += stride) {
        const long long slot = c * 64 + lane;
        const bool in = slot < qparams().n;
        const long long i = (ORD && in) ? (long long)qparams().order[slot] : slot;   // the sorted batch: this slot's ray
        Ray r{v3(0, 0, 0), v3(0, 0, 1)};
        bool ok = in;
        // (shade_kernel's lines too: a shared inline function changed both kernels' code, profiles/caller_rays/helper_forms.txt)
        if (in) {
            KQP& Q = qparams();
            if (Q.pixel) {                                     // the camera's sample-0 ray (trace_kernel's primary)
                r = camera_at(kld(Q.cam), (float)Q.pixel[2 * i], (float)Q.pixel[2 * i + 1]);
            } else {
                const V3 o = v3(Q.origin[3 * i], Q.origin[3 * i + 1], Q.origin[3 * i + 2]);
                const V3 d = v3(Q.dir[3 * i], Q.dir[3 * i + 1], Q.dir[3 * i + 2]);
                r = make_ray(o, d);                            // Ray ctor (geometry.h:216)
                ok = rtk::finite3(d);
            }
            // (rtk::caller_ray's value, kept in these two steps: one call per branch measured one
            // VGPR more in every instantiation)
            ok = ok && rtk::ray_traceable(r);
            if (Q.rays_out) {
                float* ro = Q.rays_out + 6 * i;
                ro[0] = r.o.x; ro[1] = r.o.y; ro[2] = r.o.z; ro[3] = r.d.x; ro[4] = r.d.y; ro[5] = r.d.z;
            }
            if (!ok) r = Ray{v3(0, 0, 0), v3(0, 0, 1)};        // nothing non-finite enters the wave's arithmetic
        }
        const float tm = (in && qparams().tmax) ? qparams().tmax[i] : INFINITY;
        // Occlusion early exit: a lane stops at an accepted hit with time <= tm (1 - margin).  Each
        // later accept (at most one per instance: cast_local sets the time once) is below the
        // previous time in its own local units, so it raises the world time by the rescaling's
        // rounding at most (a factor < 1 + 2^-20); `margin` >= n_inst 2^-19 covers the chain, so the
        // closest hit is < tm as well and the boolean is the closest-hit query's.
        float occl = -1.0f;
        if (ANY && qparams().any_margin >= 0.0f && tm > 0.0f) occl = tm * (1.0f - qparams().any_margin);
        Best b;
        b.time = INFINITY; b.inst = -1; b.tri = -1; b.u = 0.0f; b.v = 0.0f;
        const float zc = FT ? ray_zcut_slack<qparams>(r.o) : -1.0f;
        closest_hit<false, STATS, FT, false, false, BRUTE && !STATS>(S, bv, ok, r, b, wc, occl, INFINITY, zc);
        const bool hit = ok && b.time < tm;                    // (nothing accepted: b.time = +inf)
        if (in) {
            KQP& Q = qparams();
            if (Q.hit) Q.hit[i] = hit ? 1 : 0;
            if (!ANY) {                                        // (an early exit leaves b short of the closest hit)
                if (Q.t) Q.t[i] = hit ? b.time : INFINITY;
                if (Q.inst) Q.inst[i] = hit ? b.inst : -1;
                if (Q.tri) Q.tri[i] = hit ? b.tri : -1;
                if (Q.uv) { Q.uv[2 * i] = hit ? b.u : 0.0f; Q.uv[2 * i + 1] = hit ? b.v : 0.0f; }
                if (Q.normal) {
                    V3 nrm = v3(0, 0, 0);
                    int mat = 0;
                    if (hit) nrm = hit_normal(S, bv, b, mat);
                    (void)mat;
                    Q.normal[3 * i] = nrm.x; Q.normal[3 * i + 1] = nrm.y; Q.normal[3 * i + 2] = nrm.z;
                }
            }
        }
    }
    if (STATS && qparams().stats && lane == 0) {
        KQP& Q = qparams();
        if (wc.rays) atomicAdd(&Q.stats[0], wc.rays);
        if (wc.nodes) atomicAdd(&Q.stats[1], wc.nodes);
        if (wc.leaves) atomicAdd(&Q.stats[2], wc.leaves);
        if (wc.tris) atomicAdd(&Q.stats[3], wc.tris);
    }
}

// The coherence keys of a batch (RT_QUERY_ORDER_SORTED): keys[i] = rtk::ray_key of ray i as
// query_kernel traces it (the same caller_ray / camera_at and the same test), idx[i] = i; the
// stable sort of the pairs is the order the ORD kernels read.  One ray per lane.  A lane's
// origin and direction are three dwords 12 bytes apart: a wave's three loads each touch the
// same 768 contiguous bytes, so every fetched line is used whole, and the key and index stores
// are contiguous (8 and 4 bytes a lane).  The box and pointers come as kernel arguments.
constexpr int KEY_BLOCK = 256;
__global__ __launch_bounds__(KEY_BLOCK) void ray_key_kernel(RayBatch Q, rtk::KeyBox box, unsigned long long* __restrict__ keys,
                                                            uint32_t* __restrict__ idx) {
    const long long i = (long long)blockIdx.x * KEY_BLOCK + threadIdx.x;
    if (i >= Q.n) return;
    Ray r;
    bool ok;
    if (Q.pixel) {
        r = camera_at(Q.cam, (float)Q.pixel[2 * i], (float)Q.pixel[2 * i + 1]);
        ok = rtk::ray_traceable(r);
    } else {
        const V3 o = v3(Q.origin[3 * i], Q.origin[3 * i + 1], Q.origin[3 * i + 2]);
        const V3 d = v3(Q.dir[3 * i], Q.dir[3 * i + 1], Q.dir[3 * i + 2]);
        ok = rtk::caller_ray(o, d, r);
    }
    keys[i] = rtk::ray_key(r, ok, box);
    idx[i] = (uint32_t)i;
}

// ---------------------------------------------------------------------------
// Shading caller-supplied rays (rt_shade): the integrator (trace_sample) for rays
// the caller forms, or for the camera's rays of one sample of given pixels.  query_kernel's small
// form: 256-thread blocks, one ray per lane, wave c of the grid takes rays 64 c .. 64 c + 63 (with
// an order: the rays order[64 c .. 64 c + 63]), tail lanes inactive, nothing staged.  The rays are
// formed and accepted as query_kernel forms and accepts them; a rejected ray is inactive from the
// start and its radiance is the integrator's initial zero.  The sample runs unparked and uncounted
// (no LDS, no counters), with the scene as rt_query's (camera-ray shortcuts, hints and near-first
// off), so its radiance is what trace_kernel computes for the same ray.
// trace_sample, hit_kd and dbg read the launch's TraceParams and SceneView in place from the
// kernel-argument segment (kparams(), kscene()): they are this kernel's first two arguments, as
// trace_kernel's, and ShadeParams follows them, read in place as well.
// The order is a wave-uniform run-time branch, not a template parameter (trace_sample is large).
// ---------------------------------------------------------------------------
typedef __attribute__((address_space(4))) const ShadeParams KSP;
static_assert((sizeof(TraceParams) + sizeof(SceneView)) % alignof(ShadeParams) == 0 && sizeof(TraceParams) + sizeof(SceneView) == 552,
              "ShadeParams follows TraceParams and SceneView in the kernarg segment");
__device__ __forceinline__ KSP& sparams() {
    const __attribute__((address_space(4))) char* p =
        (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(KSP*)(p + sizeof(TraceParams) + sizeof(SceneView));   // the third kernel argument
}

template <int NS, int TREE, bool TEX>
__global__ __launch_bounds__(SHADE_BLOCK) void shade_kernel(TraceParams P_arg, SceneView S, ShadeParams Q_arg) {
    (void)P_arg; (void)Q_arg;                                  // read in place: kparams(), sparams()
    constexpr bool FT = TREE == QT_ORDERED, BRUTE = TREE == QT_BRUTE;
    const BvhRefs bv = stage_bvh<false, FT, false, BRUTE>(S, nullptr);
    const int lane = threadIdx.x & 63;
    const long long c = (long long)blockIdx.x * (SHADE_BLOCK / 64) + (long long)(threadIdx.x >> 6);   // this wave's chunk
    const long long slot = c * 64 + lane;
    const bool in = slot < sparams().n;
    long long i = slot;
    if (sparams().order != nullptr && in) i = (long long)sparams().order[slot];   // the sorted batch: this slot's ray
    Ray r{v3(0, 0, 0), v3(0, 0, 1)};
    bool ok = in;
    if (in) {                                                  // (query_kernel's lines, with the sample's offset: see there)
        KSP& Q = sparams();
        if (Q.pixel) {                                         // the camera's ray of sample k (trace_kernel's primary)
            const float2 o = spp_offset_dev(Q.sample);
            r = camera_at(kld(Q.cam), (float)Q.pixel[2 * i] + o.x, (float)Q.pixel[2 * i + 1] + o.y);
        } else {
            const V3 o = v3(Q.origin[3 * i], Q.origin[3 * i + 1], Q.origin[3 * i + 2]);
            const V3 d = v3(Q.dir[3 * i], Q.dir[3 * i + 1], Q.dir[3 * i + 2]);
            r = make_ray(o, d);                                // Ray ctor (geometry.h:216)
            ok = rtk::finite3(d);
        }
        ok = ok && rtk::ray_traceable(r);                      // (rtk::caller_ray's value, as query_kernel)
        if (Q.rays_out) {
            float* ro = Q.rays_out + 6 * i;
            ro[0] = r.o.x; ro[1] = r.o.y; ro[2] = r.o.z; ro[3] = r.d.x; ro[4] = r.d.y; ro[5] = r.d.z;
        }
        if (!ok) r = Ray{v3(0, 0, 0), v3(0, 0, 1)};            // nothing non-finite enters the wave's arithmetic
    }
    WaveCounters wc{0, 0, 0, 0};
    int nq = 0;
    // unparked, uncounted, no axis-plane path, no profiling: one sample per lane, no hit ids, no debug pixel
    const V4 acc = trace_sample<NS, false, false, TEX, FT, false, false, BRUTE, false>(S, bv, ok, r, false, false, 0, wc, nullptr, nq);
    if (in) {
        KSP& Q = sparams();
        long long j = slot;                                    // the ray's own index, read again (not held across the trace)
        if (Q.order != nullptr) j = (long long)Q.order[slot];
        // the 1-spp frame's resolve (rt_accum.h): the sums of one sample, raw and clamped, and their mean
        V4 sum_r = v4(0, 0, 0, 0), sum_c = v4(0, 0, 0, 0);
        rta::fold(sum_r, sum_c, acc);
        if (Q.radiance) {
            const V4 m = rta::resolve_radiance(sum_r, 1);
            Q.radiance[j] = make_float4(m.x, m.y, m.z, m.w);
        }
        if (Q.rgba) Q.rgba[j] = rta::resolve_rgba(sum_c, 1);
    }
}

// ---------------------------------------------------------------------------
// Ambient occlusion (rt_occlusion; rt_occl.h): how much of the hemisphere above
// every pixel's primary hit is unoccluded within a radius.  Three kernels beside the query
// kernels, none of which touches them: the surface record once per accumulation, the occlusion
// rays of a launch's samples, and the test hook that writes one sample's rays out (the last two
// once more for the interleaved pattern), then the filtered resolve.  One pixel
// per lane, 256-thread blocks, nothing staged (the small form of query_kernel); the scene comes
// as rt_query's (camera-ray shortcuts off).  TREE as query_kernel's.
// ---------------------------------------------------------------------------
typedef __attribute__((address_space(4))) const OcclParams KOP;
__device__ __forceinline__ KOP& oparams() {                    // read in place, as qparams()
    KOP* p = (KOP*)__builtin_amdgcn_kernarg_segment_ptr();     // the first kernel argument
    asm volatile("" : "+s"(p));
    return *p;
}
// The pixel (row-major index, or -1: none) of lane `lane` of wave g.  OCCL_MAP_ROW: pixels
// [64 g, 64 g + 64) of the frame; OCCL_MAP_TILE: the 8 x 8 tile g (n_tx tiles a row), lane l its
// pixel (l & 7, l >> 3), clipped to the canvas.  g is wave-uniform: its division is scalar.
__device__ __forceinline__ long long occl_pixel(int map, int W, int H, int g, int lane) {
    if (map == OCCL_MAP_TILE) {
        const int n_tx = (W + 7) >> 3, ty = g / n_tx, tx = g - ty * n_tx;
        const int x = 8 * tx + (lane & 7), y = 8 * ty + (lane >> 3);
        return (x < W && y < H) ? (long long)y * W + x : -1;
    }
    const long long i = (long long)g * 64 + lane;
    return i < (long long)W * H ? i : -1;
}
__device__ __forceinline__ int occl_wave() {
    return __builtin_amdgcn_readfirstlane((int)blockIdx.x * (OCCL_BLOCK / 64) + (int)(threadIdx.x >> 6));
}
// OCCL_MAP_CLASS (the interleaved pattern): wave g takes class c = g & 15 = (cx, cy) of the 32 x 32
// region g >> 4 (n_rx regions a row), lane l the pixel (32 rx + 4 (l & 7) + cx, 32 ry + 4 (l >> 3) + cy),
// clipped to the canvas.  g is wave-uniform: the division by the region count is scalar.
__device__ __forceinline__ long long occl_pixel_class(int W, int H, int g, int lane) {
    const int c = g & 15, rg = g >> 4;
    const int n_rx = (W + 31) >> 5, ry = rg / n_rx, rx = rg - ry * n_rx;
    const int x = 32 * rx + 4 * (lane & 7) + (c & 3), y = 32 * ry + 4 * (lane >> 3) + (c >> 2);
    return (x < W && y < H) ? (long long)y * W + x : -1;
}

// The surface record: pixel i's primary hit as query_kernel's pixel mode finds it (camera_at's
// sample-0 ray, the closest hit with nothing cut but the zero-axis leaves, hit_normal), then
// p = o + t d and the normal faced to the viewer.  surf[2 i] = (p, 1), surf[2 i + 1] = (n, 0);
// a pixel whose primary misses holds zeros.
template <int TREE>
__global__ __launch_bounds__(OCCL_BLOCK) void occl_surface_kernel(OcclParams P_arg, SceneView S) {
    (void)P_arg;
    constexpr bool FT = TREE == QT_ORDERED, BRUTE = TREE == QT_BRUTE;
    const BvhRefs bv = stage_bvh<false, FT, false, BRUTE>(S, nullptr);
    const int g = occl_wave();
    if (g >= oparams().n_waves) return;                        // (wave-uniform)
    const long long i = occl_pixel(oparams().map, oparams().W, oparams().H, g, (int)(threadIdx.x & 63));
    const bool in = i >= 0;
    Ray r{v3(0, 0, 0), v3(0, 0, 1)};
    bool ok = in;
    if (in) {
        const int W = oparams().W, y = (int)(i / W), x = (int)(i - (long long)y * W);
        r = camera_at(kld(oparams().cam), (float)x, (float)y);
        ok = rtk::ray_traceable(r);
        if (!ok) r = Ray{v3(0, 0, 0), v3(0, 0, 1)};
    }
    Best b;
    b.time = INFINITY; b.inst = -1; b.tri = -1; b.u = 0.0f; b.v = 0.0f;
    const float zc = FT ? ray_zcut_slack<oparams>(r.o) : -1.0f;
    WaveCounters wc{0, 0, 0, 0};
    closest_hit<false, false, FT, false, false, BRUTE>(S, bv, ok, r, b, wc, -1.0f, INFINITY, zc);
    if (!in) return;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), c = a;
    if (ok && b.time < INFINITY) {
        int mat = 0;
        const V3 nrm = hit_normal(S, bv, b, mat);
        (void)mat;
        const V3 p = rto::surface_point(r.o, r.d, b.time), n = rto::faced(nrm, r.d);
        a = make_float4(p.x, p.y, p.z, 1.0f);
        c = make_float4(n.x, n.y, n.z, 0.0f);
    }
    float4* surf = oparams().surf;
    surf[2 * i] = a; surf[2 * i + 1] = c;
}

// Samples k0 ... k0 + samples - 1 of every pixel.  The frame (origin p + bias n, t1, t2, n) is
// formed once and stays in registers; per sample the table entry is a scalar load (k is
// wave-uniform), the ray is rmath::Ray(origin, raw direction) as query_kernel makes a caller's,
// and one closest_hit with the occlusion exit answers it as rt_query(any_hit = 1, tmax = radius)
// does: accept THRESH <= t < radius, the same early-exit margin and per-ray zero-axis cut.  A ray
// rt_query would reject counts as not occluded, and so does every sample of a pixel without a
// primary hit.  After the loop one read-modify-write of the count (k0 = 0: the count starts at
// zero and is not read); `resolve` (the call's last launch) writes the outputs for n_total samples.
// No ray goes to memory.
//
// IL: the interleaved pattern (rt_occl.h), a kernel of its own (occlusion_il_kernel) so that the
// shared pattern's compiles to what it was.  Sample k's entry is 16 k + the pixel's class: under
// OCCL_MAP_CLASS the class is the wave's (a scalar load as above), under the other maps it is the
// lane's (a per-lane load; the wave's rays fan out over 16 directions).  Nothing else differs.
template <int TREE, bool IL>
__device__ __forceinline__ void occlusion_samples(const SceneView& S) {
    constexpr bool FT = TREE == QT_ORDERED, BRUTE = TREE == QT_BRUTE;
    const BvhRefs bv = stage_bvh<false, FT, false, BRUTE>(S, nullptr);
    const int g = occl_wave();
    if (g >= oparams().n_waves) return;                        // (wave-uniform)
    const bool by_class = IL && oparams().map == OCCL_MAP_CLASS;   // (wave-uniform)
    const long long i = by_class ? occl_pixel_class(oparams().W, oparams().H, g, (int)(threadIdx.x & 63))
                                 : occl_pixel(oparams().map, oparams().W, oparams().H, g, (int)(threadIdx.x & 63));
    const bool in = i >= 0;
    int cls = 0;                                               // IL: the lane's class (by_class: the wave's, g & 15)
    if (IL && !by_class && in) {
        const int W = oparams().W, y = (int)(i / W), x = (int)(i - (long long)y * W);
        cls = rto::pixel_class(x, y);
    }
    rto::Frame f = rto::make_frame(v3(0, 0, 0), v3(0, 0, 1));
    bool live = false;
    if (in) {
        const float4 a = oparams().surf[2 * i], c = oparams().surf[2 * i + 1];
        live = a.w != 0.0f;
        f = rto::make_frame(v3(a.x, a.y, a.z), v3(c.x, c.y, c.z));
    }
    f.p = rto::ray_origin(f, oparams().bias);                  // every sample's origin
    const float zc = FT ? ray_zcut_slack<oparams>(f.p) : -1.0f;
    int cnt = 0;
    WaveCounters wc{0, 0, 0, 0};
    const int k0 = oparams().k0, k1 = k0 + oparams().samples;
    for (int k = k0; k < k1; k++) {
        V3 dk;
        if (!IL) dk = ldc(oparams().table, k);
        else if (by_class) dk = ldc(oparams().table, rto::interleaved_entry(k, g & 15));
        else dk = oparams().table[rto::interleaved_entry(k, cls)];
        const V3 raw = rto::raw_direction(f, dk);
        Ray r = make_ray(f.p, raw);                            // Ray ctor (geometry.h:216)
        const bool ok = live && rtk::finite3(raw) && rtk::ray_traceable(r);
        if (!ok) r = Ray{v3(0, 0, 0), v3(0, 0, 1)};            // nothing non-finite enters the wave's arithmetic
        const float tm = oparams().radius;
        float occl = -1.0f;
        if (oparams().any_margin >= 0.0f && tm > 0.0f) occl = tm * (1.0f - oparams().any_margin);
        Best b;
        b.time = INFINITY; b.inst = -1; b.tri = -1; b.u = 0.0f; b.v = 0.0f;
        closest_hit<false, false, FT, false, false, BRUTE>(S, bv, ok, r, b, wc, occl, INFINITY, zc);
        cnt += (ok && b.time < tm) ? 1 : 0;
    }
    if (!in) return;
    KOP& P = oparams();
    if (k0 > 0 || P.accumulate) cnt += P.count[i];             // (accumulate: seeded counts, or k0 = 0 after the table's wrap)
    P.count[i] = cnt;
    if (P.resolve) {
        const float vis = rto::visibility(cnt, P.n_total);
        if (P.visibility) P.visibility[i] = vis;
        if (P.occluded) P.occluded[i] = cnt;
        if (P.rgba) P.rgba[i] = rto::grey(vis);
    }
}
template <int TREE>
__global__ __launch_bounds__(OCCL_BLOCK) void occlusion_kernel(OcclParams P_arg, SceneView S) {
    (void)P_arg;
    occlusion_samples<TREE, false>(S);
}
template <int TREE>
__global__ __launch_bounds__(OCCL_BLOCK) void occlusion_il_kernel(OcclParams P_arg, SceneView S) {
    (void)P_arg;
    occlusion_samples<TREE, true>(S);
}

// Test hook (rt_occlusion_rays): sample k0's ray of every pixel as occlusion_kernel forms it,
// origin and RAW direction (before the Ray constructor), zeros where the primary misses.
__global__ __launch_bounds__(OCCL_BLOCK) void occl_rays_kernel(OcclParams P) {
    const long long i = (long long)blockIdx.x * OCCL_BLOCK + threadIdx.x;
    if (i >= (long long)P.W * P.H) return;
    const float4 a = P.surf[2 * i], c = P.surf[2 * i + 1];
    V3 o = v3(0, 0, 0), d = v3(0, 0, 0);
    if (a.w != 0.0f) {
        const rto::Frame f = rto::make_frame(v3(a.x, a.y, a.z), v3(c.x, c.y, c.z));
        o = rto::ray_origin(f, P.bias);
        d = rto::raw_direction(f, P.table[P.k0]);
    }
    float* ro = P.rays + 6 * i;
    ro[0] = o.x; ro[1] = o.y; ro[2] = o.z; ro[3] = d.x; ro[4] = d.y; ro[5] = d.z;
}
// The same in the interleaved pattern: pixel (x, y)'s entry 16 k0 + its class.
__global__ __launch_bounds__(OCCL_BLOCK) void occl_rays_il_kernel(OcclParams P) {
    const long long i = (long long)blockIdx.x * OCCL_BLOCK + threadIdx.x;
    if (i >= (long long)P.W * P.H) return;
    const int y = (int)(i / P.W), x = (int)(i - (long long)y * P.W);
    const float4 a = P.surf[2 * i], c = P.surf[2 * i + 1];
    V3 o = v3(0, 0, 0), d = v3(0, 0, 0);
    if (a.w != 0.0f) {
        const rto::Frame f = rto::make_frame(v3(a.x, a.y, a.z), v3(c.x, c.y, c.z));
        o = rto::ray_origin(f, P.bias);
        d = rto::raw_direction(f, P.table[rto::interleaved_entry(P.k0, rto::pixel_class(x, y))]);
    }
    float* ro = P.rays + 6 * i;
    ro[0] = o.x; ro[1] = o.y; ro[2] = o.z; ro[3] = d.x; ro[4] = d.y; ro[5] = d.z;
}

// The filtered resolve (rt_occlusion_set_filter; rt_occl.h): visibility and rgba of every pixel from
// the counts of the accepted taps among the 16 pixels C + (dx, dy), dx, dy in [-2, 1] -- a window
// that holds each class of the interleaved pattern once.  One lane a pixel, a block a 32 x 8 tile
// (OCCL_FILTER_TX x _TY).  The block stages its pixels' records and counts with the halo (35 x 11
// entries) in LDS once, an array per field: a wave's 64 lanes are two rows of 32 consecutive
// entries, so a tap read is two runs of consecutive dwords (no two lanes of a row on one bank).
// A staged count < 0 means "not live": a pixel outside the canvas or without a primary hit; no tap
// reads outside the canvas.  Reads surf and count, writes visibility and rgba only.
// HIST (history across camera moves): the history weights n_h are staged as
// well, and the denominator is the integer sum of the accepted taps' n_h + n_total in place of
// m n_total.  A form of its own, so that the plain one compiles to what it was.
template <bool HIST>
__global__ __launch_bounds__(OCCL_FILTER_TX * OCCL_FILTER_TY) void occl_filter_kernel(OcclParams P) {
    constexpr int LO = rto::AO_FILTER_LO, HI = rto::AO_FILTER_HI;
    constexpr int SW = OCCL_FILTER_TX + LO + HI, SH = OCCL_FILTER_TY + LO + HI, SN = SW * SH;
    __shared__ float spx[SN], spy[SN], spz[SN], snx[SN], sny[SN], snz[SN];
    __shared__ int scnt[SN];
    __shared__ int swgt[HIST ? SN : 1];
    const int W = P.W, H = P.H;
    const int x0 = (int)blockIdx.x * OCCL_FILTER_TX - LO, y0 = (int)blockIdx.y * OCCL_FILTER_TY - LO;
    for (int e = (int)threadIdx.x; e < SN; e += OCCL_FILTER_TX * OCCL_FILTER_TY) {
        const int sy = e / SW, sx = e - sy * SW, x = x0 + sx, y = y0 + sy;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), c = a;
        int cnt = -1, wgt = 0;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const long long i = (long long)y * W + x;
            a = P.surf[2 * i];
            if (a.w != 0.0f) {
                c = P.surf[2 * i + 1]; cnt = P.count[i];
                if (HIST) wgt = P.weight[i];
            }
        }
        spx[e] = a.x; spy[e] = a.y; spz[e] = a.z; snx[e] = c.x; sny[e] = c.y; snz[e] = c.z; scnt[e] = cnt;
        if (HIST) swgt[e] = wgt;
    }
    __syncthreads();
    const int tx = (int)threadIdx.x % OCCL_FILTER_TX, ty = (int)threadIdx.x / OCCL_FILTER_TX;
    const int x = x0 + LO + tx, y = y0 + LO + ty;
    if (x >= W || y >= H) return;
    const int ce = (ty + LO) * SW + tx + LO;
    float vis = 1.0f;                                          // a centre without a primary hit
    if (scnt[ce] >= 0) {
        const V3 pc = v3(spx[ce], spy[ce], spz[ce]), nc = v3(snx[ce], sny[ce], snz[ce]);
        int sum = scnt[ce], m = 1;                             // the centre tap, unconditionally
        int wsum = HIST ? swgt[ce] : 0;
#pragma unroll
        for (int dy = -LO; dy <= HI; dy++) {
#pragma unroll
            for (int dx = -LO; dx <= HI; dx++) {
                if (dx == 0 && dy == 0) continue;
                const int q = ce + dy * SW + dx, cq = scnt[q];
                if (rto::filter_accept(pc, nc, v3(spx[q], spy[q], spz[q]), v3(snx[q], sny[q], snz[q]), cq >= 0, P.normal_min, P.plane_tol)) {
                    sum += cq; m++;
                    if (HIST) wsum += swgt[q];
                }
            }
        }
        vis = HIST ? rto::filtered_visibility_total(sum, wsum + m * P.n_total) : rto::filtered_visibility(sum, m, P.n_total);
    }
    const long long i = (long long)y * W + x;
    if (P.visibility) P.visibility[i] = vis;
    if (P.rgba) P.rgba[i] = rto::grey(vis);
}

// History across camera moves (rt_occlusion_set_history; rt_occl.h).  The seed:
// one lane a pixel of the NEW frame under the 8 x 8 tile map, so that a wave's sources fall into
// one small neighbourhood of the previous frame.  A lane reads its record (32 B), reprojects its
// point through the previous camera, gathers the source's record (32 B), count and weight and
// writes its seeded count and weight -- zeros without a primary hit or an accepted source.  The
// source index is inside the canvas by rto::reproject's float comparisons (and clamped once more
// in integers before it addresses memory).  No LDS, no atomics.
__global__ __launch_bounds__(OCCL_BLOCK) void occl_reproject_kernel(OcclReprojParams R) {
    const int W = R.W, H = R.H;
    const int g = occl_wave();
    if (g >= ((W + 7) >> 3) * ((H + 7) >> 3)) return;          // (wave-uniform)
    const long long i = occl_pixel(OCCL_MAP_TILE, W, H, g, (int)(threadIdx.x & 63));
    if (i < 0) return;
    int c_h = 0, n_h = 0;
    const float4 a = R.surf[2 * i];
    if (a.w != 0.0f) {
        const float4 c = R.surf[2 * i + 1];
        const V3 p = v3(a.x, a.y, a.z), n = v3(c.x, c.y, c.z);
        int qx = 0, qy = 0;
        if (rto::reproject(p, R.prev_cam, qx, qy) && qx < W && qy < H) {
            const long long q = (long long)qy * W + qx;
            const float4 aq = R.prev_surf[2 * q], cq = R.prev_surf[2 * q + 1];
            if (rto::filter_accept(p, n, v3(aq.x, aq.y, aq.z), v3(cq.x, cq.y, cq.z), aq.w != 0.0f, R.normal_min, R.plane_tol))
                rto::history_seed(R.prev_count[q], R.prev_weight[q] + R.n_prev, R.max_history, c_h, n_h);
        }
    }
    R.count[i] = c_h; R.weight[i] = n_h;
}
// The unfiltered outputs with per-pixel totals: n_total samples since the move over weight + n_total.
// A pixel without a primary hit holds count 0: visibility 1.
__global__ __launch_bounds__(OCCL_BLOCK) void occl_resolve_kernel(OcclParams P) {
    const long long i = (long long)blockIdx.x * OCCL_BLOCK + threadIdx.x;
    if (i >= (long long)P.W * P.H) return;
    const int cnt = P.count[i];
    const float vis = rto::visibility(cnt, P.weight[i] + P.n_total);
    if (P.visibility) P.visibility[i] = vis;
    if (P.occluded) P.occluded[i] = cnt;
    if (P.rgba) P.rgba[i] = rto::grey(vis);
}

// ---------------------------------------------------------------------------
// BVH build: ropt::gpu::BVH::BVH (bvh.cu:74-91) + create_boxes (raytracer.cu:54-74)
// in one workgroup.  Output: heap-ordered nodes[1 .. 2n-1].
// ---------------------------------------------------------------------------
template <bool LDS_TREE>
__global__ __launch_bounds__(1024) void bvh_build_kernel(BvhArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);
    int* idx = reinterpret_cast<int*>(smem + sizeof(unsigned long long) * A.n);
    TreeStore<LDS_TREE> tree;
    if constexpr (LDS_TREE) { tree.f = reinterpret_cast<float*>(smem + 12 * (size_t)A.n); tree.cap = 2 * A.n - 1; }
    else tree.t = A.tree;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int n = A.n;
    for (int i = tid; i < A.n_work; i += nt) A.work[i] = 0;
    if (A.hctl && tid < 2) A.hctl[tid] = 0;

    // instance boxes (create_boxes, raytracer.cu:54-74: from_local of the mesh box) and
    // Morton keys (gen_morton, bvh.cu:20-32); padding is degenerate -> ULONG_MAX
    auto inst_box = [&](int i) { return bvh_inst_box(A, i); };
    for (int i = tid; i < n; i += nt) {
        keys[i] = bvh_key(inst_box(i));
        idx[i] = i;
    }
    __syncthreads();
    // Sort on (key, index): identical order to a stable sort by key (thrust sort_by_key,
    // bvh.cu:86).  Entries [n_inst, n) are padding with key ~0 and the largest indices, so
    // they already sit at their rank; only [0, n_inst) moves.
    const int m = A.n_inst, nch = (m + 63) >> 6;
    bool sorted = false;
    if constexpr (LDS_TREE) {
        if (bvh_rank_sort(n, m, nt)) {
            // Chunked rank sort: wave w sorts entries [64w, 64w + 64) in registers (bitonic
            // network over lanes), then each entry's rank = its lane + its rank in every other
            // sorted chunk (branchless binary search in LDS).  Earlier chunks hold smaller
            // indices, so equal keys count there (<=) and not in later chunks (<).  Three
            // barriers instead of the bitonic network's 20 LDS phases.  The sorted chunks are
            // staged in the tree's LDS region (8 * 64 * nch <= 8n < 28 (2n - 1) bytes).
            unsigned long long* S = reinterpret_cast<unsigned long long*>(smem + 12 * (size_t)n);
            const int lane = tid & 63, c = tid >> 6;
            unsigned long long k = ~0ull;
            int x = tid;
            if (tid < nch * 64) {                                  // whole waves
                if (tid < m) k = keys[tid];
                for (int size = 2; size <= 64; size <<= 1) {
                    const bool up = (lane & size) == 0;
                    for (int st = size >> 1; st > 0; st >>= 1) {
                        const unsigned lo = __shfl_xor((unsigned)k, st), hi = __shfl_xor((unsigned)(k >> 32), st);
                        const unsigned long long pk = ((unsigned long long)hi << 32) | lo;
                        const int px = __shfl_xor(x, st);
                        const bool mine_less = k < pk || (k == pk && x < px);
                        if (mine_less != (((lane & st) == 0) == up)) { k = pk; x = px; }
                    }
                }
                S[tid] = k;
            }
            __syncthreads();
            int pos = lane;
            if (tid < m) {
                for (int cb = 0; cb < nch; cb += 4) {              // four independent searches in flight
                    int p4[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int sp = 32; sp >= 1; sp >>= 1) {
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            const int cc = cb + u;
                            if (cc < nch && cc != c) {
                                const unsigned long long v = S[(cc << 6) + p4[u] + sp - 1];
                                if (cc < c ? v <= k : v < k) p4[u] += sp;
                            }
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int cc = cb + u;
                        if (cc < nch && cc != c) {
                            const unsigned long long v = S[(cc << 6) + 63];
                            pos += p4[u] + (p4[u] == 63 && (cc < c ? v <= k : v < k));
                        }
                    }
                }
            }
            __syncthreads();
            if (tid < m) { keys[pos] = k; idx[pos] = x; }
            __syncthreads();
            sorted = true;
        }
    }
    // bitonic sort on (key, index) otherwise.  Strides >= 64 exchange through the LDS; the
    // strides below 64 of each merge run in registers within the wave (lane ^ stride), one
    // LDS round trip and barrier per merge instead of per stride.
    for (int size = 2; size <= n && !sorted; size <<= 1) {
        int stride = size >> 1;
        for (; stride >= 64 || (n < 64 && stride > 0); stride >>= 1) {
            for (int i = tid; i < n; i += nt) {
                int j = i ^ stride;
                if (j > i) {
                    bool up = (i & size) == 0;
                    unsigned long long ki = keys[i], kj = keys[j];
                    int ii = idx[i], ij = idx[j];
                    bool gt = (ki > kj) || (ki == kj && ii > ij);
                    if (gt == up) { keys[i] = kj; keys[j] = ki; idx[i] = ij; idx[j] = ii; }
                }
            }
            __syncthreads();
        }
        if (stride > 0) {                                      // n >= 64: whole waves in range
            for (int i = tid; i < n; i += nt) {
                unsigned long long k = keys[i];
                int x = idx[i];
                const bool up = (i & size) == 0;
                for (int st = stride; st > 0; st >>= 1) {
                    const unsigned lo = __shfl_xor((unsigned)k, st), hi = __shfl_xor((unsigned)(k >> 32), st);
                    const unsigned long long pk = ((unsigned long long)hi << 32) | lo;
                    const int px = __shfl_xor(x, st);
                    const bool mine_less = k < pk || (k == pk && x < px);
                    if (mine_less != (((i & st) == 0) == up)) { k = pk; x = px; }   // lower lane keeps min iff up
                }
                keys[i] = k; idx[i] = x;
            }
            __syncthreads();
        }
    }
    // reorder (bvh.cu:34-41: the box is recomputed, same arithmetic) and pairwise level
    // merges (bvh.cu:43-61)
    for (int i = tid; i < n; i += nt) tree.put(i, inst_box(idx[i]));
    __syncthreads();
    {
        int lvl = 0, size = n, out = n;
        while (size >= 2) {
            for (int i = tid; i < size / 2; i += nt) tree.put(out + i, merge(tree.get(lvl + 2 * i), tree.get(lvl + 2 * i + 1)));
            __syncthreads();
            lvl += size; out += size / 2; size >>= 1;
        }
    }
    for (int k = tid; k < 2 * n; k += nt) bvh_heap_node(A, idx, tree, k);
    for (int i = tid; i < A.n_real - 1; i += nt) bvh_fnode(A, keys, idx, tree, i);
}

// ---------------------------------------------------------------------------
// Device KAT kernel (test hook): the same inline functions the trace kernel uses.
// ---------------------------------------------------------------------------
__global__ void kat_kernel(int op, int n, const float* a, const float* b, const float* c, float* of, int* oi,
                           unsigned long long* ou) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    auto L3 = [](const float* p) { return v3(p[0], p[1], p[2]); };
    auto S3 = [](float* p, V3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; };
    switch (op) {
        case 0: S3(of + 3 * i, normalized(L3(a + 3 * i))); break;
        case 1: S3(of + 3 * i, cross(L3(a + 3 * i), L3(b + 3 * i))); break;
        case 2: S3(of + 3 * i, reflect(L3(a + 3 * i), L3(b + 3 * i))); break;
        case 3: { bool t; S3(of + 3 * i, refract(L3(a + 3 * i), L3(b + 3 * i), c[2 * i], c[2 * i + 1], t)); oi[i] = t; break; }
        case 4: {
            Q q{a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]};
            Pose e{};  // exercise the same Pose path the kernels use (incl. the identity specialisation)
            e.identity = (__float_as_uint(q.i) == 0u && __float_as_uint(q.j) == 0u && __float_as_uint(q.k) == 0u &&
                          __float_as_uint(q.r) == 0x3f800000u);
            e.tn = qnormalized(q); e.ti = qinverse(q);
            S3(of + 3 * i, vec_to_local(e, L3(b + 3 * i)));
            break;
        }
        case 5: { Q r = qinverse(Q{a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]}); of[4 * i] = r.i; of[4 * i + 1] = r.j; of[4 * i + 2] = r.k; of[4 * i + 3] = r.r; break; }
        case 6: {
            Q r = qmul(Q{a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]}, Q{b[4 * i], b[4 * i + 1], b[4 * i + 2], b[4 * i + 3]});
            of[4 * i] = r.i; of[4 * i + 1] = r.j; of[4 * i + 2] = r.k; of[4 * i + 3] = r.r; break;
        }
        case 7: {
            const float* t = a + 9 * i;
            V3 A = L3(t), B = L3(t + 3), C = L3(t + 6);
            V3 pn = cross(B - A, C - A);
            Ray r = make_ray(L3(b + 6 * i), L3(b + 6 * i + 3));
            float tm = NAN, u = NAN, v = NAN;
            bool h = tri_hit(A, B, C, normalized(pn), len(pn), r, tm, u, v);
            oi[i] = h; of[3 * i] = h ? tm : NAN; of[3 * i + 1] = h ? u : NAN; of[3 * i + 2] = h ? v : NAN;
            break;
        }
        case 8: { Ray r = make_ray(L3(a + 6 * i), L3(a + 6 * i + 3)); S3(of + 6 * i, r.o); S3(of + 6 * i + 3, r.d); break; }
        case 9: ou[i] = z_order(L3(a + 3 * i)); break;
        case 10: { float m[3][3]; to_mat3(Q{a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]}, m);
                   for (int x = 0; x < 9; x++) of[9 * i + x] = m[x / 3][x % 3]; break; }
        case 11: {
            const float* bx = a + 7 * i;
            Ray r = make_ray(L3(b + 6 * i), L3(b + 6 * i + 3));
            oi[i] = bx[6] != 0 && box_hit(L3(bx), L3(bx + 3), r);
            break;
        }
        case 12: of[i] = pow_ref(a[i], b[i]); break;
        case 13: {   // filtered triangle test (best = +inf): must equal the exact test bit for bit
            const float* t = a + 9 * i;
            V3 A = L3(t), B = L3(t + 3), C = L3(t + 6);
            V3 pn = cross(B - A, C - A);
            float area = len(pn);
            Ray r = make_ray(L3(b + 6 * i), L3(b + 6 * i + 3));
            float tm = NAN, u = NAN, v = NAN;
            bool h = tri_accept_f(A, B, C, normalized(pn), area, 1.0f / area, r, INFINITY, tm, u, v);
            oi[i] = h; of[3 * i] = h ? tm : NAN; of[3 * i + 1] = h ? u : NAN; of[3 * i + 2] = h ? v : NAN;
            break;
        }
        case 14: {   // filtered box test
            const float* bx = a + 7 * i;
            Ray r = make_ray(L3(b + 6 * i), L3(b + 6 * i + 3));
            oi[i] = bx[6] != 0 && box_hit_f(L3(bx), L3(bx + 3), r, ray_inv(r));
            break;
        }
        case 18: case 19: {   // box_from_local (create_boxes' from_local) / box_merge (the level merges)
            const float* x = a + 7 * i;
            const float* y = b + 7 * i;
            Box bx; bx.mn = L3(x); bx.mx = L3(x + 3); bx.nd = x[6] != 0;
            Box r;
            if (op == 18) {
                const Q o{y[0], y[1], y[2], y[3]};
                Pose e;
                e.p = L3(y + 4);
                e.identity = __float_as_uint(o.i) == 0u && __float_as_uint(o.j) == 0u && __float_as_uint(o.k) == 0u &&
                             __float_as_uint(o.r) == 0x3f800000u;
                e.tn = qnormalized(o); e.ti = qinverse(o);
                const Q inv = qinverse(o);
                e.fn = qnormalized(inv); e.fi = qinverse(inv);
                r = from_local(bx, e);
            } else {
                Box by; by.mn = L3(y); by.mx = L3(y + 3); by.nd = y[6] != 0;
                r = merge(bx, by);
            }
            S3(of + 6 * i, r.mn); S3(of + 6 * i + 3, r.mx); oi[i] = r.nd ? 1 : 0;
            break;
        }
        case 20: {   // entity pose transforms (cast_local / Hitable::hit pose chain)
            const float* y = a + 7 * i;
            const Q o{y[0], y[1], y[2], y[3]};
            Pose e;
            e.p = L3(y + 4);
            e.identity = __float_as_uint(o.i) == 0u && __float_as_uint(o.j) == 0u && __float_as_uint(o.k) == 0u &&
                         __float_as_uint(o.r) == 0x3f800000u;
            e.tn = qnormalized(o); e.ti = qinverse(o);
            const Q inv = qinverse(o);
            e.fn = qnormalized(inv); e.fi = qinverse(inv);
            const V3 v = L3(b + 3 * i);
            S3(of + 12 * i, point_to_local(e, v)); S3(of + 12 * i + 3, vec_to_local(e, v));
            S3(of + 12 * i + 6, point_from_local(e, v)); S3(of + 12 * i + 9, vec_from_local(e, v));
            break;
        }
        case 16: of[i] = rcp_cr(a[i]); break;                   // device CR reciprocal (rt_math.h)
        case 17: of[i] = sqrt_cr(a[i]); break;                  // device CR sqrt
        case 15: {   // packed child-pair box test (pair_hit): two boxes (mn, mx, nd) x 2 vs one ray
            const float* bx = a + 14 * i;
            float q[12];
            for (int c = 0; c < 2; c++) {
                const float* x = bx + 7 * c;
                const bool nd = x[6] != 0;
                for (int j = 0; j < 3; j++) {
                    q[2 * j + c] = nd ? x[j] : INFINITY;
                    q[6 + 2 * j + c] = nd ? x[3 + j] : -INFINITY;
                }
            }
            const float4 np[3] = {make_float4(q[0], q[1], q[2], q[3]), make_float4(q[4], q[5], q[6], q[7]),
                                  make_float4(q[8], q[9], q[10], q[11])};
            Ray r = make_ray(L3(b + 6 * i), L3(b + 6 * i + 3));
            bool h0, h1;
            float t0, t1;
            pair_hit(np, 0, r, ray_inv(r), true, h0, h1, t0, t1);
            oi[2 * i] = h0; oi[2 * i + 1] = h1;
            break;
        }
        case 21: {   // ray_key (rt_raykey.h): a ray as traced (origin, unit direction) in a box (mn, mx)
            const Ray r{L3(a + 6 * i), L3(a + 6 * i + 3)};
            ou[i] = rtk::ray_key(r, rtk::KeyBox{L3(b + 6 * i), L3(b + 6 * i + 3)});
            break;
        }
        // the shading chains' voted forms (one vote per wave of 64 consecutive elements): the
        // generic functions' bits, whichever arm the wave takes
        case 22: S3(of + 3 * i, normalized_vote(L3(a + 3 * i))); break;
        case 23: { const V3 v = L3(a + 3 * i); len_rcp_vote(dot(v, v), of[2 * i], of[2 * i + 1]); break; }
        case 24: S3(of + 3 * i, reflect_vote(L3(a + 3 * i), L3(b + 3 * i))); break;
        case 25: S3(of + 3 * i, c[i] * normalized_vote(reflect_w(L3(a + 3 * i), L3(b + 3 * i)))); break;   // phong_factor's
        default: break;
    }
}

// ---------------------------------------------------------------------------
// Small kernels of the host runtime's side paths
// ---------------------------------------------------------------------------
// Multi-device frames (rt_multi.cpp): the gathered row-cyclic slices back into frame order.
__global__ __launch_bounds__(256) void unpermute_kernel(const uint32_t* __restrict__ g, uint32_t* __restrict__ out, int W,
                                                        int H, int N, int rows_max) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)W * H) return;
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    out[i] = g[((size_t)(y % N) * rows_max + y / N) * W + x];         // frame row y = slice y % N, row y / N
}

// rt_accumulate's fold: pixel i's running sums take one more sample, the raw radiance `pass`
// of a 1-sample frame (rta::fold), and with `resolve` (uniform: the call's last pass) the frame of
// n_before + 1 samples is written (rta::resolve_*: the trace kernel's mean and truncation).
// n_before = 0: the sums start at zero and are not read (0 + c_0 is still added: -0 becomes +0,
// as in the trace kernel's own sum).  One pixel per lane, every access but the RGBA word 16 bytes
// wide and contiguous over the wave; per pixel 16 B of the pass and 32 B of sums read, 32 B
// written, plus 4 + 16 B resolved: 80 to 100 B, no reuse -- bandwidth-bound.  No LDS, no atomics.
constexpr int FOLD_BLOCK = 256;
__global__ __launch_bounds__(FOLD_BLOCK) void accum_fold_kernel(const float4* __restrict__ pass, float4* __restrict__ sum_r,
                                                                float4* __restrict__ sum_c, int n_px, int n_before, int resolve,
                                                                uint32_t* __restrict__ rgba, float4* __restrict__ radiance) {
    const long long i = (long long)blockIdx.x * FOLD_BLOCK + threadIdx.x;   // (n_px may be within a block of 2^31)
    if (i >= n_px) return;                                                   // the tail block
    const float4 r = pass[i];
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
    if (n_before > 0) { a = sum_r[i]; b = sum_c[i]; }
    V4 sr = v4(a.x, a.y, a.z, a.w), sc = v4(b.x, b.y, b.z, b.w);
    rta::fold(sr, sc, v4(r.x, r.y, r.z, r.w));
    sum_r[i] = make_float4(sr.x, sr.y, sr.z, sr.w);
    sum_c[i] = make_float4(sc.x, sc.y, sc.z, sc.w);
    if (resolve) {
        if (rgba) rgba[i] = rta::resolve_rgba(sc, n_before + 1);
        if (radiance) {
            const V4 m = rta::resolve_radiance(sr, n_before + 1);
            radiance[i] = make_float4(m.x, m.y, m.z, m.w);
        }
    }
}

// ---- rt_accumulate's adaptive mode (rt_adapt.h) ----
// Byte g of a flag array padded to whole dwords, g wave-uniform: a scalar load.
__device__ __forceinline__ unsigned tile_flag(const unsigned char* f, int g) {
    return (ldc(reinterpret_cast<const uint32_t*>(f), g >> 2) >> (8 * (g & 3))) & 0xffu;
}
__device__ __forceinline__ V4 ld_v4(const float4* p, long long i) { const float4 v = p[i]; return v4(v.x, v.y, v.z, v.w); }

// Which tiles have an edge: once per accumulation, after sample 0's fold, from sum_c (= 0 +
// clamp1(r0)).  One wave per tile, one pixel per lane; each lane reads its own sum and its eight
// neighbours' with plain 16-byte loads (the frame is L2-resident and this runs once: a 10 x 10
// LDS halo would save loads the L2 serves and cost a barrier and the partial-tile cases), lanes
// outside the canvas do not vote, lane 0 stores the ballot as a byte.  No atomics.
constexpr int TILE_BLOCK = 256;
__global__ __launch_bounds__(TILE_BLOCK) void accum_edge_kernel(const float4* __restrict__ sum_c, rtad::TileGrid t, float thr,
                                                                unsigned char* __restrict__ need) {
    const int g = __builtin_amdgcn_readfirstlane((int)blockIdx.x * (TILE_BLOCK / 64) + (int)(threadIdx.x >> 6));
    if (g >= rtad::n_tiles(t)) return;
    int x, y;
    const bool in = rtad::tile_lane(t, g, (int)(threadIdx.x & 63), x, y);
    const bool e = in && rtad::edge_pixel(t, x, y, thr, [&](int qx, int qy) { return ld_v4(sum_c, (long long)qy * t.W + qx); });
    const unsigned long long m = __ballot(e);
    if ((threadIdx.x & 63) == 0) need[g] = m ? 1 : 0;
}

// The needed tiles' live lists, in the form sky_kernel leaves them: block b (64 tiles, one per
// lane) ballot-compacts its needed tiles and appends them to list b % NQ with one atomicAdd, so a
// list holds at most live_cap = layout_of(n_groups).live_q entries.  `image` is a WORK_INTS image
// of the work counters (zeroed before: tickets and the heavy length stay zero, the list lengths
// are set here); the host sums the NQ lengths for the count of needed tiles.  The order of a
// list's entries is the order its blocks arrive in: it differs from run to run, as sky_kernel's.
__global__ __launch_bounds__(64) void accum_lists_kernel(const unsigned char* __restrict__ need, int n_tiles, int* __restrict__ live,
                                                         int live_cap, int* __restrict__ image) {
    const int lane = threadIdx.x, g = (int)blockIdx.x * 64 + lane;
    const bool nd = g < n_tiles && need[g] != 0;
    const unsigned long long m = __ballot(nd);
    if (!m) return;
    const int q = blockIdx.x % NQ, n = __popcll(m);
    int base = 0;
    if (lane == 0) base = atomicAdd(&image[16 * (NQ + 1 + q)], n);
    base = __builtin_amdgcn_readfirstlane(base);
    if (nd) live[q * live_cap + base + __popcll(m & ((1ull << lane) - 1ull))] = g;
}

// The fold of a refinement pass (sample k >= 1): one wave per tile over all tiles, need[g] read
// with a scalar load and branched on wave-uniformly.  A tile not needed: nothing without
// `resolve`; with it the sums are read and the 1-sample frame written (resolve_*(sum, 1)) -- the
// pass buffer is not read, no sum is written.  A needed tile: accum_fold_kernel's arithmetic,
// resolved with n_before + 1.  16 bytes per lane, a tile row of 8 pixels a 128-byte piece.
__global__ __launch_bounds__(TILE_BLOCK) void accum_fold_tiles_kernel(const float4* __restrict__ pass, float4* __restrict__ sum_r,
                                                                      float4* __restrict__ sum_c, const unsigned char* __restrict__ need,
                                                                      rtad::TileGrid t, int n_before, int resolve,
                                                                      uint32_t* __restrict__ rgba, float4* __restrict__ radiance) {
    const int g = __builtin_amdgcn_readfirstlane((int)blockIdx.x * (TILE_BLOCK / 64) + (int)(threadIdx.x >> 6));
    if (g >= rtad::n_tiles(t)) return;
    const bool nd = tile_flag(need, g) != 0;
    if (!nd && !resolve) return;
    int x, y;
    if (!rtad::tile_lane(t, g, (int)(threadIdx.x & 63), x, y)) return;
    const long long i = (long long)y * t.W + x;
    V4 sr = ld_v4(sum_r, i), sc = ld_v4(sum_c, i);
    int n = 1;
    if (nd) {
        rta::fold(sr, sc, ld_v4(pass, i));
        sum_r[i] = make_float4(sr.x, sr.y, sr.z, sr.w);
        sum_c[i] = make_float4(sc.x, sc.y, sc.z, sc.w);
        n = n_before + 1;
    }
    if (resolve) {
        if (rgba) rgba[i] = rta::resolve_rgba(sc, n);
        if (radiance) {
            const V4 m = rta::resolve_radiance(sr, n);
            radiance[i] = make_float4(m.x, m.y, m.z, m.w);
        }
    }
}

extern "C" {   // (unmangled names: profiler traces are searched for them, tools/pmc_step.py)
// Profile marker (rt_profile_marker): an empty kernel whose grid (64 x tag threads) tells a
// rocprofv3 trace where a caller's timed region begins and ends (tools/pmc_step.py).
__global__ __launch_bounds__(64) void profile_marker_kernel(int tag) { (void)tag; }

// rt_copy_engines_warm's gate: one wave that holds the copies queued behind it pending until the
// host opens the gate (a flag in coherent host memory) or `max_ticks` of the wall clock pass, so
// that every queued copy finds the engines of the copies before it busy.  Vector loads only.
__global__ __launch_bounds__(64) void copy_gate_kernel(const unsigned* flag, unsigned long long max_ticks) {
    const unsigned long long t0 = wall_clock64();
    while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) == 0u && wall_clock64() - t0 < max_ticks)
        __builtin_amdgcn_s_sleep(32);
}
}  // extern "C"

}  // namespace

// ===========================================================================
// Launch layer (rt_device.h): the only functions that name a kernel
// ===========================================================================
namespace rtd {

size_t scene_image_bytes(const SceneView& S) { return lds_bytes(S, true, true); }

// The trace kernels: every instantiation of trace_kernel is named here, once, and nowhere else.
// trace_variant_key (rt_plan.h) decides which of them a frame gets.
struct TraceEntry { int ns; bool lds; int mode; const void* fn; };
constexpr int NG = MAX_FRAMES - 1;                         // generic frame-stack depth
#define TK(NS, LDS, MODE) TraceEntry{NS, LDS, MODE, (const void*)trace_kernel<NS, LDS, MODE>}
#define TK3(LDS, MODE) TK(0, LDS, MODE), TK(2, LDS, MODE), TK(NG, LDS, MODE)   // one per frame-stack bucket
#define TKG(MODE) TK(NG, false, MODE), TK(NG, true, MODE)                      // generic depth, BVH in HBM / LDS
static const TraceEntry trace_kernels[] = {
    // reference heap traversal: plain, parked
    TK3(false, 0), TK3(true, 0), TK3(true, M_PARK),
    // counted / multi-round frames and the generic textured kernels
    TKG(M_MULTI), TKG(M_STATS), TKG(M_MULTI | M_STATS),
    TKG(M_TEX), TKG(M_TEX | M_MULTI), TKG(M_TEX | M_STATS), TKG(M_TEX | M_MULTI | M_STATS),
    // fast frames (ordered LBVH): unparked, parked, + axis-plane triangles, + PROF, + LDS shading cache
    TK3(true, M_FT), TK3(true, M_PARK | M_FT), TK3(true, M_PARK | M_FT | M_AXIS),
    TK3(true, M_PARK | M_FT | M_AXIS | M_PROF), TK3(true, M_PARK | M_FT | M_AXIS | M_SHADE),
    // textured fast frames: unparked, NS 2 and NG only
    TK(2, true, M_TEX | M_FT), TK(NG, true, M_TEX | M_FT),
    TK(2, true, M_TEX | M_FT | M_AXIS), TK(NG, true, M_TEX | M_FT | M_AXIS),
    // brute-force fast frames
    TK3(true, M_BRUTE | M_PARK | M_SHADE | M_AXIS),
    // partial parking: NS = 0 only
    TK(0, true, M_PARK | M_FT | M_AXIS | M_SHADE | M_PART), TK(0, true, M_PARK | M_FT | M_AXIS | M_SHADE | M_PART | M_TEX),
};
#undef TKG
#undef TK3
#undef TK
static_assert(sizeof trace_kernels / sizeof *trace_kernels == 47, "the trace kernels of the build");

TraceVariant choose_trace_variant(const SceneView& S, int spp, bool tex, bool want_stats, bool prof, int ns) {
    TraceVariant v{};
    static_cast<TraceKey&>(v) = trace_variant_key(S, spp, tex, want_stats, prof, ns, getenv("RT_NO_PART") != nullptr,
                                                  getenv("RT_NO_BRUTE_SKY") != nullptr);
    v.per_cu = 1;
    // AXIS kernels hold no general-pose arm (cast_local): the key asks for one only through
    // S.tri_ax, which view_of sets only when every rotation is the identity
    if ((v.mode & M_AXIS) && !S.ident_all) return v;            // no kernel: the caller reports the key
    for (const TraceEntry& e : trace_kernels)
        if (e.ns == v.ns_bucket && e.lds == v.lds && e.mode == v.mode) v.fn = e.fn;
    if (!v.fn) return v;                                       // no such kernel: the caller reports the key
    if (v.shm > 64 * 1024) (void)hipFuncSetAttribute(v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.shm);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v.per_cu, v.fn, TRACE_BLOCK_P, v.shm) != hipSuccess || v.per_cu < 1)
        v.per_cu = 1;
    return v;
}

// The query kernels (rt_query): every instantiation of query_kernel, named here once.  query_plan
// (rt_plan.h) decides which of them a batch gets.
struct QueryEntry { int tree; bool lds, any_hit, counted, ordered; const void* fn; };
#define QK(TREE, LDS, ANY, STATS) QueryEntry{TREE, LDS, ANY, STATS, false, (const void*)query_kernel<TREE, LDS, ANY, STATS>}
#define QK4(TREE) QK(TREE, false, false, false), QK(TREE, true, false, false), QK(TREE, false, true, false), QK(TREE, true, true, false)
#define QKO(TREE, LDS, ANY) QueryEntry{TREE, LDS, ANY, false, true, (const void*)query_kernel<TREE, LDS, ANY, false, true>}
#define QKO4(TREE) QKO(TREE, false, false), QKO(TREE, true, false), QKO(TREE, false, true), QKO(TREE, true, true)
static const QueryEntry query_kernels[] = {
    QK4(QT_ORDERED), QK4(QT_HEAP), QK4(QT_BRUTE),
    // counted: the reference heap walk, or the reference's instance loop
    QK(QT_HEAP, false, false, true), QK(QT_HEAP, true, false, true),
    QK(QT_BRUTE, false, false, true), QK(QT_BRUTE, true, false, true),
    // ORD: the uncounted kernels over a sorted batch (RT_QUERY_ORDER_SORTED)
    QKO4(QT_ORDERED), QKO4(QT_HEAP), QKO4(QT_BRUTE),
};
#undef QKO4
#undef QKO
#undef QK4
#undef QK
static_assert(sizeof query_kernels / sizeof *query_kernels == 28, "the query kernels of the build");

QueryVariant choose_query_variant(long long n_rays, const SceneView& S, bool any_hit, bool counted, int n_cu, int form,
                                  bool ordered) {
    QueryVariant v{};
    static_cast<QueryKey&>(v) = query_plan(n_rays, S, any_hit, counted, n_cu, form);
    v.ordered = ordered;
    for (const QueryEntry& e : query_kernels)
        if (e.tree == v.tree && e.lds == v.lds && e.any_hit == v.any_hit && e.counted == v.counted && e.ordered == ordered) v.fn = e.fn;
    if (v.fn && v.shm > 64 * 1024) (void)hipFuncSetAttribute(v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.shm);
    return v;
}

hipError_t launch_query_kernel(const QueryVariant& v, QueryParams& Q, SceneView& S, hipStream_t st) {
    void* args[] = {&Q, &S};
    return hipExtLaunchKernel(v.fn, dim3(v.blocks), dim3(v.block), args, v.shm, st, nullptr, nullptr, 0);
}

hipError_t launch_ray_keys(const RayBatch& B, const rtk::KeyBox& box, unsigned long long* keys, uint32_t* idx, hipStream_t st) {
    hipLaunchKernelGGL(ray_key_kernel, dim3((unsigned)((B.n + KEY_BLOCK - 1) / KEY_BLOCK)), dim3(KEY_BLOCK), 0, st, B, box, keys, idx);
    return hipGetLastError();
}

// The shade kernels (rt_shade): every instantiation of shade_kernel, named here once.  shade_plan
// (rt_plan.h) decides which of them a batch gets.
struct ShadeEntry { int ns, tree; bool tex; const void* fn; };
#define SK(NS, TREE, TEX) ShadeEntry{NS, TREE, TEX, (const void*)shade_kernel<NS, TREE, TEX>}
#define SK4(TREE) SK(0, TREE, false), SK(0, TREE, true), SK(NG, TREE, false), SK(NG, TREE, true)
static const ShadeEntry shade_kernels[] = {SK4(QT_ORDERED), SK4(QT_HEAP), SK4(QT_BRUTE)};
#undef SK4
#undef SK
static_assert(sizeof shade_kernels / sizeof *shade_kernels == 12, "the shade kernels of the build");

ShadeVariant choose_shade_variant(long long n_rays, const SceneView& S, int ns, bool tex) {
    ShadeVariant v{};
    static_cast<ShadeKey&>(v) = shade_plan(n_rays, S, ns, tex);
    for (const ShadeEntry& e : shade_kernels)
        if (e.ns == v.ns_bucket && e.tree == v.tree && e.tex == v.tex) v.fn = e.fn;
    return v;
}

hipError_t launch_shade_kernel(const ShadeVariant& v, TraceParams& P, SceneView& S, ShadeParams& Q, hipStream_t st,
                               hipEvent_t e0, hipEvent_t e1) {
    void* args[] = {&P, &S, &Q};
    return hipExtLaunchKernel(v.fn, dim3(v.blocks), dim3(v.block), args, 0, st, e0, e1, 0);
}

hipError_t launch_sky(bool brute, int blocks, TraceParams& P, SceneView& S, unsigned char* gsky, int* live,
                      const Box* mesh_box, float slack_a, float slack_b, hipStream_t st, hipEvent_t e0) {
    void* sargs[] = {&P, &S, &gsky, &live, &mesh_box, &slack_a, &slack_b};
    return hipExtLaunchKernel(brute ? (const void*)sky_kernel<true> : (const void*)sky_kernel<false>, dim3(blocks), dim3(SKY_THREADS), sargs, 0, st, e0, nullptr, 0);
}

hipError_t launch_trace_kernel(const TraceVariant& v, int blocks, TraceParams& P, SceneView& S, hipStream_t st,
                               hipEvent_t e0, hipEvent_t e1) {
    void* args[] = {&P, &S};
    return hipExtLaunchKernel(v.fn, dim3(blocks), dim3(TRACE_BLOCK_P), args, v.shm, st, e0, e1, 0);
}

hipError_t launch_bvh_build(BvhArgs& A, bool lds_tree, size_t lds, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    const void* fn = lds_tree ? (const void*)bvh_build_kernel<true> : (const void*)bvh_build_kernel<false>;
    if (lds > 64 * 1024) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    void* args[] = {&A};
    return hipExtLaunchKernel(fn, dim3(1), dim3(BVH_WG_THREADS), args, lds, st, e0, e1, 0);
}

hipError_t launch_accum_fold(const float4* pass, float4* sum_r, float4* sum_c, int n_px, int n_before, bool resolve,
                             uint32_t* rgba, float4* radiance, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    if (n_px <= 0) return hipSuccess;
    int res = resolve ? 1 : 0;
    void* args[] = {&pass, &sum_r, &sum_c, &n_px, &n_before, &res, &rgba, &radiance};
    return hipExtLaunchKernel((const void*)accum_fold_kernel, dim3((unsigned)((n_px + FOLD_BLOCK - 1) / FOLD_BLOCK)), dim3(FOLD_BLOCK),
                              args, 0, st, e0, e1, 0);
}

hipError_t launch_accum_edge(const float4* sum_c, const rtad::TileGrid& t, float threshold, unsigned char* need, hipStream_t st,
                             hipEvent_t e0, hipEvent_t e1) {
    const int n = rtad::n_tiles(t);
    if (n <= 0) return hipSuccess;
    rtad::TileGrid tg = t;
    void* args[] = {&sum_c, &tg, &threshold, &need};
    return hipExtLaunchKernel((const void*)accum_edge_kernel, dim3((unsigned)((n + TILE_BLOCK / 64 - 1) / (TILE_BLOCK / 64))),
                              dim3(TILE_BLOCK), args, 0, st, e0, e1, 0);
}

hipError_t launch_accum_lists(const unsigned char* need, int n_tiles, int* live, int live_cap, int* image, hipStream_t st,
                              hipEvent_t e0, hipEvent_t e1) {
    if (n_tiles <= 0) return hipSuccess;
    void* args[] = {&need, &n_tiles, &live, &live_cap, &image};
    return hipExtLaunchKernel((const void*)accum_lists_kernel, dim3((unsigned)((n_tiles + 63) / 64)), dim3(64), args, 0, st, e0, e1, 0);
}

hipError_t launch_accum_fold_tiles(const float4* pass, float4* sum_r, float4* sum_c, const unsigned char* need,
                                   const rtad::TileGrid& t, int n_before, bool resolve, uint32_t* rgba, float4* radiance,
                                   hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    const int n = rtad::n_tiles(t);
    if (n <= 0) return hipSuccess;
    rtad::TileGrid tg = t;
    int res = resolve ? 1 : 0;
    void* args[] = {&pass, &sum_r, &sum_c, &need, &tg, &n_before, &res, &rgba, &radiance};
    return hipExtLaunchKernel((const void*)accum_fold_tiles_kernel, dim3((unsigned)((n + TILE_BLOCK / 64 - 1) / (TILE_BLOCK / 64))),
                              dim3(TILE_BLOCK), args, 0, st, e0, e1, 0);
}

// The ambient-occlusion kernels (rt_occlusion): one surface and one occlusion kernel per tree form,
// named here once.  occlusion_plan (rt_plan.h) decides which a call gets.
struct OcclEntry { int tree; const void* surface; const void* occlusion; const void* interleaved; };
#define OCK(TREE) OcclEntry{TREE, (const void*)occl_surface_kernel<TREE>, (const void*)occlusion_kernel<TREE>, (const void*)occlusion_il_kernel<TREE>}
static const OcclEntry occl_kernels[] = {OCK(QT_ORDERED), OCK(QT_HEAP), OCK(QT_BRUTE)};
#undef OCK
static const OcclEntry* occl_entry(int tree) {
    for (const OcclEntry& e : occl_kernels)
        if (e.tree == tree) return &e;
    return nullptr;
}

hipError_t launch_occl_surface(const OcclPlan& plan, OcclParams& P, SceneView& S, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    const OcclEntry* e = occl_entry(plan.tree);
    if (!e) return hipErrorInvalidValue;
    void* args[] = {&P, &S};
    return hipExtLaunchKernel(e->surface, dim3(plan.blocks), dim3(plan.block), args, 0, st, e0, e1, 0);
}

hipError_t launch_occlusion(const OcclPlan& plan, OcclParams& P, SceneView& S, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    const OcclEntry* e = occl_entry(plan.tree);
    if (!e) return hipErrorInvalidValue;
    void* args[] = {&P, &S};
    return hipExtLaunchKernel(plan.pattern == OCCL_PATTERN_INTERLEAVED ? e->interleaved : e->occlusion, dim3(plan.blocks), dim3(plan.block),
                              args, 0, st, e0, e1, 0);
}

hipError_t launch_occl_filter(const OcclPlan& plan, OcclParams& P, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    if ((long long)P.W * P.H <= 0) return hipSuccess;
    void* args[] = {&P};
    return hipExtLaunchKernel((const void*)occl_filter_kernel<false>, dim3(plan.filter_bx, plan.filter_by), dim3(OCCL_FILTER_TX * OCCL_FILTER_TY),
                              args, 0, st, e0, e1, 0);
}

hipError_t launch_occl_filter_history(const OcclPlan& plan, OcclParams& P, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    if ((long long)P.W * P.H <= 0) return hipSuccess;
    void* args[] = {&P};
    return hipExtLaunchKernel((const void*)occl_filter_kernel<true>, dim3(plan.filter_bx, plan.filter_by), dim3(OCCL_FILTER_TX * OCCL_FILTER_TY),
                              args, 0, st, e0, e1, 0);
}

hipError_t launch_occl_reproject(OcclReprojParams& R, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    if ((long long)R.W * R.H <= 0) return hipSuccess;
    const long long waves = (long long)((R.W + 7) / 8) * ((R.H + 7) / 8);
    void* args[] = {&R};
    return hipExtLaunchKernel((const void*)occl_reproject_kernel, dim3((unsigned)((waves + OCCL_BLOCK / 64 - 1) / (OCCL_BLOCK / 64))),
                              dim3(OCCL_BLOCK), args, 0, st, e0, e1, 0);
}

hipError_t launch_occl_resolve(OcclParams& P, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    const long long px = (long long)P.W * P.H;
    if (px <= 0) return hipSuccess;
    void* args[] = {&P};
    return hipExtLaunchKernel((const void*)occl_resolve_kernel, dim3((unsigned)((px + OCCL_BLOCK - 1) / OCCL_BLOCK)), dim3(OCCL_BLOCK),
                              args, 0, st, e0, e1, 0);
}

hipError_t launch_occl_rays(OcclParams& P, hipStream_t st) {
    const long long px = (long long)P.W * P.H;
    if (px <= 0) return hipSuccess;
    void* args[] = {&P};
    return hipExtLaunchKernel(P.pattern == OCCL_PATTERN_INTERLEAVED ? (const void*)occl_rays_il_kernel : (const void*)occl_rays_kernel, dim3((unsigned)((px + OCCL_BLOCK - 1) / OCCL_BLOCK)), dim3(OCCL_BLOCK),
                              args, 0, st, nullptr, nullptr, 0);
}

void launch_unpermute(const uint32_t* g, uint32_t* out, int W, int H, int N, int rows_max, hipStream_t st) {
    const long long px = (long long)W * H;
    hipLaunchKernelGGL(unpermute_kernel, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, st, g, out, W, H, N, rows_max);
}
void launch_profile_marker(int tag, hipStream_t st) {
    hipLaunchKernelGGL(profile_marker_kernel, dim3(tag), dim3(64), 0, st, tag);
}
void launch_copy_gate(const unsigned* flag, unsigned long long max_ticks, hipStream_t st) {
    hipLaunchKernelGGL(copy_gate_kernel, dim3(1), dim3(64), 0, st, flag, max_ticks);
}
void launch_kat(int op, int n, const float* a, const float* b, const float* c, float* of, int* oi, unsigned long long* ou) {
    hipLaunchKernelGGL(kat_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, op, n, a, b, c, of, oi, ou);
}

}  // namespace rtd
