// rt_device.h — what the host runtime (rt_runtime.cpp and the entry families' files) and the
// kernel translation unit (rt_kernels.hip) share: the kernel argument structs, the launch
// geometry the host sizes buffers and grids by, the launch plan (rt_plan.h, included below:
// LDS layout, kernel choice, frame geometry, grid) and the launch layer's declarations.  The
// launch layer is defined at the end of rt_kernels.hip; its functions are the only ones that
// name a kernel, so every kernel is instantiated in that one translation unit.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rt_adapt.h"
#include "rt_bvh.h"
#include "rt_math.h"
#include "rt_occl.h"
#include "rt_raykey.h"
#include "rt_scene.h"

// Tuning parameters (build switches; the A/B logs under profiles/ record the values tried).
#ifndef RT_BLOCK
#define RT_BLOCK 1024
#endif
#ifndef RT_NQ
#define RT_NQ 8
#endif
#ifndef RT_HIST_GROUPS_PER_WAVE
#define RT_HIST_GROUPS_PER_WAVE 12  // longest-first history only at <= this many groups per wave
#endif
#ifndef RT_SMALL_FRAME_GPW
#define RT_SMALL_FRAME_GPW 48       // groups per wave (half grid) below which overlapping frames take a quarter of the CUs
#endif
#ifndef RT_HEAVY_Q_DEFAULT
#define RT_HEAVY_Q_DEFAULT 6        // hist = 2: a group of >= this many wave queries is heavy
#endif
#ifndef RT_HEAVY_STATIC
#define RT_HEAVY_STATIC 1    // frames issued alone: heavy-list tickets assigned statically (trace_kernel)
#endif
#ifndef RT_TPC_WIDE
#define RT_TPC_WIDE 16       // live-list tickets of one-pixel groups (spp >= 64, M_PART): 16 consecutive pixels
#endif
#ifndef RT_LDS_SUM
#define RT_LDS_SUM 1         // spp >= 16 in parked kernels: per-channel in-order sample sums through LDS
#endif
#ifndef RT_TPC
#define RT_TPC 3             // work indices claimed per ticket (trace_kernel's group loop) over all
                             // groups; 3 vs 2: -0.8% world8_stress, -1.3% world8 (profiles/r01/ab_tpc_v33.log)
#endif
#ifndef RT_TPC_LIVE
#define RT_TPC_LIVE 1        // the same over live-group lists (sky pre-pass): ~8x fewer groups per
                             // wave, one per ticket balances them (profiles/r02/sky_live_tpc.log)
#endif
#ifndef RT_SKY_WAVES
#define RT_SKY_WAVES 4       // waves per sky_kernel block (64 groups per block)
#endif

namespace rtd {

constexpr int MAX_FRAMES = 10;           // renv::gpu::MAX_DEPTH (scene.cu:25)
constexpr int BVH_WG_LEAVES = 8192;      // single-workgroup BVH build (LDS keys); above: bvh_build_large
constexpr int TRACE_BLOCK_P = RT_BLOCK;  // persistent block: 16 waves (4 per SIMD, 128-VGPR budget) sharing one LDS BVH copy
constexpr int NQ = RT_NQ;                    // work queues (one per XCD dispatch slot), 64-B apart
// work counters: [16 q] queue q's tickets, [16 NQ] the heavy list's, [16 (NQ + 1 + q)] the
// length of live-group list q (sky_kernel), [16 (2 NQ + 1)] the length of this frame's heavy
// live list (hist = 2)
constexpr int WORK_INTS = 16 * (2 * NQ + 2);
// Statistics / profiling counters (d_stats): [0, 22) rt_stats and the PROF step counts and
// cycle split (rt_experiment), [22, 24) spare, [24, 64) the PROF variant's query-occupancy
// counters (PROF_* below, rt_frame_work).
constexpr int STATS_N = 64;
enum : int {
    PROF_LANES_PRIMARY = 24, PROF_LANES_SECONDARY = 25, PROF_LANES_SHADOW = 26, PROF_LANES_UNLIT = 27,
    PROF_LIVE_WQ = 28, PROF_LIVE_LANES = 29,
    PROF_HIST_WQ = 30,      // [8] live wave queries by active lanes, buckets of 8 (1-8, 9-16, ..., 57-64)
    PROF_HIST_PAIR = 38,    // [8] their child-pair steps
    PROF_HIST_LEAF = 46,    // [8] their leaf visits
    PROF_END = 54
};
constexpr int TPC = RT_TPC;
constexpr int SKY_THREADS = 64 * RT_SKY_WAVES;

// Unsigned division by a launch constant d with host-computed magic numbers (round-up
// method: l = ceil(log2 d), m = floor(2^32 (2^l - d) / d) + 1, q = (t + ((n - t) >> 1)) >> (l - 1),
// t = mulhi(n, m); exact for every 32-bit n; d = 1 passes through).  Wave-uniform operands stay
// on the scalar unit (the compiler's own sequence keeps a VGPR reciprocal live across the
// group loop, which was spilled and reloaded from scratch at every group).
struct UDiv { unsigned m, d; int s; };
__host__ inline UDiv udiv_make(unsigned d) {
    UDiv r{0u, d, 0};
    if (d <= 1) return r;
    int l = 0;
    while ((1ull << l) < d) l++;
    r.m = (unsigned)((((1ull << l) - d) << 32) / d + 1);
    r.s = l - 1;
    return r;
}

struct SceneView {           // read-only scene data (HBM, L2-resident)
    const rt::DTri* __restrict__ tris;
    const rt::DMesh* __restrict__ meshes;
    const rt::DInst* __restrict__ insts;
    const rt::DMat* __restrict__ mats;
    const rt::DLight* __restrict__ lights;
    const float4* node_pair;  // BVH child pairs, heap order (written by bvh_build_kernel), see BvhRefs
    const float4* fnode;      // ordered LBVH of the fast kernel (bvh_build_kernel)
    int n_real, ftree;        // its leaf count; 1 if usable (>= 2 leaves, depth <= 31)
    const int* leaf_inst;
    const float4* inst4;      // compact instance records
    int n_leaf, n_inst, n_lights, use_bvh;
    int n_mats, n_tris, n_meshes;   // record counts (LDS shading cache, M_SHADE)
    int ident_all;            // every instance and mesh rotation is the identity (cube worlds)
    float prune_abs;          // distance-pruning slack M0 (< 0: pruning off), see closest_hit
    const rtm::TriAx* tri_ax; // axis-plane triangle records (fast kernel; null unless ident_all)
    // Shadow-query occluder hints (trace_sample, closest_hit's seed; rt_plan.h: hint_*): the scene's
    // table of HINT_SLOTS entries per instance, then its counters (hint_bytes).  Null: off.
    // Last, so that no field the kernels read in place moves (the kernarg-layout record).
    int* hint;
    // Nearer child first (closest_hit; rt_plan.h: NF_*): the counters' block (the hint counters'
    // stripes, bound whether or not the hints are on; null: not counted) and the mode.  After `hint`,
    // for the same reason.
    unsigned long long* nf_ctr;
    int near_first, nf_pad;
};

struct TraceParams {
    rt::DCamera cam;
    rtm::V3 dist_atten;
    rtm::V4 ambience;
    int W, H, row0, row_step, n_rows, compact, spp, depth;
    float spp_recip;          // 2^-k when spp = 2^k (exact reciprocal), else 0
    int lanes_per_px, px_per_wave, gw, gh, n_gx, n_groups;   // sample-parallel lane mapping
    int l_shift, gw_shift;    // log2(lanes_per_px), log2(gw) when powers of two, else -1
    UDiv div_ngx, div_perq;   // g / n_gx and ticket permutation mod per-queue length
    int scramble;             // ticket -> group permutation factor (coprime with the queue length)
    int scramble_small;       // 1: ticket * scramble < 2^32 for every ticket (32-bit modulo)
    const float2* __restrict__ spp_off;
    uint32_t* rgba;
    float4* radiance;
    int* hit_inst;
    int* hit_tri;
    unsigned long long* stats;
    int* work;                // persistent-wave work counters (zeroed before each launch); work[16 NQ]: heavy list
    // Longest-first scheduling history (fast frames only, hist = 1): the previous frame's
    // heavy groups (hl_prev[0, *hc_prev)) run first and are skipped in the normal queues
    // (hf_prev); this frame records its own into the *_next buffers.  hs_* = summed group
    // durations (100 MHz ticks) for the threshold (4x the mean group).
    int hist, heavy_cap;      // heavy_cap: most heavy groups recorded per frame
    // hist = 2 (whole frames with the sky pre-pass): heavy = a group that took >= heavy_q wave
    // queries (counted, no clock); hf_next[g] = 1 records it, and the next frame's sky pre-pass
    // puts the groups flagged in hf_prev on a heavy live list the trace kernel drains first
    int heavy_q;
    const int* hl_prev; int* hl_next;
    const unsigned char* hf_prev; unsigned char* hf_next;
    const unsigned long long* hctl_prev; unsigned long long* hctl_next;   // {count, sum}
    int occl_exit;            // shadow-ray occlusion early exit (all-opaque scene, no statistics)
    const float4* atlas;      // textured mode: atlas texels, byte / 255 (rt_scene_set_atlas)
    int atlas_w, atlas_h;
    int* dbg_log;             // debug_cast event log (NULL in normal frames)
    int dbg_x, dbg_y;
    unsigned* gdur;           // profiling (rt_profile_groups): per-group duration, 100 MHz ticks; NULL normally
    // Sky pre-pass (sky_kernel, fast frames): gsky[g] = 1 when no primary of group g enters
    // the tree's root -- its outputs are written already and the trace kernel skips it.
    // NULL: no pre-pass (the trace kernel runs the same test itself).
    const unsigned char* gsky;
    // Live-group lists (sky_kernel): queue q's groups are live[q * live_cap + i] for i below
    // work[16 (NQ + 1 + q)], in arrival order.  NULL: queue q's groups are q + NQ j.
    const int* live; int live_cap;
    int tpc;                  // work indices per ticket (normal queues)
    int grid_waves;           // waves of this launch (the heavy list's static rounds)
    int heavy_static;         // 1: heavy-list tickets assigned statically (frames issued alone)
    int unlit_skip;           // fast frames: no shadow segments for a light whose phong factor is zero (1),
                              // and no phong term for it either (2)
    int k0;                   // sample base (rt_accumulate), 1-spp launches only: the launch's one sample is the
                              // frame's sample k0 -- its sub-pixel offset, and whether it is "sample 0" (hit ids;
                              // no debug pixel with k0 > 0); 0 in every other launch
};

// query_kernel's arguments (rt_query): n caller-supplied rays (origin / dir, normalised on the
// device as rmath::Ray does) or the camera's sample-0 rays of n pixels (pixel), and the
// per-ray outputs, each optional.  Device pointers.
struct QueryParams {
    rt::DCamera cam;          // pixel mode: camera_at
    long long n;
    const float* origin; const float* dir;      // [3n]
    const float* tmax;                          // [n] or null (+inf)
    float any_margin;                           // occlusion early exit at time <= tmax (1 - any_margin); < 0: off
    float zcut_scene;                           // zero-axis cut: the scene's part of a ray's slack (+ 2^-14 |o|); < 0: off
    const int* pixel;                           // [2n] (x, y), or null
    float* t; int* inst; int* tri;              // miss: +inf, -1, -1
    float* uv;                                  // [2n]
    float* normal;                              // [3n]
    unsigned char* hit;                         // [n]
    float* rays_out;                            // [6n] origin, normalised direction
    unsigned long long* stats;                  // counted kernels: rays, nodes, leaves, triangle tests
    const uint32_t* order;                      // ORD kernels: lane l of chunk c traces ray order[64 c + l] (a permutation of [0, n))
};

// shade_kernel's third argument (rt_shade), after the TraceParams and the SceneView the integrator
// reads in place: n caller-supplied rays (origin / dir, as QueryParams') or the camera's rays of
// sample `sample` of n pixels, and the per-ray outputs, each optional.  Device pointers.
struct ShadeParams {
    rt::DCamera cam;          // pixel mode: camera_at
    long long n;
    const float* origin; const float* dir;      // [3n]
    const int* pixel;                           // [2n] (x, y), or null
    int sample, pad;                            // pixel mode: the frame's sample k (spp_offset_dev), uniform per call
    float4* radiance;                           // [n] the integrator's unclamped sum (miss, rejected ray: zeros)
    uint32_t* rgba;                             // [n] pack(clamp1(radiance)) (rt_accum.h)
    float* rays_out;                            // [6n] origin, normalised direction
    const uint32_t* order;                      // non-null: lane l of chunk c shades ray order[64 c + l] (a permutation of [0, n))
};

// The rays of a batch as the coherence sort sees them (sort_rays, launch_ray_keys, ray_key_kernel):
// the inputs QueryParams and ShadeParams share, copied from either; the fields mean what theirs do.
struct RayBatch { rt::DCamera cam; long long n; const float* origin; const float* dir; const int* pixel; };

// The ambient-occlusion kernels' arguments (rt_occlusion): occl_surface_kernel (cam -> surf),
// occlusion_kernel (surf, table -> count and, resolving, the outputs) and occl_rays_kernel (the
// test hook: sample k0's rays -> rays); occlusion_il_kernel / occl_rays_il_kernel are theirs in the
// interleaved pattern, and occl_filter_kernel (surf, count -> visibility, rgba) is the filtered
// resolve.  Device pointers.  The tracing kernels read it in place
// (oparams(), as qparams()).
struct OcclParams {
    rt::DCamera cam;
    int W, H;
    int map;                  // OCCL_MAP_* (rt_plan.h): which pixel a wave's lane takes
    int n_waves;              // occlusion_plan's: waves with a pixel
    int k0, samples;          // this launch adds samples k0 ... k0 + samples - 1
    int resolve, n_total;     // 1: write the outputs for the n_total samples held after this launch
    float radius, bias;
    float any_margin, zcut_scene;               // as QueryParams'
    const rtm::V3* table;     // [AO_MAX_SAMPLES] directions (rto::ao_direction)
    float4* surf;             // [2 W H] (p, 1 where the primary hits else 0), (faced n, 0); zeros at a miss
    int* count;               // [W H] occluded samples so far (not read when k0 = 0, unless `accumulate`)
    float* visibility; int* occluded; uint32_t* rgba;   // each may be null
    float* rays;              // occl_rays_kernel: [6 W H]
    int pattern;              // OCCL_PATTERN_* (rt_plan.h): which table entry a pixel's sample k uses
    float normal_min, plane_tol;                // occl_filter_kernel's accept test (rto::filter_accept)
    int accumulate;           // 1: the counts are read and added to even when k0 = 0 (a seeded or wrapped accumulation)
    const int* weight;        // [W H] history weights n_h (occl_resolve_kernel, occl_filter_kernel<true>); else unused
};
// occl_reproject_kernel's arguments (rt_occlusion_set_history; rto::reproject, rto::history_seed):
// the seed of every pixel of the new frame (surf -> count, weight) from the previous frame's
// record, counts and weights, seen through the previous camera.  Device pointers.
struct OcclReprojParams {
    rt::DCamera prev_cam;
    int W, H;
    int n_prev, max_history;  // the samples the previous frame took since its own move; the cap
    float normal_min, plane_tol;                // the history's accept test (rto::filter_accept)
    const float4* surf;       // [2 W H] the new frame's surface record
    const float4* prev_surf; const int* prev_count; const int* prev_weight;
    int* count; int* weight;  // [W H] each, written for every pixel
};

}  // namespace rtd

#include "rt_plan.h"   // the LDS layout and MODE bits; the launch plan (trace_variant_key and the rest)

namespace rtd {

// ---------------------------------------------------------------------------
// Launch layer (defined in rt_kernels.hip)
// ---------------------------------------------------------------------------
// The trace kernel variant for a frame: its key (trace_variant_key: instantiation, dynamic LDS,
// the decisions the host's launch set-up depends on), the kernel and the blocks of it a CU holds.
struct TraceVariant : TraceKey {
    const void* fn;           // null: no kernel with this key (a programming error; nothing is launched)
    int per_cu;
};
// ns: suspended frames a sample needs (0: no refractive material).  Looks trace_variant_key's
// key up in the table of trace kernels, sets the function's dynamic LDS limit and queries its
// occupancy.
TraceVariant choose_trace_variant(const SceneView& S, int spp, bool tex, bool want_stats, bool prof, int ns);
// e0 / e1 (optional): timestamps taken by the dispatch itself, no marker packets
hipError_t launch_sky(bool brute, int blocks, TraceParams& P, SceneView& S, unsigned char* gsky, int* live,
                      const rtm::Box* mesh_box, float slack_a, float slack_b, hipStream_t st, hipEvent_t e0);
hipError_t launch_trace_kernel(const TraceVariant& v, int blocks, TraceParams& P, SceneView& S, hipStream_t st,
                               hipEvent_t e0, hipEvent_t e1);
// The query kernel for a batch (query_plan's key looked up in the table of query kernels; null fn:
// no kernel with this key, a programming error) and its launch.  S: view_of's scene with the
// camera-ray shortcuts off (rt_query).
// ordered: the ORD = 1 instantiation, which traces the rays in QueryParams::order's order (uncounted only).
struct QueryVariant : QueryKey { const void* fn; bool ordered; };
QueryVariant choose_query_variant(long long n_rays, const SceneView& S, bool any_hit, bool counted, int n_cu, int form,
                                  bool ordered = false);
hipError_t launch_query_kernel(const QueryVariant& v, QueryParams& Q, SceneView& S, hipStream_t st);
// ray_key_kernel (RT_QUERY_ORDER_SORTED): keys[i] = ray_key of ray i of the batch as query_kernel
// would trace it (B's origin / dir or pixel and camera) in `box`, idx[i] = i.
hipError_t launch_ray_keys(const RayBatch& B, const rtk::KeyBox& box, unsigned long long* keys, uint32_t* idx, hipStream_t st);
// The shade kernel for a batch (rt_shade): shade_plan's key looked up in the table of shade kernels
// (null fn: no kernel with this key, a programming error) and its launch.  P: the fields
// trace_sample reads (rt_shade.cpp lists them); S: caller_ray_view's scene.
struct ShadeVariant : ShadeKey { const void* fn; };
ShadeVariant choose_shade_variant(long long n_rays, const SceneView& S, int ns, bool tex);
hipError_t launch_shade_kernel(const ShadeVariant& v, TraceParams& P, SceneView& S, ShadeParams& Q, hipStream_t st,
                               hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// The single-workgroup BVH build (A.n <= BVH_WG_LEAVES) with `lds` bytes of dynamic LDS.
hipError_t launch_bvh_build(rtb::BvhArgs& A, bool lds_tree, size_t lds, hipStream_t st, hipEvent_t e0, hipEvent_t e1);
size_t scene_image_bytes(const SceneView& S);   // the scene image a fast kernel's block stages in LDS
// accum_fold_kernel (rt_accumulate): one more sample (`pass`: a 1-sample frame's raw radiance)
// into n_px pixels' running sums, which hold n_before samples (0: they are taken as zero, not
// read); resolve: the frame of n_before + 1 samples into rgba / radiance (each may be null).
hipError_t launch_accum_fold(const float4* pass, float4* sum_r, float4* sum_c, int n_px, int n_before, bool resolve,
                             uint32_t* rgba, float4* radiance, hipStream_t st, hipEvent_t e0, hipEvent_t e1);
// rt_accumulate's adaptive mode (rt_adapt.h).  accum_edge_kernel: need[g] = 1 for every tile with an
// edge pixel in sum_c at `threshold` (need: n_tiles bytes padded to whole dwords).  accum_lists_kernel:
// the needed tiles as live-group lists [NQ][live_cap] and, in `image` (WORK_INTS ints, zeroed
// by the caller), the work counters a trace launch over them starts from (the list lengths sum to
// the needed-tile count).  accum_fold_tiles_kernel: launch_accum_fold for the needed tiles of a
// pass with n_before >= 1; the other tiles only resolve, as the 1-sample frame.
hipError_t launch_accum_edge(const float4* sum_c, const rtad::TileGrid& t, float threshold, unsigned char* need, hipStream_t st,
                             hipEvent_t e0, hipEvent_t e1);
hipError_t launch_accum_lists(const unsigned char* need, int n_tiles, int* live, int live_cap, int* image, hipStream_t st,
                              hipEvent_t e0, hipEvent_t e1);
hipError_t launch_accum_fold_tiles(const float4* pass, float4* sum_r, float4* sum_c, const unsigned char* need,
                                   const rtad::TileGrid& t, int n_before, bool resolve, uint32_t* rgba, float4* radiance,
                                   hipStream_t st, hipEvent_t e0, hipEvent_t e1);
// rt_occlusion's kernels.  S: rt_query's view of the scene (camera-ray shortcuts off).
// launch_occl_surface: the surface record of every pixel's primary hit; launch_occlusion: P.samples
// more directions into the counts (null fn in the plan's table: a programming error, hipErrorInvalidValue);
// launch_occl_rays: the rays of sample P.k0 as occlusion_kernel forms them, no tracing.
hipError_t launch_occl_surface(const OcclPlan& plan, OcclParams& P, SceneView& S, hipStream_t st, hipEvent_t e0, hipEvent_t e1);
hipError_t launch_occlusion(const OcclPlan& plan, OcclParams& P, SceneView& S, hipStream_t st, hipEvent_t e0, hipEvent_t e1);
hipError_t launch_occl_rays(OcclParams& P, hipStream_t st);
// launch_occlusion and launch_occl_rays take the plan's / P's pattern's kernel; the
// surface record is always built under a shared-pattern plan.  launch_occl_filter: the filtered
// resolve of P.n_total samples into P.visibility / P.rgba (each may be null), after the call's last
// launch_occlusion, which then resolves `occluded` only.
hipError_t launch_occl_filter(const OcclPlan& plan, OcclParams& P, hipStream_t st, hipEvent_t e0, hipEvent_t e1);
// History across camera moves.  launch_occl_reproject: every pixel's seed from the
// previous frame; launch_occl_resolve: the unfiltered outputs of P.n_total samples since the move
// over the per-pixel totals P.weight + P.n_total; launch_occl_filter_history: launch_occl_filter
// with those totals as the denominators.  The counting launches then run with resolve = 0.
hipError_t launch_occl_reproject(OcclReprojParams& R, hipStream_t st, hipEvent_t e0, hipEvent_t e1);
hipError_t launch_occl_resolve(OcclParams& P, hipStream_t st, hipEvent_t e0, hipEvent_t e1);
hipError_t launch_occl_filter_history(const OcclPlan& plan, OcclParams& P, hipStream_t st, hipEvent_t e0, hipEvent_t e1);
void launch_unpermute(const uint32_t* g, uint32_t* out, int W, int H, int N, int rows_max, hipStream_t st);
void launch_profile_marker(int tag, hipStream_t st);
void launch_copy_gate(const unsigned* flag, unsigned long long max_ticks, hipStream_t st);
void launch_kat(int op, int n, const float* a, const float* b, const float* c, float* of, int* oi, unsigned long long* ou);

}  // namespace rtd
