// rt_plan.h — the trace launch plan: everything between "render this frame" and the launch
// that is pure arithmetic.  Included by rt_device.h after the kernel argument structs (include
// that, not this).  Two parts:
//  * the LDS layout helpers and MODE bits the kernels (rt_kernels.hip) and the host share;
//  * host functions with no HIP call and no environment read: which trace kernel a frame gets
//    (trace_variant_key; the table of kernels it indexes is choose_trace_variant's, in
//    rt_kernels.hip), the frame's lane mapping and group geometry (frame_geometry), its shading
//    shortcuts (shade_shortcuts), its grid (grid_policy) and its scheduling history mode
//    (history_mode), which query kernel a batch of caller-supplied rays gets (query_plan,
//    rt_query), and a host-pointer batch's layout in its staging (batch_plan).  launch_trace
//    (rt_runtime.cpp) and rt_query (rt_query.cpp) fill them in from them; tests/test_plan_host.py,
//    tests/test_query_host.py and tests/test_batch_stage_host.py check them without a GPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <numeric>

#include "../../include/rt_amd.h"

namespace rtd {

// ---- LDS layout of a persistent trace block (kernels and host)
constexpr int LDS_LIMIT = 150 * 1024;    // above this the BVH is read from global memory
constexpr int PARK_LDS_LIMIT = 158 * 1024;   // BVH image + parking area (160 KB per CU)
// PROF kernels keep the occupancy counters [24, PROF_END) per wave in LDS (a global atomic per wave
// query on a few shared addresses serialised and perturbed the profile 30x) and add them to d_stats
// once per wave at the end
constexpr int PROF_WAVE_SLOTS = 32;
static_assert(PROF_END - PROF_LANES_PRIMARY <= PROF_WAVE_SLOTS, "per-wave PROF counter slots");
constexpr size_t PROF_LDS_BYTES = 16 * PROF_WAVE_SLOTS * sizeof(unsigned long long);   // 16 waves per block

// Parked fields per lane (trace_sample's parking, rt_kernels.hip).  NS = 0 kernels run only scenes
// without a refractive material (launch_trace): there a shadow ray's light is never attenuated
// (rv = the light's colour, reloaded after the query), so they park 4 fields fewer.
constexpr int PARK_FIELDS = 29;
__host__ __device__ constexpr int park_fields(int ns) { return ns == 0 ? 25 : PARK_FIELDS; }
// Partial parking (M_PART): scenes whose ordered tree fills most of the LDS (world16: 93 KB)
// park the first PART_FIELDS fields only (the ray, its attenuation and the accumulated
// radiance); the rest stay in registers.  The instance records are then read from global
// memory (L2-resident; as scalar loads they measured +1%) to leave the LDS to the tree.
constexpr int PART_FIELDS = 14;

// stage_bvh's LDS image size (16-B multiple)
__host__ __device__ inline size_t a16(size_t b) { return (b + 15) & ~(size_t)15; }
// LDS shading cache (M_SHADE): mats | lights | tris | meshes, each 16-B aligned
__host__ __device__ inline size_t shade_bytes(const SceneView& S) {
    return a16(sizeof(rt::DMat) * (size_t)S.n_mats) + a16(sizeof(rt::DLight) * (size_t)S.n_lights) +
           a16(sizeof(rt::DTri) * (size_t)S.n_tris) + a16(sizeof(rt::DMesh) * (size_t)S.n_meshes);
}
__host__ __device__ inline size_t lds_bytes(const SceneView& S, bool ft = false, bool shade = false, bool brute = false,
                                            bool part = false) {
    const size_t sh = shade ? shade_bytes(S) : 0;
    if (brute) return a16(16 * (size_t)S.n_inst) + sh;        // inst4 only (M_BRUTE)
    if (ft && part) return 64 * (size_t)(S.n_real - 1) + sh;   // the ordered tree only (M_PART)
    if (ft) return 64 * (size_t)(S.n_real - 1) + 16 * (size_t)S.n_inst + sh;
    return a16(48 * (size_t)S.n_leaf + 4 * (size_t)S.n_leaf) + a16(16 * (size_t)S.n_inst) + sh;
}

// trace_kernel<NS, LDS, MODE>'s MODE word.
// MODE bit 0 (MULTI): spp > 64 -- several rounds of samples per lane (the per-pixel sums
// then stay live across rounds, which the common single-round kernel avoids).
// MODE bit 1 (STATS): exact work counters.  The divergent state machine keeps 64-bit
// counters in VGPRs, so frames without statistics use a kernel without them.
// MODE bit 2 (PARK): park integrator state in LDS during queries (trace_sample); needs
// PARK_FIELDS x 4 B x TRACE_BLOCK_P of LDS beside the BVH image.
// MODE bit 3 (TEX): textured shading (hit_kd), generic frame depth only.
// MODE bit 4 (FT): traverse the ordered LBVH (closest_hit) instead of the reference heap.
// MODE bit 5 (AXIS): FT with the axis-plane triangle path (S.tri_ax, cast_local).
// MODE bit 6 (PROF): profiling variant of the fast kernel -- wave-level step counts and
// s_memtime cycle accounting (rt_experiment 6); results identical, timing perturbed.
// MODE bit 7 (SHADE): the shading records staged in LDS after the BVH image (shade_bytes).
// MODE bit 8 (BRUTE): brute-force frames (use_bvh = 0) with only the instance loop compiled
// (closest_hit); LDS image = inst4 (+ the shading cache, parking area).
// MODE bit 9 (PART): partial parking (PART_FIELDS) with the tree alone in LDS (see PART_FIELDS).
constexpr int M_MULTI = 1, M_STATS = 2, M_PARK = 4, M_TEX = 8, M_FT = 16, M_AXIS = 32, M_PROF = 64, M_SHADE = 128,
              M_BRUTE = 256, M_PART = 512;

// ---- Which trace kernel a frame gets
// The instantiation trace_kernel<ns_bucket, lds, mode>, its dynamic LDS, and the decisions the
// host's launch set-up depends on.
struct TraceKey {
    int ns_bucket;            // NS: 0, 2 or MAX_FRAMES - 1 (the generic frame-stack depth)
    bool lds;                 // the scene image staged in LDS
    int mode;                 // M_* bits
    size_t shm;               // dynamic LDS of the launch
    bool part_k;              // partial parking (M_PART): wide live-list tickets at 64 lanes per pixel
    bool sky, sky_brute;      // sky pre-pass before the trace kernel; over the instances' grown boxes
};

// ns: suspended frames a sample needs (0: no refractive material).  no_part / no_brute_sky: the
// RT_NO_PART / RT_NO_BRUTE_SKY switches (choose_trace_variant reads the environment).
inline TraceKey trace_variant_key(const SceneView& S, int spp, bool tex, bool want_stats, bool prof, int ns, bool no_part,
                                  bool no_brute_sky) {
    constexpr int NG = MAX_FRAMES - 1;                     // generic frame-stack depth
    const int mode = (spp > 64 ? M_MULTI : 0) | (want_stats ? M_STATS : 0);
    // brute force (the reference's -r): no tree kernel (closest_hit's FT path assumes a tree)
    const bool brute = !S.use_bvh || S.n_leaf == 0;
    const bool ft = !brute && mode == 0 && S.ftree && lds_bytes(S, true) <= (size_t)LDS_LIMIT;
    const size_t lds = lds_bytes(S, ft);
    const bool use_lds = lds <= (size_t)LDS_LIMIT;
    const size_t park_bytes = (size_t)park_fields(ns <= 0 ? 0 : 2) * 4 * TRACE_BLOCK_P;
    const bool park = !tex && mode == 0 && use_lds && lds + park_bytes + (prof ? PROF_LDS_BYTES : 0) <= (size_t)PARK_LDS_LIMIT;
    // LDS shading cache beside the parked main kernel (not with the profiling variant)
    const bool shade = park && ft && S.tri_ax && !prof &&
                       lds + shade_bytes(S) + park_bytes <= (size_t)PARK_LDS_LIMIT;
    // brute-force fast frames: the instance loop only (M_BRUTE), axis-plane triangles, parked
    // state and the LDS shading cache beside the instance records
    const size_t lds_br = lds_bytes(S, false, true, true);
    const bool brute_k = brute && !tex && mode == 0 && !prof && S.tri_ax && lds_br + park_bytes <= (size_t)PARK_LDS_LIMIT;
    // ordered tree in LDS but no room for the whole parking area beside the instance records
    // (world16: 93 KB tree + 23 KB instances): partial parking, instances from global memory
    const size_t lds_pt = lds_bytes(S, true, true, false, true);
    const size_t part_bytes = (size_t)PART_FIELDS * 4 * TRACE_BLOCK_P;
    // (textured frames too: the hit's atlas colour stays in registers; part-parked kernels
    // exist only for NS = 0)
    const bool part_k = !brute_k && ft && (!park || tex) && mode == 0 && !prof && S.tri_ax && ns <= 0 &&
                        lds_pt + part_bytes <= (size_t)PARK_LDS_LIMIT && !no_part;

    TraceKey k{};
    k.part_k = part_k;
    // The MODE word.  The part-parked and brute-force kernels are whole configurations; every
    // other kernel is the OR of the decisions above, under three rules:
    // textured frames without the ordered tree are the generic textured kernels, M_TEX | mode
    // and nothing else (tex already rules out park, and with it shade and the profiling variant)
    const bool tex_generic = tex && !ft;
    // the axis-plane triangle path belongs to the fast kernels: parked ones, and textured ones
    const bool axis = ft && S.tri_ax && (park || tex);
    // the profiling variant is the parked axis kernel's (M_SHADE is never combined with it: shade)
    const bool prof_k = prof && axis && park;
    if (part_k) k.mode = M_PARK | M_FT | M_AXIS | M_SHADE | M_PART | (tex ? M_TEX : 0);
    else if (brute_k) k.mode = M_BRUTE | M_PARK | M_SHADE | M_AXIS;
    else if (tex_generic) k.mode = M_TEX | mode;
    else
        k.mode = mode | (tex ? M_TEX : 0) | (ft ? M_FT : 0) | (park ? M_PARK : 0) | (axis ? M_AXIS : 0) |
                 (prof_k ? M_PROF : 0) | (shade ? M_SHADE : 0);
    k.lds = use_lds || brute_k;                             // (brute_k: inst4 alone fits where the heap image may not)

    // The frame-stack depth: the smallest bucket that holds ns, where that kernel exists.
    k.ns_bucket = ns <= 0 ? 0 : ns <= 2 ? 2 : NG;
    // the generic textured kernels have the generic depth only
    if (tex_generic) k.ns_bucket = NG;
    // textured fast frames exist only for NS 2 and NG: ns <= 0 takes the NS = 2 kernel
    else if (tex && !part_k) k.ns_bucket = std::max(k.ns_bucket, 2);
    // plain unparked frames (no ordered tree, nothing parked): the counted and multi-round
    // kernels have the generic depth only
    else if (!ft && !park && !brute_k && mode != 0) k.ns_bucket = NG;

    k.shm = part_k ? lds_pt + part_bytes : brute_k ? lds_br + park_bytes
                   : (park ? lds + park_bytes : use_lds ? lds : 0) + (shade ? shade_bytes(S) : 0) +
                         (prof ? PROF_LDS_BYTES : 0);
    // sky pre-pass: the fast (ordered-LBVH) kernels, one round of samples, a tree to test
    // (brute-force frames: the instances' grown boxes instead, when the pruning claim holds)
    k.sky_brute = brute_k && !prof && !want_stats && spp <= 64 && S.prune_abs >= 0.0f && S.n_inst >= 1 &&
                  S.n_inst <= 64 && !no_brute_sky;
    k.sky = (ft && !prof && spp <= 64 && S.use_bvh && S.n_leaf > 0) || k.sky_brute;
    return k;
}

// ---- Frame geometry: the sample-parallel lane mapping and the pixel groups
// A factor coprime with the queue length, so t -> t * f mod len is a permutation
// (checked with gcd; f near len * 0.618 spreads consecutive tickets across the image).
inline int ticket_scramble(int len) {
    if (len <= 2) return 1;
    int f = (int)(len * 0.6180339887) | 1;
    while (std::gcd(f % len, len) != 1) f++;
    return f % len;
}

struct FrameGeometry {        // TraceParams' fields of the same names
    int n_rows;               // <= 0: no rows in the slice, nothing else is set
    int lanes_per_px, px_per_wave, gw, gh, l_shift, gw_shift, n_gx, n_groups;
    int scramble, scramble_small;
    UDiv div_ngx, div_perq;
};
inline FrameGeometry frame_geometry(int W, int H, int row0, int row_step, int spp) {
    FrameGeometry g{};
    g.n_rows = (H - row0 + row_step - 1) / row_step;
    if (g.n_rows <= 0) return g;
    // sample-parallel mapping: L lanes per pixel (one sample each per round), 64/L pixels per wave
    g.lanes_per_px = std::min(spp, 64);
    g.px_per_wave = 64 / g.lanes_per_px;
    int gw = 1;
    if ((g.px_per_wave & (g.px_per_wave - 1)) == 0) { while (gw * gw < g.px_per_wave) gw <<= 1; }
    else gw = g.px_per_wave;
    // Row slices with rows >= 8 frame rows apart (N >= 8 ranks): a 2-row group would pair
    // rows that far apart, so groups are one row (8 x 1 at 8 spp).  Measured with four frames
    // in flight: 8-way slice 0.234 -> 0.229 ms; whole frames and 2-way slices keep 4 x 2
    // (8 x 1 there: +3.4% / +2%; profiles/r01/ab_group_shape_v31.log).
    if (row_step >= 8) gw = g.px_per_wave;
    g.gw = gw; g.gh = g.px_per_wave / gw;
    auto log2_exact = [](int v) { int k = 0; while ((1 << k) < v) k++; return (1 << k) == v ? k : -1; };
    g.l_shift = log2_exact(g.lanes_per_px); g.gw_shift = log2_exact(g.gw);
    g.n_gx = (W + g.gw - 1) / g.gw;
    g.n_groups = g.n_gx * ((g.n_rows + g.gh - 1) / g.gh);
    const int per_q = (g.n_groups + NQ - 1) / NQ;           // a work queue's length
    g.scramble = ticket_scramble(per_q);
    g.scramble_small = (unsigned long long)(per_q + TPC) * (unsigned long long)g.scramble < (1ull << 32);
    g.div_ngx = udiv_make((unsigned)g.n_gx);
    g.div_perq = udiv_make((unsigned)per_q);
    return g;
}

// ---- Shading shortcuts (per launch: rt_env_set can change ambience and depth after the scene is finished)
struct ShadeShortcuts { int unlit_skip, occl_exit, ns; };
// occl_force: 1 / 0 force the occlusion early exit on / off, < 0: on for frames without statistics
inline ShadeShortcuts shade_shortcuts(const rt::Scene& h, bool want_stats, bool dbg, int occl_force) {
    ShadeShortcuts c{};
    {   // unlit skip (trace_sample, ST_LIGHT): every incoming light must be >= +0 and finite
        bool ok = !want_stats && !dbg;                        // (the PROF variant profiles the fast frame: on)
        auto pos0 = [](float v) { return std::isfinite(v) && !std::signbit(v); };
        for (const rt::DLight& l : h.d_lights) ok = ok && pos0(l.col.x) && pos0(l.col.y) && pos0(l.col.z) && pos0(l.col.w);
        for (const rt::DMat& m : h.d_mats)
            ok = ok && pos0(m.Kt.x) && pos0(m.Kt.y) && pos0(m.Kt.z) && pos0(m.Kt.w) && m.Kt.x <= 1.0f && m.Kt.y <= 1.0f &&
                 m.Kt.z <= 1.0f && m.Kt.w <= 1.0f;
        bool start_ok = true;                                  // no -0 channel in Ke + Ka * ambience (org_light)
        for (const rt::DMat& m : h.d_mats) {
            const rtm::V4 o = m.Ke + m.Ka * h.ambience;
            for (float v : {o.x, o.y, o.z, o.w}) start_ok = start_ok && !(v == 0.0f && std::signbit(v));
        }
        c.unlit_skip = ok ? (start_ok ? 2 : 1) : 0;
    }
    bool opaque = true;                                        // no refractive material
    for (const rt::DMat& m : h.d_mats) opaque = opaque && !m.refractive;
    // shadow-ray occlusion early exit (all-opaque scene, no statistics)
    c.occl_exit = (opaque && (occl_force == 1 || (occl_force < 0 && !want_stats))) ? 1 : 0;
    // suspended frames needed (<= MAX_FRAMES - 1); none without a refractive material, where a
    // reflection child replaces its parent (trace_sample, F_REFLECT)
    // (NS = 0 kernels assume that: a depth-0 scene with refraction takes the NS = 2 bucket)
    c.ns = opaque ? 0 : std::max(h.depth, 1);
    return c;
}

// ---- Shadow-query occluder hints (SceneView::hint)
// The table is keyed by the shaded surface and the light: HINT_SLOTS entries per instance, the
// surface triangle's low 4 bits x the light's low 2 bits; aliasing is harmless (a hint only).
// An entry names a leaf of the ordered LBVH by its parent's record and side, as hint_code; 0: none.
// A code is taken only if its node is a record of the frame's tree (hint_node_ok) and that side
// of it is a leaf: the seed visit is then one the walk itself could make (the node's own pair test).
constexpr int HINT_SLOTS = 64;
constexpr int HINT_COUNTERS = 3;        // shadow wave queries, those given a seed, those ended by it
constexpr int HINT_FIELD_BITS = 21;     // a wave's three counts, packed in one 64-bit scalar until it ends
__host__ __device__ inline int hint_key(int inst, int tri) { return inst * HINT_SLOTS + (tri & 15) * 4; }   // + (light & 3)
__host__ __device__ inline int hint_code(int node, int side) { return 2 * node + side + 1; }
__host__ __device__ inline int hint_node(int code) { return (code - 1) >> 1; }
__host__ __device__ inline int hint_side(int code) { return (code - 1) & 1; }
__host__ __device__ inline bool hint_node_ok(int code, int n_real) { return code > 0 && hint_node(code) < n_real - 1; }
__host__ __device__ inline size_t hint_table_ints(int n_inst) { return (size_t)n_inst * HINT_SLOTS; }
// the counters: HINT_STRIPES copies, one 64-byte line each (a block adds to copy block % HINT_STRIPES; the host sums)
constexpr int HINT_STRIPES = 64, HINT_STRIPE_WORDS = 8;
// ---- Nearer child first in closest-hit queries (SceneView::near_first)
// Three counters, in words NF_COUNTER0 .. +2 of each stripe above: wave queries walked near-first,
// those run again in DFS order, pair steps that swapped.
constexpr int NF_COUNTERS = 3, NF_COUNTER0 = 3;
constexpr int NF_FIELD_BITS = 21;       // a wave's three counts in one 64-bit scalar (the swaps take the top 22)
enum : int { NF_OFF = 0, NF_ON = 1, NF_PROFILE = 2 };   // NF_PROFILE: the profiling variant orders its walk too
inline size_t hint_bytes(int n_inst) {
    return hint_table_ints(n_inst) * sizeof(int) + (size_t)HINT_STRIPES * HINT_STRIPE_WORDS * sizeof(unsigned long long);
}

// ---- Grid policy
struct GridPlan { int blocks, grid_waves, heavy_static, heavy_cap; };
// per_cu: blocks of the chosen kernel a CU holds; other_running: another frame of the scene is
// still in flight (any slot count, any overlap policy): the heavy list's static dealing is for
// frames whose blocks all start at once.
inline GridPlan grid_policy(int n_cu, int per_cu, int n_groups, int n_slots, int overlap, bool other_running,
                            int ranks_per_device) {
    constexpr int BLOCK_WAVES = TRACE_BLOCK_P / 64;
    // Frames in flight: a launch issued while the scene's previous frame is still running takes
    // half the CUs.  A persistent block holds its CU (the LDS image) until its slowest wave
    // ends; fewer blocks, each running twice the groups, leave fewer CUs held by one wave's last
    // group, and two frames' blocks still cover the GPU.  Measured with four in flight
    // (tools/pipe_slices.py, per-rank ms per frame at N = 1/2/4/8, same box): 0.655-0.665 /
    // 0.374 / 0.226 / 0.156-0.157 with every CU, 0.646-0.654 / 0.347-0.354 / 0.200-0.205 /
    // 0.137-0.140 with half; 3/8, 5/8 and 3/4 of the CUs in between (profiles/r03/ab_grid/).
    // A frame issued alone (no other frame running) keeps every CU.  Requiring two or three
    // running frames instead of one measured the same (profiles/r03/ab_grid/grid2.log).  A
    // pipeline that copies every frame to the host measured 12% slower this way, with the copy
    // anywhere (render stream, copy stream, high priority, fewer blit workgroups) and with the
    // optional second half of the grid gated on later frames being queued
    // (profiles/r03/ab_grid/readback.log): such callers set RT_OVERLAP_FULL.
    int cap = n_cu * per_cu;
    if (n_slots >= 4 && overlap != RT_OVERLAP_FULL) {
        const bool running = overlap == RT_OVERLAP_STREAM || other_running;   // or a stream
        // Small frames (row slices of N >= 4 ranks: under ~48 groups per wave on half the CUs)
        // take a quarter: four frames' blocks share the GPU, each block runs twice the groups,
        // so its LDS staging and its slowest wave's tail weigh half as much.  Measured per-rank
        // ms per frame, 60-frame streams, same box (profiles/r04/grid_div.log): N = 8 0.112 ->
        // 0.101, N = 4 0.175 -> 0.171; whole frames unchanged by it (0.597 / 0.599), kept at half.
        const long long half_waves = (long long)(cap / 2) * BLOCK_WAVES;
        // (Not with virtual ranks, several slices of one frame per device from one scene: those
        // slices share frame slots, and a quarter measured slower there: --gpus 1 --ranks 8 per
        // slice 0.153 -> 0.173 ms, profiles/r04/grid_div.log.)
        const int div = ((long long)n_groups < RT_SMALL_FRAME_GPW * half_waves && ranks_per_device == 1) ? 4 : 2;
        if (running) cap = std::max(1, cap / div);
    }
    GridPlan g;
    g.blocks = std::max(std::min(cap, (n_groups + BLOCK_WAVES - 1) / BLOCK_WAVES), 1);
    g.grid_waves = g.blocks * BLOCK_WAVES;                  // the launch: dim3(blocks)
    // every block starts at once: a full grid and no other frame of the scene running (RT_OVERLAP_FULL
    // and 2-3 frame slots keep the full grid for overlapping frames; those frames keep the counter)
    g.heavy_static = (g.blocks == n_cu * per_cu && !other_running) ? 1 : 0;
    g.heavy_cap = std::max(2 * g.blocks * BLOCK_WAVES, n_groups / 4);   // a bound, not a target
    return g;
}

// ---- Scheduling history mode (TraceParams::hist): 0 none, 1 longest-first by time, 2 heavy-first by work
// full_waves: the waves of a grid over every CU.
// hist = 1, longest-first history (fast frames): valid while the launch layout is unchanged.
// Only where a wave runs few groups (1080p 8-way row slices: ~8 per wave): with more (63
// for a whole 1080p frame, 16 for a 4-way slice) the dynamic queues already balance the
// frame and the two clock reads per group cost as much as the shorter tail saves or more
// (measured, four frames in flight, ms per frame with / without: whole frame 0.919 / 0.914,
// 4-way 0.360 / 0.360, 8-way 0.179-0.186 / 0.200-0.204; profiles/r02/hist_policy.log).
// hist = 2, heavy-first by work where groups per wave are many: a group whose samples took
// >= heavy_q wave queries (mirror pixels: primary, shadow and reflection chains) is flagged,
// and the next frame of the slot runs the flagged groups first off a heavy live list the sky
// pre-pass builds.  No clock reads (the timed history's cost, item 17), one byte store per
// heavy group.  RT_HEAVY_Q (environment) sets heavy_q; 0 turns it off.
// The mode must not depend on the grid (half or whole, frames in flight or alone): the two
// modes' flags mean different things (hist = 1 flags only the groups on its heavy list and
// skips them in the normal queues; hist = 2 flags by work and lists nothing), so the history
// key includes the mode and a change of mode resets the flags.
inline int history_mode(bool want_stats, bool dbg, bool sky, bool prof, int heavy_q, long long n_groups, long long full_waves) {
    if (want_stats || dbg) return 0;
    if (sky && heavy_q > 0) return 2;
    return (prof || n_groups <= RT_HIST_GROUPS_PER_WAVE * full_waves) ? 1 : 0;
}

// ---- Ray queries (rt_query): which query_kernel a batch of caller-supplied rays gets
// The fast traversal's stack holds <= FT_MAX_DEPTH entries (closest_hit, FT path); a deeper
// ordered tree, or one with fewer than two real leaves, is unusable (SceneView::ftree = 0).
constexpr int FT_MAX_DEPTH = 31;
inline bool ordered_tree_usable(int n_real, int depth) { return n_real >= 2 && depth <= FT_MAX_DEPTH; }

enum : int { QT_ORDERED = 0, QT_HEAP = 1, QT_BRUTE = 2 };   // tree form of a query kernel
constexpr int QUERY_BLOCK_SMALL = 256;                     // small form: 4 waves, the tree read from global memory / L2
// Batches of at least this many rays take the persistent form.  Measured (tools/query_bench.py,
// profiles/query/query_bench.log): on world8_stress the small form was as fast or
// faster at every batch size up to a 1080p frame (2.07 M rays: 218 against 259 us in pixel order,
// 2.80 against 3.60 ms permuted): 20 waves per CU against the persistent block's 16, and blocks
// dealt out as CUs free up against a static stride; the 45-KB tree is L2-resident either way.
// No crossover was found, so the persistent form is kept for frame-sized batches only.
#ifndef RT_QUERY_PERSIST_RAYS
#define RT_QUERY_PERSIST_RAYS (1 << 20)
#endif
struct QueryKey {
    int tree;                 // QT_*
    bool lds;                 // the tree (brute force: inst4) staged in LDS; persistent form only
    bool any_hit;             // occlusion early exit compiled in
    bool counted;             // the reference heap walk with rt_stats' counters (STATS form)
    bool persistent;          // 1024-thread blocks, at most one per CU, striding over 64-ray chunks
    int block, blocks;        // the launch: dim3(blocks), dim3(block)
    size_t shm;               // dynamic LDS
};
// One ray per lane, one wave per 64 consecutive rays (a chunk).  Small batches (picking: one
// ray) run 256-thread blocks over ceil(n / 256) chunks' worth of rays and stage nothing;
// large ones run one 1024-thread block per CU that stages the scene image once (stage_bvh)
// when it fits LDS_LIMIT and reads it from global memory otherwise.  A counted query runs the
// whole reference walk (the heap, or the instance loop without a tree) so that its counters
// are the reference's: no ordered tree and no early exit.  An unusable ordered tree falls back
// to the heap walk.  form: < 0 by batch size, 0 small, 1 persistent (measurements).
inline QueryKey query_plan(long long n_rays, const SceneView& S, bool any_hit, bool counted, int n_cu, int form = -1) {
    QueryKey k{};
    const bool brute = !S.use_bvh || S.n_leaf == 0;
    k.tree = brute ? QT_BRUTE : (S.ftree && !counted) ? QT_ORDERED : QT_HEAP;
    k.counted = counted;
    k.any_hit = any_hit && !counted;
    k.persistent = form < 0 ? n_rays >= (long long)RT_QUERY_PERSIST_RAYS : form != 0;
    const long long chunks = (n_rays + 63) / 64;
    if (k.persistent) {
        const size_t image = lds_bytes(S, k.tree == QT_ORDERED, false, k.tree == QT_BRUTE);
        k.lds = image <= (size_t)LDS_LIMIT;
        k.shm = k.lds ? image : 0;
        k.block = TRACE_BLOCK_P;
        constexpr int BLOCK_WAVES = TRACE_BLOCK_P / 64;
        k.blocks = (int)std::max(1ll, std::min((long long)std::max(n_cu, 1), (chunks + BLOCK_WAVES - 1) / BLOCK_WAVES));
    } else {
        constexpr int BLOCK_WAVES = QUERY_BLOCK_SMALL / 64;
        k.block = QUERY_BLOCK_SMALL;
        k.blocks = (int)std::max(1ll, std::min((chunks + BLOCK_WAVES - 1) / BLOCK_WAVES, (long long)INT32_MAX));
    }
    return k;
}

// ---- Shading caller-supplied rays (rt_shade): which shade_kernel a batch gets
// The tree form is query_plan's rule for an uncounted query; the form is query_plan's small one only
// (256-thread blocks over ceil(n / 256) blocks, one ray per lane, nothing staged: DESIGN §3.5 found
// no crossover to the persistent form).  ns: shade_shortcuts' suspended frames; the NS = 0 kernels
// (no frame stack) are for scenes without a refractive material only, as the trace plan's, and
// every other scene takes the generic depth MAX_FRAMES - 1.
constexpr int SHADE_BLOCK = QUERY_BLOCK_SMALL;
struct ShadeKey {
    int tree;                 // QT_*
    int ns_bucket;            // 0 or MAX_FRAMES - 1
    bool tex;                 // the textured integrator (hit_kd)
    int block, blocks;        // the launch: dim3(blocks), dim3(block)
};
inline ShadeKey shade_plan(long long n_rays, const SceneView& S, int ns, bool tex) {
    ShadeKey k{};
    k.tree = query_plan(n_rays, S, false, false, 0, 0).tree;
    k.ns_bucket = ns == 0 ? 0 : MAX_FRAMES - 1;
    k.tex = tex;
    k.block = SHADE_BLOCK;
    k.blocks = (int)std::max(1ll, std::min((n_rays + SHADE_BLOCK - 1) / SHADE_BLOCK, (long long)INT32_MAX));
    return k;
}

// ---- The ambient-occlusion pass (rt_occlusion): its kernels' tree form and grid
// The tree form is query_plan's rule; the form is the small one only (256-thread blocks, nothing
// staged: DESIGN §3.5 found no crossover to the persistent form).  One pixel per lane; a wave takes
// 64 consecutive pixels of the row-major frame (OCCL_MAP_ROW: runs continue into the next row) or
// an 8 x 8 tile clipped to the canvas (OCCL_MAP_TILE).  Measured on world8_stress 1920 x 1080
// (profiles/occlusion/bench.txt); map < 0: the pattern's default.  A call's samples go in
// launches of at most OCCL_LAUNCH_SAMPLES directions, so that no single dispatch runs for long.
enum : int { OCCL_MAP_ROW = 0, OCCL_MAP_TILE = 1, OCCL_MAP_CLASS = 2 };
#ifndef RT_OCCL_MAP_DEFAULT
#define RT_OCCL_MAP_DEFAULT OCCL_MAP_TILE
#endif
// The interleaved direction pattern (OCCL_PATTERN_INTERLEAVED = RT_AO_PATTERN_INTERLEAVED; rt_occl.h):
// under OCCL_MAP_TILE a wave holds all 16 pixel classes, so the table entry is a per-lane load and
// the wave's rays fan out over 16 directions.  OCCL_MAP_CLASS (this pattern only) gives wave g one
// class of one 32 x 32 pixel region clipped to the canvas -- ceil(W/32) ceil(H/32) regions, 16 waves
// a region, region = g / 16 and class = g % 16, lane l the pixel (32 rx + 4 (l & 7) + cx,
// 32 ry + 4 (l >> 3) + cy) -- so the entry is wave-uniform again, at the price of a 4-pixel stride
// in the surface-record reads and the count's read-modify-write.  Measured on world8_stress
// 1920 x 1080, 16 samples (profiles/occlusion_filter/bench.txt): the class map is the
// pattern's default, 1.03 ms against the tile map's 3.02 ms at radius +inf, 1.78 against 6.97 at
// radius 2.  The surface record is built under the shared pattern's plan in either pattern.
enum : int { OCCL_PATTERN_SHARED = 0, OCCL_PATTERN_INTERLEAVED = 1 };
#ifndef RT_OCCL_MAP_INTERLEAVED_DEFAULT
#define RT_OCCL_MAP_INTERLEAVED_DEFAULT OCCL_MAP_CLASS
#endif
constexpr int OCCL_BLOCK = 256;
constexpr int OCCL_LAUNCH_SAMPLES = 64;
// The filtered resolve (occl_filter_kernel): one lane a pixel, a block a 32 x 8 pixel tile whose
// records and counts, with the taps' halo (2 to the left and above, 1 to the right and below),
// are staged in LDS once, an array per field.
constexpr int OCCL_FILTER_TX = 32, OCCL_FILTER_TY = 8;
struct OcclPlan {
    int tree;                 // QT_*
    int map;                  // OCCL_MAP_*
    int n_waves;              // waves with a pixel: 64-pixel runs, tiles, or 16 a 32 x 32 region
    int block, blocks;        // the launch: dim3(blocks), dim3(block)
    int pattern;              // OCCL_PATTERN_*
    int filter_bx, filter_by; // occl_filter_kernel's grid: dim3(filter_bx, filter_by), OCCL_FILTER_TX * OCCL_FILTER_TY threads
};
inline OcclPlan occlusion_plan(int W, int H, const SceneView& S, int map = -1, int pattern = OCCL_PATTERN_SHARED) {
    OcclPlan p{};
    p.tree = query_plan((long long)W * H, S, true, false, 0, 0).tree;
    p.pattern = pattern == OCCL_PATTERN_INTERLEAVED ? OCCL_PATTERN_INTERLEAVED : OCCL_PATTERN_SHARED;
    const bool il = p.pattern == OCCL_PATTERN_INTERLEAVED;
    p.map = map == OCCL_MAP_ROW || map == OCCL_MAP_TILE || (il && map == OCCL_MAP_CLASS) ? map
            : il ? RT_OCCL_MAP_INTERLEAVED_DEFAULT : RT_OCCL_MAP_DEFAULT;
    const long long px = (long long)W * H;
    const long long waves = p.map == OCCL_MAP_CLASS ? 16ll * ((W + 31) / 32) * ((H + 31) / 32)
                            : p.map == OCCL_MAP_TILE ? (long long)((W + 7) / 8) * ((H + 7) / 8) : (px + 63) / 64;
    constexpr int BLOCK_WAVES = OCCL_BLOCK / 64;
    p.n_waves = (int)std::min<long long>(waves, INT32_MAX);
    p.block = OCCL_BLOCK;
    p.blocks = (int)std::max(1ll, (waves + BLOCK_WAVES - 1) / BLOCK_WAVES);
    p.filter_bx = std::max(1, (W + OCCL_FILTER_TX - 1) / OCCL_FILTER_TX);
    p.filter_by = std::max(1, (H + OCCL_FILTER_TY - 1) / OCCL_FILTER_TY);
    return p;
}

// ---- The coherence order of a batch (rt_query_set_order): whether rt_query sorts the batch
// by ray key (rt_raykey.h) before it traces, the key bits the sort looks at, and the scene's
// scratch for it: keys (8 B) and ray indices (4 B), double-buffered, each buffer rounded up to
// 256 B; hipCUB's temporary storage follows them (its size is the library's to say).  A counted
// query stays in caller order (its counters are sums over the rays, whatever their waves) and
// so does a batch of one wave.  Ray indices are 32-bit: the caller checks n < 2^31 first.
enum : int { QUERY_ORDER_CALLER = 0, QUERY_ORDER_SORTED = 1 };
struct QueryOrderPlan {
    bool sort;
    int key_bits;             // SortPairs' end_bit (begin_bit 0)
    size_t keys_bytes, idx_bytes;   // one buffer of each
    size_t scratch_bytes;     // 2 keys_bytes + 2 idx_bytes
};
inline QueryOrderPlan query_order_plan(long long n_rays, int mode, bool counted) {
    QueryOrderPlan p{};
    p.sort = mode == QUERY_ORDER_SORTED && !counted && n_rays > 64;
    if (!p.sort) return p;
    auto a256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
    p.key_bits = rtk::RAYKEY_BITS;
    p.keys_bytes = a256(8 * (size_t)n_rays);
    p.idx_bytes = a256(4 * (size_t)n_rays);
    p.scratch_bytes = 2 * p.keys_bytes + 2 * p.idx_bytes;
    return p;
}

// ---- A batch given with host pointers (rt_query, rt_shade): its image in the entry's staging
// (rti::BatchStage).  A part is one of the caller's arrays, made from the parameter field that
// holds its pointer: `host` (the field's value then: an input's source, an output's destination),
// its bytes, whether the call has it, and `bind`, which points the field at the part's device copy
// (so a part and its field cannot come apart; the plan looks at neither).  A present part takes
// a16(bytes) at `off`, an absent one nothing; the inputs come first, then the outputs, each in list
// order, so one copy carries [0, in_bytes) in and one carries [in_bytes, total) out.
struct BatchPart { void* host; size_t bytes; bool output, present; size_t off; void* field; void (*bind)(void* field, void* dev); };
template <class T> BatchPart batch_part(T*& field, size_t bytes, bool output) {
    return {(void*)field, bytes, output, field != nullptr, 0, &field, [](void* f, void* d) { *static_cast<T**>(f) = static_cast<T*>(d); }};
}
template <class T> BatchPart in_part(const T*& field, size_t bytes) { return batch_part(field, bytes, false); }
template <class T> BatchPart out_part(T*& field, size_t bytes) { return batch_part(field, bytes, true); }
struct BatchPlan { size_t in_bytes, total; };
inline BatchPlan batch_plan(BatchPart* parts, size_t n_parts) {
    BatchPlan p{0, 0};
    for (const bool output : {false, true}) {
        for (size_t i = 0; i < n_parts; i++)
            if (parts[i].present && parts[i].output == output) { parts[i].off = p.total; p.total += a16(parts[i].bytes); }
        if (!output) p.in_bytes = p.total;
    }
    return p;
}

}  // namespace rtd
