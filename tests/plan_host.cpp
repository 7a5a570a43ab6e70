// Host driver of tests/test_plan_host.py: the trace launch plan (csrc/rt_plan.h) is pure host
// arithmetic, so which kernel, geometry, grid and history mode a frame gets is printed here on a
// machine without a GPU.  Host pass only; nothing calls HIP.
//   plan_host variants                          one line per case of the grid below:
//                                               ns_bucket lds mode shm part_k sky sky_brute
//   plan_host key n_inst n_real ftree tri_ax use_bvh n_tris n_mats n_lights n_meshes prune_abs
//                 spp tex stats prof ns no_part no_brute_sky
//                                               the same seven fields for one SceneView of those counts
//                                               (n_leaf padded from n_inst; tests/kernel_recipes.py)
//   plan_host scene_bytes n_inst n_real n_tris n_mats n_lights n_meshes
//                                               lds_bytes(S, true, true), rt_work.scene_bytes
//   plan_host shortcuts want_stats dbg depth amb(4) n_mats n_lights {Ke(4) Ka(4) Kt(4)} x n_mats {col(4)} x n_lights
//                                               shade_shortcuts' unlit_skip, occl_exit, ns (tests/test_integrator_host.py)
//   plan_host geometry W H row0 row_step spp    frame_geometry's fields
//   plan_host grid n_cu per_cu n_groups n_slots overlap other_running ranks_per_device
//   plan_host history want_stats dbg sky prof heavy_q n_groups full_waves
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rt_device.h"

using namespace rtd;

// The grid of synthetic scenes and launch options (tests/golden/trace_variants.npz holds the
// parent's answers, in this order).  Counts only: the plan reads no array.
static void variants() {
    static const rtm::TriAx some_tri_ax{};
    static const int leaves_bvh[] = {0, 512, 1500, 2500, 4000}, leaves_brute[] = {512, 2500};
    static const int insts[] = {1, 65, 1500}, tris[] = {12, 2000}, spps[] = {8, 65}, nss[] = {0, 2, 9};
    static const float prunes_bvh[] = {0.5f}, prunes_brute[] = {-1.0f, 0.5f};
    for (int use_bvh = 1; use_bvh >= 0; use_bvh--) {
        const int* leaves = use_bvh ? leaves_bvh : leaves_brute;    // use_bvh = 0: with a non-empty tree
        const int n_leaves = use_bvh ? 5 : 2;
        const float* prunes = use_bvh ? prunes_bvh : prunes_brute;  // (the brute-force sky pre-pass reads prune_abs)
        const int n_prunes = use_bvh ? 1 : 2;
        for (int li = 0; li < n_leaves; li++)
        for (int n_inst : insts)
        for (int n_tris : tris)
        for (int ftree = 0; ftree < 2; ftree++)
        for (int ax = 0; ax < 2; ax++)
        for (int pi = 0; pi < n_prunes; pi++)
        for (int spp : spps)
        for (int tex = 0; tex < 2; tex++)
        for (int want_stats = 0; want_stats < 2; want_stats++)
        for (int prof = 0; prof < 2; prof++)
        for (int ns : nss) {
            SceneView S{};
            S.n_leaf = S.n_real = leaves[li];
            S.n_inst = n_inst;
            S.n_tris = n_tris; S.n_mats = 4; S.n_lights = 2; S.n_meshes = 2;
            S.ftree = S.n_real >= 2 ? ftree : 0;
            S.use_bvh = use_bvh;
            S.tri_ax = ax ? &some_tri_ax : nullptr; S.ident_all = ax;
            S.prune_abs = prunes[pi];
            const TraceKey k = trace_variant_key(S, spp, tex != 0, want_stats != 0, prof != 0, ns, false, false);
            printf("%d %d %d %zu %d %d %d\n", k.ns_bucket, (int)k.lds, k.mode, k.shm, (int)k.part_k, (int)k.sky, (int)k.sky_brute);
        }
    }
}

int main(int argc, char** argv) {
    auto arg = [&](int i) { return i < argc ? atoll(argv[i]) : 0ll; };
    if (argc >= 2 && !strcmp(argv[1], "variants")) {
        variants();
    } else if (argc == 19 && !strcmp(argv[1], "key")) {
        // one SceneView of the given counts, as upload and view_of (rt_runtime.cpp) set them
        static const rtm::TriAx some_tri_ax{};
        SceneView S{};
        S.n_inst = (int)arg(2); S.n_real = (int)arg(3); S.ftree = (int)arg(4);
        S.tri_ax = arg(5) ? &some_tri_ax : nullptr; S.ident_all = arg(5) != 0;
        S.use_bvh = (int)arg(6);
        S.n_tris = (int)arg(7); S.n_mats = (int)arg(8); S.n_lights = (int)arg(9); S.n_meshes = (int)arg(10);
        S.prune_abs = (float)atof(argv[11]);
        S.n_leaf = 0;                                          // padded(): 1 << ceil(log2(n)), 0 for none
        if (S.n_inst > 0) { S.n_leaf = 1; while (S.n_leaf < S.n_inst) S.n_leaf <<= 1; }
        const TraceKey k = trace_variant_key(S, (int)arg(12), arg(13) != 0, arg(14) != 0, arg(15) != 0, (int)arg(16),
                                             arg(17) != 0, arg(18) != 0);
        printf("%d %d %d %zu %d %d %d\n", k.ns_bucket, (int)k.lds, k.mode, k.shm, (int)k.part_k, (int)k.sky, (int)k.sky_brute);
    } else if (argc == 8 && !strcmp(argv[1], "scene_bytes")) {
        // lds_bytes(S, true, true): the scene image of a fast kernel's block (rt_work.scene_bytes)
        SceneView S{};
        S.n_inst = (int)arg(2); S.n_real = (int)arg(3);
        S.n_tris = (int)arg(4); S.n_mats = (int)arg(5); S.n_lights = (int)arg(6); S.n_meshes = (int)arg(7);
        printf("scene_bytes %zu\n", lds_bytes(S, true, true));
    } else if (argc == 7 && !strcmp(argv[1], "geometry")) {
        const FrameGeometry g = frame_geometry((int)arg(2), (int)arg(3), (int)arg(4), (int)arg(5), (int)arg(6));
        printf("n_rows %d lanes_per_px %d px_per_wave %d gw %d gh %d l_shift %d gw_shift %d n_gx %d n_groups %d scramble %d "
               "scramble_small %d div_ngx_d %u div_perq_d %u\n",
               g.n_rows, g.lanes_per_px, g.px_per_wave, g.gw, g.gh, g.l_shift, g.gw_shift, g.n_gx, g.n_groups, g.scramble,
               g.scramble_small, g.div_ngx.d, g.div_perq.d);
    } else if (argc == 9 && !strcmp(argv[1], "grid")) {
        const GridPlan p = grid_policy((int)arg(2), (int)arg(3), (int)arg(4), (int)arg(5), (int)arg(6), arg(7) != 0, (int)arg(8));
        printf("blocks %d grid_waves %d heavy_static %d heavy_cap %d\n", p.blocks, p.grid_waves, p.heavy_static, p.heavy_cap);
    } else if (argc == 9 && !strcmp(argv[1], "history")) {
        printf("hist %d\n", history_mode(arg(2) != 0, arg(3) != 0, arg(4) != 0, arg(5) != 0, (int)arg(6), arg(7), arg(8)));
    } else if (argc >= 11 && !strcmp(argv[1], "shortcuts") && argc == 11 + 12 * atoi(argv[9]) + 4 * atoi(argv[10])) {
        // shade_shortcuts over the fields it reads: the ambience, the depth, every material's Ke, Ka, Kt
        // (refractive as flatten sets it: some Kt channel > 0) and every light's colour
        rt::Scene h;
        h.ambience = rtm::V4{(float)atof(argv[5]), (float)atof(argv[6]), (float)atof(argv[7]), (float)atof(argv[8])};
        h.depth = (int)arg(4);
        const char* const* f = argv + 11;
        auto v4 = [&]() { rtm::V4 v{(float)atof(f[0]), (float)atof(f[1]), (float)atof(f[2]), (float)atof(f[3])}; f += 4; return v; };
        for (int i = 0; i < atoi(argv[9]); i++) {
            rt::DMat m{};
            m.Ke = v4(); m.Ka = v4(); m.Kt = v4();
            m.refractive = m.Kt.x > 0 || m.Kt.y > 0 || m.Kt.z > 0 || m.Kt.w > 0;
            h.d_mats.push_back(m);
        }
        for (int i = 0; i < atoi(argv[10]); i++) { rt::DLight l{}; l.col = v4(); h.d_lights.push_back(l); }
        const ShadeShortcuts c = shade_shortcuts(h, arg(2) != 0, arg(3) != 0, -1);
        printf("unlit_skip %d occl_exit %d ns %d\n", c.unlit_skip, c.occl_exit, c.ns);
    } else {
        fprintf(stderr, "usage: plan_host variants | key ... | scene_bytes ... | shortcuts ... | geometry ... | grid ... | history ...\n");
        return 2;
    }
    return 0;
}
