/*
 * rt_amd.h — C ABI of the MI355X-native ray-tracing core (the drop-in boundary).
 *
 * Replaces the render path of wtzhang23/gpu-ray-tracer:
 *   rtracer::gpu::update_scene(Scene*, int kernel_dim, bool optimize)   include/raytracer.h:18-22, src/raytracer.cu:102-120
 *   rtracer::gpu::debug_cast(Scene*, int x, int y)                      include/raytracer.h:21,       src/raytracer.cu:91-100
 *   procedural::gpu::generate(std::string config_path)                  include/procedural/cube_world.h:20-23, src/procedural/cube_world.cc:195-207
 *   rtracer::SceneBuilder {add_vertex, create_mesh, add_triangle, add_trans, build_cube,
 *                          add_point_light, add_directional_light, build_gpu_scene}  include/scene_builder.h:29-117
 *   renv::gpu::Scene::free(Scene&)                                       include/rayenv/gpu/scene.h:55-69
 *   Camera/Entity translate/rotate/set_position/set_orientation          include/rayprimitives/entity.h:49-74
 *   Canvas::get_color / the framebuffer SDL wraps                        include/rayenv/canvas.h:17-44, src/rayenv/canvas.cu:10-29
 * Plain pointers and sizes only; every call returns an RT_* status and sets a
 * thread-local message readable with rt_last_error() (the reference asserts).
 */
#ifndef RT_AMD_H
#define RT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: rt_work gained the query-occupancy fields; RT_EXPORT_TRIS / RT_EXPORT_TEXCOORDS list
 *    triangles in the flattened mesh order (the index space of hit_tri)
 * 4: rt_host_alloc / rt_host_free / rt_copy_to_host_async / rt_copy_engines_warm (host-readable
 *    frames through a copy engine); a finished scene is uploaded and warmed at creation when a gfx950 device is present
 * 5: rt_scene_last_trace (test hook: the trace kernel a launch used); rt_frame_work keeps its
 *    frame when rt_render_opts.rgba is set
 *    (still 5: rt_query / rt_query_opts_default were added later; the change is additive, no
 *    existing entry or struct changed, so the version callers compare against stays)
 *    (still 5: additive -- rt_query_set_order / rt_query_last and the RT_QUERY_ORDER_* modes;
 *    rt_query_opts keeps its layout, the switch is scene state)
 *    (still 5: additive -- the RT_EXPORT_BVH_* values of rt_scene_export, a test hook)
 *    (still 5: additive -- rt_scene_set_shadow_hints and its test hooks)
 *    (still 5: additive -- rt_scene_set_near_first and its counters)
 *    (still 5: additive -- rt_accumulate_set_adaptive / rt_accumulate_adaptive_info and the pass
 *    buffer's test hooks; rt_accum_opts keeps its layout, the switch is scene state)
 *    (still 5: additive -- rt_occlusion and its companions, rt_ao_direction; no existing entry or
 *    struct changed)
 *    (still 5: additive -- rt_occlusion_set_pattern / rt_occlusion_set_filter / rt_occlusion_config
 *    and the measurement hook rt_occlusion_filter_timing; rt_occlusion_opts keeps its layout, both switches are scene state)
 *    (still 5: additive -- rt_occlusion_set_history / rt_occlusion_history_info, the test hook
 *    rt_occlusion_history_weights and the measurement hook rt_occlusion_history_timing; scene state)
 *    (still 5: additive -- rt_shade / rt_shade_opts_default and the test hook rt_shade_last; no
 *    existing entry or struct changed) */
#define RT_ABI_VERSION 5

enum {
    RT_OK = 0,
    RT_ERR_ARG = -1,      /* bad argument / out-of-range index */
    RT_ERR_IO = -2,       /* file cannot be opened */
    RT_ERR_PARSE = -3,    /* malformed scene description */
    RT_ERR_HIP = -4,      /* HIP runtime error (message has the hipError string) */
    RT_ERR_STATE = -5,    /* call not valid in the current state */
    RT_ERR_NODEV = -6,    /* no usable gfx950 device */
    RT_ERR_LIMIT = -7     /* scene exceeds a build limit (see rt_last_error) */
};

typedef struct rt_scene rt_scene;

/* ---- library ---- */
int rt_abi_version(void);
const char* rt_last_error(void);
int rt_device_count(int* count);
/* Select the HIP device for subsequent scene uploads on this thread. */
int rt_set_device(int device);

/* ---- scene creation ----
 * A finished scene (rt_scene_load_json, rt_builder_finish) goes to the current device at once
 * when a gfx950 device is present, as procedural::gpu::generate / build_gpu_scene do
 * (cube_world.cc:195-207, scene_builder.cu:29-81), and one untimed 1-spp frame warms the code
 * object, the scene's stream and the frame buffers; the first rt_update_scene then only renders.
 * Without a device the scene stays host-only and render calls return RT_ERR_NODEV.
 * RT_NO_WARM=1 (environment) defers the upload to the first render. */
/* worldN.json -> scene (cube_world.cc:38-191).  width/height <= 0 keep the JSON's canvas size. */
int rt_scene_load_json(const char* path, int width, int height, rt_scene** out);
/* Empty scene for the builder API (SceneBuilder{atlas_path}, scene_builder.h:51-56). */
int rt_scene_create(const char* atlas_path, rt_scene** out);
int rt_scene_free(rt_scene* s);

/* SceneBuilder (scene_builder.h:58-112).  Indices are returned through out-params. */
int rt_builder_add_vertex(rt_scene* s, float x, float y, float z, int* idx);
int rt_builder_create_mesh(rt_scene* s, const float pos3[3], const float quat4[4], int* mesh);
/* material26: Ke[4] Ka[4] Kd[4] Ks[4] Kt[4] Kr[4] alpha eta (material.h:14-31) */
int rt_builder_add_triangle(rt_scene* s, int mesh, int i0, int i1, int i2, const float material26[26]);
/* add_triangle with rprimitives::TextureCoords (texture_coords.h:12-29): tex6 = {tx, ty, ux, uy, vx, vy};
 * a hit with barycentric weights (u, v) of vertices i1, i2 reads atlas texel (tx, ty) + u (ux, uy) + v (vx, vy)
 * in the textured shading mode (build-defined: the reference never samples, phong.cu:18-23). */
int rt_builder_add_triangle_tex(rt_scene* s, int mesh, int i0, int i1, int i2, const float material26[26],
                                const float tex6[6]);
int rt_builder_add_trans(rt_scene* s, int mesh, int* trans);
int rt_builder_set_trans(rt_scene* s, int trans, const float pos3[3], const float quat4[4]);  /* either may be NULL */
int rt_builder_build_cube(rt_scene* s, float scale, const float material26[26], int* mesh);
/* build_cube with every face mapped onto the atlas square tile3 = {tx, ty, size} (texels). */
int rt_builder_build_cube_tex(rt_scene* s, float scale, const float material26[26], const float tile3[3], int* mesh);
int rt_builder_add_point_light(rt_scene* s, const float pos3[3], const float col4[4]);
int rt_builder_add_directional_light(rt_scene* s, const float dir3[3], const float col4[4]);
/* Canvas + Camera (camera.cu:6-9) + Environment (environment.h:19-93); finalises the builder. */
int rt_builder_finish(rt_scene* s, int width, int height, float fov_radians, float unit_to_pixels,
                      const float cam_pos3[3], const float cam_quat4[4],
                      const float dist_atten3[3], const float ambience4[4], int depth);

/* ---- texture atlas (assets.cc:61-81, gputils TextureBuffer4D alloc.h:24-80) ----
 * Texels are float RGBA = byte / 255 in HBM, point-sampled with clamp addressing as the
 * reference's texture object (gfx950 has no texture units).  Only read when
 * rt_render_opts.textures = 1. */
int rt_scene_set_atlas(rt_scene* s, const uint8_t* rgba8, int width, int height);
/* Decode an 8-bit RGB/RGBA PNG.  png_path NULL: the scene's own atlas entry (JSON "atlas"
 * or SceneBuilder{atlas}), resolved against the scene file's directory, then the CWD. */
int rt_scene_load_atlas(rt_scene* s, const char* png_path);
/* atlas3 = {width, height, loaded} */
int rt_scene_atlas_info(const rt_scene* s, int32_t atlas3[3]);

/* info10 = {W, H, n_vertices, n_tris, n_meshes, n_instances, n_lights, n_point_lights, depth, n_materials} */
int rt_scene_info(const rt_scene* s, int32_t info10[10]);
/* Host copies of the scene arrays (layouts as in oracle/rt_oracle.h) for parity checks.
 * Triangles (and their texture coordinates) are listed in the flattened mesh order, the
 * index space of rt_render_opts.hit_tri. */
enum { RT_EXPORT_VERTICES = 0, RT_EXPORT_NORMALS = 1, RT_EXPORT_TRIS = 2, RT_EXPORT_MATERIALS = 3,
       RT_EXPORT_INSTANCES = 4, RT_EXPORT_INST_MESH = 5, RT_EXPORT_LIGHTS = 6, RT_EXPORT_CAMERA = 7, RT_EXPORT_ENV = 8,
       RT_EXPORT_TEXCOORDS = 9,   /* per triangle float7 {has, tx, ty, ux, uy, vx, vy} */
       RT_EXPORT_ATLAS = 10,      /* atlas RGBA8 bytes, width*height*4 (rt_scene_atlas_info) */
       /* Test hook (still ABI 5: additive values of `what`): the tree the most recent frame's BVH
        * build (rt_render, rt_update_scene, rt_frame_work) left in its frame slot, copied from the
        * device after that slot's work is done.  No kernel is launched and no frame state changes.
        * RT_ERR_STATE before any build (and so without a device).
        * INFO: int32[8] = {n_leaf, n_inst, n_real, fdepth, ftree, form, slot, 0}; n_leaf: padded
        *   leaf count; n_real: instances with a non-degenerate box; fdepth / ftree: depth of the
        *   ordered tree and whether the fast kernels are given it; form: the build that ran --
        *   1: one workgroup, tree in LDS, chunked rank sort; 2: one workgroup, tree in LDS, bitonic
        *   sort; 3: one workgroup, tree in HBM; 4: grid-wide (0 never appears: no build yet fails).
        * PAIRS: float[12 n_leaf], child-pair boxes in heap order: node k's component c of
        *   (mn.xyz, mx.xyz) at [12 (k >> 1) + (k & 1) + 2 c]; degenerate: mn = +inf, mx = -inf.
        * LEAF_INST: int32[n_leaf], instance of heap leaf n_leaf + i.
        * FNODE: max(n_real - 1, 0) records of 16 words, the ordered radix tree: 12 floats (child
        *   A / child B boxes, interleaved as PAIRS) and int32 {A, B, 0, 0} (>= 0: node, < 0:
        *   -1 - instance). */
       RT_EXPORT_BVH_INFO = 11, RT_EXPORT_BVH_PAIRS = 12, RT_EXPORT_BVH_LEAF_INST = 13, RT_EXPORT_BVH_FNODE = 14 };
int rt_scene_export(const rt_scene* s, int what, void* dst, int64_t dst_bytes);

/* ---- camera / environment (entity.h:49-74, environment.h:30-44) ---- */
int rt_camera_get(const rt_scene* s, float pos3[3], float quat4[4]);
int rt_camera_set(rt_scene* s, const float pos3[3], const float quat4[4]);      /* either may be NULL */
int rt_camera_translate(rt_scene* s, const float d3[3]);                        /* Entity::translate: p += o*d */
int rt_camera_rotate(rt_scene* s, const float dq4[4]);                          /* Entity::rotate: o = dq*o */
/* Camera::up()/right()/forward() unit directions (camera.cu:11-31) */
int rt_camera_axes(const rt_scene* s, float right3[3], float up3[3], float forward3[3]);
int rt_env_set(rt_scene* s, const float ambience4[4], const float dist_atten3[3], int depth);

/* ---- rendering ---- */
typedef struct rt_render_opts {
    int spp;            /* samples per pixel, >= 1 (1 == reference) */
    int use_bvh;        /* reference `optimize`: 1 BVH traversal, 0 brute force over instances */
    int rebuild_bvh;    /* 1: rebuild the BVH in this call (reference per-frame semantics); 0: reuse if built */
    int row0, row_step; /* render rows y = row0 + j*row_step (row-cyclic multi-GPU slice); 0,1 = full frame */
    int compact;        /* 0: outputs indexed by full-frame pixel y*W+x; 1: by slice row j*W+x */
    int kernel_dim;     /* reference's block edge (-d); accepted, the HIP path picks its own tiling */
    void* stream;       /* hipStream_t to launch on; NULL = the scene's own stream */
    uint32_t* rgba;     /* device outputs (NULL = internal canvas for rgba, skipped for the others) */
    float* radiance;    /* float4 per pixel: mean of unclamped sample radiance */
    int32_t* hit_inst;  /* primary hit of sample 0: instance index, -1 on miss */
    int32_t* hit_tri;   /* primary hit of sample 0: global triangle index, -1 on miss */
    int sync;           /* 1: wait for completion before returning (required for stats) */
    int host_outputs;   /* 1: rgba/radiance/hit_* are HOST pointers; results are copied back (implies sync) */
    int timing;         /* 1: time the BVH build and the trace kernel with start/stop events on the
                           dispatches themselves (hipExtLaunchKernel; no marker packets, no sync);
                           totals via rt_timing_collect */
    int textures;       /* 1: textured shading (build-defined, parity-unpinned): the diffuse colour of a
                           hit on a triangle with texture coordinates is its atlas texel instead of Kd
                           (the TODO branch of phong.cu:18-23).  0 (default) = the reference. */
} rt_render_opts;

typedef struct rt_stats {
    uint64_t rays;       /* closest-hit queries (= reference cast_ray calls) */
    uint64_t nodes;      /* BVH node tests, single-ray semantics */
    uint64_t leaves;     /* instance tests (= cast_local calls) */
    uint64_t tri_tests;  /* triangle tests */
    double bvh_ms;       /* BVH build kernel time (device events) */
    double trace_ms;     /* trace kernel time (device events) */
} rt_stats;

void rt_render_opts_default(rt_render_opts* o);
int rt_render(rt_scene* s, const rt_render_opts* opts, rt_stats* stats);

/* The work the fast (statistics-free) kernels do for one frame of `opts`, from a profiling
 * run of the fast kernel with wave-level counters (not timed; the frame is kept on request, below).  rt_stats
 * counts the reference's units (every cast_ray of propagate_ray, raytracer.cu:17-43); the
 * fast kernel proves some of them unnecessary and skips them (unlit shadow rays, pruned
 * subtrees, occluded-shadow early exits): this is what it does instead. */
typedef struct rt_work {
    uint64_t queries;       /* closest-hit queries issued: one per primary sample, reflection /
                               refraction ray and traced shadow segment */
    uint64_t wave_queries;  /* wave-level query steps (64 lanes each) */
    uint64_t pair_steps;    /* wave-level BVH child-pair tests */
    uint64_t leaf_visits;   /* wave-level leaf (instance) visits */
    uint64_t leaf_lanes;    /* lane-level leaf visits (cast_local calls) */
    uint64_t tri_iters;     /* wave-level triangle-loop iterations */
    uint64_t scene_bytes;   /* the scene the fast kernel reads: ordered-tree records, instance records,
                               triangles, meshes, materials, lights (staged into each block's LDS) */
    /* Query occupancy (ABI 3).  Lanes by integrator phase over every wave query: */
    uint64_t lanes_primary;    /* primary-ray queries (sample's first NORMAL frame) */
    uint64_t lanes_secondary;  /* reflection / refraction NORMAL-frame queries */
    uint64_t lanes_shadow;     /* traced shadow segments */
    uint64_t lanes_unlit;      /* shadow steps the unlit skip answers without a query */
    /* Over the wave queries of live groups only (some primary enters the tree's root; the sky
     * groups the pre-pass answers are left out): */
    uint64_t live_wave_queries;
    uint64_t live_lanes;       /* queries issued in them: occupancy = live_lanes / (64 live_wave_queries) */
    uint64_t hist_wave_queries[8];  /* live wave queries by active lanes: 1-8, 9-16, ..., 57-64 */
    uint64_t hist_pair_steps[8];    /* their child-pair steps */
    uint64_t hist_leaf_visits[8];   /* their leaf visits */
} rt_work;
/* BVH frames with 1 <= spp <= 64, untextured; RT_ERR_STATE when the scene has no profiling
 * variant (the fast kernel needs the ordered tree in LDS).
 * opts->rgba non-NULL: the profiling frame is rendered there (a device pointer, or with
 * host_outputs a host pointer it is copied to, as rt_render does; indexed as `compact` says);
 * NULL: the frame is dropped.  radiance / hit_inst / hit_tri are never written.  opts->stream is
 * ignored: the call runs on the scene's own stream and returns when the frame is done. */
int rt_frame_work(rt_scene* s, const rt_render_opts* opts, rt_work* work);

/* ---- progressive refinement: samples accumulated across calls ----
 * (still ABI 5: additive.)  The reference has no counterpart: its update_scene traces one sample
 * per pixel and starts from nothing every frame.  An interactive caller shows the 1-spp frame at
 * once and, while nothing moves, adds samples redraw by redraw: after n accumulated samples the
 * frame is the one rt_render(spp = n) returns -- sample k's sub-pixel offset depends on k alone,
 * and the sums take the samples in k order with the one-shot kernel's float32 additions, mean and
 * truncation (RGBA8 equal byte for byte).
 * Each new sample is one 1-spp trace launch (its sample index offset by the samples held) into a
 * scene-owned pass buffer, folded into scene-owned per-pixel sums; the call's last fold writes
 * the outputs.  A side entry, as rt_frame_work: it runs on the scene's own stream, waits for
 * frames in flight, rotates no frame slot and returns when the outputs are complete; its
 * launches are what rt_scene_last_trace reports.  Sums, pass buffer and kept hit ids are
 * allocated on first use and freed with the scene (RT_ERR_HIP if they cannot be: the scene stays
 * usable); rt_render and rt_update_scene never touch them.
 * The accumulation starts again by itself (sample 0 is traced anew and the restart counter goes
 * up) when anything that decides a sample changed since its first one: the camera, an instance
 * pose, rt_env_set, the atlas, or the `textures` flag.  use_bvh / rebuild_bvh do not change the
 * image and restart nothing. */
typedef struct rt_accum_opts {
    int samples;        /* samples to add in this call, >= 1 */
    int use_bvh, rebuild_bvh, textures;   /* as rt_render_opts; the BVH is built at most once per call */
    int restart;        /* 1: drop what is accumulated first */
    int host_outputs;   /* as rt_render_opts */
    uint32_t* rgba; float* radiance;      /* the frame after this call's samples; each may be NULL */
    int32_t* hit_inst; int32_t* hit_tri;  /* sample 0's primary hit, kept since it was traced */
} rt_accum_opts;
/* zeros, samples = 1, use_bvh = rebuild_bvh = 1 */
void rt_accum_opts_default(rt_accum_opts* o);
/* n_samples (may be NULL): the samples held after the call.
 * Checked before any device work -- RT_ERR_ARG: null opts, samples < 1, no output requested;
 * RT_ERR_LIMIT: the call would hold more than 65536 samples; RT_ERR_STATE: a scene split by
 * rt_scene_set_devices (and textures = 1 without an atlas).  RT_ERR_NODEV: no usable device. */
int rt_accumulate(rt_scene* s, const rt_accum_opts* opts, int* n_samples);
/* Drop what is accumulated (host state; the next rt_accumulate traces sample 0). */
int rt_accumulate_reset(rt_scene* s);
/* out4 = {samples held, W, H, restarts so far (rt_accumulate_reset, restart = 1 and the scene's
 * own changes, each counted when it dropped at least one sample)} */
int rt_accumulate_info(const rt_scene* s, int32_t out4[4]);

/* Adaptive refinement (opt-in scene state, as rt_query_set_order).  This integrator is
 * Whitted-style: a later sample differs from sample 0 only by its sub-pixel offset, so it changes
 * a pixel only where the image has an edge.  With the mode on, an accumulation traces sample 0
 * everywhere, decides once which tiles have an edge, and traces and folds every later sample for
 * those tiles only.
 * A tile is the pixel group of a whole-frame 1-spp launch (8 x 8 pixels, clipped to the canvas).
 * A pixel is an edge pixel when some pixel of its 8-neighbourhood inside the canvas differs from
 * it by more than `threshold` in some channel of sample 0's radiance clamped to 1 (float32; a NaN
 * difference flags nothing; hit ids take no part); a tile is needed when it holds an edge pixel,
 * so a contrast across a tile border flags both tiles.  The mask is decided right after sample
 * 0's fold and dropped with the sums at every restart.
 * After a call that leaves n samples held, a pixel of a needed tile is rt_render(spp = n)'s pixel
 * and a pixel of any other tile is rt_render(spp = 1)'s, both bit for bit; hit ids are sample
 * 0's; *n_samples and rt_accumulate_info[0] are the samples the needed tiles hold.  With no
 * needed tile later samples launch nothing and n still counts up.  Mode 0 is rt_accumulate as
 * documented above, unchanged. */
/* mode 0: uniform (default); 1: adaptive.  threshold >= 0, finite (ignored with mode 0).
 * Host state, no device needed.  A call that changes mode or threshold while samples are held
 * drops them (counted as a restart); a call that changes nothing does nothing.
 * RT_ERR_ARG: other modes, threshold negative / NaN / inf. */
int rt_accumulate_set_adaptive(rt_scene* s, int mode, float threshold);
#define RT_ADAPTIVE_THRESHOLD_DEFAULT (8.0f / 255.0f)
/* out8 = {mode, tile_w, tile_h, n_tx, n_ty, needed tiles (-1: no mask yet), tiles the last
 * pass's trace launch was given (n_tx*n_ty for sample 0 and for a kernel that cannot run from
 * tile lists: an unusable ordered tree, brute force over more than 64 instances), 0};
 * threshold may be NULL.  need (may be NULL): need_cap >= n_tx*n_ty bytes, 1 = needed, copied from
 * the device; RT_ERR_STATE if asked for before a mask exists, RT_ERR_ARG if too small. */
int rt_accumulate_adaptive_info(const rt_scene* s, int32_t out8[8], float* threshold, uint8_t* need, int64_t need_cap);
/* Test hooks: fill the scene's pass buffer with a 32-bit pattern / copy it out (W*H float4),
 * after every frame in flight.  RT_ERR_STATE before the first rt_accumulate. */
int rt_accumulate_pass_fill(rt_scene* s, uint32_t bits);
int rt_accumulate_pass_read(rt_scene* s, float* dst, int64_t cap_floats);
/* Test hook: the current frame slot's scheduling-history state, host state only: out12 = {parity,
 * the history slot a pending BVH build zeroes (-1: none), capacity, frame slot, the history key's
 * eight values (-1: none yet)}.  A refinement pass of the adaptive mode leaves parity, capacity, slot and key as they were. */
int rt_scene_history_info(const rt_scene* s, int32_t out12[12]);

/* ---- ray queries: closest hit or occlusion for caller-supplied rays ----
 * The reference has no counterpart: its cast_ray (scene.cu:42-73) is reachable only through the
 * integrator.  This entry runs that query for a batch of rays: the result of each ray is the
 * reference's cast_ray, the accepted triangle the integrator's primary query would find.
 * A side entry: it runs on the scene's own stream, waits for frames in flight, rotates no frame
 * slot, launches no trace kernel (rt_scene_last_trace and the scheduling history are untouched)
 * and returns when the results are complete.  A scene split by rt_scene_set_devices answers on
 * its own device.
 * A ray with a non-finite component, or whose direction normalises to the zero vector
 * (rmath::Ray: a length <= 1e-5, or one that overflows float), reports a miss. */
typedef struct rt_query_opts {
    int64_t n;              /* rays */
    const float* origin;    /* n*3 */
    const float* dir;       /* n*3, any length > 0: normalised as rmath::Ray(o, d) does */
    const float* tmax;      /* n, or NULL = +inf: hits with t >= tmax are not reported */
    const int32_t* pixel;   /* n*2 (x, y): the camera's sample-0 ray of that pixel, made on the device by
                               camera_at; exclusive with origin/dir */
    int use_bvh, rebuild_bvh;   /* as rt_render_opts */
    int any_hit;            /* 1: occlusion query, only `hit` is written (and rays_out, if asked for) */
    int host;               /* 1: every pointer is host memory (staged); 0: device pointers */
    /* outputs, each may be NULL */
    float* t; int32_t* inst; int32_t* tri;   /* miss: +inf, -1, -1 */
    float* uv;              /* n*2 barycentric weights of vertices 1, 2 (miss: 0) */
    float* normal;          /* n*3 world normal as Isect::norm after cast_local (miss: 0) */
    uint8_t* hit;           /* n: 1 = an accepted hit with THRESHOLD <= t < tmax */
    float* rays_out;        /* n*6: origin and normalised direction the kernel traced */
} rt_query_opts;
/* zeros, use_bvh = rebuild_bvh = 1 */
void rt_query_opts_default(rt_query_opts* o);
/* stats NULL: the fast query.  Non-NULL: the reference's walk (the heap, or every instance with
 * use_bvh = 0) runs instead and rays / nodes / leaves / tri_tests count it in the reference's
 * units (rays: the rays that were traced; an occlusion query then runs without its early exit);
 * bvh_ms / trace_ms are the BVH build and the query kernel.
 * RT_ERR_ARG: null opts, n < 0, neither pixel nor both of origin and dir, pixel together with
 * either, no output requested, any_hit without `hit`, and with host = 1 a pixel outside the canvas
 * (device pixels are the caller's to keep inside it).  n = 0: RT_OK, nothing is done.
 * RT_ERR_NODEV: no usable device. */
int rt_query(rt_scene* s, const rt_query_opts* opts, rt_stats* stats);

/* The order rt_query traces a batch in.  RT_QUERY_ORDER_CALLER (default): 64 consecutive rays
 * to a wave, as given.  RT_QUERY_ORDER_SORTED: for batches whose order is not a frame's
 * (occlusion rays from hit points, bounce rays, picks from many views) -- on the scene's stream
 * the call forms a 64-bit key per ray (origin cell in the scene's box, then direction; rejected
 * rays last), sorts (key, ray index) on the device (stable) and traces wave c's lane l as ray
 * order[64 c + l].  Every output is written at the ray's own index: the caller sees the arrays of
 * RT_QUERY_ORDER_CALLER, bit for bit.  A counted query (stats non-NULL) and a batch of n <= 64
 * rays run in caller order whatever the mode.  Ray indices are 32-bit: rt_query with n > 2^31 - 1
 * in sorted mode returns RT_ERR_LIMIT (checked with the arguments, before any device work).  The
 * sort's scratch (12 bytes a ray, double-buffered, plus the sort's temporary storage) belongs to
 * the scene, grows on demand and is freed with it; if it cannot be allocated the call returns
 * RT_ERR_HIP and the scene stays usable.  Sorting pays for itself on incoherent batches only: a
 * batch already in pixel order loses the sort's time.  Host-side state, no device needed; it
 * reaches nothing but rt_query.  RT_ERR_ARG: any other mode. */
enum { RT_QUERY_ORDER_CALLER = 0, RT_QUERY_ORDER_SORTED = 1 };
int rt_query_set_order(rt_scene* s, int mode);

/* The scene's most recent rt_query that reached its launch (test hook, as rt_scene_last_trace).
 * out8 = {TREE, LDS, ANY, STATS of the query kernel used, ordered kernel 0/1, persistent form
 * 0/1, blocks, batch was sorted 0/1}; bounds6 = the box (min3, max3) the keys were quantised in
 * (the instances' world boxes merged; zeros if the batch was not sorted); `order`, if non-NULL, is
 * a host array of order_cap entries that receives the last sorted batch's order, n entries
 * (copied from the device; nothing is written if the batch was not sorted).  Each may be NULL.
 * RT_ERR_STATE before the first rt_query; RT_ERR_ARG if order_cap < n. */
int rt_query_last(const rt_scene* s, int32_t out8[8], float bounds6[6], uint32_t* order, int64_t order_cap);

/* ---- shading caller-supplied rays: what a ray sees (build-defined; the reference has no counterpart) ----
 * The reference's integrator (propagate_ray, scene.cu:92-188) is reachable only for the rays of its
 * one pinhole camera.  This entry runs it for a batch of rays from anywhere: each ray's result is
 * what propagate_ray returns for it as a primary ray, with the depth, environment, lights and
 * materials of the scene as rt_env_set left them.  `radiance` is that unclamped sum and `rgba` its
 * 8-bit encoding as a 1-sample frame's (each channel clamped to 1, then truncated).  A ray that
 * misses, and a ray rt_query would reject (a non-finite component, a direction that normalises to
 * the zero vector), give (0, 0, 0, 0) and that value packed.
 * Pixel mode (`pixel`, with `sample` = k): the camera's ray of sample k of each pixel, offset as
 * rt_spp_offset(k), so the result is the radiance of sample k of rt_render; with k = 0 it is
 * rt_render(spp = 1)'s radiance and rgba, bit for bit, and `rays_out` is rt_query's.
 * A side entry like rt_query: it runs on the scene's own stream after the frames in flight, rotates
 * no frame slot, launches no trace kernel (rt_scene_last_trace, the scheduling history, the hint
 * table and the hint and near-first counters are untouched), builds the BVH at most once and
 * returns when the outputs are complete.  A call that builds the tree (rebuild_bvh = 1, or no valid
 * tree yet) leaves the build's own note behind, as rt_query's build does: the history slot the
 * build zeroes for the next frame (rt_scene_history_info's second value), which that frame
 * clears; a call on the frames' tree (rebuild_bvh = 0) changes no value rt_scene_history_info
 * reports.  A scene split by rt_scene_set_devices answers on its own device.
 * order = RT_QUERY_ORDER_SORTED, per call: the batch is keyed, sorted and indexed exactly as
 * rt_query's sorted mode (pixel mode: by the pixels' sample-0 rays) and every output is written at
 * the ray's own index, so the arrays are RT_QUERY_ORDER_CALLER's bit for bit; batches of n <= 64
 * run in caller order.  The sort uses the scene's sort scratch, the one rt_query's sorted mode
 * uses: a sorted rt_shade clears the order rt_query_last would copy out (that call then reports
 * RT_ERR_STATE for `order` until the next sorted rt_query), so rt_query_last never hands out an
 * order an rt_shade call wrote.
 * host = 1: every pointer is host memory, staged through one pinned image owned by the scene that
 * grows on demand and is freed with it; if it cannot be allocated the call returns RT_ERR_HIP and
 * the scene stays usable. */
typedef struct rt_shade_opts {
    int64_t n;              /* rays */
    const float* origin;    /* n*3 */
    const float* dir;       /* n*3, any length > 0: normalised as rmath::Ray(o, d) does */
    const int32_t* pixel;   /* n*2 (x, y): the camera's ray of sample `sample` of that pixel; exclusive with origin/dir */
    int sample;             /* pixel mode: k >= 0 */
    int use_bvh, rebuild_bvh, textures;   /* as rt_render_opts */
    int order;              /* RT_QUERY_ORDER_CALLER (default) or RT_QUERY_ORDER_SORTED, for this call */
    int host;               /* 1: every pointer is host memory (staged); 0: device pointers */
    /* outputs, each may be NULL */
    float* radiance;        /* n*4 */
    uint32_t* rgba;         /* n */
    float* rays_out;        /* n*6: origin and normalised direction the kernel shaded */
} rt_shade_opts;
/* zeros, use_bvh = rebuild_bvh = 1 */
void rt_shade_opts_default(rt_shade_opts* o);
/* Checked before any device work -- RT_ERR_ARG: null opts, n < 0, neither pixel nor both of origin
 * and dir, pixel together with either, sample < 0, no output requested, an unknown order, and with
 * host = 1 a pixel outside the canvas (device pixels are the caller's to keep inside it);
 * RT_ERR_LIMIT: sample >= 65536, RT_QUERY_ORDER_SORTED with n > 2^31 - 1, n > 256 (2^31 - 1) (one
 * 256-ray block per grid slot); RT_ERR_STATE: textures = 1
 * without an atlas.  n = 0: RT_OK, nothing is done.  RT_ERR_NODEV: no usable device. */
int rt_shade(rt_scene* s, const rt_shade_opts* opts);
/* The scene's most recent rt_shade that reached its launch (test hook, as rt_query_last): out8 =
 * {NS, TREE, TEX of the shade kernel used, batch was sorted 0/1, blocks, n's low 31 bits, 0, 0}.
 * RT_ERR_STATE before the first rt_shade. */
int rt_shade_last(const rt_scene* s, int32_t out8[8]);

/* ---- ambient occlusion (build-defined; the reference has no counterpart) ----
 * For every pixel of the current camera: how much of the hemisphere above its primary hit is
 * unoccluded within `radius`, estimated with cosine-weighted directions and accumulated across
 * calls as rt_accumulate accumulates radiance: show the first samples at once, add more per redraw
 * while nothing moves.  The result is not fed into the integrator's ambient term.
 *
 * Primary hit.  Pixel (x, y)'s primary hit is rt_query's pixel-mode result: the sample-0 ray
 * camera_at(x, y) as traced, (o, d) = rays_out, its t and its normal (Isect::norm).  A pixel whose
 * primary misses takes no part: count 0, visibility 1.
 * Surface point and frame (float32, one rounding per operation, no contraction; the order is fixed
 * in csrc/rt_occl.h):
 *   p = o + t d per component (t x d, then + o);
 *   n = the query's normal, each component negated (exactly) when dot(n, d) > 0, so it faces the viewer;
 *   s = copysignf(1, n.z), a = -1 / (s + n.z), b = (n.x n.y) a,
 *   t1 = (1 + ((s n.x) n.x) a, s b, -(s n.x)),  t2 = (b, s + (n.y n.y) a, -n.y)
 *   (the branchless orthonormal basis; n.z = -1 gives a = 1/2, finite).
 * Sample k, the global sample index, 0 <= k < RT_AO_MAX_SAMPLES, uses entry k = (x_k, y_k, z_k) of a
 * direction table every pixel shares (no per-pixel decorrelation): point k of the R2 sequence of
 * rt_spp_offset, (u, v) -> sqrt(u) (cos 2 pi v, sin 2 pi v) on the unit disk, z = sqrt(max(0, 1 -
 * x^2 - y^2)), computed on the host in double and rounded to float32 (rt_ao_direction).
 * Its occlusion ray: origin p + bias n (bias x n, then + p), raw direction (x_k t1 + y_k t2) + z_k n,
 * made by the Ray(o, d) constructor and traced exactly as rt_query(any_hit = 1, tmax = radius)
 * traces a caller's ray (accept THRESHOLD <= t < radius, the same early exit, the camera-ray
 * shortcuts off); a ray rt_query would reject (non-finite, direction normalising to zero) counts
 * as not occluded.
 * Result after n samples: occluded[pixel] = the count of occluded samples (int32), visibility[pixel]
 * = 1.0f - (float)count / (float)n with a correctly rounded division, rgba = visibility as an
 * opaque grey (v, v, v, 1) through Color's truncation to bytes.
 *
 * The call runs on the scene's own stream after every frame in flight, rotates no frame slot,
 * launches no trace kernel (rt_scene_last_trace and the scheduling history stay as they were) and
 * builds the BVH at most once; it returns when the outputs are written.  The counts, the surface
 * record (32 bytes a pixel, built with sample 0) and the table belong to the scene: allocated on
 * first use, freed with it; if they cannot be allocated the call returns RT_ERR_HIP and the scene
 * stays usable.  The accumulation restarts by itself (counted in rt_occlusion_info) when the
 * camera, an instance pose, `radius` or `bias` changed since its sample 0; rt_env_set, the atlas
 * and use_bvh restart nothing.
 * Checked before any device work -- RT_ERR_ARG: null opts, samples < 1, radius <= 0 or NaN, bias
 * negative or non-finite, no output requested; RT_ERR_LIMIT: the call would hold more than
 * RT_AO_MAX_SAMPLES samples; RT_ERR_STATE: a scene split by rt_scene_set_devices; RT_ERR_NODEV: no
 * usable device. */
#define RT_AO_MAX_SAMPLES 1024
#define RT_AO_BIAS_DEFAULT 1e-3f   /* world units: above the rounding of p for scenes a few hundred units across */
typedef struct rt_occlusion_opts {
    int samples;            /* directions to add in this call, >= 1 */
    float radius;           /* > 0; +inf = sky visibility */
    float bias;             /* >= 0, finite; RT_AO_BIAS_DEFAULT */
    int use_bvh, rebuild_bvh, restart, host_outputs;   /* as rt_accum_opts */
    float* visibility; int32_t* occluded; uint32_t* rgba;   /* W*H each, each may be NULL */
} rt_occlusion_opts;
/* zeros; samples = 1, radius = +inf, bias = RT_AO_BIAS_DEFAULT, use_bvh = rebuild_bvh = 1 */
void rt_occlusion_opts_default(rt_occlusion_opts* o);
/* *n_samples (may be NULL): the samples held after the call. */
int rt_occlusion(rt_scene* s, const rt_occlusion_opts* opts, int* n_samples);
/* Drop the samples held (counted as a restart if there were any).  Host state. */
int rt_occlusion_reset(rt_scene* s);
/* out4 = {samples held, W, H, restarts so far}.  Host state. */
int rt_occlusion_info(const rt_scene* s, int32_t out4[4]);
/* Entry k of the direction table.  RT_ERR_ARG: k outside [0, RT_AO_MAX_SAMPLES). */
int rt_ao_direction(int k, float out3[3]);
/* Test hook: the rays sample k traces for the current accumulation (its camera, poses and bias),
 * W*H*6 floats to host memory: origin, RAW direction before the Ray constructor; zeros where the
 * primary misses.  RT_ERR_STATE without an accumulation. */
int rt_occlusion_rays(rt_scene* s, int k, float* dst, int64_t cap_floats);

/* ---- ambient occlusion: interleaved directions and a geometry-aware filter (still ABI 5: additive) ----
 * Two opt-in pieces of scene state, host state both (no device needed).  With the pattern shared
 * and the filter off -- the defaults -- rt_occlusion writes every byte as described above.
 *
 * Direction pattern.  RT_AO_PATTERN_SHARED: every pixel's sample k uses table entry k (above): an
 * image of n samples is n shadow layers, n + 1 grey levels.  RT_AO_PATTERN_INTERLEAVED: pixel
 * (x, y) has class c = (x & 3) + 4 (y & 3) and its sample k uses entry 16 k + c of the same
 * table; origin, raw direction, the Ray constructor, the accept rule, the rejected-ray rule and
 * the count are as above with that entry in place of entry k (no new float arithmetic).  After n
 * samples any 4 x 4 window of pixels has used entries 0 ... 16 n - 1 between its pixels, each
 * exactly once.  The pattern holds at most RT_AO_INTERLEAVED_MAX_SAMPLES samples: a call that
 * would hold more returns RT_ERR_LIMIT, checked with the arguments; rt_occlusion_rays(s, k, ...)
 * exports entry 16 k + c per pixel and accepts 0 <= k < RT_AO_INTERLEAVED_MAX_SAMPLES.  The
 * pattern reaches rt_occlusion and rt_occlusion_rays only and is part of what an accumulation was
 * started with: a call that changes it while samples are held drops them (one restart, as
 * rt_accumulate_set_adaptive); a call that changes nothing does nothing.  RT_ERR_ARG: any other
 * value.  A split scene may set it (rt_occlusion refuses split scenes).
 *
 * Filtered resolve.  The counts do not depend on it, so setting it restarts nothing; the next
 * rt_occlusion call's outputs follow the new setting.  With the filter on, after a call that
 * leaves n samples held: occluded[pixel] is the raw count, unchanged.  A pixel is live when it has
 * a primary hit.  For a live centre C with surface record (p_C, n_C) the taps are the 16 pixels
 * Q = C + (dx, dy), dx, dy in {-2, -1, 0, 1}, that lie inside the canvas (any such window holds
 * each class once).  Tap Q is accepted when Q is live, dot(n_C, n_Q) >= normal_min and
 * fabsf(dot(n_C, e)) <= plane_tol with e = p_Q - p_C per component: float32, one rounding per
 * operation, dot as ((0 + x x) + y y) + z z; a NaN accepts nothing.  The centre tap is accepted
 * unconditionally.  With S the integer sum of the accepted taps' counts and m their number:
 * visibility = 1.0f - (float)S / (float)(m * n), rgba = its grey as above.  A centre without a
 * primary hit has visibility 1.  The filter works with either pattern.
 * RT_ERR_ARG: on outside {0, 1}; normal_min NaN or outside [-1, 1]; plane_tol negative, NaN or
 * infinite (validated, then ignored, with on = 0). */
enum { RT_AO_PATTERN_SHARED = 0, RT_AO_PATTERN_INTERLEAVED = 1 };
#define RT_AO_INTERLEAVED_MAX_SAMPLES (RT_AO_MAX_SAMPLES / 16)   /* 64 */
#define RT_AO_FILTER_NORMAL_DEFAULT 0.9f
#define RT_AO_FILTER_PLANE_DEFAULT  1e-2f  /* world units: far above the rounding of p, far below a cube's edge */
int rt_occlusion_set_pattern(rt_scene* s, int pattern);
int rt_occlusion_set_filter(rt_scene* s, int on, float normal_min, float plane_tol);
/* out4 = {pattern, filter on, samples the pattern can hold, OCCL_MAP_* the last call used (-1: none yet;
 * 0 row, 1 tile, 2 class: the lane-to-pixel mapping, on which no result depends)};
 * f2 = {normal_min, plane_tol}; either may be NULL.  Host state. */
int rt_occlusion_config(const rt_scene* s, int32_t out4[4], float f2[2]);
/* Measurement hook: with `on`, later filtered calls take start/stop events on occl_filter_kernel's
 * dispatch; *ms (may be NULL): the last timed dispatch's milliseconds, < 0: none yet.  Host state. */
int rt_occlusion_filter_timing(rt_scene* s, int on, float* ms);

/* ---- ambient occlusion: samples kept across camera moves by reprojection (still ABI 5: additive) ----
 * Ambient occlusion belongs to the surface point, not to the view: what a point collected under
 * the previous camera is still valid under the next.  Opt-in scene state, host state only (no
 * device needed), off by default; with it off rt_occlusion writes every byte as described above,
 * and with it on and no move yet every output byte equals what history off writes.
 *
 * rt_occlusion_set_history.  RT_ERR_ARG: on outside {0, 1}; max_history outside [1,
 * RT_AO_MAX_SAMPLES]; normal_min NaN or outside [-1, 1]; plane_tol negative, NaN or infinite
 * (validated with on = 0 too).  A call that changes `on` or `max_history` while samples are held
 * drops them (one restart, as rt_occlusion_set_pattern); a change of the two thresholds alone
 * drops nothing and applies at the next move; a call that changes nothing does nothing.  A split
 * scene may set it.
 *
 * Move.  With history on, an rt_occlusion call without `restart` that finds samples held and only
 * the camera changed since they were started (instance poses, radius, bias and pattern as they
 * were) does not drop them, it moves them: the buffers of the accumulation being left (surface
 * record, counts, history weights, camera) become the previous frame, a new surface record is
 * built for the current camera, every pixel is seeded from the previous frame (below) and the
 * call's samples are added.  A move is no restart: it is counted in `moves`, and
 * rt_occlusion_info[0] and *n_samples become the samples traced since the move.  Every camera
 * entry counts as a change, so rt_camera_set to the same pose is a move.  Everything else --
 * restart = 1, rt_occlusion_reset, an instance, radius, bias or pattern change, a failed launch --
 * drops history, weights and cursor together, as a restart.
 *
 * Sample cursor.  K counts the samples traced since the last drop, across moves.  Sample number K
 * uses the pattern's sample index k = K mod capacity(pattern) (entry k shared, entry 16 k + c
 * interleaved): a moved pixel takes new directions, and k stays the same for every pixel.
 * RT_ERR_LIMIT, checked with the arguments: the samples since the last move or drop plus the
 * call's may not exceed the capacity, so a call wraps the table at most once.
 * rt_occlusion_rays(s, k, ...) keeps its meaning: k is a sample index of the pattern.
 *
 * Reprojection (float32, one rounding per operation, no contraction, dot as above; fixed in
 * csrc/rt_occl.h).  For a new pixel with a live record (p, n) and the previous camera C' = (pos,
 * r, u, f, near, unit, W, H):
 *   v = p - pos per component;  a = dot(v, f), sx = dot(v, r), sy = dot(v, u);  no history unless a > 0;
 *   gx = (near x sx) / a, gy = (near x sy) / a;
 *   cx = gx x unit + 0.5f x W, cy = 0.5f x H - gy x unit        (the inverse of camera_at);
 *   fx = floorf(cx + 0.5f), fy = floorf(cy + 0.5f);
 *   no history unless fx >= 0, fx < W, fy >= 0 and fy < H, compared in float (a NaN rejects);
 *   the source is pixel q = ((int)fx, (int)fy) of the previous frame, accepted when q is live,
 *   dot(n, n_q) >= normal_min and fabsf(dot(n, p_q - p)) <= plane_tol: the filter's accept test
 *   with the history's thresholds and the new pixel as the centre.
 * Seed.  With c = the source's count and T = its history weight + the samples of the previous
 * frame: T <= max_history gives (c_h, n_h) = (c, T); otherwise n_h = max_history and c_h =
 * (c x max_history + T / 2) / T in int32 with truncating divisions.  A pixel without an accepted
 * source or without a primary hit gets (0, 0).
 * Resolve.  After a call that leaves n samples since the move: occluded[i] = c_h + the occluded
 * samples since the move; visibility[i] = 1.0f - (float)occluded / (float)(n_h + n), 1 without a
 * primary hit; rgba its grey.  With the filter on, S is the sum of the accepted taps' counts as
 * above and the denominator is the integer sum N of the accepted taps' (n_h + n), the centre
 * included: visibility = 1.0f - (float)S / (float)N.  Before any move every n_h is 0. */
#define RT_AO_HISTORY_DEFAULT 32
int rt_occlusion_set_history(rt_scene* s, int on, int max_history, float normal_min, float plane_tol);
/* out8 = {on, max_history, moves so far, cursor K, samples since the last move or drop
 *         (= rt_occlusion_info[0]), 1 if history weights are in use (a move since the last drop), 0, 0};
 * f2 = {normal_min, plane_tol}; either may be NULL.  Host state. */
int rt_occlusion_history_info(const rt_scene* s, int32_t out8[8], float f2[2]);
/* Test hook: the per-pixel history weight n_h, W*H int32 to host memory; RT_ERR_STATE without an
 * accumulation, RT_ERR_ARG if cap is too small. */
int rt_occlusion_history_weights(rt_scene* s, int32_t* dst, int64_t cap);
/* Measurement hook: with `on`, later calls take start/stop events on the dispatches of
 * occl_reproject_kernel (a move) and of the resolve with per-pixel totals (occl_resolve_kernel, or
 * the filter's history form); ms2 (may be NULL) = their last timed milliseconds, < 0: none yet. */
int rt_occlusion_history_timing(rt_scene* s, int on, float ms2[2]);

/* Frame slots (1 = default, up to 8).  The reference rebuilds its BVH inside every
 * update_scene call (raytracer.cu:103-119), so a frame owns per-frame state: BVH, work
 * counters and scheduling history.  With n slots, consecutive rt_render calls rotate
 * through n copies of that state.  Frames issued on other streams then overlap the
 * previous frames' tails on the CUs they have freed.  Each call waits (stream-ordered, no
 * host sync) for the last frame of its slot.  The caller gives frames in flight distinct
 * outputs.  Images are identical either way.  Waits for the device when changed. */
int rt_scene_set_frame_slots(rt_scene* s, int n_slots);

/* Grid of a frame issued while another frame of the scene is still running (four frame
 * slots): RT_OVERLAP_HALF (default) = half the CUs, so that two frames' persistent blocks
 * share the GPU and a block's tail (its slowest wave) holds fewer CUs; RT_OVERLAP_FULL =
 * every CU, as a frame issued alone gets.  HALF measured faster for device-resident
 * pipelines (frame -3%, row slices -4..-11%); FULL was faster for pipelines whose host copies
 * ran as blit kernels on the CUs (round 3), not for copy-engine copies (rt_copy_to_host_async,
 * DESIGN.md §4.2).  RT_OVERLAP_STREAM = half the CUs for every frame, the
 * first of a stream included, for callers that issue frames back to back: the first two
 * frames then run side by side instead of the second waiting for the first's tail (20-frame
 * streams -2%), but a frame issued alone takes half the GPU, so set it for the stream only.
 * Images are identical either way.  Host-side state. */
enum { RT_OVERLAP_HALF = 0, RT_OVERLAP_FULL = 1, RT_OVERLAP_STREAM = 2 };
int rt_scene_set_overlap(rt_scene* s, int policy);

/* Multi-GPU frames from one host process (the reference's single-device
 * update_scene, raytracer.cu:102-120, split over a node's GPUs).  After this call every
 * whole-frame rt_render / rt_update_scene of the scene renders n_ranks row-cyclic slices
 * (slice r = rows r, r + n_ranks, ...), ranks [i k, (i+1) k) on devices[i] (k = n_ranks /
 * n_devices; each device holds a replica of the scene and rebuilds the same BVH), gathers
 * them to devices[0] with RCCL (ncclGather over ncclCommInitAll communicators) and
 * un-permutes the rows there: the caller sees one frame, RGBA8 only.  devices[0] is the
 * scene's device.  n_ranks > n_devices gives several slices per device (on one GPU the
 * whole sequence runs with a one-rank communicator).  n_devices = n_ranks = 1 returns to
 * single-device frames.  Camera, instance and environment changes reach every replica. */
int rt_scene_set_devices(rt_scene* s, const int* devices, int n_devices, int n_ranks);

/* Sum of the event-timed kernel durations of all rt_render calls with timing=1
 * since the last collect (synchronizes those events), then resets. */
int rt_timing_collect(rt_scene* s, double* bvh_ms_total, double* trace_ms_total, int* n_frames);

/* ---- host-readable frames (the post-condition of update_scene, raytracer.cu:102-120 /
 * canvas.cu:23-29: the canvas is host memory the caller reads after the call) ---- */
/* Pinned (page-locked) host memory: the copy engines write it directly over PCIe. */
int rt_host_alloc(int64_t bytes, void** out);
int rt_host_free(void* p);
/* Enqueue a device -> host copy of `bytes` on `stream` (a hipStream_t; NULL = the null stream)
 * on a DMA copy engine: no compute unit is taken from frames in flight.  host_dst should come
 * from rt_host_alloc (pageable memory is staged by the runtime).  Stream-ordered: record an
 * event after it, or synchronize the stream, before reading host_dst. */
int rt_copy_to_host_async(void* host_dst, const void* dev_src, int64_t bytes, void* stream);
/* Start the device's SDMA copy engines a host-copy pipeline will use, once per process and
 * device: one gated copy from each of the n streams (hipStream_t; the streams the pipeline
 * copies from or orders copies behind).  The runtime gives a copy queued while earlier copies
 * are still pending the next idle engine, and a copy's first use of an engine creates that
 * engine's queue (~7 ms of host time inside the enqueue): a pipeline with frames in flight
 * would pay that inside its first timed frames.  Blocks until done. */
int rt_copy_engines_warm(void* const* streams, int n_streams);

/* Reference-equivalent frame: rebuild BVH if optimize, trace 1 spp, copy the frame into the
 * pinned host canvas on a copy engine, wait for that stream; the framebuffer is host-readable
 * afterwards (raytracer.cu:102-120). */
int rt_update_scene(rt_scene* s, int kernel_dim, int optimize);
/* Host framebuffer (RGBA8 packed R<<24|G<<16|B<<8|A, row-major W*H) after rt_update_scene. */
int rt_canvas_read(const rt_scene* s, uint32_t* dst, int64_t n_pixels);
const uint32_t* rt_canvas_host_ptr(const rt_scene* s);
/* Canvas::get_color(x, y) of the last rt_update_scene frame (canvas.cu:14-17). */
int rt_canvas_get_color(const rt_scene* s, int x, int y, uint8_t rgba4[4]);

/* debug_cast (raytracer.cu:91-100): trace pixel (x, y) and write an event log
 * ("shooting a ray", "preparing to shoot a reflection ray", ...) into buf. */
int rt_debug_cast(rt_scene* s, int x, int y, char* buf, int64_t cap);

/* Device-side math known-answer entry (test hook): evaluates `op` element-wise on
 * the GPU.  op names as in oracle/rt_oracle.h's orc_kat_*, plus the filtered variants
 * tri_hit_f, box_hit_f and box_pair (two boxes per element, two int results), and
 * box_from_local / box_merge (box7 = min3 max3 nondegenerate; entity7 = quat4 pos3 -> box6 +
 * int) and entity (entity7, v3 -> point/vec to/from local, 12 floats), and ray_key (in0 = n*6
 * rays as traced: origin, unit direction; in1 = n*6 boxes: min3, max3; out_u = the coherence
 * keys of RT_QUERY_ORDER_SORTED), and the shading chains' unit-length forms as the trace kernel
 * runs them, one vote per wave of 64 consecutive elements between the closed and the generic
 * form: normalized_unit (v3 -> normalized), unit_len_rcp (v3 -> len, 1 / len), reflect_unit
 * (dir3, nrm3 -> reflect) and reflect_pre_unit (unit dir3, unit nrm3, length -> reflect's tail).
 * Host pointers in/out. */
int rt_kat_device(const char* op, int n, const float* in0, const float* in1, const float* in2,
                  float* out_f, int32_t* out_i, uint64_t* out_u);

/* The trace kernel of the scene's most recent trace launch (test hook), from any entry that
 * launches one (rt_render, rt_update_scene, rt_frame_work, rt_debug_cast): what the launch used,
 * recorded when it was issued.  out8 = {NS, LDS, MODE of trace_kernel<NS, LDS, MODE>, dynamic LDS
 * bytes, partial parking, sky pre-pass, sky pre-pass over the instances' boxes, ordered tree
 * usable}.  RT_ERR_STATE before the first launch.  Host state only: no device call.  A scene
 * split by rt_scene_set_devices launches on its replicas, which this does not see. */
int rt_scene_last_trace(const rt_scene* s, int32_t out8[8]);

/* Shadow-query occluder hints: a per-scene device table, keyed by the shaded
 * surface (instance, triangle) and the light, that remembers which leaf of the scene's tree last
 * occluded a shadow query from there; the fast frames of all-opaque scenes try that leaf first.
 * A hint only: a frame is the same with any table contents, and with the switch off.  Default on;
 * scenes too large for the single-workgroup BVH build have no table.  A scene split by
 * rt_scene_set_devices switches its replicas too. */
int rt_scene_set_shadow_hints(rt_scene* s, int on);
/* Test hooks.  rt_scene_shadow_hints_fill sets every table entry to `value` (any 32-bit value) and
 * zeroes the counters, after every frame in flight.  rt_scene_shadow_hint_code gives the entry
 * value that names instance `inst`'s leaf in the most recently built ordered tree (0: the instance
 * is no leaf of it, or no such tree was built).  rt_scene_shadow_hint_counters reads the counters
 * accumulated since the last fill: shadow wave queries of the hinted kernels, those given a seed,
 * those ended entirely by the seed; out4[3] = the table's entry count (0: no table).
 * rt_scene_shadow_hints_read copies the table's entries out (`cap` entries of room; entry
 * inst * 64 + (tri & 15) * 4 + (light & 3)).  RT_ERR_STATE before the scene is on a device. */
int rt_scene_shadow_hints_fill(rt_scene* s, int32_t value);
int rt_scene_shadow_hints_read(rt_scene* s, int32_t* dst, int64_t cap);
int rt_scene_shadow_hint_code(rt_scene* s, int inst, int32_t* code);
int rt_scene_shadow_hint_counters(rt_scene* s, uint64_t out4[4]);

/* Nearer child first in closest-hit queries: the fast frames of all-opaque
 * scenes whose boxes provably hold their triangles visit, at a step where both children are hit,
 * the child more lanes enter first; a query whose result could depend on that order is detected
 * and walked again in the fixed order, so a frame is the same with the switch on or off.
 * mode 0: off; 1: on (the default; RT_NEAR_FIRST=0 in the environment: off); 2: on, and the
 * profiling variant (rt_frame_work, rt_profile_groups) orders its walk too -- its counts are the
 * fixed order's otherwise.  A scene split by rt_scene_set_devices switches its replicas too, and
 * replicas made later take the scene's mode.
 * rt_scene_near_first_counters (test hook) reads the counters accumulated since the last
 * rt_scene_shadow_hints_fill: wave queries walked near-first, those walked again in the fixed
 * order, pair steps that swapped; all 0 for a scene without a hint table. */
int rt_scene_set_near_first(rt_scene* s, int mode);
int rt_scene_near_first_counters(rt_scene* s, uint64_t out3[3]);

/* Profiling hook: launches an empty marker kernel of `tag` (1..64) workgroups on `stream` (a
 * hipStream_t; NULL = the default stream), so a rocprofv3 kernel or counter trace can find the
 * caller's timed region between two markers (bench.py --pmc-window, tools/pmc_step.py). */
int rt_profile_marker(int tag, void* stream);

/* Sample offset table of the build-defined spp extension (k=0 -> (0,0)). */
int rt_spp_offset(int k, float* dx, float* dy);

#ifdef __cplusplus
}
#endif
#endif
