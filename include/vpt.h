/* vpt.h — C-ABI of the MI355X wavefront render backend.
 *
 * Drop-in boundary for the hot path of Zydak/Vulkan-Path-Tracer.
 * The reference has no FFI; the seam is the C++ class surface its Editor calls:
 *   PathTracer     (PathTracer/PathTracer.h:83-183)
 *   PostProcessor  (PathTracer/PostProcessor.h:8-33)
 * Each entry point below names the reference member(s) it replaces.  The C++
 * facade in vulkan-path-tracer_amd/host/ (class PathTracer / PostProcessor /
 * FlyCamera with the reference's method names) is a thin shim over these calls;
 * INTEGRATION.md shows the binding a maintainer would add upstream.
 *
 * Conventions: plain pointers and sizes only; return 0 or a negative VPT_ERR_*;
 * never aborts; device memory is owned by the context, host buffers by the
 * caller; one host thread per context; matrices are float[16] column-major
 * exactly as glm stores a mat4; all struct layouts are the reference's scalar
 * layouts (Bindings.slang) so existing host data can be passed through.
 */
#ifndef VPT_H
#define VPT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VPT_OK 0
#define VPT_ERR_INVALID_ARGUMENT (-1)
#define VPT_ERR_NO_DEVICE (-2)     /* HIP device/runtime missing: the backend never falls back to a CPU path */
#define VPT_ERR_OUT_OF_MEMORY (-3)
#define VPT_ERR_NO_SCENE (-4)
#define VPT_ERR_DEVICE (-5)        /* a HIP call failed; see vpt_last_error() */
#define VPT_ERR_UNSUPPORTED (-6)
#define VPT_ERR_LIMIT (-7)         /* MAX_ENTITIES / MAX_INSTANCES / MAX_EMISSIVE_MESHES, PathTracer.h:192-195 */

/* Limits, PathTracer.h:192-195 (asserts PathTracer.cpp:182-184). */
#define VPT_MAX_ENTITIES 10000u
#define VPT_MAX_INSTANCES 100000u
#define VPT_MAX_EMISSIVE_MESHES 10000u

/* Feature flags == the Slang #define set assembled at PathTracer.cpp:621-654. */
#define VPT_FLAG_SKY_MIS (1u << 0)             /* ENABLE_SKY_MIS            SetSkyMIS            */
#define VPT_FLAG_MESH_MIS (1u << 1)            /* ENABLE_MESH_MIS           SetMeshMIS           */
#define VPT_FLAG_SHOW_ENV_DIRECTLY (1u << 2)   /* SHOW_ENV_MAP_DIRECTLY     SetEnvMapShownDirectly */
#define VPT_FLAG_GEOMETRY_NORMALS (1u << 3)    /* USE_ONLY_GEOMETRY_NORMALS SetUseOnlyGeometryNormals */
#define VPT_FLAG_ENERGY_COMPENSATION (1u << 4) /* USE_ENERGY_COMPENSATION   SetUseEnergyCompensation */
#define VPT_FLAG_FURNACE (1u << 5)             /* FURNACE_TEST_MODE         SetFurnaceTestMode   */
#define VPT_FLAG_RAY_QUERIES (1u << 6)         /* USE_RAY_QUERIES: shadow / distance queries as ray queries (RTCommon.slang:52-63, 88-101: direction as it is,
                                                * TMin 1e-4 / 1e-5, TMax 1e6, closest committed hit).  CLEAR = the TraceRay forms (RTCommon.slang:64-84, 103-117,
                                                * MissShadow.slang:4-9): normalised direction, TMin 1e-5, TMax 1000, accept-first-hit.  Upstream, the light-identity
                                                * compare of an emissive-mesh NEE sample then reads payload.TriangleIdx / InstanceIdx, which nothing on that path
                                                * writes (closest-hit shader skipped, MissShadow leaves them alone): an UNDEFINED word.  Pinned here (oracle and
                                                * kernels alike) as "never equal": in this mode an emissive-mesh NEE sample is drawn and never visible, so meshes
                                                * light the scene through BSDF-sampled hits only; sky visibility and GetDistanceToGeometry are well defined and exact */
/* Tonemap.slang:170 samples the bloom image with a sampler whose filter is VulkanHelper's
 * default (PostProcessor.cpp:67, unpinned): set = LINEAR (default), clear = NEAREST. */
#define VPT_FLAG_TONEMAP_LINEAR_BLOOM_TAP (1u << 7)
/* Strict, structure-independent hit rule (no reference counterpart; off by default): a ray/triangle candidate only counts
 * where the ray is inside the triangle's own bounding box (vpt_fp32.h hit_is_local).  Without it, a ray grazing a small
 * triangle at < 1e-3 rad can be given a hit up to ~1e-2 scene units off the triangle by fp32 rounding, which a box
 * hierarchy sees or not depending on its shape — about one ray in 1e9, 1e-11 relative L2 on a 531 M-sample image.
 * With it the image equals brute-force intersection bit for bit at any size.  Cost in throughput, measured at 1080p on the default
 * pipelines (profiles/r04_strict_rate.json): Cornell box (fused per-bounce kernels) 11.5 %, atrium (streams) 6.8 %, glass bust (streams, depth 32) 0.5 %. */
#define VPT_FLAG_LOCAL_HITS (1u << 8)
#define VPT_FLAGS_DEFAULT                                                                                   \
    (VPT_FLAG_SKY_MIS | VPT_FLAG_MESH_MIS | VPT_FLAG_SHOW_ENV_DIRECTLY | VPT_FLAG_ENERGY_COMPENSATION |    \
     VPT_FLAG_RAY_QUERIES | VPT_FLAG_TONEMAP_LINEAR_BLOOM_TAP) /* PathTracer.h:211-221 */

/* == PathTracer::Material (PathTracer.h:12-34) == CPUMaterial (Bindings.slang:55-77); 112 bytes. */
typedef struct vpt_material {
    float base_color[3];
    float emissive_color[3];
    float specular_color[3];
    float medium_color[3];
    float medium_emissive_color[3];
    float metallic;
    float roughness;
    float ior;
    float transmission;
    float anisotropy;
    float anisotropy_rotation;
    float medium_density;
    float medium_anisotropy;
    uint32_t base_color_texture;
    uint32_t normal_texture;
    uint32_t roughness_texture;
    uint32_t metallic_texture;
    uint32_t emissive_texture;
} vpt_material;

/* == Vertex (Bindings.slang:7-12) == VulkanHelper::LoadedMeshVertex (PathTracer.cpp:190-194); 32 bytes. */
typedef struct vpt_vertex {
    float position[3];
    float normal[3];
    float texcoord[2];
} vpt_vertex;

/* == VulkanHelper Mesh as used at PathTracer.cpp:204-225. */
typedef struct vpt_mesh {
    const vpt_vertex* vertices;
    uint32_t vertex_count;
    const uint32_t* indices;
    uint32_t index_count;
} vpt_mesh;

/* == VulkanHelper::MeshInstance as used at PathTracer.cpp:449-481. */
typedef struct vpt_instance {
    uint32_t mesh_index;
    uint32_t material_index;
    float transform[16];
} vpt_instance;

/* == TextureAsset, PathTracer.cpp:815-836: channels 4 = RGBA8 UNORM, 1 = R8 UNORM. */
typedef struct vpt_texture {
    uint32_t width;
    uint32_t height;
    uint32_t channels;
    const uint8_t* data;
} vpt_texture;

/* Scene as PathTracer::SetScene assembles it (PathTracer.cpp:158-676).  Texture indices in the
 * materials index `textures`.  `env_rgba` is the RGBA32F environment image (alpha is ignored;
 * importance, alias table and the per-texel pdf in alpha are derived by the backend exactly as
 * LoadEnvironmentMap does, PathTracer.cpp:1137-1332).  The three energy-compensation tables are
 * the contents of Assets/LookupTables/ (.bin files; 64x64x32, 128x128x32, 128x128x32 floats). */
typedef struct vpt_scene_desc {
    const vpt_mesh* meshes;
    uint32_t mesh_count;
    const vpt_material* materials;
    uint32_t material_count;
    const vpt_instance* instances;
    uint32_t instance_count;
    const vpt_texture* textures;
    uint32_t texture_count;
    const float* env_rgba;
    uint32_t env_width;
    uint32_t env_height;
    const float* lut_reflection;
    const float* lut_refraction_outside;
    const float* lut_refraction_inside;
} vpt_scene_desc;

/* Scalar state of PathTracer (PathTracer.h:197-233) that reaches the shaders through
 * PathTracerUniform (PathTracer.h:271-302) plus the feature-flag set, plus the one thing the
 * reference does not expose: the seed.  Reference: Seed = PCGHash(wall-clock ms)
 * (PathTracer.cpp:127-140); here Seed(dispatch k) = PCGHash(base_seed + k). */
typedef struct vpt_params {
    uint32_t samples_per_frame; /* SetSamplesPerFrame, default 1 */
    uint32_t max_samples;       /* SetMaxSamplesAccumulated, default 5000 */
    uint32_t max_depth;         /* SetMaxDepth, default 200 */
    float max_luminance;        /* SetMaxLuminance, default 500 */
    float focus_distance;       /* SetFocusDistance, default 1 */
    float dof_strength;         /* SetDepthOfFieldStrength, default 0 */
    float sky_azimuth;          /* SetSkyAzimuth, degrees */
    float sky_altitude;         /* SetSkyAltitude, degrees */
    float sky_intensity;        /* SetSkyIntensity, default 1 */
    uint32_t screen_chunk_count;/* SetSplitScreenCount, default 1 */
    float emissive_pdf_bias;    /* SetEmissiveMeshSamplingPDFBias, default 0 */
    uint32_t flags;             /* VPT_FLAG_* */
    uint32_t base_seed;
} vpt_params;

/* PostProcessor::TonemappingData + BloomData (PostProcessor.h:8-21). */
typedef struct vpt_post_params {
    float exposure;        /* 1.0 */
    float gamma;           /* 2.2 */
    float bloom_threshold; /* 2.0 */
    float bloom_strength;  /* 1.0 */
    uint32_t mip_count;    /* 10 */
    float falloff_range;   /* 5.0 */
    uint32_t schedule;     /* VPT_POST_FUSED (default) | VPT_POST_REFERENCE_PASSES; the output is identical, byte for byte */
} vpt_post_params;
#define VPT_POST_FUSED 0u            /* threshold inside the first down-sample; middle mips down in one launch, up in one; the smallest down and up in one; last up-sample + tonemap in one */
#define VPT_POST_REFERENCE_PASSES 1u /* one kernel per pass as PostProcessor.cpp:193-246 records them (the A/B baseline) */

typedef struct vpt_config {
    int device;          /* HIP device ordinal */
    uint32_t width;      /* output image, RGBA32F (PathTracer.cpp:507-512, 698) */
    uint32_t height;
    uint32_t shard_rank; /* this context renders rows y with y % shard_count == shard_rank */
    uint32_t shard_count;/* 1 = whole image */
    uint32_t frames_in_flight; /* largest batch (frames per wavefront batch) the context will hold; 0 = ~448M paths (226 frames at 1080p), never more than 60 % of
                                * the free device memory, at most 8192 frames.  This is a CAP, not an allocation: vpt_create allocates the path records of ONE
                                * frame (~0.8 GB at 1080p) and the buffers grow to the largest batch a vpt_render / vpt_render_async call actually asks for
                                * (min(dispatches, cap) frames, 380 B per path; vpt_stats.frames_allocated) — an interactive host that renders a frame per
                                * call never holds more than that one frame.  Contexts whose batches run as whole-path launches (VPT_PIPELINE_WHOLE, or AUTO
                                * where it applies) keep their paths in registers and allocate 36 B per sample + the records of one frame
                                * (vpt_stats.resident_frames == 1).
                                * DEFAULT SCHEDULE (this field 0 AND resident_frames 0): a context that regenerates paths (see resident_frames) or runs whole-path
                                * launches takes batches of 4 x F frames, F being the cap above (904 frames at 1080p), with F / 2 frames of paths resident
                                * (113; none for whole-path launches): 126 GB on a 1080p scene whose BVH lives in memory (profiles/r05_frames_sweep.json).
                                * To CAP THE MEMORY of a drop-in host set this field: e.g. frames_in_flight = 64, resident_frames = 16 holds
                                * 64 x pixels x 36 B + 16 x pixels x 290 B = 14.4 GB at 1080p (INTEGRATION.md "Device memory"). */
    uint32_t profile;    /* 1 = bracket every kernel launch with hipEvents (vpt_get_stats kernel times) */
    uint32_t count_traversal; /* 1 = count BVH node/triangle visits (slower; for the roofline's algorithmic bytes) */
    uint32_t pipeline;   /* VPT_PIPELINE_* */
    uint32_t build_flags; /* VPT_BUILD_*: how vpt_set_scene builds the BVH of this context (reported back in vpt_stats.build_flags) */
    /* Path regeneration: frames of PATHS a batch keeps in flight at a time.  A batch of F frames has F x pixels samples; with K < F resident
     * frames the camera-ray launch starts the first K x pixels samples, and behind every shade stage the room that ended paths left in the
     * next ray queue is REFILLED with the batch's next unstarted samples — a contiguous run of sample ids, i.e. a block of coherent camera
     * rays appended behind the survivors (seeds depend on pixel and frame only, a sample's result lands in its own slot of the frame sums
     * and the running mean is applied in frame order when the batch has finished) — so every launch works on ~K x pixels paths until the
     * samples run out: ~290 B per resident path + 36 B per sample instead of 380 B per sample.  Applies to the streams pipeline (scenes whose
     * BVH lives in memory; VPT_PIPELINE_AUTO / _STAGED / _STAGED_SORTED).  Whole-path launches (scenes that ride in LDS) hold no path records
     * at all, whatever this says; the fused per-bounce kernels, media batches, split-screen dispatch and VPT_PIPELINE_STAGED_R1 keep every
     * sample resident.  0 (default): with frames_in_flight == 0 too, batches of 4 x F frames keep F / 2 frames of paths resident (the default schedule
     * described at frames_in_flight); with an explicit frames_in_flight, every sample resident.  A value >= the batch size: every sample resident.
     * Measured trade: profiles/r05_frames_sweep.json
     * (DESIGN.md §3 "Regeneration by refill").  Images do not depend on it, bit for bit.  Reference loop being unrolled: RayGen.slang:28-33,116-159. */
    uint32_t resident_frames;
} vpt_config;

/* Spatial splits in the BVH builder (bvh_build.hpp): identical images, pays on scenes of uneven triangle sizes only (profiles/REJECTED.md).
 * Per context, never read from the environment: two contexts of one process cannot silently build different trees. */
#define VPT_BUILD_SBVH 1u
/* Keep the general instantiation of the whole-path / fused per-bounce kernels even when the scene qualifies for the class-specialised one
 * (every texture 1x1 and a black environment: k_whole<PLAIN>, kernels_whole.hip; k_bounce<PLAIN>, kernels_bounce.hip).  Images are identical; this is the A/B switch of that choice. */
#define VPT_BUILD_GENERAL_KERNELS 2u
/* Streams pipeline: never hand the rest of a batch to the one-launch finisher (kernels_finish.hip k_finish), i.e. run every bounce of every batch
 * through the stream stages.  By default a small batch (<= 6M samples: a frame or two per call) goes there after three bounces and a large one once
 * the host sees fewer than 262,144 paths alive: seven dependent launches per bounce on a short queue cost more than the finisher's one launch of
 * persistent waves.  Images are identical; this is the A/B switch of that choice. */
#define VPT_BUILD_STREAMS_ONLY 4u

/* AUTO = WHOLE where it applies (BVH in LDS, no media, one sample per pixel and frame), FUSED for the other scenes whose BVH fits in LDS next to
 * the traversal stacks, else STAGED.  Results are identical. */
#define VPT_PIPELINE_AUTO 0u
#define VPT_PIPELINE_FUSED 1u   /* one kernel per bounce */
#define VPT_PIPELINE_STAGED 2u  /* extend -> shade -> connect with compacted queues; traversal on the vote-scheduled persistent kernels */
#define VPT_PIPELINE_STAGED_SORTED 4u /* STAGED with the shade queue sorted by material class (miss | plain | textured | glass | emissive),
                                       * one shade launch per class, the miss and plain ones specialised.  Bit-identical; measured
                                       * 10-14 % SLOWER than STAGED on the BASELINE scenes (profiles/REJECTED.md), so AUTO never picks it */
#define VPT_PIPELINE_WHOLE 5u  /* one launch per batch (a batch of the headline's order of size: one per PART of it, a few — see vpt_stats.kernel_launches): persistent waves run every path from its camera ray to its end, a lane whose path has ended takes
                               * the batch's next sample (kernels_whole.hip k_whole; the reference's own shape: one RayGen thread = one whole path).
                               * For scenes whose BVH rides in LDS, no media, samples_per_frame == 1, every sample resident — VPT_ERR_UNSUPPORTED
                               * otherwise.  Bit-identical.  AUTO takes it wherever it applies: measured faster than FUSED at every batch size
                               * (Cornell box 1080p: 8.3 vs 7.4 Gsamples/s at 226 frames per batch, 3.8 vs 2.4 at one; profiles/r04_whole_ab.json) */
#define VPT_PIPELINE_STAGED_R1 3u /* LABORATORY build only (include/vpt_lab.h, libvpt_hip_lab.so): the same stages with round 1's kernels (slot-addressed records, 64 rays per
                                   * wave at a time), kept as the measured baseline.  vpt_create of the product library answers VPT_ERR_UNSUPPORTED */

#define VPT_KERNEL_COUNT 10
enum vpt_kernel_id {
    VPT_K_PRIMARY = 0,  /* whole-path pipeline: the batch's launches of k_whole, one per part (below); fused pipeline: bounce 0 (camera ray + extend + shade + connect);
                         * staged pipeline: raygen */
    VPT_K_EXTEND = 1,
    VPT_K_SHADE = 2,
    VPT_K_CONNECT = 3,  /* shadow rays + light accumulation + end-of-sample in one kernel (VPT_PIPELINE_STAGED_R1, laboratory build) */
    VPT_K_BOUNCE = 4,   /* bounce >= 1 fused (LDS-resident scenes): extend + shade + connect in one kernel */
    VPT_K_RESOLVE = 5,
    VPT_K_BLOOM = 6,
    VPT_K_TONEMAP = 7,
    VPT_K_SHADOW = 8,   /* staged pipeline: shadow-ray streams (sky rays, light rays) traced as any-hit searches */
    VPT_K_JOIN = 9      /* staged pipeline: NEE contributions joined with the emission, pathLight, end of sample */
};

typedef struct vpt_stats {
    uint64_t samples;          /* camera paths finished (GetSamplesAccumulated * pixels) */
    uint64_t frames;           /* m_FrameCount */
    uint64_t dispatches;       /* m_DispatchCount */
    uint64_t closest_rays;     /* rays traced by the extend kernel */
    uint64_t shadow_rays;      /* rays traced by the connect kernel */
    uint64_t connect_paths;    /* path-bounces that went through the connect kernel (staged pipelines); whole-path launches: hits of bounces >= 1, whose
                                * pathLight waits in the frame-sum slot while the hit is parked (16 B written + 16 B read each) */
    uint64_t primary_hits;     /* camera rays that hit geometry */
    uint64_t primary_survivors;   /* paths that continue after bounce 0 */
    uint64_t primary_shadow_rays; /* shadow rays traced inside the primary kernel */
    uint64_t nodes_visited;    /* extend kernel, only when count_traversal */
    uint64_t tris_tested;      /* extend kernel, only when count_traversal */
    uint64_t shadow_nodes_visited; /* connect kernel, only when count_traversal */
    uint64_t shadow_tris_tested;   /* connect kernel, only when count_traversal */
    uint64_t kernel_launches[VPT_KERNEL_COUNT];   /* whole-path batches count PARTS under VPT_K_PRIMARY and VPT_K_RESOLVE: a batch of at least ~450 M samples on a scene
                                * with 1x1 textures and a black environment runs as 3 parts of consecutive frames, each part's resolve on a second stream
                                * beside the next part's launch; every other batch is one part (csrc/path_plan.hpp decide) */
    double kernel_ms[VPT_KERNEL_COUNT]; /* only when profile (a part's resolve is timed on its own stream: it overlaps the next part's launch) */
    uint64_t total_vertex_count; /* GetTotalVertexCount */
    uint64_t total_index_count;  /* GetTotalIndexCount */
    uint32_t bvh_nodes;
    uint32_t bvh_triangles;
    uint32_t bvh_node_bytes;
    uint32_t bvh_tri_bytes;
    uint32_t emissive_mesh_count;
    uint32_t emissive_triangle_count;
    uint32_t frames_in_flight; /* the largest batch this context renders at once, in frames: NOT an echo of vpt_config.frames_in_flight — on the default
                                * schedule it is 4 x that cap (see vpt_config.frames_in_flight) */
    uint32_t shard_pixels;
    uint32_t bvh8_nodes;       /* laboratory build: eight-wide nodes of the BVH8 experiment (0 in the product library) */
    uint32_t build_flags;      /* VPT_BUILD_* the scene's BVH was built with */
    uint32_t frames_allocated; /* frames of samples the buffers currently hold (grows with the largest batch requested, <= frames_in_flight) */
    uint32_t resident_frames;  /* frames of paths the queues / stream records hold (vpt_config.resident_frames; < frames_allocated when paths are regenerated) */
    uint32_t reserved0;
    uint32_t graph_launches;   /* batches replayed from a captured hipGraph by vpt_render_async since vpt_reset_stats */
    /* Words of the traversal stacks' global SPILL regions written since vpt_set_scene (a lane's stack is 14 LDS entries, deeper entries
     * spill to a per-thread region; api_context.hip keeps one region per concurrently running traversal grid): [0] the context's main
     * stream, [1] the second stream the shadow kernels of bounce k run on beside the extend of bounce k + 1.  Counted from the regions
     * themselves (they are preset to a pattern no stack entry can be), so the figure belongs to the product kernels, not to counting variants. */
    uint64_t stack_spills[2];
    double set_scene_ms;       /* wall time of the last vpt_set_scene (validation, BVH build, uploads, derived tables) */
    double bvh_build_ms;       /* of which: the host-side BVH build (bvh_build.cpp; the reference builds BLAS / TLAS on the device, PathTracer.cpp:484-505) */
    /* Streams pipeline, the one-launch finisher (kernels_finish.hip k_finish, timed under VPT_K_BOUNCE): paths it took over from the streams, and the
     * closest-hit / shadow rays it traced — both also counted in closest_rays / shadow_rays above. */
    uint64_t finish_paths;
    uint64_t finish_closest_rays;
    uint64_t finish_shadow_rays;
    double set_environment_ms; /* wall time of the last vpt_set_environment (alias table and pdf on the host, upload); 0 before the first */
} vpt_stats;

typedef struct vpt_ctx vpt_ctx;

/* PathTracer::New (PathTracer.cpp:21-120) + CreateOutputImageView (692-710). NULL on failure;
 * *err (if non-NULL) receives the VPT_ERR_* code.  Fails with VPT_ERR_NO_DEVICE when no HIP
 * device is usable: there is no CPU fallback behind this API. */
vpt_ctx* vpt_create(const vpt_config* cfg, int* err);
void vpt_destroy(vpt_ctx* ctx);
const char* vpt_last_error(const vpt_ctx* ctx);

/* PathTracer::SetScene (PathTracer.cpp:158-676): uploads geometry/materials/textures, derives the
 * emissive-mesh list (449-469) and the env importance/alias tables (1137-1332), builds the BVH
 * (replaces BLASBuilder/TLAS, 488-505; builder options: vpt_config.build_flags), resets accumulation. Arrays are borrowed
 * for the call only. */
int vpt_set_scene(vpt_ctx* ctx, const vpt_scene_desc* scene);
/* PathTracer::SetMaterial (PathTracer.cpp:712-810): patches one material, rebuilds the emissive list
 * if emission changed, resets accumulation. */
int vpt_set_material(vpt_ctx* ctx, uint32_t index, const vpt_material* material);
int vpt_get_material(const vpt_ctx* ctx, uint32_t index, vpt_material* out);
/* Replaces the transforms of instances [first, first + count) of the installed scene (float[16] column-major each, as vpt_instance.transform)
 * and nothing else: no tree build, no geometry upload.  The world triangles are re-transformed and the BVH is REFITTED on the device — same
 * topology, every box recomputed bottom-up — and the tables derived from the matrices (normals, shading lines, lights) are filled again.
 * Afterwards the context renders the scene vpt_set_scene would have installed from the same description with these transforms: with
 * VPT_FLAG_LOCAL_HITS bit for bit at any size, without it exactly as far as two different trees agree (see that flag).  A refit does not restore
 * the quality of a fresh build: a host that has carried things far should call vpt_set_scene again when it has the time.
 * Accumulation is reset; lanes and spill regions, mesh and material indices, materials edited since, environment, volumes, atmosphere, camera and
 * parameters stay; vpt_stats.set_scene_ms / bvh_build_ms keep their values and vpt_get_set_transforms_ms answers this call's.  Waits for batches in flight.
 * VPT_ERR_NO_SCENE before the first vpt_set_scene; VPT_ERR_INVALID_ARGUMENT for a NULL array with count > 0 or a range past the instance count;
 * count == 0 is VPT_OK and changes nothing, not even the accumulation.  The set of degenerate triangles (slivers, which the tree holds no leaf
 * slot for) must stay what it was when the scene was installed: transforms that flatten a triangle, or revive one, return VPT_ERR_UNSUPPORTED —
 * use vpt_set_scene.  A rejected or failed call leaves the previous transforms installed.  In the laboratory build vpt_lab_trace's
 * VPT_TRACE_VOTE8 / VPT_TRACE_VOTE4S answer VPT_ERR_UNSUPPORTED after a move, until the next vpt_set_scene. */
int vpt_set_instance_transforms(vpt_ctx* ctx, uint32_t first, uint32_t count, const float* transforms);
/* Wall time of the last vpt_set_instance_transforms that moved something (re-transform, refit, derived tables); 0 before the first.  A call of its
 * own and not a field of vpt_stats: that struct ends with set_environment_ms, and its size and layout stay what hosts were compiled against.  Reads
 * the context only: it waits for nothing. */
int vpt_get_set_transforms_ms(const vpt_ctx* ctx, double* out_ms);
/* PathTracer::SetEnvMapFilepath (PathTracer.h:154) = LoadEnvironmentMap (PathTracer.cpp:1137-1332) with the .hdr already decoded by the
 * caller: replaces the environment map of the installed scene and nothing else.  env_rgba is what vpt_scene_desc.env_rgba is (RGBA32F,
 * alpha ignored, borrowed for the call); the importance, alias table and pdf are derived as vpt_set_scene derives them, so the context is
 * the one vpt_set_scene would have produced from the same description with this environment and every later image is bit-identical to
 * that context's.  The BVH, the pools, the derived tables, materials edited since, volumes, atmosphere, camera and parameters stay as
 * they are (no BLAS / TLAS work upstream either); vpt_stats.set_scene_ms / bvh_build_ms keep their values and set_environment_ms takes
 * this call's.  Waits for batches in flight.  VPT_ERR_NO_SCENE before the first vpt_set_scene, VPT_ERR_INVALID_ARGUMENT for a NULL map
 * or a zero dimension, VPT_ERR_LIMIT for 2^32 texels or more; a rejected or failed call leaves the previous environment installed.
 * Resets accumulation. */
int vpt_set_environment(vpt_ctx* ctx, const float* env_rgba, uint32_t env_width, uint32_t env_height);
/* ---- participating media: homogeneous box volumes ---------------------------------
 * PathTracer::Volume / VolumeGPU (PathTracer.h:36-74, 341-400) as the shaders read it (Volume.slang:19-52).
 * corner_min / corner_max are the WORLD-space box, i.e. Position + Corner * Scale already applied
 * (PathTracer.h:395-396).  Heterogeneous volumes take their density from a grid, dense (vpt_add_density_grid below: the
 * OpenVDB / NanoVDB tree of the reference, densified) or in the tree's own 8x8x8 leaves (vpt_add_density_bricks), including emission from
 * temperature / blackbody.
 * The integrator side is RayGen.slang:162-380 (free-flight sampling per box,
 * nearest scatter vs. distance to geometry, NEE towards sky and emissive meshes through every box's Beer-Lambert
 * transmittance, phase-function scattering) and ClosestHit.slang:332-333,364 (volumes shadow surface NEE). */
typedef struct vpt_volume {
    float corner_min[3];
    float corner_max[3];
    float color[3];              /* single-scattering albedo */
    float emissive_color[3];
    float density;               /* extinction per unit length */
    float anisotropy;            /* g of Henyey-Greenstein / Draine */
    float alpha;                 /* Draine alpha */
    float droplet_size;          /* HG+Draine fit parameter d (micrometres) */
    int32_t density_data_index;  /* -1: homogeneous; >= 0: a grid added with vpt_add_density_grid / _bricks */
    int32_t approximated_scattering;          /* ApproximatedScatteringForClouds: g^(1+depth), density * falloff^depth */
    float approximated_scattering_falloff;
    float grid_sharpness;                     /* GridSharpness (heterogeneous only) */
    /* Emission from temperature (Volume.slang:233-258).  Upstream the host writes the normalised temperature INTO the
     * density grid wherever it is positive (PathTracer.cpp:1444-1454) and the shader reads that same grid
     * (Volume.slang:238): has_temperature_data = 1 means "the grid attached to this volume is that merged grid". */
    int32_t has_temperature_data;
    int32_t use_blackbody;                    /* 1: Blackbody(kelvin), 0: temperature_color */
    float temperature_color[3];
    float temperature_gamma, temperature_scale, emissive_color_gamma;
    int32_t kelvin_min, kelvin_max;
} vpt_volume;
#define VPT_MAX_VOLUMES 32       /* the reference sorts into fixed float[100] / int[100] arrays (RayGen.slang:165-166) */
#define VPT_PHASE_HENYEY_GREENSTEIN 0        /* PathTracer.h:76-81 PhaseFunction */
#define VPT_PHASE_DRAINE 1
#define VPT_PHASE_HENYEY_GREENSTEIN_PLUS_DRAINE 2
/* AddVolume / RemoveVolume / SetVolume (PathTracer.h:157-159): the whole list is replaced; count 0 removes all
 * volumes.  Resets accumulation. */
int vpt_set_volumes(vpt_ctx* ctx, const vpt_volume* volumes, uint32_t count);
/* AddDensityDataToVolume (PathTracer.cpp:1347-1516) with the .vdb file already decoded by the caller: a dense grid of
 * raw densities over the active-voxel bounding box (x fastest, then y, then z, in the file's index order).  The library
 * does what the reference does after reading the file: MaxDensityInTheGrid, the 32x32x32 table of per-block maxima of
 * density / max used for empty-space skipping (y flipped "for Vulkan", :1425-1442), upload.  Lookups mirror
 * SampleNanoVDBBuffer (Volume.slang:69-117): position normalised in the box, y flipped, floor to a voxel, +-1 voxel
 * of random jitter per axis (three PCG draws), clamp to the grid.  Returns the grid's index (the value to put in
 * vpt_volume.density_data_index) or a negative VPT_ERR_*.  At most VPT_MAX_DENSITY_GRIDS grids. */
#define VPT_MAX_DENSITY_GRIDS 16
int vpt_add_density_grid(vpt_ctx* ctx, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, const float* density);
/* AddDensityDataToVolume (PathTracer.cpp:1347-1516) with the grid handed over as the NanoVDB tree holds it (nanovdb::LeafNode, the 8x8x8 nodes
 * SampleNanoVDBBuffer reads through its accessor, Volume.slang:69-117): brick_count bricks of VPT_BRICK_DIM^3 voxels and a background of 0.
 * The index box is [0, dim) as for vpt_add_density_grid; brick (bx, by, bz) covers voxels [8bx, 8bx + 8) x [8by, 8by + 8) x [8bz, 8bz + 8), its
 * 512 values x fastest, then y, then z.  Voxels of a brick outside the index box are ignored (never read, not part of any maximum); a voxel no
 * brick covers has density 0.  The grid IS the dense grid with those values: MaxDensityInTheGrid and the block maxima (:1425-1442) equal, bit for
 * bit, what vpt_add_density_grid computes from the equivalent dense array, and every later image is bit-identical to that grid's — but the dense
 * box is never formed, on the host or on the device: the work is proportional to brick_count and the device holds brick_count * 2 KB of values
 * plus one 32-bit word per brick cell.  Returns the grid's index, in the index space of vpt_add_density_grid (both kinds count towards
 * VPT_MAX_DENSITY_GRIDS and vpt_clear_density_grids frees both), or a negative VPT_ERR_*: VPT_ERR_INVALID_ARGUMENT for a NULL pointer, a zero
 * dimension, a brick coordinate at or beyond ceil(dim / 8), a coordinate given twice, brick_count == 0 or no positive value inside the box;
 * VPT_ERR_LIMIT for more than VPT_MAX_DENSITY_GRIDS grids, more than 2^26 brick cells or more than 2^22 bricks.  Waits for batches in flight; a
 * rejected or failed call leaves the list of grids as it was. */
#define VPT_BRICK_DIM 8u            /* a brick is 8 x 8 x 8 voxels = one NanoVDB leaf node */
int vpt_add_density_bricks(vpt_ctx* ctx, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z,
                           uint32_t brick_count, const uint32_t* brick_coords /* 3 per brick: bx, by, bz */,
                           const float* brick_values /* 512 per brick, x fastest, then y, then z */);
int vpt_clear_density_grids(vpt_ctx* ctx);   /* RemoveDensityDataFromVolume for all; volumes must not reference grids afterwards */
/* What a grid added with either call holds (the reference keeps the same facts per volume: the NanoVDB buffer's size and
 * MaxDensityInTheGrid, PathTracer.cpp:1416-1423). */
typedef struct vpt_density_grid_info {
    uint32_t dim[3];
    uint32_t brick_count;   /* 0: dense */
    uint64_t device_bytes;  /* values + brick table + block maxima */
    float max_density;
    uint32_t reserved;
} vpt_density_grid_info;
int vpt_get_density_grid_info(const vpt_ctx* ctx, uint32_t grid, vpt_density_grid_info* out);
/* Test hook, like vpt_trace_rays: the raw value the device lookup (SampleNanoVDBBuffer's accessor.getValue, Volume.slang:112) returns at n voxels
 * (ijk: 3 int32 each, host memory; clamped to the index box as the sampler clamps). */
int vpt_read_density_grid(vpt_ctx* ctx, uint32_t grid, const int32_t* ijk, uint32_t n, float* out_host);
/* SetPhaseFunction (PathTracer.h:106); default VPT_PHASE_HENYEY_GREENSTEIN (PathTracer.h:219).  Resets accumulation. */
int vpt_set_phase_function(vpt_ctx* ctx, uint32_t phase_function);
/* ---- atmosphere ----------------------------------------------------------------------
 * SetEnableAtmosphere + the planet / density setters (PathTracer.h:168-179; defaults :221-232; UBO fields
 * :276-288).  With an atmosphere the sky is no environment map: rays that leave the scene return black
 * (Miss.slang:11-14) and all sky light is in-scattered sunlight — delta-tracked scatter events on Rayleigh / Mie /
 * ozone profiles (Atmosphere.slang:131-201, RayGen.slang:212-262,382-470), ONE colour channel per path once it has
 * scattered (ColorChannel, RayGen.slang:120-129), sun-disk NEE (Sampler.slang:431-462; its direction comes from
 * sky_azimuth / sky_altitude) through ratio-tracked transmittance (Atmosphere.slang:33-107).  Units are metres.
 * Runs on the fused pipeline. */
typedef struct vpt_atmosphere {
    float planet_position[3];
    float planet_radius;
    float atmosphere_height;
    float rayleigh_density_falloff, mie_density_falloff, ozone_density_falloff, ozone_peak;
    float rayleigh_multiplier[3];   /* RayleighScatteringCoefficientMultiplier */
    float mie_multiplier[3];        /* MieScatteringCoefficientMultiplier */
    float ozone_multiplier[3];      /* OzoneAbsorptionCoefficientMultiplier */
    float sun_color[3];
} vpt_atmosphere;
void vpt_default_atmosphere(vpt_atmosphere* out);                       /* PathTracer.h:222-232 */
int vpt_set_atmosphere(vpt_ctx* ctx, const vpt_atmosphere* atmosphere); /* NULL: SetEnableAtmosphere(false). Resets accumulation. */
/* SetCameraViewInverse / SetCameraProjectionInverse. */
int vpt_set_camera(vpt_ctx* ctx, const float view_inverse[16], const float projection_inverse[16]);
/* The pixels a whole-path batch (VPT_PIPELINE_WHOLE) rendered now would start paths for: rect = {x0, y0, x1, y1}, inclusive, in pixels of the whole
 * image.  No camera ray of a pixel outside it can reach the scene's bounding box (the union of the BVH root's child boxes, projected through the
 * current camera and grown by two pixels), so such a sample is given its frame sum — exactly zero — without a path; images and vpt_stats are
 * what they are without the rectangle.  The whole image {0, 0, width - 1, height - 1} wherever that cannot be said: depth of field on, the camera
 * inside or beside the box, VPT_FLAG_FURNACE, an environment that is shown directly and is not black, a scene whose BVH does not ride in LDS, a
 * context that counts traversal steps (vpt_config.count_traversal), and a camera so far from the world's origin for its focus_distance (which
 * counts with depth of field off too: the focus point is rounded to fp32) that the rays' rounding may pass a pixel.
 * x0 > x1: no pixel can see the scene.  Reads the context only: it waits for nothing.  VPT_ERR_NO_SCENE before the first vpt_set_scene. */
int vpt_get_whole_cull(const vpt_ctx* ctx, uint32_t rect[4]);
/* All scalar setters + the #define toggles (PathTracer.cpp:1010-1015, 1623-1716). Resets accumulation — except when
 * max_samples is the only field that changed (SetMaxSamplesAccumulated keeps the image, PathTracer.cpp:1003-1006). */
int vpt_set_params(vpt_ctx* ctx, const vpt_params* params);
void vpt_default_params(vpt_params* params);
void vpt_default_post_params(vpt_post_params* params);
/* PathTracer::ResizeImage. */
int vpt_resize(vpt_ctx* ctx, uint32_t width, uint32_t height);
/* PathTracer::ResetPathTracing (PathTracer.h:183). */
int vpt_reset(vpt_ctx* ctx);

/* PathTracer::PathTrace x dispatches (PathTracer.cpp:122-156); blocking. *done (if non-NULL) is
 * PathTrace's return value: 1 once samples accumulated >= max_samples (then nothing is launched). */
int vpt_render(vpt_ctx* ctx, uint32_t dispatches, int* done);

/* ---- the reference's asynchronous per-frame shape --------------------------------------------------------------------
 * PathTracer::PathTrace(cmd) RECORDS the dispatch and returns (PathTracer.cpp:122-156); Editor::Draw calls it once and then
 * PostProcessor::PostProcess(cmd) every frame (Editor.cpp:116,129); both outputs stay on the device (PathTracer.h:94-95
 * GetOutputImage, PostProcessor GetOutputImageView) and the host waits on a fence of an EARLIER frame.  Same here:
 *   vpt_render_async      enqueues `dispatches` dispatches on the context's stream and returns; bookkeeping (frame count, *done) advances
 *                         at enqueue time as PathTrace's does.  *ticket (optional) identifies the work enqueued so far.
 *   vpt_postprocess_device the post chain behind it on the same stream, no synchronisation, RGBA8 left in the context's output image
 *                         (vpt_output_device) and, if rgba8_device != NULL, copied there device-to-device (an interop / swapchain image).
 *   vpt_wait(ticket)      blocks until that ticket's work has finished (0: everything enqueued so far).
 * When every path of a batch provably ends within max_depth * samples_per_frame bounces (no material scatters inside a medium, no
 * volumes / atmosphere) and that number is <= VPT_ASYNC_MAX_BOUNCES — or when the batch is ONE whole-path launch (VPT_PIPELINE_WHOLE, which
 * AUTO takes for LDS-resident scenes: every path runs to its end inside it, whatever max_depth is) — a batch is a fixed schedule: nothing in
 * it waits for the host, any number of frames can be in flight, and such a batch — the whole-path / fused pipelines', and the streams pipeline's ~7 launches
 * per bounce on one stream — is captured once as a hipGraph and replayed while nothing changes (vpt_stats.graph_launches).  Otherwise the enqueued part is the first VPT_ASYNC_MAX_BOUNCES bounces and the NEXT call on the context
 * (or vpt_wait) finishes the batch first, exactly as vpt_render would have.  Images are bit-identical to vpt_render's either way.
 * Every other entry point that reads or changes device state drains outstanding work first. */
#define VPT_ASYNC_MAX_BOUNCES 32u
int vpt_render_async(vpt_ctx* ctx, uint32_t dispatches, int* done, uint64_t* ticket);
int vpt_postprocess_device(vpt_ctx* ctx, const vpt_post_params* params, void* rgba8_device, uint64_t* ticket);
int vpt_wait(vpt_ctx* ctx, uint64_t ticket);
/* GetOutputImageView(): device pointer to the RGBA8 UNORM image of the last vpt_postprocess / vpt_postprocess_device (width*height*4 bytes,
 * owned by the context, valid until vpt_resize / vpt_destroy); NULL before the first post-process. */
const void* vpt_output_device(vpt_ctx* ctx);
/* The same image read back (waits for outstanding work): width*height*4 bytes to host memory.  VPT_ERR_INVALID_ARGUMENT before the first post-process. */
int vpt_get_output(vpt_ctx* ctx, uint8_t* rgba8_host);

/* GetOutputImage(): the RGBA32F accumulation image (alpha 1). Whole image (shard_count==1, or after
 * vpt_assemble_shards) to a caller-owned host / device buffer of width*height*4 floats. */
int vpt_get_radiance(vpt_ctx* ctx, float* rgba_host);
int vpt_get_radiance_device(vpt_ctx* ctx, void* rgba_device);
/* Checkpoint/resume hook: overwrite the accumulation image and frame counter. */
int vpt_set_radiance(vpt_ctx* ctx, const float* rgba_host, uint32_t frame_count);

/* Multi-GPU: this context's rows (y % shard_count == shard_rank), packed in increasing y, as
 * rows*width*4 floats in device memory (the buffer handed to the RCCL gather), and the inverse on
 * the gathering rank: `gathered` holds shard_count shards back to back, each padded to
 * vpt_shard_floats(ctx) floats. */
size_t vpt_shard_floats(const vpt_ctx* ctx);
int vpt_get_shard_device(vpt_ctx* ctx, void* shard_device);
int vpt_assemble_shards(vpt_ctx* ctx, const void* gathered_device, uint32_t shard_count);

/* The one collective of the path.  The reference's only image partition is the interleaved
 * split-screen chunking of RayGen.slang:16-25 / PathTracer.cpp:141-153; here shard r owns rows y % N == r and
 * the finished shards meet ONCE, on `root`, over xGMI.  Nothing else ever crosses devices.
 *   process per GPU (torchrun / mpirun launch): vpt_comm_unique_id() on one rank, the 128 bytes handed to the
 *     others out of band (any control plane), vpt_comm_init() = ncclCommInitRank on the context's device,
 *     vpt_comm_gather_shards() = ncclGather of the padded shards (vpt_shard_floats each) on the context's stream
 *     followed, on root, by the row re-interleave: root's vpt_get_radiance / vpt_postprocess then see the whole
 *     image.  rank must equal the context's shard_rank and world its shard_count.
 *   one process driving N devices (the C++ host, `vpt_render --gpus N`): vpt_multi_gather_shards() over the N
 *     contexts, shard k at index k: peer copies (hipMemcpyPeerAsync, direct xGMI links) into root + re-interleave.
 * Both return VPT_ERR_DEVICE with the RCCL / HIP message in vpt_last_error() on failure. */
#define VPT_COMM_ID_BYTES 128
int vpt_comm_unique_id(void* id_out);
int vpt_comm_init(vpt_ctx* ctx, const void* id, int rank, int world);
int vpt_comm_gather_shards(vpt_ctx* ctx, int root);
int vpt_comm_destroy(vpt_ctx* ctx);
/* What the communicator actually is: the RCCL the process has MAPPED (a host that loaded another librccl first — PyTorch ships its
 * own — gets that one behind this library's calls, whatever it was linked against), the one this library was compiled against,
 * and what RCCL itself reports for the communicator.  vpt_comm_init refuses (VPT_ERR_DEVICE) a mapped RCCL whose major version
 * differs from the compiled one.  Valid after vpt_comm_init; without a communicator nranks = 0 and only the versions / path are filled. */
typedef struct vpt_comm_info {
    int32_t rccl_version_runtime;   /* ncclGetVersion() of the mapped library, e.g. 22606 */
    int32_t rccl_version_compiled;  /* NCCL_VERSION_CODE of the headers this library was built with */
    int32_t nranks;                 /* ncclCommCount */
    int32_t rank;                   /* ncclCommUserRank */
    int32_t device;                 /* ncclCommCuDevice */
    int32_t reserved;
    char library_path[232];         /* file the ncclGather symbol in use comes from (dladdr) */
} vpt_comm_info;
int vpt_comm_get_info(vpt_ctx* ctx, vpt_comm_info* out);
/* "<PCI bus id>" of the context's device (e.g. 0000:05:00.0): lets the host's control plane refuse two ranks on one device before
 * ncclCommInitRank is entered (RCCL rejects that configuration itself, but only after its bootstrap has run). out: >= 32 bytes. */
int vpt_device_identity(vpt_ctx* ctx, char* out, uint32_t out_bytes);
int vpt_multi_gather_shards(vpt_ctx* const* ctxs, uint32_t count, uint32_t root);

/* PostProcessor::SetTonemappingData/SetBloomData + PostProcess (PostProcessor.cpp:193-246) on the
 * accumulation image: threshold -> (mip-1)x down -> (mip-1)x up -> tonemap. rgba8_host receives
 * GetOutputImageView() (RGBA8 UNORM, width*height*4 bytes); bloom0_host (optional) receives bloom
 * mip 0 after the up-sample chain (RGBA32F) for testing. */
int vpt_postprocess(vpt_ctx* ctx, const vpt_post_params* params, uint8_t* rgba8_host, float* bloom0_host);

int vpt_get_stats(vpt_ctx* ctx, vpt_stats* out);
int vpt_reset_stats(vpt_ctx* ctx);

/* Test hook on the extend kernel alone: closest hit of n rays (origin xyz, tmin, dir xyz, tmax —
 * 32 B each, host memory) -> n hits {t, u, v, primitive, instance} (20 B each). */
typedef struct vpt_ray { float origin[3]; float tmin; float direction[3]; float tmax; } vpt_ray;
typedef struct vpt_hit { float t; float u; float v; uint32_t primitive; uint32_t instance; } vpt_hit;
int vpt_trace_rays(vpt_ctx* ctx, const vpt_ray* rays_host, uint32_t n, vpt_hit* hits_host);

/* ---- picking and guide buffers ------------------------------------------------------------------------------------------
 * What the camera sees FIRST through every pixel: the inputs of a denoiser or an edge-aware filter (depth, shading normal, albedo)
 * and what an editor's viewport picks (instance, primitive, material, mesh).  The reference has no counterpart: its only such views
 * are the commented-out normal / validity outputs of ClosestHit.slang:69-71,206-218.  One kernel runs the integrator's camera-ray
 * closest-hit query (RayGen.slang:70: tmin 0.01, tmax 100000) and the head of ClosestHit.slang — SurfaceFrame (Surface.slang:26-147)
 * and Material.Initialize's base colour (Material.slang:44) — and stops there.
 *   camera and state  the current camera, flags (VPT_FLAG_LOCAL_HITS, _GEOMETRY_NORMALS, _FURNACE included), materials edited
 *                     (vpt_set_material) and instances moved (vpt_set_instance_transforms) since the scene was installed all apply.
 *   media             volumes and the atmosphere are ignored: the buffers describe the first SURFACE.
 *   coverage          always the WHOLE width x height image, on a shard context too (every context holds the whole scene).
 *   VPT_FEATURES_SAMPLE  the RNG state is the one the integrator gives sample 0 of pixel (x, y) in dispatch `frame`, the ray is the
 *                     integrator's camera ray (jitter and lens offset included), bit for bit.
 *   VPT_FEATURES_CENTER  the same expressions with both jitter draws equal to 0.5 and a zero lens offset; `frame` is ignored.
 *   side effects      waits for work in flight; does NOT reset or touch the accumulation, the frame counters or any vpt_stats field
 *                     (beyond the recount of stack_spills every traversal causes, as vpt_trace_rays does).
 *   errors            VPT_ERR_NO_SCENE before vpt_set_scene; VPT_ERR_INVALID_ARGUMENT for a NULL ctx or out, an unknown mode, all
 *                     four pointers NULL, or (vpt_pick) a pixel outside the image.  A failed call leaves the caller's buffers
 *                     unspecified and the context usable. */
#define VPT_FEATURES_CENTER 0u  /* the ray through the pixel centre, no lens offset */
#define VPT_FEATURES_SAMPLE 1u  /* the camera ray of sample 0 of dispatch `frame`, exactly as the integrator draws it */
typedef struct vpt_feature_buffers {   /* any pointer may be NULL: that buffer is not produced */
    float*    depth;   /* width*height     : t of the closest hit along the ray, -1 on a miss */
    uint32_t* ids;     /* width*height*4   : instance, primitive, material, mesh; 0xffffffff x4 on a miss */
    float*    normal;  /* width*height*4   : SurfaceFrame N (after normal map and the two corrections; Ng under VPT_FLAG_GEOMETRY_NORMALS), w = 1 inside / 0 outside; 0 on a miss */
    float*    albedo;  /* width*height*4   : Material.Initialize base colour at the hit's uv (1,1,1 under VPT_FLAG_FURNACE), w = transmission; 0 on a miss */
    uint32_t  device;  /* 0: host pointers; 1: device pointers on the context's device */
    uint32_t  reserved;
} vpt_feature_buffers;
int vpt_render_features(vpt_ctx* ctx, uint32_t mode, uint32_t frame, const vpt_feature_buffers* out);
/* The VPT_FEATURES_CENTER ray of ONE pixel: the same launch with one ray, so ids and t equal the CENTER buffers' at (x, y) bit for bit.
 * u, v: the hit's barycentrics; position = origin + t * direction.  A miss is VPT_OK with ids 0xffffffff, t = -1 and the rest 0. */
typedef struct vpt_pick_result { uint32_t instance, primitive, material, mesh; float t, u, v; float position[3]; } vpt_pick_result;
int vpt_pick(vpt_ctx* ctx, uint32_t x, uint32_t y, vpt_pick_result* out);   /* CENTER ray of one pixel; a miss is VPT_OK with ids 0xffffffff and t = -1 */

/* ---- denoising -----------------------------------------------------------------------------------------------------------
 * An edge-avoiding a-trous wavelet filter (Dammertz et al. 2010, as SVGF uses it) over the accumulation image, steered by the
 * VPT_FEATURES_CENTER guide images above, on the device, in the context's stream: what turns a 1-4 spp viewport frame into something
 * to show.  The reference has no counterpart.  Every call traces the guides anew (camera, scene, materials, instance transforms, flags
 * and size as they stand), prepares, and runs `iterations` passes of 5 x 5 taps at steps 1, 2, 4 ...; the arithmetic, tap by tap, is
 * csrc/denoise.hpp's, and the device result equals a host compile of that header bit for bit.
 *   hit pixels        e' = sum k w e / sum k w over the taps that are inside the image and hits; w = exp(-(dn + dz + dc)) with
 *                     dn = max(0, 1 - n_p.n_q) / sigma_normal, dz = |t_p - t_q| / (sigma_depth step max(t_p, 1e-6)),
 *                     dc = |e_p - e_q|^2 / (sigma_color 2^-pass)^2; w = 1 at the centre.
 *   VPT_DENOISE_DEMODULATE  the filter runs on colour / max(albedo, 1e-3) and the last pass multiplies it back: texture detail survives.
 *   miss pixels       (nothing hit: environment) keep their input bit for bit and are never a tap of another pixel.
 *   iterations == 0   the output is a copy of the input.
 *   non-finite input  propagates to every pixel whose weight for it is not exactly 0; there is no guard.
 *   result            an RGBA32F image kept in the context (alpha copied from the input) — a SNAPSHOT: later renders do not update it —
 *                     and, if the pointer is not NULL, copied to the caller (width*height*16 bytes; a device pointer 16-byte aligned).
 *   memory            on first use, 84 bytes per pixel (36 of guides, three RGBA32F images); re-made after vpt_resize.
 *   side effects      like vpt_render_features: the accumulation, the frame counters and vpt_stats are untouched (stack_spills is recounted).
 *   vpt_denoise       blocking.  vpt_denoise_device: enqueued behind the frames in flight like vpt_postprocess_device, with a ticket.
 *   errors            VPT_ERR_NO_SCENE before vpt_set_scene; VPT_ERR_INVALID_ARGUMENT for a NULL ctx or params, iterations >
 *                     VPT_DENOISE_MAX_ITERATIONS, a sigma that is not > 0, unknown flag bits, an unaligned device pointer, a sharded
 *                     context before vpt_assemble_shards.  A failed call leaves the context usable and the previous result valid.
 * vpt_set_post_source: which image vpt_postprocess / vpt_postprocess_device read.  VPT_POST_SOURCE_DENOISED: the latest denoised image;
 * without one of the current size (never denoised, or resized since) they return VPT_ERR_INVALID_ARGUMENT. */
#define VPT_DENOISE_DEMODULATE 1u
#define VPT_DENOISE_MAX_ITERATIONS 6u
typedef struct vpt_denoise_params {
    uint32_t iterations;
    float sigma_color, sigma_normal, sigma_depth;
    uint32_t flags;      /* VPT_DENOISE_* */
    uint32_t reserved;
} vpt_denoise_params;
void vpt_default_denoise_params(vpt_denoise_params* out);   /* 5 iterations, VPT_DENOISE_DEMODULATE, sigma_color 1 (in units of radiance), sigma_normal 0.1, sigma_depth 0.05 */
int vpt_denoise(vpt_ctx* ctx, const vpt_denoise_params* params, float* rgba_host);
int vpt_denoise_device(vpt_ctx* ctx, const vpt_denoise_params* params, void* rgba_device, uint64_t* ticket);
#define VPT_POST_SOURCE_RADIANCE 0u   /* the accumulation image (default) */
#define VPT_POST_SOURCE_DENOISED 1u   /* the image the latest vpt_denoise / vpt_denoise_device left in the context */
int vpt_set_post_source(vpt_ctx* ctx, uint32_t source);

/* ---- temporal accumulation -------------------------------------------------------------------------------------------------
 * SVGF's other half: the previous result is reprojected through the first-hit geometry of the current frame, kept where the same surface
 * is still seen, and the new samples are blended in — so a camera that moves does not start every frame from 1 spp.  The reference has no
 * counterpart: its accumulation restarts with every camera change, as vpt_set_camera still does.  On the device, in the context's stream;
 * the arithmetic is csrc/temporal.hpp's, and the device result equals a host compile of that header bit for bit.  The loop of a viewport:
 *     vpt_set_camera -> vpt_render(k) -> vpt_temporal_accumulate -> vpt_denoise -> vpt_postprocess
 *   a call            traces the VPT_FEATURES_CENTER guides anew (depth, normal, albedo, ids; camera, scene and flags as they stand, like
 *                     vpt_denoise), blends the accumulation image of m frames (m = the context's frame count at the call; for the _device
 *                     form at enqueue time) with the stored previous record, and makes the new record the previous one, with the camera it
 *                     was made with.  Calling twice without a vpt_reset / vpt_set_camera in between counts those m frames twice.
 *   hit pixels        X = the pixel's first hit; (fx, fy) = where the previous camera saw X; the four pixels around it are taps with their
 *                     bilinear weights b.  A tap counts when it is inside the image, was a hit, |t_q - |X - o_prev|| <= depth_tolerance
 *                     |X - o_prev|, n_p.n_q >= normal_threshold and (VPT_TEMPORAL_MATCH_INSTANCE) has the pixel's instance id.  With
 *                     sum b > 0.01 there is a history: hist = sum b hist_q / sum b, n = sum b len_q / sum b, n' = min(n + m, max_history),
 *                     out = hist + (cur - hist) min(m / n', 1), length n' — where that factor is 1 (m alone reaches max_history) out is cur
 *                     itself, not the rounding of the expression, so max_history = 1 gives exactly the result without history.  Otherwise
 *                     out = cur, length min(m, max_history).  A point behind the previous camera (clip w <= 0) or a singular previous
 *                     camera has no history.
 *   VPT_TEMPORAL_DEMODULATE  history and blend are of colour / max(albedo, 1e-3); the image handed out is multiplied by that of the current pixel.
 *   miss pixels       keep their input bit for bit, have length 0 and are never a tap.
 *   non-finite input  propagates into the result and the history; there is no guard.
 *   result            an RGBA32F image kept in the context (alpha copied from the input) — a SNAPSHOT — and, if the pointer is not NULL, copied
 *                     to the caller (width*height*16 bytes; a device pointer 16-byte aligned).  vpt_get_temporal_history: the history
 *                     length of the latest result, width*height floats (a test hook and a debug view).
 *   history           survives vpt_set_camera, vpt_reset, renders, vpt_denoise*, vpt_render_features, vpt_pick and the post calls.  It is
 *                     dropped by everything else that resets the accumulation or changes what a pixel means — vpt_set_scene,
 *                     vpt_set_material, vpt_set_instance_transforms (count > 0), vpt_set_environment, the volume, density-grid,
 *                     phase-function and atmosphere calls, a vpt_set_params that resets, vpt_set_radiance, vpt_resize — and by
 *                     vpt_temporal_reset; the next call then has no history anywhere.  Moving an instance drops the history unless
 *                     vpt_temporal_options.instance_motion is 1 (below): then it is reprojected through the instance's previous transform.
 *   memory            on first use, 124 bytes per pixel: the result (16), two records of history (r, g, b, length: 16), packed guide (n.xyz,
 *                     t: 16) and instance id (4), and 36 of guides (albedo 16, ids 16, depth 4); re-made after vpt_resize.
 *   side effects      like vpt_denoise: the accumulation, the frame counters and vpt_stats are untouched (stack_spills is recounted).
 *   vpt_temporal_accumulate  blocking.  vpt_temporal_accumulate_device: enqueued behind the frames in flight like vpt_denoise_device, with a ticket.
 *   errors            VPT_ERR_NO_SCENE before vpt_set_scene; VPT_ERR_INVALID_ARGUMENT for a NULL ctx or params, max_history == 0, a
 *                     depth_tolerance that is not > 0, a normal_threshold outside [-1, 1] (or NaN), unknown flag bits, non-zero reserved
 *                     words, an unaligned device pointer, a sharded context before vpt_assemble_shards, nothing rendered since the last
 *                     reset (m == 0); for vpt_set_denoise_source a NULL ctx or an unknown source; for vpt_get_temporal_history a NULL
 *                     argument or no result of the current size.  A failed call leaves the context usable and the previous history and
 *                     result valid.
 * vpt_set_denoise_source: which image vpt_denoise / vpt_denoise_device filter.  VPT_DENOISE_SOURCE_TEMPORAL: the latest temporal image
 * (iterations == 0 copies it, so the post chain reaches it through VPT_POST_SOURCE_DENOISED); without one of the current size they return
 * VPT_ERR_INVALID_ARGUMENT. */
#define VPT_TEMPORAL_DEMODULATE     1u
#define VPT_TEMPORAL_MATCH_INSTANCE 2u
typedef struct vpt_temporal_params {
    uint32_t max_history;     /* cap of the history length, in frames; >= 1 */
    float depth_tolerance;    /* relative; > 0 */
    float normal_threshold;   /* cosine; in [-1, 1] */
    uint32_t flags;           /* VPT_TEMPORAL_* */
    uint32_t reserved[2];
} vpt_temporal_params;
void vpt_default_temporal_params(vpt_temporal_params* out);   /* max_history 32, depth_tolerance 0.02, normal_threshold 0.9, both flags */
int vpt_temporal_accumulate(vpt_ctx* ctx, const vpt_temporal_params* params, float* rgba_host);
int vpt_temporal_accumulate_device(vpt_ctx* ctx, const vpt_temporal_params* params, void* rgba_device, uint64_t* ticket);
int vpt_temporal_reset(vpt_ctx* ctx);                              /* drop the history; the next call starts afresh */
int vpt_get_temporal_history(vpt_ctx* ctx, float* length_host);    /* VPT_ERR_INVALID_ARGUMENT without a result of the current size */
#define VPT_DENOISE_SOURCE_RADIANCE 0u   /* the accumulation image (default) */
#define VPT_DENOISE_SOURCE_TEMPORAL 1u   /* the image the latest vpt_temporal_accumulate / _device left in the context */
int vpt_set_denoise_source(vpt_ctx* ctx, uint32_t source);

/* ---- SVGF: reseeding, luminance variance, variance-guided a-trous ------------------------------------------------------------------
 * What turns the two calls above into SVGF (Schied et al. 2017).  The loop of a viewport:
 *     vpt_set_camera -> vpt_set_base_seed(frame_index) -> vpt_render(k) -> vpt_temporal_accumulate -> vpt_denoise -> vpt_postprocess
 * vpt_set_base_seed: vpt_params.base_seed and nothing else.  Every vpt_set_camera restarts the accumulation at dispatch 0, so without a new
 *                     seed every frame of a moving viewport draws the same random numbers per pixel and the history averages the same noise.
 *                     The accumulation restarts as after vpt_set_camera: the temporal history SURVIVES (vpt_set_params would drop it).  Waits
 *                     for work in flight; a captured batch is not replayed with the old seed.  Afterwards the context renders, bit for bit,
 *                     what a context given that seed through vpt_set_params renders (vpt_render_features in VPT_FEATURES_SAMPLE mode included).
 *                     Setting the seed it already has still restarts the accumulation.  VPT_ERR_INVALID_ARGUMENT for a NULL ctx.
 * vpt_set_svgf_options: context state, like vpt_set_denoise_source.  With variance == 0 (default) every call returns the bits it returned
 *                     without these options, and nothing more is allocated or launched.  With variance == 1:
 *   vpt_temporal_accumulate*  keeps, beside the colour record, the first and second moment (mu1, mu2) of the luminance l = (0.2126 r + 0.7152 g)
 *                     + 0.0722 b of the colour the blend takes in (demodulated under VPT_TEMPORAL_DEMODULATE): reprojected over the same counted
 *                     taps with the same weights, blended with the colour's own factor — mu' = h + (new - h) a, the new value (l, l l) itself
 *                     where a is 1 or there is no history — and writes a variance image: max(0, mu2 - mu1 mu1) where the pixel's new
 *                     history length is >= min_history * m, -1 ("unknown") where it is shorter, 0 on a miss (whose moments are (0, 0)).  Image
 *                     and history length keep their bits.  The moments share every fate of the history.
 *   vpt_denoise*      with VPT_DENOISE_SOURCE_TEMPORAL (with VPT_DENOISE_SOURCE_RADIANCE the option is ignored): the variance v rides through
 *                     the passes beside the colour.  A pixel with v_p < 0 is filtered by the fixed-sigma_color rule above, tap for tap, and
 *                     stays at -1.  Otherwise g = the 3 x 3 Gaussian (1/4, 1/8, 1/16) of v over the pixels at distance 1 (whatever the
 *                     step) that are inside the image, hits and have v >= 0, normalised by the weights that counted; taps with v_q < 0 are
 *                     skipped; w = exp(-(dn + dz + dl)) with dl = |lum(e_p) - lum(e_q)| / (sigma_luminance sqrt(g) + 1e-6), w = 1 at the
 *                     centre; e' = sum k w e / sum k w and v' = sum (k w)^2 v / (sum k w)^2.  The last pass re-modulates and returns the
 *                     source's alpha; iterations == 0 stays a copy.  The arithmetic is csrc/denoise.hpp's atrous_pixel_variance; the taps
 *                     of every step are read from memory.
 *   memory            20 bytes per pixel more on the first temporal call with the option on (two moment records, the variance image).
 *   changing `variance`  drops the temporal history, like vpt_temporal_reset.
 *   errors            VPT_ERR_INVALID_ARGUMENT for a NULL argument, a variance other than 0 or 1, a sigma_luminance that is not > 0,
 *                     min_history == 0, a non-zero reserved word; for vpt_denoise* when the option is on, the source is the temporal image and
 *                     the latest temporal result was made with the option off; for the two read-backs (test hooks and debug views) a NULL
 *                     argument or no temporal result of the current size made with variance == 1. */
typedef struct vpt_svgf_options {
    uint32_t variance;        /* 0 (default): off, everything as without these options.  1: on */
    float    sigma_luminance; /* SVGF's sigma_l; default 4; > 0 */
    uint32_t min_history;     /* images a pixel's moments must hold before its variance is trusted; default 4; >= 1 */
    uint32_t reserved;        /* 0 */
} vpt_svgf_options;
int vpt_set_base_seed(vpt_ctx* ctx, uint32_t base_seed);
void vpt_default_svgf_options(vpt_svgf_options* out);   /* variance 0, sigma_luminance 4, min_history 4 */
int vpt_set_svgf_options(vpt_ctx* ctx, const vpt_svgf_options* options);
int vpt_get_svgf_options(const vpt_ctx* ctx, vpt_svgf_options* out);
int vpt_get_temporal_variance(vpt_ctx* ctx, float* var_host);   /* width*height floats */
int vpt_get_temporal_moments(vpt_ctx* ctx, float* mu_host);     /* width*height*2 floats: mu1, mu2 per pixel */

/* ---- SVGF: the variance of young pixels from their neighbourhood ------------------------------------------------------------------------
 * The variance image above is -1 wherever a hit pixel's new history length is below min_history * m — such a pixel is YOUNG: every pixel of the
 * first min_history images after a reset or a scene edit, and the band a moving camera or a moved instance uncovers, every frame — and vpt_denoise*
 * filters those with the fixed-sigma_color rule.  SVGF (Schied et al. 2017, §4.2) estimates their variance spatially instead.
 * vpt_set_svgf_spatial_options: context state, like vpt_set_svgf_options; the call only validates and stores, and does NOT drop the temporal
 *                     history (it touches no record).  With vpt_svgf_options.variance == 0 it is stored and ignored.  With mode == 0 (default)
 *                     every call returns the bits it returned without these options, and nothing more is launched.  With mode == 1 and variance == 1:
 *   vpt_temporal_accumulate*  runs one more launch behind the temporal one, on the same stream.  Per young pixel p, over the (2 radius + 1)^2 window
 *                     around it, rows then columns: a tap q outside the image or on a miss is skipped; the centre has weight 1; any other tap, at
 *                     ring r = max(|dx|, |dy|), has w = exp(-(dn + dz)) with dn = max(0, 1 - dot(n_p, n_q)) / sigma_normal and dz = |t_p - t_q| /
 *                     (sigma_depth r max(t_p, 1e-6)).  sw = sum w, M1 = sum w mu1_q / sw, M2 = sum w mu2_q / sw over the moments the call has just
 *                     written.  The pixel's variance becomes max(0, M2 - M1 M1) where sw >= min_weight and stays -1 where it is not (too little of
 *                     the window is this surface).  The instance id is not tested, and there is no history-length boost: long-lived neighbours
 *                     bring their temporal moments, history-less ones (l, l l), and both estimate the per-call variance the temporal one estimates.
 *                     The arithmetic is csrc/svgf_spatial.hpp's spatial_variance_pixel.
 *   what survives     everything but the variance image at young pixels: image, record, moments, history length, motion image and the variance of
 *                     every other pixel (misses: 0) keep their bits.  The variance image is not history: nothing feeds back into the next call.
 *   vpt_denoise*      is unchanged: a young pixel now enters the passes with a variance >= 0 and takes the variance-guided rule.
 *   memory            none.
 *   errors            VPT_ERR_INVALID_ARGUMENT for a NULL argument, mode > 1, a radius outside 1..3, a sigma that is not finite or not > 0, a
 *                     min_weight that is not finite or below 1, a non-zero reserved word.  A refused call changes nothing. */
typedef struct vpt_svgf_spatial_options {
    uint32_t mode;         /* 0 (default): off — every call returns the bits it returned before, nothing more is launched.  1: on */
    uint32_t radius;       /* 1..3; default 3 (7 x 7) */
    float    sigma_normal; /* default 0.1; > 0 */
    float    sigma_depth;  /* default 0.05; > 0 */
    float    min_weight;   /* least sum of tap weights that is an estimate; default 4; >= 1 */
    uint32_t reserved[3];  /* 0 */
} vpt_svgf_spatial_options;
void vpt_default_svgf_spatial_options(vpt_svgf_spatial_options* out);   /* mode 0, radius 3, sigma_normal 0.1, sigma_depth 0.05, min_weight 4 */
int vpt_set_svgf_spatial_options(vpt_ctx* ctx, const vpt_svgf_spatial_options* options);
int vpt_get_svgf_spatial_options(const vpt_ctx* ctx, vpt_svgf_spatial_options* out);

/* ---- outlier ("firefly") rejection ahead of the two filters -------------------------------------------------------------------------------
 * One 1-spp spike on a dark wall enters the temporal history and stays for max_history images, inflates its own second moment so that the
 * variance-guided rule widens around it, is spread into a 5 x 5 blot by every a-trous pass and drags the exposure histogram's top bin.  The
 * integrator's max_luminance clamp is global: a pixel at 400 on a wall whose neighbours sit at 0.3 passes it untouched.
 * vpt_set_firefly_options: context state, like vpt_set_svgf_spatial_options; the call only validates and stores, and does NOT drop the temporal
 *                     history (it touches no record).  With mode == 0 (default) every call returns the bits it returned without these options and
 *                     nothing is allocated or launched.  With mode == 1 one image pass runs ahead of the filter and the filter reads ITS output:
 *   vpt_temporal_accumulate*  between the first-hit guides and the temporal launch, on the accumulation image; demodulate = VPT_TEMPORAL_DEMODULATE.
 *   vpt_denoise*      from VPT_DENOISE_SOURCE_RADIANCE with iterations > 0 only, between the guides and the prepare pass; demodulate =
 *                     VPT_DENOISE_DEMODULATE.  From VPT_DENOISE_SOURCE_TEMPORAL the filter has already run ahead of the history and is not run
 *                     again; iterations == 0 stays a copy of the unfiltered source; vpt_postprocess* from VPT_POST_SOURCE_RADIANCE is untouched.
 *   the rule          l(q) = luminance (0.2126, 0.7152, 0.0722) of the pixel as the filter sees it: c.rgb / max(albedo, 1e-3) when the call
 *                     demodulates, c.rgb otherwise.  A miss keeps its bits and is never a tap.  A hit pixel p looks at the (2 radius + 1)^2 window
 *                     without its centre: a tap counts when it is inside the image, a hit and l_q >= 0 (a NaN is no tap, +inf is one); n = the
 *                     counted taps, L = the rank-th largest counted luminance.  n < rank: untouched.  limit = max(threshold L, floor); l_p > limit:
 *                     rgb is multiplied by limit / l_p, alpha kept (CLAMPED); otherwise untouched — a NaN centre too.  A hit with n >= rank is
 *                     CONSIDERED.  No guard beyond that: a +inf centre over a finite limit gets 0 in its finite channels and NaN in its infinite
 *                     ones.  The arithmetic is csrc/firefly.hpp's firefly_pixel.
 *   two limits        The clamp REMOVES energy — it is a bias: the mean of the filtered images lies below the unfiltered mean.  And an emitter ONE
 *                     pixel wide has no neighbour as bright as itself: it is dimmed to threshold x its surroundings; floor is the lever for that —
 *                     nothing at or below floor is ever touched.
 *   what survives     the accumulation image (vpt_get_radiance) keeps its bits: the pass writes an image of its own.  vpt_stats is untouched.
 *   vpt_get_firefly_state  of the latest filtered call: clamped and considered pixels, and the filtered calls since mode went to 1.  VPT_OK with
 *                     zeros before the first filtered call of the current size.
 *   vpt_get_firefly_image  the filtered image of the latest filtered call, width*height*4 floats; VPT_ERR_INVALID_ARGUMENT before the first one
 *                     of the current size.  Both read-backs wait for the work in flight.
 *   memory            16 B per pixel and 8 KB of counters: allocated by the first filtered call, re-made after vpt_resize, freed by vpt_destroy.
 *   sharded contexts  vpt_denoise's rule: the calls need vpt_assemble_shards first and filter the whole image.
 *   errors            VPT_ERR_INVALID_ARGUMENT for a NULL argument, mode > 1, a radius outside 1..2, a rank outside 1..3 (every window holds at
 *                     least 8 taps, so no rank in range exceeds it), a threshold that is not finite or below 1, a floor that is not finite or below
 *                     0, a non-zero reserved word.  A refused call changes nothing. */
typedef struct vpt_firefly_options {
    uint32_t mode;         /* 0 (default): off — every call returns the bits it returned before; nothing allocated or launched.  1: on */
    uint32_t radius;       /* 1..2; default 1 (3 x 3) */
    uint32_t rank;         /* 1..3; default 2 */
    float    threshold;    /* default 2; finite, >= 1 */
    float    floor;        /* default 1 (radiance units, like sigma_color); finite, >= 0 */
    uint32_t reserved[3];  /* 0 */
} vpt_firefly_options;
typedef struct vpt_firefly_state {
    uint64_t clamped;      /* pixels the latest filtered call scaled down */
    uint64_t considered;   /* hit pixels with at least rank counted neighbours */
    uint32_t calls;        /* filtered calls since mode went to 1 */
    uint32_t reserved;
} vpt_firefly_state;
void vpt_default_firefly_options(vpt_firefly_options* out);   /* mode 0, radius 1, rank 2, threshold 2, floor 1 */
int vpt_set_firefly_options(vpt_ctx* ctx, const vpt_firefly_options* options);
int vpt_get_firefly_options(const vpt_ctx* ctx, vpt_firefly_options* out);
int vpt_get_firefly_state(vpt_ctx* ctx, vpt_firefly_state* out);
int vpt_get_firefly_image(vpt_ctx* ctx, float* rgba_host);    /* width*height*4 floats */

/* ---- the temporal history across instance moves -------------------------------------------------------------------------------------
 * The loop of an animated viewport:
 *     vpt_set_instance_transforms -> vpt_set_base_seed(frame_index) -> vpt_render(k) -> vpt_temporal_accumulate -> vpt_denoise -> vpt_postprocess
 * vpt_set_temporal_options: context state, like vpt_set_svgf_options.  With instance_motion == 0 (default) every call returns the bits it
 *                     returned without these options, nothing more is allocated, uploaded or launched, a move drops the history, and
 *                     vpt_get_temporal_motion answers VPT_ERR_INVALID_ARGUMENT.  With instance_motion == 1:
 *   vpt_set_instance_transforms  a call with count > 0 that succeeds restarts the accumulation the way vpt_set_camera does: the history, the
 *                     moments and the stored previous camera survive.  A rejected or failed call changes nothing.
 *   previous transform  of an instance: the matrix it had when the latest temporal record was made, however many moves lie between —
 *                     two moves compose, a move there and back is no move.  Only the moved instances' matrices are kept.
 *   vpt_temporal_accumulate*  compares previous and current matrix byte for byte, per instance.  Where none differs the call is the one above.
 *                     Otherwise, per instance on the host in double, rounded to float once: D = M_prev M_cur^-1 and nt = the inverse transpose
 *                     of D's upper 3 x 3.  A hit pixel of a moved instance uses Xp = D (X, 1) — where its surface WAS — for X in the clip
 *                     transform and in the depth |Xp - o_prev|, and normalize(nt n_p) for n_p in the normal test; the instance test, the
 *                     weights, the blend, the moments and the variance are untouched.  An instance whose M_cur or D is singular or not
 *                     finite has no history; nothing else is affected.  The arithmetic is csrc/temporal.hpp's temporal_pixel_motion.
 *   vpt_get_temporal_motion  width*height*2 floats: (fx - x, fy - y) per pixel — where the previous image saw the pixel's surface, minus the
 *                     pixel's own coordinates — on hit pixels for which (fx, fy) was computed (a previous record, clip w > 0, an instance
 *                     with a history), (0, 0) elsewhere.  A debug view and test hook, and what a host's own TAA or upscaler wants.  Valid
 *                     for a result of the current size made with the option on.
 *   the limit         a reprojection follows the surface, not the light: the history of a pixel NEAR a moved object still carries the old
 *                     lighting — its shadow and its reflection lag by up to max_history frames.  This is SVGF's behaviour too.
 *   memory            8 bytes per pixel (the motion image) on the first temporal call with the option on, and two tables of 112 bytes per
 *                     instance on the first call after a move; freed with the temporal records.
 *   changing `instance_motion`  drops the temporal history, like vpt_temporal_reset.  Everything that drops the history without the option
 *                     still drops it, and forgets the previous transforms.
 *   errors            VPT_ERR_INVALID_ARGUMENT for a NULL argument, instance_motion > 1, a non-zero reserved word; a refused call changes
 *                     nothing. */
typedef struct vpt_temporal_options {
    uint32_t instance_motion;   /* 0 (default): a move drops the history.  1: the history is reprojected through the move */
    uint32_t reserved[3];       /* 0 */
} vpt_temporal_options;
void vpt_default_temporal_options(vpt_temporal_options* out);   /* instance_motion 0 */
int vpt_set_temporal_options(vpt_ctx* ctx, const vpt_temporal_options* options);
int vpt_get_temporal_options(const vpt_ctx* ctx, vpt_temporal_options* out);
int vpt_get_temporal_motion(vpt_ctx* ctx, float* motion_host);   /* width*height*2 floats */

/* ---- auto-exposure: luminance histogram metering ahead of the tonemap ------------------------------------------------------------------
 * vpt_post_params.exposure is a constant the host chooses without seeing the image; swapping the environment, moving an emitter or flying from
 * the lamp into the shadow changes the mean radiance by orders of magnitude.  With the option on, every vpt_postprocess / vpt_postprocess_device
 * meters its source image on the device and the tonemap follows — nothing is read back, nothing is waited for, any number of frames can be in
 * flight.  The reference has no counterpart.  The loop of a viewport ends as before, the exposure following the image:
 *     ... -> vpt_temporal_accumulate -> vpt_denoise -> vpt_postprocess
 * vpt_set_exposure_options: context state, like vpt_set_post_source and vpt_set_svgf_options; the call only validates and stores.  With mode == 0
 *                     (default) every call returns the bits it returned without these options, and nothing is allocated or launched.  With mode == 1
 *                     a post-process call first runs two more launches on the context's stream; the arithmetic is csrc/exposure.hpp's, the sums
 *                     are of integers, and the device result equals a host compile of that header bit for bit.
 *   histogram         256 bins over the post source (the accumulation image, or the denoised one under VPT_POST_SOURCE_DENOISED) BEFORE bloom, of
 *                     l = (0.2126 r + 0.7152 g) + 0.0722 b; alpha is ignored.  Bin 0, the black bin: l zero, negative or NaN — it never takes part
 *                     in the average, so a black environment or miss pixels do not drag the exposure.  Bin 255: l infinite, or at or above
 *                     2^max_log2.  Bin 1 also holds everything below 2^min_log2.  Otherwise 1 + floor((log2 l - min_log2) 254 / (max_log2 - min_log2)).
 *   metering          N = the pixels in bins 1..255.  In order of luminance, the pixels [lo, hi) are averaged: lo = (N rint(low_percentile 65536)) >> 16,
 *                     hi = min(max((N rint(high_percentile 65536)) >> 16, lo + 1), N).  avg_log2 = min_log2 + (their mean bin - 0.5) (max_log2 -
 *                     min_log2) / 254, and target_log2 = clamp(log2 key - avg_log2 + compensation_log2, min_exposure_log2, max_exposure_log2).
 *   adaptation        the first metering after mode went to 1 or after vpt_exposure_reset sets cur_log2 = target_log2.  Every other one blends:
 *                     cur += (target - cur) a with a = rate_up where the target is brighter (larger) and rate_down where it is darker; where a is 1,
 *                     cur is the target itself, not the rounding of the expression.  A metering with N == 0 (an all-black image) has no target and
 *                     leaves cur_log2, target_log2 and avg_log2 as they are; if nothing has been metered with a target yet, cur_log2 is 0, valid stays
 *                     0 and the next metering with a target jumps.  scale = 2^cur_log2.
 *   the tonemap       multiplies by exposure * scale — vpt_post_params.exposure times the adapted scale, the product formed once in fp32 — where it
 *                     multiplied by exposure; both schedules, both bloom taps.  Bloom threshold and strength act on the unexposed image, as before.
 *   two calls         on the same image meter twice and adapt twice, as two vpt_temporal_accumulate calls count their frames twice.
 *   the state         is a scalar about the scene's brightness: it survives vpt_resize, vpt_set_camera, vpt_reset, scene edits and everything else
 *                     except a change of `mode` (which starts it afresh, meterings included) and vpt_exposure_reset.  Changing only rates, key,
 *                     percentiles, range or clamps keeps it, so a host can set time-based rates every frame.
 *   vpt_get_exposure_state  waits for the work in flight like the other read-backs.  With mode == 0, or before the first metering, it is VPT_OK
 *                     with scale = 1 and everything else 0.  vpt_get_exposure_histogram: the 256 counts of the latest metering (a test hook and a
 *                     debug view); VPT_ERR_INVALID_ARGUMENT before the first metering.
 *   vpt_stats         the two launches are counted and (profile) timed under VPT_K_TONEMAP.
 *   memory            2.1 KB on the device, allocated by the first metering and kept until vpt_destroy.
 *   errors            VPT_ERR_INVALID_ARGUMENT for a NULL argument, a field that is not finite, a violated constraint below, a non-zero reserved
 *                     word.  A refused call changes nothing and leaves the context usable. */
typedef struct vpt_exposure_options {
    uint32_t mode;              /* 0 (default): off — every call returns the bits it returned without these options, nothing allocated or launched. 1: on */
    float min_log2, max_log2;   /* luminance range of the histogram, log2; defaults -10, 6; min < max, both finite */
    float low_percentile, high_percentile; /* trimmed mean; defaults 0.5, 0.95; 0 <= low < high <= 1 */
    float key;                  /* luminance the average is mapped to; default 0.18; > 0 */
    float compensation_log2;    /* default 0 */
    float min_exposure_log2, max_exposure_log2; /* clamp of the result; defaults -8, 8; min <= max */
    float rate_up, rate_down;   /* blend per metering towards a brighter / darker exposure, in (0, 1]; defaults 0.1, 0.25; 1 = at once */
    uint32_t reserved;          /* 0 */
} vpt_exposure_options;
typedef struct vpt_exposure_state {
    float scale, cur_log2, target_log2, avg_log2;
    uint32_t valid, meterings;  /* valid: a metering with a target has set cur_log2; meterings: post-process calls metered since mode went to 1 */
    uint64_t counted;           /* N of the latest metering */
} vpt_exposure_state;
void vpt_default_exposure_options(vpt_exposure_options* out);
int vpt_set_exposure_options(vpt_ctx* ctx, const vpt_exposure_options* options);
int vpt_get_exposure_options(const vpt_ctx* ctx, vpt_exposure_options* out);
int vpt_get_exposure_state(vpt_ctx* ctx, vpt_exposure_state* out);
int vpt_get_exposure_histogram(vpt_ctx* ctx, uint32_t out[256]);
int vpt_exposure_reset(vpt_ctx* ctx);   /* the next metering jumps to its target */

/* ---- energy-compensation lookup tables -------------------------------------------
 * Replaces LookupTableCalculator::CalculateTable(tableSize, sampleCount) (LookupTableCalculator.cpp:44-157)
 * with its shaders LookupReflect.slang / LookupRefract.slang (+ ABOVE_SURFACE / BELOW_SURFACE): sampleCount/20
 * passes of 20 samples per cell, pass i seeded with PCG(i*2 + sampleCount + PCG(time_ms)), summed in pass
 * order and divided by the pass count.  The reference puts wall-clock milliseconds into time_ms (one reading
 * per pass); here it is one caller-chosen value, so a table is reproducible.  Application.cpp:41,54,67 use
 * sizes 64x64x32 (reflect) and 128x128x32 (refract) with 10'000'000 samples.
 * out_host receives size_x*size_y*size_z floats, x fastest.  Needs no context (runs on `device`).
 * Known disagreement with the shipped tables (tests/test_oracle_lut_fp64.py): in the grazing near-mirror corner of
 * the two refraction tables (rows y <= 4 with x <= 31, and layer z = 0) this generator — like a float64 evaluation of the same
 * algorithm — gives 0.896 where Assets/LookupTables/RefractionLookup*.bin hold 0.819.  Everywhere else the generated tables match the
 * shipped ones within Monte-Carlo error.  Rendering is unaffected: the integrator consumes whichever tables vpt_set_scene is given. */
#define VPT_LUT_REFLECT 0
#define VPT_LUT_REFRACT_ABOVE 1
#define VPT_LUT_REFRACT_BELOW 2
int vpt_lut_calculate(int device, uint32_t kind, uint32_t size_x, uint32_t size_y, uint32_t size_z, uint32_t sample_count,
                      uint32_t time_ms, float* out_host);

#ifdef __cplusplus
}
#endif
#endif /* VPT_H */
