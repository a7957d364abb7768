/*
 * lsr.h -- C ABI of the MI355X-native LangSplat Gaussian rasterizer (liblsr.so).
 *
 * This is the drop-in boundary for the hot path named in BASELINE.json "north_star": the
 * forward and backward of RasterizeGaussians.  Each entry point replaces one native entry of
 * the reference's (absent) submodules/langsplat-rasterization extension, whose Python face
 * is used at:
 *
 *   reference interface (call site)                              replaced by
 *   ------------------------------------------------------------ ---------------------------
 *   _C.rasterize_gaussians            (called via GaussianRasterizer.forward,
 *                                      gaussian_renderer/__init__.py:96-105)        lsr_forward
 *   _C.rasterize_gaussians_backward   (autograd backward of the same call;
 *                                      train.py:104 loss.backward())                lsr_backward
 *   _C.mark_visible                   (GaussianRasterizer.markVisible; upstream API,
 *                                      unused by the reference scripts)             lsr_mark_visible
 *   C++ exception text -> RuntimeError (upstream error path)        lsr_last_error
 *
 * Conventions:
 *   - All array pointers are DEVICE pointers to contiguous fp32/int32 data, borrowed for the
 *     duration of the call.  Outputs are written in full; callers never need to pre-zero.
 *   - Matrices are the reference's row-vector matrices stored row-major, exactly the memory of
 *     Camera.world_view_transform / full_proj_transform (scene/cameras.py:54-56).
 *   - Work is enqueued on `stream` (a hipStream_t; NULL = legacy default stream).  lsr_forward
 *     waits once for the device to learn num_rendered (as upstream does) -- except in capacity mode
 *     (lsr_forward_args.capacity_rendered > 0), which sizes everything from caller capacities and
 *     never waits, so that a whole train step can be captured into a HIP graph.
 *   - Scratch is owned by the caller and requested through `alloc` (upstream's resizable
 *     geometry/binning/image buffers).  The three forward buffers must be kept alive, unchanged,
 *     and passed back to lsr_backward.
 *   - Return value: LSR_OK or an error code; lsr_last_error() describes the last failure on the
 *     calling thread.  The only process-wide state is the opt-in kernel profiler below (off by
 *     default, mutex-protected); rasterization itself is re-entrant.
 */
#ifndef LSR_H
#define LSR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSR_ABI_VERSION 18

enum lsr_status {
    LSR_OK = 0,
    LSR_ERR_INVALID = 1,     /* bad argument (null pointer, negative size, ...) */
    LSR_ERR_HIP = 2,         /* a HIP runtime call or kernel launch failed */
    LSR_ERR_ALLOC = 3,       /* the alloc callback returned NULL */
    LSR_ERR_PREFILTERED = 4  /* prefiltered=1 but a Gaussian failed the frustum test */
};

/* Scratch buffers requested through the allocator (upstream geomBuffer/binningBuffer/imgBuffer) */
enum lsr_buffer {
    LSR_BUF_GEOM = 0,     /* per Gaussian; forward -> backward */
    LSR_BUF_BINNING = 1,  /* per tile instance; forward -> backward */
    LSR_BUF_IMAGE = 2,    /* per pixel / per tile; forward -> backward */
    LSR_BUF_BACKWARD = 3, /* per Gaussian gradient scratch, backward only */
    LSR_BUF_LEVELS = 4    /* per Gaussian: the extra levels' activated features, lsr_forward_levels only */
};

/* Returns device memory of at least `bytes` bytes, 256-byte aligned, valid until the caller
 * releases it; NULL on failure.  Called synchronously from the calling thread. */
typedef void* (*lsr_alloc_fn)(void* user, int32_t which, size_t bytes);

/* Fused parameter activation.  Each bit set in lsr_forward_args.raw /
 * lsr_backward_args.raw says the matching input is GaussianModel's RAW parameter; the kernels
 * apply the model's activation (scene/gaussian_model.py:33-41 setup_functions, getters :134-161;
 * language normalisation gaussian_renderer/__init__.py:87) and the backward returns the gradient
 * w.r.t. the raw tensor.  raw == 0 is the reference's API: every input already activated. */
enum lsr_raw_flags {
    LSR_RAW_OPACITY = 1,    /* opacities = _opacity:            sigmoid(x) = 1 / (1 + exp(-x))      */
    LSR_RAW_SCALES = 2,     /* scales = _scaling:               exp(x)                              */
    LSR_RAW_ROTATIONS = 4,  /* rotations = _rotation:           x / max(||x||, 1e-12) (F.normalize) */
    LSR_RAW_LANGUAGE = 8    /* language_feature = _language_feature: x / (||x|| + 1e-9)             */
};

/* The language step's backward (no geometry gradient, no colour gradient) accumulates 20-byte
 * per-Gaussian gradient records that must start at zero.  With LSR_FWD_ZERO_GRAD_RECORDS the
 * forward clears them inside its compositing kernel (stores beside a VALU-bound loop: no separate
 * memset launch) in the geometry buffer; the FIRST backward of that forward then passes
 * LSR_BWD_RECORDS_ZEROED and uses them as they are.  Any other backward clears its own records.
 * LSR_BWD_RECORDS_ZEROED is only valid for the first backward of a forward that passed
 * LSR_FWD_ZERO_GRAD_RECORDS, and lsr_backward_args.dL_dloss only for a forward that fused the loss
 * (out_loss set): the forward records both in its image buffer, and with settings.debug the
 * backward checks them and fails with LSR_ERR_INVALID instead of reading stale records or codes. */
/* LSR_FWD_NO_COLOR_GRAD: the caller promises that the backward of this forward gets no colour
 * gradient (lsr_backward_args.dL_dout_color == NULL), as in LangSplat's language step
 * (train.py:96-104: the loss reads the language image only).  The compositing kernel then stores
 * only the transmittance and feature sums of its split-replay states (half the state traffic).  A
 * backward with dL_dout_color after such a forward would start long tiles' replay chunks from
 * missing colour sums: it is invalid, and with settings.debug it fails with LSR_ERR_INVALID. */
/* LSR_FWD_NO_BACKWARD (ABI 13): the caller promises that no lsr_backward follows this forward
 * (inference: render.py:24-55 renders under torch.no_grad()).  The compositing kernel then writes
 * only the images (and the fused loss, if asked): not the state only the backward reads -- the
 * per-instance cover masks, the split-replay states, the backward's work lists, and the image
 * buffer's final transmittance and contributor counts.  With settings.debug a backward of such a
 * forward fails with LSR_ERR_INVALID. */
enum lsr_forward_flags { LSR_FWD_ZERO_GRAD_RECORDS = 1, LSR_FWD_NO_COLOR_GRAD = 2, LSR_FWD_NO_BACKWARD = 4 };
/* LSR_BWD_SHARED_CU (ABI 14): another stream's kernels run beside this backward (the pipelined step,
 * langsplat_amd/pipeline.py: the next view's preprocess, sort and binning).  The render backward
 * then runs at most 6 workgroups per CU instead of 8 (extra dynamic LDS), leaving wave slots and LDS
 * to the other stream's workgroups: measured at C3, 0.417-0.421 -> 0.400-0.401 ms per pipelined step
 * (DESIGN.md §5b).  Results are unchanged. */
/* LSR_BWD_DEFER_TAIL (ABI 16): the fused update (lsr_backward_args.update) split around a gradient
 * all-reduce (train.py:104 + 134-137 with the views of N ranks: langsplat_amd.pipeline at N > 1).
 * lsr_backward then runs the render backward only and leaves the language step's gradient records
 * in the geometry buffer (lsr_state_layout.grad_records) in planar form: float[3P] language partials
 * (dL/d of the activated feature, before the activation's chain rule), one word holding
 * *update_skip (0 when NULL), three padding words, then float[2P] screen-space partials.  The caller
 * reduces the first 3 P + 1 floats over the ranks -- an AVG: the chain rule and the Adam step are
 * linear / pointwise in the partials, a Gaussian another rank saw has partials here too, and the
 * skip word (0 or the bits of 1.0f) stays non-zero on every rank once one rank's view overflowed --
 * then calls lsr_language_tail with the same arguments: ONE pass writes dL_dmeans2D (this view's,
 * from the unreduced screen-space partials), dL_dlanguage_feature (from the reduced partials) and
 * the Adam step on the reduced skip word (+ the fill): what lsr_backward with update does at N = 1,
 * with no gradient epilogue before the collective.  The records need no LSR_BWD_RECORDS_ZEROED (they
 * are cleared here otherwise). */
enum lsr_backward_flags { LSR_BWD_RECORDS_ZEROED = 1, LSR_BWD_SHARED_CU = 2, LSR_BWD_DEFER_TAIL = 4 };

/* GaussianRasterizationSettings (gaussian_renderer/__init__.py:37-51), device-pointer form. */
typedef struct lsr_settings {
    int32_t image_height;
    int32_t image_width;
    float tanfovx;
    float tanfovy;
    float scale_modifier;
    int32_t sh_degree;        /* active SH degree D (0..3) */
    int32_t prefiltered;
    int32_t debug;            /* sync + check after every kernel */
    int32_t include_feature;  /* composite the 3-channel language feature */
    int32_t reserved;
    const float* bg;          /* [3] */
    const float* viewmatrix;  /* [16] world_view_transform */
    const float* projmatrix;  /* [16] full_proj_transform */
    const float* campos;      /* [3] camera_center */
} lsr_settings;

/* Inputs/outputs of _C.rasterize_gaussians.  Exactly one of {shs, colors_precomp} and one of
 * {scales+rotations, cov3D_precomp} is non-NULL (GaussianRasterizer.forward validates). */
typedef struct lsr_forward_args {
    int32_t P;                       /* number of Gaussians */
    int32_t M;                       /* SH coefficients stored per Gaussian (shs: P x M x 3) */
    const float* means3D;            /* P x 3 */
    const float* shs;                /* P x M x 3 or NULL */
    const float* colors_precomp;     /* P x 3 or NULL */
    const float* language_feature;   /* P x 3, or NULL when include_feature == 0 */
    const float* opacities;          /* P */
    const float* scales;             /* P x 3 or NULL */
    const float* rotations;          /* P x 4 (already normalised) or NULL */
    const float* cov3D_precomp;      /* P x 6 or NULL */
    float* out_color;                /* 3 x H x W */
    float* out_language_feature;     /* 3 x H x W */
    int32_t* radii;                  /* P */
    int32_t raw;                     /* lsr_raw_flags; 0 = activated inputs (reference API) */
    int32_t flags;                   /* lsr_forward_flags */
    const float* shs_rest;           /* NULL, or P x (M-1) x 3 (_features_rest) with shs = P x 1 x 3
                                        (_features_dc): the SH rows without torch.cat
                                        (scene/gaussian_model.py:146-150) */
    uint8_t* visible;                /* NULL, or P bytes: radii > 0 (render()'s visibility_filter,
                                        gaussian_renderer/__init__.py:99), written by preprocess */
    /* Fused language-feature loss (train.py:96-99):
     *     *out_loss = l1_loss(language_feature_image * mask, loss_target * mask)
     *               = sum |f m - gt m| / (3 H W)          (utils/loss_utils.py:17-18)
     * computed by the compositing kernel from the pixels it just produced (deterministic order).
     * out_loss NULL: off.  Needs include_feature and language_feature. */
    const float* loss_target;        /* 3 x H x W, or NULL */
    const uint8_t* loss_mask;        /* H x W bool bytes (scene/cameras.py:72 seg != -1), or NULL */
    float* out_loss;                 /* one float (device), or NULL */
    /* Capacity mode (graph capture): capacity_rendered > 0 bounds the tile instances and
     * capacity_entries (> 0) the super-tile entries of this view; the buffers and launch grids are
     * sized from them, the device reads the true counts, and the call enqueues its work without
     * waiting for the device.  *num_rendered then returns capacity_rendered (the value lsr_backward
     * needs).  A view that exceeds either capacity is not rasterized (background image, zero
     * gradients) and sets *overflow (device int32, written by every capacity-mode forward: 0, or
     * when set 0x3F800000 -- the bits of 1.0f, ABI 14 -- so the flag tests non-zero as an int and
     * can be all-reduced as a float beside the gradients: with a SUM or an average over ranks it is
     * non-zero on every rank as soon as one rank's view overflowed); the caller re-runs it with
     * larger capacities.  capacity_rendered == 0: the host reads the
     * counts after the preprocess (one wait) and sizes exactly. */
    int64_t capacity_rendered;
    int64_t capacity_entries;
    int32_t* overflow;               /* device int32 or NULL */
    int64_t* out_num_entries;        /* HOST pointer or NULL: the super-tile entry count (not in
                                        capacity mode), the capacity_entries a later call needs */
    /* Deferred language feature (the gradient all-reduce overlap).  NULL: off.
     * Otherwise a hipEvent_t: the preprocess, depth order and binning run without reading
     * language_feature, and the stream waits for this event only before a small kernel copies
     * (raw: activates) language_feature into the per-Gaussian records and the compositing starts.
     * A trainer records the event after the previous step's all-reduce and optimiser update of the
     * language feature on another stream, so that update overlaps this view's geometry work
     * (langsplat_amd.distributed.UpdateOverlap, langsplat_amd.pipeline).  Results are identical to a
     * call without it.  In capacity mode (a graph capture) the event is one recorded in the same
     * capture (a join of two branches). */
    void* language_ready;
    /* Forward in two calls (capacity mode only; the ABI 11 pipelined graph step): LSR_PHASE_GEOMETRY
     * enqueues the preprocess (language feature deferred), depth order and binning and returns;
     * LSR_PHASE_COMPOSITE, with the same arguments and an allocator that returns the same buffers,
     * enqueues the rest: the language feature into the records and the compositing (+ fused loss).
     * Whatever the caller orders between the two calls on the stream (e.g. a wait for the feature's
     * update) runs between them, so the two halves can be captured into two HIP graphs replayed on
     * different streams.  The compositing of a composite phase runs at fewer workgroups per CU (6,
     * leaving wave slots and registers to the other stream), which
     * changes no result.  LSR_PHASE_ALL (0): one call does everything. */
    int32_t phase;
} lsr_forward_args;
/* LSR_PHASE_COMPOSITE_FILLED (ABI 12): as LSR_PHASE_COMPOSITE, but the records' language slots already
 * hold the activated feature -- written by a fused update's fill_record (lsr_backward_args), which
 * may run before or while the geometry call runs: the geometry call of a split forward never writes
 * those slots. */
enum lsr_forward_phase { LSR_PHASE_ALL = 0, LSR_PHASE_GEOMETRY = 1, LSR_PHASE_COMPOSITE = 2, LSR_PHASE_COMPOSITE_FILLED = 3 };

/* Inputs/outputs of _C.rasterize_gaussians_backward.  Every non-NULL output is fully written
 * (zeros for culled Gaussians).  dL_dsh may be NULL when shs is NULL; dL_dscales/dL_drotations
 * may be NULL when cov3D_precomp is given; dL_dcov3D may be NULL when scales are given.
 * Geometry gradients are all-or-nothing: when dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D,
 * dL_dsh, dL_dsh_rest, dL_dscales and dL_drotations are ALL NULL (no geometry input needs a
 * gradient: ctx.needs_input_grad, e.g. LangSplat's language step, scene/gaussian_model.py:203-217),
 * only dL_dmeans2D and dL_dlanguage_feature (either may be NULL too) are computed and the
 * preprocess backward is not run. */
typedef struct lsr_backward_args {
    int32_t P;
    int32_t M;
    int64_t num_rendered;            /* value returned by lsr_forward */
    const float* means3D;
    const float* shs;
    const float* colors_precomp;
    const float* language_feature;
    const float* opacities;
    const float* scales;
    const float* rotations;
    const float* cov3D_precomp;
    const int32_t* radii;
    const float* dL_dout_color;             /* 3 x H x W or NULL (treated as zeros) */
    const float* dL_dout_language_feature;  /* 3 x H x W or NULL (treated as zeros) */
    void* geom_buffer;
    void* binning_buffer;
    void* image_buffer;
    float* dL_dmeans2D;              /* P x 3 (z = 0) */
    float* dL_dcolors;               /* P x 3 */
    float* dL_dlanguage_feature;     /* P x 3 */
    float* dL_dopacity;              /* P */
    float* dL_dmeans3D;              /* P x 3 */
    float* dL_dcov3D;                /* P x 6 or NULL */
    float* dL_dsh;                   /* P x M x 3 or NULL */
    float* dL_dscales;               /* P x 3 or NULL */
    float* dL_drotations;            /* P x 4 or NULL */
    int32_t raw;                     /* as in the forward; gradients are then w.r.t. the raw inputs */
    int32_t flags;                   /* lsr_backward_flags */
    const float* shs_rest;           /* as in the forward */
    float* dL_dsh_rest;              /* P x (M-1) x 3 when shs_rest is set (dL_dsh is then P x 1 x 3) */
    const float* dL_dloss;           /* NULL, or the device scalar dL/d(out_loss) of a forward that fused
                                        the loss: its gradient dL/dloss * sign(f m - gt m) * m / (3 H W)
                                        (autograd's) is added to dL_dout_language_feature (NULL = 0) */
    /* ABI 12: LangSplat's language step with its optimiser step fused into the backward's epilogue
     * (train.py:104 + 134-137 at N = 1, where nothing happens between the two: langsplat_amd.graph /
     * langsplat_amd.pipeline use it in their captured steps).  update != NULL needs the language-only
     * backward (every geometry output NULL, dL_dout_color NULL), raw & LSR_RAW_LANGUAGE and
     * update->param == language_feature.  Then, after the render backward, ONE pass per Gaussian reads
     * its gradient record, writes dL_dmeans2D and dL_dlanguage_feature as always, and applies the
     * Adam step of lsr_adam_multi (device form: update_step_dev is that call's step block, tensor 0;
     * update_skip its skip flag) to param / exp_avg / exp_avg_sq -- the same operations, so the same
     * values as lsr_backward followed by lsr_adam_multi.  fill_record (NULL: off) is the record array
     * (lsr_state_layout.record) of another forward's geometry buffer over the same P Gaussians: every
     * Gaussian's language slots there receive the activated updated feature (skipped or not), so that
     * forward's composite call (LSR_PHASE_COMPOSITE_FILLED) needs no fill of its own. */
    const struct lsr_adam_tensor* update;  /* (defined with lsr_adam_multi below) */
    int64_t* update_step_dev;
    const int32_t* update_skip;
    float* fill_record;
} lsr_backward_args;

/* Byte offsets of the internal state inside the forward buffers, for inspection by tests and
 * for debug dumps.  All arrays are tightly packed at the given offsets. */
typedef struct lsr_state_layout {
    /* geometry buffer */
    size_t depth_key;      /* uint32[P]  float bits of view depth, 0xFFFFFFFF if culled */
    size_t tiles_touched;  /* uint32[P] */
    size_t rect;           /* uint32[2P] (minx | miny << 16, maxx | maxy << 16) */
    size_t record;         /* float4[3P] {x, y, conic.x, conic.y}{conic.z, opacity, r, g}{b, f0, f1, f2} */
    size_t clamped;        /* uint32[P]  bit c = SH colour channel c clamped */
    size_t sorted_ids;     /* uint32[P]  Gaussians by (depth, id); culled ones tie with the farthest */
    size_t super_offset;   /* uint32[P]  first super-tile entry of the Gaussian of depth rank r */
    /* image buffer */
    size_t counters;       /* uint32[16] {reserved, num_rendered, error, forward flags, super entries, ...} */
    size_t ranges;         /* uint32[2T] [start, end) of each tile in point_list */
    size_t final_T;        /* float[H*W] */
    size_t n_contrib;      /* uint32[H*W] */
    /* binning buffer */
    size_t point_list;     /* uint32[num_rendered] Gaussian ids, tile-major, (depth, id) order;
                              entry k belongs to the tile t with ranges[t].x <= k < ranges[t].y */
    /* geometry buffer (ABI 16) */
    size_t grad_records;   /* float[5P] the language step's gradient records; after a backward with
                              LSR_BWD_DEFER_TAIL: float[3P] language partials, the skip word, 3 words,
                              then float[2P] dx, dy */
} lsr_state_layout;

int32_t lsr_abi_version(void);
const char* lsr_last_error(void);

/* Sizes (bytes) of the forward scratch buffers, exactly what lsr_forward requests for the geometry
 * and image buffers (the geometry buffer holds one fused-loss word per tile, so it depends on the
 * image size too); binning: an upper bound for any scene with num_rendered tile instances (the
 * forward requests the size its super-tile entry count needs, at most this). */
size_t lsr_geom_bytes(int32_t P, int32_t width, int32_t height);
size_t lsr_image_bytes(int32_t width, int32_t height);
size_t lsr_binning_bytes(int32_t width, int32_t height, int64_t num_rendered);
size_t lsr_backward_bytes(int32_t P);
int32_t lsr_state_layout_of(int32_t P, int32_t width, int32_t height, int64_t num_rendered,
                            lsr_state_layout* out);

/* _C.rasterize_gaussians: preprocess, depth sort, tile binning (super-tile lists + per-tile
 * ranks), front-to-back compositing.  Writes out_color, out_language_feature, radii and *num_rendered. */
int32_t lsr_forward(const lsr_settings* settings, const lsr_forward_args* args,
                    lsr_alloc_fn alloc, void* alloc_user, void* stream, int64_t* num_rendered);

/* _C.rasterize_gaussians_backward: back-to-front replay and per-Gaussian chain rule. */
int32_t lsr_backward(const lsr_settings* settings, const lsr_backward_args* args,
                     lsr_alloc_fn alloc, void* alloc_user, void* stream);

/* Per-stage device time, measured with HIP events recorded on the caller's stream around each
 * launch group while profiling is enabled (measurement support for bench.py; no reference
 * counterpart).  lsr_profile_enable(1) clears and starts, (0) stops; lsr_profile_report
 * synchronises the recorded events and returns the number of stages written to `out`. */
typedef struct lsr_kernel_stat {
    char name[32];
    int64_t launches;
    double total_ms;
} lsr_kernel_stat;

int32_t lsr_profile_enable(int32_t on);
int32_t lsr_profile_report(lsr_kernel_stat* out, int32_t capacity);
/* Restricts profiling to the comma-separated stage names (NULL or "" = every stage), so a timed
 * run can time its dominant kernel live without event overhead around the other stages. */
int32_t lsr_profile_select(const char* stages);
/* Records the events on every `every`-th launch of a selected stage only (default 1; reset by each
 * call): a timed run samples its dominant kernel's duration at a fraction of the events' cost. */
int32_t lsr_profile_sample(int32_t every);

/* _C.mark_visible: visible[i] = 1 iff Gaussian i passes the near-plane frustum test. */
int32_t lsr_mark_visible(int32_t P, const float* means3D, const float* viewmatrix,
                         const float* projmatrix, uint8_t* visible, void* stream);

/* The language slots of a forward's render records, from the parameter (ABI 14): for every Gaussian
 * with radii[i] > 0, record[i]'s three feature words receive language_feature[i] (activated as
 * the forward activates it when raw has LSR_RAW_LANGUAGE: normalised).  `record` is
 * lsr_state_layout.record of the geometry buffer of a forward made with phase LSR_PHASE_GEOMETRY
 * over the same P Gaussians, and radii that forward's radii.  What LSR_PHASE_COMPOSITE does before
 * compositing; a caller that changed the parameter after a fused update already filled the records
 * (lsr_backward_args.fill_record) refills them with this before a LSR_PHASE_COMPOSITE_FILLED call
 * (langsplat_amd/pipeline.py follow_caller). */
int32_t lsr_fill_language(int32_t P, const float* language_feature, int32_t raw, const int32_t* radii, float* record,
                          void* stream);

/* Measurement hook, not part of the reference interface: with LSR_RENDER_STATS=1 in the
 * environment the render backward counts, per wave-iteration over a culled list entry, [0]
 * entries, [1] entries passing the power test in some lane, [2] entries some lane blends, [3]
 * lanes blending, [8 + c] a histogram of lanes blending (c = 0..64).  Copies min(n, 73) counters
 * to host memory and clears them (synchronous). */
int32_t lsr_debug_render_stats(uint64_t* out, int32_t n);

/* Measurement hook, not part of the reference interface: with LSR_RENDER_STATS=1 the render
 * kernels (kernel 0 = forward, 1 = backward) record per workgroup b < n into out[11 b .. 11 b + 10]:
 * {start, end} (100 MHz wall clock, low 32 bits), the tile (-1: a workgroup that only filled empty
 * tiles), the hardware slot (XCC_ID << 16 | CU/SH/SE bits of HW_ID), and (forward) the ticks spent
 * loading, compacting and walking its batches, the batch count | the first batch's load ticks << 16,
 * and six milestones of the first batch in ticks after the start, two 16-bit fields per word
 * (begin, tile range loaded, first barrier, point-list ids loaded, records gathered, load phase
 * done; synchronous). */
int32_t lsr_debug_render_timeline(int32_t kernel, uint32_t* out, int32_t n);

/* Look-back stalls, not part of the reference interface.  The single-pass scans of the forward
 * (depth order, binning), of lsr_dist_cuda2 and the block-sum hand-off of lsr_masked_l1_forward wait
 * for values published by other workgroups.  A wait is bounded: after `limit` polls (default
 * 1 << 24) the waiting workgroup computes the value itself from the inputs -- the results are the
 * same, only slower -- and flags the event.  lsr_debug_scan_stalls returns 1 if a launch made by
 * the calling thread on the current device took that path since the last call (read it after the
 * work finished, e.g. after a stream synchronise), and clears the flag; negative on error.
 * lsr_debug_set_spin_limit sets the poll bound for launches made after it and returns the old one;
 * 0 makes every wait take the fallback at once (fault injection for tests). */
int32_t lsr_debug_scan_stalls(void);
uint32_t lsr_debug_set_spin_limit(uint32_t limit);

/* Measurement hook, not part of the reference interface: with LSR_BUCKET_TIMELINE=1 the MSD depth
 * sort's bucket kernel records per workgroup b < min(n, 256) into out[8 b .. 8 b + 7]: {start, end}
 * (100 MHz wall clock, low 32 bits), the hardware slot (XCC_ID << 16 | CU/SH/SE bits of HW_ID),
 * the bucket's key count, the end times of the first pass, of all passes and of the output gathers,
 * and the time the bucket's keys had arrived (synchronous). */
int32_t lsr_debug_bucket_timeline(uint32_t* out, int32_t n);
/* Measurement aid (ABI 14): a one-wave kernel on `stream` reads the shader-clock counter (s_memtime)
 * and the constant 100 MHz counter (s_memrealtime) before and after a ~20 us spin and stores the four
 * values into out_device[0..3] (a device array of 4 u64): the engine clock the chip ran at meanwhile
 * is 100 (out[3] - out[1]) / (out[2] - out[0]) MHz (tools/clock_probe.py). */
int32_t lsr_debug_clock_probe(uint64_t* out_device, void* stream);
/* (ABI 18 removed ABI 15's delay kernel with the phase-delay experiment it served,
 * profiles/r06_phase_delays.txt.) */
/* Host runtime helper (ABI 17): `stream` waits for each of the n_waits events, then the
 * instantiated graph `graph_exec` (a hipGraphExec_t) is launched on it and, if record_event is not
 * null, that event recorded after it -- the stream-A half of a pipelined step's replay in one call
 * (langsplat_amd/pipeline.py PipelinedGraphStep.replay), replacing torch's stream context, event
 * waits and CUDAGraph.replay() in Python (~8 us of host time before every synced step's launch,
 * profiles/r06_sync_gap.txt).  No reference counterpart: the reference has no captured step. */
int32_t lsr_graph_launch(void* graph_exec, void* stream, void* const* wait_events, int32_t n_waits,
                         void* record_event);

/* ---- the language-feature loss around the rasterizer ----------------
 *
 * lsr_masked_l1_forward replaces, in LangSplat's include_feature step (train.py:97-98),
 *     Ll1 = l1_loss(language_feature * mask, gt_language_feature * mask)
 * with l1_loss = torch.abs(a - b).mean() (utils/loss_utils.py:17-18): one pass over
 * pred / gt (C x HW fp32) and mask (HW, bool bytes or fp32, broadcast over the C channels).
 * *loss (one float, device) = sum |pred*m - gt*m| / (C*HW), summed in a fixed order
 * (deterministic).  `scratch` holds lsr_masked_l1_scratch_bytes(C, HW) bytes, zeroed once
 * before its first use and then reused (one stream at a time per scratch).
 *
 * lsr_masked_l1_backward writes the gradient torch autograd produces for that expression:
 *     grad_pred = sign(pred*m - gt*m) * (grad_loss[0] / (C*HW)) * m
 * (grad_loss is the device scalar dL/dLl1), bit-identical to autograd's mean/abs/sub/mul chain.
 *
 * lsr_decode_language_feature restates Camera.get_language_feature (scene/cameras.py:58-92) on
 * the GPU: seg = seg_map[level] (L x H x W int64), mask = (seg != -1), feature = feature_map[seg]
 * (N x D fp32; index -1 reads the last row, as torch indexing does) written as D x H x W, and
 * mask as H x W bytes -- so a training loop can decode each view's map once and keep it in HBM
 * instead of np.load + CPU gather + H2D every step.  A segment id outside [-N, N) (the reference's
 * feature_map[seg] raises IndexError) returns LSR_ERR_INVALID; the call waits for its kernel to
 * find that out (once per view). */
/* ---- optimiser step --------------------------------------------------
 * One Adam step of torch.optim.Adam (amsgrad=False, weight_decay=0), the optimiser of
 * scene/gaussian_model.py:229 stepped at train.py:134-137, over one fp32 parameter tensor of n
 * elements: exp_avg / exp_avg_sq updated in place, then param.  `step` is the 1-based step count
 * after this update (torch's state["step"]); lr may change between calls (learning-rate
 * schedules, scene/gaussian_model.py:231-241). */
int32_t lsr_adam_step(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, double lr,
                      double beta1, double beta2, double eps, int64_t step, void* stream);

/* The same step for several tensors in ONE launch (RGB mode's six parameter groups,
 * scene/gaussian_model.py:219-226, each with its own lr, betas, eps and step count, i.e. torch's
 * per-parameter state).  Every gradient is multiplied by grad_scale first (e.g. the 1 / N of a
 * gradient all-reduced as a SUM over N ranks; 1 = none).
 * step_dev (device int64[LSR_ADAM_STEP_WORDS], ABI 12) replaces the tensors' step fields AND learning
 * rates for a step replayed from a HIP graph (at most 16 tensors then):
 *   step_dev[0]                      the step count;
 *   step_dev[1 .. 48]                scratch: a one-wave kernel first advances the count by one and
 *                                    writes that step's bias-corrected scalars of every tensor here,
 *                                    which the update reads;
 *   step_dev[LSR_ADAM_WORD_SKIPPED]  the number of steps skipped through `skip` (below);
 *   step_dev[LSR_ADAM_WORD_LR + k]   tensor k's learning rate (a double's bits), which the caller keeps
 *                                    current (a learning-rate schedule, scene/gaussian_model.py:231-241,
 *                                    changes it between replays without a re-capture); the table's lr
 *                                    is not read;
 *   a tensor's `step` field is then its OFFSET from the count (ABI 14): tensor k's step of a replay
 *   is step_dev[0] + 1 + tensors[k].step (0 when all counts are equal; torch's per-parameter counts
 *   differ after replace_tensor_to_optimizer, scene/gaussian_model.py:326-339, since the replaced
 *   group skips that iteration's step).  The offset must be > -2^40 and < 2^40.
 * step_dev NULL: the host's step counts and lrs.
 * skip (device int32, or NULL): when *skip != 0 at run time the launch changes nothing -- no
 * parameter, moment or step count -- and, with step_dev, adds one to the skipped count.  A captured
 * train step passes its rasterizer's capacity overflow flag (lsr_forward_args.overflow), so a view
 * that was not rasterized is a no-op for the optimiser, exactly as if it had been left out. */
#define LSR_ADAM_STEP_WORDS 66   /* count, 16 x 3 scalar words, skipped count, 16 lrs */
#define LSR_ADAM_WORD_SKIPPED 49
#define LSR_ADAM_WORD_LR 50
typedef struct lsr_adam_tensor {
    int64_t n;
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    double lr, beta1, beta2, eps;
    int64_t step;                /* 1-based, after this update */
} lsr_adam_tensor;
int32_t lsr_adam_multi(int32_t count, const lsr_adam_tensor* tensors, float grad_scale, int64_t* step_dev,
                       const int32_t* skip, void* stream);

/* The language step's update at N > 1 (ABI 15): lsr_adam_multi of ONE tensor -- the raw language
 * feature, P x 3 (tensor->n = 3 P), its gradient the all-reduced one (times grad_scale) -- in the
 * device form (step_dev and its learning-rate word 0 as lsr_adam_multi's; skip as there), which
 * also writes the updated feature (activated when raw has LSR_RAW_LANGUAGE) into the language
 * slots of fill_record, another forward's render records (lsr_state_layout.record; the same slots
 * lsr_backward_args.fill_record receives at N = 1), so that forward's composite phase runs as
 * LSR_PHASE_COMPOSITE_FILLED.  A skipped step still fills (with the unchanged feature).  Replaces
 * lsr_adam_multi + the fill of LSR_PHASE_COMPOSITE when the gradient all-reduce sits between the
 * backward and the update (langsplat_amd.pipeline.PipelinedGraphStep with a bucket). */
int32_t lsr_adam_fill_language(const lsr_adam_tensor* tensor, float grad_scale, int64_t* step_dev, const int32_t* skip,
                               void* fill_record, int32_t raw, void* stream);

/* The second half of a backward made with LSR_BWD_DEFER_TAIL (ABI 16): settings and args as passed
 * to that lsr_backward (same buffers, update, update_step_dev, update_skip, fill_record; flags may
 * keep LSR_BWD_DEFER_TAIL), after the caller reduced the records' language partials.  Launches the
 * Adam step advance and one pass per Gaussian: dL_dmeans2D, dL_dlanguage_feature, the Adam step and
 * the fill, as lsr_backward with update (not deferred) does after its render backward. */
int32_t lsr_language_tail(const lsr_settings* settings, const lsr_backward_args* args, void* stream);

/* Densification statistics of one rendered view, one pass (train.py:125-126 with
 * GaussianModel.add_densification_stats, scene/gaussian_model.py:480-482), for Gaussians with
 * radii > 0:  max_radii2D = max(max_radii2D, radii);  xyz_gradient_accum += ||dL_dmeans2D[:, :2]||;
 * denom += 1.  dL_dmeans2D is P x 3 (viewspace_points.grad); the three outputs are P floats each
 * (the reference's (P,) and (P, 1) tensors); any of them may be NULL (not updated). */
int32_t lsr_densification_stats(int32_t P, const int32_t* radii, const float* dL_dmeans2D, float* max_radii2D,
                                float* xyz_gradient_accum, float* denom, void* stream);

/* ---- point-cloud initialisation --------------------------------------
 * simple-knn's distCUDA2 (scene/gaussian_model.py:20,180): for each of the N points (N x 3 fp32),
 * the mean of the squared distances to its 3 nearest OTHER points (exact; a duplicate of a point
 * counts at distance 0; with N < 4 the missing neighbours count as FLT_MAX).  Scratch is requested
 * once through `alloc` (which = LSR_BUF_BACKWARD).
 * Non-finite coordinates (inf, NaN) are the brute force's, unchanged: a point with one is nobody's
 * neighbour (its squared distance to anything is inf or NaN, which is never smaller than a kept one)
 * and its own output is (FLT_MAX + FLT_MAX + FLT_MAX) / 3 = inf; every other point's output is what
 * the cloud without those points gives.  They are left out of the bounding box; no error is raised
 * and the call does not wait for the device. */
int32_t lsr_dist_cuda2(int64_t N, const float* points, float* out_mean_dist, lsr_alloc_fn alloc, void* alloc_user,
                       void* stream);

/* Test hook, not part of the reference interface; host only, no device work.  The search grid
 * lsr_dist_cuda2 would size for N points (1 .. 0x3FFFFFFF) with the bounding box
 * box = {min x, y, z, max x, y, z}: out_origin_h = {x0, y0, z0, h, 1 / h}, out_dims = {nx, ny, nz}, by
 * the function the device runs (langsplat_amd/csrc/lsr_knn.hip knn_grid_size).  For every bit
 * pattern of box: 1 <= nx, ny, nz, nx * ny * nz <= 2 N + 64, h and 1 / h positive, finite and normal.
 * An axis with min > max (no finite coordinate) has origin 0 and zero extent; a non-finite box value,
 * or a cell size whose h or 1 / h is no normal float, gives one cell (1 x 1 x 1, h = 1).
 * Added without a change of LSR_ABI_VERSION (purely additive): callers detect it by symbol. */
int32_t lsr_debug_knn_grid(const float* box, int64_t N, float* out_origin_h, int32_t* out_dims);

/* ---- open-vocabulary query ------------------------------------------
 * What eval/evaluate_iou_loc.py:258-266 does with a rendered language map, for N pixels in ONE
 * kernel: Autoencoder.decode (autoencoder/model.py:42-46: the decoder's Linears with a ReLU between
 * them, then x / ||x||, no epsilon), the cosine similarities with n_pos + n_neg unit-norm phrase
 * embeddings, and OpenCLIPNetwork.get_relevancy (eval/openclip_encoder.py:42-56) for every positive:
 *     out_relevancy[j, pixel] = min over negatives n of 1 / (1 + exp(10 (s_n - s_j)))
 * -- get_max_across's (n_phrases, h*w) result of one level.  The decoded D-vectors stay on chip
 * (out_decoded, for tests and small N, writes them out).  All arithmetic is fp32 (the matrix
 * products on the exact-fp32 MFMA); no atomics; two calls give bit-identical results.
 * Supported: input width 3; 1 to 8 layers; every width a multiple of 16, at most 512; n_pos >= 1,
 * n_neg >= 1, n_pos + n_neg <= 64; weights and phrases 16-byte aligned.  Anything else returns
 * LSR_ERR_INVALID before any device work.  The call enqueues one kernel on `stream` and does not wait.
 * N == 0 is valid and enqueues nothing; the pointers (feature, weights, phrases, out_relevancy) must
 * still be non-NULL.
 * Added without a change of LSR_ABI_VERSION (purely additive): callers detect it by symbol. */
typedef struct lsr_query_args {
    int64_t N;                    /* pixels */
    const float* feature;         /* the rendered map: channel c of pixel i at feature[c * channel_stride + i * pixel_stride] */
    int64_t channel_stride, pixel_stride;  /* floats: (HW, 1) = the rasterizer's 3xHxW, (1, 3) = renders_npy's HxWx3 */
    int32_t n_layers;
    const int32_t* widths;        /* HOST int32[n_layers], widths[n_layers-1] = D */
    const float* weights;         /* device: per layer, W (out x in, row-major, nn.Linear's) then b (out), tightly packed */
    int32_t n_pos, n_neg;
    const float* phrases;         /* device: (n_pos + n_neg) x D, positives first */
    float* out_relevancy;         /* device: n_pos x N */
    float* out_decoded;           /* NULL, or device N x D: the normalised decoded vectors (tests, small N) */
} lsr_query_args;
int32_t lsr_query_relevancy(const lsr_query_args* args, void* stream);

/* lsr_query_semantic: OpenCLIPNetwork.get_semantic_map (eval/openclip_encoder.py:82-94) on the same
 * decoded pixels, in ONE kernel: an open-vocabulary segmentation.  The decoder, the normalisation and
 * the cosine similarities s_k with the n_labels + n_neg phrases (labels first) are lsr_query_relevancy's,
 * bit for bit.  Per pixel:
 *     out_label = argmax_k softmax(10 s)_k, and -1 where a negative wins (k >= n_labels).  Softmax is
 *                 monotone, so this is the FIRST index of the largest s_k (torch.argmax's tie rule: a
 *                 scan from k = 0 with a strict >; a label beats a negative of equal similarity);
 *     out_score = the winner's softmax value, 1 / sum_k exp(10 (s_k - s_max)), summed in index order
 *                 (for a -1 pixel: the winning negative's probability).  NULL: not computed.
 * A pixel whose decoded norm is 0 has every s_k NaN: label 0 (as torch.argmax gives) and a NaN score.
 * Limits, refusals (LSR_ERR_INVALID before any device work; out_label must be non-NULL), N == 0 and
 * the call's behaviour (one kernel, no wait, no atomics, bit-identical between calls) are
 * lsr_query_relevancy's.
 * Added without a change of LSR_ABI_VERSION (purely additive): callers detect it by symbol. */
typedef struct lsr_query_semantic_args {
    int64_t N;                    /* pixels */
    const float* feature;         /* as lsr_query_args */
    int64_t channel_stride, pixel_stride;
    int32_t n_layers;
    const int32_t* widths;        /* HOST int32[n_layers] */
    const float* weights;         /* device, as lsr_query_args */
    int32_t n_labels, n_neg;
    const float* phrases;         /* device: (n_labels + n_neg) x D, labels first */
    int32_t* out_label;           /* device: N labels, 0 .. n_labels - 1 or -1 */
    float* out_score;             /* NULL, or device: N floats */
} lsr_query_semantic_args;
int32_t lsr_query_semantic(const lsr_query_semantic_args* args, void* stream);

/* lsr_label_stats: what one does with label maps -- per-class counts of n_maps predicted maps against
 * ground truth, N pixels each.  gt has gt_maps = 1 map (shared by every predicted map) or n_maps.
 * A pixel is valid exactly when 0 <= gt < n_classes (any other value is an ignore label: the pixel
 * counts nowhere).  A valid pixel of class g adds one to ground_truth[g] and to valid; if
 * 0 <= pred < n_classes, one to predicted[pred]; if pred == g, one to intersection[g] and to correct.
 * A prediction of -1 (or any value outside the classes) on a valid pixel is a miss and counts in no
 * predicted cell.  The union of a class is predicted + ground_truth - intersection.
 * The call clears its outputs on the stream itself, enqueues one kernel (per 65535 maps) and does not
 * wait.  Integer atomics only: the counts are exact and identical between calls.  LSR_ERR_INVALID
 * before any device work for null args or pointers, n_classes outside 1..64, gt_maps neither 1 nor
 * n_maps, N < 0 or above 2^40, n_maps < 0, outputs not 8-byte aligned.  n_maps == 0 or N == 0 is valid
 * and enqueues nothing (the outputs are not touched).
 * Added without a change of LSR_ABI_VERSION (purely additive): callers detect it by symbol. */
typedef struct lsr_label_stats_args {
    int64_t N;                    /* pixels per map */
    int32_t n_maps, gt_maps, n_classes;
    const int32_t* pred;          /* device: n_maps x N */
    const int32_t* gt;            /* device: gt_maps x N */
    int64_t* out_counts;          /* device: n_maps x n_classes x 3 (intersection, predicted, ground truth) */
    int64_t* out_totals;          /* device: n_maps x 2 (correct, valid) */
} lsr_label_stats_args;
int32_t lsr_label_stats(const lsr_label_stats_args* args, void* stream);

/* ---- LERF evaluation -----------------------------------------------------
 * What activate_stream and lerf_localization (eval/evaluate_iou_loc.py:90-217) do with
 * get_max_across's (levels, n_prompts, H, W) relevancy after their first line, for n_maps = levels *
 * n_prompts maps of H x W floats (row-major, tightly packed), in two calls on one stream.
 *
 * lsr_eval_filter (:107-112, :176-187): per map
 *     avg   = cv2.filter2D(map, -1, ones((30, 30)) / 900) with cv2's defaults: a correlation, the
 *             anchor at ksize / 2 = 15, so the taps are offsets -15 .. +14 in both axes; border
 *             BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba, the edge sample not repeated), reflected
 *             with period 2 (n - 1) as often as needed, so any H, W >= 2 works.  Separable: 30 taps
 *             along x, then 30 along y, each as three chains of 10 consecutive taps added in a fixed
 *             order, the sum divided by 900 once (no sliding window);
 *     blend = 0.5f * (avg + map);
 *     stats = min(blend), max(blend), max(avg) and the FIRST row-major index at which avg has that
 *             maximum (np.argmax / the first row of np.nonzero(avg == max)).
 * out_avg and out_blend may each be NULL (not written); stats are always written.  While the call's
 * kernels run, a record holds order-preserving integer keys (integer atomic min / max, the arg-max as
 * a 64-bit max over key << 32 | ~index); the call's last kernel turns them into the fields below.
 * stats must be 8-byte aligned.  Maps are expected to be free of NaNs; -0 orders below +0.
 *
 * lsr_eval_masks (:129-143, eval/utils.py:46-55), after lsr_eval_filter on the same stream: per map
 *     raw mask: o = x - mn; o = o / ((mx - mn) + 1e-9f); o = o * 2.0f + (-1.0f); o = clamp(o, 0, 1);
 *               m = o > thresh   (mn, mx = the map's stats.blend_min / blend_max; the division is
 *               the correctly rounded one; a constant map divides by 1e-9f and gives an empty mask);
 *     smoothed mask: smooth() with its quirks: pixel (i, j) looks at rows max(0, i-3) ..
 *               min(i+4, H-1) - 1 and the same range of columns -- the upper bound is exclusive and
 *               clipped to H-1, not H, so the last row and the last column are never inside a window
 *               -- and becomes 1 exactly when 2 * ones > window size (a tie gives 0);
 *     with gt_mask (n_prompts x H x W bytes, non-zero = set; map m uses prompt m % n_prompts, the
 *               (levels, n_prompts, H, W) layout): out_counts[2 m] = |gt AND smoothed|,
 *               out_counts[2 m + 1] = |gt OR smoothed| (integer atomic adds).
 * out_mask_raw may be NULL.  Without gt_mask, n_prompts and out_counts are not read.
 *
 * All arithmetic is fp32 without contraction; no float atomics; two calls, on any streams, give
 * bit-identical results.  Both calls return LSR_ERR_INVALID before any device work for null args or
 * a null required pointer, H < 2, W < 2, H * W >= 2^31, n_maps < 0, and (with gt_mask) n_prompts < 1
 * or n_maps % n_prompts != 0.  n_maps == 0 is valid and enqueues nothing.  Neither call waits for
 * the device.
 * Added without a change of LSR_ABI_VERSION (purely additive): callers detect them by symbol. */
typedef struct lsr_eval_stats {
    float blend_min, blend_max;   /* of blend */
    float avg_max;                /* of avg */
    int32_t avg_argmax;           /* first row-major index (y * W + x) with avg == avg_max */
} lsr_eval_stats;
typedef struct lsr_eval_filter_args {
    int32_t n_maps, H, W;
    const float* maps;            /* device: n_maps x H x W */
    float* out_avg;               /* NULL, or device n_maps x H x W */
    float* out_blend;             /* NULL, or device n_maps x H x W */
    lsr_eval_stats* out_stats;    /* device: n_maps records */
} lsr_eval_filter_args;
int32_t lsr_eval_filter(const lsr_eval_filter_args* args, void* stream);
typedef struct lsr_eval_mask_args {
    int32_t n_maps, H, W;
    const float* blend;           /* device: n_maps x H x W (lsr_eval_filter's out_blend) */
    const lsr_eval_stats* stats;  /* device: n_maps records (lsr_eval_filter's out_stats) */
    float thresh;
    int32_t n_prompts;            /* with gt_mask: the number of ground-truth masks */
    const uint8_t* gt_mask;       /* NULL, or device n_prompts x H x W */
    uint8_t* out_mask;            /* device: n_maps x H x W, the smoothed masks (0 / 1) */
    uint8_t* out_mask_raw;        /* NULL, or device n_maps x H x W, the masks before smoothing */
    int64_t* out_counts;          /* with gt_mask: device n_maps x 2 (intersection, union) */
} lsr_eval_mask_args;
int32_t lsr_eval_masks(const lsr_eval_mask_args* args, void* stream);

/* ---- the RGB stage's loss (train.py:100-103 with include_feature=False) ------------------------
 *     Ll1  = l1_loss(image, gt_image)                                    utils/loss_utils.py:17-18
 *     loss = (1 - lambda_dssim) * Ll1 + lambda_dssim * (1 - ssim(image, gt_image))      :23-63
 * for `planes` = B * C independent image planes of H x W floats (row-major, tightly packed).
 * ssim is the reference's with size_average=True: per plane the window g g^T, g the 11-tap Gaussian
 * with sigma 1.5 (normalised in fp64, then rounded to fp32), zero padding of 5 and no renormalisation at the
 * borders, C1 = 0.01^2, C2 = 0.03^2, the mean of the map over all planes and pixels.  The window is
 * applied separably (rows, then columns): the same sums in another rounding order.
 *
 * lsr_rgb_loss_forward writes out_terms = {loss, l1, ssim}.  With out_maps it also writes, for the
 * backward, three H x W maps per plane (map m of plane p at out_maps[(m * planes + p) * H * W]): the
 * partial derivatives of the pixel's SSIM value S by its windowed means mu1 = E[x], E[x^2] and E[xy],
 * the latter two taken as variables of their own.  out_maps NULL: no gradient is wanted and nothing
 * is written.  out_ssim_map (optional) receives S per pixel.  `scratch` holds
 * lsr_rgb_loss_scratch_bytes(planes, H, W) bytes, 8-byte aligned; it needs no initialisation and one
 * scratch serves any sequence of calls on one stream.  The two sums are reduced in a fixed order
 * (per-workgroup partials in double, then one block): two calls give bit-identical terms.
 *
 * lsr_rgb_loss_backward writes
 *     dL/dimage = dL_dloss * [ (1 - lambda) / N * sign(x - y)
 *                              - lambda / N * (conv(Ma) + 2 x conv(Mb) + y conv(Mc)) ]
 * with N = planes * H * W, sign(0) = 0 (torch's abs backward), conv the same zero-padded window (it
 * is symmetric, so it is its own adjoint) and Ma, Mb, Mc the forward's maps; dL_dloss is a device
 * scalar.  There is no gradient for the target.
 *
 * Both return LSR_ERR_INVALID before any device work for null args, a null required pointer,
 * planes / H / W < 1, more than 2^31 - 1 tiles, or a scratch that is not 8-byte aligned.  Neither
 * waits for the device; no float atomics.  LSR_RGB_LOSS_TILE_H x LSR_RGB_LOSS_TILE_W is the tile of
 * one workgroup (tests place their sizes around it).
 * Added without a change of LSR_ABI_VERSION (purely additive): callers detect them by symbol. */
#define LSR_RGB_LOSS_TILE_H 32
#define LSR_RGB_LOSS_TILE_W 32
typedef struct lsr_rgb_loss_args {
    int32_t planes, H, W;
    float lambda_dssim;
    const float* image;           /* device: planes x H x W */
    const float* target;          /* device: planes x H x W */
    float* out_terms;             /* device: 3 floats {loss, l1, ssim} */
    float* out_maps;              /* NULL, or device 3 x planes x H x W */
    float* out_ssim_map;          /* NULL, or device planes x H x W */
    void* scratch;                /* device: lsr_rgb_loss_scratch_bytes(planes, H, W) bytes */
} lsr_rgb_loss_args;
typedef struct lsr_rgb_loss_bwd_args {
    int32_t planes, H, W;
    float lambda_dssim;
    const float* image;           /* device: planes x H x W */
    const float* target;          /* device: planes x H x W */
    const float* maps;            /* device: 3 x planes x H x W (the forward's out_maps) */
    const float* dL_dloss;        /* device scalar */
    float* out_dL_dimage;         /* device: planes x H x W */
} lsr_rgb_loss_bwd_args;
size_t lsr_rgb_loss_scratch_bytes(int32_t planes, int32_t H, int32_t W);
int32_t lsr_rgb_loss_forward(const lsr_rgb_loss_args* args, void* stream);
int32_t lsr_rgb_loss_backward(const lsr_rgb_loss_bwd_args* args, void* stream);

/* ---- all language levels of a scene in one rasterizer pass (inference) ---------------------------
 * LangSplat trains its semantic levels from ONE RGB checkpoint with the geometry frozen
 * (scene/gaussian_model.py:203-217 with include_feature; train.py:222 writes <model>_1/_2/_3), so
 * the level models share means, SH, opacity, scales and rotations bit for bit and differ only in
 * their P x 3 language feature -- and evaluation wants the levels together
 * (eval/evaluate_iou_loc.py:258-266 stacks the rendered maps).  lsr_forward_levels renders up to
 * LSR_MAX_LEVELS of them with one geometry pass and one compositing walk that carries 3 * levels
 * language channels.
 *
 * Contract.  The call is inference only (no backward state is written; lsr_backward must not follow).
 * The preprocess, depth order, binning, colour image, radii, `visible` and *num_rendered are those of
 * lsr_forward with the same `fwd`.  Level 0 is fwd.language_feature -> fwd.out_language_feature;
 * level l >= 1 is more_language_feature[(l - 1) P 3 ...] -> more_out_language_feature[(l - 1) 3 H W ...].
 * Level l's map is bit-identical to the out_language_feature of an lsr_forward whose language_feature
 * is level l's tensor: each channel is its own fma(f, w, acc) chain in list order, with the blend
 * weight w = alpha T shared by all channels.  There is no background term: empty tiles, P == 0 and
 * fully culled scenes give zeros in every level.  levels == 1 behaves exactly as lsr_forward.
 * fwd.raw & LSR_RAW_LANGUAGE applies to every level (all raw or all activated).
 *
 * The extra levels' activated features of the visible Gaussians are staged in one scratch array,
 * requested as LSR_BUF_LEVELS (P > 0 and levels > 1 only): ceil(3 (levels - 1) / 4) float4 per
 * Gaussian, {l1.0 l1.1 l1.2 l2.0}{l2.1 l2.2 l3.0 l3.1}{l3.2 - - -}, so a list entry's gather is whole
 * 16-byte loads.  lsr_levels_bytes is exactly that request: the array's size rounded up to 256 bytes
 * (0 for levels == 1 or P <= 0).
 *
 * Refused with LSR_ERR_INVALID before any device work, the message naming the field: levels outside
 * 1..LSR_MAX_LEVELS; reserved != 0; settings.include_feature == 0; fwd.flags != LSR_FWD_NO_BACKWARD;
 * loss_target, loss_mask or out_loss set; language_ready set; phase != LSR_PHASE_ALL;
 * capacity_rendered != 0 (no graph capture of this form); with P > 0 a NULL fwd.language_feature;
 * with levels > 1 a NULL more_out_language_feature or (P > 0) more_language_feature.
 * Added without a change of LSR_ABI_VERSION (purely additive): callers detect it by symbol. */
#define LSR_MAX_LEVELS 4            /* feature_level 0..3, scene/cameras.py:75-88 */
typedef struct lsr_forward_levels_args {
    lsr_forward_args fwd;                  /* as lsr_forward; language_feature / out_language_feature are level 0 */
    int32_t levels;                        /* 1 .. LSR_MAX_LEVELS */
    int32_t reserved;                      /* 0 */
    const float* more_language_feature;    /* (levels-1) x P x 3; raw iff fwd.raw & LSR_RAW_LANGUAGE; NULL iff levels == 1 */
    float* more_out_language_feature;      /* (levels-1) x 3 x H x W */
} lsr_forward_levels_args;
size_t lsr_levels_bytes(int32_t P, int32_t levels);
int32_t lsr_forward_levels(const lsr_settings* settings, const lsr_forward_levels_args* args, lsr_alloc_fn alloc,
                           void* alloc_user, void* stream, int64_t* num_rendered);
/* Measurement hook, not part of the reference interface: the workgroups per CU the HIP runtime grants
 * the inference compositing kernel of `levels` levels (1: lsr_forward's) on the current device, from
 * its registers and LDS with the hardware's allocation granules; negative (-lsr_status) on error. */
int32_t lsr_debug_levels_occupancy(int32_t levels);

/* ---- the language gradient of all levels in one pass (the backward of lsr_forward_levels) ---------
 * With the geometry frozen the levels' only gradient is the one of their language features, and for
 * the activated features a it is
 *     dL/da[l][k][c] = sum over pixels of w_k(pixel) * g[l][c](pixel),     w_k = alpha_k T_k,
 * with w the forward's own blend weight and g = dL/d(level l's map).  T_k is the forward's running
 * product, so lsr_backward_levels accumulates the sums front to back by running the forward's walk a
 * second time; it reads only what the inference forward leaves in its three buffers (the records,
 * the tile ranges, the point list and the longest-first tile lists).  lsr_backward still must NOT
 * follow lsr_forward_levels (no backward state was written): this call is the only backward of that
 * forward.  The buffers must be those of a lsr_forward_levels call with the same settings, P and
 * geometry (levels == 1: lsr_forward_levels with levels == 1, i.e. lsr_forward under
 * LSR_FWD_NO_BACKWARD), unchanged since, and num_rendered the value it returned.
 *
 * The seed g is dL_dout_language_feature, the fused masked-L1 seed, or their sum when both are given.
 * The fused seed is the gradient of  sum_l dL_dloss[l] * l1_loss(map_l * mask_l, target_l * mask_l):
 *     g[l][c] = dL_dloss[l] * sign(f m - gt m) * m / (3 H W)
 * (lsr_backward_args.dL_dloss's expression), formed per pixel from out_language_feature (the forward's
 * maps), loss_target and loss_mask, so no levels x 3 x H x W gradient image is materialised.  Its
 * four pointers are all set or all NULL.
 *
 * Every entry of dL_dlanguage_feature is written: the gradient w.r.t. language_feature when raw has
 * LSR_RAW_LANGUAGE (the normalisation's chain rule per level; language_feature is read only then),
 * else w.r.t. the activated features; exact zeros for culled Gaussians (radii <= 0).  With P == 0
 * nothing is written; with num_rendered == 0 or all-zero seeds the output is zeros.  `scratch` is
 * lsr_backward_levels_bytes(P, levels) bytes (P rows of 3 levels floats, rounded up to 256 bytes; 0 for
 * P <= 0 or levels outside 1..LSR_MAX_LEVELS), cleared by the call itself.  The call enqueues its work on `stream` and never
 * waits for the device.  The sums are float atomic adds: the last bits depend on arrival order.
 *
 * Refused with LSR_ERR_INVALID before any device work, the message naming the field: a NULL settings
 * or args; levels outside 1..LSR_MAX_LEVELS; reserved != 0; P < 0; num_rendered < 0;
 * settings.include_feature == 0; with P > 0 a NULL geom_buffer, binning_buffer, image_buffer, radii,
 * scratch or dL_dlanguage_feature; raw & LSR_RAW_LANGUAGE with a NULL language_feature (P > 0); a
 * partial set of out_language_feature, loss_target, loss_mask and dL_dloss; neither seed given.
 * Added without a change of LSR_ABI_VERSION (purely additive): callers detect it by symbol. */
typedef struct lsr_backward_levels_args {
    int32_t P;
    int32_t levels;                         /* 1 .. LSR_MAX_LEVELS */
    int32_t raw;                            /* lsr_raw_flags; only LSR_RAW_LANGUAGE is read */
    int32_t reserved;                       /* 0 */
    int64_t num_rendered;                   /* value returned by lsr_forward_levels */
    void* geom_buffer;                      /* the forward's three buffers */
    void* binning_buffer;
    void* image_buffer;
    const int32_t* radii;                   /* P, the forward's */
    const float* language_feature;          /* levels x P x 3, level-major; read iff raw & LSR_RAW_LANGUAGE */
    const float* dL_dout_language_feature;  /* levels x 3 x H x W, or NULL */
    const float* out_language_feature;      /* fused seed: the forward's maps, levels x 3 x H x W, or NULL */
    const float* loss_target;               /* fused seed: levels x 3 x H x W, or NULL */
    const uint8_t* loss_mask;               /* fused seed: levels x H x W bool bytes, or NULL */
    const float* dL_dloss;                  /* fused seed: levels device floats, or NULL */
    void* scratch;                          /* lsr_backward_levels_bytes(P, levels) bytes */
    float* dL_dlanguage_feature;            /* levels x P x 3 */
} lsr_backward_levels_args;
size_t lsr_backward_levels_bytes(int32_t P, int32_t levels);
int32_t lsr_backward_levels(const lsr_settings* settings, const lsr_backward_levels_args* args, void* stream);

/* ---- the joint levels step without a host wait (for a HIP graph capture) --------------------------
 * lsr_levels_step_forward is lsr_forward_levels in capacity mode, optionally split in phases;
 * lsr_levels_step_backward is lsr_backward_levels on that forward's buffers, optionally with the Adam
 * step of the (levels, P, 3) raw features and the next forward's feature fills fused into its
 * per-Gaussian tail (langsplat_amd.levels_graph.GraphedLevelsStep).  lsr_forward_levels and
 * lsr_backward_levels keep their contracts; neither call here ever waits for the device.
 *
 * lsr_levels_step_forward.  fwd.capacity_rendered > 0, fwd.capacity_entries > 0 and fwd.overflow are
 * required; *num_rendered returns fwd.capacity_rendered (as lsr_forward in capacity mode).  A view over
 * a capacity sets *fwd.overflow to 0x3F800000 (else 0) and is not binned: every tile range stays empty
 * and no tile is scheduled, so the call leaves zeros in every level's map and the background colour in
 * out_color (radii and `visible` are still the preprocess's).  A view that draws nothing (true count 0)
 * leaves the same images with *fwd.overflow == 0.  fwd.phase:
 *     LSR_PHASE_ALL               geometry, the feature fills, the compositing;
 *     LSR_PHASE_COMPOSITE         the geometry is already in the buffer set -- from a plain
 *                                 lsr_forward(phase = LSR_PHASE_GEOMETRY) with the same settings, P,
 *                                 capacities, flags and allocator (the geometry does not depend on the
 *                                 levels), or from lsr_view_restore of a pack saved from such a call --
 *                                 and this call writes the visible Gaussians' level-0 slots of the
 *                                 records and their LSR_BUF_LEVELS rows from the features, then composites;
 *     LSR_PHASE_COMPOSITE_FILLED  records and LSR_BUF_LEVELS hold the activated features already
 *                                 (lsr_levels_step_backward's fill_record / fill_levels): compositing only.
 * In the two composite phases fwd.radii is an input (what the geometry call or the restore left there)
 * and fwd.visible is not written: both belong to the phase that runs the preprocess.
 * LSR_PHASE_GEOMETRY is refused (use lsr_forward).  levels == 1 is lsr_forward's own capacity path.
 * P == 0 is served as by lsr_forward_levels (zero images, nothing else; *fwd.overflow is not written).
 * Refused with LSR_ERR_INVALID before any device work, the message naming the field: what
 * lsr_forward_levels refuses (levels, reserved, include_feature, fwd.flags != LSR_FWD_NO_BACKWARD,
 * loss_target / loss_mask / out_loss, language_ready, NULL features or outputs), fwd.capacity_rendered
 * or fwd.capacity_entries <= 0, a NULL fwd.overflow, and fwd.phase == LSR_PHASE_GEOMETRY or unknown.
 * Added without a change of LSR_ABI_VERSION (purely additive): callers detect it by symbol. */
typedef struct lsr_levels_step_forward_args {
    lsr_forward_levels_args levels;        /* as lsr_forward_levels, with the differences above */
    int32_t reserved;                      /* 0 */
} lsr_levels_step_forward_args;
int32_t lsr_levels_step_forward(const lsr_settings* settings, const lsr_levels_step_forward_args* args,
                                lsr_alloc_fn alloc, void* alloc_user, void* stream, int64_t* num_rendered);

/* lsr_levels_step_backward.  The fields shared with lsr_backward_levels_args mean what they mean there;
 * the buffers are those of a lsr_levels_step_forward call (any phase) and num_rendered is the value it
 * returned, i.e. its capacity (> 0 when P > 0).  The call cannot know whether anything was drawn: a
 * view whose true count is 0 and a view over capacity both leave empty tile ranges and no scheduled
 * tile, the gradient walk then adds nothing and the gradient is exact zeros.  The walk is
 * lsr_backward_levels' kernel.  The tail, one pass per Gaussian and level:
 *     update == NULL   dL_dlanguage_feature as lsr_backward_levels writes it (it is then required;
 *                      update_step_dev, update_skip, fill_record and fill_levels must be NULL);
 *     update != NULL   needs raw & LSR_RAW_LANGUAGE, update->param == language_feature, update->n ==
 *                      3 levels P, the moments and update_step_dev (lsr_adam_multi's device block: word 0
 *                      the count, LSR_ADAM_WORD_LR the learning rate; update->step is the offset;
 *                      update->grad and update->lr are not read).  A one-wave launch advances the step
 *                      block; then per value: the raw gradient (exact zeros where radii <= 0), written
 *                      to dL_dlanguage_feature when that is not NULL, and the Adam step of the feature
 *                      and its moments -- the operations of the update == NULL tail followed by
 *                      lsr_adam_multi(step_dev), bit for bit.  *update_skip != 0 (update_skip may be
 *                      NULL: never): no feature, moment or count changes, the skipped count grows by 1.
 *                      fill_record (another call's, or this set's, render records,
 *                      lsr_state_layout.record) receives level 0's activated updated feature in the
 *                      language slots of EVERY Gaussian, and fill_levels (a LSR_BUF_LEVELS array,
 *                      lsr_levels_bytes(P, levels)) the other levels' in lsr_forward_levels' layout,
 *                      zero padded -- skipped or not, visible or not (lsr_backward_args.fill_record's
 *                      rule) -- so the next lsr_levels_step_forward runs LSR_PHASE_COMPOSITE_FILLED.
 * P == 0: a no-op that returns LSR_OK after the argument checks (nothing is enqueued, the step block
 * does not advance).
 * Refused with LSR_ERR_INVALID before any device work, the message naming the field: what
 * lsr_backward_levels refuses (dL_dlanguage_feature may be NULL with update); num_rendered == 0 with
 * P > 0; update without raw & LSR_RAW_LANGUAGE; update->param != language_feature; update->n != 3 levels
 * P; NULL update->exp_avg / exp_avg_sq or update_step_dev; fill_levels NULL with levels > 1 and
 * fill_record set, or fill_levels set without fill_record; update_step_dev, update_skip, fill_record or
 * fill_levels without update.
 * Added without a change of LSR_ABI_VERSION (purely additive): callers detect it by symbol. */
typedef struct lsr_levels_step_backward_args {
    int32_t P;
    int32_t levels;                         /* 1 .. LSR_MAX_LEVELS */
    int32_t raw;                            /* lsr_raw_flags; only LSR_RAW_LANGUAGE is read */
    int32_t reserved;                       /* 0 */
    int64_t num_rendered;                   /* value returned by lsr_levels_step_forward (its capacity) */
    void* geom_buffer;                      /* the forward's three buffers */
    void* binning_buffer;
    void* image_buffer;
    const int32_t* radii;                   /* P, the forward's */
    const float* language_feature;          /* levels x P x 3, level-major; read iff raw & LSR_RAW_LANGUAGE */
    const float* dL_dout_language_feature;  /* levels x 3 x H x W, or NULL */
    const float* out_language_feature;      /* fused seed: the forward's maps, levels x 3 x H x W, or NULL */
    const float* loss_target;               /* fused seed: levels x 3 x H x W, or NULL */
    const uint8_t* loss_mask;               /* fused seed: levels x H x W bool bytes, or NULL */
    const float* dL_dloss;                  /* fused seed: levels device floats, or NULL */
    void* scratch;                          /* lsr_backward_levels_bytes(P, levels) bytes */
    float* dL_dlanguage_feature;            /* levels x P x 3; may be NULL with update */
    const lsr_adam_tensor* update;          /* the fused Adam step of language_feature, or NULL */
    int64_t* update_step_dev;               /* device int64[LSR_ADAM_STEP_WORDS] */
    const int32_t* update_skip;             /* device int32 (the forward's overflow flag), or NULL */
    float* fill_record;                     /* render records receiving level 0, or NULL */
    void* fill_levels;                      /* LSR_BUF_LEVELS array receiving levels 1.., or NULL */
    int64_t reserved2;                      /* 0 */
} lsr_levels_step_backward_args;
int32_t lsr_levels_step_backward(const lsr_settings* settings, const lsr_levels_step_backward_args* args,
                                 void* stream);

/* ---- a view's frozen geometry, kept across steps of the language stage ---------------------------
 * In the language stage every geometry parameter is frozen (scene/gaussian_model.py:203-217), and
 * train.py:85-87 draws each of a scene's views again every epoch: for one camera, what a
 * LSR_PHASE_GEOMETRY forward (preprocess, depth order, binning) leaves behind is the same at every
 * visit.  lsr_view_save gathers the part of it that later phases read into a compact pack;
 * lsr_view_restore puts a pack back into a buffer set of the same P, image size and capacities, in
 * place of the geometry call (langsplat_amd/pipeline.py PipelinedGraphStep's view cache).
 *
 * The pack (lsr_view_pack_bytes; every segment 16-byte aligned, sizes rounded up to 16 bytes, in
 * this order; T = the number of 16 x 16 tiles):
 *     320 B    the counter slots and the forward's 64 class counts of the longest-first schedule
 *     32 P     record[3 i], record[3 i + 1] of every Gaussian (lsr_state_layout.record)
 *     4 P      word 0 (b) of record[3 i + 2]
 *     4 P      radii
 *     4 P      clamped
 *     8 T      ranges
 *     4 T      the forward's scheduled tiles, class by class
 *     4 R      the num_rendered point-list entries
 * i.e. what LSR_PHASE_COMPOSITE[_FILLED], lsr_backward (with or without geometry gradients) and
 * lsr_language_tail read of the geometry phase's products (lsr_view_pack_bytes: a pack may end here),
 * and then, in a pack of at least lsr_view_plan_pack_bytes, the view's WALK PLAN: what a compositing
 * of that geometry derives from the geometry alone (the same bits at every visit while the geometry
 * is frozen) and is worth keeping,
 *     R        the instances' cover masks
 * The plan is valid if a render forward that writes a backward's state (not LSR_FWD_NO_BACKWARD) ran
 * on the set between its geometry call and lsr_view_save -- counter word 8 says so: the render forward
 * sets it, the geometry phase clears it, and lsr_view_save keeps it with the pack.  A pack saved
 * before any compositing has the segments (the size does not depend on it) but no plan, and a pack
 * of fewer than lsr_view_plan_pack_bytes has neither: both bind as the plain bound form.
 * lsr_view_restore ignores the plan.  Sort and scan scratch, depth keys and super-tile tables are not
 * kept, nor what else the compositing writes (split states, the backward's work lists, final_T,
 * n_contrib, loss codes: it writes them at every step), nor the records' language slots.
 * lsr_view_plan_layout gives the plan segment's offset.
 *
 * lsr_view_save reads a buffer set that a capacity-mode LSR_PHASE_GEOMETRY forward filled (the
 * compositing and backward of that view may have run on it since: nothing after the render forward
 * rewrites the cover masks -- the backward only reads them) whose view fitted its capacities;
 * num_rendered is that view's count (counter slot 1, read back by the caller).  lsr_view_restore
 * brings a set into the state that geometry call would leave, for everything a later phase reads;
 * it also re-initialises what the geometry phase clears on every run and a later phase relies on:
 * the fused loss's words, the forward flags (from `flags` and `fused_loss`, as the geometry call
 * publishes them), the overflow word and *overflow (0), and the backward's class counts (0).  It
 * never writes the records' language slots: a fused update's fill_record may fill them before,
 * while or after the restore runs, exactly as with the geometry call.
 *
 * One kernel launch per call on `stream`; neither call waits for the device.  LSR_ERR_INVALID before
 * any device work for null args or a null geom / image / binning / radii / pack, P, width, height or
 * a capacity < 1, num_rendered < 0 or > capacity_rendered, pack_bytes < lsr_view_pack_bytes(...), a
 * buffer or pack that is not 16-byte aligned, or an unknown flag.
 * Added without a change of LSR_ABI_VERSION (purely additive): callers detect them by symbol. */
typedef struct lsr_view_args {
    int32_t P, width, height;
    int32_t flags;                /* restore: the lsr_forward_flags of the forward this set serves */
    int32_t fused_loss;           /* restore: that forward fuses the loss (out_loss with the feature) */
    int32_t reserved;             /* 0 */
    int64_t capacity_rendered;    /* the set's capacities (lsr_forward_args) */
    int64_t capacity_entries;
    int64_t num_rendered;         /* the view's tile instances */
    void* geom;                   /* the set's LSR_BUF_GEOM, LSR_BUF_IMAGE and LSR_BUF_BINNING buffers */
    void* image;
    void* binning;
    int32_t* radii;               /* P: the forward's radii output */
    void* pack;                   /* device, pack_bytes bytes */
    size_t pack_bytes;
    int32_t* overflow;            /* restore: NULL, or the forward's overflow flag (set to 0) */
} lsr_view_args;
size_t lsr_view_pack_bytes(int32_t P, int32_t width, int32_t height, int64_t num_rendered);
/* Bytes of a pack that also holds the view's walk plan (see above); 0 for what lsr_view_pack_bytes
 * answers with 0. */
size_t lsr_view_plan_pack_bytes(int32_t P, int32_t width, int32_t height, int64_t num_rendered);
/* Byte offsets of the walk plan: its segment in a pack of num_rendered instances (pack_cover;
 * pack_bytes = lsr_view_plan_pack_bytes) and the array it is saved from in a buffer set of
 * capacity_rendered (set_cover, in the binning buffer; the flag word word_plan_ready of the counters at
 * set_counters in the image buffer).  TEST SUPPORT, not an interface to build on: the set_* fields are a
 * set's internal layout and may change with any library build; no caller needs them to use the plan
 * (lsr_view_plan_pack_bytes, lsr_view_save and lsr_view_bind are the interface).  For tests that compare
 * a hit with a miss it also says where the set
 * keeps the rest of what a compositing leaves for the backward, none of it part of the plan:
 * set_final_T, set_n_contrib, set_split_desc, set_bwd_lists and set_loss_code (the fused loss's
 * per-pixel code bytes) in the image buffer.  The backward's lists: class c (0 .. classes - 1) holds
 * counters[word_bwd_class + c] items at set_bwd_lists + 4 c split_items tiles.
 * Host only (no device work).  Both added without a change of
 * LSR_ABI_VERSION (the smaller pack and every earlier call behave as before): a library that has
 * these symbols keeps and binds walk plans. */
typedef struct lsr_view_plan_offsets {
    size_t pack_counters, pack_cover, pack_bytes;
    size_t set_counters, set_cover, set_final_T, set_n_contrib, set_split_desc, set_bwd_lists, set_loss_code;
    size_t tiles, classes, split_items, word_plan_ready, word_bwd_class;
} lsr_view_plan_offsets;
int32_t lsr_view_plan_layout(int32_t P, int32_t width, int32_t height, int64_t capacity_rendered, int64_t num_rendered,
                             lsr_view_plan_offsets* out);
/* The eight counter slots a capacity-mode geometry call left in `image` (the set's LSR_BUF_IMAGE
 * buffer of a width x height forward; slot 1 = num_rendered, slot 7 = the overflow word) into
 * host_counters: 8 x uint32 of pinned host memory the device can write, by one one-wave kernel on
 * `stream` -- no copy engine, no wait; the values are there once an event recorded after the call
 * has completed.  How a caller learns the num_rendered lsr_view_save needs without reading the
 * device.  LSR_ERR_INVALID for a null pointer or a size < 1. */
int32_t lsr_view_counts(int32_t width, int32_t height, const void* image, uint32_t* host_counters, void* stream);
int32_t lsr_view_save(const lsr_view_args* args, void* stream);
int32_t lsr_view_restore(const lsr_view_args* args, void* stream);

/* ---- the bound form: a cached view's geometry read in place ---------------------------------------
 * lsr_view_restore copies a pack (78 MB at 1M Gaussians and 1080p) into the set at every revisit.
 * The bound form leaves the large arrays where they are.  Every buffer set carries, at the end of its
 * geometry buffer (lsr_view_bind_layout; lsr_geom_bytes includes both),
 *   - a table of 48 bytes: { const float4* rec01; const float4* recb; const uint32_t* point_list;
 *     uint32_t s01, sb; const uint8_t* cover; uint32_t plan, pad; } -- Gaussian i's two leading record
 *     words at rec01[s01 i], rec01[s01 i + 1], its third word {b, f0, f1, f2} at recb[sb i]; the walk
 *     plan's cover masks when plan != 0 (the set is bound to a pack with a plan), else null (the
 *     kernels use the set's own array);
 *   - a plane of P float4 {b, f0, f1, f2}: the home of the language slots in this form.
 * A render forward made with LSR_BIND_FORWARD in lsr_forward_args.flags and a lsr_backward made with
 * LSR_BIND_BACKWARD in lsr_backward_args.flags read the table once per workgroup and gather the
 * records and the point list through it, so a captured composite + backward bakes the table's
 * address, not the view's: one capture serves every view.  Without the flags both behave as before.
 *
 * Who writes the table and the plane:
 *   - lsr_forward, LSR_PHASE_GEOMETRY with LSR_BIND_FORWARD (a view without a pack): the preprocess
 *     writes the identity table (the set's own records at stride 3, its point list, the plane at
 *     stride 1) and stores b into plane[i].x as well as into the records (lsr_view_save still reads a
 *     set the geometry phase filled).  LSR_BIND_FORWARD is refused with LSR_PHASE_ALL and by the
 *     levels entry points.
 *   - lsr_view_bind with a pack, in place of lsr_view_restore: the table names the pack's rec01
 *     segment (stride 2), the set's plane and the pack's point list; the pack's b words go into
 *     plane[i].x; the counters (with lsr_view_restore's re-initialisation rules), ranges, the class
 *     lists and radii are copied into the set, clamped only with LSR_BIND_CLAMPED (the backward with
 *     geometry gradients reads it, the language step does not); the fused loss's words, the forward
 *     flags, the overflow word and *overflow and the backward's class counts are re-initialised as
 *     lsr_view_restore does.  About 30 MB of traffic at 1M Gaussians and 1080p instead of 157 MB.
 *     The pack is only read: several sets may be bound to one pack at once, and the caller keeps it
 *     alive until the last composite / backward of every set bound to it has finished.
 *     If the pack holds a walk plan (decided on the device, from the pack's counter word 8, so one
 *     captured composite + backward serves packs with and without): the table names the pack's cover
 *     masks.  The render forward then reads each instance's mask from the pack instead of computing
 *     it, and stores none; the backward reads the masks through the table.  Every output is what a
 *     miss produces (the gradients up to the order of their float atomics).  The masks are those of
 *     the geometry alone, so a plan serves any later composite / backward of that view, with or
 *     without split replay.
 *   - lsr_view_bind with args->pack == NULL (num_rendered and pack_bytes ignored): the identity
 *     table, and b from the set's records into plane[i].x, for a set whose geometry phase ran
 *     without LSR_BIND_FORWARD.
 *   - the language slots plane[i].yzw: LSR_PHASE_COMPOSITE's fill (with LSR_BIND_FORWARD),
 *     lsr_fill_language_plane, lsr_adam_fill_language_plane, and a fused update whose
 *     lsr_backward_args.flags carry LSR_BIND_FILL_PLANE (fill_record is then the plane's address,
 *     Gaussian i's slots at 16 i + 4, in lsr_backward and in lsr_language_tail alike).  Neither the
 *     geometry phase nor lsr_view_bind ever writes them.
 * One launch per lsr_view_bind call on `stream`, no wait.  LSR_ERR_INVALID (message in
 * lsr_last_error) before any device work for what lsr_view_restore refuses, an unknown bind flag, or
 * a null geometry buffer (where the table lives).  Added without a change of LSR_ABI_VERSION:
 * callers detect these entry points by symbol.  The flag values sit above lsr_forward_flags' and
 * lsr_backward_flags' own. */
enum lsr_bind_flags {
    LSR_BIND_FORWARD = 16,     /* lsr_forward_args.flags */
    LSR_BIND_BACKWARD = 16,    /* lsr_backward_args.flags */
    LSR_BIND_FILL_PLANE = 32,  /* lsr_backward_args.flags: fill_record is the plane */
    LSR_BIND_CLAMPED = 1       /* lsr_view_bind's bind_flags */
};
int32_t lsr_view_bind_layout(int32_t P, int32_t width, int32_t height, size_t* plane_offset, size_t* table_offset);
int32_t lsr_view_bind(const lsr_view_args* args, int32_t bind_flags, void* stream);
int32_t lsr_fill_language_plane(int32_t P, const float* language_feature, int32_t raw, const int32_t* radii, float* plane,
                                void* stream);
int32_t lsr_adam_fill_language_plane(const lsr_adam_tensor* tensor, float grad_scale, int64_t* step_dev,
                                     const int32_t* skip, void* fill_plane, int32_t raw, void* stream);

size_t lsr_masked_l1_scratch_bytes(int32_t C, int64_t HW);
int32_t lsr_masked_l1_forward(int32_t C, int64_t HW, const float* pred, const float* gt, const void* mask,
                              int32_t mask_is_float, float* loss, void* scratch, void* stream);
int32_t lsr_masked_l1_backward(int32_t C, int64_t HW, const float* pred, const float* gt, const void* mask,
                               int32_t mask_is_float, const float* grad_loss, float* grad_pred, void* stream);
int32_t lsr_decode_language_feature(int32_t L, int32_t H, int32_t W, const int64_t* seg_map, int32_t level,
                                    int32_t N, int32_t D, const float* feature_map, float* out_feature,
                                    uint8_t* out_mask, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSR_H */
