/*
 * lentil_hip.h -- C-ABI of liblentil_hip.so: the MI355X (gfx950) implementation of
 * lentil's bidirectional bokeh redistribution + polynomial-optics ray transfer.
 *
 * This is the drop-in boundary.  A `Camera` object of the
 * reference plugin (src/lentil.h:92-196) keeps owning all render state; instead of
 * accumulating into std::vector buffers from `filter_pixel` it owns one
 * `lentil_hip_ctx` and drives it with the calls below.  Every entry point names the
 * reference code it replaces.  Plain pointers and sizes only: no torch, no HIP and no
 * Arnold types appear in any signature.
 *
 * Conventions
 *   - All functions return LENTIL_OK (0) or a negative LENTIL_ERR_* code; the text of
 *     the last error is available from lentil_hip_last_error().  Nothing aborts or
 *     exits (the reference's failures on this path are per-draw rejects, and
 *     AiRenderAbort on setup errors, src/lentil.h:225-228).
 *   - A context is bound to one GPU and one HIP stream.  Calls on one context must be
 *     serialised by the caller (the reference takes l_critsec only around
 *     setup_camera, src/lentil.h:212,235); different contexts are independent
 *     (multi-GPU = one context per device, one process per GPU).
 *   - "visit" = one (pixel, AOV-sample) pair yielded by the filter's sample iterator
 *     (src/lentil_filter.cpp:105); "draw" = one backward trace attempt for a visit
 *     (src/lentil_filter.cpp:248,311).
 */
#ifndef LENTIL_HIP_H
#define LENTIL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LENTIL_ABI_VERSION 1

#define LENTIL_OK 0
#define LENTIL_ERR_INVALID (-1)     /* bad argument / call order */
#define LENTIL_ERR_HIP (-2)         /* a HIP runtime call failed */
#define LENTIL_ERR_UNSUPPORTED (-3) /* parameter combination not implemented on the GPU */
#define LENTIL_ERR_NOMEM (-4)

/* enum CameraType, src/lentil.h:75-78 */
#define LENTIL_THINLENS 0
#define LENTIL_POLYNOMIAL_OPTICS 1
/* enum UnitModel, src/lentil.h:67-72 */
#define LENTIL_UNIT_MM 0
#define LENTIL_UNIT_CM 1
#define LENTIL_UNIT_DM 2
#define LENTIL_UNIT_M 3
/* AOVData::original_filter, src/aov_data.h:120, src/lentil.h:189-191 */
#define LENTIL_FILTER_GAUSSIAN 0
#define LENTIL_FILTER_CLOSEST 1
#define LENTIL_FILTER_VARIANCE 2
/* the lentil_debug AOV (src/lentil_operator.cpp:99-111): closest-filtered through its own z-buffer, fed by
 * redistributed draws only, value = the visit's draw count; takes no visit column (extra[k-1] may be NULL) */
#define LENTIL_FILTER_CLOSEST_DEBUG 3
/* pupil geometry strings "cyl-y" / "cyl-x" / anything else, src/lentil.h:387-389 */
#define LENTIL_GEOM_SPHERICAL 0
#define LENTIL_GEOM_CYL_Y 1
#define LENTIL_GEOM_CYL_X 2

#define LENTIL_MAX_AOVS 16 /* RGBA + up to 15 more redistributed AOVs */
#define LENTIL_MAX_CRYPTO 9 /* cryptomatte AOVs: crypto_{material,object,asset}{00,01,02} */

/* ------------------------------------------------------------------------------------
 * Camera state the kernels need: the fields of `struct Camera` (src/lentil.h:92-196,
 * SURVEY.md appendix B) that filter_pixel / trace_ray_bw_po / add_to_buffer read, with
 * the reference's own names and float/double widths (appendix C.10).  Values are the
 * ones *after* get_lentil_camera_params() clamping (src/lentil.h:1189-1243) and
 * camera_model_specific_setup() (src/lentil.h:1568-1670): e.g. PO focus_distance is
 * already x10 (mm), bokeh_anamorphic is already 1 - param.
 * ---------------------------------------------------------------------------------- */
typedef struct lentil_params {
  int32_t cameraType;      /* LENTIL_THINLENS | LENTIL_POLYNOMIAL_OPTICS */
  int32_t unitModel;       /* LENTIL_UNIT_* */
  int32_t enable_dof;
  int32_t vignetting_retries;      /* default 15, src/lentil_camera.cpp:44 */
  int32_t bokeh_aperture_blades;
  int32_t bokeh_enable_image;
  int32_t bidir_sample_mult;
  int32_t enable_bidir_transmission;
  int32_t enable_skydome;
  int32_t abb_chromatic_type;
  int32_t adaptive_sampling;       /* options.enable_adaptive_sampling, src/lentil_filter.cpp:74 */
  int32_t samples_override;        /* 0: reference draw-count formula (src/lentil_filter.cpp:177-202);
                                      >0: fixed accepted-draw count per redistributed visit (bench configs) */
  uint32_t xres, yres;             /* buffer size incl. the +1 quirk, src/lentil.h:1079-1080 */
  uint32_t xres_without_region, yres_without_region;
  int32_t region_min_x, region_min_y;

  double sensor_width;
  double focus_distance;
  double aperture_radius;
  double sensor_shift;
  double bidir_add_energy_minimum_luminance;

  float focal_length;
  float bidir_add_energy;
  float bidir_add_energy_transition;
  float abb_spherical;
  float abb_coma;
  float abb_distortion;
  float abb_chromatic;
  float circle_to_square;
  float bokeh_anamorphic;
  float optical_vignetting_distance;
  float optical_vignetting_radius;
  float filter_width;
  float inverse_sample_density;    /* 1/AA^2 as computed at src/lentil_filter.cpp:83-84 (non-adaptive) */
  float lambda_bw;                 /* 0.55, src/lentil_filter.cpp:254 */

  /* AiWorldToCameraMatrix(camera, time) of a static camera, row-vector convention
   * (p' = p * M, translation in row 3), src/lentil_filter.cpp:143-144 */
  float world_to_camera[4][4];
} lentil_params;

/* ------------------------------------------------------------------------------------
 * Lens table: replaces the generated `case <lens>: {...}` bodies spliced in at
 * src/lentil.h:1262,1278,1308,1576 (absent from the reference tree).  One sparse
 * 5-variate polynomial per output; a term is  c * x^e0 * y^e1 * dx^e2 * dy^e3 * lambda^e4
 * with integer powers evaluated like lens_ipow (src/lens.h:226-233), terms summed in
 * table order.  Partial derivatives are derived from these terms inside the library.
 * ---------------------------------------------------------------------------------- */
typedef struct lentil_term {
  double c;
  uint8_t e[5];
  uint8_t pad[3];
} lentil_term;

typedef struct lentil_poly {
  uint32_t first; /* index of first term in lentil_lens_table::terms */
  uint32_t count;
} lentil_poly;

typedef struct lentil_lens_table {
  /* lens constants, src/lentil.h:106-120 */
  double lens_outer_pupil_radius;
  double lens_inner_pupil_radius;
  double lens_length;
  double lens_back_focal_length;
  double lens_effective_focal_length;
  double lens_aperture_pos;
  double lens_aperture_housing_radius;
  double lens_inner_pupil_curvature_radius;
  double lens_outer_pupil_curvature_radius;
  double lens_field_of_view;
  double lens_fstop;
  double lens_aperture_radius_at_fstop;
  int32_t lens_inner_pupil_geometry; /* LENTIL_GEOM_* */
  int32_t lens_outer_pupil_geometry;
  lentil_poly out[5]; /* outer pupil x, y, dx, dy, transmittance (pt_evaluate) */
  lentil_poly ap[4];  /* aperture plane x, y, dx, dy (pt_evaluate_aperture) */
  uint32_t n_terms;
  uint32_t reserved;
  const lentil_term *terms; /* host pointer, copied by lentil_hip_set_lens */
} lentil_lens_table;

/* Bokeh-image importance tables exactly as imageData::bokehProbability leaves them
 * (src/imagebokeh.h:143-338); host pointers, copied by lentil_hip_set_bokeh. */
typedef struct lentil_bokeh_table {
  int32_t x, y;
  const float *cdfRow;          /* y   */
  const int32_t *rowIndices;    /* y   */
  const float *cdfColumn;       /* x*y */
  const int32_t *columnIndices; /* x*y */
} lentil_bokeh_table;

/* ------------------------------------------------------------------------------------
 * Visit stream: what filter_pixel gathers per AOV sample (src/lentil_filter.cpp:115-164,
 * 206-234), as fp32 columns of 4 floats per visit (16-byte rows, so one wave reads
 * 1 KiB per column per load):
 *     rgba          : sample RGBA                                   (:115)
 *     pos_z         : P world space .xyz, Z                         (:116-117)
 *     raydir_time   : lentil_raydir .xyz, lentil_time               (:121,141)
 *     volume_ignore : volume .rgb, lentil_ignore                    (:135,162)
 *     transmission  : transmission RGBA                             (:152)
 *     extra[k]      : AOV k+1 already widened to RGBA               (:214-232)
 * = 80 + 16*K bytes per visit.  Visits are pixel-major in iterator order.
 *
 * Pixel mapping.  visits_per_pixel > 0: uniform footprint; visit v belongs to source
 * pixel p = v / visits_per_pixel with  px = pixel_x0 + p % pixels_per_row,
 * py = pixel_y0 + (p / pixels_per_row) * pixel_row_stride  (region-relative, i.e. after
 * src/lentil_filter.cpp:100-101; row_stride > 1 expresses a row-interleaved multi-GPU
 * partition).  visits_per_pixel == 0: `pixel` holds px | (py << 16) per visit and
 * `inv_density` (optional) the per-visit inverse sample density (adaptive sampling or
 * ragged footprints, src/lentil_filter.cpp:83-84,109).
 * ---------------------------------------------------------------------------------- */
typedef struct lentil_visits {
  uint64_t n;
  uint32_t visits_per_pixel;
  uint32_t pixels_per_row;
  int32_t pixel_x0, pixel_y0;
  uint32_t pixel_row_stride;
  uint32_t n_extra;           /* K: number of extra AOV columns */
  const float *rgba;
  const float *pos_z;
  const float *raydir_time;
  const float *volume_ignore;
  const float *transmission;
  const float *extra[LENTIL_MAX_AOVS - 1];
  const uint32_t *pixel;      /* optional, see above */
  const float *inv_density;   /* optional */
} lentil_visits;

/* counters of the last lentil_hip_redistribute (device-side, fetched on demand) */
typedef struct lentil_counters {
  uint64_t visits;
  uint64_t redistributed_visits; /* visits that entered the draw loop */
  uint64_t attempted_draws;      /* total_samples_taken summed, src/lentil_filter.cpp:248 */
  uint64_t accepted_draws;
  uint64_t worklist_overflow;    /* non-zero => work list too small, results incomplete */
  uint64_t newton_iterations;    /* lane-iterations of the lt_sample_aperture solver (PO draw kernel) */
  uint64_t tries;                /* aperture draws = solves started (attempts x vignetting retries) */
  uint64_t lane_rounds;          /* 64 x scheduler rounds: iteration slots offered (utilisation = iterations / this) */
  uint64_t slow_solves;          /* solves finished by the one-wave-per-solve straggler kernel (LENTIL_SLOW_AT) */
  uint64_t blind_chunks;         /* chunks whose draw rounds were enqueued without waiting for their scan (sized from the previous pass) */
  uint64_t fallback_chunks;      /* ... of which did not fit and were redone with exact sizes */
  uint64_t streamed;             /* 1: the pass ran streamed (one scan launch feeding persistent solve waves; counts as one blind chunk) */
} lentil_counters;

/* Sums over the passes whose end has been looked at since the last reset (lentil_hip_pass_totals): what a caller that pipelines
 * frames reads once, after the frames, instead of lentil_hip_get_counters / _last_timing after every pass (each of which waits
 * for the pass).  Times are HIP-event times as lentil_hip_last_timing reports them. */
typedef struct lentil_pass_totals {
  uint64_t passes;               /* lentil_hip_redistribute calls accounted for */
  uint64_t streamed;             /* ... that ran streamed */
  uint64_t blind_chunks, fallback_chunks;      /* as lentil_counters, summed */
  uint64_t deferred;             /* passes that returned before their end was known (asynchronous end) */
  uint64_t abandoned;            /* ... whose frame was cleared before anybody observed it */
  uint64_t abandoned_incomplete; /* ... and which still needed work at that point (a second round, a redo): the frame nobody
                                  * looked at was not complete.  Their kernel times are in the sums all the same. */
  uint64_t visits, redistributed_visits, attempted_draws, accepted_draws, worklist_overflow;
  uint64_t newton_iterations, tries, lane_rounds, slow_solves;
  uint64_t scan_launches;
  uint64_t rounds_max;           /* most solve/accept rounds any of the passes needed */
  double scan_ms, draw_ms, resolve_ms;
} lentil_pass_totals;

/* one accepted draw, for index-parity tests: (visit, attempt n, linear pixel).  Polynomial optics with abb_chromatic != 0:
 * attempt is n | channel << 30, channel 0, 1, 2 for the reference's -1, 0, 1 (an attempt can have three records). */
typedef struct lentil_draw_record {
  uint32_t visit;
  uint32_t attempt;
  uint32_t pixel;
} lentil_draw_record;

typedef struct lentil_hip_ctx lentil_hip_ctx;

/* --- lifetime ----------------------------------------------------------------------
 * replaces `new Camera()` / `delete camera_data` buffer ownership
 * (src/lentil_camera.cpp:58-61,70-75; Camera::destroy_buffers src/lentil.h:1143-1148). */
int lentil_hip_abi_version(void);
int lentil_hip_create(int device, lentil_hip_ctx **out_ctx);
int lentil_hip_destroy(lentil_hip_ctx *ctx);
const char *lentil_hip_last_error(const lentil_hip_ctx *ctx);
/* Diagnostics, no counterpart in the reference: why the last streamed pass of this context that was redone the chunked way
 * (lentil_counters::fallback_chunks) gave up -- which buffer bound or which waiting wave, with the pass's sizes.  "" if none
 * was.  The redo is invisible in the results (the frame is the reference's either way); it costs time. */
const char *lentil_hip_last_redo_note(const lentil_hip_ctx *ctx);

/* --- setup (once per render) -------------------------------------------------------
 * set_params : Camera::get_lentil_camera_params + camera_model_specific_setup results
 *              (src/lentil.h:1189-1243,1568-1670)
 * set_lens   : load_lens_constants.h / load_lt_sample_aperture.h / load_pt_evaluate.h
 *              splices (src/lentil.h:1262,1278,1308,1576)
 * set_bokeh  : imageData tables (src/imagebokeh.h:30-37) after bokehProbability
 * alloc_frame: Camera::setup_filter + AOVData::allocate_regular_buffers
 *              (src/lentil.h:1096-1121, src/aov_data.h:140-143).  AOV 0 is "RGBA" and is
 *              the one that feeds filter_weight_buffer (src/lentil.h:827-828).
 *              xres/yres are taken from the params. */
int lentil_hip_set_params(lentil_hip_ctx *ctx, const lentil_params *params);
int lentil_hip_set_lens(lentil_hip_ctx *ctx, const lentil_lens_table *lens);
int lentil_hip_set_bokeh(lentil_hip_ctx *ctx, const lentil_bokeh_table *bokeh);
/* The reference compiles every lens into the plugin (switch(lensModel) over generated code,
 * src/lentil.h:1262,1278,1308); liblentil_hip likewise carries straight-line kernels for the lens
 * tables it ships (tools/gen_lens_code.py) and recognises them by a hash of the table passed to
 * set_lens.  Any other table runs through the LDS table interpreter (same arithmetic, slower).
 * lens_is_compiled: 1 if the current table has a compiled-in kernel.  set_lens_mode: 0 = auto,
 * 1 = always interpret the table (parity tests compare the two) -- in the passes' solve kernels, in
 * lentil_hip_camera_rays and in lentil_hip_focus_search alike. */
int lentil_hip_lens_is_compiled(lentil_hip_ctx *ctx);
int lentil_hip_set_lens_mode(lentil_hip_ctx *ctx, int mode);
/* A table that has no kernel compiled into the library gets one at run time -- the reference compiles every lens into the plugin
 * (include/auto_generated_lens_includes/load_lt_sample_aperture.h:4-47, used at src/lentil.h:1308): lentil_hip_set_lens starts a
 * thread that emits the lens's straight-line code, compiles it with hiprtc and keeps the code object in a cache on disk
 * (LENTIL_JIT_CACHE, default ~/.cache/lentil_hip); passes run the table interpreter until it is there.  Same results bit for
 * bit.  status: *state 0 nothing to compile (compiled-in lens, thin lens, LENTIL_LENS_JIT=0), 1 compiling, 2 the specialised
 * kernel is in use, -1 compilation failed (the interpreter keeps serving the lens); *compile_seconds: what the compilation took
 * (0 from the cache).  wait: blocks until the state is no longer 1 (timeout_seconds <= 0: no limit); an error if it failed.
 * debug_lens_jit_source: the emitted lens code (tests compare it with tools/gen_lens_code.py's). */
int lentil_hip_lens_jit_status(lentil_hip_ctx *ctx, int *state, double *compile_seconds);
int lentil_hip_lens_jit_wait(lentil_hip_ctx *ctx, double timeout_seconds);
int lentil_hip_debug_lens_jit_source(lentil_hip_ctx *ctx, char *buf, uint64_t capacity, uint64_t *length);
/* ... and without a context or a GPU (hiprtc cross-compiles): pack the table, emit the lens code and, compile != 0, compile the
 * four solve kernels and the camera-rays kernel; the emitted source and the compiler's log are copied out (truncated to the capacities). */
int lentil_hip_debug_lens_jit_compile(const lentil_lens_table *t, int compile, char *source, uint64_t source_capacity,
                                      uint64_t *source_length, char *log, uint64_t log_capacity, double *seconds, uint64_t *code_bytes);
int lentil_hip_alloc_frame(lentil_hip_ctx *ctx, uint32_t n_aovs, const uint8_t *aov_filter_kind);

/* A moving camera.  The reference asks Arnold for the matrix at every AOV sample's own time:
 * AiWorldToCameraMatrix(camera_node, lentil_time) (src/lentil_filter.cpp:141-144).  Here the caller hands over n_keys
 * world-to-camera matrices (row-vector convention like lentil_params::world_to_camera) at equidistant times over the
 * camera's shutter, shutter_start + k / (n_keys - 1) * (shutter_end - shutter_start) -- samples of AiWorldToCameraMatrix
 * at those absolute times -- and every visit uses the component-wise interpolation ((b - a) * f) + a of the two keys around
 * its lentil_time (raydir_time column, .w: Arnold's absolute sample time, inside the shutter; times outside it clamp to the
 * first / last key).  n_keys <= 1 or NULL: the static matrix of lentil_params again.  With keys the scan reads the
 * raydir_time column for every visit (80 instead of 64 bytes moved per visit) and runs register-staged.
 * set_camera_shutter: the shutter interval the keys span (Arnold's camera.shutter_start / .shutter_end; a centred shutter
 * is -0.25 ... 0.25); 0 ... 1 until set.  shutter_end must be greater than shutter_start. */
#define LENTIL_MAX_MOTION_KEYS 16
int lentil_hip_set_camera_motion(lentil_hip_ctx *ctx, uint32_t n_keys, const float *world_to_camera);
int lentil_hip_set_camera_shutter(lentil_hip_ctx *ctx, float shutter_start, float shutter_end);

/* Camera::logarithmic_focus_search (src/lentil.h:1445-1460; called per camera update at :1632): the sensor
 * shift, among the 20 001 candidates of logarithmic_values() (src/lens.h:395-407), whose axial ray crosses
 * the optical axis closest in front of focal_distance (mm).  One GPU lane per candidate instead of the
 * reference's sequential loop; the winner is the one that loop keeps (first smallest positive miss).
 * Uses the table of set_lens; lambda in micrometres. */
int lentil_hip_focus_search(lentil_hip_ctx *ctx, double focal_distance, double lambda, double *best_sensor_shift);

/* --- visit stream ------------------------------------------------------------------
 * upload_visits: host columns -> library-owned device memory (what the capturing
 *                filter_pixel hands over once per frame).
 * bind_visits  : columns already resident in HBM (device pointers owned by the caller). */
int lentil_hip_upload_visits(lentil_hip_ctx *ctx, const lentil_visits *host_visits);
int lentil_hip_bind_visits(lentil_hip_ctx *ctx, const lentil_visits *device_visits);

/* The same hand-over piece by piece, while the renderer is still rendering: a capturing filter_pixel
 * (src/lentil_filter.cpp:66-436 runs per pixel on many bucket threads) fills blocks of visits and sends each
 * block as it fills, so that the PCIe transfer (80 B per visit: 0.11 s for a 4K frame in one piece) hides
 * behind the render and the frame end waits for the last block only.
 * host_alloc / host_free : page-locked host memory for those blocks (copies from it are asynchronous DMA;
 *                ordinary memory works too, the copy then returns when the runtime has staged it).
 * visits_begin : starts a frame's stream.  `layout` gives its geometry (visits_per_pixel, pixels_per_row,
 *                pixel_x0/y0, pixel_row_stride, n_extra; n and the column pointers are ignored, except that
 *                inv_density != NULL announces per-visit densities for a ragged stream).  capacity_hint:
 *                expected number of visits (0: unknown; the columns grow by doubling).  Waits for the
 *                previous pass; the previous frame's device columns are reused when they fit.
 * visits_append: part->n visits (host columns) go to the end of the stream, in call order; thread-safe.
 *                Returns at once; *ticket (may be NULL) identifies the copies.
 * visits_wait  : returns when the copies of that ticket are complete -- the block may be refilled.
 * visits_end   : waits for all copies and makes the assembled stream the context's visits (as upload_visits
 *                would have); *n_visits (may be NULL) returns their number. */
int lentil_hip_host_alloc(void **host_ptr, uint64_t bytes);
int lentil_hip_host_free(void *host_ptr);
int lentil_hip_visits_begin(lentil_hip_ctx *ctx, const lentil_visits *layout, uint64_t capacity_hint);
int lentil_hip_visits_append(lentil_hip_ctx *ctx, const lentil_visits *part, uint64_t *ticket);
int lentil_hip_visits_wait(lentil_hip_ctx *ctx, uint64_t ticket);
int lentil_hip_visits_end(lentil_hip_ctx *ctx, uint64_t *n_visits);

/* --- the hot path ------------------------------------------------------------------
 * clear_frame : zero-initialisation done by std::vector::resize (src/lentil.h:1096-1098)
 * redistribute: the filter_pixel visit loop (src/lentil_filter.cpp:91-451) for every bound
 *               visit: predicate + draw count, trace_ray_bw_po / thin-lens draws,
 *               add_to_buffer / filter_and_add_to_buffer_new (src/lentil.h:823-851,938-955).
 *               Accumulates on top of whatever the frame holds (call clear_frame first).
 *               Returns when the pass is complete on the device: it ends with a read-back of the
 *               pass's counters (did everything fit the buffers sized from the previous pass? is any
 *               visit still short of draws?), after which it redoes or continues what is needed.
 *               LENTIL_ERR_NOMEM if the device had to drop work (a frame that is incomplete).
 *               clear_frame, resolve and the row / exchange calls are asynchronous on the context's
 *               stream (lentil_hip_stream); downloads and lentil_hip_sync wait for it.
 * resolve     : driver_process_bucket's normalisation (src/lentil_imager.cpp:112-118,169-186)
 *               into a separate resolved image (the accumulators stay intact).  A streamed pass has
 *               usually done it on its way (beside its second round); the call then costs nothing. */
int lentil_hip_clear_frame(lentil_hip_ctx *ctx);
int lentil_hip_redistribute(lentil_hip_ctx *ctx);
int lentil_hip_resolve(lentil_hip_ctx *ctx);
int lentil_hip_sync(lentil_hip_ctx *ctx);

/* --- results -----------------------------------------------------------------------
 * download_aov     : resolved AOV as xres*yres RGBA floats (what the imager writes into
 *                    bucket_data, src/lentil_imager.cpp:178,182)
 * download_accum   : raw accumulators: AOVData::buffer (xres*yres*4) and
 *                    filter_weight_buffer (xres*yres); either pointer may be NULL */
int lentil_hip_download_aov(lentil_hip_ctx *ctx, uint32_t aov, float *host_rgba);
int lentil_hip_download_accum(lentil_hip_ctx *ctx, uint32_t aov, float *host_rgba, float *host_weight);
/* download_records : every AOV's accumulators and the weight in ONE copy, as the device keeps them: xres*yres records of
 *                    *stride floats -- AOV a's RGBA at floats 4a .. 4a+3, the weight at float 4 * n_aovs, padding behind it.
 *                    host_records holds capacity_floats floats (LENTIL_ERR_INVALID if that is fewer than xres*yres * stride;
 *                    host_records NULL: only *stride is set).  download_accum copies this whole block per call and picks
 *                    one AOV's columns: a caller that looks at all AOVs of a 4K frame wants this instead. */
int lentil_hip_download_records(lentil_hip_ctx *ctx, float *host_records, uint64_t capacity_floats, uint32_t *stride);

/* Thin lens with abb_chromatic > 0 (src/lentil_filter.cpp:393-406): every attempt that passes the optical
 * vignetting test draws its colour channel from xor128 (src/global.h:22-27), whose state the reference
 * keeps in function statics -- one per process, advanced by whichever thread gets there first.  Here the
 * order is the single-threaded one (visits in stream order, attempts in order) and the state is explicit:
 * it starts at the generator's initial constants, every lentil_hip_redistribute continues from where the
 * previous one stopped, and a host that wants another starting point (or to mirror draws it made itself)
 * reads / writes the four words x, y, z, w.
 * Across GPUs (a communicator from lentil_hip_comm_init, either partition, world size 1 included) the order is the same
 * one over the whole frame: items in frame-wide visit-id order, whichever rank holds them.  lentil_hip_redistribute is
 * then a collective step -- every rank calls it, with visits of its own or none -- after which every rank's draws and
 * channels are those a single context of the whole frame makes, and every rank's state is the WHOLE frame's last one, so
 * the next pass continues as one GPU would.  Give every rank the same starting state.  Visit ids must be frame-wide and
 * distinct: the two partitions derive them from pixel_y0 / pixel_row_stride; a ragged stream numbers its visits from
 * visit_id_base (lentil_hip_set_closest_exchange), so give each rank the range its visits hold in the frame's order.  Items
 * of two ranks with one id make every rank refuse the pass (LENTIL_ERR_INVALID).  As with the exchanges, an error a rank
 * meets on its own before the ranks' lists are exchanged (work-list overflow, out of device memory) returns on that rank
 * only and leaves the others waiting in the exchange: treat it as fatal to the communicator.  Without the library's
 * communicator (lentil_hip_set_closest_exchange(ctx, 1, ...) alone) such a pass is refused.
 * lentil_hip_tl_chroma_stats: for the last such pass, the frame's items (redistributed visits; without a communicator
 * this context's), those whose generator use depends on the channels drawn (dependent_items: walked in order, the others
 * in parallel; 0 without a communicator, where one block walks every item in order), and the payload bytes this rank
 * received from the others.  Any pointer may be NULL.  Instrumentation. */
int lentil_hip_set_xor128_state(lentil_hip_ctx *ctx, const uint32_t state[4]);
int lentil_hip_get_xor128_state(lentil_hip_ctx *ctx, uint32_t state[4]);
int lentil_hip_tl_chroma_stats(lentil_hip_ctx *ctx, uint64_t *items, uint64_t *dependent_items, uint64_t *gathered_bytes);

/* Closest-filtered AOVs across GPUs (the reference's single z-buffer, src/lentil.h:832-837).
 * deferred != 0: lentil_hip_redistribute leaves the per-pixel winner keys -- (bits of |Z|) << 32 |
 * (0xFFFFFFFF - frame-wide visit id), empty = all ones -- in lentil_hip_zkey_buffer instead of gathering
 * the winners' values.  The caller takes the unsigned 64-bit minimum of that buffer over all GPUs, then
 * calls lentil_hip_closest_gather on each: a GPU writes the values of the winners it owns and leaves the
 * others zero, so the sum all-reduce of lentil_hip_accum_buffer completes the closest AOVs too.
 * Frame-wide visit ids: uniform streams derive them from pixel_y0 / pixel_row_stride (the id a single
 * process walking the whole frame would give the visit -- row bands and row-interleaved partitions alike);
 * ragged streams use visit_id_base + index.
 * Candidates at depth 0 / NaN (order-dependent upstream, lentil_closest_replay.h): with the library's communicator
 * (lentil_hip_comm_init) the pass leaves them to lentil_hip_allreduce / _exchange_bands, which replay their pixels over every
 * rank's candidates; a caller that min-reduces the keys itself (deferred != 0, no communicator) gets the pass refused
 * (LENTIL_ERR_UNSUPPORTED). */
int lentil_hip_set_closest_exchange(lentil_hip_ctx *ctx, int deferred, uint32_t visit_id_base);
int lentil_hip_zkey_buffer(lentil_hip_ctx *ctx, void **device_ptr, uint64_t *n_keys);
int lentil_hip_closest_gather(lentil_hip_ctx *ctx);

/* --- multi-GPU, tiled output (BASELINE north_star: "the output frame tiles across the GPUs,
 * cross-tile splat contributions are exchanged") ------------------------------------------------------
 * Every GPU processes the visits of its band of rows into full-frame accumulators; what its draws add
 * outside the band belongs to the band's owner.
 * touched_rows : [row_lo, row_hi) of the frame the last redistribute added anything to (own visits and
 *                splats; 0,0 when nothing).  Also lets the next clear_frame wipe only those rows.
 * merge_rows   : merges n_rows rows, starting at row_begin, of another GPU's accumulator block (device
 *                memory, same record layout: xres * stride floats per row; stride = n_floats of
 *                accum_buffer / (xres * yres)) into this frame: gaussian slots and the weight add up,
 *                closest-filtered slots follow the smaller winner key (dev_key_rows: the matching rows of
 *                the sender's lentil_hip_zkey_buffer, required iff the frame has closest AOVs; the sender
 *                must have gathered its local winners, i.e. not be in deferred mode).
 * pack_rows / merge_packed_rows : the same exchange without the padding of the pixel records: pack_rows writes
 *                n_rows * xres * (4 n_aovs + 1) floats (a record's RGBA values and weight, back to back) to
 *                dev_dst; merge_packed_rows merges rows that arrived in that form.  5 instead of 8 floats per
 *                pixel for a beauty-only frame.
 * compact_rows / merge_sparse : the same exchange for rows that are mostly empty (a band's draws reach ~100 rows into
 *                its neighbours but touch ~2 % of their pixels when highlights are rare): compact_rows turns every
 *                pixel of the rows that holds anything (weight != 0, or a winner key) into one entry -- frame-wide
 *                pixel index (uint32), its 4 n_aovs + 1 floats, its key (uint64, only with closest AOVs) -- in three
 *                device arrays of `capacity` entries and returns the number of entries found (synchronises; if it
 *                exceeds capacity nothing beyond capacity was written: send the rows whole instead).  merge_sparse
 *                merges n such entries of one sender, all inside rows [row_begin, row_begin + n_rows).
 * resolve_rows : lentil_hip_resolve restricted to a band of rows. */
int lentil_hip_touched_rows(lentil_hip_ctx *ctx, int32_t *row_lo, int32_t *row_hi);
int lentil_hip_merge_rows(lentil_hip_ctx *ctx, uint32_t row_begin, uint32_t n_rows, const void *dev_acc_rows,
                          const void *dev_key_rows);
int lentil_hip_pack_rows(lentil_hip_ctx *ctx, uint32_t row_begin, uint32_t n_rows, void *dev_dst);
int lentil_hip_merge_packed_rows(lentil_hip_ctx *ctx, uint32_t row_begin, uint32_t n_rows, const void *dev_packed_rows,
                                 const void *dev_key_rows);
int lentil_hip_compact_rows(lentil_hip_ctx *ctx, uint32_t row_begin, uint32_t n_rows, void *dev_idx, void *dev_vals,
                            void *dev_keys, uint32_t capacity, uint32_t *count);
int lentil_hip_merge_sparse(lentil_hip_ctx *ctx, uint32_t row_begin, uint32_t n_rows, uint32_t n, const void *dev_idx,
                            const void *dev_vals, const void *dev_keys);
int lentil_hip_resolve_rows(lentil_hip_ctx *ctx, uint32_t row_begin, uint32_t n_rows);

/* --- multi-GPU ---------------------------------------------------------------------
 * accum_buffer: device pointer + float count of the contiguous accumulator block (one record per
 *               pixel: n_aovs x RGBA, the filter weight, padding to a multiple of 8 floats); a sum
 *               all-reduce over it (RCCL) merges the cross-tile splats of all GPUs (SURVEY.md
 *               section 8e).  The reference has no counterpart (single process, shared buffers). */
int lentil_hip_accum_buffer(lentil_hip_ctx *ctx, void **device_ptr, uint64_t *n_floats);
int lentil_hip_stream(lentil_hip_ctx *ctx, void **hip_stream);

/* --- multi-GPU, the exchange itself (RCCL over xGMI; one process per GPU, one context per process) ------
 * The library owns its communicator: librccl.so is loaded on the first of these calls (dlopen; a process
 * that already holds an RCCL gets that same instance), so a renderer linking liblentil_hip.so for one GPU
 * needs no RCCL.  No reference counterpart (src/lentil.h:823-851 adds into buffers all threads share).
 * comm_unique_id : rank 0 fills the 128-byte id (ncclGetUniqueId) and hands it to the other processes by
 *                  whatever channel the host has (the renderer's own job description, a file, MPI ...).
 * comm_init      : collective over `world` processes, rank in [0, world); replaces an earlier communicator.
 * allreduce      : row-interleaved partition, every GPU holds the whole frame.  After lentil_hip_redistribute
 *                  on every rank: closest-AOV winner keys are min-reduced and the winners gathered (requires
 *                  set_closest_exchange(deferred = 1) when the frame has closest AOVs), then one sum all-reduce
 *                  of accum_buffer.  lentil_hip_resolve afterwards gives every rank the whole image.
 *                  Frames with closest AOVs start with a one-word all-gather (did any rank's pass meet a candidate at
 *                  depth 0 / NaN?); if one did, the pixels such candidates reached are replayed in frame-wide visit order
 *                  over every rank's candidates (all-gathered) before the gather: the same winner keys on every rank.
 * exchange_bands : tiled output.  Rank r's visits are rows [bounds[r], bounds[r+1]) (bounds == NULL: an even split
 *                  of visit_rows); its band of the frame is the same rows, the last band reaching to yres.
 *                  After lentil_hip_redistribute on every rank: the touched rows are all-gathered, what a
 *                  rank added to another's band travels point to point (sparse != 0: as pixel entries when
 *                  at most a quarter of the pixels hold anything, else as packed rows), the owner merges
 *                  the arrivals in rank order and resolves its band; band_lo / band_hi (may be NULL) return it.
 *                  Frames with closest AOVs: the same one-word agreement first; if some rank met a candidate at depth
 *                  0 / NaN, every rank's candidates at the flagged pixels go to the owner with their values, and the owner
 *                  replays those pixels in visit order after its merges, before the resolve.  In both exchanges a rank
 *                  whose pass kept no complete draw log runs it again with one first (lentil_hip_degenerate_stats).
 *                  Collective: every rank calls it with the same bounds / visit_rows / sparse. */
int lentil_hip_comm_unique_id(uint8_t id[128]);
int lentil_hip_comm_init(lentil_hip_ctx *ctx, const uint8_t id[128], int rank, int world);
int lentil_hip_comm_destroy(lentil_hip_ctx *ctx);
int lentil_hip_allreduce(lentil_hip_ctx *ctx);
int lentil_hip_exchange_bands(lentil_hip_ctx *ctx, const int32_t *bounds, int32_t visit_rows, int32_t sparse,
                              int32_t *band_lo, int32_t *band_hi);
/* payload bytes this rank sent / received over xGMI in its last lentil_hip_exchange_bands (pixel entries or packed rows,
 * winner keys included) or lentil_hip_allreduce (ring traffic of the reduced buffers); either pointer may be NULL.
 * Instrumentation for the scaling bench; no reference counterpart. */
int lentil_hip_exchange_stats(lentil_hip_ctx *ctx, uint64_t *bytes_sent, uint64_t *bytes_received);
/* lentil_hip_exchange_bands(sparse != 0) since the communicator was made: exchanges that ran in the fixed-capacity form
 * (every message's size known to both ends beforehand, no host wait between compaction and merge) and directed pairs whose
 * entries did not fit their message and followed as whole rows; either pointer may be NULL.  Instrumentation. */
int lentil_hip_exchange_counts(lentil_hip_ctx *ctx, uint64_t *fixed_form, uint64_t *pairs_overflowed);
/* Closest-filtered candidates at depth (Z) 0 or NaN (src/lentil.h:832-845: their outcome depends on the order of the
 * candidates at the pixel), for the last lentil_hip_redistribute and the exchange behind it: *degenerate = 1 when the pass
 * met one in a frame with a closest-filtered AOV; the distinct pixels the ranks flagged for the replay across GPUs; the
 * candidate nodes this rank sent to / received from other ranks; passes wiped and run again to get a draw log (one GPU: the
 * pass itself; across GPUs: inside the exchange, on a rank that met no such candidate but holds draws at a flagged pixel).
 * Any pointer may be NULL.  Instrumentation. */
int lentil_hip_degenerate_stats(lentil_hip_ctx *ctx, uint32_t *degenerate, uint64_t *flagged_pixels, uint64_t *nodes_sent,
                                uint64_t *nodes_received, uint64_t *passes_rerun);
/* *concurrent = 1 when the four HIP streams a streamed pass keeps kernels resident on run them side by side (they were
 * chosen so at lentil_hip_create: streams that share one of the runtime's hardware queues serialise, and the pass then
 * takes about 1.5 x as long; 2: and a fifth one beside them, on which a pass with cryptomatte AOVs replays the own-pixel
 * adds while its draws go on -- GPU_MAX_HW_QUEUES > 4), 0 when fewer than four hardware queues were to be had or
 * LENTIL_STREAM_PROBE=0.
 * Instrumentation; no reference counterpart. */
int lentil_hip_streams_concurrent(lentil_hip_ctx *ctx, int *concurrent);
/* What this GPU delivers right now, for putting timings of different boxes side by side (bench.py's `box` block; no reference
 * counterpart).  Three short kernels on the context's stream, ~10 ms in all:
 *   probe[0]  fp64 multiply / add rate of dependent chains, three waves per SIMD on every CU -- the form of the Newton solves
 *             (no FMA) -- in TFLOP/s; [1] the shader clock it ran at, MHz (clock64() against the 100 MHz real-time counter);
 *   probe[2]  float4 copy, GB/s read + written; [3] float4 read-only stream, GB/s;
 *   probe[4]  hardware queues the runtime multiplexes this process's streams onto (GPU_MAX_HW_QUEUES as the library sees it;
 *             0: unset, the runtime's default of 4); [5] compute units. */
int lentil_hip_box_probe(lentil_hip_ctx *ctx, double probe[6]);

/* --- cryptomatte AOVs ------------------------------------------------------------------
 * The reference keeps a std::map<float, float> id -> weight and a total weight per pixel for every ranked
 * cryptomatte AOV (AOVData::crypto_hash_map / crypto_total_weight, src/aov_data.h:127-128,145-150).  Each add of a
 * visit to a pixel -- its own pixel (src/lentil.h:952) or the pixel of an accepted draw
 * (src/lentil_filter.cpp:296,443) -- adds the visit's cache {id -> weight} times the sample weight
 * (Camera::add_to_buffer_cryptomatte, src/lentil.h:814-819); the imager writes the pairs at positions rank, rank + 1
 * of a pixel's map sorted by weight (src/lentil_imager.cpp:121-161).
 *
 * lentil_crypto_visits carries, per cryptomatte AOV, the cache of every visit of the bound stream as `entries`
 * (id, weight) pairs (what Camera::cryptomatte_construct_cache, src/lentil.h:781-811, leaves: ids distinct; a pair
 * whose weight has the bits 0xFFFFFFFF is unused; -0 counts as +0, which is one key to the reference's map too).
 * Host arrays with lentil_hip_upload_crypto, device arrays with lentil_hip_bind_crypto; after the visits they belong
 * to (binding other visits makes them stale: the pass then refuses), before lentil_hip_redistribute.  lentil_hip_alloc_crypto follows lentil_hip_alloc_frame (which drops the tables);
 * slots_per_pixel is the number of distinct ids a pixel can hold (0: 16, at most 64) -- a pass that meets more
 * returns LENTIL_ERR_NOMEM, as does one whose accepted draws exceed the draw log the adds are replayed from (sized
 * by the library from the previous pass unless lentil_hip_set_draw_log was called; clear the frame and redistribute
 * again).  lentil_hip_clear_frame empties the tables.  Across GPUs the tables travel with the tiled exchange:
 * lentil_hip_exchange_bands sends the map entries this rank's draws added outside its band to the bands' owners (16-byte
 * records) and adds what arrives; lentil_hip_allreduce (interleaved rows) refuses contexts with cryptomatte AOVs.
 *
 * lentil_hip_download_crypto: np RGBA = (id, weight / total) of positions rank and rank + 1 -- rank 0 / 2 / 4 for
 * the AOVs named ...00 / ...01 / ...02 (:124-126); equal weights stay in id order (what std::sort does to the up
 * to 16 pairs it sorts by insertion).  host_has_rank (np bytes, may be NULL): 0 where the pixel's map has no more
 * than `rank` entries -- the reference stops copying the bucket row at such a pixel (:132-134).
 * lentil_hip_download_crypto_table: the raw tables (np * slots ids as bits, 0xFFFFFFFF = free, and weights; np
 * totals); any pointer may be NULL. */
typedef struct lentil_crypto_visits {
  uint64_t n;                               /* visits (the bound stream's n) */
  uint32_t n_crypto;                        /* cryptomatte AOVs */
  uint32_t entries;                         /* pairs per visit and AOV, 1..64 */
  const float *hash[LENTIL_MAX_CRYPTO];     /* n * entries ids */
  const float *weight[LENTIL_MAX_CRYPTO];   /* n * entries weights */
} lentil_crypto_visits;
int lentil_hip_alloc_crypto(lentil_hip_ctx *ctx, uint32_t n_crypto, uint32_t slots_per_pixel);
int lentil_hip_upload_crypto(lentil_hip_ctx *ctx, const lentil_crypto_visits *c);
int lentil_hip_bind_crypto(lentil_hip_ctx *ctx, const lentil_crypto_visits *c);
/* the caches with a piecewise upload (lentil_hip_visits_begin ... _end above): lentil_hip_visits_begin_crypto right
 * after _visits_begin announces `entries` pairs per visit and cryptomatte AOV; every part then goes through
 * lentil_hip_visits_append_crypto with its caches (caches->n == part->n; page-locked like the part); _visits_end
 * makes them the context's cryptomatte columns */
int lentil_hip_visits_begin_crypto(lentil_hip_ctx *ctx, uint32_t entries);
int lentil_hip_visits_append_crypto(lentil_hip_ctx *ctx, const lentil_visits *part, const lentil_crypto_visits *caches,
                                    uint64_t *ticket);
int lentil_hip_download_crypto(lentil_hip_ctx *ctx, uint32_t crypto, uint32_t rank, float *host_rgba, uint8_t *host_has_rank);
int lentil_hip_download_crypto_table(lentil_hip_ctx *ctx, uint32_t crypto, uint32_t *slots_per_pixel, uint32_t *host_id_bits,
                                     float *host_weight, float *host_total);

/* --- instrumentation ----------------------------------------------------------------
 * timings are HIP-event times on the context's stream for the last redistribute/resolve:
 * ms[0] scan+compaction+direct accumulate, ms[1] draw/splat kernel, ms[2] resolve. */
int lentil_hip_get_counters(lentil_hip_ctx *ctx, lentil_counters *out);
int lentil_hip_last_timing(lentil_hip_ctx *ctx, float ms[3]);
/* kernel launches of the last redistribute: n[0] scan launches (one per chunk of the visit stream; ms[0]
 * of last_timing covers all of them), n[1] solve/accept rounds of the chunk that needed most. */
int lentil_hip_last_launches(lentil_hip_ctx *ctx, uint32_t n[2]);
/* First batches sized from the lens and the frame (round 5).  The reference's loop (src/lentil_filter.cpp:248-299) keeps
 * tracing until `samples` draws of a sample have landed inside the frame, at most 5 x samples attempts of up to
 * vignetting_retries + 1 tries each (src/lentil.h:592-648); this library computes every trace once, in batches, and sizes a
 * sample's FIRST batch from a calibration of the lens (where its rays land, which it vignettes) so that a streamed pass needs
 * no second round of traces.  No result depends on it: surplus traces are never looked at, a shortfall is served by further
 * rounds.  stats[0] calibrations run, [1] passes that ran without a second round in flight, [2] ... of which needed one
 * after all, [3] sixteenths by which the model's margin has been widened since the camera set-up last changed.
 * debug_batch_estimate: the model's answer for n camera-space points (cm, z < 0 in front of the camera) and a draw count:
 * out[n][4] = share of the passing aperture points that land well inside the frame, share that land inside it, share the lens
 * vignettes, traces in the first batch.  LENTIL_ERR_INVALID without a polynomial-optics lens and parameters. */
int lentil_hip_batch_model_stats(lentil_hip_ctx *ctx, uint64_t stats[4]);
/* What the streamed passes of ALL contexts of this process have met (no context needed): stats[0] streamed passes begun,
 * [1] passes whose resident waves gave up waiting (the stuck time-out; the pass is then redone in the chunked form and its
 * result is the same), [2] ... of which were asked for (LENTIL_INJECT_STALL), [3] passes wiped and run again because draws
 * had been accepted by then.  A stall costs time, never results -- so nothing else would ever show one: the GPU test
 * session asserts stats[1] == stats[2] when it ends (tests/conftest.py). */
int lentil_hip_process_stats(uint64_t stats[4]);
/* ... and what the waves that gave up saw (lentil_hip_last_redo_note's text, one line per pass, the first eight that were not
 * asked for), NUL-terminated, truncated to capacity. */
int lentil_hip_process_stall_notes(char *buf, uint64_t capacity);
/* Occlusion probes (round 6).  The reference asks the renderer, before every backward trace, whether anything stands between the
 * sample and the point of the aperture the trace is to go through -- AiTraceProbe along the segment from the sample's world
 * position to cam_to_world * (-aperture * 0.1 / unit) (src/lentil.h:613-629; thin lens: to cam_to_world * (lens / unit),
 * src/lentil_filter.cpp:356-375) -- and a try that is occluded fails like one the lens vignettes (samples the skydome supplied are
 * exempt).  The GPU has no scene.  With a probe set, a pass runs in its round-by-round form, and in every round, once the
 * round's traces are solved and before any of them is accepted, the library hands the host ONE list of segments -- one per try
 * of the round that got through the lens (whether it landed in the frame or not: an occluded try hands its attempt on to the
 * next try) -- and the host answers one byte per segment, non-zero = occluded; the accept then treats those tries as failed.
 * Results are what the reference computes with the same probe (oracle: orc_frame_set_probe; tests/test_gpu_probe.py).
 *   fn(user, n, segments, occluded): called from the thread that called lentil_hip_redistribute, once per round and chunk;
 *   it may spread the n probes over threads of its own.  origin / target are world-space points; the reference's ray is
 *   AiMakeRay(AI_RAY_SHADOW, origin, normalize(target - origin), |target - origin|).
 *   camera_to_world: 16 floats, row-vector convention like lentil_params::world_to_camera (AiCameraToWorldMatrix); NULL: the
 *   inverse of params.world_to_camera (of every motion key, where lentil_hip_set_camera_motion has set keys), computed in fp64.
 *   fn == NULL switches probing off.
 *   Thin lens with abb_chromatic > 0: the reference draws an attempt's colour channel AFTER its probe, from one generator in visit
 *   order, and an occluded attempt draws none.  There the probes come before the walk that draws the channels, in a loop: the
 *   attempts every item can possibly reach (no item goes past its samples-th attempt that lands in the frame in all three
 *   channels) that have not been asked about go to the callback in ONE list, the occluded ones are lost, which lets items reach
 *   further -- until a turn has nothing to ask.  One callback per turn of that loop and pass (tests/test_gpu_probe_tl_chroma.py);
 *   with a communicator every rank asks about its own items.  A pass the library runs a second time (closest-filtered AOVs with
 *   candidates at depth 0 / NaN and no draw log) re-applies the first run's answers and does not call back.
 *   Polynomial optics with abb_chromatic != 0 and a probe: LENTIL_ERR_UNSUPPORTED from the pass.
 * Cost: INTEGRATION.md section 3c (the list travels over PCIe: 24 B out and 1 B back per try that got through the lens). */
typedef struct lentil_probe_segment {
  float origin[3];   /* the sample, world space */
  float target[3];   /* the point on the aperture, world space */
} lentil_probe_segment;
typedef void (*lentil_probe_fn)(void *user, uint64_t n, const lentil_probe_segment *segments, uint8_t *occluded);
int lentil_hip_set_occlusion_probe(lentil_hip_ctx *ctx, lentil_probe_fn fn, void *user, const float *camera_to_world);
/* stats[0] segments handed to the callback since the context was created, [1] of them answered "occluded", [2] callback calls.
 * Under a device callback (below) segments and occluded answers are counted on the device and read when the call observes the
 * context; [2] counts the callback's calls, and a round enqueued blind calls even when its list turns out empty. */
int lentil_hip_probe_stats(lentil_hip_ctx *ctx, uint64_t stats[3]);

/* Occlusion probes answered on the GPU.  A renderer whose scene lives in device memory needs neither the list's trip over PCIe
 * nor the host waits around it: the segments are written in device memory, the renderer's own kernels answer them there, and
 * the library's apply kernel reads the answers there.  The list is the host form's list, segment for segment; so are the
 * results.
 *   fn(user, hip_stream, capacity, d_n, d_segments, d_occluded)
 *   When and where: on the thread that runs the pass -- the caller of lentil_hip_redistribute, or the call that observes the pass
 *     and finishes it --, once per list.
 *   What it receives: d_n, d_segments and d_occluded are device memory of the context's GPU.  The list has min(*d_n, capacity)
 *     entries.  *d_n is final only once the work already enqueued on hip_stream has run: the callback must not read it on the
 *     host.
 *   What it must do: ENQUEUE its work on hip_stream (a hipStream_t) and return.  hip_stream is the chunk's stream, not necessarily
 *     lentil_hip_stream(ctx): chunks run on streams of their own.  d_occluded[0 .. capacity) is zero on entry; the callback writes
 *     non-zero for an occluded segment.  It must not call into the context.  It may synchronise the stream: legal, and it costs
 *     the overlap.
 *   Errors and switching: a non-zero return fails the pass with LENTIL_ERR_INVALID, the code in the message; the context stays
 *     usable.  Host and device callbacks are mutually exclusive: setting either replaces the other, fn == NULL on either setter
 *     switches probing off.  camera_to_world means what it means for the host setter.
 *   With a device callback the rounds of polynomial optics (abb_chromatic == 0) and of the plain thin lens are enqueued without
 *   any host wait or copy.  Every chunk's lists are made with the capacity of the chunk's result pool, which bounds every round's
 *   list whatever the renderer answers (29 B of list per result slot).  A list that does not fit all the same (LENTIL_PROBE_DEVICE_CAP)
 *   is detected on the device: nothing of that round is accepted, the chunk's draws are redone with every list counted on
 *   the host first (one 4-byte read-back per round; lentil_counters::fallback_chunks, lentil_hip_last_redo_note), and an overflow
 *   the redo cannot cover -- in a later round, after the chunk has accepted draws -- fails the pass with LENTIL_ERR_NOMEM; the
 *   next pass is sized afresh.  Thin lens with abb_chromatic > 0 keeps two 4-byte read-backs per
 *   turn of its loop (the list's length, the occluded count).  A probed pass, host or device, does not stream.
 * probe_device_stats, since the context was created: [0] lists handed to the device callback, [1] host waits the library made
 *   on behalf of probes under a device callback, [2] lists that did not fit their buffers, [3] the longest list so far.
 * lentil_hip_test_sphere_occluder_device (lentil_hip_test_* family): a lentil_probe_device_fn -- one lane per segment, the
 *   analytic sphere test of the tests' CPU occluder (fp32 in, fp64 operations in the same order, no contraction: the same answers
 *   bit for bit).  user: four host floats {cx, cy, cz, r}, read at call time; user == NULL returns 1 and enqueues nothing.
 * LENTIL_PROBE_DEVICE_CAP (read at lentil_hip_create): caps a blind pass's list capacity -- a test hook. */
typedef int (*lentil_probe_device_fn)(void *user, void *hip_stream, uint32_t capacity, const uint32_t *d_n,
                                      const lentil_probe_segment *d_segments, uint8_t *d_occluded);
int lentil_hip_set_occlusion_probe_device(lentil_hip_ctx *ctx, lentil_probe_device_fn fn, void *user, const float *camera_to_world);
int lentil_hip_probe_device_stats(lentil_hip_ctx *ctx, uint64_t stats[4]);
int lentil_hip_test_sphere_occluder_device(void *user, void *hip_stream, uint32_t capacity, const uint32_t *d_n,
                                           const lentil_probe_segment *d_segments, uint8_t *d_occluded);

/* The asynchronous end of a pass (round 6).  lentil_hip_redistribute no longer ends with the host waiting for the device: a
 * streamed pass returns once its kernels are enqueued, and whether it needs more work (buffers that were too small, a draw
 * batch that fell short, a wave that gave up waiting) is found out by the next call that OBSERVES the context -- every entry
 * point except lentil_hip_clear_frame, _bind_visits, _redistribute and _resolve: that call waits for the pass, does what is
 * left and only then proceeds, so lentil_hip_sync, the downloads, _get_counters, _last_timing ... return what they always
 * returned (an error of the pass -- LENTIL_ERR_NOMEM for dropped work -- is reported by that call).  A caller that pipelines
 * frames (clear, redistribute, resolve, clear, ...) keeps the device fed instead: the next frame's clear and scan are
 * enqueued while the pass still runs.  Clearing a frame that nobody has observed abandons its pass: the counters are still read
 * (lentil_hip_pass_totals; they size the next passes), work it still needed is not done, and totals.abandoned_incomplete says
 * so.  The visit columns of a pass must stay valid until the pass has been observed or its frame cleared AND the device has
 * passed it (lentil_hip_sync).  At most two passes are in flight unobserved; a third waits for the oldest.
 * set_async(0): every lentil_hip_redistribute waits for its own end, as before round 6 (also LENTIL_ASYNC_END=0).
 * pass_totals: waits for nothing but the events of passes already observed or abandoned; reset != 0 zeroes the sums afterwards. */
int lentil_hip_set_async(lentil_hip_ctx *ctx, int on);
int lentil_hip_pass_totals(lentil_hip_ctx *ctx, lentil_pass_totals *out, int reset);
int lentil_hip_debug_batch_estimate(lentil_hip_ctx *ctx, uint64_t n, const float *cs_xyz, uint32_t samples, float *out);
int lentil_hip_set_draw_log(lentil_hip_ctx *ctx, uint64_t capacity); /* 0 disables */
int lentil_hip_download_draw_log(lentil_hip_ctx *ctx, lentil_draw_record *out, uint64_t capacity,
                                 uint64_t *n_records);

/* --- forward camera rays in batches ---------------------------------------------------
 * camera_create_ray (src/lentil_camera.cpp:78-125) for n camera samples at once: Camera::trace_ray_fw_po /
 * trace_ray_fw_thinlens (src/lentil.h:283-569) for the ray and, at sx + dsx * 0.001f and sy + dsy * 0.001f, for the two
 * rays its differentials are the finite differences to -- what lentil_host_camera_create_ray (lentil_host.h) computes for
 * one ray on the CPU, operation for operation, one GPU lane per ray.  For a renderer whose camera samples live on the GPU.
 * Uses the context's parameters, the table of set_lens (polynomial optics; the thin lens needs none) and the tables of
 * set_bokeh (bokeh_enable_image); needs no frame and no visits.
 *   in    [n][6]  sx, sy, dsx, dsy, lensx, lensy
 *   out   [n][21] the layout of lentil_host_camera_ray: origin, dir, weight, dOdx, dOdy, dDdx, dDdy.  weight = exposure, or
 *                 0 * exposure when every try of the ray was vignetted (polynomial optics: or a NaN came out)
 *   tries [n]     optional: the vignetted tries of the ray's own trace (what trace_ray_fw_* returns for deriv_ray = 0)
 * xor128 (src/global.h:22-27; the lens sample of a retry): the reference keeps one state per process in function statics.
 * Here ray i owns one, derived from its id = first_ray + i (which must fit 32 bits): w0 = tea8(id, rng_seed),
 * w1 = tea8(id, w0), w2 = tea8(id, w1), w3 = tea8(id, w2) (tea<8>, src/global.h:32-57), the generator's initial constants
 * should all four come out zero -- so a batch does not depend on how it is split into calls.
 * flags: LENTIL_RAYS_DEVICE_POINTERS: in / out / tries are device memory of the context's GPU; the call enqueues its kernel
 * on lentil_hip_stream(ctx) and returns (order it with lentil_hip_sync or the stream).  Without it they are host memory and
 * the call returns when out is filled.  LENTIL_RAYS_NO_DIFFERENTIALS: one trace per ray, the four derivative vectors zero.
 * The call observes the context (a pass in flight is finished first) and takes no part in the streamed passes' turns.
 * LENTIL_ERR_INVALID: no parameters, polynomial optics without a lens, bokeh_enable_image without tables, in or out NULL
 * with n > 0, first_ray + n > 2^32.  n == 0 launches nothing. */
#define LENTIL_RAYS_DEVICE_POINTERS 1u
#define LENTIL_RAYS_NO_DIFFERENTIALS 2u
typedef struct lentil_camera_ray_batch {
  uint64_t n;              /* rays in this call */
  uint64_t first_ray;      /* id of ray 0; ray i has id first_ray + i (must fit 32 bits) */
  const float *in;         /* [n][6]: sx, sy, dsx, dsy, lensx, lensy -- the in[6] of lentil_host_camera_create_ray */
  float *out;              /* [n][21]: layout of lentil_host_camera_ray (origin, dir, weight, dOdx, dOdy, dDdx, dDdy) */
  int32_t *tries;          /* optional [n]: tries of the main trace (what trace_ray_fw_* returns for deriv_ray = 0) */
  double lambda;           /* micrometres, PO only */
  float exposure;
  uint32_t rng_seed;
  uint32_t flags;          /* LENTIL_RAYS_DEVICE_POINTERS: in/out/tries are device memory; LENTIL_RAYS_NO_DIFFERENTIALS */
} lentil_camera_ray_batch;
int lentil_hip_camera_rays(lentil_hip_ctx *ctx, const lentil_camera_ray_batch *batch);
/* What the last lentil_hip_camera_rays call of this context ran: *path 0 the thin lens (or no call yet), 1 the table
 * interpreter, 2 the straight-line kernel of a compiled-in lens, 3 the kernel compiled for the table at run time (once
 * lentil_hip_lens_jit_status reports state 2; until then, and after a failed compilation, the interpreter).  The rays are the
 * same bit for bit whichever ran.  Paths 2 and 3 are taken by a context created with LENTIL_RAYS_COMPILED=1 in the
 * environment; without it, or with LENTIL_RAYS_COMPILED=0, camera rays run path 1 (the default until the compiled kernels'
 * rate has been measured against the interpreter's).  lentil_hip_set_lens_mode(ctx, 1) forces path 1 too. */
int lentil_hip_camera_rays_path(lentil_hip_ctx *ctx, int *path);
/* lentil_hip_camera_rays with a wavelength per ray, for a spectral renderer that draws one per path: ray i is, word for word
 * of its 21 floats and its tries, the ray lentil_hip_camera_rays gives for id first_ray + i with lambda = lambdas[i].
 *   lambdas [n]  micrometres; host or device memory as LENTIL_RAYS_DEVICE_POINTERS says for in / out / tries.  The values are
 *                used as given: there is no range check (a NaN or a wavelength far outside the fit gives what the polynomials
 *                give for it, weight 0 where a NaN comes out).  batch->lambda is ignored.
 * The per-ray xor128 state, the flags and the independence from how a batch is split are lentil_hip_camera_rays' (the split
 * moves lambdas along with in).  Thin lens: the wavelengths are ignored as the scalar one is, lambdas may be NULL, the result
 * is the scalar call's.  Observes the context like the scalar call; takes no part in the streamed passes' turns.
 * LENTIL_ERR_INVALID: where lentil_hip_camera_rays returns it, and for lambdas NULL with polynomial optics and n > 0.
 * n == 0 launches nothing.  lentil_hip_camera_rays_path reports this call too: 0, 1, or 2 (LENTIL_RAYS_COMPILED=1 and a
 * compiled-in lens); a table compiled at run time is served by the interpreter (1) -- there is no spectral run-time kernel. */
int lentil_hip_camera_rays_spectral(lentil_hip_ctx *ctx, const lentil_camera_ray_batch *batch, const double *lambdas);

/* --- scene points traced backward through the lens in batches --------------------------
 * The backward counterpart of lentil_hip_camera_rays: for a camera-space point and a draw number, where on the sensor a draw
 * of the redistribution pass puts it -- for a renderer that keeps its own film (another reconstruction filter, a tiled or
 * spectral film, deep output, light-tracing connections) and wants the library's lens, not its frame.  Uses the context's
 * parameters, the table of set_lens (polynomial optics) and the tables of set_bokeh (bokeh_enable_image); needs no frame and
 * no visits, touches no accumulator, and does not consult an occlusion probe (lentil_hip_trace_points_probed, below, does).
 * Queries: n_points * attempts of them, point-major: query q is point q / attempts, attempt number
 * first_attempt[point] + q % attempts (the reference's total_samples_taken of that draw).  The draws are seeded as the pass
 * seeds them, tea<8>(px * py + px, attempt + tries) with (px, py) the point's source pixel, so query (point, m) is what the
 * pass computes for the m-th attempt of a visit at that point and pixel.
 *   Polynomial optics: target = -cs * 10 in fp64 (src/lentil_filter.cpp:271), Camera::trace_ray_bw_po with
 *     vignetting_retries + 1 tries at seeds attempt + tries (src/lentil.h:573-661), then the sensor -> pixel mapping of
 *     src/lentil_filter.cpp:276-290; operation for operation, fp64.  vignetting_retries < 0: no try is made, every query is
 *     LENTIL_POINT_VIGNETTED.  lambda (micrometres) is the wavelength the polynomials are evaluated at; 0: params.lambda_bw.
 *   Thin lens: the draw of src/lentil_filter.cpp:311-434 at the unshifted focus distance -- what the pass computes for
 *     abb_chromatic == 0.  With abb_chromatic > 0 the points are projected the same way: the per-channel shift of the focus
 *     plane follows the pass's xor128 order, which a batch does not have, and is NOT offered.  One try per attempt
 *     (out_tries 0); lambda is ignored.
 *   out_pixel   the linear pixel ix + iy * xres, or LENTIL_POINT_VIGNETTED (every try failed in the lens), or
 *               LENTIL_POINT_OUTSIDE (through the lens, outside the frame; a NaN coordinate counts as outside)
 *   out_xy      optional: the continuous pixel coordinates before floor (pixel0, pixel1: fp64 for polynomial optics, the thin
 *               lens's fp32 values widened) -- also for LENTIL_POINT_OUTSIDE, so a caller can clip to a window of its own; two
 *               quiet NaNs for LENTIL_POINT_VIGNETTED
 *   out_sensor  optional, polynomial optics: sensor x, y (mm) after sensor_shift; NaNs for LENTIL_POINT_VIGNETTED and for
 *               the thin lens
 *   out_tries   optional: the vignetted tries before the one that got through (all of them for LENTIL_POINT_VIGNETTED)
 * flags: LENTIL_POINTS_DEVICE_POINTERS: every pointer of the batch is device memory of the context's GPU; the call enqueues
 * its kernel on lentil_hip_stream(ctx) and returns (order it with lentil_hip_sync or the stream).  Without it they are host
 * memory and the call returns when the outputs are filled.  A batch's results do not depend on how it is split into calls,
 * by points or by attempts.
 * The call observes the context (a pass in flight is finished first) and takes no part in the streamed passes' turns.
 * LENTIL_ERR_INVALID: no parameters, polynomial optics without a lens, bokeh_enable_image without tables, cs / pixel /
 * out_pixel NULL with n_points > 0, attempts == 0, n_points * attempts >= 2^32, a point whose first_attempt + attempts +
 * max(vignetting_retries, 0) does not fit 32 bits (checked for host pointers; with device pointers it is the caller's duty:
 * the seeds wrap).  n_points == 0 launches nothing. */
#define LENTIL_POINTS_DEVICE_POINTERS 1u
#define LENTIL_POINT_VIGNETTED 0xFFFFFFFFu   /* every try of the attempt failed in the lens (the probed call: or at the probe) */
#define LENTIL_POINT_OUTSIDE   0xFFFFFFFEu   /* got through the lens, landed outside the frame (or NaN) */
typedef struct lentil_point_batch {
  uint64_t n_points;
  uint32_t attempts;             /* K >= 1: attempts per point; query q = point q / K, attempt first_attempt[point] + q % K */
  uint32_t flags;                /* LENTIL_POINTS_DEVICE_POINTERS: every pointer is device memory of the context's GPU */
  const float *cs;               /* [n_points][3] camera space, cm, z < 0 in front: the reference's camera_space_sample_position */
  const uint32_t *pixel;         /* [n_points] px | py << 16: the source pixel whose seed (px * py + px) the draws use */
  const uint32_t *first_attempt; /* optional [n_points]; NULL: 0.  attempt = the reference's total_samples_taken */
  double lambda;                 /* polynomial optics, micrometres; 0: params.lambda_bw */
  uint32_t *out_pixel;           /* [n_points * K] linear pixel (ix + iy * xres) or one of the two codes */
  double *out_xy;                /* optional [n_points * K][2]: continuous pixel coordinates before floor */
  double *out_sensor;            /* optional, polynomial optics only: sensor x, y (mm) after sensor_shift */
  int32_t *out_tries;            /* optional: vignetted tries before the one that got through (thin lens: 0) */
} lentil_point_batch;
int lentil_hip_trace_points(lentil_hip_ctx *ctx, const lentil_point_batch *batch);
/* What the last lentil_hip_trace_points call of this context ran: *path 0 the thin lens (or no call yet), 1 the table
 * interpreter, 2 the straight-line kernel of a compiled-in lens -- the default for the shipped lenses, the polynomials the
 * passes run for them by default too.  A table compiled at run time (lentil_hip_lens_jit_status) is served by the
 * interpreter; lentil_hip_set_lens_mode(ctx, 1) forces the interpreter.  The results are the same bit for bit. */
int lentil_hip_trace_points_path(lentil_hip_ctx *ctx, int *path);
/* lentil_hip_trace_points with a wavelength per point, for a spectral film: all `attempts` queries of point j are, bit for
 * bit in out_pixel, out_xy, out_sensor and out_tries, what lentil_hip_trace_points gives with lambda = lambdas[j].
 *   lambdas [n_points]  micrometres; an entry of 0 means params.lambda_bw, as the scalar field does.  Host or device memory
 *                       as LENTIL_POINTS_DEVICE_POINTERS says for the batch's own pointers.  The values are used as given:
 *                       there is no range check.  batch->lambda is ignored.
 * Thin lens: the wavelengths are ignored as the scalar one is, lambdas may be NULL, the result is the scalar call's.
 * Observes the context like the scalar call; takes no part in the streamed passes' turns.
 * LENTIL_ERR_INVALID: where lentil_hip_trace_points returns it, and for lambdas NULL with polynomial optics and n_points > 0.
 * n_points == 0 launches nothing.  lentil_hip_trace_points_path reports this call too (0, 1 or 2). */
int lentil_hip_trace_points_spectral(lentil_hip_ctx *ctx, const lentil_point_batch *batch, const double *lambdas);
/* lentil_hip_trace_points under the context's occlusion probe (lentil_hip_set_occlusion_probe or _device): query (point, m) is
 * Camera::trace_ray_bw_po as the reference runs it in a scene -- vignetting_retries + 1 tries at seeds m + tries, and a try
 * whose segment, from `origin` to camera_to_world * (-aperture * 0.1 / unit), is occluded fails like one the lens vignettes
 * (src/lentil.h:613-629) -- then the sensor -> pixel mapping.  Thin lens: one try per attempt, the segment goes to
 * camera_to_world * (lens / unit), an occluded attempt is lost (src/lentil_filter.cpp:356-375).  A caller cannot do this with
 * the unprobed call: no call hands out the aperture point, and an occluded try hands the attempt on to the next seed, which
 * lands elsewhere.  The answers agree with the pass and with lentil_hip_list_draws(LENTIL_DRAWS_PROBED) for a visit of that
 * position, source pixel and time.
 *   Outputs: lentil_point_batch's.  out_tries counts occluded tries too; LENTIL_POINT_VIGNETTED reads "every try failed, in the
 *   lens or at the probe"; out_xy and out_sensor are those of the try that got through.  For a query that no occluded seed
 *   touches every output is the unprobed call's, bit for bit; with `exempt` set for every point the whole batch is, and the
 *   callback is never called.
 *   What is asked: only seeds that got through the lens, each (point, seed) at most once per call, and exactly these: (point,
 *   s) is asked if and only if the batch has a query m with m <= s <= m + retries whose seeds in [m, s) all fail, in the lens
 *   or at the probe, and s gets through the lens.  The segments are bit for bit what the probed list writes for a visit with
 *   that position, source pixel and time (camera_to_world: the one given to the setter, or the fp64 inverse; motion keys
 *   blended and clamped at `time` as the pass blends them).
 *   Turns: the batch is traced in turns; every open query asks about its next seed in every turn, so while a turn's list fits
 *   the buffers the callback is called at most max(vignetting_retries, 0) + 1 times (thin lens: once), on the calling thread,
 *   never with an empty list.  lentil_hip_probe_stats and lentil_hip_probe_device_stats grow as for the probed list.
 *   With LENTIL_POINTS_DEVICE_POINTERS every pointer of the batch and of lentil_point_probe is device memory; the call still
 *   returns only when the outputs are final (it waits once per turn).  With lambdas (polynomial optics) point j is traced at
 *   lambdas[j] as lentil_hip_trace_points_spectral traces it and batch->lambda is ignored; the thin lens ignores them.
 * Observes the context like the scalar call; takes no part in the streamed passes' turns; leaves frame, visits, xor128 state
 * and pass counters alone.  lentil_hip_trace_points_path reports this call too.  The thin lens with abb_chromatic > 0 is
 * projected as lentil_hip_trace_points projects it.
 * LENTIL_ERR_INVALID: where lentil_hip_trace_points returns it; no occlusion probe set; probe or probe->origin NULL with
 * n_points > 0; a device callback that returns non-zero (the context stays usable).  LENTIL_ERR_UNSUPPORTED: polynomial
 * optics with abb_chromatic != 0 (the pass and the probed list refuse the pair too).  LENTIL_ERR_NOMEM: an answer store (two
 * bits per seed offset 0 ... attempts + max(vignetting_retries, 0) - 1 of every point) of 2^27 words or more per array, or
 * one that does not fit: split the batch.  n_points == 0 launches nothing. */
typedef struct lentil_point_probe {
  const float   *origin;   /* [n_points][3] world space: the segment's origin, the sample's world position as the renderer holds
                              it (what the visit stream carries in pos_z.xyz).  Required. */
  const float   *time;     /* optional [n_points]: the sample's time, for lentil_hip_set_camera_motion's keys (blended and clamped
                              as the pass blends them); NULL: 0 for every point */
  const uint8_t *exempt;   /* optional [n_points]: non-zero = the skydome supplied the sample (src/lentil_filter.cpp:119-133):
                              nothing of it is occluded, nothing of it is asked */
  const double  *lambdas;  /* optional [n_points], polynomial optics: a wavelength per point, 0 = params.lambda_bw, as
                              lentil_hip_trace_points_spectral takes them; NULL: batch->lambda for all */
} lentil_point_probe;
int lentil_hip_trace_points_probed(lentil_hip_ctx *ctx, const lentil_point_batch *batch, const lentil_point_probe *probe);

/* --- a visit range's plan and its accepted draws, for a renderer with its own film ---------------
 * lentil_hip_trace_points answers where attempt m of a point lands.  These two calls answer what the pass makes of the
 * context's bound visit stream (upload_visits / bind_visits / visits_end), so that a caller never restates the visit prologue
 * (src/lentil_filter.cpp:105-240) or the draw loop's selection (:249-300, :311-447):
 *   plan_visits  per visit, what the prologue decides: whether the visit is redistributed, its camera-space position, its
 *                draw count, fitted_bidir_add_energy and what one contribution of it weighs;
 *   list_draws   per accepted draw of the redistributed visits, the visit, the attempt, the pixel and the continuous
 *                pixel coordinates -- the draw list of the reference's pass, record for record.
 * Both use the context's parameters, the bound visits, the table of set_lens, the tables of set_bokeh, the camera motion keys
 * and the shutter.  A visit's source pixel and inverse density are derived as the pass derives them: from pixel_x0 / pixel_y0 /
 * pixel_row_stride / pixels_per_row and params.inverse_sample_density for a uniform stream, from the pixel and inv_density
 * columns for a ragged one.  Neither needs a frame, touches an accumulator, a cryptomatte table, the counter block
 * (lentil_hip_get_counters) or the xor128 state; plan_visits consults no occlusion probe, list_draws only with
 * LENTIL_DRAWS_PROBED (below).  Both observe the context (a pass in flight is
 * finished first) and take no part in the streamed passes' turns.  Visits are numbered as in the bound stream; a range is
 * [first_visit, first_visit + n_visits), and must lie inside the stream and below 2^32.
 *
 * lentil_hip_plan_visits: one kernel, one record per visit of the range, out[i] for visit first_visit + i.
 *   cs          camera_space_sample_position: world position (or the skydome substitute) through the world-to-camera matrix at
 *               the visit's time, times the unit scale -- what lentil_hip_trace_points takes as cs
 *   add_energy  fitted_bidir_add_energy; 0 for a visit that stays in its pixel (the reference adds none there)
 *   weight      what one contribution of this visit weighs, formed in fp32 as the pass forms it: inv_density for a visit that
 *               stays, 1.0f * inv_density * inv_samples (inv_samples = 1.0 / (float)samples, rounded to fp32) for a
 *               redistributed one
 *   samples     the draw count (src/lentil_filter.cpp:177-202), computed for every visit as upstream computes it
 *   pixel       px | py << 16: the region-relative source pixel (the px, py of the draws' seed)
 *   flags       LENTIL_PLAN_REDISTRIBUTE: the visit is redistributed
 *   totals      optional, host memory: [0] visits in the range, [1] redistributed ones, [2] the sum of their samples -- an
 *               upper bound on what list_draws finds for the same range: size its `out` with it (the chromatic list of
 *               LENTIL_DRAWS_CHANNELS: 11 times it).
 *   flags LENTIL_PLAN_DEVICE_POINTERS: `out` is device memory of the context's GPU.  With it and totals == NULL the call
 *   only enqueues on lentil_hip_stream(ctx); in every other case it returns when out / totals are filled.
 *
 * lentil_hip_list_draws: polynomial optics with abb_chromatic == 0 and the thin lens with abb_chromatic <= 0; polynomial
 * optics with abb_chromatic != 0 under LENTIL_DRAWS_CHANNELS (further down).
 *   A redistributed visit contributes one record for each of the first `samples` attempts n < 5 * samples whose trace is a
 *   pixel -- the attempts the reference's loop accepts before it stops.  The trace of attempt n is
 *   lentil_hip_trace_points' for (plan.cs, plan.pixel, n), the arithmetic is trace_points_kernel's operation for operation:
 *   polynomial optics use vignetting_retries + 1 tries at seeds n + tries (vignetting_retries < 0: no try is made, no
 *   records), the thin lens one try.  lambda: as in lentil_point_batch.
 *   visit / attempt / pixel  equal the draw log of the reference's pass over these visits (lentil_hip_set_draw_log's records)
 *   tries                    the vignetted tries before the one that got through (thin lens: 0)
 *   xy                       the continuous pixel coordinates before floor (trace_points' out_xy)
 *   The order of the records is unspecified.  Their content is not: the list, as a set, does not depend on the grid, on the
 *   capacity or on how a stream is split into visit ranges.
 *   capacity / out   records `out` holds.  *n_draws (host memory, required) is the number of accepted draws found; where it
 *                    exceeds capacity, `capacity` records were written, nothing beyond out[capacity - 1], and the caller asks
 *                    again with more room (the records written are some `capacity` of the list).  n_draws is read back, so
 *                    the call returns when the list is complete -- with LENTIL_DRAWS_DEVICE_POINTERS (`out` is device memory
 *                    of the context's GPU) too.
 *   attempts         optional, host memory: the attempts made -- the reference's attempted_draws for these visits
 *   LENTIL_ERR_UNSUPPORTED, with a message: polynomial optics with abb_chromatic != 0 without LENTIL_DRAWS_CHANNELS (three
 *   traces per attempt under another counting rule: below), the thin lens with abb_chromatic > 0 (the channels follow the
 *   pass's xor128 order; trace_points does not offer it either), with or without that flag.
 *   flags LENTIL_DRAWS_CHANNELS: the caller reads lentil_draw::attempt as n | channel << 30, channel 0, 1, 2 for the
 *   reference's -1, 0, 1 -- as lentil_draw_record::attempt of a pass's draw log carries it.  A caller that does not know of
 *   the channel bits would misread `attempt`, so the chromatic list is given only to one who sets the flag.  For every mode
 *   the plain list serves, the flag changes nothing: the plain list, bit for bit (channel bits 0).
 *     Polynomial optics with abb_chromatic != 0 (src/lentil_filter.cpp:248-299): attempt n traces the three channels of
 *     lentil_hip_draw_channels, each with the seeds n + try, its own vignetting_retries + 1 tries and its own wavelength.
 *     Every channel that gets through the lens and lands in the frame is a record: its `tries`, `xy` and `pixel` are that
 *     channel's own -- lentil_hip_trace_points' for (plan.cs, plan.pixel, n) at the channel's wavelength.  Every channel that
 *     does not takes one off the reference's `count`, the attempt itself adds one: count += successes - 2, a signed count
 *     that may go down.  Attempts are made while count < samples and n < 5 * samples.  So a visit yields up to 11 * samples
 *     records (count + 2 * attempts), and plan_visits' totals[2] no longer bounds the list: 11 * totals[2] does; or ask with
 *     capacity 0 first and size `out` by *n_draws.  *n_draws counts records, *attempts attempts (the reference's
 *     attempted_draws: one per attempt, not one per channel).  abb_chromatic > 0: `lambda` must be 0 (LENTIL_ERR_INVALID
 *     otherwise; the wavelengths are the mode's own), and channel c belongs to colour component c alone (rgb_weight of
 *     lentil_hip_draw_channels).  abb_chromatic < 0: three white channels at `lambda` (0: params.lambda_bw) -- every attempt
 *     that lands gives three records with one pixel.  The channel bits need 5 * samples + vignetting_retries < 2^30, where
 *     `samples` is samples_override, or 2000, the draw count formula's clamp, without one: with set_params' limit on
 *     samples_override (2^24) only a vignetting_retries near 2^30 breaks it; refused with LENTIL_ERR_UNSUPPORTED.
 *     With LENTIL_DRAWS_PROBED as well: LENTIL_ERR_UNSUPPORTED (not built; a pass under a probe refuses this mode too).
 *     Capacity, LENTIL_DRAWS_DEVICE_POINTERS and lentil_hip_list_draws_path are as without the flag.
 *   flags LENTIL_DRAWS_PROBED: the list under the context's occlusion probe (lentil_hip_set_occlusion_probe or
 *   lentil_hip_set_occlusion_probe_device, with its camera_to_world or the fp64 inverse, motion keys included) -- the draw
 *   list of the reference's pass under that probe.  Without the flag a probe is ignored: the unprobed list, bit for bit.
 *   With the flag and no probe the call fails with LENTIL_ERR_INVALID.
 *     Polynomial optics: seed m = attempt + try of a visit is occluded or it is not, whichever attempt looks at it.  An
 *     attempt's outcome is the first seed in attempt ... attempt + vignetting_retries that is neither vignetted nor
 *     occluded; `tries` counts the failed tries before it, vignetted or occluded; xy and pixel are that try's.
 *     Thin lens: an occluded attempt is lost, `tries` stays 0.  Samples the skydome supplied are exempt and never asked about.
 *     The selection is the same: the first `samples` attempts below 5 * samples that land in the frame.  *attempts is the
 *     reference's attempted_draws under the probe.  plan_visits' totals[2] still bounds the list.
 *     What the callback is asked: one segment per (visit, seed) that the reference's walk reaches and that got through the
 *     lens (a vignetted try is never asked about: its answer cannot matter), each at most once per call, each bit-identical
 *     to the segment a pass lists for that try.  (With enable_dof == 0 every seed of a visit has the same aperture point, so
 *     a visit's segments coincide; they are still one per seed.)
 *     Which seeds a visit reaches depends on the answers, so the list is made in turns: the callback may be called several
 *     times per list_draws call, always on the calling thread, with the segments no earlier turn asked about.  It must not
 *     call into the context.  Answers are not kept between calls: a counting call (capacity == 0) followed by the real one
 *     asks twice.  Host callback: segments and answers travel as in a pass.  Device callback: segments and answers stay on
 *     the device, the host reads back each turn's list length (and waits for it); every list is made into buffers that hold
 *     it, so `capacity` as handed to the callback is at least *d_n.  A device callback that returns non-zero fails the call
 *     with LENTIL_ERR_INVALID and the code in the message, as it fails a pass; the context stays usable.
 *     lentil_hip_probe_stats counts these segments, occluded answers and calls too, lentil_hip_probe_device_stats the lists
 *     (and one wait per turn).  The list as a set, and the set of segments asked per visit, do not depend on the grid, on
 *     the capacity or on how the stream is split into ranges.  The call keeps two bits per seed 0 ... 5 * samples +
 *     vignetting_retries of every redistributed visit of the range; LENTIL_ERR_NOMEM, with a message, where that store
 *     does not fit: split the range.  LENTIL_DRAWS_DEVICE_POINTERS combines freely with the flag.
 * LENTIL_ERR_INVALID (both calls): no parameters or no visits, polynomial optics without a lens, bokeh_enable_image without
 * tables (list_draws), a range outside the stream or beyond 2^32, out NULL with n_visits > 0 (plan) or capacity > 0 (list),
 * n_draws NULL.  n_visits == 0 launches nothing (zero totals, zero n_draws).
 * lentil_hip_list_draws_path: what the last list_draws call of this context ran, as lentil_hip_trace_points_path: 0 the thin
 * lens (or no call yet), 1 the table interpreter (also a table compiled at run time, and lentil_hip_set_lens_mode(ctx, 1)),
 * 2 the straight-line kernel of a compiled-in lens.  The lists are the same bit for bit. */
#define LENTIL_PLAN_DEVICE_POINTERS 1u
#define LENTIL_PLAN_REDISTRIBUTE    1u      /* lentil_visit_plan::flags bit 0 */
typedef struct lentil_visit_plan {          /* 32 bytes, one per visit */
  float cs[3];        /* camera space after unit scaling: camera_space_sample_position (what trace_points takes as cs) */
  float add_energy;   /* fitted_bidir_add_energy (0 for a visit that stays in its pixel) */
  float weight;       /* what one contribution of this visit weighs (see above) */
  uint32_t samples;   /* the draw count (computed for every visit, as upstream) */
  uint32_t pixel;     /* px | py << 16, region-relative source pixel (the seed's px, py) */
  uint32_t flags;     /* LENTIL_PLAN_REDISTRIBUTE */
} lentil_visit_plan;
int lentil_hip_plan_visits(lentil_hip_ctx *ctx, uint64_t first_visit, uint64_t n_visits, lentil_visit_plan *out,
                           uint32_t flags, uint64_t totals[3] /* optional: visits, redistributed, sum of their samples */);

#define LENTIL_DRAWS_DEVICE_POINTERS 1u
#define LENTIL_DRAWS_PROBED 2u              /* the list under the context's occlusion probe (see above) */
#define LENTIL_DRAWS_CHANNELS 4u            /* the caller reads lentil_draw::attempt as n | channel << 30 (see above) */
typedef struct lentil_draw {                /* 32 bytes */
  uint32_t visit;     /* index into the bound stream */
  uint32_t attempt;   /* the reference's total_samples_taken of the draw; the chromatic list: | channel << 30 */
  uint32_t pixel;     /* linear pixel ix + iy * xres */
  int32_t  tries;     /* vignetted (LENTIL_DRAWS_PROBED: or occluded) tries before the one that got through (thin lens: 0) */
  double   xy[2];     /* continuous pixel coordinates before floor (trace_points' out_xy) */
} lentil_draw;
typedef struct lentil_draw_list {
  uint64_t first_visit, n_visits;
  uint32_t flags;
  uint64_t capacity;      /* records `out` holds */
  lentil_draw *out;
  double lambda;          /* polynomial optics, micrometres; 0: params.lambda_bw */
  uint64_t *n_draws;      /* host: accepted draws found; > capacity: nothing beyond capacity was written, ask again */
  uint64_t *attempts;     /* optional, host: attempts made (the reference's attempted_draws for these visits) */
} lentil_draw_list;
int lentil_hip_list_draws(lentil_hip_ctx *ctx, const lentil_draw_list *list);
int lentil_hip_list_draws_path(lentil_hip_ctx *ctx, int *path);   /* 0 thin lens / none yet, 1 interpreter, 2 compiled-in lens */
/* lentil_hip_list_draws with a wavelength per visit, for a spectral film: the records of visit v are, bit for bit in visit,
 * attempt, pixel, tries and xy, those that lentil_hip_list_draws gives for the range [v, v + 1) with
 * lambda = lambdas[v - first_visit]; *n_draws and *attempts are the sums over the visits.
 *   lambdas [n_visits]  micrometres; lambdas[i] belongs to visit first_visit + i (the index is relative to the range).  An
 *                       entry of 0 means params.lambda_bw, as the scalar field does.  Host or device memory as
 *                       LENTIL_DRAWS_DEVICE_POINTERS says for `out`.  The values are used as given: there is no range check.
 *                       list->lambda is ignored.
 * Everything else is the scalar call's: capacity and the counting call, the unspecified order of the records, the independence
 * of the list as a set from the grid, the capacity and the split into ranges, and lentil_hip_list_draws_path, which reports
 * this call too.
 * LENTIL_DRAWS_PROBED, with a host or a device callback: the list of the reference's pass under the probe with each visit at
 * its own wavelength.  The turns, the answer store, the statistics and the promises about segments are the scalar probed
 * list's: one segment per (visit, seed) that the walk reaches and that got through the lens, at most once per call.  A
 * segment does not depend on the wavelength; which seeds get through the lens does.
 * Thin lens: the wavelengths are ignored as the scalar one is, lambdas may be NULL, the result is the scalar call's.
 * LENTIL_DRAWS_CHANNELS follows the scalar call: where the plain list serves the mode, the flag changes nothing.  Polynomial
 * optics with abb_chromatic != 0 are refused here with LENTIL_ERR_UNSUPPORTED and a message, with or without the flag: the
 * three channels are RGB, each at a wavelength of the mode's own, which a spectral film has no use for.
 * LENTIL_ERR_INVALID: where lentil_hip_list_draws returns it, and for lambdas NULL with polynomial optics and n_visits > 0.
 * n_visits == 0 launches nothing. */
int lentil_hip_list_draws_spectral(lentil_hip_ctx *ctx, const lentil_draw_list *list, const double *lambdas);
/* A wavelength per visit in the pass itself, for a spectral renderer that lets the library keep the film: with a column set,
 * lentil_hip_redistribute over polynomial optics is the reference's pass with lambda_per_sample (src/lentil_filter.cpp:254) =
 * lambdas[v] for visit v -- the accepted-draw list bit for bit, accumulators, weights and the resolved image at the pass's
 * usual bar -- with any AOV kinds, cryptomatte, an occlusion probe (host or device callback) and a communicator.
 *   lambdas [n]  micrometres; lambdas[v] belongs to visit v of the context's stream.  An entry of 0 means params.lambda_bw.
 *                The values are used as given: there is no range check.  Host memory: copied into device memory of the
 *                library's before the call returns.  LENTIL_LAMBDAS_DEVICE_POINTER: the column is bound; the caller keeps it
 *                alive and unchanged while a pass runs.
 *   lambdas NULL switches the column off: the next pass is the pass without one in every respect.
 * The column belongs to the stream that was current when it was set.  lentil_hip_upload_visits, lentil_hip_bind_visits and
 * lentil_hip_visits_end make it stale, and the pass then returns LENTIL_ERR_INVALID until the column is set again or switched
 * off; so does a column of n wavelengths over a stream of another number of visits (the message names both).
 * Such a pass runs in the chunked, round-by-round form (lentil_counters::streamed is 0), its solves in solve_po_spectral_kernel:
 * a wave takes 64 consecutive seeds of one visit at a time, at that visit's wavelength.  A table compiled at run time is served
 * by the interpreter in it; passes without a column keep their run-time kernel.
 * Polynomial optics with abb_chromatic != 0: LENTIL_ERR_UNSUPPORTED from the pass, as lentil_hip_list_draws_spectral refuses.
 * Thin lens: the column's length is checked, the wavelengths are not read; the pass is the pass without a column, and the
 * statistics below do not count it.  lentil_hip_plan_visits, lentil_hip_list_draws*, lentil_hip_trace_points* and
 * lentil_hip_camera_rays* do not look at the column.
 * lentil_hip_spectral_pass_stats: [0] passes run with a column (polynomial optics) since the context was created, [1] the
 * solve tasks the spectral kernel took in them, [2] the lens path of the last such pass in lentil_hip_list_draws_path's
 * encoding (1 interpreter, 2 compiled-in lens, 0 none yet), [3] 0. */
#define LENTIL_LAMBDAS_DEVICE_POINTER 1u
int lentil_hip_set_visit_lambdas(lentil_hip_ctx *ctx, const double *lambdas, uint64_t n, uint32_t flags);
int lentil_hip_spectral_pass_stats(lentil_hip_ctx *ctx, uint64_t stats[4]);
/* The colour channels the draw loop of these parameters traces per attempt (src/lentil_filter.cpp:254-268); needs no context
 * and no GPU.  *n_channels: 3 for polynomial optics with abb_chromatic != 0, else 1 (the thin lens with abb_chromatic > 0
 * picks a channel per attempt from xor128: not described here).  lambda[c]: the channel's wavelength in micrometres, the
 * fp32 arithmetic of the reference widened to double -- abb_chromatic > 0: lerp(1 - c, 0.35, 0.55), 0.55, lerp(c, 0.55, 0.85);
 * otherwise params.lambda_bw throughout (all three entries are always filled).  rgb_weight[c][k] (optional): what a draw of
 * channel c adds to colour component k, as a factor -- {3,0,0}, {0,3,0}, {0,0,3} for abb_chromatic > 0, else 1 everywhere;
 * alpha and the weight always take 1.  The pass and the chromatic list take their channels from this very function. */
int lentil_hip_draw_channels(const lentil_params *p, uint32_t *n_channels, double lambda[3], float rgb_weight[3][3]);

/* --- single-function device tests (parity of the optics primitives) -----------------
 * Runs n independent evaluations on the GPU; host pointers in/out.
 * lt_sample_aperture: Camera::lens_lt_sample_aperture (src/lentil.h:1296-1313) for
 *    scene[n][3], ap[n][2] -> sensor[n][5], out[n][5], transmittance[n]
 * trace_bw_po: Camera::trace_ray_bw_po (src/lentil.h:573-661) for target[n][3]
 *    (already -P_cs*10), px[n], py[n], attempt[n] -> sensor_xy[n][2], ok[n]
 * aperture_sample: the aperture draw of trace_ray_bw_po (src/lentil.h:596-609) for
 *    seed pairs (a[n] = px*py+px, b[n] = total_samples_taken+tries) -> xy[n][2]
 * y0_intersection: Camera::camera_get_y0_intersection_distance (src/lentil.h:1361-1386) for
 *    sensor_shift[n] -> distance[n], and what lens_pt_sample_aperture / lens_evaluate (:1257-1291)
 *    left on the way: sensor[n][5] (x, y, dx, dy, lambda), out[n][5] (x, y, dx, dy, transmittance);
 *    sensor / out may be NULL */
int lentil_hip_test_y0_intersection(lentil_hip_ctx *ctx, uint64_t n, const double *sensor_shift, double lambda,
                                    double *distance, double *sensor, double *out);
int lentil_hip_test_lt_sample_aperture(lentil_hip_ctx *ctx, uint64_t n, const double *scene,
                                       const double *ap, double lambda, double *sensor,
                                       double *out, double *transmittance);
int lentil_hip_test_trace_bw_po(lentil_hip_ctx *ctx, uint64_t n, const double *target,
                                const int32_t *px, const int32_t *py, const int32_t *attempt,
                                double *sensor_xy, int32_t *ok);
int lentil_hip_test_aperture_sample(lentil_hip_ctx *ctx, uint64_t n, const uint32_t *a,
                                    const uint32_t *b, double *xy);
/* Test hook: xor128 (src/global.h:22-27) advanced by k outputs with the jump-ahead the parallel thin-lens walk uses
 * (products with T^(2^j), the generator's step matrix over GF(2)^128), run by one wave on the current device. */
int lentil_hip_test_xor128_jump(const uint32_t in[4], uint64_t k, uint32_t out[4]);
/* Test hook, needs no GPU.  The scan decides `get_coc_thinlens(z) < 0.4` (src/lentil.h:674-692,
 * src/lentil_filter.cpp:185-190) from the camera-space depth alone wherever that is certain; this returns the
 * intervals it would use for `params`: out[0..1] / out[2..3] lower / upper ends of the (at most two) closed depth
 * intervals on which the circle of confusion is certainly below 0.4, out[4..5] / out[6..7] those outside of which it is
 * certainly not (an interval with lower > upper end is empty).  In between the kernel evaluates the function. */
int lentil_hip_debug_scan_bands(const lentil_params *params, float out[8]);
/* Test hook, needs no GPU.  scan_dma2_kernel runs a tile with only the depth column in its ring wherever the depth decides
 * (the lean body) or with all three decision columns (the full body): out[0] the lean ring's slots, out[1] the open groups
 * that make a tile busy (a wave goes to the full body after a busy tile), out[2] the tiles in a row that are not busy before
 * it returns to the lean body. */
int lentil_hip_debug_scan_lean_counts(uint32_t out[3]);
/* Test hook.  The scan kernels a pass may start with; which one runs follows from the stream's shape (visits per pixel, extra
 * AOV columns and their filters, whether the last pixel is whole, pixels per row) and from the LDS the resident solve blocks
 * of a streamed pass leave. */
enum {
  LENTIL_SCAN_DMA2 = 1,          /* beauty only, whole pixels, rows of >= 2 pixels: 64-pixel tiles pipelined through LDS */
  LENTIL_SCAN_DMA = 2,           /* ... its unpipelined form: one visit per pixel, one pixel per row, or no LDS for the other */
  LENTIL_SCAN_DMA_MULTI = 3,     /* extra AOVs, all gaussian, whole pixels of <= 64 visits: groups of <= 64 / M pixels */
  LENTIL_SCAN_UNIFORM = 4,       /* register-staged, one column at a time: what the three above do not take */
  LENTIL_SCAN_UNIFORM_MULTI = 5, /* register-staged, all columns: extras with a closest-filtered AOV or a truncated last pixel */
  LENTIL_SCAN_RUNS = 6,          /* visits_per_pixel == 0: runs of a pixel's visits summed in their order */
  LENTIL_SCAN_RAGGED = 7         /* visits_per_pixel == 0, LENTIL_SCAN_RUNS=0: an atomic per visit and float */
};
/* the scan launch of the last pass (of its last chunk, where the pass ran in chunks): out[0] kernel (LENTIL_SCAN_*), out[1]
 * pixels per tile/group (0 for the two ragged kernels), out[2] dynamic LDS bytes, out[3] blocks launched.  All zero before
 * the first pass.  No effect on the pass. */
int lentil_hip_debug_last_scan(lentil_hip_ctx *ctx, uint32_t out[4]);
/* Test hook.  The kernels that replay, after a pass, the cryptomatte adds of the visits that stay in their own pixel; which
 * one runs follows from the stream's shape and from the LDS a tile needs. */
enum {
  LENTIL_CRYPTO_DIRECT_ATOMIC = 1, /* any stream (ragged, or a last pixel short of visits): a lane per visit, atomics */
  LENTIL_CRYPTO_DIRECT_OWNER = 2,  /* whole pixels: a lane per pixel walks its visits in stream order, no atomics */
  LENTIL_CRYPTO_DIRECT_TILE = 3    /* ... its tiled form, 128 pixels per block through LDS, where a tile fits 64 KiB */
};
/* the own-pixel cryptomatte kernel of the last pass: out[0] kernel (LENTIL_CRYPTO_DIRECT_*; 0 none), out[1] for the tile
 * kernel its variant (0 the tables are read, added to and written; 1 they hold nothing yet and are only written; 2 the wipe
 * was put off and every line is written whole), 0 otherwise, out[2] blocks launched, out[3] bit 0: the redistributed-visit
 * flags came from the pass's work lists, bit 1: a wipe that had been put off was flushed in this call.  All zero before the
 * first pass with cryptomatte AOVs.  No effect on the pass. */
int lentil_hip_debug_last_crypto(lentil_hip_ctx *ctx, uint32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* LENTIL_HIP_H */
