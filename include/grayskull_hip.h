/*
 * include/grayskull_hip.h -- device-resident / batched entry points of
 * libgrayskull_hip.so (MI355X, gfx950).  Plain C ABI: pointers and sizes only.
 *
 * The reference API (grayskull.h) is one image per call on caller-owned host
 * memory.  A 4K frame is ~2 us of HBM traffic, the same as one kernel boundary, so
 * throughput needs (a) images that already live in HBM and (b) many frames per
 * launch.  The gsh_* functions are that: every pointer is a DEVICE pointer, a
 * batch is `n` frames of w*h bytes laid out back to back, calls are enqueued on
 * the calling thread's stream and return immediately (no host sync) unless noted.
 *
 * Each batch function computes, per frame, exactly what the cited reference
 * function computes (bit-exact; tests/ compare against the oracle).
 */
#ifndef GRAYSKULL_HIP_H
#define GRAYSKULL_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "grayskull.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- runtime ------------------------------------------------------------------- */
const char *gsh_version(void);
int gsh_device_count(void);               /* 0 when no GPU is visible                 */
void gsh_set_device(int ordinal);         /* per calling thread; default device 0      */
/* gsh_set_stream selects the stream the calling thread's next calls are enqueued on (NULL => the library's own
 * per-thread one).  The device scratch, the cascade / table caches and the internal side stream belong to the THREAD,
 * not to the stream, so a switch orders the newly selected stream behind everything the thread has enqueued on the
 * previous one: leaving the library's own stream synchronises the host with it and destroys it; leaving a caller's
 * stream -- for another caller's stream or for NULL -- records an event on the stream left and makes the stream entered
 * wait for it on the device (no host sync).  The caller guarantees that (a) the previous stream still exists when
 * gsh_set_stream is called (destroy it after the switch, not before), (b) one thread's calls are issued from that
 * thread only, and (c) work of its own that it enqueues on a stream it has switched away from is ordered against the
 * library's later calls by its own means: the library orders only what went through it. */
void gsh_set_stream(void *hip_stream);
void *gsh_get_stream(void);
void gsh_set_async(int on);               /* drop-in gs_* calls on device pointers skip
                                             the final stream sync when on             */
void gsh_sync(void);                      /* hipStreamSynchronize(current stream)       */
/* ---- launch tuning.  gsh_tune(key, value) sets one entry of a PROCESS-WIDE table of launch heuristics (every entry an
 * atomic; nothing in a product path writes them): measurement scripts and the test-suite use it to force the paths a
 * heuristic would not take on a given input.  RESULTS NEVER DEPEND ON ANY KEY.  (The two probes that did change results --
 * the cascade without rect emission, gs_sobel without its column reads -- exist only in builds with -DGS_EXPERIMENT, see
 * below.)  0 is every key's default.  A RETIRED key or value forced a path that has since been removed; gsh_tune ignores it
 * (one line on stderr), and its number is never reused: the logs under profiles/ cite it. */
enum gsh_tune_key {
  GSH_TUNE_STRIP_BAND_ROWS = 0,   /* rows per band of the strip kernels (0 = auto) */
  GSH_TUNE_STRIP_BLOCK_SHAPE = 1, /* 0: by frame width (default), 1: 64x4, 2: 128x2, 3: 256x1 */
  GSH_TUNE_RETIRED_2 = 2,         /* retired */
  GSH_TUNE_RETIRED_3 = 3,         /* retired (gsh_edge_pipeline_batch forced onto the separate per-call kernels) */
  GSH_TUNE_LBP_PHASE_PRESET = 4,  /* k_lbp_cascade: preset of the stages at which a block re-packs survivors (1: never; >= 1000: custom split) */
  GSH_TUNE_PIPELINE_CHUNK = 5,    /* frames per chunk of gsh_edge_pipeline_batch's internal overlap (0 = 32, negative = never split) */
  GSH_TUNE_COMPARE = 6,           /* 3 integral-image route for gs_blur(r > 3) / gs_adaptive_threshold, 4 the any-radius box kernel also for
                                     radii <= 16, 7 k_box_edge always on the side stream, 8 gs_integral without the streaming loads of
                                     batches beyond the Infinity Cache (1, 2, 5, 6 retired) */
  GSH_TUNE_FAST_SCORE = 7,        /* 0: k_fast_score_q4 (LDS tile, candidates queued), 2: k_fast_score_px (one global byte load per ring pixel) */
  GSH_TUNE_FRAMES_PER_LAUNCH = 8, /* test hook for the batch splitting of every launcher */
  GSH_TUNE_LBP_ADAPTIVE = 9,      /* k_lbp_cascade: max stages + 16 * tenths [+ later points] of the first re-packing point */
  GSH_TUNE_RETIRED_10 = 10,       /* retired (gs_histogram's trips per block, block size and load policy) */
  GSH_TUNE_HIST_BLOCKS = 11,      /* blocks per frame of gs_histogram (test hook: several blocks on small frames) */
  GSH_TUNE_HIST_PIECE = 12,       /* bytes per histogram piece (test hook for images above 1 GiB) */
  GSH_TUNE_LBP_XCD = 13,          /* chunk / tile -> XCD mapping of the LBP kernels: 1 dispatch order, 2 XCD-aware always (0: k_lbp_cascade
                                     by table size, k_lbp_tile in dispatch order; >= 3 retired) */
  GSH_TUNE_LBP_KERNEL = 14,       /* 0: per scale by rule (k_lbp_tile with the tile shape the scale's LDS footprint allows, else
                                     k_lbp_cascade), 1: k_lbp_cascade for every scale, 2 + i: tile shape i (0..2) of k_lbp_tile wherever
                                     it fits (-1, 5, 6 retired) */
  GSH_TUNE_LBP_TILE_SWITCH = 15,  /* k_lbp_tile: first + 16 * tenths -- dense stages [0, first), then while more than tenths/10 of a
                                     wave's windows live, then one lane per (window, classifier) pair */
  GSH_TUNE_EXPERIMENT_16 = 16,    /* GS_EXPERIMENT builds only: gs_lbp_detect runs its kernels but emits nothing */
  GSH_TUNE_RETIRED_17 = 17,       /* retired (k_lbp_cascade's one lane per re-packed window) */
  GSH_TUNE_STRIP_XCD = 18,        /* band -> XCD mapping of the strip kernels / tile -> XCD mapping of the gs_fast score pass: 1 dispatch
                                     order, 2 XCD-aware always */
  GSH_TUNE_FAST_NMS = 19,         /* 0: k_fast_nms_sparse behind the score kernel's bitmap, 1: k_fast_nms item by item */
  GSH_TUNE_TMATCH = 20,           /* 1: gs_match_template on the VALU dot-product kernels; 2 / 3: matrix-core kernel with 64 x 128 / 32 x 64
                                     tiles whatever the image size; 4 / 5: window sums of squares always by passes / always from the table */
  GSH_TUNE_RETIRED_21 = 21,       /* retired (round 3's rule for the strip kernels) */
  GSH_TUNE_EXPERIMENT_22 = 22,    /* GS_EXPERIMENT builds only: gs_sobel without the reads that preserve columns 0 / w-1 */
  GSH_TUNE_EXPERIMENT_23 = 23,    /* GS_EXPERIMENT builds only: the strip-copy probe keeps the stencils' halo load */
  GSH_TUNE_RETIRED_24 = 24,       /* retired (realigning strip flavour never / always) */
  GSH_TUNE_GEOM_FORM = 25,        /* the resize kernels: 1 gather every tap from global memory (no LDS staging), 2 stage the source
                                     rectangle wherever it fits the LDS, also beyond four source pixels per result pixel */
  GSH_TUNE_TMATCH_CHUNK = 26,     /* most frames per chunk of the template-matching batch entries (0 = by their scratch budget; test
                                     hook: a chunk boundary with three small frames) */
  GSH_TUNE_TMATCH_BANK = 27,      /* gsh_match_templates_batch / gsh_locate_templates_batch: 0 by rule, 1 always the loop over the
                                     templates, 2 the bank kernel wherever it is valid; results never depend on it */
  GSH_TUNE_PIPELINE_CODES = 28    /* gsh_edge_pipeline_batch, the chunks after the first of a call that is cut into chunks (radius 2):
                                     0 by rule -- 4-bit edge codes around a guess of each frame's Otsu threshold, taken from the
                                     frame at the same place two chunks back (chunk 1: one back), expanded by a second pass; a
                                     frame whose guess missed is redone exactly --, -1 never (every chunk writes edge bytes and
                                     thresholds them in place), -2 / -3 the guess from two chunks / one chunk back, v >= 1 every
                                     guess forced to v - 1 (test hook: window edges and misses on small inputs); results never
                                     depend on it */
};
void gsh_tune(int key, int value);
/* measurement aid for bench.py: while on, gsh_edge_pipeline_batch brackets every launch of its
 * fused blur+sobel+histogram kernel with HIP events on the stream it is launched on (up to 4096
 * launches between reads; on > 1 pre-creates that many event pairs so none is created inside a
 * timed region); gsh_profile_read synchronises, returns how many launches were bracketed since
 * the last read and their summed duration in milliseconds. */
void gsh_profile(int on);
unsigned gsh_profile_read(double *total_ms);
#ifdef GS_EXPERIMENT
/* Experiment builds only (make experiment -> build_variants/libgs_experiment.so; the release library does not export it):
 * strip-kernel traffic pattern with no arithmetic (access-pattern ceiling).  The same builds honour the result-changing
 * keys 16 / 22 / 23 and the compile-time hooks GS_FUSED_SPARE, GS_FUSED_VGPR_ATTR, GS_EVENT_FLAGS, GS_ORDER_EVENT_FLAGS,
 * GS_LOAD_AUX, GS_STORE_AUX, GS_LBP_PREFETCH, GS_MAD2_OPAQUE, GS_LBP_TILE_ODD_STRIDE. */
void gsh_probe_strip_copy(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h, unsigned n);
#endif
void gsh_shutdown(void);                  /* free this thread's scratch + stream        */

void *gsh_malloc(size_t bytes);           /* hipMalloc; aborts on failure               */
void gsh_free(void *dev);
/* page-locked host memory (hipHostMalloc): gsh_upload / gsh_download and host-pointer gs_* calls
 * on it move at the full PCIe rate without the driver's pageable staging copy; aborts on failure */
void *gsh_host_alloc(size_t bytes);
void gsh_host_free(void *host);
void gsh_memset(void *dev, int byte, size_t bytes);             /* stream-ordered      */
void gsh_upload(void *dev, const void *host, size_t bytes);     /* synchronous         */
void gsh_download(void *host, const void *dev, size_t bytes);   /* synchronous         */
int gsh_is_device_ptr(const void *p);

/* ---- stencils over a batch (ref grayskull.h:268, :306, :303-304) ----------------- */
void gsh_blur_batch(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h, unsigned n,
                    unsigned radius);
void gsh_sobel_batch(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h, unsigned n);
void gsh_erode_batch(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h, unsigned n);
void gsh_dilate_batch(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h, unsigned n);
/* `iterations` applications of gs_erode (dilate = 0) or gs_dilate (dilate != 0) to each of n frames, equal bit for bit to
 * calling the 3x3 operator that many times (ref grayskull.h:286-304; nanomagick.c:110-135).  Runs ceil(iterations / 4)
 * passes.  tmp: n*w*h bytes, used when more than one pass is needed; NULL = the library's own grow-only scratch
 * (growing it synchronises once).  dst, src, tmp must not overlap; src is never written.  Stream-ordered. */
void gsh_morph_batch(uint8_t *dst, const uint8_t *src, uint8_t *tmp, unsigned w, unsigned h, unsigned n,
                     int dilate, unsigned iterations);

/* ---- histogram / otsu / threshold (ref :199, :205, :225) ------------------------- */
/* hist: n x 256 u32 (device).  thr: n x u8 (device). */
void gsh_histogram_batch(const uint8_t *img, unsigned w, unsigned h, unsigned n, unsigned *hist);
void gsh_otsu_batch(const uint8_t *img, unsigned w, unsigned h, unsigned n, unsigned *hist_scratch,
                    uint8_t *thr);
void gsh_threshold_batch(uint8_t *img, unsigned w, unsigned h, unsigned n, uint8_t thresh);
void gsh_threshold_batch_dev(uint8_t *img, unsigned w, unsigned h, unsigned n, const uint8_t *thr);
/* frame f thresholded at (uint8_t)(thr[f] + offset) -- the conversion C performs for gs_threshold(img,
 * gs_otsu_threshold(img) + 10) (ref nanomagick.c:191): Otsu 250 + 10 thresholds at 4.  thr is not modified. */
void gsh_threshold_batch_dev_offset(uint8_t *img, unsigned w, unsigned h, unsigned n, const uint8_t *thr,
                                    int offset);

/* gs_blur(src, radius) followed by gs_sobel into a zeroed dst, per frame, in one pass over the frame
 * for radius 1..3 (the blurred image stays in registers; ref :268, :306) */
void gsh_blur_sobel_batch(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h, unsigned n,
                          unsigned radius);

/* config-2 chain per frame: blur(radius) -> sobel (dst frame pre-zeroed) -> otsu -> threshold.
 * dst: n*w*h bytes, thr: the n Otsu thresholds.  tmp: n*w*h bytes that receive the blurred
 * frames, or NULL when the caller does not need them -- then blur, sobel and the histogram run
 * as ONE fused kernel and the blurred image never touches memory (same dst / thr bytes). */
void gsh_edge_pipeline_batch(uint8_t *dst, uint8_t *tmp, const uint8_t *src, unsigned w, unsigned h,
                             unsigned n, unsigned radius, unsigned *hist_scratch, uint8_t *thr);

/* ---- integral image + LBP cascade (ref :744, :815) ------------------------------- */
/* ii: n frames of w*h u32, same unpadded layout as the reference. */
void gsh_integral_batch(const uint8_t *src, unsigned w, unsigned h, unsigned n, unsigned *ii);

/* Cascade tables are flattened once into device memory. `c` points at HOST tables. */
typedef struct gsh_cascade gsh_cascade;
gsh_cascade *gsh_cascade_create(const struct gs_lbp_cascade *c);
void gsh_cascade_destroy(gsh_cascade *dc);

/* Per frame f: rects[f*max_rects ...] gets the first min(count,max_rects) detections in the
 * reference's (scale, y, x) order, counts[f] that number.  ii as produced by gsh_integral_batch.
 * rects/counts are device pointers; records at and beyond counts[f] are not written.  Stream-ordered. */
void gsh_lbp_detect_batch(const gsh_cascade *dc, const unsigned *ii, unsigned iw, unsigned ih,
                          unsigned n, struct gs_rect *rects, unsigned *counts, unsigned max_rects,
                          float scale_factor, float min_scale, float max_scale, int step);
/* Measurement aid: while `counter_dev` (FOUR device u64, caller-zeroed) is set, every cascade launch
 * of this thread adds [0] the number of windows it really evaluated -- chunks skipped because
 * max_rects detections precede them in scan order (ref :819-823) are not counted --, [1] the
 * number of weak classifiers evaluated, summed over windows (every window pays the classifiers of the stages
 * it enters, like the reference), [2] the dword table loads the kernels issued, summed over lanes, [3] nothing
 * any more (round 3's stage prefilter counted its windows here; the buffer keeps four entries so that callers of
 * either round stay inside their allocation).  NULL = off (the default kernels). */
void gsh_lbp_count_evaluated(unsigned long long *counter_dev);
/* number of windows gs_lbp_detect visits for this geometry (for Mwin/s reporting) */
uint64_t gsh_lbp_window_count(const struct gs_lbp_cascade *c, unsigned iw, unsigned ih,
                              float scale_factor, float min_scale, float max_scale, int step);

/* ---- FAST / ORB / matching (ref :482, :651, :680) -------------------------------- */
/* pass 1 of gs_fast alone (ref :487-513): the FAST-9 score map of n frames (interior pixels; the 3-px frame is not written,
 * ref :489); w, h >= 7 */
void gsh_fast_score_batch(uint8_t *score, const uint8_t *img, unsigned w, unsigned h, unsigned n, unsigned threshold);
/* kps: n*nkps records (device), counts: n (device).  scoremap: n frames; only the interior is
 * written, the 3-px frame is read by the NMS exactly like the reference does.  Frame f's first counts[f] records are
 * written whole (angle and descriptor as 0, ref :530), the records at and beyond counts[f] are not written. */
void gsh_fast_batch(const uint8_t *img, uint8_t *scoremap, unsigned w, unsigned h, unsigned n,
                    struct gs_keypoint *kps, unsigned *counts, unsigned nkps, unsigned threshold);

/* Device image -> HOST keypoints.  Synchronous (orientation uses the host libm, like the
 * reference: grayskull.h:100-101).  Returns the number of keypoints written; the records behind them are not written. */
unsigned gsh_orb_extract(const uint8_t *img_dev, unsigned w, unsigned h, uint8_t *scoremap_dev,
                         struct gs_keypoint *kps_host, unsigned nkps, unsigned threshold);

/* gs_orb_extract for n frames of one size (frames w*h bytes apart): frame f's keypoints go to
 * kps_host[f*nkps ...], their number to counts_host[f].  scoremap_dev: n frames, same role as in
 * gsh_fast_batch.  Two host round trips for the whole batch.  Synchronous.  Records at and beyond counts_host[f] are
 * not written. */
void gsh_orb_extract_batch(const uint8_t *img_dev, unsigned w, unsigned h, unsigned n,
                           uint8_t *scoremap_dev, struct gs_keypoint *kps_host, unsigned *counts_host,
                           unsigned nkps, unsigned threshold);
/* gs_orb_extract for n device frames with NO host round trip: the selection (stable sort by response,
 * border filter, cap) and the trig run on the device.  The trig is the reference's GS_NO_STDLIB pair
 * (ref :70-88, the polynomials its wasm build uses), so results equal the reference header compiled
 * with -DGS_NO_STDLIB bit for bit -- angles and descriptors differ from the libm build's, like the
 * reference's own two builds differ.  kps_dev: n x nkps records, counts_dev: n; stream-ordered.  Records at and beyond
 * counts_dev[f] are not written. */
void gsh_orb_extract_batch_nostdlib(const uint8_t *img_dev, unsigned w, unsigned h, unsigned n,
                                    uint8_t *scoremap_dev, struct gs_keypoint *kps_dev, unsigned *counts_dev,
                                    unsigned nkps, unsigned threshold);

/* The reference's ORB caller (examples/nanomagick/nanomagick.c:245-290, extract_pyramid_orb_nm) with
 * every pyramid level resident on the device: up to 4 levels, each gs_downsample (ref :189) of the
 * previous, stopping before a level narrower or lower than 32; nkps / n_levels keypoints per level
 * (the last level takes the remainder); coordinates scaled back by 2^level.  buffer_dev has the
 * reference's layout -- levels 1.. back to back, then one scoremap per level -- and its bytes are
 * the caller's (the NMS reads the never-written 3-px scoremap frames, ref :524).  Synchronous.  Returns the number of
 * keypoints written to kps_host; the records behind them are not written. */
size_t gsh_orb_pyramid_buffer_bytes(unsigned w, unsigned h, unsigned n_levels);
unsigned gsh_orb_extract_pyramid(const uint8_t *img_dev, unsigned w, unsigned h, uint8_t *buffer_dev,
                                 struct gs_keypoint *kps_host, unsigned nkps, unsigned threshold,
                                 unsigned n_levels);

/* ---- pyramid ORB over a batch (docs/design/detectors.md "Pyramid ORB over a batch") ----------------------------------
 * levels 1 .. L-1 of n frames, L as the ORB driver counts it (n_levels clamped to 4, stop before a level narrower or
 * lower than 32): plane l holds n frames of lw[l] x lh[l] back to back, planes back to back in level order.  Frame f
 * of plane l is gs_downsample applied l times to frame f, byte for byte.  ONE launch per kMaxZ frames
 * (GSH_TUNE_FRAMES_PER_LAUNCH).  L <= 1 writes nothing.  Device pointers at any alignment, stream-ordered; n == 0
 * returns before any check or launch; GS_ASSERT: non-NULL levels_dev and img_dev, w and h non-zero. */
void gsh_pyramid_batch(uint8_t *levels_dev, const uint8_t *img_dev, unsigned w, unsigned h, unsigned n, unsigned n_levels);

size_t gsh_orb_pyramid_batch_buffer_bytes(unsigned w, unsigned h, unsigned n_levels, unsigned n);  /* = n * gsh_orb_pyramid_buffer_bytes */

/* extract_pyramid_orb_nm (examples/nanomagick/nanomagick.c:245-290) of a reference built -DGS_NO_STDLIB for n frames of
 * one size.  All pointers device pointers, stream-ordered on the current stream, no host synchronisation and no read-back
 * (the grow-only scratch may synchronise once when it grows).  n == 0 returns before any check or launch.  GS_ASSERT:
 * non-NULL img_dev, buffer_dev, kps_dev, counts_dev; w and h non-zero.
 * buffer_dev: gsh_orb_pyramid_batch_buffer_bytes bytes in gsh_orb_extract_pyramid's layout with every plane replaced by
 * n planes, level-major: the level planes 1 .. L-1 as gsh_pyramid_batch writes them, then the score-map planes 0 .. L-1 of
 * n frames each (n == 1: the single-frame layout).  The score maps' bytes are the caller's: only their interior is written,
 * the 3-px frames are read by the NMS (ref :524) and never written.
 * Frame f's result is what extract_pyramid_orb_nm(frame f, kps, nkps, threshold, buf_f, n_levels) returns and writes, buf_f
 * being frame f's planes laid out as one buffer: per = nkps / L keypoints from each level l < L-1 (skipped, score maps
 * untouched, when per == 0), nkps - (what the earlier levels of THIS frame produced) from the last; each level is
 * gs_orb_extract of the level's image with that quota (FAST cap min(4 * quota, 5000)), coordinates shifted left by the
 * level.  The records lie back to back in level order at kps_dev + f * nkps, counts_dev[f] is their number, records at and
 * beyond it are not written.  level_counts_dev (n x 4, may be NULL): level l's share at [4 * f + l]; all four words are
 * written, 0 for levels not run.  n_levels == 0, nkps == 0, w < 7 or h < 7: counts_dev (and level_counts_dev) are zeroed
 * and nothing else is touched.  The output is the layout gsh_match_orb_batch reads (cap = nkps, n1 = counts_dev). */
void gsh_orb_extract_pyramid_batch_nostdlib(const uint8_t *img_dev, unsigned w, unsigned h, unsigned n,
                                            uint8_t *buffer_dev, struct gs_keypoint *kps_dev, unsigned *counts_dev,
                                            unsigned *level_counts_dev /* n x 4, may be NULL */,
                                            unsigned nkps, unsigned threshold, unsigned n_levels);

/* The same for the reference's DEFAULT build, whose atan2f / sinf are glibc's (ref :100-101): what `nanomagick orb` computes.
 * Arguments, buffer layout, output layout, the skipped levels, the degenerate cases, n == 0, the GS_ASSERTs and the frame
 * split are those of gsh_orb_extract_pyramid_batch_nostdlib; frame f's result is what extract_pyramid_orb_nm of the default
 * build returns and writes, bit for bit (angles and descriptors differ from the GS_NO_STDLIB flavour's for nearly every
 * keypoint).  The records and counts stay on the device, in the layout gsh_match_orb_batch reads.
 * The trig runs on the host, as in gsh_orb_extract_batch: FAST and the selection of every level of every frame, the disc
 * moments of every kept keypoint in one launch, ONE round trip for the whole call (moments and counts down, {angle, sin,
 * cos} up; from 4096 kept keypoints the host half runs on the library's thread pool), the descriptors in one launch.  The
 * call BLOCKS for that round trip -- also under gsh_set_async(1) -- and returns once the upload has left its pinned staging;
 * what it enqueues behind the round trip is stream-ordered on the current stream like every other batch entry. */
void gsh_orb_extract_pyramid_batch(const uint8_t *img_dev, unsigned w, unsigned h, unsigned n,
                                   uint8_t *buffer_dev, struct gs_keypoint *kps_dev, unsigned *counts_dev,
                                   unsigned *level_counts_dev /* n x 4, may be NULL */,
                                   unsigned nkps, unsigned threshold, unsigned n_levels);

/* Measurement hook (scripts/ubench_orb_pyramid_libm.py): where this thread's last gsh_orb_extract_pyramid_batch call that ran
 * under gsh_profile(1) spent its time, in ms: [0] device work before the round trip, [1] the copy down, [2] the host trig,
 * [3] the copy up, [4] device work after it.  Under gsh_profile(1) the call ends synchronised.  Zeros before such a call. */
void gsh_orb_pyramid_batch_times(double ms[5]);

/* Every plane p of every frame f of a batch buffer (gsh_orb_pyramid_batch_buffer_bytes(w, h, n_levels, n) bytes, the
 * level-major layout above) becomes a copy of plane p of single_dev, one frame's buffer in gsh_orb_extract_pyramid's layout
 * (gsh_orb_pyramid_buffer_bytes(w, h, n_levels) bytes): n identical frames.  For callers that reproduce a process in which
 * the pyramid is built over what an earlier extraction left behind -- `nanomagick orb` builds the scene's over the
 * template's -- since the never-written 3-px frames of the score maps are read by the NMS.  ONE launch per kMaxZ frames
 * (GSH_TUNE_FRAMES_PER_LAUNCH).  Device pointers at any alignment, stream-ordered.  n == 0 or n_levels == 0 writes nothing
 * and checks nothing.  GS_ASSERT: non-NULL pointers, w and h non-zero, the two buffers do not overlap. */
void gsh_orb_pyramid_buffer_fill_batch(uint8_t *buffer_dev, const uint8_t *single_dev,
                                       unsigned w, unsigned h, unsigned n_levels, unsigned n);

/* All pointers device; matches: max_matches records, the first *count written, the rest not; count: 1 u32.
 * Stream-ordered. */
void gsh_match_orb_dev(const struct gs_keypoint *k1, unsigned n1, const struct gs_keypoint *k2,
                       unsigned n2, struct gs_match *matches, unsigned *count,
                       unsigned max_matches, float max_distance);

/* ---- descriptor matching over a batch (ref :680-699; docs/design/detectors.md "Descriptor matching over a batch") -----
 * gs_match_orb for n pairs of keypoint sets in one launch.  All pointers device pointers, stream-ordered on the current
 * stream, no host synchronisation and no read-back (the library's grow-only scratch synchronises once when it has to
 * grow; it stays within 64 MiB whatever n is, unless a single pair needs more).  n == 0 returns before any check or launch.
 * GS_ASSERT: non-NULL k1, k2, matches, counts; cap1, cap2 non-zero; nset1 == 1 || nset1 == n; nset2 == 1 || nset2 == n.
 * Pair p takes its queries from set (nset1 == 1 ? 0 : p) of k1 -- the records at k1 + set * cap1, of which the first
 * min(n1[set], cap1) count, all cap1 when n1 is NULL -- and its train set from k2, cap2, n2, nset2 in the same way.  n1 and
 * n2 are read ON THE DEVICE: this is the layout gsh_orb_extract_batch_nostdlib leaves (cap = its nkps), so the two calls
 * chain with nothing in between.  k1 and k2 may alias; neither is written.
 * counts[p] and matches[p * max_matches ...] are what gs_match_orb(Q, nq, T, nt, out, max_matches, max_distance) returns
 * and writes, bit for bit: the ratio test in float, the first index of the minimum, matches in ascending query order;
 * the records at and beyond counts[p] are not written.  max_matches == 0 zeroes counts and does nothing else.
 * matches needs 4-byte alignment only.  The pairs of a call are split at GSH_TUNE_FRAMES_PER_LAUNCH like every batch. */
void gsh_match_orb_batch(const struct gs_keypoint *k1, unsigned cap1, const unsigned *n1, unsigned nset1,
                         const struct gs_keypoint *k2, unsigned cap2, const unsigned *n2, unsigned nset2,
                         unsigned n, struct gs_match *matches, unsigned *counts,
                         unsigned max_matches, float max_distance);

/* ---- "next" rows (ref :230, :255, :189) ------------------------------------------ */
void gsh_adaptive_threshold_batch(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h,
                                  unsigned n, unsigned radius, int c);
void gsh_filter_batch(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h, unsigned n,
                      const int8_t *kernel_host, unsigned kw, unsigned kh, unsigned norm);
void gsh_downsample_batch(uint8_t *dst, const uint8_t *src, unsigned sw, unsigned sh, unsigned n);

/* ---- geometry on batches and patches (ref :154-187; docs/design/stencils.md "Geometry") ------------
 * Frames dense and back to back (sw * sh resp. dw * dh bytes apart), all pointers device pointers, stream-ordered on the
 * current stream: no host synchronisation, no allocation, no table built on the host, no read-back.  n == 0 (or
 * npatches == 0) returns before any check or launch.  Sizes are non-zero, the roi of gsh_crop_batch lies inside the frame
 * and dst does not overlap src (GS_ASSERT).  Results are the reference's, frame by frame and bit for bit:
 *   gsh_crop_batch        frame f = gs_crop(dst_f, src_f, roi), dst frames roi.w x roi.h
 *   gsh_resize_batch      frame f = gs_resize(dst_f, src_f);  gsh_resize_nn_batch: gs_resize_nn
 *   gsh_crop_resize_batch patch p (dw x dh) = gs_resize -- gs_resize_nn when `nearest` -- of the image gs_crop gives for
 *                         rois_dev[p] of frame frame_of_dev[p] (frame p when frame_of_dev is NULL): the bilinear taps
 *                         clamp at the WINDOW's edges.  rois_dev and frame_of_dev are read on the device, e.g. as
 *                         gsh_lbp_detect_batch or gsh_blob_largest_batch left them; nothing can assert there, so a patch
 *                         whose rectangle is empty or does not lie inside the frame (x + w is tested without 32-bit
 *                         overflow) or whose frame index is >= n is filled with zeros, and nothing else is touched. */
void gsh_crop_batch(uint8_t *dst, const uint8_t *src, unsigned sw, unsigned sh, unsigned n, struct gs_rect roi);
void gsh_resize_batch(uint8_t *dst, unsigned dw, unsigned dh, const uint8_t *src, unsigned sw, unsigned sh, unsigned n);
void gsh_resize_nn_batch(uint8_t *dst, unsigned dw, unsigned dh, const uint8_t *src, unsigned sw, unsigned sh, unsigned n);
void gsh_crop_resize_batch(uint8_t *dst, unsigned dw, unsigned dh, const uint8_t *src, unsigned sw, unsigned sh, unsigned n,
                           const struct gs_rect *rois_dev, const unsigned *frame_of_dev /* NULL: patch p comes from frame p */,
                           unsigned npatches, int nearest);

/* ---- template matching over a batch (ref :705, :726; docs/design/stencils.md "Template matching over a batch") -----
 * All pointers device pointers, stream-ordered on the current stream, no host synchronisation and no read-back (the
 * library's grow-only scratch synchronises once when it has to grow).  n == 0 returns before any check or launch.
 * GS_ASSERT: non-NULL pointers, non-zero sizes, tw <= iw, th <= ih, ntmpl == 1 || ntmpl == n.
 * Each frame takes the route gs_match_template takes for one frame of that size (matrix cores, dot products, wide
 * templates); the matrix-core route chooses between its 64 x 128 and 32 x 64 tiles by the blocks of the whole launch.
 * Scratch: the frames are worked through in chunks whose prefix tables and window sums (ih (iw + 1) 4 + rw rh 4 bytes
 * per frame on the matrix-core route) stay within 128 MiB of context scratch whatever n is -- a single frame that needs
 * more is a chunk of its own; GSH_TUNE_TMATCH_CHUNK caps the frames of a chunk. */
/* n frames of iw x ih, frame f at img + f*iw*ih; ntmpl == 1: one template for all frames, ntmpl == n: template f at
   tmpl + f*tw*th; result: n maps of rw x rh = (iw-tw+1) x (ih-th+1), each byte for byte the reference's gs_match_template */
void gsh_match_template_batch(const uint8_t *img, unsigned iw, unsigned ih, unsigned n,
                              const uint8_t *tmpl, unsigned tw, unsigned th, unsigned ntmpl, uint8_t *result);
/* per frame the reference's gs_find_best_match (first maximum in raster order; an all-zero map gives {0,0});
   score[f] = the map's value there (0 for an all-zero map); score may be NULL */
void gsh_find_best_match_batch(const uint8_t *result, unsigned rw, unsigned rh, unsigned n,
                               struct gs_point *best, uint8_t *score);
/* == gsh_match_template_batch followed by gsh_find_best_match_batch, without a caller-visible result map: on the
   matrix-core route no map is written at all (each wave sends its best score and place to the frame's key word with one
   64-bit atomic maximum), the other routes keep a chunk's maps in scratch */
void gsh_locate_template_batch(const uint8_t *img, unsigned iw, unsigned ih, unsigned n,
                               const uint8_t *tmpl, unsigned tw, unsigned th, unsigned ntmpl,
                               struct gs_point *best, uint8_t *score);
/* A BANK of templates: every frame against m templates of one size (a marker dictionary, glyphs, patches cut by
 * gsh_crop_resize_batch).  Contract as above; n == 0 || m == 0 returns before any check or launch.  GS_ASSERT: non-NULL
 * pointers, non-zero sizes, tw <= iw, th <= ih.  From a handful of templates (GSH_TUNE_TMATCH_BANK) the cross term of all
 * templates is ONE matrix product on the matrix cores (positions x templates x taps; templates up to 512 wide and 32768
 * taps), below that a loop of the single-template launches; either way a frame's window sums are computed once, and the
 * scratch per frame is the prefix table and ONE plane of window sums whatever m is. */
/* n frames of iw x ih against a bank of m templates, all tw x th, template t at tmpl + t*tw*th.
 * result: n*m maps of rw x rh, map (f, t) at result + (f*m + t)*rw*rh, each byte for byte gs_match_template(frame f, template t) */
void gsh_match_templates_batch(const uint8_t *img, unsigned iw, unsigned ih, unsigned n,
                               const uint8_t *tmpl, unsigned tw, unsigned th, unsigned m, uint8_t *result);
/* == the above followed by gs_find_best_match on every map, with no caller-visible map:
 * best[f*m + t], score[f*m + t] (score may be NULL; an all-zero map gives {0,0} / 0);
 * winner (n entries, may be NULL): per frame the template with the highest score, the lowest index on ties */
void gsh_locate_templates_batch(const uint8_t *img, unsigned iw, unsigned ih, unsigned n,
                                const uint8_t *tmpl, unsigned tw, unsigned th, unsigned m,
                                struct gs_point *best, uint8_t *score, unsigned *winner);
/* WINDOWS read on the device: look for a patch only near where it was (a tracker's step).  Per window the result is the
 * reference's gs_find_best_match(gs_match_template(gs_crop(frame, window), tmpl)), bit for bit.
 * Common to the three entries: all pointers device pointers; stream-ordered on the current stream, obeying gsh_set_async;
 * no host synchronisation, no read-back and no table built on the host (the grow-only context scratch may synchronise
 * when it grows).  nwin == 0 returns before any check or launch.  GS_ASSERT: non-NULL pointers (score may be NULL),
 * non-zero sizes, tw <= max_ww && th <= max_wh, max_ww <= iw && max_wh <= ih, ntmpl == 1 || ntmpl == nwin, and
 * nwin <= n when frame_of_dev is NULL.
 * A window is VALID when its frame index is < n, w >= tw, h >= th, w <= max_ww, h <= max_wh and it lies inside the frame
 * (x + w <= iw is tested without 32-bit overflow, as gsh_crop_resize_batch does).  Nothing can assert on the device: an
 * invalid window gets best[p] = {0xFFFFFFFF, 0xFFFFFFFF} and score[p] = 0, and its map bytes are left untouched.
 * locate: for a valid window with c = gs_crop(frame, window), m = gs_match_template(c, tmpl), b = gs_find_best_match(m):
 *   best[p] = {window.x + b.x, window.y + b.y} in FRAME coordinates, score[p] = m[b]; the first maximum in the window's
 *   own raster order wins; an all-zero map gives the window's origin and score 0 (the reference's {0,0}; not the
 *   invalid sentinel).
 * match: map p is rw_p x rh_p = (w - tw + 1) x (h - th + 1) bytes with row pitch rw_p, at
 *   result + p * (max_ww - tw + 1) * (max_wh - th + 1); each map byte is the reference's; the bytes of the slot beyond the
 *   map are left untouched.
 * Any template size that fits a window is taken; the frames are neither copied nor required to have iw % 4 == 0. */
/* nwin windows; window p is windows_dev[p] (frame coordinates) in frame frame_of_dev[p]
   (frame p when frame_of_dev is NULL; then nwin <= n).  ntmpl == 1: one template for all windows,
   ntmpl == nwin: template p at tmpl + p*tw*th.  max_ww x max_wh: the host's upper bound on a window's size
   (it sizes the grid and the map pitch).  Everything else is read on the device. */
void gsh_locate_template_windows_batch(const uint8_t *img, unsigned iw, unsigned ih, unsigned n,
                                       const uint8_t *tmpl, unsigned tw, unsigned th, unsigned ntmpl,
                                       const struct gs_rect *windows_dev, const unsigned *frame_of_dev, unsigned nwin,
                                       unsigned max_ww, unsigned max_wh, struct gs_point *best, uint8_t *score /* may be NULL */);
void gsh_match_template_windows_batch(const uint8_t *img, unsigned iw, unsigned ih, unsigned n,
                                      const uint8_t *tmpl, unsigned tw, unsigned th, unsigned ntmpl,
                                      const struct gs_rect *windows_dev, const unsigned *frame_of_dev, unsigned nwin,
                                      unsigned max_ww, unsigned max_wh, uint8_t *result);
/* the glue that makes one time step's `best` the next step's windows with nothing in between:
 * windows_dev[p] = the box {at.x, at.y, bw, bh} grown by mx / my on every side and clipped to the frame --
 * x0 = at.x > mx ? at.x - mx : 0, x1 = min(at.x + bw + mx, iw) computed in 64 bits, the same for y, {x0, y0, x1 - x0, y1 - y0}.
 * A point with x >= iw or y >= ih gives {0, 0, 0, 0} -- the invalid sentinel among them, so invalidity propagates down
 * a chain.  GS_ASSERT: non-NULL pointers, bw, bh, iw, ih > 0. */
void gsh_search_windows_batch(const struct gs_point *at_dev, unsigned nwin, unsigned bw, unsigned bh,
                              unsigned mx, unsigned my, unsigned iw, unsigned ih, struct gs_rect *windows_dev);

/* ---- connected components, blob corners, perspective correction (ref :330, :404, :423) ----------
 * The reference's document-scanner chain (blur -> Otsu threshold -> gs_blobs -> largest blob ->
 * gs_blob_corners -> gs_perspective_correct) on n same-size frames without a host round trip.
 * labels: n x w x h; blobs: n x nblobs records, frame f's first counts[f] written (all 32 bytes, the two padding bytes
 * behind `label` as 0; the rest untouched);
 * counts: n.  Corners: blobs holds ONE record per frame (e.g. each frame's largest), corners n x 4
 * points {tl, tr, br, bl}; perspective: dst n x dw x dh from src n x sw x sh and n x 4 corners. */
void gsh_blobs_batch(const uint8_t *img, unsigned w, unsigned h, unsigned n, gs_label *labels,
                     struct gs_blob *blobs, unsigned *counts, unsigned nblobs);
void gsh_blob_corners_batch(const uint8_t *img, const gs_label *labels, unsigned w, unsigned h,
                            unsigned n, const struct gs_blob *blobs, struct gs_point *corners);
void gsh_perspective_correct_batch(uint8_t *dst, unsigned dw, unsigned dh, const uint8_t *src,
                                   unsigned sw, unsigned sh, unsigned n,
                                   const struct gs_point *corners);
/* gsh_blob_largest_batch: largest[f] = the FIRST record of maximum area among the first min(counts[f], nblobs) of
 * frame f (the strict `>` of ref nanomagick.c:197-199), index[f] (index may be NULL) its position; a frame without
 * blobs gets 32 zero bytes and index 0xffffffff (the reference reads an uninitialised record there).
 * gsh_blob_paint_batch: the picture nanomagick's `blobs` verb draws (ref nanomagick.c:160-169) from blobs / counts as
 * gsh_blobs_batch left them (records in label order: box.y never decreases): dst (n x w x h, every byte written, must
 * not overlap img) = 255 where img > 128, else 128 inside a blob's box padded by 2, else 0.  The reference's loops are
 * inclusive and address y * w + x with x <= w, y <= h: a box that reaches the right edge also marks column 0 of the
 * next row, and where the reference would write at or past w * h (outside its buffer) nothing is written.  One pass
 * over the pixels; frames wider than 65521 pixels take two.  GSH_TUNE_STRIP_BAND_ROWS also sets this kernel's rows
 * per band.  Both are stream-ordered, all pointers device pointers. */
void gsh_blob_largest_batch(const struct gs_blob *blobs, unsigned nblobs, const unsigned *counts, unsigned n,
                            struct gs_blob *largest, unsigned *index);
void gsh_blob_paint_batch(uint8_t *dst, const uint8_t *img, unsigned w, unsigned h, unsigned n,
                          const struct gs_blob *blobs, unsigned nblobs, const unsigned *counts);

/* ---- contours (ref :446; docs/design/contours.md) -------------------------------------------------
 * gsh_trace_contours_batch: frame f traces contours[f * per_frame + k] for k < counts[f] (counts == NULL: all
 * per_frame; values above per_frame are clamped) ONE AFTER THE OTHER IN INDEX ORDER on frame f's own `visited` plane
 * (n x w x h, the caller's bytes: 0 = not visited) -- what the same sequence of gs_trace_contour calls does: a
 * later contour's length skips the pixels an earlier one marked.  Frames run side by side.  Of each record `start`
 * is read, `box` and `length` are written.  status[f * per_frame + k] (may be NULL): 0 the walk ended, 1 it is
 * endless in the reference (a state repeated; box, length and visited are the values it converges to), 2 the cap
 * on the moves of one walk was reached (a bug).  Records and status bytes at and beyond counts[f] are not written.
 * img and visited must not overlap.
 * gsh_blob_contour_starts_batch: for blob k < counts[f] of frame f (counts == NULL: all nblobs; labels, blobs,
 * counts as gsh_blobs_batch left them), contours[f * nblobs + k].start = the raster-first pixel that carries the
 * blob's label (it lies in row box.y, at x >= box.x); nothing else of the record is written. */
void gsh_trace_contours_batch(const uint8_t *img, uint8_t *visited, unsigned w, unsigned h, unsigned n,
                              struct gs_contour *contours, unsigned per_frame, const unsigned *counts,
                              uint8_t *status);
void gsh_blob_contour_starts_batch(const gs_label *labels, unsigned w, unsigned h, unsigned n,
                                   const struct gs_blob *blobs, unsigned nblobs, const unsigned *counts,
                                   struct gs_contour *contours);

/* ---- synthetic frames + checksums on device (SURVEY.md 8c generator) ------------- */
/* frame f = synth(w, h, seed0 + f): bit-identical to the CPU generator. */
void gsh_synth_batch(uint8_t *dst, unsigned w, unsigned h, unsigned n, uint32_t seed0);
/* sums[f] = order-independent 64-bit checksum of frame f (sum of (i+1)*FNVmix(byte)) */
void gsh_checksum_batch(const uint8_t *img, size_t frame_bytes, unsigned n, uint64_t *sums);

/* ---- multi-GPU control plane for one-process host programs ---------
 * One host thread per device (gsh_set_device) and one communicator per device, created together by
 * ncclCommInitAll over the listed devices (devices == NULL: 0 .. ndev-1).  RCCL over xGMI carries control traffic
 * only -- the cascade blob, per-file counts and checksums, the closing max of the elapsed time; frames shard by
 * file / frame and never cross GPUs (the reference has no counterpart: grayskull.h holds no state across images).
 * librccl.so is dlopen()ed by gsh_comm_init_all: ndev == 1 takes local copies (GS_COMM_RCCL=1 asks for a one-rank RCCL
 * communicator), ndev > 1 without a usable librccl (or with GS_COMM_BACKEND=host) a host-rendezvous backend: the KB-scale
 * payloads bounce through host memory, the worker threads meet at a rendezvous.
 * Every collective takes DEVICE buffers, must be called by the thread that drives that communicator's device and is
 * enqueued on that thread's stream (gsh_sync() before the host reads a result).  Precondition failures and RCCL
 * errors abort like everything else here. */
typedef struct gsh_comm gsh_comm;
int gsh_comm_init_all(gsh_comm **comms, int ndev, const int *devices); /* 0 (a backend is always found) */
void gsh_comm_destroy_all(gsh_comm **comms, int ndev);
int gsh_comm_rank(const gsh_comm *c);
int gsh_comm_world(const gsh_comm *c);
const char *gsh_comm_backend(const gsh_comm *c); /* "rccl 2.x.y (ncclCommInitAll, N ranks)" | "local copies ..." */
void gsh_comm_broadcast(gsh_comm *c, void *buf_dev, size_t bytes, int root);
void gsh_comm_all_gather(gsh_comm *c, const void *send_dev, void *recv_dev, size_t bytes_per_rank);
void gsh_comm_all_reduce_u64(gsh_comm *c, unsigned long long *buf_dev, size_t n, int op); /* op: 0 sum, 1 max; in place */
void gsh_comm_all_reduce_f64(gsh_comm *c, double *buf_dev, size_t n, int op);

#ifdef __cplusplus
}
#endif
#endif /* GRAYSKULL_HIP_H */
