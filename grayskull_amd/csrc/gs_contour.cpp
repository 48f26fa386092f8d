/*
 * gs_contour.cpp -- launchers and C ABI of contour tracing (gs_trace_contour, ref grayskull.h:446-480): the reference's
 * own name and signature (include/grayskull.h) and the device-resident batch entry points (include/grayskull_hip.h).
 * The kernels and the definition of what they compute are in k_contour.h.
 */
#include "gs_internal.h"

#include "k_contour.h"

namespace gsi {

static_assert(sizeof(struct gs_blob) == 4u * kContourBlobWords, "struct gs_blob is 32 bytes (ref :27-34)");
static_assert(sizeof(ContourRec) == sizeof(struct gs_contour) && sizeof(struct gs_contour) == 28, "struct gs_contour is 28 bytes (ref :36-40)");

/* the walk is a map on at most 16 w h + 1 states (p inside the image or the start, dir, seenstart); Brent's search finds
 * the first repeat within three times the moves up to it, the extra trip is one cycle more */
static unsigned long long move_cap(unsigned w, unsigned h) {
  const unsigned long long np = (unsigned long long)w * h; /* < 2^62 */
  return np >= (1ull << 56) ? ~0ull : 5ull * (16ull * np + 1ull) + 64ull; /* saturates: no frame that fits a memory gets there */
}

static void launch_trace(const uint8_t *img, uint8_t *visited, unsigned w, unsigned h, unsigned n, ContourRec *recs, unsigned per_frame,
                         const unsigned *counts, uint8_t *status) {
  const size_t np = (size_t)w * h;
  hipStream_t st = ctx().s();
  for_frames(n, [&](unsigned f0, unsigned nn) {
    GS_LAUNCH(k_contour_trace, dim3(nn), dim3(64), 0, st, img + np * f0, visited + np * f0, w, h, recs + (size_t)per_frame * f0, per_frame,
              counts ? counts + f0 : (const unsigned *)nullptr, status ? status + (size_t)per_frame * f0 : (uint8_t *)nullptr, move_cap(w, h));
  });
}

static void launch_starts(const uint16_t *labels, unsigned w, unsigned h, unsigned n, const uint32_t *blobs, unsigned nblobs,
                          const unsigned *counts, ContourRec *recs) {
  const size_t np = (size_t)w * h;
  hipStream_t st = ctx().s();
  for_frames(n, [&](unsigned f0, unsigned nn) {
    GS_LAUNCH(k_contour_starts, dim3((nblobs + 3u) / 4u, nn), dim3(256), 0, st, labels + np * f0, w, h, blobs + (size_t)nblobs * kContourBlobWords * f0, nblobs,
              counts ? counts + f0 : (const unsigned *)nullptr, recs + (size_t)nblobs * f0);
  });
}

}  // namespace gsi

extern "C" {

/* ---- drop-in ------------------------------------------------------------------------------------------------------ */
void gs_trace_contour(struct gs_image img, struct gs_image visited, struct gs_contour *c) { /* ref :446 */
  if (!(GS_VALID(img) && GS_VALID(visited) && img.w == visited.w && img.h == visited.h)) { /* the reference's own text (ref :447) */
    fprintf(stderr, "Assertion failed: %s\n", "gs_valid(img) && gs_valid(visited) && img.w == visited.w && img.h == visited.h");
    abort();
  }
  GS_ASSERT(c != NULL);
  GS_ASSERT(img.w <= 0x7fffffffu && img.h <= 0x7fffffffu); /* the reference compares coordinates as int */
  const size_t np = (size_t)img.w * img.h;
  const uint8_t *s = stage_in(img.data, np, SL_IN);
  const Staged<uint8_t> v(visited.data, np, SL_OUT, /*copy_in=*/true);
  ContourRec *rec = (ContourRec *)ctx().scratch(SL_BLOB_REC, sizeof(ContourRec));
  ContourRec *back = (ContourRec *)ctx().pinned(Ctx::PIN_A, sizeof(ContourRec));
  GS_HIP(hipMemcpyAsync(rec, c, sizeof(ContourRec), hipMemcpyHostToDevice, ctx().s()));
  launch_trace(s, v.dev, img.w, img.h, 1, rec, 1, nullptr, nullptr);
  GS_HIP(hipMemcpyAsync(back, rec, sizeof(ContourRec), hipMemcpyDeviceToHost, ctx().s()));
  v.back();
  ctx().sync();
  c->box.x = back->bx, c->box.y = back->by, c->box.w = back->bw, c->box.h = back->bh;
  c->length = back->length;
}

/* ---- device-resident batches -------------------------------------------------------------------------------------- */
void gsh_trace_contours_batch(const uint8_t *img, uint8_t *visited, unsigned w, unsigned h, unsigned n, struct gs_contour *contours,
                              unsigned per_frame, const unsigned *counts, uint8_t *status) {
  GS_ASSERT(img && visited && contours && w > 0 && h > 0);
  GS_ASSERT(w <= 0x7fffffffu && h <= 0x7fffffffu);
  if (n == 0 || per_frame == 0) return;
  launch_trace(img, visited, w, h, n, (ContourRec *)contours, per_frame, counts, status);
}

void gsh_blob_contour_starts_batch(const gs_label *labels, unsigned w, unsigned h, unsigned n, const struct gs_blob *blobs,
                                   unsigned nblobs, const unsigned *counts, struct gs_contour *contours) {
  GS_ASSERT(labels && blobs && contours && w > 0 && h > 0);
  if (n == 0 || nblobs == 0) return;
  launch_starts(labels, w, h, n, (const uint32_t *)blobs, nblobs, counts, (ContourRec *)contours);
}

}  // extern "C"
