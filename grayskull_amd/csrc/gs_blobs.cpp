/*
 * gs_blobs.cpp -- launchers and C ABI of connected components (gs_blobs, ref grayskull.h:330-402), blob corners
 * (gs_blob_corners, ref :404-421) and perspective correction (gs_perspective_correct, ref :423-444): the reference's
 * own names and signatures (include/grayskull.h) and the device-resident batch entry points (include/grayskull_hip.h),
 * among them what nanomagick's `scan` and `blobs` verbs do with the records: each frame's largest blob and the picture of
 * the padded boxes (ref nanomagick.c:160-169, :196-199).
 * The kernels and the definition of what they compute are in k_blobs.h.
 */
#include "gs_internal.h"

#include "k_blobs.h"

namespace gsi {

static_assert(sizeof(BlobRec) == sizeof(struct gs_blob), "struct gs_blob is 32 bytes (ref :27-34)");
constexpr size_t kBlobParBudget = (size_t)4 << 30; /* bytes of parent array per launch group */

/* the blobs of n frames: labels n x w x h, records n x stride (the first counts[f] of each frame written), counts n */
static void launch_blobs(const uint8_t *img, unsigned w, unsigned h, unsigned n, uint16_t *labels, BlobRec *blobs, size_t stride,
                         unsigned *counts, unsigned nblobs) {
  /* gs_label is u16: at most 65535 labels.  With nblobs >= 65535 the reference's label counter wraps to 0 once 65535
   * start pixels have been numbered; k_blob_compact reproduces what it returns then (m = 0). */
  const unsigned cap = std::min(nblobs, kBlobCapMax), nslot = cap + 1u, wrap = nblobs >= kBlobCapMax ? 1u : 0u;
  const unsigned W = (w + 63u) / 64u;
  const size_t np = (size_t)w * h, words = (size_t)h * W;
  /* the parent array takes 4 B per pixel of every frame in a launch (only run starts are touched): launches of at most
   * 4 GiB of it, 128 frames of 3840 x 2160 */
  const unsigned G = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min(kMaxZ, n), kBlobParBudget / (np * 4u)));
  uint64_t *bits = (uint64_t *)ctx().scratch(SL_BLOB_BITS, (size_t)G * words * 8u);
  unsigned *par = (unsigned *)ctx().scratch(SL_BLOB_PAR, (size_t)G * np * 4u);
  unsigned *stats = (unsigned *)ctx().scratch(SL_BLOB_STAT, (size_t)G * nslot * kBlobSlot * 4u);
  unsigned *rowcnt = (unsigned *)ctx().scratch(SL_BLOB_ROW, (size_t)G * (2u * h + kBlobInfo) * 4u);
  unsigned *rowpre = rowcnt + (size_t)G * h, *info = rowpre + (size_t)G * h;
  hipStream_t st = ctx().s();
  const dim3 rows((h + 3u) / 4u);
  for_frames(n, G, [&](unsigned f0, unsigned nn) {
    const uint8_t *im = img + np * f0;
    uint16_t *lab = labels + np * f0;
    GS_HIP(hipMemsetAsync(stats, 0, (size_t)nn * nslot * kBlobSlot * 4u, st));
    GS_LAUNCH(k_blob_fg, dim3(rows.x, nn), dim3(256), 0, st, im, w, h, W, bits);
    GS_LAUNCH(k_blob_count, dim3(rows.x, nn), dim3(256), 0, st, (const uint64_t *)bits, h, W, rowcnt);
    GS_LAUNCH(k_blob_scan, dim3(nn), dim3(1024), 0, st, (const unsigned *)rowcnt, (const uint64_t *)bits, w, h, W, cap, rowpre, info);
    /* from here on `bits` holds M: frames without a P exit at once, the others are closed by one wave each */
    GS_LAUNCH(k_blob_close, dim3(nn), dim3(64), 0, st, bits, w, h, W, (const unsigned *)info);
    GS_LAUNCH(k_blob_init, dim3(rows.x, nn), dim3(256), 0, st, (const uint64_t *)bits, w, h, W, par);
    GS_LAUNCH(k_blob_union, dim3(rows.x, nn), dim3(256), 0, st, (const uint64_t *)bits, w, h, W, par);
    /* k_blob_roots reads the start pixels of fg, which k_blob_close changed for capped frames -- but only after P,
     * and every root lies before P, where M = fg: the start bits it needs are still those of fg */
    GS_LAUNCH(k_blob_roots, dim3(rows.x, nn), dim3(256), 0, st, (const uint64_t *)bits, (const uint64_t *)bits, w, h, W, par,
              (const unsigned *)rowpre, lab);
    GS_LAUNCH(k_blob_label, dim3((h + 4u * kBlobBand - 1u) / (4u * kBlobBand), nn), dim3(256), 0, st, (const uint64_t *)bits, w, h, W,
              (const unsigned *)par, lab, stats, nslot);
    GS_LAUNCH(k_blob_compact, dim3(nn), dim3(1024), 0, st, (const unsigned *)stats, nslot, cap, wrap, (const unsigned *)info,
              blobs + stride * f0, stride, counts + f0);
  });
}

static void launch_corners(const uint8_t *img, const uint16_t *labels, unsigned w, unsigned h, unsigned n, const BlobRec *blobs,
                           uint32_t *corners) {
  unsigned long long *keys = (unsigned long long *)ctx().scratch(SL_BLOB_ROW, (size_t)std::min(kMaxZ, n) * kCornerKeys * 8u);
  hipStream_t st = ctx().s();
  const size_t np = (size_t)w * h;
  const unsigned nb = std::min((h + 3u) / 4u, 128u); /* blocks per frame: waves stride over the rows of the box */
  for_frames(n, [&](unsigned f0, unsigned nn) {
    GS_LAUNCH(k_corners_init, dim3(nn), dim3(64), 0, st, keys);
    GS_LAUNCH(k_corners, dim3(nb, nn), dim3(256), 0, st, img + np * f0, labels + np * f0, w, h, blobs + f0, keys);
    GS_LAUNCH(k_corners_final, dim3(nn), dim3(64), 0, st, (const unsigned long long *)keys, blobs + f0, corners + (size_t)8u * f0);
  });
}

static void launch_perspective(uint8_t *dst, unsigned dw, unsigned dh, const uint8_t *src, unsigned sw, unsigned sh, unsigned n,
                               const uint32_t *corners) {
  hipStream_t st = ctx().s();
  for_frames(n, [&](unsigned f0, unsigned nn) {
    GS_LAUNCH(k_perspective, grid2d(dw, dh, nn), dim3(64, 4), 0, st, dst + (size_t)dw * dh * f0, dw, dh, src + (size_t)sw * sh * f0, sw, sh,
              corners + (size_t)8u * f0);
  });
}

static void launch_largest(const BlobRec *blobs, unsigned nblobs, const unsigned *counts, unsigned n, BlobRec *largest,
                           unsigned *index) {
  hipStream_t st = ctx().s();
  const dim3 block(nblobs <= 4096u ? 64u : 256u); /* one wave per frame; a block for long record lists */
  for_frames(n, [&](unsigned f0, unsigned nn) {
    GS_LAUNCH(k_blob_largest, dim3(nn), block, 0, st, blobs + (size_t)nblobs * f0, nblobs, counts + f0, largest + f0, index ? index + f0 : nullptr);
  });
}

/* rows per band of k_blob_paint: about 32 KB of pixels per block (eight 16-byte steps per lane), fewer while the launch
 * has under four blocks per CU to hand out, never more than the coverage bits of a block hold; gsh_tune key 0 (rows per
 * band) overrides the first two.  0: a row does not fit (w > kPaintBits - 15 = 65521) -- the two-pass fallback. */
static unsigned paint_band_rows(unsigned w, unsigned h, unsigned n) {
  if (w > kPaintBits - 15u) return 0;
  const unsigned fit = (kPaintBits - 15u) / w;
  unsigned R = (32768u + w - 1u) / w;
  while (R > 1u && (size_t)n * ((h + R - 1u) / R) < (size_t)4u * topo().cus) R = (R + 1u) / 2u;
  if (g_tune[GSH_TUNE_STRIP_BAND_ROWS] > 0) R = (unsigned)g_tune[GSH_TUNE_STRIP_BAND_ROWS];
  return std::max(1u, std::min(std::min(R, fit), h));
}

static void launch_paint(uint8_t *dst, const uint8_t *img, unsigned w, unsigned h, unsigned n, const BlobRec *blobs, unsigned nblobs,
                         const unsigned *counts) {
  hipStream_t st = ctx().s();
  const size_t np = (size_t)w * h;
  const unsigned R = paint_band_rows(w, h, n);
  for_frames(n, [&](unsigned f0, unsigned nn) {
    uint8_t *d = dst + np * f0;
    const uint8_t *s = img + np * f0;
    const BlobRec *b = blobs + (size_t)nblobs * f0;
    if (R) {
      GS_LAUNCH(k_blob_paint, dim3((h + R - 1u) / R, nn), dim3(256), 0, st, d, s, w, h, R, b, nblobs, counts + f0);
    } else {
      const unsigned bx = (unsigned)std::max<size_t>(1, std::min<size_t>((np + 4095u) / 4096u, 2048));
      GS_LAUNCH(k_blob_paint_base, dim3(bx, nn), dim3(256), 0, st, d, s, np);
      GS_LAUNCH(k_blob_paint_fill, dim3(std::min(nblobs, 1024u), nn), dim3(256), 0, st, d, s, w, h, b, nblobs, counts + f0);
    }
  });
}

}  // namespace gsi

extern "C" {

/* ---- drop-in ------------------------------------------------------------------------------------------------------ */
unsigned gs_blobs(struct gs_image img, gs_label *labels, struct gs_blob *blobs, unsigned nblobs) { /* ref :330 */
  GS_ASSERT(GS_VALID(img) && labels != NULL && blobs != NULL && nblobs > 0);
  GS_ASSERT((unsigned long long)img.w * img.h <= 0xffffffffull); /* pixel indices are u32 (so are the reference's) */
  const size_t np = (size_t)img.w * img.h;
  const unsigned cap = std::min(nblobs, kBlobCapMax);
  const uint8_t *s = stage_in(img.data, np, SL_IN);
  const Staged<uint16_t> l(labels, np * 2u, SL_BLOB_LAB);
  const bool bhost = !is_dev(blobs);
  char *rec = (char *)ctx().scratch(SL_BLOB_REC, 16u + (bhost ? (size_t)cap * sizeof(BlobRec) : 0u));
  unsigned *count = (unsigned *)rec;
  BlobRec *b = bhost ? (BlobRec *)(rec + 16) : (BlobRec *)blobs;
  launch_blobs(s, img.w, img.h, 1, l.dev, b, cap, count, nblobs);
  unsigned *m = (unsigned *)ctx().pinned(Ctx::PIN_A, sizeof(unsigned));
  GS_HIP(hipMemcpyAsync(m, count, sizeof(unsigned), hipMemcpyDeviceToHost, ctx().s()));
  l.back();
  ctx().sync();
  const unsigned nb = *m;
  /* records [m, nblobs) are not written (the reference leaves stale provisional data there) */
  if (bhost && nb) {
    GS_HIP(hipMemcpyAsync(blobs, b, (size_t)nb * sizeof(BlobRec), hipMemcpyDeviceToHost, ctx().s()));
    ctx().sync();
  }
  return nb;
}

void gs_blob_corners(struct gs_image img, gs_label *labels, struct gs_blob *b, struct gs_point c[4]) { /* ref :404 */
  GS_ASSERT(GS_VALID(img) && b && labels);
  const size_t np = (size_t)img.w * img.h;
  const uint8_t *s = stage_in(img.data, np, SL_IN);
  const uint16_t *l = stage_in(labels, np * 2u, SL_BLOB_LAB);
  const BlobRec *bd = (const BlobRec *)stage_in(b, sizeof(BlobRec), SL_BLOB_REC);
  const Staged<uint32_t> cd((uint32_t *)c, 4u * sizeof(struct gs_point), SL_BLOB_STAT);
  launch_corners(s, l, img.w, img.h, 1, bd, cd.dev);
  cd.done();
}

void gs_perspective_correct(struct gs_image dst, struct gs_image src, struct gs_point c[4]) { /* ref :423 */
  GS_ASSERT(GS_VALID(dst) && GS_VALID(src));
  const uint32_t *cd = (const uint32_t *)stage_in(c, 4u * sizeof(struct gs_point), SL_BLOB_REC);
  image_to_image(dst, src, [&](uint8_t *d, const uint8_t *s) { launch_perspective(d, dst.w, dst.h, s, src.w, src.h, 1, cd); });
}

/* ---- device-resident batches -------------------------------------------------------------------------------------- */
void gsh_blobs_batch(const uint8_t *img, unsigned w, unsigned h, unsigned n, gs_label *labels, struct gs_blob *blobs,
                     unsigned *counts, unsigned nblobs) {
  GS_ASSERT(img && labels && blobs && counts && w > 0 && h > 0 && nblobs > 0);
  GS_ASSERT((unsigned long long)w * h <= 0xffffffffull);
  if (n == 0) return;
  launch_blobs(img, w, h, n, labels, (BlobRec *)blobs, nblobs, counts, nblobs);
}

void gsh_blob_corners_batch(const uint8_t *img, const gs_label *labels, unsigned w, unsigned h, unsigned n,
                            const struct gs_blob *blobs, struct gs_point *corners) {
  GS_ASSERT(img && labels && blobs && corners && w > 0 && h > 0);
  if (n == 0) return;
  launch_corners(img, labels, w, h, n, (const BlobRec *)blobs, (uint32_t *)corners);
}

void gsh_perspective_correct_batch(uint8_t *dst, unsigned dw, unsigned dh, const uint8_t *src, unsigned sw, unsigned sh,
                                   unsigned n, const struct gs_point *corners) {
  GS_ASSERT(dst && src && corners && dw > 0 && dh > 0 && sw > 0 && sh > 0);
  if (n == 0) return;
  launch_perspective(dst, dw, dh, src, sw, sh, n, (const uint32_t *)corners);
}

void gsh_blob_largest_batch(const struct gs_blob *blobs, unsigned nblobs, const unsigned *counts, unsigned n,
                            struct gs_blob *largest, unsigned *index) {
  GS_ASSERT(blobs && counts && largest && nblobs > 0);
  if (n == 0) return;
  launch_largest((const BlobRec *)blobs, nblobs, counts, n, (BlobRec *)largest, index);
}

void gsh_blob_paint_batch(uint8_t *dst, const uint8_t *img, unsigned w, unsigned h, unsigned n, const struct gs_blob *blobs,
                          unsigned nblobs, const unsigned *counts) {
  GS_ASSERT(dst && img && blobs && counts && w > 0 && h > 0 && nblobs > 0);
  GS_ASSERT((unsigned long long)w * h <= 0xffffffffull);
  if (n == 0) return;
  GS_ASSERT(dst + (size_t)w * h * n <= img || img + (size_t)w * h * n <= dst); /* dst is written while img is read */
  launch_paint(dst, img, w, h, n, (const BlobRec *)blobs, nblobs, counts);
}

}  // extern "C"
