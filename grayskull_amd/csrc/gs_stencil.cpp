/*
 * gs_stencil.cpp -- launchers and C ABI of the pixel-plane operations of libgrayskull_hip.so: gs_blur / gs_sobel /
 * gs_erode / gs_dilate, histogram / Otsu / threshold, the fused config-2 pipeline, gs_integral, adaptive threshold /
 * filter / downsample, geometry and template matching, the synthetic-frame generator and the checksums.  Both the
 * reference's own names and signatures (include/grayskull.h, each citing the reference definition it replaces) and the
 * device-resident batch entry points of include/grayskull_hip.h.  Every compute step is a HIP kernel from k_*.h.
 */
#include "gs_internal.h"

#include "k_geom.h"
#include "k_codes.h"
#include "k_integral.h"
#include "k_pointwise.h"
#include "k_resize.h"
#include "k_stencil.h"
#include "k_tmatch.h"
#include "k_tmatch_win.h"

namespace gsi {

/* rows: output rows per frame.  One wave per (1024-px column block, band, frame).
 * HBM-bound per-call kernels (waves_per_simd >= 5) take SHORT bands of 8 rows (more for wide halos):
 * blocks are dispatched in band order, so the few thousand waves that are resident at any time work
 * on neighbouring rows of a few frames -- the DRAM pages they stream through are shared and the
 * halo rows of the next band are still in the Infinity Cache -- instead of each wave streaming its
 * own distant band.  Measured (profiles/r02g_small_bands_*.log, 64 frames): gs_sobel 4096x4096
 * 4.87 -> 5.62 TB/s (0.61 -> 0.70 of 8 TB/s) although it re-reads 2 halo rows per 8, 3840x2160
 * 4.76 -> 5.23; gs_blur(2) 4.88 -> 5.34 / 4.65 -> 4.90; erode 5.05 -> 5.57; plain strip copy 5.08 ->
 * 5.59.  Round 1 sized bands so that every wave of the launch was resident at once (20 bands of
 * 108 rows for 64 4K frames) and never tried bands below 16 rows.
 * The VALU-heavy fused kernels (waves_per_simd 3) keep long bands: each band first recomputes
 * 2R+2 rows of horizontal sums (8-row bands: 0.25 -> 0.38 ms per 64 frames). */
StripCfg strip_cfg(unsigned w, unsigned rows, unsigned n, unsigned waves_per_simd, unsigned halo_rows, unsigned short_T, int rg) {
  StripCfg c;
  /* lanes to place (k_strip.h): ragged rows may idle lane 0, the realigning flavour uses the lane behind the last one.
   * rg = -1: the caller's kernel has no flavours (or ignores the extra lane) */
  const unsigned strips = (w + 15) / 16 + (rg == 2 ? strip_realign_shift(w) + strip_realign_helper(w) : rg == 1 ? strip_ragged_shift(w) : (w & 15u) ? 1u : 0u);
  const unsigned long long waves_x = (strips + 63) / 64;
  unsigned long long t;
  if (g_tune[GSH_TUNE_STRIP_BAND_ROWS] > 0) {
    t = (unsigned long long)g_tune[GSH_TUNE_STRIP_BAND_ROWS];
  } else if (waves_per_simd >= 5) {
    /* round 3, with the XCD-aware band mapping (a band's halo rows were just fetched by its own XCD) even shorter bands
     * pay: gs_sobel 6 rows (4096^2 0.706 -> 0.720 of the peak, 512 x 4K 0.705 -> 0.722; odd heights break its 2-row
     * unroll groups), gs_blur(2) 6 (0.671 -> 0.703 / 0.692 -> 0.705), gs_blur(1) and the morphology 4 (0.707 -> 0.730,
     * 0.716 -> 0.738 / 0.728 -> 0.746); profiles/r03l_strip_band_height_xcd.log.  short_T is the caller's choice. */
    t = std::max(short_T, 2u * halo_rows);
  } else {
    /* bands per frame: the launch should fill the chip's resident-wave capacity a whole number of
     * times.  One round when the batch is small enough; for big batches (512 4K frames: 2048 wave
     * columns against 3072 slots at 3 waves per SIMD) one band per frame would leave a third of the
     * chip idle for the whole launch and two bands would run a 1.33rd round at a third occupancy, so
     * take the band count whose last round is fullest (here 3: exactly two rounds; gsh_blur_sobel_batch
     * 512 frames 1.96 -> 1.89 ms, 200 frames 0.90 -> 0.74 ms, profiles/r02f_band_count_512.log). */
    const unsigned long long cap = (unsigned long long)topo().simds() * waves_per_simd, wn = waves_x * n;
    const unsigned long long nb_max = rows / 8 ? rows / 8 : 1; /* bands of >= 8 rows */
    unsigned long long nb = cap / wn;
    if (nb < 1) nb = 1;
    if (nb > nb_max) nb = nb_max;
    /* (only for the VALU-heavy fused kernels, which run 3 waves per SIMD: the HBM-bound per-call
     * kernels lose 3-6 % to the extra halo rows of shorter bands, profiles/r02f_band_count_512.log) */
    if (waves_per_simd <= 3 && nb < 4 && wn * nb * 8 < cap * 7) { /* a lone round under 7/8 full: try 2..6 rounds */
      double best = (double)((wn * nb + cap - 1) / cap) * cap / (double)(wn * nb);
      for (unsigned long long c = nb + 1; c <= nb_max && c <= nb + 6; c++) {
        const double waste = (double)((wn * c + cap - 1) / cap) * cap / (double)(wn * c);
        if (waste < best - 0.02) best = waste, nb = c;
      }
    }
    t = (rows + nb - 1) / nb;
  }
  c.T = (unsigned)t;
  const unsigned nb = (rows + c.T - 1) / c.T;
  /* block shape: 256 threads = 4 waves; a wave is 1024 px of a row.  Frames narrower than 4096 px put the spare
   * waves on further BANDS (64 x 4 up to 1024 px, 128 x 2 up to 2048 px) instead of columns that do not exist --
   * a 1920-px row kept two of a 256 x 1 block's four waves busy computing on zero fill (8 x 1080p gs_sobel at 0.21
   * of the HBM peak).  Key 1: 1 / 2 / 3 force 64 x 4 / 128 x 2 / 256 x 1, 0 = by width. */
  unsigned bx = 256, by = 1;
  if (g_tune[GSH_TUNE_STRIP_BLOCK_SHAPE] == 1 || (g_tune[GSH_TUNE_STRIP_BLOCK_SHAPE] == 0 && strips <= 64)) bx = 64, by = 4;
  else if (g_tune[GSH_TUNE_STRIP_BLOCK_SHAPE] == 2 || (g_tune[GSH_TUNE_STRIP_BLOCK_SHAPE] == 0 && strips <= 128)) bx = 128, by = 2;
  c.block = dim3(bx, by);
  c.grid = dim3((strips + bx - 1) / bx, (nb + by - 1) / by, n);
  /* XCD-aware band mapping for the short-band (HBM-bound) kernels: one block per band row (w <= 4096), the band
   * count padded to a multiple of 8 (blocks past the last band return at once).  Key 18: 1 = off, 2 = always. */
  /* measured (profiles/r03g_strip_xcd_bands.log): 512 x 4K gs_blur(2) +3.1 %, gs_erode +2.6 %, gs_sobel +2.0 %,
   * 64 x 4096^2 copy +2 %, sobel -1 % (noise); gs_filter (waves_per_simd 6) -3.5 %: not for that one */
  const bool want = g_tune[GSH_TUNE_STRIP_XCD] == 2 || (g_tune[GSH_TUNE_STRIP_XCD] == 0 && waves_per_simd == 5 && nb >= 64 && topo().eight_xcds());
  if (want && c.grid.x == 1 && by == 1) {
    c.grid.y = (nb + 7u) & ~7u;
    c.xcd_flag = kStripXcdFlag;
  }
  return c;
}
/* ------------------------------------------------------------------ stencil launchers */
/* keep_cols: true = columns 0 / w-1 keep dst's bytes like the reference (the kernel re-writes
 * them unchanged); false = the caller does not care (it copies back the interior only, or zeroes
 * the frame afterwards), which saves one dword load per row in the two edge lanes. */
void launch_sobel(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h, unsigned n, bool keep_cols) {
  if (w < 3 || h < 3 || n == 0) return;
#ifdef GS_EXPERIMENT
  if (g_tune[GSH_TUNE_EXPERIMENT_22] == 1) keep_cols = false; /* probe: without the dst column reads (columns 0 / w-1 then receive junk) */
#endif
  hipStream_t st = ctx().s();
  const size_t fb = (size_t)w * h;
  for_frames(n, [&](unsigned f0, unsigned nn) {
    uint8_t *d = dst + fb * f0;
    const uint8_t *s = src + fb * f0;
    if (!strip_ok(w, h)) {
      GS_LAUNCH(k_sobel_px, grid2d(w, h, nn), dim3(64, 4), 0, st, d, s, w, h, fb);
      return;
    }
    const int rg = strip_mode(w, s);
    const StripCfg c = strip_cfg(w, h - 2, nn, 5, 2, 6, rg);
    with_const<false, true>(keep_cols, [&](auto KEEP) {
      with_const<0, 1, 2>(rg, [&](auto RG) {
        GS_LAUNCH((k_sobel16<GS_CV(KEEP), GS_CV(RG)>), c.grid, c.block, 0, st, d, s, w, h, c.T, fb | c.xcd_flag);
      });
    });
  });
}

template <bool DILATE>
void launch_morph(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h, unsigned n) {
  if (n == 0) return;
  hipStream_t st = ctx().s();
  const size_t fb = (size_t)w * h;
  for_frames(n, [&](unsigned f0, unsigned nn) {
    uint8_t *d = dst + fb * f0;
    const uint8_t *s = src + fb * f0;
    if (!strip_ok(w, h)) {
      GS_LAUNCH(k_morph_px<DILATE>, grid2d(w, h, nn), dim3(64, 4), 0, st, d, s, w, h, fb);
      return;
    }
    const int rg = strip_mode(w, s);
    const StripCfg c = strip_cfg(w, h, nn, 5, 2, 4, rg);
    with_const<0, 1, 2>(rg, [&](auto RG) {
      GS_LAUNCH((k_morph16<DILATE, GS_CV(RG)>), c.grid, c.block, 0, st, d, s, w, h, c.T, fb | c.xcd_flag);
    });
  });
}

/* one pass of radius K = 2..4 (k_morphk.h) over frames that pass strip_ok; the band height of the short-band route is
 * max(kMorphkBandRows[K], 4 K): each band first runs its 2 K halo rows through the horizontal step */
constexpr unsigned kMorphkBandRows[5] = {0, 0, 16, 24, 32};
template <bool DILATE, int K>
void launch_morphk(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h, unsigned n) {
  hipStream_t st = ctx().s();
  const size_t fb = (size_t)w * h;
  for_frames(n, [&](unsigned f0, unsigned nn) {
    uint8_t *d = dst + fb * f0;
    const uint8_t *s = src + fb * f0;
    const int rg = strip_mode(w, s);
    const StripCfg c = strip_cfg(w, h, nn, 5, 2 * K, kMorphkBandRows[K], rg);
    with_const<0, 1, 2>(rg, [&](auto RG) {
      GS_LAUNCH((k_morphk16<DILATE, K, GS_CV(RG)>), c.grid, c.block, 0, st, d, s, w, h, c.T, fb | c.xcd_flag);
    });
  });
}
/* `iterations` applications of the 3x3 operator as ceil(iterations / 4) passes: radius 4 while it fits, then the remainder
 * 1..3 (1 is launch_morph).  The planes alternate so that the last pass writes dst and src is only read:
 * src -> dst -> tmp -> dst ... for an odd pass count, src -> tmp -> dst ... for an even one.  Frames that fail strip_ok
 * take one per-pixel launch of radius `iterations`, src -> dst. */
template <bool DILATE>
void launch_morph_iter(uint8_t *dst, const uint8_t *src, uint8_t *tmp, unsigned w, unsigned h, unsigned n, unsigned iterations) {
  if (n == 0) return;
  const size_t fb = (size_t)w * h;
  if (!strip_ok(w, h)) {
    if (iterations == 1) return launch_morph<DILATE>(dst, src, w, h, n);
    for_frames(n, [&](unsigned f0, unsigned nn) {
      GS_LAUNCH(k_morphr_px<DILATE>, grid2d(w, h, nn), dim3(64, 4), 0, ctx().s(), dst + fb * f0, src + fb * f0, w, h, fb, iterations);
    });
    return;
  }
  const unsigned passes = (iterations + 3u) / 4u;
  if (passes > 1 && !tmp) tmp = (uint8_t *)ctx().scratch(SL_AUX, fb * n);
  const uint8_t *from = src;
  for (unsigned p = 0, left = iterations; p < passes; p++) {
    const unsigned k = left >= 4u ? 4u : left;
    uint8_t *to = ((passes - p) & 1u) ? dst : tmp; /* the last pass (passes - p == 1) writes dst */
    if (k == 1) launch_morph<DILATE>(to, from, w, h, n);
    else with_const<2, 3, 4>(k, [&](auto K) { launch_morphk<DILATE, GS_CV(K)>(to, from, w, h, n); });
    from = to, left -= k;
  }
}

/* which table launch_integral builds, and the k_integral_wave variants that are compiled: 18.  The squares table, streaming
 * loads and wide frames exist at 16 tiles only (the Makefile notes what this kernel already costs hipcc's register
 * allocator). */
enum Table { PLAIN = 0, SQUARES = 1, STREAM = 2 };
template <unsigned TILES, bool RAGGED, bool WIDE, Table TAB> struct IntegralWaveVariant {
  static constexpr bool compiled = TILES == 16u || (TAB == PLAIN && !WIDE);
  static constexpr auto fn() { return k_integral_wave<(int)TILES, RAGGED, WIDE, TAB == SQUARES, TAB == STREAM>; } /* instantiated where called */
};
/* sq: the table of (p - 128)^2 (gs_match_template); only the banded form builds it -- false is returned, and nothing launched,
 * when this geometry would take the rows + columns form */
bool launch_integral(const uint8_t *src, unsigned w, unsigned h, unsigned n, unsigned *ii, bool sq) {
  if (n == 0) return true;
  hipStream_t st = ctx().s();
  const size_t fp = (size_t)w * h;
  /* the banded form takes any width >= 32 at any alignment (round 4: ragged rows, frames wider than 4096 px in column
   * chunks) */
  const bool banded = fp * 4 < 0x7fffffffull && w >= 32;
  if (sq && !banded) return false;
  if (!banded) {
    for_frames(n, [&](unsigned f0, unsigned nn) {
      GS_LAUNCH(k_integral_rows, dim3(h, nn), dim3(256), 0, st, src + fp * f0, w, h, ii + fp * f0);
      GS_LAUNCH(k_integral_cols, dim3((w + 255) / 256, nn), dim3(256), 0, st, ii + fp * f0, w, h);
    });
    return true;
  }
  const bool wide = w > 4096, rg = (w & 3u) != 0u;
  for_frames(n, [&](unsigned f0, unsigned nn) {
    /* bands per frame: ~8 blocks per CU in flight, and for narrow frames no band taller than 32 rows (48 up to 2048 px).
     * A wave of k_integral_wave owns one band and walks it row by row; a 4K row is 16 tiles of arithmetic and 8 waves per
     * CU keep HBM busy, a 612-px row is three, and a large batch of such frames -- 8 bands of 102 rows each -- ran at
     * 2.5 TB/s (256 x 612x816 0.255 ms; with bands of 26 rows and 4-tile waves 0.21; profiles/r06h_integral_ab_tiles_and_band_height.log).
     * Every band costs 12 B per column (its sums: written, scanned, read), which is why wide frames keep tall bands:
     * 64 x 1080p with 64 bands instead of 32 measured 9 % slower. */
    unsigned nb = std::max(1u, 8u * topo().cus / nn);
    if (w <= 1024) nb = std::max(nb, (h + 31u) / 32u);
    else if (w <= 2048) nb = std::max(nb, (h + 47u) / 48u);
    nb = std::min(nb, std::max(1u, h / 8));
    if (wide) nb = std::max(nb, (h + kIntegralWideRows - 1) / kIntegralWideRows); /* a row's carry waits in LDS */
    const unsigned BH = (h + nb - 1) / nb;
    nb = (h + BH - 1) / BH;
    unsigned *cs = (unsigned *)ctx().scratch(SL_HISTP, (size_t)nn * nb * w * 4);
    const uint8_t *s = src + fp * f0;
    unsigned *o = ii + fp * f0;
    /* source planes the Infinity Cache (256 MB, shared with the table being written) cannot keep between the first pass and
     * the third: both read them with streaming loads (k_integral.h).  Same-box A/B of that policy for every batch: 16 x 4096^2
     * (256 MiB) -7 %, 64 x 4K -4 ... -12 %, 64 x 1080p (133 MB) +-0, 8 x 1080p +22 %, 32 x 720p +23 %
     * (profiles/r06i_integral_nt_loads.log, r06j_integral_ab.log).  The plain table of frames wider than 2048 px only --
     * the 16-tile waves -- to keep the instantiations few. */
    const bool beyond_cache = (size_t)nn * fp >= ((size_t)192 << 20) && g_tune[GSH_TUNE_COMPARE] != 8; /* key 6 = 8: default policy for every batch (A/B) */
    const bool nt = !sq && w > 2048 && beyond_cache;
    /* the first pass streams at that size whatever the width (256 x 720p -4 %); from 48 MiB it cost 64 - 75 MiB batches 7-12 %:
     * the third pass then misses the cache for its source (profiles/r06aa_integral_first_pass_nt.log) */
    const bool nt_first = !sq && beyond_cache;
    /* the first pass: three variants, one per table */
    const dim3 gc((w + 4095) / 4096, nb, nn);
    with_const<PLAIN, SQUARES, STREAM>(sq ? SQUARES : (nt || nt_first) ? STREAM : PLAIN, [&](auto TAB) {
      GS_LAUNCH((k_integral_colsum<GS_CV(TAB) == SQUARES, GS_CV(TAB) == STREAM>), gc, dim3(256), 0, st, s, w, h, BH, nb, cs);
    });
    GS_LAUNCH(k_integral_colbase, dim3((w + 63) / 64, nn), dim3(64, 16), 0, st, cs, w, nb);
    const dim3 gw(1, (nb + 3) / 4, nn);
    /* tiles of 256 px per row: the smallest of 2 / 4 / 8 / 16 that spans it (a tile past the row's end still costs its wave scan);
     * the squares table 16 tiles whatever the width: four instantiations instead of six.  (nt and wide imply w > 2048.) */
    const unsigned tiles = (sq || w > 2048) ? 16u : w <= 512 ? 2u : w <= 1024 ? 4u : 8u;
    with_const<2u, 4u, 8u, 16u>(tiles, [&](auto TILES) {
      with_const<false, true>(rg, [&](auto RG) {
        with_const<false, true>(wide, [&](auto WIDE) {
          with_const<PLAIN, SQUARES, STREAM>(sq ? SQUARES : nt ? STREAM : PLAIN, [&](auto TAB) {
            using K = IntegralWaveVariant<GS_CV(TILES), GS_CV(RG), GS_CV(WIDE), GS_CV(TAB)>;
            if constexpr (K::compiled) GS_LAUNCH(K::fn(), gw, dim3(256), 0, st, s, w, h, BH, nb, (const unsigned *)cs, o);
            else GS_ASSERT(!"k_integral_wave: a combination the rule above does not produce");
          });
        });
      });
    });
  });
  return true;
}

/* gs_blur for any radius: register strips for r = 1..3 on aligned frames, otherwise clipped box
 * sums from a scratch integral image (exact: both are u32-modular like the reference). */
template <int MODE>
void launch_box_generic(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h, unsigned n,
                        unsigned radius, int c) {
  hipStream_t st = ctx().s();
  const size_t fp = (size_t)w * h;
  const unsigned r = std::min(radius, std::max(w, h)); /* larger windows clip identically */
  if (g_tune[GSH_TUNE_COMPARE] != 3 && r >= 1 && r <= 127 && w <= 4096 && strip_ok(w, h)) {
    /* sliding box sums straight from the source rows (k_box.h): 3-4 B/px instead of the ~16 of the integral-image
     * route below (64 4K frames: 2.8 ms whatever the radius; this one: r = 16 0.36 ms, r = 40 0.63 ms); the kernel's
     * u16 column sums and LDS halo hold up to r = 127 */
    for_frames(n, [&](unsigned f0, unsigned nn) {
      /* r <= 16: the window's raw rows stay in registers (k_box16r: 2 B/px instead of 3-4; 64 x 4K: 0.22 ms for r <= 9,
       * 0.28 up to 16, against 0.31-0.42 -- profiles/r03r_box_ring.log).  Key 6 = 4: k_box16 always. */
      /* ragged rows: the ring kernel over the whole strips (the last one only feeds its neighbour) + k_box_edge for the
       * last 16 + w % 16 columns in a launch of its own (round 5).  Round 4's RAGGED form of the ring kernels (per-pixel
       * choice between two edge divisors, shifted tail loads inside the block) was no faster than the any-radius kernel --
       * 116-152 registers at r = 4..5 instead of 84-92, one wave per SIMD from r = 12
       * (profiles/r04k_box_ring_ragged_not_kept.log: 3838 x 2160 r = 5 0.446 vs 0.434 ms, r = 16 0.73 vs 0.53). */
      const bool ring = g_tune[GSH_TUNE_COMPARE] != 4 && r <= box_ring_max() && w >= 32 && h >= 2 * r + 1 &&
                        (MODE == 0 || (c > -(1 << 30) && c < (1 << 30)));
      /* band height: the launch should be whole rounds of the blocks the chip holds (256 CUs x 4 of them, fewer for the
       * register-heavy ring kernels of r >= 8 / 10), and a band first loads 2r+1 rows it does not output -- loads and
       * adds only since the vertical-first form, ~0.3 of an output row each.  Pick the band count with the smallest
       * rounds x (T + 0.3 (2r+1)): 64 4K frames -> 16 bands of 135 rows (r = 16: 0.50 -> 0.36 ms, r = 40: 1.11 -> 0.63),
       * 8 frames -> 128 bands (r = 40: 1.0 -> 0.16 ms; profiles/r02l_box_T.log).  Round 1's "at least four window
       * heights per band" dates from a prologue that cost more than the rows it preceded. */
      const unsigned threads = w <= 1024 ? 64u : w <= 2048 ? 128u : 256u; /* a thread owns 16 px of the row */
      const unsigned slots = topo().cus * box_blocks_per_cu(MODE, ring ? r : 0u, threads);
      unsigned T = h;
      if (g_tune[GSH_TUNE_STRIP_BAND_ROWS] > 0) {
        T = (unsigned)g_tune[GSH_TUNE_STRIP_BAND_ROWS];
      } else {
        /* once the launch is several full rounds, more bands only add prologues (cost ~ nn h / slots + nn nbc k / slots
         * grows with nbc), so the search stops at 4 rounds' worth of blocks: at most 4096 candidates however tall
         * the image is; the last answer is kept per (h, nn, r, slots) */
        static thread_local struct { unsigned h, nn, r, slots, T; } memo = {0, 0, 0, 0, 0};
        if (memo.h == h && memo.nn == nn && memo.r == r && memo.slots == slots) {
          T = memo.T;
        } else {
          double best = 1e30;
          const unsigned nbc_max = std::max(1u, std::min(h / 8u, std::max(1u, 4u * slots / nn)));
          for (unsigned nbc = 1; nbc <= nbc_max; nbc++) {
            const unsigned t = (h + nbc - 1) / nbc;
            const double rounds = (double)(((unsigned long long)nn * ((h + t - 1) / t) + slots - 1) / slots);
            const double cost = rounds * ((double)t + (ring ? 0.12 : 0.3) * (2.0 * r + 1.0)); /* ring: 16 VALU per start-up row */
            if (cost < best - 1e-9) best = cost, T = t;
          }
          memo = {h, nn, r, slots, T};
        }
      }
      const unsigned nb = (h + T - 1) / T;
      if (ring && ragged(w)) {
        /* about four waves per SIMD, and bands at least two windows tall (a band starts with 2 r + 1 rows of loads) */
        const unsigned want = std::max(1u, 4u * 4u * topo().cus / nn);
        const int band_rows = g_tune[GSH_TUNE_STRIP_BAND_ROWS];
        const unsigned Te = band_rows > 0 ? (unsigned)band_rows : std::max((h + want - 1) / want, std::min(h, 2u * (2u * r + 1u)));
        const dim3 ge(1, (h + Te - 1) / Te, nn);
        /* The edge launch is a chain of memory latencies (15-30 us however little it computes, growing with the 2 r + 1
         * start-up rows) and touches other columns of dst than the body.  For r >= 12 on large batches it goes to the side
         * stream, ordered behind everything the caller's stream holds so far, and the caller's stream waits for it after the
         * body: it hides under the body launch instead of following it (64 x 3838x2160: r = 16 0.307 -> 0.296 ms, adaptive
         * r = 15 0.308 -> 0.292; r = 5 and 9 are 2 % better off in sequence -- profiles/r05l_box_ragged_buffer_ops.log).
         * Key 6 = 7: always on the side stream. */
        bool side = false;
#ifndef GS_EMU
        side = g_tune[GSH_TUNE_COMPARE] == 7 || (r >= 12u && (size_t)nn * fp >= ((size_t)16 << 20));
        if (side) {
          Ctx &cx = ctx();
          cx.ensure_side();
          GS_HIP(hipEventRecord(cx.ev_chunk[0], st));
          GS_HIP(hipStreamWaitEvent(cx.side, cx.ev_chunk[0], 0));
          launch_box_edge(MODE, ge, cx.side, dst + fp * f0, src + fp * f0, w, h, Te, fp, r, c);
          GS_HIP(hipEventRecord(cx.ev_join, cx.side));
        }
#endif
        launch_box(MODE, r, dim3(1, nb, nn), threads, st, dst + fp * f0, src + fp * f0, w, h, T, fp, r, c);
#ifndef GS_EMU
        if (side) GS_HIP(hipStreamWaitEvent(st, ctx().ev_join, 0));
#endif
        if (!side) launch_box_edge(MODE, ge, st, dst + fp * f0, src + fp * f0, w, h, Te, fp, r, c);
      } else {
        launch_box(MODE, ring ? r : 0u, dim3(1, nb, nn), threads, st, dst + fp * f0, src + fp * f0, w, h, T, fp, r, c);
      }
    });
    return;
  }
  const unsigned group = (unsigned)std::max<size_t>(1, std::min<size_t>(n, (256u << 20) / (fp * 4) + 1));
  unsigned *ii = (unsigned *)ctx().scratch(SL_II, fp * 4 * group);
  for_frames(n, group, [&](unsigned f0, unsigned nn) {
    launch_integral(src + fp * f0, w, h, nn, ii);
    GS_LAUNCH(k_box_px<MODE>, grid2d(w, h, nn), dim3(64, 4), 0, st, dst + fp * f0, src + fp * f0, (const unsigned *)ii, w, h, r, c, fp);
  });
}

void launch_blur(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h, unsigned n,
                 unsigned radius) {
  if (n == 0) return;
  hipStream_t st = ctx().s();
  const size_t fb = (size_t)w * h;
  if (radius >= 1 && radius <= 3 && strip_ok(w, h) && h > 2 * radius && w > 2 * radius) {
    for_frames(n, [&](unsigned f0, unsigned nn) {
      uint8_t *d = dst + fb * f0;
      const uint8_t *s = src + fb * f0;
      const int rg = strip_mode(w, s);
      const StripCfg c = strip_cfg(w, h, nn, 5, radius, radius == 1 ? 4 : radius == 2 ? 6 : 12, rg);
      with_const<1, 2, 3>(radius, [&](auto R) {
        with_const<0, 1, 2>(rg, [&](auto RG) {
          GS_LAUNCH((k_blur16<GS_CV(R), GS_CV(RG)>), c.grid, c.block, 0, st, d, s, w, h, c.T, fb | c.xcd_flag);
        });
      });
      /* the 2*radius vertically clipped rows of each frame get their true divisors */
      GS_LAUNCH(k_blur_edge_rows, dim3((w + 255) / 256, 2 * radius, nn), dim3(256), 0, st, d, s, w, h, (int)radius, fb);
    });
    return;
  }
  if (radius == 0) { /* 1x1 window: identity (sum/1) */
    if (dst != src) GS_HIP(hipMemcpyAsync(dst, src, fb * n, hipMemcpyDeviceToDevice, st));
    return;
  }
  launch_box_generic<0>(dst, src, w, h, n, radius, 0);
}

/* ------------------------------------------------------------------ histogram / otsu / threshold */
/* blocks per frame of k_hist_partial.  A block pays for zeroing and folding its 32 KB of LDS counters and for
 * filling its load queue, so it should run ~64 trips of 16 B per lane (512 4K frames: 4.9 Tpx/s at 31 trips,
 * 5.8 at 63; profiles/r02i_hist.log, r02i_hist_trips.log); a handful of frames is spread over the CUs
 * (256 CUs x 5 resident blocks) down to 16 trips per block, at most 256 blocks per frame for k_hist_reduce. */
constexpr unsigned kHistThreads = 256;
unsigned hist_bpf(size_t frame_bytes, unsigned n) {
  if (g_tune[GSH_TUNE_HIST_BLOCKS] > 0) return (unsigned)g_tune[GSH_TUNE_HIST_BLOCKS];
  const size_t bt = kHistThreads, trips = 64;
  const size_t chunks = frame_bytes / 16 + 1;
  const size_t by_size = (chunks + bt * trips - 1) / (bt * trips);
  const size_t by_fill = std::min<size_t>(std::min<size_t>((5u * topo().cus + n - 1) / n, chunks / (bt * 16)), 256); /* 5 resident blocks per CU */
  return (unsigned)std::max<size_t>(1, std::min<size_t>(std::max(by_size, by_fill), 2048));
}
void launch_hist_partial(dim3 grid, hipStream_t st, const uint8_t *img, size_t frame_bytes, unsigned *partial) {
  /* more bytes than the Infinity Cache keeps (192 MiB and up): streaming loads (k_pointwise.h) */
  with_const<false, true>((size_t)grid.y * grid.z * frame_bytes >= ((size_t)192 << 20), [&](auto NT) {
    GS_LAUNCH((k_hist_partial<kHistThreads, GS_CV(NT)>), grid, dim3(kHistThreads), 0, st, img, frame_bytes, partial);
  });
}
void launch_histogram(const uint8_t *img, size_t frame_bytes, unsigned n, unsigned *hist) {
  if (n == 0) return;
  hipStream_t st = ctx().s();
  /* k_hist_partial addresses a frame with 32-bit offsets: count a huge image in pieces (key 12: piece size in
   * bytes, so that tests reach this path with small images) */
  const size_t piece_bytes = g_tune[GSH_TUNE_HIST_PIECE] > 0 ? (size_t)g_tune[GSH_TUNE_HIST_PIECE] : kHistMaxFrame;
  if (frame_bytes > piece_bytes) {
    const unsigned pieces = (unsigned)(frame_bytes / piece_bytes);
    const size_t rest = frame_bytes - (size_t)pieces * piece_bytes;
    const unsigned bpf = hist_bpf(piece_bytes, pieces), bpr = rest ? hist_bpf(rest, 1) : 0;
    unsigned *partial = (unsigned *)ctx().scratch(SL_HISTP, ((size_t)pieces * bpf + bpr) * 256 * 4);
    for (unsigned f = 0; f < n; f++) {
      const uint8_t *p = img + frame_bytes * f;
      launch_hist_partial(dim3(bpf, pieces), st, p, piece_bytes, partial);
      if (rest)
        launch_hist_partial(dim3(bpr, 1), st, p + (size_t)pieces * piece_bytes, rest, partial + (size_t)pieces * bpf * 256);
      GS_LAUNCH(k_hist_reduce, dim3(1), dim3(256), 0, st, (const unsigned *)partial, pieces * bpf + bpr,
                hist + (size_t)f * 256, 0u);
    }
    return;
  }
  const unsigned bpf = hist_bpf(frame_bytes, n);
  for_frames(n, [&](unsigned f0, unsigned nn) {
    unsigned *partial = (unsigned *)ctx().scratch(SL_HISTP, (size_t)nn * bpf * 256 * 4);
    launch_hist_partial(dim3(bpf, nn), st, img + frame_bytes * f0, frame_bytes, partial);
    GS_LAUNCH(k_hist_reduce, dim3(nn), dim3(256), 0, st, (const unsigned *)partial, bpf, hist + (size_t)f0 * 256, 0u);
  });
}
void launch_threshold(uint8_t *img, size_t frame_bytes, unsigned n, const uint8_t *thr_dev,
                      unsigned thr_const, hipStream_t on = nullptr, int thr_off = 0) {
  if (n == 0) return;
  hipStream_t st = on ? on : ctx().s();
  const size_t chunks = frame_bytes / 16 + 2;
  const unsigned bx = (unsigned)std::max<size_t>(1, std::min<size_t>((chunks + 255) / 256, 2048));
  for_frames(n, [&](unsigned f0, unsigned nn) {
    GS_LAUNCH(k_threshold, dim3(bx, nn), dim3(256), 0, st, img + frame_bytes * f0, frame_bytes, thr_dev ? thr_dev + f0 : nullptr, thr_const,
              thr_off);
  });
}
void launch_otsu(const uint8_t *img, unsigned w, unsigned h, unsigned n, unsigned *hist,
                 uint8_t *thr) {
  launch_histogram(img, (size_t)(w * h), n, hist);
  for_frames(n, [&](unsigned f0, unsigned nn) {
    GS_LAUNCH(k_otsu, dim3(nn), dim3(256), 0, ctx().s(), hist + (size_t)f0 * 256, w * h, thr + f0, (const unsigned *)nullptr, 0u, 0u, (uint8_t *)nullptr, 0);
  });
}

void synth_jump_table(SynthJump &J) {
  auto step = [](uint32_t x) {
    x ^= x << 13;
    x ^= x >> 17;
    x ^= x << 5;
    return x;
  };
  for (int b = 0; b < 32; b++) J.col[0][b] = step(1u << b);
  for (int k = 1; k < 32; k++)
    for (int b = 0; b < 32; b++) {
      uint32_t v = J.col[k - 1][b], r = 0;
      for (int q = 0; q < 32; q++)
        if ((v >> q) & 1u) r ^= J.col[k - 1][q];
      J.col[k][b] = r;
    }
}

void launch_integral_pad(dim3 grid, hipStream_t st, const unsigned *ii, unsigned w, unsigned h, unsigned *padded) {
  GS_LAUNCH(k_integral_pad, grid, dim3(64, 4), 0, st, ii, w, h, padded);
}

/* ---------------------------------------------------------------- geometry: crop, resize, patches (k_resize.h)
 * One kernel family for the batch entries and the drop-in calls (n = 1).
 * k_resize_tile stages a block's source rectangle in LDS where that pays and fits and gathers from global memory where
 * not; the block decides from the window and the rectangle it computes, the launcher only sizes the LDS and the band:
 *   whole frames: more than four source pixels per result pixel (sw sh > 4 dw dh): no LDS, every block gathers (staged
 *     against gathered, ms: 64 x 4K to 640x360 0.228 against 0.044, to 1279x719 0.233 against 0.162, 512 x 612x816 to
 *     300x400 0.264 against 0.241 -- but 64 x 4K to 1920x1080 0.266 against 0.343 and 256 x 720p to 1080p 0.51 against
 *     0.97; profiles/geom_batch.json).  Else the rectangle of 256 columns x `band` rows is at most E(256, sw, dw) x
 *     E(band, sh, dh) source pixels, E(c, s, d) = min(s, ceil(c s / d) + 3): the largest band of 16, 8, 4 rows whose
 *     rectangle fits kResizeLdsSmall (several blocks per CU); else 4 rows if they fit kResizeLdsMax; else no LDS.
 *   windows read on the device (gsh_crop_resize_batch): kResizeLdsSmall and bands of 16 rows; a block whose window is
 *     too large for that gathers.
 * GSH_TUNE_GEOM_FORM = 1 gives no LDS at all (the gather form everywhere), 2 stages whatever the scale wherever the
 * rectangle fits (both for A/B measurements). */
constexpr unsigned kResizeLdsSmall = 16u * 1024u, kResizeLdsMax = 48u * 1024u;
static unsigned resize_extent(unsigned c, unsigned s, unsigned d) {
  return (unsigned)std::min<unsigned long long>(s, ((unsigned long long)c * s + d - 1) / d + 3);
}
struct ResizePlan { unsigned band, lds; };
static ResizePlan resize_plan(unsigned dw, unsigned dh, unsigned sw, unsigned sh, bool windows) {
  ResizePlan pl = {16u, 0u};
  const bool dense = (unsigned long long)sw * sh <= 4ull * dw * dh || g_tune[GSH_TUNE_GEOM_FORM] == 2;
  if (g_tune[GSH_TUNE_GEOM_FORM] != 1 && (windows || dense)) {
    if (windows) {
      pl.lds = kResizeLdsSmall;
    } else {
      const unsigned pitch = (resize_extent(std::min(dw, 256u), sw, dw) + 3u) & ~3u;
      for (unsigned band = 16; band >= 4 && !pl.lds; band >>= 1) {
        const unsigned long long need = (unsigned long long)pitch * resize_extent(std::min(band, dh), sh, dh);
        if (need <= (band > 4 ? kResizeLdsSmall : kResizeLdsMax)) pl.band = band, pl.lds = (unsigned)need;
      }
    }
  }
  if ((dh + pl.band - 1) / pl.band > 65535u) pl.band = (((dh + 65534u) / 65535u) + 3u) & ~3u; /* grid.y; such a block gathers */
  return pl;
}
/* count patches (rois == NULL: the n whole frames) of dw x dh from n frames of sw x sh */
static void launch_resize(uint8_t *dst, unsigned dw, unsigned dh, const uint8_t *src, unsigned sw, unsigned sh, unsigned n,
                          const unsigned *rois, const unsigned *frame_of, unsigned count, bool nearest) {
  const ResizePlan pl = resize_plan(dw, dh, sw, sh, rois != nullptr);
  ResizeArgs a;
  a.dst = dst, a.src = src, a.rois = rois, a.frame_of = frame_of;
  a.dw = dw, a.dh = dh, a.sw = sw, a.sh = sh, a.n = n;
  a.band = pl.band, a.lds = pl.lds, a.any_density = g_tune[GSH_TUNE_GEOM_FORM] == 2 ? 1u : 0u;
  const bool nt = (unsigned long long)dw * dh * count > (256ull << 20); /* beyond the Infinity Cache: streaming stores */
  hipStream_t st = ctx().s();
  for_frames(count, [&](unsigned f0, unsigned nn) {
    const dim3 grid((dw + 255) / 256, (dh + pl.band - 1) / pl.band, nn);
    a.z0 = f0;
    with_const<false, true>(nearest, [&](auto NEAREST) {
      with_const<false, true>(nt, [&](auto NT) { GS_LAUNCH((k_resize_tile<GS_CV(NEAREST), GS_CV(NT)>), grid, dim3(64, 4), pl.lds, st, a); });
    });
  });
}
static void launch_crop(uint8_t *dst, const uint8_t *src, unsigned sw, unsigned sh, unsigned n, struct gs_rect roi) {
  GS_ASSERT(roi.x <= sw && roi.w <= sw - roi.x && roi.y <= sh && roi.h <= sh - roi.y); /* inside the frame, no 32-bit wrap */
  const size_t sfb = (size_t)sw * sh, dfb = (size_t)roi.w * roi.h;
  const bool nt = (unsigned long long)dfb * n > (256ull << 20);
  hipStream_t st = ctx().s();
  for_frames(n, [&](unsigned f0, unsigned nn) {
    const dim3 grid(((roi.w + 15) / 16 + 63) / 64, (roi.h + 3) / 4, nn);
    with_const<false, true>(nt, [&](auto NT) {
      GS_LAUNCH(k_crop_rows<GS_CV(NT)>, grid, dim3(64, 4), 0, st, dst + dfb * f0, src + sfb * f0, sw, sh, roi.x, roi.y, roi.w, roi.h);
    });
  });
}
static bool apart(const uint8_t *a, size_t na, const uint8_t *b, size_t nb) { return a + na <= b || b + nb <= a; }

/* ---- template matching: ONE launcher for gs_match_template (a launch of one frame) and the batch entries ------------------ */
/* the form of k_match_template_mfma for a launch of `frames` frames */
struct TmForm {
  bool split, band;
  unsigned istride;
  size_t lds;
};
static TmForm tm_form(unsigned tw, unsigned th, unsigned rw, unsigned rh, unsigned frames) {
  TmForm f;
  const unsigned nkc = (tw + 31 + 31) / 32;
  /* few 64 x 128 tiles: 32 x 64 tiles, the template rows split over the block's four waves.  The rule counts the blocks of
   * the WHOLE launch, tiles per frame times frames: a 720p frame alone has 120 whole tiles for 256 CUs, five of them fill
   * the chip.  key 20 = 8: 64 x 128 tiles, banded, whatever the size */
  const int key = g_tune[GSH_TUNE_TMATCH];
  f.split = key == 3 || (key != 2 && key != 8 && (unsigned long long)((rw + 127) / 128) * ((rh + 63) / 64) * frames < 512);
  f.istride = (f.split ? 32 : 96) + 32 * nkc + 16;
  /* SPLIT = 1 takes templates taller than a band kTmBand rows at a time (k_tmatch.h BAND: 33 KB of LDS per block instead of 79 at
   * 128 x 128, four blocks per CU); key 20 = 2: the whole template resident, as in round 3 */
  f.band = !f.split && key != 2 && th > kTmBand;
  const unsigned rows = f.band ? kTmBand : th;
  f.lds = std::max<size_t>((size_t)((f.split ? 31 : 63) + rows) * f.istride + (size_t)rows * (32 * nkc + 48) + 16, f.split ? 32768 : 0);
  return f;
}
/* templates of 512 .. 32768 taps, 16 .. 257 wide, whose block fits the LDS: the cross term on the matrix cores (k_tmatch.h;
 * smaller ones are as fast on the dot-product kernels: 1280x720, 16 x 16: 39 vs 47 us).
 * gsh_tune key 20 = 1: the VALU dot-product kernels; 2 / 3: always 64 x 128 tiles / always 32 x 64 tiles with split rows.
 * The route is a property of ONE frame's geometry -- a batch takes, frame by frame, the route gs_match_template takes for a frame
 * of that size; only the tile form looks at the launch (tm_form). */
enum TmRoute { TM_MFMA, TM_DOT, TM_PX };
static TmRoute tm_route(unsigned iw, unsigned ih, unsigned tw, unsigned th) {
  const size_t ib = (size_t)iw * ih, tb = (size_t)tw * th;
  const unsigned nkc = (tw + 31 + 31) / 32;
  const TmForm one = tm_form(tw, th, iw - tw + 1, ih - th + 1, 1);
  const int key = g_tune[GSH_TUNE_TMATCH];
  if (key != 1 && tw >= 16 && nkc <= 9 && th >= 4 && (tb >= 512 || key == 2 || key == 3 || key == 8) && tb <= 32768 &&
      one.lds <= 150 * 1024 && ib < 0x7fffffffull)
    return TM_MFMA;
  return tw <= kTmplTile - 3 ? TM_DOT : TM_PX;
}
/* The batch entries work through their frames in chunks so that the context scratch stays below kTmScratchBudget however
 * many frames a call brings: the matrix-core route keeps a u32 prefix table (ih (iw + 1) entries) and the u32 window sums
 * (rw rh entries) per frame -- 7.2 MB for a 720p frame, 66 MB for a 4K one --, the other routes a result map per frame
 * when they locate.  128 MiB: half the Infinity Cache, so that what one pass of a chunk writes the next still finds there;
 * 18 frames of 720p (about 2000 whole tiles) or two 4K frames (1900).  A frame that alone needs more is a chunk of its own, as it
 * is for gs_match_template.  gsh_tune key 26 caps the frames of a chunk (test hook). */
constexpr size_t kTmScratchBudget = (size_t)128 << 20;
static unsigned tm_chunk_frames(TmRoute route, unsigned iw, unsigned ih, unsigned rw, unsigned rh, unsigned n, bool locate) {
  const size_t per = route == TM_MFMA ? ((size_t)ih * (iw + 1) + (size_t)rw * rh) * 4 : locate ? (size_t)rw * rh : 0;
  size_t c = std::min<size_t>(n, kMaxZ);
  if (per) c = std::min(c, std::max<size_t>(1, kTmScratchBudget / per));
  if (g_tune[GSH_TUNE_TMATCH_CHUNK] > 0) c = std::min<size_t>(c, (size_t)g_tune[GSH_TUNE_TMATCH_CHUNK]);
  return (unsigned)c;
}
/* THE list of the k_match_template_mfma variants, for the launch and for the attribute that lets a variant take more than
 * 64 KB of dynamic LDS: form 0 = 64 x 128 tiles, 1 = 32 x 64 tiles with the template rows split over four waves, 2 = 64 x 128
 * tiles, banded; one instantiation per number of K steps (k_tmatch.h): nkc = 2 .. 9 for templates 16 .. 257 wide */
typedef void (*TmKernel)(TmArgs);
template <class F> static void tm_variant(unsigned form, unsigned nkc, F &&f) {
  with_const<0u, 1u, 2u>(form, [&](auto FORM) {
    with_const<2u, 3u, 4u, 5u, 6u, 7u, 8u, 9u>(nkc, [&](auto NKC) {
      f((TmKernel)k_match_template_mfma<GS_CV(FORM) == 1u ? 4 : 1, GS_CV(NKC), GS_CV(FORM) == 2u>);
    });
  });
}
/* the window sums of (I - 128)^2 of nn frames, rw x rh u32 per frame (SL_PAD; the prefix table they come from: SL_II).  They
 * depend on the template's SIZE only; have: a launch of the same frames and size left them there, nothing is launched. */
static unsigned *tm_window_sums(const uint8_t *s, unsigned iw, unsigned ih, unsigned nn, unsigned tw, unsigned th, bool have) {
  const unsigned rw = iw - tw + 1, rh = ih - th + 1;
  const size_t ib = (size_t)iw * ih, rb = (size_t)rw * rh;
  hipStream_t st = ctx().s();
  unsigned *rowp = (unsigned *)ctx().scratch(SL_II, (size_t)nn * ih * (iw + 1) * 4);
  unsigned *s2 = (unsigned *)ctx().scratch(SL_PAD, (size_t)nn * rb * 4);
  if (have) return s2;
  /* four corners of the banded integral table of squares (round 4) for frames of 4 Mpx and
   * more -- 4K, 128 x 128: 0.269 -> 0.249 ms, 64 x 64: 0.135 -> 0.125; on a 720p frame the four short launches are 6-10 us
   * SLOWER than the two passes of round 3 (row prefix + sliding columns), which stay for small frames, for key 20 = 4 and
   * for geometries the banded integral does not take (key 20 = 5: the table route whatever the size);
   * profiles/r04v_match_template_integral_squares.log */
  if (g_tune[GSH_TUNE_TMATCH] != 4 && (ib >= (4u << 20) || g_tune[GSH_TUNE_TMATCH] == 5) && launch_integral(s, iw, ih, nn, rowp, /*sq=*/true)) {
    GS_LAUNCH(k_tm_s2_corners, dim3((rw + 255) / 256, rh, nn), dim3(256), 0, st, (const unsigned *)rowp, iw, ih, tw, th, rw, rh, s2);
  } else {
    GS_LAUNCH(k_tm_rowprefix, dim3((ih + 3) / 4, 1, nn), dim3(64, 4), 0, st, s, iw, ih, rowp);
    GS_LAUNCH(k_tm_colsq, dim3((rw + 63) / 64, (rh + kTmRun - 1) / kTmRun, nn), dim3(64), 0, st, (const unsigned *)rowp, iw, ih, tw, th,
              rw, rh, s2);
  }
  return s2;
}
/* nn frames (iw x ih, back to back) against one template (ntmpl == 1) or template f for frame f (ntmpl == nn) in one set of
 * launches on the current stream.  d: the nn result maps, rstep bytes apart (0: rw * rh, back to back); d == nullptr (matrix-core
 * route only): the locate epilogue, keys[f] (zeroed, stream-ordered, before this call) receives frame f's best key.
 * have_s2: the call before this one was for these frames and this template size (a loop over a bank, tm_bank). */
static void tm_launch(const uint8_t *s, unsigned iw, unsigned ih, unsigned nn, const uint8_t *t, unsigned tw, unsigned th, unsigned ntmpl,
                      uint8_t *d, unsigned long long *keys, size_t rstep = 0, bool have_s2 = false) {
  const unsigned rw = iw - tw + 1, rh = ih - th + 1;
  const size_t ib = (size_t)iw * ih, tb = (size_t)tw * th, rb = (size_t)rw * rh;
  const TmRoute route = tm_route(iw, ih, tw, th);
  hipStream_t st = ctx().s();
  if (!rstep) rstep = rb;
  if (route == TM_MFMA) {
    TmForm f = tm_form(tw, th, rw, rh, nn);
    if (f.lds > 150 * 1024) f = tm_form(tw, th, rw, rh, 1); /* the form one frame takes fits (tm_route) */
    const bool tm_split = f.split, tm_band = f.band;
    const unsigned nkc = (tw + 31 + 31) / 32, istride = f.istride, tstride = 32 * nkc + 48;
    const size_t tm_lds = f.lds, tpb = (size_t)th * tstride; /* tstride is a multiple of 16 */
    uint8_t *tpad = (uint8_t *)ctx().scratch(SL_PRE, ntmpl * tpb + (size_t)ntmpl * 4 + 16);
    unsigned *tsqp = (unsigned *)(tpad + ((ntmpl * tpb + 3) & ~(size_t)3));
    GS_LAUNCH(k_tm_prep, dim3(ntmpl), dim3(1024), 0, st, t, tw, th, tstride, tpad, tsqp);
    const unsigned *s2 = tm_window_sums(s, iw, ih, nn, tw, th, have_s2);
#ifndef GS_EMU
    /* more than the default 64 KB of dynamic LDS: a per-DEVICE attribute of the function (a thread that moved to
     * another device with gsh_set_device kept a thread-local "done" flag and the launch failed there) */
    static std::atomic<unsigned long long> lds_raised{0};
    const unsigned long long dev_bit = 1ull << ((unsigned)ctx().device & 63u);
    if (ctx().device >= 64 || !(lds_raised.load(std::memory_order_acquire) & dev_bit)) {
      for (unsigned form = 0; form < 3; form++)
        for (unsigned k = 2; k <= 9; k++)
          tm_variant(form, k, [](TmKernel fn) { GS_HIP(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); });
      lds_raised.fetch_or(dev_bit, std::memory_order_release);
    }
#endif
    TmArgs ta{s, iw, ih, (const uint8_t *)tpad, (const unsigned *)tsqp, tw, th, s2, d, rw, rh, nkc, istride, tstride,
              ntmpl > 1 ? (unsigned)tpb : 0u, ntmpl > 1 ? 1u : 0u, keys, rstep};
    const dim3 grid = tm_split ? dim3((rw + 63) / 64, (rh + 31) / 32, nn) : dim3((rw + 127) / 128, (rh + 63) / 64, nn);
    tm_variant(tm_split ? 1u : tm_band ? 2u : 0u, nkc, [&](TmKernel fn) { GS_LAUNCH(fn, grid, dim3(256), tm_lds, st, ta); });
    return;
  }
  GS_ASSERT(d != nullptr); /* the other routes locate through a map (tm_batch) */
  const dim3 g((rw + 63) / 64, (rh + 3) / 4, nn);
  const unsigned tstep = ntmpl > 1 ? (unsigned)tb : 0u;
  if (route == TM_DOT) {
    unsigned long long *tsq = (unsigned long long *)ctx().scratch(SL_PFX, (size_t)ntmpl * 8);
    GS_LAUNCH(k_sum_squares, dim3(ntmpl), dim3(256), 0, st, t, (unsigned long long)tb, tsq);
    const size_t twp = ((size_t)tw + 3) & ~(size_t)3;
    const size_t lds = std::min<size_t>(twp * th, (kTmplTile / twp) * twp);
    /* four results per thread when image rows start 4-byte aligned (see k_match_template4) */
    if (iw % 4 == 0 && ((uintptr_t)s & 3) == 0 && ib < 0x7fffffffull)
      GS_LAUNCH(k_match_template4, dim3((rw + 255) / 256, (rh + 3) / 4, nn), dim3(64, 4), lds, st, s, iw, ih, t, tw, th, tstep,
                (const unsigned long long *)tsq, d, rw, rh, rstep);
    else
      GS_LAUNCH(k_match_template, g, dim3(64, 4), lds, st, s, iw, ih, t, tw, th, tstep, (const unsigned long long *)tsq, d, rw, rh, rstep);
  } else {
    GS_LAUNCH(k_match_template_px, g, dim3(64, 4), 0, st, s, iw, ih, t, tw, th, tstep, d, rw, rh, rstep);
  }
}
/* best / score of n maps of rw x rh from their keys; maps == nullptr: the keys are there already */
static void tm_argmax(const uint8_t *maps, unsigned rw, unsigned rh, unsigned n, unsigned long long *keys) {
  const unsigned long long rb = (unsigned long long)rw * rh;
  for_frames(n, [&](unsigned f0, unsigned nn) {
    GS_LAUNCH(k_argmax_first, dim3((unsigned)((rb + 2047) / 2048), nn), dim3(256), 0, ctx().s(), maps + (size_t)rb * f0, rb,
              (unsigned long long *)nullptr, keys + f0);
  });
}
/* gsh_match_template_batch (result != nullptr) and gsh_locate_template_batch (best != nullptr) */
static void tm_batch(const uint8_t *img, unsigned iw, unsigned ih, unsigned n, const uint8_t *tmpl, unsigned tw, unsigned th, unsigned ntmpl,
                     uint8_t *result, struct gs_point *best, uint8_t *score) {
  if (n == 0) return;
  GS_ASSERT(img && iw > 0 && ih > 0 && tmpl && tw > 0 && th > 0 && (result || best));
  GS_ASSERT(iw >= tw && ih >= th);
  GS_ASSERT(ntmpl == 1 || ntmpl == n);
  const unsigned rw = iw - tw + 1, rh = ih - th + 1;
  const size_t ib = (size_t)iw * ih, tb = (size_t)tw * th, rb = (size_t)rw * rh;
  const TmRoute route = tm_route(iw, ih, tw, th);
  const unsigned chunk = tm_chunk_frames(route, iw, ih, rw, rh, n, result == nullptr);
  hipStream_t st = ctx().s();
  unsigned long long *keys = nullptr;
  if (!result) {
    keys = (unsigned long long *)ctx().scratch(SL_BEST, (size_t)n * 8);
    GS_HIP(hipMemsetAsync(keys, 0, (size_t)n * 8, st));
  }
  for_frames(n, chunk, [&](unsigned f0, unsigned nn) {
    const uint8_t *s = img + ib * f0, *t = ntmpl > 1 ? tmpl + tb * f0 : tmpl;
    const unsigned nt = ntmpl > 1 ? nn : 1u;
    if (result) tm_launch(s, iw, ih, nn, t, tw, th, nt, result + rb * f0, nullptr);
    else if (route == TM_MFMA) tm_launch(s, iw, ih, nn, t, tw, th, nt, nullptr, keys + f0);
    else { /* a chunk's maps in scratch, then the batched argmax */
      uint8_t *maps = (uint8_t *)ctx().scratch(SL_OUT, (size_t)nn * rb);
      tm_launch(s, iw, ih, nn, t, tw, th, nt, maps, nullptr);
      tm_argmax(maps, rw, rh, nn, keys + f0);
    }
  });
  if (!result) GS_LAUNCH(k_best_from_keys, dim3((n + 255) / 256), dim3(256), 0, st, (const unsigned long long *)keys, n, rw, (unsigned *)best, score);
}

/* ---- templates inside windows read on the device (k_tmatch_win.h; docs/design/stencils.md 3.6) ---------------------------- */
/* The bands of k_tmatch_windows: at most kTmwBandCols template columns at a time, and as many template rows as keep
 * (31 + rows) image rows and the rows of the template within kTmwLdsPlan.  ipdw: the dwords a lane can touch (8 + the band's
 * dwords), rounded up to 8 mod 16 (the bank rule of k_tmatch_win.h).  The widest band: 72 + 64 dwords a row, 28 rows. */
struct TmWinForm {
  unsigned band_rows, band_cols, ipdw, tpdw;
  size_t lds;
};
static TmWinForm tm_win_form(unsigned tw, unsigned th) {
  TmWinForm f;
  f.band_cols = std::min(tw, kTmwBandCols);
  f.tpdw = (f.band_cols + 3) / 4;
  f.ipdw = f.tpdw + 8;
  f.ipdw += (8 - f.ipdw % 16 + 16) % 16;
  const unsigned plan = kTmwLdsPlan / 4;
  f.band_rows = std::min(th, (plan - (kTmwTile - 1) * f.ipdw) / (f.ipdw + f.tpdw));
  f.lds = ((size_t)(kTmwTile - 1 + f.band_rows) * f.ipdw + (size_t)f.band_rows * f.tpdw) * 4;
  return f;
}
/* gsh_match_template_windows_batch (result != nullptr) and gsh_locate_template_windows_batch (best != nullptr) */
static void tm_windows(const uint8_t *img, unsigned iw, unsigned ih, unsigned n, const uint8_t *tmpl, unsigned tw, unsigned th, unsigned ntmpl,
                       const struct gs_rect *windows_dev, const unsigned *frame_of_dev, unsigned nwin, unsigned max_ww, unsigned max_wh,
                       uint8_t *result, struct gs_point *best, uint8_t *score) {
  GS_ASSERT(img && tmpl && windows_dev);
  GS_ASSERT(iw > 0 && ih > 0 && n > 0 && tw > 0 && th > 0);
  GS_ASSERT(tw <= max_ww && th <= max_wh);
  GS_ASSERT(max_ww <= iw && max_wh <= ih);
  GS_ASSERT(ntmpl == 1 || ntmpl == nwin);
  GS_ASSERT(frame_of_dev != NULL || nwin <= n);
  const unsigned mrw = max_ww - tw + 1, mrh = max_wh - th + 1;
  const TmWinForm f = tm_win_form(tw, th);
  hipStream_t st = ctx().s();
  unsigned long long *keys = nullptr;
  if (!result) {
    keys = (unsigned long long *)ctx().scratch(SL_BEST, (size_t)nwin * 8);
    GS_HIP(hipMemsetAsync(keys, 0, (size_t)nwin * 8, st));
  }
  TmWinArgs a{img, iw, ih, n, tmpl, tw, th, ntmpl > 1 ? (size_t)tw * th : (size_t)0, (const unsigned *)windows_dev, frame_of_dev, 0u, max_ww, max_wh,
              result, (size_t)mrw * mrh, keys, f.band_rows, f.band_cols, f.ipdw, f.tpdw};
  for_frames(nwin, [&](unsigned p0, unsigned nn) {
    a.z0 = p0;
    GS_LAUNCH(k_tmatch_windows, dim3((mrw + kTmwTile - 1) / kTmwTile, (mrh + kTmwTile - 1) / kTmwTile, nn), dim3(64, 4), f.lds, st, a);
  });
  if (!result)
    GS_LAUNCH(k_tmw_best, dim3((nwin + 255) / 256), dim3(256), 0, st, (const unsigned long long *)keys, (const unsigned *)windows_dev, frame_of_dev,
              nwin, tw, th, max_ww, max_wh, iw, ih, n, (unsigned *)best, score);
}

/* ---- a bank of m templates of one size against every frame (k_tmatch.h: k_match_bank_mfma) ------------------------------------ */
struct TmBankForm {
  bool valid;
  unsigned nt, ngroups, rb, band, istride, tstride;
  size_t lds;
};
/* The bank kernel takes templates up to 512 wide (32 slots of 16 bytes a row) of at most 32768 taps on frames below 2^31
 * bytes.  Rows per band: as many as give 32 slots, an even number where it can be (an odd number of slots ends in a zero
 * slot).  LDS: 38 KB at 16 x 16 and 64 templates, 40 KB at the widest. */
static TmBankForm tm_bank_form(unsigned iw, unsigned ih, unsigned tw, unsigned th, unsigned m) {
  TmBankForm f;
  const unsigned spr = (tw + 15) / 16, rh = ih - th + 1;
  f.rb = 16 * spr;
  f.nt = m > 32 ? 2 : 1;
  f.ngroups = (m + 32 * f.nt - 1) / (32 * f.nt);
  f.valid = spr <= 32 && (size_t)tw * th <= 32768 && (size_t)iw * ih < 0x7fffffffull && (rh + 7) / 8 <= 65535 && f.ngroups <= 65535;
  f.band = std::max(1u, 32 / std::max(1u, std::min(spr, 32u)));
  if (f.band >= 2) f.band &= ~1u;
  f.band = std::min(f.band, th);
  const unsigned ns2 = (f.band * spr + 1) & ~1u;
  f.tstride = (ns2 + 1) * 16, f.istride = 64 + f.rb + 16;
  f.lds = std::max<size_t>((size_t)(8 + f.band) * f.istride + (size_t)32 * f.nt * f.tstride, 2048 * f.nt);
  return f;
}
/* gsh_tune key 27: 1 the loop over the templates whatever the bank, 2 the bank kernel wherever it is valid; 0: by the
 * measurement of docs/design/stencils.md 3.5 (profiles/tmatch_bank.json; 32 frames of 720p).  Where one template takes the
 * dot-product kernels (16 x 16: the loop gains nothing from shared window sums) the bank kernel wins from 4 templates (x 0.63;
 * 2: x 1.1); where it takes the matrix cores (32 x 32) the loop with the window sums computed once wins up to 8 templates
 * (0.99 against 1.49 ms) and the bank kernel from 16 (1.71 against 1.82 ms, locate 1.89 against 2.99). */
constexpr unsigned kTmBankLeastDot = 4, kTmBankLeastMfma = 16;
/* gsh_match_templates_batch (result != nullptr) and gsh_locate_templates_batch (best != nullptr).  The keys of the locate form
 * lie template-major, keys[t * n + f], so that a trip of the loop -- one template against a chunk's frames -- fills a run of them */
static void tm_bank(const uint8_t *img, unsigned iw, unsigned ih, unsigned n, const uint8_t *tmpl, unsigned tw, unsigned th, unsigned m,
                    uint8_t *result, struct gs_point *best, uint8_t *score, unsigned *winner) {
  if (n == 0 || m == 0) return;
  GS_ASSERT(img && iw > 0 && ih > 0 && tmpl && tw > 0 && th > 0 && (result || best));
  GS_ASSERT(tw <= iw && th <= ih);
  GS_ASSERT((unsigned long long)n * m <= 0x7fffffffull);
  const unsigned rw = iw - tw + 1, rh = ih - th + 1;
  const size_t ib = (size_t)iw * ih, tb = (size_t)tw * th, rb = (size_t)rw * rh;
  const TmRoute route = tm_route(iw, ih, tw, th);
  const TmBankForm bf = tm_bank_form(iw, ih, tw, th, m);
  const int key = g_tune[GSH_TUNE_TMATCH_BANK];
  const bool bank = bf.valid && key != 1 && (key == 2 || m >= (route == TM_MFMA ? kTmBankLeastMfma : kTmBankLeastDot));
  unsigned chunk = tm_chunk_frames(bank ? TM_MFMA : route, iw, ih, rw, rh, n, result == nullptr);
  if (bank) chunk = std::min(chunk, 65535u / bf.ngroups); /* blockIdx.z = frame x template group */
  hipStream_t st = ctx().s();
  unsigned long long *keys = nullptr;
  if (!result) {
    keys = (unsigned long long *)ctx().scratch(SL_BEST, (size_t)n * m * 8);
    GS_HIP(hipMemsetAsync(keys, 0, (size_t)n * m * 8, st));
  }
  uint8_t *bankp = nullptr;
  unsigned *tsqp = nullptr;
  if (bank) {
    const size_t bb = (size_t)m * th * bf.rb; /* a multiple of 16 */
    bankp = (uint8_t *)ctx().scratch(SL_PRE, bb + (size_t)m * 4);
    tsqp = (unsigned *)(bankp + bb);
    GS_LAUNCH(k_tm_bank_prep, dim3(m), dim3(256), 0, st, tmpl, tw, th, bf.rb, bankp, tsqp);
  }
  for_frames(n, chunk, [&](unsigned f0, unsigned nn) {
    const uint8_t *s = img + ib * f0;
    if (bank) {
      const unsigned *s2 = tm_window_sums(s, iw, ih, nn, tw, th, false);
      TmBankArgs ba{s, iw, ih, (const uint8_t *)bankp, (const unsigned *)tsqp, tw, th, m, s2, result ? result + rb * m * f0 : nullptr, rw, rh,
                    bf.rb, bf.band, bf.istride, bf.tstride, bf.ngroups, result ? nullptr : keys + f0, n};
      const dim3 grid((rw + 63) / 64, (rh + 7) / 8, nn * bf.ngroups);
      with_const<1u, 2u>(bf.nt, [&](auto NT) { GS_LAUNCH(k_match_bank_mfma<GS_CV(NT)>, grid, dim3(256), bf.lds, st, ba); });
      return;
    }
    for (unsigned t = 0; t < m; t++) { /* one template against the chunk's frames; the window sums of trip 0 serve the others */
      const uint8_t *tp = tmpl + tb * t;
      if (result) tm_launch(s, iw, ih, nn, tp, tw, th, 1, result + rb * ((size_t)m * f0 + t), nullptr, rb * m, t > 0);
      else if (route == TM_MFMA) tm_launch(s, iw, ih, nn, tp, tw, th, 1, nullptr, keys + (size_t)t * n + f0, 0, t > 0);
      else {
        uint8_t *maps = (uint8_t *)ctx().scratch(SL_OUT, (size_t)nn * rb);
        tm_launch(s, iw, ih, nn, tp, tw, th, 1, maps, nullptr);
        tm_argmax(maps, rw, rh, nn, keys + (size_t)t * n + f0);
      }
    }
  });
  if (!result)
    GS_LAUNCH(k_tm_bank_best, dim3((n * m + 255) / 256), dim3(256), 0, st, (const unsigned long long *)keys, n, m, rw, (unsigned *)best, score, winner);
}

}  // namespace gsi

extern "C" {

#ifdef GS_EXPERIMENT
void gsh_probe_strip_copy(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h, unsigned n) {
  GS_ASSERT(dst && src && w >= 32);
  const StripCfg c = strip_cfg(w, h, n, 5, 2, g_tune[GSH_TUNE_STRIP_BAND_ROWS] > 0 ? (unsigned)g_tune[GSH_TUNE_STRIP_BAND_ROWS] : 8u, ragged(w) ? 1 : 0);
  /* 2: whole strips with the stencils' halo load */
  with_const<0, 1, 2>(g_tune[GSH_TUNE_EXPERIMENT_23] == 1 ? 2 : ragged(w) ? 1 : 0, [&](auto V) {
    GS_LAUNCH((k_strip_copy<GS_CV(V) == 1 ? 1 : 0, GS_CV(V) == 2>), c.grid, c.block, 0, ctx().s(), dst, src, w, h, c.T, (size_t)w * h | c.xcd_flag);
  });
}
#endif
/* ---------------------------------------------------------------- batch: stencils */
void gsh_blur_batch(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h, unsigned n,
                    unsigned radius) {
  GS_ASSERT(dst && src && w > 0 && h > 0);
  launch_blur(dst, src, w, h, n, radius);
}
void gsh_sobel_batch(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h, unsigned n) {
  GS_ASSERT(dst && src && w > 0 && h > 0);
  launch_sobel(dst, src, w, h, n);
}
void gsh_erode_batch(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h, unsigned n) {
  GS_ASSERT(dst && src && w > 0 && h > 0);
  launch_morph<false>(dst, src, w, h, n);
}
void gsh_dilate_batch(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h, unsigned n) {
  GS_ASSERT(dst && src && w > 0 && h > 0);
  launch_morph<true>(dst, src, w, h, n);
}
void gsh_morph_batch(uint8_t *dst, const uint8_t *src, uint8_t *tmp, unsigned w, unsigned h, unsigned n, int dilate,
                     unsigned iterations) {
  GS_ASSERT(dst && src && w > 0 && h > 0);
  GS_ASSERT(iterations >= 1);
  if (n == 0) return;
  const size_t nb = (size_t)w * h * n;
  GS_ASSERT(dst + nb <= src || src + nb <= dst); /* dst is written while src is read */
  if (tmp && iterations > 4) {                   /* the plane between two passes */
    GS_ASSERT(tmp + nb <= dst || dst + nb <= tmp);
    GS_ASSERT(tmp + nb <= src || src + nb <= tmp);
  }
  if (dilate) launch_morph_iter<true>(dst, src, tmp, w, h, n, iterations);
  else launch_morph_iter<false>(dst, src, tmp, w, h, n, iterations);
}

/* ---------------------------------------------------------------- batch: histogram etc. */
void gsh_histogram_batch(const uint8_t *img, unsigned w, unsigned h, unsigned n, unsigned *hist) {
  GS_ASSERT(img && hist && w > 0 && h > 0);
  launch_histogram(img, (size_t)(w * h), n, hist); /* 32-bit product like ref :202 */
}
void gsh_otsu_batch(const uint8_t *img, unsigned w, unsigned h, unsigned n, unsigned *hist_scratch,
                    uint8_t *thr) {
  GS_ASSERT(img && hist_scratch && thr && w > 0 && h > 0);
  launch_otsu(img, w, h, n, hist_scratch, thr);
}
void gsh_threshold_batch(uint8_t *img, unsigned w, unsigned h, unsigned n, uint8_t thresh) {
  GS_ASSERT(img && w > 0 && h > 0);
  launch_threshold(img, (size_t)(w * h), n, nullptr, thresh);
}
void gsh_threshold_batch_dev(uint8_t *img, unsigned w, unsigned h, unsigned n, const uint8_t *thr) {
  GS_ASSERT(img && thr && w > 0 && h > 0);
  launch_threshold(img, (size_t)(w * h), n, thr, 0);
}
/* frame f at (uint8_t)(thr[f] + offset): gs_threshold(tmp, gs_otsu_threshold(tmp) + 10) of nanomagick's scan (ref
 * nanomagick.c:191) with the thresholds still on the device; thr is not modified */
void gsh_threshold_batch_dev_offset(uint8_t *img, unsigned w, unsigned h, unsigned n, const uint8_t *thr, int offset) {
  GS_ASSERT(img && thr && w > 0 && h > 0);
  launch_threshold(img, (size_t)(w * h), n, thr, 0, nullptr, offset);
}
/* gs_blur(radius) then gs_sobel into a zeroed image, per frame, in one pass (the fused kernel of
 * the pipeline without the Otsu / threshold half) */
void gsh_blur_sobel_batch(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h, unsigned n,
                          unsigned radius) {
  GS_ASSERT(dst && src && w > 0 && h > 0);
  if (n == 0) return;
  const size_t fb = (size_t)w * h;
  hipStream_t st = ctx().s();
  if (radius >= 1 && radius <= 3 && strip_ok(w, h) && h >= 3 &&
      h > 2 * radius) {
    for_frames(n, [&](unsigned f0, unsigned nn) {
      const int rg = strip_mode(w, src + fb * f0);
      const StripCfg c = strip_cfg(w, h - 2, nn, 3, 2, 8, rg);
      launch_blur_sobel(radius, dim3(c.grid.x, c.grid.y, nn), c.block, st, dst + fb * f0, src + fb * f0, w, h, c.T, fb, rg);
      GS_LAUNCH(k_zero_frame, dim3((2 * w + 2 * h + 255) / 256, nn), dim3(256), 0, st, dst + fb * f0, w, h, fb);
    });
    return;
  }
  uint8_t *t = (uint8_t *)ctx().scratch(SL_AUX, fb * n);
  launch_blur(t, src, w, h, n, radius);
  GS_HIP(hipMemsetAsync(dst, 0, fb * n, st));
  if (w >= 3 && h >= 3) launch_sobel(dst, t, w, h, n, true);
}
void gsh_edge_pipeline_batch(uint8_t *dst, uint8_t *tmp, const uint8_t *src, unsigned w, unsigned h,
                             unsigned n, unsigned radius, unsigned *hist_scratch, uint8_t *thr) {
  GS_ASSERT(dst && src && hist_scratch && thr && w > 0 && h > 0);
  const size_t fb = (size_t)w * h;
  hipStream_t st = ctx().s();
  /* gs_sobel ran "into a zeroed image": only its 1-px frame is left; frames [f0, f0 + nn) on stream `on` */
  auto zero_frame = [&](hipStream_t on, unsigned f0, unsigned nn) {
    for_frames(f0, nn, kMaxZ, [&](unsigned g0, unsigned m) {
      GS_LAUNCH(k_zero_frame, dim3((2 * w + 2 * h + 255) / 256, m), dim3(256), 0, on, dst + fb * g0, w, h, fb);
    });
  };
  if (!tmp && radius >= 1 && radius <= 3 && strip_ok16(w, h, dst, src) && w >= 32 &&
      h >= 3 && h > 2 * radius) { /* every window is clipped on at most one side per axis */
    /* fused: the blurred image only ever exists in registers (1 R + 1 W per pixel).
     * The fused kernel is VALU-bound (~40 % of HBM peak) and the passes after it HBM-bound with
     * an idle VALU.  A batch larger than kChunkFrames is cut into chunks: the fused kernels run
     * back to back on the caller's stream, each chunk's histogram reduce / Otsu / frame zeroing /
     * threshold pass on a side stream behind one event, i.e. under the next chunk's fused kernel.
     * gsh_tune key 5: frames per chunk (0 = default, negative = never split). */
    const int tune_chunk = g_tune[GSH_TUNE_PIPELINE_CHUNK];
    const unsigned per = tune_chunk < 0 ? n : tune_chunk > 0 ? (unsigned)tune_chunk : kChunkFrames;
    /* chunk sizes: `per` frames each.  (Tapering the tail -- 16, 8, 8 -- so that less of the last
     * threshold pass is exposed measured slower: small fused launches cost more than they hide.) */
    std::vector<unsigned> sizes;
    for (unsigned rem = n; rem; rem -= std::min(rem, per)) sizes.push_back(std::min(rem, per));
    /* band height per chunk size (a smaller chunk needs more bands to fill the chip) */
    auto cfg_for = [&](unsigned nn) { return strip_cfg(w, h - 2, std::min(kMaxZ, nn), 3); /* <= 168 VGPRs: 3 waves per SIMD */ };
    unsigned bpf_max = 0;
    for (unsigned nn : sizes) {
      const StripCfg c = cfg_for(nn);
      bpf_max = std::max(bpf_max, c.grid.x * c.grid.y);
    }
    unsigned *partial = (unsigned *)ctx().scratch(SL_HISTP, (size_t)n * bpf_max * 256 * 4);
    auto run_fused = [&](hipStream_t on, unsigned f0, unsigned nn) {
      const StripCfg c = cfg_for(nn);
      for_frames(f0, nn, kMaxZ, [&](unsigned g0, unsigned m) {
        const dim3 grid(c.grid.x, c.grid.y, m);
        uint8_t *d = dst + fb * g0;
        const uint8_t *sp = src + fb * g0;
        unsigned *pp = partial + (size_t)g0 * bpf_max * 256;
#ifndef GS_EMU
        ctx().prof_mark(0, on);
#endif
        launch_blur_sobel_hist(radius, grid, c.block, on, d, sp, w, h, c.T, fb, pp);
#ifndef GS_EMU
        ctx().prof_mark(1, on);
#endif
      });
    };
    /* Chunks after the first of a chunked call, radius 2 (key 28: -1 never): the coded path.  Chunk 0 runs the byte path
     * above; its k_otsu also leaves every frame's window base b (k_pointwise.h).  The fused launch of chunk i >= 1 writes
     * 4-bit codes of the edge values around the guess of frame j of chunk i - lag (the same position in the chunk: video
     * or tiles change slowly; chunks are `per` frames apart, only the last may be shorter) into a ring of chunk buffers
     * instead of edge bytes into dst, 0.5 B/px.  Behind the chunk's k_otsu, k_expand_codes (k_codes.h) writes the final
     * bytes of the frames whose threshold fell into the window (0.5 R + 1 W: 3 B/px instead of 4), and one launch of the
     * fused kernel's repair mode redoes the others exactly (every block of a frame that hit returns at once).  Guesses
     * come from this call only; thr, hist and dst never depend on them.  No host read-back, no flags in memory: the
     * streams are ordered by events alone. */
    const int tune_codes = g_tune[GSH_TUNE_PIPELINE_CODES];
    const bool chunked = sizes.size() > 1 && sizes.size() <= kMaxChunks;
    const bool coded = chunked && radius == 2 && tune_codes != -1;
    const unsigned lag = tune_codes == -2 ? 2u : tune_codes == -3 ? 1u : kCodeGuessLag;
    const int force = tune_codes > 0 ? tune_codes : 0;
    struct CodeGeom { unsigned lanes, ppb, npairs; size_t cfb; }; /* a frame's code plane (CodePairs, k_strip.h) */
    auto code_geom = [&](const StripCfg &c) {
      CodeGeom g;
      g.lanes = c.grid.x * c.block.x, g.ppb = (c.T + 1) / 2;
      g.npairs = ((h - 2 + c.T - 1) / c.T) * g.ppb;
      g.cfb = (size_t)g.npairs * g.lanes * 16;
      GS_ASSERT(g.cfb < 0x7fffffffull);
      return g;
    };
    uint8_t *guess = nullptr, *ring = nullptr;
    size_t ring_bytes = 0;
    if (coded) {
      for (size_t i = 1; i < sizes.size(); i++) ring_bytes = std::max(ring_bytes, code_geom(cfg_for(sizes[i])).cfb * sizes[i]);
      const size_t gb = ((size_t)n + 255) & ~(size_t)255;
      guess = (uint8_t *)ctx().scratch(SL_CODES, gb + kCodeRing * ring_bytes);
      ring = guess + gb;
    }
    /* the frame whose guess frame f0 of chunk i takes */
    auto guess_from = [&](size_t i, unsigned f0) { return f0 - per * (unsigned)std::min<size_t>(lag, i); };
    auto run_fused_codes = [&](hipStream_t on, size_t i, unsigned f0, unsigned nn) {
      const StripCfg c = cfg_for(nn);
      const CodeGeom cg = code_geom(c);
      uint8_t *buf = ring + (i % kCodeRing) * ring_bytes;
      const uint8_t *gs = guess + guess_from(i, f0);
      for_frames(f0, nn, kMaxZ, [&](unsigned g0, unsigned m) {
#ifndef GS_EMU
        ctx().prof_mark(0, on);
#endif
        launch_blur_sobel_codes(radius, dim3(c.grid.x, c.grid.y, m), c.block, on, src + fb * g0, w, h, c.T, fb,
                                partial + (size_t)g0 * bpf_max * 256, buf + cg.cfb * (g0 - f0), cg.cfb, cg.ppb, gs + (g0 - f0));
#ifndef GS_EMU
        ctx().prof_mark(1, on);
#endif
      });
    };
    auto run_otsu = [&](hipStream_t on, unsigned f0, unsigned nn) {
      const StripCfg c = cfg_for(nn);
      const unsigned bpf = c.grid.x * c.grid.y;
      for_frames(f0, nn, kMaxZ, [&](unsigned g0, unsigned m) {
        const unsigned *pp = partial + (size_t)g0 * bpf_max * 256;
        /* the 2w + 2(h-2) frame pixels are 0 in the result and were not counted by the kernel; the passes behind it
         * wait for this launch only (k_otsu folds the blocks' partial histograms itself) */
        GS_LAUNCH(k_otsu, dim3(m), dim3(256), 0, on, hist_scratch + (size_t)g0 * 256, w * h, thr + g0, pp, bpf,
                  2 * w + 2 * (h - 2), guess ? guess + g0 : (uint8_t *)nullptr, force);
      });
    };
    auto run_expand = [&](hipStream_t on, size_t i, unsigned f0, unsigned nn) {
      const StripCfg c = cfg_for(nn);
      const CodeGeom cg = code_geom(c);
      const uint8_t *buf = ring + (i % kCodeRing) * ring_bytes, *gs = guess + guess_from(i, f0);
      const unsigned waves = cg.npairs * (cg.lanes / 64), bx = std::max(1u, std::min((waves + 3) / 4, 2048u));
      for_frames(f0, nn, kMaxZ, [&](unsigned g0, unsigned m) {
        GS_LAUNCH(k_expand_codes, dim3(bx, m), dim3(256), 0, on, dst + fb * g0, buf + cg.cfb * (g0 - f0), w, h, c.T, fb, cg.cfb, cg.lanes,
                  cg.ppb, cg.npairs, (const uint8_t *)(thr + g0), gs + (g0 - f0));
      });
    };
    /* Once per call, behind the last chunk: the repair launch over all coded frames (per chunk, the all-exit launch and the
     * queue gap behind it took 11 of a chunk's 192 us on the side stream, which was as long as the fused launch it runs
     * under), then their 1-px frames.  Frames with the same guess distance go in one launch: chunks 1 .. lag-1, then the rest */
    auto run_repair = [&](hipStream_t on) {
      size_t i = 1;
      while (i < sizes.size()) {
        size_t j = i < lag ? i + 1 : sizes.size();
        const unsigned f0 = per * (unsigned)i, nn = std::min(n, per * (unsigned)j) - f0;
        const StripCfg c = cfg_for(std::min(nn, per));
        const uint8_t *gs = guess + guess_from(i, f0);
        for_frames(f0, nn, kMaxZ, [&](unsigned g0, unsigned m) {
          launch_blur_sobel_repair(radius, dim3(c.grid.x, c.grid.y, m), c.block, on, dst + fb * g0, src + fb * g0, w, h, c.T, fb,
                                   gs + (g0 - f0), thr + g0);
        });
        i = j;
      }
      zero_frame(on, per, n - per); /* behind the passes that write whole strips, as on the byte path */
    };
    auto run_threshold = [&](hipStream_t on, unsigned f0, unsigned nn) {
      launch_threshold(dst + fb * f0, fb, nn, thr + f0, 0, on);
      /* gs_sobel ran "into a zeroed image": only its 1-px frame is left to zero.  AFTER the threshold pass (which
       * turns whatever the fused kernel left there into 0 / 255): the frame is then 0 either way, and the
       * threshold pass need not wait for this launch. */
      zero_frame(on, f0, nn);
    };
#ifdef GS_EMU
    /* one stream: the coded path chunk after chunk, so that its logic is tested without a GPU; else one launch */
    if (!coded) {
      run_fused(st, 0, n);
      run_otsu(st, 0, n);
      run_threshold(st, 0, n);
      return;
    }
    unsigned f0 = 0;
    for (size_t i = 0; i < sizes.size(); f0 += sizes[i], i++) {
      const unsigned nn = sizes[i];
      if (i == 0) run_fused(st, f0, nn), run_otsu(st, f0, nn), run_threshold(st, f0, nn);
      else run_fused_codes(st, i, f0, nn), run_otsu(st, f0, nn), run_expand(st, i, f0, nn);
    }
    run_repair(st);
#else
    if (!chunked) {
      run_fused(st, 0, n);
      run_otsu(st, 0, n);
      run_threshold(st, 0, n);
      return;
    }
    Ctx &cx = ctx();
    cx.ensure_side();
    if (coded) cx.ensure_code_events(sizes.size());
    unsigned f0 = 0;
    size_t waited = kMaxChunks; /* the chunk whose ev_guess the caller's stream waited for last */
    for (size_t i = 0; i < sizes.size(); f0 += sizes[i], i++) {
      const unsigned nn = sizes[i];
      const bool codes = coded && i >= 1, last = i + 1 == sizes.size();
      if (codes) {
        /* the guesses are written; the same wait covers the code buffer's last reader (kCodeRing, gs_internal.h) */
        const size_t from = i - std::min<size_t>(lag, i);
        if (from != waited) GS_HIP(hipStreamWaitEvent(st, cx.ev_guess[from], 0));
        waited = from;
        run_fused_codes(st, i, f0, nn);
      } else {
        run_fused(st, f0, nn);
      }
      hipStream_t on = cx.side;
      if (last) { /* last chunk: nothing left to hide it under; rejoin the caller's stream */
        GS_HIP(hipEventRecord(cx.ev_join, cx.side));
        GS_HIP(hipStreamWaitEvent(st, cx.ev_join, 0));
        on = st;
      } else {
        GS_HIP(hipEventRecord(cx.ev_chunk[i], st));
        GS_HIP(hipStreamWaitEvent(cx.side, cx.ev_chunk[i], 0));
      }
      run_otsu(on, f0, nn);
      if (coded && !last) GS_HIP(hipEventRecord(cx.ev_guess[i], on));
      if (codes) run_expand(on, i, f0, nn);
      else run_threshold(on, f0, nn);
    }
    if (coded) run_repair(st);
#endif
    return;
  }
  if (!tmp && radius >= 1 && radius <= 3 && strip_ok(w, h) && h >= 3 &&
      h > 2 * radius) {
    /* ragged rows or frames at odd addresses: blur + sobel still in one pass (the fused kernel without its histogram
     * half), the histogram as a pass of its own: 5 B/px moved instead of 4, against 9 for the separate calls */
    gsh_blur_sobel_batch(dst, src, w, h, n, radius);
    launch_otsu(dst, w, h, n, hist_scratch, thr);
    launch_threshold(dst, fb, n, thr, 0);
    return;
  }
  uint8_t *t = tmp ? tmp : (uint8_t *)ctx().scratch(SL_AUX, fb * n);
  launch_blur(t, src, w, h, n, radius);
  /* sobel never writes its 1-px frame (ref :308-309); config 2 runs it into a zeroed image, so
   * only that frame needs zeroing (the interior is overwritten) -- after the sobel launch,
   * which then need not preserve columns 0 / w-1 */
  if (w < 3 || h < 3) GS_HIP(hipMemsetAsync(dst, 0, fb * n, st));
  launch_sobel(dst, t, w, h, n, false);
  if (w >= 3 && h >= 3) zero_frame(st, 0, n);
  launch_otsu(dst, w, h, n, hist_scratch, thr);
  launch_threshold(dst, fb, n, thr, 0);
}

/* ---------------------------------------------------------------- batch: integral + LBP */
void gsh_integral_batch(const uint8_t *src, unsigned w, unsigned h, unsigned n, unsigned *ii) {
  GS_ASSERT(src && ii && w > 0 && h > 0);
  launch_integral(src, w, h, n, ii);
}

/* ---------------------------------------------------------------- batch: "next" rows */
void gsh_adaptive_threshold_batch(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h,
                                  unsigned n, unsigned radius, int c) {
  GS_ASSERT(dst && src && w > 0 && h > 0);
  if (n) launch_box_generic<1>(dst, src, w, h, n, radius, c);
}
void gsh_filter_batch(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h, unsigned n,
                      const int8_t *kernel_host, unsigned kw, unsigned kh, unsigned norm) {
  GS_ASSERT(dst && src && kernel_host && w > 0 && h > 0 && kw > 0 && kh > 0 && norm > 0);
  hipStream_t st = ctx().s();
  int8_t *dk = (int8_t *)ctx().scratch(SL_TAB, (size_t)kw * kh);
  GS_HIP(hipMemcpyAsync(dk, kernel_host, (size_t)kw * kh, hipMemcpyHostToDevice, st));
  ctx().sync(); /* kernel_host may be a temporary */
  const size_t fb = (size_t)w * h;
  /* strip kernel: 3x3, every partial sum within int16 (sum |k| <= 128), norm <= 256 */
  unsigned abs_sum = 0;
  for (unsigned i = 0; i < kw * kh; i++) abs_sum += (unsigned)std::abs((int)kernel_host[i]);
  if (kw == 3 && kh == 3 && abs_sum <= 128 && norm <= 256 && strip_ok(w, h)) {
    FilterK fk;
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) fk.k[r][c] = ((uint32_t)(uint16_t)(int16_t)kernel_host[r * 3 + c]) * 0x10001u;
    fk.mul = (0x1000000u + norm - 1u) / norm;
    fk.cap = std::min(255u * norm, 32767u) * 0x10001u;
    fk.neg_is_255 = norm > 1 ? 0xffffffffu : 0u;
    for_frames(n, [&](unsigned f0, unsigned nn) {
      const int rg = strip_mode(w, src + fb * f0);
      const StripCfg c = strip_cfg(w, h, nn, 6, 2, 8, rg);
      uint8_t *d = dst + fb * f0;
      const uint8_t *s = src + fb * f0;
      const size_t fa = fb | c.xcd_flag;
      with_const<false, true>(norm == 1, [&](auto SHIFT) { /* multiplier 2^24: a shift (k_stencil.h) */
        with_const<0, 1, 2>(rg, [&](auto RG) { GS_LAUNCH((k_filter16<GS_CV(RG), GS_CV(SHIFT)>), c.grid, c.block, 0, st, d, s, w, h, c.T, fa, fk); });
      });
    });
    return;
  }
  for_frames(n, [&](unsigned f0, unsigned nn) {
    GS_LAUNCH(k_filter_px, grid2d(w, h, nn), dim3(64, 4), 0, st, dst + fb * f0, src + fb * f0, w, h, fb, (const int8_t *)dk, kw, kh, norm);
  });
}
void gsh_downsample_batch(uint8_t *dst, const uint8_t *src, unsigned sw, unsigned sh, unsigned n) {
  GS_ASSERT(dst && src && sw > 1 && sh > 1);
  hipStream_t st = ctx().s();
  const size_t sfb = (size_t)sw * sh, dfb = (size_t)(sw / 2) * (sh / 2);
  for_frames(n, [&](unsigned f0, unsigned nn) {
    if (sw >= 16)
      GS_LAUNCH(k_downsample8, dim3(((sw / 2 + 7) / 8 + 63) / 64, (sh / 2 + 3) / 4, nn), dim3(64, 4), 0, st, dst + dfb * f0, src + sfb * f0, sw, sh);
    else GS_LAUNCH(k_downsample_px, grid2d(sw / 2, sh / 2, nn), dim3(64, 4), 0, st, dst + dfb * f0, src + sfb * f0, sw, sh);
  });
}

/* levels 1 .. L-1 of n frames in one launch per kMaxZ frames (k_pyramid); the level rule is the ORB driver's
 * (nanomagick.c:247-260, orb_pyramid_dims) */
void gsh_pyramid_batch(uint8_t *levels_dev, const uint8_t *img_dev, unsigned w, unsigned h, unsigned n, unsigned n_levels) {
  if (n == 0) return;
  GS_ASSERT(levels_dev && img_dev && w > 0 && h > 0);
  unsigned lw[4], lh[4];
  const unsigned L = orb_pyramid_dims(w, h, n_levels, lw, lh);
  if (L <= 1) return;
  hipStream_t st = ctx().s();
  uint8_t *plane[4] = {nullptr, levels_dev, nullptr, nullptr};
  size_t fb[4] = {(size_t)w * h, 0, 0, 0};
  for (unsigned l = 1; l < 4; l++) {
    fb[l] = l < L ? (size_t)lw[l] * lh[l] : 0;
    if (l + 1 < 4) plane[l + 1] = plane[l] + fb[l] * n;
  }
  for_frames(n, [&](unsigned f0, unsigned nn) {
    GS_LAUNCH(k_pyramid, dim3(((w + 15) / 16 + 63) / 64, ((h + 7) / 8 + 3) / 4, nn), dim3(64, 4), 0, st, plane[1] + fb[1] * f0,
              plane[2] + fb[2] * f0, plane[3] + fb[3] * f0, img_dev + fb[0] * f0, w, h, L);
  });
}

void gsh_crop_batch(uint8_t *dst, const uint8_t *src, unsigned sw, unsigned sh, unsigned n, struct gs_rect roi) {
  if (n == 0) return;
  GS_ASSERT(dst && src && sw > 0 && sh > 0 && roi.w > 0 && roi.h > 0);
  GS_ASSERT(roi.x <= sw && roi.w <= sw - roi.x && roi.y <= sh && roi.h <= sh - roi.y); /* ref :155, without the wrap of x + w */
  GS_ASSERT(apart(dst, (size_t)roi.w * roi.h * n, src, (size_t)sw * sh * n));
  launch_crop(dst, src, sw, sh, n, roi);
}
static void resize_batch(uint8_t *dst, unsigned dw, unsigned dh, const uint8_t *src, unsigned sw, unsigned sh, unsigned n,
                         bool nearest) {
  if (n == 0) return;
  GS_ASSERT(dst && src && dw > 0 && dh > 0 && sw > 0 && sh > 0);
  GS_ASSERT(apart(dst, (size_t)dw * dh * n, src, (size_t)sw * sh * n));
  launch_resize(dst, dw, dh, src, sw, sh, n, nullptr, nullptr, n, nearest);
}
void gsh_resize_batch(uint8_t *dst, unsigned dw, unsigned dh, const uint8_t *src, unsigned sw, unsigned sh, unsigned n) {
  resize_batch(dst, dw, dh, src, sw, sh, n, false);
}
void gsh_resize_nn_batch(uint8_t *dst, unsigned dw, unsigned dh, const uint8_t *src, unsigned sw, unsigned sh, unsigned n) {
  resize_batch(dst, dw, dh, src, sw, sh, n, true);
}
void gsh_crop_resize_batch(uint8_t *dst, unsigned dw, unsigned dh, const uint8_t *src, unsigned sw, unsigned sh, unsigned n,
                           const struct gs_rect *rois_dev, const unsigned *frame_of_dev, unsigned npatches, int nearest) {
  if (n == 0 || npatches == 0) return;
  GS_ASSERT(dst && src && rois_dev && dw > 0 && dh > 0 && sw > 0 && sh > 0);
  GS_ASSERT(apart(dst, (size_t)dw * dh * npatches, src, (size_t)sw * sh * n));
  launch_resize(dst, dw, dh, src, sw, sh, n, (const unsigned *)rois_dev, frame_of_dev, npatches, nearest != 0);
}

/* ---- template matching over a batch (ref :705, :726; docs/design/stencils.md) ------------------------------------------ */
void gsh_match_template_batch(const uint8_t *img, unsigned iw, unsigned ih, unsigned n, const uint8_t *tmpl, unsigned tw, unsigned th,
                              unsigned ntmpl, uint8_t *result) {
  if (n == 0) return;
  GS_ASSERT(result != NULL);
  tm_batch(img, iw, ih, n, tmpl, tw, th, ntmpl, result, nullptr, nullptr);
}
void gsh_find_best_match_batch(const uint8_t *result, unsigned rw, unsigned rh, unsigned n, struct gs_point *best, uint8_t *score) {
  if (n == 0) return;
  GS_ASSERT(result && rw > 0 && rh > 0 && best);
  hipStream_t st = ctx().s();
  unsigned long long *keys = (unsigned long long *)ctx().scratch(SL_BEST, (size_t)n * 8);
  GS_HIP(hipMemsetAsync(keys, 0, (size_t)n * 8, st));
  tm_argmax(result, rw, rh, n, keys);
  GS_LAUNCH(k_best_from_keys, dim3((n + 255) / 256), dim3(256), 0, st, (const unsigned long long *)keys, n, rw, (unsigned *)best, score);
}
void gsh_locate_template_batch(const uint8_t *img, unsigned iw, unsigned ih, unsigned n, const uint8_t *tmpl, unsigned tw, unsigned th,
                               unsigned ntmpl, struct gs_point *best, uint8_t *score) {
  if (n == 0) return;
  GS_ASSERT(best != NULL);
  tm_batch(img, iw, ih, n, tmpl, tw, th, ntmpl, nullptr, best, score);
}
void gsh_match_templates_batch(const uint8_t *img, unsigned iw, unsigned ih, unsigned n, const uint8_t *tmpl, unsigned tw, unsigned th,
                               unsigned m, uint8_t *result) {
  if (n == 0 || m == 0) return;
  GS_ASSERT(result != NULL);
  tm_bank(img, iw, ih, n, tmpl, tw, th, m, result, nullptr, nullptr, nullptr);
}
void gsh_locate_templates_batch(const uint8_t *img, unsigned iw, unsigned ih, unsigned n, const uint8_t *tmpl, unsigned tw, unsigned th,
                                unsigned m, struct gs_point *best, uint8_t *score, unsigned *winner) {
  if (n == 0 || m == 0) return;
  GS_ASSERT(best != NULL);
  tm_bank(img, iw, ih, n, tmpl, tw, th, m, nullptr, best, score, winner);
}
void gsh_match_template_windows_batch(const uint8_t *img, unsigned iw, unsigned ih, unsigned n, const uint8_t *tmpl, unsigned tw, unsigned th,
                                      unsigned ntmpl, const struct gs_rect *windows_dev, const unsigned *frame_of_dev, unsigned nwin,
                                      unsigned max_ww, unsigned max_wh, uint8_t *result) {
  if (nwin == 0) return;
  GS_ASSERT(result != NULL);
  tm_windows(img, iw, ih, n, tmpl, tw, th, ntmpl, windows_dev, frame_of_dev, nwin, max_ww, max_wh, result, nullptr, nullptr);
}
void gsh_locate_template_windows_batch(const uint8_t *img, unsigned iw, unsigned ih, unsigned n, const uint8_t *tmpl, unsigned tw, unsigned th,
                                       unsigned ntmpl, const struct gs_rect *windows_dev, const unsigned *frame_of_dev, unsigned nwin,
                                       unsigned max_ww, unsigned max_wh, struct gs_point *best, uint8_t *score) {
  if (nwin == 0) return;
  GS_ASSERT(best != NULL);
  tm_windows(img, iw, ih, n, tmpl, tw, th, ntmpl, windows_dev, frame_of_dev, nwin, max_ww, max_wh, nullptr, best, score);
}
void gsh_search_windows_batch(const struct gs_point *at_dev, unsigned nwin, unsigned bw, unsigned bh, unsigned mx, unsigned my, unsigned iw,
                              unsigned ih, struct gs_rect *windows_dev) {
  if (nwin == 0) return;
  GS_ASSERT(at_dev && windows_dev && bw > 0 && bh > 0 && iw > 0 && ih > 0);
  GS_LAUNCH(k_search_windows, dim3((nwin + 255) / 256), dim3(256), 0, ctx().s(), (const unsigned *)at_dev, nwin, bw, bh, mx, my, iw, ih,
            (unsigned *)windows_dev);
}


/* ---------------------------------------------------------------- synthetic frames, checksums */
void gsh_synth_batch(uint8_t *dst, unsigned w, unsigned h, unsigned n, uint32_t seed0) {
  GS_ASSERT(dst && w > 0 && h > 0);
  if (!n) return;
  hipStream_t st = ctx().s();
  bool &jump_ready = ctx().jump_ready; /* cleared when the scratch is released (shutdown / device switch) */
  SynthJump *dj = (SynthJump *)ctx().scratch(SL_JUMP, sizeof(SynthJump));
  if (!jump_ready) {
    SynthJump J;
    synth_jump_table(J);
    GS_HIP(hipMemcpyAsync(dj, &J, sizeof J, hipMemcpyHostToDevice, st));
    ctx().sync();
    jump_ready = true;
  }
  const unsigned nlev = ((w + 31) / 32) * ((h + 31) / 32);
  const size_t npx = (size_t)w * h;
  for_frames(n, [&](unsigned f0, unsigned nn) {
    uint8_t *lev = (uint8_t *)ctx().scratch(SL_LEV, (size_t)nlev * nn);
    const unsigned per = 256 * kSynthRun;
    GS_LAUNCH(k_synth_levels, dim3((nlev + per - 1) / per, nn), dim3(256), 0, st, lev, nlev, seed0 + f0, (const SynthJump *)dj);
    GS_LAUNCH(k_synth_pixels, dim3((unsigned)((npx + per - 1) / per), nn), dim3(256), 0, st, dst + npx * f0, (const uint8_t *)lev, w, h,
              seed0 + f0, (const SynthJump *)dj);
  });
}
void gsh_checksum_batch(const uint8_t *img, size_t frame_bytes, unsigned n, uint64_t *sums) {
  GS_ASSERT(img && sums && frame_bytes > 0);
  if (!n) return;
  hipStream_t st = ctx().s();
  GS_HIP(hipMemsetAsync(sums, 0, (size_t)n * 8, st));
  const unsigned bx = (unsigned)std::max<size_t>(1, std::min<size_t>((frame_bytes + 4095) / 4096, 256));
  for_frames(n, [&](unsigned f0, unsigned nn) {
    GS_LAUNCH(k_checksum, dim3(bx, nn), dim3(256), 0, st, img + frame_bytes * f0, frame_bytes, (unsigned long long *)sums + f0);
  });
}

/* =====================================================================================
 *              drop-in functions: the reference's own names and signatures
 * ===================================================================================== */

void gs_blur(struct gs_image dst, struct gs_image src, unsigned radius) { /* ref :268 */
  GS_ASSERT(GS_VALID(src) && GS_VALID(dst) && dst.w == src.w && dst.h == src.h);
  image_to_image(dst, src, [&](uint8_t *d, const uint8_t *s) { launch_blur(d, s, src.w, src.h, 1, radius); });
}
void gs_erode(struct gs_image dst, struct gs_image src) { /* ref :303 */
  GS_ASSERT(GS_VALID(dst) && GS_VALID(src) && dst.w == src.w && dst.h == src.h);
  image_to_image(dst, src, [&](uint8_t *d, const uint8_t *s) { launch_morph<false>(d, s, src.w, src.h, 1); });
}
void gs_dilate(struct gs_image dst, struct gs_image src) { /* ref :304 */
  GS_ASSERT(GS_VALID(dst) && GS_VALID(src) && dst.w == src.w && dst.h == src.h);
  image_to_image(dst, src, [&](uint8_t *d, const uint8_t *s) { launch_morph<true>(d, s, src.w, src.h, 1); });
}
void gs_adaptive_threshold(struct gs_image dst, struct gs_image src, unsigned radius, int c) {
  GS_ASSERT(GS_VALID(dst) && GS_VALID(src) && dst.w == src.w && dst.h == src.h); /* ref :232 */
  image_to_image(dst, src, [&](uint8_t *d, const uint8_t *s) { launch_box_generic<1>(d, s, src.w, src.h, 1, radius, c); });
}

void gs_sobel(struct gs_image dst, struct gs_image src) { /* ref :306 */
  GS_ASSERT(GS_VALID(dst) && GS_VALID(src) && dst.w == src.w && dst.h == src.h);
  const unsigned w = src.w, h = src.h;
  if (w < 3 || h < 3) return; /* reference loops are empty */
  const size_t nb = (size_t)w * h;
  const uint8_t *s = stage_in(src.data, nb, SL_IN);
  const Staged<uint8_t> out(dst.data, nb, SL_OUT);
  uint8_t *d = out.dev;
  if (out.host) {
    /* The 1-px frame of dst is never written (ref :308-309).  Rows 0 / h-1 are simply not copied
     * back; columns 0 / w-1 of the other rows are planted into the device copy (2h bytes up) so
     * rows 1..h-2 can come back as ONE contiguous copy (a pitched interior copy is 3x slower). */
    std::vector<uint8_t> cols(2 * (size_t)h);
    for (unsigned y = 1; y + 1 < h; y++) cols[2 * y] = dst.data[(size_t)y * w], cols[2 * y + 1] = dst.data[(size_t)y * w + w - 1];
    uint8_t *dc = (uint8_t *)ctx().scratch(SL_AUX2, 2 * (size_t)h);
    GS_HIP(hipMemcpyAsync(dc, cols.data(), 2 * (size_t)h, hipMemcpyHostToDevice, ctx().s()));
    GS_LAUNCH(k_put_cols, dim3((2 * h + 255) / 256), dim3(256), 0, ctx().s(), d, (const uint8_t *)dc, w, h);
    ctx().sync(); /* cols is a local */
  }
  launch_sobel(d, s, w, h, 1, true);
  if (out.host) GS_HIP(hipMemcpyAsync(dst.data + w, d + w, (size_t)w * (h - 2), hipMemcpyDeviceToHost, ctx().s())); /* the interior rows only */
  finish(out.host);
}

void gs_filter(struct gs_image dst, struct gs_image src, struct gs_image kernel, unsigned norm) {
  GS_ASSERT(GS_VALID(src) && GS_VALID(dst) && dst.w == src.w && dst.h == src.h && norm > 0);
  const size_t kb = (size_t)kernel.w * kernel.h;
  /* ref :260-261: the kernel is read through gs_get, so an invalid kernel contributes nothing */
  std::vector<int8_t> k(std::max<size_t>(1, kb), 0);
  unsigned kw = kernel.w, kh = kernel.h;
  if (GS_VALID(kernel)) {
    if (is_dev(kernel.data)) gsh_download(k.data(), kernel.data, kb);
    else memcpy(k.data(), kernel.data, kb);
  } else {
    kw = kh = 1; /* empty loop in the reference: sum = 0 */
    k[0] = 0;
  }
  image_to_image(dst, src, [&](uint8_t *d, const uint8_t *s) { gsh_filter_batch(d, s, src.w, src.h, 1, k.data(), kw, kh, norm); });
}

void gs_downsample(struct gs_image dst, struct gs_image src) { /* ref :189 */
  GS_ASSERT(GS_VALID(src) && GS_VALID(dst) && dst.w == src.w / 2 && dst.h == src.h / 2);
  image_to_image(dst, src, [&](uint8_t *d, const uint8_t *s) { gsh_downsample_batch(d, s, src.w, src.h, 1); });
}

/* ---- geometry + template matching ------------------------------------------ */
void gs_crop(struct gs_image dst, struct gs_image src, struct gs_rect roi) { /* ref :154 */
  GS_ASSERT(GS_VALID(dst) && GS_VALID(src) && roi.x + roi.w <= src.w && roi.y + roi.h <= src.h &&
            dst.w == roi.w && dst.h == roi.h);
  image_to_image(dst, src, [&](uint8_t *d, const uint8_t *s) {
    if (roi.x <= src.w && roi.w <= src.w - roi.x && roi.y <= src.h && roi.h <= src.h - roi.y)
      launch_crop(d, s, src.w, src.h, 1, roi);
    else /* accepted only because the reference's sums wrap: its gs_get semantics pixel by pixel */
      GS_LAUNCH(k_crop_wrapped, dim3((roi.w + 63) / 64, (roi.h + 3) / 4), dim3(64, 4), 0, ctx().s(), d, s, src.w, src.h, roi.x, roi.y,
                roi.w, roi.h);
  });
}
void gs_copy(struct gs_image dst, struct gs_image src) { /* ref :160 */
  const struct gs_rect all = {0, 0, src.w, src.h};
  gs_crop(dst, src, all);
}
static void resize_common(struct gs_image dst, struct gs_image src, bool nearest) {
  GS_ASSERT(GS_VALID(dst) && GS_VALID(src));
  image_to_image(dst, src, [&](uint8_t *d, const uint8_t *s) { launch_resize(d, dst.w, dst.h, s, src.w, src.h, 1, nullptr, nullptr, 1, nearest); });
}
void gs_resize_nn(struct gs_image dst, struct gs_image src) { resize_common(dst, src, true); } /* ref :164 (asserts nothing there) */
void gs_resize(struct gs_image dst, struct gs_image src) { resize_common(dst, src, false); }   /* ref :171 */
void gs_match_template(struct gs_image img, struct gs_image tmpl, struct gs_image result) { /* ref :705 */
  GS_ASSERT(GS_VALID(img) && GS_VALID(tmpl) && GS_VALID(result));
  GS_ASSERT(img.w >= tmpl.w && img.h >= tmpl.h);
  GS_ASSERT(result.w == img.w - tmpl.w + 1 && result.h == img.h - tmpl.h + 1);
  const size_t ib = (size_t)img.w * img.h, tb = (size_t)tmpl.w * tmpl.h, rb = (size_t)result.w * result.h;
  const uint8_t *s = stage_in(img.data, ib, SL_IN), *t = stage_in(tmpl.data, tb, SL_AUX);
  const Staged<uint8_t> d(result.data, rb, SL_OUT);
  tm_launch(s, img.w, img.h, 1, t, tmpl.w, tmpl.h, 1, d.dev, nullptr); /* the batch launcher with one frame: route and tile form as ever */
  d.done();
}
struct gs_point gs_find_best_match(struct gs_image result) { /* ref :726 */
  GS_ASSERT(GS_VALID(result));
  const unsigned long long n = (unsigned long long)result.w * result.h;
  const uint8_t *s = stage_in(result.data, (size_t)n, SL_IN);
  const unsigned blocks = (unsigned)((n + 2047) / 2048);
  unsigned long long *part = (unsigned long long *)ctx().scratch(SL_PFX, (size_t)blocks * 8);
  GS_LAUNCH(k_argmax_first, dim3(blocks), dim3(256), 0, ctx().s(), s, n, part, (unsigned long long *)nullptr);
  std::vector<unsigned long long> hp(blocks);
  GS_HIP(hipMemcpyAsync(hp.data(), part, (size_t)blocks * 8, hipMemcpyDeviceToHost, ctx().s()));
  ctx().sync();
  unsigned long long best = 0;
  for (unsigned long long k : hp) best = std::max(best, k);
  struct gs_point p = {0, 0};
  if (best >> 32) { /* a zero maximum leaves the reference's initial {0,0} */
    const unsigned idx = 0xffffffffu - (unsigned)(best & 0xffffffffu);
    p.x = idx % result.w, p.y = idx / result.w;
  }
  return p;
}

void gs_histogram(struct gs_image img, unsigned hist[256]) { /* ref :199 */
  GS_ASSERT(GS_VALID(img) && hist != NULL);
  const size_t nb = (size_t)(img.w * img.h);
  const uint8_t *s = stage_in(img.data, nb, SL_IN);
  const Staged<unsigned> dh(hist, 1024, SL_HIST);
  launch_histogram(s, nb, 1, dh.dev);
  dh.done();
}

uint8_t gs_otsu_threshold(struct gs_image img) { /* ref :205 */
  GS_ASSERT(GS_VALID(img));
  const size_t nb = (size_t)(img.w * img.h);
  const uint8_t *s = stage_in(img.data, nb, SL_IN);
  unsigned *dh = (unsigned *)ctx().scratch(SL_HIST, 1024);
  uint8_t *dt = (uint8_t *)ctx().scratch(SL_THR, 16);
  launch_otsu(s, img.w, img.h, 1, dh, dt);
  uint8_t t = 0;
  GS_HIP(hipMemcpyAsync(&t, dt, 1, hipMemcpyDeviceToHost, ctx().s()));
  ctx().sync();
  return t;
}

void gs_threshold(struct gs_image img, uint8_t thresh) { /* ref :225 */
  GS_ASSERT(GS_VALID(img));
  const size_t nb = (size_t)(img.w * img.h);
  const Staged<uint8_t> d(img.data, nb, SL_IN, /*copy_in=*/true);
  launch_threshold(d.dev, nb, 1, nullptr, thresh);
  d.done();
}

void gs_integral(struct gs_image src, unsigned *ii) { /* ref :744 */
  GS_ASSERT(GS_VALID(src) && ii);
  const size_t np = (size_t)src.w * src.h;
  const uint8_t *s = stage_in(src.data, np, SL_IN);
  const Staged<unsigned> d(ii, np * 4, SL_II);
  launch_integral(s, src.w, src.h, 1, d.dev);
  d.done();
}

}  /* extern "C" */
