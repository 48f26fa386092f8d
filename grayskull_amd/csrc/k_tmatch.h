/*
 * k_tmatch.h -- gs_match_template (grayskull.h:705-724) on the matrix cores.
 *
 * The sum of squared differences over a tw x th window is the one dense contraction of this library:
 *   SSD(x, y) = sum I'^2 - 2 sum I' T' + sum T'^2      with I' = I - 128, T' = T - 128 (signed bytes; the shift cancels
 * in I - T).  The cross term is a correlation, and a correlation along x is a matrix product with a Toeplitz matrix:
 *   C[m][n] = sum_k A[m][k] B[k][n],   A[m][k] = I'[y0 + m + j][x0 + k],   B[k][n] = T'[j][k - n]  (0 outside the row)
 * gives C[m][n] = sum_i I'[y0 + m + j][x0 + n + i] T'[j][i], template row j's share of the 32 x 32 results at
 * (x0 + n, y0 + m); summed over j in the MFMA accumulator.  K runs over tw + 31 (the Toeplitz band), in steps of 32:
 * v_mfma_i32_32x32x32_i8, efficiency tw / (32 ceil((tw + 31) / 32)).  A operand of lane (m, g): 16 consecutive image
 * bytes of row y0 + m + j; B operand of lane (n, g): 16 consecutive bytes of the zero-padded template row, starting
 * 32 kc + 16 g - n bytes in -- both straight out of LDS (the image region of the block and the template, both
 * shifted to signed bytes once when they are staged).  A wave owns 32 rows x 64 columns of results (two accumulator
 * tiles: the right tile's A operand at step kc is the left tile's at kc + 1, so each LDS read feeds two MFMAs), a
 * block 2 x 2 waves = 64 x 128 results.
 *   sum I'^2 over the window comes from a row-prefix pass and a sliding column pass (k_tm_rowprefix, k_tm_colsq: u32, exact
 * modulo 2^32 and the window sums themselves are below it while
 * tw th <= 32768, which also keeps |sum I' T'| < 2^31), sum T'^2 comes with the padded template (k_tm_prep).
 * The quotient SSD 255 / (tw th 255^2) is a float estimate made exact by its 64-bit remainder.
 */
#ifndef GS_K_TMATCH_H
#define GS_K_TMATCH_H
#include "prims.h"
#include "k_geom.h" /* wave_max_u64, the key of k_argmax_first */

namespace gs {

/* A FRAME AXIS (gsh_match_template_batch, gsh_locate_template_batch): every kernel here but k_tm_prep takes the frame from
 * blockIdx.z -- frame f's image lies iw * ih bytes, its prefix table pstride, its s2 plane and its result rw * rh entries
 * behind frame f - 1's -- and k_tm_prep prepares template blockIdx.x.  The launcher hands a launch as many frames as its
 * scratch budget allows (gs_stencil.cpp), so a clip of video-sized frames fills the chip with whole 64 x 128 tiles. */

struct TmArgs {
  const uint8_t *img;
  unsigned iw, ih;
  const uint8_t *tpad; /* th rows of tstride bytes: 32 zeros, the row as signed bytes, zeros (k_tm_prep) */
  const unsigned *tsq; /* sum (T - 128)^2 */
  unsigned tw, th;
  const unsigned *s2; /* rh x rw window sums of (I - 128)^2 */
  uint8_t *result;
  unsigned rw, rh;
  unsigned nkc;     /* K steps of 32: ceil((tw + 31) / 32) */
  unsigned istride; /* LDS image row: 96 + 32 nkc bytes + 16 (an odd number of 16-byte slots: conflict-free b128 reads) */
  unsigned tstride; /* template row: 32 zeros, the row, zeros up to 32 nkc + 48 (a multiple of 16) */
  /* frame blockIdx.z: img, s2 and result move on by one frame, tpad by tstep bytes and tsq by sqstep entries (0: one
   * template for every frame; th * tstride and 1: one per frame) */
  unsigned tstep, sqstep;
  /* result == nullptr: the locate epilogue -- no score byte is stored; keys[blockIdx.z] (zeroed before the launch) receives
   * the maximum of score << 32 | ~(ry * rw + rx) over the frame, one 64-bit atomicMax per wave that saw a non-zero score */
  unsigned long long *keys;
  size_t rstep; /* frame f's result map lies f * rstep bytes behind result: rw * rh, or more where other maps lie between */
};

/* the template as the MFMA kernel wants it: th rows of tstride bytes (32 zeros, T ^ 0x80, zeros), and sum (T - 128)^2.
 * One block of 1024 threads per template (a template has at most 32768 taps): block b reads template b (tw * th bytes each)
 * and writes padded template b (th * tstride bytes each) and tsq[b]. */
__global__ __launch_bounds__(1024) void k_tm_prep(const uint8_t *tmpl, unsigned tw, unsigned th, unsigned tstride, uint8_t *tpad,
                                                   unsigned *tsq) {
  __shared__ unsigned part[16];
  tmpl += (size_t)blockIdx.x * tw * th, tpad += (size_t)blockIdx.x * th * tstride, tsq += blockIdx.x;
  const unsigned tid = threadIdx.x, tdw = tstride / 4u, ntd = th * tdw;
  unsigned t2 = 0;
  for (unsigned i = tid; i < ntd; i += 1024u) {
    const unsigned j = i / tdw, q = 4u * (i - j * tdw);
    uint32_t sv = 0;
    for (unsigned b = 0; b < 4; b++)
      if (q + b >= 32u && q + b - 32u < tw) {
        const unsigned t = tmpl[(size_t)j * tw + q + b - 32u];
        const int d = (int)t - 128;
        t2 += (unsigned)(d * d);
        sv |= (t ^ 0x80u) << (8 * b);
      }
    ((uint32_t *)tpad)[i] = sv;
  }
  t2 = wave_sum(t2);
  if ((tid & 63u) == 0) part[tid >> 6] = t2;
  __syncthreads();
  if (tid == 0) {
    unsigned t = 0;
    for (unsigned k = 0; k < 16; k++) t += part[k];
    *tsq = t;
  }
}

/* P[r][x] = sum_{i < x} (I[r][i] - 128)^2 for x = 0 .. iw (iw + 1 entries per row): one wave per row, 16 pixels per lane
 * and pass, a wave scan per pass.  grid (ceil(ih / 4), 1, frames), block (64, 4) */
__global__ __launch_bounds__(256) void k_tm_rowprefix(const uint8_t *img, unsigned iw, unsigned ih, unsigned *P) {
  const unsigned r = blockIdx.x * 4u + threadIdx.y, lane = threadIdx.x;
  if (r >= ih) return; /* whole wave */
  img += (size_t)blockIdx.z * iw * ih, P += (size_t)blockIdx.z * ih * (iw + 1u);
  const uint8_t *row = img + (size_t)r * iw;
  unsigned *o = P + (size_t)r * (iw + 1u);
  unsigned carry = 0;
  if (lane == 0) o[0] = 0;
  auto fetch = [&](unsigned x, uint32_t (&d)[4]) { /* 16 pixels from x (zeros past the row's end) */
    if (x + 16u <= iw) {
#pragma unroll
      for (unsigned q = 0; q < 4; q++) d[q] = load_u32_unaligned(row + x + 4u * q);
    } else {
#pragma unroll
      for (unsigned q = 0; q < 4; q++) d[q] = 0x80808080u; /* 128 - 128 = 0 */
      for (unsigned k = 0; k < 16 && x + k < iw; k++) d[k >> 2] = (d[k >> 2] & ~(0xffu << (8 * (k & 3)))) | ((uint32_t)row[x + k] << (8 * (k & 3)));
    }
  };
  uint32_t nxt[4];
  fetch(lane * 16u, nxt);
  for (unsigned x0 = 0; x0 < iw; x0 += 1024u) { /* wave-uniform; the next pass's pixels are requested before this pass's scan */
    const unsigned x = x0 + lane * 16u;
    const uint32_t cur[4] = {nxt[0], nxt[1], nxt[2], nxt[3]};
    if (x0 + 1024u < iw) fetch(x + 1024u, nxt);
    unsigned loc[16], run = 0;
#pragma unroll
    for (unsigned k = 0; k < 16; k++) {
      const int v = (int)((cur[k >> 2] >> (8 * (k & 3))) & 0xffu) - 128;
      run += (unsigned)(v * v);
      loc[k] = run;
    }
    const unsigned before = carry + wave_incl_scan(run) - run;
    if (x + 16u <= iw) { /* 64 consecutive bytes per lane */
      struct __attribute__((aligned(4))) Q4 { uint32_t a, b, c, d; }; /* one 16-byte store at a 4-byte aligned address */
#pragma unroll
      for (unsigned k = 0; k < 16; k += 4)
        *(Q4 *)(o + x + k + 1u) = Q4{before + loc[k], before + loc[k + 1], before + loc[k + 2], before + loc[k + 3]};
    } else {
#pragma unroll
      for (unsigned k = 0; k < 16; k++)
        if (x + k < iw) o[x + k + 1u] = before + loc[k];
    }
    carry = shfl(before + run, 63);
  }
}
/* s2[y][x] = sum_{j < th} (P[y + j][x + tw] - P[y + j][x]); a thread slides down kTmRun result rows of one column, the rows
 * that enter and leave requested 16 steps at a time.  grid (ceil(rw / 64), ceil(rh / kTmRun), frames), block 64;
 * ih: the rows of a frame's table (the frames' tables lie ih * (iw + 1) entries apart) */
constexpr unsigned kTmRun = 64;
__global__ __launch_bounds__(64) void k_tm_colsq(const unsigned *P, unsigned iw, unsigned ih, unsigned tw, unsigned th, unsigned rw,
                                                 unsigned rh, unsigned *s2) {
  const unsigned x = blockIdx.x * 64u + threadIdx.x, y0 = blockIdx.y * kTmRun;
  if (x >= rw) return;
  const size_t ps = (size_t)iw + 1u;
  P += (size_t)blockIdx.z * ih * ps, s2 += (size_t)blockIdx.z * rw * rh;
  const unsigned last = rh - 1u + th - 1u; /* last image row a window touches */
  auto h = [&](unsigned r) { /* rows past the image only feed results that are not stored */
    const unsigned rr = r <= last ? r : last;
    return P[(size_t)rr * ps + x + tw] - P[(size_t)rr * ps + x];
  };
  unsigned s = 0;
#pragma unroll 16
  for (unsigned j = 0; j < th; j++) s += h(y0 + j);
  s2[(size_t)y0 * rw + x] = s;
  for (unsigned k0 = 1; k0 < kTmRun && y0 + k0 < rh; k0 += 16u) { /* uniform per block */
    unsigned in[16], out[16];
#pragma unroll
    for (unsigned k = 0; k < 16; k++) in[k] = h(y0 + k0 + k + th - 1u), out[k] = h(y0 + k0 + k - 1u);
#pragma unroll
    for (unsigned k = 0; k < 16; k++) {
      s += in[k] - out[k];
      if (k0 + k < kTmRun && y0 + k0 + k < rh) s2[(size_t)(y0 + k0 + k) * rw + x] = s;
    }
  }
}

/* s2 from the integral table Q of (I - 128)^2 (k_integral.h, SQ; round 4): four corners per result, modulo 2^32 like the
 * table -- three short launches for the table and this one instead of the row-prefix + sliding-column passes above, which
 * move 140 MB through a u32 prefix table for a 4K frame (75 us; this route: see DESIGN.md 3).  grid (ceil(rw / 256), rh, frames),
 * block 256; the frames' tables lie iw * ih entries apart, as launch_integral leaves them */
__global__ __launch_bounds__(256) void k_tm_s2_corners(const unsigned *Q, unsigned iw, unsigned ih, unsigned tw, unsigned th, unsigned rw,
                                                      unsigned rh, unsigned *s2) {
  const unsigned x = blockIdx.x * 256u + threadIdx.x, y = blockIdx.y;
  if (x >= rw) return;
  Q += (size_t)blockIdx.z * iw * ih, s2 += (size_t)blockIdx.z * rw * rh;
  const unsigned *lo = Q + (size_t)(y + th - 1u) * iw, *hi = y ? Q + (size_t)(y - 1u) * iw : nullptr;
  unsigned s = lo[x + tw - 1u];
  if (x) s -= lo[x - 1u];
  if (hi) {
    s -= hi[x + tw - 1u];
    if (x) s += hi[x - 1u];
  }
  s2[(size_t)y * rw + x] = s;
}

/* SPLIT = 1: a block's four waves own 2 x 2 tiles of 32 rows x 64 columns (64 x 128 results per block; grid (ceil(rw / 128),
 * ceil(rh / 64))) -- least staging per result, for launches with enough blocks to fill the chip.  SPLIT = 4: the four
 * waves share ONE 32 x 64 tile and take every fourth template row each, their accumulators meet in LDS (grid (ceil(rw / 64),
 * ceil(rh / 32))): 8 x the blocks, for video-sized images where 64 x 128 tiles leave most CUs idle.
 * block 256, dynamic LDS max(irows * istride + th * tstride, SPLIT == 4 ? 32 KB : 0) with irows = (SPLIT == 1 ? 63 : 31) + th */
#ifndef GS_TM_VARIANT
#define GS_TM_VARIANT 0 /* timing experiments (wrong results): 1 no MFMA, 2 no operand loads in the loop, 3 no image staging, 4 no template staging, 5 no epilogue */
#endif
/* NK = a.nkc, the K steps of this template width (2 .. 9: one instantiation each, round 4): the operand registers are sized
 * for it (with arrays for 9 steps whatever the template, a 128-px template ran with 178 registers) and the row loop has no
 * run-time guards -- one basic block per template row, so the next row's LDS reads are scheduled between this row's MFMAs
 * (guards on a run-time nkc cut the loop into a block per MFMA pair) */
/* BAND (SPLIT = 1; round 4): the template is taken kTmBand rows at a time -- per band the block stages the TR - 1 + kTmBand image
 * rows those template rows meet and the band's template rows, between two barriers -- so a block holds 33 KB of LDS at
 * tw = 128 instead of 79 and FOUR blocks (16 waves, four per SIMD) fit a CU instead of two: the kernel is paced by LDS
 * latency under the occupancy its footprint allows.  The rows shared by consecutive bands are staged again
 * (they come from the L2). */
/* The frame axis and the locate epilogue are run-time arguments (TmArgs), wave-uniform, so the batch entries add no
 * instantiation: SPLIT x NK x BAND stays at 24 kernels (docs/design/stencils.md has their registers before and after). */
constexpr unsigned kTmBand = 32;
template <int SPLIT, unsigned NK = 9, bool BAND = false>
__global__ __launch_bounds__(256) void k_match_template_mfma(TmArgs a) {
  static_assert(SPLIT == 1 || !BAND, "the split form keeps the whole template resident");
  GS_DYN_LDS(smem);
  const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  { /* this block's frame (scalar arithmetic on the kernel's arguments) */
    const size_t f = blockIdx.z;
    a.img += f * a.iw * a.ih, a.s2 += f * a.rw * a.rh, a.tpad += f * a.tstep, a.tsq += f * a.sqstep;
    if (a.result) a.result += f * a.rstep;
  }
  constexpr unsigned TR = SPLIT == 1 ? 64u : 32u, TC = SPLIT == 1 ? 128u : 64u;
  const unsigned bx0 = blockIdx.x * TC, by0 = blockIdx.y * TR;
  const unsigned jband = BAND ? kTmBand : a.th; /* template rows resident at a time */
  const unsigned irows = TR - 1u + jband, idw = (a.istride - 16u) / 4u;
  uint8_t *limg = (uint8_t *)smem;
  uint8_t *ltm = limg + (size_t)irows * a.istride;
  const unsigned i16 = idw / 4u; /* idw is a multiple of 8 */
  /* image rows by0 + jc .. + TR - 2 + nj of the block's columns, as signed bytes (bytes outside the image: 0; they only ever
   * meet template zeros or results that are not stored), and template rows jc .. jc + nj - 1 (k_tm_prep's padded form): 16
   * bytes per item, eight items per thread requested before the first is stored (a trip is one memory round trip) */
  auto stage = [&](unsigned jc, unsigned nj) {
    const unsigned nitems = (TR - 1u + nj) * i16;
    for (unsigned base = tid; base < (GS_TM_VARIANT == 3 ? 0u : nitems); base += 2048u) {
      /* four scalar arrays, every index a constant once unrolled: an array of structs written under a condition, or bytes
       * inserted at a run-time index, live in scratch memory with hipcc (144 B per lane and a round trip through it for every
       * staged dword until round 4) */
      uint32_t v0[8], v1[8], v2[8], v3[8];
#pragma unroll
      for (unsigned u = 0; u < 8; u++) {
        const unsigned i = base + 256u * u;
        v0[u] = v1[u] = v2[u] = v3[u] = 0;
        if (i < nitems) {
          const unsigned r = i / i16, c = i - r * i16;
          const unsigned y = by0 + jc + r, x = bx0 + 16u * c;
          if (y < a.ih && x < a.iw) {
            const uint8_t *p = a.img + (size_t)y * a.iw + x;
            if (x + 16u <= a.iw) {
              v0[u] = load_u32_unaligned(p) ^ 0x80808080u, v1[u] = load_u32_unaligned(p + 4) ^ 0x80808080u;
              v2[u] = load_u32_unaligned(p + 8) ^ 0x80808080u, v3[u] = load_u32_unaligned(p + 12) ^ 0x80808080u;
            } else {
              uint32_t d0 = 0, d1 = 0, d2 = 0, d3 = 0;
#pragma unroll
              for (unsigned b = 0; b < 4; b++) {
                if (x + b < a.iw) d0 |= (uint32_t)(p[b] ^ 0x80u) << (8 * b);
                if (x + 4 + b < a.iw) d1 |= (uint32_t)(p[4 + b] ^ 0x80u) << (8 * b);
                if (x + 8 + b < a.iw) d2 |= (uint32_t)(p[8 + b] ^ 0x80u) << (8 * b);
                if (x + 12 + b < a.iw) d3 |= (uint32_t)(p[12 + b] ^ 0x80u) << (8 * b);
              }
              v0[u] = d0, v1[u] = d1, v2[u] = d2, v3[u] = d3;
            }
          }
        }
      }
#pragma unroll
      for (unsigned u = 0; u < 8; u++) {
        const unsigned i = base + 256u * u;
        if (i < nitems) {
          const unsigned r = i / i16, c = i - r * i16;
          *(U4 *)(limg + (size_t)r * a.istride + 16u * c) = U4{v0[u], v1[u], v2[u], v3[u]};
        }
      }
    }
    const unsigned nt16 = nj * a.tstride / 16u; /* tstride is a multiple of 16 */
    const U4 *tsrc = (const U4 *)(a.tpad + (size_t)jc * a.tstride);
    for (unsigned base = tid; base < (GS_TM_VARIANT == 4 ? 0u : nt16); base += 2048u) {
      uint32_t v0[8], v1[8], v2[8], v3[8];
#pragma unroll
      for (unsigned u = 0; u < 8; u++) {
        v0[u] = v1[u] = v2[u] = v3[u] = 0;
        if (base + 256u * u < nt16) {
          const U4 t = tsrc[base + 256u * u];
          v0[u] = t.x, v1[u] = t.y, v2[u] = t.z, v3[u] = t.w;
        }
      }
#pragma unroll
      for (unsigned u = 0; u < 8; u++)
        if (base + 256u * u < nt16) ((U4 *)ltm)[base + 256u * u] = U4{v0[u], v1[u], v2[u], v3[u]};
    }
  };
  const unsigned wy = SPLIT == 1 ? (wave >> 1) * 32u : 0u, wx = SPLIT == 1 ? (wave & 1u) * 64u : 0u, m = lane & 31u, g = lane >> 5;
  const unsigned j0 = SPLIT == 1 ? 0u : wave, jstep = (unsigned)SPLIT;
  int32_t acc0[16], acc1[16];
#pragma unroll
  for (int r = 0; r < 16; r++) acc0[r] = 0, acc1[r] = 0;
  /* Row by row: the NK + 1 image operands and NK template operands of template row j sit in registers (static indices) and
   * the operands of row j + jstep are requested before row j's 2 NK MFMAs are issued.  j counts inside the resident band. */
  constexpr unsigned kTmMaxK = NK; /* == a.nkc (the launcher picks the instantiation) */
  U4 Ac[kTmMaxK + 1], Bc[kTmMaxK], An[kTmMaxK + 1], Bn[kTmMaxK];
  auto load_row = [&](unsigned j, U4 (&A)[kTmMaxK + 1], U4 (&B)[kTmMaxK]) {
    const uint8_t *ar = limg + (wy + m + j) * a.istride + wx + 16u * g;
    const uint8_t *tr = ltm + j * a.tstride;
    const unsigned ob = 16u * g + 32u - m, sh = 8u * (ob & 3u); /* 32 kc keeps the byte phase */
    const uint32_t *tp = (const uint32_t *)(tr + (ob & ~3u));
#pragma unroll
    for (unsigned k = 0; k <= kTmMaxK; k++) A[k] = *(const U4 *)(ar + 32u * k);
#pragma unroll
    for (unsigned k = 0; k < kTmMaxK; k++) {
      const uint32_t d0 = tp[8u * k], d1 = tp[8u * k + 1u], d2 = tp[8u * k + 2u], d3 = tp[8u * k + 3u], d4 = tp[8u * k + 4u];
      B[k] = U4{alignbit(d1, d0, sh), alignbit(d2, d1, sh), alignbit(d3, d2, sh), alignbit(d4, d3, sh)};
    }
  };
  for (unsigned jc = 0; jc < a.th; jc += jband) { /* block-uniform: one trip unless BAND */
    const unsigned nj = a.th - jc < jband ? a.th - jc : jband;
    if (jc) __syncthreads(); /* the previous band's operand reads are done */
    stage(jc, nj);
    __syncthreads();
    if (j0 < nj) { /* wave-uniform */
      load_row(j0, Ac, Bc);
      for (unsigned j = j0; j < nj; j += jstep) {
        /* no branch inside a trip: the last one requests its own row again (and drops it) */
        const unsigned jn = j + jstep < nj ? j + jstep : j;
        if (GS_TM_VARIANT != 2) load_row(jn, An, Bn);
#pragma unroll
        for (unsigned k = 0; k < kTmMaxK; k++) {
#if GS_TM_VARIANT == 1
          acc0[0] += (int)(Ac[k].x ^ Bc[k].x), acc1[0] += (int)(Ac[k + 1].x ^ Bc[k].y);
#else
          mfma_i32_32x32x32_i8(Ac[k], Bc[k], acc0);
          mfma_i32_32x32x32_i8(Ac[k + 1], Bc[k], acc1);
#endif
        }
        if (GS_TM_VARIANT != 2) {
#pragma unroll
          for (unsigned k = 0; k <= kTmMaxK; k++) Ac[k] = An[k];
#pragma unroll
          for (unsigned k = 0; k < kTmMaxK; k++) Bc[k] = Bn[k];
        }
      }
    }
  }
  /* results: register r of lane (n, g) is row (r & 3) + 8 (r >> 2) + 4 g of the tile, column n */
  /* score = floor(SSD 255 / (taps 255^2)) = floor(SSD / (255 taps)); SSD <= 65025 taps < 2^32 for taps <= 32768: a float
   * estimate of the quotient (within 1), exact through its 32-bit remainder */
  const unsigned dv = 255u * a.tw * a.th;
  const float inv = 1.0f / (float)dv;
  const unsigned tsq = *a.tsq;
  auto s2_of = [&](int c, int r) -> unsigned { /* requested for all of a lane's results before the first is used */
    const unsigned x = bx0 + wx + 32u * (unsigned)c + m;
    const unsigned y = by0 + wy + (unsigned)((r & 3) + 8 * (r >> 2)) + 4u * g;
    return (x < a.rw && y < a.rh) ? a.s2[(size_t)y * a.rw + x] : 0u;
  };
  unsigned long long best = 0; /* the locate epilogue's key: the largest score at the lowest raster index of this lane's results */
  auto finish = [&](int c, int r, int d, unsigned s2v) {
    const unsigned x = bx0 + wx + 32u * (unsigned)c + m;
    const unsigned y = by0 + wy + (unsigned)((r & 3) + 8 * (r >> 2)) + 4u * g;
    if (x < a.rw && y < a.rh && (GS_TM_VARIANT != 5 || d == 12345)) {
      const unsigned ssd = s2v + tsq - 2u * (unsigned)d; /* >= 0 and < 2^32: modular arithmetic is exact */
      unsigned q = (unsigned)((float)ssd * inv);
      int rem = (int)(ssd - q * dv); /* |true quotient - q| <= 1, so the remainder fits */
      if (rem < 0) q--;
      else if ((unsigned)rem >= dv) q++;
      const unsigned score = q < 255u ? q : 255u;
      if (a.result) a.result[(size_t)y * a.rw + x] = (uint8_t)(255u - score); /* wave-uniform */
      else {
        const unsigned long long key = ((unsigned long long)(255u - score) << 32) | (0xffffffffu - (y * a.rw + x));
        best = key > best ? key : best;
      }
    }
  };
  if constexpr (SPLIT == 1) {
    unsigned sv[32];
#pragma unroll
    for (int r = 0; r < 16; r++) sv[r] = s2_of(0, r), sv[16 + r] = s2_of(1, r);
#pragma unroll
    for (int r = 0; r < 16; r++) finish(0, r, acc0[r], sv[r]), finish(1, r, acc1[r], sv[16 + r]);
  } else {
    /* the four partial tiles meet in LDS ([wave][32 values][lane], over the image region, which is done with);
     * wave w then finishes values w, w + 4, ... */
    __syncthreads();
    int32_t *red = (int32_t *)smem;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      red[(wave * 32u + (unsigned)r) * 64u + lane] = acc0[r];
      red[(wave * 32u + 16u + (unsigned)r) * 64u + lane] = acc1[r];
    }
    __syncthreads();
    unsigned sv[8];
#pragma unroll
    for (int k = 0; k < 8; k++) sv[k] = s2_of((int)((wave + 4u * (unsigned)k) >> 4), (int)((wave + 4u * (unsigned)k) & 15u));
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const unsigned v = wave + 4u * (unsigned)k; /* 0 .. 31: tile v >> 4, register v & 15 */
      int d = 0;
#pragma unroll
      for (unsigned w = 0; w < 4; w++) d += red[(w * 32u + v) * 64u + lane];
      finish((int)(v >> 4), (int)(v & 15u), d, sv[k]);
    }
  }
  if (!a.result) { /* wave-uniform; every lane of the wave is here.  The maximum over all waves of all blocks is the frame's
                    * first maximum whatever order they arrive in; a wave that saw only zeros leaves the key word alone */
    best = wave_max_u64(best);
    if (lane == 0 && (best >> 32)) atomicMax(a.keys + blockIdx.z, best);
  }
}

/* ---- A BANK of templates (gsh_match_templates_batch, gsh_locate_templates_batch) -------------------------------------------
 * m templates of one size against every frame: the cross term is a real matrix product,
 *   C[t][pos] = sum_k T'_t[k] patch(pos)[k],   M = templates, N = result positions, K = the template's taps,
 * with no structural zeros in either operand.  The K axis runs over the template row by row, every row padded with zeros to
 * rb = 16 ceil(tw / 16) bytes, so a K step of 32 is two 16-byte slots and slot s is 16 consecutive taps of row s / (rb / 16):
 *   A operand of lane (t, g): slot 2 k + g of template t -- one aligned 16-byte LDS read out of the bank;
 *   B operand of lane (n, g): the 16 image bytes that slot meets at position (x0 + n, y): consecutive lanes are one byte apart,
 *     so five dword reads and four v_alignbit, as the B operand of k_match_template_mfma; where the template side is padding
 *     the image side holds whatever lies there.
 * Positions are the N side so that a register of the result is 32 consecutive bytes of ONE map (templates on the N side would
 * scatter 4-byte pieces over 32 maps).  A wave owns 4 result rows x 32 columns for NT x 32 templates (4 NT accumulator tiles:
 * every A operand feeds four MFMAs, every B operand NT), a block 2 x 2 waves = 8 rows x 64 columns; blockIdx.z = frame x
 * template group of 32 NT.  Templates past m in the last group are zero rows whose results go nowhere.
 *   The template's rows are taken `band` at a time (a.band rows = at most 32 slots, so the block's share of the bank stays at
 * 16 NT KB whatever th and m are); a band with an odd number of slots ends with a zero slot.
 *   Epilogue: the arithmetic of k_match_template_mfma's finish, bit for bit.  Locate form: one key word per (frame, template),
 * reduced over the lane's rows, the 32 lanes of a template, the block's four waves, and only then sent -- and not sent at all
 * where the word already holds as much (it only ever grows, so a stale read errs on the side of sending). */
struct TmBankArgs {
  const uint8_t *img;
  unsigned iw, ih;
  const uint8_t *bank; /* m templates of th rows of rb signed bytes, zero padded (k_tm_bank_prep) */
  const unsigned *tsq; /* m sums of (T - 128)^2 */
  unsigned tw, th, m;
  const unsigned *s2; /* per frame rh x rw window sums of (I - 128)^2 */
  uint8_t *result;    /* map (f, t) at result + (f m + t) rw rh; nullptr: the locate epilogue */
  unsigned rw, rh;
  unsigned rb;      /* bytes of a padded template row */
  unsigned band;    /* template rows resident at a time */
  unsigned istride; /* LDS image row: 64 + rb + 16 bytes */
  unsigned tstride; /* LDS bytes of one template's band: an odd number of 16-byte slots (conflict-free b128 reads) */
  unsigned ngroups; /* template groups per frame */
  unsigned long long *keys; /* locate: keys[t * kstride + frame of the launch], zeroed before the launch */
  unsigned kstride;
};

/* template b of the bank as the kernel wants it (th rows of rb bytes: T ^ 0x80, zeros) and sum (T - 128)^2.  grid m, block 256 */
__global__ __launch_bounds__(256) void k_tm_bank_prep(const uint8_t *tmpl, unsigned tw, unsigned th, unsigned rb, uint8_t *bank, unsigned *tsq) {
  __shared__ unsigned part[4];
  tmpl += (size_t)blockIdx.x * tw * th, bank += (size_t)blockIdx.x * th * rb, tsq += blockIdx.x;
  const unsigned tid = threadIdx.x, tdw = rb / 4u, ntd = th * tdw;
  unsigned t2 = 0;
  for (unsigned i = tid; i < ntd; i += 256u) {
    const unsigned j = i / tdw, q = 4u * (i - j * tdw);
    uint32_t sv = 0;
    for (unsigned b = 0; b < 4; b++)
      if (q + b < tw) {
        const unsigned t = tmpl[(size_t)j * tw + q + b];
        const int d = (int)t - 128;
        t2 += (unsigned)(d * d);
        sv |= (t ^ 0x80u) << (8 * b);
      }
    ((uint32_t *)bank)[i] = sv;
  }
  t2 = wave_sum(t2);
  if ((tid & 63u) == 0) part[tid >> 6] = t2;
  __syncthreads();
  if (tid == 0) *tsq = part[0] + part[1] + part[2] + part[3];
}

/* grid (ceil(rw / 64), ceil(rh / 8), frames x a.ngroups), block 256,
 * dynamic LDS max((8 + band) istride + 32 NT tstride, 2048 NT) */
template <unsigned NT>
__global__ __launch_bounds__(256, 2) void k_match_bank_mfma(TmBankArgs a) {
  GS_DYN_LDS(smem);
  const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const unsigned fl = blockIdx.z / a.ngroups, tg0 = (blockIdx.z - fl * a.ngroups) * (32u * NT); /* frame of the launch, first template */
  a.img += (size_t)fl * a.iw * a.ih, a.s2 += (size_t)fl * a.rw * a.rh;
  const unsigned bx0 = blockIdx.x * 64u, by0 = blockIdx.y * 8u;
  const unsigned spr = a.rb / 16u; /* slots per template row */
  uint8_t *limg = (uint8_t *)smem;
  uint8_t *ltm = limg + (size_t)(8u + a.band) * a.istride; /* a multiple of 16 */
  const unsigned idw = a.istride / 4u;
  /* image rows by0 + jc .. + 6 + nj of the block's columns as signed bytes (0 outside the image: such bytes only meet template
   * zeros or results that are not stored) and slots [0, ns2) of rows jc .. of the group's templates (zeros past nj rows, past m) */
  auto stage = [&](unsigned jc, unsigned nj, unsigned ns2) {
    const unsigned nitems = (7u + nj) * idw;
    for (unsigned i = tid; i < nitems; i += 256u) {
      const unsigned r = i / idw, c = i - r * idw;
      const unsigned y = by0 + jc + r, x = bx0 + 4u * c;
      uint32_t v = 0;
      if (y < a.ih && x < a.iw) {
        const uint8_t *p = a.img + (size_t)y * a.iw + x;
        if (x + 4u <= a.iw) v = load_u32_unaligned(p) ^ 0x80808080u;
        else
          for (unsigned b = 0; x + b < a.iw; b++) v |= (uint32_t)(p[b] ^ 0x80u) << (8 * b);
      }
      *(uint32_t *)(limg + (size_t)r * a.istride + 4u * c) = v;
    }
    const unsigned nsl = nj * spr, nt16 = 32u * NT * ns2;
    for (unsigned i = tid; i < nt16; i += 256u) {
      const unsigned tt = i / ns2, sl = i - tt * ns2, t = tg0 + tt;
      uint32_t v0 = 0, v1 = 0, v2 = 0, v3 = 0; /* four scalars: a struct written under a condition lives in scratch memory */
      if (t < a.m && sl < nsl) {
        const U4 v = *(const U4 *)(a.bank + ((size_t)t * a.th + jc) * a.rb + 16u * sl);
        v0 = v.x, v1 = v.y, v2 = v.z, v3 = v.w;
      }
      *(U4 *)(ltm + (size_t)tt * a.tstride + 16u * sl) = U4{v0, v1, v2, v3};
    }
  };
  const unsigned wy = (wave >> 1) * 4u, wx = (wave & 1u) * 32u, n = lane & 31u, g = lane >> 5;
  const unsigned sh = 8u * (n & 3u); /* istride, wx and a slot's column are multiples of 4: the byte phase is the lane's */
  int32_t acc[NT][4][16];
#pragma unroll
  for (unsigned q = 0; q < NT; q++)
#pragma unroll
    for (unsigned p = 0; p < 4; p++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[q][p][r] = 0;
  /* K step k of a band: lane half g takes slot 2 k + g = 16 taps from column c of the band's row j */
  auto load_step = [&](unsigned k, unsigned j, unsigned c, U4 (&A)[NT], U4 (&B)[4]) {
#pragma unroll
    for (unsigned q = 0; q < NT; q++) A[q] = *(const U4 *)(ltm + (size_t)(32u * q + n) * a.tstride + 16u * (2u * k + g));
#pragma unroll
    for (unsigned p = 0; p < 4; p++) {
      const uint32_t *ip = (const uint32_t *)(limg + (size_t)(wy + p + j) * a.istride + ((wx + n + c) & ~3u));
      const uint32_t d0 = ip[0], d1 = ip[1], d2 = ip[2], d3 = ip[3], d4 = ip[4];
      B[p] = U4{alignbit(d1, d0, sh), alignbit(d2, d1, sh), alignbit(d3, d2, sh), alignbit(d4, d3, sh)};
    }
  };
  for (unsigned jc = 0; jc < a.th; jc += a.band) { /* block-uniform */
    const unsigned nj = a.th - jc < a.band ? a.th - jc : a.band;
    const unsigned ns2 = (nj * spr + 1u) & ~1u, nk = ns2 / 2u;
    if (jc) __syncthreads(); /* the previous band's operand reads are done */
    stage(jc, nj, ns2);
    __syncthreads();
    unsigned j = spr == 1u ? g : 0u, c = spr == 1u ? 0u : 16u * g; /* slot g */
    U4 Ac[NT], Bc[4], An[NT], Bn[4];
    load_step(0, j, c, Ac, Bc);
    for (unsigned k = 0; k < nk; k++) {
      /* no branch inside a trip: the last one requests its own operands again (and drops them) */
      unsigned jn = j, cn = c + 32u; /* two slots on: at most two rows on */
      if (cn >= a.rb) cn -= a.rb, jn++;
      if (cn >= a.rb) cn -= a.rb, jn++;
      const bool more = k + 1u < nk;
      jn = more ? jn : j, cn = more ? cn : c;
      load_step(more ? k + 1u : k, jn, cn, An, Bn);
#pragma unroll
      for (unsigned q = 0; q < NT; q++)
#pragma unroll
        for (unsigned p = 0; p < 4; p++) mfma_i32_32x32x32_i8(Ac[q], Bc[p], acc[q][p]);
#pragma unroll
      for (unsigned q = 0; q < NT; q++) Ac[q] = An[q];
#pragma unroll
      for (unsigned p = 0; p < 4; p++) Bc[p] = Bn[p];
      j = jn, c = cn;
    }
  }
  /* results: register r of lane (n, g) of tile (q, p) is template tg0 + 32 q + (r & 3) + 8 (r >> 2) + 4 g at position
   * (bx0 + wx + n, by0 + wy + p); score = floor(SSD / (255 taps)) as in k_match_template_mfma */
  const unsigned dv = 255u * a.tw * a.th;
  const float inv = 1.0f / (float)dv;
  const unsigned x = bx0 + wx + n;
  const size_t rbm = (size_t)a.rw * a.rh;
  unsigned sv[4];
#pragma unroll
  for (unsigned p = 0; p < 4; p++) sv[p] = (x < a.rw && by0 + wy + p < a.rh) ? a.s2[(size_t)(by0 + wy + p) * a.rw + x] : 0u;
  unsigned long long *red = (unsigned long long *)smem; /* locate: [wave][32 NT templates], over the image rows */
  if (!a.result) __syncthreads();                       /* block-uniform: every wave is done with the operands */
#pragma unroll
  for (unsigned q = 0; q < NT; q++) {
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const unsigned tl = 32u * q + (unsigned)((r & 3) + 8 * (r >> 2)) + 4u * g, t = tg0 + tl;
      const unsigned tsq = t < a.m ? a.tsq[t] : 0u;
      unsigned long long best = 0; /* the largest score at the lowest raster index of this lane's four results */
#pragma unroll
      for (unsigned p = 0; p < 4; p++) {
        const unsigned y = by0 + wy + p;
        if (t < a.m && x < a.rw && y < a.rh) {
          const unsigned ssd = sv[p] + tsq - 2u * (unsigned)acc[q][p][r]; /* >= 0 and < 2^32: modular arithmetic is exact */
          unsigned qq = (unsigned)((float)ssd * inv);
          const int rem = (int)(ssd - qq * dv); /* |true quotient - qq| <= 1, so the remainder fits */
          if (rem < 0) qq--;
          else if ((unsigned)rem >= dv) qq++;
          const unsigned score = qq < 255u ? qq : 255u;
          if (a.result) a.result[((size_t)fl * a.m + t) * rbm + (size_t)y * a.rw + x] = (uint8_t)(255u - score); /* block-uniform */
          else {
            const unsigned long long key = ((unsigned long long)(255u - score) << 32) | (0xffffffffu - (y * a.rw + x));
            best = key > best ? key : best;
          }
        }
      }
      if (!a.result) { /* every lane of the wave is here: the 32 lanes of a half hold one template */
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) {
          const uint32_t lo = shfl((uint32_t)best, (int)(lane ^ (unsigned)d)), hi = shfl((uint32_t)(best >> 32), (int)(lane ^ (unsigned)d));
          const unsigned long long o = ((unsigned long long)hi << 32) | lo;
          best = o > best ? o : best;
        }
        if (n == 0) red[wave * (32u * NT) + tl] = best;
      }
    }
  }
  if (!a.result) {
    __syncthreads();
    if (tid < 32u * NT && tg0 + tid < a.m) {
      unsigned long long best = red[tid];
#pragma unroll
      for (unsigned w = 1; w < 4; w++) best = red[w * (32u * NT) + tid] > best ? red[w * (32u * NT) + tid] : best;
      unsigned long long *word = a.keys + (size_t)(tg0 + tid) * a.kstride + fl;
      /* the maximum over all blocks is the map's first maximum whatever order they arrive in; a block that saw only zeros, or
       * no more than the word holds, leaves it alone */
      if ((best >> 32) && best > *(volatile unsigned long long *)word) atomicMax(word, best);
    }
  }
}

/* keys[t * n + f] (value << 32 | ~(y * rw + x); 0 in the high half: no non-zero value seen) -> best[f * m + t] = {x, y},
 * score[f * m + t] (may be NULL) and winner[f] (may be NULL): the template with the highest score, the lowest index on ties.
 * grid ceil(n m / 256), block 256 */
__global__ __launch_bounds__(256) void k_tm_bank_best(const unsigned long long *keys, unsigned n, unsigned m, unsigned rw, unsigned *best,
                                                      uint8_t *score, unsigned *winner) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n * m) return;
  const unsigned f = i / m, t = i - f * m;
  const unsigned long long key = keys[(size_t)t * n + f];
  const unsigned v = (unsigned)(key >> 32), idx = 0xffffffffu - (unsigned)key;
  best[2u * i] = v ? idx % rw : 0u, best[2u * i + 1u] = v ? idx / rw : 0u;
  if (score) score[i] = (uint8_t)v;
  if (winner && i < n) { /* frame i */
    unsigned w = 0, top = 0;
    for (unsigned k = 0; k < m; k++) {
      const unsigned s = (unsigned)(keys[(size_t)k * n + i] >> 32);
      if (s > top) top = s, w = k;
    }
    winner[i] = w;
  }
}

}  // namespace gs
#endif
