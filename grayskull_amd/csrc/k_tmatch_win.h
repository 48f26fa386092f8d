/*
 * k_tmatch_win.h -- gs_find_best_match(gs_match_template(gs_crop(frame, window), tmpl)) (ref grayskull.h:154, :705, :725)
 * for windows read on the device: gsh_match_template_windows_batch, gsh_locate_template_windows_batch, and the glue that
 * makes a tracker of them, gsh_search_windows_batch.  docs/design/stencils.md 3.6.
 *
 * A window's rows lie iw bytes apart and start at any byte, so no pointer offset makes the whole-frame kernels
 * (k_geom.h, k_tmatch.h) search one: they have no row stride.  k_tmatch_windows stages what a tile of results needs in
 * LDS and runs the sum of squared differences from there,
 *   SSD = sum I^2 + sum T^2 - 2 sum I T     on v_dot4_u32_u8, as k_match_template4 does from global memory.
 *
 * grid (ceil(mrw / 32), ceil(mrh / 32), windows of the launch) with mrw x mrh = (max_ww - tw + 1) x (max_wh - th + 1), the
 * largest map a window of the call can have; block (64, 4).  A block reads its window and frame index (wave-uniform),
 * leaves where the window is not valid (tmw_valid) or its 32 x 32 tile lies outside the window's own rw x rh map.
 * Lane l of wave v owns the four adjacent results (4 (l & 7) .. + 3, 8 v + (l >> 3)) of the tile.
 *
 * The template is walked in BANDS of band_rows rows x band_cols columns (band_cols a multiple of 4, at most 256) chosen
 * by the launcher so that a block's LDS stays within kTmwLdsPlan whatever the template's size; a template that fits is
 * one band.  Per band, between two barriers:
 *   image   31 + nj rows (nj: the band's rows) of 8 + ceil(ni / 4) dwords (ni: the band's columns), row r = frame row
 *           wy + by0 + j0 + r from column wx + bx0 + i0 on.  A wave loads four rows at a time, each as dwords from the 4-byte
 *           aligned address at or below the row's first byte -- the phase differs from row to row when iw % 4 != 0 --
 *           through a buffer resource of its own that ends with the frame batch (what lies beyond reads 0, the one dword
 *           that straddles the end comes byte by byte), and v_alignbyte_b32 puts the row's first byte at byte 0 of the LDS
 *           row.  Bytes right of or below the window are staged with the rest; they only meet results outside the window's
 *           map, which are not stored.
 *   tmpl    nj rows of ceil(ni / 4) dwords, the taps beyond ni zero; sum T^2 is taken on the way (every block needs the
 *           whole template anyway), so there is no preparing launch.
 * Image row pitch: ipdw dwords with ipdw % 16 == 8.  A ds_read_b32 is served in two groups of 32 lanes over 32 banks; a group
 * reads dword (r0 + (l >> 3)) ipdw + (l & 7) + q, and (l >> 3) ipdw mod 32 runs through 0, 8, 16, 24 for its four rows, so the 32
 * lanes hit the 32 banks once each; the template dword is the same address in every lane (a broadcast).
 * Per four taps of a template row: one image dword (the other one is the step before's), one template dword, three
 * v_alignbyte_b32 and eight v_dot4_u32_u8 for 16 tap-results and their squares.  Row sums are u32 (at most 256 taps x
 * 65025), added to 64-bit totals after every template row.
 *
 * result != nullptr: the map bytes (row pitch rw, slot p of mrw * mrh bytes).  result == nullptr: the locate epilogue of
 * k_match_template_mfma -- per wave the maximum of score << 32 | ~(ry * rw + rx), one 64-bit atomicMax on keys[p] (zeroed
 * before the launch) from a wave that saw a non-zero score -- and k_tmw_best turns the keys into frame coordinates.
 */
#ifndef GS_K_TMATCH_WIN_H
#define GS_K_TMATCH_WIN_H
#include "prims.h"
#include "k_geom.h"   /* wave_max_u64 */
#include "k_resize.h" /* geom_store4 */

namespace gs {

constexpr unsigned kTmwTile = 32;           /* results per side of a block's tile */
constexpr unsigned kTmwBandCols = 256;      /* template columns resident at a time (a u32 row sum holds 66051 taps) */
constexpr unsigned kTmwLdsPlan = 24 * 1024; /* bytes of LDS a block may take: six blocks a CU */
constexpr unsigned kTmwInvalid = 0xFFFFFFFFu;

struct TmWinArgs {
  const uint8_t *img; /* frame f at img + f * iw * ih */
  unsigned iw, ih, n;
  const uint8_t *tmpl; /* window p's template at tmpl + p * tstep */
  unsigned tw, th;
  size_t tstep; /* 0: one template for every window; tw * th: one per window */
  const unsigned *windows;  /* {x, y, w, h} of window p at windows + 4 p */
  const unsigned *frame_of; /* NULL: window p lies in frame p */
  unsigned z0;              /* window of blockIdx.z == 0 (launches are split at kMaxZ windows) */
  unsigned max_ww, max_wh;
  uint8_t *result; /* map p at result + p * rslot, row pitch rw_p; nullptr: the locate epilogue */
  size_t rslot;
  unsigned long long *keys;        /* locate: keys[p] */
  unsigned band_rows, band_cols;   /* template rows / columns resident at a time */
  unsigned ipdw, tpdw;             /* dwords of an LDS image row (% 16 == 8) and of an LDS template row */
};

struct TmWin {
  unsigned x, y, w, h, f;
};
/* window p and its frame, the same in every lane */
GS_DEV TmWin tmw_read(const unsigned *windows, const unsigned *frame_of, unsigned p) {
  const unsigned *r = windows + 4u * (size_t)p;
  return TmWin{uniform(r[0]), uniform(r[1]), uniform(r[2]), uniform(r[3]), uniform(frame_of ? frame_of[p] : p)};
}
/* THE validity rule of the windows entries (include/grayskull_hip.h): the frame exists, the template fits the window, the
 * window fits the host's bound and lies inside the frame -- x + w tested without 32-bit overflow, as k_resize_tile does */
GS_DEV bool tmw_valid(const TmWin &w, unsigned tw, unsigned th, unsigned max_ww, unsigned max_wh, unsigned iw, unsigned ih, unsigned n) {
  return w.f < n && w.w >= tw && w.h >= th && w.w <= max_ww && w.h <= max_wh && w.x < iw && w.w <= iw - w.x && w.y < ih && w.h <= ih - w.y;
}
/* the dword at byte `off` of a buffer of nb bytes was requested where it lies whole inside (v; 0 otherwise, which is what lies
 * beyond the end).  The one dword that STRADDLES the end -- the batch's last bytes -- comes byte by byte */
GS_DEV uint32_t tmw_end_dword(const BufRsrc &B, uint32_t nb, uint32_t off, uint32_t v) {
  if (off < nb && off + 4u > nb) {
    v = 0;
    for (unsigned b = 0; off + b < nb; b++) v |= buf_load1(B, off + b) << (8u * b);
  }
  return v;
}

__global__ __launch_bounds__(256) void k_tmatch_windows(const TmWinArgs a) {
  GS_DYN_LDS(smem);
  __shared__ unsigned long long part[4];
  const unsigned lane = threadIdx.x, wave = uniform(threadIdx.y), tid = wave * 64u + lane;
  const unsigned p = a.z0 + blockIdx.z;
  const TmWin w = tmw_read(a.windows, a.frame_of, p);
  if (!tmw_valid(w, a.tw, a.th, a.max_ww, a.max_wh, a.iw, a.ih, a.n)) return; /* block-uniform */
  const unsigned rw = w.w - a.tw + 1u, rh = w.h - a.th + 1u;
  const unsigned bx0 = blockIdx.x * kTmwTile, by0 = blockIdx.y * kTmwTile;
  if (bx0 >= rw || by0 >= rh) return; /* a tile of the largest map that this window's map does not have */
  const unsigned c = lane & 7u, r = wave * 8u + (lane >> 3);
  const bool wave_in = by0 + wave * 8u < rh;
  uint32_t *limg = (uint32_t *)smem;
  uint32_t *ltm = limg + (size_t)(kTmwTile - 1u + a.band_rows) * a.ipdw;
  const size_t fb = (size_t)a.iw * a.ih;
  const uintptr_t frame = (uintptr_t)a.img + (size_t)w.f * fb, end = (uintptr_t)a.img + (size_t)a.n * fb;
  const uint8_t *tmpl = a.tmpl + (size_t)p * a.tstep;
  unsigned long long s_it[4] = {0, 0, 0, 0}, s_ii[4] = {0, 0, 0, 0}, tsq = 0;
  for (unsigned j0 = 0; j0 < a.th; j0 += a.band_rows) { /* block-uniform */
    const unsigned nj = a.th - j0 < a.band_rows ? a.th - j0 : a.band_rows;
    for (unsigned i0 = 0; i0 < a.tw; i0 += a.band_cols) {
      const unsigned ni = a.tw - i0 < a.band_cols ? a.tw - i0 : a.band_cols;
      const unsigned g4 = ni >> 2, rem = ni & 3u, nid = g4 + (rem ? 1u : 0u);
      __syncthreads(); /* the band before is done with */
      /* image rows: wave v takes rows v, v + 4, ..., four of them at a time -- the eight loads of a trip (a lane's dword d
       * and the one behind it, per row) are requested before the first is used; a row has its own buffer resource, from the
       * aligned address at or below its first byte to the end of the batch (no bytes for a row below the frame: zeros) */
      const unsigned nrows = kTmwTile - 1u + nj, nd = nid + 8u;
      for (unsigned d0 = 0; d0 < nd; d0 += 64u) { /* two trips from 224 template columns on */
        const unsigned d = d0 + lane;
        const uint32_t off = d < nd ? 4u * d : kOOB;
        for (unsigned rr0 = wave; rr0 < nrows; rr0 += 16u) {
          uint32_t lo[4], hi[4], ph[4], nb[4];
          BufRsrc B[4];
#pragma unroll
          for (unsigned u = 0; u < 4; u++) {
            const unsigned rr = rr0 + 4u * u;
            const unsigned long long y = (unsigned long long)w.y + by0 + j0 + rr;
            const bool in = rr < nrows && y < a.ih; /* wave-uniform */
            const uintptr_t first = frame + (size_t)(in ? y : w.y) * a.iw + w.x + bx0 + i0; /* inside the frame */
            ph[u] = (uint32_t)(first & 3u);
            const uintptr_t base = first - ph[u];
            const size_t left = end - base;
            nb[u] = !in ? 0u : left > 0x7fffffffu ? 0x7fffffffu : (uint32_t)left;
            B[u] = make_buf((const void *)(((uintptr_t)uniform((uint32_t)((unsigned long long)base >> 32)) << 32) | uniform((uint32_t)base)), nb[u]);
            lo[u] = buf_load4(B[u], off + 4u <= nb[u] ? off : kOOB), hi[u] = buf_load4(B[u], off + 8u <= nb[u] ? off + 4u : kOOB);
          }
#pragma unroll
          for (unsigned u = 0; u < 4; u++) {
            const unsigned rr = rr0 + 4u * u;
            lo[u] = tmw_end_dword(B[u], nb[u], off, lo[u]), hi[u] = tmw_end_dword(B[u], nb[u], off + 4u, hi[u]);
            if (rr < nrows && d < nd) limg[(size_t)rr * a.ipdw + d] = alignbyte(hi[u], lo[u], ph[u]);
          }
        }
      }
      /* template rows j0 .. j0 + nj - 1, columns i0 .. i0 + ni - 1, the taps beyond them zero; sum T^2 */
      uint32_t t2 = 0;
      for (unsigned i = tid; i < nj * nid; i += 256u) {
        const unsigned j = i / nid, q = i - j * nid;
        const uint8_t *src = tmpl + (size_t)(j0 + j) * a.tw + i0 + 4u * q;
        uint32_t v = 0;
        if (4u * q + 4u <= ni) v = load_u32_unaligned(src);
        else
          for (unsigned b = 0; 4u * q + b < ni; b++) v |= (uint32_t)src[b] << (8u * b);
        ltm[(size_t)j * a.tpdw + q] = v;
        t2 = udot4(v, v, t2); /* at most kTmwLdsPlan / 256 bytes per lane and band: far below 2^32 */
      }
      tsq += t2;
      __syncthreads();
      const uint32_t tailmask = rem ? (0xffffffffu >> (8u * (4u - rem))) : 0u; /* the ni % 4 last taps of a row */
      /* a wave whose eight rows lie below the window's map stages and waits with the block, and computes nothing */
      for (unsigned j = 0; j < (wave_in ? nj : 0u); j++) {
        const uint32_t *ir = limg + (size_t)(r + j) * a.ipdw + c;
        const uint32_t *tr = ltm + (size_t)j * a.tpdw;
        uint32_t it[4] = {0, 0, 0, 0}, ii[4] = {0, 0, 0, 0};
        uint32_t lo = ir[0];
#pragma unroll 4
        for (unsigned q = 0; q < g4; q++) {
          const uint32_t hi = ir[q + 1u], T4 = tr[q];
          const uint32_t w1 = alignbyte(hi, lo, 1), w2 = alignbyte(hi, lo, 2), w3 = alignbyte(hi, lo, 3);
          it[0] = udot4(lo, T4, it[0]), ii[0] = udot4(lo, lo, ii[0]);
          it[1] = udot4(w1, T4, it[1]), ii[1] = udot4(w1, w1, ii[1]);
          it[2] = udot4(w2, T4, it[2]), ii[2] = udot4(w2, w2, ii[2]);
          it[3] = udot4(w3, T4, it[3]), ii[3] = udot4(w3, w3, ii[3]);
          lo = hi;
        }
        if (rem) { /* block-uniform; the template's padded taps are 0, the image's are masked out of sum I^2 */
          const uint32_t hi = ir[g4 + 1u], T4 = tr[g4];
          const uint32_t w0 = lo & tailmask, w1 = alignbyte(hi, lo, 1) & tailmask, w2 = alignbyte(hi, lo, 2) & tailmask,
                         w3 = alignbyte(hi, lo, 3) & tailmask;
          it[0] = udot4(w0, T4, it[0]), ii[0] = udot4(w0, w0, ii[0]);
          it[1] = udot4(w1, T4, it[1]), ii[1] = udot4(w1, w1, ii[1]);
          it[2] = udot4(w2, T4, it[2]), ii[2] = udot4(w2, w2, ii[2]);
          it[3] = udot4(w3, T4, it[3]), ii[3] = udot4(w3, w3, ii[3]);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) s_it[k] += it[k], s_ii[k] += ii[k];
      }
    }
  }
  /* sum T^2: every thread's share of every band, over the block */
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t lo = shfl((uint32_t)tsq, (int)(lane ^ (unsigned)d)), hi = shfl((uint32_t)(tsq >> 32), (int)(lane ^ (unsigned)d));
    tsq += ((unsigned long long)hi << 32) | lo;
  }
  if (lane == 0) part[wave] = tsq;
  __syncthreads();
  tsq = part[0] + part[1] + part[2] + part[3];
  /* score = floor(SSD 255 / (taps 255^2)) = floor(SSD / (255 taps)) (ref :719-721).  Up to 32768 taps SSD < 2^32: the
   * float estimate of the quotient made exact by its remainder, as in k_match_template_mfma; beyond, the 64-bit division */
  const unsigned long long taps = (unsigned long long)a.tw * a.th, dv64 = 255ull * taps;
  const bool small = taps <= 32768ull;
  const unsigned dv = (unsigned)dv64;
  const float inv = 1.0f / (float)dv;
  const unsigned ry = by0 + r, rx0 = bx0 + 4u * c;
  const bool row_in = ry < rh;
  uint32_t out = 0;
  unsigned long long best = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const unsigned long long sum = s_ii[k] + tsq - 2ull * s_it[k]; /* = sum (I - T)^2 >= 0 where the result is inside the map */
    unsigned q;
    if (small) {
      const unsigned ssd = (unsigned)sum;
      q = (unsigned)((float)ssd * inv);
      const int rm = (int)(ssd - q * dv); /* |true quotient - q| <= 1, so the remainder fits */
      if (rm < 0) q--;
      else if ((unsigned)rm >= dv) q++;
    } else {
      const unsigned long long q64 = sum / dv64;
      q = q64 < 255ull ? (unsigned)q64 : 255u;
    }
    const unsigned v = 255u - (q < 255u ? q : 255u);
    out |= v << (8 * k);
    if (row_in && rx0 + (unsigned)k < rw) {
      const unsigned long long key = ((unsigned long long)v << 32) | (0xffffffffu - (ry * rw + rx0 + (unsigned)k));
      best = key > best ? key : best;
    }
  }
  if (a.result) { /* block-uniform */
    if (row_in && rx0 < rw) {
      uint8_t *o = a.result + (size_t)p * a.rslot + (size_t)ry * rw + rx0;
      if (rx0 + 4u <= rw) geom_store4<false>(o, out);
      else
        for (unsigned k = 0; rx0 + k < rw; k++) o[k] = (uint8_t)(out >> (8u * k));
    }
  } else { /* every lane of the wave is here.  The maximum over all waves of all blocks is the map's first maximum whatever
            * order they arrive in; a wave that saw only zeros leaves the key word alone */
    best = wave_max_u64(best);
    if (lane == 0 && (best >> 32)) atomicMax(a.keys + p, best);
  }
}

/* keys[p] (score << 32 | ~(ry * rw_p + rx); 0 in the high half: no non-zero score seen) -> best[p] in FRAME coordinates and
 * score[p] (may be NULL); a window that is not valid -- the same rule as the kernel that filled the keys -- gets the
 * sentinel {0xFFFFFFFF, 0xFFFFFFFF} and score 0.  grid ceil(nwin / 256), block 256 */
__global__ __launch_bounds__(256) void k_tmw_best(const unsigned long long *keys, const unsigned *windows, const unsigned *frame_of,
                                                  unsigned nwin, unsigned tw, unsigned th, unsigned max_ww, unsigned max_wh, unsigned iw,
                                                  unsigned ih, unsigned n, unsigned *best, uint8_t *score) {
  const unsigned p = blockIdx.x * 256u + threadIdx.x;
  if (p >= nwin) return;
  const unsigned *r = windows + 4u * (size_t)p;
  const TmWin w{r[0], r[1], r[2], r[3], frame_of ? frame_of[p] : p};
  unsigned bx = kTmwInvalid, by = kTmwInvalid, v = 0;
  if (tmw_valid(w, tw, th, max_ww, max_wh, iw, ih, n)) {
    const unsigned long long key = keys[p];
    const unsigned rw = w.w - tw + 1u, idx = 0xffffffffu - (unsigned)key;
    v = (unsigned)(key >> 32);
    bx = w.x + (v ? idx % rw : 0u), by = w.y + (v ? idx / rw : 0u);
  }
  best[2u * p] = bx, best[2u * p + 1u] = by;
  if (score) score[p] = (uint8_t)v;
}

/* windows[p] = the box {at[p].x, at[p].y, bw, bh} grown by mx / my on every side and clipped to the frame; a point outside
 * the frame (the sentinel of k_tmw_best among them) gives {0, 0, 0, 0}, which no entry takes for a valid window.
 * grid ceil(nwin / 256), block 256 */
__global__ __launch_bounds__(256) void k_search_windows(const unsigned *at, unsigned nwin, unsigned bw, unsigned bh, unsigned mx, unsigned my,
                                                        unsigned iw, unsigned ih, unsigned *windows) {
  const unsigned p = blockIdx.x * 256u + threadIdx.x;
  if (p >= nwin) return;
  const unsigned x = at[2u * p], y = at[2u * p + 1u];
  unsigned x0 = 0, y0 = 0, ww = 0, wh = 0;
  if (x < iw && y < ih) {
    x0 = x > mx ? x - mx : 0u, y0 = y > my ? y - my : 0u;
    const unsigned long long x1 = (unsigned long long)x + bw + mx, y1 = (unsigned long long)y + bh + my;
    ww = (unsigned)(x1 < iw ? x1 : iw) - x0, wh = (unsigned)(y1 < ih ? y1 : ih) - y0;
  }
  windows[4u * p] = x0, windows[4u * p + 1u] = y0, windows[4u * p + 2u] = ww, windows[4u * p + 3u] = wh;
}

}  // namespace gs
#endif
