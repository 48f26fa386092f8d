/*
 * k_resize.h -- gs_crop / gs_copy (ref grayskull.h:154-162), gs_resize_nn (:164-169) and gs_resize (:171-187) for
 * batches of frames and for patches cut out of frames (gsh_crop_batch, gsh_resize_batch, gsh_resize_nn_batch,
 * gsh_crop_resize_batch); the drop-in calls are the same kernels with one frame.  docs/design/stencils.md, "Geometry".
 *
 * k_resize_tile<NEAREST, NT>: grid (ceil(dw / 256), ceil(dh / band), patches), block (64, 4).  A block owns 256 output columns
 * -- a lane four adjacent ones, stored as one dword at any byte address -- and walks `band` output rows, wave v the rows
 * v, v + 4, ...  The source position sx depends on x alone and sy on y alone (ref :174-175), so a lane keeps its four
 * (xi, x1, dx) in registers for the whole band and the (yi, y1, dy) of a row are the same in every lane.  sx and sy are
 * monotone (every float operation of :174-177 rounds monotonically), so all the block reads lies in the source columns
 * xi(first column) .. x1(last column) and rows yi(first row) .. y1(last row).  Where that rectangle fits the block's LDS it
 * is STAGED first: row by row, one dword per lane (unaligned dword loads that stay inside the rectangle, bytes for the last
 * span % 4 columns), each source row once however many output rows tap it; the taps are then LDS byte reads.  Where it
 * does not fit (a wide frame squeezed in x and stretched in y), where the window has more than four source pixels per
 * result pixel (staging would read mostly bytes that nobody taps: measured slower than gathering from 2.04 x 2.04
 * on), where the launcher gave no LDS, or where nearest-neighbour's wrapping products make sx non-monotone, the same body
 * GATHERS its taps from global memory.  The choice is made per block from the rectangle the block computes itself, so no launcher estimate can make a
 * block overrun its LDS.
 *
 * Exactness (must survive any change here): the float32 operations of ref :174-184 in their order, no FMA contraction,
 * the correctly rounded division, the products (c * (1 - dx)) * (1 - dy) with unmerged weights, the float -> uint8_t
 * truncation; nearest-neighbour keeps the reference's wrapping 32-bit products x * sw.
 *
 * A patch of gsh_crop_resize_batch is the resize of a WINDOW (origin, size, row stride sw) read on the device: the taps
 * clamp at the window's edges.  A window that is empty, does not lie inside its frame (tested without 32-bit overflow)
 * or names a frame >= n gives a patch of zeros.
 */
#ifndef GS_K_RESIZE_H
#define GS_K_RESIZE_H
#include "prims.h"

namespace gs {

struct ResizeArgs {
  uint8_t *dst;          /* patch p at dst + p * dw * dh */
  const uint8_t *src;    /* frame f at src + f * sw * sh */
  const unsigned *rois;  /* NULL: patch p is the whole frame p; else {x, y, w, h} of patch p at rois + 4 p */
  const unsigned *frame_of; /* with rois: NULL = patch p comes from frame p */
  unsigned dw, dh, sw, sh, n;
  unsigned z0;           /* patch of blockIdx.z == 0 (launches are split at kMaxZ patches) */
  unsigned band;         /* output rows per block */
  unsigned lds;          /* bytes of dynamic LDS the launch gave every block (0: gather) */
  unsigned any_density;  /* stage whatever the scale (GSH_TUNE_GEOM_FORM = 2, measurements) */
};

/* a dword / four dwords to any byte address; NT: the streaming policy of the strip kernels' stores, for results larger
 * than the Infinity Cache (a template parameter: hipcc merges the two stores of a run-time choice into one plain store) */
template <bool NT> GS_DEV void geom_store4(uint8_t *p, uint32_t v) {
#ifdef GS_EMU
  memcpy(p, &v, 4);
#else
  typedef uint32_t u32_a1 __attribute__((aligned(1)));
  if (NT) __builtin_nontemporal_store(v, (u32_a1 *)p);
  else *(u32_a1 *)p = v;
#endif
}
template <bool NT> GS_DEV void geom_store16(uint8_t *p, const U4 &v) {
#ifdef GS_EMU
  memcpy(p, &v, 16);
#else
  if (NT) __builtin_nontemporal_store(gs_u32x4{v.x, v.y, v.z, v.w}, (gs_u32x4_a1 *)p);
  else store_u32x4_any(p, v);
#endif
}
/* the low min(4, dw - x0) bytes of `out` to row y of the patch at columns x0 .. */
template <bool NT> GS_DEV void resize_store(uint8_t *patch, unsigned dw, unsigned y, unsigned x0, uint32_t out) {
  if (x0 >= dw) return;
  uint8_t *o = patch + (size_t)y * dw + x0;
  if (x0 + 4u <= dw) {
    geom_store4<NT>(o, out);
  } else {
    for (unsigned j = 0; x0 + j < dw; j++) o[j] = (uint8_t)(out >> (8u * j));
  }
}

/* source position of output coordinate x of d on an axis of s pixels: ref :174, :176, :178-180 (:166 for NEAREST) */
template <bool NEAREST> GS_DEV void resize_axis(unsigned x, unsigned s, unsigned d, unsigned &i0, unsigned &i1, float &frac) {
#ifndef GS_EMU
#pragma clang fp contract(off)
#endif
  if (NEAREST) {
    i0 = i1 = x * s / d; /* the reference's 32-bit product: wraps */
    frac = 0.0f;
    return;
  }
  float sx = ((float)x + 0.5f) * (float)s / (float)d - 0.5f;
  const float mx = (float)s - 1.0f;
  sx = sx < mx ? sx : mx, sx = 0.0f > sx ? 0.0f : sx;
  i0 = (unsigned)sx;
  i1 = i0 + 1 < s - 1 ? i0 + 1 : s - 1;
  frac = sx - (float)i0;
}

/* rows y0 + wave, + 4, ... < yend of the block's columns.  taps(row, col) = tap at window row / column; base points at
 * (row0, col0) of a plane of `pitch` bytes per row -- the window itself (global memory) or its staged rectangle (LDS). */
template <bool NEAREST, bool NT>
GS_DEV void resize_rows(const ResizeArgs &a, uint8_t *patch, const uint8_t *base, size_t pitch, unsigned row0, unsigned col0,
                        unsigned wh, unsigned x0, unsigned y0, unsigned yend, const unsigned (&xi)[4], const unsigned (&x1)[4],
                        const float (&dx)[4]) {
#ifndef GS_EMU
#pragma clang fp contract(off)
#endif
  for (unsigned y = y0 + threadIdx.y; y < yend; y += 4u) {
    unsigned yi, y1;
    float dy;
    resize_axis<NEAREST>(y, wh, a.dh, yi, y1, dy);
    const uint8_t *r0 = base + (size_t)(yi - row0) * pitch, *r1 = base + (size_t)(y1 - row0) * pitch;
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (NEAREST) {
        out |= (uint32_t)r0[xi[j] - col0] << (8 * j);
      } else {
        const int c00 = (int)r0[xi[j] - col0], c01 = (int)r0[x1[j] - col0];
        const int c10 = (int)r1[xi[j] - col0], c11 = (int)r1[x1[j] - col0];
        const float p = ((float)c00 * (1 - dx[j]) * (1 - dy)) + ((float)c01 * dx[j] * (1 - dy)) +
                        ((float)c10 * (1 - dx[j]) * dy) + ((float)c11 * dx[j] * dy);
        out |= (uint32_t)(uint8_t)(int)p << (8 * j); /* float -> uint8_t truncation (value < 256) */
      }
    }
    resize_store<NT>(patch, a.dw, y, x0, out);
  }
}

template <bool NEAREST, bool NT>
__global__ __launch_bounds__(256) void k_resize_tile(const ResizeArgs a) {
  GS_DYN_LDS(smem);
  uint8_t *lds = (uint8_t *)smem;
  const unsigned lane = threadIdx.x, wv = threadIdx.y;
  const unsigned p = a.z0 + blockIdx.z;
  unsigned f = p, wx = 0, wy = 0, ww = a.sw, wh = a.sh;
  bool valid = true;
  if (a.rois) {
    const unsigned *r = a.rois + 4u * (size_t)p;
    wx = r[0], wy = r[1], ww = r[2], wh = r[3];
    if (a.frame_of) f = a.frame_of[p];
    valid = ww > 0 && wh > 0 && wx < a.sw && ww <= a.sw - wx && wy < a.sh && wh <= a.sh - wy && f < a.n;
  }
  uint8_t *patch = a.dst + (size_t)p * a.dw * a.dh;
  const unsigned xt = blockIdx.x * 256u, x0 = xt + lane * 4u;
  const unsigned y0 = blockIdx.y * a.band, yend = a.dh - y0 < a.band ? a.dh : y0 + a.band;
  if (!valid) { /* block-uniform */
    for (unsigned y = y0 + wv; y < yend; y += 4u) resize_store<NT>(patch, a.dw, y, x0, 0u);
    return;
  }
  const uint8_t *win = a.src + (size_t)f * a.sw * a.sh + (size_t)wy * a.sw + wx;
  unsigned xi[4], x1[4];
  float dx[4];
#pragma unroll
  for (int j = 0; j < 4; j++) { /* columns behind the row end compute the last column's taps and store nothing */
    const unsigned x = x0 + (unsigned)j < a.dw ? x0 + (unsigned)j : a.dw - 1u;
    resize_axis<NEAREST>(x, ww, a.dw, xi[j], x1[j], dx[j]);
  }
  /* the source rectangle of this block: the columns from lane 0's first to lane 63's last (the lanes behind the row end
   * hold the last column), the rows of the band's first and last output row; wave-uniform, so in SGPRs */
  unsigned rlo, rhi, t;
  float tf;
  const unsigned clo = readlane_at(xi[0], 0u), chi = readlane_last(x1[3]);
  resize_axis<NEAREST>(y0, wh, a.dh, rlo, t, tf);
  resize_axis<NEAREST>(yend - 1u, wh, a.dh, t, rhi, tf);
  rlo = uniform(rlo), rhi = uniform(rhi);
  /* nearest-neighbour's products wrap beyond 2^32: sx is monotone only below that */
  const bool mono = !NEAREST || ((((unsigned long long)(a.dw - 1u) * ww) | ((unsigned long long)(a.dh - 1u) * wh)) >> 32) == 0;
  /* staging reads the whole rectangle, gathering four taps per result pixel: beyond four source pixels per result pixel
   * (a downscale of more than 2 x 2) the rectangle is mostly bytes nobody taps, and gathering wins (docs/design/stencils.md) */
  const bool dense = (unsigned long long)ww * wh <= 4ull * a.dw * a.dh || a.any_density;
  bool staged = false;
  unsigned span = 0, pitch = 0, nrows = 0;
  if (mono && dense && a.lds) {
    span = chi - clo + 1u, pitch = (span + 3u) & ~3u, nrows = rhi - rlo + 1u;
    staged = (unsigned long long)pitch * nrows <= a.lds;
  }
  if (staged) { /* block-uniform */
    const unsigned nd = span >> 2, tail = span & 3u;
    for (unsigned r = wv; r < nrows; r += 4u) {
      const uint8_t *srow = win + (size_t)(rlo + r) * a.sw + clo;
      uint32_t *lrow = (uint32_t *)(lds + r * pitch);
      for (unsigned k = lane; k < nd; k += 64u) lrow[k] = load_u32_unaligned(srow + 4u * k);
      if (lane < tail) lds[r * pitch + 4u * nd + lane] = srow[4u * nd + lane];
    }
    __syncthreads();
    resize_rows<NEAREST, NT>(a, patch, lds, pitch, rlo, clo, wh, x0, y0, yend, xi, x1, dx);
  } else {
    resize_rows<NEAREST, NT>(a, patch, win, a.sw, 0u, 0u, wh, x0, y0, yend, xi, x1, dx);
  }
}

/* gs_crop of n frames: dst frame f (rw x rh) = the window (rx, ry, rw, rh) of src frame f, a strided row copy.  grid
 * (ceil(ceil(rw / 16) / 64), ceil(rh / 4), frames), block (64, 4): a lane moves 16 bytes of a row, at whatever byte
 * address the window's origin and the row lengths put source and destination (global memory takes a dwordx4 at any
 * address); the last lane of a row moves the rw % 16 bytes left as dwords and bytes.  Nothing outside the window is
 * read, nothing outside the result written. */
template <bool NT>
__global__ __launch_bounds__(256) void k_crop_rows(uint8_t *dst, const uint8_t *src, unsigned sw, unsigned sh, unsigned rx,
                                                   unsigned ry, unsigned rw, unsigned rh) {
  const unsigned x0 = (blockIdx.x * 64u + threadIdx.x) * 16u, y = blockIdx.y * 4u + threadIdx.y;
  if (x0 >= rw || y >= rh) return;
  const uint8_t *s = src + (size_t)blockIdx.z * sw * sh + (size_t)(ry + y) * sw + rx + x0;
  uint8_t *d = dst + (size_t)blockIdx.z * rw * rh + (size_t)y * rw + x0;
  const unsigned m = rw - x0 < 16u ? rw - x0 : 16u;
  if (m == 16u) {
    geom_store16<NT>(d, load_u32x4_any(s));
    return;
  }
  unsigned k = 0;
  for (; k + 4u <= m; k += 4u) geom_store4<NT>(d + k, load_u32_unaligned(s + k));
  for (; k < m; k++) d[k] = s[k];
}

/* gs_crop with a rectangle that only the reference's own WRAPPING test accepts (ref :155: roi.x + roi.w in 32 bits, e.g.
 * roi.x = 2^32 - 1, roi.w = 2): dst(x, y) = gs_get(src, roi.x + x, roi.y + y) with the reference's 32-bit sums, 0 outside
 * the source (ref :143-145, :157).  One thread per pixel, blocks of 64 x 4; the drop-in call's quirk path only. */
__global__ __launch_bounds__(256) void k_crop_wrapped(uint8_t *dst, const uint8_t *src, unsigned sw, unsigned sh, unsigned rx,
                                                      unsigned ry, unsigned rw, unsigned rh) {
  const unsigned x = blockIdx.x * 64u + threadIdx.x, y = blockIdx.y * 4u + threadIdx.y;
  if (x >= rw || y >= rh) return;
  const unsigned sx = rx + x, sy = ry + y;
  dst[(size_t)y * rw + x] = (sx < sw && sy < sh) ? src[(size_t)sy * sw + sx] : (uint8_t)0;
}

}  // namespace gs
#endif
