/*
 * k_morphk.h -- K applications of the 3x3 erode / dilate in ONE pass, K = 2, 3, 4 (k_morph16 of k_stencil.h stays the
 * K = 1 kernel), and the per-pixel form for any number of applications.  Included by k_stencil.h.
 *
 * Why one pass may stand for K: gs_morph (ref grayskull.h:286-302) takes the max (min) over the IN-IMAGE taps of the 3x3
 * window.  The image is a rectangle: two in-image pixels at Chebyshev distance <= K are joined by a king-move path of <= K
 * steps inside their bounding box, hence inside the image.  So K applications are the max (min) over the (2K+1)^2 window
 * clipped to the image -- max with 0 fill, min with 255 fill -- bit for bit, and a radius-a pass followed by a radius-b
 * pass is one radius-(a+b) pass.  tests/morph_cases.py proves it against the reference's own loop.
 *
 * Same strip form as k_morph16: Strip<!DILATE, RG>, 16 px per lane, erode as ~dilate(~x).  Strip::unpack delivers the
 * columns x0-4 .. x0+19 (everything outside the image 0), which is exactly radius 4.
 *   horizontal, once per input row: with P(s) = (px s, px s+1) as a u16 pair -- even s: U[] itself, odd s: one
 *     v_alignbit_b32 -- W2(s) = max(P(s), P(s+1)) and W4(s) = max(W2(s), W2(s+2)) are the running maxima of width 2 and
 *     4 for both halves of the pair; the (2K+1)-wide maximum of own pair k (pixels 2k, 2k+1) is
 *         K = 2: max(W4(2k-2), P(2k+2))     K = 3: max(W4(2k-3), W4(2k))     K = 4: max(W4(2k-4), W4(2k), P(2k+4))
 *     34 / 53 / 48 lane-ops per row of 16 px (K = 3 needs W4 at both parities) instead of 2K per pixel pair.
 *   vertical: a ring of the last 2K+1 horizontal rows, 8 registers each, indexed at compile time (the row loop is
 *     unrolled 2K+1 deep); the output row is the direct maximum over the ring.
 *   band prologue: rows y0-K .. y0+K-1 pass through the horizontal step before the first output row (lead = K); rows
 *     outside [0, h) read the zero fill through row_off.  Nothing depends on the band height T or the block shape.
 * Registers on gfx950 (hipcc -O3, -Rpass-analysis=kernel-resource-usage; no scratch anywhere), VGPRs for RG 0 / 1 / 2 and
 * waves per SIMD:   K = 2  dilate 70 / 71 / 73, erode 70 / 72 / 74   7 / 7 / 6 waves
 *                   K = 3  dilate 87 / 89 / 90, erode 93 / 91 / 95   5 waves
 *                   K = 4  dilate 105 / 110 / 108, erode 106 / 109 / 113   4 waves (72 registers are the ring)
 * (k_morph16: 42-56, 8 waves).  A byte-packed ring would return K = 4 to 5 waves for 72 more lane-ops per row; not built
 * before a measurement says that 4 waves of 16-byte loads leave HBM idle (docs/design/stencils.md 3.2).
 */
#ifndef GS_K_MORPHK_H
#define GS_K_MORPHK_H
#include "k_strip.h"

namespace gs {

/* (2K+1)-wide running maximum of a row for the lane's 8 own pairs; reads U[0..11] (index i = s + 4 below) */
template <int K> GS_DEV void morphk_hmax(const uint32_t (&U)[12], uint32_t (&H)[8]) {
  static_assert(K >= 2 && K <= 4, "radius 1 is k_morph16, beyond 4 the strip's halo ends");
  uint32_t P[23], W2[22], W4[20];
#pragma unroll
  for (int i = 0; i < 23; i++) P[i] = (i & 1) ? alignbit(U[(i + 1) / 2], U[(i - 1) / 2], 16) : U[i / 2];
#pragma unroll
  for (int i = 0; i < 22; i++) W2[i] = pk_max_u16(P[i], P[i + 1]);
#pragma unroll
  for (int i = 0; i < 20; i++) W4[i] = pk_max_u16(W2[i], W2[i + 2]);
  /* what a K does not reach is never computed: every index is a compile-time constant */
#pragma unroll
  for (int k = 0; k < 8; k++) {
    if constexpr (K == 2) H[k] = pk_max_u16(W4[2 * k + 2], P[2 * k + 6]);
    else if constexpr (K == 3) H[k] = pk_max_u16(W4[2 * k + 1], W4[2 * k + 4]);
    else H[k] = pk_max_u16(pk_max_u16(W4[2 * k], W4[2 * k + 4]), P[2 * k + 8]);
  }
}

template <bool DILATE, int K, int RG = 0>
__global__ __launch_bounds__(256) void k_morphk16(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h, unsigned T,
                                                  size_t frame_bytes) {
  constexpr int N = 2 * K + 1;
  const Strip<!DILATE, RG> S(src, dst, w, h, frame_bytes);
  if (S.wave_outside()) return; /* block wider than the frame */
  const int y0 = (int)(S.band * T);
  if (y0 >= (int)h) return;
  const int nrows = ((int)h - y0) < (int)T ? ((int)h - y0) : (int)T;
  uint32_t ring[N][8];
#pragma unroll
  for (int r = 0; r < N - 1; r++) { /* image rows y0-K .. y0+K-1 */
    uint32_t U[12];
    S.unpack(S.load(y0 - K + r), U);
    morphk_hmax<K>(U, ring[r]);
  }
  strip_rows<N, !DILATE>(S, y0, nrows, K, S.load(y0 + K), [&](auto I, int, const uint32_t(&U)[12]) {
    constexpr int slot = (decltype(I)::value + N - 1) % N; /* row i-K-1 leaves, row i+K enters */
    morphk_hmax<K>(U, ring[slot]);
    uint32_t M[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      uint32_t m = ring[0][k];
#pragma unroll
      for (int r = 1; r < N; r++) m = pk_max_u16(m, ring[r][k]);
      M[k] = m;
    }
    return U4{pack_lohi(M[0], M[1]), pack_lohi(M[2], M[3]), pack_lohi(M[4], M[5]), pack_lohi(M[6], M[7])};
  });
}

/* any w, h, alignment and radius: one thread per pixel, the clipped (2r+1)^2 window.  grid (ceil(w/64), ceil(h/4), n),
 * block (64, 4) like k_morph_px, which stays the radius-1 kernel */
template <bool DILATE>
__global__ __launch_bounds__(256) void k_morphr_px(uint8_t *dst, const uint8_t *src, unsigned w, unsigned h,
                                                   size_t frame_bytes, unsigned r) {
  const unsigned x = blockIdx.x * 64u + threadIdx.x, y = blockIdx.y * 4u + threadIdx.y;
  if (x >= w || y >= h) return;
  const uint8_t *f = src + (size_t)blockIdx.z * frame_bytes;
  const unsigned xa = x > r ? x - r : 0u, xb = w - 1u - x > r ? x + r : w - 1u;
  const unsigned ya = y > r ? y - r : 0u, yb = h - 1u - y > r ? y + r : h - 1u;
  unsigned v = DILATE ? 0u : 255u;
  for (unsigned yy = ya; yy <= yb; yy++)
    for (unsigned xx = xa; xx <= xb; xx++) {
      const unsigned p = f[(size_t)yy * w + xx];
      v = DILATE ? (p > v ? p : v) : (p < v ? p : v);
    }
  dst[(size_t)blockIdx.z * frame_bytes + (size_t)y * w + x] = (uint8_t)v;
}

}  // namespace gs
#endif
