/*
 * k_codes.h -- the second pass of the coded edge pipeline: 4-bit edge codes (k_fused.h, kFusedCodes) -> final 0 / 255 bytes.
 * HBM-bound like k_threshold: 0.5 B/px read, 1 B/px written.  Built by gs_stencil.cpp.
 */
#ifndef GS_K_CODES_H
#define GS_K_CODES_H
#include "prims.h"

namespace gs {

/* eight codes (one dword, nibbles low to high = px 0, 2, 4, 6, 1, 3, 5, 7: the fused kernel's shift-or fold of four u16
 * pairs) -> eight bytes c > k ? 255 : 0.  add = (127 - k) in every byte, k = 0..14: a nibble spread to a byte is <= 15,
 * so byte + add <= 142 never carries and its bit 7 says c > k. */
GS_DEV void expand_codes8(uint32_t d, uint32_t add, uint32_t &lo, uint32_t &hi) {
  const uint32_t even = d & 0x0f0f0f0fu, odd = (d >> 4) & 0x0f0f0f0fu; /* bytes: px 0, 4, 1, 5 / px 2, 6, 3, 7 */
  const uint32_t me = (((even + add) & 0x80808080u) >> 7) * 0xffu, mo = (((odd + add) & 0x80808080u) >> 7) * 0xffu;
  lo = perm_b32(mo, me, 0x06040200u); /* px 0, 1, 2, 3 */
  hi = perm_b32(mo, me, 0x07050301u); /* px 4, 5, 6, 7 */
}

/* grid (blocks, frames of the launch), block 256.  codes: the planes k_blur_sobel_codes wrote (layout: CodePairs, k_strip.h)
 * with bands of T rows, `pairs_per_band` = (T + 1) / 2, `lanes` = strips placed per row (a multiple of 64), `npairs` =
 * bands * pairs_per_band.  thr[f] = the frame's Otsu threshold t, guess[f] = the b its codes were written against.
 * A frame whose guess missed is left to k_blur_sobel_repair: every block of it returns before its first load.  Otherwise a
 * lane reads the 16 bytes of one row pair and strip and writes the two rows' 16 bytes of dst (streaming stores).  Like
 * the fused kernel's byte mode it writes whole strips of rows 1 .. h-2: columns 0 and w-1 are zeroed by k_zero_frame
 * behind it. */
__global__ __launch_bounds__(256) void k_expand_codes(uint8_t *dst, const uint8_t *codes, unsigned w, unsigned h, unsigned T,
                                                      size_t frame_bytes, size_t code_frame_bytes, unsigned lanes,
                                                      unsigned pairs_per_band, unsigned npairs, const uint8_t *thr,
                                                      const uint8_t *guess) {
  const unsigned f = blockIdx.y;
  const unsigned t = thr[f], b = guess[f];
  if (t < b || t > b + 14u) return; /* a miss: block-uniform */
  const uint32_t add = (0x7fu - (t - b)) * 0x01010101u;
  const BufRsrc cb = make_buf(codes + (size_t)f * code_frame_bytes, code_frame_bytes);
  const BufRsrc db = make_buf(dst + (size_t)f * frame_bytes, frame_bytes);
  const unsigned lane = threadIdx.x & 63u, wpr = lanes >> 6, nw = npairs * wpr; /* one wave per (row pair, 64 strips) */
  for (unsigned wv = uniform(blockIdx.x * 4u + (threadIdx.x >> 6)); wv < nw; wv += gridDim.x * 4u) {
    const unsigned q = wv / wpr, gid = (wv - q * wpr) * 64u + lane;
    const unsigned band = q / pairs_per_band, p = q - band * pairs_per_band;
    const unsigned y0 = 1u + band * T, left = h - 1u - y0;            /* the band's first row and the rows from there to h-2 */
    const unsigned nrows = left < T ? left : T, y = y0 + 2u * p;
    const uint32_t col = gid * 16u < w ? gid * 16u : kOOB;
    const U4 c = buf_load16(cb, (q * lanes + gid) * 16u);
    U4 r0, r1;
    expand_codes8(c.x, add, r0.x, r0.y), expand_codes8(c.y, add, r0.z, r0.w);
    expand_codes8(c.z, add, r1.x, r1.y), expand_codes8(c.w, add, r1.z, r1.w);
    /* rows past the band's end: pairs nobody wrote and the junk half of an odd band's last pair */
    buf_store16(db, (2u * p < nrows ? y * w : kRowOOB) + col, r0);
    buf_store16(db, (2u * p + 1u < nrows ? (y + 1u) * w : kRowOOB) + col, r1);
  }
}

}  // namespace gs
#endif
