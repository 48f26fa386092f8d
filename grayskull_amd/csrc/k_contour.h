/*
 * k_contour.h -- gs_trace_contour (grayskull.h:446-480) and the glue that takes gs_blobs records to contour starts.
 *
 * The walk (docs/design/contours.md has the contract in full): state (p, dir, seenstart), p = c->start, dir = 7.  Per
 * iteration: count p if visited[p] == 0, mark it; look at the 8 neighbours in the order d = (dir + 1 + i) % 8 with
 * dx = {1,1,0,-1,-1,-1,0,1}, dy = {0,1,1,1,0,-1,-1,-1}, a neighbour counting when it is inside the image and > 128;
 * none: stop; else move there, dir = (d + 6) % 8, update the box by the reference's running expressions, and stop the
 * second time p is the start.  The reference does not return when this map on (p, dir, seenstart) enters a cycle that
 * misses its exit; length, box and visited converge there, and those limits are what k_contour_trace delivers, with
 * status 1: Brent's cycle detection on the full state, then one more trip round the cycle so that box.w / box.h have
 * seen the final box.x / box.y.  A cap on the moves (5 x the number of states + 64, more than Brent's search and the
 * extra trip can take) stands behind the detector; reaching it is a bug and sets status 2.
 *
 * One WAVE per frame, the contours of a frame one after the other on the frame's `visited` plane.  The walk is one
 * dependent chain, so it runs on wave-uniform values (SGPRs) over a 64 x 64 BIT TILE of img > 128 held in registers:
 * lane l has row y0 + l as one 64-bit word (bit b = column x0 + b, 0 outside the image), and a second word collects
 * the pixels marked while the tile is current.  A step reads the three rows round p with v_readlane (wave-uniform
 * lane select), builds the 8-bit neighbour ring, rotates it by dir + 1 and takes the first set bit: no memory access.
 * When p reaches the tile's outermost rows / columns the tile is FLUSHED -- each lane loads the `visited` bytes of
 * its marked pixels, counts the zeros and stores 255 -- and re-centred on p, 31 moves at least from the next reload.
 * A pixel marked in two tiles is counted once: the first flush's store is waited for and fenced before any lane
 * loads again.  Plain loads / stores, readlanes and ballots only.
 */
#ifndef GS_K_CONTOUR_H
#define GS_K_CONTOUR_H
#include "prims.h"

namespace gs {

struct ContourRec { /* struct gs_contour, 28 B (ref :36-40) */
  uint32_t bx, by, bw, bh, sx, sy, length;
};

/* struct gs_blob as eight u32 (ref :29-34): label (u16 + padding), area, box x / y / w / h, centroid x / y */
constexpr unsigned kContourBlobWords = 8;
/* dx + 1 / dy + 1 of direction d in bits 2 d, 2 d + 1 (ref :448-449) */
constexpr uint32_t kContourDx = 2u | 2u << 2 | 1u << 4 | 0u << 6 | 0u << 8 | 0u << 10 | 1u << 12 | 2u << 14;
constexpr uint32_t kContourDy = 1u | 2u << 2 | 2u << 4 | 2u << 6 | 1u << 8 | 0u << 10 | 0u << 12 | 0u << 14;

/* this wave's earlier stores to global memory are complete and visible to the loads any of its lanes issues later */
GS_DEV void contour_fence() {
#ifndef GS_EMU
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
#endif
}

/* lanes k - 1, k, k + 1 of a 3-bit value, for a wave-uniform k in 1 .. 62: bits 0-2, 3-5, 6-8 (three v_readlane_b32;
 * the emulator's lanes meet once) */
GS_DEV uint32_t contour_rows3(uint32_t t, unsigned k) {
#ifdef GS_EMU
  return emu::wave_exchange(t, [=](const uint64_t *s, const bool *) { return (uint32_t)(s[k - 1u] | s[k] << 3 | s[k + 1u] << 6); });
#else
  return readlane_at(t, k - 1u) | readlane_at(t, k) << 3 | readlane_at(t, k + 1u) << 6;
#endif
}

/* 4 bytes -> 4 bits of (byte > 128), bit i = byte i: bit 7 set and one of the low seven */
GS_DEV uint32_t gt128_bits4(uint32_t d) {
  const uint32_t m = d & ((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) & 0x80808080u;
  return ((m >> 7) * 0x00204081u) >> 21 & 0xfu;
}
GS_DEV uint32_t gt128_bits16(const U4 &v) {
  return gt128_bits4(v.x) | gt128_bits4(v.y) << 4 | gt128_bits4(v.z) << 8 | gt128_bits4(v.w) << 12;
}

/* columns x0 .. x0 + 63 of row Y as bits of img > 128; 0 outside the image (x0, Y: two's complement coordinates).
 * Rows of 16 pixels and more: four 16-byte loads at any byte address, issued together -- a group that sticks out of the
 * row is loaded from the nearest place inside it (the row's first or last 16 bytes) and its bits shifted into place,
 * which also clears those outside the row; a row outside the image loads the nearest row and drops the result.  No
 * branch depends on where the tile lies, so the wave waits for memory once per reload. */
GS_DEV uint64_t contour_load_row(const uint8_t *img, unsigned w, unsigned h, uint32_t x0, uint32_t Y) {
  const bool rowin = Y < h;
  const uint8_t *row = img + (size_t)(rowin ? Y : ((int32_t)Y < 0 ? 0u : h - 1u)) * w;
  uint64_t m = 0;
  if (w >= 16u) {
    U4 v[4];
    long long sh[4];
#pragma unroll
    for (unsigned j = 0; j < 4u; j++) {
      const long long xs = (long long)(int32_t)(x0 + 16u * j);
      const long long xc = xs < 0 ? 0 : (xs > (long long)w - 16 ? (long long)w - 16 : xs);
      sh[j] = xs - xc; /* byte i of the load is column xc + i = xs + (i - sh) */
      v[j] = load_u32x4_any(row + xc);
    }
#pragma unroll
    for (unsigned j = 0; j < 4u; j++) {
      const uint32_t b = gt128_bits16(v[j]);
      const uint32_t g = sh[j] <= -16 || sh[j] >= 16 ? 0u : (sh[j] >= 0 ? b >> (unsigned)sh[j] : (b << (unsigned)(-sh[j])) & 0xffffu);
      m |= (uint64_t)g << (16u * j);
    }
  } else { /* the whole row is shorter than one load */
    for (unsigned X = 0; X < w; X++) {
      const uint32_t b = X - x0;
      if (b < 64u && row[X] > 128u) m |= 1ull << b;
    }
  }
  return rowin ? m : 0ull;
}

/* step 1 of the walk for the pixels of row Y marked in this tile: how many had visited == 0 (gs_get: 0 outside the
 * image); 255 stored to those inside */
GS_DEV uint32_t contour_flush_row(uint8_t *visited, unsigned w, unsigned h, uint32_t x0, uint32_t Y, uint64_t mark) {
  uint32_t cnt = 0;
  const bool rowin = Y < h;
  uint8_t *row = visited + (rowin ? (size_t)Y * w : (size_t)0);
  while (mark) {
    const uint32_t X = x0 + (uint32_t)__builtin_ctzll(mark);
    mark &= mark - 1ull;
    if (rowin && X < w) {
      cnt += row[X] == 0u ? 1u : 0u;
      row[X] = 255u;
    } else {
      cnt++;
    }
  }
  return cnt;
}

/* grid (frames), block 64.  recs: frames x per_frame records, frame f's first min(counts[f], per_frame) traced in index
 * order (counts == nullptr: all); status: one byte per record or nullptr; cap: the most moves of one walk */
__global__ __launch_bounds__(64) void k_contour_trace(const uint8_t *img, uint8_t *visited, unsigned w, unsigned h, ContourRec *recs,
                                                      unsigned per_frame, const unsigned *counts, uint8_t *status,
                                                      unsigned long long cap) {
  const unsigned f = blockIdx.x, lane = threadIdx.x & 63u;
  const size_t np = (size_t)w * h;
  img += np * f, visited += np * f;
  const unsigned nc = counts ? umin(uniform(counts[f]), per_frame) : per_frame;
  /* the tile outlives a contour: the image does not change, and the next start is often near */
  bool have = false;
  uint32_t x0 = 0, y0 = 0;
  uint64_t bits = 0, mark = 0;
  for (unsigned k = 0; k < nc; k++) {
    ContourRec *c = recs + (size_t)f * per_frame + k;
    const uint32_t sx = uniform(c->sx), sy = uniform(c->sy);
    uint32_t px = sx, py = sy, dir = 7u, seen = 0u, st = 0u;
    uint32_t bx = sx, by = sy, bw = 1u, bh = 1u;
    uint32_t cnt = 0; /* per lane: pixels this lane found unvisited */
    /* Brent: the saved state, the moves since it was saved, the window after which it is replaced */
    uint32_t tx = sx, ty = sy, tdir = 7u, tseen = 0u;
    unsigned long long power = 1ull, lam = 0ull, moves = 0ull, extra = 0ull;
    bool cyc = false;
    for (;;) {
      uint32_t lx = px - x0, ly = py - y0;
      if (!have || lx - 1u > 61u || ly - 1u > 61u) {
        if (have) {
          cnt += contour_flush_row(visited, w, h, x0, y0 + lane, mark);
          contour_fence();
        }
        x0 = px - 32u, y0 = py - 32u, lx = ly = 32u;
        bits = contour_load_row(img, w, h, x0, y0 + lane);
        mark = 0ull, have = true;
      }
      if (lane == ly) mark |= 1ull << lx;
      const uint32_t t = (uint32_t)(bits >> (lx - 1u)) & 7u; /* bit 0: x - 1, bit 1: x, bit 2: x + 1 */
      const uint32_t r = contour_rows3(t, ly), r0 = r & 7u, r1 = r >> 3 & 7u, r2 = r >> 6;
      /* bit d of ring: the neighbour in direction d */
      const uint32_t ring = (r1 >> 2 & 1u) | (r2 >> 2 & 1u) << 1 | (r2 >> 1 & 1u) << 2 | (r2 & 1u) << 3 | (r1 & 1u) << 4 | (r0 & 1u) << 5 |
                            (r0 >> 1 & 1u) << 6 | (r0 >> 2 & 1u) << 7;
      const uint32_t nd = (dir + 1u) & 7u, rot = ((ring | ring << 8) >> nd) & 0xffu;
      if (!rot) break; /* open contour */
      const uint32_t d = (nd + (uint32_t)__builtin_ctz(rot)) & 7u;
      px += (kContourDx >> (2u * d) & 3u) - 1u, py += (kContourDy >> (2u * d) & 3u) - 1u;
      dir = (d + 6u) & 7u;
      moves++;
      bx = umin(bx, px), by = umin(by, py);
      bw = umax(bw, px - bx + 1u), bh = umax(bh, py - by + 1u);
      if (cyc) { /* the extra trip round the cycle */
        if (--extra == 0ull) break;
        continue;
      }
      if (px == sx && py == sy) {
        if (seen) break; /* second time at the starting point */
        seen = 1u;
      }
      lam++;
      if (px == tx && py == ty && dir == tdir && seen == tseen) { /* a state repeats: the reference never returns */
        cyc = true, st = 1u, extra = lam;
      } else if (lam == power) {
        tx = px, ty = py, tdir = dir, tseen = seen;
        power *= 2ull, lam = 0ull;
      }
      if (moves >= cap) {
        st = 2u;
        break;
      }
    }
    cnt += contour_flush_row(visited, w, h, x0, y0 + lane, mark);
    contour_fence();
    mark = 0ull;
    cnt = wave_sum(cnt);
    if (lane == 0u) {
      c->bx = bx, c->by = by, c->bw = bw, c->bh = bh, c->length = cnt;
      if (status) status[(size_t)f * per_frame + k] = (uint8_t)st;
    }
  }
}

/* grid (ceil(nblobs / 4), frames), block 256: one wave per blob record; the first pixel of row box.y, from box.x on,
 * that carries the record's label is the blob's raster-first pixel */
__global__ __launch_bounds__(256) void k_contour_starts(const uint16_t *labels, unsigned w, unsigned h, const uint32_t *blobs,
                                                        unsigned nblobs, const unsigned *counts, ContourRec *recs) {
  const unsigned f = blockIdx.y, k = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (k >= nblobs) return; /* whole wave */
  if (counts && k >= counts[f]) return;
  const uint32_t *b = blobs + ((size_t)f * nblobs + k) * kContourBlobWords;
  const uint32_t label = b[0] & 0xffffu, bx = b[2], by = b[3], bw = b[4];
  if (by >= h || bx >= w) return; /* not a record of this frame */
  const unsigned x1 = bw > w - bx ? w : bx + bw;
  const uint16_t *row = labels + ((size_t)f * h + by) * w;
  for (unsigned xb = bx; xb < x1; xb += 64u) {
    const unsigned x = xb + lane;
    const uint64_t m = ballot(x < x1 && row[x] == label);
    if (m) {
      if (lane == 0u) {
        ContourRec *c = recs + (size_t)f * nblobs + k;
        c->sx = xb + (uint32_t)__builtin_ctzll(m), c->sy = by;
      }
      return;
    }
  }
}

}  // namespace gs
#endif
