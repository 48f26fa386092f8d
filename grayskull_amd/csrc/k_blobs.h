/*
 * k_blobs.h -- gs_blobs (grayskull.h:330-402), gs_blob_corners (:404-421), gs_perspective_correct (:423-444).
 *
 * gs_blobs labels the 4-connected components of a labelled set M with the rank of each component's raster-first
 * pixel among the START pixels (fg pixels whose left and top neighbours are not fg; fg = img >= 128).  With at most
 * `cap` start pixels M = fg; otherwise, with P the start pixel of rank cap + 1, M holds every fg pixel before P and,
 * after P, the fg pixels whose left or top neighbour is in M (the reference's "out of labels" skip, ref :348).
 *
 * Everything works on 1-bit rows: word k of row y holds pixels 64 k .. 64 k + 63 (bit b = pixel 64 k + b), W words
 * per row, bits at and beyond w zero.  One WAVE per row, lane l on words l, l + 64, ...; runs of consecutive set bits
 * ("runs") are the union-find nodes, keyed by the frame-local raster index of their first pixel so that a component's
 * minimum node is its raster-first pixel.
 *
 *   k_blob_fg      image -> fg words
 *   k_blob_count   start pixels per row
 *   k_blob_scan    per frame: row prefix of the start counts, total, P (0xffffffff when total <= cap)
 *   k_blob_close   frames with a P only: one wave walks the rows from P on and turns fg into M in place -- a seeded
 *                  fill per word, s = fg & top-in-M, M = fg & (s | ((fg + s + c) ^ fg ^ s)), whose carries cross the
 *                  words of a row as one more fill over the wave's ballots
 *   k_blob_init    parent[r] = r for every run r of M
 *   k_blob_union   vertically touching runs: atomicMin union (Playne & Hawick), roots are minima
 *   k_blob_roots   roots: label = rank of the root's start pixel, written at the root's own label position; other
 *                  runs: parent = root
 *   k_blob_label   the whole labels array, and per-label area / box / coordinate sums accumulated per lane over a
 *                  band of rows (atomics only when the label changes; at the end of the band lanes holding the
 *                  same label reduce across the wave first)
 *   k_blob_compact per frame: the non-empty label slots in label order as struct gs_blob records, and their count
 *
 * Only atomicMin / atomicMax / atomicAdd are used (k_blob_paint, further down: atomicOr on LDS words).
 *
 * Behind the three functions: k_blob_largest (each frame's first record of maximum area) and k_blob_paint (the picture
 * nanomagick's `blobs` verb draws from the records), both described where they stand.
 */
#ifndef GS_K_BLOBS_H
#define GS_K_BLOBS_H
#include "prims.h"

namespace gs {

constexpr unsigned kBlobCapMax = 65535;   /* gs_label is u16: labels 1 .. 65535 */
constexpr unsigned kBlobNoP = 0xffffffffu; /* k_blob_scan: frame not capped */
constexpr unsigned kBlobBand = 8;          /* rows per wave in k_blob_label */
constexpr unsigned kBlobCloseLds = 4096;   /* words of the previous row k_blob_close keeps in LDS (w <= 262144) */
/* label slot: area, ~min x, ~min y, max x, max y, sum x, sum y, (pad) -- a zeroed slot is empty */
constexpr unsigned kBlobSlot = 8;
/* per frame info words: total start pixels, P */
constexpr unsigned kBlobInfo = 2;

struct BlobRec { /* struct gs_blob, 32 B (ref :27-34) */
  uint32_t label, area, bx, by, bw, bh, cx, cy;
};

GS_DEV uint64_t shfl64(uint64_t v, int src) {
  return (uint64_t)shfl((uint32_t)v, src) | ((uint64_t)shfl((uint32_t)(v >> 32), src) << 32);
}
GS_DEV uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t t = shfl(v, (int)(lane_id() ^ (unsigned)d));
    v = t > v ? t : v;
  }
  return v;
}
/* inclusive max-scan across the wave */
GS_DEV uint32_t wave_incl_max(uint32_t v) {
  const unsigned l = lane_id();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = shfl(v, (int)l - d);
    if ((int)l >= d) v = t > v ? t : v;
  }
  return v;
}
GS_DEV uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint64_t t = shfl64(v, (int)(lane_id() ^ (unsigned)d));
    v = t < v ? t : v;
  }
  return v;
}
GS_DEV uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint64_t t = shfl64(v, (int)(lane_id() ^ (unsigned)d));
    v = t > v ? t : v;
  }
  return v;
}

/* parent entries change under other waves' atomics: read them at device scope (a stale value from the CU's cache is
 * still an ancestor, so this is for convergence, not for correctness) */
GS_DEV unsigned par_load(const unsigned *p) {
#ifdef GS_EMU
  return *p;
#else
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
GS_DEV unsigned uf_find(const unsigned *par, unsigned a) {
  unsigned p = par_load(par + a);
  while (p != a) a = p, p = par_load(par + a);
  return a;
}
/* parent[x] <= x always; the smaller root wins.  A lost race (old != a) means a was linked meanwhile: go on from there. */
GS_DEV void uf_union(unsigned *par, unsigned a, unsigned b) {
  for (;;) {
    a = uf_find(par, a), b = uf_find(par, b);
    if (a == b) return;
    if (a < b) {
      const unsigned t = a;
      a = b, b = t;
    }
    const unsigned old = atomicMin(par + a, b);
    if (old == a) return;
    a = old;
  }
}

/* 16 bytes -> 16 fg bits (byte >= 128), little-endian: bit i = byte i */
GS_DEV uint32_t fg_bits4(uint32_t d) { return (((d >> 7) & 0x01010101u) * 0x00204081u) >> 21 & 0xfu; }
GS_DEV uint32_t fg_bits16(const U4 &v) {
  return fg_bits4(v.x) | fg_bits4(v.y) << 4 | fg_bits4(v.z) << 8 | fg_bits4(v.w) << 12;
}

/* row y of a frame's bit rows, chunk k0: the word of this lane and the carry bookkeeping of the row */
struct RowWord {
  uint64_t m;   /* this lane's word */
  uint64_t rs;  /* run starts: set bits whose left neighbour is clear */
  uint32_t r0;  /* x of the run that reaches bit 0 from the left (meaningful when bit 0 is set and not a run start) */
};
/* call with all 64 lanes; carry_hi / carry_r0 are the row's chunk carries (start: 0, 0) */
GS_DEV RowWord row_word(uint64_t m, unsigned k, uint32_t &carry_hi, uint32_t &carry_r0) {
  RowWord r;
  r.m = m;
  const uint32_t hi = (uint32_t)(m >> 63);
  const uint32_t cin = wave_shr1(hi, carry_hi);
  r.rs = m & ~((m << 1) | (uint64_t)cin);
  /* x + 1 of the highest clear bit: a run reaching bit 0 of word k started right after the last clear bit before it */
  const uint64_t z = ~m;
  const uint32_t hz = z ? 64u * k + 64u - (uint32_t)__builtin_clzll(z) : 0u;
  const uint32_t inc = wave_incl_max(hz);
  uint32_t ex = wave_shr1(inc, 0u);
  ex = ex > carry_r0 ? ex : carry_r0;
  r.r0 = ex;
  carry_hi = readlane_last(hi);
  const uint32_t last = readlane_last(inc);
  carry_r0 = last > carry_r0 ? last : carry_r0;
  return r;
}
/* x of the first pixel of the run that holds bit b (set) of word k */
GS_DEV uint32_t run_start_x(const RowWord &r, unsigned k, unsigned b) {
  const uint64_t below = b ? (~r.m & ((1ull << b) - 1ull)) : 0ull;
  return below ? 64u * k + 64u - (uint32_t)__builtin_clzll(below) : r.r0;
}
/* start pixels of fg word `cur` (top: the word above, 0 on row 0) */
GS_DEV uint64_t start_bits(uint64_t cur, uint64_t top, uint32_t &carry_hi) {
  const uint32_t hi = (uint32_t)(cur >> 63);
  const uint32_t cin = wave_shr1(hi, carry_hi);
  carry_hi = readlane_last(hi);
  return cur & ~((cur << 1) | (uint64_t)cin) & ~top;
}

/* grid (ceil(h / 4), frames), block 256: one wave per row */
__global__ __launch_bounds__(256) void k_blob_fg(const uint8_t *img, unsigned w, unsigned h, unsigned W, uint64_t *bits) {
  const unsigned y = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (y >= h) return;
  const uint8_t *row = img + (size_t)blockIdx.y * w * h + (size_t)y * w;
  uint64_t *out = bits + ((size_t)blockIdx.y * h + y) * W;
  for (unsigned k = lane; k < W; k += 64u) {
    const unsigned x0 = 64u * k, nb = w - x0 < 64u ? w - x0 : 64u;
    uint64_t m = 0;
    if (nb == 64u && ((uintptr_t)(row + x0) & 15u) == 0u) {
      const U4 *p = (const U4 *)(row + x0);
      const U4 a = p[0], b = p[1], c = p[2], d = p[3];
      m = (uint64_t)fg_bits16(a) | (uint64_t)fg_bits16(b) << 16 | (uint64_t)fg_bits16(c) << 32 | (uint64_t)fg_bits16(d) << 48;
    } else {
      for (unsigned i = 0; i < nb; i++) m |= (uint64_t)(row[x0 + i] >> 7) << i;
    }
    out[k] = m;
  }
}

/* grid (ceil(h / 4), frames), block 256: start pixels per row */
__global__ __launch_bounds__(256) void k_blob_count(const uint64_t *fg, unsigned h, unsigned W, unsigned *rowcnt) {
  const unsigned y = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (y >= h) return; /* whole wave */
  const uint64_t *cur = fg + ((size_t)blockIdx.y * h + y) * W, *top = y > 0 ? cur - W : nullptr;
  uint32_t carry = 0, cnt = 0;
  for (unsigned k0 = 0; k0 < W; k0 += 64u) {
    const unsigned k = k0 + lane;
    const uint64_t c = k < W ? cur[k] : 0ull, t = (k < W && y > 0) ? top[k] : 0ull;
    cnt += (uint32_t)__popcll(start_bits(c, t, carry));
  }
  cnt = wave_sum(cnt);
  if (lane == 0) rowcnt[(size_t)blockIdx.y * h + y] = cnt;
}

/* grid (frames), block 1024: rowpre = exclusive prefix of rowcnt, info = {total, P} */
__global__ __launch_bounds__(1024) void k_blob_scan(const unsigned *rowcnt, const uint64_t *fg, unsigned w, unsigned h,
                                                    unsigned W, unsigned cap, unsigned *rowpre, unsigned *info) {
  __shared__ unsigned wsum[16];
  __shared__ unsigned carry_s, p_s;
  const unsigned tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const unsigned *cf = rowcnt + (size_t)blockIdx.x * h;
  unsigned *pf = rowpre + (size_t)blockIdx.x * h;
  if (tid == 0) carry_s = 0, p_s = kBlobNoP;
  __syncthreads();
  for (unsigned base = 0; base < h; base += 1024u) {
    const unsigned y = base + tid;
    const unsigned v = y < h ? cf[y] : 0u;
    const unsigned inc = wave_incl_scan(v);
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    unsigned woff = 0;
    for (unsigned k = 0; k < wv; k++) woff += wsum[k];
    const unsigned carry = carry_s, pre = carry + woff + inc - v;
    if (y < h) {
      pf[y] = pre;
      if (pre <= cap && cap - pre < v) { /* start pixel number cap + 1 (0-based: cap) lies in this row */
        const uint64_t *cur = fg + ((size_t)blockIdx.x * h + y) * W, *top = y > 0 ? cur - W : nullptr;
        unsigned need = cap - pre;
        uint64_t prev = 0;
        for (unsigned k = 0; k < W; k++) {
          const uint64_t c = cur[k], t = y > 0 ? top[k] : 0ull;
          uint64_t s = c & ~((c << 1) | (prev >> 63)) & ~t;
          prev = c;
          const unsigned pc = (unsigned)__popcll(s);
          if (need < pc) {
            for (unsigned i = 0; i < need; i++) s &= s - 1ull;
            p_s = y * w + 64u * k + (unsigned)__builtin_ctzll(s);
            break;
          }
          need -= pc;
        }
      }
    }
    __syncthreads();
    if (tid == 1023) carry_s = carry + woff + inc;
    __syncthreads();
  }
  if (tid == 0) {
    info[(size_t)blockIdx.x * kBlobInfo + 0] = carry_s;
    info[(size_t)blockIdx.x * kBlobInfo + 1] = p_s;
  }
}

/* seeded fill of one row chunk: bits of x reachable from a seed of s (s within x) or from the chunk's carry-in by moving
 * right through x; the carry-out crosses to the next word by the same fill over the wave's ballots */
GS_DEV uint64_t fill_row_chunk(uint64_t x, uint64_t s, uint32_t &carry) {
  const uint64_t s0 = x + s;
  const bool co0 = s0 < x;              /* carries out with no carry in */
  const bool co1 = co0 || s0 == ~0ull;  /* ... with a carry in */
  const uint64_t G = ballot(co0), X = G | ballot(co1);
  const uint64_t CO = X & (G | ((X + G + (uint64_t)carry) ^ X ^ G));
  const unsigned l = lane_id();
  const uint64_t ci = l == 0 ? (uint64_t)carry : (CO >> (l - 1)) & 1ull;
  carry = (uint32_t)(CO >> 63);
  return x & (s | ((x + s + ci) ^ x ^ s));
}

/* grid (frames), block 64: frames with a P turn fg into M in place, row by row from P's row on */
__global__ __launch_bounds__(64) void k_blob_close(uint64_t *bits, unsigned w, unsigned h, unsigned W, const unsigned *info) {
  __shared__ uint64_t prevM[kBlobCloseLds];
  const unsigned P = info[(size_t)blockIdx.x * kBlobInfo + 1];
  if (P == kBlobNoP) return;
  const unsigned lane = threadIdx.x, yP = P / w, xP = P % w, kP = xP >> 6, bP = xP & 63u;
  uint64_t *fb = bits + (size_t)blockIdx.x * h * W;
  /* the row above P's row is in M whole */
  for (unsigned k = lane; k < W && k < kBlobCloseLds; k += 64u) prevM[k] = yP > 0 ? fb[(size_t)(yP - 1) * W + k] : 0ull;
  wave_sync();
  for (unsigned y = yP; y < h; y++) {
    uint64_t *row = fb + (size_t)y * W;
    const uint64_t *above = y > 0 ? fb + (size_t)(y - 1) * W : nullptr;
    uint32_t carry = 0;
    for (unsigned k0 = 0; k0 < W; k0 += 64u) {
      const unsigned k = k0 + lane;
      const uint64_t f = k < W ? row[k] : 0ull;
      const uint64_t top = k >= W || y == 0 ? 0ull : k < kBlobCloseLds ? prevM[k] : above[k];
      uint64_t keep = ~0ull, low = 0ull; /* P's row: bits before P stay (M = fg there), P and the bits after are filled */
      if (y == yP) {
        if (k < kP) keep = 0ull, low = ~0ull;
        else if (k == kP) low = (1ull << bP) - 1ull, keep = bP == 63u ? 0ull : ~0ull << (bP + 1u);
      }
      const uint64_t x = f & keep;
      const uint64_t m = (f & low) | fill_row_chunk(x, x & top, carry);
      wave_sync(); /* every lane has read prevM of this chunk */
      if (k < W) {
        row[k] = m;
        if (k < kBlobCloseLds) prevM[k] = m;
      }
    }
    wave_sync();
  }
}

/* grid (ceil(h / 4), frames), block 256: parent[r] = r for every run r of M */
__global__ __launch_bounds__(256) void k_blob_init(const uint64_t *M, unsigned w, unsigned h, unsigned W, unsigned *par) {
  const unsigned y = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (y >= h) return;
  const uint64_t *cur = M + ((size_t)blockIdx.y * h + y) * W;
  unsigned *pf = par + (size_t)blockIdx.y * w * h;
  const unsigned base = y * w;
  uint32_t carry = 0;
  for (unsigned k0 = 0; k0 < W; k0 += 64u) {
    const unsigned k = k0 + lane;
    const uint64_t m = k < W ? cur[k] : 0ull;
    const uint32_t cin = wave_shr1((uint32_t)(m >> 63), carry);
    carry = readlane_last((uint32_t)(m >> 63));
    uint64_t rs = m & ~((m << 1) | (uint64_t)cin);
    while (rs) {
      const unsigned node = base + 64u * k + (unsigned)__builtin_ctzll(rs);
      pf[node] = node;
      rs &= rs - 1ull;
    }
  }
}

/* grid (ceil(h / 4), frames), block 256: rows y >= 1 unite their runs with the runs above them.  Two runs touch over an
 * interval of columns that starts where one of them starts: one union per such column. */
__global__ __launch_bounds__(256) void k_blob_union(const uint64_t *M, unsigned w, unsigned h, unsigned W, unsigned *par) {
  const unsigned y = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (y >= h || y == 0) return;
  const uint64_t *cur = M + ((size_t)blockIdx.y * h + y) * W, *top = cur - W; /* y >= 1 here */
  unsigned *pf = par + (size_t)blockIdx.y * w * h;
  uint32_t ch = 0, cr = 0, th = 0, tr = 0;
  for (unsigned k0 = 0; k0 < W; k0 += 64u) {
    const unsigned k = k0 + lane;
    const RowWord c = row_word(k < W ? cur[k] : 0ull, k, ch, cr);
    const RowWord t = row_word(k < W ? top[k] : 0ull, k, th, tr);
    uint64_t u = c.m & t.m & (c.rs | t.rs);
    while (u) {
      const unsigned b = (unsigned)__builtin_ctzll(u);
      u &= u - 1ull;
      uf_union(pf, y * w + run_start_x(c, k, b), (y - 1) * w + run_start_x(t, k, b));
    }
  }
}

/* grid (ceil(h / 4), frames), block 256: roots get their label (the rank of their start pixel) at their own position
 * of `labels`; every other run points straight at its root */
__global__ __launch_bounds__(256) void k_blob_roots(const uint64_t *M, const uint64_t *fg, unsigned w, unsigned h, unsigned W,
                                                    unsigned *par, const unsigned *rowpre, uint16_t *labels) {
  const unsigned y = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (y >= h) return;
  const size_t rw = ((size_t)blockIdx.y * h + y) * W;
  const uint64_t *cur = M + rw, *fcur = fg + rw, *ftop = y > 0 ? fcur - W : nullptr;
  unsigned *pf = par + (size_t)blockIdx.y * w * h;
  uint16_t *lf = labels + (size_t)blockIdx.y * w * h;
  const unsigned base = y * w;
  uint32_t mc = 0, fc = 0, rank = rowpre[(size_t)blockIdx.y * h + y];
  for (unsigned k0 = 0; k0 < W; k0 += 64u) {
    const unsigned k = k0 + lane;
    const uint64_t m = k < W ? cur[k] : 0ull;
    const uint64_t st = start_bits(k < W ? fcur[k] : 0ull, (k < W && y > 0) ? ftop[k] : 0ull, fc);
    const uint32_t cin = wave_shr1((uint32_t)(m >> 63), mc);
    mc = readlane_last((uint32_t)(m >> 63));
    uint64_t rs = m & ~((m << 1) | (uint64_t)cin);
    const uint32_t pc = (uint32_t)__popcll(st), inc = wave_incl_scan(pc);
    const uint32_t before = rank + inc - pc;
    rank += readlane_last(inc);
    while (rs) {
      const unsigned b = (unsigned)__builtin_ctzll(rs);
      rs &= rs - 1ull;
      const unsigned node = base + 64u * k + b, r = uf_find(pf, node);
      if (r == node) /* a root is a start pixel (its left and top are not in M, hence -- before P -- not fg) */
        lf[node] = (uint16_t)(before + (unsigned)__popcll(st & ((1ull << b) - 1ull)) + 1u);
      else
        pf[node] = r;
    }
  }
}

/* per-lane running statistics of one label */
struct BlobAcc {
  uint32_t label, area, nminx, nminy, maxx, maxy, sx, sy;
};
GS_DEV void acc_flush(unsigned *slot, const BlobAcc &a) {
  atomicAdd(slot + 0, a.area);
  atomicMax(slot + 1, a.nminx);
  atomicMax(slot + 2, a.nminy);
  atomicMax(slot + 3, a.maxx);
  atomicMax(slot + 4, a.maxy);
  atomicAdd(slot + 5, a.sx);
  atomicAdd(slot + 6, a.sy);
}

/* grid (ceil(h / (4 * kBlobBand)), frames), block 256: one wave per band of kBlobBand rows */
__global__ __launch_bounds__(256) void k_blob_label(const uint64_t *M, unsigned w, unsigned h, unsigned W, const unsigned *par,
                                                    uint16_t *labels, unsigned *stats, unsigned nslot) {
  const unsigned band = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  const unsigned y0 = band * kBlobBand;
  if (y0 >= h) return;
  const unsigned y1 = y0 + kBlobBand < h ? y0 + kBlobBand : h;
  const unsigned *pf = par + (size_t)blockIdx.y * w * h;
  uint16_t *lf = labels + (size_t)blockIdx.y * w * h;
  unsigned *sf = stats + (size_t)blockIdx.y * nslot * kBlobSlot;
  BlobAcc acc = {0, 0, 0, 0, 0, 0, 0, 0};
  for (unsigned y = y0; y < y1; y++) {
    const uint64_t *cur = M + ((size_t)blockIdx.y * h + y) * W;
    const unsigned base = y * w;
    uint32_t ch = 0, cr = 0;
    for (unsigned k0 = 0; k0 < W; k0 += 64u) {
      const unsigned k = k0 + lane;
      const RowWord r = row_word(k < W ? cur[k] : 0ull, k, ch, cr);
      if (k >= W) continue;
      /* the run reaching bit 0 from the word before */
      uint32_t L = ((r.m & 1ull) && !(r.rs & 1ull)) ? lf[pf[base + r.r0]] : 0u;
      for (unsigned g = 0; g < 8u; g++) {
        const unsigned x0 = 64u * k + 8u * g;
        if (x0 >= w) break;
        const uint32_t bits = (uint32_t)(r.m >> (8u * g)) & 0xffu, starts = (uint32_t)(r.rs >> (8u * g)) & 0xffu;
        uint32_t out[4];
#pragma unroll
        for (unsigned j = 0; j < 8u; j++) {
          uint32_t v = 0;
          if ((bits >> j) & 1u) {
            const unsigned x = x0 + j;
            if ((starts >> j) & 1u) L = lf[pf[base + x]];
            v = L;
            if (L != acc.label) {
              if (acc.label && acc.label < nslot) acc_flush(sf + (size_t)acc.label * kBlobSlot, acc);
              acc = BlobAcc{L, 0, 0, 0, 0, 0, 0, 0};
            }
            acc.area++;
            acc.nminx = ~x > acc.nminx ? ~x : acc.nminx;
            acc.nminy = ~y > acc.nminy ? ~y : acc.nminy;
            acc.maxx = x > acc.maxx ? x : acc.maxx;
            acc.maxy = y > acc.maxy ? y : acc.maxy;
            acc.sx += x, acc.sy += y;
          }
          if (j & 1u) out[j >> 1] |= v << 16;
          else out[j >> 1] = v;
        }
        uint16_t *dst = lf + base + x0;
        if (x0 + 8u <= w && ((uintptr_t)dst & 15u) == 0u) {
          *(U4 *)dst = U4{out[0], out[1], out[2], out[3]};
        } else {
          for (unsigned j = 0; j < 8u && x0 + j < w; j++) dst[j] = (uint16_t)(out[j >> 1] >> (16u * (j & 1u)));
        }
      }
    }
  }
  /* lanes that hold the same label add up across the wave first (a frame-filling blob: one flush per band, not 64) */
  for (unsigned round = 0; round < 4u; round++) {
    const uint64_t pend = ballot(acc.label != 0u);
    if (!pend) break;
    const uint32_t lead = readlane_at(acc.label, (unsigned)__builtin_ctzll(pend));
    const bool mine = acc.label == lead;
    if (__popcll(ballot(mine)) < 2) break;
    const uint32_t area = wave_sum(mine ? acc.area : 0u), sx = wave_sum(mine ? acc.sx : 0u), sy = wave_sum(mine ? acc.sy : 0u);
    const uint32_t nminx = wave_max_u32(mine ? acc.nminx : 0u), nminy = wave_max_u32(mine ? acc.nminy : 0u);
    const uint32_t maxx = wave_max_u32(mine ? acc.maxx : 0u), maxy = wave_max_u32(mine ? acc.maxy : 0u);
    if (mine && lane == (unsigned)__builtin_ctzll(pend) && lead < nslot)
      acc_flush(sf + (size_t)lead * kBlobSlot, BlobAcc{lead, area, nminx, nminy, maxx, maxy, sx, sy});
    if (mine) acc.label = 0;
  }
  if (acc.label && acc.label < nslot) acc_flush(sf + (size_t)acc.label * kBlobSlot, acc);
}

/* grid (frames), block 1024: slots 1 .. min(total, cap) that are not empty, in label order, as records; counts[f] = m.
 * wrap (nblobs >= 65535): a frame with 65535 or more start pixels has run the reference's u16 label counter round to 0,
 * after which it returns 0 (its merge and compact loops run to next - 1 = -1; with more start pixels it writes
 * blobs[-1], undefined) -- m = 0 and no records for such frames, the labels stay as written */
__global__ __launch_bounds__(1024) void k_blob_compact(const unsigned *stats, unsigned nslot, unsigned cap, unsigned wrap,
                                                       const unsigned *info, BlobRec *blobs, size_t stride, unsigned *counts) {
  __shared__ unsigned wsum[16];
  __shared__ unsigned carry_s;
  const unsigned tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const unsigned total = info[(size_t)blockIdx.x * kBlobInfo];
  if (wrap && total >= kBlobCapMax) { /* whole block */
    if (tid == 0) counts[blockIdx.x] = 0;
    return;
  }
  const unsigned last = total < cap ? total : cap;
  const unsigned *sf = stats + (size_t)blockIdx.x * nslot * kBlobSlot;
  BlobRec *out = blobs + (size_t)blockIdx.x * stride;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (unsigned base = 1; base <= last; base += 1024u) {
    const unsigned L = base + tid;
    const unsigned *s = sf + (size_t)L * kBlobSlot;
    const unsigned area = L <= last ? s[0] : 0u, v = area ? 1u : 0u;
    const unsigned inc = wave_incl_scan(v);
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    unsigned woff = 0;
    for (unsigned k = 0; k < wv; k++) woff += wsum[k];
    const unsigned carry = carry_s;
    if (v) {
      const unsigned minx = ~s[1], miny = ~s[2];
      out[carry + woff + inc - 1u] = BlobRec{L, area, minx, miny, s[3] - minx + 1u, s[4] - miny + 1u, s[5] / area, s[6] / area};
    }
    __syncthreads();
    if (tid == 1023) carry_s = carry + woff + inc;
    __syncthreads();
  }
  if (tid == 0) counts[blockIdx.x] = carry_s;
}

/* ---- gs_blob_corners (ref :404-421) ----------------------------------------------------------------------------- */
/* keys: tl = min (x + y, y), br = max (x + y, ~y), bl = min (x - y, y), tr = max (x - y, ~y); sums and differences as
 * the reference's int, mapped to order-preserving u32.  The low half makes the first pixel in (y, x) order win ties. */
constexpr unsigned kCornerKeys = 4;
GS_DEV uint32_t ord_i32(int v) { return (uint32_t)v ^ 0x80000000u; }

/* grid (frames), block 64: keys to their empty values */
__global__ __launch_bounds__(64) void k_corners_init(unsigned long long *keys) {
  if (threadIdx.x < kCornerKeys) keys[(size_t)blockIdx.x * kCornerKeys + threadIdx.x] = (threadIdx.x & 1u) ? 0ull : ~0ull;
}

/* grid (blocks, frames), block 256: waves take rows of the box, lanes columns */
__global__ __launch_bounds__(256) void k_corners(const uint8_t *img, const uint16_t *labels, unsigned w, unsigned h,
                                                 const BlobRec *blobs, unsigned long long *keys) {
  __shared__ unsigned long long part[4][kCornerKeys];
  const unsigned wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const BlobRec b = blobs[blockIdx.y];
  const size_t fo = (size_t)blockIdx.y * w * h;
  /* the reference's loops: y from box.y while y < box.y + box.h (u32), likewise x; gs_get skips pixels outside */
  const unsigned ey = b.by + b.bh, ex = b.bx + b.bw;
  const unsigned y1 = ey < h ? ey : h, x1 = ex < w ? ex : w;
  unsigned long long tl = ~0ull, br = 0ull, bl = ~0ull, tr = 0ull;
  if (ey > b.by && ex > b.bx && b.by < y1 && b.bx < x1) {
    for (unsigned y = b.by + blockIdx.x * 4u + wv; y < y1; y += gridDim.x * 4u) {
      const uint8_t *ir = img + fo + (size_t)y * w;
      const uint16_t *lr = labels + fo + (size_t)y * w;
      for (unsigned x = b.bx + lane; x < x1; x += 64u) {
        if (ir[x] < 128 || lr[x] != (uint16_t)b.label) continue;
        const uint32_t s = ord_i32((int)x + (int)y), d = ord_i32((int)x - (int)y);
        const unsigned long long ks = (unsigned long long)s << 32, kd = (unsigned long long)d << 32;
        const unsigned long long ktl = ks | y, kbr = ks | (uint32_t)~y, kbl = kd | y, ktr = kd | (uint32_t)~y;
        tl = ktl < tl ? ktl : tl;
        br = kbr > br ? kbr : br;
        bl = kbl < bl ? kbl : bl;
        tr = ktr > tr ? ktr : tr;
      }
    }
  }
  tl = wave_min_u64(tl), br = wave_max_u64(br), bl = wave_min_u64(bl), tr = wave_max_u64(tr);
  if (lane == 0) part[wv][0] = tl, part[wv][1] = br, part[wv][2] = bl, part[wv][3] = tr;
  __syncthreads();
  if (threadIdx.x < kCornerKeys) {
    const unsigned i = threadIdx.x;
    unsigned long long v = part[0][i];
    for (unsigned k = 1; k < 4u; k++) v = (i & 1u) ? (part[k][i] > v ? part[k][i] : v) : (part[k][i] < v ? part[k][i] : v);
    unsigned long long *dst = keys + (size_t)blockIdx.y * kCornerKeys + i;
    if ((i & 1u) ? v != 0ull : v != ~0ull) {
      if (i & 1u) atomicMax(dst, v);
      else atomicMin(dst, v);
    }
  }
}

/* grid (frames), block 64: corners = {tl, tr, br, bl} (struct gs_point[4]); the centroid four times without a pixel */
__global__ __launch_bounds__(64) void k_corners_final(const unsigned long long *keys, const BlobRec *blobs, uint32_t *corners) {
  if (threadIdx.x != 0) return;
  const unsigned long long *k = keys + (size_t)blockIdx.x * kCornerKeys;
  const BlobRec b = blobs[blockIdx.x];
  uint32_t *c = corners + (size_t)blockIdx.x * 8u;
  if (k[0] == ~0ull) {
    for (unsigned i = 0; i < 4u; i++) c[2 * i] = b.cx, c[2 * i + 1] = b.cy;
    return;
  }
  const uint32_t tly = (uint32_t)k[0], bry = ~(uint32_t)k[1], bly = (uint32_t)k[2], try_ = ~(uint32_t)k[3];
  const uint32_t tls = (uint32_t)(k[0] >> 32) ^ 0x80000000u, brs = (uint32_t)(k[1] >> 32) ^ 0x80000000u;
  const uint32_t bld = (uint32_t)(k[2] >> 32) ^ 0x80000000u, trd = (uint32_t)(k[3] >> 32) ^ 0x80000000u;
  c[0] = tls - tly, c[1] = tly;   /* tl: x = (x + y) - y */
  c[2] = trd + try_, c[3] = try_; /* tr: x = (x - y) + y */
  c[4] = brs - bry, c[5] = bry;   /* br */
  c[6] = bld + bly, c[7] = bly;   /* bl */
}

/* ---- gs_perspective_correct (ref :423-444) ------------------------------------------------------------------------ */
GS_DEV unsigned persp_px(const uint8_t *img, unsigned w, unsigned h, unsigned x, unsigned y) {
  return (x < w && y < h) ? img[(size_t)y * w + x] : 0u; /* gs_get (ref :143-145) */
}
/* grid (ceil(dw / 64), ceil(dh / 4), frames), block (64, 4): the reference's float32 expression, operation for operation
 * (no contraction, correctly rounded division, GS_MIN / GS_MAX as ternaries: a NaN coordinate clamps to src.w - 1) */
__global__ __launch_bounds__(256) void k_perspective(uint8_t *dst, unsigned dw, unsigned dh, const uint8_t *src, unsigned sw,
                                                     unsigned sh, const uint32_t *corners) {
#ifndef GS_EMU
#pragma clang fp contract(off)
#endif
  const unsigned x = blockIdx.x * 64u + threadIdx.x, y = blockIdx.y * 4u + threadIdx.y;
  if (x >= dw || y >= dh) return;
  const uint32_t *c = corners + (size_t)blockIdx.z * 8u;
  const uint8_t *s = src + (size_t)blockIdx.z * sw * sh;
  const float w = (float)dw - 1.0f, h = (float)dh - 1.0f;
  const float u = (float)x / w, v = (float)y / h;
  const float c0x = (float)c[0], c0y = (float)c[1], c1x = (float)c[2], c1y = (float)c[3];
  const float c2x = (float)c[4], c2y = (float)c[5], c3x = (float)c[6], c3y = (float)c[7];
  const float top_x = c0x * (1 - u) + c1x * u;
  const float top_y = c0y * (1 - u) + c1y * u;
  const float bot_x = c3x * (1 - u) + c2x * u;
  const float bot_y = c3y * (1 - u) + c2y * u;
  float src_x = top_x * (1 - v) + bot_x * v;
  float src_y = top_y * (1 - v) + bot_y * v;
  const float mx = (float)sw - 1.0f, my = (float)sh - 1.0f;
  src_x = src_x < mx ? src_x : mx, src_x = 0.0f > src_x ? 0.0f : src_x;
  src_y = src_y < my ? src_y : my, src_y = 0.0f > src_y ? 0.0f : src_y;
  const unsigned sx = (unsigned)src_x, sy = (unsigned)src_y;
  const unsigned sx1 = sx + 1 < sw - 1 ? sx + 1 : sw - 1, sy1 = sy + 1 < sh - 1 ? sy + 1 : sh - 1;
  const float dx = src_x - (float)sx, dy = src_y - (float)sy;
  const int c00 = (int)persp_px(s, sw, sh, sx, sy), c01 = (int)persp_px(s, sw, sh, sx1, sy);
  const int c10 = (int)persp_px(s, sw, sh, sx, sy1), c11 = (int)persp_px(s, sw, sh, sx1, sy1);
  const float p = ((float)c00 * (1 - dx) * (1 - dy)) + ((float)c01 * dx * (1 - dy)) + ((float)c10 * (1 - dx) * dy) +
                  ((float)c11 * dx * dy);
  dst[(size_t)blockIdx.z * dw * dh + (size_t)y * dw + x] = (uint8_t)(int)p; /* float -> uint8_t truncation (value < 256) */
}

/* ---- gsh_blob_largest_batch: the scan chain's "largest blob" (ref nanomagick.c:196-199) ---------------------------- */
/* grid (frames), block 64 or 256: the FIRST record of maximum area among the first min(counts[f], nblobs) -- the
 * reference's strict `>` -- as the maximum of the keys (area << 32) | ~index, like k_argmax_first (k_geom.h).  No record:
 * largest[f] = 32 zero bytes, index[f] = 0xffffffff (the reference reads an uninitialised record there). */
__global__ __launch_bounds__(256) void k_blob_largest(const BlobRec *blobs, unsigned nblobs, const unsigned *counts,
                                                      BlobRec *largest, unsigned *index) {
  __shared__ unsigned long long part[4];
  const unsigned tid = threadIdx.x, nw = blockDim.x >> 6;
  const BlobRec *bf = blobs + (size_t)blockIdx.x * nblobs;
  const unsigned c = counts[blockIdx.x], cnt = c < nblobs ? c : nblobs;
  unsigned long long best = 0; /* below every key: ~i = 0 needs i = 0xffffffff >= cnt */
  for (unsigned i = tid; i < cnt; i += blockDim.x) {
    const unsigned long long key = ((unsigned long long)bf[i].area << 32) | (0xffffffffu - i);
    best = key > best ? key : best;
  }
  best = wave_max_u64(best);
  if ((tid & 63u) == 0) part[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    for (unsigned q = 1; q < nw; q++) best = part[q] > best ? part[q] : best;
    part[0] = best;
  }
  __syncthreads();
  const unsigned at = 0xffffffffu - (unsigned)part[0]; /* cnt == 0: part[0] == 0, at == 0xffffffff */
  if (tid < 8u) ((uint32_t *)(largest + blockIdx.x))[tid] = cnt ? ((const uint32_t *)(bf + at))[tid] : 0u;
  if (tid == 0 && index) index[blockIdx.x] = at;
}

/* ---- gsh_blob_paint_batch: the picture nanomagick's `blobs` verb draws (ref nanomagick.c:160-169) ------------------
 * dst = 0; every record's padded box := 128; every pixel with img > 128 := 255.  The reference's loops are INCLUSIVE
 * (y1 <= y <= y2, x1 <= x <= x2, x2 <= w, y2 <= h) and write the linear index y * w + x, so a box that reaches the right
 * edge also paints column 0 of the next row, and one that reaches the bottom addresses indices >= w * h: the reference
 * writes past its buffer there, the library drops them.  So a box is a set of SPANS of the frame's linear index, one per
 * row y: [y w + x1, y w + x2] cut at w h, and the kernel works on the linear index throughout.
 *
 * One pass, 2 B/px: a block owns a band of R rows of one frame (linear range [r0 w, r1 w)).  It builds the band's coverage
 * as one BIT per pixel in LDS -- the spans of the records that reach the band are OR-ed in word-wise -- and then streams
 * the band: 16 bytes of img in, 16 bytes of dst out per lane-step (dst chunks 16-byte aligned, bit 0 of the coverage is the
 * byte at dst's band address rounded down to 16, so a chunk's 16 bits are one half of one LDS word; the ragged ends of
 * the band go bytewise).
 *
 * Records: lanes read 256 records per step.  Records are in label order = raster order of each blob's first pixel, which
 * lies in row box.y: box.y never decreases, so a wave stops after the step in which it saw a padded box that starts
 * at or below the band's end.  A lane ORs a small box itself; a box of more than kPaintOwn (row, word) pairs in the band
 * is handed to its wave, whose 64 lanes share the pairs (a frame-filling box: ~2000 ORs per band, 33 per lane), and the
 * bands of a frame are independent blocks -- nothing serialises on one wave. */
constexpr unsigned kPaintWords = 2048;            /* coverage words per block: 8 KB of LDS, 8 blocks of 256 per CU */
constexpr unsigned kPaintBits = kPaintWords * 32; /* a band has at most kPaintBits - 15 pixels (15: the alignment phase) */
constexpr unsigned kPaintOwn = 8;                 /* (row, word) pairs a lane ORs alone */

/* per byte: x > 128 ? 0xff : 0 (bit 7 set and a low bit set) */
GS_DEV uint32_t gt128_bytes(uint32_t x) { return ((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) & x & 0x80808080u) >> 7) * 0xffu; }
/* 4 coverage bits -> 128 in the covered bytes (bit i -> byte i) */
GS_DEV uint32_t cov_bytes4(uint32_t b) { return (((b & 0xfu) * 0x00204081u) & 0x01010101u) << 7; }

/* the reference's bounds in its own mixed arithmetic (nanomagick.c:162-164): x1, y1 through int, x2, y2 in wrapping u32 */
struct PaintBox {
  unsigned x1, y1, x2, y2;
};
GS_DEV PaintBox paint_box(const BlobRec &b, unsigned w, unsigned h) {
  const int ix = (int)(b.bx - 2u), iy = (int)(b.by - 2u);
  const unsigned ex = b.bx + b.bw + 2u, ey = b.by + b.bh + 2u;
  return PaintBox{ix > 0 ? (unsigned)ix : 0u, iy > 0 ? (unsigned)iy : 0u, ex < w ? ex : w, ey < h ? ey : h};
}
/* row y of a box as coverage bits of the band [lo, hi) (bit = linear index - lo + ph): false when it misses the band */
GS_DEV bool paint_row_bits(unsigned y, unsigned x1, unsigned x2, unsigned w, size_t lo, size_t hi, unsigned ph, unsigned &a,
                           unsigned &b) {
  size_t s = (size_t)y * w + x1, e = (size_t)y * w + x2;
  s = s < lo ? lo : s;
  if (e >= hi) e = hi - 1; /* hi > lo >= 0 */
  if (s > e || e < lo) return false;
  a = (unsigned)(s - lo) + ph, b = (unsigned)(e - lo) + ph;
  return true;
}

/* grid (ceil(h / R), frames), block 256; R * w + 15 <= kPaintBits */
__global__ __launch_bounds__(256) void k_blob_paint(uint8_t *dst, const uint8_t *img, unsigned w, unsigned h, unsigned R,
                                                    const BlobRec *blobs, unsigned nblobs, const unsigned *counts) {
  __shared__ uint32_t cov[kPaintWords];
  const unsigned tid = threadIdx.x, lane = tid & 63u;
  const unsigned r0 = blockIdx.x * R, r1 = r0 + R < h ? r0 + R : h;
  const size_t np = (size_t)w * h, lo = (size_t)r0 * w, hi = (size_t)r1 * w;
  if (r0 >= h) return; /* whole block */
  uint8_t *d = dst + (size_t)blockIdx.y * np + lo;
  const uint8_t *s = img + (size_t)blockIdx.y * np + lo;
  const uintptr_t a0 = (uintptr_t)d & ~(uintptr_t)15;
  const unsigned ph = (unsigned)((uintptr_t)d - a0);
  const size_t nbits = (size_t)ph + (hi - lo);
  if (nbits > kPaintBits) return; /* the launcher never asks for it */
  const unsigned nwords = (unsigned)((nbits + 31u) / 32u);
  for (unsigned k = tid; k < nwords; k += 256u) cov[k] = 0u;
  __syncthreads();

  const BlobRec *bf = blobs + (size_t)blockIdx.y * nblobs;
  const unsigned c = counts[blockIdx.y], cnt = c < nblobs ? c : nblobs;
  for (unsigned base = 0; base < cnt; base += 256u) { /* block-uniform bound, wave-uniform exit */
    const unsigned i = base + tid;
    bool below = false, hit = false;
    unsigned x1 = 0, x2 = 0, ya = 0, yb = 0;
    if (i < cnt) {
      const PaintBox p = paint_box(bf[i], w, h);
      below = p.y1 >= r1;
      if (!below && p.x1 <= p.x2 && p.y1 <= p.y2) {
        /* the rows whose spans reach the band: its own, and the one above when the span wraps to column 0 (x2 == w) */
        const unsigned first = (r0 > 0 && p.x2 == w) ? r0 - 1u : r0;
        ya = p.y1 > first ? p.y1 : first, yb = p.y2 < r1 - 1u ? p.y2 : r1 - 1u;
        hit = ya <= yb;
        x1 = p.x1, x2 = p.x2;
      }
    }
    const unsigned wpr = (x2 - x1) / 32u + 2u; /* words a row's span can touch */
    const bool own = hit && (yb - ya + 1u) * wpr <= kPaintOwn;
    if (own) {
      for (unsigned y = ya; y <= yb; y++) {
        unsigned a, b;
        if (!paint_row_bits(y, x1, x2, w, lo, hi, ph, a, b)) continue;
        const uint32_t ma = ~0u << (a & 31u), mb = ~0u >> (31u - (b & 31u));
        const unsigned wa = a >> 5, wb = b >> 5;
        if (wa == wb) {
          atomicOr(&cov[wa], ma & mb);
        } else {
          atomicOr(&cov[wa], ma);
          for (unsigned k = wa + 1u; k < wb; k++) atomicOr(&cov[k], ~0u);
          atomicOr(&cov[wb], mb);
        }
      }
    }
    uint64_t big = ballot(hit && !own);
    while (big) { /* wave-uniform: the wave's lanes share one large box's (row, word) pairs */
      const unsigned src = (unsigned)__builtin_ctzll(big);
      big &= big - 1ull;
      const unsigned X1 = readlane_at(x1, src), X2 = readlane_at(x2, src), YA = readlane_at(ya, src), YB = readlane_at(yb, src);
      const unsigned per = (X2 - X1) / 32u + 2u, total = (YB - YA + 1u) * per;
      for (unsigned t = lane; t < total; t += 64u) {
        const unsigned row = t / per, k = t - row * per;
        unsigned a, b;
        if (!paint_row_bits(YA + row, X1, X2, w, lo, hi, ph, a, b)) continue;
        const unsigned wa = a >> 5, wb = b >> 5, word = wa + k;
        if (word > wb) continue;
        uint32_t m = ~0u;
        if (word == wa) m &= ~0u << (a & 31u);
        if (word == wb) m &= ~0u >> (31u - (b & 31u));
        atomicOr(&cov[word], m);
      }
    }
    if (ballot(below)) break;
  }
  __syncthreads();

  /* stream the band: chunk ci = bytes [16 ci, 16 ci + 16) from a0 = coverage bits 16 ci .. 16 ci + 15 */
  const size_t nch = (nbits + 15u) / 16u;
  const bool same_phase = ((((uintptr_t)s) ^ ((uintptr_t)d)) & 15u) == 0u;
  for (size_t ci = tid; ci < nch; ci += 256u) {
    const size_t b0 = ci * 16u;
    const uint32_t bits = (cov[ci >> 1] >> (16u * (unsigned)(ci & 1u))) & 0xffffu;
    if (b0 >= ph && b0 + 16u <= nbits) {
      uint8_t *p = (uint8_t *)(a0 + b0);
      const uint8_t *q = s + (b0 - ph);
      U4 v;
#ifndef GS_EMU
      typedef unsigned int v4u __attribute__((ext_vector_type(4)));
      if (same_phase) { /* read once, written once: stream both (k_threshold) */
        const v4u t = __builtin_nontemporal_load((const v4u *)q);
        v = U4{t.x, t.y, t.z, t.w};
      } else {
        v = load_u32x4_any(q);
      }
#else
      (void)same_phase;
      v = load_u32x4_any(q);
#endif
      v.x = gt128_bytes(v.x) | cov_bytes4(bits), v.y = gt128_bytes(v.y) | cov_bytes4(bits >> 4);
      v.z = gt128_bytes(v.z) | cov_bytes4(bits >> 8), v.w = gt128_bytes(v.w) | cov_bytes4(bits >> 12);
#ifndef GS_EMU
      __builtin_nontemporal_store(v4u{v.x, v.y, v.z, v.w}, (v4u *)p);
#else
      store_u32x4(p, v);
#endif
    } else { /* the band's ragged first / last chunk */
      const size_t k0 = b0 < ph ? ph : b0, k1 = b0 + 16u > nbits ? nbits : b0 + 16u;
      for (size_t k = k0; k < k1; k++) d[k - ph] = s[k - ph] > 128 ? 255 : ((bits >> (unsigned)(k - b0)) & 1u) ? 128 : 0;
    }
  }
}

/* Frames wider than kPaintBits - 15 pixels (not one row's bits fit the block's LDS): dst = img > 128 ? 255 : 0, then the
 * boxes' pixels that are not 255 := 128, two plain passes.  grid (blocks, frames), block 256. */
__global__ __launch_bounds__(256) void k_blob_paint_base(uint8_t *dst, const uint8_t *img, size_t np) {
  uint8_t *d = dst + (size_t)blockIdx.y * np;
  const uint8_t *s = img + (size_t)blockIdx.y * np;
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < np; i += (size_t)gridDim.x * 256u) d[i] = s[i] > 128 ? 255 : 0;
}
__global__ __launch_bounds__(256) void k_blob_paint_fill(uint8_t *dst, const uint8_t *img, unsigned w, unsigned h,
                                                         const BlobRec *blobs, unsigned nblobs, const unsigned *counts) {
  const size_t np = (size_t)w * h;
  uint8_t *d = dst + (size_t)blockIdx.y * np;
  const uint8_t *s = img + (size_t)blockIdx.y * np;
  const BlobRec *bf = blobs + (size_t)blockIdx.y * nblobs;
  const unsigned c = counts[blockIdx.y], cnt = c < nblobs ? c : nblobs;
  for (unsigned i = blockIdx.x; i < cnt; i += gridDim.x) {
    const PaintBox p = paint_box(bf[i], w, h);
    if (p.x1 > p.x2 || p.y1 > p.y2) continue;
    const size_t bw = (size_t)(p.x2 - p.x1) + 1u, total = bw * ((size_t)(p.y2 - p.y1) + 1u);
    for (size_t t = threadIdx.x; t < total; t += 256u) {
      const size_t row = t / bw, at = ((size_t)p.y1 + row) * w + p.x1 + (t - row * bw);
      if (at < np && !(s[at] > 128)) d[at] = 128;
    }
  }
}

}  // namespace gs
#endif
