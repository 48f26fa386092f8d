/*
 * k_match.h -- gsh_match_orb_batch: gs_match_orb (grayskull.h:680-699) for n pairs of keypoint sets in one launch.
 *
 * k_match (k_orb.h) gives a WAVE to a query and lets every lane fetch whole train descriptors: 32 bytes of vector loads
 * per (query, train) pair.  Here the loop is turned inside out: a LANE owns a query -- its 8 descriptor dwords and its
 * (best, second, arg) state stay in registers -- and the train descriptors reach the ALU wave-uniformly, so a pair costs
 * the XORs, the accumulating popcounts and the state update and no vector memory instruction: the wave stages kMatchTile
 * descriptors in LDS (one per lane, 2 KiB, a region of its own: no block barrier) and every lane reads them back at ONE
 * address -- a broadcast, no bank conflict; the next tile's global loads are in flight while the current one is compared.
 * (The other wave-uniform form, s_load_dwordx8 into SGPRs that are the v_xor operands, measured the same within the run-to-run
 * spread and was not kept: docs/design/detectors.md, "Descriptor matching over a batch".)
 *
 * A block takes 64 queries of one pair (one word of the compaction mask); its kMatchSlices waves cut the pair's train range
 * into as many contiguous slices.  A lane visits its slice in ascending order, so the strict `<` of ref :690 keeps the first
 * minimum; the waves' states then merge through LDS by the rule above k_match (k_orb.h), which gives the sequential loop's
 * result for any order: best = min, second = min(max of the bests, both seconds), arg = that of the smaller best, the lower
 * index on ties.
 *
 * Distances are integers 0..256, so the state is kept in integers: for an integer d and the reference's float start value
 * init = max_distance + 1, d < init <=> d < ceil(init), and a stored value equals ceil(init) only while it still IS the
 * start value (a distance has to be smaller to get in).  kMatchFar stands for a start value above 256, 0 for one that no
 * distance is below (init <= 0, NaN).  The acceptance test of ref :695 is then made in float on init or (float)d -- the
 * same operands the reference compares.
 */
#ifndef GS_K_MATCH_H
#define GS_K_MATCH_H
#include <math.h>

#include "k_compact.h"

namespace gs {

constexpr unsigned kMatchTile = 64;   /* train descriptors per staged tile: one per lane */
constexpr unsigned kMatchSlices = 16; /* waves per block = slices of a pair's train range */
constexpr unsigned kMatchFar = 0xffffffffu;

struct MatchState { unsigned best, second, arg; };

/* the body of ref :690-693 for the next index of an ascending walk */
GS_DEV void match_visit(MatchState &s, unsigned d, unsigned j) {
  s.second = umin(s.second, umax(d, s.best));
  if (d < s.best) s.arg = j;
  s.best = umin(s.best, d);
}
GS_DEV void match_merge(MatchState &s, const MatchState &o) {
  s.second = umin(umin(s.second, o.second), umax(s.best, o.best));
  if (o.best < s.best || (o.best == s.best && o.arg < s.arg)) s.arg = o.arg;
  s.best = umin(s.best, o.best);
}

/* grid (ceil(cap1 / 64), pairs of the launch), block 64 * kMatchSlices.  Pair p reads set p * per1 of k1 (per1 = 0: one
 * query set for all pairs) and set p * per2 of k2; n1 / n2 (NULL: cap records) are read here, clamped to cap.  Leaves
 * best_idx / best_dist [p * cap1 + query] of the accepted queries, bit (query % 64) of mask word p * nchunks * kChunkWords +
 * query / 64 and the chunk counters; mask and counters pre-zeroed (the blocks beyond a pair's count write nothing). */
__global__ __launch_bounds__(64 * kMatchSlices) void k_match_batch(
    const uint32_t *__restrict__ k1, unsigned cap1, const unsigned *__restrict__ n1, unsigned per1,
    const uint32_t *__restrict__ k2, unsigned cap2, const unsigned *__restrict__ n2, unsigned per2, float max_distance,
    unsigned *__restrict__ best_idx, unsigned *__restrict__ best_dist, unsigned long long *__restrict__ mask,
    unsigned *__restrict__ chunk_count, unsigned nchunks) {
  __shared__ __attribute__((aligned(16))) uint32_t tile[kMatchSlices][kMatchTile * 8];
  __shared__ unsigned m_best[kMatchSlices][64], m_second[kMatchSlices][64], m_arg[kMatchSlices][64];
  const unsigned p = blockIdx.y, lane = threadIdx.x & 63u, wv = uniform(threadIdx.x >> 6);
  const unsigned s1 = p * per1, s2 = p * per2;
  const unsigned nq = n1 ? umin(n1[s1], cap1) : cap1, nt = n2 ? umin(n2[s2], cap2) : cap2;
  const unsigned q = blockIdx.x * 64u + lane;
  if (blockIdx.x * 64u >= nq) return; /* whole block */
  uint32_t d1[8];
  {
    const uint32_t *qd = k1 + ((size_t)s1 * cap1 + umin(q, nq - 1u)) * 12u + 4; /* lanes beyond the count: a copy of the last query, never accepted */
#pragma unroll
    for (int i = 0; i < 8; i++) d1[i] = qd[i];
  }
  const float init = max_distance + 1; /* ref :686 */
  const unsigned ci = !(init > 0.0f) ? 0u : init > 256.0f ? kMatchFar : (unsigned)ceilf(init);
  MatchState st{ci, ci, 0u};
  const unsigned len = (nt - 1u) / kMatchSlices + 1u; /* nt == 0: every slice is empty whatever len is */
  const unsigned long long lo = (unsigned long long)wv * len;
  const unsigned j0 = lo < nt ? (unsigned)lo : nt, j1 = nt - j0 < len ? nt : j0 + len; /* this wave's slice [j0, j1) */
  const uint32_t *t = k2 + (size_t)s2 * cap2 * 12u + 4;
  uint32_t *mine = tile[wv];
  uint32_t nx[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (lane < j1 - j0) {
#pragma unroll
    for (int i = 0; i < 8; i++) nx[i] = t[(size_t)(j0 + lane) * 12u + i];
  }
  for (unsigned b = j0; b < j1; b += kMatchTile) { /* wave-uniform */
    const unsigned cnt = umin(kMatchTile, j1 - b);
    wave_sync(); /* every lane has finished with the tile before */
#pragma unroll
    for (int i = 0; i < 8; i++) mine[lane * 8u + i] = nx[i];
    wave_sync();
    if (j1 - b > kMatchTile && lane < j1 - b - kMatchTile) { /* the next tile's loads fly under this tile's compares */
#pragma unroll
      for (int i = 0; i < 8; i++) nx[i] = t[(size_t)(b + kMatchTile + lane) * 12u + i];
    }
    /* two descriptors per trip, read one trip ahead (one address for the wave: a broadcast); the read-ahead wraps
     * inside the tile, its surplus is never used.  The register copies at the end of a trip cost less than they look: a trip
     * with two register sets in turn and no copy has 25 instead of 30 vector instructions per pair, but hipcc then waits
     * for ALL outstanding LDS reads right behind the read-ahead, and the launch takes 8 % longer (detectors.md) */
    uint32_t cur[16], nxt[16];
#pragma unroll
    for (int i = 0; i < 16; i++) cur[i] = mine[i];
    for (unsigned u = 0; u < cnt; u += 2u) {
      const unsigned un = ((u + 2u) & (kMatchTile - 1u)) * 8u;
#pragma unroll
      for (int i = 0; i < 16; i++) nxt[i] = mine[un + i];
      sched_fence();
      unsigned da = 0, db = 0;
#pragma unroll
      for (int i = 0; i < 8; i++) da += (unsigned)__popc(d1[i] ^ cur[i]), db += (unsigned)__popc(d1[i] ^ cur[8 + i]);
      match_visit(st, da, b + u);
      if (u + 1u < cnt) match_visit(st, db, b + u + 1u);
#pragma unroll
      for (int i = 0; i < 16; i++) cur[i] = nxt[i];
    }
  }
  m_best[wv][lane] = st.best, m_second[wv][lane] = st.second, m_arg[wv][lane] = st.arg;
  __syncthreads();
  if (wv != 0) return;
  for (unsigned w = 1; w < kMatchSlices; w++) match_merge(st, MatchState{m_best[w][lane], m_second[w][lane], m_arg[w][lane]});
  const float bf = st.best == ci ? init : (float)st.best, sf = st.second == ci ? init : (float)st.second;
  const bool ok = q < nq && bf <= max_distance && bf < 0.8f * sf; /* ref :695, in float */
  if (ok) {
    const size_t qi = (size_t)p * cap1 + q;
    best_idx[qi] = st.arg, best_dist[qi] = st.best;
  }
  publish_flags(ok, mask + (size_t)p * nchunks * kChunkWords, chunk_count + (size_t)p * nchunks, blockIdx.x);
}

/* compaction functor: query `item` of pair `frame` -> gs_match {item, best_idx, distance} (ref :696) */
struct MatchBatchEmit {
  const unsigned *best_idx, *best_dist;
  unsigned cap1;
  unsigned *matches; /* pairs x max_matches x 3 u32 */
  unsigned max_matches;
  GS_DEV void operator()(unsigned frame, size_t item, unsigned r) const {
    unsigned *o = matches + ((size_t)frame * max_matches + r) * 3u;
    const size_t qi = (size_t)frame * cap1 + item;
    o[0] = (unsigned)item, o[1] = best_idx[qi], o[2] = best_dist[qi];
  }
};

}  // namespace gs
#endif
