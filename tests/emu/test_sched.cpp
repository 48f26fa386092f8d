/* tests/emu/test_sched.cpp -- the emulator's schedules (hip_emu.h, SCHEDULES), checked without any kernel of the library.
 *
 * A switch that silently did nothing would let every test that runs kernels "under a schedule" pass, so this program
 * logs the order in which emu::launch really runs blocks and threads:
 *   - every block runs exactly once and every thread of every block runs, for every kind of either order;
 *   - kinds 0..2 give exactly the promised order (ascending, descending, outside-in);
 *   - kind 3 gives a permutation that is the same for the same seed, another one for another seed, and a new one for
 *     every launch;
 *   - a kernel with __syncthreads(), a wave exchange and a quad exchange in a loop terminates under every kind and
 *     computes what it should.
 * Built and run by tests/test_emu_schedules.py:  g++ -DGS_EMU -std=c++17 -O1 test_sched.cpp hip_emu.cpp
 * Usage: test_sched        all checks, prints "all passed"
 *        test_sched env    prints the schedule that GS_EMU_SCHEDULE selected and the block order of a 5-block launch
 */
#include "hip_emu.h"

#include <utility>

struct Log {
  std::vector<std::pair<unsigned, unsigned>> v; /* (linear block, linear thread) in order of execution */
};

static unsigned lin_block() { return blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z); }
static unsigned lin_thread() { return threadIdx.x + blockDim.x * (threadIdx.y + blockDim.y * threadIdx.z); }

__global__ void k_log(Log *log) { log->v.emplace_back(lin_block(), lin_thread()); }

/* per iteration: barrier, sum over the wave, swap inside the quad, barrier-protected LDS hand-over to the next thread */
__global__ void k_sync_loop(unsigned long long *out, unsigned iters) {
  __shared__ unsigned long long hand[1024];
  const unsigned t = lin_thread(), nt = blockDim.x * blockDim.y * blockDim.z;
  unsigned long long acc = t + 1;
  for (unsigned i = 0; i < iters; i++) {
    hand[t] = acc;
    __syncthreads();
    const unsigned long long left = hand[(t + 1) % nt];
    __syncthreads();
    const unsigned long long wsum = emu::wave_exchange(left & 0xffffu, [](const uint64_t *slot, const bool *valid) {
      unsigned long long s = 0;
      for (int l = 0; l < emu::WAVE; l++)
        if (valid[l]) s += slot[l];
      return s;
    });
    unsigned sel = (t + 1) & 3u; /* a lane that exists: the last quad of a 65-thread block has one */
    if (t / 4 * 4 + sel >= nt) sel = t & 3u;
    const unsigned long long q = emu::quad_exchange(left, sel);
    acc = left * 3 + wsum + (q & 0xffu) + i;
  }
  out[(size_t)lin_block() * nt + t] = acc;
}

/* the same arithmetic, thread by thread */
static std::vector<unsigned long long> sync_loop_expected(unsigned nt, unsigned iters) {
  std::vector<unsigned long long> acc(nt), left(nt), next(nt);
  for (unsigned t = 0; t < nt; t++) acc[t] = t + 1;
  for (unsigned i = 0; i < iters; i++) {
    for (unsigned t = 0; t < nt; t++) left[t] = acc[(t + 1) % nt];
    for (unsigned t = 0; t < nt; t++) {
      unsigned long long wsum = 0;
      for (unsigned l = t / 64 * 64; l < t / 64 * 64 + 64 && l < nt; l++) wsum += left[l] & 0xffffu;
      unsigned src = t / 4 * 4 + ((t + 1) & 3u);
      if (src >= nt) src = t;
      const unsigned long long q = left[src];
      next[t] = left[t] * 3 + wsum + (q & 0xffu) + i;
    }
    acc = next;
  }
  return acc;
}

static uint64_t promised(int kind, uint64_t n, uint64_t i) {
  return kind == 1 ? n - 1 - i : kind == 2 ? ((i & 1) ? n - 1 - i / 2 : i / 2) : i;
}

static int failures = 0;
#define CHECK(cond, ...)                  \
  do {                                    \
    if (!(cond)) {                        \
      if (failures++ < 20) {              \
        fprintf(stderr, "FAILED: ");      \
        fprintf(stderr, __VA_ARGS__);     \
        fprintf(stderr, "\n");            \
      }                                   \
    }                                     \
  } while (0)

static Log run_log(dim3 grid, dim3 block) {
  Log log;
  Log *p = &log;
  log.v.reserve((size_t)grid.x * grid.y * grid.z * block.x * block.y * block.z);
  GS_LAUNCH(k_log, grid, block, 0, nullptr, p);
  return log;
}

/* every (block, thread) once; a block's threads in one run; returns the order of the blocks */
static std::vector<unsigned> check_complete(const Log &log, unsigned nb, unsigned nt, const char *what) {
  std::vector<unsigned> border;
  CHECK(log.v.size() == (size_t)nb * nt, "%s: %zu log entries for %u x %u", what, log.v.size(), nb, nt);
  if (log.v.size() != (size_t)nb * nt) return border;
  std::vector<char> seen((size_t)nb * nt, 0);
  for (size_t i = 0; i < log.v.size(); i++) {
    const unsigned b = log.v[i].first, t = log.v[i].second;
    CHECK(b < nb && t < nt, "%s: entry (%u, %u) out of range", what, b, t);
    if (b >= nb || t >= nt) return border;
    CHECK(!seen[(size_t)b * nt + t], "%s: (%u, %u) ran twice", what, b, t);
    seen[(size_t)b * nt + t] = 1;
    if (i % nt == 0) border.push_back(b);
    else CHECK(b == border.back(), "%s: block %u interleaved with block %u", what, b, border.back());
  }
  return border;
}

static void check_config(dim3 grid, unsigned nt, int kb, int kt) {
  const unsigned nb = grid.x * grid.y * grid.z;
  char what[128];
  snprintf(what, sizeof what, "grid %ux%ux%u block %u kinds (%d, %d)", grid.x, grid.y, grid.z, nt, kb, kt);
  /* a two-dimensional block for the sizes that allow it: tid.x / tid.y must follow the linear index */
  const dim3 block = nt % 4 == 0 ? dim3(nt / 4, 2, 2) : dim3(nt);
  emu::set_schedule(kb, kt, 12345);
  const Log a = run_log(grid, block);
  const Log a2 = run_log(grid, block); /* second launch after the same set_schedule */
  const std::vector<unsigned> border = check_complete(a, nb, nt, what);
  check_complete(a2, nb, nt, what);
  if (border.size() != nb) return;
  if (kb < 3)
    for (unsigned i = 0; i < nb; i++) CHECK(border[i] == promised(kb, nb, i), "%s: block %u ran at position %u", what, border[i], i);
  if (kt < 3)
    for (size_t i = 0; i < a.v.size(); i++)
      CHECK(a.v[i].second == promised(kt, nt, i % nt), "%s: thread %u ran at position %zu of its block", what, a.v[i].second, i % nt);
  if (kb < 3 && kt < 3) CHECK(a.v == a2.v, "%s: fixed kinds changed between two launches", what);
  if (kb == 3 || kt == 3) {
    /* 7 blocks have 42 affine orders, 64 threads 2048: below that two draws may well coincide */
    const bool room = (kb == 3 && nb >= 7) || (kt == 3 && nt >= 64);
    if (room) CHECK(a.v != a2.v, "%s: kind 3 gave the same order for two launches", what);
    emu::set_schedule(kb, kt, 12345); /* the launch counter restarts */
    const Log b = run_log(grid, block), b2 = run_log(grid, block);
    CHECK(a.v == b.v && a2.v == b2.v, "%s: kind 3 is not reproducible from the seed and the launch counter", what);
    emu::set_schedule(kb, kt, 54321);
    const Log c = run_log(grid, block);
    check_complete(c, nb, nt, what);
    if (room) CHECK(a.v != c.v, "%s: kind 3 gave the same order for another seed", what);
  }
  /* barriers + wave and quad exchanges in a loop: terminates (the emulator aborts on a deadlock) and computes the same */
  emu::set_schedule(kb, kt, 777);
  const unsigned iters = 3;
  std::vector<unsigned long long> out((size_t)nb * nt, 0);
  unsigned long long *po = out.data();
  GS_LAUNCH(k_sync_loop, grid, block, 0, nullptr, po, iters);
  const std::vector<unsigned long long> want = sync_loop_expected(nt, iters);
  for (size_t i = 0; i < out.size(); i++) CHECK(out[i] == want[i % nt], "%s: sync loop, block %zu thread %zu", what, i / nt, i % nt);
}

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "env")) { /* what the environment variable alone selects */
    const emu::Schedule s = emu::schedule();
    printf("schedule %d %d %llu\n", s.blocks, s.threads, (unsigned long long)s.seed);
    const Log l = run_log(dim3(5), dim3(3));
    printf("order");
    for (auto &e : l.v) printf(" %u.%u", e.first, e.second);
    printf("\n");
    return 0;
  }
  const dim3 grids[] = {dim3(1), dim3(2), dim3(7), dim3(64, 3, 2)};
  const unsigned blocks[] = {1, 64, 65, 256, 1024};
  for (const dim3 &g : grids)
    for (unsigned nt : blocks)
      for (int kb = 0; kb < 4; kb++)
        for (int kt = 0; kt < 4; kt++) {
          /* the two orders are independent: every pair on the small grids, on the 384-block grid with the large blocks
           * every kind of either order once (the diagonal) */
          if (g.x * g.y * g.z * nt > 30000u && kb != kt) continue;
          check_config(g, nt, kb, kt);
        }
  /* set_schedule(0, 0) is today's order again, and a grid no table could hold still works */
  emu::set_schedule(3, 0, 9);
  {
    const Log l = run_log(dim3(40000, 1, 3), dim3(1));
    const std::vector<unsigned> order = check_complete(l, 120000, 1, "120000 blocks, kind 3");
    unsigned in_place = 0;
    for (unsigned i = 0; i < order.size(); i++) in_place += order[i] == i;
    CHECK(in_place < order.size(), "120000 blocks, kind 3: the ascending order");
  }
  emu::set_schedule(0, 0, 0);
  {
    const Log l = run_log(dim3(3, 2, 2), dim3(2, 3));
    for (size_t i = 0; i < l.v.size(); i++) CHECK(l.v[i].first == i / 6 && l.v[i].second == i % 6, "default order, entry %zu", i);
  }
  if (failures) {
    fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  printf("all passed\n");
  return 0;
}
