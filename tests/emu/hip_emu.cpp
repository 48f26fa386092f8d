/* tests/emu/hip_emu.cpp -- fiber scheduler of the SIMT emulator (TEST TOOL ONLY, see hip_emu.h) */
/* fibers hop between malloc'ed stacks with _setjmp / _longjmp: glibc's fortified longjmp would take that for a
 * corrupted frame */
#undef _FORTIFY_SOURCE
#include "hip_emu.h"
#undef threadIdx
#undef blockIdx
#undef blockDim
#undef gridDim

namespace emu {

State &S() {
  static thread_local State s; /* one emulated device per host thread */
  return s;
}

/* swapcontext saves and restores the signal mask with a system call each way; a kernel test switches fibers
 * millions of times.  So a fiber is ENTERED once through its ucontext and from then on leaves and resumes through
 * _setjmp / _longjmp (registers only). */
/* (Under AddressSanitizer every longjmp makes the runtime re-scan the stack it leaves -- the sanitizer build of
 * tests/test_gsbatch.py went from one minute to twenty-four -- so that build keeps swapcontext.) */
#if defined(__SANITIZE_ADDRESS__)
#define EMU_UCONTEXT_ONLY 1
#else
#define EMU_UCONTEXT_ONLY 0
#endif
static void resume(Fiber &to) { /* never returns */
  if (to.started) _longjmp(to.jb, 1);
  to.started = true;
  setcontext(&to.ctx);
  abort();
}
/* leave the running context `from_*` for fiber `to` (or, to == nullptr, for the scheduler) */
static void hop(ucontext_t *from_ctx, jmp_buf &from_jb, Fiber *to) {
  State &s = S();
#if EMU_UCONTEXT_ONLY
  (void)from_jb;
  swapcontext(from_ctx, to ? &to->ctx : &s.sched);
#else
  (void)from_ctx;
  if (_setjmp(from_jb) == 0) {
    if (to) resume(*to);
    _longjmp(s.sched_jb, 1);
  }
#endif
}

static void fiber_entry() {
  State &s = S();
  (*s.body)();
  Fiber &f = s.fibers[s.cur];
  f.done = true;
  s.alive--;
  s.waves[f.lin / WAVE].alive--;
  hop(&f.ctx, f.jb, nullptr);
}

void yield() {
  State &s = S();
  Fiber &f = s.fibers[s.cur];
  hop(&f.ctx, f.jb, nullptr);
}

/* hardware s_barrier counts only waves that have not exited; same here with threads */
void block_barrier() {
  State &s = S();
  unsigned g = s.bar_gen;
  s.bar_count++;
  while (s.bar_gen == g) {
    if (s.bar_count >= s.alive) {
      s.bar_count = 0;
      s.bar_gen++;
      break;
    }
    yield();
  }
}

static void switch_to(unsigned t);

void wave_rendezvous() {
  State &s = S();
  const unsigned me = s.fibers[s.cur].lin, wv = me / WAVE, l = me % WAVE;
  State::WaveX &w = s.waves[wv];
  unsigned g = w.gen;
  w.count++;
  w.arrived[l] = g + 1;
  while (w.gen == g) {
    if (w.count >= w.alive) {
      w.count = 0;
      w.gen++;
      break;
    }
    /* hand the CPU to a lane of this wave that has not arrived yet (a full round of the block's fibers per wait
     * made wave-level code quadratic); a lane blocked elsewhere gives it back through the scheduler */
    bool handed = false;
    for (unsigned k = 1; k < (unsigned)WAVE && !handed; k++) {
      const unsigned t = wv * WAVE + (l + k) % WAVE;
      if (t < s.nthreads && !s.fibers[t].done && w.arrived[t % WAVE] != g + 1) {
        switch_to(t);
        handed = true;
      }
    }
    if (!handed) yield();
  }
}

/* run fiber t now; the caller stays runnable and is resumed by the scheduler's round-robin (or by a sibling) */
static void switch_to(unsigned t) {
  State &s = S();
  Fiber &me = s.fibers[s.cur], &to = s.fibers[t];
  s.cur = (int)t;
  s.tidx = to.tid;
  hop(&me.ctx, me.jb, &to);
  /* resumed: the scheduler (or a sibling) has set s.cur / s.tidx for us again */
}

uint64_t quad_exchange(uint64_t v, unsigned sel) {
  State &s = S();
  const unsigned me = s.fibers[s.cur].lin, q = me / 4, l = me & 3u;
  State::QuadX &x = s.quads[q];
  const unsigned g = x.gen, buf = g & 1u;
  unsigned live = 0;
  for (unsigned i = 0; i < 4; i++)
    if (q * 4 + i < s.nthreads && !s.fibers[q * 4 + i].done) live++;
  x.slot[buf][l] = v;
  x.count++;
  unsigned next = l;
  while (x.gen == g) {
    if (x.count >= live) {
      x.count = 0;
      x.gen++;
      break;
    }
    /* hand over to the next live sibling; if it is blocked elsewhere it comes straight back via the scheduler */
    bool handed = false;
    for (unsigned k = 1; k <= 3 && !handed; k++) {
      const unsigned t = q * 4 + ((next + k) & 3u);
      if (t < s.nthreads && !s.fibers[t].done && t != me) {
        next = (next + k) & 3u;
        switch_to(t);
        handed = true;
      }
    }
    if (!handed) yield();
  }
  return x.slot[buf][sel & 3u];
}

/* ---- schedules (see hip_emu.h) ---- */
/* process-wide: the host thread pools of the batch entry points launch under it too.  The environment is read once, by
 * whichever thread comes first (a function-local static: initialised under the language's own lock); set_schedule is
 * called between launches, from the thread that drives the test. */
static Schedule schedule_from_env() { /* GS_EMU_SCHEDULE=blocks,threads[,seed] */
  Schedule s;
  const char *e = getenv("GS_EMU_SCHEDULE");
  if (!e || !*e) return s;
  int b = 0, t = 0;
  unsigned long long seed = 0;
  const int n = sscanf(e, "%d,%d,%llu", &b, &t, &seed);
  if (n < 2 || b < 0 || b > 3 || t < 0 || t > 3) {
    fprintf(stderr, "emu: GS_EMU_SCHEDULE=%s is not blocks,threads[,seed] with kinds 0..3\n", e);
    abort();
  }
  s.blocks = b, s.threads = t, s.seed = seed;
  return s;
}
static Schedule &the_schedule() {
  static Schedule s = schedule_from_env();
  return s;
}

Schedule schedule() { return the_schedule(); }

void set_schedule(int blocks, int threads, uint64_t seed) {
  if (blocks < 0 || blocks > 3 || threads < 0 || threads > 3) {
    fprintf(stderr, "emu: schedule kinds are 0..3 (got %d, %d)\n", blocks, threads);
    abort();
  }
  Schedule &s = the_schedule(); /* an explicit call replaces what the environment selected */
  s.blocks = blocks, s.threads = threads, s.seed = seed;
  s.epoch++; /* every host thread restarts its launch counter: kind 3 is reproducible from here on */
}

/* splitmix64 over (seed, launch, block, round) */
static uint64_t mix(uint64_t seed, uint64_t launch, uint64_t block, uint64_t round) {
  uint64_t z = seed;
  const uint64_t in[3] = {launch, block, round};
  for (uint64_t v : in) {
    z += 0x9e3779b97f4a7c15ull + v;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
  }
  return z;
}

static uint64_t gcd64(uint64_t a, uint64_t b) {
  while (b) {
    const uint64_t r = a % b;
    a = b, b = r;
  }
  return a;
}

/* position i of the order -> index in [0, n): no table, whatever the grid's size */
struct Perm {
  int kind;
  uint64_t n, a = 1, b = 0;
  Perm(int kind_, uint64_t n_, uint64_t key) : kind(kind_), n(n_) {
    if (kind == 3 && n > 1) { /* affine map i -> (a i + b) mod n, a coprime to n */
      a = 1 + key % (n - 1);
      while (gcd64(a, n) != 1) a = a + 1 < n ? a + 1 : 1;
      b = (key >> 32 | key << 32) % n;
    }
  }
  uint64_t operator()(uint64_t i) const {
    switch (kind) {
      case 1: return n - 1 - i;
      case 2: return (i & 1u) ? n - 1 - (i >> 1) : (i >> 1);
      case 3: return (uint64_t)(((unsigned __int128)a * i + b) % n);
      default: return i;
    }
  }
};

void launch(dim3 grid, dim3 block, size_t shmem, const std::function<void()> &body) {
  State &s = S();
  unsigned nt = block.x * block.y * block.z;
  if (nt == 0 || nt > 1024) {
    fprintf(stderr, "emu: bad block size %u\n", nt);
    abort();
  }
  if (s.fibers.size() < nt) {
    size_t old = s.fibers.size();
    s.fibers.resize(nt);
    for (size_t i = old; i < nt; i++) s.fibers[i].stack = (char *)malloc(STACK);
  }
  s.bdim = block;
  s.gdim = grid;
  s.body = &body;
  s.nthreads = nt;
  s.waves.assign((nt + WAVE - 1) / WAVE, State::WaveX());
  s.quads.assign((nt + 3) / 4, State::QuadX());
  std::vector<char> lds(shmem + 16);
  s.dyn_lds = lds.data();
  /* the schedule of this launch: read once, so that a launch never changes order half way */
  const Schedule sch = schedule();
  if (s.sched_epoch != sch.epoch) s.sched_epoch = sch.epoch, s.launches = 0;
  const uint64_t launch_no = s.launches++;
  const uint64_t nblocks = (uint64_t)grid.x * grid.y * grid.z;
  const Perm bperm(sch.blocks, nblocks, mix(sch.seed, launch_no, ~0ull, 0));
  for (uint64_t bi = 0; bi < nblocks; bi++) {
    /* kind 0 is the ascending (z, y, x) order of three nested loops */
    const uint64_t b = bperm(bi);
    const unsigned bx = (unsigned)(b % grid.x), by = (unsigned)(b / grid.x % grid.y), bz = (unsigned)(b / ((uint64_t)grid.x * grid.y));
    s.bidx = {bx, by, bz};
    s.bar_count = 0;
    s.alive = nt;
    for (auto &w : s.waves) {
      w.count = 0;
      w.alive = 0;
      memset(w.valid, 0, sizeof w.valid);
      memset(w.arrived, 0, sizeof w.arrived);
      w.gen = 0;
    }
    for (auto &x : s.quads) x.count = 0;
    for (unsigned t = 0; t < nt; t++) {
      Fiber &f = s.fibers[t];
      f.done = false;
      f.started = false;
      f.lin = t;
      f.tid = {t % block.x, (t / block.x) % block.y, t / (block.x * block.y)};
      s.waves[t / WAVE].alive++;
      getcontext(&f.ctx);
      f.ctx.uc_stack.ss_sp = f.stack;
      f.ctx.uc_stack.ss_size = STACK;
      f.ctx.uc_link = nullptr;
      makecontext(&f.ctx, fiber_entry, 0);
    }
    unsigned long spins = 0;
    while (s.alive > 0) {
      /* one scheduling round: every live fiber is resumed once, in the order of the threads kind (kind 3: a new
       * permutation per round, from the seed, the launch, the block and the round) */
      const Perm tperm(sch.threads, nt, sch.threads == 3 ? mix(sch.seed, launch_no, b, spins) : 0);
      for (unsigned k = 0; k < nt; k++) {
        const unsigned t = sch.threads ? (unsigned)tperm(k) : k;
        Fiber &f = s.fibers[t];
        if (f.done) continue;
        s.cur = (int)t;
        s.tidx = f.tid;
        hop(&s.sched, s.sched_jb, &f);
      }
      if (++spins > 50000000ul) {
        fprintf(stderr, "emu: deadlock (divergent barrier / wave op?)\n");
        abort();
      }
    }
  }
  s.cur = -1;
  s.body = nullptr;
}

}  // namespace emu

/* the switch for tests that load the emulator library (ctypes): kinds as in hip_emu.h */
extern "C" void emu_set_schedule(int blocks, int threads, unsigned long long seed) { emu::set_schedule(blocks, threads, seed); }
extern "C" void emu_get_schedule(int *blocks, int *threads, unsigned long long *seed) {
  const emu::Schedule s = emu::schedule();
  *blocks = s.blocks, *threads = s.threads, *seed = s.seed;
}
