/*
 * gs_ctx.cpp -- the per-thread context of libgrayskull_hip.so and the device / stream / memory / tuning entry points of
 * the C ABI (include/grayskull_hip.h).  There is no CPU fallback: without a HIP device every entry point aborts.
 */
#include "gs_internal.h"

namespace gsi {
Ctx &ctx() {
  static thread_local Ctx c;
  return c;
}
TuneTable g_tune;
}  // namespace gsi

extern "C" {

const char *gsh_version(void) {
#ifdef GS_EMU
  return "grayskull_hip 0.1 (kernel-logic emulator build -- test tool, not a product)";
#else
  return "grayskull_hip 0.1 gfx950";
#endif
}
int gsh_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}
void gsh_set_device(int ordinal) {
  Ctx &c = ctx();
  if (c.device_set && c.device != ordinal) c.release();
  c.device = ordinal;
  c.device_set = false;
  c.ensure_device();
}
void gsh_set_stream(void *s) {
  Ctx &c = ctx();
  if (c.own_stream) {
    c.sync();
    (void)hipStreamDestroy(c.stream);
    c.own_stream = false;
  }
#ifndef GS_EMU
  /* Scratch, caches and the side stream belong to the thread, not to the stream: whatever this thread enqueued on the
   * caller's stream it leaves may still read or write them, so the stream it enters waits for that work on the device.
   * (Leaving the library's own stream was a host sync above; a thread that never touched the device has enqueued nothing.) */
  const hipStream_t old = c.stream;
  const bool leaves_user = c.user_stream && c.device_set && old != (hipStream_t)s;
  if (leaves_user) {
    if (!c.ev_switch) GS_HIP(hipEventCreateWithFlags(&c.ev_switch, order_event_flags()));
    GS_HIP(hipEventRecord(c.ev_switch, old));
  }
#endif
  c.stream = (hipStream_t)s;
  c.user_stream = s != nullptr;
#ifndef GS_EMU
  if (leaves_user) GS_HIP(hipStreamWaitEvent(c.s(), c.ev_switch, 0)); /* s == NULL: the own stream is created here */
#endif
}
void *gsh_get_stream(void) { return (void *)ctx().s(); }
void gsh_set_async(int on) { ctx().async = on != 0; }
void gsh_profile(int on) {
#ifndef GS_EMU
  Ctx &c = ctx();
  c.ensure_device();
  c.prof_on = on != 0;
  c.prof_n = 0;
  /* on > 1: create that many event pairs now, so that none is created inside a timed region */
  for (int i = 0; on > 1 && i < 2 * std::min(on, (int)Ctx::kProfPairs); i++)
    if (!c.prof_ev[i]) GS_HIP(hipEventCreateWithFlags(&c.prof_ev[i], sync_event_flags())); /* timing on, no system fence */
#else
  (void)on;
#endif
}
unsigned gsh_profile_read(double *total_ms) {
  unsigned n = 0;
  double sum = 0;
#ifndef GS_EMU
  Ctx &c = ctx();
  c.sync();
  for (unsigned i = 0; i < c.prof_n; i++) {
    float ms = 0;
    GS_HIP(hipEventSynchronize(c.prof_ev[2 * i + 1]));
    GS_HIP(hipEventElapsedTime(&ms, c.prof_ev[2 * i], c.prof_ev[2 * i + 1]));
    sum += ms;
  }
  n = c.prof_n;
  c.prof_n = 0;
#endif
  if (total_ms) *total_ms = sum;
  return n;
}
void gsh_tune(int key, int value) {
  /* retired keys and values forced paths that have been removed (include/grayskull_hip.h); the keys that change results exist in
   * experiment builds only */
  const bool retired = key == 2 || key == 3 || key == 10 || key == 17 || key == 21 || key == 24 ||
                       (key == 6 && (value == 1 || value == 2 || value == 5 || value == 6)) || (key == 13 && value >= 3) ||
                       (key == 14 && (value == -1 || value >= 5));
#ifndef GS_EXPERIMENT
  const bool probe = key == 16 || key == 22 || key == 23;
#else
  const bool probe = false;
#endif
  if ((retired || probe) && value != 0) {
    fprintf(stderr, "grayskull_hip: gsh_tune(%d, %d) ignored: %s\n", key, value,
            retired ? "retired, the path it forced was removed" : "that probe needs a -DGS_EXPERIMENT build (make experiment)");
    return;
  }
  if (key >= 0 && key < 32) g_tune.set(key, value);
}
void gsh_sync(void) { ctx().sync(); }
void gsh_shutdown(void) { ctx().release(); }
void *gsh_malloc(size_t bytes) {
  ctx().ensure_device();
  void *p = nullptr;
  GS_HIP(hipMalloc(&p, bytes ? bytes : 1));
  return p;
}
void gsh_free(void *p) {
  if (p) GS_HIP(hipFree(p));
}
void *gsh_host_alloc(size_t bytes) {
  ctx().ensure_device();
  void *p = nullptr;
  GS_HIP(hipHostMalloc(&p, bytes ? bytes : 1, 0));
  return p;
}
void gsh_host_free(void *p) {
  if (p) GS_HIP(hipHostFree(p));
}
void gsh_memset(void *dev, int byte, size_t bytes) {
  GS_HIP(hipMemsetAsync(dev, byte, bytes, ctx().s()));
}
void gsh_upload(void *dev, const void *host, size_t bytes) {
  GS_HIP(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, ctx().s()));
  ctx().sync();
}
void gsh_download(void *host, const void *dev, size_t bytes) {
  GS_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx().s()));
  ctx().sync();
}
int gsh_is_device_ptr(const void *p) { return is_dev(p) ? 1 : 0; }

#ifdef GS_EMU
static std::atomic<int> g_emu_device_pointers{0};
void emu_device_pointers(int on) { g_emu_device_pointers.store(on != 0); }
int emu_device_pointers_on(void) { return g_emu_device_pointers.load(); }
#endif

}  /* extern "C" */
