// The launch profiler's entries: rrin_prof_create / destroy / reset / read / read_spans.  The
// profiler's state (struct rrin_prof) and ProfScope, which brackets each launch of a forward with
// its events, are net_plan.hpp's; nothing here launches a kernel.
#include "net_plan.hpp"

extern "C" int rrin_prof_create(int32_t capacity, rrin_prof** out) {
  if (!out || capacity < 1) return RRIN_E_ARG;
  rrin_prof* p = new rrin_prof();
  p->ev.resize(2 * (size_t)capacity);
  p->start.resize(capacity);
  p->kind.resize(capacity);
  p->flops.resize(capacity);
  // timing-only events: no system-scope fence (a default event record writes
  // back and invalidates the caches, which the next launch then pays for)
  for (auto& e : p->ev) {
    hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
    if (r != hipSuccess) {
      delete p;
      return (int)r;
    }
  }
  *out = p;
  return 0;
}

extern "C" int rrin_prof_destroy(rrin_prof* p) {
  if (!p) return RRIN_E_ARG;
  for (auto& e : p->ev)
    if (e) (void)hipEventDestroy(e);
  delete p;
  return 0;
}

extern "C" int rrin_prof_reset(rrin_prof* p) {
  if (!p) return RRIN_E_ARG;
  p->count = 0;
  p->chain = false;
  return 0;
}

extern "C" int rrin_prof_read(rrin_prof* p, int32_t* kinds, float* ms, double* flops, int32_t cap,
                              int32_t* count) {
  if (!p || !count) return RRIN_E_ARG;
  const int n = p->count < cap ? p->count : cap;
  for (int i = 0; i < n; ++i) {
    if (kinds) kinds[i] = p->kind[i];
    if (flops) flops[i] = p->flops[i];
    if (ms) {
      hipError_t r = hipEventElapsedTime(&ms[i], p->ev[p->start[i]], p->ev[2 * i + 1]);
      if (r != hipSuccess) return (int)r;
    }
  }
  *count = n;
  return 0;
}

extern "C" int rrin_prof_read_spans(rrin_prof* p, float* t0_ms, float* t1_ms, int32_t cap, int32_t* count) {
  if (!p || !count || !t0_ms || !t1_ms) return RRIN_E_ARG;
  const int n = p->count < cap ? p->count : cap;
  for (int i = 0; i < n; ++i) {
    hipError_t r = hipEventElapsedTime(&t0_ms[i], p->ev[0], p->ev[p->start[i]]);
    if (r == hipSuccess) r = hipEventElapsedTime(&t1_ms[i], p->ev[0], p->ev[2 * i + 1]);
    if (r != hipSuccess) return (int)r;
  }
  *count = n;
  return 0;
}
