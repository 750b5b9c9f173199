// dev_scratch.hpp -- PRIVATE to libfpca.so: owners of what ONE CALL needs on the device and gives back on every way out of it -- device
// memory (DevMem), pinned host memory (PinnedMem), events (DevEvent) -- the one allocation function behind them (dev_alloc) and the one
// sized out-of-memory report (throw_oom).  What lives as long as a context stays with fpca_ctx / ctx_free (ctx.hpp).
//
// Test build only (-DFPCA_TEST_HOOKS): counts of the live objects of the three kinds, and a one-shot countdown that makes the n-th
// acquisition from now (a dev_alloc, a PinnedMem or a DevEvent) throw FPCA_ENOMEM before the runtime is asked for anything
// (fpca_debug_scratch_live / fpca_debug_scratch_fail_at, include/fpca_debug.h).  The product's types carry neither.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <string>
#include <utility>

#include "../../include/fpca.h"
#include "common.hpp"

namespace fpca {

enum { SCRATCH_DEV = 0, SCRATCH_PINNED = 1, SCRATCH_EVENT = 2 };

#ifdef FPCA_TEST_HOOKS
inline std::atomic<uint64_t> g_scratch_live[3];
inline std::atomic<uint64_t> g_scratch_fail_at{0}; // 0: disarmed
inline void scratch_live(int kind, int delta) { g_scratch_live[kind] += (uint64_t)(int64_t)delta; }
// true for exactly one acquisition: the one that takes the countdown from 1 to 0
inline bool scratch_fail_now()
{
   uint64_t n = g_scratch_fail_at.load();
   while (n && !g_scratch_fail_at.compare_exchange_weak(n, n - 1)) {
   }
   return n == 1;
}
#else
inline void scratch_live(int, int) {}
constexpr bool scratch_fail_now() { return false; }
#endif

inline void scratch_check(hipError_t e, const char *what)
{
   if (e != hipSuccess) throw Error(FPCA_EHIP, std::string(what) + " failed: " + hipGetErrorString(e));
}

// FPCA_ENOMEM with the sizes: what the call wanted, in the caller's words, and what the device has left
[[noreturn]] inline void throw_oom(const char *fn, const char *what, size_t need_bytes, const char *detail, int device)
{
   size_t fr = 0, tot = 0;
   (void)hipMemGetInfo(&fr, &tot);
   const double mb = 1.0 / (1024.0 * 1024.0);
   char msg[384];
   std::snprintf(msg, sizeof(msg), "%s: the %s needs %.1f MiB of device memory (%s); %.1f of %.1f MiB are free on device %d", fn, what,
                 (double)need_bytes * mb, detail, (double)fr * mb, (double)tot * mb, device);
   throw Error(FPCA_ENOMEM, msg);
}

// hipMalloc for one call of entry point `fn`: out of memory is FPCA_ENOMEM -- throw_oom's report where the caller gives a `detail`, else
// "<fn>: <what> (<bytes> bytes) does not fit in device memory" -- and anything else FPCA_EHIP
inline void *dev_alloc(size_t bytes, const char *fn, const char *what, const char *detail = nullptr, int device = 0)
{
   void *p = nullptr;
   const hipError_t e = scratch_fail_now() ? hipErrorOutOfMemory : hipMalloc(&p, bytes);
   if (e == hipErrorOutOfMemory) {
      (void)hipGetLastError();
      if (detail) throw_oom(fn, what, bytes, detail, device);
      throw Error(FPCA_ENOMEM, std::string(fn) + ": " + what + " (" + std::to_string(bytes) + " bytes) does not fit in device memory");
   }
   if (e != hipSuccess) throw Error(FPCA_EHIP, std::string(fn) + ": hipMalloc of " + what + " failed: " + hipGetErrorString(e));
   return p;
}

// one device allocation of `count` elements (at least min_bytes; nothing at all for 0 bytes), freed when the owner goes
template <typename T> struct DevMem {
   T *p = nullptr;
   DevMem() = default;
   DevMem(size_t count, const char *fn, const char *what, size_t min_bytes = 0, const char *detail = nullptr, int device = 0)
   {
      const size_t bytes = count * sizeof(T) > min_bytes ? count * sizeof(T) : min_bytes;
      if (!bytes) return;
      p = static_cast<T *>(dev_alloc(bytes, fn, what, detail, device));
      scratch_live(SCRATCH_DEV, 1);
   }
   DevMem(DevMem &&o) noexcept : p(o.p) { o.p = nullptr; }
   DevMem &operator=(DevMem &&o) noexcept
   {
      if (this != &o) {
         reset();
         p = o.p;
         o.p = nullptr;
      }
      return *this;
   }
   DevMem(const DevMem &) = delete;
   DevMem &operator=(const DevMem &) = delete;
   ~DevMem() { reset(); }
   T *release() // the caller (a context) owns the allocation from here on
   {
      if (p) scratch_live(SCRATCH_DEV, -1);
      T *r = p;
      p = nullptr;
      return r;
   }

 private:
   void reset()
   {
      if (!p) return;
      (void)hipFree(p);
      scratch_live(SCRATCH_DEV, -1);
      p = nullptr;
   }
};

// pinned host memory of one call (the bounce buffers of an upload)
struct PinnedMem {
   uint8_t *p = nullptr;
   PinnedMem(size_t bytes, const char *fn, const char *what)
   {
      if (scratch_fail_now()) throw Error(FPCA_ENOMEM, std::string(fn) + ": " + what + " (" + std::to_string(bytes) + " bytes) does not fit in pinned host memory");
      scratch_check(hipHostMalloc(&p, bytes, hipHostMallocDefault), (std::string(fn) + ": hipHostMalloc of " + what).c_str());
      scratch_live(SCRATCH_PINNED, 1);
   }
   PinnedMem(PinnedMem &&o) noexcept : p(o.p) { o.p = nullptr; }
   PinnedMem(const PinnedMem &) = delete;
   PinnedMem &operator=(const PinnedMem &) = delete;
   ~PinnedMem()
   {
      if (!p) return;
      (void)hipHostFree(p);
      scratch_live(SCRATCH_PINNED, -1);
   }
};

// an event of one call of entry point `fn`, created with the owner
struct DevEvent {
   hipEvent_t e = nullptr;
   explicit DevEvent(const char *fn)
   {
      if (scratch_fail_now()) throw Error(FPCA_ENOMEM, std::string(fn) + ": no room for another event");
      scratch_check(hipEventCreate(&e), (std::string(fn) + ": hipEventCreate").c_str());
      scratch_live(SCRATCH_EVENT, 1);
   }
   DevEvent(DevEvent &&o) noexcept : e(o.e) { o.e = nullptr; }
   DevEvent(const DevEvent &) = delete;
   DevEvent &operator=(const DevEvent &) = delete;
   ~DevEvent()
   {
      if (!e) return;
      (void)hipEventDestroy(e);
      scratch_live(SCRATCH_EVENT, -1);
   }
   operator hipEvent_t() const { return e; }
};

inline float elapsed_ms(hipEvent_t e0, hipEvent_t e1)
{
   float ms = 0;
   scratch_check(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime");
   return ms;
}

// mean milliseconds of `reps` calls of launch() on stream s, after `warm` untimed ones; synchronises
template <typename F> float time_launches(hipStream_t s, const char *fn, int warm, int reps, F &&launch)
{
   DevEvent e0(fn), e1(fn);
   for (int i = 0; i < warm; i++) launch();
   scratch_check(hipEventRecord(e0, s), "hipEventRecord");
   for (int i = 0; i < reps; i++) launch();
   scratch_check(hipEventRecord(e1, s), "hipEventRecord");
   scratch_check(hipEventSynchronize(e1), "hipEventSynchronize");
   return elapsed_ms(e0, e1) / reps;
}

} // namespace fpca
