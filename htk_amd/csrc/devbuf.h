// devbuf.h -- the device plumbing of every host launcher: a buffer that grows on demand and never shrinks (a handle's workspaces), the
// scratch of one call, and the event pair that times a kernel section.
// The empty rule: a typed reserve or upload of zero elements leaves a valid non-null pointer to a minimal allocation and copies nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "internal.h"
#include "hipcheck.h"

// Owner: the name the owner's errors start with ("fb", "viterbi"), an array of static storage; DEVBUF_OWNER("fb") declares it with the
// file's DevBuf and DevScratch.
template <const char *Owner> struct DevBufT {
   void *p = nullptr;
   size_t cap = 0;
   DevBufT() = default; DevBufT(const DevBufT &) = delete; DevBufT &operator=(const DevBufT &) = delete;      // (owns p)
   ~DevBufT() { release(); }
   int reserve(size_t bytes)
   {
      if (bytes <= cap) return HTKAMD_OK;
      if (p) (void)hipFree(p);
      p = nullptr; cap = 0;
      const size_t want = bytes + bytes / 8 + 64;
      hipError_t e = hipMalloc(&p, want);
      if (e != hipSuccess) { p = nullptr; htkamd_set_error("%s: hipMalloc(%zu bytes): %s", Owner, want, hipGetErrorString(e)); return HTKAMD_ENOMEM; }
      cap = want;
      return HTKAMD_OK;
   }
   void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
   // typed: a size is stated once, in elements
   template <typename T> int reserve(size_t n) { return reserve(sizeof(T) * (n ? n : 1)); }
   template <typename T> T *as() const { return (T *)p; }
   template <typename T> int upload(const T *src, size_t n, hipStream_t s)
   {
      int rc = reserve<T>(n);
      if (n) HIPCHECK_RC(rc, Owner, hipMemcpyAsync(p, src, sizeof(T) * n, hipMemcpyHostToDevice, s));
      return rc;
   }
   template <typename T> int upload(const std::vector<T> &v, hipStream_t s) { return upload(v.data(), v.size(), s); }
   template <typename T> int download(T *dst, size_t n, hipStream_t s) const
   {
      int rc = HTKAMD_OK;
      if (n) HIPCHECK_RC(rc, Owner, hipMemcpyAsync(dst, p, sizeof(T) * n, hipMemcpyDeviceToHost, s));
      return rc;
   }
};

// device scratch of one call, released on every way out; the empty rule holds
template <const char *Owner> struct DevScratchT {
   std::vector<void *> all;
   DevScratchT() = default; DevScratchT(const DevScratchT &) = delete; DevScratchT &operator=(const DevScratchT &) = delete;
   ~DevScratchT() { for (void *q : all) (void)hipFree(q); }
   template <typename T> int get(T **out, size_t count)
   {
      const size_t bytes = sizeof(T) * (count ? count : 1);
      void *q = nullptr;
      hipError_t e = hipMalloc(&q, bytes);
      if (e != hipSuccess) { *out = nullptr; htkamd_set_error("%s: hipMalloc(%zu bytes): %s", Owner, bytes, hipGetErrorString(e)); return HTKAMD_ENOMEM; }
      all.push_back(q);
      *out = (T *)q;
      return HTKAMD_OK;
   }
};

#define DEVBUF_OWNER(name)                                                                     \
   namespace {                                                                                 \
   constexpr char devOwner[] = name;                                                           \
   typedef DevBufT<devOwner> DevBuf;                                                           \
   typedef DevScratchT<devOwner> DevScratch;                                                   \
   }

// the time of a kernel section: start and stop in stream order, ms() after the caller's synchronise; the events are made on first use
struct KernelTimer {
   hipEvent_t e0 = nullptr, e1 = nullptr;
   KernelTimer() = default; KernelTimer(const KernelTimer &) = delete; KernelTimer &operator=(const KernelTimer &) = delete;
   ~KernelTimer() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
   hipError_t start(hipStream_t s)
   {
      hipError_t e = e0 ? hipSuccess : hipEventCreate(&e0);
      if (e == hipSuccess && !e1) e = hipEventCreate(&e1);
      return e == hipSuccess ? hipEventRecord(e0, s) : e;
   }
   hipError_t stop(hipStream_t s) { return hipEventRecord(e1, s); }
   hipError_t ms(float *out) const { return hipEventElapsedTime(out, e0, e1); }
};
