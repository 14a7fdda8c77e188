// devbuf.h -- a device buffer that grows on demand and never shrinks (forward-backward's and the aligner's workspaces).
#pragma once
#include <hip/hip_runtime.h>
#include "internal.h"

// Owner: the name the owner's errors start with ("fb", "viterbi"), an array of static storage:
//    static constexpr char owner[] = "fb";  typedef DevBufT<owner> DevBuf;
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
      if (e != hipSuccess) { htkamd_set_error("%s: hipMalloc(%zu bytes): %s", Owner, want, hipGetErrorString(e)); return HTKAMD_ENOMEM; }
      cap = want;
      return HTKAMD_OK;
   }
   void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};
