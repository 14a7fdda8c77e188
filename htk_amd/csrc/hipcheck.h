// hipcheck.h -- turn a failing HIP runtime call into an HTKAMD_EHIP return with a message (HTKAMD_ENODEV where there is no device).
#ifndef HTKAMD_HIPCHECK_H
#define HTKAMD_HIPCHECK_H
#include <hip/hip_runtime.h>
#include "internal.h"

#define HIPCHECK(call)                                                                         \
   do {                                                                                        \
      hipError_t e_ = (call);                                                                  \
      if (e_ != hipSuccess) {                                                                  \
         htkamd_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
         return (e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice) ? HTKAMD_ENODEV : HTKAMD_EHIP; \
      }                                                                                        \
   } while (0)

// the same into rc, for a function that has to clean up before it returns: the call is skipped once rc is set, so a chain of these
// stops at the first failure of any kind.  owner: the name the message starts with.
#define HIPCHECK_RC(rc, owner, call)                                                           \
   do {                                                                                        \
      if (!(rc)) {                                                                             \
         hipError_t e_ = (call);                                                               \
         if (e_ != hipSuccess) {                                                               \
            htkamd_set_error("%s: %s -> %s", owner, #call, hipGetErrorString(e_));             \
            (rc) = (e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice) ? HTKAMD_ENODEV : HTKAMD_EHIP; \
         }                                                                                     \
      }                                                                                        \
   } while (0)

#endif
