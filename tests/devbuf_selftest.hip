// devbuf_selftest.hip -- csrc/devbuf.h and csrc/hipcheck.h on their own: the typed buffer, the scratch list and the kernel timer, with a
// device and without one (tests/test_devbuf.py runs it; built by htk_amd/build.py).  Prints one line and returns 0, or says what failed.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "devbuf.h"
#include "htk_amd.h"

DEVBUF_OWNER("selftest")

static int g_failed = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, htkamd_last_error()); g_failed++; } } while (0)

template <typename T> static void round_trip(size_t n, hipStream_t s)
{
   std::vector<T> in(n), out(n);
   for (size_t i = 0; i < n; i++) in[i] = (T)(i * 2654435761u % 1000003u) / (T)7;
   DevBuf b;
   EXPECT(b.upload(in, s) == HTKAMD_OK);
   EXPECT(b.p != nullptr && b.cap >= sizeof(T) * n);
   EXPECT(b.download(out.data(), n, s) == HTKAMD_OK);
   EXPECT(hipStreamSynchronize(s) == hipSuccess);
   EXPECT(memcmp(in.data(), out.data(), sizeof(T) * n) == 0);
}

static void with_device(void)
{
   hipStream_t s = nullptr;
   for (size_t n : {1, 63, 64, 65}) round_trip<int>(n, s);
   for (size_t n : {1, 1000}) round_trip<double>(n, s);
   {                                                     // the empty rule
      DevBuf b;
      EXPECT(b.upload((const int *)nullptr, 0, s) == HTKAMD_OK && b.p != nullptr);
      DevBuf c;
      EXPECT(c.reserve<double>(0) == HTKAMD_OK && c.p != nullptr);
      EXPECT(c.upload(std::vector<float>(), s) == HTKAMD_OK && c.p != nullptr);
      int sink = 7;
      EXPECT(c.download(&sink, 0, s) == HTKAMD_OK && sink == 7);
   }
   {                                                     // grow-only
      DevBuf b;
      EXPECT(b.reserve<int>(1000) == HTKAMD_OK);
      void *p = b.p; const size_t cap = b.cap;
      EXPECT(cap >= 4000);
      EXPECT(b.reserve<int>(10) == HTKAMD_OK && b.p == p && b.cap == cap);
      EXPECT(b.reserve(cap) == HTKAMD_OK && b.p == p && b.cap == cap);
      // growing replaces the allocation: the old one is freed first, so the allocator may hand its address out again, and what shows
      // the new one is its capacity and that all of it takes a copy
      EXPECT(b.reserve(cap + 1) == HTKAMD_OK && b.p != nullptr && b.cap > cap);
      EXPECT(b.as<int>() == (int *)b.p);
      std::vector<char> in(b.cap, 'x'), out(b.cap, 0);
      const size_t grown = b.cap;
      EXPECT(b.upload(in, s) == HTKAMD_OK && b.cap == grown);
      EXPECT(b.download(out.data(), grown, s) == HTKAMD_OK && hipStreamSynchronize(s) == hipSuccess && in == out);
   }
   {                                                     // the timer: an empty section, twice
      KernelTimer t;
      for (int k = 0; k < 2; k++) {
         float ms = -1.0f;
         EXPECT(t.start(s) == hipSuccess && t.stop(s) == hipSuccess);
         EXPECT(hipStreamSynchronize(s) == hipSuccess);
         EXPECT(t.ms(&ms) == hipSuccess && isfinite(ms) && ms >= 0.0f);
      }
   }
   {                                                     // the scratch list
      DevScratch b;
      int *a = nullptr, *e = nullptr; double *d = nullptr;
      EXPECT(b.get(&a, 100) == HTKAMD_OK && b.get(&d, 100) == HTKAMD_OK && b.get(&e, 0) == HTKAMD_OK);
      EXPECT(a && d && e && (void *)a != (void *)d && (void *)a != (void *)e && (void *)d != (void *)e);
      EXPECT(b.all.size() == 3);
   }
   int rc = HTKAMD_OK;                                   // the check leaves rc alone on success and skips the call once rc is set
   HIPCHECK_RC(rc, devOwner, hipStreamSynchronize(s));
   EXPECT(rc == HTKAMD_OK);
   rc = HTKAMD_EINVAL;
   int calls = 0;
   HIPCHECK_RC(rc, devOwner, (calls++, hipSuccess));
   EXPECT(rc == HTKAMD_EINVAL && calls == 0);
}

static void without_device(void)
{
   const int data[4] = {1, 2, 3, 4};
   int back[4] = {0, 0, 0, 0};
   {
      DevBuf b;
      EXPECT(b.reserve<int>(4) != HTKAMD_OK && b.p == nullptr && b.cap == 0);
      EXPECT(strstr(htkamd_last_error(), "selftest") != nullptr);
      EXPECT(b.upload(data, 4, nullptr) != HTKAMD_OK && b.p == nullptr && b.cap == 0);
      EXPECT(b.upload((const int *)nullptr, 0, nullptr) != HTKAMD_OK && b.p == nullptr && b.cap == 0);
      EXPECT(strstr(htkamd_last_error(), "selftest") != nullptr);
      b.release();
      EXPECT(b.p == nullptr && b.cap == 0);
   }
   {
      DevScratch b;
      int *a = (int *)back;
      EXPECT(b.get(&a, 4) != HTKAMD_OK && a == nullptr && b.all.empty());
      EXPECT(strstr(htkamd_last_error(), "selftest") != nullptr);
   }
   {
      KernelTimer t;
      EXPECT(t.start(nullptr) != hipSuccess);
   }
   int rc = HTKAMD_OK;                                   // a missing device is HTKAMD_ENODEV, and the message names the owner
   HIPCHECK_RC(rc, devOwner, hipErrorNoDevice);
   EXPECT(rc == HTKAMD_ENODEV && strstr(htkamd_last_error(), "selftest: hipErrorNoDevice") != nullptr);
}

int main(void)
{
   int nd = 0;
   const bool dev = hipGetDeviceCount(&nd) == hipSuccess && nd > 0;
   if (dev) with_device(); else without_device();
   if (g_failed) return 1;
   printf("devbuf selftest ok (%s)\n", dev ? "device" : "no device");
   return 0;
}
