// lmscan.h -- the integer scans of the label-statistics and network-building kernels (lstats.hip, netbuild.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ int lm_wave_incl_scan(int v, int lane)
{
   for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(v, o, 64); if (lane >= o) v += u; }
   return v;
}

// out[i] = in[0] + .. + in[i-1] for i <= n, by ONE workgroup of 1024: the tables here have a vocabulary's length (at most 65 535 rows).
// in == out is allowed.
__global__ __launch_bounds__(1024) void k_lm_scan(const int *in, int *out, int n)
{
   __shared__ int sWave[16];
   __shared__ int sCarry;
   const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
   if (tid == 0) sCarry = 0;
   __syncthreads();
   for (int base = 0; base < n; base += 1024) {
      const int i = base + tid;
      const int v = i < n ? in[i] : 0;
      const int incl = lm_wave_incl_scan(v, lane);
      if (lane == 63) sWave[w] = incl;
      __syncthreads();
      int before = sCarry;
      for (int k = 0; k < w; k++) before += sWave[k];
      if (i < n) out[i] = before + incl - v;
      __syncthreads();
      if (tid == 1023) sCarry = before + incl;
      __syncthreads();
   }
   if (tid == 0) out[n] = sCarry;
}

}
