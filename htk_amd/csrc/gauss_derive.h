// gauss_derive.h -- the derived tables of one tied state's Gaussians, rebuilt in place by the workgroup that has just written their
// parameters (hinit.hip, hrest.hip): 1/variance (ConvDiagC HUtil.c:413), gConst (FixDiagGConst HModel.c:5641), the exact kernels' rows
// and the log weights (MixLogWeight HModel.c:5288).  A thread per component; call behind a barrier.
#pragma once
#include <hip/hip_runtime.h>
#include "internal.h"

struct GaussTables {
   int D, PS; float logTpiD;                                // logTpiD: D log(2 pi) as the host's libm gives it, rounded to float
   const int *stateCompOff, *compGauss;
   const float *mean, *var, *compWeight;
   float *ivar, *gconst, *gparam, *compLogWt;
};

static __device__ void htkamd_derive_state(const GaussTables &a, int st, int nThreads)
{
   const int D = a.D, c0 = a.stateCompOff[st], M = a.stateCompOff[st + 1] - c0;
   for (int k = threadIdx.x; k < M; k += nThreads) {
      const int g = a.compGauss[c0 + k];
      float *row = a.gparam + (size_t)g * a.PS;
      float sum = a.logTpiD;
      for (int d = 0; d < D; d++) {
         const float v = a.var[(size_t)g * D + d];
         float vc = v;
         if (vc > 1.0E+30f) vc = 1.0E+30f;
         if (vc < 1.0E-30f) vc = 1.0E-30f;
         const float iv = __fdiv_rn(1.0f, vc);
         a.ivar[(size_t)g * D + d] = iv;
         row[2 * d] = a.mean[(size_t)g * D + d]; row[2 * d + 1] = iv;
         const float z = ((double)v <= MINLARG) ? (float)LZERO : (float)log((double)v);
         sum = __fadd_rn(sum, z);
      }
      a.gconst[g] = sum; row[2 * D] = sum;
      const float w = a.compWeight[c0 + k];
      a.compLogWt[c0 + k] = ((double)w < MINMIX) ? (float)LZERO : (float)log((double)w);
   }
}
