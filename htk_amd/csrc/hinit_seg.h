/* hinit_seg.h -- UCollectData's rule (HInit.c:515-520), one copy for the kernels (csrc/hinit.hip) and the host twin (host/hinit.c). */
#ifndef HTKAMD_HINIT_SEG_H
#define HTKAMD_HINIT_SEG_H

#ifdef __HIPCC__
#define HINIT_FN static __host__ __device__ inline
#else
#define HINIT_FN static inline
#endif

/* 0-based emitting state of frame j0 (0-based) of a token of L >= nEmit frames: n = (int)(((float)(j-1) / obsPerState) + 2), the
   quotient and the sum in float (the sum can round up where the quotient alone would not).  The reference writes past its table when
   that reaches the exit state; here the last emitting state takes the frame. */
HINIT_FN int htkamd_hinit_state_of(int j0, int L, int nEmit)
{
#ifdef __HIP_DEVICE_COMPILE__
   const float per = __fdiv_rn((float)L, (float)nEmit);
   const float n = __fadd_rn(__fdiv_rn((float)j0, per), 2.0f);
#else
   const float per = (float)L / (float)nEmit;           /* (built without contraction; x86-64 float arithmetic is single precision) */
   const float q = (float)j0 / per;
   const float n = q + 2.0f;
#endif
   int s = (int)n - 2;
   if (s > nEmit - 1) s = nEmit - 1;
   return s;
}

#endif
