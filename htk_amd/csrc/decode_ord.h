// decode_ord.h -- HRec's instance list on the device: what the exact-order kernels (decode_ord.hip: 1-best; decode_n.hip: k_decode_ord_n,
// token sets) share -- the list and its upkeep.  See decode_ord.hip for the design.
#pragma once
#include <hip/hip_runtime.h>
#include "decode.h"
#include "decode_dev.h"

#define ORD_THREADS 256
#define ORD_STACK 64               /* depth of ReOrderList's recursion (a chain of zero-time nodes) */

// what the walking wavefront shares: LDS, written by lane 0 or by all lanes with the same value
struct OrdShared {
   int tail;                      // entries of seq in use
   int nPath;                     // Path records allocated
   int status;                    // 0, or the error the utterance ends with
   int base, cn;                  // the chunk of seq the walk holds: [base, base + cn)
   int chunkNode[64];
   float chunkMax[64];
   int stkNode[ORD_STACK], stkCur[ORD_STACK];
};

struct OrdCtx {
   const DecNet *N;
   volatile int *seq; volatile int *pos; volatile unsigned char *ooo;
   volatile double *imax;
   int seqCap;
   OrdShared *sh;
};

// MoveToRecent (HRec.c:1123) / the list part of DetachInst: by ONE lane
__device__ __forceinline__ void o_blank(const OrdCtx &c, int n)
{
   const int p = c.pos[n];
   c.seq[p] = -1;
   if (p >= c.sh->base && p < c.sh->base + c.sh->cn) ((volatile int *)c.sh->chunkNode)[p - c.sh->base] = -1;
}
__device__ __forceinline__ bool o_append(const OrdCtx &c, int n)
{
   const int tl = ((volatile OrdShared *)c.sh)->tail;
   if (tl >= c.seqCap) { c.sh->status = -5; return false; }
   c.seq[tl] = n; c.pos[n] = tl; ((volatile OrdShared *)c.sh)->tail = tl + 1;
   c.ooo[n] = 1;
   return true;
}

// ReOrderList (HRec.c:1152) on node n0, whose instance has just been appended: by ONE lane, the recursion on an explicit stack
__device__ void o_reorder(const OrdCtx &c, int n0)
{
   const DecNet &N = *c.N;
   OrdShared *sh = c.sh;
   int sp = 0;
   sh->stkNode[0] = n0; sh->stkCur[0] = -1; sp = 1;
   while (sp > 0) {
      const int n = sh->stkNode[sp - 1];
      const int cur = sh->stkCur[sp - 1];
      const int k0 = N.linkOff[n], nt = N.nTr0[n];
      if (cur < 0) {
         if (c.pos[n] < 0 || !c.ooo[n]) { sp--; continue; }
         c.ooo[n] = 0;
         for (int k = 0; k < nt; k++) {
            const int d = N.linkDest[k0 + k];
            if (c.pos[d] >= 0) { o_blank(c, d); if (!o_append(c, d)) return; }
         }
         sh->stkCur[sp - 1] = 0;
      } else if (cur >= nt) sp--;
      else {
         sh->stkCur[sp - 1] = cur + 1;
         const int d = N.linkDest[k0 + cur];
         if (c.pos[d] >= 0) {
            if (sp >= ORD_STACK) { sh->status = -6; return; }
            sh->stkNode[sp] = d; sh->stkCur[sp] = -1; sp++;
         }
      }
   }
}

// AttachInst (HRec.c:1200): by ONE lane.  The node's tokens are null already (DetachInst and the start leave them so).
__device__ __forceinline__ void o_attach(const OrdCtx &c, int n)
{
   if (!o_append(c, n)) return;
   if (c.N->nTr0[n] > 0) o_reorder(c, n);
   else c.ooo[n] = 0;
}

// The blanks out of the list (its order stays): seq -> the other of the utterance's two buffers.  By the whole workgroup; scan:
// ORD_THREADS / 64 ints of LDS.
__device__ __forceinline__ void ord_compact(OrdCtx &c, int *seqA, int *seqB, int *scan)
{
   const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
   int *src = (int *)c.seq, *dst = (src == seqA) ? seqB : seqA;
   const int tl = c.sh->tail;
   int outBase = 0;
   for (int b0 = 0; b0 < tl; b0 += ORD_THREADS) {
      const int i = b0 + tid;
      const int n = (i < tl) ? src[i] : -1;
      const unsigned long long m = __ballot(n >= 0);
      if (lane == 0) scan[wv] = __popcll(m);
      __syncthreads();
      int off = outBase;
      for (int w = 0; w < wv; w++) off += scan[w];
      int tot = 0;
      for (int w = 0; w < ORD_THREADS / 64; w++) tot += scan[w];
      if (n >= 0) { const int o = off + __popcll(m & ((1ull << lane) - 1ull)); dst[o] = n; c.pos[n] = o; }
      outBase += tot;
      __syncthreads();
   }
   c.seq = dst;
   if (tid == 0) c.sh->tail = outBase;
   __syncthreads();
}
