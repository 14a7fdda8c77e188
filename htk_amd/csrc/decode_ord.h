// decode_ord.h -- HRec's instance list on the device: what the exact-order kernels (decode_ord.hip: k_decode_ord, 1-best; decode_n.hip:
// k_decode_ord_n, token sets) share -- the list, its upkeep and its walk.  See decode_ord.hip for the design.
//
// The walk is the kernels' whole frame loop (ord_frames): maximum-model pruning, compaction, pass 1 over the list, the beam thresholds,
// and pass 2 -- one wavefront stepping the list while it grows under it.  It is written ONCE, as a template over a TOKEN FORM, the struct
// through which a kernel says what a state holds (a Tok; a TSet).  A form F has, all inlined (no form crosses a call that stays a call):
//    typename F::Exit                     what StepInst2 hands to the links: Tok / TSet
//    null_exit(n), null_state(i)          ex[n] / the state token(s) at index i become null (pruning: one thread; DetachInst: lane 0 / lane i)
//    thresholds(thr)                      where a pass reads gT / wT: what else the form wants from LDS (N-best: nT)
//    step1(n, ni, t, gT, myGen, myWord)   StepInst1 on one list entry (StepHMM1 / StepWord1): its tokens, ex[n], imax[n]; raises the two tops
//    extra_threshold(thr, genMax)         by thread 0 next to dec_beam_thresholds (N-best: thr[2])
//    end_pass1()                          by every thread behind pass 1's barrier (N-best: the columns change places)
//    step2(n, ni, t, lane, vs)            StepInst2 on one node by the walking wavefront: ex[n] stored; false: vs->status is set, the walk ends
//    exit_of(n)                           ... and the exit token / set in every lane, read only behind that test (1-best: from the lanes'
//                                         registers; N-best: ex[n], which lane 0 made -- a load in front of the test costs the kernel scratch)
//    set_entry(e, d, lm, xl)              SetEntryState over one link (to node d, LM log probability lm, token likelihood xl), by the lane
//                                         that owns the link; returns the entry's likelihood afterwards
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

// The LDS of a list kernel beside OrdShared (the kernel declares it: its sizes are the kernel's)
struct OrdLds {
   double *red, *red2;            // ORD_THREADS / 64 each (dec_block_max)
   float *thr;                    // [0] gT, [1] wT, what the form keeps behind them
   unsigned int *usel; int *uhist;      // dec_prune_threshold
   int *scan;                     // ord_compact
};
// ... and the run's constants the walk itself reads
struct OrdBeams { int maxActive; float genBeam, wordBeam, lmScale; };

// Pass 2 of frame t (HRec.c:2011-2021; at t = 0 StartRecognition's): ONE wavefront walks the list while it changes.
template <class F>
__device__ __forceinline__ void ord_walk(const OrdCtx &c, F &f, const float *thr, const float lmScale, const int t)
{
   const DecNet &N = *c.N;
   const int lane = threadIdx.x & 63;
   const float gT = thr[0], wT = thr[1];
   f.thresholds(thr);
   volatile OrdShared *vs = c.sh;
   volatile double *imax = c.imax; volatile int *pos = c.pos;
   int idx = 0;
   while (idx < vs->tail && vs->status == 0) {
      const int tl = vs->tail;
      const int cn = (tl - idx < 64) ? tl - idx : 64;
      {
         const int n = (lane < cn) ? c.seq[idx + lane] : -1;
         vs->chunkNode[lane] = n;
         vs->chunkMax[lane] = (n >= 0) ? (float)imax[n] : 0.0f;
         if (lane == 0) { vs->base = idx; vs->cn = cn; }
      }
      __builtin_amdgcn_wave_barrier();
      for (int i = 0; i < cn && vs->status == 0; i++) {
         const int n = vs->chunkNode[i];
         if (n < 0) continue;                           // moved or detached since the chunk was fetched
         const float nmax = vs->chunkMax[i];
         const int4 ni = N.nodeInfo[n];
         const int kind = ni.x & 15, NS = (ni.x >> 4) & 255, t0 = ni.y;
         if (nmax < gT) {                               // DetachInst (HRec.c:1270): every token of the instance goes
            if (lane == 0) { o_blank(c, n); pos[n] = -1; imax[n] = LZERO; f.null_exit(n); }
            const int nt = (kind == HTKAMD_NODE_HMM) ? NS - 1 : 1;
            if (lane < nt) f.null_state(t0 + lane);
            __threadfence_block();
            continue;
         }
         // StepInst2 (HRec.c:1360)
         if (!f.step2(n, ni, t, lane, vs)) break;
         const typename F::Exit e = f.exit_of(n);
         double tkLike = e.like;                        // what travels along the links (with e.lm: set_entry)
         if (kind != HTKAMD_NODE_HMM && tkLike < wT) tkLike = LZERO;
         if (tkLike > gT) {
            const int k0 = N.linkOff[n], k1 = N.linkOff[n + 1];
            const bool dup = N.dupDest[n] != 0;
            for (int kb = k0; kb < k1; kb += 64) {
               const int k = kb + lane;
               const bool act = k < k1;
               const int d = act ? N.linkDest[k] : 0;
               const float lm = act ? N.linkLike[k] : 0.0f;
               const double xl = tkLike + lm * lmScale;
               const bool pass = act && xl > gT;
               // AttachInst for the destinations without an instance, link by link (appending is what orders the list)
               unsigned long long need = __ballot(pass && pos[d] < 0);
               while (need) {
                  const int j = __ffsll((long long)need) - 1;
                  need &= need - 1;
                  const int dj = __shfl(d, j);
                  if (lane == 0 && pos[dj] < 0) o_attach(c, dj);       // (a destination met twice among the links is attached once)
                  __threadfence_block();
               }
               if (vs->status != 0) break;
               // SetEntryState (HRec.c:1303): the first of equal tokens stays (the order of the merges is the result); the instance's max follows
               unsigned long long todo = __ballot(pass);
               if (!dup) todo = pass ? (1ull << lane) : 0ull;          // distinct destinations: every lane its own, at once
               while (todo) {
                  const int j = dup ? __ffsll((long long)todo) - 1 : lane;
                  todo = dup ? (todo & (todo - 1)) : 0ull;
                  if (lane == j) {
                     const double el = f.set_entry(e, d, lm, xl);
                     const double m0 = imax[d];
                     if (el > m0) {
                        const float nm = (float)el;
                        imax[d] = (double)nm;
                        const int pd = pos[d];
                        if (pd >= vs->base && pd < vs->base + vs->cn) vs->chunkMax[pd - vs->base] = nm;
                     }
                  }
                  if (dup) __threadfence_block();
               }
               __threadfence_block();
            }
         }
      }
      idx += cn;
   }
}

// The frame loop of a list kernel, by the whole workgroup of ORD_THREADS threads: frames 0 .. T, or up to the frame in which the walk ran
// out of a capacity (sh.status, which the kernel's ending reads).  seqA / seqB: the utterance's two list buffers.
template <class F>
__device__ __forceinline__ void ord_frames(OrdCtx &c, F &f, const OrdLds &l, int *seqA, int *seqB, const int T, const OrdBeams b)
{
   const DecNet &N = *c.N;
   OrdShared &sh = *c.sh;
   volatile double *imax = c.imax; volatile int *pos = c.pos;
   const int tid = threadIdx.x, wv = tid >> 6;
   for (int t = 0; t <= T; t++) {
      if (t >= 1) {
         // ---- maximum-model pruning (ProcessObservation HRec.c:1966-1985): more than maxActive instances on the list -> those whose max
         // lies below the (maxActive + 1)-th largest (as floats) are detached (the threshold: dec_prune_threshold, decode_dev.h)
         if (b.maxActive > 0 && sh.tail > b.maxActive) {
            const float uth = dec_prune_threshold<ORD_THREADS>(sh.tail, b.maxActive, l.usel, l.uhist, [&](const int i, float &key) {
               const int n = c.seq[i];
               if (n < 0) return false;
               key = (float)imax[n];
               return true;
            });
            if (uth > (float)LSMALL)
               for (int i = tid; i < sh.tail; i += ORD_THREADS) {
                  const int n = c.seq[i];
                  if (n < 0 || !((float)imax[n] < uth)) continue;
                  c.seq[i] = -1; pos[n] = -1; imax[n] = LZERO; f.null_exit(n);
                  const int4 ni = N.nodeInfo[n];
                  const int nt = ((ni.x & 15) == HTKAMD_NODE_HMM) ? ((ni.x >> 4) & 255) - 1 : 1;
                  for (int q = 0; q < nt; q++) f.null_state(ni.y + q);
               }
            __syncthreads();
         }
         ord_compact(c, seqA, seqB, l.scan);
         // ---- pass 1: StepInst1 on every instance (no order in it: the beams' tops are maxima)
         const float gT = l.thr[0];                         // threshold of the previous frame
         f.thresholds(l.thr);
         double myGen = LZERO, myWord = LZERO;
         const int nLive = sh.tail;
         for (int i = tid; i < nLive; i += ORD_THREADS) {
            const int n = c.seq[i];
            f.step1(n, N.nodeInfo[n], t, gT, myGen, myWord);
         }
         const double genMax = dec_block_max<ORD_THREADS>(myGen, l.red);
         const double wordMax = dec_block_max<ORD_THREADS>(myWord, l.red2);
         if (tid == 0) { dec_beam_thresholds(l.thr, genMax, wordMax, b.genBeam, b.wordBeam); f.extra_threshold(l.thr, genMax); }
         __threadfence_block();
         __syncthreads();
         f.end_pass1();
      }
      if (wv == 0) ord_walk(c, f, l.thr, b.lmScale, t);
      __threadfence_block();
      __syncthreads();
      if (sh.status != 0) break;
   }
}
