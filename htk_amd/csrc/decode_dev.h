// decode_dev.h -- device code the four token-passing kernels share (k_decode: decode.hip; k_decode_ord: decode_ord.hip; k_decode_n and
// k_decode_ord_n: decode_n.hip): the null token, the workgroup maximum, the CreateSEIndex range, the beam thresholds, the threshold of
// HVite -u's maximum-model pruning and the 1-best traceback.  Each is HRec.c's semantics stated ONCE; decode_ord.h adds the instance list
// and its walk: the frame loop of the two list kernels, a template over their token form.
// Everything here is inlined into its caller: k_decode<NPT > 0> keeps its tokens in registers and spills when pushed.
#pragma once
#include <hip/hip_runtime.h>
#include "decode.h"

__device__ __forceinline__ Tok dec_null() { Tok t; t.like = LZERO; t.lm = 0.0f; t.path = -1; return t; }

// maximum of v over the workgroup of NTHR threads; red: NTHR / 64 doubles of LDS
template <int NTHR>
__device__ __forceinline__ double dec_block_max(double v, double *red)
{
#pragma unroll
   for (int o = 32; o > 0; o >>= 1) { const double w = __shfl_xor(v, o); v = (w > v) ? w : v; }
   const int wv = threadIdx.x >> 6;
   __syncthreads();
   if ((threadIdx.x & 63) == 0) red[wv] = v;
   __syncthreads();
   double r = red[0];
   for (int i = 1; i < NTHR / 64; i++) r = (red[i] > r) ? red[i] : r;
   return r;
}

// CreateSEIndex (HRec.c:1403): the range (lo, hi) of states with a transition into state j (1-based) of the NS x NS log transition matrix
// tp -- what StepHMM1 takes its maximum over.  lo0: where the range may start, 1 for an emitting state, 2 for the exit state (j = NS), which
// does not take from the entry state.  A column without a transition gets the whole range (lo0, NS - 1).  (Also the host's: the ranges
// packed into the register-resident models' records, decode.hip.)
__host__ __device__ __forceinline__ void dec_se_range(const float *tp, const int NS, const int j, const int lo0, int &lo, int &hi)
{
   lo = lo0; hi = NS - 1;
   while (lo < NS && !(tp[(lo - 1) * NS + (j - 1)] > LSMALL)) lo++;
   while (hi > 1 && !(tp[(hi - 1) * NS + (j - 1)] > LSMALL)) hi--;
   if (lo > hi) { lo = lo0; hi = NS - 1; }
}

// The beam thresholds of the next pass from this frame's tops (ProcessObservation HRec.c:1996-2005), floats floored at LSMALL:
// thr[0] = genMax - genBeam, thr[1] = wordMax - wordBeam.  By ONE thread.
__device__ __forceinline__ void dec_beam_thresholds(float *thr, const double genMax, const double wordMax, const float genBeam, const float wordBeam)
{
   float w = (float)(wordMax - wordBeam); if (w < (float)LSMALL) w = (float)LSMALL;
   float g = (float)(genMax - genBeam); if (g < (float)LSMALL) g = (float)LSMALL;
   thr[0] = g; thr[1] = w;
}

// ... and the third of the N-best kernels: TokSetMerge's cut nThresh = genMax - nBeam (HRec.c:2002), floored at LSMALL / 2, not LSMALL
__device__ __forceinline__ float dec_nbest_threshold(const double genMax, const float nBeam)
{
   const float nn = (float)(genMax - nBeam);
   return (nn < (float)(LSMALL / 2)) ? (float)(LSMALL / 2) : nn;
}

// Maximum-model pruning (HVite -u; ProcessObservation HRec.c:1966-1985): when more than maxActive instances are attached, those whose
// max (a float, NetInst.max) lies below the (maxActive + 1)-th largest are detached before pass 1.  live(i, key), i in [0, n): entry i is
// an attached instance, key = its max as a float.  Returns that (maxActive + 1)-th largest max -- the caller detaches the live entries
// below it where it exceeds (float)LSMALL -- or -infinity when no more than maxActive are attached.  By the whole workgroup of NTHR
// threads (barriers inside); usel: [0] attached instances, [1] key prefix, [2] rank still to skip; uhist: 256 counters.
// Selection: radix select on the float keys, a byte per pass.
template <int NTHR, class Live>
__device__ __forceinline__ float dec_prune_threshold(const int n, const int maxActive, unsigned int *usel, int *uhist, Live live)
{
   const int tid = threadIdx.x;
   if (tid == 0) usel[0] = 0;
   __syncthreads();
   int cnt = 0;
   for (int i = tid; i < n; i += NTHR) { float key; if (live(i, key)) cnt++; }
   if (cnt) atomicAdd(&usel[0], (unsigned)cnt);
   __syncthreads();
   if ((int)usel[0] <= maxActive) return -INFINITY;
   if (tid == 0) { usel[1] = 0; usel[2] = (unsigned)maxActive; }
   unsigned int mask = 0;
   for (int pass = 0; pass < 4; pass++) {
      const int shift = 24 - 8 * pass;
      for (int i = tid; i < 256; i += NTHR) uhist[i] = 0;
      __syncthreads();
      const unsigned int prefix = usel[1];
      for (int i = tid; i < n; i += NTHR) {
         float key;
         if (!live(i, key)) continue;
         unsigned int k = __float_as_uint(key);
         k ^= (k >> 31) ? 0xFFFFFFFFu : 0x80000000u;          // ascending order of the floats
         if ((k & mask) == prefix) atomicAdd(&uhist[(k >> shift) & 255], 1);
      }
      __syncthreads();
      if (tid == 0) {
         unsigned int skip = usel[2], cum = 0; int b = 255;
         for (; b > 0; b--) { if (cum + (unsigned)uhist[b] > skip) break; cum += (unsigned)uhist[b]; }
         usel[1] = prefix | ((unsigned)b << shift); usel[2] = skip - cum;
      }
      mask |= 255u << shift;
      __syncthreads();
   }
   unsigned int kk = usel[1];
   kk ^= (kk >> 31) ? 0x80000000u : 0xFFFFFFFFu;
   return __uint_as_float(kk);
}

// Where a Path record lies: the dense [frame][word node] table of the batch kernels (pathFrame = pathNode = NULL: record p is column
// p % nW of frame p / nW), or records allocated one by one with their frame and node beside them (the list kernels)
struct PathView {
   const int *pathFrame, *pathNode; int nW; const int *wordNode;
   __device__ __forceinline__ int frame(int p) const { return pathFrame ? pathFrame[p] : p / nW; }
   __device__ __forceinline__ int node(int p) const { return pathNode ? pathNode[p] : wordNode[p % nW]; }
};

// CompleteRecognition (HRec.c:2054) + LatFromPaths (:1512) + TranscriptionFromLattice (:2176) for the 1-best chain that ends in the
// final token `fin`: the utterance's total, its words with their boundaries and LArcTotLike scores (the float / double mix of aclike and
// sc is HVite's, operand for operand).  By ONE thread.
__device__ __forceinline__ void dec_traceback(const DecArgs &a, const DecUtt &ud, const int u, const Tok fin, const PathView view)
{
   const DecNet &N = a.net;
   const int *pathPrev = a.pathPrev + ud.path0; const double *pathLike = a.pathLike + ud.path0; const float *pathLm = a.pathLm + ud.path0;
   const int fp = fin.path;
   int nW = 0;
   a.total[u] = LZERO; a.finalLm[u] = 0.0f;
   if (fp >= 0) {
      a.total[u] = fin.like; a.finalLm[u] = fin.lm;
      for (int p = fp; p >= 0; p = pathPrev[p]) nW++;
      if (nW > a.maxWords) nW = -3;
      else {
         int w = nW;
         for (int p = fp; p >= 0;) {
            const int prev = pathPrev[p];
            const double prlk = (prev >= 0) ? pathLike[prev] : 0.0;
            const double wp = a.wordPen;
            const float plm = pathLm[p];
            float aclike = (float)(pathLike[p] - prlk - plm * a.lmScale - wp);
            const int node = view.node(p);
            const float pr = N.pronProb[node];
            aclike -= pr * a.prScale;
            const float sc = (float)((double)((aclike * 1.0f + plm * a.lmScale) + pr * a.prScale) + (double)a.wordPen);
            w--;
            a.wordPron[ud.out0 + w] = N.model[node];
            a.wordEnd[ud.out0 + w] = view.frame(p);
            a.wordStart[ud.out0 + w] = (prev >= 0) ? view.frame(prev) : 0;
            a.wordScore[ud.out0 + w] = sc;
            a.wordLm[ud.out0 + w] = plm;
            a.wordAc[ud.out0 + w] = aclike;
            a.wordLike[ud.out0 + w] = pathLike[p];
            p = prev;
         }
      }
   } else nW = -1;
   a.nWords[u] = nW;
}
