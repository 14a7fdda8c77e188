// decode_ord.hip -- K7o: network decoding in HRec's own instance order (the exact-tie path of HVite -w).
//
// Why it exists.  HRec keeps one NetInst per active network node on a list that CHANGES while pass 2 walks it: AttachInst appends
// (HRec.c:1200-1268), ReOrderList / MoveToRecent (:1123-1170) re-append every live successor over zero-time links behind a new
// instance, DetachInst (:1270-1301) unlinks.  SetEntryState (:1303) keeps the FIRST of two tokens of exactly equal likelihood, so which
// of two equally likely histories survives at a node is a function of that list's order -- of the whole activation history of the
// utterance.  k_decode (decode.hip) pulls in a static order that coincides with the list's in all but manufactured cases; it now FLAGS
// an utterance in which two tokens of equal likelihood and different histories met at a node, and such utterances are decoded again
// here, where the list itself is kept on the device and walked as the reference walks it.  (Without a tie every order gives the same
// tokens: the fast kernel's result stands.)
//
// The list as an array.  A node has at most one instance, so an instance is its node; the list is `seq[]` (node numbers in list order,
// -1 where an instance was taken out) with `pos[node]` = the node's place.  AttachInst = append at `tail`; MoveToRecent = blank the
// old place, append; DetachInst = blank.  Pass 2 is one walk over seq[0 .. tail) while tail grows -- what a step attaches or moves
// lies behind the cursor and is reached in the same walk, exactly as `next = pri->nxtInst->link` does (a node moved while it is being
// stepped leaves a blank at the cursor: the walk goes on with what followed it).  Blanks are squeezed out once per frame.
//
// Mapping.  One workgroup of 256 threads per utterance.  Pass 1 (StepHMM1 / StepWord1, beam tops) has no order: all threads, an
// instance each.  Pass 2 is sequential by nature: wavefront 0 walks, 64 list entries fetched at a time; the links of the node being
// stepped are the lanes (the tokens a node sends go to different nodes; attaching, which appends, is taken link by link).  Tokens,
// exit tokens and instance maxima are the arrays k_decode uses; Path records are allocated one by one (StepWord2 may run twice on a node
// in one frame -- "may be repeated", HRec.c:1046 -- and both records can stay referenced).
//
// Where the code is.  The list, its compaction and the frame loop with the walk are decode_ord.h's, shared with k_decode_ord_n
// (decode_n.hip); the pruning threshold, the beam thresholds and the traceback are decode_dev.h's.  This file has what is 1-best about
// it: the token form OrdTok (a Tok per state, strict > where two tokens meet), the kernel's prologue and its ending.  Output
// probabilities come from the same score block (K1, exact mode).  Tested against HVite on the tie files and sweeps
// (tests/test_gpu_decode.py, tests/fuzz_parity.py) and against oracle/orc_decode.c, which walks the same list (oracle/orc_ilist.h).
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include "internal.h"
#include "hipcheck.h"
#include "kernels.h"
#include "decode.h"

#include "decode_ord.h"

// The 1-best token form of the walk (decode_ord.h says what a form is)
struct OrdTok {
   typedef Tok Exit;
   const DecArgs &a; const DecUtt &ud; const DecNet &N;
   Tok *tok, *ex; volatile double *imax;
   const float *tpBase;
   size_t pathCap;
   int *pathPrev, *pathNode, *pathFrame; double *pathLike; float *pathLm;
   Tok e;                       // the exit token step2 has just computed, in every lane (exit_of)

   __device__ __forceinline__ void null_exit(const int n) const { ex[n] = dec_null(); }
   __device__ __forceinline__ void null_state(const int i) const { tok[i] = dec_null(); }
   __device__ __forceinline__ void thresholds(const float *) const {}
   __device__ __forceinline__ void extra_threshold(float *, double) const {}
   __device__ __forceinline__ void end_pass1() const {}

   // StepHMM1 (HRec.c:642) with the model's tokens in registers; StepWord1 (:1038) for the rest
   __device__ __forceinline__ void step1(const int n, const int4 ni, const int t, const float gT, double &myGen, double &myWord) const
   {
      if ((ni.x & 15) != HTKAMD_NODE_HMM) { tok[ni.y] = dec_null(); ex[n] = dec_null(); imax[n] = LZERO; return; }
      const int NS = (ni.x >> 4) & 255, t0 = ni.y;
      const float *tp = tpBase + ni.z;
      Tok s[DEC_MAXN];
      bool live = false;
#pragma unroll
      for (int q = 1; q < DEC_MAXN; q++) { s[q] = dec_null(); if (q < NS) s[q] = tok[t0 + q - 1]; }
#pragma unroll
      for (int q = 1; q < DEC_MAXN; q++) if (q < NS && s[q].like > LSMALL) live = true;
      Tok exT = dec_null();
      double mx = LZERO;
      if (live) {
         Tok nw[DEC_MAXN];
#pragma unroll
         for (int j = 2; j < DEC_MAXN; j++) {
            nw[j] = dec_null();
            if (j < NS) {
               int lo, hi;
               dec_se_range(tp, NS, j, 1, lo, hi);
               Tok best = s[1]; double bl = LZERO;
#pragma unroll
               for (int q = 1; q < DEC_MAXN; q++)
                  if (q >= lo && q <= hi) {
                     const double cc = s[q].like + tp[(q - 1) * NS + (j - 1)];
                     if (q == lo || cc > bl) { best = s[q]; bl = cc; }
                  }
               best.like = bl;
               if (best.like > gT) {
                  const int st = N.hmmState[ni.w + (j - 2)];
                  best.like += a.score[ud.score0 + (size_t)(t - 1) * a.ns + N.stateSlot[st]];
                  nw[j] = best;
                  if (best.like > mx) mx = best.like;
               }
            }
         }
         {
            int lo, hi;
            dec_se_range(tp, NS, NS, 2, lo, hi);
            Tok best = nw[2]; double bl = LZERO;
#pragma unroll
            for (int q = 2; q < DEC_MAXN; q++)
               if (q >= lo && q <= hi) {
                  const double cc = nw[q].like + tp[(q - 1) * NS + (NS - 1)];
                  if (q == lo || cc > bl) { best = nw[q]; bl = cc; }
               }
            best.like = bl;
            if (best.like > LSMALL) {
               exT = best;
               const double w = best.like + N.wdlk[n];
               if (w > myWord) myWord = w;
            }
         }
         tok[t0] = dec_null();                            // entry consumed
#pragma unroll
         for (int j = 2; j < DEC_MAXN; j++) if (j < NS) tok[t0 + j - 1] = nw[j];
         if (mx > myGen) myGen = mx;
      }
      ex[n] = exT; imax[n] = (double)(float)mx;         // inst->max is a LogFloat (HRec.c:138)
   }

   // StepInst2 (HRec.c:1360): every lane computes the exit token, lane 0 stores it
   __device__ __forceinline__ bool step2(const int n, const int4 ni, const int t, const int lane, volatile OrdShared *vs)
   {
      const int kind = ni.x & 15, NS = (ni.x >> 4) & 255, t0 = ni.y;
      if (kind == HTKAMD_NODE_WORD) {               // StepWord2 (HRec.c:1046): a Path record per call
         const Tok st = tok[t0];
         e = st;
         e.like += a.wordPen;
         e.like += N.pronProb[n] * a.prScale;
         const int pid = vs->nPath;
         if ((size_t)pid >= pathCap) { if (lane == 0) vs->status = -4; return false; }
         if (lane == 0) {
            pathPrev[pid] = st.path; pathLike[pid] = e.like; pathLm[pid] = e.lm; pathNode[pid] = n; pathFrame[pid] = t;
            vs->nPath = pid + 1;
         }
         e.path = pid; e.lm = 0.0f;
         if (lane == 0) ex[n] = e;
      } else if (kind == HTKAMD_NODE_NULL) {
         e = tok[t0];
         if (lane == 0) ex[n] = e;
      } else {
         e = ex[n];
         if ((ni.x >> 12) & 1) {                    // tee model: StepHMM2 (HRec.c:790)
            const Tok st = tok[t0];
            const double cc = st.like + tpBase[ni.z + (NS - 1)];
            if (cc > e.like) { e = st; e.like = cc; if (lane == 0) ex[n] = e; }
         }
      }
      return true;
   }
   __device__ __forceinline__ Tok exit_of(int) const { return e; }

   // SetEntryState (HRec.c:1303): strict >, the first of equal tokens stays
   __device__ __forceinline__ double set_entry(const Tok &e, const int d, const float lm, const double xl) const
   {
      const int td = N.nodeInfo[d].y;
      Tok x = e;
      x.like = xl; x.lm = e.lm + lm;
      Tok cur = tok[td];
      if (x.like > cur.like) { tok[td] = x; cur = x; }
      return cur.like;
   }
};

__global__ __launch_bounds__(ORD_THREADS) void k_decode_ord(OrdArgs oa)
{
   const DecArgs &a = oa.d;
   __shared__ double red[ORD_THREADS / 64];
   __shared__ double red2[ORD_THREADS / 64];
   __shared__ float thr[2];
   __shared__ float ltp[2048];
   __shared__ int uhist[256];
   __shared__ unsigned int usel[4];
   __shared__ int scan[ORD_THREADS / 64 + 1];
   __shared__ OrdShared sh;
   const int sel = blockIdx.x, tid = threadIdx.x;
   if (sel >= a.nUtt) return;
   const DecUtt ud = a.utt[sel];
   const DecNet &N = a.net;
   const int T = ud.T, u = ud.idx;
   Tok *tok = a.tok + ud.tok0, *ex = a.ex + ud.node0;
   volatile double *imax = a.imax + ud.node0;
   volatile int *pos = oa.list.pos + ud.node0;
   volatile unsigned char *ooo = oa.list.ooo + ud.node0;
   int *seqA = oa.list.seq + (size_t)sel * 2 * oa.list.seqCap, *seqB = seqA + oa.list.seqCap;
   const size_t pathCap = 3 * ((size_t)(T + 1) * N.nWordNodes) + (size_t)oa.list.pathExtra;      // as the host laid the records out (decode.hip)
   int *pathNode = oa.list.pathNode + ud.path0, *pathFrame = oa.list.pathFrame + ud.path0;
   // (this form only: the transition matrices in LDS where they fit -- pass 1 reads them per state pair, the N-best form through set_step1's sets)
   const bool tpInLds = N.nTpFloats <= 2048;
   if (tpInLds) for (int i = tid; i < N.nTpFloats; i += ORD_THREADS) ltp[i] = N.transP[i];

   for (int i = tid; i < N.nTok; i += ORD_THREADS) tok[i] = dec_null();
   for (int i = tid; i < N.nNodes; i += ORD_THREADS) { ex[i] = dec_null(); imax[i] = LZERO; pos[i] = -1; ooo[i] = 0; }
   if (tid == 0) { thr[0] = (float)LSMALL; thr[1] = (float)LSMALL; sh.tail = 0; sh.nPath = 0; sh.status = 0; sh.base = 0; sh.cn = 0; }
   __syncthreads();
   OrdCtx c;
   c.N = &N; c.seq = seqA; c.pos = pos; c.ooo = ooo; c.imax = imax; c.seqCap = oa.list.seqCap; c.sh = &sh;
   if (tid == 0) {                                          // StartRecognition (HRec.c:1884): the initial node's instance, a token of likelihood 0
      o_attach(c, N.initial);
      Tok z; z.like = 0.0; z.lm = 0.0f; z.path = -1;
      tok[N.nodeInfo[N.initial].y] = z; imax[N.initial] = 0.0;
   }
   __syncthreads();

   OrdTok f{a, ud, N, tok, ex, imax, tpInLds ? ltp : N.transP, pathCap, a.pathPrev + ud.path0, pathNode, pathFrame, a.pathLike + ud.path0, a.pathLm + ud.path0, dec_null()};
   ord_frames(c, f, OrdLds{red, red2, thr, usel, uhist, scan}, seqA, seqB, T, OrdBeams{a.maxActive, a.genBeam, a.wordBeam, a.lmScale});

   // ---- CompleteRecognition: the 1-best chain (dec_traceback, decode_dev.h)
   if (tid == 0) {
      // (this form only: a capacity of the LIST walk is no reason to lose an answer the batch kernel has already given -- a tie-free order
      // is one valid order of HRec's; the status codes -4 / -5 / -6 then never reach the caller in the default mode)
      if (sh.status != 0 && oa.keepFast && a.nWords[u] >= 0) return;
      if (sh.status != 0) { a.total[u] = LZERO; a.finalLm[u] = 0.0f; a.nWords[u] = sh.status; }
      else dec_traceback(a, ud, u, (pos[N.final] >= 0) ? ex[N.final] : dec_null(), PathView{pathFrame, pathNode, N.nWordNodes, N.wordNode});
   }
}

int htkamd_launch_decode_ord(const OrdArgs &a, int nSel, hipStream_t s)
{
   if (nSel <= 0) return HTKAMD_OK;
   hipLaunchKernelGGL(k_decode_ord, dim3(nSel), dim3(ORD_THREADS), 0, s, a);
   hipError_t e = hipGetLastError();
   if (e != hipSuccess) { htkamd_set_error("decode_ord: launch: %s", hipGetErrorString(e)); return HTKAMD_EHIP; }
   return HTKAMD_OK;
}
