// decode_n.hip -- K7n: N-best token passing and lattice generation over a recognition network (HVite -n N [-z ext]).
//
// Reference semantics (HRec.c with nToks > 1; oracle/orc_decode_n.c is the restatement this kernel is tested against):
//   TokenSet :100 = the state's best token + up to N-1 RelTokens (float likelihood relative to it, lm, path), sorted, distinct in the
//   word-end node their path ends in; TokSetMerge :279 wherever the 1-best code takes a maximum (StepHMM1 :642, StepHMM2 :790,
//   SetEntryState :1303) with the cut nThresh = genMax - nBeam (:2002); StepWord2 :1046 opens a Path record for the best token and a
//   NxtPath per alternative; CompleteRecognition :2054 -> CreateLattice :1679: MarkPaths numbers the reachable Path records depth
//   first, LatFromPaths :1512 makes every Path / NxtPath an arc (aclike, lmlike, prlike).
//
// Mapping: decode.hip's (one 1024-thread workgroup per utterance, every node PULLS from its predecessors in the order the reference's
// senders are stepped, emitting models in registers, zero-time nodes level by level), with token SETS where it has tokens:
//   * a set is a 128-byte record in global memory (L2-resident per utterance); a thread merges into a register-resident copy with the
//     reference's algorithm operand for operand -- the relative likelihoods are floats re-based at every merge, so the order of the
//     merges is the reference's order and the arcs come out with the reference's values;
//   * the state sets of the emitting models are double-buffered per frame (state j of the new column reads several states of the old);
//   * nodes with a large fan-in (loop / back-off null nodes): every thread merges a CONTIGUOUS run of predecessors in order into a
//     partial set in LDS, thread 0 merges the non-empty partial sets in run order -- the sets are the reference's, the re-basing of
//     the relative likelihoods is associated differently (last-bit differences of alternatives' scores are possible there);
//   * Path records: the dense [frame][word node] table of decode.hip plus N-1 alternative slots per entry;
//   * the lattice is built on the device by one thread (depth-first over the table with an explicit stack) and only its nodes and
//     arcs go back to the host.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>
#include "internal.h"
#include "hipcheck.h"
#include "kernels.h"
#include "decode.h"
#include "decode_ord.h"

#define NT DEC_MAX_TOKS             /* capacity of a token set (HVite -n up to 8) */

struct __attribute__((aligned(16))) TSet {
   double like; float lm; int path;    // the best token
   int n, align;                       // align: Token.align (an index into the utterance's Align records, -1 = NULL; k_decode_ord_n with -m / -f)
   float rl[NT], rlm[NT]; int rp[NT];  // relative tokens; [0] mirrors the best (like 0)
   int ra[NT];                         // RelToken.align (-DPHNALG)
};
// a wide node's partial set in LDS (k_decode_n): a token set without the alignment fields, which that kernel never makes -- 1024 whole
// TSets are all 160 KB of a workgroup's LDS and leave none for the kernel's other arrays: the launch was refused
struct __attribute__((aligned(8))) PSet { double like; float lm; int path; int n; float rl[NT], rlm[NT]; int rp[NT]; };
struct __attribute__((aligned(8))) AlignRec { int node, state, frame, prev; double like; };      // Align (HRec.c:150-164)

struct NArgs {
   DecNet net;
   const DecUtt *utt; int nUtt;
   const float *score; int ns;         // frame-major: score[score0 + (t-1)*ns + slot]
   TSet *tokA, *tokB;                  // [sum nTok] state sets, double-buffered
   TSet *ex; double *imax;             // [sum nNodes]
   int *pathPrev; double *pathLike; float *pathLm;             // [sum (T+1)*nWordNodes]
   int *altN, *altPrev; double *altLike; float *altLm;         // alternatives: altN[path], others [path*(NT-1) + k]
   int *mark;                                                  // [paths] MarkPaths' usage numbers
   int *stack;                                                 // [nUtt * 2*maxLatNodes] depth-first stack
   int *nodePath;                                              // [nUtt * maxLatNodes] the Path record of a lattice node
   OrdList list;                                               // k_decode_ord_n: the instance list and Path records allocated one by one
   // ... and alignment records (HVite -n with -m: alignMode & 1 = pri->models, -f: & 2 = pri->states)
   int alignMode; AlignRec *al; int alCap; int *alCount;          // [nUtt * alCap] records, [nUtt] records made
   int *pathAlign, *altAlign;                                     // Path.align [paths], NxtPath.align [paths * (NT-1)]
   int maxAlign; int *arcAlignOff, *alState, *alNode, *alDur; float *alLike;      // lAlign of the arcs: [nUtt * (maxLatArcs + 1)], [nUtt * maxAlign]
   float genBeam, wordBeam, nBeam, lmScale, wordPen, prScale;
   int nToks, maxActive;
   int maxLatNodes, maxLatArcs;
   int *latN;                          // [nUtt*2] nodes, arcs (or -1 / -3)
   int *nodeFrame, *nodeNet;           // [nUtt*maxLatNodes]
   double *nodeLike;
   int *arcStart, *arcEnd; float *arcAc, *arcLm, *arcPr; double *arcScore;     // [nUtt*maxLatArcs]
   double *total;
   const DecNet *nets;                 // k_decode_n / k_decode_ord_n<SET>: a network per utterance, nets[DecUtt::net], and DecUtt::ns rows (net and ns above are then not read)
};

// (StepWord1 / a token under the beam: the best token goes, the relative tokens stay as they are)
__device__ __forceinline__ void ts_null_head(TSet &s) { s.like = LZERO; s.lm = 0.0f; s.path = -1; s.align = -1; s.n = 1; }
__device__ __forceinline__ void ts_null(TSet &s) { s.like = LZERO; s.lm = 0.0f; s.path = -1; s.n = 1; s.align = -1; s.rl[0] = 0.0f; s.rlm[0] = 0.0f; s.rp[0] = -1; s.ra[0] = -1; }
// the word-end node a path ends in (TokSetMerge compares path->node): the dense table's column, or -- Path records allocated one by one
// (k_decode_ord_n) -- the record's node
struct KeyOf {
   const int *pathNode; int nW;
   __device__ __forceinline__ int operator()(int path) const { return path < 0 ? -1 : (pathNode ? pathNode[path] : path % nW); }
};

// TokSetMerge (HRec.c:279): token (cLike, cLm, cPath) with the relative tokens of `src` merged into `res`
__device__ void ts_merge(TSet &res, double cLike, float cLm, int cPath, const TSet &src, float nThresh, int nToks, const KeyOf key_of, const int cAlign = -1)
{
   float tl[NT], tlm[NT]; int tp[NT], ta[NT]; int tn; double tLike;
   if (cLike >= res.like) {
      if (!(cLike > nThresh)) return;
      if (res.like > nThresh) {                            // exchange
         tLike = res.like; tn = res.n;
         for (int k = 0; k < res.n; k++) { tl[k] = res.rl[k]; tlm[k] = res.rlm[k]; tp[k] = res.rp[k]; ta[k] = res.ra[k]; }
         res.like = cLike; res.lm = cLm; res.path = cPath; res.align = cAlign; res.n = src.n;
         for (int k = 0; k < src.n; k++) { res.rl[k] = src.rl[k]; res.rlm[k] = src.rlm[k]; res.rp[k] = src.rp[k]; res.ra[k] = src.ra[k]; }
      } else {
         res.like = cLike; res.lm = cLm; res.path = cPath; res.align = cAlign; res.n = src.n;
         for (int k = 0; k < src.n; k++) { res.rl[k] = src.rl[k]; res.rlm[k] = src.rlm[k]; res.rp[k] = src.rp[k]; res.ra[k] = src.ra[k]; }
         return;
      }
   } else {
      if (!(cLike > nThresh)) return;
      tLike = cLike; tn = src.n;
      for (int k = 0; k < src.n; k++) { tl[k] = src.rl[k]; tlm[k] = src.rlm[k]; tp[k] = src.rp[k]; ta[k] = src.ra[k]; }
   }
   const float diff = (float)(res.like - tLike);
   const float limit = (float)((double)nThresh - tLike);
   for (int i = 0; i < tn; i++) {
      if (tl[i] < limit) break;
      const int key = key_of(tp[i]);
      const float like = tl[i] - diff;
      int mch = -1;
      for (int k = 0; k < res.n; k++) if (key_of(res.rp[k]) == key) { mch = k; break; }
      if (mch < 0) {
         if (res.n < nToks) { mch = res.n++; res.rl[mch] = (float)LZERO; res.rlm[mch] = 0.0f; res.rp[mch] = -1; res.ra[mch] = -1; }
         else mch = res.n - 1;
      }
      if (like > res.rl[mch]) {
         for (mch--; mch >= 0 && like > res.rl[mch]; mch--) { res.rl[mch + 1] = res.rl[mch]; res.rlm[mch + 1] = res.rlm[mch]; res.rp[mch + 1] = res.rp[mch]; res.ra[mch + 1] = res.ra[mch]; }
         mch++;
         res.rp[mch] = tp[i]; res.rlm[mch] = tlm[i]; res.ra[mch] = ta[i]; res.rl[mch] = like;
      }
   }
}

// predecessors k0..k1 (step 1) of a node merged in order into `res` (SetEntryState over StepInst2's sends)
__device__ void pull_sets(const NArgs &a, const TSet *ex, int k0, int k1, float gT, float wT, float nT, TSet &res)
{
   for (int k = k0; k < k1; k++) {
      const int ps = a.net.predSrc[k];
      const float lm = a.net.predLike[k];
      const TSet &e = ex[ps & 0x7fffffff];
      if (!(e.like > gT)) continue;
      if (ps < 0 && e.like < wT) continue;
      const double c = e.like + lm * a.lmScale;
      if (!(c > gT)) continue;
      TSet x = e;
      for (int q = 0; q < x.n; q++) x.rlm[q] = e.rlm[q] + lm;
      ts_merge(res, c, e.lm + lm, e.path, x, nT, a.nToks, KeyOf{nullptr, a.net.nWordNodes});
   }
}

// StepWord2 for the token set `st` that entered word node n at frame t: the Path record and the exit set
__device__ void word_exit(const NArgs &a, const DecUtt &ud, int n, int t, const TSet &st, TSet &e)
{
   const DecNet &N = a.net;
   e = st;
   e.like += a.wordPen;
   e.like += N.pronProb[n] * a.prScale;
   const size_t pid = (size_t)t * N.nWordNodes + N.wordIdx[n];
   a.pathPrev[ud.path0 + pid] = st.path; a.pathLike[ud.path0 + pid] = e.like; a.pathLm[ud.path0 + pid] = e.lm;
   a.altN[ud.path0 + pid] = st.n - 1;
   for (int k = 1; k < st.n; k++) {
      const size_t z = (ud.path0 + pid) * (NT - 1) + (k - 1);
      a.altLike[z] = e.like + st.rl[k]; a.altLm[z] = st.rlm[k]; a.altPrev[z] = st.rp[k];
   }
   e.path = (int)pid; e.lm = 0.0f;
   e.n = 1; e.rl[0] = 0.0f; e.rlm[0] = 0.0f; e.rp[0] = e.path;
}

// lAlign of one arc (LatFromPaths HRec.c:1582-1656 with -DPHNALG): the arc's chain of records, latest first; a state record's likelihood
// is the running difference, a model record closes the model met before it.  Returns the number of records, -1 if they do not fit.
__device__ int emit_lalign(const NArgs &a, int sel, size_t outBase, int at, int a0, int pathFrame, double plike, float plm, double wp, int prevFrame, double prevLike, bool hasPrev)
{
   const AlignRec *AL = a.al + (size_t)sel * a.alCap;
   int cnt = 0;
   for (int al = a0; al >= 0; al = AL[al].prev) cnt++;
   if (cnt == 0) return 0;
   if (at + cnt > a.maxAlign) return -1;
   int i = cnt, frame = pathFrame, prr = -1, labpr = -1;
   double like = plike - plm * a.lmScale - wp;
   for (int al = a0; al >= 0; al = AL[al].prev) {
      const AlignRec A = AL[al];
      int durF, labNode;
      if (A.state < 0) {
         if (prr < 0) { prr = al; labpr = A.node; continue; }
         durF = AL[prr].frame - A.frame;
         like = AL[prr].like - A.like;
         prr = al;
         labNode = labpr; labpr = A.node;
      } else {
         labNode = A.node;
         durF = frame - A.frame;
         like = like - A.like;
         frame = A.frame;
      }
      i--;
      a.alState[outBase + at + i] = A.state; a.alNode[outBase + at + i] = labNode; a.alDur[outBase + at + i] = durF; a.alLike[outBase + at + i] = (float)like;
      like = A.like;
   }
   if (prr >= 0) {
      int durF;
      if (hasPrev) { durF = AL[prr].frame - prevFrame; like = AL[prr].like - prevLike; }
      else { durF = AL[prr].frame; like = AL[prr].like; }
      i--;
      a.alState[outBase + at + i] = -1; a.alNode[outBase + at + i] = labpr; a.alDur[outBase + at + i] = durF; a.alLike[outBase + at + i] = (float)like;
   }
   return cnt;
}

// CompleteRecognition (HRec.c:2054) -> CreateLattice (:1679): MarkPaths (:1664) numbers the Path records reachable from the final token
// set depth first, LatFromPaths (:1512) makes every Path / NxtPath an arc.  By ONE thread.  Where a Path record lies: PathView (decode_dev.h).

__device__ void build_lattice(const NArgs &a, const DecUtt &ud, int u, const TSet &fin, const PathView pv, const int sel = 0)
{
   const DecNet &N = a.net;
   const int T = ud.T;
   a.total[u] = LZERO;
   int *latN = a.latN + 2 * u;
   latN[0] = -1; latN[1] = 0;
   if (fin.path < 0) return;
   a.total[u] = fin.like;
   const size_t nb = (size_t)u * a.maxLatNodes, ab = (size_t)u * a.maxLatArcs;
   int *stk = a.stack + (size_t)u * 2 * a.maxLatNodes;
   int *nodePath = a.nodePath + nb;
   int nn = 1, nl = 0, sp = 0;
   bool overflow = false;
   // the root (a Path that is not in the table): node 1; children = fin.path, then fin.rp[1..]
   nn = 2; nl = 1;
   a.nodeFrame[nb + 0] = 0; a.nodeNet[nb + 0] = -1; a.nodeLike[nb + 0] = 0.0;
   a.nodeFrame[nb + 1] = T; a.nodeNet[nb + 1] = -2; a.nodeLike[nb + 1] = fin.like;
   // visit(p): number it, push it; children are looked at in order prev, alt 0, alt 1, ...
#define VISIT(p_) do { const int pp_ = (p_); if (pp_ >= 0 && a.mark[ud.path0 + pp_] == 0) { \
      if (nn >= a.maxLatNodes) overflow = true; else { a.mark[ud.path0 + pp_] = nn; nodePath[nn] = pp_; \
         a.nodeFrame[nb + nn] = pv.frame(pp_); a.nodeNet[nb + nn] = pv.node(pp_); a.nodeLike[nb + nn] = a.pathLike[ud.path0 + pp_]; nn++; nl++; \
         stk[2 * sp] = pp_; stk[2 * sp + 1] = 0; sp++; } } } while (0)
   for (int c = 0; c < fin.n && !overflow; c++) {
      if (c > 0) nl++;
      VISIT(c == 0 ? fin.path : fin.rp[c]);
      while (sp > 0 && !overflow) {
         const int p = stk[2 * (sp - 1)];
         const int ch = stk[2 * (sp - 1) + 1]++;
         const int nAlt = a.altN[ud.path0 + p];
         if (ch == 0) VISIT(a.pathPrev[ud.path0 + p]);
         else if (ch - 1 < nAlt) { nl++; VISIT(a.altPrev[(ud.path0 + p) * (NT - 1) + (ch - 1)]); }
         else sp--;
      }
   }
#undef VISIT
   if (overflow || nl > a.maxLatArcs) { latN[0] = -3; return; }
   int ln = 0, nAl = 0;
   const size_t aob = (size_t)u * (a.maxLatArcs + 1), alb = (size_t)u * a.maxAlign;
   // arcs of the root
   for (int c = 0; c < fin.n; c++) {
      const int prev = (c == 0) ? fin.path : fin.rp[c];
      const double plike = (c == 0) ? fin.like : fin.like + fin.rl[c];
      const float plm = (c == 0) ? fin.lm : fin.rlm[c];
      const double prlk = (prev >= 0) ? a.pathLike[ud.path0 + prev] : 0.0;
      a.arcStart[ab + ln] = (prev >= 0) ? a.mark[ud.path0 + prev] : 0; a.arcEnd[ab + ln] = 1;
      a.arcAc[ab + ln] = (float)(plike - prlk - plm * a.lmScale - 0.0); a.arcLm[ab + ln] = plm; a.arcPr[ab + ln] = 0.0f; a.arcScore[ab + ln] = plike;
      if (a.alignMode) {
         a.arcAlignOff[aob + ln] = nAl;
         const int r = emit_lalign(a, sel, alb, nAl, (c == 0) ? fin.align : fin.ra[c], T, plike, plm, 0.0, (prev >= 0) ? pv.frame(prev) : 0, prlk, prev >= 0);
         if (r < 0) { latN[0] = -3; return; }
         nAl += r;
      }
      ln++;
   }
   for (int i = 2; i < nn; i++) {
      const int p = nodePath[i];
      const int node = a.nodeNet[nb + i];
      const int nAlt = a.altN[ud.path0 + p];
      for (int c = 0; c <= nAlt; c++) {
         const size_t z = (ud.path0 + p) * (NT - 1) + (c - 1);
         const int prev = (c == 0) ? a.pathPrev[ud.path0 + p] : a.altPrev[z];
         const double plike = (c == 0) ? a.pathLike[ud.path0 + p] : a.altLike[z];
         const float plm = (c == 0) ? a.pathLm[ud.path0 + p] : a.altLm[z];
         const double prlk = (prev >= 0) ? a.pathLike[ud.path0 + prev] : 0.0;
         const double wp = a.wordPen;
         float ac = (float)(plike - prlk - plm * a.lmScale - wp);
         const float pr = N.pronProb[node];
         ac -= pr * a.prScale;
         a.arcStart[ab + ln] = (prev >= 0) ? a.mark[ud.path0 + prev] : 0; a.arcEnd[ab + ln] = i;
         a.arcAc[ab + ln] = ac; a.arcLm[ab + ln] = plm; a.arcPr[ab + ln] = pr; a.arcScore[ab + ln] = plike;
         if (a.alignMode) {
            a.arcAlignOff[aob + ln] = nAl;
            const int r = emit_lalign(a, sel, alb, nAl, (c == 0) ? a.pathAlign[ud.path0 + p] : a.altAlign[z], pv.frame(p), plike, plm, wp, (prev >= 0) ? pv.frame(prev) : 0, prlk, prev >= 0);
            if (r < 0) { latN[0] = -3; return; }
            nAl += r;
         }
         ln++;
      }
   }
   if (a.alignMode) a.arcAlignOff[aob + ln] = nAl;
   latN[0] = nn; latN[1] = ln;
}

// NewNRefAlign (HRec.c:598-622): records are allocated one by one per utterance (any thread; their numbers are not part of any result)
__device__ __forceinline__ int new_align(const NArgs &a, int sel, int node, int state, double like, int frame, int prev)
{
   const int i = atomicAdd(&a.alCount[sel], 1);
   if (i >= a.alCap) return -1;                          // (counted: the utterance ends as "did not fit")
   AlignRec r; r.node = node; r.state = state; r.frame = frame; r.prev = prev; r.like = like;
   a.al[(size_t)sel * a.alCap + i] = r;
   return i;
}

// StepHMM1 (HRec.c:642) on the token sets of model instance n, from the CreateSEIndex ranges to the exit set: cur = the sets on entry,
// nxt = the new column (the entry set consumed); exS = the exit set, mx = the instance's maximum, wordTop raised by exit + LikeToWord.
// A set under the beam loses its best token only (HRec sets tok.like: the relative tokens stay as they are; nothing reads them).
// ALIGN (k_decode_ord_n): the alignment records of HVite -m / -f, as a.alignMode asks for them.
template <bool ALIGN>
__device__ __forceinline__ void set_step1(const NArgs &a, const DecUtt &ud, const int sel, const int n, const int4 ni, const float *tp, const TSet *cur, TSet *nxt,
                                          const float gT, const float nT, const int t, const KeyOf ko, TSet &exS, double &mx, double &wordTop)
{
   const DecNet &N = a.net;
   const int NS = (ni.x >> 4) & 255, t0 = ni.y;
   for (int j = 2; j < NS; j++) {
      // CreateSEIndex (HRec.c:1403): dec_se_range (decode_dev.h).  The copy stays here and below: with the helper k_decode_n<256, true>
      // went from 255 to 260 registers, one wavefront per SIMD fewer
      int lo = 1, hi = NS - 1;
      while (lo < NS && !(tp[(lo - 1) * NS + (j - 1)] > LSMALL)) lo++;
      while (hi > 1 && !(tp[(hi - 1) * NS + (j - 1)] > LSMALL)) hi--;
      if (lo > hi) { lo = 1; hi = NS - 1; }
      TSet res = cur[t0 + lo - 1];
      res.like += tp[(lo - 1) * NS + (j - 1)];
      for (int i = lo + 1; i <= hi; i++) {
         const TSet &si = cur[t0 + i - 1];
         ts_merge(res, si.like + tp[(i - 1) * NS + (j - 1)], si.lm, si.path, si, nT, a.nToks, ko, si.align);
      }
      if (res.like > gT) {
         const int st = N.hmmState[ni.w + (j - 2)];
         const float outp = a.score[ud.score0 + (size_t)(t - 1) * a.ns + N.stateSlot[st]];
         res.like += outp;
         if (res.like > mx) mx = res.like;
         if constexpr (ALIGN)
            if (a.alignMode & 2) {                          // pri->states (HRec.c:680-704, -DPHNALG): a record where a token enters state j
               const double alk = res.like - outp - res.lm * a.lmScale;
               const AlignRec *AL = a.al + (size_t)sel * a.alCap;
               if (res.align < 0 || AL[res.align].state != j || AL[res.align].node != n) { res.align = new_align(a, sel, n, j, alk, t - 1, res.align); res.ra[0] = res.align; }
               for (int q = 1; q < res.n; q++)
                  if (res.ra[q] < 0 || AL[res.ra[q]].state != j || AL[res.ra[q]].node != n) res.ra[q] = new_align(a, sel, n, j, alk, t - 1, res.ra[q]);
            }
      } else ts_null_head(res);
      nxt[t0 + j - 1] = res;
   }
   { TSet z = cur[t0]; ts_null_head(z); nxt[t0] = z; }     // entry consumed
   int lo = 2, hi = NS - 1;
   while (lo < NS && !(tp[(lo - 1) * NS + (NS - 1)] > LSMALL)) lo++;
   while (hi > 1 && !(tp[(hi - 1) * NS + (NS - 1)] > LSMALL)) hi--;
   if (lo > hi) { lo = 2; hi = NS - 1; }
   TSet res = nxt[t0 + lo - 1];
   res.like += tp[(lo - 1) * NS + (NS - 1)];
   for (int i = lo + 1; i <= hi; i++) {
      const TSet &si = nxt[t0 + i - 1];
      ts_merge(res, si.like + tp[(i - 1) * NS + (NS - 1)], si.lm, si.path, si, nT, a.nToks, ko, si.align);
   }
   if (res.like > LSMALL) {
      const double w = res.like + N.wdlk[n];
      if (w > wordTop) wordTop = w;
      if constexpr (ALIGN)
         if ((a.alignMode & 1) && !((ni.x >> 12) & 1)) {    // pri->models, not a tee model (HRec.c:762-776): the model's exit record per token
            const double alk = res.like - res.lm * a.lmScale;
            res.align = new_align(a, sel, n, -1, alk, t, res.align); res.ra[0] = res.align;
            for (int q = 1; q < res.n; q++) res.ra[q] = new_align(a, sel, n, -1, alk, t, res.ra[q]);
         }
   } else ts_null_head(res);
   exS = res;
}

// NTHR: the workgroup (DEC_THREADS for one wide recognition network; DEC_SET_THREADS for a network per utterance: alignment and rescoring
// networks of tens to hundreds of nodes, whose NTHR partial sets are 30 KB of LDS, not 120, so that several utterances share a CU).
// SET: the utterance's network and the rows of its score columns come from its descriptor, as in k_decode (decode.hip)
template <int NTHR, bool SET>
__global__ __launch_bounds__(NTHR) void k_decode_n(NArgs a)
{
   __shared__ double red[NTHR / 64];
   __shared__ double red2[NTHR / 64];
   __shared__ float thr[3];
   __shared__ unsigned int usel[3]; __shared__ int uhist[256];
   extern __shared__ unsigned char dynLds[];           // partial sets of a wide node: NTHR x PSet
   PSet *part = (PSet *)dynLds;
   const int u = blockIdx.x, tid = threadIdx.x;
   if (u >= a.nUtt) return;
   const DecUtt ud = a.utt[u];
   // (the record is uniform over the workgroup and read before the kernel's first store, as in k_decode)
   if constexpr (SET) { a.net = a.nets[ud.net]; a.ns = ud.ns; }
   const DecNet &N = a.net;
   const int T = ud.T, nW = N.nWordNodes;
   TSet *cur = a.tokA + ud.tok0, *nxt = a.tokB + ud.tok0, *ex = a.ex + ud.node0;
   double *imax = a.imax + ud.node0;
   const float *tpBase = N.transP;

   { TSet z; ts_null(z);
     for (int i = tid; i < N.nTok; i += NTHR) { cur[i] = z; nxt[i] = z; }
     for (int i = tid; i < N.nNodes; i += NTHR) { ex[i] = z; imax[i] = LZERO; } }
   for (size_t i = tid; i < (size_t)(T + 1) * nW; i += NTHR) a.mark[ud.path0 + i] = 0;
   if (tid == 0) { thr[0] = (float)LSMALL; thr[1] = (float)LSMALL; thr[2] = (float)LSMALL; }
   __syncthreads();

   for (int t = 0; t <= T; t++) {
      if (t >= 1 && a.maxActive > 0) {
         // ---- maximum-model pruning (ProcessObservation HRec.c:1966-1985; dec_prune_threshold, decode_dev.h): when more than maxActive
         // instances are attached, those whose max (a float) lies below the (maxActive+1)-th largest lose every token set before pass 1
         const float gTp = thr[0];
         const float uth = dec_prune_threshold<NTHR>(N.nNodes, a.maxActive, usel, uhist,
                                                            [&](const int n, float &key) { const double v = imax[n]; key = (float)v; return v >= gTp && v > LSMALL; });
         if (uth > (float)LSMALL)
            for (int n = tid; n < N.nNodes; n += NTHR) {
               const double v = imax[n];
               if (!(v >= gTp && v > LSMALL) || !(v < (double)uth)) continue;
               TSet z; ts_null(z);
               imax[n] = LZERO; ex[n] = z;
               const int4 ni = N.nodeInfo[n];
               const int nt = ((ni.x & 15) == HTKAMD_NODE_HMM) ? ((ni.x >> 4) & 255) - 1 : 1;
               for (int i = 0; i < nt; i++) cur[ni.y + i] = z;
            }
         __syncthreads();
      }
      if (t >= 1) {
         const float gT = thr[0], nT = thr[2];             // thresholds of the previous frame
         double myGen = LZERO, myWord = LZERO;
         for (int hk = tid; hk < N.nHmm; hk += NTHR) {
            const int n = N.hmmNodes[hk];
            const int4 ni = N.nodeInfo[n];
            const int NS = (ni.x >> 4) & 255, t0 = ni.y;
            const bool detached = imax[n] < gT;
            bool live = false;
            for (int i = 1; i < NS; i++) {
               if (i > 1 && detached) { TSet z; ts_null(z); cur[t0 + i - 1] = z; }
               if (cur[t0 + i - 1].like > LSMALL) live = true;
            }
            TSet exS; ts_null(exS);
            double mx = LZERO;
            if (live) {
               set_step1<false>(a, ud, 0, n, ni, tpBase + ni.z, cur, nxt, gT, nT, t, KeyOf{nullptr, nW}, exS, mx, myWord);
               if (mx > myGen) myGen = mx;
            } else {
               TSet z; ts_null(z);
               for (int i = 1; i < NS; i++) nxt[t0 + i - 1] = z;
            }
            ex[n] = exS; imax[n] = (double)(float)mx;
         }
         const double genMax = dec_block_max<NTHR>(myGen, red);
         const double wordMax = dec_block_max<NTHR>(myWord, red2);
         if (tid == 0) {
            dec_beam_thresholds(thr, genMax, wordMax, a.genBeam, a.wordBeam);
            thr[2] = dec_nbest_threshold(genMax, a.nBeam);
         }
         __syncthreads();
         { TSet *sw = cur; cur = nxt; nxt = sw; }            // the new column is the current one from here on
      }
      const float gT = thr[0], wT = thr[1], nT = thr[2];
      for (int L = 0; L < N.nLevels; L++) {
         const int l0 = N.levelOffAll[L], lw = N.levelWideAll[L], l1 = N.levelOffAll[L + 1];
         for (int k = l0 + tid; k < lw; k += NTHR) {
            const int n = N.levelNodesAll[k];
            const int4 ni = N.nodeInfo[n];
            const int kind = ni.x & 15;
            TSet st; ts_null(st);
            pull_sets(a, ex, N.predOff[n], N.predOff[n + 1], gT, wT, nT, st);
            if (t == 0 && n == N.initial) { st.like = 0.0; st.lm = 0.0f; st.path = -1; st.n = 1; st.rl[0] = 0.0f; st.rlm[0] = 0.0f; st.rp[0] = -1; }
            TSet e; ts_null(e);
            if (kind == HTKAMD_NODE_HMM) {                  // tee model: StepHMM2
               const int NS = (ni.x >> 4) & 255;
               cur[ni.y] = st;
               e = ex[n];
               const double m2 = (st.like > imax[n]) ? (double)(float)st.like : imax[n];
               if (t >= 1 && m2 < gT) { ts_null(e); imax[n] = LZERO; }
               else {
                  imax[n] = m2;
                  if (st.like > LSMALL) ts_merge(e, st.like + tpBase[ni.z + (NS - 1)], st.lm, st.path, st, nT, a.nToks, KeyOf{nullptr, nW});
               }
            } else if (!(st.like > LSMALL)) imax[n] = LZERO;
            else {
               imax[n] = (double)(float)st.like;
               if (kind == HTKAMD_NODE_WORD) word_exit(a, ud, n, t, st, e);
               else e = st;
            }
            ex[n] = e;
         }
         for (int k = lw; k < l1; k++) {                   // wide fan-in: contiguous runs per thread, then thread 0 in run order
            const int n = N.levelNodesAll[k];
            const int p0 = N.predOff[n], p1 = N.predOff[n + 1];
            const int per = (p1 - p0 + NTHR - 1) / NTHR;
            TSet mine; ts_null(mine);
            const int b0 = p0 + tid * per, b1 = (b0 + per < p1) ? b0 + per : p1;
            if (b0 < p1) pull_sets(a, ex, b0, b1, gT, wT, nT, mine);
            {
               PSet &pm = part[tid];
               pm.like = mine.like; pm.lm = mine.lm; pm.path = mine.path; pm.n = mine.n;
               for (int i = 0; i < mine.n; i++) { pm.rl[i] = mine.rl[i]; pm.rlm[i] = mine.rlm[i]; pm.rp[i] = mine.rp[i]; }
            }
            __syncthreads();
            if (tid == 0) {
               TSet st; ts_null(st);
               for (int q = 0; q < NTHR; q++) {
                  if (!(part[q].like > LSMALL)) continue;
                  TSet pq; ts_null(pq);
                  pq.like = part[q].like; pq.lm = part[q].lm; pq.path = part[q].path; pq.n = part[q].n;
                  for (int i = 0; i < pq.n; i++) { pq.rl[i] = part[q].rl[i]; pq.rlm[i] = part[q].rlm[i]; pq.rp[i] = part[q].rp[i]; pq.ra[i] = -1; }
                  ts_merge(st, pq.like, pq.lm, pq.path, pq, nT, a.nToks, KeyOf{nullptr, nW});
               }
               if (t == 0 && n == N.initial) { st.like = 0.0; st.lm = 0.0f; st.path = -1; st.n = 1; st.rl[0] = 0.0f; st.rlm[0] = 0.0f; st.rp[0] = -1; }
               TSet e; ts_null(e);
               imax[n] = (st.like > LSMALL) ? (double)(float)st.like : LZERO;
               if (st.like > LSMALL) {
                  if (N.kind[n] == HTKAMD_NODE_WORD) word_exit(a, ud, n, t, st, e);
                  else e = st;
               }
               ex[n] = e;
            }
            __syncthreads();
         }
         __syncthreads();
      }
      if (t < T) {
         for (int hk = tid; hk < N.nHmm; hk += NTHR) {
            const int n = N.hmmNodes[hk];
            const int4 ni = N.nodeInfo[n];
            if ((ni.x >> 12) & 1) continue;
            TSet en; ts_null(en);
            pull_sets(a, ex, N.predOff[n], N.predOff[n + 1], gT, wT, nT, en);
            cur[ni.y] = en;
            if (en.like > imax[n]) imax[n] = (double)(float)en.like;
         }
         __syncthreads();
      }
   }

   // ---- CompleteRecognition -> CreateLattice
   if (tid == 0) build_lattice(a, ud, u, ex[N.final], PathView{nullptr, nullptr, nW, N.wordNode});
}

// ---------------------------------------------------------------------------------------------------------------------------------
// k_decode_ord_n -- N-best token passing in the order of HRec's instance list (decode_ord.hip has the design; this is its token-set
// form).  In N-best mode the list's order decides more than exact ties: every TokSetMerge re-bases its relative tokens as floats
// (HRec.c:361-364), so the order in which a node's senders are stepped is in the last bit of every alternative's likelihood -- and in
// which of two alternatives of nearly equal likelihood survives.  The run therefore always walks the list.  The frame loop and the walk
// are decode_ord.h's (ord_frames), the same code k_decode_ord runs; here are the form OrdSets (pass 1 = set_step1, token sets merged
// along the links in link order, each merge by one lane on the set in global memory; StepWord2 allocates its Path record (+ NxtPaths)
// per call), the kernel's prologue and its ending.
__device__ void word_exit_ord(const NArgs &a, const DecUtt &ud, int n, int t, const TSet &st, TSet &e, int pid, int *pathNode, int *pathFrame)
{
   const DecNet &N = a.net;
   e = st;
   e.like += a.wordPen;
   e.like += N.pronProb[n] * a.prScale;
   a.pathPrev[ud.path0 + pid] = st.path; a.pathLike[ud.path0 + pid] = e.like; a.pathLm[ud.path0 + pid] = e.lm;
   pathNode[pid] = n; pathFrame[pid] = t;
   a.altN[ud.path0 + pid] = st.n - 1;
   if (a.alignMode) a.pathAlign[ud.path0 + pid] = st.align;
   for (int k = 1; k < st.n; k++) {
      const size_t z = (ud.path0 + pid) * (NT - 1) + (k - 1);
      a.altLike[z] = e.like + st.rl[k]; a.altLm[z] = st.rlm[k]; a.altPrev[z] = st.rp[k];
      if (a.alignMode) a.altAlign[z] = st.ra[k];
   }
   e.path = pid; e.lm = 0.0f; e.align = -1;
   e.n = 1; e.rp[0] = e.path;                            // rl[0] / rlm[0] / ra[0] stay what the exit set held (AttachInst's rmax: 0, 0, NULL)
}

// The token-set form of the walk (decode_ord.h says what a form is)
struct OrdSets {
   typedef TSet Exit;
   const NArgs &a; const DecUtt &ud; const DecNet &N; const int sel;
   TSet *cur, *nxt, *ex; volatile double *imax;
   const float *tpBase; const KeyOf ko;
   size_t pathCap; int *pathNode, *pathFrame;
   float nT;                    // this form only: TokSetMerge's cut nThresh = genMax - nBeam (HRec.c:2002), floored at LSMALL / 2, not LSMALL

   __device__ __forceinline__ void null_exit(const int n) const { TSet z; ts_null(z); ex[n] = z; }
   __device__ __forceinline__ void null_state(const int i) const { TSet z; ts_null(z); cur[i] = z; nxt[i] = z; }      // both columns
   __device__ __forceinline__ void thresholds(const float *thr) { nT = thr[2]; }
   __device__ __forceinline__ void extra_threshold(float *thr, const double genMax) const
   {
      thr[2] = dec_nbest_threshold(genMax, a.nBeam);
   }
   // this form only: pass 1 wrote the new column into nxt, which is the current one from here on
   __device__ __forceinline__ void end_pass1() { TSet *sw = cur; cur = nxt; nxt = sw; }

   __device__ __forceinline__ void step1(const int n, const int4 ni, const int t, const float gT, double &myGen, double &myWord) const
   {
      if ((ni.x & 15) != HTKAMD_NODE_HMM) {             // StepWord1 (HRec.c:1038): the sets' relative tokens stay as they are (ts_null_head, not ts_null)
         const int t0 = ni.y;
         TSet z = cur[t0]; ts_null_head(z); nxt[t0] = z;
         TSet ze = ex[n]; ts_null_head(ze); ex[n] = ze;
         imax[n] = LZERO;
         return;
      }
      TSet exS; ts_null(exS);
      double mx = LZERO;
      set_step1<true>(a, ud, sel, n, ni, tpBase + ni.z, cur, nxt, gT, nT, t, ko, exS, mx, myWord);
      if (mx > myGen) myGen = mx;
      ex[n] = exS; imax[n] = (double)(float)mx;
   }

   // StepInst2 (HRec.c:1360): lane 0 makes the exit set, then every lane reads it
   __device__ __forceinline__ bool step2(const int n, const int4 ni, const int t, const int lane, volatile OrdShared *vs) const
   {
      const int kind = ni.x & 15, NS = (ni.x >> 4) & 255, t0 = ni.y;
      if (lane == 0) {
         if (kind == HTKAMD_NODE_WORD) {               // StepWord2 (HRec.c:1046): a Path record (+ NxtPaths) per call
            const int pid = vs->nPath;
            if ((size_t)pid >= pathCap) vs->status = -4;
            else {
               TSet x = ex[n];
               const TSet st = cur[t0];
               const float r0 = x.rl[0], m0 = x.rlm[0]; const int a0 = x.ra[0];
               word_exit_ord(a, ud, n, t, st, x, pid, pathNode, pathFrame);
               x.rl[0] = r0; x.rlm[0] = m0; x.ra[0] = a0;
               vs->nPath = pid + 1;
               ex[n] = x;
            }
         } else if (kind == HTKAMD_NODE_NULL) ex[n] = cur[t0];
         else if ((ni.x >> 12) & 1) {                  // tee model: StepHMM2 (HRec.c:790)
            const TSet st = cur[t0];
            TSet x = ex[n];
            ts_merge(x, st.like + tpBase[ni.z + (NS - 1)], st.lm, st.path, st, nT, a.nToks, ko, st.align);
            if (a.alignMode & 1) {                      // HRec.c:817-832
               const double alk = x.like - x.lm * a.lmScale;
               x.align = new_align(a, sel, n, -1, alk, t, x.align); x.ra[0] = x.align;
               for (int q = 1; q < x.n; q++) x.ra[q] = new_align(a, sel, n, -1, alk, t, x.ra[q]);
            }
            ex[n] = x;
         }
      }
      __threadfence_block();
      return vs->status == 0;
   }

   __device__ __forceinline__ TSet exit_of(const int n) const { return ex[n]; }

   // SetEntryState (HRec.c:1303): TokSetMerge into the destination's entry set, the relative tokens' lm shifted by the link's
   __device__ __forceinline__ double set_entry(const TSet &e, const int d, const float lm, const double xl) const
   {
      const int td = N.nodeInfo[d].y;
      TSet x = e;
      for (int q = 0; q < x.n; q++) x.rlm[q] = e.rlm[q] + lm;
      TSet res = cur[td];
      ts_merge(res, xl, e.lm + lm, e.path, x, nT, a.nToks, ko, e.align);
      cur[td] = res;
      return res.like;
   }
};

template <bool SET>      // SET: a network per utterance, as in k_decode_n
__global__ __launch_bounds__(ORD_THREADS) void k_decode_ord_n(NArgs a)
{
   __shared__ double red[ORD_THREADS / 64];
   __shared__ double red2[ORD_THREADS / 64];
   __shared__ float thr[3];
   __shared__ unsigned int usel[3]; __shared__ int uhist[256];
   __shared__ int scan[ORD_THREADS / 64 + 1];
   __shared__ OrdShared sh;
   const int sel = blockIdx.x, tid = threadIdx.x;
   if (sel >= a.nUtt) return;
   const DecUtt ud = a.utt[sel];
   if constexpr (SET) { a.net = a.nets[ud.net]; a.ns = ud.ns; }
   const DecNet &N = a.net;
   const int T = ud.T, u = ud.idx;
   TSet *cur = a.tokA + ud.tok0, *nxt = a.tokB + ud.tok0, *ex = a.ex + ud.node0;
   volatile double *imax = a.imax + ud.node0;
   volatile int *pos = a.list.pos + ud.node0;
   volatile unsigned char *ooo = a.list.ooo + ud.node0;
   int *seqA = a.list.seq + (size_t)sel * 2 * a.list.seqCap, *seqB = seqA + a.list.seqCap;
   const size_t pathCap = 3 * ((size_t)(T + 1) * N.nWordNodes) + (size_t)a.list.pathExtra;
   int *pathNode = a.list.pathNode + ud.path0, *pathFrame = a.list.pathFrame + ud.path0;

   { TSet z; ts_null(z);
     for (int i = tid; i < N.nTok; i += ORD_THREADS) { cur[i] = z; nxt[i] = z; }
     for (int i = tid; i < N.nNodes; i += ORD_THREADS) { ex[i] = z; imax[i] = LZERO; pos[i] = -1; ooo[i] = 0; } }
   for (size_t i = tid; i < pathCap; i += ORD_THREADS) a.mark[ud.path0 + i] = 0;
   if (tid == 0) { thr[0] = (float)LSMALL; thr[1] = (float)LSMALL; thr[2] = (float)LSMALL; sh.tail = 0; sh.nPath = 0; sh.status = 0; sh.base = 0; sh.cn = 0; if (a.alignMode) a.alCount[sel] = 0; }
   __syncthreads();
   OrdCtx c;
   c.N = &N; c.seq = seqA; c.pos = pos; c.ooo = ooo; c.imax = imax; c.seqCap = a.list.seqCap; c.sh = &sh;
   if (tid == 0) {                                          // StartRecognition (HRec.c:1884)
      o_attach(c, N.initial);
      TSet &s0 = cur[N.nodeInfo[N.initial].y];
      s0.like = 0.0; s0.lm = 0.0f; s0.path = -1; s0.n = 1;
      imax[N.initial] = 0.0;
   }
   __threadfence_block();
   __syncthreads();

   OrdSets f{a, ud, N, sel, cur, nxt, ex, imax, N.transP, KeyOf{pathNode, 0}, pathCap, pathNode, pathFrame, (float)LSMALL};
   ord_frames(c, f, OrdLds{red, red2, thr, usel, uhist, scan}, seqA, seqB, T, OrdBeams{a.maxActive, a.genBeam, a.wordBeam, a.lmScale});

   // ---- CompleteRecognition -> CreateLattice.  This form's ending: no batch result to keep, a full table (-4) reported as "did not fit" (-3)
   if (tid == 0) {
      if (a.alignMode && a.alCount[sel] > a.alCap) sh.status = -4;                 // more alignment records than there was room for
      if (sh.status != 0) { a.total[u] = LZERO; a.latN[2 * u] = sh.status == -4 ? -3 : sh.status; a.latN[2 * u + 1] = 0; }
      else {
         TSet fin; ts_null(fin);
         if (pos[N.final] >= 0) fin = ex[N.final];
         build_lattice(a, ud, u, fin, PathView{pathFrame, pathNode, N.nWordNodes, N.wordNode}, sel);
      }
   }
}

// ------------------------------------------------------------------------------------ host side
// The launches.  One network (htkamd_decoder): k_decode_ord_n<false> / k_decode_n<DEC_THREADS, false>, the network in NArgs::net.  A network
// per utterance (htkamd_decoder_set): ONE launch of the SET forms serves every network of the chunk -- in alignment every utterance has a
// network of its own, and a launch per network would be a launch per utterance.
template <int NTHR, bool SET>
static int launch_n(const NArgs &a, int nUtt, bool listOrder, const char *who, hipStream_t s)
{
   hipError_t e = hipSuccess;
   if (listOrder) { hipLaunchKernelGGL((k_decode_ord_n<SET>), dim3(nUtt), dim3(ORD_THREADS), 0, s, a); e = hipGetLastError(); }
   else {
      const size_t lds = sizeof(PSet) * NTHR;
      e = hipFuncSetAttribute((const void *)k_decode_n<NTHR, SET>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e == hipSuccess) { hipLaunchKernelGGL((k_decode_n<NTHR, SET>), dim3(nUtt), dim3(NTHR), lds, s, a); e = hipGetLastError(); }
   }
   if (e != hipSuccess) { htkamd_set_error("%s: launch: %s", who, hipGetErrorString(e)); return HTKAMD_EHIP; }
   return HTKAMD_OK;
}
int htkamd_launch_decode_n(const NArgs &a, int nUtt, bool listOrder, hipStream_t s) { return launch_n<DEC_THREADS, false>(a, nUtt, listOrder, "decoder_run_lattice", s); }
int htkamd_launch_decode_n_set(const NArgs &a, int nUtt, bool listOrder, hipStream_t s) { return launch_n<DEC_SET_THREADS, true>(a, nUtt, listOrder, "decoder_set_run_lattice", s); }

extern "C" int htkamd_decoder_run_lattice(htkamd_decoder *d, const htkamd_decode_config *cfg, int nToks, float nBeam, const float *dX, const int *frameOff, int nUtt,
                                          int maxLatNodes, int maxLatArcs, const htkamd_lattice_out *out, void *stream)
{
   return htkamd_decoder_run_lattice_align(d, cfg, nToks, nBeam, 0, dX, frameOff, nUtt, maxLatNodes, maxLatArcs, 0, out, nullptr, stream);
}

extern "C" int htkamd_decoder_run_lattice_align(htkamd_decoder *d, const htkamd_decode_config *cfg, int nToks, float nBeam, int alignMode, const float *dX, const int *frameOff,
                                                int nUtt, int maxLatNodes, int maxLatArcs, int maxAlign, const htkamd_lattice_out *out, const htkamd_lattice_align_out *alOut,
                                                void *stream)
{
   if (!d || !frameOff) { htkamd_set_error("decoder_run_lattice: bad argument"); return HTKAMD_EINVAL; }
   const int ns = (int)d->usedStates.size();
   const DecUttNet one = {&d->net, 0, ns, 0};
   const DecNRun r = {"decoder_run_lattice", &d->wsN, d->m, d->d_usedStates, 0, [&](int) { return one; }, &d->net, &ns, nullptr, &d->hostModel, htkamd_launch_decode_n,
                      htkamd_decoder_order(d->orderMode), &d->lastTied};
   return htkamd_decoder_run_nbest(r, cfg, nToks, nBeam, dX, frameOff, nUtt, maxLatNodes, maxLatArcs, out, alignMode, maxAlign, alOut, (hipStream_t)stream);
}

int htkamd_decoder_run_nbest(const DecNRun &r, const htkamd_decode_config *cfg, int nToks, float nBeam, const float *dX, const int *frameOff, int nUtt, int maxLatNodes,
                             int maxLatArcs, const htkamd_lattice_out *out, int alignMode, int maxAlign, const htkamd_lattice_align_out *alOut, hipStream_t s)
{
   if (!cfg || nUtt < 0 || !out || !out->nNodes || !out->nArcs || maxLatNodes < 2 || maxLatArcs < 1) { htkamd_set_error("%s: bad argument", r.who); return HTKAMD_EINVAL; }
   if (alignMode < 0 || alignMode > 3 || (alignMode && (maxAlign < 1 || !alOut || !alOut->arcAlignOff || !alOut->alState || !alOut->alModel || !alOut->alDur || !alOut->alLike))) {
      htkamd_set_error("%s_align: bad argument", r.who); return HTKAMD_EINVAL;
   }
   if (nToks < 2 || nToks > NT) { htkamd_set_error("%s: nToks = %d (2..%d tokens per state)", r.who, nToks, NT); return HTKAMD_EINVAL; }
   if (nUtt == 0) return HTKAMD_OK;
   // the list kernel (k_decode_ord_n) unless the static order was asked for: in N-best mode the order of the merges is in every
   // alternative's likelihood, so "exact" is the default here, not a fallback
   if (alignMode && r.orderMode == HTKAMD_ORDER_FAST) { htkamd_set_error("%s_align: alignment records need the list kernel (not HTKAMD_ORDER_FAST)", r.who); return HTKAMD_EINVAL; }
   *r.lastTied = 0;
   const bool one = !r.dNets;
   const int FR = SCORE_TILE_FRAMES, SL = SCORE_TASK_SLOTS;
   const bool listOrder = r.orderMode != HTKAMD_ORDER_FAST;
   const size_t pathMul = listOrder ? DEC_ORD_PATH_MUL : 1, pathExtra = listOrder ? DEC_ORD_PATH_EXTRA : 0;
   DecArena &ws = *r.ws;
   enum { WS_LIST = 32, WS_ALIGN = 40 };      // first slots of the list kernel's buffers and of the alignment records
   DecBatch bt;
   int u0 = 0;
   while (u0 < nUtt) {
      htkamd_decoder_plan_nets(r.netOf, frameOff, u0, nUtt, FR, SL,
                               [&](size_t T, const DecUttNet &un) {
                                  const DecNet &N = *un.N;
                                  return (size_t)un.ns * T * 8 + (size_t)N.nTok * 2 * sizeof(TSet) + (size_t)N.nNodes * (sizeof(TSet) + 8) +
                                         htkamd_dec_path_records(pathMul, T, N.nWordNodes, pathExtra) * (24 + 16 * (NT - 1) + 8) +
                                         (listOrder ? (size_t)htkamd_dec_ord_seq_cap(N.nNodes) * 8 : 0); },
                               0, pathMul, pathExtra, bt);
      if (one) for (DecUtt &ud : bt.utt) ud.ns = 0;      // (the kernels take the network and its rows from their arguments)
      const int u1 = bt.u1, nu = u1 - u0, maxT = bt.maxT;
      const size_t score = bt.score, tok = bt.tok, node = bt.node, path = bt.path;
      // what the chunk's kernels size alike for every utterance: the largest of its networks' (no utterance gets less than the single decoder gives its network)
      int seqCap = 0, maxHmm = 0;
      for (const DecUtt &ud : bt.utt) { seqCap = std::max(seqCap, htkamd_dec_ord_seq_cap(r.nets[ud.net].nNodes)); maxHmm = std::max(maxHmm, r.nets[ud.net].nHmm); }
      ws.begin(s, r.who);
      NArgs a; memset(&a, 0, sizeof(a));
      void *dScore = ws.get(score * 4), *dScoreT = ws.get(score * 4);
      a.tokA = (TSet *)ws.get(tok * sizeof(TSet)); a.tokB = (TSet *)ws.get(tok * sizeof(TSet)); a.ex = (TSet *)ws.get(node * sizeof(TSet)); a.imax = (double *)ws.get(node * 8);
      a.pathPrev = (int *)ws.get(path * 4); a.pathLike = (double *)ws.get(path * 8); a.pathLm = (float *)ws.get(path * 4);
      a.altN = (int *)ws.get(path * 4); a.altPrev = (int *)ws.get(path * 4 * (NT - 1)); a.altLike = (double *)ws.get(path * 8 * (NT - 1)); a.altLm = (float *)ws.get(path * 4 * (NT - 1));
      a.mark = (int *)ws.get(path * 4); a.stack = (int *)ws.get(sizeof(int) * (size_t)nu * 2 * maxLatNodes); a.nodePath = (int *)ws.get(sizeof(int) * (size_t)nu * maxLatNodes);
      void *dUtt = ws.get(sizeof(DecUtt) * nu), *dTasks = ws.get(sizeof(ScoreTask) * bt.tasks.size() + sizeof(int));
      a.latN = (int *)ws.get(sizeof(int) * 2 * nu);
      a.nodeFrame = (int *)ws.get(sizeof(int) * (size_t)nu * maxLatNodes); a.nodeNet = (int *)ws.get(sizeof(int) * (size_t)nu * maxLatNodes); a.nodeLike = (double *)ws.get(8 * (size_t)nu * maxLatNodes);
      a.arcStart = (int *)ws.get(sizeof(int) * (size_t)nu * maxLatArcs); a.arcEnd = (int *)ws.get(sizeof(int) * (size_t)nu * maxLatArcs);
      a.arcAc = (float *)ws.get(4 * (size_t)nu * maxLatArcs); a.arcLm = (float *)ws.get(4 * (size_t)nu * maxLatArcs); a.arcPr = (float *)ws.get(4 * (size_t)nu * maxLatArcs);
      a.arcScore = (double *)ws.get(8 * (size_t)nu * maxLatArcs); a.total = (double *)ws.get(8 * (size_t)nu);
      if (listOrder) {
         ws.seek(WS_LIST);
         a.list.seq = (int *)ws.get(sizeof(int) * (size_t)nu * 2 * seqCap); a.list.seqCap = seqCap; a.list.pos = (int *)ws.get(sizeof(int) * node); a.list.ooo = (unsigned char *)ws.get(node);
         a.list.pathNode = (int *)ws.get(path * 4); a.list.pathFrame = (int *)ws.get(path * 4); a.list.pathExtra = (int)pathExtra;
      }
      if (alignMode) {
         ws.seek(WS_ALIGN);
         // Align records: one per token of a set where it enters a state (-f) and where it leaves a model (-m), never freed within an
         // utterance (the reference collects garbage; here the utterance must fit): frames x model nodes x tokens x (states + 1), capped
         size_t cap = (size_t)(maxT + 1) * (size_t)maxHmm * (size_t)nToks * (size_t)((alignMode & 2 ? 3 : 0) + (alignMode & 1 ? 1 : 0));
         if (cap > ((size_t)1 << 27)) cap = (size_t)1 << 27;
         if (cap * (size_t)nu * sizeof(AlignRec) > ((size_t)16 << 30)) cap = ((size_t)16 << 30) / ((size_t)nu * sizeof(AlignRec));
         a.alignMode = alignMode; a.alCap = (int)cap; a.al = (AlignRec *)ws.get(sizeof(AlignRec) * cap * nu); a.alCount = (int *)ws.get(sizeof(int) * nu);
         a.pathAlign = (int *)ws.get(path * 4); a.altAlign = (int *)ws.get(path * 4 * (NT - 1));
         a.maxAlign = maxAlign; a.arcAlignOff = (int *)ws.get(sizeof(int) * (size_t)nu * (maxLatArcs + 1));
         a.alState = (int *)ws.get(sizeof(int) * (size_t)nu * maxAlign); a.alNode = (int *)ws.get(sizeof(int) * (size_t)nu * maxAlign); a.alDur = (int *)ws.get(sizeof(int) * (size_t)nu * maxAlign);
         a.alLike = (float *)ws.get(sizeof(float) * (size_t)nu * maxAlign);
      }
      int rc = ws.rc;
      if (!rc) rc = htkamd_decoder_score_slots(r.m, r.dUsedStates, cfg->scoreMode, dX, frameOff[u1], bt, one ? r.ns[0] : 0, r.maxNs, dUtt, dTasks, (float *)dScore, (float *)dScoreT,
                                               nullptr, r.who, s);
      if (!rc) {
         if (one) { a.net = r.nets[0]; a.ns = r.ns[0]; } else a.nets = r.dNets;
         a.utt = (const DecUtt *)dUtt; a.nUtt = nu; a.score = (const float *)dScoreT;
         a.genBeam = cfg->genBeam; a.wordBeam = cfg->wordBeam; a.nBeam = nBeam; a.lmScale = cfg->lmScale; a.wordPen = cfg->wordPen; a.prScale = cfg->prScale;
         a.nToks = nToks; a.maxActive = cfg->maxActive > 0 ? cfg->maxActive : 0; a.maxLatNodes = maxLatNodes; a.maxLatArcs = maxLatArcs;
         rc = r.launch(a, nu, listOrder, s);
         if (!rc && listOrder) *r.lastTied += nu;
      }
      std::vector<int> hN(2 * nu), hNF, hNN, hAS, hAE; std::vector<double> hNL, hSc, hT(nu); std::vector<float> hAc, hLm, hPr;
      if (!rc) {
         hNF.resize((size_t)nu * maxLatNodes); hNN.resize(hNF.size()); hNL.resize(hNF.size());
         hAS.resize((size_t)nu * maxLatArcs); hAE.resize(hAS.size()); hAc.resize(hAS.size()); hLm.resize(hAS.size()); hPr.resize(hAS.size()); hSc.resize(hAS.size());
         hipError_t e;
#define D2H(h, dptr) ((e = hipMemcpyAsync((h).data(), (dptr), sizeof((h)[0]) * (h).size(), hipMemcpyDeviceToHost, s)) != hipSuccess)
         if (D2H(hN, a.latN) || D2H(hNF, a.nodeFrame) || D2H(hNN, a.nodeNet) || D2H(hNL, a.nodeLike) || D2H(hAS, a.arcStart) || D2H(hAE, a.arcEnd) ||
             D2H(hAc, a.arcAc) || D2H(hLm, a.arcLm) || D2H(hPr, a.arcPr) || D2H(hSc, a.arcScore) || D2H(hT, a.total) ||
             (e = hipStreamSynchronize(s)) != hipSuccess) { htkamd_set_error("%s: %s", r.who, hipGetErrorString(e)); rc = HTKAMD_EHIP; }
#undef D2H
      } else (void)hipStreamSynchronize(s);
      if (rc) return rc;
      if (alignMode) {
         std::vector<int> hOff((size_t)nu * (maxLatArcs + 1)), hSt((size_t)nu * maxAlign), hNd(hSt.size()), hDu(hSt.size()); std::vector<float> hLk(hSt.size());
         hipError_t e;
         if ((e = hipMemcpy(hOff.data(), a.arcAlignOff, sizeof(int) * hOff.size(), hipMemcpyDeviceToHost)) != hipSuccess ||
             (e = hipMemcpy(hSt.data(), a.alState, sizeof(int) * hSt.size(), hipMemcpyDeviceToHost)) != hipSuccess ||
             (e = hipMemcpy(hNd.data(), a.alNode, sizeof(int) * hNd.size(), hipMemcpyDeviceToHost)) != hipSuccess ||
             (e = hipMemcpy(hDu.data(), a.alDur, sizeof(int) * hDu.size(), hipMemcpyDeviceToHost)) != hipSuccess ||
             (e = hipMemcpy(hLk.data(), a.alLike, sizeof(float) * hLk.size(), hipMemcpyDeviceToHost)) != hipSuccess) { htkamd_set_error("%s_align: %s", r.who, hipGetErrorString(e)); return HTKAMD_EHIP; }
         for (int k = 0; k < nu; k++) {
            const int uu = u0 + k;
            const std::vector<int> &hostModel = r.hostModel[bt.utt[k].net];
            const int na = hN[2 * k] > 0 ? hN[2 * k + 1] : 0;
            for (int i = 0; i <= na; i++) alOut->arcAlignOff[(size_t)uu * (maxLatArcs + 1) + i] = hOff[(size_t)k * (maxLatArcs + 1) + i];
            const int nr = na > 0 ? hOff[(size_t)k * (maxLatArcs + 1) + na] : 0;
            for (int i = 0; i < nr; i++) {
               const size_t o = (size_t)uu * maxAlign + i, si = (size_t)k * maxAlign + i;
               alOut->alState[o] = hSt[si]; alOut->alModel[o] = hostModel[hNd[si]]; alOut->alDur[o] = hDu[si]; alOut->alLike[o] = hLk[si];
            }
         }
      }
      for (int k = 0; k < nu; k++) {
         const int uu = u0 + k;
         const std::vector<int> &hostModel = r.hostModel[bt.utt[k].net];      // (nodeNet / nodePron index the utterance's own network)
         out->nNodes[uu] = hN[2 * k]; out->nArcs[uu] = hN[2 * k + 1];
         if (out->total) out->total[uu] = hT[k];
         const int nn = hN[2 * k] > 0 ? hN[2 * k] : 0, na = hN[2 * k] > 0 ? hN[2 * k + 1] : 0;
         for (int i = 0; i < nn; i++) {
            const size_t o = (size_t)uu * maxLatNodes + i, si = (size_t)k * maxLatNodes + i;
            if (out->nodeFrame) out->nodeFrame[o] = hNF[si];
            if (out->nodeNet) out->nodeNet[o] = hNN[si];
            if (out->nodePron) out->nodePron[o] = hNN[si] >= 0 ? hostModel[hNN[si]] : -1;
            if (out->nodeLike) out->nodeLike[o] = hNL[si];
         }
         for (int i = 0; i < na; i++) {
            const size_t o = (size_t)uu * maxLatArcs + i, si = (size_t)k * maxLatArcs + i;
            if (out->arcStart) out->arcStart[o] = hAS[si];
            if (out->arcEnd) out->arcEnd[o] = hAE[si];
            if (out->arcAc) out->arcAc[o] = hAc[si];
            if (out->arcLm) out->arcLm[o] = hLm[si];
            if (out->arcPr) out->arcPr[o] = hPr[si];
            if (out->arcScore) out->arcScore[o] = hSc[si];
         }
      }
      u0 = u1;
   }
   return HTKAMD_OK;
}

