// netbuild.hip -- the arc list of HBuild's bigram networks from the model's tables (ProcessBoBiGram HBuild.c:368, ProcessMatBiGram :463).
//
// The arcs come in 2N groups, words 1..N twice.  Group r < N is the unigram arc of word r + 1, out of the back-off node (back-off form
// only; the enter word has none).  Group N + r is the row of word r + 1:
//   back-off form   the back-off arc into the back-off node, then one arc per successor of the row in the table's order, the enter word and
//                   a zapped unknown word left out;
//   matrix form     one arc per column 2..N (2..N-1 from the enter word's row), a zapped column left out.
// k_nb_arcs<true> counts a group's arcs, k_lm_scan turns the counts into offsets, k_nb_arcs<false> writes start node, end node and the
// log probability of every arc.  HBuild copies the model's float into the arc (la->lmlike = se->prob): the kernel copies its bits; the
// conversions (text to float, times ln 10, log of a matrix entry) are the model reader's, on the host.
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
#include "hipcheck.h"
#include "devbuf.h"
#include "lstats.h"
#include "lmscan.h"

DEVBUF_OWNER("netbuild")

#define NB_WAVES 4

struct NbTables {
   int mode, N;
   const int *rowOff, *succ;
   const unsigned *val, *rowVal, *uni;
   const int *nodeOf, *rowKeep;
   int enterIdx, zapIdx, backNode;
};

template <bool COUNT>
__global__ __launch_bounds__(NB_WAVES * 64) void k_nb_arcs(NbTables T, int *__restrict__ groupCnt, const int *__restrict__ groupOff, int *__restrict__ arcStart,
                                                          int *__restrict__ arcEnd, unsigned *__restrict__ arcLm)
{
   const int w = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, N = T.N;
   for (int g = (int)blockIdx.x * NB_WAVES + w; g < 2 * N; g += (int)gridDim.x * NB_WAVES) {
      const int i = (g < N ? g : g - N) + 1;
      int at = COUNT ? 0 : groupOff[g];
      if (g < N) {
         const bool has = T.mode == HTKAMD_LM_BACKOFF && T.nodeOf[i] >= 0 && i != T.enterIdx;
         if (lane == 0) {
            if (COUNT) groupCnt[g] = has;
            else if (has) { arcStart[at] = T.backNode; arcEnd[at] = T.nodeOf[i]; arcLm[at] = T.uni[i]; }
         }
         continue;
      }
      if (!T.rowKeep[i]) { if (COUNT && lane == 0) groupCnt[g] = 0; continue; }
      const int from = T.nodeOf[i];
      int nCand, base = 0;
      if (T.mode == HTKAMD_LM_BACKOFF) {
         base = T.rowOff[i]; nCand = T.rowOff[i + 1] - base;
         if (!COUNT && lane == 0) { arcStart[at] = from; arcEnd[at] = T.backNode; arcLm[at] = T.rowVal[i]; }
         at++;
      } else nCand = (i == 1 ? N - 1 : N) - 1;
      for (int t0 = 0; t0 < nCand; t0 += 64) {
         const int t = t0 + lane;
         bool keep = false; int to = 0; unsigned bits = 0;
         if (t < nCand) {
            if (T.mode == HTKAMD_LM_BACKOFF) { const int s = T.succ[base + t]; to = T.nodeOf[s]; keep = to >= 0 && s != T.enterIdx; bits = T.val[base + t]; }
            else { const int j = 2 + t; to = T.nodeOf[j]; keep = j != T.zapIdx && to >= 0; bits = T.val[(size_t)i * (size_t)(N + 1) + j]; }
         }
         const unsigned long long m = __ballot(keep);
         if (!COUNT && keep) {
            const int k = at + __popcll(m & (((unsigned long long)1 << lane) - 1));
            arcStart[k] = from; arcEnd[k] = to; arcLm[k] = bits;
         }
         at += __popcll(m);
      }
      if (COUNT && lane == 0) groupCnt[g] = at;
   }
}

extern "C" int htkamd_netbuild_device(int mode, int N, const int *rowOff, const int *succ, const float *val, const float *rowVal, const float *uni, const int *nodeOf,
                                      const int *rowKeep, int enterIdx, int zapIdx, int backNode, int *arcStart, int *arcEnd, float *arcLm, int arcCap, int *nArcs,
                                      double *kernelMs, void *stream)
{
   const bool bo = mode == HTKAMD_LM_BACKOFF;
   if ((!bo && mode != HTKAMD_LM_MATRIX) || N < 1 || N > 65534 || !val || !nodeOf || !rowKeep || !nArcs || arcCap < 0 || (arcCap > 0 && (!arcStart || !arcEnd || !arcLm)) ||
       (bo && (!rowOff || !rowVal || !uni))) { htkamd_set_error("netbuild: bad argument"); return HTKAMD_EINVAL; }
   // every index a kernel will form, checked here
   size_t nVal, bound;
   if (bo) {
      if (rowOff[1] != 0) { htkamd_set_error("netbuild: the rows do not start at 0"); return HTKAMD_EINVAL; }
      for (int i = 1; i <= N; i++) if (rowOff[i + 1] < rowOff[i]) { htkamd_set_error("netbuild: the offsets of row %d run backwards", i); return HTKAMD_EINVAL; }
      nVal = (size_t)rowOff[N + 1];
      if (nVal > 0 && !succ) { htkamd_set_error("netbuild: bad argument"); return HTKAMD_EINVAL; }
      for (size_t k = 0; k < nVal; k++) if (succ[k] < 1 || succ[k] > N) { htkamd_set_error("netbuild: entry %zu names word %d of %d", k, succ[k], N); return HTKAMD_EINVAL; }
      bound = nVal + 2 * (size_t)N;
   } else { nVal = (size_t)(N + 1) * (size_t)(N + 1); bound = (size_t)N * (size_t)N; }
   if (bound > ((size_t)1 << 30)) { htkamd_set_error("netbuild: %zu arcs in one network", bound); return HTKAMD_EINVAL; }
   *nArcs = 0;
   if (kernelMs) *kernelMs = 0.0;
   if (htkamd_device_count() <= 0) { htkamd_set_error("netbuild: no HIP device"); return HTKAMD_ENODEV; }
   hipStream_t st = (hipStream_t)stream;
   DevBuf dOff, dSucc, dVal, dRowVal, dUni, dNode, dKeep, dCnt, dGOff, dS, dE, dL;
   KernelTimer timer;
   const size_t nW = (size_t)N + 1, nG = 2 * (size_t)N;
   int rc;
   if (bo && ((rc = dOff.upload(rowOff, nW + 1, st)) || (rc = dSucc.upload(succ, nVal, st)) || (rc = dRowVal.upload(rowVal, nW, st)) || (rc = dUni.upload(uni, nW, st)))) return rc;
   if ((rc = dVal.upload(val, nVal, st)) || (rc = dNode.upload(nodeOf, nW, st)) || (rc = dKeep.upload(rowKeep, nW, st)) || (rc = dCnt.reserve<int>(nG + 1)) ||
       (rc = dGOff.reserve<int>(nG + 1)) || (rc = dS.reserve<int>(bound)) || (rc = dE.reserve<int>(bound)) || (rc = dL.reserve<unsigned>(bound)))
      return rc;
   const NbTables T = {mode, N, dOff.as<const int>(), dSucc.as<const int>(), dVal.as<const unsigned>(), dRowVal.as<const unsigned>(), dUni.as<const unsigned>(),
                       dNode.as<const int>(), dKeep.as<const int>(), enterIdx, zapIdx, backNode};
   int blocks = (int)((nG + NB_WAVES - 1) / NB_WAVES);
   if (blocks > 2048) blocks = 2048;
   HIPCHECK(timer.start(st));
   hipLaunchKernelGGL(k_nb_arcs<true>, dim3((unsigned)blocks), dim3(NB_WAVES * 64), 0, st, T, dCnt.as<int>(), nullptr, nullptr, nullptr, nullptr);
   HIPCHECK(hipGetLastError());
   hipLaunchKernelGGL(k_lm_scan, dim3(1), dim3(1024), 0, st, dCnt.as<const int>(), dGOff.as<int>(), (int)nG);
   HIPCHECK(hipGetLastError());
   hipLaunchKernelGGL(k_nb_arcs<false>, dim3((unsigned)blocks), dim3(NB_WAVES * 64), 0, st, T, nullptr, dGOff.as<const int>(), dS.as<int>(), dE.as<int>(), dL.as<unsigned>());
   HIPCHECK(hipGetLastError());
   HIPCHECK(timer.stop(st));
   int total = 0;
   HIPCHECK(hipMemcpyAsync(&total, dGOff.as<int>() + nG, sizeof(int), hipMemcpyDeviceToHost, st));
   HIPCHECK(hipStreamSynchronize(st));
   if (total < 0 || (size_t)total > bound) { htkamd_set_error("netbuild: %d arcs came back, at most %zu can be", total, bound); return HTKAMD_EHIP; }
   *nArcs = total;
   if (total > arcCap) { htkamd_set_error("netbuild: the network has %d arcs, room for %d", total, arcCap); return HTKAMD_EINVAL; }
   if ((rc = dS.download(arcStart, (size_t)total, st)) || (rc = dE.download(arcEnd, (size_t)total, st)) || (rc = dL.download((unsigned *)arcLm, (size_t)total, st))) return rc;
   HIPCHECK(hipStreamSynchronize(st));
   float ms = 0.0f;
   HIPCHECK(timer.ms(&ms));
   if (kernelMs) *kernelMs = ms;
   return HTKAMD_OK;
}
