// treeclust.hip -- the device side of decision-tree state clustering (HHEd's TB command; the driver is host/treeclust.c).
//
// Evaluating a tree node means, for every question, one pass over the node's states that adds each state's statistics to the
// question's "yes" or "no" accumulator (ValidProbNode HHEd.c:2671, ClusterLogL :2611, IncSumSqr :2593), and then the log likelihood of
// the two accumulators (AccSumProb :2574).  Every (question, accumulator column) sum is strictly sequential over the node's items and
// independent of every other, so the reference's float results are reproduced exactly by keeping the order and spreading the sums.
//
// k_tree_split: block (x = node, y = tile of questions), 256 threads.  An accumulator has C = 2D+1 columns (occ, sum[D], sqr[D]).
//   A thread owns one column of TS_QPT questions: 2 * TS_QPT float accumulators in registers (no side, yes side).  The 256 threads are
//   256 / C groups of C threads, a group takes TS_QPT consecutive questions, a block (256 / C) * TS_QPT of them.
//   The node's items are walked IN LIST ORDER in tiles: a tile's item rows ([<= 64][C] floats, at most 16 KB) and the block's answers for
//   those items are staged in LDS once, then every group walks the tile -- an item row is read from memory once per block, not once per
//   question.  A group's threads read consecutive LDS words of a row (no bank conflict) and one answer byte (a broadcast).
//   The add is `acc = answer ? acc + v : acc` on the yes side and the opposite on the no side: a plain float add in list order, no
//   atomics, no reduction tree, nothing fused (-ffp-contract=off, and there is no multiply here).
//   Question number nQ is "no question": every answer FALSE, so its no side is the node's total (tProb's cluster, and with a second
//   item list "list a, then list b" MergeCost's combined cluster, :2785).
//   A state without occupation has an all-zero row (the reference skips it, InitTreeAccs :2550): adding +0.0 leaves every bit alone.
// k_tree_pick: block = node.  AccSumProb of both sides of every question in the reference's operation order (the variance in float,
//   widened; the sum over k in double; returned as float; the two sides added as floats), the outlier rule (:2695), the maximum over
//   the questions, and the CANDIDATES: the questions within a guard band of the maximum, in question order.  Their sums and the
//   node's total go into the node's record; the [nQ+1][2][C] block stays on the device.
//   The device's double log is not the C library's, so the host decides among the candidates with its own log (treeclust.c).  The
//   band ("Decision-tree clustering"): the device log is within 1 ulp (OCML's documented bound for double log), i.e.
//   2^-43 absolutely for |log| < 1024; a side's double sum is therefore off by at most D * occ/2 * 2^-43 (+ D roundings of 2^-53
//   relative), far below a float's spacing -- so a side's float value differs from the host's by at most one float ulp, the float sum
//   of two sides by at most three.  Twice that (the maximum may be off, too) is 6 ulp(M) <= M * 6 * 2^-23, M the larger magnitude of the
//   maximum and the node's own likelihood; the band is M * 2^-20 (8 ulp) plus twice the double bound.
//   A question that cannot win is no candidate: the outlier rule gives it the node's own likelihood, and so does an empty side (the other
//   side then adds the node's very sequence), and ValidProbNode wants strictly more (:2706).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include "internal.h"
#include "hipcheck.h"
#include "devbuf.h"

#define TS_THREADS 256
#define TS_QPT     4
#define TS_TILE    64                                   // items per LDS tile, at most
#define TS_TILE_FLOATS 4096                             // ... and at most this many floats of rows

__global__ __launch_bounds__(TS_THREADS) void k_tree_split(const float *stats, const int *itemCol, const unsigned char *ans, int nCols, int nQ, int C, int TI,
                                                            const htkamd_tree_node *nodes, const int *idx, float *blk)
{
   extern __shared__ float lds[];
   const int G = TS_THREADS / C, QB = G * TS_QPT;       // groups, questions per block
   float *rows = lds;                                   // [TI][C]
   int *its = (int *)(lds + TI * C);                    // [TI]
   unsigned char *ansT = (unsigned char *)(its + TI);   // [QB][TI]
   const int t = threadIdx.x, g = t / C, c = t - g * C;
   const htkamd_tree_node nd = nodes[blockIdx.x];
   const int n = nd.nA + nd.nB;
   const int qBlock = blockIdx.y * QB;
   float no[TS_QPT], yes[TS_QPT];
#pragma unroll
   for (int j = 0; j < TS_QPT; j++) { no[j] = 0.0f; yes[j] = 0.0f; }
   for (int base = 0; base < n; base += TI) {
      const int cnt = (n - base < TI) ? n - base : TI;
      if (t < cnt) { const int pos = base + t; its[t] = idx[pos < nd.nA ? nd.offA + pos : nd.offB + pos - nd.nA]; }
      __syncthreads();
      for (int i = t; i < cnt * C; i += TS_THREADS) { const int r = i / C; rows[i] = stats[(size_t)its[r] * C + (i - r * C)]; }
      for (int i = t; i < QB * cnt; i += TS_THREADS) {
         const int ql = i / cnt, r = i - ql * cnt, q = qBlock + ql;
         ansT[ql * TI + r] = (q < nQ) ? ans[(size_t)q * nCols + (itemCol ? itemCol[its[r]] : its[r])] : (unsigned char)0;
      }
      __syncthreads();
      if (g < G)
         for (int r = 0; r < cnt; r++) {
            const float v = rows[r * C + c];
#pragma unroll
            for (int j = 0; j < TS_QPT; j++) {
               const bool a = ansT[(g * TS_QPT + j) * TI + r] != 0;
               yes[j] = a ? yes[j] + v : yes[j];
               no[j] = a ? no[j] : no[j] + v;
            }
         }
      __syncthreads();
   }
   if (g < G)
#pragma unroll
      for (int j = 0; j < TS_QPT; j++) {
         const int q = qBlock + g * TS_QPT + j;
         if (q > nQ) continue;
         float *o = blk + (((size_t)blockIdx.x * (nQ + 1) + q) * 2) * C;
         o[c] = no[j]; o[C + c] = yes[j];
      }
}

// AccSumProb (HHEd.c:2574)
static __device__ float ts_acc_prob(const float *a, int D)
{
   const float occ = a[0];
   if (!(occ > 0.0f)) return 0.0f;
   double prob = 0.0;
   for (int k = 0; k < D; k++) {
      const float sum = a[1 + k], sqr = a[1 + D + k];
      const double variance = (sqr - (sum * sum / occ)) / occ;
      if (variance <= MINLARG) return (float)LZERO;
      prob += -0.5 * occ * (1.0 + log(HTK_TPI * variance));
   }
   return (float)prob;
}

__global__ __launch_bounds__(TS_THREADS) void k_tree_pick(const float *blk, int nQ, int D, float outlierThresh, int *rec)
{
   extern __shared__ float sp[];                        // [nQ] split likelihoods, then the pick
   __shared__ int nCand, cand[HTKAMD_TREE_MAXCAND];
   const int C = 2 * D + 1, t = threadIdx.x;
   const float *nb = blk + (size_t)blockIdx.x * (nQ + 1) * 2 * C;
   const float *tot = nb + (size_t)nQ * 2 * C;
   const float nodeOcc = tot[0];
   for (int q = t; q < nQ; q += TS_THREADS) {
      const float *no = nb + (size_t)q * 2 * C, *yes = no + C;
      const bool out = !(nodeOcc > 0.0f) || !(no[0] > 0.0f) || !(yes[0] > 0.0f) || (outlierThresh >= 0.0f && (no[0] < outlierThresh || yes[0] < outlierThresh));
      float s = -INFINITY;
      if (!out) { s = ts_acc_prob(no, D); s += ts_acc_prob(yes, D); }
      sp[q] = s;
   }
   __syncthreads();
   if (t == 0) {
      const float tProb = ts_acc_prob(tot, D);
      float mx = tProb;
      for (int q = 0; q < nQ; q++) if (sp[q] > mx) mx = sp[q];
      const double M = fmax(fabs((double)mx), fabs((double)tProb));
      const double lim = (double)mx - (M * 9.5367431640625e-07 + 2.0 * D * (double)nodeOcc * 0.5 * 1.1368683772161603e-13);   // 2^-20, 2^-43
      int n = 0;
      for (int q = 0; q < nQ; q++)
         if ((double)sp[q] >= lim) { if (n < HTKAMD_TREE_MAXCAND) cand[n] = q; n++; }
      nCand = n;
   }
   __syncthreads();
   int *r = rec + (size_t)blockIdx.x * HTKAMD_TREE_REC(C);
   const int n = nCand < HTKAMD_TREE_MAXCAND ? nCand : HTKAMD_TREE_MAXCAND;
   if (t == 0) r[0] = nCand;
   if (t < HTKAMD_TREE_MAXCAND) r[1 + t] = (t < n) ? cand[t] : -1;
   float *rf = (float *)(r + 1 + HTKAMD_TREE_MAXCAND);
   for (int i = t; i < C; i += TS_THREADS) rf[i] = tot[i];
   rf += C;
   for (int i = t; i < n * 2 * C; i += TS_THREADS) { const int k = i / (2 * C); rf[i] = nb[(size_t)cand[k] * 2 * C + (i - k * 2 * C)]; }
}

DEVBUF_OWNER("tree_cluster")
struct htkamd_tree_dev {
   DevBuf stats, cols, ans, nodes, idx, blk, rec;
   int nItems = 0, D = 0, C = 0, nQ = 0, nCols = 0, hasCols = 0, lastNodes = 0;
   hipStream_t st = nullptr;
};

extern "C" void htkamd_tree_dev_close(htkamd_tree_dev *t) { delete t; }

extern "C" int htkamd_tree_dev_open(htkamd_tree_dev **out, const float *itemStats, int nItems, int D, const int *itemCol, const unsigned char *answers,
                                    int nCols, int nQ, void *stream)
{
   if (!out || !itemStats || nItems < 1 || D < 1 || nQ < 0 || nCols < 0 || (nQ > 0 && (!answers || nCols < 1))) { htkamd_set_error("tree_cluster: bad argument"); return HTKAMD_EINVAL; }
   if (2 * D + 1 > TS_THREADS) { htkamd_set_error("tree_cluster: vectors of %d values (at most %d)", D, (TS_THREADS - 1) / 2); return HTKAMD_EINVAL; }
   if (!itemCol && nQ > 0 && nCols < nItems) { htkamd_set_error("tree_cluster: %d answers per question for %d items", nCols, nItems); return HTKAMD_EINVAL; }
   if (itemCol) for (int i = 0; i < nItems; i++) if (itemCol[i] < 0 || itemCol[i] >= nCols) { htkamd_set_error("tree_cluster: item %d has answer column %d of %d", i, itemCol[i], nCols); return HTKAMD_EINVAL; }
   if (htkamd_device_count() <= 0) { htkamd_set_error("tree_cluster: no HIP device"); return HTKAMD_ENODEV; }
   htkamd_tree_dev *t = new htkamd_tree_dev;
   t->nItems = nItems; t->D = D; t->C = 2 * D + 1; t->nQ = nQ; t->nCols = nCols; t->hasCols = itemCol != nullptr; t->st = (hipStream_t)stream;
   int rc = t->stats.upload(itemStats, (size_t)nItems * t->C, t->st);
   if (!rc && itemCol) rc = t->cols.upload(itemCol, (size_t)nItems, t->st);
   if (!rc && nQ > 0) rc = t->ans.upload(answers, (size_t)nQ * nCols, t->st);
   HIPCHECK_RC(rc, devOwner, hipStreamSynchronize(t->st));                      // (the caller's tables may go after the call)
   if (rc) { delete t; return rc; }
   *out = t;
   return HTKAMD_OK;
}

// the sums of every node, nQ questions + the total, into t->blk
static int ts_launch(htkamd_tree_dev *t, const htkamd_tree_node *nodes, int nNodes, const int *idx, int nIdx, int nQ)
{
   if (!t || !nodes || !idx || nNodes < 1 || nIdx < 1) { htkamd_set_error("tree_cluster: bad node batch"); return HTKAMD_EINVAL; }
   for (int b = 0; b < nNodes; b++) {                   // every index the kernel will form, checked here
      const htkamd_tree_node &nd = nodes[b];
      if (nd.nA < 0 || nd.nB < 0 || nd.offA < 0 || nd.offB < 0 || (long long)nd.offA + nd.nA > nIdx || (long long)nd.offB + nd.nB > nIdx) {
         htkamd_set_error("tree_cluster: node %d reaches outside the index list", b); return HTKAMD_EINVAL;
      }
   }
   for (int i = 0; i < nIdx; i++) if (idx[i] < 0 || idx[i] >= t->nItems) { htkamd_set_error("tree_cluster: item index %d of %d", idx[i], t->nItems); return HTKAMD_EINVAL; }
   const int C = t->C, G = TS_THREADS / C, QB = G * TS_QPT;
   const int TI = (TS_TILE_FLOATS / C < TS_TILE) ? TS_TILE_FLOATS / C : TS_TILE;
   const int tiles = (nQ + 1 + QB - 1) / QB;
   if (tiles > 65535) { htkamd_set_error("tree_cluster: %d questions", nQ); return HTKAMD_EINVAL; }
   int rc;
   if ((rc = t->nodes.upload(nodes, (size_t)nNodes, t->st))) return rc;
   if ((rc = t->idx.upload(idx, (size_t)nIdx, t->st))) return rc;
   if ((rc = t->blk.reserve<float>((size_t)nNodes * (nQ + 1) * 2 * C))) return rc;
   const size_t ldsBytes = sizeof(float) * (size_t)TI * C + sizeof(int) * (size_t)TI + (size_t)QB * TI;      // <= 16 KB + 256 B + 340 * 64 B
   hipLaunchKernelGGL(k_tree_split, dim3((unsigned)nNodes, (unsigned)tiles), dim3(TS_THREADS), ldsBytes, t->st,
                      t->stats.as<const float>(), t->hasCols ? t->cols.as<const int>() : (const int *)nullptr, t->ans.as<const unsigned char>(), t->nCols, nQ, C, TI,
                      t->nodes.as<const htkamd_tree_node>(), t->idx.as<const int>(), t->blk.as<float>());
   HIPCHECK(hipGetLastError());
   return HTKAMD_OK;
}

extern "C" int htkamd_tree_dev_split(htkamd_tree_dev *t, const htkamd_tree_node *nodes, int nNodes, const int *idx, int nIdx, float outlierThresh, int *rec)
{
   if (!rec) { htkamd_set_error("tree_cluster: bad node batch"); return HTKAMD_EINVAL; }
   int rc = ts_launch(t, nodes, nNodes, idx, nIdx, t ? t->nQ : 0);
   if (rc) return rc;
   const size_t nRec = (size_t)nNodes * HTKAMD_TREE_REC(t->C);
   if ((rc = t->rec.reserve<int>(nRec))) return rc;
   hipLaunchKernelGGL(k_tree_pick, dim3((unsigned)nNodes), dim3(TS_THREADS), sizeof(float) * (size_t)(t->nQ ? t->nQ : 1), t->st,
                      t->blk.as<const float>(), t->nQ, t->D, outlierThresh, t->rec.as<int>());
   HIPCHECK(hipGetLastError());
   if ((rc = t->rec.download(rec, nRec, t->st))) return rc;
   HIPCHECK(hipStreamSynchronize(t->st));
   t->lastNodes = nNodes;
   return HTKAMD_OK;
}

extern "C" int htkamd_tree_dev_totals(htkamd_tree_dev *t, const htkamd_tree_node *nodes, int nNodes, const int *idx, int nIdx, float *tot)
{
   if (!tot) { htkamd_set_error("tree_cluster: bad node batch"); return HTKAMD_EINVAL; }
   int rc = ts_launch(t, nodes, nNodes, idx, nIdx, 0);
   if (rc) return rc;
   const size_t row = sizeof(float) * (size_t)t->C;     // the no side of the only entry of every node
   HIPCHECK(hipMemcpy2DAsync(tot, row, t->blk.p, 2 * row, row, (size_t)nNodes, hipMemcpyDeviceToHost, t->st));
   HIPCHECK(hipStreamSynchronize(t->st));
   t->lastNodes = 0;
   return HTKAMD_OK;
}

extern "C" int htkamd_tree_dev_block(htkamd_tree_dev *t, int node, float *blk)
{
   if (!t || !blk || node < 0 || node >= t->lastNodes) { htkamd_set_error("tree_cluster: no block %d", node); return HTKAMD_EINVAL; }
   const size_t n = (size_t)(t->nQ + 1) * 2 * t->C;
   HIPCHECK(hipMemcpyAsync(blk, t->blk.as<const float>() + (size_t)node * n, sizeof(float) * n, hipMemcpyDeviceToHost, t->st));
   HIPCHECK(hipStreamSynchronize(t->st));
   return HTKAMD_OK;
}

extern "C" int htkamd_tree_split_sums(const float *itemStats, int nItems, int D, const int *nodeItems, int n, const unsigned char *answers, int nQ,
                                      float *out, void *stream)
{
   if (!itemStats || !nodeItems || !answers || !out || nItems < 1 || n < 1 || nQ < 1 || D < 1) { htkamd_set_error("tree_split_sums: bad argument"); return HTKAMD_EINVAL; }
   htkamd_tree_dev *t = nullptr;
   int rc = htkamd_tree_dev_open(&t, itemStats, nItems, D, nullptr, answers, nItems, nQ, stream);
   if (rc) return rc;
   const int C = 2 * D + 1;
   const htkamd_tree_node nd = {0, n, 0, 0};
   int *rec = (int *)malloc(sizeof(int) * HTKAMD_TREE_REC(C));
   float *blk = (float *)malloc(sizeof(float) * (size_t)(nQ + 1) * 2 * C);
   rc = htkamd_tree_dev_split(t, &nd, 1, nodeItems, n, -1.0f, rec);
   if (!rc) rc = htkamd_tree_dev_block(t, 0, blk);
   if (!rc) memcpy(out, blk, sizeof(float) * (size_t)nQ * 2 * C);
   free(rec); free(blk);
   htkamd_tree_dev_close(t);
   return rc;
}
