// mllr.hip -- the device side of MLLR mean transforms over a regression class tree (the driver is host/mllr.c).
//
// What the reference computes at transform time from its per-Gaussian sums (RegAcc: occ, spSum) is three steps here:
//
//   k_mllr_stats  AccMLLRPDFStats (HAdapt.c:1709) per base class.  For row i of a block of size bs, with xi = [mu_block ; 1]:
//                    G_i[j][k] += (occ * icov_i) * xi_j * xi_k      (j >= k: the lower triangle, the reference's form)
//                    k_i[j]    += spSum_i * xi_j * icov_i
//                 every factor a float product in the reference's order (icov = 1 / var, scale = occ * icov, (scale * mu_j) * mu_k,
//                 (spSum_i * mu_j) * icov), every sum fp64.  The bias row and column are always kept (the reference keeps them under
//                 USEBIAS only; without it the solve reads the leading bs x bs part).  One workgroup owns (class, ML_TI rows, 256 of a
//                 row's (bs+1)(bs+2)/2 + (bs+1) sums): a thread owns ONE (j, k) and its ML_TI row sums in registers; the block's means and
//                 the rows' (scale, spSum, icov) of ML_CH members are staged in LDS once per chunk.  Within a wavefront the lanes read
//                 sMean[m][j] for one m and lane-dependent j < 65: distinct words of one 65-word row (or the same word, a broadcast), so no
//                 bank is asked twice; (scale, spSum, icov) are the same address for every lane.  Members are visited in list order, no
//                 atomics: two runs give the same bits.  Registers: 16 for the sums and a handful more -- occupancy is not register bound.
//                 Members with occ <= MINOCCTHRESH enter no sum (AccMixPDFStats :1793); the node occupation is SetNodeOcc's (:1510), over
//                 ALL members, kept behind the node's sums.
//   k_mllr_tree   an inner node's record = left child's + right child's, nodes in bottom-up order; thread e owns word e of every record, so
//                 the order of the nodes is the only dependency and it is the thread's own.
//   k_mllr_solve  EstMLLRMeanXForm (:2424): one wavefront per (transform, row) solves G_i w = k_i in fp64 by a Cholesky factorisation in
//                 LDS (the reference: InvSVD).  A pivot that is not positive, or below ML_TINY of its diagonal entry, stops the row: the
//                 first such (transform, row) comes back and nothing is written for the caller to install.
//
// k_mllr_apply writes mu' = A mu + b (block diagonal; float products, float sums in index order, the bias last) for one (Gaussian, row)
// per lane into the model's mean table and the exact scorer's interleaved table; htkamd_model_params_changed then rebuilds what derives.
// -ffp-contract=off: nothing is fused.
#include <hip/hip_runtime.h>
#include <math.h>
#include <limits.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "internal.h"
#include "hipcheck.h"
#include "devbuf.h"

#define ML_THREADS 256
#define ML_TI      8
#define ML_CH      32
#define ML_MAXB    HTKAMD_MLLR_MAXBLOCK
#define ML_TINY    1.0e-12

struct MlTask { int c0, bs, row0, nRows, item0; };
struct MlArgs {
   const float *mean, *var, *occ, *spSum;
   const int *memOff, *mem, *classNode, *rowOff;
   const MlTask *tasks;
   double *out; size_t rec;
   int D; float minOcc;
};

__global__ __launch_bounds__(ML_THREADS) void k_mllr_stats(MlArgs a)
{
   __shared__ float sMean[ML_CH][ML_MAXB + 1];
   __shared__ float sRow[ML_CH][ML_TI][3];
   __shared__ float sOcc[ML_CH];
   __shared__ unsigned char sUse[ML_CH];
   const MlTask T = a.tasks[blockIdx.x];
   const int c = blockIdx.y, t = threadIdx.x, D = a.D, bs = T.bs, d = bs + 1, nTri = d * (d + 1) / 2, nItems = nTri + d;
   const int p = T.item0 + t;
   int kind = 0, j = 0, k = 0;                         // 1: G[j][k], 2: k[j]
   if (p < nTri) {
      j = (int)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
      while ((j + 1) * (j + 2) / 2 <= p) j++;
      while (j * (j + 1) / 2 > p) j--;
      k = p - j * (j + 1) / 2; kind = 1;
   } else if (p < nItems) { j = p - nTri; k = bs; kind = 2; }
   const bool hasJ = j < bs, hasK = k < bs, occOwner = blockIdx.x == 0 && t == 0;
   double acc[ML_TI], occSum = 0.0;
#pragma unroll
   for (int r = 0; r < ML_TI; r++) acc[r] = 0.0;
   const int m0 = a.memOff[c], m1 = a.memOff[c + 1];
   for (int base = m0; base < m1; base += ML_CH) {
      const int n = min(ML_CH, m1 - base);
      __syncthreads();
      for (int e = t; e < n * bs; e += ML_THREADS) { const int mm = e / bs, jj = e - mm * bs; sMean[mm][jj] = a.mean[(size_t)a.mem[base + mm] * D + T.c0 + jj]; }
      for (int e = t; e < n * ML_TI; e += ML_THREADS) {
         const int mm = e / ML_TI, r = e - mm * ML_TI;
         if (r < T.nRows) {
            const int g = a.mem[base + mm];
            const size_t x = (size_t)g * D + T.row0 + r;
            const float icov = __fdiv_rn(1.0f, a.var[x]);
            sRow[mm][r][0] = __fmul_rn(a.occ[g], icov); sRow[mm][r][1] = a.spSum[x]; sRow[mm][r][2] = icov;
         }
      }
      if (t < n) { const float o = a.occ[a.mem[base + t]]; sOcc[t] = o; sUse[t] = o > a.minOcc; }
      __syncthreads();
      if (occOwner) for (int mm = 0; mm < n; mm++) occSum += (double)sOcc[mm];
      if (kind)
         for (int mm = 0; mm < n; mm++) {
            if (!sUse[mm]) continue;
            const float mj = hasJ ? sMean[mm][j] : 1.0f, mk = hasK ? sMean[mm][k] : 1.0f;
#pragma unroll
            for (int r = 0; r < ML_TI; r++)
               if (r < T.nRows) {
                  float v;
                  if (kind == 1) { v = sRow[mm][r][0]; if (hasJ) v = __fmul_rn(v, mj); if (hasK) v = __fmul_rn(v, mk); }
                  else { v = sRow[mm][r][1]; if (hasJ) v = __fmul_rn(v, mj); v = __fmul_rn(v, sRow[mm][r][2]); }
                  acc[r] += (double)v;
               }
         }
   }
   double *out = a.out + (size_t)a.classNode[c] * a.rec;
   if (kind)
#pragma unroll
      for (int r = 0; r < ML_TI; r++) if (r < T.nRows) out[a.rowOff[T.row0 + r] + p] = acc[r];
   if (occOwner) out[a.rec - 1] = occSum;
}

__global__ __launch_bounds__(256) void k_mllr_tree(double *out, size_t rec, const int *inner, int nInner, const int *left, const int *right)
{
   const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
   if (e >= rec) return;
   for (int q = 0; q < nInner; q++) {
      const int n = inner[q];
      out[(size_t)n * rec + e] = out[(size_t)left[n] * rec + e] + out[(size_t)right[n] * rec + e];
   }
}

struct MlSolve {
   const double *stats; size_t rec;
   const int *rowOff, *rowC0, *rowBs, *xNode;
   int D, useBias, maxd;
   float *A, *bias; double *W; int *bad;
};

__global__ __launch_bounds__(64) void k_mllr_solve(MlSolve a)
{
   __shared__ double L[ML_MAXB + 1][ML_MAXB + 2];
   __shared__ double y[ML_MAXB + 1], diag0[ML_MAXB + 1];
   const int i = blockIdx.x, x = blockIdx.y, lane = threadIdx.x, bs = a.rowBs[i], d = bs + 1, n = a.useBias ? d : bs;
   const double *src = a.stats + (size_t)a.xNode[x] * a.rec + a.rowOff[i];
   for (int r = lane; r < n; r += 64) {
      for (int c = 0; c <= r; c++) L[r][c] = src[r * (r + 1) / 2 + c];
      y[r] = src[d * (d + 1) / 2 + r];
      diag0[r] = L[r][r];
   }
   __syncthreads();
   for (int c = 0; c < n; c++) {
      const double pv = L[c][c];
      if (!(pv > 0.0) || !(pv > ML_TINY * diag0[c])) {            // every lane reads the same words: the exit is uniform
         if (lane == 0) atomicMin(a.bad, x * a.D + i);
         return;
      }
      const double s = sqrt(pv);
      __syncthreads();
      for (int r = lane; r < n; r += 64) { if (r == c) L[r][c] = s; else if (r > c) L[r][c] = L[r][c] / s; }
      __syncthreads();
      for (int r = lane; r < n; r += 64)
         if (r > c) { const double lrc = L[r][c]; for (int k = c + 1; k <= r; k++) L[r][k] -= lrc * L[k][c]; }
      __syncthreads();
   }
   for (int c = 0; c < n; c++) {                                   // L z = k
      const double z = y[c] / L[c][c];
      __syncthreads();
      for (int r = lane; r < n; r += 64) { if (r == c) y[r] = z; else if (r > c) y[r] -= L[r][c] * z; }
      __syncthreads();
   }
   for (int c = n - 1; c >= 0; c--) {                              // L' w = z
      const double w = y[c] / L[c][c];
      __syncthreads();
      for (int r = lane; r < n; r += 64) { if (r == c) y[r] = w; else if (r < c) y[r] -= L[c][r] * w; }
      __syncthreads();
   }
   const size_t row = (size_t)x * a.D + i;
   for (int r = lane; r < n; r += 64) {
      if (r < bs) a.A[row * a.D + a.rowC0[i] + r] = (float)y[r]; else a.bias[row] = (float)y[r];
      if (a.W) a.W[row * a.maxd + r] = y[r];
   }
}

struct MlApply {
   const float *src, *A, *bias; const int *gaussX, *rowC0, *rowBs;
   float *mean, *gparam; int G, D, PS;
};

// gaussX[g]: the Gaussian's transform (0-based), -1 none: the mean is copied as it is.  A NULL: a plain copy (restore)
__global__ __launch_bounds__(256) void k_mllr_apply(MlApply a)
{
   const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
   if (e >= (size_t)a.G * a.D) return;
   const int g = (int)(e / a.D), i = (int)(e - (size_t)g * a.D);
   const float *mu = a.src + (size_t)g * a.D;
   float v = mu[i];
   const int x = a.A ? a.gaussX[g] : -1;
   if (x >= 0) {
      const int c0 = a.rowC0[i], bs = a.rowBs[i];
      const float *row = a.A + ((size_t)x * a.D + i) * a.D + c0;
      v = __fmul_rn(row[0], mu[c0]);
      for (int j = 1; j < bs; j++) v = __fadd_rn(v, __fmul_rn(row[j], mu[c0 + j]));
      if (a.bias) v = __fadd_rn(v, a.bias[(size_t)x * a.D + i]);
   }
   a.mean[e] = v;
   a.gparam[(size_t)g * a.PS + 2 * i] = v;
}

// ------------------------------------------------------------------------------------------ host side of the device
DEVBUF_OWNER("mllr")

struct htkamd_mllr_dev {
   DevBuf mean, var, occ, spSum, memOff, mem, classNode, rowOff, rowC0, rowBs, tasks, inner, left, right, stats, xNode, A, bias, W, bad;
   int D = 0, nNodes = 0, useBias = 0, maxd = 0;
   size_t rec = 0;
   hipStream_t st = nullptr;
   KernelTimer timer;
   float ms[3] = {0.0f, 0.0f, 0.0f};
};

template <typename Launch> static int ml_timed(htkamd_mllr_dev *t, int which, Launch launch)
{
   int rc = HTKAMD_OK; float ms = 0.0f;
   HIPCHECK_RC(rc, devOwner, t->timer.start(t->st));
   if (!rc) launch();
   HIPCHECK_RC(rc, devOwner, hipGetLastError());
   HIPCHECK_RC(rc, devOwner, t->timer.stop(t->st));
   HIPCHECK_RC(rc, devOwner, hipStreamSynchronize(t->st));
   HIPCHECK_RC(rc, devOwner, t->timer.ms(&ms));
   if (!rc) t->ms[which] += ms;
   return rc;
}

// The job was checked by host/mllr.c (ml_job_check): members in 0 .. G-1, blocks that sum to D, each 1 .. ML_MAXB, a binary tree whose
// inner nodes are listed children first.
extern "C" int htkamd_mllr_dev_stats(const htkamd_mllr_job *job, htkamd_mllr_dev **out, double *nodeOcc, void *stream)
{
   if (!job || !out || !nodeOcc) { htkamd_set_error("mllr: bad argument"); return HTKAMD_EINVAL; }
   if (htkamd_device_count() <= 0) { htkamd_set_error("mllr: no HIP device"); return HTKAMD_ENODEV; }
   const int D = job->D, G = job->G, nNodes = job->nNodes, nClass = job->nClass;
   const size_t rec = htkamd_mllr_record_len(D, job->nBlocks, job->blockSize);
   if (!rec || G < 1 || nNodes < 1 || nClass < 1) { htkamd_set_error("mllr: bad job"); return HTKAMD_EINVAL; }
   htkamd_mllr_dev *t = new htkamd_mllr_dev();
   t->D = D; t->nNodes = nNodes; t->useBias = job->useBias; t->rec = rec; t->st = (hipStream_t)stream;
   std::vector<int> rowOff((size_t)D + 1), rowC0((size_t)D), rowBs((size_t)D), inner, classNode((size_t)nClass, 0);
   std::vector<MlTask> tasks;
   for (int b = 0, c0 = 0, off = 0; b < job->nBlocks; b++) {
      const int bs = job->blockSize[b], d = bs + 1, nItems = d * (d + 1) / 2 + d;
      if (d > t->maxd) t->maxd = d;
      for (int i = 0; i < bs; i++) { rowOff[c0 + i] = off; rowC0[c0 + i] = c0; rowBs[c0 + i] = bs; off += nItems; }
      for (int r0 = 0; r0 < bs; r0 += ML_TI)
         for (int it = 0; it < nItems; it += ML_THREADS) tasks.push_back(MlTask{c0, bs, c0 + r0, bs - r0 < ML_TI ? bs - r0 : ML_TI, it});
      c0 += bs; rowOff[c0] = off;
   }
   for (int n = 0; n < nNodes; n++) if (job->termClass[n] >= 0) classNode[job->termClass[n]] = n;
   for (int q = 0; q < job->nInner; q++) inner.push_back(job->inner[q]);
   const size_t nG = (size_t)G;
   int rc = t->mean.upload(job->mean, nG * D, t->st);
   if (!rc) rc = t->var.upload(job->var, nG * D, t->st);
   if (!rc) rc = t->occ.upload(job->occ, nG, t->st);
   if (!rc) rc = t->spSum.upload(job->spSum, nG * D, t->st);
   if (!rc) rc = t->memOff.upload(job->memOff, (size_t)nClass + 1, t->st);
   if (!rc) rc = t->mem.upload(job->mem, (size_t)job->memOff[nClass], t->st);
   if (!rc) rc = t->classNode.upload(classNode, t->st);
   if (!rc) rc = t->rowOff.upload(rowOff, t->st);
   if (!rc) rc = t->rowC0.upload(rowC0, t->st);
   if (!rc) rc = t->rowBs.upload(rowBs, t->st);
   if (!rc) rc = t->tasks.upload(tasks, t->st);
   if (!rc && !inner.empty()) rc = t->inner.upload(inner, t->st);
   if (!rc) rc = t->left.upload(job->left, (size_t)nNodes, t->st);
   if (!rc) rc = t->right.upload(job->right, (size_t)nNodes, t->st);
   if (!rc) rc = t->stats.reserve<double>((size_t)nNodes * rec);
   if (!rc) {
      MlArgs a;
      a.mean = t->mean.as<const float>(); a.var = t->var.as<const float>(); a.occ = t->occ.as<const float>(); a.spSum = t->spSum.as<const float>();
      a.memOff = t->memOff.as<const int>(); a.mem = t->mem.as<const int>(); a.classNode = t->classNode.as<const int>(); a.rowOff = t->rowOff.as<const int>();
      a.tasks = t->tasks.as<const MlTask>(); a.out = t->stats.as<double>(); a.rec = rec; a.D = D; a.minOcc = job->minOcc;
      rc = ml_timed(t, 0, [&] { hipLaunchKernelGGL(k_mllr_stats, dim3((unsigned)tasks.size(), (unsigned)nClass), dim3(ML_THREADS), 0, t->st, a); });
   }
   if (!rc && !inner.empty())
      rc = ml_timed(t, 1, [&] {
         hipLaunchKernelGGL(k_mllr_tree, dim3((unsigned)((rec + 255) / 256)), dim3(256), 0, t->st, t->stats.as<double>(), rec, t->inner.as<const int>(), (int)inner.size(),
                            t->left.as<const int>(), t->right.as<const int>());
      });
   HIPCHECK_RC(rc, devOwner, hipMemcpy2DAsync(nodeOcc, sizeof(double), t->stats.as<double>() + rec - 1, sizeof(double) * rec, sizeof(double), (size_t)nNodes,
                                              hipMemcpyDeviceToHost, t->st));      // the records' last words
   HIPCHECK_RC(rc, devOwner, hipStreamSynchronize(t->st));
   if (rc) { delete t; return rc; }
   *out = t;
   return HTKAMD_OK;
}

extern "C" int htkamd_mllr_dev_fetch(htkamd_mllr_dev *t, double *stats)
{
   if (!t || !stats) { htkamd_set_error("mllr: bad argument"); return HTKAMD_EINVAL; }
   int rc = t->stats.download(stats, (size_t)t->nNodes * t->rec, t->st);
   HIPCHECK_RC(rc, devOwner, hipStreamSynchronize(t->st));
   return rc;
}

// A [nX][D][D] (zero outside the blocks), bias [nX][D] (untouched without a bias), W [nX][D][maxd] or NULL: the fp64 rows.
// HTKAMD_ERANGE with *badX, *badRow (0-based) for the first row whose matrix is not positive definite; the outputs are then not written.
extern "C" int htkamd_mllr_dev_solve(htkamd_mllr_dev *t, int nX, const int *xNode, float *A, float *bias, double *W, int *badX, int *badRow)
{
   if (!t || nX < 1 || !xNode || !A || !bias) { htkamd_set_error("mllr: bad argument"); return HTKAMD_EINVAL; }
   for (int x = 0; x < nX; x++) if (xNode[x] < 0 || xNode[x] >= t->nNodes) { htkamd_set_error("mllr: transform %d at node %d of %d", x + 1, xNode[x] + 1, t->nNodes); return HTKAMD_EINVAL; }
   const size_t D = (size_t)t->D, nA = (size_t)nX * D * D, nB = (size_t)nX * D, nW = (size_t)nX * D * t->maxd;
   const int none = INT_MAX;
   int rc = t->xNode.upload(xNode, (size_t)nX, t->st);
   if (!rc) rc = t->A.reserve<float>(nA);
   if (!rc) rc = t->bias.reserve<float>(nB);
   if (!rc && W) rc = t->W.reserve<double>(nW);
   if (!rc) rc = t->bad.upload(&none, 1, t->st);
   HIPCHECK_RC(rc, devOwner, hipMemsetAsync(t->A.as<float>(), 0, sizeof(float) * nA, t->st));
   HIPCHECK_RC(rc, devOwner, hipMemsetAsync(t->bias.as<float>(), 0, sizeof(float) * nB, t->st));
   if (W) HIPCHECK_RC(rc, devOwner, hipMemsetAsync(t->W.as<double>(), 0, sizeof(double) * nW, t->st));
   if (rc) return rc;
   MlSolve a;
   a.stats = t->stats.as<const double>(); a.rec = t->rec; a.rowOff = t->rowOff.as<const int>(); a.rowC0 = t->rowC0.as<const int>(); a.rowBs = t->rowBs.as<const int>();
   a.xNode = t->xNode.as<const int>(); a.D = t->D; a.useBias = t->useBias; a.maxd = t->maxd;
   a.A = t->A.as<float>(); a.bias = t->bias.as<float>(); a.W = W ? t->W.as<double>() : nullptr; a.bad = t->bad.as<int>();
   rc = ml_timed(t, 2, [&] { hipLaunchKernelGGL(k_mllr_solve, dim3((unsigned)t->D, (unsigned)nX), dim3(64), 0, t->st, a); });
   int bad = none;
   if (!rc) rc = t->bad.download(&bad, 1, t->st);
   HIPCHECK_RC(rc, devOwner, hipStreamSynchronize(t->st));
   if (rc) return rc;
   if (bad != none) {
      if (badX) *badX = bad / t->D;
      if (badRow) *badRow = bad % t->D;
      return HTKAMD_ERANGE;
   }
   rc = t->A.download(A, nA, t->st);
   if (!rc && t->useBias) rc = t->bias.download(bias, nB, t->st);
   if (!rc && W) rc = t->W.download(W, nW, t->st);
   HIPCHECK_RC(rc, devOwner, hipStreamSynchronize(t->st));
   return rc;
}

extern "C" void htkamd_mllr_dev_times(const htkamd_mllr_dev *t, float *ms) { for (int k = 0; k < 3; k++) ms[k] = t ? t->ms[k] : 0.0f; }
extern "C" void htkamd_mllr_dev_close(htkamd_mllr_dev *t) { delete t; }

// ------------------------------------------------------------------------------------------ the model's means
static int ml_put(htkamd_model *m, const float *src, const float *dA, const float *dBias, const int *dGaussX, const int *dC0, const int *dBs, hipStream_t s)
{
   MlApply a;
   a.src = src; a.A = dA; a.bias = dBias; a.gaussX = dGaussX; a.rowC0 = dC0; a.rowBs = dBs;
   a.mean = m->d_mean; a.gparam = m->d_gparam; a.G = m->G; a.D = m->D; a.PS = m->PS;
   const size_t nEl = (size_t)m->G * m->D;
   hipLaunchKernelGGL(k_mllr_apply, dim3((unsigned)((nEl + 255) / 256)), dim3(256), 0, s, a);
   HIPCHECK(hipGetLastError());
   return htkamd_model_params_changed(m, s, 1);
}

// gaussX [G]: transform (0-based) of every Gaussian or -1; A [nX][D][D], bias [nX][D] or NULL; rowC0 / rowBs [D]: the row's block
extern "C" int htkamd_mllr_dev_apply(htkamd_model *m, int nX, const float *A, const float *bias, const int *gaussX, const int *rowC0, const int *rowBs, void *stream)
{
   if (htkamd_device_count() <= 0) { htkamd_set_error("mllr_apply: no HIP device"); return HTKAMD_ENODEV; }
   hipStream_t s = (hipStream_t)stream;
   const size_t D = (size_t)m->D, nEl = (size_t)m->G * D;
   if (nEl >= ((size_t)1 << 31)) { htkamd_set_error("mllr_apply: %zu mean elements", nEl); return HTKAMD_EMODEL; }
   DevBuf dA, dB, dX, dC0, dBs;
   int rc = htkamd_model_device_tables(m);               // (the host copies are read back from the device's linear tables afterwards)
   if (!rc) rc = dA.upload(A, (size_t)nX * D * D, s);
   if (!rc && bias) rc = dB.upload(bias, (size_t)nX * D, s);
   if (!rc) rc = dX.upload(gaussX, (size_t)m->G, s);
   if (!rc) rc = dC0.upload(rowC0, D, s);
   if (!rc) rc = dBs.upload(rowBs, D, s);
   if (rc) return rc;
   float *saved = nullptr;
   HIPCHECK(hipMalloc((void **)&saved, sizeof(float) * nEl));
   hipError_t e = hipMemcpyAsync(saved, m->d_mean, sizeof(float) * nEl, hipMemcpyDeviceToDevice, s);
   if (e != hipSuccess) { (void)hipFree(saved); HIPCHECK(e); }
   rc = ml_put(m, saved, dA.as<const float>(), bias ? dB.as<const float>() : nullptr, dX.as<const int>(), dC0.as<const int>(), dBs.as<const int>(), s);
   e = hipStreamSynchronize(s);
   if (rc || e != hipSuccess) {
      // the kernel may have run: put the means back before the copy goes (every derived table is marked stale and follows on its next use)
      MlApply a;
      a.src = saved; a.A = nullptr; a.bias = nullptr; a.gaussX = nullptr; a.rowC0 = nullptr; a.rowBs = nullptr;
      a.mean = m->d_mean; a.gparam = m->d_gparam; a.G = m->G; a.D = m->D; a.PS = m->PS;
      hipLaunchKernelGGL(k_mllr_apply, dim3((unsigned)((nEl + 255) / 256)), dim3(256), 0, s, a);
      (void)hipStreamSynchronize(s);
      (void)hipFree(saved);
      if (!rc) HIPCHECK(e);
      return rc;
   }
   m->d_mllrMean = saved;
   return HTKAMD_OK;
}

extern "C" int htkamd_mllr_dev_restore(htkamd_model *m, void *stream)
{
   hipStream_t s = (hipStream_t)stream;
   const int rc = ml_put(m, m->d_mllrMean, nullptr, nullptr, nullptr, nullptr, nullptr, s);
   HIPCHECK(hipStreamSynchronize(s));
   if (rc) return rc;
   (void)hipFree(m->d_mllrMean);
   m->d_mllrMean = nullptr;
   return HTKAMD_OK;
}

extern "C" int htkamd_mllr_model_state(const char *who, const htkamd_model *m, int *D, int *G, int *adapted)
{
   if (!m) { htkamd_set_error("%s: no model", who); return HTKAMD_EINVAL; }
   if (m->NSt > 1) { htkamd_set_error("%s: a set with more than one stream (%d) is not supported", who, m->NSt); return HTKAMD_EMODEL; }
   if (m->fullc) { htkamd_set_error("%s: FULLC sets are not supported", who); return HTKAMD_EMODEL; }
   if (m->tiedMix) { htkamd_set_error("%s: tied-mixture sets are not supported", who); return HTKAMD_EMODEL; }
   if (m->h_meanLeader) { htkamd_set_error("%s: sets with shared mean vectors (~u) are not supported", who); return HTKAMD_EMODEL; }
   if (D) *D = m->D;
   if (G) *G = m->G;
   if (adapted) *adapted = m->d_mllrMean != nullptr;
   return HTKAMD_OK;
}
