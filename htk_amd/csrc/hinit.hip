// hinit.hip -- Viterbi training from labelled tokens (HTKTools/HInit.c) for every model of a list in one call, and FlatCluster
// (HTKLib/HTrain.c:763) for any number of pools in one launch.  The refusals and the host twin of the pool listing: host/hinit.c.  What the
// call shares with htkamd_hrest -- the model / token tables, the snapshot and k_unit_restore, the block scan, the gather, the float
// transition row, the way out of the call, an error's included -- is unit_train.h; here is HInit's own arithmetic.
//
// k_hi_count / k_hi_scan / k_hi_pooloff / k_hi_fill: UCollectData (HInit.c:505).  A pool is the frames of one (model, emitting state) in
//   token order, then frame order; the states of a token's frames never decrease, so a token's share of a pool is one run of rows:
//   per-token counts, an exclusive scan over the model's tokens per pool (a workgroup per pool), a scan over the pool sizes, a fill.
// k_flat_cluster: one workgroup per pool, the whole of FlatCluster with its control flow (k_dc_merge's arrangement in datacluster.hip).
//   Centres, average costs and sizes live in LDS; the assignment and the cost of every item in memory.  The reference's arithmetic with
//   every rounding written out: a lane per item for Distance (:424: float differences, the double sum of squares in dimension order, the
//   double square root rounded to float) and the first strict minimum (AllocateVectors :482); a lane per cluster for the cost chains
//   and one for the total, float adds in item order; a lane per (cluster, dimension) for FindCentres (:562, float adds in item order,
//   a float divide) and FindCovariance (:587, double sums in item order, a double divide rounded to float).  BiggestCluster (:649,
//   with its quirk: the running maximum moves even where the cluster is too small to be chosen), FullestCluster (:665) and the
//   bookkeeping of AllocateVectors (averages up to the first cluster below MIN_CLUST_SIZE only) are one thread's.
// k_hi_init: UniformSegment (HInit.c:533): weights csize / nItems, centres, floored variances -- what uFlags selects -- into the
//   model's arrays, a workgroup per model; a model with a failed pool is left alone.
// Passes (EstimateModel :1205): the rows of the running models' tokens are gathered behind one another (k_hi_gather) and aligned in one
//   htkamd_viterbi_align_mode call; k_hi_logp: a lane per model, the float sum of its tokens' log probabilities in token order;
//   k_hi_best: a lane per frame, FindBestMixes (:739); k_hi_acc: a wavefront per (token, state) segment, UpdateCounts (:878) into fp64
//   sums with atomic adds (lanes are dimensions; a run of frames with the same component is summed in registers first); k_hi_update: a
//   workgroup per model, UpWeights / UpMeans / UpVars / UpTrans (:997-1097).  Whoever writes a model's parameters rebuilds the derived
//   tables of its Gaussians behind a barrier (gauss_derive.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "internal.h"
#include "hipcheck.h"
#include "hinit_seg.h"
#include "unit_train.h"

#define HI_THREADS     256
#define FC_MIN_CLUST   3                                  // MIN_CLUST_SIZE, HTrain.c:69
#define FC_MAX_ITER    10                                 // MAX_CLUST_ITER, HTrain.c:70
#define FC_MAX_NC      (HI_THREADS - 1)                   // a lane per cluster and one for the total
#define FC_MAX_LDS     (60 * 1024)

// ------------------------------------------------------------------------------------------ FlatCluster
struct FcArgs {
   const float *X; int D;
   const int *poolOff, *items, *nc, *cOff;
   float minVar;
   int *size; float *centre, *var; int *assign; float *cost; int *status;
};

// FindCentres(1, k)
static __device__ void fc_centres(const FcArgs &a, int k, int n, const int *item, const int *cmap, float *ctr, const int *csize)
{
   const int D = a.D;
   for (int e = threadIdx.x; e < k * D; e += HI_THREADS) {
      const int c = e / D, d = e - c * D;
      float s = 0.0f;
      for (int i = 0; i < n; i++) if (cmap[i] == c) s = __fadd_rn(s, a.X[(size_t)item[i] * D + d]);
      ctr[e] = __fdiv_rn(s, (float)csize[c]);
   }
   __syncthreads();
}

// Perturb(n, n, n2)
static __device__ void fc_perturb(int D, float *ctr, int from, int n2)
{
   for (int d = threadIdx.x; d < D; d += HI_THREADS) {
      const float v = ctr[from * D + d];
      float x = (float)fabs(__dmul_rn((double)v, 0.01));
      if ((double)x < 0.0001) x = 0.0001f;
      const float up = __fadd_rn(v, x);
      if (n2 == from) ctr[from * D + d] = __fsub_rn(up, x);
      else { ctr[from * D + d] = up; ctr[n2 * D + d] = __fsub_rn(v, x); }
   }
   __syncthreads();
}

// AllocateVectors over clusters 0 .. k-1: *sCe = 1 + the first cluster with fewer than MIN_CLUST_SIZE items (0: none), *sNew the total cost
static __device__ void fc_allocate(const FcArgs &a, int k, int n, const int *item, int *cmap, float *mn, const float *ctr, float *ave, int *csize, int *sCe, float *sNew)
{
   const int D = a.D, t = threadIdx.x;
   for (int i = t; i < n; i += HI_THREADS) {
      const float *x = a.X + (size_t)item[i] * D;
      float best = 0.0f; int bi = 0;
      for (int c = 0; c < k; c++) {
         double s = 0.0;
         for (int d = 0; d < D; d++) { const double df = (double)__fsub_rn(x[d], ctr[c * D + d]); s = __dadd_rn(s, __dmul_rn(df, df)); }
         const float dist = (float)__dsqrt_rn(s);
         if (c == 0 || dist < best) { best = dist; bi = c; }
      }
      cmap[i] = bi; mn[i] = best;
   }
   __syncthreads();
   if (t <= k) {
      float s = 0.0f; int cnt = 0;
      if (t == k) for (int i = 0; i < n; i++) s = __fadd_rn(s, mn[i]);
      else for (int i = 0; i < n; i++) if (cmap[i] == t) { s = __fadd_rn(s, mn[i]); cnt++; }
      if (t == k) *sNew = s; else { ave[t] = s; csize[t] = cnt; }
   }
   __syncthreads();
   if (t == 0) {
      int ce = 0;
      for (int c = 0; c < k; c++) {
         if (csize[c] < FC_MIN_CLUST) { ce = c + 1; break; }
         ave[c] = __fdiv_rn(ave[c], (float)csize[c]);
      }
      *sCe = ce;
   }
   __syncthreads();
}

__global__ __launch_bounds__(HI_THREADS) void k_flat_cluster(FcArgs a)
{
   extern __shared__ float fcLds[];
   __shared__ int sCe, sPick;
   __shared__ float sNew;
   const int p = blockIdx.x, t = threadIdx.x, D = a.D;
   const int i0 = a.poolOff[p], n = a.poolOff[p + 1] - i0, nc = a.nc[p], c0 = a.cOff[p];
   if (n < nc) { if (t == 0) a.status[p] = HTKAMD_HINIT_ECLUSTER; return; }       // InitClustering :720
   float *ctr = fcLds, *ave = fcLds + (size_t)nc * D;
   int *csize = (int *)(ave + nc);
   const int *item = a.items + i0;
   int *cmap = a.assign + i0;
   float *mn = a.cost + i0;
   for (int i = t; i < n; i += HI_THREADS) cmap[i] = 0;
   if (t == 0) { csize[0] = n; ave[0] = 1.0f; }
   __syncthreads();
   fc_centres(a, 1, n, item, cmap, ctr, csize);
   bool fail = false;
   for (int c = 2; c <= nc && !fail; c++) {
      if (t == 0) {                                      // BiggestCluster over the c-1 clusters there are
         float mx = ave[0]; int big = 0;
         for (int k = 1; k < c - 1; k++) if (ave[k] > mx) { mx = ave[k]; if (csize[k] >= FC_MIN_CLUST) big = k; }
         sPick = big;
      }
      __syncthreads();
      fc_perturb(D, ctr, sPick, c - 1);
      float old = 1.0e10f;
      for (int it = 0;; it++) {
         int repair = 0;
         fc_allocate(a, c, n, item, cmap, mn, ctr, ave, csize, &sCe, &sNew);
         int ce = sCe;
         while (ce != 0) {                               // fill a cluster that came out too small by splitting the fullest
            if (++repair > c) break;
            if (t == 0) {
               int mx = csize[0], full = 0;
               for (int k = 0; k < c; k++) if (csize[k] > mx) { mx = csize[k]; full = k; }
               sPick = full;
            }
            __syncthreads();
            fc_perturb(D, ctr, sPick, ce - 1);
            fc_allocate(a, c, n, item, cmap, mn, ctr, ave, csize, &sCe, &sNew);
            ce = sCe;
         }
         if (ce != 0) { fail = true; break; }            // "Failed to make %d clusters"
         const float nw = sNew;
         const bool conv = it >= FC_MAX_ITER || (double)__fdiv_rn(__fsub_rn(old, nw), old) < 0.001;
         fc_centres(a, c, n, item, cmap, ctr, csize);
         old = nw;
         if (conv) break;
      }
   }
   if (fail) { if (t == 0) a.status[p] = HTKAMD_HINIT_ECLUSTER; return; }
   for (int e = t; e < nc * D; e += HI_THREADS) {        // FindCovariance, DIAGC
      const int c = e / D, d = e - c * D;
      const float mu = ctr[e];
      double s = 0.0;
      for (int i = 0; i < n; i++) if (cmap[i] == c) { const double df = (double)__fsub_rn(a.X[(size_t)item[i] * D + d], mu); s = __dadd_rn(s, __dmul_rn(df, df)); }
      const float v = (float)__ddiv_rn(s, (double)csize[c]);
      a.centre[(size_t)c0 * D + e] = mu;
      a.var[(size_t)c0 * D + e] = v < a.minVar ? a.minVar : v;
   }
   for (int c = t; c < nc; c += HI_THREADS) a.size[c0 + c] = csize[c];
   if (t == 0) a.status[p] = HTKAMD_HINIT_OK;
}

DEVBUF_OWNER("hinit")

static size_t fc_lds_bytes(int nc, int D) { return sizeof(float) * (size_t)nc * D + (sizeof(float) + sizeof(int)) * (size_t)nc; }

extern "C" int htkamd_flat_cluster(const float *dX, int nRows, int D, int nPools, const int *poolOff, const int *items, const int *nc, float minVar,
                                   int *size, float *centre, float *var, int *assign, int *status, void *stream)
{
   if (!dX || nRows < 1 || D < 1 || nPools < 1 || !poolOff || !items || !nc || !size || !centre || !var || !assign || !status) { htkamd_set_error("flat_cluster: bad argument"); return HTKAMD_EINVAL; }
   if (poolOff[0] != 0) { htkamd_set_error("flat_cluster: the first pool starts at item %d", poolOff[0]); return HTKAMD_EINVAL; }
   std::vector<int> cOff((size_t)nPools + 1, 0);
   int maxNc = 1;
   for (int p = 0; p < nPools; p++) {
      if (poolOff[p + 1] < poolOff[p]) { htkamd_set_error("flat_cluster: pool %d has a negative size", p); return HTKAMD_EINVAL; }
      if (nc[p] < 1 || nc[p] > FC_MAX_NC) { htkamd_set_error("flat_cluster: pool %d asks for %d clusters (1 .. %d)", p, nc[p], FC_MAX_NC); return HTKAMD_EINVAL; }
      if (fc_lds_bytes(nc[p], D) > FC_MAX_LDS) { htkamd_set_error("flat_cluster: pool %d: %d centres of %d values do not fit the workgroup's LDS", p, nc[p], D); return HTKAMD_EINVAL; }
      cOff[p + 1] = cOff[p] + nc[p];
      if (nc[p] > maxNc) maxNc = nc[p];
   }
   const int nItems = poolOff[nPools], nClust = cOff[nPools];
   for (int i = 0; i < nItems; i++)
      if (items[i] < 0 || items[i] >= nRows) { htkamd_set_error("flat_cluster: item %d is row %d of %d", i, items[i], nRows); return HTKAMD_EINVAL; }
   if (htkamd_device_count() <= 0) { htkamd_set_error("flat_cluster: no HIP device"); return HTKAMD_ENODEV; }
   hipStream_t s = (hipStream_t)stream;
   DevBuf dOff, dItems, dNc, dCOff, dSize, dCtr, dVar, dAssign, dCost, dStatus;
   int rc;
   const size_t nI = (size_t)nItems, nCD = (size_t)nClust * D;
   if ((rc = dOff.upload(poolOff, (size_t)nPools + 1, s)) || (rc = dItems.upload(items, nI, s)) || (rc = dNc.upload(nc, (size_t)nPools, s)) ||
       (rc = dCOff.upload(cOff, s)) || (rc = dSize.reserve<int>((size_t)nClust)) || (rc = dCtr.reserve<float>(nCD)) || (rc = dVar.reserve<float>(nCD)) ||
       (rc = dAssign.reserve<int>(nI)) || (rc = dCost.reserve<float>(nI)) || (rc = dStatus.reserve<int>((size_t)nPools)))
      return rc;
   HIPCHECK(hipMemsetAsync(dSize.p, 0, sizeof(int) * (size_t)nClust, s));
   HIPCHECK(hipMemsetAsync(dCtr.p, 0, sizeof(float) * nCD, s));
   HIPCHECK(hipMemsetAsync(dVar.p, 0, sizeof(float) * nCD, s));
   HIPCHECK(hipMemsetAsync(dAssign.p, 0, sizeof(int) * (nI ? nI : 1), s));
   FcArgs a;
   a.X = dX; a.D = D; a.poolOff = dOff.as<const int>(); a.items = dItems.as<const int>(); a.nc = dNc.as<const int>(); a.cOff = dCOff.as<const int>();
   a.minVar = minVar; a.size = dSize.as<int>(); a.centre = dCtr.as<float>(); a.var = dVar.as<float>(); a.assign = dAssign.as<int>(); a.cost = dCost.as<float>();
   a.status = dStatus.as<int>();
   hipLaunchKernelGGL(k_flat_cluster, dim3((unsigned)nPools), dim3(HI_THREADS), fc_lds_bytes(maxNc, D), s, a);
   HIPCHECK(hipGetLastError());
   if ((rc = dSize.download(size, (size_t)nClust, s)) || (rc = dCtr.download(centre, nCD, s)) || (rc = dVar.download(var, nCD, s)) ||
       (rc = dAssign.download(assign, nI, s)) || (rc = dStatus.download(status, (size_t)nPools, s)))
      return rc;
   HIPCHECK(hipStreamSynchronize(s));
   return HTKAMD_OK;
}

// ------------------------------------------------------------------------------------------ HInit: tables
struct HiArgs {
   UnitParams p;                                           // the model's arrays and their snapshot
   int uFlags;
   float minVar;
   // the call's
   const float *X;
   const UnitModel *mdl; int nMdl, maxNe;
   const int *tokFrame, *tokLen, *tokMdl; int nTok;
   int *tokCnt, *tokPos;                                   // [nTok][maxNe]
   const int *poolMdl, *poolState; int nPools;
   int *poolSize, *poolOff, *items;
   int *mstatus;                                           // [nMdl]
   // a pass's
   float *Xg;                                              // the running tokens' rows behind one another
   const int *uMdl, *uFrame0, *uSrc, *uSeg0; int nUtt, nFrames;      // uFrame0 [nUtt+1]
   const int *segUtt, *segJ; int nSeg;
   const int *segStart, *segEnd; const double *total; const int *uttStatus;
   const int *runMdl, *runUtt0; int nRun;                  // runUtt0 [nRun+1]
   const int *updFlag;                                     // [nMdl]
   const int *updList; int nUpd;
   int *frameComp;
   double *accMu, *accVa; int *accCnt, *trCnt, *occCnt;
   float *logpOut; int *statOut;                           // [nRun]
};

__global__ void k_hi_count(HiArgs a)
{
   const int k = blockIdx.x * blockDim.x + threadIdx.x;
   if (k >= a.nTok) return;
   const int ne = a.mdl[a.tokMdl[k]].ne, L = a.tokLen[k];
   int *cnt = a.tokCnt + (size_t)k * a.maxNe;
   for (int s = 0; s < ne; s++) cnt[s] = 0;
   for (int j = 0; j < L; j++) cnt[htkamd_hinit_state_of(j, L, ne)]++;
}

__global__ __launch_bounds__(HI_THREADS) void k_hi_scan(HiArgs a)
{
   __shared__ int lds[HI_THREADS];
   const int p = blockIdx.x, s = a.poolState[p];
   const UnitModel m = a.mdl[a.poolMdl[p]];
   int base = 0;
   for (int k0 = 0; k0 < m.nTok; k0 += HI_THREADS) {
      const int k = k0 + threadIdx.x;
      const int v = k < m.nTok ? a.tokCnt[(size_t)(m.tok0 + k) * a.maxNe + s] : 0;
      int tot;
      const int ex = unit_block_excl_scan<HI_THREADS>(v, lds, &tot);
      if (k < m.nTok) a.tokPos[(size_t)(m.tok0 + k) * a.maxNe + s] = base + ex;
      base += tot;
   }
   if (threadIdx.x == 0) a.poolSize[p] = base;
}

__global__ __launch_bounds__(HI_THREADS) void k_hi_pooloff(HiArgs a)
{
   __shared__ int lds[HI_THREADS];
   int base = 0;
   for (int p0 = 0; p0 < a.nPools; p0 += HI_THREADS) {
      const int p = p0 + threadIdx.x;
      const int v = p < a.nPools ? a.poolSize[p] : 0;
      int tot;
      const int ex = unit_block_excl_scan<HI_THREADS>(v, lds, &tot);
      if (p < a.nPools) a.poolOff[p] = base + ex;
      base += tot;
   }
   if (threadIdx.x == 0) a.poolOff[a.nPools] = base;
}

__global__ void k_hi_fill(HiArgs a)
{
   const int k = blockIdx.x * blockDim.x + threadIdx.x;
   if (k >= a.nTok) return;
   const UnitModel m = a.mdl[a.tokMdl[k]];
   const int L = a.tokLen[k], f0 = a.tokFrame[k];
   const int *pos = a.tokPos + (size_t)k * a.maxNe;
   int prev = -1, run = 0;
   for (int j = 0; j < L; j++) {
      const int s = htkamd_hinit_state_of(j, L, m.ne);
      if (s != prev) { prev = s; run = 0; }
      a.items[a.poolOff[m.pool0 + s] + pos[s] + run++] = f0 + j;
   }
}

struct FcOut { const int *size; const float *centre, *var; const int *status, *cOff; };

__global__ __launch_bounds__(HI_THREADS) void k_hi_init(HiArgs a, FcOut f)
{
   const UnitModel m = a.mdl[blockIdx.x];
   const int D = a.p.g.D, t = threadIdx.x;
   bool fail = false;
   for (int s = 0; s < m.ne; s++) if (f.status[m.pool0 + s] != HTKAMD_HINIT_OK) fail = true;
   if (fail) { if (t == 0) a.mstatus[blockIdx.x] = HTKAMD_HINIT_ECLUSTER; return; }
   for (int s = 0; s < m.ne; s++) {
      const int p = m.pool0 + s, st = a.p.hmmState[m.st0 + s], c0 = a.p.g.stateCompOff[st], M = a.p.g.stateCompOff[st + 1] - c0, k0 = f.cOff[p];
      const int n = a.poolOff[p + 1] - a.poolOff[p];
      for (int e = t; e < M * D; e += HI_THREADS) {
         const int k = e / D, d = e - k * D, g = a.p.g.compGauss[c0 + k];
         if (a.uFlags & HTKAMD_UPMEANS) a.p.mean[(size_t)g * D + d] = f.centre[(size_t)k0 * D + e];
         if (a.uFlags & HTKAMD_UPVARS) a.p.var[(size_t)g * D + d] = f.var[(size_t)k0 * D + e];
      }
      if (a.uFlags & HTKAMD_UPMIXES) for (int k = t; k < M; k += HI_THREADS) a.p.compWeight[c0 + k] = __fdiv_rn((float)f.size[k0 + k], (float)n);
   }
   __syncthreads();
   for (int s = 0; s < m.ne; s++) htkamd_derive_state(a.p.g, a.p.hmmState[m.st0 + s], HI_THREADS);
}

// ------------------------------------------------------------------------------------------ HInit: a pass
__global__ __launch_bounds__(HI_THREADS) void k_hi_gather(HiArgs a)
{
   const int u = blockIdx.x, D = a.p.g.D;
   unit_gather_rows<HI_THREADS>(a.Xg + (size_t)a.uFrame0[u] * D, a.X + (size_t)a.uSrc[u] * D, (size_t)(a.uFrame0[u + 1] - a.uFrame0[u]) * D);
}

__global__ void k_hi_logp(HiArgs a)
{
   const int q = blockIdx.x * blockDim.x + threadIdx.x;
   if (q >= a.nRun) return;
   float s = 0.0f; int bad = 0;
   for (int u = a.runUtt0[q]; u < a.runUtt0[q + 1]; u++) {
      if (a.uttStatus[u] != HTKAMD_UTT_OK) bad = 1;
      s = __fadd_rn(s, (float)a.total[u]);
   }
   int ms = a.mstatus[a.runMdl[q]];
   if (!ms && bad) { ms = HTKAMD_HINIT_ENOPATH; a.mstatus[a.runMdl[q]] = ms; }      // (this lane alone writes the model's status now)
   a.logpOut[q] = s;
   a.statOut[q] = ms;
}

// FindBestMixes: the component of the aligned state with the first maximum of MOutP (DOutP's form, HModel.c:5347)
__global__ void k_hi_best(HiArgs a)
{
   const int f = blockIdx.x * blockDim.x + threadIdx.x;
   if (f >= a.nFrames) return;
   int lo = 0, hi = a.nUtt - 1;
   while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (a.uFrame0[mid] <= f) lo = mid; else hi = mid - 1; }
   const int u = lo, r = a.uMdl[u];
   if (!a.updFlag[r]) return;
   const UnitModel m = a.mdl[r];
   const int tl = f - a.uFrame0[u], D = a.p.g.D;
   int j = -1;
   for (int s = 0; s < m.ne; s++) { const int st = a.segStart[a.uSeg0[u] + s]; if (st >= 0 && st <= tl && tl < a.segEnd[a.uSeg0[u] + s]) j = s; }
   int comp = -1;
   if (j >= 0) {
      const int st = a.p.hmmState[m.st0 + j], c0 = a.p.g.stateCompOff[st], M = a.p.g.stateCompOff[st + 1] - c0;
      if (M == 1) comp = c0;
      else {
         const float *x = a.Xg + (size_t)f * D;
         float bestP = (float)LZERO; int best = -1;
         for (int k = 0; k < M; k++) {
            const int g = a.p.g.compGauss[c0 + k];
            const float *mu = a.p.mean + (size_t)g * D, *va = a.p.var + (size_t)g * D;
            float sum = a.p.g.gconst[g];
            for (int d = 0; d < D; d++) { const float xmm = __fsub_rn(x[d], mu[d]); sum = __fadd_rn(sum, __fdiv_rn(__fmul_rn(xmm, xmm), va[d])); }
            const float pr = __fmul_rn(-0.5f, sum);
            if (pr > bestP) { bestP = pr; best = k; }
         }
         if (best >= 0) comp = c0 + best;
      }
   }
   if (comp < 0) atomicCAS(a.mstatus + r, HTKAMD_HINIT_OK, j < 0 ? HTKAMD_HINIT_ENOPATH : HTKAMD_HINIT_ENOMIX);
   a.frameComp[f] = comp;
}

// UpdateCounts: a wavefront per (token, state) segment, lanes are dimensions
__global__ __launch_bounds__(HI_THREADS) void k_hi_acc(HiArgs a)
{
   const int w = blockIdx.x * (HI_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
   if (w >= a.nSeg) return;
   const int u = a.segUtt[w], j = a.segJ[w], r = a.uMdl[u];
   if (!a.updFlag[r]) return;
   const UnitModel m = a.mdl[r];
   const int D = a.p.g.D, st = a.segStart[w], en = a.segEnd[w], f0 = a.uFrame0[u];
   if (st >= 0 && (a.uFlags & (HTKAMD_UPMEANS | HTKAMD_UPVARS | HTKAMD_UPMIXES)))
      for (int d0 = 0; d0 < D; d0 += 64) {
         const int d = d0 + lane;
         int cur = -1, g = 0, run = 0;
         float mu = 0.0f;
         double sm = 0.0, sv = 0.0;
         for (int f = f0 + st; f <= f0 + en; f++) {
            const int c = f < f0 + en ? a.frameComp[f] : -2;       // the last turn only flushes
            if (c != cur) {
               if (cur >= 0 && run > 0) {
                  if (d < D) { atomicAdd(a.accMu + (size_t)g * D + d, sm); atomicAdd(a.accVa + (size_t)g * D + d, sv); }
                  if (d == 0) atomicAdd(a.accCnt + cur, run);
               }
               cur = c; run = 0; sm = 0.0; sv = 0.0;
               if (c >= 0) { g = a.p.g.compGauss[c]; mu = d < D ? a.p.mean[(size_t)g * D + d] : 0.0f; }
            }
            if (c >= 0) {
               if (d < D) { const double x = (double)__fsub_rn(a.Xg[(size_t)f * D + d], mu); sm += x; sv += x * x; }
               run++;
            }
         }
      }
   if (j == 0 && lane == 0 && (a.uFlags & HTKAMD_UPTRANS)) {       // the token's state sequence: entry = 1, exit = N
      int last = 1;
      for (int s = 0; s < m.ne; s++) {
         const int s0 = a.segStart[w + s], s1 = a.segEnd[w + s];
         if (s0 < 0) continue;
         const int n = s1 - s0, i = s + 2;
         atomicAdd(a.occCnt + m.occ0 + last - 1, 1); atomicAdd(a.trCnt + m.tp0 + (last - 1) * m.N + (i - 1), 1);
         if (n > 1) { atomicAdd(a.occCnt + m.occ0 + i - 1, n - 1); atomicAdd(a.trCnt + m.tp0 + (i - 1) * m.N + (i - 1), n - 1); }
         last = i;
      }
      atomicAdd(a.occCnt + m.occ0 + last - 1, 1); atomicAdd(a.trCnt + m.tp0 + (last - 1) * m.N + (m.N - 1), 1);
   }
}

// UpdateParameters: a workgroup per model
__global__ __launch_bounds__(HI_THREADS) void k_hi_update(HiArgs a)
{
   const int r = a.updList[blockIdx.x], t = threadIdx.x, D = a.p.g.D;
   const UnitModel m = a.mdl[r];
   bool fail = a.mstatus[r] != HTKAMD_HINIT_OK;
   for (int s = 0; s < m.ne && !fail; s++) {
      const int st = a.p.hmmState[m.st0 + s], c0 = a.p.g.stateCompOff[st], M = a.p.g.stateCompOff[st + 1] - c0;
      int tot = 0;
      for (int k = 0; k < M; k++) {
         const int n = a.accCnt[c0 + k];
         tot += n;
         if (n == 0 && (a.uFlags & (HTKAMD_UPMEANS | HTKAMD_UPVARS))) fail = true;      // UpMeans / UpVars: zero occ
      }
      if (tot == 0 && M > 1 && (a.uFlags & HTKAMD_UPMIXES)) fail = true;                   // UpWeights: zero occ
   }
   if (a.uFlags & HTKAMD_UPTRANS) for (int i = 1; i < m.N && !fail; i++) if (a.occCnt[m.occ0 + i - 1] == 0) fail = true;     // UpTrans: zero occ
   if (fail) { if (t == 0) atomicCAS(a.mstatus + r, HTKAMD_HINIT_OK, HTKAMD_HINIT_EZEROOCC); return; }
   for (int s = 0; s < m.ne; s++) {
      const int st = a.p.hmmState[m.st0 + s], c0 = a.p.g.stateCompOff[st], M = a.p.g.stateCompOff[st + 1] - c0;
      if (a.uFlags & (HTKAMD_UPMEANS | HTKAMD_UPVARS))
         for (int e = t; e < M * D; e += HI_THREADS) {
            const int k = e / D, d = e - k * D, g = a.p.g.compGauss[c0 + k];
            const double occ = (double)a.accCnt[c0 + k], old = (double)a.p.mean[(size_t)g * D + d];
            const double nm = old + a.accMu[(size_t)g * D + d] / occ;
            const double x = (a.uFlags & HTKAMD_UPMEANS) ? nm - old : 0.0;
            if (a.uFlags & HTKAMD_UPVARS) {
               const float z = (float)(a.accVa[(size_t)g * D + d] / occ - x * x);
               a.p.var[(size_t)g * D + d] = z < a.minVar ? a.minVar : z;
            }
            if (a.uFlags & HTKAMD_UPMEANS) a.p.mean[(size_t)g * D + d] = (float)nm;
         }
      if (M > 1 && (a.uFlags & HTKAMD_UPMIXES)) {
         int tot = 0;
         for (int k = 0; k < M; k++) tot += a.accCnt[c0 + k];
         for (int k = t; k < M; k += HI_THREADS) a.p.compWeight[c0 + k] = __fdiv_rn((float)a.accCnt[c0 + k], (float)tot);
      }
   }
   if ((a.uFlags & HTKAMD_UPTRANS) && t >= 1 && t < m.N) {             // UpTrans: row t from the integer counts
      const int *cnt = a.trCnt + m.tp0 + (t - 1) * m.N;
      unit_trans_row(a.p.transP + m.tp0 + (t - 1) * m.N, m.N, [cnt](int j) { return (float)cnt[j]; }, (float)a.occCnt[m.occ0 + t - 1]);
   }
   __syncthreads();
   for (int s = 0; s < m.ne; s++) htkamd_derive_state(a.p.g, a.p.hmmState[m.st0 + s], HI_THREADS);
}

// ------------------------------------------------------------------------------------------ HInit: the call
extern "C" int htkamd_hinit(htkamd_model *m, const float *dX, int nFrames, int nTokens, const int *tokFrame, const int *tokLen, const int *tokModel,
                            const htkamd_hinit_config *cfg, int nModels, const int *models,
                            int *status, int *nPass, int *converged, float *logP, void *stream)
{
   if (!m || !cfg || !status || !nPass || !converged || !logP) { htkamd_set_error("hinit: NULL argument"); return HTKAMD_EINVAL; }
   int rc;
   htkamd_model_desc d;
   if ((rc = unit_refuse_handle(m, "hinit", "HInit", &d)) || (rc = htkamd_hinit_check(&d, nFrames, nTokens, tokFrame, tokLen, tokModel, cfg, nModels, models))) return rc;
   if (!dX && nTokens > 0) { htkamd_set_error("hinit: no feature table"); return HTKAMD_EINVAL; }
   if (htkamd_device_count() <= 0) { htkamd_set_error("hinit: no HIP device"); return HTKAMD_ENODEV; }
   hipStream_t s = (hipStream_t)stream;
   const int D = m->D, maxIter = cfg->maxIter;
   for (int k = 0; k < nModels; k++) { status[k] = HTKAMD_HINIT_OK; nPass[k] = 0; converged[k] = 0; }
   for (size_t i = 0; i < (size_t)nModels * maxIter; i++) logP[i] = 0.0f;

   // ---- the models that can be trained, their tokens behind one another (the given order within a model), their pools
   UnitTables tb;
   std::vector<int> poolMdl, poolState, poolNc, cOff(1, 0);
   int maxNe = 1, maxNc = 1;
   rc = unit_tables("hinit", m, nTokens, tokFrame, tokLen, tokModel, nullptr, nModels, models,
      [&](int k, int ne, const std::vector<int> &toks) {                   // main :276 (-m), UCollectData :516
         if ((int)toks.size() < cfg->minSeg) { status[k] = HTKAMD_HINIT_EFEWSEGS; return false; }
         bool tooShort = false;
         for (int t : toks) if (tokLen[t] < ne) tooShort = true;
         if (tooShort || ne < 1) { status[k] = HTKAMD_HINIT_ESHORT; return false; }
         return true;
      },
      [&](UnitModel &x, int r) -> int {                                    // a pool per emitting state
         x.pool0 = (int)poolMdl.size();
         for (int j = 0; j < x.ne; j++) {
            const int st = m->h_hmmState[x.st0 + j], M = m->h_stateCompOff[st + 1] - m->h_stateCompOff[st];
            if (M > FC_MAX_NC || fc_lds_bytes(M, D) > FC_MAX_LDS) { htkamd_set_error("hinit: state %d of model %d has %d components of %d values: more than a workgroup clusters", j + 2, x.h, M, D); return HTKAMD_EMODEL; }
            poolMdl.push_back(r); poolState.push_back(j); poolNc.push_back(M); cOff.push_back(cOff.back() + M);
            if (M > maxNc) maxNc = M;
         }
         if (x.ne > maxNe) maxNe = x.ne;
         return HTKAMD_OK;
      }, tb);
   if (rc || tb.mdl.empty()) return rc;
   const std::vector<UnitModel> &mdl = tb.mdl;
   const std::vector<int> &mdlOf = tb.mdlOf, &aFrame = tb.aFrame, &aLen = tb.aLen;
   const long long totFrames = tb.totFrames;
   const int nMdl = (int)mdl.size(), nTok = (int)aFrame.size(), nPools = (int)poolMdl.size(), nClust = cOff.back();

   htkamd_viterbi *vit = nullptr;
   if ((rc = htkamd_viterbi_create(m, &vit))) return rc;
   struct VitGuard { htkamd_viterbi *v; ~VitGuard() { htkamd_viterbi_destroy(v); } } guard{vit};

   DevBuf bMdl, bTokFrame, bTokLen, bTokMdl, bTokCnt, bTokPos, bPoolMdl, bPoolState, bPoolNc, bCOff, bPoolSize, bPoolOff, bItems, bMstatus;
   DevBuf bFcSize, bFcCtr, bFcVar, bFcAssign, bFcCost, bFcStatus, bBak, bXg, bUtt, bSeg, bRun, bUpd, bFrameComp, bAcc, bOut;
   const size_t nGD = (size_t)m->G * D, nTp = (size_t)m->h_transOff[m->nT], nOcc = (size_t)m->h_trOccOff[m->nT];
   const size_t nF = (size_t)totFrames, nCD = (size_t)nClust * D, accBytes = sizeof(double) * 2 * nGD + sizeof(int) * ((size_t)m->C + nTp + nOcc);
   if ((rc = bMdl.upload(mdl, s)) || (rc = bTokFrame.upload(aFrame, s)) || (rc = bTokLen.upload(aLen, s)) || (rc = bTokMdl.upload(tb.aMdl, s)) ||
       (rc = bPoolMdl.upload(poolMdl, s)) || (rc = bPoolState.upload(poolState, s)) || (rc = bPoolNc.upload(poolNc, s)) || (rc = bCOff.upload(cOff, s)) ||
       (rc = bTokCnt.reserve<int>((size_t)nTok * maxNe)) || (rc = bTokPos.reserve<int>((size_t)nTok * maxNe)) ||
       (rc = bPoolSize.reserve<int>((size_t)nPools)) || (rc = bPoolOff.reserve<int>((size_t)nPools + 1)) ||
       (rc = bItems.reserve<int>(nF)) || (rc = bMstatus.reserve<int>((size_t)nMdl)) || (rc = bXg.reserve<float>(nF * D)) || (rc = bFrameComp.reserve<int>(nF)) ||
       (rc = bAcc.reserve(accBytes)) || (rc = bOut.reserve<float>(2 * (size_t)nMdl)))      // (bOut: a float and an int per model)
      return rc;
   HIPCHECK(hipMemsetAsync(bMstatus.p, 0, sizeof(int) * (size_t)nMdl, s));
   HiArgs a;
   memset(&a, 0, sizeof(a));
   if ((rc = unit_snapshot(m, bBak, s, &a.p))) return rc;
   a.uFlags = cfg->uFlags; a.minVar = cfg->minVar;
   a.X = dX; a.mdl = bMdl.as<const UnitModel>(); a.nMdl = nMdl; a.maxNe = maxNe;
   a.tokFrame = bTokFrame.as<const int>(); a.tokLen = bTokLen.as<const int>(); a.tokMdl = bTokMdl.as<const int>(); a.nTok = nTok;
   a.tokCnt = bTokCnt.as<int>(); a.tokPos = bTokPos.as<int>(); a.poolMdl = bPoolMdl.as<const int>(); a.poolState = bPoolState.as<const int>(); a.nPools = nPools;
   a.poolSize = bPoolSize.as<int>(); a.poolOff = bPoolOff.as<int>(); a.items = bItems.as<int>(); a.mstatus = bMstatus.as<int>();
   a.Xg = bXg.as<float>(); a.frameComp = bFrameComp.as<int>();
   a.accMu = bAcc.as<double>(); a.accVa = a.accMu + nGD; a.accCnt = (int *)(a.accVa + nGD); a.trCnt = a.accCnt + m->C; a.occCnt = a.trCnt + nTp;
   a.logpOut = bOut.as<float>(); a.statOut = bOut.as<int>() + nMdl;
   const unsigned tokBlocks = (unsigned)((nTok + HI_THREADS - 1) / HI_THREADS);
   std::vector<int> mstat((size_t)nMdl, 0);

   auto train = [&]() -> int {
      // ---- UniformSegment: pools, FlatCluster, the first parameters
      if (cfg->newModel) {
         if ((rc = bFcSize.reserve<int>((size_t)nClust)) || (rc = bFcCtr.reserve<float>(nCD)) || (rc = bFcVar.reserve<float>(nCD)) ||
             (rc = bFcAssign.reserve<int>(nF)) || (rc = bFcCost.reserve<float>(nF)) || (rc = bFcStatus.reserve<int>((size_t)nPools)))
            return rc;
         hipLaunchKernelGGL(k_hi_count, dim3(tokBlocks), dim3(HI_THREADS), 0, s, a);
         hipLaunchKernelGGL(k_hi_scan, dim3((unsigned)nPools), dim3(HI_THREADS), 0, s, a);
         hipLaunchKernelGGL(k_hi_pooloff, dim3(1), dim3(HI_THREADS), 0, s, a);
         hipLaunchKernelGGL(k_hi_fill, dim3(tokBlocks), dim3(HI_THREADS), 0, s, a);
         HIPCHECK(hipGetLastError());
         FcArgs f;
         f.X = dX; f.D = D; f.poolOff = a.poolOff; f.items = a.items; f.nc = bPoolNc.as<const int>(); f.cOff = bCOff.as<const int>();
         // UniformSegment floors with vFloor (:592) where it copies, and only under UPVARS
         f.minVar = cfg->minVar; f.size = bFcSize.as<int>(); f.centre = bFcCtr.as<float>(); f.var = bFcVar.as<float>(); f.assign = bFcAssign.as<int>();
         f.cost = bFcCost.as<float>(); f.status = bFcStatus.as<int>();
         hipLaunchKernelGGL(k_flat_cluster, dim3((unsigned)nPools), dim3(HI_THREADS), fc_lds_bytes(maxNc, D), s, f);
         HIPCHECK(hipGetLastError());
         FcOut fo;
         fo.size = f.size; fo.centre = f.centre; fo.var = f.var; fo.status = f.status; fo.cOff = f.cOff;
         hipLaunchKernelGGL(k_hi_init, dim3((unsigned)nMdl), dim3(HI_THREADS), 0, s, a, fo);
         HIPCHECK(hipGetLastError());
         if ((rc = bMstatus.download(mstat.data(), mstat.size(), s))) return rc;
         HIPCHECK(hipStreamSynchronize(s));
      }

      // ---- EstimateModel's passes
      std::vector<int> running, iter((size_t)nMdl, 0);
      std::vector<float> totalP((size_t)nMdl, (float)LZERO);
      for (int r = 0; r < nMdl; r++) { if (mstat[r]) status[mdlOf[r]] = mstat[r]; else running.push_back(r); }
      bool changed = true;
      std::vector<int> uMdl, uFrame0, uSrc, uSeg0, segUtt, segJ, labs, labOff, runUtt0, updFlag((size_t)nMdl), updList;
      std::vector<float> outHost;
      while (!running.empty()) {
         if (changed) {                                      // the batch of the models still running
            uMdl.clear(); uFrame0.assign(1, 0); uSrc.clear(); uSeg0.clear(); segUtt.clear(); segJ.clear(); labs.clear(); runUtt0.assign(1, 0);
            for (int r : running) {
               const UnitModel &x = mdl[r];
               for (int k = x.tok0; k < x.tok0 + x.nTok; k++) {
                  const int u = (int)uMdl.size();
                  uMdl.push_back(r); uSrc.push_back(aFrame[k]); uSeg0.push_back((int)segUtt.size()); uFrame0.push_back(uFrame0.back() + aLen[k]); labs.push_back(x.h);
                  for (int j = 0; j < x.ne; j++) { segUtt.push_back(u); segJ.push_back(j); }
               }
               runUtt0.push_back((int)uMdl.size());
            }
            labOff.resize(uMdl.size() + 1);
            for (size_t u = 0; u <= uMdl.size(); u++) labOff[u] = (int)u;
            const size_t nU = uMdl.size();
            std::vector<int> pack;                          // one upload: uMdl, uFrame0, uSrc, uSeg0 | segUtt, segJ | running, runUtt0
            pack.insert(pack.end(), uMdl.begin(), uMdl.end()); pack.insert(pack.end(), uFrame0.begin(), uFrame0.end());
            pack.insert(pack.end(), uSrc.begin(), uSrc.end()); pack.insert(pack.end(), uSeg0.begin(), uSeg0.end());
            if ((rc = bUtt.upload(pack, s))) return rc;
            a.uMdl = bUtt.as<const int>(); a.uFrame0 = a.uMdl + nU; a.uSrc = a.uFrame0 + nU + 1; a.uSeg0 = a.uSrc + nU;
            a.nUtt = (int)nU; a.nFrames = uFrame0.back();
            pack.assign(segUtt.begin(), segUtt.end()); pack.insert(pack.end(), segJ.begin(), segJ.end());
            if ((rc = bSeg.upload(pack, s))) return rc;
            a.segUtt = bSeg.as<const int>(); a.segJ = a.segUtt + segUtt.size(); a.nSeg = (int)segUtt.size();
            pack.assign(running.begin(), running.end()); pack.insert(pack.end(), runUtt0.begin(), runUtt0.end());
            if ((rc = bRun.upload(pack, s))) return rc;
            a.runMdl = bRun.as<const int>(); a.runUtt0 = a.runMdl + running.size(); a.nRun = (int)running.size();
            hipLaunchKernelGGL(k_hi_gather, dim3((unsigned)nU), dim3(HI_THREADS), 0, s, a);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipStreamSynchronize(s));              // (pack goes)
            changed = false;
         }
         htkamd_batch_desc b;
         b.nUtt = a.nUtt; b.dX = a.Xg; b.frameOff = uFrame0.data(); b.labOff = labOff.data(); b.labs = labs.data();
         if ((rc = htkamd_viterbi_align_mode(vit, &b, 1.0e10f, HTKAMD_SCORE_SOUTP | HTKAMD_SCORE_DIAGC, s))) return rc;
         htkamd_viterbi_dev vr;
         if ((rc = htkamd_viterbi_device_results(vit, &vr))) return rc;
         a.segStart = vr.segStart; a.segEnd = vr.segEnd; a.total = vr.total; a.uttStatus = vr.status;
         hipLaunchKernelGGL(k_hi_logp, dim3((unsigned)((a.nRun + 63) / 64)), dim3(64), 0, s, a);
         HIPCHECK(hipGetLastError());
         outHost.resize(2 * (size_t)nMdl);
         if ((rc = bOut.download(outHost.data(), outHost.size(), s))) return rc;
         HIPCHECK(hipStreamSynchronize(s));
         const int *statHost = (const int *)(outHost.data() + nMdl);
         std::vector<int> next;
         updList.clear();
         std::fill(updFlag.begin(), updFlag.end(), 0);
         for (size_t q = 0; q < running.size(); q++) {
            const int r = running[q], k = mdlOf[r];
            if (statHost[q] != HTKAMD_HINIT_OK) { status[k] = statHost[q]; mstat[r] = statHost[q]; changed = true; continue; }
            const int it = ++iter[r];
            const float newP = outHost[q] / (float)mdl[r].nTok;
            const float delta = newP - totalP[r];
            const bool conv = it > 1 && fabs((double)delta) < (double)cfg->epsilon;
            logP[(size_t)k * maxIter + it - 1] = newP; nPass[k] = it; totalP[r] = newP;
            if (conv) { converged[k] = 1; changed = true; continue; }
            updList.push_back(r); updFlag[r] = 1;
            if (it < maxIter) next.push_back(r); else changed = true;
         }
         if (!updList.empty()) {
            std::vector<int> pack(updFlag);
            pack.insert(pack.end(), updList.begin(), updList.end());
            if ((rc = bUpd.upload(pack, s))) return rc;
            a.updFlag = bUpd.as<const int>(); a.updList = a.updFlag + nMdl; a.nUpd = (int)updList.size();
            HIPCHECK(hipMemsetAsync(bAcc.p, 0, accBytes, s));
            hipLaunchKernelGGL(k_hi_best, dim3((unsigned)((a.nFrames + HI_THREADS - 1) / HI_THREADS)), dim3(HI_THREADS), 0, s, a);
            hipLaunchKernelGGL(k_hi_acc, dim3((unsigned)((a.nSeg + HI_THREADS / 64 - 1) / (HI_THREADS / 64))), dim3(HI_THREADS), 0, s, a);
            hipLaunchKernelGGL(k_hi_update, dim3((unsigned)a.nUpd), dim3(HI_THREADS), 0, s, a);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipStreamSynchronize(s));              // (pack goes)
         }
         running.swap(next);
      }

      // ---- statuses raised by the last updates; the models that ended with one take back the parameters they came with
      if ((rc = bMstatus.download(mstat.data(), mstat.size(), s))) return rc;
      HIPCHECK(hipStreamSynchronize(s));
      bool anyBad = false;
      for (int r = 0; r < nMdl; r++) if (mstat[r]) { status[mdlOf[r]] = mstat[r]; converged[mdlOf[r]] = 0; anyBad = true; }
      if (anyBad) { hipLaunchKernelGGL(k_unit_restore<HI_THREADS>, dim3((unsigned)nMdl), dim3(HI_THREADS), 0, s, a.p, a.mdl, a.mstatus); HIPCHECK(hipGetLastError()); }
      return HTKAMD_OK;
   };
   const int rcTrain = train();
   if (rcTrain) {
      // a call that ends in an error leaves no model half trained: every model of the call goes back to its snapshot (as far as the
      // device still answers), then the mirror follows as below and the error is returned; status / nPass / logP are then undefined
      hipLaunchKernelGGL(k_unit_restore<HI_THREADS>, dim3((unsigned)nMdl), dim3(HI_THREADS), 0, s, a.p, a.mdl, (const int *)nullptr);
      (void)hipGetLastError();
   }
   rc = unit_finish(m, s);                                   // the host mirror and the derived tables follow
   return rcTrain ? rcTrain : rc;
}
