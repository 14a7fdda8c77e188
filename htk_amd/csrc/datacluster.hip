// datacluster.hip -- the device side of data-driven state clustering (HHEd's TC / NC commands; the driver is host/treeclust.c).
//
// Clustering (HHEd.c:2005) is a furthest-neighbour agglomeration over an N x N matrix of state distances.  Three kernels:
//
// k_dc_divergence: thread = one pair (i, j) of a command's items, single-Gaussian DIAGC states.  Divergence (:1749) in the reference's
//   float/double mix, every rounding written out: x = m1 - m2 and x*x in float, v1*v2 in float, widened; double sqrt and divide; the
//   double sum rounded to float at every dimension; sum / V as a float divide, double sqrt, rounded to float.  Nothing is fused.
// k_dc_gdist: the same grid for sets with mixtures, GDistance (:1771): the scores of every component mean under every item come from
//   htkamd_outp_block_mode (SOutP's rounding, DOutP's form: HHEd never calls ConvDiagC before it clusters); the kernel only adds them
//   in the reference's order, s1's means under s2 and then s2's means under s1, as float adds, and returns -(sum / M), M = s2's count.
// k_dc_merge: one workgroup per command, the merge loop and RemOutliers (:1975) on the full symmetric group matrix in memory.
//   Complete linkage: after merging a <- b, g[a][k] = max(g[a][k], g[b][k]); max is exact, so this is SetGDist's (:1818) full
//   recomputation (which also starts every maximum at 0.0: the first merge lifts negative entries to 0).  A slot keeps its place for good: retiring b shifts the reference's later groups down without reordering them, so
//   "first in row-major order over the current numbering" (MinGDist :1869, strict <) is the lexicographic first among the live slots,
//   and a group's current number is one plus the live slots before it.  Every live row i keeps the first minimum over the live
//   columns j > i in LDS (value and column); a merge rescans only row a and the rows whose minimum sat in column a or b -- an entry
//   of column a can only have grown, so every other row's first minimum stands.  RemOutliers' merged group stays in the sparsest
//   group's slot (MergeGroups(sparsest, mini) appends to cvec[sparsest], also when mini < sparsest); no row minima are needed there.
//   Occupation sums are float adds over a group's member chain in chain order (SetOccSums :1924), then sum[a] += sum[b] per merge
//   (UpdateOccSums :1950).  The log holds (i, j) of every merge in the numbering current at that merge, 1-based as in the reference.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "internal.h"
#include "hipcheck.h"
#include "devbuf.h"

#define DC_THREADS 256
#define DC_WAVES   (DC_THREADS / 64)
#define DC_TILE    16

// ------------------------------------------------------------------------------------------ distances
__global__ __launch_bounds__(DC_TILE * DC_TILE) void k_dc_divergence(const float *mean, const float *var, int V, int off, int n, float *dist)
{
   const int i = blockIdx.y * DC_TILE + threadIdx.y, j = blockIdx.x * DC_TILE + threadIdx.x;
   if (i >= n || j >= n || j < i) return;
   if (i == j) { dist[(size_t)i * n + i] = 0.0f; return; }
   const float *m1 = mean + (size_t)(off + i) * V, *m2 = mean + (size_t)(off + j) * V;
   const float *v1 = var + (size_t)(off + i) * V, *v2 = var + (size_t)(off + j) * V;
   float sum = 0.0f;
   for (int k = 0; k < V; k++) {
      const float x = __fsub_rn(m1[k], m2[k]);
      const float xx = __fmul_rn(x, x);
      const float vv = __fmul_rn(v1[k], v2[k]);
      const double q = __ddiv_rn((double)xx, __dsqrt_rn((double)vv));
      sum = (float)__dadd_rn((double)sum, q);
   }
   const float d = (float)__dsqrt_rn((double)__fdiv_rn(sum, (float)V));
   const float x = __fadd_rn(0.0f, d);                  // StateDistance (:1792): x = 0.0; x += Divergence; x / 1
   dist[(size_t)i * n + j] = x; dist[(size_t)j * n + i] = x;
}

// score[slot][obs], slot = item, obs = the component means of the items in item order (obsOff[i] .. obsOff[i+1])
__global__ __launch_bounds__(DC_TILE * DC_TILE) void k_dc_gdist(const float *score, int T, const int *obsOff, int n, float *dist)
{
   const int i = blockIdx.y * DC_TILE + threadIdx.y, j = blockIdx.x * DC_TILE + threadIdx.x;
   if (i >= n || j >= n || j < i) return;
   if (i == j) { dist[(size_t)i * n + i] = 0.0f; return; }
   float sum = 0.0f;
   for (int o = obsOff[i]; o < obsOff[i + 1]; o++) sum = __fadd_rn(sum, score[(size_t)j * T + o]);
   for (int o = obsOff[j]; o < obsOff[j + 1]; o++) sum = __fadd_rn(sum, score[(size_t)i * T + o]);
   const float d = -__fdiv_rn(sum, (float)(obsOff[j + 1] - obsOff[j]));
   const float x = __fadd_rn(0.0f, d);
   dist[(size_t)i * n + j] = x; dist[(size_t)j * n + i] = x;
}

// ------------------------------------------------------------------------------------------ the merge loop
struct DcCmd { long long mat; int off, n, numReq; float threshold; };      // mat: the command's first matrix element; off: its first item

// (value, index): the smaller value, on equal values the smaller index; index -1 = nothing
static __device__ __forceinline__ void dc_take(float &v, int &ix, float ov, int oi)
{
   if (oi >= 0 && (ix < 0 || ov < v || (ov == v && oi < ix))) { v = ov; ix = oi; }
}
static __device__ __forceinline__ void dc_wave_min(float &v, int &ix)
{
#pragma unroll
   for (int d = 32; d >= 1; d >>= 1) { const float ov = __shfl_xor(v, d); const int oi = __shfl_xor(ix, d); dc_take(v, ix, ov, oi); }
}
// the whole block's first minimum; every thread gets it (two barriers)
static __device__ void dc_block_min(float &v, int &ix, float *redV, int *redI)
{
   dc_wave_min(v, ix);
   __syncthreads();
   if ((threadIdx.x & 63) == 0) { redV[threadIdx.x >> 6] = v; redI[threadIdx.x >> 6] = ix; }
   __syncthreads();
   v = redV[0]; ix = redI[0];
#pragma unroll
   for (int w = 1; w < DC_WAVES; w++) dc_take(v, ix, redV[w], redI[w]);
}
// first minimum of row k over the live columns j > k, by one wavefront
static __device__ void dc_row_min(const float *g, int n, int k, const int *alive, float *rowMin, int *rowArg)
{
   const int lane = threadIdx.x & 63;
   float v = 0.0f; int ix = -1;
   for (int j = k + 1 + lane; j < n; j += 64) if (alive[j]) dc_take(v, ix, g[(size_t)k * n + j], j);
   dc_wave_min(v, ix);
   if (lane == 0) { rowMin[k] = v; rowArg[k] = ix; }
}

__global__ __launch_bounds__(DC_THREADS) void k_dc_merge(const DcCmd *cmds, float *gAll, const float *occ, float outlierThresh, int *chain /*[2][items]: next, tail*/,
                                                          int nItems, int *merges, int *nMerges)
{
   extern __shared__ int lds[];
   __shared__ float redV[DC_WAVES];
   __shared__ int redI[DC_WAVES], cnt[2], nList;
   const DcCmd c = cmds[blockIdx.x];
   const int n = c.n, t = threadIdx.x;
   float *g = gAll + c.mat;
   int *alive = lds, *rowArg = lds + n, *list = lds + 2 * n;
   float *rowMin = (float *)(lds + 3 * n), *occSum = (float *)(lds + 4 * n);
   int *next = chain + c.off, *tail = chain + nItems + c.off, *log = merges + 2 * (size_t)c.off;
   for (int i = t; i < n; i += DC_THREADS) { alive[i] = 1; next[i] = -1; tail[i] = i; }
   __syncthreads();
   for (int k = t >> 6; k < n; k += DC_WAVES) dc_row_min(g, n, k, alive, rowMin, rowArg);
   int numClust = n, nLog = 0;
   // Clustering's loop (:2036)
   while (numClust > c.numReq) {
      __syncthreads();                                  // the row minima of the round before
      float v = 0.0f; int a = -1;
      for (int i = t; i < n; i += DC_THREADS) if (alive[i] && rowArg[i] >= 0) dc_take(v, a, rowMin[i], i);
      dc_block_min(v, a, redV, redI);
      if (a < 0 || !(v < c.threshold)) break;
      const int b = rowArg[a];
      if (t == 0) { cnt[0] = 0; cnt[1] = 0; nList = 0; }
      __syncthreads();
      {  // the groups' current numbers, and the rows to look at again
         int ca = 0, cb = 0;
         for (int i = t; i < b; i += DC_THREADS) if (alive[i]) { cb++; if (i < a) ca++; }
         for (int d = 32; d >= 1; d >>= 1) { ca += __shfl_xor(ca, d); cb += __shfl_xor(cb, d); }
         if ((t & 63) == 0) { atomicAdd(&cnt[0], ca); atomicAdd(&cnt[1], cb); }
         for (int k = t; k < n; k += DC_THREADS)
            if (alive[k] && k != a && k != b) {
               const float m = fmaxf(g[(size_t)a * n + k], g[(size_t)b * n + k]);
               g[(size_t)a * n + k] = m; g[(size_t)k * n + a] = m;
               if (rowArg[k] == a || rowArg[k] == b) list[atomicAdd(&nList, 1)] = k;
            }
      }
      __syncthreads();
      if (t == 0) {
         alive[b] = 0;
         log[2 * nLog] = cnt[0] + 1; log[2 * nLog + 1] = cnt[1] + 1;
         next[tail[a]] = b; tail[a] = tail[b];
         list[nList] = a;
      }
      __syncthreads();
      if (nLog == 0) {                                  // the first SetGDist starts every maximum at 0.0 (:1829): from here on no entry is below it
         for (size_t x = t; x < (size_t)n * n; x += DC_THREADS) { const float v = g[x]; g[x] = v > 0.0f ? v : 0.0f; }
         __syncthreads();
         for (int k = t >> 6; k < n; k += DC_WAVES) if (alive[k]) dc_row_min(g, n, k, alive, rowMin, rowArg);
      } else {
         const int nl = nList + 1;
         for (int q = t >> 6; q < nl; q += DC_WAVES) dc_row_min(g, n, list[q], alive, rowMin, rowArg);
      }
      nLog++; numClust--;
   }
   __syncthreads();
   // RemOutliers (:1975)
   if (occ) {
      for (int i = t; i < n; i += DC_THREADS)
         if (alive[i]) { float s = 0.0f; for (int m = i; m >= 0; m = next[m]) s = __fadd_rn(s, occ[c.off + m]); occSum[i] = s; }
      __syncthreads();
      while (numClust > 1) {
         float v = 0.0f; int sp = -1;
         for (int i = t; i < n; i += DC_THREADS) if (alive[i]) dc_take(v, sp, occSum[i], i);
         dc_block_min(v, sp, redV, redI);
         if (sp < 0 || !(v < outlierThresh)) break;
         float mv = 0.0f; int b = -1;
         for (int k = t; k < n; k += DC_THREADS) if (alive[k] && k != sp) dc_take(mv, b, g[(size_t)sp * n + k], k);
         dc_block_min(mv, b, redV, redI);
         if (b < 0) break;
         if (t == 0) { cnt[0] = 0; cnt[1] = 0; }
         __syncthreads();
         int ca = 0, cb = 0;
         for (int i = t; i < n; i += DC_THREADS) if (alive[i]) { if (i < sp) ca++; if (i < b) cb++; }
         for (int d = 32; d >= 1; d >>= 1) { ca += __shfl_xor(ca, d); cb += __shfl_xor(cb, d); }
         if ((t & 63) == 0) { atomicAdd(&cnt[0], ca); atomicAdd(&cnt[1], cb); }
         for (int k = t; k < n; k += DC_THREADS)
            if (alive[k] && k != sp && k != b) {
               const float m = fmaxf(g[(size_t)sp * n + k], g[(size_t)b * n + k]);
               g[(size_t)sp * n + k] = m; g[(size_t)k * n + sp] = m;
            }
         __syncthreads();
         if (t == 0) {
            alive[b] = 0;
            log[2 * nLog] = cnt[0] + 1; log[2 * nLog + 1] = cnt[1] + 1;
            next[tail[sp]] = b; tail[sp] = tail[b];
            occSum[sp] = __fadd_rn(occSum[sp], occSum[b]);
         }
         __syncthreads();
         if (nLog == 0) {
            for (size_t x = t; x < (size_t)n * n; x += DC_THREADS) { const float v = g[x]; g[x] = v > 0.0f ? v : 0.0f; }
            __syncthreads();
         }
         nLog++; numClust--;
      }
   }
   if (t == 0) nMerges[blockIdx.x] = nLog;
}

// ------------------------------------------------------------------------------------------ host side of the device
DEVBUF_OWNER("data_cluster")

extern "C" int htkamd_dc_dev_run(const htkamd_dc_job *job, float *idistOut, int *merges, int *nMerges, void *stream)
{
   if (!job || job->nCmds < 1 || !job->cmds || job->nItems < 1) { htkamd_set_error("data_cluster: bad argument"); return HTKAMD_EINVAL; }
   const int sources = (job->idist != nullptr) + (job->mean != nullptr) + (job->desc != nullptr);
   if (sources != 1 || (job->mean && (!job->var || job->V < 1)) || (job->desc && !job->itemState) || (!job->noMerge && (!merges || !nMerges))) {
      htkamd_set_error("data_cluster: bad argument"); return HTKAMD_EINVAL;
   }
   // every index the kernels will form, checked here
   DcCmd *hc = (DcCmd *)malloc(sizeof(DcCmd) * (size_t)job->nCmds);
   long long tot = 0; int items = 0, maxN = 0;
   for (int k = 0; k < job->nCmds; k++) {
      const htkamd_dc_cmd &c = job->cmds[k];
      if (c.n < 1 || c.off != items || c.numReq < 1 || (long long)items + c.n > job->nItems) { free(hc); htkamd_set_error("data_cluster: command %d: bad item range or cluster count", k); return HTKAMD_EINVAL; }
      if (c.n > HTKAMD_DC_MAXITEMS) { free(hc); htkamd_set_error("data_cluster: command %d has %d items (at most %d)", k, c.n, HTKAMD_DC_MAXITEMS); return HTKAMD_EINVAL; }
      hc[k].mat = tot; hc[k].off = c.off; hc[k].n = c.n; hc[k].numReq = c.numReq; hc[k].threshold = c.threshold;
      tot += (long long)c.n * c.n; items += c.n;
      if (c.n > maxN) maxN = c.n;
   }
   if (items != job->nItems) { free(hc); htkamd_set_error("data_cluster: %d items in the commands, %d given", items, job->nItems); return HTKAMD_EINVAL; }
   if (htkamd_device_count() <= 0) { free(hc); htkamd_set_error("data_cluster: no HIP device"); return HTKAMD_ENODEV; }
   hipStream_t st = (hipStream_t)stream;
   DevBuf dist, cmds, a, b, occ, chain, log, nlog, score, obs, sts;
   htkamd_model *model = nullptr;
   int *obsOff = nullptr; float *X = nullptr;
   int rc = dist.reserve<float>((size_t)tot);
   if (!rc) rc = cmds.upload(hc, (size_t)job->nCmds, st);
   if (job->idist) { if (!rc) rc = dist.upload(job->idist, (size_t)tot, st); }
   else if (job->mean) {
      if (!rc) rc = a.upload(job->mean, (size_t)items * job->V, st);
      if (!rc) rc = b.upload(job->var, (size_t)items * job->V, st);
      for (int k = 0; k < job->nCmds && !rc; k++) {
         const unsigned tiles = (unsigned)((hc[k].n + DC_TILE - 1) / DC_TILE);
         hipLaunchKernelGGL(k_dc_divergence, dim3(tiles, tiles), dim3(DC_TILE, DC_TILE), 0, st, a.as<const float>(), b.as<const float>(), job->V, hc[k].off, hc[k].n,
                            dist.as<float>() + hc[k].mat);
         HIPCHECK_RC(rc, devOwner, hipGetLastError());
      }
   } else {
      // GDistance: the observations are every component mean of every item, the states are the items
      const htkamd_model_desc *d = job->desc;
      const int D = d->vecSize;
      obsOff = (int *)malloc(sizeof(int) * ((size_t)items + 1));
      int T = 0, maxT = 0;
      for (int i = 0; i < items && !rc; i++) {
         const int s = job->itemState[i];
         if (s < 0 || s >= d->numStates) { htkamd_set_error("data_cluster: item %d names state %d of %d", i, s, d->numStates); rc = HTKAMD_EINVAL; break; }
         obsOff[i] = T; T += d->stateCompOff[s + 1] - d->stateCompOff[s];
      }
      obsOff[items] = T;
      if (!rc) rc = htkamd_model_create(d, &model);
      if (!rc) {
         X = (float *)malloc(sizeof(float) * (size_t)(T ? T : 1) * D);
         for (int i = 0; i < items; i++) {
            const int s = job->itemState[i], c0 = d->stateCompOff[s];
            for (int m = 0; m < obsOff[i + 1] - obsOff[i]; m++) memcpy(X + (size_t)(obsOff[i] + m) * D, d->mean + (size_t)d->compGauss[c0 + m] * D, sizeof(float) * (size_t)D);
         }
         for (int k = 0; k < job->nCmds; k++) { const int Tc = obsOff[hc[k].off + hc[k].n] - obsOff[hc[k].off]; if (Tc > maxT) maxT = Tc; }
         rc = a.reserve<float>((size_t)maxT * D);
         if (!rc) rc = obs.reserve<int>((size_t)maxN + 1);
         if (!rc) rc = sts.upload(job->itemState, (size_t)items, st);
         if (!rc) rc = score.reserve<float>((size_t)maxN * maxT);
      }
      for (int k = 0; k < job->nCmds && !rc; k++) {
         // the command's own offsets start at 0
         const int o0 = obsOff[hc[k].off], Tc = obsOff[hc[k].off + hc[k].n] - o0;
         int *rel = (int *)malloc(sizeof(int) * ((size_t)hc[k].n + 1));
         for (int i = 0; i <= hc[k].n; i++) rel[i] = obsOff[hc[k].off + i] - o0;
         if (!rc) rc = obs.upload(rel, (size_t)hc[k].n + 1, st);
         if (!rc) rc = a.upload(X + (size_t)o0 * D, (size_t)Tc * D, st);
         HIPCHECK_RC(rc, devOwner, hipStreamSynchronize(st));               // (rel goes; the observation and score buffers are one command's)
         free(rel);
         if (!rc) rc = htkamd_outp_block_mode(model, a.as<const float>(), Tc, sts.as<const int>() + hc[k].off, hc[k].n, score.as<float>(), Tc,
                                              HTKAMD_SCORE_SOUTP | HTKAMD_SCORE_DIAGC, st);
         if (rc) break;
         const unsigned tiles = (unsigned)((hc[k].n + DC_TILE - 1) / DC_TILE);
         hipLaunchKernelGGL(k_dc_gdist, dim3(tiles, tiles), dim3(DC_TILE, DC_TILE), 0, st, score.as<const float>(), Tc, obs.as<const int>(), hc[k].n,
                            dist.as<float>() + hc[k].mat);
         HIPCHECK_RC(rc, devOwner, hipGetLastError());
         HIPCHECK_RC(rc, devOwner, hipStreamSynchronize(st));
      }
   }
   if (idistOut && !rc) rc = dist.download(idistOut, (size_t)tot, st);
   if (!job->noMerge) {
      if (!rc) rc = chain.reserve<int>(2 * (size_t)items);
      if (!rc) rc = log.reserve<int>(2 * (size_t)items);
      if (!rc) rc = nlog.reserve<int>((size_t)job->nCmds);
      if (!rc && job->occ) rc = occ.upload(job->occ, (size_t)items, st);
      if (!rc) {
         hipLaunchKernelGGL(k_dc_merge, dim3((unsigned)job->nCmds), dim3(DC_THREADS), sizeof(int) * 5 * (size_t)maxN + sizeof(int), st, cmds.as<const DcCmd>(), dist.as<float>(),
                            job->occ ? occ.as<const float>() : (const float *)nullptr, job->outlierThresh, chain.as<int>(), items, log.as<int>(), nlog.as<int>());
         HIPCHECK_RC(rc, devOwner, hipGetLastError());
      }
      if (!rc) rc = log.download(merges, 2 * (size_t)items, st);
      if (!rc) rc = nlog.download(nMerges, (size_t)job->nCmds, st);
   }
   HIPCHECK_RC(rc, devOwner, hipStreamSynchronize(st));
   if (model) htkamd_model_destroy(model);
   free(hc); free(obsOff); free(X);
   return rc;
}
