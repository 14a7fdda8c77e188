// vquant.hip -- VQ codebooks and VQ coding: FlatCluster (HTKLib/HTrain.c:763) and TreeCluster (:806) of ONE pool of N vectors spread
// over the grid (HQuant's pools: every frame of a training set), and GetVQ (HTKLib/HVQ.c:459) for a batch.  k_flat_cluster (hinit.hip)
// is the same algorithm for many small pools, a workgroup each; here nothing but the centres' tile lives in a workgroup.
// The reference's arithmetic with every rounding written out (the file is compiled with FMA contraction off):
//
// k_vq_assign   AllocateVectors (:482), a lane per item.  The item's vector is in registers (the kernels are instantiated for up to 16,
//               40 and VQ_MAX_D values; at the largest the compiler keeps it in private memory); the centres pass through LDS in tiles of
//               VQ_TILE floats laid out [centre][dimension], so that the 64 lanes of a wavefront read ONE address at a time (a broadcast,
//               no bank conflict); the covariance of Distance (:424) -- one for the whole pool: D floats, or the D(D+1)/2 of FULLC --
//               stands in front of the tile.  Distance: float differences, the double sum in dimension order (FULLC: float products of
//               the strict lower triangle in (i, j) order, doubled, then the diagonal), the double square root rounded to float; the
//               first strict minimum over the centres in order.  Writes cmap[i] and min[i].
//               LDS: 4 * (VQ_TILE + covLen) bytes; at D = VQ_MAX_D = 128 and FULLC 16384 + 33024 = 49408 bytes, K up to 1024 in
//               ceil(K / (VQ_TILE / D)) tiles (32 centres a tile at D = 128, 105 at D = 39).
// k_vq_split    SplitVectors (:530) for every node of a tree's row in one launch: an item looks its node's two children up.
// k_vq_rank / k_vq_scan / k_vq_scatter   the items' numbers bucketed by cluster STABLY.  A workgroup ranks a chunk of VQ_CHUNK items:
//               a wavefront at a time, in item order, lanes with the same cluster find one another by ballot, the group's first lane
//               reads the chunk's running count of that cluster from LDS and the group writes it back increased -- no atomic, so a
//               rank is the number of earlier items of the cluster.  Then a lane per cluster walks the chunks' counts (an exclusive
//               scan down the chunks, the cluster's size at the end), a block scan over the sizes gives every bucket's start, and the
//               scatter places item i at start + chunk offset + rank: buckets in item order.
// k_vq_centres  FindCentres (:562): a lane per (cluster, dimension) walks its OWN bucket in order: float adds, a float divide by
// k_vq_costs    (float)csize.  A lane per cluster walks its bucket for aveCost; one lane walks min[] through LDS-staged chunks (the
// k_vq_cov      other 255 load the next chunk meanwhile) for totalCost.  FindCovariance (:587) over the same buckets: double sums
//               of double products of float differences, a double divide rounded to float (FULLC: the covariance's triangle; the
//               host inverts it as CovInvert does, host/vqtab.c).
//               The reference adds in item order; a bucket holds a cluster's items in item order; so every sum sees the same
//               operands in the same order, and no atomic touches a value that reaches the output: two runs give the same bytes.
// k_vq_finish / k_vq_perturb / k_vq_tree_perturb   the control flow that stays on the device: the averages up to the first cluster
//               below minClustSize, FullestCluster (:665), BiggestCluster (:649, with its quirk: the running maximum moves even where
//               the cluster is too small to be chosen), Perturb (:678).  The host reads one 12-byte record per AllocateVectors round
//               (the cluster to repair, the total cost, the fullest cluster) and decides repair / convergence / next cluster count.
//               One flat iteration is 7 launches (assign, rank, scan, scatter, costs, finish, centres) and one read-back; one tree
//               level is 7 launches (perturb, split, rank, scan, scatter, centres, covariance) and one read-back of the children's sizes.
// k_vq_code     GetVQ: a lane per (frame, stream).  Linear tables: the nodes pass through LDS in list order, a node's mean, inverse
//               covariance and gconst behind one another (VQ_CODE_TILE floats a tile; a broadcast read again); VQNodeScore (:414) with
//               its FLOAT sum, gconst + sum, the first strict minimum.  Trees: the lane descends, (xr < xl) ? right : left.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "internal.h"
#include "hipcheck.h"
#include "devbuf.h"
#include "vquant.h"

#define VQ_THREADS    256
#define VQ_MAX_D      128
#define VQ_MAX_NC     1024
#define VQ_CHUNK      1024                                 // items a workgroup ranks
#define VQ_TILE       4096                                 // floats of centres in LDS
#define VQ_CODE_TILE  12288                                // floats of table nodes in LDS (one FULLC node of 128 dimensions is 8385)
#define VQ_SUM_CHUNK  2048                                 // floats of min[] staged for the total's lane

DEVBUF_OWNER("vq")

static __host__ __device__ inline int vq_cov_len(int D, int kind)
{
   return kind == HTKAMD_CK_NULLC ? 0 : kind == HTKAMD_CK_FULLC ? D * (D + 1) / 2 : (kind == HTKAMD_CK_DIAGC || kind == HTKAMD_CK_INVDIAGC) ? D : -1;
}

struct VqArgs {
   const float *X; int N, D;
   int distKind, clustKind, dCovLen, cCovLen, minClust;
   const float *distCov;
   float *ctr, *cov, *ave; int *csize;                     // per node
   int *cmap; float *mn;                                   // per item
   int *lrank, *bucket;                                    // per item
   int *cnt; int nChunks;                                  // [nChunks][Kc]
   int *start;                                             // [VQ_MAX_NC]
   int *rec;                                               // ce, total (float bits), fullest
};

// ------------------------------------------------------------------------------------------ Distance
// x: the item in registers; ctr, cov: LDS or memory.  FULLC indexes the differences by loop counters that are not unrolled: they live
// in private memory there.
template <int DCAP> static __device__ float vq_distance(int kind, int D, const float (&x)[DCAP], const float *ctr, const float *cov)
{
   double s = 0.0;
   if (kind == HTKAMD_CK_FULLC) {
      float df[DCAP];
#pragma unroll
      for (int d = 0; d < DCAP; d++) df[d] = d < D ? __fsub_rn(x[d], ctr[d]) : 0.0f;
#pragma unroll 1
      for (int i = 1; i < D; i++) {
         const float *row = cov + i * (i + 1) / 2;
#pragma unroll 1
         for (int j = 0; j < i; j++) s = __dadd_rn(s, (double)__fmul_rn(__fmul_rn(df[i], df[j]), row[j]));
      }
      s = __dmul_rn(s, 2.0);
#pragma unroll 1
      for (int i = 0; i < D; i++) s = __dadd_rn(s, (double)__fmul_rn(__fmul_rn(df[i], df[i]), cov[i * (i + 1) / 2 + i]));
   } else {
#pragma unroll
      for (int d = 0; d < DCAP; d++)
         if (d < D) {
            const double df = (double)__fsub_rn(x[d], ctr[d]);
            double q = __dmul_rn(df, df);
            if (kind == HTKAMD_CK_DIAGC) q = __ddiv_rn(q, (double)cov[d]);
            else if (kind == HTKAMD_CK_INVDIAGC) q = __dmul_rn(q, (double)cov[d]);
            s = __dadd_rn(s, q);
         }
   }
   return (float)__dsqrt_rn(s);
}

template <int DCAP> static __device__ void vq_load_item(const VqArgs &a, int i, float (&x)[DCAP])
{
   const bool ok = i < a.N;
   const float *row = a.X + (size_t)(ok ? i : 0) * a.D;
#pragma unroll
   for (int d = 0; d < DCAP; d++) x[d] = (ok && d < a.D) ? row[d] : 0.0f;
}

// AllocateVectors over clusters 0 .. k-1
template <int DCAP> __global__ __launch_bounds__(VQ_THREADS) void k_vq_assign(VqArgs a, int k)
{
   extern __shared__ float vqLds[];
   float *cov = vqLds, *tile = vqLds + a.dCovLen;
   const int t = threadIdx.x, i = blockIdx.x * VQ_THREADS + t, D = a.D;
   float x[DCAP];
   vq_load_item<DCAP>(a, i, x);
   for (int e = t; e < a.dCovLen; e += VQ_THREADS) cov[e] = a.distCov[e];
   const int per = VQ_TILE / D;
   float best = 0.0f; int bi = 0;
   for (int c0 = 0; c0 < k; c0 += per) {
      const int nc = k - c0 < per ? k - c0 : per;
      __syncthreads();                                    // the tile's last readers are through (and cov is there, the first time)
      for (int e = t; e < nc * D; e += VQ_THREADS) tile[e] = a.ctr[(size_t)c0 * D + e];
      __syncthreads();
      for (int c = 0; c < nc; c++) {
         const float dist = vq_distance<DCAP>(a.distKind, D, x, tile + c * D, cov);
         if (c0 + c == 0 || dist < best) { best = dist; bi = c0 + c; }
      }
   }
   if (i < a.N) { a.cmap[i] = bi; a.mn[i] = best; }
}

// SplitVectors for every node of the row [row0, row0 + rowSize): the children of node n are row0 + rowSize + 2 (n - row0) and the next
template <int DCAP> __global__ __launch_bounds__(VQ_THREADS) void k_vq_split(VqArgs a, int row0, int rowSize)
{
   extern __shared__ float vqLds[];
   float *cov = vqLds;
   const int t = threadIdx.x, i = blockIdx.x * VQ_THREADS + t, D = a.D;
   float x[DCAP];
   vq_load_item<DCAP>(a, i, x);
   for (int e = t; e < a.dCovLen; e += VQ_THREADS) cov[e] = a.distCov[e];
   __syncthreads();
   if (i >= a.N) return;
   const int n = a.cmap[i];
   if (n < row0 || n >= row0 + rowSize) return;            // (every item is in the row: the root's pool is the whole pool)
   const int n1 = row0 + rowSize + 2 * (n - row0), n2 = n1 + 1;
   const float d1 = vq_distance<DCAP>(a.distKind, D, x, a.ctr + (size_t)n1 * D, cov);
   const float d2 = vq_distance<DCAP>(a.distKind, D, x, a.ctr + (size_t)n2 * D, cov);
   a.cmap[i] = d1 < d2 ? n1 : n2;
}

// ------------------------------------------------------------------------------------------ stable buckets
// keys cmap[i] - keyBase in [0, Kc), Kc <= VQ_MAX_NC
__global__ __launch_bounds__(VQ_THREADS) void k_vq_rank(VqArgs a, int keyBase, int Kc)
{
   __shared__ int hist[VQ_MAX_NC];
   const int t = threadIdx.x, w = t >> 6, lane = t & 63, b = blockIdx.x;
   for (int c = t; c < Kc; c += VQ_THREADS) hist[c] = 0;
   __syncthreads();
   for (int r = 0; r < VQ_CHUNK / VQ_THREADS; r++) {
      const int i = b * VQ_CHUNK + r * VQ_THREADS + t;
      int c = i < a.N ? a.cmap[i] - keyBase : -1;
      if (c >= Kc) c = -1;                                 // (cannot be: the caller's keys are in range)
      int rk = 0, cnt = 0;
      unsigned long long todo = __ballot(c >= 0);
      while (todo) {                                       // one turn per distinct cluster of the wavefront
         const int src = __ffsll((long long)todo) - 1;
         const int v = __shfl(c, src);
         const unsigned long long m = __ballot(c == v);
         if (c == v) { rk = __popcll(m & ((1ull << lane) - 1ull)); cnt = __popcll(m); }
         todo &= ~m;
      }
      for (int ww = 0; ww < VQ_THREADS / 64; ww++) {       // the wavefronts in item order
         if (w == ww && c >= 0) {
            const int base = hist[c];
            __builtin_amdgcn_wave_barrier();               // every lane of a group has read before its first lane writes
            if (rk == 0) hist[c] = base + cnt;
            a.lrank[i] = base + rk;
         }
         __syncthreads();
      }
   }
   for (int c = t; c < Kc; c += VQ_THREADS) a.cnt[(size_t)b * Kc + c] = hist[c];
}

// a lane per cluster: the chunks' counts to offsets, the size; then every bucket's start.  One workgroup of VQ_MAX_NC lanes.
__global__ __launch_bounds__(VQ_MAX_NC) void k_vq_scan(VqArgs a, int keyBase, int Kc)
{
   __shared__ int buf[2][VQ_MAX_NC];
   const int c = threadIdx.x;
   int run = 0;
   if (c < Kc) {
      for (int b = 0; b < a.nChunks; b++) {
         const size_t at = (size_t)b * Kc + c;
         const int v = a.cnt[at];
         a.cnt[at] = run;
         run += v;
      }
      a.csize[keyBase + c] = run;
   }
   int cur = 0;
   buf[0][c] = run;
   __syncthreads();
   for (int step = 1; step < VQ_MAX_NC; step <<= 1) {
      buf[cur ^ 1][c] = buf[cur][c] + (c >= step ? buf[cur][c - step] : 0);
      cur ^= 1;
      __syncthreads();
   }
   if (c < Kc) a.start[c] = buf[cur][c] - run;
}

__global__ __launch_bounds__(VQ_THREADS) void k_vq_scatter(VqArgs a, int keyBase, int Kc)
{
   const int i = blockIdx.x * VQ_THREADS + threadIdx.x;
   if (i >= a.N) return;
   const int c = a.cmap[i] - keyBase;
   if (c < 0 || c >= Kc) return;
   const int at = a.start[c] + a.cnt[(size_t)(i / VQ_CHUNK) * Kc + c] + a.lrank[i];
   if (at >= 0 && at < a.N) a.bucket[at] = i;
}

// ------------------------------------------------------------------------------------------ the walks over a bucket
// FindCentres(keyBase, keyBase + Kc - 1)
__global__ __launch_bounds__(VQ_THREADS) void k_vq_centres(VqArgs a, int keyBase, int Kc)
{
   const int e = blockIdx.x * VQ_THREADS + threadIdx.x, D = a.D;
   if (e >= Kc * D) return;
   const int c = e / D, d = e - c * D, n = a.csize[keyBase + c];
   const int *item = a.bucket + a.start[c];
   float s = 0.0f;
   int q = 0;
   for (; q + 4 <= n; q += 4) {                            // four loads in flight, the adds in order
      const float v0 = a.X[(size_t)item[q] * D + d], v1 = a.X[(size_t)item[q + 1] * D + d], v2 = a.X[(size_t)item[q + 2] * D + d], v3 = a.X[(size_t)item[q + 3] * D + d];
      s = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(s, v0), v1), v2), v3);
   }
   for (; q < n; q++) s = __fadd_rn(s, a.X[(size_t)item[q] * D + d]);
   a.ctr[(size_t)(keyBase + c) * D + d] = __fdiv_rn(s, (float)n);
}

// the cost chains of AllocateVectors over clusters 0 .. k-1: workgroup 0 the total, the others a lane per cluster
__global__ __launch_bounds__(VQ_THREADS) void k_vq_costs(VqArgs a, int k)
{
   __shared__ float stage[2][VQ_SUM_CHUNK];
   const int t = threadIdx.x;
   if (blockIdx.x == 0) {
      const int nCh = (a.N + VQ_SUM_CHUNK - 1) / VQ_SUM_CHUNK;
      float s = 0.0f;
      for (int e = t; e < VQ_SUM_CHUNK; e += VQ_THREADS) stage[0][e] = e < a.N ? a.mn[e] : 0.0f;
      __syncthreads();
      for (int ch = 0; ch < nCh; ch++) {
         const int cur = ch & 1, base = (ch + 1) * VQ_SUM_CHUNK;
         if (t == 0) {
            const int n = a.N - ch * VQ_SUM_CHUNK < VQ_SUM_CHUNK ? a.N - ch * VQ_SUM_CHUNK : VQ_SUM_CHUNK;
            for (int e = 0; e < n; e++) s = __fadd_rn(s, stage[cur][e]);
         } else if (ch + 1 < nCh)
            for (int e = t - 1; e < VQ_SUM_CHUNK; e += VQ_THREADS - 1) stage[cur ^ 1][e] = base + e < a.N ? a.mn[base + e] : 0.0f;
         __syncthreads();
      }
      if (t == 0) a.rec[1] = __float_as_int(s);
      return;
   }
   const int c = (blockIdx.x - 1) * VQ_THREADS + t;
   if (c >= k) return;
   const int n = a.csize[c];
   const int *item = a.bucket + a.start[c];
   float s = 0.0f;
   int q = 0;
   for (; q + 4 <= n; q += 4) {
      const float v0 = a.mn[item[q]], v1 = a.mn[item[q + 1]], v2 = a.mn[item[q + 2]], v3 = a.mn[item[q + 3]];
      s = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(s, v0), v1), v2), v3);
   }
   for (; q < n; q++) s = __fadd_rn(s, a.mn[item[q]]);
   a.ave[c] = s;
}

// the end of AllocateVectors (averages up to the first cluster that is too small) and FullestCluster
__global__ void k_vq_finish(VqArgs a, int k)
{
   if (blockIdx.x != 0 || threadIdx.x != 0) return;
   int ce = 0;
   for (int c = 0; c < k; c++) {
      if (a.csize[c] < a.minClust) { ce = c + 1; break; }
      a.ave[c] = __fdiv_rn(a.ave[c], (float)a.csize[c]);
   }
   int mx = a.csize[0], full = 0;
   for (int c = 0; c < k; c++) if (a.csize[c] > mx) { mx = a.csize[c]; full = c; }
   a.rec[0] = ce; a.rec[2] = full;
}

static __device__ float vq_perturb_step(float v)
{
   float x = (float)fabs(__dmul_rn((double)v, 0.01));
   if ((double)x < 0.0001) x = 0.0001f;
   return x;
}

// Perturb(from, from, to); from < 0: BiggestCluster over the kBig clusters there are
__global__ __launch_bounds__(VQ_THREADS) void k_vq_perturb(VqArgs a, int from, int to, int kBig)
{
   __shared__ int sPick;
   if (threadIdx.x == 0) {
      int big = from;
      if (from < 0) {
         float mx = a.ave[0]; big = 0;
         for (int c = 1; c < kBig; c++) if (a.ave[c] > mx) { mx = a.ave[c]; if (a.csize[c] >= a.minClust) big = c; }
      }
      sPick = big;
   }
   __syncthreads();
   const int n = sPick, D = a.D;
   for (int d = threadIdx.x; d < D; d += VQ_THREADS) {
      const float v = a.ctr[(size_t)n * D + d], x = vq_perturb_step(v), up = __fadd_rn(v, x);
      if (to == n) a.ctr[(size_t)n * D + d] = __fsub_rn(up, x);
      else { a.ctr[(size_t)n * D + d] = up; a.ctr[(size_t)to * D + d] = __fsub_rn(v, x); }
   }
}

// Perturb(n, n1, n2) for every node of a tree's row
__global__ __launch_bounds__(VQ_THREADS) void k_vq_tree_perturb(VqArgs a, int row0, int rowSize)
{
   const int e = blockIdx.x * VQ_THREADS + threadIdx.x, D = a.D;
   if (e >= rowSize * D) return;
   const int r = e / D, d = e - r * D, n = row0 + r, n1 = row0 + rowSize + 2 * r;
   const float v = a.ctr[(size_t)n * D + d], x = vq_perturb_step(v);
   a.ctr[(size_t)n1 * D + d] = __fadd_rn(v, x);
   a.ctr[(size_t)(n1 + 1) * D + d] = __fsub_rn(v, x);
}

// FindCovariance of clusters keyBase .. keyBase + Kc - 1: DIAGC / INVDIAGC a lane per (cluster, dimension), FULLC a lane per (cluster,
// j, k <= j) and the covariance itself (the host inverts)
__global__ __launch_bounds__(VQ_THREADS) void k_vq_cov(VqArgs a, int keyBase, int Kc)
{
   const int e = blockIdx.x * VQ_THREADS + threadIdx.x, D = a.D, L = a.cCovLen;
   if (L <= 0 || e >= Kc * L) return;
   const int c = e / L, p = e - c * L, n = a.csize[keyBase + c];
   const int *item = a.bucket + a.start[c];
   const float *mean = a.ctr + (size_t)(keyBase + c) * D;
   const double nx = (double)n;
   float out;
   if (a.clustKind == HTKAMD_CK_FULLC) {
      int j = (int)((sqrtf(8.0f * (float)p + 1.0f) - 1.0f) * 0.5f);
      while (j * (j + 1) / 2 > p) j--;
      while ((j + 1) * (j + 2) / 2 <= p) j++;
      const int k = p - j * (j + 1) / 2;
      const float mj = mean[j], mk = mean[k];
      double s = 0.0;
      for (int q = 0; q < n; q++) {
         const float *v = a.X + (size_t)item[q] * D;
         s = __dadd_rn(s, __dmul_rn((double)__fsub_rn(v[j], mj), (double)__fsub_rn(v[k], mk)));
      }
      out = (float)__ddiv_rn(s, nx);
   } else {
      const float mu = mean[p];
      double s = 0.0;
      for (int q = 0; q < n; q++) { const double df = (double)__fsub_rn(a.X[(size_t)item[q] * D + p], mu); s = __dadd_rn(s, __dmul_rn(df, df)); }
      out = a.clustKind == HTKAMD_CK_DIAGC ? (float)__ddiv_rn(s, nx) : (float)__ddiv_rn(nx, s);
   }
   a.cov[(size_t)(keyBase + c) * L + p] = out;
}

__global__ void k_vq_init(VqArgs a, int nodes)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i < a.N) a.cmap[i] = 0;
   if (i < nodes) { a.csize[i] = i == 0 ? a.N : 0; a.ave[i] = i == 0 ? 1.0f : 0.0f; }
   if (i < 3) a.rec[i] = 0;
}

// ------------------------------------------------------------------------------------------ the host's side
extern "C" int htkamd_vq_max_dim(void) { return VQ_MAX_D; }
extern "C" int htkamd_vq_max_clusters(void) { return VQ_MAX_NC; }
extern "C" int htkamd_vq_cov_len(int D, int kind) { return D < 1 ? -1 : vq_cov_len(D, kind); }
extern "C" int htkamd_vq_num_nodes(int nc, int tree)
{
   if (nc < 1) return 0;
   if (!tree) return nc;
   for (int n = nc; n > 2; n /= 2) if (n % 2 == 1) return 0;      // NumTreeNodes :699
   return 2 * nc - 1;
}

namespace {
struct VqRun {
   VqArgs a;
   hipStream_t s;
   int launches;
   unsigned itemBlocks() const { return (unsigned)((a.N + VQ_THREADS - 1) / VQ_THREADS); }
   size_t ldsAssign() const { return sizeof(float) * (size_t)(VQ_TILE + a.dCovLen); }
   template <typename K, typename... A> void go(K k, dim3 g, dim3 b, size_t lds, A... args) { hipLaunchKernelGGL(k, g, b, lds, s, args...); launches++; }
   void assign(int k)
   {
      if (a.D <= 16) go(k_vq_assign<16>, dim3(itemBlocks()), dim3(VQ_THREADS), ldsAssign(), a, k);
      else if (a.D <= 40) go(k_vq_assign<40>, dim3(itemBlocks()), dim3(VQ_THREADS), ldsAssign(), a, k);
      else go(k_vq_assign<VQ_MAX_D>, dim3(itemBlocks()), dim3(VQ_THREADS), ldsAssign(), a, k);
   }
   void split(int row0, int rowSize)
   {
      const size_t lds = sizeof(float) * (size_t)(a.dCovLen ? a.dCovLen : 1);
      if (a.D <= 16) go(k_vq_split<16>, dim3(itemBlocks()), dim3(VQ_THREADS), lds, a, row0, rowSize);
      else if (a.D <= 40) go(k_vq_split<40>, dim3(itemBlocks()), dim3(VQ_THREADS), lds, a, row0, rowSize);
      else go(k_vq_split<VQ_MAX_D>, dim3(itemBlocks()), dim3(VQ_THREADS), lds, a, row0, rowSize);
   }
   void buckets(int keyBase, int Kc)
   {
      go(k_vq_rank, dim3((unsigned)a.nChunks), dim3(VQ_THREADS), 0, a, keyBase, Kc);
      go(k_vq_scan, dim3(1), dim3(VQ_MAX_NC), 0, a, keyBase, Kc);
      go(k_vq_scatter, dim3(itemBlocks()), dim3(VQ_THREADS), 0, a, keyBase, Kc);
   }
   void centres(int keyBase, int Kc) { go(k_vq_centres, dim3((unsigned)((Kc * a.D + VQ_THREADS - 1) / VQ_THREADS)), dim3(VQ_THREADS), 0, a, keyBase, Kc); }
   void cov(int keyBase, int Kc)
   {
      if (a.cCovLen > 0) go(k_vq_cov, dim3((unsigned)(((size_t)Kc * a.cCovLen + VQ_THREADS - 1) / VQ_THREADS)), dim3(VQ_THREADS), 0, a, keyBase, Kc);
   }
};
}

extern "C" int htkamd_vq_cluster(const float *dX, int N, int D, int nc, int tree, int distKind, const float *distCov, const htkamd_vq_config *cfg,
                                 htkamd_vq_clusters *out, void *stream)
{
   const int maxIter = cfg && cfg->maxIter > 0 ? cfg->maxIter : 10, minClust = cfg && cfg->minClustSize > 0 ? cfg->minClustSize : 3;
   const int clustKind = cfg && cfg->clustKind >= 0 ? cfg->clustKind : distKind;
   if (!dX || !out || N < 1 || D < 1 || nc < 1) { htkamd_set_error("vq_cluster: bad argument"); return HTKAMD_EINVAL; }
   if (D > VQ_MAX_D) { htkamd_set_error("vq_cluster: vectors of %d values (the library's maximum is %d)", D, VQ_MAX_D); return HTKAMD_EINVAL; }
   if (nc > VQ_MAX_NC) { htkamd_set_error("vq_cluster: %d clusters (the library's maximum is %d)", nc, VQ_MAX_NC); return HTKAMD_EINVAL; }
   const int dCovLen = vq_cov_len(D, distKind), cCovLen = vq_cov_len(D, clustKind);
   if (dCovLen < 0) { htkamd_set_error("vq_cluster: Distance: bad cov kind %d", distKind); return HTKAMD_VQ_EKIND; }
   if (cCovLen < 0) { htkamd_set_error("vq_cluster: InitClustering: bad cluster ckind %d", clustKind); return HTKAMD_VQ_EKIND; }
   if (dCovLen > 0 && !distCov) { htkamd_set_error("vq_cluster: a distance of kind %d needs its covariance", distKind); return HTKAMD_EINVAL; }
   if (N < nc) { htkamd_set_error("vq_cluster: InitClustering: only %d items for %d clusters", N, nc); return HTKAMD_VQ_ECLUSTER; }
   const int nodes = htkamd_vq_num_nodes(nc, tree);
   if (nodes == 0) { htkamd_set_error("vq_cluster: NumTreeNodes: nc %d not a power of 2", nc); return HTKAMD_VQ_EPOW2; }
   if (!out->size || !out->centre || !out->aveCost || (cCovLen > 0 && !out->cov)) { htkamd_set_error("vq_cluster: an output array is missing"); return HTKAMD_EINVAL; }
   if (htkamd_device_count() <= 0) { htkamd_set_error("vq_cluster: no HIP device"); return HTKAMD_ENODEV; }

   VqRun r;
   r.s = (hipStream_t)stream; r.launches = 0;
   VqArgs &a = r.a;
   memset(&a, 0, sizeof(a));
   a.X = dX; a.N = N; a.D = D; a.distKind = distKind; a.clustKind = clustKind; a.dCovLen = dCovLen; a.cCovLen = cCovLen; a.minClust = minClust;
   a.nChunks = (N + VQ_CHUNK - 1) / VQ_CHUNK;
   DevBuf bDist, bCtr, bCov, bAve, bSize, bMap, bMn, bRank, bBucket, bCnt, bStart, bRec;
   int rc;
   const size_t nI = (size_t)N, nCD = (size_t)nodes * D, nCL = (size_t)nodes * (cCovLen > 0 ? cCovLen : 1);
   if ((rc = bDist.upload(distCov, (size_t)dCovLen, r.s)) || (rc = bCtr.reserve<float>(nCD)) || (rc = bCov.reserve<float>(nCL)) || (rc = bAve.reserve<float>((size_t)nodes)) ||
       (rc = bSize.reserve<int>((size_t)nodes)) || (rc = bMap.reserve<int>(nI)) || (rc = bMn.reserve<float>(nI)) || (rc = bRank.reserve<int>(nI)) ||
       (rc = bBucket.reserve<int>(nI)) || (rc = bCnt.reserve<int>((size_t)a.nChunks * VQ_MAX_NC)) || (rc = bStart.reserve<int>(VQ_MAX_NC)) || (rc = bRec.reserve<int>(4)))
      return rc;
   a.distCov = bDist.as<const float>(); a.ctr = bCtr.as<float>(); a.cov = bCov.as<float>(); a.ave = bAve.as<float>(); a.csize = bSize.as<int>();
   a.cmap = bMap.as<int>(); a.mn = bMn.as<float>(); a.lrank = bRank.as<int>(); a.bucket = bBucket.as<int>(); a.cnt = bCnt.as<int>();
   a.start = bStart.as<int>(); a.rec = bRec.as<int>();
   HIPCHECK(hipMemsetAsync(a.ctr, 0, sizeof(float) * nCD, r.s));
   HIPCHECK(hipMemsetAsync(a.cov, 0, sizeof(float) * nCL, r.s));
   KernelTimer tm;
   HIPCHECK(tm.start(r.s));
   const int initN = N > nodes ? N : nodes;
   r.go(k_vq_init, dim3((unsigned)((initN + VQ_THREADS - 1) / VQ_THREADS)), dim3(VQ_THREADS), 0, a, nodes);
   r.buckets(0, 1);
   r.centres(0, 1);                                        // InitClustering: FindCentres(1, 1)
   int iterations = 0, err = 0;
   if (!tree) {
      for (int c = 2; c <= nc && !err; c++) {
         r.go(k_vq_perturb, dim3(1), dim3(VQ_THREADS), 0, a, -1, c - 1, c - 1);
         float oldCost = 1.0e10f;
         for (int iter = 0;; iter++) {
            int repair = 0, rec[3];
            for (;;) {
               r.assign(c);
               r.buckets(0, c);
               r.go(k_vq_costs, dim3((unsigned)(1 + (c + VQ_THREADS - 1) / VQ_THREADS)), dim3(VQ_THREADS), 0, a, c);
               r.go(k_vq_finish, dim3(1), dim3(64), 0, a, c);
               HIPCHECK(hipGetLastError());
               HIPCHECK(hipMemcpyAsync(rec, a.rec, sizeof(rec), hipMemcpyDeviceToHost, r.s));
               HIPCHECK(hipStreamSynchronize(r.s));
               iterations++;
               if (rec[0] == 0 || ++repair > c) break;
               r.go(k_vq_perturb, dim3(1), dim3(VQ_THREADS), 0, a, rec[2], rec[0] - 1, 0);      // fill it by splitting the fullest
            }
            if (rec[0] != 0) {
               htkamd_set_error("vq_cluster: FlatCluster: Failed to make %d clusters at iter %d (cluster %d has fewer than %d items)", c, iter, rec[0], minClust);
               err = HTKAMD_VQ_ECLUSTER; break;
            }
            float newCost;
            memcpy(&newCost, &rec[1], sizeof(float));
            const float rel = (oldCost - newCost) / oldCost;
            const bool conv = iter >= maxIter || (double)rel < 0.001;
            r.centres(0, c);
            oldCost = newCost;
            if (conv) break;
         }
      }
      if (!err) r.cov(0, nc);
   } else {
      r.cov(0, 1);
      std::vector<int> sz;
      for (int row0 = 0, rowSize = 1; rowSize < nc && !err; row0 += rowSize, rowSize *= 2) {
         const int kid0 = row0 + rowSize, Kc = 2 * rowSize;
         r.go(k_vq_tree_perturb, dim3((unsigned)((rowSize * D + VQ_THREADS - 1) / VQ_THREADS)), dim3(VQ_THREADS), 0, a, row0, rowSize);
         r.split(row0, rowSize);
         r.buckets(kid0, Kc);
         HIPCHECK(hipGetLastError());
         sz.resize((size_t)Kc);
         HIPCHECK(hipMemcpyAsync(sz.data(), a.csize + kid0, sizeof(int) * (size_t)Kc, hipMemcpyDeviceToHost, r.s));
         HIPCHECK(hipStreamSynchronize(r.s));
         iterations++;
         for (int q = 0; q < Kc && !err; q++)
            if (sz[(size_t)q] == 0) {
               htkamd_set_error("vq_cluster: SplitVectors: empty cluster %d -> %d[%d] + %d[%d]", row0 + q / 2 + 1, kid0 + (q & ~1) + 1, sz[(size_t)(q & ~1)], kid0 + (q | 1) + 1, sz[(size_t)(q | 1)]);
               err = HTKAMD_VQ_ECLUSTER;
            }
         if (err) break;
         r.centres(kid0, Kc);
         r.cov(kid0, Kc);
      }
   }
   HIPCHECK(hipGetLastError());
   HIPCHECK(tm.stop(r.s));
   if (!err) {
      if ((rc = bSize.download(out->size, (size_t)nodes, r.s)) || (rc = bCtr.download(out->centre, nCD, r.s)) || (rc = bAve.download(out->aveCost, (size_t)nodes, r.s)) ||
          (cCovLen > 0 && (rc = bCov.download(out->cov, (size_t)nodes * cCovLen, r.s))) || (out->cmap && (rc = bMap.download(out->cmap, nI, r.s))))
         return rc;
   }
   HIPCHECK(hipStreamSynchronize(r.s));
   float ms = 0.0f;
   HIPCHECK(tm.ms(&ms));
   out->numNodes = nodes; out->iterations = iterations; out->launches = r.launches; out->kernelMs = ms;
   if (err) return err;
   if (clustKind == HTKAMD_CK_FULLC) {                     // FindCovariance: CovInvert(t, c); Mat2Tri(c, t)
      std::vector<float> inv((size_t)cCovLen);
      for (int n = 0; n < nodes; n++) {
         float *tri = out->cov + (size_t)n * cCovLen;
         if (htkamd_host_cov_invert(D, tri, inv.data()) != 0) { htkamd_set_error("vq_cluster: CovInvert: [%f ...] not invertible (cluster %d)", tri[0], n + 1); return HTKAMD_VQ_EINVERT; }
         memcpy(tri, inv.data(), sizeof(float) * (size_t)cCovLen);
      }
   }
   return HTKAMD_OK;
}

// ------------------------------------------------------------------------------------------ the coder
struct VqDevStream { int n, width, covLen, col0; const int *vqidx, *left, *right; const float *gconst, *mean, *cov; };
struct VqCodeArgs { const float *X; int nFrames, nCols, kind, type; VqDevStream st[VQ_SMAX]; short *codes; int nStreams; };

// VQNodeScore: the FLOAT sum
template <int DCAP> static __device__ float vq_node_score(int kind, int D, const float (&x)[DCAP], const float *mean, const float *cov, float gconst)
{
   float sum = 0.0f;
   if (kind == HTKAMD_CK_FULLC) {
      float vx[DCAP];
#pragma unroll
      for (int d = 0; d < DCAP; d++) vx[d] = d < D ? __fsub_rn(x[d], mean[d]) : 0.0f;
#pragma unroll 1
      for (int i = 1; i < D; i++) {
         const float *row = cov + i * (i + 1) / 2;
#pragma unroll 1
         for (int j = 0; j < i; j++) sum = __fadd_rn(sum, __fmul_rn(__fmul_rn(vx[i], vx[j]), row[j]));
      }
      sum = __fmul_rn(sum, 2.0f);
#pragma unroll 1
      for (int i = 0; i < D; i++) sum = __fadd_rn(sum, __fmul_rn(__fmul_rn(vx[i], vx[i]), cov[i * (i + 1) / 2 + i]));
   } else {
#pragma unroll
      for (int d = 0; d < DCAP; d++)
         if (d < D) {
            const float df = __fsub_rn(x[d], mean[d]);
            float q = __fmul_rn(df, df);
            if (kind == HTKAMD_CK_INVDIAGC) q = __fmul_rn(q, cov[d]);
            sum = __fadd_rn(sum, q);
         }
   }
   return __fadd_rn(gconst, sum);
}

template <int DCAP> __global__ __launch_bounds__(VQ_THREADS) void k_vq_code(VqCodeArgs a)
{
   extern __shared__ float vqLds[];
   const int t = threadIdx.x, f = blockIdx.x * VQ_THREADS + t, s = blockIdx.y;
   const VqDevStream st = a.st[s];
   const int D = st.width, L = st.covLen, per = D + L + 1;
   const bool ok = f < a.nFrames;
   float x[DCAP];
   {
      const float *row = a.X + (size_t)(ok ? f : 0) * a.nCols + st.col0;
#pragma unroll
      for (int d = 0; d < DCAP; d++) x[d] = (ok && d < D) ? row[d] : 0.0f;
   }
   int idx = 0;
   if (a.type == HTKAMD_VQ_LINTREE) {
      const int cap = VQ_CODE_TILE / per;
      float bestx = 0.0f; int bestn = 0;
      for (int n0 = 0; n0 < st.n; n0 += cap) {
         const int nn = st.n - n0 < cap ? st.n - n0 : cap;
         __syncthreads();
         for (int e = t; e < nn * per; e += VQ_THREADS) {  // a node: mean [D], cov [L], gconst
            const int n = e / per, p = e - n * per;
            vqLds[e] = p < D ? st.mean[(size_t)(n0 + n) * D + p] : p < D + L ? st.cov[(size_t)(n0 + n) * L + (p - D)] : st.gconst[n0 + n];
         }
         __syncthreads();
         for (int n = 0; n < nn; n++) {
            const float *nd = vqLds + n * per;
            const float sc = vq_node_score<DCAP>(a.kind, D, x, nd, nd + D, nd[D + L]);
            if (n0 + n == 0 || sc < bestx) { bestx = sc; bestn = n0 + n; }
         }
      }
      idx = st.vqidx[bestn];
   } else {
      int n = 0;
      for (int depth = 0; depth < st.n && st.right[n] >= 0 && st.left[n] >= 0; depth++) {
         const int rn = st.right[n], ln = st.left[n];
         const float xr = vq_node_score<DCAP>(a.kind, D, x, st.mean + (size_t)rn * D, st.cov + (size_t)rn * L, st.gconst[rn]);
         const float xl = vq_node_score<DCAP>(a.kind, D, x, st.mean + (size_t)ln * D, st.cov + (size_t)ln * L, st.gconst[ln]);
         n = xr < xl ? rn : ln;
      }
      idx = st.vqidx[n];
   }
   if (ok) a.codes[(size_t)f * a.nStreams + s] = (short)idx;
}

namespace {
struct VqDev { DevBuf ints, floats; VqDevStream st[VQ_SMAX]; KernelTimer tm; };
void vq_dev_free(void *p) { delete (VqDev *)p; }

int vq_dev_make(htkamd_vqtab *t, hipStream_t s)
{
   VqDev *d = new VqDev();
   std::vector<int> ints;
   std::vector<float> fl;
   size_t io[VQ_SMAX], fo[VQ_SMAX];
   for (int k = 0; k < t->nStreams; k++) {
      const vq_stream &v = t->st[k];
      io[k] = ints.size(); fo[k] = fl.size();
      ints.insert(ints.end(), v.vqidx, v.vqidx + v.n); ints.insert(ints.end(), v.left, v.left + v.n); ints.insert(ints.end(), v.right, v.right + v.n);
      fl.insert(fl.end(), v.gconst, v.gconst + v.n); fl.insert(fl.end(), v.mean, v.mean + (size_t)v.n * v.width);
      if (v.covLen > 0) fl.insert(fl.end(), v.cov, v.cov + (size_t)v.n * v.covLen);
   }
   fl.push_back(0.0f);                                    // (a NULLC table's cov pointer stays inside the buffer)
   int rc;
   if ((rc = d->ints.upload(ints, s)) || (rc = d->floats.upload(fl, s))) { delete d; return rc; }
   hipError_t e = hipStreamSynchronize(s);                 // the vectors go out of scope
   if (e != hipSuccess) { delete d; htkamd_set_error("vq_code: %s", hipGetErrorString(e)); return HTKAMD_EHIP; }
   int col = 0;
   for (int k = 0; k < t->nStreams; k++) {
      const vq_stream &v = t->st[k];
      VqDevStream &o = d->st[k];
      o.n = v.n; o.width = v.width; o.covLen = v.covLen; o.col0 = col; col += v.width;
      o.vqidx = d->ints.as<const int>() + io[k]; o.left = o.vqidx + v.n; o.right = o.left + v.n;
      o.gconst = d->floats.as<const float>() + fo[k]; o.mean = o.gconst + v.n; o.cov = o.mean + (size_t)v.n * v.width;
   }
   t->dev = d; t->devFree = vq_dev_free;
   return HTKAMD_OK;
}
}

extern "C" double htkamd_vq_code_last_kernel_ms(const htkamd_vqtab *t) { return t ? t->codeMs : 0.0; }

extern "C" int htkamd_vq_code(htkamd_vqtab *t, const float *dX, int nUtt, const int *frameOff, int nCols, short *codes, void *stream)
{
   if (!t || !dX || nUtt < 0 || !frameOff || !codes || nCols < 1) { htkamd_set_error("vq_code: bad argument"); return HTKAMD_EINVAL; }
   if (frameOff[0] != 0) { htkamd_set_error("vq_code: the first utterance starts at frame %d", frameOff[0]); return HTKAMD_EINVAL; }
   for (int u = 0; u < nUtt; u++) if (frameOff[u + 1] < frameOff[u]) { htkamd_set_error("vq_code: utterance %d has a negative length", u); return HTKAMD_EINVAL; }
   if (t->kind != HTKAMD_CK_NULLC && t->kind != HTKAMD_CK_INVDIAGC && t->kind != HTKAMD_CK_FULLC) { htkamd_set_error("vq_code: VQNodeScore: bad kind %d", t->kind); return HTKAMD_VQ_ETABKIND; }
   int sum = 0, maxW = 0;
   for (int k = 0; k < t->nStreams; k++) {
      const vq_stream &v = t->st[k];
      if (v.n < 1) { htkamd_set_error("vq_code: GetVQ: null tree in stream %d", k + 1); return HTKAMD_EINVAL; }
      if (v.width > VQ_MAX_D) { htkamd_set_error("vq_code: stream %d has %d values (the library's maximum is %d)", k + 1, v.width, VQ_MAX_D); return HTKAMD_EINVAL; }
      if (v.width + v.covLen + 1 > VQ_CODE_TILE) { htkamd_set_error("vq_code: a node of stream %d does not fit the workgroup's LDS", k + 1); return HTKAMD_EINVAL; }
      sum += v.width; if (v.width > maxW) maxW = v.width;
   }
   if (sum != nCols) { htkamd_set_error("vq_code: GetVQ: the streams' widths add up to %d, the data has %d columns", sum, nCols); return HTKAMD_EINVAL; }
   const int nFrames = frameOff[nUtt];
   if (nFrames == 0) return HTKAMD_OK;
   if (htkamd_device_count() <= 0) { htkamd_set_error("vq_code: no HIP device"); return HTKAMD_ENODEV; }
   hipStream_t s = (hipStream_t)stream;
   int rc;
   if (!t->dev && (rc = vq_dev_make(t, s))) return rc;
   VqDev *d = (VqDev *)t->dev;
   DevBuf bCodes;
   const size_t nOut = (size_t)nFrames * t->nStreams;
   if ((rc = bCodes.reserve<short>(nOut))) return rc;
   VqCodeArgs a;
   memset(&a, 0, sizeof(a));
   a.X = dX; a.nFrames = nFrames; a.nCols = nCols; a.kind = t->kind; a.type = t->type; a.nStreams = t->nStreams; a.codes = bCodes.as<short>();
   for (int k = 0; k < t->nStreams; k++) a.st[k] = d->st[k];
   const dim3 grid((unsigned)((nFrames + VQ_THREADS - 1) / VQ_THREADS), (unsigned)t->nStreams), block(VQ_THREADS);
   const size_t lds = sizeof(float) * VQ_CODE_TILE;
   HIPCHECK(d->tm.start(s));
   if (maxW <= 16) hipLaunchKernelGGL(k_vq_code<16>, grid, block, lds, s, a);
   else if (maxW <= 40) hipLaunchKernelGGL(k_vq_code<40>, grid, block, lds, s, a);
   else hipLaunchKernelGGL(k_vq_code<VQ_MAX_D>, grid, block, lds, s, a);
   HIPCHECK(hipGetLastError());
   HIPCHECK(d->tm.stop(s));
   if ((rc = bCodes.download(codes, nOut, s))) return rc;
   HIPCHECK(hipStreamSynchronize(s));
   float ms = 0.0f;
   HIPCHECK(d->tm.ms(&ms));
   t->codeMs = ms;
   return HTKAMD_OK;
}
