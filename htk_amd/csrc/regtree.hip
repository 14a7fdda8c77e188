// regtree.hip -- the device side of regression class trees (HHEd's RC command; the driver is host/regtree.c).
//
// The set's Gaussians ("members", in the order InitRegTree's scan meets them) stay on the device for the whole command: their means and
// the AccSum rows (occupation-scaled mean, mean^2 + variance, occupation).  A node is a range of the member list.  One launch of
// k_rt_split, ONE workgroup, does a whole ClusterChildren (HHEd.c:5961) for a node:
//
//   distances   CalcDistance's (:5863) two Distance calls (:5657) per member, a thread per member: float differences, squares and sums
//               in the order k = 1..D, the square root of the double, rounded to float.  score1 < score2 sends the member left, anything
//               else (a tie, a NaN) right.  Nothing here depends on another member.
//   centroids   sum1 / sum2, clustAcc and clusterScore are float sums over the members IN LIST ORDER, and the next assignment depends on
//               their bits: lane k < D walks the list for dimension k, one further lane (the first of the next wavefront, so that its walk
//               does not serialise with the dimension lanes') walks it for both occupations and both scores.  The flags and the products
//               occ * score come from the distance step.  Sixteen members' loads are issued before their adds; the adds stay in order.
//   loop        oldDistance - newDistance > thresh, capped by MAX_ITER, decided by every thread from the same LDS words: no host round
//               trip and no device-wide flag -- the workgroup is the loop.
//   partition   CreateChildNodes (:5912): the distances once more against the final centroids, a ballot prefix sum over the flags, the
//               left members then the right members written behind one another in their old order.
//   children    CalcClusterDistribution (:5692) and CalcNodeScore (:5673) of both children, again as ordered walks.
//
// A member without an AccSum record (no occupation in the statistics) takes part in the assignment and the partition and in no sum.
// k_rt_node is the children step alone, for InitRegTree's root nodes.  -ffp-contract=off: nothing is fused.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "internal.h"
#include "hipcheck.h"
#include "devbuf.h"

#define RT_THREADS 1024
#define RT_WAVES   (RT_THREADS / 64)
#define RT_AHEAD   16

struct RtSet { const float *mean, *sum, *sqr, *occ; const unsigned char *has; int D; };

// Distance (:5657)
static __device__ __forceinline__ float rt_distance(const float *m, const float *c, int D)
{
   float dist = 0.0f;
   for (int k = 0; k < D; k++) {
      float x = __fsub_rn(m[k], c[k]);
      x = __fmul_rn(x, x);
      dist = __fadd_rn(dist, x);
   }
   return (float)__dsqrt_rn((double)dist);
}

// flag[i]: bit 0 = right child, bit 1 = no AccSum record; val[i] = occ * the smaller score (CalcDistance's addend)
static __device__ void rt_assign(const RtSet &S, const int *L, int n, const float *cen, unsigned char *flag, float *val)
{
   for (int i = threadIdx.x; i < n; i += RT_THREADS) {
      const int id = L[i];
      const float *m = S.mean + (size_t)id * S.D;
      const float s1 = rt_distance(m, cen, S.D), s2 = rt_distance(m, cen + S.D, S.D);
      const int right = !(s1 < s2);
      flag[i] = (unsigned char)(right | (S.has[id] ? 0 : 2));
      val[i] = __fmul_rn(S.occ[id], right ? s2 : s1);
   }
}

// an ordered add into one of two sums, without a branch: f == 0 the left child's, f == 1 the right child's, else (no AccSum record) neither
static __device__ __forceinline__ void rt_add2(float &s1, float &s2, int f, float v)
{
   const float n1 = __fadd_rn(s1, v), n2 = __fadd_rn(s2, v);
   s1 = f == 0 ? n1 : s1; s2 = f == 1 ? n2 : s2;
}

// lane k of CalcDistance's loop: sum1[k] / sum2[k] over the members in list order
static __device__ __forceinline__ float2 rt_walk_sums(const float *col, int D, const int *L, const unsigned char *flag, int n)
{
   float s1 = 0.0f, s2 = 0.0f;
   int i = 0;
   for (; i + RT_AHEAD <= n; i += RT_AHEAD) {
      float v[RT_AHEAD]; int f[RT_AHEAD];
#pragma unroll
      for (int u = 0; u < RT_AHEAD; u++) { f[u] = flag[i + u]; v[u] = col[(size_t)L[i + u] * D]; }
#pragma unroll
      for (int u = 0; u < RT_AHEAD; u++) rt_add2(s1, s2, f[u], v[u]);
   }
   for (; i < n; i++) rt_add2(s1, s2, flag[i], col[(size_t)L[i] * D]);
   return make_float2(s1, s2);
}

// the same walk for clustAcc and clusterScore of both children: st[0], st[1] occupations, st[2], st[3] scores
static __device__ __forceinline__ void rt_walk_occ(const float *occ, const int *L, const unsigned char *flag, const float *val, int n, float *st)
{
   float a1 = 0.0f, a2 = 0.0f, c1 = 0.0f, c2 = 0.0f;
   int i = 0;
   for (; i + RT_AHEAD <= n; i += RT_AHEAD) {
      float o[RT_AHEAD], v[RT_AHEAD]; int f[RT_AHEAD];
#pragma unroll
      for (int u = 0; u < RT_AHEAD; u++) { f[u] = flag[i + u]; o[u] = occ[L[i + u]]; v[u] = val[i + u]; }
#pragma unroll
      for (int u = 0; u < RT_AHEAD; u++) { rt_add2(a1, a2, f[u], o[u]); rt_add2(c1, c2, f[u], v[u]); }
   }
   for (; i < n; i++) { const int f = flag[i]; rt_add2(a1, a2, f, occ[L[i]]); rt_add2(c1, c2, f, val[i]); }
   st[0] = a1; st[1] = a2; st[2] = c1; st[3] = c2;
}

// one lane's float sum, in list order, over the members that have an AccSum record: of val[i], or of the occupations when val is NULL
static __device__ float rt_walk_has(const RtSet &S, const int *L, int n, const float *val)
{
   float s = 0.0f;
   int i = 0;
   for (; i + RT_AHEAD <= n; i += RT_AHEAD) {
      float v[RT_AHEAD]; int h[RT_AHEAD];
#pragma unroll
      for (int u = 0; u < RT_AHEAD; u++) { const int id = L[i + u]; h[u] = S.has[id]; v[u] = val ? val[i + u] : S.occ[id]; }
#pragma unroll
      for (int u = 0; u < RT_AHEAD; u++) if (h[u]) s = __fadd_rn(s, v[u]);
   }
   for (; i < n; i++) { const int id = L[i]; if (S.has[id]) s = __fadd_rn(s, val ? val[i] : S.occ[id]); }
   return s;
}

// CalcClusterDistribution (:5692) and CalcNodeScore (:5673) of the node L[0 .. n): out[2D+2].  ave: D floats of LDS, st: 2 floats of LDS.
// Called by the whole workgroup; ends on a barrier.
static __device__ void rt_node(const RtSet &S, const int *L, int n, float *val, float *ave, float *st, float *out)
{
   const int t = threadIdx.x, D = S.D, occLane = (D + 63) & ~63;
   float sum = 0.0f, sqr = 0.0f;
   if (t < D) {
      int i = 0;
      for (; i + RT_AHEAD <= n; i += RT_AHEAD) {
         float a[RT_AHEAD], b[RT_AHEAD]; int h[RT_AHEAD];
#pragma unroll
         for (int u = 0; u < RT_AHEAD; u++) { const int id = L[i + u]; h[u] = S.has[id]; a[u] = S.sum[(size_t)id * D + t]; b[u] = S.sqr[(size_t)id * D + t]; }
#pragma unroll
         for (int u = 0; u < RT_AHEAD; u++) if (h[u]) { sum = __fadd_rn(sum, a[u]); sqr = __fadd_rn(sqr, b[u]); }
      }
      for (; i < n; i++) { const int id = L[i]; if (S.has[id]) { sum = __fadd_rn(sum, S.sum[(size_t)id * D + t]); sqr = __fadd_rn(sqr, S.sqr[(size_t)id * D + t]); } }
   } else if (t == occLane) {
      st[0] = rt_walk_has(S, L, n, nullptr);
   }
   __syncthreads();
   const float occ = st[0];
   if (t < D) {
      const float mean = __fdiv_rn(sum, occ);
      ave[t] = mean; out[t] = mean;
      out[D + t] = __fdiv_rn(__fsub_rn(sqr, __fdiv_rn(__fmul_rn(sum, sum), occ)), occ);
   }
   __syncthreads();
   for (int i = t; i < n; i += RT_THREADS) { const int id = L[i]; val[i] = __fmul_rn(rt_distance(S.mean + (size_t)id * D, ave, D), S.occ[id]); }
   __syncthreads();
   if (t == 0) {
      out[2 * D] = occ; out[2 * D + 1] = rt_walk_has(S, L, n, val);
   }
   __syncthreads();
}

__global__ __launch_bounds__(RT_THREADS) void k_rt_node(RtSet S, const int *list, float *val, int off, int n, float *out)
{
   extern __shared__ float lds[];
   rt_node(S, list + off, n, val + off, lds, lds + S.D, out);
}

__global__ __launch_bounds__(RT_THREADS) void k_rt_split(RtSet S, int *list, int *tmp, unsigned char *flagAll, float *valAll, int off, int n, const float *seeds,
                                                          int *outI, float *outF)
{
   extern __shared__ float lds[];
   __shared__ int cnt[RT_WAVES], nLeftS;
   const int t = threadIdx.x, D = S.D, occLane = (D + 63) & ~63;
   float *cen = lds, *st = lds + 2 * D, *ave = lds + 2 * D + 4;
   int *L = list + off, *T = tmp + off;
   unsigned char *flag = flagAll + off;
   float *val = valAll + off;
   for (int k = t; k < 2 * D; k += RT_THREADS) cen[k] = seeds[k];
   if (t == 0) nLeftS = 0;
   __syncthreads();
   // ClusterChildren's loop
   const float thresh = 1.0e-12f;
   int iter = 0, calls = 0;
   float oldDistance, newDistance = 0.0f;
   for (;;) {
      iter++;
      if (iter >= HTKAMD_RT_MAXITER) break;
      rt_assign(S, L, n, cen, flag, val);
      calls++;
      __syncthreads();
      float2 s12 = make_float2(0.0f, 0.0f);
      if (t < D) s12 = rt_walk_sums(S.sum + t, D, L, flag, n);
      else if (t == occLane) rt_walk_occ(S.occ, L, flag, val, n, st);
      __syncthreads();
      if (t < D) { cen[t] = __fdiv_rn(s12.x, st[0]); cen[D + t] = __fdiv_rn(s12.y, st[1]); }
      const float d = __fdiv_rn(__fadd_rn(st[2], st[3]), __fadd_rn(st[0], st[1]));
      oldDistance = iter == 1 ? __fadd_rn(__fadd_rn(d, thresh), 1.0f) : newDistance;
      newDistance = d;
      __syncthreads();
      if (!(__fsub_rn(oldDistance, newDistance) > thresh)) break;
   }
   // CreateChildNodes: the assignment against the final centroids, then the stable partition
   rt_assign(S, L, n, cen, flag, val);
   __syncthreads();
   {
      int c = 0;
      for (int i = t; i < n; i += RT_THREADS) c += !(flag[i] & 1);
      for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
      if ((t & 63) == 0 && c) atomicAdd(&nLeftS, c);
   }
   __syncthreads();
   const int nLeft = nLeftS;
   int baseL = 0;
   for (int base = 0; base < n; base += RT_THREADS) {
      const int i = base + t, lane = t & 63, w = t >> 6;
      const bool valid = i < n, isL = valid && !(flag[i] & 1);
      const unsigned long long b = __ballot(isL);
      const int rank = __popcll(b & ((1ull << lane) - 1ull));
      if (lane == 0) cnt[w] = __popcll(b);
      __syncthreads();
      int pre = 0, tot = 0;
#pragma unroll
      for (int k = 0; k < RT_WAVES; k++) { const int c = cnt[k]; tot += c; if (k < w) pre += c; }
      const int before = baseL + pre + rank;                                  // the left members before this one
      if (valid) T[isL ? before : nLeft + (i - before)] = L[i];
      baseL += tot;
      __syncthreads();
   }
   for (int i = t; i < n; i += RT_THREADS) L[i] = T[i];
   if (t == 0) { outI[0] = nLeft; outI[1] = n - nLeft; outI[2] = calls; }
   __syncthreads();
   rt_node(S, L, nLeft, val, ave, st, outF);
   rt_node(S, L + nLeft, n - nLeft, val + nLeft, ave, st, outF + 2 * D + 2);
}

// ------------------------------------------------------------------------------------------ host side of the device
DEVBUF_OWNER("regtree")

struct htkamd_rt_dev {
   DevBuf mean, sum, sqr, occ, has, list, tmp, flag, val, seeds, outI, outF;
   int G = 0, D = 0;
   hipStream_t st = nullptr;
   KernelTimer timer;
   float ms = 0.0f;
};

static RtSet rt_set(const htkamd_rt_dev *t)
{
   RtSet S;
   S.mean = t->mean.as<const float>(); S.sum = t->sum.as<const float>(); S.sqr = t->sqr.as<const float>(); S.occ = t->occ.as<const float>();
   S.has = t->has.as<const unsigned char>(); S.D = t->D;
   return S;
}

extern "C" int htkamd_rt_dev_open(htkamd_rt_dev **out, const float *mean, const float *sum, const float *sqr, const float *occ, const unsigned char *hasAcc,
                                  int G, int D, void *stream)
{
   if (!out || !mean || !sum || !sqr || !occ || !hasAcc || G < 1 || D < 1 || D > HTKAMD_RT_MAXDIM) { htkamd_set_error("regtree: bad argument"); return HTKAMD_EINVAL; }
   if (htkamd_device_count() <= 0) { htkamd_set_error("regtree: no HIP device"); return HTKAMD_ENODEV; }
   htkamd_rt_dev *t = new htkamd_rt_dev();
   t->G = G; t->D = D; t->st = (hipStream_t)stream;
   const size_t nG = (size_t)G, rows = nG * D;
   std::vector<int> ident(nG);
   for (int i = 0; i < G; i++) ident[i] = i;
   int rc = t->mean.upload(mean, rows, t->st);
   if (!rc) rc = t->sum.upload(sum, rows, t->st);
   if (!rc) rc = t->sqr.upload(sqr, rows, t->st);
   if (!rc) rc = t->occ.upload(occ, nG, t->st);
   if (!rc) rc = t->has.upload(hasAcc, nG, t->st);
   if (!rc) rc = t->list.upload(ident, t->st);
   if (!rc) rc = t->tmp.reserve<int>(nG);
   if (!rc) rc = t->flag.reserve<unsigned char>(nG);
   if (!rc) rc = t->val.reserve<float>(nG);
   if (!rc) rc = t->seeds.reserve<float>(2 * (size_t)D);
   if (!rc) rc = t->outI.reserve<int>(4);
   if (!rc) rc = t->outF.reserve<float>(2 * (2 * (size_t)D + 2));
   HIPCHECK_RC(rc, devOwner, hipStreamSynchronize(t->st));
   if (rc) { htkamd_rt_dev_close(t); return rc; }
   *out = t;
   return HTKAMD_OK;
}

// one launch between the timer's two events; its time is added once its figures are fetched
template <typename Launch> static int rt_timed(htkamd_rt_dev *t, Launch launch)
{
   int rc = HTKAMD_OK;
   HIPCHECK_RC(rc, devOwner, t->timer.start(t->st));
   if (!rc) launch();
   HIPCHECK_RC(rc, devOwner, hipGetLastError());
   HIPCHECK_RC(rc, devOwner, t->timer.stop(t->st));
   return rc;
}
static int rt_elapsed(htkamd_rt_dev *t)
{
   int rc = HTKAMD_OK; float ms = 0.0f;
   HIPCHECK_RC(rc, devOwner, hipStreamSynchronize(t->st));
   HIPCHECK_RC(rc, devOwner, t->timer.ms(&ms));
   if (!rc) t->ms += ms;
   return rc;
}

extern "C" int htkamd_rt_dev_node(htkamd_rt_dev *t, int off, int n, float *node)
{
   if (!t || !node || off < 0 || n < 0 || (long long)off + n > t->G) { htkamd_set_error("regtree: node range %d + %d of %d members", off, n, t ? t->G : 0); return HTKAMD_EINVAL; }
   const int D = t->D;
   int rc = rt_timed(t, [&] {
      hipLaunchKernelGGL(k_rt_node, dim3(1), dim3(RT_THREADS), sizeof(float) * ((size_t)D + 2), t->st, rt_set(t), t->list.as<const int>(), t->val.as<float>(), off, n, t->outF.as<float>());
   });
   if (!rc) rc = t->outF.download(node, 2 * (size_t)D + 2, t->st);
   if (!rc) rc = rt_elapsed(t);
   return rc;
}

extern "C" int htkamd_rt_dev_split(htkamd_rt_dev *t, int off, int n, const float *seeds, int *counts, float *nodes)
{
   if (!t || !seeds || !counts || !nodes || off < 0 || n < 1 || (long long)off + n > t->G) { htkamd_set_error("regtree: split range %d + %d of %d members", off, n, t ? t->G : 0); return HTKAMD_EINVAL; }
   const int D = t->D;
   int rc = t->seeds.upload(seeds, 2 * (size_t)D, t->st);
   if (!rc) rc = rt_timed(t, [&] {
      hipLaunchKernelGGL(k_rt_split, dim3(1), dim3(RT_THREADS), sizeof(float) * (3 * (size_t)D + 6), t->st, rt_set(t), t->list.as<int>(), t->tmp.as<int>(), t->flag.as<unsigned char>(),
                         t->val.as<float>(), off, n, t->seeds.as<const float>(), t->outI.as<int>(), t->outF.as<float>());
   });
   if (!rc) rc = t->outI.download(counts, 3, t->st);
   if (!rc) rc = t->outF.download(nodes, 2 * (2 * (size_t)D + 2), t->st);
   if (!rc) rc = rt_elapsed(t);
   if (!rc && (counts[0] < 0 || counts[1] < 0 || counts[0] + counts[1] != n)) { htkamd_set_error("regtree: a split of %d members came back as %d + %d", n, counts[0], counts[1]); rc = HTKAMD_EHIP; }
   return rc;
}

extern "C" int htkamd_rt_dev_list(htkamd_rt_dev *t, int *list)
{
   if (!t || !list) { htkamd_set_error("regtree: bad argument"); return HTKAMD_EINVAL; }
   int rc = t->list.download(list, (size_t)t->G, t->st);
   HIPCHECK_RC(rc, devOwner, hipStreamSynchronize(t->st));
   return rc;
}

// Test aid: the device steps alone over a caller's member arrays, in order on one htkamd_rt_dev, so a later step sees the list as the
// earlier splits left it.  Step s is steps[3s .. 3s+3) = (kind, off, n): kind 0 a node step (figures[s][0] is written), kind 1 a split
// with the seeds seeds[s][2][D] (counts[s][3] and figures[s][2] are written).  What a step does not write stays as the caller left it.
extern "C" int htkamd_regtree_probe(const float *mean, const float *sum, const float *sqr, const float *occ, const unsigned char *hasAcc, int G, int D,
                                    const int *steps, const float *seeds, int nSteps, int *counts, float *figures, int *list, void *stream)
{
   if (!steps || !seeds || !counts || !figures || !list || nSteps < 0) { htkamd_set_error("regtree_probe: bad argument"); return HTKAMD_EINVAL; }
   for (int s = 0; s < nSteps; s++)
      if (steps[3 * s] != 0 && steps[3 * s] != 1) { htkamd_set_error("regtree_probe: step %d is of kind %d (0: node, 1: split)", s, steps[3 * s]); return HTKAMD_EINVAL; }
   htkamd_rt_dev *t = nullptr;
   int rc = htkamd_rt_dev_open(&t, mean, sum, sqr, occ, hasAcc, G, D, stream);
   if (rc) return rc;
   const size_t C = 2 * (size_t)D + 2;
   for (int s = 0; s < nSteps && !rc; s++) {
      const int off = steps[3 * s + 1], n = steps[3 * s + 2];
      if (steps[3 * s]) rc = htkamd_rt_dev_split(t, off, n, seeds + (size_t)s * 2 * D, counts + 3 * (size_t)s, figures + (size_t)s * 2 * C);
      else rc = htkamd_rt_dev_node(t, off, n, figures + (size_t)s * 2 * C);
   }
   if (!rc) rc = htkamd_rt_dev_list(t, list);
   htkamd_rt_dev_close(t);
   return rc;
}

extern "C" float htkamd_rt_dev_kernel_ms(const htkamd_rt_dev *t) { return t ? t->ms : 0.0f; }

extern "C" void htkamd_rt_dev_close(htkamd_rt_dev *t) { delete t; }
