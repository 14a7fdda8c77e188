// fb_mixwide.hip -- K4s-x: the mixture statistics bucketed by tied state (K4s, k_mixstate in fb_kernels.hip) for ANY vector size up to
// 128 and ANY number of components per state.  UpMixParms HFB.c:1573-1721, one stream, DIAGC, left-to-right path.
//
// k_mixstate holds a state's 16 components in one wavefront's lanes and a dimension per lane, for D = 13 / 26 / 39 as a template
// argument.  Nothing in that split needs those sizes: a component's posterior x = seed + log w + prob does not look at the other
// components of its state, and the sums are per (Gaussian, dimension).  So here
//   * the grid is (tied state of the range, part of MSX_CAP pairs, TILE of 16 components): a tile needs nothing from the other tiles
//     of its state, and a large mixture costs more workgroups, not more registers;
//   * a workgroup is W wavefronts, W = 1 for D <= 64 and 2 for D <= 128: in the sum phase a THREAD is a dimension, so the running sums
//     stay at 16 x 2 doubles per thread as in k_mixstate (two dimensions per lane would be 128 registers of sums: one wavefront per SIMD);
//   * D is a run-time number: the tile's parameters lie in LDS as (mean d, mean d+1, 1/var d, 1/var d+1) per component and pair of
//     dimensions, read 16 components wide and broadcast to the lane groups, the chunk's feature rows beside them.
// LDS is sized by the launcher from D (msx_lds_bytes): 256 (D+1)/2 + 128 XS + 4 352 (+ 144 for W = 2) bytes, XS = D rounded up to 4 --
// 13.5 KB at D = 36, 20.4 KB at D = 64, 36.4 KB at D = 128 (four workgroups = eight wavefronts per CU at the cap).
// The matrix pipe has no place here: z = x - mean depends on the component (no shared operand), the reference rounds z L to float
// before it is summed, and ~4 of 16 components survive a pair, so a dense product would be three quarters zeros.
#include <hip/hip_runtime.h>
#include "internal.h"
#include "hipcheck.h"
#include "kernels.h"

#define MSX_CHUNK 32             /* pairs per chunk, as k_mixstate's MS_CHUNK */
#define MSX_CAP 128              /* pairs per part of a state, as k_mixstate's MS_CAP: the counts and ranges mean the same for both kernels */
#define MSX_PARTS 4
#define MSX_GS 16                /* components per tile = lanes per lane group */

static size_t msx_lds_bytes(int D, int W)
{
   const size_t NQ = (size_t)(D + 1) / 2, XS = ((size_t)D + 3) & ~(size_t)3;
   return NQ * MSX_GS * sizeof(float4) + sizeof(double) * (MSX_CHUNK * MSX_GS + MSX_CHUNK + (W > 1 ? MSX_GS + 2 : 0)) + sizeof(float) * MSX_CHUNK * XS;
}

template <int W, int MODE>       // MODE: 3 means and variances (HFB.c:1673-1678), 1 means only (:1697), 2 variances only (:1706), 0 weights only
__global__ __launch_bounds__(64 * W) void k_mixstate_x(FbArgs a)
{
   constexpr int GS = MSX_GS, CH = MSX_CHUNK, HPR = 4 * W;      // HPR: pairs per round of the posterior phase (a lane group each)
   constexpr bool upMu = (MODE & 1) != 0, upVa = (MODE & 2) != 0;
   const int st = a.stBase + blockIdx.x, part = blockIdx.y, tile = blockIdx.z;
   const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), grp = lane / GS, sub = lane % GS;
   const int D = a.D, NQ = (D + 1) >> 1, XS = (D + 3) & ~3;
   const int nst = a.stCnt[st] < a.stCap ? a.stCnt[st] : a.stCap;
   const int r0 = part * MSX_CAP, r1 = (part == (int)gridDim.y - 1 || r0 + MSX_CAP > nst) ? nst : r0 + MSX_CAP;      // the last part takes what is left
   const int cS = a.stateCompOff[st], MS = a.stateCompOff[st + 1] - cS;
   const int c0 = cS + tile * GS, M = (MS - tile * GS < GS) ? MS - tile * GS : GS;      // this tile's components
   if (r0 >= nst || M <= 0) return;                      // an empty part or tile: before anything touches LDS
   const HitS *bucket = a.stBucket + (size_t)st * a.stCap;
   const bool single = (MS == 1 || a.maxM == 1);
   const bool upWt = a.uFlags & HTKAMD_UPMIXES;

   extern __shared__ float4 msxLds[];
   float4 *pl = msxLds;                                  // [NQ][GS]: (mean d, mean d+1, 1/var d, 1/var d+1) of component `sub`, d = 2q
   double *Lt = (double *)(pl + (size_t)NQ * GS);        // [CH][GS]: the chunk's posteriors
   double *hSeed = Lt + CH * GS;                         // [CH]
   double *red = hSeed + CH;                             // W = 2: [GS] the second wavefront's weight sums, [1] its triples
   float *xs = (float *)(red + (W > 1 ? GS + 2 : 0));    // [CH][XS]: the chunk's feature rows

   int g = 0;
   float wt = 0.0f, gcst = 0.0f;
   if (sub < M) {
      g = a.compGauss[c0 + sub];
      wt = a.compLogWt[c0 + sub];
      const float *P = a.gparam + (size_t)g * a.PS;
      gcst = P[2 * D];
      // (rows are PS = 4k floats long and 16-byte aligned, the padding behind gConst zeros: the last word of an odd D holds gConst where a
      //  mean would be -- the posterior loop below never reads that half); the words of a row split between the workgroup's lane groups
      const float4 *P4 = (const float4 *)P;
      for (int q = wv * 4 + grp; q < NQ; q += HPR) { const float4 pv = P4[q]; pl[q * GS + sub] = make_float4(pv.x, pv.z, pv.y, pv.w); }
   }
   // second view: thread = dimension; the means of the tile's Gaussians at that dimension (their numbers by one load, a lane each)
   const int dim = tid < D ? tid : 0;
   const int gOfLane = (lane < M) ? a.compGauss[c0 + lane] : 0;
   float meanR[GS];
#pragma unroll
   for (int m = 0; m < GS; m++) { const int gm = __builtin_amdgcn_readlane(gOfLane, m); meanR[m] = (m < M && tid < D) ? a.mean[(size_t)gm * D + dim] : 0.0f; }
   double sMu[GS], sVa[GS];
#pragma unroll
   for (int m = 0; m < GS; m++) { sMu[m] = 0.0; sVa[m] = 0.0; }
   double wtAcc = 0.0;                                   // posteriors of the lane's component over the pairs of its lane group
   int nTriples = 0;
   const double minF = uniform_f64((double)a.minFrwdP);

   for (int base = r0; base < r1; base += CH) {
      const int n = (r1 - base < CH) ? r1 - base : CH;
      __syncthreads();
      // every wavefront reads the chunk's bucket entries itself (its own copy of the frame numbers: no LDS round trip in front of the loads)
      int hfr = 0;
      if (lane < n) { const HitS h = bucket[base + lane]; hfr = h.frame; if (wv == 0) hSeed[lane] = h.seed; }
      // the rows by LDS-DMA, split between the wavefronts; 64 floats per load instruction, so a row of D > 64 takes two
      for (int r = wv; r < n; r += W) {
         const int fr = __builtin_amdgcn_readlane(hfr, r);
         const float *src = a.X + (size_t)fr * D;
#pragma unroll
         for (int k0 = 0; k0 < 64 * W; k0 += 64)
            if (k0 + lane < D)
               __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + k0 + lane),
                                                (__attribute__((address_space(3))) void *)(xs + r * XS + k0), 4, 0, 0);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      // ---- the posteriors of the chunk: lane group = pair, lane in the group = component of the tile (HFB.c:1581-1606)
      for (int it = 0; it * HPR < n; it++) {
         const int h = it * HPR + wv * 4 + grp;
         const bool have = h < n;
         bool pass = false;
         double Lr = 0.0;
         if (have && sub < M) {
            const double seed = hSeed[h];
            if (single) { pass = true; Lr = exp(seed); }
            else if (wt > (float)LMINMIX) {
               typedef float v2f __attribute__((ext_vector_type(2)));
               const v2f *xr = (const v2f *)(xs + h * XS);
               const float4 *pc = pl + sub;
               float sum = gcst;
               const int nFull = D >> 1;
#pragma unroll 4
               for (int q = 0; q < nFull; q++) {            // the reference's sum, a dimension after the other (HModel.c:5420-5431); the products two at a time
                  const float4 pv = pc[q * GS];
                  const v2f xv = xr[q];
                  v2f mu; mu[0] = pv.x; mu[1] = pv.y;
                  v2f iv; iv[0] = pv.z; iv[1] = pv.w;
                  const v2f xmm = xv - mu;
                  const v2f tt = xmm * xmm * iv;
                  sum += tt[0];
                  sum += tt[1];
               }
               if (D & 1) { const float4 pv = pc[nFull * GS]; const float xmm = xs[h * XS + D - 1] - pv.x; sum += xmm * xmm * pv.z; }
               const float prob = -0.5f * sum;
               const double x = (seed + (double)wt) + (double)prob;
               if (-x < minF) { pass = true; Lr = a.fastMath ? (double)__builtin_amdgcn_exp2f((float)x * 1.44269504088896341f) : exp(x); }
            }
         }
         if (have) Lt[h * GS + sub] = pass ? Lr : 0.0;
         wtAcc += pass ? Lr : 0.0;
         nTriples += pass ? 1 : 0;
      }
      __syncthreads();
      // ---- first- and second-order sums of the chunk: thread = dimension, a Gaussian after the other, the pairs it survived in (HFB.c:1673-1709)
      if (upMu || upVa) {
         unsigned long long bmAll[GS];                   // (every wavefront takes the same sixteen ballots: n <= 32 pairs, a lane each)
#pragma unroll
         for (int m4 = 0; m4 < GS; m4 += 4) {
            double Lq[4];
#pragma unroll
            for (int i = 0; i < 4; i++) Lq[i] = (lane < n) ? Lt[lane * GS + m4 + i] : 0.0;
#pragma unroll
            for (int i = 0; i < 4; i++) bmAll[m4 + i] = __ballot(Lq[i] != 0.0);
         }
         const float *xcol = xs + dim;
#pragma unroll
         for (int m = 0; m < GS; m++) {
            if (m < M) {
               unsigned long long bm = bmAll[m];
               double mu = sMu[m], va = sVa[m];            // (two scalars around the loop and no branch inside it, as in k_mixstate)
               const float mean = meanR[m];
               while (bm) {                                  // four pairs' operands requested together; an empty slot adds zeros
                  double Lv[4]; float xv[4];
#pragma unroll
                  for (int i = 0; i < 4; i++) {
                     const bool live = bm != 0;
                     const int h = live ? (int)__builtin_ctzll(bm) : 0;
                     bm &= bm - 1;
                     Lv[i] = live ? Lt[h * GS + m] : 0.0;
                     xv[i] = xcol[h * XS];
                  }
#pragma unroll
                  for (int i = 0; i < 4; i++) {
                     const double L = Lv[i];
                     const float z = xv[i] - mean;
                     if constexpr (upMu && upVa) { const float zl = (float)((double)z * L); mu += (double)zl; va += (double)(z * zl); }
                     else if constexpr (upMu) mu += (double)z * L;
                     else va += (double)(z * z) * L;
                  }
               }
               sMu[m] = mu; sVa[m] = va;
            }
         }
      }
   }
   // ---- out: one atomic per accumulator element of the tile's Gaussians and per component; the state's cells once per workgroup
#pragma unroll
   for (int m = 0; m < GS; m++) {
      if (m < M && tid < D) {
         const int gm = __builtin_amdgcn_readlane(gOfLane, m);
         if (upMu && sMu[m] != 0.0) atomicAdd(a.acc + a.lay.mu + (size_t)gm * D + tid, sMu[m]);
         if (upVa && sVa[m] != 0.0) atomicAdd(a.acc + a.lay.va + (size_t)gm * D + tid, sVa[m]);
      }
   }
   double w = wtAcc;
   w += __shfl_xor(w, 16); w += __shfl_xor(w, 32);       // the four lane groups' shares of the component
#pragma unroll
   for (int o = 32; o > 0; o >>= 1) nTriples += __shfl_xor(nTriples, o);
   if constexpr (W > 1) {                                 // ... and the second wavefront's, through LDS
      if (wv == 1 && grp == 0) red[sub] = w;
      if (wv == 1 && lane == 0) red[GS] = (double)nTriples;
      __syncthreads();
      if (wv != 0) return;
      w += red[sub];
      nTriples += (int)red[GS];
   }
   if (grp == 0 && sub < M && w != 0.0) {
      if (upWt) atomicAdd(a.acc + a.lay.wt + c0 + sub, w);
      if (upMu) atomicAdd(a.acc + a.lay.muOcc + g, w);
      if (upVa) atomicAdd(a.acc + a.lay.vaOcc + g, w);
   }
   // the state's counts in its own two cells (htkamd_fb_mix_counts sums them): the pairs once, the triples a workgroup's share at a time
   if (lane == 0) { if (part == 0 && tile == 0) a.stCnt[a.nTiedStates + 4 + 2 * st] = nst; atomicAdd(a.stCnt + a.nTiedStates + 5 + 2 * st, nTriples); }
   double so = (sub < M) ? w : 0.0;
#pragma unroll
   for (int o = GS / 2; o > 0; o >>= 1) so += __shfl_xor(so, o);
   if (lane == 0 && so != 0.0) atomicAdd(a.acc + a.lay.wtOcc + st, so);      // the tile's share of the state's occupation
}

// tied states [a.stBase, a.stBase + S): htkamd_launch_mixstate_range hands over what k_mixstate<13 | 26 | 39> with <= 16 components does not take
int htkamd_launch_mixstate_x(const FbArgs &a, int S, hipStream_t s)
{
   if (a.D < 1 || a.D > 128) { htkamd_set_error("mixture statistics by state: vector size %d outside 1 .. 128", a.D); return HTKAMD_EINVAL; }
   const int W = a.D <= 64 ? 1 : 2;
   const int mode = ((a.uFlags & HTKAMD_UPMEANS) ? 1 : 0) | ((a.uFlags & HTKAMD_UPVARS) ? 2 : 0);
   const dim3 grid(S, MSX_PARTS, (a.maxM + MSX_GS - 1) / MSX_GS), block(64 * W);
   const size_t lds = msx_lds_bytes(a.D, W);
#define MSX_LAUNCH(W_) \
   do { \
      if (mode == 3) hipLaunchKernelGGL((k_mixstate_x<W_, 3>), grid, block, lds, s, a); \
      else if (mode == 1) hipLaunchKernelGGL((k_mixstate_x<W_, 1>), grid, block, lds, s, a); \
      else if (mode == 2) hipLaunchKernelGGL((k_mixstate_x<W_, 2>), grid, block, lds, s, a); \
      else hipLaunchKernelGGL((k_mixstate_x<W_, 0>), grid, block, lds, s, a); \
   } while (0)
   if (W == 1) MSX_LAUNCH(1); else MSX_LAUNCH(2);
#undef MSX_LAUNCH
   HIPCHECK(hipGetLastError());
   return HTKAMD_OK;
}
