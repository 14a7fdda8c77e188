// gmm_full.hip -- full-covariance (FULLC) GMM state log-likelihoods, bit-exact to the reference.
//
// Replaces FOutP (HModel.c:5361-5381), reached through MOutP from ShStrP (HFB.c:935-960) / cSOutP (HRec.c:460-482) / SOutP:
//     xmm[i] = x[i]-mean[i];  sum = 0
//     for j < D: for i > j: sum += (xmm[i]*xmm[j])*m[i][j]        (float, in this order, no FMA)
//     sum *= 2;  sum += gConst;  for i: sum += (xmm[i]*xmm[i])*m[i][i]
//     return -0.5*sum                                               (double product, stored to float)
// followed by the same mixture sum as gmm_exact.hip: the float LAdd of ShStrP / cSOutP or SOutP's double form, the single-Gaussian
// shortcut and LMINMIX skipping.
//
// MI355X mapping: k_score_exact's.  Lanes are FRAMES, two per lane as float2 {frame lane, frame lane+64} in packed FP32 (v_pk_add_f32 /
// v_pk_mul_f32), the Gaussian is wave-uniform, and its row of the model's FULLC table (mean[D], the packed lower triangle, gConst:
// htkamd_model::d_fparam) comes through scalar loads in the constant address space and feeds the packed instructions as SGPR pairs.
// xmm is formed once per Gaussian and held in VGPRs (2*D of them, 78 at D = 39); the feature rows are re-read for every Gaussian (L1 hits,
// 2*D loads against ~3*D(D+1)/2 packed flop) because keeping them as well would spill at D = 39.  Same task table and persistent waves
// as the diagonal kernel.
//
// Algorithmic work per (frame, Gaussian): D subtractions, 3*D(D-1)/2 + 1 for the off-diagonal terms, 3*D + 1 for the diagonal ones,
// i.e. 3*D(D+1)/2 + D + 2 flop (2 381 at D = 39, 1 081 at D = 26 against 4*D+8 = 164 / 112 for DIAGC); VALU (packed FP32) bound.
// The sum is one dependent chain per frame, as the reference's: the latency is hidden by the other waves of the SIMD, not inside one.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "internal.h"
#include "hipcheck.h"
#include "kernels.h"
#include "ladd.h"

typedef float v2f __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(4))) float cfloat;    // constant address space -> s_load
typedef const __attribute__((address_space(4))) int cint;

// FOutP of the two frames of a lane (feature rows r0, r1); P = the Gaussian's row: mean [0, D), triangle [D, D + D(D+1)/2), gConst behind it
template <int D>
__device__ __forceinline__ v2f fout_p2(const float *r0, const float *r1, cfloat *P)
{
   constexpr int TRI = D * (D + 1) / 2;
   v2f xm[D];
#pragma unroll
   for (int i = 0; i < D; i++) { v2f x = {r0[i], r1[i]}; xm[i] = x - P[i]; }
   v2f sum = {0.0f, 0.0f};
#pragma unroll
   for (int j = 0; j < D - 1; j++)
#pragma unroll
      for (int i = j + 1; i < D; i++) {
         v2f p = xm[i] * xm[j];
         p = p * P[D + i * (i + 1) / 2 + j];
         sum = sum + p;
      }
   sum = sum * 2.0f;
   sum = sum + P[D + TRI];
#pragma unroll
   for (int i = 0; i < D; i++) {
      v2f p = xm[i] * xm[i];
      p = p * P[D + i * (i + 1) / 2 + i];
      sum = sum + p;
   }
   v2f r;
   r.x = (float)(-0.5 * (double)sum.x);
   r.y = (float)(-0.5 * (double)sum.y);
   return r;
}

template <int D, bool SOUTP>
__global__ __launch_bounds__(256) void k_score_full(ScoreArgs a)
{
   __shared__ double tab[LADD_TAB_DOUBLES];
   ladd_table_to_lds(tab, a.laddTab);
   __syncthreads();
   const int lane = threadIdx.x & 63;
   const double mle = a.minLogExp;
   cint *slotState = (cint *)a.slotState;
   cint *stateCompOff = (cint *)a.stateCompOff;
   cint *compGauss = (cint *)a.compGauss;
   cfloat *compLogWt = (cfloat *)a.compLogWt;

   for (;;) {
      int task = 0;
      if (lane == 0) task = atomicAdd(a.taskCounter, 1);
      task = __builtin_amdgcn_readfirstlane(task);
      if (task >= a.nTasks) break;
      const ScoreTask tk = a.tasks[task];

      int t0 = lane, t1 = lane + 64;
      if (t0 > tk.nFrames - 1) t0 = tk.nFrames - 1;
      if (t1 > tk.nFrames - 1) t1 = tk.nFrames - 1;
      const float *r0 = a.X + (size_t)(tk.frame0 + t0) * D;
      const float *r1 = a.X + (size_t)(tk.frame0 + t1) * D;

      for (int k = 0; k < tk.nSlots; k++) {
         const int s = slotState[tk.slot0 + k];
         const int c0 = stateCompOff[s], c1 = stateCompOff[s + 1];
         float acc0, acc1;
         if (c1 - c0 == 1) {                    // single Gaussian: no weight, no LAdd (HFB.c:917-928)
            const v2f px = fout_p2<D>(r0, r1, (cfloat *)(a.gparam + (size_t)compGauss[c0] * a.PS));
            acc0 = px.x; acc1 = px.y;
         } else {
            acc0 = (float)LZERO; acc1 = (float)LZERO;
            double dacc0 = LZERO, dacc1 = LZERO;
            for (int c = c0; c < c1; c++) {
               const float wt = compLogWt[c];
               if (wt > (float)LMINMIX) {       // wave-uniform branch
                  const v2f px = fout_p2<D>(r0, r1, (cfloat *)(a.gparam + (size_t)compGauss[c] * a.PS));
                  if constexpr (SOUTP) {
                     dacc0 = ladd_tab(dacc0, (double)wt + (double)px.x, mle, tab);
                     dacc1 = ladd_tab(dacc1, (double)wt + (double)px.y, mle, tab);
                  } else {
                     const v2f y = wt + px;
                     ladd_tab_f2(acc0, y.x, acc1, y.y, mle, tab);
                  }
               }
            }
            if constexpr (SOUTP) { acc0 = (float)dacc0; acc1 = (float)dacc1; }
         }
         float *o = a.out + tk.outBase + (size_t)(tk.outSlot0 + k) * tk.ldo;
         if (lane < tk.nFrames) o[lane] = acc0;
         if (lane + 64 < tk.nFrames) o[lane + 64] = acc1;
      }
   }
}

// Any vector size: one frame per lane at a time, features re-read from global memory (L1-resident rows) and xmm re-formed where it is
// used (the same float subtraction, so the same value).
template <bool SOUTP>
__global__ __launch_bounds__(256) void k_score_full_anyD(ScoreArgs a)
{
   __shared__ double tab[LADD_TAB_DOUBLES];
   ladd_table_to_lds(tab, a.laddTab);
   __syncthreads();
   const int lane = threadIdx.x & 63;
   const int D = a.D;
   const int TRI = D * (D + 1) / 2;
   for (;;) {
      int task = 0;
      if (lane == 0) task = atomicAdd(a.taskCounter, 1);
      task = __builtin_amdgcn_readfirstlane(task);
      if (task >= a.nTasks) break;
      const ScoreTask tk = a.tasks[task];
      for (int f = 0; f < 2; f++) {
         int t = lane + 64 * f;
         const bool live = t < tk.nFrames;
         if (!live) t = tk.nFrames - 1;
         const float *row = a.X + (size_t)(tk.frame0 + t) * D;
         for (int k = 0; k < tk.nSlots; k++) {
            const int s = a.slotState[tk.slot0 + k];
            const int c0 = a.stateCompOff[s], c1 = a.stateCompOff[s + 1];
            float acc = (float)LZERO;
            double dacc = LZERO;
            for (int c = c0; c < c1; c++) {
               const float wt = a.compLogWt[c];
               if (c1 - c0 > 1 && !(wt > (float)LMINMIX)) continue;
               const float *P = a.gparam + (size_t)a.compGauss[c] * a.PS;
               const float *M = P + D;
               float sum = 0.0f;
               for (int j = 0; j < D - 1; j++) {
                  const float xj = row[j] - P[j];
                  for (int i = j + 1; i < D; i++) {
                     const float xi = row[i] - P[i];
                     const float p = xi * xj;
                     sum += p * M[i * (i + 1) / 2 + j];
                  }
               }
               sum *= 2.0f;
               sum += P[D + TRI];
               for (int i = 0; i < D; i++) {
                  const float xi = row[i] - P[i];
                  const float p = xi * xi;
                  sum += p * M[i * (i + 1) / 2 + i];
               }
               const float mixp = (float)(-0.5 * (double)sum);
               if (c1 - c0 == 1) acc = mixp;
               else if constexpr (SOUTP) dacc = ladd_tab(dacc, (double)wt + (double)mixp, a.minLogExp, tab);
               else {
                  float y = wt + mixp;
                  acc = ladd_tab_f(acc, y, a.minLogExp, tab);
               }
            }
            if (SOUTP && c1 - c0 > 1) acc = (float)dacc;
            if (live) a.out[tk.outBase + (size_t)(tk.outSlot0 + k) * tk.ldo + t] = acc;
         }
      }
   }
}

// Called by htkamd_launch_score_exact for a FULLC model: the scoring arguments with the model's FULLC table in place of the DIAGC one.
int htkamd_launch_score_full(const htkamd_model *m, const ScoreArgs &a0, hipStream_t stream, hipEvent_t evStart, hipEvent_t evStop, bool soutp, bool diagc)
{
   if (a0.nTasks <= 0) return HTKAMD_OK;
   if (!m->fullc || !m->d_fparam) { htkamd_set_error("score_full: not a FULLC model"); return HTKAMD_EMODEL; }
   if (diagc) { htkamd_set_error("score_full: the DIAGC score form (HTKAMD_SCORE_DIAGC) does not apply to a FULLC model"); return HTKAMD_EMODEL; }
   if (a0.NSt > 1) { htkamd_set_error("score_full: several streams are not supported with FULLC"); return HTKAMD_EMODEL; }
   ScoreArgs a = a0;
   a.gparam = m->d_fparam; a.PS = m->FPS;
   HIPCHECK(hipMemsetAsync(a.taskCounter, 0, sizeof(int), stream));
   int blocks = (a.nTasks + 3) / 4;
   if (blocks > 256 * 3) blocks = 256 * 3;      // persistent four-wave blocks, one resident set per CU: the D = 39 kernel (117-120 VGPRs) runs at
                                                // 3 waves per SIMD (compiler report for gfx950), i.e. 3 blocks per CU; more would only queue
   dim3 grid(blocks), block(256);
   switch (m->D) {
   case 39: if (soutp) hipExtLaunchKernelGGL((k_score_full<39, true>), grid, block, 0, stream, evStart, evStop, 0, a);
            else hipExtLaunchKernelGGL((k_score_full<39, false>), grid, block, 0, stream, evStart, evStop, 0, a); break;
   case 26: if (soutp) hipExtLaunchKernelGGL((k_score_full<26, true>), grid, block, 0, stream, evStart, evStop, 0, a);
            else hipExtLaunchKernelGGL((k_score_full<26, false>), grid, block, 0, stream, evStart, evStop, 0, a); break;
   case 13: if (soutp) hipExtLaunchKernelGGL((k_score_full<13, true>), grid, block, 0, stream, evStart, evStop, 0, a);
            else hipExtLaunchKernelGGL((k_score_full<13, false>), grid, block, 0, stream, evStart, evStop, 0, a); break;
   default: if (soutp) hipExtLaunchKernelGGL((k_score_full_anyD<true>), grid, block, 0, stream, evStart, evStop, 0, a);
            else hipExtLaunchKernelGGL((k_score_full_anyD<false>), grid, block, 0, stream, evStart, evStop, 0, a); break;
   }
   HIPCHECK(hipGetLastError());
   return HTKAMD_OK;
}
