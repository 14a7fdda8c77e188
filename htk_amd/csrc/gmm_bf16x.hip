// gmm_bf16x.hip -- K1bx: K1b's arithmetic (gmm_bf16.hip: bf16 x 3 operand splitting on v_mfma_f32_16x16x32_bf16) for WIDE feature
// vectors, 46 <= D <= 120: NC = ceil(D/15) = 4 .. 8 K chunks of 32.
//
// The quantity and the contract are K1b's (gmm_bf16.hip:1-33): both operands split exactly into three bf16 pieces, six piece products
// per chunk, every chunk carrying complete squares (dimensions as (x^2, x) pairs, the chunk's share -0.5 sum mu^2 ivar at k = 30 against
// a constant 1 in B), accumulators that start at zero, (log w - 0.5 gConst) log2(e) added last by the vector unit, the mixture's
// log-sum-exp by v_exp_f32 / v_log_f32 and the permlane16/32 row swaps, a running maximum and sum across the tiles of a state with more
// than 16 components.  The five correction products go to an accumulator of their own (Cc, stays below ~2) beside the leading products'
// (Cx), as k_score_bf16w keeps them: a chunk's six products are then issued together and the table is read ONCE, chunk by chunk.
//
// What does not fit K1b's shape at these sizes, and what this kernel does instead:
//   B operand (frames).  K1b holds zb[2 column tiles][3][NC] bf8 = 24 NC registers: 192 at NC = 8.  Here a wavefront holds CT column
//       tiles of 16 frames: CT = 2 at NC = 4 (96 registers, K1b's own figure at NC = 4 would be the same), CT = 1 for NC = 5 .. 8
//       (60 .. 96 registers), so the operand never takes more than 96 and every instantiation stays clear of scratch.  A workgroup is four
//       wavefronts = 64 CT frames; a 128-frame task is taken in 2 / CT parts, each a queue entry of its own (K1b's "half tasks").
//       The rows are read straight from global memory, once per part, and split once per part (amortised over the part's <= 64 states).
//   A operand (Gaussians).  A tile is 3 NC KB + 64 bytes (24.6 KB at NC = 8): K1b's double buffer of whole tiles would be 49 KB.  Here the
//       table streams through LDS by (tile, chunk) ROWS of 3 KB (three pieces x 64 lanes x 16 bytes; the row of chunk 0 carries the
//       tile's 16 constants behind it).  A ring of three rows: while row r is multiplied, row r + 1 is stored (it was loaded during
//       row r - 1) and the load of row r + 2 is issued -- one 16-byte word per thread, plain loads and stores, one barrier per row.  The
//       word in flight lives in one of three registers chosen by the chunk number at compile time (chunk & 1, and a third for the last
//       chunk of an odd NC), so no copy between them makes the wavefront wait for a load before its time.
//       LDS per workgroup: 3 x 3136 + 4 = 9412 bytes (9424 as laid out), whatever NC: sixteen workgroups fit the 160 KB; the registers decide.
//   Table layout (k_build_bf16xtab below): per tile [chunk NC][piece 3][lane 64][8 bf16], then 16 f32 (log w - 0.5 gConst) log2(e)
//       (-1e30 for a dead or missing component); lane l holds row l & 15, k = 32 chunk + 8 (l >> 4) + j.  Chunk c covers the
//       dimensions dpc c .. dpc c + dpc - 1, dpc = ceil(D / NC) <= 15, as K1b's.  Constants in double, rounded once.
//   Forward-backward's queues and ranges (ScoreArgs::qStart / qCounters, slotRange) are IGNORED, as k_score_bf16 ignores them: every part
//       is pulled from taskCounter and every (frame, state) of a task is written.  NSt is ignored as there (the callers refuse
//       multi-stream sets in the matrix-core modes or score stream rows one by one).
//
// Registers, LDS and occupancy as the compiler reports them for gfx950 (-Rpass-analysis=kernel-resource-usage), scratch 0 everywhere:
//   NC   CT   VGPRs   wavefronts / SIMD (= workgroups / CU, __launch_bounds__' second figure)   LDS / workgroup
//    4    2    168     3                                                                         9424 bytes
//    5    1    120     4                                                                         9424
//    6    1    128     4                                                                         9424
//    7    1    144     3                                                                         9424
//    8    1    152     3                                                                         9424
// (no AGPRs; left alone the compiler takes 176 / 118 / 146 / 166 / 170 registers: the second figure of __launch_bounds__ buys a
//  wavefront per SIMD at NC = 4, 6 and 8.  LDS: four workgroups take 37 KB of the CU's 160.)
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "internal.h"
#include "hipcheck.h"
#include "kernels.h"

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef unsigned int u4 __attribute__((ext_vector_type(4)));

#define EXP2(x) __builtin_amdgcn_exp2f(x)
#define LOG2(x) __builtin_amdgcn_logf(x)
#define MFMA(a_, b_, c_) __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_, b_, c_, 0, 0, 0)

__device__ __forceinline__ float rows_max_x(float v)
{
   auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
   v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
   auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
   return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float rows_sum_x(float v)
{
   auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
   v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
   auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
   return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// (v.x, v.y) = p1 + p2 + p3 + O(2^-27): three packed bf16 pairs (round to nearest even), every difference exact in fp32
__device__ __forceinline__ void split3_pair(v2f v, unsigned int &p1, unsigned int &p2, unsigned int &p3)
{
   p1 = __builtin_bit_cast(unsigned int, __builtin_convertvector(v, bf2));
   v = v - (v2f){__uint_as_float(p1 << 16), __uint_as_float(p1 & 0xffff0000u)};
   p2 = __builtin_bit_cast(unsigned int, __builtin_convertvector(v, bf2));
   v = v - (v2f){__uint_as_float(p2 << 16), __uint_as_float(p2 & 0xffff0000u)};
   p3 = __builtin_bit_cast(unsigned int, __builtin_convertvector(v, bf2));
}

#define BX_ROW4 192                                    /* 16-byte words of a (tile, chunk) row: piece 3 x lane 64 */
#define BX_SLOT4 (BX_ROW4 + 4)                         /* ... of a ring slot: the row, then the tile's 16 constants (with chunk 0) */
#define BX_RING 3
#define BX_EU4 3
#define BX_EU5 4
#define BX_EU6 4
#define BX_EU7 3
#define BX_EU8 3
constexpr int bx_ct(int NC) { return NC <= 4 ? 2 : 1; }                              // column tiles of 16 frames per wavefront
constexpr int bx_eu(int NC) { return NC <= 4 ? BX_EU4 : NC == 5 ? BX_EU5 : NC == 6 ? BX_EU6 : NC == 7 ? BX_EU7 : BX_EU8; }      // wavefronts per SIMD the registers allow (the table above)
constexpr int bx_reg(int NC, int c) { return ((NC & 1) && c == NC - 1) ? 2 : (c & 1); }      // the staging register of chunk c's row

template <int NC>
__global__ __launch_bounds__(256, bx_eu(NC)) void k_score_bf16x(ScoreArgs a)
{
   constexpr int CT = bx_ct(NC), FPW = 16 * CT, FPB = 4 * FPW, PARTS = B16_TASK_FRAMES / FPB;
   constexpr int TW4 = NC * BX_ROW4 + 4;               // 16-byte words per tile in the table
   __shared__ u4 ring[BX_RING][BX_SLOT4];
   __shared__ int taskSh;
   const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
   const int col = lane & 15, kg = lane >> 4;
   const int D = a.D;
   const int dpc = (D + NC - 1) / NC;                  // dimensions per K chunk (<= 15)
   const u4 *tab = (const u4 *)a.bf16Tab;
   // this thread's word of a row: 0 .. 191 the row itself, 192 .. 195 the tile's constants (they travel with the row of chunk 0)
   auto row_word = [&](int tile, int c) -> const u4 * { return tab + (size_t)tile * TW4 + (tid < BX_ROW4 ? c * BX_ROW4 + tid : NC * BX_ROW4 + tid - BX_ROW4); };

   for (;;) {
      if (tid == 0) taskSh = atomicAdd(a.taskCounter, 1);
      __syncthreads();
      const int vtask = __builtin_amdgcn_readfirstlane(taskSh);
      const int task = vtask / PARTS;
      if (task >= a.nTasks) break;
      const ScoreTask tk = a.tasks[task];
      const int f0 = FPB * (vtask % PARTS);            // the part's first frame in the task
      if (PARTS > 1 && f0 >= tk.nFrames) { __syncthreads(); continue; }      // (the barrier: nobody is still reading taskSh)
      const int fw = f0 + FPW * wv;                    // this wavefront's
      const bool active = fw < tk.nFrames;

      // first tile and the tile after the last of every state of the task, one per lane (tasks hold at most 64 states)
      int tFirstV = 0, tEndV = 0;
      if (lane < tk.nSlots) { const int stl = a.slotState[tk.slot0 + lane]; tFirstV = a.stateTileOff[stl]; tEndV = a.stateTileOff[stl + 1]; }
      int tile = __builtin_amdgcn_readlane(tFirstV, 0);
      // rows 0 and 1 of the task: the first into the ring, the second into its register
      u4 stg[3];
      stg[0] = stg[1] = stg[2] = (u4)(0u);
      if (tid < BX_SLOT4) ring[0][tid] = *row_word(tile, 0);
      if (tid < BX_ROW4) stg[bx_reg(NC, 1)] = *row_word(tile, 1);

      // B operand: this lane's frame (col) of each column tile, the 8 k of lane group kg in every chunk, in three bf16 pieces
      bf8 zb[CT][3][NC];
      if (active) {
         int kgL = kg, colL = col;
         asm volatile("" : "+v"(kgL), "+v"(colL));      // (cheap to recompute per task: hoisted out of the task loop they are spilled)
#pragma unroll
         for (int ft = 0; ft < CT; ft++) {
            int f = fw + ft * 16 + colL;
            if (f > tk.nFrames - 1) f = tk.nFrames - 1;
            const float *row = a.X + (size_t)(tk.frame0 + f) * D;
#pragma unroll
            for (int c = 0; c < NC; c++) {
               const int d0 = dpc * c + 4 * kgL;        // dimensions d0 .. d0 + 3 -> k = 32 c + 8 kg + (0 .. 7) = (x^2, x) pairs
               unsigned int w[3][4];
#pragma unroll
               for (int i = 0; i < 4; i++) {
                  int dim = d0 + i;
                  const bool pad = 4 * kgL + i >= dpc || dim >= D;
                  if (pad) dim = D - 1;
                  float v = row[dim];
                  if (pad) v = 0.0f;
                  float v2 = v * v;
                  if (i == 3 && kgL == 3) v2 = 1.0f;    // k = 30: the constant that meets the chunk's -0.5 sum mu^2 ivar
                  split3_pair((v2f){v2, v}, w[0][i], w[1][i], w[2][i]);
               }
#pragma unroll
               for (int s = 0; s < 3; s++) zb[ft][s][c] = __builtin_bit_cast(bf8, (u4){w[s][0], w[s][1], w[s][2], w[s][3]});
            }
         }
      }
      __syncthreads();

      int rs = 0;                                       // the ring slot of the row being multiplied
      for (int k = 0; k < tk.nSlots; k++) {
         const int t1 = __builtin_amdgcn_readlane(tEndV, k);
         const int nextFirst = (k + 1 < tk.nSlots) ? __builtin_amdgcn_readlane(tFirstV, (k + 1) & 63) : -1;
         float rM[CT], rS[CT];
         bool first = true;
         for (;;) {
            const int nextTile = (tile + 1 < t1) ? tile + 1 : nextFirst;
            f4 Cx[CT], Cc[CT], ci = (f4)(0.0f);
#pragma unroll
            for (int ft = 0; ft < CT; ft++) { Cx[ft] = (f4)(0.0f); Cc[ft] = (f4)(0.0f); }
#pragma unroll
            for (int c = 0; c < NC; c++) {
               // the load of the row after the next: chunk c + 2 of this tile, or chunk c + 2 - NC of the next one
               {
                  const int c2 = (c + 2) % NC;
                  const int t2 = (c + 2 < NC) ? tile : nextTile;
                  if (t2 >= 0 && tid < (c2 == 0 ? BX_SLOT4 : BX_ROW4)) stg[bx_reg(NC, c2)] = *row_word(t2, c2);
               }
               if (active) {
                  const u4 *R = ring[rs];
                  const bf8 a1 = __builtin_bit_cast(bf8, R[lane]), a2 = __builtin_bit_cast(bf8, R[64 + lane]), a3 = __builtin_bit_cast(bf8, R[128 + lane]);
                  if (c == 0) ci = __builtin_bit_cast(f4, R[BX_ROW4 + kg]);      // rows 4 kg .. 4 kg + 3 of the tile
                  // the corrections, smallest first, into Cc; the leading product into Cx: complete squares per chunk, both from zero
#pragma unroll
                  for (int ft = 0; ft < CT; ft++) {
                     Cc[ft] = MFMA(a2, zb[ft][1][c], Cc[ft]);
                     Cc[ft] = MFMA(a1, zb[ft][2][c], Cc[ft]);
                     Cc[ft] = MFMA(a3, zb[ft][0][c], Cc[ft]);
                     Cc[ft] = MFMA(a1, zb[ft][1][c], Cc[ft]);
                     Cc[ft] = MFMA(a2, zb[ft][0][c], Cc[ft]);
                     Cx[ft] = MFMA(a1, zb[ft][0][c], Cx[ft]);
                  }
               }
               // the next row (loaded a row ago) into its slot: nobody has read that slot since the row before this one
               {
                  const int c1 = (c + 1) % NC;
                  const int tn = (c + 1 < NC) ? tile : nextTile;
                  const int ws = rs == BX_RING - 1 ? 0 : rs + 1;
                  if (tn >= 0 && tid < (c1 == 0 ? BX_SLOT4 : BX_ROW4)) ring[ws][tid] = stg[bx_reg(NC, c1)];
                  __syncthreads();
                  rs = ws;
               }
            }
            if (active) {
               // log-sum-exp over the tile's 16 rows: 4 in this lane, the rest in lanes ^16, ^32, ^48 (base-2 logs)
#pragma unroll
               for (int ft = 0; ft < CT; ft++) {
                  const f4 y = (Cx[ft] + Cc[ft]) + ci;
                  float mx = fmaxf(fmaxf(y[0], y[1]), fmaxf(y[2], y[3]));
                  mx = rows_max_x(mx);
                  float sm = (EXP2(y[0] - mx) + EXP2(y[1] - mx)) + (EXP2(y[2] - mx) + EXP2(y[3] - mx));
                  sm = rows_sum_x(sm);
                  if (first) { rM[ft] = mx; rS[ft] = sm; }
                  else {
                     const float M2 = fmaxf(rM[ft], mx);
                     rS[ft] = rS[ft] * EXP2(rM[ft] - M2) + sm * EXP2(mx - M2);
                     rM[ft] = M2;
                  }
               }
               first = false;
            }
            tile++;
            if (tile >= t1) break;
         }
         tile = nextFirst;
         if (active) {
            float res = 0.0f;
#pragma unroll
            for (int ft = 0; ft < CT; ft++) {
               const float r = (rM[ft] + LOG2(rS[ft])) * 0.69314718055994531f;
               if (kg == ft) res = r;
            }
            float *o = a.out + tk.outBase + (size_t)(tk.outSlot0 + k) * tk.ldo + fw;
            if (lane < FPW && fw + lane < tk.nFrames) o[lane] = res;
         }
      }
   }
}

int htkamd_launch_score_bf16x(const htkamd_model *m, const ScoreArgs &a, hipStream_t stream, hipEvent_t evStart, hipEvent_t evStop)
{
   // persistent workgroups, as many as the registers let a CU hold; a part of a task (64 or 128 frames x up to 64 states) at a time
#define X_LAUNCH(NC_) do { const long long parts_ = (long long)a.nTasks * (2 / bx_ct(NC_)); const int cap_ = 256 * bx_eu(NC_); \
                           hipExtLaunchKernelGGL((k_score_bf16x<NC_>), dim3((unsigned)(parts_ < cap_ ? parts_ : cap_)), dim3(256), 0, stream, evStart, evStop, 0, a); } while (0)
   switch (m->bf16NC) {
   case 4: X_LAUNCH(4); break;
   case 5: X_LAUNCH(5); break;
   case 6: X_LAUNCH(6); break;
   case 7: X_LAUNCH(7); break;
   case 8: X_LAUNCH(8); break;
   default: htkamd_set_error("score_bf16: no wide-vector kernel for %d K-chunks", m->bf16NC); return HTKAMD_EMODEL;
   }
#undef X_LAUNCH
   HIPCHECK(hipGetLastError());
   return HTKAMD_OK;
}

// ------------------------------------------------------------------------------------ the A-operand table, built on the device
struct Bf16xTabArgs {
   int D, NC, nTiles;
   const int *stateCompOff, *stateTileOff, *compGauss, *tileState;
   const float *mean, *ivar, *gconst, *compLogWt;
   u4 *tab;                    // [tile][ chunk NC ][ piece 3 ][ lane 64 ] 16-byte words, then 4 words = 16 f32
};

// one thread per (tile, chunk, lane): its 8 coefficients in three pieces = three 16-byte stores, consecutive lanes to consecutive words;
// the 16 threads (chunk 0, lane group 0) of a tile also write their component's constant.  The values are k_build_bf16tab's.
__global__ void k_build_bf16xtab(Bf16xTabArgs a)
{
   const int NC = a.NC, D = a.D;
   const int idx = blockIdx.x * blockDim.x + threadIdx.x;
   if (idx >= a.nTiles * NC * 64) return;
   const int t = idx / (NC * 64), r = idx - t * (NC * 64), ch = r >> 6, lane = r & 63, rowc = lane & 15, kg = lane >> 4;
   const int s = a.tileState[t], c0 = a.stateCompOff[s], c1 = a.stateCompOff[s + 1];
   const int c = c0 + 16 * (t - a.stateTileOff[s]) + rowc;
   u4 *T = a.tab + (size_t)t * (NC * BX_ROW4 + 4);
   const bool live = c < c1 && (c1 - c0 == 1 || a.compLogWt[c] > (float)LMINMIX);
   const double L2E = 1.4426950408889634;
   const float *mu = nullptr, *iv = nullptr;
   if (live) { const int g = a.compGauss[c]; mu = a.mean + (size_t)g * D; iv = a.ivar + (size_t)g * D; }
   const int dpc = (D + NC - 1) / NC, dlo = dpc * ch, dhi = (dlo + dpc < D) ? dlo + dpc : D;     // this chunk's dimensions
   unsigned int w[3][4];
#pragma unroll
   for (int i = 0; i < 4; i++) {                         // the pair (k, k + 1) = (8 kg + 2 i, + 1): (x^2, x) coefficients of one dimension
      const int kk = 8 * kg + 2 * i, dim = dlo + (kk >> 1);
      v2f v = {0.0f, 0.0f};
      if (live && dim < dhi) v = (v2f){(float)(-0.5 * (double)iv[dim] * L2E), (float)((double)mu[dim] * iv[dim] * L2E)};
      if (live && kk == 30) {                            // against B's constant 1: -0.5 sum mu^2 ivar over the chunk
         double q = 0.0;
         for (int d = dlo; d < dhi; d++) q += (double)mu[d] * mu[d] * iv[d];
         v.x = (float)(-0.5 * q * L2E);
      }
      split3_pair(v, w[0][i], w[1][i], w[2][i]);
   }
#pragma unroll
   for (int pc = 0; pc < 3; pc++) T[(ch * 3 + pc) * 64 + lane] = (u4){w[pc][0], w[pc][1], w[pc][2], w[pc][3]};
   if (ch == 0 && kg == 0) {
      float ci = -1.0e30f;
      if (live) ci = (float)(((c1 - c0 == 1 ? 0.0 : (double)a.compLogWt[c]) - 0.5 * (double)a.gconst[a.compGauss[c]]) * L2E);
      ((float *)(T + NC * BX_ROW4))[rowc] = ci;
   }
}

int htkamd_model_refresh_bf16x_device(htkamd_model *m, void *stream)
{
   Bf16xTabArgs t;
   t.D = m->D; t.NC = m->bf16NC; t.nTiles = m->nTiles;
   t.stateCompOff = m->d_stateCompOff; t.stateTileOff = m->d_stateTileOff; t.compGauss = m->d_compGauss; t.tileState = m->d_tileState;
   t.mean = m->d_mean; t.ivar = m->d_ivar; t.gconst = m->d_gconst; t.compLogWt = m->d_compLogWt; t.tab = (u4 *)m->d_bf16Tab;
   const int n = m->nTiles * m->bf16NC * 64;
   hipLaunchKernelGGL(k_build_bf16xtab, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, t);
   HIPCHECK(hipGetLastError());
   return HTKAMD_OK;
}
