// compv_full.hip -- weighted second-order statistics of a frame table on the fp64 matrix pipe:
//    S_k = sum over the frames f of class k of  w_f [x_f, 1]^T [x_f, 1]
// which is what HCompV accumulates for a <FULLC> prototype (AccVar HCompV.c:392-411) with weights and classes added: the last row of
// S_k holds sum w x and sum w, the rows above it the lower triangle of sum w x x^T.
//
// k_cvf_chunk<NT, HASW>: one workgroup owns one chunk of up to CVF_CHUNK frames of one segment.  The augmented row [x, 1] is padded
// with zeros to DP = 16 NT columns; frames are the K dimension of v_mfma_f64_16x16x4_f64 and only the NT(NT+1)/2 tiles on or below
// the diagonal are computed.  The tiles are dealt to the workgroup's NW wavefronts, TPW each (NW * TPW is exactly the tile count for
// every NT, see CvfShape), and a wavefront keeps its TPW accumulator tiles in registers over the whole chunk.
//   Staging: the chunk passes through LDS once, CVF_SUB frames at a time.  A thread fetches elements of the padded [CVF_SUB][DP]
//   sub-block with 4-byte loads (rows of an odd D are only 4-byte aligned), holds them in registers while the sub-block before is
//   multiplied, and writes them to LDS as doubles: sA = w x (the row operand, rounded once in fp64; column D holds w) and, under
//   weights, sB = x (the column operand; column D holds 1).  Without weights both operands are sA.  Columns past D and frames past
//   the chunk's end are zeros in LDS, so a tail needs no branch around the MFMA: the K loop's bound is uniform.
//   LDS rows are LD doubles apart, LD = 16 (mod 32), so the four frame rows of a K step fall into different banks.
// A chunk writes its tiles to P[chunk][tile][16 x 16] (a tile in row-major order); k_cvf_reduce adds the partials of a class in chunk
// order, CVF_RSL contiguous runs of chunks summed side by side and then joined in run order, and writes count, sum and the triangle.
// No floating-point atomics: the bytes are the same run to run.
#include <hip/hip_runtime.h>
#include <vector>
#include "devbuf.h"

DEVBUF_OWNER("compv_full")

#define CVF_CHUNK  512      // frames of a chunk
#define CVF_SUB    32       // frames of a staged sub-block (8 K steps)
#define CVF_MAXDIM 128
#define CVF_REL    16       // k_cvf_reduce: elements of a workgroup ...
#define CVF_RSL    16       // ... and runs of chunks summed side by side

typedef double cvf_d4 __attribute__((ext_vector_type(4)));

struct CvfChunk { long long first; int n; int pad; };

// NT tiles a side: wavefronts of the workgroup and tiles of a wavefront; NW * TPW == NT (NT + 1) / 2
template <int NT> struct CvfShape {
   static constexpr int TILES = NT * (NT + 1) / 2;
   static constexpr int NW = NT == 1 ? 1 : NT <= 3 ? 3 : NT <= 5 ? 5 : NT <= 7 ? 7 : NT == 8 ? 6 : 5;
   static constexpr int TPW = TILES / NW;
   static constexpr int DP = 16 * NT;
   static constexpr int LD = (DP % 32 == 0) ? DP + 16 : DP;
   static constexpr int THREADS = 64 * NW;
   static constexpr int EPT = (CVF_SUB * DP + THREADS - 1) / THREADS;      // staged elements of a thread
   static_assert(NW * TPW == TILES, "the tiles are dealt evenly");
};

template <int NT, bool HASW>
__global__ __launch_bounds__(CvfShape<NT>::THREADS) void k_cvf_chunk(const float *__restrict__ X, const float *__restrict__ W, int D,
                                                                     const CvfChunk *__restrict__ chunks, double *__restrict__ P)
{
   typedef CvfShape<NT> Sh;
   constexpr int DP = Sh::DP, LD = Sh::LD, TPW = Sh::TPW, EPT = Sh::EPT, THREADS = Sh::THREADS;
   __shared__ double sA[CVF_SUB * LD];
   __shared__ double sB[HASW ? CVF_SUB * LD : 1];
   const CvfChunk ch = chunks[blockIdx.x];
   const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
   const float *Xc = X + (size_t)ch.first * D;
   const float *Wc = HASW ? W + ch.first : nullptr;

   // this wavefront's tiles: t = wave + n NW in the row-major count of the lower triangle
   int aOff[TPW], bOff[TPW];
#pragma unroll
   for (int n = 0; n < TPW; n++) {
      const int t = wave + n * Sh::NW;
      int ti = 0;
      while ((ti + 1) * (ti + 2) / 2 <= t) ti++;
      const int tj = t - ti * (ti + 1) / 2;
      aOff[n] = (lane >> 4) * LD + ti * 16 + (lane & 15);
      bOff[n] = (lane >> 4) * LD + tj * 16 + (lane & 15);
   }
   cvf_d4 acc[TPW];
#pragma unroll
   for (int n = 0; n < TPW; n++) acc[n] = (cvf_d4){0.0, 0.0, 0.0, 0.0};

   float xv[EPT], wv[EPT];
   auto fetch = [&](int f0) {      // sub-block at frame f0 of the chunk into registers; what lies outside the table's row is 0 (x) and 0 (w)
#pragma unroll
      for (int i = 0; i < EPT; i++) {
         const int e = tid + i * THREADS, fr = e / DP, c = e - fr * DP;
         const bool in = (e < CVF_SUB * DP) && (f0 + fr < ch.n) && (c <= D);
         xv[i] = in ? (c < D ? Xc[(size_t)(f0 + fr) * D + c] : 1.0f) : 0.0f;
         wv[i] = in ? (HASW ? Wc[f0 + fr] : 1.0f) : 0.0f;
      }
   };
   const double *sBr = HASW ? sB : sA;
   fetch(0);
   for (int f0 = 0; f0 < ch.n; f0 += CVF_SUB) {
      __syncthreads();      // the sub-block before has been multiplied
#pragma unroll
      for (int i = 0; i < EPT; i++) {
         const int e = tid + i * THREADS, fr = e / DP, c = e - fr * DP;
         if (e < CVF_SUB * DP) {
            const double x = (double)xv[i];
            if (HASW) { sA[fr * LD + c] = (double)wv[i] * x; sB[fr * LD + c] = x; }
            else sA[fr * LD + c] = x;
         }
      }
      __syncthreads();
      if (f0 + CVF_SUB < ch.n) fetch(f0 + CVF_SUB);      // in flight under the products below
      const int rem = ch.n - f0, ks = rem >= CVF_SUB ? CVF_SUB / 4 : (rem + 3) >> 2;      // uniform; a tail's last step reads zero rows
      for (int k = 0; k < ks; k++) {
#pragma unroll
         for (int n = 0; n < TPW; n++)
            acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(sA[k * 4 * LD + aOff[n]], sBr[k * 4 * LD + bOff[n]], acc[n], 0, 0, 0);
      }
   }
   // lane l holds rows 4 r + l / 16 (r = 0..3) of column l % 16
   double *Pc = P + (size_t)blockIdx.x * Sh::TILES * 256;
#pragma unroll
   for (int n = 0; n < TPW; n++) {
      double *Pt = Pc + (size_t)(wave + n * Sh::NW) * 256;
#pragma unroll
      for (int r = 0; r < 4; r++) Pt[(4 * r + (lane >> 4)) * 16 + (lane & 15)] = acc[n][r];
   }
}

// Element e of the augmented triangle ((i, j), j <= i <= D, at i (i + 1) / 2 + j) of class blockIdx.x: rows below D are the triangle
// of squares, row D is sum w x and, at its end, sum w.  Thread (el, sl) adds run sl of the class's chunks in order; the runs are then
// joined in run order.
__global__ __launch_bounds__(CVF_REL * CVF_RSL) void k_cvf_reduce(const double *__restrict__ P, const int *__restrict__ clsOff, int D, int tiles,
                                                                  double *__restrict__ count, double *__restrict__ sum, double *__restrict__ sq)
{
   __shared__ double part[CVF_RSL][CVF_REL];
   const int k = blockIdx.x, el = threadIdx.x % CVF_REL, sl = threadIdx.x / CVF_REL;
   const int nEl = (D + 1) * (D + 2) / 2, e = blockIdx.y * CVF_REL + el;
   int i = 0, j = 0;
   double s = 0.0;
   if (e < nEl) {
      i = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
      while ((i + 1) * (i + 2) / 2 <= e) i++;
      while (i * (i + 1) / 2 > e) i--;
      j = e - i * (i + 1) / 2;
      const int ti = i >> 4, tj = j >> 4;
      const size_t at = (size_t)(ti * (ti + 1) / 2 + tj) * 256 + (i & 15) * 16 + (j & 15);
      const int c0 = clsOff[k], n = clsOff[k + 1] - c0;
      const int a = c0 + (int)((long long)n * sl / CVF_RSL), b = c0 + (int)((long long)n * (sl + 1) / CVF_RSL);
      for (int c = a; c < b; c++) s += P[(size_t)c * tiles * 256 + at];
   }
   part[sl][el] = s;
   __syncthreads();
   if (sl == 0 && e < nEl) {
      double t = part[0][el];
      for (int q = 1; q < CVF_RSL; q++) t += part[q][el];
      if (i < D) sq[(size_t)k * (D * (D + 1) / 2) + e] = t;
      else if (j < D) sum[(size_t)k * D + j] = t;
      else count[k] = t;
   }
}

template <int NT> static void cvf_launch(bool hasW, int nChunks, hipStream_t s, const float *dX, const float *dW, int D, const CvfChunk *dCh, double *dP)
{
   if (hasW) hipLaunchKernelGGL((k_cvf_chunk<NT, true>), dim3(nChunks), dim3(CvfShape<NT>::THREADS), 0, s, dX, dW, D, dCh, dP);
   else hipLaunchKernelGGL((k_cvf_chunk<NT, false>), dim3(nChunks), dim3(CvfShape<NT>::THREADS), 0, s, dX, dW, D, dCh, dP);
}

static double cvfLastMs = 0.0;      // the two kernels of the last call

extern "C" double htkamd_compv_full_last_kernel_ms(void) { return cvfLastMs; }
extern "C" int htkamd_compv_full_chunk(void) { return CVF_CHUNK; }
extern "C" int htkamd_compv_full_max_dim(void) { return CVF_MAXDIM; }

extern "C" int htkamd_compv_full(const float *dX, long long nFrames, int D, const float *dW, const htkamd_seg *segs, int nSeg, int nClass,
                                 double *count, double *sum, double *sq, void *stream)
{
   if (!dX || !count || !sum || !sq || D < 1 || nFrames < 0 || nClass < 1 || (segs && nSeg < 0)) { htkamd_set_error("compv_full: bad argument"); return HTKAMD_EINVAL; }
   if (D > CVF_MAXDIM) { htkamd_set_error("compv_full: vector size %d is above the limit of %d", D, CVF_MAXDIM); return HTKAMD_EINVAL; }
   const htkamd_seg whole = {0, 0, 0};
   if (!segs) nSeg = 1;
   // the checks, all before any launch; a whole table is cut like a segment, so its length is kept in 64 bits here
   long long nChunks = 0;
   for (int g = 0; g < nSeg; g++) {
      const long long first = segs ? segs[g].first : whole.first, cnt = segs ? (long long)segs[g].count : nFrames;
      const int cls = segs ? segs[g].cls : 0;
      if (first < 0 || cnt < 0 || first > nFrames || cnt > nFrames - first) {
         htkamd_set_error("compv_full: segment %d (frames %lld .. %lld) lies outside the table's 0 .. %lld", g, first, first + cnt, nFrames);
         return HTKAMD_EINVAL;
      }
      if (cls < 0 || cls >= nClass) { htkamd_set_error("compv_full: segment %d names class %d, outside 0 .. %d", g, cls, nClass - 1); return HTKAMD_EINVAL; }
      nChunks += (cnt + CVF_CHUNK - 1) / CVF_CHUNK;
   }
   if (nChunks > 0x3fffffff) { htkamd_set_error("compv_full: %lld chunks of %d frames are more than one call takes", nChunks, CVF_CHUNK); return HTKAMD_EINVAL; }
   // chunks in class order, a class's chunks in segment and frame order: the order the partial sums are added in
   std::vector<int> clsOff((size_t)nClass + 1, 0);
   for (int g = 0; g < nSeg; g++) {
      const long long cnt = segs ? (long long)segs[g].count : nFrames;
      clsOff[(size_t)(segs ? segs[g].cls : 0) + 1] += (int)((cnt + CVF_CHUNK - 1) / CVF_CHUNK);
   }
   for (int k = 0; k < nClass; k++) clsOff[(size_t)k + 1] += clsOff[k];
   std::vector<CvfChunk> chunks((size_t)nChunks);
   std::vector<int> next(clsOff.begin(), clsOff.end() - 1);
   for (int g = 0; g < nSeg; g++) {
      const long long first = segs ? segs[g].first : 0, cnt = segs ? (long long)segs[g].count : nFrames;
      const int cls = segs ? segs[g].cls : 0;
      for (long long f = 0; f < cnt; f += CVF_CHUNK) {
         const long long left = cnt - f;
         chunks[(size_t)next[cls]++] = CvfChunk{first + f, (int)(left < CVF_CHUNK ? left : CVF_CHUNK), 0};
      }
   }
   const int NT = (D + 1 + 15) / 16, tiles = NT * (NT + 1) / 2, tri = D * (D + 1) / 2;
   hipStream_t s = (hipStream_t)stream;
   DevBuf dCh, dOff;
   KernelTimer timer;
   DevScratch b;
   double *dP = nullptr, *dOut = nullptr;
   const size_t outLen = (size_t)nClass * (1 + (size_t)D + tri);
   int rc;
   if ((rc = dCh.upload(chunks, s)) || (rc = dOff.upload(clsOff, s))) return rc;
   if ((rc = b.get(&dP, (size_t)nChunks * tiles * 256)) || (rc = b.get(&dOut, outLen))) return rc;
   HIPCHECK(timer.start(s));
   if (nChunks > 0) {
      const CvfChunk *c = dCh.as<CvfChunk>();
      const bool w = dW != nullptr;
      switch (NT) {
      case 1: cvf_launch<1>(w, (int)nChunks, s, dX, dW, D, c, dP); break;
      case 2: cvf_launch<2>(w, (int)nChunks, s, dX, dW, D, c, dP); break;
      case 3: cvf_launch<3>(w, (int)nChunks, s, dX, dW, D, c, dP); break;
      case 4: cvf_launch<4>(w, (int)nChunks, s, dX, dW, D, c, dP); break;
      case 5: cvf_launch<5>(w, (int)nChunks, s, dX, dW, D, c, dP); break;
      case 6: cvf_launch<6>(w, (int)nChunks, s, dX, dW, D, c, dP); break;
      case 7: cvf_launch<7>(w, (int)nChunks, s, dX, dW, D, c, dP); break;
      case 8: cvf_launch<8>(w, (int)nChunks, s, dX, dW, D, c, dP); break;
      default: cvf_launch<9>(w, (int)nChunks, s, dX, dW, D, c, dP); break;
      }
      HIPCHECK(hipGetLastError());
   }
   double *dCount = dOut, *dSum = dOut + nClass, *dSq = dSum + (size_t)nClass * D;
   const int nEl = (D + 1) * (D + 2) / 2;
   hipLaunchKernelGGL(k_cvf_reduce, dim3(nClass, (nEl + CVF_REL - 1) / CVF_REL), dim3(CVF_REL * CVF_RSL), 0, s, dP, dOff.as<int>(), D, tiles, dCount, dSum, dSq);
   HIPCHECK(hipGetLastError());
   HIPCHECK(timer.stop(s));
   std::vector<double> h(outLen);
   HIPCHECK(hipMemcpyAsync(h.data(), dOut, sizeof(double) * outLen, hipMemcpyDeviceToHost, s));
   HIPCHECK(hipStreamSynchronize(s));      // (also: the uploads' host vectors outlive their copies)
   float ms = 0.0f;
   HIPCHECK(timer.ms(&ms));
   cvfLastMs = ms;
   for (int k = 0; k < nClass; k++) count[k] = h[k];
   for (size_t q = 0; q < (size_t)nClass * D; q++) sum[q] = h[(size_t)nClass + q];
   for (size_t q = 0; q < (size_t)nClass * tri; q++) sq[q] = h[(size_t)nClass * (1 + D) + q];
   return HTKAMD_OK;
}
