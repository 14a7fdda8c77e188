// cepsnorm.hip -- side-based cepstral mean and variance normalisation on the device: the statistics `HCompV -c -k -q nmv` estimates per
// speaker / conversation side (AccGenUtt, UpdateSpkrAccList, UpdateMeanVar: HTKTools/HCompV.c:520-656) and the tail of AddQualifiers that
// applies them (HTKLib/HParm.c:1728-1741 side mean, :1804-1812 variance scaling).  Files, masks, checks and the scale table: host/cepsnorm.c.
//
// Statistics.  The reference sums floats in file order; here the sums are fp64 (as htkamd_compv) and DETERMINISTIC -- two stages, no
// floating-point atomics:
//   k_side_partial   block = (utterance, chunk of 64 columns), 4 wavefronts.  A lane owns a column, the wavefronts stride the frames, so a
//                    wavefront reads one row's columns side by side.  The four partial sums of a column meet in LDS and are added in
//                    wavefront order into part[u][0..D) = sum x, part[u][D..2D) = sum x^2.
//   k_side_merge     thread = (side, entry of the 2D vector): adds the utterances of the side in utterance order (the host lists them).
// Normalisation.  k_row_side finds every row's side (binary search over the utterances, as k_mfcc_index), k_side_normalise is one thread
// per element of the leading max(dMean, dScale) columns: x = x - mean, then x = x * scale: two separately rounded float operations.
// Both are bandwidth-bound: the table is read once (and, for the normalisation, its leading columns written once).
#include <hip/hip_runtime.h>
#include <vector>
#include "internal.h"
#include "hipcheck.h"
#include "devbuf.h"

#define SS_WAVES 4
#define SS_LANES 64

__global__ __launch_bounds__(SS_WAVES * SS_LANES) void k_side_partial(const float *X, const int *frameOff, int nCols, int D, double *part)
{
   __shared__ double lds[SS_WAVES][2][SS_LANES];
   const int u = blockIdx.x, lane = threadIdx.x & (SS_LANES - 1), w = threadIdx.x / SS_LANES;
   const int c = blockIdx.y * SS_LANES + lane;
   const int f0 = frameOff[u], f1 = frameOff[u + 1];
   double s = 0.0, q = 0.0;
   if (c < D)
      for (int f = f0 + w; f < f1; f += SS_WAVES) { const double v = (double)X[(size_t)f * nCols + c]; s += v; q += v * v; }
   lds[w][0][lane] = s; lds[w][1][lane] = q;
   __syncthreads();
   if (w == 0 && c < D) {
      for (int k = 1; k < SS_WAVES; k++) { s += lds[k][0][lane]; q += lds[k][1][lane]; }
      part[(size_t)u * 2 * D + c] = s;
      part[(size_t)u * 2 * D + D + c] = q;
   }
}

// sideOff [nSide+1], sideUtt: the utterances of every side in utterance order; out [nSide x 2D]: sums, then sums of squares
__global__ void k_side_merge(const double *part, const int *sideOff, const int *sideUtt, int nSide, int D, double *out)
{
   const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= (size_t)nSide * 2 * D) return;
   const int side = (int)(i / (2 * (size_t)D)), j = (int)(i % (2 * (size_t)D));
   double a = 0.0;
   for (int k = sideOff[side]; k < sideOff[side + 1]; k++) a += part[(size_t)sideUtt[k] * 2 * D + j];
   out[i] = a;
}

__global__ void k_row_side(const int *frameOff, const int *uttSide, int nUtt, int nFrames, int *rowSide)
{
   const int f = blockIdx.x * blockDim.x + threadIdx.x;
   if (f >= nFrames) return;
   int lo = 0, hi = nUtt - 1;                            // the last u with frameOff[u] <= f (empty utterances share an offset: the last one owns the row)
   while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (frameOff[mid] <= f) lo = mid; else hi = mid - 1; }
   rowSide[f] = uttSide[lo];
}

__global__ void k_side_normalise(float *X, const int *rowSide, size_t nFrames, int nCols, int W, const float *mean, int dMean, const float *scale, int dScale)
{
   const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= nFrames * W) return;
   const size_t f = i / W;
   const int c = (int)(i % W), side = rowSide[f];
   float x = X[f * nCols + c];
   if (c < dMean) x = x - mean[(size_t)side * dMean + c];
   if (c < dScale) x = x * scale[(size_t)side * dScale + c];
   X[f * nCols + c] = x;
}

// the arguments both entry points share; F = rows of the table
static int check_batch(const char *who, const int *frameOff, const int *uttSide, int nUtt, int nSide, int *F)
{
   if (!frameOff || nUtt < 0 || nSide < 0 || (nUtt > 0 && !uttSide)) { htkamd_set_error("%s: bad argument", who); return HTKAMD_EINVAL; }
   if (nUtt > 0 && frameOff[0] != 0) { htkamd_set_error("%s: frameOff[0] is %d", who, frameOff[0]); return HTKAMD_EINVAL; }
   for (int u = 0; u < nUtt; u++) {
      if (frameOff[u + 1] < frameOff[u]) { htkamd_set_error("%s: frameOff not monotone", who); return HTKAMD_EINVAL; }
      if (uttSide[u] < 0 || uttSide[u] >= nSide) { htkamd_set_error("%s: utterance %d is of side %d of %d", who, u, uttSide[u], nSide); return HTKAMD_EINVAL; }
   }
   *F = nUtt ? frameOff[nUtt] : 0;
   return HTKAMD_OK;
}

DEVBUF_OWNER("cepsnorm")

extern "C" int htkamd_side_stats(const float *dX, const int *frameOff, const int *uttSide, int nUtt, int nSide, int nCols, int D,
                                 double *sum, double *sqsum, long long *nFrames, void *stream)
{
   int F = 0;
   if (!sum || !sqsum || !nFrames || nCols < 1 || D < 1 || D > nCols) { htkamd_set_error("side_stats: bad argument"); return HTKAMD_EINVAL; }
   { const int rc = check_batch("side_stats", frameOff, uttSide, nUtt, nSide, &F); if (rc) return rc; }
   if (F > 0 && !dX) { htkamd_set_error("side_stats: NULL table"); return HTKAMD_EINVAL; }
   if (htkamd_device_count() <= 0) { htkamd_set_error("side_stats: no HIP device"); return HTKAMD_ENODEV; }
   for (int s = 0; s < nSide; s++) nFrames[s] = 0;
   for (size_t i = 0; i < (size_t)nSide * D; i++) sum[i] = sqsum[i] = 0.0;
   if (nUtt == 0 || nSide == 0) return HTKAMD_OK;
   std::vector<int> sideOff((size_t)nSide + 1, 0), sideUtt((size_t)nUtt), fill((size_t)nSide, 0);
   for (int u = 0; u < nUtt; u++) { sideOff[uttSide[u] + 1]++; nFrames[uttSide[u]] += frameOff[u + 1] - frameOff[u]; }
   for (int s = 0; s < nSide; s++) sideOff[s + 1] += sideOff[s];
   for (int u = 0; u < nUtt; u++) sideUtt[sideOff[uttSide[u]] + fill[uttSide[u]]++] = u;
   hipStream_t st = (hipStream_t)stream;
   DevScratch b;
   int rc;
   int *dOff = nullptr, *dSideOff = nullptr, *dSideUtt = nullptr;
   double *dPart = nullptr, *dOut = nullptr;
   if ((rc = b.get(&dOff, (size_t)nUtt + 1)) || (rc = b.get(&dSideOff, sideOff.size())) || (rc = b.get(&dSideUtt, sideUtt.size())) ||
       (rc = b.get(&dPart, (size_t)nUtt * 2 * D)) || (rc = b.get(&dOut, (size_t)nSide * 2 * D)))
      return rc;
   HIPCHECK(hipMemcpyAsync(dOff, frameOff, sizeof(int) * ((size_t)nUtt + 1), hipMemcpyHostToDevice, st));
   HIPCHECK(hipMemcpyAsync(dSideOff, sideOff.data(), sizeof(int) * sideOff.size(), hipMemcpyHostToDevice, st));
   HIPCHECK(hipMemcpyAsync(dSideUtt, sideUtt.data(), sizeof(int) * sideUtt.size(), hipMemcpyHostToDevice, st));
   const int nChunk = (D + SS_LANES - 1) / SS_LANES;
   if (nChunk > 65535) { htkamd_set_error("side_stats: %d columns", D); return HTKAMD_EINVAL; }
   hipLaunchKernelGGL(k_side_partial, dim3((unsigned)nUtt, (unsigned)nChunk), dim3(SS_WAVES * SS_LANES), 0, st, dX, dOff, nCols, D, dPart);
   HIPCHECK(hipGetLastError());
   const size_t n = (size_t)nSide * 2 * D;
   hipLaunchKernelGGL(k_side_merge, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dPart, dSideOff, dSideUtt, nSide, D, dOut);
   HIPCHECK(hipGetLastError());
   std::vector<double> h(n);
   HIPCHECK(hipMemcpyAsync(h.data(), dOut, sizeof(double) * n, hipMemcpyDeviceToHost, st));
   HIPCHECK(hipStreamSynchronize(st));
   for (int s = 0; s < nSide; s++)
      for (int i = 0; i < D; i++) { sum[(size_t)s * D + i] = h[(size_t)s * 2 * D + i]; sqsum[(size_t)s * D + i] = h[(size_t)s * 2 * D + D + i]; }
   return HTKAMD_OK;
}

extern "C" int htkamd_parm_normalise(float *dX, const int *frameOff, const int *uttSide, int nUtt, int nSide, int nCols,
                                     const float *mean, int dMean, const float *scale, int dScale, void *stream)
{
   int F = 0;
   if (!mean) dMean = 0;
   if (!scale) dScale = 0;
   if (nCols < 1 || dMean < 0 || dScale < 0 || dMean > nCols || dScale > nCols) {
      htkamd_set_error("parm_normalise: %d mean and %d scale columns for rows of %d", dMean, dScale, nCols); return HTKAMD_EINVAL;
   }
   { const int rc = check_batch("parm_normalise", frameOff, uttSide, nUtt, nSide, &F); if (rc) return rc; }
   if (F > 0 && !dX) { htkamd_set_error("parm_normalise: NULL table"); return HTKAMD_EINVAL; }
   if (htkamd_device_count() <= 0) { htkamd_set_error("parm_normalise: no HIP device"); return HTKAMD_ENODEV; }
   const int W = dMean > dScale ? dMean : dScale;
   if (F == 0 || W == 0) return HTKAMD_OK;
   hipStream_t st = (hipStream_t)stream;
   DevScratch b;
   int rc;
   int *dOff = nullptr, *dUttSide = nullptr, *dRowSide = nullptr;
   float *dMeanTab = nullptr, *dScaleTab = nullptr;
   if ((rc = b.get(&dOff, (size_t)nUtt + 1)) || (rc = b.get(&dUttSide, (size_t)nUtt)) || (rc = b.get(&dRowSide, (size_t)F)) ||
       (rc = b.get(&dMeanTab, (size_t)nSide * dMean)) || (rc = b.get(&dScaleTab, (size_t)nSide * dScale)))
      return rc;
   HIPCHECK(hipMemcpyAsync(dOff, frameOff, sizeof(int) * ((size_t)nUtt + 1), hipMemcpyHostToDevice, st));
   HIPCHECK(hipMemcpyAsync(dUttSide, uttSide, sizeof(int) * (size_t)nUtt, hipMemcpyHostToDevice, st));
   if (dMean) HIPCHECK(hipMemcpyAsync(dMeanTab, mean, sizeof(float) * (size_t)nSide * dMean, hipMemcpyHostToDevice, st));
   if (dScale) HIPCHECK(hipMemcpyAsync(dScaleTab, scale, sizeof(float) * (size_t)nSide * dScale, hipMemcpyHostToDevice, st));
   hipLaunchKernelGGL(k_row_side, dim3((unsigned)(((size_t)F + 255) / 256)), dim3(256), 0, st, dOff, dUttSide, nUtt, F, dRowSide);
   HIPCHECK(hipGetLastError());
   const size_t n = (size_t)F * W;
   hipLaunchKernelGGL(k_side_normalise, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dX, dRowSide, (size_t)F, nCols, W, dMeanTab, dMean, dScaleTab, dScale);
   HIPCHECK(hipGetLastError());
   HIPCHECK(hipStreamSynchronize(st));                   // (the tables and offsets are the caller's: the copies above must be over when the call returns)
   return HTKAMD_OK;
}
