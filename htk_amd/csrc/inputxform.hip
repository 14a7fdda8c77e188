// inputxform.hip -- the global linear input transform on the device: ApplyStaticMat (HTKLib/HParm.c:1235-1280), the last step of
// AddQualifiers (:1834-1843; with <PREQUAL> its first, :1645-1652).  The transform itself -- <INPUTXFORM> of a model set, a ~j macro,
// a file of its own -- is read, checked and written by host/mmf.c.
//
// The reference hard-wires preFrames = postFrames = 0, so a row depends on no other row: out[r][j] = sum over m of M[j][m] * in[r][m],
// each output starting at 0.0f, m ascending, the product and the sum each rounded to float (no fused multiply-add; subnormals kept).
//
// k_parm_xform: a wavefront owns 64 rows, a lane one row.
//   - The 64 rows are staged through LDS on the way in and on the way out, so that the global reads and writes of a wavefront run
//     through the rows' bytes in order (rows of 39..52 floats read lane-per-row would touch 64 cache lines per instruction).  The LDS
//     row stride is odd, so that the lane-per-row accesses of the staging area spread over the banks.
//   - A lane holds its mcols inputs in registers (x[MC], MC the instantiation's bound).
//   - The matrix is the same for every lane: it is read through the constant address space at wavefront-uniform addresses, which the
//     compiler turns into scalar loads (s_load_dwordx8 and the like) whose results the multiplies take as scalar operands -- no
//     vector memory access and no LDS access per multiply.  Two vector instructions per multiply-add (v_mul_f32, v_add_f32) remain.
//   - One buffer serves both directions: the inputs are in registers before the first output is stored.
// In place (out == in, equal strides) is safe: a wavefront reads only its own rows, and all of them before it writes any.
#include <hip/hip_runtime.h>
#include "internal.h"
#include "hipcheck.h"
#include "devbuf.h"

// Product and sum are rounded separately: the project builds every file with -ffp-contract=off, and the two helpers are compiled under
// a pragma that turns contraction off besides, which every mode that honours pragmas respects (off, on, fast-honor-pragmas -- hipcc's
// default for device code --, and hipcc's -ffp-contract=fast as this toolchain passes it on: the assembly holds no v_fma / v_fmac under
// any of the four).  clang's own `fast` mode is documented to fuse across statements and to disregard the pragma: a build that hands
// that to the device compiler is not the reference's arithmetic, and tests/test_gpu_inputxform.py fails on it.  (The toolchain's
// __fmul_rn / __fadd_rn are plain `x * y` / `x + y` inlined from a header compiled under the command line's contraction state and
// fuse under fast-honor-pragmas already, so they are not used.)
#pragma clang fp contract(off)
static __device__ __forceinline__ float xf_mul_rn(float a, float b) { return a * b; }
static __device__ __forceinline__ float xf_add_rn(float a, float b) { return a + b; }

#define XF_LANES 64
#define XF_MAX   128                                     // widest matrix side of the register form

typedef const __attribute__((address_space(4))) float *xf_const_ptr;

template <int MC>
__global__ __launch_bounds__(XF_LANES) void k_parm_xform(const float *in, int inCols, float *out, int outCols, long long nRows,
                                                          const float *mat, int mrows, int mcols, int stride)
{
   extern __shared__ float lds[];                        // [64 rows x stride], stride = max(mrows, mcols) | 1
   const int lane = threadIdx.x;
   const long long r0 = (long long)blockIdx.x * XF_LANES;
   const long long left = nRows - r0;
   const int nr = left < XF_LANES ? (int)left : XF_LANES;
   {  // rows in: element i of the wavefront's nr x mcols values goes to lane i % 64; (row, col) advance by 64 without a division
      const int dRow = XF_LANES / mcols, dCol = XF_LANES % mcols, n = nr * mcols;
      int row = lane / mcols, col = lane % mcols;
      for (int i = lane; i < n; i += XF_LANES) {
         lds[row * stride + col] = in[(size_t)(r0 + row) * inCols + col];
         row += dRow; col += dCol;
         if (col >= mcols) { col -= mcols; row++; }
      }
   }
   __syncthreads();
   float x[MC];
#pragma unroll
   for (int m = 0; m < MC; m++) x[m] = (m < mcols) ? lds[lane * stride + m] : 0.0f;      // (a lane beyond nr reads what the buffer holds: in bounds, never stored)
   __syncthreads();
   const xf_const_ptr cm = (xf_const_ptr)mat;
   for (int j = 0; j < mrows; j++) {
      const xf_const_ptr mr = cm + (size_t)j * mcols;
      float acc = 0.0f;
#pragma unroll
      for (int m0 = 0; m0 < MC; m0 += 8) {
         if (m0 + 8 <= mcols) {
#pragma unroll
            for (int k = 0; k < 8; k++) acc = xf_add_rn(acc, xf_mul_rn(mr[m0 + k], x[m0 + k]));
         } else {
#pragma unroll
            for (int k = 0; k < 8; k++) if (m0 + k < mcols) acc = xf_add_rn(acc, xf_mul_rn(mr[m0 + k], x[m0 + k]));
         }
      }
      lds[lane * stride + j] = acc;
   }
   __syncthreads();
   {  // rows out
      const int dRow = XF_LANES / mrows, dCol = XF_LANES % mrows, n = nr * mrows;
      int row = lane / mrows, col = lane % mrows;
      for (int i = lane; i < n; i += XF_LANES) {
         out[(size_t)(r0 + row) * outCols + col] = lds[row * stride + col];
         row += dRow; col += dCol;
         if (col >= mrows) { col -= mrows; row++; }
      }
   }
}

extern "C" int htkamd_parm_xform(const float *dIn, int inCols, float *dOut, int outCols, long long nRows,
                                 const float *dMat, int mrows, int mcols, void *stream)
{
   if (nRows < 0 || mrows < 1 || mcols < 1 || inCols < 1 || outCols < 1) { htkamd_set_error("parm_xform: bad argument"); return HTKAMD_EINVAL; }
   if (mrows > XF_MAX || mcols > XF_MAX) { htkamd_set_error("parm_xform: a %d x %d matrix (at most %d x %d)", mrows, mcols, XF_MAX, XF_MAX); return HTKAMD_EINVAL; }
   if (mcols > inCols) { htkamd_set_error("parm_xform: %d matrix columns for input rows of %d", mcols, inCols); return HTKAMD_EINVAL; }
   if (mrows > outCols) { htkamd_set_error("parm_xform: %d matrix rows for output rows of %d", mrows, outCols); return HTKAMD_EINVAL; }
   if ((const float *)dOut == dIn && dIn && inCols != outCols) { htkamd_set_error("parm_xform: in place needs equal row widths (%d and %d)", inCols, outCols); return HTKAMD_EINVAL; }
   if (nRows > 0 && (!dIn || !dOut || !dMat)) { htkamd_set_error("parm_xform: NULL table"); return HTKAMD_EINVAL; }
   if (htkamd_device_count() <= 0) { htkamd_set_error("parm_xform: no HIP device"); return HTKAMD_ENODEV; }
   if (nRows == 0) return HTKAMD_OK;
   const long long nBlocks = (nRows + XF_LANES - 1) / XF_LANES;
   if (nBlocks > 0x7fffffffLL) { htkamd_set_error("parm_xform: %lld rows", nRows); return HTKAMD_EINVAL; }
   hipStream_t st = (hipStream_t)stream;
   const int stride = (mrows > mcols ? mrows : mcols) | 1;
   const size_t ldsBytes = sizeof(float) * XF_LANES * (size_t)stride;         // at most 64 x 129 floats = 33 KB
   const dim3 grid((unsigned)nBlocks), block(XF_LANES);
   if (mcols <= 16) hipLaunchKernelGGL(k_parm_xform<16>, grid, block, ldsBytes, st, dIn, inCols, dOut, outCols, nRows, dMat, mrows, mcols, stride);
   else if (mcols <= 40) hipLaunchKernelGGL(k_parm_xform<40>, grid, block, ldsBytes, st, dIn, inCols, dOut, outCols, nRows, dMat, mrows, mcols, stride);
   else if (mcols <= 64) hipLaunchKernelGGL(k_parm_xform<64>, grid, block, ldsBytes, st, dIn, inCols, dOut, outCols, nRows, dMat, mrows, mcols, stride);
   else hipLaunchKernelGGL(k_parm_xform<128>, grid, block, ldsBytes, st, dIn, inCols, dOut, outCols, nRows, dMat, mrows, mcols, stride);
   HIPCHECK(hipGetLastError());
   return HTKAMD_OK;
}

// ------------------------------------------------------------------------------------ the qualifier step of a transformed set
extern "C" int htkamd_inputxform_apply_cols(const htkamd_inputxform *x, const htkamd_parm_quals *q)
{
   if (!x || !q || q->nStat <= 0) return 0;
   if (!x->preQual) return x->mrows;
   return x->mrows * (1 + (q->hasD ? 1 : 0) + (q->hasA ? 1 : 0) + (q->hasT ? 1 : 0));
}

DEVBUF_OWNER("inputxform_apply")

extern "C" int htkamd_inputxform_apply(const htkamd_inputxform *x, const float *dStatic, const int *frameOff, int nUtt,
                                       const htkamd_parm_quals *q, float *dOut, void *stream)
{
   if (!x || !q || !frameOff || nUtt < 0 || q->nStat <= 0) { htkamd_set_error("inputxform_apply: bad argument"); return HTKAMD_EINVAL; }
   if (q->nullECol >= 0) { htkamd_set_error("inputxform_apply: _N together with an input transform is not supported"); return HTKAMD_EINVAL; }
   const int qCols = htkamd_parm_quals_cols(q);
   const int width = x->preQual ? q->nStat : qCols;
   if (x->mcols != width) { htkamd_set_error("input transform: %d matrix columns for rows of %d values", x->mcols, width); return HTKAMD_EINVAL; }
   if (x->mrows > XF_MAX || x->mcols > XF_MAX) { htkamd_set_error("input transform: a %d x %d matrix (at most %d x %d)", x->mrows, x->mcols, XF_MAX, XF_MAX); return HTKAMD_EINVAL; }
   if (htkamd_device_count() <= 0) { htkamd_set_error("inputxform_apply: no HIP device"); return HTKAMD_ENODEV; }
   const long long F = nUtt ? frameOff[nUtt] : 0;
   if (F == 0) return HTKAMD_OK;
   if (!dStatic || !dOut) { htkamd_set_error("inputxform_apply: NULL table"); return HTKAMD_EINVAL; }
   hipStream_t st = (hipStream_t)stream;
   DevScratch b;
   float *dMat = nullptr, *dTmp = nullptr;
   int rc;
   if ((rc = b.get(&dMat, (size_t)x->mrows * x->mcols))) return rc;
   HIPCHECK(hipMemcpyAsync(dMat, x->mat, sizeof(float) * (size_t)x->mrows * x->mcols, hipMemcpyHostToDevice, st));
   if (!x->preQual) {                                    // the qualifiers, then the transform over the whole row (HParm.c:1834-1843)
      if ((rc = b.get(&dTmp, (size_t)F * qCols))) return rc;
      if ((rc = htkamd_parm_qualify(dStatic, frameOff, nUtt, q, dTmp, stream))) return rc;
      if ((rc = htkamd_parm_xform(dTmp, qCols, dOut, x->mrows, F, dMat, x->mrows, x->mcols, stream))) return rc;
   } else {                                              // the transform over the statics, then the qualifiers on mrows statics (HParm.c:1645-1652)
      htkamd_parm_quals q2 = *q;
      q2.nStat = x->mrows;
      q2.nZeroMean = q->nZeroMean > 0 ? x->mrows : 0;    // "No idea where the statics are so do everything" (HParm.c:1716-1720): base + C0 + energy = every static
      if ((rc = b.get(&dTmp, (size_t)F * x->mrows))) return rc;
      if ((rc = htkamd_parm_xform(dStatic, q->nStat, dTmp, x->mrows, F, dMat, x->mrows, x->mcols, stream))) return rc;
      if ((rc = htkamd_parm_qualify(dTmp, frameOff, nUtt, &q2, dOut, stream))) return rc;
   }
   HIPCHECK(hipStreamSynchronize(st));                   // (the scratch is released on return)
   return HTKAMD_OK;
}
