/* compv_full.c -- from one class's full-covariance statistics (csrc/compv_full.hip) to what a <FULLC> Gaussian holds: CalcCovs
 * (HTKTools/HCompV.c:261-297) restated in double.  The reference divides and subtracts in float; this keeps fp64 until the results are
 * stored, so the two agree to the reference's own rounding.  Pure host code.
 *
 * Triangles are packed row-major: (x, y), y <= x, at x (x + 1) / 2 + y -- the order of the reference's TriMat and of an MMF's <InvCovar>.
 */
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include "../csrc/internal.h"

#define TRI(x, y) ((size_t)(x) * ((x) + 1) / 2 + (y))

/* Choleski factor L (lower, packed) of the packed symmetric matrix a, in place (Choleski HMath.c:514, which CovInvert :567 reports as
   its error 5220): 0, or -1 where a pivot is not positive.  The reference asks sum <= 0.0; a pivot below the rounding error of its own
   sum, D eps a[i][i], is no information either, so a matrix that is singular in exact arithmetic (two equal columns) is refused whatever
   sign its last bits leave. */
static int choleski(int D, double *a)
{
   for (int i = 0; i < D; i++)
      for (int j = 0; j <= i; j++) {
         const double diag = a[TRI(i, j)];
         double s = diag;
         for (int k = 0; k < j; k++) s -= a[TRI(i, k)] * a[TRI(j, k)];
         if (i == j) {
            if (!(s > D * DBL_EPSILON * diag)) return -1;
            a[TRI(i, i)] = sqrt(s);
         } else
            a[TRI(i, j)] = s / a[TRI(j, j)];
      }
   return 0;
}

/* inv = (L L^T)^-1, its lower triangle: column c of the inverse by the two triangular solves of MSolve (HMath.c:542), rows c .. D-1 kept */
static void chol_invert(int D, const double *L, double *col, double *inv)
{
   for (int c = 0; c < D; c++) {
      for (int i = 0; i < D; i++) {      /* L y = e_c */
         double s = (i == c) ? 1.0 : 0.0;
         for (int k = 0; k < i; k++) s -= L[TRI(i, k)] * col[k];
         col[i] = s / L[TRI(i, i)];
      }
      for (int i = D - 1; i >= 0; i--) {      /* L^T z = y */
         double s = col[i];
         for (int k = i + 1; k < D; k++) s -= L[TRI(k, i)] * col[k];
         col[i] = s / L[TRI(i, i)];
      }
      for (int i = c; i < D; i++) inv[TRI(i, c)] = col[i];
   }
}

int htkamd_compv_full_cov(int D, double count, const double *sum, const double *sq, float minVar, float *mean, float *cov, float *invCov)
{
   if (D < 1 || !sum || !sq || !mean) { htkamd_set_error("compv_full_cov: bad argument"); return HTKAMD_EINVAL; }
   if (!(count >= 2.0)) {      /* CalcCovs :267-268 */
      htkamd_set_error("compv_full_cov: only %g speech frames accumulated (HCompV error 2021)", count);
      return HTKAMD_EINVAL;
   }
   const size_t tri = TRI(D, 0);
   double *c = (double *)malloc(sizeof(double) * (2 * tri + 2 * (size_t)D));
   if (!c) { htkamd_set_error("compv_full_cov: out of memory"); return HTKAMD_ENOMEM; }
   double *L = c + tri, *m = L + tri, *col = m + D;
   for (int x = 0; x < D; x++) m[x] = sum[x] / count;      /* :274-275 */
   for (int x = 0; x < D; x++)
      for (int y = 0; y <= x; y++) {      /* :279-284: the floor on the diagonal only */
         const double v = sq[TRI(x, y)] / count - m[x] * m[y];
         c[TRI(x, y)] = (x != y || v > (double)minVar) ? v : (double)minVar;
      }
   int rc = HTKAMD_OK;
   if (invCov) {      /* :291-296 */
      for (size_t q = 0; q < tri; q++) L[q] = c[q];
      if (choleski(D, L)) {
         htkamd_set_error("compv_full_cov: the covariance matrix is not positive definite and cannot be inverted (the reference's 5220)");
         rc = HTKAMD_EMODEL;
      }
   }
   if (!rc) {
      for (int x = 0; x < D; x++) mean[x] = (float)m[x];
      if (cov) for (size_t q = 0; q < tri; q++) cov[q] = (float)c[q];
      if (invCov) {
         chol_invert(D, L, col, c);      /* (c is free now) */
         for (size_t q = 0; q < tri; q++) invCov[q] = (float)c[q];
      }
   }
   free(c);
   return rc;
}
