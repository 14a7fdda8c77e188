/* vquant.h -- the VQ table as host/vqtab.c holds it and csrc/vquant.hip codes with it. */
#ifndef HTKAMD_VQUANT_H
#define HTKAMD_VQUANT_H
#include "internal.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VQ_SMAX      4                        /* streams 1 .. SMAX-1 (HModel.h SMAX 5) */
#define VQ_MAXNODES  32767                    /* what a short node id can name */

/* one stream's nodes in the order the coder walks them: a linear table's list, a tree in StoreTree's order (root first) */
typedef struct {
   int n, width, covLen;
   int *vqidx, *left, *right;                 /* children as indices into this order, -1 none */
   float *gconst, *mean, *cov;                /* [n], [n x width], [n x covLen] */
} vq_stream;

struct htkamd_vqtab {
   int magic, type, kind, nStreams;
   vq_stream st[VQ_SMAX];
   void *dev;                                 /* the coder's copy on the device, made on first use */
   void (*devFree)(void *);
   double codeMs;
};

/* CovInvert (HMath.c:567) of a packed lower triangle into a packed lower triangle, Choleski and both substitutions in double; -1: not
   positive definite */
int htkamd_host_cov_invert(int D, const float *tri, float *inv);

#ifdef __cplusplus
}
#endif
#endif
