/* latrescore.h -- the lattice set as host/latrescore.c (dictionary, files, orders, text) and csrc/latrescore.hip (the device side) share
 * it, and the one statement of LArcTotLike. */
#ifndef HTKAMD_LATRESCORE_H
#define HTKAMD_LATRESCORE_H
#include "internal.h"

#if defined(__HIPCC__)
#define HTKAMD_HD __host__ __device__
#else
#define HTKAMD_HD
#endif

/* LArcTotLike (HNet.h:257): the three scaled likelihoods summed in float, the word penalty added in DOUBLE (the macro's `? 0.0 :
   wdpenalty` makes the last operand a double); nullEnd: the arc's end node carries no word or !NULL.  Compiled with -ffp-contract=off. */
static inline HTKAMD_HD double htkamd_larc_tot_like(float ac, float lm, float pr, float acScale, float lmScale, float prScale, float wordPen, int nullEnd)
{
   const float a = ac * acScale, l = lm * lmScale, p = pr * prScale;
   return (double)((a + l) + p) + (nullEnd ? 0.0 : (double)wordPen);
}

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { int pnum; char *outSym; } htkamd_lat_pron;                 /* outSym NULL: `[]` in the dictionary */
typedef struct { char *name; int nProns; htkamd_lat_pron *pron; } htkamd_lat_word;
typedef struct {                                                            /* shared by the sets made with htkamd_latset_create_like */
   int refs;
   int nWords, capWords; htkamd_lat_word *word;                             /* [0] = !NULL, [1] = !SUBLATID */
   int *hash; int hashCap;
} htkamd_lat_dict;

typedef struct { char *label; float dur, like; } htkamd_lat_align;       /* LAlign (HNet.h:103): one record of an arc's d= field */
typedef struct {
   int nn, na, start, end;
   double *nodeTime; int *nodeWord, *nodeVar;
   int *arcStart, *arcEnd; float *arcAc, *arcLm, *arcPr;
   int *arcNAlign; htkamd_lat_align **arcAlign;                           /* [na]; NULL arrays: no arc has records */
   int *topOrder, *fwdArcs, *bwdArcs;
   char *utterance, *vocab, *hmms, *lmName;
   float logbase, tscale;
} htkamd_lat_one;

struct htkamd_latset {
   htkamd_lat_dict *dict;
   int nLats, capLats; htkamd_lat_one *lat;
   long long totalNodes, totalArcs;
   int latsOnDevice;                       /* lattices the device copy holds */
   void *dev; void (*devFree)(void *);     /* csrc/latrescore.hip's buffers (set where they are made: the host code links without the device side) */
   double kernelMs;
};

#ifdef __cplusplus
}
#endif
#endif
