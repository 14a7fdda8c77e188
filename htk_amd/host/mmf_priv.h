/* mmf_priv.h -- the model-set holder of mmf.c (struct htkamd_mmf) for the host files that edit a loaded set in place (mmf.c itself:
 * MU; treeclust.c: RO/QS/TB/ST, TC/NC/TI, LT/AU/CO).  Not part of the public interface. */
#ifndef HTKAMD_MMF_PRIV_H
#define HTKAMD_MMF_PRIV_H
#include "../csrc/internal.h"

typedef struct { char *name; int nMix; int comp0; int inlineOwner; int src; int *sMix; float *sw; int dur; } mmf_state;   /* name NULL = un-named (inline); src: index of the file it came from;
   several streams: nMix = all components of the state, sMix[s] those of stream s (consecutive from comp0), sw = <SWEIGHTS> or NULL; dur: its duration vector (dm[]) or -1 */
typedef struct { char *name; int N; int off; int src; } mmf_trans;
typedef struct { char *name; int N; int *state; int trans; int src; int dur; } mmf_hmm;     /* src: index of the file it came from; dur: the model's duration vector (dm[]) or -1 */

/* The trees HHEd keeps between commands (treeList and the question list, HHEd.c:2421 / qHead): left by TB, read by LT, used by AU and ST.
   A question's patterns stand in QS order (htkamd_trees_write's convention: the file shows them last first); node n of a tree asks question
   quest[n], no[n] / yes[n] >= 0 is a node, < 0 the leaf -1-k whose ~s macro is leaf[k]; nNodes = 0: the single leaf leaf[0]. */
typedef struct { char *name; int nPat; char **pat; } mmf_quest;
typedef struct { char *name; int state, nNodes, nLeaves; int *quest, *no, *yes; char **leaf; } mmf_tree;
typedef struct { mmf_quest *q; int nQ; mmf_tree *t; int nT; } mmf_trees;

struct htkamd_mmf {
   int vecSize, streamWidth, hasOpts;
   int nStreams, swidth[8], *dimStream, curStream;                  /* several streams (<STREAMINFO> S w1..wS): dimension -> stream over the undivided vector */
   char kind[64], cov[16], dur[16], setId[128];
   /* pools */
   mmf_state *st; int nSt, capSt;
   float *wt; int *cg; int nComp, capComp;
   float *mean, *var, *gconst; unsigned char *hasG; int nG, capG;
   char **gName; int *gSrc; int capGN;                              /* ~m macro name of Gaussian g or NULL, and the file it was defined in */
   mmf_trans *tr; int nTr, capTr; float *tp; int nTp, capTp;       /* tp: LOG transition values */
   mmf_hmm *hm; int nHm, capHm;
   float *varFloor;                                                 /* ~v "varFloor1" or NULL */
   /* shared vectors: ~u (means) and ~v (variances) macros; gMeanMac/gVarMac[g] = macro of Gaussian g's mean / variance or -1 */
   struct { char type; char *name; float *v; int src; int stream; } *vm; int nVm, capVm;      /* stream: of a varFloorN macro of a multi-stream set, else -1 */
   int *gMeanMac, *gVarMac; int capMac;
   /* ~w stream-weight macros (GetSWeights HModel.c:1621): nStreams numbers under a name; a state that names one takes a copy (the set is written
      back with <SWEIGHTS> in the states) */
   struct { char *name; float w[8]; } *wm; int nWm, capWm;
   /* duration vectors (GetDuration HModel.c:1580, PutDuration :2840): <DURATION> n v1..vn behind a state's streams or a model's transition matrix, inline or as
      a ~d macro.  Nothing on the path reads them (HERest / HVite neither): they are carried and written back where they stood */
   struct { char *name; int n; float *v; int src; } *dm; int nDm, capDm;
   /* logical list */
   char **logName; int *logPhys; int nLog; int *logSorted;        /* logSorted: list positions in name order (stable) */
   /* desc arrays */
   htkamd_model_desc d; int *stateCompOff, *transN, *transOff, *hmmTrans, *hmmStateOff, *hmmState;
   int *gStr;                                                       /* stream of Gaussian g */
   float *swAll;                                                    /* [nSt*NS] stream weights for the desc */
   int tiedMix;                                                     /* hsKind TIEDHS: <TMIX> streams (GetStream HModel.c:1878-1892) */
   /* full covariances (<FULLC>, <INVCOVAR> D + the lower triangle; GetCovar HModel.c:1511, ReadTriMat HMath.c:406): per Gaussian the
      triangle packed row-major, element (i, j), j <= i, at i(i+1)/2 + j; allocated on the first <INVCOVAR> or <FULLC> only */
   float *icov; int capIcov, fullc, sawVar, sawInv;
   char *tmName[8]; int tmM[8];                                     /* per stream: generic ~m macro name and pool size (tmRecs[s].mixId / nMix) */
   int *gPend; int capPend, lastVecN;                                         /* a ~m macro of a multi-stream set read before its stream is known: its width, values at [0..width) of the row */
   /* input transforms (GetInputXForm HModel.c:2373): the ~j macros met so far, and the set's own (<INPUTXFORM> of the global options:
      one of jm[], or an inline body that the set owns) */
   struct htkamd_inputxform **jm; int nJm, capJm;
   struct htkamd_inputxform *xf; int xfInline;
   int finished, nFiles;
   /* HHEd's synthesis commands (treeclust.c: LT / AU / CO).  hmCreate / logCreate: the physical / logical models in the order their
      macros were made, where that is no longer the order of hm[] / logName[] (SwapLists and CompactCommand re-make them); NULL = array order.
      The reference's scan of the macro table (htkamd_hmm_scan_order) takes the names in this order. */
   mmf_trees *trees;
   int *hmCreate, *logCreate;
};

void htkamd_mmf_trees_free(mmf_trees *t);

/* treeclust.c's helpers that treesynth.c shares (library-internal names) */
#define tc_match        htkamd_tc_match
#define tc_logical_walk htkamd_tc_logical_walk
#define tc_compact      htkamd_tc_compact
#define dc_fix_gconsts  htkamd_dc_fix_gconsts
#define st_hold         htkamd_st_hold
int  tc_match(const char *s, const char *p);                      /* DoMatch */
int *tc_logical_walk(const struct htkamd_mmf *s);                 /* the logical names in the macro table's order (malloc'd) */
void tc_compact(struct htkamd_mmf *s, const int *newSeq, int nNew);   /* drops states nobody uses, rebuilds the state side of the description */
void dc_fix_gconsts(struct htkamd_mmf *s);                        /* FixAllGConsts (DIAGC) */
void st_hold(struct htkamd_mmf *s, const htkamd_tree_question *q, int nQ, const htkamd_tree_desc *t, int nT);   /* TB's trees stay on the holder */

#endif
