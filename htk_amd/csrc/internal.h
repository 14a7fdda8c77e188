/* internal.h -- shared declarations of the htk_amd native library (not part of the C ABI). */
#ifndef HTKAMD_INTERNAL_H
#define HTKAMD_INTERNAL_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/htk_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* HTK constants (HMath.h:42-45, HModel.h:52-53) */
#define LZERO    (-1.0E10)
#define LSMALL   (-0.5E10)
#define MINEARG  (-708.3)
#define MINLARG  2.45E-308
#define HTK_TPI  6.28318530717959
#define MINMIX   1.0E-5
#define LMINMIX  (-11.5129254649702)

void htkamd_set_error(const char *fmt, ...);

/* ---- the SLF text both lattice writers share (htk_amd/host/slfout.c) ---- */
void htkamd_slf_put_word(FILE *f, const char *s);                               /* "W=%-19s ", quoted only when needed */
void htkamd_slf_sort_arcs(int *order, int nArcs, const int *arcStart, const int *arcEnd, const int *nodeRank);   /* QSCmpArcs (HNet.c:466) */

/* ---- host-side preparation (htk_amd/host/prep.c) ---- */
void   htkamd_host_fix_diag_gconst(int D, const float *var, float *gconst);   /* HModel.c:5641 */
void   htkamd_host_conv_diagc(size_t n, const float *var, float *ivar);        /* HUtil.c:413  */
int    htkamd_host_fix_full_gconst(int D, const float *tri, float *gconst);    /* HModel.c:5682 + CovDet HMath.c:593; -1: not positive definite */
float  htkamd_host_mix_log_weight(float w);                                    /* HModel.c:5288 */
int    htkamd_host_min_dur(int N, const float *tp);                            /* HFB.c:106    */
int    htkamd_host_stream_dims(const char *kind, int vecSize, int S, const int *width, int *dimStream, char *why, size_t whyLen);   /* HParm.c:3094,2843 */
void   htkamd_host_fix_diag_gconst_ms(int D, const float *var, const int *dimStream, int stream, float *gconst);
int    htkamd_host_trans_is_lr(int N, const float *tp);                        /* left-to-right, no skips (fb_lr.hip) */
double htkamd_host_min_log_exp(void);                                          /* HMath.c:1680 */

/* ---- decision-tree clustering: the device side (csrc/treeclust.hip) as host/treeclust.c drives it ----
 * A node is its item list: idx[offA .. offA+nA), then idx[offB .. offB+nB) (nB > 0: "list a, then list b" of a merge candidate).
 * C = 2D+1 floats per accumulator: occ, sum[D], sqr[D].  htkamd_tree_dev_split leaves every node's [nQ+1][2][C] block (question q: no
 * side, yes side; the last entry is "no question" = the node's total on the no side) on the device and returns one record per node:
 *   rec[0] = number of candidate questions (an int; more than HTKAMD_TREE_MAXCAND: fetch the block with htkamd_tree_dev_block),
 *   rec[1 .. MAXCAND] = their numbers in question order (ints), then the total [C], then the candidates' [2][C] sums. */
#define HTKAMD_TREE_MAXCAND 8
#define HTKAMD_TREE_REC(C) (1 + HTKAMD_TREE_MAXCAND + (C) + HTKAMD_TREE_MAXCAND * 2 * (C))
typedef struct { int offA, nA, offB, nB; } htkamd_tree_node;
typedef struct htkamd_tree_dev htkamd_tree_dev;
int  htkamd_tree_dev_open(htkamd_tree_dev **out, const float *itemStats, int nItems, int D, const int *itemCol /*[nItems] or NULL = the item itself*/,
                          const unsigned char *answers /*[nQ][nCols]*/, int nCols, int nQ, void *stream);
int  htkamd_tree_dev_split(htkamd_tree_dev *t, const htkamd_tree_node *nodes, int nNodes, const int *idx, int nIdx, float outlierThresh, int *rec /*[nNodes][HTKAMD_TREE_REC(C)]*/);
int  htkamd_tree_dev_totals(htkamd_tree_dev *t, const htkamd_tree_node *nodes, int nNodes, const int *idx, int nIdx, float *tot /*[nNodes][C]*/);
int  htkamd_tree_dev_block(htkamd_tree_dev *t, int node, float *blk /*[nQ+1][2][C]*/);      /* of the last htkamd_tree_dev_split */
void htkamd_tree_dev_close(htkamd_tree_dev *t);

/* ---- data-driven clustering: the device side (csrc/datacluster.hip) as host/treeclust.c drives it ----
 * The commands of a call own consecutive item ranges (off = the items before it).  The distances come from exactly one of: idist (the
 * caller's [n][n] matrices, command after command), mean / var (a row of V values per item: Divergence), or desc / itemState (the set
 * and every item's state: GDistance over the exact scoring path).  merges: per command at 2 * off the pairs (i, j), 1-based in the
 * numbering current at that merge; nMerges[command] how many. */
#define HTKAMD_DC_MAXITEMS 3000                        /* items of one command: five words of LDS each */
typedef struct { int off, n, numReq; float threshold; } htkamd_dc_cmd;
typedef struct {
   int nCmds; const htkamd_dc_cmd *cmds; int nItems;
   const float *idist;
   const float *mean, *var; int V;
   const htkamd_model_desc *desc; const int *itemState;
   const float *occ; float outlierThresh;              /* occ: per item, or NULL = no outlier phase */
   int noMerge;                                        /* distances only */
} htkamd_dc_job;
int  htkamd_dc_dev_run(const htkamd_dc_job *job, float *idistOut /* or NULL */, int *merges /*[2 * nItems]*/, int *nMerges /*[nCmds]*/, void *stream);

/* ---- regression class trees: the device side (csrc/regtree.hip) as host/regtree.c drives it ----
 * A member is one Gaussian of the scan: row m of mean / sum / sqr ([G][D]), occ[m], hasAcc[m] (0: no AccSum record, HHEd's hook == NULL).
 * The member list starts as 0 .. G-1; a node is a range [off, off+n) of it, and a split leaves the left child's members in
 * [off, off+nLeft) and the right child's behind them, both in the order they had.  A node's figures are 2D+2 floats: aveMean[D],
 * aveCovar[D], clustAcc, clusterScore. */
#define HTKAMD_RT_MAXDIM  960                          /* one lane per dimension and one for occupation and score, in one workgroup */
#define HTKAMD_RT_MAXITER 500                          /* MAX_ITER (HHEd.c:61) */
typedef struct htkamd_rt_dev htkamd_rt_dev;
int  htkamd_rt_dev_open(htkamd_rt_dev **out, const float *mean, const float *sum, const float *sqr, const float *occ, const unsigned char *hasAcc,
                        int G, int D, void *stream);
int  htkamd_rt_dev_node(htkamd_rt_dev *t, int off, int n, float *node /*[2D+2]*/);
int  htkamd_rt_dev_split(htkamd_rt_dev *t, int off, int n, const float *seeds /*[2][D]*/, int *counts /*nLeft, nRight, CalcDistance calls*/,
                         float *nodes /*[2][2D+2]*/);
int  htkamd_rt_dev_list(htkamd_rt_dev *t, int *list /*[G]*/);
float htkamd_rt_dev_kernel_ms(const htkamd_rt_dev *t);
void htkamd_rt_dev_close(htkamd_rt_dev *t);

/* ---- MLLR mean transforms: the device side (csrc/mllr.hip) as host/mllr.c drives it ----
 * A job: the set's Gaussians (mean, var [G][D]; occ [G] and spSum [G][D] as the floats the reference keeps), the base classes as member
 * lists (class c: mem[memOff[c] .. memOff[c+1])), the tree with 0-based nodes (left / right: -1 for a terminal; termClass: a terminal's
 * class, -1 for an inner node; inner: the inner nodes, children before parents).  dev_stats runs the class statistics and the sums up the
 * tree and brings back the node occupations; a node's record is htkamd_mllr_record_len doubles: per row i of a block of size bs the packed
 * lower triangle of G_i ((bs+1)(bs+2)/2), then k_i (bs+1); the node's occupation last. */
#define HTKAMD_MLLR_MAXBLOCK 64
typedef struct {
   int G, D, nBlocks, useBias, nClass, nNodes, nInner;
   const int *blockSize;
   const float *mean, *var, *occ, *spSum;
   float minOcc;
   const int *memOff, *mem, *left, *right, *termClass, *inner;
} htkamd_mllr_job;
typedef struct htkamd_mllr_dev htkamd_mllr_dev;
struct htkamd_model;
int  htkamd_mllr_dev_stats(const htkamd_mllr_job *job, htkamd_mllr_dev **out, double *nodeOcc /*[nNodes]*/, void *stream);
int  htkamd_mllr_dev_fetch(htkamd_mllr_dev *t, double *stats /*[nNodes][record]*/);
int  htkamd_mllr_dev_solve(htkamd_mllr_dev *t, int nX, const int *xNode, float *A /*[nX][D][D]*/, float *bias /*[nX][D]*/, double *W /*[nX][D][maxd] or NULL*/,
                           int *badX, int *badRow);
void htkamd_mllr_dev_times(const htkamd_mllr_dev *t, float *ms /*[3]: statistics, tree sums, solves*/);
void htkamd_mllr_dev_close(htkamd_mllr_dev *t);
int  htkamd_mllr_dev_apply(struct htkamd_model *m, int nX, const float *A, const float *bias /*or NULL*/, const int *gaussX /*[G]*/, const int *rowC0, const int *rowBs, void *stream);
int  htkamd_mllr_dev_restore(struct htkamd_model *m, void *stream);
int  htkamd_mllr_model_state(const char *who, const struct htkamd_model *m, int *D, int *G, int *adapted);   /* mllr.hip: what host/mllr.c may know of a model; EMODEL + reason for a set apply refuses */

/* ---- unseen models from the trees: the device side (csrc/treesynth.hip) as host/treeclust.c drives it ----
 * Names and patterns are NUL-terminated strings in byte pools: name n at namePool + nameOff[n] (nameOff[N] = the pool's size), pattern k
 * at patPool + patOff[k], question q owns patterns qPat[q] .. qPat[q+1]-1.  The trees' node tables lie behind one another (tree t: nodes
 * treeOff[t] .. treeOff[t+1]-1, none = a single leaf; a child >= 0 a node of the tree, < 0 the leaf -1-k, k < treeLeaves[t]); a pair is
 * (name, tree), tree -1 = none.  answers [nQ][N] bytes and leaf [nPairs] come back (either may be NULL when not wanted). */
typedef struct {
   int N; const char *namePool; const int *nameOff;
   int nQ; const char *patPool; const int *patOff, *qPat;
   int nTrees; const int *treeOff, *quest, *no, *yes, *treeLeaves;
   int nPairs; const int *pairName, *pairTree;
} htkamd_synth_job;
int  htkamd_synth_dev_run(const htkamd_synth_job *job, unsigned char *answers, int *leaf, void *stream);

/* ---- the aligner's results where they lie on the device (csrc/viterbi.hip), for csrc/hinit.hip: per chain state in utterance order
 * segStart / segEnd, per utterance total and status.  Valid until the handle aligns again. */
typedef struct { const int *segStart, *segEnd; const double *total; const int *status; } htkamd_viterbi_dev;
int  htkamd_viterbi_device_results(htkamd_viterbi *v, htkamd_viterbi_dev *out);

/* ---- a forward-backward pass's results where they lie on the device (csrc/fb.hip), for csrc/hrest.hip: per utterance the log
 * probability and the status word.  Valid until the handle is prepared again; written by the pass in stream order. */
typedef struct { const double *pr; const int *status; } htkamd_fb_dev;
int  htkamd_fb_device_results(htkamd_fb *fb, htkamd_fb_dev *out);

/* ---- the refusals htkamd_hinit_check and htkamd_hrest_check share (host/unit_train.c): the fields both configurations have, the prefix
 * and the tool's name as the messages carry them */
typedef struct { int maxIter, minSeg, uFlags; } htkamd_unit_cfg;
__attribute__((visibility("hidden"))) int htkamd_unit_check(const char *pfx, const char *tool, const htkamd_model_desc *d, int nFrames, int nTokens, const int *tokFrame, const int *tokLen,
                       const int *tokModel, const htkamd_unit_cfg *cfg /* NULL: the caller had none */, int nModels, const int *models);

/* device LAdd table: 4 intervals per unit of d over [minLogExp, 0] = [-23.03, 0], degree-10 Taylor rows (8 KB) */
#define LADD_INV_H 4
#define LADD_DEG   10
#define LADD_NK    93           /* floor(23.0259 * 4) + 1 */
int    htkamd_host_ladd_table_size(void);
void   htkamd_host_build_ladd_table(double *tab);

/* ---- MFCC front-end tables (htk_amd/host/fbank.c) ---- */
struct htkamd_mfcc_tables {
   int frSize, frRate, fftN, klo, khi;
   float mfnorm;
   float *ham;                 /* [frSize+1] 1-based */
   float *cepWin;              /* [numCeps+1] */
   float *loWt;                /* [fftN/2+2] 1-based */
   int *binA0, *binA1, *binB0, *binB1;   /* [numChans+2] k ranges feeding each bin (one allocation at binA0) */
   double *dct;                /* [(numCeps+1)*(numChans+1)] cos(x_j*(k-0.5)) */
   double *tw;                 /* FFT twiddles (wr,wi), stages concatenated: fftN/2 pairs */
   double *rtw;                /* Realft (yr,yi) for i = 2..fftN/4 at [2i],[2i+1] */
   short *brev;                /* [fftN/2] bit-reversed complex index */
   int takeLogs;               /* the bins are logged (MFCC, FBANK), or left linear (MELSPEC, PLP) */
   float *eql;                 /* PLP: [numChans+1] 1-based equal-loudness curve (InitPLP HSigP.c:663), at the warped centres under a warp */
   double *cm;                 /* PLP: [(lpcOrder+1)*(numChans+2)] IDFT cosines, row = lag, 0-based */
   float *edge;                /* [numChans+3] mel edges of the filters: melLo, the reference's cf[1..numChans+1] (warped under a warp), the guard */
};
int  htkamd_mfcc_tables_build(const htkamd_mfcc_config *c, struct htkamd_mfcc_tables *t);
void htkamd_mfcc_tables_free(struct htkamd_mfcc_tables *t);
/* the tables of every FFT front end (htk_amd/host/fbank.c): validates as htkamd_frontend_num_cols does, then builds the MFCC
   path's tables plus what the base kind needs after the bins; htkamd_frontend_check: the validation alone, 0 or HTKAMD_EINVAL */
int  htkamd_frontend_check(const htkamd_frontend_config *c);
int  htkamd_frontend_tables_build(const htkamd_frontend_config *c, struct htkamd_mfcc_tables *t);
/* VTLN: htkamd_frontend_check plus ValidCodeParms' checks of the warp (HParm.c:1366-1372) and the triples on which WarpFreq
   (HSigP.c:449) divides by zero or stops increasing; the tables with the filters' edges warped (InitFBank HSigP.c:513-526): loWt, the
   bins' k ranges and PLP's eql follow from them, every other table is the un-warped one.  warp NULL, or warpFreq 1.0: no warping */
int  htkamd_frontend_warp_check(const htkamd_frontend_config *c, const htkamd_warp *w);
int  htkamd_frontend_tables_build_warped(const htkamd_frontend_config *c, const htkamd_warp *w, struct htkamd_mfcc_tables *t);

/* ---- input transforms (htk_amd/host/mmf.c reads and writes them, csrc/inputxform.hip applies them) ---- */
struct htkamd_inputxform {
   char *name, *mask;          /* macro name (an inline transform: the file it stood in); <MMFIDMASK> */
   char kind[64];              /* parameter kind of the rows it takes */
   int preQual;                /* <PREQUAL>: applied to the statics, before the qualifiers */
   int vecSize, blockSize;     /* <VECSIZE> and the one block's size of <BLOCKINFO>: carried */
   int nBias; float *bias;     /* <OFFSET> <BIAS>: carried, not applied (ApplyStaticMat uses the matrix alone) */
   float det;                  /* <LOGDET>: carried (0 = none) */
   int mrows, mcols; float *mat;   /* <XFORM> r c, row-major */
};

/* ---- packed model ---- */
struct htkamd_model {
   int D, S, C, G, nT, H, maxN, maxM;
   int PS;                     /* floats per Gaussian in gparam: 2*D+1 rounded up to a multiple of 4 */
   /* host copies */
   int   *h_stateCompOff, *h_compGauss, *h_transN, *h_transOff, *h_hmmTrans, *h_hmmStateOff, *h_hmmState, *h_minDur;
   int   *h_trOccOff;          /* [nT+1] prefix sum of transN */
   unsigned char *h_transLR;   /* [nT] the matrix is left-to-right without skips: a_1j only for j = 2, a_ij only for j = i, i+1, a_iN only from N-1
                                  (kept with h_minDur; a change bumps topoVersion) */
   float *h_mean, *h_var, *h_ivar, *h_gconst, *h_compWeight, *h_compLogWt, *h_transP;
   /* device copies */
   float *d_gparam;            /* [G*PS]: (mean[i], ivar[i]) pairs, 8-byte aligned, then gconst at [2*D] */
   double *d_laddTab;          /* [LADD_NK*(LADD_DEG+1)] */
   float *d_mean, *d_ivar, *d_gconst, *d_compLogWt, *d_transP;
   int   *d_stateCompOff, *d_compGauss, *d_transN, *d_transOff;
   /* device-side update (update.hip): linear parameters and topology, uploaded on first use */
   float *d_var, *d_compWeight;
   int   *d_trOccOff, *d_hmmTrans, *d_hmmStateOff, *d_hmmState;
   void  *d_updScratch; size_t updScratchCap;
   void  *evUpd; int updPending;  /* htkamd_model_update_device_begin .. _end: the event behind the update's copy */
   void  *h_updPin;            /* pinned: transition matrices + the 16 counters of a device update, one D2H copy */
   int    topoVersion;         /* bumped whenever a minimum duration (hence tee-ness) of a transition matrix changes: batch tables
                                  prepared before that (htkamd_fb_prepare) no longer describe the model */
   void  *obRing;              /* task-table ring of htkamd_outp_block (gmm_exact.hip) */
   int    hostStale;           /* the host copies of mean/var/gconst/weights are older than the device's (after htkamd_model_update_device) */
   /* MFMA scoring path (gmm_mfma.hip): A-operand fragments [tile][mfmaNS+4][64], 16 components per tile */
   float *d_mfmaTab;           /* NULL when D has no MFMA kernel */
   int   *d_stateTileOff;      /* [S+1] */
   int   *d_tileState;         /* [nTiles] tied state of every fragment tile */
   int    mfmaNS, nTiles;
   void  *d_bf16Tab;           /* bf16 x 3 scoring path (gmm_bf16.hip): A-operand pieces per tile; NULL when D > 45 */
   int    bf16NC;              /* K chunks of 32 per piece: ceil(D/15) */
   int    bf16Dense;           /* the 32 x 32 bf16 kernel's five-k-step layout (31 <= D <= 39, every state in one tile): gmm_bf16.hip, k_score_bf16w<5> */
   void  *d_f16Tab;            /* fp16 x 2 scoring path (gmm_f16.hip): A-operand pieces per tile, K chunks as the bf16 path; NULL when D > 45 */
   int    f16Wide;             /* every state fits one tile (<= 16 components): the 32 x 32 form of the kernel and its table layout */
   float *d_f16Ctl;            /* its control block: scale[96], 1/scale[96], range[192], flag of the last table build, sticky range flag */
   /* freshness of the three derived tables above (model.hip: htkamd_model_params_changed, htkamd_model_table_current).  The rule: after
      a change of the parameters on the device, the tables of the paths that have scored are rebuilt on the update's stream; every
      other table is rebuilt on its next use, on the scoring call's stream */
   int    tabStale;            /* HTKAMD_SCORE_MFMA / _BF16 / _F16 bits: the path's table is older than the parameters */
   int    compat;              /* HTKAMD_COMPAT_* bits (htkamd_model_set_compat) */
   unsigned char *h_rawLogWt, *d_rawLogWt;   /* [C] HTKAMD_COMPAT_SHARED_LOGWT: the component's weight is read as a LOG weight as it stands (ConvLogWt skipped it), or NULL */
   int    fastUse;             /* HTKAMD_SCORE_BF16 / _F16 bits: the paths that have scored with this model (their tables follow every device update) */
   /* shared mean / variance vectors (~u / ~v macros; htkamd_model_set_sharing): first Gaussian of the group a Gaussian's mean / variance
      belongs to (itself when private), members of its variance group; NULL = no sharing in the set */
   int   *h_meanLeader, *h_varLeader, *h_varGroupSize;
   int   *d_shareTab;                 /* meanLeader[G] varLeader[G] varGroupSize[G] muMemOff[G+1] vaMemOff[G+1] muMem[] vaMem[] (update.hip) */
   int    shareMuMem, shareVaMem;     /* lengths of the two member lists */
   /* several streams (htkamd_model_desc::numStreams > 1): S counts (state, stream) ELEMENTS, element = tied state * NSt + stream, and
      h_hmmState lists the NSt elements of every emitting state; a Gaussian is an undivided row whose dimensions outside its stream
      carry mean 0, 1/variance 0 */
   int    NSt;                 /* streams (1: none of the following is allocated) */
   int   *h_dimStream, *h_gaussStream, *d_dimStream, *d_gaussStream;   /* [D] stream of a dimension, [G] stream of a Gaussian */
   /* tied mixtures (htkamd_model_desc::hsKind == HTKAMD_HS_TIED): the pool of stream k is what element k (state 0) lists */
   int    tiedMix, tmPool;     /* tmPool: Gaussians in all pools together */
   float  tmBeam;              /* aligner / decoders: PrecomputeTMix's threshold (HVite -c, default 10.0; htkamd_model_set_tm_beam) */
   int   *h_tmPoolOff, *d_tmPoolOff;   /* [NSt+1] first pool entry of a stream in the per-frame pool table (fb.hip tmE) */
   float *h_streamWt, *d_streamWt;    /* [S] stream weight of every element (1 unless <SWEIGHTS>) */
   int   *d_msCompOff;         /* [S+1] = 2e: what the recursion kernels read as "components of the chain state" (they only ask == 1) */
   int   *h_scanOrder;         /* [H] the reference's HMM scan order of the physical models (htkamd_model_set_scan_order), or NULL */
   /* full covariances (htkamd_model_create_full): the inverse covariance of every Gaussian as its lower triangle packed row-major
      ((i, j), j <= i, at i(i+1)/2 + j), and the exact FULLC scorer's table (gmm_full.hip): per Gaussian mean[D], triangle, gConst, zero
      padding to FPS floats (a multiple of 4).  h_var is a placeholder of ones and d_gparam describes no density; the matrix-core tables,
      forward-backward and the accumulators are not built for such a model */
   int    fullc, FPS;
   float *h_invCov, *d_fparam;
   double minLogExp;
   float *d_mllrMean;          /* htkamd_mllr_apply (mllr.hip): the means as they were, [G*D]; NULL = the set is not adapted */
};

void htkamd_outp_ring_free(void *ring);                      /* gmm_exact.hip */
/* the builders of the derived tables, each the only one of its table (stream: hipStream_t); called through the two functions below */
int htkamd_model_refresh_mfma_device(struct htkamd_model *m, void *stream);   /* update.hip */
int htkamd_model_refresh_bf16_device(struct htkamd_model *m, void *stream);   /* gmm_bf16.hip */
int htkamd_model_refresh_f16_device(struct htkamd_model *m, void *stream);    /* gmm_f16.hip */
/* model.hip.  The parameters on the device changed: every derived table is stale; fromDevice (a device update): those of the paths in
   fastUse are rebuilt on `stream` and the host copies are stale; otherwise (the host pushed them) all are rebuilt and waited for */
__attribute__((visibility("hidden"))) int htkamd_model_params_changed(struct htkamd_model *m, void *stream, int fromDevice);
/* the head of a matrix-core launcher: refuses a vector size the path (one HTKAMD_SCORE_* bit) has no table for, rebuilds its table on
   `stream` if it is stale and notes the path in fastUse */
__attribute__((visibility("hidden"))) int htkamd_model_table_current(const struct htkamd_model *m, int path, void *stream);
int htkamd_model_f16_flag(struct htkamd_model *m, void *stream, int *flag);   /* gmm_f16.hip: the sticky range flag, read and cleared */
/* range flag of the fp16 path (ScoreArgs::rangeFlag) */
#define HTKAMD_F16_EMODEL 1    /* a scaled coefficient of the model exceeds fp16's range */
#define HTKAMD_F16_EFEAT  2    /* a scaled feature value (x or x^2) exceeds fp16's range */
int htkamd_model_device_tables(struct htkamd_model *m);      /* model.hip: uploads d_var etc. once */
static inline size_t htkamd_tri_size(int D) { return (size_t)D * (D + 1) / 2; }
int htkamd_model_sync_host(struct htkamd_model *m);          /* model.hip: device -> host parameter copies when stale */
void htkamd_model_refresh_topology(struct htkamd_model *m);  /* model.hip: minimum durations and left-to-right flags from h_transP; topoVersion moves where one changed */
int htkamd_update_models(struct htkamd_model *m, const htkamd_accs_layout *lay, const double *acc,
                         const htkamd_update_config *cfg, htkamd_update_stats *st);   /* host/update.c */

struct htkamd_accs {
   struct htkamd_model *m;
   htkamd_accs_layout lay;
   double *d_vec;
   int stateOrder;             /* htkamd_accs_state_ranges: 0 not looked at yet, 1 compGauss[c] == c throughout (a state's Gaussians are a range of the vector), -1 not so */
};

#ifdef __cplusplus
}
#endif
#endif
