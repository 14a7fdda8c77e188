/* htk_amd.h -- C ABI of the MI355X-native HTK acoustic-scoring / Baum-Welch / Viterbi core.
 *
 * This is the drop-in boundary for the HERest / HVite hot path of HTK 3.4.1:
 * plain C, plain pointers and sizes, no C++ or torch types.  An HTKLib build binds these entry
 * points from the places cited on each declaration (INTEGRATION.md shows the shim a maintainer
 * adds to HModel.c / HFB.c / HRec.c / HParm.c).  Everything numeric runs in hand-written HIP
 * kernels for gfx950; there is no CPU fallback -- every call fails with HTKAMD_ENODEV when no
 * device is present.
 *
 * Conventions
 *  - "host" pointers are ordinary memory, "device" pointers are HBM addresses (hipMalloc or any
 *    allocator that yields device memory, e.g. a torch CUDA tensor's data_ptr()).
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *  - All functions return 0 on success or a negative HTKAMD_E* code; htkamd_last_error() gives
 *    the message of the most recent failure on the calling thread.
 *  - Indices are 0-based; HMM state numbers inside a model keep HTK's 1..N (1 entry, N exit).
 */
#ifndef HTK_AMD_H
#define HTK_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HTKAMD_OK        0
#define HTKAMD_EINVAL   (-1)   /* bad argument */
#define HTKAMD_ENODEV   (-2)   /* no HIP device / kernel image not loadable */
#define HTKAMD_ENOMEM   (-3)
#define HTKAMD_EHIP     (-4)   /* HIP runtime error, see htkamd_last_error() */
#define HTKAMD_EMODEL   (-5)   /* model violates a restriction of this path (streams>1, non-diagonal cov...) */
#define HTKAMD_EIO      (-6)   /* file cannot be opened / read / written */
#define HTKAMD_ERANGE   (-7)   /* HTKAMD_SCORE_F16 only: a feature value or a model coefficient does not fit the fp16 scoring path's range;
                                  nothing of the pass can be used -- repeat it with HTKAMD_SCORE_BF16 (same tolerance class, fp32's exponent) */

/* HTK's log-arithmetic constants (HMath.h:42-45, HModel.h:52-53, HFB.h:31) */
#define HTKAMD_LZERO    (-1.0E10)
#define HTKAMD_LSMALL   (-0.5E10)
#define HTKAMD_NOPRUNE  1.0E20

/* UPDSet bits used by HERest (HModel.h UPDSet; HERest.c:97 default "tmvw") */
#define HTKAMD_UPMEANS  1
#define HTKAMD_UPVARS   2
#define HTKAMD_UPTRANS  4
#define HTKAMD_UPMIXES  8
#define HTKAMD_UPMAP    32   /* HERest -u p: MAP instead of ML re-estimation of means / variances / weights (HMap.c:413 MAPUpdateModels) */

int         htkamd_version(void);
const char *htkamd_last_error(void);
int         htkamd_device_count(void);
int         htkamd_set_device(int ordinal);

/* Device-memory plumbing for hosts that do not bring their own allocator (the C drivers, the tests). */
int htkamd_dev_malloc(void **dptr, size_t bytes);
int htkamd_dev_free(void *dptr);
int htkamd_memcpy_h2d(void *dDst, const void *hSrc, size_t bytes, void *stream);   /* synchronous on return */
/* page-locked host memory and a copy from it that does not wait: ordered before the work queued behind it on `stream`; refill the buffer only
   after that work has been waited for (the HFB shim stages an utterance's observations this way: shim/htklib_hfb_shim.c, FBFile HFB.c:1923) */
int htkamd_host_malloc(void **hptr, size_t bytes);
int htkamd_host_free(void *hptr);
int htkamd_memcpy_h2d_async(void *dDst, const void *hSrc, size_t bytes, void *stream);
int htkamd_memcpy_d2h(void *hDst, const void *dSrc, size_t bytes, void *stream);   /* synchronous on return */
int htkamd_stream_sync(void *stream);
/* streams for hosts without HIP headers (C drivers of the exchange in parts): a stream of one's own, and "the work queued on `waiter` from
   here on starts behind what has been queued on `signaller` so far" (an event recorded on the one, waited for by the other; NULL = the default stream) */
int htkamd_stream_create(void **stream);
int htkamd_stream_destroy(void *stream);
int htkamd_stream_wait(void *waiter, void *signaller);

/* ------------------------------------------------------------------------------------------
 * Packed HMM set.  Flat restatement of HMMSet / HMMDef / StateInfo / StreamElem / MixPDF
 * (HModel.h:85-152,297-340) for one stream, diagonal covariances, PLAINHS/SHAREDHS:
 *   tied states   <-> StateInfo with sIdx 1..S   (SetIndexes, HModel.c:3942)
 *   components    <-> MixtureElem {weight, mpdf}
 *   Gaussians     <-> MixPDF with mIdx 1..G      (several components may share one: ~m macros)
 *   transP        <-> SMatrix with tIdx, LOG probabilities, LZERO for "no transition"
 * Parameters are given as they stand after LoadHMMSet (DIAGC variances, linear weights);
 * the library applies FixDiagGConst (HModel.c:5641) when gconst==NULL, ConvDiagC (HUtil.c:413)
 * and ConvLogWt (HUtil.c:474) itself, exactly once, as HERest.c:592-645 / HVite.c:503 do.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
   int vecSize;               /* D  (hset->vecSize)                                  */
   int numStates;             /* S  tied states                                       */
   int numComp;               /* C  = sum over states of nMix                         */
   int numGauss;              /* G  distinct MixPDFs                                  */
   int numTrans;              /* nT distinct transition matrices                      */
   int numPhys;               /* H  physical HMMs                                     */
   const int   *stateCompOff; /* [S+1] components of state s: stateCompOff[s]..[s+1)  */
   const float *compWeight;   /* [C] linear mixture weights (MixtureElem.weight)      */
   const int   *compGauss;    /* [C] Gaussian index of each component                 */
   const float *mean;         /* [G*D] MixPDF.mean                                    */
   const float *var;          /* [G*D] MixPDF.cov.var, DIAGC (variances)              */
   const float *gconst;       /* [G] MixPDF.gConst or NULL to have it computed        */
   const int   *transN;       /* [nT] numStates N of each matrix (entry+exit included)*/
   const int   *transOff;     /* [nT+1] offset of matrix t inside transP              */
   const float *transP;       /* row-major N*N log probs per matrix                   */
   const int   *hmmTrans;     /* [H] tIdx of each physical HMM                        */
   const int   *hmmStateOff;  /* [H+1]                                                */
   const int   *hmmState;     /* tied-state index of the emitting states 2..N-1       */
   /* Several streams (hset->swidth[0] > 1; HModel.h StreamElem, HParm.c:3094 SetStreamWidths).  numStreams 0 or 1: one stream, the
      fields above as described.  numStreams = NS > 1: stateCompOff has numStates*NS + 1 entries, the components of stream k of state
      s are stateCompOff[s*NS + k] .. [s*NS + k + 1); a Gaussian belongs to one stream and is held in an UNDIVIDED row of vecSize
      elements: its values at the dimensions d with dimStream[d] == its stream, mean 0 and variance +infinity elsewhere (such a
      dimension contributes nothing to a score and is never re-estimated); the feature rows stay undivided as well.
      WHERE THIS LIBRARY DELIBERATELY DIFFERS FROM THE REFERENCE'S HERest (both differences are defects of the reference; the oracle
      restates them bit for bit, oracle/htk_oracle.c, and DESIGN.md §4b / §4c measures them):
        * NS != 3: when a tied state is met a second time in one frame (by another chain state), Setotprob sums the cached stream
          vectors it has already overwritten with "the sum of the others" and halves the result (HFB.c:1044-1064) -- the first visit's
          value for NS = 3 only; for NS = 2 every repeated state gets HALF its log probability (the reference reports -33.6 per frame
          on the demo set split 13 | 13 where the sum of the streams' log probabilities gives -59.1).  This library computes the
          first visit's value at every visit: equal to HERest for NS = 1 and NS = 3, NOT for NS = 2 or NS >= 4 on sets with repeated
          tied states -- unless htkamd_model_set_compat(HTKAMD_COMPAT_STREAM_REVISIT) asks for the reference's value.
        * SHAREDHS sets whose mixtures share pdfs (~m macros without HHEd's TIEDHS conversion): ConvLogWt converts the weights of the
          FIRST state that uses a shared pdf only (HUtil.c:474-485), the others are read as log weights; this library converts
          every weight once -- unless htkamd_model_set_compat(HTKAMD_COMPAT_SHARED_LOGWT) asks for the reference's reading. */
   int numStreams;
   const int   *dimStream;    /* [D] stream (0-based) of each dimension, NULL for one stream (htkamd_mmf computes it from the kind) */
   /* HTKAMD_HS_TIED: a tied-mixture set (hsKind TIEDHS, <TMIX>): every (state, stream) lists the SAME pool of Gaussians of its stream
      (compGauss equal across states) with its own weights; output probabilities and statistics go through the pool's top-M arithmetic
      (PrecomputeTMix HModel.c:5308, SOutP :5555, UpMixParms HFB.c:1524-1600), the pool is re-estimated once per set (HERest.c:1272). */
   int hsKind;
   const float *streamWeight; /* [numStates*NS] <SWEIGHTS> of every state, NULL = all 1 (GetStateInfo HModel.c:1994).  Used by the aligner and
                                 the decoder (OutP = sum_s w_s SOutP_s, HModel.c:5570-5583 / HRec.c:510-548); HFB ignores them (HFB.c:1057) */
} htkamd_model_desc;
#define HTKAMD_HS_PLAIN 0
#define HTKAMD_HS_TIED  1
/* dimStream for a parameter kind given as text ("MFCC_E_D") and the stream widths of <STREAMINFO>: the split SetStreamWidths /
   ExtractObservation make (HParm.c:3094,2843 -- the standard splits take the energy terms out into the last stream, any other split is
   consecutive pieces).  Returns 0, or -1 with the reason in `why`. */
int htkamd_host_stream_dims(const char *kind, int vecSize, int S, const int *width, int *dimStream /*[vecSize]*/, char *why, size_t whyLen);

typedef struct htkamd_model htkamd_model;

int  htkamd_model_create(const htkamd_model_desc *desc, htkamd_model **out);
/* Full-covariance sets (<FULLC>, MixPDF ckind FULLC with cov.inv, HModel.h; scored by FOutP HModel.c:5361-5381).  invCov: the inverse
   covariance of every Gaussian as its lower triangle packed row-major, element (i, j), j <= i, at g*D(D+1)/2 + i(i+1)/2 + j (what
   htkamd_mmf_inv_cov gives).  desc->var is ignored; desc->gconst NULL = FixFullGConst(mp, -CovDet(inv)) (CheckMix HModel.c:210, the
   reference's Choleski in double, HMath.c:514,593).  One stream, continuous densities only.  Such a model is scored by the exact kernel
   (HTKAMD_SCORE_EXACT, with or without HTKAMD_SCORE_SOUTP) wherever the library scores -- htkamd_outp_block[_mode], the aligner, the
   decoders --; the matrix-core score modes return HTKAMD_EMODEL, and so do htkamd_fb_create and htkamd_accs_create: re-estimation of
   FULLC sets is not supported yet. */
int  htkamd_model_create_full(const htkamd_model_desc *desc, const float *invCov, htkamd_model **out);
/* mp->cov.inv of every Gaussian, packed as above.  set: gconst NULL = FixFullGConst(mp, -CovDet(inv)) as FixGConsts (HModel.c:5688);
   HTKAMD_EMODEL on a DIAGC model or an inverse that is not positive definite (the reference's HError 5220). */
int  htkamd_model_set_inv_cov(htkamd_model *m, const float *invCov, const float *gconst);
int  htkamd_model_get_inv_cov(htkamd_model *m, float *invCov /*[G*D(D+1)/2]*/);
int  htkamd_model_is_full(const htkamd_model *m);              /* 1 for a model made by htkamd_model_create_full */
/* Tied mean / variance vectors (~u / ~v macros: SVector with nUse > 1, HModel.c:1737-1790).  meanShare[g] / varShare[g] >= 0 name the
 * vector Gaussian g's mean / variance is a copy of (-1 = private; either array may be NULL); htkamd_mmf_sharing gives them for a set
 * read from files.  Scoring and the statistics are per Gaussian as always; htkamd_model_update pools the statistics of the sharers
 * as the reference's hooks on the shared vector do (one MuAcc / VaAcc per vector; a tied variance gets no mean-shift correction,
 * HERest.c:1080) and keeps the copies equal; htkamd_model_update_device does the same where the accumulators lie (the "first mixture
 * to reach the vector" of the reference's scan as a minimum over scan positions). */
int  htkamd_model_set_sharing(htkamd_model *m, const int *meanShare /*[G]*/, const int *varShare /*[G]*/);
/* The order in which UpdateModels (HERest.c:1262-1321) visits the physical models: the reference's HMM scan, i.e. htkamd_hmm_scan_order of
   their names.  It matters only for sets with mean vectors shared across models (which Gaussian's variance takes the mean-shift term);
   NULL (the default) = definition order. */
int  htkamd_model_set_scan_order(htkamd_model *m, const int *order /*[numPhys]*/);
int  htkamd_model_has_sharing(const htkamd_model *m);
/* Tied-mixture sets in the aligner and the decoders: the pruning threshold of the pool (HVite -c f, tmBeam HVite.c:115: pool entries more
   than f below the frame's best are left out of every state's sum; default 10.0).  Forward-backward uses its own (minFrwdP, HFB.c:1011). */
int  htkamd_model_set_tm_beam(htkamd_model *m, float tmBeam);
/* The reference's own arithmetic where this library deliberately computes something else (htkamd_model_desc, "WHERE THIS LIBRARY
   DELIBERATELY DIFFERS").  HTKAMD_COMPAT_STREAM_REVISIT: forward-backward on PLAINHS / SHAREDHS sets with NS != 3 streams gives a chain
   state whose tied state was met before in the same Setotprob call -- by a model further right in the beam, or an earlier state of the
   same model -- the value HFB.c:1059 gives it: the float sum of the streams' "sum of the others", halved, i.e. (NS - 1) / 2 times the
   state's log probability.  The recursions, occupation and transition counts see that value, the mixture statistics the first visit's
   "sum of the others", as in the reference (HFB.c:1062-1064,1611).  Batches then run on the general workgroup-per-utterance kernels
   (call before htkamd_fb_prepare).  No effect on sets with one or three streams or on tied-mixture sets (the reference's defect is not
   reached there).
   HTKAMD_COMPAT_SHARED_LOGWT: PLAINHS / SHAREDHS sets whose mixtures share pdfs (~m macros): ConvLogWt passes over a component whose pdf
   it has met before (GoNextMix, HUtil.c:371-394,474-485), so only the first state's weight of a shared pdf becomes a logarithm and the
   others are read as log weights as they stand.  "First" is in HMM scan order (htkamd_model_set_scan_order; either call order works).
   The scoring tables (and every refresh of them after an update) then hold the linear weight where the reference reads it as a log. */
#define HTKAMD_COMPAT_STREAM_REVISIT 1
#define HTKAMD_COMPAT_SHARED_LOGWT   2
int  htkamd_model_set_compat(htkamd_model *m, int flags);
void htkamd_model_destroy(htkamd_model *m);
/* Replace the parameters after a re-estimation pass (same topology). Any pointer may be NULL = unchanged. */
int  htkamd_model_set_params(htkamd_model *m, const float *mean, const float *var, const float *gconst,
                             const float *compWeight, const float *transP);
/* Prepared tables as an HTKLib front-end holds them after ConvDiagC (HUtil.c:413), FixGConsts (HModel.c:5688) and ConvLogWt (HUtil.c:474):
   1/variance [G*D], gConst [G], log mixture weights [C] (LZERO below MINMIX).  The kernels then read exactly these floats (the
   HTKLib shim, shim/htklib_hfb_shim.c, hands over the values of the HMMSet it was given).  Any pointer may be NULL = unchanged. */
int  htkamd_model_set_prepared(htkamd_model *m, const float *ivar, const float *gconst, const float *compLogWt);
/* Read back the prepared device-side values (test/debug aid): each may be NULL. */
int  htkamd_model_get_prepared(htkamd_model *m, float *ivar /*[G*D]*/, float *gconst /*[G]*/,
                               float *compLogWt /*[C]*/, int *minDur /*[nT]*/);

/* ------------------------------------------------------------------------------------------
 * Model definition files: replaces LoadHMMSet (HModel.c:3809) = MakeHMMSet (:3580) + LoadMacroFiles (:3721) with the
 * -d directory search, and SaveHMMSet (:4979) / SaveInOneFile (:4858), for text definitions of one-stream DIAGC or FULLC
 * continuous-density sets, text or binary (macros ~o ~s ~t ~m ~h ~v"varFloor"; ~u/~v sharing inside a pdf, streams and durations as
 * described with their accessors; <INPUTXFORM> and ~j input transforms: see "Global linear input transforms" below; <PARENTXFORM> and
 * the other transform macros are rejected with HTKAMD_EMODEL).  Pure host code.
 *   mmf_read    : one master macro file, or one HMM file (a definition without ~h takes `defName` / the file's base name)
 *   mmf_finish  : HMM list "logical [physical]" (NULL: every defined model is its own logical name); physical models still
 *                 undefined are read from dir/name[.ext]; builds the flat description for htkamd_model_create.
 *                 Transition values are logs (GetTransMat, HModel.c:1965), variances as in the file.
 *   mmf_write   : text output of the given parameter arrays (layout of the description; transP logs), into one file
 *                 (macros in the reference's hash-table order) or one file per physical HMM under dir (SAVEGLOBOPTS form).
 * ------------------------------------------------------------------------------------------ */
typedef struct htkamd_mmf htkamd_mmf;
int  htkamd_mmf_create(htkamd_mmf **out);
/* Mixture splitting as HHEd's MU command does it (MixUpCommand HHEd.c:4020, UpMix :2149, SplitMix :1318, HeaviestMix :2112): every
   state with stateSel[state] != 0 (NULL = all) goes to `target` components, or gains -target if target < 0; afterwards
   htkamd_mmf_desc / htkamd_mmf_write reflect the new set.  The step between single-Gaussian and mixture systems in a recipe. */
int  htkamd_mmf_mixup(htkamd_mmf *s, int target, const unsigned char *stateSel);
/* Decision-tree state clustering as HHEd's RO / QS / TB / ST commands do it (BuildTree HHEd.c:2961) for state items of one-stream,
   single-Gaussian DIAGC sets: the step between cloned single-Gaussian triphones plus an HERest -s statistics file and a tied-state set.
     stats_read_file  : LoadStatsFile (HUtil.c:1291): occ[state] = the occupation of every state a model of the file owns (a float, as
                        the reference keeps it), count[phys] = the model's number of examples (may be NULL); states of models the file
                        does not list keep 0.  A name that is not in the set or a wrong number of counts is refused.
     mmf_tree_cluster : `outlierThresh` is RO's (< 0: none), `q` the QS commands in order (a name and model-name patterns with * and ?;
                        a question no model answers is dropped, htkamd_last_error then holds a warning), `t` the TB commands in order
                        (threshold, macro name, item list "{ pat.state[i] }" / "{ (pat,pat).state[i] }" with a single state index;
                        trees must not overlap).  All trees are built together on the device (the sums of every node over every
                        question, in the reference's order and bit for bit) with the deciding likelihoods evaluated on the host; then
                        the leaves are tied in order: ~s macros `macRoot` + number.  With HTKAMD_TREE_LEAFSTATS the tied state's mean
                        and variance come from the leaf's statistics, floored by varFloor1; every gConst is then refreshed, as HHEd does
                        before it saves (FixAllGConsts, HHEd.c:6469).  Afterwards htkamd_mmf_desc / htkamd_mmf_write reflect the tied set
                        (fewer states; state numbers change).  `treesPath`: the ST command's file, or NULL.
     trees_write      : ShowTreesCommand (HHEd.c:3263) for trees given as tables: node n asks question quest[n]; no[n] / yes[n] >= 0 is
                        a node, < 0 the leaf -1-k whose macro is leafMacro[k]; nNodes = 0: the single leaf leafMacro[0].
     mmf_item_list / mmf_question_answers / tree_split_sums : test aids -- an item list's (model, state number) pairs in the order of the
                        reference's list; a question's answer per physical model; the raw sums of one node on the device. */
typedef struct { const char *name; const char *const *patterns; int nPatterns; } htkamd_tree_question;
typedef struct { float threshold; const char *macRoot; const char *itemList; } htkamd_tree_spec;
typedef struct { const char *name; int state; int nNodes; const int *quest, *no, *yes; const char *const *leafMacro; int nLeaves; } htkamd_tree_desc;
#define HTKAMD_TREE_MERGE      1   /* TREEMERGE (default T in the reference)    */
#define HTKAMD_TREE_LEAFSTATS  2   /* USELEAFSTATS (default T in the reference) */
int  htkamd_stats_read_file(const htkamd_mmf *s, const char *path, float *occ /*[numStates]*/, int *count /*[numPhys]*/);
int  htkamd_mmf_tree_cluster(htkamd_mmf *s, const float *occ /*[numStates]*/, float outlierThresh, const htkamd_tree_question *q, int nQ,
                             const htkamd_tree_spec *t, int nT, int flags, const char *treesPath, void *stream);
int  htkamd_trees_write(const char *path, const htkamd_tree_question *q, int nQ, const htkamd_tree_desc *t, int nT);
int  htkamd_mmf_item_list(const htkamd_mmf *s, const char *itemList, int *phys /*[cap]*/, int *state /*[cap]*/, int cap, int *n);
int  htkamd_mmf_question_answers(const htkamd_mmf *s, const htkamd_tree_question *q, unsigned char *answers /*[numPhys]*/);
/* the raw split sums of one node, [nQ][2][2D+1] floats (no side, then yes side; occ, sum[D], sqr[D]) */
int  htkamd_tree_split_sums(const float *itemStats /*[nItems][2D+1]*/, int nItems, int D, const int *nodeItems, int n,
                            const unsigned char *answers /*[nQ][nItems]*/, int nQ, float *out, void *stream);
/* Data-driven state clustering as HHEd's TC / NC commands do it (Clustering HHEd.c:2005: furthest-neighbour agglomeration of the listed
   states, then one ~s macro per cluster), and the TI command.  One-stream DIAGC sets; the distances (Divergence :1749 for a set whose
   largest mixture has one component, else GDistance :1771 over the library's exact scores) and the merge loops run on the device,
   bit for bit the reference's; all commands of a call run together, one workgroup each.
     data_cluster     : `occ` NULL = no statistics loaded (no outlier phase), else the occupations of htkamd_stats_read_file and RO's
                        threshold: groups below it are merged into their nearest group (RemOutliers :1975).  A command is
                        NC (byCount 1, value = number of clusters) or TC (byCount 0, value = threshold on the group distance);
                        cluster k of a command becomes the macro "<macro>k", k from 1, tied to its typical state (TypicalState :990).
                        numClusters[c]: what command c ended with.  A command whose list is empty is skipped (numClusters 0) and
                        htkamd_last_error then holds a warning (the reference's -2631).  States nobody refers to any more are dropped;
                        htkamd_mmf_desc / htkamd_mmf_write reflect the tied set afterwards (state numbers change).
                        Refused before a device is touched (HTKAMD_EINVAL / HTKAMD_EMODEL and the reason): items that are not
                        .state[i]; a state that is a ~s macro already; an item selected by two commands of the call; sets with more
                        than one stream, FULLC, tied-mixture and discrete sets; more than 3000 items in one command; and a macro name
                        over 20 characters -- the reference only warns there (-2639), this library refuses.
     tie              : TI for a list of .state[i] items (TieState :1021) or of .transP items (TieTrans :1049: the first item's matrix);
                        host only.  Every other item type is refused by name, and so are a state or a matrix that is a macro already
                        and a macro name over 20 characters.
   Diagnostic entry points (test aids, as htkamd_tree_split_sums is one):
     state_distances  : the item-distance matrix [n][n] of an item list, in the list's order (dist NULL: only *n is set).
     cluster_merges   : the merge loop alone on a caller's symmetric matrix idist[N][N]: merges[2m], merges[2m+1] = the groups (i, j)
                        of merge m, 1-based in the numbering current at that merge (room for N - 1 pairs); occ NULL = no outlier phase. */
typedef struct { int byCount; float value; const char *macro; const char *items; } htkamd_cluster_spec;
int  htkamd_mmf_data_cluster(htkamd_mmf *s, const float *occ /*[numStates] or NULL*/, float outlierThresh, const htkamd_cluster_spec *specs, int nSpecs,
                             int *numClusters /*[nSpecs]*/, void *stream);
int  htkamd_mmf_tie(htkamd_mmf *s, const char *macro, const char *items);
int  htkamd_state_distances(htkamd_mmf *s, const char *items, float *dist /*[n][n] or NULL*/, int cap, int *n, void *stream);
int  htkamd_cluster_merges(const float *idist, int N, const float *occ /*[N] or NULL*/, int numReq, float threshold, float outlierThresh,
                           int *merges /*[2(N-1)]*/, int *nMerges);
/* Regression class trees as HHEd's RC command builds them (RegClassesCommand HHEd.c:6177): the two files every adaptation path of HTK
   starts from, `<identifier>.tree` and `<identifier>.base`.  One-stream DIAGC sets with any number of mixture components.
     mmf_regtree      : `occ` the state occupations of htkamd_stats_read_file (RC needs a loaded statistics file), `nTerminals` RC's number
                        (0 .. 256), `itemList` RC's optional list of non-speech states "{ pat.state[i-j].mix }" (the only item form of
                        type 'p' that a one-stream set has; NULL or "" = none): their Gaussians become node 2, the others node 3 under the
                        root.  The Gaussians are taken in the order of InitRegTree's scan (:5734: models in the macro table's order, the
                        unseen states of a model, their unseen mixture components), each with the AccSum record that InitTreeAccs (:2535)
                        gives it -- none where the state has no occupation.  Every split (ClusterChildren :5961: the distances, the
                        centroid sums in list order, the convergence loop, the stable partition, the children's distributions and scores)
                        is one workgroup's work on the device (csrc/regtree.hip), bit for bit the reference's floats; which terminal to
                        split next, the perturbed seeds and the node numbers are BuildRegClusters' (:6096) on the host.  The set itself is
                        not changed.  Refused before a device is touched (HTKAMD_EINVAL / HTKAMD_EMODEL and the reason): sets with more than
                        one stream, FULLC, tied-mixture and discrete sets; a vector size above 960; an item list that is not of that form.
     regtree_from_tables : a tree from tables, for the writers alone: node i (1-based) has children left[i-1], right[i-1] (0, 0: a terminal);
                        the terminals' components stand behind one another in node order, compOff[i-1] .. compOff[i] (nNodes + 1 offsets).
     regtree_write    : PrintRegTree (:6010) into dir/<identifier>.tree and the base classes beside it (:6040) into dir/<identifier>.base
                        (dir NULL: the working directory; <MMFIDMASK> is the reference's default "*").  `identifier` is a plain name.
     accessors        : nodes are numbered from 1 as in the files; a terminal has children 0, 0; base class k (from 1) is terminal_node(k);
                        component i of a terminal node is (physical model name, state, mixture).  regtree_stats: the CalcDistance calls
                        of every split in the order the splits were made (at most `cap` are written; the return value is their number),
                        and the device time of the call's kernels in ms.
   Diagnostic entry point (a test aid, as htkamd_tree_split_sums is one):
     regtree_probe    : the device steps of mmf_regtree alone over a caller's members: mean / sum / sqr rows, occupations and the flag
                        "has an AccSum record" per member, the member list starting as 0 .. G-1.  steps[s] = (kind, off, n) run in order
                        on one device state, so a later step sees the list as the earlier splits left it: kind 0 is
                        CalcClusterDistribution and CalcNodeScore of the range (figures[s][0]: aveMean[D], aveCovar[D], clustAcc,
                        clusterScore), kind 1 a ClusterChildren of it from seeds[s][2][D] (counts[s]: members left, right, CalcDistance
                        calls; figures[s][0 .. 1]: the two children).  list[G]: the members as the last step left them.  Refused: a
                        range outside the members, a split of no member, D above 960, any other kind. */
typedef struct htkamd_regtree htkamd_regtree;
int  htkamd_mmf_regtree(htkamd_mmf *s, const float *occ /*[numStates]*/, int nTerminals, const char *itemList /*may be NULL*/, htkamd_regtree **out, void *stream);
int  htkamd_regtree_from_tables(int nNodes, const int *left, const int *right, const int *compOff /*[nNodes+1]*/, const char *const *compModel, const int *compState,
                                const int *compMix, htkamd_regtree **out);
int  htkamd_regtree_num_nodes(const htkamd_regtree *t);
int  htkamd_regtree_children(const htkamd_regtree *t, int node, int *left, int *right);
int  htkamd_regtree_num_terminals(const htkamd_regtree *t);
int  htkamd_regtree_terminal_node(const htkamd_regtree *t, int baseClass);
int  htkamd_regtree_num_components(const htkamd_regtree *t, int node);
const char *htkamd_regtree_component(const htkamd_regtree *t, int node, int i, int *state, int *mix);      /* the physical model's name */
int  htkamd_regtree_stats(const htkamd_regtree *t, int *iters /*[cap] or NULL*/, int cap, float *kernelMs /*or NULL*/);
int  htkamd_regtree_write(const htkamd_regtree *t, const char *identifier, const char *dir /*may be NULL*/);
void htkamd_regtree_destroy(htkamd_regtree *t);
int  htkamd_regtree_probe(const float *mean /*[G][D]*/, const float *sum /*[G][D]*/, const float *sqr /*[G][D]*/, const float *occ /*[G]*/,
                          const unsigned char *hasAcc /*[G]*/, int G, int D, const int *steps /*[nSteps][3]*/, const float *seeds /*[nSteps][2][D]*/,
                          int nSteps, int *counts /*[nSteps][3]*/, float *figures /*[nSteps][2][2D+2]*/, int *list /*[G]*/, void *stream);
/* Unseen triphones from the trees and the compacted set: HHEd's LT / AU / CO commands (and ST for trees that were loaded).
   htkamd_mmf_tree_cluster leaves its trees on the holder, as HHEd's treeList and question list outlive TB: the kept questions with their
   patterns and per tree the base phone, the state number, the node table and the leaves' ~s macros.  Trees of further calls are added.
     load_trees  : LoadTreesCommand (HHEd.c:3433) with LoadQuestion :417 and LoadTree :3346: the QS lines, then state trees "base[i]" as a
                   node table "{ -n 'question' no yes ... }" or as a single leaf.  The patterns of a question are prepended as they are
                   read, so a file that is loaded and saved again shows every question's patterns in the opposite order -- as with HHEd;
                   a second round gives the first file back.  Refused with the reason: a question named twice or already held
                   (HTKAMD_EINVAL, the reference's 2661 "Question name invalid"); a node's question or a leaf's macro that is not recognised
                   (HTKAMD_EMODEL, 2661; a leaf must be a ~s macro of the set); a node number that is not in the tree, named by two parents
                   or never defined (HTKAMD_EINVAL, 2661); a file without questions when none are held (HTKAMD_EINVAL, 2660
                   "Questions Expected") or without trees; model trees -- a name without [i], the reference's 'h' trees -- which are
                   not built (HTKAMD_EMODEL); text that cannot be parsed (HTKAMD_EIO).  A refused file leaves the held trees as they were.
     save_trees  : ShowTreesCommand (HHEd.c:3263) for the held trees, through htkamd_trees_write.
     add_unseen  : AddUnseenCommand (HHEd.c:5082) with TreeFilter :3219, SynthModel :3180, AssignStructure :3115, FindProtoModel :3160 and
                   SwapLists :3497.  `hmmListPath` lists one model name per line.  A name the set knows as a logical model keeps its model;
                   every other name becomes a new physical model: the number of states, the duration and the transition matrix of its
                   proto -- the first model in the reference's macro-table scan (htkamd_hmm_scan_order; models synthesised earlier in the
                   call take part, as they do there) whose name without contexts (TriStrip) is the new name's -- the matrix shared when it
                   is a ~t macro and copied otherwise, and as state i the leaf that the walk down tree "base[i]" ends in.  The wildcard
                   matching of all new names against the questions the trees ask and the walks run on the device (csrc/treesynth.hip);
                   HTKAMD_ENODEV without one.  Afterwards the set's models, physical and logical, are exactly the list's, in list order
                   (SwapLists): htkamd_mmf_desc, _num_logical, _logical_name, _find_logical, _phys_name and htkamd_mmf_write reflect it
                   (model and state numbers change; states nobody uses any more are dropped; every gConst is refreshed as before HHEd
                   saves).  Refused as the reference fails: no trees held (2662); a new name without a proto (2662 "no proto for ..");
                   a new name whose base has no tree for an emitting state (2662 "cannot find tree for .. state i") -- the first such
                   name in the reference's order of work; and with the reason: a list line with a physical name of its own, a name
                   twice in the list, names of more than HTKAMD_SYNTH_MAXNAME characters (TriStrip's buffer), sets with more than one
                   stream, tied-mixture and discrete sets (HTKAMD_EMODEL).  Any number of mixture components per state.
     compact     : CompactCommand (HHEd.c:4340) with EquivHMM :685 and SaveHMMList (HModel.c:5029).  Two models are one when they have the
                   same number of states, the SAME transition matrix (identity, not value) and state for state the same state -- or,
                   when the set has ~m macros or both ~u and ~v macros (varFloor macros count, as there), states whose components name the
                   same mean and variance vectors with the same weights (EquivState :670).  The first of a group in the macro-table scan
                   stays, the others become logical names of it.  One pass with a hash over (matrix, states ..) in place of the
                   reference's list walk; host only.  `listPath`: the list file "logical [physical]" in the scan's order, or NULL.
     name_question_answers / tree_descend / mmf_num_trees / mmf_tree_info / mmf_tree_leaf / mmf_state_macro : test aids -- answers[q][n]
                   of any names against any questions on the device; for names against the HELD trees, per name and state number
                   firstState .. firstState+nStates-1 the tree (-1: none for that base and state) and the leaf the walk ends in (-1 with
                   no tree); the held trees' names, sizes and leaf macros; the ~s macro name of a state of the set (NULL: un-named). */
#define HTKAMD_SYNTH_MAXNAME 99
int  htkamd_mmf_load_trees(htkamd_mmf *s, const char *path);
int  htkamd_mmf_save_trees(const htkamd_mmf *s, const char *path);
int  htkamd_mmf_add_unseen(htkamd_mmf *s, const char *hmmListPath, int *nSeen, int *nUnseen, void *stream);
int  htkamd_mmf_compact(htkamd_mmf *s, const char *listPath, int *nLog, int *nPhys);
int  htkamd_name_question_answers(const char *const *names, int N, const htkamd_tree_question *q, int nQ, unsigned char *answers /*[nQ][N]*/, void *stream);
int  htkamd_tree_descend(const htkamd_mmf *s, const char *const *names, int N, int firstState, int nStates, int *tree /*[N][nStates]*/,
                         int *leaf /*[N][nStates]*/, void *stream);
int  htkamd_mmf_num_trees(const htkamd_mmf *s);
const char *htkamd_mmf_tree_info(const htkamd_mmf *s, int t, int *state, int *nNodes, int *nLeaves);      /* the base phone's name */
const char *htkamd_mmf_tree_leaf(const htkamd_mmf *s, int t, int leaf);
const char *htkamd_mmf_state_macro(const htkamd_mmf *s, int state);
void htkamd_synth_last_kernel_ms(float *ms /*[2]*/);      /* the device time of the last call's matching and walking kernels (tools/synth_bench.py) */
/* HCompV's PutVFloor (HCompV.c:359-389): "~v varFloor1 <Variance> D" with scale*var, written like WriteVector(" %e"). */
int  htkamd_mmf_write_vfloors(const char *path, const float *var, int D, float scale);
void htkamd_mmf_destroy(htkamd_mmf *s);
int  htkamd_mmf_read(htkamd_mmf *s, const char *path, const char *defName);
int  htkamd_mmf_finish(htkamd_mmf *s, const char *hmmList, const char *dir, const char *ext);
const htkamd_model_desc *htkamd_mmf_desc(const htkamd_mmf *s);
int  htkamd_mmf_num_logical(const htkamd_mmf *s);
const char *htkamd_mmf_logical_name(const htkamd_mmf *s, int i);
int  htkamd_mmf_logical_phys(const htkamd_mmf *s, int i);
int  htkamd_mmf_find_logical(const htkamd_mmf *s, const char *name);     /* physical index or -1 */
const char *htkamd_mmf_phys_name(const htkamd_mmf *s, int h);
const char *htkamd_mmf_parm_kind(const htkamd_mmf *s);                   /* e.g. "MFCC_E_D" */
const float *htkamd_mmf_var_floor(const htkamd_mmf *s);                  /* ~v "varFloor1" [vecSize] or NULL */
/* A <FULLC> set (GetCovar HModel.c:1511: <INVCOVAR> D + the lower triangle in ReadTriMat's order, HMath.c:406): the inverse covariances,
   [numGauss * D(D+1)/2] packed as htkamd_model_create_full takes them; NULL for a DIAGC set.  The description of such a set has var = NULL,
   so that htkamd_model_create refuses it (only htkamd_model_create_full makes a model of a FULLC set), and its gconst is always given (the file's <GCONST>, else FixFullGConst(mp, -CovDet(inv))).  Refused with
   HTKAMD_EMODEL: ~i macros, ~u / ~v sharing inside a FULLC set (the ~v varFloor macros excepted), <VARIANCE> and <INVCOVAR> mixtures in
   one set, FULLC with <STREAMINFO> S > 1 or with <TMIX>; LLTC, XFORMC and INVDIAGC as before. */
const float *htkamd_mmf_inv_cov(const htkamd_mmf *s);
int  htkamd_mmf_sharing(const htkamd_mmf *s, int *meanShare /*[numGauss]*/, int *varShare /*[numGauss]*/);   /* ~u / ~v macros; returns the number of Gaussians sharing a vector */
int  htkamd_mmf_write(const htkamd_mmf *s, const float *mean, const float *var, const float *gconst, const float *compWeight,
                      const float *transP, const char *oneFile, const char *dir);
/* the same in HTK's binary form (SaveHMMSet with binary = TRUE, HERest/HHEd -B); htkamd_mmf_read takes either form */
int  htkamd_mmf_write_binary(const htkamd_mmf *s, const float *mean, const float *var, const float *gconst, const float *compWeight,
                             const float *transP, const char *oneFile, const char *dir);
/* SaveHMMSet for a set loaded from several master files (HERest -H macros -H hmmdefs): every macro goes back to the file it was loaded
   from (HModel.c:4388-4470).  masterOut[k] = path for the k-th file read (order of the htkamd_mmf_read calls); models read from files of
   their own beyond those go to dir/<name>. */
int  htkamd_mmf_write_sources(const htkamd_mmf *s, const float *mean, const float *var, const float *gconst, const float *compWeight,
                              const float *transP, const char *const *masterOut, int nMaster, const char *dir, int binary);
/* FULLC sets: htkamd_mmf_write / _write_binary (binary != 0) and htkamd_mmf_write_sources with the packed inverse covariances in place of
   the variances, written by PutCovar(.., INVCOVAR) (HModel.c:2780, WriteTriMat HMath.c:431).  The DIAGC writers refuse a FULLC set and
   these refuse a DIAGC one. */
int  htkamd_mmf_write_full(const htkamd_mmf *s, const float *mean, const float *invCov, const float *gconst, const float *compWeight,
                           const float *transP, const char *oneFile, const char *dir, int binary);
int  htkamd_mmf_write_sources_full(const htkamd_mmf *s, const float *mean, const float *invCov, const float *gconst, const float *compWeight,
                                   const float *transP, const char *const *masterOut, int nMaster, const char *dir, int binary);

/* Script files (-S scp): white-space separated or quoted words (ScriptWord HShell.c:661), each a data file name or an extended
 * file name logical=physical[start,end] (RegisterExtFileName HShell.c:86: frames start..end of `physical`, known as `logical`). */
typedef struct htkamd_scp htkamd_scp;
int  htkamd_scp_read(const char *path, htkamd_scp **out);
void htkamd_scp_free(htkamd_scp *s);
int  htkamd_scp_count(const htkamd_scp *s);
const char *htkamd_scp_logical(const htkamd_scp *s, int i);
const char *htkamd_scp_physical(const htkamd_scp *s, int i);
long htkamd_scp_start(const htkamd_scp *s, int i);      /* -1 = whole file */
long htkamd_scp_end(const htkamd_scp *s, int i);

/* Label OUTPUT: a transcription (one label list, up to two auxiliary labels per entry, as TranscriptionFromLattice HRec.c:2176
 * builds them: word level none; HVite -m [word]; -f -m [model, word]), HVite's -o formatting (FormatTranscription HRec.c:2368)
 * and the writers (SaveHTKLabels HLabel.c:1481: a score column appears only if some label of the list has a non-zero score in it;
 * master label files as HVite -i writes them).  Times in 100 ns units, -1 = absent. */
#define HTKAMD_OUT_NOSCORES   1      /* -o S */
#define HTKAMD_OUT_NOWORDS    2      /* -o W */
#define HTKAMD_OUT_NOTIMES    4      /* -o T */
#define HTKAMD_OUT_NORMSCORES 8      /* -o N : scores per frame */
#define HTKAMD_OUT_TRISTRIP   16     /* -o X : a-b+c -> b */
#define HTKAMD_OUT_CENTRE     32     /* -o C */
#define HTKAMD_OUT_NOMODELS   64     /* -o M */
typedef struct htkamd_trans htkamd_trans;
typedef struct htkamd_mlf_out htkamd_mlf_out;
int  htkamd_trans_create(int maxAux, htkamd_trans **out);
void htkamd_trans_free(htkamd_trans *t);
int  htkamd_trans_add(htkamd_trans *t, double start, double end, const char *name, float score,
                      const char *aux1, float aux1Score, const char *aux2, float aux2Score);
int  htkamd_trans_format(htkamd_trans *t, double frameDur, int states, int models, int flags);
int  htkamd_trans_append_alternative(htkamd_trans *t, htkamd_trans *alt);   /* N-best: further label lists, written after a line of "///"; t owns alt */
int  htkamd_trans_write(const htkamd_trans *t, const char *path);
int  htkamd_mlf_out_open(const char *path, htkamd_mlf_out **out);
int  htkamd_mlf_out_add(htkamd_mlf_out *o, const char *labFile, const htkamd_trans *t);
void htkamd_mlf_out_close(htkamd_mlf_out *o);

/* ------------------------------------------------------------------------------------------
 * Transcriptions: HTK label files (LoadHTKLabels, HLabel.c:748) and master label files with immediate definitions
 * (LoadMasterFile, HLabel.c:1410).  "[start [end]] name [score] ..." per line, times in 100 ns; only the first
 * alternative ("///") is kept; start/end are -1 when absent.  Pure host code.
 * ------------------------------------------------------------------------------------------ */
typedef struct htkamd_labels htkamd_labels;
typedef struct htkamd_mlf htkamd_mlf;
int  htkamd_labels_read(const char *path, htkamd_labels **out);
void htkamd_labels_free(htkamd_labels *l);
int  htkamd_labels_count(const htkamd_labels *l);
const char *htkamd_labels_name(const htkamd_labels *l, int i);
long long htkamd_labels_start(const htkamd_labels *l, int i);
long long htkamd_labels_end(const htkamd_labels *l, int i);
float htkamd_labels_score(const htkamd_labels *l, int i);
int  htkamd_mlf_read(const char *path, htkamd_mlf **out);
void htkamd_mlf_free(htkamd_mlf *m);
const htkamd_labels *htkamd_mlf_find(const htkamd_mlf *m, const char *labFile);   /* first matching pattern, or NULL */
int  htkamd_mlf_count(const htkamd_mlf *m);                                          /* the entries in file order */
const char *htkamd_mlf_pattern(const htkamd_mlf *m, int i);
const htkamd_labels *htkamd_mlf_entry(const htkamd_mlf *m, int i);

/* ------------------------------------------------------------------------------------------
 * GMM scoring: replaces the state output-probability calls
 *     LogFloat OutP(Observation*,HLink,int)  HModel.h:560 / POutP :561 / SOutP :567 /
 *     MOutP, IDOutP :577-578, and the per-tool caching wrappers ShStrP (HFB.c:898) and
 *     cSOutP/cPOutP (HRec.c:438,512)
 * with one batched call: scores of `ns` tied states for T frames.
 *   dX      device [T*D] row-major feature matrix (Observation.fv[1][1..D] per frame)
 *   dStates device [ns] tied-state indices
 *   dOut    device [ns*ldo]: dOut[k*ldo + t] = log b_{states[k]}(x_t),  ldo >= T
 * Arithmetic = ShStrP/cSOutP: float Mahalanobis sum in dimension order, mixture log-sum with the
 * double-precision LAdd (HMath.c:1576) re-rounded to float after every component: results are
 * bit-identical to the reference.
 * Asynchronous on `stream` (dOut is ready once the stream reaches this point); the call itself allocates and frees nothing after
 * the first few calls.
 * ------------------------------------------------------------------------------------------ */
int htkamd_outp_block(htkamd_model *m, const float *dX, int T, const int *dStates, int ns,
                      float *dOut, int ldo, void *stream);
/* The same scores with a choice of arithmetic:
 *   HTKAMD_SCORE_EXACT  as above (packed-FP32 vector path).
 *   HTKAMD_SCORE_MFMA   Mahalanobis contraction as an fp32 GEMM on the matrix cores ([x^2|x] times per-Gaussian
 *                       coefficients) and a float log-sum-exp over the mixture: within ~1e-4 absolute of the
 *                       reference's float sum (vector sizes up to 40; HTKAMD_EMODEL beyond).  For HERest-style
 *                       accumulation, where the bar is 1e-4 relative on the re-estimated parameters. */
#define HTKAMD_SCORE_EXACT 0
#define HTKAMD_SCORE_MFMA  1
/* Forward-backward only (htkamd_fb_config.scoreMode, may be or-ed with HTKAMD_SCORE_MFMA): the log-add of the alpha/beta
 * recursions (LAdd HMath.c:1576) and the occupation exponentials on fp32 hardware transcendentals; running values stay double.
 * Increment error ~1e-7 absolute: utterance log-probabilities ~1e-9 relative, occupancies / accumulators ~1e-5 relative --
 * inside the 1e-4 bar of the HERest path.  Chains that need the general kernels (models of > 5 states) ignore the bit. */
#define HTKAMD_SCORE_FASTLADD 2
/* The same expanded form on the BF16 matrix pipe, both operands split exactly into three bf16 pieces and the six piece products that
 * matter at fp32 accuracy summed in fp32 (gmm_bf16.hip): the tolerance class of HTKAMD_SCORE_MFMA at ~2.5x its speed (vector sizes up
 * to 48; HTKAMD_EMODEL beyond).  Takes precedence over HTKAMD_SCORE_MFMA when both bits are set. */
#define HTKAMD_SCORE_BF16  4
/* Exact arithmetic with SOutP's rounding (HModel.c:5538-5552: the mixture log-sum kept in double, one rounding to float at the end)
 * instead of ShStrP's / cSOutP's float after every component: what OutP / POutP / SOutP return to a direct caller (HRest, HInit).
 * Bit-identical to the reference's SOutP. */
#define HTKAMD_SCORE_SOUTP 8
/* htkamd_outp_block_mode, htkamd_viterbi_align_mode and htkamd_fb_config.scoreMode; may be or-ed with HTKAMD_SCORE_SOUTP: DOutP's form for DIAGC sets (HModel.c:5347: xmm*xmm/var, the float
 * division) -- what MOutP dispatches to when the set has not been through ConvDiagC, as in HRest / HInit.  Bit-identical to DOutP. */
#define HTKAMD_SCORE_DIAGC 16
/* The expanded form on the FP16 matrix pipe, both operands split into TWO fp16 pieces (11 + 11 significant bits and the signs: fp32's 24)
 * and the three piece products that matter summed in fp32 (gmm_f16.hip): half the matrix instructions of HTKAMD_SCORE_BF16 for the same
 * tolerance class (measured |score - exact| rms 3.4e-5 against 3.2e-5), ~1.45x its speed.  fp16's range is bridged by a power-of-two
 * scale per term, chosen from the model on the device; a feature value far outside anything the model describes (or a model whose
 * coefficients span more than the format) is DETECTED, not computed wrongly: htkamd_fb_results / htkamd_outp_block_mode return
 * HTKAMD_ERANGE and the pass is to be repeated with HTKAMD_SCORE_BF16.  Forward-backward and htkamd_outp_block_mode (vector sizes up
 * to 45); takes precedence over HTKAMD_SCORE_BF16 and HTKAMD_SCORE_MFMA. */
#define HTKAMD_SCORE_F16   32
#define HTKAMD_SCORE_FAST  (HTKAMD_SCORE_MFMA | HTKAMD_SCORE_FASTLADD)
#define HTKAMD_SCORE_FASTEST (HTKAMD_SCORE_F16 | HTKAMD_SCORE_FASTLADD)
int htkamd_outp_block_mode(htkamd_model *m, const float *dX, int T, const int *dStates, int ns,
                           float *dOut, int ldo, int scoreMode, void *stream);
/* HTKAMD_SCORE_F16 through htkamd_outp_block_mode: the calls are asynchronous, so the range flag they raise is the model's.  This waits
 * for the stream and returns HTKAMD_ERANGE if a call since the last check raised it (and clears it): the scores of those calls are to
 * be recomputed with HTKAMD_SCORE_BF16.  (Forward-backward passes carry their own flag: htkamd_fb_results.) */
int htkamd_model_f16_check(htkamd_model *m, void *stream);

/* ------------------------------------------------------------------------------------------
 * Baum-Welch accumulators: MuAcc / VaAcc / WtAcc / TrAcc of HTrain.h:211-232 plus the
 * per-model example counters (hmm->hook, HFB.c:1768-1772) and HERest's totals
 * (totalPr, totalT: HERest.c:779-780), kept on the device as ONE flat vector of doubles so
 * that the parallel-mode merge (HERest -p N dump + -p 0 load: HTrain.c:1453,1625) is a single
 * sum all-reduce over that vector.
 * Vector layout (offsets via htkamd_accs_layout):
 *   mu[G*D] muOcc[G] va[G*D] vaOcc[G] wt[C] wtOcc[S] tr[transOff[nT]] trOcc[sum N] nEgs[H]
 *   totalPr totalT nUttDone nUttSkipped nEval
 * ------------------------------------------------------------------------------------------ */
typedef struct htkamd_accs htkamd_accs;
typedef struct {
   size_t mu, muOcc, va, vaOcc, wt, wtOcc, tr, trOcc, nEgs, totalPr, totalT, nUttDone, nUttSkipped, nEval;
   size_t total;              /* number of doubles */
} htkamd_accs_layout;

int  htkamd_accs_create(htkamd_model *m, htkamd_accs **out);
void htkamd_accs_destroy(htkamd_accs *a);
int  htkamd_accs_zero(htkamd_accs *a, void *stream);                          /* ZeroAccs HTrain.c */
int  htkamd_accs_get_layout(const htkamd_accs *a, htkamd_accs_layout *out);
int  htkamd_accs_device_vector(htkamd_accs *a, double **dVec, size_t *n);      /* for the all-reduce */
int  htkamd_accs_download(htkamd_accs *a, double *hostVec /*[layout.total]*/, void *stream);
int  htkamd_accs_upload_add(htkamd_accs *a, const double *hostVec, void *stream); /* LoadAccs: adds */

/* The exchange step of a multi-GPU pass from C: sum all-reduce of the accumulator vector over RCCL (xGMI inside a node), one process
 * per GPU.  Replaces the dump / load round trip of HERest's parallel mode (DumpAccs HTrain.c:1453 per `-p k` process, LoadAccs
 * HTrain.c:1625 + sum in the `-p 0` process, HERest.c:514-550); afterwards every rank holds the same sums and runs the same update.
 *   comm_unique_id : rank 0 obtains the 128-byte rendezvous id and passes it to the other ranks (file, socket, environment ...)
 *   comm_init      : every rank, same id; nRanks == 1 needs neither RCCL nor an id
 *   accs_allreduce : in place, asynchronous on `stream`
 * RCCL is bound at run time (librccl.so.1); HTKAMD_ENODEV if it cannot be found when nRanks > 1. */
typedef struct htkamd_comm htkamd_comm;
int  htkamd_comm_unique_id(void *id128);
int  htkamd_comm_init(htkamd_comm **out, int nRanks, int rank, const void *id128);
void htkamd_comm_destroy(htkamd_comm *c);
int  htkamd_comm_ranks(const htkamd_comm *c);
int  htkamd_accs_allreduce(htkamd_accs *a, htkamd_comm *c, void *stream);
/* The exchange with fp32 on the wire (half the bytes: SURVEY §8(e)'s 25.9 MB): every rank rounds its fp64 partial statistics to float
 * once, RCCL sums floats, the sums return to the fp64 vector; nEgs / totalPr / totalT / the counters stay fp64 (a second, small
 * all-reduce).  The reference's merge adds float dumps (LoadAccs HTrain.c:1625-1687): this is tighter.  accs_wire_round applies the
 * rounding alone (one rank's share of it, for emulating the exchange in tests); comm_agree_max = max over the ranks of one int,
 * synchronous -- a decision all ranks must take alike (the fp16 -> bf16 fallback of an iteration). */
#define HTKAMD_WIRE_F64 0
#define HTKAMD_WIRE_F32 1
int  htkamd_accs_allreduce_wire(htkamd_accs *a, htkamd_comm *c, int wire, void *stream);
int  htkamd_accs_wire_round(htkamd_accs *a, void *stream);
int  htkamd_comm_agree_max(htkamd_comm *c, int *value, void *stream);
/* The exchange in parts, behind a pass in two phases (htkamd_fb_execute_begin / _mix): the statistics of tied states [state0, state1) travel
 * while the next range of states is still being summed.  One logical exchange per iteration (what `HERest -p 0 HER*.acc` merges,
 * HERest.c:514-557, HTrain.c:1625-1687), cut along the accumulator vector.
 *   htkamd_accs_state_ranges   the ranges of the vector that belong to those states -- mu, muOcc, va, vaOcc of their Gaussians, wt of their
 *                              components, wtOcc -- and with `withRest` what no state owns and the whole-vector exchange sends as
 *                              statistics (tr, trOcc): up to 7 ranges in off[] / len[] (doubles), their number in *n.  Needs a set whose
 *                              components own their Gaussians in state order (compGauss[c] == c: no shared pdfs); else HTKAMD_EMODEL,
 *                              and the caller exchanges the vector whole.
 *   htkamd_accs_pack_ranges    the ranges, one behind the other, into `dst` as floats (HTKAMD_WIRE_F32) or doubles; _unpack_ranges back.
 *                              For hosts with a collective of their own (bench.py: torch.distributed).
 *   htkamd_accs_allreduce_states   pack, sum over the ranks (RCCL), unpack -- all on `stream`; `withRest` adds tr / trOcc to the part and
 *                              sums the counters behind them (nEgs ... nEval) in fp64 as htkamd_accs_allreduce_wire does.  Calls with
 *                              withRest = 1 once per iteration, and every state once, leave every rank with the vector the whole
 *                              exchange would have left (bit for bit on the fp64 wire, for any ring order on the fp32 wire: the same
 *                              values are rounded and summed). */
int  htkamd_accs_state_ranges(htkamd_accs *a, int state0, int state1, int withRest, size_t off[7], size_t len[7], int *n);
int  htkamd_accs_pack_ranges(htkamd_accs *a, int n, const size_t *off, const size_t *len, int wire, void *dst, void *stream);
int  htkamd_accs_unpack_ranges(htkamd_accs *a, int n, const size_t *off, const size_t *len, int wire, const void *src, void *stream);
int  htkamd_accs_allreduce_states(htkamd_accs *a, htkamd_comm *c, int wire, int state0, int state1, int withRest, void *stream);

/* HTK parameter files: header + big-endian float rows, _C compression and _K checksum on input
 * (ReadHTKHeader HWave.c:1408, OpenParmChannel HParm.c:3561, GetParm :3464, UpdateCRCC :3357).  *data is malloc'd
 * (release with htkamd_free); *kind comes back without the _C/_K bits. */
int  htkamd_parm_read(const char *path, float **data, int *nFrames, int *nCols, int *sampPeriod, int *kind);
int  htkamd_parm_write(const char *path, const float *data, int nFrames, int nCols, int sampPeriod, int kind, int withCrc);
void htkamd_free(void *p);
/* Waveform files, the sources of the MFCC front end: SOURCEFORMAT = WAV (RIFF 16-bit mono PCM, GetWAVHeaderInfo HWave.c:1052) or
 * HTK (big-endian WAVEFORM file).  *samples is malloc'd (htkamd_free); *sampPeriod in 100 ns units (625 at 16 kHz). */
#define HTKAMD_WAVE_HTK 1
#define HTKAMD_WAVE_WAV 2
int  htkamd_wave_read(const char *path, int format, short **samples, long *nSamples, double *sampPeriod);

/* Accumulator files (HERN.acc) for exchanging statistics with the reference's parallel mode: DumpAccs
 * (HTrain.c:1453) + trailer (HERest.c:546-548) and LoadAccs (HTrain.c:1625; adds).  Pure host functions on the
 * flat vector; `names[h]` is the physical HMM name in definition order (the HMM list).  Files follow the
 * reference's HMM-scan order, so `HERest -p 0` reads what is written here and vice versa. */
int htkamd_accs_layout_from_desc(const htkamd_model_desc *d, htkamd_accs_layout *out);
int htkamd_hmm_scan_order(const char *const *names, int H, int *order);
int htkamd_accs_dump_file(const htkamd_model_desc *d, const double *hostVec, const char *const *names, int uFlags, const char *path);
int htkamd_accs_load_file(const htkamd_model_desc *d, double *hostVec, const char *const *names, int uFlags, const char *path);
/* The same for a set with tied mean / variance vectors (meanShare / varShare as in htkamd_model_set_sharing, either may be NULL): a
 * shared vector has ONE MuAcc / VaAcc record in the file, where the scan first meets it (HTrain.c:1484-1493).  The writer puts the sum
 * over the sharers there; the reader adds the record to the vector's first sharer, which is all htkamd_model_update needs. */
int htkamd_accs_dump_file_shared(const htkamd_model_desc *d, const double *hostVec, const char *const *names, int uFlags,
                                 const int *meanShare, const int *varShare, const char *path);
int htkamd_accs_load_file_shared(const htkamd_model_desc *d, double *hostVec, const char *const *names, int uFlags,
                                 const int *meanShare, const int *varShare, const char *path);
/* HERest -s file: per physical HMM (scan order) its index, quoted name, example count and the occupation of each emitting
 * state -- StatReport / PrintStats (HERest.c:708-747), the input of HHEd's RO / TB / TC commands. */
int htkamd_stats_write_file(const htkamd_model_desc *d, const double *hostVec, const char *const *names, const char *path);

/* ------------------------------------------------------------------------------------------
 * Model update after a pass: UpdateModels (HERest.c:1326) -> MLUpdateModels (HERest.c:1262) with
 * UpdateTrans :795, UpdateWeights :897 (+FloorMixes :819), UpdateVars :1045, UpdateMeans :974 and
 * FixGConsts (HModel.c:5688).  Runs on the host (milliseconds, as in the reference) from a host copy of
 * the summed accumulator vector, then refreshes the device tables.  With HTKAMD_UPMAP in uFlags: MAPUpdateModels (HMap.c:413)
 * with its UpdateWeights :205, UpdateVars :314, UpdateMeans :279 -- host update only.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
   int   minEgs;            /* HERest -m, default 3 (HERest.c:96)                                  */
   float minVar;            /* HERest -v, default 0.0 (HERest.c:95)                                */
   float mixWeightFloor;    /* HERest -w f gives f*MINMIX (HERest.c:425), default 0.0              */
   int   uFlags;            /* HTKAMD_UP* bits                                                     */
   int   singleProcess;     /* 1 = parMode -1: ForceDiagC/ConvExpWt round trips (HERest.c:1336-1339) */
   const float *varFloor;   /* [vecSize] per-component floor = the ~v "varFloor1" macro (SetVFloor HModel.c:3512: when the
                               macro exists it replaces minVar); NULL = minVar everywhere                */
   int   rowNormalise;      /* 1 = transition rows renormalised by their sum, as the isolated-unit trainer does
                               (RestTransP HRest.c:1015); 0 = HERest's UpdateTrans                       */
   float mapTau;            /* HTKAMD_UPMAP only: HMAP: MAPTAU, the weight of the prior (HMap.c:82, default there 20.0).  With UPMAP the
                               other fields mean what HMap's own configuration means: minEgs = HMAP: MINEGS (default 0), minVar = HMAP:
                               MINVAR (default 0.0), mixWeightFloor = MINMIX * HMAP: MIXWEIGHTFLOOR; HTKAMD_UPTRANS is refused
                               (HError 999 "No support for MAP updating transition probabilities", HMap.c:434)   */
   float mapMinObs;         /* HMAP: MINOBS: a mean counts as observed in stats.nMapObserved above this occupation          */
} htkamd_update_config;
typedef struct {
   int nFloorVar, nFloorVarMix;      /* "Total %d floored variance elements in %d different mixes"  */
   int nSkippedHmm;                  /* models copied because they had < minEgs examples (-2331)     */
   int nNoTransOut, nNoMixUse, nNoVarUse;   /* warnings -2326 / -2330                                */
   int nWeightAboveOne;              /* re-estimated mixture weights above 1.001: fatal HError 2393 in UpdateWeights (HERest.c:926);
                                        the update is carried out (weights clamped to 1) and the call returns HTKAMD_EMODEL */
   int nMapObserved;                 /* HTKAMD_UPMAP: "Observed components (means) %d of ..." (HMap.c:452)                    */
} htkamd_update_stats;
int htkamd_model_update(htkamd_model *m, const htkamd_accs *accs, const double *hostVec,
                        const htkamd_update_config *cfg, htkamd_update_stats *stats);
/* The same update on the device, straight from the accumulator vector where it lies (after the all-reduce): nothing but the
   transition matrices (for the host's minimum-duration table) and the counters of `stats` crosses PCIe, and every table the kernels
   read -- 1/variance, the interleaved scoring rows, log weights, the matrix-core fragment table -- is rebuilt in place.
   Arithmetic as htkamd_model_update; `stats` may be NULL.  Synchronises `stream` before returning. */
int htkamd_model_update_device(htkamd_model *m, htkamd_accs *accs, const htkamd_update_config *cfg, htkamd_update_stats *stats, void *stream);
/* The same in two halves for a host loop that wants the next pass queued behind the update's kernels before it waits: _begin launches
   everything and the copy of the transition matrices + counters and returns; _end waits for that copy only (an event, not the stream) and
   folds it into the host tables.  Between the two the host tables are the OLD ones: a pass queued in between runs on the new parameters
   (stream order) with batch tables prepared for the old minimum durations -- after _end, htkamd_fb_prepared_current tells whether that
   pass has to be repeated (a minimum duration changed: rare).  One update in flight per model. */
int htkamd_model_update_device_begin(htkamd_model *m, htkamd_accs *accs, const htkamd_update_config *cfg, void *stream);
int htkamd_model_update_device_end(htkamd_model *m, htkamd_update_stats *stats);

/* MLLR mean transforms of one speaker over a regression class tree (htkamd_mmf_regtree): what HERest -u a estimates at transform time (HAdapt.c), from the statistics of any
   forward-backward pass over the speaker's data.  One-stream DIAGC continuous sets.  A separate surface: no pass, update or decoder changes.
     config           : splitThresh SPLITTHRESH (<= 0: MLLRMEANSPLITTHRESH's default 1000), minOccThresh MINOCCTHRESH, useBias USEBIAS,
                        blockSize[nBlocks] BLOCKSIZE (nBlocks 0: one block of the vector size; a block has at most 64 rows).
     mllr_check       : the refusals alone, no device (HTKAMD_EMODEL / HTKAMD_EINVAL and the reason): sets with more than one stream, FULLC,
                        tied-mixture and discrete sets; no tree (ADAPTKIND = BASE); blocks that do not sum to the vector size; a tree with
                        a component that is no Gaussian of the set.
     mllr_estimate    : per Gaussian occ = muOcc and spSum = the plain sum of gamma o.  htkamd_accs holds mu = sum of gamma (o - mean), so
                        spSum = mu + occ * mean, formed in fp64 and rounded to float once (the reference keeps occ and spSum as floats).
                        On the device (csrc/mllr.hip): G and k of every base class as AccMLLRPDFStats (:1709) forms them -- float factors in
                        the reference's order, fp64 sums in a fixed order, no atomics --, the sums up the tree (the reference re-accumulates
                        every node from its Gaussians: another fp64 order), and per chosen node and row the solve of G w = k in fp64.
                        Which nodes get a transform, their numbering and the classes' transforms are ParseNode's (:1547) with the strict >.
                        Returns HTKAMD_OK and the set; HTKAMD_MLLR_NOSET (positive; a set without transforms) when the root's occupation
                        does not exceed the threshold; HTKAMD_ERANGE, naming node and row, when a row's G is not positive definite (the
                        reference's InvSVD would zero the small singular values; here nothing is estimated on such statistics).
     xformset_*       : accessors (transforms and classes count from 1; xform gives A as [D][D], zero outside the blocks; node_occ
                        SetNodeOcc's occupations by node; kernel_ms the device time of statistics, tree sums and solves);
                        write / read: the text form of a transform file as SaveOneXForm (HModel.c:4804) writes it for -K, byte for byte.
                        read refuses, by name: <PARENTXFORM>, <XFORMKIND> other than MLLRMEAN, <ADAPTKIND> other than TREE, binary files.
     mllr_apply       : mean' = A mean + b for every Gaussian of a class with a transform (float products, float sums in index order, the
                        bias last), into the model's mean table; every derived scoring table follows as after htkamd_model_update_device.
                        gaussClass[G]: the base class (from 1; 0 none) of every Gaussian, or NULL for a set that mllr_estimate made.
                        The original means are kept: mllr_restore puts them back bit for bit.  A second apply without a restore is refused
                        (parent transforms are not supported), and so are sets with shared mean vectors (mllr_check and mllr_estimate
                        refuse those too).  While a model is adapted its parameters are not to be replaced: htkamd_model_update*,
                        htkamd_model_set_params and the unit trainers do not know of the kept means, and a later mllr_restore would put
                        the means of before the apply over theirs.  Restore first, then re-estimate.
   Diagnostic entry point (a test aid, as htkamd_regtree_probe is one):
     mllr_probe       : the device steps over a caller's tables: mean, var [G][D], occ [G], spSum [G][D], the class (from 1; 0 none) of
                        every Gaussian, the tree (children from 1, 0 0 a terminal; classes count the terminals in node order).  stats
                        [nNodes][htkamd_mllr_record_len] (or NULL): per row i of a block of size bs the lower triangle of G_i packed by
                        rows ((bs+1)(bs+2)/2, the bias row and column last), then k_i (bs+1); the node's occupation is the record's last
                        word.  A [nNodes][D][D], bias [nNodes][D], W [nNodes][D][maxBlock+1] (or NULL; the fp64 rows) of the first nX. */
#define HTKAMD_MLLR_NOSET 1
typedef struct htkamd_xformset htkamd_xformset;
typedef struct { float splitThresh, minOccThresh; int useBias, nBlocks; const int *blockSize; } htkamd_mllr_config;
int  htkamd_mllr_check(const htkamd_mmf *s, const htkamd_regtree *t, const htkamd_mllr_config *cfg);
int  htkamd_mllr_estimate(htkamd_mmf *s, htkamd_model *m, htkamd_accs *a, const htkamd_regtree *t, const htkamd_mllr_config *cfg, htkamd_xformset **out, void *stream);
int  htkamd_mllr_gauss_classes(const htkamd_mmf *s, const htkamd_regtree *t, int *cls /*[numGauss]*/);
int  htkamd_mllr_select(int nNodes, const int *left, const int *right, const double *nodeOcc, float thresh, int *nX, int *xNode /*[nNodes]*/, int *classX /*[terminals]*/);
int  htkamd_mllr_apply(htkamd_model *m, const htkamd_xformset *x, const int *gaussClass /*[numGauss] or NULL*/, void *stream);
int  htkamd_mllr_restore(htkamd_model *m, void *stream);
int  htkamd_xformset_from_tables(int D, int nBlocks, const int *blockSize, int useBias, int nX, const float *A /*[nX][D][D]*/, const float *bias /*[nX][D]*/, int nClass,
                                 const int *classX, const char *name, const char *baseName, htkamd_xformset **out);
int  htkamd_xformset_set_names(htkamd_xformset *x, const char *name /*or NULL*/, const char *baseName /*or NULL*/);
int  htkamd_xformset_num_xforms(const htkamd_xformset *x);
int  htkamd_xformset_num_classes(const htkamd_xformset *x);
int  htkamd_xformset_vec_size(const htkamd_xformset *x);
int  htkamd_xformset_use_bias(const htkamd_xformset *x);
int  htkamd_xformset_blocks(const htkamd_xformset *x, int *blockSize /*[cap] or NULL*/, int cap);
int  htkamd_xformset_class_xform(const htkamd_xformset *x, int baseClass);
int  htkamd_xformset_xform_node(const htkamd_xformset *x, int xform);
int  htkamd_xformset_xform(const htkamd_xformset *x, int xform, float *A /*[D][D] or NULL*/, float *bias /*[D] or NULL*/);
int  htkamd_xformset_node_occ(const htkamd_xformset *x, double *occ /*[cap] or NULL*/, int cap);
void htkamd_xformset_kernel_ms(const htkamd_xformset *x, float *ms /*[3]*/);
int  htkamd_xformset_write(const htkamd_xformset *x, const char *path);
int  htkamd_xformset_read(const char *path, htkamd_xformset **out);
void htkamd_xformset_destroy(htkamd_xformset *x);
size_t htkamd_mllr_record_len(int D, int nBlocks, const int *blockSize);
int  htkamd_mllr_probe(const float *mean, const float *var, const double *occ, const double *spSum, const int *cls, int G, int D, int nNodes, const int *left,
                       const int *right, const htkamd_mllr_config *cfg, double *stats, size_t statsCap, double *nodeOcc, int *nX, int *xNode, int *classX,
                       float *A, float *bias, double *W, int *badNode, int *badRow, float *ms, void *stream);
/* Current parameters (DIAGC variances, linear weights, log transitions); any pointer may be NULL. */
int htkamd_model_get_params(htkamd_model *m, float *mean, float *var, float *gconst, float *compWeight, float *transP);

/* ------------------------------------------------------------------------------------------
 * Forward-backward over a batch of utterances: replaces, per utterance,
 *     Boolean FBFile(FBInfo*, UttInfo*, char *datafn)          HFB.h:143 / HFB.c:1923
 * i.e. StepBack (SetBeamTaper, Setotprob, SetBeta with the beta beam and its retry loop) and
 * StepForward (StepAlpha with the alpha beam, SetOcct, UpMixParms, UpTranParms).
 * The label sequence of an utterance is the list of physical-HMM indices CreateInsts
 * (HFB.c:508) derives from the transcription.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
   double pruneInit, pruneInc, pruneLim;   /* HERest -t f [i l]; HTKAMD_NOPRUNE = off (HERest.c:121-123) */
   float  minFrwdP;                        /* HFB MINFORPROB / HERest -c, default 10.0 (HFB.c:83)        */
   int    uFlags;                          /* HTKAMD_UP* bits                                            */
   int    scoreMode;                       /* HTKAMD_SCORE_EXACT (0, default), or HTKAMD_SCORE_MFMA | HTKAMD_SCORE_FASTLADD bits; the EXACT
                                              family's HTKAMD_SCORE_SOUTP | HTKAMD_SCORE_DIAGC for HRest's arithmetic (htkamd_hrest) */
} htkamd_fb_config;

typedef struct {
   int          nUtt;
   const float *dX;          /* device [frameOff[nUtt]*D] all utterances' frames, row-major  */
   const int   *frameOff;    /* host [nUtt+1]                                               */
   const int   *labOff;      /* host [nUtt+1]                                               */
   const int   *labs;        /* host [labOff[nUtt]] physical HMM index of each label        */
} htkamd_batch_desc;

/* per-utterance status values */
#define HTKAMD_UTT_OK        1
#define HTKAMD_UTT_SKIPPED   0        /* HError -7324: no path / qt > T (HFB.c:1339-1356)   */
#define HTKAMD_UTT_ETEE     (-7332)   /* tee-model placement (HFB.c:557,564)                */
#define HTKAMD_UTT_EALPHA   (-7390)   /* alpha prune failed (HFB.c:706,718)                 */

typedef struct htkamd_fb htkamd_fb;

int  htkamd_fb_create(htkamd_model *m, htkamd_fb **out);
void htkamd_fb_destroy(htkamd_fb *fb);
/* Test aid; call before prepare.  bit 0: keep every alpha column (T*cells doubles more per utterance);
   bit 1: force the general workgroup-per-utterance kernels even where the wave-per-utterance path applies;
   bit 2: keep utterances off the lane-per-chain-state kernels (they then take the lane-per-model ones). */
int  htkamd_fb_set_debug(htkamd_fb *fb, int on);
/* Host part of CreateInsts/SetBeamTaper for the whole batch + upload of the chain tables.
   Limits per utterance: chains of up to 512 models when no model has more than 5 states, otherwise up to
   1024 model states; an utterance beyond them fails the call with HTKAMD_EINVAL (nothing is truncated). */
int  htkamd_fb_prepare(htkamd_fb *fb, const htkamd_batch_desc *batch, void *stream);
/* The batch tables depend on the transcriptions and on the models' minimum durations only, so a batch may be prepared ahead of the
   pass that uses it (e.g. for the next EM iteration while this one's kernels run) and executed any number of times.  Returns 0 when
   a model update has since changed a minimum duration (a transition reached or left zero): htkamd_fb_execute then refuses the batch
   (HTKAMD_EINVAL) and it must be prepared again. */
int  htkamd_fb_prepared_current(const htkamd_fb *fb);
/* Device part: scores, beta pass, alpha pass + statistics into `accs`. Asynchronous on `stream`. */
int  htkamd_fb_execute(htkamd_fb *fb, const htkamd_fb_config *cfg, htkamd_accs *accs, void *stream);
/* Waits for the stream and copies per-utterance log-probabilities (utt->pr) and status. */
/* The pass in two phases (multi-GPU hosts: a range of states' statistics is exchanged while the next is being summed).  _begin: everything
   but the state-bucketed mixture statistics (UpMixParms HFB.c:1426 for the left-to-right path's surviving pairs); *deferred = 1 when those
   wait for _mix, 0 when the pass was of another kind and is complete.  _mix: the statistics of tied states [state0, state1); every state
   once per pass, any order.  Behind _mix the ranges htkamd_accs_state_ranges names for those states are final on this rank; what no state
   owns is final behind _begin.  htkamd_fb_execute = _begin + _mix(0, numStates). */
int  htkamd_fb_execute_begin(htkamd_fb *fb, const htkamd_fb_config *cfg, htkamd_accs *accs, void *stream, int *deferred);
int  htkamd_fb_execute_mix(htkamd_fb *fb, int state0, int state1, void *stream);
int  htkamd_fb_results(htkamd_fb *fb, double *pr /*[nUtt]*/, int *status /*[nUtt]*/, void *stream);
/* For host loops that queue the next pass before they read this one's results: the copy of the results queued on `stream` (the stream
   htkamd_fb_execute ran on) right behind the pass; htkamd_fb_results then only waits for that copy. */
int  htkamd_fb_results_begin(htkamd_fb *fb, void *stream);
/* Number of (frame, chain-state) output-probability evaluations the reference would perform
   for the prepared batch without pruning (Setotprob visits) -- the unit of the throughput metric. */
long long htkamd_fb_frame_states(const htkamd_fb *fb);
/* Debug/test access to one utterance's trellis after execute (device -> host copies):
   beta/alpha [T*Q*maxN] (NaN where the reference holds no vector), outp [T*Q*maxN], beams [T]. */
int  htkamd_fb_get_trellis(htkamd_fb *fb, int utt, double *beta, double *alpha, float *outp,
                           int *qLo, int *qHi, int *aLo, int *aHi, int *T, int *Q, int *maxN, void *stream);
/* Seconds spent in the kernels of the last execute, measured with HIP events on `stream`:
   out[0]=scoring (the dispatch's own start -> stop, hipExtLaunchKernel: what a kernel trace reports even when other streams share
   the device) out[1]=beta out[2]=alpha+occ/trans out[3]=mixture statistics (intervals between stream events). Synchronises.
   An interval the pass did not measure (htkamd_fb_set_event_mode(fb, 1)) reads -1, and so does a sum with one. */
int  htkamd_fb_kernel_times(htkamd_fb *fb, double out[4]);
/* the same with the alpha pass and the left-to-right path's frame-parallel statistics apart: scoring, beta, alpha, statistics, mixture statistics */
int  htkamd_fb_kernel_times5(htkamd_fb *fb, double out[5]);
/* Which events htkamd_fb_execute records for the two calls above: 0 (default) the scoring dispatch's own start / stop plus stream events between
   the kernels (each a barrier packet: 20 - 40 us of a 2 ms pass in all); 1 the scoring dispatch's only -- the other intervals then read -1. */
int  htkamd_fb_set_event_mode(htkamd_fb *fb, int mode);
/* the last pass's mixture statistics in units (UpMixParms HFB.c:1573-1721): out[0] (frame, state) pairs past the MINFORPROB prune, out[1] (frame,
   state, component) triples accumulated; -1 where the pass did not count them (sets of several streams, states of more than 16 components) */
int  htkamd_fb_mix_counts(htkamd_fb *fb, long long out[2]);
/* the prepared batch's work on the matrix cores, counted on the host from its task list (the 32 x 32 x 16 pair kernels, one state per
   16-component tile): out[0] matrix instructions (per operand-piece product and k-step 1; multiply by the kernel's 6 x 5 or 3 x 5) a pass
   issues per (wavefront, pair of states) it does not sit out, out[1] the same with every wavefront of a task working on every pair (before the
   per-state frame ranges of Setotprob, HFB.c:1014, reached the kernel), out[2] what the (frame, chain state) evaluations need: units / 64 */
int  htkamd_fb_score_work(const htkamd_fb *fb, long long out[3]);

/* ------------------------------------------------------------------------------------------
 * Viterbi forced alignment of a batch (HVite -a): replaces, per utterance, the frame loop of
 * HVite.c:640-710 ProcessFile on the alignment network of DoAlignment (HVite.c:830):
 *     StartRecognition / ProcessObservation / CompleteRecognition      HRec.h:170-190
 *     TranscriptionFromLattice (HRec.c:2176) for the state (-f) and model (-m) level labels
 * The network is the linear chain of the transcription's physical models (LatticeFromLabels +
 * ExpandWordNet with one pronunciation per word).  genBeam is HVite's -t value (1e10 = off).
 * Results are per chain state (one segment per emitting state, start = -1 if the state was skipped):
 * frames [segStart, segEnd) 0-based and segScore = acoustic score of the segment, and per model
 * [modStart, modEnd), modScore -- the numbers HVite prints as "start end s<j> score model score".
 * Token likelihoods are the same double additions in the same order as HRec's, on bit-exact output
 * probabilities, so segmentations are bit-identical to the reference's.
 * Chains of <= 512 models of <= 5 states run on 1..8 wavefronts per utterance; longer chains and larger
 * models a workgroup per utterance (same results).  Word networks: htkamd_decode_* below.
 * ------------------------------------------------------------------------------------------ */
typedef struct htkamd_viterbi htkamd_viterbi;
int  htkamd_viterbi_create(htkamd_model *m, htkamd_viterbi **out);
void htkamd_viterbi_destroy(htkamd_viterbi *v);
int  htkamd_viterbi_align(htkamd_viterbi *v, const htkamd_batch_desc *batch, float genBeam, void *stream);
/* The same with the state scores in another arithmetic of the EXACT family: HTKAMD_SCORE_SOUTP (SOutP's double accumulation with one
 * float rounding, HModel.c:5538) and / or HTKAMD_SCORE_DIAGC (DOutP's division by the variance, HModel.c:5347) -- what HInit's
 * ViterbiAlign (HInit.c:792, OutP on a set that has not been through ConvDiagC) computes.  0 = htkamd_viterbi_align. */
int  htkamd_viterbi_align_mode(htkamd_viterbi *v, const htkamd_batch_desc *batch, float genBeam, int scoreMode, void *stream);
int  htkamd_viterbi_sizes(const htkamd_viterbi *v, size_t *nSeg /* sum of chain states */, size_t *nMod /* sum of models */);
int  htkamd_viterbi_results(htkamd_viterbi *v, int *segStart, int *segEnd, double *segScore,
                            int *modStart, int *modEnd, double *modScore,
                            double *total /*[nUtt]*/, int *status /*[nUtt]*/, void *stream);

/* ------------------------------------------------------------------------------------------
 * Recognition network: word lattice (SLF) + dictionary -> model-level network, for context-independent sets.
 * Replaces ReadLattice (HNet.c:631), ReadDict (HDict.c:224) and ExpandWordNet (HNet.c:3438, xc == 0 form): per lattice
 * node and pronunciation a chain of HMM nodes ending in a WORD node, NULL nodes for !NULL words, lattice arcs as links
 * carrying the LM log probability, node 0 = the network's initial null node, node 1 = its final null node
 * (AddInitialFinal HNet.c:2180).  Pure host code.
 * ------------------------------------------------------------------------------------------ */
#define HTKAMD_NODE_HMM  0     /* model = physical HMM index */
#define HTKAMD_NODE_WORD 1     /* model = pronunciation index (htkamd_net_out_sym), pronProb = log pron prob */
#define HTKAMD_NODE_NULL 2
typedef struct {
   int nNodes, nLinks, nProns, initial, final;
   const int   *kind, *model;
   const float *pronProb;
   const int   *linkOff;     /* [nNodes+1] links of node n: linkOff[n]..linkOff[n+1) */
   const int   *linkDest;
   const float *linkLike;    /* LM log probability of the link (NetLink.like) */
} htkamd_net_desc;
typedef struct htkamd_net htkamd_net;
int  htkamd_net_build(const char *slfPath, const char *dictPath, const htkamd_mmf *hmms, htkamd_net **out);
/* The same with HNet's configuration switches (HNet.c:122-127; HVite reads them from its -C file):
 *   ALLOWXWRDEXP   contexts may cross word boundaries: when the model set defines contexts and the dictionary cannot be built from
 *                  word-internal models alone (or one of the FORCE switches is set) the network is expanded with CROSS-WORD contexts
 *                  (ExpandWordNet HNet.c:3438 with xc > 0): a word's first model depends on the last context phone of the word before,
 *                  its last model on the first context phone of the word after; context-free phones (sp) and null words pass contexts on
 *   FORCECXTEXP    expand contexts even when every dictionary phone is a model name      FORCELEFTBI / FORCERIGHTBI   biphone names only
 * flags = 0 is htkamd_net_build.  With cross-word expansion `hmms` must stay alive as long as the network (htkamd_net_seq_models). */
#define HTKAMD_NET_ALLOWXWRDEXP 1
#define HTKAMD_NET_FORCECXTEXP  2
#define HTKAMD_NET_FORCELEFTBI  4
#define HTKAMD_NET_FORCERIGHTBI 8
int  htkamd_net_build_ex(const char *slfPath, const char *dictPath, const htkamd_mmf *hmms, int flags, htkamd_net **out);
int  htkamd_net_is_xwrd(const htkamd_net *n);
/* Physical models of pronunciation `pron` when it stands between the pronunciations prevPron and nextPron (-1: utterance boundary;
 * pronunciations without phones are transparent, so pass the nearest one that has phones): what HVite -m labels for a recognised
 * word sequence.  Without cross-word expansion this is htkamd_net_pron_models.  Returns the number of models (may exceed `max`). */
int  htkamd_net_seq_models(const htkamd_net *n, int pron, int prevPron, int nextPron, int *models, int max);
/* Alignment network of HVite -a from a word-level transcription: LatticeFromLabels (HNet.c:1516: one node per label, the boundary
   word of HVite -b at both ends when non-NULL) + the same expansion; decoding it with htkamd_decoder_* is HVite -a (DoAlignment
   HVite.c:830), word- or model-level (-m) labels. */
int  htkamd_net_build_words(const char *const *words, int nWords, const char *boundary, const char *dictPath,
                            const htkamd_mmf *hmms, htkamd_net **out);
void htkamd_net_destroy(htkamd_net *n);
const htkamd_net_desc *htkamd_net_get(const htkamd_net *n);
const char *htkamd_net_out_sym(const htkamd_net *n, int pron);
/* physical models of pronunciation `pron` after context expansion; returns their number (which may exceed max) */
int  htkamd_net_pron_models(const htkamd_net *n, int pron, int *models, int max);
const char *htkamd_net_word_name(const htkamd_net *n, int pron);

/* ------------------------------------------------------------------------------------------
 * Network decoding of a batch (HVite -w net): replaces, per utterance, InitVRecInfo / StartRecognition /
 * ProcessObservation / CompleteRecognition (HRec.h:150-190) with nToks = 1 and TranscriptionFromLattice (HRec.c:2176)
 * for the word-level 1-best labels.  genBeam / wordBeam = HVite -t / -v (1e10 = off), lmScale -s, wordPen -p, prScale -r.
 * LikeToWord look-ahead (HRec.c:1172) depends on the LM scale, hence lmScale at creation.
 * Results per utterance u: nWords[u] (-1: no token reached the end of the network, -3: more than maxWords words; from the walk of HRec's
 * instance list -- HTKAMD_ORDER_EXACT and N-best runs only, in the default HTKAMD_ORDER_AUTO mode such an utterance keeps the batch kernel's
 * answer --: -4 out of Path records, -5 more list appends in one frame than 8 nNodes + 1024, -6 zero-time nodes nested deeper than 64), and for
 * word w < nWords[u] at [u*maxWords + w]: pronunciation index (htkamd_net_out_sym), frames [start, end), score = LArcTotLike
 * (acoustic + scaled LM + scaled pron prob + word penalty, HNet.h:257), wordLm (may be NULL) = the arc's LM log probability
 * (LArc.lmlike: what HVite -m/-f print, scaled and with the word penalty, as the word's auxiliary score); total[u] = likelihood
 * of the final token.  Model-level labels of the recognised words (HVite -m with -w) = htkamd_viterbi_align on the chain of
 * htkamd_net_pron_models of the recognised pronunciations: for a fixed word sequence the LM terms are constants, so the best
 * alignment of that chain is the decoder's path.
 * Models of up to 8 states; tee models may not have more than 95 predecessors.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
   float genBeam, wordBeam, lmScale, wordPen, prScale;
   int   scoreMode;   /* HTKAMD_SCORE_EXACT (0): scores, token likelihoods and therefore paths are the reference's bit for bit;
                         HTKAMD_SCORE_MFMA: matrix-core scores (1e-4 class) -- same words unless two paths tie within that */
   int   maxActive;   /* HVite -u: maximum-model pruning (ProcessObservation HRec.c:1966-1985); 0 = off */
} htkamd_decode_config;
typedef struct htkamd_decoder htkamd_decoder;
int  htkamd_decoder_create(htkamd_model *m, const htkamd_net_desc *net, float lmScale, htkamd_decoder **out);
/* N-best token passing and lattice generation (HVite -n N [-z ext]; HRec.c with nToks > 1: TokSetMerge :279, StepWord2's NxtPath
 * chains :1046, CreateLattice :1679 / LatFromPaths :1512).  Every state keeps its best token and up to nToks-1 alternatives that
 * differ in the word they came from; the lattice of an utterance = the word ends reachable from the final token set:
 *   node 0 = start, node 1 = end (both !NULL, nodePron -1), the others word ends {frame, pronunciation, likelihood of the Path};
 *   arc = one way into a word end: aclike, lmlike (unscaled LM log probability), prlike (log pronunciation probability).
 * nToks: 2..8;  nBeam: alternatives more than this below the frame's best token are dropped (HVite uses its -t value);
 * cfg->maxActive must be 0.  Outputs per utterance u at [u*maxLatNodes + i] / [u*maxLatArcs + j]; nNodes[u] = -1: no token reached
 * the end, -3: the lattice did not fit.  Pointers other than nNodes / nArcs may be NULL. */
typedef struct {
   int *nNodes, *nArcs;
   int *nodeFrame, *nodePron, *nodeNet;
   double *nodeLike;
   int *arcStart, *arcEnd;
   float *arcAc, *arcLm, *arcPr;
   double *arcScore;
   double *total;
} htkamd_lattice_out;
int  htkamd_decoder_run_lattice(htkamd_decoder *d, const htkamd_decode_config *cfg, int nToks, float nBeam, const float *dX, const int *frameOff, int nUtt,
                                int maxLatNodes, int maxLatArcs, const htkamd_lattice_out *out, void *stream);
/* The same with alignment records inside the arcs (HVite -n together with -m: alignMode & 1, model records / -f: alignMode & 2, state
 * records; LatFromPaths' lAlign, HRec.c:1582-1656, as the reference built with -DPHNALG -- HTKLib/Makefile.in:45 -- writes it: the records
 * of a relative token carry the BEST token's likelihoods, so an alternative's alignment likelihoods need not add up to its arc's).  Arc j
 * of utterance u owns records [arcAlignOff[u*(maxLatArcs+1) + j], .. + j + 1) of alState (-1: a model record) / alModel (physical model)
 * / alDur (frames) / alLike at u*maxAlign + i.  Alignment records are kept for the whole utterance on the device (frames x models x
 * tokens of them): meant for rescoring-size networks.  nNodes[u] = -3 also when they (or maxAlign) do not fit. */
typedef struct {
   int *arcAlignOff;
   int *alState, *alModel, *alDur;
   float *alLike;
} htkamd_lattice_align_out;
int  htkamd_decoder_run_lattice_align(htkamd_decoder *d, const htkamd_decode_config *cfg, int nToks, float nBeam, int alignMode, const float *dX, const int *frameOff,
                                      int nUtt, int maxLatNodes, int maxLatArcs, int maxAlign, const htkamd_lattice_out *out, const htkamd_lattice_align_out *alOut,
                                      void *stream);
/* One utterance's lattice for the host-side functions below (pointers into the arrays above). */
typedef struct {
   int nNodes, nArcs;
   const int *nodeFrame, *nodePron;
   const double *nodeLike;
   const int *arcStart, *arcEnd;
   const float *arcAc, *arcLm, *arcPr;
   float lmScale, wordPen, prScale;     /* of the recognition run (header fields, LArcTotLike) */
   double frameDur;                     /* seconds per frame */
} htkamd_lattice;
/* WriteLattice (HNet.c:631): the SLF text file, byte for byte the reference's for the supported fields.  format = HVite -q letters as
 * bits; 0 = HTKAMD_LAT_DEFAULT (t v a l).  utterance / lmName / vocabName: header lines (NULL = left out).  Without an lmName -- a lattice
 * made in DoAlignment, a network per file -- the lmscale / wdpenalty line is left out too and l= holds lmlike * lmScale + wordPen to two
 * decimals, as WriteLattice writes a lattice that has no network (HNet.c:609-615). */
#define HTKAMD_LAT_ALABS  0x0001
#define HTKAMD_LAT_LBIN   0x0002
#define HTKAMD_LAT_TIMES  0x0008
#define HTKAMD_LAT_PRON   0x0010
#define HTKAMD_LAT_ACLIKE 0x0020
#define HTKAMD_LAT_LMLIKE 0x0040
#define HTKAMD_LAT_ALIGN  0x0080
#define HTKAMD_LAT_PRLIKE 0x0400
#define HTKAMD_LAT_DEFAULT (HTKAMD_LAT_TIMES | HTKAMD_LAT_PRON | HTKAMD_LAT_ACLIKE | HTKAMD_LAT_LMLIKE)
int  htkamd_lattice_write(const htkamd_lattice *lat, const htkamd_net *net, const char *path, const char *utterance, const char *lmName,
                          const char *vocabName, int format);
/* ... with the arcs' alignment records (htkamd_decoder_run_lattice_align) as WriteLattice's OutputAlign writes them (HNet.c:503-516):
 * `d=:label[,duration][,likelihood]: ...` per arc that has records -- label = the physical model's name for a model record, "s<j>" for a
 * state record when model records were made too (models != 0), "<model>[<j>]" otherwise; format bits HTKAMD_LAT_ALIGN / _ALDUR / _ALLIKE
 * (HVite's default -q is all of t v a l d with durations and likelihoods: HTKAMD_LAT_DEFAULT_ALIGN). */
typedef struct {
   const int *arcAlignOff;              /* [nArcs + 1] */
   const int *alState, *alModel, *alDur;
   const float *alLike;
   int models;
} htkamd_lattice_align;
#define HTKAMD_LAT_ALDUR  0x0100
#define HTKAMD_LAT_ALLIKE 0x0200
#define HTKAMD_LAT_DEFAULT_ALIGN 0x03f8
int  htkamd_lattice_write_align(const htkamd_lattice *lat, const htkamd_lattice_align *al, const htkamd_mmf *hmms, const htkamd_net *net, const char *path,
                                const char *utterance, const char *lmName, const char *vocabName, int format);
/* TranscriptionFromLattice's label list for ONE alternative (arcs from htkamd_lattice_nbest) whose arcs carry alignment records
 * (HRec.c:2284-2338): model labels (-m), state labels (-f; with -m too the model rides as their first auxiliary label), the word as the last
 * auxiliary label of an arc's first label.  *out = NULL when an arc of the alternative has no records (word labels are then the caller's). */
int  htkamd_lattice_align_trans(const htkamd_lattice *lat, const htkamd_lattice_align *al, const htkamd_mmf *hmms, const htkamd_net *net,
                                const int *arcs, int nArcs, htkamd_trans **out);
/* TranscriptionFromLattice (HRec.c:2176) with N > 1: the N most likely paths with distinct word sequences, best first.  Alternative i has
 * altLen[i] arcs altArcs[i*maxLen + 0..], start to end, the closing arc into the end node left out. */
int  htkamd_lattice_nbest(const htkamd_lattice *lat, const htkamd_net *net, int N, int maxLen, int *nAlt, int *altLen, int *altArcs);
float htkamd_lattice_arc_score(const htkamd_lattice *lat, int arc);      /* LArcTotLike (HNet.h:257): the score a label of that word carries */
int  htkamd_net_pron_num(const htkamd_net *n, int pron);                  /* v= : number of the pronunciation within its word, from 1 */
void htkamd_decoder_destroy(htkamd_decoder *d);
/* The order in which equally likely tokens reach a node.  SetEntryState (HRec.c:1303) keeps the FIRST of two tokens of exactly equal
 * likelihood, and "first" is a matter of HRec's instance list, which AttachInst / MoveToRecent / ReOrderList / DetachInst
 * (HRec.c:1123-1301) re-order as the utterance goes.  The batch kernel pulls in a static order and NOTES when two such tokens with
 * different histories meet; HTKAMD_ORDER_AUTO (default) then decodes that utterance again with the list itself kept and walked on the
 * device (exact: HVite's choice among homophones of equal score, at a fraction of the batch kernel's speed); _FAST keeps the static
 * order's answer (same likelihoods, possibly the other of two equally scored words); _EXACT sends every utterance through the list
 * kernel.  The environment variable HTKAMD_DECODE_ORDER = auto | fast | exact overrides.  decoder_last_tied: how many utterances of the
 * last htkamd_decoder_run took the list kernel.  N-best runs (htkamd_decoder_run_lattice) always use the list. */
#define HTKAMD_ORDER_AUTO  0
#define HTKAMD_ORDER_FAST  1
#define HTKAMD_ORDER_EXACT 2
int  htkamd_decoder_set_order(htkamd_decoder *d, int mode);
int  htkamd_decoder_last_tied(const htkamd_decoder *d);
/* Device time of the last htkamd_decoder_run: the scoring kernels (K1 + the score block's transposition) and the token kernel(s), milliseconds. */
int  htkamd_decoder_last_times(const htkamd_decoder *d, double *scoreMs, double *tokenMs);
/* Model-instance steps of the last htkamd_decoder_run's token kernel (the register-resident models of the network): out[0] with a live
 * token (StepHMM1 ran: HRec.c:642), out[1] with none (the instance would not be in HRec's list: DetachInst HRec.c:1330).  out[0] 3 states
 * is what demand-driven scoring (HRec.c:438-551) would evaluate against the dense block's tied states x frames. */
int  htkamd_decoder_last_live(const htkamd_decoder *d, long long out[2]);
int  htkamd_decoder_run(htkamd_decoder *d, const htkamd_decode_config *cfg, const float *dX, const int *frameOff, int nUtt,
                        int maxWords, int *nWords, int *wordPron, int *wordStart, int *wordEnd, float *wordScore, float *wordLm,
                        double *total, void *stream);

/* The same with every per-word quantity of the 1-best path that CompleteRecognition's lattice carries (LatFromPaths HRec.c:1512):
   wordAc = LArc.aclike (acoustic log likelihood of the word's segment, float), wordLike = Path.like (the token's likelihood at the
   word end, double).  Any of wordLm / wordAc / wordLike may be NULL. */
typedef struct {
   int *nWords, *wordPron, *wordStart, *wordEnd;
   float *wordScore, *wordLm, *wordAc;
   double *wordLike, *total;
   float *finalLm;             /* [nUtt] LM log probability the final token collected after the last word end (may be NULL) */
} htkamd_decode_out;
int  htkamd_decoder_run_out(htkamd_decoder *d, const htkamd_decode_config *cfg, const float *dX, const int *frameOff, int nUtt,
                            int maxWords, const htkamd_decode_out *out, void *stream);

/* A batch in which every utterance has a network of its own -- DoAlignment (HVite.c:830): HVite -a from word-level transcriptions
 * (htkamd_net_build_words per file) and HVite -w without a network name, a lattice per file (-L dir -X ext; htkamd_net_build_ex per file).
 * The set holds the tables of nNets networks over one model set in one device allocation; htkamd_decoder_set_run decodes utterance u
 * against nets[netOf[u]] (0 .. nNets-1, repeats allowed) in ONE launch of a token kernel that reads its network from the utterance's
 * descriptor.  Outputs, status codes and every number are those of htkamd_decoder_run_out on a decoder created for nets[netOf[u]]
 * alone, bit for bit; wordPron[u] indexes THAT network's pronunciations.  The limits are the single decoder's (models of up to 8 states,
 * tee models with at most 95 predecessors: the same messages from htkamd_decoder_set_create).  cfg->maxActive (HVite -u) is carried
 * through.  A netOf[u] out of range is refused before anything is launched.  Exact ties go through the list kernel as in the single
 * decoder (htkamd_decoder_set_order's modes; HTKAMD_DECODE_ORDER overrides), a launch per network that has such utterances.
 * The descriptors may be freed after htkamd_decoder_set_create.
 * N-best token sets and lattices (HVite -n i [N] [-z ext] together with -a or a lattice per file): htkamd_decoder_set_run_lattice and
 * _align are htkamd_decoder_run_lattice and _align with utterance u over nets[netOf[u]] -- the same arguments, outputs and status codes
 * (nNodes[u] = -1: no token reached the final node; a lattice that does not fit: the single decoder's code), every number that of a
 * decoder created for nets[netOf[u]] alone, bit for bit in list order; nodeNet / nodePron index THAT network.  One launch per chunk serves
 * every network in it.  Order modes: the list kernel unless HTKAMD_ORDER_FAST, which _align refuses; htkamd_decoder_set_last_tied
 * counts the utterances that went through the list kernel.  nToks outside 2..8 and a netOf[u] out of range are HTKAMD_EINVAL before a
 * device is needed; nUtt = 0 is HTKAMD_OK. */
typedef struct htkamd_decoder_set htkamd_decoder_set;
int  htkamd_decoder_set_create(htkamd_model *m, const htkamd_net_desc *const *nets, int nNets, float lmScale, htkamd_decoder_set **out);
void htkamd_decoder_set_destroy(htkamd_decoder_set *d);
int  htkamd_decoder_set_run(htkamd_decoder_set *d, const htkamd_decode_config *cfg, const float *dX, const int *frameOff,
                            const int *netOf /*[nUtt], 0..nNets-1, repeats allowed*/, int nUtt, int maxWords,
                            const htkamd_decode_out *out, void *stream);
int  htkamd_decoder_set_run_lattice(htkamd_decoder_set *d, const htkamd_decode_config *cfg, int nToks, float nBeam, const float *dX, const int *frameOff,
                                    const int *netOf, int nUtt, int maxLatNodes, int maxLatArcs, const htkamd_lattice_out *out, void *stream);
int  htkamd_decoder_set_run_lattice_align(htkamd_decoder_set *d, const htkamd_decode_config *cfg, int nToks, float nBeam, int alignMode, const float *dX,
                                          const int *frameOff, const int *netOf, int nUtt, int maxLatNodes, int maxLatArcs, int maxAlign,
                                          const htkamd_lattice_out *out, const htkamd_lattice_align_out *alOut, void *stream);
int  htkamd_decoder_set_last_tied(const htkamd_decoder_set *d);
int  htkamd_decoder_set_set_order(htkamd_decoder_set *d, int mode);      /* HTKAMD_ORDER_* */

/* ------------------------------------------------------------------------------------------
 * Waveform -> MFCC(+_0/_E)(+_D)(+_A)(+_Z) on the device: replaces what OpenBuffer (HParm.h, HParm.c:4357)
 * does for a waveform source with maxObs == 0 (whole file converted into a table):
 *   GetWave HWave.c:1683 frame slicing; ConvertFrame HParm.c:2214 = PreEmphasise HSigP.c:134, Ham :122,
 *   Wave2FBank :558 (Realft :362 / FFT :311, mel binning, log), FBank2MFCC :607, FBank2C0 :647,
 *   WeightCepstrum :773, raw log energy; NormaliseLogEnergy :911; AddQualifiers HParm.c:1618 =
 *   AddRegression HSigP.c:860 for deltas/accelerations, FZeroMean :803 for _Z.
 * Configuration names follow the HParm config variables (HParm.c:258-367).
 * Output rows have the reference's column order: c1..cN [c0] [E] [deltas] [accs]; the output buffer is a
 * feature matrix that htkamd_outp_block / htkamd_fb_* / htkamd_viterbi_* take as dX.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
   double sampPeriod;          /* SOURCERATE (100 ns units; 625 = 16 kHz)                 */
   double winDur, frPeriod;    /* WINDOWSIZE, TARGETRATE (100 ns units)                    */
   int    numChans, numCeps, cepLifter;                        /* NUMCHANS NUMCEPS CEPLIFTER */
   float  preEmph;                                             /* PREEMCOEF                 */
   int    useHam, usePower, zMeanSource, rawEnergy, eNormalise;/* USEHAMMING USEPOWER ZMEANSOURCE RAWENERGY ENORMALISE */
   float  loFreq, hiFreq, cepScale, silFloor, eScale;          /* LOFREQ HIFREQ (<0 off) CEPSCALE SILFLOOR ESCALE */
   int    hasC0, hasE, hasD, hasA, hasZ;                       /* qualifiers of TARGETKIND   */
   int    delWin, accWin;                                      /* DELTAWINDOW ACCWINDOW      */
} htkamd_mfcc_config;

typedef struct htkamd_mfcc htkamd_mfcc;
int  htkamd_mfcc_create(const htkamd_mfcc_config *cfg, htkamd_mfcc **out);
void htkamd_mfcc_destroy(htkamd_mfcc *f);
int  htkamd_mfcc_num_frames(const htkamd_mfcc_config *cfg, int nSamples);     /* FramesInWave HWave.c:1663 */
int  htkamd_mfcc_num_cols(const htkamd_mfcc_config *cfg);
/* dWav: device int16 samples of nUtt waveforms back to back; sampOff host [nUtt+1]; frameOff host OUT [nUtt+1];
   dOut: device float [frameOff[nUtt] * cols].  Asynchronous on `stream` except for the table upload of the first call. */
/* AddQualifiers (HParm.c:1618 -> AddDiffs :1552 -> Regress HSigP.c:827) on an already parameterised table, e.g. MFCC_E
   files read with TARGETKIND = MFCC_E_D (HTKDemo/toolconfs/herest.conf): dStatic [F x nStat] -> dOut [F x nStat*(1+D+A)],
   regression windows per utterance (frameOff host [nUtt+1]). */
int  htkamd_parm_add_qualifiers(const float *dStatic, const int *frameOff, int nUtt, int nStat, int hasD, int hasA,
                                int delWin, int accWin, float *dOut, void *stream);
/* The whole qualifier step of AddQualifiers for a table: _D _A _T (third differentials = regression of the accelerations over
   THIRDWINDOW, HParm.c:1675-1681), then _Z (FZeroMean over the first nZeroMean columns per utterance, HParm.c:1700-1726: the base
   coefficients, plus C0 when the kind has _0 and not _N), and _N (the row is handed out without its absolute energy / C0 column
   `nullECol`, ExtractObservation HParm.c:2882-2893; needs _D).  dOut: [F x htkamd_parm_quals_cols(q)]. */
typedef struct {
   int nStat;                       /* static columns incl. C0 / energy                        */
   int nZeroMean;                   /* _Z: leading columns to zero-mean (0 = no _Z)            */
   int hasD, hasA, hasT;            /* _D _A _T                                                */
   int delWin, accWin, thirdWin;    /* DELTAWINDOW ACCWINDOW THIRDWINDOW                       */
   int nullECol;                    /* _N: column left out of every row (-1 = none)            */
   int v1Compat, simpleDiffs;       /* V1COMPAT (edge rows = plain differences), SIMPLEDIFFS    */
} htkamd_parm_quals;
int  htkamd_parm_quals_cols(const htkamd_parm_quals *q);
int  htkamd_parm_qualify(const float *dStatic, const int *frameOff, int nUtt, const htkamd_parm_quals *q, float *dOut, void *stream);
/* The same qualifiers in HParm's BUFFER mode (OpenBuffer / ReadAsBuffer, HParm.c:4000-4116 FillBufFromChannel; HVite.c:664 opens its
   input this way): static rows arrive in pushes, an observation is handed out as soon as the qwin = DELTAWINDOW + ACCWINDOW
   (+ THIRDWINDOW) rows of look-ahead its regression windows need have arrived; the last push (last = 1) flushes the remaining rows
   with the end-of-utterance replication.  The rows handed out are bit-identical to htkamd_parm_qualify over the whole utterance.
   _Z is refused (it needs the whole utterance: table mode), as HParm refuses ENORMALISE on a live buffer (HParm.c:4096).
     open : maxRows = the largest push;   push : dStatic [nRows x nStat] on the device, dOut receives *nOut <= nRows + qwin rows. */
typedef struct htkamd_parm_stream htkamd_parm_stream;
int  htkamd_parm_stream_open(const htkamd_parm_quals *q, int maxRows, htkamd_parm_stream **out);
int  htkamd_parm_stream_push(htkamd_parm_stream *s, const float *dStatic, int nRows, int last, float *dOut, int *nOut, void *stream);
int  htkamd_parm_stream_lookahead(const htkamd_parm_stream *s);
void htkamd_parm_stream_close(htkamd_parm_stream *s);
/* HCompV's global statistics over a device table of frames: replaces AccVar / CalcCovs (HTKTools/HCompV.c:392-411, :261-291) --
   mean and diagonal variance of all frames, variance floored at minVar (HCompV -v, default 0).  The reference sums in float in
   file order; this sums in fp64 (order-free), so the results agree to the reference's own rounding (~1e-6 relative at a few
   thousand frames, growing with the frame count on the reference's side).  Flat start = every Gaussian's mean/variance set to
   these (HCompV -m), the variance floor macro = f * var (HCompV -f f, htkamd_mmf_write_vfloors). */
int  htkamd_compv(const float *dX, long long nFrames, int D, float minVar, float *mean /*[D]*/, float *var /*[D]*/, void *stream);
int  htkamd_mfcc_compute(htkamd_mfcc *f, const short *dWav, const int *sampOff, int nUtt, int *frameOff, float *dOut, void *stream);

/* ------------------------------------------------------------------------------------------
 * Waveform -> MFCC, FBANK, MELSPEC or PLP (+_0/_E)(+_D)(+_A)(+_Z) on the device: the FFT front ends of ConvertFrame
 * (HParm.c:2214).  The window, FFT and mel bins are the MFCC path's; after the bins
 *   FBANK   : log with floor 1.0 (Wave2FBank HSigP.c:598-603), the numChans bins are the statics;
 *   MELSPEC : the linear bins (InitFBank with takeLogs = FALSE);
 *   PLP     : FBank2ASpec :693 (equal-loudness curve, cube-root compression), MatrixIDFT :710, Durbin :167,
 *             LPC2Cepstrum :262, C0 = the LPC gain (ASpec2LPCep :735), WeightCepstrum, CEPSCALE.
 * Columns: c1..cN (or the N bins) [C0] [E] [deltas] [accs].  baseKind = 6 gives the bits htkamd_mfcc_compute gives.
 * Refused (HTKAMD_EINVAL and the reason, before any device is touched): base kinds other than 6 / 7 / 8 / 11 (the LPC kinds among
 * them), _0 on FBANK / MELSPEC, and for PLP lpcOrder outside 2..1000, numCeps outside 2..lpcOrder or compressFact outside (0, 1)
 * (ValidCodeParms HParm.c:1317).  Argument conventions of create / num_frames / compute are those of htkamd_mfcc_*.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
   htkamd_mfcc_config base;    /* every HParm variable the MFCC path has; hasC0 / hasE / hasD / hasA / hasZ as there */
   int   baseKind;             /* HTK base code of TARGETKIND: 6 MFCC, 7 FBANK, 8 MELSPEC, 11 PLP */
   int   lpcOrder;             /* LPCORDER (12) */
   float compressFact;         /* COMPRESSFACT (0.33) */
} htkamd_frontend_config;
typedef struct htkamd_frontend htkamd_frontend;
int  htkamd_frontend_create(const htkamd_frontend_config *cfg, htkamd_frontend **out);
void htkamd_frontend_destroy(htkamd_frontend *f);
int  htkamd_frontend_num_frames(const htkamd_frontend_config *cfg, int nSamples);
int  htkamd_frontend_num_cols(const htkamd_frontend_config *cfg);      /* < 0 and the error string set on a refused config */
int  htkamd_frontend_compute(htkamd_frontend *f, const short *dWav, const int *sampOff, int nUtt, int *frameOff, float *dOut, void *stream);

/* ------------------------------------------------------------------------------------------
 * Vocal-tract-length normalisation (VTLN): the mel filterbank's frequency axis warped per speaker, HParm's WARPFREQ, WARPLCUTOFF and
 * WARPUCUTOFF (HParm.c:249-251; InitFBank HSigP.c:513-526 warps the filters' centres through WarpFreq :449-468).  A front end is
 * created with 1..64 warps; the window, FFT and magnitudes are the un-warped ones, the filter weights (and PLP's equal-loudness
 * curve, taken at the warped centres) are one table set per warp.
 *   htkamd_frontend_compute_warped : utterance u is coded with warps[uttWarp[u]] (uttWarp NULL: all with warps[0]); an entry outside
 *                                    0..nWarp-1 is HTKAMD_EINVAL.  htkamd_frontend_compute on such a handle codes with warps[0].
 *   htkamd_frontend_compute_grid   : every utterance under every warp, each frame transformed once and binned nWarp times: dOut holds
 *                                    nWarp tables of [F x nCols], table w at dOut + w*F*nCols, each bit-equal to what
 *                                    htkamd_frontend_compute_warped gives with every utterance on warp w (the grid search of VTLN
 *                                    warp estimation; frameOff [nUtt+1] describes every table).
 * warpFreq 1.0 is the un-warped front end whatever the cut-offs.  Refused (HTKAMD_EINVAL and the reason, before any device is
 * touched): nWarp outside 1..64; warpFreq outside 0.5..2.0; for warpFreq != 1 a cut-off equal to 0 or warpLCutoff > warpUCutoff
 * (ValidCodeParms HParm.c:1366-1372); and what the reference leaves unchecked but what makes WarpFreq divide by zero or stop
 * increasing: with scale = 1/warpFreq and the corners cl, cu = cut-off * 2 / (1 + scale), cl <= minFreq, cu >= maxFreq,
 * scale*cu >= maxFreq or scale*cl <= minFreq (minFreq, maxFreq: the band's ends, LOFREQ / HIFREQ or 0 / half the sample rate).
 * ------------------------------------------------------------------------------------------ */
typedef struct { float warpFreq, warpLCutoff, warpUCutoff; } htkamd_warp;      /* WARPFREQ WARPLCUTOFF WARPUCUTOFF */
int  htkamd_frontend_create_warped(const htkamd_frontend_config *cfg, const htkamd_warp *warps, int nWarp /*1..64*/, htkamd_frontend **out);
int  htkamd_frontend_num_warps(const htkamd_frontend *f);      /* 1 for a handle made by htkamd_frontend_create */
int  htkamd_warp_check(const htkamd_warp *w);                  /* ValidCodeParms' checks alone (no configuration, no device): 0, or HTKAMD_EINVAL and the reason */
int  htkamd_frontend_compute_warped(htkamd_frontend *f, const short *dWav, const int *sampOff, int nUtt, const int *uttWarp,
                                    int *frameOff, float *dOut, void *stream);
int  htkamd_frontend_compute_grid(htkamd_frontend *f, const short *dWav, const int *sampOff, int nUtt,
                                  int *frameOff, float *dOut, void *stream);

/* ------------------------------------------------------------------------------------------
 * Side-based cepstral mean and variance normalisation: HParm's CMEANDIR / CMEANMASK / CMEANPATHMASK and VARSCALEDIR / VARSCALEMASK /
 * VARSCALEPATHMASK / VARSCALEFN (HParm.c:859-866), and what `HCompV -c dir -k mask [-p mask] -q nmv` estimates (HCompV.c:520-740).
 * A "side" is a speaker or conversation side: the characters a mask's % capture from a file's name.  The host functions look for no
 * device; every refusal is HTKAMD_EINVAL (HTKAMD_EIO: a file that cannot be opened or written) with the reason in htkamd_last_error.
 *
 *   htkamd_mask_match          the behaviour of MaskMatch (HShell.c:1851): % captures one character, ? matches one, * any run.  Returns 1 and the
 *                              captured characters in out, 0 (out empty) when the name does not match, HTKAMD_EINVAL when the mask
 *                              captures outLen characters or more.
 *   htkamd_parm_kind_parse     Str2ParmKind (HParm.c:1109): "MFCC_E_D_A" -> base code + qualifier bits; -1 for an unknown name.
 *   htkamd_parm_kind_str       ParmKind2Str (HParm.c:1092), qualifiers in the reference's order.
 *   htkamd_cepsnorm_read       a `<CEPSNORM> <KIND>` side file as LoadCMeanVector / LoadVarScaleVector read it (HParm.c:3172-3349): skips to
 *                              `<MEAN> n` / `<VARIANCE> n` and reads n floats into mean / var (each may be NULL: not wanted; at most
 *                              maxDim values each).  *dimMean / *dimVar = 0 for a vector the file does not hold, *nFrames = -1 without
 *                              <NFRAMES>.
 *   htkamd_cepsnorm_write      ExportNMV (HCompV.c:686-740): " %e" per value; flags = HCompV's -q subsets "m" "v" "mv" "nv" "nmv".
 *   htkamd_varscale_read       the global `<VARSCALE> n ...` file of VARSCALEFN (LoadVarScale HParm.c:560-615).
 *   htkamd_cepsnorm_check_kinds  a mean file's kind equals the target kind once the target's _D _A _T _Z _V bits are masked out of both
 *                              (HParm.c:3221-3224); a variance file's kind equals the target kind, or lacks only its _V (:3298).
 *                              meanKind / varKind -1: no such file.
 *   htkamd_cepsnorm_scale      scale[side][i] = (float)sqrt(varScale[i] / sideVar[side][i]): a float quotient, the double sqrt, stored as
 *                              a float (HParm.c:1624, :1806).  dScale != dVar is refused (:1797-1800), and so is a side variance that is
 *                              not positive, with the side's name (sideNames may be NULL: its index).
 *   htkamd_side_stats_finish   UpdateMeanVar (HCompV.c:640-656) from the fp64 sums: mean = sum/N, var = sqsum/N - mean^2, formed in fp64
 *                              and rounded once; a side without frames keeps zeros.
 *
 * On the device (csrc/cepsnorm.hip; HTKAMD_ENODEV without one, after the arguments were checked):
 *   htkamd_side_stats          AccGenUtt / UpdateSpkrAccList (HCompV.c:520-636): per side and column the sum, the sum of squares and the
 *                              frame count over the first D columns of the table dX [frameOff[nUtt] x nCols]; utterance u belongs to
 *                              side uttSide[u].  frameOff, uttSide and the results are host arrays (sum, sqsum: [nSide x D]).  The
 *                              reference sums floats in file order; this sums in fp64 in a fixed order (per-utterance partial sums,
 *                              then the utterances of a side in utterance order, no atomics): the same bits on every call.
 *   htkamd_parm_normalise      the tail of AddQualifiers, in place: row - mean[side] over the first dMean columns (HParm.c:1728-1741), then
 *                              row * scale[side] over the first dScale columns (:1804-1812): two separately rounded float operations.
 *                              mean [nSide x dMean] and scale [nSide x dScale] are host tables; either may be NULL.
 *   An uttSide entry outside 0..nSide-1 is HTKAMD_EINVAL before anything is launched.
 * Order of calls for TARGETKIND = <kind>_Z with side means: htkamd_parm_qualify with nZeroMean = 0 (the reference skips FZeroMean when
 * it has a side mean, HParm.c:1709-1741), then htkamd_parm_normalise.  Without _Z in the target the mean is not applied at all
 * (HParm.c:4375); variance scaling needs no _Z.  With _N in the target the reference applies the side vectors while the energy column
 * is still in the row (it leaves when an observation is extracted, HParm.c:2882): a caller with _N normalises a table qualified without
 * nullECol and drops the column itself; the command-line drivers refuse _N together with side normalisation.
 * Not served: side transforms (SIDEXFORMMASK, sideXForm), USEOLDXFORMCVN, HIGHDIFF, side normalisation together with an input
 * transform (below), and buffer mode (htkamd_parm_stream_* keeps refusing _Z).
 * ------------------------------------------------------------------------------------------ */
int  htkamd_mask_match(const char *mask, const char *name, char *out, int outLen);
int  htkamd_parm_kind_parse(const char *str);
int  htkamd_parm_kind_str(int kind, char *buf, int bufLen);
int  htkamd_cepsnorm_read(const char *path, int *kind, int *nFrames, float *mean, int *dimMean, float *var, int *dimVar, int maxDim);
int  htkamd_cepsnorm_write(const char *path, int kind, const char *flags, int nFrames, const float *mean, const float *var, int dim);
int  htkamd_varscale_read(const char *path, float *v, int *dim, int maxDim);
int  htkamd_cepsnorm_check_kinds(int targetKind, int meanKind, int varKind);
int  htkamd_cepsnorm_scale(const float *varScale, int dScale, const float *sideVar /*[nSide x dVar]*/, int dVar, int nSide,
                           const char *const *sideNames, float *scale /*[nSide x dVar]*/);
int  htkamd_side_stats_finish(const double *sum, const double *sqsum, const long long *nFrames, int nSide, int D, float *mean, float *var);
int  htkamd_side_stats(const float *dX, const int *frameOff /*[nUtt+1]*/, const int *uttSide /*[nUtt]*/, int nUtt, int nSide, int nCols, int D,
                       double *sum /*[nSide x D]*/, double *sqsum, long long *nFrames /*[nSide]*/, void *stream);
int  htkamd_parm_normalise(float *dX, const int *frameOff, const int *uttSide, int nUtt, int nSide, int nCols,
                           const float *mean, int dMean, const float *scale, int dScale, void *stream);

/* ------------------------------------------------------------------------------------------
 * Global linear input transforms (HLDA and other projections): <INPUTXFORM> of a model set's global options -- the body inline, or
 * ~j "name", a ~j macro of the loaded files or else a file of that name (looked for as given, then beside the file that names it) --,
 * ~j macro definitions in a model file, and transform files of their own (what HParm's MATTRANFN names).  Reader and writer restate
 * GetInputXForm / GetLinXForm / LoadInputXForm and PutInputXForm / PutLinXForm / SaveInputXForm (HModel.c:2373, :2195, :4640, :3177,
 * :3116, :4839), text and binary.  The body:
 *   <MMFIDMASK> mask <kind> [<PREQUAL>] <LINXFORM> <VECSIZE> n [<OFFSET> <BIAS> n ..] [<LOGDET> x] <BLOCKINFO> 1 b <BLOCK> 1 <XFORM> r c ..
 * An <OFFSET> bias and a <LOGDET> are carried and written back; applying the transform uses the matrix alone (ApplyStaticMat
 * HParm.c:1235).  More than one block is HTKAMD_EMODEL (SetInputXFormConfig HParm.c:631), and so are ~f ~x ~y references inside a
 * transform; <PARENTXFORM>, ~a ~b ~g ~f macros and side transforms stay refused.  htkamd_mmf_write* put the set's transform back
 * behind the global options, in full, as SaveHMMSet does for a transform read either way (PutOptions HModel.c:3257).
 *
 *   htkamd_mmf_inputxform        the set's transform, owned by the set, or NULL;   htkamd_mmf_set_id: <HMMSETID> ("" without);
 *                                htkamd_mmf_vec_size: <VECSIZE>.
 *   htkamd_inputxform_read       a transform file, with or without its ~j "name" header (without: known by the file's name); the handle
 *                                is released with htkamd_inputxform_free.   htkamd_inputxform_write: SaveInputXForm.
 *   htkamd_inputxform_name .. _logdet   macro name (an inline transform: the file it stood in), <MMFIDMASK>, parameter kind, <PREQUAL>,
 *                                matrix rows, columns and the row-major matrix [rows x cols]; <VECSIZE>, bias (NULL without), <LOGDET>.
 *   htkamd_inputxform_check      what the reference checks where it applies a transform, each with its own message (HTKAMD_EINVAL):
 *                                the transform's kind against the data's (base kind, _E and _0; with <PREQUAL> also _Z of the source
 *                                rows, HParm.c:1636-1647; without, the whole kind of the qualified rows, :1835); the matrix columns
 *                                against the width of the rows it meets (:1256); the set's <VECSIZE> (0: not checked) against what the
 *                                transform produces -- its rows, with <PREQUAL> rows x (1 + differentials present), :2199-2208 --; and
 *                                <MMFIDMASK> against <HMMSETID> (NULL or "": not checked, :691).  srcKind: kind of the rows the
 *                                qualifiers start from, nStat their width; kinds as htkamd_parm_kind_parse gives them.  _N is refused.
 * On the device (csrc/inputxform.hip; HTKAMD_ENODEV without one, after the arguments were checked):
 *   htkamd_parm_xform            row r of dOut holds, in its first mrows columns, M . dIn[r][0..mcols): each output starts at 0.0f, then
 *                                acc = acc + (M[j][m] * x[m]) for m = 0 .. mcols-1, product and sum each rounded to float (no fused
 *                                multiply-add, subnormals kept): the reference's bits.  Columns of dIn beyond mcols are ignored, columns
 *                                of dOut beyond mrows are left untouched.  dOut == dIn is allowed when inCols == outCols; otherwise the
 *                                tables must not overlap.  dMat [mrows x mcols] row-major on the device.  mrows or mcols above 128 is
 *                                refused with HTKAMD_EINVAL (there is no slower path).  Asynchronous on `stream`.
 *   htkamd_inputxform_apply      the whole qualifier step of a transformed set in the reference's order (AddQualifiers HParm.c:1636-1844,
 *                                USEOLDXFORMCVN unset), so that no caller re-derives it: dStatic [F x q->nStat] -> dOut
 *                                [F x htkamd_inputxform_apply_cols(x, q)].  q describes the qualifiers as for a set without a transform
 *                                (nZeroMean by the usual rule, HParm.c:1712-1715).  Without <PREQUAL>: htkamd_parm_qualify, then the
 *                                transform over the whole qualified row; the row becomes mrows wide.  With <PREQUAL>: the transform over
 *                                the statics, then htkamd_parm_qualify on mrows statics, and _Z (q->nZeroMean > 0) takes the mean off
 *                                every one of them (the reference's "do everything" rule, HParm.c:1716-1720).  q->nullECol >= 0 (_N) is
 *                                refused.  Synchronises `stream`.
 * Not served: side transforms (SIDEXFORMMASK), <PARENTXFORM>, USEOLDXFORMCVN, HIGHDIFF, an input transform together with side
 * normalisation (CMEAN* / VARSCALE*: the command-line drivers refuse that combination before they touch a device), and source rows that
 * already carry _D _A _T (the reference applies a transform without <PREQUAL> to files qualified beforehand, HParm.c:1633;
 * htkamd_inputxform_check refuses them: qualifiers are appended here, on the device, never found in the files).
 * ~j macros nobody names: a ~j macro of the loaded files that is not the set's <INPUTXFORM> is read and dropped by htkamd_mmf_write*, and
 * the set's own is written inline, not as a macro -- both as the reference does (SaveMacros HModel.c:4350 writes a ~j macro only when a
 * ~j reference inside a structure has counted it, and <INPUTXFORM> ~j "name" is no such reference, :647): HHEd's re-save of a set with a
 * used and an unused ~j macro holds neither definition (tests/golden/make_inputxform_golden.py).
 * ------------------------------------------------------------------------------------------ */
typedef struct htkamd_inputxform htkamd_inputxform;
const htkamd_inputxform *htkamd_mmf_inputxform(const htkamd_mmf *s);
const char *htkamd_mmf_set_id(const htkamd_mmf *s);
int  htkamd_mmf_vec_size(const htkamd_mmf *s);
int  htkamd_inputxform_read(const char *path, htkamd_inputxform **out);
int  htkamd_inputxform_write(const htkamd_inputxform *x, const char *path, int binary);
void htkamd_inputxform_free(htkamd_inputxform *x);
const char *htkamd_inputxform_name(const htkamd_inputxform *x);
const char *htkamd_inputxform_mask(const htkamd_inputxform *x);
const char *htkamd_inputxform_parm_kind(const htkamd_inputxform *x);
int  htkamd_inputxform_prequal(const htkamd_inputxform *x);
int  htkamd_inputxform_rows(const htkamd_inputxform *x);
int  htkamd_inputxform_cols(const htkamd_inputxform *x);
const float *htkamd_inputxform_matrix(const htkamd_inputxform *x);
int  htkamd_inputxform_vec_size(const htkamd_inputxform *x);
const float *htkamd_inputxform_bias(const htkamd_inputxform *x, int *n);
float htkamd_inputxform_logdet(const htkamd_inputxform *x);
int  htkamd_inputxform_check(const htkamd_inputxform *x, int srcKind, int targetKind, int nStat, const char *setId, int vecSize);
int  htkamd_parm_xform(const float *dIn, int inCols, float *dOut, int outCols, long long nRows,
                       const float *dMat /* [mrows x mcols], row-major, device */, int mrows, int mcols, void *stream);
int  htkamd_inputxform_apply_cols(const htkamd_inputxform *x, const htkamd_parm_quals *q);
int  htkamd_inputxform_apply(const htkamd_inputxform *x, const float *dStatic, const int *frameOff, int nUtt,
                             const htkamd_parm_quals *q, float *dOut, void *stream);

/* ------------------------------------------------------------------------------------------
 * Viterbi training from labelled tokens: replaces HInit (HTKTools/HInit.c) for every model of a list in ONE call, on one-stream
 * DIAGC continuous-density sets (csrc/hinit.hip; the checks and the host twin of the pool listing: host/hinit.c).
 *   EstimateModel (HInit.c:1192)   htkamd_hinit: per model the reference's loop, all models side by side
 *   UCollectData (:505)            pools of frames per (model, emitting state): count, scan, fill kernels; frame j (1-based) of a token
 *                                  of L frames goes to state (int)((float)(j-1) / ((float)L / (float)(N-2)) + 2), the sum in float
 *   FlatCluster (HTrain.c:763)     one workgroup per pool (htkamd_flat_cluster is that launch on its own): Euclidean distance, diagonal
 *                                  cluster covariances; BiggestCluster / Perturb / AllocateVectors / FullestCluster / FindCentres /
 *                                  FindCovariance in the reference's float / double mix and item order, so sizes, centres and
 *                                  variances are the reference's bits
 *   ViterbiAlign (:792)            htkamd_viterbi_align_mode(HTKAMD_SCORE_SOUTP | HTKAMD_SCORE_DIAGC), one single-model utterance per
 *                                  token, every token of the models still running in one call per pass
 *   FindBestMixes (:739)           a lane per frame: MOutP of every component in DOutP's form, the first maximum
 *   UpdateCounts (:878)            a wavefront per (token, state): counts and fp64 sums of x - mean and its square (atomic adds: the
 *                                  order of the sums is not fixed), transition counts along the state sequence
 *   UpWeights / UpMeans / UpVars / UpTrans (:997-1097)   a workgroup per model; only what uFlags selects is written, then 1/variance,
 *                                  gConst, log weights and the scoring rows of the model's Gaussians are rebuilt in place
 * The host reads one (log probability sum, status) pair per running model per pass and decides convergence as the reference does:
 * newP = sum / tokens in float, |newP - totalP| < epsilon from the second pass on.
 * Tokens: tokFrame / tokLen / tokModel [nTokens] on the host -- first row in dX, frames, physical model --, in the reference's order
 * within each model (file order, then label order; FlatCluster's float sums run in that order).  Tokens of models that are not in
 * `models` are ignored.
 * Per model: status[k] (HTKAMD_HINIT_*; a model with a status other than OK keeps the parameters it had), nPass[k], converged[k] and
 * logP[k * maxIter + pass] ("Iteration k: Average LogP").  Every other model is trained exactly as if it had been called alone.
 * Refused before a device is touched (HTKAMD_EMODEL / HTKAMD_EINVAL and the reason; htkamd_hinit_check is these checks on a set's
 * description): FULLC, tied-mixture and multi-stream sets; sets with ~u / ~v sharing; models to be trained that use a state, a Gaussian
 * or a transition matrix twice, among or within them (HInit trains in isolation: shared structure would make the result depend on the
 * order); a model named twice or out of range; a token outside the table or of an unknown model; maxIter < 1, minSeg < 1.
 * mixWeightFloor is carried for the reference's -w; UpWeights (HInit.c:997) applies it to discrete sets only, so no continuous weight
 * is ever floored.  On return the device arrays hold the estimates, the derived tables follow as after htkamd_model_update_device, and
 * the host mirror is current.  Synchronises `stream`.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
   int   maxIter;          /* -i, 20                                                               */
   float epsilon;          /* -e, 1.0e-4                                                           */
   float minVar;           /* -v, 1.0e-2                                                           */
   int   minSeg;           /* -m, 3                                                                */
   float mixWeightFloor;   /* -w f: MINMIX * f (carried, see above)                                */
   int   uFlags;           /* -u: HTKAMD_UPMEANS | _UPVARS | _UPTRANS | _UPMIXES                   */
   int   newModel;         /* 1 (default): uniform segmentation + FlatCluster first; 0: -n, skip it */
} htkamd_hinit_config;
#define HTKAMD_HINIT_OK         0
#define HTKAMD_HINIT_EFEWSEGS   2121   /* fewer than minSeg tokens                                              */
#define HTKAMD_HINIT_ESHORT     2122   /* a token with fewer frames than emitting states                        */
#define HTKAMD_HINIT_ENOMIX     2125   /* FindBestMixes: no best mix                                            */
#define HTKAMD_HINIT_ENOPATH    2126   /* ViterbiAlign: no path in a token                                      */
#define HTKAMD_HINIT_EZEROOCC   2127   /* a component nobody chose, or a state no token left                    */
#define HTKAMD_HINIT_ECLUSTER   7120   /* a pool with fewer items than components, or one FlatCluster cannot split */
int htkamd_hinit_check(const htkamd_model_desc *d, int nFrames, int nTokens, const int *tokFrame, const int *tokLen, const int *tokModel,
                       const htkamd_hinit_config *cfg, int nModels, const int *models);
int htkamd_hinit(htkamd_model *m, const float *dX, int nFrames, int nTokens, const int *tokFrame, const int *tokLen, const int *tokModel,
                 const htkamd_hinit_config *cfg, int nModels, const int *models,
                 int *status /*[nModels]*/, int *nPass /*[nModels]*/, int *converged /*[nModels]*/, float *logP /*[nModels * maxIter]*/, void *stream);
/* The pool listing of UCollectData on the host, as the kernels make it (test aid): for tokens of ONE model with nEmit emitting states,
   state[k] = 0-based emitting state of the k-th frame of the tokens behind one another; returns 0, or HTKAMD_EINVAL for a token shorter
   than nEmit. */
int htkamd_hinit_uniform_states(int nEmit, int nTokens, const int *tokLen, int *state);
/* FlatCluster (HTrain.c:763, NULLC distance, DIAGC cluster covariances) over nPools pools in one launch.  dX [nRows x D] on the device;
   pool p owns items[poolOff[p] .. poolOff[p+1]) (row numbers, host) and is split into nc[p] clusters, which lie behind one another:
   cluster c of pool p is entry cOff[p] + c, cOff = prefix sum of nc.  Outputs (host): size [sum nc], centre and var [sum nc x D] (var
   floored at minVar), assign [items] = cluster of every item, status [nPools] = HTKAMD_HINIT_OK or HTKAMD_HINIT_ECLUSTER (that pool's
   other outputs are then undefined, the other pools unaffected).  HTKAMD_EINVAL: a row outside the table, nc < 1, sizes that do not fit
   the workgroup's LDS (nc x D floats). */
int htkamd_flat_cluster(const float *dX, int nRows, int D, int nPools, const int *poolOff, const int *items, const int *nc, float minVar,
                        int *size, float *centre, float *var, int *assign, int *status, void *stream);

/* ------------------------------------------------------------------------------------------
 * Isolated-unit Baum-Welch re-estimation: replaces HRest (HTKTools/HRest.c) for every model of a list in ONE call, on one-stream DIAGC
 * continuous-density sets (csrc/hrest.hip; the checks and the token bookkeeping: host/hrest.c).
 *   LoadFile (HRest.c:458)         tokens shorter than the model's emitting states are dropped once (segReject, :500), then the -m test
 *                                  (main :295) on what is left
 *   ReEstimateModel (:1309)        htkamd_hrest: per model the reference's loop, all models side by side.  A pass is ONE forward-backward
 *                                  batch (htkamd_fb_*, no beam, MINFORPROB out of the way, HTKAMD_SCORE_SOUTP | HTKAMD_SCORE_DIAGC: what
 *                                  OutP gives HRest) over every kept token of every model still running, one single-model utterance each;
 *                                  the running tokens are listed on the device (count, scan, fill) and their rows gathered
 *   ZeroAccs (HTrain.c)            once per pass, the running models' statistics only
 *   newP (:1328)                   a lane per running model: the float sum of its usable tokens' log probabilities in token order and
 *                                  their count ("Example skipped": a token whose alpha pass gives no more than LSMALL)
 *   UpdateTheModel (:1287)         a workgroup per running model: RestTransP (:1015), RestMixWeights (:1124), RestMean (:1165) and
 *                                  RestCoVar (:1185) of the components whose new weight exceeds MINMIX (floor first, then vDefunct),
 *                                  FloorMixes (:1043); only what uFlags selects is re-estimated; then 1/variance, gConst, log weights and
 *                                  the scoring rows of the model's Gaussians are rebuilt in place.  As in the reference the model is
 *                                  updated in every pass, the one that meets epsilon included
 * The host reads one (log probability sum, tokens used, status) triple per running model per pass and decides as the reference does:
 * newP = sum / used in float, delta = newP - oldP with oldP starting at LZERO, stop on |delta| < epsilon or after maxIter passes.  A model
 * that has stopped is frozen: later passes neither score its tokens nor touch its parameters.
 * Tokens as for htkamd_hinit.  Per model: status[k] (HTKAMD_HREST_*; a model with a status other than OK keeps exactly the parameters it
 * came with), nPass[k], converged[k], logP[k * maxIter + pass] ("Ave LogProb at iter") and nUsed[k * maxIter + pass] ("using N examples").
 * Every other model is trained as if it had been called alone.  A defunct component (the reference's warning -2225: a floored variance
 * below vDefunct in a state of several components) gets weight 0 and the model goes on.
 * Refused before a device is touched (HTKAMD_EMODEL / HTKAMD_EINVAL and the reason): FULLC, tied-mixture, multi-stream and discrete sets;
 * models to be trained that use a state, a Gaussian or a transition matrix twice, among or within them; a model named twice or out of
 * range; a token outside the table or of an unknown model; maxIter < 1, minSeg < 1 -- htkamd_hrest_check is exactly these checks on a
 * set's description.  A description does not say which mean / variance vectors are tied, so the refusal of ~u / ~v sharing
 * (htkamd_model_set_sharing) is htkamd_hrest's own, on the handle, also before the call looks for a device.  minVar is the floor of every
 * dimension (SetVFloor without a varFloor1 macro).
 * On return the device arrays hold the estimates, the derived tables follow as after htkamd_model_update_device, and the host mirror
 * is current.  Synchronises `stream`.  A call that ends in an error (a negative return: a failed allocation, a HIP error) puts every model
 * of the call back to the parameters it came with before it returns; status / nPass / converged / logP / nUsed are then undefined.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
   int   maxIter;          /* -i, 20                                                                               */
   float epsilon;          /* -e, 1.0e-4                                                                           */
   float minVar;           /* -v, 0.0                                                                              */
   int   minSeg;           /* -m, 3                                                                                */
   float mixWeightFloor;   /* -w f: MINMIX * f -- HRest DOES floor continuous weights (FloorMixes HRest.c:1043)    */
   int   uFlags;           /* -u: HTKAMD_UPMEANS | _UPVARS | _UPTRANS | _UPMIXES                                   */
   int   segReject;        /* 1 (default): drop tokens shorter than the model's emitting states; 0: -t             */
   float vDefunct;         /* HREST: VDEFUNCT, 0.0                                                                 */
} htkamd_hrest_config;
#define HTKAMD_HREST_OK         0
#define HTKAMD_HREST_EFEWSEGS   2221   /* fewer than minSeg tokens after the short ones were dropped            */
#define HTKAMD_HREST_EZEROOCC   2222   /* zero occupation of a state, a mean, a variance or a weight set        */
#define HTKAMD_HREST_EFLOORSUM  2223   /* FloorMixes: floor sum too large                                       */
#define HTKAMD_HREST_ENOUSABLE  2226   /* a pass in which no token was usable                                   */
int htkamd_hrest_check(const htkamd_model_desc *d, int nFrames, int nTokens, const int *tokFrame, const int *tokLen, const int *tokModel,
                       const htkamd_hrest_config *cfg, int nModels, const int *models);
int htkamd_hrest(htkamd_model *m, const float *dX, int nFrames, int nTokens, const int *tokFrame, const int *tokLen, const int *tokModel,
                 const htkamd_hrest_config *cfg, int nModels, const int *models,
                 int *status /*[nModels]*/, int *nPass /*[nModels]*/, int *converged /*[nModels]*/, float *logP /*[nModels * maxIter]*/,
                 int *nUsed /*[nModels * maxIter]*/, void *stream);
/* The token bookkeeping of LoadFile and main on the host, as the call does it (needs no device): hmmStateOff [numPhys + 1] as in
   htkamd_model_desc; keep[k] (may be NULL) = 1 for a token of a listed model that is not dropped, nKept[m] the kept tokens of
   models[m], status[m] = HTKAMD_HREST_EFEWSEGS where they are fewer than minSeg, else HTKAMD_HREST_OK. */
int htkamd_hrest_token_counts(const int *hmmStateOff, int numPhys, int nTokens, const int *tokLen, const int *tokModel, const htkamd_hrest_config *cfg,
                              int nModels, const int *models, int *keep /*[nTokens]*/, int *nKept /*[nModels]*/, int *status /*[nModels]*/);

/* ------------------------------------------------------------------------------------------
 * Scoring recognition output: replaces HResults (HTKTools/HResults.c) for K hypothesis sets x U utterances in ONE call
 * (csrc/results.hip; names, references, refusals and every line of text: host/results.c).
 *   AddEquiv / NormaliseName (:346)  htkamd_results_label_id: a label's name -> its id.  -s strips the contexts first (l-c+r -> c), then
 *                                    the -e equivalences in the reference's order (the last one given first), then -c upper-cases a name
 *                                    that has a lower-case letter.  Id 0 is the null class (-z, "???"); ids 1..nList are the label list's
 *                                    names as they stand (ReadHMMList :1121), later names follow in order of first use
 *   MatchFiles (:1720)               htkamd_results_ref_for: the reference of a hypothesis file (MakeFN with -L / -X, looked up in the
 *                                    -I files first); a missing reference is HTKAMD_EIO and names the file
 *   CreateGrid / DoCompare /         htkamd_results_score: a wavefront per (reference, hypothesis) pair, lanes along an anti-diagonal of
 *   DoCompareNIST (:835-1020)        the grid; per pair H, D, S, I, N = H+D+S and whether HResults counts it: a pair whose reference or
 *                                    hypothesis is EMPTY is aligned (its counts are the edge cell's) but, as in MatchFiles :1728 and
 *                                    MatchRecFiles :1308, left out of the totals, the text and the confusion matrix (status 0)
 *   AppendCell / CollectStats        the traceback from (nTest, nRef): (op, refId, testId) triples in the order -t prints them, -1 for
 *   (:1050, :1259)                   the side an insertion / deletion lacks; steps that involve the null class are dropped as both drop them
 *   RecordFileStats (:530)           totals per set: H D S I N, sentences, correct sentences; the -p matrix [V+1][V+1] (V = nList):
 *                                    [r][t] label r recognised as t, [r][0] deletions of r, [0][t] insertions of t
 *   Print* / OutTrans / OutConMat    htkamd_results_write: the reference's text from those numbers, no device involved
 * Not supported, each refused with a message that names it (htkamd_results_check_switch for a tool's command line): word spotting
 * (-w, -u), per-speaker results (-k), the NIST output format (-h), N-best scoring (-d), file limits (-m, -j), renaming the phrase and
 * phone labels (-a, -b); label levels other than 0 (refLevel / testLevel).
 * ------------------------------------------------------------------------------------------ */
typedef struct htkamd_results htkamd_results;
typedef struct {
   const char *nullName;                 /* -z; NULL = "???"                                                        */
   int ignoreCase, stripContexts, nist;  /* -c, -s, -n (penalties 4 / 3 / 3 and DoCompareNIST's tie order)          */
   int nEquiv;                           /* -e class label, in command-line order                                   */
   const char *const *equivClass, *const *equivLabel;
   int nList; const char *const *list;   /* the label list; only the confusion matrix needs it (at most 200 names)  */
   int refLevel, testLevel;              /* REFLEVEL / TESTLEVEL: must be 0                                         */
} htkamd_results_config;
#define HTKAMD_RES_ALIGN   1             /* score: return the alignment triples                                     */
#define HTKAMD_RES_CONF    2             /* score: fill the confusion matrices (runs the traceback too)             */
#define HTKAMD_RES_FULL    4             /* write: -f, a line per file                                              */
#define HTKAMD_RES_TRANS   8             /* write: -t, the aligned transcriptions of the files with an error        */
#define HTKAMD_RES_PSTATS 16             /* write: -p, the confusion matrix                                         */
#define HTKAMD_RES_HIT 0
#define HTKAMD_RES_SUB 1
#define HTKAMD_RES_DEL 2
#define HTKAMD_RES_INS 3
int  htkamd_results_create(const htkamd_results_config *cfg, htkamd_results **out);
void htkamd_results_destroy(htkamd_results *r);
int  htkamd_results_check_switch(const char *sw);                     /* "-w" ...: HTKAMD_OK for a switch this path has, HTKAMD_EINVAL and the reason otherwise */
int  htkamd_results_label_id(htkamd_results *r, const char *name);    /* >= 0, or a negative HTKAMD_E* code                                          */
const char *htkamd_results_label_name(const htkamd_results *r, int id);
int  htkamd_results_num_labels(const htkamd_results *r);              /* ids 0 .. n-1 exist                                                         */
/* A reference transcription by utterance name: returns its index (>= 0; a name given again keeps its first transcription) or HTKAMD_E*. */
int  htkamd_results_add_ref(htkamd_results *r, const char *utt, int n, const char *const *names);
int  htkamd_results_find_ref(const htkamd_results *r, const char *utt);       /* index or -1 */
int  htkamd_results_ref_len(const htkamd_results *r, int ref);
/* The reference of hypothesis file `recFile`: its name (directory labDir or the file's own, extension labExt or "lab") goes to labFile;
   taken from the first of the nMlf master label files that has it, else from that file; added under that name and its index returned. */
int  htkamd_results_ref_for(htkamd_results *r, const char *recFile, const htkamd_mlf *const *mlfs, int nMlf, const char *labDir, const char *labExt,
                            char *labFile, size_t labFileLen);
int  htkamd_results_ids(htkamd_results *r, const htkamd_labels *l, int *ids /*[htkamd_labels_count(l)]*/);
/* Pair p = k * U + u: hypothesis hypIds[hypOff[p] .. hypOff[p+1]) of set k against reference uttRef[u].  counts [K*U][6]: H D S I N status.
   With HTKAMD_RES_ALIGN: pair p's triples are aln[3 * alnOff[p] .. 3 * alnOff[p+1]); alnCap (in triples) must hold the sum of nRef + nTest
   over all pairs.  totals [K][7]: H D S I N sentences correct.  conf [K][(V+1)*(V+1)] with HTKAMD_RES_CONF (a label outside the list is
   HTKAMD_EINVAL and named, Index :1151).  Outputs that are not wanted may be NULL.  Synchronises `stream`. */
int  htkamd_results_score(htkamd_results *r, int K, int U, const int *uttRef, const int *hypOff, const int *hypIds, int flags,
                          int *counts, int *alnOff, int *aln, long long alnCap, long long *totals, int *conf, void *stream);
double htkamd_results_last_kernel_ms(const htkamd_results *r);       /* device time of the last call's kernels (events around them) */
int  htkamd_results_dir_tile(void);                                   /* grid cells (nRef * nTest) whose `dir` bytes a wavefront keeps in LDS; a larger pair uses global scratch */
typedef struct {
   int flags;                            /* HTKAMD_RES_FULL | _TRANS | _PSTATS                                       */
   const char *refId;                    /* "Ref :": the last -I file, else the -L directory, else NULL              */
   int nRecId; const char *const *recId; /* "Rec :": the hypothesis arguments (the first five are printed)           */
   int nFiles;
   const char *const *recFile, *const *labFile;   /* per file, as HResults names them                               */
   const int *counts;                    /* [nFiles][6]                                                              */
   const int *alnOff, *aln;              /* -t                                                                       */
   const long long *totals;              /* [7]                                                                      */
   const int *conf;                      /* -p: [(V+1)*(V+1)]                                                        */
} htkamd_results_report;
/* path NULL = stdout; append: add to the file instead of replacing it */
int  htkamd_results_write(const htkamd_results *r, const htkamd_results_report *rep, const char *path, int append);

/* ------------------------------------------------------------------------------------------
 * Rescoring lattices: replaces HLRescore (HTKTools/HLRescore.c) -f / -t / -u / -w for U lattices under a grid of K settings
 * {acscale -a, lmscale -s, wdpenalty -p, prscale -r} in ONE call (csrc/latrescore.hip; files, orders, labels and text: host/latrescore.c).
 *   ReadLattice (HNet.c:1230)         htkamd_latset_add_file: header, I= lines with t= W= v=, J= lines with S= E= W= v= a= l= r= d= (the alignment
 *                                     records travel with their arcs); what ReadLattice refuses is refused with its reason; sub-lattices (SUBLAT=, L=) and
 *                                     binary fields (~) are refused by name.  htkamd_latset_add: a lattice from the decoder's arrays
 *   LatStartNode / LatEndNode /       done once per lattice when it is added: the node order of the depth-first walk from the end node
 *   LatTopSort (HLat.c:367-455)       over the pred lists (an arc joins the FRONT of its nodes' lists as its J= line is read), the order in
 *                                     which the forward loop meets arcs (nodes in that order, each foll list front to back) and its mirror;
 *                                     a cyclic lattice is HTKAMD_EMODEL with LatTopSort's message
 *   LatFindBest (HLat.c:575)          htkamd_latset_best: per (k, u) the best path's arcs, start to end, and the ac lm pr tot sums of -T 4;
 *                                     of two equally good arcs into a node the first met stays (score > end->score)
 *   LatForwBackw (.., LATFB_MAX :490) htkamd_latset_fb_max: Fw, Bw per node and best = Bw[first node of the order]
 *   LatPrune (HLat.c:711)             htkamd_latset_prune: keep flags per node and arc (beamPruneArcs = T, HLat.c:77), the arcs-per-second
 *                                     histogram included; htkamd_latset_add_pruned compacts the survivors into another set
 *   LatSetScores (HLat.c:688)         htkamd_latset_fb_max on the pruned set: score = Fw + Bw
 *   WriteLattice (HNet.c:631)         htkamd_latset_write
 * LArcTotLike (HNet.h:257) is float arithmetic plus a double word penalty, added to fp64 node scores in the reference's order: every
 * number compares bit for bit.  Per-node arrays of K settings are INTERLEAVED: node n of lattice u under setting k stands at
 * K * nodeOff[u] + n * K + k (nodeOff = the nodes of the lattices before u), so that a wavefront's lanes touch neighbouring addresses.
 * Not served, each refused by name (htkamd_latset_check_switch): -n / -wn (LatExpand), -m, -c, -I, -d, -P, FIXBADLATS; LATFB_SUM
 * is reached by no switch of the tool.
 * ------------------------------------------------------------------------------------------ */
typedef struct htkamd_latset htkamd_latset;
typedef struct { float acScale, lmScale, wordPen, prScale; } htkamd_lat_scales;
int  htkamd_latset_create(const char *dictPath, const char *startWord, const char *endWord, htkamd_latset **out);
int  htkamd_latset_create_like(const htkamd_latset *src, htkamd_latset **out);      /* an empty set over the same dictionary */
void htkamd_latset_destroy(htkamd_latset *s);
int  htkamd_latset_add_file(htkamd_latset *s, const char *path);                    /* returns the lattice's index (>= 0) or HTKAMD_E* */
int  htkamd_latset_add(htkamd_latset *s, const htkamd_lattice *lat, const htkamd_net *net);
/* LatPrune's new lattice: the nodes and arcs of src's lattice u whose flags are set, in their order, renumbered */
int  htkamd_latset_add_pruned(htkamd_latset *dst, const htkamd_latset *src, int u, const unsigned char *keepNode, const unsigned char *keepArc);
int  htkamd_latset_count(const htkamd_latset *s);
int  htkamd_latset_check_switch(const char *sw);
int  htkamd_latset_tile(void);            /* nodes of a lattice whose scores a lane keeps in LDS; a larger lattice goes through global scratch */
typedef struct {
   int nNodes, nArcs, start, end;
   const double *nodeTime; const int *nodeWord, *nodeVar;      /* nodeWord: index for htkamd_latset_word_name, 0 = !NULL */
   const int *arcStart, *arcEnd; const float *arcAc, *arcLm, *arcPr;
   const int *topOrder;                   /* [nNodes] LatTopSort */
   const int *fwdArcs, *bwdArcs;          /* [nArcs] arcs as the forward / backward loop meets them */
} htkamd_latset_view;
int  htkamd_latset_get(const htkamd_latset *s, int u, htkamd_latset_view *out);
const char *htkamd_latset_word_name(const htkamd_latset *s, int word);
/* Outputs for pair (k, u): nPath / status [k * U + u] (status 1, or 0 where no arc leads into the end node: an empty path), the path's arcs
 * at pathArcs[k * totalNodes + nodeOff[u] ..], totals [4 * (k * U + u)] = ac lm pr tot.  Synchronises `stream`. */
typedef struct { int *nPath, *status, *pathArcs; double *totals; } htkamd_latset_best_out;
int  htkamd_latset_best(htkamd_latset *s, int K, const htkamd_lat_scales *scales, const htkamd_latset_best_out *out, void *stream);
/* fw, bw: [K * totalNodes], interleaved (above); best [K * U] */
typedef struct { double *fw, *bw, *best; } htkamd_latset_fb_out;
int  htkamd_latset_fb_max(htkamd_latset *s, int K, const htkamd_lat_scales *scales, const htkamd_latset_fb_out *out, void *stream);
/* keepNode [k * totalNodes + nodeOff[u] + n], keepArc [k * totalArcs + arcOff[u] + a]; thresh / arcsPerSec [K]: -t f [a] */
int  htkamd_latset_prune(htkamd_latset *s, int K, const htkamd_lat_scales *scales, const double *thresh, const float *arcsPerSec,
                         unsigned char *keepNode, unsigned char *keepArc, void *stream);
double htkamd_latset_last_kernel_ms(const htkamd_latset *s);
/* LatFindBest's label list for one path: outSym of the pronunciation v=, the word's name where that variant is missing; null words and
 * empty output symbols give no label; times = node time * 1e7; score = (float)LArcTotLike */
int  htkamd_latset_trans(const htkamd_latset *s, int u, const htkamd_lat_scales *sc, const int *arcs, int nArcs, htkamd_trans **out);
/* K x U best paths -> the hypOff [K*U + 1] / hypIds arrays of htkamd_results_score (pair k * U + u); returns the number of ids, which may
 * exceed cap (nothing past cap is written), or HTKAMD_E* */
int  htkamd_latset_best_ids(const htkamd_latset *s, htkamd_results *r, int K, const int *nPath, const int *pathArcs, int *hypOff, int *hypIds, int cap);
/* WriteLattice with the header scales as HLRescore sets them; nodeScore [nNodes] (LatSetScores) or NULL = zeros (SORTLATTICE = F);
 * format: HTKAMD_LAT_* bits, 0 = HLRescore's default (HLAT_DEFAULT | HLAT_PRLIKE: t v a l d m n r) */
int  htkamd_latset_write(const htkamd_latset *s, int u, const htkamd_lat_scales *sc, const double *nodeScore, const char *path, int format);

/* ------------------------------------------------------------------------------------------
 * Label statistics and bigram models (HLStats): a batch of label sequences counted in one call.
 * Replaces InitStats (HLStats.c:367), GatherStats (:471) and OutputStats (:888).  The counting is integer work on the device
 * (csrc/lstats.hip); the probabilities are host arithmetic in the reference's types and order (host/lstats.c), so the files match the
 * reference's byte for byte.
 * Word ids: 0 = a label that is not in the list (the reference's !NULL slot), 1..htkamd_lstats_nwords = the list as the reference sorts
 * it: the start label first, the end label last (both added when the list lacks them), strcmp order between.  The list is HLStats'
 * hmmList with one name a line (no logical -> physical pairs, so -p is refused and -c's PCount column counts the same labels).
 * A start label at the head of an utterance and an end label at its tail are skipped, as GatherStats skips them.
 * ------------------------------------------------------------------------------------------ */
typedef struct htkamd_lstats htkamd_lstats;
int  htkamd_lstats_create(const char *const *words, int nWords, const char *enterWord /* -s; NULL = !ENTER */, const char *exitWord /* NULL = !EXIT */, htkamd_lstats **out);
void htkamd_lstats_destroy(htkamd_lstats *s);
int  htkamd_lstats_nwords(const htkamd_lstats *s);
const char *htkamd_lstats_word(const htkamd_lstats *s, int id);
int  htkamd_lstats_id(const htkamd_lstats *s, const char *name);      /* 0: not in the list */
/* ids (and times, either may be NULL) of a label list: [htkamd_labels_count(l)] */
int  htkamd_lstats_ids(const htkamd_lstats *s, const htkamd_labels *l, int *ids, long long *start, long long *end);
/* Counts the batch: utterance u = labIds[labOff[u] .. labOff[u+1]), the form htkamd_results_score takes.  start / end: the labels' times in
 * 100 ns units for the duration statistics (-d), or both NULL.  A call replaces what the call before counted.  Synchronises `stream`. */
int  htkamd_lstats_count(htkamd_lstats *s, int nUtt, const int *labOff, const int *labIds, const long long *start, const long long *end, void *stream);
/* Results over ids 0..nwords: count = lTab[].count (with the start and end label of every utterance), pcount = occurrences as labels,
 * durations in 100 ns units (min / max of a word never seen: LLONG_MAX / LLONG_MIN), rowOff [nwords + 2] = the CSR rows by predecessor.
 * Any pointer may be NULL. */
int  htkamd_lstats_get(const htkamd_lstats *s, int *count, int *pcount, long long *durSum, long long *durMin, long long *durMax, int *rowOff);
int  htkamd_lstats_bigrams(const htkamd_lstats *s, int *succ, int *cnt);      /* [rowOff[nwords + 1]]: successors increasing within a row */
double htkamd_lstats_last_kernel_ms(const htkamd_lstats *s);
/* HLStats -b path: backoff != 0 is -o (OutputBoBigram; uniFloor -u, bigThresh -t, discount = the DISCOUNT configuration value, 0.5),
 * else the matrix bigram (OutputMatBigram; bigFloor -f).  tracePath: the lines -T 4 prints are APPENDED to that file; NULL = none. */
int  htkamd_lstats_bigram_write(const htkamd_lstats *s, const char *path, int backoff, float uniFloor, int bigThresh, float bigFloor, double discount, const char *tracePath);
/* What HLStats prints: flags HTKAMD_LS_DURS (-d; needs the times), HTKAMD_LS_LIST (-l listPath), HTKAMD_LS_COUNTS (-c countLimit), in the
 * reference's order.  HLStats prints the -T 4 lines of the bigram between the durations and the counts: write the durations, then the
 * bigram with tracePath = path, then the rest with append != 0. */
#define HTKAMD_LS_DURS   1
#define HTKAMD_LS_LIST   2
#define HTKAMD_LS_COUNTS 4
int  htkamd_lstats_stats_write(const htkamd_lstats *s, const char *path, int append, int flags, int countLimit, const char *listPath);
int  htkamd_lstats_check_switch(const char *sw);      /* 0 for a switch of HLStats that is served ("-b"), else HTKAMD_EINVAL and the refusal by name */
/* Counts planted in place of a counting run (tests of the host arithmetic): count = occurrences as labels, then the CSR table and the durations */
int  htkamd_lstats_plant(htkamd_lstats *s, int nUtt, const int *count, const int *rowOff, const int *succ, const int *cnt, const long long *durSum, const long long *durMin,
                         const long long *durMax);
/* The device chain over caller tables: V ids, boundary ids, and the capacities of the wavefront path and the workgroup path of the row
 * kernel (1 <= waveCap <= htkamd_lstats_wave_cap(), waveCap <= groupCap <= htkamd_lstats_group_cap(); a row longer than groupCap goes
 * through the histogram path with windows of groupCap ids).  count / dur* [V], rowOff [V + 1], succ / cnt [pairCap]. */
int  htkamd_lstats_probe(int V, int nUtt, const int *labOff, const int *labIds, const long long *start, const long long *end, int enterId, int exitId, int waveCap, int groupCap,
                         int *count, long long *durSum, long long *durMin, long long *durMax, int *rowOff, int *succ, int *cnt, int pairCap, void *stream);
int  htkamd_lstats_wave_cap(void);
int  htkamd_lstats_group_cap(void);

/* ------------------------------------------------------------------------------------------
 * Word networks from a word list or a bigram model (HBuild).  htkamd_bigram_read = ReadLModel (HLM.c:813) for the two text forms HLStats
 * writes; words 1..N in file order, log probabilities natural.  The networks are ProcessWordLoop (HBuild.c:299), ProcessBoBiGram (:368)
 * and ProcessMatBiGram (:463): nodes, arcs and l= values as HBuild saves them, the arcs of the bigram forms written on the device
 * (csrc/netbuild.hip).  The word loop's nodes follow the word list (the reference's follow the addresses of its name table and change
 * from run to run).  `words` = HBuild's word list: every word of the model must be in it.
 * ------------------------------------------------------------------------------------------ */
#define HTKAMD_LM_BACKOFF 0
#define HTKAMD_LM_MATRIX  1
typedef struct htkamd_bigram htkamd_bigram;
int  htkamd_bigram_read(const char *path, htkamd_bigram **out);
void htkamd_bigram_destroy(htkamd_bigram *b);
int  htkamd_bigram_type(const htkamd_bigram *b);
int  htkamd_bigram_nwords(const htkamd_bigram *b);
const char *htkamd_bigram_word(const htkamd_bigram *b, int i);      /* 1..N */
int  htkamd_bigram_nbigrams(const htkamd_bigram *b);
/* back-off form: unigram / bowt / hasEntry [N + 1], rowOff [N + 2], succ / prob [nbigrams]; matrix form: mat [(N + 1) * (N + 1)] */
int  htkamd_bigram_get(const htkamd_bigram *b, float *unigram, float *bowt, int *hasEntry, int *rowOff, int *succ, float *prob, float *mat);
typedef struct htkamd_wordnet htkamd_wordnet;
/* bracketStart / bracketEnd: -t s1 s2, or both NULL */
int  htkamd_netbuild_loop(const char *const *words, int nWords, const char *bracketStart, const char *bracketEnd, htkamd_wordnet **out);
/* -n / -m by the model's form; enterWord / exitWord -s (NULL = !ENTER / !EXIT), unknownWord -u (NULL = !NULL), zapUnknown -z */
int  htkamd_netbuild_bigram(const htkamd_bigram *b, const char *const *words, int nWords, const char *enterWord, const char *exitWord, const char *unknownWord, int zapUnknown,
                            htkamd_wordnet **out, void *stream);
void htkamd_wordnet_destroy(htkamd_wordnet *n);
/* the network as a lattice: nodePron = index for htkamd_wordnet_word (-1: !NULL), times and acoustic scores 0, lmScale 1 */
const htkamd_lattice *htkamd_wordnet_lattice(const htkamd_wordnet *n);
const char *htkamd_wordnet_word(const htkamd_wordnet *n, int w);
double htkamd_wordnet_last_kernel_ms(const htkamd_wordnet *n);
int  htkamd_wordnet_write(const htkamd_wordnet *n, const char *path);      /* SaveLattice: the SLF file; the bigram networks byte for byte HBuild's */
int  htkamd_wordnet_nwords(const htkamd_wordnet *n);
/* the network (htkamd_wordnet_lattice and the words its nodePron index) expanded over a dictionary and a model set as htkamd_net_build_ex
 * expands its SLF file, without the file: arcs in the file's order, every l= through the file's two decimals */
int  htkamd_net_build_lattice(const htkamd_lattice *lat, const char *const *words, int nWords, const char *dictPath, const htkamd_mmf *hmms, int flags,
                              htkamd_net **out);
int  htkamd_netbuild_check_switch(const char *sw);
/* k_nb_arcs over caller tables, words 1..N: mode HTKAMD_LM_*; back-off: rowOff [N + 2] / succ / val = the rows, rowVal [N + 1] the back-off
 * weights, uni [N + 1] the unigrams; matrix: val [(N + 1) * (N + 1)].  nodeOf [N + 1] (-1: no node), rowKeep [N + 1]. */
int  htkamd_netbuild_probe(int mode, int N, const int *rowOff, const int *succ, const float *val, const float *rowVal, const float *uni, const int *nodeOf, const int *rowKeep,
                           int enterIdx, int zapIdx, int backNode, int *arcStart, int *arcEnd, float *arcLm, int arcCap, int *nArcs, void *stream);

#ifdef __cplusplus
}
#endif
#endif
