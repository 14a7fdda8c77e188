// decode.h -- what the network decoder's kernels (decode.hip: 1-best; decode_n.hip: N-best token sets + lattice) and their host code share
// (the kernels' shared DEVICE code: decode_dev.h, decode_ord.h).
#pragma once
#include <hip/hip_runtime.h>
#include <functional>
#include <vector>
#include "internal.h"
#include "kernels.h"

#define DEC_THREADS 1024
#define DEC_MAXN 8              /* states per model incl. entry/exit */
#define DEC_SET_THREADS 256     /* workgroup of the kernel that takes a network per utterance (alignment networks: tens to hundreds of nodes) */
#define DEC_MAX_TOKS 8          /* capacity of a token set (HVite -n up to 8; decode_n.hip) */
#define DEC_WIDE 96             /* fan-in from which a node is reduced by the whole workgroup */

struct DecNet {
   int nNodes, nHmm, nLevels, nWordNodes, initial, final, nTok, nTpFloats;
   const int *kind, *model;            // [nNodes]
   const float *pronProb;              // [nNodes]
   const int *predOff, *predSrc;       // reverse CSR; bit 31 of predSrc: the predecessor is a word/null node
   const float *predLike;
   const int4 *nodeInfo;               // [nNodes] {kind | N << 4 | tee << 12, first token, offset of transP, offset into hmmState}
   const int *tok0;                    // [nNodes] first token (state 1) of the node
   const int *hmmNodes;                // [nHmm] model nodes (tee or not)
   const int *nodeN, *nodeTp, *nodeSt; // [nNodes] HMM: numStates, offset of transP, offset into hmmState
   const unsigned char *nodeTee;       // [nNodes]
   const float *wdlk;                  // [nNodes]
   const int *wordIdx;                 // [nNodes] dense index of WORD nodes (path table column) or -1
   const int *wordNode;                // [nWordNodes] inverse of wordIdx
   const int *levelOff, *levelNodes;   // zero-time nodes by level: narrow ones first, then wide ones
   const int *levelWide;               // [nLevels] index in levelNodes where the wide nodes of the level start
   const int *levelOffAll, *levelNodesAll, *levelWideAll;   // the same with the nodes k_decode<NPT > 0> steps from registers (regFused) left in
   const float *transP;
   const int *hmmState;
   const int *stateSlot;               // [S] row of the tied state in the score block, -1 if unused
   // forward CSR in the network's own link order (the tr0 links first, ExpandWordNet HNet.c:3632-3645): the exact-order kernels
   // (decode_ord.hip) PUSH along it as HRec does
   const int *linkOff, *linkDest;      // [nNodes + 1], [nLinks]
   const float *linkLike;
   const int *nTr0;                    // [nNodes] number of leading links whose destination is a zero-time node (word end, null node, tee model)
   const unsigned char *dupDest;       // [nNodes] two links of the node share a destination
   // k_decode<NPT > 0>: hmmNodes[0 .. nReg) are plain models of at most three emitting states whose tokens live in registers
   int nReg;
   const int *regFused;                // [nReg] the word / null node whose only predecessor is this model (stepped by its owner), or -1
   const float *regFusedLike;          // [nReg] LM log probability of that link
   const unsigned char *regNoEx;       // [nReg] nobody pulls this model's exit token from memory
   // k_decode<.., EXL>: the exit tokens the register-resident models pull are kept in LDS beside memory -- a WORD node's as its likelihood alone
   // (its lm is 0 and its path is frame * nWordNodes + wordIdx: StepWord2 HRec.c:1046), a null node's whole
   const int *zl;                      // [nNodes] -1, or bit 30 | wordIdx (WORD node), or the null node's slot in the LDS table
   int nNullLds;                       // null nodes with a slot (<= DEC_NULL_LDS)
   const int2 *predRecL;               // [links] predRec with x = bit 31 | bit 30 | wordIdx for a WORD predecessor, bit 31 | bit 29 | slot for a null node with a slot
   const int *regFusedZl;              // [nReg] zl of the model's fused node (-1: none / no slot)
   const int4 *regFusedRec;            // [nReg] {fused node or -1, its zl, bits of its pronProb, its wordIdx or -1}: StepWord2 without four dependent loads
   const int2 *regPred;                // [nReg] the model's range in predRecReg / predRecRegL: the entry pull's range without the two loads behind the node's number
   const int2 *predRecReg, *predRecRegL;   // the register-resident models' lists of predRec / predRecL, in the models' order
   const int2 *predRec;                // [links] {predSrc, bits of predLike}: one load per predecessor
   const int4 *regRecA, *regRecB; const float2 *regRecF;      // [nReg] the same and the model's constants packed: {node, kind | N << 4, transP offset, fused node}, {score slots of states 2..4, regNoEx}, {wdlk, fused link's LM}
};
// 1024 threads x 6 models: four wavefronts per SIMD hide one another's memory latencies; 512 x 12 (round 4: no register spills to speak of,
// two wavefronts per SIMD) took 50 ms where this takes 41 on the 6 000-word bigram network, 768 x 8 42 (tools/r05_decvar.sh)
#define DEC_REG_THREADS 1024
#define DEC_REG_MAXNPT 6
#define DEC_NULL_LDS 64             /* null nodes whose tokens k_decode<.., EXL> keeps in LDS */

struct DecUtt {
   int T, frame0, status, idx;         // idx: the utterance's number in the batch (its slot in the per-utterance outputs)
   size_t score0;      // floats: score[score0 + slot*T + (t-1)]
   size_t tok0;        // token arrays base
   size_t node0;       // exit-token / instance-max arrays base
   size_t path0;       // path table base: (t*nWordNodes + w)
   size_t out0;        // word output base
   int net, ns;        // k_decode<.., SET> (decode_set.hip): the utterance's network in DecArgs::nets and the rows of its score columns; 0 elsewhere
};

struct __attribute__((aligned(16))) Tok { double like; float lm; int path; };   // one 16-byte load/store per token

struct DecArgs {
   DecNet net;
   const DecUtt *utt; int nUtt;
   const float *score; int ns;         // frame-major since round 4: score[score0 + (t-1)*ns + slot] (k_score_transpose), ns = tied states of the network
   Tok *tok;                           // [sum nTok]   state tokens
   Tok *ex; double *imax;              // [sum nNodes] exit tokens, instance maxima
   int *pathPrev; double *pathLike; float *pathLm;
   float genBeam, wordBeam, lmScale, wordPen, prScale;
   int maxActive;                      // HVite -u: maximum number of model instances kept per frame (0 = off)
   int maxWords;
   int *nWords, *wordPron, *wordStart, *wordEnd; float *wordScore, *wordLm, *wordAc; double *wordLike; double *total; float *finalLm;
   unsigned long long *liveCnt;        // [nUtt][2] k_decode<NPT > 0>: register-resident model instances stepped with a live token / with none (htkamd_decoder_last_live)
   int *tieFlag;                       // [nUtt] k_decode: two tokens of exactly equal likelihood and different histories met at a node (see decode_ord.hip)
   const DecNet *nets;                 // k_decode<.., SET>: a network per utterance, nets[DecUtt::net] (net and ns above are then not read); NULL elsewhere
};

// Exact-order decoding (decode_ord.hip, k_decode_ord_n of decode_n.hip): HRec's instance list and the Path records it needs
struct OrdList {
   int *seq; int seqCap;               // [nSel * 2 * seqCap] the instance list as an array (two buffers per utterance)
   int *pos; unsigned char *ooo;       // [sum nNodes] (at DecUtt.node0) position of the node's instance in seq (-1: none); NetInst.ooo
   int *pathNode, *pathFrame;          // [paths] (at DecUtt.path0) Path records are allocated one by one here
   int pathExtra;                      // records per utterance beyond (T + 1) * nWordNodes
};
// k_decode_ord: the utterances k_decode flagged, or every utterance of a run in HTKAMD_ORDER_EXACT
struct OrdArgs {
   DecArgs d;                          // utt = the selected utterances' descriptors (idx = slot in the outputs)
   OrdList list;
   int keepFast;                       // the outputs hold k_decode's result of the same utterance (HTKAMD_ORDER_AUTO): a walk that runs out of one of its
                                       // fixed capacities (-4 path records, -5 list appends of a frame, -6 nesting of zero-time nodes) leaves it standing
};
int htkamd_launch_decode_ord(const OrdArgs &a, int nSel, hipStream_t s);
// The capacities the list kernels (k_decode_ord, k_decode_ord_n) assume per utterance.  Path records: StepWord2 "may be repeated"
// (HRec.c:1046), so the list kernels get room for every word node thrice per frame and some more (the static order: pathMul = 1, pathExtra = 0).
enum { DEC_ORD_PATH_MUL = 3, DEC_ORD_PATH_EXTRA = 64 };
inline size_t htkamd_dec_path_records(size_t pathMul, size_t T, int nWordNodes, size_t pathExtra) { return pathMul * (T + 1) * (size_t)nWordNodes + pathExtra; }
// ... and the instance list: appends of one frame's pass 2 (attaches + moves) on top of the live instances
inline int htkamd_dec_ord_seq_cap(int nNodes) { return 8 * nNodes + 1024; }
// K1 writes a score block state-major (a state's frames are a lane's stores); the token loops read a COLUMN per frame: one 128-byte line per
// state and frame -- 640 KB per utterance and frame on the 5k-state set.  Transposed once (tiles through LDS), a frame's column is 20 KB.
// ns > 0: rows per utterance (one network); ns = 0: DecUtt::ns rows, at most maxNs (a network per utterance)
int htkamd_launch_score_transpose(const float *in, float *out, const DecUtt *dUtt, int nUtt, int maxT, int ns, hipStream_t s, int maxNs = 0);


// The decoders' device workspace: a fixed table of buffers kept between calls and grown (never shrunk) when a batch needs more -- the score
// block and the path tables are gigabytes at 256 utterances: allocating and freeing them per call cost 5 - 500 ms of a 130 ms call.
// A call takes its buffers in a fixed order from slot 0 (begin, get, get, ...); a group of buffers that only some calls need starts at a
// slot of its own (seek), so that the buffers after it keep their slots whether the group is there or not.
struct DecArena {
   enum { SLOTS = 64 };
   void *ptr[SLOTS] = {};
   size_t cap[SLOTS] = {};
   hipStream_t stream = nullptr;       // of the current call: synchronised before a buffer in use is replaced
   const char *who = "";               // ... and the name its errors start with
   int next = 0;                       // slot the next get() takes
   int rc = HTKAMD_OK;                 // first failure of the call: every later get() returns NULL
   void begin(hipStream_t s, const char *prefix) { stream = s; who = prefix; next = 0; rc = HTKAMD_OK; }
   void seek(int slot)                 // the next get() takes `slot` (HTKAMD_EINVAL where the buffers before it have reached it)
   {
      if (next > slot && !rc) { htkamd_set_error("%s: workspace buffers run into slot %d", who, slot); rc = HTKAMD_EINVAL; }
      next = slot;
   }
   void *get(size_t bytes);            // at least `bytes` (0 counts as 1); NULL and rc on failure: HTKAMD_ENOMEM, HTKAMD_EINVAL out of slots
   void release() { for (int i = 0; i < SLOTS; i++) { if (ptr[i]) (void)hipFree(ptr[i]); ptr[i] = nullptr; cap[i] = 0; } }
};

// What the decoders do alike (decode.hip).
int htkamd_decoder_order(int mode);      // a decoder's order mode, HTKAMD_DECODE_ORDER (fast | exact | anything else: auto) overriding it
// The per-utterance work space a chunk of a batch may take by the caller's estimate (htkamd_decoder_plan_nets; HTKAMD_DECODE_CHUNK_BYTES overrides)
constexpr size_t DEC_CHUNK_BYTES = (size_t)24 << 30;
// Utterances u0 .. u1 of a batch: as many as stay under DEC_CHUNK_BYTES of per-utterance work space by the caller's estimate (at least one), their
// descriptors, the score block's tasks and the sizes of the per-utterance arrays in elements.
struct DecBatch {
   int u1, maxT;
   std::vector<DecUtt> utt;
   std::vector<ScoreTask> tasks;
   size_t score, tok, node, path;
};
// uttBytes(T): the estimate for an utterance of T frames; DecUtt::out0 = k * outStride; path records per utterance: htkamd_dec_path_records
void htkamd_decoder_plan(const DecNet &N, const int *frameOff, int u0, int nUtt, int ns, int FR, int SL, const std::function<size_t(size_t)> &uttBytes,
                         size_t outStride, size_t pathMul, size_t pathExtra, DecBatch &b);
// The same with a network per utterance (decode_set.hip): what utterance u decodes against, as the plan needs it
struct DecUttNet { const DecNet *N; int net, ns, slot0; };      // slot0: the network's first entry in the scorer's slotState
void htkamd_decoder_plan_nets(const std::function<DecUttNet(int)> &netOf, const int *frameOff, int u0, int nUtt, int FR, int SL,
                              const std::function<size_t(size_t, const DecUttNet &)> &uttBytes, size_t outStride, size_t pathMul, size_t pathExtra, DecBatch &b);
// Uploads the batch's descriptors and tasks (dTasks: room for the tasks and the queue's counter behind them), scores the network's states
// for the batch's frames into dScore (state-major) and transposes that into dScoreT.  evScore (may be NULL): recorded before the scoring launch.
int htkamd_decoder_score(const htkamd_decoder *d, int scoreMode, const float *dX, int nRows, const DecBatch &b, int ns, void *dUtt, void *dTasks,
                         float *dScore, float *dScoreT, hipEvent_t evScore, const char *who, hipStream_t s);
// ... for the model m and the slot table dUsedStates; ns = 0: a network per utterance (DecUtt::ns rows, at most maxNs)
int htkamd_decoder_score_slots(const htkamd_model *m, const int *dUsedStates, int scoreMode, const float *dX, int nRows, const DecBatch &b, int ns, int maxNs,
                               void *dUtt, void *dTasks, float *dScore, float *dScoreT, hipEvent_t evScore, const char *who, hipStream_t s);

// One network's device tables as htkamd_decoder_create builds them (decode.hip), handed table by table to `put` in the order of the single
// decoder's uploads: put(data, bytes, where) stores the table's device address at *where (now, or before the tables are used).
// noReg: no register-resident models (DecNet::nReg = 0: what the kernels that keep every token in memory read).  hmmState (the same for
// every network of a model set) is left NULL when withHmmState is false; usedStates (the tied states in slot order) is uploaded too where
// dUsedStates is not NULL.
typedef std::function<int(const void *, size_t, const void **)> DecPut;
int htkamd_decoder_pack(htkamd_model *m, const htkamd_net_desc *nd, float lmScale, bool noReg, bool withHmmState, const DecPut &put, DecNet &N,
                        std::vector<int> &usedStates, const int **dUsedStates);
// The token kernel's launch.  One network N: tokens of its plain models in registers where it has such models (DecNet::nReg).
int htkamd_launch_decode(const DecArgs &a, const DecNet &N, int nUtt, hipStream_t s);
int htkamd_launch_decode_set(const DecArgs &a, int nUtt, hipStream_t s);      // k_decode<0, DEC_SET_THREADS, true, false, true>

// A 1-best run (htkamd_decoder_run_out, htkamd_decoder_set_run): the batch in chunks under DEC_CHUNK_BYTES, each scored, decoded by `launch`,
// decoded again in exact order where the mode asks for it (k_decode_ord, a launch per network among the chosen utterances) and copied into
// the caller's arrays.  What the two callers differ in:
struct DecRun {
   const char *who;                                    // the name errors start with
   DecArena *ws;
   const htkamd_model *m; const int *dUsedStates;      // the scorer's slot table ...
   int maxNs;                                          // ... and the most rows a network takes of it (0: one network)
   std::function<DecUttNet(int)> netOf;                // what utterance u decodes against
   const DecNet *nets; const int *ns;                  // host side, by DecUttNet::net: the record with its device pointers, the tied states
   const DecNet *dNets;                                // DecArgs::nets; NULL: one network, handed over in DecArgs::net / ns (DecUtt::ns = 0)
   std::function<int(const DecArgs &, int, hipStream_t)> launch;
   int orderMode;
   int *lastTied;                                      // utterances that went through k_decode_ord
   hipEvent_t *ev;                                     // [4] or NULL: around the scoring kernels and around the token kernel ...
   float *scoreMs, *tokenMs;                           // ... whose times are added up over the chunks here
   long long *live;                                    // [2] or NULL: DecArgs::liveCnt summed over the batch
};
int htkamd_decoder_run_1best(const DecRun &r, const htkamd_decode_config *cfg, const float *dX, const int *frameOff, int nUtt, int maxWords,
                             const htkamd_decode_out *out, hipStream_t s);

// An N-best run (htkamd_decoder_run_lattice[_align], htkamd_decoder_set_run_lattice[_align]; decode_n.hip): the batch in chunks under
// DEC_CHUNK_BYTES, each scored, decoded to token sets and lattices by ONE launch (`launch`: the list kernel k_decode_ord_n, or the
// static order k_decode_n with listOrder false) and copied into the caller's arrays.  What the two callers differ in:
struct NArgs;                                          // the token-set kernels' arguments (decode_n.hip)
struct DecNRun {
   const char *who;                                    // the name errors start with (who + "_align" where the alignment records are concerned)
   DecArena *ws;
   const htkamd_model *m; const int *dUsedStates;      // the scorer's slot table ...
   int maxNs;                                          // ... and the most rows a network takes of it (0: one network)
   std::function<DecUttNet(int)> netOf;                // what utterance u decodes against
   const DecNet *nets; const int *ns;                  // host side, by DecUttNet::net: the record with its device pointers, the tied states
   const DecNet *dNets;                                // NArgs::nets; NULL: one network, handed over in NArgs::net / ns (DecUtt::ns = 0)
   const std::vector<int> *hostModel;                  // by DecUttNet::net: [nNodes] htkamd_net_desc.model, for nodePron / alModel
   std::function<int(const NArgs &, int, bool, hipStream_t)> launch;
   int orderMode;                                      // the list kernel unless HTKAMD_ORDER_FAST
   int *lastTied;                                      // utterances that went through the list kernel
};
int htkamd_launch_decode_n(const NArgs &a, int nUtt, bool listOrder, hipStream_t s);          // k_decode_ord_n<false> / k_decode_n<DEC_THREADS, false>
int htkamd_launch_decode_n_set(const NArgs &a, int nUtt, bool listOrder, hipStream_t s);      // k_decode_ord_n<true> / k_decode_n<DEC_SET_THREADS, true>
// alignMode 0: no alignment records (maxAlign and alOut are not read)
int htkamd_decoder_run_nbest(const DecNRun &r, const htkamd_decode_config *cfg, int nToks, float nBeam, const float *dX, const int *frameOff, int nUtt, int maxLatNodes,
                             int maxLatArcs, const htkamd_lattice_out *out, int alignMode, int maxAlign, const htkamd_lattice_align_out *alOut, hipStream_t s);

struct htkamd_decoder {
   htkamd_model *m;
   DecNet net;                         // device pointers
   std::vector<void *> owned;
   std::vector<int> usedStates;        // tied states of the network in slot order
   std::vector<int> hostModel;         // [nNodes] htkamd_net_desc.model (WORD nodes: the pronunciation)
   int *d_usedStates;
   int maxWidthNodes;
   DecArena ws, wsN;                   // workspaces of htkamd_decoder_run and of htkamd_decoder_run_lattice (one each: alternating calls do not evict each other)
   int orderMode;                      // HTKAMD_ORDER_AUTO / _FAST / _EXACT (htkamd_decoder_set_order)
   int lastTied;                       // utterances of the last run that went through the exact-order kernel
   hipEvent_t ev[4];                   // around the scoring kernels and around the token kernel of the last chunk of a run
   float lastScoreMs, lastTokenMs;
   long long lastLive[2];              // model-instance steps of the last run's register kernel: with a live token, without
};
