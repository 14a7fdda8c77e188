// lstats.h -- what the label-statistics launcher (lstats.hip), its host arithmetic (host/lstats.c) and the network builder
// (host/netbuild.c, netbuild.hip) share.  Plain C.
#pragma once
#include "internal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Word ids: 0 = a label that is not in the list (HLStats' !NULL slot, lTab[0]); 1..lSize = the list as InitStats sorts it (wd_cmp
   HLStats.c:343: the enter word first, the exit word last, strcmp between). */
struct htkamd_lstats {
   int lSize, enterId, exitId;
   char **name;                          /* [lSize + 1], name[0] = "!NULL" */
   int counted, haveDur, nUtt, durOdd;
   int *count, *pcount;                  /* [lSize + 1]: lTab[].count (the boundary words coerced per utterance included) / pCntr->count */
   long long *durSum, *durMin, *durMax;  /* [lSize + 1], 100 ns units; min / max untouched (LLONG_MAX / LLONG_MIN) for a word never seen */
   int *rowOff, *succ, *cnt;             /* CSR over predecessors 0..lSize: rowOff[lSize + 2] */
   double kernelMs;
   void *dev;                            /* the launcher's workspaces (htkamd_lstats_device_free) */
};

/* the whole device chain over caller tables (lstats.hip); dev = NULL: workspaces of this call only.  succ / cnt: [pairCap]. */
int htkamd_lstats_device(void **dev, int V, int nUtt, const int *labOff, const int *labIds, const long long *start, const long long *end, int enterId, int exitId,
                         int waveCap, int groupCap, int *count, long long *durSum, long long *durMin, long long *durMax, int *rowOff, int **succ, int **cnt,
                         int *durOdd /* labels whose duration is no whole number of ms; may be NULL */, double *kernelMs, void *stream);
void htkamd_lstats_device_free(void *dev);

/* A bigram model as HLM.c's ReadLModel keeps it.  Words 1..N in file order. */
struct htkamd_bigram {
   int type;                             /* HTKAMD_LM_BACKOFF / HTKAMD_LM_MATRIX */
   int N;
   char **name;                          /* [N + 1] */
   float *unigram, *bowt;                /* [N + 1] natural logs; back-off only */
   int *hasEntry;                        /* [N + 1] a back-off weight was read for the word (GetNEntry != NULL) */
   int *rowOff, *succ;                   /* [N + 2], [nBigrams]: rows by predecessor, successors increasing */
   float *prob;                          /* [nBigrams] */
   float *mat;                           /* matrix form: [(N + 1) * (N + 1)] natural logs */
};

/* A word network: HBuild's Lattice.  nodeWord -1 = !NULL. */
struct htkamd_wordnet {
   int nNodes, nArcs, nWords;
   char **word;                          /* [nWords] */
   int *nodeWord, *nodeFrame; double *nodeLike;
   int *arcStart, *arcEnd; float *arcLm, *arcZero;
   htkamd_lattice lat;
   double kernelMs;
};

/* k_nb_arcs over caller tables (netbuild.hip): rows 1..N; see netbuild.hip for the tables. */
int htkamd_netbuild_device(int mode, int N, const int *rowOff, const int *succ, const float *val, const float *rowVal, const float *uni, const int *nodeOf,
                           const int *rowKeep, int enterIdx, int zapIdx, int backNode, int *arcStart, int *arcEnd, float *arcLm, int arcCap, int *nArcs,
                           double *kernelMs, void *stream);

#ifdef __cplusplus
}
#endif
