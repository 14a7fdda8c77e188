/* regtree.c -- regression class trees: HHEd's RC command for one-stream DIAGC sets.  Restated from the reference:
 *   RegClassesCommand (HHEd.c:6177), InitRegTree :5734 with NewHMMScan / GoNextState / GoNextStream / GoNextMix (HUtil.c:246-400) and
 *     InitTreeAccs (HHEd.c:2535): the member list -- which Gaussians, in which ORDER, each with which AccSum record
 *   PItemList (HUtil.c:1100) down to PStatecomp :894 for the one item form of type 'p': hname.state[i-j].mix
 *   BuildRegClusters (HHEd.c:6096), FindBestTerminal :6073, PerturbMean :5850: which terminal is split next, from which seeds
 *   PrintRegTree :6010, PrintBaseClass :6040, GetTreeVector :5997: the two files
 * ClusterChildren (:5961) and everything below it -- the distances, the sums in list order, the convergence loop, the partition, the
 * children's distributions and scores -- runs on the device (csrc/regtree.hip), one launch per split. */
#include <ctype.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mmf_priv.h"
#include "htktext.h"

/* The device side is in the HIP part of the library; a build of the host files alone says so when it is needed (see treeclust.c). */
#pragma weak htkamd_rt_dev_open
#pragma weak htkamd_rt_dev_node
#pragma weak htkamd_rt_dev_split
#pragma weak htkamd_rt_dev_list
#pragma weak htkamd_rt_dev_kernel_ms
#pragma weak htkamd_rt_dev_close

#define RT_MAXTERM 256                                  /* ChkedInt("Maximum number of terminal nodes is 256", 0, 256) */

struct htkamd_regtree {
   int nNodes, nTerm;
   int *left, *right;                                   /* [nNodes], node i at i-1; 0 = none */
   int *compOff;                                        /* [nNodes+1]: a terminal's components; an inner node has none */
   char **compModel; int *compState, *compMix; int nComp;
   int nNames; char **names;                            /* the distinct model names, owned; compModel points into them */
   int nSplits, *iters; float kernelMs;
};

/* ------------------------------------------------------------------------------------------ the tree as tables */
/* The tree's own copy of a model name.  slot[hash] = 1 + index into names (0: free), open addressing over a power of two that is at least
 * twice the number of components, so a look-up is one hash and a compare or two however the classes interleave the models. */
static const char *rt_intern(htkamd_regtree *t, const char *name, int *cap, int *slot, unsigned mask)
{
   if (t->nNames && !strcmp(t->names[t->nNames - 1], name)) return t->names[t->nNames - 1];      /* components come model by model */
   unsigned h = 2166136261u;
   for (const unsigned char *p = (const unsigned char *)name; *p; p++) h = (h ^ *p) * 16777619u;
   for (h &= mask; slot[h]; h = (h + 1) & mask) if (!strcmp(t->names[slot[h] - 1], name)) return t->names[slot[h] - 1];
   if (t->nNames + 1 > *cap) { *cap = *cap * 2 + 16; t->names = (char **)realloc(t->names, sizeof(char *) * (size_t)*cap); }
   t->names[t->nNames++] = strdup(name);
   slot[h] = t->nNames;
   return t->names[t->nNames - 1];
}

int htkamd_regtree_from_tables(int nNodes, const int *left, const int *right, const int *compOff, const char *const *compModel, const int *compState,
                               const int *compMix, htkamd_regtree **out)
{
   if (nNodes < 1 || !left || !right || !compOff || !out || compOff[0] != 0) { htkamd_set_error("regtree_from_tables: bad argument"); return HTKAMD_EINVAL; }
   unsigned char *isChild = (unsigned char *)calloc((size_t)nNodes + 1, 1);
   int bad = 0;
   for (int i = 0; i < nNodes && !bad; i++) {
      const int l = left[i], r = right[i];
      if (compOff[i + 1] < compOff[i]) bad = 1;
      if (l == 0 && r == 0) continue;
      if (l < 2 || r < 2 || l > nNodes || r > nNodes || l == r || l == i + 1 || r == i + 1 || isChild[l] || isChild[r] || compOff[i + 1] != compOff[i]) bad = 1;
      else isChild[l] = isChild[r] = 1;
   }
   for (int i = 2; i <= nNodes && !bad; i++) if (!isChild[i]) bad = 1;      /* every node but the root hangs under one parent */
   free(isChild);
   const int nComp = bad ? 0 : compOff[nNodes];
   if (bad || (nComp > 0 && (!compModel || !compState || !compMix))) { htkamd_set_error("regtree_from_tables: the tables do not describe a binary tree over %d nodes", nNodes); return HTKAMD_EINVAL; }
   htkamd_regtree *t = (htkamd_regtree *)calloc(1, sizeof(*t));
   t->nNodes = nNodes; t->nComp = nComp;
   t->left = (int *)malloc(sizeof(int) * (size_t)nNodes); t->right = (int *)malloc(sizeof(int) * (size_t)nNodes);
   t->compOff = (int *)malloc(sizeof(int) * ((size_t)nNodes + 1));
   memcpy(t->left, left, sizeof(int) * (size_t)nNodes); memcpy(t->right, right, sizeof(int) * (size_t)nNodes);
   memcpy(t->compOff, compOff, sizeof(int) * ((size_t)nNodes + 1));
   for (int i = 0; i < nNodes; i++) if (!left[i]) t->nTerm++;
   t->compModel = (char **)malloc(sizeof(char *) * (size_t)(nComp ? nComp : 1));
   t->compState = (int *)malloc(sizeof(int) * (size_t)(nComp ? nComp : 1)); t->compMix = (int *)malloc(sizeof(int) * (size_t)(nComp ? nComp : 1));
   int cap = 0;
   unsigned mask = 15;
   while (mask < 2u * (unsigned)nComp) mask = mask * 2 + 1;
   int *slot = (int *)calloc((size_t)mask + 1, sizeof(int));
   for (int c = 0; c < nComp; c++) {
      if (!compModel[c]) { free(slot); htkamd_regtree_destroy(t); htkamd_set_error("regtree_from_tables: component %d has no model name", c); return HTKAMD_EINVAL; }
      t->compModel[c] = (char *)rt_intern(t, compModel[c], &cap, slot, mask); t->compState[c] = compState[c]; t->compMix[c] = compMix[c];
   }
   free(slot);
   *out = t;
   return HTKAMD_OK;
}

void htkamd_regtree_destroy(htkamd_regtree *t)
{
   if (!t) return;
   for (int k = 0; k < t->nNames; k++) free(t->names[k]);
   free(t->names); free(t->left); free(t->right); free(t->compOff); free(t->compModel); free(t->compState); free(t->compMix); free(t->iters);
   free(t);
}

int htkamd_regtree_num_nodes(const htkamd_regtree *t) { return t ? t->nNodes : 0; }
int htkamd_regtree_num_terminals(const htkamd_regtree *t) { return t ? t->nTerm : 0; }

static int rt_node_ok(const htkamd_regtree *t, int node, const char *who)
{
   if (t && node >= 1 && node <= t->nNodes) return 1;
   htkamd_set_error("%s: node %d of %d", who, node, t ? t->nNodes : 0);
   return 0;
}

int htkamd_regtree_children(const htkamd_regtree *t, int node, int *left, int *right)
{
   if (!rt_node_ok(t, node, "regtree_children")) return HTKAMD_EINVAL;
   if (left) *left = t->left[node - 1];
   if (right) *right = t->right[node - 1];
   return HTKAMD_OK;
}

int htkamd_regtree_terminal_node(const htkamd_regtree *t, int baseClass)
{
   if (t) for (int i = 0, k = 0; i < t->nNodes; i++) if (!t->left[i] && ++k == baseClass) return i + 1;      /* the classes count the terminals in node order (:6054) */
   return 0;
}

int htkamd_regtree_num_components(const htkamd_regtree *t, int node)
{
   if (!rt_node_ok(t, node, "regtree_num_components")) return -1;
   return t->compOff[node] - t->compOff[node - 1];
}

const char *htkamd_regtree_component(const htkamd_regtree *t, int node, int i, int *state, int *mix)
{
   if (!rt_node_ok(t, node, "regtree_component")) return NULL;
   if (i < 0 || i >= t->compOff[node] - t->compOff[node - 1]) { htkamd_set_error("regtree_component: component %d of %d in node %d", i, t->compOff[node] - t->compOff[node - 1], node); return NULL; }
   const int c = t->compOff[node - 1] + i;
   if (state) *state = t->compState[c];
   if (mix) *mix = t->compMix[c];
   return t->compModel[c];
}

int htkamd_regtree_stats(const htkamd_regtree *t, int *iters, int cap, float *kernelMs)
{
   if (!t) return 0;
   if (iters) for (int k = 0; k < t->nSplits && k < cap; k++) iters[k] = t->iters[k];
   if (kernelMs) *kernelMs = t->kernelMs;
   return t->nSplits;
}

/* ------------------------------------------------------------------------------------------ the two files */
int htkamd_regtree_write(const htkamd_regtree *t, const char *identifier, const char *dir)
{
   if (!t || !identifier || !*identifier) { htkamd_set_error("regtree_write: bad argument"); return HTKAMD_EINVAL; }
   if (strpbrk(identifier, "/.") || strlen(identifier) > 200) {      /* MakeFN (HShell.c:1739) would take a path and an extension off it */
      htkamd_set_error("regtree_write: the identifier '%s' is not a plain name (no directory, no extension, at most 200 characters)", identifier); return HTKAMD_EINVAL;
   }
   const size_t np = (dir ? strlen(dir) : 0) + strlen(identifier) + 16;
   char *path = (char *)malloc(np), tname[256], bname[256], quoted[600];
   snprintf(tname, sizeof(tname), "%s.tree", identifier);
   snprintf(bname, sizeof(bname), "%s.base", identifier);
   const char *sep = (dir && *dir && dir[strlen(dir) - 1] != '/') ? "/" : "";
   int rc = HTKAMD_OK;
   /* PrintRegTree */
   snprintf(path, np, "%s%s%s", dir ? dir : "", sep, tname);
   FILE *f = fopen(path, "w");
   if (!f) { htkamd_set_error("regtree_write: cannot create output file %s", path); free(path); return HTKAMD_EIO; }
   htx_rewrite(tname, '"', quoted, sizeof(quoted));
   fprintf(f, "~r %s\n", quoted);
   htx_rewrite(bname, '"', quoted, sizeof(quoted));
   fprintf(f, "<BASECLASS>~b %s\n", quoted);
   for (int i = 1, nT = 0; i <= t->nNodes; i++) {
      if (t->left[i - 1]) fprintf(f, "<NODE> %d 2 %d %d \n", i, t->left[i - 1], t->right[i - 1]);
      else fprintf(f, "<TNODE> %d 1 %d\n", i, ++nT);              /* always one base class */
   }
   if (fclose(f)) { htkamd_set_error("regtree_write: writing %s failed", path); rc = HTKAMD_EIO; }
   /* PrintBaseClass */
   if (!rc) {
      snprintf(path, np, "%s%s%s", dir ? dir : "", sep, bname);
      f = fopen(path, "w");
      if (!f) { htkamd_set_error("regtree_write: cannot create output file %s", path); free(path); return HTKAMD_EIO; }
      fprintf(f, "~b %s\n", quoted);
      fprintf(f, "<MMFIDMASK> %s\n", "*");
      fprintf(f, "<PARAMETERS> MIXBASE\n");
      fprintf(f, "<NUMCLASSES> %d\n", t->nTerm);
      for (int i = 1, cls = 0; i <= t->nNodes; i++) {
         if (t->left[i - 1]) continue;
         fprintf(f, "<CLASS> %d {", ++cls);
         for (int c = t->compOff[i - 1]; c < t->compOff[i]; c++)
            fprintf(f, "%s%s.state[%d].mix[%d]", c != t->compOff[i - 1] ? "," : "", t->compModel[c], t->compState[c], t->compMix[c]);
         fprintf(f, "}\n");
      }
      if (fclose(f)) { htkamd_set_error("regtree_write: writing %s failed", path); rc = HTKAMD_EIO; }
   }
   free(path);
   return rc;
}

/* ------------------------------------------------------------------------------------------ RC's item list
 * "{ hname.state[i-j,..].mix , ... }": nonSp[state of the set] = 1 for every state an item names.  Only membership matters
 * (InitRegTree looks every stream up in the list), so the list's order is not kept.  *any: the list has an item. */
typedef struct { const char *p; } rt_src;
static void rt_skip(rt_src *r) { while (isspace((unsigned char)*r->p)) r->p++; }
static int rt_alpha(rt_src *r, char *out, int cap)      /* GetAlpha (HUtil.c:660) */
{
   htx_src src = {r->p, r->p + strlen(r->p), 0};
   const int got = htx_read_string(&src, 0, ".,)}", out, (size_t)cap);
   r->p = src.p;
   if (got == HTX_NONE) out[0] = 0;
   return got < 0 ? -1 : (int)strlen(out);
}
static int rt_key(rt_src *r, const char *want)
{
   char key[16]; int n = 0;
   rt_skip(r);
   while (isalpha((unsigned char)*r->p) && n < 15) key[n++] = (char)toupper((unsigned char)*r->p++);
   key[n] = 0;
   return !strcmp(key, want);
}

static int rt_parse_items(const struct htkamd_mmf *s, const char *text, unsigned char *nonSp, int *any)
{
   rt_src r = { text };
   int maxStates = 0, rc = HTKAMD_OK;
   for (int h = 0; h < s->nHm; h++) if (s->hm[h].N > maxStates) maxStates = s->hm[h].N;
   int *walk = tc_logical_walk(s);
   unsigned char *models = (unsigned char *)malloc((size_t)s->nHm + 1), *states = (unsigned char *)malloc((size_t)maxStates + 2);
   char buf[512];
#define RT_BAD(...) do { htkamd_set_error(__VA_ARGS__); rc = HTKAMD_EINVAL; goto done; } while (0)
   rt_skip(&r);
   if (*r.p != '{') RT_BAD("mmf_regtree: item list: { expected in \"%s\"", text);
   r.p++;
   for (;;) {
      memset(models, 0, (size_t)s->nHm + 1); memset(states, 0, (size_t)maxStates + 2);
      rt_skip(&r);
      const int paren = *r.p == '(';
      do {                                                                    /* PHName / PHIdent */
         if (paren || *r.p == ',') r.p++;
         rt_skip(&r);
         if (rt_alpha(&r, buf, sizeof(buf)) < 0) RT_BAD("mmf_regtree: item list: unterminated quote or over-long name in \"%s\"", text);
         if (!strpbrk(buf, "*?%")) { const int h = htkamd_mmf_find_logical(s, buf); if (h >= 0) models[h] = 1; }
         else for (int k = 0; k < s->nLog; k++) if (tc_match(s->logName[walk[k]], buf)) models[s->logPhys[walk[k]]] = 1;
         rt_skip(&r);
      } while (paren && *r.p == ',');
      if (paren) { if (*r.p != ')') RT_BAD("mmf_regtree: item list: ) expected in \"%s\"", text); r.p++; rt_skip(&r); }
      if (*r.p != '.') RT_BAD("mmf_regtree: item list \"%s\": a list of whole models ('h' items): RC takes the pdfs of states, hname.state[i-j].mix", text);
      r.p++;
      if (!rt_key(&r, "STATE")) RT_BAD("mmf_regtree: item list \"%s\": state expected (transP items are not pdfs)", text);
      rt_skip(&r);
      if (*r.p != '[') RT_BAD("mmf_regtree: item list: [ expected after state in \"%s\"", text);
      do {                                                                    /* PIndex / PIntRange */
         r.p++; rt_skip(&r);
         char *e; long i1 = strtol(r.p, &e, 10), i2;
         if (e == r.p) RT_BAD("mmf_regtree: item list: state index expected in \"%s\"", text);
         r.p = e; rt_skip(&r); i2 = i1;
         if (*r.p == '-') { r.p++; rt_skip(&r); i2 = strtol(r.p, &e, 10); if (e == r.p) RT_BAD("mmf_regtree: item list: state index expected in \"%s\"", text); r.p = e; rt_skip(&r); }
         if (i1 < 1 || i1 > maxStates || i2 < 1 || i2 > maxStates) RT_BAD("mmf_regtree: item list: state index out of range 1 .. %d in \"%s\"", maxStates, text);
         for (long i = i1; i <= i2; i++) states[i] = 1;
      } while (*r.p == ',');
      if (*r.p != ']') RT_BAD("mmf_regtree: item list: ] expected in \"%s\"", text);
      r.p++; rt_skip(&r);
      if (*r.p != '.') RT_BAD("mmf_regtree: item list \"%s\": whole states ('s' items): RC takes the pdfs of states, hname.state[i-j].mix", text);
      r.p++;
      if (!rt_key(&r, "MIX")) RT_BAD("mmf_regtree: item list \"%s\": only hname.state[i-j].mix is taken (the pdf of a one-stream state; no stream, dur or weights items)", text);
      rt_skip(&r);
      if (*r.p == '[') RT_BAD("mmf_regtree: item list \"%s\": mixture components ('m' items): RC takes whole pdfs, hname.state[i-j].mix", text);
      for (int h = 0; h < s->nHm; h++)
         if (models[h]) for (int j = 2; j < s->hm[h].N; j++) if (states[j]) { nonSp[s->hm[h].state[j - 1]] = 1; *any = 1; }
      if (*r.p == ',') { r.p++; continue; }
      if (*r.p != '}') RT_BAD("mmf_regtree: item list: } expected in \"%s\"", text);
      break;
   }
#undef RT_BAD
done:
   free(walk); free(models); free(states);
   return rc;
}

/* ------------------------------------------------------------------------------------------ the command */
typedef struct { int left, right, off, n; float score; float *dist; } rt_node;      /* dist: aveMean[D], aveCovar[D], clustAcc, clusterScore */

/* FindBestTerminal (:6073): the first terminal, children in order, whose score is above every one before it and that has the components */
static int rt_find_best(const rt_node *nd, int t, float *score, int D, int best)
{
   if (nd[t].left) {
      best = rt_find_best(nd, nd[t].left, score, D, best);
      best = rt_find_best(nd, nd[t].right, score, D, best);
   } else if (*score < nd[t].score && nd[t].n > D * 3) { *score = nd[t].score; best = t; }
   return best;
}

static void rt_perturb(const float *mean, const float *covar, float pertDepth, int D, float *out)      /* PerturbMean (:5850) on a copy */
{
   for (int k = 0; k < D; k++) { const float x = pertDepth * covar[k]; out[k] = mean[k] + x; }
}

int htkamd_mmf_regtree(htkamd_mmf *s, const float *occ, int nTerminals, const char *itemList, htkamd_regtree **out, void *stream)
{
   if (!s || !s->finished || !out) { htkamd_set_error("mmf_regtree: bad argument"); return HTKAMD_EINVAL; }
   if (!occ) { htkamd_set_error("mmf_regtree: building regression classes must load the stats file (no occupations given)"); return HTKAMD_EINVAL; }
   if (nTerminals < 0 || nTerminals > RT_MAXTERM) { htkamd_set_error("mmf_regtree: %d terminal nodes asked for (0 .. %d)", nTerminals, RT_MAXTERM); return HTKAMD_EINVAL; }
   if (s->nStreams > 1) { htkamd_set_error("mmf_regtree: a set with more than one stream (%d) is not supported", s->nStreams); return HTKAMD_EMODEL; }
   if (s->fullc) { htkamd_set_error("mmf_regtree: FULLC sets are not supported"); return HTKAMD_EMODEL; }
   if (s->tiedMix) { htkamd_set_error("mmf_regtree: tied-mixture sets are not supported"); return HTKAMD_EMODEL; }
   if (strstr(s->kind, "DISCRETE")) { htkamd_set_error("mmf_regtree: discrete sets are not supported"); return HTKAMD_EMODEL; }
   const int D = s->vecSize;
   if (D < 1 || D > HTKAMD_RT_MAXDIM) { htkamd_set_error("mmf_regtree: vector size %d (1 .. %d)", D, HTKAMD_RT_MAXDIM); return HTKAMD_EMODEL; }
   int rc = HTKAMD_OK, anyItem = 0;
   unsigned char *nonSp = (unsigned char *)calloc((size_t)s->nSt + 1, 1);
   if (itemList) { const char *p = itemList; while (isspace((unsigned char)*p)) p++; if (*p) rc = rt_parse_items(s, itemList, nonSp, &anyItem); }
   if (rc) { free(nonSp); return rc; }

   /* InitRegTree's scan */
   const int nG = s->nG, nHm = s->nHm;
   int *scan = (int *)malloc(sizeof(int) * (size_t)(nHm + 1));
   {
      const char **nm = (const char **)malloc(sizeof(char *) * (size_t)(nHm + 1));
      for (int k = 0; k < nHm; k++) nm[k] = s->hm[s->hmCreate ? s->hmCreate[k] : k].name;
      htkamd_hmm_scan_order(nm, nHm, scan);
      if (s->hmCreate) for (int k = 0; k < nHm; k++) scan[k] = s->hmCreate[scan[k]];
      free(nm);
   }
   unsigned char *seenSt = (unsigned char *)calloc((size_t)s->nSt + 1, 1), *seenG = (unsigned char *)calloc((size_t)nG + 1, 1), *hook = (unsigned char *)calloc((size_t)nG + 1, 1);
   float *accOcc = (float *)calloc((size_t)nG + 1, sizeof(float));
   float *accSum = (float *)calloc((size_t)(nG + 1) * D, sizeof(float)), *accSqr = (float *)calloc((size_t)(nG + 1) * D, sizeof(float));
   int *mG[2], *mH[2], *mJ[2], *mM[2], nM[2] = {0, 0};      /* [0] speech, [1] non-speech: Gaussian, model, state, mixture */
   for (int c = 0; c < 2; c++) { mG[c] = (int *)malloc(sizeof(int) * (size_t)(nG + 1)); mH[c] = (int *)malloc(sizeof(int) * (size_t)(nG + 1)); mJ[c] = (int *)malloc(sizeof(int) * (size_t)(nG + 1)); mM[c] = (int *)malloc(sizeof(int) * (size_t)(nG + 1)); }
   for (int pos = 0; pos < nHm; pos++) {
      const int h = scan[pos];
      for (int j = 2; j < s->hm[h].N; j++) {
         const int si = s->hm[h].state[j - 1];
         if (seenSt[si]) continue;
         seenSt[si] = 1;
         const mmf_state *st = &s->st[si];
         for (int m = 0; m < st->nMix; m++) {                                /* InitTreeAccs */
            const int g = s->cg[st->comp0 + m];
            float x = occ[si];
            if (!hook[g] && x > 0.0) {
               hook[g] = 1;
               x *= s->wt[st->comp0 + m];
               accOcc[g] = x;
               const float *mean = s->mean + (size_t)g * D, *var = s->var + (size_t)g * D;
               for (int k = 0; k < D; k++) { accSum[(size_t)g * D + k] = mean[k] * x; accSqr[(size_t)g * D + k] = (var[k] + mean[k] * mean[k]) * x; }
            }
         }
         const int c = anyItem && nonSp[si];
         for (int m = 0; m < st->nMix; m++) {
            const int g = s->cg[st->comp0 + m];
            if (seenG[g]) continue;
            seenG[g] = 1;
            mG[c][nM[c]] = g; mH[c][nM[c]] = h; mJ[c][nM[c]] = j; mM[c][nM[c]] = m + 1; nM[c]++;
         }
      }
   }
   const int G = nM[0] + nM[1], rootSplit = nM[1] > 0;
   float *mean = NULL, *sum = NULL, *sqr = NULL, *mocc = NULL, *seeds = NULL, *two = NULL;
   unsigned char *has = NULL;
   int *gOf = NULL, *hOf = NULL, *jOf = NULL, *mOf = NULL, *list = NULL, *iters = NULL, nSplits = 0, nNodes = 1;
   rt_node *nd = NULL;
   htkamd_rt_dev *dev = NULL;
   if (G < 1 || nM[0] < 1) { htkamd_set_error("mmf_regtree: %s", G < 1 ? "the set has no Gaussians" : "the item list names every Gaussian of the set: nothing is left for the speech node"); rc = HTKAMD_EMODEL; goto done; }
   if (anyItem && !rootSplit) { htkamd_set_error("mmf_regtree: the item list selects no Gaussian of the set"); rc = HTKAMD_EINVAL; goto done; }
   /* no split is asked for (RC 0 / 1, RC 2 behind a non-speech list): the tree is the scan's lists as they stand, and no figure of a node is needed */
   const int splits = (rootSplit ? 2 : 1) < nTerminals;
   if (splits && !htkamd_rt_dev_open) { htkamd_set_error("mmf_regtree: no HIP device: this build holds the host files only"); rc = HTKAMD_ENODEV; goto done; }
   /* the members: the non-speech list (node 2) first when there is one, then the speech list */
   gOf = (int *)malloc(sizeof(int) * (size_t)G); hOf = (int *)malloc(sizeof(int) * (size_t)G); jOf = (int *)malloc(sizeof(int) * (size_t)G); mOf = (int *)malloc(sizeof(int) * (size_t)G);
   for (int c = 1, i = 0; c >= 0; c--) for (int k = 0; k < nM[c]; k++, i++) { gOf[i] = mG[c][k]; hOf[i] = mH[c][k]; jOf[i] = mJ[c][k]; mOf[i] = mM[c][k]; }
   mean = (float *)malloc(sizeof(float) * (size_t)G * D); sum = (float *)malloc(sizeof(float) * (size_t)G * D); sqr = (float *)malloc(sizeof(float) * (size_t)G * D);
   mocc = (float *)malloc(sizeof(float) * (size_t)G); has = (unsigned char *)malloc((size_t)G);
   for (int i = 0; i < G; i++) {
      const int g = gOf[i];
      memcpy(mean + (size_t)i * D, s->mean + (size_t)g * D, sizeof(float) * (size_t)D);
      memcpy(sum + (size_t)i * D, accSum + (size_t)g * D, sizeof(float) * (size_t)D);
      memcpy(sqr + (size_t)i * D, accSqr + (size_t)g * D, sizeof(float) * (size_t)D);
      mocc[i] = accOcc[g]; has[i] = hook[g];
   }
   if (splits && (rc = htkamd_rt_dev_open(&dev, mean, sum, sqr, mocc, has, G, D, stream))) goto done;
   const int C = 2 * D + 2;
   nd = (rt_node *)calloc((size_t)2 * RT_MAXTERM + 8, sizeof(rt_node));
   iters = (int *)malloc(sizeof(int) * (RT_MAXTERM + 1));
   seeds = (float *)malloc(sizeof(float) * 2 * (size_t)D); two = (float *)malloc(sizeof(float) * 2 * (size_t)C);
   /* the root: node 1; with a non-speech list an empty node 1 over node 2 (non-speech) and node 3 (speech) */
   int index;
   if (rootSplit) {
      nd[1].left = 2; nd[1].right = 3;
      nd[2].off = 0; nd[2].n = nM[1]; nd[3].off = nM[1]; nd[3].n = nM[0];
      for (int i = 3; i >= 2 && !rc && splits; i--) {                         /* r1 (speech) before r2, as there */
         nd[i].dist = (float *)malloc(sizeof(float) * (size_t)C);
         rc = htkamd_rt_dev_node(dev, nd[i].off, nd[i].n, nd[i].dist);
         if (!rc) nd[i].score = nd[i].dist[2 * D + 1];
      }
      index = 4;
   } else {
      nd[1].off = 0; nd[1].n = G;
      if (splits) {
         nd[1].dist = (float *)malloc(sizeof(float) * (size_t)C);
         rc = htkamd_rt_dev_node(dev, 0, G, nd[1].dist);
         if (!rc) nd[1].score = nd[1].dist[2 * D + 1];
      }
      index = 2;
   }
   /* BuildRegClusters: k counts terminals; index is the next node number */
   for (int k = index / 2; !rc && k < nTerminals; k++) {
      float score = 0.0;
      const int t = rt_find_best(nd, 1, &score, D, 1);
      if ((k > 1 || score == 0.0) && t == 1) break;                           /* "No more nodes to split.." */
      rt_perturb(nd[t].dist, nd[t].dist + D, 0.2, D, seeds);
      rt_perturb(nd[t].dist, nd[t].dist + D, -0.2, D, seeds + D);
      int counts[3];
      if ((rc = htkamd_rt_dev_split(dev, nd[t].off, nd[t].n, seeds, counts, two))) break;
      iters[nSplits++] = counts[2];
      for (int c = 0; c < 2; c++) {
         rt_node *n = &nd[index];
         n->off = nd[t].off + (c ? counts[0] : 0); n->n = counts[c];
         n->dist = (float *)malloc(sizeof(float) * (size_t)C);
         memcpy(n->dist, two + (size_t)c * C, sizeof(float) * (size_t)C);
         n->score = n->dist[2 * D + 1];
         if (c) nd[t].right = index; else nd[t].left = index;
         index++;
      }
   }
   nNodes = index - 1;
   if (!rc) {
      list = (int *)malloc(sizeof(int) * (size_t)G);
      if (dev) rc = htkamd_rt_dev_list(dev, list); else for (int i = 0; i < G; i++) list[i] = i;
   }
   if (!rc) {
      int *left = (int *)malloc(sizeof(int) * (size_t)nNodes), *right = (int *)malloc(sizeof(int) * (size_t)nNodes), *compOff = (int *)malloc(sizeof(int) * ((size_t)nNodes + 1));
      const char **cm = (const char **)malloc(sizeof(char *) * (size_t)G);
      int *cs = (int *)malloc(sizeof(int) * (size_t)G), *cx = (int *)malloc(sizeof(int) * (size_t)G), nc = 0;
      compOff[0] = 0;
      for (int i = 1; i <= nNodes && !rc; i++) {
         left[i - 1] = nd[i].left; right[i - 1] = nd[i].right;
         if (!nd[i].left)
            for (int q = nd[i].off; q < nd[i].off + nd[i].n; q++) {
               const int m = list[q];
               if (m < 0 || m >= G || nc >= G) { htkamd_set_error("mmf_regtree: the member list came back with entry %d of %d", m, G); rc = HTKAMD_EHIP; break; }
               cm[nc] = s->hm[hOf[m]].name; cs[nc] = jOf[m]; cx[nc] = mOf[m]; nc++;
            }
         compOff[i] = nc;
      }
      if (!rc) rc = htkamd_regtree_from_tables(nNodes, left, right, compOff, cm, cs, cx, out);
      if (!rc) { (*out)->nSplits = nSplits; (*out)->iters = iters; iters = NULL; (*out)->kernelMs = dev ? htkamd_rt_dev_kernel_ms(dev) : 0.0f; }
      free(left); free(right); free(compOff); free(cm); free(cs); free(cx);
   }
done:
   if (dev) htkamd_rt_dev_close(dev);
   if (nd) for (int i = 0; i < 2 * RT_MAXTERM + 8; i++) free(nd[i].dist);
   free(nd); free(iters); free(seeds); free(two); free(list);
   free(gOf); free(hOf); free(jOf); free(mOf); free(mean); free(sum); free(sqr); free(mocc); free(has);
   for (int c = 0; c < 2; c++) { free(mG[c]); free(mH[c]); free(mJ[c]); free(mM[c]); }
   free(nonSp); free(scan); free(seenSt); free(seenG); free(hook); free(accOcc); free(accSum); free(accSqr);
   return rc;
}
