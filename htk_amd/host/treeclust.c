/* treeclust.c -- decision-tree state clustering: HHEd's RO / QS / TB / ST commands for state items of one-stream, single-Gaussian
 * DIAGC sets (the case ChkTreeObject, HHEd.c:2503, allows for states).  Restated from the reference:
 *   LoadStatsFile (HUtil.c:1291)      htkamd_stats_read_file: the HERest -s file, occupations kept as floats (si->hook)
 *   PItemList (HUtil.c:1100) with PItemSet :1067, PHName :1040, PHIdent :1001, PState :971, AddItem :519 (prepends)
 *                                     tc_parse_items: which states, and in which ORDER -- the order decides every float sum
 *   QuestionCommand (HHEd.c:5018), LoadQuestion :417, DoMatch (HShell.c:1806)
 *   BuildTree (HHEd.c:2961) with InitTreeAccs :2535, ValidProbNode :2671, AccSumProb :2574, ClusterLogL :2611, FindBestSplit :2768,
 *     SplitTreeNode :2723, MergeLeaves / MergeNode / MergeCost :2785-2868, TieLeafNodes :2871, TieState :1021, TypicalState :990
 *   ShowTreesCommand (HHEd.c:3263), DownTree :3252, ReWriteString (HShell.c:1303)
 *   (LoadTreesCommand, AddUnseenCommand and CompactCommand: treesynth.c)
 * The sums over a node's items are made on the device (csrc/treeclust.hip) in list order; every likelihood that decides something is
 * evaluated HERE, with the C library's log, from the device's sums (bit-equal to the reference's by construction).  All trees of a call
 * advance together: one batch of nodes per round. */
#include <ctype.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mmf_priv.h"
#include "htktext.h"

/* The device side is in the HIP part of the library.  The host files are also built on their own (the sanitizer build of
   tests/test_host_sanitizers.py): there the device entry points are absent, and a call that needs them says so. */
#pragma weak htkamd_tree_dev_open
#pragma weak htkamd_tree_dev_split
#pragma weak htkamd_tree_dev_totals
#pragma weak htkamd_tree_dev_block
#pragma weak htkamd_tree_dev_close
#pragma weak htkamd_dc_dev_run

#define GROW_INT(p, n, cap) do { if ((n) + 1 > (cap)) { (cap) = (cap) * 2 + 16; (p) = (int *)realloc((p), sizeof(int) * (size_t)(cap)); } } while (0)

/* ------------------------------------------------------------------------------------------ small helpers */
/* DoMatch / RMatch (HShell.c:1787-1816): '*' any run (also empty), '?' one character */
int tc_match(const char *s, const char *p)
{
   const char *star = NULL, *back = NULL;
   while (*s) {
      if (*p == '*') { star = p++; back = s; }
      else if (*p == '?' || *p == *s) { p++; s++; }
      else if (star) { p = star + 1; s = ++back; }
      else return 0;
   }
   while (*p == '*') p++;
   return *p == 0;
}

static int tc_has_wild(const char *p) { return strpbrk(p, "*?%") != NULL; }      /* PHIdent :1013 */

/* the logical names in the order PHIdent's walk over the macro table meets them (:1027): the hash order mmf.c writes macros in,
   over the list's names in list order ('l' macros are made in list order, MakeHMMSet HModel.c:3580) */
int *tc_logical_walk(const struct htkamd_mmf *s)
{
   int *order = (int *)malloc(sizeof(int) * (size_t)(s->nLog ? s->nLog : 1));
   if (!s->logCreate) { htkamd_hmm_scan_order((const char *const *)s->logName, s->nLog, order); return order; }
   const char **nm = (const char **)malloc(sizeof(char *) * (size_t)(s->nLog ? s->nLog : 1));      /* after AU / CO: the order the 'l' macros were re-made in */
   for (int k = 0; k < s->nLog; k++) nm[k] = s->logName[s->logCreate[k]];
   htkamd_hmm_scan_order(nm, s->nLog, order);
   for (int k = 0; k < s->nLog; k++) order[k] = s->logCreate[order[k]];
   free(nm);
   return order;
}

/* ------------------------------------------------------------------------------------------ stats file */
int htkamd_stats_read_file(const htkamd_mmf *s, const char *path, float *occ, int *count)
{
   if (!s || !s->finished || !path || !occ) { htkamd_set_error("stats_read_file: bad argument"); return HTKAMD_EINVAL; }
   FILE *f = fopen(path, "r");
   if (!f) { htkamd_set_error("stats_read_file: cannot open %s", path); return HTKAMD_EIO; }
   for (int i = 0; i < s->nSt; i++) occ[i] = 0.0f;
   if (count) for (int h = 0; h < s->nHm; h++) count[h] = 0;
   char *line = NULL; size_t cap = 0; int lnum = 0, rc = HTKAMD_OK;
   while (!rc && getline(&line, &cap, f) >= 0) {
      char *p = line, *e;
      while (isspace((unsigned char)*p)) p++;
      if (!*p) continue;
      lnum++;
      (void)strtol(p, &e, 10);
      if (e == p) { htkamd_set_error("stats_read_file: format error in file %s line %d", path, lnum); rc = HTKAMD_EIO; break; }
      p = e;
      while (isspace((unsigned char)*p)) p++;
      char name[1024];
      htx_src src = {p, p + strlen(p), 0};
      const int got1 = htx_read_string(&src, HTX_LINE, NULL, name, sizeof(name));
      if (got1 != HTX_GOT) { htkamd_set_error("stats_read_file: %s line %d: model name: %s", path, lnum, htx_result_text(got1)); rc = HTKAMD_EIO; break; }
      p = (char *)src.p;
      const long cnt = strtol(p, &e, 10);
      if (e == p) { htkamd_set_error("stats_read_file: format error in file %s line %d", path, lnum); rc = HTKAMD_EIO; break; }
      p = e;
      const int h = htkamd_mmf_find_logical(s, name);
      if (h < 0) { htkamd_set_error("stats_read_file: unknown model %s at line %d of %s", name, lnum, path); rc = HTKAMD_EMODEL; break; }
      const int N = s->hm[h].N;
      int got = 0;
      for (;;) {
         const float x = strtof(p, &e);
         if (e == p) break;
         if (got < N - 2) occ[s->hm[h].state[1 + got]] = x;
         got++; p = e;
      }
      while (isspace((unsigned char)*p)) p++;
      if (*p || got != N - 2) {
         htkamd_set_error("stats_read_file: %s line %d: %d occupation counts for model %s, which has %d emitting states", path, lnum, got, name, N - 2);
         rc = HTKAMD_EMODEL; break;
      }
      if (count) count[h] = (int)cnt;
   }
   free(line);
   fclose(f);
   return rc;
}

/* ------------------------------------------------------------------------------------------ item lists */
typedef struct { int phys, j; } tc_item;              /* model and HTK state number (2 .. N-1) */

typedef struct { const char *p; } tc_src;
static void tc_skip(tc_src *r) { while (isspace((unsigned char)*r->p)) r->p++; }
/* GetAlpha (HUtil.c:660): a name up to one of ".,)}" or white space, or quoted; < 0 when it cannot be read */
static int tc_alpha(tc_src *r, char *out, int cap)
{
   htx_src src = {r->p, r->p + strlen(r->p), 0};
   const int got = htx_read_string(&src, 0, ".,)}", out, (size_t)cap);
   r->p = src.p;
   if (got == HTX_NONE) out[0] = 0;
   return got < 0 ? -1 : (int)strlen(out);
}

/* PHIdent: the models one name or pattern selects, appended in walk order */
static void tc_ident(const struct htkamd_mmf *s, const int *walk, const char *pat, int **phys, int *n, int *cap)
{
   if (!tc_has_wild(pat)) {
      const int h = htkamd_mmf_find_logical(s, pat);
      if (h >= 0) { GROW_INT(*phys, *n, *cap); (*phys)[(*n)++] = h; }
      return;
   }
   for (int k = 0; k < s->nLog; k++)
      if (tc_match(s->logName[walk[k]], pat)) { GROW_INT(*phys, *n, *cap); (*phys)[(*n)++] = s->logPhys[walk[k]]; }
}

/* The items of "{ hname.state[i] , ... }" in the order of the reference's list.  A set's models are collected by prepending (PHIdent ->
   AddItem), PState walks that list and prepends again: within a set the items stand in walk order, and a later set stands BEFORE an
   earlier one.  Anything but single-index state items is refused. */
static int tc_parse_items_typed(const struct htkamd_mmf *s, const char *text, tc_item **out, int *nOut, char *type /* NULL: states only; else 's' or 't' comes back */)
{
   char seen = 0;
   tc_src r = { text };
   tc_item *items = NULL; int nI = 0;
   int *walk = tc_logical_walk(s);
   int rc = HTKAMD_OK;
   char buf[512];
#define TC_BAD(...) do { htkamd_set_error(__VA_ARGS__); rc = HTKAMD_EINVAL; goto done; } while (0)
   tc_skip(&r);
   if (*r.p != '{') TC_BAD("item list: { expected in \"%s\"", text);
   r.p++;
   for (;;) {
      int *phys = NULL, nP = 0, capP = 0;
      tc_skip(&r);
      if (*r.p == '(') {
         do {
            r.p++;
            if (tc_alpha(&r, buf, sizeof(buf)) < 0) { free(phys); TC_BAD("item list: unterminated quote or over-long name in \"%s\"", text); }
            tc_ident(s, walk, buf, &phys, &nP, &capP);
            tc_skip(&r);
         } while (*r.p == ',');
         if (*r.p != ')') { free(phys); TC_BAD("item list: ) expected in \"%s\"", text); }
         r.p++;
      } else {
         if (tc_alpha(&r, buf, sizeof(buf)) < 0) { free(phys); TC_BAD("item list: unterminated quote or over-long name in \"%s\"", text); }
         tc_ident(s, walk, buf, &phys, &nP, &capP);
      }
      tc_skip(&r);
      int j = 0;
      const char *why = NULL;
      if (*r.p != '.') why = "a list of whole models ('h' items): only state items are clustered";
      else {
         r.p++; tc_skip(&r);
         char key[16]; int n = 0;
         while (isalpha((unsigned char)*r.p) && n < 15) key[n++] = (char)toupper((unsigned char)*r.p++);
         key[n] = 0;
         if (type && !strcmp(key, "TRANSP")) {             /* AddTransP (HUtil.c:767): an item per model, j = 0 */
            if (seen == 's') why = "items of different types in one list";
            seen = 't';
         } else if (strcmp(key, "STATE")) why = "only .state[i] items are clustered (transP and the like are not)";
         else if (seen == 't') why = "items of different types in one list";
         else {
            seen = 's';
            tc_skip(&r);
            if (*r.p != '[') why = "[ expected after state";
            else {
               r.p++; tc_skip(&r);
               char *e; j = (int)strtol(r.p, &e, 10);
               if (e == r.p) why = "state index expected";
               else {
                  r.p = e; tc_skip(&r);
                  if (*r.p == '-' || *r.p == ',') why = "an index range: a tree clusters one state position, give a single state index";
                  else if (*r.p != ']') why = "] expected";
                  else {
                     r.p++; tc_skip(&r);
                     if (*r.p == '.') why = "items below the state (streams, mixtures, means, variances, durations, weights): only whole states are clustered";
                  }
               }
            }
         }
      }
      if (why) { free(phys); TC_BAD("item list \"%s\": %s", text, why); }
      /* this set's items go in front of the earlier sets' */
      int add = 0;
      for (int k = 0; k < nP; k++) if (seen == 't' || (j >= 2 && j < s->hm[phys[k]].N)) add++;
      tc_item *ni = (tc_item *)malloc(sizeof(tc_item) * (size_t)(nI + add + 1));
      int m = 0;
      for (int k = 0; k < nP; k++) if (seen == 't' || (j >= 2 && j < s->hm[phys[k]].N)) { ni[m].phys = phys[k]; ni[m].j = j; m++; }
      if (nI) memcpy(ni + m, items, sizeof(tc_item) * (size_t)nI);
      free(items); free(phys);
      items = ni; nI += add;
      tc_skip(&r);
      if (*r.p == ',') { r.p++; continue; }
      if (*r.p != '}') TC_BAD("item list: } expected in \"%s\"", text);
      break;
   }
done:
#undef TC_BAD
   free(walk);
   if (rc) { free(items); items = NULL; nI = 0; }
   *out = items; *nOut = nI;
   if (type) *type = seen;
   return rc;
}

static int tc_parse_items(const struct htkamd_mmf *s, const char *text, tc_item **out, int *nOut) { return tc_parse_items_typed(s, text, out, nOut, NULL); }

int htkamd_mmf_item_list(const htkamd_mmf *s, const char *itemList, int *phys, int *state, int cap, int *n)
{
   if (!s || !s->finished || !itemList || !n) { htkamd_set_error("mmf_item_list: bad argument"); return HTKAMD_EINVAL; }
   tc_item *it; int nI;
   const int rc = tc_parse_items(s, itemList, &it, &nI);
   if (rc) return rc;
   for (int i = 0; i < nI && i < cap; i++) { if (phys) phys[i] = it[i].phys; if (state) state[i] = it[i].j; }
   *n = nI;
   free(it);
   return HTKAMD_OK;
}

/* A question's answer per PHYSICAL model: TRUE when a logical name that stands for it matches one of the patterns -- the question's
   item list holds the models PHIdent finds under their logical names (parsePhysicalHMM is FALSE, HUtil.c:57), and BuildTree links
   items to questions through the model itself (owner->hook, HHEd.c:3020-3026). */
static int tc_answers(const struct htkamd_mmf *s, const htkamd_tree_question *q, unsigned char *ans)
{
   int any = 0;
   memset(ans, 0, (size_t)s->nHm);
   for (int k = 0; k < q->nPatterns; k++) {
      const char *pat = q->patterns[k];
      if (!tc_has_wild(pat)) { const int h = htkamd_mmf_find_logical(s, pat); if (h >= 0) { ans[h] = 1; any = 1; } continue; }
      for (int i = 0; i < s->nLog; i++) if (tc_match(s->logName[i], pat)) { ans[s->logPhys[i]] = 1; any = 1; }
   }
   return any;
}

int htkamd_mmf_question_answers(const htkamd_mmf *s, const htkamd_tree_question *q, unsigned char *answers)
{
   if (!s || !s->finished || !q || !q->name || !answers || q->nPatterns < 1 || !q->patterns) { htkamd_set_error("mmf_question_answers: bad argument"); return HTKAMD_EINVAL; }
   tc_answers(s, q, answers);
   return HTKAMD_OK;
}

/* ------------------------------------------------------------------------------------------ trees file */
int htkamd_trees_write(const char *path, const htkamd_tree_question *q, int nQ, const htkamd_tree_desc *t, int nT)
{
   if (!path || nQ < 0 || nT < 0 || (nQ && !q) || (nT && !t)) { htkamd_set_error("trees_write: bad argument"); return HTKAMD_EINVAL; }
   FILE *f = fopen(path, "w");
   if (!f) { htkamd_set_error("trees_write: cannot create %s", path); return HTKAMD_EIO; }
   for (int i = 0; i < nQ; i++) {                    /* LoadQuestion prepends the patterns (:453): they come out last first */
      fputs("QS ", f); htx_write_string(f, q[i].name, '\'', 0); fputc(' ', f);
      for (int k = q[i].nPatterns - 1; k >= 0; k--) { fputs(k == q[i].nPatterns - 1 ? "{ " : ",", f); htx_write_string(f, q[i].patterns[k], '"', 0); }
      fprintf(f, " }\n");
   }
   fprintf(f, "\n");
   for (int i = 0; i < nT; i++) {
      const htkamd_tree_desc *tr = &t[i];
      if (tr->state > 0) { htx_write_string(f, tr->name, HTX_ESCAPE, 0); fprintf(f, "[%d]\n", tr->state); } else fprintf(f, "%s\n", tr->name);
      if (tr->nNodes == 0) { fputs("   ", f); htx_write_string(f, tr->leafMacro[0], '"', 0); fputs("\n\n", f); continue; }
      fprintf(f, "{\n");
      for (int n = 0; n < tr->nNodes; n++) {
         fprintf(f, " %3d ", -n); htx_write_string(f, q[tr->quest[n]].name, '\'', 24); fputc(' ', f);
         for (int side = 0; side < 2; side++) {
            const int c = side ? tr->yes[n] : tr->no[n];
            if (c >= 0) fprintf(f, "  %5d    ", -c);
            else { fputc(' ', f); htx_write_string(f, tr->leafMacro[-1 - c], '"', 9); fputc(' ', f); }
         }
         fprintf(f, "\n");
      }
      fprintf(f, "}\n\n");
   }
   if (fclose(f)) { htkamd_set_error("trees_write: write error on %s", path); return HTKAMD_EIO; }
   return HTKAMD_OK;
}

/* ------------------------------------------------------------------------------------------ the trees */
typedef struct {
   int head;                     /* first cluster item (tree-local), -1: none */
   float occ, tProb, sProb;
   int quest, snum, parent, yes, no, next, prev, leafNo;
   float *tot;                   /* [C] the cluster's sums in list order */
} tc_node;

typedef struct {
   const htkamd_tree_spec *spec;
   tc_item *items; int nItems, base;      /* base: the first of its rows in the call's item table */
   int *cnext;                            /* cluster list links (CRec.next) */
   tc_node *nd; int nNd, capNd;
   int root, leaf, size, nClust;
   int pend[2], nPend;                    /* nodes waiting for ValidProbNode */
   int cursor;                            /* MergeLeaves' node */
   char name[256]; int state;
} tc_tree;

typedef struct { int C, D, nQ; float outlier; } tc_ctx;

static int tc_new_node(tc_tree *t, int head, int parent, int C)
{
   if (t->nNd + 1 > t->capNd) { t->capNd = t->capNd * 2 + 16; t->nd = (tc_node *)realloc(t->nd, sizeof(tc_node) * (size_t)t->capNd); }
   tc_node *n = &t->nd[t->nNd];
   memset(n, 0, sizeof(*n));
   n->head = head; n->parent = parent; n->yes = n->no = n->next = n->prev = -1; n->quest = -1; n->snum = -1; n->leafNo = -1;
   n->tot = (float *)calloc((size_t)C, sizeof(float));
   return t->nNd++;
}

/* AccSumProb (HHEd.c:2574): the variance in float, widened; the sum in double; returned as float */
static float tc_acc_prob(const float *a, int D)
{
   const float occ = a[0];
   double variance, prob = 0.0;
   if (occ > 0.0) {
      for (int k = 0; k < D; k++) {
         const float sum = a[1 + k], sqr = a[1 + D + k];
         variance = (sqr - (sum * sum / occ)) / occ;
         if (variance <= MINLARG) return LZERO;
         prob += -0.5 * occ * (1.0 + log(HTK_TPI * variance));
      }
   }
   return prob;
}

/* one question of ValidProbNode's loop (:2694-2709) */
static void tc_try_question(const tc_ctx *c, tc_node *n, int q, const float *no, const float *yes, float *best)
{
   float sProb = tc_acc_prob(no, c->D);
   sProb += tc_acc_prob(yes, c->D);
   if (n->occ <= 0.0 || (c->outlier >= 0.0 && (no[0] < c->outlier || yes[0] < c->outlier))) sProb = n->tProb;
   if (sProb > *best) { *best = sProb; n->quest = q; }
}

/* ValidProbNode from the node's record: the candidates in question order (every question from the node's block where they did not fit) */
static int tc_valid_prob_node(const tc_ctx *c, htkamd_tree_dev *dev, int slot, const int *rec, tc_node *n)
{
   const int C = c->C;
   const float *tot = (const float *)(rec + 1 + HTKAMD_TREE_MAXCAND), *cand = tot + C;
   memcpy(n->tot, tot, sizeof(float) * (size_t)C);
   n->tProb = tc_acc_prob(tot, c->D);
   n->occ = tot[0];
   n->quest = -1;
   float best = n->tProb;
   if (rec[0] > HTKAMD_TREE_MAXCAND) {
      float *blk = (float *)malloc(sizeof(float) * (size_t)(c->nQ + 1) * 2 * C);
      const int rc = htkamd_tree_dev_block(dev, slot, blk);
      if (rc) { free(blk); return rc; }
      for (int q = 0; q < c->nQ; q++) tc_try_question(c, n, q, blk + (size_t)q * 2 * C, blk + (size_t)q * 2 * C + C, &best);
      free(blk);
   } else
      for (int k = 0; k < rec[0]; k++) tc_try_question(c, n, rec[1 + k], cand + (size_t)k * 2 * C, cand + (size_t)k * 2 * C + C, &best);
   n->sProb = best;
   return HTKAMD_OK;
}

/* SplitTreeNode (:2723): the items go to the children by prepending (each child's list is reversed), yes before no in the leaf chain */
static void tc_split_node(tc_tree *t, int ni, const unsigned char *ans /* the question's answers per model */, int C)
{
   const int y = tc_new_node(t, -1, ni, C), o = tc_new_node(t, -1, ni, C);
   tc_node *n = &t->nd[ni], *ny = &t->nd[y], *no = &t->nd[o];
   for (int cl = n->head, nx; cl >= 0; cl = nx) {
      nx = t->cnext[cl];
      tc_node *to = ans[t->items[cl].phys] ? ny : no;
      t->cnext[cl] = to->head; to->head = cl;
   }
   n->head = -1; n->yes = y; n->no = o;
   ny->next = o; no->prev = y;
   no->next = n->next; ny->prev = n->prev;
   if (n->next >= 0) t->nd[n->next].prev = o;
   if (n->prev < 0) t->leaf = y; else t->nd[n->prev].next = y;
   t->nClust++;
}

/* FindBestSplit (:2768) */
static int tc_find_best_split(const tc_tree *t, float threshold)
{
   int best = -1; float imp = 0.0;
   for (int n = t->leaf; n >= 0; n = t->nd[n].next) {
      const float sProb = t->nd[n].sProb - t->nd[n].tProb;
      if (sProb > imp && sProb > threshold) { best = n; imp = sProb; }
   }
   return best;
}

static int tc_flatten(const tc_tree *t, int head, int *idx)
{
   int n = 0;
   for (int cl = head; cl >= 0; cl = t->cnext[cl]) idx[n++] = t->base + cl;
   return n;
}

static void tc_free_tree(tc_tree *t)
{
   for (int i = 0; i < t->nNd; i++) free(t->nd[i].tot);
   free(t->nd); free(t->items); free(t->cnext);
}

/* TieLeafNodes (:2871) + TieState (:1021) on the holder: the leaf's states become one ~s macro */
static void tc_tie_leaf(struct htkamd_mmf *s, tc_tree *t, tc_node *n, const char *macName, int leafStats, int vfSet, int *seq, int *newSeq)
{
   const int D = s->vecSize;
   /* ilist = the cluster list reversed (:2915-2922); TypicalState (:990): the first of the largest gConst, a dead weight costs 200 */
   int cnt = 0;
   for (int cl = n->head; cl >= 0; cl = t->cnext[cl]) cnt++;
   int *il = (int *)malloc(sizeof(int) * (size_t)cnt);
   { int k = cnt; for (int cl = n->head; cl >= 0; cl = t->cnext[cl]) il[--k] = cl; }
   float gmax = LZERO; int imax = -1;
   for (int k = 0; k < cnt; k++) {
      const tc_item *it = &t->items[il[k]];
      const int c = s->st[s->hm[it->phys].state[it->j - 1]].comp0;
      float gsum = 0;
      if (s->wt[c] > MINMIX) gsum += s->gconst[s->cg[c]]; else gsum -= 200.0;
      if (gsum > gmax) { gmax = gsum; imax = k; }
   }
   if (imax < 0) imax = 0;
   const int keep = s->hm[t->items[il[imax]].phys].state[t->items[il[imax]].j - 1];
   s->st[keep].name = strdup(macName);
   s->st[keep].src = 0;
   newSeq[keep] = (*seq)++;
   for (int k = 0; k < cnt; k++) { const tc_item *it = &t->items[il[k]]; s->hm[it->phys].state[it->j - 1] = keep; }
   if (leafStats) {                                  /* :2936-2951, in float as there */
      const int g = s->cg[s->st[keep].comp0];
      float *mean = s->mean + (size_t)g * D, *var = s->var + (size_t)g * D;
      const float *sum = n->tot + 1, *sqr = n->tot + 1 + D, occ = n->tot[0];
      for (int k = 0; k < D; k++) {
         mean[k] = sum[k] / occ;
         var[k] = sqr[k] / occ - mean[k] * mean[k];
         if (vfSet && var[k] < s->varFloor[k]) var[k] = s->varFloor[k];
      }
   }
   free(il);
}

/* The pools after the ties: states nobody uses any more go, the new ~s macros stand behind the older states in the order they were made
   (NewMacro's order decides their place in the saved file's hash chains), components and Gaussians follow their states. */
void tc_compact(struct htkamd_mmf *s, const int *newSeq, int nNew)
{
   const int D = s->vecSize, nSt0 = s->nSt;
   unsigned char *used = (unsigned char *)calloc((size_t)nSt0 + 1, 1);
   for (int h = 0; h < s->nHm; h++) for (int i = 1; i < s->hm[h].N - 1; i++) used[s->hm[h].state[i]] = 1;
   int *map = (int *)malloc(sizeof(int) * (size_t)(nSt0 + 1)), *byNew = (int *)malloc(sizeof(int) * (size_t)(nNew + 1));
   mmf_state *nst = (mmf_state *)malloc(sizeof(mmf_state) * (size_t)(nSt0 + 1));
   int n = 0;
   for (int i = 0; i < nSt0; i++) {
      map[i] = -1;
      if (newSeq[i] >= 0) { byNew[newSeq[i]] = i; continue; }
      if (used[i] || s->st[i].name) { map[i] = n; nst[n++] = s->st[i]; }
      else { free(s->st[i].sMix); free(s->st[i].sw); }
   }
   for (int k = 0; k < nNew; k++) { map[byNew[k]] = n; nst[n++] = s->st[byNew[k]]; }
   free(s->st); s->st = nst; s->nSt = n; s->capSt = nSt0 + 1;
   for (int h = 0; h < s->nHm; h++) for (int i = 1; i < s->hm[h].N - 1; i++) s->hm[h].state[i] = map[s->hm[h].state[i]];
   /* components in the new state order, Gaussians in their old order without the ones no component names any more */
   int nc = 0;
   for (int i = 0; i < s->nSt; i++) nc += s->st[i].nMix;
   float *nwt = (float *)malloc(sizeof(float) * (size_t)(nc + 1)); int *ncg = (int *)malloc(sizeof(int) * (size_t)(nc + 1));
   int *gmap = (int *)malloc(sizeof(int) * (size_t)(s->nG + 1));
   for (int g = 0; g < s->nG; g++) gmap[g] = (g < s->capGN && s->gName[g]) ? 0 : -1;
   for (int i = 0; i < s->nSt; i++) for (int m = 0; m < s->st[i].nMix; m++) gmap[s->cg[s->st[i].comp0 + m]] = 0;
   int ng = 0;
   for (int g = 0; g < s->nG; g++) {
      if (gmap[g] < 0) { if (g < s->capGN) { free(s->gName[g]); s->gName[g] = NULL; } continue; }
      const int d = ng++;
      gmap[g] = d;
      if (d == g) continue;
      memcpy(s->mean + (size_t)d * D, s->mean + (size_t)g * D, sizeof(float) * (size_t)D);
      memcpy(s->var + (size_t)d * D, s->var + (size_t)g * D, sizeof(float) * (size_t)D);
      s->gconst[d] = s->gconst[g]; s->hasG[d] = s->hasG[g];
      if (g < s->capGN) { s->gName[d] = s->gName[g]; s->gSrc[d] = s->gSrc[g]; s->gName[g] = NULL; }
      if (g < s->capMac) { s->gMeanMac[d] = s->gMeanMac[g]; s->gVarMac[d] = s->gVarMac[g]; }
      if (s->gStr) s->gStr[d] = s->gStr[g];
   }
   s->nG = ng;
   nc = 0;
   for (int i = 0; i < s->nSt; i++) {
      const int c0 = s->st[i].comp0;
      for (int m = 0; m < s->st[i].nMix; m++) { nwt[nc + m] = s->wt[c0 + m]; ncg[nc + m] = gmap[s->cg[c0 + m]]; }
      s->st[i].comp0 = nc; nc += s->st[i].nMix;
   }
   free(s->wt); free(s->cg);
   s->wt = nwt; s->cg = ncg; s->nComp = nc; s->capComp = nc + 1;
   /* the flat description (one stream) */
   s->stateCompOff = (int *)realloc(s->stateCompOff, sizeof(int) * ((size_t)s->nSt + 1));
   for (int i = 0; i < s->nSt; i++) s->stateCompOff[i] = s->st[i].comp0;
   s->stateCompOff[s->nSt] = s->nComp;
   int tot = 0;
   for (int h = 0; h < s->nHm; h++) for (int i = 1; i < s->hm[h].N - 1; i++) s->hmmState[tot++] = s->hm[h].state[i];
   htkamd_model_desc *d = &s->d;
   d->numStates = s->nSt; d->numComp = s->nComp; d->numGauss = s->nG;
   d->stateCompOff = s->stateCompOff; d->compWeight = s->wt; d->compGauss = s->cg; d->mean = s->mean; d->var = s->var; d->gconst = s->gconst;
   free(used); free(map); free(byNew); free(gmap);
}

int htkamd_mmf_tree_cluster(htkamd_mmf *s, const float *occ, float outlierThresh, const htkamd_tree_question *q, int nQ, const htkamd_tree_spec *specs, int nT,
                            int flags, const char *treesPath, void *stream)
{
   if (!s || !s->finished || nQ < 0 || nT < 1 || !specs || (nQ > 0 && !q)) { htkamd_set_error("mmf_tree_cluster: bad argument"); return HTKAMD_EINVAL; }
   if (!occ) { htkamd_set_error("mmf_tree_cluster: no stats loaded (the state occupations of an HERest -s file: htkamd_stats_read_file)"); return HTKAMD_EINVAL; }
   if (s->nStreams > 1) { htkamd_set_error("mmf_tree_cluster: a set with more than one stream (%d) is not supported", s->nStreams); return HTKAMD_EMODEL; }
   if (s->fullc) { htkamd_set_error("mmf_tree_cluster: FULLC sets are not supported (TB only valid for 1 mix diagonal covar models)"); return HTKAMD_EMODEL; }
   if (s->tiedMix) { htkamd_set_error("mmf_tree_cluster: tied-mixture sets are not supported"); return HTKAMD_EMODEL; }
   for (int i = 0; i < nQ; i++) {
      if (!q[i].name || q[i].nPatterns < 1 || !q[i].patterns) { htkamd_set_error("mmf_tree_cluster: question %d has no name or no pattern", i); return HTKAMD_EINVAL; }
      for (int k = 0; k < i; k++) if (!strcmp(q[i].name, q[k].name)) { htkamd_set_error("mmf_tree_cluster: question name %s invalid: defined twice", q[i].name); return HTKAMD_EINVAL; }
   }
   const int D = s->vecSize, C = 2 * D + 1, H = s->nHm;
   htkamd_set_error("%s", "");                                     /* (a warning of this call is found there afterwards) */
   int rc = HTKAMD_OK, nItems = 0, nKept = 0;
   char warn[512] = "";
   tc_tree *tr = (tc_tree *)calloc((size_t)nT, sizeof(tc_tree));
   htkamd_tree_question *kq = (htkamd_tree_question *)malloc(sizeof(htkamd_tree_question) * (size_t)(nQ + 1));
   unsigned char *ans = (unsigned char *)malloc((size_t)(nQ + 1) * (size_t)H);
   int *owner = (int *)malloc(sizeof(int) * (size_t)(s->nSt + 1));           /* the tree that took a state */
   float *stats = NULL; int *itemCol = NULL, *idx = NULL, *rec = NULL, *slotTree = NULL, *slotNode = NULL, *newSeq = NULL;
   htkamd_tree_node *batch = NULL; float *tots = NULL;
   htkamd_tree_dev *dev = NULL;
   for (int i = 0; i < s->nSt; i++) owner[i] = -1;
   /* QS: a question no model answers is dropped (QuestionCommand :5032) */
   for (int i = 0; i < nQ; i++) {
      if (tc_answers(s, &q[i], ans + (size_t)nKept * H)) kq[nKept++] = q[i];
      else snprintf(warn, sizeof(warn), "mmf_tree_cluster: warning: no items for question %s: dropped", q[i].name);
   }
   /* TB: the item lists */
   for (int t = 0; t < nT && !rc; t++) {
      tc_tree *T = &tr[t];
      T->spec = &specs[t];
      if (!specs[t].macRoot || !specs[t].itemList) { htkamd_set_error("mmf_tree_cluster: tree %d has no macro name or no item list", t); rc = HTKAMD_EINVAL; break; }
      if ((rc = tc_parse_items(s, specs[t].itemList, &T->items, &T->nItems))) break;
      if (T->nItems == 0) { htkamd_set_error("mmf_tree_cluster: no items to cluster for %s (%s)", specs[t].macRoot, specs[t].itemList); rc = HTKAMD_EINVAL; break; }
      T->base = nItems; nItems += T->nItems;
      for (int i = 0; i < T->nItems && !rc; i++) {
         const tc_item *it = &T->items[i];
         const int si = s->hm[it->phys].state[it->j - 1];
         const mmf_state *st = &s->st[si];
         const int g = s->cg[st->comp0];
         if (owner[si] >= 0) {
            htkamd_set_error("mmf_tree_cluster: state %d of model %s is selected twice (by %s and %s): trees must not overlap", it->j, s->hm[it->phys].name,
                             specs[owner[si]].macRoot, specs[t].macRoot); rc = HTKAMD_EINVAL;
         } else if (st->nMix != 1) {
            htkamd_set_error("mmf_tree_cluster: state %d of model %s has %d mixture components: TB only valid for 1 mix diagonal covar models", it->j, s->hm[it->phys].name, st->nMix); rc = HTKAMD_EMODEL;
         } else if (st->name) {
            htkamd_set_error("mmf_tree_cluster: state %d of model %s is the ~s macro %s already: tying tied states is not supported", it->j, s->hm[it->phys].name, st->name); rc = HTKAMD_EMODEL;
         } else if ((g < s->capGN && s->gName[g]) || (g < s->capMac && (s->gMeanMac[g] >= 0 || s->gVarMac[g] >= 0))) {
            htkamd_set_error("mmf_tree_cluster: state %d of model %s shares its pdf or its vectors (~m / ~u / ~v macros): not supported", it->j, s->hm[it->phys].name); rc = HTKAMD_EMODEL;
         }
         owner[si] = t;
      }
      if (rc) break;
      /* the tree's name: the first item's model without its contexts (TriStrip HLabel.c:1021; USEMODELNAME is T) */
      const char *nm = s->hm[T->items[0].phys].name, *p = strchr(nm, '-');
      snprintf(T->name, sizeof(T->name), "%s", p ? p + 1 : nm);
      char *plus = strrchr(T->name, '+');
      if (plus) *plus = 0;
      T->state = T->items[0].j;
   }
   if (rc) goto done;
   for (int g = 0; g < s->nG; g++) if (!s->hasG[g]) { htkamd_host_fix_diag_gconst(D, s->var + (size_t)g * D, s->gconst + g); s->hasG[g] = 1; }      /* CheckMix at load, HModel.c:206 */
   /* InitTreeAccs (:2535): a row per item, occ | sum[D] | sqr[D]; x = occupation * weight, float products, nothing fused */
   stats = (float *)calloc((size_t)nItems * C, sizeof(float));
   itemCol = (int *)malloc(sizeof(int) * (size_t)nItems);
   for (int t = 0; t < nT; t++)
      for (int i = 0; i < tr[t].nItems; i++) {
         const tc_item *it = &tr[t].items[i];
         const int si = s->hm[it->phys].state[it->j - 1], c = s->st[si].comp0, g = s->cg[c];
         float *row = stats + (size_t)(tr[t].base + i) * C, x = occ[si];
         itemCol[tr[t].base + i] = it->phys;
         if (!(x > 0.0)) continue;
         x *= s->wt[c];
         row[0] = x;
         for (int k = 0; k < D; k++) {
            const float m = s->mean[(size_t)g * D + k], v = s->var[(size_t)g * D + k];
            row[1 + k] = m * x;
            row[1 + D + k] = (v + m * m) * x;
         }
      }
   if (!htkamd_tree_dev_open) { htkamd_set_error("mmf_tree_cluster: no HIP device: this build holds the host files only"); rc = HTKAMD_ENODEV; goto done; }
   if ((rc = htkamd_tree_dev_open(&dev, stats, nItems, D, itemCol, ans, H, nKept, stream))) goto done;
   const tc_ctx ctx = { C, D, nKept, outlierThresh };
   idx = (int *)malloc(sizeof(int) * (size_t)nItems * 2 + 16);
   batch = (htkamd_tree_node *)malloc(sizeof(htkamd_tree_node) * ((size_t)nItems + 2 * (size_t)nT));
   slotTree = (int *)malloc(sizeof(int) * ((size_t)nItems + 2 * (size_t)nT)); slotNode = (int *)malloc(sizeof(int) * ((size_t)nItems + 2 * (size_t)nT));
   rec = (int *)malloc(sizeof(int) * (size_t)(2 * nT) * HTKAMD_TREE_REC(C));
   tots = (float *)malloc(sizeof(float) * (size_t)(nItems + 1) * C);
   /* the roots: one cluster per tree, built by prepending over the item list (:3006-3018) -- the list reversed */
   for (int t = 0; t < nT; t++) {
      tc_tree *T = &tr[t];
      T->cnext = (int *)malloc(sizeof(int) * (size_t)T->nItems);
      int head = -1;
      for (int i = 0; i < T->nItems; i++) { T->cnext[i] = head; head = i; }
      T->root = T->leaf = tc_new_node(T, head, -1, C);
      T->nClust = 1; T->pend[0] = T->root; T->nPend = 1;
   }
   /* splitting: every round evaluates the pending nodes of all trees in one batch, then each tree splits its best leaf */
   for (;;) {
      int nB = 0, nIdx = 0;
      for (int t = 0; t < nT; t++)
         for (int k = 0; k < tr[t].nPend; k++) {
            const int n = tc_flatten(&tr[t], tr[t].nd[tr[t].pend[k]].head, idx + nIdx);
            batch[nB].offA = nIdx; batch[nB].nA = n; batch[nB].offB = 0; batch[nB].nB = 0;
            slotTree[nB] = t; slotNode[nB] = tr[t].pend[k];
            nIdx += n; nB++;
         }
      if (!nB) break;
      if ((rc = htkamd_tree_dev_split(dev, batch, nB, idx, nIdx, outlierThresh, rec))) goto done;
      for (int b = 0; b < nB; b++)
         if ((rc = tc_valid_prob_node(&ctx, dev, b, rec + (size_t)b * HTKAMD_TREE_REC(C), &tr[slotTree[b]].nd[slotNode[b]]))) goto done;
      for (int t = 0; t < nT; t++) {
         tc_tree *T = &tr[t];
         if (!T->nPend) continue;
         T->nPend = 0;
         const int best = tc_find_best_split(T, T->spec->threshold);
         if (best < 0) continue;
         T->nd[best].snum = T->size++;
         tc_split_node(T, best, ans + (size_t)T->nd[best].quest * H, C);
         T->pend[0] = T->nd[best].yes; T->pend[1] = T->nd[best].no; T->nPend = 2;
      }
   }
   /* MergeLeaves (:2862): every round is one MergeNode step of every tree, all of its pairs "node + a later leaf" in one batch */
   if (flags & HTKAMD_TREE_MERGE) {
      for (int t = 0; t < nT; t++) tr[t].cursor = tr[t].leaf;
      for (;;) {
         int nB = 0, nIdx = 0;
         for (int t = 0; t < nT; t++) {
            tc_tree *T = &tr[t];
            if (T->cursor < 0) continue;
            const int offA = nIdx, nA = tc_flatten(T, T->nd[T->cursor].head, idx + nIdx);
            nIdx += nA;
            for (int p = T->nd[T->cursor].next; p >= 0; p = T->nd[p].next) {
               const int n = tc_flatten(T, T->nd[p].head, idx + nIdx);
               batch[nB].offA = offA; batch[nB].nA = nA; batch[nB].offB = nIdx; batch[nB].nB = n;
               slotTree[nB] = t; slotNode[nB] = p;
               nIdx += n; nB++;
            }
         }
         if (nB && (rc = htkamd_tree_dev_totals(dev, batch, nB, idx, nIdx, tots))) goto done;
         int live = 0;
         for (int t = 0, b = 0; t < nT; t++) {
            tc_tree *T = &tr[t];
            if (T->cursor < 0) continue;
            tc_node *a = &T->nd[T->cursor];
            const float threshold = T->spec->threshold;
            float minCost = threshold; int min = -1, minB = -1;
            for (; b < nB && slotTree[b] == t; b++) {                        /* MergeNode (:2798), MergeCost (:2785) */
               const float combProb = tc_acc_prob(tots + (size_t)b * C, D);
               const float cost = a->tProb + T->nd[slotNode[b]].tProb - combProb;
               if (cost < minCost) { minCost = cost; min = slotNode[b]; minB = b; }
            }
            if (minCost < threshold) {
               tc_node *m = &T->nd[min];
               int tail = a->head;
               while (T->cnext[tail] >= 0) tail = T->cnext[tail];
               T->cnext[tail] = m->head;
               a->tProb += m->tProb - minCost;
               a->occ += m->occ;
               memcpy(a->tot, tots + (size_t)minB * C, sizeof(float) * (size_t)C);
               tc_node *mp = &T->nd[m->parent];
               if (mp->yes == min) mp->yes = T->cursor; else if (mp->no == min) mp->no = T->cursor;
               if (m->prev >= 0) T->nd[m->prev].next = m->next;
               if (m->next >= 0) T->nd[m->next].prev = m->prev;
               T->nClust--;
            }
            T->cursor = a->next;
            if (T->cursor >= 0) live = 1;
         }
         if (!live) break;
      }
   }
   /* TieLeafNodes, tree after tree in the order of the call */
   {
      int vfSet = s->varFloor != NULL, seq = 0;
      if (vfSet) for (int k = 0; k < D; k++) if (s->varFloor[k] < 0.0) vfSet = 0;
      newSeq = (int *)malloc(sizeof(int) * (size_t)(s->nSt + 1));
      for (int i = 0; i < s->nSt; i++) newSeq[i] = -1;
      htkamd_tree_desc *td = (htkamd_tree_desc *)calloc((size_t)nT, sizeof(htkamd_tree_desc));
      for (int t = 0; t < nT; t++) {
         tc_tree *T = &tr[t];
         int clidx = T->nClust, k = 0;
         char **leafName = (char **)malloc(sizeof(char *) * (size_t)(T->nClust + 1));
         for (int n = T->leaf; n >= 0; n = T->nd[n].next, k++) {
            char buf[300];
            snprintf(buf, sizeof(buf), "%s%d", T->spec->macRoot, clidx--);
            leafName[k] = strdup(buf);
            T->nd[n].leafNo = k;
            tc_tie_leaf(s, T, &T->nd[n], buf, (flags & HTKAMD_TREE_LEAFSTATS) != 0, vfSet, &seq, newSeq);
         }
         int *quest = (int *)malloc(sizeof(int) * (size_t)(T->size + 1)), *no = (int *)malloc(sizeof(int) * (size_t)(T->size + 1)), *yes = (int *)malloc(sizeof(int) * (size_t)(T->size + 1));
         for (int n = 0; n < T->nNd; n++) {                                  /* DownTree (:3252): the split nodes by their numbers */
            const tc_node *nd = &T->nd[n];
            if (nd->snum < 0) continue;
            quest[nd->snum] = nd->quest;
            no[nd->snum] = T->nd[nd->no].yes >= 0 ? T->nd[nd->no].snum : -1 - T->nd[nd->no].leafNo;
            yes[nd->snum] = T->nd[nd->yes].yes >= 0 ? T->nd[nd->yes].snum : -1 - T->nd[nd->yes].leafNo;
         }
         td[t].name = T->name; td[t].state = T->state; td[t].nNodes = T->size; td[t].quest = quest; td[t].no = no; td[t].yes = yes;
         td[t].leafMacro = (const char *const *)leafName; td[t].nLeaves = T->nClust;
      }
      tc_compact(s, newSeq, seq);
      for (int g = 0; g < s->nG; g++) htkamd_host_fix_diag_gconst(D, s->var + (size_t)g * D, s->gconst + g);      /* FixAllGConsts before HHEd saves (:6469) */
      st_hold(s, kq, nKept, td, nT);                  /* treeList and the questions outlive the command (LT / AU / ST below) */
      if (treesPath) rc = htkamd_trees_write(treesPath, kq, nKept, td, nT);
      for (int t = 0; t < nT; t++) {
         for (int k = 0; k < td[t].nLeaves; k++) free((char *)td[t].leafMacro[k]);
         free((void *)td[t].leafMacro); free((void *)td[t].quest); free((void *)td[t].no); free((void *)td[t].yes);
      }
      free(td);
   }
done:
   if (dev) htkamd_tree_dev_close(dev);
   for (int t = 0; t < nT; t++) tc_free_tree(&tr[t]);
   free(tr); free(kq); free(ans); free(owner); free(stats); free(itemCol); free(idx); free(rec); free(slotTree); free(slotNode); free(newSeq); free(batch); free(tots);
   if (!rc && warn[0]) htkamd_set_error("%s", warn);
   return rc;
}

/* ------------------------------------------------------------------------------------------ data-driven clustering: TC / NC / TI
 * Restated from the reference: ClusterCommand (HHEd.c:4239), Clustering :2005 (BuildCVec :1901, SetIDist :1845, MergeGroups :1887, RemOutliers :1975),
 * TieCommand :4102, ApplyTie :1515, TieState :1021 with TypicalState :990, TieTrans :1049.  The distances and the merge loop run on the
 * device (csrc/datacluster.hip); the host resolves the item lists, replays the merge log into member chains and ties. */

/* TieState on the holder: the listed states (list order) become one ~s macro, the typical one is kept */
static void dc_tie_states(struct htkamd_mmf *s, const tc_item *il, int cnt, const char *macName, int *seq, int *newSeq)
{
   float gmax = LZERO; int imax = -1;
   for (int k = 0; k < cnt; k++) {
      const mmf_state *st = &s->st[s->hm[il[k].phys].state[il[k].j - 1]];
      float gsum = 0;
      for (int m = 0; m < st->nMix; m++)
         if (s->wt[st->comp0 + m] > MINMIX) gsum += s->gconst[s->cg[st->comp0 + m]]; else gsum -= 200.0;
      if (gsum > gmax) { gmax = gsum; imax = k; }
   }
   if (imax < 0) imax = 0;
   const int keep = s->hm[il[imax].phys].state[il[imax].j - 1];
   s->st[keep].name = strdup(macName);
   s->st[keep].src = 0;
   newSeq[keep] = (*seq)++;
   for (int k = 0; k < cnt; k++) s->hm[il[k].phys].state[il[k].j - 1] = keep;
}

void dc_fix_gconsts(struct htkamd_mmf *s)        /* FixAllGConsts (Clustering :2019, TieState :1027) */
{
   for (int g = 0; g < s->nG; g++) { htkamd_host_fix_diag_gconst(s->vecSize, s->var + (size_t)g * s->vecSize, s->gconst + g); s->hasG[g] = 1; }
   s->d.gconst = s->gconst;
}

static int dc_check_set(const struct htkamd_mmf *s, const char *who)
{
   if (s->nStreams > 1) { htkamd_set_error("%s: a set with more than one stream (%d) is not supported", who, s->nStreams); return HTKAMD_EMODEL; }
   if (s->fullc) { htkamd_set_error("%s: FULLC sets are not supported", who); return HTKAMD_EMODEL; }
   if (s->tiedMix) { htkamd_set_error("%s: tied-mixture sets are not supported (TDistance)", who); return HTKAMD_EMODEL; }
   if (strstr(s->kind, "DISCRETE")) { htkamd_set_error("%s: discrete sets are not supported (DDistance)", who); return HTKAMD_EMODEL; }
   return HTKAMD_OK;
}

static int dc_check_state_item(const struct htkamd_mmf *s, const tc_item *it, const char *who)
{
   const mmf_state *st = &s->st[s->hm[it->phys].state[it->j - 1]];
   if (st->name) {
      htkamd_set_error("%s: state %d of model %s is the ~s macro %s already: tying tied states is not supported", who, it->j, s->hm[it->phys].name, st->name);
      return HTKAMD_EMODEL;
   }
   for (int m = 0; m < st->nMix; m++) {
      const int g = s->cg[st->comp0 + m];
      if ((g < s->capGN && s->gName[g]) || (g < s->capMac && (s->gMeanMac[g] >= 0 || s->gVarMac[g] >= 0))) {
         htkamd_set_error("%s: state %d of model %s shares its pdf or its vectors (~m / ~u / ~v macros): not supported", who, it->j, s->hm[it->phys].name);
         return HTKAMD_EMODEL;
      }
   }
   return HTKAMD_OK;
}

static int dc_max_mixes(const struct htkamd_mmf *s)      /* MaxMixInSet */
{
   int mx = 0;
   for (int h = 0; h < s->nHm; h++) for (int i = 1; i < s->hm[h].N - 1; i++) if (s->st[s->hm[h].state[i]].nMix > mx) mx = s->st[s->hm[h].state[i]].nMix;
   return mx;
}

/* the device job of item lists over the set: Divergence rows for a single-Gaussian set, else the set and the items' states */
static int dc_run(struct htkamd_mmf *s, const tc_item *items, int nItems, const htkamd_dc_cmd *cmds, int nCmds, const float *occ, float outlierThresh, int noMerge,
                  float *idistOut, int *merges, int *nMerges, void *stream, const char *who)
{
   if (!htkamd_dc_dev_run) { htkamd_set_error("%s: no HIP device: this build holds the host files only", who); return HTKAMD_ENODEV; }
   const int D = s->vecSize, single = dc_max_mixes(s) == 1;
   htkamd_dc_job job;
   memset(&job, 0, sizeof(job));
   job.nCmds = nCmds; job.cmds = cmds; job.nItems = nItems; job.outlierThresh = outlierThresh; job.noMerge = noMerge;
   float *mean = NULL, *var = NULL, *iocc = NULL; int *ist = (int *)malloc(sizeof(int) * (size_t)nItems);
   for (int i = 0; i < nItems; i++) ist[i] = s->hm[items[i].phys].state[items[i].j - 1];
   if (single) {
      mean = (float *)malloc(sizeof(float) * (size_t)nItems * D); var = (float *)malloc(sizeof(float) * (size_t)nItems * D);
      for (int i = 0; i < nItems; i++) {
         const int g = s->cg[s->st[ist[i]].comp0];
         memcpy(mean + (size_t)i * D, s->mean + (size_t)g * D, sizeof(float) * (size_t)D);
         memcpy(var + (size_t)i * D, s->var + (size_t)g * D, sizeof(float) * (size_t)D);
      }
      job.mean = mean; job.var = var; job.V = D;
   } else { job.desc = &s->d; job.itemState = ist; }
   if (occ) {
      iocc = (float *)malloc(sizeof(float) * (size_t)nItems);
      for (int i = 0; i < nItems; i++) iocc[i] = occ[ist[i]];
      job.occ = iocc;
   }
   const int rc = htkamd_dc_dev_run(&job, idistOut, merges, nMerges, stream);
   free(mean); free(var); free(iocc); free(ist);
   return rc;
}

int htkamd_state_distances(htkamd_mmf *s, const char *items, float *dist, int cap, int *n, void *stream)
{
   if (!s || !s->finished || !items || !n) { htkamd_set_error("state_distances: bad argument"); return HTKAMD_EINVAL; }
   int rc = dc_check_set(s, "state_distances");
   if (rc) return rc;
   tc_item *it; int nI;
   if ((rc = tc_parse_items(s, items, &it, &nI))) return rc;
   *n = nI;
   if (!dist || nI == 0) { free(it); return HTKAMD_OK; }
   if ((long long)cap < (long long)nI * nI) { free(it); htkamd_set_error("state_distances: room for %d values, %d x %d needed", cap, nI, nI); return HTKAMD_EINVAL; }
   dc_fix_gconsts(s);
   const htkamd_dc_cmd cmd = { 0, nI, 1, 0.0f };
   rc = dc_run(s, it, nI, &cmd, 1, NULL, 0.0f, 1, dist, NULL, NULL, stream, "state_distances");
   free(it);
   return rc;
}

int htkamd_cluster_merges(const float *idist, int N, const float *occ, int numReq, float threshold, float outlierThresh, int *merges, int *nMerges)
{
   if (!idist || N < 1 || numReq < 1 || !merges || !nMerges) { htkamd_set_error("cluster_merges: bad argument"); return HTKAMD_EINVAL; }
   if (!htkamd_dc_dev_run) { htkamd_set_error("cluster_merges: no HIP device: this build holds the host files only"); return HTKAMD_ENODEV; }
   const htkamd_dc_cmd cmd = { 0, N, numReq, threshold };
   htkamd_dc_job job;
   memset(&job, 0, sizeof(job));
   job.nCmds = 1; job.cmds = &cmd; job.nItems = N; job.idist = idist; job.occ = occ; job.outlierThresh = outlierThresh;
   int *log = (int *)malloc(sizeof(int) * 2 * (size_t)N);
   const int rc = htkamd_dc_dev_run(&job, NULL, log, nMerges, NULL);
   if (!rc) memcpy(merges, log, sizeof(int) * 2 * (size_t)*nMerges);
   free(log);
   return rc;
}

int htkamd_mmf_data_cluster(htkamd_mmf *s, const float *occ, float outlierThresh, const htkamd_cluster_spec *specs, int nSpecs, int *numClusters, void *stream)
{
   if (!s || !s->finished || !specs || nSpecs < 1 || !numClusters) { htkamd_set_error("mmf_data_cluster: bad argument"); return HTKAMD_EINVAL; }
   int rc = dc_check_set(s, "mmf_data_cluster");
   if (rc) return rc;
   htkamd_set_error("%s", "");
   char warn[512] = "";
   tc_item *items = NULL; int nItems = 0, nCmds = 0;
   htkamd_dc_cmd *cmds = (htkamd_dc_cmd *)malloc(sizeof(htkamd_dc_cmd) * (size_t)nSpecs);
   int *cmdSpec = (int *)malloc(sizeof(int) * (size_t)nSpecs);
   int *owner = (int *)malloc(sizeof(int) * (size_t)(s->nSt + 1));
   int *merges = NULL, *nMerges = NULL, *newSeq = NULL, *next = NULL, *cvec = NULL;
   for (int i = 0; i < s->nSt; i++) owner[i] = -1;
   for (int t = 0; t < nSpecs && !rc; t++) {
      const htkamd_cluster_spec *sp = &specs[t];
      numClusters[t] = 0;
      if (!sp->macro || !sp->items) { htkamd_set_error("mmf_data_cluster: command %d has no macro name or no item list", t); rc = HTKAMD_EINVAL; break; }
      if (strlen(sp->macro) > 20) { htkamd_set_error("mmf_data_cluster: %s is rather long for a macro name (over 20 characters)", sp->macro); rc = HTKAMD_EINVAL; break; }
      if (sp->byCount ? !(sp->value >= 1.0f) : !(sp->value >= 0.0f)) { htkamd_set_error("mmf_data_cluster: command %d (%s): bad %s %g", t, sp->macro, sp->byCount ? "cluster count" : "threshold", sp->value); rc = HTKAMD_EINVAL; break; }
      tc_item *it; int nI;
      if ((rc = tc_parse_items(s, sp->items, &it, &nI))) break;
      if (nI == 0) { snprintf(warn, sizeof(warn), "mmf_data_cluster: warning: no items to cluster for %s: skipped", sp->macro); free(it); continue; }
      if (nI > HTKAMD_DC_MAXITEMS) { htkamd_set_error("mmf_data_cluster: %d items for %s (at most %d in one command)", nI, sp->macro, HTKAMD_DC_MAXITEMS); rc = HTKAMD_EINVAL; free(it); break; }
      for (int i = 0; i < nI && !rc; i++) {
         const int si = s->hm[it[i].phys].state[it[i].j - 1];
         if (owner[si] >= 0) {
            htkamd_set_error("mmf_data_cluster: state %d of model %s is selected twice (by %s and %s): commands must not overlap", it[i].j, s->hm[it[i].phys].name,
                             specs[owner[si]].macro, sp->macro); rc = HTKAMD_EINVAL;
         } else rc = dc_check_state_item(s, &it[i], "mmf_data_cluster");
         owner[si] = t;
      }
      if (rc) { free(it); break; }
      items = (tc_item *)realloc(items, sizeof(tc_item) * (size_t)(nItems + nI));
      memcpy(items + nItems, it, sizeof(tc_item) * (size_t)nI);
      free(it);
      cmds[nCmds].off = nItems; cmds[nCmds].n = nI;
      cmds[nCmds].numReq = sp->byCount ? (int)sp->value : 1;
      cmds[nCmds].threshold = sp->byCount ? 1.0E15f : sp->value;
      cmdSpec[nCmds++] = t;
      nItems += nI;
   }
   if (rc || !nCmds) goto done;
   dc_fix_gconsts(s);
   merges = (int *)malloc(sizeof(int) * 2 * (size_t)nItems); nMerges = (int *)malloc(sizeof(int) * (size_t)nCmds);
   if ((rc = dc_run(s, items, nItems, cmds, nCmds, occ, outlierThresh, 0, NULL, merges, nMerges, stream, "mmf_data_cluster"))) goto done;
   {
      int seq = 0, maxN = 0;
      for (int c = 0; c < nCmds; c++) if (cmds[c].n > maxN) maxN = cmds[c].n;
      newSeq = (int *)malloc(sizeof(int) * (size_t)(s->nSt + 1));
      for (int i = 0; i < s->nSt; i++) newSeq[i] = -1;
      next = (int *)malloc(sizeof(int) * (size_t)maxN); cvec = (int *)malloc(sizeof(int) * (size_t)maxN);
      tc_item *il = (tc_item *)malloc(sizeof(tc_item) * (size_t)maxN);
      for (int c = 0; c < nCmds && !rc; c++) {
         const int n = cmds[c].n; int nc = n;
         const int *log = merges + 2 * (size_t)cmds[c].off;
         for (int i = 0; i < n; i++) { next[i] = -1; cvec[i] = i; }
         for (int m = 0; m < nMerges[c]; m++) {                /* MergeGroups (:1887) */
            const int i = log[2 * m] - 1, j = log[2 * m + 1] - 1;
            if (i < 0 || j < 0 || i >= nc || j >= nc || i == j) { htkamd_set_error("mmf_data_cluster: merge %d of %s names groups %d and %d of %d", m, specs[cmdSpec[c]].macro, i + 1, j + 1, nc); rc = HTKAMD_EHIP; break; }
            int p = cvec[i];
            while (next[p] >= 0) p = next[p];
            next[p] = cvec[j];
            for (int k = j; k < nc - 1; k++) cvec[k] = cvec[k + 1];
            nc--;
         }
         if (rc) break;
         numClusters[cmdSpec[c]] = nc;
         for (int k = 0; k < nc; k++) {                       /* the chain reversed (:2068), then ApplyTie */
            int cnt = 0;
            for (int p = cvec[k]; p >= 0; p = next[p]) cnt++;
            int w = cnt;
            for (int p = cvec[k]; p >= 0; p = next[p]) il[--w] = items[cmds[c].off + p];
            char buf[64];
            snprintf(buf, sizeof(buf), "%s%d", specs[cmdSpec[c]].macro, k + 1);
            dc_tie_states(s, il, cnt, buf, &seq, newSeq);
         }
      }
      free(il);
      if (!rc) tc_compact(s, newSeq, seq);
   }
done:
   free(items); free(cmds); free(cmdSpec); free(owner); free(merges); free(nMerges); free(newSeq); free(next); free(cvec);
   if (!rc && warn[0]) htkamd_set_error("%s", warn);
   return rc;
}

int htkamd_mmf_tie(htkamd_mmf *s, const char *macro, const char *items)
{
   if (!s || !s->finished || !macro || !items) { htkamd_set_error("mmf_tie: bad argument"); return HTKAMD_EINVAL; }
   if (strlen(macro) > 20) { htkamd_set_error("mmf_tie: %s is rather long for a macro name (over 20 characters)", macro); return HTKAMD_EINVAL; }
   tc_item *it; int nI; char type = 0;
   int rc = tc_parse_items_typed(s, items, &it, &nI, &type);
   if (rc) return rc;
   htkamd_set_error("%s", "");
   if (nI == 0) { free(it); htkamd_set_error("mmf_tie: warning: macro %s has nothing to tie", macro); return HTKAMD_OK; }      /* ApplyTie's -2631 */
   if (type == 't') {                                   /* TieTrans: the first item's matrix */
      const int t0 = s->hm[it[0].phys].trans;
      if (s->tr[t0].name) { htkamd_set_error("mmf_tie: the transition matrix of model %s is the ~t macro %s already: tying tied matrices is not supported", s->hm[it[0].phys].name, s->tr[t0].name); free(it); return HTKAMD_EMODEL; }
      for (int t = 0; t < s->nTr; t++) if (s->tr[t].name && !strcmp(s->tr[t].name, macro)) { htkamd_set_error("mmf_tie: ~t macro %s exists already", macro); free(it); return HTKAMD_EINVAL; }
      for (int k = 0; k < nI; k++) if (s->hm[it[k].phys].N != s->hm[it[0].phys].N) {
         htkamd_set_error("mmf_tie: model %s has %d states, %s has %d: their transition matrices cannot be tied", s->hm[it[k].phys].name, s->hm[it[k].phys].N, s->hm[it[0].phys].name, s->hm[it[0].phys].N);
         free(it); return HTKAMD_EMODEL;
      }
      /* the macro is a new record behind the others (NewMacro's order decides its place in the saved file), with the matrix's values */
      const int N = s->tr[t0].N, t1 = s->nTr;
      s->tr = (mmf_trans *)realloc(s->tr, sizeof(mmf_trans) * (size_t)(s->nTr + 1)); s->capTr = s->nTr + 1;
      s->tp = (float *)realloc(s->tp, sizeof(float) * (size_t)(s->nTp + N * N)); s->capTp = s->nTp + N * N;
      memcpy(s->tp + s->nTp, s->tp + s->tr[t0].off, sizeof(float) * (size_t)N * N);
      s->tr[t1].name = strdup(macro); s->tr[t1].N = N; s->tr[t1].off = s->nTp; s->tr[t1].src = 0;
      s->nTp += N * N; s->nTr++;
      for (int h = 0; h < s->nHm; h++) if (s->hm[h].trans == t0) s->hm[h].trans = t1;
      for (int k = 0; k < nI; k++) s->hm[it[k].phys].trans = t1;
      s->transN = (int *)realloc(s->transN, sizeof(int) * (size_t)s->nTr);
      s->transOff = (int *)realloc(s->transOff, sizeof(int) * ((size_t)s->nTr + 1));
      for (int t = 0; t < s->nTr; t++) { s->transN[t] = s->tr[t].N; s->transOff[t] = s->tr[t].off; }
      s->transOff[s->nTr] = s->nTp;
      for (int h = 0; h < s->nHm; h++) s->hmmTrans[h] = s->hm[h].trans;
      s->d.numTrans = s->nTr; s->d.transN = s->transN; s->d.transOff = s->transOff; s->d.transP = s->tp;
      free(it);
      return HTKAMD_OK;
   }
   if ((rc = dc_check_set(s, "mmf_tie"))) { free(it); return rc; }
   for (int i = 0; i < nI && !rc; i++) {
      rc = dc_check_state_item(s, &it[i], "mmf_tie");
      for (int k = 0; k < i && !rc; k++)
         if (s->hm[it[k].phys].state[it[k].j - 1] == s->hm[it[i].phys].state[it[i].j - 1]) {
            htkamd_set_error("mmf_tie: state %d of model %s is selected twice", it[i].j, s->hm[it[i].phys].name); rc = HTKAMD_EINVAL;
         }
   }
   for (int i = 0; i < s->nSt && !rc; i++) if (s->st[i].name && !strcmp(s->st[i].name, macro)) { htkamd_set_error("mmf_tie: ~s macro %s exists already", macro); rc = HTKAMD_EINVAL; }
   if (rc) { free(it); return rc; }
   dc_fix_gconsts(s);
   int seq = 0, *newSeq = (int *)malloc(sizeof(int) * (size_t)(s->nSt + 1));
   for (int i = 0; i < s->nSt; i++) newSeq[i] = -1;
   dc_tie_states(s, it, nI, macro, &seq, newSeq);
   tc_compact(s, newSeq, seq);
   free(newSeq); free(it);
   return HTKAMD_OK;
}
