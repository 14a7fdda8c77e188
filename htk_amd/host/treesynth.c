/* treesynth.c -- unseen triphones from the trees and the compacted set: HHEd's LT / AU / CO commands, and ST for the trees a holder keeps.
 * Restated from the reference:
 *   LoadTreesCommand (HHEd.c:3433), LoadQuestion :417 with ParseAlpha :381, LoadTree :3346 with GetNode :3327, ReadString (HShell.c:1242)
 *   AddUnseenCommand (HHEd.c:5082), TreeFilter :3219, SynthModel :3180, AssignStructure :3115, FindProtoModel :3160, SwapLists :3497,
 *     TriStrip (HLabel.c:1021), MakeHMMSet (HModel.c:4320), NewMacro :3324 (head insertion), DeleteMacro :3395 (the entry stays, typed '*')
 *   CompactCommand (HHEd.c:4340), EquivHMM :685, EquivState :670, EquivStream :650, EquivMix :642, SaveHMMList (HModel.c:5029)
 * The wildcard matching of the new names against the trees' questions and the walks down the trees run on the device
 * (csrc/treesynth.hip); this file reads the files, resolves base phones to trees and protos, wires the new models and keeps the order of
 * the reference's macro table, which decides the order of everything HHEd writes afterwards. */
#include <ctype.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mmf_priv.h"
#include "htktext.h"

/* the device side is absent from a build of the host files alone (treeclust.c) */
#pragma weak htkamd_synth_dev_run

/* ------------------------------------------------------------------------------------------ the held trees */
static int ts_find_quest(const mmf_trees *T, const char *name)
{
   for (int i = 0; i < T->nQ; i++) if (!strcmp(T->q[i].name, name)) return i;
   return -1;
}

static int ts_add_quest(mmf_trees *T, const char *name, const char *const *pat, int nPat)
{
   T->q = (mmf_quest *)realloc(T->q, sizeof(mmf_quest) * (size_t)(T->nQ + 1));
   mmf_quest *q = &T->q[T->nQ];
   q->name = strdup(name); q->nPat = nPat; q->pat = (char **)malloc(sizeof(char *) * (size_t)(nPat ? nPat : 1));
   for (int k = 0; k < nPat; k++) q->pat[k] = strdup(pat[k]);
   return T->nQ++;
}

static void ts_add_tree(mmf_trees *T, const htkamd_tree_desc *d, const int *qmap)
{
   T->t = (mmf_tree *)realloc(T->t, sizeof(mmf_tree) * (size_t)(T->nT + 1));
   mmf_tree *t = &T->t[T->nT++];
   const int n = d->nNodes;
   t->name = strdup(d->name); t->state = d->state; t->nNodes = n; t->nLeaves = d->nLeaves;
   t->quest = (int *)malloc(sizeof(int) * (size_t)(n + 1)); t->no = (int *)malloc(sizeof(int) * (size_t)(n + 1)); t->yes = (int *)malloc(sizeof(int) * (size_t)(n + 1));
   for (int k = 0; k < n; k++) { t->quest[k] = qmap ? qmap[d->quest[k]] : d->quest[k]; t->no[k] = d->no[k]; t->yes[k] = d->yes[k]; }
   t->leaf = (char **)malloc(sizeof(char *) * (size_t)(d->nLeaves + 1));
   for (int k = 0; k < d->nLeaves; k++) t->leaf[k] = strdup(d->leafMacro[k]);
}

/* TB's questions and trees join the ones the holder has (a question it has already is the same question: every call passes the script's
   whole list) */
void st_hold(struct htkamd_mmf *s, const htkamd_tree_question *q, int nQ, const htkamd_tree_desc *t, int nT)
{
   if (!s->trees) s->trees = (mmf_trees *)calloc(1, sizeof(mmf_trees));
   int *qmap = (int *)malloc(sizeof(int) * (size_t)(nQ + 1));
   for (int i = 0; i < nQ; i++) {
      qmap[i] = ts_find_quest(s->trees, q[i].name);
      if (qmap[i] < 0) qmap[i] = ts_add_quest(s->trees, q[i].name, q[i].patterns, q[i].nPatterns);
   }
   for (int i = 0; i < nT; i++) ts_add_tree(s->trees, &t[i], qmap);
   free(qmap);
}

int htkamd_mmf_num_trees(const htkamd_mmf *s) { return (s && s->trees) ? s->trees->nT : 0; }

const char *htkamd_mmf_tree_info(const htkamd_mmf *s, int t, int *state, int *nNodes, int *nLeaves)
{
   if (!s || !s->trees || t < 0 || t >= s->trees->nT) return NULL;
   const mmf_tree *tr = &s->trees->t[t];
   if (state) *state = tr->state;
   if (nNodes) *nNodes = tr->nNodes;
   if (nLeaves) *nLeaves = tr->nLeaves;
   return tr->name;
}

const char *htkamd_mmf_tree_leaf(const htkamd_mmf *s, int t, int leaf)
{
   if (!s || !s->trees || t < 0 || t >= s->trees->nT || leaf < 0 || leaf >= s->trees->t[t].nLeaves) return NULL;
   return s->trees->t[t].leaf[leaf];
}

const char *htkamd_mmf_state_macro(const htkamd_mmf *s, int state) { return (s && state >= 0 && state < s->nSt) ? s->st[state].name : NULL; }

int htkamd_mmf_save_trees(const htkamd_mmf *s, const char *path)
{
   if (!s || !s->finished || !path) { htkamd_set_error("mmf_save_trees: bad argument"); return HTKAMD_EINVAL; }
   if (!s->trees || !s->trees->nT) { htkamd_set_error("mmf_save_trees: no trees are held (TB builds them, LT loads them)"); return HTKAMD_EINVAL; }
   const mmf_trees *T = s->trees;
   htkamd_tree_question *q = (htkamd_tree_question *)calloc((size_t)T->nQ + 1, sizeof(htkamd_tree_question));
   htkamd_tree_desc *t = (htkamd_tree_desc *)calloc((size_t)T->nT + 1, sizeof(htkamd_tree_desc));
   for (int i = 0; i < T->nQ; i++) { q[i].name = T->q[i].name; q[i].patterns = (const char *const *)T->q[i].pat; q[i].nPatterns = T->q[i].nPat; }
   for (int i = 0; i < T->nT; i++) {
      const mmf_tree *m = &T->t[i];
      t[i].name = m->name; t[i].state = m->state; t[i].nNodes = m->nNodes; t[i].quest = m->quest; t[i].no = m->no; t[i].yes = m->yes;
      t[i].leafMacro = (const char *const *)m->leaf; t[i].nLeaves = m->nLeaves;
   }
   const int rc = htkamd_trees_write(path, q, T->nQ, t, T->nT);
   free(q); free(t);
   return rc;
}

/* ------------------------------------------------------------------------------------------ LT */
typedef htx_src ts_src;

/* ReadString: 1, 0 at the end of the text, -1 when a quote is left open or the string does not fit */
static int ts_string(ts_src *r, char *out, int cap)
{
   const int got = htx_read_string(r, 0, NULL, out, (size_t)cap);
   return got < 0 ? -1 : got;
}

typedef struct { int num, quest, kid[2]; } ts_line;      /* kid: >= 0 a node number, < 0 the leaf -1-k */

static int ts_cmp_state_name(const void *a, const void *b) { return strcmp(*(char *const *)a, *(char *const *)b); }

int htkamd_mmf_load_trees(htkamd_mmf *s, const char *path)
{
   if (!s || !s->finished || !path) { htkamd_set_error("mmf_load_trees: bad argument"); return HTKAMD_EINVAL; }
   size_t len; int why;
   char *text = htx_read_file(path, &len, &why);
   if (!text) { htkamd_set_error(why == HTX_ENOMEM ? "mmf_load_trees: out of memory reading %s" : "mmf_load_trees: cannot open file %s", path); return why == HTX_ENOMEM ? HTKAMD_ENOMEM : HTKAMD_EIO; }
   mmf_trees *N = (mmf_trees *)calloc(1, sizeof(mmf_trees));      /* what the file holds; joins the held trees only when all of it is good */
   const mmf_trees *H = s->trees;
   const int nHeldQ = H ? H->nQ : 0;
   char **stName = (char **)malloc(sizeof(char *) * (size_t)(s->nSt + 1)); int nStName = 0;
   for (int i = 0; i < s->nSt; i++) if (s->st[i].name) stName[nStName++] = s->st[i].name;
   qsort(stName, (size_t)nStName, sizeof(char *), ts_cmp_state_name);
   ts_src r = { text, text + len, 0 };
   char info[4200], buf[4200];
   char **pat = NULL; int nPat = 0, capPat = 0, rc = HTKAMD_OK, k;
   ts_line *ln = NULL; int nLn = 0, capLn = 0;
   char **leaf = NULL; int nLeaf = 0, capLeaf = 0;
   unsigned char *ann = NULL;
#define LT_BAD(code, ...) do { htkamd_set_error(__VA_ARGS__); rc = (code); goto done; } while (0)
   /* the questions: "QS name { pat, pat ... }", a line each */
   while ((k = ts_string(&r, info, sizeof(info))) > 0 && !strcmp(info, "QS")) {
      char qname[512];
      if (ts_string(&r, qname, sizeof(qname)) <= 0) LT_BAD(HTKAMD_EIO, "mmf_load_trees: %s: question name expected", path);
      const char *e = r.p;
      while (e < r.end && *e != '\n') e++;
      const char *p = r.p, *last = e;
      r.p = e;
      while (p < last && isspace((unsigned char)*p)) p++;
      while (last > p && isspace((unsigned char)last[-1])) last--;
      if (p >= last || *p != '{') LT_BAD(HTKAMD_EIO, "mmf_load_trees: %s: no { in the item list of question %s", path, qname);
      if (last[-1] != '}') LT_BAD(HTKAMD_EIO, "mmf_load_trees: %s: no } in the item list of question %s", path, qname);
      if ((H && ts_find_quest(H, qname) >= 0) || ts_find_quest(N, qname) >= 0) LT_BAD(HTKAMD_EINVAL, "mmf_load_trees: question name %s invalid: defined twice", qname);
      p++; last--;                                      /* LoadQuestion: the closing brace stands for the last comma */
      nPat = 0;
      do {                                              /* ParseAlpha: quoted, or up to white space or one of ".,)" */
         htx_src ps = {p, last, 0};
         const int got = htx_read_string(&ps, 0, ".,)", buf, sizeof(buf));
         if (got == HTX_OPEN) LT_BAD(HTKAMD_EIO, "mmf_load_trees: %s: unterminated quote in question %s", path, qname);
         if (got == HTX_LONG) LT_BAD(HTKAMD_EIO, "mmf_load_trees: %s: a pattern of question %s is too long", path, qname);
         if (got == HTX_NONE) buf[0] = 0;
         p = ps.p;
         while (p < last && isspace((unsigned char)*p)) p++;
         if (p < last && *p != ',') LT_BAD(HTKAMD_EIO, "mmf_load_trees: %s: missing , in the item list of question %s", path, qname);
         p++;
         if (nPat + 1 > capPat) { capPat = capPat * 2 + 16; pat = (char **)realloc(pat, sizeof(char *) * (size_t)capPat); }
         pat[nPat++] = strdup(buf);
      } while (p < last);
      /* the patterns are prepended as they are read (:453): the file's first is the list's last -- in QS order (what this library keeps,
         the list reversed) they stand as the file has them */
      ts_add_quest(N, qname, (const char *const *)pat, nPat);
      for (int i = 0; i < nPat; i++) free(pat[i]);
   }
   if (k < 0) LT_BAD(HTKAMD_EIO, "mmf_load_trees: %s: a string is not terminated", path);
   if (nHeldQ + N->nQ == 0) LT_BAD(HTKAMD_EINVAL, "mmf_load_trees: %s: Questions Expected", path);
   if (k == 0) LT_BAD(HTKAMD_EINVAL, "mmf_load_trees: %s holds no trees", path);
   /* the trees */
   do {
      char bname[sizeof(info)];
      strcpy(bname, info);
      const size_t L = strlen(bname);
      char *br = strchr(bname, '[');
      int state = 0;
      if (!(L && bname[L - 1] == ']' && br)) LT_BAD(HTKAMD_EMODEL, "mmf_load_trees: %s is a model tree (a name without [state], the reference's 'h' trees): model trees are not built", info);
      *br++ = 0;
      if (sscanf(br, "%d", &state) != 1 || state < 2) LT_BAD(HTKAMD_EINVAL, "mmf_load_trees: Cannot parse tree state %s", info);
      if (!bname[0]) LT_BAD(HTKAMD_EINVAL, "mmf_load_trees: Cannot parse tree name %s (base-phone)", info);
      if (ts_string(&r, buf, sizeof(buf)) <= 0) LT_BAD(HTKAMD_EIO, "mmf_load_trees: %s: tree %s has no body", path, info);
      nLn = 0; nLeaf = 0;
#define LT_LEAF(name, dst) do { \
         char *key_ = (name); \
         if (!bsearch(&key_, stName, (size_t)nStName, sizeof(char *), ts_cmp_state_name)) LT_BAD(HTKAMD_EMODEL, "mmf_load_trees: Macro %s not recognised (tree %s: a leaf must be a ~s macro of the set)", (name), info); \
         int at_ = 0; \
         while (at_ < nLeaf && strcmp(leaf[at_], (name))) at_++; \
         if (at_ == nLeaf) { if (nLeaf + 1 > capLeaf) { capLeaf = capLeaf * 2 + 16; leaf = (char **)realloc(leaf, sizeof(char *) * (size_t)capLeaf); } leaf[nLeaf++] = strdup(name); } \
         (dst) = -1 - at_; } while (0)
      if (strcmp(buf, "{")) {                           /* a single leaf */
         int only; LT_LEAF(buf, only); (void)only;
      } else {
         for (;;) {
            const int g = ts_string(&r, buf, sizeof(buf));
            if (g <= 0) LT_BAD(HTKAMD_EIO, "mmf_load_trees: %s: tree %s is not closed by }", path, info);
            if (!strcmp(buf, "}")) break;
            int n;
            if (sscanf(buf, "%d", &n) != 1 || n > 0 || n < -(1 << 20)) LT_BAD(HTKAMD_EINVAL, "mmf_load_trees: tree %s: node number expected, not %s", info, buf);
            if (nLn + 1 > capLn) { capLn = capLn * 2 + 64; ln = (ts_line *)realloc(ln, sizeof(ts_line) * (size_t)capLn); }
            ts_line *l = &ln[nLn];
            l->num = -n;
            if (ts_string(&r, buf, sizeof(buf)) <= 0) LT_BAD(HTKAMD_EIO, "mmf_load_trees: %s: tree %s ends inside a node", path, info);
            l->quest = ts_find_quest(N, buf);
            if (l->quest >= 0) l->quest += nHeldQ; else if (H) l->quest = ts_find_quest(H, buf);
            if (l->quest < 0) LT_BAD(HTKAMD_EMODEL, "mmf_load_trees: Question %s not recognised (tree %s)", buf, info);
            for (int side = 0; side < 2; side++) {      /* no, then yes: a number is a node, anything else a macro */
               int num;
               if (ts_string(&r, buf, sizeof(buf)) <= 0) LT_BAD(HTKAMD_EIO, "mmf_load_trees: %s: tree %s ends inside a node", path, info);
               if (sscanf(buf, "%d", &num) == 1) {
                  if (num >= 0 || num < -(1 << 20)) LT_BAD(HTKAMD_EINVAL, "mmf_load_trees: Node %d not in tree %s (a child is a node number below 0 or a macro)", num, info);
                  l->kid[side] = -num;
               } else LT_LEAF(buf, l->kid[side]);
            }
            nLn++;
         }
         if (nLn == 0) LT_BAD(HTKAMD_EINVAL, "mmf_load_trees: tree %s has no node", info);
         /* GetNode (:3327): a line's node is the root or a child some earlier line named; ShowTrees numbers the nodes 0 .. size-1 */
         ann = (unsigned char *)calloc((size_t)nLn, 1);   /* 1: named as a child (or the root), 2: defined */
         ann[0] = 1;
         for (int i = 0; i < nLn; i++) {
            if (ln[i].num >= nLn || !ann[ln[i].num]) LT_BAD(HTKAMD_EINVAL, "mmf_load_trees: Node %d not in tree %s", -ln[i].num, info);
            if (ann[ln[i].num] == 2) LT_BAD(HTKAMD_EINVAL, "mmf_load_trees: Node %d of tree %s is defined twice", -ln[i].num, info);
            ann[ln[i].num] = 2;
            for (int side = 0; side < 2; side++) {
               const int c = ln[i].kid[side];
               if (c < 0) continue;
               if (c >= nLn) LT_BAD(HTKAMD_EINVAL, "mmf_load_trees: Node %d not in tree %s (%d nodes)", -c, info, nLn);
               if (ann[c]) LT_BAD(HTKAMD_EINVAL, "mmf_load_trees: Node %d of tree %s has two parents", -c, info);
               ann[c] = 1;
            }
         }
         for (int i = 0; i < nLn; i++) if (ann[i] != 2) LT_BAD(HTKAMD_EINVAL, "mmf_load_trees: Node %d of tree %s is never defined", -i, info);
         free(ann); ann = NULL;
      }
      {
         int *quest = (int *)malloc(sizeof(int) * (size_t)(nLn + 1)), *no = (int *)malloc(sizeof(int) * (size_t)(nLn + 1)), *yes = (int *)malloc(sizeof(int) * (size_t)(nLn + 1));
         for (int i = 0; i < nLn; i++) { quest[ln[i].num] = ln[i].quest; no[ln[i].num] = ln[i].kid[0]; yes[ln[i].num] = ln[i].kid[1]; }
         const htkamd_tree_desc d = { bname, state, nLn, quest, no, yes, (const char *const *)leaf, nLeaf };
         ts_add_tree(N, &d, NULL);
         free(quest); free(no); free(yes);
         for (int i = 0; i < nLeaf; i++) free(leaf[i]);
         nLeaf = 0;
      }
   } while ((k = ts_string(&r, info, sizeof(info))) > 0);
   if (k < 0) LT_BAD(HTKAMD_EIO, "mmf_load_trees: %s: a string is not terminated", path);
#undef LT_LEAF
#undef LT_BAD
   /* all good: behind the held ones (LoadQuestion appends to the question list, CreateTree to the tree list) */
   if (!s->trees) s->trees = (mmf_trees *)calloc(1, sizeof(mmf_trees));
   {
      mmf_trees *T = s->trees;
      T->q = (mmf_quest *)realloc(T->q, sizeof(mmf_quest) * (size_t)(T->nQ + N->nQ + 1));
      memcpy(T->q + T->nQ, N->q, sizeof(mmf_quest) * (size_t)N->nQ); T->nQ += N->nQ;
      T->t = (mmf_tree *)realloc(T->t, sizeof(mmf_tree) * (size_t)(T->nT + N->nT + 1));
      memcpy(T->t + T->nT, N->t, sizeof(mmf_tree) * (size_t)N->nT); T->nT += N->nT;
      N->nQ = N->nT = 0;
   }
done:
   for (int i = 0; i < nLeaf; i++) free(leaf[i]);
   free(leaf); free(ln); free(ann); free(pat); free(stName); free(text);
   htkamd_mmf_trees_free(N);
   return rc;
}

/* ------------------------------------------------------------------------------------------ the device job */
typedef struct { char *pool; int *off; int n, bytes, capBytes; } ts_pool;

static void ts_pool_add(ts_pool *p, const char *str)
{
   const int L = (int)strlen(str) + 1;
   if (p->bytes + L > p->capBytes) { p->capBytes = (p->capBytes + L) * 2 + 256; p->pool = (char *)realloc(p->pool, (size_t)p->capBytes); }
   memcpy(p->pool + p->bytes, str, (size_t)L);
   p->off[p->n++] = p->bytes;
   p->bytes += L;
   p->off[p->n] = p->bytes;
}
static void ts_pool_init(ts_pool *p, int nMax) { memset(p, 0, sizeof(*p)); p->off = (int *)calloc((size_t)nMax + 2, sizeof(int)); }
static void ts_pool_free(ts_pool *p) { free(p->pool); free(p->off); }

static int ts_check_names(const char *who, const char *const *names, int N)
{
   for (int n = 0; n < N; n++) {
      if (!names[n] || !names[n][0]) { htkamd_set_error("%s: name %d is empty", who, n); return HTKAMD_EINVAL; }
      if (strlen(names[n]) > HTKAMD_SYNTH_MAXNAME) {
         htkamd_set_error("%s: the name %.40s... has %d characters (at most %d: the reference strips the contexts in a buffer of 100)", who, names[n], (int)strlen(names[n]), HTKAMD_SYNTH_MAXNAME);
         return HTKAMD_EINVAL;
      }
   }
   return HTKAMD_OK;
}

int htkamd_name_question_answers(const char *const *names, int N, const htkamd_tree_question *q, int nQ, unsigned char *answers, void *stream)
{
   if (!names || N < 1 || !q || nQ < 1 || !answers) { htkamd_set_error("name_question_answers: bad argument"); return HTKAMD_EINVAL; }
   int rc = ts_check_names("name_question_answers", names, N), nPat = 0;
   if (rc) return rc;
   for (int i = 0; i < nQ; i++) {
      if (!q[i].name || q[i].nPatterns < 1 || !q[i].patterns) { htkamd_set_error("name_question_answers: question %d has no name or no pattern", i); return HTKAMD_EINVAL; }
      nPat += q[i].nPatterns;
   }
   if (!htkamd_synth_dev_run) { htkamd_set_error("name_question_answers: no HIP device: this build holds the host files only"); return HTKAMD_ENODEV; }
   ts_pool nm, pt;
   ts_pool_init(&nm, N); ts_pool_init(&pt, nPat);
   int *qPat = (int *)malloc(sizeof(int) * ((size_t)nQ + 1));
   for (int n = 0; n < N; n++) ts_pool_add(&nm, names[n]);
   for (int i = 0; i < nQ; i++) { qPat[i] = pt.n; for (int k = 0; k < q[i].nPatterns; k++) ts_pool_add(&pt, q[i].patterns[k]); }
   qPat[nQ] = pt.n;
   htkamd_synth_job job;
   memset(&job, 0, sizeof(job));
   job.N = N; job.namePool = nm.pool; job.nameOff = nm.off; job.nQ = nQ; job.patPool = pt.pool; job.patOff = pt.off; job.qPat = qPat;
   rc = htkamd_synth_dev_run(&job, answers, NULL, stream);
   ts_pool_free(&nm); ts_pool_free(&pt); free(qPat);
   return rc;
}

/* TriStrip (HLabel.c:1021): behind the first '-', before the last '+' */
static void ts_tristrip(const char *name, char *out, size_t cap)
{
   const char *p = strchr(name, '-');
   snprintf(out, cap, "%s", p ? p + 1 : name);
   char *plus = strrchr(out, '+');
   if (plus) *plus = 0;
}

/* the first tree of the list for a base phone and a state (AssignStructure :3129), -1: none */
typedef struct { const char *name; int state, idx; } ts_tkey;
static int ts_cmp_tkey(const void *a, const void *b)
{
   const ts_tkey *x = (const ts_tkey *)a, *y = (const ts_tkey *)b;
   const int c = strcmp(x->name, y->name);
   if (c) return c;
   if (x->state != y->state) return (x->state > y->state) - (x->state < y->state);
   return (x->idx > y->idx) - (x->idx < y->idx);
}
static ts_tkey *ts_tree_index(const mmf_trees *T)
{
   ts_tkey *k = (ts_tkey *)malloc(sizeof(ts_tkey) * (size_t)(T->nT + 1));
   for (int i = 0; i < T->nT; i++) { k[i].name = T->t[i].name; k[i].state = T->t[i].state; k[i].idx = i; }
   qsort(k, (size_t)T->nT, sizeof(ts_tkey), ts_cmp_tkey);
   return k;
}
static int ts_find_tree(const ts_tkey *k, int n, const char *base, int state)
{
   int lo = 0, hi = n - 1, hit = -1;
   while (lo <= hi) {
      const int mid = (lo + hi) / 2;
      int c = strcmp(k[mid].name, base);
      if (!c) c = (k[mid].state > state) - (k[mid].state < state);
      if (c == 0) { hit = mid; hi = mid - 1; } else if (c < 0) lo = mid + 1; else hi = mid - 1;
   }
   return hit < 0 ? -1 : k[hit].idx;
}

/* The walks of `nPairs` (name, tree) pairs over the held trees on the device: only the questions some tree asks are matched. */
static int ts_descend(const mmf_trees *T, const char *const *names, int N, const int *pairName, const int *pairTree, int nPairs, int *leaf, void *stream, const char *who)
{
   if (!htkamd_synth_dev_run) { htkamd_set_error("%s: no HIP device: this build holds the host files only", who); return HTKAMD_ENODEV; }
   int *qUse = (int *)malloc(sizeof(int) * (size_t)(T->nQ + 1)), nUse = 0, nPat = 0, nNodes = 0;
   for (int i = 0; i < T->nQ; i++) qUse[i] = -1;
   for (int t = 0; t < T->nT; t++) { nNodes += T->t[t].nNodes; for (int k = 0; k < T->t[t].nNodes; k++) qUse[T->t[t].quest[k]] = 0; }
   for (int i = 0; i < T->nQ; i++) if (qUse[i] == 0) { qUse[i] = nUse++; nPat += T->q[i].nPat; }
   ts_pool nm, pt;
   ts_pool_init(&nm, N); ts_pool_init(&pt, nPat);
   int *qPat = (int *)malloc(sizeof(int) * ((size_t)nUse + 1));
   int *treeOff = (int *)malloc(sizeof(int) * ((size_t)T->nT + 1)), *treeLeaves = (int *)malloc(sizeof(int) * ((size_t)T->nT + 1));
   int *quest = (int *)malloc(sizeof(int) * ((size_t)nNodes + 1)), *no = (int *)malloc(sizeof(int) * ((size_t)nNodes + 1)), *yes = (int *)malloc(sizeof(int) * ((size_t)nNodes + 1));
   for (int n = 0; n < N; n++) ts_pool_add(&nm, names[n]);
   for (int i = 0, u = 0; i < T->nQ; i++) if (qUse[i] >= 0) { qPat[u++] = pt.n; for (int k = 0; k < T->q[i].nPat; k++) ts_pool_add(&pt, T->q[i].pat[k]); }
   qPat[nUse] = pt.n;
   nNodes = 0;
   for (int t = 0; t < T->nT; t++) {
      const mmf_tree *m = &T->t[t];
      treeOff[t] = nNodes; treeLeaves[t] = m->nLeaves;
      for (int k = 0; k < m->nNodes; k++) { quest[nNodes] = qUse[m->quest[k]]; no[nNodes] = m->no[k]; yes[nNodes] = m->yes[k]; nNodes++; }
   }
   treeOff[T->nT] = nNodes;
   htkamd_synth_job job;
   memset(&job, 0, sizeof(job));
   job.N = N; job.namePool = nm.pool; job.nameOff = nm.off; job.nQ = nUse; job.patPool = pt.pool; job.patOff = pt.off; job.qPat = qPat;
   job.nTrees = T->nT; job.treeOff = treeOff; job.quest = quest; job.no = no; job.yes = yes; job.treeLeaves = treeLeaves;
   job.nPairs = nPairs; job.pairName = pairName; job.pairTree = pairTree;
   const int rc = htkamd_synth_dev_run(&job, NULL, leaf, stream);
   ts_pool_free(&nm); ts_pool_free(&pt);
   free(qUse); free(qPat); free(treeOff); free(treeLeaves); free(quest); free(no); free(yes);
   return rc;
}

int htkamd_tree_descend(const htkamd_mmf *s, const char *const *names, int N, int firstState, int nStates, int *tree, int *leaf, void *stream)
{
   if (!s || !s->finished || !names || N < 1 || nStates < 1 || !tree || !leaf) { htkamd_set_error("tree_descend: bad argument"); return HTKAMD_EINVAL; }
   if (!s->trees || !s->trees->nT) { htkamd_set_error("tree_descend: there are no existing trees"); return HTKAMD_EINVAL; }
   int rc = ts_check_names("tree_descend", names, N);
   if (rc) return rc;
   ts_tkey *idx = ts_tree_index(s->trees);
   int *pairName = (int *)malloc(sizeof(int) * (size_t)N * nStates);
   char base[HTKAMD_SYNTH_MAXNAME + 1];
   for (int n = 0; n < N; n++) {
      ts_tristrip(names[n], base, sizeof(base));
      for (int k = 0; k < nStates; k++) { pairName[(size_t)n * nStates + k] = n; tree[(size_t)n * nStates + k] = ts_find_tree(idx, s->trees->nT, base, firstState + k); }
   }
   rc = ts_descend(s->trees, names, N, pairName, tree, N * nStates, leaf, stream, "tree_descend");
   free(idx); free(pairName);
   return rc;
}

/* ------------------------------------------------------------------------------------------ AU */
static char **g_tsSortNames;
static int ts_cmp_idx_name(const void *a, const void *b)
{
   const int x = *(const int *)a, y = *(const int *)b, c = strcmp(g_tsSortNames[x], g_tsSortNames[y]);
   return c ? c : (x > y) - (x < y);
}

/* the model side of the flat description after hm[] changed; the state side (and states nobody uses any more) is tc_compact's */
static void ts_rebuild_desc(struct htkamd_mmf *s)
{
   int tot = 0;
   for (int h = 0; h < s->nHm; h++) tot += s->hm[h].N - 2;
   s->transN = (int *)realloc(s->transN, sizeof(int) * (size_t)(s->nTr + 1));
   s->transOff = (int *)realloc(s->transOff, sizeof(int) * ((size_t)s->nTr + 1));
   for (int t = 0; t < s->nTr; t++) { s->transN[t] = s->tr[t].N; s->transOff[t] = s->tr[t].off; }
   s->transOff[s->nTr] = s->nTp;
   s->hmmTrans = (int *)realloc(s->hmmTrans, sizeof(int) * (size_t)(s->nHm + 1));
   s->hmmStateOff = (int *)realloc(s->hmmStateOff, sizeof(int) * ((size_t)s->nHm + 1));
   s->hmmState = (int *)realloc(s->hmmState, sizeof(int) * (size_t)(tot + 1));
   tot = 0;
   for (int h = 0; h < s->nHm; h++) { s->hmmTrans[h] = s->hm[h].trans; s->hmmStateOff[h] = tot; tot += s->hm[h].N - 2; }
   s->hmmStateOff[s->nHm] = tot;
   htkamd_model_desc *d = &s->d;
   d->numTrans = s->nTr; d->transN = s->transN; d->transOff = s->transOff; d->transP = s->tp;
   d->numPhys = s->nHm; d->hmmTrans = s->hmmTrans; d->hmmStateOff = s->hmmStateOff; d->hmmState = s->hmmState;
   int *none = (int *)malloc(sizeof(int) * (size_t)(s->nSt + 1));
   for (int i = 0; i < s->nSt; i++) none[i] = -1;
   tc_compact(s, none, 0);
   free(none);
   g_tsSortNames = s->logName;
   s->logSorted = (int *)realloc(s->logSorted, sizeof(int) * (size_t)(s->nLog ? s->nLog : 1));
   for (int i = 0; i < s->nLog; i++) s->logSorted[i] = i;
   qsort(s->logSorted, (size_t)s->nLog, sizeof(int), ts_cmp_idx_name);
}

static int ts_check_set(const struct htkamd_mmf *s, const char *who)
{
   if (s->nStreams > 1) { htkamd_set_error("%s: a set with more than one stream (%d) is not supported", who, s->nStreams); return HTKAMD_EMODEL; }
   if (s->tiedMix) { htkamd_set_error("%s: tied-mixture sets are not supported", who); return HTKAMD_EMODEL; }
   if (strstr(s->kind, "DISCRETE")) { htkamd_set_error("%s: discrete sets are not supported", who); return HTKAMD_EMODEL; }
   return HTKAMD_OK;
}

int htkamd_mmf_add_unseen(htkamd_mmf *s, const char *hmmListPath, int *nSeen, int *nUnseen, void *stream)
{
   if (!s || !s->finished || !hmmListPath) { htkamd_set_error("mmf_add_unseen: bad argument"); return HTKAMD_EINVAL; }
   if (!s->trees || !s->trees->nT) { htkamd_set_error("mmf_add_unseen: there are no existing trees (TB builds them, LT loads them)"); return HTKAMD_EINVAL; }
   int rc = ts_check_set(s, "mmf_add_unseen");
   if (rc) return rc;
   const mmf_trees *T = s->trees;
   size_t listLen; int why;
   char *listTxt = htx_read_file(hmmListPath, &listLen, &why);
   if (!listTxt) { htkamd_set_error(why == HTX_ENOMEM ? "mmf_add_unseen: out of memory reading HMM list %s" : "mmf_add_unseen: cannot open HMM list %s", hmmListPath); return why == HTX_ENOMEM ? HTKAMD_ENOMEM : HTKAMD_EIO; }
   char **names = NULL; int nL = 0, capL = 0;
   int *order = NULL, *phys = NULL, *sortIdx = NULL, *uOf = NULL, *proto = NULL, *pairName = NULL, *pairTree = NULL, *leaf = NULL, *pairOff = NULL;
   const char **uNames = NULL;
   ts_tkey *tidx = NULL;
   int *baseProto = NULL; char **baseName = NULL; int nBase = 0;
   char **stName = NULL; int *stIdx = NULL;
   {
      char a[1024], b[1024]; int r;
      htx_src src = {listTxt, listTxt + listLen, 0};
      while ((r = htx_hmmlist_next(&src, a, sizeof(a), b, sizeof(b))) == HTX_GOT) {
         if (b[0] && strcmp(a, b)) { htkamd_set_error("mmf_add_unseen: %s: model %s has the physical name %s: a list of plain names is expected", hmmListPath, a, b); rc = HTKAMD_EINVAL; break; }
         if (nL + 1 > capL) { capL = capL * 2 + 256; names = (char **)realloc(names, sizeof(char *) * (size_t)capL); }
         names[nL++] = strdup(a);
      }
      if (r < 0) { htkamd_set_error("mmf_add_unseen: HMM list %s, entry %d: %s", hmmListPath, nL + 1, htx_result_text(r)); rc = HTKAMD_EMODEL; }
      free(listTxt);
   }
   if (!rc && nL == 0) { htkamd_set_error("mmf_add_unseen: %s lists no model", hmmListPath); rc = HTKAMD_EINVAL; }
   if (!rc) rc = ts_check_names("mmf_add_unseen", (const char *const *)names, nL);
   if (rc) goto done;
   sortIdx = (int *)malloc(sizeof(int) * (size_t)nL);
   for (int i = 0; i < nL; i++) sortIdx[i] = i;
   g_tsSortNames = names;
   qsort(sortIdx, (size_t)nL, sizeof(int), ts_cmp_idx_name);
   for (int i = 1; i < nL; i++) if (!strcmp(names[sortIdx[i - 1]], names[sortIdx[i]])) { htkamd_set_error("mmf_add_unseen: %s lists model %s twice", hmmListPath, names[sortIdx[i]]); rc = HTKAMD_EINVAL; goto done; }
   /* FindProtoModel: per base phone the first physical model of the macro table's scan (bucket by bucket, the later-made first).  A model
      synthesised earlier in the call may come before it in the scan, but it has that very proto's size, duration and matrix. */
   {
      int *scan = (int *)malloc(sizeof(int) * (size_t)(s->nHm + 1));
      const char **nm = (const char **)malloc(sizeof(char *) * (size_t)(s->nHm + 1));
      for (int k = 0; k < s->nHm; k++) nm[k] = s->hm[s->hmCreate ? s->hmCreate[k] : k].name;
      htkamd_hmm_scan_order(nm, s->nHm, scan);
      baseName = (char **)malloc(sizeof(char *) * (size_t)(s->nHm + 1)); baseProto = (int *)malloc(sizeof(int) * (size_t)(s->nHm + 1));
      int *bIdx = (int *)malloc(sizeof(int) * (size_t)(s->nHm + 1));
      char base[600];
      for (int k = 0; k < s->nHm; k++) { ts_tristrip(nm[k], base, sizeof(base)); baseName[k] = strdup(base); bIdx[k] = k; }
      g_tsSortNames = baseName;
      qsort(bIdx, (size_t)s->nHm, sizeof(int), ts_cmp_idx_name);
      int *rank = (int *)malloc(sizeof(int) * (size_t)(s->nHm + 1));       /* place in the scan */
      for (int k = 0; k < s->nHm; k++) rank[scan[k]] = k;
      char **ub = (char **)malloc(sizeof(char *) * (size_t)(s->nHm + 1));
      for (int k = 0; k < s->nHm; ) {
         int e = k, best = bIdx[k];
         while (e < s->nHm && !strcmp(baseName[bIdx[e]], baseName[bIdx[k]])) { if (rank[bIdx[e]] < rank[best]) best = bIdx[e]; e++; }
         ub[nBase] = strdup(baseName[bIdx[k]]); baseProto[nBase] = s->hmCreate ? s->hmCreate[best] : best; nBase++;
         k = e;
      }
      for (int k = 0; k < s->nHm; k++) free(baseName[k]);
      free(baseName); baseName = ub;
      free(scan); free(nm); free(bIdx); free(rank);
   }
   /* TreeFilter: the new list's names in the order of ITS macro table */
   order = (int *)malloc(sizeof(int) * (size_t)nL); phys = (int *)malloc(sizeof(int) * (size_t)nL); uOf = (int *)malloc(sizeof(int) * (size_t)nL);
   htkamd_hmm_scan_order((const char *const *)names, nL, order);
   int nU = 0, seen = 0, nPairs = 0;
   uNames = (const char **)malloc(sizeof(char *) * (size_t)nL); proto = (int *)malloc(sizeof(int) * (size_t)nL); pairOff = (int *)malloc(sizeof(int) * ((size_t)nL + 1));
   tidx = ts_tree_index(T);
   int capPairs = 0;
   for (int k = 0; k < nL; k++) {
      const int i = order[k];
      phys[i] = htkamd_mmf_find_logical(s, names[i]);
      uOf[i] = -1;
      if (phys[i] >= 0) { seen++; continue; }
      char base[HTKAMD_SYNTH_MAXNAME + 1];
      ts_tristrip(names[i], base, sizeof(base));
      int lo = 0, hi = nBase - 1, hit = -1;
      while (lo <= hi) { const int mid = (lo + hi) / 2, c = strcmp(baseName[mid], base); if (!c) { hit = mid; break; } if (c < 0) lo = mid + 1; else hi = mid - 1; }
      if (hit < 0) { htkamd_set_error("mmf_add_unseen: FindProtoModel: no proto for %s in hSet", names[i]); rc = HTKAMD_EMODEL; goto done; }
      const int N = s->hm[baseProto[hit]].N;
      if (nPairs + N > capPairs) { capPairs = (capPairs + N) * 2 + 1024; pairName = (int *)realloc(pairName, sizeof(int) * (size_t)capPairs); pairTree = (int *)realloc(pairTree, sizeof(int) * (size_t)capPairs); }
      pairOff[nU] = nPairs;
      for (int j = 2; j < N; j++) {
         const int t = ts_find_tree(tidx, T->nT, base, j);
         if (t < 0) { htkamd_set_error("mmf_add_unseen: AssignStructure: cannot find tree for %s state %d", names[i], j); rc = HTKAMD_EMODEL; goto done; }
         pairName[nPairs] = nU; pairTree[nPairs] = t; nPairs++;
      }
      uOf[i] = nU; uNames[nU] = names[i]; proto[nU] = baseProto[hit]; nU++;
   }
   pairOff[nU] = nPairs;
   if (nU > 0) {
      leaf = (int *)malloc(sizeof(int) * (size_t)(nPairs + 1));
      if ((rc = ts_descend(T, uNames, nU, pairName, pairTree, nPairs, leaf, stream, "mmf_add_unseen"))) goto done;
      /* the leaves' macros as states of the set */
      stName = (char **)malloc(sizeof(char *) * (size_t)(s->nSt + 1)); stIdx = (int *)malloc(sizeof(int) * (size_t)(s->nSt + 1));
      int nS = 0;
      for (int i = 0; i < s->nSt; i++) if (s->st[i].name) stIdx[nS++] = i;
      for (int i = 0; i < s->nSt; i++) stName[i] = s->st[i].name;
      /* (sorted through the index: un-named states are not in it) */
      g_tsSortNames = stName;
      qsort(stIdx, (size_t)nS, sizeof(int), ts_cmp_idx_name);
      for (int p = 0; p < nPairs; p++) {
         const mmf_tree *m = &T->t[pairTree[p]];
         if (leaf[p] < 0 || leaf[p] >= m->nLeaves) { htkamd_set_error("mmf_add_unseen: the walk down tree %s[%d] for %s ended nowhere", m->name, m->state, uNames[pairName[p]]); rc = HTKAMD_EHIP; goto done; }
         const char *mac = m->leaf[leaf[p]];
         int lo = 0, hi = nS - 1, hit = -1;
         while (lo <= hi) { const int mid = (lo + hi) / 2, c = strcmp(stName[stIdx[mid]], mac); if (!c) { hit = stIdx[mid]; break; } if (c < 0) lo = mid + 1; else hi = mid - 1; }
         if (hit < 0) { htkamd_set_error("mmf_add_unseen: the leaf %s of tree %s[%d] is no ~s macro of the set any more", mac, m->name, m->state); rc = HTKAMD_EMODEL; goto done; }
         leaf[p] = hit;
      }
   }
   /* SynthModel for the new names, then SwapLists: the set's models are the list's, physical and logical, in list order */
   {
      mmf_hmm *nh = (mmf_hmm *)malloc(sizeof(mmf_hmm) * (size_t)nL);
      for (int i = 0; i < nL; i++) {
         const mmf_hmm *src = &s->hm[phys[i] >= 0 ? phys[i] : proto[uOf[i]]];
         mmf_hmm *h = &nh[i];
         h->name = strdup(names[i]); h->N = src->N; h->src = phys[i] >= 0 ? src->src : 0; h->dur = src->dur; h->trans = src->trans;
         h->state = (int *)malloc(sizeof(int) * (size_t)src->N);
         memcpy(h->state, src->state, sizeof(int) * (size_t)src->N);
         if (phys[i] >= 0) continue;
         const int u = uOf[i];
         for (int j = 2; j < h->N; j++) h->state[j - 1] = leaf[pairOff[u] + j - 2];
         if (!s->tr[src->trans].name) {                 /* CloneSMatrix: a matrix that is no macro is copied */
            const int N = src->N, t0 = src->trans;
            if (s->nTr + 1 > s->capTr) { s->capTr = s->capTr * 2 + 64; s->tr = (mmf_trans *)realloc(s->tr, sizeof(mmf_trans) * (size_t)s->capTr); }
            if (s->nTp + N * N > s->capTp) { s->capTp = (s->capTp + N * N) * 2; s->tp = (float *)realloc(s->tp, sizeof(float) * (size_t)s->capTp); }
            memcpy(s->tp + s->nTp, s->tp + s->tr[t0].off, sizeof(float) * (size_t)N * N);
            s->tr[s->nTr].name = NULL; s->tr[s->nTr].N = N; s->tr[s->nTr].off = s->nTp; s->tr[s->nTr].src = 0;
            h->trans = s->nTr++; s->nTp += N * N;
         }
      }
      for (int h = 0; h < s->nHm; h++) { free(s->hm[h].name); free(s->hm[h].state); }
      free(s->hm);
      s->hm = nh; s->nHm = s->capHm = nL;
      for (int i = 0; i < s->nLog; i++) free(s->logName[i]);
      free(s->logName); free(s->logPhys);
      s->logName = names; names = NULL;
      s->logPhys = (int *)malloc(sizeof(int) * (size_t)nL);
      s->nLog = nL;
      /* SwapLists re-makes the macros walking the list's table, itself made by head insertion: in the set's table the names of a bucket
         stand in list order -- as if made last first */
      s->hmCreate = (int *)realloc(s->hmCreate, sizeof(int) * (size_t)nL); s->logCreate = (int *)realloc(s->logCreate, sizeof(int) * (size_t)nL);
      for (int i = 0; i < nL; i++) { s->logPhys[i] = i; s->hmCreate[i] = s->logCreate[i] = nL - 1 - i; }
      ts_rebuild_desc(s);
      if (!s->fullc) dc_fix_gconsts(s);               /* FixAllGConsts before HHEd saves (:6469) */
   }
   if (nSeen) *nSeen = seen;
   if (nUnseen) *nUnseen = nU;
done:
   if (names) { for (int i = 0; i < nL; i++) free(names[i]); free(names); }
   for (int k = 0; k < nBase; k++) free(baseName[k]);
   free(baseName); free(baseProto);
   free(order); free(phys); free(sortIdx); free(uOf); free(proto); free(pairName); free(pairTree); free(leaf); free(pairOff); free((void *)uNames); free(tidx);
   free(stName); free(stIdx);
   return rc;
}

/* ------------------------------------------------------------------------------------------ CO */
static unsigned ts_hash_ints(const int *v, int n)
{
   unsigned h = 2166136261u;
   for (int i = 0; i < n; i++) { h ^= (unsigned)v[i]; h *= 16777619u; h ^= h >> 15; }
   return h;
}

/* what EquivState compares of a state (:670, EquivStream :650, EquivMix :642): per stream the number of components, per component the
   weight (only where there are several) and WHICH mean and variance vector -- a ~u / ~v macro, or the Gaussian's own */
static int ts_state_sig(const struct htkamd_mmf *s, int si, int *v)
{
   const mmf_state *st = &s->st[si];
   const int NS = s->nStreams > 1 ? s->nStreams : 1;
   int n = 0, c = st->comp0;
   for (int k = 0; k < NS; k++) {
      const int M = (NS > 1 && st->sMix) ? st->sMix[k] : st->nMix;
      v[n++] = M;
      for (int m = 0; m < M; m++, c++) {
         const int g = s->cg[c];
         int w = 0;
         if (M > 1) memcpy(&w, &s->wt[c], sizeof(int));
         v[n++] = w;
         v[n++] = (g < s->capMac && s->gMeanMac[g] >= 0) ? -1 - s->gMeanMac[g] : g;
         v[n++] = (g < s->capMac && s->gVarMac[g] >= 0) ? -1 - s->gVarMac[g] : g;
      }
   }
   return n;
}

int htkamd_mmf_compact(htkamd_mmf *s, const char *listPath, int *nLog, int *nPhys)
{
   if (!s || !s->finished) { htkamd_set_error("mmf_compact: bad argument"); return HTKAMD_EINVAL; }
   /* equivState (:4356-4366): a ~m macro, or both a ~u and a ~v macro (a varFloor is a ~v) */
   int seenMean = 0, seenVar = 0;
   for (int g = 0; g < s->nG && g < s->capGN; g++) if (s->gName[g]) seenMean = seenVar = 1;
   for (int i = 0; i < s->nVm; i++) { if (s->vm[i].type == 'u') seenMean = 1; else seenVar = 1; }
   const int equivState = seenMean && seenVar && !s->tiedMix && !strstr(s->kind, "DISCRETE");
   const int H = s->nHm;
   int maxN = 3, maxM = 1;
   for (int h = 0; h < H; h++) if (s->hm[h].N > maxN) maxN = s->hm[h].N;
   for (int i = 0; i < s->nSt; i++) if (s->st[i].nMix > maxM) maxM = s->st[i].nMix;
   /* states that count as one */
   int *canon = (int *)malloc(sizeof(int) * (size_t)(s->nSt + 1));
   for (int i = 0; i < s->nSt; i++) canon[i] = i;
   if (equivState) {
      unsigned cap = 16;
      while (cap < 2u * (unsigned)s->nSt) cap *= 2;
      int *tab = (int *)malloc(sizeof(int) * cap), *va = (int *)malloc(sizeof(int) * (size_t)(3 * maxM + 16)), *vb = (int *)malloc(sizeof(int) * (size_t)(3 * maxM + 16));
      for (unsigned i = 0; i < cap; i++) tab[i] = -1;
      for (int i = 0; i < s->nSt; i++) {
         const int na = ts_state_sig(s, i, va);
         unsigned at = ts_hash_ints(va, na) & (cap - 1);
         for (;; at = (at + 1) & (cap - 1)) {
            if (tab[at] < 0) { tab[at] = i; break; }
            const int nb = ts_state_sig(s, tab[at], vb);
            if (na == nb && !memcmp(va, vb, sizeof(int) * (size_t)na)) { canon[i] = tab[at]; break; }
         }
      }
      free(tab); free(va); free(vb);
   }
   /* the physical models in the macro table's order: the first of a group stays (EquivHMM :685: size, the matrix ITSELF, the states) */
   int *scan = (int *)malloc(sizeof(int) * (size_t)(H + 1)), *surv = (int *)malloc(sizeof(int) * (size_t)(H + 1)), *newIdx = (int *)malloc(sizeof(int) * (size_t)(H + 1));
   {
      const char **nm = (const char **)malloc(sizeof(char *) * (size_t)(H + 1));
      for (int k = 0; k < H; k++) nm[k] = s->hm[s->hmCreate ? s->hmCreate[k] : k].name;
      htkamd_hmm_scan_order(nm, H, scan);
      if (s->hmCreate) for (int k = 0; k < H; k++) scan[k] = s->hmCreate[scan[k]];
      free(nm);
   }
   {
      unsigned cap = 16;
      while (cap < 2u * (unsigned)H) cap *= 2;
      int *tab = (int *)malloc(sizeof(int) * cap), *va = (int *)malloc(sizeof(int) * (size_t)(maxN + 2)), *vb = (int *)malloc(sizeof(int) * (size_t)(maxN + 2));
      for (unsigned i = 0; i < cap; i++) tab[i] = -1;
#define HSIG(h, v, n) do { const mmf_hmm *m_ = &s->hm[h]; (n) = 0; (v)[(n)++] = m_->N; (v)[(n)++] = m_->trans; for (int j_ = 1; j_ < m_->N - 1; j_++) (v)[(n)++] = canon[m_->state[j_]]; } while (0)
      for (int k = 0; k < H; k++) {
         const int h = scan[k];
         int na, nb;
         HSIG(h, va, na);
         unsigned at = ts_hash_ints(va, na) & (cap - 1);
         for (;; at = (at + 1) & (cap - 1)) {
            if (tab[at] < 0) { tab[at] = h; surv[h] = h; break; }
            HSIG(tab[at], vb, nb);
            if (na == nb && !memcmp(va, vb, sizeof(int) * (size_t)na)) { surv[h] = tab[at]; break; }
         }
      }
#undef HSIG
      free(tab); free(va); free(vb);
   }
   /* the logical names of a model that went become names of the one that stayed: new 'l' macros, made in the table's order (:4389-4404) */
   int *walk = tc_logical_walk(s);
   int *create = (int *)malloc(sizeof(int) * (size_t)(s->nLog + 1)), nC = 0;
   for (int k = 0; k < s->nLog; k++) { const int i = s->logCreate ? s->logCreate[k] : k; if (surv[s->logPhys[i]] == s->logPhys[i]) create[nC++] = i; }
   for (int k = 0; k < s->nLog; k++) { const int i = walk[k]; if (surv[s->logPhys[i]] != s->logPhys[i]) create[nC++] = i; }
   free(walk);
   int nKeep = 0;
   for (int h = 0; h < H; h++) {
      if (surv[h] != h) { free(s->hm[h].name); free(s->hm[h].state); newIdx[h] = -1; continue; }
      newIdx[h] = nKeep;
      if (nKeep != h) s->hm[nKeep] = s->hm[h];
      nKeep++;
   }
   for (int i = 0; i < s->nLog; i++) s->logPhys[i] = newIdx[surv[s->logPhys[i]]];
   {
      int *hc = (int *)malloc(sizeof(int) * (size_t)(nKeep + 1)), n = 0;
      for (int k = 0; k < H; k++) { const int h = s->hmCreate ? s->hmCreate[k] : k; if (newIdx[h] >= 0) hc[n++] = newIdx[h]; }
      free(s->hmCreate); s->hmCreate = hc;
   }
   free(s->logCreate); s->logCreate = create;
   s->nHm = nKeep;
   ts_rebuild_desc(s);
   if (!s->fullc) dc_fix_gconsts(s);                  /* FixAllGConsts before HHEd saves (:6469) */
   free(canon); free(scan); free(surv); free(newIdx);
   if (nLog) *nLog = s->nLog;
   if (nPhys) *nPhys = s->nHm;
   if (!listPath) return HTKAMD_OK;
   /* SaveHMMList (HModel.c:5029) */
   FILE *f = fopen(listPath, "w");
   if (!f) { htkamd_set_error("mmf_compact: cannot create HMM list file %s", listPath); return HTKAMD_EIO; }
   walk = tc_logical_walk(s);
   for (int k = 0; k < s->nLog; k++) {
      const int i = walk[k];
      const char *ph = s->hm[s->logPhys[i]].name;
      htx_write_string(f, s->logName[i], HTX_ESCAPE, 0);
      if (strcmp(ph, s->logName[i])) { fputc(' ', f); htx_write_string(f, ph, HTX_ESCAPE, 0); }
      fprintf(f, "\n");
   }
   free(walk);
   if (fclose(f)) { htkamd_set_error("mmf_compact: write error on %s", listPath); return HTKAMD_EIO; }
   return HTKAMD_OK;
}
