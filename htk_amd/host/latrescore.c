/* latrescore.c -- the host side of HLRescore for a batch of lattices (the device side: csrc/latrescore.hip):
 *   ReadDict (HDict.c:287) as far as HLRescore needs it: words, and per pronunciation its number and output symbol;
 *   ReadLattice / ReadOneLattice (HNet.c:878-1269): one level of SLF text, its refusals with the reference's reasons;
 *   LatStartNode / LatEndNode / LatTopSort (HLat.c:367-455) and the two orders in which LatFindBest and LatForwBackw meet arcs --
 *   they decide which of two equally good arcs stays, so they are part of the result;
 *   LatPrune's compaction (HLat.c:818-851), LatFindBest's label list (:634-673), WriteLattice (HNet.c:530-677).
 * Pure host code: links and runs without a device.
 */
#include <ctype.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../csrc/latrescore.h"
#include "htktext.h"

static void align_free(htkamd_lat_align *al, int n) { for (int i = 0; al && i < n; i++) free(al[i].label); free(al); }

/* ReadAlign (HNet.c:838): ":label[,duration[,likelihood]]:..." -> records; *n = 0 and no records for fewer than two colons */
static int read_align(const char *buf, htkamd_lat_align **out, int *n, const char *path)
{
   int cnt = -1;
   for (const char *p = buf; *p; p++) cnt += *p == ':';
   *out = NULL; *n = 0;
   if (cnt < 1) return HTKAMD_OK;
   htkamd_lat_align *al = (htkamd_lat_align *)calloc((size_t)cnt, sizeof(*al));
   if (!al) { htkamd_set_error("latset: out of memory"); return HTKAMD_ENOMEM; }
   const char *p = buf;
   int rc = HTKAMD_OK;
   for (int i = 0; i < cnt && !rc; i++) {
      if (*p != ':') { htkamd_set_error("%s: ReadAlign: ':' Expected at start of field %d in %s (8250)", path, i, buf); rc = HTKAMD_EMODEL; break; }
      const char *str = ++p;
      while (*p && *p != ':' && *p != ',') p++;
      if (!*p) { htkamd_set_error("%s: ReadAlign: Unexpected end of field %s (8250)", path, buf); rc = HTKAMD_EMODEL; break; }
      al[i].label = (char *)malloc((size_t)(p - str) + 1);
      if (!al[i].label) { htkamd_set_error("latset: out of memory"); rc = HTKAMD_ENOMEM; break; }
      memcpy(al[i].label, str, (size_t)(p - str)); al[i].label[p - str] = 0;
      char *e;
      if (*p == ',') {
         str = p + 1; al[i].dur = (float)strtod(str, &e); p = e;
         if (p == str || (*p != ':' && *p != ',')) { htkamd_set_error("%s: ReadAlign: Cannot read duration %d from field %s (8250)", path, i, buf); rc = HTKAMD_EMODEL; break; }
      }
      if (*p == ',') {
         str = p + 1; al[i].like = (float)strtod(str, &e); p = e;
         if (p == str || *p != ':') { htkamd_set_error("%s: ReadAlign: Cannot read like %d from field %s (8250)", path, i, buf); rc = HTKAMD_EMODEL; break; }
      }
   }
   if (rc) { align_free(al, cnt); return rc; }
   *out = al; *n = cnt;
   return HTKAMD_OK;
}

/* ConvLogLikeFromBase / ToBase (HNet.c:524) */
static double from_base(float base, double ll) { return base == 0.0f ? log(ll) : (base == 1.0f ? ll : ll * log(base)); }
static double to_base(float base, double ll) { return base == 0.0f ? exp(ll) : (base == 1.0f ? ll : ll / log(base)); }

/* ------------------------------------------------------------------------------------------ dictionary */
static unsigned hash_name(const char *s) { unsigned h = 2166136261u; for (; *s; s++) h = (h ^ (unsigned char)*s) * 16777619u; return h; }

static int dict_find(const htkamd_lat_dict *d, const char *name)
{
   if (!d->hashCap) return -1;
   for (unsigned h = hash_name(name) & (unsigned)(d->hashCap - 1);; h = (h + 1) & (unsigned)(d->hashCap - 1)) {
      const int w = d->hash[h];
      if (w < 0) return -1;
      if (!strcmp(d->word[w].name, name)) return w;
   }
}

static int dict_word(htkamd_lat_dict *d, const char *name)            /* GetWord(.., TRUE) */
{
   int w = dict_find(d, name);
   if (w >= 0) return w;
   if (2 * (d->nWords + 1) > d->hashCap) {
      const int cap = d->hashCap ? d->hashCap * 2 : 1024;
      int *h = (int *)malloc(sizeof(int) * (size_t)cap);
      if (!h) return -1;
      for (int i = 0; i < cap; i++) h[i] = -1;
      for (int i = 0; i < d->nWords; i++) {
         unsigned k = hash_name(d->word[i].name) & (unsigned)(cap - 1);
         while (h[k] >= 0) k = (k + 1) & (unsigned)(cap - 1);
         h[k] = i;
      }
      free(d->hash); d->hash = h; d->hashCap = cap;
   }
   if (d->nWords + 1 > d->capWords) {
      const int cap = d->capWords * 2 + 256;
      htkamd_lat_word *nw = (htkamd_lat_word *)realloc(d->word, sizeof(htkamd_lat_word) * (size_t)cap);
      if (!nw) return -1;
      d->word = nw; d->capWords = cap;
   }
   char *copy = strdup(name);
   if (!copy) return -1;
   w = d->nWords++;
   d->word[w].name = copy; d->word[w].nProns = 0; d->word[w].pron = NULL;
   unsigned k = hash_name(name) & (unsigned)(d->hashCap - 1);
   while (d->hash[k] >= 0) k = (k + 1) & (unsigned)(d->hashCap - 1);
   d->hash[k] = w;
   return w;
}

static void dict_release(htkamd_lat_dict *d)
{
   if (!d || --d->refs > 0) return;
   for (int i = 0; i < d->nWords; i++) {
      for (int k = 0; k < d->word[i].nProns; k++) free(d->word[i].pron[k].outSym);
      free(d->word[i].pron); free(d->word[i].name);
   }
   free(d->word); free(d->hash); free(d);
}

/* ReadDict / ReadDictWord (HDict.c:224-327): WORD ['['OUTSYM']'] [PRONPROB] PHONE ...; a pronunciation's number is its place in its
   word's list (NewPron :151) */
static int dict_read(htkamd_lat_dict *d, const char *path)
{
   size_t len; int why;
   char *txt = htx_read_file(path, &len, &why);
   if (!txt) {
      if (why == HTX_ENOMEM) { htkamd_set_error("latset_create: out of memory"); return HTKAMD_ENOMEM; }
      htkamd_set_error("latset_create: ReadDict: Can't open file %s (8010)", path); return HTKAMD_EIO;
   }
   htx_src s = {txt, txt + len, 0};
   htx_dict_entry e = {0};
   int rc;
   while ((rc = htx_dict_next(&s, path, &e)) == HTX_GOT) {
      rc = HTKAMD_ENOMEM;
      const int w = dict_word(d, e.word);
      if (w < 0) break;
      htkamd_lat_word *W = &d->word[w];
      htkamd_lat_pron *np = (htkamd_lat_pron *)realloc(W->pron, sizeof(htkamd_lat_pron) * (size_t)(W->nProns + 1));
      if (!np) break;
      W->pron = np;
      char *outSym = e.outKind == HTX_OUT_EMPTY ? NULL : strdup(e.outKind == HTX_OUT_GIVEN ? e.outSym : e.word);
      if (e.outKind != HTX_OUT_EMPTY && !outSym) break;
      W->pron[W->nProns].pnum = W->nProns + 1;
      W->pron[W->nProns].outSym = outSym;
      W->nProns++;
   }
   if (rc == HTKAMD_ENOMEM) htkamd_set_error("latset_create: out of memory");
   htx_dict_free(&e);
   free(txt);
   return rc == HTX_NONE ? HTKAMD_OK : rc;
}

/* ------------------------------------------------------------------------------------------ the set */
static const char *const unserved[][2] = {
   {"-n", "-n (expanding the lattice with an n-gram language model, LatExpand) is not supported"},
   {"-wn", "-wn (a word pair network applied to label lattices) is not supported"},
   {"-m", "-m (merging lattice nodes and arcs, MergeLatNodesArcs) is not supported"},
   {"-c", "-c (lattice statistics, CalcStats) is not supported"},
   {"-I", "-I (label files turned into lattices, LatticeFromLabels) is not supported"},
   {"-d", "-d (pronunciation probabilities taken from the dictionary, FixPronProbs) is not supported"},
   {"-P", "-P (a label output format other than HTK) is not supported"},
   {"FIXBADLATS", "FIXBADLATS (FixBadLat) is not supported"},
};
static const char *const served[] = {"-f", "-t", "-u", "-w", "-s", "-p", "-a", "-r", "-i", "-l", "-y", "-o", "-L", "-X", "-q", "-C", "-T", "STARTWORD", "ENDWORD", "SORTLATTICE"};

int htkamd_latset_check_switch(const char *sw)
{
   if (!sw) { htkamd_set_error("latset_check_switch: NULL argument"); return HTKAMD_EINVAL; }
   for (size_t i = 0; i < sizeof(served) / sizeof(served[0]); i++) if (!strcmp(sw, served[i])) return HTKAMD_OK;
   for (size_t i = 0; i < sizeof(unserved) / sizeof(unserved[0]); i++)
      if (!strcmp(sw, unserved[i][0])) { htkamd_set_error("hlrescore: %s", unserved[i][1]); return HTKAMD_EINVAL; }
   htkamd_set_error("HLRescore: Unknown switch %s (4019)", sw);
   return HTKAMD_EINVAL;
}

static int set_new(htkamd_lat_dict *d, struct htkamd_latset **out)
{
   struct htkamd_latset *s = (struct htkamd_latset *)calloc(1, sizeof(*s));
   if (!s) { htkamd_set_error("latset_create: out of memory"); return HTKAMD_ENOMEM; }
   s->dict = d; d->refs++;
   *out = s;
   return HTKAMD_OK;
}

int htkamd_latset_create(const char *dictPath, const char *startWord, const char *endWord, struct htkamd_latset **out)
{
   if (!dictPath || !out) { htkamd_set_error("latset_create: NULL argument"); return HTKAMD_EINVAL; }
   htkamd_lat_dict *d = (htkamd_lat_dict *)calloc(1, sizeof(*d));
   if (!d) { htkamd_set_error("latset_create: out of memory"); return HTKAMD_ENOMEM; }
   d->refs = 1;
   int rc = HTKAMD_OK;
   if (dict_word(d, "!NULL") != 0 || dict_word(d, "!SUBLATID") != 1) { htkamd_set_error("latset_create: out of memory"); rc = HTKAMD_ENOMEM; }      /* InitVocab (HDict.c:210) */
   if (!rc) rc = dict_read(d, dictPath);
   /* HLRescore.c:448-453: both boundary words must be names the tool has seen (the words and output symbols of the dictionary here) */
   const char *bw[2] = {startWord, endWord}, *bn[2] = {"STARTWORD", "ENDWORD"};
   for (int b = 0; b < 2 && !rc; b++) {
      if (!bw[b]) continue;
      int found = dict_find(d, bw[b]) >= 0;
      for (int w = 0; w < d->nWords && !found; w++)
         for (int k = 0; k < d->word[w].nProns && !found; k++) found = d->word[w].pron[k].outSym && !strcmp(d->word[w].pron[k].outSym, bw[b]);
      if (!found) { htkamd_set_error("HLRescore: cannot find %s '%s' (9999)", bn[b], bw[b]); rc = HTKAMD_EMODEL; }
   }
   if (!rc) rc = set_new(d, out);
   dict_release(d);
   return rc;
}

int htkamd_latset_create_like(const struct htkamd_latset *src, struct htkamd_latset **out)
{
   if (!src || !out) { htkamd_set_error("latset_create_like: NULL argument"); return HTKAMD_EINVAL; }
   return set_new(src->dict, out);
}

static void lat_free(htkamd_lat_one *l)
{
   for (int a = 0; l->arcAlign && a < l->na; a++) align_free(l->arcAlign[a], l->arcNAlign ? l->arcNAlign[a] : 0);
   free(l->arcAlign); free(l->arcNAlign);
   free(l->nodeTime); free(l->nodeWord); free(l->nodeVar); free(l->arcStart); free(l->arcEnd); free(l->arcAc); free(l->arcLm); free(l->arcPr);
   free(l->topOrder); free(l->fwdArcs); free(l->bwdArcs); free(l->utterance); free(l->vocab); free(l->hmms); free(l->lmName);
   memset(l, 0, sizeof(*l));
}

void htkamd_latset_destroy(struct htkamd_latset *s)
{
   if (!s) return;
   if (s->dev && s->devFree) s->devFree(s->dev);
   for (int u = 0; u < s->nLats; u++) lat_free(&s->lat[u]);
   free(s->lat);
   dict_release(s->dict);
   free(s);
}

int htkamd_latset_count(const struct htkamd_latset *s) { return s ? s->nLats : 0; }
double htkamd_latset_last_kernel_ms(const struct htkamd_latset *s) { return s ? s->kernelMs : 0.0; }
const char *htkamd_latset_word_name(const struct htkamd_latset *s, int w) { return (s && w >= 0 && w < s->dict->nWords) ? s->dict->word[w].name : NULL; }

static int lat_alloc(htkamd_lat_one *l, int nn, int na)
{
   memset(l, 0, sizeof(*l));
   l->nn = nn; l->na = na; l->logbase = 1.0f; l->tscale = 1.0f;
   const size_t N = (size_t)(nn > 0 ? nn : 1), A = (size_t)(na > 0 ? na : 1);
   l->nodeTime = (double *)calloc(N, sizeof(double)); l->nodeWord = (int *)calloc(N, sizeof(int)); l->nodeVar = (int *)calloc(N, sizeof(int));
   l->arcStart = (int *)calloc(A, sizeof(int)); l->arcEnd = (int *)calloc(A, sizeof(int));
   l->arcAc = (float *)calloc(A, sizeof(float)); l->arcLm = (float *)calloc(A, sizeof(float)); l->arcPr = (float *)calloc(A, sizeof(float));
   l->topOrder = (int *)calloc(N, sizeof(int)); l->fwdArcs = (int *)calloc(A, sizeof(int)); l->bwdArcs = (int *)calloc(A, sizeof(int));
   if (!l->nodeTime || !l->nodeWord || !l->nodeVar || !l->arcStart || !l->arcEnd || !l->arcAc || !l->arcLm || !l->arcPr || !l->topOrder || !l->fwdArcs || !l->bwdArcs) {
      lat_free(l); htkamd_set_error("latset: out of memory"); return HTKAMD_ENOMEM;
   }
   return HTKAMD_OK;
}

/* The orders.  lineOrder [na]: the arcs in the order their J= lines were read (NULL: by number): each joins the FRONT of its start node's
   foll list and of its end node's pred list (HNet.c:1189-1192, HLat.c:842-846). */
static int lat_prepare(htkamd_lat_one *l, const int *lineOrder, const char *what)
{
   const int nn = l->nn, na = l->na;
   int *foll = (int *)malloc(sizeof(int) * (size_t)(4 * nn + 2 * na + 4));
   if (!foll) { htkamd_set_error("latset: out of memory"); return HTKAMD_ENOMEM; }
   int *pred = foll + nn, *num = pred + nn, *stack = num + nn, *farc = stack + nn + 2, *parc = farc + na;
   for (int i = 0; i < nn; i++) { foll[i] = pred[i] = -1; num[i] = -1; }
   for (int i = 0; i < na; i++) {
      const int a = lineOrder ? lineOrder[i] : i;
      farc[a] = foll[l->arcStart[a]]; foll[l->arcStart[a]] = a;
      parc[a] = pred[l->arcEnd[a]]; pred[l->arcEnd[a]] = a;
   }
   l->start = l->end = -1;
   for (int i = 0; i < nn && l->start < 0; i++) if (pred[i] < 0) l->start = i;                /* LatStartNode */
   for (int i = 0; i < nn && l->end < 0; i++) if (foll[i] < 0) l->end = i;                    /* LatEndNode */
   int rc = HTKAMD_OK;
   if (l->start < 0) { htkamd_set_error("%s: HLat: lattice has no start node (8622)", what); rc = HTKAMD_EMODEL; }
   else if (l->end < 0) { htkamd_set_error("%s: HLat: lattice has no end node (8622)", what); rc = HTKAMD_EMODEL; }
   if (!rc) {
      /* LatTopSortVisit from the end node, without recursion: stack of nodes, `stack2` = the pred arc each will look at next */
      int *next = (int *)malloc(sizeof(int) * (size_t)(nn + 1)), sp = 0, time = -1;
      if (!next) { free(foll); htkamd_set_error("latset: out of memory"); return HTKAMD_ENOMEM; }
      stack[sp] = l->end; next[sp] = pred[l->end]; sp++; num[l->end] = -2;
      while (sp > 0) {
         const int a = next[sp - 1];
         if (a < 0) { num[stack[sp - 1]] = ++time; sp--; continue; }
         next[sp - 1] = parc[a];
         const int st = l->arcStart[a];
         if (num[st] == -1) { num[st] = -2; stack[sp] = st; next[sp] = pred[st]; sp++; }
      }
      free(next);
      if (time + 1 != nn) {
         htkamd_set_error("%s: LatTopSort: the end node is reached from %d of %d nodes (the reference's assertion time+1 == lat->nn fails)", what, time + 1, nn);
         rc = HTKAMD_EMODEL;
      }
      for (int a = 0; a < na && !rc; a++)
         if (!(num[l->arcStart[a]] < num[l->arcEnd[a]])) { htkamd_set_error("%s: LatTopSort: Lattice contains cycles (8622)", what); rc = HTKAMD_EMODEL; }
   }
   if (!rc) {
      for (int i = 0; i < nn; i++) l->topOrder[num[i]] = i;
      int k = 0;
      for (int i = 0; i < nn; i++) for (int a = foll[l->topOrder[i]]; a >= 0; a = farc[a]) l->fwdArcs[k++] = a;
      k = 0;
      for (int i = nn - 1; i >= 0; i--) for (int a = pred[l->topOrder[i]]; a >= 0; a = parc[a]) l->bwdArcs[k++] = a;
   }
   free(foll);
   return rc;
}

static int set_push(struct htkamd_latset *s, htkamd_lat_one *l)
{
   if (s->nLats + 1 > s->capLats) {
      const int cap = s->capLats * 2 + 64;
      htkamd_lat_one *nl = (htkamd_lat_one *)realloc(s->lat, sizeof(htkamd_lat_one) * (size_t)cap);
      if (!nl) { lat_free(l); htkamd_set_error("latset: out of memory"); return HTKAMD_ENOMEM; }
      s->lat = nl; s->capLats = cap;
   }
   s->lat[s->nLats] = *l;
   s->totalNodes += l->nn; s->totalArcs += l->na;
   return s->nLats++;
}

int htkamd_latset_add_file(struct htkamd_latset *s, const char *path)
{
   if (!s || !path) { htkamd_set_error("latset_add_file: NULL argument"); return HTKAMD_EINVAL; }
   size_t len; int why;
   char *txt = htx_read_file(path, &len, &why);
   if (!txt) {
      if (why == HTX_ENOMEM) { htkamd_set_error("latset: out of memory"); return HTKAMD_ENOMEM; }
      htkamd_set_error("HLRescore: Cannot open Lattice file %s (4010)", path); return HTKAMD_EIO;
   }
   htx_src src = {txt, txt + len, 0};
   char name[132], val[4200];
   htkamd_lat_one l;
   memset(&l, 0, sizeof(l));
   int nn = 0, na = 0, rc = HTKAMD_OK, t = 0, sized = 0;
   char *utt = NULL, *voc = NULL, *hmms = NULL, *lmn = NULL;
   float logbase = 1.0f, tscale = 1.0f;
   double v;
   int *lineOrder = NULL, *seenNode = NULL, *seenArc = NULL, nLines = 0, nodesLeft = 0, arcsLeft = 0, alabs = 1;
   /* header (HNet.c:904-948): ends at the first end of line after both N and L are known */
   while (!rc) {
      t = htx_slf_next_field(&src, path, name, sizeof(name), val, sizeof(val));
      if (t == HTX_F_ERR) { rc = HTKAMD_EMODEL; break; }
      if (t == HTX_F_EOF || t == HTX_F_DOT) { htkamd_set_error("%s: ReadLattice: Premature end of lattice file before header (8250)", path); rc = HTKAMD_EMODEL; break; }
      if (t == HTX_F_EOL) { if (na != 0 && nn != 0) break; continue; }
      if (!strcmp(name, "N")) { if (!(rc = htx_slf_number(val, &v, 1, path, 'N'))) nn = (int)v; }
      else if (!strcmp(name, "L")) { if (!(rc = htx_slf_number(val, &v, 1, path, 'L'))) na = (int)v; }
      else if (!strcmp(name, "UTTERANCE")) { free(utt); utt = strdup(val); }
      else if (!strcmp(name, "SUBLAT")) { htkamd_set_error("%s: SUBLAT=%s: multi-level lattices (sub-lattices) are not supported", path, val); rc = HTKAMD_EMODEL; }
      else if (!strcmp(name, "vocab")) { free(voc); voc = strdup(val); }
      else if (!strcmp(name, "hmms")) { free(hmms); hmms = strdup(val); }
      else if (!strcmp(name, "lmname")) { free(lmn); lmn = strdup(val); }
      else if (!strcmp(name, "base")) { if (!(rc = htx_slf_number(val, &v, 0, path, 'b'))) logbase = (float)v; }
      else if (!strcmp(name, "tscale")) { if (!(rc = htx_slf_number(val, &v, 0, path, 't'))) tscale = (float)v; }
      else if (!strcmp(name, "wdpenalty") || !strcmp(name, "lmscale") || !strcmp(name, "prscale") || !strcmp(name, "acscale")) rc = htx_slf_number(val, &v, 0, path, name[0] == 'w' ? 'p' : (name[0] == 'a' ? 'a' : 's'));
   }
   if (!rc && (nn < 0 || na < 0)) { htkamd_set_error("%s: ReadLattice: N=%d L=%d", path, nn, na); rc = HTKAMD_EMODEL; }
   if (!rc && logbase < 0.0f) { htkamd_set_error("%s: ReadLattice: Illegal log base in lattice (8251)", path); rc = HTKAMD_EMODEL; }
   if (!rc) rc = lat_alloc(&l, nn, na);
   if (!rc) {
      sized = 1;
      l.logbase = logbase; l.tscale = tscale;
      lineOrder = (int *)malloc(sizeof(int) * (size_t)(na + 1)); seenNode = (int *)calloc((size_t)nn + 1, sizeof(int)); seenArc = (int *)calloc((size_t)na + 1, sizeof(int));
      if (!lineOrder || !seenNode || !seenArc) { htkamd_set_error("latset: out of memory"); rc = HTKAMD_ENOMEM; }
      for (int i = 0; i < nn; i++) l.nodeVar[i] = -1;
      nodesLeft = nn; arcsLeft = na;
   }
   /* body (HNet.c:1004-1208) */
   while (!rc) {
      t = htx_slf_next_field(&src, path, name, sizeof(name), val, sizeof(val));
      if (t == HTX_F_ERR) { rc = HTKAMD_EMODEL; break; }
      if (t == HTX_F_EOF || t == HTX_F_DOT) break;
      if (t == HTX_F_EOL) continue;
      const int isNode = !strcmp(name, "I"), isArc = !strcmp(name, "J");
      int n = -1;
      if (isNode || isArc) {
         if ((rc = htx_slf_number(val, &v, 1, path, 'I'))) break;
         n = (int)v;
      }
      if (isNode) {
         if (n < 0 || n >= nn) { htkamd_set_error("%s: ReadLattice: Lattice does not contain node %d (8251)", path, n); rc = HTKAMD_EMODEL; break; }
         if (seenNode[n]) { htkamd_set_error("%s: ReadLattice: Duplicate info info for node %d (8251)", path, n); rc = HTKAMD_EMODEL; break; }
         double time = 0.0; int word = 0, var = -1;
         while (!rc && (t = htx_slf_next_field(&src, path, name, sizeof(name), val, sizeof(val))) == HTX_F_FIELD) {
            switch (name[0]) {
            case 't': if (!(rc = htx_slf_number(val, &v, 0, path, 't'))) { time = v; time *= tscale; } break;
            case 'W':
               word = dict_find(s->dict, val);
               if (word < 0) { htkamd_set_error("%s: ReadLattice: Word %s not in dict (8251)", path, val); rc = HTKAMD_EMODEL; }
               break;
            case 'L': htkamd_set_error("%s: node %d names the sub-lattice %s: multi-level lattices are not supported", path, n, val); rc = HTKAMD_EMODEL; break;
            case 'v': if (!(rc = htx_slf_number(val, &v, 1, path, 'v'))) var = (int)v; break;
            default: break;                                         /* s= (a tag) and anything else is passed over */
            }
         }
         if (t == HTX_F_ERR) rc = HTKAMD_EMODEL;
         if (rc) break;
         if (word != 0) alabs = 0;
         l.nodeTime[n] = time; l.nodeWord[n] = word; l.nodeVar[n] = var;
         seenNode[n] = 1; nodesLeft--;
      } else if (isArc) {
         if (n < 0 || n >= na) { htkamd_set_error("%s: ReadLattice: Lattice does not contain arc %d (8251)", path, n); rc = HTKAMD_EMODEL; break; }
         if (seenArc[n]) { htkamd_set_error("%s: ReadLattice: Duplicate info for arc %d (8251)", path, n); rc = HTKAMD_EMODEL; break; }
         int st = -1, en = -1, word = -1, var = -1;
         double ac = 0.0, lm = 0.0, pr = 0.0;
         while (!rc && (t = htx_slf_next_field(&src, path, name, sizeof(name), val, sizeof(val))) == HTX_F_FIELD) {
            switch (name[0]) {
            case 'S':
               if ((rc = htx_slf_number(val, &v, 1, path, 'S'))) break;
               st = (int)v;
               if (st < 0 || st >= nn) { htkamd_set_error("%s: ReadLattice: Lattice does not contain start node %d (8251)", path, st); rc = HTKAMD_EMODEL; }
               break;
            case 'E':
               if ((rc = htx_slf_number(val, &v, 1, path, 'E'))) break;
               en = (int)v;
               if (en < 0 || en >= nn) { htkamd_set_error("%s: ReadLattice: Lattice does not contain end node %d (8251)", path, en); rc = HTKAMD_EMODEL; }
               break;
            case 'W':
               word = dict_find(s->dict, val);
               if (word < 0 || word == 1) { htkamd_set_error("%s: ReadLattice: Word %s not in dict (8251)", path, val); rc = HTKAMD_EMODEL; }
               break;
            case 'v': if (!(rc = htx_slf_number(val, &v, 1, path, 'v'))) var = (int)v; break;
            case 'a': if (!(rc = htx_slf_number(val, &v, 0, path, 'a'))) ac = from_base(logbase, v); break;
            case 'l': if (!(rc = htx_slf_number(val, &v, 0, path, 'l'))) lm = from_base(logbase, v); break;
            case 'r': if (!(rc = htx_slf_number(val, &v, 0, path, 'r'))) pr = from_base(logbase, v); break;
            case 'd': {
               htkamd_lat_align *al; int nal;
               if ((rc = read_align(val, &al, &nal, path))) break;
               if (!l.arcAlign) {
                  l.arcAlign = (htkamd_lat_align **)calloc((size_t)na + 1, sizeof(*l.arcAlign)); l.arcNAlign = (int *)calloc((size_t)na + 1, sizeof(int));
                  if (!l.arcAlign || !l.arcNAlign) { align_free(al, nal); htkamd_set_error("latset: out of memory"); rc = HTKAMD_ENOMEM; break; }
               }
               align_free(l.arcAlign[n], l.arcNAlign[n]);
               l.arcAlign[n] = al; l.arcNAlign[n] = nal;
               break;
            }
            default: break;
            }
         }
         if (t == HTX_F_ERR) rc = HTKAMD_EMODEL;
         if (rc) break;
         if (st < 0 || en < 0 || (word < 0 && alabs)) { htkamd_set_error("%s: ReadLattice: Need to know S,E [and W] for arc %d (8250)", path, n); rc = HTKAMD_EMODEL; break; }
         if (alabs && l.nodeWord[en] == 0) { l.nodeWord[en] = word; l.nodeVar[en] = var; }
         if (word >= 0 && l.nodeWord[en] != word) {
            htkamd_set_error("%s: ReadLattice: Lattice arc (%d) W field (%s) different from node (%s) (8251)", path, n, s->dict->word[word].name, s->dict->word[l.nodeWord[en]].name);
            rc = HTKAMD_EMODEL; break;
         }
         l.arcStart[n] = st; l.arcEnd[n] = en; l.arcAc[n] = (float)ac; l.arcLm[n] = (float)lm; l.arcPr[n] = (float)pr;
         seenArc[n] = 1; lineOrder[nLines++] = n; arcsLeft--;
      } else {                                                      /* an unknown line: passed over */
         while ((t = htx_slf_next_field(&src, path, name, sizeof(name), val, sizeof(val))) == HTX_F_FIELD) {}
         if (t == HTX_F_ERR) rc = HTKAMD_EMODEL;
      }
      if (t == HTX_F_EOF || t == HTX_F_DOT) break;
   }
   if (!rc && (arcsLeft != 0 || (nodesLeft != 0 && nodesLeft != nn))) {
      htkamd_set_error("%s: ReadLattice: %d Arcs unseen and %d Nodes unseen (8250)", path, arcsLeft, nodesLeft); rc = HTKAMD_EMODEL;
   }
   if (!rc) {                                                       /* CheckStEndNodes (HNet.c:685) */
      int *deg = (int *)calloc(2 * (size_t)nn + 1, sizeof(int)), nStart = 0, nEnd = 0;
      if (!deg) { htkamd_set_error("latset: out of memory"); rc = HTKAMD_ENOMEM; }
      for (int a = 0; deg && a < na; a++) { deg[l.arcEnd[a]]++; deg[nn + l.arcStart[a]]++; }
      for (int i = 0; deg && i < nn; i++) { nStart += deg[i] == 0; nEnd += deg[nn + i] == 0; }
      free(deg);
      if (!rc && (nStart != 1 || nEnd != 1)) {
         htkamd_set_error("%s: ReadLattice: Start/End nodes incorrect: lattice has %d start nodes, %d end nodes (8252, 8250)", path, nStart, nEnd); rc = HTKAMD_EMODEL;
      }
   }
   if (!rc) rc = lat_prepare(&l, lineOrder, path);
   free(lineOrder); free(seenNode); free(seenArc); free(txt);
   if (rc) { if (sized) lat_free(&l); free(utt); free(voc); free(hmms); free(lmn); return rc; }
   l.utterance = utt; l.vocab = voc; l.hmms = hmms; l.lmName = lmn;
   return set_push(s, &l);
}

int htkamd_latset_add(struct htkamd_latset *s, const htkamd_lattice *lat, const struct htkamd_net *net)
{
   if (!s || !lat || !net || lat->nNodes < 2 || lat->nArcs < 1 || !lat->nodeFrame || !lat->nodePron || !lat->arcStart || !lat->arcEnd || !lat->arcAc || !lat->arcLm || !lat->arcPr) {
      htkamd_set_error("latset_add: bad argument"); return HTKAMD_EINVAL;
   }
   htkamd_lat_one l;
   int rc = lat_alloc(&l, lat->nNodes, lat->nArcs);
   if (rc) return rc;
   for (int i = 0; i < l.nn && !rc; i++) {
      const int pron = lat->nodePron[i];
      l.nodeTime[i] = lat->nodeFrame[i] * lat->frameDur;
      l.nodeWord[i] = 0; l.nodeVar[i] = -1;
      if (pron < 0) continue;
      const char *w = htkamd_net_word_name(net, pron);
      const int id = w ? dict_find(s->dict, w) : -1;
      if (id < 0) { htkamd_set_error("latset_add: ReadLattice: Word %s not in dict (8251)", w ? w : "?"); rc = HTKAMD_EMODEL; break; }
      l.nodeWord[i] = id; l.nodeVar[i] = htkamd_net_pron_num(net, pron);
   }
   for (int a = 0; a < l.na && !rc; a++) {
      if (lat->arcStart[a] < 0 || lat->arcStart[a] >= l.nn || lat->arcEnd[a] < 0 || lat->arcEnd[a] >= l.nn) { htkamd_set_error("latset_add: arc %d has bad end points", a); rc = HTKAMD_EINVAL; break; }
      l.arcStart[a] = lat->arcStart[a]; l.arcEnd[a] = lat->arcEnd[a]; l.arcAc[a] = lat->arcAc[a]; l.arcLm[a] = lat->arcLm[a]; l.arcPr[a] = lat->arcPr[a];
   }
   if (!rc) rc = lat_prepare(&l, NULL, "latset_add");
   if (rc) { lat_free(&l); return rc; }
   return set_push(s, &l);
}

static char *dup_or_null(const char *s) { return s ? strdup(s) : NULL; }

int htkamd_latset_add_pruned(struct htkamd_latset *dst, const struct htkamd_latset *src, int u, const unsigned char *keepNode, const unsigned char *keepArc)
{
   if (!dst || !src || u < 0 || u >= src->nLats || !keepNode || !keepArc || dst->dict != src->dict) {
      htkamd_set_error("latset_add_pruned: bad argument (the sets must share a dictionary: htkamd_latset_create_like)"); return HTKAMD_EINVAL;
   }
   const htkamd_lat_one *o = &src->lat[u];
   int nn = 0, na = 0;
   int *renum = (int *)malloc(sizeof(int) * (size_t)(o->nn + 1));
   if (!renum) { htkamd_set_error("latset: out of memory"); return HTKAMD_ENOMEM; }
   for (int i = 0; i < o->nn; i++) renum[i] = keepNode[i] ? nn++ : -1;
   for (int a = 0; a < o->na; a++) {
      if (!keepArc[a]) continue;
      if (renum[o->arcStart[a]] < 0 || renum[o->arcEnd[a]] < 0) { free(renum); htkamd_set_error("latset_add_pruned: arc %d of lattice %d is kept, one of its nodes is not", a, u); return HTKAMD_EINVAL; }
      na++;
   }
   htkamd_lat_one l;
   int rc = lat_alloc(&l, nn, na);
   if (rc) { free(renum); return rc; }
   for (int i = 0; i < o->nn; i++) {
      const int n = renum[i];
      if (n < 0) continue;
      l.nodeTime[n] = o->nodeTime[i]; l.nodeWord[n] = o->nodeWord[i]; l.nodeVar[n] = o->nodeVar[i];
   }
   for (int a = 0, k = 0; a < o->na; a++) {
      if (!keepArc[a]) continue;
      l.arcStart[k] = renum[o->arcStart[a]]; l.arcEnd[k] = renum[o->arcEnd[a]]; l.arcAc[k] = o->arcAc[a]; l.arcLm[k] = o->arcLm[a]; l.arcPr[k] = o->arcPr[a];
      k++;
   }
   free(renum);
   if (o->arcAlign && na > 0) {                                      /* the surviving arcs keep their alignment records */
      l.arcAlign = (htkamd_lat_align **)calloc((size_t)na, sizeof(*l.arcAlign)); l.arcNAlign = (int *)calloc((size_t)na, sizeof(int));
      int bad = !l.arcAlign || !l.arcNAlign;
      for (int a = 0, k = 0; !bad && a < o->na; a++) {
         if (!keepArc[a]) continue;
         const int n = o->arcNAlign[a];
         if (n > 0) {
            l.arcAlign[k] = (htkamd_lat_align *)calloc((size_t)n, sizeof(htkamd_lat_align));
            if (!l.arcAlign[k]) { bad = 1; break; }
            l.arcNAlign[k] = n;
            for (int i = 0; i < n; i++) {
               l.arcAlign[k][i] = o->arcAlign[a][i];
               if (!(l.arcAlign[k][i].label = strdup(o->arcAlign[a][i].label))) bad = 1;
            }
         }
         k++;
      }
      if (bad) { lat_free(&l); htkamd_set_error("latset: out of memory"); return HTKAMD_ENOMEM; }
   }
   l.logbase = o->logbase; l.tscale = o->tscale;
   rc = lat_prepare(&l, NULL, "latset_add_pruned");
   if (rc) { lat_free(&l); return rc; }
   l.utterance = dup_or_null(o->utterance); l.vocab = dup_or_null(o->vocab); l.hmms = dup_or_null(o->hmms); l.lmName = dup_or_null(o->lmName);
   return set_push(dst, &l);
}

int htkamd_latset_get(const struct htkamd_latset *s, int u, htkamd_latset_view *out)
{
   if (!s || !out || u < 0 || u >= s->nLats) { htkamd_set_error("latset_get: bad argument"); return HTKAMD_EINVAL; }
   const htkamd_lat_one *l = &s->lat[u];
   out->nNodes = l->nn; out->nArcs = l->na; out->start = l->start; out->end = l->end;
   out->nodeTime = l->nodeTime; out->nodeWord = l->nodeWord; out->nodeVar = l->nodeVar;
   out->arcStart = l->arcStart; out->arcEnd = l->arcEnd; out->arcAc = l->arcAc; out->arcLm = l->arcLm; out->arcPr = l->arcPr;
   out->topOrder = l->topOrder; out->fwdArcs = l->fwdArcs; out->bwdArcs = l->bwdArcs;
   return HTKAMD_OK;
}

/* ------------------------------------------------------------------------------------------ from paths to labels */
/* the label LatFindBest makes for the arc's end node (HLat.c:640-648), NULL for none */
static const char *out_label(const struct htkamd_latset *s, const htkamd_lat_one *l, int node)
{
   const int w = l->nodeWord[node];
   if (w == 0) return NULL;
   const htkamd_lat_word *W = &s->dict->word[w];
   for (int k = 0; k < W->nProns; k++) if (W->pron[k].pnum == l->nodeVar[node]) return W->pron[k].outSym;
   return W->name;
}

static int path_ok(const htkamd_lat_one *l, const int *arcs, int nArcs, const char *what)
{
   if (nArcs < 0 || (nArcs > 0 && !arcs)) { htkamd_set_error("%s: bad argument", what); return HTKAMD_EINVAL; }
   for (int i = 0; i < nArcs; i++) if (arcs[i] < 0 || arcs[i] >= l->na) { htkamd_set_error("%s: path arc %d is %d (the lattice has %d)", what, i, arcs[i], l->na); return HTKAMD_EINVAL; }
   return HTKAMD_OK;
}

int htkamd_latset_trans(const struct htkamd_latset *s, int u, const htkamd_lat_scales *sc, const int *arcs, int nArcs, htkamd_trans **out)
{
   if (!s || !sc || !out || u < 0 || u >= s->nLats) { htkamd_set_error("latset_trans: bad argument"); return HTKAMD_EINVAL; }
   const htkamd_lat_one *l = &s->lat[u];
   int rc = path_ok(l, arcs, nArcs, "latset_trans");
   if (rc) return rc;
   htkamd_trans *tr;
   if ((rc = htkamd_trans_create(0, &tr))) return rc;
   for (int i = 0; i < nArcs && !rc; i++) {
      const int a = arcs[i], e = l->arcEnd[a];
      const char *lab = out_label(s, l, e);
      if (!lab) continue;
      const float score = (float)htkamd_larc_tot_like(l->arcAc[a], l->arcLm[a], l->arcPr[a], sc->acScale, sc->lmScale, sc->prScale, sc->wordPen, l->nodeWord[e] == 0);
      rc = htkamd_trans_add(tr, l->nodeTime[l->arcStart[a]] * 1.0e7, l->nodeTime[e] * 1.0e7, lab, score, NULL, 0.0f, NULL, 0.0f);
   }
   if (rc) { htkamd_trans_free(tr); return rc; }
   *out = tr;
   return HTKAMD_OK;
}

int htkamd_latset_best_ids(const struct htkamd_latset *s, struct htkamd_results *r, int K, const int *nPath, const int *pathArcs, int *hypOff, int *hypIds, int cap)
{
   if (!s || !r || K < 0 || !nPath || !pathArcs || !hypOff || cap < 0 || (cap > 0 && !hypIds)) { htkamd_set_error("latset_best_ids: bad argument"); return HTKAMD_EINVAL; }
   const int U = s->nLats;
   long long n = 0;
   for (int k = 0; k < K; k++) {
      long long nodeOff = 0;
      for (int u = 0; u < U; u++) {
         const htkamd_lat_one *l = &s->lat[u];
         const int p = k * U + u, *arcs = pathArcs + (size_t)k * (size_t)s->totalNodes + nodeOff;
         const int rc = path_ok(l, arcs, nPath[p], "latset_best_ids");
         if (rc) return rc;
         hypOff[p] = (int)n;
         for (int i = 0; i < nPath[p]; i++) {
            const char *lab = out_label(s, l, l->arcEnd[arcs[i]]);
            if (!lab) continue;
            const int id = htkamd_results_label_id(r, lab);
            if (id < 0) return id;
            if (n < cap) hypIds[n] = id;
            n++;
         }
         nodeOff += l->nn;
      }
   }
   if (n > 0x7fffffff) { htkamd_set_error("latset_best_ids: %lld labels in one call", n); return HTKAMD_EINVAL; }
   hypOff[(size_t)K * U] = (int)n;
   return (int)n;
}

/* ------------------------------------------------------------------------------------------ WriteLattice */
static const htkamd_lat_one *g_lat;                /* qsort context (the reference's `slat`) */
static const double *g_score;

static int cmp_nodes(const void *v1, const void *v2)                 /* QSCmpNodes (HNet.c:448) */
{
   const int s1 = *(const int *)v1, s2 = *(const int *)v2;
   const double tdiff = g_lat->nodeTime[s1] - g_lat->nodeTime[s2], sdiff = g_score ? g_score[s1] - g_score[s2] : 0.0;
   if (tdiff == 0.0) { if (sdiff == 0.0) return s1 - s2; return sdiff > 0.0 ? 1 : -1; }
   return tdiff > 0.0 ? 1 : -1;
}
int htkamd_latset_write(const struct htkamd_latset *s, int u, const htkamd_lat_scales *sc, const double *nodeScore, const char *path, int format)
{
   if (!s || !sc || !path || u < 0 || u >= s->nLats) { htkamd_set_error("latset_write: bad argument"); return HTKAMD_EINVAL; }
   if (!format) format = HTKAMD_LAT_DEFAULT_ALIGN | HTKAMD_LAT_PRLIKE;      /* HLAT_DEFAULT | HLAT_PRLIKE (HLRescore.c:595) */
   if (format & (HTKAMD_LAT_LBIN | HTKAMD_LAT_ALABS)) { htkamd_set_error("latset_write: -q A / B are not supported"); return HTKAMD_EINVAL; }
   const htkamd_lat_one *l = &s->lat[u];
   FILE *f = fopen(path, "w");
   if (!f) { htkamd_set_error("ProcessLattice: Could not open file '%s' for lattice output (4014)", path); return HTKAMD_EIO; }
   fprintf(f, "VERSION=1.0\n");
   if (l->utterance) fprintf(f, "UTTERANCE=%s\n", l->utterance);
   if (l->lmName) fprintf(f, "lmname=%s\nlmscale=%-6.2f wdpenalty=%-6.2f\n", l->lmName, sc->lmScale, sc->wordPen);
   if (format & HTKAMD_LAT_PRLIKE) fprintf(f, "prscale=%-6.2f\n", sc->prScale);
   if (format & HTKAMD_LAT_ACLIKE) fprintf(f, "acscale=%-6.2f\n", sc->acScale);
   if (l->vocab) fprintf(f, "vocab=%s\n", l->vocab);
   if (l->hmms) fprintf(f, "hmms=%s\n", l->hmms);
   if (l->logbase != 1.0f) fprintf(f, "base=%f\n", l->logbase);
   if (l->tscale != 1.0f) fprintf(f, "tscale=%f\n", l->tscale);
   fprintf(f, "N=%-4d L=%-5d\n", l->nn, l->na);
   const int nn = l->nn, na = l->na;
   int *order = (int *)malloc(sizeof(int) * (size_t)(nn > na ? nn : na) + 4), *rorder = (int *)malloc(sizeof(int) * (size_t)nn + 4);
   if (!order || !rorder) { free(order); free(rorder); fclose(f); htkamd_set_error("latset: out of memory"); return HTKAMD_ENOMEM; }
   for (int i = 0; i < nn; i++) order[i] = i;
   g_lat = l; g_score = nodeScore;
   qsort(order, (size_t)nn, sizeof(int), cmp_nodes);
   for (int i = 0; i < nn; i++) {
      const int n = order[i];
      rorder[n] = i;
      fprintf(f, "I=%-4d ", i);
      if (format & HTKAMD_LAT_TIMES) fprintf(f, "t=%-5.2f ", (float)(l->nodeTime[n] / l->tscale));
      htkamd_slf_put_word(f, s->dict->word[l->nodeWord[n]].name);
      if ((format & HTKAMD_LAT_PRON) && l->nodeVar[n] >= 0) fprintf(f, "v=%-2d ", l->nodeVar[n]);
      fprintf(f, "\n");
   }
   htkamd_slf_sort_arcs(order, na, l->arcStart, l->arcEnd, rorder);
   for (int i = 0; i < na; i++) {
      const int a = order[i];
      fprintf(f, "J=%-5d S=%-4d E=%-4d ", i, rorder[l->arcStart[a]], rorder[l->arcEnd[a]]);
      if (format & HTKAMD_LAT_ACLIKE) fprintf(f, "a=%-9.2f ", (float)to_base(l->logbase, l->arcAc[a]));
      if ((format & HTKAMD_LAT_LMLIKE) && !l->lmName) { const float tl = l->arcLm[a] * sc->lmScale; fprintf(f, "l=%-8.2f ", (float)to_base(l->logbase, (float)(tl + sc->wordPen))); }
      else if (format & HTKAMD_LAT_LMLIKE) fprintf(f, "l=%-7.3f ", (float)to_base(l->logbase, l->arcLm[a]));
      if (format & HTKAMD_LAT_PRLIKE) fprintf(f, "r=%-6.2f ", (float)to_base(l->logbase, l->arcPr[a]));
      if ((format & HTKAMD_LAT_ALIGN) && l->arcAlign && l->arcNAlign[a] > 0) {                  /* OutputAlign (HNet.c:503) */
         fprintf(f, "d=:");
         for (int q = 0; q < l->arcNAlign[a]; q++) {
            fprintf(f, "%s", l->arcAlign[a][q].label);
            if (format & HTKAMD_LAT_ALDUR) fprintf(f, ",%.2f", l->arcAlign[a][q].dur);
            if (format & HTKAMD_LAT_ALLIKE) fprintf(f, ",%.2f", l->arcAlign[a][q].like);
            fprintf(f, ":");
         }
      }
      fprintf(f, "\n");
   }
   free(order); free(rorder);
   g_lat = NULL; g_score = NULL;
   if (fclose(f)) { htkamd_set_error("latset_write: write error on %s", path); return HTKAMD_EIO; }
   return HTKAMD_OK;
}
