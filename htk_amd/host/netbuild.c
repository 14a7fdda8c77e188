/* netbuild.c -- HBuild: the bigram files HLStats writes read back as HLM.c's ReadLModel reads them (ReadBoNGram :489, ReadMatBigram :623),
 * and HBuild's three flat word networks (ProcessWordLoop HBuild.c:299, ProcessBoBiGram :368, ProcessMatBiGram :463).  The arcs of the two
 * bigram networks are written by the device (csrc/netbuild.hip) from the model's tables; the word loop has 2 nWords + 3 arcs of three
 * values and is made here.  The network is an htkamd_lattice (htkamd_wordnet_lattice), written as SLF with the shared pieces of
 * host/slfout.c, and host/net.c expands it without a file (htkamd_net_build_lattice).
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "../csrc/lstats.h"
#include "htktext.h"

#pragma weak htkamd_netbuild_device      /* csrc/netbuild.hip: absent in a build of the host code alone */

#define LN10 2.30258509299404568

typedef struct htkamd_bigram bigram;
typedef struct htkamd_wordnet wordnet;

void htkamd_bigram_destroy(bigram *b)
{
   if (!b) return;
   for (int i = 0; b->name && i <= b->N; i++) free(b->name[i]);
   free(b->name); free(b->unigram); free(b->bowt); free(b->hasEntry); free(b->rowOff); free(b->succ); free(b->prob); free(b->mat);
   free(b);
}

static int str_cmp(const void *a, const void *b) { return strcmp(*(const char *const *)a, *(const char *const *)b); }
static int word_index(const bigram *b, const char *w) { for (int i = 1; i <= b->N; i++) if (b->name[i] && !strcmp(b->name[i], w)) return i; return 0; }

/* a name -> index table for the reader: sorted copies */
typedef struct { const char *name; int idx; } nidx;
static int nidx_cmp(const void *a, const void *b) { return strcmp(((const nidx *)a)->name, ((const nidx *)b)->name); }
static int nidx_find(const nidx *t, int n, const char *w)
{
   int lo = 0, hi = n - 1;
   while (lo <= hi) { const int mid = (lo + hi) / 2, c = strcmp(w, t[mid].name); if (!c) return t[mid].idx; if (c < 0) hi = mid - 1; else lo = mid + 1; }
   return 0;
}

static int get_line(htx_src *s, char *buf, size_t nb)        /* GetInLine */
{
   if (s->p >= s->end) return 0;
   size_t n = 0;
   while (s->p < s->end && *s->p != '\n') { if (n + 1 < nb) buf[n++] = *s->p; s->p++; }
   if (s->p < s->end) s->p++;
   buf[n] = 0;
   return 1;
}
static int sync_str(htx_src *s, char *buf, size_t nb, const char *str)
{
   while (strcmp(buf, str)) if (!get_line(s, buf, nb)) return 0;
   return 1;
}
/* ReadFloat in text form: white space, then a number; 0 when there is none */
static int get_float(htx_src *s, float *x)
{
   while (s->p < s->end && (*s->p == ' ' || *s->p == '\t' || *s->p == '\n' || *s->p == '\r')) s->p++;
   if (s->p >= s->end) return 0;
   char *e;
   *x = strtof(s->p, &e);
   if (e == s->p) return 0;
   s->p = e;
   return 1;
}
/* SkipWhiteSpace: returns whether a newline was passed (source.wasNewline) */
static int skip_white(htx_src *s)
{
   int nl = 0;
   while (s->p < s->end && (*s->p == ' ' || *s->p == '\t' || *s->p == '\n' || *s->p == '\r')) { nl |= *s->p == '\n'; s->p++; }
   return nl || s->p >= s->end;
}

#define LM_BAD(...) do { htkamd_set_error(__VA_ARGS__); rc = HTKAMD_EMODEL; goto done; } while (0)

static int read_backoff(bigram *b, htx_src *s, const char *path)
{
   char buf[1100], wd[300];
   int rc = HTKAMD_OK, counts[3] = {0, 0, 0}, j, k;
   char ch;
   nidx *tab = NULL;
   buf[0] = 0;
   get_line(s, buf, sizeof(buf));
   if (!sync_str(s, buf, sizeof(buf), "\\data\\")) LM_BAD("SyncStr: EOF searching for \\data\\ in %s", path);
   for (int i = 1; i <= 3; i++) {
      get_line(s, buf, sizeof(buf));
      if (sscanf(buf, "ngram %d%c%d", &j, &ch, &k) != 3 && i > 1) break;
      if (i != j || k == 0) LM_BAD("ReadBoNGram: %dGram count missing (%s)", i, buf);
      if (ch != '=') LM_BAD("%s: binary n-gram sections are not supported", path);
      if (i > 2) LM_BAD("ProcessBoBiGram: Not BiGram LM: Order = %d", i);
      counts[i] = k;
   }
   const int N = counts[1];
   if (N < 1 || N > 65534) LM_BAD("%s: %d unigrams", path, N);
   b->N = N;
   b->name = (char **)calloc((size_t)N + 1, sizeof(char *));
   b->unigram = (float *)calloc((size_t)N + 1, sizeof(float)); b->bowt = (float *)calloc((size_t)N + 1, sizeof(float));
   b->hasEntry = (int *)calloc((size_t)N + 1, sizeof(int)); b->rowOff = (int *)calloc((size_t)N + 2, sizeof(int));
   b->succ = (int *)calloc((size_t)counts[2] + 1, sizeof(int)); b->prob = (float *)calloc((size_t)counts[2] + 1, sizeof(float));
   if (!b->name || !b->unigram || !b->bowt || !b->hasEntry || !b->rowOff || !b->succ || !b->prob) { htkamd_set_error("bigram_read: out of memory"); rc = HTKAMD_ENOMEM; goto done; }
   if (!sync_str(s, buf, sizeof(buf), "\\1-grams:")) LM_BAD("SyncStr: EOF searching for \\1-grams: in %s", path);
   for (int g = 1; g <= N; g++) {
      float x;
      if (!get_float(s, &x)) LM_BAD("GetFloat: Float Expected in the 1-grams of %s", path);
      if (htx_read_string(s, 0, NULL, wd, sizeof(wd)) != HTX_GOT) LM_BAD("%s: word expected in 1-gram %d", path, g);
      if (!(b->name[g] = strdup(wd))) { htkamd_set_error("bigram_read: out of memory"); rc = HTKAMD_ENOMEM; goto done; }
      b->unigram[g] = x * LN10;
      if (!skip_white(s)) {
         if (!get_float(s, &x)) LM_BAD("GetFloat: Float Expected in the 1-grams of %s", path);
         b->bowt[g] = x * LN10; b->hasEntry[g] = 1;
      }
   }
   tab = (nidx *)malloc(sizeof(nidx) * (size_t)N);
   if (!tab) { htkamd_set_error("bigram_read: out of memory"); rc = HTKAMD_ENOMEM; goto done; }
   for (int g = 1; g <= N; g++) { tab[g - 1].name = b->name[g]; tab[g - 1].idx = g; }
   qsort(tab, (size_t)N, sizeof(nidx), nidx_cmp);
   for (int g = 1; g < N; g++) if (!strcmp(tab[g].name, tab[g - 1].name)) LM_BAD("ReadNGrams: Duplicate word (%s) in 1-gram list", tab[g].name);
   if (counts[2] > 0) {
      if (!sync_str(s, buf, sizeof(buf), "\\2-grams:")) LM_BAD("SyncStr: EOF searching for \\2-grams: in %s", path);
      int last = 0;
      for (int g = 1; g <= counts[2]; g++) {
         float x;
         int ndx[2];
         if (!get_float(s, &x)) LM_BAD("GetFloat: Float Expected in the 2-grams of %s", path);
         for (int i = 0; i < 2; i++) {
            if (htx_read_string(s, 0, NULL, wd, sizeof(wd)) != HTX_GOT) LM_BAD("%s: word expected in 2-gram %d", path, g);
            if (!(ndx[1 - i] = nidx_find(tab, N, wd))) LM_BAD("ReadNGrams: Unseen word (%s) in 2Gram", wd);
         }
         const int pred = ndx[1];
         if (!b->hasEntry[pred]) LM_BAD("ReadNGrams: Backoff weight not seen for %dth 2Gram", g);
         if (pred < last || (pred != last && b->rowOff[pred + 1] != 0)) LM_BAD("ReadNGrams: %dth 2Grams out of order", g);
         /* (rows in file order must be rows in word order for the CSR table: HLStats writes them so) */
         last = pred;
         b->rowOff[pred + 1]++;
         b->succ[g - 1] = ndx[0]; b->prob[g - 1] = x * LN10;
         if (!skip_white(s)) { if (!get_float(s, &x)) LM_BAD("GetFloat: Float Expected in the 2-grams of %s", path); }      /* (a bigram's own weight: no trigrams here) */
      }
      b->rowOff[1] = 0;
      for (int i = 1; i <= N; i++) b->rowOff[i + 1] += b->rowOff[i];
      for (int i = 1; i <= N; i++)                            /* qsort(le->se, .., se_cmp): successors by word */
         for (int a = b->rowOff[i] + 1; a < b->rowOff[i + 1]; a++) {
            const int w = b->succ[a]; const float p = b->prob[a];
            int q = a - 1;
            while (q >= b->rowOff[i] && b->succ[q] > w) { b->succ[q + 1] = b->succ[q]; b->prob[q + 1] = b->prob[q]; q--; }
            b->succ[q + 1] = w; b->prob[q + 1] = p;
         }
   }
   if (!sync_str(s, buf, sizeof(buf), "\\end\\")) LM_BAD("SyncStr: EOF searching for \\end\\ in %s", path);
done:
   free(tab);
   return rc;
}

/* ReadRow: numbers, each with an optional *count, to the end of the line */
static int read_row(htx_src *s, float *v, int N, int *rc, const char *path)
{
   int i = 0, nl = 0;
   while (!nl) {
      float x;
      int cnt = 1;
      if (!get_float(s, &x)) { htkamd_set_error("GetFloat: Float Expected in %s", path); *rc = HTKAMD_EMODEL; return 0; }
      if (s->p < s->end && *s->p == '*') { s->p++; char *e; cnt = (int)strtol(s->p, &e, 10); if (e == s->p) { htkamd_set_error("GetInt: Int Expected in %s", path); *rc = HTKAMD_EMODEL; return 0; } s->p = e; }
      nl = skip_white(s);
      for (int j = 0; j < cnt; j++) { i++; if (i <= N) v[i] = x; }
   }
   return i;
}

static int read_matrix(bigram *b, htx_src *s, const char *path)
{
   char wd[300];
   int rc = HTKAMD_OK, P = 0, p;
   float *first = (float *)calloc(65536, sizeof(float)), sum, x;
   if (!first) { htkamd_set_error("bigram_read: out of memory"); return HTKAMD_ENOMEM; }
   if (htx_read_string(s, 0, NULL, wd, sizeof(wd)) != HTX_GOT) LM_BAD("%s: not a bigram file", path);
   if (skip_white(s)) LM_BAD("ReadMatBigram: First row invalid (0 entries)");
   P = read_row(s, first, 65534, &rc, path);
   if (rc) goto done;
   if (P <= 0 || P > 65534) LM_BAD("ReadMatBigram: First row invalid (%d entries)", P);
   b->N = P;
   b->name = (char **)calloc((size_t)P + 1, sizeof(char *));
   b->mat = (float *)calloc((size_t)(P + 1) * (size_t)(P + 1), sizeof(float));
   if (!b->name || !b->mat) { htkamd_set_error("bigram_read: out of memory"); rc = HTKAMD_ENOMEM; goto done; }
   for (p = 1;; p++) {
      float *row = b->mat + (size_t)p * (size_t)(P + 1);
      if (p == 1) memcpy(row, first, sizeof(float) * ((size_t)P + 1));
      else {
         if (htx_read_string(s, 0, NULL, wd, sizeof(wd)) != HTX_GOT) break;
         if (p > P) LM_BAD("ReadMatBigram: More rows than columns in bigram %s", path);
         if (skip_white(s) || read_row(s, row, P, &rc, path) != P) { if (rc) goto done; LM_BAD("ReadMatBigram: Wrong number of items in row %d", p); }
      }
      if (!(b->name[p] = strdup(wd))) { htkamd_set_error("bigram_read: out of memory"); rc = HTKAMD_ENOMEM; goto done; }
      sum = 0.0;
      for (int j = 1; j <= P; j++) {
         x = row[j];
         if (x < 0) LM_BAD("ReadMatBigram: In bigram, entry %d for %s is -ve (%e)", j, wd, x);
         sum += x;
         row[j] = ((x < MINLARG) ? LZERO : log(x));
      }
   }
   if (P > p - 1) LM_BAD("ReadMatBigram: More columns than rows in bigram %s", path);
   {                                                          /* the names are looked at once, sorted, not row by row */
      const char **sorted = (const char **)malloc(sizeof(char *) * (size_t)P);
      if (!sorted) { htkamd_set_error("bigram_read: out of memory"); rc = HTKAMD_ENOMEM; goto done; }
      for (int i = 0; i < P; i++) sorted[i] = b->name[i + 1];
      qsort(sorted, (size_t)P, sizeof(char *), str_cmp);
      for (int i = 1; i < P && !rc; i++)
         if (!strcmp(sorted[i], sorted[i - 1])) { htkamd_set_error("ReadMatBigram: Duplicated name %s in bigram %s", sorted[i], path); rc = HTKAMD_EMODEL; }
      free(sorted);
   }
done:
   free(first);
   return rc;
}

int htkamd_bigram_read(const char *path, bigram **out)
{
   if (!path || !out) { htkamd_set_error("bigram_read: NULL argument"); return HTKAMD_EINVAL; }
   size_t len; int why = 0;
   char *txt = htx_read_file(path, &len, &why);
   if (!txt) { htkamd_set_error("ReadLModel: Can't open file %s", path); return why == HTX_ENOMEM ? HTKAMD_ENOMEM : HTKAMD_EIO; }
   bigram *b = (bigram *)calloc(1, sizeof(bigram));
   if (!b) { free(txt); htkamd_set_error("bigram_read: out of memory"); return HTKAMD_ENOMEM; }
   /* ReadLModel: a back-off file has a \data\ line among its first thousand */
   htx_src s = {txt, txt + len, 0};
   char buf[1100];
   int isBo = 0;
   for (int i = 0; i < 1000 && get_line(&s, buf, sizeof(buf)); i++) if (!strcmp(buf, "\\data\\")) { isBo = 1; break; }
   htx_src s2 = {txt, txt + len, 0};
   b->type = isBo ? HTKAMD_LM_BACKOFF : HTKAMD_LM_MATRIX;
   const int rc = isBo ? read_backoff(b, &s2, path) : read_matrix(b, &s2, path);
   free(txt);
   if (rc) { htkamd_bigram_destroy(b); return rc; }
   *out = b;
   return HTKAMD_OK;
}

int htkamd_bigram_type(const bigram *b) { return b ? b->type : -1; }
int htkamd_bigram_nwords(const bigram *b) { return b ? b->N : 0; }
const char *htkamd_bigram_word(const bigram *b, int i) { return (b && i >= 1 && i <= b->N) ? b->name[i] : NULL; }
int htkamd_bigram_nbigrams(const bigram *b) { return (b && b->rowOff) ? b->rowOff[b->N + 1] : 0; }
int htkamd_bigram_get(const bigram *b, float *unigram, float *bowt, int *hasEntry, int *rowOff, int *succ, float *prob, float *mat)
{
   if (!b) { htkamd_set_error("bigram_get: NULL handle"); return HTKAMD_EINVAL; }
   const size_t W = (size_t)b->N + 1;
   if (b->type == HTKAMD_LM_BACKOFF) {
      const size_t n = (size_t)b->rowOff[b->N + 1];
      if (unigram) memcpy(unigram, b->unigram, sizeof(float) * W);
      if (bowt) memcpy(bowt, b->bowt, sizeof(float) * W);
      if (hasEntry) memcpy(hasEntry, b->hasEntry, sizeof(int) * W);
      if (rowOff) memcpy(rowOff, b->rowOff, sizeof(int) * (W + 1));
      if (succ && n) memcpy(succ, b->succ, sizeof(int) * n);
      if (prob && n) memcpy(prob, b->prob, sizeof(float) * n);
   } else if (mat) memcpy(mat, b->mat, sizeof(float) * W * W);
   return HTKAMD_OK;
}

/* ---- networks ---- */

void htkamd_wordnet_destroy(wordnet *n)
{
   if (!n) return;
   for (int i = 0; n->word && i < n->nWords; i++) free(n->word[i]);
   free(n->word); free(n->nodeWord); free(n->nodeFrame); free(n->nodeLike); free(n->arcStart); free(n->arcEnd); free(n->arcLm); free(n->arcZero);
   free(n);
}

static wordnet *wordnet_new(int nNodes, int arcCap, int nWords)
{
   wordnet *n = (wordnet *)calloc(1, sizeof(wordnet));
   if (!n) return NULL;
   n->nNodes = nNodes; n->nWords = nWords;
   n->word = (char **)calloc((size_t)nWords + 1, sizeof(char *));
   n->nodeWord = (int *)calloc((size_t)nNodes + 1, sizeof(int)); n->nodeFrame = (int *)calloc((size_t)nNodes + 1, sizeof(int));
   n->nodeLike = (double *)calloc((size_t)nNodes + 1, sizeof(double));
   n->arcStart = (int *)calloc((size_t)arcCap + 1, sizeof(int)); n->arcEnd = (int *)calloc((size_t)arcCap + 1, sizeof(int));
   n->arcLm = (float *)calloc((size_t)arcCap + 1, sizeof(float));
   n->arcZero = (float *)calloc((size_t)arcCap + 1, sizeof(float));
   if (!n->word || !n->nodeWord || !n->nodeFrame || !n->nodeLike || !n->arcStart || !n->arcEnd || !n->arcLm || !n->arcZero) { htkamd_wordnet_destroy(n); return NULL; }
   return n;
}
/* lat->lmscale = 1.0, wdpenalty = 0.0, no times, no acoustic scores */
static void wordnet_finish(wordnet *n)
{
   htkamd_lattice *l = &n->lat;
   l->nNodes = n->nNodes; l->nArcs = n->nArcs;
   l->nodeFrame = n->nodeFrame; l->nodePron = n->nodeWord; l->nodeLike = n->nodeLike;
   l->arcStart = n->arcStart; l->arcEnd = n->arcEnd; l->arcAc = n->arcZero; l->arcLm = n->arcLm; l->arcPr = n->arcZero;
   l->lmScale = 1.0f; l->wordPen = 0.0f; l->prScale = 1.0f; l->frameDur = 0.0;
}

const htkamd_lattice *htkamd_wordnet_lattice(const wordnet *n) { return n ? &n->lat : NULL; }
int htkamd_wordnet_nwords(const wordnet *n) { return n ? n->nWords : 0; }
const char *htkamd_wordnet_word(const wordnet *n, int w) { return (n && w >= 0 && w < n->nWords) ? n->word[w] : NULL; }
double htkamd_wordnet_last_kernel_ms(const wordnet *n) { return n ? n->kernelMs : 0.0; }


/* The words in the order of the list.  (The reference walks its vocabulary's hash table, whose slots are the ADDRESSES of the names modulo
   701: its node order changes from run to run.  The network is the same one.) */
int htkamd_netbuild_loop(const char *const *words, int nWords, const char *bracketStart, const char *bracketEnd, wordnet **out)
{
   if (!words || nWords < 1 || !out || (bracketStart == NULL) != (bracketEnd == NULL)) { htkamd_set_error("netbuild_loop: bad argument"); return HTKAMD_EINVAL; }
   for (int i = 0; i < nWords; i++) if (!words[i] || !strcmp(words[i], "!NULL")) { htkamd_set_error("netbuild_loop: word %d of the list is empty or !NULL", i); return HTKAMD_EINVAL; }
   const int nNode = nWords + 4, nArc = nWords * 2 + 3;
   wordnet *n = wordnet_new(nNode, nArc, nWords + 2);
   if (!n) { htkamd_set_error("netbuild_loop: out of memory"); return HTKAMD_ENOMEM; }
   for (int i = 0; i < nWords; i++) {
      if (!(n->word[i] = strdup(words[i]))) { htkamd_wordnet_destroy(n); htkamd_set_error("netbuild_loop: out of memory"); return HTKAMD_ENOMEM; }
      n->nodeWord[2 + i] = i;
   }
   n->nodeWord[0] = n->nodeWord[1] = n->nodeWord[nNode - 1] = n->nodeWord[nNode - 2] = -1;
   n->nWords = nWords;
   int *S = n->arcStart, *E = n->arcEnd; float *L = n->arcLm;
   S[0] = 0; E[0] = 1; L[0] = 0.0;
   S[1] = nNode - 2; E[1] = nNode - 1; L[1] = 0.0;
   S[2] = nNode - 2; E[2] = 1; L[2] = 0.0;
   for (int i = 0; i < nWords; i++) { S[3 + i] = 1; E[3 + i] = 2 + i; L[3 + i] = log(1.0 / (float)(nWords)); }
   for (int i = 0; i < nWords; i++) { S[3 + nWords + i] = 2 + i; E[3 + nWords + i] = nNode - 2; L[3 + nWords + i] = 0.0; }
   if (bracketStart) {
      n->word[nWords] = strdup(bracketStart); n->word[nWords + 1] = strdup(bracketEnd); n->nWords = nWords + 2;
      n->nodeWord[0] = nWords; n->nodeWord[nNode - 1] = nWords + 1;
   }
   n->nArcs = nArc;
   wordnet_finish(n);
   *out = n;
   return HTKAMD_OK;
}

int htkamd_netbuild_bigram(const bigram *b, const char *const *words, int nWords, const char *enterWord, const char *exitWord, const char *unknownWord, int zapUnknown,
                           wordnet **out, void *stream)
{
   if (!b || !words || nWords < 1 || !out) { htkamd_set_error("netbuild_bigram: bad argument"); return HTKAMD_EINVAL; }
   if (!htkamd_netbuild_device) { htkamd_set_error("netbuild_bigram: this build has no device code"); return HTKAMD_ENODEV; }
   if (!enterWord) enterWord = "!ENTER";
   if (!exitWord) exitWord = "!EXIT";
   if (!unknownWord) unknownWord = "!NULL";
   const int N = b->N, bo = b->type == HTKAMD_LM_BACKOFF;
   const int enterIdx = word_index(b, enterWord), exitIdx = word_index(b, exitWord), zapIdx = zapUnknown ? word_index(b, unknownWord) : 0;
   const char *who = bo ? "ProcessBoBiGram" : "ProcessMatBiGram";
   if (bo ? !enterIdx : enterIdx != 1) { htkamd_set_error("%s: Bigram does not contain ENTER symbol %s", who, enterWord); return HTKAMD_EMODEL; }
   if (bo ? !exitIdx : exitIdx != N) { htkamd_set_error("%s: Bigram does not contain EXIT symbol %s", who, exitWord); return HTKAMD_EMODEL; }
   int *nodeOf = (int *)calloc((size_t)N + 1, sizeof(int)), *rowKeep = (int *)calloc((size_t)N + 1, sizeof(int));
   const char **sorted = (const char **)malloc(sizeof(char *) * (size_t)nWords);      /* the word list, for N look-ups */
   if (!nodeOf || !rowKeep || !sorted) { free(nodeOf); free(rowKeep); free(sorted); htkamd_set_error("netbuild_bigram: out of memory"); return HTKAMD_ENOMEM; }
   for (int i = 0; i < nWords; i++) sorted[i] = words[i] ? words[i] : "";
   qsort(sorted, (size_t)nWords, sizeof(char *), str_cmp);
   int j = bo ? 1 : 0, rc = HTKAMD_OK;
   nodeOf[0] = -1;
   for (int i = 1; i <= N && !rc; i++) {
      if (i == zapIdx) { nodeOf[i] = -1; continue; }
      if (strcmp(b->name[i], "!NULL") && !bsearch(&b->name[i], sorted, (size_t)nWords, sizeof(char *), str_cmp)) { htkamd_set_error("%s: Word %s in LM not in WordList", who, b->name[i]); rc = HTKAMD_EMODEL; break; }
      nodeOf[i] = j++;
      rowKeep[i] = bo ? i != exitIdx : i < N;
   }
   wordnet *n = NULL;
   if (!rc) {
      const int nNodes = j, arcCap = bo ? b->rowOff[N + 1] + 2 * N : N * N;
      n = wordnet_new(nNodes, arcCap, N + 1);
   }
   if (!rc && !n) { htkamd_set_error("netbuild_bigram: out of memory"); rc = HTKAMD_ENOMEM; }
   if (!rc) {
      n->nodeWord[0] = -1;
      for (int i = 1; i <= N; i++) {
         n->word[i] = strdup(b->name[i]);
         if (nodeOf[i] >= 0) n->nodeWord[nodeOf[i]] = strcmp(b->name[i], "!NULL") ? i : -1;
      }
      n->word[0] = strdup("!NULL");
      for (int i = 0; i <= N && !rc; i++) if (!n->word[i]) { htkamd_set_error("netbuild_bigram: out of memory"); rc = HTKAMD_ENOMEM; }
   }
   if (!rc) {
      const int arcCap = bo ? b->rowOff[N + 1] + 2 * N : N * N;
      rc = htkamd_netbuild_device(b->type, N, b->rowOff, b->succ, bo ? b->prob : b->mat, b->bowt, b->unigram, nodeOf, rowKeep, enterIdx, zapIdx, 0,
                                  n->arcStart, n->arcEnd, n->arcLm, arcCap, &n->nArcs, &n->kernelMs, stream);
   }
   free(nodeOf); free(rowKeep); free(sorted);
   if (rc) { htkamd_wordnet_destroy(n); return rc; }
   wordnet_finish(n);
   *out = n;
   return HTKAMD_OK;
}

int htkamd_netbuild_probe(int mode, int N, const int *rowOff, const int *succ, const float *val, const float *rowVal, const float *uni, const int *nodeOf, const int *rowKeep,
                          int enterIdx, int zapIdx, int backNode, int *arcStart, int *arcEnd, float *arcLm, int arcCap, int *nArcs, void *stream)
{
   if (!htkamd_netbuild_device) { htkamd_set_error("netbuild_probe: this build has no device code"); return HTKAMD_ENODEV; }
   return htkamd_netbuild_device(mode, N, rowOff, succ, val, rowVal, uni, nodeOf, rowKeep, enterIdx, zapIdx, backNode, arcStart, arcEnd, arcLm, arcCap, nArcs, NULL, stream);
}

/* WriteLattice with HBuild's format (HLAT_LMLIKE alone): no times, no lmname, so l= holds the arc's log probability to two decimals */
int htkamd_wordnet_write(const wordnet *n, const char *path)
{
   if (!n || !path) { htkamd_set_error("wordnet_write: NULL argument"); return HTKAMD_EINVAL; }
   FILE *f = fopen(path, "w");
   if (!f) { htkamd_set_error("SaveLattice : Cannot create new lattice file  %s", path); return HTKAMD_EIO; }
   const htkamd_lattice *lat = &n->lat;
   fprintf(f, "VERSION=1.0\nN=%-4d L=%-5d\n", lat->nNodes, lat->nArcs);
   int *rank = (int *)malloc(sizeof(int) * (size_t)lat->nNodes), *order = (int *)malloc(sizeof(int) * ((size_t)lat->nArcs + 1));
   for (int i = 0; i < lat->nNodes; i++) {                    /* QSCmpNodes: every time and score is 0, so the nodes keep their order */
      rank[i] = i;
      fprintf(f, "I=%-4d ", i);
      if (lat->nodePron[i] >= 0) htkamd_slf_put_word(f, n->word[lat->nodePron[i]]);
      else fprintf(f, "W=%-19s ", "!NULL");
      fprintf(f, "\n");
   }
   htkamd_slf_sort_arcs(order, lat->nArcs, lat->arcStart, lat->arcEnd, rank);
   for (int i = 0; i < lat->nArcs; i++) {
      const int a = order[i];
      const float tl = lat->arcLm[a] * lat->lmScale;
      fprintf(f, "J=%-5d S=%-4d E=%-4d l=%-8.2f \n", i, lat->arcStart[a], lat->arcEnd[a], (float)(tl + lat->wordPen));
   }
   free(rank); free(order);
   if (fclose(f)) { htkamd_set_error("wordnet_write: write error on %s", path); return HTKAMD_EIO; }
   return HTKAMD_OK;
}

/* The switches of HBuild this library serves; the rest is refused by name. */
int htkamd_netbuild_check_switch(const char *sw)
{
   if (!sw || sw[0] != '-' || !sw[1] || sw[2]) { htkamd_set_error("HBuild: Bad switch %s; must be single letter", sw ? sw : "(null)"); return HTKAMD_EINVAL; }
   if (strchr("mnstuz", sw[1])) return HTKAMD_OK;
   switch (sw[1]) {
   case 'x': htkamd_set_error("HBuild: -x (multi-level lattices) is not supported"); break;
   case 'w': htkamd_set_error("HBuild: -w (word-pair grammars) is not supported"); break;
   case 'L': case 'j': htkamd_set_error("HBuild: -%c (lattice input) is not supported", sw[1]); break;
   case 'b': htkamd_set_error("HBuild: -b (binary lattice output) is not supported"); break;
   default: htkamd_set_error("HBuild: Unknown switch %s", sw);
   }
   return HTKAMD_EINVAL;
}
