/* lstats.c -- HLStats around the device's integer tables (csrc/lstats.hip): the word list as InitStats sorts it (HLStats.c:367), and every
 * floating-point step of the tool in the reference's types and statement order:
 *   htkamd_lstats_bigram_write   OutputBoBigram (:701) with BuildNEntry (:657) and WriteBoNGram (HLM.c:546), or OutputMatBigram (:790) with
 *                                WriteMatBigram (HLM.c:699); the -T 4 lines go to a trace file;
 *   htkamd_lstats_stats_write    OutputDurs (:587), OutputList (:610), OutputCounts (:558).
 * The sums over a predecessor's successors (tot, cnt, bsum, the entropies) are doubles added in the order of the reference's list, which
 * RebuildAETab (:631) leaves in DECREASING hash value of the bigram: ae_hash below.  With the table size a prime above every word id two
 * successors of one predecessor never share a slot, so the order does not depend on the corpus.
 */
#include <limits.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "../csrc/lstats.h"
#include "htktext.h"

/* the device side (csrc/lstats.hip): absent in a build of the host code alone */
#pragma weak htkamd_lstats_device
#pragma weak htkamd_lstats_device_free
#pragma weak htkamd_lstats_wave_cap
#pragma weak htkamd_lstats_group_cap

#define LN10 2.30258509299404568
#define AETABSIZE 87793u            /* hashsizes[0]: HLStats without -h */
#define log2x(x) (log(x) / log(2.0))
#define ent2(x) ((x) > 0.0 ? ((x) * log2x(x)) : 0.0)

typedef struct htkamd_lstats lstats;

/* wd_cmp (HLStats.c:343) between the words that are neither boundary label: those two are put at the ends by hand */
static int wd_cmp(const void *a, const void *b) { return strcmp(*(char *const *)a, *(char *const *)b); }

static void drop_counts(lstats *s)
{
   free(s->succ); free(s->cnt);
   s->succ = s->cnt = NULL; s->counted = 0;
}

void htkamd_lstats_destroy(lstats *s)
{
   if (!s) return;
   if (s->dev && htkamd_lstats_device_free) htkamd_lstats_device_free(s->dev);
   for (int i = 0; s->name && i <= s->lSize; i++) free(s->name[i]);
   free(s->name); free(s->count); free(s->pcount); free(s->durSum); free(s->durMin); free(s->durMax); free(s->rowOff);
   drop_counts(s);
   free(s);
}

int htkamd_lstats_create(const char *const *words, int nWords, const char *enterWord, const char *exitWord, lstats **out)
{
   if (!out || nWords < 0 || (nWords > 0 && !words)) { htkamd_set_error("lstats_create: bad argument"); return HTKAMD_EINVAL; }
   if (!enterWord) enterWord = "!ENTER";
   if (!exitWord) exitWord = "!EXIT";
   if (!strcmp(enterWord, exitWord)) { htkamd_set_error("lstats_create: the start and end labels are both %s", enterWord); return HTKAMD_EINVAL; }
   int hasEnter = 0, hasExit = 0;
   for (int i = 0; i < nWords; i++) {
      if (!words[i] || !words[i][0]) { htkamd_set_error("lstats_create: word %d of the list is empty", i); return HTKAMD_EINVAL; }
      hasEnter |= !strcmp(words[i], enterWord); hasExit |= !strcmp(words[i], exitWord);
   }
   const int n = nWords + !hasEnter + !hasExit;
   if (n > 65534) { htkamd_set_error("lstats_create: %d words (HLStats keeps a word id in 16 bits)", n); return HTKAMD_EINVAL; }
   lstats *s = (lstats *)calloc(1, sizeof(lstats));
   if (!s || !(s->name = (char **)calloc((size_t)n + 1, sizeof(char *)))) { free(s); htkamd_set_error("lstats_create: out of memory"); return HTKAMD_ENOMEM; }
   s->lSize = n;
   s->name[0] = strdup("!NULL");
   s->name[1] = strdup(enterWord); s->name[n] = strdup(exitWord);
   for (int i = 0, k = 2; i < nWords; i++) if (strcmp(words[i], enterWord) && strcmp(words[i], exitWord) && k < n) s->name[k++] = strdup(words[i]);
   for (int i = 0; i <= n; i++)
      if (!s->name[i]) {                                      /* out of memory, or a boundary label that the list holds twice */
         int twice = 0;
         for (int a = 0; a < nWords; a++) for (int b = a + 1; b < nWords; b++) twice |= !strcmp(words[a], words[b]);
         htkamd_set_error(twice ? "lstats_create: a boundary label is in the list twice" : "lstats_create: out of memory");
         htkamd_lstats_destroy(s);
         return twice ? HTKAMD_EINVAL : HTKAMD_ENOMEM;
      }
   if (n > 3) qsort(s->name + 2, (size_t)n - 2, sizeof(char *), wd_cmp);
   for (int i = 2; i <= n; i++)
      if (!strcmp(s->name[i], s->name[i - 1])) { htkamd_set_error("lstats_create: %s is in the list twice", s->name[i]); htkamd_lstats_destroy(s); return HTKAMD_EINVAL; }
   s->enterId = 1; s->exitId = n;
   const size_t V = (size_t)n + 1;
   s->count = (int *)calloc(V, sizeof(int)); s->pcount = (int *)calloc(V, sizeof(int)); s->rowOff = (int *)calloc(V + 1, sizeof(int));
   s->durSum = (long long *)calloc(V, sizeof(long long)); s->durMin = (long long *)calloc(V, sizeof(long long)); s->durMax = (long long *)calloc(V, sizeof(long long));
   if (!s->count || !s->pcount || !s->rowOff || !s->durSum || !s->durMin || !s->durMax) { htkamd_lstats_destroy(s); htkamd_set_error("lstats_create: out of memory"); return HTKAMD_ENOMEM; }
   *out = s;
   return HTKAMD_OK;
}

int htkamd_lstats_nwords(const lstats *s) { return s ? s->lSize : 0; }
const char *htkamd_lstats_word(const lstats *s, int id) { return (s && id >= 0 && id <= s->lSize) ? s->name[id] : NULL; }
double htkamd_lstats_last_kernel_ms(const lstats *s) { return s ? s->kernelMs : 0.0; }

int htkamd_lstats_id(const lstats *s, const char *name)
{
   if (!s || !name) return 0;
   if (!strcmp(name, s->name[s->enterId])) return s->enterId;
   if (!strcmp(name, s->name[s->exitId])) return s->exitId;
   int lo = 2, hi = s->lSize - 1;
   while (lo <= hi) {
      const int mid = (lo + hi) / 2, c = strcmp(name, s->name[mid]);
      if (c == 0) return mid;
      if (c < 0) hi = mid - 1; else lo = mid + 1;
   }
   return 0;
}

int htkamd_lstats_ids(const lstats *s, const htkamd_labels *l, int *ids, long long *start, long long *end)
{
   if (!s || !l || !ids) { htkamd_set_error("lstats_ids: NULL argument"); return HTKAMD_EINVAL; }
   const int n = htkamd_labels_count(l);
   for (int i = 0; i < n; i++) {
      ids[i] = htkamd_lstats_id(s, htkamd_labels_name(l, i));
      if (start) start[i] = htkamd_labels_start(l, i);
      if (end) end[i] = htkamd_labels_end(l, i);
   }
   return HTKAMD_OK;
}

/* what the counting leaves behind, however it was made */
static void finish_counts(lstats *s, int nUtt, int haveDur)
{
   const int V = s->lSize + 1;
   memcpy(s->pcount, s->count, sizeof(int) * (size_t)V);
   s->count[s->enterId] += nUtt; s->count[s->exitId] += nUtt;      /* GatherStats coerces both per utterance; pCntr is not touched */
   s->nUtt = nUtt; s->haveDur = haveDur; s->counted = 1;
}

int htkamd_lstats_count(lstats *s, int nUtt, const int *labOff, const int *labIds, const long long *start, const long long *end, void *stream)
{
   if (!s) { htkamd_set_error("lstats_count: NULL handle"); return HTKAMD_EINVAL; }
   if (!htkamd_lstats_device) { htkamd_set_error("lstats_count: this build has no device code"); return HTKAMD_ENODEV; }
   drop_counts(s);
   const int rc = htkamd_lstats_device(&s->dev, s->lSize + 1, nUtt, labOff, labIds, start, end, s->enterId, s->exitId, htkamd_lstats_wave_cap(), htkamd_lstats_group_cap(),
                                       s->count, s->durSum, s->durMin, s->durMax, s->rowOff, &s->succ, &s->cnt, &s->durOdd, &s->kernelMs, stream);
   if (rc) return rc;
   finish_counts(s, nUtt, start != NULL);
   return HTKAMD_OK;
}

int htkamd_lstats_probe(int V, int nUtt, const int *labOff, const int *labIds, const long long *start, const long long *end, int enterId, int exitId, int waveCap, int groupCap,
                        int *count, long long *durSum, long long *durMin, long long *durMax, int *rowOff, int *succ, int *cnt, int pairCap, void *stream)
{
   int *hs = NULL, *hc = NULL;
   if (!htkamd_lstats_device) { htkamd_set_error("lstats_probe: this build has no device code"); return HTKAMD_ENODEV; }
   if (pairCap < 0 || (pairCap > 0 && (!succ || !cnt))) { htkamd_set_error("lstats_probe: bad argument"); return HTKAMD_EINVAL; }
   int rc = htkamd_lstats_device(NULL, V, nUtt, labOff, labIds, start, end, enterId, exitId, waveCap, groupCap, count, durSum, durMin, durMax, rowOff, &hs, &hc, NULL, NULL, stream);
   if (!rc && rowOff[V] > pairCap) { htkamd_set_error("lstats_probe: %d table entries, room for %d", rowOff[V], pairCap); rc = HTKAMD_EINVAL; }
   if (!rc && hs) { memcpy(succ, hs, sizeof(int) * (size_t)rowOff[V]); memcpy(cnt, hc, sizeof(int) * (size_t)rowOff[V]); }
   free(hs); free(hc);
   return rc;
}

/* counts planted by the caller in place of a counting run: loop counts per word (what the device gives), the CSR table, the durations */
int htkamd_lstats_plant(lstats *s, int nUtt, const int *count, const int *rowOff, const int *succ, const int *cnt, const long long *durSum, const long long *durMin,
                        const long long *durMax)
{
   if (!s || nUtt < 0 || !count || !rowOff) { htkamd_set_error("lstats_plant: bad argument"); return HTKAMD_EINVAL; }
   const int V = s->lSize + 1;
   if (rowOff[0] != 0) { htkamd_set_error("lstats_plant: the rows do not start at 0"); return HTKAMD_EINVAL; }
   for (int r = 0; r < V; r++) if (rowOff[r + 1] < rowOff[r]) { htkamd_set_error("lstats_plant: the offsets of row %d run backwards", r); return HTKAMD_EINVAL; }
   const int n = rowOff[V];
   if (n > 0 && (!succ || !cnt)) { htkamd_set_error("lstats_plant: bad argument"); return HTKAMD_EINVAL; }
   for (int k = 0; k < n; k++) if (succ[k] < 0 || succ[k] >= V || cnt[k] < 1) { htkamd_set_error("lstats_plant: entry %d is word %d, %d times", k, succ[k], cnt[k]); return HTKAMD_EINVAL; }
   drop_counts(s);
   memcpy(s->count, count, sizeof(int) * (size_t)V);
   memcpy(s->rowOff, rowOff, sizeof(int) * ((size_t)V + 1));
   s->succ = (int *)malloc(sizeof(int) * (size_t)(n ? n : 1)); s->cnt = (int *)malloc(sizeof(int) * (size_t)(n ? n : 1));
   if (!s->succ || !s->cnt) { drop_counts(s); htkamd_set_error("lstats_plant: out of memory"); return HTKAMD_ENOMEM; }
   s->durOdd = 0;                                             /* (planted sums say nothing about single labels) */
   if (n) { memcpy(s->succ, succ, sizeof(int) * (size_t)n); memcpy(s->cnt, cnt, sizeof(int) * (size_t)n); }
   if (durSum && durMin && durMax) {
      memcpy(s->durSum, durSum, sizeof(long long) * (size_t)V); memcpy(s->durMin, durMin, sizeof(long long) * (size_t)V); memcpy(s->durMax, durMax, sizeof(long long) * (size_t)V);
   }
   finish_counts(s, nUtt, durSum && durMin && durMax);
   return HTKAMD_OK;
}

int htkamd_lstats_get(const lstats *s, int *count, int *pcount, long long *durSum, long long *durMin, long long *durMax, int *rowOff)
{
   if (!s || !s->counted) { htkamd_set_error("lstats_get: nothing has been counted"); return HTKAMD_EINVAL; }
   const size_t V = (size_t)s->lSize + 1;
   if (count) memcpy(count, s->count, sizeof(int) * V);
   if (pcount) memcpy(pcount, s->pcount, sizeof(int) * V);
   if (durSum) memcpy(durSum, s->durSum, sizeof(long long) * V);
   if (durMin) memcpy(durMin, s->durMin, sizeof(long long) * V);
   if (durMax) memcpy(durMax, s->durMax, sizeof(long long) * V);
   if (rowOff) memcpy(rowOff, s->rowOff, sizeof(int) * (V + 1));
   return HTKAMD_OK;
}

int htkamd_lstats_bigrams(const lstats *s, int *succ, int *cnt)
{
   if (!s || !s->counted) { htkamd_set_error("lstats_bigrams: nothing has been counted"); return HTKAMD_EINVAL; }
   const size_t n = (size_t)s->rowOff[s->lSize + 1];
   if (succ && n) memcpy(succ, s->succ, sizeof(int) * n);
   if (cnt && n) memcpy(cnt, s->cnt, sizeof(int) * n);
   return HTKAMD_OK;
}

/* ---- the bigram files ---- */

/* GetAEntry's slot of bigram (pred, word) (HLStats.c:444) */
static unsigned ae_hash(int word, int pred)
{
   unsigned hash = ((0u << 16) + (unsigned)word) % AETABSIZE;
   return ((hash << 16) + (unsigned)pred) % AETABSIZE;
}

typedef struct { int word, count; unsigned hash; } aent;
static int ae_cmp(const void *a, const void *b)
{
   const aent *x = (const aent *)a, *y = (const aent *)b;
   return x->hash < y->hash ? 1 : (x->hash > y->hash ? -1 : 0);
}
/* row i as RebuildAETab leaves aelists[i] */
static int ae_list(const lstats *s, int i, aent *e)
{
   const int b = s->rowOff[i], n = s->rowOff[i + 1] - b;
   for (int k = 0; k < n; k++) { e[k].word = s->succ[b + k]; e[k].count = s->cnt[b + k]; e[k].hash = ae_hash(e[k].word, i); }
   qsort(e, (size_t)n, sizeof(aent), ae_cmp);
   return n;
}

typedef struct { int word; float prob; } sent;
static int se_cmp(const void *a, const void *b) { return ((const sent *)a)->word - ((const sent *)b)->word; }

static void put_name(FILE *f, const char *name, int width) { htx_write_string(f, name, HTX_ESCAPE, width); }

static int write_backoff(const lstats *s, FILE *f, FILE *tr, float uniFloor, int bigThresh, float disCount)
{
   const int lSize = s->lSize, enter = s->enterId, exitI = s->exitId;
   int maxRow = 1;
   for (int i = 1; i <= lSize; i++) if (s->rowOff[i + 1] - s->rowOff[i] > maxRow) maxRow = s->rowOff[i + 1] - s->rowOff[i];
   float *uni = (float *)calloc((size_t)lSize + 1, sizeof(float)), *bowt = (float *)calloc((size_t)lSize + 1, sizeof(float));
   int *nse = (int *)calloc((size_t)lSize + 2, sizeof(int));
   sent *se = (sent *)calloc((size_t)(s->rowOff[lSize + 1] ? s->rowOff[lSize + 1] : 1), sizeof(sent));
   aent *ae = (aent *)calloc((size_t)maxRow, sizeof(aent));
   if (!uni || !bowt || !nse || !se || !ae) { free(uni); free(bowt); free(nse); free(se); free(ae); htkamd_set_error("lstats_bigram_write: out of memory"); return HTKAMD_ENOMEM; }
   int i, tot, nBig = 0;
   double uent, ent, bent;
   for (i = 1, tot = 0.0; i <= lSize; i++) {                  /* the unigrams first; `tot` is an int in the reference too */
      if (i == enter) uni[i] = 0.0;
      else if (s->count[i] < uniFloor) uni[i] = uniFloor;
      else uni[i] = s->count[i];
      tot += uni[i];
   }
   for (i = 1, uent = 0.0; i <= lSize; i++) {
      uni[i] = uni[i] / tot;
      uent -= ent2(uni[i]);
   }
   if (tr) fprintf(tr, "\n  UNIGRAM NEntry        - %4d foll, ent %.3f [= %.3f]\n\n  BIGRAMS NEntries\n", lSize, uent, pow(2.0, uent));
   for (i = 1, bent = 0.0; i <= lSize; i++) {                 /* BuildNEntry */
      sent *row = se + s->rowOff[i] - s->rowOff[1];
      const int n = ae_list(s, i, ae);
      double bw, bsum, cnt, total, prob;
      int k, m = 0;
      total = cnt = 0.0;
      bsum = 1.0;
      if (i != exitI)
         for (k = 0; k < n; k++) {
            total += ae[k].count;
            if (ae[k].word != 0 && ae[k].word != enter && ae[k].count > bigThresh)
               cnt += (ae[k].count - disCount), m++, bsum -= uni[ae[k].word];
         }
      const float bentArg = uent;                             /* BuildNEntry takes the unigram entropy, and returns the row's, as a float */
      if (m == 0) { bowt[i] = 0.0; ent = bentArg; }
      else {
         bw = (bsum > 0.0) ? (1.0 - cnt / total) / bsum : 0.0;
         ent = (bw > 0.0) ? bw * (bentArg - log2x(bw)) : 0.0;
         for (k = 0, m = 0; k < n; k++)
            if (ae[k].word != 0 && ae[k].word != enter && ae[k].count > bigThresh) {
               prob = ((double)ae[k].count - disCount) / total;
               row[m].word = ae[k].word;
               row[m].prob = log(prob);
               ent -= ent2(prob);
               prob = bw * uni[row[m].word];
               ent += ent2(prob);
               m++;
            }
         if (bw > 0.0) bowt[i] = log(bw);
         else bowt[i] = LZERO;
         qsort(row, (size_t)m, sizeof(sent), se_cmp);
      }
      ent = (float)ent;
      nse[i] = m; nBig += m;
      if (tr && i != exitI) {
         if (i == enter) bent += uni[exitI] * ent;
         else bent += uni[i] * ent;
         fprintf(tr, "   %-20s - %4d foll, ent %6.3f [= %6.2f]\n", s->name[i], m, ent, pow(2.0, ent));
      }
   }
   if (tr) fprintf(tr, "\n  BIGRAM: training data entropy %.3f (perplexity %.2f)\n", bent, pow(2.0, bent));
   for (i = 1; i <= lSize; i++) {
      if (uni[i] > 0) uni[i] = log(uni[i]);
      else uni[i] = LZERO;
   }
   /* WriteBoNGram */
   const float scale = 1.0 / LN10;
   fprintf(f, "\\data\\\nngram 1=%d\nngram 2=%d\n", lSize, nBig);
   fprintf(f, "\n\\1-grams:\n");
   for (i = 1; i <= lSize; i++) {
      const float p = uni[i] * scale;
      if (p < -99.999) fprintf(f, "%+6.3f", -99.999);
      else fprintf(f, "%+6.4f", p);
      fputc('\t', f); put_name(f, s->name[i], 0);
      if (nse[i] > 0) fprintf(f, "\t%+6.4f\n", (float)(bowt[i] * scale));
      else fprintf(f, "\n");
   }
   if (nBig > 0) {                                            /* (nsize is 1 when no bigram survived: CreateBoNGram stops at the first zero count) */
      fprintf(f, "\n\\2-grams:\n");
      for (i = 1; i <= lSize; i++) {
         const sent *row = se + s->rowOff[i] - s->rowOff[1];
         for (int k = 0; k < nse[i]; k++) {
            const float p = row[k].prob * scale;
            if (p < -99.999) fprintf(f, "%+6.3f", -99.999);
            else fprintf(f, "%+6.4f", p);
            fputc('\t', f); put_name(f, s->name[i], 0); fputc(' ', f); put_name(f, s->name[row[k].word], 0);
            fprintf(f, "\n");
         }
      }
   }
   fprintf(f, "\n\\end\\\n");
   free(uni); free(bowt); free(nse); free(se); free(ae);
   return HTKAMD_OK;
}

static int write_matrix(const lstats *s, FILE *f, FILE *tr, float bigFloor)
{
   const int lSize = s->lSize, enter = s->enterId, exitI = s->exitId;
   int maxRow = 1;
   for (int r = 1; r <= lSize; r++) if (s->rowOff[r + 1] - s->rowOff[r] > maxRow) maxRow = s->rowOff[r + 1] - s->rowOff[r];
   float *vec = (float *)calloc((size_t)lSize + 1, sizeof(float));
   aent *ae = (aent *)calloc((size_t)maxRow, sizeof(aent));
   if (!vec || !ae) { free(vec); free(ae); htkamd_set_error("lstats_bigram_write: out of memory"); return HTKAMD_ENOMEM; }
   double vsum, fsum, tot, scale;
   double ent, bent, prob, fent;
   int i, j, k, nf, tf = 0, nu, tu = 0, np, tp = 0, tn = 0;
   const float epsilon = 0.000001;
   if (tr) fprintf(tr, "\n  BIGRAMS from MatBigram\n");
   bent = 0.0;
   fent = ent2(bigFloor);
   for (i = 1; i <= lSize; i++) {
      const int n = ae_list(s, i, ae);
      for (k = 0, tot = 0.0; k < n; k++)
         if (ae[k].word != 0) tot += ae[k].count;
      fsum = (lSize - 1) * bigFloor; vsum = 0.0;
      for (k = 0; k < n; k++)
         if (ae[k].count / tot > bigFloor && ae[k].word != 0)
            fsum -= bigFloor, vsum += ae[k].count;
         else
            ae[k].count = 0;
      scale = (1.0 - fsum) / vsum;
      for (j = 1; j <= lSize; j++) {
         if (j == enter) vec[j] = 0.0;
         else if (tot == 0.0) vec[j] = 1.0 / (lSize - 1);
         else vec[j] = bigFloor;
      }
      for (k = 0; k < n; k++)
         if (ae[k].count > 0) vec[ae[k].word] = ae[k].count * scale;
      if (tr) {
         nf = nu = np = 0;
         if (tot == 0.0)
            ent = -log2x(1.0 / (lSize - 1)), prob = 1.0, nu = lSize - 1;
         else
            ent = -(lSize - 1) * fent, prob = bigFloor * (lSize - 1), nf += lSize - 1;
         for (k = 0; k < n; k++)
            if (ae[k].count > 0) {
               prob += vec[ae[k].word] - bigFloor;
               ent -= ent2(vec[ae[k].word]);
               ent += fent;
               nf--; np++;
            }
         if (i != exitI) {
            j = s->count[i];
            bent += j * ent; tn += j;
            if (tot == 0.0) fprintf(tr, "   %-20s - %4d unis, ent %6.3f [= %6.2f] (P=%7.5f)\n", s->name[i], nu, ent, pow(2.0, ent), prob);
            else fprintf(tr, "   %-20s - %4d foll, ent %6.3f [= %6.2f] (P=%7.5f)\n", s->name[i], np, ent, pow(2.0, ent), prob);
         }
         tf += nf; tu += nu; tp += np;
      }
      /* to logs, then WriteMatBigram's row */
      for (j = 1; j <= lSize; j++) vec[j] = ((vec[j] < MINLARG) ? LZERO : log(vec[j]));
      put_name(f, s->name[i], -8); fputc(' ', f);
      int rep = 0;
      double x = -1.0, y;
      for (j = 1; j <= lSize; j++) {
         y = (vec[j] < LSMALL) ? 0.0 : exp(vec[j]);
         if (fabs(y - x) <= epsilon) rep++;
         else {
            if (rep > 0) { fprintf(f, "*%d", rep + 1); rep = 0; }
            x = y;
            if (x == 0.0) fprintf(f, " 0");
            else if (x == 1.0) fprintf(f, " 1");
            else fprintf(f, " %e", x);
         }
      }
      if (rep > 0) fprintf(f, "*%d", rep + 1);
      fprintf(f, "\n");
   }
   if (tr) {
      bent /= tn;
      fprintf(tr, "\n  BIGRAM: training data entropy %.3f (perplexity %.2f)\n", bent, pow(2.0, bent));
      fprintf(tr, "         Estimated %d, floored %d, unigrammed %d for %d\n", tp, tf, tu, lSize);
   }
   free(vec); free(ae);
   return HTKAMD_OK;
}

int htkamd_lstats_bigram_write(const lstats *s, const char *path, int backoff, float uniFloor, int bigThresh, float bigFloor, double discount, const char *tracePath)
{
   if (!s || !path) { htkamd_set_error("lstats_bigram_write: NULL argument"); return HTKAMD_EINVAL; }
   if (!s->counted) { htkamd_set_error("lstats_bigram_write: nothing has been counted"); return HTKAMD_EINVAL; }
   if (uniFloor < 0.0f || uniFloor > 1000.0f) { htkamd_set_error("HLStats: -u %f is outside 0 .. 1000", uniFloor); return HTKAMD_EINVAL; }
   if (bigFloor < 0.0f || bigFloor > 1000.0f) { htkamd_set_error("HLStats: -f %f is outside 0 .. 1000", bigFloor); return HTKAMD_EINVAL; }
   if (bigThresh < 0 || bigThresh > 100) { htkamd_set_error("HLStats: -t %d is outside 0 .. 100", bigThresh); return HTKAMD_EINVAL; }
   FILE *f = fopen(path, "w");
   if (!f) { htkamd_set_error("lstats_bigram_write: cannot create %s", path); return HTKAMD_EIO; }
   FILE *tr = NULL;
   if (tracePath && !(tr = fopen(tracePath, "a"))) { fclose(f); htkamd_set_error("lstats_bigram_write: cannot open %s", tracePath); return HTKAMD_EIO; }
   const float disCount = discount;                           /* SetConfParms: a float filled from a double */
   int rc = backoff ? write_backoff(s, f, tr, uniFloor, bigThresh, disCount) : write_matrix(s, f, tr, bigFloor);
   if (tr && fclose(tr) && !rc) { htkamd_set_error("lstats_bigram_write: write error on %s", tracePath); rc = HTKAMD_EIO; }
   if (fclose(f) && !rc) { htkamd_set_error("lstats_bigram_write: write error on %s", path); rc = HTKAMD_EIO; }
   return rc;
}

/* ---- standard output ---- */

typedef struct { int word, count; } wcount;
static int cmp_count(const void *a, const void *b)             /* CmpWordInfo (HLStats.c:546) */
{
   const wcount *x = (const wcount *)a, *y = (const wcount *)b;
   return x->count == y->count ? y->word - x->word : x->count - y->count;
}

int htkamd_lstats_stats_write(const lstats *s, const char *path, int append, int flags, int countLimit, const char *listPath)
{
   if (!s || !s->counted) { htkamd_set_error("lstats_stats_write: nothing has been counted"); return HTKAMD_EINVAL; }
   if ((flags & (HTKAMD_LS_DURS | HTKAMD_LS_COUNTS)) && !path) { htkamd_set_error("lstats_stats_write: no output file"); return HTKAMD_EINVAL; }
   if ((flags & HTKAMD_LS_LIST) && !listPath) { htkamd_set_error("HLStats: Output label list file name expected"); return HTKAMD_EINVAL; }
   if ((flags & HTKAMD_LS_DURS) && !s->haveDur) { htkamd_set_error("lstats_stats_write: the durations (-d) need the labels' start and end times"); return HTKAMD_EINVAL; }
   if ((flags & HTKAMD_LS_COUNTS) && (countLimit < 0 || countLimit > 100000)) { htkamd_set_error("HLStats: -c %d is outside 0 .. 100000", countLimit); return HTKAMD_EINVAL; }
   const int lSize = s->lSize;
   if (flags & HTKAMD_LS_DURS) {
      /* HLStats adds each label's float duration (ticks / 10000.0, in ms) into a float; the integer sums give the same numbers exactly when
         every duration is a whole number of milliseconds and every word's sum stays below 2^24 ms.  Outside that the listing is not made. */
      if (s->durOdd > 0) { htkamd_set_error("lstats_stats_write: %d labels last no whole number of milliseconds: the duration listing (-d) would not be HLStats's", s->durOdd); return HTKAMD_EINVAL; }
      for (int i = 1; i <= lSize; i++)
         if (s->durSum[i] >= ((long long)1 << 24) * 10000) { htkamd_set_error("lstats_stats_write: the durations of %s add up to 2^24 ms or more: the duration listing (-d) would not be HLStats's float sum", s->name[i]); return HTKAMD_EINVAL; }
   }
   FILE *f = NULL;
   if (path && !(f = fopen(path, append ? "a" : "w"))) { htkamd_set_error("lstats_stats_write: cannot create %s", path); return HTKAMD_EIO; }
   if (flags & HTKAMD_LS_DURS) {                              /* OutputDurs */
      fprintf(f, "\nDuration Statistics:\n       Label   Count  AveDur  MinDur  MaxDur\n");
      for (int i = 1; i <= lSize; i++) {
         fprintf(f, "%12s %7d", s->name[i], s->count[i]);
         if (s->count[i] > 0 && i != s->enterId && i != s->exitId) {
            const float sumDur = (float)((double)s->durSum[i] / 10000.0);
            const float minDur = s->durMin[i] == LLONG_MAX ? 1E30 : (float)((float)s->durMin[i] / 10000.0);
            const float maxDur = s->durMax[i] <= 0 ? 0.0 : (float)((float)s->durMax[i] / 10000.0);
            fprintf(f, "%8.1f", sumDur / s->count[i]);
            if (minDur < 1E30) fprintf(f, "%8.1f", minDur);
            else fprintf(f, "%8s", "---");
            fprintf(f, "%8.1f", maxDur);
         }
         fprintf(f, "\n");
      }
      fprintf(f, "\n");
   }
   int rc = HTKAMD_OK;
   if (flags & HTKAMD_LS_LIST) {                              /* OutputList */
      FILE *lf = fopen(listPath, "w");
      if (!lf) { htkamd_set_error("OutputList: Cannot create label list file %s", listPath); rc = HTKAMD_EIO; }
      else {
         for (int i = 1; i <= lSize; i++) if (s->count[i] > 0) fprintf(lf, "%s\n", s->name[i]);
         if (fclose(lf)) { htkamd_set_error("lstats_stats_write: write error on %s", listPath); rc = HTKAMD_EIO; }
      }
   }
   if (!rc && (flags & HTKAMD_LS_COUNTS)) {                   /* OutputCounts: by count, equal counts in decreasing list order */
      wcount *order = (wcount *)malloc(sizeof(wcount) * (size_t)lSize);
      if (!order) { fclose(f); htkamd_set_error("lstats_stats_write: out of memory"); return HTKAMD_ENOMEM; }
      for (int i = 0; i < lSize; i++) { order[i].word = i + 1; order[i].count = s->count[i + 1]; }
      qsort(order, (size_t)lSize, sizeof(wcount), cmp_count);
      fprintf(f, "\nLogical Model Counts:\n       Label   LCount   PCount\n");
      for (int i = 0; i < lSize; i++) {
         const int w = order[i].word;
         if (s->count[w] > countLimit) break;
         fprintf(f, "%12s %8d %8d\n", s->name[w], s->count[w], s->pcount[w]);
      }
      fprintf(f, "\n");
      free(order);
   }
   if (f && fclose(f) && !rc) { htkamd_set_error("lstats_stats_write: write error on %s", path); rc = HTKAMD_EIO; }
   return rc;
}

/* The switches of HLStats this library serves; anything else the tool accepts is refused by name, before a device is touched. */
int htkamd_lstats_check_switch(const char *sw)
{
   static const char *served = "botufscdlIGLX";
   if (!sw || sw[0] != '-' || !sw[1] || sw[2]) { htkamd_set_error("HLStats: Bad switch %s; must be single letter", sw ? sw : "(null)"); return HTKAMD_EINVAL; }
   if (strchr(served, sw[1])) return HTKAMD_OK;
   if (sw[1] == 'p') htkamd_set_error("HLStats: -p (physical model counts) is not supported: the word list here maps no logical name to another physical one");
   else if (sw[1] == 'h') htkamd_set_error("HLStats: -h (hash table size) is not supported: the counting keeps no hash table, and the order of the sums follows the small table");
   else if (strchr("ACDSTV", sw[1])) htkamd_set_error("HLStats: -%c is not supported", sw[1]);
   else htkamd_set_error("HLStats: Unknown switch %s", sw);
   return HTKAMD_EINVAL;
}
