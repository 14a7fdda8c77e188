/* lstats_sanitize.c -- host/lstats.c and host/netbuild.c with a main of their own, for a build with -fsanitize=address,undefined
 * (tests/test_lstats_sanitize.py): a case of tests/golden/lm is read (word list, MLF), counted here as GatherStats counts, PLANTED, and the
 * bigram files, listings and the word loop are written; the bigram files are read back.  The device entries are stubs that refuse.
 *    lstats_sanitize CASEDIR OUTDIR */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <limits.h>
#include "htk_amd.h"

static char g_err[1024];
void htkamd_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap); }
const char *htkamd_last_error(void) { return g_err; }
int htkamd_lstats_wave_cap(void) { return 1024; }
int htkamd_lstats_group_cap(void) { return 8192; }
void htkamd_lstats_device_free(void *d) { (void)d; }
int htkamd_lstats_device(void **dev, int V, int nUtt, const int *o, const int *i, const long long *s, const long long *e, int a, int b, int w, int g, int *c, long long *ds,
                         long long *dn, long long *dx, int *ro, int **su, int **cn, int *odd, double *ms, void *st) { htkamd_set_error("no device in this build"); return HTKAMD_ENODEV; }
int htkamd_netbuild_device(int mode, int N, const int *ro, const int *su, const float *v, const float *rv, const float *u, const int *no, const int *rk, int en, int z, int bn,
                           int *S, int *E, float *L, int cap, int *n, double *ms, void *st) { htkamd_set_error("no device in this build"); return HTKAMD_ENODEV; }
/* host/net.c is not linked: the hand-over is not this program's subject */
int htkamd_labels_count(const htkamd_labels *l);

#define OK(x) do { if ((x) != HTKAMD_OK) { fprintf(stderr, "%s: %s\n", #x, g_err); return 1; } } while (0)

int main(int argc, char **argv)
{
   if (argc != 3) return 2;
   char path[4096], out[4096], lst[4096];
   char *words[512]; int nWords = 0;
   snprintf(path, sizeof(path), "%s/wordlist", argv[1]);
   FILE *f = fopen(path, "r");
   if (!f) return 2;
   char line[256];
   while (nWords < 512 && fscanf(f, "%255s", line) == 1) words[nWords++] = strdup(line);
   fclose(f);
   htkamd_lstats *s = NULL;
   OK(htkamd_lstats_create((const char *const *)words, nWords, NULL, NULL, &s));
   const int V = htkamd_lstats_nwords(s) + 1, enter = 1, exitI = V - 1;
   htkamd_mlf *mlf = NULL;
   snprintf(path, sizeof(path), "%s/labels.mlf", argv[1]);
   OK(htkamd_mlf_read(path, &mlf));
   int *count = calloc((size_t)V, sizeof(int)), *dense = calloc((size_t)V * V, sizeof(int));
   long long *dsum = calloc((size_t)V, sizeof(long long)), *dmin = malloc(sizeof(long long) * (size_t)V), *dmax = malloc(sizeof(long long) * (size_t)V);
   for (int w = 0; w < V; w++) { dmin[w] = LLONG_MAX; dmax[w] = LLONG_MIN; }
   const int nUtt = htkamd_mlf_count(mlf);
   for (int u = 0; u < nUtt; u++) {
      const htkamd_labels *l = htkamd_mlf_entry(mlf, u);
      const int n = htkamd_labels_count(l);
      int *ids = malloc(sizeof(int) * (size_t)(n + 1));
      long long *st = malloc(sizeof(long long) * (size_t)(n + 1)), *en = malloc(sizeof(long long) * (size_t)(n + 1));
      OK(htkamd_lstats_ids(s, l, ids, st, en));
      int a = 0, b = n, prev = enter;
      if (n && ids[0] == enter) a++;
      if (n && ids[n - 1] == exitI) b--;
      for (int p = a; p < b; p++) {
         const int w = ids[p];
         const long long d = en[p] - st[p];
         count[w]++; dsum[w] += d;
         if (d < dmin[w]) dmin[w] = d;
         if (d > dmax[w]) dmax[w] = d;
         if (w != enter && w != exitI) { dense[prev * V + w]++; prev = w; }
      }
      dense[prev * V + exitI]++;
      free(ids); free(st); free(en);
   }
   int *rowOff = calloc((size_t)V + 1, sizeof(int)), *succ = malloc(sizeof(int) * (size_t)V * V), *cnt = malloc(sizeof(int) * (size_t)V * V), k = 0;
   for (int p = 0; p < V; p++) {
      rowOff[p] = k;
      for (int w = 0; w < V; w++) if (dense[p * V + w]) { succ[k] = w; cnt[k++] = dense[p * V + w]; }
   }
   rowOff[V] = k;
   OK(htkamd_lstats_plant(s, nUtt, count, rowOff, succ, cnt, dsum, dmin, dmax));
   snprintf(out, sizeof(out), "%s/lists.out", argv[2]); snprintf(lst, sizeof(lst), "%s/lists.list", argv[2]); snprintf(path, sizeof(path), "%s/lists.bigram", argv[2]);
   OK(htkamd_lstats_stats_write(s, out, 0, HTKAMD_LS_DURS, 0, NULL));
   OK(htkamd_lstats_bigram_write(s, path, 1, 1.0f, 0, 0.0f, 0.5, out));
   OK(htkamd_lstats_stats_write(s, out, 1, HTKAMD_LS_LIST | HTKAMD_LS_COUNTS, 5, lst));
   htkamd_bigram *b = NULL;
   OK(htkamd_bigram_read(path, &b));
   printf("backoff %d words %d bigrams\n", htkamd_bigram_nwords(b), htkamd_bigram_nbigrams(b));
   htkamd_bigram_destroy(b);
   snprintf(path, sizeof(path), "%s/mat_f001.bigram", argv[2]); snprintf(out, sizeof(out), "%s/mat_f001.out", argv[2]);
   OK(htkamd_lstats_bigram_write(s, path, 0, 1.0f, 0, 0.01f, 0.5, out));
   OK(htkamd_bigram_read(path, &b));
   printf("matrix %d words\n", htkamd_bigram_nwords(b));
   htkamd_wordnet *net = NULL;
   if (htkamd_netbuild_bigram(b, (const char *const *)words, nWords, NULL, NULL, NULL, 0, &net, NULL) != HTKAMD_EMODEL) return 3;      /* the list lacks the boundary words */
   htkamd_bigram_destroy(b);
   OK(htkamd_netbuild_loop((const char *const *)words, nWords, "!ENTER", "!EXIT", &net));
   snprintf(path, sizeof(path), "%s/loop_t.slf", argv[2]);
   OK(htkamd_wordnet_write(net, path));
   htkamd_wordnet_destroy(net);
   if (htkamd_lstats_check_switch("-p") != HTKAMD_EINVAL || htkamd_netbuild_check_switch("-x") != HTKAMD_EINVAL) return 3;
   htkamd_lstats_destroy(s); htkamd_mlf_free(mlf);
   free(count); free(dense); free(dsum); free(dmin); free(dmax); free(rowOff); free(succ); free(cnt);
   for (int i = 0; i < nWords; i++) free(words[i]);
   return 0;
}
