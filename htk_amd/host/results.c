/* results.c -- the host side of htkamd_results_* (csrc/results.hip aligns and counts): label names -> ids as HResults normalises them,
 * the reference transcriptions, the refusals, and every line of text HResults prints, from numbers alone.  Pure C, no device.
 *   names        AddEquiv / NormaliseName HResults.c:346-394, TriStrip HLabel.c:1021, ReadHMMList :1121, Initialise :1703
 *   references   MatchFiles :1720, MakeFN HShell.c:1739
 *   text         PrintBar :558, PClip :592, PrintHeader :609, PrintFileStats :656, PrintGlobalStats :730, OutTrans :1080, OutConMat :1191
 */
#include <ctype.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "../csrc/results.h"

#define RES_MAXCONMAT 200                 /* MAXCONMATSIZE :1165 */
#define RES_WIDTH     66                  /* htkWidth :428 */
#define RES_MAXWORD   5                   /* maxWordLen :84 */

/* ---- the switches of HResults this path does not have ------------------------------------------------------------------------- */

int htkamd_results_check_switch(const char *sw)
{
   static const struct { char c; const char *what; } out[] = {
      { 'w', "word spotting" }, { 'u', "word spotting (false alarm time units)" }, { 'k', "per-speaker results" }, { 'h', "the NIST output format" },
      { 'd', "N-best scoring" }, { 'm', "a limit on the number of files" }, { 'j', "a limit on the number of files" },
      { 'a', "renaming the phrase label" }, { 'b', "renaming the phone label" } };
   static const char in[] = "ecsznftpILX";
   if (!sw || sw[0] != '-' || !sw[1] || sw[2]) { htkamd_set_error("results: bad switch %s; must be a single letter", sw ? sw : "(null)"); return HTKAMD_EINVAL; }
   if (strchr(in, sw[1])) return HTKAMD_OK;
   for (size_t k = 0; k < sizeof(out) / sizeof(out[0]); k++)
      if (out[k].c == sw[1]) { htkamd_set_error("results: switch -%c (%s) is not supported", sw[1], out[k].what); return HTKAMD_EINVAL; }
   htkamd_set_error("results: unknown switch -%c", sw[1]);
   return HTKAMD_EINVAL;
}

/* ---- names -------------------------------------------------------------------------------------------------------------------- */

static unsigned hash_of(const char *s)
{
   unsigned h = 2166136261u;
   for (; *s; s++) h = (h ^ (unsigned char)*s) * 16777619u;
   return h;
}

static int hash_grow(struct htkamd_results *r)
{
   const int cap = r->hashCap ? r->hashCap * 2 : 256;
   int *h = (int *)malloc(sizeof(int) * (size_t)cap);
   if (!h) return HTKAMD_ENOMEM;
   for (int k = 0; k < cap; k++) h[k] = -1;
   for (int k = 0; k < r->hashCap; k++) {
      if (r->hash[k] < 0) continue;
      unsigned p = hash_of(r->name[r->hash[k]]) & (unsigned)(cap - 1);
      while (h[p] >= 0) p = (p + 1) & (unsigned)(cap - 1);
      h[p] = r->hash[k];
   }
   free(r->hash); r->hash = h; r->hashCap = cap;
   return HTKAMD_OK;
}

/* the id of `s` as it stands; add: a new name gets the next id; overwrite: the name's entry is given to a new id (a list's repeated name) */
static int name_id(struct htkamd_results *r, const char *s, int add, int overwrite)
{
   if (!strcmp(s, r->nullName) && !overwrite) return 0;
   if ((r->nNames + 1) * 2 > r->hashCap && hash_grow(r) != HTKAMD_OK) { htkamd_set_error("results: out of memory"); return HTKAMD_ENOMEM; }
   unsigned p = hash_of(s) & (unsigned)(r->hashCap - 1);
   while (r->hash[p] >= 0 && strcmp(r->name[r->hash[p]], s)) p = (p + 1) & (unsigned)(r->hashCap - 1);
   if (r->hash[p] >= 0 && !overwrite) return r->hash[p];
   if (!add) return -1;
   if (r->nNames + 1 > r->capNames) {
      const int cap = r->capNames * 2 + 64;
      char **n = (char **)realloc(r->name, sizeof(char *) * (size_t)cap);
      if (!n) { htkamd_set_error("results: out of memory"); return HTKAMD_ENOMEM; }
      r->name = n; r->capNames = cap;
   }
   if (!(r->name[r->nNames] = strdup(s))) { htkamd_set_error("results: out of memory"); return HTKAMD_ENOMEM; }
   if (strcmp(s, r->nullName)) r->hash[p] = r->nNames;          /* the null class's name, where a list has it, keeps id 0 */
   return r->nNames++;
}

int htkamd_results_label_id(htkamd_results *r, const char *name)
{
   char buf[256];
   if (!r || !name) { htkamd_set_error("results_label_id: NULL argument"); return HTKAMD_EINVAL; }
   if (strlen(name) >= sizeof(buf)) { htkamd_set_error("results: label name %.40s... is too long", name); return HTKAMD_EINVAL; }
   const char *s = name;
   if (r->strip) {                                               /* TriStrip: behind the first '-', before the last '+' */
      const char *p = strchr(name, '-');
      strcpy(buf, p ? p + 1 : name);
      char *q = strrchr(buf, '+');
      if (q) *q = 0;
      s = buf;
   }
   for (int e = r->nEquiv - 1; e >= 0; e--)                      /* eqlist is built at its head: the last -e is applied first */
      if (!strcmp(s, r->eqLabel[e])) s = r->eqClass[e];
   if (r->ignoreCase) {
      const char *p = s;
      while (*p && !islower((unsigned char)*p)) p++;
      if (*p) {
         if (s != buf) { if (strlen(s) >= sizeof(buf)) { htkamd_set_error("results: label name %.40s... is too long", s); return HTKAMD_EINVAL; } strcpy(buf, s); }
         for (char *q = buf; *q; q++) *q = (char)toupper((unsigned char)*q);
         s = buf;
      }
   }
   return name_id(r, s, 1, 0);
}

const char *htkamd_results_label_name(const htkamd_results *r, int id) { return (r && id >= 0 && id < r->nNames) ? r->name[id] : NULL; }
int htkamd_results_num_labels(const htkamd_results *r) { return r ? r->nNames : 0; }

void htkamd_results_destroy(htkamd_results *r)
{
   if (!r) return;
   if (r->dev && r->devFree) r->devFree(r->dev);
   for (int k = 0; k < r->nEquiv; k++) { free(r->eqClass[k]); free(r->eqLabel[k]); }
   for (int k = 0; k < r->nNames; k++) free(r->name[k]);
   for (int k = 0; k < r->nRefs; k++) free(r->refName[k]);
   free(r->eqClass); free(r->eqLabel); free(r->name); free(r->hash); free(r->refName); free(r->refOff); free(r->refIds); free(r->nullName); free(r);
}

int htkamd_results_create(const htkamd_results_config *cfg, htkamd_results **out)
{
   if (!cfg || !out) { htkamd_set_error("results_create: NULL argument"); return HTKAMD_EINVAL; }
   if (cfg->refLevel != 0 || cfg->testLevel != 0) {
      htkamd_set_error("results: label level %d is not supported (REFLEVEL / TESTLEVEL: only level 0 is scored)", cfg->refLevel ? cfg->refLevel : cfg->testLevel);
      return HTKAMD_EINVAL;
   }
   if (cfg->nEquiv < 0 || cfg->nList < 0 || (cfg->nEquiv > 0 && (!cfg->equivClass || !cfg->equivLabel)) || (cfg->nList > 0 && !cfg->list)) {
      htkamd_set_error("results_create: bad argument"); return HTKAMD_EINVAL;
   }
   struct htkamd_results *r = (struct htkamd_results *)calloc(1, sizeof(*r));
   if (!r) { htkamd_set_error("results: out of memory"); return HTKAMD_ENOMEM; }
   r->nullName = strdup(cfg->nullName ? cfg->nullName : "???");
   r->ignoreCase = cfg->ignoreCase != 0; r->strip = cfg->stripContexts != 0; r->nist = cfg->nist != 0;
   r->eqClass = (char **)calloc((size_t)cfg->nEquiv + 1, sizeof(char *)); r->eqLabel = (char **)calloc((size_t)cfg->nEquiv + 1, sizeof(char *));
   r->refOff = (int *)calloc(1, sizeof(int));
   if (!r->nullName || !r->eqClass || !r->eqLabel || !r->refOff) { htkamd_results_destroy(r); htkamd_set_error("results: out of memory"); return HTKAMD_ENOMEM; }
   for (int k = 0; k < cfg->nEquiv; k++) {
      if (!cfg->equivClass[k] || !cfg->equivLabel[k]) { htkamd_results_destroy(r); htkamd_set_error("results_create: equivalence %d has a NULL name", k); return HTKAMD_EINVAL; }
      r->eqClass[k] = strdup(cfg->equivClass[k]); r->eqLabel[k] = strdup(cfg->equivLabel[k]); r->nEquiv = k + 1;
   }
   int rc = name_id(r, r->nullName, 1, 1);                       /* id 0 */
   for (int k = 0; k < cfg->nList && rc >= 0; k++) {
      if (!cfg->list[k]) { htkamd_results_destroy(r); htkamd_set_error("results_create: list name %d is NULL", k); return HTKAMD_EINVAL; }
      rc = name_id(r, cfg->list[k], 1, 1);                       /* as they stand; a name given twice answers to its last place (Index :1151) */
   }
   if (rc < 0) { htkamd_results_destroy(r); return rc; }
   r->nList = cfg->nList;
   *out = r;
   return HTKAMD_OK;
}

/* ---- references --------------------------------------------------------------------------------------------------------------- */

int htkamd_results_find_ref(const htkamd_results *r, const char *utt)
{
   if (!r || !utt) return -1;
   for (int k = 0; k < r->nRefs; k++) if (!strcmp(r->refName[k], utt)) return k;
   return -1;
}

int htkamd_results_ref_len(const htkamd_results *r, int ref) { return (r && ref >= 0 && ref < r->nRefs) ? r->refOff[ref + 1] - r->refOff[ref] : -1; }

static int ref_room(struct htkamd_results *r, int n)
{
   if (r->nRefs + 1 > r->capRefs) {
      const int cap = r->capRefs * 2 + 64;
      char **nm = (char **)realloc(r->refName, sizeof(char *) * (size_t)cap);
      if (nm) r->refName = nm;
      int *off = (int *)realloc(r->refOff, sizeof(int) * ((size_t)cap + 1));
      if (off) r->refOff = off;
      if (!nm || !off) { htkamd_set_error("results: out of memory"); return HTKAMD_ENOMEM; }
      r->capRefs = cap;
   }
   const int need = r->refOff[r->nRefs] + n;
   if (need > r->capRefIds) {
      const int cap = need + need / 2 + 256;
      int *ids = (int *)realloc(r->refIds, sizeof(int) * (size_t)cap);
      if (!ids) { htkamd_set_error("results: out of memory"); return HTKAMD_ENOMEM; }
      r->refIds = ids; r->capRefIds = cap;
   }
   return HTKAMD_OK;
}

int htkamd_results_add_ref(htkamd_results *r, const char *utt, int n, const char *const *names)
{
   if (!r || !utt || n < 0 || (n > 0 && !names)) { htkamd_set_error("results_add_ref: bad argument"); return HTKAMD_EINVAL; }
   int k = htkamd_results_find_ref(r, utt);
   if (k >= 0) return k;
   if ((k = ref_room(r, n)) != HTKAMD_OK) return k;
   int *ids = r->refIds + r->refOff[r->nRefs];
   for (k = 0; k < n; k++) {
      if (!names[k]) { htkamd_set_error("results_add_ref: %s: label %d is NULL", utt, k); return HTKAMD_EINVAL; }
      if ((ids[k] = htkamd_results_label_id(r, names[k])) < 0) return ids[k];
   }
   if (!(r->refName[r->nRefs] = strdup(utt))) { htkamd_set_error("results: out of memory"); return HTKAMD_ENOMEM; }
   r->refOff[r->nRefs + 1] = r->refOff[r->nRefs] + n;
   return r->nRefs++;
}

int htkamd_results_ids(htkamd_results *r, const htkamd_labels *l, int *ids)
{
   if (!r || !l || (!ids && htkamd_labels_count(l) > 0)) { htkamd_set_error("results_ids: NULL argument"); return HTKAMD_EINVAL; }
   for (int k = 0; k < htkamd_labels_count(l); k++)
      if ((ids[k] = htkamd_results_label_id(r, htkamd_labels_name(l, k))) < 0) return ids[k];
   return HTKAMD_OK;
}

int htkamd_results_ref_for(htkamd_results *r, const char *recFile, const htkamd_mlf *const *mlfs, int nMlf, const char *labDir, const char *labExt,
                           char *labFile, size_t labFileLen)
{
   if (!r || !recFile || !labFile || nMlf < 0 || (nMlf > 0 && !mlfs)) { htkamd_set_error("results_ref_for: bad argument"); return HTKAMD_EINVAL; }
   /* MakeFN: the directory (labDir, else the file's own), the name without its last extension, the extension */
   const char *slash = strrchr(recFile, '/');
   const char *base = slash ? slash + 1 : recFile;
   const char *dot = strrchr(base, '.');
   const size_t nBase = dot ? (size_t)(dot - base) : strlen(base);
   const size_t nDir = labDir ? strlen(labDir) : (size_t)(base - recFile);
   const char *dir = labDir ? labDir : recFile;
   const char *ext = labExt ? labExt : "lab";
   const int sep = nDir > 0 && dir[nDir - 1] != '/';
   if (nDir + sep + nBase + 1 + strlen(ext) + 1 > labFileLen) { htkamd_set_error("results: the reference's file name of %s is too long", recFile); return HTKAMD_EINVAL; }
   char *o = labFile;
   memcpy(o, dir, nDir); o += nDir;
   if (sep) *o++ = '/';
   memcpy(o, base, nBase); o += nBase;
   *o = 0;
   if (*ext) { *o++ = '.'; strcpy(o, ext); }
   int k = htkamd_results_find_ref(r, labFile);
   if (k >= 0) return k;
   const htkamd_labels *l = NULL;
   htkamd_labels *own = NULL;
   for (k = 0; k < nMlf && !l; k++) l = htkamd_mlf_find(mlfs[k], labFile);
   if (!l && !strchr(labFile, '/') && strlen(labFile) + 3 <= labFileLen) {     /* a "*" "/name" pattern also answers to the bare name (HLabel.c: MLF_SIMPLE) */
      char *withDir = (char *)malloc(strlen(labFile) + 3);
      if (withDir) {
         sprintf(withDir, "./%s", labFile);
         for (k = 0; k < nMlf && !l; k++) l = htkamd_mlf_find(mlfs[k], withDir);
         free(withDir);
      }
   }
   if (!l) {
      if (htkamd_labels_read(labFile, &own) != HTKAMD_OK) {
         htkamd_set_error("results: no reference transcription for %s: %s cannot be opened%s", recFile, labFile, nMlf > 0 ? " and no master label file has it" : "");
         return HTKAMD_EIO;
      }
      l = own;
   }
   const int n = htkamd_labels_count(l);
   if ((k = ref_room(r, n)) == HTKAMD_OK) k = htkamd_results_ids(r, l, r->refIds + r->refOff[r->nRefs]);
   htkamd_labels_free(own);
   if (k != HTKAMD_OK) return k;
   if (!(r->refName[r->nRefs] = strdup(labFile))) { htkamd_set_error("results: out of memory"); return HTKAMD_ENOMEM; }
   r->refOff[r->nRefs + 1] = r->refOff[r->nRefs] + n;
   return r->nRefs++;
}

/* ---- text --------------------------------------------------------------------------------------------------------------------- */

static void bar(FILE *f, char c, const char *title)                      /* PrintBar(0, htkWidth, c, title) */
{
   int tlen = (int)strlen(title);
   if (tlen > 0) tlen += 2;
   const int k = (RES_WIDTH - tlen) / 2;
   for (int i = 1; i <= k; i++) fputc(c, f);
   if (tlen > 0) fprintf(f, " %s ", title);
   for (int i = k + tlen; i <= RES_WIDTH; i++) fputc(c, f);
   fputc('\n', f);
}

static void clip(const char *in, char *out, size_t max)                   /* PClip: the last `max` characters behind a '>' */
{
   if (!in) { out[0] = 0; return; }
   const size_t n = strlen(in);
   if (n <= max) { strcpy(out, in); return; }
   strcpy(out, in + n - max);
   out[0] = '>';
}

static void header(FILE *f, const htkamd_results_report *rep)
{
   char buf[100], date[64];
   time_t now = time(NULL);
   const char *ct = ctime(&now);
   snprintf(date, sizeof(date), "%s", ct ? ct : "");
   if (date[0]) date[strlen(date) - 1] = 0;
   bar(f, '=', "HTK Results Analysis");
   fprintf(f, "  Date: %s\n", date);
   clip(rep->refId, buf, 70); fprintf(f, "  Ref : %s\n", buf);
   clip(rep->nRecId > 0 ? rep->recId[0] : NULL, buf, 70); fprintf(f, "  Rec : %s\n", buf);
   for (int i = 1; i < rep->nRecId && i < 5; i++) { clip(rep->recId[i], buf, 70); fprintf(f, "      : %s\n", buf); }
}

/* one line of -t: `item` and blanks up to `width` */
static int put_item(char **line, size_t *len, size_t *cap, const char *item, size_t width)
{
   if (*len + width + 1 > *cap) {
      const size_t c = (*len + width + 1) * 2;
      char *p = (char *)realloc(*line, c);
      if (!p) return -1;
      *line = p; *cap = c;
   }
   const size_t n = strlen(item);
   memcpy(*line + *len, item, n);
   memset(*line + *len + n, ' ', width - n);
   *len += width; (*line)[*len] = 0;
   return 0;
}

static int aligned(FILE *f, const htkamd_results *r, const htkamd_results_report *rep, int k)
{
   size_t capA = 0, capB = 0, lenA = 0, lenB = 0;
   char *a = NULL, *b = NULL;
   int bad = put_item(&a, &lenA, &capA, " LAB: ", 6) || put_item(&b, &lenB, &capB, " REC: ", 6);
   for (int t = rep->alnOff[k]; t < rep->alnOff[k + 1] && !bad; t++) {
      const int *tr = rep->aln + 3 * (size_t)t;
      const char *rn = tr[1] >= 0 ? htkamd_results_label_name(r, tr[1]) : "", *tn = tr[2] >= 0 ? htkamd_results_label_name(r, tr[2]) : "";
      if (!rn || !tn) { free(a); free(b); htkamd_set_error("results_write: file %d: an alignment names label %d, which the table does not have", k, rn ? tr[2] : tr[1]); return HTKAMD_EINVAL; }
      const size_t la = strlen(rn), lb = strlen(tn), w = (la >= lb ? la : lb) + 1;
      bad = put_item(&a, &lenA, &capA, rn, w) || put_item(&b, &lenB, &capB, tn, w);
   }
   if (bad) { free(a); free(b); htkamd_set_error("results: out of memory"); return HTKAMD_ENOMEM; }
   fprintf(f, "Aligned transcription: %s vs %s\n", rep->labFile[k], rep->recFile[k]);
   fprintf(f, "%s\n%s\n", a, b);
   free(a); free(b);
   return HTKAMD_OK;
}

static void conmat(FILE *f, const htkamd_results *r, const int *conf, long nsyms)
{
   const int V = r->nList, W = V + 1;
   unsigned char *seen = (unsigned char *)calloc((size_t)V + 2, 1);
   int maxlen = 0, i, j, k;
   for (i = 1; i <= V; i++) { k = (int)strlen(r->name[i]); if (k > maxlen) maxlen = k; }
   if (maxlen > RES_MAXWORD) maxlen = RES_MAXWORD;
   bar(f, '-', "Confusion Matrix");
   for (j = 1; j <= V; j++) {                                    /* a column is shown when something was recognised as it */
      for (i = 1, k = conf[j]; i <= V; i++) k += conf[i * W + j];
      seen[j] = k != 0;
   }
   for (j = 0; j < maxlen; j++) {                                /* the column heads, a letter per line */
      fputs("     ", f);
      for (i = 1; i <= V; i++) {
         if (!seen[i]) continue;
         const char *s = r->name[i];
         fprintf(f, "  %c ", j < (int)strlen(s) ? s[j] : ' ');
      }
      if (j == maxlen - 1) fputs(" Del [ %c / %e]", f);
      fputc('\n', f);
   }
   for (i = 1; i <= V; i++) {
      char buf[8];
      for (j = 1, k = conf[i * W]; j <= V; j++) k += conf[i * W + j];
      if (k == 0) continue;
      snprintf(buf, 5, "%s", r->name[i]);
      fprintf(f, "%4s ", buf);
      int rowerr = 0;
      for (j = 1; j <= V; j++) {
         if (!seen[j]) continue;
         const int err = conf[i * W + j];
         if (i != j) rowerr += err;
         fprintf(f, err < 100 ? " %2d " : "%4d", err);
      }
      fprintf(f, "%4d", conf[i * W]);
      if (rowerr > 0) {
         const float correct = 100.0 * (float)conf[i * W + i] / (float)(conf[i * W + i] + rowerr);
         const float errprop = 100.0 * (float)rowerr / (float)nsyms;
         fprintf(f, " [%4.1f/%3.1f]\n", correct, errprop);
      } else
         fputc('\n', f);
   }
   fputs("Ins ", f);
   for (j = 1; j <= V; j++) if (seen[j]) fprintf(f, "%4d", conf[j]);
   fputc('\n', f);
   free(seen);
}

int htkamd_results_write(const htkamd_results *r, const htkamd_results_report *rep, const char *path, int append)
{
   if (!r || !rep || rep->nFiles < 0 || !rep->totals || (rep->nFiles > 0 && !rep->counts) || (rep->nRecId > 0 && !rep->recId)) {
      htkamd_set_error("results_write: bad argument"); return HTKAMD_EINVAL;
   }
   const int full = (rep->flags & HTKAMD_RES_FULL) != 0, trans = (rep->flags & HTKAMD_RES_TRANS) != 0, pstats = (rep->flags & HTKAMD_RES_PSTATS) != 0;
   if ((full || trans) && rep->nFiles > 0 && !rep->recFile) { htkamd_set_error("results_write: -f and -t need the files' names"); return HTKAMD_EINVAL; }
   if (trans && rep->nFiles > 0 && (!rep->alnOff || !rep->aln || !rep->labFile)) { htkamd_set_error("results_write: -t needs the alignments and the references' names"); return HTKAMD_EINVAL; }
   if (pstats && !rep->conf) { htkamd_set_error("results_write: -p needs the confusion matrix"); return HTKAMD_EINVAL; }
   if (pstats && r->nList > RES_MAXCONMAT) { htkamd_set_error("results: a confusion matrix of %d labels would be too large (at most %d)", r->nList, RES_MAXCONMAT); return HTKAMD_EINVAL; }
   FILE *f = path ? fopen(path, append ? "a" : "w") : stdout;
   if (!f) { htkamd_set_error("results_write: cannot open %s", path); return HTKAMD_EIO; }
   int printed = 0, rc = HTKAMD_OK;
   if (full) bar(f, '-', "Sentence Scores");
   for (int k = 0; k < rep->nFiles && rc == HTKAMD_OK; k++) {
      const int *c = rep->counts + 6 * (size_t)k;
      if (!c[5]) continue;                                       /* an empty transcription: HResults warns and goes on */
      const int h = c[0], d = c[1], s = c[2], i = c[3];
      if (full) {
         if (!printed) { header(f, rep); bar(f, '-', "File Results"); printed = 1; }
         const char *fn = strrchr(rep->recFile[k], '/');
         fn = fn ? fn + 1 : rep->recFile[k];
         const int nc = h + d + s;
         const float accuracy = 100.0 * ((float)(h - i) / (float)nc);
         const float correct = 100.0 * ((float)h / (float)nc);
         fprintf(f, "%s:  %6.2f(%6.2f)  [H=%4d, D=%3d, S=%3d, I=%3d, N=%3d]\n", fn, correct, accuracy, h, d, s, i, nc);
      }
      if (trans && (d || s || i)) rc = aligned(f, r, rep, k);
   }
   if (rc == HTKAMD_OK) {
      if (rep->nFiles == 0)
         fputs("No transcriptions found\n", f);
      else {
         const long hits = (long)rep->totals[0], del = (long)rep->totals[1], sub = (long)rep->totals[2], ins = (long)rep->totals[3], nsyms = (long)rep->totals[4];
         const long nphr = (long)rep->totals[5], phrcor = (long)rep->totals[6];
         if (!printed) header(f, rep);
         const float accuracy = 100.0 * (float)(hits - ins) / (float)nsyms;
         const float correct = 100.0 * (float)hits / (float)nsyms;
         const float phrcorrect = 100.0 * ((float)phrcor / (float)nphr);
         bar(f, '-', "Overall Results");
         fprintf(f, "SENT: %%Correct=%.2f [H=%ld, S=%ld, N=%ld]\n", phrcorrect, phrcor, nphr - phrcor, nphr);
         fprintf(f, "WORD: %%Corr=%.2f, Acc=%.2f", correct, accuracy);
         fprintf(f, " [H=%ld, D=%ld, S=%ld, I=%ld, N=%ld]\n", hits, del, sub, ins, nsyms);
         if (pstats) conmat(f, r, rep->conf, nsyms);
         bar(f, '=', "");
      }
   }
   if (path) fclose(f); else fflush(f);
   return rc;
}
