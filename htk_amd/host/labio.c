/* labio.c -- HTK label files and master label files (MLF), the transcription inputs of HERest -L/-I and HVite -a.
 *
 * Replaces LoadHTKLabels (HLabel.c:748-840: "[start [end]] name [score] {aux}" per line, times in 100 ns units,
 * a line of "///" separates alternatives -- only the first is kept, as HERest/HVite -a use it) and the immediate-definition
 * part of LoadMasterFile / the MLF search (HLabel.c:1410-1560: "#!MLF!#", then per entry a quoted pattern line and label
 * lines up to a single "."; patterns match with '*' and '?' like MaskMatch).  Sub-directory redirection ("->" / "=>")
 * is not supported.
 */
#include <ctype.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../csrc/internal.h"
#include "htktext.h"

struct htkamd_labels {
   int n;
   char **name;
   long long *start, *end;       /* -1 when absent */
   float *score;                 /* 0 when absent */
};

struct htkamd_mlf {
   int n;
   char **pattern;
   struct htkamd_labels **lab;
};

static int is_number(const char *t)
{
   char *e;
   if (!*t) return 0;
   strtod(t, &e);
   return *e == 0;
}

/* One label line, split as LoadHTKList (HLabel.c:748) splits it: [start [end]] name [score] {aux}, every token a ReadString string; a token
   that stood in quotes is never a number.  Appended to L; returns 0, 1 for the alternative separator, or an error code. */
static int add_line(struct htkamd_labels *L, int *cap, htx_src *s, const char *path)
{
   char tok[8][1024]; int quoted[8], nt = 0, r;
   while (nt < 8 && (r = htx_read_string(s, HTX_LINE, NULL, tok[nt], sizeof(tok[nt]))) == HTX_GOT) quoted[nt++] = s->wasQuoted;
   if (nt < 8 && r < 0) { htkamd_set_error("%s: label %d: %s", path, L->n + 1, htx_result_text(r)); return HTKAMD_EMODEL; }
   htx_skip_line(s);
   if (nt == 0) return 0;
   if (!quoted[0] && !strcmp(tok[0], "///")) return 1;
#define IS_NUM(k) (!quoted[k] && is_number(tok[k]))
   long long st = -1, en = -1; float sc = 0.0f; int k = 0;
   if (nt >= 2 && IS_NUM(0) && (isdigit((unsigned char)tok[0][0]) || tok[0][0] == '-')) {
      st = atoll(tok[k++]);
      if (nt >= 3 && IS_NUM(1)) en = atoll(tok[k++]);
   }
   const char *name = tok[k++];
   if (k < nt && IS_NUM(k)) sc = strtof(tok[k], NULL);
#undef IS_NUM
   if (L->n + 1 > *cap) {
      *cap = *cap * 2 + 32;
      L->name = (char **)realloc(L->name, sizeof(char *) * (size_t)*cap);
      L->start = (long long *)realloc(L->start, sizeof(long long) * (size_t)*cap);
      L->end = (long long *)realloc(L->end, sizeof(long long) * (size_t)*cap);
      L->score = (float *)realloc(L->score, sizeof(float) * (size_t)*cap);
   }
   L->name[L->n] = strdup(name); L->start[L->n] = st; L->end[L->n] = en; L->score[L->n] = sc; L->n++;
   return 0;
}

/* the label lines up to the end of the text or, inside an MLF, up to a line that holds a single "."; only the first alternative is kept */
static int read_list(struct htkamd_labels *L, htx_src *s, int mlf, const char *path)
{
   int cap = 0, alt = 0;
   while (s->p < s->end) {
      const char *q = s->p;
      while (q < s->end && isspace((unsigned char)*q) && *q != '\n') q++;
      if (mlf && q < s->end && *q == '.' && (q + 1 == s->end || isspace((unsigned char)q[1]))) { htx_skip_line(s); break; }
      if (alt) { htx_skip_line(s); continue; }
      const int r = add_line(L, &cap, s, path);
      if (r < 0) return r;
      alt = r;
   }
   return HTKAMD_OK;
}

static char *read_text(const char *path, const char *who, size_t *len, int *rc)
{
   int why;
   char *txt = htx_read_file(path, len, &why);
   if (!txt && why == HTX_ENOMEM) { htkamd_set_error("%s: out of memory reading %s", who, path); *rc = HTKAMD_ENOMEM; }
   else if (!txt) { htkamd_set_error("%s: cannot open %s", who, path); *rc = HTKAMD_EIO; }
   return txt;
}

void htkamd_labels_free(struct htkamd_labels *L)
{
   if (!L) return;
   for (int i = 0; i < L->n; i++) free(L->name[i]);
   free(L->name); free(L->start); free(L->end); free(L->score); free(L);
}

int htkamd_labels_read(const char *path, struct htkamd_labels **out)
{
   if (!path || !out) { htkamd_set_error("labels_read: NULL argument"); return HTKAMD_EINVAL; }
   size_t len; int rc;
   char *txt = read_text(path, "labels_read", &len, &rc);
   if (!txt) return rc;
   struct htkamd_labels *L = (struct htkamd_labels *)calloc(1, sizeof(*L));
   htx_src s = {txt, txt + len, 0};
   rc = read_list(L, &s, 0, path);
   free(txt);
   if (rc) { htkamd_labels_free(L); return rc; }
   *out = L;
   return HTKAMD_OK;
}

int htkamd_labels_count(const struct htkamd_labels *L) { return L ? L->n : 0; }
const char *htkamd_labels_name(const struct htkamd_labels *L, int i) { return (L && i >= 0 && i < L->n) ? L->name[i] : NULL; }
long long htkamd_labels_start(const struct htkamd_labels *L, int i) { return (L && i >= 0 && i < L->n) ? L->start[i] : -1; }
long long htkamd_labels_end(const struct htkamd_labels *L, int i) { return (L && i >= 0 && i < L->n) ? L->end[i] : -1; }
float htkamd_labels_score(const struct htkamd_labels *L, int i) { return (L && i >= 0 && i < L->n) ? L->score[i] : 0.0f; }

/* MaskMatch-style wildcard match ('*' any run, '?' one character) */
static int wild(const char *p, const char *s)
{
   if (*p == 0) return *s == 0;
   if (*p == '*') { for (;; s++) { if (wild(p + 1, s)) return 1; if (*s == 0) return 0; } }
   if (*s == 0) return 0;
   if (*p == '?' || *p == *s) return wild(p + 1, s + 1);
   return 0;
}

void htkamd_mlf_free(struct htkamd_mlf *m)
{
   if (!m) return;
   for (int i = 0; i < m->n; i++) { free(m->pattern[i]); htkamd_labels_free(m->lab[i]); }
   free(m->pattern); free(m->lab); free(m);
}

int htkamd_mlf_read(const char *path, struct htkamd_mlf **out)
{
   if (!path || !out) { htkamd_set_error("mlf_read: NULL argument"); return HTKAMD_EINVAL; }
   size_t len; int rc;
   char *txt = read_text(path, "mlf_read", &len, &rc);
   if (!txt) return rc;
   if (strncmp(txt, "#!MLF!#", 7)) { free(txt); htkamd_set_error("mlf_read: %s has no #!MLF!# header", path); return HTKAMD_EMODEL; }
   htx_src s = {txt, txt + len, 0};
   htx_skip_line(&s);
   struct htkamd_mlf *m = (struct htkamd_mlf *)calloc(1, sizeof(*m));
   int capM = 0;
   char pattern[1024];
   rc = HTKAMD_OK;
   while (!rc) {
      while (s.p < s.end && isspace((unsigned char)*s.p)) s.p++;
      if (s.p >= s.end) break;
      const char *eol = (const char *)memchr(s.p, '\n', (size_t)(s.end - s.p));
      if (!eol) eol = s.end;
      for (const char *q = s.p; q + 1 < eol && !rc; q++)
         if ((q[0] == '-' || q[0] == '=') && q[1] == '>') { htkamd_set_error("mlf_read: %s: sub-directory entries are not supported", path); rc = HTKAMD_EMODEL; }
      if (rc) break;
      const int r = htx_read_string(&s, HTX_LINE, NULL, pattern, sizeof(pattern));      /* a ReadString string (HLabel.c:1203) */
      if (r != HTX_GOT) { htkamd_set_error("mlf_read: %s: pattern %d: %s", path, m->n + 1, htx_result_text(r)); rc = HTKAMD_EMODEL; break; }
      htx_skip_line(&s);
      if (m->n + 1 > capM) { capM = capM * 2 + 32; m->pattern = (char **)realloc(m->pattern, sizeof(char *) * (size_t)capM); m->lab = (struct htkamd_labels **)realloc(m->lab, sizeof(void *) * (size_t)capM); }
      struct htkamd_labels *L = (struct htkamd_labels *)calloc(1, sizeof(*L));
      m->pattern[m->n] = strdup(pattern); m->lab[m->n] = L; m->n++;
      rc = read_list(L, &s, 1, path);                /* a last entry may end at EOF without '.' */
   }
   free(txt);
   if (rc) { htkamd_mlf_free(m); return rc; }
   *out = m;
   return HTKAMD_OK;
}

/* Labels of `labFile` (e.g. "lab/u00001.lab"; callers derive it from the data file name as HERest does: base name + ".lab"):
   first entry whose pattern matches; NULL if none. */
const struct htkamd_labels *htkamd_mlf_find(const struct htkamd_mlf *m, const char *labFile)
{
   if (!m || !labFile) return NULL;
   for (int i = 0; i < m->n; i++) if (wild(m->pattern[i], labFile)) return m->lab[i];
   return NULL;
}

/* the entries in file order (HResults scores a hypothesis MLF entry by entry: main HResults.c:294) */
int htkamd_mlf_count(const struct htkamd_mlf *m) { return m ? m->n : 0; }
const char *htkamd_mlf_pattern(const struct htkamd_mlf *m, int i) { return (m && i >= 0 && i < m->n) ? m->pattern[i] : NULL; }
const struct htkamd_labels *htkamd_mlf_entry(const struct htkamd_mlf *m, int i) { return (m && i >= 0 && i < m->n) ? m->lab[i] : NULL; }

/* ---- script files (-S): the list of data files of a tool run ------------------------------------------------------------
 * ScriptWord (HShell.c:661-688): words separated by white space, or enclosed in single / double quotes (no escapes);
 * RegisterExtFileName (HShell.c:86-140): a word may be an extended file name  logical=physical[start,end]  (either part optional):
 * the data are read from `physical`, frames start..end inclusive, and the file is known (label lookup) as `logical`. */
struct htkamd_scp {
   int n;
   char **logical, **physical;
   long *start, *end;            /* -1 = whole file */
};

void htkamd_scp_free(struct htkamd_scp *s)
{
   if (!s) return;
   for (int i = 0; i < s->n; i++) { free(s->logical[i]); free(s->physical[i]); }
   free(s->logical); free(s->physical); free(s->start); free(s->end); free(s);
}

int htkamd_scp_read(const char *path, struct htkamd_scp **out)
{
   if (!path || !out) { htkamd_set_error("scp_read: NULL argument"); return HTKAMD_EINVAL; }
   FILE *f = fopen(path, "r");
   if (!f) { htkamd_set_error("scp_read: cannot open script file %s", path); return HTKAMD_EIO; }
   struct htkamd_scp *s = (struct htkamd_scp *)calloc(1, sizeof(*s));
   int cap = 0, ch;
   char buf[4096];
   for (;;) {
      int i = 0;
      do ch = fgetc(f); while (ch != EOF && isspace(ch));
      if (ch == EOF) break;
      if (ch == '\'' || ch == '"') {
         const int q = ch;
         while ((ch = fgetc(f)) != q && ch != EOF) if (i < (int)sizeof(buf) - 1) buf[i++] = (char)ch;
         if (ch == EOF) { fclose(f); htkamd_scp_free(s); htkamd_set_error("scp_read: %s: closing quote missing", path); return HTKAMD_EINVAL; }
      } else {
         do { if (i < (int)sizeof(buf) - 1) buf[i++] = (char)ch; ch = fgetc(f); } while (ch != EOF && !isspace(ch));
      }
      buf[i] = 0;
      if (s->n + 1 > cap) {
         cap = cap * 2 + 64;
         s->logical = (char **)realloc(s->logical, sizeof(char *) * (size_t)cap); s->physical = (char **)realloc(s->physical, sizeof(char *) * (size_t)cap);
         s->start = (long *)realloc(s->start, sizeof(long) * (size_t)cap); s->end = (long *)realloc(s->end, sizeof(long) * (size_t)cap);
      }
      long st = -1, en = -1;
      char *eq = strchr(buf, '='), *lb = strchr(buf, '[');
      if (lb) {
         char *co = strchr(buf, ','), *rb = strchr(buf, ']');
         if (!co || !rb) { fclose(f); htkamd_scp_free(s); htkamd_set_error("scp_read: %s: bad index spec in %s", path, buf); return HTKAMD_EINVAL; }
         *rb = 0; en = atol(co + 1);
         *co = 0; st = atol(lb + 1);
         *lb = 0;
      }
      if (eq) { *eq = 0; s->physical[s->n] = strdup(eq + 1); s->logical[s->n] = strdup(buf); }
      else { s->physical[s->n] = strdup(buf); s->logical[s->n] = strdup(buf); }
      s->start[s->n] = st; s->end[s->n] = en; s->n++;
   }
   fclose(f);
   *out = s;
   return HTKAMD_OK;
}

int htkamd_scp_count(const struct htkamd_scp *s) { return s ? s->n : 0; }
const char *htkamd_scp_logical(const struct htkamd_scp *s, int i) { return (s && i >= 0 && i < s->n) ? s->logical[i] : NULL; }
const char *htkamd_scp_physical(const struct htkamd_scp *s, int i) { return (s && i >= 0 && i < s->n) ? s->physical[i] : NULL; }
long htkamd_scp_start(const struct htkamd_scp *s, int i) { return (s && i >= 0 && i < s->n) ? s->start[i] : -1; }
long htkamd_scp_end(const struct htkamd_scp *s, int i) { return (s && i >= 0 && i < s->n) ? s->end[i] : -1; }

/* ---- label output: a transcription being built, FormatTranscription and SaveHTKLabels ---------------------------------------
 * One label list (one level) with up to two auxiliary labels per entry, as TranscriptionFromLattice builds it for HVite
 * (HRec.c:2176-2360: word level = no auxiliary labels; -m = [word]; -f -m = [model, word]); htkamd_trans_format applies HVite's
 * -o flags the way FormatTranscription does (HRec.c:2368-2472); htkamd_trans_write prints like SaveHTKLabels (HLabel.c:1481-1525:
 * times "%.0f" in 100 ns units when present, a score column only if ANY label of the list has a non-zero score in it). */
#include <math.h>

typedef struct { double start, end; char *name; float score; char *aux[2]; float auxScore[2]; } trans_lab;
struct htkamd_trans { int n, cap, maxAux; trans_lab *lab; struct htkamd_trans *next; };     /* next: the next alternative (label list) */

int htkamd_trans_create(int maxAux, struct htkamd_trans **out)
{
   if (!out || maxAux < 0 || maxAux > 2) { htkamd_set_error("trans_create: bad argument"); return HTKAMD_EINVAL; }
   struct htkamd_trans *t = (struct htkamd_trans *)calloc(1, sizeof(*t));
   t->maxAux = maxAux;
   *out = t;
   return HTKAMD_OK;
}

void htkamd_trans_free(struct htkamd_trans *t)
{
   while (t) {
      struct htkamd_trans *nx = t->next;
      for (int i = 0; i < t->n; i++) { free(t->lab[i].name); free(t->lab[i].aux[0]); free(t->lab[i].aux[1]); }
      free(t->lab); free(t);
      t = nx;
   }
}

/* N-best output: `alt` becomes the last alternative of `t` (a Transcription with several label lists, AddLabelList HLabel.c;
   written one after the other with a line of "///" between them, SaveHTKLabels :1522).  `t` owns it from here on. */
int htkamd_trans_append_alternative(struct htkamd_trans *t, struct htkamd_trans *alt)
{
   if (!t || !alt || t == alt) { htkamd_set_error("trans_append_alternative: bad argument"); return HTKAMD_EINVAL; }
   while (t->next) t = t->next;
   t->next = alt;
   return HTKAMD_OK;
}

/* start / end in 100 ns units (-1 = absent); aux1 / aux2 may be NULL */
int htkamd_trans_add(struct htkamd_trans *t, double start, double end, const char *name, float score,
                     const char *aux1, float aux1Score, const char *aux2, float aux2Score)
{
   if (!t || !name) { htkamd_set_error("trans_add: NULL argument"); return HTKAMD_EINVAL; }
   if (t->n + 1 > t->cap) { t->cap = t->cap * 2 + 32; t->lab = (trans_lab *)realloc(t->lab, sizeof(trans_lab) * (size_t)t->cap); }
   trans_lab *l = &t->lab[t->n++];
   l->start = start; l->end = end; l->name = strdup(name); l->score = score;
   l->aux[0] = (aux1 && t->maxAux >= 1) ? strdup(aux1) : NULL; l->auxScore[0] = aux1Score;
   l->aux[1] = (aux2 && t->maxAux >= 2) ? strdup(aux2) : NULL; l->auxScore[1] = aux2Score;
   return HTKAMD_OK;
}

static void tri_strip_inplace(char *s)                       /* TriStrip (HLabel/HUtil): a-b+c -> b */
{
   char *p = strchr(s, '-');
   if (p) memmove(s, p + 1, strlen(p + 1) + 1);
   if ((p = strrchr(s, '+')) != NULL) *p = 0;
}

/* flags: the letters of HVite -o / HTKAMD_OUT_* bits.  frameDur in 100 ns units; states / models = the -f / -m switches. */
int htkamd_trans_format(struct htkamd_trans *t, double frameDur, int states, int models, int flags)
{
   if (!t || frameDur <= 0) { htkamd_set_error("trans_format: bad argument"); return HTKAMD_EINVAL; }
   if (t->next) { const int rc = htkamd_trans_format(t->next, frameDur, states, models, flags); if (rc) return rc; }
   if (flags & HTKAMD_OUT_NOSCORES)
      for (int i = 0; i < t->n; i++) { t->lab[i].score = 0.0f; t->lab[i].auxScore[0] = t->lab[i].auxScore[1] = 0.0f; }
   if (flags & HTKAMD_OUT_TRISTRIP)
      for (int i = 0; i < t->n; i++) {
         trans_lab *l = &t->lab[i];
         if (states && !models) {                             /* "model[state]" names: keep the tail */
            char tail[64] = "", *p = strrchr(l->name, '[');
            if (p) { snprintf(tail, sizeof(tail), "%s", p); *p = 0; }
            tri_strip_inplace(l->name);
            char *nn = (char *)malloc(strlen(l->name) + strlen(tail) + 1);
            strcpy(nn, l->name); strcat(nn, tail); free(l->name); l->name = nn;
         } else if (!states && models) tri_strip_inplace(l->name);
         else if (states && models && l->aux[0]) tri_strip_inplace(l->aux[0]);
      }
   if (flags & HTKAMD_OUT_NORMSCORES)
      for (int i = 0; i < t->n; i++) {
         trans_lab *l = &t->lab[i];
         int frames = (int)floor((l->end - l->start) / frameDur + 0.4);
         l->score = frames == 0 ? 0.0f : l->score / frames;
         if (states && models && t->maxAux > 0 && l->aux[0]) {          /* the model spans the labels up to the next model label */
            double end = l->end;
            for (int k = i + 1; k < t->n && !t->lab[k].aux[0]; k++) end = t->lab[k].end;
            frames = (int)floor((end - l->start) / frameDur + 0.4);
            l->auxScore[0] = frames == 0 ? 0.0f : l->auxScore[0] / frames;
         }
      }
   if (flags & HTKAMD_OUT_NOTIMES)
      for (int i = 0; i < t->n; i++) t->lab[i].start = t->lab[i].end = -1.0;
   if (flags & HTKAMD_OUT_CENTRE)
      for (int i = 0; i < t->n; i++) { t->lab[i].start += frameDur / 2; t->lab[i].end -= frameDur / 2; }
   if ((flags & HTKAMD_OUT_NOWORDS) && t->maxAux > 0)
      for (int i = 0; i < t->n; i++) { free(t->lab[i].aux[t->maxAux - 1]); t->lab[i].aux[t->maxAux - 1] = NULL; }
   if ((flags & HTKAMD_OUT_NOMODELS) && models && states && t->maxAux == 2)
      for (int i = 0; i < t->n; i++) {
         trans_lab *l = &t->lab[i];
         free(l->aux[0]); l->aux[0] = l->aux[1]; l->auxScore[0] = l->auxScore[1]; l->aux[1] = NULL;
      }
   return HTKAMD_OK;
}

static void write_name(FILE *f, const char *s) { htx_write_string(f, s, 0, 0); }      /* WriteString with q = 0 (HShell.c:1268) */

static void trans_print_one(FILE *f, const struct htkamd_trans *t);
static void trans_print(FILE *f, const struct htkamd_trans *t)
{
   for (; t; t = t->next) { trans_print_one(f, t); if (t->next) fprintf(f, "///\n"); }
}
static void trans_print_one(FILE *f, const struct htkamd_trans *t)
{
   int has[3] = {0, 0, 0};
   for (int i = 0; i < t->n; i++) {
      if (t->lab[i].score != 0.0f) has[0] = 1;
      for (int j = 0; j < t->maxAux; j++) if (t->lab[i].auxScore[j] != 0.0f) has[j + 1] = 1;
   }
   for (int i = 0; i < t->n; i++) {
      const trans_lab *l = &t->lab[i];
      if (l->start >= 0.0) {
         fprintf(f, "%.0f ", l->start);
         if (l->end >= 0.0) fprintf(f, "%.0f ", l->end);
      }
      write_name(f, l->name);
      if (has[0]) fprintf(f, " %f", l->score);
      for (int j = 0; j < t->maxAux; j++)
         if (l->aux[j]) { fputc(' ', f); write_name(f, l->aux[j]); if (has[j + 1]) fprintf(f, " %f", l->auxScore[j]); }
      fprintf(f, "\n");
   }
}

int htkamd_trans_write(const struct htkamd_trans *t, const char *path)
{
   if (!t || !path) { htkamd_set_error("trans_write: NULL argument"); return HTKAMD_EINVAL; }
   FILE *f = fopen(path, "w");
   if (!f) { htkamd_set_error("trans_write: cannot create %s", path); return HTKAMD_EIO; }
   trans_print(f, t);
   fclose(f);
   return HTKAMD_OK;
}

/* master label file output (HVite -i): "#!MLF!#", then per transcription its quoted name, the labels and "." */
struct htkamd_mlf_out { FILE *f; };
int htkamd_mlf_out_open(const char *path, struct htkamd_mlf_out **out)
{
   if (!path || !out) { htkamd_set_error("mlf_out_open: NULL argument"); return HTKAMD_EINVAL; }
   FILE *f = fopen(path, "w");
   if (!f) { htkamd_set_error("mlf_out_open: cannot create %s", path); return HTKAMD_EIO; }
   fprintf(f, "#!MLF!#\n");
   struct htkamd_mlf_out *o = (struct htkamd_mlf_out *)calloc(1, sizeof(*o));
   o->f = f; *out = o;
   return HTKAMD_OK;
}
int htkamd_mlf_out_add(struct htkamd_mlf_out *o, const char *labFile, const struct htkamd_trans *t)
{
   if (!o || !labFile || !t) { htkamd_set_error("mlf_out_add: NULL argument"); return HTKAMD_EINVAL; }
   fprintf(o->f, "\"%s\"\n", labFile);
   trans_print(o->f, t);
   fprintf(o->f, ".\n");
   return HTKAMD_OK;
}
void htkamd_mlf_out_close(struct htkamd_mlf_out *o) { if (o) { fclose(o->f); free(o); } }
