/* cepsnorm.c -- host-side (C) side-based cepstral mean and variance normalisation: the files, masks and tables of HParm's
 * CMEANDIR / CMEANMASK / CMEANPATHMASK and VARSCALEDIR / VARSCALEMASK / VARSCALEPATHMASK / VARSCALEFN, and of `HCompV -c -k -p -q`.
 *   mask matching        the behaviour of MaskMatch           HTKLib/HShell.c:1851 (own two-pass matcher, see below)
 *   <CEPSNORM> files     LoadCMeanVector / LoadVarScaleVector HTKLib/HParm.c:3172-3349 (read), ExportNMV HTKTools/HCompV.c:686-740 (write)
 *   <VARSCALE> file      LoadVarScale                         HTKLib/HParm.c:560-615
 *   kinds, lengths       HParm.c:3221-3224, :3298, :1797-1800
 *   scale table          AddQualifiers                        HParm.c:1806
 *   mean and variance    UpdateMeanVar                        HCompV.c:640-656 (here from fp64 sums: htkamd_side_stats)
 * Everything here is plain host code; every refusal is HTKAMD_EINVAL (HTKAMD_EIO for a file that cannot be opened) with the reason
 * in htkamd_last_error, and none of it looks for a device.  The kernels are in csrc/cepsnorm.hip.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../csrc/internal.h"

/* parameter kinds (HParm.h:40-75) */
#define HASENERGY 0100
#define HASNULLE  0200
#define HASDELTA  0400
#define HASACCS   01000
#define HASCOMPX  02000
#define HASZEROM  04000
#define HASCRCC   010000
#define HASZEROC  020000
#define HASVQ     040000
#define HASTHIRD  0100000
#define BASEMASK  077
static const char *const pmkmap[] = {"WAVEFORM", "LPC", "LPREFC", "LPCEPSTRA", "LPDELCEP", "IREFC", "MFCC", "FBANK", "MELSPEC", "USER", "DISCRETE", "PLP"};
#define NBASE ((int)(sizeof(pmkmap) / sizeof(pmkmap[0])))

/* Str2ParmKind (HParm.c:1109): the qualifiers are peeled off the end; -1 for a name it does not know */
int htkamd_parm_kind_parse(const char *str)
{
   char buf[256];
   int len, i, k = -1, q = 0;
   if (!str || strlen(str) >= sizeof(buf)) return -1;
   strcpy(buf, str); len = (int)strlen(buf);
   while (len > 2 && buf[len - 2] == '_') {
      switch (buf[len - 1]) {
      case 'E': q |= HASENERGY; break; case 'D': q |= HASDELTA; break; case 'N': q |= HASNULLE; break; case 'A': q |= HASACCS; break;
      case 'C': q |= HASCOMPX; break;  case 'T': q |= HASTHIRD; break; case 'K': q |= HASCRCC; break;  case 'Z': q |= HASZEROM; break;
      case '0': q |= HASZEROC; break;  case 'V': q |= HASVQ; break;
      default: return -1;
      }
      len -= 2; buf[len] = 0;
   }
   for (i = 0; i < NBASE; i++) if (!strcmp(buf, pmkmap[i])) k = i;
   if (k < 0) return -1;
   if (k == 4) k = 3 | HASDELTA;                         /* LPDELCEP (HParm.c:1146) */
   return k | q;
}

/* ParmKind2Str (HParm.c:1092): the order of the qualifiers is the reference's */
int htkamd_parm_kind_str(int kind, char *buf, int bufLen)
{
   char s[64];
   if (!buf || kind < 0 || (kind & BASEMASK) >= NBASE) { htkamd_set_error("parm_kind_str: bad argument"); return HTKAMD_EINVAL; }
   strcpy(s, pmkmap[kind & BASEMASK]);
   if (kind & HASENERGY) strcat(s, "_E");
   if (kind & HASDELTA) strcat(s, "_D");
   if (kind & HASNULLE) strcat(s, "_N");
   if (kind & HASACCS) strcat(s, "_A");
   if (kind & HASTHIRD) strcat(s, "_T");
   if (kind & HASCOMPX) strcat(s, "_C");
   if (kind & HASCRCC) strcat(s, "_K");
   if (kind & HASZEROM) strcat(s, "_Z");
   if (kind & HASZEROC) strcat(s, "_0");
   if (kind & HASVQ) strcat(s, "_V");
   if ((int)strlen(s) >= bufLen) { htkamd_set_error("parm_kind_str: buffer of %d bytes is too small", bufLen); return HTKAMD_EINVAL; }
   strcpy(buf, s);
   return HTKAMD_OK;
}

/* ---- masks ---- */
/* A file name against a mask (the behaviour of MaskMatch, HShell.c:1851): a literal matches itself, ? and % one character, * a run of any
   length; the characters under % are handed out in order.  Where a name matches in several ways the reference lets the leftmost * take
   the longest run that still leaves a match, then the next one, and so on.  Done here in two passes and in O(|mask| x |name|): `ok` marks
   every (mask position, name position) from which the rest of the mask matches the rest of the name, filled from the ends backwards;
   then one walk forwards, every * extended as far as `ok` allows, copies the characters under % out. */
int htkamd_mask_match(const char *mask, const char *name, char *out, int outLen)
{
   size_t nm, nn, i, j, captures = 0, w = 0;
   unsigned char *ok;
   if (!mask || !name || !out || outLen < 1) { htkamd_set_error("mask_match: NULL argument"); return HTKAMD_EINVAL; }
   nm = strlen(mask); nn = strlen(name);
   for (i = 0; i < nm; i++) if (mask[i] == '%') captures++;
   if (captures >= (size_t)outLen) {
      htkamd_set_error("mask_match: mask %s captures %d characters, the buffer holds %d", mask, (int)captures, outLen - 1); return HTKAMD_EINVAL;
   }
   out[0] = 0;
   ok = (unsigned char *)calloc((nm + 1) * (nn + 1), 1);
   if (!ok) { htkamd_set_error("mask_match: out of memory"); return HTKAMD_ENOMEM; }
#define OK(a, b) ok[(a) * (nn + 1) + (b)]
   OK(nm, nn) = 1;
   for (i = nm; i-- > 0;)
      for (j = nn + 1; j-- > 0;) {
         const char c = mask[i];
         if (c == '*') OK(i, j) = OK(i + 1, j) || (j < nn && OK(i, j + 1));
         else OK(i, j) = j < nn && (c == '?' || c == '%' || c == name[j]) && OK(i + 1, j + 1);
      }
   if (!OK(0, 0)) { free(ok); return 0; }
   for (i = 0, j = 0; i < nm; i++) {
      if (mask[i] == '*') {
         size_t end = nn;                                   /* the longest run behind which the rest still matches */
         while (!OK(i + 1, end)) end--;
         j = end;
      } else {
         if (mask[i] == '%') out[w++] = name[j];
         j++;
      }
   }
#undef OK
   out[w] = 0;
   free(ok);
   return 1;
}

/* ---- files ---- */
/* one whitespace-delimited token, as ReadString hands them to the loaders (no quoting in these files) */
static int next_token(FILE *f, char *buf, int n) { char fmt[16]; snprintf(fmt, sizeof(fmt), "%%%ds", n - 1); return fscanf(f, fmt, buf) == 1; }

/* `<TAG> n` has been read up to the tag: n, then n floats (ReadInt, ReadVector) */
static int read_vector(FILE *f, const char *path, const char *tag, float *v, int maxDim, int *dim)
{
   char tok[256], *end;
   int n, i;
   if (!next_token(f, tok, sizeof(tok)) || (n = (int)strtol(tok, &end, 10), *end) || n < 1) { htkamd_set_error("%s: no vector length behind %s", path, tag); return HTKAMD_EINVAL; }
   if (n > maxDim) { htkamd_set_error("%s: %s holds %d values, the caller takes %d", path, tag, n, maxDim); return HTKAMD_EINVAL; }
   for (i = 0; i < n; i++) {
      if (!next_token(f, tok, sizeof(tok)) || (v[i] = strtof(tok, &end), *end || end == tok)) { htkamd_set_error("%s: couldn't read the %d values of %s", path, n, tag); return HTKAMD_EINVAL; }
   }
   *dim = n;
   return HTKAMD_OK;
}

int htkamd_cepsnorm_read(const char *path, int *kind, int *nFrames, float *mean, int *dimMean, float *var, int *dimVar, int maxDim)
{
   FILE *f;
   char tok[256];
   int rc = HTKAMD_OK, dm = 0, dv = 0, nf = -1, pk;
   tok[0] = 0;
   if (!path || !kind || maxDim < 1 || (!mean && !var)) { htkamd_set_error("cepsnorm_read: bad argument"); return HTKAMD_EINVAL; }
   f = fopen(path, "r");
   if (!f) { htkamd_set_error("cepsnorm_read: can't open side file %s", path); return HTKAMD_EIO; }
   if (!next_token(f, tok, sizeof(tok)) || strcmp(tok, "<CEPSNORM>")) { fclose(f); htkamd_set_error("%s: <CEPSNORM> missing, read: %s", path, tok); return HTKAMD_EINVAL; }
   if (!next_token(f, tok, sizeof(tok)) || tok[0] != '<' || tok[strlen(tok) - 1] != '>') { fclose(f); htkamd_set_error("%s: <KIND> missing behind <CEPSNORM>", path); return HTKAMD_EINVAL; }
   tok[strlen(tok) - 1] = 0;
   pk = htkamd_parm_kind_parse(tok + 1);
   if (pk < 0) { fclose(f); htkamd_set_error("%s: unknown parameter kind %s", path, tok + 1); return HTKAMD_EINVAL; }
   while (rc == HTKAMD_OK && next_token(f, tok, sizeof(tok))) {
      if (!strcmp(tok, "<NFRAMES>")) {
         if (!next_token(f, tok, sizeof(tok))) { htkamd_set_error("%s: no count behind <NFRAMES>", path); rc = HTKAMD_EINVAL; }
         else nf = atoi(tok);
      }
      else if (!strcmp(tok, "<MEAN>") && mean) rc = read_vector(f, path, "<MEAN>", mean, maxDim, &dm);
      else if (!strcmp(tok, "<VARIANCE>") && var) rc = read_vector(f, path, "<VARIANCE>", var, maxDim, &dv);
   }
   fclose(f);
   if (rc) return rc;
   *kind = pk;
   if (nFrames) *nFrames = nf;
   if (dimMean) *dimMean = dm;
   if (dimVar) *dimVar = dv;
   return HTKAMD_OK;
}

int htkamd_cepsnorm_write(const char *path, int kind, const char *flags, int nFrames, const float *mean, const float *var, int dim)
{
   static const char *const ok[] = {"m", "v", "mv", "nv", "nmv"};                 /* ReportOutput HCompV.c:659-682 */
   char ks[64];
   FILE *f;
   int i, known = 0;
   if (!path || !flags || dim < 1) { htkamd_set_error("cepsnorm_write: bad argument"); return HTKAMD_EINVAL; }
   for (i = 0; i < 5; i++) if (!strcmp(flags, ok[i])) known = 1;
   if (!known) { htkamd_set_error("cepsnorm_write: unrecognisable output flag setting: %s (m v mv nv nmv)", flags); return HTKAMD_EINVAL; }
   if ((strchr(flags, 'm') && !mean) || (strchr(flags, 'v') && !var)) { htkamd_set_error("cepsnorm_write: flags %s without the vector", flags); return HTKAMD_EINVAL; }
   if (htkamd_parm_kind_str(kind, ks, sizeof(ks))) return HTKAMD_EINVAL;
   f = fopen(path, "w");
   if (!f) { htkamd_set_error("cepsnorm_write: output file creation error %s", path); return HTKAMD_EIO; }
   fprintf(f, "<CEPSNORM> <%s>", ks);
   if (strchr(flags, 'n')) fprintf(f, "\n<NFRAMES> %d", nFrames);
   if (strchr(flags, 'm')) { fprintf(f, "\n<MEAN> %d\n", dim); for (i = 0; i < dim; i++) fprintf(f, " %e", mean[i]); }
   if (strchr(flags, 'v')) { fprintf(f, "\n<VARIANCE> %d\n", dim); for (i = 0; i < dim; i++) fprintf(f, " %e", var[i]); }
   fprintf(f, "\n");
   if (fclose(f)) { htkamd_set_error("cepsnorm_write: cannot write %s", path); return HTKAMD_EIO; }
   return HTKAMD_OK;
}

int htkamd_varscale_read(const char *path, float *v, int *dim, int maxDim)
{
   FILE *f;
   char tok[256];
   int rc;
   tok[0] = 0;
   if (!path || !v || !dim || maxDim < 1) { htkamd_set_error("varscale_read: bad argument"); return HTKAMD_EINVAL; }
   f = fopen(path, "r");
   if (!f) { htkamd_set_error("varscale_read: can't open varscale file %s", path); return HTKAMD_EIO; }
   if (!next_token(f, tok, sizeof(tok)) || strcmp(tok, "<VARSCALE>")) { fclose(f); htkamd_set_error("%s: <VARSCALE> missing, read: %s", path, tok); return HTKAMD_EINVAL; }
   rc = read_vector(f, path, "<VARSCALE>", v, maxDim, dim);
   fclose(f);
   return rc;
}

/* ---- checks ---- */
int htkamd_cepsnorm_check_kinds(int targetKind, int meanKind, int varKind)
{
   char a[64], b[64];
   if (targetKind < 0) { htkamd_set_error("cepsnorm_check_kinds: bad target kind"); return HTKAMD_EINVAL; }
   if (meanKind >= 0) {                                  /* HParm.c:3221-3224 */
      const int tgtMask = ~(targetKind & (HASDELTA | HASACCS | HASTHIRD | HASZEROM | HASVQ));
      if ((meanKind & tgtMask) != (targetKind & tgtMask)) {
         if (htkamd_parm_kind_str(meanKind, a, sizeof(a)) || htkamd_parm_kind_str(targetKind, b, sizeof(b))) return HTKAMD_EINVAL;
         htkamd_set_error("side mean: ParmKind mismatch %s not a subset of %s", a, b); return HTKAMD_EINVAL;
      }
   }
   if (varKind >= 0 && targetKind != varKind && targetKind != (varKind | HASVQ)) {      /* HParm.c:3298 */
      if (htkamd_parm_kind_str(varKind, a, sizeof(a)) || htkamd_parm_kind_str(targetKind, b, sizeof(b))) return HTKAMD_EINVAL;
      htkamd_set_error("side variance: ParmKind mismatch %s != %s", a, b); return HTKAMD_EINVAL;
   }
   return HTKAMD_OK;
}

int htkamd_cepsnorm_scale(const float *varScale, int dScale, const float *sideVar, int dVar, int nSide, const char *const *sideNames, float *scale)
{
   int s, i;
   if (!varScale || !sideVar || !scale || nSide < 0 || dScale < 1 || dVar < 1) { htkamd_set_error("cepsnorm_scale: bad argument"); return HTKAMD_EINVAL; }
   if (dScale != dVar) { htkamd_set_error("cepsnorm_scale: mismatch between varScale (%d) and target size %d", dScale, dVar); return HTKAMD_EINVAL; }   /* HParm.c:1797-1800 */
   for (s = 0; s < nSide; s++)
      for (i = 0; i < dVar; i++) {
         const float sv = sideVar[(size_t)s * dVar + i];
         if (!(sv > 0.0f) || !(varScale[i] >= 0.0f)) {
            char num[16]; snprintf(num, sizeof(num), "%d", s);
            htkamd_set_error("cepsnorm_scale: side %s: variance %d is %g (global %g): not positive", (sideNames && sideNames[s]) ? sideNames[s] : num, i, sv, varScale[i]);
            return HTKAMD_EINVAL;
         }
         {  /* scale = sqrt(varScale / sideVar) with a float quotient, the double sqrt and a float result (HParm.c:1624, :1806) */
            const float quot = varScale[i] / sv;
            scale[(size_t)s * dVar + i] = (float)sqrt((double)quot);
         }
      }
   return HTKAMD_OK;
}

/* UpdateMeanVar (HCompV.c:640-656) from fp64 sums: mean = sum/N, var = sqsum/N - mean^2, each rounded once */
int htkamd_side_stats_finish(const double *sum, const double *sqsum, const long long *nFrames, int nSide, int D, float *mean, float *var)
{
   int s, i;
   if (!sum || !sqsum || !nFrames || nSide < 0 || D < 1 || (!mean && !var)) { htkamd_set_error("side_stats_finish: bad argument"); return HTKAMD_EINVAL; }
   for (s = 0; s < nSide; s++)
      for (i = 0; i < D; i++) {
         const size_t k = (size_t)s * D + i;
         double m = 0.0, v = 0.0;
         if (nFrames[s] > 0) { const double n = (double)nFrames[s]; m = sum[k] / n; v = sqsum[k] / n - m * m; }
         if (mean) mean[k] = (float)m;
         if (var) var[k] = (float)v;
      }
   return HTKAMD_OK;
}
