/* cli_common.h -- what the command-line drivers (tools/herest.c, tools/hvite.c) share: HTK-style option scanning, the configuration
 * file, parameter kinds, file-name composition, and loading a batch of parameter files into one device table of observations.
 * Host code over include/htk_amd.h only (the drivers are the programs a user of the reference's HERest / HVite switches to;
 * flags follow HTKBook ref.tex "HERest" / "HVite" for the subset SURVEY.md 8(b) lists).
 */
#ifndef HTKAMD_CLI_COMMON_H
#define HTKAMD_CLI_COMMON_H

#include <ctype.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include "htk_amd.h"

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "ERROR [%d] %s: %s\n", rc_, #call, htkamd_last_error()); exit(1); } } while (0)
#define DIE(...) do { fprintf(stderr, "ERROR "); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } while (0)

/* ---- string list ---- */
typedef struct { char **v; int n, cap; } strlist;
static void sl_add(strlist *l, const char *s)
{
   if (l->n + 1 > l->cap) { l->cap = l->cap * 2 + 64; l->v = (char **)realloc(l->v, sizeof(char *) * (size_t)l->cap); }
   l->v[l->n++] = strdup(s);
}

/* ---- configuration file: NAME = value lines, optional MODULE: prefix, # comments (ReadConfigFile HShell.c:392) ---- */
typedef struct { strlist key, val, mod; } config;
static void cfg_read(config *c, const char *path)
{
   FILE *f = fopen(path, "r");
   char line[2048];
   if (!f) DIE("cannot open configuration file %s", path);
   while (fgets(line, sizeof(line), f)) {
      char *p = line, *eq, *k, *v, *e;
      char *hash = strchr(p, '#'); if (hash) *hash = 0;
      eq = strchr(p, '=');
      if (!eq) continue;
      *eq = 0;
      k = p; while (isspace((unsigned char)*k)) k++;
      e = k + strlen(k); while (e > k && isspace((unsigned char)e[-1])) *--e = 0;
      char *modname = (char *)"";
      { char *colon = strrchr(k, ':'); if (colon) { *colon = 0; modname = k; k = colon + 1; while (isspace((unsigned char)*k)) k++; } }   /* HPARM: TARGETKIND -> TARGETKIND */
      for (char *q = modname; *q; q++) *q = (char)toupper((unsigned char)*q);
      { char *e2 = modname + strlen(modname); while (e2 > modname && isspace((unsigned char)e2[-1])) *--e2 = 0; }
      v = eq + 1; while (isspace((unsigned char)*v)) v++;
      e = v + strlen(v); while (e > v && isspace((unsigned char)e[-1])) *--e = 0;
      for (char *q = k; *q; q++) *q = (char)toupper((unsigned char)*q);
      sl_add(&c->key, k); sl_add(&c->val, v); sl_add(&c->mod, modname);
   }
   fclose(f);
}
static const char *cfg_get(const config *c, const char *key)
{
   for (int i = c->key.n - 1; i >= 0; i--) if (!strcmp(c->key.v[i], key)) return c->val.v[i];
   return NULL;
}
/* a module's own parameter: `MODULE: NAME = v` or an unqualified `NAME = v` (GetConfig(name, incGlob = TRUE) HShell.c:601) */
__attribute__((unused)) static const char *cfg_get_mod(const config *c, const char *module, const char *key)
{
   for (int i = c->key.n - 1; i >= 0; i--)
      if (!strcmp(c->key.v[i], key) && (c->mod.v[i][0] == 0 || !strcmp(c->mod.v[i], module))) return c->val.v[i];
   return NULL;
}
static int cfg_int(const config *c, const char *key, int dflt) { const char *v = cfg_get(c, key); return v ? atoi(v) : dflt; }
static int cfg_bool(const config *c, const char *key, int dflt) { const char *v = cfg_get(c, key); return v ? (v[0] == 'T' || v[0] == 't') : dflt; }

/* ---- parameter kinds (HParm.h:40-75): base code in the low 6 bits, qualifier bits above ---- */
#define PK_HASENERGY 0100
#define PK_HASNULLE  0200
#define PK_HASDELTA  0400
#define PK_HASACCS   01000
#define PK_HASZEROM  04000
#define PK_HASZEROC  020000
#define PK_HASTHIRD  0100000
static const char *const pk_base[] = {"WAVEFORM", "LPC", "LPREFC", "LPCEPSTRA", "LPDELCEP", "IREFC", "MFCC", "FBANK", "MELSPEC", "USER", "DISCRETE", "PLP", NULL};
/* the library's parser (htkamd_parm_kind_parse = Str2ParmKind), in any letter case; the storage qualifiers _C _K have no effect on the observation */
static int kind_parse(const char *s)
{
   char buf[128];
   snprintf(buf, sizeof(buf), "%s", s);
   for (char *q = buf; *q; q++) *q = (char)toupper((unsigned char)*q);
   const int k = htkamd_parm_kind_parse(buf);
   if (k < 0) DIE("unknown parameter kind %s", s);
   if (k & 040000) DIE("parameter kind %s: _V (vector quantisation) is not supported", s);
   return k & ~(02000 | 010000);
}

/* ---- file names: MakeFN (HShell.c:1258): directory and extension of `fn` replaced ---- */
static void make_fn(const char *fn, const char *dir, const char *ext, char *out, size_t n)
{
   const char *base = strrchr(fn, '/'); base = base ? base + 1 : fn;
   char stem[1024];
   snprintf(stem, sizeof(stem), "%s", base);
   if (ext) { char *dot = strrchr(stem, '.'); if (dot) *dot = 0; }
   if (dir) snprintf(out, n, "%s/%s%s%s", dir, stem, ext ? "." : "", ext ? ext : "");
   else if (ext) { char d2[1024]; snprintf(d2, sizeof(d2), "%.*s", (int)(base - fn), fn); snprintf(out, n, "%s%s.%s", d2, stem, ext); }
   else snprintf(out, n, "%s", fn);
}

/* ---- a batch of parameter files -> one device table of observations of the TARGET kind ----
 * The files hold `fileKind` (all the same); the qualifiers the target kind has beyond it (_D _A _T _Z _N) are computed on the device
 * (htkamd_parm_qualify = AddQualifiers HParm.c:1618), as OpenBuffer does when TARGETKIND asks for more than the file has; side means
 * and variances (CMEANDIR ..., VARSCALEDIR ...) are applied behind them (normalise_sides). */
typedef struct {
   int nUtt, cols, period, *frameOff;
   float *dX;                  /* device [frameOff[nUtt] * cols] */
} obs_batch;

static double cfg_flt(const config *c, const char *key, double dflt) { const char *v = cfg_get(c, key); return v ? atof(v) : dflt; }

static int waveform_source(const config *cfg)
{
   const char *sfmt = cfg_get(cfg, "SOURCEFORMAT"), *skind = cfg_get(cfg, "SOURCEKIND");
   return (sfmt && !strcasecmp(sfmt, "WAV")) || (skind && !strcasecmp(skind, "WAVEFORM"));
}

/* the base kinds a waveform is coded as on the device; the drivers call this before they touch a device */
static void check_waveform_kind(int targetKind)
{
   const int base = targetKind < 0 ? -1 : (targetKind & 077);
   if (base >= 1 && base <= 3)
      DIE("waveform sources: TARGETKIND %s is a time-domain LPC kind, which is not coded on the device (MFCC, FBANK, MELSPEC or PLP)", pk_base[base]);
   if (base != 6 && base != 7 && base != 8 && base != 11)
      DIE("waveform sources are coded as MFCC, FBANK, MELSPEC or PLP: TARGETKIND = <kind>[_0][_E][_D][_A][_T][_Z][_N] expected");
}

/* WARPFREQ / WARPLCUTOFF / WARPUCUTOFF of a waveform source */
static htkamd_warp waveform_warp(const config *cfg)
{
   htkamd_warp w;
   w.warpFreq = (float)cfg_flt(cfg, "WARPFREQ", 1.0); w.warpLCutoff = (float)cfg_flt(cfg, "WARPLCUTOFF", 0.0); w.warpUCutoff = (float)cfg_flt(cfg, "WARPUCUTOFF", 0.0);
   return w;
}
/* what the library refuses of them whatever the files' rate (htkamd_warp_check: ValidCodeParms HParm.c:1366-1372); the drivers call this
   before they touch a device.  What depends on the band the library refuses when the front end is made (code_waveforms) */
static void check_waveform_warp(const config *cfg)
{
   const htkamd_warp w = waveform_warp(cfg);
   if (htkamd_warp_check(&w)) DIE("waveform sources: %s", htkamd_last_error());
}

/* Waveform sources (SOURCEFORMAT = WAV, or SOURCEKIND = WAVEFORM with HTK waveform files): the files of the batch are coded on the
   device as OpenBuffer does for a waveform file (htkamd_frontend_compute: statics + _0 / _E of TARGETKIND's base kind -- MFCC, FBANK,
   MELSPEC or PLP -- with HParm's configuration variables and their defaults, HParm.c:337-367; WARPFREQ, WARPLCUTOFF and WARPUCUTOFF
   among them: a one-warp front end, refused with the library's reason on a triple that ValidCodeParms or WarpFreq cannot take); the
   differentials, _Z and _N of TARGETKIND follow in load_observations as for parameter files.  Returns the parameter kind of the table
   (base kind + _0 / _E). */
static int code_waveforms(const strlist *files, int first, int count, int targetKind, const config *cfg, obs_batch *ob, float **dStatOut, int *nStatOut)
{
   const char *sfmt = cfg_get(cfg, "SOURCEFORMAT");
   const int fmt = (sfmt && !strcasecmp(sfmt, "WAV")) ? HTKAMD_WAVE_WAV : HTKAMD_WAVE_HTK;
   check_waveform_kind(targetKind);
   check_waveform_warp(cfg);
   const int base = targetKind & 077;
   short *all = NULL; size_t cap = 0;
   int *sampOff = (int *)calloc((size_t)count + 1, sizeof(int));
   double period = cfg_flt(cfg, "SOURCERATE", 0.0);
   for (int u = 0; u < count; u++) {
      short *x; long n; double per;
      CHECK(htkamd_wave_read(files->v[first + u], fmt, &x, &n, &per));
      if (period <= 0.0) period = per;                               /* SOURCERATE, when set, replaces the header's value (HParm.c:3940) */
      const size_t need = (size_t)sampOff[u] + (size_t)n;
      if (need > cap) { cap = need * 2 + 4096; all = (short *)realloc(all, sizeof(short) * cap); }
      memcpy(all + sampOff[u], x, sizeof(short) * (size_t)n);
      sampOff[u + 1] = sampOff[u] + (int)n;
      htkamd_free(x);
   }
   htkamd_frontend_config fc; memset(&fc, 0, sizeof(fc));
   htkamd_mfcc_config *const m = &fc.base;
   fc.baseKind = base; fc.lpcOrder = cfg_int(cfg, "LPCORDER", 12); fc.compressFact = (float)cfg_flt(cfg, "COMPRESSFACT", 0.33);
   m->sampPeriod = period; m->winDur = cfg_flt(cfg, "WINDOWSIZE", 256000.0); m->frPeriod = cfg_flt(cfg, "TARGETRATE", 100000.0);
   m->numChans = cfg_int(cfg, "NUMCHANS", 20); m->numCeps = cfg_int(cfg, "NUMCEPS", 12); m->cepLifter = cfg_int(cfg, "CEPLIFTER", 22);
   m->preEmph = (float)cfg_flt(cfg, "PREEMCOEF", 0.97); m->useHam = cfg_bool(cfg, "USEHAMMING", 1); m->usePower = cfg_bool(cfg, "USEPOWER", 0);
   m->zMeanSource = cfg_bool(cfg, "ZMEANSOURCE", 0); m->rawEnergy = cfg_bool(cfg, "RAWENERGY", 1); m->eNormalise = cfg_bool(cfg, "ENORMALISE", 1);
   m->loFreq = (float)cfg_flt(cfg, "LOFREQ", -1.0); m->hiFreq = (float)cfg_flt(cfg, "HIFREQ", -1.0); m->cepScale = (float)cfg_flt(cfg, "CEPSCALE", 1.0);
   m->silFloor = (float)cfg_flt(cfg, "SILFLOOR", 50.0); m->eScale = (float)cfg_flt(cfg, "ESCALE", 0.1);
   m->hasC0 = (targetKind & PK_HASZEROC) != 0; m->hasE = (targetKind & PK_HASENERGY) != 0;
   m->delWin = 2; m->accWin = 2;
   const int cols = htkamd_frontend_num_cols(&fc);
   if (cols < 0) DIE("waveform sources: %s", htkamd_last_error());
   const htkamd_warp warp = waveform_warp(cfg);
   htkamd_frontend *fe;
   { const int rc = htkamd_frontend_create_warped(&fc, &warp, 1, &fe); if (rc == HTKAMD_EINVAL) DIE("waveform sources: %s", htkamd_last_error()); CHECK(rc); }
   int F = 0;
   for (int u = 0; u < count; u++) F += htkamd_frontend_num_frames(&fc, sampOff[u + 1] - sampOff[u]);
   short *dWav; float *dStat;
   CHECK(htkamd_dev_malloc((void **)&dWav, sizeof(short) * (size_t)(sampOff[count] ? sampOff[count] : 1)));
   CHECK(htkamd_memcpy_h2d(dWav, all, sizeof(short) * (size_t)sampOff[count], NULL));
   CHECK(htkamd_dev_malloc((void **)&dStat, sizeof(float) * (size_t)(F ? F : 1) * cols));
   CHECK(htkamd_frontend_compute(fe, dWav, sampOff, count, ob->frameOff, dStat, NULL));
   CHECK(htkamd_stream_sync(NULL));
   CHECK(htkamd_dev_free(dWav)); htkamd_frontend_destroy(fe); free(all); free(sampOff);
   ob->period = (int)(m->frPeriod + 0.5);
   *dStatOut = dStat; *nStatOut = cols;
   return base | (m->hasC0 ? PK_HASZEROC : 0) | (m->hasE ? PK_HASENERGY : 0);
}

/* ---- side-based cepstral mean and variance normalisation (HParm.c:3172-3349, :1728-1741, :1793-1812) ----
 * CMEANDIR / CMEANMASK [/ CMEANPATHMASK]: with _Z in TARGETKIND (and not in the files) the mean vector of the file's side --
 * <CMEANDIR>/[<path mask's capture>/]<mask's capture> -- is subtracted in place of the utterance's own mean.  VARSCALEDIR / VARSCALEMASK
 * [/ VARSCALEPATHMASK] + VARSCALEFN: every column is scaled by sqrt(global variance / side variance).  For parameter files and waveforms alike. */
static const char *const side_norm_vars[] = {"CMEANDIR", "CMEANMASK", "CMEANPATHMASK", "VARSCALEDIR", "VARSCALEMASK", "VARSCALEPATHMASK", "VARSCALEFN", NULL};
static int side_mean_set(const config *c) { return cfg_get(c, "CMEANDIR") || cfg_get(c, "CMEANMASK"); }       /* HParm.c:4376 */
static int side_var_set(const config *c) { return cfg_get(c, "VARSCALEDIR") || cfg_get(c, "VARSCALEMASK"); }  /* HParm.c:4380 */

/* what can be refused from the configuration alone; the drivers call this before they touch a device */
static void check_side_norm(const config *c)
{
   if (side_mean_set(c) && !(cfg_get(c, "CMEANDIR") && cfg_get(c, "CMEANMASK"))) DIE("side mean (CMEANDIR / CMEANMASK): mask or dir missing");
   if (side_var_set(c) && !(cfg_get(c, "VARSCALEDIR") && cfg_get(c, "VARSCALEMASK"))) DIE("side variance (VARSCALEDIR / VARSCALEMASK): mask or dir missing");
   if (side_var_set(c) && !cfg_get(c, "VARSCALEFN")) DIE("VARSCALEDIR is set without VARSCALEFN: the side variances have no global variance to be scaled to");
   if (cfg_get(c, "VARSCALEFN") && !side_var_set(c)) DIE("VARSCALEFN without VARSCALEDIR / VARSCALEMASK: no variance scaling vector found");
   if ((side_mean_set(c) || side_var_set(c)) &&            /* what the reference mixes into this step and this path does not serve */
       (cfg_get(c, "MATTRANFN") || cfg_get(c, "SIDEXFORMMASK") || cfg_bool(c, "USEOLDXFORMCVN", 0) || cfg_bool(c, "HIGHDIFF", 0)))
      DIE("side normalisation together with MATTRANFN, SIDEXFORMMASK, USEOLDXFORMCVN or HIGHDIFF is not supported");
}

/* the side files read so far: each is read once per process */
typedef struct { strlist path; float **vec; int *dim, *kind; } side_cache;
static side_cache g_sideMeans, g_sideVars;
static const float *side_vector(side_cache *sc, int wantVar, const char *what, const char *dir, const char *mask, const char *pathMask, const char *fname,
                                int targetKind, int *dim, const char **pathOut)
{
   char side[1024], sub[1024], path[4096];
   int rc = htkamd_mask_match(mask, fname, side, sizeof(side));
   if (rc < 0) DIE("%s", htkamd_last_error());
   if (rc == 0) DIE("%s: non-matching mask %s (file %s)", what, mask, fname);
   if (pathMask) {
      rc = htkamd_mask_match(pathMask, fname, sub, sizeof(sub));
      if (rc < 0) DIE("%s", htkamd_last_error());
      if (rc == 0) DIE("%s: non-matching path mask %s (file %s)", what, pathMask, fname);
      snprintf(path, sizeof(path), "%s/%s/%s", dir, sub, side);
   } else snprintf(path, sizeof(path), "%s/%s", dir, side);
   int i;
   for (i = 0; i < sc->path.n; i++) if (!strcmp(sc->path.v[i], path)) break;
   if (i == sc->path.n) {
      float buf[4096];
      int kind, d = 0;
      if (wantVar) CHECK(htkamd_cepsnorm_read(path, &kind, NULL, NULL, NULL, buf, &d, 4096));
      else CHECK(htkamd_cepsnorm_read(path, &kind, NULL, buf, &d, NULL, NULL, 4096));
      if (d == 0) DIE("%s: %s missing in %s", what, wantVar ? "<VARIANCE>" : "<MEAN>", path);
      sl_add(&sc->path, path);
      sc->vec = (float **)realloc(sc->vec, sizeof(float *) * (size_t)sc->path.n);
      sc->dim = (int *)realloc(sc->dim, sizeof(int) * (size_t)sc->path.n);
      sc->kind = (int *)realloc(sc->kind, sizeof(int) * (size_t)sc->path.n);
      sc->vec[i] = (float *)malloc(sizeof(float) * (size_t)d); memcpy(sc->vec[i], buf, sizeof(float) * (size_t)d);
      sc->dim[i] = d; sc->kind[i] = kind;
   }
   if (htkamd_cepsnorm_check_kinds(targetKind, wantVar ? -1 : sc->kind[i], wantVar ? sc->kind[i] : -1)) DIE("%s: %s", sc->path.v[i], htkamd_last_error());
   *dim = sc->dim[i]; *pathOut = sc->path.v[i];
   return sc->vec[i];
}

/* the tail of AddQualifiers on the table of a batch: every file goes to its side through the masks; the sides of the batch get one row
   each in the mean and scale tables, and the device normalises in place (htkamd_parm_normalise) */
static void normalise_sides(const strlist *files, int first, int count, int targetKind, int useMean, const config *cfg, int cols, const int *frameOff, float *dX)
{
   const int useVar = side_var_set(cfg);
   if (!useMean && !useVar) return;
   /* _N: the reference applies the side vectors while the energy column is still in the row (AddQualifiers) and drops it when an
      observation is extracted (HParm.c:2882); here the column is gone by now, so vectors beyond the statics would meet the wrong columns */
   if (targetKind & PK_HASNULLE) DIE("side normalisation (CMEAN* / VARSCALE*) with _N in TARGETKIND is not supported");
   static float *varScale = NULL; static int dVS = 0;
   if (useVar && !varScale) {                              /* LoadVarScale: once per process */
      varScale = (float *)malloc(sizeof(float) * 4096);
      CHECK(htkamd_varscale_read(cfg_get(cfg, "VARSCALEFN"), varScale, &dVS, 4096));
   }
   strlist keys = {0};
   int *uttSide = (int *)calloc((size_t)count + 1, sizeof(int));
   float *mean = NULL, *var = NULL, *scale = NULL;
   const char **names = NULL;
   int dMean = 0, dVar = 0, nSide = 0;
   for (int u = 0; u < count; u++) {
      const char *fn = files->v[first + u], *mp = "", *vp = "";
      const float *mv = NULL, *vv = NULL;
      int dm = 0, dv = 0;
      if (useMean) mv = side_vector(&g_sideMeans, 0, "side mean (CMEANMASK)", cfg_get(cfg, "CMEANDIR"), cfg_get(cfg, "CMEANMASK"), cfg_get(cfg, "CMEANPATHMASK"), fn, targetKind, &dm, &mp);
      if (useVar) vv = side_vector(&g_sideVars, 1, "side variance (VARSCALEMASK)", cfg_get(cfg, "VARSCALEDIR"), cfg_get(cfg, "VARSCALEMASK"), cfg_get(cfg, "VARSCALEPATHMASK"), fn, targetKind, &dv, &vp);
      if (u == 0) { dMean = dm; dVar = dv; }
      if (dm != dMean || dv != dVar) DIE("%s: the side's vectors have %d / %d values, those of the batch's first file %d / %d", fn, dm, dv, dMean, dVar);
      if (dMean > cols || dVar > cols) DIE("%s: side vectors of %d / %d values for observations of %d", fn, dMean, dVar, cols);
      char key[8192]; snprintf(key, sizeof(key), "%s|%s", mp, vp);
      int s;
      for (s = 0; s < nSide; s++) if (!strcmp(keys.v[s], key)) break;
      if (s == nSide) {
         sl_add(&keys, key); nSide++;
         mean = (float *)realloc(mean, sizeof(float) * (size_t)nSide * (size_t)(dMean ? dMean : 1));
         var = (float *)realloc(var, sizeof(float) * (size_t)nSide * (size_t)(dVar ? dVar : 1));
         names = (const char **)realloc((void *)names, sizeof(char *) * (size_t)nSide);
         if (mv) memcpy(mean + (size_t)s * dMean, mv, sizeof(float) * (size_t)dMean);
         if (vv) memcpy(var + (size_t)s * dVar, vv, sizeof(float) * (size_t)dVar);
         names[s] = vp;
      }
      uttSide[u] = s;
   }
   if (useVar && nSide) {
      scale = (float *)malloc(sizeof(float) * (size_t)nSide * (size_t)dVar);
      if (htkamd_cepsnorm_scale(varScale, dVS, var, dVar, nSide, names, scale)) DIE("variance scaling (VARSCALEFN %s): %s", cfg_get(cfg, "VARSCALEFN"), htkamd_last_error());
   }
   CHECK(htkamd_parm_normalise(dX, frameOff, uttSide, count, nSide, cols, useMean ? mean : NULL, dMean, scale, dVar, NULL));
   for (int s = 0; s < nSide; s++) free(keys.v[s]);
   free(keys.v); free(uttSide); free(mean); free(var); free(scale); free((void *)names);
}

/* ---- the input transform of the model set (<INPUTXFORM>, inline or ~j): ApplyStaticMat, HParm.c:1235 ----
 * The drivers honour the transform of the set they load (the configuration variable MATTRANFN stays ignored): load_observations hands the
 * qualifier step to htkamd_inputxform_apply, which runs transform and qualifiers in the reference's order.  Together with side
 * normalisation (CMEAN* / VARSCALE*) a transformed set is refused: that combination is not served. */
static const htkamd_inputxform *g_inputXf;
static const char *g_inputXfSetId;
static int g_inputXfVecSize;
static void use_input_xform(const htkamd_mmf *mmf)
{
   g_inputXf = htkamd_mmf_inputxform(mmf); g_inputXfSetId = htkamd_mmf_set_id(mmf); g_inputXfVecSize = htkamd_mmf_vec_size(mmf);
}
static void refuse_xform_with_side_norm(const config *cfg, const htkamd_mmf *mmf)
{
   if (htkamd_mmf_inputxform(mmf) && (side_mean_set(cfg) || side_var_set(cfg)))
      DIE("a model set with an input transform (INPUTXFORM) together with side normalisation (CMEAN* / VARSCALE*) is not supported");
}
/* The same before a device is touched: with side normalisation configured the model files are read once more on the host alone, only to
   see whether the set carries a transform.  A set that cannot be read is the business of the load proper, with its own message. */
static void check_input_xform(const config *cfg, const strlist *mmfs, const char *hmmList, const char *hmmDir, const char *hmmExt)
{
   if (!side_mean_set(cfg) && !side_var_set(cfg)) return;
   htkamd_mmf *m;
   if (htkamd_mmf_create(&m)) return;
   int rc = 0;
   for (int i = 0; i < mmfs->n && !rc; i++) rc = htkamd_mmf_read(m, mmfs->v[i], NULL);
   if (!rc) rc = htkamd_mmf_finish(m, hmmList, hmmDir, hmmExt);
   if (!rc) refuse_xform_with_side_norm(cfg, m);
   htkamd_mmf_destroy(m);
}

static void load_observations(const strlist *files, int first, int count, int targetKind, const config *cfg, obs_batch *ob)
{
   float *stat = NULL; size_t cap = 0;
   int nStat = 0, fileKind = -1;
   float *dStat = NULL;
   ob->nUtt = count; ob->frameOff = (int *)calloc((size_t)count + 1, sizeof(int)); ob->period = 100000;
   const int waveform = waveform_source(cfg);
   if (waveform) fileKind = code_waveforms(files, first, count, targetKind, cfg, ob, &dStat, &nStat);
   else
   for (int u = 0; u < count; u++) {
      float *x; int T, cols, pk, per;
      CHECK(htkamd_parm_read(files->v[first + u], &x, &T, &cols, &per, &pk));
      if (u == 0) { nStat = cols; fileKind = pk; ob->period = per; }
      if (cols != nStat || pk != fileKind) DIE("%s: kind/width differs from the first file of the batch", files->v[first + u]);
      const size_t need = (size_t)(ob->frameOff[u] + T) * nStat;
      if (need > cap) { cap = need * 2 + 4096; stat = (float *)realloc(stat, sizeof(float) * cap); }
      memcpy(stat + (size_t)ob->frameOff[u] * nStat, x, sizeof(float) * (size_t)T * nStat);
      ob->frameOff[u + 1] = ob->frameOff[u] + T;
      htkamd_free(x);
   }
   if (targetKind < 0) targetKind = fileKind;
   if ((targetKind & 077) != (fileKind & 077)) DIE("files hold base kind %s, TARGETKIND wants %s", pk_base[fileKind & 077], pk_base[targetKind & 077]);
   const int add = targetKind & ~fileKind, lost = fileKind & ~targetKind;
   if (lost & ~PK_HASNULLE) DIE("TARGETKIND drops qualifiers the files have (0%o)", lost);
   if (add & (PK_HASENERGY | PK_HASZEROC)) DIE("TARGETKIND asks for _E / _0, which cannot be derived from parameter files");
   const int F = ob->frameOff[count];
   if (!waveform) {
      CHECK(htkamd_dev_malloc((void **)&dStat, sizeof(float) * (size_t)(F ? F : 1) * nStat));
      CHECK(htkamd_memcpy_h2d(dStat, stat, sizeof(float) * (size_t)F * nStat, NULL));
      free(stat);
   }
   if (g_inputXf) {                                        /* a transformed set: the checks of HParm.c:1636-1647, :1835, :1256, :2199-2208, :691, then the whole step */
      if (htkamd_inputxform_check(g_inputXf, fileKind, targetKind, nStat, g_inputXfSetId, g_inputXfVecSize)) DIE("%s", htkamd_last_error());
      htkamd_parm_quals q; memset(&q, 0, sizeof(q));
      const int nE = ((fileKind & PK_HASENERGY) ? 1 : 0) + ((fileKind & PK_HASZEROC) ? 1 : 0);
      q.nStat = nStat; q.nullECol = -1;
      q.hasD = (targetKind & PK_HASDELTA) != 0; q.hasA = (targetKind & PK_HASACCS) != 0; q.hasT = (targetKind & PK_HASTHIRD) != 0;
      q.delWin = cfg_int(cfg, "DELTAWINDOW", 2); q.accWin = cfg_int(cfg, "ACCWINDOW", 2); q.thirdWin = cfg_int(cfg, "THIRDWINDOW", 2);
      q.nZeroMean = (add & PK_HASZEROM) ? nStat - nE + ((targetKind & PK_HASZEROC) ? 1 : 0) : 0;                 /* HParm.c:1712-1715 */
      q.v1Compat = cfg_bool(cfg, "V1COMPAT", 0); q.simpleDiffs = cfg_bool(cfg, "SIMPLEDIFFS", 0);
      ob->cols = htkamd_inputxform_apply_cols(g_inputXf, &q);
      CHECK(htkamd_dev_malloc((void **)&ob->dX, sizeof(float) * (size_t)(F ? F : 1) * ob->cols));
      CHECK(htkamd_inputxform_apply(g_inputXf, dStat, ob->frameOff, count, &q, ob->dX, NULL));
      CHECK(htkamd_dev_free(dStat));
      return;
   }
   /* a side mean takes the place of the utterance's own (HParm.c:1709-1741, :4375): _Z asked for, not in the files, CMEANDIR / CMEANMASK set */
   const int sideMean = side_mean_set(cfg) && (add & PK_HASZEROM);
   if (add == 0) { ob->dX = dStat; ob->cols = nStat; normalise_sides(files, first, count, targetKind, 0, cfg, ob->cols, ob->frameOff, ob->dX); return; }
   if (fileKind & (PK_HASDELTA | PK_HASACCS | PK_HASTHIRD)) DIE("files already carry differentials: further qualifiers cannot be appended");
   htkamd_parm_quals q; memset(&q, 0, sizeof(q));
   const int nE = ((fileKind & PK_HASENERGY) ? 1 : 0) + ((fileKind & PK_HASZEROC) ? 1 : 0), base = nStat - nE;
   q.nStat = nStat;
   q.hasD = (targetKind & PK_HASDELTA) != 0; q.hasA = (targetKind & PK_HASACCS) != 0; q.hasT = (targetKind & PK_HASTHIRD) != 0;
   q.delWin = cfg_int(cfg, "DELTAWINDOW", 2); q.accWin = cfg_int(cfg, "ACCWINDOW", 2); q.thirdWin = cfg_int(cfg, "THIRDWINDOW", 2);
   q.nZeroMean = ((add & PK_HASZEROM) && !sideMean) ? base + (((targetKind & PK_HASZEROC) && !(targetKind & PK_HASNULLE)) ? 1 : 0) : 0;   /* HParm.c:1712-1715 */
   q.nullECol = ((targetKind & PK_HASNULLE) && nE) ? base : -1;
   q.v1Compat = cfg_bool(cfg, "V1COMPAT", 0); q.simpleDiffs = cfg_bool(cfg, "SIMPLEDIFFS", 0);
   ob->cols = htkamd_parm_quals_cols(&q);
   CHECK(htkamd_dev_malloc((void **)&ob->dX, sizeof(float) * (size_t)(F ? F : 1) * ob->cols));
   CHECK(htkamd_parm_qualify(dStat, ob->frameOff, count, &q, ob->dX, NULL));
   CHECK(htkamd_stream_sync(NULL));
   CHECK(htkamd_dev_free(dStat));
   normalise_sides(files, first, count, targetKind, sideMean, cfg, ob->cols, ob->frameOff, ob->dX);
}

static void free_observations(obs_batch *ob) { if (ob->dX) htkamd_dev_free(ob->dX); free(ob->frameOff); memset(ob, 0, sizeof(*ob)); }

/* --help: the configuration variables the drivers honour */
static void print_config_help(FILE *f)
{
   fprintf(f, "Configuration variables (-C file):\n"
              "  TARGETKIND DELTAWINDOW ACCWINDOW THIRDWINDOW V1COMPAT SIMPLEDIFFS\n"
              "  waveform sources (SOURCEFORMAT = WAV or SOURCEKIND = WAVEFORM): SOURCERATE TARGETRATE WINDOWSIZE NUMCHANS NUMCEPS CEPLIFTER\n"
              "    PREEMCOEF USEHAMMING USEPOWER ZMEANSOURCE RAWENERGY ENORMALISE LOFREQ HIFREQ CEPSCALE SILFLOOR ESCALE LPCORDER COMPRESSFACT\n"
              "    WARPFREQ WARPLCUTOFF WARPUCUTOFF\n"
              "  side-based mean and variance normalisation:");
   for (int i = 0; side_norm_vars[i]; i++) fprintf(f, " %s", side_norm_vars[i]);
   fprintf(f, "\n");
}

/* ---- option scanning in HTK's style: switches first ("-x", optionally followed by values), then positional arguments ---- */
typedef struct { int argc, at; char **argv; } args;
static int is_switch(const char *s) { return s[0] == '-' && s[1] && !isdigit((unsigned char)s[1]) && s[1] != '.'; }
static const char *next_switch(args *a) { return (a->at < a->argc && is_switch(a->argv[a->at])) ? a->argv[a->at++] + 1 : NULL; }
static const char *str_arg(args *a, const char *sw) { if (a->at >= a->argc) DIE("-%s: value expected", sw); return a->argv[a->at++]; }
static double flt_arg(args *a, const char *sw) { return atof(str_arg(a, sw)); }
static __attribute__((unused)) int has_num_arg(const args *a) { return a->at < a->argc && !is_switch(a->argv[a->at]) && (isdigit((unsigned char)a->argv[a->at][0]) || a->argv[a->at][0] == '.' || a->argv[a->at][0] == '-'); }

#endif
