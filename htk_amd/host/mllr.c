/* mllr.c -- MLLR mean transforms over a regression class tree: what HERest -u a does at transform time (HAdapt.c), from a pass's
 * statistics.  Restated from the reference:
 *   SetNodeOcc :1510, ParseNode :1547, ParseTree :1585, GetSplitThresh :435: which nodes get a transform, in which order, for which classes
 *   PutAdaptXForm (HModel.c:3196), PutXFormSet :3154, PutLinXForm :3116, PutBias :2820, PutTransform :2800, SaveOneXForm :4804: the file
 * The statistics of the classes, the sums up the tree and the solves run on the device (csrc/mllr.hip).
 *
 * The per-Gaussian sums: htkamd_accs keeps mu = sum of gamma (o - mu_m) (HFB.c UpMixParms subtracts the mean; csrc/update.hip adds
 * mu / muOcc to the old mean), so the reference's spSum = sum of gamma o is mu + muOcc mu_m, formed here in fp64 and rounded to float once,
 * which is the type the reference keeps it in (RegAcc).
 *
 * Not served, each refused by name: CMLLR, MLLRCOV, MLLRDIAGCOV and semi-tied transforms, <PARENTXFORM> chains, <ADAPTKIND> BASE,
 * multi-stream, FULLC, tied-mixture and discrete sets. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <ctype.h>
#include "mmf_priv.h"
#include "htktext.h"

#pragma weak htkamd_mllr_dev_stats
#pragma weak htkamd_mllr_dev_fetch
#pragma weak htkamd_mllr_dev_solve
#pragma weak htkamd_mllr_dev_times
#pragma weak htkamd_mllr_dev_close
#pragma weak htkamd_mllr_dev_apply
#pragma weak htkamd_mllr_dev_restore
#pragma weak htkamd_mllr_model_state
#pragma weak htkamd_accs_get_layout
#pragma weak htkamd_accs_download
#pragma weak htkamd_model_get_params

#define ML_DEFAULT_SPLIT 1000.0f                        /* mllrMeanSplitThresh */

struct htkamd_xformset {
   char *name, *baseName;
   int D, nBlocks, *blockSize, useBias;
   int nX; float *A, *bias, *logdet;                    /* [nX][D][D] zero outside the blocks, [nX][D], [nX] */
   int nClass, *classX;                                 /* transform (from 1) of class c, 0 = none */
   int nNodes, *xNode; double *nodeOcc;                 /* estimate: the node (from 1) of every transform, SetNodeOcc's occupations */
   int G, *gaussClass;                                  /* estimate: base class (from 1) of every Gaussian of the set, 0 = none */
   float ms[3];
};

/* ------------------------------------------------------------------------------------------ configuration */
static int ml_blocks(const char *who, const htkamd_mllr_config *cfg, int D, int *nBlocks, const int **blockSize, int *one)
{
   if (!cfg || cfg->nBlocks <= 0) { *one = D; *nBlocks = 1; *blockSize = one; }      /* the default: one block of D */
   else { *nBlocks = cfg->nBlocks; *blockSize = cfg->blockSize; }
   if (!*blockSize) { htkamd_set_error("%s: BLOCKSIZE: %d blocks and no sizes", who, *nBlocks); return HTKAMD_EINVAL; }
   int sum = 0;
   for (int b = 0; b < *nBlocks; b++) {
      const int bs = (*blockSize)[b];
      if (bs < 1) { htkamd_set_error("%s: BLOCKSIZE: block %d has size %d", who, b + 1, bs); return HTKAMD_EINVAL; }
      if (bs > HTKAMD_MLLR_MAXBLOCK) { htkamd_set_error("%s: BLOCKSIZE: block %d has size %d (at most %d)", who, b + 1, bs, HTKAMD_MLLR_MAXBLOCK); return HTKAMD_EINVAL; }
      sum += bs;
   }
   if (sum != D) { htkamd_set_error("%s: BLOCKSIZE: the blocks sum to %d, the vector size is %d", who, sum, D); return HTKAMD_EINVAL; }
   return HTKAMD_OK;
}

/* doubles in a node's record of statistics (csrc/mllr.hip): per row of a block of size bs a triangle of (bs+1)(bs+2)/2 and a vector of bs+1; the occupation */
size_t htkamd_mllr_record_len(int D, int nBlocks, const int *blockSize)
{
   size_t n = 0; int sum = 0;
   if (D < 1 || nBlocks < 1 || !blockSize) return 0;
   for (int b = 0; b < nBlocks; b++) {
      const size_t bs = (size_t)blockSize[b];
      if (blockSize[b] < 1 || blockSize[b] > HTKAMD_MLLR_MAXBLOCK) return 0;
      n += bs * ((bs + 1) * (bs + 2) / 2 + bs + 1); sum += blockSize[b];
   }
   return sum == D ? n + 1 : 0;
}

static float ml_thresh(const htkamd_mllr_config *cfg) { return (cfg && cfg->splitThresh > 0.0f) ? cfg->splitThresh : ML_DEFAULT_SPLIT; }      /* GetSplitThresh: SPLITTHRESH, else MLLRMEANSPLITTHRESH */

/* base class (from 1, the terminals in node order) of every Gaussian of the set, 0 = in no class */
static int ml_gauss_classes(const char *who, const htkamd_mmf *s, const htkamd_regtree *t, int *cls)
{
   memset(cls, 0, sizeof(int) * (size_t)(s->nG ? s->nG : 1));
   const int nNodes = htkamd_regtree_num_nodes(t);
   for (int node = 1, c = 0; node <= nNodes; node++) {
      int l = 0, r = 0;
      htkamd_regtree_children(t, node, &l, &r);
      if (l) continue;
      c++;
      const int n = htkamd_regtree_num_components(t, node);
      for (int i = 0; i < n; i++) {
         int j = 0, mix = 0;
         const char *name = htkamd_regtree_component(t, node, i, &j, &mix);
         const int h = name ? htkamd_mmf_find_logical(s, name) : -1;
         if (h < 0) { htkamd_set_error("%s: the tree's component %s.state[%d].mix[%d] (class %d): the set has no model %s", who, name ? name : "?", j, mix, c, name ? name : "?"); return HTKAMD_EMODEL; }
         if (j < 2 || j >= s->hm[h].N) { htkamd_set_error("%s: the tree's component %s.state[%d].mix[%d] (class %d): the model has the emitting states 2 .. %d", who, name, j, mix, c, s->hm[h].N - 1); return HTKAMD_EMODEL; }
         const mmf_state *st = &s->st[s->hm[h].state[j - 1]];
         if (mix < 1 || mix > st->nMix) { htkamd_set_error("%s: the tree's component %s.state[%d].mix[%d] (class %d): the state has %d mixture components", who, name, j, mix, c, st->nMix); return HTKAMD_EMODEL; }
         const int g = s->cg[st->comp0 + mix - 1];
         if (cls[g] && cls[g] != c) { htkamd_set_error("%s: the tree's component %s.state[%d].mix[%d] is in class %d and in class %d", who, name, j, mix, cls[g], c); return HTKAMD_EMODEL; }
         cls[g] = c;
      }
   }
   return HTKAMD_OK;
}

static int ml_check(const char *who, const htkamd_mmf *s, const htkamd_regtree *t, const htkamd_mllr_config *cfg, int **clsOut)
{
   if (!s || !s->finished) { htkamd_set_error("%s: bad argument", who); return HTKAMD_EINVAL; }
   if (s->nStreams > 1) { htkamd_set_error("%s: a set with more than one stream (%d) is not supported", who, s->nStreams); return HTKAMD_EMODEL; }
   if (s->fullc) { htkamd_set_error("%s: FULLC sets are not supported", who); return HTKAMD_EMODEL; }
   if (s->tiedMix) { htkamd_set_error("%s: tied-mixture sets are not supported", who); return HTKAMD_EMODEL; }
   if (strstr(s->kind, "DISCRETE")) { htkamd_set_error("%s: discrete sets are not supported", who); return HTKAMD_EMODEL; }
   if (s->gMeanMac) for (int g = 0; g < s->nG && g < s->capMac; g++) if (s->gMeanMac[g] >= 0) { htkamd_set_error("%s: sets with shared mean vectors (~u) are not supported", who); return HTKAMD_EMODEL; }
   if (!t) { htkamd_set_error("%s: ADAPTKIND = BASE (no regression class tree) is not supported", who); return HTKAMD_EINVAL; }
   int nb, one; const int *bsz;
   int rc = ml_blocks(who, cfg, s->vecSize, &nb, &bsz, &one);
   if (rc) return rc;
   int *cls = (int *)malloc(sizeof(int) * (size_t)(s->nG ? s->nG : 1));
   rc = ml_gauss_classes(who, s, t, cls);
   if (rc || !clsOut) free(cls); else *clsOut = cls;
   return rc;
}

int htkamd_mllr_check(const htkamd_mmf *s, const htkamd_regtree *t, const htkamd_mllr_config *cfg) { return ml_check("mllr_check", s, t, cfg, NULL); }

int htkamd_mllr_gauss_classes(const htkamd_mmf *s, const htkamd_regtree *t, int *cls)
{
   if (!s || !t || !cls) { htkamd_set_error("mllr_gauss_classes: bad argument"); return HTKAMD_EINVAL; }
   return ml_gauss_classes("mllr_gauss_classes", s, t, cls);
}

/* ------------------------------------------------------------------------------------------ which nodes get a transform */
typedef struct { int nNodes; const int *left, *right; const double *occ; float thresh; int *termClass; int nX, *xNode, *classX, nClass; } ml_sel;

static void ml_gen(ml_sel *p, int node, const unsigned char *classes)      /* GenXForm: the next transform, for the marked classes */
{
   p->xNode[p->nX++] = node;
   for (int c = 0; c < p->nClass; c++) if (classes[c]) p->classX[c] = p->nX;
}

static int ml_parse_node(ml_sel *p, int node, unsigned char *classes)      /* ParseNode */
{
   const int l = p->left[node - 1], r = p->right[node - 1];
   if ((float)p->occ[node - 1] > p->thresh) {
      unsigned char *lcl = (unsigned char *)calloc((size_t)p->nClass + 1, 1);
      if (l) {
         int gen = 0;
         if (ml_parse_node(p, l, lcl)) gen = 1;
         if (ml_parse_node(p, r, lcl)) gen = 1;
         if (gen) ml_gen(p, node, lcl);
      } else { lcl[p->termClass[node - 1]] = 1; ml_gen(p, node, lcl); }
      free(lcl);
      return 0;
   }
   if (l) { ml_parse_node(p, l, classes); ml_parse_node(p, r, classes); }
   else classes[p->termClass[node - 1]] = 1;
   return 1;
}

int htkamd_mllr_select(int nNodes, const int *left, const int *right, const double *nodeOcc, float thresh, int *nX, int *xNode, int *classX)
{
   if (nNodes < 1 || !left || !right || !nodeOcc || !nX || !xNode || !classX) { htkamd_set_error("mllr_select: bad argument"); return HTKAMD_EINVAL; }
   for (int i = 0; i < nNodes; i++) {
      const int l = left[i], r = right[i];
      if ((l == 0) != (r == 0) || l < 0 || r < 0 || l > nNodes || r > nNodes || (l && (l <= i + 1 || r <= i + 1))) {
         htkamd_set_error("mllr_select: node %d has the children %d, %d (children are numbered behind their parent)", i + 1, l, r); return HTKAMD_EINVAL;
      }
   }
   ml_sel p = { nNodes, left, right, nodeOcc, thresh, (int *)malloc(sizeof(int) * (size_t)nNodes), 0, xNode, classX, 0 };
   for (int i = 0; i < nNodes; i++) p.termClass[i] = left[i] ? -1 : p.nClass++;
   for (int c = 0; c < p.nClass; c++) classX[c] = 0;
   *nX = 0;
   int rc = HTKAMD_MLLR_NOSET;
   if (!((float)nodeOcc[0] < thresh)) {                     /* ParseTree: "not enough data to generate transforms" */
      unsigned char *classes = (unsigned char *)calloc((size_t)p.nClass + 1, 1);
      ml_parse_node(&p, 1, classes);
      free(classes);
      if (p.nX > 0) rc = HTKAMD_OK;
   }
   free(p.termClass);
   *nX = p.nX;
   return rc;
}

/* ------------------------------------------------------------------------------------------ the transform set */
static htkamd_xformset *ml_new(int D, int nBlocks, const int *blockSize, int useBias, int nX, int nClass)
{
   htkamd_xformset *x = (htkamd_xformset *)calloc(1, sizeof(*x));
   x->D = D; x->nBlocks = nBlocks; x->useBias = useBias; x->nX = nX; x->nClass = nClass;
   x->blockSize = (int *)malloc(sizeof(int) * (size_t)nBlocks);
   memcpy(x->blockSize, blockSize, sizeof(int) * (size_t)nBlocks);
   x->A = (float *)calloc((size_t)(nX ? nX : 1) * D * D, sizeof(float));
   x->bias = (float *)calloc((size_t)(nX ? nX : 1) * D, sizeof(float));
   x->logdet = (float *)calloc((size_t)(nX ? nX : 1), sizeof(float));
   x->classX = (int *)calloc((size_t)(nClass ? nClass : 1), sizeof(int));
   return x;
}

void htkamd_xformset_destroy(htkamd_xformset *x)
{
   if (!x) return;
   free(x->name); free(x->baseName); free(x->blockSize); free(x->A); free(x->bias); free(x->logdet); free(x->classX); free(x->xNode); free(x->nodeOcc); free(x->gaussClass);
   free(x);
}

int htkamd_xformset_from_tables(int D, int nBlocks, const int *blockSize, int useBias, int nX, const float *A, const float *bias, int nClass, const int *classX,
                                const char *name, const char *baseName, htkamd_xformset **out)
{
   if (D < 1 || nX < 0 || nClass < 1 || !classX || !out || (nX && !A) || (nX && useBias && !bias)) { htkamd_set_error("xformset_from_tables: bad argument"); return HTKAMD_EINVAL; }
   htkamd_mllr_config cfg = { 0.0f, 0.0f, useBias, nBlocks, blockSize };
   int nb, one; const int *bsz;
   const int rc = ml_blocks("xformset_from_tables", &cfg, D, &nb, &bsz, &one);
   if (rc) return rc;
   for (int c = 0; c < nClass; c++) if (classX[c] < 0 || classX[c] > nX) { htkamd_set_error("xformset_from_tables: class %d names transform %d of %d", c + 1, classX[c], nX); return HTKAMD_EINVAL; }
   htkamd_xformset *x = ml_new(D, nb, bsz, useBias != 0, nX, nClass);
   for (int k = 0; k < nX; k++)
      for (int b = 0, c0 = 0; b < nb; c0 += bsz[b], b++)
         for (int i = c0; i < c0 + bsz[b]; i++)
            for (int j = c0; j < c0 + bsz[b]; j++) x->A[((size_t)k * D + i) * D + j] = A[((size_t)k * D + i) * D + j];
   if (useBias && nX) memcpy(x->bias, bias, sizeof(float) * (size_t)nX * D);
   memcpy(x->classX, classX, sizeof(int) * (size_t)nClass);
   x->name = strdup(name ? name : "mllr"); x->baseName = strdup(baseName ? baseName : "rtree.base");
   *out = x;
   return HTKAMD_OK;
}

int htkamd_xformset_num_xforms(const htkamd_xformset *x) { return x ? x->nX : 0; }
int htkamd_xformset_num_classes(const htkamd_xformset *x) { return x ? x->nClass : 0; }
int htkamd_xformset_vec_size(const htkamd_xformset *x) { return x ? x->D : 0; }
int htkamd_xformset_use_bias(const htkamd_xformset *x) { return x ? x->useBias : 0; }
int htkamd_xformset_class_xform(const htkamd_xformset *x, int baseClass) { return (x && baseClass >= 1 && baseClass <= x->nClass) ? x->classX[baseClass - 1] : 0; }
int htkamd_xformset_xform_node(const htkamd_xformset *x, int xform) { return (x && x->xNode && xform >= 1 && xform <= x->nX) ? x->xNode[xform - 1] : 0; }
int htkamd_xformset_blocks(const htkamd_xformset *x, int *blockSize, int cap)
{
   if (!x) return 0;
   if (blockSize) for (int b = 0; b < x->nBlocks && b < cap; b++) blockSize[b] = x->blockSize[b];
   return x->nBlocks;
}
int htkamd_xformset_xform(const htkamd_xformset *x, int xform, float *A, float *bias)
{
   if (!x || xform < 1 || xform > x->nX) { htkamd_set_error("xformset_xform: transform %d of %d", xform, x ? x->nX : 0); return HTKAMD_EINVAL; }
   if (A) memcpy(A, x->A + (size_t)(xform - 1) * x->D * x->D, sizeof(float) * (size_t)x->D * x->D);
   if (bias) memcpy(bias, x->bias + (size_t)(xform - 1) * x->D, sizeof(float) * (size_t)x->D);
   return HTKAMD_OK;
}
int htkamd_xformset_node_occ(const htkamd_xformset *x, double *occ, int cap)
{
   if (!x || !x->nodeOcc) return 0;
   if (occ) for (int n = 0; n < x->nNodes && n < cap; n++) occ[n] = x->nodeOcc[n];
   return x->nNodes;
}
void htkamd_xformset_kernel_ms(const htkamd_xformset *x, float *ms) { if (ms) for (int k = 0; k < 3; k++) ms[k] = x ? x->ms[k] : 0.0f; }

/* ------------------------------------------------------------------------------------------ the file */
int htkamd_xformset_write(const htkamd_xformset *x, const char *path)
{
   if (!x || !path) { htkamd_set_error("xformset_write: bad argument"); return HTKAMD_EINVAL; }
   FILE *f = fopen(path, "w");
   if (!f) { htkamd_set_error("xformset_write: cannot create output file %s", path); return HTKAMD_EIO; }
   const int D = x->D;
   fprintf(f, "~a "); htx_write_string(f, x->name, '"', 0); fprintf(f, "\n");
   fprintf(f, "<ADAPTKIND>TREE\n");
   fprintf(f, "<BASECLASS>~b "); htx_write_string(f, x->baseName, '"', 0); fprintf(f, "\n");
   fprintf(f, "<XFORMSET>\n<XFORMKIND>MLLRMEAN\n<NUMXFORMS> %d\n", x->nX);
   for (int k = 0; k < x->nX; k++) {
      fprintf(f, "<LINXFORM> %d\n<VECSIZE> %d\n", k + 1, D);
      if (x->useBias) {
         fprintf(f, "<OFFSET>\n<BIAS> %d\n", D);
         for (int i = 0; i < D; i++) fprintf(f, " %e", x->bias[(size_t)k * D + i]);
         fprintf(f, "\n");
      }
      if (x->logdet[k] != 0.0f) fprintf(f, "<LOGDET> %e\n", x->logdet[k]);
      fprintf(f, "<BLOCKINFO> %d", x->nBlocks);
      for (int b = 0; b < x->nBlocks; b++) fprintf(f, " %d", x->blockSize[b]);
      fprintf(f, "\n");
      for (int b = 0, c0 = 0; b < x->nBlocks; c0 += x->blockSize[b], b++) {
         const int bs = x->blockSize[b];
         fprintf(f, "<BLOCK> %d\n<XFORM> %d %d\n", b + 1, bs, bs);
         for (int i = c0; i < c0 + bs; i++) {
            for (int j = c0; j < c0 + bs; j++) fprintf(f, " %e", x->A[((size_t)k * D + i) * D + j]);
            fprintf(f, "\n");
         }
      }
   }
   fprintf(f, "<XFORMWGTSET>\n");
   for (int c = 0; c < x->nClass; c++) fprintf(f, "<CLASSXFORM> %d %d\n", c + 1, x->classX[c]);
   if (fclose(f)) { htkamd_set_error("xformset_write: writing %s failed", path); return HTKAMD_EIO; }
   return HTKAMD_OK;
}

/* tokens of the text form: <KEY> (upper-cased, without the brackets, kind 1), ~c (kind 2), a quoted or plain word (kind 0) */
typedef struct { const char *p, *end; char tok[512]; int kind; } ml_rd;
static int ml_next(ml_rd *r)
{
   while (r->p < r->end && isspace((unsigned char)*r->p)) r->p++;
   if (r->p >= r->end) return -1;
   int n = 0;
   if (*r->p == '<') {
      r->p++;
      while (r->p < r->end && *r->p != '>' && n < 500) r->tok[n++] = (char)toupper((unsigned char)*r->p++);
      if (r->p < r->end) r->p++;
      r->kind = 1;
   } else if (*r->p == '~' && r->p + 1 < r->end) { r->tok[n++] = r->p[1]; r->p += 2; r->kind = 2; }
   else if (*r->p == '"' || *r->p == '\'') {
      htx_src src = { r->p, r->end, 0 };
      if (htx_read_string(&src, 0, "", r->tok, sizeof(r->tok)) < 0) return -2;
      r->p = src.p; r->kind = 0;
      return 0;
   } else {
      while (r->p < r->end && !isspace((unsigned char)*r->p) && *r->p != '<' && n < 500) r->tok[n++] = *r->p++;
      r->kind = 0;
   }
   r->tok[n] = 0;
   return 0;
}

int htkamd_xformset_read(const char *path, htkamd_xformset **out)
{
   if (!path || !out) { htkamd_set_error("xformset_read: bad argument"); return HTKAMD_EINVAL; }
   FILE *f = fopen(path, "rb");
   if (!f) { htkamd_set_error("xformset_read: cannot open %s", path); return HTKAMD_EIO; }
   fseek(f, 0, SEEK_END);
   const long sz = ftell(f);
   fseek(f, 0, SEEK_SET);
   char *text = (char *)malloc((size_t)sz + 1);
   if (fread(text, 1, (size_t)sz, f) != (size_t)sz) { fclose(f); free(text); htkamd_set_error("xformset_read: reading %s failed", path); return HTKAMD_EIO; }
   fclose(f);
   text[sz] = 0;
   ml_rd r = { text, text + sz, "", 0 };
   htkamd_xformset *x = NULL;
   char *name = NULL, *base = NULL;
   int rc = HTKAMD_OK, nX = -1, D = 0, nb = 0, *bsz = NULL, *classX = NULL, nClass = 0, capClass = 0, useBias = -1, cur = -1;
   float *A = NULL, *bias = NULL, *logdet = NULL;
#define ML_BAD(...) do { htkamd_set_error(__VA_ARGS__); rc = HTKAMD_EINVAL; goto done; } while (0)
#define ML_WORD(what) do { if (ml_next(&r) || r.kind != 0) ML_BAD("xformset_read: %s: %s expected", path, what); } while (0)
   for (int i = 0; i < sz; i++) if (!text[i]) ML_BAD("xformset_read: %s is a binary file: only the text form is read", path);
   if (ml_next(&r) || r.kind != 2 || r.tok[0] != 'a') ML_BAD("xformset_read: %s: ~a macro expected", path);
   ML_WORD("the transform's name");
   name = strdup(r.tok);
   while (ml_next(&r) == 0) {
      if (r.kind != 1) ML_BAD("xformset_read: %s: unexpected '%s'", path, r.tok);
      if (!strcmp(r.tok, "ADAPTKIND")) {
         ML_WORD("the adaptation kind");
         if (strcmp(r.tok, "TREE")) ML_BAD("xformset_read: %s: <ADAPTKIND> %s is not supported (only TREE)", path, r.tok);
      } else if (!strcmp(r.tok, "BASECLASS")) {
         if (ml_next(&r) || r.kind != 2 || r.tok[0] != 'b') ML_BAD("xformset_read: %s: <BASECLASS> must name a ~b macro (inline base classes are not read)", path);
         ML_WORD("the base class macro's name");
         base = strdup(r.tok);
      } else if (!strcmp(r.tok, "PARENTXFORM")) ML_BAD("xformset_read: %s: <PARENTXFORM> chains are not supported", path);
      else if (!strcmp(r.tok, "XFORMSET") || !strcmp(r.tok, "XFORMWGTSET") || !strcmp(r.tok, "OFFSET")) continue;
      else if (!strcmp(r.tok, "XFORMKIND")) {
         ML_WORD("the transform kind");
         if (strcmp(r.tok, "MLLRMEAN")) ML_BAD("xformset_read: %s: <XFORMKIND> %s is not supported (only MLLRMEAN)", path, r.tok);
      } else if (!strcmp(r.tok, "NUMXFORMS")) {
         ML_WORD("a number"); nX = atoi(r.tok);
         if (nX < 0 || nX > 100000) ML_BAD("xformset_read: %s: <NUMXFORMS> %d", path, nX);
      } else if (!strcmp(r.tok, "LINXFORM")) {
         ML_WORD("a number"); cur = atoi(r.tok) - 1;
         if (cur < 0 || cur >= nX) ML_BAD("xformset_read: %s: <LINXFORM> %d of %d", path, cur + 1, nX);
      } else if (!strcmp(r.tok, "VECSIZE")) {
         ML_WORD("a number");
         const int v = atoi(r.tok);
         if (v < 1 || (D && v != D)) ML_BAD("xformset_read: %s: <VECSIZE> %d%s", path, v, D ? " differs from the first transform's" : "");
         if (!D) { D = v; A = (float *)calloc((size_t)nX * D * D, sizeof(float)); bias = (float *)calloc((size_t)nX * D, sizeof(float)); logdet = (float *)calloc((size_t)nX, sizeof(float)); }
      } else if (!strcmp(r.tok, "BIAS")) {
         ML_WORD("a number");
         if (cur < 0 || !D || atoi(r.tok) != D) ML_BAD("xformset_read: %s: <BIAS> %s in a transform of size %d", path, r.tok, D);
         if (useBias == 0) ML_BAD("xformset_read: %s: some transforms have a bias and some have none", path);
         useBias = 1;
         for (int i = 0; i < D; i++) { ML_WORD("a bias value"); bias[(size_t)cur * D + i] = strtof(r.tok, NULL); }
      } else if (!strcmp(r.tok, "LOGDET")) {
         ML_WORD("a number"); if (cur >= 0 && logdet) logdet[cur] = strtof(r.tok, NULL);
      } else if (!strcmp(r.tok, "BLOCKINFO")) {
         ML_WORD("a number");
         const int n = atoi(r.tok);
         if (cur < 0 || !D || n < 1 || n > D || (bsz && n != nb)) ML_BAD("xformset_read: %s: <BLOCKINFO> %d", path, n);
         const int first = !bsz;
         if (first) { nb = n; bsz = (int *)calloc((size_t)n, sizeof(int)); }
         for (int b = 0; b < n; b++) {
            ML_WORD("a block size");
            const int v = atoi(r.tok);
            if (first) bsz[b] = v; else if (bsz[b] != v) ML_BAD("xformset_read: %s: transform %d has other blocks than the first", path, cur + 1);
            if (v < 1 || v > HTKAMD_MLLR_MAXBLOCK) ML_BAD("xformset_read: %s: <BLOCKINFO>: a block of size %d (1 .. %d)", path, v, HTKAMD_MLLR_MAXBLOCK);
         }
         if (useBias < 0) useBias = 0;                      /* <OFFSET> <BIAS> stands before <BLOCKINFO>: this transform has none */
      } else if (!strcmp(r.tok, "BLOCK")) {
         ML_WORD("a number");
         const int b = atoi(r.tok) - 1;
         if (cur < 0 || !bsz || b < 0 || b >= nb) ML_BAD("xformset_read: %s: <BLOCK> %d", path, b + 1);
         if (ml_next(&r) || r.kind != 1 || strcmp(r.tok, "XFORM")) ML_BAD("xformset_read: %s: <XFORM> expected behind <BLOCK> (~x references are not read)", path);
         ML_WORD("a number"); const int nr = atoi(r.tok);
         ML_WORD("a number"); const int nc = atoi(r.tok);
         int c0 = 0, sum = 0;
         for (int q = 0; q < nb; q++) { if (q < b) c0 += bsz[q]; sum += bsz[q]; }
         if (nr != bsz[b] || nc != bsz[b] || sum != D) ML_BAD("xformset_read: %s: <XFORM> %d %d in block %d of size %d (vector size %d)", path, nr, nc, b + 1, bsz[b], D);
         for (int i = 0; i < nr; i++) for (int j = 0; j < nc; j++) { ML_WORD("a matrix value"); A[((size_t)cur * D + c0 + i) * D + c0 + j] = strtof(r.tok, NULL); }
      } else if (!strcmp(r.tok, "CLASSXFORM")) {
         ML_WORD("a number"); const int c = atoi(r.tok);
         ML_WORD("a number"); const int k = atoi(r.tok);
         if (c != nClass + 1 || k < 0 || k > nX) ML_BAD("xformset_read: %s: <CLASSXFORM> %d %d", path, c, k);
         if (nClass + 1 > capClass) { capClass = capClass * 2 + 16; classX = (int *)realloc(classX, sizeof(int) * (size_t)capClass); }
         classX[nClass++] = k;
      } else ML_BAD("xformset_read: %s: <%s> is not supported in a transform file", path, r.tok);
   }
   if (nX < 0 || nClass < 1 || !base) ML_BAD("xformset_read: %s: not a transform set (<NUMXFORMS>, <BASECLASS> and <CLASSXFORM> are needed)", path);
   if (nX > 0 && (!D || !bsz)) ML_BAD("xformset_read: %s: %d transforms announced, none defined", path, nX);
   if (nX == 0) { int one = 1; x = ml_new(1, 1, &one, 0, 0, nClass); }
   else {
      x = ml_new(D, nb, bsz, useBias == 1, nX, nClass);
      memcpy(x->A, A, sizeof(float) * (size_t)nX * D * D); memcpy(x->bias, bias, sizeof(float) * (size_t)nX * D); memcpy(x->logdet, logdet, sizeof(float) * (size_t)nX);
   }
   memcpy(x->classX, classX, sizeof(int) * (size_t)nClass);
   x->name = name; x->baseName = base; name = base = NULL;
   *out = x;
done:
#undef ML_BAD
#undef ML_WORD
   free(text); free(name); free(base); free(bsz); free(classX); free(A); free(bias); free(logdet);
   return rc;
}

/* ------------------------------------------------------------------------------------------ the estimate */
typedef struct {
   int G, D, nNodes; const float *mean, *var; const double *occ, *spSum; const int *cls; const int *left, *right;      /* 1-based tree and classes */
   const htkamd_mllr_config *cfg;
} ml_tables;
typedef struct { double *stats; size_t statsCap; double *nodeOcc; int *nX, *xNode, *classX; float *A, *bias; double *W; int *badNode, *badRow; float *ms; } ml_outs;

/* the device steps over tables: statistics and tree sums, the choice of the nodes, the solves.  HTKAMD_OK, HTKAMD_MLLR_NOSET, or an error */
static int ml_run(const char *who, const ml_tables *T, const ml_outs *O, void *stream)
{
   int nb, one; const int *bsz;
   int rc = ml_blocks(who, T->cfg, T->D, &nb, &bsz, &one);
   if (rc) return rc;
   const int G = T->G, D = T->D, nNodes = T->nNodes;
   if (G < 1 || nNodes < 1) { htkamd_set_error("%s: %d Gaussians, %d nodes", who, G, nNodes); return HTKAMD_EINVAL; }
   int nX = 0, *xNode = (int *)malloc(sizeof(int) * (size_t)nNodes), *termClass = (int *)malloc(sizeof(int) * (size_t)nNodes), nClass = 0;
   int *l0 = (int *)malloc(sizeof(int) * (size_t)nNodes), *r0 = (int *)malloc(sizeof(int) * (size_t)nNodes), *inner = (int *)malloc(sizeof(int) * (size_t)nNodes), nInner = 0;
   int *classX = NULL, *memOff = NULL, *mem = NULL, *fill = NULL;
   float *occF = NULL, *spF = NULL;
   double *nodeOcc = (double *)calloc((size_t)nNodes, sizeof(double));
   htkamd_mllr_dev *dev = NULL;
   for (int i = 0; i < nNodes; i++) {
      const int l = T->left[i], r = T->right[i];
      if ((l == 0) != (r == 0) || l < 0 || r < 0 || l > nNodes || r > nNodes || (l && (l <= i + 1 || r <= i + 1 || l == r))) {
         htkamd_set_error("%s: node %d has the children %d, %d (children are numbered behind their parent)", who, i + 1, l, r); rc = HTKAMD_EINVAL; goto done;
      }
      l0[i] = l - 1; r0[i] = r - 1; termClass[i] = l ? -1 : nClass++;
   }
   for (int i = nNodes - 1; i >= 0; i--) if (T->left[i]) inner[nInner++] = i;      /* children carry higher numbers: descending order is bottom-up */
   classX = (int *)calloc((size_t)nClass, sizeof(int)); memOff = (int *)calloc((size_t)nClass + 2, sizeof(int));
   for (int g = 0; g < G; g++) {
      if (T->cls[g] < 0 || T->cls[g] > nClass) { htkamd_set_error("%s: Gaussian %d is in class %d of %d", who, g, T->cls[g], nClass); rc = HTKAMD_EINVAL; goto done; }
      if (T->cls[g]) memOff[T->cls[g]]++;
   }
   for (int c = 0; c < nClass; c++) memOff[c + 1] += memOff[c];
   mem = (int *)malloc(sizeof(int) * (size_t)(memOff[nClass] ? memOff[nClass] : 1)); fill = (int *)malloc(sizeof(int) * (size_t)nClass);
   memcpy(fill, memOff, sizeof(int) * (size_t)nClass);
   for (int g = 0; g < G; g++) if (T->cls[g]) mem[fill[T->cls[g] - 1]++] = g;       /* a class's members in the set's order */
   occF = (float *)malloc(sizeof(float) * (size_t)G); spF = (float *)malloc(sizeof(float) * (size_t)G * D);
   for (int g = 0; g < G; g++) occF[g] = (float)T->occ[g];
   for (size_t e = 0; e < (size_t)G * D; e++) spF[e] = (float)T->spSum[e];
   if (!htkamd_mllr_dev_stats) { htkamd_set_error("%s: no HIP device: this build holds the host files only", who); rc = HTKAMD_ENODEV; goto done; }
   {
      htkamd_mllr_job job = { G, D, nb, T->cfg ? T->cfg->useBias != 0 : 1, nClass, nNodes, nInner, bsz, T->mean, T->var, occF, spF,
                              T->cfg ? T->cfg->minOccThresh : 0.0f, memOff, mem, l0, r0, termClass, inner };
      if ((rc = htkamd_mllr_dev_stats(&job, &dev, nodeOcc, stream))) goto done;
   }
   if (O->nodeOcc) memcpy(O->nodeOcc, nodeOcc, sizeof(double) * (size_t)nNodes);
   if (O->stats) {
      const size_t need = (size_t)nNodes * htkamd_mllr_record_len(D, nb, bsz);
      if (O->statsCap < need) { htkamd_set_error("%s: the statistics take %zu doubles, %zu are offered", who, need, O->statsCap); rc = HTKAMD_EINVAL; goto done; }
      if ((rc = htkamd_mllr_dev_fetch(dev, O->stats))) goto done;
   }
   rc = htkamd_mllr_select(nNodes, T->left, T->right, nodeOcc, ml_thresh(T->cfg), &nX, xNode, classX);
   if (O->nX) *O->nX = nX;
   if (O->classX) memcpy(O->classX, classX, sizeof(int) * (size_t)nClass);
   if (O->xNode) memcpy(O->xNode, xNode, sizeof(int) * (size_t)nX);
   if (rc == HTKAMD_OK) {
      int badX = -1, badRow = -1;
      for (int k = 0; k < nX; k++) xNode[k]--;
      rc = htkamd_mllr_dev_solve(dev, nX, xNode, O->A, O->bias, O->W, &badX, &badRow);
      if (rc == HTKAMD_ERANGE) {
         if (O->badNode) *O->badNode = xNode[badX] + 1;
         if (O->badRow) *O->badRow = badRow + 1;
         htkamd_set_error("%s: node %d, row %d: the matrix G of the row is not positive definite (a pivot is zero, negative or below 1e-12 of its diagonal entry): "
                          "the node's Gaussians have too few distinct means for a transform of this block size; nothing is installed", who, xNode[badX] + 1, badRow + 1);
      }
   }
   if (O->ms) htkamd_mllr_dev_times(dev, O->ms);
done:
   if (dev) htkamd_mllr_dev_close(dev);
   free(xNode); free(termClass); free(l0); free(r0); free(inner); free(classX); free(memOff); free(mem); free(fill); free(occF); free(spF); free(nodeOcc);
   return rc;
}

int htkamd_mllr_probe(const float *mean, const float *var, const double *occ, const double *spSum, const int *cls, int G, int D, int nNodes, const int *left,
                      const int *right, const htkamd_mllr_config *cfg, double *stats, size_t statsCap, double *nodeOcc, int *nX, int *xNode, int *classX,
                      float *A, float *bias, double *W, int *badNode, int *badRow, float *ms, void *stream)
{
   if (!mean || !var || !occ || !spSum || !cls || !left || !right || !nX || !xNode || !classX || !A || !bias) { htkamd_set_error("mllr_probe: bad argument"); return HTKAMD_EINVAL; }
   const ml_tables T = { G, D, nNodes, mean, var, occ, spSum, cls, left, right, cfg };
   const ml_outs O = { stats, statsCap, nodeOcc, nX, xNode, classX, A, bias, W, badNode, badRow, ms };
   return ml_run("mllr_probe", &T, &O, stream);
}

int htkamd_mllr_estimate(htkamd_mmf *s, htkamd_model *m, htkamd_accs *a, const htkamd_regtree *t, const htkamd_mllr_config *cfg, htkamd_xformset **out, void *stream)
{
   int *cls = NULL;
   int rc = ml_check("mllr_estimate", s, t, cfg, &cls);      /* every refusal, before a device is looked for */
   if (rc) return rc;
   if (!m || !a || !out) { free(cls); htkamd_set_error("mllr_estimate: bad argument"); return HTKAMD_EINVAL; }
   if (!htkamd_accs_download || !htkamd_accs_get_layout || !htkamd_model_get_params) { free(cls); htkamd_set_error("mllr_estimate: no HIP device: this build holds the host files only"); return HTKAMD_ENODEV; }
   htkamd_accs_layout lay;
   if ((rc = htkamd_accs_get_layout(a, &lay))) { free(cls); return rc; }
   const int G = s->nG, D = s->vecSize, nNodes = htkamd_regtree_num_nodes(t);
   const int nClass = htkamd_regtree_num_terminals(t);
   int mD = 0, mG = 0, adapted = 0;
   if (htkamd_mllr_model_state && !(rc = htkamd_mllr_model_state("mllr_estimate", m, &mD, &mG, &adapted))) {
      if (mD != D || mG != G) { htkamd_set_error("mllr_estimate: the model has %d Gaussians of size %d, the set %d of size %d", mG, mD, G, D); rc = HTKAMD_EINVAL; }
      else if (adapted) { htkamd_set_error("mllr_estimate: the model is adapted (htkamd_mllr_restore first): transforms on top of a parent transform are not supported"); rc = HTKAMD_EINVAL; }
   }
   if (rc) { free(cls); return rc; }
   double *vec = (double *)malloc(sizeof(double) * lay.total), *sp = (double *)malloc(sizeof(double) * (size_t)G * D);
   float *mean = (float *)malloc(sizeof(float) * (size_t)G * D), *var = (float *)malloc(sizeof(float) * (size_t)G * D);
   int *left = (int *)malloc(sizeof(int) * (size_t)nNodes), *right = (int *)malloc(sizeof(int) * (size_t)nNodes), *xNode = (int *)malloc(sizeof(int) * (size_t)nNodes);
   htkamd_xformset *x = NULL;
   int nb, one; const int *bsz;
   ml_blocks("mllr_estimate", cfg, D, &nb, &bsz, &one);
   if ((rc = htkamd_accs_download(a, vec, stream))) goto done;
   if ((rc = htkamd_model_get_params(m, mean, var, NULL, NULL, NULL))) goto done;      /* the model's own means: what the pass scored with */
   for (int g = 0; g < G; g++)
      for (int k = 0; k < D; k++) sp[(size_t)g * D + k] = vec[lay.mu + (size_t)g * D + k] + vec[lay.muOcc + g] * (double)mean[(size_t)g * D + k];
   for (int i = 0; i < nNodes; i++) htkamd_regtree_children(t, i + 1, &left[i], &right[i]);
   x = ml_new(D, nb, bsz, cfg ? cfg->useBias != 0 : 1, nNodes, nClass);
   x->nodeOcc = (double *)calloc((size_t)nNodes, sizeof(double)); x->nNodes = nNodes;
   {
      int nX = 0;
      const ml_tables T = { G, D, nNodes, mean, var, vec + lay.muOcc, sp, cls, left, right, cfg };
      const ml_outs O = { NULL, 0, x->nodeOcc, &nX, xNode, x->classX, x->A, x->bias, NULL, NULL, NULL, x->ms };
      rc = ml_run("mllr_estimate", &T, &O, stream);
      x->nX = rc == HTKAMD_OK ? nX : 0;
      if (rc == HTKAMD_OK || rc == HTKAMD_MLLR_NOSET) {
         if (rc == HTKAMD_MLLR_NOSET) memset(x->classX, 0, sizeof(int) * (size_t)nClass);
         x->xNode = xNode; xNode = NULL;
         x->G = G; x->gaussClass = cls; cls = NULL;
         x->name = strdup("mllr"); x->baseName = strdup("rtree.base");
         *out = x; x = NULL;
      }
   }
done:
   htkamd_xformset_destroy(x);
   free(vec); free(sp); free(mean); free(var); free(left); free(right); free(xNode); free(cls);
   return rc;
}

int htkamd_xformset_set_names(htkamd_xformset *x, const char *name, const char *baseName)
{
   if (!x) { htkamd_set_error("xformset_set_names: bad argument"); return HTKAMD_EINVAL; }
   if (name) { free(x->name); x->name = strdup(name); }
   if (baseName) { free(x->baseName); x->baseName = strdup(baseName); }
   return HTKAMD_OK;
}

/* ------------------------------------------------------------------------------------------ the model's means */
int htkamd_mllr_apply(htkamd_model *m, const htkamd_xformset *x, const int *gaussClass, void *stream)
{
   if (!m || !x) { htkamd_set_error("mllr_apply: bad argument"); return HTKAMD_EINVAL; }
   if (!htkamd_mllr_model_state) { htkamd_set_error("mllr_apply: no HIP device: this build holds the host files only"); return HTKAMD_ENODEV; }
   int D = 0, G = 0, adapted = 0;
   int rc = htkamd_mllr_model_state("mllr_apply", m, &D, &G, &adapted);
   if (rc) return rc;
   if (adapted) { htkamd_set_error("mllr_apply: the model is adapted already: htkamd_mllr_restore first (a second set on top is a parent transform chain, which is not supported)"); return HTKAMD_EINVAL; }
   if (x->nX < 1) { htkamd_set_error("mllr_apply: the set has no transform"); return HTKAMD_EINVAL; }
   if (x->D != D) { htkamd_set_error("mllr_apply: transforms of size %d for a model of size %d", x->D, D); return HTKAMD_EINVAL; }
   const int *cls = gaussClass ? gaussClass : x->gaussClass;
   if (!cls || (!gaussClass && x->G != G)) { htkamd_set_error("mllr_apply: the base class of every Gaussian is needed (htkamd_mllr_gauss_classes) for a set that was not estimated on this model set"); return HTKAMD_EINVAL; }
   int *gx = (int *)malloc(sizeof(int) * (size_t)G), *c0 = (int *)malloc(sizeof(int) * (size_t)D), *bs = (int *)malloc(sizeof(int) * (size_t)D);
   for (int g = 0; g < G && !rc; g++) {
      if (cls[g] < 0 || cls[g] > x->nClass) { htkamd_set_error("mllr_apply: Gaussian %d is in class %d of %d", g, cls[g], x->nClass); rc = HTKAMD_EINVAL; }
      else gx[g] = cls[g] ? x->classX[cls[g] - 1] - 1 : -1;
   }
   for (int b = 0, o = 0; b < x->nBlocks; o += x->blockSize[b], b++) for (int i = o; i < o + x->blockSize[b]; i++) { c0[i] = o; bs[i] = x->blockSize[b]; }
   if (!rc) rc = htkamd_mllr_dev_apply(m, x->nX, x->A, x->useBias ? x->bias : NULL, gx, c0, bs, stream);
   free(gx); free(c0); free(bs);
   return rc;
}

int htkamd_mllr_restore(htkamd_model *m, void *stream)
{
   if (!m) { htkamd_set_error("mllr_restore: bad argument"); return HTKAMD_EINVAL; }
   if (!htkamd_mllr_model_state) { htkamd_set_error("mllr_restore: no HIP device: this build holds the host files only"); return HTKAMD_ENODEV; }
   int adapted = 0;
   const int rc = htkamd_mllr_model_state("mllr_restore", m, NULL, NULL, &adapted);
   if (rc) return rc;
   if (!adapted) { htkamd_set_error("mllr_restore: the model is not adapted"); return HTKAMD_EINVAL; }
   return htkamd_mllr_dev_restore(m, stream);
}
