/* vqtab.c -- the VQ table of HTKLib/HVQ.c on the host: made from cluster sets as HQuant numbers the nodes (AddLinEntries HQuant.c:316,
 * AddBinEntries :335), read as LoadVQTab (:244) reads it and written as StoreVQTab (:330) writes it, byte for byte.
 *
 * A stream's nodes are kept in ONE order, the one StoreTree (:308) writes and GetVQ (:459) walks: the node, its left subtree, its right
 * subtree.  For a linear table that is the list (every node's right link is the next one); HQuant's list starts at the LAST cluster
 * (AddLinEntries links every new node in front), so a table of K clusters holds vqidx K, K-1, .. 1.  The ids of the file are MarkTree's
 * (:291): position + 1, whatever ids the file read had.  gconst: CreateVQNode (:134-140), in the reference's types.
 * The covariance of a FULLC cluster is inverted here too (CovInvert HMath.c:567) for csrc/vquant.hip. */
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../csrc/vquant.h"
#include "htktext.h"

static int tab_cov_len(int D, int kind) { return kind == HTKAMD_CK_NULLC ? 0 : kind == HTKAMD_CK_FULLC ? D * (D + 1) / 2 : D; }

/* Choleski (HMath.c:514) of a packed lower triangle into L [D][D]; 0: not positive definite */
static int choleski(int D, const float *tri, double *L)
{
   int i, j, k;
   for (i = 0; i < D; i++)
      for (j = 0; j <= i; j++) {
         double sum = tri[(size_t)i * (i + 1) / 2 + j];
         for (k = 0; k < j; k++) sum -= L[(size_t)i * D + k] * L[(size_t)j * D + k];
         if (i == j && sum <= 0.0) return 0;
         else if (i == j) sum = sqrt(sum);
         else if (L[(size_t)j * D + j] == 0.0) return 0;
         else sum /= L[(size_t)j * D + j];
         L[(size_t)i * D + j] = sum;
      }
   return 1;
}

int htkamd_host_cov_invert(int D, const float *tri, float *inv)
{
   double *L = (double *)malloc(sizeof(double) * ((size_t)D * D + 2 * (size_t)D)), *x, *y;
   int i, j, k;
   if (!L) return -1;
   x = L + (size_t)D * D; y = x + D;
   if (!choleski(D, tri, L)) { free(L); return -1; }
   for (i = 0; i < D; i++) {                               /* MSolve (:542): L y = e_i, then L' x = y */
      for (j = 0; j < i; j++) y[j] = 0.0;
      y[i] = 1.0 / L[(size_t)i * D + i];
      for (j = i + 1; j < D; j++) {
         double sum = 0.0;
         for (k = i; k < j; k++) sum -= L[(size_t)j * D + k] * y[k];
         y[j] = sum / L[(size_t)j * D + j];
      }
      x[D - 1] = y[D - 1] / L[(size_t)(D - 1) * D + D - 1];
      for (j = D - 2; j >= 0; j--) {
         double sum = y[j];
         for (k = j + 1; k < D; k++) sum -= L[(size_t)k * D + j] * x[k];
         x[j] = sum / L[(size_t)j * D + j];
      }
      for (j = i; j < D; j++) inv[(size_t)j * (j + 1) / 2 + i] = (float)x[j];      /* column i of the full inverse; Mat2Tri keeps the lower triangle */
   }
   free(L);
   return 0;
}

int htkamd_vq_cov_invert(int D, const float *tri, float *inv)
{
   if (D < 1 || !tri || !inv) { htkamd_set_error("vq_cov_invert: bad argument"); return HTKAMD_EINVAL; }
   if (htkamd_host_cov_invert(D, tri, inv) != 0) { htkamd_set_error("vq_cov_invert: CovInvert: [%f ...] not invertible", tri[0]); return HTKAMD_VQ_EINVERT; }
   return HTKAMD_OK;
}

/* CreateVQNode's gconst; -1: a FULLC inverse that is not positive definite (CovDet's 5220) */
static int node_gconst(int kind, int D, const float *cov, float *out)
{
   if (kind == HTKAMD_CK_NULLC) *out = 0.0f;
   else if (kind == HTKAMD_CK_INVDIAGC) {                 /* InvDiagGConst (:105): a float sum, the logarithms in double */
      float sum = D * log(HTK_TPI);
      int i;
      for (i = 0; i < D; i++) sum -= log(cov[i]);
      *out = sum;
   } else return htkamd_host_fix_full_gconst(D, cov, out);      /* FullInvGConst (:117) = n log(2 pi) - CovDet(ic), FixFullGConst's sum */
   return 0;
}

static void stream_free(vq_stream *v)
{
   free(v->vqidx); free(v->left); free(v->right); free(v->gconst); free(v->mean); free(v->cov);
   memset(v, 0, sizeof(*v));
}

static int stream_alloc(vq_stream *v, int n, int width, int covLen)
{
   v->n = n; v->width = width; v->covLen = covLen;
   v->vqidx = (int *)malloc(sizeof(int) * (size_t)n); v->left = (int *)malloc(sizeof(int) * (size_t)n); v->right = (int *)malloc(sizeof(int) * (size_t)n);
   v->gconst = (float *)malloc(sizeof(float) * (size_t)n); v->mean = (float *)malloc(sizeof(float) * (size_t)n * width);
   v->cov = (float *)malloc(sizeof(float) * ((size_t)n * covLen + 1));
   if (v->vqidx && v->left && v->right && v->gconst && v->mean && v->cov) return HTKAMD_OK;
   htkamd_set_error("vqtab: out of memory");
   return HTKAMD_ENOMEM;
}

void htkamd_vqtab_destroy(htkamd_vqtab *t)
{
   int s;
   if (!t) return;
   if (t->dev && t->devFree) t->devFree(t->dev);
   for (s = 0; s < VQ_SMAX; s++) stream_free(&t->st[s]);
   free(t);
}

static int kind_check(int kind, const char *who)
{
   if (kind == HTKAMD_CK_NULLC || kind == HTKAMD_CK_INVDIAGC || kind == HTKAMD_CK_FULLC) return HTKAMD_OK;
   if (kind == HTKAMD_CK_DIAGC) htkamd_set_error("%s: CKCheck: bad covkind %d: a VQ table holds no DIAGC covariances (NULLC, INVDIAGC or FULLC)", who, kind);
   else htkamd_set_error("%s: CKCheck: bad covkind %d", who, kind);
   return HTKAMD_VQ_ETABKIND;
}

/* AddBinEntries: heap node nid (from 1) of numClust nodes into position *pos, its subtrees behind it; returns the position */
static int add_bin(vq_stream *v, int nid, int numClust, int *pos, int *heapOf)
{
   int p;
   if (nid > numClust) return -1;
   p = (*pos)++;
   heapOf[p] = nid - 1;
   v->vqidx[p] = nid > numClust / 2 ? nid - numClust / 2 : 0;
   v->left[p] = add_bin(v, 2 * nid, numClust, pos, heapOf);
   v->right[p] = add_bin(v, 2 * nid + 1, numClust, pos, heapOf);
   return p;
}

int htkamd_vqtab_from_clusters(int magic, int type, int kind, int nStreams, const int *width, const htkamd_vq_clusters *cs, const float *const *globalCov,
                               htkamd_vqtab **out)
{
   htkamd_vqtab *t;
   int s, rc, total = 0;
   if (!out || !width || !cs || nStreams < 1) { htkamd_set_error("vqtab_from_clusters: bad argument"); return HTKAMD_EINVAL; }
   *out = NULL;
   if (nStreams > VQ_SMAX) { htkamd_set_error("vqtab_from_clusters: %d streams (at most %d)", nStreams, VQ_SMAX); return HTKAMD_EINVAL; }
   if (type != HTKAMD_VQ_LINTREE && type != HTKAMD_VQ_BINTREE) { htkamd_set_error("vqtab_from_clusters: tree type %d", type); return HTKAMD_EINVAL; }
   if ((rc = kind_check(kind, "vqtab_from_clusters"))) return rc;
   t = (htkamd_vqtab *)calloc(1, sizeof(*t));
   if (!t) { htkamd_set_error("vqtab: out of memory"); return HTKAMD_ENOMEM; }
   t->magic = magic; t->type = type; t->kind = kind; t->nStreams = nStreams;
   for (s = 0; s < nStreams; s++) {
      const htkamd_vq_clusters *c = &cs[s];
      const int K = c->numNodes, D = width[s], L = tab_cov_len(D, kind);
      vq_stream *v = &t->st[s];
      int *heapOf, p, pos = 0;
      if (K < 1 || D < 1 || !c->centre || (L > 0 && !c->cov && !(globalCov && globalCov[s])) || (type == HTKAMD_VQ_BINTREE && K % 2 == 0)) {
         htkamd_set_error("vqtab_from_clusters: stream %d: a cluster set of %d nodes, width %d", s + 1, K, D); htkamd_vqtab_destroy(t); return HTKAMD_EINVAL;
      }
      total += K;
      if (total > VQ_MAXNODES) { htkamd_set_error("vqtab_from_clusters: more than %d nodes", VQ_MAXNODES); htkamd_vqtab_destroy(t); return HTKAMD_EINVAL; }
      if ((rc = stream_alloc(v, K, D, L))) { htkamd_vqtab_destroy(t); return rc; }
      heapOf = (int *)malloc(sizeof(int) * (size_t)K);
      if (!heapOf) { htkamd_set_error("vqtab: out of memory"); htkamd_vqtab_destroy(t); return HTKAMD_ENOMEM; }
      if (type == HTKAMD_VQ_BINTREE) add_bin(v, 1, K, &pos, heapOf);
      else for (p = 0; p < K; p++) { heapOf[p] = K - 1 - p; v->vqidx[p] = K - p; v->left[p] = -1; v->right[p] = p + 1 < K ? p + 1 : -1; }
      for (p = 0; p < K; p++) {
         const int h = heapOf[p];
         const float *cov = L == 0 ? NULL : (globalCov && globalCov[s]) ? globalCov[s] : c->cov + (size_t)h * L;
         memcpy(v->mean + (size_t)p * D, c->centre + (size_t)h * D, sizeof(float) * (size_t)D);
         if (L > 0) memcpy(v->cov + (size_t)p * L, cov, sizeof(float) * (size_t)L);
         if (node_gconst(kind, D, cov, &v->gconst[p]) != 0) {
            htkamd_set_error("vqtab_from_clusters: stream %d, cluster %d: CovDet: [%f ...] not invertible", s + 1, h + 1, cov[0]);
            free(heapOf); htkamd_vqtab_destroy(t); return HTKAMD_VQ_EINVERT;
         }
      }
      free(heapOf);
   }
   *out = t;
   return HTKAMD_OK;
}

/* ---- the file ---- */
static void put_floats(FILE *f, const float *x, int n) { int i; for (i = 0; i < n; i++) fprintf(f, " %e", x[i]); }

int htkamd_vqtab_write(const htkamd_vqtab *t, const char *path)
{
   FILE *f;
   int s, p, i, j, total = 0;
   if (!t || !path) { htkamd_set_error("vqtab_write: bad argument"); return HTKAMD_EINVAL; }
   f = fopen(path, "w");
   if (!f) { htkamd_set_error("vqtab_write: StoreVQTab: cannot create file %s", path); return HTKAMD_EIO; }
   for (s = 0; s < t->nStreams; s++) total += t->st[s].n;
   fprintf(f, "%d %d %d %d %d ", t->magic, t->type, t->kind, total, t->nStreams);
   for (s = 0; s < t->nStreams; s++) fprintf(f, "%d ", t->st[s].width);
   fprintf(f, "\n");
   for (s = 0; s < t->nStreams; s++) {
      const vq_stream *v = &t->st[s];
      const int D = v->width;
      for (p = 0; p < v->n; p++) {
         fprintf(f, "%d %d %d %d %d\n", s + 1, v->vqidx[p], p + 1, v->left[p] + 1, v->right[p] + 1);
         put_floats(f, v->mean + (size_t)p * D, D); fputc('\n', f);
         if (t->kind == HTKAMD_CK_INVDIAGC) { put_floats(f, v->cov + (size_t)p * D, D); fputc('\n', f); }
         else if (t->kind == HTKAMD_CK_FULLC) {            /* WriteTriMat (HMath.c:431): column j from the diagonal down */
            const float *m = v->cov + (size_t)p * v->covLen;
            for (j = 0; j < D; j++) {
               for (i = j; i < D; i++) fprintf(f, " %e", m[(size_t)i * (i + 1) / 2 + j]);
               fputc('\n', f);
            }
         }
         fprintf(f, "\n");
      }
   }
   if (fclose(f) != 0) { htkamd_set_error("vqtab_write: %s: write error", path); return HTKAMD_EIO; }
   return HTKAMD_OK;
}

typedef struct { htx_src src; const char *path; } vq_reader;

static int get_int(vq_reader *r, long lo, long hi, const char *item, int *out)
{
   char *end;
   long x;
   while (r->src.p < r->src.end && (*r->src.p == ' ' || *r->src.p == '\t' || *r->src.p == '\n' || *r->src.p == '\r')) r->src.p++;
   errno = 0;
   x = strtol(r->src.p, &end, 10);
   if (end == r->src.p || r->src.p >= r->src.end) { htkamd_set_error("vqtab_read: %s: GetVal: cant read %s", r->path, item); return HTKAMD_EIO; }
   r->src.p = end;
   if (!(lo == 0 && hi == 0) && (x < lo || x > hi)) { htkamd_set_error("vqtab_read: %s: GetVal: %s out of range (%ld)", r->path, item, x); return HTKAMD_EIO; }
   *out = (int)x;
   return HTKAMD_OK;
}

static int get_floats(vq_reader *r, float *x, int n, const char *item)
{
   int i;
   for (i = 0; i < n; i++) {
      char *end;
      while (r->src.p < r->src.end && (*r->src.p == ' ' || *r->src.p == '\t' || *r->src.p == '\n' || *r->src.p == '\r')) r->src.p++;
      x[i] = strtof(r->src.p, &end);
      if (end == r->src.p || r->src.p >= r->src.end) { htkamd_set_error("vqtab_read: %s: GetNode: cannot read %s", r->path, item); return HTKAMD_EIO; }
      r->src.p = end;
   }
   return HTKAMD_OK;
}

/* one entry of the file as LoadVQTab keeps it before SortEntries */
typedef struct { int stream, vqidx, nid, lid, rid, used; float *mean, *cov; } vq_entry;

static int find_entry(vq_entry *e, int n, int stream, int nid)
{
   int i;
   for (i = n - 1; i >= 0; i--)                            /* the list is built front first: the last entry read is found first */
      if (e[i].stream == stream && !e[i].used && e[i].nid == nid) { e[i].used = 1; return i; }
   return -1;
}

int htkamd_vqtab_read(const char *path, int magic, htkamd_vqtab **out)
{
   htkamd_vqtab *t = NULL;
   vq_entry *ent = NULL;
   char *text;
   size_t len;
   vq_reader r;
   int why, rc, fmagic, type, kind, numNodes = 0, nS, width[VQ_SMAX], s, i;
   int *stack = NULL, *parent = NULL;
   if (!path || !out) { htkamd_set_error("vqtab_read: bad argument"); return HTKAMD_EINVAL; }
   *out = NULL;
   text = htx_read_file(path, &len, &why);
   if (!text) {
      if (why == HTX_ENOMEM) { htkamd_set_error("vqtab_read: out of memory"); return HTKAMD_ENOMEM; }
      htkamd_set_error("vqtab_read: LoadVQTab: Can't open file %s", path); return HTKAMD_EIO;
   }
   r.src.p = text; r.src.end = text + len; r.src.wasQuoted = 0; r.path = path;
   if ((rc = get_int(&r, 0, 0, "magic number", &fmagic))) goto done;
   if (magic != 0 && magic != fmagic) { htkamd_set_error("vqtab_read: LoadVQTab: %s has magic=%d but reqd magic=%d", path, fmagic, magic); rc = HTKAMD_EINVAL; goto done; }
   if ((rc = get_int(&r, HTKAMD_VQ_LINTREE, HTKAMD_VQ_BINTREE, "tree type", &type)) || (rc = get_int(&r, HTKAMD_CK_DIAGC, HTKAMD_CK_NULLC, "cov kind", &kind))) goto done;
   if ((rc = kind_check(kind, "vqtab_read"))) goto done;
   if ((rc = get_int(&r, 1, VQ_MAXNODES, "number of nodes", &numNodes)) || (rc = get_int(&r, 1, VQ_SMAX, "number of streams", &nS))) goto done;
   for (s = 0; s < nS; s++) if ((rc = get_int(&r, 1, 10000, "stream width", &width[s]))) goto done;
   ent = (vq_entry *)calloc((size_t)numNodes, sizeof(*ent));
   stack = (int *)malloc(sizeof(int) * 2 * ((size_t)numNodes + 1));
   t = (htkamd_vqtab *)calloc(1, sizeof(*t));
   if (!ent || !stack || !t) { htkamd_set_error("vqtab_read: out of memory"); rc = HTKAMD_ENOMEM; goto done; }
   parent = stack + numNodes + 1;
   t->magic = fmagic; t->type = type; t->kind = kind; t->nStreams = nS;
   for (i = 0; i < numNodes; i++) {
      vq_entry *e = &ent[i];
      int D, L;
      if ((rc = get_int(&r, 1, nS, "stream index", &e->stream)) || (rc = get_int(&r, 0, 0, "VQ Index", &e->vqidx)) || (rc = get_int(&r, 0, 0, "Node Id", &e->nid)) ||
          (rc = get_int(&r, 0, 0, "Left Id", &e->lid)) || (rc = get_int(&r, 0, 0, "Right Id", &e->rid)))
         goto done;
      D = width[e->stream - 1]; L = tab_cov_len(D, kind);
      e->mean = (float *)malloc(sizeof(float) * ((size_t)D + L + 1));
      if (!e->mean) { htkamd_set_error("vqtab_read: out of memory"); rc = HTKAMD_ENOMEM; goto done; }
      e->cov = e->mean + D;
      if ((rc = get_floats(&r, e->mean, D, "mean vector"))) goto done;
      if (kind == HTKAMD_CK_INVDIAGC) rc = get_floats(&r, e->cov, D, "variance vector");
      else if (kind == HTKAMD_CK_FULLC) {                 /* ReadTriMat (HMath.c:406): column j from the diagonal down */
         int a, b;
         for (b = 0; b < D && !rc; b++) for (a = b; a < D && !rc; a++) rc = get_floats(&r, e->cov + (size_t)a * (a + 1) / 2 + b, 1, "covariance matrix");
      }
      if (rc) goto done;
   }
   for (s = 0; s < nS; s++) {                              /* SortEntries (:225) from node 1: the node, its left subtree, its right subtree */
      vq_stream *v = &t->st[s];
      const int D = width[s], L = tab_cov_len(D, kind);
      int n = 0, sp = 0, pos = 0;
      for (i = 0; i < numNodes; i++) if (ent[i].stream == s + 1) n++;
      if (n == 0) { htkamd_set_error("vqtab_read: %s: SortEntries: cannot find node 1 (stream %d)", path, s + 1); rc = HTKAMD_EIO; goto done; }
      if ((rc = stream_alloc(v, n, D, L))) goto done;
      stack[sp] = 1; parent[sp++] = -1;                    /* parent: position * 2 + (1 for the right link), -1 the root */
      while (sp > 0) {
         const int nid = stack[--sp], par = parent[sp];
         const int k = find_entry(ent, numNodes, s + 1, nid);
         if (k < 0 || pos >= n) { htkamd_set_error("vqtab_read: %s: SortEntries: cannot find node %d (stream %d)", path, nid, s + 1); rc = HTKAMD_EIO; goto done; }
         v->vqidx[pos] = ent[k].vqidx; v->left[pos] = -1; v->right[pos] = -1;
         memcpy(v->mean + (size_t)pos * D, ent[k].mean, sizeof(float) * (size_t)D);
         if (L > 0) memcpy(v->cov + (size_t)pos * L, ent[k].cov, sizeof(float) * (size_t)L);
         if (node_gconst(kind, D, ent[k].cov, &v->gconst[pos]) != 0) {
            htkamd_set_error("vqtab_read: %s: CovDet: [%f ...] not invertible (stream %d, node %d)", path, ent[k].cov[0], s + 1, nid); rc = HTKAMD_VQ_EINVERT; goto done;
         }
         if (par >= 0) { if (par & 1) v->right[par >> 1] = pos; else v->left[par >> 1] = pos; }
         if (ent[k].rid != 0) { stack[sp] = ent[k].rid; parent[sp++] = pos * 2 + 1; }      /* the left subtree first: it is pushed last */
         if (ent[k].lid != 0) { stack[sp] = ent[k].lid; parent[sp++] = pos * 2; }
         pos++;
      }
      v->n = pos;                                          /* (entries that no link reaches are dropped, as SortEntries drops them) */
      if (type == HTKAMD_VQ_BINTREE)
         for (i = 0; i < pos; i++)
            if ((v->left[i] < 0) != (v->right[i] < 0)) { htkamd_set_error("vqtab_read: %s: a tree node of stream %d has one child", path, s + 1); rc = HTKAMD_EIO; goto done; }
   }
   rc = HTKAMD_OK;
done:
   if (ent) { for (i = 0; i < numNodes; i++) free(ent[i].mean); free(ent); }
   free(stack);
   free(text);
   if (rc) { htkamd_vqtab_destroy(t); return rc; }
   *out = t;
   return HTKAMD_OK;
}

int htkamd_vqtab_info(const htkamd_vqtab *t, int *info, int *width)
{
   int s, total = 0;
   if (!t) { htkamd_set_error("vqtab_info: bad argument"); return HTKAMD_EINVAL; }
   for (s = 0; s < t->nStreams; s++) { total += t->st[s].n; if (width) width[s] = t->st[s].width; }
   if (info) { info[0] = t->magic; info[1] = t->type; info[2] = t->kind; info[3] = total; info[4] = t->nStreams; }
   return HTKAMD_OK;
}

int htkamd_vqtab_stream(const htkamd_vqtab *t, int s, int *vqidx, int *left, int *right, float *gconst, float *mean, float *cov)
{
   const vq_stream *v;
   if (!t || s < 0 || s >= t->nStreams) { htkamd_set_error("vqtab_stream: no stream %d", s); return HTKAMD_EINVAL; }
   v = &t->st[s];
   if (vqidx) memcpy(vqidx, v->vqidx, sizeof(int) * (size_t)v->n);
   if (left) memcpy(left, v->left, sizeof(int) * (size_t)v->n);
   if (right) memcpy(right, v->right, sizeof(int) * (size_t)v->n);
   if (gconst) memcpy(gconst, v->gconst, sizeof(float) * (size_t)v->n);
   if (mean) memcpy(mean, v->mean, sizeof(float) * (size_t)v->n * v->width);
   if (cov && v->covLen > 0) memcpy(cov, v->cov, sizeof(float) * (size_t)v->n * v->covLen);
   return v->n;
}

int htkamd_hquant_check_switch(const char *sw)
{
   if (!sw || sw[0] != '-' || !sw[1] || sw[2]) { htkamd_set_error("HQuant: Bad switch %s; must be single letter", sw ? sw : "(null)"); return HTKAMD_EINVAL; }
   if (strchr("dfgnstF", sw[1])) return HTKAMD_OK;
   if (strchr("lGILX", sw[1])) htkamd_set_error("HQuant: -%c is not supported: pools are whole parameter files here, not the segments of a label (-l with -G -I -L -X)", sw[1]);
   else if (sw[1] == 'w') htkamd_set_error("HQuant: -w (stream widths by hand) is not supported: the streams take the widths of the parameter kind");
   else if (sw[1] == 'H') htkamd_set_error("HQuant: -H is not supported: HQuant reads no HMM definitions");
   else if (strchr("ACDSTV", sw[1])) htkamd_set_error("HQuant: -%c is not supported", sw[1]);
   else htkamd_set_error("HQuant: Unknown switch %s", sw);
   return HTKAMD_EINVAL;
}
