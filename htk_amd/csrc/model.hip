// model.hip -- packed HMM set on the device, accumulator vector, error plumbing.
#include <hip/hip_runtime.h>
#include <vector>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include "internal.h"
#include "hipcheck.h"

static thread_local char g_err[512] = "";

extern "C" void htkamd_set_error(const char *fmt, ...)
{
   va_list ap;
   va_start(ap, fmt);
   vsnprintf(g_err, sizeof(g_err), fmt, ap);
   va_end(ap);
}

extern "C" const char *htkamd_last_error(void) { return g_err; }
extern "C" int htkamd_version(void) { return 100; }

extern "C" int htkamd_device_count(void)
{
   int n = 0;
   if (hipGetDeviceCount(&n) != hipSuccess) return 0;
   return n;
}

extern "C" int htkamd_set_device(int ordinal)
{
   HIPCHECK(hipSetDevice(ordinal));
   return HTKAMD_OK;
}

extern "C" int htkamd_dev_malloc(void **dptr, size_t bytes)
{
   if (!dptr) { htkamd_set_error("dev_malloc: NULL"); return HTKAMD_EINVAL; }
   hipError_t e = hipMalloc(dptr, bytes ? bytes : 1);
   if (e != hipSuccess) { htkamd_set_error("dev_malloc(%zu): %s", bytes, hipGetErrorString(e)); return (e == hipErrorOutOfMemory) ? HTKAMD_ENOMEM : HTKAMD_EHIP; }
   return HTKAMD_OK;
}

extern "C" int htkamd_dev_free(void *dptr)
{
   if (dptr) HIPCHECK(hipFree(dptr));
   return HTKAMD_OK;
}

extern "C" int htkamd_memcpy_h2d(void *dDst, const void *hSrc, size_t bytes, void *stream)
{
   if (bytes == 0) return HTKAMD_OK;
   HIPCHECK(hipMemcpyAsync(dDst, hSrc, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
   HIPCHECK(hipStreamSynchronize((hipStream_t)stream));
   return HTKAMD_OK;
}

// host memory the device can read directly (page-locked): a copy from it is a plain DMA, and htkamd_memcpy_h2d_async need not wait for it --
// the copy is ordered before whatever follows on the same stream; the buffer may be refilled once that work has been waited for
extern "C" int htkamd_host_malloc(void **hptr, size_t bytes)
{
   if (!hptr) { htkamd_set_error("host_malloc: NULL"); return HTKAMD_EINVAL; }
   hipError_t e = hipHostMalloc(hptr, bytes ? bytes : 1, hipHostMallocDefault);
   if (e != hipSuccess) { htkamd_set_error("host_malloc(%zu): %s", bytes, hipGetErrorString(e)); return (e == hipErrorOutOfMemory) ? HTKAMD_ENOMEM : HTKAMD_EHIP; }
   return HTKAMD_OK;
}

extern "C" int htkamd_host_free(void *hptr)
{
   if (hptr) HIPCHECK(hipHostFree(hptr));
   return HTKAMD_OK;
}

extern "C" int htkamd_memcpy_h2d_async(void *dDst, const void *hSrc, size_t bytes, void *stream)
{
   if (bytes == 0) return HTKAMD_OK;
   HIPCHECK(hipMemcpyAsync(dDst, hSrc, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
   return HTKAMD_OK;
}

extern "C" int htkamd_memcpy_d2h(void *hDst, const void *dSrc, size_t bytes, void *stream)
{
   if (bytes == 0) return HTKAMD_OK;
   HIPCHECK(hipMemcpyAsync(hDst, dSrc, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
   HIPCHECK(hipStreamSynchronize((hipStream_t)stream));
   return HTKAMD_OK;
}

extern "C" int htkamd_stream_sync(void *stream)
{
   HIPCHECK(hipStreamSynchronize((hipStream_t)stream));
   return HTKAMD_OK;
}

extern "C" int htkamd_stream_create(void **stream)
{
   if (!stream) { htkamd_set_error("stream_create: NULL"); return HTKAMD_EINVAL; }
   hipStream_t s;
   HIPCHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
   *stream = (void *)s;
   return HTKAMD_OK;
}

extern "C" int htkamd_stream_destroy(void *stream)
{
   if (stream) HIPCHECK(hipStreamDestroy((hipStream_t)stream));
   return HTKAMD_OK;
}

// what is queued on `waiter` from here on starts behind what has been queued on `signaller` so far
extern "C" int htkamd_stream_wait(void *waiter, void *signaller)
{
   hipEvent_t ev;
   HIPCHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
   hipError_t e = hipEventRecord(ev, (hipStream_t)signaller);
   if (e == hipSuccess) e = hipStreamWaitEvent((hipStream_t)waiter, ev, 0);
   (void)hipEventDestroy(ev);                            // (released when the record has completed)
   if (e != hipSuccess) { htkamd_set_error("stream_wait: %s", hipGetErrorString(e)); return HTKAMD_EHIP; }
   return HTKAMD_OK;
}

template <typename T> static T *dupHost(const T *src, size_t n)
{
   T *p = (T *)malloc(sizeof(T) * (n ? n : 1));
   if (src && n) memcpy(p, src, sizeof(T) * n);
   return p;
}

// Every array of the model, once: its host field, its device field (NOF: none), the element size and the count as a function of the
// model's sizes.  The loops over this list free, upload and read back; a new array needs its line here, its fill and its use.
// AR_PARAM: a re-estimated parameter -- pushed by model_refresh, read back by htkamd_model_sync_host after a device update.
// AR_UPD: the device copy serves the device update and the DIAGC form alone (htkamd_model_device_tables uploads it on first use).
enum { AR_PARAM = 1, AR_UPD = 2 };
struct ModelArray { size_t h, d, elem; size_t (*count)(const htkamd_model *); int flags; };
#define NOF ((size_t)-1)
#define OF(f) offsetof(htkamd_model, f)
#define CNT(expr) [](const htkamd_model *m) -> size_t { return (size_t)(expr); }
#define TABLE_BYTES(pieces) ((size_t)m->nTiles * ((size_t)(pieces) * m->bf16NC * 64 * 16 + 64 * 16))      /* bf16 x 3, fp16 x 2 (gmm_bf16.hip) */
static const ModelArray MODEL_ARRAYS[] = {
   {OF(h_stateCompOff), OF(d_stateCompOff), sizeof(int), CNT(m->S + 1), 0},
   {OF(h_compGauss), OF(d_compGauss), sizeof(int), CNT(m->C), 0},
   {OF(h_transN), OF(d_transN), sizeof(int), CNT(m->nT), 0},
   {OF(h_transOff), OF(d_transOff), sizeof(int), CNT(m->nT + 1), 0},
   {OF(h_trOccOff), OF(d_trOccOff), sizeof(int), CNT(m->nT + 1), AR_UPD},
   {OF(h_hmmTrans), OF(d_hmmTrans), sizeof(int), CNT(m->H), AR_UPD},
   {OF(h_hmmStateOff), OF(d_hmmStateOff), sizeof(int), CNT(m->H + 1), AR_UPD},
   {OF(h_hmmState), OF(d_hmmState), sizeof(int), CNT(m->h_hmmStateOff[m->H]), AR_UPD},
   {OF(h_minDur), NOF, sizeof(int), CNT(m->nT), 0},
   {OF(h_transLR), NOF, 1, CNT(m->nT), 0},
   {OF(h_mean), OF(d_mean), sizeof(float), CNT((size_t)m->G * m->D), AR_PARAM},
   {OF(h_var), OF(d_var), sizeof(float), CNT((size_t)m->G * m->D), AR_PARAM | AR_UPD},
   {OF(h_ivar), OF(d_ivar), sizeof(float), CNT((size_t)m->G * m->D), AR_PARAM},
   {OF(h_gconst), OF(d_gconst), sizeof(float), CNT(m->G), AR_PARAM},
   {OF(h_compWeight), OF(d_compWeight), sizeof(float), CNT(m->C), AR_PARAM | AR_UPD},
   {OF(h_compLogWt), OF(d_compLogWt), sizeof(float), CNT(m->C), AR_PARAM},
   {OF(h_transP), OF(d_transP), sizeof(float), CNT(m->h_transOff[m->nT]), 0},      // (the device side has 16 counters behind it: model_refresh)
   {OF(h_rawLogWt), OF(d_rawLogWt), 1, CNT(m->C), 0},
   {OF(h_meanLeader), NOF, sizeof(int), CNT(m->G), 0},
   {OF(h_varLeader), NOF, sizeof(int), CNT(m->G), 0},
   {OF(h_varGroupSize), NOF, sizeof(int), CNT(m->G), 0},
   {OF(h_dimStream), OF(d_dimStream), sizeof(int), CNT(m->D), 0},
   {OF(h_gaussStream), OF(d_gaussStream), sizeof(int), CNT(m->G), 0},
   {OF(h_tmPoolOff), OF(d_tmPoolOff), sizeof(int), CNT(m->NSt + 1), 0},
   {OF(h_streamWt), OF(d_streamWt), sizeof(float), CNT(m->S), 0},
   {OF(h_scanOrder), NOF, sizeof(int), CNT(m->H), 0},
   {OF(h_invCov), NOF, sizeof(float), CNT((size_t)m->G * htkamd_tri_size(m->D)), 0},
   {NOF, OF(d_gparam), sizeof(float), CNT((size_t)m->G * m->PS), 0},
   {NOF, OF(d_fparam), sizeof(float), CNT((size_t)m->G * m->FPS), 0},
   {NOF, OF(d_laddTab), sizeof(double), CNT(htkamd_host_ladd_table_size()), 0},
   {NOF, OF(d_msCompOff), sizeof(int), CNT(m->S + 1), 0},
   {NOF, OF(d_shareTab), sizeof(int), CNT(5 * (size_t)m->G + 2 + m->shareMuMem + m->shareVaMem), 0},
   {NOF, OF(d_stateTileOff), sizeof(int), CNT(m->S + 1), 0},
   {NOF, OF(d_tileState), sizeof(int), CNT(m->nTiles), 0},
   {NOF, OF(d_mfmaTab), sizeof(float), CNT((size_t)m->nTiles * (m->mfmaNS + 8) * 64), 0},
   {NOF, OF(d_bf16Tab), 1, CNT(TABLE_BYTES(3)), 0},
   {NOF, OF(d_f16Tab), 1, CNT(TABLE_BYTES(2)), 0},
   {NOF, OF(d_f16Ctl), sizeof(float), CNT(512), 0},
};
static void *&field(htkamd_model *m, size_t off) { return *(void **)((char *)m + off); }
static const ModelArray &array_of(size_t off)           // by its host or device field
{
   for (const ModelArray &a : MODEL_ARRAYS) if (a.h == off || a.d == off) return a;
   abort();
}
static size_t array_bytes(const htkamd_model *m, size_t off) { const ModelArray &a = array_of(off); return a.count(m) * a.elem; }
#define BYTES(m, f) array_bytes(m, OF(f))

// the device side of an array allocated (on first use), and filled from `src` or, src NULL, from its host side
static int upload(htkamd_model *m, const ModelArray &a, const void *src = nullptr)
{
   const size_t n = a.count(m) * a.elem;
   if (!field(m, a.d)) HIPCHECK(hipMalloc(&field(m, a.d), n ? n : 1));
   if (!src && a.h != NOF) src = field(m, a.h);
   if (n && src) HIPCHECK(hipMemcpy(field(m, a.d), src, n, hipMemcpyHostToDevice));
   return HTKAMD_OK;
}
#define UPLOAD(m, f, ...) upload(m, array_of(OF(f)), ##__VA_ARGS__)

// ---- the derived tables of the matrix-core paths: fp32 fragments (gmm_mfma.hip), bf16 x 3 (gmm_bf16.hip), fp16 x 2 (gmm_f16.hip), named
// by their HTKAMD_SCORE_* bit.  Each has one builder, on the device; a FULLC model has none of them.
static const struct DerivedTable { int path; size_t tab; int (*build)(htkamd_model *, void *); const char *refusal; } DERIVED[] = {
   {HTKAMD_SCORE_MFMA, OF(d_mfmaTab), htkamd_model_refresh_mfma_device, "score_mfma: vector size %d not supported by the MFMA path (up to 40)"},
   {HTKAMD_SCORE_BF16, OF(d_bf16Tab), htkamd_model_refresh_bf16_device, "score_bf16: vector size %d not supported by the bf16 matrix-core path (up to 45)"},
   {HTKAMD_SCORE_F16, OF(d_f16Tab), htkamd_model_refresh_f16_device, "score_f16: vector size %d not supported by the fp16 matrix-core path (up to 45)"},
};
// the paths whose tables follow every device update once they have scored; the fp32 table is always rebuilt on its next use
static const int FOLLOWING_PATHS = HTKAMD_SCORE_BF16 | HTKAMD_SCORE_F16, ALL_PATHS = HTKAMD_SCORE_MFMA | FOLLOWING_PATHS;

static int rebuild(htkamd_model *m, int paths, void *stream)
{
   for (const DerivedTable &t : DERIVED)
      if (paths & m->tabStale & t.path) {
         const int rc = t.build(m, stream);
         if (rc) return rc;
         m->tabStale &= ~t.path;
      }
   return HTKAMD_OK;
}

int htkamd_model_params_changed(htkamd_model *m, void *stream, int fromDevice)
{
   m->tabStale = ALL_PATHS;
   const int rc = rebuild(m, fromDevice ? m->fastUse : ALL_PATHS, stream);
   if (rc) return rc;
   if (fromDevice) m->hostStale = 1;
   else HIPCHECK(hipStreamSynchronize((hipStream_t)stream));
   return HTKAMD_OK;
}

int htkamd_model_table_current(const htkamd_model *cm, int path, void *stream)
{
   htkamd_model *m = const_cast<htkamd_model *>(cm);      // (a launcher reads the model; bringing a table up to date is the one thing it may change)
   for (const DerivedTable &t : DERIVED)
      if (t.path == path && !field(m, t.tab)) { htkamd_set_error(t.refusal, m->D); return HTKAMD_EMODEL; }
   const int rc = rebuild(m, path, stream);
   if (rc) return rc;
   m->fastUse |= path & FOLLOWING_PATHS;
   return HTKAMD_OK;
}

// The tile bookkeeping of the derived tables and their memory, once per model: 16 components per tile, a state's tiles one behind the other.
static int derived_tables_alloc(htkamd_model *m)
{
   const int D = m->D;
   if (D > 48 || m->d_stateTileOff) return HTKAMD_OK;    // D > 48: no matrix-core kernel, the exact path serves such sets
   // fp32 path: K steps of 4 = 2 dimensions each; kernels exist for 7, 13 and 20 steps, smaller sizes are zero-padded up to the next
   const int need = (D + 1) / 2;
   m->mfmaNS = need <= 7 ? 7 : (need <= 13 ? 13 : 20);
   std::vector<int> off((size_t)m->S + 1), ts;
   for (int s = 0; s < m->S; s++) {
      off[s + 1] = off[s] + (m->h_stateCompOff[s + 1] - m->h_stateCompOff[s] + 15) / 16;
      for (int t = off[s]; t < off[s + 1]; t++) ts.push_back(s);
   }
   m->nTiles = off[m->S];
   int rc;
   if ((rc = UPLOAD(m, d_stateTileOff, off.data())) || (rc = UPLOAD(m, d_tileState, ts.data()))) return rc;
   m->bf16NC = (D + 14) / 15;                         // 15 dimensions as (x^2, x) pairs + the chunk's constant per K chunk of 32 (gmm_bf16.hip)
   if (m->bf16NC <= 3) {                              // D <= 45
      m->f16Wide = m->nTiles == m->S;
      m->bf16Dense = m->f16Wide && D >= 31 && D <= 39;
      if ((rc = UPLOAD(m, d_bf16Tab)) || (rc = UPLOAD(m, d_f16Tab)) || (rc = UPLOAD(m, d_f16Ctl))) return rc;
      HIPCHECK(hipMemset(m->d_f16Ctl, 0, BYTES(m, d_f16Ctl)));
   }
   return D > 40 ? HTKAMD_OK : UPLOAD(m, d_mfmaTab);     // (the fp32 kernels go up to 20 K steps)
}

// The exact FULLC scorer's parameter table (gmm_full.hip): per Gaussian mean[D], the packed triangle, gConst, zeros up to FPS.
static int fullc_refresh(htkamd_model *m)
{
   const int D = m->D, FPS = m->FPS;
   const size_t TRI = htkamd_tri_size(D);
   float *fp = (float *)calloc((size_t)m->G * FPS, sizeof(float));
   if (!fp) { htkamd_set_error("model: out of memory (FULLC table)"); return HTKAMD_ENOMEM; }
   for (int g = 0; g < m->G; g++) {
      float *p = fp + (size_t)g * FPS;
      memcpy(p, m->h_mean + (size_t)g * D, sizeof(float) * D);
      memcpy(p + D, m->h_invCov + (size_t)g * TRI, sizeof(float) * TRI);
      p[D + TRI] = m->h_gconst[g];
   }
   const int rc = UPLOAD(m, d_fparam, fp);
   free(fp);
   return rc;
}

// What the host derives from its transition matrices, after any change of h_transP: minimum durations (CreateInsts) and left-to-right flags
extern "C" void htkamd_model_refresh_topology(htkamd_model *m)
{
   for (int t = 0; t < m->nT; t++) {
      const int md = htkamd_host_min_dur(m->h_transN[t], m->h_transP + m->h_transOff[t]);
      if (md != m->h_minDur[t]) { m->h_minDur[t] = md; m->topoVersion++; }
      const unsigned char lr = (unsigned char)htkamd_host_trans_is_lr(m->h_transN[t], m->h_transP + m->h_transOff[t]);
      if (lr != m->h_transLR[t]) { m->h_transLR[t] = lr; m->topoVersion++; }
   }
}

// (Re)derive ivar / log weights / min durations / the interleaved scoring table and push them.
static int model_refresh(htkamd_model *m, bool derive = true)
{
   const int D = m->D, PS = m->PS;
   if (derive) {
      htkamd_host_conv_diagc((size_t)m->G * D, m->h_var, m->h_ivar);
      if (m->NSt > 1)                                    // a dimension outside the Gaussian's stream takes no part in its score
         for (int g = 0; g < m->G; g++)
            for (int k = 0; k < D; k++) if (m->h_dimStream[k] != m->h_gaussStream[g]) m->h_ivar[(size_t)g * D + k] = 0.0f;
      for (int c = 0; c < m->C; c++)
         m->h_compLogWt[c] = (m->h_rawLogWt && m->h_rawLogWt[c]) ? m->h_compWeight[c] : htkamd_host_mix_log_weight(m->h_compWeight[c]);
   }
   htkamd_model_refresh_topology(m);
   float *gp = (float *)calloc((size_t)m->G * PS, sizeof(float));
   for (int g = 0; g < m->G; g++) {
      float *p = gp + (size_t)g * PS;
      for (int i = 0; i < D; i++) {
         p[2 * i] = m->h_mean[(size_t)g * D + i];
         p[2 * i + 1] = m->h_ivar[(size_t)g * D + i];
      }
      p[2 * D] = m->h_gconst[g];
   }
   int rc = UPLOAD(m, d_gparam, gp);
   free(gp);
   if (rc) return rc;
   if (!m->d_transP) HIPCHECK(hipMalloc((void **)&m->d_transP, BYTES(m, h_transP) + sizeof(float) * 16));      // + the device update's 16 counters: one copy brings both back (update.hip)
   if ((rc = UPLOAD(m, h_transP))) return rc;
   for (const ModelArray &a : MODEL_ARRAYS)
      if ((a.flags & AR_PARAM) && (!(a.flags & AR_UPD) || m->d_var) && (rc = upload(m, a))) return rc;
   if (m->fullc) return fullc_refresh(m);             // (no matrix-core table: only the exact kernel scores a FULLC set)
   if ((rc = derived_tables_alloc(m))) return rc;
   return htkamd_model_params_changed(m, nullptr, 0);
}

// Linear parameters and the model topology on the device, for the device-side update (uploaded on its first call).
int htkamd_model_device_tables(htkamd_model *m)
{
   if (m->d_var) return HTKAMD_OK;
   for (const ModelArray &a : MODEL_ARRAYS) {
      const int rc = (a.flags & AR_UPD) ? upload(m, a) : HTKAMD_OK;
      if (rc) return rc;
   }
   return HTKAMD_OK;
}

// After a device-side update the host copies are refreshed on demand (get_params, the host update, set_params).
int htkamd_model_sync_host(htkamd_model *m)
{
   if (!m->hostStale) return HTKAMD_OK;
   for (const ModelArray &a : MODEL_ARRAYS)
      if (a.flags & AR_PARAM) HIPCHECK(hipMemcpy(field(m, a.h), field(m, a.d), a.count(m) * a.elem, hipMemcpyDeviceToHost));
   m->hostStale = 0;
   return HTKAMD_OK;
}

static int model_create(const htkamd_model_desc *d, const float *invCov, htkamd_model **out);
extern "C" int htkamd_model_create(const htkamd_model_desc *d, htkamd_model **out) { return model_create(d, nullptr, out); }

// A full-covariance set (MixPDF with ckind FULLC and cov.inv, HModel.h; scored by FOutP HModel.c:5361): desc->var is ignored, invCov holds
// the inverse covariances [G*D(D+1)/2] packed as htkamd_mmf_inv_cov gives them; desc->gconst NULL = FixFullGConst(mp, -CovDet(inv)) (CheckMix).
extern "C" int htkamd_model_create_full(const htkamd_model_desc *d, const float *invCov, htkamd_model **out)
{
   if (!d || !invCov || !out) { htkamd_set_error("model_create_full: NULL argument"); return HTKAMD_EINVAL; }
   if (d->numStreams > 1) { htkamd_set_error("model_create_full: FULLC together with several streams is not supported"); return HTKAMD_EMODEL; }
   if (d->hsKind == HTKAMD_HS_TIED) { htkamd_set_error("model_create_full: FULLC together with tied mixtures (<TMIX>) is not supported"); return HTKAMD_EMODEL; }
   return model_create(d, invCov, out);
}

static int model_create(const htkamd_model_desc *d, const float *invCov, htkamd_model **out)
{
   if (!d || !out) { htkamd_set_error("model_create: NULL argument"); return HTKAMD_EINVAL; }
   if (!invCov && !d->var) {                         // (the description of a FULLC set read by htkamd_mmf_* has no variances)
      htkamd_set_error("model_create: no variances in the description (a FULLC set is made a model by htkamd_model_create_full)"); return HTKAMD_EMODEL;
   }
   if (htkamd_device_count() <= 0) { htkamd_set_error("model_create: no HIP device"); return HTKAMD_ENODEV; }
   if (d->vecSize <= 0 || d->numStates <= 0 || d->numComp <= 0 || d->numGauss <= 0 || d->numTrans <= 0 || d->numPhys <= 0) {
      htkamd_set_error("model_create: empty model"); return HTKAMD_EINVAL;
   }
   htkamd_model *m = (htkamd_model *)calloc(1, sizeof(htkamd_model));
   const int NSt = d->numStreams > 1 ? d->numStreams : 1;
   if (NSt > 1 && !d->dimStream) { free(m); htkamd_set_error("model_create: numStreams = %d without dimStream", NSt); return HTKAMD_EINVAL; }
   m->NSt = NSt;
   m->D = d->vecSize; m->S = d->numStates * NSt; m->C = d->numComp; m->G = d->numGauss; m->nT = d->numTrans; m->H = d->numPhys;
   m->PS = ((2 * m->D + 1) + 3) & ~3;
   m->minLogExp = htkamd_host_min_log_exp();
   m->h_stateCompOff = dupHost(d->stateCompOff, (size_t)m->S + 1);
   m->h_compGauss = dupHost(d->compGauss, (size_t)m->C);
   m->h_compWeight = dupHost(d->compWeight, (size_t)m->C);
   m->h_compLogWt = dupHost((const float *)nullptr, (size_t)m->C);
   m->h_mean = dupHost(d->mean, (size_t)m->G * m->D);
   m->h_var = dupHost(invCov ? nullptr : d->var, (size_t)m->G * m->D);
   if (invCov) {
      for (size_t i = 0; i < (size_t)m->G * m->D; i++) m->h_var[i] = 1.0f;
      m->fullc = 1;
      m->FPS = (int)((m->D + htkamd_tri_size(m->D) + 1 + 3) & ~(size_t)3);
      m->h_invCov = dupHost(invCov, (size_t)m->G * htkamd_tri_size(m->D));
   }
   m->h_ivar = dupHost((const float *)nullptr, (size_t)m->G * m->D);
   m->h_transN = dupHost(d->transN, (size_t)m->nT);
   m->h_transOff = dupHost(d->transOff, (size_t)m->nT + 1);
   m->h_transP = dupHost(d->transP, (size_t)d->transOff[m->nT]);
   m->h_hmmTrans = dupHost(d->hmmTrans, (size_t)m->H);
   m->h_hmmStateOff = dupHost(d->hmmStateOff, (size_t)m->H + 1);
   m->h_hmmState = dupHost(d->hmmState, (size_t)d->hmmStateOff[m->H]);
   if (NSt > 1) {                                        // every emitting state becomes its NSt elements
      const int n = d->hmmStateOff[m->H];
      free(m->h_hmmState);
      m->h_hmmState = (int *)malloc(sizeof(int) * (size_t)(n ? n : 1) * NSt);
      for (int i = 0; i < n; i++) for (int k = 0; k < NSt; k++) m->h_hmmState[(size_t)i * NSt + k] = d->hmmState[i] * NSt + k;
      for (int h = 0; h <= m->H; h++) m->h_hmmStateOff[h] = d->hmmStateOff[h] * NSt;
      m->h_dimStream = dupHost(d->dimStream, (size_t)m->D);
      m->h_gaussStream = (int *)malloc(sizeof(int) * (size_t)m->G);
      for (int g = 0; g < m->G; g++) m->h_gaussStream[g] = -1;
      for (int k = 0; k < m->D; k++) if (d->dimStream[k] < 0 || d->dimStream[k] >= NSt) { htkamd_set_error("model_create: dimStream[%d] = %d", k, d->dimStream[k]); htkamd_model_destroy(m); return HTKAMD_EINVAL; }
      for (int e = 0; e < m->S; e++)
         for (int c = d->stateCompOff[e]; c < d->stateCompOff[e + 1]; c++) {
            const int g = d->compGauss[c];
            if (m->h_gaussStream[g] >= 0 && m->h_gaussStream[g] != e % NSt) { htkamd_set_error("model_create: Gaussian %d is used by streams %d and %d", g, m->h_gaussStream[g] + 1, e % NSt + 1); htkamd_model_destroy(m); return HTKAMD_EINVAL; }
            m->h_gaussStream[g] = e % NSt;
         }
      for (int g = 0; g < m->G; g++) if (m->h_gaussStream[g] < 0) m->h_gaussStream[g] = 0;
      m->h_streamWt = (float *)malloc(sizeof(float) * (size_t)m->S);
      for (int e = 0; e < m->S; e++) m->h_streamWt[e] = d->streamWeight ? d->streamWeight[e] : 1.0f;
   }
   m->h_minDur = dupHost((const int *)nullptr, (size_t)m->nT);
   for (int t = 0; t < m->nT; t++) m->h_minDur[t] = -1;
   m->h_transLR = (unsigned char *)malloc((size_t)(m->nT ? m->nT : 1));
   for (int t = 0; t < m->nT; t++) m->h_transLR[t] = 2;          // unknown: model_refresh sets it
   m->h_trOccOff = dupHost((const int *)nullptr, (size_t)m->nT + 1);
   m->h_gconst = dupHost(d->gconst, (size_t)m->G);
   if (!d->gconst && m->fullc) {                     // CheckMix: FixFullGConst(mp, -CovDet(mp->cov.inv)) (HModel.c:210)
      for (int g = 0; g < m->G; g++)
         if (htkamd_host_fix_full_gconst(m->D, m->h_invCov + (size_t)g * htkamd_tri_size(m->D), m->h_gconst + g)) {
            htkamd_set_error("model_create_full: the inverse covariance of Gaussian %d is not positive definite (CovDet)", g);
            htkamd_model_destroy(m); return HTKAMD_EMODEL;
         }
   } else if (!d->gconst)                            // CheckMix: gConst fixed at load (HModel.c:206-208)
      for (int g = 0; g < m->G; g++) htkamd_host_fix_diag_gconst_ms(m->D, m->h_var + (size_t)g * m->D, m->h_dimStream, m->h_gaussStream ? m->h_gaussStream[g] : 0, m->h_gconst + g);
   m->maxN = 0; m->maxM = 1; m->h_trOccOff[0] = 0;
   for (int t = 0; t < m->nT; t++) {
      if (m->h_transN[t] > m->maxN) m->maxN = m->h_transN[t];
      m->h_trOccOff[t + 1] = m->h_trOccOff[t] + m->h_transN[t];
      if (m->h_transOff[t + 1] - m->h_transOff[t] != m->h_transN[t] * m->h_transN[t]) {
         htkamd_set_error("model_create: transOff inconsistent with transN at matrix %d", t);
         htkamd_model_destroy(m); return HTKAMD_EINVAL;
      }
   }
   for (int s = 0; s < m->S; s++) {
      int M = m->h_stateCompOff[s + 1] - m->h_stateCompOff[s];
      if (M < 1) { htkamd_set_error("model_create: state %d has no mixture component", s); htkamd_model_destroy(m); return HTKAMD_EINVAL; }
      if (M > m->maxM) m->maxM = M;
   }
   for (int h = 0; h < m->H; h++) {
      int N = m->h_transN[m->h_hmmTrans[h]];
      if (m->h_hmmStateOff[h + 1] - m->h_hmmStateOff[h] != (N - 2) * NSt) {
         htkamd_set_error("model_create: HMM %d has %d emitting states but its transP has %d states", h,
                          (m->h_hmmStateOff[h + 1] - m->h_hmmStateOff[h]) / NSt, N);
         htkamd_model_destroy(m); return HTKAMD_EINVAL;
      }
   }
   int rc;
   if ((rc = UPLOAD(m, d_stateCompOff)) || (rc = UPLOAD(m, d_compGauss)) || (rc = UPLOAD(m, d_transN)) || (rc = UPLOAD(m, d_transOff)) ||
       (rc = model_refresh(m))) {
      htkamd_model_destroy(m); return rc;
   }
   if (d->hsKind == HTKAMD_HS_TIED) {
      m->tiedMix = 1; m->tmBeam = 10.0f;
      m->h_tmPoolOff = (int *)calloc((size_t)NSt + 1, sizeof(int));
      for (int k = 0; k < NSt; k++) m->h_tmPoolOff[k + 1] = m->h_tmPoolOff[k] + (m->h_stateCompOff[k + 1] - m->h_stateCompOff[k]);
      m->tmPool = m->h_tmPoolOff[NSt];
      for (int e = 0; e < m->S; e++) {
         const int k = e % NSt, c0 = m->h_stateCompOff[e], M = m->h_stateCompOff[e + 1] - c0, p0 = m->h_stateCompOff[k];
         bool same = M == m->h_stateCompOff[k + 1] - p0;
         for (int i = 0; same && i < M; i++) same = m->h_compGauss[c0 + i] == m->h_compGauss[p0 + i];
         if (!same) { htkamd_set_error("model_create: tied-mixture set: stream %d of state %d does not list its stream's pool", k + 1, e / NSt); htkamd_model_destroy(m); return HTKAMD_EINVAL; }
         if (M < 2) { htkamd_set_error("model_create: tied-mixture set: a pool of one Gaussian"); htkamd_model_destroy(m); return HTKAMD_EINVAL; }
      }
      if ((rc = UPLOAD(m, d_tmPoolOff)) || (rc = htkamd_model_device_tables(m))) { htkamd_model_destroy(m); return rc; }
   }
   if (NSt > 1 || m->tiedMix) {
      std::vector<int> two((size_t)m->S + 1);
      for (int e = 0; e <= m->S; e++) two[e] = 2 * e;
      if ((NSt > 1 && ((rc = UPLOAD(m, d_dimStream)) || (rc = UPLOAD(m, d_gaussStream)) || (rc = UPLOAD(m, d_streamWt)))) ||
          (rc = UPLOAD(m, d_msCompOff, two.data()))) { htkamd_model_destroy(m); return rc; }
   }
   {
      const int n = htkamd_host_ladd_table_size();
      double *tab = (double *)malloc(sizeof(double) * (size_t)n);
      htkamd_host_build_ladd_table(tab);
      rc = UPLOAD(m, d_laddTab, tab);
      free(tab);
      if (rc) { htkamd_model_destroy(m); return rc; }
   }
   *out = m;
   return HTKAMD_OK;
}

extern "C" void htkamd_model_destroy(htkamd_model *m)
{
   if (!m) return;
   for (const ModelArray &a : MODEL_ARRAYS) {
      if (a.h != NOF) free(field(m, a.h));
      if (a.d != NOF) (void)hipFree(field(m, a.d));
   }
   (void)hipFree(m->d_updScratch);
   (void)hipFree(m->d_mllrMean);
   htkamd_outp_ring_free(m->obRing);
   if (m->h_updPin) (void)hipHostFree(m->h_updPin);
   if (m->evUpd) (void)hipEventDestroy((hipEvent_t)m->evUpd);
   free(m);
}

static int compat_raw_logwt(htkamd_model *m);
// Shared mean / variance vectors: share[g] >= 0 names the vector Gaussian g's mean (variance) is a copy of, -1 = private.
extern "C" int htkamd_model_set_scan_order(htkamd_model *m, const int *order)
{
   if (!m) { htkamd_set_error("model_set_scan_order: NULL"); return HTKAMD_EINVAL; }
   free(m->h_scanOrder); m->h_scanOrder = nullptr;
   if (!order) return HTKAMD_OK;
   unsigned char *seen = (unsigned char *)calloc((size_t)(m->H ? m->H : 1), 1);
   for (int k = 0; k < m->H; k++) {
      if (order[k] < 0 || order[k] >= m->H || seen[order[k]]) { free(seen); htkamd_set_error("model_set_scan_order: not a permutation of the %d physical models", m->H); return HTKAMD_EINVAL; }
      seen[order[k]] = 1;
   }
   free(seen);
   m->h_scanOrder = (int *)malloc(sizeof(int) * (size_t)(m->H ? m->H : 1));
   memcpy(m->h_scanOrder, order, sizeof(int) * (size_t)m->H);
   if (m->compat & HTKAMD_COMPAT_SHARED_LOGWT) {           // which state is the FIRST user of a shared pdf depends on the order
      int rc = compat_raw_logwt(m);
      if (rc) return rc;
      if ((rc = model_refresh(m))) return rc;
   }
   return HTKAMD_OK;
}

extern "C" int htkamd_model_set_sharing(htkamd_model *m, const int *meanShare, const int *varShare)
{
   if (!m) { htkamd_set_error("model_set_sharing: NULL model"); return HTKAMD_EINVAL; }
   free(m->h_meanLeader); free(m->h_varLeader); free(m->h_varGroupSize);
   m->h_meanLeader = m->h_varLeader = m->h_varGroupSize = nullptr;
   if (m->d_shareTab) { (void)hipFree(m->d_shareTab); m->d_shareTab = nullptr; }
   bool any = false;
   for (int g = 0; g < m->G; g++) if ((meanShare && meanShare[g] >= 0) || (varShare && varShare[g] >= 0)) any = true;
   if (!any) return HTKAMD_OK;
   int rc = htkamd_model_sync_host(m);
   if (rc) return rc;
   const int G = m->G, D = m->D;
   m->h_meanLeader = (int *)malloc(sizeof(int) * (size_t)G);
   m->h_varLeader = (int *)malloc(sizeof(int) * (size_t)G);
   m->h_varGroupSize = (int *)calloc((size_t)G, sizeof(int));
   for (int pass = 0; pass < 2; pass++) {
      const int *share = pass ? varShare : meanShare;
      int *leader = pass ? m->h_varLeader : m->h_meanLeader;
      const float *vec = pass ? m->h_var : m->h_mean;
      int maxId = -1;
      for (int g = 0; g < G; g++) if (share && share[g] > maxId) maxId = share[g];
      std::vector<int> first((size_t)(maxId + 1), -1);
      for (int g = 0; g < G; g++) {
         leader[g] = g;
         if (!share || share[g] < 0) continue;
         if (first[share[g]] < 0) first[share[g]] = g;
         leader[g] = first[share[g]];
         if (memcmp(vec + (size_t)g * D, vec + (size_t)leader[g] * D, sizeof(float) * (size_t)D)) {
            htkamd_set_error("model_set_sharing: Gaussians %d and %d are declared to share a %s but hold different values", leader[g], g, pass ? "variance" : "mean");
            free(m->h_meanLeader); free(m->h_varLeader); free(m->h_varGroupSize);
            m->h_meanLeader = m->h_varLeader = m->h_varGroupSize = nullptr;
            return HTKAMD_EINVAL;
         }
      }
   }
   for (int g = 0; g < G; g++) m->h_varGroupSize[m->h_varLeader[g]]++;
   // the device update's copy: leaders, group sizes and, per leader, the other members of its group in ascending order (the order
   // in which htkamd_update_models pools their statistics)
   {
      std::vector<int> tab((size_t)3 * G + 2 * ((size_t)G + 1));
      memcpy(tab.data(), m->h_meanLeader, sizeof(int) * (size_t)G);
      memcpy(tab.data() + G, m->h_varLeader, sizeof(int) * (size_t)G);
      memcpy(tab.data() + 2 * (size_t)G, m->h_varGroupSize, sizeof(int) * (size_t)G);
      std::vector<int> mem[2];
      for (int pass = 0; pass < 2; pass++) {
         const int *leader = pass ? m->h_varLeader : m->h_meanLeader;
         int *off = tab.data() + 3 * (size_t)G + (size_t)pass * (G + 1);
         std::vector<int> cnt((size_t)G + 1, 0);
         for (int g = 0; g < G; g++) if (leader[g] != g) cnt[leader[g] + 1]++;
         off[0] = 0;
         for (int g = 0; g < G; g++) off[g + 1] = off[g] + cnt[g + 1];
         mem[pass].resize((size_t)off[G] + 1);
         std::vector<int> fill(off, off + G);
         for (int g = 0; g < G; g++) if (leader[g] != g) mem[pass][fill[leader[g]]++] = g;
         (pass ? m->shareVaMem : m->shareMuMem) = off[G];
      }
      tab.insert(tab.end(), mem[0].begin(), mem[0].begin() + m->shareMuMem);
      tab.insert(tab.end(), mem[1].begin(), mem[1].begin() + m->shareVaMem);
      HIPCHECK(hipMalloc(&m->d_shareTab, sizeof(int) * tab.size()));
      HIPCHECK(hipMemcpy(m->d_shareTab, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice));
   }
   return HTKAMD_OK;
}

extern "C" int htkamd_model_set_tm_beam(htkamd_model *m, float tmBeam)
{
   if (!m || !(tmBeam >= 0.0f)) { htkamd_set_error("model_set_tm_beam: bad argument"); return HTKAMD_EINVAL; }
   m->tmBeam = tmBeam;
   return HTKAMD_OK;
}

// HTKAMD_COMPAT_SHARED_LOGWT: ConvLogWt (HUtil.c:474-485) walks the set with GoNextMix(noSkip = FALSE), which passes over a mixture
// component whose pdf it has met before (HUtil.c:371-394: IsSeen(mp->nUse)) -- the WEIGHT of that component stays linear and is read as
// a log weight from then on (MixLogWeight returns it as it stands once hset->logWt is set, HModel.c:5290).  The walk: models in HMM scan
// order, a model's states 2 .. N - 1 (a state met before is skipped whole), streams, components.
static int compat_raw_logwt(htkamd_model *m)
{
   free(m->h_rawLogWt); m->h_rawLogWt = nullptr;
   if (m->d_rawLogWt) { (void)hipFree(m->d_rawLogWt); m->d_rawLogWt = nullptr; }
   if (!(m->compat & HTKAMD_COMPAT_SHARED_LOGWT) || m->tiedMix) return HTKAMD_OK;
   unsigned char *raw = (unsigned char *)calloc((size_t)(m->C ? m->C : 1), 1);
   const int NSt = m->NSt > 1 ? m->NSt : 1;
   unsigned char *seenS = (unsigned char *)calloc((size_t)(m->S ? m->S : 1) * NSt, 1), *seenG = (unsigned char *)calloc((size_t)(m->G ? m->G : 1), 1);
   int any = 0;
   for (int hh = 0; hh < m->H; hh++) {
      const int h = m->h_scanOrder ? m->h_scanOrder[hh] : hh;
      for (int j = m->h_hmmStateOff[h]; j < m->h_hmmStateOff[h + 1]; j++) {
         const int e = m->h_hmmState[j];                    // a (state, stream) element: the list holds a state's streams one after the other
         if (seenS[e]) continue;                            // (a state met before is skipped whole: its elements with it)
         seenS[e] = 1;
         for (int c = m->h_stateCompOff[e]; c < m->h_stateCompOff[e + 1]; c++) {
            const int g = m->h_compGauss[c];
            if (seenG[g]) { raw[c] = 1; any = 1; } else seenG[g] = 1;
         }
      }
   }
   free(seenS); free(seenG);
   if (!any) { free(raw); return HTKAMD_OK; }             // no pdf is shared: nothing differs
   m->h_rawLogWt = raw;
   HIPCHECK(hipMalloc((void **)&m->d_rawLogWt, (size_t)m->C));
   HIPCHECK(hipMemcpy(m->d_rawLogWt, raw, (size_t)m->C, hipMemcpyHostToDevice));
   return HTKAMD_OK;
}

extern "C" int htkamd_model_set_compat(htkamd_model *m, int flags)
{
   if (!m || (flags & ~(HTKAMD_COMPAT_STREAM_REVISIT | HTKAMD_COMPAT_SHARED_LOGWT))) { htkamd_set_error("model_set_compat: unknown flags %d", flags); return HTKAMD_EINVAL; }
   const bool wtChange = ((m->compat ^ flags) & HTKAMD_COMPAT_SHARED_LOGWT) != 0;
   m->compat = flags;
   if (wtChange) {
      int rc = compat_raw_logwt(m);
      if (rc) return rc;
      if ((rc = model_refresh(m))) return rc;
   }
   return HTKAMD_OK;
}

extern "C" int htkamd_model_has_sharing(const htkamd_model *m) { return m && m->h_meanLeader ? 1 : 0; }

extern "C" int htkamd_model_set_params(htkamd_model *m, const float *mean, const float *var, const float *gconst,
                                       const float *compWeight, const float *transP)
{
   if (!m) { htkamd_set_error("model_set_params: NULL model"); return HTKAMD_EINVAL; }
   if (m->fullc && var) { htkamd_set_error("model_set_params: a FULLC model has no variances (htkamd_model_set_inv_cov)"); return HTKAMD_EMODEL; }
   { int rc0 = htkamd_model_sync_host(m); if (rc0) return rc0; }
   if (mean) memcpy(m->h_mean, mean, BYTES(m, h_mean));
   if (var) memcpy(m->h_var, var, BYTES(m, h_var));
   if (gconst) memcpy(m->h_gconst, gconst, BYTES(m, h_gconst));
   else if (var)
      for (int g = 0; g < m->G; g++) htkamd_host_fix_diag_gconst_ms(m->D, m->h_var + (size_t)g * m->D, m->h_dimStream, m->h_gaussStream ? m->h_gaussStream[g] : 0, m->h_gconst + g);
   if (compWeight) memcpy(m->h_compWeight, compWeight, BYTES(m, h_compWeight));
   if (transP) memcpy(m->h_transP, transP, BYTES(m, h_transP));
   return model_refresh(m);
}

// Prepared tables given by the caller (an HTKLib front-end that has already run ConvDiagC / ConvLogWt / FixGConsts on its HMMSet):
// the kernels then read the caller's own floats, bit for bit, instead of values re-derived from variances and linear weights.
extern "C" int htkamd_model_set_prepared(htkamd_model *m, const float *ivar, const float *gconst, const float *compLogWt)
{
   if (!m) { htkamd_set_error("model_set_prepared: NULL model"); return HTKAMD_EINVAL; }
   if (m->fullc) { htkamd_set_error("model_set_prepared: the prepared DIAGC tables do not apply to a FULLC model"); return HTKAMD_EMODEL; }
   { int rc0 = htkamd_model_sync_host(m); if (rc0) return rc0; }
   if (ivar) memcpy(m->h_ivar, ivar, BYTES(m, h_ivar));
   if (gconst) memcpy(m->h_gconst, gconst, BYTES(m, h_gconst));
   if (compLogWt) memcpy(m->h_compLogWt, compLogWt, BYTES(m, h_compLogWt));
   return model_refresh(m, false);
}

extern "C" int htkamd_model_get_prepared(htkamd_model *m, float *ivar, float *gconst, float *compLogWt, int *minDur)
{
   if (!m) { htkamd_set_error("model_get_prepared: NULL model"); return HTKAMD_EINVAL; }
   // read back from the DEVICE copies so that tests see what the kernels see
   if (ivar) HIPCHECK(hipMemcpy(ivar, m->d_ivar, BYTES(m, d_ivar), hipMemcpyDeviceToHost));
   if (gconst) HIPCHECK(hipMemcpy(gconst, m->d_gconst, BYTES(m, d_gconst), hipMemcpyDeviceToHost));
   if (compLogWt) HIPCHECK(hipMemcpy(compLogWt, m->d_compLogWt, BYTES(m, d_compLogWt), hipMemcpyDeviceToHost));
   if (minDur) memcpy(minDur, m->h_minDur, BYTES(m, h_minDur));
   return HTKAMD_OK;
}

extern "C" int htkamd_model_update(htkamd_model *m, const htkamd_accs *accs, const double *hostVec,
                                   const htkamd_update_config *cfg, htkamd_update_stats *stats)
{
   if (!m || !accs || !hostVec || !cfg || !stats) { htkamd_set_error("model_update: NULL argument"); return HTKAMD_EINVAL; }
   if (accs->m != m) { htkamd_set_error("model_update: accumulators belong to a different model"); return HTKAMD_EINVAL; }
   int rc = htkamd_model_sync_host(m);
   if (rc) return rc;
   rc = htkamd_update_models(m, &accs->lay, hostVec, cfg, stats);
   if (rc && rc != HTKAMD_EMODEL) return rc;
   const int rc2 = model_refresh(m);
   return rc2 ? rc2 : rc;
}

extern "C" int htkamd_model_get_params(htkamd_model *m, float *mean, float *var, float *gconst, float *compWeight, float *transP)
{
   if (!m) { htkamd_set_error("model_get_params: NULL model"); return HTKAMD_EINVAL; }
   { int rc0 = htkamd_model_sync_host(m); if (rc0) return rc0; }
   if (mean) memcpy(mean, m->h_mean, BYTES(m, h_mean));
   if (var) memcpy(var, m->h_var, BYTES(m, h_var));
   if (gconst) memcpy(gconst, m->h_gconst, BYTES(m, h_gconst));
   if (compWeight) memcpy(compWeight, m->h_compWeight, BYTES(m, h_compWeight));
   if (transP) memcpy(transP, m->h_transP, BYTES(m, h_transP));
   return HTKAMD_OK;
}

// The inverse covariances of a FULLC model (mp->cov.inv, HModel.h), packed as htkamd_model_create_full takes them.  set: gconst NULL =
// FixFullGConst(mp, -CovDet(inv)) for every Gaussian, as FixGConsts does after an update (HModel.c:5688, HERest.c:1309).
extern "C" int htkamd_model_set_inv_cov(htkamd_model *m, const float *invCov, const float *gconst)
{
   if (!m || !invCov) { htkamd_set_error("model_set_inv_cov: NULL argument"); return HTKAMD_EINVAL; }
   if (!m->fullc) { htkamd_set_error("model_set_inv_cov: not a FULLC model"); return HTKAMD_EMODEL; }
   const size_t TRI = htkamd_tri_size(m->D);
   float *gc = (float *)malloc(sizeof(float) * (size_t)(m->G ? m->G : 1));
   for (int g = 0; g < m->G; g++) {
      if (gconst) gc[g] = gconst[g];
      else if (htkamd_host_fix_full_gconst(m->D, invCov + (size_t)g * TRI, gc + g)) {
         free(gc); htkamd_set_error("model_set_inv_cov: the inverse covariance of Gaussian %d is not positive definite (CovDet)", g); return HTKAMD_EMODEL;
      }
   }
   memcpy(m->h_invCov, invCov, BYTES(m, h_invCov));
   memcpy(m->h_gconst, gc, BYTES(m, h_gconst));
   free(gc);
   return model_refresh(m);
}

extern "C" int htkamd_model_get_inv_cov(htkamd_model *m, float *invCov)
{
   if (!m || !invCov) { htkamd_set_error("model_get_inv_cov: NULL argument"); return HTKAMD_EINVAL; }
   if (!m->fullc) { htkamd_set_error("model_get_inv_cov: not a FULLC model"); return HTKAMD_EMODEL; }
   memcpy(invCov, m->h_invCov, BYTES(m, h_invCov));
   return HTKAMD_OK;
}

extern "C" int htkamd_model_is_full(const htkamd_model *m) { return m && m->fullc ? 1 : 0; }

// ------------------------------------------------------------------------------------ accumulators

extern "C" int htkamd_accs_create(htkamd_model *m, htkamd_accs **out)
{
   if (!m || !out) { htkamd_set_error("accs_create: NULL argument"); return HTKAMD_EINVAL; }
   if (m->fullc) { htkamd_set_error("accs_create: re-estimation of FULLC models is not supported yet (scoring, alignment and decoding are)"); return HTKAMD_EMODEL; }
   htkamd_accs *a = (htkamd_accs *)calloc(1, sizeof(htkamd_accs));
   a->m = m;
   size_t o = 0, GD = (size_t)m->G * m->D;
   a->lay.mu = o; o += GD;
   a->lay.muOcc = o; o += m->G;
   a->lay.va = o; o += GD;
   a->lay.vaOcc = o; o += m->G;
   a->lay.wt = o; o += m->C;
   a->lay.wtOcc = o; o += m->S;
   a->lay.tr = o; o += m->h_transOff[m->nT];
   a->lay.trOcc = o; o += m->h_trOccOff[m->nT];
   a->lay.nEgs = o; o += m->H;
   a->lay.totalPr = o++; a->lay.totalT = o++; a->lay.nUttDone = o++; a->lay.nUttSkipped = o++; a->lay.nEval = o++;
   a->lay.total = o;
   // (room to the next 256 bytes behind the vector: htkamd_accs_zero clears whole 256-byte blocks -- a size that is not such a multiple is
   //  filled by two kernels, bulk and tail, 4 us apart in every EM iteration)
   const size_t oPad = (o + 31) & ~(size_t)31;
   hipError_t e = hipMalloc((void **)&a->d_vec, sizeof(double) * oPad);
   if (e != hipSuccess) { htkamd_set_error("accs_create: hipMalloc(%zu doubles): %s", o, hipGetErrorString(e)); free(a); return HTKAMD_ENOMEM; }
   e = hipMemset(a->d_vec, 0, sizeof(double) * oPad);
   if (e != hipSuccess) { htkamd_set_error("accs_create: hipMemset: %s", hipGetErrorString(e)); (void)hipFree(a->d_vec); free(a); return HTKAMD_EHIP; }
   *out = a;
   return HTKAMD_OK;
}

extern "C" void htkamd_accs_destroy(htkamd_accs *a)
{
   if (!a) return;
   (void)hipFree(a->d_vec);
   free(a);
}

extern "C" int htkamd_accs_zero(htkamd_accs *a, void *stream)
{
   if (!a) { htkamd_set_error("accs_zero: NULL"); return HTKAMD_EINVAL; }
   HIPCHECK(hipMemsetAsync(a->d_vec, 0, sizeof(double) * ((a->lay.total + 31) & ~(size_t)31), (hipStream_t)stream));
   return HTKAMD_OK;
}

extern "C" int htkamd_accs_get_layout(const htkamd_accs *a, htkamd_accs_layout *out)
{
   if (!a || !out) { htkamd_set_error("accs_get_layout: NULL"); return HTKAMD_EINVAL; }
   *out = a->lay;
   return HTKAMD_OK;
}

extern "C" int htkamd_accs_device_vector(htkamd_accs *a, double **dVec, size_t *n)
{
   if (!a || !dVec || !n) { htkamd_set_error("accs_device_vector: NULL"); return HTKAMD_EINVAL; }
   *dVec = a->d_vec; *n = a->lay.total;
   return HTKAMD_OK;
}

extern "C" int htkamd_accs_download(htkamd_accs *a, double *hostVec, void *stream)
{
   if (!a || !hostVec) { htkamd_set_error("accs_download: NULL"); return HTKAMD_EINVAL; }
   HIPCHECK(hipMemcpyAsync(hostVec, a->d_vec, sizeof(double) * a->lay.total, hipMemcpyDeviceToHost, (hipStream_t)stream));
   HIPCHECK(hipStreamSynchronize((hipStream_t)stream));
   return HTKAMD_OK;
}

__global__ void k_vec_add(double *__restrict__ dst, const double *__restrict__ src, size_t n)
{
   size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, st = (size_t)gridDim.x * blockDim.x;
   for (; i < n; i += st) dst[i] += src[i];
}

extern "C" int htkamd_accs_upload_add(htkamd_accs *a, const double *hostVec, void *stream)
{
   if (!a || !hostVec) { htkamd_set_error("accs_upload_add: NULL"); return HTKAMD_EINVAL; }
   double *tmp = nullptr;
   HIPCHECK(hipMalloc((void **)&tmp, sizeof(double) * a->lay.total));
   struct Free { double *p; ~Free() { (void)hipFree(p); } } freeTmp{tmp};      // released on every path
   hipStream_t s = (hipStream_t)stream;
   HIPCHECK(hipMemcpyAsync(tmp, hostVec, sizeof(double) * a->lay.total, hipMemcpyHostToDevice, s));
   hipLaunchKernelGGL(k_vec_add, dim3(1024), dim3(256), 0, s, a->d_vec, tmp, a->lay.total);
   HIPCHECK(hipGetLastError());
   HIPCHECK(hipStreamSynchronize(s));
   return HTKAMD_OK;
}
