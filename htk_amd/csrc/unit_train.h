// unit_train.h -- what the isolated-unit trainers share (hinit.hip, hrest.hip; the host refusals: host/unit_train.c): the models of a call
// are independent and run side by side, a workgroup per model wherever a model's parameters are written.  Here: the model / token tables,
// the snapshot of the parameters a failed model is put back to, the restore, the block scan, the gather of the running tokens' rows, a
// transition row renormalised and logged in float, and the way out of a call.  NT is the workgroup size of the calling kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <vector>
#include "internal.h"
#include "hipcheck.h"
#include "devbuf.h"
#include "gauss_derive.h"

// tok0: its first token; tp0 / occ0: first element of its transition matrix / row occupations; st0: of its state list; pool0: its first pool (HInit)
struct UnitModel { int h, ne, N, tok0, nTok, tp0, st0, occ0, pool0; };

struct UnitParams {
   GaussTables g;
   const int *hmmState;
   float *mean, *var, *compWeight, *transP;
   const float *bakMean, *bakVar, *bakWeight, *bakTransP;    // the snapshot made before the first pass
};

template <int NT> static __device__ int unit_block_excl_scan(int v, int *lds, int *total)
{
   const int t = threadIdx.x;
   lds[t] = v;
   __syncthreads();
   for (int o = 1; o < NT; o <<= 1) {
      const int x = t >= o ? lds[t - o] : 0;
      __syncthreads();
      lds[t] += x;
      __syncthreads();
   }
   const int incl = lds[t];
   *total = lds[NT - 1];
   __syncthreads();
   return incl - v;
}

template <int NT> static __device__ void unit_gather_rows(float *dst, const float *src, size_t n)
{
   for (size_t e = threadIdx.x; e < n; e += NT) dst[e] = src[e];
}

// the parameters of one model from the snapshot, by the whole workgroup
template <int NT> static __device__ void unit_restore(const UnitParams &p, const UnitModel &m)
{
   const int D = p.g.D, t = threadIdx.x;
   for (int s = 0; s < m.ne; s++) {
      const int st = p.hmmState[m.st0 + s], c0 = p.g.stateCompOff[st], M = p.g.stateCompOff[st + 1] - c0;
      for (int e = t; e < M * D; e += NT) {
         const size_t x = (size_t)p.g.compGauss[c0 + e / D] * D + e % D;
         p.mean[x] = p.bakMean[x]; p.var[x] = p.bakVar[x];
      }
      for (int k = t; k < M; k += NT) p.compWeight[c0 + k] = p.bakWeight[c0 + k];
   }
   for (int e = t; e < m.N * m.N; e += NT) p.transP[m.tp0 + e] = p.bakTransP[m.tp0 + e];
}

// the models of a call back to their snapshot, derived tables included: those with only[r] != 0, or every one where `only` is null
template <int NT> __global__ __launch_bounds__(NT) void k_unit_restore(UnitParams p, const UnitModel *mdl, const int *only)
{
   if (only && !only[blockIdx.x]) return;
   const UnitModel m = mdl[blockIdx.x];
   unit_restore<NT>(p, m);
   __syncthreads();
   for (int s = 0; s < m.ne; s++) htkamd_derive_state(p.g, p.hmmState[m.st0 + s], NT);
}

// row (of N) of a transition matrix from the counts count(0 .. N-1) of its transitions and its occupation: renormalised, logged, all in float
template <typename F> static __device__ void unit_trans_row(float *row, int N, F count, float occ)
{
   float sum = 0.0f;
   for (int j = 2; j <= N; j++) sum = __fadd_rn(sum, __fdiv_rn(count(j - 1), occ));
   row[0] = (float)LZERO;
   for (int j = 2; j <= N; j++) {
      const float x = __fdiv_rn(__fdiv_rn(count(j - 1), occ), sum);
      row[j - 1] = ((double)x < MINLARG) ? (float)LZERO : (float)log((double)x);
   }
}

// ------------------------------------------------------------------------------------------ host
// what the call itself refuses on the handle; *d: the description the model was made from, for the tool's own check (host/unit_train.c)
static int unit_refuse_handle(const htkamd_model *m, const char *pfx, const char *tool, htkamd_model_desc *d)
{
   if (m->fullc) { htkamd_set_error("%s: a FULLC set (%s on full covariances is not supported)", pfx, tool); return HTKAMD_EMODEL; }
   if (m->h_meanLeader) { htkamd_set_error("%s: a set with shared mean / variance vectors (~u / ~v)", pfx); return HTKAMD_EMODEL; }
   if (m->h_rawLogWt) { htkamd_set_error("%s: HTKAMD_COMPAT_SHARED_LOGWT is set (mixtures that share pdfs)", pfx); return HTKAMD_EMODEL; }
   memset(d, 0, sizeof(*d));
   d->vecSize = m->D; d->numStates = m->S / m->NSt; d->numComp = m->C; d->numGauss = m->G; d->numTrans = m->nT; d->numPhys = m->H;
   d->stateCompOff = m->h_stateCompOff; d->compGauss = m->h_compGauss; d->var = m->h_var; d->hmmTrans = m->h_hmmTrans;
   d->hmmStateOff = m->h_hmmStateOff; d->hmmState = m->h_hmmState; d->numStreams = m->NSt; d->hsKind = m->tiedMix ? HTKAMD_HS_TIED : HTKAMD_HS_PLAIN;
   return HTKAMD_OK;
}

struct UnitTables {
   std::vector<UnitModel> mdl; std::vector<int> mdlOf;      // mdlOf[r] = its place in `models`
   std::vector<int> aFrame, aLen, aMdl;                     // the tokens of the models in `mdl`, behind one another per model (the given order within a model)
   long long totFrames = 0;
};

// The models of the call that take part and their tokens (those of `keep`, every one where it is null).  takes(k, ne, its tokens) says
// whether model k of the list does; extra(x, r) sees the record of such a model before it becomes t.mdl[r], adds what the tool keeps per
// model (x.pool0 is its to set) and may refuse with an error code.  Nothing to train leaves t.mdl empty and returns HTKAMD_OK.
template <typename Takes, typename Extra>
static int unit_tables(const char *pfx, htkamd_model *m, int nTokens, const int *tokFrame, const int *tokLen, const int *tokModel, const int *keep,
                       int nModels, const int *models, Takes takes, Extra extra, UnitTables &t)
{
   std::vector<int> ofPhys((size_t)m->H, -1);
   for (int k = 0; k < nModels; k++) ofPhys[models[k]] = k;
   std::vector<std::vector<int>> toks((size_t)nModels);
   for (int k = 0; k < nTokens; k++) if (ofPhys[tokModel[k]] >= 0 && (!keep || keep[k])) toks[ofPhys[tokModel[k]]].push_back(k);
   for (int k = 0; k < nModels; k++) {
      const int h = models[k], ti = m->h_hmmTrans[h];
      UnitModel x;
      x.h = h; x.N = m->h_transN[ti]; x.ne = x.N - 2; x.tok0 = (int)t.aFrame.size(); x.nTok = (int)toks[k].size(); x.pool0 = 0;
      x.tp0 = m->h_transOff[ti]; x.st0 = m->h_hmmStateOff[h]; x.occ0 = m->h_trOccOff[ti];
      if (!takes(k, x.ne, toks[k])) continue;
      for (int tk : toks[k]) { t.aFrame.push_back(tokFrame[tk]); t.aLen.push_back(tokLen[tk]); t.aMdl.push_back((int)t.mdl.size()); t.totFrames += tokLen[tk]; }
      const int rc = extra(x, (int)t.mdl.size());
      if (rc) return rc;
      t.mdl.push_back(x); t.mdlOf.push_back(k);
   }
   if (t.mdl.empty()) return HTKAMD_OK;
   if (t.totFrames >= ((long long)1 << 31)) { htkamd_set_error("%s: %lld frames in the tokens (the tables index with 32 bits)", pfx, t.totFrames); return HTKAMD_EINVAL; }
   const int rc = htkamd_model_sync_host(m);
   return rc ? rc : htkamd_model_device_tables(m);
}

// *p points at the model's arrays on the device and at a copy of mean / var / weights / transP made now, in `bak`
template <const char *Owner> int unit_snapshot(const htkamd_model *m, DevBufT<Owner> &bak, hipStream_t s, UnitParams *p)
{
   const size_t nGD = (size_t)m->G * m->D, nC = (size_t)m->C, nTp = (size_t)m->h_transOff[m->nT];
   const int rc = bak.template reserve<float>(2 * nGD + nC + nTp);
   if (rc) return rc;
   float *b = bak.template as<float>();
   HIPCHECK(hipMemcpyAsync(b, m->d_mean, sizeof(float) * nGD, hipMemcpyDeviceToDevice, s));
   HIPCHECK(hipMemcpyAsync(b + nGD, m->d_var, sizeof(float) * nGD, hipMemcpyDeviceToDevice, s));
   HIPCHECK(hipMemcpyAsync(b + 2 * nGD, m->d_compWeight, sizeof(float) * nC, hipMemcpyDeviceToDevice, s));
   HIPCHECK(hipMemcpyAsync(b + 2 * nGD + nC, m->d_transP, sizeof(float) * nTp, hipMemcpyDeviceToDevice, s));
   GaussTables &g = p->g;
   g.D = m->D; g.PS = m->PS; g.logTpiD = (float)(m->D * log(HTK_TPI)); g.stateCompOff = m->d_stateCompOff; g.compGauss = m->d_compGauss;
   g.mean = m->d_mean; g.var = m->d_var; g.compWeight = m->d_compWeight; g.ivar = m->d_ivar; g.gconst = m->d_gconst; g.gparam = m->d_gparam;
   g.compLogWt = m->d_compLogWt;
   p->hmmState = m->d_hmmState; p->mean = m->d_mean; p->var = m->d_var; p->compWeight = m->d_compWeight; p->transP = m->d_transP;
   p->bakMean = b; p->bakVar = b + nGD; p->bakWeight = b + 2 * nGD; p->bakTransP = b + 2 * nGD + nC;
   return HTKAMD_OK;
}

// the way out of a call, error or not: the derived tables, the host's transition matrices with what follows from them, the host mirror
static int unit_finish(htkamd_model *m, hipStream_t s)
{
   const int rc = htkamd_model_params_changed(m, s, 1);
   if (rc) return rc;
   HIPCHECK(hipMemcpyAsync(m->h_transP, m->d_transP, sizeof(float) * (size_t)m->h_transOff[m->nT], hipMemcpyDeviceToHost, s));
   HIPCHECK(hipStreamSynchronize(s));
   htkamd_model_refresh_topology(m);
   return htkamd_model_sync_host(m);
}
