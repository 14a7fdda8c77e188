// hrest.hip -- isolated-unit Baum-Welch re-estimation (HTKTools/HRest.c) for every model of a list in one call.  The refusals and the
// token bookkeeping: host/hrest.c.  What the call shares with htkamd_hinit -- the model / token tables, the snapshot with unit_restore and
// k_unit_restore, the block scan, the gather, the float transition row, the way out of the call -- is unit_train.h; here is HRest's own.
//
// A pass (ReEstimateModel HRest.c:1309) is one forward-backward batch (htkamd_fb_*) over the kept tokens of the models still running,
// one single-model utterance per token, with these kernels around it:
// k_hr_compact: the running-token list.  The kept tokens lie behind one another per model (the given order within a model); one workgroup
//   counts the tokens of running models chunk by chunk, scans the counts and the frame counts, and fills the list: utterance u is token
//   uTok[u], its rows start at uFrame0[u]; a model's utterances start at mdlUtt0[r].  Run only when the set of running models changed.
// k_hr_gather: the utterances' rows behind one another (what htkamd_fb_prepare takes).
// k_hr_zero: ZeroAccs for the running models only, a workgroup per model.
// k_hr_logp: a lane per running model: newP (:1328) as the float sum of its usable tokens' log probabilities in token order, and
//   nTokUsed; no usable token is HError 2226.
// k_hr_update: UpdateTheModel (:1287), a workgroup per running model, from the fp64 statistics rounded to float once: RestTransP (:1015),
//   per state RestMixWeights (:1124), RestMean (:1165) / RestCoVar (:1185) of the components whose new weight exceeds MINMIX -- the
//   variance floored first, then tested against vDefunct: a defunct component of a mixture gets weight 0 (-2225), a single Gaussian is
//   HError 2222 --, FloorMixes (:1043, 2223); every zero occupation is 2222.  A model that fails takes back the parameters it came with
//   (the snapshot made before the first pass) in the same kernel; then the derived tables of its Gaussians are rebuilt (gauss_derive.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "internal.h"
#include "hipcheck.h"
#include "unit_train.h"

#define HR_THREADS 256

struct HrOut { float sum; int used, status; };                     // per running model and pass

struct HrArgs {
   UnitParams p;                                            // the model's arrays and their snapshot
   int uFlags;
   float minVar, vDefunct, mixWeightFloor;
   double *acc; htkamd_accs_layout lay;
   const float *X; float *Xg;
   const UnitModel *mdl; int nMdl;                          // (tok0: its first kept token)
   const int *tokFrame, *tokLen, *tokMdl; int nTok;
   const int *runFlag;                                      // [nMdl]
   int *uTok, *uFrame0, *mdlUtt0, *nUttOut;                 // uFrame0 [nTok+1]; nUttOut: utterances, frames
   const int *runMdl; int nRun;
   const double *pr; const int *uttStatus;
   int *mstatus;                                            // [nMdl]
   HrOut *out;                                              // [nRun]
};

// (INVARIANT shared with the host loop of htkamd_hrest: utterance u is the u-th kept token of a running model in the order of the token
// arrays; the host lays out the same list for htkamd_fb_prepare and compares the two totals written here)
__global__ __launch_bounds__(HR_THREADS) void k_hr_compact(HrArgs a)
{
   __shared__ int lds[HR_THREADS];
   int baseU = 0, baseF = 0;
   for (int k0 = 0; k0 < a.nTok; k0 += HR_THREADS) {
      const int k = k0 + threadIdx.x;
      const bool in = k < a.nTok;
      const int r = in ? a.tokMdl[k] : 0;
      const int run = in ? a.runFlag[r] : 0, len = run ? a.tokLen[k] : 0;
      int totU, totF;
      const int exU = unit_block_excl_scan<HR_THREADS>(run, lds, &totU);
      const int exF = unit_block_excl_scan<HR_THREADS>(len, lds, &totF);
      if (in && k == a.mdl[r].tok0) a.mdlUtt0[r] = baseU + exU;
      if (run) { a.uTok[baseU + exU] = k; a.uFrame0[baseU + exU] = baseF + exF; }
      baseU += totU; baseF += totF;
   }
   if (threadIdx.x == 0) { a.uFrame0[baseU] = baseF; a.nUttOut[0] = baseU; a.nUttOut[1] = baseF; }
}

__global__ __launch_bounds__(HR_THREADS) void k_hr_gather(HrArgs a)
{
   const int u = blockIdx.x, D = a.p.g.D;
   if (u >= a.nUttOut[0]) return;
   unit_gather_rows<HR_THREADS>(a.Xg + (size_t)a.uFrame0[u] * D, a.X + (size_t)a.tokFrame[a.uTok[u]] * D, (size_t)(a.uFrame0[u + 1] - a.uFrame0[u]) * D);
}

__global__ __launch_bounds__(HR_THREADS) void k_hr_zero(HrArgs a)
{
   const UnitModel m = a.mdl[a.runMdl[blockIdx.x]];
   const int D = a.p.g.D, t = threadIdx.x;
   for (int s = 0; s < m.ne; s++) {
      const int st = a.p.hmmState[m.st0 + s], c0 = a.p.g.stateCompOff[st], M = a.p.g.stateCompOff[st + 1] - c0;
      for (int e = t; e < M * D; e += HR_THREADS) {
         const size_t x = (size_t)a.p.g.compGauss[c0 + e / D] * D + e % D;
         a.acc[a.lay.mu + x] = 0.0; a.acc[a.lay.va + x] = 0.0;
      }
      for (int k = t; k < M; k += HR_THREADS) {
         const int g = a.p.g.compGauss[c0 + k];
         a.acc[a.lay.muOcc + g] = 0.0; a.acc[a.lay.vaOcc + g] = 0.0; a.acc[a.lay.wt + c0 + k] = 0.0;
      }
      if (t == 0) a.acc[a.lay.wtOcc + st] = 0.0;
   }
   for (int e = t; e < m.N * m.N; e += HR_THREADS) a.acc[a.lay.tr + m.tp0 + e] = 0.0;
   for (int e = t; e < m.N; e += HR_THREADS) a.acc[a.lay.trOcc + m.occ0 + e] = 0.0;
   if (t == 0) a.acc[a.lay.nEgs + m.h] = 0.0;
}

__global__ void k_hr_logp(HrArgs a)
{
   const int q = blockIdx.x * blockDim.x + threadIdx.x;
   if (q >= a.nRun) return;
   const int r = a.runMdl[q], u0 = a.mdlUtt0[r], n = a.mdl[r].nTok;
   float s = 0.0f; int used = 0;
   for (int u = u0; u < u0 + n; u++)
      if (a.uttStatus[u] == HTKAMD_UTT_OK) { s = __fadd_rn(s, (float)a.pr[u]); used++; }      // else "Example skipped"
   int ms = a.mstatus[r];
   if (!ms && used == 0) { ms = HTKAMD_HREST_ENOUSABLE; a.mstatus[r] = ms; }     // (this lane alone writes the model's status now)
   a.out[q].sum = s; a.out[q].used = used; a.out[q].status = ms;
}

#define ACCF(off, idx) ((float)a.acc[(off) + (size_t)(idx)])

__global__ __launch_bounds__(HR_THREADS) void k_hr_update(HrArgs a)
{
   extern __shared__ int firstBad[];                        // [maxM] per component of the state in hand: the first dimension below vDefunct
   __shared__ int sFail;
   const int q = blockIdx.x, r = a.runMdl[q], t = threadIdx.x, D = a.p.g.D;
   const UnitModel m = a.mdl[r];
   const int incoming = a.mstatus[r];                       // k_hr_logp's 2226 (uniform: every thread reads the same word, nobody writes it before the last barrier)
   if (t == 0) sFail = 0;
   __syncthreads();
   if (!incoming && (a.uFlags & HTKAMD_UPTRANS))            // RestTransP: row i by one thread, from the fp64 sums rounded to float
      for (int i = 1 + t; i < m.N; i += HR_THREADS) {
         const float occi = ACCF(a.lay.trOcc, m.occ0 + i - 1);
         if (occi == 0.0f) { atomicCAS(&sFail, 0, HTKAMD_HREST_EZEROOCC); continue; }
         const double *tr = a.acc + a.lay.tr + (size_t)(m.tp0 + (i - 1) * m.N);
         unit_trans_row(a.p.transP + m.tp0 + (i - 1) * m.N, m.N, [tr](int j) { return (float)tr[j]; }, occi);
      }
   if (!incoming && (a.uFlags & (HTKAMD_UPMEANS | HTKAMD_UPVARS | HTKAMD_UPMIXES)))
      for (int s = 0; s < m.ne; s++) {                      // RestStream
         const int st = a.p.hmmState[m.st0 + s], c0 = a.p.g.stateCompOff[st], M = a.p.g.stateCompOff[st + 1] - c0;
         for (int k = t; k < M; k += HR_THREADS) firstBad[k] = D;
         if (a.uFlags & HTKAMD_UPMIXES) {                   // RestMixWeights
            const float occ = ACCF(a.lay.wtOcc, st);
            if (occ == 0.0f) { if (t == 0) atomicCAS(&sFail, 0, HTKAMD_HREST_EZEROOCC); }
            else if (M > 1)
               for (int k = t; k < M; k += HR_THREADS) {
                  float x = __fdiv_rn(ACCF(a.lay.wt, c0 + k), occ);
                  if (x > 1.0f) x = 1.0f;                   // (the fp64 sums of a component cannot exceed the state's but by their rounding to float)
                  a.p.compWeight[c0 + k] = ((double)x > MINMIX) ? x : 0.0f;
               }
         }
         __syncthreads();
         for (int e = t; e < M * D; e += HR_THREADS) {      // RestMean, RestCoVar: a thread per (component, dimension)
            const int k = e / D, d = e - k * D, g = a.p.g.compGauss[c0 + k];
            if (!((double)a.p.compWeight[c0 + k] > MINMIX)) continue;
            const size_t x = (size_t)g * D + d;
            const float old = a.p.mean[x];
            float nm = old;
            if (a.uFlags & HTKAMD_UPMEANS) {
               const float occ = ACCF(a.lay.muOcc, g);
               if (occ == 0.0f) { atomicCAS(&sFail, 0, HTKAMD_HREST_EZEROOCC); continue; }
               nm = __fadd_rn(old, __fdiv_rn(ACCF(a.lay.mu, x), occ));
               a.p.mean[x] = nm;
            }
            if (a.uFlags & HTKAMD_UPVARS) {
               const float occ = ACCF(a.lay.vaOcc, g);
               if (occ == 0.0f) { atomicCAS(&sFail, 0, HTKAMD_HREST_EZEROOCC); continue; }
               const float muDiff = __fsub_rn(nm, old);     // (0 without UPMEANS)
               float v = __fsub_rn(__fdiv_rn(ACCF(a.lay.va, x), occ), __fmul_rn(muDiff, muDiff));
               if (v < a.minVar) v = a.minVar;
               if (v < a.vDefunct) atomicMin(firstBad + k, d);
               a.p.g.gparam[(size_t)g * a.p.g.PS + 2 * d] = v;   // parked in the row that is rebuilt below: written once the component's first defunct dimension is known
            }
         }
         __syncthreads();
         if (a.uFlags & HTKAMD_UPVARS)
            for (int e = t; e < M * D; e += HR_THREADS) {
               const int k = e / D, d = e - k * D, g = a.p.g.compGauss[c0 + k];
               if (!((double)a.p.compWeight[c0 + k] > MINMIX)) continue;
               if (d < firstBad[k]) a.p.var[(size_t)g * D + d] = a.p.g.gparam[(size_t)g * a.p.g.PS + 2 * d];       // RestCoVar returns at the first one
            }
         __syncthreads();
         if (t == 0) {
            for (int k = 0; k < M; k++)
               if (firstBad[k] < D && (double)a.p.compWeight[c0 + k] > MINMIX) {
                  if (M > 1) a.p.compWeight[c0 + k] = 0.0f;   // "Defunct Mix"
                  else atomicCAS(&sFail, 0, HTKAMD_HREST_EZEROOCC);     // "Zero Covariance"
               }
            if (M > 1) {                                    // FloorMixes, whatever uFlags says (RestStream :1270)
               const float floor = a.mixWeightFloor;
               float sum = 0.0f, fsum = 0.0f;
               for (int k = 0; k < M; k++) {
                  if (a.p.compWeight[c0 + k] > floor) sum = __fadd_rn(sum, a.p.compWeight[c0 + k]);
                  else { fsum = __fadd_rn(fsum, floor); a.p.compWeight[c0 + k] = floor; }
               }
               if ((double)fsum > 1.0) atomicCAS(&sFail, 0, HTKAMD_HREST_EFLOORSUM);
               const float scale = (float)((1.0 - (double)fsum) / (double)sum);
               for (int k = 0; k < M; k++) if (a.p.compWeight[c0 + k] > floor) a.p.compWeight[c0 + k] = __fmul_rn(a.p.compWeight[c0 + k], scale);
            }
         }
         __syncthreads();
      }
   __syncthreads();
   const int fail = incoming ? incoming : sFail;
   if (fail) {                                              // the model keeps what it came with, whichever pass it failed in
      unit_restore<HR_THREADS>(a.p, m);
      if (t == 0) { a.mstatus[r] = fail; a.out[q].status = fail; }
   }
   __syncthreads();
   for (int s = 0; s < m.ne; s++) htkamd_derive_state(a.p.g, a.p.hmmState[m.st0 + s], HR_THREADS);
}

DEVBUF_OWNER("hrest")

extern "C" int htkamd_hrest(htkamd_model *m, const float *dX, int nFrames, int nTokens, const int *tokFrame, const int *tokLen, const int *tokModel,
                            const htkamd_hrest_config *cfg, int nModels, const int *models,
                            int *status, int *nPass, int *converged, float *logP, int *nUsed, void *stream)
{
   if (!m || !cfg || !status || !nPass || !converged || !logP || !nUsed) { htkamd_set_error("hrest: NULL argument"); return HTKAMD_EINVAL; }
   int rc;
   htkamd_model_desc d;
   if ((rc = unit_refuse_handle(m, "hrest", "HRest", &d)) || (rc = htkamd_hrest_check(&d, nFrames, nTokens, tokFrame, tokLen, tokModel, cfg, nModels, models))) return rc;
   if (!dX && nTokens > 0) { htkamd_set_error("hrest: no feature table"); return HTKAMD_EINVAL; }
   if (htkamd_device_count() <= 0) { htkamd_set_error("hrest: no HIP device"); return HTKAMD_ENODEV; }
   hipStream_t s = (hipStream_t)stream;
   const int D = m->D, maxIter = cfg->maxIter;
   for (int k = 0; k < nModels; k++) { nPass[k] = 0; converged[k] = 0; }
   for (size_t i = 0; i < (size_t)nModels * maxIter; i++) { logP[i] = 0.0f; nUsed[i] = 0; }

   // ---- short-token rejection and the -m test, once; the kept tokens of the models that go on, behind one another per model
   std::vector<int> keep((size_t)(nTokens ? nTokens : 1)), nKept((size_t)nModels);
   if ((rc = htkamd_hrest_token_counts(m->h_hmmStateOff, m->H, nTokens, tokLen, tokModel, cfg, nModels, models, keep.data(), nKept.data(), status))) return rc;
   UnitTables tb;
   int maxM = 1;
   rc = unit_tables("hrest", m, nTokens, tokFrame, tokLen, tokModel, keep.data(), nModels, models,
      [&](int k, int, const std::vector<int> &) { return status[k] == HTKAMD_HREST_OK; },
      [&](UnitModel &x, int) -> int {                          // the widest state: k_hr_update's LDS
         for (int j = 0; j < x.ne; j++) {
            const int st = m->h_hmmState[x.st0 + j], M = m->h_stateCompOff[st + 1] - m->h_stateCompOff[st];
            if (M > maxM) maxM = M;
         }
         return HTKAMD_OK;
      }, tb);
   if (rc || tb.mdl.empty()) return rc;
   const std::vector<UnitModel> &mdl = tb.mdl;
   const std::vector<int> &mdlOf = tb.mdlOf, &aLen = tb.aLen;
   const long long totFrames = tb.totFrames;
   const int nMdl = (int)mdl.size(), nTok = (int)aLen.size();

   htkamd_fb *fb = nullptr; htkamd_accs *accs = nullptr;
   struct Guard { htkamd_fb *&f; htkamd_accs *&a; ~Guard() { if (f) htkamd_fb_destroy(f); if (a) htkamd_accs_destroy(a); } } guard{fb, accs};
   if ((rc = htkamd_fb_create(m, &fb)) || (rc = htkamd_accs_create(m, &accs)) || (rc = htkamd_accs_zero(accs, s))) return rc;

   DevBuf bMdl, bTokFrame, bTokLen, bTokMdl, bRunFlag, bUTok, bUFrame0, bMdlUtt0, bNUtt, bRun, bMstatus, bBak, bXg, bOut;
   const size_t nM = (size_t)nMdl;
   if ((rc = bMdl.upload(mdl, s)) || (rc = bTokFrame.upload(tb.aFrame, s)) || (rc = bTokLen.upload(aLen, s)) || (rc = bTokMdl.upload(tb.aMdl, s)) ||
       (rc = bRunFlag.reserve<int>(nM)) || (rc = bUTok.reserve<int>((size_t)nTok)) || (rc = bUFrame0.reserve<int>((size_t)nTok + 1)) ||
       (rc = bMdlUtt0.reserve<int>(nM)) || (rc = bNUtt.reserve<int>(2)) || (rc = bRun.reserve<int>(nM)) ||
       (rc = bMstatus.reserve<int>(nM)) || (rc = bXg.reserve<float>((size_t)totFrames * D)) || (rc = bOut.reserve<HrOut>(nM)))
      return rc;
   HIPCHECK(hipMemsetAsync(bMstatus.p, 0, sizeof(int) * nM, s));
   HrArgs a;
   memset(&a, 0, sizeof(a));
   if ((rc = unit_snapshot(m, bBak, s, &a.p))) return rc;      // the snapshot a failed model is put back to
   a.uFlags = cfg->uFlags; a.minVar = cfg->minVar; a.vDefunct = cfg->vDefunct; a.mixWeightFloor = cfg->mixWeightFloor;
   a.acc = accs->d_vec; a.lay = accs->lay;
   a.X = dX; a.Xg = bXg.as<float>(); a.mdl = bMdl.as<const UnitModel>(); a.nMdl = nMdl;
   a.tokFrame = bTokFrame.as<const int>(); a.tokLen = bTokLen.as<const int>(); a.tokMdl = bTokMdl.as<const int>(); a.nTok = nTok;
   a.runFlag = bRunFlag.as<const int>(); a.uTok = bUTok.as<int>(); a.uFrame0 = bUFrame0.as<int>(); a.mdlUtt0 = bMdlUtt0.as<int>(); a.nUttOut = bNUtt.as<int>();
   a.runMdl = bRun.as<const int>(); a.mstatus = bMstatus.as<int>(); a.out = bOut.as<HrOut>();

   htkamd_fb_config fc;
   memset(&fc, 0, sizeof(fc));                              // HRest prunes nothing: no beam, and every state posterior counts
   fc.pruneInit = HTKAMD_NOPRUNE; fc.pruneInc = 0.0; fc.pruneLim = HTKAMD_NOPRUNE; fc.minFrwdP = 700.0f;
   fc.uFlags = HTKAMD_UPMEANS | HTKAMD_UPVARS | HTKAMD_UPTRANS | HTKAMD_UPMIXES; fc.scoreMode = HTKAMD_SCORE_SOUTP | HTKAMD_SCORE_DIAGC;

   // ---- ReEstimateModel's passes
   std::vector<int> running((size_t)nMdl), next, runFlag, iter((size_t)nMdl, 0), frameOff, labOff, labs;
   std::vector<float> oldP((size_t)nMdl, (float)LZERO);
   std::vector<HrOut> out((size_t)nMdl);
   for (int r = 0; r < nMdl; r++) running[r] = r;
   bool changed = true;
   auto passes = [&]() -> int {
      while (!running.empty()) {
         const int nRun = (int)running.size();
         if (changed) {                                        // the batch of the models still running
            // INVARIANT shared with k_hr_compact: utterance u is the u-th kept token of a running model in the order of the token arrays
            // (models in the order of `mdl`, which `running` keeps; within a model the given order).  The host lays that order out for
            // htkamd_fb_prepare, which needs the offsets here; the device lists the same tokens for the gather and for k_hr_logp
            runFlag.assign((size_t)nMdl, 0);
            frameOff.assign(1, 0); labs.clear();
            for (int r : running) {
               runFlag[r] = 1;
               for (int k = mdl[r].tok0; k < mdl[r].tok0 + mdl[r].nTok; k++) { frameOff.push_back(frameOff.back() + aLen[k]); labs.push_back(mdl[r].h); }
            }
            const int nU = (int)labs.size();
            labOff.resize((size_t)nU + 1);
            for (int u = 0; u <= nU; u++) labOff[u] = u;
            if ((rc = bRunFlag.upload(runFlag, s)) || (rc = bRun.upload(running, s))) return rc;
            a.nRun = nRun;
            hipLaunchKernelGGL(k_hr_compact, dim3(1), dim3(HR_THREADS), 0, s, a);
            hipLaunchKernelGGL(k_hr_gather, dim3((unsigned)nU), dim3(HR_THREADS), 0, s, a);
            HIPCHECK(hipGetLastError());
            int onDev[2];                                       // the two lists agree in utterances and frames, or the call ends
            if ((rc = bNUtt.download(onDev, 2, s))) return rc;
            HIPCHECK(hipStreamSynchronize(s));
            if (onDev[0] != nU || onDev[1] != frameOff.back()) {
               htkamd_set_error("hrest: the device lists %d running tokens of %d frames, the host %d of %d", onDev[0], onDev[1], nU, frameOff.back());
               return HTKAMD_EINVAL;
            }
            htkamd_batch_desc b;
            b.nUtt = nU; b.dX = a.Xg; b.frameOff = frameOff.data(); b.labOff = labOff.data(); b.labs = labs.data();
            if ((rc = htkamd_fb_prepare(fb, &b, s))) return rc;
            htkamd_fb_dev fr;
            if ((rc = htkamd_fb_device_results(fb, &fr))) return rc;
            a.pr = fr.pr; a.uttStatus = fr.status;
            changed = false;
         }
         hipLaunchKernelGGL(k_hr_zero, dim3((unsigned)nRun), dim3(HR_THREADS), 0, s, a);
         HIPCHECK(hipGetLastError());
         if ((rc = htkamd_fb_execute(fb, &fc, accs, s))) return rc;
         hipLaunchKernelGGL(k_hr_logp, dim3((unsigned)((nRun + 63) / 64)), dim3(64), 0, s, a);
         hipLaunchKernelGGL(k_hr_update, dim3((unsigned)nRun), dim3(HR_THREADS), sizeof(int) * (size_t)maxM, s, a);
         HIPCHECK(hipGetLastError());
         if ((rc = bOut.download(out.data(), (size_t)nRun, s))) return rc;
         HIPCHECK(hipStreamSynchronize(s));
         next.clear();
         for (int q = 0; q < nRun; q++) {
            const int r = running[q], k = mdlOf[r];
            if (out[q].status != HTKAMD_HREST_OK) { status[k] = out[q].status; converged[k] = 0; changed = true; continue; }
            const int it = ++iter[r];
            const float newP = out[q].sum / (float)out[q].used;
            const float delta = newP - oldP[r];
            oldP[r] = newP;
            logP[(size_t)k * maxIter + it - 1] = newP; nUsed[(size_t)k * maxIter + it - 1] = out[q].used; nPass[k] = it;
            if (fabs((double)delta) < (double)cfg->epsilon) { converged[k] = 1; changed = true; }
            else if (it < maxIter) next.push_back(r);
            else changed = true;
         }
         running.swap(next);
      }
      return HTKAMD_OK;
   };
   const int rcPass = passes();
   if (rcPass) {
      // a call that ends in an error leaves no model half re-estimated: every model of the call goes back to its snapshot (as far as the
      // device still answers), then the mirror follows as below and the error is returned; status / nPass / logP are then undefined
      hipLaunchKernelGGL(k_unit_restore<HR_THREADS>, dim3((unsigned)nMdl), dim3(HR_THREADS), 0, s, a.p, a.mdl, (const int *)nullptr);
      (void)hipGetLastError();
   }
   rc = unit_finish(m, s);                                  // the host mirror and the derived tables follow
   return rcPass ? rcPass : rc;
}
