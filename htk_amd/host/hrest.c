/* hrest.c -- the host side of htkamd_hrest (csrc/hrest.hip): everything that is refused before a device is touched, and the token
 * bookkeeping that needs no device.  Pure C, no device.
 *   HRest's own checks    main HRest.c:228 (-m), :295 (too few examples), LoadFile :500 (short segments), Initialise1 :356
 *   isolation             HRest loads ONE model (MakeOneHMM :351); here the models of a call must not use a state, a Gaussian or a
 *                         transition matrix twice, or the result would depend on the order they are trained in
 */
#include <stdlib.h>
#include <string.h>
#include "../csrc/internal.h"

int htkamd_hrest_check(const htkamd_model_desc *d, int nFrames, int nTokens, const int *tokFrame, const int *tokLen, const int *tokModel,
                       const htkamd_hrest_config *cfg, int nModels, const int *models)
{
   int k, j, c, t, rc = HTKAMD_OK;
   unsigned char *usedH = NULL, *usedS = NULL, *usedG = NULL, *usedT = NULL;
   if (!d || !cfg || nModels < 1 || !models || nTokens < 0 || (nTokens > 0 && (!tokFrame || !tokLen || !tokModel)) || nFrames < 0) {
      htkamd_set_error("hrest: bad argument"); return HTKAMD_EINVAL;
   }
   if (!d->var) { htkamd_set_error("hrest: a FULLC set (HRest on full covariances is not supported)"); return HTKAMD_EMODEL; }
   if (d->hsKind == HTKAMD_HS_TIED) { htkamd_set_error("hrest: a tied-mixture set (HRest on TIEDHS sets, the -c threshold, is not supported)"); return HTKAMD_EMODEL; }
   if (d->hsKind != HTKAMD_HS_PLAIN) { htkamd_set_error("hrest: a discrete set (hsKind %d; continuous densities only)", d->hsKind); return HTKAMD_EMODEL; }
   if (d->numStreams > 1) { htkamd_set_error("hrest: a set of %d streams (one stream only)", d->numStreams); return HTKAMD_EMODEL; }
   if (cfg->maxIter < 1 || cfg->minSeg < 1) { htkamd_set_error("hrest: maxIter %d, minSeg %d (both at least 1)", cfg->maxIter, cfg->minSeg); return HTKAMD_EINVAL; }
   if (cfg->uFlags & ~(HTKAMD_UPMEANS | HTKAMD_UPVARS | HTKAMD_UPTRANS | HTKAMD_UPMIXES)) { htkamd_set_error("hrest: update flags %d (-u takes t, m, v, w)", cfg->uFlags); return HTKAMD_EINVAL; }
   usedH = (unsigned char *)calloc((size_t)d->numPhys + 1, 1); usedS = (unsigned char *)calloc((size_t)d->numStates + 1, 1);
   usedG = (unsigned char *)calloc((size_t)d->numGauss + 1, 1); usedT = (unsigned char *)calloc((size_t)d->numTrans + 1, 1);
   if (!usedH || !usedS || !usedG || !usedT) { htkamd_set_error("hrest: out of memory"); rc = HTKAMD_ENOMEM; }
   for (k = 0; k < nModels && !rc; k++) {
      const int h = models[k];
      if (h < 0 || h >= d->numPhys) { htkamd_set_error("hrest: model %d of the list names physical model %d of %d", k, h, d->numPhys); rc = HTKAMD_EINVAL; break; }
      if (usedH[h]) { htkamd_set_error("hrest: physical model %d is named twice in the list", h); rc = HTKAMD_EINVAL; break; }
      usedH[h] = 1;
      t = d->hmmTrans[h];
      if (usedT[t]) { htkamd_set_error("hrest: transition matrix %d is shared by models to be trained (model %d): HRest trains in isolation", t, h); rc = HTKAMD_EMODEL; break; }
      usedT[t] = 1;
      for (j = d->hmmStateOff[h]; j < d->hmmStateOff[h + 1] && !rc; j++) {
         const int s = d->hmmState[j];
         if (usedS[s]) { htkamd_set_error("hrest: state %d is shared by models to be trained (model %d): HRest trains in isolation", s, h); rc = HTKAMD_EMODEL; break; }
         usedS[s] = 1;
         for (c = d->stateCompOff[s]; c < d->stateCompOff[s + 1]; c++) {
            const int g = d->compGauss[c];
            if (usedG[g]) { htkamd_set_error("hrest: Gaussian %d is shared by models to be trained (model %d): HRest trains in isolation", g, h); rc = HTKAMD_EMODEL; break; }
            usedG[g] = 1;
         }
      }
   }
   for (k = 0; k < nTokens && !rc; k++) {
      if (tokModel[k] < 0 || tokModel[k] >= d->numPhys) { htkamd_set_error("hrest: token %d names physical model %d of %d", k, tokModel[k], d->numPhys); rc = HTKAMD_EINVAL; break; }
      if (tokLen[k] < 1 || tokFrame[k] < 0 || (long long)tokFrame[k] + tokLen[k] > nFrames) {
         htkamd_set_error("hrest: token %d (frames %d .. %lld) lies outside the table of %d frames", k, tokFrame[k], (long long)tokFrame[k] + tokLen[k] - 1, nFrames);
         rc = HTKAMD_EINVAL; break;
      }
   }
   free(usedH); free(usedS); free(usedG); free(usedT);
   return rc;
}

int htkamd_hrest_token_counts(const int *hmmStateOff, int numPhys, int nTokens, const int *tokLen, const int *tokModel, const htkamd_hrest_config *cfg,
                              int nModels, const int *models, int *keep, int *nKept, int *status)
{
   int k, *ofPhys;
   if (!hmmStateOff || numPhys < 1 || !cfg || nModels < 1 || !models || !nKept || !status || nTokens < 0 || (nTokens > 0 && (!tokLen || !tokModel))) {
      htkamd_set_error("hrest_token_counts: bad argument"); return HTKAMD_EINVAL;
   }
   ofPhys = (int *)malloc(sizeof(int) * (size_t)numPhys);
   if (!ofPhys) { htkamd_set_error("hrest: out of memory"); return HTKAMD_ENOMEM; }
   for (k = 0; k < numPhys; k++) ofPhys[k] = -1;
   for (k = 0; k < nModels; k++) {
      if (models[k] < 0 || models[k] >= numPhys) { free(ofPhys); htkamd_set_error("hrest_token_counts: model %d of the list names physical model %d of %d", k, models[k], numPhys); return HTKAMD_EINVAL; }
      ofPhys[models[k]] = k; nKept[k] = 0;
   }
   for (k = 0; k < nTokens; k++) {
      const int h = tokModel[k];
      const int q = (h >= 0 && h < numPhys) ? ofPhys[h] : -1;
      /* LoadFile HRest.c:500: a segment shorter than the model's emitting states is skipped unless -t */
      const int ok = q >= 0 && (!cfg->segReject || tokLen[k] >= hmmStateOff[h + 1] - hmmStateOff[h]);
      if (keep) keep[k] = ok;
      if (ok) nKept[q]++;
   }
   for (k = 0; k < nModels; k++) status[k] = nKept[k] < cfg->minSeg ? HTKAMD_HREST_EFEWSEGS : HTKAMD_HREST_OK;      /* main :295 */
   free(ofPhys);
   return HTKAMD_OK;
}
