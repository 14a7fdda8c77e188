/* hinit.c -- the host side of htkamd_hinit (csrc/hinit.hip): everything that is refused before a device is touched, and the host twin
 * of the pool listing.  Pure C, no device.
 *   HInit's own checks    Initialise HInit.c:342 (discrete / tied-mixture sets), main :276 (-m), UCollectData :516
 *   isolation             HInit loads ONE model (MakeOneHMM :337); here the models of a call must not use a state, a Gaussian or a
 *                         transition matrix twice, or the result would depend on the order they are trained in
 */
#include <stdlib.h>
#include <string.h>
#include "../csrc/internal.h"
#include "../csrc/hinit_seg.h"

int htkamd_hinit_check(const htkamd_model_desc *d, int nFrames, int nTokens, const int *tokFrame, const int *tokLen, const int *tokModel,
                       const htkamd_hinit_config *cfg, int nModels, const int *models)
{
   int k, j, c, t, rc = HTKAMD_OK;
   unsigned char *usedH = NULL, *usedS = NULL, *usedG = NULL, *usedT = NULL;
   if (!d || !cfg || nModels < 1 || !models || nTokens < 0 || (nTokens > 0 && (!tokFrame || !tokLen || !tokModel)) || nFrames < 0) {
      htkamd_set_error("hinit: bad argument"); return HTKAMD_EINVAL;
   }
   if (!d->var) { htkamd_set_error("hinit: a FULLC set (HInit on full covariances is not supported)"); return HTKAMD_EMODEL; }
   if (d->hsKind == HTKAMD_HS_TIED) { htkamd_set_error("hinit: a tied-mixture set (HInit on TIEDHS sets is not supported)"); return HTKAMD_EMODEL; }
   if (d->numStreams > 1) { htkamd_set_error("hinit: a set of %d streams (one stream only)", d->numStreams); return HTKAMD_EMODEL; }
   if (cfg->maxIter < 1 || cfg->minSeg < 1) { htkamd_set_error("hinit: maxIter %d, minSeg %d (both at least 1)", cfg->maxIter, cfg->minSeg); return HTKAMD_EINVAL; }
   if (cfg->uFlags & ~(HTKAMD_UPMEANS | HTKAMD_UPVARS | HTKAMD_UPTRANS | HTKAMD_UPMIXES)) { htkamd_set_error("hinit: update flags %d (-u takes t, m, v, w)", cfg->uFlags); return HTKAMD_EINVAL; }
   usedH = (unsigned char *)calloc((size_t)d->numPhys + 1, 1); usedS = (unsigned char *)calloc((size_t)d->numStates + 1, 1);
   usedG = (unsigned char *)calloc((size_t)d->numGauss + 1, 1); usedT = (unsigned char *)calloc((size_t)d->numTrans + 1, 1);
   if (!usedH || !usedS || !usedG || !usedT) { htkamd_set_error("hinit: out of memory"); rc = HTKAMD_ENOMEM; }
   for (k = 0; k < nModels && !rc; k++) {
      const int h = models[k];
      if (h < 0 || h >= d->numPhys) { htkamd_set_error("hinit: model %d of the list names physical model %d of %d", k, h, d->numPhys); rc = HTKAMD_EINVAL; break; }
      if (usedH[h]) { htkamd_set_error("hinit: physical model %d is named twice in the list", h); rc = HTKAMD_EINVAL; break; }
      usedH[h] = 1;
      t = d->hmmTrans[h];
      if (usedT[t]) { htkamd_set_error("hinit: transition matrix %d is shared by models to be trained (model %d): HInit trains in isolation", t, h); rc = HTKAMD_EMODEL; break; }
      usedT[t] = 1;
      for (j = d->hmmStateOff[h]; j < d->hmmStateOff[h + 1] && !rc; j++) {
         const int s = d->hmmState[j];
         if (usedS[s]) { htkamd_set_error("hinit: state %d is shared by models to be trained (model %d): HInit trains in isolation", s, h); rc = HTKAMD_EMODEL; break; }
         usedS[s] = 1;
         for (c = d->stateCompOff[s]; c < d->stateCompOff[s + 1]; c++) {
            const int g = d->compGauss[c];
            if (usedG[g]) { htkamd_set_error("hinit: Gaussian %d is shared by models to be trained (model %d): HInit trains in isolation", g, h); rc = HTKAMD_EMODEL; break; }
            usedG[g] = 1;
         }
      }
   }
   for (k = 0; k < nTokens && !rc; k++) {
      if (tokModel[k] < 0 || tokModel[k] >= d->numPhys) { htkamd_set_error("hinit: token %d names physical model %d of %d", k, tokModel[k], d->numPhys); rc = HTKAMD_EINVAL; break; }
      if (tokLen[k] < 1 || tokFrame[k] < 0 || (long long)tokFrame[k] + tokLen[k] > nFrames) {
         htkamd_set_error("hinit: token %d (frames %d .. %lld) lies outside the table of %d frames", k, tokFrame[k], (long long)tokFrame[k] + tokLen[k] - 1, nFrames);
         rc = HTKAMD_EINVAL; break;
      }
   }
   free(usedH); free(usedS); free(usedG); free(usedT);
   return rc;
}

int htkamd_hinit_uniform_states(int nEmit, int nTokens, const int *tokLen, int *state)
{
   int k, j, at = 0;
   if (nEmit < 1 || nTokens < 0 || (nTokens > 0 && (!tokLen || !state))) { htkamd_set_error("hinit_uniform_states: bad argument"); return HTKAMD_EINVAL; }
   for (k = 0; k < nTokens; k++) {
      if (tokLen[k] < nEmit) { htkamd_set_error("hinit_uniform_states: token %d has %d frames for %d emitting states (UCollectData: segment too short)", k, tokLen[k], nEmit); return HTKAMD_EINVAL; }
      for (j = 0; j < tokLen[k]; j++) state[at++] = htkamd_hinit_state_of(j, tokLen[k], nEmit);
   }
   return HTKAMD_OK;
}
