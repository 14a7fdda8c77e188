/* unit_train.c -- what htkamd_hinit and htkamd_hrest (csrc/hinit.hip, csrc/hrest.hip) both refuse before a device is touched; the tools'
 * own host sides are hinit.c and hrest.c.  Pure C, no device.  pfx / tool: "hinit" / "HInit" or "hrest" / "HRest", as the messages name them.
 *   isolation             either tool loads ONE model (MakeOneHMM HInit.c:337, HRest.c:351); here the models of a call must not use a state,
 *                         a Gaussian or a transition matrix twice, or the result would depend on the order they are trained in
 */
#include <stdlib.h>
#include <string.h>
#include "../csrc/internal.h"

int htkamd_unit_check(const char *pfx, const char *tool, const htkamd_model_desc *d, int nFrames, int nTokens, const int *tokFrame, const int *tokLen,
                      const int *tokModel, const htkamd_unit_cfg *cfg, int nModels, const int *models)
{
   const int hrest = strcmp(pfx, "hrest") == 0;
   int k, j, c, t, rc = HTKAMD_OK;
   unsigned char *usedH = NULL, *usedS = NULL, *usedG = NULL, *usedT = NULL;
   if (!d || !cfg || nModels < 1 || !models || nTokens < 0 || (nTokens > 0 && (!tokFrame || !tokLen || !tokModel)) || nFrames < 0) {
      htkamd_set_error("%s: bad argument", pfx); return HTKAMD_EINVAL;
   }
   if (!d->var) { htkamd_set_error("%s: a FULLC set (%s on full covariances is not supported)", pfx, tool); return HTKAMD_EMODEL; }
   /* HRest alone names the switch that only means something on such a set */
   if (d->hsKind == HTKAMD_HS_TIED) { htkamd_set_error("%s: a tied-mixture set (%s on TIEDHS sets%s is not supported)", pfx, tool, hrest ? ", the -c threshold," : ""); return HTKAMD_EMODEL; }
   /* HRest alone refuses the remaining kinds here; HInit has no twin of this */
   if (hrest && d->hsKind != HTKAMD_HS_PLAIN) { htkamd_set_error("%s: a discrete set (hsKind %d; continuous densities only)", pfx, d->hsKind); return HTKAMD_EMODEL; }
   if (d->numStreams > 1) { htkamd_set_error("%s: a set of %d streams (one stream only)", pfx, d->numStreams); return HTKAMD_EMODEL; }
   if (cfg->maxIter < 1 || cfg->minSeg < 1) { htkamd_set_error("%s: maxIter %d, minSeg %d (both at least 1)", pfx, cfg->maxIter, cfg->minSeg); return HTKAMD_EINVAL; }
   if (cfg->uFlags & ~(HTKAMD_UPMEANS | HTKAMD_UPVARS | HTKAMD_UPTRANS | HTKAMD_UPMIXES)) { htkamd_set_error("%s: update flags %d (-u takes t, m, v, w)", pfx, cfg->uFlags); return HTKAMD_EINVAL; }
   usedH = (unsigned char *)calloc((size_t)d->numPhys + 1, 1); usedS = (unsigned char *)calloc((size_t)d->numStates + 1, 1);
   usedG = (unsigned char *)calloc((size_t)d->numGauss + 1, 1); usedT = (unsigned char *)calloc((size_t)d->numTrans + 1, 1);
   if (!usedH || !usedS || !usedG || !usedT) { htkamd_set_error("%s: out of memory", pfx); rc = HTKAMD_ENOMEM; }
   for (k = 0; k < nModels && !rc; k++) {
      const int h = models[k];
      if (h < 0 || h >= d->numPhys) { htkamd_set_error("%s: model %d of the list names physical model %d of %d", pfx, k, h, d->numPhys); rc = HTKAMD_EINVAL; break; }
      if (usedH[h]) { htkamd_set_error("%s: physical model %d is named twice in the list", pfx, h); rc = HTKAMD_EINVAL; break; }
      usedH[h] = 1;
      t = d->hmmTrans[h];
      if (usedT[t]) { htkamd_set_error("%s: transition matrix %d is shared by models to be trained (model %d): %s trains in isolation", pfx, t, h, tool); rc = HTKAMD_EMODEL; break; }
      usedT[t] = 1;
      for (j = d->hmmStateOff[h]; j < d->hmmStateOff[h + 1] && !rc; j++) {
         const int s = d->hmmState[j];
         if (usedS[s]) { htkamd_set_error("%s: state %d is shared by models to be trained (model %d): %s trains in isolation", pfx, s, h, tool); rc = HTKAMD_EMODEL; break; }
         usedS[s] = 1;
         for (c = d->stateCompOff[s]; c < d->stateCompOff[s + 1]; c++) {
            const int g = d->compGauss[c];
            if (usedG[g]) { htkamd_set_error("%s: Gaussian %d is shared by models to be trained (model %d): %s trains in isolation", pfx, g, h, tool); rc = HTKAMD_EMODEL; break; }
            usedG[g] = 1;
         }
      }
   }
   for (k = 0; k < nTokens && !rc; k++) {
      if (tokModel[k] < 0 || tokModel[k] >= d->numPhys) { htkamd_set_error("%s: token %d names physical model %d of %d", pfx, k, tokModel[k], d->numPhys); rc = HTKAMD_EINVAL; break; }
      if (tokLen[k] < 1 || tokFrame[k] < 0 || (long long)tokFrame[k] + tokLen[k] > nFrames) {
         htkamd_set_error("%s: token %d (frames %d .. %lld) lies outside the table of %d frames", pfx, k, tokFrame[k], (long long)tokFrame[k] + tokLen[k] - 1, nFrames);
         rc = HTKAMD_EINVAL; break;
      }
   }
   free(usedH); free(usedS); free(usedG); free(usedT);
   return rc;
}
