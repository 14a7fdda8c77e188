/* hrest.c -- the host side of htkamd_hrest (csrc/hrest.hip): everything that is refused before a device is touched (the checks HInit
 * shares, isolation among them: unit_train.c), and the token bookkeeping that needs no device.  Pure C, no device.
 *   HRest's own checks    main HRest.c:228 (-m), :295 (too few examples), LoadFile :500 (short segments), Initialise1 :356
 */
#include <stdlib.h>
#include <string.h>
#include "../csrc/internal.h"

int htkamd_hrest_check(const htkamd_model_desc *d, int nFrames, int nTokens, const int *tokFrame, const int *tokLen, const int *tokModel,
                       const htkamd_hrest_config *cfg, int nModels, const int *models)
{
   const htkamd_unit_cfg c = { cfg ? cfg->maxIter : 0, cfg ? cfg->minSeg : 0, cfg ? cfg->uFlags : 0 };
   return htkamd_unit_check("hrest", "HRest", d, nFrames, nTokens, tokFrame, tokLen, tokModel, cfg ? &c : NULL, nModels, models);
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
