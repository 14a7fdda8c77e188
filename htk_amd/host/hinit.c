/* hinit.c -- the host side of htkamd_hinit (csrc/hinit.hip): everything that is refused before a device is touched (the checks HRest
 * shares, isolation among them: unit_train.c), and the host twin of the pool listing.  Pure C, no device.
 *   HInit's own checks    Initialise HInit.c:342 (discrete / tied-mixture sets), main :276 (-m), UCollectData :516
 */
#include <stdlib.h>
#include <string.h>
#include "../csrc/internal.h"
#include "../csrc/hinit_seg.h"

int htkamd_hinit_check(const htkamd_model_desc *d, int nFrames, int nTokens, const int *tokFrame, const int *tokLen, const int *tokModel,
                       const htkamd_hinit_config *cfg, int nModels, const int *models)
{
   const htkamd_unit_cfg c = { cfg ? cfg->maxIter : 0, cfg ? cfg->minSeg : 0, cfg ? cfg->uFlags : 0 };
   return htkamd_unit_check("hinit", "HInit", d, nFrames, nTokens, tokFrame, tokLen, tokModel, cfg ? &c : NULL, nModels, models);
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
