/* frontend_geom_sanitize.c -- stand-alone driver (TEST INFRASTRUCTURE) for the host C of the waveform front end, meant to be built with
 * -fsanitize=address,undefined together with htk_amd/host/fbank.c and oracle/orc_mfcc.c (tests/test_frontend_geometry.py does that).
 *
 * Reads one front-end configuration per line from the file named on the command line:
 *    name baseKind sampPeriod winDur frPeriod numChans numCeps cepLifter preEmph useHam usePower zMeanSource rawEnergy eNormalise
 *    loFreq hiFreq hasC0 hasE hasD hasA hasZ delWin accWin lpcOrder compressFact nSamples
 * and for each of them
 *   - builds the tables (htkamd_frontend_tables_build) and reads every table over exactly the extent that fe_create copies to the
 *     device, so that a table built one element short, or copied one element long, is a sanitizer report;
 *   - checks what the kernels index LDS with: the bit-reversal table, the band klo..khi and every filter's two k ranges;
 *   - MFCC: runs the oracle's restatement (orc_mfcc) on nSamples of noise.
 * Prints "OK <n>" and returns 0 when all lines passed.
 */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../htk_amd/csrc/internal.h"
#include "../oracle/htk_oracle.h"

static char g_err[1024];
void htkamd_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }

#define FAIL(...) do { fprintf(stderr, "%s: ", name); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

static volatile double g_sink;
#define READ_ALL(p, n) do { size_t i_; for (i_ = 0; i_ < (size_t)(n); i_++) g_sink += (double)(p)[i_]; } while (0)

static int one(const char *name, const htkamd_frontend_config *fc, int nSamples)
{
   const htkamd_mfcc_config *c = &fc->base;
   struct htkamd_mfcc_tables t;
   int nn, b, i, k;
   const int nCep = (fc->baseKind == 6 || fc->baseKind == 11) ? c->numCeps : 0, nDct = (fc->baseKind == 6) ? c->numCeps : 0;
   if (htkamd_frontend_tables_build(fc, &t) != HTKAMD_OK) FAIL("tables_build refused: %s", g_err);
   nn = t.fftN / 2;
   if (t.frSize > t.fftN || (t.fftN > 2 && t.frSize <= t.fftN / 2)) FAIL("fftN %d is not the power of two at or above frSize %d", t.fftN, t.frSize);
   /* the extents of fe_create's copies (csrc/mfcc.hip) */
   READ_ALL(t.ham, t.frSize + 1); READ_ALL(t.cepWin, nCep + 1); READ_ALL(t.loWt, nn + 2); READ_ALL(t.binA0, 4 * (c->numChans + 2));
   READ_ALL(t.dct, (size_t)(nDct + 1) * (c->numChans + 1)); READ_ALL(t.tw, 2 * nn); READ_ALL(t.rtw, 2 * (nn / 2 + 2)); READ_ALL(t.brev, nn);
   if (fc->baseKind == 11) { READ_ALL(t.eql, c->numChans + 1); READ_ALL(t.cm, (size_t)(fc->lpcOrder + 1) * (c->numChans + 2)); }
   /* the kernels' LDS indices: xs[2 brev[c]] for c < nn; xs[2k - 2], uk[k], vk[k] for klo <= k <= khi and for the filters' ranges */
   {
      char *seen = (char *)calloc((size_t)nn, 1);
      for (i = 0; i < nn; i++) {
         if (t.brev[i] < 0 || t.brev[i] >= nn || seen[t.brev[i]]) { free(seen); FAIL("brev[%d] = %d is no permutation of 0..%d", i, t.brev[i], nn - 1); }
         seen[t.brev[i]] = 1;
      }
      free(seen);
   }
   if (t.klo < 2 || t.khi > nn) FAIL("band %d..%d outside 2..%d", t.klo, t.khi, nn);
   for (b = 1; b <= c->numChans; b++) {
      if (t.binA0[b] <= t.binA1[b] && (t.binA0[b] < t.klo || t.binA1[b] > t.khi)) FAIL("filter %d: range A %d..%d outside the band", b, t.binA0[b], t.binA1[b]);
      if (t.binB0[b] <= t.binB1[b] && (t.binB0[b] < t.klo || t.binB1[b] > t.khi)) FAIL("filter %d: range B %d..%d outside the band", b, t.binB0[b], t.binB1[b]);
   }
   for (k = t.klo; k <= t.khi; k++) if (!(t.loWt[k] >= 0.0f && t.loWt[k] <= 1.0f)) FAIL("loWt[%d] = %g", k, (double)t.loWt[k]);
   if (htkamd_mfcc_num_frames(c, nSamples) < 1) FAIL("%d samples hold no frame", nSamples);
   htkamd_mfcc_tables_free(&t);
   if (fc->baseKind == 6) {
      orc_mfcc_cfg oc;
      short *w = (short *)malloc(sizeof(short) * (size_t)nSamples);
      float *out;
      unsigned s = 12345u;
      int T;
      memcpy(&oc, c, sizeof(oc));                    /* the two configurations have the same members in the same order */
      for (i = 0; i < nSamples; i++) { s = s * 1664525u + 1013904223u; w[i] = (short)((int)(s >> 18) - 8192); }
      T = orc_mfcc_frames(nSamples, &oc, NULL, NULL);
      if (T != htkamd_mfcc_num_frames(c, nSamples)) { free(w); FAIL("oracle counts %d frames", T); }
      out = (float *)malloc(sizeof(float) * (size_t)T * orc_mfcc_cols(&oc));
      if (orc_mfcc(w, nSamples, &oc, out) != T) { free(w); free(out); FAIL("oracle coded another number of frames"); }
      READ_ALL(out, (size_t)T * orc_mfcc_cols(&oc));
      free(w); free(out);
   }
   return 0;
}

int main(int argc, char **argv)
{
   FILE *f;
   char name[64];
   int n = 0, bad = 0, nSamples;
   htkamd_frontend_config fc;
   _Static_assert(sizeof(orc_mfcc_cfg) == sizeof(htkamd_mfcc_config), "orc_mfcc_cfg mirrors htkamd_mfcc_config");
   if (argc != 2 || !(f = fopen(argv[1], "r"))) { fprintf(stderr, "usage: %s <cases file>\n", argv[0]); return 2; }
   for (;;) {
      htkamd_mfcc_config *c = &fc.base;
      memset(&fc, 0, sizeof(fc));
      if (fscanf(f, "%63s %d %lf %lf %lf %d %d %d %f %d %d %d %d %d %f %f %d %d %d %d %d %d %d %d %f %d", name, &fc.baseKind, &c->sampPeriod,
                 &c->winDur, &c->frPeriod, &c->numChans, &c->numCeps, &c->cepLifter, &c->preEmph, &c->useHam, &c->usePower, &c->zMeanSource,
                 &c->rawEnergy, &c->eNormalise, &c->loFreq, &c->hiFreq, &c->hasC0, &c->hasE, &c->hasD, &c->hasA, &c->hasZ, &c->delWin,
                 &c->accWin, &fc.lpcOrder, &fc.compressFact, &nSamples) != 26) break;
      c->cepScale = 1.0f; c->silFloor = 50.0f; c->eScale = 0.1f;
      bad += one(name, &fc, nSamples);
      n++;
   }
   fclose(f);
   if (bad || n == 0) { fprintf(stderr, "%d of %d configurations failed\n", bad, n); return 1; }
   printf("OK %d\n", n);
   return 0;
}
