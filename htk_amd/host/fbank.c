/* fbank.c -- host-side (C) tables of the MFCC front end: everything the reference computes once per
 * configuration with libm is computed here the same way and handed to the device as tables, so that the
 * per-frame kernels only do the reference's multiply/add sequences:
 *   frame geometry        HWave.c:1575-1576 (frSize, frRate), :1663 FramesInWave
 *   mel filterbank        InitFBank HSigP.c:471-555 (fres, centre frequencies, loChan, loWt) -> per-bin k ranges
 *   Hamming window        GenHamWindow HSigP.c:108-120
 *   lifter                GenCepWin HSigP.c:755-770
 *   DCT cosines           FBank2MFCC HSigP.c:607-621 (cos(x*(k-0.5)) per term, double)
 *   FFT twiddles          the double-precision recurrences of FFT HSigP.c:332-349 and Realft :371-386, tabulated
 *   PLP                   InitPLP HSigP.c:663-690: equal-loudness curve at the filters' centres, IDFT cosine matrix
 *   VTLN                  WarpFreq HSigP.c:449-468 on the filters' centres (InitFBank :513-526), ValidCodeParms HParm.c:1366-1383
 * and the validation of the other FFT front ends (FBANK, MELSPEC, PLP: ValidCodeParms HParm.c:1317-1365).
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "../csrc/internal.h"

#define HTK_PI 3.14159265358979

/* mel value of FFT bin k (1-based): Mel(k, fres) HSigP.c:443 */
static float bin_mel(int k, float fres) { return 1127 * log(1 + (k - 1) * fres); }
static float hz_mel(float hz) { return 1127 * log(1 + hz / 700.0); }

/* The reference generates its FFT and Realft twiddles by walking round the unit circle in double:
      w_0 = 1,  w_{n+1} = w_n + w_n * ((cos t - 1) + i sin t),   cos t - 1 = -2 sin^2(t/2)
   (HSigP.c:332-349, :371-386).  Emits steps first .. first+count-1 of that walk as (re, im) pairs, with the same double operations
   in the same order, so that the tabulated values are the ones the reference multiplies with. */
static void unit_walk(double theta, int first, int count, double *out)
{
   const double h = sin(0.5 * theta), dRe = -2.0 * h * h, dIm = sin(theta);
   double re = 1.0, im = 0.0;
   int n;
   for (n = 0; n < first + count; n++) {
      const double re0 = re;
      if (n >= first) { out[2 * (n - first)] = re; out[2 * (n - first) + 1] = im; }
      re = re * dRe - im * dIm + re;
      im = im * dRe + re0 * dIm + im;
   }
}

int htkamd_mfcc_num_frames(const htkamd_mfcc_config *c, int nSamples)
{
   const int fs = (int)(c->winDur / c->sampPeriod), fr = (int)(c->frPeriod / c->sampPeriod);
   if (fs <= 0 || fr <= 0 || fs > nSamples) return 0;
   return (nSamples - fs) / fr + 1;
}

int htkamd_mfcc_num_cols(const htkamd_mfcc_config *c)
{
   const int nStat = c->numCeps + (c->hasC0 ? 1 : 0) + (c->hasE ? 1 : 0);
   return nStat * (1 + (c->hasD ? 1 : 0) + (c->hasA ? 1 : 0));
}

void htkamd_mfcc_tables_free(struct htkamd_mfcc_tables *t)
{
   free(t->ham); free(t->cepWin); free(t->loWt); free(t->binA0); free(t->dct); free(t->tw); free(t->rtw); free(t->brev);
   free(t->eql); free(t->cm); free(t->edge);
   memset(t, 0, sizeof(*t));
}

/* frame and FFT geometry, channel and cepstrum counts: MFCC keeps its own limits (numChans <= 63, numCeps <= 64); the other kinds take
   ValidCodeParms' 2..1000 channels (HParm.c:1340) and need numCeps only for PLP */
static int check_geometry(const htkamd_mfcc_config *c, int baseKind)
{
   const int frSize = (int)(c->winDur / c->sampPeriod), frRate = (int)(c->frPeriod / c->sampPeriod);
   int fftN = 2;
   if (baseKind == 6) {
      if (frSize < 2 || frRate < 1 || c->numChans < 1 || c->numCeps < 1 || c->numCeps > 64 || c->numChans > 63) {
         htkamd_set_error("mfcc: unsupported geometry (frSize %d frRate %d chans %d ceps %d)", frSize, frRate, c->numChans, c->numCeps);
         return HTKAMD_EINVAL;
      }
   } else if (frSize < 2 || frRate < 1 || c->numChans < 2 || c->numChans > 1000) {
      htkamd_set_error("frontend: unsupported geometry (frSize %d frRate %d chans %d; NUMCHANS must lie in 2..1000)", frSize, frRate, c->numChans);
      return HTKAMD_EINVAL;
   }
   while (frSize > fftN) fftN *= 2;
   if (fftN < 8 || fftN > 4096) { htkamd_set_error("mfcc: FFT size %d outside 8..4096", fftN); return HTKAMD_EINVAL; }
   return HTKAMD_OK;
}

int htkamd_frontend_check(const htkamd_frontend_config *f)
{
   const htkamd_mfcc_config *c;
   if (!f) { htkamd_set_error("frontend: NULL configuration"); return HTKAMD_EINVAL; }
   c = &f->base;
   switch (f->baseKind) {
   case 6: case 7: case 8: case 11: break;
   case 1: case 2: case 3:
      htkamd_set_error("frontend: %s is a time-domain LPC kind (Wave2LPC); only MFCC, FBANK, MELSPEC and PLP are coded on the device",
                       f->baseKind == 1 ? "LPC" : f->baseKind == 2 ? "LPREFC" : "LPCEPSTRA");
      return HTKAMD_EINVAL;
   default:
      htkamd_set_error("frontend: base kind %d is not an FFT front end (MFCC 6, FBANK 7, MELSPEC 8, PLP 11)", f->baseKind);
      return HTKAMD_EINVAL;
   }
   if ((f->baseKind == 7 || f->baseKind == 8) && c->hasC0) {
      htkamd_set_error("frontend: _0 on %s: the filterbank kinds have no C0", f->baseKind == 7 ? "FBANK" : "MELSPEC");
      return HTKAMD_EINVAL;
   }
   if (f->baseKind == 11) {                           /* ValidCodeParms HParm.c:1347-1362 */
      if (f->lpcOrder < 2 || f->lpcOrder > 1000) { htkamd_set_error("frontend: PLP: unlikely LPCORDER %d (2..1000)", f->lpcOrder); return HTKAMD_EINVAL; }
      if (c->numCeps < 2 || c->numCeps > f->lpcOrder) {
         htkamd_set_error("frontend: PLP: unlikely NUMCEPS %d (2..LPCORDER = %d)", c->numCeps, f->lpcOrder); return HTKAMD_EINVAL;
      }
      if (!(f->compressFact > 0.0f && f->compressFact < 1.0f)) {
         htkamd_set_error("frontend: PLP: COMPRESSFACT %g must lie strictly between 0 and 1", (double)f->compressFact); return HTKAMD_EINVAL;
      }
   }
   return check_geometry(c, f->baseKind);
}

/* FFT size, band of interest (FFT bins klo..khi, mel range melLo..melHi, optionally narrowed by LOFREQ / HIFREQ): InitFBank HSigP.c:485-504 */
static void fbank_band(const htkamd_mfcc_config *c, int *fftNOut, float *fresOut, int *kloOut, int *khiOut, float *melLoOut, float *melHiOut)
{
   const int frSize = (int)(c->winDur / c->sampPeriod);
   int fftN = 2, half, klo, khi;
   float fres, melLo, melHi;
   while (frSize > fftN) fftN *= 2;
   half = fftN / 2;
   fres = 1.0E7 / ((long)c->sampPeriod * fftN * 700.0);
   klo = 2; khi = half;
   melLo = 0; melHi = bin_mel(half + 1, fres);
   if (c->loFreq >= 0.0) {
      melLo = hz_mel(c->loFreq);
      klo = (int)((c->loFreq * (long)c->sampPeriod * 1.0e-7 * fftN) + 2.5);
      if (klo < 2) klo = 2;
   }
   if (c->hiFreq >= 0.0) {
      melHi = hz_mel(c->hiFreq);
      khi = (int)((c->hiFreq * (long)c->sampPeriod * 1.0e-7 * fftN) + 0.5);
      if (khi > half) khi = half;
   }
   *fftNOut = fftN; *fresOut = fres; *kloOut = klo; *khiOut = khi; *melLoOut = melLo; *melHiOut = melHi;
}

/* the band's ends in Hz as InitFBank forms them for WarpFreq (HSigP.c:518-519): exp in double, stored as float */
static float mel_hz(float mel) { return 700.0 * (exp(mel / 1127.0) - 1.0); }

/* WarpFreq HSigP.c:449-468, every step in float as there: piecewise linear, slope 1/alpha between the two corner frequencies cl and cu,
   the pieces below and above them bent so that minFreq and maxFreq stay where they are */
static float warp_freq(float fcl, float fcu, float freq, float minFreq, float maxFreq, float alpha)
{
   if (alpha == 1.0)
      return freq;
   else {
      float scale = 1.0 / alpha;
      float cu = fcu * 2 / (1 + scale);
      float cl = fcl * 2 / (1 + scale);
      float au = (maxFreq - cu * scale) / (maxFreq - cu);
      float al = (cl * scale - minFreq) / (cl - minFreq);
      if (freq > cu) return au * (freq - cu) + scale * cu;
      else if (freq < cl) return al * (freq - minFreq) + minFreq;
      else return scale * freq;
   }
}

/* ValidCodeParms' own checks of a warp (HParm.c:1366-1372): they need no front-end configuration */
int htkamd_warp_check(const htkamd_warp *w)
{
   if (!w) { htkamd_set_error("frontend: NULL warp"); return HTKAMD_EINVAL; }
   if (!(w->warpFreq >= 0.5f && w->warpFreq <= 2.0f)) {
      htkamd_set_error("frontend: unlikely warping factor WARPFREQ %g (0.5..2.0)", (double)w->warpFreq); return HTKAMD_EINVAL;
   }
   if (w->warpFreq != 1.0 && (w->warpLCutoff == 0.0 || w->warpUCutoff == 0.0 || !(w->warpLCutoff <= w->warpUCutoff))) {
      htkamd_set_error("frontend: invalid warping cut-off frequencies WARPLCUTOFF %g WARPUCUTOFF %g (both set, lower <= upper)",
                       (double)w->warpLCutoff, (double)w->warpUCutoff);
      return HTKAMD_EINVAL;
   }
   return HTKAMD_OK;
}

int htkamd_frontend_warp_check(const htkamd_frontend_config *f, const htkamd_warp *w)
{
   int rc, fftN, klo, khi;
   float fres, melLo, melHi;
   if ((rc = htkamd_warp_check(w)) != HTKAMD_OK || (rc = htkamd_frontend_check(f)) != HTKAMD_OK) return rc;
   if (w->warpFreq == 1.0) return HTKAMD_OK;
   /* what the reference leaves unchecked: WarpFreq's two outer pieces divide by cl - minFreq and maxFreq - cu, and the map only
      increases while both pieces keep a positive slope */
   fbank_band(&f->base, &fftN, &fres, &klo, &khi, &melLo, &melHi);
   {
      const float minFreq = mel_hz(melLo), maxFreq = mel_hz(melHi);
      const float scale = 1.0 / w->warpFreq, cu = w->warpUCutoff * 2 / (1 + scale), cl = w->warpLCutoff * 2 / (1 + scale);
      if (!(cl > minFreq)) {
         htkamd_set_error("frontend: WARPLCUTOFF %g: the lower corner %g Hz does not lie above the band's lower end %g Hz",
                          (double)w->warpLCutoff, (double)cl, (double)minFreq);
         return HTKAMD_EINVAL;
      }
      if (!(cu < maxFreq)) {
         htkamd_set_error("frontend: WARPUCUTOFF %g: the upper corner %g Hz does not lie below the band's upper end %g Hz",
                          (double)w->warpUCutoff, (double)cu, (double)maxFreq);
         return HTKAMD_EINVAL;
      }
      if (!(scale * cu < maxFreq)) {
         htkamd_set_error("frontend: WARPFREQ %g maps the upper corner %g Hz to %g Hz, at or beyond the band's upper end %g Hz",
                          (double)w->warpFreq, (double)cu, (double)(scale * cu), (double)maxFreq);
         return HTKAMD_EINVAL;
      }
      if (!(scale * cl > minFreq)) {
         htkamd_set_error("frontend: WARPFREQ %g maps the lower corner %g Hz to %g Hz, at or below the band's lower end %g Hz",
                          (double)w->warpFreq, (double)cl, (double)(scale * cl), (double)minFreq);
         return HTKAMD_EINVAL;
      }
   }
   return HTKAMD_OK;
}

int htkamd_mfcc_tables_build(const htkamd_mfcc_config *c, struct htkamd_mfcc_tables *t)
{
   htkamd_frontend_config f;
   memset(&f, 0, sizeof(f));
   f.base = *c; f.baseKind = 6;
   return htkamd_frontend_tables_build(&f, t);
}

int htkamd_frontend_tables_build(const htkamd_frontend_config *fc, struct htkamd_mfcc_tables *t)
{
   return htkamd_frontend_tables_build_warped(fc, NULL, t);
}

/* warp NULL: no warping (the reference's alpha == 1.0 branch) */
int htkamd_frontend_tables_build_warped(const htkamd_frontend_config *fc, const htkamd_warp *warp, struct htkamd_mfcc_tables *t)
{
   const htkamd_mfcc_config *c = &fc->base;
   /* cepstra (and the lifter) for MFCC and PLP, the DCT for MFCC alone; the filterbank kinds ignore NUMCEPS */
   const int nCep = (fc->baseKind == 6 || fc->baseKind == 11) ? c->numCeps : 0, nDct = (fc->baseKind == 6) ? c->numCeps : 0;
   int fftN, half, nEdge, k, i, j, b, rc;
   float fres, melLo, melHi, *edge;
   memset(t, 0, sizeof(*t));
   if ((rc = warp ? htkamd_frontend_warp_check(fc, warp) : htkamd_frontend_check(fc)) != HTKAMD_OK) return rc;
   t->frSize = (int)(c->winDur / c->sampPeriod);
   t->frRate = (int)(c->frPeriod / c->sampPeriod);
   t->takeLogs = fc->baseKind == 6 || fc->baseKind == 7;
   /* ---- mel filterbank (InitFBank HSigP.c:471-555 supplies the numbers; the tables are this file's own form). */
   fbank_band(c, &fftN, &fres, &t->klo, &t->khi, &melLo, &melHi);
   t->fftN = fftN; half = fftN / 2;
   /* numChans triangular filters share numChans+2 equally spaced mel edges: edge[0] = melLo, edge[e] = e/(numChans+1) of the span.
      Under a warp (VTLN) every edge goes back to Hz, through WarpFreq and back to mel, in the reference's types at every step
      (HSigP.c:516-525); the band's ends stay, the last edge up to rounding */
   nEdge = c->numChans + 1;
   edge = t->edge = (float *)malloc(sizeof(float) * (size_t)(nEdge + 2));
   edge[0] = melLo;
   if (!warp || warp->warpFreq == 1.0)
      for (b = 1; b <= nEdge; b++) edge[b] = ((float)b / (float)nEdge) * (melHi - melLo) + melLo;
   else {
      const float ms = melHi - melLo, minFreq = mel_hz(melLo), maxFreq = mel_hz(melHi);
      for (b = 1; b <= nEdge; b++) {
         float cf = ((float)b / (float)nEdge) * ms + melLo;
         cf = 700 * (exp(cf / 1127.0) - 1.0);
         edge[b] = 1127.0 * log(1.0 + warp_freq(warp->warpLCutoff, warp->warpUCutoff, cf, minFreq, maxFreq, warp->warpFreq) / 700.0);
      }
   }
   edge[nEdge + 1] = edge[nEdge] + 1.0f;                /* guard: a top bin whose centre rounds above HIFREQ feeds no filter */
   /* An FFT bin k between edge[lo] and edge[lo+1] feeds filter lo with weight loWt[k] = (edge[lo+1] - mel)/(edge[lo+1] - edge[lo]) and
      filter lo+1 with the rest (Wave2FBank HSigP.c:558-604 adds loWt*ek to bin lo and ek - loWt*ek to bin lo+1, for k ascending).
      lo never decreases with k, so filter b receives, in this order, the "rest" terms of the bins with lo == b-1 and then the
      weighted terms of the bins with lo == b: two contiguous k ranges per filter, [binA0,binA1] and [binB0,binB1]. */
   t->loWt = (float *)calloc((size_t)half + 2, sizeof(float));
   t->binA0 = (int *)calloc((size_t)4 * (c->numChans + 2), sizeof(int));
   t->binA1 = t->binA0 + (c->numChans + 2); t->binB0 = t->binA1 + (c->numChans + 2); t->binB1 = t->binB0 + (c->numChans + 2);
   for (b = 1; b <= c->numChans; b++) { t->binA0[b] = 1; t->binA1[b] = 0; t->binB0[b] = 1; t->binB1[b] = 0; }
   {
      int lo = 0;                                        /* edges 1..lo lie below the current bin's mel value */
      for (k = 1; k <= half; k++) {
         const float mel = bin_mel(k, fres);
         if (k < t->klo || k > t->khi) continue;        /* outside the band: weight 0, feeds nothing */
         while (lo < nEdge && edge[lo + 1] < mel) lo++;
         t->loWt[k] = (edge[lo + 1] - mel) / (edge[lo + 1] - edge[lo]);
         if (lo >= 1 && lo <= c->numChans) { if (t->binB1[lo] < t->binB0[lo]) t->binB0[lo] = k; t->binB1[lo] = k; }
         if (lo < c->numChans) { if (t->binA1[lo + 1] < t->binA0[lo + 1]) t->binA0[lo + 1] = k; t->binA1[lo + 1] = k; }
      }
   }
   if (fc->baseKind == 11) {
      /* equal-loudness curve at the centre of filter b (edge[b] is the reference's cf[b]): the centre back to Hz with exp in double,
         then the curve in float, its two ratios formed in double as the reference's double constants make them */
      const int nFreq = c->numChans + 2;
      double angle;
      t->eql = (float *)calloc((size_t)c->numChans + 1, sizeof(float));
      for (b = 1; b <= c->numChans; b++) {
         const float hz = (float)(700.0 * (exp((double)(edge[b] / 1127.0f)) - 1.0));
         const float sq = hz * hz;
         const float sub = (float)((double)sq / ((double)sq + 1.6e5));
         t->eql[b] = (float)((double)(sub * sub) * (((double)sq + 1.44e6) / ((double)sq + 9.61e6)));
      }
      /* IDFT from the numChans + 2 auditory-spectrum points to lpcOrder + 1 autocorrelation lags: row i = lag i, weights 1, 2 cos, .., cos */
      angle = HTK_PI / (double)(nFreq - 1);
      t->cm = (double *)calloc((size_t)(fc->lpcOrder + 1) * nFreq, sizeof(double));
      for (i = 0; i <= fc->lpcOrder; i++) {
         double *row = t->cm + (size_t)i * nFreq;
         row[0] = 1.0;
         for (j = 1; j < nFreq - 1; j++) row[j] = 2.0 * cos(angle * (double)i * (double)j);
         row[nFreq - 1] = cos(angle * (double)i * (double)(nFreq - 1));
      }
   }
   t->ham = (float *)calloc((size_t)t->frSize + 1, sizeof(float));
   { const float a = HTK_TPI / (t->frSize - 1); for (i = 1; i <= t->frSize; i++) t->ham[i] = 0.54 - 0.46 * cos(a * (i - 1)); }
   t->cepWin = (float *)calloc((size_t)nCep + 1, sizeof(float));
   for (i = 1; i <= nCep; i++) t->cepWin[i] = 1.0f;
   if (c->cepLifter > 0) {
      const float a = HTK_PI / c->cepLifter, Lby2 = c->cepLifter / 2.0;
      for (i = 1; i <= nCep; i++) t->cepWin[i] = 1.0 + Lby2 * sin(i * a);
   }
   t->mfnorm = sqrt(2.0 / (float)c->numChans);
   t->dct = (double *)calloc((size_t)(nDct + 1) * (c->numChans + 1), sizeof(double));
   {
      const float pi_factor = HTK_PI / (float)c->numChans;
      for (j = 1; j <= nDct; j++) {
         const float x = (float)j * pi_factor;
         for (k = 1; k <= c->numChans; k++) t->dct[(size_t)j * (c->numChans + 1) + k] = cos(x * (k - 0.5));
      }
   }
   /* complex FFT of nn = fftN/2 points: the stage that combines blocks of `limit/2` points uses steps 0..limit/2-1 of the walk with
      angle 2 pi/limit; Realft's post-pass (i = 2..nn/2) steps 1.. of the walk with angle pi/nn */
   {
      const int nn = fftN / 2;
      int limit, off = 0, bits = 0;
      t->tw = (double *)calloc((size_t)2 * nn, sizeof(double));
      for (limit = 2; limit < fftN; limit *= 2) {
         unit_walk(HTK_TPI / limit, 0, limit / 2, t->tw + 2 * off);
         off += limit / 2;
      }
      t->rtw = (double *)calloc((size_t)2 * (nn / 2 + 2), sizeof(double));
      if (nn / 2 >= 2) unit_walk(HTK_PI / nn, 1, nn / 2 - 1, t->rtw + 4);
      /* bit reversal of the complex index (the swap loop of HSigP.c:319-331) */
      while ((1 << bits) < nn) bits++;
      t->brev = (short *)calloc((size_t)nn, sizeof(short));
      for (i = 0; i < nn; i++) {
         int r = 0;
         for (j = 0; j < bits; j++) if (i & (1 << j)) r |= 1 << (bits - 1 - j);
         t->brev[i] = (short)r;
      }
   }
   return HTKAMD_OK;
}
