// latrescore.hip -- HLRescore's dynamic programmes for K scale settings x U lattices in one call (htkamd_latset_best / _fb_max / _prune).
//
// The reference walks one lattice at a time: LatFindBest (HLat.c:575) and LatForwBackw (:490, LATFB_MAX) visit the nodes in LatTopSort's
// order and relax every arc once; LatPrune (:711) compares Fw + LArcTotLike + Bw with best - thresh.  Each (setting k, lattice u) pair is an
// independent chain of dependent fp64 additions and compares, so here:
//   ONE LANE PER PAIR.  The pairs are flattened as rank(u) * K + k with the lattices ranked by arc count: the lanes of a wavefront finish
//   together, and with K >= 64 they share a lattice -- the arc records are then one broadcast read and the node scores of the 64 settings
//   lie side by side.  The host has already put each lattice's arcs in the order the reference's loops meet them (host/latrescore.c), so a
//   lane makes ONE linear pass over a pre-ordered list, forward and backward.
//   Node scores: a lattice of at most LAT_TILE nodes keeps them in LDS, [node][lane] -- a lane's bank is fixed by its number, whatever node
//   it touches, so 64 lanes on 64 different lattices never conflict.  A larger lattice works in global memory, interleaved
//   [K * nodeOff[u] + node * K + k].  The choice is per lane (a generic pointer and a stride), no lattice size is refused.
//   Fw and Bw come back in that interleaved layout; the prune kernel reads them there.
// Arithmetic: LArcTotLike is htkamd_larc_tot_like (latrescore.h; float products and sums, the word penalty joined in double), the rest fp64
// in the reference's order of operations; the file is built with -ffp-contract=off, so no product is fused into a sum.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "hipcheck.h"
#include "devbuf.h"
#include "latrescore.h"

DEVBUF_OWNER("latset")

#define LAT_TILE      64          // nodes of a lattice whose scores a lane keeps in LDS
#define LAT_MAXBLOCKS 4096
#define LAT_NBIN      1000        // LatPrune's histogram (HLat.c:726)

struct LatDesc { int nodeOff, arcOff, nn, na, start, end, first, pad; double endTime; };      // nodeOff / arcOff: in the set's flat arrays
struct LatDev {
   const LatDesc *lat; const int *rank;                          // rank [U]: lattices by arc count, largest first
   const int *arcStart, *arcEnd, *fwd, *bwd; const float *ac, *lm, *pr; const unsigned char *nullEnd;
   int U, K; long long totalNodes, totalArcs;
   const htkamd_lat_scales *scales;
};

__device__ __forceinline__ double arc_like(const LatDev &D, int a, const htkamd_lat_scales &s)
{
   return htkamd_larc_tot_like(D.ac[a], D.lm[a], D.pr[a], s.acScale, s.lmScale, s.prScale, s.wordPen, D.nullEnd[a]);
}

// pair p of the launch -> (k, u); false past the end
__device__ __forceinline__ bool pair_of(const LatDev &D, long long p, int &k, int &u)
{
   if (p >= (long long)D.U * D.K) return false;
   k = (int)(p % D.K); u = D.rank[p / D.K];
   return true;
}

// LatFindBest: scores and back-pointers, then the walk back from the end node.  gScore / gBack: interleaved scratch for lattices beyond the tile.
__global__ __launch_bounds__(64) void k_lat_best(LatDev D, double *gScore, int *gBack, int *nPath, int *status, int *pathArcs, double *totals)
{
   __shared__ double sScore[LAT_TILE * 64];
   __shared__ int sBack[LAT_TILE * 64];
   const int lane = threadIdx.x;
   for (long long p = (long long)blockIdx.x * 64 + lane; ; p += (long long)gridDim.x * 64) {
      int k, u;
      if (!pair_of(D, p, k, u)) break;
      const LatDesc L = D.lat[u];
      const htkamd_lat_scales sc = D.scales[k];
      const bool tile = L.nn <= LAT_TILE;
      const size_t stride = tile ? 64 : (size_t)D.K, gbase = (size_t)D.K * (size_t)L.nodeOff + (size_t)k;
      double *score = tile ? &sScore[lane] : gScore + gbase;
      int *back = tile ? &sBack[lane] : gBack + gbase;
      for (int n = 0; n < L.nn; n++) { score[n * stride] = LZERO; back[n * stride] = -1; }
      score[L.start * stride] = 0.0;
      for (int i = 0; i < L.na; i++) {
         const int a = L.arcOff + D.fwd[L.arcOff + i], s = D.arcStart[a], e = D.arcEnd[a];
         const double v = score[s * stride] + arc_like(D, a, sc);
         if (v > score[e * stride]) { score[e * stride] = v; back[e * stride] = a - L.arcOff; }
      }
      // the path: counted first, then written start to end; the sums run from the end, as the reference's do
      int len = 0;
      for (int n = L.end, a; len < L.nn && (a = back[n * stride]) >= 0; len++) n = D.arcStart[L.arcOff + a];
      int *out = pathArcs + (size_t)k * (size_t)D.totalNodes + L.nodeOff;
      double ac = 0, lm = 0, pr = 0, tot = 0;
      int n = L.end;
      for (int i = len - 1; i >= 0; i--) {
         const int a = back[n * stride], ga = L.arcOff + a;
         out[i] = a;
         ac += D.ac[ga]; lm += D.lm[ga]; pr += D.pr[ga]; tot += arc_like(D, ga, sc);
         n = D.arcStart[ga];
      }
      const size_t q = (size_t)k * D.U + u;
      nPath[q] = len; status[q] = len > 0;
      totals[4 * q] = ac; totals[4 * q + 1] = lm; totals[4 * q + 2] = pr; totals[4 * q + 3] = tot;
   }
}

// LatForwBackw (LATFB_MAX): Fw, then Bw, each in the tile or in place in the interleaved output; best = Bw[first node of the order]
__global__ __launch_bounds__(64) void k_lat_fb(LatDev D, double *fw, double *bw, double *best)
{
   __shared__ double sScore[LAT_TILE * 64];
   const int lane = threadIdx.x;
   for (long long p = (long long)blockIdx.x * 64 + lane; ; p += (long long)gridDim.x * 64) {
      int k, u;
      if (!pair_of(D, p, k, u)) break;
      const LatDesc L = D.lat[u];
      const htkamd_lat_scales sc = D.scales[k];
      const bool tile = L.nn <= LAT_TILE;
      const size_t K = (size_t)D.K, stride = tile ? 64 : K, gbase = K * (size_t)L.nodeOff + (size_t)k;
      for (int dir = 0; dir < 2; dir++) {
         double *g = (dir ? bw : fw) + gbase, *score = tile ? &sScore[lane] : g;
         const int *order = (dir ? D.bwd : D.fwd) + L.arcOff;
         for (int n = 0; n < L.nn; n++) score[n * stride] = LZERO;
         score[(dir ? L.end : L.start) * stride] = 0.0;
         for (int i = 0; i < L.na; i++) {
            const int a = L.arcOff + order[i], from = dir ? D.arcEnd[a] : D.arcStart[a], to = dir ? D.arcStart[a] : D.arcEnd[a];
            const double v = score[from * stride] + arc_like(D, a, sc);
            if (v > score[to * stride]) score[to * stride] = v;
         }
         if (tile) for (int n = 0; n < L.nn; n++) g[n * K] = score[n * 64];
         if (dir) best[(size_t)k * D.U + u] = score[L.first * stride];
      }
   }
}

// LatPrune's limit (the arcs-per-second histogram included) and the >= limit tests
__global__ __launch_bounds__(64) void k_lat_prune(LatDev D, const double *fw, const double *bw, const double *best, const double *thresh, const float *arcsPerSec,
                                                  unsigned char *keepNode, unsigned char *keepArc)
{
   for (long long p = (long long)blockIdx.x * 64 + threadIdx.x; ; p += (long long)gridDim.x * 64) {
      int k, u;
      if (!pair_of(D, p, k, u)) break;
      const LatDesc L = D.lat[u];
      const htkamd_lat_scales sc = D.scales[k];
      const size_t K = (size_t)D.K;
      const double *F = fw + K * (size_t)L.nodeOff + (size_t)k, *B = bw + K * (size_t)L.nodeOff + (size_t)k;
      const double bst = best[(size_t)k * D.U + u];
      double th = thresh[k], limit = bst - th;
      const float aps = arcsPerSec[k];
      if (aps > 0) {
         // hist[bin] is never stored: the new beam is the first bin at which the running count passes nArcLimit, found by bisection over
         // the bins, each probe one pass over the arcs (the number of arcs whose bin is <= i grows with i)
         const int nArcLimit = (int)(L.endTime * aps);                        // HTime length * float arcsPerSec, truncated
         const float binWidth = (float)(th / LAT_NBIN);
         auto upTo = [&](int bin) {
            int cnt = 0;
            for (int i = 0; i < L.na; i++) {
               const int a = L.arcOff + i;
               const double score = F[(size_t)D.arcStart[a] * K] + arc_like(D, a, sc) + B[(size_t)D.arcEnd[a] * K];
               const double q = (bst - score) / binWidth;
               cnt += q < (double)LAT_NBIN && (int)q <= bin;                  // (a bin that does not fit an int is far outside the beam)
            }
            return cnt;
         };
         if (upTo(LAT_NBIN - 1) > nArcLimit) {
            int lo = 0, hi = LAT_NBIN - 1;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (upTo(mid) > nArcLimit) hi = mid; else lo = mid + 1; }
            th = (double)((float)lo * binWidth); limit = bst - th;
         }
      }
      unsigned char *kn = keepNode + (size_t)k * (size_t)D.totalNodes + L.nodeOff, *ka = keepArc + (size_t)k * (size_t)D.totalArcs + L.arcOff;
      for (int n = 0; n < L.nn; n++) kn[n] = (F[(size_t)n * K] + B[(size_t)n * K]) >= limit;
      for (int i = 0; i < L.na; i++) {
         const int a = L.arcOff + i;
         ka[i] = (F[(size_t)D.arcStart[a] * K] + arc_like(D, a, sc) + B[(size_t)D.arcEnd[a] * K]) >= limit;
      }
   }
}

struct LatBufs {
   DevBuf desc, rank, arcStart, arcEnd, fwd, bwd, ac, lm, pr, nullEnd, scales, score, back, nPath, status, path, totals, fw, bw, best, thresh, aps, keepNode, keepArc;
   KernelTimer timer;
};
static void lat_dev_free(void *dev) { delete (LatBufs *)dev; }

extern "C" int htkamd_latset_tile(void) { return LAT_TILE; }

// uploads the set's flat arrays when lattices were added since the last call, and this call's scales
static int lat_upload(htkamd_latset *s, int K, const htkamd_lat_scales *scales, hipStream_t st, LatDev &D, const char *what)
{
   if (!s || K < 1 || !scales) { htkamd_set_error("%s: bad argument", what); return HTKAMD_EINVAL; }
   if (s->nLats < 1) { htkamd_set_error("%s: the set is empty", what); return HTKAMD_EINVAL; }
   if (s->totalNodes * K > ((long long)1 << 31) - 1 || s->totalArcs * K > ((long long)1 << 31) - 1 || s->totalArcs > ((long long)1 << 30)) {
      htkamd_set_error("%s: %lld nodes and %lld arcs under %d settings are too many for one call", what, s->totalNodes, s->totalArcs, K); return HTKAMD_EINVAL;
   }
   if (htkamd_device_count() <= 0) { htkamd_set_error("%s: no HIP device", what); return HTKAMD_ENODEV; }
   if (!s->dev) { s->dev = new LatBufs(); s->devFree = lat_dev_free; }
   LatBufs &B = *(LatBufs *)s->dev;
   const int U = s->nLats;
   const size_t TA = (size_t)s->totalArcs;
   int rc;
   if (s->latsOnDevice != U) {
      std::vector<LatDesc> desc((size_t)U);
      std::vector<int> rank((size_t)U), aS(TA + 1), aE(TA + 1), fwd(TA + 1), bwd(TA + 1);
      std::vector<float> ac(TA + 1), lm(TA + 1), pr(TA + 1);
      std::vector<unsigned char> ne(TA + 1);
      int no = 0, ao = 0;
      for (int u = 0; u < U; u++) {
         const htkamd_lat_one &l = s->lat[u];
         LatDesc &d = desc[(size_t)u];
         d.nodeOff = no; d.arcOff = ao; d.nn = l.nn; d.na = l.na; d.start = l.start; d.end = l.end; d.first = l.topOrder[0]; d.pad = 0;
         d.endTime = l.nodeTime[l.end];                       // LatPrune's `length` (HLat.c:732)
         for (int a = 0; a < l.na; a++) {
            aS[(size_t)ao + a] = l.arcStart[a]; aE[(size_t)ao + a] = l.arcEnd[a]; fwd[(size_t)ao + a] = l.fwdArcs[a]; bwd[(size_t)ao + a] = l.bwdArcs[a];
            ac[(size_t)ao + a] = l.arcAc[a]; lm[(size_t)ao + a] = l.arcLm[a]; pr[(size_t)ao + a] = l.arcPr[a]; ne[(size_t)ao + a] = l.nodeWord[l.arcEnd[a]] == 0;
         }
         no += l.nn; ao += l.na; rank[(size_t)u] = u;
      }
      std::stable_sort(rank.begin(), rank.end(), [&](int a, int b) { return s->lat[a].na > s->lat[b].na; });
      if ((rc = B.desc.upload(desc, st)) || (rc = B.rank.upload(rank, st)) || (rc = B.arcStart.upload(aS, st)) || (rc = B.arcEnd.upload(aE, st)) ||
          (rc = B.fwd.upload(fwd, st)) || (rc = B.bwd.upload(bwd, st)) || (rc = B.ac.upload(ac, st)) || (rc = B.lm.upload(lm, st)) || (rc = B.pr.upload(pr, st)) ||
          (rc = B.nullEnd.upload(ne, st)))
         return rc;
      HIPCHECK(hipStreamSynchronize(st));                     // (the vectors go out of scope)
      s->latsOnDevice = U;
   }
   if ((rc = B.scales.upload(scales, (size_t)K, st))) return rc;
   D.lat = B.desc.as<const LatDesc>(); D.rank = B.rank.as<const int>();
   D.arcStart = B.arcStart.as<const int>(); D.arcEnd = B.arcEnd.as<const int>(); D.fwd = B.fwd.as<const int>(); D.bwd = B.bwd.as<const int>();
   D.ac = B.ac.as<const float>(); D.lm = B.lm.as<const float>(); D.pr = B.pr.as<const float>(); D.nullEnd = B.nullEnd.as<const unsigned char>();
   D.U = U; D.K = K; D.totalNodes = s->totalNodes; D.totalArcs = s->totalArcs;
   D.scales = B.scales.as<const htkamd_lat_scales>();
   s->kernelMs = 0.0;
   return HTKAMD_OK;
}

// the end of a timed call: its copies are over and its kernel time is the set's
static int lat_finish(htkamd_latset *s, hipStream_t st)
{
   float ms = 0.0f;
   HIPCHECK(hipStreamSynchronize(st));
   HIPCHECK(((LatBufs *)s->dev)->timer.ms(&ms));
   s->kernelMs = ms;
   return HTKAMD_OK;
}

static unsigned lat_blocks(const htkamd_latset *s, int K)
{
   const long long pairs = (long long)s->nLats * K, b = (pairs + 63) / 64;
   return (unsigned)(b > LAT_MAXBLOCKS ? LAT_MAXBLOCKS : b);
}

extern "C" int htkamd_latset_best(htkamd_latset *s, int K, const htkamd_lat_scales *scales, const htkamd_latset_best_out *out, void *stream)
{
   if (!out || !out->nPath || !out->status || !out->pathArcs || !out->totals) { htkamd_set_error("latset_best: bad argument"); return HTKAMD_EINVAL; }
   hipStream_t st = (hipStream_t)stream;
   LatDev D;
   int rc = lat_upload(s, K, scales, st, D, "latset_best");
   if (rc) return rc;
   LatBufs &B = *(LatBufs *)s->dev;
   const size_t KN = (size_t)K * (size_t)s->totalNodes, P = (size_t)K * (size_t)s->nLats;
   bool big = false;
   for (int u = 0; u < s->nLats && !big; u++) big = s->lat[u].nn > LAT_TILE;
   if (big && ((rc = B.score.reserve<double>(KN)) || (rc = B.back.reserve<int>(KN)))) return rc;
   if ((rc = B.nPath.reserve<int>(P)) || (rc = B.status.reserve<int>(P)) || (rc = B.path.reserve<int>(KN)) || (rc = B.totals.reserve<double>(4 * P))) return rc;
   HIPCHECK(B.timer.start(st));
   hipLaunchKernelGGL(k_lat_best, dim3(lat_blocks(s, K)), dim3(64), 0, st, D, big ? B.score.as<double>() : nullptr, big ? B.back.as<int>() : nullptr, B.nPath.as<int>(),
                      B.status.as<int>(), B.path.as<int>(), B.totals.as<double>());
   HIPCHECK(hipGetLastError());
   HIPCHECK(B.timer.stop(st));
   if ((rc = B.nPath.download(out->nPath, P, st)) || (rc = B.status.download(out->status, P, st)) || (rc = B.path.download(out->pathArcs, KN, st)) ||
       (rc = B.totals.download(out->totals, 4 * P, st)))
      return rc;
   return lat_finish(s, st);
}

// the forward-backward launch both entry points share; leaves Fw / Bw / best on the device
static int lat_fb_launch(htkamd_latset *s, int K, const LatDev &D, hipStream_t st)
{
   LatBufs &B = *(LatBufs *)s->dev;
   const size_t KN = (size_t)K * (size_t)s->totalNodes, P = (size_t)K * (size_t)s->nLats;
   int rc;
   if ((rc = B.fw.reserve<double>(KN)) || (rc = B.bw.reserve<double>(KN)) || (rc = B.best.reserve<double>(P))) return rc;
   hipLaunchKernelGGL(k_lat_fb, dim3(lat_blocks(s, K)), dim3(64), 0, st, D, B.fw.as<double>(), B.bw.as<double>(), B.best.as<double>());
   HIPCHECK(hipGetLastError());
   return HTKAMD_OK;
}

extern "C" int htkamd_latset_fb_max(htkamd_latset *s, int K, const htkamd_lat_scales *scales, const htkamd_latset_fb_out *out, void *stream)
{
   if (!out || !out->fw || !out->bw || !out->best) { htkamd_set_error("latset_fb_max: bad argument"); return HTKAMD_EINVAL; }
   hipStream_t st = (hipStream_t)stream;
   LatDev D;
   int rc = lat_upload(s, K, scales, st, D, "latset_fb_max");
   if (rc) return rc;
   LatBufs &B = *(LatBufs *)s->dev;
   const size_t KN = (size_t)K * (size_t)s->totalNodes, P = (size_t)K * (size_t)s->nLats;
   HIPCHECK(B.timer.start(st));
   if ((rc = lat_fb_launch(s, K, D, st))) return rc;
   HIPCHECK(B.timer.stop(st));
   if ((rc = B.fw.download(out->fw, KN, st)) || (rc = B.bw.download(out->bw, KN, st)) || (rc = B.best.download(out->best, P, st))) return rc;
   return lat_finish(s, st);
}

extern "C" int htkamd_latset_prune(htkamd_latset *s, int K, const htkamd_lat_scales *scales, const double *thresh, const float *arcsPerSec,
                                   unsigned char *keepNode, unsigned char *keepArc, void *stream)
{
   if (!thresh || !arcsPerSec || !keepNode || !keepArc) { htkamd_set_error("latset_prune: bad argument"); return HTKAMD_EINVAL; }
   for (int k = 0; k < K; k++) if (!(thresh[k] >= 0.0) || !(arcsPerSec[k] >= 0.0f)) { htkamd_set_error("latset_prune: setting %d has a negative beam or arc rate", k); return HTKAMD_EINVAL; }
   // (binWidth = thresh / 1000 would be zero: the reference divides by it and asserts on what comes out)
   for (int k = 0; k < K; k++) if (arcsPerSec[k] > 0.0f && !((float)(thresh[k] / LAT_NBIN) > 0.0f)) { htkamd_set_error("latset_prune: setting %d has an arcs-per-second limit and a beam of %g: the histogram needs a beam above zero", k, thresh[k]); return HTKAMD_EINVAL; }
   hipStream_t st = (hipStream_t)stream;
   LatDev D;
   int rc = lat_upload(s, K, scales, st, D, "latset_prune");
   if (rc) return rc;
   LatBufs &B = *(LatBufs *)s->dev;
   const size_t KN = (size_t)K * (size_t)s->totalNodes, KA = (size_t)K * (size_t)s->totalArcs;
   if ((rc = B.thresh.upload(thresh, (size_t)K, st)) || (rc = B.aps.upload(arcsPerSec, (size_t)K, st)) || (rc = B.keepNode.reserve<unsigned char>(KN)) ||
       (rc = B.keepArc.reserve<unsigned char>(KA)))
      return rc;
   HIPCHECK(B.timer.start(st));
   if ((rc = lat_fb_launch(s, K, D, st))) return rc;
   hipLaunchKernelGGL(k_lat_prune, dim3(lat_blocks(s, K)), dim3(64), 0, st, D, B.fw.as<const double>(), B.bw.as<const double>(), B.best.as<const double>(),
                      B.thresh.as<const double>(), B.aps.as<const float>(), B.keepNode.as<unsigned char>(), B.keepArc.as<unsigned char>());
   HIPCHECK(hipGetLastError());
   HIPCHECK(B.timer.stop(st));
   if ((rc = B.keepNode.download(keepNode, KN, st)) || (rc = B.keepArc.download(keepArc, KA, st))) return rc;
   return lat_finish(s, st);
}
