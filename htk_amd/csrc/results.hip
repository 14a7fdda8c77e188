// results.hip -- HResults' string alignment for K hypothesis sets x U utterances in one call (htkamd_results_score).
//
// The reference fills a (nTest+1) x (nRef+1) grid of cells {score, ins, del, sub, hit, dir} row by row (CreateGrid HResults.c:835,
// DoCompare :883, DoCompareNIST :953), then walks `dir` back from the last cell (AppendCell :1050, CollectStats :1259).  Here:
//   k_results_align   ONE WAVEFRONT PER PAIR.  Cell (i, j) -- test label i against reference label j -- needs (i-1, j), (i-1, j-1) and
//                     (i, j-1), so the lanes run along an anti-diagonal: lane l owns column j0 + l + 1 of a 64-column stripe and in step
//                     t fills row t - l.  What a lane needs from its left neighbour (that lane's cell of the step before, and the test
//                     label it used) arrives by a one-lane wavefront shift; (i-1, j-1) is what arrived one step earlier, (i-1, j) the
//                     lane's own last cell.  So the three running diagonals of all five numbers live in registers.  Lane 0's left
//                     neighbour is the stripe's boundary column: column 0 (computed) for the first stripe, else the last column of the
//                     stripe before, which its lane 63 left in global scratch; either way 64 rows of it are held a lane each and read
//                     by step number.  A pair's chain is (nTest + 63) dependent steps per stripe and nothing hides it but other pairs:
//                     four wavefronts per workgroup, every CU full of them.
//                     `dir` is the only thing kept per cell: a byte, in the wavefront's LDS tile where nTest * nRef <= RES_DIR_TILE, in
//                     global scratch (sized by the call's largest pair) where not; written only when the caller wants alignments or a
//                     confusion matrix.  The edge rows are not stored: row 0 is VERT, column 0 HOR.  Lane 0 then walks it back and
//                     writes the triples from the END of the pair's slice, so that they stand in the reference's output order.
//   k_results_totals  adds the pairs' counts into their set's totals and their triples into its confusion matrix, integer atomics.
// Everything is integer: the results do not depend on the order of anything.
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
#include "hipcheck.h"
#include "devbuf.h"
#include "results.h"

DEVBUF_OWNER("results")

#define RES_WAVES      4          // pairs in flight per workgroup
#define RES_DIR_TILE   8192       // dir bytes (grid cells off the edge rows) a wavefront keeps in LDS
#define RES_MAXBLOCKS  1024       // 4 workgroups of 32 KB LDS on each of 256 CUs
#define RES_MAXSCRATCH ((size_t)2 << 30)

enum { DIR_DIAG = 0, DIR_VERT = 1, DIR_HOR = 2 };

struct Cell { int score, ins, del, sub, hit; };
struct PairDesc { int refPos, nRef, hypPos, nTest; long long alnPos; };

// lane l takes lane l-1's value (DPP wave_shr:1); lane 0's result is not used
__device__ __forceinline__ int wave_shr1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ Cell wave_shr1(const Cell &c) { return Cell{wave_shr1(c.score), wave_shr1(c.ins), wave_shr1(c.del), wave_shr1(c.sub), wave_shr1(c.hit)}; }
__device__ __forceinline__ Cell read_lane(const Cell &c, int l)
{
   return Cell{__builtin_amdgcn_readlane(c.score, l), __builtin_amdgcn_readlane(c.ins, l), __builtin_amdgcn_readlane(c.del, l), __builtin_amdgcn_readlane(c.sub, l),
               __builtin_amdgcn_readlane(c.hit, l)};
}
__device__ __forceinline__ int wave_incl_scan(int v, int lane)
{
   for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(v, o, 64); if (lane >= o) v += u; }
   return v;
}

// The grid of one pair; returns cell (T, R).  dir: [T * R] bytes or NULL.  bndA / bndB: [T + 1] cells each, touched only when R > 64.
template <bool NIST>
__device__ __forceinline__ Cell align_pair(const int *__restrict__ ref, int R, const int *__restrict__ test, int T, unsigned char *dir, Cell *bndA, Cell *bndB, int lane)
{
   constexpr int subP = NIST ? 4 : 10, delP = NIST ? 3 : 7, insP = NIST ? 3 : 7;
   if (R == 0) {                                              // column 0 alone: the test labels that are not null are insertions
      int c = 0;
      for (int k = lane; k < T; k += 64) c += test[k] != 0;
      c = __builtin_amdgcn_readlane(wave_incl_scan(c, lane), 63);
      return Cell{insP * c, c, 0, 0, 0};
   }
   const int nStripes = (R + 63) >> 6;
   int rowCarry = 0;                                          // reference labels before the stripe that are not null
   Cell fin = {0, 0, 0, 0, 0};
   for (int s = 0; s < nStripes; s++) {
      const int j0 = s << 6, j = j0 + lane + 1;
      const bool valid = j <= R, more = s + 1 < nStripes;
      const int rid = valid ? ref[j - 1] : 0;
      const int cnt = rowCarry + wave_incl_scan(valid && rid != 0, lane);
      Cell cur = {delP * cnt, 0, cnt, 0, 0};                  // row 0: a null label costs nothing
      Cell *bin = (s & 1) ? bndB : bndA, *bout = (s & 1) ? bndA : bndB;
      if (more && lane == 63) bout[0] = cur;
      Cell recv = {delP * rowCarry, 0, rowCarry, 0, 0}, prev, chunk = {0, 0, 0, 0, 0};      // (0, j0)
      int tid = 0, tchunk = 0, colCarry = 0;
      const int nl = (R - j0 < 64) ? R - j0 : 64;
      const int steps = T > 0 ? T + nl - 1 : 0;
      for (int t = 1; t <= steps; t++) {
         const int q = (t - 1) & 63;
         if (q == 0) {                                        // the next 64 rows of the boundary column and of the test labels, a lane each
            const int ib = t + lane;
            tchunk = ib <= T ? test[ib - 1] : 0;
            if (s == 0) {                                     // column 0
               const int c = colCarry + wave_incl_scan(ib <= T && tchunk != 0, lane);
               chunk = Cell{insP * c, c, 0, 0, 0};
               colCarry = __builtin_amdgcn_readlane(c, 63);
            } else if (ib <= T)
               chunk = bin[ib];
         }
         prev = recv;
         const Cell fromLeft = wave_shr1(cur), fromEdge = read_lane(chunk, q);
         const int tidLeft = wave_shr1(tid), tidEdge = __builtin_amdgcn_readlane(tchunk, q);
         recv = lane == 0 ? fromEdge : fromLeft;
         tid = lane == 0 ? tidEdge : tidLeft;
         const int i = t - lane;
         if (valid && i >= 1 && i <= T) {
            const bool rn = rid == 0, tn = tid == 0, normal = !rn && !tn, same = rid == tid;
            int h = cur.score, d = prev.score, v = recv.score;      // HOR from (i-1, j), DIAG from (i-1, j-1), VERT from (i, j-1)
            if (normal) { h += insP; v += delP; if (!same) d += subP; }
            int go;
            if (rn != tn) go = rn ? DIR_VERT : DIR_HOR;              // one side null: it is skipped
            else if (!NIST) go = (d <= h && d <= v) ? DIR_DIAG : (h < v ? DIR_HOR : DIR_VERT);
            else go = (v <= d && v <= h) ? DIR_VERT : (d <= h ? DIR_DIAG : DIR_HOR);
            Cell n = go == DIR_DIAG ? prev : (go == DIR_HOR ? cur : recv);
            n.score = go == DIR_DIAG ? d : (go == DIR_HOR ? h : v);
            if (normal) {
               n.hit += go == DIR_DIAG && same; n.sub += go == DIR_DIAG && !same;
               n.ins += go == DIR_HOR; n.del += go == DIR_VERT;
            }
            cur = n;
            if (dir) dir[(size_t)(i - 1) * R + (j - 1)] = (unsigned char)go;
            if (more && lane == 63) bout[i] = cur;
         }
      }
      rowCarry = __builtin_amdgcn_readlane(cnt, 63);
      if (more) {                                             // lane 63's column is read by other lanes in the next stripe
         __threadfence_block();
         __builtin_amdgcn_wave_barrier();
      } else {
         const int last = (R - 1) & 63;
         fin = read_lane(cur, last);
      }
   }
   return fin;
}

// Walks dir back from (T, R) and writes the triples backwards from out[3 * (T + R)); returns how many.
__device__ __forceinline__ int trace_back(const int *__restrict__ ref, int R, const int *__restrict__ test, int T, const unsigned char *dir, int *out)
{
   int i = T, j = R, n = 0;
   int *w = out + 3 * (size_t)(T + R);
   while (i > 0 || j > 0) {
      const int go = i == 0 ? DIR_VERT : (j == 0 ? DIR_HOR : dir[(size_t)(i - 1) * R + (j - 1)]);
      int op = -1, rl = -1, tl = -1;
      if (go == DIR_DIAG) {
         rl = ref[--j]; tl = test[--i];
         if (rl != 0 && tl != 0) op = rl == tl ? HTKAMD_RES_HIT : HTKAMD_RES_SUB;
      } else if (go == DIR_VERT) {
         rl = ref[--j];
         if (rl != 0) op = HTKAMD_RES_DEL;
         tl = -1;
      } else {
         tl = test[--i];
         if (tl != 0) op = HTKAMD_RES_INS;
         rl = -1;
      }
      if (op >= 0) { w -= 3; w[0] = op; w[1] = rl; w[2] = tl; n++; }
   }
   return n;
}

template <bool NIST>
__global__ __launch_bounds__(RES_WAVES * 64) void k_results_align(const PairDesc *__restrict__ pairs, int nPairs, const int *__restrict__ refIds, const int *__restrict__ hypIds,
                                                                    int wantDir, unsigned char *gDir, size_t gDirStride, Cell *gBnd, size_t bndStride,
                                                                    int *__restrict__ counts, int *__restrict__ aln, int *__restrict__ alnLen)
{
   __shared__ unsigned char sDir[RES_WAVES][RES_DIR_TILE];
   const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
   const int slot = __builtin_amdgcn_readfirstlane((int)blockIdx.x * RES_WAVES + w), nSlots = (int)gridDim.x * RES_WAVES;
   Cell *bndA = gBnd ? gBnd + (size_t)slot * 2 * bndStride : nullptr, *bndB = gBnd ? bndA + bndStride : nullptr;
   for (int p = slot; p < nPairs; p += nSlots) {
      const PairDesc pd = pairs[p];
      const int R = pd.nRef, T = pd.nTest;
      const int *ref = refIds + pd.refPos, *test = hypIds + pd.hypPos;
      const size_t cells = (size_t)R * (size_t)T;
      const bool inLds = cells <= RES_DIR_TILE;
      Cell fin;
      unsigned char *dir = nullptr;
      if (!wantDir || cells == 0)
         fin = align_pair<NIST>(ref, R, test, T, nullptr, bndA, bndB, lane);
      else if (inLds)
         fin = align_pair<NIST>(ref, R, test, T, dir = sDir[w], bndA, bndB, lane);
      else
         fin = align_pair<NIST>(ref, R, test, T, dir = gDir + (size_t)slot * gDirStride, bndA, bndB, lane);
      __threadfence_block();                                  // lane 0 reads what every lane wrote
      __builtin_amdgcn_wave_barrier();
      if (lane == 0) {
         int *c = counts + 6 * (size_t)p;
         c[0] = fin.hit; c[1] = fin.del; c[2] = fin.sub; c[3] = fin.ins; c[4] = fin.hit + fin.del + fin.sub; c[5] = R > 0 && T > 0;
         if (wantDir) alnLen[p] = trace_back(ref, R, test, T, dir, aln + 3 * (size_t)pd.alnPos);
      }
      __builtin_amdgcn_wave_barrier();                        // the tile is the next pair's
   }
}

// grid (ceil(U / 256), K): thread u of set k adds pair k * U + u to the set's totals; its triples to the set's confusion matrix
__global__ __launch_bounds__(256) void k_results_totals(const int *__restrict__ counts, int U, unsigned long long *__restrict__ totals, const PairDesc *__restrict__ pairs,
                                                        const int *__restrict__ aln, const int *__restrict__ alnLen, int *__restrict__ conf, int V)
{
   const int u = (int)(blockIdx.x * blockDim.x + threadIdx.x), k = (int)blockIdx.y, lane = threadIdx.x & 63;
   int v[7] = {0, 0, 0, 0, 0, 0, 0};
   if (u < U) {
      const size_t p = (size_t)k * U + u;
      const int *c = counts + 6 * p;
      if (c[5]) {                                             // an empty transcription is not counted (MatchFiles :1728, MatchRecFiles :1308)
         for (int f = 0; f < 5; f++) v[f] = c[f];
         v[5] = 1; v[6] = c[1] == 0 && c[2] == 0 && c[3] == 0;
         if (conf) {
            const PairDesc pd = pairs[p];
            const int W = V + 1, n = alnLen[p];
            const int *tr = aln + 3 * (size_t)(pd.alnPos + pd.nRef + pd.nTest - n);
            int *m = conf + (size_t)k * W * W;
            for (int t = 0; t < n; t++, tr += 3) atomicAdd(&m[(tr[1] < 0 ? 0 : tr[1]) * W + (tr[2] < 0 ? 0 : tr[2])], 1);
         }
      }
   }
   for (int f = 0; f < 7; f++) {
      int x = v[f];
      for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
      if (lane == 0 && x) atomicAdd(&totals[(size_t)k * 7 + f], (unsigned long long)x);
   }
}

struct ResDev {
   DevBuf refs, hyps, pairs, counts, aln, alnLen, totals, conf, dir, bnd;
   KernelTimer timer;
};

static void res_dev_free(void *dev) { delete (ResDev *)dev; }
extern "C" double htkamd_results_last_kernel_ms(const htkamd_results *r) { return r ? r->kernelMs : 0.0; }
extern "C" int htkamd_results_dir_tile(void) { return RES_DIR_TILE; }

extern "C" int htkamd_results_score(htkamd_results *r, int K, int U, const int *uttRef, const int *hypOff, const int *hypIds, int flags,
                                    int *counts, int *alnOff, int *aln, long long alnCap, long long *totals, int *conf, void *stream)
{
   if (!r || K < 0 || U < 0 || ((size_t)K * (size_t)U > 0 && (!uttRef || !hypOff)) || (size_t)K * (size_t)U > (size_t)1 << 30) { htkamd_set_error("results_score: bad argument"); return HTKAMD_EINVAL; }
   const bool wantAln = (flags & HTKAMD_RES_ALIGN) != 0, wantConf = (flags & HTKAMD_RES_CONF) != 0, wantDir = wantAln || wantConf;
   if ((wantAln && (!alnOff || (!aln && alnCap > 0) || alnCap < 0)) || (wantConf && !conf)) { htkamd_set_error("results_score: an output that the flags ask for is NULL"); return HTKAMD_EINVAL; }
   const int nPairs = K * U, V = r->nList, W = V + 1;
   // every index a kernel will form, checked here
   for (int u = 0; u < U; u++)
      if (uttRef[u] < 0 || uttRef[u] >= r->nRefs) { htkamd_set_error("results_score: utterance %d names reference %d of %d", u, uttRef[u], r->nRefs); return HTKAMD_EINVAL; }
   if (nPairs > 0 && hypOff[0] != 0) { htkamd_set_error("results_score: the hypotheses do not start at 0"); return HTKAMD_EINVAL; }
   for (int p = 0; p < nPairs; p++) if (hypOff[p + 1] < hypOff[p]) { htkamd_set_error("results_score: the offsets of pair %d run backwards", p); return HTKAMD_EINVAL; }
   const int nHyp = nPairs > 0 ? hypOff[nPairs] : 0, idLimit = wantConf ? W : r->nNames;
   if (nHyp > 0 && !hypIds) { htkamd_set_error("results_score: bad argument"); return HTKAMD_EINVAL; }
   for (int k = 0; k < nHyp; k++)
      if (hypIds[k] < 0 || hypIds[k] >= idLimit) {
         if (hypIds[k] >= 0 && hypIds[k] < r->nNames) htkamd_set_error("results: label %s is not in the list (%d names), which the confusion matrix needs", r->name[hypIds[k]], V);
         else htkamd_set_error("results_score: hypothesis label %d has id %d (the table has %d)", k, hypIds[k], r->nNames);
         return HTKAMD_EINVAL;
      }
   if (wantConf)
      for (int u = 0; u < U; u++)
         for (int k = r->refOff[uttRef[u]]; k < r->refOff[uttRef[u] + 1]; k++)
            if (r->refIds[k] >= W) { htkamd_set_error("results: label %s is not in the list (%d names), which the confusion matrix needs", r->name[r->refIds[k]], V); return HTKAMD_EINVAL; }
   std::vector<PairDesc> pd((size_t)nPairs);
   long long alnTotal = 0;
   size_t maxDir = 0; int maxBndT = -1;
   for (int p = 0; p < nPairs; p++) {
      const int ref = uttRef[p % U];
      PairDesc &d = pd[(size_t)p];
      d.refPos = r->refOff[ref]; d.nRef = r->refOff[ref + 1] - r->refOff[ref]; d.hypPos = hypOff[p]; d.nTest = hypOff[p + 1] - hypOff[p]; d.alnPos = alnTotal;
      alnTotal += (long long)d.nRef + d.nTest;
      const size_t cells = (size_t)d.nRef * (size_t)d.nTest;
      if (wantDir && cells > RES_DIR_TILE && cells > maxDir) maxDir = cells;
      if (d.nRef > 64 && d.nTest > maxBndT) maxBndT = d.nTest;
   }
   if (wantAln && alnTotal > alnCap) { htkamd_set_error("results_score: the alignments may take %lld triples, alnCap is %lld", alnTotal, alnCap); return HTKAMD_EINVAL; }
   if (alnTotal > ((long long)1 << 30) / 3) { htkamd_set_error("results_score: %lld labels in one call", alnTotal); return HTKAMD_EINVAL; }
   if (maxDir > RES_MAXSCRATCH / RES_WAVES) { htkamd_set_error("results_score: a pair of %zu grid cells is too long for the alignment scratch", maxDir); return HTKAMD_EINVAL; }
   if (totals) memset(totals, 0, sizeof(long long) * 7 * (size_t)K);
   if (wantConf) memset(conf, 0, sizeof(int) * (size_t)K * W * W);
   if (wantAln) memset(alnOff, 0, sizeof(int) * ((size_t)nPairs + 1));
   r->kernelMs = 0.0;
   if (nPairs == 0) return HTKAMD_OK;
   if (htkamd_device_count() <= 0) { htkamd_set_error("results_score: no HIP device"); return HTKAMD_ENODEV; }
   if (!r->dev) { r->dev = new ResDev(); r->devFree = res_dev_free; }
   ResDev &D = *(ResDev *)r->dev;
   hipStream_t st = (hipStream_t)stream;
   int blocks = (nPairs + RES_WAVES - 1) / RES_WAVES;
   if (blocks > RES_MAXBLOCKS) blocks = RES_MAXBLOCKS;
   maxDir = (maxDir + 255) & ~(size_t)255;
   if (maxDir > 0 && (size_t)blocks * RES_WAVES * maxDir > RES_MAXSCRATCH) blocks = (int)(RES_MAXSCRATCH / (RES_WAVES * maxDir));
   if (blocks < 1) blocks = 1;
   const size_t slots = (size_t)blocks * RES_WAVES, bndStride = (size_t)(maxBndT + 1);
   int rc;
   const size_t nP = (size_t)nPairs, nTot = 7 * (size_t)K, nConf = (size_t)K * W * W;
   if (r->refsOnDevice != r->nRefs) {
      if ((rc = D.refs.upload(r->refIds, (size_t)r->refOff[r->nRefs], st))) return rc;
      HIPCHECK(hipStreamSynchronize(st));                     // (the host array may move when a reference is added)
      r->refsOnDevice = r->nRefs;
   }
   if ((rc = D.hyps.upload(hypIds, (size_t)nHyp, st))) return rc;
   if ((rc = D.pairs.upload(pd, st))) return rc;
   if ((rc = D.counts.reserve<int>(6 * nP))) return rc;
   if ((rc = D.totals.reserve<unsigned long long>(nTot))) return rc;
   if (wantDir && (rc = D.aln.reserve<int>(3 * (size_t)alnTotal))) return rc;
   if (wantDir && (rc = D.alnLen.reserve<int>(nP))) return rc;
   if (wantConf && (rc = D.conf.reserve<int>(nConf))) return rc;
   if (maxDir > 0 && (rc = D.dir.reserve<unsigned char>(slots * maxDir))) return rc;
   if (maxBndT >= 0 && (rc = D.bnd.reserve<Cell>(slots * 2 * bndStride))) return rc;
   HIPCHECK(hipMemsetAsync(D.totals.p, 0, sizeof(unsigned long long) * nTot, st));
   if (wantConf) HIPCHECK(hipMemsetAsync(D.conf.p, 0, sizeof(int) * nConf, st));
   HIPCHECK(D.timer.start(st));
   auto kern = r->nist ? k_results_align<true> : k_results_align<false>;
   hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(RES_WAVES * 64), 0, st, D.pairs.as<const PairDesc>(), nPairs, D.refs.as<const int>(), D.hyps.as<const int>(), (int)wantDir,
                      maxDir > 0 ? D.dir.as<unsigned char>() : nullptr, maxDir, maxBndT >= 0 ? D.bnd.as<Cell>() : nullptr, bndStride, D.counts.as<int>(),
                      wantDir ? D.aln.as<int>() : nullptr, wantDir ? D.alnLen.as<int>() : nullptr);
   HIPCHECK(hipGetLastError());
   hipLaunchKernelGGL(k_results_totals, dim3((unsigned)((U + 255) / 256), (unsigned)K), dim3(256), 0, st, D.counts.as<const int>(), U, D.totals.as<unsigned long long>(),
                      D.pairs.as<const PairDesc>(), D.aln.as<const int>(), D.alnLen.as<const int>(), wantConf ? D.conf.as<int>() : nullptr, V);
   HIPCHECK(hipGetLastError());
   HIPCHECK(D.timer.stop(st));
   std::vector<int> hCounts, hLen, hAln;
   int *cnt = counts;
   if (!cnt) { hCounts.resize(6 * nP); cnt = hCounts.data(); }
   if ((rc = D.counts.download(cnt, 6 * nP, st))) return rc;
   if (totals && (rc = D.totals.download((unsigned long long *)totals, nTot, st))) return rc;
   if (wantConf && (rc = D.conf.download(conf, nConf, st))) return rc;
   if (wantAln) {
      hLen.resize(nP); hAln.resize(3 * (size_t)alnTotal + 1);
      if ((rc = D.alnLen.download(hLen.data(), nP, st)) || (rc = D.aln.download(hAln.data(), 3 * (size_t)alnTotal, st))) return rc;
   }
   HIPCHECK(hipStreamSynchronize(st));
   float ms = 0.0f;
   HIPCHECK(D.timer.ms(&ms));
   r->kernelMs = ms;
   if (wantAln) {                                             // the pairs' triples, closed up
      int at = 0;
      for (int p = 0; p < nPairs; p++) {
         const PairDesc &d = pd[(size_t)p];
         const int n = hLen[(size_t)p];
         if (n < 0 || n > d.nRef + d.nTest) { htkamd_set_error("results_score: pair %d came back with %d alignment steps", p, n); return HTKAMD_EHIP; }
         alnOff[p] = at;
         if (n) memcpy(aln + 3 * (size_t)at, hAln.data() + 3 * (size_t)(d.alnPos + d.nRef + d.nTest - n), sizeof(int) * 3 * (size_t)n);
         at += n;
      }
      alnOff[nPairs] = at;
   }
   return HTKAMD_OK;
}
