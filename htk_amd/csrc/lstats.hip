// lstats.hip -- HLStats' counting for a batch of label sequences in one call (htkamd_lstats_count): what GatherStats (HLStats.c:471) adds
// up label by label into a hash table of bigrams, as a sorted CSR table.
//
// An ITEM is a label position of the batch, or (items nLab .. nLab + nUtt) the transition into the exit word that closes an utterance.
// ls_item gives an item's (predecessor, word) as GatherStats sees it: a leading enter word and a trailing exit word are skipped, the
// predecessor of the first label is the enter word, and an enter or exit word in mid-sentence is counted but starts and ends no bigram.
//   k_ls_unigram   per item: word count, duration sum / min / max (64-bit integers, 100 ns units), length of the predecessor's row;
//   k_lm_scan      row lengths -> each row's bucket;
//   k_ls_scatter   per item: the word into the predecessor's bucket (the order inside a bucket is whatever the atomics give);
//   k_ls_rows      sorts a bucket by word and run-length encodes it into (word, count).  One WAVEFRONT per row of up to LS_WAVE_CAP pairs,
//                  bitonic sort in the wavefront's LDS tile: 4 KiB a wavefront, so that the 32 wavefronts a CU holds use 128 of its 160 KiB.
//                  One WORKGROUP per longer row of up to LS_GROUP_CAP pairs (32 KiB tile, five workgroups a CU).  A row longer than that
//                  is counted instead of sorted: the tile becomes a histogram over a window of LS_GROUP_CAP word ids, the bucket is
//                  streamed from global memory once per window, and the windows' non-zero bins follow each other in word order;
//   k_lm_scan      distinct successors per row -> CSR offsets;   k_ls_compact closes the rows up.
// Everything is integer and every row ends up sorted: the result does not depend on the order of anything.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "hipcheck.h"
#include "devbuf.h"
#include "lstats.h"
#include "lmscan.h"

DEVBUF_OWNER("lstats")

#define LS_WAVES      4
#define LS_WAVE_CAP   1024        // pairs a wavefront sorts in its LDS tile
#define LS_GROUP_CAP  8192        // pairs a workgroup sorts in its tile; also the width of the histogram window
#define LS_THREADS    256
#define LS_MAXBLOCKS  2048

struct LsBatch { const int *off, *ids; int nUtt, nLab, enterId, exitId; };

// the utterance of label position p: off[u] <= p < off[u + 1]
__device__ __forceinline__ int ls_utt_of(const int *__restrict__ off, int nUtt, int p)
{
   int lo = 0, hi = nUtt;
   while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= p) lo = mid; else hi = mid; }
   return lo;
}

// counted: the item is a label that GatherStats' loop visits (word = its id, pos = its position); returns whether it ends a bigram (pred, word)
__device__ __forceinline__ bool ls_item(const LsBatch &B, int item, int &pred, int &word, int &pos, bool &counted)
{
   const bool closing = item >= B.nLab;
   const int u = closing ? item - B.nLab : ls_utt_of(B.off, B.nUtt, item);
   const int b = B.off[u], e = B.off[u + 1];
   int st = b, en = e;
   if (e > b) { if (B.ids[b] == B.enterId) st++; if (B.ids[e - 1] == B.exitId) en--; }
   counted = false;
   if (closing) { word = B.exitId; pos = en; }
   else {
      pos = item;
      if (pos < st || pos >= en) return false;
      word = B.ids[pos];
      counted = true;
      if (word == B.enterId || word == B.exitId) return false;
   }
   pred = B.enterId;
   for (int q = pos - 1; q >= st; q--) { const int x = B.ids[q]; if (x != B.enterId && x != B.exitId) { pred = x; break; } }
   return true;
}

__global__ __launch_bounds__(LS_THREADS) void k_ls_unigram(LsBatch B, const long long *__restrict__ start, const long long *__restrict__ end, int *__restrict__ count,
                                                           int *__restrict__ rowLen, long long *__restrict__ durSum, long long *__restrict__ durMin, long long *__restrict__ durMax,
                                                           int *__restrict__ durOdd)
{
   const int nItems = B.nLab + B.nUtt, stride = (int)(gridDim.x * blockDim.x);
   for (int item = (int)(blockIdx.x * blockDim.x + threadIdx.x); item < nItems; item += stride) {
      int pred = 0, word = 0, pos = 0; bool counted;
      if (ls_item(B, item, pred, word, pos, counted)) atomicAdd(&rowLen[pred], 1);
      if (counted) {
         atomicAdd(&count[word], 1);
         if (start) {
            const long long d = end[pos] - start[pos];
            atomicAdd((unsigned long long *)&durSum[word], (unsigned long long)d);
            atomicMin(&durMin[word], d);
            atomicMax(&durMax[word], d);
            if (d < 0 || d % 10000 != 0) atomicAdd(durOdd, 1);      // not a whole number of milliseconds: see OutputDurs in host/lstats.c
         }
      }
   }
}

__global__ __launch_bounds__(LS_THREADS) void k_ls_scatter(LsBatch B, const int *__restrict__ rowOff, int *__restrict__ cursor, int *__restrict__ bucket)
{
   const int nItems = B.nLab + B.nUtt, stride = (int)(gridDim.x * blockDim.x);
   for (int item = (int)(blockIdx.x * blockDim.x + threadIdx.x); item < nItems; item += stride) {
      int pred = 0, word = 0, pos = 0; bool counted;
      if (!ls_item(B, item, pred, word, pos, counted)) continue;
      const int slot = rowOff[pred] + atomicAdd(&cursor[pred], 1);
      if (slot < rowOff[pred + 1]) bucket[slot] = word;
   }
}

template <bool GROUP> __device__ __forceinline__ void ls_sync()
{
   if (GROUP) __syncthreads();
   else { __threadfence_block(); __builtin_amdgcn_wave_barrier(); }
}

// inclusive scan of v over the row's threads (a wavefront, or the workgroup's four); total = the sum
template <bool GROUP> __device__ __forceinline__ int ls_scan(int v, int tid, int *sScan, int &total)
{
   const int lane = tid & 63;
   int incl = lm_wave_incl_scan(v, lane);
   if (!GROUP) { total = __shfl(incl, 63, 64); return incl; }
   const int w = tid >> 6;
   if (lane == 63) sScan[w] = incl;
   __syncthreads();
   int before = 0; total = 0;
   for (int k = 0; k < LS_WAVES; k++) { const int s = sScan[k]; total += s; if (k < w) before += s; }
   __syncthreads();
   return before + incl;
}

// n <= the tile: sort, then one (word, count) per run
template <bool GROUP> __device__ __forceinline__ int ls_sort_rle(int *tile, const int *__restrict__ bucket, int n, int tid, int *__restrict__ outWord, int *__restrict__ outCnt, int *sScan)
{
   constexpr int NT = GROUP ? LS_THREADS : 64;
   int m = 1;
   while (m < n) m <<= 1;
   for (int i = tid; i < m; i += NT) tile[i] = i < n ? bucket[i] : INT_MAX;
   ls_sync<GROUP>();
   for (int k = 2; k <= m; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
         for (int i = tid; i < m; i += NT) {
            const int p = i ^ j;
            if (p > i) {
               const int a = tile[i], b = tile[p];
               if ((a > b) == ((i & k) == 0)) { tile[i] = b; tile[p] = a; }
            }
         }
         ls_sync<GROUP>();
      }
   int runs = 0;
   for (int base = 0; base < n; base += NT) {
      const int i = base + tid;
      const int v = i < n ? tile[i] : 0;
      const bool head = i < n && (i == 0 || tile[i - 1] != v);
      int total;
      const int incl = ls_scan<GROUP>(head, tid, sScan, total);
      if (head) {
         int lo = i + 1, hi = n;                              // the run's end
         while (lo < hi) { const int mid = (lo + hi) >> 1; if (tile[mid] <= v) lo = mid + 1; else hi = mid; }
         outWord[runs + incl - 1] = v; outCnt[runs + incl - 1] = lo - i;
      }
      runs += total;
   }
   return runs;
}

// a row of any length, by a workgroup: a histogram over `width` word ids at a time
__device__ __forceinline__ int ls_hist_rle(int *tile, const int *__restrict__ bucket, int n, int V, int width, int tid, int *__restrict__ outWord, int *__restrict__ outCnt, int *sScan)
{
   int runs = 0;
   for (int lo = 0; lo < V; lo += width) {
      for (int i = tid; i < width; i += LS_THREADS) tile[i] = 0;
      __syncthreads();
      for (int i = tid; i < n; i += LS_THREADS) { const int x = bucket[i] - lo; if (x >= 0 && x < width) atomicAdd(&tile[x], 1); }
      __syncthreads();
      const int top = V - lo < width ? V - lo : width;
      for (int base = 0; base < top; base += LS_THREADS) {
         const int j = base + tid;
         const int c = j < top ? tile[j] : 0;
         int total;
         const int incl = ls_scan<true>(c > 0, tid, sScan, total);
         if (c > 0) { outWord[runs + incl - 1] = lo + j; outCnt[runs + incl - 1] = c; }
         runs += total;
      }
      __syncthreads();
   }
   return runs;
}

// GROUP = false: a wavefront per row of 1..waveCap pairs.  GROUP = true: a workgroup per longer row.
template <bool GROUP>
__global__ __launch_bounds__(LS_THREADS) void k_ls_rows(const int *__restrict__ rowOff, int V, const int *__restrict__ bucket, int waveCap, int groupCap,
                                                        int *__restrict__ rleWord, int *__restrict__ rleCnt, int *__restrict__ nDistinct)
{
   __shared__ int sTile[GROUP ? LS_GROUP_CAP : LS_WAVES * LS_WAVE_CAP];
   __shared__ int sScan[LS_WAVES];
   const int tid = (int)threadIdx.x;
   if (GROUP) {
      for (int r = (int)blockIdx.x; r < V; r += (int)gridDim.x) {
         const int b = rowOff[r], n = rowOff[r + 1] - b;
         if (n <= waveCap) continue;
         const int runs = n <= groupCap ? ls_sort_rle<true>(sTile, bucket + b, n, tid, rleWord + b, rleCnt + b, sScan)
                                        : ls_hist_rle(sTile, bucket + b, n, V, groupCap, tid, rleWord + b, rleCnt + b, sScan);
         if (tid == 0) nDistinct[r] = runs;
         __syncthreads();
      }
   } else {
      const int w = tid >> 6, lane = tid & 63;
      int *tile = sTile + w * LS_WAVE_CAP;
      for (int r = (int)blockIdx.x * LS_WAVES + w; r < V; r += (int)gridDim.x * LS_WAVES) {
         const int b = rowOff[r], n = rowOff[r + 1] - b;
         if (n <= 0 || n > waveCap) continue;
         const int runs = ls_sort_rle<false>(tile, bucket + b, n, lane, rleWord + b, rleCnt + b, sScan);
         if (lane == 0) nDistinct[r] = runs;
         ls_sync<false>();                                    // the tile is the next row's
      }
   }
}

// a wavefront per row: the row's runs to their place in the CSR table
__global__ __launch_bounds__(LS_THREADS) void k_ls_compact(const int *__restrict__ rowOff, const int *__restrict__ csrOff, int V, const int *__restrict__ rleWord,
                                                           const int *__restrict__ rleCnt, int *__restrict__ succ, int *__restrict__ cnt)
{
   const int w = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
   for (int r = (int)blockIdx.x * LS_WAVES + w; r < V; r += (int)gridDim.x * LS_WAVES) {
      const int from = rowOff[r], to = csrOff[r], n = csrOff[r + 1] - to;
      for (int i = lane; i < n; i += 64) { succ[to + i] = rleWord[from + i]; cnt[to + i] = rleCnt[from + i]; }
   }
}

struct LsDev {
   DevBuf off, ids, start, end, count, rowLen, rowOff, cursor, bucket, rleWord, rleCnt, nDistinct, csrOff, succ, cnt, durSum, durMin, durMax, durOdd;
   KernelTimer timer;
};

extern "C" void htkamd_lstats_device_free(void *dev) { delete (LsDev *)dev; }
extern "C" int htkamd_lstats_wave_cap(void) { return LS_WAVE_CAP; }
extern "C" int htkamd_lstats_group_cap(void) { return LS_GROUP_CAP; }

static int grid_for(long long n, int per, int most) { long long b = (n + per - 1) / per; return (int)(b < 1 ? 1 : (b > most ? most : b)); }

extern "C" int htkamd_lstats_device(void **devp, int V, int nUtt, const int *labOff, const int *labIds, const long long *start, const long long *end, int enterId, int exitId,
                                    int waveCap, int groupCap, int *count, long long *durSum, long long *durMin, long long *durMax, int *rowOffOut, int **succOut, int **cntOut,
                                    int *durOdd, double *kernelMs, void *stream)
{
   // every index a kernel will form, checked here
   if (V < 1 || V > 65536 || nUtt < 0 || (nUtt > 0 && !labOff) || !count || !rowOffOut || !succOut || !cntOut) { htkamd_set_error("lstats: bad argument"); return HTKAMD_EINVAL; }
   if (enterId < 0 || enterId >= V || exitId < 0 || exitId >= V || enterId == exitId) { htkamd_set_error("lstats: boundary words %d and %d of %d", enterId, exitId, V); return HTKAMD_EINVAL; }
   if (waveCap < 1 || waveCap > LS_WAVE_CAP || groupCap < waveCap || groupCap > LS_GROUP_CAP) { htkamd_set_error("lstats: capacities %d / %d (at most %d / %d)", waveCap, groupCap, LS_WAVE_CAP, LS_GROUP_CAP); return HTKAMD_EINVAL; }
   if ((start == NULL) != (end == NULL) || (start && !(durSum && durMin && durMax))) { htkamd_set_error("lstats: the label times come as start AND end, with all three duration outputs"); return HTKAMD_EINVAL; }
   if (nUtt > 0 && labOff[0] != 0) { htkamd_set_error("lstats: the labels do not start at 0"); return HTKAMD_EINVAL; }
   for (int u = 0; u < nUtt; u++) if (labOff[u + 1] < labOff[u]) { htkamd_set_error("lstats: the offsets of utterance %d run backwards", u); return HTKAMD_EINVAL; }
   const int nLab = nUtt > 0 ? labOff[nUtt] : 0;
   if ((long long)nLab + nUtt > ((long long)1 << 30)) { htkamd_set_error("lstats: %d labels in one call", nLab); return HTKAMD_EINVAL; }
   if (nLab > 0 && !labIds) { htkamd_set_error("lstats: bad argument"); return HTKAMD_EINVAL; }
   for (int k = 0; k < nLab; k++) if (labIds[k] < 0 || labIds[k] >= V) { htkamd_set_error("lstats: label %d has id %d (the list has %d)", k, labIds[k], V); return HTKAMD_EINVAL; }
   const size_t nV = (size_t)V;
   memset(count, 0, sizeof(int) * nV);
   memset(rowOffOut, 0, sizeof(int) * (nV + 1));
   *succOut = *cntOut = NULL;
   if (durOdd) *durOdd = 0;
   if (kernelMs) *kernelMs = 0.0;
   std::vector<long long> mn(nV, LLONG_MAX), mx(nV, LLONG_MIN);
   if (start) { memset(durSum, 0, sizeof(long long) * nV); memcpy(durMin, mn.data(), sizeof(long long) * nV); memcpy(durMax, mx.data(), sizeof(long long) * nV); }
   if (nUtt == 0) return HTKAMD_OK;
   if (htkamd_device_count() <= 0) { htkamd_set_error("lstats: no HIP device"); return HTKAMD_ENODEV; }
   LsDev *own = NULL;
   if (!devp) own = new LsDev();
   else if (!*devp) *devp = new LsDev();
   LsDev &D = own ? *own : *(LsDev *)*devp;
   struct Guard { LsDev *p; ~Guard() { delete p; } } guard{own};
   hipStream_t st = (hipStream_t)stream;
   const size_t nPairs = (size_t)nLab + (size_t)nUtt;        // at most this many bigram tokens
   int rc;
   if ((rc = D.off.upload(labOff, (size_t)nUtt + 1, st)) || (rc = D.ids.upload(labIds, (size_t)nLab, st))) return rc;
   if (start && ((rc = D.start.upload(start, (size_t)nLab, st)) || (rc = D.end.upload(end, (size_t)nLab, st)))) return rc;
   if ((rc = D.count.reserve<int>(nV)) || (rc = D.rowLen.reserve<int>(nV + 1)) || (rc = D.rowOff.reserve<int>(nV + 1)) || (rc = D.cursor.reserve<int>(nV)) ||
       (rc = D.nDistinct.reserve<int>(nV + 1)) || (rc = D.csrOff.reserve<int>(nV + 1)) || (rc = D.bucket.reserve<int>(nPairs)) || (rc = D.rleWord.reserve<int>(nPairs)) ||
       (rc = D.rleCnt.reserve<int>(nPairs)) || (rc = D.succ.reserve<int>(nPairs)) || (rc = D.cnt.reserve<int>(nPairs)))
      return rc;
   if (start) {
      if ((rc = D.durSum.reserve<long long>(nV)) || (rc = D.durMin.upload(mn, st)) || (rc = D.durMax.upload(mx, st))) return rc;
      HIPCHECK(hipMemsetAsync(D.durSum.p, 0, sizeof(long long) * nV, st));
      if ((rc = D.durOdd.reserve<int>(1))) return rc;
      HIPCHECK(hipMemsetAsync(D.durOdd.p, 0, sizeof(int), st));
   }
   HIPCHECK(hipMemsetAsync(D.count.p, 0, sizeof(int) * nV, st));
   HIPCHECK(hipMemsetAsync(D.rowLen.p, 0, sizeof(int) * (nV + 1), st));
   HIPCHECK(hipMemsetAsync(D.cursor.p, 0, sizeof(int) * nV, st));
   HIPCHECK(hipMemsetAsync(D.nDistinct.p, 0, sizeof(int) * (nV + 1), st));
   const LsBatch B = {D.off.as<const int>(), D.ids.as<const int>(), nUtt, nLab, enterId, exitId};
   const int itemBlocks = grid_for((long long)nPairs, LS_THREADS, LS_MAXBLOCKS), rowBlocks = grid_for(V, LS_WAVES, LS_MAXBLOCKS), longBlocks = grid_for(V, 1, 1024);
   HIPCHECK(D.timer.start(st));
   hipLaunchKernelGGL(k_ls_unigram, dim3((unsigned)itemBlocks), dim3(LS_THREADS), 0, st, B, start ? D.start.as<const long long>() : nullptr, start ? D.end.as<const long long>() : nullptr,
                      D.count.as<int>(), D.rowLen.as<int>(), D.durSum.as<long long>(), D.durMin.as<long long>(), D.durMax.as<long long>(), D.durOdd.as<int>());
   HIPCHECK(hipGetLastError());
   hipLaunchKernelGGL(k_lm_scan, dim3(1), dim3(1024), 0, st, D.rowLen.as<const int>(), D.rowOff.as<int>(), V);
   HIPCHECK(hipGetLastError());
   hipLaunchKernelGGL(k_ls_scatter, dim3((unsigned)itemBlocks), dim3(LS_THREADS), 0, st, B, D.rowOff.as<const int>(), D.cursor.as<int>(), D.bucket.as<int>());
   HIPCHECK(hipGetLastError());
   hipLaunchKernelGGL(k_ls_rows<false>, dim3((unsigned)rowBlocks), dim3(LS_THREADS), 0, st, D.rowOff.as<const int>(), V, D.bucket.as<const int>(), waveCap, groupCap,
                      D.rleWord.as<int>(), D.rleCnt.as<int>(), D.nDistinct.as<int>());
   HIPCHECK(hipGetLastError());
   hipLaunchKernelGGL(k_ls_rows<true>, dim3((unsigned)longBlocks), dim3(LS_THREADS), 0, st, D.rowOff.as<const int>(), V, D.bucket.as<const int>(), waveCap, groupCap,
                      D.rleWord.as<int>(), D.rleCnt.as<int>(), D.nDistinct.as<int>());
   HIPCHECK(hipGetLastError());
   hipLaunchKernelGGL(k_lm_scan, dim3(1), dim3(1024), 0, st, D.nDistinct.as<const int>(), D.csrOff.as<int>(), V);
   HIPCHECK(hipGetLastError());
   hipLaunchKernelGGL(k_ls_compact, dim3((unsigned)rowBlocks), dim3(LS_THREADS), 0, st, D.rowOff.as<const int>(), D.csrOff.as<const int>(), V, D.rleWord.as<const int>(),
                      D.rleCnt.as<const int>(), D.succ.as<int>(), D.cnt.as<int>());
   HIPCHECK(hipGetLastError());
   HIPCHECK(D.timer.stop(st));
   if ((rc = D.count.download(count, nV, st)) || (rc = D.csrOff.download(rowOffOut, nV + 1, st))) return rc;
   if (start && ((rc = D.durSum.download(durSum, nV, st)) || (rc = D.durMin.download(durMin, nV, st)) || (rc = D.durMax.download(durMax, nV, st)))) return rc;
   int odd = 0;
   if (start && (rc = D.durOdd.download(&odd, 1, st))) return rc;
   HIPCHECK(hipStreamSynchronize(st));
   if (durOdd) *durOdd = odd;
   const int total = rowOffOut[V];
   if (total < 0 || (size_t)total > nPairs) { htkamd_set_error("lstats: the table came back with %d entries for %zu pairs", total, nPairs); return HTKAMD_EHIP; }
   int *hs = (int *)malloc(sizeof(int) * (size_t)(total ? total : 1)), *hc = (int *)malloc(sizeof(int) * (size_t)(total ? total : 1));
   if (!hs || !hc) { free(hs); free(hc); htkamd_set_error("lstats: out of memory"); return HTKAMD_ENOMEM; }
   rc = D.succ.download(hs, (size_t)total, st);
   if (!rc) rc = D.cnt.download(hc, (size_t)total, st);
   HIPCHECK_RC(rc, "lstats", hipStreamSynchronize(st));
   float ms = 0.0f;
   HIPCHECK_RC(rc, "lstats", D.timer.ms(&ms));
   if (rc) { free(hs); free(hc); return rc; }
   if (kernelMs) *kernelMs = ms;
   *succOut = hs; *cntOut = hc;
   return HTKAMD_OK;
}
