// treesynth.hip -- the device side of HHEd's AU command (the driver is host/treeclust.c): which leaf of which tree every state of every
// unseen model name ends in.
//
// AssignStructure (HHEd.c:3115) walks a tree by asking QMatch (:458) at every node: DoMatch (HShell.c:1806) of the model's name against
// each pattern of the node's question, pattern by pattern, for every name.  Here the answers are made once per (question, name) and the
// walks read them.
//
// k_name_answers: block (x = 256 names, y = a block of SY_QB questions), a lane per name.  Names and patterns are NUL-terminated strings
//   in byte pools with offset tables.  The patterns of the block's questions are one contiguous piece of the pattern pool: it is staged
//   in LDS once (every lane reads the same patterns, but after the first mismatch not at the same place: LDS takes the scattered byte
//   reads, the offset tables stay wave-uniform loads).  A lane reads its own name from memory (a few bytes, the wavefront's names are
//   neighbours in the pool).  The matcher is tc_match of host/treeclust.c statement for statement: iterative, the last '*' and the place
//   in the name it was tried at are the only state -- nothing recursive, no scratch.  A lane leaves a question at its first matching
//   pattern; lanes of a wavefront differ in how long they loop (the divergence is the data's, names of one list are alike).
//   answers[q][n] is one byte, the layout htkamd_tree_split_sums takes.
// k_tree_descend: a lane per (name, tree) pair.  The trees' node tables (quest / no / yes, a child >= 0 a node, < 0 the leaf -1-k) lie
//   behind one another, treeOff[t] the first node of tree t; a tree without nodes is its single leaf 0.  pairTree -1 = no tree: leaf -1.
//   The walk is bounded by the tree's node count (the host has checked that the tables are trees; the bound costs nothing).
// Plain loads and byte / int stores only.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include "internal.h"
#include "hipcheck.h"
#include "devbuf.h"

#define SY_THREADS 256
#define SY_QB      4                                    // questions per block
#define SY_LDS_MAX 49152                                // bytes of patterns a block of questions may hold

// DoMatch / RMatch (HShell.c:1787-1816) as tc_match restates them: '*' any run (also empty), '?' one character
static __device__ int sy_match(const char *s, const char *p)
{
   int si = 0, pi = 0, star = -1, back = 0;
   while (s[si]) {
      const char pc = p[pi];
      if (pc == '*') { star = pi++; back = si; }
      else if (pc == '?' || pc == s[si]) { pi++; si++; }
      else if (star >= 0) { pi = star + 1; si = ++back; }
      else return 0;
   }
   while (p[pi] == '*') pi++;
   return p[pi] == 0;
}

__global__ __launch_bounds__(SY_THREADS) void k_name_answers(const char *namePool, const int *nameOff, int N, const char *patPool, const int *patOff,
                                                              const int *qPat, int nQ, unsigned char *answers)
{
   extern __shared__ char pats[];
   const int q0 = blockIdx.y * SY_QB, q1 = (q0 + SY_QB < nQ) ? q0 + SY_QB : nQ;
   const int b0 = patOff[qPat[q0]], b1 = patOff[qPat[q1]];       // the block's piece of the pattern pool
   for (int i = threadIdx.x; i < b1 - b0; i += SY_THREADS) pats[i] = patPool[b0 + i];
   __syncthreads();
   const int n = blockIdx.x * SY_THREADS + threadIdx.x;
   if (n >= N) return;
   const char *name = namePool + nameOff[n];
   for (int q = q0; q < q1; q++) {
      int a = 0;
      for (int k = qPat[q]; k < qPat[q + 1] && !a; k++) a = sy_match(name, pats + (patOff[k] - b0));
      answers[(size_t)q * N + n] = (unsigned char)a;
   }
}

__global__ __launch_bounds__(SY_THREADS) void k_tree_descend(const unsigned char *answers, int N, const int *treeOff, const int *quest, const int *no, const int *yes,
                                                              const int *pairName, const int *pairTree, int nPairs, int *leaf)
{
   const int i = blockIdx.x * SY_THREADS + threadIdx.x;
   if (i >= nPairs) return;
   const int t = pairTree[i], n = pairName[i];
   int out = -1;
   if (t >= 0) {
      const int off = treeOff[t], nNodes = treeOff[t + 1] - off;
      if (nNodes == 0) out = 0;
      int node = 0;
      for (int step = 0; step < nNodes; step++) {
         const int c = answers[(size_t)quest[off + node] * N + n] ? yes[off + node] : no[off + node];
         if (c < 0) { out = -1 - c; break; }
         node = c;
      }
   }
   leaf[i] = out;
}

DEVBUF_OWNER("add_unseen")
namespace { float g_kernelMs[2]; }

extern "C" void htkamd_synth_last_kernel_ms(float *ms) { if (ms) { ms[0] = g_kernelMs[0]; ms[1] = g_kernelMs[1]; } }

extern "C" int htkamd_synth_dev_run(const htkamd_synth_job *j, unsigned char *answers, int *leaf, void *stream)
{
   if (!j || j->N < 1 || j->nQ < 0 || !j->namePool || !j->nameOff || (j->nQ > 0 && (!j->patPool || !j->patOff || !j->qPat)) || j->nPairs < 0 || j->nTrees < 0 ||
       (j->nPairs > 0 && (!j->pairName || !j->pairTree || !leaf)) || (j->nTrees > 0 && !j->treeOff)) { htkamd_set_error("add_unseen: bad job"); return HTKAMD_EINVAL; }
   // every index a kernel will form, checked here
   const int N = j->N, nQ = j->nQ;
   if (j->nameOff[0] != 0) { htkamd_set_error("add_unseen: the name pool does not start at 0"); return HTKAMD_EINVAL; }
   for (int n = 0; n < N; n++) {
      const long long len = (long long)j->nameOff[n + 1] - j->nameOff[n] - 1;
      if (len < 0 || j->namePool[j->nameOff[n + 1] - 1] != 0 || (long long)strlen(j->namePool + j->nameOff[n]) != len) { htkamd_set_error("add_unseen: name %d is not terminated in the pool", n); return HTKAMD_EINVAL; }
      if (len > HTKAMD_SYNTH_MAXNAME) { htkamd_set_error("add_unseen: the name %.40s... has %lld characters (at most %d)", j->namePool + j->nameOff[n], len, HTKAMD_SYNTH_MAXNAME); return HTKAMD_EINVAL; }
   }
   int nPat = 0;
   size_t ldsBytes = 0;
   if (nQ > 0) {
      nPat = j->qPat[nQ];
      if (j->qPat[0] != 0 || nPat < 1 || j->patOff[0] != 0) { htkamd_set_error("add_unseen: bad pattern tables"); return HTKAMD_EINVAL; }
      for (int q = 0; q < nQ; q++) if (j->qPat[q + 1] <= j->qPat[q]) { htkamd_set_error("add_unseen: question %d has no pattern", q); return HTKAMD_EINVAL; }
      for (int k = 0; k < nPat; k++) {
         const long long len = (long long)j->patOff[k + 1] - j->patOff[k] - 1;
         if (len < 0 || j->patPool[j->patOff[k + 1] - 1] != 0 || (long long)strlen(j->patPool + j->patOff[k]) != len) { htkamd_set_error("add_unseen: pattern %d is not terminated in the pool", k); return HTKAMD_EINVAL; }
      }
      for (int q0 = 0; q0 < nQ; q0 += SY_QB) {
         const int q1 = (q0 + SY_QB < nQ) ? q0 + SY_QB : nQ;
         const size_t b = (size_t)(j->patOff[j->qPat[q1]] - j->patOff[j->qPat[q0]]);
         if (b > SY_LDS_MAX) { htkamd_set_error("add_unseen: the patterns of questions %d to %d take %zu bytes (at most %d for %d questions)", q0, q1 - 1, b, SY_LDS_MAX, SY_QB); return HTKAMD_EINVAL; }
         if (b > ldsBytes) ldsBytes = b;
      }
      if ((nQ + SY_QB - 1) / SY_QB > 65535) { htkamd_set_error("add_unseen: %d questions", nQ); return HTKAMD_EINVAL; }
   }
   int nNodes = 0;
   if (j->nTrees > 0) {
      nNodes = j->treeOff[j->nTrees];
      if (j->treeOff[0] != 0 || nNodes < 0 || (nNodes > 0 && (!j->quest || !j->no || !j->yes))) { htkamd_set_error("add_unseen: bad tree tables"); return HTKAMD_EINVAL; }
      for (int t = 0; t < j->nTrees; t++) {
         const int off = j->treeOff[t], n = j->treeOff[t + 1] - off, nl = j->treeLeaves ? j->treeLeaves[t] : n + 1;
         if (n < 0) { htkamd_set_error("add_unseen: bad tree tables"); return HTKAMD_EINVAL; }
         for (int k = 0; k < n; k++) {
            const int a = j->no[off + k], b = j->yes[off + k], q = j->quest[off + k];
            if (q < 0 || q >= nQ || a >= n || b >= n || -1 - a >= nl || -1 - b >= nl) { htkamd_set_error("add_unseen: node %d of tree %d reaches outside its tables", k, t); return HTKAMD_EINVAL; }
         }
      }
   }
   for (int i = 0; i < j->nPairs; i++)
      if (j->pairName[i] < 0 || j->pairName[i] >= N || j->pairTree[i] < -1 || j->pairTree[i] >= j->nTrees) { htkamd_set_error("add_unseen: pair %d names model %d of %d, tree %d of %d", i, j->pairName[i], N, j->pairTree[i], j->nTrees); return HTKAMD_EINVAL; }
   if (htkamd_device_count() <= 0) { htkamd_set_error("add_unseen: no HIP device"); return HTKAMD_ENODEV; }
   hipStream_t st = (hipStream_t)stream;
   DevBuf dNames, dNameOff, dPats, dPatOff, dQPat, dAns, dTreeOff, dQuest, dNo, dYes, dPairName, dPairTree, dLeaf;
   KernelTimer tAns, tLeaf;
   int rc;
   if ((rc = dNames.upload(j->namePool, (size_t)j->nameOff[N], st))) return rc;
   if ((rc = dNameOff.upload(j->nameOff, (size_t)N + 1, st))) return rc;
   if ((rc = dAns.reserve<unsigned char>((size_t)nQ * N))) return rc;
   g_kernelMs[0] = g_kernelMs[1] = 0.0f;
   if (nQ > 0) {
      if ((rc = dPats.upload(j->patPool, (size_t)j->patOff[nPat], st))) return rc;
      if ((rc = dPatOff.upload(j->patOff, (size_t)nPat + 1, st))) return rc;
      if ((rc = dQPat.upload(j->qPat, (size_t)nQ + 1, st))) return rc;
      HIPCHECK(tAns.start(st));
      hipLaunchKernelGGL(k_name_answers, dim3((unsigned)((N + SY_THREADS - 1) / SY_THREADS), (unsigned)((nQ + SY_QB - 1) / SY_QB)), dim3(SY_THREADS), ldsBytes, st,
                         dNames.as<const char>(), dNameOff.as<const int>(), N, dPats.as<const char>(), dPatOff.as<const int>(), dQPat.as<const int>(), nQ, dAns.as<unsigned char>());
      HIPCHECK(hipGetLastError());
      HIPCHECK(tAns.stop(st));
      if (answers && (rc = dAns.download(answers, (size_t)nQ * N, st))) return rc;
   }
   if (j->nPairs > 0) {
      if ((rc = dTreeOff.upload(j->treeOff, (size_t)j->nTrees + 1, st))) return rc;
      if ((rc = dQuest.upload(j->quest, (size_t)nNodes, st))) return rc;
      if ((rc = dNo.upload(j->no, (size_t)nNodes, st))) return rc;
      if ((rc = dYes.upload(j->yes, (size_t)nNodes, st))) return rc;
      if ((rc = dPairName.upload(j->pairName, (size_t)j->nPairs, st))) return rc;
      if ((rc = dPairTree.upload(j->pairTree, (size_t)j->nPairs, st))) return rc;
      if ((rc = dLeaf.reserve<int>((size_t)j->nPairs))) return rc;
      HIPCHECK(tLeaf.start(st));
      hipLaunchKernelGGL(k_tree_descend, dim3((unsigned)((j->nPairs + SY_THREADS - 1) / SY_THREADS)), dim3(SY_THREADS), 0, st,
                         dAns.as<const unsigned char>(), N, dTreeOff.as<const int>(), dQuest.as<const int>(), dNo.as<const int>(), dYes.as<const int>(),
                         dPairName.as<const int>(), dPairTree.as<const int>(), j->nPairs, dLeaf.as<int>());
      HIPCHECK(hipGetLastError());
      HIPCHECK(tLeaf.stop(st));
      if ((rc = dLeaf.download(leaf, (size_t)j->nPairs, st))) return rc;
   }
   HIPCHECK(hipStreamSynchronize(st));
   if (nQ > 0) HIPCHECK(tAns.ms(&g_kernelMs[0]));
   if (j->nPairs > 0) HIPCHECK(tLeaf.ms(&g_kernelMs[1]));
   return HTKAMD_OK;
}
