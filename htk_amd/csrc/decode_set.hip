// decode_set.hip -- a batch in which every utterance is decoded against a network of its own: HVite -a from word-level transcriptions
// and HVite -w with a lattice per file (both DoAlignment, HVite.c:830).  Host side; the token kernel is k_decode<0, DEC_SET_THREADS, true,
// false, true> of decode.hip, which takes the network's record from nets[DecUtt::net] instead of its arguments.
//
// Packing.  Every network's tables are built by htkamd_decoder_pack -- the code of htkamd_decoder_create -- without register-resident
// models (the kernel keeps every token in memory) and appended, 256-byte aligned, to ONE host buffer that becomes ONE device allocation;
// the records' pointers are offsets until that allocation exists.  hmmState (a property of the model set) is there once.  The tied
// states of the networks follow one another in the scorer's slot table: utterance u scores the ns[netOf[u]] rows from usedOff[netOf[u]]
// on, into a block of its own with T columns, and reads it back transposed with ns[netOf[u]] rows per frame (DecUtt::ns).
// Ties.  k_decode flags them as in the single decoder; the flagged utterances (all of them: HTKAMD_ORDER_EXACT) are grouped by network and
// k_decode_ord (decode_ord.hip, unchanged: a network per launch) is launched once per group.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>
#include "internal.h"
#include "hipcheck.h"
#include "kernels.h"
#include "decode.h"

struct htkamd_decoder_set {
   htkamd_model *m = nullptr;
   std::vector<DecNet> nets;           // absolute device pointers
   std::vector<int> ns, usedOff;       // per network: tied states it uses, its first entry in d_used
   int maxNs = 0;
   char *d_tables = nullptr;           // every network's tables
   DecNet *d_nets = nullptr;
   int *d_used = nullptr;
   DecArena ws;
   int orderMode = HTKAMD_ORDER_AUTO, lastTied = 0;
};

extern "C" void htkamd_decoder_set_destroy(htkamd_decoder_set *d)
{
   if (!d) return;
   if (d->d_tables) (void)hipFree(d->d_tables);
   if (d->d_nets) (void)hipFree(d->d_nets);
   if (d->d_used) (void)hipFree(d->d_used);
   d->ws.release();
   delete d;
}

extern "C" int htkamd_decoder_set_create(htkamd_model *m, const htkamd_net_desc *const *nets, int nNets, float lmScale, htkamd_decoder_set **out)
{
   if (!m || !nets || nNets < 1 || !out) { htkamd_set_error("decoder_set_create: bad argument"); return HTKAMD_EINVAL; }
   for (int i = 0; i < nNets; i++) if (!nets[i]) { htkamd_set_error("decoder_set_create: network %d is NULL", i); return HTKAMD_EINVAL; }
   htkamd_decoder_set *d = new htkamd_decoder_set();
   d->m = m;
   d->nets.resize(nNets); d->ns.resize(nNets); d->usedOff.resize(nNets);
   std::vector<char> host;
   std::vector<const void **> fix;            // pointer fields of d->nets holding offset + 1 into `host`
   const DecPut put = [&](const void *data, size_t bytes, const void **where) -> int {
      const size_t at = (host.size() + 255) & ~(size_t)255;
      host.resize(at + (bytes ? bytes : 1));
      if (bytes) memcpy(host.data() + at, data, bytes);
      *where = (const void *)(at + 1);
      fix.push_back(where);
      return HTKAMD_OK;
   };
   std::vector<int> used, us;
   for (int i = 0; i < nNets; i++) {
      const int rc = htkamd_decoder_pack(m, nets[i], lmScale, true, i == 0, put, d->nets[i], us, nullptr);
      if (rc) { htkamd_decoder_set_destroy(d); return rc; }
      d->usedOff[i] = (int)used.size(); d->ns[i] = (int)us.size();
      d->maxNs = std::max(d->maxNs, d->ns[i]);
      used.insert(used.end(), us.begin(), us.end());
   }
   hipError_t e;
   if ((e = hipMalloc((void **)&d->d_tables, host.size() ? host.size() : 1)) != hipSuccess || (e = hipMalloc((void **)&d->d_nets, sizeof(DecNet) * nNets)) != hipSuccess ||
       (e = hipMalloc((void **)&d->d_used, sizeof(int) * (used.size() ? used.size() : 1))) != hipSuccess) {
      htkamd_set_error("decoder_set_create: hipMalloc: %s", hipGetErrorString(e)); htkamd_decoder_set_destroy(d);
      return (e == hipErrorNoDevice || e == hipErrorInvalidDevice) ? HTKAMD_ENODEV : HTKAMD_ENOMEM;
   }
   for (const void **w : fix) *w = d->d_tables + ((size_t)*w - 1);
   for (int i = 1; i < nNets; i++) d->nets[i].hmmState = d->nets[0].hmmState;
   if ((e = hipMemcpy(d->d_tables, host.data(), host.size(), hipMemcpyHostToDevice)) != hipSuccess ||
       (e = hipMemcpy(d->d_nets, d->nets.data(), sizeof(DecNet) * nNets, hipMemcpyHostToDevice)) != hipSuccess ||
       (e = hipMemcpy(d->d_used, used.data(), sizeof(int) * used.size(), hipMemcpyHostToDevice)) != hipSuccess) {
      htkamd_set_error("decoder_set_create: %s", hipGetErrorString(e)); htkamd_decoder_set_destroy(d); return HTKAMD_EHIP;
   }
   *out = d;
   return HTKAMD_OK;
}

extern "C" int htkamd_decoder_set_set_order(htkamd_decoder_set *d, int mode)
{
   if (!d || mode < HTKAMD_ORDER_AUTO || mode > HTKAMD_ORDER_EXACT) { htkamd_set_error("decoder_set_set_order: bad argument"); return HTKAMD_EINVAL; }
   d->orderMode = mode;
   return HTKAMD_OK;
}
extern "C" int htkamd_decoder_set_last_tied(const htkamd_decoder_set *d) { return d ? d->lastTied : 0; }

extern "C" int htkamd_decoder_set_run(htkamd_decoder_set *d, const htkamd_decode_config *cfg, const float *dX, const int *frameOff, const int *netOf, int nUtt,
                                      int maxWords, const htkamd_decode_out *out, void *stream)
{
   if (!d || !cfg || !out || nUtt < 0 || maxWords < 1 || (nUtt > 0 && (!frameOff || !netOf)) || !out->nWords || !out->wordPron || !out->wordStart || !out->wordEnd ||
       !out->wordScore || !out->total) {
      htkamd_set_error("decoder_set_run: bad argument"); return HTKAMD_EINVAL;
   }
   const int nNets = (int)d->nets.size();
   for (int u = 0; u < nUtt; u++)
      if (netOf[u] < 0 || netOf[u] >= nNets) { htkamd_set_error("decoder_set_run: utterance %d names network %d of %d", u, netOf[u], nNets); return HTKAMD_EINVAL; }
   d->lastTied = 0;
   if (nUtt == 0) return HTKAMD_OK;
   hipStream_t s = (hipStream_t)stream;
   const int FR = SCORE_TILE_FRAMES, SL = (cfg->scoreMode & (HTKAMD_SCORE_BF16 | HTKAMD_SCORE_MFMA)) ? SCORE_TASK_SLOTS_WIDE : SCORE_TASK_SLOTS;
   int orderMode = d->orderMode;
   if (const char *ev = getenv("HTKAMD_DECODE_ORDER")) orderMode = !strcmp(ev, "fast") ? HTKAMD_ORDER_FAST : !strcmp(ev, "exact") ? HTKAMD_ORDER_EXACT : HTKAMD_ORDER_AUTO;
   DecArena &ws = d->ws;
   enum { WS_ORDER = 16 };      // first slot of the exact-order pass's buffers
   DecBatch bt;
   const auto uttNet = [&](int u) { const int g = netOf[u]; return DecUttNet{&d->nets[g], g, d->ns[g], d->usedOff[g]}; };
   int u0 = 0;
   while (u0 < nUtt) {
      // (the work space per utterance as htkamd_decoder_run counts it, with the utterance's own network: chunks stay under ~24 GB)
      htkamd_decoder_plan_nets(uttNet, frameOff, u0, nUtt, FR, SL,
                               [](size_t T, const DecUttNet &un) { return (size_t)un.ns * T * 8 + (size_t)un.N->nTok * 16 + (size_t)un.N->nNodes * 24 + (T + 1) * (size_t)un.N->nWordNodes * 16; },
                               (size_t)maxWords, 1, 0, bt);
      const int u1 = bt.u1, nu = u1 - u0;
      const size_t score = bt.score, tok = bt.tok, node = bt.node, path = bt.path;
      ws.begin(s, "decoder_set_run");
      void *dScore = ws.get(score * 4), *dScoreT = ws.get(score * 4), *dTok = ws.get(tok * sizeof(Tok)), *dEx = ws.get(node * sizeof(Tok)), *dImax = ws.get(node * 8);
      void *dPPrev = ws.get(path * 4), *dPLike = ws.get(path * 8), *dPLm = ws.get(path * 4);
      void *dUtt = ws.get(sizeof(DecUtt) * nu), *dTasks = ws.get(sizeof(ScoreTask) * bt.tasks.size() + sizeof(int));
      void *dOutI = ws.get(sizeof(int) * ((size_t)nu * maxWords * 3 + nu)), *dOutF = ws.get(sizeof(float) * ((size_t)nu * maxWords * 3 + nu)), *dTot = ws.get(sizeof(double) * nu);
      void *dOutD = ws.get(sizeof(double) * (size_t)nu * maxWords);
      void *dTie = ws.get(sizeof(int) * nu);
      int rc = ws.rc;
      if (!rc) rc = htkamd_decoder_score_slots(d->m, d->d_used, cfg->scoreMode, dX, frameOff[u1], bt, 0, d->maxNs, dUtt, dTasks, (float *)dScore, (float *)dScoreT, nullptr,
                                               "decoder_set_run", s);
      DecArgs a;
      memset(&a, 0, sizeof(a));
      if (!rc) {
         a.nets = d->d_nets; a.utt = (const DecUtt *)dUtt; a.nUtt = nu; a.score = (const float *)dScoreT;
         a.tok = (Tok *)dTok; a.ex = (Tok *)dEx; a.imax = (double *)dImax;
         a.pathPrev = (int *)dPPrev; a.pathLike = (double *)dPLike; a.pathLm = (float *)dPLm;
         a.genBeam = cfg->genBeam; a.wordBeam = cfg->wordBeam; a.lmScale = cfg->lmScale; a.wordPen = cfg->wordPen; a.prScale = cfg->prScale; a.maxActive = cfg->maxActive;
         a.maxWords = maxWords;
         int *oi = (int *)dOutI;
         a.nWords = oi; a.wordPron = oi + nu; a.wordStart = a.wordPron + (size_t)nu * maxWords; a.wordEnd = a.wordStart + (size_t)nu * maxWords;
         a.wordScore = (float *)dOutF; a.wordLm = (float *)dOutF + (size_t)nu * maxWords; a.wordAc = (float *)dOutF + (size_t)nu * maxWords * 2; a.finalLm = (float *)dOutF + (size_t)nu * maxWords * 3; a.total = (double *)dTot;
         a.wordLike = (double *)dOutD;
         a.tieFlag = (int *)dTie;
         (void)hipMemsetAsync(dTie, 0, sizeof(int) * nu, s);
         rc = htkamd_launch_decode_set(a, nu, s);
      }
      if (!rc && orderMode != HTKAMD_ORDER_FAST) {
         // as htkamd_decoder_run: the flagged utterances (or all) again in the order of HRec's instance list -- k_decode_ord takes ONE network from
         // its arguments, so the selected utterances are sorted by network and each network's run of them is a launch
         std::vector<int> flags(nu, 1);
         if (orderMode == HTKAMD_ORDER_AUTO) {
            hipError_t e;
            if ((e = hipMemcpyAsync(flags.data(), dTie, sizeof(int) * nu, hipMemcpyDeviceToHost, s)) != hipSuccess || (e = hipStreamSynchronize(s)) != hipSuccess) {
               htkamd_set_error("decoder_set_run: %s", hipGetErrorString(e)); rc = HTKAMD_EHIP;
            }
         }
         std::vector<int> pick;
         for (int k = 0; k < nu && !rc; k++) if (flags[k]) pick.push_back(k);
         std::stable_sort(pick.begin(), pick.end(), [&](int x, int y) { return bt.utt[x].net < bt.utt[y].net; });
         if (!rc && !pick.empty()) {
            const int nSel = (int)pick.size();
            const int pathExtra = 64;
            std::vector<DecUtt> sel(nSel);
            struct Group { int first, n, net, seqCap; size_t seq0; };
            std::vector<Group> groups;
            size_t opath = 0, seqTotal = 0;
            for (int i = 0; i < nSel; i++) {
               DecUtt ud = bt.utt[pick[i]];
               const DecNet &N = d->nets[ud.net];
               ud.path0 = opath;
               opath += 3 * ((size_t)(ud.T + 1) * N.nWordNodes) + pathExtra;      // (htkamd_decoder_run: room for every word node thrice per frame)
               sel[i] = ud;
               if (groups.empty() || groups.back().net != ud.net) { groups.push_back(Group{i, 0, ud.net, 8 * N.nNodes + 1024, seqTotal}); }
               groups.back().n++;
               seqTotal += 2 * (size_t)groups.back().seqCap;
            }
            ws.seek(WS_ORDER);
            void *dSel = ws.get(sizeof(DecUtt) * nSel), *dSeq = ws.get(sizeof(int) * seqTotal), *dPos = ws.get(sizeof(int) * node), *dOoo = ws.get(node);
            void *oPrev = ws.get(opath * 4), *oLike = ws.get(opath * 8), *oLm = ws.get(opath * 4), *oNode = ws.get(opath * 4), *oFrame = ws.get(opath * 4);
            rc = ws.rc;
            if (!rc) {
               hipError_t e = hipMemcpyAsync(dSel, sel.data(), sizeof(DecUtt) * nSel, hipMemcpyHostToDevice, s);
               if (e != hipSuccess) { htkamd_set_error("decoder_set_run: %s", hipGetErrorString(e)); rc = HTKAMD_EHIP; }
            }
            for (size_t g = 0; g < groups.size() && !rc; g++) {
               const Group &G = groups[g];
               OrdArgs oa;
               oa.d = a; oa.d.net = d->nets[G.net]; oa.d.ns = d->ns[G.net]; oa.d.nets = nullptr;
               oa.d.utt = (const DecUtt *)dSel + G.first; oa.d.nUtt = G.n;
               oa.d.pathPrev = (int *)oPrev; oa.d.pathLike = (double *)oLike; oa.d.pathLm = (float *)oLm;
               oa.list.seq = (int *)dSeq + G.seq0; oa.list.seqCap = G.seqCap; oa.list.pos = (int *)dPos; oa.list.ooo = (unsigned char *)dOoo;
               oa.list.pathNode = (int *)oNode; oa.list.pathFrame = (int *)oFrame; oa.list.pathExtra = pathExtra;
               oa.keepFast = orderMode == HTKAMD_ORDER_AUTO ? 1 : 0;
               rc = htkamd_launch_decode_ord(oa, G.n, s);
            }
            // (sel stays alive until the synchronisation below: its copy is asynchronous)
            if (!rc) d->lastTied += nSel;
            if (hipStreamSynchronize(s) != hipSuccess && !rc) { htkamd_set_error("decoder_set_run: the exact-order pass failed"); rc = HTKAMD_EHIP; }
         }
      }
      std::vector<int> hI; std::vector<float> hF; std::vector<double> hT, hD;
      if (!rc) {
         hI.resize((size_t)nu * maxWords * 3 + nu); hF.resize((size_t)nu * maxWords * 3 + nu); hT.resize(nu); hD.resize((size_t)nu * maxWords);
         hipError_t e;
         if ((e = hipMemcpyAsync(hI.data(), dOutI, sizeof(int) * hI.size(), hipMemcpyDeviceToHost, s)) != hipSuccess ||
             (e = hipMemcpyAsync(hF.data(), dOutF, sizeof(float) * hF.size(), hipMemcpyDeviceToHost, s)) != hipSuccess ||
             (e = hipMemcpyAsync(hT.data(), dTot, sizeof(double) * nu, hipMemcpyDeviceToHost, s)) != hipSuccess ||
             (e = hipMemcpyAsync(hD.data(), dOutD, sizeof(double) * hD.size(), hipMemcpyDeviceToHost, s)) != hipSuccess ||
             (e = hipStreamSynchronize(s)) != hipSuccess) { htkamd_set_error("decoder_set_run: %s", hipGetErrorString(e)); rc = HTKAMD_EHIP; }
      } else (void)hipStreamSynchronize(s);
      if (rc) return rc;
      for (int k = 0; k < nu; k++) {
         out->nWords[u0 + k] = hI[k]; out->total[u0 + k] = hT[k];
         if (out->finalLm) out->finalLm[u0 + k] = hF[(size_t)nu * maxWords * 3 + k];
         const size_t o = (size_t)(u0 + k) * maxWords, si = (size_t)k * maxWords;
         for (int w = 0; w < maxWords; w++) {
            out->wordPron[o + w] = hI[nu + si + w]; out->wordStart[o + w] = hI[nu + (size_t)nu * maxWords + si + w];
            out->wordEnd[o + w] = hI[nu + (size_t)nu * maxWords * 2 + si + w]; out->wordScore[o + w] = hF[si + w];
            if (out->wordLm) out->wordLm[o + w] = hF[(size_t)nu * maxWords + si + w];
            if (out->wordAc) out->wordAc[o + w] = hF[(size_t)nu * maxWords * 2 + si + w];
            if (out->wordLike) out->wordLike[o + w] = hD[si + w];
         }
      }
      u0 = u1;
   }
   return HTKAMD_OK;
}
