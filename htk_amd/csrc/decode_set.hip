// decode_set.hip -- a batch in which every utterance is decoded against a network of its own: HVite -a from word-level transcriptions
// and HVite -w with a lattice per file (both DoAlignment, HVite.c:830).  Host side; the token kernel is k_decode<0, DEC_SET_THREADS, true,
// false, true> of decode.hip, which takes the network's record from nets[DecUtt::net] instead of its arguments.
//
// Packing.  Every network's tables are built by htkamd_decoder_pack -- the code of htkamd_decoder_create -- without register-resident
// models (the kernel keeps every token in memory) and appended, 256-byte aligned, to ONE host buffer that becomes ONE device allocation;
// the records' pointers are offsets until that allocation exists.  hmmState (a property of the model set) is there once.  The tied
// states of the networks follow one another in the scorer's slot table: utterance u scores the ns[netOf[u]] rows from usedOff[netOf[u]]
// on, into a block of its own with T columns, and reads it back transposed with ns[netOf[u]] rows per frame (DecUtt::ns).
// Running.  htkamd_decoder_set_run checks its arguments and hands the single decoder's driver (htkamd_decoder_run_1best, decode.hip) the
// set's networks, slot table and launch: chunks, work space, the exact-order pass for ties (k_decode_ord takes a network per launch, so the
// driver groups the chosen utterances by network) and the outputs are that one code for both.
// N-best.  htkamd_decoder_set_run_lattice[_align] do the same with the N-best driver (htkamd_decoder_run_nbest, decode_n.hip) and the SET
// forms of the token-set kernels: one launch per chunk whatever the number of networks in it.
#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>
#include <algorithm>
#include "internal.h"
#include "hipcheck.h"
#include "devbuf.h"
#include "kernels.h"
#include "decode.h"

DEVBUF_OWNER("decoder_set_create")

struct htkamd_decoder_set {
   htkamd_model *m = nullptr;
   std::vector<DecNet> nets;           // absolute device pointers
   std::vector<int> ns, usedOff;       // per network: tied states it uses, its first entry in d_used
   int maxNs = 0;
   DevBuf d_tables, d_nets, d_used;    // every network's tables (char), the records (DecNet), the slot table (int)
   std::vector<std::vector<int>> hostModel;     // per network: [nNodes] htkamd_net_desc.model (WORD nodes: the pronunciation)
   DecArena ws, wsN;                   // workspaces of htkamd_decoder_set_run and of htkamd_decoder_set_run_lattice, as htkamd_decoder's
   int orderMode = HTKAMD_ORDER_AUTO, lastTied = 0;
};

extern "C" void htkamd_decoder_set_destroy(htkamd_decoder_set *d)
{
   if (!d) return;
   d->ws.release();
   d->wsN.release();
   delete d;
}

extern "C" int htkamd_decoder_set_create(htkamd_model *m, const htkamd_net_desc *const *nets, int nNets, float lmScale, htkamd_decoder_set **out)
{
   if (!m || !nets || nNets < 1 || !out) { htkamd_set_error("decoder_set_create: bad argument"); return HTKAMD_EINVAL; }
   for (int i = 0; i < nNets; i++) if (!nets[i]) { htkamd_set_error("decoder_set_create: network %d is NULL", i); return HTKAMD_EINVAL; }
   htkamd_decoder_set *d = new htkamd_decoder_set();
   d->m = m;
   d->nets.resize(nNets); d->ns.resize(nNets); d->usedOff.resize(nNets); d->hostModel.resize(nNets);
   for (int i = 0; i < nNets; i++) d->hostModel[i].assign(nets[i]->model, nets[i]->model + nets[i]->nNodes);
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
   int rc;
   if ((rc = d->d_tables.reserve<char>(host.size())) || (rc = d->d_nets.reserve<DecNet>((size_t)nNets)) || (rc = d->d_used.reserve<int>(used.size()))) {
      htkamd_decoder_set_destroy(d); return rc;
   }
   for (const void **w : fix) *w = d->d_tables.as<char>() + ((size_t)*w - 1);
   for (int i = 1; i < nNets; i++) d->nets[i].hmmState = d->nets[0].hmmState;
   HIPCHECK_RC(rc, devOwner, hipMemcpy(d->d_tables.p, host.data(), host.size(), hipMemcpyHostToDevice));
   HIPCHECK_RC(rc, devOwner, hipMemcpy(d->d_nets.p, d->nets.data(), sizeof(DecNet) * nNets, hipMemcpyHostToDevice));
   HIPCHECK_RC(rc, devOwner, hipMemcpy(d->d_used.p, used.data(), sizeof(int) * used.size(), hipMemcpyHostToDevice));
   if (rc) { htkamd_decoder_set_destroy(d); return rc; }
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
   const auto uttNet = [&](int u) { const int g = netOf[u]; return DecUttNet{&d->nets[g], g, d->ns[g], d->usedOff[g]}; };
   const DecRun r = {"decoder_set_run", &d->ws, d->m, d->d_used.as<int>(), d->maxNs, uttNet, d->nets.data(), d->ns.data(), d->d_nets.as<DecNet>(), htkamd_launch_decode_set,
                     htkamd_decoder_order(d->orderMode), &d->lastTied, nullptr, nullptr, nullptr, nullptr};
   return htkamd_decoder_run_1best(r, cfg, dX, frameOff, nUtt, maxWords, out, (hipStream_t)stream);
}

// HVite -n i [N] [-z ext] with a network per utterance: the token sets and the lattice of utterance u over nets[netOf[u]]
extern "C" int htkamd_decoder_set_run_lattice(htkamd_decoder_set *d, const htkamd_decode_config *cfg, int nToks, float nBeam, const float *dX, const int *frameOff,
                                              const int *netOf, int nUtt, int maxLatNodes, int maxLatArcs, const htkamd_lattice_out *out, void *stream)
{
   return htkamd_decoder_set_run_lattice_align(d, cfg, nToks, nBeam, 0, dX, frameOff, netOf, nUtt, maxLatNodes, maxLatArcs, 0, out, nullptr, stream);
}

extern "C" int htkamd_decoder_set_run_lattice_align(htkamd_decoder_set *d, const htkamd_decode_config *cfg, int nToks, float nBeam, int alignMode, const float *dX,
                                                    const int *frameOff, const int *netOf, int nUtt, int maxLatNodes, int maxLatArcs, int maxAlign,
                                                    const htkamd_lattice_out *out, const htkamd_lattice_align_out *alOut, void *stream)
{
   // (what needs no set is checked first: a set cannot be made without a device)
   if (nToks < 2 || nToks > DEC_MAX_TOKS) { htkamd_set_error("decoder_set_run_lattice: nToks = %d (2..%d tokens per state)", nToks, DEC_MAX_TOKS); return HTKAMD_EINVAL; }
   if (!d || nUtt < 0 || (nUtt > 0 && (!frameOff || !netOf))) { htkamd_set_error("decoder_set_run_lattice: bad argument"); return HTKAMD_EINVAL; }
   const int nNets = (int)d->nets.size();
   for (int u = 0; u < nUtt; u++)
      if (netOf[u] < 0 || netOf[u] >= nNets) { htkamd_set_error("decoder_set_run_lattice: utterance %d names network %d of %d", u, netOf[u], nNets); return HTKAMD_EINVAL; }
   const auto uttNet = [&](int u) { const int g = netOf[u]; return DecUttNet{&d->nets[g], g, d->ns[g], d->usedOff[g]}; };
   const DecNRun r = {"decoder_set_run_lattice", &d->wsN, d->m, d->d_used.as<int>(), d->maxNs, uttNet, d->nets.data(), d->ns.data(), d->d_nets.as<DecNet>(), d->hostModel.data(),
                      htkamd_launch_decode_n_set, htkamd_decoder_order(d->orderMode), &d->lastTied};
   return htkamd_decoder_run_nbest(r, cfg, nToks, nBeam, dX, frameOff, nUtt, maxLatNodes, maxLatArcs, out, alignMode, maxAlign, alOut, (hipStream_t)stream);
}
