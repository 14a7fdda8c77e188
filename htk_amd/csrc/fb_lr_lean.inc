// fb_lr_lean.inc -- included by fb_lr.hip (round 5): the same left-to-right recursions and statistics with the instruction count of a
// wave-step as the first design constraint.  profiles/r04d_sq.json: k_alpha_lr issues 100 vector + 100 scalar instructions per
// wave-step, k_beta_lr 63 + 63, and their times follow instructions x wavefronts on the busiest SIMD x ~4.4 cycles (2 500 wavefronts on
// 1 024 SIMDs: nothing hides an in-order wavefront's issue slots) -- so the lever is what a step executes, of any kind:
//
//  * k_beta_np: HERest's default is NO pruning beam; the beta beams are then SetBeamTaper's alone (HFB.c:1116-1145, 1259-1264), known
//    on the host when the batch is prepared (FbArgs::qBeamNP).  The kernel carries no beam logic, no ballots, no retry loop: a step is
//    one add, one exchange of (score + beta), the log-add and a masked store.  (A pruning pass keeps k_beta_lr.)
//  * k_alpha_f: the fp32-transcendental class only.  MaxModelProb (HFB.c:655-683) is never formed as a maximum: "pr - max > minFrwdP"
//    holds iff it holds for every term, so every lane tests its own alpha + beta, the model's first lane the exit state of the model
//    before it, and ONE ballot of the kept lanes replaces the LDS column of sums and its three reads.  The beam decision needs the
//    first and the last kept lane only (a model's lanes are contiguous, so "my model is at or after the first kept model" is "my last
//    lane >= the first kept lane"): each wavefront reduces its own word BEFORE the barrier of the next step, 4 bytes per wavefront
//    cross it.  The entry-state term alpha_1 + beta_1 is dropped: alpha_2 >= alpha_1 + a_12 + b_2 and beta_1 = a_12 + b_2 + beta_2, so it
//    never exceeds the first state's own term but for the last bit (tolerance class).  Scores and beta columns come four frames per
//    register block, the step loop is unrolled by four (no LDS parking of scores, no per-step address arithmetic).
//  * k_stats_sp: with MINFORPROB's beam the alpha beam is one or two models wide (3-6 of 128 lanes), so the frame-parallel statistics
//    kernel spent its instructions on lanes that hold nothing.  Here a workgroup lists the (frame, lane) pairs inside the alpha beams
//    of its 32 frames and works on them densely -- a pair per lane, every operand gathered (the beta kernels leave a 32-byte record
//    per chain state: transitions, position, tied state).
//
// Reference semantics unchanged: SetBeta HFB.c:1149, StepAlpha :686, MaxModelProb :655, SetOcct :399, UpTranParms :1371, UpMixParms :1479.

// ------------------------------------------------------------------------------------ K2n: beta, no pruning beam, fp32-transcendental class
template <int W>
__global__ __launch_bounds__(64 * W) void k_beta_np(FbArgs a)
{
   constexpr int L = 64 * W, LP = L + 2 * SPAD;
   __shared__ double xz[2][LP];                        // b_j + beta_j of the column just computed, by step parity
   __shared__ double prSlot;
   const int gl = threadIdx.x;
   const int li = blockIdx.x;
   if (li >= a.nList) return;
   const int u = a.uttList[li];
   const UttDesc ud = a.utt[u];
   if (ud.status != HTKAMD_UTT_OK) {
      if (gl == 0) { a.status[u] = ud.status; a.pr[u] = LZERO; }
      return;
   }
   const int T = ud.T, Q = ud.Q, nS = ud.nSlots;
   const bool valid = gl < nS;
   LrRegs s;
   load_lr(s, a, ud, gl, valid);
   store_lane_rec(a, ud, gl, valid, s);
   for (int i = gl; i < LP; i += L) { xz[0][i] = LZERO; xz[1][i] = LZERO; }
   if (gl == 0) prSlot = LZERO;
   __syncthreads();
   const int q = s.q;                                  // 0 for the lanes past the chain: in no beam
   const double dSelf = (double)s.aSelf;
   // into the lane next door: the next state of the model, or (last lane) the exit state and the entry transition of the model after
   const double cN = s.last ? (double)s.aExit + (double)s.aEntryNext : (double)s.aNext;
   const double dEntry = (double)s.aEntry;             // (log-zero but at the models' first lanes)
   cint_lr *wB = (cint_lr *)(a.qBeamNP + ud.frame0 - 1);          // 1-based t
   const float *row = a.outp + ud.outp0 + (size_t)(valid ? gl : 0) * T;
   double *pB = a.betaW + ud.betaW0 + gl;

   // ---- t = T (HFB.c:1175-1198): only the last model can end the utterance
   int w = wB[T];
   int lo = w & 0xffff, hi = w >> 16;
   bool in = q >= lo && q <= hi;
   // Scores: a lane reads its OWN row of the state-major score block (64 cache lines per load instruction, an HBM miss every fourth
   // block), so a block of BK = 8 frames is requested a whole block ahead of its use; the beam words of a block likewise.
   constexpr int BK = 8;
   const int bT = (T - 1) / BK;
   float Rc[BK], Rn[BK];
   auto load8 = [&](float *R, const int b) {
      const f4s lo4 = *(const f4s *)(row + BK * b), hi4 = *(const f4s *)(row + BK * b + 4);
#pragma unroll
      for (int k = 0; k < 4; k++) { R[k] = lo4[k]; R[4 + k] = hi4[k]; }
   };
   auto pick = [](const float *R, int k) { float v = R[0];
#pragma unroll
      for (int i = 1; i < BK; i++) v = (k == i) ? R[i] : v;
      return v; };
   load8(Rc, bT);
   double bJ;
   {
      double mine = 0.0;
      for (int k = Q; k > q && k > lo; k--) mine += (double)(float)LZERO;
      bJ = in ? (double)s.aExit + mine : LZERO;
   }
   float oLast = pick(Rc, (T - 1) % BK);
   *(in ? pB + (size_t)(T - 1) * L : a.sink) = bJ;
   double z = in ? (double)oLast + bJ : LZERO;
   xz[T & 1][SPAD + gl] = z;

   // ---- t = T-1 .. 1 (HFB.c:1205-1277 without the pruning branch)
   auto step = [&](const int t, const float o_t, const int w_t) {
      xsync<W>();
      const double zN = xz[(t + 1) & 1][SPAD + gl + 1];
      const double bn = ladd_fast(cN + zN, dSelf + z);
      if (w_t != w) { w = w_t; lo = w & 0xffff; hi = w >> 16; in = q >= lo && q <= hi; }
      bJ = in ? bn : LZERO;
      *(in ? pB + (size_t)(t - 1) * L : a.sink) = bJ;      // (outside the beam: a sink line.  A store under a branch makes the compiler drain ALL
                                                           // vector memory operations before it touches a prefetched register -- s_waitcnt vmcnt(0) per block)
      oLast = o_t;
      z = in ? (double)o_t + bn : LZERO;            // (a score outside the beam may never have been computed: it must not reach the sum)
      xz[t & 1][SPAD + gl] = z;
   };
   for (int f = T - 2; f >= BK * bT; f--) step(f + 1, pick(Rc, f % BK), wB[f + 1]);
   if (bT >= 1) {
      load8(Rn, bT - 1);
      int wn[BK];
#pragma unroll
      for (int k = 0; k < BK; k++) wn[k] = wB[BK * (bT - 1) + 1 + k];
      for (int b = bT - 1; b >= 0; b--) {
         int wc[BK];
#pragma unroll
         for (int k = 0; k < BK; k++) { Rc[k] = Rn[k]; wc[k] = wn[k]; }
         if (b >= 1) {
            load8(Rn, b - 1);
#pragma unroll
            for (int k = 0; k < BK; k++) wn[k] = wB[BK * (b - 1) + 1 + k];
         }
#pragma unroll
         for (int k = BK - 1; k >= 0; k--) step(BK * b + k + 1, Rc[k], wc[k]);
      }
   }
   // utt->pr = beta_1 of the lowest model of column 1 (own values of its first lane)
   if (valid && s.first && q == lo) prSlot = (dEntry + (double)oLast) + bJ;
   __syncthreads();
   const double pr = prSlot;
   const int ok = pr > LSMALL;
   if (gl == 0) {
      a.pr[u] = ok ? pr : LZERO;
      a.status[u] = ok ? HTKAMD_UTT_OK : HTKAMD_UTT_SKIPPED;
   }
}

// ------------------------------------------------------------------------------------ K3f: alpha (the chain only), fp32-transcendental class
// what the beam decisions need of a beta beam word (lo | hi << 16): the first lanes of the models that bound it
struct BeamD {
   int lo, hi;
   int fLo, fHi, fHiEnd, fE;           // first lane of model lo, of model hi, of model hi + 1, of model min(hi + 1, Q) + 1
   unsigned long long inB, mLo, mE;    // this wavefront's lanes: in the beam; at or after fLo; before fE
};

template <int W, bool DBG>
__global__ __launch_bounds__(64 * W) void k_alpha_f(FbArgs a)
{
   constexpr int L = 64 * W, LP = L + 2 * SPAD;
   __shared__ double xal[2][LP];                       // alpha_j(t) by step parity (not yet cut to the alpha beam of t)
   __shared__ int cand[2][8];                          // the wavefronts' first / last kept lane (+1; 0 = none), by step parity
   __shared__ short flOf[L + 2];
   const int gl = threadIdx.x, lane = gl & 63, wv = __builtin_amdgcn_readfirstlane(gl >> 6);
   const int li = blockIdx.x;
   if (li >= a.nList) return;
   const int u = a.uttList[li];
   const UttDesc ud = a.utt[u];
   if (a.status[u] != HTKAMD_UTT_OK) {                   // skipped in the beta pass (or pre-check)
      if (gl == 0) atomicAdd(a.acc + a.lay.nUttSkipped, 1.0);
      return;
   }
   const int T = ud.T, Q = ud.Q, nS = ud.nSlots, nC = ud.nCells;
   const bool valid = gl < nS;
   LrRegs s;
   load_lr(s, a, ud, gl, valid);
   for (int i = gl; i < LP; i += L) { xal[0][i] = LZERO; xal[1][i] = LZERO; }
   if (valid && s.first) flOf[s.q] = (short)gl;
   if (gl == 0) { flOf[Q + 1] = (short)nS; flOf[0] = 0; }
   __syncthreads();
   const int q = s.q, N = s.N, j = s.j;
   const int cHmm = valid ? a.mHmm[s.mi] : 0, mc0 = valid ? a.mCell0[s.mi] : 0;
   // bounds of the own model, and of the model of the lane before (a first lane: the model before)
   const int myFirst = valid ? gl - (j - 2) : 0x7fff, myLast = valid ? gl - (j - 2) + (N - 3) : -1;
   int pFirst = myFirst, pLast = myLast;
   if (valid && s.first) { pLast = (q > 1) ? gl - 1 : -1; pFirst = (q > 1) ? flOf[q - 1] : 0x7fff; }
   const double dSelf = (double)s.aSelf;
   const double dIn = (double)(s.first ? s.aEntry : s.aPrev);       // into the state from the entry state / from the lane before
   const double dExitPrev = (valid && s.first && q > 1) ? (double)s.aExitPrev : 0.0;      // first lane: exit transition of the model before
   const double dEntry = (double)s.aEntry;             // (log-zero but at the models' first lanes)
   const bool isFirst = valid && s.first;
   cint_lr *qB = (cint_lr *)(a.qBeam + ud.frame0 - 1);           // final beta beams, 1-based t
   int *gaBeam = a.aBeam + ud.frame0 - 1;                        // alpha beams as LANES: first kept lane (raised to the beta beam) | last << 16;
                                                                  // a lane is inside iff its model's last lane >= the one and its first lane <= the other
   const float *row = a.outp + ud.outp0 + (size_t)(valid ? gl : 0) * T;
   const double *pBeta = a.betaW + ud.betaW0 + gl;               // + (t-1) L
   double *pS = a.alphaW + ud.alphaW0 + gl;                      // + (t-1) L
   const double pr = a.pr[u], minF = (double)a.minFrwdP;

   auto derive = [&](const int w_) {
      BeamD d;
      d.lo = w_ & 0xffff; d.hi = w_ >> 16;
      const int hh = d.hi > 0 ? d.hi : 1;
      d.fLo = __builtin_amdgcn_readfirstlane((int)flOf[d.lo]);
      d.fHi = __builtin_amdgcn_readfirstlane((int)flOf[hh]);
      d.fHiEnd = __builtin_amdgcn_readfirstlane((int)flOf[hh + 1]);
      d.fE = __builtin_amdgcn_readfirstlane((int)flOf[((hh < Q) ? hh + 1 : hh) + 1]);
      d.inB = __ballot(q >= d.lo && q <= d.hi);
      d.mLo = __ballot(gl >= d.fLo);
      d.mE = __ballot(gl < d.fE);
      return d;
   };
   int wCur = qB[1], wNxt = (T >= 2) ? qB[2] : wCur;
   BeamD cur = derive(wCur);                             // (of the word after it only the bounds are needed until it becomes the current one)
   auto exit_mask = [&]() { const int nlo = wNxt & 0xffff, nhi = wNxt >> 16; return __ballot(isFirst && q > 1 && q - 1 >= cur.lo && q - 1 <= cur.hi && q >= nlo && q <= nhi); };
   unsigned long long mX = exit_mask();

   double aJ = LZERO;                                    // alpha_j of the column before, inside its alpha beam
   double inc = LZERO;                                   // what comes in from the lane before: its alpha of the column before (+ the exit
                                                         // transition of the model before, at a first lane: alpha_1(q,t))
   double od, od1 = 0.0, bT, bT1 = LZERO;                // score and beta of columns t and t+1
   int candL = -1, candH = -1;                           // W == 1: first / last kept lane
   int candW = 0;                                        // W > 1: this wavefront's word for the next barrier
   int err = 0;
   int beamV = 0;                                        // lane (t & 63) holds the beam word of column t until 64 of them go out together
   int sl = 0, el = 0;

   // the kept lanes of column t (MaxModelProb of every model against pr - minFrwdP), reduced to this wavefront's candidates
   auto flags = [&]() {
      const double s1 = aJ + bT;                          // alpha_j(t) + beta_j(t)
      const double eT1 = (dEntry + od1) + bT1;            // entry-state beta of the own model in column t+1 (first lanes)
      const double s2 = inc + eT1;                        // exit state of the model before in column t
      const unsigned long long B = (cur.inB & __ballot(!(pr - s1 > minF))) | (mX & __ballot(!(pr - s2 > minF)));
      const unsigned long long bl = B & cur.mLo, bh = B & cur.mE;
      const int l_ = bl ? (int)__builtin_ctzll(bl) : -1, h_ = bh ? 63 - (int)__builtin_clzll(bh) : -1;
      if constexpr (W == 1) { candL = l_; candH = h_; }
      else candW = ((l_ < 0) ? 0 : 64 * wv + l_ + 1) | (((h_ < 0) ? 0 : 64 * wv + h_ + 1) << 16);
   };
   // the beta beam words move on by one column; w3 = the word of column t+2 (or the last one again)
   auto advance = [&](const int w3) {
      if (w3 == wNxt && wNxt == wCur) return;
      if (wNxt != wCur) { cur = derive(wNxt); wCur = wNxt; }
      wNxt = w3;
      mX = exit_mask();
   };
   auto put_beam = [&](const int t, const int word) {
      beamV = (lane == (t & 63)) ? word : beamV;
      if ((t & 63) == 63 || t == T) {
         const int tb = t & ~63;
         if (wv == 0 && tb + lane <= t && tb + lane >= 1) gaBeam[tb + lane] = beamV;
      }
   };
   auto debug_out = [&](const int t, const double aE_) {
      if constexpr (DBG) {
         if (a.alphaDbg && valid) {
            double *ad = a.alphaDbg + ud.beta0 + (size_t)(t - 1) * nC + mc0;
            ad[j - 1] = aJ;
            if (s.first) ad[0] = aE_;
            if (s.last) { const double aa = s.aExit; ad[N - 1] = (aa > LSMALL && (t == 1 || aJ > LSMALL)) ? ladd_fast(LZERO, aJ + aa) : LZERO; }
         }
      }
   };

   // ---- column 1: InitAlpha (HFB.c:616-651); without tee models only the first model starts
   {
      od = (double)row[0];
      bT = pBeta[0];
      if (T >= 2) { od1 = (double)row[1]; bT1 = pBeta[L]; }
      const int eq = cur.hi;
      double a1 = 0.0;
      for (int k = 2; k <= q && k <= eq; k++) a1 += (double)(float)LZERO;
      const bool in = valid && q <= eq;
      const double aE = in ? a1 : LZERO;
      const double xpre = aE + (double)s.aEntry;
      aJ = (in && (double)s.aEntry > LSMALL) ? xpre + od : LZERO;
      sl = 0; el = cur.fHi;
      xal[1][SPAD + gl] = aJ;
      xsync<W>();
      const double yPrev = xal[1][SPAD + gl - 1];
      *(in ? pS : a.sink) = xpre;
      put_beam(1, sl | (el << 16));
      debug_out(1, aE);
      inc = yPrev + dExitPrev;
      if (T >= 2) { flags(); advance((T >= 3) ? qB[3] : wNxt); }
   }

   // ---- columns 2 .. T (HFB.c:699-771).  oN / bN: score and beta of column t+1 (anything at t = T)
   auto step = [&](const int t, const float oN, const double bN, const int qw, auto inner_) -> bool {      // (qw: the beam word of column t + 2, see k_alpha_f2)
      constexpr bool INNER = decltype(inner_)::value;      // t + 2 <= T
      const int par = t & 1;
      od = od1; bT = bT1;
      od1 = (double)oN; bT1 = bN;
      // alpha_j(t) as if the state were in the beam: from the lane before (or the entry state), then from the state itself
      const double a1 = inc;
      const double x = ladd_fast(inc + dIn, aJ + dSelf);
      const double aJn = x + od;
      xal[par][SPAD + gl] = aJn;
      if constexpr (W > 1) { if (lane == 0) cand[par][wv] = candW; }
      xsync<W>();
      const double yp = xal[par][SPAD + gl - 1];
      // ---- the alpha beam (HFB.c:699-722) from the first and the last kept lane of column t-1
      int l_ = -1, h_ = -1;
      if constexpr (W == 1) { l_ = candL; h_ = candH; }
      else {
#pragma unroll
         for (int k = W - 1; k >= 0; k--) { const int c = cand[par][k] & 0xffff; l_ = c ? c - 1 : l_; }
#pragma unroll
         for (int k = 0; k < W; k++) { const int c = (cand[par][k] >> 16) & 0xffff; h_ = c ? c - 1 : h_; }
         l_ = __builtin_amdgcn_readfirstlane(l_); h_ = __builtin_amdgcn_readfirstlane(h_);
      }
      if (l_ < 0 || l_ >= cur.fHiEnd) { err = 1; return false; }            // no model kept from qLo[t-1] on, or sq > qHi[t]
      sl = (l_ < cur.fLo) ? cur.fLo : l_;                                   // start-point below the beta beam: pulled back
      if (h_ < 0 || h_ < sl) { err = 1; return false; }                     // eq < sq
      el = (h_ > cur.fHi) ? cur.fHi : h_;
      const bool in = myLast >= sl && myFirst <= el;
      const bool inP = pLast >= sl && pFirst <= el;
      aJ = in ? aJn : LZERO;
      const double yPrev = inP ? yp : LZERO;
      *(in ? pS + (size_t)(t - 1) * L : a.sink) = x;    // (outside the beam: the sink line, see k_beta_np)
      put_beam(t, sl | (el << 16));
      debug_out(t, in ? a1 : LZERO);
      inc = yPrev + dExitPrev;
      if (INNER || t < T) {
         flags();
         advance((INNER || t + 2 <= T) ? qw : wNxt);
      }
      return true;
   };
   {
      // column t takes the score and beta of column t+1 = frame index t: block c holds frame indices BK c .. BK c + BK - 1, requested a
      // whole block ahead (k_beta_np: a lane reads its own row of the score block); reads past the utterance's last column stay
      // inside the padded buffers and are never used
      constexpr int BK = 8;
      float Rc[BK], Rn[BK];
      double Bc[BK], Bn[BK];
      auto load8 = [&](float *R, double *B, const int c) {
         const f4s lo4 = *(const f4s *)(row + BK * c), hi4 = *(const f4s *)(row + BK * c + 4);
#pragma unroll
         for (int k = 0; k < 4; k++) { R[k] = lo4[k]; R[4 + k] = hi4[k]; }
#pragma unroll
         for (int k = 0; k < BK; k++) B[k] = pBeta[(size_t)(BK * c + k) * L];
      };
      auto pick = [](const float *R, int k) { float v = R[0];
#pragma unroll
         for (int i = 1; i < BK; i++) v = (k == i) ? R[i] : v;
         return v; };
      auto pickd = [](const double *B, int k) { double v = B[0];
#pragma unroll
         for (int i = 1; i < BK; i++) v = (k == i) ? B[i] : v;
         return v; };
      load8(Rc, Bc, 0);
      int t = 2;
      bool ok = true;
      for (; ok && t <= T && t < BK; t++) ok = step(t, pick(Rc, t), pickd(Bc, t), (t + 2 <= T) ? qB[t + 2] : 0, std::false_type{});
      if (ok && T >= BK) {
         int c = 1;
         load8(Rn, Bn, 1);
         for (; ok && BK * c + BK - 1 <= T - 2; c++) {
#pragma unroll
            for (int k = 0; k < BK; k++) { Rc[k] = Rn[k]; Bc[k] = Bn[k]; }
            load8(Rn, Bn, c + 1);
            int qw[BK];
#pragma unroll
            for (int k = 0; k < BK; k++) qw[k] = qB[BK * c + k + 2];
#pragma unroll
            for (int k = 0; k < BK; k++) ok = ok && step(BK * c + k, Rc[k], Bc[k], qw[k], std::true_type{});
         }
         // the rest, a column at a time: block c is in Rn / Bn, a block after it (if the utterance reaches it) is fetched when it starts
         t = BK * c;
#pragma unroll
         for (int k = 0; k < BK; k++) { Rc[k] = Rn[k]; Bc[k] = Bn[k]; }
         for (; ok && t <= T; t++) {
            if (t % BK == 0 && t != BK * c) load8(Rc, Bc, t / BK);
            ok = step(t, pick(Rc, t % BK), pickd(Bc, t % BK), (t + 2 <= T) ? qB[t + 2] : 0, std::false_type{});
         }
      }
   }

   if (err) {
      if (gl == 0) { a.status[u] = HTKAMD_UTT_EALPHA; atomicAdd(a.acc + a.lay.nUttSkipped, 1.0); }
      return;
   }
   if (valid && s.first) atomicAdd(a.acc + a.lay.nEgs + cHmm, 1.0);
   if (gl == 0) {
      atomicAdd(a.acc + a.lay.totalPr, pr);
      atomicAdd(a.acc + a.lay.totalT, (double)T);
      atomicAdd(a.acc + a.lay.nUttDone, 1.0);
      atomicAdd(a.acc + a.lay.nEval, (double)ud.nEval);
   }
}

// ------------------------------------------------------------------------------------ K3y: occupation / transition counts, mixture seeds -- the pairs inside the alpha beams only
#define STATS_EU 1
template <int W, bool FAST>
__global__ __launch_bounds__(64 * W, STATS_EU) void k_stats_sp(FbArgs a)
{
   constexpr int L = 64 * W, FC = STATS_FC;
   static_assert(FC <= 64, "the frames of a chunk are listed by one wavefront");
   __shared__ double etab[FAST ? 1 : EXP_TAB_N];
   __shared__ int plist[FC * L];                         // frame of the chunk << 16 | lane
   __shared__ int nPairs, nHits;
   if constexpr (!FAST) exp_table_to_lds(etab);
   const int gl = threadIdx.x, lane = gl & 63, wv = gl >> 6;
   const int li = blockIdx.x, ch = blockIdx.y;
   const size_t region = (size_t)((size_t)li * gridDim.y + ch) * W + wv;      // this wavefront's row of partial counts and region of the hit list
   double *part = a.trPart + region * TR_ROW;
   const int u = a.uttList[li];
   const UttDesc ud = a.utt[u];
   const int T = ud.T, Q = ud.Q, nS = ud.nSlots;
   const int t0 = ch * FC + 1;
   if (a.status[u] != HTKAMD_UTT_OK || t0 > T) {         // skipped, failed in the alpha pass, or shorter than this chunk's first frame
      if (lane == 0) { part[TR_ROW - 1] = -1.0; a.hitCtl[region] = 0; }
      return;
   }
   const int t1 = (t0 + FC - 1 < T) ? t0 + FC - 1 : T, nf = t1 - t0 + 1;
   const LaneRec *recs = a.laneRec + ud.slot0;
   if (gl == 0) nHits = 0;
   // ---- the pairs of the chunk: every lane of every model inside the alpha beam of its frame
   if (wv == 0) {
      int first = 0, cnt = 0;
      if (lane < nf) {
         const int wa = a.aBeam[ud.frame0 - 1 + t0 + lane];
         int sl = wa & 0xffff, el = (wa >> 16) & 0xffff;
         if (sl >= nS) sl = nS - 1;
         if (el >= nS) el = nS - 1;
         const LaneRec rs = recs[sl], re = recs[el];
         first = sl - (rs.j - 2);
         const int last = el - (re.j - 2) + (re.N - 3);
         cnt = last - first + 1;
         if (first < 0 || cnt < 0) cnt = 0;
         if (cnt > L) cnt = L;
      }
      int inc = cnt;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(inc, o); if (lane >= o) inc += v; }
      const int excl = inc - cnt;
      for (int k = 0; k < cnt; k++) plist[excl + k] = (lane << 16) | (first + k);
      if (lane == 63) nPairs = inc;
   }
   __syncthreads();
   const int P = nPairs;
   const double pr = a.pr[u], minF = (double)a.minFrwdP;
   const bool wantMix = (a.uFlags & (HTKAMD_UPMEANS | HTKAMD_UPVARS | HTKAMD_UPMIXES)) != 0;
   const bool wantTrans = (a.uFlags & HTKAMD_UPTRANS) != 0;
   const bool single = (a.maxM == 1);
   const int t0m = a.mTrans[ud.q0];
   // the workgroup's pairs go to ONE list: the regions of its wavefronts lie side by side, the first one's counter tells the lot (k_mixhits
   // keeps a state's parameters in registers along a run of its pairs: the longer the list, the longer the runs)
   MixHit *hreg = a.hits + (region - wv) * (size_t)(STATS_FC * 64);
   double bSelf[3] = {0.0, 0.0, 0.0}, bOut[3] = {0.0, 0.0, 0.0}, bOcc[3] = {0.0, 0.0, 0.0}, bEntry = 0.0, bOccE = 0.0;
   const double *aW = a.alphaW + ud.alphaW0, *bW = a.betaW + ud.betaW0;

   for (int p0 = 0; p0 < P; p0 += L) {
      const int p = p0 + gl;
      const bool have = p < P;
      const int e = have ? plist[p] : 0;
      const int ln = e & 0xffff, t = t0 + (e >> 16);
      const bool tLtT = t < T, nb = ln + 1 < nS;
      LaneRec r = recs[ln];
      const double xp = have ? aW[(size_t)(t - 1) * L + ln] : LZERO;
      const double bT = have ? bW[(size_t)(t - 1) * L + ln] : LZERO;
      const double bT1 = (have && tLtT) ? bW[(size_t)t * L + ln] : LZERO;
      const double bN1 = (have && tLtT && nb) ? bW[(size_t)t * L + ln + 1] : LZERO;
      const float *orow = a.outp + ud.outp0 + (size_t)ln * T;
      const double oT = have ? (double)orow[t - 1] : 0.0;
      const double oT1 = (have && tLtT) ? (double)orow[t] : 0.0;
      const double oN1 = (have && tLtT && nb) ? (double)orow[T + t] : 0.0;
      const int wb = (have && tLtT) ? a.qBeam[ud.frame0 - 1 + t + 1] : 1;
      // the lane before at the frame before: what the entry state of a model's first lane holds (alpha_1(q,t) = alpha_N(q-1,t-1), HFB.c:744)
      const int lp = ln - 1;
      const bool hasPrev = have && ln >= 1 && t >= 2;
      const LaneRec rp = recs[hasPrev ? lp : 0];
      const int waP = hasPrev ? a.aBeam[ud.frame0 - 1 + t - 1] : 0;
      const double xpP = hasPrev ? aW[(size_t)(t - 2) * L + lp] : LZERO;
      const double oP = hasPrev ? (double)(a.outp + ud.outp0 + (size_t)lp * T)[t - 2] : 0.0;
      const int q = r.q, j = r.j, N = r.N;
      const bool first = j == 2, last = j == N - 1;
      double aE = LZERO;
      if (first) {
         if (t == 1) aE = (q == 1) ? 0.0 : LZERO;
         else if (q > 1) {
            const int slP = waP & 0xffff, elP = (waP >> 16) & 0xffff;
            const bool inPrev = lp >= slP && lp - (rp.j - 2) <= elP;          // the model before was inside the alpha beam of t-1
            const double aP = (t == 2 && !((double)rp.aEntry > LSMALL)) ? LZERO : xpP + oP;
            aE = (inPrev ? aP : LZERO) + (double)rp.aOut;
         }
      }
      const int cT = have ? a.mTrans[ud.q0 + q - 1] : t0m;
      const bool hasNext = q < Q;
      const int lo2 = wb & 0xffff, hi2 = tLtT ? (wb >> 16) : 0;
      const bool bqt1ok = tLtT && q >= lo2 && q <= hi2;
      const double aJ = (t == 1 && !((double)r.aEntry > LSMALL)) ? LZERO : xp + oT;
      // Every count of a state at a frame is bounded by the state's occupation there (a transition count is a part of it), and that is
      // nothing (below e^-100) for all but the few states along the alignment
      const double xo = aJ + bT - pr;
      const bool occd = have && xo > EXPFLOOR;
      if (__any(occd)) {
         double vOcc = 0.0, vOccE = 0.0, vSelf = 0.0, vOut = 0.0, vEntry = 0.0;
         if (occd) {
            // SetOcct + UpTranParms for state j, and for the entry state at the model's first lane
            double x = xo;
            vOcc = (double)(float)exp_sel<FAST>(x, etab);
            if (first) {
               x = aE + entry_beta<FAST>(r.aEntry, oT, bT) - pr;
               vOccE = (double)((x > EXPFLOOR) ? (float)exp_sel<FAST>(x, etab) : 0.0f);
            }
            if (wantTrans) {
               if (first) { x = aE + (double)r.aEntry + oT + bT - pr; EXP_TERM(vEntry, x); }
               if (bqt1ok) {
                  x = aJ + (double)r.aSelf + (oT1 + bT1) - pr;
                  EXP_TERM(vSelf, x);
                  if (!last) { x = aJ + (double)r.aOut + (oN1 + bN1) - pr; EXP_TERM(vOut, x); }
               }
               if (last) {
                  // beta_N(q,t): 0 for the last model at T, else beta_1(q+1,t+1) where that is in the beam of t+1
                  const double bN = (t == T) ? ((q == Q) ? 0.0 : LZERO)
                                             : ((hasNext && q + 1 >= lo2 && q + 1 <= hi2) ? entry_beta<FAST>(r.aEntryNext, oN1, bN1) : LZERO);
                  x = aJ + (double)r.aOut + bN - pr;
                  EXP_TERM(vOut, x);
               }
            }
            if (cT != t0m && wantTrans) {                   // a chain of several transition matrices: this pair's counts go straight to its own
               double *tr = a.acc + a.lay.tr + a.transOff[cT];
               double *oc = a.acc + a.lay.trOcc + a.trOccOff[cT];
               if (vSelf != 0.0) atomicAdd(tr + (size_t)(j - 1) * N + (j - 1), vSelf);
               if (vOut != 0.0) atomicAdd(tr + (size_t)(j - 1) * N + j, vOut);
               if (vEntry != 0.0) atomicAdd(tr + 1, vEntry);
               if (vOcc != 0.0) atomicAdd(oc + (j - 1), vOcc);
               if (first && vOccE != 0.0) atomicAdd(oc, vOccE);
               vOcc = vOccE = vSelf = vOut = vEntry = 0.0;
            }
         }
#pragma unroll
         for (int i = 0; i < 3; i++) {
            const bool mine = j == i + 2;
            bSelf[i] += mine ? vSelf : 0.0; bOut[i] += mine ? vOut : 0.0; bOcc[i] += mine ? vOcc : 0.0;
         }
         bEntry += vEntry; bOccE += vOccE;
      }
      {
         // UpMixParms seed (HFB.c:1479-1489,1573-1606): the pairs the MINFORPROB prune lets through go to the list of k_mixhits
         double seed = LZERO;
         if (have && wantMix) {
            if (r.cM == 1 || single) {
               const double x = aJ + bT - pr;
               if (-x < minF) seed = x;
            } else {
               const double initx = xp + (bT - pr);
               const double ub = initx + oT;
               if (ub > -minF - 0.01) seed = initx;
            }
         }
         bool hit = seed > LSMALL;
         if (a.stCnt && hit) {                            // the pair's bucket (k_mixstate); the list below only takes what a full bucket turns away
            const int pos = atomicAdd(a.stCnt + r.sidx, 1);
            if (pos < a.stCap) {
               HitS o; o.frame = ud.frame0 + t - 1; o.pad = 0; o.seed = seed;
               a.stBucket[(size_t)r.sidx * a.stCap + pos] = o;
               hit = false;
            } else atomicAdd(a.stCnt + a.nTiedStates, 1);
         }
         const unsigned long long hm = __ballot(hit);
         if (hm) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&nHits, __popcll(hm));
            base = __builtin_amdgcn_readfirstlane(base);
            if (hit) {
               MixHit h; h.st = a.hitSlots ? ud.slot0 + ln : r.sidx; h.frame = ud.frame0 + t - 1; h.seed = seed;
               hreg[base + __popcll(hm & ((1ull << lane) - 1))] = h;
            }
         }
      }
   }
   __syncthreads();
   if (lane == 0) a.hitCtl[region] = (wv == 0) ? nHits : 0;

   // ---- this wavefront's counts for the chain's (first) transition matrix: a row of partial sums for k_trans_reduce -- [0..2] a_ii,
   // [3..5] a_i,i+1 (or a_iN from the last state), i = 2..4; [6] a_12; [7..9] occupation of states 2..4; [10] of the entry state; [15] the matrix
   {
      double rowv[11];
#pragma unroll
      for (int i = 0; i < 3; i++) { rowv[i] = bSelf[i]; rowv[3 + i] = bOut[i]; rowv[7 + i] = bOcc[i]; }
      rowv[6] = bEntry; rowv[10] = bOccE;
#pragma unroll
      for (int k = 0; k < 11; k++) {
         double v = rowv[k];
#pragma unroll
         for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
         rowv[k] = v;
      }
      if (lane == 0) {
#pragma unroll
         for (int k = 0; k < 11; k++) part[k] = wantTrans ? rowv[k] : 0.0;
         part[TR_ROW - 1] = wantTrans ? (double)t0m : -1.0;
      }
   }
}

// ------------------------------------------------------------------------------------ one wavefront, TWO chain states per lane (chains of 65 .. 128 states)
// The columns keep the layout of the two-wavefront class (L = 128 values per frame), but ONE wavefront works on the utterance: lane l
// holds states 2l and 2l+1.  No workgroup barrier and no LDS in a step: of the two neighbour values a lane needs one is its own other
// state, the other comes from the lane next door by a whole-wavefront DPP shift (v_mov_b32_dpp wave_shl / wave_shr), and the two
// log-adds of a lane are independent instruction streams that fill each other's latency.  1 250 wavefronts on 1 024 SIMDs: a wavefront
// runs (nearly) alone, so a step costs its dependent chain, not the issue slots of three wavefronts sharing a SIMD.
__device__ __forceinline__ double dpp_from_next(const double v, const double edge)      // lane l: v of lane l + 1 (lane 63: edge)
{
   const long long b = __double_as_longlong(v), e = __double_as_longlong(edge);
   const int lo = __builtin_amdgcn_update_dpp((int)e, (int)b, 0x130, 0xf, 0xf, false);
   const int hi = __builtin_amdgcn_update_dpp((int)(e >> 32), (int)(b >> 32), 0x130, 0xf, 0xf, false);
   return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double dpp_from_prev(const double v, const double edge)      // lane l: v of lane l - 1 (lane 0: edge)
{
   const long long b = __double_as_longlong(v), e = __double_as_longlong(edge);
   const int lo = __builtin_amdgcn_update_dpp((int)e, (int)b, 0x138, 0xf, 0xf, false);
   const int hi = __builtin_amdgcn_update_dpp((int)(e >> 32), (int)(b >> 32), 0x138, 0xf, 0xf, false);
   return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
typedef double d2s __attribute__((ext_vector_type(2), aligned(8)));

#define LEAN2_EU 1
__global__ __launch_bounds__(64, LEAN2_EU) void k_beta_np2(FbArgs a)
{
   constexpr int L = 128;
   const int lane = threadIdx.x, g0 = 2 * lane, g1 = g0 + 1;
   const int li = blockIdx.x;
   if (li >= a.nList) return;
   const int u = a.uttList[li];
   const UttDesc ud = a.utt[u];
   if (ud.status != HTKAMD_UTT_OK) {
      if (lane == 0) { a.status[u] = ud.status; a.pr[u] = LZERO; }
      return;
   }
   const int T = ud.T, Q = ud.Q, nS = ud.nSlots;
   const bool v0 = g0 < nS, v1 = g1 < nS;
   LrRegs s0, s1;
   load_lr(s0, a, ud, g0, v0); load_lr(s1, a, ud, g1, v1);
   store_lane_rec(a, ud, g0, v0, s0); store_lane_rec(a, ud, g1, v1, s1);
   const int q0 = s0.q, q1 = s1.q;                     // 0 for the states past the chain: in no beam
   const double dSelf0 = (double)s0.aSelf, dSelf1 = (double)s1.aSelf;
   const double cN0 = s0.last ? (double)s0.aExit + (double)s0.aEntryNext : (double)s0.aNext;
   const double cN1 = s1.last ? (double)s1.aExit + (double)s1.aEntryNext : (double)s1.aNext;
   cint_lr *wB = (cint_lr *)(a.qBeamNP + ud.frame0 - 1);          // 1-based t
   const float *row0 = a.outp + ud.outp0 + (size_t)(v0 ? g0 : 0) * T, *row1 = a.outp + ud.outp0 + (size_t)(v1 ? g1 : 0) * T;
   double *pB = a.betaW + ud.betaW0 + g0;

   // ---- t = T (HFB.c:1175-1198)
   int w = wB[T];
   int lo = w & 0xffff, hi = w >> 16;
   bool in0 = q0 >= lo && q0 <= hi, in1 = q1 >= lo && q1 <= hi;
   constexpr int BK = 8;                               // (frames per block of scores: see k_beta_np)
   const int bT = (T - 1) / BK;
   float Rc0[BK], Rc1[BK], Rn0[BK], Rn1[BK];
   auto load8 = [&](float *R, const float *row, const int b) {
      const f4s lo4 = *(const f4s *)(row + BK * b), hi4 = *(const f4s *)(row + BK * b + 4);
#pragma unroll
      for (int k = 0; k < 4; k++) { R[k] = lo4[k]; R[4 + k] = hi4[k]; }
   };
   auto pick = [](const float *R, int k) { float v = R[0];
#pragma unroll
      for (int i = 1; i < BK; i++) v = (k == i) ? R[i] : v;
      return v; };
   load8(Rc0, row0, bT); load8(Rc1, row1, bT);
   double b0, b1;
   {
      double m0 = 0.0, m1 = 0.0;
      for (int k = Q; k > q0 && k > lo; k--) m0 += (double)(float)LZERO;
      for (int k = Q; k > q1 && k > lo; k--) m1 += (double)(float)LZERO;
      b0 = in0 ? (double)s0.aExit + m0 : LZERO;
      b1 = in1 ? (double)s1.aExit + m1 : LZERO;
   }
   float o0 = pick(Rc0, (T - 1) % BK), o1 = pick(Rc1, (T - 1) % BK);
   { d2s st; st[0] = b0; st[1] = b1; *(d2s *)((in0 || in1) ? pB + (size_t)(T - 1) * L : a.sink) = st; }
   double z0 = in0 ? (double)o0 + b0 : LZERO, z1 = in1 ? (double)o1 + b1 : LZERO;

   auto step = [&](const int t, const float o0_t, const float o1_t, const int w_t) {
      const double zN = dpp_from_next(z0, LZERO);            // state 2l+2 of the column before
      const double n0 = ladd_fast(cN0 + z1, dSelf0 + z0);
      const double n1 = ladd_fast(cN1 + zN, dSelf1 + z1);
      if (w_t != w) { w = w_t; lo = w & 0xffff; hi = w >> 16; in0 = q0 >= lo && q0 <= hi; in1 = q1 >= lo && q1 <= hi; }
      b0 = in0 ? n0 : LZERO; b1 = in1 ? n1 : LZERO;
      d2s st; st[0] = b0; st[1] = b1;
      // (a lane with neither state in the beam "stores" to a sink line: the column costs the beam's cache lines and one more, not 1 KB --
      // and no branch, behind which the compiler would drain every outstanding load)
      // (streamed: 0.47 GB that the alpha pass reads once, from the other end -- without the hint the stores cost 8 us more)
      __builtin_nontemporal_store(st, (d2s *)((in0 || in1) ? pB + (size_t)(t - 1) * L : a.sink));
      o0 = o0_t; o1 = o1_t;
      z0 = in0 ? (double)o0_t + n0 : LZERO;
      z1 = in1 ? (double)o1_t + n1 : LZERO;
   };
   for (int f = T - 2; f >= BK * bT; f--) step(f + 1, pick(Rc0, f % BK), pick(Rc1, f % BK), wB[f + 1]);
   if (bT >= 1) {
      load8(Rn0, row0, bT - 1); load8(Rn1, row1, bT - 1);
      int wn[BK];
#pragma unroll
      for (int k = 0; k < BK; k++) wn[k] = wB[BK * (bT - 1) + 1 + k];
      for (int b = bT - 1; b >= 0; b--) {
         int wc[BK];
#pragma unroll
         for (int k = 0; k < BK; k++) { Rc0[k] = Rn0[k]; Rc1[k] = Rn1[k]; wc[k] = wn[k]; }
         if (b >= 1) {
            load8(Rn0, row0, b - 1); load8(Rn1, row1, b - 1);
#pragma unroll
            for (int k = 0; k < BK; k++) wn[k] = wB[BK * (b - 1) + 1 + k];
         }
#pragma unroll
         for (int k = BK - 1; k >= 0; k--) step(BK * b + k + 1, Rc0[k], Rc1[k], wc[k]);
      }
   }
   // utt->pr = beta_1 of the lowest model of column 1 (own values of its first state)
   double prv = LZERO;
   if (v0 && s0.first && q0 == lo) prv = ((double)s0.aEntry + (double)o0) + b0;
   if (v1 && s1.first && q1 == lo) prv = ((double)s1.aEntry + (double)o1) + b1;
#pragma unroll
   for (int o = 32; o > 0; o >>= 1) prv = fmax(prv, __shfl_xor(prv, o));
   const int ok = prv > LSMALL;
   if (lane == 0) {
      a.pr[u] = ok ? prv : LZERO;
      a.status[u] = ok ? HTKAMD_UTT_OK : HTKAMD_UTT_SKIPPED;
   }
}

template <bool DBG>
// (the beta columns are read once here, streamed: -2 % on the kernel)
#define ALPHA_LD(p_) __builtin_nontemporal_load((const d2s *)(p_))
// (NOT the score rows: a lane takes 32 bytes of its row per block, the line serves four blocks -- streamed, the kernel took 0.49 ms for 0.36)
#define ALPHA_LDF(p_) (*(const f4s *)(p_))
__global__ __launch_bounds__(64, LEAN2_EU) void k_alpha_f2(FbArgs a)
{
   constexpr int L = 128;
   __shared__ short flOf[L + 2];
   const int lane = threadIdx.x, g0 = 2 * lane, g1 = g0 + 1;
   const int li = blockIdx.x;
   if (li >= a.nList) return;
   const int u = a.uttList[li];
   const UttDesc ud = a.utt[u];
   if (a.status[u] != HTKAMD_UTT_OK) {                   // skipped in the beta pass (or pre-check)
      if (lane == 0) atomicAdd(a.acc + a.lay.nUttSkipped, 1.0);
      return;
   }
   const int T = ud.T, Q = ud.Q, nS = ud.nSlots, nC = ud.nCells;
   const bool v0 = g0 < nS, v1 = g1 < nS;
   LrRegs s0, s1;
   load_lr(s0, a, ud, g0, v0); load_lr(s1, a, ud, g1, v1);
   if (v0 && s0.first) flOf[s0.q] = (short)g0;
   if (v1 && s1.first) flOf[s1.q] = (short)g1;
   if (lane == 0) { flOf[Q + 1] = (short)nS; flOf[0] = 0; }
   __syncthreads();
   const int q0 = s0.q, q1 = s1.q;
   const int cHmm0 = v0 ? a.mHmm[s0.mi] : 0, cHmm1 = v1 ? a.mHmm[s1.mi] : 0;
   const int mF0 = v0 ? g0 - (s0.j - 2) : 0x7fff, mL0 = v0 ? g0 - (s0.j - 2) + (s0.N - 3) : -1;      // bounds of the state's model
   const int mF1 = v1 ? g1 - (s1.j - 2) : 0x7fff, mL1 = v1 ? g1 - (s1.j - 2) + (s1.N - 3) : -1;
   const double dSelf0 = (double)s0.aSelf, dSelf1 = (double)s1.aSelf;
   const double dIn0 = (double)(s0.first ? s0.aEntry : s0.aPrev), dIn1 = (double)(s1.first ? s1.aEntry : s1.aPrev);
   const bool f0 = v0 && s0.first, f1 = v1 && s1.first;
   const double dXp0 = (f0 && q0 > 1) ? (double)s0.aExitPrev : 0.0, dXp1 = (f1 && q1 > 1) ? (double)s1.aExitPrev : 0.0;
   const double dEntry0 = (double)s0.aEntry, dEntry1 = (double)s1.aEntry;     // (log-zero but at the models' first states)
   cint_lr *qB = (cint_lr *)(a.qBeam + ud.frame0 - 1);
   int *gaBeam = a.aBeam + ud.frame0 - 1;
   const float *row0 = a.outp + ud.outp0 + (size_t)(v0 ? g0 : 0) * T, *row1 = a.outp + ud.outp0 + (size_t)(v1 ? g1 : 0) * T;
   const double *pBeta = a.betaW + ud.betaW0 + g0;
   double *pS = a.alphaW + ud.alphaW0 + g0;
   const double pr = a.pr[u], minF = (double)a.minFrwdP;

   struct BeamD2 { int lo, hi, fLo, fHi, fHiEnd, fE; unsigned long long inB0, inB1, mLo0, mLo1, mE0, mE1; };
   auto derive = [&](const int w_) {
      BeamD2 d;
      d.lo = w_ & 0xffff; d.hi = w_ >> 16;
      const int hh = d.hi > 0 ? d.hi : 1;
      d.fLo = __builtin_amdgcn_readfirstlane((int)flOf[d.lo]);
      d.fHi = __builtin_amdgcn_readfirstlane((int)flOf[hh]);
      d.fHiEnd = __builtin_amdgcn_readfirstlane((int)flOf[hh + 1]);
      d.fE = __builtin_amdgcn_readfirstlane((int)flOf[((hh < Q) ? hh + 1 : hh) + 1]);
      d.inB0 = __ballot(q0 >= d.lo && q0 <= d.hi); d.inB1 = __ballot(q1 >= d.lo && q1 <= d.hi);
      d.mLo0 = __ballot(g0 >= d.fLo); d.mLo1 = __ballot(g1 >= d.fLo);
      d.mE0 = __ballot(g0 < d.fE); d.mE1 = __ballot(g1 < d.fE);
      return d;
   };
   int wCur = qB[1], wNxt = (T >= 2) ? qB[2] : wCur;
   BeamD2 cur = derive(wCur);
   unsigned long long mX0 = 0, mX1 = 0;
   auto exit_masks = [&]() {
      const int nlo = wNxt & 0xffff, nhi = wNxt >> 16;
      mX0 = __ballot(f0 && q0 > 1 && q0 - 1 >= cur.lo && q0 - 1 <= cur.hi && q0 >= nlo && q0 <= nhi);
      mX1 = __ballot(f1 && q1 > 1 && q1 - 1 >= cur.lo && q1 - 1 <= cur.hi && q1 >= nlo && q1 <= nhi);
   };
   exit_masks();

   double aJ0 = LZERO, aJ1 = LZERO, inc0 = LZERO, inc1 = LZERO;
   double od0, od1, on0 = 0.0, on1 = 0.0, bT0, bT1, bN0 = LZERO, bN1 = LZERO;      // score / beta of column t (od, bT) and t+1 (on, bN), both states
   int candL = -1, candH = -1, err = 0, beamV = 0, sl = 0, el = 0;

   // the kept states of column t -> the first and the last of them (as state numbers)
   auto flags = [&]() {
      const unsigned long long k0 = (cur.inB0 & __ballot(!(pr - (aJ0 + bT0) > minF))) | (mX0 & __ballot(!(pr - (inc0 + ((dEntry0 + on0) + bN0)) > minF)));
      const unsigned long long k1 = (cur.inB1 & __ballot(!(pr - (aJ1 + bT1) > minF))) | (mX1 & __ballot(!(pr - (inc1 + ((dEntry1 + on1) + bN1)) > minF)));
      const unsigned long long l0 = k0 & cur.mLo0, l1 = k1 & cur.mLo1, h0 = k0 & cur.mE0, h1 = k1 & cur.mE1;
      // state 2l before state 2l+1: the lowest lane of either word, its even state if that is set
      const unsigned long long la = l0 | l1, ha = h0 | h1;
      if (la) { const int ll = (int)__builtin_ctzll(la); candL = 2 * ll + (((l0 >> ll) & 1ull) ? 0 : 1); } else candL = -1;
      if (ha) { const int hl = 63 - (int)__builtin_clzll(ha); candH = 2 * hl + (((h1 >> hl) & 1ull) ? 1 : 0); } else candH = -1;
   };
   auto advance = [&](const int w3) {
      if (w3 == wNxt && wNxt == wCur) return;
      if (wNxt != wCur) { cur = derive(wNxt); wCur = wNxt; }
      wNxt = w3;
      exit_masks();
   };
   auto put_beam = [&](const int t, const int word) {
      beamV = (lane == (t & 63)) ? word : beamV;
      if ((t & 63) == 63 || t == T) {
         const int tb = t & ~63;
         if (tb + lane <= t && tb + lane >= 1) gaBeam[tb + lane] = beamV;
      }
   };
   auto debug_out = [&](const int t, const double aE0, const double aE1) {
      if constexpr (DBG) {
         if (a.alphaDbg) {
            if (v0) {
               double *ad = a.alphaDbg + ud.beta0 + (size_t)(t - 1) * nC + a.mCell0[s0.mi];
               ad[s0.j - 1] = aJ0;
               if (s0.first) ad[0] = aE0;
               if (s0.last) { const double aa = s0.aExit; ad[s0.N - 1] = (aa > LSMALL && (t == 1 || aJ0 > LSMALL)) ? ladd_fast(LZERO, aJ0 + aa) : LZERO; }
            }
            if (v1) {
               double *ad = a.alphaDbg + ud.beta0 + (size_t)(t - 1) * nC + a.mCell0[s1.mi];
               ad[s1.j - 1] = aJ1;
               if (s1.first) ad[0] = aE1;
               if (s1.last) { const double aa = s1.aExit; ad[s1.N - 1] = (aa > LSMALL && (t == 1 || aJ1 > LSMALL)) ? ladd_fast(LZERO, aJ1 + aa) : LZERO; }
            }
         }
      }
   };
   // what comes into the two states from the states before them, from the column just finished (inside its alpha beam)
   auto incoming = [&]() {
      const double yp = dpp_from_prev(aJ1, LZERO);           // state 2l-1
      inc0 = yp + dXp0;
      inc1 = aJ0 + dXp1;
   };

   // ---- column 1: InitAlpha (HFB.c:616-651)
   {
      od0 = (double)row0[0]; od1 = (double)row1[0];
      { const d2s bv = *(const d2s *)pBeta; bT0 = bv[0]; bT1 = bv[1]; }
      if (T >= 2) { on0 = (double)row0[1]; on1 = (double)row1[1]; const d2s bv = *(const d2s *)(pBeta + L); bN0 = bv[0]; bN1 = bv[1]; }
      const int eq = cur.hi;
      double a10 = 0.0, a11 = 0.0;
      for (int k = 2; k <= q0 && k <= eq; k++) a10 += (double)(float)LZERO;
      for (int k = 2; k <= q1 && k <= eq; k++) a11 += (double)(float)LZERO;
      const bool i0 = v0 && q0 <= eq, i1 = v1 && q1 <= eq;
      const double aE0 = i0 ? a10 : LZERO, aE1 = i1 ? a11 : LZERO;
      const double xp0 = aE0 + (double)s0.aEntry, xp1 = aE1 + (double)s1.aEntry;
      aJ0 = (i0 && (double)s0.aEntry > LSMALL) ? xp0 + od0 : LZERO;
      aJ1 = (i1 && (double)s1.aEntry > LSMALL) ? xp1 + od1 : LZERO;
      sl = 0; el = cur.fHi;
      { d2s st; st[0] = xp0; st[1] = xp1; *(d2s *)((i0 || i1) ? pS : a.sink) = st; }
      put_beam(1, sl | (el << 16));
      debug_out(1, aE0, aE1);
      incoming();
      if (T >= 2) { flags(); advance((T >= 3) ? qB[3] : wNxt); }
   }

   // (qw: the beam word of column t + 2, requested by the caller a block ahead -- read here, behind the scalar work on the flags, its load
   //  was waited for in every step: s_load, s_waitcnt lgkmcnt(0), 200 cycles of a 1 500-cycle step)
   auto step = [&](const int t, const float oN0, const float oN1, const double bNn0, const double bNn1, const int qw, auto inner_) -> bool {
      constexpr bool INNER = decltype(inner_)::value;      // t + 2 <= T
      od0 = on0; od1 = on1; bT0 = bN0; bT1 = bN1;
      on0 = (double)oN0; on1 = (double)oN1; bN0 = bNn0; bN1 = bNn1;
      const double a10 = inc0, a11 = inc1;
      const double x0 = ladd_fast(inc0 + dIn0, aJ0 + dSelf0);
      const double x1 = ladd_fast(inc1 + dIn1, aJ1 + dSelf1);
      // ---- the alpha beam (HFB.c:699-722) from the first and the last kept state of column t-1
      const int l_ = candL, h_ = candH;
      if (l_ < 0 || l_ >= cur.fHiEnd) { err = 1; return false; }
      sl = (l_ < cur.fLo) ? cur.fLo : l_;
      if (h_ < 0 || h_ < sl) { err = 1; return false; }
      el = (h_ > cur.fHi) ? cur.fHi : h_;
      const bool i0 = mL0 >= sl && mF0 <= el, i1 = mL1 >= sl && mF1 <= el;
      aJ0 = i0 ? x0 + od0 : LZERO;
      aJ1 = i1 ? x1 + od1 : LZERO;
      d2s st; st[0] = x0; st[1] = x1;
      *(d2s *)((i0 || i1) ? pS + (size_t)(t - 1) * L : a.sink) = st;      // (outside the alpha beam: the sink line, see k_beta_np2)
      put_beam(t, sl | (el << 16));
      debug_out(t, i0 ? a10 : LZERO, i1 ? a11 : LZERO);
      incoming();
      if (INNER || t < T) {
         flags();
         advance((INNER || t + 2 <= T) ? qw : wNxt);
      }
      return true;
   };
   {
      constexpr int BK = 8;                               // (blocks of frames: see k_alpha_f)
      float Rc0[BK], Rc1[BK], Rn0[BK], Rn1[BK];
      d2s Bc[BK], Bn[BK];
      auto load8 = [&](float *R0, float *R1, d2s *B, const int c) {
         const f4s a4 = ALPHA_LDF(row0 + BK * c), b4 = ALPHA_LDF(row0 + BK * c + 4), c4 = ALPHA_LDF(row1 + BK * c), d4 = ALPHA_LDF(row1 + BK * c + 4);
#pragma unroll
         for (int k = 0; k < 4; k++) { R0[k] = a4[k]; R0[4 + k] = b4[k]; R1[k] = c4[k]; R1[4 + k] = d4[k]; }
#pragma unroll
         for (int k = 0; k < BK; k++) B[k] = ALPHA_LD(pBeta + (size_t)(BK * c + k) * L);
      };
      auto pick = [](const float *R, int k) { float v = R[0];
#pragma unroll
         for (int i = 1; i < BK; i++) v = (k == i) ? R[i] : v;
         return v; };
      auto pickd = [](const d2s *B, int k) { d2s v = B[0];
#pragma unroll
         for (int i = 1; i < BK; i++) v = (k == i) ? B[i] : v;
         return v; };
      load8(Rc0, Rc1, Bc, 0);
      int t = 2;
      bool ok = true;
      for (; ok && t <= T && t < BK; t++) { const d2s bb = pickd(Bc, t); ok = step(t, pick(Rc0, t), pick(Rc1, t), bb[0], bb[1], (t + 2 <= T) ? qB[t + 2] : 0, std::false_type{}); }
      if (ok && T >= BK) {
         int c = 1;
         load8(Rn0, Rn1, Bn, 1);
         for (; ok && BK * c + BK - 1 <= T - 2; c++) {
#pragma unroll
            for (int k = 0; k < BK; k++) { Rc0[k] = Rn0[k]; Rc1[k] = Rn1[k]; Bc[k] = Bn[k]; }
            load8(Rn0, Rn1, Bn, c + 1);
            int qw[BK];                                      // columns BK c + 2 .. BK c + 9 <= T here
#pragma unroll
            for (int k = 0; k < BK; k++) qw[k] = qB[BK * c + k + 2];
#pragma unroll
            for (int k = 0; k < BK; k++) ok = ok && step(BK * c + k, Rc0[k], Rc1[k], Bc[k][0], Bc[k][1], qw[k], std::true_type{});
         }
         t = BK * c;
#pragma unroll
         for (int k = 0; k < BK; k++) { Rc0[k] = Rn0[k]; Rc1[k] = Rn1[k]; Bc[k] = Bn[k]; }
         for (; ok && t <= T; t++) {
            if (t % BK == 0 && t != BK * c) load8(Rc0, Rc1, Bc, t / BK);
            const d2s bb = pickd(Bc, t % BK);
            ok = step(t, pick(Rc0, t % BK), pick(Rc1, t % BK), bb[0], bb[1], (t + 2 <= T) ? qB[t + 2] : 0, std::false_type{});
         }
      }
   }

   if (err) {
      if (lane == 0) { a.status[u] = HTKAMD_UTT_EALPHA; atomicAdd(a.acc + a.lay.nUttSkipped, 1.0); }
      return;
   }
   if (f0) atomicAdd(a.acc + a.lay.nEgs + cHmm0, 1.0);
   if (f1) atomicAdd(a.acc + a.lay.nEgs + cHmm1, 1.0);
   if (lane == 0) {
      atomicAdd(a.acc + a.lay.totalPr, pr);
      atomicAdd(a.acc + a.lay.totalT, (double)T);
      atomicAdd(a.acc + a.lay.nUttDone, 1.0);
      atomicAdd(a.acc + a.lay.nEval, (double)ud.nEval);
   }
}
