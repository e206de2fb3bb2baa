// Batched beam search of Model:generateAnswers (reference model.lua:466-573) on the device: the candidate bookkeeping the
// per-dialog host loops keep in SplitEval.generateAnswers (split_eval.py) and Model:generateAnswers (lua/model.lua), and
// oracle/visdial_oracle.py:generate_beam restates in fp64, for every QA round of a batch at once.  One *group* = one round,
// with k = beamSize slots; hypothesis row r = group * k + slot.
//
// The rules all three agree on, reproduced here exactly:
//  1. slot state starts from the round's encoder state (Gen_begin, rt_decoders.h; model.lua:478-503); beams[0] = <START>,
//     scores = 0 in fp64.
//  2. step s = 1 .. beamLen-1:
//     - explore slot 0 only at s == 1, all k slots after that;
//     - the top-k of an explored row is taken value descending, index ascending (a stable argsort);
//     - a row whose input token is 0 (a slot never filled) has an ALL-ZERO log-probability row (MaskZero(LogSoftMax),
//       decoders/gen.lua:24): its top-k is indices 0..k-1 at value 0, and its LSTM state is zero (maskZero);
//     - token = index + 1; candidate score = scores[w] + (double)logp, added in fp64;
//     - insertion order is (w, rank).  <END> candidates go to the finished set; the rest are sorted stably by descending
//       score and the first n_keep = min(#cands, k) are kept;
//     - slot i < n_keep takes the candidate's column, score and the STEPPED state of its source slot; slots >= n_keep keep
//       their old column, score and PRE-step state (so their next token is 0 and the zero-row rule applies).
//  3. the answer is the finished candidate with the highest score, ties to the earliest inserted (step, then w, then rank);
//     if nothing finished, column 0 (the reference errors there).
//  4. all beamLen-1 steps run: zero rows can still add finished candidates.
//
// Diverse beam search (Vijayakumar et al. 2016, Hamming diversity) extends rules 1-4.  (In D1-D7 a "group" is one of the G beam groups
// WITHIN a round; the `groups` argument of the kernels and entry points below counts the units that keep one finished set: rounds in
// the plain search, (round, beam group) pairs in the grouped one.)  beamGroups G >= 1 divides k, k' = k / G, group
// g owns slots g k' .. g k' + k' - 1 of its round, beamDiversity lambda is a finite real >= 0; G = 1 is rules 1-4 unchanged.
// split_eval.py:beam_search_round restates D1-D7 on the host.
//  D1. rule 1 for every slot: every group starts from <START>, the round's encoder state and score 0.
//  D2. at step s = 1 .. beamLen-1 the groups run in the order g = 0 .. G-1.  count[v] = the number of slots of groups 0 .. g-1 of the
//      same round that were FILLED (slot i < n_keep of D6) with word v at this step: all zero for group 0, from zero at every step.
//      <END> never enters a slot, so it is never counted and never penalised.
//  D3. a group explores its first slot only at s == 1, all k' slots after that.  An explored slot's row is rule 2's: log-softmax, or
//      all zero if the slot's input token is 0.
//  D4. the row is penalised in fp32: a[v] = logp[v] - (float)lambda * (float)count[v], product and difference rounded separately (no
//      fused multiply-add: __fmul_rn / __fsub_rn).  The slot's candidates are the top k' of a, value descending, index ascending.  An
//      all-zero row is penalised the same way.
//  D5. a candidate of slot w with word v carries two fp64 sums: the KEY scores[w] + (double)a[v], which only orders the unfinished
//      candidates of this group at this step, and the SCORE scores[w] + (double)logp[v], the true log-likelihood, which is carried
//      into the slot and reported.
//  D6. rule 2 within the group: insertion order (w, rank in D4); <END> candidates go to the group's own finished set with their score;
//      the rest are sorted stably by descending key and the first n_keep = min(#cands, k') fill the group's slots 0 .. n_keep-1 with
//      column, score and the stepped state of the source slot; slots >= n_keep keep column, score and pre-step state.
//  D7. a group's answer is its best finished candidate by score, ties to the earliest inserted; its first slot's column and score if
//      it finished nothing.  The round's answer is the highest-scoring answer among the groups that finished something, ties to the
//      lower group; group 0's if none did.  All beamLen-1 steps run.
// A penalty only lowers a value, and at most (G-1) k' distinct words are penalised, so the top k' of a penalised row lie within the
// top k of the unpenalised one: beam_topk_kernel at the full k delivers everything a step needs, and ONE beam_advance_kernel takes G as
// an argument (G = 1 ranks nothing anew and penalises nothing).  Per (round, group) the best finished candidate, the initial state and
// the answer are rule 1 / rule 3 of N * G groups of k' slots, so beam_init_kernel and beam_finish_kernel take (N * G, k').
//
// Constraints (behind rules 1-4 and D1-D7; all off by default, and then everything above is unchanged): minimum length m >= 0, no-repeat
// n-gram size n >= 0, length penalty alpha >= 0 (finite).  split_eval.py restates them (beam_banned, beam_search_round, pick_answer).
//  C1. the words of a slot's column at step s are g_1 .. g_(s-1), positions 1 .. s-1 of the column.  Position 0, <START>, is not a word.
//      An n-gram that holds a 0 is ignored (a 0 stands in the column of a slot that was never filled).
//  C2. minimum length: at every step s <= m, <END> is banned (a candidate that ends at step s has s - 1 words).
//  C3. no-repeat n-gram, for n >= 1 once s >= n: p = the last n - 1 words (empty for n = 1); for every i in 1 .. s - n with
//      g_i .. g_(i+n-2) = p the word g_(i+n-1) is banned.  A column yields at most s - 1 bans: at most beamLen - 1 with <END>.
//  C4. a banned word's value is -inf in the explored row, the log-softmax row and the all-zero row of a token-0 slot alike.  Nothing is
//      renormalised: the log-sum-exp is the full row's, so every other value is bit-identical.  The top-k stays rule 2 over what remains
//      (value descending, index ascending); D4 penalises what remains.  vd_model_beam_search refuses vocabSize < beamSize + beamLen - 1
//      while a ban is on, so that k finite candidates always exist, and m > beamLen - 2 (<END> must be allowed at the last step).
//  C5. scores stay the true log-likelihood, carried and reported as before.
//  C6. length penalty: a finished candidate that ends at step s has length s (its words plus <END>).  Within one step the best finished
//      candidate is chosen by score as before (one length).  Across steps a new best x replaces the incumbent y iff
//      x.score * lp[y.len] > y.score * lp[x.len], lp[s] = s^alpha computed ON THE HOST in fp64 (std::pow here, float(s) ** alpha in
//      Python: one libm) and uploaded as a table; each product is one IEEE fp64 multiplication (__dmul_rn).  No division and no device
//      pow: host and device decide bit for bit alike.  Ties stay with the earliest inserted.  D7's choice among the groups of a round
//      uses the same comparison, ties to the lower group, the length being the position of <END> in the answer.  "Nothing finished"
//      falls back as before.
// On the device C2-C4 are the constrained form of the top-k kernel (it reads the row's column from the PRE-advance history), C6 the
// advance kernel's `lp` argument (nullptr = off); with every knob off the top-k is the plain kernel with the arguments it always had.
//
// Rollout (VD_BEAM_ROLLOUT = 1 at vd_model_create; generate.py -rollout 1): round r is answered on a history that holds the model's OWN
// answers to the rounds before it, not the ground truth's.  split_eval.py restates R2 / R3 (rollout_history_row) and the host loop.  Th is
// the width of the uploaded history, lq the number of non-zero tokens of a question row.
//  R1. round 0's history row is the uploaded one (the caption).
//  R2. for r >= 1, history row r of a dialog is the non-zero tokens of question row r - 1, in order, then the first min(la, Th - lq) words
//      of the answer chosen for round r - 1 (la of them), right-aligned in Th columns with zeros in front.  lq = 0 and no words: an
//      all-zero row (what the test split's missing rounds produce).  The question is kept whole; the answer is what is cut.
//  R3. the words of an answer are entries 1, 2, ... of the round's returned token row [beamLen], up to but excluding the first <END> or 0.
//      Entry 0 is <START> and is not a word.  An answer that never finished (slot 0's column, no <END>) gives all its beamLen - 1 words.
//  R4. the answer chosen for a round is exactly what the search returns for it: rule 3 (C6 under a length penalty), with C1-C4 in force if
//      they are on; its score stays the true log-likelihood.  Groups (D1-D7) are refused: the choice among them is the host's.
//  R5. round r is answered from an encoder pass in which rows 0 .. r of its dialog are as above.  Whatever rows > r hold at that time does
//      not reach round r: every encoder is causal over the rounds (lf reads its own row, hre runs a forward dialog LSTM, mn attends over
//      the earlier rounds only).
//  R6. the uploaded contents of history rows >= 1 are ignored and overwritten; after the call the batch's device history holds the
//      generated rows.
// On the device a chunk of B dialogs runs R passes (Gen_beam_search, rt_decoders.h): encoder forward, the search of round r of every dialog
// (B groups, the kernels above unchanged), beam_rollout_append_kernel for row r + 1.  Nothing waits for the host between passes.
//
// Rollout of the discriminative decoder (VD_RETRIEVE_ROLLOUT = 1 at vd_model_create; evaluate.py -rollout 1): the candidates of round r are
// RANKED on a history that holds the model's own picks for the rounds before it.  split_eval.py restates E2 - E4 (rollout_pick,
// rollout_candidate_row, rollout_history_row) and the host loop (retrieve_rollout_batch).  O = numOptions, To = the width of an option row.
//  E1. round 0's history row is the uploaded one (R1).
//  E2. the answer chosen for round r is the candidate that vd_ranks gives rank 1 among the round's O scores: the highest score, and among
//      equal scores the lowest index (duplicate candidates inside one round are common).
//  E3. the words of a candidate are entries 0, 1, ... of its `options` row [To], up to but excluding the first 0: the rows are left-aligned
//      and hold neither <START> nor <END>.  An all-zero row is an empty answer.
//  E4. history row r + 1 is built by R2 from question row r and those words: the question's non-zero tokens first and whole, then the first
//      min(la, Th - lq) words, right-aligned in Th columns; lq = 0 and no words: an all-zero row.
//  E5. R5 and R6 hold as written: round r is scored from an encoder pass in which rows 0 .. r are final; the uploaded rows >= 1 are ignored
//      and overwritten; after the call the slot's device history holds the generated rows.  The scores, ranks and loss the call leaves are
//      those of the pass after the last append, an ordinary scoring of all N rounds: rows <= r of a dialog do not change after pass r and
//      every encoder is causal, so that pass scores round r exactly as pass r did.
// An option's encoding depends on its tokens and the weights only, so the option LSTM runs ONCE; a chunk then runs R passes (Disc::
// retrieve_rollout, rt_decoders.h): encoder forward, vd_score_ce over all N rounds, disc_rollout_pick_kernel for row r + 1 (not after the
// last).  Nothing waits for the host between passes.  For decoder gen the answer fed back is the beam search's (R4).
//
// Rollout on a concatenated history (VD_ROLLOUT_CONCAT_END = the <END> id at vd_model_create, with either rollout above; evaluate.py -rollout 1
// -rolloutHistory concat): the encoders whose history row is the running concatenation of the dialog (lf-ques-hist, lf-ques-im-hist,
// lf-att-ques-im-hist; dataloader.lua:243-255).  split_eval.py restates CH2 - CH4 (rollout_concat_row) and the host loops.  W is the width of
// the uploaded history, END the <END> token id.
//  CH1. row 0 is the uploaded row (R1).
//  CH2. lenH(r) = W - (the index of the first non-zero column of row r), and 0 for an all-zero row.  The last lenH columns of row r are its
//       tokens, carried over as they are (a 0 among them included).
//  CH3. the new tokens of round r are END, then the non-zero tokens of question row r in order, then the answer's words: R3 for a beam answer,
//       E2 / E3 for a picked candidate.  END is appended even when the question is empty and there are no words, as dataloader.lua:243-255
//       does for the missing rounds of the test split.
//  CH4. row r + 1 is row r's lenH tokens followed by the first min(n_new, W - lenH) new tokens, right-aligned in W columns with zeros in
//       front.  What does not fit is cut at the end: words first, then question tokens, then END; a full row repeats itself.  (The
//       reference's loader has no such case: it would index out of range.)  The cut keeps every row a prefix extension of the one before;
//       CH6 rests on that.
//  CH5. R5, R6 and E5 hold as written: an lf encoder reads only its own row.
//  CH6. prefix property: the history stack's state after row r + 1 is its state after row r continued over the kept new tokens.
// On the device the append and pick kernels below write the row through rollout_concat_row instead of R2's body when the model's END is set;
// the passes are otherwise the ones above.
#include "common.h"

#define VD_BEAM_KMAX 32
#define VD_BEAM_GKMAX (VD_BEAM_KMAX / 2)   // the largest k' = k / G at G >= 2
// VD_BEAM_LMAX (common.h): the longest beamLen while n-gram blocking is on -- a column and its ban list sit in LDS

namespace {

// value descending, index ascending
__device__ __forceinline__ bool beam_better(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

// Fused nn.LogSoftMax + top-k of one hypothesis row per workgroup.  The log-sum-exp is block_row_lse (common.h), which
// log_softmax_rows_kernel (loss.hip) calls too, so every value is bit-identical to that kernel's output row[c] - lse.  Each
// thread keeps a sorted list of its KM best (value, index) pairs in registers (compile-time indices only: no scratch), then
// k rounds of a workgroup arg-max over the list heads pop the row's top-k in order.
//
// BAN (C1-C4): `hist` is the PRE-advance history [rows x L], `step` the step being taken.  Wave 0 builds the row's ban list (word
// indices, at most L - 1 <= VD_BEAM_LMAX - 1 of them) in LDS: lane i tests the window that starts at word i against the last n - 1
// words.  A thread scans the columns c = tid (mod 256), so it first notes whether any banned index is one of its own; only such a
// thread (almost none: the list is short) asks the list again, for a column that would enter its sorted list.  The token-0 row returns
// the k lowest unbanned indices at value 0.
template <int KM, bool BAN>
__device__ __forceinline__ void
beam_topk_body(const float* x, long ld, int V, const int32_t* tok, int k, const int32_t* hist, int L,
               int step, int min_len, int no_repeat, int end_tok, int32_t* top_idx, float* top_val) {
  __shared__ float red[8];
  __shared__ float wv[4];
  __shared__ int wi[4];
  __shared__ int col[BAN ? VD_BEAM_LMAX : 1], ban[BAN ? VD_BEAM_LMAX : 1];
  __shared__ int n_ban;
  const long r = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t* oi = top_idx + r * k;
  float* ov = top_val + r * k;
  int nb = 0;
  if constexpr (BAN) {
    const bool ngram = no_repeat >= 1 && step >= no_repeat;        // C3; the entry point holds L <= VD_BEAM_LMAX while n >= 1
    if (ngram && tid < step) col[tid] = hist[r * L + tid];         // positions 0 .. s-1
    if (tid == 0) {
      n_ban = 0;
      if (step <= min_len) { ban[0] = end_tok - 1; n_ban = 1; }    // C2
    }
    __syncthreads();
    if (ngram && tid >= 1 && tid <= step - no_repeat) {            // the window g_tid .. g_(tid+n-2) against p = g_(s-n+1) .. g_(s-1)
      const int w = col[tid + no_repeat - 1];
      bool hit = w != 0;                                           // C1: an n-gram that holds a 0 is ignored
      for (int j = 0; j < no_repeat - 1; ++j) {
        const int a = col[tid + j], b = col[step - no_repeat + 1 + j];
        hit = hit && a == b && b != 0;
      }
      if (hit) ban[atomicAdd(&n_ban, 1)] = w - 1;                  // at most s - n <= L - 2 of these next to <END>
    }
    __syncthreads();
    nb = n_ban;
  }
  auto banned = [&](int c) {
    bool b = false;
    for (int j = 0; j < nb; ++j) b = b || ban[j] == c;
    return b;
  };
  if (tok[r] == 0) {                     // MaskZero(LogSoftMax): an all-zero row, ties to the lower index
    if constexpr (BAN) {
      if (wave == 0) {                   // the k lowest unbanned indices: 64 columns at a time, a lane's place from the ballot
        int q0 = 0;
        for (int base = 0; q0 < k && base < V; base += 64) {
          const int c = base + lane;
          const bool ok = c < V && !banned(c);
          const unsigned long long mask = __ballot(ok);
          const int q = q0 + __popcll(mask & ((1ull << lane) - 1ull));
          if (ok && q < k) { oi[q] = c; ov[q] = 0.f; }
          q0 += __popcll(mask);
        }
      }
    } else {
      if (tid < k) { oi[tid] = tid; ov[tid] = 0.f; }
    }
    return;
  }
  const float* row = x + r * ld;
  const float lse = block_row_lse(row, V, red);

  bool mine = false;                     // BAN: does a banned index fall among this thread's columns
  for (int j = 0; j < nb; ++j) mine = mine || (ban[j] & 255) == tid;
  float lv[KM];
  int li[KM];
#pragma unroll
  for (int j = 0; j < KM; ++j) { lv[j] = -INFINITY; li[j] = INT_MAX; }
  for (int c = tid; c < V; c += 256) {   // ascending c: an equal value never overtakes an earlier index
    const float v = row[c] - lse;
    if (beam_better(v, c, lv[KM - 1], li[KM - 1]) && !(BAN && mine && banned(c))) {
      lv[KM - 1] = v;
      li[KM - 1] = c;
#pragma unroll
      for (int j = KM - 1; j > 0; --j) {
        if (beam_better(lv[j], li[j], lv[j - 1], li[j - 1])) {
          const float tv = lv[j]; lv[j] = lv[j - 1]; lv[j - 1] = tv;
          const int ti = li[j]; li[j] = li[j - 1]; li[j - 1] = ti;
        }
      }
    }
  }
  for (int q = 0; q < k; ++q) {
    float bv = lv[0];
    int bi = li[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float v2 = __shfl_xor(bv, o, 64);
      const int i2 = __shfl_xor(bi, o, 64);
      if (beam_better(v2, i2, bv, bi)) { bv = v2; bi = i2; }
    }
    if (lane == 0) { wv[wave] = bv; wi[wave] = bi; }
    __syncthreads();
    bv = wv[0]; bi = wi[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (beam_better(wv[w], wi[w], bv, bi)) { bv = wv[w]; bi = wi[w]; }
    if (tid == 0) { oi[q] = bi; ov[q] = bv; }
    if (li[0] == bi) {                   // indices are unique across threads: exactly one owner pops its head
#pragma unroll
      for (int j = 0; j < KM - 1; ++j) { lv[j] = lv[j + 1]; li[j] = li[j + 1]; }
      lv[KM - 1] = -INFINITY;
      li[KM - 1] = INT_MAX;
    }
    __syncthreads();                     // wv / wi are rewritten by the next round
  }
}

template <int KM>
__global__ void __launch_bounds__(256)
beam_topk_kernel(const float* __restrict__ x, long ld, int V, const int32_t* __restrict__ tok, int k,
                 int32_t* __restrict__ top_idx, float* __restrict__ top_val) {
  beam_topk_body<KM, false>(x, ld, V, tok, k, nullptr, 0, 0, 0, 0, 0, top_idx, top_val);
}

template <int KM>
__global__ void __launch_bounds__(256)
beam_topk_ban_kernel(const float* __restrict__ x, long ld, int V, const int32_t* __restrict__ tok, int k, const int32_t* __restrict__ hist,
                     int L, int step, int min_len, int no_repeat, int end_tok, int32_t* __restrict__ top_idx,
                     float* __restrict__ top_val) {
  beam_topk_body<KM, true>(x, ld, V, tok, k, hist, L, step, min_len, no_repeat, end_tok, top_idx, top_val);
}

// rule 1 for every group: history column <START>, 0, ..., next token <START>, scores 0, no finished candidate
__global__ void beam_init_kernel(int groups, int k, int L, int start, int32_t* __restrict__ hist, int32_t* __restrict__ tok,
                                 double* __restrict__ scores, double* __restrict__ best_score, int32_t* __restrict__ best_len) {
  const long n = (long)groups * k;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n * L; e += (long)gridDim.x * blockDim.x) {
    hist[e] = e % L == 0 ? start : 0;
    if (e < n) { tok[e] = start; scores[e] = 0.0; }
    if (e < groups) { best_score[e] = 0.0; best_len[e] = 0; }
  }
}

// C6: `lp` [L] holds s^alpha at index s, the length of a candidate that ends at step s
__device__ __forceinline__ bool beam_replaces(double x_score, int x_len, double y_score, int y_len, const double* __restrict__ lp) {
  return __dmul_rn(x_score, lp[y_len]) > __dmul_rn(y_score, lp[x_len]);
}

// Rule 2 / D2-D6 for one round per workgroup, its G groups of k' = k / G slots one after another (a group's penalties need the earlier
// groups' slots).  Candidate c = w * k' + rank (insertion order) carries a KEY and a SCORE (D5).  A candidate's place among its kind is
// the number of that kind with a higher value or an equal value inserted earlier: for the unfinished ones, by key, that is the stable
// sort's position; for the finished ones, by score, place 0 is this step's best.  The best finished candidate so far is kept per
// (round, group) (score, length + 1, column); a later one replaces it only with a strictly higher score -- under `lp` (C6, nullptr =
// off) by beam_replaces, best_len - 1 the incumbent's length -- so ties stay with the earliest inserted (rule 3).
//  G == 1: a candidate's rank is its position in the row the caller handed over (vd_beam_advance takes rows in any order), and its key
//          IS its score: the candidate tables are filled straight from top_idx / top_val, and `ckey` aliases `csc`.
//  G >= 2: `count` is a list of (word, multiplicity) pairs, at most one per slot of the earlier groups.  The k candidates of every
//          explored slot (beam_topk_kernel's, unpenalised order) get their penalised value and their rank under it (D4); the ranks
//          < k' are the slot's candidates.  k' <= VD_BEAM_GKMAX.
// best_* are indexed round * G + group; `src` is a round-local slot index.  ONE: G == 1 at compile time -- the same source with the G >= 2
// passes and tables folded away, because the kernel with G read at run time took 6.7 us against 6.0 us (profiles/beam_fold.txt).
template <bool ONE>
__global__ void __launch_bounds__(256)
beam_advance_kernel(const int32_t* __restrict__ top_idx, const float* __restrict__ top_val, int k, int groups, float lambda, int step, int L,
                    int end_tok, double* __restrict__ scores, const int32_t* __restrict__ hist_in, int32_t* __restrict__ hist_out,
                    int32_t* __restrict__ src, int32_t* __restrict__ next_tok, double* __restrict__ best_score,
                    int32_t* __restrict__ best_len, int32_t* __restrict__ best_hist, const double* __restrict__ lp) {
  constexpr int KP = ONE ? VD_BEAM_KMAX : VD_BEAM_GKMAX;          // the largest k'
  __shared__ float pen[ONE ? 1 : KP * VD_BEAM_KMAX];
  __shared__ double key_tab[ONE ? 1 : KP * KP], csc[KP * KP];
  __shared__ int ctok[KP * KP];
  __shared__ double slot_sc[KP];
  __shared__ int slot_src[KP], slot_tok[KP];
  __shared__ int cnt_word[VD_BEAM_KMAX], cnt_mult[VD_BEAM_KMAX];
  __shared__ int n_cnt, n_cands, best_c;
  const int r = blockIdx.x, tid = threadIdx.x;
  const long r0 = (long)r * k;
  const int G = ONE ? 1 : groups, kp = k / G, explore = step == 1 ? 1 : kp, C = explore * kp, E = explore * k;
  double* ckey = ONE ? csc : key_tab;
  if (tid == 0) n_cnt = 0;
  for (int g = 0; g < G; ++g) {
    const long g0 = r0 + (long)g * kp;                             // the group's first hypothesis row
    __syncthreads();                                               // the earlier group is done with the tables; its counts are in
    if (tid == 0) { n_cands = 0; best_c = -1; }
    if (tid < KP) { slot_src[tid] = 0; slot_tok[tid] = 0; slot_sc[tid] = 0.0; }   // valid even if a NaN left a place unfilled
    if (ONE) {
      for (int c = tid; c < C; c += blockDim.x) {
        const int w = c / k;
        ctok[c] = top_idx[g0 * k + c] + 1;                         // vocabulary ids are 1-based
        csc[c] = scores[g0 + w] + (double)top_val[g0 * k + c];     // fp64, as the hosts add
      }
    } else {
      for (int c = tid; c < C; c += blockDim.x) { ctok[c] = 0; ckey[c] = 0.0; csc[c] = 0.0; }
      for (int e = tid; e < E; e += blockDim.x) {                  // D4
        const int w = e / k, q = e - w * k;
        const long t = (g0 + w) * k + q;
        const int v = top_idx[t];
        int mult = 0;
        for (int j = 0; j < n_cnt; ++j) mult = cnt_word[j] == v ? cnt_mult[j] : mult;
        pen[e] = __fsub_rn(top_val[t], __fmul_rn(lambda, (float)mult));
      }
      __syncthreads();
      for (int e = tid; e < E; e += blockDim.x) {
        const int w = e / k, q = e - w * k;
        const long t0 = (g0 + w) * k;
        const float av = pen[e];
        const int ai = top_idx[t0 + q];
        int rank = 0;
        for (int q2 = 0; q2 < k; ++q2) rank += beam_better(pen[w * k + q2], top_idx[t0 + q2], av, ai) ? 1 : 0;
        if (rank < kp) {                                           // D5
          const int c = w * kp + rank;
          const double s = scores[g0 + w];
          ctok[c] = ai + 1;
          ckey[c] = s + (double)av;
          csc[c] = s + (double)top_val[t0 + q];
        }
      }
    }
    __syncthreads();
    for (int c = tid; c < C; c += blockDim.x) {                    // D6
      const bool fin = ctok[c] == end_tok;
      const double v = fin ? csc[c] : ckey[c];
      int pos = 0;
      for (int c2 = 0; c2 < C; ++c2) {
        if ((ctok[c2] == end_tok) != fin) continue;
        const double v2 = fin ? csc[c2] : ckey[c2];
        pos += (v2 > v || (v2 == v && c2 < c)) ? 1 : 0;
      }
      if (fin) {
        if (pos == 0) best_c = c;
      } else {
        atomicAdd(&n_cands, 1);
        if (pos < kp) { slot_sc[pos] = csc[c]; slot_src[pos] = c / kp; slot_tok[pos] = ctok[c]; }
      }
    }
    __syncthreads();
    const int n_keep = min(n_cands, kp);
    if (tid == 0) {
      const long bg = (long)r * G + g;
      if (best_c >= 0) {
        const double sc = csc[best_c];
        if (best_len[bg] == 0 || (lp ? beam_replaces(sc, step, best_score[bg], best_len[bg] - 1, lp) : sc > best_score[bg])) {
          const int32_t* col = hist_in + (g0 + best_c / kp) * L;
          best_score[bg] = sc;
          best_len[bg] = step + 1;
          for (int p = 0; p < L; ++p) best_hist[bg * L + p] = p < step ? col[p] : p == step ? end_tok : 0;
        }
      }
      for (int i = 0; g + 1 < G && i < n_keep; ++i) {              // D2: the filled slots' words, for the groups after this one
        const int v = slot_tok[i] - 1;
        int j = 0;
        while (j < n_cnt && cnt_word[j] != v) ++j;
        if (j == n_cnt) { cnt_word[j] = v; cnt_mult[j] = 0; n_cnt = j + 1; }
        cnt_mult[j] += 1;
      }
    }
    for (int e = tid; e < kp * L; e += blockDim.x) {
      const int i = e / L, p = e - i * L;
      int v;
      if (i < n_keep) v = p == step ? slot_tok[i] : hist_in[(g0 + slot_src[i]) * L + p];
      else v = hist_in[(g0 + i) * L + p];
      hist_out[(g0 + i) * L + p] = v;
      if (p == step) next_tok[g0 + i] = v;
    }
    for (int i = tid; i < kp; i += blockDim.x) {
      src[g0 + i] = i < n_keep ? g * kp + slot_src[i] : -1;
      if (i < n_keep) scores[g0 + i] = slot_sc[i];                 // the group's reads of `scores` are a barrier or more back
    }
  }
}

// cur[r] = stepped[group(r) * k + src[r]] where src[r] >= 0; the row is left alone otherwise
__global__ void beam_select_rows_kernel(float* __restrict__ cur, const float* __restrict__ stepped, const int32_t* __restrict__ src,
                                        long rows, int k, int H) {
  const long n = rows * H;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    const long r = e / H;
    const int s = src[r];
    if (s >= 0) cur[e] = stepped[((r / k) * k + s) * H + (e - r * H)];
  }
}

// rule 3: the best finished candidate, else column 0 and its score
__global__ void beam_finish_kernel(int groups, int k, int L, const int32_t* __restrict__ hist, const double* __restrict__ scores,
                                   const double* __restrict__ best_score, const int32_t* __restrict__ best_len,
                                   const int32_t* __restrict__ best_hist, int32_t* __restrict__ out_tok, double* __restrict__ out_score) {
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < (long)groups * L; e += (long)gridDim.x * blockDim.x) {
    const long g = e / L, p = e - g * L;
    const bool fin = best_len[g] > 0;
    out_tok[e] = fin ? best_hist[e] : hist[g * k * L + p];
    if (p == 0) out_score[g] = fin ? best_score[g] : scores[g * k];
  }
}

// R2 for one history row, by the one wave of the workgroup: row nq + 1 of the step-major tokens from question row nq and `la` words, word i at
// words[i * stride] (stride 1: a row of answer tokens; the row count of a step-major token table: one of its rows).  The wave counts lq
// with ballots while it compacts the question's non-zero tokens into LDS (a lane's place = the set bits below it) and then makes ONE pass
// over the Th columns: column c holds 0, a question token or a word by its distance from the right edge alone, so every column is written
// exactly once, with plain vector stores, into the step-major tokens [Th x N] and (inv != nullptr) the length-sorted copy the wavefront
// masks with.  Both are step-major, so a dialog's columns lie N apart: a wave's stores are strided whatever the lane order, and at
// B x Th x 4 bytes per pass (1.1 KB at B = 20, Th = 14) the launch is what costs.  Tq <= VD_ROLLOUT_TMAX (the LDS list), lq <= Tq <= Th.
#define VD_ROLLOUT_TMAX 1024
__device__ __forceinline__ void rollout_write_row(const int32_t* __restrict__ ques, int Tq, long N, long nq, const int32_t* __restrict__ words,
                                                  long stride, int la, int Th, int32_t* __restrict__ hist_tok,
                                                  int32_t* __restrict__ hist_sorted, const int32_t* __restrict__ inv) {
  __shared__ int32_t qc[VD_ROLLOUT_TMAX];
  const int lane = threadIdx.x;
  const long nh = nq + 1;                                          // the history row the round just answered becomes
  int lq = 0;
  for (int base = 0; base < Tq; base += 64) {
    const int t = base + lane;
    const int32_t v = t < Tq ? ques[(long)t * N + nq] : 0;
    const unsigned long long mask = __ballot(v != 0);
    if (v != 0) qc[lq + __popcll(mask & ((1ull << lane) - 1ull))] = v;
    lq += __popcll(mask);
  }
  __syncthreads();
  const int pad = Th - lq - min(la, Th - lq);                      // R2: zeros in front
  for (int base = 0; base < Th; base += 64) {
    const int c = base + lane, j = c - pad;
    if (c >= Th) break;
    const int32_t v = j < 0 ? 0 : j < lq ? qc[j] : words[(long)(j - lq) * stride];
    hist_tok[(long)c * N + nh] = v;
    if (hist_sorted) hist_sorted[(long)c * N + inv[nh]] = v;
  }
}

// CH2 - CH4 for one history row, by the one wave of the workgroup: row nq + 1 from ROW nq, <END>, question row nq and `la` words (as above).
// The wave compacts the question as above, finds row nq's first non-zero column with a ballot per 64 columns (CH2: lenH = W - that column) and
// makes ONE pass over the W columns.  With keep = min(1 + lq + la, W - lenH) new tokens kept, the new row is the old one moved `keep` columns
// to the left with the kept tokens behind it, so column c holds old column c + keep while that lies inside the row (its leading zeros
// included: lenH + keep <= W, nothing non-zero moves out) and new token c + keep - W otherwise: a value by the distance from the right edge
// alone, every column written exactly once, plain vector stores into both layouts.  keep = 0: the row repeats itself.  Rows nq and nq + 1
// are different columns of the table, so nothing read here is written here; the previous pass's stores are visible across the launch.
// CH2 by the one wave of the workgroup: the first non-zero column of row n of the step-major tokens [W x N], W for an all-zero row
__device__ __forceinline__ int rollout_first_column(const int32_t* hist_tok, long N, long n, int W) {
  const int lane = threadIdx.x;
  for (int base = 0; base < W; base += 64) {
    const int c = base + lane;
    const unsigned long long mask = __ballot(c < W && hist_tok[(long)c * N + n] != 0);
    if (mask) return base + __ffsll((long long)mask) - 1;
  }
  return W;
}
__device__ __forceinline__ void rollout_concat_row(const int32_t* __restrict__ ques, int Tq, long N, long nq, const int32_t* __restrict__ words,
                                                   long stride, int la, int W, int end_tok, int32_t* hist_tok,
                                                   int32_t* __restrict__ hist_sorted, const int32_t* __restrict__ inv) {
  __shared__ int32_t qn[VD_ROLLOUT_TMAX];
  const int lane = threadIdx.x;
  const long nh = nq + 1;
  int lq = 0;
  for (int base = 0; base < Tq; base += 64) {
    const int t = base + lane;
    const int32_t v = t < Tq ? ques[(long)t * N + nq] : 0;
    const unsigned long long mask = __ballot(v != 0);
    if (v != 0) qn[lq + __popcll(mask & ((1ull << lane) - 1ull))] = v;
    lq += __popcll(mask);
  }
  __syncthreads();
  const int first = rollout_first_column(hist_tok, N, nq, W);     // CH2
  const int keep = min(1 + lq + la, first);                        // CH4: W - lenH = first columns are free
  for (int base = 0; base < W; base += 64) {
    const int c = base + lane;
    if (c >= W) break;
    const int i = c + keep - W;                                    // >= 0: new token i (CH3); < 0: old column c + keep
    const int32_t v = i < 0 ? hist_tok[(long)(c + keep) * N + nq] : i == 0 ? end_tok : i <= lq ? qn[i - 1] : words[(long)(i - 1 - lq) * stride];
    hist_tok[(long)c * N + nh] = v;
    if (hist_sorted) hist_sorted[(long)c * N + inv[nh]] = v;
  }
}

// CH6 for the round pass (rt_encoders.h history_round_concat): the kept new tokens of history row r of every dialog, right-aligned in a
// step-major window [Wn x B] with zeros in front.  Row r is row r - 1 moved left with the kept tokens behind it (CH4), so they are its last
// keep = first(r - 1) - first(r) columns; the append kernels kept at most 1 + Tq + (words of an answer) of them, which the caller's Wn
// covers -- the clamp below only keeps a caller's mistake inside the window.  One wave per dialog, plain vector stores.
__global__ void __launch_bounds__(64)
rollout_concat_window_kernel(const int32_t* __restrict__ hist_tok, long N, int R, int r, int W, int Wn, int B, int32_t* __restrict__ win) {
  const int lane = threadIdx.x;
  const long n = (long)blockIdx.x * R + r;
  const int keep = max(0, min(rollout_first_column(hist_tok, N, n - 1, W) - rollout_first_column(hist_tok, N, n, W), Wn));
  for (int base = 0; base < Wn; base += 64) {
    const int c = base + lane;
    if (c >= Wn) break;
    const int j = c - (Wn - keep);
    win[(long)c * B + blockIdx.x] = j < 0 ? 0 : hist_tok[(long)(W - keep + j) * N + n];
  }
}

// R2 / R3 for one pass of a rollout: one wave per dialog writes history row r + 1 from question row r and the answer just chosen for
// round r.  The answer's word count is the first lane whose entry is <END>, 0 or past the row; the words start behind <START>.
// concat_end != 0 (VD_ROLLOUT_CONCAT_END): the row by CH2 - CH4 instead of R2.
__global__ void __launch_bounds__(64)
beam_rollout_append_kernel(const int32_t* __restrict__ answers, int L, int end_tok, const int32_t* __restrict__ ques, int Tq, long N, int R,
                           int r, int Th, int32_t* hist_tok, int32_t* __restrict__ hist_sorted,
                           const int32_t* __restrict__ inv, int concat_end) {
  const int lane = threadIdx.x;
  const int32_t* a = answers + (long)blockIdx.x * L;
  int la = 0;                                                      // R3: entries 1 .. la are the words
  for (int base = 1;; base += 64) {
    const int c = base + lane;
    const bool stop = c >= L || a[c] == end_tok || a[c] == 0;
    const unsigned long long mask = __ballot(stop);
    if (mask) {
      la = base + __ffsll((long long)mask) - 2;
      break;
    }
  }
  if (concat_end)
    rollout_concat_row(ques, Tq, N, (long)blockIdx.x * R + r, a + 1, 1, la, Th, concat_end, hist_tok, hist_sorted, inv);
  else
    rollout_write_row(ques, Tq, N, (long)blockIdx.x * R + r, a + 1, 1, la, Th, hist_tok, hist_sorted, inv);
}

// E2 - E4 for one pass of a discriminative rollout: one wave per dialog picks the rank-1 candidate of round r among its O <= 128 scores
// (two per lane; beam_better IS ranks_kernel's "nothing ranks before it" for finite scores: the highest score, the lowest index among
// equals), finds its tokens in the option tokens the step already holds -- step-major [To x rows], row = opt_uid[candidate] where the
// upload de-duplicated, the candidate itself otherwise --, counts its words up to the first 0 with a ballot (E3: left-aligned, no
// <START>, no <END>) and writes history row r + 1 through rollout_write_row.  Lane 0's result is broadcast: with a NaN among the scores
// the butterfly's lanes need not agree, and the row must come from ONE candidate.
#define VD_DISC_PICK_OMAX 128   // loss.hip's MAX_OPT
__global__ void __launch_bounds__(64)
disc_rollout_pick_kernel(const float* __restrict__ scores, int O, const int32_t* __restrict__ opt_tok, long rows, int To,
                         const int32_t* __restrict__ opt_uid, const int32_t* __restrict__ ques, int Tq, long N, int R, int r, int Th,
                         int32_t* hist_tok, int32_t* __restrict__ hist_sorted, const int32_t* __restrict__ inv, int concat_end) {
  const int lane = threadIdx.x;
  const long nq = (long)blockIdx.x * R + r;
  const float* s = scores + nq * O;
  float bv = lane < O ? s[lane] : -INFINITY;                       // (a lane without a score never wins: INT_MAX is no index)
  int bi = lane < O ? lane : INT_MAX;
  if (lane + 64 < O && beam_better(s[lane + 64], lane + 64, bv, bi)) { bv = s[lane + 64]; bi = lane + 64; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(bv, o, 64);
    const int i2 = __shfl_xor(bi, o, 64);
    if (beam_better(v2, i2, bv, bi)) { bv = v2; bi = i2; }
  }
  bi = __shfl(bi, 0, 64);                                          // E2; lane 0 holds an index < O whatever the scores are
  const long cand = nq * O + bi;
  const int32_t* w = opt_tok + (opt_uid ? (long)opt_uid[cand] : cand);
  int la = 0;                                                      // E3: entries 0 .. la - 1 are the words
  for (int base = 0;; base += 64) {
    const int t = base + lane;
    const bool stop = t >= To || w[(long)t * rows] == 0;
    const unsigned long long mask = __ballot(stop);
    if (mask) {
      la = base + __ffsll((long long)mask) - 1;
      break;
    }
  }
  if (concat_end)                                                  // VD_ROLLOUT_CONCAT_END: CH2 - CH4 instead of E4
    rollout_concat_row(ques, Tq, N, nq, w, rows, la, Th, concat_end, hist_tok, hist_sorted, inv);
  else
    rollout_write_row(ques, Tq, N, nq, w, rows, la, Th, hist_tok, hist_sorted, inv);
}

}  // namespace

// R2 / R3 (rt_core.h): history row r + 1 of `dialogs` dialogs from question row r and `answers` [dialogs x beam_len]
int vd_beam_rollout_append_p(const int32_t* answers, int beam_len, int end_token, const int32_t* ques, int Tq, int dialogs, int R, int r,
                             int32_t* hist_tok, int32_t* hist_sorted, const int32_t* inv, int Th, hipStream_t stream, int concat_end) {
  VD_CHECK_ARG(answers && ques && hist_tok && beam_len >= 1 && dialogs >= 0 && (hist_sorted == nullptr) == (inv == nullptr) && concat_end >= 0,
               "vd_beam_rollout_append: bad args");
  VD_CHECK_ARG(R >= 2 && r >= 0 && r + 1 < R, "vd_beam_rollout_append: round %d has no next round among %d", r, R);
  VD_CHECK_ARG(Tq >= 1 && Tq <= VD_ROLLOUT_TMAX && Th >= Tq, "vd_beam_rollout_append: question width %d must be in [1, %d] and <= history width %d",
               Tq, VD_ROLLOUT_TMAX, Th);
  if (dialogs == 0) return VD_OK;
  hipLaunchKernelGGL(beam_rollout_append_kernel, dim3((unsigned)dialogs), dim3(64), 0, stream, answers, beam_len, end_token, ques, Tq,
                     (long)dialogs * R, R, r, Th, hist_tok, hist_sorted, inv, concat_end);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

// CH6 (rt_core.h): the kept new tokens of history row r of `dialogs` dialogs as a window [Wn x dialogs]
int vd_rollout_concat_window_p(const int32_t* hist_tok, int dialogs, int R, int r, int W, int Wn, int32_t* win, hipStream_t stream) {
  VD_CHECK_ARG(hist_tok && win && dialogs >= 0 && R >= 2 && r >= 1 && r < R && Wn >= 1 && Wn <= W,
               "vd_rollout_concat_window: bad args (round %d of %d, window %d of %d columns)", r, R, Wn, W);
  if (dialogs == 0) return VD_OK;
  hipLaunchKernelGGL(rollout_concat_window_kernel, dim3((unsigned)dialogs), dim3(64), 0, stream, hist_tok, (long)dialogs * R, R, r, W, Wn,
                     dialogs, win);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

// E2 - E4 (rt_core.h): history row r + 1 of `dialogs` dialogs from question row r and the rank-1 candidate of scores row dialog * R + r
int vd_disc_rollout_pick_p(const float* scores, int O, const int32_t* opt_tok, int64_t opt_rows, int To, const int32_t* opt_uid,
                           const int32_t* ques, int Tq, int dialogs, int R, int r, int32_t* hist_tok, int32_t* hist_sorted,
                           const int32_t* inv, int Th, hipStream_t stream, int concat_end) {
  VD_CHECK_ARG(scores && opt_tok && ques && hist_tok && To >= 1 && dialogs >= 0 && (hist_sorted == nullptr) == (inv == nullptr) && concat_end >= 0,
               "vd_disc_rollout_pick: bad args");
  VD_CHECK_ARG(O >= 1 && O <= VD_DISC_PICK_OMAX, "vd_disc_rollout_pick: O = %d candidates per round must be in [1, MAX_OPT = %d]", O,
               VD_DISC_PICK_OMAX);
  VD_CHECK_ARG(R >= 2 && r >= 0 && r + 1 < R, "vd_disc_rollout_pick: round %d has no next round among %d", r, R);
  VD_CHECK_ARG(Tq >= 1 && Tq <= VD_ROLLOUT_TMAX && Th >= Tq, "vd_disc_rollout_pick: question width %d must be in [1, %d] and <= history width %d",
               Tq, VD_ROLLOUT_TMAX, Th);
  // without opt_uid a candidate is its own row: the table has to hold every candidate (with it, the upload numbered the rows it holds)
  VD_CHECK_ARG(opt_rows >= 1 && (opt_uid || opt_rows == (int64_t)dialogs * R * O),
               "vd_disc_rollout_pick: %lld option rows for %d x %d x %d candidates", (long long)opt_rows, dialogs, R, O);
  if (dialogs == 0) return VD_OK;
  hipLaunchKernelGGL(disc_rollout_pick_kernel, dim3((unsigned)dialogs), dim3(64), 0, stream, scores, O, opt_tok, (long)opt_rows, To, opt_uid,
                     ques, Tq, (long)dialogs * R, R, r, Th, hist_tok, hist_sorted, inv, concat_end);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

// vd_beam_advance (rt_core.h): `rounds` rounds of G groups of k / G slots
int vd_beam_advance_p(const int32_t* top_idx, const float* top_val, int rounds, int k, int G, float lambda, int step, int beam_len,
                      int end_token, double* scores, const int32_t* hist_in, int32_t* hist_out, int32_t* src, int32_t* next_tok,
                      double* best_score, int32_t* best_len, int32_t* best_hist, const double* lp, hipStream_t stream) {
  VD_CHECK_ARG(top_idx && top_val && scores && hist_in && hist_out && src && next_tok && best_score && best_len && best_hist &&
               rounds >= 0 && hist_in != hist_out, "vd_beam_advance: bad args");
  VD_CHECK_ARG(k >= 1 && k <= VD_BEAM_KMAX, "vd_beam_advance: k = %d must be in [1, %d]", k, VD_BEAM_KMAX);
  VD_CHECK_ARG(G >= 1 && k % G == 0, "vd_beam_advance: G = %d must be >= 1 and divide k = %d", G, k);
  VD_CHECK_ARG(lambda >= 0.f && lambda < INFINITY, "vd_beam_advance: lambda = %g must be finite and >= 0", (double)lambda);
  VD_CHECK_ARG(step >= 1 && step < beam_len, "vd_beam_advance: step %d outside [1, %d)", step, beam_len);
  if (rounds == 0) return VD_OK;
  auto kern = G == 1 ? beam_advance_kernel<true> : beam_advance_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)rounds), dim3(256), 0, stream, top_idx, top_val, k, G, lambda, step, beam_len, end_token, scores,
                     hist_in, hist_out, src, next_tok, best_score, best_len, best_hist, lp);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

// vd_beam_topk under C1-C4 (rt_core.h): `hist` [rows x beam_len] is the PRE-advance history, `step` the step being taken
int vd_beam_topk_ban_p(const float* logits, int64_t ld, int64_t rows, int V, const int32_t* tok, int k, const int32_t* hist, int beam_len,
                       int step, int min_len, int no_repeat, int end_token, int32_t* top_idx, float* top_val, hipStream_t stream) {
  VD_CHECK_ARG(logits && tok && hist && top_idx && top_val && rows >= 0 && V >= 1 && ld >= V, "vd_beam_topk_ban: bad args");
  VD_CHECK_ARG(k >= 1 && k <= VD_BEAM_KMAX, "vd_beam_topk_ban: k = %d must be in [1, %d]", k, VD_BEAM_KMAX);
  VD_CHECK_ARG(step >= 1 && step < beam_len, "vd_beam_topk_ban: step %d outside [1, %d)", step, beam_len);
  VD_CHECK_ARG(min_len >= 0 && no_repeat >= 0 && end_token >= 1 && end_token <= V,
               "vd_beam_topk_ban: min_len = %d and no_repeat = %d must be >= 0 and end_token = %d in [1, V = %d]", min_len, no_repeat,
               end_token, V);
  VD_CHECK_ARG(no_repeat == 0 || beam_len <= VD_BEAM_LMAX, "vd_beam_topk_ban: beam_len = %d exceeds VD_BEAM_LMAX = %d with no_repeat = %d",
               beam_len, VD_BEAM_LMAX, no_repeat);
  VD_CHECK_ARG((long)V >= (long)k + beam_len - 1, "vd_beam_topk_ban: V = %d is below k + beam_len - 1 = %ld: a row could run out of unbanned words",
               V, (long)k + beam_len - 1);
  if (rows == 0) return VD_OK;
  if (k <= 8)
    hipLaunchKernelGGL(beam_topk_ban_kernel<8>, dim3((unsigned)rows), dim3(256), 0, stream, logits, (long)ld, V, tok, k, hist, beam_len,
                       step, min_len, no_repeat, end_token, top_idx, top_val);
  else
    hipLaunchKernelGGL(beam_topk_ban_kernel<VD_BEAM_KMAX>, dim3((unsigned)rows), dim3(256), 0, stream, logits, (long)ld, V, tok, k, hist,
                       beam_len, step, min_len, no_repeat, end_token, top_idx, top_val);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

extern "C" {

int vd_beam_topk(const float* logits, int64_t ld, int64_t rows, int V, const int32_t* tok, int k, int32_t* top_idx, float* top_val,
                 void* stream) {
  VD_CHECK_ARG(logits && tok && top_idx && top_val && rows >= 0 && V >= 1 && ld >= V, "vd_beam_topk: bad args");
  VD_CHECK_ARG(k >= 1 && k <= VD_BEAM_KMAX && k <= V, "vd_beam_topk: k = %d must be in [1, %d] and <= V = %d", k, VD_BEAM_KMAX, V);
  if (rows == 0) return VD_OK;
  if (k <= 8)
    hipLaunchKernelGGL(beam_topk_kernel<8>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, logits, (long)ld, V, tok, k,
                       top_idx, top_val);
  else
    hipLaunchKernelGGL(beam_topk_kernel<VD_BEAM_KMAX>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, logits, (long)ld, V,
                       tok, k, top_idx, top_val);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

int vd_beam_init(int groups, int k, int beam_len, int start_token, int32_t* hist, int32_t* tok, double* scores, double* best_score,
                 int32_t* best_len, void* stream) {
  VD_CHECK_ARG(hist && tok && scores && best_score && best_len && groups >= 0 && beam_len >= 1, "vd_beam_init: bad args");
  VD_CHECK_ARG(k >= 1 && k <= VD_BEAM_KMAX, "vd_beam_init: k = %d must be in [1, %d]", k, VD_BEAM_KMAX);
  if (groups == 0) return VD_OK;
  const long n = (long)groups * k * beam_len;
  hipLaunchKernelGGL(beam_init_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, groups, k, beam_len, start_token, hist,
                     tok, scores, best_score, best_len);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

int vd_beam_advance(const int32_t* top_idx, const float* top_val, int groups, int k, int step, int beam_len, int end_token,
                    double* scores, const int32_t* hist_in, int32_t* hist_out, int32_t* src, int32_t* next_tok, double* best_score,
                    int32_t* best_len, int32_t* best_hist, void* stream) {
  return vd_beam_advance_p(top_idx, top_val, groups, k, 1, 0.f, step, beam_len, end_token, scores, hist_in, hist_out, src, next_tok,
                           best_score, best_len, best_hist, nullptr, (hipStream_t)stream);
}

int vd_beam_select_rows(float* cur, const float* stepped, const int32_t* src, int64_t rows, int k, int H, void* stream) {
  VD_CHECK_ARG(cur && stepped && src && rows >= 0 && H >= 1 && cur != stepped, "vd_beam_select_rows: bad args");
  VD_CHECK_ARG(k >= 1 && rows % k == 0, "vd_beam_select_rows: %lld rows are not whole groups of k = %d", (long long)rows, k);
  if (rows == 0) return VD_OK;
  hipLaunchKernelGGL(beam_select_rows_kernel, dim3(grid_for(rows * H)), dim3(256), 0, (hipStream_t)stream, cur, stepped, src,
                     (long)rows, k, H);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

int vd_beam_finish(int groups, int k, int beam_len, const int32_t* hist, const double* scores, const double* best_score,
                   const int32_t* best_len, const int32_t* best_hist, int32_t* out_tokens, double* out_scores, void* stream) {
  VD_CHECK_ARG(hist && scores && best_score && best_len && best_hist && out_tokens && out_scores && groups >= 0 && k >= 1 &&
               beam_len >= 1, "vd_beam_finish: bad args");
  if (groups == 0) return VD_OK;
  const long n = (long)groups * beam_len;
  hipLaunchKernelGGL(beam_finish_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, groups, k, beam_len, hist, scores,
                     best_score, best_len, best_hist, out_tokens, out_scores);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

}  // extern "C"
