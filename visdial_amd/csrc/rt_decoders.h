// Native step runtime, part 3: the decoder plug-ins (reference decoders/disc.lua, decoders/gen.lua) and the two
// branches of Model:forwardBackward / Model:retrieveBatch they select (model.lua:306-338, 344-430).  Mirrors
// visdial_amd/decoders/disc.py, gen.py and visdial_amd/model.py.  Included by runtime.hip only.
#pragma once
#include "rt_encoders.h"

namespace vdrt {

int option_cache_resolve(vd_model* m, BatchSlot& sl, const int32_t* options, long NO, int To, hipStream_t s);   // runtime.hip

struct Decoder {
  virtual ~Decoder() {}
  virtual void declare(vd_model* m) = 0;
  // Model:forwardBackward on slot b: encoder + decoder forward, criterion, and (unless only_forward) both backwards
  virtual int forward_backward(vd_model* m, BatchSlot& b, bool only_forward) = 0;
  // Model:retrieveBatch up to the scores: leaves [N x O] option scores in m->scores
  virtual int retrieve(vd_model* m, BatchSlot& b) = 0;
  // the same through the live-row log-likelihood head (vd_model_retrieve_lhood); generative decoder only
  virtual int retrieve_lhood(vd_model*, BatchSlot&) {
    vd_set_error("vd_model_retrieve_lhood: the live-row log-likelihood head scores candidates of decoder 'gen'; this model's decoder is 'disc'");
    return VD_ERR_ARG;
  }
  // Model:generateAnswers device steps (model.lua:432-613); generative decoder only
  virtual int gen_begin(vd_model*, const int32_t*, int) { return no_gen(); }
  virtual int gen_step(vd_model*, const int32_t*, float*) { return no_gen(); }
  virtual int gen_select(vd_model*, const int32_t*, int) { return no_gen(); }
  virtual int gen_beam_search(vd_model*, int, int, int, int, int32_t*, double*) { return no_gen(); }
  virtual int gen_sample(vd_model*, int, int, int, double, const double*, int32_t*, double*) { return no_gen(); }
  static int no_gen() {
    vd_set_error("sampling / beam search only for the generative decoder (model.lua:436-438)");
    return VD_ERR_STATE;
  }
};

inline int stage_loss(vd_model* m, const float* loss_rows, long n, bool is_sum, hipStream_t s) {
  if (m->loss_cap < n) {
    if (m->loss_host) VD_HIP(hipHostFree(m->loss_host));
    m->loss_host = nullptr;
    VD_HIP(hipHostMalloc((void**)&m->loss_host, (size_t)n * sizeof(float), hipHostMallocDefault));
    m->loss_cap = n;
  }
  m->loss_n = n;
  m->loss_is_sum = is_sum;
  m->loss_div = 0.0;
  VD_HIP(hipMemcpyAsync(m->loss_host, loss_rows, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
  VD_HIP(hipEventRecord(m->ev_loss, s));
  return VD_OK;
}

// What the two rollout drivers (Disc::retrieve_rollout, Gen_beam_search) share.  VD_ROLLOUT_ENCODER = round is refused in training mode:
inline int refuse_round_rollout_in_training(vd_model* m, const char* call) {
  if (!(m->training && m->sw.rollout_round)) return VD_OK;
  vd_set_error("%s: this model was created with VD_ROLLOUT_ENCODER = round, which encodes a rollout's later passes one round at a time on the "
               "state of the first: under training-mode dropout the passes would not describe one model; call vd_model_set_training(0) first",
               call);
  return VD_ERR_STATE;
}
// the encoder of a pass r >= 1: round r of every dialog alone, or all N rounds again
inline int rollout_encode(vd_model* m, hipStream_t s, BatchSlot& b, int r, float** enc_out) {
  return m->sw.rollout_round ? m->enc->forward_round(m, s, b, r, enc_out) : m->enc->forward(m, s, b, enc_out);
}
// the history the append / pick kernels write: the uploaded rows and, where the upload sorted them by length, the sorted copy and its index
struct HistRows {
  int32_t *tok, *tok_sorted, *inv;
  explicit HistRows(BatchSlot& b) : tok(b.h.tok), tok_sorted(b.h.sorted ? b.h.tok_sorted : nullptr), inv(b.h.sorted ? b.h.inv : nullptr) {}
};

// ------------------------------------------------------------------------------------------------------------
// Discriminative decoder (decoders/disc.lua:3-38): the 100 candidate answers of a round share one embedding and one
// LSTM; option scores = <last hidden state, encoder output>; criterion = CrossEntropy over the options.
//   * 100 clones under nn.Concat(2) -> ONE recurrence over N*O rows
//   * LookupTable + Wx*x + b -> a [V+1 x 4H] table gathered by token id inside the step kernel
//   * nn.MM + CrossEntropyCriterion (+ their backward) -> vd_score_ce
// The option LSTM (a handful of big launches) runs on the main stream, the encoder (~200 small ones) beside it.
// ------------------------------------------------------------------------------------------------------------
#ifdef VD_PROBE_PHASES
inline hipEvent_t* probe_events() {
  static hipEvent_t e[6];
  static bool made = false;
  if (!made) { for (auto& x : e) (void)hipEventCreate(&x); made = true; }
  return e;
}
#define VD_PROBE_REC(i, stream) (void)hipEventRecord(probe_events()[i], stream)
#else
#define VD_PROBE_REC(i, stream)
#endif
struct Disc : Decoder {
  void declare(vd_model* m) override { add_lstm(m, "opt", m->p.embedSize, m->p.rnnHiddenSize); }
  // The candidates' final states, on the main stream: the projection table, then ONE recurrence over the NO rows the upload kept (N * O, or
  // the distinct candidates).  They depend on the option tokens and the weights only (decoders/disc.lua:4-15).  `opt` is the token set it
  // runs: b.opt, or b.opt_live in a live dense step (loss.hip DL3).
  struct OptStates {
    bool c16;                 // bf16 pass at a throughput shape: COMPACT state (common.h)
    float *table, *gates, *h, *c, *h_last;
    vd_bf16_bits *gates16, *h16;
    const float* optH;        // [NO x H]
  };
  int option_states(vd_model* m, const SeqTok& opt, OptStates* o) {
    const int NO = opt.N, To = opt.T;
    const long H = m->p.rnnHiddenSize, E = m->p.embedSize, V = m->p.vocabSize;
    hipStream_t s = m->s_main;
    VD_TRY(ws_get(m, "opt.table", (size_t)(V + 1) * 4 * H, &o->table));
    VD_TRY(ws_get(m, "opt.gates", (size_t)To * NO * 4 * H, &o->gates));
    VD_TRY(ws_get(m, "opt.h", (size_t)To * NO * H, &o->h));
    VD_TRY(ws_get(m, "opt.c", (size_t)To * NO * H, &o->c));
    float* Wopt = Wp(m, "opt.W");
    const int flags = m->flags;
    VD_TRY(vd_gemm_nn(Wp(m, "embed"), E, Wopt, 4 * H, Wp(m, "opt.b"), o->table, 4 * H, (int)V + 1, (int)(4 * H), (int)E, 0, s));
    // bf16 pass at a throughput shape: COMPACT state (common.h) -- gates / da only as bf16 (in the first half of `gates`), the
    // projection table as bf16 rows, h as bf16 plus the last step's fp32 state; c stays fp32
    o->c16 = (flags & VD_FLAG_BF16) && vd_lstm_c16_fits(NO, (int)H);
    o->gates16 = reinterpret_cast<vd_bf16_bits*>(o->gates);
    o->h16 = reinterpret_cast<vd_bf16_bits*>(o->h);
    o->h_last = nullptr;
    vd_bf16_bits* table16 = nullptr;
    if (o->c16) {
      float* t16;
      VD_TRY(ws_get(m, "opt.table16", (size_t)(V + 1) * 2 * H, &t16));
      VD_TRY(ws_get(m, "opt.h_last", (size_t)NO * H, &o->h_last));
      table16 = reinterpret_cast<vd_bf16_bits*>(t16);
      VD_TRY(vd_f32_to_bf16(o->table, table16, (V + 1) * 4 * H, s));
    }
    VD_HIP(hipEventRecord(m->ev_prof[0], s));
    {
      VdRange r("disc: option LSTM forward");
      if (o->c16) VD_TRY(vd_lstm_forward_c16(table16, 4 * H, opt.tok, Wopt + E * 4 * H, o->gates16, o->h16, o->h_last, o->c, To, NO, (int)H, s));
      else VD_TRY(vd_lstm_forward(o->table, 0, 4 * H, opt.tok, nullptr, Wopt + E * 4 * H, nullptr, nullptr, o->gates, o->h, o->c, To, NO, (int)H, flags, s));
    }
    VD_HIP(hipEventRecord(m->ev_prof[1], s));
    o->optH = o->c16 ? o->h_last : o->h + (long)(To - 1) * NO * H;
    return VD_OK;
  }
  // the state of every candidate (n, o), [N * O x H]: after a de-duplicating upload candidate (n, o) reads the state of its distinct row
  int option_states_full(vd_model* m, BatchSlot& b, const OptStates& o, const float** optH) {
    *optH = o.optH;
    if (!b.opt_uid) return VD_OK;
    const long NOfull = (long)b.q.N * m->p.numOptions, H = m->p.rnnHiddenSize;
    float* full;
    VD_TRY(ws_get(m, "opt.h_full", (size_t)NOfull * H, &full));
    VD_TRY(vd_embed_gather(o.optH, b.opt_uid, nullptr, full, NOfull, (int)H, 1.f, m->s_main));
    *optH = full;
    return VD_OK;
  }
  int forward_backward(vd_model* m, BatchSlot& b, bool only_forward) override {
    VD_CHECK_ARG(b.opt.present, "decoder 'disc' needs batch.options");
    VD_CHECK_ARG(only_forward || b.has_gt, "training decoder 'disc' needs batch.answer_ind");
    if (b.cached) return forward_cached(m, b, only_forward);
    const bool dense = !only_forward && b.rel != nullptr;   // loss.hip DT5
    VD_CHECK_ARG(!dense || m->sw.label_smoothing == 0.0,
                 "vd_model_forward_backward: the batch carries '@dense_relevance' and this model was created with VD_LABEL_SMOOTHING = %g: a "
                 "dense target is not smoothed; create the model without it", m->sw.label_smoothing);
    VD_CHECK_ARG(!dense || b.rel_W > 0.0,
                 "vd_model_forward_backward: the batch's '@dense_relevance' gives every round the weight 0 (W = 0, VD_DENSE_MIX = %g): no "
                 "annotated round has a relevant candidate and rounds without an annotation weigh VD_DENSE_MIX", m->sw.dense_mix);
    // DL3: the batch carries '@dense_relevance_live' and some rounds do not train: the candidate rows of the live rounds only, which the
    // attachment compacted (opt_uid resolved there: no gather, no scatter-add)
    const bool live = dense && b.n_live > 0;
    const SeqTok& opt = live ? b.opt_live : b.opt;
    // NO = rows the option LSTM executes: N * O, the number of DISTINCT candidates when the upload de-duplicated them, or n_live * O
    const int N = b.q.N, O = m->p.numOptions, NOfull = N * O, NO = opt.N, To = opt.T;
    const bool dedup = !live && b.opt_uid != nullptr;
    VD_CHECK_ARG(live ? NO == b.n_live * O : dedup ? NO <= NOfull : NO == NOfull, "decoder 'disc': %d option rows for %d x %d candidates", NO, N, O);
    const long H = m->p.rnnHiddenSize, E = m->p.embedSize, V = m->p.vocabSize;
    hipStream_t s = m->s_main;
    hipStream_t sd = side_stream(m, s);   // encoder, then the table-gradient chain, in this function's enqueue order
    float *scores, *loss_rows;
    VD_TRY(ws_get(m, "opt.scores", (size_t)N * O, &scores));
    VD_TRY(ws_get(m, "crit.loss_rows", (size_t)N, &loss_rows));
    float* Wopt = Wp(m, "opt.W");
    const int flags = m->flags;
    VD_TRY(fork_stream(m, s, sd));
    float* enc_out = nullptr;
    OptStates os;
    VD_TRY(option_states(m, opt, &os));
    const bool c16 = os.c16;
    float *gates = os.gates, *h = os.h, *c = os.c;
    vd_bf16_bits *gates16 = os.gates16, *h16 = os.h16;
    {
      VdRange r("encoder forward");
      VD_TRY(m->enc->forward(m, sd, b, &enc_out));                                 // model.lua:297
      VD_PROBE_REC(0, sd);
    }
    VD_TRY(join_stream(m, sd, s));
    // criterion (+ nn.MM backward) in one kernel (model.lua:330-335)
    const float* optH = os.optH;
    if (!live) VD_TRY(option_states_full(m, b, os, &optH));
    float *d_optH = nullptr, *d_enc = nullptr, *d_optH_full = nullptr;
    if (!only_forward) {
      VD_TRY(ws_get(m, "crit.d_optH", (size_t)NO * H, &d_optH));
      VD_TRY(ws_get(m, "crit.d_enc", (size_t)N * H, &d_enc));
      if (dedup) VD_TRY(ws_get(m, "crit.d_optH_full", (size_t)NOfull * H, &d_optH_full));
    }
    // a training step's targets are smoothed by VD_LABEL_SMOOTHING (loss.hip LS1, LS3); 0 is vd_score_ce itself.  A batch that carries
    // "@dense_relevance" trains on DT3's targets instead (DT4: gscale = 1 / W)
    if (live)
      VD_TRY(vd_score_ce_dense_live_p(optH, enc_out, b.gt, b.rel, b.live_slot, scores, loss_rows, d_optH, d_enc, N, O, (int)H,
                                      (float)(1.0 / b.rel_W), (float)m->sw.dense_mix, s));
    else if (dense)
      VD_TRY(vd_score_ce_dense_p(optH, enc_out, b.gt, b.rel, scores, loss_rows, dedup ? d_optH_full : d_optH, d_enc, N, O, (int)H,
                                 (float)(1.0 / b.rel_W), (float)m->sw.dense_mix, s));
    else
      VD_TRY(vd_score_ce_p(optH, enc_out, b.gt, scores, loss_rows, dedup ? d_optH_full : d_optH, d_enc, N, O, (int)H, 1.0f / N,
                           only_forward ? 0.f : (float)m->sw.label_smoothing, s));
    if (dedup && !only_forward) {   // the gradients of the copies of a distinct row add up
      VD_TRY(vd_memset(d_optH, 0, (long)NO * H * 4, s));
      VD_TRY(vd_embed_scatter_acc(d_optH, b.opt_uid, nullptr, d_optH_full, NOfull, (int)H, 1.f, s));
    }
    VD_TRY(stage_loss(m, loss_rows, N, false, s));
    if (dense) m->loss_div = b.rel_W;
    m->step_live = live;
    m->scores = scores;
    m->prof_valid = !only_forward;
    if (only_forward) return VD_OK;
    // decoder backward on the main stream, encoder backward beside it (model.lua:335-337)
    VD_TRY(fork_stream(m, s, sd));
    float *dc, *dtab;
    int32_t* perm = live ? b.live_sort_perm : b.opt_sort_perm;   // sorted at upload / attach time (runtime.hip)
    VD_TRY(ws_get(m, "opt.dc", (size_t)NO * H, &dc));
    VD_TRY(ws_get(m, "opt.dtable", (size_t)(V + 1) * 4 * H, &dtab));
    VD_CHECK_ARG(perm, "decoder 'disc': the batch slot carries no option-token sort");
    VD_TRY(vd_memset(dtab, 0, (V + 1) * 4 * H * 4, sd));
    VD_HIP(hipEventRecord(m->ev_prof[2], s));
    // off-chain parameter-gradient work of the encoder on its own (middle-priority) stream = its own hardware queue in a bf16 pass
    // (the encoder chain is that step's critical path: 12.34 -> 12.02 ms, profiles/r03_experiments.txt section 21); in fp32 the step
    // is work-conserving on the matrix pipe and it stays on the side lane.  Never joined into `sd`: a wait there would be a
    // barrier packet in front of the table-gradient chain.
    m->wg_active = m->streams && m->s_wg && (flags & VD_FLAG_BF16) != 0;
    m->wg_used = false;
    auto enc_bwd = [&]() -> int {
      VdRange r("encoder backward");
      m->wgrad_hold = true;      // the grouped weight-gradient launch is flushed below, behind the option recurrence's fork
      const int rc = m->enc->backward(m, sd, b, d_enc);
      m->wgrad_hold = false;
      VD_TRY(rc);
      VD_PROBE_REC(1, sd);
      if (m->wg_used) VD_PROBE_REC(2, m->s_wg);
      if (m->wg_used) {   // encoder tensors final = the chain on `sd` AND the gradient work on s_wg
        VD_TRY(fork_stream(m, sd, m->s_wg));
        VD_HIP(hipEventRecord(m->ev_enc_grads, m->s_wg));
      } else {
        VD_HIP(hipEventRecord(m->ev_enc_grads, sd));                                // encoder tensors final (data-parallel bucket 1)
      }
      m->enc_grads_recorded = true;
      return VD_OK;
    };
    {
      VdRange r("disc: option LSTM backward");
      if (c16) VD_TRY(vd_lstm_backward_c16(Wopt + E * 4 * H, gates16, c, d_optH, dc, To, NO, (int)H, s));
      else VD_TRY(vd_lstm_backward(Wopt + E * 4 * H, gates, c, nullptr, nullptr, d_optH, nullptr, dc, nullptr, nullptr, nullptr, To, NO, (int)H, flags, s));
    }
    VD_HIP(hipEventRecord(m->ev_prof[3], s));
    VD_TRY(enc_bwd());       // enqueued behind the option recurrence: it runs beside it on the side lane
    // table gradient + its consumers beside the dWh contraction.  This fork stays BEHIND the encoder backward's enqueue: the lane runs
    // in order, so the HBM-bound row sum starts when the encoder chain has drained, not with the MFMA-bound dWh contraction, where it
    // takes 2.9 ms instead of 0.7 and dWh 6.9 instead of 6.1 (profiles/r03_experiments.txt section 9)
    VdRange rwg("disc: table gradient + dWh");
    VD_TRY(fork_stream(m, s, sd));
    // the encoder LSTMs' held-back weight gradients (wgrad_hold above), one launch: behind this fork it runs beside the dWh contraction
    // instead of beside the last option-backward launches, which all have every workgroup resident and stretch with whatever shares their
    // CUs (profiles/enc_wgrad_group.txt section 2: parent 22.30 ms, flushed at the end of the encoder backward 22.26, here 21.96).  A group exists only outside a
    // bf16 pass, so the encoder's tensors are final on `sd` alone
    if (!m->wgrad.empty()) {
      VD_TRY(wgrad_flush(m, b, sd));
      VD_HIP(hipEventRecord(m->ev_enc_grads, sd));
    }
    if (c16) VD_TRY(vd_segment_rowsum_acc_bf16(gates16, 4 * H, opt.tok, perm, (long)To * NO, (int)(4 * H), dtab, 4 * H, sd));
    else VD_TRY(vd_segment_rowsum_acc(gates, 4 * H, opt.tok, perm, (long)To * NO, (int)(4 * H), dtab, 4 * H, sd));
    VD_TRY(vd_colsum_acc(dtab, 4 * H, (int)V + 1, (int)(4 * H), Gp(m, "opt.b"), sd));
    VD_TRY(vd_gemm_tn_acc(Wp(m, "embed"), E, dtab, 4 * H, Gp(m, "opt.W"), 4 * H, (int)E, (int)(4 * H), (int)V + 1, 0, sd));
    VD_HIP(hipEventRecord(m->ev_prof[4], s));
    if (To > 1 && c16)
      VD_TRY(vd_gemm_tn_acc_bf16(h16, gates16 + (long)NO * 4 * H, Gp(m, "opt.W") + E * 4 * H, 4 * H, (int)H, (int)(4 * H), (To - 1) * NO, s));
    else if (To > 1)
      VD_TRY(vd_gemm_tn_acc(h, H, gates + (long)NO * 4 * H, 4 * H, Gp(m, "opt.W") + E * 4 * H, 4 * H, (int)H, (int)(4 * H), (To - 1) * NO,
                            flags & (VD_FLAG_BF16 | VD_FLAG_SPLIT9), s));
    VD_HIP(hipEventRecord(m->ev_prof[5], s));
    // dEmb += dTable * Wx^T behind the table gradient on the side lane, with float atomics: the SHARED embedding gradient has concurrent atomic
    // writers (the encoder's scatters), and the product is off the main stream's critical path this way
    VD_TRY(vd_gemm_nt(dtab, 4 * H, Wopt, 4 * H, nullptr, Gp(m, "embed"), E, (int)V + 1, (int)E, (int)(4 * H), VD_ACT_NONE, 2, sd));
    VD_PROBE_REC(3, sd);
    VD_TRY(join_stream(m, sd, s));         // encoder backward and table-gradient chain: one lane, one event
    if (m->wg_used) VD_TRY(join_stream(m, m->s_wg, s));
    m->wg_active = m->wg_used = false;
    VD_PROBE_REC(4, s);
    return VD_OK;
  }
  int retrieve(vd_model* m, BatchSlot& b) override {                                          // model.lua:421-425
    if (m->sw.retrieve_rollout && m->use_hist) return retrieve_rollout(m, b);   // (no history: nothing depends on an answer)
    return forward_backward(m, b, true);
  }

  // VD_RETRIEVE_ROLLOUT (beam.hip E1-E5): the candidates' states once, then R = maxQuesCount passes on the main stream: encoder forward
  // (pass 0's beside the option recurrence, as in the plain step), vd_score_ce over all N rounds, and -- not after the last -- the pick
  // kernel, which writes history row r + 1 of every dialog from the rank-1 candidate of its round r.  Nothing waits for the host between
  // passes.  The last pass IS the result for every round: rows <= r of a dialog are final after pass r and every encoder is causal.
  // VD_ROLLOUT_CONCAT_END (CH1-CH6): the pick kernel writes the concatenated row instead; the passes are the same.
  int retrieve_rollout(vd_model* m, BatchSlot& b) {
    VD_TRY(refuse_round_rollout_in_training(m, "vd_model_retrieve"));
    if (m->training) {
      vd_set_error("vd_model_retrieve: this model was created with VD_RETRIEVE_ROLLOUT = 1, and a rollout re-runs the encoder once per round: "
                   "under training-mode dropout the passes would not describe one model; call vd_model_set_training(0) first");
      return VD_ERR_STATE;
    }
    VD_CHECK_ARG(b.opt.present && !b.cached, "decoder 'disc' needs batch.options");
    const int N = b.q.N, O = m->p.numOptions, NOfull = N * O, NO = b.opt.N, R = m->p.maxQuesCount, B = N / R;
    const bool dedup = b.opt_uid != nullptr;
    VD_CHECK_ARG(dedup ? NO <= NOfull : NO == NOfull, "decoder 'disc': %d option rows for %d x %d candidates", NO, N, O);
    VD_CHECK_ARG(b.h.present && b.q.present && b.h.N == N && N == B * R && b.h.T >= b.q.T,
                 "vd_model_retrieve: VD_RETRIEVE_ROLLOUT = 1 needs the batch's history, Th >= Tq");
    const long H = m->p.rnnHiddenSize;
    hipStream_t s = m->s_main;
    hipStream_t sd = side_stream(m, s);
    float *scores, *loss_rows;
    VD_TRY(ws_get(m, "opt.scores", (size_t)N * O, &scores));
    VD_TRY(ws_get(m, "crit.loss_rows", (size_t)N, &loss_rows));
    VD_TRY(fork_stream(m, s, sd));
    OptStates os;
    VD_TRY(option_states(m, b.opt, &os));
    float* enc_out = nullptr;
    {
      VdRange r("encoder forward");
      VD_TRY(m->enc->forward(m, sd, b, &enc_out));
    }
    VD_TRY(join_stream(m, sd, s));
    const float* optH;
    VD_TRY(option_states_full(m, b, os, &optH));
    const HistRows hr(b);
    m->rollout_max_words = b.opt.T;
    for (int r = 0; r < R; ++r) {
      if (r > 0) {                                                            // E5: rows 0 .. r of every dialog are final now
        VdRange rr("encoder forward");
        VD_TRY(rollout_encode(m, s, b, r, &enc_out));
      }
      VD_TRY(vd_score_ce(optH, enc_out, b.gt, scores, loss_rows, nullptr, nullptr, N, O, (int)H, 1.0f / N, s));
      if (r + 1 < R)                                                          // E2 - E4: the pick becomes history row r + 1
        VD_TRY(vd_disc_rollout_pick_p(scores, O, b.opt.tok, NO, b.opt.T, b.opt_uid, b.q.tok, b.q.T, B, R, r, hr.tok, hr.tok_sorted, hr.inv,
                                      b.h.T, s, m->sw.rollout_concat_end));
    }
    VD_TRY(stage_loss(m, loss_rows, N, false, s));
    m->scores = scores;
    m->prof_valid = false;
    return VD_OK;
  }

  // Evaluation through the answer-encoding cache (OptionCache, rt_core.h): b.opt holds the rows the cache did not have at upload time
  // (possibly none) and b.opt_uid the table row of every candidate.  The state-only recurrence runs over those rows alone, their final h
  // goes to the table, and the scores read the table through one gather -- a batch of known answers launches no recurrence kernel.
  int forward_cached(vd_model* m, BatchSlot& b, bool only_forward) {
    if (!only_forward || m->training) {
      vd_set_error("decoder 'disc': this batch was uploaded for cached evaluation (VD_OPTION_CACHE with training off) and carries only the "
                   "candidate rows the cache did not hold; upload it again after vd_model_set_training(1) for a training step");
      return VD_ERR_STATE;
    }
    OptionCache& oc = m->ocache;
    const int N = b.q.N, O = m->p.numOptions, NOfull = N * O, To = b.opt.T;
    const long H = m->p.rnnHiddenSize, E = m->p.embedSize, V = m->p.vocabSize;
    hipStream_t s = m->s_main;
    hipStream_t sd = side_stream(m, s);
    if (b.cache_stamp != oc.stamp) {   // flushed or stepped since the upload: resolve again (the copy out of the staging buffers has to land first)
      VD_HIP(hipEventSynchronize(b.ready));
      VD_TRY(option_cache_resolve(m, b, b.opt_host.data(), NOfull, To, s));
      VD_HIP(hipStreamSynchronize(s));   // (the next upload into this slot waits for `ready` only before it rewrites the staging buffers)
    }
    const int U = b.opt.N;
    const long count = oc.index.size();
    VD_CHECK_ARG(b.opt_total == NOfull && (long)b.miss_keys.size() == (long)U * To && count <= oc.capacity,
                 "decoder 'disc': inconsistent cached batch (%d candidates, %d misses)", b.opt_total, U);
    if (oc.table_rows < count + U) {   // grow: doubling up to the capacity (+ this batch's rows beyond it)
      const long want = std::min(std::max(2 * oc.table_rows, VD_OPTION_CACHE_FIRST_ROWS), oc.capacity);
      const long rows = std::max(want, count + U);
      float* nt = nullptr;
      VD_HIP(hipMalloc((void**)&nt, (size_t)rows * H * sizeof(float)));
      if (oc.table) {
        if (count > 0) VD_HIP(hipMemcpyAsync(nt, oc.table, (size_t)count * H * sizeof(float), hipMemcpyDeviceToDevice, s));
        VD_HIP(hipStreamSynchronize(s));   // earlier steps' gathers read the old table
        VD_HIP(hipFree(oc.table));
      }
      oc.table = nt;
      oc.table_rows = rows;
    }
    float *scores, *loss_rows, *full;
    VD_TRY(ws_get(m, "opt.scores", (size_t)N * O, &scores));
    VD_TRY(ws_get(m, "crit.loss_rows", (size_t)N, &loss_rows));
    VD_TRY(ws_get(m, "opt.h_full", (size_t)NOfull * H, &full));
    VD_TRY(fork_stream(m, s, sd));
    if (U > 0) {
      VdRange r("disc: option LSTM forward (state only, cache misses)");
      float *table, *h, *c;
      VD_TRY(ws_get(m, "opt.table", (size_t)(V + 1) * 4 * H, &table));
      VD_TRY(ws_get(m, "opt.h2", (size_t)2 * U * H, &h));
      VD_TRY(ws_get(m, "opt.c2", (size_t)2 * U * H, &c));
      float* Wopt = Wp(m, "opt.W");
      VD_TRY(vd_gemm_nn(Wp(m, "embed"), E, Wopt, 4 * H, Wp(m, "opt.b"), table, 4 * H, (int)V + 1, (int)(4 * H), (int)E, 0, s));
      VD_TRY(vd_lstm_forward(table, 0, 4 * H, b.opt.tok, nullptr, Wopt + E * 4 * H, nullptr, nullptr, nullptr, h, c, To, U, (int)H,
                             m->flags | VD_FLAG_STATE_ONLY, s));
      VD_HIP(hipMemcpyAsync(oc.table + count * H, h + (long)((To - 1) & 1) * U * H, (size_t)U * H * sizeof(float), hipMemcpyDeviceToDevice, s));
      // the fill is enqueued: the rows that fit become entries (slot = count + i, the numbering the upload used)
      const long fit = std::min<long>(U, oc.capacity - count);
      for (long i = 0; i < fit; ++i) oc.index.add(b.miss_keys.data() + (size_t)i * To);
    }
    ++oc.stamp;   // this slot's resolution is spent: rows beyond the capacity live in the table's tail for this step only
    float* enc_out = nullptr;
    {
      VdRange r("encoder forward");
      VD_TRY(m->enc->forward(m, sd, b, &enc_out));
    }
    VD_TRY(join_stream(m, sd, s));
    VD_TRY(vd_embed_gather(oc.table, b.opt_uid, nullptr, full, NOfull, (int)H, 1.f, s));
    VD_TRY(vd_score_ce(full, enc_out, b.gt, scores, loss_rows, nullptr, nullptr, N, O, (int)H, 1.0f / N, s));
    VD_TRY(stage_loss(m, loss_rows, N, false, s));
    m->scores = scores;
    m->prof_valid = false;
    return VD_OK;
  }
};

// ------------------------------------------------------------------------------------------------------------
// Generative decoder (decoders/gen.lua:3-68):
//   answer_in -> shared embedding -> numLayers x SeqLSTM(maskZero) -> Linear(H, V) -> LogSoftMax,
//   criterion = sum over non-pad steps of -log p(answer_out)            (model.lua:32-36, 306-324)
// The encoder's per-layer final (h, c) seed the decoder layers and the encoder output replaces the top layer's initial
// h (forwardConnect, gen.lua:30-42); backwardConnect hands the gradients w.r.t. those states back (gen.lua:45-60).
// ------------------------------------------------------------------------------------------------------------
struct Gen;
int Gen_begin(Gen* g, vd_model* m, const int32_t* rounds, int n);
int Gen_step(Gen* g, vd_model* m, const int32_t* tokens, float* host_logp);
int Gen_select(Gen* g, vd_model* m, const int32_t* src, int n_keep);
int Gen_beam_search(Gen* g, vd_model* m, int k, int L, int start, int end, int32_t* host_tokens, double* host_scores);
int Gen_sample(Gen* g, vd_model* m, int L, int start, int end, double T, const double* host_u, int32_t* host_tokens,
               double* host_loglik);

struct Gen : Decoder {
  int gen_begin(vd_model* m, const int32_t* r, int n) override { return Gen_begin(this, m, r, n); }
  int gen_step(vd_model* m, const int32_t* t, float* lp) override { return Gen_step(this, m, t, lp); }
  int gen_select(vd_model* m, const int32_t* src, int k) override { return Gen_select(this, m, src, k); }
  int gen_beam_search(vd_model* m, int k, int L, int st, int en, int32_t* t, double* sc) override {
    return Gen_beam_search(this, m, k, L, st, en, t, sc);
  }
  int gen_sample(vd_model* m, int L, int st, int en, double T, const double* u, int32_t* t, double* ll) override {
    return Gen_sample(this, m, L, st, en, T, u, t, ll);
  }
  std::vector<SeqLSTM> rnn;
  long E = 0, H = 0, V = 0, Vp = 0;
  int gen_n = 0;                                     // live hypotheses of the running generation
  void declare(vd_model* m) override {
    E = m->p.embedSize; H = m->p.rnnHiddenSize; V = m->p.vocabSize; Vp = (V + 3) / 4 * 4;
    rnn.resize(m->p.numLayers);
    for (int l = 0; l < m->p.numLayers; ++l) {
      add_lstm(m, "dec" + std::to_string(l + 1), l == 0 ? E : H, H);              // gen.lua:17-22
      rnn[l].init("dec" + std::to_string(l + 1), l == 0 ? E : H, H);
    }
    add_linear(m, "vocab", H, V);                                                   // gen.lua:23
  }
  // gen.lua:30-42; `rep` (retrieval) replicates every encoder state row over the chunk's options
  int forwardConnect(vd_model* m, hipStream_t s, const float* encOut, int seqLen, const int32_t* rep, long rows) {
    auto put = [&](const float* x, const std::string& key, const float** dst) -> int {
      if (!rep) {
        *dst = x;
        return VD_OK;
      }
      float* r;
      VD_TRY(ws_get(m, key, (size_t)rows * H, &r));
      VD_TRY(vd_embed_gather(x, rep, nullptr, r, rows, (int)H, 1.f, s));
      *dst = r;
      return VD_OK;
    };
    std::vector<SeqLSTM>* layers = m->enc->rnnLayers();
    if (layers) {
      for (size_t i = 0; i < layers->size(); ++i) {
        VD_TRY(put((*layers)[i].out_at(seqLen - 1), "ret.h0_" + std::to_string(i), &rnn[i].userPrevOutput));
        VD_TRY(put((*layers)[i].cell_at(seqLen - 1), "ret.c0_" + std::to_string(i), &rnn[i].userPrevCell));
      }
      return put(encOut, "ret.enc", &rnn[layers->size() - 1].userPrevOutput);
    }
    return put(encOut, "ret.enc", &rnn.back().userPrevOutput);
  }
  // gen.lua:45-60: returns dL/d encOut
  const float* backwardConnect(vd_model* m) {
    std::vector<SeqLSTM>* layers = m->enc->rnnLayers();
    if (layers) {
      const size_t n = rnn.size();
      for (size_t i = 0; i < n; ++i) {
        (*layers)[i].userNextGradCell = rnn[i].userGradPrevCell;
        if (i != n - 1) (*layers)[i].gradPrevOutput = rnn[i].userGradPrevOutput;
      }
      return rnn[layers->size() - 1].userGradPrevOutput;
    }
    return rnn.back().userGradPrevOutput;
  }
  int forward_backward(vd_model* m, BatchSlot& b, bool only_forward) override {
    VD_CHECK_ARG(b.ain.present && b.aout.present, "decoder 'gen' needs batch.answer_in / answer_out");
    VD_CHECK_ARG(only_forward || !b.rel,
                 "vd_model_forward_backward: the batch carries '@dense_relevance', which trains the option scores of decoder 'disc' (loss.hip "
                 "DT5); this model's decoder is 'gen', which reads the attachment for '@ndcg' only");
    hipStream_t s = m->s_main;
    const int N = b.q.N, Ta = b.ain.T;
    const long rows = (long)Ta * N;
    float* encOut;
    {
      VdRange r("encoder forward");
      VD_TRY(m->enc->forward(m, s, b, &encOut));                                    // model.lua:297
    }
    VdRange rdec("gen: decoder forward + criterion + backward");
    VD_TRY(forwardConnect(m, s, encOut, m->enc->seqLen(b), nullptr, N));            // model.lua:300
    float *x, *h, *logits, *loss_rows;
    VD_TRY(ws_get(m, "dec.x", (size_t)rows * E, &x));
    VD_TRY(ws_get(m, "dec.logits", (size_t)rows * Vp, &logits));
    VD_TRY(ws_get(m, "dec.loss_rows", (size_t)rows, &loss_rows));
    VD_TRY(vd_embed_gather(Wp(m, "embed"), b.ain.tok, nullptr, x, rows, (int)E, 1.f, s));
    VD_TRY(lstm_stack_forward(m, s, rnn, {x}, Ta, N, b.ain.tok, &h));
    m->prof_valid = false;
    m->prof_hist = false;
    VD_HIP(hipEventRecord(m->ev_prof[4], s));          // family 3 of a gen pair: vocabulary projection + criterion + their gradients
    VD_TRY(vd_gemm_nt(h, H, Wp(m, "vocab.W"), H, Wp(m, "vocab.b"), logits, Vp, (int)rows, (int)V, (int)H, VD_ACT_NONE, 0, s));
    // model.lua:309-311; a training step's targets are smoothed by VD_LABEL_SMOOTHING (loss.hip LS2, LS3); 0 is vd_logsoftmax_nll itself
    VD_TRY(vd_logsoftmax_nll_p(logits, Vp, rows, (int)V, b.ain.tok, b.aout.tok, loss_rows, only_forward ? 0 : 1,
                               only_forward ? 0.f : (float)m->sw.label_smoothing, s));
    VD_TRY(stage_loss(m, loss_rows, rows, true, s));
    if (only_forward) return VD_OK;
    float* dh;                                                                      // logits now hold d loss / d logits
    VD_TRY(ws_get(m, "dec.dh", (size_t)rows * H, &dh));
    VD_TRY(vd_gemm_tn_acc(logits, Vp, h, H, Gp(m, "vocab.W"), H, (int)V, (int)H, (int)rows, 0, s));
    VD_TRY(vd_colsum_acc(logits, Vp, (int)rows, (int)V, Gp(m, "vocab.b"), s));
    VD_TRY(vd_gemm_nn(logits, Vp, Wp(m, "vocab.W"), H, nullptr, dh, H, (int)rows, (int)H, (int)V, 0, s));
    VD_HIP(hipEventRecord(m->ev_prof[5], s));
    std::vector<float*> dx;
    VD_TRY(lstm_stack_backward(m, s, rnn, nullptr, dh, &dx));                       // model.lua:316
    VD_TRY(vd_embed_scatter_acc(Gp(m, "embed"), b.ain.tok, nullptr, dx[0], rows, (int)E, 1.f, s));
    const float* gradDecOut = backwardConnect(m);                                   // model.lua:319
    VD_CHECK_ARG(gradDecOut, "backwardConnect produced no gradient");
    {
      VdRange r("encoder backward");
      VD_TRY(m->enc->backward(m, s, b, gradDecOut));                                // model.lua:322
    }
    VD_HIP(hipEventRecord(m->ev_enc_grads, s));
    m->enc_grads_recorded = true;
    m->prof_valid = m->prof_hist;       // [history branch fwd, history branch bwd, vocabulary family] (vd_model_family_ms)
    return VD_OK;
  }
  // Model:retrieveBatch gen branch (model.lua:392-420) + utils.computeLhood (utils.lua:86-102).  The reference loops
  // over the 100 options; here chunks of options are ONE decoder batch (rows = round x option) seeded by the replicated
  // encoder state, and the [rows x V] logits only ever exist for one chunk (retrieve_dense).
  int retrieve(vd_model* m, BatchSlot& b) override {
    Retrieval r;
    VD_TRY(retrieve_begin(m, b, false, &r));
    VD_TRY(retrieve_dense(m, b, r));
    return retrieve_end(m, r);
  }
  // vd_model_retrieve_lhood: the same encoder forward; the head is csrc/lhood.hip's, with no logits buffer.  Where the chunk fits the
  // order kernels the candidates run in order of descending length (retrieve_ordered), else as they come (retrieve_live).
  // With VD_LHOOD_TREE (third mode): over a prefix tree of the candidates' tokens (retrieve_tree); a batch the tree was not built
  // for (a token behind a pad) takes the length-ordered path unchanged, and the counters then report that path
  int retrieve_lhood(vd_model* m, BatchSlot& b) override {
    Retrieval r;
    VD_TRY(retrieve_begin(m, b, true, &r));
    if (m->sw.lhood_tree && b.tree_ok) VD_TRY(retrieve_tree(m, b, r));
    else if (vd_lhood_prefix_fits(r.T, (long)r.N * std::min(r.O, r.oc))) VD_TRY(retrieve_ordered(m, b, r));
    else VD_TRY(retrieve_live(m, b, r));
    return retrieve_end(m, r);
  }

  // What every retrieval mode starts from: the encoder forward on the main stream, the [N x O] score buffer, the options per chunk, and
  // (log-likelihood head) the counters of vd_model_option_rows, which the mode adds its executed rows to.
  struct Retrieval {
    hipStream_t s;
    int N, O, T, seqLen, oc;
    float *encOut, *lhood;
  };
  int retrieve_begin(vd_model* m, BatchSlot& b, bool live, Retrieval* r) {
    VD_CHECK_ARG(b.oin.present && b.oout.present, "retrieval with decoder 'gen' needs batch.option_in / option_out");
    r->s = m->s_main;
    r->N = b.q.N; r->O = m->p.numOptions; r->T = b.oin.T;
    VD_TRY(m->enc->forward(m, r->s, b, &r->encOut));
    r->seqLen = m->enc->seqLen(b);
    VD_TRY(ws_get(m, "ret.lhood", (size_t)r->N * r->O, &r->lhood));
    // floats one option adds to a chunk's workspace.  Dense head: the [T*N x Vp] logits dominate, <= 4 GiB of them.  Live-row head:
    // what is still materialised is the decoder's input and saved state, (E + 6 H per layer: gates 4H, h, c) floats per (step, row),
    // held to the same 4 GiB -- and to the 32-bit row byte offsets of h in the fused kernel (T * rows * H * 4 < 4 GiB, implied).
    const long per_opt = (long)r->T * r->N * (live ? E + 6 * H * (long)rnn.size() : Vp);
    r->oc = (int)std::max<long>(1, std::min<long>(r->O, (1L << 30) / std::max<long>(1, per_opt)));
    if (live) {
      m->lhood_exec = 0;
      m->lhood_total = (long)r->T * r->N * r->O;
    }
    return VD_OK;
  }
  int retrieve_end(vd_model* m, const Retrieval& r) {
    m->scores = r.lhood;
    m->prof_valid = false;
    return VD_OK;
  }
  // layer 1's input projection of every token id, Emb * Wx + b, made once per retrieval (the ordered and the tree recurrence gather it)
  int retrieve_table(vd_model* m, hipStream_t s, float** table) {
    VD_TRY(ws_get(m, "ret.table", (size_t)(V + 1) * 4 * H, table));
    return vd_gemm_nn(Wp(m, "embed"), E, rnn[0].Wx(m), 4 * H, Wp(m, rnn[0].name + ".b"), *table, 4 * H, (int)V + 1, (int)(4 * H), (int)E, 0, s);
  }
  // options [o0, o0 + C) of the batch as one decoder batch: cin / cout [T x rows] = those columns of option_in / option_out
  // [T*N x O] (a strided dword copy), nll [T x rows] for the chunk's head
  struct Chunk {
    int o0, C;
    long rows;
    int32_t *cin, *cout;
    float* nll;
  };
  int retrieve_chunk(vd_model* m, BatchSlot& b, const Retrieval& r, int o0, Chunk* k) {
    k->o0 = o0;
    k->C = std::min(r.O, o0 + r.oc) - o0;
    k->rows = (long)r.N * k->C;
    VD_TRY(ws_get(m, "ret.cin", (size_t)r.T * k->rows, &k->cin));
    VD_TRY(ws_get(m, "ret.cout", (size_t)r.T * k->rows, &k->cout));
    VD_TRY(vd_copy_2d((float*)k->cin, k->C, (const float*)(b.oin.tok + o0), r.O, (long)r.T * r.N, k->C, r.s));
    VD_TRY(vd_copy_2d((float*)k->cout, k->C, (const float*)(b.oout.tok + o0), r.O, (long)r.T * r.N, k->C, r.s));
    return ws_get(m, "ret.nll", (size_t)r.T * k->rows, &k->nll);
  }
  // forwardConnect replication over the chunk in candidate order, the embedded tokens, the decoder stack over every (step, row)
  int retrieve_chunk_forward(vd_model* m, const Retrieval& r, const Chunk& k, float** h) {
    std::vector<int32_t> hidx(k.rows);
    for (long i = 0; i < k.rows; ++i) hidx[i] = (int32_t)(i / k.C);
    int32_t* idx;
    float* x;
    VD_TRY(index_array(m, "idx.ret." + std::to_string(k.rows) + "." + std::to_string(k.C), hidx, &idx));
    VD_TRY(forwardConnect(m, r.s, r.encOut, r.seqLen, idx, k.rows));
    VD_TRY(ws_get(m, "ret.x", (size_t)r.T * k.rows * E, &x));
    VD_TRY(vd_embed_gather(Wp(m, "embed"), k.cin, nullptr, x, r.T * k.rows, (int)E, 1.f, r.s));
    return lstm_stack_forward(m, r.s, rnn, {x}, r.T, (int)k.rows, k.cin, h);
  }
  // the live-row list of a chunk and the scratch of vd_lhood_live_rows
  int retrieve_act(vd_model* m, const Retrieval& r, const Chunk& k, int32_t** act, int32_t** work) {
    VD_TRY(ws_get(m, "ret.act", (size_t)r.T * k.rows, act));
    return ws_get(m, "ret.act_work", (size_t)(r.T * k.rows + 1023) / 1024 + 1, work);
  }

  // vocabulary projection of every (step, row) into logits + log-softmax NLL, summed over time
  int retrieve_dense(vd_model* m, BatchSlot& b, const Retrieval& r) {
    hipStream_t s = r.s;
    for (int o0 = 0; o0 < r.O; o0 += r.oc) {
      Chunk k;
      float *h, *logits, *acc;
      VD_TRY(retrieve_chunk(m, b, r, o0, &k));
      VD_TRY(retrieve_chunk_forward(m, r, k, &h));
      VD_TRY(ws_get(m, "ret.logits", (size_t)r.T * k.rows * Vp, &logits));
      VD_TRY(ws_get(m, "ret.acc", (size_t)k.rows, &acc));
      VD_TRY(vd_gemm_nt(h, H, Wp(m, "vocab.W"), H, Wp(m, "vocab.b"), logits, Vp, (int)(r.T * k.rows), (int)V, (int)H, VD_ACT_NONE, 0, s));
      VD_TRY(vd_logsoftmax_nll(logits, Vp, r.T * k.rows, (int)V, k.cin, k.cout, k.nll, 0, s));
      VD_TRY(vd_memset(acc, 0, k.rows * 4, s));
      VD_TRY(vd_colsum_acc(k.nll, k.rows, r.T, (int)k.rows, acc, s));                // sum over time (utils.lua:98)
      VD_TRY(vd_copy_2d(r.lhood + o0, r.O, acc, k.C, r.N, k.C, s));
    }
    return vd_axpby(r.lhood, nullptr, r.lhood, (long)r.N * r.O, -1.f, 0.f, s);       // log-likelihood = -NLL
  }
  // the same decoder pass; the head is vd_lhood_live_rows + vd_lhood_nll + vd_lhood_sum over the live rows of the chunk
  int retrieve_live(vd_model* m, BatchSlot& b, const Retrieval& r) {
    for (int o0 = 0; o0 < r.O; o0 += r.oc) {
      Chunk k;
      float* h;
      int32_t *act, *work, n_act = 0;
      VD_TRY(retrieve_chunk(m, b, r, o0, &k));
      VD_TRY(retrieve_chunk_forward(m, r, k, &h));
      VD_TRY(retrieve_act(m, r, k, &act, &work));
      VD_TRY(vd_lhood_live_rows(k.cin, k.cout, r.T * k.rows, act, work, &n_act, r.s));   // the chunk's one host synchronisation
      VD_TRY(vd_lhood_nll(h, H, r.T * k.rows, act, n_act, k.cout, Wp(m, "vocab.W"), H, Wp(m, "vocab.b"), (int)V, (int)H, k.nll, r.s));
      VD_TRY(vd_lhood_sum(k.nll, act, n_act, r.T, k.rows, k.C, r.lhood + o0, r.O, r.s));   // log-likelihood = -NLL, summed over time
      m->lhood_exec += (long)r.T * k.rows;
    }
    return VD_OK;
  }
  // The chunk's candidates go through the decoder in order of descending length (lhood_order_*, csrc/lhood.hip), so that the live rows
  // of every step are a prefix of the rows and the recurrence can skip the rest (VD_FLAG_LIVE_PREFIX).  Layer 1 then reads its input
  // projection from the table by token id; vd_lhood_sum_p scatters the scores back to candidate order.
  int retrieve_ordered(vd_model* m, BatchSlot& b, const Retrieval& r) {
    hipStream_t s = r.s;
    const int T = r.T;
    float* table;
    VD_TRY(retrieve_table(m, s, &table));
    for (int o0 = 0; o0 < r.O; o0 += r.oc) {
      Chunk k;
      VD_TRY(retrieve_chunk(m, b, r, o0, &k));
      const long rows = k.rows;
      int32_t *perm, *rep, *cin_s, *cout_s, *owork, *info, *act, *work, n_act = 0;
      void* info_host;
      VD_TRY(ws_get(m, "ret.perm", (size_t)rows, &perm));
      VD_TRY(ws_get(m, "ret.rep", (size_t)rows, &rep));
      VD_TRY(ws_get(m, "ret.cin_s", (size_t)T * rows, &cin_s));
      VD_TRY(ws_get(m, "ret.cout_s", (size_t)T * rows, &cout_s));
      VD_TRY(ws_get(m, "ret.order_work", (size_t)vd_lhood_order_work_ints(T, rows), &owork));
      VD_TRY(ws_get(m, "ret.order_info", (size_t)T + 1, &info));
      VD_TRY(pin_get(b.pinned, "ret.order_info", ((size_t)T + 1) * sizeof(int32_t), &info_host));
      VD_TRY(retrieve_act(m, r, k, &act, &work));
      VD_TRY(vd_lhood_order_p(k.cin, k.cout, T, rows, k.C, perm, rep, cin_s, cout_s, owork, info, s));
      VD_HIP(hipMemcpyAsync(info_host, info, ((size_t)T + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
      // the chunk's one host synchronisation, in front of the recurrence (it depends on the tokens only): the live-row count, and
      // with it the order's status word and per-step counts
      VD_TRY(vd_lhood_live_rows(cin_s, cout_s, T * rows, act, work, &n_act, s));
      const int32_t* hinfo = static_cast<const int32_t*>(info_host);
      // a candidate that is not one left-aligned run: no prefix promise -- the chunk runs every row, as without the order
      const int flags = hinfo[0] ? 0 : VD_FLAG_LIVE_PREFIX;
      int Tl = T;   // steps behind the longest candidate hold no token at all: not launched
      long ran = (long)T * rows;
      if (flags) {
        const long tile = vd_lstm_fwd_row_tile(rows);
        Tl = 1;
        ran = 0;
        for (int t = 0; t < T; ++t) {
          if (hinfo[1 + t] > 0) Tl = t + 1;
          ran += std::min<long>(rows, (hinfo[1 + t] + tile - 1) / tile * tile);
        }
      }
      m->lhood_exec += ran;
      float* h;
      VD_TRY(forwardConnect(m, s, r.encOut, r.seqLen, rep, rows));
      VD_TRY(rnn[0].forward_only(m, s, table, nullptr, Tl, (int)rows, cin_s, flags, (int)rows, true, &h));
      for (size_t l = 1; l < rnn.size(); ++l) VD_TRY(rnn[l].forward_only(m, s, nullptr, h, Tl, (int)rows, cin_s, flags, (int)rows, true, &h));
      VD_TRY(vd_lhood_nll(h, H, Tl * rows, act, n_act, cout_s,   // (every live row lies in the Tl steps that ran)
                           Wp(m, "vocab.W"), H, Wp(m, "vocab.b"), (int)V, (int)H, k.nll, s));
      VD_TRY(vd_lhood_sum_p(k.nll, act, n_act, T, rows, k.C, perm, r.lhood + o0, r.O, s));   // log-likelihood = -NLL, summed over time
    }
    return VD_OK;
  }
  // The decoder state after a candidate's first t tokens depends on the round's encoder state and on those tokens only, so the chunk's
  // candidates run as a forest: one node per distinct (round, token prefix), levels packed densely (no pad rows, no length order), the
  // depth-0 parents are the rounds' rows of the encoder state (no forwardConnect replication).  The head runs once per NODE
  // (vd_lhood_lse_p: the log-sum-exp belongs to the prefix), and a candidate's score is the sum over its edges of target logit - lse
  // (vd_lhood_edge_sum_p), written straight into candidate order.  The host built every list at upload time (runtime.hip
  // build_lhood_tree): the step needs no host synchronisation.
  int retrieve_tree(vd_model* m, BatchSlot& b, const Retrieval& r) {
    hipStream_t s = r.s;
    const int N = r.N;
    float* table;
    VD_TRY(retrieve_table(m, s, &table));
    for (const TreeChunk& tc : b.tree) {
      const long rows = (long)N * tc.C;
      const long tile = vd_lstm_fwd_row_tile(tc.Nw);
      for (int t = 0; t < tc.Tl; ++t) m->lhood_exec += std::min<long>(tc.Nw, (tc.widths[t] + tile - 1) / tile * tile);
      float *h = nullptr, *lse;
      VD_TRY(ws_get(m, "ret.lse", (size_t)std::max<long>(1, tc.n_nodes), &lse));
      if (tc.Tl > 0) {
        VD_TRY(forwardConnect(m, s, r.encOut, r.seqLen, nullptr, N));
        VD_TRY(rnn[0].forward_only(m, s, table, nullptr, tc.Tl, tc.Nw, tc.mask2, VD_FLAG_TREE, N, false, &h));
        for (size_t l = 1; l < rnn.size(); ++l) VD_TRY(rnn[l].forward_only(m, s, nullptr, h, tc.Tl, tc.Nw, tc.mask2, VD_FLAG_TREE, N, false, &h));
        VD_TRY(vd_lhood_lse_p(h, H, (long)tc.Tl * tc.Nw, tc.node_row, tc.n_nodes, Wp(m, "vocab.W"), H, Wp(m, "vocab.b"), (int)V, (int)H, lse, s));
      }
      VD_TRY(vd_lhood_edge_sum_p(h, H, tc.node_row, lse, tc.enode, tc.etgt, tc.Tl, rows, tc.C, Wp(m, "vocab.W"), H, Wp(m, "vocab.b"), (int)H,
                                 r.lhood + tc.o0, r.O, s));
    }
    return VD_OK;
  }
};

// ---- Model:generateAnswers (model.lua:432-613): the device side of sampling / beam search.  The host keeps the
// candidate bookkeeping (as the reference does in Lua); one call = one decoder step for all live hypotheses.
inline int gen_rows(vd_model* m, const char* key, const int32_t* host, int n, int32_t** out) {
  VD_TRY(ws_get(m, key, (size_t)std::max(n, 1), out));
  VD_HIP(hipMemcpyAsync(*out, host, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, m->s_main));
  VD_HIP(hipStreamSynchronize(m->s_main));           // `host` may be a temporary of the caller
  return VD_OK;
}
// Layer l's state of the n hypotheses, [n x H] each: the current state a step starts from (gen.h<l> / gen.c<l>) and the stepped
// state vd_model_decode_step keeps for vd_model_decode_select (gen.hn<l> / gen.cn<l>).
struct GenState {
  float *h, *c, *hn, *cn;
};
inline int gen_state(Gen* g, vd_model* m, size_t l, int n, GenState* st) {
  const std::string sfx = std::to_string(l);
  const size_t count = (size_t)n * g->H;
  VD_TRY(ws_get(m, "gen.h" + sfx, count, &st->h));
  VD_TRY(ws_get(m, "gen.c" + sfx, count, &st->c));
  VD_TRY(ws_get(m, "gen.hn" + sfx, count, &st->hn));
  VD_TRY(ws_get(m, "gen.cn" + sfx, count, &st->cn));
  return VD_OK;
}
// decoderConnect (gen.lua:63-68): the stepped state rnn[l].out_at(0) / cell_at(0) of the n hypotheses goes to the current state
// (`next`: to the stepped buffers hn / cn).  With `src` (beam search), row r takes stepped row group(r) * k + src[r] and a row
// with src[r] < 0 is left alone (vd_beam_select_rows); without, every row is copied.
inline int gen_carry(Gen* g, vd_model* m, int n, bool next, const int32_t* src = nullptr, int k = 1) {
  hipStream_t s = m->s_main;
  const long H = g->H;
  for (size_t l = 0; l < g->rnn.size(); ++l) {
    GenState st;
    VD_TRY(gen_state(g, m, l, n, &st));
    float* dst[2] = {next ? st.hn : st.h, next ? st.cn : st.c};
    const float* stepped[2] = {g->rnn[l].out_at(0), g->rnn[l].cell_at(0)};
    for (int i = 0; i < 2; ++i) {
      if (src) VD_TRY(vd_beam_select_rows(dst[i], stepped[i], src, n, k, (int)H, s));
      else VD_TRY(vd_memcpy_d2d(dst[i], stepped[i], (long)n * H * 4, s));
    }
  }
  return VD_OK;
}
// hiddenBeams (model.lua:478-503): hypothesis i starts from the encoder state of QA round rounds[i]
// (gen_begin_rows: the same from round indices that are on the device already -- a rollout's passes, which must not wait for the host)
inline int gen_begin_rows(Gen* g, vd_model* m, const int32_t* idx, int n) {
  hipStream_t s = m->s_main;
  std::vector<SeqLSTM>* layers = m->enc->rnnLayers();
  const int L = (int)g->rnn.size(), seqLen = m->gen_seq_len;
  const long H = g->H;
  for (int l = 0; l < L; ++l) {
    GenState st;
    VD_TRY(gen_state(g, m, l, n, &st));
    if (layers) {
      VD_CHECK_ARG(l < (int)layers->size(), "decoder has more layers than the encoder's recurrence");
      const float* hs = l == (int)layers->size() - 1 ? m->gen_enc_out : (*layers)[l].out_at(seqLen - 1);
      VD_TRY(vd_embed_gather(hs, idx, nullptr, st.h, n, (int)H, 1.f, s));
      VD_TRY(vd_embed_gather((*layers)[l].cell_at(seqLen - 1), idx, nullptr, st.c, n, (int)H, 1.f, s));
    } else {
      VD_TRY(vd_memset(st.c, 0, (long)n * H * 4, s));
      if (l == L - 1) VD_TRY(vd_embed_gather(m->gen_enc_out, idx, nullptr, st.h, n, (int)H, 1.f, s));
      else VD_TRY(vd_memset(st.h, 0, (long)n * H * 4, s));
    }
  }
  g->gen_n = n;
  return VD_OK;
}
inline int Gen_begin(Gen* g, vd_model* m, const int32_t* rounds, int n) {
  VD_CHECK_ARG(m->gen_enc_out && rounds && n > 0, "vd_model_decode_begin: call vd_model_encode first");
  for (int i = 0; i < n; ++i) VD_CHECK_ARG(rounds[i] >= 0 && rounds[i] < m->N, "vd_model_decode_begin: round %d out of range", rounds[i]);
  int32_t* idx;
  VD_TRY(gen_rows(m, "gen.idx", rounds, n, &idx));
  return gen_begin_rows(g, m, idx, n);
}
// The device part of one decoder step (model.lua:518-522): the n hypotheses' tokens (device) through embedding, LSTM stack
// and vocabulary projection from the current state gen.h<l> / gen.c<l> -> logits [n x Vp]; the stepped state is left in
// rnn[l].out_at(0) / cell_at(0).  Shared by vd_model_decode_step and the batched generations.
inline int gen_forward(Gen* g, vd_model* m, const int32_t* tok, int n, float** logits) {
  hipStream_t s = m->s_main;
  const long H = g->H, E = g->E, V = g->V, Vp = g->Vp;
  for (size_t l = 0; l < g->rnn.size(); ++l) {
    GenState st;
    VD_TRY(gen_state(g, m, l, n, &st));
    g->rnn[l].userPrevOutput = st.h;
    g->rnn[l].userPrevCell = st.c;
  }
  float *x, *top;
  VD_TRY(ws_get(m, "gen1.x", (size_t)n * E, &x));
  VD_TRY(ws_get(m, "gen1.logits", (size_t)n * Vp, logits));
  VD_TRY(vd_embed_gather(Wp(m, "embed"), tok, nullptr, x, n, (int)E, 1.f, s));
  VD_TRY(lstm_stack_forward(m, s, g->rnn, {x}, 1, n, tok, &top));
  VD_TRY(vd_gemm_nt(top, H, Wp(m, "vocab.W"), H, Wp(m, "vocab.b"), *logits, Vp, n, (int)V, (int)H, VD_ACT_NONE, 0, s));
  return VD_OK;
}
// model.lua:518-522 / :590-596: one decoder step for the n live hypotheses -> log-probabilities [n x V] on the host
inline int Gen_step(Gen* g, vd_model* m, const int32_t* tokens, float* host_logp) {
  const int n = g->gen_n;
  VD_CHECK_ARG(n > 0 && tokens && host_logp, "vd_model_decode_step: call vd_model_decode_begin first");
  hipStream_t s = m->s_main;
  const long E = g->E, V = g->V, Vp = g->Vp;
  int32_t* tok;
  VD_TRY(gen_rows(m, "gen.tok", tokens, n, &tok));
  VD_TRY(vd_memset(Wp(m, "embed"), 0, E * 4, s));                                   // LookupTableMaskZero pad row
  float* logits;
  VD_TRY(gen_forward(g, m, tok, n, &logits));
  VD_TRY(vd_log_softmax_rows(logits, Vp, n, (int)V, s));
  VD_TRY(gen_carry(g, m, n, true));                                                  // kept for vd_model_decode_select
  VD_HIP(hipMemcpy2DAsync(host_logp, (size_t)V * 4, logits, (size_t)Vp * 4, (size_t)V * 4, (size_t)n, hipMemcpyDeviceToHost, s));
  VD_HIP(hipStreamSynchronize(s));
  // Sequencer(MaskZero(Linear)) + Sequencer(MaskZero(LogSoftMax)) (decoders/gen.lua:23-24): the row of a hypothesis whose token is 0 -- a
  // beam slot that was never filled (model.lua:560) -- is all ZEROS, not log_softmax(bias); its state is already zero (maskZero)
  for (int i = 0; i < n; ++i)
    if (tokens[i] == 0) memset(host_logp + (size_t)i * V, 0, (size_t)V * 4);
  return VD_OK;
}
// model.lua:560-575: hypothesis i continues from the stepped state of hypothesis src[i]; slots >= n_keep keep theirs
inline int Gen_select(Gen* g, vd_model* m, const int32_t* src, int n_keep) {
  const int n = g->gen_n;
  VD_CHECK_ARG(n > 0 && src && n_keep >= 0 && n_keep <= n, "vd_model_decode_select: bad arguments");
  for (int i = 0; i < n_keep; ++i) VD_CHECK_ARG(src[i] >= 0 && src[i] < n, "vd_model_decode_select: src[%d] = %d out of range", i, src[i]);
  if (n_keep == 0) return VD_OK;
  hipStream_t s = m->s_main;
  int32_t* idx;
  VD_TRY(gen_rows(m, "gen.idx", src, n_keep, &idx));
  for (size_t l = 0; l < g->rnn.size(); ++l) {
    GenState st;
    VD_TRY(gen_state(g, m, l, n, &st));
    VD_TRY(vd_embed_gather(st.hn, idx, nullptr, st.h, n_keep, (int)g->H, 1.f, s));
    VD_TRY(vd_embed_gather(st.cn, idx, nullptr, st.c, n_keep, (int)g->H, 1.f, s));
  }
  return VD_OK;
}

// The batched generations (vd_model_beam_search, vd_model_sample) run every round of the last vd_model_encode batch at once, on
// s_main only.  gen_batch_begin: hypothesis row i = slot i % k of round i / k starts from that round's encoder state (hiddenBeams,
// model.lua:478-503).  gen_batch_steps: steps 1 .. `steps` of gen_forward on the device tokens `tok` -> `head(step, logits)`, the
// mode's kernels, which leave the next tokens in `tok` -> gen_carry (by the beam's back-pointers `src`, or a copy); the tokens never
// leave the device.  gen_read_back: the results come back in ONE copy after the last step.
inline int gen_batch_begin(Gen* g, vd_model* m, int k) {
  const int n = m->N * k;
  std::vector<int32_t> rounds(n);
  for (int i = 0; i < n; ++i) rounds[i] = i / k;
  return Gen_begin(g, m, rounds.data(), n);
}
template <class Head>
inline int gen_batch_steps(Gen* g, vd_model* m, int steps, const int32_t* tok, const int32_t* src, int k, Head head) {
  const int n = g->gen_n;
  VD_TRY(vd_memset(Wp(m, "embed"), 0, g->E * 4, m->s_main));                       // LookupTableMaskZero pad row
  for (int step = 1; step <= steps; ++step) {
    float* logits;
    VD_TRY(gen_forward(g, m, tok, n, &logits));
    VD_TRY(head(step, logits));
    VD_TRY(gen_carry(g, m, n, false, src, k));
  }
  return VD_OK;
}
inline int gen_read_back(vd_model* m, const void* out, size_t bytes, std::vector<uint8_t>* staged) {
  staged->resize(bytes);
  VD_HIP(hipMemcpyAsync(staged->data(), out, bytes, hipMemcpyDeviceToHost, m->s_main));
  VD_HIP(hipStreamSynchronize(m->s_main));
  return VD_OK;
}

// Model:generateAnswers' beam search (model.lua:466-573): N rounds of k slots = N * k hypothesis rows.  Per step: fused
// log-softmax + top-k -> advance (candidate bookkeeping, csrc/beam.hip) -> state select; then the best answer and score per round.
// A model created with VD_BEAM_GROUPS = G > 1 searches every round in G groups of k / G slots (beam.hip D1-D7): the same top-k at the
// full k, the same advance and select with G as an argument; the best-finished state, the start and the answers are those of N * G
// groups of k / G slots, so init and finish take (N * G, k / G) and the answers come back [N x G x L] / [N x G].
// VD_BEAM_MIN_LEN / VD_BEAM_NO_REPEAT (beam.hip C1-C4) swap the top-k for its constrained form, VD_BEAM_LENGTH_PENALTY (C6) hands the
// advance the table s^alpha.
// VD_BEAM_ROLLOUT (beam.hip R1-R6) over an encoder with a history: R = maxQuesCount passes over the chunk's B dialogs instead of one search
// of all N = B * R rounds.  Pass r: the encoder forward on the slot (pass 0's is vd_model_encode's -- by R5 round 0 sees its caption row
// only), the search of round r of every dialog (hypothesis row i = slot i % k of round (i / k) * R + r: B groups through the same
// kernels), vd_beam_finish into the B rows of pass r of the device output [R x B x L] / [R x B], and the append kernel for history row
// r + 1.  Every pass is enqueued on s_main behind the one before it and nothing waits for the host in between; the one copy back is
// re-ordered on the host into the [N x L] / [N] layout (row = dialog * R + round) of the plain call.
inline int Gen_beam_search(Gen* g, vd_model* m, int k, int L, int start, int end, int32_t* host_tokens, double* host_scores) {
  VD_CHECK_ARG(m->gen_enc_out && m->N > 0, "vd_model_beam_search: call vd_model_encode first");
  VD_CHECK_ARG(host_tokens && host_scores && L >= 1, "vd_model_beam_search: bad arguments");
  VD_CHECK_ARG(k >= 1 && k <= 32 && k <= g->V, "vd_model_beam_search: beam size %d must be in [1, min(32, vocabSize)]", k);
  const int groups = m->sw.beam_groups;
  VD_CHECK_ARG(k % groups == 0, "vd_model_beam_search: VD_BEAM_GROUPS = %d does not divide beam size %d", groups, k);
  const bool rollout = m->sw.beam_rollout && m->use_hist;                      // (no history: nothing depends on an answer -- the plain search)
  const int R = m->p.maxQuesCount, passes = rollout ? R : 1;
  const int N = m->N / passes, n = N * k, G = N * groups, kg = k / groups;  // per pass: G answers, each the best of kg slots
  const int min_len = m->sw.beam_min_len, no_repeat = m->sw.beam_no_repeat;
  const bool ban = min_len > 0 || no_repeat > 0, penalty = m->sw.beam_length_penalty > 0.0;
  if (ban) {
    VD_CHECK_ARG(no_repeat == 0 || L <= VD_BEAM_LMAX, "vd_model_beam_search: VD_BEAM_NO_REPEAT = %d needs a beam length %d <= VD_BEAM_LMAX = %d",
                 no_repeat, L, VD_BEAM_LMAX);
    VD_CHECK_ARG((long)g->V >= (long)k + L - 1,
                 "vd_model_beam_search: VD_BEAM_MIN_LEN = %d / VD_BEAM_NO_REPEAT = %d need vocabSize %ld >= beam size %d + beam length %d - 1, "
                 "so that a row never runs out of unbanned words", min_len, no_repeat, (long)g->V, k, L);
    VD_CHECK_ARG(min_len <= L - 2, "vd_model_beam_search: VD_BEAM_MIN_LEN = %d exceeds beam length %d - 2: <END> must be allowed at the last step",
                 min_len, L);
  }
  BatchSlot& b = m->slot[m->cur];
  int32_t* pass_rounds = nullptr;
  if (rollout) {   // the round indices of every pass, cached on the device by shape
    VD_TRY(refuse_round_rollout_in_training(m, "vd_model_beam_search"));
    VD_CHECK_ARG(b.h.present && b.q.present && b.h.N == m->N && b.h.T >= b.q.T, "vd_model_beam_search: VD_BEAM_ROLLOUT = 1 needs the batch's history");
    VD_CHECK_ARG(m->sw.rollout_concat_end == 0 || end == m->sw.rollout_concat_end,
                 "vd_model_beam_search: end_token = %d, but this model was created with VD_ROLLOUT_CONCAT_END = %d: the <END> that separates the "
                 "rounds of a concatenated history row is the one that ends an answer", end, m->sw.rollout_concat_end);
    std::vector<int32_t> rounds((size_t)R * n);
    for (int r = 0; r < R; ++r)
      for (int i = 0; i < n; ++i) rounds[(size_t)r * n + i] = (i / k) * R + r;
    VD_TRY(index_array(m, "idx.rollout." + std::to_string(N) + "." + std::to_string(k) + "." + std::to_string(R), rounds, &pass_rounds));
  } else {
    VD_TRY(gen_batch_begin(g, m, k));
  }
  hipStream_t s = m->s_main;
  int32_t *tok, *top_idx, *src, *hist[2], *best_len, *best_hist;
  float* top_val;
  double *scores, *best_score;
  uint8_t* out;
  const size_t Gall = (size_t)G * passes, tok_bytes = (Gall * L * 4 + 7) / 8 * 8;
  VD_TRY(ws_get(m, "beam.tok", (size_t)n, &tok));
  VD_TRY(ws_get(m, "beam.top_idx", (size_t)n * k, &top_idx));
  VD_TRY(ws_get(m, "beam.top_val", (size_t)n * k, &top_val));
  VD_TRY(ws_get(m, "beam.src", (size_t)n, &src));
  VD_TRY(ws_get(m, "beam.hist0", (size_t)n * L, &hist[0]));
  VD_TRY(ws_get(m, "beam.hist1", (size_t)n * L, &hist[1]));
  VD_TRY(ws_get(m, "beam.scores", (size_t)n, &scores));
  VD_TRY(ws_get(m, "beam.best_score", (size_t)G, &best_score));
  VD_TRY(ws_get(m, "beam.best_len", (size_t)G, &best_len));
  VD_TRY(ws_get(m, "beam.best_hist", (size_t)G * L, &best_hist));
  VD_TRY(ws_get(m, "beam.out", tok_bytes + Gall * 8, &out));
  double* lp = nullptr;
  if (penalty) {                                                            // C6: s^alpha on the host in fp64, uploaded as a table
    m->beam_lp.resize((size_t)L);
    for (int i = 0; i < L; ++i) m->beam_lp[i] = std::pow((double)i, m->sw.beam_length_penalty);
    VD_TRY(ws_get(m, "beam.lp", (size_t)L, &lp));
    VD_HIP(hipMemcpyAsync(lp, m->beam_lp.data(), (size_t)L * 8, hipMemcpyHostToDevice, s));
  }
  const HistRows hr(b);
  m->rollout_max_words = L - 1;
  for (int r = 0; r < passes; ++r) {
    int32_t* out_tok = reinterpret_cast<int32_t*>(out) + (size_t)r * G * L;
    if (rollout) {
      if (r > 0) {                                                          // R5: rows 0 .. r of every dialog are final now
        float* enc_out = nullptr;
        m->gen_enc_out = nullptr;
        VD_TRY(rollout_encode(m, s, b, r, &enc_out));
        m->gen_enc_out = enc_out;
        m->gen_seq_len = m->enc->seqLen(b);
      }
      VD_TRY(gen_begin_rows(g, m, pass_rounds + (size_t)r * n, n));
    }
    VD_TRY(vd_beam_init(G, kg, L, start, hist[0], tok, scores, best_score, best_len, s));
    VD_TRY(gen_batch_steps(g, m, L - 1, tok, src, k, [&](int step, float* logits) -> int {
      if (ban)
        VD_TRY(vd_beam_topk_ban_p(logits, g->Vp, n, (int)g->V, tok, k, hist[0], L, step, min_len, no_repeat, end, top_idx, top_val, s));
      else
        VD_TRY(vd_beam_topk(logits, g->Vp, n, (int)g->V, tok, k, top_idx, top_val, s));
      VD_TRY(vd_beam_advance_p(top_idx, top_val, N, k, groups, (float)m->sw.beam_diversity, step, L, end, scores, hist[0], hist[1], src, tok,
                               best_score, best_len, best_hist, lp, s));
      std::swap(hist[0], hist[1]);
      return VD_OK;
    }));
    VD_TRY(vd_beam_finish(G, kg, L, hist[0], scores, best_score, best_len, best_hist, out_tok,
                          reinterpret_cast<double*>(out + tok_bytes) + (size_t)r * G, s));
    if (rollout && r + 1 < R)                                               // R2: the answer becomes history row r + 1
      VD_TRY(vd_beam_rollout_append_p(out_tok, L, end, b.q.tok, b.q.T, N, R, r, hr.tok, hr.tok_sorted, hr.inv, b.h.T, s, m->sw.rollout_concat_end));
  }
  std::vector<uint8_t> staged;
  VD_TRY(gen_read_back(m, out, tok_bytes + Gall * 8, &staged));
  if (!rollout) {
    memcpy(host_tokens, staged.data(), Gall * L * 4);
    memcpy(host_scores, staged.data() + tok_bytes, Gall * 8);
    return VD_OK;
  }
  for (int r = 0; r < R; ++r)                                               // [R x B] -> row = dialog * R + round
    for (int i = 0; i < N; ++i) {
      memcpy(host_tokens + ((size_t)i * R + r) * L, staged.data() + ((size_t)r * N + i) * L * 4, (size_t)L * 4);
      memcpy(host_scores + (size_t)i * R + r, staged.data() + tok_bytes + ((size_t)r * N + i) * 8, 8);
    }
  return VD_OK;
}

// Model:generateAnswers' temperature sampling (model.lua:576-613): hypothesis row i = round i.  The host's uniforms [L x N] go up
// in one copy; per step: fused log-softmax + inverse-CDF draw (csrc/sample.hip; over the top-k / nucleus kept set for a model created with
// VD_SAMPLE_TOPK / VD_SAMPLE_TOPP) -> the stepped state becomes the current one.
// History, log-likelihoods and the status word share one buffer and come back together.
inline int Gen_sample(Gen* g, vd_model* m, int L, int start, int end, double T, const double* host_u, int32_t* host_tokens,
                      double* host_loglik) {
  VD_CHECK_ARG(m->gen_enc_out && m->N > 0, "vd_model_sample: call vd_model_encode first");
  VD_CHECK_ARG(!m->sw.beam_rollout, "vd_model_sample: this model was created with VD_BEAM_ROLLOUT = 1: a rollout feeds the beam search's answers "
               "back, and one divergent draw would cascade over the rounds; create the sampling model without the variable");
  VD_CHECK_ARG(host_u && host_tokens && host_loglik, "vd_model_sample: bad arguments");
  VD_CHECK_ARG(L >= 1, "vd_model_sample: beam_len = %d must be >= 1", L);
  VD_CHECK_ARG(std::isfinite(T) && T > 0, "vd_model_sample: temperature %g must be finite and > 0", T);
  const int n = m->N;
  for (long i = 0; i < (long)L * n; ++i)
    VD_CHECK_ARG(host_u[i] >= 0.0 && host_u[i] < 1.0, "vd_model_sample: uniform %ld = %g is outside [0, 1)", i, host_u[i]);
  VD_TRY(gen_batch_begin(g, m, 1));
  hipStream_t s = m->s_main;
  const size_t cols = (size_t)L + 1, hist_bytes = ((size_t)n * cols * 4 + 7) / 8 * 8, out_bytes = hist_bytes + (size_t)n * 8 + 8;
  uint8_t* out;
  double* u;
  int32_t* tok;
  VD_TRY(ws_get(m, "sample.out", out_bytes, &out));
  VD_TRY(ws_get(m, "sample.u", (size_t)L * n, &u));
  VD_TRY(ws_get(m, "sample.tok", (size_t)n, &tok));
  int32_t* hist = reinterpret_cast<int32_t*>(out);
  double* loglik = reinterpret_cast<double*>(out + hist_bytes);
  int32_t* status = reinterpret_cast<int32_t*>(out + hist_bytes + (size_t)n * 8);
  VD_HIP(hipMemcpyAsync(u, host_u, (size_t)L * n * 8, hipMemcpyHostToDevice, s));
  VD_TRY(vd_sample_init(n, L, start, hist, tok, loglik, status, s));
  const int top_k = m->sw.sample_topk >= g->V ? 0 : m->sw.sample_topk;   // k >= V keeps every column: off
  const double top_p = m->sw.sample_topp;
  VD_TRY(gen_batch_steps(g, m, L, tok, nullptr, 1, [&](int step, float* logits) {
    if (top_k > 0 || top_p < 1.0)
      return vd_sample_draw_trunc_p(logits, g->Vp, n, (int)g->V, tok, u + (size_t)(step - 1) * n, T, top_k, top_p, step, L, end, hist, loglik,
                                    status, s);
    return vd_sample_draw(logits, g->Vp, n, (int)g->V, tok, u + (size_t)(step - 1) * n, T, step, L, end, hist, loglik, status, s);
  }));
  std::vector<uint8_t> staged;
  VD_TRY(gen_read_back(m, out, out_bytes, &staged));
  int32_t st;
  memcpy(&st, staged.data() + hist_bytes + (size_t)n * 8, 4);
  VD_CHECK_ARG(st == 0, "vd_model_sample: every weight exp(logp / temperature) of a row underflowed at temperature %g: nothing to sample "
               "from (the per-dialog path fails there too)", T);
  memcpy(host_tokens, staged.data(), (size_t)n * cols * 4);
  memcpy(host_loglik, staged.data() + hist_bytes, (size_t)n * 8);
  return VD_OK;
}

inline std::unique_ptr<Decoder> make_decoder(const std::string& n) {
  if (n == "disc") return std::unique_ptr<Decoder>(new Disc());
  if (n == "gen") return std::unique_ptr<Decoder>(new Gen());
  return nullptr;
}

}  // namespace vdrt
