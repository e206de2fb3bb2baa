// Native step runtime, part 2: the encoder plug-ins (reference encoders/<name>.lua, 11 files) as launch orders over the
// operator-level entry points.  Mirrors visdial_amd/encoders/_blocks.py, _late_fusion.py, _hre.py and the four
// nngraph encoder files.  Included by runtime.hip only.
//   WaveStack      one two-layer length-sorted maskZero stack; wave_forward / wave_backward launch n of them as one wavefront
//   TextBranches   the history + question stacks of the nngraph encoders (n = 2)
//   HistoryBranch  hist1..histL of the Sequential encoders: the wavefront (n = 1) at two layers, one recurrence per layer otherwise
//   history_round  the history branch of a round pass, every family
#pragma once
#include "rt_core.h"

namespace vdrt {

struct Encoder {
  virtual ~Encoder() {}
  virtual void declare(vd_model* m) = 0;
  // returns the encoder output [N x H] (a workspace buffer); everything is enqueued on `s` and the library's side lane
  // that are joined back into `s` before returning
  virtual int forward(vd_model* m, hipStream_t s, BatchSlot& b, float** out) = 0;
  virtual int backward(vd_model* m, hipStream_t s, BatchSlot& b, const float* grad_out) = 0;
  // One pass r >= 1 of a rollout (VD_ROLLOUT_ENCODER = round), for the encoders with a history, evaluation mode, everything on `s`.
  //   before: forward() ran on this slot since its upload (pass 0), then forward_round for 1 .. r - 1, and history row r of every dialog
  //           has just been written into b.h.tok
  //   after:  *out is the [N x H] buffer forward() returned; rows d * R + r are final, rows of rounds < r are untouched (rows of later
  //           rounds stay what they were: stale, finite, rewritten by their own pass)
  // It reads what pass 0 left and does not depend on the history -- the question stacks' states (rnnLayers() / seqLen), q.last, the
  // SAN's per-image `pre` -- and writes none of it; its own workspace is named rnd.* so that no buffer of pass 0 is resized.
  virtual int forward_round(vd_model* m, hipStream_t s, BatchSlot& b, int r, float** out) {
    vd_set_error("encoder '%s' has no history: a rollout never asks it for a round pass", m->enc_name.c_str());
    return VD_ERR_STATE;
  }
  float* out_ = nullptr;   // what the last forward() returned: a round pass writes its rows into it
  // the precondition of a round pass; `state` = what else the encoder keeps from pass 0
  int round_ready(vd_model* m, const BatchSlot& b, bool state = true) const {
    const int N = b.q.N, R = m->p.maxQuesCount;
    VD_CHECK_ARG(out_ && state && N == N / R * R && b.h.N == N, "round pass without a full encoder pass on this batch");
    return VD_OK;
  }
  // enc.rnnLayers of the Sequential encoders (read by decoders/gen.lua:31-35,46-52); null for the nngraph encoders
  virtual std::vector<SeqLSTM>* rnnLayers() { return nullptr; }
  virtual int seqLen(const BatchSlot& b) const { return b.q.T; }
};

// arithmetic of the encoder's recurrent products: bf16 operands in a bf16 pass (lstmPrecision = 'bf16', BASELINE configs[4] "bf16 LSTM
// step"), fp32 MFMA otherwise (the exact-split modes of the option recurrence leave the encoder on fp32: it is not on their critical path)
inline int tick_flags(const vd_model* m) { return m->flags & VD_FLAG_BF16; }

inline int causal_mask(vd_model* m, int B, int R, uint8_t** out) {
  // model.lua:280-294: mask[i][j] = 0 iff j <= i, tiled over the batch ([N x R] bytes, 1 = hidden)
  const std::string key = "causal." + std::to_string(B);
  DevBuf& d = m->ws[key];
  const size_t n = (size_t)B * R * R;
  if (!d.p) {
    std::vector<uint8_t> host(n);
    for (int r = 0; r < B * R; ++r)
      for (int j = 0; j < R; ++j) host[(size_t)r * R + j] = j > (r % R) ? 1 : 0;
    VD_HIP(hipMalloc(&d.p, n + 16));
    d.bytes = n;
    VD_HIP(hipMemcpy(d.p, host.data(), n, hipMemcpyHostToDevice));
  }
  *out = static_cast<uint8_t*>(d.p);
  return VD_OK;
}

// ------------------------------------------------------------------------------------------------------------
// One text stack: shared embedding [-> Dropout(0.5)] -> 2 x SeqLSTM(maskZero) -> Select(1,-1), on rows sorted by length at upload
// (right-aligned input: the leading pad steps of the shorter rows are skipped, maskZero's zero state is what they would produce).  Both
// layers advance as ONE skewed wavefront (vd_lstm2_forward_p / vd_lstm2_backward_p: T + 1 launches instead of 2 T), several stacks per
// launch; weight gradients run over the non-pad (t, row) pairs.
//   the nngraph encoders (mn-att:21-45): history + question stacks in one launch, Dropout behind the embedding (TextBranches)
//   the Sequential encoders (lf-ques-hist.lua:38-45, lf-ques-im-hist.lua:38-45, hre-*.lua:30-38): the history stack at the default two
//   layers, no Dropout (HistoryBranch).  At lf-ques-im-hist's Th <= 300 (the concatenated dialog, dataloader.lua:243-255) it IS the step
//   (configs[1]).
// ------------------------------------------------------------------------------------------------------------
struct WaveStack {
  SeqLSTM *l1 = nullptr, *l2 = nullptr;
  std::string tag;            // workspace tag: "h" or "q"
  bool drop = false;          // the nn.Dropout(0.5) behind the shared embedding (mn-att:24-25)
  uint8_t* mask = nullptr;    // its keep-mask of this step (null without `drop` and in evaluate mode)

  int prepare(vd_model* m, hipStream_t s, const SeqTok& ss) {
    VD_CHECK_ARG(ss.sorted, "the '%s' stack (%s, %s) runs on length-sorted rows only", tag.c_str(), l1->name.c_str(), l2->name.c_str());
    const long E = l1->D, H = l1->H;
    const long TN = (long)ss.T * ss.N;
    mask = nullptr;
    if (drop) VD_TRY(drop_mask(m, tag + "_emb", (size_t)TN * E, 0.5f, s, &mask));
    float *x, *xs;
    VD_TRY(ws_get(m, tag + ".x", (size_t)TN * E, &x));
    VD_TRY(ws_get(m, tag + ".xs", (size_t)TN * E, &xs));
    VD_TRY(l1->alloc(m, ss.T, ss.N));
    VD_TRY(l2->alloc(m, ss.T, ss.N));
    l1->h0 = l1->c0 = l2->h0 = l2->c0 = nullptr;
    VD_TRY(vd_embed_gather(Wp(m, "embed"), ss.tok, mask, x, TN, (int)E, drop ? 2.0f : 1.0f, s));
    VD_TRY(vd_embed_gather(x, ss.fwd_idx, nullptr, xs, TN, (int)E, 1.0f, s));      // permute rows per step (length sort)
    VD_TRY(vd_gemm_nn(xs, E, l1->Wx(m), 4 * H, Wp(m, l1->name + ".b"), l1->gates, 4 * H, (int)TN, (int)(4 * H), (int)E, 0, s));
    // skipped (t, row) pairs must read as zeros: previous state of rows that become active later, da = 0 in the
    // weight-gradient contractions.  Only the skipped pairs, all six buffers in one launch: the active rows are written by the
    // recurrence before anything reads them
    VdZeroSet z{{l1->gates, l1->h, l1->c, l2->h, l2->c, l2->gates}, {(int)(4 * H), (int)H, (int)H, (int)H, (int)H, (int)(4 * H)}, 6, 0};
    VD_TRY(vd_zero_inactive_multi(z, ss.nact_dev, ss.T, ss.N, s));
    l1->xs = {xs};
    l2->xs = {l1->h};
    l1->rows = l2->rows = &ss;
    return VD_OK;
  }
  // T steps of N rows through the layers' weights on the buffers {layer 1, layer 2} of gates / h / c; nact = null: every row at every step
  static void fill_fwd(vd_model* m, const SeqLSTM& l1, const SeqLSTM& l2, int T, int N, const int32_t* tok_mask, const int32_t* nact,
                       float* const* gates, float* const* h, float* const* c, vd_lstm2_fwd_t* o) {
    o->T = T; o->N = N;
    o->tok_mask = tok_mask;
    o->Wh1 = l1.Wh(m); o->Wx2 = l2.Wx(m); o->b2 = Wp(m, l2.name + ".b"); o->Wh2 = l2.Wh(m);
    o->gates1 = gates[0]; o->h1 = h[0]; o->c1 = c[0]; o->gates2 = gates[1]; o->h2 = h[1]; o->c2 = c[1];
    o->nact = nact;
  }
  void fill_fwd(vd_model* m, const SeqTok& ss, vd_lstm2_fwd_t* o) const {
    float *gates[2] = {l1->gates, l2->gates}, *h[2] = {l1->h, l2->h}, *c[2] = {l1->c, l2->c};
    fill_fwd(m, *l1, *l2, ss.T, ss.N, ss.tok_sorted, ss.nact.data(), gates, h, c, o);
  }
  // also requests <l1>.dhseq, <l1>.dc and <l2>.dc; dlast = the gradient of the top layer's last state, in sorted row order
  int fill_bwd(vd_model* m, const SeqTok& ss, const float* dlast, vd_lstm2_bwd_t* o) const {
    const long H = l1->H;
    float *dhseq, *dc1, *dc2;
    VD_TRY(ws_get(m, l1->name + ".dhseq", (size_t)ss.T * ss.N * H, &dhseq));
    VD_TRY(ws_get(m, l1->name + ".dc", (size_t)ss.N * H, &dc1));
    VD_TRY(ws_get(m, l2->name + ".dc", (size_t)ss.N * H, &dc2));
    o->T = ss.T; o->N = ss.N;
    o->Wh1 = l1->Wh(m); o->Wx2 = l2->Wx(m); o->Wh2 = l2->Wh(m);
    o->gates1 = l1->gates; o->c1 = l1->c; o->gates2 = l2->gates; o->c2 = l2->c;
    o->dh_last2 = dlast;
    o->dh1_seq = dhseq; o->dc1 = dc1; o->dc2 = dc2;
    o->nact = ss.nact.data();
    return VD_OK;
  }
  // Select(1,-1) of the top layer, back to batch order, into <tag>.last
  int gather_last(vd_model* m, hipStream_t s, const SeqTok& ss, float** last) const {
    const long H = l2->H;
    VD_TRY(ws_get(m, tag + ".last", (size_t)ss.N * H, last));
    return vd_embed_gather(l2->out_at(ss.T - 1), ss.inv, nullptr, *last, ss.N, (int)H, 1.f, s);
  }
  // its gradient, into sorted row order, into <tag>.dlast
  int gather_dlast(vd_model* m, hipStream_t s, const SeqTok& ss, const float* dlast, float** sorted) const {
    const long H = l2->H;
    VD_TRY(ws_get(m, tag + ".dlast", (size_t)ss.N * H, sorted));
    return vd_embed_gather(dlast, ss.perm, nullptr, *sorted, ss.N, (int)H, 1.f, s);
  }
  // behind the recurrences only parameter gradients are left: layer 2, layer 1, the embedding rows
  int param_tail(vd_model* m, hipStream_t s, const SeqTok& ss) const {
    const long E = l1->D, TN = (long)ss.T * ss.N;
    std::vector<float*> dx;
    float* dxo;
    VD_TRY(l2->param_grads(m, s, {false}, nullptr));
    VD_TRY(l1->param_grads(m, s, {true}, &dx));
    VD_TRY(ws_get(m, tag + ".dxo", (size_t)TN * E, &dxo));
    VD_TRY(vd_embed_gather(dx[0], ss.inv_idx, nullptr, dxo, TN, (int)E, 1.f, s));     // back to batch order
    return vd_embed_scatter_acc(Gp(m, "embed"), ss.tok, mask, dxo, TN, (int)E, drop ? 2.f : 1.f, s);
  }
};

// n <= 2 stacks as one wavefront.  last[k] / dlast[k]: the top layer's last state of stack k and its gradient [N x H], batch order.
// wave_backward ends behind the recurrences: the caller runs every stack's param_tail on the stream it chooses.
inline int wave_forward(vd_model* m, hipStream_t s, WaveStack* const* st, const SeqTok* const* ss, int n, float** last) {
  vd_lstm2_fwd_t fw[2];
  for (int k = 0; k < n; ++k) VD_TRY(st[k]->prepare(m, s, *ss[k]));
  for (int k = 0; k < n; ++k) st[k]->fill_fwd(m, *ss[k], &fw[k]);
  VD_TRY(vd_lstm2_forward_p(fw, n, (int)st[0]->l1->H, tick_flags(m), s));
  for (int k = 0; k < n; ++k) VD_TRY(st[k]->gather_last(m, s, *ss[k], &last[k]));
  return VD_OK;
}
inline int wave_backward(vd_model* m, hipStream_t s, WaveStack* const* st, const SeqTok* const* ss, int n, const float* const* dlast) {
  vd_lstm2_bwd_t bw[2];
  float* sorted[2];
  for (int k = 0; k < n; ++k) VD_TRY(st[k]->gather_dlast(m, s, *ss[k], dlast[k], &sorted[k]));
  for (int k = 0; k < n; ++k) VD_TRY(st[k]->fill_bwd(m, *ss[k], sorted[k], &bw[k]));
  return vd_lstm2_backward_p(bw, n, (int)st[0]->l1->H, tick_flags(m), s);
}

// history + question branches of the nngraph encoders (mn-att:21-45)
struct TextBranches {
  SeqLSTM hist1, hist2, ques1, ques2;
  WaveStack hist{&hist1, &hist2, "h", true}, ques{&ques1, &ques2, "q", true};
  static void declare(vd_model* m) {
    const long E = m->p.embedSize, H = m->p.rnnHiddenSize;
    add_lstm(m, "hist1", E, H); add_lstm(m, "hist2", H, H); add_lstm(m, "ques1", E, H); add_lstm(m, "ques2", H, H);
  }
  void init(vd_model* m) {
    const long E = m->p.embedSize, H = m->p.rnnHiddenSize;
    hist1.init("hist1", E, H); hist2.init("hist2", H, H); ques1.init("ques1", E, H); ques2.init("ques2", H, H);
  }
  int forward(vd_model* m, hipStream_t s, BatchSlot& b, float** q3, float** h3) {
    WaveStack* st[2] = {&hist, &ques};
    const SeqTok* ss[2] = {&b.h, &b.q};
    float* last[2];
    VD_TRY(wave_forward(m, s, st, ss, 2, last));
    *h3 = last[0];
    *q3 = last[1];
    return VD_OK;
  }
  int backward(vd_model* m, hipStream_t s, BatchSlot& b, const float* dq3, const float* dh3) {
    WaveStack* st[2] = {&hist, &ques};
    const SeqTok* ss[2] = {&b.h, &b.q};
    const float* dlast[2] = {dh3, dq3};
    VD_TRY(wave_backward(m, s, st, ss, 2, dlast));
    hipStream_t sw;
    VD_TRY(wg_fork(m, s, &sw));                 // the recurrences are done: only parameter gradients are left
    wgrad_begin(m);                             // both stacks' dense weight gradients: one live-row launch behind the tails
    for (int k = 0; k < 2; ++k) VD_TRY(st[k]->param_tail(m, sw, *ss[k]));
    return wgrad_end(m, b, sw);
  }
};

inline int rows_copy(float* dst, long dst_ld, const float* src, long src_ld, long rows, int cols, hipStream_t s) {
  const int64_t ld = src_ld;
  return vd_rows_cat_p(dst, dst_ld, &src, &ld, &cols, 1, rows, s);
}
inline int round_linear(vd_model* m, hipStream_t s, const std::string& name, const float* x, long ldx, long in, long out, int rows, bool tanh,
                        float* y, long ldy) {
  return vd_gemm_nt(x, ldx, Wp(m, name + ".W"), in, Wp(m, name + ".b"), y, ldy, rows, (int)out, (int)in, tanh ? VD_ACT_TANH : VD_ACT_NONE, 0, s);
}
// The history branch of a round pass on a CONCATENATED history (VD_ROLLOUT_CONCAT_END; beam.hip CH6): row r of a dialog is row r - 1 followed by
// the new tokens CH4 kept, so the stack's state after row r is its state after row r - 1 continued over those tokens -- at most 1 + Tq +
// (words of an answer) columns (41 at full size) instead of Th (300).  Pass 1 first gathers every dialog's row-0 final (h, c) of both layers
// from what pass 0 left (the rows are length-sorted on the wavefront path: through `inv`) into rnd.carry.* [B x H].  Pass r: the window of new
// tokens [Wn x B] (vd_rollout_concat_window_p), its embedding, and per layer the input projection and ONE vd_lstm_forward from the carry with
// VD_FLAG_HOLD (a row's pad in front of its tokens keeps the carried state); the last step is the new carry and *last.  9 + 2 Wn launches and
// four copies.  Every precondition that fails is an error: the full-width history_round is never substituted.
// (A wavefront with an initial state -- Wn + 2 launches instead of 2 Wn -- is a follow-up; DESIGN.md "One round per pass" has the contract.)
inline int history_round_concat(vd_model* m, hipStream_t s, BatchSlot& b, const std::vector<const SeqLSTM*>& layers, int r, float* cache,
                                const float** last) {
  const int N = b.h.N, W = b.h.T, R = m->p.maxQuesCount, B = N / R, L = (int)layers.size();
  VD_CHECK_ARG(b.h.present && b.q.present && N == B * R && r >= 1 && r < R, "round pass %d of %d rounds over %d history rows", r, R, N);
  VD_CHECK_ARG(L == 2, "VD_ROLLOUT_ENCODER = round on a concatenated history (VD_ROLLOUT_CONCAT_END) continues a two-layer history stack; this "
               "model has numLayers = %d: use VD_ROLLOUT_ENCODER = full", L);
  VD_CHECK_ARG(!(m->flags & VD_FLAG_BF16), "VD_ROLLOUT_ENCODER = round on a concatenated history continues the history stack through "
               "VD_FLAG_HOLD, which runs exact fp32 steps; this model's recurrences run in bf16: use VD_ROLLOUT_ENCODER = full");
  VD_CHECK_ARG(m->rollout_max_words >= 0 && layers[0]->h && layers[0]->T == W && layers[0]->N == N && layers[1]->T == W && layers[1]->N == N,
               "round pass on a concatenated history without a full encoder pass on this batch");
  const long E = layers[0]->D, H = layers[0]->H, BH = (long)B * H;
  const int Wn = (int)std::min<long>(W, 1L + b.q.T + m->rollout_max_words);
  const long TB = (long)Wn * B;
  float* carry[2][2];   // [layer][h, c]
  for (int l = 0; l < 2; ++l)
    for (int k = 0; k < 2; ++k)
      VD_TRY(ws_get(m, std::string("rnd.carry.") + (k ? "c" : "h") + std::to_string(l + 1), (size_t)BH, &carry[l][k]));
  if (r == 1) {   // the states pass 0 left for row 0 of every dialog: the last step, sorted row inv[d * R] (or row d * R without a sort)
    float* rows;
    VD_TRY(ws_get(m, "rnd.carry.rows", (size_t)N * H, &rows));
    for (int l = 0; l < 2; ++l)
      for (int k = 0; k < 2; ++k) {
        const float* src = k ? layers[l]->cell_at(W - 1) : layers[l]->out_at(W - 1);
        if (b.h.sorted) {
          VD_TRY(vd_embed_gather(src, b.h.inv, nullptr, rows, N, (int)H, 1.f, s));
          src = rows;
        }
        VD_TRY(rows_copy(carry[l][k], H, src, (long)R * H, B, (int)H, s));
      }
  }
  int32_t* tok;
  float* x;
  VD_TRY(ws_get(m, "rnd.cw.tok", (size_t)TB, &tok));
  VD_TRY(ws_get(m, "rnd.cw.x", (size_t)TB * E, &x));
  VD_TRY(vd_rollout_concat_window_p(b.h.tok, B, R, r, W, Wn, tok, s));
  VD_TRY(vd_embed_gather(Wp(m, "embed"), tok, nullptr, x, TB, (int)E, 1.f, s));
  float *xp, *h[2], *c[2];
  VD_TRY(ws_get(m, "rnd.cw.xp", (size_t)TB * 4 * H, &xp));
  for (int l = 0; l < 2; ++l) {
    VD_TRY(ws_get(m, "rnd.cw.h" + std::to_string(l + 1), (size_t)TB * H, &h[l]));
    VD_TRY(ws_get(m, "rnd.cw.c" + std::to_string(l + 1), (size_t)TB * H, &c[l]));
    VD_TRY(vd_gemm_nn(l ? h[0] : x, l ? H : E, layers[l]->Wx(m), 4 * H, Wp(m, layers[l]->name + ".b"), xp, 4 * H, (int)TB, (int)(4 * H),
                      (int)(l ? H : E), 0, s));
    VD_TRY(vd_lstm_forward(xp, (int64_t)B * 4 * H, 4 * H, nullptr, tok, layers[l]->Wh(m), carry[l][0], carry[l][1], nullptr, h[l], c[l], Wn, B,
                           (int)H, VD_FLAG_HOLD, s));
  }
  for (int l = 0; l < 2; ++l) {   // the last step is the state after row r (a dialog without a kept token held its carry through)
    VD_HIP(hipMemcpyAsync(carry[l][0], h[l] + (long)(Wn - 1) * BH, (size_t)BH * 4, hipMemcpyDeviceToDevice, s));
    VD_HIP(hipMemcpyAsync(carry[l][1], c[l] + (long)(Wn - 1) * BH, (size_t)BH * 4, hipMemcpyDeviceToDevice, s));
  }
  *last = carry[1][0];
  if (cache) VD_TRY(rows_copy(cache + (long)r * H, (long)R * H, *last, H, B, (int)H, s));
  return VD_OK;
}

// The history branch of a round pass (Encoder::forward_round), every encoder family: history row r of the B dialogs as a B-row sequence at
// full width -- step-major [Th x B], every row active at every step, maskZero per token (a rollout model lays rows >= 1 out at full width
// anyway, runtime.hip upload_tokens) -- through the branch's layers: the two-layer wavefront, or one recurrence per layer for another
// depth.  *last = the top layer's final state [B x H], also copied into rows d * R + r of `cache` [N x H], pass 0's last states (null: no
// copy).  Th + 4 launches with two layers, and the copy.
inline int history_round(vd_model* m, hipStream_t s, BatchSlot& b, const std::vector<const SeqLSTM*>& layers, int r, float* cache,
                         const float** last) {
  if (m->sw.rollout_concat_end) return history_round_concat(m, s, b, layers, r, cache, last);   // CH6: the new tokens alone
  const int N = b.h.N, Th = b.h.T, R = m->p.maxQuesCount, B = N / R, L = (int)layers.size();
  const long E = layers[0]->D, H = layers[0]->H, TB = (long)Th * B;
  VD_CHECK_ARG(b.h.present && N == B * R && r >= 1 && r < R && L >= 1, "round pass %d of %d rounds over %d history rows", r, R, N);
  int32_t* tok;
  float* x;
  VD_TRY(ws_get(m, "rnd.h.tok", (size_t)TB, &tok));
  VD_TRY(ws_get(m, "rnd.h.x", (size_t)TB * E, &x));
  VD_TRY(vd_round_embed_p(Wp(m, "embed"), b.h.tok, Th, N, R, r, tok, x, (int)E, s));
  std::vector<float*> gates(L), h(L), c(L);
  for (int l = 0; l < L; ++l) {
    const std::string key = "rnd.h" + std::to_string(l + 1);
    VD_TRY(ws_get(m, key + ".gates", (size_t)TB * 4 * H, &gates[l]));
    VD_TRY(ws_get(m, key + ".h", (size_t)TB * H, &h[l]));
    VD_TRY(ws_get(m, key + ".c", (size_t)TB * H, &c[l]));
  }
  VD_TRY(vd_gemm_nn(x, E, layers[0]->Wx(m), 4 * H, Wp(m, layers[0]->name + ".b"), gates[0], 4 * H, (int)TB, (int)(4 * H), (int)E, 0, s));
  if (L == 2) {
    vd_lstm2_fwd_t fw;
    WaveStack::fill_fwd(m, *layers[0], *layers[1], Th, B, tok, nullptr, gates.data(), h.data(), c.data(), &fw);
    VD_TRY(vd_lstm2_forward_p(&fw, 1, (int)H, tick_flags(m), s));
  } else {
    for (int l = 0; l < L; ++l) {
      if (l > 0)
        VD_TRY(vd_gemm_nn(h[l - 1], H, layers[l]->Wx(m), 4 * H, Wp(m, layers[l]->name + ".b"), gates[l], 4 * H, (int)TB, (int)(4 * H), (int)H, 0, s));
      VD_TRY(vd_lstm_forward(gates[l], (int64_t)B * 4 * H, 4 * H, nullptr, tok, layers[l]->Wh(m), nullptr, nullptr, gates[l], h[l], c[l], Th, B,
                             (int)H, 0, s));
    }
  }
  *last = h[L - 1] + (long)(Th - 1) * B * H;
  if (cache) VD_TRY(rows_copy(cache + (long)r * H, (long)R * H, *last, H, B, (int)H, s));
  return VD_OK;
}

// The history branch of the Sequential encoders (encoders/lf-ques-hist.lua:38-45, lf-ques-im-hist.lua:38-45, hre-*.lua:30-38):
// numLayers x SeqLSTM:maskZero() whose only consumer is Select(1,-1) of the top layer.  Two layers, on the rows the upload then sorts
// (runtime.hip vd_model_upload_batch): one WaveStack, its parameter tail on the caller's stream.  Any other depth: the embedding gathered
// into "h.x" and one recurrence per layer.  The caller forks and joins the stream it hands in.
struct HistoryBranch {
  std::vector<SeqLSTM> hist;
  WaveStack wave;
  void declare(vd_model* m) {
    const long E = m->p.embedSize, H = m->p.rnnHiddenSize;
    hist.resize(m->p.numLayers);
    for (size_t l = 0; l < hist.size(); ++l) {
      add_lstm(m, "hist" + std::to_string(l + 1), l == 0 ? E : H, H);
      hist[l].init("hist" + std::to_string(l + 1), l == 0 ? E : H, H);
    }
    if (hist.size() == 2) wave = WaveStack{&hist[0], &hist[1], "h", false};
  }
  bool waved(const BatchSlot& b) const { return hist.size() == 2 && b.h.sorted; }
  // *last = the top layer's last state [N x H] in batch order: "h.last" on the wavefront path, the top layer's last step otherwise
  int forward(vd_model* m, hipStream_t s, BatchSlot& b, float** last) {
    if (waved(b)) {
      WaveStack* st = &wave;
      const SeqTok* ss = &b.h;
      return wave_forward(m, s, &st, &ss, 1, last);
    }
    const int N = b.h.N, Th = b.h.T;
    const long E = hist[0].D;
    float *hx, *ht;
    VD_TRY(ws_get(m, "h.x", (size_t)Th * N * E, &hx));
    VD_TRY(vd_embed_gather(Wp(m, "embed"), b.h.tok, nullptr, hx, (long)Th * N, (int)E, 1.f, s));
    VD_TRY(lstm_stack_forward(m, s, hist, {hx}, Th, N, b.h.tok, &ht));
    *last = hist.back().out_at(Th - 1);
    return VD_OK;
  }
  // ends in the scatter into the embedding gradient
  int backward(vd_model* m, hipStream_t s, BatchSlot& b, const float* dlast) {
    if (waved(b)) {
      WaveStack* st = &wave;
      const SeqTok* ss = &b.h;
      VD_TRY(wave_backward(m, s, &st, &ss, 1, &dlast));
      wgrad_begin(m);
      VD_TRY(wave.param_tail(m, s, b.h));
      return wgrad_end(m, b, s);
    }
    std::vector<float*> dx;
    VD_TRY(lstm_stack_backward(m, s, hist, dlast, nullptr, &dx));
    return vd_embed_scatter_acc(Gp(m, "embed"), b.h.tok, nullptr, dx[0], (long)b.h.T * b.h.N, (int)hist[0].D, 1.f, s);
  }
  int round(vd_model* m, hipStream_t s, BatchSlot& b, int r, float* cache, const float** hl) {
    std::vector<const SeqLSTM*> layers;
    for (const SeqLSTM& l : hist) layers.push_back(&l);
    return history_round(m, s, b, layers, r, cache, hl);
  }
};

// img [B x F] -> "img.rep" [N x F]: the image row of every round (model.lua:262-265)
inline int image_repeat(vd_model* m, hipStream_t s, const BatchSlot& b, int N, float** out) {
  const int R = m->p.maxQuesCount, F = m->p.imgFeatureSize;
  int32_t* rep;
  VD_TRY(round_index(m, N, R, &rep));
  VD_TRY(ws_get(m, "img.rep", (size_t)N * F, out));
  return vd_embed_gather(b.img, rep, nullptr, *out, N, F, 1.f, s);
}

// nn.MM(false,true) -> MaskSoftMax -> nn.MM -> Tanh(Linear(Dropout)) -> Tanh(Linear(hAttTr + query)) (mn-att:48-65)
struct MemoryBlock {
  Linear mn1, mn2;
  long H = 0;
  int R = 0, N = 0, B = 0;
  const float *query = nullptr, *h3 = nullptr;
  float *prob = nullptr, *s2 = nullptr;
  uint8_t* m_hatt = nullptr;
  static void declare(vd_model* m) {
    const long H = m->p.rnnHiddenSize;
    add_linear(m, "mn1", H, H); add_linear(m, "mn2", H, H);
  }
  void init(vd_model* m) {
    H = m->p.rnnHiddenSize; R = m->p.maxQuesCount;
    mn1.init("mn1", H, H); mn2.init("mn2", H, H);
  }
  int forward(vd_model* m, hipStream_t s, const float* query_, const float* h3_, int N_, float** out) {
    query = query_; h3 = h3_; N = N_; B = N / R;
    uint8_t* mask;
    VD_TRY(causal_mask(m, B, R, &mask));
    float* hatt;
    VD_TRY(ws_get(m, "mn.prob", (size_t)N * R, &prob));
    VD_TRY(ws_get(m, "mn.hatt", (size_t)N * H, &hatt));
    VD_TRY(ws_get(m, "mn.s2", (size_t)N * H, &s2));
    VD_TRY(vd_mn_attention_forward(query, h3, mask, prob, hatt, B, R, (int)H, s));
    VD_TRY(drop_mask(m, "hatt", (size_t)N * H, 0.5f, s, &m_hatt));
    const float* hd;
    VD_TRY(dropout_fwd(m, "mn.hatt_d", hatt, m_hatt, 2.f, (long)N * H, s, &hd));
    float* hattTr;
    VD_TRY(mn1.forward(m, s, hd, N, true, &hattTr));
    VD_TRY(vd_axpby(hattTr, query, s2, (long)N * H, 1.f, 1.f, s));   // CAddTable
    return mn2.forward(m, s, s2, N, true, out);
  }
  // round r of every dialog: the query of dialog d is row d of [B x q_ld], the facts are rows (d, 0 .. r) of h3 [N x H]; y [B x ldy]
  int forward_round(vd_model* m, hipStream_t s, const float* query_, long q_ld, const float* h3_, int B_, int r, float* y, long ldy) {
    float *hatt, *qc, *t1, *s2r;
    VD_TRY(ws_get(m, "rnd.mn.hatt", (size_t)B_ * H, &hatt));
    VD_TRY(ws_get(m, "rnd.mn.q", (size_t)B_ * H, &qc));
    VD_TRY(ws_get(m, "rnd.mn.t1", (size_t)B_ * H, &t1));
    VD_TRY(ws_get(m, "rnd.mn.s2", (size_t)B_ * H, &s2r));
    VD_TRY(vd_mn_attention_round_p(query_, q_ld, h3_, nullptr, hatt, qc, B_, R, r, (int)H, s));
    VD_TRY(round_linear(m, s, "mn1", hatt, H, H, H, B_, true, t1, H));
    VD_TRY(vd_axpby(t1, qc, s2r, (long)B_ * H, 1.f, 1.f, s));   // CAddTable
    return round_linear(m, s, "mn2", s2r, H, H, H, B_, true, y, ldy);
  }
  int backward(vd_model* m, hipStream_t s, const float* dqh2, float** dquery, float** dh3) {
    float *ds2, *dhatt_d;
    VD_TRY(mn2.backward(m, s, dqh2, true, &ds2));
    VD_TRY(mn1.backward(m, s, ds2, true, &dhatt_d));
    const float* dha;
    VD_TRY(dropout_fwd(m, "mn.dhatt", dhatt_d, m_hatt, 2.f, (long)N * H, s, &dha));
    float *dq_att, *dh, *dq;
    VD_TRY(ws_get(m, "mn.dq", (size_t)N * H, &dq_att));
    VD_TRY(ws_get(m, "mn.dh", (size_t)N * H, &dh));
    VD_TRY(ws_get(m, "mn.dquery", (size_t)N * H, &dq));
    VD_TRY(vd_mn_attention_backward(query, h3, prob, dha, dq_att, dh, B, R, (int)H, s));
    VD_TRY(vd_axpby(dq_att, ds2, dq, (long)N * H, 1.f, 1.f, s));
    *dquery = dq;
    *dh3 = dh;
    return VD_OK;
  }
};

// Stacked attention over the S x S image regions + output layer (mn-att:68-106), numAttentionLayers hops, each with its
// OWN img_common / ques_common / att Linears and Dropout; `pre` = tanh(Linear(img)) once per IMAGE, per-round Dropout
// masks applied by the GEMM loaders, the 10x repeat (model.lua:262-265) never materialises.
struct SANBlock {
  Linear img_proj, out;
  std::vector<Linear> ques_common;
  long H = 0, C = 0, K = 0;
  int S2 = 0, R = 0, L = 1, N = 0;
  float* pre = nullptr;
  uint8_t *m1 = nullptr, *m_u = nullptr;
  std::vector<uint8_t*> m2;
  std::vector<const float*> u_in;
  std::vector<float*> iqc, patt;
  float sc = 1.f;
  float* xdrop = nullptr;   // split9 pass: dropout1(gather(pre)) [N*S2 x H], materialised once per step
  const int32_t* cnt = nullptr;   // the slot's "@img_regions" [B] or null (attention.hip IR1): the head walks the live regions only
  int iflags = 0;
  static void declare(vd_model* m) {
    const long H = m->p.rnnHiddenSize, C = m->p.imgFeatureSize, K = m->p.commonEmbeddingSize;
    add_linear(m, "img_proj", C, H);
    for (int i = 0; i < std::max(1, m->p.numAttentionLayers); ++i) {
      add_linear(m, "img_common" + hop_sfx(i), H, K);
      add_linear(m, "ques_common" + hop_sfx(i), H, K);
      add_linear(m, "att" + hop_sfx(i), K, 1);
    }
    add_linear(m, "out", H, H);
  }
  void init(vd_model* m) {
    H = m->p.rnnHiddenSize; C = m->p.imgFeatureSize; K = m->p.commonEmbeddingSize;
    S2 = m->p.imgSpatialSize * m->p.imgSpatialSize; R = m->p.maxQuesCount; L = std::max(1, m->p.numAttentionLayers);
    img_proj.init("img_proj", C, H); out.init("out", H, H);
    ques_common.resize(L);
    for (int i = 0; i < L; ++i) ques_common[i].init("ques_common" + hop_sfx(i), H, K);
  }
  // per-image projection + this step's dropout masks: independent of the text branches -> own stream
  int prefetch(vd_model* m, hipStream_t s, BatchSlot& b, int N_) {
    N = N_;
    cnt = b.regions;
    hipStream_t si = side_stream(m, s);
    VD_TRY(fork_stream(m, s, si));
    VD_TRY(img_proj.forward(m, si, b.img, (long)b.B * S2, true, &pre));           // mn-att:74-78 (pre-dropout)
    VD_TRY(drop_mask(m, "img_tr", (size_t)N * S2 * H, 0.5f, si, &m1));
    m2.assign(L, nullptr);
    for (int i = 0; i < L; ++i) VD_TRY(drop_mask(m, "iqc" + hop_sfx(i), (size_t)N * S2 * K, 0.5f, si, &m2[i]));
    sc = m1 ? 2.f : 1.f;
    // split9 pass: the attention's dense products run on the exact split, from the materialised per-round image tensor (attention.hip)
    iflags = (m->flags & VD_FLAG_SPLIT9) && vd_img_split_ok((long)N * S2, (int)H, (int)K) ? VD_FLAG_SPLIT9 : 0;
    xdrop = nullptr;
    if (iflags) {
      VD_TRY(ws_get(m, "att.xdrop", (size_t)N * S2 * H, &xdrop));
      VD_TRY(vd_img_drop_gather(pre, m1, xdrop, N, R, S2, (int)H, sc, si));
    }
    return VD_OK;
  }
  int forward(vd_model* m, hipStream_t s, const float* u0, float** y) {
    VD_TRY(join_stream(m, side_stream(m, s), s));
    u_in.assign(L, nullptr); iqc.assign(L, nullptr); patt.assign(L, nullptr);
    const float* u = u0;
    for (int i = 0; i < L; ++i) {
      const std::string sf = hop_sfx(i);
      float *qc, *u1;
      VD_TRY(ques_common[i].forward(m, s, u, N, false, &qc));                     // mn-att:88
      VD_TRY(ws_get(m, "att.iqc" + sf, (size_t)N * S2 * K, &iqc[i]));
      VD_TRY(ws_get(m, "att.p" + sf, (size_t)N * S2, &patt[i]));
      VD_TRY(ws_get(m, "att.u1" + sf, (size_t)N * H, &u1));
      VD_TRY(vd_img_common_forward_p(pre, m1, xdrop, Wp(m, "img_common" + sf + ".W"), Wp(m, "img_common" + sf + ".b"), qc, m2[i], iqc[i], N, R,
                                     S2, (int)H, (int)K, sc, iflags, s));         // mn-att:83-92
      VD_TRY(vd_img_att_forward_p(iqc[i], Wp(m, "att" + sf + ".W"), Wp(m, "att" + sf + ".b"), pre, m1, u, patt[i], u1, N, R, S2, (int)H,
                                  (int)K, sc, cnt, s));                           // mn-att:93-102
      u_in[i] = u;
      u = u1;
    }
    VD_TRY(drop_mask(m, "u", (size_t)N * H, 0.5f, s, &m_u));
    const float* ud;
    VD_TRY(dropout_fwd(m, "att.u1_d", u, m_u, 2.f, (long)N * H, s, &ud));
    return out.forward(m, s, ud, N, true, y);                                      // mn-att:106
  }
  // round r of every dialog: B rows u0 [B x H], one per image (R = 1 in the row -> image map), `pre` from pass 0; y [B x ldy]
  int forward_round(vd_model* m, hipStream_t s, const float* u0, int B_, float* y, long ldy) {
    const int fl = (m->flags & VD_FLAG_SPLIT9) && vd_img_split_ok((long)B_ * S2, (int)H, (int)K) ? VD_FLAG_SPLIT9 : 0;
    const float* u = u0;
    for (int i = 0; i < L; ++i) {
      const std::string sf = hop_sfx(i);
      float *qc, *iq, *pa, *u1;
      VD_TRY(ws_get(m, "rnd.att.qc" + sf, (size_t)B_ * K, &qc));
      VD_TRY(ws_get(m, "rnd.att.iqc" + sf, (size_t)B_ * S2 * K, &iq));
      VD_TRY(ws_get(m, "rnd.att.p" + sf, (size_t)B_ * S2, &pa));
      VD_TRY(ws_get(m, "rnd.att.u1" + sf, (size_t)B_ * H, &u1));
      VD_TRY(round_linear(m, s, "ques_common" + sf, u, H, H, K, B_, false, qc, K));
      // without dropout the per-round image tensor of a B-row pass IS `pre`
      VD_TRY(vd_img_common_forward_p(pre, nullptr, fl ? pre : nullptr, Wp(m, "img_common" + sf + ".W"), Wp(m, "img_common" + sf + ".b"), qc, nullptr,
                                     iq, B_, 1, S2, (int)H, (int)K, 1.f, fl, s));
      VD_TRY(vd_img_att_forward_p(iq, Wp(m, "att" + sf + ".W"), Wp(m, "att" + sf + ".b"), pre, nullptr, u, pa, u1, B_, 1, S2, (int)H, (int)K, 1.f,
                                  cnt, s));
      u = u1;
    }
    return round_linear(m, s, "out", u, H, H, H, B_, true, y, ldy);
  }
  int backward(vd_model* m, hipStream_t s, BatchSlot& b, const float* grad_out, float** du0) {
    float* du1d;
    VD_TRY(out.backward(m, s, grad_out, true, &du1d));
    const float* dcur;
    VD_TRY(dropout_fwd(m, "att.du1", du1d, m_u, 2.f, (long)N * H, s, &dcur));
    float *dpre, *dscore;
    VD_TRY(ws_get(m, "att.dpre", (size_t)b.B * S2 * H, &dpre));
    VD_TRY(ws_get(m, "att.dscore", (size_t)N * S2, &dscore));
    VD_TRY(vd_memset(dpre, 0, (long)b.B * S2 * H * 4, s));
    for (int i = L - 1; i >= 0; --i) {
      const std::string sf = hop_sfx(i);
      float *dqc, *duq, *dun;
      VD_TRY(ws_get(m, "att.dqc" + sf, (size_t)N * K, &dqc));
      VD_TRY(ws_get(m, "att.du0" + sf, (size_t)N * H, &dun));
      VD_TRY(vd_img_att_backward_p(iqc[i], Wp(m, "att" + sf + ".W"), pre, m1, m2[i], patt[i], dcur, Gp(m, "att" + sf + ".W"),
                                   Gp(m, "att" + sf + ".b"), dqc, dscore, N, R, S2, (int)H, (int)K, sc, cnt, s));   // iqc now holds dz
      // dz is final: what follows on `sw` feeds parameter gradients only (the chain to the text branches continues with dqc)
      hipStream_t sw;
      VD_TRY(wg_fork(m, s, &sw));
      VD_TRY(vd_colsum_acc(iqc[i], K, N * S2, (int)K, Gp(m, "img_common" + sf + ".b"), sw));
      VD_TRY(vd_img_common_wgrad_p(iqc[i], pre, m1, xdrop, Gp(m, "img_common" + sf + ".W"), N, R, S2, (int)H, (int)K, sc, iflags, sw));
      VD_TRY(vd_img_tr_backward_p(iqc[i], Wp(m, "img_common" + sf + ".W"), patt[i], dcur, m1, dpre, N, R, S2, (int)H, (int)K, sc, iflags, sw));
      VD_TRY(ques_common[i].backward(m, s, dqc, true, &duq));
      VD_TRY(vd_axpby(duq, dcur, dun, (long)N * H, 1.f, 1.f, s));                 // residual CAddTable (mn-att:102)
      dcur = dun;
    }
    hipStream_t sw;
    VD_TRY(wg_fork(m, s, &sw));
    VD_TRY(img_proj.backward(m, sw, dpre, false, nullptr));                       // tanh' + dW, db of mn-att:77
    *du0 = const_cast<float*>(dcur);
    return VD_OK;
  }
};

// ------------------------------------------------------------------------------------------------------------
// the four nngraph encoders: mn-att-ques-im-hist, mn-ques-hist, mn-ques-im-hist, lf-att-ques-im-hist
// ------------------------------------------------------------------------------------------------------------
struct GraphEncoder : Encoder {
  bool memory_ = false, san_ = false, qi_ = false, qh_ = false;
  TextBranches text;
  MemoryBlock memory;
  SANBlock san;
  CatLinear qi, qh;
  explicit GraphEncoder(const std::string& name) {
    memory_ = name.rfind("mn", 0) == 0;
    san_ = name.find("att") != std::string::npos;
    qi_ = name == "mn-ques-im-hist";
    qh_ = name == "lf-att-ques-im-hist";
  }
  void declare(vd_model* m) override {
    const long H = m->p.rnnHiddenSize, F = m->p.imgFeatureSize;
    TextBranches::declare(m);
    if (qi_) add_linear(m, "qi", H + F, H);
    if (qh_) add_linear(m, "qh", 2 * H, H);
    if (memory_) MemoryBlock::declare(m);
    if (san_) SANBlock::declare(m);
    text.init(m);
    if (memory_) memory.init(m);
    if (san_) san.init(m);
    if (qi_) qi.init("qi", {H, F}, H);
    if (qh_) qh.init("qh", {H, H}, H);
  }
  int forward(vd_model* m, hipStream_t s, BatchSlot& b, float** out) override {
    const int N = b.q.N;
    if (san_) VD_TRY(san.prefetch(m, s, b, N));
    float *q3, *h3;
    VD_TRY(text.forward(m, s, b, &q3, &h3));
    float* u = nullptr;
    if (qh_) {
      VD_TRY(qh.forward(m, s, {q3, h3}, N, nullptr, 1.f, &u));                     // lf-att:43
    } else {
      const float* query = q3;
      if (qi_) {                                                                   // mn-ques-im-hist.lua:47-48
        float *img_rep, *qp;
        VD_TRY(image_repeat(m, s, b, N, &img_rep));
        VD_TRY(qi.forward(m, s, {q3, img_rep}, N, nullptr, 1.f, &qp));
        query = qp;
      }
      VD_TRY(memory.forward(m, s, query, h3, N, &u));                              // mn-att:48-65
    }
    if (san_) VD_TRY(san.forward(m, s, u, &u));                                    // mn-att:68-106
    *out = out_ = u;
    return VD_OK;
  }
  int forward_round(vd_model* m, hipStream_t s, BatchSlot& b, int r, float** out) override {
    const int N = b.q.N, R = m->p.maxQuesCount, B = N / R;
    const long H = m->p.rnnHiddenSize, F = m->p.imgFeatureSize;
    VD_TRY(round_ready(m, b));
    const float* hl;
    float *hc, *qc;
    VD_TRY(ws_get(m, "h.last", (size_t)N * H, &hc));
    VD_TRY(ws_get(m, "q.last", (size_t)N * H, &qc));
    VD_TRY(history_round(m, s, b, {&text.hist1, &text.hist2}, r, hc, &hl));         // into h.last too: the facts of later rounds
    const float* qr = qc + (long)r * H;                                            // round r of q.last in place: leading dimension R * H
    float* y = out_ + (long)r * H;
    float* u = nullptr;
    if (san_) VD_TRY(ws_get(m, "rnd.u", (size_t)B * H, &u));
    if (qh_) {                                                                     // lf-att:43
      float* cat;
      VD_TRY(ws_get(m, "rnd.qh.cat", (size_t)B * 2 * H, &cat));
      const float* src[2] = {qr, hl};
      const int64_t ld[2] = {(int64_t)R * H, H};
      const int cols[2] = {(int)H, (int)H};
      VD_TRY(vd_rows_cat_p(cat, 2 * H, src, ld, cols, 2, B, s));
      VD_TRY(round_linear(m, s, "qh", cat, 2 * H, 2 * H, H, B, true, san_ ? u : y, san_ ? H : (long)R * H));
    } else {
      const float* query = qr;
      long q_ld = (long)R * H;
      if (qi_) {                                                                   // mn-ques-im-hist.lua:47-48, on the image rows directly
        float *cat, *qp;
        VD_TRY(ws_get(m, "rnd.qi.cat", (size_t)B * (H + F), &cat));
        VD_TRY(ws_get(m, "rnd.qi.y", (size_t)B * H, &qp));
        const float* src[2] = {qr, b.img};
        const int64_t ld[2] = {(int64_t)R * H, F};
        const int cols[2] = {(int)H, (int)F};
        VD_TRY(vd_rows_cat_p(cat, H + F, src, ld, cols, 2, B, s));
        VD_TRY(round_linear(m, s, "qi", cat, H + F, H + F, H, B, true, qp, H));
        query = qp;
        q_ld = H;
      }
      VD_TRY(memory.forward_round(m, s, query, q_ld, hc, B, r, san_ ? u : y, san_ ? H : (long)R * H));
    }
    if (san_) VD_TRY(san.forward_round(m, s, u, B, y, (long)R * H));
    *out = out_;
    return VD_OK;
  }
  int backward(vd_model* m, hipStream_t s, BatchSlot& b, const float* grad_out) override {
    const float* du = grad_out;
    if (san_) {
      float* t;
      VD_TRY(san.backward(m, s, b, grad_out, &t));
      du = t;
    }
    const float *dq3, *dh3;
    if (qh_) {
      std::vector<float*> g;
      VD_TRY(qh.backward(m, s, du, {}, &g));
      dq3 = g[0];
      dh3 = g[1];
    } else {
      float *dquery, *dh;
      VD_TRY(memory.backward(m, s, du, &dquery, &dh));
      dq3 = dquery;
      dh3 = dh;
      if (qi_) {
        std::vector<float*> g;
        VD_TRY(qi.backward(m, s, dquery, {true, false}, &g));
        dq3 = g[0];
      }
    }
    return text.backward(m, s, b, dq3, dh3);
  }
};

// ------------------------------------------------------------------------------------------------------------
// Late fusion (encoders/lf-ques.lua, lf-ques-im.lua, lf-ques-hist.lua, lf-ques-im-hist.lua):
//   [quesLSTM last step ; img ; histLSTM last step] -> Dropout(p) -> Linear(., H) -> Tanh
// ------------------------------------------------------------------------------------------------------------
struct LateFusion : Encoder {
  bool use_im, use_hist;
  std::vector<SeqLSTM> rnn;
  HistoryBranch hist;
  CatLinear fuse;
  long E = 0, H = 0, F = 0;
  float pdrop = 0.5f;
  LateFusion(bool im, bool hs) : use_im(im), use_hist(hs) {}
  void declare(vd_model* m) override {
    E = m->p.embedSize; H = m->p.rnnHiddenSize; F = m->p.imgFeatureSize; pdrop = m->p.dropout;
    const int L = m->p.numLayers;
    rnn.resize(L);
    for (int l = 0; l < L; ++l) {
      add_lstm(m, "ques" + std::to_string(l + 1), l == 0 ? E : H, H);              // lf-ques-im-hist.lua:19-26
      rnn[l].init("ques" + std::to_string(l + 1), l == 0 ? E : H, H);
    }
    if (use_hist) hist.declare(m);                                                 // :38-45
    std::vector<long> dims = {H};
    if (use_im) dims.push_back(F);
    if (use_hist) dims.push_back(H);
    long D = 0;
    for (long d : dims) D += d;
    add_linear(m, "fuse", D, H);                                                   // :58
    fuse.init("fuse", dims, H);
  }
  std::vector<SeqLSTM>* rnnLayers() override { return &rnn; }
  int forward(vd_model* m, hipStream_t s, BatchSlot& b, float** out) override {
    const int N = b.q.N, Tq = b.q.T;
    hipStream_t sh = side_stream(m, s);
    float* hh_last = nullptr;
    if (use_hist) {
      VD_TRY(fork_stream(m, s, sh));
      const bool prof = m->dec_name == "gen";     // (disc pairs: ev_prof belongs to the option-LSTM families)
      if (prof) VD_HIP(hipEventRecord(m->ev_prof[0], sh));
      VD_TRY(hist.forward(m, sh, b, &hh_last));
      if (prof) VD_HIP(hipEventRecord(m->ev_prof[1], sh));
    }
    float *qx, *qt;
    VD_TRY(ws_get(m, "q.x", (size_t)Tq * N * E, &qx));
    VD_TRY(vd_embed_gather(Wp(m, "embed"), b.q.tok, nullptr, qx, (long)Tq * N, (int)E, 1.f, s));
    VD_TRY(lstm_stack_forward(m, s, rnn, {qx}, Tq, N, b.q.tok, &qt));
    std::vector<const float*> parts = {rnn.back().out_at(Tq - 1)};
    if (use_im) {
      float* img_rep;
      VD_TRY(image_repeat(m, s, b, N, &img_rep));
      parts.push_back(img_rep);
    }
    if (use_hist) {
      VD_TRY(join_stream(m, sh, s));
      parts.push_back(hh_last);
    }
    uint8_t* mk;
    VD_TRY(drop_mask(m, "fuse", (size_t)N * fuse.D, pdrop, s, &mk));
    VD_TRY(fuse.forward(m, s, parts, N, mk, pdrop > 0.f ? 1.f / (1.f - pdrop) : 1.f, out));
    out_ = *out;
    return VD_OK;
  }
  int forward_round(vd_model* m, hipStream_t s, BatchSlot& b, int r, float** out) override {
    const int N = b.q.N, Tq = b.q.T, R = m->p.maxQuesCount, B = N / R;
    VD_TRY(round_ready(m, b, use_hist));
    const float* hl;
    float* hc = nullptr;                                                           // (the h.last cache exists on the wavefront path only)
    if (hist.waved(b)) VD_TRY(ws_get(m, "h.last", (size_t)N * H, &hc));
    VD_TRY(hist.round(m, s, b, r, hc, &hl));
    // [question state of round r ; image ; history state] gathered by the join itself, then Linear + Tanh into the output rows
    float* cat;
    VD_TRY(ws_get(m, "rnd.fuse.cat", (size_t)B * fuse.D, &cat));
    const float* src[3] = {rnn.back().out_at(Tq - 1) + (long)r * H, use_im ? b.img : hl, hl};
    const int64_t ld[3] = {(int64_t)R * H, use_im ? F : H, H};
    const int cols[3] = {(int)H, (int)(use_im ? F : H), (int)H};
    VD_TRY(vd_rows_cat_p(cat, fuse.D, src, ld, cols, use_im ? 3 : 2, B, s));
    VD_TRY(round_linear(m, s, "fuse", cat, fuse.D, fuse.D, H, B, true, out_ + (long)r * H, (long)R * H));
    *out = out_;
    return VD_OK;
  }
  int backward(vd_model* m, hipStream_t s, BatchSlot& b, const float* grad_out) override {
    std::vector<bool> need = {true};
    if (use_im) need.push_back(false);
    if (use_hist) need.push_back(true);
    std::vector<float*> g;
    VD_TRY(fuse.backward(m, s, grad_out, need, &g));
    hipStream_t sh = side_stream(m, s);
    if (use_hist) {
      VD_TRY(fork_stream(m, s, sh));
      const bool prof = m->dec_name == "gen";
      if (prof) VD_HIP(hipEventRecord(m->ev_prof[2], sh));
      VD_TRY(hist.backward(m, sh, b, g.back()));
      if (prof) VD_HIP(hipEventRecord(m->ev_prof[3], sh));
      m->prof_hist = prof;
    }
    std::vector<float*> dx;
    VD_TRY(lstm_stack_backward(m, s, rnn, g[0], nullptr, &dx));
    VD_TRY(vd_embed_scatter_acc(Gp(m, "embed"), b.q.tok, nullptr, dx[0], (long)b.q.T * b.q.N, (int)E, 1.f, s));
    if (use_hist) VD_TRY(join_stream(m, sh, s));
    return VD_OK;
  }
};

// ------------------------------------------------------------------------------------------------------------
// Hierarchical recurrent encoders (encoders/hre-ques-hist.lua, hre-ques-im-hist.lua, hrea-ques-im-hist.lua)
// ------------------------------------------------------------------------------------------------------------
struct Hre : Encoder {
  bool use_im, attention;
  std::vector<SeqLSTM> rnn;
  HistoryBranch hist;
  SeqLSTM dialog;
  Linear img_embed;
  long E = 0, H = 0, F = 0, DI = 0;
  int R = 0;
  float *hh = nullptr, *hq = nullptr, *sq = nullptr, *sh_ = nullptr, *P = nullptr;
  uint8_t* m_img = nullptr;
  Hre(bool im, bool att) : use_im(im), attention(att) {}
  void declare(vd_model* m) override {
    E = m->p.embedSize; H = m->p.rnnHiddenSize; F = m->p.imgFeatureSize; DI = use_im ? m->p.imgEmbedSize : 0; R = m->p.maxQuesCount;
    const int L = m->p.numLayers;
    rnn.resize(L);
    hist.declare(m);
    if (use_im) {
      add_linear(m, "img_embed", F, DI);
      img_embed.init("img_embed", F, DI);
    }
    for (int l = 0; l < L; ++l) {
      const long D = l == 0 ? E + DI : H;
      add_lstm(m, "ques" + std::to_string(l + 1), D, H);
      rnn[l].init("ques" + std::to_string(l + 1), D, H, (l == 0 && use_im) ? std::vector<long>{E, DI} : std::vector<long>{});
    }
    if (attention) {
      add_linear(m, "att_q", H, 1);
      add_linear(m, "att_h", H, 1);
    }
    add_lstm(m, "dialog", 2 * H, H);
    dialog.init("dialog", 2 * H, H, {H, H});
  }
  std::vector<SeqLSTM>* rnnLayers() override { return &rnn; }
  // round-major <-> dialog-major row permutations (nn.View + nn.Transpose({1,2}), hre:88-93)
  int indices(vd_model* m, int N, int32_t** to_rb, int32_t** to_n) {
    const int B = N / R;
    std::vector<int32_t> a(N), c(N);
    for (int n = 0; n < N; ++n) {
      a[n] = (n % B) * R + n / B;   // row r*B+b  <- n = b*R + r
      c[n] = (n % R) * B + n / R;   // row b*R+r  <- r*B + b
    }
    VD_TRY(index_array(m, "idx.to_rb." + std::to_string(N), a, to_rb));
    return index_array(m, "idx.to_n." + std::to_string(N), c, to_n);
  }
  int forward(vd_model* m, hipStream_t s, BatchSlot& b, float** out) override {
    const int N = b.q.N, Tq = b.q.T, B = N / R;
    int32_t *to_rb, *to_n;
    VD_TRY(indices(m, N, &to_rb, &to_n));
    hipStream_t sh = side_stream(m, s);
    VD_TRY(fork_stream(m, s, sh));
    VD_TRY(hist.forward(m, sh, b, &hh));
    float* qx;
    VD_TRY(ws_get(m, "q.x", (size_t)Tq * N * E, &qx));
    VD_TRY(vd_embed_gather(Wp(m, "embed"), b.q.tok, nullptr, qx, (long)Tq * N, (int)E, 1.f, s));
    std::vector<const float*> x = {qx};
    if (use_im) {
      float *img_rep, *imgE, *xi;
      VD_TRY(image_repeat(m, s, b, N, &img_rep));
      m_img = nullptr;
      if (attention) VD_TRY(drop_mask(m, "img", (size_t)N * F, 0.5f, s, &m_img));          // hrea:47
      const float* img_in;
      VD_TRY(dropout_fwd(m, "img.in", img_rep, m_img, 2.f, (long)N * F, s, &img_in));
      VD_TRY(img_embed.forward(m, s, img_in, N, false, &imgE));                           // hre:43-48
      VD_TRY(ws_get(m, "q.ximg", (size_t)Tq * N * DI, &xi));
      VD_TRY(vd_mask_time_forward(imgE, b.q.tok, xi, Tq, N, (int)DI, s));                 // MaskTime hre:50-53
      x.push_back(xi);
    }
    float* qt;
    VD_TRY(lstm_stack_forward(m, s, rnn, x, Tq, N, b.q.tok, &qt));
    hq = rnn.back().out_at(Tq - 1);
    VD_TRY(join_stream(m, sh, s));
    const float *first = hq, *second = hh;
    if (attention) {                                                                       // hrea:83-131
      float* att;
      VD_TRY(ws_get(m, "hrea.sq", (size_t)N, &sq));
      VD_TRY(ws_get(m, "hrea.sh", (size_t)N, &sh_));
      VD_TRY(ws_get(m, "hrea.P", (size_t)N * R, &P));
      VD_TRY(ws_get(m, "hrea.att", (size_t)N * H, &att));
      VD_TRY(vd_rowdot_forward(hq, Wp(m, "att_q.W"), Wp(m, "att_q.b"), sq, N, (int)H, s));
      VD_TRY(vd_rowdot_forward(hh, Wp(m, "att_h.W"), Wp(m, "att_h.b"), sh_, N, (int)H, s));
      VD_TRY(vd_hrea_attention_forward(sq, sh_, hh, P, att, B, R, (int)H, s));
      first = att;                                                                         // concat4: {att, ques}
      second = hq;
    }
    float *f_rb, *s_rb, *d, *o;
    VD_TRY(ws_get(m, "hre.f_rb", (size_t)N * H, &f_rb));
    VD_TRY(ws_get(m, "hre.s_rb", (size_t)N * H, &s_rb));
    VD_TRY(ws_get(m, "hre.out", (size_t)N * H, &o));
    VD_TRY(vd_embed_gather(first, to_rb, nullptr, f_rb, N, (int)H, 1.f, s));
    VD_TRY(vd_embed_gather(second, to_rb, nullptr, s_rb, N, (int)H, 1.f, s));
    VD_TRY(dialog.forward(m, s, {f_rb, s_rb}, R, B, nullptr, &d));                        // hre:90-94 (no maskZero)
    VD_TRY(vd_embed_gather(d, to_n, nullptr, o, N, (int)H, 1.f, s));
    *out = out_ = o;
    return VD_OK;
  }
  int forward_round(vd_model* m, hipStream_t s, BatchSlot& b, int r, float** out) override {
    const int N = b.q.N, B = N / R;
    VD_TRY(round_ready(m, b, hh && hq && dialog.T == R && dialog.N == B));
    const float* hl;
    VD_TRY(hist.round(m, s, b, r, hh, &hl));                                        // into hh too: hrea attends over it in later rounds
    const float *first = hq + (long)r * H, *second = hl;                           // round r of the question state in place
    long ld1 = (long)R * H, ld2 = H;
    if (attention) {                                                               // hrea:83-131; sq is pass 0's, sh of the new rows is not
      float* att;
      VD_TRY(ws_get(m, "rnd.hrea.att", (size_t)B * H, &att));
      VD_TRY(vd_rowdot_forward(hh, Wp(m, "att_h.W"), Wp(m, "att_h.b"), sh_, N, (int)H, s));
      VD_TRY(vd_hrea_attention_round_p(sq, sh_, hh, nullptr, att, B, R, r, (int)H, s));
      second = first; ld2 = ld1;                                                   // concat4: {att, ques}
      first = att; ld1 = H;
    }
    // ONE step of the dialog LSTM from its step r - 1 state, written in place as step r of pass 0's step-major buffers
    float* g = dialog.gates + (long)r * B * 4 * H;
    VD_TRY(vd_gemm_nn(first, ld1, dialog.Wx(m), 4 * H, Wp(m, "dialog.b"), g, 4 * H, B, (int)(4 * H), (int)H, 0, s));
    VD_TRY(vd_gemm_nn(second, ld2, dialog.Wx(m) + H * 4 * H, 4 * H, nullptr, g, 4 * H, B, (int)(4 * H), (int)H, 1, s));
    VD_TRY(vd_lstm_forward(g, (int64_t)B * 4 * H, 4 * H, nullptr, nullptr, dialog.Wh(m), dialog.out_at(r - 1), dialog.cell_at(r - 1), g,
                           dialog.out_at(r), dialog.cell_at(r), 1, B, (int)H, 0, s));
    VD_TRY(rows_copy(out_ + (long)r * H, (long)R * H, dialog.out_at(r), H, B, (int)H, s));
    *out = out_;
    return VD_OK;
  }
  int backward(vd_model* m, hipStream_t s, BatchSlot& b, const float* grad_out) override {
    const int N = b.q.N, Tq = b.q.T, B = N / R;
    int32_t *to_rb, *to_n;
    VD_TRY(indices(m, N, &to_rb, &to_n));
    float *g_rb, *dfirst, *dsecond;
    VD_TRY(ws_get(m, "hre.g_rb", (size_t)N * H, &g_rb));
    VD_TRY(ws_get(m, "hre.dfirst", (size_t)N * H, &dfirst));
    VD_TRY(ws_get(m, "hre.dsecond", (size_t)N * H, &dsecond));
    VD_TRY(vd_embed_gather(grad_out, to_rb, nullptr, g_rb, N, (int)H, 1.f, s));
    std::vector<float*> dd;
    VD_TRY(dialog.backward(m, s, g_rb, nullptr, {}, &dd));
    VD_TRY(vd_embed_gather(dd[0], to_n, nullptr, dfirst, N, (int)H, 1.f, s));
    VD_TRY(vd_embed_gather(dd[1], to_n, nullptr, dsecond, N, (int)H, 1.f, s));
    const float *dq = dfirst, *dh = dsecond;
    if (attention) {
      float *dsq, *dsh, *dh_att, *dq_s, *dh_s, *dqq, *dhh;
      VD_TRY(ws_get(m, "hrea.dsq", (size_t)N, &dsq));
      VD_TRY(ws_get(m, "hrea.dsh", (size_t)N, &dsh));
      VD_TRY(ws_get(m, "hrea.dh", (size_t)N * H, &dh_att));
      VD_TRY(ws_get(m, "hrea.dq_s", (size_t)N * H, &dq_s));
      VD_TRY(ws_get(m, "hrea.dh_s", (size_t)N * H, &dh_s));
      VD_TRY(ws_get(m, "hrea.dq", (size_t)N * H, &dqq));
      VD_TRY(ws_get(m, "hrea.dhh", (size_t)N * H, &dhh));
      VD_TRY(vd_hrea_attention_backward(hh, P, dfirst, dsq, dsh, dh_att, B, R, (int)H, s));
      VD_TRY(vd_rowdot_backward(hq, Wp(m, "att_q.W"), dsq, Gp(m, "att_q.W"), Gp(m, "att_q.b"), dq_s, N, (int)H, s));
      VD_TRY(vd_rowdot_backward(hh, Wp(m, "att_h.W"), dsh, Gp(m, "att_h.W"), Gp(m, "att_h.b"), dh_s, N, (int)H, s));
      VD_TRY(vd_axpby(dsecond, dq_s, dqq, (long)N * H, 1.f, 1.f, s));
      VD_TRY(vd_axpby(dh_att, dh_s, dhh, (long)N * H, 1.f, 1.f, s));
      dq = dqq;
      dh = dhh;
    }
    hipStream_t sh = side_stream(m, s);
    VD_TRY(fork_stream(m, s, sh));
    VD_TRY(hist.backward(m, sh, b, dh));
    std::vector<float*> dx;
    VD_TRY(lstm_stack_backward(m, s, rnn, dq, nullptr, &dx));
    // the two scatters into the shared embedding gradient use float atomics: concurrent streams are fine
    VD_TRY(vd_embed_scatter_acc(Gp(m, "embed"), b.q.tok, nullptr, dx[0], (long)Tq * N, (int)E, 1.f, s));
    if (use_im) {
      float* dimgE;
      VD_TRY(ws_get(m, "q.dimgE", (size_t)N * DI, &dimgE));
      VD_TRY(vd_mask_time_backward(dx[1], b.q.tok, dimgE, Tq, N, (int)DI, s));
      // (hrea: the Dropout in front of the image Linear only scales its input; its gradient is not needed)
      VD_TRY(img_embed.backward(m, s, dimgE, false, nullptr));
    }
    return join_stream(m, sh, s);
  }
};

inline std::unique_ptr<Encoder> make_encoder(const std::string& n) {
  if (n == "mn-att-ques-im-hist" || n == "mn-ques-hist" || n == "mn-ques-im-hist" || n == "lf-att-ques-im-hist")
    return std::unique_ptr<Encoder>(new GraphEncoder(n));
  if (n == "lf-ques") return std::unique_ptr<Encoder>(new LateFusion(false, false));
  if (n == "lf-ques-im") return std::unique_ptr<Encoder>(new LateFusion(true, false));
  if (n == "lf-ques-hist") return std::unique_ptr<Encoder>(new LateFusion(false, true));
  if (n == "lf-ques-im-hist") return std::unique_ptr<Encoder>(new LateFusion(true, true));
  if (n == "hre-ques-hist") return std::unique_ptr<Encoder>(new Hre(false, false));
  if (n == "hre-ques-im-hist") return std::unique_ptr<Encoder>(new Hre(true, false));
  if (n == "hrea-ques-im-hist") return std::unique_ptr<Encoder>(new Hre(true, true));
  return nullptr;
}

}  // namespace vdrt
