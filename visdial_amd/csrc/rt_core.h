// Native step runtime, part 1: the model object, memory / stream helpers and the host-side building blocks
// (nn.Linear, CatLinear, nn.SeqLSTM with its hand-off fields, LSTM stacks).  Included by runtime.hip only.
//
// The building blocks mirror the Python host one to one (visdial_amd/nn.py, encoders/_blocks.py): they own no
// arithmetic -- every forward / backward is an ordered list of operator-level launches of this same library -- only
// buffers, shapes and launch order.  The parity tests pin both hosts against the same oracle.
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "../../include/visdial_hip.h"
#include "common.h"
#include "paths.h"
#include "rt_switches.h"
#include "wgrad_plan.h"

static_assert(VD_OK == 0 && VD_ERR_ARG == -1, "rt_switches.h returns the two as literals: it includes no common.h");

// lstm.hip: the two-layer wavefront with the pass's arithmetic (flags & VD_FLAG_BF16: bf16 operands on the ticks' MFMAs in a bf16 pass;
// the C-ABI entry points vd_lstm2_forward / vd_lstm2_backward are these with flags = 0)
int vd_lstm2_forward_p(const vd_lstm2_fwd_t* st, int nstacks, int H, int flags, hipStream_t stream);
int vd_lstm2_backward_p(const vd_lstm2_bwd_t* st, int nstacks, int H, int flags, hipStream_t stream);

// attention.hip: the image attention's dense products with a pass's arithmetic (flags & VD_FLAG_SPLIT9: on the exact split, from the
// materialised dropped image tensor `xdrop`; else the C-ABI entry points)
int vd_img_drop_gather(const float* pre, const uint8_t* mask1, float* xdrop, int N, int R, int S2, int H, float scale, hipStream_t stream);
int vd_img_common_forward_p(const float* pre, const uint8_t* mask1, const float* xdrop, const float* Wc, const float* bc, const float* qc,
                            const uint8_t* mask2, float* iqc, int N, int R, int S2, int H, int Kc, float scale, int flags, hipStream_t stream);
int vd_img_tr_backward_p(const float* dz, const float* Wc, const float* p, const float* datt, const uint8_t* mask1, float* dpre, int N, int R,
                         int S2, int H, int Kc, float scale, int flags, hipStream_t stream);
int vd_img_common_wgrad_p(const float* dz, const float* pre, const uint8_t* mask1, const float* xdrop, float* dWc, int N, int R, int S2, int H,
                          int Kc, float scale, int flags, hipStream_t stream);

// attention.hip: the attention head over the live regions of every image (IR1 - IR6).  cnt [ceil(N / R)] int32 on the device: round n attends
// the first cnt[n / R] regions of its image and writes exact zeros for the rest; cnt = null is vd_img_att_forward / vd_img_att_backward,
// argument for argument
int vd_img_att_forward_p(const float* iqc, const float* wa, const float* ba, const float* pre, const uint8_t* mask1, const float* u0, float* p,
                         float* u1, int N, int R, int S2, int H, int Kc, float scale, const int32_t* cnt, hipStream_t stream);
int vd_img_att_backward_p(float* iqc_dz, const float* wa, const float* pre, const uint8_t* mask1, const uint8_t* mask2, const float* p,
                          const float* datt, float* dwa, float* dba, float* dqc, float* work, int N, int R, int S2, int H, int Kc, float scale,
                          const int32_t* cnt, hipStream_t stream);

// attention.hip: one round of a rollout (VD_ROLLOUT_ENCODER = round; rt_encoders.h forward_round).  Row (d, r) of vd_mn_attention_forward /
// vd_hrea_attention_forward under the causal mask, bit for bit, from facts (d, 0 .. r) alone: hAtt / att [B x H] and P [B x R] (or null) are
// compact.  The memory query of dialog d is row d of Q [B x q_ld] (q_ld = R * H reads round r of a per-round tensor in place); Qout [B x H]
// or null receives it compact.
int vd_mn_attention_round_p(const float* Q, int64_t q_ld, const float* Hm, float* P, float* hAtt, float* Qout, int B, int R, int r, int H,
                            hipStream_t stream);
int vd_hrea_attention_round_p(const float* sq, const float* sh, const float* Hm, float* P, float* att, int B, int R, int r, int H,
                              hipStream_t stream);
// row r of every dialog of the step-major tokens tok [T x N] (N = B * R) as a B-row sequence tok_r [T x B], with its embedding rows x [T*B x E]
int vd_round_embed_p(const float* emb, const int32_t* tok, int T, int N, int R, int r, int32_t* tok_r, float* x, int E, hipStream_t stream);
// dst [rows x sum(cols)] (leading dimension dst_ld) = up to three column blocks src[i] [rows x cols[i]] (leading dimension ld[i]) side by side;
// one block with a strided source / destination is the gather / scatter of a round's rows
int vd_rows_cat_p(float* dst, int64_t dst_ld, const float* const* src, const int64_t* ld, const int* cols, int nparts, int64_t rows,
                  hipStream_t stream);

// gemm_ops.hip: vd_gemm_nn over rows that carry a token id, with the row-group predicate of VD_FLAG_LIVE_PREFIX -- a row tile of
// `row_tile` (32 or 128) rows whose first row has tok_mask == 0 is not computed and its C rows are left unwritten
int vd_gemm_nn_live_p(const float* A, int64_t lda, const float* B, int64_t ldb, const float* bias, float* C, int64_t ldc, int M, int N, int K,
                      const int32_t* tok_mask, int row_tile, hipStream_t stream);
// lhood.hip: the length order of a chunk of candidates (stable counting sort, descending length), the tokens / targets / replication
// index gathered in that order, and vd_lhood_sum with the scores scattered back through `perm`
int vd_lhood_order_p(const int32_t* tok_in, const int32_t* target, int T, int64_t rows, int C, int32_t* perm, int32_t* rep, int32_t* tok_in_s,
                     int32_t* target_s, int32_t* work, int32_t* info, hipStream_t stream);
int64_t vd_lhood_order_work_ints(int T, int64_t rows);
int vd_lhood_sum_p(const float* nll, const int32_t* act, int64_t n_act, int T, int64_t rows, int C, const int32_t* perm, float* out, int64_t ldo,
                   hipStream_t stream);

// lhood.hip, prefix-tree head (VD_LHOOD_TREE): the log-sum-exp of the listed rows of h (the kernels of vd_lhood_nll without a target), and
// every candidate's score as the sum over its (node, target) edges, in step order, written in candidate order
int vd_lhood_lse_p(const float* h, int64_t ldh, int64_t rows, const int32_t* act, int64_t n_act, const float* W, int64_t ldw, const float* bias,
                   int V, int H, float* lse, hipStream_t stream);
int vd_lhood_edge_sum_p(const float* h, int64_t ldh, const int32_t* node_row, const float* lse, const int32_t* enode, const int32_t* etgt, int T,
                        int64_t rows, int C, const float* W, int64_t ldw, const float* bias, int H, float* out, int64_t ldo, hipStream_t stream);

// sample.hip: vd_sample_draw over the top-k / nucleus kept set (VD_SAMPLE_TOPK / VD_SAMPLE_TOPP; the rule is sample.hip's header T1-T4)
int vd_sample_draw_trunc_p(const float* logits, int64_t ld, int64_t rows, int V, int32_t* tok, const double* uniforms, double temperature,
                           int top_k, double top_p, int step, int beam_len, int end_token, int32_t* hist, double* loglik, int32_t* status,
                           hipStream_t stream);

// beam.hip: vd_beam_advance with the knobs of the search.  `rounds` rounds of k slots in G >= 1 groups (VD_BEAM_GROUPS / VD_BEAM_DIVERSITY;
// the rule is beam.hip's header D1-D7): group g of a round owns slots g k/G .. , G divides k, lambda is finite and >= 0 (unused at G = 1);
// best_score / best_len / best_hist are [rounds x G].  lp (VD_BEAM_LENGTH_PENALTY, C6 there): the best finished candidate is replaced
// across steps by x.score * lp[y.len] > y.score * lp[x.len], lp [beam_len] on the device, lp[s] = s^alpha computed on the host in fp64;
// nullptr = off.  vd_beam_advance is G = 1, lambda = 0, lp = nullptr.
int vd_beam_advance_p(const int32_t* top_idx, const float* top_val, int rounds, int k, int G, float lambda, int step, int beam_len,
                      int end_token, double* scores, const int32_t* hist_in, int32_t* hist_out, int32_t* src, int32_t* next_tok,
                      double* best_score, int32_t* best_len, int32_t* best_hist, const double* lp, hipStream_t stream);
// beam.hip: vd_beam_topk with the words banned that minimum length and n-gram blocking ban for the row's column (VD_BEAM_MIN_LEN /
// VD_BEAM_NO_REPEAT; C1-C4 there), read from the PRE-advance history `hist` [rows x beam_len] at `step`; needs V >= k + beam_len - 1, and
// beam_len <= VD_BEAM_LMAX while no_repeat >= 1
int vd_beam_topk_ban_p(const float* logits, int64_t ld, int64_t rows, int V, const int32_t* tok, int k, const int32_t* hist, int beam_len,
                       int step, int min_len, int no_repeat, int end_token, int32_t* top_idx, float* top_val, hipStream_t stream);

// beam.hip: one pass of a rollout (VD_BEAM_ROLLOUT; R2 / R3 there): history row r + 1 of every dialog (row dialog * R + r + 1 of the
// step-major tokens hist_tok [Th x dialogs * R]) = the non-zero tokens of question row r (ques, step-major [Tq x dialogs * R]), then the
// words of answers [dialogs x beam_len] that fit, right-aligned.  hist_sorted / inv: the length-sorted copy [Th x N] and the place of
// every row in it, both or neither.  Needs r + 1 < R and Tq <= Th.
int vd_beam_rollout_append_p(const int32_t* answers, int beam_len, int end_token, const int32_t* ques, int Tq, int dialogs, int R, int r,
                             int32_t* hist_tok, int32_t* hist_sorted, const int32_t* inv, int Th, hipStream_t stream, int concat_end = 0);
// beam.hip: one pass of a discriminative rollout (VD_RETRIEVE_ROLLOUT; E2 - E4 there): history row r + 1 of every dialog = the non-zero tokens
// of question row r, then the words that fit of the candidate that ranks first among scores row dialog * R + r ([dialogs * R x O], O <= 128:
// the highest score, ties to the lowest index), right-aligned.  The candidate's tokens are read from opt_tok, step-major [To x opt_rows], at
// row opt_uid[candidate] (the de-duplicated upload) or, with opt_uid == nullptr, at the candidate's own row (opt_rows = dialogs * R * O);
// its words end at the first 0.  ques / hist_tok / hist_sorted / inv / Tq / Th as above.
int vd_disc_rollout_pick_p(const float* scores, int O, const int32_t* opt_tok, int64_t opt_rows, int To, const int32_t* opt_uid,
                           const int32_t* ques, int Tq, int dialogs, int R, int r, int32_t* hist_tok, int32_t* hist_sorted,
                           const int32_t* inv, int Th, hipStream_t stream, int concat_end = 0);
// concat_end != 0 (both; VD_ROLLOUT_CONCAT_END, CH1 - CH6 there): the <END> id; row r + 1 = ROW r's tokens, <END>, the question's non-zero tokens
// and the words, cut at the end where they do not fit Th columns, right-aligned.  0: the per-round row described above.
// beam.hip: the round pass of a concatenated history (CH6): win [Wn x dialogs], step-major, = the last first(r - 1) - first(r) columns of
// history row r of every dialog (the new tokens CH4 kept), right-aligned with zeros in front.  1 <= r < R, 1 <= Wn <= W.
int vd_rollout_concat_window_p(const int32_t* hist_tok, int dialogs, int R, int r, int W, int Wn, int32_t* win, hipStream_t stream);

// loss.hip: the two training heads on targets smoothed by `smooth` in [0, 1) (VD_LABEL_SMOOTHING; LS1 - LS4 there): vd_score_ce /
// vd_logsoftmax_nll with t = (1 - smooth) onehot + smooth / K in the place of onehot (K = O options / V valid columns).  smooth = 0 IS the
// C-ABI entry point: the same kernel with the same arguments.  The smoothed vd_score_ce_p needs gt and loss_rows.
int vd_score_ce_p(const float* optH, const float* enc, const int32_t* gt, float* scores, float* loss_rows, float* dOptH, float* dEnc, int N,
                  int O, int H, float gscale, float smooth, hipStream_t stream);
int vd_logsoftmax_nll_p(float* logits, int64_t ld, int64_t rows, int V, const int32_t* tok_in, const int32_t* target, float* loss_rows,
                        int write_grad, float smooth, hipStream_t stream);
// loss.hip: the discriminative training head on dense relevance targets (DT3 / DT4 there): rel [N x O] holds DT1's rows, mix is mu, gscale is
// 1 / W; loss_rows[n] = w_n loss_n.  vd_ndcg_p: DT2, one double per round (-1: no relevant candidate, -2: not annotated).
int vd_score_ce_dense_p(const float* optH, const float* enc, const int32_t* gt, const float* rel, float* scores, float* loss_rows,
                        float* dOptH, float* dEnc, int N, int O, int H, float gscale, float mix, hipStream_t stream);
int vd_ndcg_p(const float* scores, const float* rel, double* ndcg, int N, int O, hipStream_t stream);
// loss.hip: a live dense step (DL1 - DL5 there).  vd_dense_live_tokens_p: the option tokens of the live rounds, out [To x n_live * O] from
// the uploaded tok [To x rows], through uid [N * O] where the upload de-duplicated (or null); live_idx [n_live] ascending, on the device.
// vd_score_ce_dense_live_p: vd_score_ce_dense_p over all N rounds with optH / dOptH [n_live * O x H] holding the live rounds' rows;
// live_slot [N] (device) = a round's place among the live rounds or -1, whose scores, loss and dEnc row come back 0.
int vd_dense_live_tokens_p(const int32_t* tok, int64_t rows, int To, const int32_t* uid, const int32_t* live_idx, int n_live, int O,
                           int32_t* out, hipStream_t stream);
int vd_score_ce_dense_live_p(const float* optH, const float* enc, const int32_t* gt, const float* rel, const int32_t* live_slot, float* scores,
                             float* loss_rows, float* dOptH, float* dEnc, int N, int O, int H, float gscale, float mix, hipStream_t stream);
// elementwise.hip: the update with a global-norm clip and decoupled weight decay (VD_GRAD_CLIP_NORM / VD_WEIGHT_DECAY; GC1 - GC3, WD1
// there).  vd_grad_clip_scale_p: work[0] = c / || gscale g ||_2 where that norm is finite and > c > 0, else 1; work[1] = the norm; two
// launches on `stream`, no atomic, no host read, the same bits on every run; work holds vd_clip_work_floats() floats.
// vd_clip_decay_adam_p: vd_clamp_adam on gscale * scale_dev[0] * g (scale_dev null: 1), then w -= decay * w_old.
int64_t vd_clip_work_floats();
int vd_grad_clip_scale_p(const float* g, int64_t n, float gscale, float c, float* work, hipStream_t stream);
int vd_clip_decay_adam_p(float* w, float* g, float* m, float* v, int64_t n, float gscale, float clip, float beta1, float beta2, float eps,
                         float step, const float* scale_dev, float decay, hipStream_t stream);

#define VD_TRY(expr)                  \
  do {                                \
    const int rc__ = (expr);          \
    if (rc__ != VD_OK) return rc__;   \
  } while (0)

namespace vdrt {

struct Tensor {
  std::string name;
  long off, rows, cols;
  int kind;  // 0 embed, 1 lstm weight, 2 lstm bias, 3 linear weight, 4 linear bias
  long numel() const { return rows * cols; }
};

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

// time-major [T x N] token matrix on the device (+ length-sort metadata for the nngraph encoders' text branches)
struct SeqTok {
  int T = 0, N = 0;
  bool present = false, sorted = false;
  int32_t* tok = nullptr;
  std::vector<int32_t> nact;  // host [T]
  int32_t *tok_sorted = nullptr, *fwd_idx = nullptr, *inv_idx = nullptr, *perm = nullptr, *inv = nullptr, *nact_dev = nullptr;
  // the non-pad (t, row) pairs as linear row indices of the sorted [T*N x .] tensors, in step order; act1 / prev1 =
  // the pairs with t >= 1 and their previous-step rows (weight gradients contract these only)
  int32_t *act = nullptr, *act1 = nullptr, *prev1 = nullptr;
  int n_act = 0, n_act1 = 0;
  // the same pairs as segments of whole k-steps (wgrad_plan.h), [0]: the pairs of one step, [1]: (t - 1, t) pairs; host copy + device table
  std::vector<vdplan::Seg> seg_host[2];
  int32_t* seg_dev[2] = {nullptr, nullptr};
  int seg_ksteps[2] = {0, 0};
};

// Prefix tree of a chunk of candidates (generative retrieval with VD_LHOOD_TREE; built on the host at upload time, runtime.hip): the
// candidates of options [o0, o0 + C) of every round as a forest over the rounds' encoder states.  Nodes are numbered level-major; a
// level's nodes are rows [0, widths[t]) of step t of a [Tl x Nw] recurrence (VD_FLAG_TREE).
struct TreeChunk {
  int o0 = 0, C = 0, Tl = 0, Nw = 0;
  long n_nodes = 0;
  std::vector<int32_t> widths;   // [Tl]
  int32_t* mask2 = nullptr;      // device [2 x Tl x Nw]: token (0 = no node) | parent row (level 0: the round)
  int32_t* node_row = nullptr;   // device [n_nodes]: t * Nw + n, ascending -- the row list of the head
  int32_t *enode = nullptr, *etgt = nullptr;   // device [T x N*C]: node id and 1-based target of candidate r's edge at step t (target 0 = none)
};

struct BatchSlot {
  int B = 0;
  // VD_LHOOD_TREE: the prefix trees of the batch's option_in / option_out, one per chunk of options; tree_ok = false for a batch with a
  // token behind a pad (or out of the vocabulary) in any candidate, which takes the length-ordered path instead
  bool tree_ok = false;
  std::vector<TreeChunk> tree;
  SeqTok q, h, opt, ain, aout, oin, oout;
  float* img = nullptr;
  int32_t* gt = nullptr;  // [N] 0-based
  std::vector<int32_t> gt_host;
  bool has_gt = false;
  // batch attachment "@dense_relevance" (vd_model_set_tensor; loss.hip DT1): the relevance matrix [N x O] of this upload, or null; the next
  // upload into the slot clears it.  rel_W = the sum of DT3's weights over the batch with the model's mu
  float* rel = nullptr;
  double rel_W = 0.0;
  // "@dense_relevance_live" (loss.hip DL1 - DL3) where some but not all rounds are live: the live rounds' option tokens, compacted and
  // sorted behind the attachment on the side lane.  opt_live.N = n_live * O rows; live_slot [N] on the device; n_live = 0: all rows
  // batch attachment "@img_regions" (attention.hip IR1): the number of live regions of every image of this upload [B] on the device, or
  // null = every image holds all S2; the next upload into the slot clears it
  int32_t* regions = nullptr;
  SeqTok opt_live;
  int n_live = 0;
  int32_t *live_slot = nullptr, *live_sort_off = nullptr, *live_sort_perm = nullptr;
  // option de-duplication (decoder disc): the option LSTM encodes every DISTINCT candidate once (decoders/disc.lua:4-15 --
  // the encoding depends on the tokens only); opt_uid[n * O + o] = its row among the opt.N unique rows, or null
  int32_t* opt_uid = nullptr;
  int opt_total = 0;           // N * O
  // counting sort of the option tokens (the table gradient's row order), done with the upload on the side lane: it depends on the
  // batch alone, and inside the step it stood in front of the encoder backward on that in-order lane
  int32_t *opt_sort_off = nullptr, *opt_sort_perm = nullptr;
  // answer-encoding cache (OptionCache): the slot was resolved against the cache -- opt = the MISS rows only, opt_uid = table row of every
  // candidate; miss_keys [opt.N x To] wait for the step's commit, opt_host keeps the batch's rows for a second resolution
  bool cached = false;
  uint64_t cache_stamp = 0;
  std::vector<int32_t> miss_keys, opt_host;
  // work list of the encoder backward's live-row weight-gradient launch (wgrad_flush): built on the first backward over this upload's
  // sequence sets, kept while the products stay the same (wgrad_sig; an upload of tokens clears it)
  std::vector<long> wgrad_sig;
  int32_t *wgrad_items = nullptr, *wgrad_chunk_start = nullptr;
  int wgrad_chunks = 0;
  hipEvent_t ready = nullptr;  // recorded on the side lane when the upload has landed
  hipEvent_t done = nullptr;   // recorded on the main stream behind the last reader of this slot
  bool used = false;      // a step has read this slot (done is recorded)
  bool uploaded = false;  // ready is recorded (an upload has been issued into this slot)
  std::map<std::string, DevBuf> bufs, pinned;
};

// Host index of distinct token rows (open addressing over the rows' tokens): id = order of insertion.  The option de-duplication of one
// batch and the answer-encoding cache (OptionCache) both key candidate rows with it.
struct RowIndex {
  int T = 0;
  std::vector<int32_t> keys;    // [size x T]
  std::vector<int32_t> table;   // power of two, -1 = empty
  int32_t size() const { return T ? (int32_t)(keys.size() / (size_t)T) : 0; }
  void reset(int T_) {
    T = T_;
    keys.clear();
    table.assign(1024, -1);
  }
  size_t home(const int32_t* row) const {
    uint64_t h = 1469598103934665603ull;
    for (int t = 0; t < T; ++t) h = (h ^ (uint32_t)row[t]) * 1099511628211ull;
    return (size_t)(h ^ (h >> 29)) & (table.size() - 1);
  }
  int32_t find(const int32_t* row) const {
    for (size_t pos = home(row);; pos = (pos + 1) & (table.size() - 1)) {
      const int32_t u = table[pos];
      if (u < 0) return -1;
      if (memcmp(keys.data() + (size_t)u * T, row, (size_t)T * sizeof(int32_t)) == 0) return u;
    }
  }
  int32_t add(const int32_t* row) {   // the row is not in the index
    if ((size_t)(size() + 1) * 2 > table.size()) {
      table.assign(table.size() * 2, -1);
      for (int32_t u = 0; u < size(); ++u) place(keys.data() + (size_t)u * T, u);
    }
    const int32_t id = size();
    keys.insert(keys.end(), row, row + T);
    place(keys.data() + (size_t)id * T, id);
    return id;
  }
  void place(const int32_t* row, int32_t id) {
    size_t pos = home(row);
    while (table[pos] >= 0) pos = (pos + 1) & (table.size() - 1);
    table[pos] = id;
  }
};

// Answer-encoding cache of the discriminative decoder (VD_OPTION_CACHE; include/visdial_hip.h at vd_model_retrieve).  A candidate's
// encoding depends on its tokens, on To (trailing pads advance the state) and on the weights only, so while the weights stand still
// the final h of every distinct (row, To) is kept in `table` [rows x H]; slot = RowIndex id.  The index flushes when To changes.
//   * upload (side lane, ahead of the step): resolves the N * O rows against the COMMITTED index; rows it does not hold are
//     de-duplicated inside the batch and numbered count, count + 1, ... (the slot's miss_keys); nothing is inserted yet, so a batch
//     that is replaced or never stepped leaves no entry behind
//   * step: runs the state-only recurrence over the misses, copies their final h to table rows [count, count + misses) and only then
//     inserts the first (capacity - count) of them.  Misses beyond the capacity stay in the tail of the table for this step alone.
//   * `stamp` moves with every flush and every step; a slot resolved under another stamp (stepped twice, flushed in between) is
//     resolved again from the host copy of its rows at step time.
struct OptionCache {
  long capacity = 0;       // rows; 0 = off
  RowIndex index;
  float* table = nullptr;
  long table_rows = 0;     // allocated; grows geometrically up to capacity + the largest batch's misses
  uint64_t stamp = 1;
  void flush() {
    index.reset(index.T);
    ++stamp;
  }
};
static constexpr long VD_OPTION_CACHE_FIRST_ROWS = 16384;      // first allocation; doubles from there

// one dense weight-gradient product of a length-sorted encoder LSTM, held back for the backward's grouped launch (wgrad_flush)
struct WgradProduct {
  VdLiveProduct p;      // (segs: filled in by the flush)
  const SeqTok* rows;
  int t_first;          // 0: x and da of one step; 1: h of step t - 1 with da of step t
};

struct Encoder;
struct Decoder;

}  // namespace vdrt

struct vd_model {
  vd_model_params p;
  int flags = 0;   // p.lstmBf16 as VD_FLAG_* (paths.h vd_precision_flags): the arithmetic of every pass
  std::string enc_name, dec_name;
  std::vector<vdrt::Tensor> spec;
  std::map<std::string, int> index;
  long numel = 0;
  float *W = nullptr, *G = nullptr, *M = nullptr, *V = nullptr;
  std::map<std::string, vdrt::DevBuf> ws;
  std::map<std::string, vdrt::DevBuf> ext_masks;
  // two lanes (runtime.hip vd_model_create): the throughput work on s_main, everything that runs beside it -- encoder chains, image
  // prefetch / history branch, table-gradient chain, batch uploads -- on s_side, in the host's enqueue order
  hipStream_t s_main = nullptr, s_side = nullptr;
  // parameter-gradient work of the nngraph encoders that nothing downstream in the backward pass waits for (image-attention
  // weight gradients, the recurrences' weight / input gradients): middle priority = its own hardware queue beside the side
  // lane (runtime.hip).  wg_active: the current backward uses it; wg_used: it holds un-joined work
  hipStream_t s_wg = nullptr;
  bool wg_active = false, wg_used = false;
  // wgrad_open: SeqLSTM::param_grads appends its eligible products (paths.h vd_wgrad_group_fits) here instead of launching them, and the
  // encoder backward that opened the group flushes it as one launch (wgrad_flush) -- or, with wgrad_hold set by its caller, leaves the
  // products here for the caller's flush
  std::vector<vdrt::WgradProduct> wgrad;
  bool wgrad_open = false, wgrad_hold = false;
  std::vector<hipEvent_t> ev_pool;
  size_t ev_next = 0;
  hipEvent_t ev_enc_grads = nullptr;  // recorded behind the encoder backward: its gradient tensors are final
  hipEvent_t ev_updated = nullptr;    // recorded behind the optimiser launch: the prefetch upload's kernels (the option tokens'
                                      // counting sort) wait for it instead of sharing HBM with clamp_adam (65 -> 104 us beside them)
  bool updated_recorded = false;
  bool enc_grads_recorded = false;
  hipEvent_t ev_loss = nullptr, ev_prof[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  bool training = true, streams = true, prof_valid = false;
  long step = 0;
  int adam_t = 0;
  double lr = 1e-3;
  vdrt::BatchSlot slot[2];
  int cur = -1, uploaded = -1;
  float* loss_host = nullptr;  // pinned
  long loss_cap = 0, loss_n = 0;
  bool loss_is_sum = false;
  double loss_div = 0.0;   // a dense step (loss.hip DT4): vd_model_loss divides the sum of the rows by W; 0 = by loss_n
  std::unique_ptr<vdrt::Encoder> enc;
  std::unique_ptr<vdrt::Decoder> dec;
  float* scores = nullptr;  // [N x O] of the last forward / retrieval
  float* gen_enc_out = nullptr;  // encoder output of the last vd_model_encode (generation)
  int gen_seq_len = 0;
  int N = 0, O = 0;
  // vd_model_option_rows after vd_model_retrieve_lhood: (step, candidate) rows in a row group the candidate recurrence ran, of To * N * O;
  // -1 = the last step call was another one
  long lhood_exec = -1, lhood_total = 0;
  bool step_live = false;   // the last step call ran the live rounds' candidate rows only (DL3): vd_model_option_rows reports them
  // capability flags from the encoder NAME (opts.lua:54-67)
  bool use_im = false, use_hist = false, is_att = false, is_graph = false;
  vdrt::OptionCache ocache;
  vdrt::Switches sw;   // what vd_model_create read from the environment (rt_switches.h)
  int rollout_max_words = 0;     // the most words an answer of the running rollout appends (disc: To, gen: beamLen - 1): the round pass of a
                                 // concatenated history sizes its window of new tokens with it (rt_encoders.h history_round_concat)
  std::vector<double> beam_lp;   // host copy of the table s^alpha, s < beamLen (VD_BEAM_LENGTH_PENALTY), kept until its upload has run
  bool prof_hist = false;   // ev_prof[0..3] bracket the history branch of a Sequential encoder (gen pairs: vd_model_family_ms)
  ~vd_model();
};

namespace vdrt {

// ------------------------------------------------------------------------------------------------------------
// memory / stream helpers
// ------------------------------------------------------------------------------------------------------------
inline int dev_get(std::map<std::string, DevBuf>& m, const std::string& key, size_t bytes, void** out) {
  DevBuf& b = m[key];
  if (b.bytes < bytes) {
    if (b.p) VD_HIP(hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
    VD_HIP(hipMalloc(&b.p, bytes ? bytes : 16));
    b.bytes = bytes ? bytes : 16;
  }
  *out = b.p;
  return VD_OK;
}
inline int pin_get(std::map<std::string, DevBuf>& m, const std::string& key, size_t bytes, void** out) {
  DevBuf& b = m[key];
  if (b.bytes < bytes) {
    if (b.p) VD_HIP(hipHostFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
    VD_HIP(hipHostMalloc(&b.p, bytes ? bytes : 16, hipHostMallocDefault));
    b.bytes = bytes ? bytes : 16;
  }
  *out = b.p;
  return VD_OK;
}

template <class T>
int ws_get(vd_model* m, const std::string& key, size_t count, T** out) {
  void* p = nullptr;
  VD_TRY(dev_get(m->ws, key, count * sizeof(T), &p));
  *out = static_cast<T*>(p);
  return VD_OK;
}

inline void add_lstm(vd_model* m, const std::string& name, long D, long H) {
  m->spec.push_back(Tensor{name + ".W", 0, D + H, 4 * H, 1});
  m->spec.push_back(Tensor{name + ".b", 0, 1, 4 * H, 2});
}
inline void add_linear(vd_model* m, const std::string& name, long in, long out) {
  m->spec.push_back(Tensor{name + ".W", 0, out, in, 3});
  m->spec.push_back(Tensor{name + ".b", 0, 1, out, 4});
}
inline std::string hop_sfx(int i) { return i == 0 ? std::string() : std::to_string(i + 1); }

inline float* Wp(vd_model* m, const std::string& n) { return m->W + m->spec[m->index.at(n)].off; }
inline float* Gp(vd_model* m, const std::string& n) { return m->G + m->spec[m->index.at(n)].off; }

// fork: `side` waits for everything enqueued on `from` so far; join: `to` waits for `side`
inline int fork_stream(vd_model* m, hipStream_t from, hipStream_t side) {
  if (side == from) return VD_OK;
  hipEvent_t e = m->ev_pool[m->ev_next++ % m->ev_pool.size()];
  VD_HIP(hipEventRecord(e, from));
  VD_HIP(hipStreamWaitEvent(side, e, 0));
  return VD_OK;
}
inline int join_stream(vd_model* m, hipStream_t side, hipStream_t to) { return fork_stream(m, side, to); }
// the side lane (`cur` itself with useStreams = 0).  A caller that already runs on it gets `cur` back, and its fork / join are no-ops
inline hipStream_t side_stream(vd_model* m, hipStream_t cur) { return m->streams ? m->s_side : cur; }
// the stream for off-chain parameter-gradient work enqueued after everything on `cur` so far (cur itself when the feature is off)
inline int wg_fork(vd_model* m, hipStream_t cur, hipStream_t* out) {
  *out = cur;
  if (!m->wg_active || !m->s_wg) return VD_OK;
  VD_TRY(fork_stream(m, cur, m->s_wg));
  m->wg_used = true;
  *out = m->s_wg;
  return VD_OK;
}

// The live-row weight-gradient group of one encoder backward.  Between wgrad_begin and wgrad_flush the length-sorted LSTMs' param_grads
// hold their eligible products back; the flush contracts them in ONE launch on `s` over the live rows only (the pad pairs hold da = 0:
// exact zeros leave the sums).  About one round of workgroups (3 per CU), a chunk no shorter than 32 k-steps: every item ends in 64 KB
// of float atomics.  The work list depends on the batch's lengths and the products' tiles alone: built once per upload into the slot.
// (384 and 1536 chunks measured the same step time as 768, profiles/enc_wgrad_group.txt.)
// The group ends with the encoder backward (wgrad_end): flushed there, or, under wgrad_hold, left to the caller's own wgrad_flush -- the
// discriminative step puts it behind its option recurrence (rt_decoders.h).
constexpr int VD_WGRAD_CHUNKS = 768, VD_WGRAD_MIN_KSTEPS = 32;
inline void wgrad_begin(vd_model* m) {
  m->wgrad.clear();
  m->wgrad_open = true;
}
inline int wgrad_flush(vd_model* m, BatchSlot& b, hipStream_t s) {
  m->wgrad_open = false;
  const int n = (int)m->wgrad.size();
  if (n == 0) return VD_OK;
  VD_CHECK_ARG(n <= VD_LIVE_MAXP, "%d weight-gradient products in one encoder backward, the grouped launch takes %d", n, VD_LIVE_MAXP);
  VdLiveProduct lp[VD_LIVE_MAXP];
  vdplan::Product prod[VD_LIVE_MAXP];
  std::vector<long> sig;
  long total = 0;
  for (int i = 0; i < n; ++i) {
    const WgradProduct& w = m->wgrad[i];
    const int f = w.t_first;
    lp[i] = w.p;
    lp[i].segs = w.rows->seg_dev[f];
    prod[i] = vdplan::Product{w.rows->seg_host[f].data(), (int)w.rows->seg_host[f].size() - 1, w.rows->seg_ksteps[f], (w.p.M / 128) * (w.p.N / 128)};
    total += (long)prod[i].ksteps * prod[i].tiles;
    for (const long v : {(long)(intptr_t)w.rows, (long)f, (long)w.p.M, (long)w.p.N}) sig.push_back(v);
  }
  m->wgrad.clear();
  if (total == 0) return VD_OK;   // no live pair at all
  if (sig != b.wgrad_sig) {
    std::vector<vdplan::Item> items;
    std::vector<int32_t> start;
    const int chunks = (int)std::min<long>(VD_WGRAD_CHUNKS, (total + VD_WGRAD_MIN_KSTEPS - 1) / VD_WGRAD_MIN_KSTEPS);
    vdplan::work_list(prod, n, chunks, &items, &start);
    const size_t ints = 4 * items.size() + start.size();
    int32_t *stage, *dev;
    VD_TRY(pin_get(b.pinned, "wgrad.plan", ints * sizeof(int32_t), (void**)&stage));
    VD_TRY(dev_get(b.bufs, "wgrad.plan", ints * sizeof(int32_t), (void**)&dev));
    for (size_t i = 0; i < items.size(); ++i) {
      const vdplan::Item& it = items[i];
      const int32_t packed[4] = {(it.product << 24) | it.tile, it.seg, it.j, it.nk};
      memcpy(stage + 4 * i, packed, sizeof(packed));
    }
    memcpy(stage + 4 * items.size(), start.data(), start.size() * sizeof(int32_t));
    VD_HIP(hipMemcpyAsync(dev, stage, ints * sizeof(int32_t), hipMemcpyHostToDevice, s));
    b.wgrad_items = dev;
    b.wgrad_chunk_start = dev + 4 * items.size();
    b.wgrad_chunks = chunks;
    b.wgrad_sig = sig;
  }
  return vd_gemm_tn_live_grouped(lp, n, b.wgrad_items, b.wgrad_chunk_start, b.wgrad_chunks, s);
}
inline int wgrad_end(vd_model* m, BatchSlot& b, hipStream_t s) {
  m->wgrad_open = false;
  return m->wgrad_hold ? VD_OK : wgrad_flush(m, b, s);
}

// nn.Dropout keep-mask for a call site (null in evaluate mode or p == 0); external masks pin the noise for parity runs
inline int drop_mask(vd_model* m, const std::string& site, size_t numel, float p, hipStream_t s, uint8_t** out) {
  *out = nullptr;
  if (!m->training || p <= 0.f) return VD_OK;
  auto it = m->ext_masks.find(site);
  if (it != m->ext_masks.end()) {
    VD_CHECK_ARG(it->second.bytes >= numel, "dropout mask '%s' holds %zu bytes, the batch needs %zu", site.c_str(),
                 it->second.bytes, numel);
    *out = static_cast<uint8_t*>(it->second.p);
    return VD_OK;
  }
  if (!m->ext_masks.empty()) {
    vd_set_error("external dropout masks are set but none for site '%s'", site.c_str());
    return VD_ERR_STATE;
  }
  uint8_t* buf = nullptr;
  VD_TRY(ws_get(m, "dropmask." + site, numel + 4, &buf));
  uint32_t h = 2166136261u;  // FNV-1a of the site name: one independent stream per (seed, step, site)
  for (const char c : site) h = (h ^ (uint8_t)c) * 16777619u;
  const uint64_t seed = ((uint64_t)((m->p.seed * 1000003ull + (uint64_t)m->step) & 0xffffffffull) << 32) | h;
  VD_TRY(vd_dropout_mask(buf, (int64_t)numel, seed, p, s));
  *out = buf;
  return VD_OK;
}
// y = dropout(x) (x itself when mask is null)
inline int dropout_fwd(vd_model* m, const std::string& key, const float* x, const uint8_t* mask, float scale, long n, hipStream_t s,
                       const float** y) {
  *y = x;
  if (!mask) return VD_OK;
  float* buf;
  VD_TRY(ws_get(m, key, (size_t)n, &buf));
  VD_TRY(vd_dropout_apply(x, mask, buf, n, scale, s));
  *y = buf;
  return VD_OK;
}

// small int32 index arrays cached on the device (row permutations / per-round image index)
inline int index_array(vd_model* m, const std::string& key, const std::vector<int32_t>& host, int32_t** out) {
  DevBuf& b = m->ws[key];
  if (b.bytes != host.size() * sizeof(int32_t) || !b.p) {
    if (b.p) VD_HIP(hipFree(b.p));
    b.p = nullptr;
    VD_HIP(hipMalloc(&b.p, host.size() * sizeof(int32_t) + 16));
    b.bytes = host.size() * sizeof(int32_t);
    VD_HIP(hipMemcpy(b.p, host.data(), b.bytes, hipMemcpyHostToDevice));
  }
  *out = static_cast<int32_t*>(b.p);
  return VD_OK;
}
inline int round_index(vd_model* m, int N, int R, int32_t** out) {  // row n of a per-round tensor -> its image row n / R
  std::vector<int32_t> h(N);
  for (int n = 0; n < N; ++n) h[n] = n / R;
  return index_array(m, "idx.rep." + std::to_string(N) + "." + std::to_string(R), h, out);
}

// ------------------------------------------------------------------------------------------------------------
// nn.Linear (+ optional fused nn.Tanh)                                                  visdial_amd/nn.py:Linear
// ------------------------------------------------------------------------------------------------------------
struct Linear {
  std::string name;
  long in = 0, out = 0;
  const float* x = nullptr;
  float* y = nullptr;
  long M = 0;
  bool tanh_ = false;
  void init(const std::string& n, long i, long o) { name = n; in = i; out = o; }
  int forward(vd_model* m, hipStream_t s, const float* x_, long M_, bool tanh, float** y_out) {
    x = x_; M = M_; tanh_ = tanh;
    VD_TRY(ws_get(m, name + ".y", (size_t)M * out, &y));
    VD_TRY(vd_gemm_nt(x, in, Wp(m, name + ".W"), in, Wp(m, name + ".b"), y, out, (int)M, (int)out, (int)in,
                      tanh ? VD_ACT_TANH : VD_ACT_NONE, 0, s));
    if (y_out) *y_out = y;
    return VD_OK;
  }
  int backward(vd_model* m, hipStream_t s, const float* dy, bool need_dx, float** dx_out) {
    const float* d = dy;
    if (tanh_) {
      float* dpre;
      VD_TRY(ws_get(m, name + ".dpre", (size_t)M * out, &dpre));
      VD_TRY(vd_tanh_backward(dy, y, dpre, M * out, s));
      d = dpre;
    }
    VD_TRY(vd_gemm_tn_acc(d, out, x, in, Gp(m, name + ".W"), in, (int)out, (int)in, (int)M, 0, s));
    VD_TRY(vd_colsum_acc(d, out, (int)M, (int)out, Gp(m, name + ".b"), s));
    if (dx_out) *dx_out = nullptr;
    if (need_dx) {
      float* dx;
      VD_TRY(ws_get(m, name + ".dx", (size_t)M * in, &dx));
      VD_TRY(vd_gemm_nn(d, out, Wp(m, name + ".W"), in, nullptr, dx, in, (int)M, (int)in, (int)out, 0, s));
      if (dx_out) *dx_out = dx;
    }
    return VD_OK;
  }
};

// Tanh(Linear(JoinTable(parts))) with optional Dropout on the joined vector            _blocks.py:CatLinear
struct CatLinear {
  std::string name;
  std::vector<long> dims;
  long D = 0, H = 0, N = 0;
  Linear lin;
  const uint8_t* mask = nullptr;
  float scale = 1.f;
  void init(const std::string& n, const std::vector<long>& d, long H_) {
    name = n; dims = d; H = H_; D = 0;
    for (long v : d) D += v;
    lin.init(n, D, H_);
  }
  int forward(vd_model* m, hipStream_t s, const std::vector<const float*>& parts, long N_, const uint8_t* mask_, float scale_,
              float** y) {
    N = N_; mask = mask_; scale = scale_;
    float* cat;
    VD_TRY(ws_get(m, name + ".cat", (size_t)N * D, &cat));
    long off = 0;
    for (size_t i = 0; i < dims.size(); ++i) {
      VD_TRY(vd_copy_2d(cat + off, D, parts[i], dims[i], N, dims[i], s));
      off += dims[i];
    }
    const float* catd;
    VD_TRY(dropout_fwd(m, name + ".in", cat, mask, scale, N * D, s, &catd));
    return lin.forward(m, s, catd, N, true, y);
  }
  // per-part gradients ([N x d_i] contiguous; null where not needed)
  int backward(vd_model* m, hipStream_t s, const float* dy, const std::vector<bool>& need, std::vector<float*>* out) {
    float* dcatd;
    VD_TRY(lin.backward(m, s, dy, true, &dcatd));
    const float* dcat;
    VD_TRY(dropout_fwd(m, name + ".din", dcatd, mask, scale, N * D, s, &dcat));
    out->assign(dims.size(), nullptr);
    long off = 0;
    for (size_t i = 0; i < dims.size(); ++i) {
      if (need.empty() || need[i]) {
        float* g;
        VD_TRY(ws_get(m, name + ".dpart" + std::to_string(i), (size_t)N * dims[i], &g));
        VD_TRY(vd_copy_2d(g, dims[i], dcat + off, D, N, dims[i], s));
        (*out)[i] = g;
      }
      off += dims[i];
    }
    return VD_OK;
  }
};

// ------------------------------------------------------------------------------------------------------------
// nn.SeqLSTM(D, H)[:maskZero()] over a whole time-major sequence                        visdial_amd/nn.py:SeqLSTM
// The input may arrive as several column blocks (`parts`): x*Wx is then the sum of the per-block products against
// the matching row blocks of Wx (nn.JoinTable(-1) in front of an LSTM folded away).  State hand-off fields carry the
// reference's names (rnn SeqLSTM; used by decoders/gen.lua:30-60).
// ------------------------------------------------------------------------------------------------------------
struct SeqLSTM {
  std::string name;
  long D = 0, H = 0;
  std::vector<long> parts;
  const float *userPrevOutput = nullptr, *userPrevCell = nullptr, *userNextGradCell = nullptr, *gradPrevOutput = nullptr;
  float *userGradPrevOutput = nullptr, *userGradPrevCell = nullptr;
  int T = 0, N = 0;
  std::vector<const float*> xs;
  const int32_t* tok_mask = nullptr;
  const float *h0 = nullptr, *c0 = nullptr;
  float *gates = nullptr, *h = nullptr, *c = nullptr;
  const SeqTok* rows = nullptr;   // set for length-sorted stacks: weight gradients skip the pad (t, row) pairs

  void init(const std::string& n, long D_, long H_, const std::vector<long>& p = {}) {
    name = n; D = D_; H = H_;
    parts = p.empty() ? std::vector<long>{D_} : p;
  }
  float* Wx(vd_model* m) const { return Wp(m, name + ".W"); }
  float* Wh(vd_model* m) const { return Wp(m, name + ".W") + D * 4 * H; }
  float* out_at(int t) const { return h + (long)t * N * H; }    // .output[t]
  float* cell_at(int t) const { return c + (long)t * N * H; }   // .cell[t]

  int alloc(vd_model* m, int T_, int N_) {
    T = T_; N = N_;
    VD_TRY(ws_get(m, name + ".gates", (size_t)T * N * 4 * H, &gates));
    VD_TRY(ws_get(m, name + ".h", (size_t)T * N * H, &h));
    VD_TRY(ws_get(m, name + ".c", (size_t)T * N * H, &c));
    return VD_OK;
  }
  // hands userPrevOutput / userPrevCell to the pass (h0, c0), the missing one of a pair as zeros
  int take_state(vd_model* m, hipStream_t s, int N_) {
    h0 = userPrevOutput; c0 = userPrevCell;
    userPrevOutput = userPrevCell = nullptr;                       // consumed once (rnn semantics)
    if (h0 && !c0) {
      float* z;
      VD_TRY(ws_get(m, name + ".c0zero", (size_t)N_ * H, &z));
      VD_TRY(vd_memset(z, 0, (long)N_ * H * 4, s));
      c0 = z;
    }
    if (c0 && !h0) {
      float* z;
      VD_TRY(ws_get(m, name + ".h0zero", (size_t)N_ * H, &z));
      VD_TRY(vd_memset(z, 0, (long)N_ * H * 4, s));
      h0 = z;
    }
    return VD_OK;
  }
  int forward(vd_model* m, hipStream_t s, const std::vector<const float*>& x, int T_, int N_, const int32_t* tok, float** h_out) {
    VD_TRY(take_state(m, s, N_));
    VD_TRY(alloc(m, T_, N_));
    xs = x; tok_mask = tok; rows = nullptr;
    // hoisted input projection, written straight into the gates buffer (the recurrence runs in place)
    long roff = 0;
    for (size_t i = 0; i < parts.size(); ++i) {
      VD_TRY(vd_gemm_nn(xs[i], parts[i], Wx(m) + roff * 4 * H, 4 * H, i == 0 ? Wp(m, name + ".b") : nullptr, gates, 4 * H,
                        T * N, (int)(4 * H), (int)parts[i], i > 0 ? 1 : 0, s));
      roff += parts[i];
    }
    VD_TRY(vd_lstm_forward(gates, (int64_t)N * 4 * H, 4 * H, nullptr, tok, Wh(m), h0, c0, gates, h, c, T, N, (int)H, 0, s));
    if (h_out) *h_out = h;
    return VD_OK;
  }
  // Forward-only pass of generative retrieval (rt_decoders.h).  `table` (layer 1): xproj = Emb * Wx + b gathered by token id inside the
  // step kernel; else `x` [T*N x D] (the h of the layer below) is projected here.  `mask` and `flags` go to the step kernel:
  //   0                    tokens [T x N], every row runs
  //   VD_FLAG_LIVE_PREFIX  tokens of length-ordered candidates: the projection and the steps skip the row tiles without a live row (the
  //                        same tiles: one launch per step, the step kernel's tile height), whose gates / h / c rows are left unwritten
  //   VD_FLAG_TREE         a forest, level by level: mask [2 x T x N] = token | parent row; the parents of level 0 are rows of the state
  //                        in userPrevOutput / userPrevCell, which holds `state_rows` rows; the row tiles without a node are skipped
  // keep_gates = false: only h and c of every step are kept, no gate value is stored (and with a table there is no gates buffer).
  int forward_only(vd_model* m, hipStream_t s, const float* table, const float* x, int T_, int N_, const int32_t* mask, int flags,
                   int state_rows, bool keep_gates, float** h_out) {
    VD_TRY(take_state(m, s, state_rows));
    if (keep_gates) {
      VD_TRY(alloc(m, T_, N_));
    } else {
      T = T_; N = N_;
      VD_TRY(ws_get(m, name + ".h", (size_t)T * N * H, &h));
      VD_TRY(ws_get(m, name + ".c", (size_t)T * N * H, &c));
      if (!table) VD_TRY(ws_get(m, name + ".gates", (size_t)T * N * 4 * H, &gates));   // the projection's buffer only
    }
    xs.clear(); tok_mask = mask; rows = nullptr;
    float* gates_out = keep_gates ? gates : nullptr;
    if (table) {
      VD_TRY(vd_lstm_forward(table, 0, 4 * H, mask, mask, Wh(m), h0, c0, gates_out, h, c, T, N, (int)H, flags, s));
    } else {
      if (flags & (VD_FLAG_LIVE_PREFIX | VD_FLAG_TREE)) {
        for (int t = 0; t < T; ++t)
          VD_TRY(vd_gemm_nn_live_p(x + (long)t * N * D, D, Wx(m), 4 * H, Wp(m, name + ".b"), gates + (long)t * N * 4 * H, 4 * H, N, (int)(4 * H),
                                   (int)D, mask + (long)t * N, vd_lstm_fwd_row_tile(N), s));
      } else {
        VD_TRY(vd_gemm_nn(x, D, Wx(m), 4 * H, Wp(m, name + ".b"), gates, 4 * H, T * N, (int)(4 * H), (int)D, 0, s));
      }
      VD_TRY(vd_lstm_forward(gates, (int64_t)N * 4 * H, 4 * H, nullptr, mask, Wh(m), h0, c0, gates_out, h, c, T, N, (int)H, flags, s));
    }
    if (h_out) *h_out = h;
    return VD_OK;
  }
  // weight / bias / input gradients from da (held in the gates buffer after BPTT)
  int param_grads(vd_model* m, hipStream_t s, const std::vector<bool>& need_dx, std::vector<float*>* dxs) {
    const long TN = (long)T * N;
    float* dW = Gp(m, name + ".W");
    float* dWh = dW + D * 4 * H;
    const bool by_rows = rows && rows->act;
    // Where the shape fits the k-major LDS-DMA contraction (M, N multiples of 128: the recurrent weights and the
    // layer-2 input weights at H = 512) the DENSE product over all T*N rows on that kernel beats the index-list
    // contraction of the non-pad pairs: the pad pairs hold da = 0 (rt_encoders.h zero-fills them), the kernel streams at
    // the option dWh kernel's rate, and its workgroups live ~0.1 ms instead of ~0.8 ms -- the index-list kernel is a chain
    // of dependent (row index -> row) loads per K tile whose long-lived workgroups take the third slot of a third of the
    // CUs away from the option-LSTM backward kernels for most of their run.  (Inside an encoder backward those products do not
    // launch here at all: `grouped` below hands them to the backward's one live-row launch, which skips the pad pairs without an
    // index list -- the live rows of a step are a contiguous prefix.  The dense path remains for a recurrence outside such a group.)
    auto dense_fits = [&](long Mrows, long K) { return vd_tn_kmajor_fits(Mrows, 4 * H, K); };
    // bf16 pass (lstmPrecision = 'bf16', configs[4]): the dense contractions whose shape the bf16 kernel takes (256-row tiles) round both
    // fp32 operands to bf16 in registers and multiply on the bf16 MFMA (gemm_ops.hip: 77 vs 167 us at K = 8 000)
    auto wg_flags = [&](long Mrows) { return (m->flags & VD_FLAG_BF16) && vd_tn_split_tiles(Mrows, 4 * H) ? VD_FLAG_BF16 : 0; };
    // inside an encoder backward's group (wgrad_begin): the products the grouped live-row launch takes wait for its flush
    auto grouped = [&](const float* A, long Mrows, const float* B, float* C, int t_first) {
      if (!m->wgrad_open || !vd_wgrad_group_fits(by_rows, Mrows, 4 * H, m->flags)) return false;
      m->wgrad.push_back(WgradProduct{VdLiveProduct{A, B, C, nullptr, Mrows, 4 * H, 4 * H, (int)Mrows, (int)(4 * H)}, rows, t_first});
      return true;
    };
    if (T > 1 && grouped(h, H, gates + (long)N * 4 * H, dWh, 1)) {
    } else if (by_rows && !(T > 1 && dense_fits(H, (long)(T - 1) * N))) {
      if (rows->n_act1 > 0)
        VD_TRY(vd_gemm_tn_rows_acc(h, H, rows->prev1, gates, 4 * H, rows->act1, dWh, 4 * H, (int)H, (int)(4 * H), rows->n_act1, s));
    } else if (T > 1) {
      VD_TRY(vd_gemm_tn_acc(h, H, gates + (long)N * 4 * H, 4 * H, dWh, 4 * H, (int)H, (int)(4 * H), (T - 1) * N, wg_flags(H), s));
    }
    if (h0) VD_TRY(vd_gemm_tn_acc(h0, H, gates, 4 * H, dWh, 4 * H, (int)H, (int)(4 * H), N, 0, s));
    VD_TRY(vd_colsum_acc(gates, 4 * H, (int)TN, (int)(4 * H), Gp(m, name + ".b"), s));
    if (dxs) dxs->assign(parts.size(), nullptr);
    long roff = 0;
    for (size_t i = 0; i < parts.size(); ++i) {
      if (grouped(xs[i], parts[i], gates, dW + roff * 4 * H, 0)) {
      } else if (by_rows && !dense_fits(parts[i], TN)) {
        if (rows->n_act > 0)
          VD_TRY(vd_gemm_tn_rows_acc(xs[i], parts[i], rows->act, gates, 4 * H, rows->act, dW + roff * 4 * H, 4 * H, (int)parts[i],
                                     (int)(4 * H), rows->n_act, s));
      } else {
        VD_TRY(vd_gemm_tn_acc(xs[i], parts[i], gates, 4 * H, dW + roff * 4 * H, 4 * H, (int)parts[i], (int)(4 * H), (int)TN, wg_flags(parts[i]), s));
      }
      if (need_dx.empty() || need_dx[i]) {
        float* dx;
        VD_TRY(ws_get(m, name + ".dx" + std::to_string(i), (size_t)TN * parts[i], &dx));
        VD_TRY(vd_gemm_nt(gates, 4 * H, Wx(m) + roff * 4 * H, 4 * H, nullptr, dx, parts[i], (int)TN, (int)parts[i], (int)(4 * H),
                          VD_ACT_NONE, 0, s));
        if (dxs) (*dxs)[i] = dx;
      }
      roff += parts[i];
    }
    return VD_OK;
  }
  int backward(vd_model* m, hipStream_t s, const float* dh_seq, const float* dh_last, const std::vector<bool>& need_dx,
               std::vector<float*>* dxs) {
    if (gradPrevOutput) {
      if (!dh_last) dh_last = gradPrevOutput;
      else {
        float* t;
        VD_TRY(ws_get(m, name + ".dhl", (size_t)N * H, &t));
        VD_TRY(vd_axpby(dh_last, gradPrevOutput, t, (long)N * H, 1.f, 1.f, s));
        dh_last = t;
      }
    }
    const float* dc_last = userNextGradCell;
    gradPrevOutput = userNextGradCell = nullptr;
    float *dc, *dh0 = nullptr;
    VD_TRY(ws_get(m, name + ".dc", (size_t)N * H, &dc));
    if (h0) VD_TRY(ws_get(m, name + ".dh0", (size_t)N * H, &dh0));
    VD_TRY(vd_lstm_backward(Wh(m), gates, c, c0, dh_seq, dh_last, dc_last, dc, dh0, nullptr, nullptr, T, N, (int)H, 0, s));
    userGradPrevOutput = dh0;
    userGradPrevCell = h0 ? dc : nullptr;
    return param_grads(m, s, need_dx, dxs);
  }
};

// numLayers x SeqLSTM(maskZero) (encoders/lf-ques.lua:18-24)
inline int lstm_stack_forward(vd_model* m, hipStream_t s, std::vector<SeqLSTM>& layers, const std::vector<const float*>& x, int T,
                              int N, const int32_t* tok, float** h_top) {
  float* h = nullptr;
  VD_TRY(layers[0].forward(m, s, x, T, N, tok, &h));
  for (size_t l = 1; l < layers.size(); ++l) VD_TRY(layers[l].forward(m, s, {h}, T, N, tok, &h));
  *h_top = h;
  return VD_OK;
}
inline int lstm_stack_backward(vd_model* m, hipStream_t s, std::vector<SeqLSTM>& layers, const float* dh_last_top,
                               const float* dh_seq_top, std::vector<float*>* dxs) {
  const float* dseq = dh_seq_top;
  for (int i = (int)layers.size() - 1; i >= 0; --i) {
    std::vector<float*> d;
    VD_TRY(layers[i].backward(m, s, dseq, i == (int)layers.size() - 1 ? dh_last_top : nullptr, {}, &d));
    if (i > 0) dseq = d[0];
    else if (dxs) *dxs = d;
  }
  return VD_OK;
}

}  // namespace vdrt
