// Discriminative decoder head: option scoring (decoders/disc.lua:22-29 nn.MM + Squeeze),
// nn.CrossEntropyCriterion (model.lua:37-38,330,334) and the rank computation of
// utils.lua:106-128 (computeRanks), all as wave-reduction kernels (HBM-bound: the
// [N x O x H] option encodings are read exactly once in forward and once in backward).
//
// Label smoothing eps in [0, 1) (VD_LABEL_SMOOTHING; not in the reference), the rule of the two training heads:
//   LS1 disc: the target of round n over its O options is t = (1 - eps) onehot(gt) + eps / O;
//       loss_n = lse - sum_o t_o s_o ; ds_o = (softmax_o - t_o) gscale.
//   LS2 gen: for every row that contributes without smoothing (non-pad input and target > 0), t = (1 - eps) onehot(target) + eps / V
//       over the V valid columns; loss_r = lse - sum_c t_c logit_c ; the gradient written in place is softmax - t; the alignment pad
//       columns stay 0 and masked rows stay all zero.
//   LS3 smoothing applies to vd_model_forward_backward(m, 0) only: only_forward = 1, vd_model_retrieve*, perplexity and every score or
//       rank are what they were; vd_model_loss after a training step reports the smoothed loss.
//   LS4 eps = 0 launches score_ce_kernel / logsoftmax_nll_kernel with their arguments; the smoothed forms are the <true> instantiations
//       of the same bodies under kernel names of their own.  block_row_lse is untouched; the row sum of the logits is a reduction of
//       its own (block_row_sum_stage below).
// Both heads evaluate t as onehot - eps (onehot - 1/K), i.e. loss = (lse - s_gt) + eps (s_gt - sum s / K): a head with one class
// (O = 1) then gives the plain head's bits, because onehot - 1/1 and s_gt - sum s / 1 are exactly 0.
//
// Dense relevance (the VisDial v1.0 annotations: one annotated round per dialog, a relevance in [0, 1] for each candidate; not in the
// reference).  visdial_amd/dense.py restates the rules in fp64 numpy:
//   DT1 a batch of N rounds may carry a relevance matrix rel [N x O] of floats (vd_model_set_tensor "@dense_relevance").  A row is annotated
//       -- every entry finite and >= 0 -- or not annotated -- every entry -1; anything else (a mixed row, a NaN, another negative value) is
//       refused by name on the host, before it reaches the device.
//   DT2 NDCG of an annotated row: k = #{o : rel_o > 0}; candidates ranked by score with the rule of ranks_kernel (higher score first, lower
//       index first among equal scores); DCG = sum over the candidates of rank r <= k of rel / log2(1 + r); IDCG = the same sum with the
//       candidates ranked by relevance, descending, lower index first among equal values; NDCG = DCG / IDCG (the official v1.0 evaluation).
//       A row with k = 0 has none: -1, left out of the mean.  A row that is not annotated: -2.
//   DT3 the target of an annotated row with sum_o rel > 0 is t = rel / sum rel with weight w = 1; an annotated row whose relevances are all 0
//       has w = 0.  A row that is not annotated keeps t = onehot(gt) with w = mu (VD_DENSE_MIX in [0, 1]; 0 or unset: such rounds do not train).
//   DT4 loss_n = lse - sum_o t_o s_o; the step's loss is sum_n w_n loss_n / W with W = sum_n w_n over this batch; ds_o = w_n (softmax_o - t_o)
//       / W.  A batch with W = 0 is refused by name.  loss_rows[n] holds w_n loss_n; the host divides the sum by W (vd_model_loss).
//   DT5 the dense target applies to vd_model_forward_backward(m, 0) of a disc model only, as LS3: only_forward = 1, retrieval, scores and
//       ranks ignore it; a batch without the matrix launches score_ce_kernel / score_ce_smooth_kernel with their arguments; a dense batch on
//       a model created with VD_LABEL_SMOOTHING > 0 and a dense training step of a gen model are refused by name (gen accepts it for NDCG).
//
// Live rounds (vd_model_set_tensor "@dense_relevance_live": the same matrix, the same validation, and the candidate rows of the rounds that
// train only).  visdial_amd/dense.py restates DL1 and the compaction (live_rounds, live_option_tokens):
//   DL1 a round is live iff its DT3 weight w_n is > 0 under the model's mu: annotated with sum rel > 0, or not annotated with mu > 0.  The live
//       rounds are taken in ascending round order (live_idx [n_live]; live_slot [N] = the place of round n in it, or -1), candidate order kept.
//   DL2 if every round is live the attachment IS "@dense_relevance": the same kernels with the same arguments, nothing extra.  W = 0 is refused
//       at the step as before.
//   DL3 otherwise vd_model_forward_backward(m, 0) runs the option recurrence, its backward, the table-gradient row sum and the dWh contraction
//       over the n_live * O candidate rows of the live rounds (dense_live_tokens_kernel compacts their tokens at attach time, resolving a
//       de-duplicated upload's opt_uid: one row per (live round, candidate)); the encoder runs over all N rounds.  Loss, loss_div and every
//       gradient are those of the all-rows dense step up to fp32 summation order: a round of weight 0 adds exact zeros to each of them.
//       score_ce_dense_live_kernel writes the live rounds' scores; every other round's score row, loss_rows entry and d_enc row is 0.
//   DL4 only_forward = 1, retrieval and "@ndcg" ignore the live set (DT5): they see all rounds.  After a live training step "@ndcg" is still
//       right for every row that has an NDCG: k > 0 <=> w = 1 <=> live.
//   DL5 refused by name, before anything is enqueued: a model with lstmBf16 = 1 (the compact-state path is not covered), a gen model's
//       training step and VD_LABEL_SMOOTHING > 0 (both with DT5's words).  Candidates that repeat among the live rows are not de-duplicated.
#include "common.h"

#define MAX_OPT 128

// the heads read optH / enc and write dOptH / dEnc as float4 at multiples of H floats (H % 4 == 0): null, or 16-byte aligned
static inline bool score_ce_aligned(const float* optH, const float* enc, const float* dOptH, const float* dEnc) {
  return (((uintptr_t)optH | (uintptr_t)enc | (uintptr_t)dOptH | (uintptr_t)dEnc) & 15) == 0;
}

// One workgroup per QA round n.
//   score[o] = <optH[n,o,:], enc[n,:]> ; loss_n = logsumexp(score) - score[gt]
//   if train: ds = (softmax - onehot) * gscale ; dOptH[n,o,:] = ds[o]*enc[n,:] ; dEnc[n,:] = sum_o ds[o]*optH[n,o,:]
//   TARGET_SMOOTH: onehot is LS1's target.  TARGET_DENSE: the target and the weight of DT3 from the round's row of `rel` (staged in LDS next
//   to sc / ds); `smooth` is mu and gscale is 1 / W; a round of weight 0 writes its scores, loss 0 and zero gradients and reads optH once.
//   Two row indices: enc, dEnc, scores, loss_rows, gt and rel are read and written at round n, optH / dOptH at the O rows of round-sized block
//   `hn` (the three all-rows kernels pass n twice; the live head passes the round's slot among the live rounds: DL3).
enum ScoreTarget { TARGET_ONEHOT, TARGET_SMOOTH, TARGET_DENSE };
template <ScoreTarget TARGET>
__device__ __forceinline__ void score_ce_body(const float* __restrict__ optH, const float* __restrict__ enc, const int* __restrict__ gt,
                                              float* __restrict__ scores, float* __restrict__ loss_rows, float* __restrict__ dOptH,
                                              float* __restrict__ dEnc, int O, int H, float gscale, float smooth,
                                              const int n, const int hn, const float* __restrict__ rel = nullptr, float* rl = nullptr,
                                              float* row_w = nullptr) {
  __shared__ float sc[MAX_OPT];
  __shared__ float ds[MAX_OPT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* e = enc + (long)n * H;
  const float* oh = optH + (long)hn * O * H;
  for (int o = wave; o < O; o += 4) {
    float a = 0.f;
    for (int k = lane * 4; k < H; k += 256) {
      const float4 x = *reinterpret_cast<const float4*>(oh + (long)o * H + k);
      const float4 y = *reinterpret_cast<const float4*>(e + k);
      a += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
    }
    a = wave_sum(a);
    if (lane == 0) {
      sc[o] = a;
      scores[(long)n * O + o] = a;
    }
  }
  if constexpr (TARGET == TARGET_DENSE)
    for (int o = tid; o < O; o += 256) rl[o] = rel[(long)n * O + o];
  __syncthreads();
  if (gt == nullptr) return;
  if (wave == 0) {
    float mx = -INFINITY;
    for (int o = lane; o < O; o += 64) mx = fmaxf(mx, sc[o]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int o = lane; o < O; o += 64) sum += expf(sc[o] - mx);
    sum = wave_sum(sum);
    const float lse = mx + logf(sum);
    const int g = gt[n];
    if constexpr (TARGET == TARGET_DENSE) {
      float tot = 0.f;
      for (int o = lane; o < O; o += 64) tot += rl[o];
      tot = wave_sum(tot);
      const bool annotated = rl[0] >= 0.f;               // DT1: a row is all -1 or all >= 0
      const float w = annotated ? (tot > 0.f ? 1.f : 0.f) : smooth;
      const float inv = annotated && tot > 0.f ? 1.f / tot : 0.f;
      float dot = 0.f;
      for (int o = lane; o < O; o += 64) {
        const float t = annotated ? rl[o] * inv : (o == g ? 1.f : 0.f);
        dot += t * sc[o];
        ds[o] = (expf(sc[o] - lse) - t) * (w * gscale);
      }
      dot = wave_sum(dot);
      if (lane == 0) {
        loss_rows[n] = w > 0.f ? w * (lse - dot) : 0.f;
        *row_w = w;
      }
    } else if constexpr (TARGET == TARGET_SMOOTH) {
      const float invO = 1.f / (float)O;
      float tot = 0.f;
      for (int o = lane; o < O; o += 64) tot += sc[o];
      tot = wave_sum(tot);
      if (lane == 0) loss_rows[n] = (lse - sc[g]) + smooth * (sc[g] - tot * invO);
      for (int o = lane; o < O; o += 64)
        ds[o] = (expf(sc[o] - lse) - (o == g ? 1.f : 0.f) + smooth * ((o == g ? 1.f : 0.f) - invO)) * gscale;
    } else {
      if (lane == 0) loss_rows[n] = lse - sc[g];
      for (int o = lane; o < O; o += 64) ds[o] = (expf(sc[o] - lse) - (o == g ? 1.f : 0.f)) * gscale;
    }
  }
  if (dOptH == nullptr) return;
  __syncthreads();
  if constexpr (TARGET == TARGET_DENSE) {
    if (*row_w == 0.f) {   // DT3: the round does not train
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int k = tid * 4; k < H; k += 1024) {
        for (int o = 0; o < O; ++o) *reinterpret_cast<float4*>(dOptH + ((long)hn * O + o) * H + k) = z;
        *reinterpret_cast<float4*>(dEnc + (long)n * H + k) = z;
      }
      return;
    }
  }
  for (int k = tid * 4; k < H; k += 1024) {
    const float4 ev = *reinterpret_cast<const float4*>(e + k);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int o = 0; o < O; ++o) {
      const float d = ds[o];
      const float4 x = *reinterpret_cast<const float4*>(oh + (long)o * H + k);
      acc.x += d * x.x;
      acc.y += d * x.y;
      acc.z += d * x.z;
      acc.w += d * x.w;
      *reinterpret_cast<float4*>(dOptH + ((long)hn * O + o) * H + k) =
          make_float4(d * ev.x, d * ev.y, d * ev.z, d * ev.w);
    }
    *reinterpret_cast<float4*>(dEnc + (long)n * H + k) = acc;
  }
}
__global__ void __launch_bounds__(256)
score_ce_kernel(const float* __restrict__ optH, const float* __restrict__ enc, const int* __restrict__ gt,
                float* __restrict__ scores, float* __restrict__ loss_rows, float* __restrict__ dOptH,
                float* __restrict__ dEnc, int O, int H, float gscale) {
  score_ce_body<TARGET_ONEHOT>(optH, enc, gt, scores, loss_rows, dOptH, dEnc, O, H, gscale, 0.f, blockIdx.x, blockIdx.x);
}
__global__ void __launch_bounds__(256)
score_ce_smooth_kernel(const float* __restrict__ optH, const float* __restrict__ enc, const int* __restrict__ gt,
                       float* __restrict__ scores, float* __restrict__ loss_rows, float* __restrict__ dOptH,
                       float* __restrict__ dEnc, int O, int H, float gscale, float smooth) {
  score_ce_body<TARGET_SMOOTH>(optH, enc, gt, scores, loss_rows, dOptH, dEnc, O, H, gscale, smooth, blockIdx.x, blockIdx.x);
}
__global__ void __launch_bounds__(256)
score_ce_dense_kernel(const float* __restrict__ optH, const float* __restrict__ enc, const int* __restrict__ gt,
                      float* __restrict__ scores, float* __restrict__ loss_rows, float* __restrict__ dOptH,
                      float* __restrict__ dEnc, int O, int H, float gscale, float mix, const float* __restrict__ rel) {
  __shared__ float rl[MAX_OPT];   // the round's relevance row, next to the body's sc[] / ds[]
  __shared__ float row_w;
  score_ce_body<TARGET_DENSE>(optH, enc, gt, scores, loss_rows, dOptH, dEnc, O, H, gscale, mix, blockIdx.x, blockIdx.x, rel, rl, &row_w);
}
// DL3: the dense head over all N rounds with optH / dOptH holding the live rounds' rows only, [n_live * O x H].  A round that is not live
// (live_slot[n] < 0) writes its zero score row, loss 0 and its zero dEnc row and reads no optH.
__global__ void __launch_bounds__(256)
score_ce_dense_live_kernel(const float* __restrict__ optH, const float* __restrict__ enc, const int* __restrict__ gt,
                           float* __restrict__ scores, float* __restrict__ loss_rows, float* __restrict__ dOptH,
                           float* __restrict__ dEnc, int O, int H, float gscale, float mix, const float* __restrict__ rel,
                           const int* __restrict__ live_slot) {
  __shared__ float rl[MAX_OPT];
  __shared__ float row_w;
  const int n = blockIdx.x, tid = threadIdx.x, slot = live_slot[n];
  if (slot < 0) {
    if (tid < O) scores[(long)n * O + tid] = 0.f;
    if (tid == 0) loss_rows[n] = 0.f;
    if (dEnc != nullptr)
      for (int k = tid * 4; k < H; k += 1024) *reinterpret_cast<float4*>(dEnc + (long)n * H + k) = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  score_ce_body<TARGET_DENSE>(optH, enc, gt, scores, loss_rows, dOptH, dEnc, O, H, gscale, mix, n, slot, rel, rl, &row_w);
}

// DL3: the option tokens of the live rounds, step-major [To x n_live * O], from the uploaded step-major tok [To x rows]: output row
// (slot, o) = the row of candidate (live_idx[slot], o), through uid [N * O] where the upload de-duplicated the candidates.  One thread per
// output element; consecutive lanes write consecutive candidate rows of one step.
__global__ void __launch_bounds__(256)
dense_live_tokens_kernel(const int* __restrict__ tok, long rows, const int* __restrict__ uid, const int* __restrict__ live_idx, int O,
                         long live_rows, long total, int* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long t = i / live_rows, r = i - t * live_rows;
  const long slot = r / O, o = r - slot * O;
  const long cand = (long)live_idx[slot] * O + o;
  const long src = uid != nullptr ? (long)uid[cand] : cand;
  out[i] = tok[t * rows + src];
}

// rank[n,o] = 1 + #{j : s[j] > s[o]  or (s[j] == s[o] and j < o)}   (descending sort position)
__global__ void __launch_bounds__(128)
ranks_kernel(const float* __restrict__ scores, int* __restrict__ ranks, int O) {
  __shared__ float sc[MAX_OPT];
  const int n = blockIdx.x, o = threadIdx.x;
  if (o < O) sc[o] = scores[(long)n * O + o];
  __syncthreads();
  if (o >= O) return;
  const float s = sc[o];
  int r = 1;
  for (int j = 0; j < O; ++j) r += (sc[j] > s) || (sc[j] == s && j < o);
  ranks[(long)n * O + o] = r;
}

// DT2: NDCG of round n from its scores and its row of rel, one double per round (-1: k = 0, -2: not annotated).  Thread o ranks candidate o
// by score (the comparison of ranks_kernel) and by relevance and computes its two terms in double with log2 in double; thread 0 adds the
// <= 128 terms in index order (a candidate outside the first k adds an exact 0), so the value is the fp64 restatement's to rounding.  No
// atomics, no host read.
__global__ void __launch_bounds__(128)
ndcg_kernel(const float* __restrict__ scores, const float* __restrict__ rel, double* __restrict__ out, int O) {
  __shared__ float sc[MAX_OPT];
  __shared__ float rl[MAX_OPT];
  __shared__ int srank[MAX_OPT];
  __shared__ int rrank[MAX_OPT];
  __shared__ double dterm[MAX_OPT];
  __shared__ double iterm[MAX_OPT];
  __shared__ int kk;
  const int n = blockIdx.x, o = threadIdx.x;
  if (o < O) {
    sc[o] = scores[(long)n * O + o];
    rl[o] = rel[(long)n * O + o];
  }
  __syncthreads();
  if (o < O) {
    const float s = sc[o], v = rl[o];
    int r = 1, q = 1;
    for (int j = 0; j < O; ++j) {
      r += (sc[j] > s) || (sc[j] == s && j < o);
      q += (rl[j] > v) || (rl[j] == v && j < o);
    }
    srank[o] = r;
    rrank[o] = q;
  }
  if (o == 0) {
    int k = 0;
    for (int j = 0; j < O; ++j) k += rl[j] > 0.f;
    kk = k;
  }
  __syncthreads();
  const int k = kk;
  if (o < O) {
    dterm[o] = srank[o] <= k ? (double)rl[o] / log2(1.0 + (double)srank[o]) : 0.0;
    iterm[o] = rrank[o] <= k ? (double)rl[o] / log2(1.0 + (double)rrank[o]) : 0.0;
  }
  __syncthreads();
  if (o != 0) return;
  if (rl[0] < 0.f) {
    out[n] = -2.0;
    return;
  }
  if (k == 0) {
    out[n] = -1.0;
    return;
  }
  double dcg = 0.0, idcg = 0.0;
  for (int j = 0; j < O; ++j) {
    dcg += dterm[j];
    idcg += iterm[j];
  }
  out[n] = dcg / idcg;
}

// sum of one row of V logits for a 256-thread block (LS4): 256 strided threads, wave_sum, the four wave partials added in a fixed order.
// `red4` is a 4-float shared buffer of its own; the caller reads the result behind a later __syncthreads (block_row_lse has two).
__device__ __forceinline__ void block_row_sum_stage(const float* row, int V, float* red4) {
  const int tid = threadIdx.x;
  float s = 0.f;
  for (int c = tid; c < V; c += 256) s += row[c];
  s = wave_sum(s);
  if ((tid & 63) == 0) red4[tid >> 6] = s;
}

// Generative head, per (t, n) row of logits [rows x ld] (V valid columns):
//   nn.Sequencer(nn.MaskZero(nn.LogSoftMax(), 1)) + SequencerCriterion(MaskZeroCriterion(ClassNLL(sum)))
//   (decoders/gen.lua:23-24, model.lua:33-36): rows whose decoder input token is 0 contribute nothing.
//   loss_rows[r] = logsumexp(logits[r]) - logits[r, target-1]   (target ids are 1-based vocabulary ids)
//   logits[r, :] <- (softmax - onehot) (the gradient, unscaled: sizeAverage = false), zeros for pad rows.
//   SMOOTH: onehot is LS2's target; loss_rows[r] = (lse - logits[r, target-1]) + eps (logits[r, target-1] - sum_c logits[r, c] / V)
template <bool SMOOTH>
__device__ __forceinline__ void logsoftmax_nll_body(float* __restrict__ logits, long ld, int V, const int* __restrict__ tok_in,
                                                    const int* __restrict__ target, float* __restrict__ loss_rows, int write_grad,
                                                    float smooth) {
  __shared__ float red[8];
  const long r = blockIdx.x;
  const int tid = threadIdx.x;
  float* row = logits + r * ld;
  if (write_grad)
    for (long c = V + tid; c < ld; c += 256) row[c] = 0.f;  // keep the alignment pad columns finite (K-padding rule), however many
  // masked rows: a pad decoder input (MaskZero, gen.lua:23-24) or a pad TARGET -- utils.computeLhood masks on
  // words == 0 (utils.lua:86-102): an empty candidate has option_in = <START>,0.. and option_out = 0.. (processOptions
  // writes no <END> for length 0), so its first row has a non-pad input and target 0; it must contribute 0, not
  // read column -1
  if (tok_in[r] == 0 || target[r] <= 0) {
    if (tid == 0) loss_rows[r] = 0.f;
    if (write_grad)
      for (int c = tid; c < V; c += 256) row[c] = 0.f;
    return;
  }
  if constexpr (SMOOTH) {
    __shared__ float red_sum[4];
    block_row_sum_stage(row, V, red_sum);
    const float lse = block_row_lse(row, V, red);
    const int tgt = target[r] - 1;
    const float invV = 1.f / (float)V;
    if (tid == 0) {
      const float tot = (red_sum[0] + red_sum[1]) + (red_sum[2] + red_sum[3]);
      loss_rows[r] = (lse - row[tgt]) + smooth * (row[tgt] - tot * invV);
    }
    if (write_grad) {
      __syncthreads();
      for (int c = tid; c < V; c += 256)
        row[c] = expf(row[c] - lse) - (c == tgt ? 1.f : 0.f) + smooth * ((c == tgt ? 1.f : 0.f) - invV);
    }
  } else {
    const float lse = block_row_lse(row, V, red);
    const int tgt = target[r] - 1;
    if (tid == 0) loss_rows[r] = lse - row[tgt];
    if (write_grad) {
      __syncthreads();
      for (int c = tid; c < V; c += 256) row[c] = expf(row[c] - lse) - (c == tgt ? 1.f : 0.f);
    }
  }
}
__global__ void __launch_bounds__(256)
logsoftmax_nll_kernel(float* __restrict__ logits, long ld, int V, const int* __restrict__ tok_in,
                      const int* __restrict__ target, float* __restrict__ loss_rows, int write_grad) {
  logsoftmax_nll_body<false>(logits, ld, V, tok_in, target, loss_rows, write_grad, 0.f);
}
__global__ void __launch_bounds__(256)
logsoftmax_nll_smooth_kernel(float* __restrict__ logits, long ld, int V, const int* __restrict__ tok_in,
                             const int* __restrict__ target, float* __restrict__ loss_rows, int write_grad, float smooth) {
  logsoftmax_nll_body<true>(logits, ld, V, tok_in, target, loss_rows, write_grad, smooth);
}

// in-place log-softmax of `rows` rows of V logits (decoders/gen.lua:24 at sampling / beam-search time)
__global__ void __launch_bounds__(256)
log_softmax_rows_kernel(float* __restrict__ x, long ld, int V) {
  __shared__ float red[8];
  float* row = x + (long)blockIdx.x * ld;
  const int tid = threadIdx.x;
  const float lse = block_row_lse(row, V, red);
  for (int c = tid; c < V; c += 256) row[c] -= lse;
}

extern "C" {

int vd_log_softmax_rows(float* x, int64_t ld, int64_t rows, int V, void* stream) {
  VD_CHECK_ARG(x && rows >= 0 && V >= 1 && ld >= V, "vd_log_softmax_rows: bad args");
  if (rows == 0) return VD_OK;
  hipLaunchKernelGGL(log_softmax_rows_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, (long)ld, V);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

int vd_logsoftmax_nll(float* logits, int64_t ld, int64_t rows, int V, const int32_t* tok_in,
                      const int32_t* target, float* loss_rows, int write_grad, void* stream) {
  VD_CHECK_ARG(logits && tok_in && target && loss_rows && rows >= 0 && V >= 1 && ld >= V,
               "vd_logsoftmax_nll: bad args");
  if (rows == 0) return VD_OK;
  hipLaunchKernelGGL(logsoftmax_nll_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, logits,
                     (long)ld, V, tok_in, target, loss_rows, write_grad);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

// gt: 0-based ground-truth option per round, or null for scores only.
// dOptH/dEnc: null for forward-only.  gscale = 1/N_global (CrossEntropyCriterion sizeAverage).
int vd_score_ce(const float* optH, const float* enc, const int32_t* gt, float* scores, float* loss_rows,
                float* dOptH, float* dEnc, int N, int O, int H, float gscale, void* stream) {
  VD_CHECK_ARG(optH && enc && scores && N >= 0 && O >= 1 && O <= MAX_OPT && H % 4 == 0,
               "vd_score_ce: bad args (O=%d must be <= %d)", O, MAX_OPT);
  VD_CHECK_ARG(gt == nullptr || loss_rows != nullptr, "vd_score_ce: loss_rows required with gt");
  VD_CHECK_ARG((dOptH == nullptr) == (dEnc == nullptr), "vd_score_ce: dOptH and dEnc go together");
  VD_CHECK_ARG(score_ce_aligned(optH, enc, dOptH, dEnc), "vd_score_ce: pointer must be 16-byte aligned and leading dimension a multiple of 4 (optH, enc, dOptH, dEnc; H=%d)", H);
  VD_CHECK_ARG(dOptH == nullptr || gt != nullptr, "vd_score_ce: gradients need gt");
  if (N == 0) return VD_OK;
  hipLaunchKernelGGL(score_ce_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, optH, enc, gt, scores,
                     loss_rows, dOptH, dEnc, O, H, gscale);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

int vd_ranks(const float* scores, int32_t* ranks, int N, int O, void* stream) {
  VD_CHECK_ARG(scores && ranks && N >= 0 && O >= 1 && O <= MAX_OPT, "vd_ranks: bad args");
  if (N == 0) return VD_OK;
  hipLaunchKernelGGL(ranks_kernel, dim3(N), dim3(128), 0, (hipStream_t)stream, scores, ranks, O);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

}  // extern "C"

// internal (rt_core.h): the two training heads with label smoothing `smooth` in [0, 1) (LS1 / LS2 above); smooth = 0 is the C-ABI entry
// point, kernel and arguments (LS4)
int vd_score_ce_p(const float* optH, const float* enc, const int32_t* gt, float* scores, float* loss_rows, float* dOptH, float* dEnc, int N,
                  int O, int H, float gscale, float smooth, hipStream_t stream) {
  VD_CHECK_ARG(smooth >= 0.f && smooth < 1.f, "vd_score_ce_p: label smoothing %g is not in [0, 1)", (double)smooth);
  if (smooth == 0.f) return vd_score_ce(optH, enc, gt, scores, loss_rows, dOptH, dEnc, N, O, H, gscale, stream);
  VD_CHECK_ARG(optH && enc && scores && gt && loss_rows && N >= 0 && O >= 1 && O <= MAX_OPT && H % 4 == 0,
               "vd_score_ce_p: bad args (O=%d must be <= %d; the smoothed head needs gt and loss_rows)", O, MAX_OPT);
  VD_CHECK_ARG((dOptH == nullptr) == (dEnc == nullptr), "vd_score_ce_p: dOptH and dEnc go together");
  VD_CHECK_ARG(score_ce_aligned(optH, enc, dOptH, dEnc), "vd_score_ce_p: pointer must be 16-byte aligned and leading dimension a multiple of 4 (optH, enc, dOptH, dEnc; H=%d)", H);
  if (N == 0) return VD_OK;
  hipLaunchKernelGGL(score_ce_smooth_kernel, dim3(N), dim3(256), 0, stream, optH, enc, gt, scores, loss_rows, dOptH, dEnc, O, H, gscale,
                     smooth);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

// internal (rt_core.h): the discriminative training head on the targets of DT3 / DT4 (rel [N x O], validated by the host: DT1); gscale = 1 / W
int vd_score_ce_dense_p(const float* optH, const float* enc, const int32_t* gt, const float* rel, float* scores, float* loss_rows,
                        float* dOptH, float* dEnc, int N, int O, int H, float gscale, float mix, hipStream_t stream) {
  VD_CHECK_ARG(optH && enc && scores && gt && rel && loss_rows && N >= 0 && O >= 1 && O <= MAX_OPT && H % 4 == 0,
               "vd_score_ce_dense_p: bad args (O=%d must be <= %d; the dense head needs gt, rel and loss_rows)", O, MAX_OPT);
  VD_CHECK_ARG((dOptH == nullptr) == (dEnc == nullptr), "vd_score_ce_dense_p: dOptH and dEnc go together");
  VD_CHECK_ARG(score_ce_aligned(optH, enc, dOptH, dEnc), "vd_score_ce_dense_p: pointer must be 16-byte aligned and leading dimension a multiple of 4 (optH, enc, dOptH, dEnc; H=%d)", H);
  VD_CHECK_ARG(mix >= 0.f && mix <= 1.f, "vd_score_ce_dense_p: the mix %g is not in [0, 1]", (double)mix);
  if (N == 0) return VD_OK;
  hipLaunchKernelGGL(score_ce_dense_kernel, dim3(N), dim3(256), 0, stream, optH, enc, gt, scores, loss_rows, dOptH, dEnc, O, H, gscale, mix,
                     rel);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

// internal (rt_core.h): the dense head of a live step (DL3): optH / dOptH [n_live * O x H] hold the rows of the live rounds in live order,
// live_slot [N] (device) = a round's place among them or -1; everything else as vd_score_ce_dense_p, which live_slot[n] = n reproduces
int vd_score_ce_dense_live_p(const float* optH, const float* enc, const int32_t* gt, const float* rel, const int32_t* live_slot, float* scores,
                             float* loss_rows, float* dOptH, float* dEnc, int N, int O, int H, float gscale, float mix, hipStream_t stream) {
  VD_CHECK_ARG(optH && enc && scores && gt && rel && live_slot && loss_rows && N >= 0 && O >= 1 && O <= MAX_OPT && H % 4 == 0,
               "vd_score_ce_dense_live_p: bad args (O=%d must be <= %d; the live dense head needs gt, rel, live_slot and loss_rows)", O, MAX_OPT);
  VD_CHECK_ARG((dOptH == nullptr) == (dEnc == nullptr), "vd_score_ce_dense_live_p: dOptH and dEnc go together");
  VD_CHECK_ARG(score_ce_aligned(optH, enc, dOptH, dEnc), "vd_score_ce_dense_live_p: pointer must be 16-byte aligned and leading dimension a multiple of 4 (optH, enc, dOptH, dEnc; H=%d)", H);
  VD_CHECK_ARG(mix >= 0.f && mix <= 1.f, "vd_score_ce_dense_live_p: the mix %g is not in [0, 1]", (double)mix);
  if (N == 0) return VD_OK;
  hipLaunchKernelGGL(score_ce_dense_live_kernel, dim3(N), dim3(256), 0, stream, optH, enc, gt, scores, loss_rows, dOptH, dEnc, O, H, gscale,
                     mix, rel, live_slot);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

// internal (rt_core.h): DL3's token compaction: out [To x n_live * O] from tok [To x rows], uid [N * O] or null, live_idx [n_live] (device)
int vd_dense_live_tokens_p(const int32_t* tok, int64_t rows, int To, const int32_t* uid, const int32_t* live_idx, int n_live, int O,
                           int32_t* out, hipStream_t stream) {
  VD_CHECK_ARG(tok && live_idx && out && rows >= 1 && To >= 1 && n_live >= 0 && O >= 1, "vd_dense_live_tokens_p: bad args");
  const long live_rows = (long)n_live * O, total = (long)To * live_rows;
  VD_CHECK_ARG((total + 255) / 256 <= 0x7fffffffL, "vd_dense_live_tokens_p: %ld elements are more than one launch covers", total);
  if (total == 0) return VD_OK;
  hipLaunchKernelGGL(dense_live_tokens_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, tok, (long)rows, uid, live_idx, O,
                     live_rows, total, out);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

// internal (rt_core.h): DT2, ndcg [N] doubles from scores and rel [N x O]
int vd_ndcg_p(const float* scores, const float* rel, double* ndcg, int N, int O, hipStream_t stream) {
  VD_CHECK_ARG(scores && rel && ndcg && N >= 0 && O >= 1 && O <= MAX_OPT, "vd_ndcg_p: bad args");
  if (N == 0) return VD_OK;
  hipLaunchKernelGGL(ndcg_kernel, dim3(N), dim3(128), 0, stream, scores, rel, ndcg, O);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

int vd_logsoftmax_nll_p(float* logits, int64_t ld, int64_t rows, int V, const int32_t* tok_in, const int32_t* target, float* loss_rows,
                        int write_grad, float smooth, hipStream_t stream) {
  VD_CHECK_ARG(smooth >= 0.f && smooth < 1.f, "vd_logsoftmax_nll_p: label smoothing %g is not in [0, 1)", (double)smooth);
  if (smooth == 0.f) return vd_logsoftmax_nll(logits, ld, rows, V, tok_in, target, loss_rows, write_grad, stream);
  VD_CHECK_ARG(logits && tok_in && target && loss_rows && rows >= 0 && V >= 1 && ld >= V, "vd_logsoftmax_nll_p: bad args");
  if (rows == 0) return VD_OK;
  hipLaunchKernelGGL(logsoftmax_nll_smooth_kernel, dim3((unsigned)rows), dim3(256), 0, stream, logits, (long)ld, V, tok_in, target,
                     loss_rows, write_grad, smooth);
  VD_LAUNCH_CHECK();
  return VD_OK;
}
