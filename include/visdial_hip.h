/* visdial_hip.h -- C ABI of libvisdial_hip.so (MI355X / gfx950).
 *
 * The reference (batra-mlp-lab/visdial) is Lua/Torch7; its only native boundary is the
 * LuaJIT-FFI call into THNN in model_utils/MaskSoftMax.lua:16-19,35-40.  Every arithmetic
 * op on its training hot path lives in un-vendored Lua rocks (nn, rnn, cunn).  This header is
 * the operator-level boundary that replaces those calls: each entry point names the reference
 * module call it stands in for (file:line under /root/reference).  A host (LuaJIT ffi.cdef,
 * Python ctypes, ...) composes them exactly as encoders/<name>.lua / decoders/<name>.lua compose nn
 * modules; see INTEGRATION.md for the Lua-side binding.
 *
 * Conventions
 *  - plain C types only; all pointers are DEVICE pointers unless the name says host.
 *  - every function returns 0 on success, <0 on error (never throws / longjmps);
 *    vd_last_error() returns a thread-local message.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); calls only enqueue.
 *  - caller owns every buffer; float buffers must be 16-byte aligned, row strides multiples of 4.
 *  - fp32 throughout (IEEE, exact-fp32 MFMA); token ids are int32, 0 = padding; byte masks are uint8.
 *  - LSTM weights follow nn.SeqLSTM: weight [(D+H) x 4H] = [Wx ; Wh], gate column order i,f,o,g;
 *    nn.Linear weights are [out x in]; the embedding table is [(V+1) x E] with row 0 = pad (zero).
 */
#ifndef VISDIAL_HIP_H
#define VISDIAL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VD_ACT_NONE 0
#define VD_ACT_TANH 1

/* ---- library ------------------------------------------------------------------------- */
const char* vd_last_error(void);
/* Bumped whenever an exported symbol is removed or the meaning of an argument changes; hosts compare it with the VD_ABI_VERSION they
 * were written against right after loading (visdial_amd/_lib.py, lua/visdial_ffi.lua).  2 = round 4's surface: vd_tune_set /
 * vd_tune_clear / vd_lstm_seq_status removed, vd_model_params.lstmBf16 also takes 3 / 6 / 9 (exact-operand split).  Adding entry points
 * does not bump it: 101 entry points (61 operator-level, 33 model-level, 7 vd_comm_*), vd_beam_* / vd_model_beam_search,
 * vd_sample_* / vd_model_sample and vd_lhood_* / vd_model_retrieve_lhood added under 2. */
#define VD_ABI_VERSION 2
int vd_abi_version(void);
int vd_device_count(int* count);
int vd_set_device(int device);                 /* replaces cutorch.setDevice, train.lua:19 */
int vd_device_info(int device, char* name256, char* arch256, int* num_cus, int64_t* hbm_bytes);
int vd_malloc(void** ptr, int64_t bytes);      /* for hosts without a tensor library (Lua) */
int vd_free(void* ptr);
int vd_memset(void* ptr, int value, int64_t bytes, void* stream);
int vd_memcpy_h2d(void* dst, const void* src_host, int64_t bytes, void* stream); /* :cuda() dataloader.lua:410-416 */
int vd_memcpy_d2h(void* dst_host, const void* src, int64_t bytes, void* stream);
int vd_memcpy_d2d(void* dst, const void* src, int64_t bytes, void* stream);
int vd_stream_synchronize(void* stream);
/* strided 2-D device copy of rows x cols floats (nn.JoinTable / nn.Narrow on column blocks,
 * encoders/lf-ques-im-hist.lua:49-55) */
int vd_copy_2d(float* dst, int64_t dst_ld, const float* src, int64_t src_ld, int64_t rows, int64_t cols,
               void* stream);

/* `flags` of the contraction / recurrence entry points: VD_FLAG_BF16 rounds the GEMM operands to bf16 (RNE) and
 * multiplies them on the bf16 MFMA with fp32 accumulation -- the opt-in "bf16 LSTM step" of BASELINE.json
 * configs[4].  0 = exact fp32 (the reference's arithmetic, the headline configuration). */
#define VD_FLAG_BF16 1
/* VD_FLAG_SPLIT9 (vd_lstm_forward / vd_lstm_backward, throughput shapes): the recurrent product h*Wh / da*Wh^T as the EXACT
 * three-way bf16 split of both fp32 operands -- nine bf16 MFMAs with fp32 accumulation per fp32 one, every product exact
 * (csrc/split_core.h): fp32-grade results at 9/16 of the matrix-pipe time.  Opt-in; VD_FLAG_SPLIT6 / VD_FLAG_SPLIT3 drop the
 * smallest products (NOT fp32-grade: they exist for the error table of tests/test_ops_gpu.py). */
#define VD_FLAG_SPLIT9 2
#define VD_FLAG_SPLIT6 4
#define VD_FLAG_SPLIT3 8
/* VD_FLAG_LIVE_PREFIX (vd_lstm_forward, with tok_mask): the caller promises that at every step the rows with tok_mask != 0 are a
 * PREFIX of the N rows (sequences left-aligned and ordered by descending length).  Row groups that hold no live row are then not
 * computed and their gates / h / c rows are left UNWRITTEN.  A group is the row tile of the step kernel that runs (32 or 128 rows);
 * VD_LIVE_PREFIX_ROWS is a multiple of every forward step kernel's row tile: rows at or beyond ceil(live rows of the step /
 * VD_LIVE_PREFIX_ROWS) * VD_LIVE_PREFIX_ROWS are never written, whichever kernel ran.  A group with a live row computes exactly
 * what it computes without the flag, its pad rows included (zeroed by tok_mask).  Exact fp32 only: together with VD_FLAG_BF16 or a
 * VD_FLAG_SPLIT* the call is refused with an argument error. */
#define VD_FLAG_LIVE_PREFIX 16
#define VD_LIVE_PREFIX_ROWS 128
/* VD_FLAG_STATE_ONLY (vd_lstm_forward): a forward pass that no backward follows.  `gates` must be NULL and `h` / `c` are
 * [2 x N x H] ping-pong buffers: step t reads slot (t - 1) & 1 (h0 / c0 / zeros at t = 0) and writes slot t & 1, so on return the
 * final state lies in slot (T - 1) & 1.  The gate activations and the cell update stay in registers: no gate value reaches memory
 * (4 KB instead of 12 KB written per row and step at H = 512).  Same step kernels, tile shapes and arithmetic as the saving call:
 * for equal (T, N, H, flags) and inputs the final h and c equal the saving call's last step bit for bit.  Combines with flags 0
 * and VD_FLAG_SPLIT*, dense and table mode, tok_mask; refused (argument error) with VD_FLAG_BF16, with VD_FLAG_LIVE_PREFIX and
 * with a non-NULL `gates`.  Without the flag a NULL `gates` is refused. */
#define VD_FLAG_STATE_ONLY 32
/* VD_FLAG_TREE (vd_lstm_forward): a level-by-level recurrence over a forest -- every row of step t continues the state of a PARENT ROW
 * of step t - 1, not of the same row (the candidates of generative retrieval as a prefix tree of their tokens: a shared beginning is
 * computed once).  tok_mask is required and is [2 x T x N]: plane 0 is the mask (in table mode also passed as tok_gather: the token),
 * non-zero = a node, and the nodes of step t are a PREFIX of the N rows (level widths may grow or shrink from step to step); plane 1
 * is the parent row of node (t, n) -- for t >= 1 a row of step t - 1, for t = 0 a row of h0 / c0, which may then have any number of
 * rows R (R * H * 4 bytes below 4 GB; with NULL h0 / c0 the parent state is zero).  Parent entries of rows without a node are not
 * read as rows.  Forward only: `gates` must be NULL and no gate activation reaches memory (as with VD_FLAG_STATE_ONLY); h and c are
 * [T x N x H], every level is kept.  Row tiles without a node return before loading anything and their rows stay unwritten, with the
 * guarantee of VD_FLAG_LIVE_PREFIX: rows at or beyond ceil(nodes of the step / VD_LIVE_PREFIX_ROWS) * VD_LIVE_PREFIX_ROWS are never
 * written; the other rows without a node in a tile with one are written as zeros.  Dense and table mode; a second layer reads layer
 * 1's h of the same node row as dense xproj input.  Same step kernels, tiles and K order as VD_FLAG_LIVE_PREFIX: with identity parents
 * h and c equal that flag's bit for bit.  Exact fp32 only: refused (argument error) with VD_FLAG_BF16, any VD_FLAG_SPLIT*,
 * VD_FLAG_STATE_ONLY, a non-NULL `gates` or a NULL tok_mask. */
#define VD_FLAG_TREE 64
/* VD_FLAG_HOLD (vd_lstm_forward): a row whose tok_mask entry is 0 at step t KEEPS (h, c) of step t - 1 -- (h0, c0) at t = 0, zero with
 * NULL h0 / c0 -- instead of being zeroed: the recurrence continued from a carried state over right-aligned windows of new tokens (the
 * prefix property of a concatenated history, csrc/beam.hip CH6).  A live row is the plain cell.  tok_mask ([T x N]) is required.  Forward
 * only: `gates` must be NULL and no gate activation reaches memory; h and c are [T x N x H] and hold the running state of every row at
 * every step (a held row writes what it kept), so row n of h [T - 1] is the state after the row's last token.  Dense and table mode.  It
 * runs the exact fp32 step kernels at any N -- the distributed split-K epilogue below 2048 rows, the register-staged generic kernel from
 * there on; the LDS-DMA pipeline has no form of this epilogue and a HOLD pass is routed away from it.  Refused (argument error) with every
 * other flag -- VD_FLAG_BF16, any VD_FLAG_SPLIT*, VD_FLAG_LIVE_PREFIX, VD_FLAG_STATE_ONLY, VD_FLAG_TREE --, a non-NULL `gates` or a NULL
 * tok_mask. */
#define VD_FLAG_HOLD 128

/* ---- dense contractions (nn.Linear / hoisted SeqLSTM input projection / weight grads) -- */
/* C[MxN] (+)= act(A[MxK] * W[NxK]^T + bias)   -- nn.Linear:updateOutput (+nn.Tanh),
 * e.g. encoders/mn-att-ques-im-hist.lua:64-65,77,88,106; also dX = dA * Wh^T style products.
 * accumulate: 0 = overwrite, 1 = C += (plain read-modify-write), 2 = C += with float atomics (C has other
 * concurrent atomic writers: the shared embedding gradient) */
int vd_gemm_nt(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias, float* C,
               int64_t ldc, int M, int N, int K, int act, int accumulate, void* stream);
/* C[MxN] (+)= A[MxK] * B[KxN] + bias           -- x*Wx+b of nn.SeqLSTM (mn-att:27-41), nn.Linear:updateGradInput */
int vd_gemm_nn(const float* A, int64_t lda, const float* B, int64_t ldb, const float* bias, float* C,
               int64_t ldc, int M, int N, int K, int accumulate, void* stream);
/* C[MxN] += A[KxM]^T * B[KxN]                  -- accGradParameters of nn.Linear / nn.SeqLSTM */
int vd_gemm_tn_acc(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int M,
                   int N, int K, int flags, void* stream);
/* C[MxN] += sum_k A[a_rows[k], :M]^T * B[b_rows[k], :N], k < K  -- the same accGradParameters contraction over an
 * explicit list of (row of A, row of B) pairs: nn.SeqLSTM:maskZero() zeroes the gradient of padded (timestep, row)
 * pairs (encoders/mn-att-ques-im-hist.lua:27-41), so only the non-pad pairs are contracted (~55 % of T*N) */
int vd_gemm_tn_rows_acc(const float* A, int64_t lda, const int32_t* a_rows, const float* B, int64_t ldb,
                        const int32_t* b_rows, float* C, int64_t ldc, int M, int N, int K, void* stream);
/* out[N] += column sums of X[MxN]              -- gradBias */
int vd_colsum_acc(const float* X, int64_t ld, int M, int N, float* out, void* stream);

/* ---- nn.SeqLSTM (Element-Research rnn; call sites mn-att:27-45, disc.lua:4-15, gen.lua:17-22,
 *      lf-ques.lua:18-24, hre-ques-im-hist.lua:34,74,92) ---------------------------------------- */
/* Recurrence over T steps, time-major.  The input projection (x_t*Wx + b) is supplied already
 * computed: dense mode xproj[t] = xproj + t*x_tstride, row n at +n*x_ld ([N x 4H]); table mode
 * (tok_gather != NULL, [T x N]): row = xproj + tok_gather[t,n]*x_ld (xproj = Emb*Wx+b, [V+1 x 4H]).
 * tok_mask ([T x N] or NULL) implements :maskZero(): rows with token 0 get h = c = gates = 0.
 * h0/c0 ([N x H] or both NULL = zeros) are userPrevOutput/userPrevCell (gen.lua:32-38).
 * Outputs: gates [T x N x 4H] post-activation (i,f,o,g), h and c [T x N x H].
 * Limits: one step's slice of every tensor below 4 GB (N * 4H * 4 bytes; a projection table: its rows * x_ld * 4 bytes --
 * 524 288 table rows at H = 512): the epilogue uses 32-bit byte offsets.  Larger batches: call per row range.
 * One kernel launch per step.  Throughput shapes (N >= 2048) take the LDS-DMA pipeline (csrc/lstm.hip), which multiplies
 * by a gate-interleaved transpose of Wh [4H x H] made once per call; that work buffer is library-owned per (device, stream),
 * so calls on different streams may overlap.
 * flags: VD_FLAG_BF16 / VD_FLAG_SPLIT* choose the arithmetic of the recurrent product; VD_FLAG_LIVE_PREFIX (above) skips the
 * row groups without a live row; VD_FLAG_STATE_ONLY (above) keeps only the running state (gates NULL, h / c [2 x N x H]);
 * VD_FLAG_TREE (above) runs a forest level by level (gates NULL, tok_mask [2 x T x N] = mask | parent row); VD_FLAG_HOLD (above)
 * holds the state of a masked row instead of zeroing it (gates NULL, alone among the flags). */
int vd_lstm_forward(const float* xproj, int64_t x_tstride, int64_t x_ld, const int32_t* tok_gather,
                    const int32_t* tok_mask, const float* Wh, const float* h0, const float* c0, float* gates,
                    float* h, float* c, int T, int N, int H, int flags, void* stream);
/* Backward through time.  gates is overwritten IN PLACE by da (gradient w.r.t. the pre-activation
 * gates, = gradient of xproj).  dh_seq [T x N x H] or NULL: gradient arriving at every h_t;
 * dh_last [N x H] or NULL: extra gradient at h_{T-1} (nn.Select(1,-1)); dc_last or NULL:
 * userNextGradCell (gen.lua:49).  dc_work [N x H] scratch, on return = dL/dc0 (userGradPrevCell);
 * dh0 [N x H] or NULL receives dL/dh0 (userGradPrevOutput, gen.lua:50-58).
 * h_seq [T x N x H] + dWh_acc [H x 4H] (both or neither): also accumulate the recurrent weight gradient
 * dWh += sum_{t>=1} h_{t-1}^T da_t (accGradParameters). */
int vd_lstm_backward(const float* Wh, float* gates, const float* c, const float* c0, const float* dh_seq,
                     const float* dh_last, const float* dc_last, float* dc_work, float* dh0, const float* h_seq,
                     float* dWh_acc, int T, int N, int H, int flags, void* stream);


/* Two stacked nn.SeqLSTM layers (the pattern of every encoder branch: mn-att:27-45, lf-ques.lua:17-24)
 * advanced as a skewed wavefront, up to 2 independent stacks per call (history + question branches):
 * tick tau launches ONE grouped kernel doing L1 step tau, the layer-2 input projection of step tau-1
 * and L2 step tau-2 of every stack, so a T-step stack costs T+2 launches instead of 2T.
 * Forward: gates1 must hold x*Wx1+b1 on entry (vd_gemm_nn); outputs as vd_lstm_forward for both layers.
 * Backward: gates1/gates2 are overwritten by da1/da2; dh_last2 [N x H] is the gradient at the top
 * layer's last step; dh1_seq [T x N x H], dc1, dc2 [N x H] are scratch.  Weight gradients are then
 * formed by the caller with vd_gemm_tn_acc / vd_colsum_acc exactly as for vd_lstm_backward.
 * Live-row counts (nact != NULL).  The rows are sorted by decreasing length and a row is pad BEFORE its first token, so the
 * counts are NON-DECREASING in t, each in [0, N]; both entries refuse a count outside [0, N] and the backward entry refuses
 * counts that decrease (VD_ERR_ARG, nothing is written).  Inside its span a row is still masked per token by tok_mask.
 * Only rows [0, nact[t]) of step t are read or written; the CALLER zero-fills what the skipped (t, row) pairs must read as:
 *   forward:  rows >= nact[t] of gates1 (vd_zero_inactive_rows), and h1, c1, gates2, h2, c2 (whole buffers or those rows);
 *   backward: nothing more -- gates1 / gates2 / c1 / c2 come from that forward; rows >= nact[t] of da1, da2 and dh1_seq
 *             stay as they were (zero in gates1 / gates2, so the weight-gradient contractions may run over every row).
 * dc1 / dc2 on return: without counts dL/dc0 of each layer, all N rows.  With counts, rows < nact[T-1] only (the others are
 * not written): a row that is live from step t0 on holds the cell gradient flowing INTO step t0, which is dL/dc0 of its own
 * sequence (its state before t0 is zero); for t0 = 0 that is dL/dc0. */
typedef struct {
  int T, N;
  const int32_t* tok_mask;               /* [T x N] or NULL (maskZero) */
  const float *Wh1, *Wx2, *b2, *Wh2;
  float *gates1, *h1, *c1, *gates2, *h2, *c2;
  const int32_t* nact;                   /* HOST int32[T] or NULL.  Rows sorted by sequence length: only rows
                                            [0, nact[t]) are non-pad at step t and are computed; the caller
                                            zero-fills the rest (vd_zero_inactive_rows / memset).  Non-decreasing
                                            in t, 0 <= nact[t] <= N (see above) */
} vd_lstm2_fwd_t;
typedef struct {
  int T, N;
  const float *Wh1, *Wx2, *Wh2;
  float* gates1;
  const float* c1;
  float* gates2;
  const float* c2;
  const float* dh_last2;
  float* dh1_seq;
  float *dc1, *dc2;
  const int32_t* nact;                   /* HOST int32[T] or NULL, as in vd_lstm2_fwd_t: non-decreasing in t (checked),
                                            0 <= nact[t] <= N; dc1 / dc2 are written for rows < nact[T-1] only */
} vd_lstm2_bwd_t;
int vd_lstm2_forward(const vd_lstm2_fwd_t* stacks, int nstacks, int H, void* stream);
int vd_lstm2_backward(const vd_lstm2_bwd_t* stacks, int nstacks, int H, void* stream);
/* the same wavefront with a pass's arithmetic: flags = 0 (fp32 MFMA, = the two calls above) or VD_FLAG_BF16 (both operands of every
 * recurrent product rounded to bf16 while staged, fp32 accumulate and state: the encoder ticks of a `lstmPrecision = bf16` pass) */
int vd_lstm2_forward_flags(const vd_lstm2_fwd_t* stacks, int nstacks, int H, int flags, void* stream);
int vd_lstm2_backward_flags(const vd_lstm2_bwd_t* stacks, int nstacks, int H, int flags, void* stream);

/* zero rows [nact[t], N) of every time slice of a [T x N x ld] buffer (nact_dev: DEVICE int32[T]).
 * float4 stores: buf 16-byte aligned; ncols, ld and tstride multiples of 4 (refused otherwise) */
int vd_zero_inactive_rows(float* buf, int64_t tstride, int64_t ld, int ncols, const int32_t* nact_dev, int T,
                          int N, void* stream);

/* ---- nn.LookupTableMaskZero / nn.Dropout / small glue ------------------------------------- */
/* out[r,:] = emb[tok[r],:] * (mask ? mask*scale : 1)        mn-att:21,24-25; disc.lua:12
 * E % 4 == 0, emb and out 16-byte aligned, mask 4-byte aligned (refused otherwise) */
int vd_embed_gather(const float* emb, const int32_t* tok, const uint8_t* mask, float* out, int64_t rows,
                    int E, float scale, void* stream);
/* demb[tok[r],:] += dx[r,:] * mask*scale                    LookupTable:accGradParameters */
int vd_embed_scatter_acc(float* demb, const int32_t* tok, const uint8_t* mask, const float* dx, int64_t rows,
                         int E, float scale, void* stream);
/* nn.MaskTime (model_utils/MaskTime.lua:12-40): out[t,n,:] = tok[t,n] != 0 ? feat[n,:] : 0, and its
 * backward dfeat[n,:] = sum_t (tok[t,n] != 0) * dout[t,n,:]   (encoders/hre-ques-im-hist.lua:50-53) */
int vd_mask_time_forward(const float* feat, const int32_t* tok, float* out, int T, int N, int D, void* stream);
int vd_mask_time_backward(const float* dout, const int32_t* tok, float* dfeat, int T, int N, int D,
                          void* stream);
/* counting sort of token ids (prepares the option-table gradient); offset int32[V+1],
 * work int32[2V], perm int32[n] */
int vd_token_sort(const int32_t* tok, int64_t n, int V, int32_t* offset, int32_t* work, int32_t* perm,
                  void* stream);
/* out[tok[r], 0:ncol] += X[r, 0:ncol] for all n rows; X 16-byte aligned, ncol, ldx and ldo multiples of 4 */
int vd_segment_rowsum_acc(const float* X, int64_t ldx, const int32_t* tok, const int32_t* perm, int64_t n,
                          int ncol, float* out, int64_t ldo, void* stream);
/* Bernoulli(1-p) keep-mask bytes from a counter-based generator (nn.Dropout noise) */
int vd_dropout_mask(uint8_t* mask, int64_t n, uint64_t seed, float p, void* stream);
/* y = x*mask*scale (nn.Dropout forward and backward) */
int vd_dropout_apply(const float* x, const uint8_t* mask, float* y, int64_t n, float scale, void* stream);
/* dx = dy*(1-y^2) (nn.Tanh:updateGradInput) */
int vd_tanh_backward(const float* dy, const float* y, float* dx, int64_t n, void* stream);
/* c = alpha*a + beta*b (b may be NULL)  (nn.CAddTable and gradient fan-in) */
int vd_axpby(const float* a, const float* b, float* c, int64_t n, float alpha, float beta, void* stream);

/* ---- memory-network attention: nn.MM(false,true) -> nn.MaskSoftMax -> nn.MM
 *      (mn-att:48-62; model_utils/MaskSoftMax.lua:5-46; mask from model.lua:280-294, 1 = hidden) */
int vd_mn_attention_forward(const float* Q, const float* Hm, const uint8_t* mask, float* P, float* hAtt, int B,
                            int R, int H, void* stream);
int vd_mn_attention_backward(const float* Q, const float* Hm, const float* P, const float* dhAtt, float* dQ,
                             float* dHm, int B, int R, int H, void* stream);

/* history attention of encoders/hrea-ques-im-hist.lua:83-131 (Linear(H,1) scores, Replicate+CAddTable,
 * model_utils/MaskFuture.lua, model_utils/ReplaceZero.lua(-inf), SoftMax, CMulTable+Sum):
 * sq, sh [B*R] scores; Hm [B x R x H]; P [B x R x R]; att [B x R x H] */
int vd_hrea_attention_forward(const float* sq, const float* sh, const float* Hm, float* P, float* att, int B, int R,
                              int H, void* stream);
int vd_hrea_attention_backward(const float* Hm, const float* P, const float* datt, float* dsq, float* dsh,
                               float* dHm, int B, int R, int H, void* stream);
/* nn.Linear(H, 1) (hrea:83-85): out[n] = <x[n,:], w> + b; backward accumulates dw, db and writes dx */
int vd_rowdot_forward(const float* x, const float* w, const float* bias, float* out, int N, int H, void* stream);
int vd_rowdot_backward(const float* x, const float* w, const float* dout, float* dw, float* db, float* dx, int N,
                       int H, void* stream);

/* ---- SAN image attention (mn-att:68-104).  pre = tanh(Linear(img)) per IMAGE [B*S2 x H];
 *      mask1/mask2 = dropout keep-masks of img_tr / img_ques_common per ROUND (NULL in evaluate()) */
int vd_img_common_forward(const float* pre, const uint8_t* mask1, const float* Wc, const float* bc,
                          const float* qc, const uint8_t* mask2, float* iqc, int N, int R, int S2, int H, int Kc,
                          float scale, void* stream);
int vd_img_att_forward(const float* iqc, const float* wa, const float* ba, const float* pre,
                       const uint8_t* mask1, const float* u0, float* p, float* u1, int N, int R, int S2, int H,
                       int Kc, float scale, void* stream);
int vd_img_att_backward(float* iqc_dz, const float* wa, const float* pre, const uint8_t* mask1,
                        const uint8_t* mask2, const float* p, const float* datt, float* dwa, float* dba,
                        float* dqc, float* work /* [N x S2] scratch */, int N, int R, int S2, int H, int Kc,
                        float scale, void* stream);
int vd_img_tr_backward(const float* dz, const float* Wc, const float* p, const float* datt,
                       const uint8_t* mask1, float* dpre, int N, int R, int S2, int H, int Kc, float scale,
                       void* stream);
int vd_img_common_wgrad(const float* dz, const float* pre, const uint8_t* mask1, float* dWc, int N, int R,
                        int S2, int H, int Kc, float scale, void* stream);

/* ---- discriminative head: nn.MM + nn.Squeeze (disc.lua:22-29) + nn.CrossEntropyCriterion
 *      (model.lua:37-38,330,334).  gt is 0-based here (the reference's answer_ind is 1-based). */
int vd_score_ce(const float* optH, const float* enc, const int32_t* gt, float* scores, float* loss_rows,
                float* dOptH, float* dEnc, int N, int O, int H, float gscale, void* stream);
/* generative head: nn.Sequencer(nn.MaskZero(nn.LogSoftMax(),1)) (decoders/gen.lua:24) +
 * SequencerCriterion(MaskZeroCriterion(ClassNLLCriterion, sizeAverage=false)) (model.lua:33-36).
 * logits [rows x ld] (V valid columns, ld = V rounded up to 4), tok_in/target int32[rows] (1-based
 * vocabulary ids, 0 = pad).  loss_rows[r] = -log p(target); with write_grad the row is overwritten
 * by d loss / d logits (softmax - onehot, zero rows at pads). */
int vd_logsoftmax_nll(float* logits, int64_t ld, int64_t rows, int V, const int32_t* tok_in,
                      const int32_t* target, float* loss_rows, int write_grad, void* stream);
/* ---- live-row log-likelihood head of generative retrieval (model.lua:392-420 + utils.computeLhood, utils.lua:86-102;
 *      csrc/lhood.hip): the candidate scores of vd_gemm_nt + vd_logsoftmax_nll + a sum over time, computed from the rows that
 *      count only and without a [rows x V] logits buffer.  Deterministic: no atomics, fixed reduction orders.
 *   live_rows  act = the linear indices i in [0, n) with tok_in[i] != 0 and target[i] > 0, ascending (for time-major
 *              [T x rows] tokens: step-major, then row); `work` is device int32[(n + 1023) / 1024 + 1]; *host_count = their
 *              number, returned with ONE stream synchronisation
 *   nll        nll[i] = logsumexp_v(h[act[i]] . W[v] + bias[v]) - (h[act[i]] . W[target[act[i]] - 1] + bias[...]), i < n_act:
 *              h [rows x ldh] (H valid columns), act values in [0, rows), target int32[rows] 1-based vocabulary ids, W [V x ldw],
 *              bias [V] or NULL; fp32 operands on v_mfma_f32, online log-sum-exp.  Two live rows with the same h row and
 *              target get bit-identical values.  n_act = 0 returns at once.
 *   sum        out[(r / C) * ldo + r % C] = -(sum over t of the nll of row t * rows + r, in step order), r < rows; a row of
 *              `act` (ascending, as live_rows writes it) that is absent contributes nothing, a candidate without one scores 0 */
int vd_lhood_live_rows(const int32_t* tok_in, const int32_t* target, int64_t n, int32_t* act, int32_t* work, int32_t* host_count,
                       void* stream);
int vd_lhood_nll(const float* h, int64_t ldh, int64_t rows, const int32_t* act, int64_t n_act, const int32_t* target, const float* W,
                 int64_t ldw, const float* bias, int V, int H, float* nll, void* stream);
int vd_lhood_sum(const float* nll, const int32_t* act, int64_t n_act, int T, int64_t rows, int C, float* out, int64_t ldo,
                 void* stream);
/* in-place nn.LogSoftMax over `rows` rows of V logits (sampling / beam search, model.lua:432-613) */
int vd_log_softmax_rows(float* x, int64_t ld, int64_t rows, int V, void* stream);
/* utils.computeRanks (utils.lua:106-128): 1-based descending-sort position of every option */
int vd_ranks(const float* scores, int32_t* ranks, int N, int O, void* stream);

/* ---- batched beam search (Model:generateAnswers, model.lua:466-573; csrc/beam.hip states the rules).  One group = one QA
 *      round with k = beamSize slots (k <= 32), hypothesis row r = group * k + slot; scores are fp64 [groups x k]; the token
 *      history is int32 [groups x k x beam_len], double-buffered (hist_in != hist_out).
 *   topk         nn.LogSoftMax of logits [rows x ld] (V valid columns; bit-identical to vd_log_softmax_rows) fused with the
 *                top-k of every row, value descending then index ascending (model.lua:524-531); a row whose token tok[r] is 0
 *                is the all-zero row of MaskZero(LogSoftMax) (decoders/gen.lua:24): indices 0..k-1 at 0.  logits are not written.
 *   init         beams[1] = <START>, scores = 0, no finished candidate (model.lua:466-477); tok = <START> for every row
 *   advance      one step s in [1, beam_len): candidates of slot 0 (s = 1) or all slots, <END> ones tracked as the group's best
 *                finished (best_len = 0: none yet), the rest sorted stably and the first min(#, k) kept (model.lua:532-573);
 *                src[r] = source slot of slot r or -1 (keeps its column, score and pre-step state), next_tok = the history
 *                token at s
 *   select_rows  cur[r] = stepped[group(r) * k + src[r]] where src[r] >= 0 (the hidden-state copies of model.lua:556-566)
 *   finish       per group the best finished column and score, else column 0 (the reference errors there) */
int vd_beam_topk(const float* logits, int64_t ld, int64_t rows, int V, const int32_t* tok, int k, int32_t* top_idx, float* top_val,
                 void* stream);
int vd_beam_init(int groups, int k, int beam_len, int start_token, int32_t* hist, int32_t* tok, double* scores, double* best_score,
                 int32_t* best_len, void* stream);
int vd_beam_advance(const int32_t* top_idx, const float* top_val, int groups, int k, int step, int beam_len, int end_token,
                    double* scores, const int32_t* hist_in, int32_t* hist_out, int32_t* src, int32_t* next_tok, double* best_score,
                    int32_t* best_len, int32_t* best_hist, void* stream);
int vd_beam_select_rows(float* cur, const float* stepped, const int32_t* src, int64_t rows, int k, int H, void* stream);
int vd_beam_finish(int groups, int k, int beam_len, const int32_t* hist, const double* scores, const double* best_score,
                   const int32_t* best_len, const int32_t* best_hist, int32_t* out_tokens, double* out_scores, void* stream);

/* ---- batched temperature sampling (Model:generateAnswers with sampleWords = 1, model.lua:576-613; csrc/sample.hip states the
 *      rule).  One hypothesis row per QA round; the token history is int32 [rows x (beam_len + 1)] with column 0 = <START>, the
 *      log-likelihood fp64 [rows], status one int32 (0 = every draw made).  The uniforms are the host's: no device RNG.
 *   init   history <START>, 0, ...; tok = <START>; log-likelihood 0; status 0
 *   draw   step s in [1, beam_len]: nn.LogSoftMax of logits [rows x ld] (V valid columns; bit-identical to vd_log_softmax_rows; a
 *          row whose token tok[r] is 0 is the all-zero row of MaskZero(LogSoftMax)) and the inverse-CDF draw of
 *          RandomState.choice(V, p) from the fp64 weights exp(logp / temperature) with the uniform uniforms[r] in [0, 1) (not
 *          checked here): history column s and tok[r] = the drawn id, the log-likelihood adds its logp until the row has
 *          emitted <END> (the <END> counts).  A row whose weights all underflow sets status = 1 and draws nothing (token 0).
 *          temperature must be finite and > 0; logits are not written. */
int vd_sample_init(int64_t rows, int beam_len, int start_token, int32_t* hist, int32_t* tok, double* loglik, int32_t* status,
                   void* stream);
int vd_sample_draw(const float* logits, int64_t ld, int64_t rows, int V, int32_t* tok, const double* uniforms, double temperature,
                   int step, int beam_len, int end_token, int32_t* hist, double* loglik, int32_t* status, void* stream);

/* ---- wrapperdW:clamp(-5,5) + adam (model.lua:96-99; model_utils/optim_updates.lua:62-91) ---- */
int vd_clamp_adam(float* w, float* g, float* m, float* v, int64_t n, float gscale, float clip, float beta1,
                  float beta2, float eps, float step, void* stream);

/* ======================================================================================================
 * Model-level entry points (csrc/runtime.hip): the whole training / retrieval step behind the ABI, for every plug-in
 * pair of the reference: encoders lf-ques, lf-ques-im, lf-ques-hist, lf-ques-im-hist, lf-att-ques-im-hist,
 * hre-ques-hist, hre-ques-im-hist, hrea-ques-im-hist, mn-ques-hist, mn-ques-im-hist, mn-att-ques-im-hist
 * (encoders/<name>.lua) x decoders disc, gen (decoders/<name>.lua).  A LuaJIT host's model.lua needs only these
 * (INTEGRATION.md): stream fork/join, the skewed two-layer wavefront, the length sort, workspaces, forwardConnect /
 * backwardConnect and launch order live in the library.  One host thread per model; calls enqueue on library-owned
 * streams and block only where a host value is returned (loss, scores, ranks, tensors, log-probabilities).
 * ====================================================================================================== */
typedef struct vd_model vd_model;
typedef struct vd_model_params {   /* the `params` keys Model() consumes: opts.lua:15-40, train.lua:55-59 */
  int32_t vocabSize, embedSize, rnnHiddenSize, imgFeatureSize, imgSpatialSize, commonEmbeddingSize,
          numAttentionLayers, maxQuesCount, numOptions;
  float learningRate, lrDecayRate, minLRate;     /* opts.lua:35-38 */
  uint64_t seed;                                 /* dropout noise stream */
  int32_t lstmBf16;                              /* option recurrence: 0 = fp32 MFMA (a zeroed struct; the hosts' own default is 9); 1 = bf16 operands and compact bf16 state, plus bf16 operands in the encoder's recurrent products and dense weight gradients (configs[4] "bf16 LSTM step"); 9 = exact 3-way bf16 split of both operands, 9 products, in the two step kernels, the dWh contraction and the image attention's three dense products (fp32-grade; what bench.py measures and what -lstmPrecision defaults to in opts.py / lua/model.lua); 6 / 3 = fewer products (data only); vd_model_create rejects any other value */
  int32_t useStreams;                            /* 0 = everything on one stream (debug) */
  int32_t numLayers;                             /* -numLayers (opts.lua:27): lf-*, hre-* encoders and the gen decoder; <1 = 2 */
  int32_t imgEmbedSize;                          /* -imgEmbedSize (opts.lua:24): hre-ques-im-hist, hrea-ques-im-hist */
  float dropout;                                 /* -dropout (opts.lua:29): the fusion Dropout of lf-ques* */
} vd_model_params;
typedef struct vd_batch {          /* HOST pointers, dataloader layout (dataloader.lua:324-339, 378-475) */
  int32_t B, Tq, Th, To;           /* dialogs; trimmed question / history / option lengths (To: columns of options,
                                      or of option_in / option_out for gen retrieval) */
  const int32_t* ques_fwd;         /* [B*R x Tq] right-aligned, 0 = pad */
  const int32_t* hist;             /* [B*R x Th] right-aligned                      (encoders with `hist`) */
  const float* img_feat;           /* [B x S*S x C] attention encoders, [B x F] otherwise (encoders with `im`) */
  const int32_t* options;          /* [B*R x O x To] left-aligned                   (decoder disc) */
  const int32_t* answer_ind;       /* [B*R] 1-based, or NULL (test split) */
  int32_t Ta;                      /* trimmed answer length + 1 */
  const int32_t* answer_in;        /* [B*R x Ta] <START>+tokens, left-aligned       (decoder gen, training) */
  const int32_t* answer_out;       /* [B*R x Ta] tokens+<END> */
  const int32_t* option_in;        /* [B*R x O x To] <START>+tokens                 (decoder gen, retrieval) */
  const int32_t* option_out;       /* [B*R x O x To] tokens+<END> */
} vd_batch;
/* Model:__init (model.lua:10-63): parameter vectors (zeroed), optimiser state, streams.
 * Reads the opt-in switches of the calls below from the environment, once (each is described at its call).  One of them belongs to both
 * rollouts: VD_ROLLOUT_ENCODER = full | round (unset = full; any other value is refused by name).  With `round`, passes 1 .. R - 1 of
 * vd_model_retrieve under VD_RETRIEVE_ROLLOUT = 1 and of vd_model_beam_search under VD_BEAM_ROLLOUT = 1 encode only the round they rank /
 * answer -- history row r of every dialog through the history branch at B rows, then the B rows of the encoder's head on the state the
 * first pass left -- instead of all B * R rounds again: the same picks, answers and ranks, scores within fp32 rounding of the full pass
 * (a product over B rows may take another tile than over B * R).  Ignored where nothing rolls out (neither rollout variable set, or an
 * encoder without a history); with training on, both calls refuse it by name.
 * A second one belongs to both rollouts too: VD_ROLLOUT_CONCAT_END = an integer >= 0 (0 / unset = off; text, a negative value and a value
 * above vocabSize are refused by name).  Any other value is the <END> token id and means CONCATENATED history rows, for the encoders whose
 * history row is the running concatenation of the dialog (lf-ques-hist, lf-ques-im-hist, lf-att-ques-im-hist; an encoder with per-round
 * rows is refused by name): a rollout then writes history row r + 1 as row r's tokens, <END>, the non-zero tokens of question row r and the
 * answer's words, right-aligned in the Th uploaded columns, cut at the end where they do not fit (csrc/beam.hip CH1-CH6) instead of the
 * per-round row.  vd_model_beam_search refuses an end_token that differs from it.  With VD_ROLLOUT_ENCODER = round the later passes continue
 * the two-layer history stack from a carried state over the new tokens alone (vd_lstm_forward with VD_FLAG_HOLD); a model with another
 * number of history layers or bf16 recurrences gets an argument error from the call, never the full-width pass.  Ignored where nothing
 * rolls out. */
int vd_model_create(const vd_model_params* p, const char* encoder, const char* decoder, vd_model** out);
void vd_model_destroy(vd_model* m);
/* wrapper:getParameters() (model.lua:55): flat layout = embed | encoder tensors | decoder tensors, every tensor
 * 16-byte aligned; tensor i = name, element offset, rows x cols */
int64_t vd_model_num_tensors(const vd_model* m);
int64_t vd_model_flat_size(const vd_model* m);
int vd_model_tensor_info(const vd_model* m, int64_t i, char* name64, int64_t* offset, int64_t* rows, int64_t* cols);
/* device pointers of wrapperW, wrapperdW and the Adam moments (for a host-side RCCL all-reduce of wrapperdW) */
int vd_model_flat_pointers(vd_model* m, float** W, float** dW, float** adam_m, float** adam_v);
void* vd_model_stream(vd_model* m);                       /* the main hipStream_t */
/* data-parallel bucketing (new relative to the single-GPU reference): flat element range [lo, hi) of the
 * encoder's own tensors, and "make `stream` wait until those gradients of the last forward_backward are final" -- under
 * a disc decoder that is the end of the encoder backward, well before the option-LSTM backward ends */
int vd_model_encoder_range(const vd_model* m, int64_t* lo, int64_t* hi);
int vd_model_wait_encoder_grads(vd_model* m, void* stream);
/* ---- data-parallel gradient exchange inside the library (csrc/comm.hip).  The reference is
 * single-GPU (train.lua:19); a host that wants N GPUs runs one process per GPU and makes three extra calls: rank 0
 * creates the 128-byte rendezvous token and the host hands it to the peers by any channel it has; every rank joins the
 * RCCL communicator on its current device; then once per step, between forward_backward and update(1/world),
 * vd_model_allreduce_grads sums wrapperdW over all ranks in two buckets -- the encoder's own tensors on a library-owned
 * communication stream underneath the option-LSTM backward, the shared embedding + decoder tensors behind the step --
 * and makes the main stream wait for both.  RCCL (librccl.so.1) is loaded at run time on first use. ---- */
int vd_comm_unique_id(void* out128);                      /* ncclGetUniqueId: 128 bytes */
int vd_comm_init(int rank, int world, const void* id128); /* ncclCommInitRank on the current device (collective) */
int vd_comm_info(int* rank, int* world);                  /* world = 0: no communicator */
int vd_comm_destroy(void);
/* no collective, no device: can this process load RCCL?  version = NCCL_VERSION_CODE of the loaded library (0 = unknown).
 * Hosts exchange the answer over their own channel before any rank enters vd_comm_unique_id / vd_comm_init. */
int vd_comm_available(int* version);
/* the last vd_model_allreduce_grads: floats in bucket 1 (encoder tensors, reduced under the decoder's backward) and bucket 2
 * (embedding + decoder), whether bucket 1 was issued early, calls since vd_comm_init */
int vd_comm_stats(int64_t* bucket1_floats, int64_t* bucket2_floats, int* overlapped, int64_t* calls);
/* the last vd_model_allreduce_grads: ms between "bucket 1 summed over the ranks" (communication stream) and "backward ended" (main
 * stream); positive = hidden under the decoder's backward with that much to spare, negative = exposed.  Waits for both events. */
int vd_comm_overlap_ms(float* lead_ms);
int vd_model_allreduce_grads(vd_model* m);                /* enqueue only; every rank, once per step */
int vd_model_init_params(vd_model* m, uint64_t seed);     /* library-default init */
/* Names that start with '@' are batch attachments, not parameters (no parameter's name starts with it).
 * "@dense_relevance", n = N * O floats: the dense relevance matrix (VisDial v1.0 annotations) of the batch uploaded last, row n = round
 * n.  A row is annotated (every entry finite and >= 0) or not annotated (every entry -1); a mixed row, a NaN, an infinity or another
 * negative value, a wrong n, and a call before any upload are argument errors that name the attachment.  The matrix is checked on the
 * host, staged in pinned memory and copied on the upload lane; the call waits for no step and does not empty the answer-encoding cache.
 * The next upload into the batch's slot drops it.  What it changes: vd_model_forward_backward(m, 0) of a disc model trains on it
 * (below), and vd_model_get_tensor "@ndcg" ranks with it.  Everything else ignores it.
 * "@dense_relevance_live": the same matrix through the same checks, named by their own name; an attachment replaces the one before it on
 * the same upload.  It asks in addition that the next TRAINING step run the option recurrence, its backward, the table-gradient row sum
 * and the dWh contraction over the candidate rows of the LIVE rounds only -- the rounds whose weight (below) is > 0, in ascending order,
 * one row per (live round, candidate); the encoder runs over all N rounds.  Loss and gradients are those of "@dense_relevance" up to fp32
 * summation order (a round of weight 0 adds exact zeros).  After such a step vd_model_scores holds the live rounds' scores and 0.0 in
 * every other round's row, and vd_model_option_rows reports (n_live * O, N * O).  With every round live it IS "@dense_relevance".
 * only_forward = 1, retrieval and "@ndcg" see all rounds either way.  Refused by name: a model with lstmBf16 = 1 (rules DL1-DL5 at the
 * top of csrc/loss.hip).
 * "@img_regions", n = B floats: the number of live regions of every image of the batch uploaded last, for the two encoders with the image
 * attention (mn-att-ques-im-hist, lf-att-ques-im-hist) -- detector regions, a different number per image, padded to imgSpatialSize^2 rows
 * in img_feat.  Every value is an integer in 1 .. imgSpatialSize^2; they come as floats because that is the signature.  The image
 * attention of every pass over that upload (training step, only_forward, retrieval, encode, beam search, sampling, both rollouts and the
 * round pass) then looks at the first counts[b] regions of image b and at nothing else: softmax over the live regions, probability +0.0
 * and zero gradient for the others (rules IR1-IR6 at the top of csrc/attention.hip).  The hidden rows of img_feat must be finite (write
 * zeros): the dense products still read them.  Same transport as "@dense_relevance": checked on the host, staged in pinned memory, copied
 * on the upload lane, no wait for a step, dropped by the next upload into the slot, replaced by a second attachment on the same upload.
 * With every count = imgSpatialSize^2 the outputs are the unattached pass's (bit for bit where no atomic is involved).  Argument errors
 * that name the attachment: a call before any upload, an encoder without the image attention, n != B, a value that is not an integer in
 * range.  Without the attachment every call launches what it launched before. */
int vd_model_set_tensor(vd_model* m, const char* name, const float* host, int64_t n);   /* wrapperW:copy(...) */
/* "@ndcg", which = 0, n = 2 N: runs the NDCG kernel on the scores of the last forward or retrieval of the current batch (either decoder)
 * and its "@dense_relevance"; `host` receives N DOUBLES, bit for bit, in the 2 N floats of the signature (read the buffer as double[N]).
 * k = the number of candidates with relevance > 0; candidates ranked by score as vd_model_ranks ranks them; DCG = the sum over ranks
 * r <= k of relevance / log2(1 + r); IDCG = the same with the candidates ranked by relevance (ties: the lower index first); the value is
 * DCG / IDCG, -1 for an annotated round with k = 0 (leave it out of a mean) and -2 for a round that is not annotated.  Without an
 * attachment on the current batch: a state error that names it. */
int vd_model_get_tensor(vd_model* m, const char* name, int which /*0 W, 1 dW, 2 m, 3 v*/, float* host, int64_t n);
int vd_model_set_training(vd_model* m, int on);           /* wrapper:training() / :evaluate() (model.lua:57,111) */
int vd_model_set_dropout_mask(vd_model* m, const char* site, const uint8_t* host_keep, int64_t n); /* NULL host = clear */
/* batch re-layout + upload (model.lua:255-294, dataloader.lua:410-475), asynchronous, double-buffered */
int vd_model_upload_batch(vd_model* m, const vd_batch* host_batch);
/* Model:forwardBackward on the uploaded batch (model.lua:249-342); zeroes the gradients first unless only_forward.
 * Environment VD_LABEL_SMOOTHING = eps, a real in [0, 1) (0 / unset = off; any other text is refused by name), read by vd_model_create
 * for both decoders: a TRAINING step (only_forward = 0) takes soft targets t = (1 - eps) onehot + eps / K in the place of the one-hot
 * ones -- disc: K = the O options of a round, loss_n = lse - sum_o t_o s_o, ds_o = (softmax_o - t_o) gscale; gen: K = the V vocabulary
 * words, on every row that contributes without it (non-pad input and target > 0), loss_r = lse - sum_c t_c logit_c, gradient
 * softmax - t (rules LS1-LS4 at the top of csrc/loss.hip).  vd_model_loss then reports the smoothed loss.  only_forward = 1,
 * vd_model_retrieve*, perplexity and every score or rank are what they are without the variable, and eps = 0 launches the kernels
 * of a library that does not know it, with the same arguments.
 * Dense fine-tuning (decoder disc): when the batch carries "@dense_relevance" (vd_model_set_tensor), a TRAINING step takes the target
 * t = rel / sum(rel) with weight w = 1 for an annotated round with a relevant candidate, w = 0 for an annotated round without one, and
 * t = onehot(answer_ind) with w = mu for a round that is not annotated; loss = sum_n w_n (lse_n - sum_o t_o s_o) / W with W = sum_n w_n
 * over the batch, ds = w_n (softmax - t) / W (rules DT1-DT5 at the top of csrc/loss.hip); vd_model_loss reports that weighted mean.
 * mu is the environment's VD_DENSE_MIX, a finite real in [0, 1] (0 / unset: rounds without an annotation do not train), read by
 * vd_model_create, which refuses any other text by name.  A batch with W = 0, a model created with VD_LABEL_SMOOTHING > 0 and a
 * model of decoder gen refuse the dense step by name; only_forward = 1, retrieval, scores and ranks ignore the attachment, and a batch
 * without one launches the kernels it launched before. */
int vd_model_forward_backward(vd_model* m, int only_forward);
int vd_model_loss(vd_model* m, float* loss);              /* curLoss of the last forward (waits for it): disc = mean
                                                             cross-entropy, gen = summed NLL (model.lua:309-311,330) */
/* Model:retrieveBatch up to the option scores (model.lua:344-425): disc = scores of a forward pass, gen = candidate
 * log-likelihoods (utils.computeLhood, utils.lua:86-102); read with vd_model_scores / vd_model_ranks.
 * Answer-encoding cache (decoder disc, opt-in): with the environment variable VD_OPTION_CACHE set when vd_model_create runs
 * (0 / unset = off, 1 = on with 262 144 rows, a larger value = the capacity in rows) and training off, vd_model_retrieve and
 * vd_model_forward_backward(only_forward = 1) keep the final hidden state of every distinct candidate row (key: its tokens and
 * To) in a device table and run the option recurrence (VD_FLAG_STATE_ONLY) over the rows not seen before only.  The table is
 * emptied by vd_model_set_training(on != 0), vd_model_set_tensor, vd_model_init_params, vd_model_update,
 * vd_model_forward_backward(only_forward = 0) and vd_model_flat_pointers; a host that writes the weights through the pointers of
 * the latter must call one of these afterwards.  A batch uploaded while the cache is on and training is off carries the unseen
 * rows only: it serves these two calls, not a backward pass.  vd_model_create refuses the variable for decoder gen and for
 * lstmBf16 = 1.
 * Rollout (decoder disc, opt-in): VD_RETRIEVE_ROLLOUT = 1 (0 / unset = off; read once by vd_model_create, which refuses any other
 * value by name and refuses 1 together with VD_OPTION_CACHE -- a cached batch carries only the rows the cache did not hold;
 * ignored for decoder gen, whose rollout is VD_BEAM_ROLLOUT at vd_model_beam_search).  With training off and an encoder that has
 * a history, this call then ranks round r of a dialog on a history that holds THE MODEL'S OWN answers to rounds < r instead of
 * the uploaded ones (the rule is E1-E5 at the top of csrc/beam.hip): the answer of a round is the candidate vd_model_ranks would
 * give rank 1 (the highest score, among equal scores the lowest index); history row r + 1 is the non-zero tokens of question row
 * r, then the candidate's words (entries 0, 1, ... of its options row up to the first 0) as far as they fit, right-aligned in
 * the Th columns.  The option recurrence runs ONCE (an option's encoding does not depend on the history); then R = maxQuesCount
 * passes -- encoder forward, the scoring of all N rounds, one kernel that writes history row r + 1 of every dialog -- with no host
 * synchronisation between them.  The scores, ranks and loss the call leaves are those of the last pass, which is the result for
 * every round (rows <= r of a dialog do not change after pass r and every encoder is causal over the rounds); vd_model_scores /
 * vd_model_ranks / vd_model_loss read them as ever.  The uploaded contents of history rows >= 1 are ignored and overwritten:
 * after the call the batch's device history holds the generated rows.  vd_model_upload_batch lays the history rows >= 1 of such
 * a model out at full width and refuses, by name, Th < Tq; pass the history at its untrimmed width, a picked answer may be longer
 * than the ground truth's.  With training on the call returns a state error that names the variable.  An encoder without a
 * history ranks as before; vd_model_forward_backward is the plain step in both modes; with the variable 0 or unset nothing
 * changes.  The host loop it equals: split_eval.py retrieve_rollout_batch.
 * For decoder gen the same measurement composes existing calls on ONE slot: vd_model_upload_batch (with option_in / option_out),
 * vd_model_encode, vd_model_beam_search on a model created with VD_BEAM_ROLLOUT = 1 (it leaves the generated history in the
 * slot), then vd_model_retrieve or vd_model_retrieve_lhood. */
int vd_model_retrieve(vd_model* m);
/* the same contract for the generative decoder through the live-row head (vd_lhood_* above): scores within the fp32 rounding of
 * vd_model_retrieve's, no logits buffer, one host synchronisation per chunk of options (the live-row count).  An argument error
 * that names the decoder for `disc`.
 * Prefix tree (opt-in): with the environment variable VD_LHOOD_TREE set to 1 when vd_model_create runs (0 / unset = off), this call
 * scores the candidates over a prefix tree of their tokens: the decoder state after a candidate's first t tokens depends on the
 * round's encoder state and on those tokens only, so every distinct (round, token prefix) is ONE node -- computed once by the
 * level-by-level recurrence (VD_FLAG_TREE; <START>, shared by the 100 candidates of a round, is one row per round) and projected on
 * the vocabulary once (its log-sum-exp); a candidate's score is the sum over its steps of target logit - log-sum-exp of the node,
 * in step order, so two identical candidates tie exactly and an empty one scores 0.0.  vd_model_upload_batch builds the tree on the
 * host from option_in / option_out, one per chunk of options sized by the nodes it holds; the call adds no host synchronisation.
 * A batch with a token behind a pad in any candidate takes the path without the variable, unchanged.  vd_model_option_rows then
 * reports executed = sum over the levels of min(N, ceil(n_t / G) * G) (n_t = nodes of level t, N = the widest level, G = the step
 * kernel's row tile for N), total = To * rounds * options.  vd_model_retrieve is unaffected.  vd_model_create refuses the variable
 * for decoder disc and for lstmBf16 = 1. */
int vd_model_retrieve_lhood(vd_model* m);
/* wrapperdW*gscale -> clamp(-5,5) -> adam -> lr decay (model.lua:96-105; optim_updates.lua:62-91).
 * Environment VD_GRAD_CLIP_NORM = c and VD_WEIGHT_DECAY = lambda, finite reals >= 0 (0 / unset = off; any other text is refused by
 * name), read by vd_model_create for both decoders (rules GC1-GC3 and WD1 in csrc/elementwise.hip).  c > 0: the norm
 * || gscale wrapperdW ||_2 of the whole flat gradient -- after the caller's all-reduce -- is computed on the main stream by a
 * partial-sum kernel and a one-workgroup kernel (no atomic, no host read, no synchronisation; a fixed order, so two runs give the same
 * bits); where it is finite and > c every element is scaled by c / norm in front of the clamp, otherwise by 1, so a non-finite norm
 * never turns finite gradients into NaN.  wrapperdW keeps the clamped value, as without the variable.  lambda > 0: decoupled decay,
 * w <- w - step m / (sqrt(v) + eps) - lr lambda w_old on every element, lr the learning rate before this call's decay.  With both off
 * the call launches vd_clamp_adam as a library that does not know the variables does. */
int vd_model_update(vd_model* m, float gscale);
int vd_model_learning_rate(vd_model* m, double* lr, int set);
/* Model:generateAnswers, device side (model.lua:432-613; generative decoder).  The host keeps the candidate
 * bookkeeping exactly as the reference's Lua does; each call advances all live hypotheses together.
 *   encode        encoder forward of the uploaded batch = forwardBackward(batch, true, true) (model.lua:464)
 *   decode_begin  hiddenBeams (model.lua:478-503): hypothesis i starts from the encoder state of QA round rounds[i] (0-based)
 *   decode_step   one decoder step (model.lua:518-522, 590-596): tokens[n] in, log-probabilities [n x vocabSize] out (host)
 *   decode_select hypothesis i continues from the stepped state of hypothesis src[i] (model.lua:560-575); slots >= n_keep
 *                 keep their previous state; sampling passes the identity */
int vd_model_encode(vd_model* m);
int vd_model_decode_begin(vd_model* m, const int32_t* rounds, int n);
int vd_model_decode_step(vd_model* m, const int32_t* tokens, float* host_logprobs);
int vd_model_decode_select(vd_model* m, const int32_t* src, int n_keep);
/* the whole beam search of Model:generateAnswers (model.lua:466-573) for EVERY round of the last vd_model_encode batch at once,
 * on the device (the vd_beam_* kernels above): N = B*R groups of beam_size hypotheses, beam_len-1 steps enqueued without a host
 * synchronisation, then one copy back.  host_tokens [N x beam_len] = each round's answer (best finished column, else column 0;
 * zero-padded), host_scores [N] its fp64 score.  Same answers as the host loop over decode_begin / step / select.
 *
 * !! LAYOUT CHANGE UNDER VD_BEAM_GROUPS !!  A model created with the environment variable VD_BEAM_GROUPS = G > 1 (decoder gen; an
 * integer >= 1, 1 / unset = off) runs DIVERSE beam search (Vijayakumar et al. 2016, Hamming diversity; the rule is D1-D7 at the top of
 * csrc/beam.hip): the beam_size slots of a round are G groups of beam_size / G, searched one after another within a step, a group's
 * log-probabilities lowered by VD_BEAM_DIVERSITY (a finite real >= 0, unset = 0.5) for every slot of an earlier group that took the
 * same word at that step.  Such a model REFUSES a beam_size that G does not divide and writes EVERY group's answer:
 *   host_tokens [N x G x beam_len], host_scores [N x G]   (round-major, then group) -- G times the buffers of a plain model.
 * A score is the answer's true (unpenalised) log-likelihood.  The caller picks the round's answer: the highest score among the
 * groups whose answer holds end_token, ties to the lower group; group 0's if none does.  vd_model_create reads both variables once
 * and refuses any other value by name; both are ignored for decoder disc.  decode_begin / step / select need nothing new.
 *
 * Constraints (decoder gen; the rule is C1-C6 at the top of csrc/beam.hip; each 0 / unset = off, and with all three off the call
 * launches the kernels with the arguments it always did; they combine freely with VD_BEAM_GROUPS).  vd_model_create reads them once,
 * refuses any other value with an argument error that names the variable, and ignores all three for decoder disc:
 *   VD_BEAM_MIN_LEN = m         an integer >= 0: no answer of fewer than m words -- end_token is banned at every step <= m
 *   VD_BEAM_NO_REPEAT = n       an integer >= 0: no n-gram of words occurs twice in a hypothesis (start_token is not a word)
 *   VD_BEAM_LENGTH_PENALTY = a  a finite real >= 0: finished hypotheses compete on score / length^a, length = words + end_token;
 *                               decided without a division on a table length^a computed on the host in fp64
 * A banned word counts as -inf in its row; nothing is renormalised, so every other value and every returned score (the true
 * log-likelihood) is what it was.  With m or n on, vd_model_beam_search REFUSES, naming the variable,
 *   vocabSize < beam_size + beam_len - 1   (a row must keep beam_size unbanned words),
 *   m > beam_len - 2                       (end_token must be allowed at the last step),
 *   beam_len > VD_BEAM_LMAX = 64 with n on (the column and its ban list sit in LDS).
 * A host that keeps the bookkeeping itself over decode_begin / step / select follows split_eval.beam_search_round.
 *
 * Rollout: VD_BEAM_ROLLOUT = 1 (decoder gen; 0 / unset = off; read once by vd_model_create, which refuses any other value by name and
 * refuses 1 together with VD_BEAM_GROUPS > 1; ignored for decoder disc).  Such a model answers round r of a dialog on a history that
 * holds ITS OWN answers to rounds < r instead of the uploaded ones (the rule is R1-R6 at the top of csrc/beam.hip): history row 0 is
 * the uploaded caption row; row r >= 1 is the non-zero tokens of question row r - 1, then the words of the answer returned for round
 * r - 1 (entries 1, 2, ... of its token row up to the first end_token or 0) as far as they fit, right-aligned in the Th columns.  The
 * call runs R = maxQuesCount passes over the batch's dialogs -- encoder forward, the search of round r of every dialog, one kernel that
 * writes history row r + 1 -- with no host synchronisation between passes and one copy back in the layout above: host_tokens
 * [N x beam_len], host_scores [N], row = dialog * R + round, every score the true log-likelihood under the constraints in force.  The
 * uploaded contents of history rows >= 1 are ignored and overwritten: after the call the batch's device history holds the generated
 * rows.  vd_model_upload_batch lays the history rows >= 1 of such a model out at full width and refuses, by name, Th < Tq (a history
 * row has to hold a whole question); vd_model_sample on such a model is refused by name.  An encoder without a history (lf-ques,
 * lf-ques-im) accepts the variable and runs the plain single-pass search with the launches it always made.  With the variable 0 or
 * unset nothing changes.  The host loop it equals: split_eval.py rollout_dialog. */
int vd_model_beam_search(vd_model* m, int beam_size, int beam_len, int start_token, int end_token, int32_t* host_tokens,
                         double* host_scores);
/* temperature sampling of Model:generateAnswers (sampleWords = 1, model.lua:576-613) for EVERY round of the last vd_model_encode
 * batch at once, on the device (the vd_sample_* kernels above): N = B*R rows, all beam_len steps (the reference samples through
 * <END>) enqueued without a host synchronisation after one upload of the host's uniforms [beam_len x N] (step-major, row =
 * dialog * R + round, each in [0, 1)), then one copy back.  host_tokens [N x (beam_len + 1)] = <START> and the sampled ids,
 * host_loglik [N] the fp64 log-likelihood through the first <END>.  The tokens of the host loop over decode_step drawing with
 * RandomState.choice from the same uniforms, up to draws within rounding of a CDF boundary.  Argument errors: no
 * vd_model_encode first, beam_len < 1, a temperature that is not finite and > 0, a uniform outside [0, 1), and a row whose
 * weights exp(logp / temperature) all underflow (nothing to draw from; the host path fails there too).
 * Top-k / nucleus truncation: VD_SAMPLE_TOPK (an integer >= 0; 0 / unset = off) and VD_SAMPLE_TOPP (a real in (0, 1]; 1 / unset = off)
 * are read once by vd_model_create, which refuses any other value by name (both are ignored for decoder disc).  A model created with
 * one of them draws each token from the kept set only: candidates by descending fp32 log-probability, equal values by ascending id, the
 * first k of them, then the shortest prefix of those whose weights reach the share p of their sum.  host_loglik still adds the
 * UNtruncated log-probability of every drawn token, so truncated, untruncated and per-dialog runs report comparable numbers.  Two calls
 * on the same inputs return the same arrays.  The rule: csrc/sample.hip, visdial_amd/split_eval.py truncated_weights. */
int vd_model_sample(vd_model* m, int beam_len, int start_token, int end_token, double temperature, const double* host_uniforms,
                    int32_t* host_tokens, double* host_loglik);
int vd_model_scores(vd_model* m, float* host_scores, int64_t n);        /* [N x O] of the last forward / retrieve */
int vd_model_ranks(vd_model* m, int use_gt, int32_t* host_ranks);       /* utils.computeRanks (utils.lua:106-128) */
/* decoder disc: rows the option LSTM executed for the batch of the LAST STEP (before any step: of the uploaded batch) vs the N * O
 * candidates they stand for -- the upload encodes every DISTINCT candidate row once (decoders/disc.lua:4-15: the encoding depends on
 * the tokens only).  In a pipelined loop this is the batch that was stepped, not the one prefetched behind it.  With the
 * answer-encoding cache (vd_model_retrieve) `executed` counts the rows the recurrence ran in that step -- the rows the cache did
 * not hold, possibly 0. */
int vd_model_option_rows(vd_model* m, int64_t* executed, int64_t* total);
int vd_model_family_ms(vd_model* m, float* ms3);          /* device ms of option-LSTM fwd, bwd, dWh in the last step */
int vd_model_synchronize(vd_model* m);

#ifdef __cplusplus
}
#endif
#endif /* VISDIAL_HIP_H */
