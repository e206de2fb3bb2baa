// Kernel-path policy: the precision and shape tests that more than one module, or more than one entry point, applies before it
// launches.  Host code only, and no kernel header: runtime.hip and comm.hip include it and instantiate no GEMM kernels.  A test that
// only one entry point reads stays next to it (the LDS-DMA condition of vd_gemm_nt, the H % 64 of the bf16 ticks).
#pragma once
#include "common.h"

// ---- precision of a model-level pass -------------------------------------------------------------------------------------------
// vd_model_params.lstmBf16 -> VD_FLAG_*, or -1 for a value that names no precision.  vd_model_create converts it once (vd_model::flags)
static inline int vd_precision_flags(int lstmBf16) {
  switch (lstmBf16) {
    case 0: return 0;
    case 1: return VD_FLAG_BF16;
    case 3: return VD_FLAG_SPLIT3;
    case 6: return VD_FLAG_SPLIT6;
    case 9: return VD_FLAG_SPLIT9;
    default: return -1;
  }
}
// products per step of the exact split a flag word asks for (split_core.h): 9 / 6 / 3, 0 = none
static inline int vd_split_nprod(int flags) {
  return (flags & VD_FLAG_SPLIT9) ? 9 : (flags & VD_FLAG_SPLIT6) ? 6 : (flags & VD_FLAG_SPLIT3) ? 3 : 0;
}

// ---- option recurrence (lstm.hip: vd_lstm_forward / vd_lstm_backward / the _c16 pair; rt_decoders.h) ---------------------------
// rows from which a recurrence step takes the throughput kernels (LDS-DMA pipeline, bf16 operands, exact split) instead of the
// latency-shape ones
constexpr long VD_THROUGHPUT_ROWS = 2048;
// row tile of the fp32 forward step kernel a recurrence over N rows runs (lstm.hip asserts that its tile configurations agree): the
// height of the row groups VD_FLAG_LIVE_PREFIX skips
constexpr int VD_LSTM_FWD_TILE_BIG = 128, VD_LSTM_FWD_TILE_SMALL = 32;
static inline int vd_lstm_fwd_row_tile(long N) { return N >= VD_THROUGHPUT_ROWS ? VD_LSTM_FWD_TILE_BIG : VD_LSTM_FWD_TILE_SMALL; }
// LDS-DMA step pipeline of the fp32 operands (and of the exact split): K % 16 == 0 and 32-bit row byte offsets of the streamed operand
// (h [N x H] forward, da [N x 4H] backward)
static inline bool vd_lstm_glds_fwd_fits(long N, int H) { return N >= VD_THROUGHPUT_ROWS && H % 32 == 0 && N * H * 4 < (1L << 32); }
static inline bool vd_lstm_glds_bwd_fits(long N, int H) { return N >= VD_THROUGHPUT_ROWS && H % 32 == 0 && N * 4 * H * 4 < (1L << 32); }
// bf16 operands in the step kernels, which also write the bf16 shadows of h / da (common.h)
static inline bool vd_lstm_bf16_fits(long N, int H) { return N >= VD_THROUGHPUT_ROWS && H % 32 == 0; }
// compact bf16 state (common.h): the recurrence of a bf16 pass of the model-level runtime, vd_lstm_forward_c16 / vd_lstm_backward_c16
static inline bool vd_lstm_c16_fits(long N, int H) { return N >= VD_THROUGHPUT_ROWS && H % 128 == 0; }

// ---- weight-gradient contraction vd_gemm_tn_acc (gemm_ops.hip), as the runtime plans around it (rt_core.h) ----------------------
// k-major LDS-DMA pipeline of the fp32 operands: C [M x N] += A[K x M]^T * B[K x N]
static inline bool vd_tn_kmajor_fits(long M, long N, long K) { return M % 128 == 0 && N % 128 == 0 && K >= 1024; }
// tile of the contraction that splits (or rounds to bf16) both fp32 operands in registers: split_core.h SplitTnCfg asserts the same
constexpr int VD_SPLIT_TN_BM = 256, VD_SPLIT_TN_BN = 128;
static inline bool vd_tn_split_tiles(long M, long N) { return M % VD_SPLIT_TN_BM == 0 && N % VD_SPLIT_TN_BN == 0; }

// live-row group of an encoder backward (vd_gemm_tn_live_grouped, gemm_ops.hip; rt_core.h wgrad_flush): a product C [M x N] += A^T * B of an
// encoder LSTM waits for the backward's one grouped launch when its rows are a length-sorted sequence set (the live rows of a step are a
// prefix of it), M and N are multiples of the 128 x 128 tile and the pass is not bf16.  Everything else keeps vd_gemm_tn_acc /
// vd_gemm_tn_rows_acc: layer-1 input weights at E = 300, the bf16 pass, the unsorted stacks
static inline bool vd_wgrad_group_fits(bool sorted_rows, long M, long N, int flags) {
  return sorted_rows && M % 128 == 0 && N % 128 == 0 && !(flags & VD_FLAG_BF16);
}

// ---- image attention (attention.hip vd_img_*_p; rt_encoders.h) -----------------------------------------------------------------
// the dense products of a split9 pass on the exact split, from the materialised dropped image tensor xdrop [rows x H] (rows = N * S2);
// the runtime materialises xdrop exactly when this holds
static inline bool vd_img_split_ok(long rows, int H, int Kc) {
  return rows >= 128 && H % 16 == 0 && Kc % 16 == 0 && rows * (H > Kc ? H : Kc) * 4 < (1L << 32);
}

// ---- live-row log-likelihood head of generative retrieval (lhood.hip vd_lhood_nll; rt_decoders.h Gen::retrieve_lhood) -------------
// fused MFMA kernel (vocabulary tiles through the LDS-DMA pipeline, online log-sum-exp): K % 16 == 0, 16-byte rows and 32-bit row byte
// offsets of both operands (h [rows x ldh] gathered by row index, W [V x ldw]), and at least one full 128-wide vocabulary tile.  Every
// other shape (the small H and V of the test models) takes the one-workgroup-per-row kernel of the same entry point.
static inline bool vd_lhood_fused_fits(long rows, long ldh, long V, long ldw, int H) {
  return H >= 64 && H % 16 == 0 && V >= 128 && ldh % 4 == 0 && ldw % 4 == 0 && rows * ldh * 4 < (1L << 32) && V * ldw * 4 < (1L << 32);
}
// length-ordered candidate recurrence of the same retrieval (lhood.hip lhood_order_p; rt_decoders.h): the chunk's candidates go through
// the decoder in order of descending length and the recurrence takes VD_FLAG_LIVE_PREFIX.  The counting sort holds one key per
// possible length (0 .. T) in a 256-thread block; the recurrence of retrieval is exact fp32 (flags 0), which is what the flag is
// implemented for.  Otherwise the chunk runs in candidate order, all rows.
static inline bool vd_lhood_prefix_fits(int T, long rows) { return T >= 1 && T < 256 && rows >= 1; }
