// Shared helpers for the visdial HIP library (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#define VD_OK 0
#define VD_ERR_ARG -1
#define VD_ERR_HIP -2
#define VD_ERR_STATE -3
#define VD_FLAG_BF16 1  // see include/visdial_hip.h
#define VD_FLAG_SPLIT9 2
#define VD_FLAG_SPLIT6 4
#define VD_FLAG_SPLIT3 8
#define VD_FLAG_SPLIT (VD_FLAG_SPLIT9 | VD_FLAG_SPLIT6 | VD_FLAG_SPLIT3)
#define VD_FLAG_LIVE_PREFIX 16
#define VD_FLAG_STATE_ONLY 32
#define VD_FLAG_TREE 64
#define VD_FLAG_HOLD 128
#define VD_LIVE_PREFIX_ROWS 128
#define VD_BEAM_LMAX 64  // beam.hip: the longest beamLen while n-gram blocking is on (a column and its ban list sit in LDS)

// thread-local message returned by vd_last_error()
void vd_set_error(const char* fmt, ...);

#define VD_CHECK_ARG(cond, ...)                                   \
  do {                                                            \
    if (!(cond)) {                                                \
      vd_set_error(__VA_ARGS__);                                  \
      return VD_ERR_ARG;                                          \
    }                                                             \
  } while (0)

#define VD_HIP(expr)                                                          \
  do {                                                                        \
    hipError_t e__ = (expr);                                                  \
    if (e__ != hipSuccess) {                                                  \
      vd_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr,              \
                   hipGetErrorString(e__));                                   \
      return VD_ERR_HIP;                                                      \
    }                                                                         \
  } while (0)

#define VD_LAUNCH_CHECK() VD_HIP(hipGetLastError())

static inline int vd_cdiv(long a, long b) { return (int)((a + b - 1) / b); }
// blocks of 256 threads for a grid-stride loop over n elements: one per 256, at least 1, at most 4096
static inline unsigned grid_for(long n) { return (unsigned)std::max<long>(1, std::min<long>((n + 255) / 256, 4096)); }

// ROCTx ranges around the phases of a step (SURVEY.md section 5 "tracing"): host-side ranges on the enqueuing thread, visible in
// `rocprofv3 --marker-trace --kernel-trace` next to the kernels dispatched inside them.  librocprofiler-sdk-roctx.so / libroctx64.so is
// dlopen'ed on first use and ONLY when the environment says VD_ROCTX=1 (scripts/measure_round.sh sets it for the trace pass); otherwise,
// or when neither library loads, the calls are no-ops.  (api.hip)
void vd_range_push(const char* name);
void vd_range_pop();
struct VdRange {
  explicit VdRange(const char* name) { vd_range_push(name); }
  ~VdRange() { vd_range_pop(); }
  VdRange(const VdRange&) = delete;
  VdRange& operator=(const VdRange&) = delete;
};

// Library-owned per-(device, stream) scratch (api.hip): work buffers whose lifetime is one stream-ordered call
// (the gate-interleaved Wh^T copy and the tile queues / arrival counters of the persistent recurrence kernels).
// Calls on different streams get different buffers, so they may overlap freely.
struct VdStreamScratch {
  float* wht = nullptr;      // [4H x H]
  size_t wht_bytes = 0;
  unsigned* sync = nullptr;  // persistent-kernel queue heads + arrival counters
  size_t sync_bytes = 0;
};
int vd_stream_scratch(hipStream_t stream, size_t wht_bytes, size_t sync_bytes, VdStreamScratch* out);
int vd_num_cus();  // compute units of the current device (cached)

// zero rows [nact[t], N) of every time slice of up to 6 dense [T x N x ncols[i]] buffers in one launch (elementwise.hip)
struct VdZeroSet {
  float* buf[6];
  int ncols[6];
  int n;
  long quads_per_row;   // filled in by the launcher
};
int vd_zero_inactive_multi(const VdZeroSet& z, const int32_t* nact_dev, int T, int N, hipStream_t stream);

// C_p [M x N] += A_p^T * B_p over the live rows of length-sorted steps, up to VD_LIVE_MAXP products in ONE launch (gemm_ops.hip;
// wgrad_plan.h has the segment tables and the work list, all device arrays here; M, N multiples of 128, 16-byte rows)
constexpr int VD_LIVE_MAXP = 8;   // (two stacks of two layers: 2 x (two dWh + the layer-2 dWx) = 6)
struct VdLiveProduct {
  const float *A, *B;      // B from the row that pairs with row 0 of A
  float* C;
  const int32_t* segs;     // [segments + sentinel][4]
  long lda, ldb, ldc;
  int M, N;
};
int vd_gemm_tn_live_grouped(const VdLiveProduct* prod, int nprod, const int32_t* items, const int32_t* chunk_start, int chunks,
                            hipStream_t stream);

typedef unsigned short vd_bf16_bits;
// ---- compact bf16 state of the option recurrence (model-level runtime, lstmBf16 = 1: BASELINE configs[4]) --------------------
// The saved gates / da live ONLY as bf16 [T x N x 4H], the projection table as bf16 rows, h as bf16 (+ the last step's fp32 h):
// 291 / 414 instead of 496 / 660 MB of epilogue traffic per forward / backward launch at the headline shape (lstm.hip).
int vd_lstm_forward_c16(const vd_bf16_bits* table16, int64_t tab_ld, const int32_t* tok_gather, const float* Wh, vd_bf16_bits* gates16,
                        vd_bf16_bits* h16, float* h_last, float* c, int T, int N, int H, hipStream_t stream);
int vd_lstm_backward_c16(const float* Wh, vd_bf16_bits* gates16, const float* c, const float* dh_last, float* dc_work, int T, int N, int H,
                         hipStream_t stream);
int vd_f32_to_bf16(const float* src, vd_bf16_bits* dst, int64_t n, hipStream_t stream);
int vd_gemm_tn_acc_bf16(const vd_bf16_bits* A16, const vd_bf16_bits* B16, float* C, int64_t ldc, int M, int N, int K, hipStream_t stream);
int vd_segment_rowsum_acc_bf16(const vd_bf16_bits* X16, int64_t ldx, const int32_t* tok, const int32_t* perm, int64_t n, int ncol,
                               float* out, int64_t ldo, hipStream_t stream);

// bf16 shadows of fp32 activations (opt-in bf16 option recurrence, VD_FLAG_BF16; api.hip).  The producing kernels of a
// bf16 pass (LSTM forward: h; LSTM backward: da) also write a bf16 copy of what they store, into a library-owned buffer
// registered against the fp32 tensor's address range; the weight-gradient contraction of the same pass finds the two
// shadows by address and multiplies them directly (LDS-DMA + transpose reads, no fp32 -> bf16 conversion while staging).
// One shadow per registered tensor (keyed by device + base address: two models in a process never share one; the `slot` argument of the
// older two-slot registry is ignored).  A shadow is valid until the next producer call on the same tensor, or
// until an fp32 producer overwrites its range (vd_bf16_shadow_invalidate: the fp32 recurrences, a forward pass over the gates buffer,
// vd_memset).  The registry is process-global and keyed by address only: VD_FLAG_BF16 on vd_gemm_tn_acc is meant for the contraction that
// directly follows the bf16 recurrences of the same pass -- a host that writes those ranges by other means (its own kernels, a tensor
// library) must not pass the flag afterwards.  What the registry can do against an entry that outlived its tensor (a host that freed h / gates
// to an allocator which hands the addresses out again) it does: vd_gemm_tn_acc takes the shadows only for the contraction the producers
// leave behind -- A = h from its registered base, B = da from step 1 up to its registered end (`anchor` of vd_bf16_shadow_find) -- so an
// unrelated pair of operands that merely lies inside two stale ranges is contracted from its fp32 rows.
#define VD_SHADOW_ANYWHERE 0
#define VD_SHADOW_AT_BASE 1
#define VD_SHADOW_AT_END 2
int vd_bf16_shadow_get(int slot, const float* base, size_t floats, vd_bf16_bits** out);
const vd_bf16_bits* vd_bf16_shadow_find(const float* p, size_t floats, int anchor = VD_SHADOW_ANYWHERE);
void vd_bf16_shadow_invalidate(const float* p, size_t floats);

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Gate nonlinearities on the hardware exp and reciprocal (v_exp_f32, v_rcp_f32: ~1 ulp each): absolute error ~1e-7,
// two orders below the 1e-5 per-op / 1e-4 end-to-end parity budget.  The reciprocal is the bare instruction on
// purpose: `__fdividef` / `1.0f / x` expand to the IEEE division sequence (2 v_div_scale, v_rcp, 4 v_fma, v_div_fmas,
// v_div_fixup = ~10 VALU instructions), which was HALF of the LSTM step epilogue's 1 550 VALU instructions -- and VALU
// issue in the epilogue comes straight out of the co-resident waves' matrix-pipe time.
__device__ __forceinline__ float vd_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float vd_sigmoid(float x) { return vd_rcp(1.0f + __expf(-x)); }
__device__ __forceinline__ float vd_tanh(float x) {
  const float e = __expf(-2.0f * fabsf(x));          // in (0, 1]: no overflow
  const float t = (1.0f - e) * vd_rcp(1.0f + e);
  return copysignf(t, x);
}

// Buffer addressing for the step kernels' epilogues: an SGPR descriptor per tensor + a 32-bit VGPR byte offset + an
// SGPR byte offset for the uniform part (gate / row-group strides).  buffer_load / buffer_store compute the address in the
// memory pipeline, so the ~130 64-bit VALU address instructions a tile's epilogue spent on `ptr + (long)row * ld + j` go away --
// and VALU issue is what the epilogue costs (profiles/r03_experiments.txt section 13c).  The compiler tracks vmcnt for these
// builtins (unlike inline asm).  No reliance on the hardware range check: the SGPR offset is not part of it on gfx9.
typedef unsigned vd_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned vd_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t vd_rsrc(const void* p) {
  // num_records = 2^32 - 1: byte offsets are 32-bit, every tensor addressed this way is < 4 GB per launch (checked by the callers)
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, -1, 0x00020000);
}
__device__ __forceinline__ float4 vd_buf_ld4(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  const vd_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
__device__ __forceinline__ void vd_buf_st4(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, const float4& v) {
  const vd_u32x4 t = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
  __builtin_amdgcn_raw_buffer_store_b128(t, r, voff, soff, 0);
}
__device__ __forceinline__ void vd_buf_st4_bf16(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, const float4& v) {
  typedef __bf16 bf4 __attribute__((ext_vector_type(4)));
  const bf4 t = {(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(vd_u32x2, t), r, voff, soff, 0);
}

// 4 packed bf16 -> float4
__device__ __forceinline__ float4 vd_bf16x4_unpack(const vd_u32x2 v) {
  return make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16),
                     __uint_as_float(v.y & 0xffff0000u));
}
// 4 consecutive bf16 (one 8-byte buffer load) -> float4
__device__ __forceinline__ float4 vd_buf_ld4_bf16(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  return vd_bf16x4_unpack(__builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
}

// 4 consecutive fp32 -> 4 bf16 (RNE, v_cvt_pk_bf16_f32), one 8-byte store
__device__ __forceinline__ void vd_st4_bf16(vd_bf16_bits* p, const float4& v) {
  typedef __bf16 bf4 __attribute__((ext_vector_type(4)));
  bf4 t = {(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
  *reinterpret_cast<bf4*>(p) = t;
}

// wave64 all-reduce helpers
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Dropout on four consecutive elements: m holds their four mask bytes (byte 0 = v.x), a non-zero byte keeps the element times scale, a zero
// byte gives +0 whatever the element holds (a select, not a product: NaN or Inf in a dropped element does not come through).
__device__ __forceinline__ float4 vd_mask4(float4 v, uint32_t m, float scale) {
  v.x = (m & 0xffu) ? v.x * scale : 0.f;
  v.y = (m & 0xff00u) ? v.y * scale : 0.f;
  v.z = (m & 0xff0000u) ? v.z * scale : 0.f;
  v.w = (m & 0xff000000u) ? v.w * scale : 0.f;
  return v;
}

// Log-sum-exp of one row of V logits for a 256-thread block: 256 strided threads take the max, then the sum of exp(x - max),
// each reduced by wave_max / wave_sum with the four wave partials combined in a fixed order; `red` is the block's 8-float
// shared buffer.  The one row arithmetic of vd_logsoftmax_nll, vd_log_softmax_rows, vd_beam_topk and vd_sample_draw: the
// generation kernels' log-probabilities are bit-identical to vd_log_softmax_rows because all of them call this.
__device__ __forceinline__ float block_row_lse(const float* row, int V, float* red) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float mx = -INFINITY;
  for (int c = tid; c < V; c += 256) mx = fmaxf(mx, row[c]);
  mx = wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float sum = 0.f;
  for (int c = tid; c < V; c += 256) sum += expf(row[c] - mx);
  sum = wave_sum(sum);
  if (lane == 0) red[4 + wave] = sum;
  __syncthreads();
  return mx + logf(red[4] + red[5] + red[6] + red[7]);
}
