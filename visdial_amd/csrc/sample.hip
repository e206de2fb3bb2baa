// Batched temperature sampling of Model:generateAnswers (reference model.lua:576-613, generate.lua -sampleWords / -temperature)
// on the device: one hypothesis row per QA round, every round of a batch at once.  The randomness stays on the host: each draw
// takes one fp64 uniform u in [0, 1) from the host's generator (numpy RandomState.random_sample / the torch generator of the
// Lua host) and makes the inverse-CDF draw that RandomState.choice(V, p=pr) / torch.multinomial make from it, so the batched
// path samples what the per-dialog host loops (split_eval.py, lua/model.lua) sample.
//
// The per-row rule, for a row whose input token is t and whose raw logits are x[0..V), at step s with uniform u:
//  1. logp[c] = x[c] - lse in fp32 with lse = block_row_lse (common.h), bit-identical to log_softmax_rows_kernel (loss.hip),
//     which calls the same.  If t == 0 the row is all zeros (MaskZero(LogSoftMax), decoders/gen.lua:24); sampling never feeds a
//     0, but the rule is defined.
//  2. w[c] = exp((double)logp[c] / temperature) in fp64 (a division, as the hosts divide).
//  3. S = the fp64 sum of w.  The token is the first c with w[c] > 0 whose inclusive prefix sum exceeds u * S; if rounding
//     leaves no such c (u within rounding of 1), the last c with w[c] > 0.  The vocabulary id is c + 1.  Prefix sums: thread t
//     owns the contiguous chunk [t * ceil(V / 256), ...), P(c) = excl[t] + (w[c0] + ... + w[c]) summed left to right, excl =
//     the block's exclusive scan of the chunk sums.  P is non-decreasing within a chunk and P(chunk end) = excl[t] + sum[t],
//     so the first chunk with sum[t] > 0 whose end exceeds u * S holds the token and only its thread walks its chunk again.
//     (Across chunks the scan's rounding need not keep P monotone, hence the w > 0 conditions: a chunk or a column without
//     weight never takes the draw, as it never does on the host.)
//  4. S == 0 (every weight underflowed at a tiny temperature; the host path raises there) or no usable weight (NaN logits):
//     the status word is set, the token is 0 and the log-likelihood is left alone.  No token is guessed.
//  5. history column s (column 0 is <START>) and the next input token get the id; the row's fp64 log-likelihood adds
//     (double)logp[c] unless an earlier column 1..s-1 holds <END> (the <END> itself counts).
// The stepped LSTM state becoming the current one (decoderConnect, gen.lua:63-68) is the caller's copy.
#include <cmath>

#include "common.h"

namespace {

// history [rows x cols]: <START>, 0, ...; next token <START>; log-likelihood 0; status clear
__global__ void sample_init_kernel(long rows, int cols, int start, int32_t* __restrict__ hist, int32_t* __restrict__ tok,
                                   double* __restrict__ loglik, int32_t* __restrict__ status) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *status = 0;
  const long n = rows * cols;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    hist[e] = e % cols == 0 ? start : 0;
    if (e < rows) { tok[e] = start; loglik[e] = 0.0; }
  }
}

// rule 2 for one column; the same expression wherever a weight is needed, so a chunk's walk repeats its sum exactly
__device__ __forceinline__ double sample_weight(const float* row, int c, float lse, bool zero_row, double temperature) {
  const float lp = zero_row ? 0.f : row[c] - lse;
  return exp((double)lp / temperature);
}

// rules 1-5 for one row per workgroup
__global__ void __launch_bounds__(256)
sample_draw_kernel(const float* __restrict__ x, long ld, int V, int32_t* __restrict__ tok, const double* __restrict__ u,
                   double temperature, int step, int cols, int end_tok, int32_t* __restrict__ hist, double* __restrict__ loglik,
                   int32_t* __restrict__ status) {
  __shared__ float red[8];
  __shared__ double wtot[4];
  __shared__ int owner, last_pos, pick;
  const long r = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* row = x + r * ld;
  const bool zero_row = tok[r] == 0;
  float lse = 0.f;
  if (!zero_row) lse = block_row_lse(row, V, red);   // rule 1

  // rules 2-3: chunk sums, then the block's exclusive scan of them
  const int chunk = (V + 255) / 256;
  const int c0 = min(V, tid * chunk), c1 = min(V, c0 + chunk);
  double part = 0.0;
  for (int c = c0; c < c1; ++c) part += sample_weight(row, c, lse, zero_row, temperature);
  double incl = part;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
  double excl = __shfl_up(incl, 1, 64);
  if (lane == 0) excl = 0.0;
  if (lane == 63) wtot[wave] = incl;
  if (tid == 0) { owner = 256; last_pos = -1; pick = -1; }
  __syncthreads();
  double off = 0.0;
  for (int w = 0; w < wave; ++w) off += wtot[w];
  excl = off + excl;
  const double S = (wtot[0] + wtot[1]) + (wtot[2] + wtot[3]);
  if (S == 0.0) {                        // rule 4 (block-uniform)
    if (tid == 0) { *status = 1; hist[r * cols + step] = 0; tok[r] = 0; }
    return;
  }
  const double target = u[r] * S;
  if (part > 0.0 && excl + part > target) atomicMin(&owner, tid);
  if (part > 0.0) atomicMax(&last_pos, tid);
  __syncthreads();
  if (owner < 256) {
    if (tid == owner) {
      double run = 0.0;
      for (int c = c0; c < c1; ++c) {
        const double w = sample_weight(row, c, lse, zero_row, temperature);
        run += w;
        if (w > 0.0 && excl + run > target) { pick = c; break; }
      }
    }
  } else if (tid == last_pos) {          // u within rounding of 1
    for (int c = c1 - 1; c >= c0; --c)
      if (sample_weight(row, c, lse, zero_row, temperature) > 0.0) { pick = c; break; }
  }
  __syncthreads();
  if (tid != 0) return;
  const int c = pick;
  if (c < 0) {                           // rule 4: NaN weights leave nothing to draw from
    *status = 1; hist[r * cols + step] = 0; tok[r] = 0;
    return;
  }
  const float lp = zero_row ? 0.f : row[c] - lse;
  const int32_t* h = hist + r * cols;
  bool ended = false;
  for (int p = 1; p < step; ++p) ended = ended || h[p] == end_tok;
  if (!ended) loglik[r] += (double)lp;
  hist[r * cols + step] = c + 1;
  tok[r] = c + 1;
}

}  // namespace

extern "C" {

int vd_sample_init(int64_t rows, int beam_len, int start_token, int32_t* hist, int32_t* tok, double* loglik, int32_t* status,
                   void* stream) {
  VD_CHECK_ARG(hist && tok && loglik && status && rows >= 0 && beam_len >= 1, "vd_sample_init: bad args");
  hipLaunchKernelGGL(sample_init_kernel, dim3(grid_for(rows * (beam_len + 1))), dim3(256), 0, (hipStream_t)stream, (long)rows,
                     beam_len + 1, start_token, hist, tok, loglik, status);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

int vd_sample_draw(const float* logits, int64_t ld, int64_t rows, int V, int32_t* tok, const double* uniforms, double temperature,
                   int step, int beam_len, int end_token, int32_t* hist, double* loglik, int32_t* status, void* stream) {
  VD_CHECK_ARG(logits && tok && uniforms && hist && loglik && status && rows >= 0 && V >= 1 && ld >= V, "vd_sample_draw: bad args");
  VD_CHECK_ARG(std::isfinite(temperature) && temperature > 0, "vd_sample_draw: temperature %g must be finite and > 0", temperature);
  VD_CHECK_ARG(step >= 1 && step <= beam_len, "vd_sample_draw: step %d outside [1, %d]", step, beam_len);
  if (rows == 0) return VD_OK;
  hipLaunchKernelGGL(sample_draw_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, logits, (long)ld, V, tok, uniforms,
                     temperature, step, beam_len + 1, end_token, hist, loglik, status);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

}  // extern "C"
