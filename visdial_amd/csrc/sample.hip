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
//
// Top-k / nucleus truncation (a model created with VD_SAMPLE_TOPK / VD_SAMPLE_TOPP; sample_draw_kernel<true>, reached only through
// vd_model_sample): between rules 2 and 3 every column outside the kept set gets weight 0, rules 3-5 run on what is left and the
// log-likelihood still adds the UNtruncated logp[c].  The host statement is split_eval.truncated_weights.  The kept set:
//  T1. order: logp descending as fp32 values (-0 = +0), equal values by ascending column.  key(c) = the bits of logp[c] for a
//      negative value, bits ^ 0x7fffffff otherwise, so ascending unsigned key = that order with ties left to the column.
//  T2. topK = k > 0 (the caller passes 0 for k >= V): the first k of the order.
//  T3. topP = p < 1: masses are 64-bit INTEGERS q[c] = trunc(exp(((double)logp[c] - (double)max logp) / temperature) * 2^40)
//      (0 where that is not > 0), so every sum of them is exact and no result depends on the order LDS atomics arrive in: two
//      calls on the same inputs give the same tokens.  Q = the sum of q over what T2 kept (every column without T2), target =
//      min(Q, max(1, ceil(p * (double)Q))); kept is the shortest prefix of the order whose q sum reaches the target: at least one
//      column, none with q = 0, and never more than T2 kept.  Q = 0 (NaN logits): T3 is skipped and rule 4 reports the row.
//      q is used for this decision only; the draw keeps w of rule 2.  Against the host's fp64 prefix sums the set can differ only
//      where a prefix mass is within V * 2^-40 (relative to the largest weight) plus fp64 rounding of p * S_k.
//  T4. how: the kept set is {key < B} + {key = B and c <= I}.  B comes from a radix select over the keys, four passes of 8 bits
//      from the top; a pass re-reads the row from global memory (it stays in L2, so V is not bound by LDS), histograms the
//      columns that match the prefix found so far into 256 LDS bins (count and q sum; a thread adds a run of equal bins once),
//      and a block scan over the bins finds the one where the running count reaches k (T2) or the running q sum reaches the
//      target (T3).  T2's select also yields Q: the q sum of the bins before B plus (ties kept) * q(B).  With both knobs on,
//      T3's prefix lies inside T2's set, so T3's (B, ties) is the answer.  The first pass is shared by both selects.  The ties
//      kept are the first m of key = B by column: m = k - count(key < B), or ceil((target - q sum before B) / q(B)); I = the
//      column of the m-th, from a scan over the threads' contiguous chunks.
//  Every loop runs over V, 256 bins or 4 passes; every branch around a barrier is block-uniform.
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

// ---- top-k / nucleus truncation (T1-T4 of the header) ----------------------------------------------------------------------------
constexpr double TRUNC_SCALE = 1099511627776.0;   // 2^40: V < 2^23 (vd_model_create's table bound) keeps every q sum below 2^63

__device__ __forceinline__ uint32_t trunc_key(float lp) {
  const uint32_t b = __float_as_uint(lp + 0.f);
  return (b >> 31) ? b : b ^ 0x7fffffffu;
}
__device__ __forceinline__ float trunc_key_value(uint32_t k) { return __uint_as_float((k >> 31) ? k : k ^ 0x7fffffffu); }
__device__ __forceinline__ unsigned long long trunc_mass(float lp, float lp_max, double temperature) {
  const double e = exp(((double)lp - (double)lp_max) / temperature) * TRUNC_SCALE;
  return e > 0.0 ? (unsigned long long)e : 0ull;
}

// inclusive scan of one value per thread over the block of 256, threads in order; `tot` = the block's sum; wt: 4 shared words
__device__ __forceinline__ unsigned long long block_scan_u64(unsigned long long v, unsigned long long* wt, unsigned long long* tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long y = __shfl_up(v, o, 64);
    if (lane >= o) v += y;
  }
  __syncthreads();                      // the previous scan's readers are done with wt
  if (lane == 63) wt[wave] = v;
  __syncthreads();
  for (int w = 0; w < wave; ++w) v += wt[w];
  *tot = (wt[0] + wt[1]) + (wt[2] + wt[3]);
  return v;
}

struct TruncShared {
  uint32_t cnt[256];
  unsigned long long mass[256];
  unsigned long long wt[4];
  uint32_t bin;                  // the bin a pass selected
  unsigned long long rem, below; // what is left of the target inside that bin; (T2) the q sum of the bins before it
};

// one histogram pass: columns whose key matches `prefix` above bit shift + 8, binned by key bits [shift, shift + 8); the q sums only
// `with_mass` (block-uniform; top-k alone needs none)
__device__ __forceinline__ void trunc_histogram(const float* row, int V, float lse, bool zero_row, float lp_max, double temperature,
                                                bool with_mass, uint32_t prefix, int shift, TruncShared& sh) {
  const int tid = threadIdx.x;
  const uint32_t hi = shift == 24 ? 0u : ~0u << (shift + 8);
  sh.cnt[tid] = 0;
  sh.mass[tid] = 0;
  __syncthreads();
  int cur = -1;
  uint32_t n = 0;
  unsigned long long q = 0;
  for (int c = tid; c < V; c += 256) {
    const float lp = zero_row ? 0.f : row[c] - lse;
    const uint32_t k = trunc_key(lp);
    if ((k & hi) != prefix) continue;
    const int b = (int)((k >> shift) & 255u);
    if (b != cur) {
      if (n) { atomicAdd(&sh.cnt[cur], n); atomicAdd(&sh.mass[cur], q); }
      cur = b; n = 0; q = 0;
    }
    ++n;
    if (with_mass) q += trunc_mass(lp, lp_max, temperature);
  }
  if (n) { atomicAdd(&sh.cnt[cur], n); atomicAdd(&sh.mass[cur], q); }
  __syncthreads();
}

// the bin where the running total of `mine` (this thread's bin) reaches `target` (1 <= target <= the sum over the bins, which
// the callers guarantee): sh.bin, sh.rem = target - the total before it, sh.below += `carry` summed over the bins before it
// (`with_carry`, block-uniform)
__device__ __forceinline__ void trunc_pick_bin(unsigned long long mine, bool with_carry, unsigned long long carry, unsigned long long target,
                                               TruncShared& sh) {
  unsigned long long tot, cincl = carry;
  const unsigned long long incl = block_scan_u64(mine, sh.wt, &tot);
  if (with_carry) cincl = block_scan_u64(carry, sh.wt, &tot);
  if (incl - mine < target && target <= incl) {   // exactly one bin
    sh.bin = threadIdx.x;
    sh.rem = target - (incl - mine);
    sh.below += cincl - carry;
  }
  __syncthreads();
}

// rules 1-5 for one row per workgroup; TRUNC: with T1-T4 between rules 2 and 3 (top_k / top_p are read with TRUNC only)
template <bool TRUNC>
__global__ void __launch_bounds__(256)
sample_draw_kernel(const float* __restrict__ x, long ld, int V, int32_t* __restrict__ tok, const double* __restrict__ u,
                   double temperature, int top_k, double top_p, int step, int cols, int end_tok, int32_t* __restrict__ hist,
                   double* __restrict__ loglik, int32_t* __restrict__ status) {
  __shared__ float red[8];
  __shared__ double wtot[4];
  __shared__ int owner, last_pos, pick;
  const long r = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* row = x + r * ld;
  const bool zero_row = tok[r] == 0;
  float lse = 0.f, lp_max = 0.f;
  if (!zero_row) {
    lse = block_row_lse(row, V, red);   // rule 1
    if constexpr (TRUNC) lp_max = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) - lse;   // the row maximum block_row_lse left behind
  }
  const int chunk = (V + 255) / 256;   // thread t owns the columns [c0, c1)
  const int c0 = min(V, tid * chunk), c1 = min(V, c0 + chunk);

  uint32_t B = 0xffffffffu;            // the kept set {key < B} + {key = B and c <= I}: every column unless T2 / T3 cut
  int I = V - 1;
  if constexpr (TRUNC) {
    __shared__ TruncShared sh;
    __shared__ int tie_col;
    // T4, first pass: shared by both selects, each thread keeps its bin
    const bool with_mass = top_p < 1.0;
    if (tid == 0) { sh.bin = 255; sh.rem = 0; sh.below = 0; tie_col = V - 1; }
    trunc_histogram(row, V, lse, zero_row, lp_max, temperature, with_mass, 0u, 24, sh);
    const uint32_t cnt1 = sh.cnt[tid];
    const unsigned long long mass1 = sh.mass[tid];
    unsigned long long ties = 0;       // how many of the boundary key's ties are kept
    bool cut = false;
    unsigned long long Q;
    {
      unsigned long long t;
      (void)block_scan_u64(mass1, sh.wt, &t);
      Q = t;
    }
    if (top_k > 0) {                   // T2 (block-uniform: kernel arguments only)
      uint32_t prefix = 0;
      unsigned long long target = (unsigned long long)top_k;
      for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (pass) trunc_histogram(row, V, lse, zero_row, lp_max, temperature, with_mass, prefix, shift, sh);
        trunc_pick_bin(pass ? sh.cnt[tid] : cnt1, with_mass, pass ? sh.mass[tid] : mass1, target, sh);
        prefix |= sh.bin << shift;
        target = sh.rem;
      }
      B = prefix;
      ties = target;
      cut = true;
      Q = sh.below + ties * trunc_mass(trunc_key_value(B), lp_max, temperature);
    }
    if (top_p < 1.0 && Q > 0) {        // T3 (block-uniform: Q comes from shared memory)
      const double want = ceil(top_p * (double)Q);
      unsigned long long target = want >= 1.0 ? (unsigned long long)want : 1ull;
      if (target > Q) target = Q;
      uint32_t prefix = 0;
      for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (pass) trunc_histogram(row, V, lse, zero_row, lp_max, temperature, with_mass, prefix, shift, sh);
        trunc_pick_bin(pass ? sh.mass[tid] : mass1, false, 0ull, target, sh);
        prefix |= sh.bin << shift;
        target = sh.rem;
      }
      B = prefix;
      const unsigned long long qb = trunc_mass(trunc_key_value(B), lp_max, temperature);
      ties = qb ? (target + qb - 1) / qb : 1ull;
      cut = true;
    }
    if (cut) {                         // T4: the column of the last tie kept
      unsigned long long mine = 0;
      for (int c = c0; c < c1; ++c) mine += trunc_key(zero_row ? 0.f : row[c] - lse) == B;
      unsigned long long tot;
      const unsigned long long incl = block_scan_u64(mine, sh.wt, &tot);
      if (incl - mine < ties && ties <= incl) {
        unsigned long long seen = incl - mine;
        for (int c = c0; c < c1; ++c)
          if (trunc_key(zero_row ? 0.f : row[c] - lse) == B && ++seen == ties) { tie_col = c; break; }
      }
      __syncthreads();
    }
    I = tie_col;
  }
  // rule 2 on the kept set
  auto weight = [&](int c) -> double {
    if constexpr (TRUNC) {
      const float lp = zero_row ? 0.f : row[c] - lse;
      const uint32_t k = trunc_key(lp);
      return (k < B || (k == B && c <= I)) ? exp((double)lp / temperature) : 0.0;
    } else {
      return sample_weight(row, c, lse, zero_row, temperature);
    }
  };

  // rules 2-3: chunk sums, then the block's exclusive scan of them
  double part = 0.0;
  for (int c = c0; c < c1; ++c) part += weight(c);
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
        const double w = weight(c);
        run += w;
        if (w > 0.0 && excl + run > target) { pick = c; break; }
      }
    }
  } else if (tid == last_pos) {          // u within rounding of 1
    for (int c = c1 - 1; c >= c0; --c)
      if (weight(c) > 0.0) { pick = c; break; }
  }
  __syncthreads();
  if (tid != 0) return;
  const int c = pick;
  if (c < 0) {                           // rule 4: NaN weights leave nothing to draw from
    *status = 1; hist[r * cols + step] = 0; tok[r] = 0;
    return;
  }
  const float lp = zero_row ? 0.f : row[c] - lse;   // rule 5: the untruncated log-probability
  const int32_t* h = hist + r * cols;
  bool ended = false;
  for (int p = 1; p < step; ++p) ended = ended || h[p] == end_tok;
  if (!ended) loglik[r] += (double)lp;
  hist[r * cols + step] = c + 1;
  tok[r] = c + 1;
}

// vd_sample_draw and vd_sample_draw_trunc_p (TRUNC) behind their argument lists; `who` prefixes the error texts
template <bool TRUNC>
int sample_draw(const char* who, const float* logits, int64_t ld, int64_t rows, int V, int32_t* tok, const double* uniforms, double temperature,
                int top_k, double top_p, int step, int beam_len, int end_token, int32_t* hist, double* loglik, int32_t* status,
                hipStream_t stream) {
  VD_CHECK_ARG(logits && tok && uniforms && hist && loglik && status && rows >= 0 && V >= 1 && ld >= V, "%s: bad args", who);
  VD_CHECK_ARG(std::isfinite(temperature) && temperature > 0, "%s: temperature %g must be finite and > 0", who, temperature);
  VD_CHECK_ARG(step >= 1 && step <= beam_len, "%s: step %d outside [1, %d]", who, step, beam_len);
  if constexpr (TRUNC)
    VD_CHECK_ARG(top_k >= 0 && top_k < V && top_p > 0.0 && top_p <= 1.0 && (top_k > 0 || top_p < 1.0) && V < (1 << 23),
                 "%s: top_k %d must lie in [0, V = %d), top_p %g in (0, 1], one of them on, V below 2^23", who, top_k, V, top_p);
  if (rows == 0) return VD_OK;
  hipLaunchKernelGGL(sample_draw_kernel<TRUNC>, dim3((unsigned)rows), dim3(256), 0, stream, logits, (long)ld, V, tok, uniforms, temperature,
                     top_k, top_p, step, beam_len + 1, end_token, hist, loglik, status);
  VD_LAUNCH_CHECK();
  return VD_OK;
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
  return sample_draw<false>("vd_sample_draw", logits, ld, rows, V, tok, uniforms, temperature, 0, 1.0, step, beam_len, end_token, hist, loglik,
                            status, (hipStream_t)stream);
}

}  // extern "C"

// vd_sample_draw with the kept set of T1-T4: top_k in [0, V) (0 = off), top_p in (0, 1] (1 = off), at least one of them on.  Internal to
// the library (csrc/rt_core.h): vd_model_sample of a model created with VD_SAMPLE_TOPK / VD_SAMPLE_TOPP.
int vd_sample_draw_trunc_p(const float* logits, int64_t ld, int64_t rows, int V, int32_t* tok, const double* uniforms, double temperature,
                           int top_k, double top_p, int step, int beam_len, int end_token, int32_t* hist, double* loglik, int32_t* status,
                           hipStream_t stream) {
  return sample_draw<true>("vd_sample_draw_trunc_p", logits, ld, rows, V, tok, uniforms, temperature, top_k, top_p, step, beam_len, end_token,
                           hist, loglik, status, stream);
}
