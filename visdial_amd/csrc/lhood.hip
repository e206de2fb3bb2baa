// Live-row log-likelihood head of generative retrieval (model.lua:392-420 + utils.computeLhood, utils.lua:86-102).
//
// A candidate answer is left-aligned (option_in = <START> w1..wL 0.., option_out = w1..wL <END> 0..): of the T x rows (step, candidate)
// rows the decoder LSTM produces, only those with option_in != 0 and option_out > 0 count, and from each of them retrieval needs
// two scalars: the logit of the target token and the row's log-sum-exp.  So instead of vd_gemm_nt over ALL rows into a
// [rows x V] logits buffer + vd_logsoftmax_nll over it, three kernels:
//   vd_lhood_live_rows  the list `act` of live linear row indices (ascending = step-major, then candidate), counted on the device
//   vd_lhood_nll        nll[i] = logsumexp_v(h[act[i]] . W[v] + bias[v]) - (h[act[i]] . W[target - 1] + bias[target - 1]):
//                       fp32 MFMA over the live rows only, online log-sum-exp in registers, no logits in memory
//   vd_lhood_sum        score[candidate] = -(sum of its rows' nll, in step order)
// With a length order of the chunk's candidates (lhood_order_*, below) the recurrence in front of the head runs only where there are
// tokens (VD_FLAG_LIVE_PREFIX) and vd_lhood_sum scatters the scores back to candidate order.
// Everything is deterministic: no atomics, fixed reduction orders, and a row's arithmetic does not depend on where in a tile it sits.
#include "gemm_core.h"
#include "paths.h"

// ---- vd_lhood_nll, throughput shapes ---------------------------------------------------------------------------------------------
// The product is computed TRANSPOSED: the MFMA's A operand is the vocabulary matrix W [V x H], the B operand the live rows of h
// gathered through `act` (gemm_block_glds `brows`).  An accumulator lane then holds 16 vocabulary entries of ONE live row per
// 32 x 32 tile (column = lane & 31), so the running (max, sum, target logit) of a row are plain per-lane registers and the hot
// loop has no cross-lane traffic.  A workgroup owns 128 live rows and walks the vocabulary in 128-wide tiles through the
// LDS-DMA pipeline vd_gemm_nt uses for the dense head; after the last tile the 8 partial states of a row (4 waves = 4 groups of
// 32 vocabulary rows per tile, x 2 lane halves) are combined through LDS in a fixed order.  The K order of every tile is fixed
// (no K-tile rotation): two live rows with the same h row and target get the same bits whatever tile or lane they land in.
// Tile = vd_gemm_nt's throughput tile (128 x 128, BK 16), which its LDS request holds to 3 workgroups per CU; here the register
// budget says so too (3 waves per SIMD = 168 registers: the running state lives across the K loop), and the LDS request is three DMA
// buffers for BOTH operands (48 KB).
using LhoodCfg = GemmCfg<4, 1, 4, 16, 0, 3, 49152>;

struct LhoodState {
  float m[4], s[4], pick[4];   // per live row of the lane: running max, running sum of exp(x - m), target logit (0 until seen)
  int tgt[4];                  // 0-based target column, -1 for a row beyond n_act
};

struct EpiLhood {
  const float* bias;   // [V] or null
  LhoodState* st;
  // acc[j][r] = logit (without bias) of vocabulary entry row0 + mfma_row(r, lane) for live row col0 + j * 32 + (lane & 31); M = V
  __device__ __forceinline__ void operator()(const f32x16 (&acc)[4], int row0, int /*col0*/, int lane, int M, int /*N*/,
                                             float* /*scr*/ = nullptr) const {
    const int v0 = row0 + 4 * (lane >> 5);
    float bv[16];   // bias, or -inf for the entries of a ragged last tile: x = acc + (-inf) drops out of max and sum
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int v = v0 + (r & 3) + 8 * (r >> 2);
      bv[r] = v < M ? (bias ? bias[v] : 0.f) : -INFINITY;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int rel = st->tgt[j] - v0;
      float tmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float x = acc[j][r] + bv[r];
        tmax = fmaxf(tmax, x);
        if (rel == (r & 3) + 8 * (r >> 2)) st->pick[j] = x;
      }
      const float mo = st->m[j], mn = fmaxf(mo, tmax);
      if (mn > -INFINITY) {   // else: nothing but masked entries so far
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += __expf((acc[j][r] + bv[r]) - mn);   // recomputed: 16 fewer live registers
        st->s[j] = st->s[j] * __expf(mo - mn) + sum;
        st->m[j] = mn;
      }
    }
  }
};

__global__ void __launch_bounds__(LhoodCfg::THREADS, LhoodCfg::MINW)
lhood_nll_mfma_kernel(const float* __restrict__ h, long ldh, const int* __restrict__ act, int n_act, const int* __restrict__ target,
                      const float* __restrict__ W, long ldw, const float* __restrict__ bias, int V, int K, float* __restrict__ nll) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col_base = blockIdx.x * LhoodCfg::BN;
  LhoodState st;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = col_base + j * 32 + (lane & 31);
    st.m[j] = -INFINITY;
    st.s[j] = 0.f;
    st.pick[j] = 0.f;
    st.tgt[j] = col < n_act ? target[act[col]] - 1 : -1;
  }
  const EpiLhood epi{bias, &st};
  const int tiles_v = (V + LhoodCfg::BM - 1) / LhoodCfg::BM;
  for (int vt = 0; vt < tiles_v; ++vt) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));   // per-lane address terms are re-derived per tile, not kept live across the epilogue
    gemm_block_glds<LhoodCfg, false>(V, n_act, 0, K, vt * LhoodCfg::BM, col_base, -1, W, ldw, h, ldh, epi, smem, tid, act);
  }
  // combine the 8 partial states of each of the 128 live rows, partial p = wave * 2 + lane half, in the order p = 0..7
  __syncthreads();   // every wave is past its last fragment read: the DMA buffers are free
  float* red = smem;   // [3][8][128]
  const int p = wave * 2 + (lane >> 5);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = j * 32 + (lane & 31);
    red[(0 * 8 + p) * 128 + c] = st.m[j];
    red[(1 * 8 + p) * 128 + c] = st.s[j];
    red[(2 * 8 + p) * 128 + c] = st.pick[j];
  }
  __syncthreads();
  const int c = threadIdx.x, col = col_base + c;
  if (c >= 128 || col >= n_act) return;
  float mx = -INFINITY;
#pragma unroll
  for (int q = 0; q < 8; ++q) mx = fmaxf(mx, red[(0 * 8 + q) * 128 + c]);
  float sum = 0.f, pick = 0.f;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float mq = red[(0 * 8 + q) * 128 + c];
    if (mq > -INFINITY) sum += red[(1 * 8 + q) * 128 + c] * expf(mq - mx);
    pick += red[(2 * 8 + q) * 128 + c];   // seven of them are exactly 0
  }
  nll[col] = (mx + logf(sum)) - pick;
}

// ---- vd_lhood_nll, every other shape (the small H and V of the test models): one 256-thread workgroup per live row, the h row in
// LDS, thread t takes vocabulary entries t, t + 256, ... with a sequential dot product and its own online (max, sum); the wave and
// workgroup combines are butterflies and a fixed-order sum.  Same result contract, no MFMA.
__global__ void __launch_bounds__(256)
lhood_nll_rows_kernel(const float* __restrict__ h, long ldh, const int* __restrict__ act, const int* __restrict__ target,
                      const float* __restrict__ W, long ldw, const float* __restrict__ bias, int V, int K, float* __restrict__ nll) {
  extern __shared__ __attribute__((aligned(16))) float hs[];
  __shared__ float red[3][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long row = act[blockIdx.x];
  const int tgt = target[row] - 1;
  for (int k = tid; k < K; k += 256) hs[k] = h[row * ldh + k];
  __syncthreads();
  float m = -INFINITY, s = 0.f, pick = 0.f;
  for (int v = tid; v < V; v += 256) {
    const float* w = W + (long)v * ldw;
    float x = bias ? bias[v] : 0.f;
    for (int k = 0; k < K; ++k) x = fmaf(hs[k], w[k], x);
    if (v == tgt) pick = x;
    const float mn = fmaxf(m, x);
    s = s * expf(m - mn) + expf(x - mn);   // m = -inf at first: s = 0 * 0
    m = mn;
  }
  const float mw = wave_max(m);
  s = wave_sum(m > -INFINITY ? s * expf(m - mw) : 0.f);
  pick = wave_sum(pick);
  if (lane == 0) {
    red[0][wave] = mw;
    red[1][wave] = s;
    red[2][wave] = pick;
  }
  __syncthreads();
  if (tid != 0) return;
  const float mx = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
  float sum = 0.f, pk = 0.f;
  for (int q = 0; q < 4; ++q) {
    if (red[0][q] > -INFINITY) sum += red[1][q] * expf(red[0][q] - mx);
    pk += red[2][q];
  }
  nll[blockIdx.x] = (mx + logf(sum)) - pk;
}

// ---- the prefix-tree head (vd_lhood_lse_p below): the twin of lhood_nll_mfma_kernel without a target -- the same tiles, the same
// pipeline, the same online max / sum (EpiLhood with every target at -1) and the same combine; lse[i] is the listed row's
// log-sum-exp.  A kernel of its own, so that lhood_nll_mfma_kernel stays as it is.
__global__ void __launch_bounds__(LhoodCfg::THREADS, LhoodCfg::MINW)
lhood_lse_mfma_kernel(const float* __restrict__ h, long ldh, const int* __restrict__ act, int n_act, const float* __restrict__ W, long ldw,
                      const float* __restrict__ bias, int V, int K, float* __restrict__ lse) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col_base = blockIdx.x * LhoodCfg::BN;
  LhoodState st;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    st.m[j] = -INFINITY;
    st.s[j] = 0.f;
    st.pick[j] = 0.f;
    st.tgt[j] = -1;
  }
  const EpiLhood epi{bias, &st};
  const int tiles_v = (V + LhoodCfg::BM - 1) / LhoodCfg::BM;
  for (int vt = 0; vt < tiles_v; ++vt) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));   // per-lane address terms are re-derived per tile, not kept live across the epilogue
    gemm_block_glds<LhoodCfg, false>(V, n_act, 0, K, vt * LhoodCfg::BM, col_base, -1, W, ldw, h, ldh, epi, smem, tid, act);
  }
  // combine the 8 partial states of each of the 128 listed rows, partial p = wave * 2 + lane half, in the order p = 0..7
  __syncthreads();
  float* red = smem;   // [2][8][128]
  const int p = wave * 2 + (lane >> 5);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = j * 32 + (lane & 31);
    red[(0 * 8 + p) * 128 + c] = st.m[j];
    red[(1 * 8 + p) * 128 + c] = st.s[j];
  }
  __syncthreads();
  const int c = threadIdx.x, col = col_base + c;
  if (c >= 128 || col >= n_act) return;
  float mx = -INFINITY;
#pragma unroll
  for (int q = 0; q < 8; ++q) mx = fmaxf(mx, red[(0 * 8 + q) * 128 + c]);
  float sum = 0.f;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float mq = red[(0 * 8 + q) * 128 + c];
    if (mq > -INFINITY) sum += red[(1 * 8 + q) * 128 + c] * expf(mq - mx);
  }
  lse[col] = mx + logf(sum);
}

// the twin of lhood_nll_rows_kernel without a target (small shapes of the prefix-tree head)
__global__ void __launch_bounds__(256)
lhood_lse_rows_kernel(const float* __restrict__ h, long ldh, const int* __restrict__ act, const float* __restrict__ W, long ldw,
                      const float* __restrict__ bias, int V, int K, float* __restrict__ lse) {
  extern __shared__ __attribute__((aligned(16))) float hs[];
  __shared__ float red[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long row = act[blockIdx.x];
  for (int k = tid; k < K; k += 256) hs[k] = h[row * ldh + k];
  __syncthreads();
  float m = -INFINITY, s = 0.f;
  for (int v = tid; v < V; v += 256) {
    const float* w = W + (long)v * ldw;
    float x = bias ? bias[v] : 0.f;
    for (int k = 0; k < K; ++k) x = fmaf(hs[k], w[k], x);
    const float mn = fmaxf(m, x);
    s = s * expf(m - mn) + expf(x - mn);   // m = -inf at first: s = 0 * 0
    m = mn;
  }
  const float mw = wave_max(m);
  s = wave_sum(m > -INFINITY ? s * expf(m - mw) : 0.f);
  if (lane == 0) {
    red[0][wave] = mw;
    red[1][wave] = s;
  }
  __syncthreads();
  if (tid != 0) return;
  const float mx = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
  float sum = 0.f;
  for (int q = 0; q < 4; ++q)
    if (red[0][q] > -INFINITY) sum += red[1][q] * expf(red[0][q] - mx);
  lse[blockIdx.x] = mx + logf(sum);
}

// ---- edge sum of the prefix-tree head: candidate r walks its (node, target) edges in step order,
//   score[r] = sum_t ( W[target_t - 1] . h[row of node(r, t)] + bias[target_t - 1] - lse[node(r, t)] ).
// One wave per candidate: the 64 lanes read the W row and the h row in 16-byte pieces (coalesced), a butterfly adds the lanes' partial
// dot products in a fixed order, lane 0 adds the terms in step order and stores straight into candidate order.  No atomics; two
// identical candidates walk the same nodes and tie exactly; a candidate without an edge scores +0.
__global__ void __launch_bounds__(256)
lhood_edge_sum_kernel(const float* __restrict__ h, long ldh, const int* __restrict__ node_row, const float* __restrict__ lse,
                      const int* __restrict__ enode, const int* __restrict__ etgt, int T, long rows, int C, const float* __restrict__ W,
                      long ldw, const float* __restrict__ bias, int K, float* __restrict__ out, long ldo) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  float sum = 0.f;
  for (int t = 0; t < T; ++t) {
    const int tgt = etgt[t * rows + r];
    if (tgt <= 0) continue;   // (uniform over the wave)
    const int nd = enode[t * rows + r];
    const float* hr = h + (long)node_row[nd] * ldh;
    const float* wr = W + (long)(tgt - 1) * ldw;
    float d = 0.f;
    for (int k = lane * 4; k < K; k += 256) {
      const float4 a = *reinterpret_cast<const float4*>(hr + k), w = *reinterpret_cast<const float4*>(wr + k);
      d = fmaf(a.x, w.x, d); d = fmaf(a.y, w.y, d); d = fmaf(a.z, w.z, d); d = fmaf(a.w, w.w, d);
    }
    d = wave_sum(d);
    sum += (d + (bias ? bias[tgt - 1] : 0.f)) - lse[nd];
  }
  if (lane == 0) out[(r / C) * ldo + r % C] = sum;
}

// ---- vd_lhood_live_rows: stream compaction in index order.  Pass 1 counts the live rows of every 1024-row block; pass 2 gives each
// block the sum of the counts before it and each thread its rank inside the block (wave prefix by shuffles + the waves' totals).
__device__ __forceinline__ bool lhood_live(const int* tok_in, const int* target, long i, long n) {
  return i < n && tok_in[i] != 0 && target[i] > 0;
}
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(256)
lhood_live_count_kernel(const int* __restrict__ tok_in, const int* __restrict__ target, long n, int* __restrict__ counts) {
  __shared__ int red[4];
  const int tid = threadIdx.x;
  const long base = (long)blockIdx.x * 1024 + tid * 4;
  int c = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) c += lhood_live(tok_in, target, base + q, n) ? 1 : 0;
  c = wave_sum_int(c);
  if ((tid & 63) == 0) red[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) counts[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ void __launch_bounds__(256)
lhood_live_write_kernel(const int* __restrict__ tok_in, const int* __restrict__ target, long n, const int* __restrict__ counts,
                        int* __restrict__ act, int* __restrict__ total) {
  __shared__ int red[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int before = 0;
  for (int b = tid; b < (int)blockIdx.x; b += 256) before += counts[b];
  before = wave_sum_int(before);
  const long base = (long)blockIdx.x * 1024 + tid * 4;
  bool live[4];
  int c = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    live[q] = lhood_live(tok_in, target, base + q, n);
    c += live[q] ? 1 : 0;
  }
  int incl = c;   // inclusive prefix over the wave's lanes
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  if (lane == 0) red[wave] = before;
  if (lane == 63) red[4 + wave] = incl;
  __syncthreads();
  int pos = red[0] + red[1] + red[2] + red[3] + (incl - c);
  for (int w = 0; w < wave; ++w) pos += red[4 + w];
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (live[q]) act[pos++] = (int)(base + q);
  if (blockIdx.x == gridDim.x - 1 && tid == 255) *total = pos;
}

// ---- vd_lhood_sum: one thread per candidate; `act` is ascending, so the position of row t * rows + r is a binary search, and the
// candidate's terms are added in step order
__global__ void __launch_bounds__(256)
lhood_sum_kernel(const float* __restrict__ nll, const int* __restrict__ act, int n_act, int T, long rows, int C, float* __restrict__ out,
                 long ldo, const int* __restrict__ perm) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  float sum = 0.f;
  for (int t = 0; t < T; ++t) {
    const int want = (int)(t * rows + r);
    int lo = 0, hi = n_act;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (act[mid] < want) lo = mid + 1;
      else hi = mid;
    }
    if (lo < n_act && act[lo] == want) sum += nll[lo];
  }
  const long cand = perm ? perm[r] : r;   // length-ordered rows: back to candidate order
  out[(cand / C) * ldo + cand % C] = 0.f - sum;   // a candidate without a live row scores +0
}

// ---- length order of a chunk's candidates (rows = round x option of tok_in [T x rows]): a STABLE counting sort by descending length, in
// the style of vd_lhood_live_rows -- a count per block, then block offset + rank inside the block; no atomics, so equal lengths keep
// their row order from run to run (vd_token_sort's atomic bucket cursor does not).  length = number of leading non-pad steps, key = T -
// length in [0, T].  Pass 1, one row per thread: length, "hole" (a token behind the first pad: not one left-aligned run), and per block
// the count of every key (thread k counts key k in the block's LDS key list) and whether a row has a hole.  Pass 2: thread k sums key
// k's counts over the blocks (before this block / all), thread 0 turns them into the block's first position per key; a row's position =
// that + the rows of its key before it in the block.  Block 0 also writes info = [holed rows?, nact[0 .. T)], nact[t] = rows longer than
// t: in this order the non-pad rows of step t are rows [0, nact[t]) and nact falls with t.
constexpr int ORDER_ROWS = 256;   // rows per block = threads; T + 1 keys <= ORDER_ROWS (paths.h vd_lhood_prefix_fits)

__global__ void __launch_bounds__(ORDER_ROWS)
lhood_order_count_kernel(const int* __restrict__ tok_in, int T, long rows, int* __restrict__ len_out, int* __restrict__ counts,
                         int* __restrict__ holes) {
  __shared__ int keys[ORDER_ROWS];
  const int tid = threadIdx.x;
  const long r = (long)blockIdx.x * ORDER_ROWS + tid;
  int len = 0, hole = 0, key = -1;
  if (r < rows) {
    bool run = true;
    for (int t = 0; t < T; ++t) {
      const bool tok = tok_in[(long)t * rows + r] != 0;
      run = run && tok;
      len += run ? 1 : 0;
      hole |= (!run && tok) ? 1 : 0;
    }
    len_out[r] = len;
    key = T - len;
  }
  keys[tid] = key;
  const int any_hole = __syncthreads_or(hole);   // (also the barrier behind the key list)
  if (tid == 0) holes[blockIdx.x] = any_hole ? 1 : 0;
  if (tid <= T) {
    int c = 0;
    for (int j = 0; j < ORDER_ROWS; ++j) c += keys[j] == tid ? 1 : 0;
    counts[(long)blockIdx.x * (T + 1) + tid] = c;
  }
}

__global__ void __launch_bounds__(ORDER_ROWS)
lhood_order_write_kernel(const int* __restrict__ len, int T, long rows, int C, const int* __restrict__ counts, const int* __restrict__ holes,
                         int* __restrict__ perm, int* __restrict__ rep, int* __restrict__ info) {
  __shared__ int keys[ORDER_ROWS], before[ORDER_ROWS], total[ORDER_ROWS], first[ORDER_ROWS];
  const int tid = threadIdx.x, nb = (int)gridDim.x;
  const long r = (long)blockIdx.x * ORDER_ROWS + tid;
  const int key = r < rows ? T - len[r] : -1;
  keys[tid] = key;
  if (tid <= T) {
    int bef = 0, all = 0;
    for (int b = 0; b < nb; ++b) {
      const int c = counts[(long)b * (T + 1) + tid];
      all += c;
      bef += b < (int)blockIdx.x ? c : 0;
    }
    before[tid] = bef;
    total[tid] = all;
  }
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int k = 0; k <= T; ++k) {
      first[k] = run + before[k];
      run += total[k];
    }
    if (blockIdx.x == 0) {
      int holed = 0;
      for (int b = 0; b < nb; ++b) holed |= holes[b];
      info[0] = holed;
      int longer = 0;   // rows with key < T - t  <=>  length > t
      for (int t = T - 1; t >= 0; --t) {
        longer += total[T - 1 - t];
        info[1 + t] = longer;
      }
    }
  }
  __syncthreads();
  if (r >= rows) return;
  int rank = 0;
  for (int j = 0; j < tid; ++j) rank += keys[j] == key ? 1 : 0;
  const int pos = first[key] + rank;
  perm[pos] = (int)r;
  rep[pos] = (int)(r / C);   // the round whose encoder state the candidate starts from (forwardConnect replication)
}

// tokens and targets in that order: dst[t][p] = src[t][perm[p]]
__global__ void __launch_bounds__(256)
lhood_order_gather_kernel(const int* __restrict__ a, const int* __restrict__ b, const int* __restrict__ perm, int T, long rows,
                          int* __restrict__ a_s, int* __restrict__ b_s) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)T * rows) return;
  const long t = i / rows, src = t * rows + perm[i - t * rows];
  a_s[i] = a[src];
  b_s[i] = b[src];
}

int64_t vd_lhood_order_work_ints(int T, int64_t rows) {
  const int64_t blocks = (rows + ORDER_ROWS - 1) / ORDER_ROWS;
  return rows + blocks * (T + 1) + blocks;
}

int vd_lhood_order_p(const int32_t* tok_in, const int32_t* target, int T, int64_t rows, int C, int32_t* perm, int32_t* rep, int32_t* tok_in_s,
                     int32_t* target_s, int32_t* work, int32_t* info, hipStream_t s) {
  VD_CHECK_ARG(tok_in && target && perm && rep && tok_in_s && target_s && work && info && C >= 1 && vd_lhood_prefix_fits(T, rows) &&
                   (long)T * rows < (1L << 31),
               "lhood order: bad args T=%d rows=%ld", T, (long)rows);
  const int blocks = vd_cdiv(rows, ORDER_ROWS);
  int32_t *len = work, *counts = work + rows, *holes = counts + (long)blocks * (T + 1);
  hipLaunchKernelGGL(lhood_order_count_kernel, dim3(blocks), dim3(ORDER_ROWS), 0, s, tok_in, T, (long)rows, len, counts, holes);
  VD_LAUNCH_CHECK();
  hipLaunchKernelGGL(lhood_order_write_kernel, dim3(blocks), dim3(ORDER_ROWS), 0, s, len, T, (long)rows, C, counts, holes, perm, rep, info);
  VD_LAUNCH_CHECK();
  hipLaunchKernelGGL(lhood_order_gather_kernel, dim3(vd_cdiv((long)T * rows, 256)), dim3(256), 0, s, tok_in, target, perm, T, (long)rows,
                     tok_in_s, target_s);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

// log-sum-exp of the rows of h listed in `act` (the nodes of a prefix tree): the kernels of vd_lhood_nll without a target
int vd_lhood_lse_p(const float* h, int64_t ldh, int64_t rows, const int32_t* act, int64_t n_act, const float* W, int64_t ldw, const float* bias,
                   int V, int H, float* lse, hipStream_t s) {
  VD_CHECK_ARG(n_act >= 0 && n_act < (1L << 31) && rows >= 0 && V >= 1 && H >= 1 && ldh >= H && ldw >= H, "lhood lse: bad args");
  if (n_act == 0) return VD_OK;
  VD_CHECK_ARG(h && act && W && lse, "lhood lse: null pointer");
  if (vd_lhood_fused_fits(rows, ldh, V, ldw, H) && ((uintptr_t)h & 15) == 0 && ((uintptr_t)W & 15) == 0) {
    auto kern = lhood_lse_mfma_kernel;
    static bool attr_set = false;
    if (!attr_set) {
      VD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, LhoodCfg::LDS_BYTES));
      attr_set = true;
    }
    hipLaunchKernelGGL(kern, dim3(vd_cdiv(n_act, LhoodCfg::BN)), dim3(LhoodCfg::THREADS), LhoodCfg::LDS_BYTES, s, h, (long)ldh, act,
                       (int)n_act, W, (long)ldw, bias, V, H, lse);
    VD_LAUNCH_CHECK();
    return VD_OK;
  }
  VD_CHECK_ARG((size_t)H * 4 <= 48 * 1024, "lhood lse: H = %d too large for the row kernel", H);
  hipLaunchKernelGGL(lhood_lse_rows_kernel, dim3((unsigned)n_act), dim3(256), (size_t)H * 4, s, h, (long)ldh, act, W, (long)ldw, bias, V, H,
                     lse);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

// score of every candidate of a chunk from its edges: enode / etgt [T x rows] (node id into node_row / lse, 1-based target, 0 = no edge)
int vd_lhood_edge_sum_p(const float* h, int64_t ldh, const int32_t* node_row, const float* lse, const int32_t* enode, const int32_t* etgt, int T,
                        int64_t rows, int C, const float* W, int64_t ldw, const float* bias, int H, float* out, int64_t ldo, hipStream_t s) {
  VD_CHECK_ARG(out && T >= 0 && rows >= 0 && C >= 1 && ldo >= C && (long)T * rows < (1L << 31) && H % 4 == 0 && ldh % 4 == 0 && ldw % 4 == 0,
               "lhood edge sum: bad args");
  if (rows == 0) return VD_OK;
  VD_CHECK_ARG(T == 0 || (h && node_row && lse && enode && etgt && W), "lhood edge sum: null pointer");
  hipLaunchKernelGGL(lhood_edge_sum_kernel, dim3(vd_cdiv(rows, 4)), dim3(256), 0, s, h, (long)ldh, node_row, lse, enode, etgt, T, (long)rows, C,
                     W, (long)ldw, bias, H, out, (long)ldo);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

int vd_lhood_sum_p(const float* nll, const int32_t* act, int64_t n_act, int T, int64_t rows, int C, const int32_t* perm, float* out, int64_t ldo,
                   hipStream_t s) {
  VD_CHECK_ARG(out && T >= 0 && rows >= 0 && C >= 1 && ldo >= C && n_act >= 0 && n_act < (1L << 31) && (long)T * rows < (1L << 31),
               "vd_lhood_sum: bad args");
  VD_CHECK_ARG(n_act == 0 || (nll && act), "vd_lhood_sum: null pointer");
  if (rows == 0) return VD_OK;
  hipLaunchKernelGGL(lhood_sum_kernel, dim3(vd_cdiv(rows, 256)), dim3(256), 0, s, nll, act, (int)n_act, T, (long)rows, C, out, (long)ldo, perm);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

extern "C" {

int vd_lhood_live_rows(const int32_t* tok_in, const int32_t* target, int64_t n, int32_t* act, int32_t* work, int32_t* host_count,
                       void* stream) {
  VD_CHECK_ARG(tok_in && target && act && work && host_count && n >= 0 && n < (1L << 31), "vd_lhood_live_rows: bad args");
  *host_count = 0;
  if (n == 0) return VD_OK;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = vd_cdiv(n, 1024);
  hipLaunchKernelGGL(lhood_live_count_kernel, dim3(blocks), dim3(256), 0, s, tok_in, target, (long)n, work);
  VD_LAUNCH_CHECK();
  hipLaunchKernelGGL(lhood_live_write_kernel, dim3(blocks), dim3(256), 0, s, tok_in, target, (long)n, work, act, work + blocks);
  VD_LAUNCH_CHECK();
  VD_HIP(hipMemcpyAsync(host_count, work + blocks, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  VD_HIP(hipStreamSynchronize(s));
  return VD_OK;
}

int vd_lhood_nll(const float* h, int64_t ldh, int64_t rows, const int32_t* act, int64_t n_act, const int32_t* target, const float* W,
                 int64_t ldw, const float* bias, int V, int H, float* nll, void* stream) {
  VD_CHECK_ARG(n_act >= 0 && n_act < (1L << 31) && rows >= 0 && V >= 1 && H >= 1 && ldh >= H && ldw >= H, "vd_lhood_nll: bad args");
  if (n_act == 0) return VD_OK;
  VD_CHECK_ARG(h && act && target && W && nll, "vd_lhood_nll: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (vd_lhood_fused_fits(rows, ldh, V, ldw, H) && ((uintptr_t)h & 15) == 0 && ((uintptr_t)W & 15) == 0) {
    auto kern = lhood_nll_mfma_kernel;
    static bool attr_set = false;
    if (!attr_set) {
      VD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, LhoodCfg::LDS_BYTES));
      attr_set = true;
    }
    hipLaunchKernelGGL(kern, dim3(vd_cdiv(n_act, LhoodCfg::BN)), dim3(LhoodCfg::THREADS), LhoodCfg::LDS_BYTES, s, h, (long)ldh, act,
                       (int)n_act, target, W, (long)ldw, bias, V, H, nll);
    VD_LAUNCH_CHECK();
    return VD_OK;
  }
  VD_CHECK_ARG((size_t)H * 4 <= 48 * 1024, "vd_lhood_nll: H = %d too large for the row kernel", H);
  hipLaunchKernelGGL(lhood_nll_rows_kernel, dim3((unsigned)n_act), dim3(256), (size_t)H * 4, s, h, (long)ldh, act, target, W, (long)ldw,
                     bias, V, H, nll);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

int vd_lhood_sum(const float* nll, const int32_t* act, int64_t n_act, int T, int64_t rows, int C, float* out, int64_t ldo,
                 void* stream) {
  return vd_lhood_sum_p(nll, act, n_act, T, rows, C, nullptr, out, ldo, (hipStream_t)stream);
}

}  // extern "C"
