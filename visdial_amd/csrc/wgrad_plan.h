// Contraction plan of the encoder LSTMs' weight gradients over the LIVE rows of a length-sorted sequence set (rt_core.h SeqTok: the
// non-pad rows of step t are the prefix [0, nact[t]) of its N rows).  Host code only, no HIP type: tests/test_enc_wgrad_plan_cpu.py
// compiles it alone.
//
//   segments   one per step with a live row: the K rows a product contracts there, cut into k-steps of 16 consecutive rows (the K tile of
//              the LDS-DMA pipeline, gemm_core.h).  A k-step may take in zero-filled pad rows [nact[t], N) of the SAME step to stay whole;
//              where the step has no 16 rows left (N % 16 != 0, nact[t] close to N, or N < 16) its last k-step is SHORT: `tail` < 16 rows.
//              No k-step holds a row of another step.
//   t_first    0: the x row and the da row of the same (t, i) (dWx): segment rows t * N + [0, ..)
//              1: the pairs (h row (t - 1) * N + i, da row t * N + i), t >= 1 (dWh).  Rows are counted in the FIRST operand: the caller
//              hands the second operand in from its row N on, so both operands walk one row index
//   work list  the k-steps of every (product, output tile) laid end to end and cut into `chunks` pieces that differ by at most one
//              k-step; a chunk is one workgroup's share, an item the part of it inside one (product, tile)
#pragma once
#include <stdint.h>

#include <vector>

namespace vdplan {

constexpr int KSTEP = 16;

struct Seg {
  int32_t row;     // first row of the segment
  int32_t nks;     // k-steps: k-step j holds rows row + 16 j .. + 15 (the last one: `tail` rows)
  int32_t tail;    // rows of the last k-step, 1 .. 16
  int32_t kfirst;  // k-steps of the product in front of this segment
};

struct Item {
  int32_t product, tile;
  int32_t seg, j;   // first k-step: k-step j of segment seg of the product
  int32_t nk;       // k-steps
};

// the segments of one product, closed by a sentinel a walker never leaves ({0, 2^30, 16, total k-steps}); returns the k-steps
inline int live_segments(const int32_t* nact, int T, int N, int t_first, std::vector<Seg>* out) {
  out->clear();
  int total = 0;
  for (int t = t_first; t < T; ++t) {
    const int n = nact[t] < N ? nact[t] : N;
    if (n <= 0) continue;
    int full = (n + KSTEP - 1) / KSTEP;
    if (full > N / KSTEP) full = N / KSTEP;          // whole k-steps inside the step's N rows
    const int rest = n - full * KSTEP;               // live rows behind them (> 0 only where no 16 rows are left)
    const int nks = full + (rest > 0 ? 1 : 0);
    out->push_back(Seg{(t - t_first) * N, nks, rest > 0 ? rest : KSTEP, total});
    total += nks;
  }
  out->push_back(Seg{0, 1 << 30, KSTEP, total});
  return total;
}

struct Product {
  const Seg* segs;   // live_segments' table
  int nseg;          // without the sentinel
  int ksteps;        // its k-steps
  int tiles;         // output tiles
};

// items [chunk_start[w], chunk_start[w + 1]) are chunk w's; chunks without a k-step (more chunks than k-steps) are empty
inline void work_list(const Product* prod, int nprod, int chunks, std::vector<Item>* items, std::vector<int32_t>* chunk_start) {
  items->clear();
  chunk_start->assign(1, 0);
  long total = 0;
  for (int p = 0; p < nprod; ++p) total += (long)prod[p].ksteps * prod[p].tiles;
  if (chunks < 1) chunks = 1;
  const long q = total / chunks, r = total % chunks;   // the first r chunks hold q + 1 k-steps
  int p = 0, tile = 0, seg = 0, j = 0, k = 0;          // cursor: k-step k of (p, tile) = k-step j of segment seg
  auto skip_empty = [&]() { while (p < nprod && (prod[p].ksteps == 0 || prod[p].tiles == 0)) ++p; };
  skip_empty();
  for (int w = 0; w < chunks; ++w) {
    long left = q + (w < r ? 1 : 0);
    while (left > 0) {
      const Product& P = prod[p];
      const int nk = (int)(left < P.ksteps - k ? left : P.ksteps - k);
      items->push_back(Item{p, tile, seg, j, nk});
      left -= nk;
      k += nk;
      if (k == P.ksteps) {   // next tile of the product, or the next product
        k = seg = j = 0;
        if (++tile == P.tiles) { tile = 0; ++p; skip_empty(); }
      } else {
        int adv = nk;
        while (adv >= P.segs[seg].nks - j) { adv -= P.segs[seg].nks - j; ++seg; j = 0; }
        j += adv;
      }
    }
    chunk_start->push_back((int32_t)items->size());
  }
}

}  // namespace vdplan
