// Stand-alone check of visdial_amd/csrc/wgrad_plan.h (built and run by tests/test_enc_wgrad_plan_cpu.py with the host compiler and
// -fsanitize=address,undefined).  It walks every work list the way the kernel does (gemm_core.h gemm_block_glds_live: one table entry per
// segment, row += 16 per k-step) and counts what each (product, tile) contracts.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "wgrad_plan.h"

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd(unsigned n) {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (unsigned)((rng_state >> 11) % n);
}

#define CHECK(cond, ...)                                      \
  do {                                                        \
    if (!(cond)) {                                            \
      fprintf(stderr, "FAILED %s (line %d): ", #cond, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                           \
      fprintf(stderr, "\n");                                  \
      exit(1);                                                \
    }                                                         \
  } while (0)

// kind 0: random non-decreasing; 1: leading zeros (no row of full length); 2: drawn from the edge values {0, 1, 15, 16, 17, N}; 3: all N
static std::vector<int32_t> make_nact(int T, int N, int kind) {
  std::vector<int32_t> a(T);
  const int edge[6] = {0, 1, 15, 16, 17, N};
  for (int t = 0; t < T; ++t) {
    if (kind == 0) a[t] = (int32_t)rnd(N + 1);
    else if (kind == 1) a[t] = t < (T + 1) / 2 ? 0 : (int32_t)rnd(N + 1);
    else if (kind == 2) a[t] = std::min(edge[rnd(6)], N);
    else a[t] = N;
  }
  std::sort(a.begin(), a.end());
  return a;
}

static long check_case(int T, int N, const std::vector<int32_t>& nact, int chunks) {
  using namespace vdplan;
  std::vector<Seg> segs[2];
  int ksteps[2];
  for (int f = 0; f < 2; ++f) {
    ksteps[f] = live_segments(nact.data(), T, N, f, &segs[f]);
    CHECK(!segs[f].empty() && segs[f].back().nks == (1 << 30) && segs[f].back().kfirst == ksteps[f], "sentinel");
    int k = 0;
    for (size_t s = 0; s + 1 < segs[f].size(); ++s) {
      const Seg& g = segs[f][s];
      CHECK(g.kfirst == k && g.nks >= 1 && g.tail >= 1 && g.tail <= 16, "segment %zu", s);
      k += g.nks;
    }
    CHECK(k == ksteps[f], "k-steps %d vs %d", k, ksteps[f]);
  }
  // one flush: dWh (pairs (t - 1, t)) on 3 tiles, dWx (one step) on 2 tiles, dWh again on 1 tile
  const int first[3] = {1, 0, 1}, tiles[3] = {3, 2, 1};
  Product prod[3];
  for (int p = 0; p < 3; ++p) prod[p] = Product{segs[first[p]].data(), (int)segs[first[p]].size() - 1, ksteps[first[p]], tiles[p]};
  std::vector<Item> items;
  std::vector<int32_t> start;
  work_list(prod, 3, chunks, &items, &start);
  CHECK((int)start.size() == chunks + 1 && start[0] == 0 && start.back() == (int)items.size(), "chunk table");
  // cover[p][tile][t * N + i]: times the pair (t, i) of the da operand is contracted
  std::vector<std::vector<int>> cover(6, std::vector<int>((size_t)T * N, 0));
  const int slot0[3] = {0, 3, 5};
  long lo = 1L << 60, hi = 0, total = 0;
  for (int w = 0; w < chunks; ++w) {
    CHECK(start[w] <= start[w + 1], "chunk %d", w);
    long len = 0;
    for (int it = start[w]; it < start[w + 1]; ++it) {
      const Item& I = items[it];
      CHECK(I.product >= 0 && I.product < 3 && I.tile >= 0 && I.tile < tiles[I.product] && I.nk >= 1, "item %d", it);
      const int f = first[I.product];
      const std::vector<Seg>& tab = segs[f];
      CHECK(I.seg >= 0 && I.seg + 1 < (int)tab.size() && I.j >= 0 && I.j < tab[I.seg].nks, "item %d starts at (%d, %d)", it, I.seg, I.j);
      std::vector<int>& cv = cover[slot0[I.product] + I.tile];
      // the kernel's walker
      int seg = I.seg, j = I.j;
      Seg sg = tab[seg];
      for (int k = 0; k < I.nk; ++k) {
        const int row = sg.row + j * 16, cnt = j + 1 == sg.nks ? sg.tail : 16;
        if (++j == sg.nks) {
          CHECK(seg + 1 < (int)tab.size(), "walked off the table");
          sg = tab[++seg];
          j = 0;
        }
        // rows row .. row + 15 are READ (a short k-step re-reads its last row instead of the rows behind it), the first cnt are multiplied
        const int ta = row / N;                        // step of the first operand's rows
        const int t = ta + f;                          // step of the da rows: the second operand starts N rows on when f = 1
        CHECK(row >= 0 && t < T, "row %d", row);
        for (int r = 0; r < 16; ++r) {
          const int rr = r < cnt ? row + r : row + cnt - 1;
          CHECK(rr / N == ta, "k-step at row %d reads row %d of another step (N = %d)", row, rr, N);
        }
        for (int r = 0; r < cnt; ++r) {
          const int i = (row + r) % N;
          if (i >= nact[t]) CHECK(cnt == 16 && i < N, "pad row %d of step %d in a short k-step", i, t);   // taken in: pad rows of the same step
          const int a_row = row + r, b_row = a_row + f * N;
          CHECK(b_row == t * N + i && a_row == (t - f) * N + i, "pairing");
          ++cv[(size_t)t * N + i];
        }
      }
      len += I.nk;
    }
    lo = std::min(lo, len);
    hi = std::max(hi, len);
    total += len;
  }
  long want = 0;
  for (int p = 0; p < 3; ++p) want += (long)ksteps[first[p]] * tiles[p];
  CHECK(total == want, "k-steps %ld of %ld", total, want);
  CHECK(hi - lo <= 1, "chunks of %ld .. %ld k-steps", lo, hi);
  for (int p = 0; p < 3; ++p)
    for (int tile = 0; tile < tiles[p]; ++tile)
      for (int t = 0; t < T; ++t)
        for (int i = 0; i < N; ++i) {
          const int c = cover[slot0[p] + tile][(size_t)t * N + i];
          const bool live = t >= first[p] && i < nact[t];
          if (live) CHECK(c == 1, "product %d tile %d: live pair (%d, %d) contracted %d times", p, tile, t, i, c);
          else CHECK(c <= 1, "product %d tile %d: pad pair (%d, %d) contracted %d times", p, tile, t, i, c);
          if (t < first[p]) CHECK(c == 0, "product %d: step %d has no previous step", p, t);
        }
  return total;
}

int main() {
  const int Ns[6] = {1, 15, 16, 17, 40, 200}, Ts[4] = {1, 2, 7, 40}, Cs[4] = {1, 5, 64, 768};
  long cases = 0, ksteps = 0;
  for (int N : Ns)
    for (int T : Ts)
      for (int kind = 0; kind < 4; ++kind)
        for (int rep = 0; rep < (kind < 3 ? 3 : 1); ++rep) {
          const std::vector<int32_t> nact = make_nact(T, N, kind);
          for (int chunks : Cs) {
            ksteps += check_case(T, N, nact, chunks);
            ++cases;
          }
        }
  printf("OK %ld cases, %ld k-steps\n", cases, ksteps);
  return 0;
}
