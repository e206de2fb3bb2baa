// split_core.h -- exact-operand bf16 split of an fp32 GEMM for the option recurrence (opt-in, `lstmPrecision = split9`).
//
// fp32 MFMA (v_mfma_f32_32x32x2_f32) runs at 1/16 of the bf16 rate.  An fp32 value is the exact sum of three bf16 values
// (hi = RNE(v), mid = RNE(v - hi), lo = RNE(v - hi - mid): 3 x 8 significand bits + signs cover the 24), the product of two
// bf16 values is exact in fp32, so  A * B = sum_{i,j in {hi,mid,lo}} A_i * B_j  -- nine bf16 MFMAs (v_mfma_f32_32x32x16_bf16,
// fp32 accumulation) per fp32 one, 9/16 of the matrix-pipe time, every product exact.  NPROD selects the products that are
// issued: 9 = all (fp32-grade), 6 = those with i + j <= 2 (drops terms below 2^-24 of the largest), 3 = i + j <= 1, 1 = plain
// bf16.  Only 9 is a substitute for fp32; the others exist for the error table (tests/test_ops_gpu.py).
//
// Operands: A [M x K] fp32 rows exactly as the fp32 kernels read them -- the activations stay fp32 in memory, a wave splits its
// fragments into three bf16 planes IN REGISTERS -- and B as three precomputed bf16 planes Bt_p [N x K] (k contiguous; the recurrent
// weights, converted once per pass).
//
// Step kernels (gemm_split_kernel): v_mfma_f32_16x16x32_bf16.  The two bf16 shapes have the same peak (1024 FLOP per cycle and SIMD), but
// this chip holds a higher clock on the 16x16x32 one under load: +10 % by wall in a register-only loop on random operands, equal on
// zeros (scripts/probes/mfma_bf16_peak.hip, profiles/mfma_shape.txt).  A wave still owns 32 rows x 128 columns: 2 x 8 accumulators of
// 16 x 16, 64 registers, all in VGPRs (in AGPRs the short instruction loses 1 to 2.5 cycles: the probe's first build).  One macro step =
// 32 k = one MFMA's depth; K = 16 (mod 32) ends on a half step whose upper k half multiplies zeros.
//   A: each wave reads only its own 32 rows, so they go global -> registers, one macro step ahead: lane l holds k = 8 (l >> 4) .. + 7 of rows
//      l & 15 and 16 + (l & 15), 2 x 32 contiguous bytes; the four lanes of a row fetch one 128-byte line.
//   B: three planes [128 x 32] bf16 by LDS-DMA, 64-byte rows, 24 KB per stage, two stages = 48 KB; chunk swizzle split_swz (below):
//      ds_read_b128 conflict-free.  Per plane the eight fragments are read once, four at a time (16 registers), and multiplied with the
//      three A planes of both row halves, column tile innermost: consecutive MFMAs never share an accumulator.
//   Workgroup: four waves (128 x 128), three per CU -- 3 x 48 KB = 144 KB of LDS.  The suggested six-wave workgroup (192 rows, two per CU,
//      96 KB) keeps the same 12 waves per CU but measured SLOWER than the 32x32x16 kernel (434 / 498 us per forward / backward launch in
//      the step against 374 / 437): with two workgroups per CU the epilogue of one (gates, c, h, the projection-table gather) has only one
//      other workgroup's MFMAs to hide under.  With three, 341 / 423 us, and the step's side streams still run beside it (profiles/mfma_shape.txt).
//   Epilogues take 32 x 32 tiles in the 32x32 layout: each 2 x 2 quad of 16 x 16 results passes the wave's scratch once (gemm_core.h quad_to_tile).
//
// What bounds it (profiles/r05_experiments.txt section 1): POWER.  On non-zero operands the clock falls to ~1.75-1.9 GHz on 32x32x16 and to
// ~2.05-2.15 GHz on 16x16x32; the same K loop ran 299 us on random operands and 206 us on zeros on the old shape (same code, same cycles).
// The weight-gradient contraction below (gemm_split_tn_kernel) stays on v_mfma_f32_32x32x16_bf16.
#pragma once
#include "gemm_core.h"
#include "paths.h"

typedef __bf16 vd_bf16x8 __attribute__((ext_vector_type(8)));

// The split's four operations as ONE vector instruction each.  Written out in C++ the compiler SLP-packs neighbouring subtractions into
// v_pk_add_f32 (which costs more beside MFMAs than the two v_sub_f32 it replaces), converts some values singly and re-packs them, and
// copies registers in between; here a pair of values costs 3 conversions, 4 unpacks and 4 subtractions, 5.5 instructions per value
// (scripts/loop_isa.py, profiles/split_loop_isa.txt).  The conversion is the instruction the compiler chooses too: RNE, bf16(a) low.
__device__ __forceinline__ unsigned vd_cvt_pk_bf16(float a, float b) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float vd_bf16_lo_f32(unsigned p) {    // the low bf16 of a pair as fp32
  float r;
  asm("v_lshlrev_b32 %0, 16, %1" : "=v"(r) : "v"(p));
  return r;
}
__device__ __forceinline__ float vd_bf16_hi_f32(unsigned p) {    // the high one
  float r;
  asm("v_and_b32 %0, 0xffff0000, %1" : "=v"(r) : "v"(p));
  return r;
}
__device__ __forceinline__ float vd_sub_f32(float a, float b) {
  float r;
  asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// two values -> their packed hi / mid / lo: hi = RNE(v), mid = RNE(v - hi), lo = RNE(v - hi - mid); both subtractions are exact
__device__ __forceinline__ void vd_split3_pair(float a, float b, unsigned& hi, unsigned& mid, unsigned& lo) {
  hi = vd_cvt_pk_bf16(a, b);
  const float ra = vd_sub_f32(a, vd_bf16_lo_f32(hi)), rb = vd_sub_f32(b, vd_bf16_hi_f32(hi));
  mid = vd_cvt_pk_bf16(ra, rb);
  lo = vd_cvt_pk_bf16(vd_sub_f32(ra, vd_bf16_lo_f32(mid)), vd_sub_f32(rb, vd_bf16_hi_f32(mid)));
}

typedef unsigned vd_u32x4 __attribute__((ext_vector_type(4)));
// v (8 consecutive k of one row) -> hi / mid / lo planes
__device__ __forceinline__ void vd_split3(const float4& u, const float4& w, vd_bf16x8& hi, vd_bf16x8& mid, vd_bf16x8& lo) {
  unsigned h[4], m[4], l[4];
  vd_split3_pair(u.x, u.y, h[0], m[0], l[0]);
  vd_split3_pair(u.z, u.w, h[1], m[1], l[1]);
  vd_split3_pair(w.x, w.y, h[2], m[2], l[2]);
  vd_split3_pair(w.z, w.w, h[3], m[3], l[3]);
  hi = __builtin_bit_cast(vd_bf16x8, (vd_u32x4){h[0], h[1], h[2], h[3]});
  mid = __builtin_bit_cast(vd_bf16x8, (vd_u32x4){m[0], m[1], m[2], m[3]});
  lo = __builtin_bit_cast(vd_bf16x8, (vd_u32x4){l[0], l[1], l[2], l[3]});
}

// fp32 matrix -> three bf16 planes (dst + p * plane), same element order
static __global__ void __launch_bounds__(256) f32_to_bf16x3_kernel(const float* __restrict__ src, vd_bf16_bits* __restrict__ dst, long n4, long plane) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 v = reinterpret_cast<const float4*>(src)[i];
  float4 r1, r2;
  typedef __bf16 bf4 __attribute__((ext_vector_type(4)));
  const bf4 h = {(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
  r1.x = v.x - (float)h[0]; r1.y = v.y - (float)h[1]; r1.z = v.z - (float)h[2]; r1.w = v.w - (float)h[3];
  const bf4 m = {(__bf16)r1.x, (__bf16)r1.y, (__bf16)r1.z, (__bf16)r1.w};
  r2.x = r1.x - (float)m[0]; r2.y = r1.y - (float)m[1]; r2.z = r1.z - (float)m[2]; r2.w = r1.w - (float)m[3];
  const bf4 l = {(__bf16)r2.x, (__bf16)r2.y, (__bf16)r2.z, (__bf16)r2.w};
  *reinterpret_cast<bf4*>(dst + i * 4) = h;
  *reinterpret_cast<bf4*>(dst + plane + i * 4) = m;
  *reinterpret_cast<bf4*>(dst + 2 * plane + i * 4) = l;
}
static int weights_to_bf16x3(const float* src, vd_bf16_bits* dst, long n, hipStream_t s) {
  hipLaunchKernelGGL(f32_to_bf16x3_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, src, dst, n / 4, n);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

// The dynamic-LDS limit of a kernel is an attribute of the kernel ON ONE DEVICE: it is raised once per device ordinal, not once per process
// (past the table, on every launch).
constexpr int SPLIT_ATTR_DEVS = 64;
static int split_lds_attr(const void* kern, bool (&done)[SPLIT_ATTR_DEVS]) {
  int dev = 0;
  VD_HIP(hipGetDevice(&dev));
  if (dev >= 0 && dev < SPLIT_ATTR_DEVS && done[dev]) return VD_OK;
  VD_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  if (dev >= 0 && dev < SPLIT_ATTR_DEVS) done[dev] = true;
  return VD_OK;
}

struct SplitCfg {
    static constexpr int NT = 4, WM = 4, THREADS = 64 * WM;
  static constexpr int BM = 32 * WM, BN = 128, KS = 32;           // four waves of 32 rows x 128 columns; one macro step = 32 k
  static constexpr int BTILE = BN * 64;                           // [BN rows][32 bf16]      = 64-byte rows, one per plane
  static constexpr int STAGE = 3 * BTILE;                         // 24 KB: the B planes only (A goes global -> registers)
  static constexpr int LDS_BYTES = 2 * STAGE;                     // 48 KB, three workgroups per CU (the registers allow no more)
  static constexpr int SCR = LDS_BYTES / WM / 4;                     // floats of epilogue scratch per wave (3072 >= 32 x QUAD_LD)
  static_assert(SCR >= 32 * QUAD_LD, "quad_to_tile's 32 rows of QUAD_LD floats");
};

// workgroup id -> tile.  Block b runs on XCD b % 8 (round-robin dispatch), so the map decides which operand bytes each XCD's private L2
// sees.  When the column tiles divide over VD_SPLIT_CG column groups, the 8 XCDs form a CG x (8 / CG) grid: an XCD owns the weight planes
// of tiles_n / CG column tiles (resident in its 4 MB L2) and walks 1 / (8 / CG) of the row tiles, column tile fastest (a row tile's A rows
// are fetched once per XCD that needs them and shared by its column tiles through L2).  CG = 8 (round 5): smallest weight slice, but every
// XCD fetches ALL of A -- 8 x 41 MB per forward launch, the 1.6 x over-fetch of profiles/r05_pmc_option_lstm_kernels.txt; CG = 2: A is
// fetched twice, 3 MB of planes per XCD.  Else XCD-contiguous ranges with the column tile fastest (the backward step: 4 column tiles).
// The grid is padded to 8 x rows-per-group x columns-per-group workgroups; a workgroup whose row tile is past the end leaves at once.
#ifndef VD_SPLIT_CG
#define VD_SPLIT_CG 2
#endif
static_assert(VD_SPLIT_CG >= 1 && VD_SPLIT_CG <= 8 && 8 % VD_SPLIT_CG == 0, "the XCD grid is VD_SPLIT_CG x (8 / VD_SPLIT_CG)");
__device__ __forceinline__ bool split_tile_of(int bid, int nwg, int tiles_m, int tiles_n, int& tile_m, int& tile_n) {
  constexpr int CG = VD_SPLIT_CG, RG = 8 / CG;
  if ((tiles_n % CG) == 0 && tiles_n >= 8) {
    const int xcd = bid & 7, li = bid >> 3, cpg = tiles_n / CG, rpg = (tiles_m + RG - 1) / RG;
    tile_n = (xcd % CG) * cpg + li % cpg;
    tile_m = (xcd / CG) * rpg + li / cpg;
    return tile_m < tiles_m && li / cpg < rpg;
  }
  const int wg = xcd_remap(bid, nwg);
  tile_n = wg % tiles_n;
  tile_m = wg / tiles_n;
  return true;
}
// chunk swizzle of the 64-byte B rows: row group q = (row >> 2) & 3 stores k chunk c at c ^ {0, 2, 3, 1}[q].  A B fragment read (lane l: row
// l & 15, chunk l >> 4) then puts the 16 lanes of each ds_read_b128 group -- {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 -- on
// 16 different 16-byte bank groups: rows q = 0, 3 of one chunk with rows q = 1, 2 of its neighbour, {s0, s3, 1 ^ s1, 1 ^ s2} all different.
__device__ __forceinline__ int split_swz(int q) { return (0x78 >> (2 * (q & 3))) & 3; }
static int split_grid(int tiles_m, int tiles_n) {
  constexpr int CG = VD_SPLIT_CG, RG = 8 / CG;
  if ((tiles_n % CG) == 0 && tiles_n >= 8) return 8 * ((tiles_m + RG - 1) / RG) * (tiles_n / CG);
  return tiles_m * tiles_n;
}

template <int NPROD, class Epi>
__global__ void __launch_bounds__(SplitCfg::THREADS, 3)
gemm_split_kernel(int M, int N, int K, int tiles_n, const float* A, long lda, const vd_bf16_bits* B, long ldb, long bplane, Epi epi) {
  using Cfg = SplitCfg;
  constexpr int NT = Cfg::NT;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int tile_m, tile_n;
  if (!split_tile_of((int)blockIdx.x, (int)gridDim.x, (M + Cfg::BM - 1) / Cfg::BM, tiles_n, tile_m, tile_n)) return;
  const int row_base = tile_m * Cfg::BM, col_base = tile_n * Cfg::BN;
  constexpr int NIB = 24 / Cfg::WM;                                       // 24 pieces of 16 rows x 64 bytes per stage, six per wave
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wm = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nfull = K / 32, nm = nfull + ((K >> 4) & 1);         // macro steps; the last one is a half step when K = 16 (mod 32)
  const int wrow = row_base + wm * 32;                           // first row of this wave
  const int g = lane >> 4, l15 = lane & 15;                      // MFMA operand lane: row / column l15, k = 8 g .. 8 g + 7

  vd_f32x4 acc[2][2 * NT];                                       // [16-row half][16-column tile]
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int j = 0; j < 2 * NT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[rt][j][r] = 0.f;

  typename EpiPreOf<Epi>::type pre;
  if constexpr (EpiPreOf<Epi>::value) epi.preload(pre, wrow, lane, M);

  // A: the lane's own 8 k of rows l15 and 16 + l15 of this wave, 32 bytes each, straight into registers one macro step ahead (the four
  // lanes of a row fetch one whole 128-byte line).  In a half step the lanes of the upper k half load nothing and multiply zeros.
  unsigned aoff[2];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) aoff[rt] = (unsigned)(((long)min(wrow + rt * 16 + l15, M - 1) * lda + g * 8) * 4);
  float4 an[2][2];
  auto load_a = [&](int m) {
    const char* ak = reinterpret_cast<const char*>(A + (long)m * 32);
    const bool live = m < nfull || g < 2;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      an[rt][0] = an[rt][1] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (live) {
        an[rt][0] = *reinterpret_cast<const float4*>(ak + aoff[rt]);
        an[rt][1] = *reinterpret_cast<const float4*>(ak + aoff[rt] + 16);
      }
    }
  };
  // B: per-thread source byte offsets of this wave's DMA instructions; the DMA writes lane-linear (row lane >> 2, chunk lane & 3 of the
  // piece), the chunk index is swizzled on the source side by split_swz(row >> 2).  In a half step the chunks of the upper k half fetch
  // the lower half again (finite values that meet the zeros of A): nothing is read past k = K.
  const int csrc = (lane & 3) ^ split_swz(lane >> 4);            // (row >> 2) & 3 = lane >> 4: a piece starts on a multiple of 16 rows
  unsigned voffb[NIB];
#pragma unroll
  for (int i = 0; i < NIB; ++i) {
    const int r = ((wm * NIB + i) & 7) * 16 + (lane >> 2);
    voffb[i] = (unsigned)(((long)min(col_base + r, N - 1) * ldb + csrc * 8) * 2);
  }
  const unsigned lds0 = (unsigned)(uintptr_t)smem;
  auto issue_b = [&](int m, int st) {
    const unsigned back = m < nfull ? 0u : (unsigned)(csrc >> 1) * 32u;
#pragma unroll
    for (int i = 0; i < NIB; ++i) {
      const int q = wm * NIB + i;                                // piece q: plane q >> 3, rows (q & 7) * 16 .. + 15
      glds16(voffb[i] - back, reinterpret_cast<const float*>(B + (long)(q >> 3) * bplane + (long)m * 32), lds0 + st * Cfg::STAGE + q * 1024);
    }
  };
  const int bfrag = l15 * 64 + ((g ^ split_swz(l15 >> 2)) * 16);  // this lane's 8 bf16 k of column l15 of a 16-column tile

  // the same when macro step m is known to be a full one: no predicate, no zero fill, no source offset
  auto load_a_full = [&](int m) {
    const char* ak = reinterpret_cast<const char*>(A + (long)m * 32);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      an[rt][0] = *reinterpret_cast<const float4*>(ak + aoff[rt]);
      an[rt][1] = *reinterpret_cast<const float4*>(ak + aoff[rt] + 16);
    }
  };
  auto issue_b_full = [&](int m, int st) {
#pragma unroll
    for (int i = 0; i < NIB; ++i) {
      const int q = wm * NIB + i;
      glds16(voffb[i], reinterpret_cast<const float*>(B + (long)(q >> 3) * bplane + (long)m * 32), lds0 + st * Cfg::STAGE + q * 1024);
    }
  };

  // one macro step on stage st; full_next: step m + 1 exists and is a full one
  auto step = [&](int m, int st, auto full_next) {
    vd_bf16x8 ap[2][3];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) vd_split3(an[rt][0], an[rt][1], ap[rt][0], ap[rt][1], ap[rt][2]);
    __builtin_amdgcn_sched_barrier(0);                         // the split in front of the barrier, not behind it
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");                    // every wave's share of macro step m has landed
    if constexpr (decltype(full_next)::value) {                // step m + 1 flies under the 144 MFMAs of step m
      issue_b_full(m + 1, st ^ 1);
      load_a_full(m + 1);
    } else if (m + 1 < nm) {
      issue_b(m + 1, st ^ 1);
      load_a(m + 1);
    }
    // the loads stay HERE, in front of the MFMAs they fly under (the split above has freed their registers; left free, the scheduler
    // sinks them to the end of the step to save registers and the next step's split waits for them with nothing in between)
    __builtin_amdgcn_sched_barrier(0);
    const char* sbase = reinterpret_cast<const char*>(smem) + st * Cfg::STAGE + bfrag;
    // plane p of B against planes i of A, smallest terms first; column tile innermost: consecutive MFMAs never share an accumulator
#pragma unroll
    for (int p = 2; p >= 0; --p)
#pragma unroll
      for (int jh = 0; jh < 2; ++jh) {                         // four column tiles at a time: 16 fragment registers, not 32
        vd_bf16x8 bp[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const vd_f32x4 t = *reinterpret_cast<const vd_f32x4*>(sbase + p * Cfg::BTILE + (jh * NT + j) * 1024);
          bp[j] = __builtin_bit_cast(vd_bf16x8, t);
        }
#pragma unroll
        for (int i = 2; i >= 0; --i) {
          constexpr int LIM = NPROD >= 9 ? 4 : NPROD >= 6 ? 2 : NPROD >= 3 ? 1 : 0;     // products with i + p <= LIM are issued
          if (i + p > LIM) continue;
#pragma unroll
          for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int j = 0; j < NT; ++j)
              acc[rt][jh * NT + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap[rt][i], bp[j], acc[rt][jh * NT + j], 0, 0, 0);
        }
      }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // stage `st` may be refilled
  };
  if (nm > 0) {
    issue_b(0, 0);
    load_a(0);
    // The main loop runs the full steps that a full step follows: unconditional loads, nothing but the split between the MFMAs.  Peeled
    // behind it: the last full step (which may prefetch the half step) and the half step itself, K = 16 (mod 32), with the predicated loads.
    int m = 0;
    for (; m + 1 < nfull; ++m) step(m, m & 1, std::true_type{});
    if (m < nm) {
      step(m, m & 1, std::false_type{});
      if (++m < nm) step(m, m & 1, std::false_type{});
    }
  }
  // the epilogues take 32 x 32 tiles in the layout of the 32x32 MFMAs: each 2 x 2 quad of 16 x 16 results goes through the wave's scratch once
  float* scr = smem + wm * Cfg::SCR;
  f32x16 tile[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) tile[j] = quad_to_tile(acc[0][2 * j], acc[0][2 * j + 1], acc[1][2 * j], acc[1][2 * j + 1], scr, lane);
  if constexpr (EpiPreOf<Epi>::value) epi(tile, wrow, col_base, lane, M, N, scr, &pre);
  else epi(tile, wrow, col_base, lane, M, N, scr);
}

// C[M x N] = epi(A[M x K] (fp32 rows) * Bt[N x K]^T), Bt given as three bf16 planes; K % 16 == 0
template <int NPROD, class Epi>
static int launch_gemm_split(int M, int N, int K, const float* A, long lda, const vd_bf16_bits* B, long ldb, long bplane, const Epi& e,
                             hipStream_t stream) {
  if (M <= 0 || N <= 0) return VD_OK;
  using Cfg = SplitCfg;
  VD_CHECK_ARG(K % 16 == 0 && lda % 4 == 0 && ldb % 8 == 0 && (long)M * lda * 4 < (1L << 32) && (long)N * ldb * 2 < (1L << 32),
               "launch_gemm_split: unsupported shape M=%d N=%d K=%d", M, N, K);
  const int tiles_m = vd_cdiv(M, Cfg::BM), tiles_n = vd_cdiv(N, Cfg::BN);
  auto kern = gemm_split_kernel<NPROD, Epi>;
  static bool attr_set[SPLIT_ATTR_DEVS] = {};
  if (const int rc = split_lds_attr(reinterpret_cast<const void*>(kern), attr_set)) return rc;
  hipLaunchKernelGGL(kern, dim3(split_grid(tiles_m, tiles_n)), dim3(Cfg::THREADS), Cfg::LDS_BYTES, stream, M, N, K, tiles_n, A, lda, B, ldb, bplane, e);
  VD_LAUNCH_CHECK();
  return VD_OK;
}

// the same with the product count of the pass chosen at run time (paths.h vd_split_nprod: 9, 6 or 3)
template <class Epi>
static int launch_gemm_split(int nprod, int M, int N, int K, const float* A, long lda, const vd_bf16_bits* B, long ldb, long bplane,
                             const Epi& e, hipStream_t stream) {
  if (nprod == 9) return launch_gemm_split<9>(M, N, K, A, lda, B, ldb, bplane, e, stream);
  if (nprod == 6) return launch_gemm_split<6>(M, N, K, A, lda, B, ldb, bplane, e, stream);
  return launch_gemm_split<3>(M, N, K, A, lda, B, ldb, bplane, e, stream);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The same exact split for the weight-gradient contraction  C[M x N] += A[K x M]^T * B[K x N]  (dWh = h^T * da over all
// (timestep, row) pairs: K = 380 000 at the headline shape).  Both operands are fp32 rows contracted over their ROW index, so
// NEITHER can be converted ahead of time without another pass over 4 GB: tiles go global -> LDS by DMA as fp32, A as [16 k][256 m]
// (k-major, dense: a row of the tile is a row segment of the operand), B as four column tiles [16 k][32 n].  A wave owns 64 m x 128 n
// (8 accumulator tiles).  Its A rows are its own: it reads the fragments with ds_read_b32 (lane = one m, 8 consecutive k: conflict-free,
// lanes 0-31 walk one k row) and splits them in registers.  The B tile is shared by the four waves and is split ONCE per workgroup: wave
// w splits column tile w and leaves the three planes in LDS as MFMA fragments, every wave reads them with ds_read_b128 -- 16 + 8 split
// values per wave and 72 MFMAs where a split per wave took 16 + 32 (profiles/dwh_coop_split.txt).  Split-K over the rows with
// float atomics at the end; the splits of one K range run on ONE XCD (block b runs on XCD b % 8), so the 16 column tiles that
// read the same h rows and the 2 row tiles that read the same da rows share them through that XCD's L2.
// ---------------------------------------------------------------------------------------------------------------------------
struct SplitTnCfg {
  static constexpr int BM = 256, BN = 128, THREADS = 256;
  static constexpr int ATILE = 16 * BM * 4;                       // [16 k][256 m] fp32
  static constexpr int BQUART = 16 * 32 * 4;                      // [16 k][32 n] fp32: one column tile of B, what one wave splits
  // the same column tile as MFMA fragments, [plane][lane] 16 bytes, is written over the fp32 quarter: a block holds the larger of the two
  static constexpr int nplanes(int nprod) { return nprod >= 6 ? 3 : nprod >= 3 ? 2 : 1; }   // planes of B that an issued product reads
  static constexpr int bblock(int nprod) { return nplanes(nprod) * 1024 > BQUART ? nplanes(nprod) * 1024 : BQUART; }
  static constexpr int stage(int nprod) { return ATILE + 4 * bblock(nprod); }               // 28 KB (24 KB below six products)
  static constexpr int lds_bytes(int nprod) { return 2 * stage(nprod); }
  static constexpr int LDS_BYTES = 2 * (ATILE + 4 * 3 * 1024);    // 56 KB = lds_bytes(9): two workgroups per CU (the registers allow no more)
  static constexpr int SIDE_LDS = 41 * 1024;                      // the table-gradient chain / grouped weight gradients beside it
};
static_assert(SplitTnCfg::BM == VD_SPLIT_TN_BM && SplitTnCfg::BN == VD_SPLIT_TN_BN, "paths.h vd_tn_split_tiles");
// two of these and one 41 KB side-lane workgroup share a CU's 160 KB: 2 x 56 + 41 = 153.  At 60 KB (a plane buffer beside the fp32 tile)
// the side lane is locked out and the step loses what the contraction gains (profiles/r06_experiments.txt section 5c).
static_assert(SplitTnCfg::LDS_BYTES == SplitTnCfg::lds_bytes(9) && SplitTnCfg::lds_bytes(1) == 48 * 1024, "nine products: 56 KB; one: 48 KB");
static_assert(2 * SplitTnCfg::LDS_BYTES + SplitTnCfg::SIDE_LDS <= 160 * 1024, "the side lane's workgroups must fit beside two of these");

template <int NPROD>
__global__ void __launch_bounds__(256, 2)
gemm_split_tn_kernel(int M, int N, int kchunk, int K, int tiles, int tiles_n, int splits, const float* A, long lda, const float* B, long ldb,
                     float* C, long ldc) {
  using Cfg = SplitTnCfg;
  constexpr int NPL = Cfg::nplanes(NPROD), BBLK = Cfg::bblock(NPROD), STAGE = Cfg::stage(NPROD);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  // tile / K-range of this workgroup: XCD x takes the K ranges [x * spx, (x + 1) * spx) (spx = splits / 8) and all tiles of each
  int tile, split;
  if ((splits & 7) == 0) {
    const int xcd = (int)blockIdx.x & 7, li = (int)blockIdx.x >> 3;
    split = xcd * (splits >> 3) + li / tiles;
    tile = li % tiles;
  } else {
    split = (int)blockIdx.x / tiles;
    tile = (int)blockIdx.x % tiles;
  }
  const int m_base = (tile / tiles_n) * Cfg::BM, n_base = (tile % tiles_n) * Cfg::BN;
  const int ks = split * kchunk, ke = min(K, ks + kchunk);
  const int nm = ke > ks ? (ke - ks) / 16 : 0;
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wm = __builtin_amdgcn_readfirstlane(tid >> 6);

  f32x16 acc[2][4];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mb][j][r] = 0.f;

  // DMA: A rows are 1 KB (one instruction per k row: 4 per wave).  B lands as four column tiles [j][16 k][32 n], each at the head of its
  // 3 KB block; wave w fetches column tile w, the one it splits: 8 k rows of 128 bytes per instruction (lane: k row lane >> 3, 16-byte
  // chunk lane & 7; the eight lanes of a k row fetch one 128-byte line), 2 per wave
  unsigned voffa[4], voffb[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) voffa[i] = (unsigned)(((long)(wm * 4 + i) * lda + m_base + lane * 4) * 4);
#pragma unroll
  for (int i = 0; i < 2; ++i) voffb[i] = (unsigned)(((long)(i * 8 + (lane >> 3)) * ldb + n_base + wm * 32 + (lane & 7) * 4) * 4);
  const unsigned lds0 = (unsigned)(uintptr_t)smem;
  auto issue = [&](int m, int st) {
    const unsigned base = lds0 + st * STAGE;
    const float* ak = A + (long)(ks + m * 16) * lda;
    const float* bk = B + (long)(ks + m * 16) * ldb;
#pragma unroll
    for (int i = 0; i < 2; ++i) glds16(voffb[i], bk, base + Cfg::ATILE + wm * BBLK + i * 1024);
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16(voffa[i], ak, base + (wm * 4 + i) * 1024);
  };
  const int hi = lane >> 5, l31 = lane & 31;

  // the second 32-row block of A gets a base of its own, opaque to the compiler, which then pairs the k rows of one block into
  // ds_read2st64_b32 with immediate offsets; given one base it pairs the two blocks of a k row and spends a register or an add per k row
  int mb1 = 32;
  asm("" : "+v"(mb1));
  const float* sA0 = smem + (hi * 8) * Cfg::BM + wm * 64 + l31;
  const float* sA1 = sA0 + mb1;
  const float* sBq = smem + (Cfg::ATILE + wm * BBLK) / 4 + (hi * 8) * 32 + l31;            // this wave's column tile, fp32
  const char* sBp = reinterpret_cast<const char*>(smem) + Cfg::ATILE + lane * 16;          // the planes: + j * BBLK + plane * 1024
  constexpr int LIM = NPROD >= 9 ? 4 : NPROD >= 6 ? 2 : NPROD >= 3 ? 1 : 0;                // products with pa + pb <= LIM are issued
  // The B tile is shared by the four waves, so it is split ONCE per workgroup: wave w fetches column tile w itself, reads it (lane = one n,
  // 8 consecutive k) behind its own vmcnt, splits it and stores the planes as MFMA fragments, [plane][lane] 16 bytes, over the block whose
  // first 2 KB it has just read -- no other wave reads that fp32 quarter or writes that block, so the wave's own program order guards it.
  auto read_own = [&](int st, float4& u, float4& w) {
    const float* p = sBq + st * (STAGE / 4);
    u = make_float4(p[0], p[32], p[2 * 32], p[3 * 32]);
    w = make_float4(p[4 * 32], p[5 * 32], p[6 * 32], p[7 * 32]);
  };
  auto write_own = [&](int st, const float4& u, const float4& w) {
    vd_bf16x8 own[3];
    vd_split3(u, w, own[0], own[1], own[2]);
    char* d = const_cast<char*>(sBp) + st * STAGE + wm * BBLK;
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) *reinterpret_cast<vd_bf16x8*>(d + pl * 1024) = own[pl];
  };
  // One 16-k step on stage st -- in the main loop a compile-time constant: every LDS address of the step is then a lane register plus an
  // immediate; the last step of a K range takes it at run time.  A step is entered behind ONE barrier, in front of which every wave has
  // waited for its DMA share of this step (vmcnt), for its reads of the other stage and for its plane stores of this step (lgkmcnt): the
  // other stage may be refilled at once, A and the planes of this stage may be read.  Every wave reads the planes of all four column
  // tiles, 3 ds_read_b128 per tile in place of 8 ds_read_b32 and a split: those of tile j + 1 under the 18 MFMAs of tile j.  Under the
  // MFMAs of the LAST tile the wave splits its column tile of the NEXT step, whose two DMA instructions it issued first at the top of
  // this step (vmcnt(4): the four of A may still fly), and stores the planes into the other stage: the split of B has left the front of
  // the step, and the step's one barrier publishes it.  In front of the MFMAs stands the split of the wave's first A block only, while
  // the first planes are on their way; the second block is split between the first tile's MFMAs.
  // Planes, products and their order per accumulator are those of a per-wave split, so a workgroup's sum is bit for bit the same.
  // Measured (profiles/dwh_coop_split.txt): the split behind the step's first barrier with a barrier of its own to publish it, as the
  // per-wave kernel's pipeline suggests, 5.44 -> 5.31 ms alone; this schedule 5.82 -> 5.31 ms on a slower box.
  // (Measured and dropped on the per-wave split: three LDS stages with the NEXT step's first conversions under the last column tile's
  //  MFMAs -- 5.82 ms; largest products first so that a step's first MFMAs need only the hi planes -- 5.68 vs 5.61 ms.)
  auto step = [&](int m, auto stage, auto has_next) {
    const int st = stage, other = st ^ 1;
    constexpr bool next = decltype(has_next)::value;
    if constexpr (next) issue(m + 1, st ^ 1);
    vd_bf16x8 ap[2][3], bp[2][3];
    float4 au[2], aw[2], u, w;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      const float* q = (mb ? sA1 : sA0) + st * (STAGE / 4);
      au[mb] = make_float4(q[0], q[Cfg::BM], q[2 * Cfg::BM], q[3 * Cfg::BM]);
      aw[mb] = make_float4(q[4 * Cfg::BM], q[5 * Cfg::BM], q[6 * Cfg::BM], q[7 * Cfg::BM]);
    }
    const char* sP = sBp + st * STAGE;
    auto load_b = [&](int j, vd_bf16x8 (&dst)[3]) {
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) dst[pl] = *reinterpret_cast<const vd_bf16x8*>(sP + j * BBLK + pl * 1024);
    };
    load_b(0, bp[0]);
    __builtin_amdgcn_sched_barrier(0);                            // all the reads are in flight before the first conversion waits
    vd_split3(au[0], aw[0], ap[0][0], ap[0][1], ap[0][2]);
    // column tile 0: the products of the first A block first, the second block's split between them, pair by pair (an accumulator still
    // receives its products in the same order; a chain on one accumulator costs this MFMA nothing)
    __builtin_amdgcn_sched_barrier(0);
    {
      unsigned h[4], md[4], lo[4];
      auto pair = [&](int i) {
        vd_split3_pair(i == 0 ? au[1].x : i == 1 ? au[1].z : i == 2 ? aw[1].x : aw[1].z, i == 0 ? au[1].y : i == 1 ? au[1].w : i == 2 ? aw[1].y : aw[1].w,
                       h[i], md[i], lo[i]);
      };
      int idx = 0;
#pragma unroll
      for (int pb = 2; pb >= 0; --pb)
#pragma unroll
        for (int pa = 2; pa >= 0; --pa) {
          if (pa + pb > LIM) continue;
          acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[0][pa], bp[0][pb], acc[0][0], 0, 0, 0);
          if (idx < 4) {
            __builtin_amdgcn_sched_barrier(0);
            pair(idx);
            if (idx == 3) load_b(1, bp[1]);                       // (behind the last pair: its registers are free by now)
            __builtin_amdgcn_sched_barrier(0);
          }
          ++idx;
        }
#pragma unroll
      for (int i = idx; i < 4; ++i) pair(i);
      if (idx < 4) load_b(1, bp[1]);
      ap[1][0] = __builtin_bit_cast(vd_bf16x8, (vd_u32x4){h[0], h[1], h[2], h[3]});
      ap[1][1] = __builtin_bit_cast(vd_bf16x8, (vd_u32x4){md[0], md[1], md[2], md[3]});
      ap[1][2] = __builtin_bit_cast(vd_bf16x8, (vd_u32x4){lo[0], lo[1], lo[2], lo[3]});
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int pb = 2; pb >= 0; --pb)
#pragma unroll
        for (int pa = 2; pa >= 0; --pa) {
          if (pa + pb > LIM) continue;
          acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[1][pa], bp[0][pb], acc[1][0], 0, 0, 0);
        }
    }
#pragma unroll
    for (int j = 1; j < 4; ++j) {
      __builtin_amdgcn_sched_barrier(0);
      if (j + 1 < 4) {
        load_b(j + 1, bp[(j + 1) & 1]);
      } else if constexpr (next) {
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");          // this wave's column tile of step m + 1 has landed
        read_own(other, u, w);
      }
#pragma unroll
      for (int pb = 2; pb >= 0; --pb)
#pragma unroll
        for (int pa = 2; pa >= 0; --pa) {
          if (pa + pb > LIM) continue;
#pragma unroll
          for (int mb = 0; mb < 2; ++mb) acc[mb][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[mb][pa], bp[j & 1][pb], acc[mb][j], 0, 0, 0);
        }
      if (j + 1 < 4) {
        __builtin_amdgcn_sched_group_barrier(0x100, NPL, 0);      // the next tile's plane reads first: they fly under these MFMAs
      } else if constexpr (next) {
        write_own(other, u, w);
        __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);        // the reads, then the split between the MFMAs by its dependences
        __builtin_amdgcn_sched_group_barrier(0x008, LIM >= 4 ? 14 : 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x200, NPL, 0);      // the stores leave under the last MFMAs
      }
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  };
  if (nm > 0) {
    const std::integral_constant<int, 0> s0{};
    const std::integral_constant<int, 1> s1{};
    issue(0, 0);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    float4 u, w;
    read_own(0, u, w);
    write_own(0, u, w);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    // the main loop runs the steps that a step follows, two at a time (one per stage); the last step, on either stage, is peeled behind it
    int m = 0;
    for (; m + 2 < nm; m += 2) {
      step(m, s0, std::true_type{});
      step(m + 1, s1, std::true_type{});
    }
    if (m + 2 == nm) step(m++, s0, std::true_type{});
    step(m, m & 1, std::false_type{});
  }
  if (nm == 0) return;                            // (a K range past the end: the range count is rounded up to a multiple of 8)
  const EpiAtomic<4> e{C, ldc};
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) e(acc[mb], m_base + wm * 64 + mb * 32, n_base, lane, M, N);
}

// gemm_ops.hip: launch_gemm_split_tn<nprod> and nothing else, for the tests (bound by visdial_amd._lib.internal)
int vd_gemm_split_tn_p(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int M, int N, int K, int nprod,
                       hipStream_t stream);

// C[M x N] += A[K x M]^T * B[K x N] on the exact split; M % 256 == 0, N % 128 == 0, K % 16 == 0 (the caller contracts a ragged tail elsewhere)
template <int NPROD>
static int launch_gemm_split_tn(int M, int N, int K, const float* A, long lda, const float* B, long ldb, float* C, long ldc, hipStream_t stream) {
  using Cfg = SplitTnCfg;
  VD_CHECK_ARG(M % Cfg::BM == 0 && N % Cfg::BN == 0 && K % 16 == 0 && lda % 4 == 0 && ldb % 4 == 0 && 16L * lda * 4 < (1L << 31) && 16L * ldb * 4 < (1L << 31),
               "launch_gemm_split_tn: unsupported shape M=%d N=%d K=%d", M, N, K);
  if (K == 0) return VD_OK;
  const int tiles_n = N / Cfg::BN, tiles = (M / Cfg::BM) * tiles_n;
  // one full round of workgroups at two per CU; a multiple of 8 K ranges so that each XCD owns whole ranges
  int splits = vd_cdiv(2L * vd_num_cus(), tiles);
  splits = (splits + 7) & ~7;
  int kchunk = vd_cdiv(vd_cdiv(K, splits), 16) * 16;
  if (kchunk < 64) kchunk = 64;
  splits = vd_cdiv(K, kchunk);
  if (splits >= 8) splits = (splits + 7) & ~7;        // (trailing K ranges past the end are empty workgroups)
  auto kern = gemm_split_tn_kernel<NPROD>;
  static bool attr_set[SPLIT_ATTR_DEVS] = {};                  // per instantiation
  if (const int rc = split_lds_attr(reinterpret_cast<const void*>(kern), attr_set)) return rc;
  hipLaunchKernelGGL(kern, dim3(tiles * splits), dim3(256), Cfg::lds_bytes(NPROD), stream, M, N, kchunk, K, tiles, tiles_n, splits, A, lda, B, ldb, C, ldc);
  VD_LAUNCH_CHECK();
  return VD_OK;
}
