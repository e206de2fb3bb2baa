// Probe: sustained v_mfma_f32_32x32x16_bf16 rate of the chip on NON-ZERO operands (the clock follows the power budget:
// MI355X_MICROARCH.md "DVFS give-back"), register-only loop, 1 / 2 / 3 waves per SIMD.  The exact-split recurrence
// (csrc/split_core.h) can at best run at this rate.
// Second part: the two bf16 MFMA shapes side by side (v_mfma_f32_32x32x16_bf16 against v_mfma_f32_16x16x32_bf16: the same peak,
// but the chip may hold a different clock on each), at equal FLOP per wave, on zeros and on random operands, 1 / 2 / 3 waves per
// SIMD -- one workgroup of 4 / 8 / 12 waves per CU; a register-only arm and an arm that re-reads the B fragments from LDS by ds_read_b128 in the nine-product order of the
// split kernels (a 32 x 128 wave tile).  Each wave stamps s_memtime / s_memrealtime around its loop into a buffer of its own:
// the columns are wall, TFLOP/s, wave-cycles per MFMA per SIMD (MEDIAN wave; above one wave per SIMD the matrix pipe serves the oldest
// wave first, so the waves of a SIMD finish one after the other and the median reads 2/3 of the SIMD's cycles at three waves: compare
// cycles at one wave per SIMD, wall everywhere) and the in-kernel clock (s_memtime over s_memrealtime x 100 MHz).
//   hipcc --offload-arch=gfx950 -O3 scripts/probes/mfma_bf16_peak.hip -o scripts/probes/mfma_bf16_peak
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

template <int NACC>
__global__ void __launch_bounds__(256) mfma_loop(float* out, int iters, float seed) {
  f32x16 acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  bf16x8 a[3], b[4];
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int i = 0; i < 8; ++i) a[p][i] = (__bf16)(seed * (float)((threadIdx.x * 37 + i * 11 + p * 5) % 97 - 48) * 0.01f);
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int i = 0; i < 8; ++i) b[p][i] = (__bf16)(seed * (float)((threadIdx.x * 53 + i * 7 + p * 3) % 89 - 44) * 0.01f);
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int u = 0; u < 9; ++u)
#pragma unroll
      for (int j = 0; j < NACC; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[u % 3], b[(u + j) & 3], acc[j], 0, 0, 0);
  }
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NACC; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) s += acc[j][r];
  if (s == 12345.f) out[threadIdx.x] = s;
}

// the same for v_mfma_f32_32x32x2_f32 (4096 FLOP per instruction, 64 cycles per SIMD)
template <int NACC>
__global__ void __launch_bounds__(256) mfma_f32_loop(float* out, int iters, float seed) {
  f32x16 acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  float a[4], b[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    a[p] = seed * (float)((threadIdx.x * 37 + p * 5) % 97 - 48) * 0.0123f;
    b[p] = seed * (float)((threadIdx.x * 53 + p * 3) % 89 - 44) * 0.0117f;
  }
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int j = 0; j < NACC; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u & 3], b[(u + j) & 3], acc[j], 0, 0, 0);
  }
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NACC; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) s += acc[j][r];
  if (s == 12345.f) out[threadIdx.x] = s;
}
static void run_f32(const char* name, int blocks, int iters, float seed) {
  float* out;
  (void)hipMalloc(&out, 4096);
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  mfma_f32_loop<4><<<blocks, 256>>>(out, iters, seed);
  (void)hipDeviceSynchronize();
  (void)hipEventRecord(e0);
  mfma_f32_loop<4><<<blocks, 256>>>(out, iters, seed);
  (void)hipEventRecord(e1);
  (void)hipDeviceSynchronize();
  float ms;
  (void)hipEventElapsedTime(&ms, e0, e1);
  const double mfmas = (double)iters * 8 * 4;
  printf("%-52s %8.3f ms  %6.1f cycles@2.4GHz/MFMA/SIMD  %8.1f TFLOP/s\n", name, ms, ms * 1e-3 * 2.4e9 / (mfmas * blocks / 256.0), (double)blocks * 4 * mfmas * 4096.0 / ms / 1e9);
  (void)hipFree(out);
}

template <int NACC>
static void run(const char* name, int blocks, int iters, float seed) {
  float* out;
  (void)hipMalloc(&out, 4096);
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  mfma_loop<NACC><<<blocks, 256>>>(out, iters, seed);
  (void)hipDeviceSynchronize();
  (void)hipEventRecord(e0);
  mfma_loop<NACC><<<blocks, 256>>>(out, iters, seed);
  (void)hipEventRecord(e1);
  (void)hipDeviceSynchronize();
  float ms;
  (void)hipEventElapsedTime(&ms, e0, e1);
  const double waves = (double)blocks * 4;
  const double mfmas = (double)iters * 9 * NACC;
  printf("%-52s %8.3f ms  %6.1f cycles@2.4GHz/MFMA/SIMD  %8.1f TFLOP/s\n", name, ms, ms * 1e-3 * 2.4e9 / (mfmas * blocks / 256.0), waves * mfmas * 32768.0 / ms / 1e9);
  (void)hipFree(out);
}

// ---- shape comparison ------------------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
struct Stamp { unsigned long long cyc, rt; };
#define STAMP_BEGIN const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime()
#define STAMP_END                                                                                                   \
  if ((threadIdx.x & 63) == 0) {                                                                                    \
    Stamp st{__builtin_amdgcn_s_memtime() - c0, __builtin_amdgcn_s_memrealtime() - r0};                             \
    stamps[blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)] = st;                                                              \
  }
__device__ __forceinline__ bf16x8 frag_init(float seed, int mul, int p) {
  bf16x8 v;
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = (__bf16)(seed * (float)((threadIdx.x * mul + i * 11 + p * 5) % 97 - 48) * 0.01f);
  return v;
}

// register-only: SHAPE 32 = 8 accumulators of 16 registers, SHAPE 16 = 16 accumulators of 4 (equal FLOP per wave and iteration);
// consecutive MFMAs never share an accumulator
template <int SHAPE>
__global__ void __launch_bounds__(768) shape_reg_loop(float* out, Stamp* stamps, int iters, float seed) {
  constexpr int NACC = SHAPE == 32 ? 8 : 16;
  typedef typename std::conditional<SHAPE == 32, f32x16, f32x4>::type acc_t;
  acc_t acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; ++j)
#pragma unroll
    for (int r = 0; r < (SHAPE == 32 ? 16 : 4); ++r) acc[j][r] = 0.f;
  bf16x8 a[3], b[4];
#pragma unroll
  for (int p = 0; p < 3; ++p) a[p] = frag_init(seed, 37, p);
#pragma unroll
  for (int p = 0; p < 4; ++p) b[p] = frag_init(seed, 53, p);
  STAMP_BEGIN;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int u = 0; u < 9; ++u)
#pragma unroll
      for (int j = 0; j < NACC; ++j) {
        if constexpr (SHAPE == 32) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[u % 3], b[(u + j) & 3], acc[j], 0, 0, 0);
        else acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u % 3], b[(u + j) & 3], acc[j], 0, 0, 0);
      }
  }
  STAMP_END;
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NACC; ++j)
#pragma unroll
    for (int r = 0; r < (SHAPE == 32 ? 16 : 4); ++r) s += acc[j][r];
  if (s == 12345.f) out[threadIdx.x] = s;
}

// B from LDS: one iteration = 32 k of a 32 x 128 wave tile, all nine products.  Per B plane the fragments are read by ds_read_b128
// (16 bytes per lane, a contiguous 1 KB per wave instruction: conflict-free) and multiplied with the three A planes held in registers:
// SHAPE 32 = 2 k halves x (4 reads + 12 MFMAs), SHAPE 16 = 8 reads + 48 MFMAs.  Equal LDS bytes, equal FLOP, 64 accumulator registers.
// The stage alternates per iteration so that the reads stay in the loop.
template <int SHAPE>
__global__ void __launch_bounds__(768) shape_lds_loop(float* out, Stamp* stamps, int iters, float seed) {
  constexpr int NACC = SHAPE == 32 ? 4 : 16;
  constexpr int STAGE = 3 * 8 * 1024;
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];
  typedef typename std::conditional<SHAPE == 32, f32x16, f32x4>::type acc_t;
  for (int i = threadIdx.x; i < 2 * STAGE / 16; i += blockDim.x) *reinterpret_cast<bf16x8*>(lds + i * 16) = frag_init(seed, 53, i);
  __syncthreads();
  acc_t acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; ++j)
#pragma unroll
    for (int r = 0; r < (SHAPE == 32 ? 16 : 4); ++r) acc[j][r] = 0.f;
  bf16x8 a[2][3];                                  // SHAPE 32: [k half][plane]; SHAPE 16: [row tile][plane]
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int p = 0; p < 3; ++p) a[h][p] = frag_init(seed, 37, h * 3 + p);
  const int lane = threadIdx.x & 63;
  STAMP_BEGIN;
  for (int it = 0; it < iters; ++it) {
    const char* sb = lds + (it & 1) * STAGE + lane * 16;
    if constexpr (SHAPE == 32) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int p = 2; p >= 0; --p) {
          bf16x8 bp[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) bp[j] = *reinterpret_cast<const bf16x8*>(sb + (p * 8 + h * 4 + j) * 1024);
#pragma unroll
          for (int i = 2; i >= 0; --i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[h][i], bp[j], acc[j], 0, 0, 0);
        }
    } else {
#pragma unroll
      for (int p = 2; p >= 0; --p) {
        bf16x8 bp[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) bp[j] = *reinterpret_cast<const bf16x8*>(sb + (p * 8 + j) * 1024);
#pragma unroll
        for (int i = 2; i >= 0; --i)
#pragma unroll
          for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[rt * 8 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[rt][i], bp[j], acc[rt * 8 + j], 0, 0, 0);
      }
    }
  }
  STAMP_END;
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NACC; ++j)
#pragma unroll
    for (int r = 0; r < (SHAPE == 32 ? 16 : 4); ++r) s += acc[j][r];
  if (s == 12345.f) out[threadIdx.x] = s;
}

static int cmp_u64(const void* a, const void* b) {
  const unsigned long long x = *(const unsigned long long*)a, y = *(const unsigned long long*)b;
  return x < y ? -1 : x > y;
}
// one line: `flop` per wave and iteration, `mfmas` instructions per wave and iteration
template <class K>
static double run_shape(K kern, const char* name, int wps, int iters, float seed, double mfmas, double flop) {
  const int blocks = 256, threads = 256 * wps, waves = blocks * 4 * wps;   // one workgroup per CU: its waves are resident together
  float* out;
  Stamp* stamps;
  (void)hipMalloc(&out, 4096);
  (void)hipMalloc(&stamps, waves * sizeof(Stamp));
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  kern<<<blocks, threads>>>(out, stamps, iters, seed);                 // warm: code, clocks
  (void)hipDeviceSynchronize();
  (void)hipEventRecord(e0);
  kern<<<blocks, threads>>>(out, stamps, iters, seed);
  (void)hipEventRecord(e1);
  (void)hipDeviceSynchronize();
  float ms;
  (void)hipEventElapsedTime(&ms, e0, e1);
  Stamp* h = (Stamp*)malloc(waves * sizeof(Stamp));
  (void)hipMemcpy(h, stamps, waves * sizeof(Stamp), hipMemcpyDeviceToHost);
  unsigned long long* c = (unsigned long long*)malloc(waves * 8);
  unsigned long long* r = (unsigned long long*)malloc(waves * 8);
  for (int i = 0; i < waves; ++i) { c[i] = h[i].cyc; r[i] = h[i].rt; }
  qsort(c, waves, 8, cmp_u64);
  qsort(r, waves, 8, cmp_u64);
  const double cyc = (double)c[waves / 2], rt = (double)r[waves / 2];
  const double tf = (double)waves * iters * flop / ms / 1e9;
  printf("%-46s %8.3f ms %8.1f TFLOP/s %6.2f wave-cyc/MFMA/SIMD %6.3f GHz\n", name, ms, tf, cyc / (iters * mfmas * wps), cyc / rt * 0.1);
  free(h); free(c); free(r);
  (void)hipFree(out);
  (void)hipFree(stamps);
  return tf;
}
static void shape_pair(const char* arm, bool lds, int wps, int iters, float seed) {
  char n32[96], n16[96];
  snprintf(n32, sizeof n32, "%s 32x32x16 %d w/SIMD %s", arm, wps, seed == 0.f ? "zeros " : "random");
  snprintf(n16, sizeof n16, "%s 16x16x32 %d w/SIMD %s", arm, wps, seed == 0.f ? "zeros " : "random");
  double t32, t16;
  if (lds) {
    t32 = run_shape(shape_lds_loop<32>, n32, wps, iters, seed, 72, 72 * 32768.0);
    t16 = run_shape(shape_lds_loop<16>, n16, wps, iters, seed, 144, 144 * 16384.0);
  } else {
    t32 = run_shape(shape_reg_loop<32>, n32, wps, iters, seed, 72, 72 * 32768.0);
    t16 = run_shape(shape_reg_loop<16>, n16, wps, iters, seed, 144, 144 * 16384.0);
  }
  printf("%-46s 16x16x32 / 32x32x16 by wall = %.3f\n", "", t16 / t32);
}

int main() {
  run<8>("256 blocks (1 wave/SIMD), 8 acc, zero operands", 256, 40000, 0.f);
  run<8>("256 blocks (1 wave/SIMD), 8 acc, random operands", 256, 40000, 1.f);
  run<8>("512 blocks (2 waves/SIMD), 8 acc, random operands", 512, 20000, 1.f);
  run<4>("768 blocks (3 waves/SIMD), 4 acc, random operands", 768, 20000, 1.f);
  run<8>("256 blocks (1 wave/SIMD), 8 acc, random, long (0.4 s)", 256, 400000, 1.f);
  run_f32("f32 32x32x2: 256 blocks (1 wave/SIMD), zero operands", 256, 20000, 0.f);
  run_f32("f32 32x32x2: 256 blocks (1 wave/SIMD), random operands", 256, 20000, 1.f);
  run_f32("f32 32x32x2: 768 blocks (3 waves/SIMD), random operands", 768, 10000, 1.f);
  run_f32("f32 32x32x2: 256 blocks, random, long (0.4 s)", 256, 200000, 1.f);
  printf("\nbf16 MFMA shape, equal FLOP per wave (each line ~0.1-0.2 s after a warm launch of the same length)\n");
  for (int lds = 0; lds < 2; ++lds)
    for (int wps = 1; wps <= 3; ++wps) {
      shape_pair(lds ? "LDS-B" : "reg  ", lds, wps, 120000 / wps, 0.f);
      shape_pair(lds ? "LDS-B" : "reg  ", lds, wps, 120000 / wps, 1.f);
    }
  return 0;
}
