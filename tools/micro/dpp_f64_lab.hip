// tools/micro/dpp_f64_lab.hip -- the gfx950 64-bit DPP forms behind wave_hip.h fnma_bcast16_run / fnma_bcast16_self / bcast16_b64:
//   (a) v_fmac_f64_dpp and v_mov_b64_dpp with row_newbcast:0..15 return lane J of each of the four 16-lane rows -- all lanes active,
//       and with one 32-lane half masked off (the state of the two-environments-per-wavefront kernel's divergent branches);
//   (b) issue cost of `acc[k] -= m * (lane k of src)` over 24 independent accumulators, one wave and two waves per SIMD:
//       2 x v_readlane_b32 + v_fma_f64 | 2 x v_mov_b32_dpp + v_fma_f64 | v_mov_b64_dpp + v_fma_f64 | v_fmac_f64_dpp.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I sgrl_amd/csrc -o tools/micro/dpp_f64_lab.exe tools/micro/dpp_f64_lab.hip && tools/micro/dpp_f64_lab.exe
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

#define SGRL_CONST_AS __attribute__((address_space(4)))
#define SGRL_ITAB_AS __attribute__((address_space(3)))
#define SGRL_FTAB_AS __attribute__((address_space(4)))
#include "wave_hip.h"

using Prim = sgrl::HipHalfPrim<sgrl::DimsAny>;

// ---- (a) out[test][lane]: tests 0..15 bcast16_b64<J>, 16..31 fnma_bcast16_run (one group of 16), 32..47 fnma_bcast16_self<1, J>
template <int J>
__device__ __forceinline__ void check_one(double x, double m, double* out, int t) {
  out[J * 64 + t] = sgrl::bcast16_b64<J>(x);
  double s = x;
  sgrl::fnma_bcast16_self<1, J>(&s, (t & 15) == J ? 0.0 : m);
  out[(32 + J) * 64 + t] = s;
  if constexpr (J + 1 < 16) check_one<J + 1>(x, m, out, t);
}
__global__ void k_check(const double* in, double* out, int mode) {
  const int t = threadIdx.x;
  const double x = in[t], m = in[64 + t];
  auto body = [&]() {
    check_one<0>(x, m, out, t);
    double acc[16];
#pragma unroll
    for (int k = 0; k < 16; k++) acc[k] = in[128 + t] + k;
    sgrl::fnma_bcast16_run<16, 0>(acc, x, m);
#pragma unroll
    for (int k = 0; k < 16; k++) out[(16 + k) * 64 + t] = acc[k];
  };
  if (mode == 0) body();
  else if (mode == 1) { if (t < 32) body(); }
  else { if (t >= 32) body(); }
}

// ---- (b) one block of 24 accumulators per repetition; the source is made opaque every repetition (a fresh pivot column)
template <int FORM>
__device__ __forceinline__ void block24(double* acc, double src, double m) {
  if constexpr (FORM == 0) {
#pragma unroll
    for (int k = 0; k < 24; k++) acc[k] -= m * sgrl::read_lane(src, k);
  } else if constexpr (FORM == 1) {
#pragma unroll
    for (int k = 0; k < 24; k++) acc[k] -= m * Prim::bcast16(src, k & 15);
  } else if constexpr (FORM == 2) {
#pragma unroll
    for (int k = 0; k < 24; k++) {
      switch (k & 15) {
        case 0: acc[k] -= m * sgrl::bcast16_b64<0>(src); break;    case 1: acc[k] -= m * sgrl::bcast16_b64<1>(src); break;
        case 2: acc[k] -= m * sgrl::bcast16_b64<2>(src); break;    case 3: acc[k] -= m * sgrl::bcast16_b64<3>(src); break;
        case 4: acc[k] -= m * sgrl::bcast16_b64<4>(src); break;    case 5: acc[k] -= m * sgrl::bcast16_b64<5>(src); break;
        case 6: acc[k] -= m * sgrl::bcast16_b64<6>(src); break;    case 7: acc[k] -= m * sgrl::bcast16_b64<7>(src); break;
        case 8: acc[k] -= m * sgrl::bcast16_b64<8>(src); break;    case 9: acc[k] -= m * sgrl::bcast16_b64<9>(src); break;
        case 10: acc[k] -= m * sgrl::bcast16_b64<10>(src); break;  case 11: acc[k] -= m * sgrl::bcast16_b64<11>(src); break;
        case 12: acc[k] -= m * sgrl::bcast16_b64<12>(src); break;  case 13: acc[k] -= m * sgrl::bcast16_b64<13>(src); break;
        case 14: acc[k] -= m * sgrl::bcast16_b64<14>(src); break;  default: acc[k] -= m * sgrl::bcast16_b64<15>(src); break;
      }
    }
  } else {
    sgrl::fnma_bcast16_run<16, 0>(acc, src, m);
    sgrl::fnma_bcast16_run<8, 0>(acc + 16, src, m);
  }
}
template <int FORM>
__global__ void k_time(const double* in, double* out, long long* cyc, int reps) {
  const int t = threadIdx.x;
  double acc[24];
#pragma unroll
  for (int k = 0; k < 24; k++) acc[k] = in[128 + (t & 63)] + k;
  double src = in[t & 63];
  const double m = in[64 + (t & 63)] * 1e-3;
  const long long t0 = __builtin_readcyclecounter();
#pragma unroll 1
  for (int r = 0; r < reps; r++) {
    asm volatile("" : "+v"(src));
    block24<FORM>(acc, src, m);
  }
  const long long t1 = __builtin_readcyclecounter();
  double s = 0;
#pragma unroll
  for (int k = 0; k < 24; k++) s += acc[k];
  out[t] = s;
  if ((t & 63) == 0) cyc[t >> 6] = t1 - t0;
}

template <int FORM>
static int time_form(const char* name, const double* din, double* dout, long long* dcyc, const std::vector<double>& in) {
  const int reps = 2000;
  double first[64];
  for (int waves = 4; waves <= 8; waves += 4) {          // one workgroup on one CU: 4 waves = one per SIMD, 8 = two per SIMD
    long long best = 0;
    std::vector<double> out(64 * waves);
    for (int trial = 0; trial < 5; trial++) {
      hipLaunchKernelGGL(k_time<FORM>, dim3(1), dim3(64 * waves), 0, 0, din, dout, dcyc, reps);
      if (hipDeviceSynchronize() != hipSuccess) { printf("%s: kernel failed\n", name); return 1; }
      std::vector<long long> cyc(waves);
      hipMemcpy(cyc.data(), dcyc, 8 * waves, hipMemcpyDeviceToHost);
      long long mx = 0;
      for (long long c : cyc) mx = c > mx ? c : mx;
      if (trial == 0 || mx < best) best = mx;
    }
    hipMemcpy(out.data(), dout, 8 * 64 * waves, hipMemcpyDeviceToHost);
    printf("%-36s %d wave(s) per SIMD: %8.1f counter ticks per block of 24 (per wave)\n", name, waves / 4, (double)best / reps);
    if (waves == 4) for (int i = 0; i < 64; i++) first[i] = out[i];
  }
  // every form computes the same sums: form 0 on the host's lanes 0..23 is the odd one out (it reads lanes 16..23 of row 0, the
  // DPP forms lanes 0..7 of the lane's own row), so the forms are compared among themselves by the caller
  double chk = 0;
  for (int i = 0; i < 64; i++) chk += first[i];
  printf("%-36s checksum %.17g\n", name, chk);
  (void)in;
  return 0;
}

int main() {
  std::vector<double> in(192), out(48 * 64);
  for (int i = 0; i < 64; i++) { in[i] = std::sin(1.0 + i) * 100.0 + i; in[64 + i] = std::cos(0.5 + i) + 1.5; in[128 + i] = 0.25 * i - 3.0; }
  double *din, *dout; long long* dcyc;
  hipMalloc(&din, 192 * 8); hipMalloc(&dout, 48 * 64 * 8); hipMalloc(&dcyc, 64 * 8);
  hipMemcpy(din, in.data(), 192 * 8, hipMemcpyHostToDevice);
  int bad = 0;
  for (int mode = 0; mode < 3; mode++) {
    hipMemset(dout, 0xff, 48 * 64 * 8);
    hipLaunchKernelGGL(k_check, dim3(1), dim3(64), 0, 0, din, dout, mode);
    if (hipDeviceSynchronize() != hipSuccess) { printf("kernel failed\n"); return 2; }
    hipMemcpy(out.data(), dout, 48 * 64 * 8, hipMemcpyDeviceToHost);
    for (int t = 0; t < 64; t++) {
      if ((mode == 1 && t >= 32) || (mode == 2 && t < 32)) continue;        // masked half: nothing written
      for (int j = 0; j < 16; j++) {
        const double b = in[(t & ~15) | j], m = in[64 + t];                 // lane j of the lane's own 16-lane row
        const double mov = out[j * 64 + t], run = out[(16 + j) * 64 + t], self = out[(32 + j) * 64 + t];
        const double want_run = std::fma(-m, b, in[128 + t] + j);
        const double want_self = (t & 15) == j ? in[t] : std::fma(-m, b, in[t]);
        if (mov != b) { if (bad++ < 10) printf("mode %d v_mov_b64_dpp j=%d lane %d: %g != %g\n", mode, j, t, mov, b); }
        if (run != want_run) { if (bad++ < 10) printf("mode %d v_fmac_f64_dpp run j=%d lane %d: %.17g != %.17g\n", mode, j, t, run, want_run); }
        if (self != want_self) { if (bad++ < 10) printf("mode %d v_fmac_f64_dpp self j=%d lane %d: %.17g != %.17g\n", mode, j, t, self, want_self); }
      }
    }
  }
  printf(bad ? "dpp_f64_lab: %d MISMATCHES\n" : "dpp_f64_lab: v_mov_b64_dpp and v_fmac_f64_dpp row_newbcast:0..15 ok (all lanes, half 0 alone, half 1 alone)\n", bad);
  if (bad) return 1;
  if (time_form<0>("2 x v_readlane_b32 + v_fma_f64", din, dout, dcyc, in)) return 2;
  if (time_form<1>("2 x v_mov_b32_dpp + v_fma_f64", din, dout, dcyc, in)) return 2;
  if (time_form<2>("v_mov_b64_dpp + v_fma_f64 (builtin)", din, dout, dcyc, in)) return 2;
  if (time_form<3>("v_fmac_f64_dpp (asm)", din, dout, dcyc, in)) return 2;
  return 0;
}
