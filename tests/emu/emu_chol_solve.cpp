// tests/emu/emu_chol_solve.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// HalfWaveT::chol_solve_packed (sgrl_amd/csrc/wave_half.h: the register solver of lcp_block_pivot for one right-hand side) alone on the
// lane fibers of emu_pair.cpp: two problems per emulated wavefront, lanes 0..31 / 32..63, each half with its own n, matrix and
// right-hand side.  The scaffolding (fibers, rendezvous, EmuHalfPrim) is emu_pair.cpp's, included as it is.
//
// Built as a shared library by tests/test_chol_solve_emu.py; with -DSGRL_EMU_CHOL_MAIN it is a stand-alone program (own main, fixed
// cases) for a host sanitizer build.

#include "emu_pair.cpp"

namespace {
constexpr int kLd = 352, kGuard = 32;      // doubles per packed triangle slot (n <= 26), guard words around every buffer

struct CholCall {
  int inverse;
  int n[2];
  double* C[2];
  double* x[2];
  double* wv[2];
  int ok[2];
} cc;

void chol_lane_body(int) {
  EmuHalfWave w;
  const int h = w.half, n = cc.n[h];
  double* C = cc.C[h];
  double* x = cc.x[h];
  double* wv = cc.wv[h];
  bool done;
  if (!cc.inverse) {
    done = w.chol_solve_packed(n, C, x, sgrl::kMinVal);
  } else {                     // the explicit-inverse path as lcp_block_pivot runs it for a policy without the primitive
    done = w.chol_inv_packed(n, C, sgrl::kMinVal);
    if (done) {
      w.lanes(n, [&](int i) {
        double z = 0;
        for (int c = 0; c <= i; c++) z += C[i * (i + 1) / 2 + c] * x[c];
        wv[i] = z;
      });
      w.lanes(n, [&](int k) {
        double s = 0;
        for (int i = k; i < n; i++) s += C[i * (i + 1) / 2 + k] * wv[i];
        x[k] = s;
      });
    }
  }
  if (w.lane == 0) cc.ok[h] = done ? 1 : 0;
}
}  // namespace

extern "C" {

// Two problems (p = 0, 1): n[p] rows (0 .. 26), packed lower triangle at C + p * 352, right-hand side at x + p * 32, both in place;
// ok[p] = what the primitive returned.  inverse = 1: the explicit-inverse path instead.  Returns 0; -1 bad n; -2 the lanes of a half
// diverged; -3 an access left its triangle (n (n + 1) / 2 doubles) or its vector (32 doubles).
int sgrl_emu_chol_solve(int inverse, const int32_t* n, double* C, double* x, int32_t* ok) {
  for (int p = 0; p < 2; p++)
    if (n[p] < 0 || n[p] * (n[p] + 1) / 2 > kLd) return -1;
  const uint64_t pat = 0x7ff8dead0000beefull;
  std::vector<double> buf[2][3];
  for (int p = 0; p < 2; p++) {
    const int tri = n[p] * (n[p] + 1) / 2;
    const int len[3] = {tri > 0 ? tri : 1, 32, 32};      // an empty problem still reads entry 0 (as the engine's scratch allows)
    for (int k = 0; k < 3; k++) {
      buf[p][k].resize(len[k] + 2 * kGuard);
      for (auto& v : buf[p][k]) std::memcpy(&v, &pat, 8);
    }
    std::memcpy(buf[p][0].data() + kGuard, C + p * kLd, sizeof(double) * len[0]);
    std::memcpy(buf[p][1].data() + kGuard, x + p * 32, sizeof(double) * 32);
    cc.n[p] = n[p];
    cc.C[p] = buf[p][0].data() + kGuard;
    cc.x[p] = buf[p][1].data() + kGuard;
    cc.wv[p] = buf[p][2].data() + kGuard;
    cc.ok[p] = -1;
  }
  cc.inverse = inverse;
  if (run_wave(chol_lane_body) != 0) return -2;
  for (int p = 0; p < 2; p++) {
    for (int k = 0; k < 3; k++) {
      const size_t len = buf[p][k].size() - 2 * kGuard;
      for (int q = 0; q < kGuard; q++) {
        uint64_t a, b;
        std::memcpy(&a, &buf[p][k][q], 8); std::memcpy(&b, &buf[p][k][kGuard + len + q], 8);
        if (a != pat || b != pat) return -3;
      }
    }
    std::memcpy(C + p * kLd, cc.C[p], sizeof(double) * (buf[p][0].size() - 2 * kGuard));
    std::memcpy(x + p * 32, cc.x[p], sizeof(double) * 32);
    ok[p] = cc.ok[p];
  }
  return 0;
}
}

#ifdef SGRL_EMU_CHOL_MAIN
// stand-alone run of the sizes the tests use: A = Y Y' + diag(R) from a small generator, residual of the solution checked
int main() {
  const int pairs[][2] = {{1, 9}, {10, 15}, {16, 0}, {3, 14}, {15, 0}, {9, 9}};
  uint64_t s = 12345;
  auto rnd = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0 * 2.0 - 1.0; };
  int bad = 0;
  for (const auto& pr : pairs) {
    std::vector<double> C(2 * kLd, 0.0), x(64, 0.0), A(2 * kLd, 0.0), b(64, 0.0);
    int32_t n[2] = {pr[0], pr[1]}, ok[2];
    for (int p = 0; p < 2; p++) {
      std::vector<double> Y(26 * 24);
      for (auto& v : Y) v = rnd();
      for (int i = 0; i < n[p]; i++) {
        for (int j = 0; j <= i; j++) {
          double a = i == j ? 1e-4 : 0.0;
          for (int d = 0; d < 24; d++) a += Y[i * 24 + d] * Y[j * 24 + d];
          C[p * kLd + i * (i + 1) / 2 + j] = a;
        }
        x[p * 32 + i] = rnd();
      }
    }
    A = C; b = x;
    const int rc = sgrl_emu_chol_solve(0, n, C.data(), x.data(), ok);
    if (rc != 0) { std::printf("n = (%d, %d): rc %d\n", n[0], n[1], rc); bad++; continue; }
    for (int p = 0; p < 2; p++) {
      if (ok[p] != (n[p] <= 15 ? 1 : 0)) { std::printf("n = %d: ok %d\n", n[p], ok[p]); bad++; }
      if (!ok[p]) continue;
      double worst = 0.0, scale = 1e-300;
      for (int i = 0; i < n[p]; i++) {
        double r = -b[p * 32 + i];
        for (int j = 0; j < n[p]; j++) r += A[p * kLd + (i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i)] * x[p * 32 + j];
        worst = std::fmax(worst, std::fabs(r));
        scale = std::fmax(scale, std::fabs(b[p * 32 + i]));
      }
      std::printf("n = %2d  residual %.2e\n", n[p], worst / scale);
      if (!(worst / scale < 1e-9)) bad++;
    }
  }
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad ? 1 : 0;
}
#endif
