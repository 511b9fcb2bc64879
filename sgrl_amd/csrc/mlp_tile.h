// mlp_tile.h -- the device code the MLP family's row-tile kernels share (mlp_actor.hip: k_mlp_forward, k_mlp_critic, k_mlp_chain;
// mlp_train.hip: k_mlp_critic_fb, k_mlp_actor_fb): the tile loaders, the one panel product (tile_gemm, forward and backward), the one
// layer walk over it (mlp_walk, with or without a stash of the hidden activations), the critic's input tile from action rows the
// workgroup has just stored, and the zero tail of an output row.
//
// A workgroup is 4 waves and owns BM = 32 rows; its activation tile X[32][sx] lives in LDS beside two panel stages Ws.  Wave w owns
// the 32-column tiles w and w + 4 of each 256-column chunk (a narrow layer -- the 21 action columns -- costs one tile on one wave, not
// a 64-column pair).  MAXCH = chunks a workgroup keeps accumulators for (widths up to 256 MAXCH).  LDS operand layout as
// csrc/gemm_f32.h k_gemm2: rows of BK + 4 (panel) / sx = kmax + 4 (activations) floats, a lane (row, half) reads the contiguous k range
// [BK / 2 * half, + BK / 2) of its row with ds_read_b128; both strides are 4 * odd, so the 16 lanes of a read group fall on distinct
// 4-bank groups.
#ifndef SGRL_MLP_TILE_H
#define SGRL_MLP_TILE_H

#include "mlp_internal.h"

namespace sgrl_mlp_detail {

// X[r][col0 + k] for k in [0, fill): src[row0 + r][k] where k < valid and the row exists, zeros elsewhere.
__device__ __forceinline__ void load_rows(float* X, int sx, int col0, int valid, int fill, const float* __restrict__ src, int ld, int row0,
                                          int n_env) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < BM; r += 4) {
    const int row = row0 + r;
    for (int k = lane; k < fill; k += 64) X[r * sx + col0 + k] = (row < n_env && k < valid) ? src[(size_t)row * ld + k] : 0.f;
  }
}

// C/D layout of a 32 x 32 tile: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
__device__ __forceinline__ int tile_row(int e) { return (e & 3) + 8 * (e >> 2) + 4 * ((threadIdx.x & 63) >> 5); }

// acc (per owned 32-column tile) = X[32][0 : R) . B, then epi(column, acc) per owned tile, then a barrier (X and the panels free).
//   BWD false: B[k][n] = W[n * ldw + k]  (a layer forward: W the packed [N][ldw] weight, R = kpad, N = npad, a multiple of 32)
//   BWD true:  B[k][n] = W[k * ldw + n]  (a layer backward: rows k < R of the packed weight, columns n < N of them; any N)
// The caller has put a barrier behind its writes of X.  R is a multiple of BK.
template <int MAXCH, int BK, bool BWD, class Epi>
__device__ __forceinline__ void tile_gemm(const float* __restrict__ W, int ldw, int R, int N, float* X, float* Ws, int sx, Epi&& epi) {
  constexpr int SK = BK + 4;                   // forward panel: [CH][SK]
  constexpr int SB = CH + 4;                   // backward panel: [BK][SB]
  constexpr int STAGE = CH * SK;
  static_assert(BK * SB <= STAGE, "the backward panel must fit in a forward stage");
  constexpr int QPR = BK / 4;                  // float4 per forward panel row
  constexpr int RPP = 256 / QPR;               // forward panel rows covered per staging pass
  constexpr int NP = CH / RPP;                 // staging passes per forward panel
  static_assert(4 * NP == BK, "staging registers");
  constexpr int KH = BK / 2;                   // k values per lane half
  constexpr int NQ = KH / 4;                   // float4 per lane per operand row per k block
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, lh = lane >> 5;
  const int kq = t % QPR, r0 = t / QPR;
  const int Nt = (N + 31) & ~31;
  const int nkb = R / BK, nch = (Nt + CH - 1) / CH;
  f32x16 acc[MAXCH][2];
#pragma unroll
  for (int c = 0; c < MAXCH; c++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[c][j][e] = 0.f;
  float rw[BK];
  auto gload = [&](int kb, int c) {
    if (BWD) {
      const int col = CH * c + t;
#pragma unroll
      for (int i = 0; i < BK; i++) rw[i] = (col < N) ? W[(size_t)(kb * BK + i) * ldw + col] : 0.f;
    } else {
#pragma unroll
      for (int i = 0; i < NP; i++) {
        const int n = CH * c + r0 + RPP * i;
        const float4 v = (n < N) ? *reinterpret_cast<const float4*>(W + (size_t)n * ldw + kb * BK + 4 * kq) : make_float4(0.f, 0.f, 0.f, 0.f);
        rw[4 * i] = v.x; rw[4 * i + 1] = v.y; rw[4 * i + 2] = v.z; rw[4 * i + 3] = v.w;
      }
    }
  };
  auto sstore = [&](int st) {
    if (BWD) {
#pragma unroll
      for (int i = 0; i < BK; i++) Ws[st * STAGE + i * SB + t] = rw[i];
    } else {
#pragma unroll
      for (int i = 0; i < NP; i++)
        *reinterpret_cast<float4*>(Ws + st * STAGE + (r0 + RPP * i) * SK + 4 * kq) = make_float4(rw[4 * i], rw[4 * i + 1], rw[4 * i + 2], rw[4 * i + 3]);
    }
  };
  gload(0, 0);
  sstore(0);
  __syncthreads();
  int st = 0;
  const float* arow = X + li * sx + KH * lh;
  for (int kb = 0; kb < nkb; kb++) {
#pragma unroll
    for (int c = 0; c < MAXCH; c++) {
      if (c < nch) {
        // the panel after (kb, c): global loads in flight under this panel's matrix instructions, LDS writes into the idle stage
        int nc = c + 1, nk = kb;
        if (nc == nch) { nc = 0; nk = kb + 1; }
        const bool more = nk < nkb;
        if (more) gload(nk, nc);
        float4 av[NQ];
#pragma unroll
        for (int q = 0; q < NQ; q++) av[q] = *reinterpret_cast<const float4*>(arow + kb * BK + 4 * q);
#pragma unroll
        for (int j = 0; j < 2; j++) {
          const int colb = 32 * (wave + 4 * j);
          if (CH * c + colb < Nt) {           // wave-uniform
            float4 bv[NQ];
            if (BWD) {
              const float* bcol = Ws + st * STAGE + (KH * lh) * SB + colb + li;
#pragma unroll
              for (int q = 0; q < NQ; q++) bv[q] = make_float4(bcol[(4 * q) * SB], bcol[(4 * q + 1) * SB], bcol[(4 * q + 2) * SB], bcol[(4 * q + 3) * SB]);
            } else {
              const float* brow = Ws + st * STAGE + (colb + li) * SK + KH * lh;
#pragma unroll
              for (int q = 0; q < NQ; q++) bv[q] = *reinterpret_cast<const float4*>(brow + 4 * q);
            }
#pragma unroll
            for (int q = 0; q < NQ; q++) {
              acc[c][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q].x, bv[q].x, acc[c][j], 0, 0, 0);
              acc[c][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q].y, bv[q].y, acc[c][j], 0, 0, 0);
              acc[c][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q].z, bv[q].z, acc[c][j], 0, 0, 0);
              acc[c][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q].w, bv[q].w, acc[c][j], 0, 0, 0);
            }
          }
        }
        if (more) sstore(st ^ 1);
        __syncthreads();
        st ^= 1;
      }
    }
  }
  // every read of X and of the panels is behind the last barrier
#pragma unroll
  for (int c = 0; c < MAXCH; c++)
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int colb = CH * c + 32 * (wave + 4 * j);
      if (colb >= Nt) continue;
      epi(colb + li, acc[c][j]);
    }
  __syncthreads();
}

// Every layer of `a` forward over the activation tile X (input in columns [0, kpad[0]), the caller has put a barrier behind its
// writes): hidden layers write relu(. + bias) back over X in place -- the hidden activations never leave the chip -- and, where the
// caller passes a stash A (null: none), also to A[l] [B][npad_l] for the rows < B; the last layer's accumulators go to
// last(n, acc, bias_n) once per 32-column tile the wave owns (n = the lane's column, rows by tile_row).  Returns behind a barrier: X and
// the panels are free.
template <int MAXCH, int BK, class Last>
__device__ __forceinline__ void mlp_walk(const Net& a, float* const* A, float* X, float* Ws, int sx, int row0, int B, Last&& last) {
  for (int l = 0; l < a.n_layers; l++) {
    const int K = a.kpad[l], N = a.npad[l];
    const float* __restrict__ bias = a.wp + a.b_off[l];
    const bool is_last = l + 1 == a.n_layers;
    float* Al = A ? A[l] : nullptr;
    tile_gemm<MAXCH, BK, false>(a.wp + a.w_off[l], K, K, N, X, Ws, sx, [&](int n, const f32x16& acc) {
      const float bvv = bias[n];
      if (!is_last) {
#pragma unroll
        for (int e = 0; e < 16; e++) {
          const int m = tile_row(e);
          const float v = fmaxf(acc[e] + bvv, 0.f);
          X[m * sx + n] = v;
          if (Al && row0 + m < B) Al[(size_t)(row0 + m) * N + n] = v;
        }
      } else {
        last(n, acc, bvv);
      }
    });
  }
}

// A critic's input tile cat([obs, action]) where the action rows are the ones this workgroup's walk of the actor has just stored to
// abuf: observation columns from global again, zeros behind the action columns up to the padded width kpad0, and the action columns
// re-read by the very lanes that stored them -- the (chunk, wave, lane) -> column mapping of the actor's last layer, n_act_pad columns
// wide -- so same-thread program order is all the ordering it needs: no fence, no cross-workgroup traffic (abuf must not be
// restrict-qualified at the caller).  The caller puts the barrier behind it.
template <int MAXCH>
__device__ __forceinline__ void load_obs_stored_actions(float* X, int sx, const float* obs, int obs_ld, int in_dim, const float* abuf, int abuf_ld,
                                                        int out_dim, int n_act_pad, int kpad0, int row0, int n_env) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31;
  load_rows(X, sx, 0, in_dim, in_dim, obs, obs_ld, row0, n_env);
  load_rows(X, sx, in_dim + out_dim, 0, kpad0 - in_dim - out_dim, obs, 0, row0, n_env);
#pragma unroll
  for (int c = 0; c < MAXCH; c++)
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int n = CH * c + 32 * (wave + 4 * j) + li;
      if (CH * c + 32 * (wave + 4 * j) >= n_act_pad || n >= out_dim) continue;
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int m = tile_row(e);
        X[m * sx + in_dim + n] = (row0 + m < n_env) ? abuf[(size_t)(row0 + m) * abuf_ld + n] : 0.f;
      }
    }
}

// dst[row][out_dim : ld) of the workgroup's rows that exist: exact zeros (the slots beyond the output width, up to the caller's
// leading dimension)
__device__ __forceinline__ void zero_tail(float* dst, int ld, int out_dim, int row0, int n_env) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < BM; r += 4) {
    const int row = row0 + r;
    if (row >= n_env) break;
    for (int n = out_dim + lane; n < ld; n += 64) dst[(size_t)row * ld + n] = 0.f;
  }
}

}  // namespace sgrl_mlp_detail

#endif  // SGRL_MLP_TILE_H
