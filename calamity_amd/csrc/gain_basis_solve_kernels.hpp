// gain_basis_solve_kernels.hpp -- gains confined to a frequency basis, g = g0 + B y, in closed form (cal_solver_solve_gain_coeffs):
// the damped StefCal sweeps of gain_solve_kernels.hpp projected on the basis.  With the other antennas held fixed, the chi-square is
// quadratic in one antenna's y; num and den are the per-antenna sums of gain_solve_ant_kernel from the OLD gains (autocorrelations
// left out).  For antenna row a (one antenna of one slice), g_a the current expanded gains, B [nfreqs][K] the attached basis:
//   r_a[f]  = num_a[f] - den_a[f] g_a[f]                 (complex; minus half the chi-square gradient w.r.t. g_a)
//   N_a     = B^T diag(den_a) B                          [K][K], real symmetric
//   rhs_a   = B^T r_a                                    [K], complex
//   (N_a + ridge (tr N_a / K) I) delta_a = rhs_a         (one factorisation, two right-hand sides: re, im)
//   y_a    <- y_a + damping delta_a                      then gains = g0 + B y for the whole array (gain_expand_kernel)
// Every antenna is solved from the old gains (a Jacobi sweep); the gains are rebuilt once per sweep.  B = I, ridge = 0 is the update
// of gain_solve_apply_kernel; damping = 1, ridge = 0 lands on the exact per-antenna minimiser.  Unlike the per-channel sweep a channel
// with den = 0 of a non-singular antenna does move: the basis interpolates across it.  Two kernels behind gain_solve_ant_kernel:
//   gain_basis_gram_kernel   N_a (lower triangle) and rhs_a of every antenna row on the matrix cores, in T, from the transposed basis copy
//   gain_basis_chol_kernel   per antenna row, in double: Cholesky of N_a + ridge, both substitutions, the masked damped update of y
//                            (also the factor step of gain_time_solve_kernels.hpp: L blocks of K unknowns per antenna, no mask)
// r_a is evaluated in double from the double planes and rounded to T once; N_a and rhs_a are formed and accumulated in T in a fixed
// order (no atomics on reals: two calls give the same bits); the factorisation, the substitutions and the update run in double for
// both dtypes, the update is rounded once.  The Gram blocks and the factorisation are the shared core of normal_solve.hpp; the two
// kernels here fetch its operands and write its result.
#pragma once
#include "normal_solve.hpp"

namespace calk {

// One workgroup per (antenna row of the chunk, 64 x 64 block (bi, bj <= bi) of N_a): blockIdx.x = row * npairs + pair, the pairs in
// the order (0,0) (1,0) (1,1) (2,0) ...  (the Gram core of normal_solve.hpp; the operand columns of rhs are r_r, r_i).  The band is
// walked in steps of kNsChunk channels: a step's piece of Bt ([kpad][fpad], zero-padded, so its rows and whole 16-byte pieces inside
// fpad are read unconditionally) is the operand, den_a (rounded to T as staged) its weight.  The planes are unpadded [nants][nfreqs]
// doubles: channels >= nfreqs stage zeros and are never read.  Rows of a slice whose mask byte is 0 are skipped
// (gain_basis_chol_kernel skips them too).  Output: nmat [row - a0][K][K] and rhs [nants][2][K], both T.
template <typename T>
__global__ __launch_bounds__(256) void gain_basis_gram_kernel(const T* __restrict__ Bt, const double* __restrict__ planes,
                                                               const vec2_t<T>* __restrict__ gains, T* __restrict__ nmat, T* __restrict__ rhs,
                                                               const unsigned char* __restrict__ slice_mask, int na_slice, int a0, int npairs,
                                                               int K, int kpad, int nants, int nfreqs, int fpad) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  typedef ns_vec_t<T> vec_t;
  typedef typename MmT<T>::v4 acc_t;
  __shared__ __attribute__((aligned(16))) T s_a[kNsBlock][kNsPitch];
  __shared__ __attribute__((aligned(16))) T s_b[kNsBlock][kNsPitch];
  __shared__ T s_v[3][kNsChunk];  // the step's den_a, r_r, r_i
  const int rel = blockIdx.x / npairs;
  const int pair = blockIdx.x - rel * npairs;
  const int a = a0 + rel;
  if (slice_mask && !slice_mask[a / na_slice]) return;  // the same for the whole block
  int bi = 0;
  while ((bi + 1) * (bi + 2) / 2 <= pair) ++bi;
  const int bj = pair - bi * (bi + 1) / 2;
  const int tid = threadIdx.x;
  const int k0 = bi * kNsBlock, l0 = bj * kNsBlock;
  const bool diag = bi == bj;
  acc_t acc[4], accr;
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = acc_t{0, 0, 0, 0};
  accr = acc_t{0, 0, 0, 0};
  const int njt = normal_gram_njt(K, k0, l0, diag);
  const long long plane = (long long)nants * nfreqs;
  const double* __restrict__ pa = planes + (long long)a * nfreqs;
  const vec2_t<T>* __restrict__ ga = gains + (long long)a * fpad;
  for (int c0 = 0; c0 < nfreqs; c0 += kNsChunk) {
    __syncthreads();  // the previous step's operands have been read
    if (tid < kNsChunk) {
      const int f = c0 + tid;
      T sd = 0, sr = 0, si = 0;
      if (f < nfreqs) {
        const double den = pa[2 * plane + f];
        const vec2_t<T> g = ga[f];
        sd = (T)den;
        sr = (T)(pa[f] - den * (double)g.x);
        si = (T)(pa[plane + f] - den * (double)g.y);
      }
      s_v[0][tid] = sd;
      s_v[1][tid] = sr;
      s_v[2][tid] = si;
    }
    normal_gram_step<T>(s_a, s_b, s_v, kNsChunk, k0, l0, diag, njt, bj == 0,
                        [&](int row, int c) {
                          vec_t v;
#pragma unroll
                          for (int x = 0; x < V; ++x) v[x] = (T)0;
                          // fpad is a multiple of 8: a piece is wholly inside the row or wholly outside
                          if (c0 + c < fpad && row < kpad) v = *reinterpret_cast<const vec_t*>(Bt + (long long)row * fpad + c0 + c);
                          return v;
                        },
                        acc, accr);
  }
  if (njt == 0) return;
  normal_gram_store<T>(nmat + (long long)rel * K * K, K, k0, l0, njt, bj == 0, acc, accr,
                       [&](int col, int row) { return rhs + ((long long)a * 2 + col) * K + row; });
}

// One workgroup per row of the chunk (an antenna row; under a time basis an antenna over all its times, L > 1 blocks of K unknowns):
// normal_chol_solve of normal_solve.hpp on the row's N_a and rhs_a, n = L K, its [n + 2][ld] matrix M in LDS when it fits
// `lds_doubles` and in the chunk's L2-resident scratch otherwise.  nmat [rel][n][n]; the right-hand sides are rows [2][n] of rhs, the
// row of chunk row rel being rhs_row0 + rel: rhs_row0 = a0 for the per-row buffer [nants][2][K] gain_basis_gram_kernel fills, 0 for the
// chunk's own [ca][2][n] of gain_time_kron_kernel.  A singular row (tr N_a <= 0: no unflagged cross-correlation) leaves its y alone and
// counts in counts[1]; a solved row counts in counts[0]; the rows of a slice whose mask byte is 0 (slice_mask may be null: every row)
// do neither.  The update y[a][l][k] + damping delta[l K + k] (rows of y at pitch kpad; L = 1: y[a][k]) is rounded to T once.
// (gain_time_chol_kernel of gain_time_solve_kernels.hpp was this kernel without the mask: merged into it.)
template <typename T>
__global__ __launch_bounds__(256) void gain_basis_chol_kernel(const T* __restrict__ nmat, const T* __restrict__ rhs, double* __restrict__ dscr,
                                                               vec2_t<T>* __restrict__ y, const unsigned char* __restrict__ slice_mask, int na_slice,
                                                               int a0, int rhs_row0, int L, int K, int kpad, double damping, double ridge,
                                                               int* __restrict__ counts, int lds_doubles) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double s_m[];
  __shared__ double s_red[256];
  const int rel = blockIdx.x;
  const int a = a0 + rel;
  if (slice_mask && !slice_mask[a / na_slice]) return;
  const int tid = threadIdx.x;
  const int n = L * K;
  const bool in_lds = (long long)(n + 2) * (n | 1) <= lds_doubles;
  const int ld = in_lds ? (n | 1) : n;  // (odd pitch: the rows a column step reads side by side lie on different banks)
  double* M = in_lds ? s_m : dscr + (long long)rel * (n + 2) * n;
  const T* __restrict__ ra = rhs + (long long)(rhs_row0 + rel) * 2 * n;
  if (!normal_chol_solve(M, ld, n, nmat + (long long)rel * n * n, ra, ra + n, ridge, s_red)) {
    if (tid == 0) atomicAdd(counts + 1, 1);
    return;
  }
  const double* xr = M + (long long)n * ld;
  const double* xi = M + (long long)(n + 1) * ld;
  vec2_t<T>* __restrict__ ya = y + (long long)a * L * kpad;
  for (int i = tid; i < n; i += 256) {
    const int l = i / K, k = i - l * K;
    const vec2_t<T> old = ya[(long long)l * kpad + k];
    vec2_t<T> out;
    out.x = (T)((double)old.x + damping * xr[i]);
    out.y = (T)((double)old.y + damping * xi[i]);
    ya[(long long)l * kpad + k] = out;
  }
  if (tid == 0) atomicAdd(counts, 1);
}

}  // namespace calk
