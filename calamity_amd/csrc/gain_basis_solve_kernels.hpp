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
// r_a is evaluated in double from the double planes and rounded to T once; N_a and rhs_a are formed and accumulated in T in a fixed
// order (no atomics on reals: two calls give the same bits); the factorisation, the substitutions and the update run in double for
// both dtypes, the update is rounded once.
#pragma once
#include "multi_mfma_kernels.hpp"

namespace calk {

constexpr int kGbsBlock = 64;  // rows / columns of N_a per workgroup: one 16-row tile per wave, four column tiles
constexpr int kGbsChunk = 32;  // channels staged per step
constexpr int kGbsPitch = 36;  // elements per LDS row: 16 rows x 4 channels of an MFMA operand land on 64 distinct banks (fp32)

// One workgroup per (antenna row of the chunk, 64 x 64 block (bi, bj <= bi) of N_a): blockIdx.x = row * npairs + pair, the pairs in
// the order (0,0) (1,0) (1,1) (2,0) ...  Wave w owns rows [16 w, 16 w + 16) of the block and up to four 16 x 16 accumulator tiles
// (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64, the reduction index is the channel), plus, in the blocks of column 0, a fifth whose
// columns 0 and 1 are rhs_r and rhs_i (operand columns r_r, r_i).  The band is walked in steps of kGbsChunk channels: the step's piece
// of Bt ([kpad][fpad], zero-padded, so its rows and whole 16-byte pieces inside fpad are read unconditionally) is staged into LDS
// twice, plain for the row operand and times den_a (rounded to T as staged) for the column operand.  The planes are unpadded
// [nants][nfreqs] doubles: channels >= nfreqs stage zeros and are never read.  Only tiles on or below the diagonal are computed and
// only elements on or below it are written.  Rows of a slice whose mask byte is 0 are skipped (gain_basis_chol_kernel skips them too).
// Output: nmat [row - a0][K][K] and rhs [nants][2][K], both T.
template <typename T>
__global__ __launch_bounds__(256) void gain_basis_gram_kernel(const T* __restrict__ Bt, const double* __restrict__ planes,
                                                               const vec2_t<T>* __restrict__ gains, T* __restrict__ nmat, T* __restrict__ rhs,
                                                               const unsigned char* __restrict__ slice_mask, int na_slice, int a0, int npairs,
                                                               int K, int kpad, int nants, int nfreqs, int fpad) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  typedef typename MmT<T>::v4 acc_t;
  __shared__ __attribute__((aligned(16))) T s_a[kGbsBlock][kGbsPitch];
  __shared__ __attribute__((aligned(16))) T s_b[kGbsBlock][kGbsPitch];
  __shared__ T s_den[kGbsChunk], s_rr[kGbsChunk], s_ri[kGbsChunk];
  const int rel = blockIdx.x / npairs;
  const int pair = blockIdx.x - rel * npairs;
  const int a = a0 + rel;
  if (slice_mask && !slice_mask[a / na_slice]) return;  // the same for the whole block
  int bi = 0;
  while ((bi + 1) * (bi + 2) / 2 <= pair) ++bi;
  const int bj = pair - bi * (bi + 1) / 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int k0 = bi * kGbsBlock, l0 = bj * kGbsBlock;
  const bool diag = bi == bj;
  constexpr int vpr = kGbsChunk / V;  // 16-byte pieces per staged row
  const bool wave_live = k0 + wave * 16 < K;
  acc_t acc[4], accr;
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = acc_t{0, 0, 0, 0};
  accr = acc_t{0, 0, 0, 0};
  // column tiles this wave computes: on or below the diagonal, and inside the matrix
  int njt = 0;
  if (wave_live) {
    njt = diag ? wave + 1 : 4;
    const int have = (K - l0 + 15) / 16;
    if (njt > have) njt = have;
  }
  const long long plane = (long long)nants * nfreqs;
  const double* __restrict__ pa = planes + (long long)a * nfreqs;
  const vec2_t<T>* __restrict__ ga = gains + (long long)a * fpad;
  for (int c0 = 0; c0 < nfreqs; c0 += kGbsChunk) {
    __syncthreads();  // the previous step's operands have been read
    if (tid < kGbsChunk) {
      const int f = c0 + tid;
      T sd = 0, sr = 0, si = 0;
      if (f < nfreqs) {
        const double den = pa[2 * plane + f];
        const vec2_t<T> g = ga[f];
        sd = (T)den;
        sr = (T)(pa[f] - den * (double)g.x);
        si = (T)(pa[plane + f] - den * (double)g.y);
      }
      s_den[tid] = sd;
      s_rr[tid] = sr;
      s_ri[tid] = si;
    }
    __syncthreads();
    for (int idx = tid; idx < kGbsBlock * vpr; idx += 256) {
      const int r = idx / vpr, c = (idx - r * vpr) * V;
      vec_t va, vb;
#pragma unroll
      for (int x = 0; x < V; ++x) va[x] = vb[x] = (T)0;
      const bool inband = c0 + c < fpad;  // fpad is a multiple of 8: a piece is wholly inside the row or wholly outside
      if (inband && k0 + r < kpad) va = *reinterpret_cast<const vec_t*>(Bt + (long long)(k0 + r) * fpad + c0 + c);
      if (diag) vb = va;
      else if (inband && l0 + r < kpad) vb = *reinterpret_cast<const vec_t*>(Bt + (long long)(l0 + r) * fpad + c0 + c);
#pragma unroll
      for (int x = 0; x < V; ++x) vb[x] *= s_den[c + x];  // the column operand is den B
      *reinterpret_cast<vec_t*>(&s_a[r][c]) = va;
      *reinterpret_cast<vec_t*>(&s_b[r][c]) = vb;
    }
    __syncthreads();
    if (njt > 0) {
#pragma unroll
      for (int kk = 0; kk < kGbsChunk; kk += 4) {
        const T av = s_a[wave * 16 + col][kk + kq];
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (t < njt) acc[t] = MmT<T>::mfma(av, s_b[t * 16 + col][kk + kq], acc[t]);
        if (bj == 0) {
          const T ub = col == 0 ? s_rr[kk + kq] : col == 1 ? s_ri[kk + kq] : (T)0;
          accr = MmT<T>::mfma(av, ub, accr);
        }
      }
    }
  }
  if (njt == 0) return;
  T* __restrict__ Na = nmat + (long long)rel * K * K;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = k0 + wave * 16 + MmT<T>::row_of(kq, r);
    if (row >= K) continue;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int cc = l0 + t * 16 + col;
      if (t < njt && cc <= row) Na[(long long)row * K + cc] = acc[t][r];
    }
    if (bj == 0 && col < 2) rhs[((long long)a * 2 + col) * K + row] = accr[r];
  }
}

// One workgroup per antenna row of the chunk, everything in double.  The lower triangle of N_a (+ the ridge on its diagonal) and, as
// rows K and K + 1, the two right-hand sides form one [K + 2][ld] matrix M, in LDS when it fits `lds_doubles` and in the chunk's
// L2-resident scratch otherwise.  Left-looking Cholesky by columns: column j of every row i >= j (the right-hand-side rows included,
// which is the forward substitution) takes its dot product with row j, then the column is divided by the pivot's root.  Back
// substitution by columns, the solution of both right-hand sides left in the two rows.  A row is singular when tr N_a <= 0 (no
// unflagged cross-correlation) or a pivot is <= 0 or not finite: it leaves its y alone and counts in counts[1]; a solved row counts
// in counts[0]; the rows of a slice whose mask byte is 0 do neither.  The update y + damping delta is rounded to T once.
template <typename T>
__global__ __launch_bounds__(256) void gain_basis_chol_kernel(const T* __restrict__ nmat, const T* __restrict__ rhs, double* __restrict__ dscr,
                                                               vec2_t<T>* __restrict__ y, const unsigned char* __restrict__ slice_mask, int na_slice,
                                                               int a0, int K, int kpad, double damping, double ridge, int* __restrict__ counts,
                                                               int lds_doubles) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double s_m[];
  __shared__ double s_red[256];
  const int rel = blockIdx.x;
  const int a = a0 + rel;
  if (slice_mask && !slice_mask[a / na_slice]) return;
  const int tid = threadIdx.x;
  const int n = K;
  const bool in_lds = (long long)(n + 2) * (n | 1) <= lds_doubles;
  const int ld = in_lds ? (n | 1) : n;  // (odd pitch: the rows a column step reads side by side lie on different banks)
  double* M = in_lds ? s_m : dscr + (long long)rel * (n + 2) * n;
  const T* __restrict__ Ng = nmat + (long long)rel * n * n;
  const T* __restrict__ ra = rhs + (long long)a * 2 * n;
  // the trace, in a fixed order
  double part = 0;
  for (int k = tid; k < n; k += 256) part += (double)Ng[(long long)k * n + k];
  s_red[tid] = part;
  __syncthreads();
  if (tid == 0) {
    double tr = 0;
    for (int k = 0; k < 256; ++k) tr += s_red[k];
    s_red[0] = tr;
  }
  __syncthreads();
  const double tr = s_red[0];
  if (!(tr > 0.0) || !isfinite(tr)) {
    if (tid == 0) atomicAdd(counts + 1, 1);
    return;
  }
  const double shift = ridge * (tr / n);
  for (long long idx = tid; idx < (long long)n * n; idx += 256) {
    const int i = (int)(idx / n), k = (int)(idx - (long long)i * n);
    if (k <= i) M[(long long)i * ld + k] = (double)Ng[idx] + (k == i ? shift : 0.0);
  }
  for (int k = tid; k < n; k += 256) {
    M[(long long)n * ld + k] = (double)ra[k];
    M[(long long)(n + 1) * ld + k] = (double)ra[n + k];
  }
  __syncthreads();
  for (int j = 0; j < n; ++j) {
    const double* __restrict__ Lj = M + (long long)j * ld;
    for (int i = j + tid; i < n + 2; i += 256) {
      double* Li = M + (long long)i * ld;
      double s = Li[j];
      for (int k = 0; k < j; ++k) s -= Li[k] * Lj[k];
      Li[j] = s;
    }
    __syncthreads();
    const double d = M[(long long)j * ld + j];  // the same value in every thread: the branch is uniform
    if (!(d > 0.0) || !isfinite(d)) {
      if (tid == 0) atomicAdd(counts + 1, 1);
      return;
    }
    __syncthreads();  // every thread has read the pivot
    const double root = sqrt(d);
    for (int i = j + 1 + tid; i < n + 2; i += 256) M[(long long)i * ld + j] /= root;
    if (tid == 0) M[(long long)j * ld + j] = root;
    __syncthreads();
  }
  // L^T x = z for the two rows z = M[n], M[n + 1]; x replaces z element by element
  double* yr = M + (long long)n * ld;
  double* yi = M + (long long)(n + 1) * ld;
  for (int j = n - 1; j >= 0; --j) {
    const double* __restrict__ Lj = M + (long long)j * ld;
    const double xr = yr[j] / Lj[j], xi = yi[j] / Lj[j];
    __syncthreads();  // every thread has read element j
    for (int k = tid; k < j; k += 256) {
      yr[k] -= Lj[k] * xr;
      yi[k] -= Lj[k] * xi;
    }
    if (tid == 0) {
      yr[j] = xr;
      yi[j] = xi;
    }
    __syncthreads();
  }
  vec2_t<T>* __restrict__ ya = y + (long long)a * kpad;
  for (int k = tid; k < n; k += 256) {
    const vec2_t<T> old = ya[k];
    vec2_t<T> out;
    out.x = (T)((double)old.x + damping * yr[k]);
    out.y = (T)((double)old.y + damping * yi[k]);
    ya[k] = out;
  }
  if (tid == 0) atomicAdd(counts, 1);
}

}  // namespace calk
