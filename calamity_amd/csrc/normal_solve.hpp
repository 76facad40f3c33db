// normal_solve.hpp -- what the closed-form solves share (coeff_solve_kernels.hpp, gain_basis_solve_kernels.hpp): every one of them
// builds per unknown vector (a fitting group, an antenna row) the normal equations of a weighted least-squares problem,
//   N = A^T diag(w) A   [n][n], real symmetric        rhs = A^T u   [n], complex        (N + ridge (tr N / n) I) delta = rhs,
// N and rhs in T on the matrix cores, the solve in double.  Here are
//   the Gram core     normal_gram_njt, normal_gram_step, normal_gram_store: one workgroup per 64 x 64 block (bi, bj <= bi) of N
//   the solve         normal_chol_solve: one workgroup per N, Cholesky and both substitutions (normal_chol_load and normal_chol_factor,
//                     which the factor kernels of fit_error_kernels.hpp and gain_error_kernels.hpp call too, and their
//                     normal_chol_invert: W = L^-1 in place)
// A kernel brings what is its own: which rows A has and where they lie, the three per-channel vectors w, u_r, u_i of a step, where
// N, rhs and the update go.  N and rhs are accumulated in a fixed order (no atomics on reals: two calls give the same bits).
#pragma once
#include "multi_mfma_kernels.hpp"

namespace calk {

constexpr int kNsBlock = 64;    // rows / columns of N per workgroup: one 16-row tile per wave, four column tiles
constexpr int kNsChunk = 32;    // channels staged per step at the most
constexpr int kNsPitch = 36;    // elements per LDS row: 16 rows x 4 channels of an MFMA operand land on 64 distinct banks (fp32)

template <typename T> using ns_vec_t = T __attribute__((ext_vector_type(16 / (int)sizeof(T))));  // a 16-byte piece of a row of A

// Wave w of the block owns rows [k0 + 16 w, k0 + 16 w + 16) and up to four 16 x 16 accumulator tiles (v_mfma_f32_16x16x4_f32 /
// v_mfma_f64_16x16x4_f64, the reduction index is the channel) over columns [l0, l0 + 64).  The column tiles it computes: on or below
// the diagonal, and inside the matrix.
__device__ __forceinline__ int normal_gram_njt(int n, int k0, int l0, bool diag) {
  const int wave = threadIdx.x >> 6;
  if (k0 + wave * 16 >= n) return 0;
  int njt = diag ? wave + 1 : 4;
  const int have = (n - l0 + 15) / 16;
  return njt > have ? have : njt;
}

// One step of cw <= kNsChunk channels (a multiple of 4 and of a 16-byte piece).  The caller has written the step's w, u_r, u_i to
// LDS (s_v[0], s_v[1], s_v[2]) behind a barrier that ends the previous step's reads.  piece(row, c) yields the 16 bytes of row `row`
// of A from channel c of the step on, zeros where A has none.  Rows [k0, k0 + 64) are staged plain for the row operand, rows
// [l0, l0 + 64) times w for the column operand; then every wave runs its MFMA chain in channel order, tile by tile, and with
// `with_rhs` (the blocks of column 0) a fifth accumulator whose columns 0 and 1 are rhs_r and rhs_i.
template <typename T, typename Piece>
__device__ __forceinline__ void normal_gram_step(T (*s_a)[kNsPitch], T (*s_b)[kNsPitch], const T (*s_v)[kNsChunk], int cw, int k0, int l0,
                                                 bool diag, int njt, bool with_rhs, Piece piece, typename MmT<T>::v4 (&acc)[4],
                                                 typename MmT<T>::v4& accr) {
  constexpr int V = 16 / (int)sizeof(T);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int vpr = cw / V;  // 16-byte pieces per staged row
  __syncthreads();
  for (int idx = tid; idx < kNsBlock * vpr; idx += 256) {
    const int r = idx / vpr, c = (idx - r * vpr) * V;
    const ns_vec_t<T> va = piece(k0 + r, c);
    ns_vec_t<T> vb = diag ? va : piece(l0 + r, c);
#pragma unroll
    for (int x = 0; x < V; ++x) vb[x] *= s_v[0][c + x];  // the column operand is w A
    *reinterpret_cast<ns_vec_t<T>*>(&s_a[r][c]) = va;
    *reinterpret_cast<ns_vec_t<T>*>(&s_b[r][c]) = vb;
  }
  __syncthreads();
  if (njt > 0) {
    for (int kk = 0; kk < cw; kk += 4) {
      const T a = s_a[wave * 16 + col][kk + kq];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t < njt) acc[t] = MmT<T>::mfma(a, s_b[t * 16 + col][kk + kq], acc[t]);
      if (with_rhs) {
        const T u = s_v[1 + (col & 1)][kk + kq];  // u_r for column 0, u_i for column 1, nothing beyond
        accr = MmT<T>::mfma(a, col < 2 ? u : (T)0, accr);
      }
    }
  }
}

// The elements on or below the diagonal go to N ([n][n]); with `with_rhs`, rhs_at(col, row) is where rhs_r (col 0) / rhs_i (col 1)
// of row `row` goes.
template <typename T, typename RhsAt>
__device__ __forceinline__ void normal_gram_store(T* __restrict__ N, int n, int k0, int l0, int njt, bool with_rhs,
                                                  const typename MmT<T>::v4 (&acc)[4], const typename MmT<T>::v4& accr, RhsAt rhs_at) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = k0 + wave * 16 + MmT<T>::row_of(kq, r);
    if (row >= n) continue;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int cc = l0 + t * 16 + col;
      if (t < njt && cc <= row) N[(long long)row * n + cc] = acc[t][r];
    }
    if (with_rhs && col < 2) *rhs_at(col, row) = accr[r];
  }
}

// What every caller of the Cholesky shares (normal_chol_solve below, fit_error_factor_kernel of fit_error_kernels.hpp), by the whole
// workgroup (256 threads), everything in double; s_red: 256 doubles of LDS.
// normal_chol_load: the trace of N in a fixed order, then the lower triangle of N + ridge (tr N / n) I into rows [0, n) of M (pitch
// ld).  Returns false, the same in every thread, when tr N <= 0 or not finite.  No barrier behind the writes: the caller may fill
// further rows of M first; normal_chol_factor begins with one.  tr N stays in s_red[0] (gain_error_factor_kernel reads the shift from it).
template <typename T>
__device__ __forceinline__ bool normal_chol_load(double* M, int ld, int n, const T* __restrict__ Ng, double ridge, double* s_red) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
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
  if (!(tr > 0.0) || !isfinite(tr)) return false;
  const double shift = ridge * (tr / n);
  for (long long idx = tid; idx < (long long)n * n; idx += 256) {
    const int i = (int)(idx / n), k = (int)(idx - (long long)i * n);
    if (k <= i) M[(long long)i * ld + k] = (double)Ng[idx] + (k == i ? shift : 0.0);
  }
  return true;
}
// normal_chol_factor: left-looking Cholesky by columns of the first n columns of the [nrows][ld] matrix M, nrows >= n.  Column j of
// every row i >= j (rows [n, nrows) are right-hand sides, for which this is the forward substitution) takes its dot product with row
// j, then the column is divided by the pivot's root.  Returns false, the same in every thread, at a pivot <= 0 or not finite; true
// behind a barrier, L in the lower triangle of rows [0, n).
__device__ __forceinline__ bool normal_chol_factor(double* M, int ld, int n, int nrows) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  __syncthreads();
  for (int j = 0; j < n; ++j) {
    const double* __restrict__ Lj = M + (long long)j * ld;
    for (int i = j + tid; i < nrows; i += 256) {
      double* Li = M + (long long)i * ld;
      double s = Li[j];
      for (int k = 0; k < j; ++k) s -= Li[k] * Lj[k];
      Li[j] = s;
    }
    __syncthreads();
    const double d = M[(long long)j * ld + j];  // the same value in every thread: the branch is uniform
    if (!(d > 0.0) || !isfinite(d)) return false;
    __syncthreads();  // every thread has read the pivot
    const double root = sqrt(d);
    for (int i = j + 1 + tid; i < nrows; i += 256) M[(long long)i * ld + j] /= root;
    if (tid == 0) M[(long long)j * ld + j] = root;
    __syncthreads();
  }
  return true;
}

// normal_chol_invert: W = L^-1 replaces L (rows [0, n) of M behind normal_chol_factor) row by row:
// W[i][k] = -(sum_{j = k}^{i - 1} L[i][j] W[j][k]) / L[i][i] reads row i of L and the rows of W above it; the row goes to the spare row
// M[n] first, because its elements are still being read as L.  Ends behind a barrier.
__device__ __forceinline__ void normal_chol_invert(double* M, int ld, int n) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  double* spare = M + (long long)n * ld;
  for (int i = 0; i < n; ++i) {
    double* Li = M + (long long)i * ld;
    const double piv = Li[i];
    for (int k = tid; k <= i; k += 256) {
      double s = k == i ? 1.0 : 0.0;
      for (int j = k; j < i; ++j) s -= Li[j] * M[(long long)j * ld + k];
      spare[k] = s / piv;
    }
    __syncthreads();  // row i of L has been read
    for (int k = tid; k <= i; k += 256) Li[k] = spare[k];
    __syncthreads();
  }
}

// (N + ridge (tr N / n) I) x = rhs for both right-hand sides, by the whole workgroup (256 threads), everything in double.  The
// lower triangle of N (+ the ridge on its diagonal) and, as rows n and n + 1, the two right-hand sides form one [n + 2][ld] matrix M
// (LDS or global scratch, the caller's choice; s_red: 256 doubles of LDS): normal_chol_load, normal_chol_factor over all n + 2 rows,
// then the back substitution by columns; x replaces the two rows behind the last column.  Returns false, the same in every thread,
// when N is singular: tr N <= 0 or not finite, or a pivot <= 0 or not finite.  Returns true behind a barrier, x in M[n] and M[n + 1].
template <typename T>
__device__ __forceinline__ bool normal_chol_solve(double* M, int ld, int n, const T* __restrict__ Ng, const T* __restrict__ rhs_r,
                                                  const T* __restrict__ rhs_i, double ridge, double* s_red) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  if (!normal_chol_load(M, ld, n, Ng, ridge, s_red)) return false;
  for (int k = tid; k < n; k += 256) {
    M[(long long)n * ld + k] = (double)rhs_r[k];
    M[(long long)(n + 1) * ld + k] = (double)rhs_i[k];
  }
  if (!normal_chol_factor(M, ld, n, n + 2)) return false;
  // L^T x = z for the two rows z = M[n], M[n + 1].  Column j leaves z[j] alone (every thread divides it for itself), so no thread
  // waits for another's write inside the loop; the same division once more, behind the loop, puts x in place of z.
  double* yr = M + (long long)n * ld;
  double* yi = M + (long long)(n + 1) * ld;
  for (int j = n - 1; j >= 0; --j) {
    const double* __restrict__ Lj = M + (long long)j * ld;
    const double xr = yr[j] / Lj[j], xi = yi[j] / Lj[j];
    for (int k = tid; k < j; k += 256) {
      yr[k] -= Lj[k] * xr;
      yi[k] -= Lj[k] * xi;
    }
    __syncthreads();
  }
  for (int k = tid; k < n; k += 256) {
    const double piv = M[(long long)k * ld + k];
    yr[k] /= piv;
    yi[k] /= piv;
  }
  __syncthreads();
  return true;
}

}  // namespace calk
