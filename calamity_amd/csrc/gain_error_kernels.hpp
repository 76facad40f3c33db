// gain_error_kernels.hpp -- the error bars of gains confined to a basis (cal_solver_gain_basis_errors): the inverse of the projected
// curvature matrix the closed-form sweeps of gain_basis_solve_kernels.hpp and gain_time_solve_kernels.hpp build and throw away.  In
// their notation (den of gain_solve_ant_kernel, autocorrelations left out; shift = ridge tr N / n), conditional on the other antennas
// and the model like gain_var of fit_error_kernels.hpp, which B = I reproduces (1 / den):
//   frequency basis B [F][K], per antenna row a, n = K:
//     N_a = B^T diag(den_a) B     N_r = N_a + shift I     L L^T = N_r     W = L^-1
//     y_var[a][k]    = sum_i W[i][k]^2                          (variance of the complex y_k)
//     gain_var[a][f] = |W b_f|^2 = b_f^T N_r^-1 b_f             (b_f: row f of B), every f < nfreqs: the basis interpolates
//     gain_dof[a]    = n - shift sum_k y_var[a][k]              (= tr(N_a N_r^-1): complex parameters spent)
//   time x frequency basis Bt [T][L], per antenna a, n = L K, index l K + k, N_a as gain_time_kron_kernel forms it:
//     gain_var[t Na + a][f] = |W (Bt[t,:] (x) b_f)|^2           y_var[a][l][k] = sum_i W[i][l K + k]^2      gain_dof[a] as above
//   time basis alone, per (antenna, channel), L x L:
//     N_{a,f}[l,l'] = sum_t Bt[t,l] Bt[t,l'] den[t,a,f]         y_var[a][l][f] = (N_r^-1)[l][l]
//     gain_var[t Na + a][f] = Bt[t,:] N_r^-1 Bt[t,:]^T          gain_dof[a] = sum over the solved f of (L - shift_f sum_l y_var[a][l][f])
// Behind gain_solve_ant_kernel, gain_basis_gram_kernel and gain_time_kron_kernel, all as they are:
//   gain_error_factor_kernel      per row of the chunk, in double: the shared Cholesky and W = L^-1 (normal_solve.hpp), y_var, gain_dof;
//                                 W rounded to T once into the chunk's scratch, padded to whole 16 x 16 tiles
//   gain_error_var_kernel         per (row of gain_var, 64 channels): Z = W X on the matrix cores (fe_sumsq of fit_error_kernels.hpp),
//                                 X the rows of the transposed basis copy, times Bt[t,l] with a time basis: the Kronecker row, never stored
//   gain_time_chan_var_kernel     the time basis alone: one thread per (antenna, channel), everything in double, on the per-thread
//                                 system of gain_time_chan_kernel (ChanSystem, gain_time_solve_kernels.hpp)
//   gain_error_dof_kernel         the time basis alone: the channels' dof added in channel order
// A system that is singular by the shared tests (tr <= 0, a pivot <= 0, or not finite) leaves the zeros the host wrote in all its
// outputs and counts in counts[1]; a solved one counts in counts[0].  Every sum of reals has a fixed order, atomics only on the two
// integer counters: two calls give the same bits.
#pragma once
#include "fit_error_kernels.hpp"
#include "gain_time_solve_kernels.hpp"

namespace calk {

// One workgroup per row of the chunk (an antenna row; with a time basis an antenna): nmat [rel][n][n] T (i >= j), the factor
// M ([n + 1][ld] doubles: L, then a spare row) in LDS when [n + 2][ld] fits `lds_doubles` (the bound of
// gain_basis_chol_kernel, so that both take the same branch) and in the chunk's double scratch dscr [rel][n + 2][n] otherwise.  Output:
// wmat [rel][np][np] T, np = fe_pad(n); y_var [a][n] and gain_dof [a] (either may be null), ok[a] = 1.
template <typename T>
__global__ __launch_bounds__(256) void gain_error_factor_kernel(const T* __restrict__ nmat, double* __restrict__ dscr, T* __restrict__ wmat,
                                                                 double* __restrict__ y_var, double* __restrict__ gain_dof, int* __restrict__ ok,
                                                                 int a0, int n, double ridge, int* __restrict__ counts, int lds_doubles) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double s_m[];
  __shared__ double s_red[256];
  const int rel = blockIdx.x;
  const int a = a0 + rel;
  const int tid = threadIdx.x;
  const bool in_lds = (long long)(n + 2) * (n | 1) <= lds_doubles;
  const int ld = in_lds ? (n | 1) : n;
  double* M = in_lds ? s_m : dscr + (long long)rel * (n + 2) * n;
  if (!normal_chol_load(M, ld, n, nmat + (long long)rel * n * n, ridge, s_red) || !normal_chol_factor(M, ld, n, n)) {
    if (tid == 0) atomicAdd(counts + 1, 1);
    return;
  }
  const double shift = ridge * (s_red[0] / n);  // normal_chol_load has left tr N there
  normal_chol_invert(M, ld, n);
  double* spare = M + (long long)n * ld;
  for (int k = tid; k < n; k += 256) {
    double s = 0;
    for (int i = k; i < n; ++i) {
      const double v = M[(long long)i * ld + k];
      s += v * v;
    }
    spare[k] = s;
    if (y_var) y_var[(long long)a * n + k] = s;
  }
  const int np = fe_pad(n);
  T* __restrict__ Wg = wmat + (long long)rel * np * np;
  for (int idx = tid; idx < np * np; idx += 256) {
    const int i = idx / np, k = idx - i * np;
    Wg[idx] = (i < n && k <= i) ? (T)M[(long long)i * ld + k] : (T)0;
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0;
    for (int k = 0; k < n; ++k) s += spare[k];
    if (gain_dof) gain_dof[a] = (double)n - shift * s;
    ok[a] = 1;
    atomicAdd(counts, 1);
  }
}

// grid (rows of gain_var in the chunk * npieces): blockIdx.x = (t ca + rel) * npieces + piece with ntimes = 1, t = 0 without a time
// basis (Btb null).  Row t na + a0 + rel of gain_var takes |W x_f|^2 for the piece's 64 channels, W = wmat[rel] ([np][np], np =
// fe_pad(L K)), x_f[l K + k] = Btb[t][l] Bt[k][f]: Bt the zero-padded [kpad][fpad] transposed copy of the frequency basis, so whole
// 16-byte pieces inside fpad are read unconditionally; Btb the zero-padded [T][lpad] copy of the time basis.  Channels >= nfreqs are
// computed (zeros, or the padding's) and not written.
template <typename T>
__global__ __launch_bounds__(256) void gain_error_var_kernel(const T* __restrict__ wmat, const T* __restrict__ Bt, const T* __restrict__ Btb,
                                                              const int* __restrict__ ok, double* __restrict__ gain_var, int a0, int ca, int na,
                                                              int L, int lpad, int K, int nfreqs, int fpad, int npieces) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  typedef ns_vec_t<T> vec_t;
  __shared__ __attribute__((aligned(16))) T s_w[kNsBlock][kNsPitch];
  __shared__ __attribute__((aligned(16))) T s_at[kNsChunk][kFePitch];
  __shared__ double s_sq[16][kFePiece];  // [wave * 4 + lane quarter][channel]
  const int rowc = blockIdx.x / npieces, piece = blockIdx.x - rowc * npieces;
  const int t = rowc / ca, rel = rowc - t * ca;
  const int a = a0 + rel;
  if (!ok[a]) return;  // the same for the whole block
  const int n = L * K, np = fe_pad(n);
  const int c0 = piece * kFePiece;
  const T* __restrict__ bt = Btb ? Btb + (long long)t * lpad : nullptr;
  const double mv = fe_sumsq<T>(wmat + (long long)rel * np * np, np, s_w, s_at, s_sq, [&](int i, int c) {
    vec_t v;
#pragma unroll
    for (int x = 0; x < V; ++x) v[x] = (T)0;
    // fpad is a multiple of 8: a piece is wholly inside the row or wholly outside
    if (i < n && c0 + c < fpad) {
      const int l = i / K, k = i - l * K;
      v = *reinterpret_cast<const vec_t*>(Bt + (long long)k * fpad + c0 + c);
      if (bt) {
        const T b = bt[l];
#pragma unroll
        for (int x = 0; x < V; ++x) v[x] *= b;
      }
    }
    return v;
  });
  const int f = c0 + (int)threadIdx.x;
  if (threadIdx.x < kFePiece && f < nfreqs) gain_var[((long long)t * na + a) * nfreqs + f] = mv;
}

// The case without a frequency basis: one thread per (antenna of the chunk, channel), consecutive lanes on consecutive channels, on
// the ChanSystem of gain_time_chan_kernel (gain_time_solve_kernels.hpp): registers for LT > 0, for LT = 0 the chunk's scratch laid out
// [element][system], nsys = ca nfreqs, the row the solve is planned with (its 2 L right-hand-side slots stay unused here).
// planes: num_r, num_i, den as [3][T Na][nfreqs] doubles (den alone is read); Btb [T][lpad].  Cholesky, then W = L^-1 in place, row
// by row in ascending column order (an element of row i is read as L only by the columns before it).  Output (each may be null):
// y_var [Na][L][nfreqs], gain_var [T Na][nfreqs], dof [Na][nfreqs] (L - shift sum_l y_var of a solved system; zero otherwise).
template <typename T, int LT>
__global__ __launch_bounds__(256) void gain_time_chan_var_kernel(const double* __restrict__ planes, const T* __restrict__ Btb,
                                                                  double* __restrict__ scr, double* __restrict__ y_var,
                                                                  double* __restrict__ gain_var, double* __restrict__ dof, int a0, int ca, int na,
                                                                  int ntimes, int L, int lpad, int nfreqs, double ridge,
                                                                  int* __restrict__ counts) {
#pragma clang fp contract(off)
  const long long sys = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long nsys = (long long)ca * nfreqs;
  const bool live = sys < nsys;
  const int lim = LT > 0 ? LT : L;  // the loops' bound: a constant in the register instance
  ChanSystem<LT> A(scr, nsys, sys, L);
  bool ok = live;
  if (live) {
    const int rel = (int)(sys / nfreqs), f = (int)(sys - (long long)rel * nfreqs);
    const int a = a0 + rel;
    const long long plane = (long long)ntimes * na * nfreqs;
    A.zero();
    for (int t = 0; t < ntimes; ++t) {
      const double den = planes[2 * plane + ((long long)t * na + a) * nfreqs + f];
      const T* __restrict__ b = Btb + (long long)t * lpad;
#pragma unroll
      for (int i = 0; i < lim; ++i) {
        if (i >= L) break;
        A.accumulate_row(i, b, den);
      }
    }
    const double tr = A.trace();
    ok = tr > 0.0 && isfinite(tr);
    const double shift = ok ? ridge * (tr / L) : 0.0;
    // left-looking Cholesky by columns
#pragma unroll
    for (int j = 0; j < lim; ++j) {
      if (j >= L) break;
      A.factor_column(j, shift, ok);
    }
    // W = L^-1 in place
#pragma unroll
    for (int i = 0; i < lim; ++i) {
      if (i >= L) break;
      const double piv = A.at(i, i);
#pragma unroll
      for (int k = 0; k <= i; ++k) {
        double s = k == i ? 1.0 : 0.0;
#pragma unroll
        for (int j = k; j < i; ++j) s -= A.at(i, j) * A.at(j, k);
        A.at(i, k) = s / piv;
      }
    }
    if (ok) {
      double sum = 0.0;
#pragma unroll
      for (int l = 0; l < lim; ++l) {
        if (l >= L) break;
        double s = 0.0;
#pragma unroll
        for (int i = l; i < lim; ++i) {
          if (i >= L) break;
          s += A.at(i, l) * A.at(i, l);
        }
        sum += s;
        if (y_var) y_var[((long long)a * L + l) * nfreqs + f] = s;
      }
      if (dof) dof[(long long)a * nfreqs + f] = (double)L - shift * sum;
      if (gain_var) {
        for (int t = 0; t < ntimes; ++t) {
          const T* __restrict__ b = Btb + (long long)t * lpad;
          double v = 0.0;
#pragma unroll
          for (int i = 0; i < lim; ++i) {
            if (i >= L) break;
            double z = 0.0;
#pragma unroll
            for (int l = 0; l <= i; ++l) z += A.at(i, l) * (double)b[l];
            v += z * z;
          }
          gain_var[((long long)t * na + a) * nfreqs + f] = v;
        }
      }
    }
  }
  const int nok = __popcll(__ballot(live && ok)), nbad = __popcll(__ballot(live && !ok));
  if ((threadIdx.x & 63) == 0) {
    if (nok) atomicAdd(counts, nok);
    if (nbad) atomicAdd(counts + 1, nbad);
  }
}

// One thread per antenna: gain_dof[a] = the channels' dof in channel order (the time basis alone).
__global__ __launch_bounds__(256) void gain_error_dof_kernel(const double* __restrict__ dof, double* __restrict__ gain_dof, int na, int nfreqs) {
#pragma clang fp contract(off)
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= na) return;
  double s = 0.0;
  for (int f = 0; f < nfreqs; ++f) s += dof[(long long)a * nfreqs + f];
  gain_dof[a] = s;
}

}  // namespace calk
