// gain_time_solve_kernels.hpp -- gains confined to a time basis, g[t] = g0[t] + sum_l Bt[t,l] z_l (z_l = B y_l with a frequency basis,
// y_l without one), in closed form (cal_solver_solve_gain_time_coeffs): the damped StefCal sweeps of gain_basis_solve_kernels.hpp taken
// jointly over the times.  The solver holds T times of Na antennas as one fit (row t Na + a is antenna a at time t), y is [Na][L][W]
// complex (W = kpad with a frequency basis, fpad without).  num, den are the per-row sums of gain_solve_ant_kernel from the OLD gains
// (autocorrelations left out), r[row][f] = num - den g, evaluated in double.
// With a frequency basis B [nfreqs][K] (n = L K, index l K + k), M_{t,a} = B^T diag(den_{t,a}) B as gain_basis_gram_kernel forms it:
//   N_a[(l,k),(l',k')] = sum_t Bt[t,l] Bt[t,l'] M_{t,a}[k,k']            rhs_a[(l,k)] = sum_t Bt[t,l] (B^T r_{t,a})[k]
//   (N_a + ridge (tr N_a / n) I) delta_a = rhs_a                          y_a <- y_a + damping delta_a
// Without one the system decouples per (antenna, channel), L x L each:
//   N_{a,f}[l,l'] = sum_t Bt[t,l] Bt[t,l'] den[t,a,f]                     rhs_{a,f}[l] = sum_t Bt[t,l] r[t,a,f]
//   (N_{a,f} + ridge (tr N_{a,f} / L) I) delta = rhs                      y[a][:][f] <- y[a][:][f] + damping delta
// Every system is solved from the old gains (a Jacobi sweep); the gains are rebuilt once per sweep.  A system with tr <= 0 (no unflagged
// cross-correlation at any time) or a pivot <= 0 or not finite keeps the bits of its y.  An antenna flagged at some times only IS solved
// and its gains at the flagged times move: the time basis interpolates.  T = 1, Bt = [[1]] gives the bits of
// cal_solver_solve_gain_coeffs; Bt = I, ridge = 0 is its sweep per time; damping = 1, ridge = 0 lands on the exact minimiser.
//   gain_time_kron_kernel   N_a (lower triangle) and rhs_a from the M_{t,a} and the per-row right-hand sides of gain_basis_gram_kernel
//   gain_basis_chol_kernel  (gain_basis_solve_kernels.hpp, at L blocks of K unknowns, no mask) per antenna, in double: normal_chol_solve
//                           of normal_solve.hpp, the damped update of y; the gain_time_chol_kernel that stood here merged into it
//   gain_time_chan_kernel   the case without a frequency basis: one thread per (antenna, channel), everything in double, on the
//                           per-thread system ChanSystem that gain_time_chan_var_kernel (gain_error_kernels.hpp) shares
// M_{t,a} and B^T r are in T; the sums over t run in double in ascending t and are rounded to T once on store; the factorisation, the
// substitutions and the update of y run in double, the update is rounded once.  Every sum of reals has a fixed order, atomics only on
// the two integer counters: two calls give the same bits.
#pragma once
#include "gain_basis_solve_kernels.hpp"
#include "gain_time_basis_kernels.hpp"

namespace calk {

// grid (ca * L, ceil(L / kTimeTile)): blockIdx.x = rel * L + l', blockIdx.y the tile of kTimeTile values of l; a tile wholly above the
// diagonal (l < l') has nothing to do.  M [T][ca][K][K] (only k' <= k stored: the element (k, k') with k < k' is read as M[k'][k], which
// the blocks l > l' need), rrhs [T Na][2][K] the per-row right-hand sides, Btb the zero-padded [T][lpad] copy of the time basis: the
// weights Bt[t,l] Bt[t,l'] depend on block and loop counters only and come through wave-uniform loads.  A thread owns a 16-byte piece
// along k' of one row k and the tile's accumulators in registers.  Output N [ca][n][n] (i >= j only) and rhs [ca][2][n], n = L K.
template <typename T>
__global__ __launch_bounds__(256) void gain_time_kron_kernel(const T* __restrict__ M, const T* __restrict__ rrhs, const T* __restrict__ Btb,
                                                              T* __restrict__ N, T* __restrict__ rhs, int a0, int ca, int na, int ntimes, int L,
                                                              int lpad, int K) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  typedef ns_vec_t<T> vec_t;
  const int rel = blockIdx.x / L, lc = blockIdx.x - rel * L;
  const int l0 = (int)blockIdx.y * kTimeTile;
  if (l0 + kTimeTile - 1 < lc) return;
  const int n = L * K;
  const int nq = (K + V - 1) / V;
  const bool vec = K % V == 0;  // rows of M and of N begin on 16-byte boundaries
  const long long kk2 = (long long)K * K;
  const T* __restrict__ Ma = M + (long long)rel * kk2;
  const long long tstride = (long long)ca * kk2;
  T* __restrict__ Na_ = N + (long long)rel * n * n;
  for (int item = threadIdx.x; item < K * nq; item += 256) {
    const int k = item / nq, c0 = (item - k * nq) * V;
    const bool lower = c0 + V - 1 <= k;  // the whole piece lies on or below the diagonal of M
    double acc[kTimeTile][V];
#pragma unroll
    for (int j = 0; j < kTimeTile; ++j)
#pragma unroll
      for (int x = 0; x < V; ++x) acc[j][x] = 0.0;
    for (int t = 0; t < ntimes; ++t) {
      const T* __restrict__ Mt = Ma + (long long)t * tstride;
      double m[V];
      if (vec && lower) {
        const vec_t v = *reinterpret_cast<const vec_t*>(Mt + (long long)k * K + c0);
#pragma unroll
        for (int x = 0; x < V; ++x) m[x] = (double)v[x];
      } else {
#pragma unroll
        for (int x = 0; x < V; ++x) {
          const int c = c0 + x;
          m[x] = c < K ? (double)(c <= k ? Mt[(long long)k * K + c] : Mt[(long long)c * K + k]) : 0.0;
        }
      }
      const T* __restrict__ b = Btb + (long long)t * lpad;
      const double bc = (double)b[lc];
#pragma unroll
      for (int j = 0; j < kTimeTile; ++j) {
        const double w = (double)b[l0 + j] * bc;
#pragma unroll
        for (int x = 0; x < V; ++x) acc[j][x] = acc[j][x] + w * m[x];
      }
    }
#pragma unroll
    for (int j = 0; j < kTimeTile; ++j) {
      const int l = l0 + j;
      if (l >= L || l < lc) continue;
      T* __restrict__ dst = Na_ + (long long)(l * K + k) * n + (long long)lc * K + c0;
      if (vec && (l > lc || lower)) {
        vec_t v;
#pragma unroll
        for (int x = 0; x < V; ++x) v[x] = (T)acc[j][x];
        *reinterpret_cast<vec_t*>(dst) = v;
      } else {
#pragma unroll
        for (int x = 0; x < V; ++x)
          if (c0 + x < K && (l > lc || c0 + x <= k)) dst[x] = (T)acc[j][x];
      }
    }
  }
  if (lc != 0) return;
  // the blocks of column l' = 0 also contract the per-row right-hand sides: rhs_a[c][l K + k] = sum_t Bt[t,l] rrhs[t Na + a][c][k]
  for (int item = threadIdx.x; item < 2 * K; item += 256) {
    double acc[kTimeTile];
#pragma unroll
    for (int j = 0; j < kTimeTile; ++j) acc[j] = 0.0;
    for (int t = 0; t < ntimes; ++t) {
      const double r = (double)rrhs[((long long)t * na + a0 + rel) * 2 * K + item];
      const T* __restrict__ b = Btb + (long long)t * lpad + l0;
#pragma unroll
      for (int j = 0; j < kTimeTile; ++j) acc[j] = acc[j] + (double)b[j] * r;
    }
    const int c = item / K, k = item - c * K;
#pragma unroll
    for (int j = 0; j < kTimeTile; ++j)
      if (l0 + j < L) rhs[((long long)rel * 2 + c) * n + (long long)(l0 + j) * K + k] = (T)acc[j];
  }
}

// The L x L system of one thread, N[l,l'] = sum_t Bt[t,l] Bt[t,l'] den[t], as gain_time_chan_kernel solves it and
// gain_time_chan_var_kernel (gain_error_kernels.hpp) inverts it: the lower triangle (element i (i + 1) / 2 + j) in doubles, registers
// for LT > 0 (L <= LT, every loop unrolled over LT and cut at L), for LT = 0 the chunk's scratch laid out [element][system] (slot e of
// system sys at scr[e nsys + sys]; the slots from L (L + 1) / 2 on are the kernel's own).  Every sum has the order it is written in:
// the contraction pragma holds for the compound statement it stands in, so every body here carries its own.  The accumulation and the
// factorisation come a row and a column at a time: the kernels keep the loops over them (unrolled over LT, cut at L) and put what is
// theirs -- the solve's right-hand sides -- beside the call.  (A helper holding those loops itself, with a hook per column, costs the
// register instances a wave per SIMD: 174 VGPRs against 132 / 148.)
template <int LT>
struct ChanSystem {
  static constexpr int LB = LT > 0 ? LT : 1;
  double reg[LB * (LB + 1) / 2];
  double* __restrict__ scr;
  long long nsys, sys;
  int L;
  __device__ __forceinline__ ChanSystem(double* __restrict__ scr_, long long nsys_, long long sys_, int L_) : scr(scr_), nsys(nsys_), sys(sys_), L(L_) {}
  __device__ __forceinline__ int lim() const { return LT > 0 ? LT : L; }  // the loops' bound: a constant in the register instance
  __device__ __forceinline__ double& slot(int e) { return scr[(long long)e * nsys + sys]; }
  __device__ __forceinline__ double& at(int i, int j) {
    if constexpr (LT > 0) return reg[i * (i + 1) / 2 + j];
    else return slot(i * (i + 1) / 2 + j);
  }
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < lim(); ++i) {
      if (i >= L) break;
#pragma unroll
      for (int j = 0; j <= i; ++j) at(i, j) = 0.0;
    }
  }
  // row i of one time's term Bt[t,i] Bt[t,j] den, j <= i: b the row Bt[t,:] of the padded basis copy
  template <typename T>
  __device__ __forceinline__ void accumulate_row(int i, const T* __restrict__ b, double den) {
#pragma clang fp contract(off)
    const double bi = (double)b[i];
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      const double w = bi * (double)b[j];
      at(i, j) = at(i, j) + w * den;
    }
  }
  __device__ __forceinline__ double trace() {
#pragma clang fp contract(off)
    double tr = 0.0;
#pragma unroll
    for (int i = 0; i < lim(); ++i) {
      if (i >= L) break;
      tr += at(i, i);
    }
    return tr;
  }
  // Column j of the left-looking Cholesky of N + shift I, in place, the columns before it done: row j of the factor is final behind
  // it, so a caller's right-hand sides can ride along.  Returns the pivot's root; ok stays true while every pivot is > 0 and finite
  // (a failed pivot divides by 1 and the factor is not to be used).
  __device__ __forceinline__ double factor_column(int j, double shift, bool& ok) {
#pragma clang fp contract(off)
    double d = at(j, j) + shift;
#pragma unroll
    for (int k = 0; k < j; ++k) d -= at(j, k) * at(j, k);
    ok = ok && d > 0.0 && isfinite(d);
    const double root = sqrt(ok ? d : 1.0);
    at(j, j) = root;
#pragma unroll
    for (int i = j + 1; i < lim(); ++i) {
      if (i >= L) break;
      double s = at(i, j);
#pragma unroll
      for (int k = 0; k < j; ++k) s -= at(i, k) * at(j, k);
      at(i, j) = s / root;
    }
    return root;
  }
};

// The case without a frequency basis: one thread per (antenna of the chunk, channel), consecutive lanes on consecutive channels.  The
// system is a ChanSystem; its two right-hand sides are doubles beside it: registers for LT > 0, for LT = 0 the 2 L slots of the
// chunk's scratch behind the triangle's, nsys = ca nfreqs.
// planes: num_r, num_i, den as [3][T Na][nfreqs] doubles; gains [T Na][fpad]; Btb [T][lpad]; y [Na][L][fpad].  Cholesky and both
// substitutions in place; a singular system keeps the bits of y[a][:][f].  One atomic per wave and counter.
template <typename T, int LT>
__global__ __launch_bounds__(256) void gain_time_chan_kernel(const double* __restrict__ planes, const vec2_t<T>* __restrict__ gains,
                                                              const T* __restrict__ Btb, vec2_t<T>* __restrict__ y, double* __restrict__ scr, int a0,
                                                              int ca, int na, int ntimes, int L, int lpad, int nfreqs, int fpad, double damping,
                                                              double ridge, int* __restrict__ counts) {
#pragma clang fp contract(off)
  constexpr int LB = LT > 0 ? LT : 1;
  double rr[LB], ri[LB];
  const long long sys = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long nsys = (long long)ca * nfreqs;
  const bool live = sys < nsys;
  const int lim = LT > 0 ? LT : L;  // the loops' bound: a constant in the register instance
  const int ntri = L * (L + 1) / 2;
  ChanSystem<LT> A(scr, nsys, sys, L);
  auto Br = [&](int l) -> double& {
    if constexpr (LT > 0) return rr[l];
    else return A.slot(ntri + l);
  };
  auto Bi = [&](int l) -> double& {
    if constexpr (LT > 0) return ri[l];
    else return A.slot(ntri + L + l);
  };
  bool ok = live;
  if (live) {
    const int rel = (int)(sys / nfreqs), f = (int)(sys - (long long)rel * nfreqs);
    const int a = a0 + rel;
    const long long plane = (long long)ntimes * na * nfreqs;
    A.zero();
#pragma unroll
    for (int i = 0; i < lim; ++i) {
      if (i >= L) break;
      Br(i) = 0.0;
      Bi(i) = 0.0;
    }
    for (int t = 0; t < ntimes; ++t) {
      const long long row = (long long)t * na + a;
      const double den = planes[2 * plane + row * nfreqs + f];
      const vec2_t<T> g = gains[row * fpad + f];
      const double r_r = planes[row * nfreqs + f] - den * (double)g.x;
      const double r_i = planes[plane + row * nfreqs + f] - den * (double)g.y;
      const T* __restrict__ b = Btb + (long long)t * lpad;
#pragma unroll
      for (int i = 0; i < lim; ++i) {
        if (i >= L) break;
        const double bi = (double)b[i];
        A.accumulate_row(i, b, den);
        Br(i) = Br(i) + bi * r_r;
        Bi(i) = Bi(i) + bi * r_i;
      }
    }
    const double tr = A.trace();
    ok = tr > 0.0 && isfinite(tr);
    const double shift = ok ? ridge * (tr / L) : 0.0;
    // left-looking Cholesky by columns; the right-hand sides ride along (the forward substitution)
#pragma unroll
    for (int j = 0; j < lim; ++j) {
      if (j >= L) break;
      const double root = A.factor_column(j, shift, ok);
      double sr = Br(j), si = Bi(j);
#pragma unroll
      for (int k = 0; k < j; ++k) {
        sr -= A.at(j, k) * Br(k);
        si -= A.at(j, k) * Bi(k);
      }
      Br(j) = sr / root;
      Bi(j) = si / root;
    }
    // L^T x = z
#pragma unroll
    for (int jj = 0; jj < lim; ++jj) {
      const int j = lim - 1 - jj;
      if (j >= L) continue;
      double sr = Br(j), si = Bi(j);
#pragma unroll
      for (int k = j + 1; k < lim; ++k) {
        if (k >= L) break;
        sr -= A.at(k, j) * Br(k);
        si -= A.at(k, j) * Bi(k);
      }
      Br(j) = sr / A.at(j, j);
      Bi(j) = si / A.at(j, j);
    }
    if (ok) {
      vec2_t<T>* __restrict__ ya = y + (long long)a * L * fpad + f;
#pragma unroll
      for (int l = 0; l < lim; ++l) {
        if (l >= L) break;
        const vec2_t<T> old = ya[(long long)l * fpad];
        vec2_t<T> out;
        out.x = (T)((double)old.x + damping * Br(l));
        out.y = (T)((double)old.y + damping * Bi(l));
        ya[(long long)l * fpad] = out;
      }
    }
  }
  const int nok = __popcll(__ballot(live && ok)), nbad = __popcll(__ballot(live && !ok));
  if ((threadIdx.x & 63) == 0) {
    if (nok) atomicAdd(counts, nok);
    if (nbad) atomicAdd(counts + 1, nbad);
  }
}

}  // namespace calk
