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
//   gain_time_chol_kernel   per antenna, in double: normal_chol_solve of normal_solve.hpp, the damped update of y
//   gain_time_chan_kernel   the case without a frequency basis: one thread per (antenna, channel), everything in double
// M_{t,a} and B^T r are in T; the sums over t run in double in ascending t and are rounded to T once on store; the factorisation, the
// substitutions and the update of y run in double, the update is rounded once.  Every sum of reals has a fixed order, atomics only on
// the two integer counters: two calls give the same bits.
#pragma once
#include "gain_time_basis_kernels.hpp"
#include "normal_solve.hpp"

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

// One workgroup per antenna of the chunk: normal_chol_solve on the antenna's N_a and rhs_a (n = L K), its [n + 2][ld] matrix in LDS when
// it fits `lds_doubles` and in the chunk's scratch otherwise.  A singular antenna leaves its y alone and counts in counts[1]; a solved
// one counts in counts[0].  The update y[a][l][k] + damping delta[l K + k] (rows of y at pitch kpad) is rounded to T once.
template <typename T>
__global__ __launch_bounds__(256) void gain_time_chol_kernel(const T* __restrict__ nmat, const T* __restrict__ rhs, double* __restrict__ dscr,
                                                              vec2_t<T>* __restrict__ y, int a0, int L, int K, int kpad, double damping, double ridge,
                                                              int* __restrict__ counts, int lds_doubles) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double s_m[];
  __shared__ double s_red[256];
  const int rel = blockIdx.x;
  const int a = a0 + rel;
  const int tid = threadIdx.x;
  const int n = L * K;
  const bool in_lds = (long long)(n + 2) * (n | 1) <= lds_doubles;
  const int ld = in_lds ? (n | 1) : n;
  double* Mx = in_lds ? s_m : dscr + (long long)rel * (n + 2) * n;
  const T* __restrict__ ra = rhs + (long long)rel * 2 * n;
  if (!normal_chol_solve(Mx, ld, n, nmat + (long long)rel * n * n, ra, ra + n, ridge, s_red)) {
    if (tid == 0) atomicAdd(counts + 1, 1);
    return;
  }
  const double* xr = Mx + (long long)n * ld;
  const double* xi = Mx + (long long)(n + 1) * ld;
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

// The case without a frequency basis: one thread per (antenna of the chunk, channel), consecutive lanes on consecutive channels.  The
// lower triangle (element i (i + 1) / 2 + j) and the two right-hand sides of the L x L system are doubles: registers for LT > 0
// (L <= LT, every loop unrolled over LT and cut at L), for LT = 0 the chunk's scratch laid out [element][system], nsys = ca nfreqs.
// planes: num_r, num_i, den as [3][T Na][nfreqs] doubles; gains [T Na][fpad]; Btb [T][lpad]; y [Na][L][fpad].  Cholesky and both
// substitutions in place; a singular system keeps the bits of y[a][:][f].  One atomic per wave and counter.
template <typename T, int LT>
__global__ __launch_bounds__(256) void gain_time_chan_kernel(const double* __restrict__ planes, const vec2_t<T>* __restrict__ gains,
                                                              const T* __restrict__ Btb, vec2_t<T>* __restrict__ y, double* __restrict__ scr, int a0,
                                                              int ca, int na, int ntimes, int L, int lpad, int nfreqs, int fpad, double damping,
                                                              double ridge, int* __restrict__ counts) {
#pragma clang fp contract(off)
  constexpr int LB = LT > 0 ? LT : 1;
  constexpr int NE = LB * (LB + 1) / 2;
  double ra[NE], rr[LB], ri[LB];
  const long long sys = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long nsys = (long long)ca * nfreqs;
  const bool live = sys < nsys;
  const int lim = LT > 0 ? LT : L;  // the loops' bound: a constant in the register instance
  const int ntri = L * (L + 1) / 2;
  auto A = [&](int e) -> double& {
    if constexpr (LT > 0) return ra[e];
    else return scr[(long long)e * nsys + sys];
  };
  auto Br = [&](int l) -> double& {
    if constexpr (LT > 0) return rr[l];
    else return scr[(long long)(ntri + l) * nsys + sys];
  };
  auto Bi = [&](int l) -> double& {
    if constexpr (LT > 0) return ri[l];
    else return scr[(long long)(ntri + L + l) * nsys + sys];
  };
  bool ok = live;
  if (live) {
    const int rel = (int)(sys / nfreqs), f = (int)(sys - (long long)rel * nfreqs);
    const int a = a0 + rel;
    const long long plane = (long long)ntimes * na * nfreqs;
#pragma unroll
    for (int i = 0; i < lim; ++i) {
      if (i >= L) break;
#pragma unroll
      for (int j = 0; j <= i; ++j) A(i * (i + 1) / 2 + j) = 0.0;
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
#pragma unroll
        for (int j = 0; j <= i; ++j) {
          const double w = bi * (double)b[j];
          A(i * (i + 1) / 2 + j) = A(i * (i + 1) / 2 + j) + w * den;
        }
        Br(i) = Br(i) + bi * r_r;
        Bi(i) = Bi(i) + bi * r_i;
      }
    }
    double tr = 0.0;
#pragma unroll
    for (int i = 0; i < lim; ++i) {
      if (i >= L) break;
      tr += A(i * (i + 1) / 2 + i);
    }
    ok = tr > 0.0 && isfinite(tr);
    const double shift = ok ? ridge * (tr / L) : 0.0;
    // left-looking Cholesky by columns; the right-hand sides ride along (the forward substitution)
#pragma unroll
    for (int j = 0; j < lim; ++j) {
      if (j >= L) break;
      double d = A(j * (j + 1) / 2 + j) + shift;
#pragma unroll
      for (int k = 0; k < j; ++k) d -= A(j * (j + 1) / 2 + k) * A(j * (j + 1) / 2 + k);
      ok = ok && d > 0.0 && isfinite(d);
      const double root = sqrt(ok ? d : 1.0);
      A(j * (j + 1) / 2 + j) = root;
#pragma unroll
      for (int i = j + 1; i < lim; ++i) {
        if (i >= L) break;
        double s = A(i * (i + 1) / 2 + j);
#pragma unroll
        for (int k = 0; k < j; ++k) s -= A(i * (i + 1) / 2 + k) * A(j * (j + 1) / 2 + k);
        A(i * (i + 1) / 2 + j) = s / root;
      }
      double sr = Br(j), si = Bi(j);
#pragma unroll
      for (int k = 0; k < j; ++k) {
        sr -= A(j * (j + 1) / 2 + k) * Br(k);
        si -= A(j * (j + 1) / 2 + k) * Bi(k);
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
        sr -= A(k * (k + 1) / 2 + j) * Br(k);
        si -= A(k * (k + 1) / 2 + j) * Bi(k);
      }
      Br(j) = sr / A(j * (j + 1) / 2 + j);
      Bi(j) = si / A(j * (j + 1) / 2 + j);
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
