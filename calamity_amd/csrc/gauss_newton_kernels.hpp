// gauss_newton_kernels.hpp -- joint Gauss-Newton steps over gains and coefficients (cal_solver_normal_product,
// cal_solver_gauss_newton_step).  Baseline row b has antennas (i, j); d, w are the data and weights, g the gains, m = A c, G = g_i conj(g_j).
// A direction p = (dg [nants][nfreqs], dc [ncoef]) is complex, held as (re, im) like the parameters.
//   (J p)[b][f] = (dg_i conj(g_j) + g_i conj(dg_j)) m + G (A dc)
//   N p = J^H W J p = -1/2 (grad(G m + s_t J p) - grad(G m)) / s_t        s_t = sqrt(sum w |G m|^2 / sum w |J p|^2) per slice
//   rhs = J^H W r   = -1/2 (grad(d) - grad(G m))
// grad(d') is the solver's own gradient pass run on substituted data planes; A dc is its model pass run on substituted coefficients.
// The kernels here are what sits between those passes:
//   gn_tangent_rows_kernel   J p over the two planes of A dc, and per row sum w |G m|^2, sum w |J p|^2 in double
//   gn_scale_kernel          s_t from the rows' sums, in row order over the slice's rows
//   gn_data_kernel           G m + s_t J p (or G m alone) into the two data planes
//   gn_precond_*             D_g = den of cal_solver_solve_gains, D_c = per group sum_b mean_f w |G|^2; entries <= 0 or non-finite: 1
//   gn_diff_kernel .. gn_update2_kernel   conjugate gradients preconditioned with D on (N + lambda_t D) p = rhs, per slice
//   gn_apply_kernel          the trial parameters of the selected slices
// The parameter space is one flat vector: the gains [nants][fpad] (re, im) interleaved, then the coefficient planes [2][ncoef] at
// element `go`.  Slice t owns gain reals [t ng, (t + 1) ng), ng = 2 na_slice fpad, and coefficients [coff[t], coff[t + 1]) of both planes.
// Vector storage: the direction s handed to the passes, the saved gradient of G m and the saved parameters are in T; the solution x, the
// residual, N s and D are double.  Every sum of reals runs in double in a fixed order (per thread ascending, a butterfly over the wave,
// the waves and then the blocks in ascending order): no atomics, two calls give the same bits.  The per-slice scalars live on the device.
#pragma once
#include "row_walk.hpp"

namespace calk {

constexpr int kGnBlocks = 128;  // blocks per slice of the vector kernels: the first stage of every dot product

struct GnScal {  // per slice
  double rz, rz0, alpha, beta, scale, lambda, resid, tol;
  int frozen, iters;
};
struct GnSpace {
  const int* coff;  // [nslices + 1]
  int na_slice, nfreqs, fpad, ncoef;
  long long go;     // 2 nants fpad: where the coefficient planes begin
};
struct GnGroup { int b0, b1, coff, nvec; };

__device__ __forceinline__ long long gn_slice_len(const GnSpace& S, int t) {
  return 2ll * S.na_slice * S.fpad + 2ll * (S.coff[t + 1] - S.coff[t]);
}
// flat index of element e of slice t; live: not a padding channel
__device__ __forceinline__ long long gn_index(const GnSpace& S, int t, long long e, bool& live) {
  const long long ng = 2ll * S.na_slice * S.fpad;
  if (e < ng) {
    live = (int)((e >> 1) % S.fpad) < S.nfreqs;
    return (long long)t * ng + e;
  }
  const long long k = e - ng;
  const int nc = S.coff[t + 1] - S.coff[t];
  const int plane = k >= nc ? 1 : 0;
  live = true;
  return S.go + (long long)plane * S.ncoef + S.coff[t] + (k - (long long)plane * nc);
}
// the block's sum (256 threads) in thread 0
__device__ __forceinline__ double gn_block_sum(double v, double* s_w) {
  v = ldsum(v);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  return s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// One wave per baseline row, four rows per block, 16-byte loads (the shape of gain_solve_rows_kernel).  t_r, t_i hold A dc and
// receive J p; channels [nfreqs, fpad) write zeros.  row_sums[2 b] = sum_f w |G m|^2, row_sums[2 b + 1] = sum_f w |J p|^2.
template <typename T>
__global__ __launch_bounds__(256) void gn_tangent_rows_kernel(const T* __restrict__ m_r, const T* __restrict__ m_i, T* __restrict__ t_r,
                                                               T* __restrict__ t_i, const vec2_t<T>* __restrict__ gains,
                                                               const vec2_t<T>* __restrict__ dgains, const T* __restrict__ wgts,
                                                               const int2* __restrict__ bl_ant, int nbls, int nfreqs, int fpad,
                                                               double* __restrict__ row_sums) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
  if (b >= nbls) return;
  const int2 ant = bl_ant[b];
  const long long row = (long long)b * fpad;
  const vec2_t<T>* __restrict__ gi = gains + (long long)ant.x * fpad;
  const vec2_t<T>* __restrict__ gj = gains + (long long)ant.y * fpad;
  const vec2_t<T>* __restrict__ di = dgains + (long long)ant.x * fpad;
  const vec2_t<T>* __restrict__ dj = dgains + (long long)ant.y * fpad;
  double sum_m = 0, sum_j = 0;
  for (int f = lane * V; f < fpad; f += 64 * V) {  // fpad is a multiple of 8: whole vectors
    const vec_t mr = *reinterpret_cast<const vec_t*>(m_r + row + f);
    const vec_t mi = *reinterpret_cast<const vec_t*>(m_i + row + f);
    const vec_t tr = *reinterpret_cast<const vec_t*>(t_r + row + f);
    const vec_t ti = *reinterpret_cast<const vec_t*>(t_i + row + f);
    const vec_t w = *reinterpret_cast<const vec_t*>(wgts + row + f);
    vec_t a2[2], b2[2], da2[2], db2[2];  // V channels of (re, im)
    a2[0] = *reinterpret_cast<const vec_t*>(gi + f);
    a2[1] = *reinterpret_cast<const vec_t*>(gi + f + V / 2);
    b2[0] = *reinterpret_cast<const vec_t*>(gj + f);
    b2[1] = *reinterpret_cast<const vec_t*>(gj + f + V / 2);
    da2[0] = *reinterpret_cast<const vec_t*>(di + f);
    da2[1] = *reinterpret_cast<const vec_t*>(di + f + V / 2);
    db2[0] = *reinterpret_cast<const vec_t*>(dj + f);
    db2[1] = *reinterpret_cast<const vec_t*>(dj + f + V / 2);
    vec_t jr, ji;
#pragma unroll
    for (int c = 0; c < V; ++c) {
      const T ax = a2[(2 * c) / V][(2 * c) % V], ay = a2[(2 * c) / V][(2 * c) % V + 1];
      const T bx = b2[(2 * c) / V][(2 * c) % V], by = b2[(2 * c) / V][(2 * c) % V + 1];
      const T dax = da2[(2 * c) / V][(2 * c) % V], day = da2[(2 * c) / V][(2 * c) % V + 1];
      const T dbx = db2[(2 * c) / V][(2 * c) % V], dby = db2[(2 * c) / V][(2 * c) % V + 1];
      const T Gr = ax * bx + ay * by, Gi = ay * bx - ax * by;  // g_i conj(g_j)
      const T Hr = (dax * bx + day * by) + (ax * dbx + ay * dby);  // dg_i conj(g_j) + g_i conj(dg_j)
      const T Hi = (day * bx - dax * by) + (ay * dbx - ax * dby);
      const T gmr = Gr * mr[c] - Gi * mi[c], gmi = Gr * mi[c] + Gi * mr[c];
      const T pr = (Hr * mr[c] - Hi * mi[c]) + (Gr * tr[c] - Gi * ti[c]);
      const T pi = (Hr * mi[c] + Hi * mr[c]) + (Gr * ti[c] + Gi * tr[c]);
      const bool live = f + c < nfreqs;
      jr[c] = live ? pr : (T)0;
      ji[c] = live ? pi : (T)0;
      if (live) {
        sum_m += (double)w[c] * ((double)gmr * (double)gmr + (double)gmi * (double)gmi);
        sum_j += (double)w[c] * ((double)pr * (double)pr + (double)pi * (double)pi);
      }
    }
    *reinterpret_cast<vec_t*>(t_r + row + f) = jr;
    *reinterpret_cast<vec_t*>(t_i + row + f) = ji;
  }
  sum_m = ldsum(sum_m);
  sum_j = ldsum(sum_j);
  if (lane == 0) {
    row_sums[2 * (long long)b] = sum_m;
    row_sums[2 * (long long)b + 1] = sum_j;
  }
}

// One block per slice: the slice's rows [row_ptr[t], row_ptr[t + 1]) are cut into 256 runs, thread k adds run k in row order, thread 0 the
// 256 runs in order (the cut depends on the slice's own row count only: a slice gives the same bits in whatever batch it sits).
// scale = sqrt(sum w |G m|^2 / sum w |J p|^2), 1 where either sum is 0 (or the ratio is not a finite positive number).
__global__ __launch_bounds__(256) void gn_scale_kernel(const double* __restrict__ row_sums, const int* __restrict__ row_ptr, GnScal* __restrict__ scal) {
  __shared__ double s_a[256], s_b[256];
  const int t = blockIdx.x;
  const int r0 = row_ptr[t], r1 = row_ptr[t + 1];
  const int per = (r1 - r0 + 255) / 256;
  const int b0 = min(r1, r0 + (int)threadIdx.x * per), b1 = min(r1, b0 + per);
  double a = 0, b = 0;
  for (int r = b0; r < b1; ++r) {
    a += row_sums[2 * (long long)r];
    b += row_sums[2 * (long long)r + 1];
  }
  s_a[threadIdx.x] = a;
  s_b[threadIdx.x] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    a = b = 0;
    for (int k = 0; k < 256; ++k) {
      a += s_a[k];
      b += s_b[k];
    }
    const double s = sqrt(a / b);
    scal[t].scale = (a > 0.0 && b > 0.0 && isfinite(s) && s > 0.0) ? s : 1.0;
  }
}

// data = G m + s_t J p (jp_r == nullptr: G m alone, the same bits of G m); the padding [nfreqs, fpad) stays zero.
template <typename T>
__global__ __launch_bounds__(256) void gn_data_kernel(const T* __restrict__ m_r, const T* __restrict__ m_i, const T* __restrict__ jp_r,
                                                       const T* __restrict__ jp_i, const vec2_t<T>* __restrict__ gains,
                                                       const int2* __restrict__ bl_ant, const GnScal* __restrict__ scal, int na_slice,
                                                       T* __restrict__ data_r, T* __restrict__ data_i, int nbls, int nfreqs, int fpad) {
#pragma clang fp contract(off)
  constexpr int V = RowWalk<T>::V;
  typedef typename RowWalk<T>::vec_t vec_t;
  RowWalk<T> R;
  if (!R.begin(bl_ant, nbls, fpad)) return;
  GainPair<T> gp(gains, R.ant, fpad);
  const T s = jp_r ? (T)scal[R.ant.x / na_slice].scale : (T)0;
  for (int f = R.lane * V; f < fpad; f += 64 * V) {
    const vec_t mr = R.load(m_r, f), mi = R.load(m_i, f);
    vec_t pr, pi;
    if (jp_r) {
      pr = R.load(jp_r, f);
      pi = R.load(jp_i, f);
    }
    gp.load(f);
    vec_t dr, di;
#pragma unroll
    for (int c = 0; c < V; ++c) {
      const auto g = gp.at(c);
      T xr = g.Gr * mr[c] - g.Gi * mi[c], xi = g.Gr * mi[c] + g.Gi * mr[c];
      if (jp_r) {
        xr = xr + s * pr[c];
        xi = xi + s * pi[c];
      }
      const bool live = f + c < nfreqs;
      dr[c] = live ? xr : (T)0;
      di[c] = live ? xi : (T)0;
    }
    R.store(data_r, f, dr);
    R.store(data_i, f, di);
  }
}

// One wave per baseline row: rowq[b] = (1 / nfreqs) sum_f w |G|^2 in double.
template <typename T>
__global__ __launch_bounds__(256) void gn_precond_rows_kernel(const vec2_t<T>* __restrict__ gains, const T* __restrict__ wgts,
                                                               const int2* __restrict__ bl_ant, int nbls, int nfreqs, int fpad,
                                                               double* __restrict__ rowq) {
#pragma clang fp contract(off)
  constexpr int V = RowWalk<T>::V;
  typedef typename RowWalk<T>::vec_t vec_t;
  RowWalk<T> R;
  if (!R.begin(bl_ant, nbls, fpad)) return;
  GainPair<T> gp(gains, R.ant, fpad);
  double sum = 0;
  for (int f = R.lane * V; f < fpad; f += 64 * V) {
    const vec_t w = R.load(wgts, f);
    gp.load(f);
#pragma unroll
    for (int c = 0; c < V; ++c) {
      if (f + c < nfreqs) {
        const auto g = gp.at(c);
        sum += (double)w[c] * ((double)g.Gr * (double)g.Gr + (double)g.Gi * (double)g.Gi);
      }
    }
  }
  sum = ldsum(sum);
  if (R.lane == 0) rowq[R.b] = sum / (double)nfreqs;
}
__device__ __forceinline__ double gn_fix_diag(double d) { return (d > 0.0 && isfinite(d)) ? d : 1.0; }
// D of the gains: den [nants][nfreqs] (the third plane of gain_solve_ant_kernel) to both reals of the (re, im) pair; the padding gets 1
__global__ __launch_bounds__(256) void gn_precond_gain_kernel(const double* __restrict__ den, double* __restrict__ D, int nants, int nfreqs,
                                                               int fpad) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;  // (antenna, channel of fpad)
  if (idx >= (long long)nants * fpad) return;
  const int a = (int)(idx / fpad), f = (int)(idx - (long long)a * fpad);
  const double d = f < nfreqs ? gn_fix_diag(den[(long long)a * nfreqs + f]) : 1.0;
  D[2 * idx] = d;
  D[2 * idx + 1] = d;
}
// D of the coefficients: one thread per group adds its rows in row order
__global__ __launch_bounds__(256) void gn_precond_coeff_kernel(const double* __restrict__ rowq, const GnGroup* __restrict__ grp, int ngrps,
                                                                int ncoef, double* __restrict__ Dc) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= ngrps) return;
  const GnGroup G = grp[g];
  double sum = 0;
  for (int b = G.b0; b < G.b1; ++b) sum += rowq[b];
  sum = gn_fix_diag(sum);
  for (int k = 0; k < G.nvec; ++k) {
    Dc[G.coff + k] = sum;
    Dc[ncoef + G.coff + k] = sum;
  }
}

// out = -1/2 (a - b) over the live elements (0 on the padding), a given as the gradient pass leaves it (gains plane, coefficient planes)
template <typename T>
__global__ __launch_bounds__(256) void gn_rhs_kernel(GnSpace S, const T* __restrict__ a_g, const T* __restrict__ a_c, const T* __restrict__ b,
                                                      double* __restrict__ out) {
  const int t = blockIdx.y;
  const long long n = gn_slice_len(S, t);
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += 256ll * gridDim.x) {
    bool live;
    const long long i = gn_index(S, t, e, live);
    const double a = (double)(i < S.go ? a_g[i] : a_c[i - S.go]);
    out[i] = live ? -0.5 * (a - (double)b[i]) : 0.0;
  }
}

// CG set-up: x = 0, s = res / D (rounded to T: what the passes will read), partials of res . z
template <typename T>
__global__ __launch_bounds__(256) void gn_init_kernel(GnSpace S, const double* __restrict__ res, const double* __restrict__ D, double* __restrict__ x,
                                                       T* __restrict__ s, double* __restrict__ part) {
  __shared__ double s_w[4];
  const int t = blockIdx.y;
  const long long n = gn_slice_len(S, t);
  double acc = 0;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += 256ll * gridDim.x) {
    bool live;
    const long long i = gn_index(S, t, e, live);
    const double z = res[i] / D[i];
    x[i] = 0.0;
    s[i] = (T)z;
    acc += res[i] * z;
  }
  acc = gn_block_sum(acc, s_w);
  if (threadIdx.x == 0) part[(long long)t * gridDim.x + blockIdx.x] = acc;
}
// one thread per slice: rz = rz0 = the partials in block order; unselected slices and slices with nothing to solve start frozen
__global__ void gn_scalar0_kernel(GnScal* __restrict__ scal, const double* __restrict__ part, int nblocks, int nslices,
                                   const unsigned char* __restrict__ mask, const double* __restrict__ lambda, double tol) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nslices) return;
  double rz = 0;
  for (int k = 0; k < nblocks; ++k) rz += part[(long long)t * nblocks + k];
  GnScal sc{};
  sc.rz = sc.rz0 = rz;
  sc.scale = 1.0;
  sc.lambda = lambda ? lambda[t] : 0.0;
  sc.tol = tol;
  const bool ok = rz > 0.0 && isfinite(rz);
  sc.resid = ok ? 1.0 : 0.0;
  sc.frozen = (mask && !mask[t]) || !ok ? 1 : 0;
  scal[t] = sc;
}

// ns = -1/2 (grad - grad0) / s_t + lambda_t D s (D == nullptr: the plain product), partials of s . ns
template <typename T>
__global__ __launch_bounds__(256) void gn_diff_kernel(GnSpace S, const T* __restrict__ a_g, const T* __restrict__ a_c, const T* __restrict__ g0,
                                                       const T* __restrict__ s, const double* __restrict__ D, const GnScal* __restrict__ scal,
                                                       double* __restrict__ ns, double* __restrict__ part) {
  __shared__ double s_w[4];
  const int t = blockIdx.y;
  const GnScal sc = scal[t];
  if (sc.frozen) return;
  const long long n = gn_slice_len(S, t);
  double acc = 0;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += 256ll * gridDim.x) {
    bool live;
    const long long i = gn_index(S, t, e, live);
    const double a = (double)(i < S.go ? a_g[i] : a_c[i - S.go]);
    const double sv = (double)s[i];
    double v = live ? -0.5 * (a - (double)g0[i]) / sc.scale : 0.0;
    if (D) v += sc.lambda * D[i] * sv;
    ns[i] = v;
    acc += sv * v;
  }
  acc = gn_block_sum(acc, s_w);
  if (threadIdx.x == 0) part[(long long)t * gridDim.x + blockIdx.x] = acc;
}
// alpha = rz / s.Ns; a slice freezes where s.Ns <= 0 or is not finite
__global__ void gn_scalar1_kernel(GnScal* __restrict__ scal, const double* __restrict__ part, int nblocks, int nslices) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nslices || scal[t].frozen) return;
  double sns = 0;
  for (int k = 0; k < nblocks; ++k) sns += part[(long long)t * nblocks + k];
  const double alpha = scal[t].rz / sns;
  if (!(sns > 0.0) || !isfinite(sns) || !isfinite(alpha)) {
    scal[t].frozen = 1;
    return;
  }
  scal[t].alpha = alpha;
}
// x += alpha s, res -= alpha ns, partials of res . (res / D)
template <typename T>
__global__ __launch_bounds__(256) void gn_update1_kernel(GnSpace S, const GnScal* __restrict__ scal, const T* __restrict__ s,
                                                          const double* __restrict__ ns, const double* __restrict__ D, double* __restrict__ x,
                                                          double* __restrict__ res, double* __restrict__ part) {
  __shared__ double s_w[4];
  const int t = blockIdx.y;
  const GnScal sc = scal[t];
  if (sc.frozen) return;
  const long long n = gn_slice_len(S, t);
  double acc = 0;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += 256ll * gridDim.x) {
    bool live;
    const long long i = gn_index(S, t, e, live);
    x[i] += sc.alpha * (double)s[i];
    const double r = res[i] - sc.alpha * ns[i];
    res[i] = r;
    acc += r * (r / D[i]);
  }
  acc = gn_block_sum(acc, s_w);
  if (threadIdx.x == 0) part[(long long)t * gridDim.x + blockIdx.x] = acc;
}
// beta = rz_new / rz; the slice freezes once sqrt(rz_new / rz0) <= tol or rz_new is not finite
__global__ void gn_scalar2_kernel(GnScal* __restrict__ scal, const double* __restrict__ part, int nblocks, int nslices) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nslices || scal[t].frozen) return;
  double rz = 0;
  for (int k = 0; k < nblocks; ++k) rz += part[(long long)t * nblocks + k];
  GnScal sc = scal[t];
  sc.iters += 1;
  sc.resid = sqrt(rz / sc.rz0);
  if (!isfinite(rz) || !(sc.resid > sc.tol)) {
    sc.frozen = 1;
  } else {
    sc.beta = rz / sc.rz;
    sc.rz = rz;
  }
  scal[t] = sc;
}
// s = res / D + beta s, rounded to T once
template <typename T>
__global__ __launch_bounds__(256) void gn_update2_kernel(GnSpace S, const GnScal* __restrict__ scal, const double* __restrict__ res,
                                                          const double* __restrict__ D, T* __restrict__ s) {
  const int t = blockIdx.y;
  const GnScal sc = scal[t];
  if (sc.frozen) return;
  const long long n = gn_slice_len(S, t);
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += 256ll * gridDim.x) {
    bool live;
    const long long i = gn_index(S, t, e, live);
    s[i] = (T)(res[i] / D[i] + sc.beta * (double)s[i]);
  }
}

// the trial parameters of the selected slices: param = (T)(param + x), evaluated in double and rounded once; padding channels and
// the slices whose mask byte is 0 are not written
template <typename T>
__global__ __launch_bounds__(256) void gn_apply_kernel(GnSpace S, const unsigned char* __restrict__ mask, const double* __restrict__ x,
                                                        T* __restrict__ gains, T* __restrict__ coef) {
  const int t = blockIdx.y;
  if (mask && !mask[t]) return;
  const long long n = gn_slice_len(S, t);
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += 256ll * gridDim.x) {
    bool live;
    const long long i = gn_index(S, t, e, live);
    if (!live) continue;
    T* p = i < S.go ? gains + i : coef + (i - S.go);
    *p = (T)((double)*p + x[i]);
  }
}
// a double vector rounded to T (the product handed back to the caller)
template <typename T>
__global__ __launch_bounds__(256) void gn_round_kernel(const double* __restrict__ src, T* __restrict__ dst, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += 256ll * gridDim.x) dst[i] = (T)src[i];
}

}  // namespace calk
