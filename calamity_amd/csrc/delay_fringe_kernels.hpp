// delay_fringe_kernels.hpp -- the delay / fringe-rate plane (cal_solver_delay_fringe_spectrum): the delay transform of T rows that are
// one baseline at T integrations, then a transform along time.  Instrument-locked residuals sit at fringe rate 0, the sky at the rate its
// baseline gives it, noise is white in fringe rate.  In the notation of delay_spectrum_kernels.hpp, for group g with rows rows[g][0 .. T)
// and scales a[g][t]:
//   mask_g[f]      = AND over t of (w[rows[g][t]][f] != 0)         the COMMON mask of all T rows (delay_cross_kernels.hpp gives the reason)
//   x_q[g][t][f]   = mask_g q[rows[g][t]][f]                       q among data, model, residual as dspec_rows_kernel forms them
//   X_q[g][t][k]   = sum_f x_q[g][t][f] (op_r + i op_i)[f][k]
//   norm_grp[g]    = sum_f mask_g norm_f[f]
//   Y_t            = a[g][t] X_q[g][t][k]                          in double, after the matrix product
//   Z_q[g][r][k]   = sum_t opt[t][r] Y_t                           complex, in double; from zero, for t ascending
//                                                                  re += (opt_r yr - opt_i yi), im += (opt_r yi + opt_i yr), contraction off
//   power[q][g][r][k] = (Re Z^2 + Im Z^2) / norm_grp[g]            0 where norm_grp[g] == 0
// Three kernels behind the model pass, per chunk of whole groups, then dspec_bin_kernel as it is (over groups instead of rows, with
// nrates ndelays columns):
//   dfringe_rows_kernel        one pass over (g, f): the common mask from the T weight rows, then the masked planes of the T rows in T
//   dfringe_transform_kernel   X = x op on the matrix cores by ds_transform_loop, row-wise over the chunk's cgroups T rows; Y in double
//   dfringe_time_kernel        Z = sum_t opt Y from a group's Y staged in LDS, |Z|^2 / norm in double
// Every sum over groups is taken in double in a fixed order (no atomics on reals): two calls give the same bits, and so do two chunkings.
#pragma once
#include "delay_cross_kernels.hpp"

namespace calk {

constexpr int kDfCols = 64;  // delays per workgroup of the time kernel: a group's Y is [T][re, im][64] doubles in LDS, 64 KiB at T = 64,
                             // so that two workgroups share a CU's 160 KiB
constexpr int kDfLanes = 4;  // rate lanes: a thread owns a delay and the rates lane, lane + 4, ...

// One wave per group, four groups per block.  The planes and bl_ant are the solver's whole ones (a group is any T rows, repeats
// allowed: a repeated row is simply read again), `rows` the chunk's first group, `ngroups` its groups.  x: [nq][re, im][ngroups T][xpitch]
// (time t of chunk group g is row g T + t; the quantities asked for in the order data, model, residual), zeros in the channels
// [nfreqs, xpitch).
template <typename T>
__global__ __launch_bounds__(256) void dfringe_rows_kernel(const T* __restrict__ model_r, const T* __restrict__ model_i, const T* __restrict__ data_r,
                                                            const T* __restrict__ data_i, const T* __restrict__ wgts,
                                                            const vec2_t<T>* __restrict__ gains, const int2* __restrict__ bl_ant,
                                                            const int* __restrict__ rows, const double* __restrict__ norm_f, int ngroups, int ntimes,
                                                            int nfreqs, int fpad, int xpitch, int what, int calibrated, T* __restrict__ x,
                                                            double* __restrict__ norm_grp) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
  if (g >= ngroups) return;
  const int* __restrict__ grow = rows + (long long)g * ntimes;
  const long long plane = (long long)ngroups * ntimes * xpitch;
  T* __restrict__ xg = x + (long long)g * ntimes * xpitch;
  double acc_n = 0;
  for (int f = lane * V; f < xpitch; f += 64 * V) {  // fpad and xpitch are multiples of 8: whole vectors
    bool live[V];
#pragma unroll
    for (int c = 0; c < V; ++c) live[c] = f < fpad && f + c < nfreqs;
    if (f < fpad) {
      for (int t = 0; t < ntimes; ++t) {
        const vec_t w = *reinterpret_cast<const vec_t*>(wgts + (long long)grow[t] * fpad + f);
#pragma unroll
        for (int c = 0; c < V; ++c) live[c] = live[c] && w[c] != (T)0;
      }
#pragma unroll
      for (int c = 0; c < V; ++c) acc_n += live[c] ? norm_f[f + c] : 0.0;
    }
    for (int t = 0; t < ntimes; ++t) {
      DcrossSide<T> side;
#pragma unroll
      for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int c = 0; c < V; ++c) side.o[q][0][c] = side.o[q][1][c] = (T)0;
      if (f < fpad) {
        const int b = grow[t];
        const long long row = (long long)b * fpad;
        const vec_t mr = *reinterpret_cast<const vec_t*>(model_r + row + f), mi = *reinterpret_cast<const vec_t*>(model_i + row + f);
        const vec_t dr = *reinterpret_cast<const vec_t*>(data_r + row + f), di = *reinterpret_cast<const vec_t*>(data_i + row + f);
        GainPair<T> gp(gains, bl_ant[b], fpad);
        gp.load(f);
        side.form(mr, mi, dr, di, gp, live, calibrated);
      }
      T* __restrict__ xrow = xg + (long long)t * xpitch;
      int slot = 0;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        if (!(what >> q & 1)) continue;
        *reinterpret_cast<vec_t*>(xrow + (2 * slot) * plane + f) = side.o[q][0];
        *reinterpret_cast<vec_t*>(xrow + (2 * slot + 1) * plane + f) = side.o[q][1];
        ++slot;
      }
    }
  }
  acc_n = ldsum(acc_n);
  if (lane == 0) norm_grp[g] = acc_n;
}

// block = (128 rows, 64 delays, quantity), the grid and row tiles of dspec_transform_kernel: the transform is row-wise and the groups'
// boundaries do not matter to it.  Rows past the chunk's last read its last row again and write nothing.  scale: [nrows] of the chunk.
// out: [nq][re, im][nrows][ndelays] doubles, Y = scale X.
template <typename T>
__global__ __launch_bounds__(256, 2) void dfringe_transform_kernel(const T* __restrict__ x, const T* __restrict__ op, const double* __restrict__ scale,
                                                                    int nrows, int xpitch, int ndelays, int ndpad, double* __restrict__ out) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  typedef typename MmT<T>::v4 acc_t;
  __shared__ __attribute__((aligned(16))) T s_op[2][kDsStep][kDsPitch<T>];  // [re, im][channel of the step][delay of the block]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int r0 = blockIdx.x * kDsRows + wave * (kDsRowTiles * 16);
  const int c0 = blockIdx.y * kDsCols;
  const long long plane = (long long)nrows * xpitch;
  const T* __restrict__ xr = x + (long long)blockIdx.z * 2 * plane;
  const T* __restrict__ xi = xr + plane;
  const T* xrow_r[kDsRowTiles];
  const T* xrow_i[kDsRowTiles];
#pragma unroll
  for (int rt = 0; rt < kDsRowTiles; ++rt) {
    int row = r0 + rt * 16 + col;
    row = row < nrows ? row : nrows - 1;
    xrow_r[rt] = xr + (long long)row * xpitch + kq * V;
    xrow_i[rt] = xi + (long long)row * xpitch + kq * V;
  }
  acc_t acc_re[kDsRowTiles][4], acc_im[kDsRowTiles][4];
  ds_transform_loop<T>(xrow_r, xrow_i, op, op + (long long)xpitch * ndpad, xpitch, ndpad, c0, s_op, acc_re, acc_im);
  const long long yplane = (long long)nrows * ndelays;
  double* __restrict__ o_re = out + (long long)blockIdx.z * 2 * yplane;
  double* __restrict__ o_im = o_re + yplane;
#pragma unroll
  for (int rt = 0; rt < kDsRowTiles; ++rt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + rt * 16 + MmT<T>::row_of(kq, r);
      if (row >= nrows) continue;
      const double a = scale[row];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int k = c0 + t * 16 + col;
        if (k >= ndelays) continue;
        o_re[(long long)row * ndelays + k] = a * (double)acc_re[rt][t][r];
        o_im[(long long)row * ndelays + k] = a * (double)acc_im[rt][t][r];
      }
    }
  }
}

// block = (group, 64 delays, quantity), 256 threads: thread (delay d = tid & 63, rate lane = tid >> 6, wave-uniform).  The group's
// Y [ntimes][re, im][64] is staged in dynamic LDS (ntimes 2 64 doubles; zeros past ndelays), then every thread sums its rates over t
// ascending in the order of the definition; opt ([ntimes][nrates] per part) is read at wave-uniform addresses.  y: the chunk's
// [nq][re, im][ngroups ntimes][ndelays]; out: [nq][ngroups][nrates][ndelays] doubles.
__global__ __launch_bounds__(256) void dfringe_time_kernel(const double* __restrict__ y, const double* __restrict__ opt_r, const double* __restrict__ opt_i,
                                                            const double* __restrict__ norm_grp, int ngroups, int ntimes, int nrates, int ndelays,
                                                            double* __restrict__ out) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double s_y[];  // [ntimes][re, im][kDfCols]
  const int tid = threadIdx.x;
  const int g = blockIdx.x, c0 = blockIdx.y * kDfCols, q = blockIdx.z;
  const long long yplane = (long long)ngroups * ntimes * ndelays;
  const double* __restrict__ yq = y + (long long)q * 2 * yplane + (long long)g * ntimes * ndelays;
  for (int idx = tid; idx < ntimes * 2 * kDfCols; idx += 256) {
    const int t = idx / (2 * kDfCols), rem = idx - t * (2 * kDfCols);
    const int part = rem / kDfCols, d = rem - part * kDfCols;
    s_y[idx] = c0 + d < ndelays ? yq[part * yplane + (long long)t * ndelays + c0 + d] : 0.0;
  }
  __syncthreads();
  const int d = tid & 63, k = c0 + d;
  const int lane_r = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (k >= ndelays) return;
  const double nb = norm_grp[g];
  double* __restrict__ o = out + ((long long)q * ngroups + g) * nrates * ndelays + k;
  for (int r = lane_r; r < nrates; r += kDfLanes) {
    double re = 0.0, im = 0.0;
    for (int t = 0; t < ntimes; ++t) {
      const double wr = opt_r[t * nrates + r], wi = opt_i[t * nrates + r];
      const double yr = s_y[t * 2 * kDfCols + d], yi = s_y[(t * 2 + 1) * kDfCols + d];
      re += (wr * yr - wi * yi);
      im += (wr * yi + wi * yr);
    }
    o[(long long)r * ndelays] = nb != 0.0 ? (re * re + im * im) / nb : 0.0;
  }
}

}  // namespace calk
