// delay_coherent_kernels.hpp -- delay / fringe-rate power of redundant averages (cal_solver_delay_coherent_spectrum): the calibrated
// visibilities of a redundant group are added BEFORE they are transformed and squared, so that noise power falls as 1 / N in the group
// size; the fringe call's mean of powers is an incoherent average and cannot.  In the notation of delay_fringe_kernels.hpp a group g has
// T = ntimes SETS; set v = g T + t holds the members k in [set_ptr[v], set_ptr[v + 1]), each a row b_k = member_row[k] with a
// coefficient omega_k = member_wgt[k] >= 0 and a flag member_conj[k]:
//   u_k[f]       = omega_k                       (weighting = 0)
//                = omega_k (double) w[b_k][f]    (weighting = 1)        both taken as 0 where w[b_k][f] == 0
//   den_v[f]     = sum_k u_k[f]                                         in double, k ascending from 0
//   xbar_q[v][f] = (sum_k u_k[f] c_k(q[b_k][f])) / den_v[f]             c_k negates Im where member_conj[k]; re and im summed separately,
//                                                                       in double, k ascending from 0, acc += u * (double) q with contraction
//                                                                       off, then divided, then rounded ONCE to the solver's dtype;
//                                                                       0 where den_v[f] == 0
//   mask_v[f]    = den_v[f] > 0
//   mask_g[f]    = AND over t of mask_(g, t)[f]
//   x_q[g][t][f] = mask_g[f] ? xbar_q[g T + t][f] : 0
// with q[b][f] formed in the solver's dtype by DcrossSide::form under the row's OWN mask (w[b][f] != 0).  From x_q on everything is the
// fringe call's: dfringe_transform_kernel, dfringe_time_kernel and dspec_bin_kernel are launched as they are.  Two kernels in front:
//   dcoherent_rows_kernel   one wave per (set, span of 64 V channels): the members serially in ascending order, sums in double in
//                           registers; writes xbar in the dtype and the set's mask in bytes.  A set is never split over waves: the
//                           definition pins one serial order
//   dcoherent_mask_kernel   one wave per group: the common mask over t, zeros where it fails, norm_grp
// No atomics, no LDS, no scratch: two calls give the same bits, and so do two chunkings.
#pragma once
#include "delay_fringe_kernels.hpp"

namespace calk {

// Block = four waves; wave j of the grid is (set v = j / nspans, span = j % nspans) of the chunk, nspans = ceil(xpitch / (64 V)).  The
// planes and bl_ant are the solver's whole ones; set_ptr points at the chunk's first set and holds positions in the call's whole member
// arrays.  x: [nq][re, im][nsets][xpitch] (the quantities asked for in the order data, model, residual), zeros in the channels
// [nfreqs, xpitch); mask: [nsets][xpitch] bytes.
template <typename T>
__global__ __launch_bounds__(256) void dcoherent_rows_kernel(const T* __restrict__ model_r, const T* __restrict__ model_i, const T* __restrict__ data_r,
                                                              const T* __restrict__ data_i, const T* __restrict__ wgts,
                                                              const vec2_t<T>* __restrict__ gains, const int2* __restrict__ bl_ant,
                                                              const long long* __restrict__ set_ptr, const int* __restrict__ member_row,
                                                              const double* __restrict__ member_wgt, const unsigned char* __restrict__ member_conj,
                                                              int nsets, int nspans, int nfreqs, int fpad, int xpitch, int what, int calibrated,
                                                              int weighting, T* __restrict__ x, unsigned char* __restrict__ mask) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  typedef unsigned char mvec_t __attribute__((ext_vector_type(V)));
  const int lane = threadIdx.x & 63;
  const long long j = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
  if (j >= (long long)nsets * nspans) return;
  const int v = (int)(j / nspans), span = (int)(j - (long long)v * nspans);
  const int f = (span * 64 + lane) * V;
  if (f >= xpitch) return;  // fpad and xpitch are multiples of 8: whole vectors
  double den[V], acc[3][2][V];
#pragma unroll
  for (int c = 0; c < V; ++c) {
    den[c] = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) acc[q][0][c] = acc[q][1][c] = 0.0;
  }
  if (f < fpad) {
    const long long k0 = set_ptr[v], k1 = set_ptr[v + 1];
    for (long long k = k0; k < k1; ++k) {
      const int b = member_row[k];
      const double omega = member_wgt[k];
      const bool cj = member_conj[k] != 0;
      const long long row = (long long)b * fpad;
      const vec_t w = *reinterpret_cast<const vec_t*>(wgts + row + f);
      const vec_t mr = *reinterpret_cast<const vec_t*>(model_r + row + f), mi = *reinterpret_cast<const vec_t*>(model_i + row + f);
      const vec_t dr = *reinterpret_cast<const vec_t*>(data_r + row + f), di = *reinterpret_cast<const vec_t*>(data_i + row + f);
      GainPair<T> gp(gains, bl_ant[b], fpad);
      gp.load(f);
      bool live[V];
#pragma unroll
      for (int c = 0; c < V; ++c) live[c] = f + c < nfreqs && w[c] != (T)0;
      DcrossSide<T> side;
      side.form(mr, mi, dr, di, gp, live, calibrated);
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const double u = live[c] ? (weighting ? omega * (double)w[c] : omega) : 0.0;
        den[c] += u;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          if (!(what >> q & 1)) continue;
          const T im = cj ? -side.o[q][1][c] : side.o[q][1][c];
          acc[q][0][c] += u * (double)side.o[q][0][c];
          acc[q][1][c] += u * (double)im;
        }
      }
    }
  }
  const long long plane = (long long)nsets * xpitch;
  T* __restrict__ xrow = x + (long long)v * xpitch + f;
  int slot = 0;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    if (!(what >> q & 1)) continue;
    vec_t o_r, o_i;
#pragma unroll
    for (int c = 0; c < V; ++c) {
      o_r[c] = den[c] > 0.0 ? (T)(acc[q][0][c] / den[c]) : (T)0;
      o_i[c] = den[c] > 0.0 ? (T)(acc[q][1][c] / den[c]) : (T)0;
    }
    *reinterpret_cast<vec_t*>(xrow + (2 * slot) * plane) = o_r;
    *reinterpret_cast<vec_t*>(xrow + (2 * slot + 1) * plane) = o_i;
    ++slot;
  }
  mvec_t m;
#pragma unroll
  for (int c = 0; c < V; ++c) m[c] = den[c] > 0.0 ? 1 : 0;
  *reinterpret_cast<mvec_t*>(mask + (long long)v * xpitch + f) = m;
}

// One wave per group, four groups per block: the common mask of the group's T sets, the planes zeroed where it fails (a vector is
// rewritten only where it changes), norm_grp in double.  nplanes = 2 nq.
template <typename T>
__global__ __launch_bounds__(256) void dcoherent_mask_kernel(const unsigned char* __restrict__ mask, const double* __restrict__ norm_f, int ngroups, int ntimes,
                                                              int xpitch, int nplanes, T* __restrict__ x, double* __restrict__ norm_grp) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  typedef unsigned char mvec_t __attribute__((ext_vector_type(V)));
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
  if (g >= ngroups) return;
  const long long plane = (long long)ngroups * ntimes * xpitch;
  const unsigned char* __restrict__ mg = mask + (long long)g * ntimes * xpitch;
  T* __restrict__ xg = x + (long long)g * ntimes * xpitch;
  double acc_n = 0;
  for (int f = lane * V; f < xpitch; f += 64 * V) {
    bool live[V];
#pragma unroll
    for (int c = 0; c < V; ++c) live[c] = true;
    for (int t = 0; t < ntimes; ++t) {
      const mvec_t m = *reinterpret_cast<const mvec_t*>(mg + (long long)t * xpitch + f);
#pragma unroll
      for (int c = 0; c < V; ++c) live[c] = live[c] && m[c] != 0;
    }
    bool all = true;
#pragma unroll
    for (int c = 0; c < V; ++c) {
      acc_n += live[c] ? norm_f[f + c] : 0.0;  // (norm_f is zero beyond nfreqs, and so is every mask)
      all = all && live[c];
    }
    if (all) continue;
    for (int t = 0; t < ntimes; ++t)
      for (int p = 0; p < nplanes; ++p) {
        T* __restrict__ at = xg + (long long)p * plane + (long long)t * xpitch + f;
        vec_t o = *reinterpret_cast<const vec_t*>(at);
#pragma unroll
        for (int c = 0; c < V; ++c) o[c] = live[c] ? o[c] : (T)0;
        *reinterpret_cast<vec_t*>(at) = o;
      }
  }
  acc_n = ldsum(acc_n);
  if (lane == 0) norm_grp[g] = acc_n;
}

}  // namespace calk
