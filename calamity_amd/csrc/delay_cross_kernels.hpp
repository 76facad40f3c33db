// delay_cross_kernels.hpp -- delay power that noise does not bias (cal_solver_delay_cross_spectrum): the cross power of two rows that
// see the same sky with independent noise (two adjacent integrations of a baseline), and the power of their half difference, the
// noise spectrum measured from the data.  In the notation of delay_spectrum_kernels.hpp, for pair p = (b0, b1) with scales (a0, a1):
//   mask_p[f]      = (w[b0][f] != 0) && (w[b1][f] != 0)            the COMMON mask: sides flagged differently would leak differently
//   x_q[p][s][f]   = mask_p q[b_s][f]                              s = 0, 1;  q among data, model, residual as dspec_rows_kernel forms them
//   X_q[p][s][k]   = sum_f x_q[p][s][f] (op_r + i op_i)[f][k]
//   norm_pair[p]   = sum_f mask_p norm_f[f]
//   Y_s            = a_s X_q[p][s][k]                              in double, after the matrix product
//   cross[q][p][k] = (Re Y_0 Re Y_1 + Im Y_0 Im Y_1) / norm_pair[p]                      0 where norm_pair[p] == 0
//   diff[q][p][k]  = ((Re Y_0 - Re Y_1)^2 + (Im Y_0 - Im Y_1)^2) / (2 norm_pair[p])
// Two kernels behind the model pass, per chunk of pairs, then dspec_bin_kernel as it is (over pairs instead of rows, nstat nq planes):
//   dcross_rows_kernel        one pass over (p, f) of both rows in step: the masked planes of both sides in T, norm_pair in double
//   dcross_transform_kernel   X = x op on the matrix cores by ds_transform_loop: a wave's row tile 0 is side 0 and its tile 1 side 1 of the
//                             same 16 pairs, so the four accumulators of (pair, delay) sit in one lane and the epilogue needs no exchange
// Every sum over pairs is taken in double in a fixed order (no atomics on reals): two calls give the same bits, and so do two chunkings.
#pragma once
#include "delay_spectrum_kernels.hpp"

namespace calk {

constexpr int kDcPairs = 4 * 16;  // pairs per workgroup of the transform: 16 per wave, both sides

// One side of a pair at V channels: data, model and residual as dspec_rows_kernel forms them (the same operations in the same order:
// a (b, b) pair gives the planes of row b), masked by `live`.
template <typename T>
struct DcrossSide {
  static constexpr int V = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  vec_t o[3][2];
  __device__ __forceinline__ void form(const vec_t& mr, const vec_t& mi, const vec_t& dr, const vec_t& di, const GainPair<T>& gp, const bool (&live)[V],
                                       int calibrated) {
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < V; ++c) {
      const auto g = gp.at(c);
      T d_r, d_i, m_r, m_i;
      if (calibrated) {
        const T den = g.Gr * g.Gr + g.Gi * g.Gi;
        const bool okg = den != (T)0;
        d_r = okg ? (dr[c] * g.Gr + di[c] * g.Gi) / den : (T)0;  // d conj(G) / |G|^2
        d_i = okg ? (di[c] * g.Gr - dr[c] * g.Gi) / den : (T)0;
        m_r = okg ? mr[c] : (T)0;
        m_i = okg ? mi[c] : (T)0;
      } else {
        d_r = dr[c], d_i = di[c];
        m_r = g.Gr * mr[c] - g.Gi * mi[c];
        m_i = g.Gi * mr[c] + g.Gr * mi[c];
      }
      o[0][0][c] = live[c] ? d_r : (T)0, o[0][1][c] = live[c] ? d_i : (T)0;
      o[1][0][c] = live[c] ? m_r : (T)0, o[1][1][c] = live[c] ? m_i : (T)0;
      o[2][0][c] = live[c] ? d_r - m_r : (T)0, o[2][1][c] = live[c] ? d_i - m_i : (T)0;
    }
  }
};

// One wave per pair, four pairs per block; two row cursors in the manner of RowWalk.  The planes and bl_ant are the solver's whole
// ones (a pair is any two rows), `pairs` the chunk's first pair, `npairs` its pairs.  x: [nq][re, im][2 sides][npairs][xpitch] (side s
// of chunk pair p is row s npairs + p; the quantities asked for in the order data, model, residual), zeros in the channels [nfreqs, xpitch).
template <typename T>
__global__ __launch_bounds__(256) void dcross_rows_kernel(const T* __restrict__ model_r, const T* __restrict__ model_i, const T* __restrict__ data_r,
                                                           const T* __restrict__ data_i, const T* __restrict__ wgts,
                                                           const vec2_t<T>* __restrict__ gains, const int2* __restrict__ bl_ant,
                                                           const int2* __restrict__ pairs, const double* __restrict__ norm_f, int npairs, int nfreqs,
                                                           int fpad, int xpitch, int what, int calibrated, T* __restrict__ x,
                                                           double* __restrict__ norm_pair) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
  if (p >= npairs) return;
  const int2 pr = pairs[p];
  const long long row[2] = {(long long)pr.x * fpad, (long long)pr.y * fpad};
  GainPair<T> gp[2] = {GainPair<T>(gains, bl_ant[pr.x], fpad), GainPair<T>(gains, bl_ant[pr.y], fpad)};
  const long long plane = 2ll * npairs * xpitch;
  T* __restrict__ xrow[2] = {x + (long long)p * xpitch, x + ((long long)npairs + p) * xpitch};
  double acc_n = 0;
  for (int f = lane * V; f < xpitch; f += 64 * V) {  // fpad and xpitch are multiples of 8: whole vectors
    DcrossSide<T> side[2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int c = 0; c < V; ++c) side[s].o[q][0][c] = side[s].o[q][1][c] = (T)0;
    if (f < fpad) {
      const vec_t w0 = *reinterpret_cast<const vec_t*>(wgts + row[0] + f), w1 = *reinterpret_cast<const vec_t*>(wgts + row[1] + f);
      bool live[V];
#pragma unroll
      for (int c = 0; c < V; ++c) {
        live[c] = f + c < nfreqs && w0[c] != (T)0 && w1[c] != (T)0;
        acc_n += live[c] ? norm_f[f + c] : 0.0;
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const vec_t mr = *reinterpret_cast<const vec_t*>(model_r + row[s] + f), mi = *reinterpret_cast<const vec_t*>(model_i + row[s] + f);
        const vec_t dr = *reinterpret_cast<const vec_t*>(data_r + row[s] + f), di = *reinterpret_cast<const vec_t*>(data_i + row[s] + f);
        gp[s].load(f);
        side[s].form(mr, mi, dr, di, gp[s], live, calibrated);
      }
    }
    int slot = 0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      if (!(what >> q & 1)) continue;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        *reinterpret_cast<vec_t*>(xrow[s] + (2 * slot) * plane + f) = side[s].o[q][0];
        *reinterpret_cast<vec_t*>(xrow[s] + (2 * slot + 1) * plane + f) = side[s].o[q][1];
      }
      ++slot;
    }
  }
  acc_n = ldsum(acc_n);
  if (lane == 0) norm_pair[p] = acc_n;
}

// block = (64 pairs, 64 delays, quantity); wave w owns the pairs 16 w .. 16 w + 15 of the block: row tile 0 of ds_transform_loop is
// their side 0, tile 1 their side 1.  Pairs past the chunk's last read its last pair again and write nothing.  scale: [npairs][2] of
// the chunk.  out: [nstat][nq][npairs][ndelays] doubles, cross (stats bit 0) before diff (bit 1).
template <typename T>
__global__ __launch_bounds__(256, 2) void dcross_transform_kernel(const T* __restrict__ x, const T* __restrict__ op, const double* __restrict__ norm_pair,
                                                                   const double* __restrict__ scale, int npairs, int xpitch, int ndelays, int ndpad,
                                                                   int stats, double* __restrict__ out) {
#pragma clang fp contract(off)
  static_assert(kDsRowTiles == 2, "a wave's two row tiles are the two sides of its pairs");
  constexpr int V = 16 / (int)sizeof(T);
  typedef typename MmT<T>::v4 acc_t;
  __shared__ __attribute__((aligned(16))) T s_op[2][kDsStep][kDsPitch<T>];  // [re, im][channel of the step][delay of the block]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int p0 = blockIdx.x * kDcPairs + wave * 16;
  const int c0 = blockIdx.y * kDsCols;
  const long long plane = 2ll * npairs * xpitch;
  const T* __restrict__ xr = x + (long long)blockIdx.z * 2 * plane;
  const T* __restrict__ xi = xr + plane;
  const T* xrow_r[kDsRowTiles];
  const T* xrow_i[kDsRowTiles];
  int pair = p0 + col;
  pair = pair < npairs ? pair : npairs - 1;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const long long row = (long long)s * npairs + pair;
    xrow_r[s] = xr + row * xpitch + kq * V;
    xrow_i[s] = xi + row * xpitch + kq * V;
  }
  acc_t acc_re[kDsRowTiles][4], acc_im[kDsRowTiles][4];
  ds_transform_loop<T>(xrow_r, xrow_i, op, op + (long long)xpitch * ndpad, xpitch, ndpad, c0, s_op, acc_re, acc_im);
  const long long stat_plane = (long long)gridDim.z * npairs * ndelays;
  double* __restrict__ o_cross = out + (long long)blockIdx.z * npairs * ndelays;
  double* __restrict__ o_diff = o_cross + ((stats & 1) ? stat_plane : 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int pw = p0 + MmT<T>::row_of(kq, r);
    if (pw >= npairs) continue;
    const double nb = norm_pair[pw];
    const double a0 = scale[2 * pw], a1 = scale[2 * pw + 1];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int k = c0 + t * 16 + col;
      if (k >= ndelays) continue;
      const double re0 = a0 * (double)acc_re[0][t][r], im0 = a0 * (double)acc_im[0][t][r];
      const double re1 = a1 * (double)acc_re[1][t][r], im1 = a1 * (double)acc_im[1][t][r];
      if (stats & 1) o_cross[(long long)pw * ndelays + k] = nb != 0.0 ? (re0 * re1 + im0 * im1) / nb : 0.0;
      if (stats & 2) {
        const double dr = re0 - re1, di = im0 - im1;
        o_diff[(long long)pw * ndelays + k] = nb != 0.0 ? (dr * dr + di * di) / (2.0 * nb) : 0.0;
      }
    }
  }
}

}  // namespace calk
