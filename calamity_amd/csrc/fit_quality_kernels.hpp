// fit_quality_kernels.hpp -- where the residual power of a fit sits (cal_solver_fit_quality): per baseline and per (antenna, channel).
//   e[b][f]         = w[b][f] |d[b][f] - g_i[f] conj(g_j[f]) m[b][f]|^2,   (i, j) the antennas of baseline b, m = A c (MODE_MODEL's planes)
//   chisq_bl[b]     = sum_f e[b][f]              wsum_bl[b]     = sum_f w[b][f]
//   chisq_ant[a][f] = sum_{b with a} e[b][f]     wsum_ant[a][f] = sum_{b with a} w[b][f]     (an autocorrelation counts once)
// Two kernels behind the model pass:
//   quality_rows_kernel   one pass over (b, f): e in T over the model_r plane, the two row sums in double
//   quality_ant_kernel    gain_grad_kernel's walk of the sorted antenna-to-baseline list over the planes e and w, sums in double
// Products are formed in T in the order of the loss kernels (fit_kernels.hpp: process_item, square_error_kernel), every sum is taken
// in double in a fixed order (lane partials, a butterfly over the wave; four segments through LDS in ascending order): no float
// atomics, two calls give the same bits.  Neither kernel looks at the loop state: a stopped slice is evaluated like any other.
#pragma once
#include "row_walk.hpp"

namespace calk {

// One wave per baseline row, four rows per block; a lane owns V = 16 / sizeof(T) adjacent channels per trip (16-byte loads of the
// five planes, 2 x 16 bytes of each antenna's interleaved gains).  Channels [nfreqs, fpad) write e = 0 and add nothing.
template <typename T>
__global__ __launch_bounds__(256) void quality_rows_kernel(T* __restrict__ model_r, const T* __restrict__ model_i, const T* __restrict__ data_r,
                                                            const T* __restrict__ data_i, const T* __restrict__ wgts,
                                                            const vec2_t<T>* __restrict__ gains, const int2* __restrict__ bl_ant, int nbls, int nfreqs,
                                                            int fpad, double* __restrict__ chisq_bl, double* __restrict__ wsum_bl) {
#pragma clang fp contract(off)
  constexpr int V = RowWalk<T>::V;
  typedef typename RowWalk<T>::vec_t vec_t;
  RowWalk<T> R;
  if (!R.begin(bl_ant, nbls, fpad)) return;
  GainPair<T> gp(gains, R.ant, fpad);
  double acc_e = 0, acc_w = 0;
  for (int f = R.lane * V; f < fpad; f += 64 * V) {  // fpad is a multiple of 8: whole vectors
    const vec_t mr = R.load(model_r, f), mi = R.load(model_i, f);
    const vec_t dr = R.load(data_r, f), di = R.load(data_i, f);
    const vec_t w = R.load(wgts, f);
    gp.load(f);
    vec_t e;
#pragma unroll
    for (int c = 0; c < V; ++c) {
      const auto g = gp.at(c);
      const T m_r = g.Gr * mr[c] - g.Gi * mi[c];
      const T m_i = g.Gi * mr[c] + g.Gr * mi[c];
      const T r_r = dr[c] - m_r;
      const T r_i = di[c] - m_i;
      const bool live = f + c < nfreqs;
      const T ec = live ? w[c] * (r_r * r_r + r_i * r_i) : (T)0;
      e[c] = ec;
      acc_e += (double)ec;
      acc_w += live ? (double)w[c] : 0.0;
    }
    R.store(model_r, f, e);
  }
  acc_e = ldsum(acc_e);
  acc_w = ldsum(acc_w);
  if (R.lane == 0) {
    chisq_bl[R.b] = acc_e;
    wsum_bl[R.b] = acc_w;
  }
}

// block = (antenna a, 64 V channels), channel-block major like gain_grad_kernel and for its reason: the two antennas of a baseline read
// the same piece of its rows of e and w, and with all the antennas of one channel block next to each other in dispatch order the
// second read finds it in the Infinity Cache.  The antenna's sorted list is cut into four segments, one per wave, eight rows' loads
// in flight; the segments' double partial sums are combined through LDS in ascending order.  The role-1 entry of an autocorrelation
// (other antenna == a) is skipped: its row entered through the role-0 entry.  An antenna without baselines writes zeros.
// Outputs are [nants][nfreqs] doubles, unpadded (they are the exchange payload and go to the host as they are).
template <typename T>
__global__ __launch_bounds__(256) void quality_ant_kernel(const T* __restrict__ e_rows, const T* __restrict__ w_rows, const int* __restrict__ ant_ptr,
                                                           const int2* __restrict__ ant_ent, int nants, int nfreqs, int fpad,
                                                           double* __restrict__ chisq_ant, double* __restrict__ wsum_ant) {
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  __shared__ double s_part[3][2][64][V];  // [segment 1..3][e, w][lane][channel]
  const int cb = blockIdx.x / nants;
  const int a = blockIdx.x - cb * nants;
  const int lane = threadIdx.x & 63;
  const int seg = threadIdx.x >> 6;
  const int f = (cb * 64 + lane) * V;
  const bool ok = f < fpad;
  double se[V], sw[V];
#pragma unroll
  for (int c = 0; c < V; ++c) se[c] = sw[c] = 0;
  const int e0 = ant_ptr[a], e1 = ant_ptr[a + 1];
  const int per = (e1 - e0 + 3) >> 2;
  const int eb = e0 + seg * per, ee = min(e1, eb + per);
  if (ok) {
#pragma unroll 8
    for (int e = eb; e < ee; ++e) {
      const int2 ent = ant_ent[e];  // (bl * 2 + role, other antenna): wave-uniform
      const bool skip = (ent.x & 1) && ent.y == a;  // (selected away below, not branched around: the unrolled loads stay together)
      const long long off = (long long)(ent.x >> 1) * fpad + f;
      const vec_t ev = *reinterpret_cast<const vec_t*>(e_rows + off);
      const vec_t wv = *reinterpret_cast<const vec_t*>(w_rows + off);
#pragma unroll
      for (int c = 0; c < V; ++c) {
        se[c] += skip ? 0.0 : (double)ev[c];
        sw[c] += skip ? 0.0 : (double)wv[c];
      }
    }
  }
  if (seg > 0) {
#pragma unroll
    for (int c = 0; c < V; ++c) {
      s_part[seg - 1][0][lane][c] = se[c];
      s_part[seg - 1][1][lane][c] = sw[c];
    }
  }
  __syncthreads();
  if (seg == 0 && ok) {
#pragma unroll
    for (int g = 0; g < 3; ++g) {
#pragma unroll
      for (int c = 0; c < V; ++c) {
        se[c] += s_part[g][0][lane][c];
        sw[c] += s_part[g][1][lane][c];
      }
    }
#pragma unroll
    for (int c = 0; c < V; ++c) {
      if (f + c < nfreqs) {
        chisq_ant[(long long)a * nfreqs + f + c] = se[c];
        wsum_ant[(long long)a * nfreqs + f + c] = sw[c];
      }
    }
  }
}

}  // namespace calk
