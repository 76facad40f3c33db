// gain_solve_kernels.hpp -- the gains in closed form (cal_solver_solve_gains): damped StefCal sweeps (Salvini & Wijnholds 2014).
// With the foreground model m = A c held fixed, chi^2 = sum w |d - g_i conj(g_j) m|^2 is linear least squares in one antenna's gain
// while the others are held fixed.  Baseline b has antennas (i, j); per channel f:
//   P[b][f] = w d conj(m)   (complex)            Q[b][f] = w |m|^2   (real)
//   role 0 (a == i):  num[a][f] += P g_j              den[a][f] += Q |g_j|^2
//   role 1 (a == j):  num[a][f] += conj(P) g_i        den[a][f] += Q |g_i|^2
//   g_new[a][f] = (1 - damping) g[a][f] + damping num / den      where den > 0, else g[a][f] stays
// An autocorrelation row (i == j) enters neither sum (its model is quadratic in one gain); every antenna is updated from the OLD
// gains (a Jacobi sweep).  Three kernels behind the model pass:
//   gain_solve_rows_kernel    once per call: P_r, P_i over the two model planes, Q into a third plane, all in T
//   gain_solve_ant_kernel     once per sweep: quality_ant_kernel's walk of a sorted antenna-to-baseline list over the three planes
//   gain_solve_apply_kernel   once per sweep: the damped update of the selected slices' gains
// Products are formed in T, num and den are accumulated in double in a fixed order (the list in baseline order, four segments
// combined through LDS in ascending order): no float atomics, two calls give the same bits.
#pragma once
#include "row_walk.hpp"

namespace calk {

// One wave per baseline row, four rows per block; a lane owns V = 16 / sizeof(T) adjacent channels per trip (16-byte loads of the
// five planes).  P_r overwrites model_r, P_i model_i.  Channels [nfreqs, fpad) and autocorrelation rows write zeros.
template <typename T>
__global__ __launch_bounds__(256) void gain_solve_rows_kernel(T* __restrict__ model_r, T* __restrict__ model_i, T* __restrict__ q_rows,
                                                               const T* __restrict__ data_r, const T* __restrict__ data_i,
                                                               const T* __restrict__ wgts, const int2* __restrict__ bl_ant, int nbls, int nfreqs,
                                                               int fpad) {
#pragma clang fp contract(off)
  constexpr int V = RowWalk<T>::V;
  typedef typename RowWalk<T>::vec_t vec_t;
  RowWalk<T> R;
  if (!R.begin(bl_ant, nbls, fpad)) return;
  const bool cross = R.ant.x != R.ant.y;
  for (int f = R.lane * V; f < fpad; f += 64 * V) {  // fpad is a multiple of 8: whole vectors
    const vec_t mr = R.load(model_r, f), mi = R.load(model_i, f);
    const vec_t dr = R.load(data_r, f), di = R.load(data_i, f);
    const vec_t w = R.load(wgts, f);
    vec_t pr, pi, q;
#pragma unroll
    for (int c = 0; c < V; ++c) {
      const bool live = cross && f + c < nfreqs;
      pr[c] = live ? w[c] * (dr[c] * mr[c] + di[c] * mi[c]) : (T)0;  // d conj(m)
      pi[c] = live ? w[c] * (di[c] * mr[c] - dr[c] * mi[c]) : (T)0;
      q[c] = live ? w[c] * (mr[c] * mr[c] + mi[c] * mi[c]) : (T)0;
    }
    R.store(model_r, f, pr);
    R.store(model_i, f, pi);
    R.store(q_rows, f, q);
  }
}

// block = (antenna a, 64 V channels), channel-block major like quality_ant_kernel and for its reason: the two antennas of a baseline
// read the same piece of its rows of P and Q, and with all the antennas of one channel block next to each other in dispatch order
// the second read finds it in the Infinity Cache.  The antenna's sorted list (cross-correlations only: the host leaves the
// autocorrelation rows out of it) is cut into four segments, one per wave, four rows' loads in flight; the other antenna's gain
// row is read per entry (nants rows per channel block: it stays in the caches).  The segments' double partial sums are combined
// through LDS in ascending order.  An antenna without baselines writes zeros.
// Output: num_r | num_i | den as [3][nants][nfreqs] doubles, unpadded (the exchange payload).
template <typename T>
__global__ __launch_bounds__(256) void gain_solve_ant_kernel(const T* __restrict__ p_r, const T* __restrict__ p_i, const T* __restrict__ q_rows,
                                                              const vec2_t<T>* __restrict__ gains, const int* __restrict__ ant_ptr,
                                                              const int2* __restrict__ ant_ent, int nants, int nfreqs, int fpad,
                                                              double* __restrict__ planes) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  __shared__ double s_part[3][3][64][V];  // [segment 1..3][num_r, num_i, den][lane][channel]
  const int cb = blockIdx.x / nants;
  const int a = blockIdx.x - cb * nants;
  const int lane = threadIdx.x & 63;
  const int seg = threadIdx.x >> 6;
  const int f = (cb * 64 + lane) * V;
  const bool ok = f < fpad;
  double nr[V], ni[V], dn[V];
#pragma unroll
  for (int c = 0; c < V; ++c) nr[c] = ni[c] = dn[c] = 0;
  const int e0 = ant_ptr[a], e1 = ant_ptr[a + 1];
  const int per = (e1 - e0 + 3) >> 2;
  const int eb = e0 + seg * per, ee = min(e1, eb + per);
  if (ok) {
#pragma unroll 4
    for (int e = eb; e < ee; ++e) {
      const int2 ent = ant_ent[e];  // (bl * 2 + role, other antenna): wave-uniform
      const T sgn = (ent.x & 1) ? (T)-1 : (T)1;  // role 1 takes conj(P)
      const long long off = (long long)(ent.x >> 1) * fpad + f;
      const vec_t pr = *reinterpret_cast<const vec_t*>(p_r + off);
      const vec_t pi = *reinterpret_cast<const vec_t*>(p_i + off);
      const vec_t q = *reinterpret_cast<const vec_t*>(q_rows + off);
      const vec2_t<T>* __restrict__ go = gains + (long long)ent.y * fpad + f;
      vec_t g2[2];  // V channels of (re, im)
      g2[0] = *reinterpret_cast<const vec_t*>(go);
      g2[1] = *reinterpret_cast<const vec_t*>(go + V / 2);
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const T gx = g2[(2 * c) / V][(2 * c) % V], gy = g2[(2 * c) / V][(2 * c) % V + 1];
        const T pic = sgn * pi[c];
        nr[c] += (double)(pr[c] * gx - pic * gy);
        ni[c] += (double)(pr[c] * gy + pic * gx);
        dn[c] += (double)(q[c] * (gx * gx + gy * gy));
      }
    }
  }
  if (seg > 0) {
#pragma unroll
    for (int c = 0; c < V; ++c) {
      s_part[seg - 1][0][lane][c] = nr[c];
      s_part[seg - 1][1][lane][c] = ni[c];
      s_part[seg - 1][2][lane][c] = dn[c];
    }
  }
  __syncthreads();
  if (seg == 0 && ok) {
#pragma unroll
    for (int g = 0; g < 3; ++g) {
#pragma unroll
      for (int c = 0; c < V; ++c) {
        nr[c] += s_part[g][0][lane][c];
        ni[c] += s_part[g][1][lane][c];
        dn[c] += s_part[g][2][lane][c];
      }
    }
    const long long plane = (long long)nants * nfreqs;
#pragma unroll
    for (int c = 0; c < V; ++c) {
      if (f + c < nfreqs) {
        const long long o = (long long)a * nfreqs + f + c;
        planes[o] = nr[c];
        planes[plane + o] = ni[c];
        planes[2 * plane + o] = dn[c];
      }
    }
  }
}

// One thread per (antenna, channel < nfreqs): g <- (1 - damping) g + damping num / den, evaluated in double and rounded to T once.
// Antennas of a slice whose mask byte is 0 (slice_mask == nullptr: every slice is selected), channels with den <= 0 (no unflagged
// baseline, or one side of the exchange has gone non-finite) and the padding [nfreqs, fpad) are not written.
template <typename T>
__global__ __launch_bounds__(256) void gain_solve_apply_kernel(vec2_t<T>* __restrict__ gains, const double* __restrict__ planes,
                                                                const unsigned char* __restrict__ slice_mask, int na_slice, int nants, int nfreqs,
                                                                int fpad, double damping) {
  const long long n = (long long)nants * nfreqs;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int a = (int)(idx / nfreqs);
  const int f = (int)(idx - (long long)a * nfreqs);
  if (slice_mask && !slice_mask[a / na_slice]) return;
  const double den = planes[2 * n + idx];
  if (!(den > 0.0)) return;
  vec2_t<T>* g = gains + (long long)a * fpad + f;
  const vec2_t<T> old = *g;
  vec2_t<T> out;
  out.x = (T)((1.0 - damping) * (double)old.x + damping * (planes[idx] / den));
  out.y = (T)((1.0 - damping) * (double)old.y + damping * (planes[n + idx] / den));
  *g = out;
}

}  // namespace calk
