// robust_weight_kernels.hpp -- downweight outliers from the residual (cal_solver_robust_weights): iteratively reweighted least squares.
// With w0 the weights as cal_solver_set_data gave them, (i, j) the antennas of baseline row b, m = A c (MODE_MODEL's planes), g the gains:
//   e[b][f]  = w0[b][f] |d[b][f] - g_i[f] conj(g_j[f]) m[b][f]|^2      (products in T, in quality_rows_kernel's order)
//   S_b      = { f < nfreqs : w0[b][f] > 0 },  n_b = |S_b|
//   med_b    = the ((n_b + 1) / 2)-th smallest of e[b][S_b]             (the lower median: an element of the row, never an average)
//   scale_b  = med_b / ln 2                                             (w |r|^2 of complex Gaussian residuals is exponential: median = ln 2 mean)
//   z2       = e / scale_b                                              (scale_b, z2 and psi in double)
//   huber  : psi = 1 if z2 <= k^2 else k / sqrt(z2)
//   cauchy : psi = 1 / (1 + z2 / k^2)
//   clip   : psi = 1 if z2 <= k^2 else 0
//   w[b][f]  = (T)(w0[b][f] * psi)        for f in S_b; every other channel keeps w0 (the padding keeps its zero)
// Rows with n_b = 0 or med_b not > 0 keep w = w0 and report scale 0, count 0.  Every call starts from w0, never from the previous w.
// One kernel behind the model pass:
//   robust_rows_kernel   one wave per baseline row: e, its exact lower median, the new weights over wgts, scale_b and the count of psi < 1
// The median needs no sort and no float atomics: e >= 0, so with the sign bit cleared its IEEE bit pattern orders like an unsigned
// integer, and the k-th smallest pattern is built from the top bit down -- per bit one count of the keys below the trial pattern
// (31 rounds in float, 63 in double).  A count is a compare per key whose lane mask the scalar unit pops (ballot): no LDS crossbar, no
// reduction tree, an integer -- two calls give the same bits.  A NaN (sign cleared) orders above every number, samples outside S_b carry
// the all-ones pattern, above every NaN: the search runs its fixed number of rounds whatever the row holds.
#pragma once
#include "fit_kernels.hpp"

namespace calk {

enum { kRobustNone = 0, kRobustHuber = 1, kRobustCauchy = 2, kRobustClip = 3 };

template <typename T> struct RobustKey;
template <> struct RobustKey<float> { typedef unsigned type; static constexpr int bits = 31; };
template <> struct RobustKey<double> { typedef unsigned long long type; static constexpr int bits = 63; };

// rows per block and the longest row whose keys stay in LDS (64 KB a block): 4096 channels in float, 2048 in double
constexpr int kRobustRows = 4;
template <typename T> constexpr int robust_lds_fpad() { return 65536 / (kRobustRows * (int)sizeof(T)); }

// One wave per baseline row, four rows per block; a lane owns V = 16 / sizeof(T) adjacent channels per trip (16-byte loads of the
// five planes, 2 x 16 bytes of each antenna's interleaved gains).  A lane reads back only the keys it wrote itself, so neither form
// needs a barrier:
//   LDS = true    the row's keys in dynamic LDS, kRobustRows * fpad keys a block (fpad <= robust_lds_fpad<T>())
//   LDS = false   longer rows: the keys in the row of the model_r plane (HBM / L2), the same rounds, slower, the same bits
// Rows of a slice that slice_mask leaves out (slice = first antenna row / na_slice) are not touched at all; kind = kRobustNone copies w0 back.
template <typename T, bool LDS>
__global__ __launch_bounds__(256) void robust_rows_kernel(T* __restrict__ model_r, const T* __restrict__ model_i, const T* __restrict__ data_r,
                                                           const T* __restrict__ data_i, const T* __restrict__ w0, T* __restrict__ wgts,
                                                           const vec2_t<T>* __restrict__ gains, const int2* __restrict__ bl_ant,
                                                           const unsigned char* __restrict__ slice_mask, int na_slice, int nbls, int nfreqs, int fpad,
                                                           int kind, double k, double* __restrict__ scale_bl, double* __restrict__ ndown_bl) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  typedef typename RobustKey<T>::type key_t;
  typedef key_t kvec_t __attribute__((ext_vector_type(V)));
  extern __shared__ __attribute__((aligned(16))) unsigned char robust_lds[];
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * kRobustRows + (threadIdx.x >> 6);  // wave-uniform
  if (b >= nbls) return;
  const int2 ant = bl_ant[b];
  if (slice_mask && !slice_mask[ant.x / na_slice]) return;
  const long long row = (long long)b * fpad;
  if (kind == kRobustNone) {
    for (int f = lane * V; f < fpad; f += 64 * V) *reinterpret_cast<vec_t*>(wgts + row + f) = *reinterpret_cast<const vec_t*>(w0 + row + f);
    if (lane == 0) scale_bl[b] = ndown_bl[b] = 0.0;
    return;
  }
  key_t* keys;
  if constexpr (LDS)
    keys = reinterpret_cast<key_t*>(robust_lds) + (size_t)(threadIdx.x >> 6) * fpad;
  else
    keys = reinterpret_cast<key_t*>(model_r + row);
  const vec2_t<T>* __restrict__ ga = gains + (long long)ant.x * fpad;
  const vec2_t<T>* __restrict__ gb = gains + (long long)ant.y * fpad;
  constexpr key_t kOut = ~(key_t)0, kAbs = kOut >> 1;
  int n = 0;
  for (int base = 0; base < fpad; base += 64 * V) {  // fpad is a multiple of 8: whole vectors; the trip count is wave-uniform
    const int f = base + lane * V;
    if (f < fpad) {
      const vec_t mr = *reinterpret_cast<const vec_t*>(model_r + row + f);
      const vec_t mi = *reinterpret_cast<const vec_t*>(model_i + row + f);
      const vec_t dr = *reinterpret_cast<const vec_t*>(data_r + row + f);
      const vec_t di = *reinterpret_cast<const vec_t*>(data_i + row + f);
      const vec_t w = *reinterpret_cast<const vec_t*>(w0 + row + f);
      vec_t a2[2], b2[2];  // V channels of (re, im)
      a2[0] = *reinterpret_cast<const vec_t*>(ga + f);
      a2[1] = *reinterpret_cast<const vec_t*>(ga + f + V / 2);
      b2[0] = *reinterpret_cast<const vec_t*>(gb + f);
      b2[1] = *reinterpret_cast<const vec_t*>(gb + f + V / 2);
      kvec_t kv;
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const T g0x = a2[(2 * c) / V][(2 * c) % V], g0y = a2[(2 * c) / V][(2 * c) % V + 1];
        const T g1x = b2[(2 * c) / V][(2 * c) % V], g1y = b2[(2 * c) / V][(2 * c) % V + 1];
        const T G_r = g0x * g1x + g0y * g1y;  // g0 conj(g1), as quality_rows_kernel
        const T G_i = g0y * g1x - g0x * g1y;
        const T m_r = G_r * mr[c] - G_i * mi[c];
        const T m_i = G_i * mr[c] + G_r * mi[c];
        const T r_r = dr[c] - m_r;
        const T r_i = di[c] - m_i;
        const T ec = w[c] * (r_r * r_r + r_i * r_i);
        const bool in = f + c < nfreqs && w[c] > (T)0;
        kv[c] = in ? (__builtin_bit_cast(key_t, ec) & kAbs) : kOut;
        n += in ? 1 : 0;
      }
      *reinterpret_cast<kvec_t*>(keys + f) = kv;
    }
  }
  n = ldsum(n);
  double scale = 0.0;
  if (n > 0) {
    // the rank-th smallest key, from the top bit down: the bit is set when fewer than rank keys lie below the trial pattern
    const int rank = (n + 1) >> 1;
    key_t med = 0;
    for (int bit = RobustKey<T>::bits - 1; bit >= 0; --bit) {
      const key_t trial = med | ((key_t)1 << bit);
      int below = 0;  // wave-uniform
      for (int base = 0; base < fpad; base += 64 * V) {
        const int f = base + lane * V;
        kvec_t kv = kOut;  // (lanes past the row's end in its last trip: above every trial)
        if (f < fpad) kv = *reinterpret_cast<const kvec_t*>(keys + f);
#pragma unroll
        for (int c = 0; c < V; ++c) below += __popcll(__ballot(kv[c] < trial));
      }
      if (below < rank) med = trial;
    }
    const T medv = __builtin_bit_cast(T, med);
    if (medv > (T)0) scale = (double)medv / 0.693147180559945309417232121458;  // (a NaN median fails the comparison too)
  }
  int ndown = 0;
  for (int base = 0; base < fpad; base += 64 * V) {
    const int f = base + lane * V;
    if (f < fpad) {
      const kvec_t kv = *reinterpret_cast<const kvec_t*>(keys + f);
      vec_t w = *reinterpret_cast<const vec_t*>(w0 + row + f);
      if (scale > 0.0) {
#pragma unroll
        for (int c = 0; c < V; ++c) {
          const key_t key = kv[c];  // (a scalar copy: __builtin_bit_cast of a vector element reads element 0)
          if (key == kOut) continue;
          const double z2 = (double)__builtin_bit_cast(T, key) / scale;
          double psi;
          if (kind == kRobustHuber)
            psi = z2 <= k * k ? 1.0 : k / sqrt(z2);
          else if (kind == kRobustCauchy)
            psi = 1.0 / (1.0 + z2 / (k * k));
          else
            psi = z2 <= k * k ? 1.0 : 0.0;
          ndown += psi < 1.0 ? 1 : 0;
          w[c] = (T)((double)w[c] * psi);
        }
      }
      *reinterpret_cast<vec_t*>(wgts + row + f) = w;
    }
  }
  ndown = ldsum(ndown);
  if (lane == 0) {
    scale_bl[b] = scale;
    ndown_bl[b] = (double)ndown;
  }
}

}  // namespace calk
