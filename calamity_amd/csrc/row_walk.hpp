// row_walk.hpp -- the row walk the post-fit kernels share (fit quality, the closed-form solves, Gauss-Newton), defined once; device
// pieces only, no kernels.  One wave per baseline row, four rows per block; a lane owns V = 16 / sizeof(T) adjacent channels per trip.
// The kernel keeps the loop for (f = lane * V; f < fpad; f += 64 * V), writes zeros to the channels [nfreqs, fpad) and adds nothing
// for them; row sums go through ldsum (fit_kernels.hpp), the one full-wave butterfly.  `#pragma clang fp contract(off)` is lexical: a
// helper that multiplies carries it in its own body, because the pragma of the kernel that calls it does not reach it.
#pragma once
#include "fit_kernels.hpp"

namespace calk {

template <typename T>
struct RowWalk {
  static constexpr int V = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  int lane, b;  // b: wave-uniform
  int2 ant; long long row;
  __device__ __forceinline__ bool begin(const int2* __restrict__ bl_ant, int nbls, int fpad) {  // false: the wave has no row and returns
    lane = threadIdx.x & 63;
    b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= nbls) return false;
    ant = bl_ant[b];
    row = (long long)b * fpad;
    return true;
  }
  __device__ __forceinline__ vec_t load(const T* __restrict__ plane, int f) const { return *reinterpret_cast<const vec_t*>(plane + row + f); }
  __device__ __forceinline__ void store(T* __restrict__ plane, int f, vec_t v) const { *reinterpret_cast<vec_t*>(plane + row + f) = v; }
};

// The interleaved (re, im) gains of a row's two antennas: load(f) reads 2 x 16 bytes of each, at(c) gives channel f + c.
template <typename T>
struct GainPair {
  static constexpr int V = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  struct Chan { T ax, ay, bx, by, Gr, Gi; };  // g_i = (ax, ay), g_j = (bx, by), G = g_i conj(g_j)
  const vec2_t<T> *__restrict__ gi, *__restrict__ gj;
  vec_t a2[2], b2[2];  // V channels of (re, im)
  __device__ __forceinline__ GainPair(const vec2_t<T>* __restrict__ gains, int2 ant, int fpad)
      : gi(gains + (long long)ant.x * fpad), gj(gains + (long long)ant.y * fpad) {}
  __device__ __forceinline__ void load(int f) {
    a2[0] = *reinterpret_cast<const vec_t*>(gi + f);
    a2[1] = *reinterpret_cast<const vec_t*>(gi + f + V / 2);
    b2[0] = *reinterpret_cast<const vec_t*>(gj + f);
    b2[1] = *reinterpret_cast<const vec_t*>(gj + f + V / 2);
  }
  __device__ __forceinline__ Chan at(int c) const {
#pragma clang fp contract(off)
    Chan g;
    g.ax = a2[(2 * c) / V][(2 * c) % V], g.ay = a2[(2 * c) / V][(2 * c) % V + 1];
    g.bx = b2[(2 * c) / V][(2 * c) % V], g.by = b2[(2 * c) / V][(2 * c) % V + 1];
    g.Gr = g.ax * g.bx + g.ay * g.by;  // g_i conj(g_j), calibration.py:1598-1601
    g.Gi = g.ay * g.bx - g.ax * g.by;
    return g;
  }
};

}  // namespace calk
