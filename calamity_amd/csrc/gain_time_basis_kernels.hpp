// gain_time_basis_kernels.hpp -- gains smooth in time (cal_solver_set_gain_time_basis): the solver holds T time slices as ONE fit
// (nants = T Na, antenna a at time t is row t Na + a) and
//   g[t Na + a](f) = g0[t Na + a](f) + sum_l Bt(t, l) z_a,l(f),   Bt real [T][L], shared by every antenna and channel;
//   z_a,l(f) = sum_k B(f, k) y_a(l, k) with a frequency basis (gain_basis_kernels.hpp), y_a(l, f) without one.
// The optimizer's gain variables are y [Na][L][W] (re, im), W = kpad with a frequency basis, else fpad.  Two kernels contract over
// time around the update kernels; a row is W complex = 2 W reals, and since Bt is real every real of a row goes its own way:
//   gain_time_project_kernel   out[plane][a][l][.] = sum_t Bt[t][l] in[plane][t Na + a][.]   (the chain rule, behind gain_project_kernel)
//   gain_time_expand_kernel    z[t Na + a][.] = (g0 row) + sum_l Bt[t][l] y[a][l][.]          (in front of gain_expand_kernel)
// Both sum in a fixed ascending order with fma_ spelled out and no float atomics (bitwise run-to-run reproducible).  A thread owns 16
// bytes of a row and a tile of kTimeTile accumulator vectors in registers (no scratch); tiles beyond the first are further blocks
// (grid.y), which read the rows again: correct for any L <= T, fast for the few vectors a slow drift needs.  The element of Bt a
// thread multiplies with depends on the block and the loop counters only: it is wave-uniform and comes through scalar loads of the
// zero-padded device copies ([T][lpad] and, transposed, [L][tpad]; lpad, tpad multiples of kTimeTile: a tile is read unconditionally).
#pragma once
#include "fit_kernels.hpp"

namespace calk {

constexpr int kTimeTile = 8;

// grid (ceil(na * row / V / 256), ceil(nvec / kTimeTile), planes); in_plane: reals between the planes of `in`
template <typename T>
__global__ __launch_bounds__(256) void gain_time_project_kernel(const T* __restrict__ in, const T* __restrict__ Bt, T* __restrict__ out, int na, int ntimes,
                                                                 int nvec, int lpad, int row, size_t in_plane) {
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  const int nq = row / V;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)na * nq) return;
  const int a = (int)(e / nq), q = (int)(e - (long long)a * nq);
  const int l0 = (int)blockIdx.y * kTimeTile, plane = blockIdx.z;
  const T* src = in + (size_t)plane * in_plane + (size_t)a * row + (size_t)q * V;
  const size_t tstride = (size_t)na * row;
  const T* b = Bt + l0;
  vec_t acc[kTimeTile];
#pragma unroll
  for (int j = 0; j < kTimeTile; ++j)
#pragma unroll
    for (int c = 0; c < V; ++c) acc[j][c] = (T)0;
#pragma unroll 4
  for (int t = 0; t < ntimes; ++t) {
    const vec_t x = *reinterpret_cast<const vec_t*>(src + (size_t)t * tstride);
#pragma unroll
    for (int j = 0; j < kTimeTile; ++j) {
      const T w = b[(size_t)t * lpad + j];
#pragma unroll
      for (int c = 0; c < V; ++c) acc[j][c] = fma_(w, x[c], acc[j][c]);
    }
  }
  T* dst = out + (((size_t)plane * na + a) * nvec + l0) * row + (size_t)q * V;
#pragma unroll
  for (int j = 0; j < kTimeTile; ++j)
    if (l0 + j < nvec) *reinterpret_cast<vec_t*>(dst + (size_t)j * row) = acc[j];
}

// grid (ceil(na * row / V / 256), ceil(ntimes / kTimeTile)); g0: the rows the sum is added to (W = fpad: z are the gains), or null
// (W = kpad: z are the coefficients gain_expand_kernel reads).  A function of (g0, Bt, y) alone, like gain_expand_kernel.
template <typename T>
__global__ __launch_bounds__(256) void gain_time_expand_kernel(const T* __restrict__ g0, const T* __restrict__ BtT, const T* __restrict__ y, T* __restrict__ z,
                                                                int na, int ntimes, int nvec, int tpad, int row) {
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  const int nq = row / V;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)na * nq) return;
  const int a = (int)(e / nq), q = (int)(e - (long long)a * nq);
  const int t0 = (int)blockIdx.y * kTimeTile;
  const T* src = y + (size_t)a * nvec * row + (size_t)q * V;
  const T* b = BtT + t0;
  vec_t acc[kTimeTile];
#pragma unroll
  for (int j = 0; j < kTimeTile; ++j)
#pragma unroll
    for (int c = 0; c < V; ++c) acc[j][c] = (T)0;
#pragma unroll 4
  for (int l = 0; l < nvec; ++l) {
    const vec_t x = *reinterpret_cast<const vec_t*>(src + (size_t)l * row);
#pragma unroll
    for (int j = 0; j < kTimeTile; ++j) {
      const T w = b[(size_t)l * tpad + j];
#pragma unroll
      for (int c = 0; c < V; ++c) acc[j][c] = fma_(w, x[c], acc[j][c]);
    }
  }
#pragma unroll
  for (int j = 0; j < kTimeTile; ++j) {
    if (t0 + j >= ntimes) continue;
    const size_t idx = ((size_t)(t0 + j) * na + a) * row + (size_t)q * V;
    vec_t v = acc[j];
    if (g0) {
      v = *reinterpret_cast<const vec_t*>(g0 + idx);
#pragma unroll
      for (int c = 0; c < V; ++c) v[c] += acc[j][c];
    }
    *reinterpret_cast<vec_t*>(z + idx) = v;
  }
}

}  // namespace calk
