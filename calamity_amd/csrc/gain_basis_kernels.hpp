// gain_basis_kernels.hpp -- gains confined to a smooth frequency basis (cal_solver_set_gain_basis):
//   g_a(f) = g0_a(f) + sum_k B(f, k) y_a(k),   B real [nfreqs][nvec], shared by every antenna; y complex, the optimizer's variables.
// The fused kernels and gain_grad_kernel keep working on the per-channel arrays.  Two kernels sit around the update kernels, which
// run on the flat y arrays ([nants][kpad][2], row length kpad in place of fpad):
//   gain_project_kernel   grad y = grad g @ B   (the chain rule; B real, so re and im project independently, and so does every plane
//                         of the regulariser's two-adjoint-set form: the fold with alpha is linear and comes after the exchange)
//   gain_expand_kernel    g = g0 + B y
// Both sum in a fixed order (no float atomics: bitwise run-to-run reproducible) with fma_ spelled out, read the basis with
// unconditional 16-byte loads (the device copies are zero-padded to [fpad][kpad] and, transposed, [kpad][fpad]) and hold their
// accumulators in registers (no scratch).  kpad = nvec rounded up to kGainBasisPad: a row of y is then a whole number of 16-byte
// vectors for both dtypes, which is also what adam2_kernel's vector path wants of a row.
#pragma once
#include "fit_kernels.hpp"

namespace calk {

constexpr int kGainBasisPad = 8;

// block (a, plane): out[plane][a][k] = sum_f r[plane][a][f] B[f][k].  A thread owns V = 16 / sizeof(T) adjacent vectors k (one
// 16-byte load of a basis row) and every nseg-th channel, nseg = 256 / (kpad / V); the nseg partial sums of an output are added
// through LDS in ascending segment order.  More than 256 V vectors: tiles of 256 V, one after the other (correct for any nvec;
// fast for the few tens of vectors a smooth gain needs).  Rows of a stopped slice of several are written as zeros, as
// gain_grad_kernel does with its own: they are part of the exchange payload.
template <typename T>
__global__ __launch_bounds__(256) void gain_project_kernel(const vec2_t<T>* __restrict__ r, const T* __restrict__ B, T* __restrict__ out, int nants,
                                                            int fpad, int kpad, const DevState* st, const SliceMap M) {
  using T2 = vec2_t<T>;
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  __shared__ T s_part[256 * 2 * V];  // [segment][vector group][V][re, im]
  const int a = blockIdx.x, plane = blockIdx.y, tid = threadIdx.x;
  r += ((size_t)plane * nants + a) * fpad;
  out += ((size_t)plane * nants + a) * kpad * 2;
  if (M.nslices > 1) st += a / M.na_slice;
  const bool stopped = (st->done | st->done_after) != 0;  // the same for the whole block
  const int nq = kpad / V;
  for (int q0 = 0; q0 < nq; q0 += 256) {
    const int kw = nq - q0 < 256 ? nq - q0 : 256;
    const int nout = kw * 2 * V;
    if (stopped) {
      if (M.nslices > 1)
        for (int o = tid; o < nout; o += 256) out[(size_t)q0 * 2 * V + o] = (T)0;
      continue;
    }
    const int nseg = 256 / kw;
    const int seg = tid / kw, kq = tid - seg * kw;
    T acc[2 * V];
#pragma unroll
    for (int c = 0; c < 2 * V; ++c) acc[c] = (T)0;
    if (seg < nseg) {
      const T* bp = B + (size_t)(q0 + kq) * V;
#pragma unroll 4
      for (int f = seg; f < fpad; f += nseg) {
        const vec_t b = *reinterpret_cast<const vec_t*>(bp + (size_t)f * kpad);
        const T2 x = r[f];
#pragma unroll
        for (int j = 0; j < V; ++j) {
          acc[2 * j] = fma_(b[j], x.x, acc[2 * j]);
          acc[2 * j + 1] = fma_(b[j], x.y, acc[2 * j + 1]);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 2 * V; ++c) s_part[tid * 2 * V + c] = acc[c];
    __syncthreads();
    // output o = (vector group, component) lies at s_part[segment * nout + o]
    for (int o = tid; o < nout; o += 256) {
      T sum = s_part[o];
      for (int s = 1; s < nseg; ++s) sum += s_part[s * nout + o];
      out[(size_t)q0 * 2 * V + o] = sum;
    }
    __syncthreads();
  }
}

// block (channel block, a): g[a][f] = g0[a][f] + sum_k B[f][k] y[a][k], k ascending; a thread owns V adjacent channels (one 16-byte
// load of a row of the transposed basis per vector), the antenna's coefficients pass through LDS 256 at a time.  The gains are a
// function of (g0, B, y) alone, so the kernel needs no loop state: a slice that did not update gets the gains it had.
template <typename T>
__global__ __launch_bounds__(256) void gain_expand_kernel(const vec2_t<T>* __restrict__ g0, const T* __restrict__ Bt, const vec2_t<T>* __restrict__ y,
                                                           vec2_t<T>* __restrict__ g, int fpad, int kpad) {
  using T2 = vec2_t<T>;
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  __shared__ T2 s_y[256];
  const int a = blockIdx.y, tid = threadIdx.x;
  const int f = ((int)blockIdx.x * 256 + tid) * V;  // fpad is a multiple of 8: a thread's channels are all inside the row or all outside
  const bool mine = f < fpad;
  y += (size_t)a * kpad;
  T acc[2 * V];
#pragma unroll
  for (int c = 0; c < 2 * V; ++c) acc[c] = (T)0;
  for (int k0 = 0; k0 < kpad; k0 += 256) {
    const int kn = kpad - k0 < 256 ? kpad - k0 : 256;
    if (tid < kn) s_y[tid] = y[k0 + tid];
    __syncthreads();
    if (mine) {
      const T* bp = Bt + (size_t)k0 * fpad + f;
#pragma unroll 4
      for (int k = 0; k < kn; ++k) {
        const vec_t b = *reinterpret_cast<const vec_t*>(bp + (size_t)k * fpad);
        const T2 c = s_y[k];
#pragma unroll
        for (int j = 0; j < V; ++j) {
          acc[2 * j] = fma_(b[j], c.x, acc[2 * j]);
          acc[2 * j + 1] = fma_(b[j], c.y, acc[2 * j + 1]);
        }
      }
    }
    __syncthreads();
  }
  if (!mine) return;
  const size_t idx = (size_t)a * fpad + f;
#pragma unroll
  for (int h = 0; h < 2; ++h) {  // V (re, im) pairs = two 16-byte vectors
    vec_t v = *reinterpret_cast<const vec_t*>(reinterpret_cast<const T*>(g0 + idx) + h * V);
#pragma unroll
    for (int c = 0; c < V; ++c) v[c] += acc[h * V + c];
    *reinterpret_cast<vec_t*>(reinterpret_cast<T*>(g + idx) + h * V) = v;
  }
}

}  // namespace calk
