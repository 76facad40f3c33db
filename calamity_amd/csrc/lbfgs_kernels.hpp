// lbfgs_kernels.hpp -- L-BFGS over the optimizer's own variables (cal_solver_lbfgs): per slice its run of the gain variables (the gains
// [na_slice][fpad] (re, im) interleaved, or rows of y with a gain basis) and its run [coff[t], coff[t + 1]) of both coefficient planes.
// The loss and its gradient come from the solver's own passes; the kernels here are what sits between them.
//
// The variable space is one flat vector like that of the Gauss-Newton step: the gain variables (`go` reals), then the coefficient planes
// [2][ncoef].  Every vector the call keeps has that layout: the ring of history + 1 slots of (s, y), the saved x_k and g_k.  The slot that
// holds no pair (the free one) carries the direction d in its s half while the line search runs -- d is dead when the next pair is formed
// into it --, so the call holds 2 history + 4 vectors in T.  The solver's own arrays (x and its gradient) are read and written in place
// through an LbView (two base pointers: the gain part and the coefficient part).
//
// This is the vector-free form of L-BFGS: per slice the device keeps the Gram matrix of [s_j, y_j (every slot), g] and lbfgs_coeff_kernel
// runs the two-loop recursion (lbfgs_core.hpp) on 2 p + 1 coefficients.  An iteration reads the history twice (the dot products of the new
// pair, the combination d = sum delta_j b_j), not 2 p times in sequence.
//   lbfgs_pair_kernel       s = x - x_k, y = g - g_k into the free slot, x_k := x, g_k := g, and in the same read the partials of the dot
//                           products of {s, y, g} with each other, then (tiles of kLbTile slots) with every stored pair
//   lbfgs_reduce_kernel     one wave per dot product of a slice: the block partials in block order
//   lbfgs_coeff_kernel      per slice: closes the iteration (loss, curvature test, ring, stop tests) and plans the next direction
//   lbfgs_direction_kernel  d = sum delta_j b_j in one read of the history
//   lbfgs_trial_kernel      x = x_k + t d of the slices still searching (steepest descent reads -g_k: no d is formed for it)
//   lbfgs_armijo_kernel     per slice accept or shrink, and the one integer the host reads per trial round
//   lbfgs_restore_kernel    x = x_k for the slices that stalled
// Padding (channels [nfreqs, fpad) of a gain row, the basis padding of a row of y) takes part in no sum and is zero in s, y and d; the saved
// x_k keeps the padding's own bits, so a trial or a restore writes back exactly what was there.
// Sums: double, per thread ascending over its chunks, a butterfly over the wave, the four waves in order, the blocks in order.  Elements are
// dealt to threads by their index RELATIVE to the slice's own runs and the block count comes from the slice's own sizes, so a slice of a
// batch gives the bits of the same slice alone; only whether a chunk is loaded as one 16-byte vector depends on where the run starts.
#pragma once
#include "fit_kernels.hpp"
#include "lbfgs_core.hpp"

namespace calk {

constexpr int kLbBlocks = 1024;                          // most blocks per slice of the vector kernels
constexpr int kLbChunksPerThread = 4;                    // fewer blocks while a thread would get fewer chunks than this
constexpr int kLbSlots = kLbfgsMaxHistory + 1;           // ring slots: one is always free
constexpr int kLbTile = 4;                               // stored pairs per tile of lbfgs_pair_kernel: 24 accumulators
constexpr int kLbOwn = 6 * kLbSlots;                     // dots: [slot][s.s_j, s.y_j, y.s_j, y.y_j, g.s_j, g.y_j], then s.s, s.y, y.y, s.g, y.g, g.g
constexpr int kLbDots = kLbOwn + 6;
constexpr int kLbM = 2 * kLbSlots + 1;                   // Gram matrix over physical vectors: s of slot j at j, y at kLbSlots + j, g last

struct LbState {  // per slice
  double f, f0, slope, t, gg;
  double gram[kLbM * kLbM];
  double delta[kLbM];      // d = sum delta_j b_j over physical vectors (zero for slots that hold no pair)
  int order[kLbSlots];     // the slots that hold pairs, oldest first
  int npairs, free_slot;
  int status, done, searching, moved, ever_moved, sd, ls, restore;
  int iters, evals, dropped, pad_;
};

struct LbSpace {
  const int* coff;       // [nslices + 1]
  long long ngs;         // gain reals per slice
  long long go;          // gain reals of all slices: where the coefficient planes begin
  int ncoef;
  int w, cols;           // complex elements per row of the gain variables, and how many of them are not padding
  int freeze;            // the coefficient runs are empty
  int nslot;             // history + 1 ring slots of (s, y), then x_k, g_k
};
template <typename T>
struct LbView {  // a vector in the flat layout whose two parts lie in arrays of their own
  T* a;
  T* c;
};
template <typename T>
__host__ __device__ inline LbView<T> lb_flat(T* p, long long go) { return LbView<T>{p, p + go}; }

struct LbParams {
  int nsteps, history, max_ls;
  double c1, shrink, ftol, curvature_eps;
};

// ---- how a slice's elements are dealt out -----------------------------------------------------------------------
template <int V>
struct LbCut {
  long long s0, s1, s2, l0, l1, c1, c2, chunks;  // flat starts of the three runs, lengths of the gain run and of a coefficient run; chunks before run 1, run 2; all chunks
  int nblk;
};
template <int V>
__device__ __forceinline__ LbCut<V> lb_cut(const LbSpace& S, int t) {
  LbCut<V> C;
  const long long nc = S.freeze ? 0 : (long long)(S.coff[t + 1] - S.coff[t]);
  C.s0 = (long long)t * S.ngs;
  C.l0 = S.ngs;
  C.s1 = S.go + S.coff[t];
  C.s2 = S.go + S.ncoef + S.coff[t];
  C.l1 = nc;
  C.c1 = (S.ngs + V - 1) / V;
  C.c2 = C.c1 + (nc + V - 1) / V;
  C.chunks = C.c2 + (nc + V - 1) / V;
  const long long per = 256ll * kLbChunksPerThread;
  const long long nb = (C.chunks + per - 1) / per;
  C.nblk = (int)(nb < 1 ? 1 : nb > kLbBlocks ? kLbBlocks : nb);
  return C;
}
// chunk q of the slice: its first flat index, how many of its V elements exist, whether it is loaded as one vector, its padding mask
template <int V>
struct LbChunk {
  long long base;
  int cnt;
  bool vec, gain;
};
template <int V>
__device__ __forceinline__ LbChunk<V> lb_chunk(const LbCut<V>& C, long long q) {
  const int r = q >= C.c2 ? 2 : q >= C.c1 ? 1 : 0;
  const long long off = (q - (r == 2 ? C.c2 : r == 1 ? C.c1 : 0)) * V;
  LbChunk<V> K;
  const long long start = r == 2 ? C.s2 : r == 1 ? C.s1 : C.s0;
  K.base = start + off;
  const long long left = (r == 0 ? C.l0 : C.l1) - off;
  K.cnt = left < V ? (int)left : V;
  K.gain = r == 0;
  K.vec = K.cnt == V && (start % V) == 0;  // (go is a multiple of V: the flat index and both parts' own indices align alike)
  return K;
}
template <typename T, int V>
__device__ __forceinline__ void lb_load(const LbView<T>& v, const LbSpace& S, const LbChunk<V>& K, T (&out)[V]) {
  typedef T vec_t __attribute__((ext_vector_type(V)));
  const T* p = K.gain ? v.a + K.base : v.c + (K.base - S.go);
  if (K.vec) {
    const vec_t x = *reinterpret_cast<const vec_t*>(p);
#pragma unroll
    for (int c = 0; c < V; ++c) out[c] = x[c];
  } else {
#pragma unroll
    for (int c = 0; c < V; ++c) out[c] = c < K.cnt ? p[c] : (T)0;
  }
}
template <typename T, int V>
__device__ __forceinline__ void lb_store(const LbView<T>& v, const LbSpace& S, const LbChunk<V>& K, const T (&in)[V]) {
  typedef T vec_t __attribute__((ext_vector_type(V)));
  T* p = K.gain ? v.a + K.base : v.c + (K.base - S.go);
  if (K.vec) {
    vec_t x;
#pragma unroll
    for (int c = 0; c < V; ++c) x[c] = in[c];
    *reinterpret_cast<vec_t*>(p) = x;
  } else {
#pragma unroll
    for (int c = 0; c < V; ++c)
      if (c < K.cnt) p[c] = in[c];
  }
}
// element c of the chunk takes part in the sums: it exists and is no padding
template <int V>
__device__ __forceinline__ bool lb_live(const LbSpace& S, const LbChunk<V>& K, int c) {
  if (c >= K.cnt) return false;
  return !K.gain || (int)(((K.base + c) >> 1) % S.w) < S.cols;
}
// the block's sums of n accumulators into part[(k0 + k) * kLbBlocks + block]
template <int N>
__device__ __forceinline__ void lb_block_sums(const double (&acc)[N], double* s_w, double* __restrict__ part, int k0) {
  __syncthreads();  // (s_w may still be read from the tile before)
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double v = ldsum(acc[k]);
    if ((threadIdx.x & 63) == 0) s_w[k * 4 + (threadIdx.x >> 6)] = v;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    const int k = threadIdx.x;
    part[(long long)(k0 + k) * kLbBlocks + blockIdx.x] = ((s_w[k * 4] + s_w[k * 4 + 1]) + s_w[k * 4 + 2]) + s_w[k * 4 + 3];
  }
}

// grid (kLbBlocks, nslices).  init: x_k := x, g_k := g and g . g alone, for every slice that is not done; else the slices that moved.
template <typename T>
__global__ __launch_bounds__(256) void lbfgs_pair_kernel(const LbSpace S, const LbView<T> x, const LbView<T> g, T* __restrict__ vec, long long np,
                                                          const LbState* __restrict__ state, double* __restrict__ part_all, int init) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  __shared__ double s_w[6 * kLbTile * 4];
  const int t = blockIdx.y;
  const LbState& st = state[t];
  if (st.done || (!init && !st.moved)) return;
  const LbCut<V> C = lb_cut<V>(S, t);
  if ((int)blockIdx.x >= C.nblk) return;
  double* part = part_all + (long long)t * kLbDots * kLbBlocks;
  const int f = st.free_slot, npairs = st.npairs;
  const LbView<T> xk = lb_flat(vec + 2ll * S.nslot * np, S.go), gk = lb_flat(vec + (2ll * S.nslot + 1) * np, S.go);
  const LbView<T> sf = lb_flat(vec + 2ll * f * np, S.go), yf = lb_flat(vec + (2ll * f + 1) * np, S.go);
  const long long q0 = (long long)blockIdx.x * 256 + threadIdx.x, dq = (long long)C.nblk * 256;
  {
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (long long q = q0; q < C.chunks; q += dq) {
      const LbChunk<V> K = lb_chunk<V>(C, q);
      T xn[V], gn[V], xo[V], go_[V], s[V], y[V];
      lb_load<T, V>(x, S, K, xn);
      lb_load<T, V>(g, S, K, gn);
      if (!init) {
        lb_load<T, V>(xk, S, K, xo);
        lb_load<T, V>(gk, S, K, go_);
      }
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const bool live = lb_live<V>(S, K, c);
        if (!live) gn[c] = (T)0;
        if (!init) {
          s[c] = live ? (T)((double)xn[c] - (double)xo[c]) : (T)0;
          y[c] = live ? (T)((double)gn[c] - (double)go_[c]) : (T)0;
          const double sd = (double)s[c], yd = (double)y[c], gd = (double)gn[c];
          acc[0] += sd * sd;
          acc[1] += sd * yd;
          acc[2] += yd * yd;
          acc[3] += sd * gd;
          acc[4] += yd * gd;
        }
        acc[5] += (double)gn[c] * (double)gn[c];
      }
      if (!init) {
        lb_store<T, V>(sf, S, K, s);
        lb_store<T, V>(yf, S, K, y);
      }
      lb_store<T, V>(xk, S, K, xn);
      lb_store<T, V>(gk, S, K, gn);
    }
    lb_block_sums<6>(acc, s_w, part, kLbOwn);
  }
  if (init) return;
  // the new pair and g against the stored pairs, kLbTile slots at a time (the thread reads back what it wrote above)
  for (int j0 = 0; j0 < npairs; j0 += kLbTile) {
    double acc[kLbTile][6];
#pragma unroll
    for (int j = 0; j < kLbTile; ++j)
#pragma unroll
      for (int k = 0; k < 6; ++k) acc[j][k] = 0;
    int slot[kLbTile];
#pragma unroll
    for (int j = 0; j < kLbTile; ++j) slot[j] = j0 + j < npairs ? st.order[j0 + j] : -1;
    for (long long q = q0; q < C.chunks; q += dq) {
      const LbChunk<V> K = lb_chunk<V>(C, q);
      T s[V], y[V], gn[V];
      lb_load<T, V>(sf, S, K, s);
      lb_load<T, V>(yf, S, K, y);
      lb_load<T, V>(gk, S, K, gn);
#pragma unroll
      for (int j = 0; j < kLbTile; ++j) {
        if (slot[j] >= 0) {  // block-uniform
        T sj[V], yj[V];
        lb_load<T, V>(lb_flat(vec + 2ll * slot[j] * np, S.go), S, K, sj);
        lb_load<T, V>(lb_flat(vec + (2ll * slot[j] + 1) * np, S.go), S, K, yj);
#pragma unroll
        for (int c = 0; c < V; ++c) {  // (padding and elements past the run are zero in every stored vector)
          const double a = (double)sj[c], b = (double)yj[c];
          acc[j][0] += (double)s[c] * a;
          acc[j][1] += (double)s[c] * b;
          acc[j][2] += (double)y[c] * a;
          acc[j][3] += (double)y[c] * b;
          acc[j][4] += (double)gn[c] * a;
          acc[j][5] += (double)gn[c] * b;
        }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kLbTile; ++j)
      if (slot[j] >= 0) lb_block_sums<6>(acc[j], s_w, part, 6 * slot[j]);  // block-uniform
  }
}

// grid (nslices, (kLbDots + 3) / 4), 256 threads: one wave per dot product, lane l adds the partials l, l + 64, .. in order, then the butterfly
template <int V>
__global__ __launch_bounds__(256) void lbfgs_reduce_kernel(const LbSpace S, const LbState* __restrict__ state, const double* __restrict__ part_all,
                                                            double* __restrict__ dots, int init) {
  const int t = blockIdx.x, k = blockIdx.y * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const LbState& st = state[t];
  if (k >= kLbDots || st.done || (!init && !st.moved)) return;
  if (k < kLbOwn) {
    bool held = false;
    for (int j = 0; j < st.npairs; ++j) held = held || st.order[j] == k / 6;
    if (!held || init) return;
  }
  const int nblk = lb_cut<V>(S, t).nblk;
  const double* part = part_all + ((long long)t * kLbDots + k) * kLbBlocks;
  double v = 0;
  for (int b = lane; b < nblk; b += 64) v += part[b];
  v = ldsum(v);
  if (lane == 0) dots[(long long)t * kLbDots + k] = v;
}

__device__ __forceinline__ void lb_steepest(LbState& st) {  // d = -g_k: no pairs, the first step length from the gradient's norm
  st.npairs = 0;
  st.sd = 1;
  st.slope = -st.gg;
  const double n = sqrt(st.gg);
  st.t = n > 1.0 ? 1.0 / n : 1.0;
  st.ls = 0;
}

// grid (nslices), 64 threads, lane 0 works: the iteration that the gradient pass before it ended is closed (loss_k[iters] := the pass's
// loss, the pair enters the ring iff s . y > eps sqrt(s . s y . y), stop tests), then the next direction is planned from the Gram matrix
__global__ __launch_bounds__(64) void lbfgs_coeff_kernel(LbState* __restrict__ state, const double* __restrict__ dots_all, const DevState* __restrict__ dev,
                                                          double* __restrict__ losses, const LbParams P, int init) {
  __shared__ int s_idx[kLbfgsMaxBasis];
  __shared__ double s_delta[kLbfgsMaxBasis], s_alpha[kLbfgsMaxHistory];
  if (threadIdx.x != 0) return;
  const int t = blockIdx.x;
  LbState& st = state[t];
  st.restore = 0;
  if (st.done) return;
  const double* dots = dots_all + (long long)t * kLbDots;
  const double fnew = dev[t].loss;
  double* loss_t = losses + (long long)t * (P.nsteps + 1);
  const int G = kLbM - 1;
  if (init) {
    const double gg = dots[kLbOwn + 5];
    if (!isfinite(fnew) || !isfinite(gg) || !(gg > 0.0)) {
      st.status = 3;
      st.done = 1;
      return;
    }
    st.f = st.f0 = fnew;
    st.gg = gg;
    st.gram[G * kLbM + G] = gg;
    loss_t[0] = fnew;
  } else {
    if (!st.moved) return;  // (every slice that is not done has moved: a stalled one is done)
    st.moved = 0;
    const double ss = dots[kLbOwn], sy = dots[kLbOwn + 1], yy = dots[kLbOwn + 2], sg = dots[kLbOwn + 3], yg = dots[kLbOwn + 4];
    st.gg = dots[kLbOwn + 5];
    st.gram[G * kLbM + G] = st.gg;
    for (int a = 0; a < st.npairs; ++a) {  // g against the pairs held
      const int j = st.order[a];
      st.gram[G * kLbM + j] = st.gram[j * kLbM + G] = dots[6 * j + 4];
      st.gram[G * kLbM + kLbSlots + j] = st.gram[(kLbSlots + j) * kLbM + G] = dots[6 * j + 5];
    }
    if (isfinite(sy) && sy > P.curvature_eps * sqrt(ss * yy)) {
      const int fs = st.free_slot, fy = kLbSlots + fs;
      int evicted = -1;
      if (st.npairs == P.history) {
        evicted = st.order[0];
        for (int a = 1; a < st.npairs; ++a) st.order[a - 1] = st.order[a];
        --st.npairs;
      }
      for (int a = 0; a < st.npairs; ++a) {
        const int j = st.order[a], jy = kLbSlots + j;
        st.gram[fs * kLbM + j] = st.gram[j * kLbM + fs] = dots[6 * j];
        st.gram[fs * kLbM + jy] = st.gram[jy * kLbM + fs] = dots[6 * j + 1];
        st.gram[fy * kLbM + j] = st.gram[j * kLbM + fy] = dots[6 * j + 2];
        st.gram[fy * kLbM + jy] = st.gram[jy * kLbM + fy] = dots[6 * j + 3];
      }
      st.gram[fs * kLbM + fs] = ss;
      st.gram[fs * kLbM + fy] = st.gram[fy * kLbM + fs] = sy;
      st.gram[fy * kLbM + fy] = yy;
      st.gram[G * kLbM + fs] = st.gram[fs * kLbM + G] = sg;
      st.gram[G * kLbM + fy] = st.gram[fy * kLbM + G] = yg;
      st.order[st.npairs++] = fs;
      if (evicted >= 0) {
        st.free_slot = evicted;
      } else {
        for (int j = 0; j <= P.history; ++j) {  // the first slot that holds no pair
          bool held = false;
          for (int a = 0; a < st.npairs; ++a) held = held || st.order[a] == j;
          if (!held) {
            st.free_slot = j;
            break;
          }
        }
      }
    } else {
      ++st.dropped;
    }
    const double fk = st.f;
    st.f = fnew;
    loss_t[++st.iters] = fnew;
    if (P.ftol > 0.0 && fk - fnew <= P.ftol * fabs(fk)) {
      st.status = 1;
      st.done = 1;
    } else if (st.iters >= P.nsteps) {
      st.status = 0;
      st.done = 1;
    }
    if (st.done) return;
  }
  // the next direction
  for (int j = 0; j < kLbM; ++j) st.delta[j] = 0.0;
  bool quasi = st.npairs > 0;
  if (quasi) {
    const int p = st.npairs;
    for (int a = 0; a < p; ++a) {
      s_idx[a] = st.order[a];
      s_idx[p + a] = kLbSlots + st.order[a];
    }
    s_idx[2 * p] = G;
    const double slope = lbfgs_two_loop(p, st.gram, kLbM, s_idx, s_delta, s_alpha);
    if (isfinite(slope) && slope < 0.0) {
      for (int a = 0; a <= 2 * p; ++a) st.delta[s_idx[a]] = s_delta[a];
      st.slope = slope;
      st.t = 1.0;
      st.sd = 0;
      st.ls = 0;
    } else {
      st.dropped += p;
      quasi = false;
    }
  }
  if (!quasi) lb_steepest(st);
  st.searching = 1;
}

// grid (kLbBlocks, nslices): d into the s half of the free slot, for the slices that search along a quasi-Newton direction
template <typename T>
__global__ __launch_bounds__(256) void lbfgs_direction_kernel(const LbSpace S, T* __restrict__ vec, long long np, const LbState* __restrict__ state) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  const int t = blockIdx.y;
  const LbState& st = state[t];
  if (st.done || !st.searching || st.sd) return;
  const LbCut<V> C = lb_cut<V>(S, t);
  if ((int)blockIdx.x >= C.nblk) return;
  const LbView<T> gk = lb_flat(vec + (2ll * S.nslot + 1) * np, S.go), d = lb_flat(vec + 2ll * st.free_slot * np, S.go);
  const double dg = st.delta[kLbM - 1];
  const int npairs = st.npairs;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < C.chunks; q += (long long)C.nblk * 256) {
    const LbChunk<V> K = lb_chunk<V>(C, q);
    T v[V];
    double acc[V];
    lb_load<T, V>(gk, S, K, v);
#pragma unroll
    for (int c = 0; c < V; ++c) acc[c] = dg * (double)v[c];
    for (int a = 0; a < npairs; ++a) {  // oldest first
      const int j = st.order[a];
      const double ds = st.delta[j], dy = st.delta[kLbSlots + j];
      T w[V];
      lb_load<T, V>(lb_flat(vec + 2ll * j * np, S.go), S, K, v);
      lb_load<T, V>(lb_flat(vec + (2ll * j + 1) * np, S.go), S, K, w);
#pragma unroll
      for (int c = 0; c < V; ++c) acc[c] = (acc[c] + ds * (double)v[c]) + dy * (double)w[c];
    }
#pragma unroll
    for (int c = 0; c < V; ++c) v[c] = lb_live<V>(S, K, c) ? (T)acc[c] : (T)0;
    lb_store<T, V>(d, S, K, v);
  }
}

// grid (kLbBlocks, nslices): x = x_k + t d, in double from the stored values and rounded once; padding keeps the bits of x_k
template <typename T>
__global__ __launch_bounds__(256) void lbfgs_trial_kernel(const LbSpace S, const LbView<T> x, const T* __restrict__ vec, long long np,
                                                           const LbState* __restrict__ state) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  const int t = blockIdx.y;
  const LbState& st = state[t];
  if (st.done || !st.searching) return;
  const LbCut<V> C = lb_cut<V>(S, t);
  if ((int)blockIdx.x >= C.nblk) return;
  T* base = const_cast<T*>(vec);
  const LbView<T> xk = lb_flat(base + 2ll * S.nslot * np, S.go);
  const LbView<T> d = st.sd ? lb_flat(base + (2ll * S.nslot + 1) * np, S.go) : lb_flat(base + 2ll * st.free_slot * np, S.go);
  const double step = st.sd ? -st.t : st.t;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < C.chunks; q += (long long)C.nblk * 256) {
    const LbChunk<V> K = lb_chunk<V>(C, q);
    T a[V], b[V];
    lb_load<T, V>(xk, S, K, a);
    lb_load<T, V>(d, S, K, b);
#pragma unroll
    for (int c = 0; c < V; ++c)
      if (lb_live<V>(S, K, c)) a[c] = (T)((double)a[c] + step * (double)b[c]);
    lb_store<T, V>(x, S, K, a);
  }
}

// one block: per slice accept iff the trial loss is finite and <= f + c1 t slope, else shrink; a search that runs out drops the pairs and
// starts over along -g_k, and without pairs the slice stalls (status 2).  *count = the slices still searching, or -1 once no slice is
// searching and every slice is done: the one integer the host reads per trial round.
__global__ __launch_bounds__(256) void lbfgs_armijo_kernel(LbState* __restrict__ state, const DevState* __restrict__ dev, int nslices, const LbParams P,
                                                            int* __restrict__ count) {
  __shared__ int s_search[256], s_active[256];
  int nsearch = 0, nactive = 0;
  for (int t = threadIdx.x; t < nslices; t += 256) {
    LbState& st = state[t];
    if (!st.done && st.searching) {
      ++st.evals;
      const double ft = dev[t].loss;
      if (isfinite(ft) && ft <= st.f + P.c1 * st.t * st.slope) {
        st.searching = 0;
        st.moved = st.ever_moved = 1;
      } else {
        st.t *= P.shrink;
        if (++st.ls >= P.max_ls) {
          if (st.npairs > 0) {
            st.dropped += st.npairs;
            lb_steepest(st);
          } else {
            st.status = 2;
            st.done = 1;
            st.searching = 0;
            st.restore = 1;
          }
        }
      }
    }
    nsearch += !st.done && st.searching;
    nactive += !st.done;
  }
  s_search[threadIdx.x] = nsearch;
  s_active[threadIdx.x] = nactive;
  __syncthreads();
  if (threadIdx.x == 0) {
    nsearch = nactive = 0;
    for (int k = 0; k < 256; ++k) {
      nsearch += s_search[k];
      nactive += s_active[k];
    }
    *count = nsearch > 0 ? nsearch : nactive > 0 ? 0 : -1;
  }
}

// grid (kLbBlocks, nslices): the bits of x_k back for the slices that stalled in the search just ended
template <typename T>
__global__ __launch_bounds__(256) void lbfgs_restore_kernel(const LbSpace S, const LbView<T> x, const T* __restrict__ vec, long long np,
                                                             const LbState* __restrict__ state) {
  constexpr int V = 16 / (int)sizeof(T);
  const int t = blockIdx.y;
  if (!state[t].restore) return;
  const LbCut<V> C = lb_cut<V>(S, t);
  if ((int)blockIdx.x >= C.nblk) return;
  const LbView<T> xk = lb_flat(const_cast<T*>(vec) + 2ll * S.nslot * np, S.go);
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < C.chunks; q += (long long)C.nblk * 256) {
    const LbChunk<V> K = lb_chunk<V>(C, q);
    T a[V];
    lb_load<T, V>(xk, S, K, a);
    lb_store<T, V>(x, S, K, a);
  }
}

}  // namespace calk
