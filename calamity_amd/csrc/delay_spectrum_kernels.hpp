// delay_spectrum_kernels.hpp -- where the power of data, model and residual sits in delay (cal_solver_delay_spectrum).  For baseline
// row b with antennas (i, j), G = g_i conj(g_j), m = A c (MODE_MODEL's planes) and mask = (w[b][f] != 0):
//   x_q[b][f]      = mask q[b][f],  q among  d, G m, d - G m   (calibrated: d / G, m, d / G - m, zero where |G|^2 == 0)
//   X_q[b][k]      = sum_f x_q[b][f] (op_r + i op_i)[f][k]
//   norm_bl[b]     = sum_f mask norm_f[f]
//   power[q][b][k] = |X_q[b][k]|^2 / norm_bl[b]      (0 where norm_bl[b] == 0)
//   power_bin[q][n][k] = sum of power[q][b][k] over the rows of bin n with norm_bl[b] > 0, in ascending b
// Three kernels behind the model pass, per chunk of rows:
//   dspec_rows_kernel        one pass over (b, f): the masked planes in T (products in the order of the loss kernels), norm_bl in double
//   dspec_transform_kernel   X = x op on the matrix cores, |X|^2 / norm in double
//   dspec_bin_kernel         a walk of the sorted row list of every bin, sums in double
// Every sum over rows is taken in double in a fixed order (no atomics on reals): two calls give the same bits, and so do two chunkings.
#pragma once
#include "normal_solve.hpp"
#include "row_walk.hpp"

namespace calk {

constexpr int kDsCols = 64;    // delays per workgroup of the transform: four 16-column tiles
constexpr int kDsRowTiles = 2; // 16-row tiles per wave: a staged piece of the operator serves 4 x 2 x 16 = 128 rows
constexpr int kDsRows = 4 * kDsRowTiles * 16;
constexpr int kDsStep = 32;    // channels of the operator staged per step; the planes' row pitch is a multiple of it
// elements per LDS row of a staged piece: lane quarter kq reads row kq V + s, and with 68 (fp32) the four rows start 4 x 68 = 272 words =
// 16 banks apart, with 72 (fp64) 2 x 72 doubles = 32 banks apart: a quarter's 16 adjacent columns do not meet another quarter's
template <typename T> constexpr int kDsPitch = sizeof(T) == 4 ? 68 : 72;

__host__ __device__ inline int ds_xpitch(int fpad) { return (fpad + kDsStep - 1) / kDsStep * kDsStep; }    // row pitch of the masked planes
__host__ __device__ inline int ds_ndpad(int ndelays) { return (ndelays + kDsCols - 1) / kDsCols * kDsCols; }  // columns of the operator image

// One wave per baseline row, four rows per block (row_walk.hpp).  Every plane pointer is that of the chunk's first row, `nrows` its
// rows.  x: [nq][2][nrows][xpitch] (re plane, then im plane, of every quantity asked for in the order data, model, residual), zeros in
// the channels [nfreqs, xpitch).
template <typename T>
__global__ __launch_bounds__(256) void dspec_rows_kernel(const T* __restrict__ model_r, const T* __restrict__ model_i, const T* __restrict__ data_r,
                                                          const T* __restrict__ data_i, const T* __restrict__ wgts,
                                                          const vec2_t<T>* __restrict__ gains, const int2* __restrict__ bl_ant,
                                                          const double* __restrict__ norm_f, int nrows, int nfreqs, int fpad, int xpitch, int what,
                                                          int calibrated, T* __restrict__ x, double* __restrict__ norm_bl) {
#pragma clang fp contract(off)
  constexpr int V = RowWalk<T>::V;
  typedef typename RowWalk<T>::vec_t vec_t;
  RowWalk<T> R;
  if (!R.begin(bl_ant, nrows, fpad)) return;
  GainPair<T> gp(gains, R.ant, fpad);
  const long long plane = (long long)nrows * xpitch;
  T* __restrict__ xrow = x + (long long)R.b * xpitch;
  double acc_n = 0;
  for (int f = R.lane * V; f < xpitch; f += 64 * V) {  // fpad and xpitch are multiples of 8: whole vectors
    vec_t o[3][2];
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int c = 0; c < V; ++c) o[q][0][c] = o[q][1][c] = (T)0;
    if (f < fpad) {
      const vec_t mr = R.load(model_r, f), mi = R.load(model_i, f);
      const vec_t dr = R.load(data_r, f), di = R.load(data_i, f);
      const vec_t w = R.load(wgts, f);
      gp.load(f);
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
        const bool live = f + c < nfreqs && w[c] != (T)0;
        o[0][0][c] = live ? d_r : (T)0, o[0][1][c] = live ? d_i : (T)0;
        o[1][0][c] = live ? m_r : (T)0, o[1][1][c] = live ? m_i : (T)0;
        o[2][0][c] = live ? d_r - m_r : (T)0, o[2][1][c] = live ? d_i - m_i : (T)0;
        acc_n += live ? norm_f[f + c] : 0.0;
      }
    }
    int slot = 0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      if (!(what >> q & 1)) continue;
      *reinterpret_cast<vec_t*>(xrow + (2 * slot) * plane + f) = o[q][0];
      *reinterpret_cast<vec_t*>(xrow + (2 * slot + 1) * plane + f) = o[q][1];
      ++slot;
    }
  }
  acc_n = ldsum(acc_n);
  if (R.lane == 0) norm_bl[R.b] = acc_n;
}

// The staged-operator loop of the transforms (dspec_transform_kernel, dcross_transform_kernel): X = x op for the wave's kDsRowTiles
// 16-row tiles and the block's 64 delays from c0 on.  The complex product is the real one of twice the depth, [x_r | x_i] . [op_r ; -op_i]
// and [x_r | x_i] . [op_i ; op_r], with the two halves of the depth taken side by side: per step of kDsStep channels the pieces
// [kDsStep][64] of op_r and op_i are staged in LDS once and serve all the block's rows (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64;
// per row tile four column tiles of Re X and four of Im X).  A lane takes its row's channels as 16-byte pieces straight from the plane
// (xrow_r, xrow_i: its row of every tile, at channel kq V): lane quarter kq holds channels kq V + s of a piece, so MFMA number s of a
// piece contracts the channels {kq V + s}, and the operator's rows are read from LDS in that order -- the sum over a piece is complete
// after its V MFMAs.  The image op ([fk][ndpad] per part, fk = xpitch) is zero beyond nfreqs and ndelays and the planes are zero beyond
// nfreqs: no tails in the loop.  All 256 threads of the block call it together (it holds the barriers of the staging).
template <typename T>
__device__ __forceinline__ void ds_transform_loop(const T* const (&xrow_r)[kDsRowTiles], const T* const (&xrow_i)[kDsRowTiles], const T* __restrict__ op_r,
                                                  const T* __restrict__ op_i, int xpitch, int ndpad, int c0, T (&s_op)[2][kDsStep][kDsPitch<T>],
                                                  typename MmT<T>::v4 (&acc_re)[kDsRowTiles][4], typename MmT<T>::v4 (&acc_im)[kDsRowTiles][4]) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  typedef ns_vec_t<T> vec_t;
  typedef typename MmT<T>::v4 acc_t;
  const int tid = threadIdx.x, lane = tid & 63;
  const int col = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int rt = 0; rt < kDsRowTiles; ++rt)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc_re[rt][t] = acc_im[rt][t] = acc_t{0, 0, 0, 0};
  for (int kp = 0; kp < xpitch; kp += kDsStep) {
    __syncthreads();  // the previous step's pieces have been read
    for (int idx = tid; idx < 2 * kDsStep * (kDsCols / V); idx += 256) {
      const int part = idx / (kDsStep * (kDsCols / V));
      const int rem = idx - part * (kDsStep * (kDsCols / V));
      const int kk = rem / (kDsCols / V), c = (rem - kk * (kDsCols / V)) * V;
      *reinterpret_cast<vec_t*>(&s_op[part][kk][c]) =
          *reinterpret_cast<const vec_t*>((part ? op_i : op_r) + (long long)(kp + kk) * ndpad + c0 + c);
    }
    __syncthreads();
#pragma unroll
    for (int pc = 0; pc < kDsStep; pc += 4 * V) {  // a piece: 4 V channels, V of them per lane quarter
      vec_t ar[kDsRowTiles], ai[kDsRowTiles];
#pragma unroll
      for (int rt = 0; rt < kDsRowTiles; ++rt) {
        ar[rt] = *reinterpret_cast<const vec_t*>(xrow_r[rt] + kp + pc);
        ai[rt] = *reinterpret_cast<const vec_t*>(xrow_i[rt] + kp + pc);
      }
#pragma unroll
      for (int s = 0; s < V; ++s) {
        T br[4], bi[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          br[t] = s_op[0][pc + kq * V + s][t * 16 + col];
          bi[t] = s_op[1][pc + kq * V + s][t * 16 + col];
        }
#pragma unroll
        for (int rt = 0; rt < kDsRowTiles; ++rt) {
          const T a_r = ar[rt][s], a_i = ai[rt][s], na_i = -a_i;
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            acc_re[rt][t] = MmT<T>::mfma(a_r, br[t], acc_re[rt][t]);
            acc_re[rt][t] = MmT<T>::mfma(na_i, bi[t], acc_re[rt][t]);
            acc_im[rt][t] = MmT<T>::mfma(a_r, bi[t], acc_im[rt][t]);
            acc_im[rt][t] = MmT<T>::mfma(a_i, br[t], acc_im[rt][t]);
          }
        }
      }
    }
  }
}

// block = (128 rows, 64 delays, quantity): wave w owns the row tiles 2 w, 2 w + 1 of ds_transform_loop.  Rows past the chunk's last read
// its last row again and write nothing.  out: [nq][nrows][ndelays] doubles.
template <typename T>
__global__ __launch_bounds__(256, 2) void dspec_transform_kernel(const T* __restrict__ x, const T* __restrict__ op, const double* __restrict__ norm_bl,
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
  double* __restrict__ o = out + (long long)blockIdx.z * nrows * ndelays;
#pragma unroll
  for (int rt = 0; rt < kDsRowTiles; ++rt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + rt * 16 + MmT<T>::row_of(kq, r);
      if (row >= nrows) continue;
      const double nb = norm_bl[row];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int k = c0 + t * 16 + col;
        if (k >= ndelays) continue;
        const double re = (double)acc_re[rt][t][r], im = (double)acc_im[rt][t][r];
        o[(long long)row * ndelays + k] = nb != 0.0 ? (re * re + im * im) / nb : 0.0;
      }
    }
  }
}

// block = (bin n, 256 delays, quantity); a thread owns one delay.  ent: the rows of every bin in ascending order, ptr[2 n], ptr[2 n + 1]
// the piece of bin n's list that lies in this chunk (rows [b0, b0 + nrows)); power: the chunk's [nq][nrows][ndelays].  The first chunk
// starts the sums at zero, a later one at what the chunks before it left: the order of the additions is that of one chunk.  A row with
// norm_bl == 0 is left out (its power is zero; it does not count).  The block of delay 0 and quantity 0 counts the bin's rows.
__global__ __launch_bounds__(256) void dspec_bin_kernel(const double* __restrict__ power, const double* __restrict__ norm_bl, const int* __restrict__ ptr,
                                                         const int* __restrict__ ent, int b0, int nrows, int ndelays, int nbins, int first,
                                                         double* __restrict__ power_bin, double* __restrict__ count_bin) {
  const int n = blockIdx.x, q = blockIdx.z;
  const int k = blockIdx.y * 256 + threadIdx.x;
  const int e0 = ptr[2 * n], e1 = ptr[2 * n + 1];
  if (k < ndelays) {
    const long long oi = ((long long)q * nbins + n) * ndelays + k;
    double s = first ? 0.0 : power_bin[oi];
    const double* __restrict__ p = power + (long long)q * nrows * ndelays + k;
    for (int e = e0; e < e1; ++e) {
      const int b = ent[e] - b0;  // block-uniform
      if (norm_bl[b] > 0.0) s += p[(long long)b * ndelays];
    }
    power_bin[oi] = s;
  }
  if (blockIdx.y == 0 && q == 0 && threadIdx.x == 0) {
    double cnt = first ? 0.0 : count_bin[n];
    for (int e = e0; e < e1; ++e) cnt += norm_bl[ent[e] - b0] > 0.0 ? 1.0 : 0.0;
    count_bin[n] = cnt;
  }
}

}  // namespace calk
