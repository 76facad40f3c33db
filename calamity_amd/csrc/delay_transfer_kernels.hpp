// delay_transfer_kernels.hpp -- how much of the power at every delay the coefficient fit itself removes (cal_solver_delay_transfer).
// In the notation of fit_error_kernels.hpp and delay_spectrum_kernels.hpp, for baseline row b of group gamma with antennas (i, j),
// G = g_i conj(g_j), q = w |G|^2, mask = (w != 0), W = L^-1 of the group's N_r and a_{b,f} row f of A_b:
//                  raw residual  d - G m        calibrated residual  d / G - m
//   s[b][f]     =  mask G                       mask                     (0 where |G|^2 == 0)
//   v[b][f]     =  mask / w                     mask / q                 (0 where |G|^2 == 0)
//   U[b][k]        = sum_f (op_r + i op_i)[f][k] s[b][f] a_{b,f}         complex, nvec numbers
//   num[b][k]      = |W U[b][k]|^2 = sum_v |sum_f S[v][f] s[b][f] op[f][k]|^2,   S = W A_b^T
//   noise_bl[b][k] = sum_f v[b][f] |op[f][k]|^2
//   absorbed_bl[b][k] = num / noise_bl      (0 where noise_bl == 0 or the group is singular)
// With noise of variance 1 / w on the unflagged samples and the coefficients at their weighted least-squares optimum, noise_bl is the
// expected delay power of the masked data and noise_bl - num that of the masked residual.
// Behind the model pass, coeff_solve_rows_kernel (q), coeff_gram_kernel (N) and fit_error_factor_kernel (W), all three as they are:
//   dtransfer_basis_kernel   per (run of a group's baselines on one row block, 64 channels): S = W A^T on the matrix cores, stored in T
//   dtransfer_power_kernel   per (baseline row, 64 delays): (S diag(s_b)) op, real x complex, on the matrix cores; |.|^2 summed over the
//                            vectors in double; noise_bl from the same staged pieces
// dspec_bin_kernel (as it is) then adds the rows of every bin.  Every sum is taken in a fixed order (no atomics on reals).
#pragma once
#include "fit_error_kernels.hpp"
#include "delay_spectrum_kernels.hpp"

namespace calk {

constexpr int kDtPass = 128;  // vectors per pass of the power kernel: two 16-row tiles per wave (one where the group has <= 64 vectors)

struct DtRun { long long soff; int grp, b0, b1, pad; };  // a run [b0, b1) of group grp's baselines on one row block; its S in the chunk's scratch
struct DtRow { long long soff; int b, grp; };             // a baseline row: S of its run, its group

// One workgroup per (run, piece of kFePiece channels): blockIdx.x = run * npieces + piece.  The product of fit_error_leverage_kernel --
// W [np][np] lower triangular in whole 16 x 16 tiles times the 32 x 64 blocks of the tiles ([vector][channel], any tile width), the
// same staging (kNsPitch, kFePitch), a wave stops at its own diagonal tile, a second pass with a[k] (-1)^k for the mirror channels of
// folded tiles -- but the product is stored, not squared: S[v][f] for v < np and the piece's channels f < nfreqs.  smat: the chunk's
// scratch, S of a run [np][xpitch] at run.soff; the host has zeroed it (the channels [nfreqs, xpitch) stay zero).
template <typename T>
__global__ __launch_bounds__(256) void dtransfer_basis_kernel(const T* __restrict__ tiles, const long long* __restrict__ bl_tile,
                                                               const CsGroup* __restrict__ grps, const long long* __restrict__ woff,
                                                               const int* __restrict__ ok, const DtRun* __restrict__ runs, T* __restrict__ smat,
                                                               int nfreqs, int fpad, int xpitch, int fold, int npieces) {
  constexpr int V = 16 / (int)sizeof(T);
  typedef ns_vec_t<T> vec_t;
  typedef typename MmT<T>::v4 acc_t;
  __shared__ __attribute__((aligned(16))) T s_w[kNsBlock][kNsPitch];
  __shared__ __attribute__((aligned(16))) T s_at[kNsChunk][kFePitch];
  const DtRun run = runs[blockIdx.x / npieces];
  const int piece = blockIdx.x % npieces;
  if (!ok[run.grp]) return;
  const CsGroup g = grps[run.grp];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int nvec = g.nvec, np = fe_pad(nvec);
  const int fb = 1 << g.fb_log2;
  const int nch = ((fold ? nfreqs / 2 : fpad) >> g.fb_log2) << g.fb_log2;  // what the group's tiles cover
  const int c0 = piece * kFePiece;
  const int cn = nch - c0 < kFePiece ? nch - c0 : kFePiece;  // a multiple of a 16-byte piece, like the tile width; <= 0: nothing
  if (cn <= 0) return;
  const T* __restrict__ Wg = smat + woff[run.grp];
  const T* __restrict__ tbase = tiles + bl_tile[run.b0];
  T* __restrict__ S = smat + run.soff;
  const int nrb = (np + kNsBlock - 1) / kNsBlock;
  for (int mirror = 0; mirror <= fold; ++mirror) {
    for (int ib = 0; ib < nrb; ++ib) {
      acc_t acc[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = acc_t{0, 0, 0, 0};
      const int r0 = ib * kNsBlock + wave * 16;                              // the wave's first row
      const int kend = np < (ib + 1) * kNsBlock ? np : (ib + 1) * kNsBlock;  // W is lower triangular
      const int kmine = r0 < np ? (r0 + 16 < kend ? r0 + 16 : kend) : 0;
      for (int kp = 0; kp < kend; kp += kNsChunk) {
        __syncthreads();  // the previous step's operands have been read
        for (int idx = tid; idx < kNsBlock * (kNsChunk / V); idx += 256) {
          const int r = idx / (kNsChunk / V), c = (idx - r * (kNsChunk / V)) * V;
          const int row = ib * kNsBlock + r, k = kp + c;
          vec_t v;
#pragma unroll
          for (int x = 0; x < V; ++x) v[x] = (T)0;
          if (row < np && k < np) v = *reinterpret_cast<const vec_t*>(Wg + (long long)row * np + k);
          *reinterpret_cast<vec_t*>(&s_w[r][c]) = v;
        }
        for (int idx = tid; idx < kNsChunk * (kFePiece / V); idx += 256) {
          const int kk = idx / (kFePiece / V), c = (idx - kk * (kFePiece / V)) * V;
          const int k = kp + kk;
          vec_t v;
#pragma unroll
          for (int x = 0; x < V; ++x) v[x] = (T)0;
          if (k < nvec && c < cn) {
            const int ch = c0 + c;
            v = *reinterpret_cast<const vec_t*>(tbase + (long long)(ch >> g.fb_log2) * nvec * fb + (long long)k * fb + (ch & (fb - 1)));
            if (mirror && (k & 1)) v = -v;
          }
          *reinterpret_cast<vec_t*>(&s_at[kk][c]) = v;
        }
        __syncthreads();
        const int ke = kmine - kp < kNsChunk ? kmine - kp : kNsChunk;
        for (int kk = 0; kk < ke; kk += 4) {
          const T a = s_w[wave * 16 + col][kk + kq];
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[t] = MmT<T>::mfma(a, s_at[kk + kq][t * 16 + col], acc[t]);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = r0 + MmT<T>::row_of(kq, r);
        if (row >= np) continue;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int c = t * 16 + col;
          const int f = mirror ? nfreqs - 1 - (c0 + c) : c0 + c;
          if (c < cn && f >= 0 && f < nfreqs) S[(long long)row * xpitch + f] = acc[t][r];
        }
      }
    }
  }
}

// s (complex) and v of one sample, from the T values in the order of the loss kernels (GainPair::at of row_walk.hpp; q as
// coeff_solve_rows_kernel forms it); v in double.
template <typename T>
__device__ __forceinline__ void dtransfer_sample(vec2_t<T> gi, vec2_t<T> gj, T w, bool live, int calibrated, T& s_r, T& s_i, double& v) {
#pragma clang fp contract(off)
  const T Gr = gi.x * gj.x + gi.y * gj.y;  // g_i conj(g_j)
  const T Gi = gi.y * gj.x - gi.x * gj.y;
  const T den = Gr * Gr + Gi * Gi;
  s_r = s_i = (T)0;
  v = 0.0;
  if (!live) return;
  if (calibrated) {
    if (den == (T)0) return;
    const T q = w * den;
    s_r = (T)1;
    v = 1.0 / (double)q;
  } else {
    s_r = Gr, s_i = Gi;
    v = 1.0 / (double)w;
  }
}

// One workgroup per (baseline row of the chunk, 64 delays): blockIdx.x = row * (ndpad / 64) + column block, so the delay pieces of one
// baseline are neighbours in the grid and S of its run is read from cache.  Per pass of kDtPass vectors (wave w owns the row tiles
// [64 rt + 16 w, + 16), rt < 2, of the pass) and per step of kDsStep channels the pieces [kDsStep][64] of op_r and op_i are staged in
// LDS as dspec_transform_kernel stages them (kDsPitch), multiplied by s[b][f] on the way (a complex product in T): diag(s_b) op is
// never stored.  S is real: a row tile takes four column tiles of Re and four of Im (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64).
// A lane takes its vector's channels as 16-byte pieces straight from S, as the transform takes its rows.  After a pass re^2 + im^2 is
// summed in double over the lane's rows, then over the 16 (wave, lane quarter) partial sums in a fixed order by the thread that owns the
// column.  In the first pass the staging threads also add v |op|^2 of their channels in double per column (a thread's column piece is
// the same in every step); the 256 / (64 / V) partial sums of a column are added in a fixed order.  rows: the chunk's rows; valid[b] =
// 1 where the group is factored and the row has an unflagged sample, else 0 (written by the first column block); such a row's outputs
// are zero.  absorbed, noise: [nbls][ndelays] doubles, either may be null.
template <typename T>
__global__ __launch_bounds__(256, 2) void dtransfer_power_kernel(const T* __restrict__ smat, const T* __restrict__ op, const T* __restrict__ wgts,
                                                                  const vec2_t<T>* __restrict__ gains, const int2* __restrict__ bl_ant,
                                                                  const CsGroup* __restrict__ grps, const int* __restrict__ ok,
                                                                  const DtRow* __restrict__ rows, int nfreqs, int fpad, int xpitch, int ndelays,
                                                                  int ndpad, int calibrated, double* __restrict__ absorbed,
                                                                  double* __restrict__ noise, double* __restrict__ valid) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  constexpr int P = kDsPitch<T>;
  constexpr int CV = kDsCols / V;    // 16-byte column pieces of a staged row
  constexpr int NI = kDsStep * CV / 256;  // staged items per thread and step
  constexpr int NPART = 256 / CV;    // threads that share a column piece
  typedef ns_vec_t<T> vec_t;
  typedef typename MmT<T>::v4 acc_t;
  __shared__ __attribute__((aligned(16))) T s_op[2][kDsStep][P];  // [re, im][channel of the step][delay of the block]
  __shared__ double s_sq[16][kDsCols];                            // [wave * 4 + lane quarter][delay]; the noise partial sums at the end
  __shared__ int s_any;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int ncb = ndpad / kDsCols;
  const DtRow rw = rows[blockIdx.x / ncb];
  const int cb = blockIdx.x % ncb;
  const int c0 = cb * kDsCols;
  const int b = rw.b;
  const int kcol = c0 + tid;  // of the threads tid < 64
  if (!ok[rw.grp]) {          // a singular group: zeros
    if (tid < kDsCols && kcol < ndelays) {
      if (absorbed) absorbed[(long long)b * ndelays + kcol] = 0.0;
      if (noise) noise[(long long)b * ndelays + kcol] = 0.0;
    }
    if (cb == 0 && tid == 0) valid[b] = 0.0;
    return;
  }
  const int nvec = grps[rw.grp].nvec, np = fe_pad(nvec);
  const int2 ant = bl_ant[b];
  const vec2_t<T>* __restrict__ gi = gains + (long long)ant.x * fpad;
  const vec2_t<T>* __restrict__ gj = gains + (long long)ant.y * fpad;
  const T* __restrict__ wrow = wgts + (long long)b * fpad;
  const T* __restrict__ S = smat + rw.soff;
  const T* __restrict__ op_r = op;
  const T* __restrict__ op_i = op + (long long)xpitch * ndpad;
  const int cpiece = (tid % CV) * V;  // the thread's column piece of every staged row
  const int kk0 = tid / CV;           // its first channel of a step; the others NPART apart
  if (tid == 0) s_any = 0;
  double nz[V];
#pragma unroll
  for (int x = 0; x < V; ++x) nz[x] = 0.0;
  int any = 0;
  double num = 0.0;  // of column kcol (tid < 64)
  const int npass = (np + kDtPass - 1) / kDtPass;
  for (int pass = 0; pass < npass; ++pass) {
    const int v0 = pass * kDtPass;
    const int nrt = np - v0 > kNsBlock ? 2 : 1;  // row tiles per wave in this pass (block-uniform)
    const T* srow[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      int row = v0 + rt * kNsBlock + wave * 16 + col;
      row = row < np ? row : np - 1;  // a row past the last reads the last again and counts nowhere
      srow[rt] = S + (long long)row * xpitch + kq * V;
    }
    acc_t acc_re[2][4], acc_im[2][4];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc_re[rt][t] = acc_im[rt][t] = acc_t{0, 0, 0, 0};
    for (int kp = 0; kp < xpitch; kp += kDsStep) {
      __syncthreads();  // the previous step's pieces have been read
#pragma unroll
      for (int it = 0; it < NI; ++it) {
        const int kk = kk0 + it * NPART;
        const int f = kp + kk;
        T s_r = (T)0, s_i = (T)0;
        double v = 0.0;
        if (f < fpad) {
          const T w = wrow[f];
          const bool live = f < nfreqs && w != (T)0;
          any |= live ? 1 : 0;
          dtransfer_sample<T>(gi[f], gj[f], w, live, calibrated, s_r, s_i, v);
        }
        const vec_t o_r = *reinterpret_cast<const vec_t*>(op_r + (long long)f * ndpad + c0 + cpiece);
        const vec_t o_i = *reinterpret_cast<const vec_t*>(op_i + (long long)f * ndpad + c0 + cpiece);
        vec_t p_r, p_i;
#pragma unroll
        for (int x = 0; x < V; ++x) {
          p_r[x] = o_r[x] * s_r - o_i[x] * s_i;
          p_i[x] = o_r[x] * s_i + o_i[x] * s_r;
          if (pass == 0) nz[x] += v * ((double)o_r[x] * (double)o_r[x] + (double)o_i[x] * (double)o_i[x]);
        }
        *reinterpret_cast<vec_t*>(&s_op[0][kk][cpiece]) = p_r;
        *reinterpret_cast<vec_t*>(&s_op[1][kk][cpiece]) = p_i;
      }
      __syncthreads();
#pragma unroll
      for (int pc = 0; pc < kDsStep; pc += 4 * V) {  // a piece: 4 V channels, V of them per lane quarter
        vec_t a[2];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
          if (rt < nrt) a[rt] = *reinterpret_cast<const vec_t*>(srow[rt] + kp + pc);
#pragma unroll
        for (int s = 0; s < V; ++s) {
          T br[4], bi[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            br[t] = s_op[0][pc + kq * V + s][t * 16 + col];
            bi[t] = s_op[1][pc + kq * V + s][t * 16 + col];
          }
#pragma unroll
          for (int rt = 0; rt < 2; ++rt) {
            if (rt >= nrt) continue;
            const T av = a[rt][s];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              acc_re[rt][t] = MmT<T>::mfma(av, br[t], acc_re[rt][t]);
              acc_im[rt][t] = MmT<T>::mfma(av, bi[t], acc_im[rt][t]);
            }
          }
        }
      }
    }
    // the pass's squares: per lane over its rows, then over the 16 partial sums of the column
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      double s = 0.0;
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
        if (rt >= nrt) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = v0 + rt * kNsBlock + wave * 16 + MmT<T>::row_of(kq, r);
          const double re = (double)acc_re[rt][t][r], im = (double)acc_im[rt][t][r];
          s += row < np ? re * re + im * im : 0.0;
        }
      }
      s_sq[wave * 4 + kq][t * 16 + col] = s;
    }
    __syncthreads();
    if (tid < kDsCols)
      for (int p = 0; p < 16; ++p) num += s_sq[p][tid];
    // (the next pass's first barrier stands between these reads and the next writes of s_sq)
  }
  __syncthreads();
#pragma unroll
  for (int x = 0; x < V; ++x) s_sq[kk0][cpiece + x] = nz[x];  // NPART <= 16 rows of s_sq
  if (any) s_any = 1;  // (every writer writes the same value)
  __syncthreads();
  if (tid < kDsCols && kcol < ndelays) {
    double nb = 0.0;
    for (int p = 0; p < NPART; ++p) nb += s_sq[p][tid];
    if (absorbed) absorbed[(long long)b * ndelays + kcol] = nb != 0.0 ? num / nb : 0.0;
    if (noise) noise[(long long)b * ndelays + kcol] = nb;
  }
  if (cb == 0 && tid == 0) valid[b] = s_any ? 1.0 : 0.0;
}

}  // namespace calk
