// fit_error_kernels.hpp -- the errors of a fit (cal_solver_fit_errors): the inverse of the curvature matrix the closed-form coefficient
// solve builds and throws away.  In the notation of coeff_solve_kernels.hpp, per fitting group gamma with q[b][f] = w |G|^2:
//   N = sum_{b in gamma} A_b^T diag(q_b) A_b       N_r = N + ridge (tr N / nvec) I       L L^T = N_r       W = L^-1
//   coeff_var[k]    = (N_r^-1)[k][k] = sum_i W[i][k]^2
//   model_var[b][f] = a_{b,f}^T N_r^-1 a_{b,f} = |W a_{b,f}|^2          (a_{b,f}: row f of A_b; the variance of m = A c)
//   leverage_bl[b]  = sum_f q[b][f] model_var[b][f]                     nsamp_bl[b] = #{f : w[b][f] != 0}
// Behind the model pass, coeff_solve_rows_kernel (q) and coeff_gram_kernel (N), both as they are:
//   fit_error_factor_kernel     per group, in double: the shared Cholesky (normal_solve.hpp), W = L^-1 row by row in place, coeff_var;
//                               W rounded to T once into the chunk's scratch, padded to whole 16 x 16 tiles
//   fit_error_leverage_kernel   per (run of a group's baselines on one row block, 64 channels of the band): Z = W A^T on the matrix
//                               cores, the squares of Z summed over the vectors in double -> model_var of the run; per row of the run the
//                               partial sum of q model_var over the piece's channels
//   fit_error_rows_kernel       per baseline row: the partial sums added in channel order -> leverage_bl; nsamp_bl
// Everything is summed in a fixed order (no atomics on reals: two calls give the same bits).
#pragma once
#include "coeff_solve_kernels.hpp"

namespace calk {

constexpr int kFePiece = 64;   // channels of the band per workgroup of the leverage kernel: four 16-column tiles per wave
constexpr int kFePitch = 80;   // elements per LDS row of the staged tiles: the four rows (vectors k .. k + 3) of an MFMA column operand
                               // start 80 elements apart, 16 (fp32: words, 32 banks per half wave) / 32 (fp64: 64 banks) banks on
                               // from each other, so a half wave's 2 x 16 elements land on distinct banks -- kNsPitch's reasoning
struct FeWork { int grp, b0, b1, piece; };  // a run [b0, b1) of group grp's baselines on one row block; 64 channels of the (half) band

__host__ __device__ inline int fe_pad(int nvec) { return (nvec + 15) & ~15; }  // rows / columns of the stored W

// One workgroup per group.  The factor M ([nvec + 1][ld] doubles: L, then a spare row) lies in LDS when [nvec + 2][ld] fits
// `lds_doubles` (the bound of coeff_chol_kernel, so that both take the same branch) and in the chunk's double scratch otherwise.
// W = L^-1 replaces L row by row (normal_chol_invert of normal_solve.hpp).  A group that is singular by the
// shared tests leaves ok[group] = 0 and its outputs alone (the host has zeroed them) and counts in counts[1].
template <typename T>
__global__ __launch_bounds__(256) void fit_error_factor_kernel(const T* __restrict__ nmat, double* __restrict__ dscr,
                                                                const CsGroup* __restrict__ grps, const int* __restrict__ order,
                                                                const long long* __restrict__ woff, T* __restrict__ wmat,
                                                                double* __restrict__ coeff_var, int* __restrict__ ok, double ridge,
                                                                int* __restrict__ counts, int lds_doubles) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double s_m[];
  __shared__ double s_red[256];
  const int gi = order[blockIdx.x];
  const CsGroup g = grps[gi];
  const int tid = threadIdx.x;
  const int n = g.nvec;
  const bool in_lds = (long long)(n + 2) * (n | 1) <= lds_doubles;
  const int ld = in_lds ? (n | 1) : n;
  double* M = in_lds ? s_m : dscr + g.doff;
  if (!normal_chol_load(M, ld, n, nmat + g.noff, ridge, s_red) || !normal_chol_factor(M, ld, n, n)) {
    if (tid == 0) atomicAdd(counts + 1, 1);
    return;
  }
  normal_chol_invert(M, ld, n);
  for (int k = tid; k < n; k += 256) {
    double s = 0;
    for (int i = k; i < n; ++i) {
      const double v = M[(long long)i * ld + k];
      s += v * v;
    }
    coeff_var[g.coff + k] = s;
  }
  const int np = fe_pad(n);
  T* __restrict__ Wg = wmat + woff[gi];
  for (int idx = tid; idx < np * np; idx += 256) {
    const int i = idx / np, k = idx - i * np;
    Wg[idx] = (i < n && k <= i) ? (T)M[(long long)i * ld + k] : (T)0;
  }
  if (tid == 0) {
    ok[gi] = 1;
    atomicAdd(counts, 1);
  }
}

// What the leverage kernel and gain_error_var_kernel (gain_error_kernels.hpp) share, by the whole workgroup (256 threads): the column
// sums of the squares of Z = W X for 64 columns (channels), W [np][np] lower triangular in whole 16 x 16 tiles, X [np][64] given by
// piece(k, c): the 16 bytes of row (vector) k from column c on, zeros where X has none.  64 rows of Z at a time: wave w owns rows
// [64 ib + 16 w, + 16) and four 16 x 16 accumulator tiles; per step of kNsChunk vectors the 64 x 32 block of W and the 32 x 64 block
// of X are staged in LDS (s_w, s_at); blocks of W above the diagonal are never staged, and a wave stops at its own diagonal tile.  The
// squares of a row block are summed in double per lane (s_sq), then over the 16 (wave, lane quarter) partial sums in a fixed order by
// the thread that owns the column: the sum of column tid is returned to the threads tid < 64.  Begins with a barrier.
template <typename T, typename Piece>
__device__ __forceinline__ double fe_sumsq(const T* __restrict__ Wg, int np, T (*s_w)[kNsPitch], T (*s_at)[kFePitch], double (*s_sq)[kFePiece],
                                           Piece piece) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  typedef ns_vec_t<T> vec_t;
  typedef typename MmT<T>::v4 acc_t;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int nrb = (np + kNsBlock - 1) / kNsBlock;
  double mv = 0;
  for (int ib = 0; ib < nrb; ++ib) {
    acc_t acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = acc_t{0, 0, 0, 0};
    const int r0 = ib * kNsBlock + wave * 16;                         // the wave's first row
    const int kend = np < (ib + 1) * kNsBlock ? np : (ib + 1) * kNsBlock;  // W is lower triangular
    const int kmine = r0 < np ? (r0 + 16 < kend ? r0 + 16 : kend) : 0;
    for (int kp = 0; kp < kend; kp += kNsChunk) {
      __syncthreads();  // the previous step's operands (and s_sq) have been read
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
        *reinterpret_cast<vec_t*>(&s_at[kk][c]) = piece(kp + kk, c);
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
    for (int t = 0; t < 4; ++t) {
      double s = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) s += (double)acc[t][r] * (double)acc[t][r];
      s_sq[wave * 4 + kq][t * 16 + col] = s;
    }
    __syncthreads();
    if (tid < kFePiece)
      for (int p = 0; p < 16; ++p) mv += s_sq[p][tid];
  }
  return mv;
}

// One workgroup per FeWork.  Z = W A^T for the piece's channels through fe_sumsq above (v_mfma_f32_16x16x4_f32 /
// v_mfma_f64_16x16x4_f64; the reduction index is the vector k); its column operand is the 32 x 64 block of the tiles ([vector][channel],
// as the tiles store it, any tile width).  Folded tiles hold channels [0, nfreqs / 2): a second pass with
// a[k] (-1)^k gives the mirror channel nfreqs - 1 - f.  Every row of the run takes the same model_var (when asked for) and its own
// partial sum of q model_var: part[row][slot], slot = piece, or 2 npieces - 1 - piece for the mirror pass, so that the slots are in
// channel order.
template <typename T>
__global__ __launch_bounds__(256) void fit_error_leverage_kernel(const T* __restrict__ tiles, const long long* __restrict__ bl_tile,
                                                                  const T* __restrict__ q_rows, const CsGroup* __restrict__ grps,
                                                                  const long long* __restrict__ woff, const int* __restrict__ ok,
                                                                  const FeWork* __restrict__ work, const T* __restrict__ wmat,
                                                                  double* __restrict__ model_var, double* __restrict__ part, int nfreqs,
                                                                  int fpad, int fold, int npieces) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  typedef ns_vec_t<T> vec_t;
  __shared__ __attribute__((aligned(16))) T s_w[kNsBlock][kNsPitch];
  __shared__ __attribute__((aligned(16))) T s_at[kNsChunk][kFePitch];
  __shared__ double s_sq[16][kFePiece];  // [wave * 4 + lane quarter][channel]
  __shared__ double s_mv[kFePiece];
  const FeWork wk = work[blockIdx.x];
  if (!ok[wk.grp]) return;
  const CsGroup g = grps[wk.grp];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nvec = g.nvec, np = fe_pad(nvec);
  const int fb = 1 << g.fb_log2;
  const int nch = ((fold ? nfreqs / 2 : fpad) >> g.fb_log2) << g.fb_log2;  // what the group's tiles cover
  const int c0 = wk.piece * kFePiece;
  const int cn = nch - c0 < kFePiece ? nch - c0 : kFePiece;  // a multiple of a 16-byte piece, like the tile width; <= 0: nothing
  const T* __restrict__ Wg = wmat + woff[wk.grp];
  const T* __restrict__ tbase = tiles + bl_tile[wk.b0];
  const int nslot = (fold ? 2 : 1) * npieces;
  for (int mirror = 0; mirror <= fold; ++mirror) {
    // of channel c0 + tid (tid < 64)
    const double mv = fe_sumsq<T>(Wg, np, s_w, s_at, s_sq, [&](int k, int c) {
      vec_t v;
#pragma unroll
      for (int x = 0; x < V; ++x) v[x] = (T)0;
      if (k < nvec && c < cn) {
        const int ch = c0 + c;
        v = *reinterpret_cast<const vec_t*>(tbase + (long long)(ch >> g.fb_log2) * nvec * fb + (long long)k * fb + (ch & (fb - 1)));
        if (mirror && (k & 1)) v = -v;
      }
      return v;
    });
    if (tid < kFePiece) s_mv[tid] = mv;
    __syncthreads();
    // the rows of the run, one wave each: lane c has channel c0 + c of the (half) band
    const int f = mirror ? nfreqs - 1 - (c0 + lane) : c0 + lane;
    const bool live = lane < cn && f < nfreqs;
    const int slot = mirror ? nslot - 1 - wk.piece : wk.piece;
    for (int bb = wk.b0 + wave; bb < wk.b1; bb += 4) {
      double lev = 0;
      if (live) {
        if (model_var) model_var[(long long)bb * nfreqs + f] = s_mv[lane];
        lev = (double)q_rows[(long long)bb * fpad + f] * s_mv[lane];
      }
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) lev += __shfl_xor(lev, o);  // (a fixed tree over the piece's channels)
      if (lane == 0) part[(long long)bb * nslot + slot] = lev;
    }
    __syncthreads();  // s_mv has been read before the mirror pass writes it
  }
}

// One wave per baseline row, four rows per block: leverage_bl[b] = the row's partial sums in slot (channel) order; nsamp_bl[b] = the
// number of channels < nfreqs with w != 0 (an integer, as a double).  Either output may be null.
template <typename T>
__global__ __launch_bounds__(256) void fit_error_rows_kernel(const double* __restrict__ part, const T* __restrict__ wgts, int nbls, int nfreqs,
                                                              int fpad, int nslot, double* __restrict__ leverage_bl,
                                                              double* __restrict__ nsamp_bl) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
  if (b >= nbls) return;
  if (nsamp_bl) {
    int n = 0;
    for (int f = lane; f < nfreqs; f += 64) n += wgts[(long long)b * fpad + f] != (T)0 ? 1 : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) n += __shfl_xor(n, o);
    if (lane == 0) nsamp_bl[b] = (double)n;
  }
  if (leverage_bl && lane == 0) {
    double s = 0;
    for (int p = 0; p < nslot; ++p) s += part[(long long)b * nslot + p];
    leverage_bl[b] = s;
  }
}

}  // namespace calk
