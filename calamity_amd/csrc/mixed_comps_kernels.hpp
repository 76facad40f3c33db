// mixed_comps_kernels.hpp -- the modeling vectors of jointly fitted groups (simple_cov.py: the leading eigenvectors of the analytic
// covariance C of a group's n = Nbls x Nfreqs samples) without the dense O(n^3) eigenproblem.  C is numerically of low rank, so per group
//   C ~ L L^T            diagonally pivoted Cholesky, stopped when the largest remaining diagonal falls below tol: k columns, O(n k^2)
//   G = L^T L            [k][k]; its eigenpairs (lambda, U) are those of L L^T, hence of C up to the residual (Weyl)
//   V = L U lambda^-1/2  the orthonormal vectors of the kept eigenvalues
// and ||C - L L^T||_F over the whole matrix as the certificate that the factorisation did not stop early on an indefinite C.
// The k x k eigenproblem is the host's.  Everything here is double; only V is written in the caller's type.
//   mixed_cov_elem        one element of C, the expression of simple_cov.simple_cov_matrix in its order of operations
//   mixed_dense_kernel    a whole C (simple_cov_matrix(device=), and the tests)
//   mixed_init_kernel     d = diag C and the argmax partials of step 0 (partial buffer 0)
//   mixed_step_kernel     one column of every unfinished group of a chunk
//   mixed_gram_kernel     G on the Gram core of normal_solve.hpp: the columns of L are its rows, the sample its channel, w = 1
//   mixed_cert_kernel     64 x 64 tiles (bi, bj <= bi) of C - L L^T: C on the fly, L L^T on v_mfma_f64_16x16x4_f64, the squares summed
//   mixed_cert_sum_kernel the tiles' sums of a group, in tile order
//   mixed_backmul_kernel  V = L (U lambda^-1/2) on the same matrix-core tile product
// L is column-major with a pitch ldl (n rounded up to 64) and zero rows behind n; its columns are padded with zero columns to a
// multiple of 16, so no tile product needs a bound on either index.  All sums have a fixed order: two calls give the same bits, and a
// group's bits do not depend on its neighbours in the call.
#pragma once
#include "normal_solve.hpp"

namespace calk {

constexpr int kMxRows = 256;   // rows of a group per workgroup of the init and step kernels: one per thread
constexpr int kMxTile = 64;    // rows / columns of a tile of the certificate and of V
constexpr int kMxStepJ = 16;   // columns of L staged per step of a tile product
constexpr int kMxPitch = 80;   // doubles per staged column: the four k-quarters of an operand read land 32 banks apart
constexpr int kMxMaxCap = 6144;  // widest factor: row p of L is staged in LDS (48 KB)

enum { MX_OK = 0, MX_RANK_CAP = 1, MX_NOT_RUN = 2 };

struct MxParams { double ant_dly, horizon, offset, min_dly; };
struct MxPart { double v; int idx; int pad; };  // a block's largest running diagonal and its row (ties: the lowest row)
struct MxState { int k, done, status, pad; double maxd; };
struct MxGroup {
  int n, ldl, cap, nblk;  // samples, pitch of L, rank cap, 256-row blocks
  int k, kpad, r, pad;    // after the factorisation: rank, columns with the zero padding; kept vectors of the back-multiplication
  long long s_off;        // first sample in the sample array
  double* L;              // [kpad or more][ldl]
  double* d;              // [ldl] running diagonal
  MxPart* part;           // [2][nblk]: step m reads [m & 1] and writes the other, so no block reads what a sibling writes in its launch
  int* piv;               // [cap]
  long long g_off;        // G [k][k] in the Gram buffer
  long long c_off;        // first tile sum in the certificate buffer
  long long u_off, sc_off, v_off;  // U [k][r], scale [r], V [n][r] in the buffers of the back-multiplication
};
struct MxWork { int grp, bi, bj; };

__device__ __forceinline__ double mx_sinc(double x) {
#pragma clang fp contract(off)
  if (x == 0.0) return 1.0;
  return sinpi(x) / (M_PI * x);
}
// Samples are (u, v, w in wavelengths, nu in Hz).  The order of operations is simple_cov_matrix's, nothing is contracted.
__device__ __forceinline__ double mixed_cov_elem(const double4 a, const double4 b, const MxParams P) {
#pragma clang fp contract(off)
  const double dx = fabs(a.x - b.x), dy = fabs(a.y - b.y), dz = fabs(a.z - b.z);
  double s = 0.0;
  s += dx * dx;
  s += dy * dy;
  s += dz * dz;
  double sep = sqrt(s) * P.horizon;
  const double dfg = fabs(a.w - b.w) / 1e9;
  sep += dfg * P.offset;
  const double x0 = 2.0 * fmax(P.min_dly * dfg, sep);
  const double x1 = 2.0 * dfg * P.ant_dly;
  return mx_sinc(x0) * mx_sinc(x1);
}

__global__ __launch_bounds__(256) void mixed_dense_kernel(const double4* __restrict__ smp, int n, MxParams P, double* __restrict__ C) {
  const long long total = (long long)n * n;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int i = (int)(idx / n), j = (int)(idx - (long long)i * n);
    C[idx] = mixed_cov_elem(smp[i], smp[j], P);
  }
}

__device__ __forceinline__ bool mx_better(double v, int i, double w, int j) { return v > w || (v == w && i < j); }

// The block's argmax of (v, idx) over its 256 threads, ties to the lowest idx: butterflies inside the waves, the four waves in order.
__device__ __forceinline__ MxPart mx_block_argmax(double v, int idx, MxPart* s_w) {
#pragma unroll
  for (int sft = 1; sft < 64; sft <<= 1) {
    const double w = __shfl_xor(v, sft, 64);
    const int j = __shfl_xor(idx, sft, 64);
    if (mx_better(w, j, v, idx)) { v = w; idx = j; }
  }
  if ((threadIdx.x & 63) == 0) { s_w[threadIdx.x >> 6].v = v; s_w[threadIdx.x >> 6].idx = idx; }
  __syncthreads();
  MxPart best = s_w[0];
#pragma unroll
  for (int w = 1; w < 4; ++w)
    if (mx_better(s_w[w].v, s_w[w].idx, best.v, best.idx)) best = s_w[w];
  return best;
}

__global__ __launch_bounds__(256) void mixed_init_kernel(const MxGroup* __restrict__ grps, const int2* __restrict__ work,
                                                         const double4* __restrict__ smp, MxParams P) {
  __shared__ MxPart s_w[4];
  const int2 wk = work[blockIdx.x];
  const MxGroup g = grps[wk.x];
  const int i = wk.y * kMxRows + threadIdx.x;
  double v = -1.0;
  if (i < g.n) {
    const double4 a = smp[g.s_off + i];
    v = mixed_cov_elem(a, a, P);
    g.d[i] = v;
  }
  const MxPart best = mx_block_argmax(v, i < g.n ? i : 0x7fffffff, s_w);
  if (threadIdx.x == 0) g.part[wk.y] = best;
}

// Step `step` of every group of the chunk that is not finished; all groups start together, so an unfinished group is at column
// m = step.  Every block of a group reduces the group's partials of the previous step itself (the same order in all of them: the
// same pivot p, the same d_p), stages row p of L, computes its 256 rows of column m, updates its part of d and leaves its new partial.
// The partials are two buffers: step m reads buffer m & 1 and writes the other one, so whatever the order in which the blocks of a
// launch run, every block of a group reduces the same partials (launches of one stream follow each other); rows of d are the block's
// own, and the columns of L it reads were written by earlier launches.  A group whose largest diagonal is below tol, or which is at
// its cap, is finished: each of its blocks carries its own partial over to the other buffer (the next launch finds the group finished
// again) and returns; its first block records rank, status and the diagonal once and counts it in *ndone.
__global__ __launch_bounds__(256) void mixed_step_kernel(const MxGroup* __restrict__ grps, const int2* __restrict__ work,
                                                         const double4* __restrict__ smp, MxState* __restrict__ state, int* __restrict__ ndone,
                                                         MxParams P, double tol, int step) {
  extern __shared__ __attribute__((aligned(16))) double s_lp[];  // row p of L, columns [0, step)
  __shared__ MxPart s_w[4];
  __shared__ MxPart s_piv;
  const int2 wk = work[blockIdx.x];
  const MxGroup g = grps[wk.x];
  const int tid = threadIdx.x;
  const MxPart* part_in = g.part + (size_t)(step & 1) * g.nblk;
  MxPart* part_out = g.part + (size_t)((step & 1) ^ 1) * g.nblk;
  if (tid < 64) {
    double v = -1.0;
    int idx = 0x7fffffff;
    for (int b = tid; b < g.nblk; b += 64) {
      const MxPart q = part_in[b];
      if (mx_better(q.v, q.idx, v, idx)) { v = q.v; idx = q.idx; }
    }
#pragma unroll
    for (int sft = 1; sft < 64; sft <<= 1) {
      const double w = __shfl_xor(v, sft, 64);
      const int j = __shfl_xor(idx, sft, 64);
      if (mx_better(w, j, v, idx)) { v = w; idx = j; }
    }
    if (tid == 0) { s_piv.v = v; s_piv.idx = idx; }
  }
  __syncthreads();
  const double dp = s_piv.v;
  const int p = s_piv.idx;
  if (!(dp >= tol) || step >= g.cap || p < 0 || p >= g.n) {  // uniform over the group
    if (tid == 0) part_out[wk.y] = part_in[wk.y];
    if (wk.y == 0 && tid == 0 && !state[wk.x].done) {
      MxState st;
      st.k = step < g.cap ? step : g.cap;
      st.done = 1;
      st.status = dp < tol ? MX_OK : MX_RANK_CAP;
      st.pad = 0;
      st.maxd = dp;
      state[wk.x] = st;
      atomicAdd(ndone, 1);
    }
    return;
  }
  const int m = step;
  for (int j = tid; j < m; j += 256) s_lp[j] = g.L[(long long)j * g.ldl + p];
  __syncthreads();
  const int i = wk.y * kMxRows + tid;
  double dn = -1.0;
  if (i < g.n) {
    double c = mixed_cov_elem(smp[g.s_off + i], smp[g.s_off + p], P);
    const double* __restrict__ Li = g.L + i;
    for (int j = 0; j < m; ++j) c -= Li[(long long)j * g.ldl] * s_lp[j];
    const double l = c / sqrt(dp);
    g.L[(long long)m * g.ldl + i] = l;
    dn = g.d[i] - l * l;
    if (!(dn > 0.0) || i == p) dn = 0.0;
    g.d[i] = dn;
  }
  const MxPart best = mx_block_argmax(dn, i < g.n ? i : 0x7fffffff, s_w);
  if (tid == 0) {
    part_out[wk.y] = best;
    if (wk.y == 0) g.piv[m] = p;
  }
}

__global__ __launch_bounds__(256) void mixed_gram_kernel(const MxGroup* __restrict__ grps, const MxWork* __restrict__ work, double* __restrict__ G) {
  typedef ns_vec_t<double> vec_t;
  typedef MmT<double>::v4 acc_t;
  __shared__ __attribute__((aligned(16))) double s_a[kNsBlock][kNsPitch];
  __shared__ __attribute__((aligned(16))) double s_b[kNsBlock][kNsPitch];
  __shared__ double s_v[3][kNsChunk];
  const MxWork wk = work[blockIdx.x];
  const MxGroup g = grps[wk.grp];
  const int k0 = wk.bi * kNsBlock, l0 = wk.bj * kNsBlock;
  const bool diag = wk.bi == wk.bj;
  if (threadIdx.x < kNsChunk) s_v[0][threadIdx.x] = 1.0;
  acc_t acc[4], accr = acc_t{0, 0, 0, 0};
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = acc_t{0, 0, 0, 0};
  const int njt = normal_gram_njt(g.k, k0, l0, diag);
  for (int s0 = 0; s0 < g.ldl; s0 += kNsChunk) {  // ldl is a multiple of 64, the rows behind n are zero
    normal_gram_step<double>(s_a, s_b, s_v, kNsChunk, k0, l0, diag, njt, false,
                             [&](int row, int c) {
                               vec_t v = {0.0, 0.0};
                               if (row < g.k) v = *reinterpret_cast<const vec_t*>(g.L + (long long)row * g.ldl + s0 + c);
                               return v;
                             },
                             acc, accr);
  }
  if (njt == 0) return;
  normal_gram_store<double>(G + g.g_off, g.k, k0, l0, njt, false, acc, accr, [&](int, int) { return (double*)nullptr; });
}

// acc[t][r] of lane (col, kq) of wave w += sum_j A[i0 + 16 w + kq + 4 r][j] B[j][16 t + col] over j in [0, kpad): A is L (rows i0 .. of
// the group), B what stage_b(j, c) yields for column c of the tile.  Steps of kMxStepJ columns of L through LDS.
template <typename StageB>
__device__ __forceinline__ void mx_tile_product(const MxGroup& g, int i0, double (*s_a)[kMxPitch], double (*s_b)[kMxPitch], StageB stage_b,
                                                MmT<double>::v4 (&acc)[4]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, kq = lane >> 4;
  for (int j0 = 0; j0 < g.kpad; j0 += kMxStepJ) {
    __syncthreads();
    for (int idx = tid; idx < kMxStepJ * kMxTile; idx += 256) {
      const int jj = idx >> 6, ii = idx & 63;
      s_a[jj][ii] = g.L[(long long)(j0 + jj) * g.ldl + i0 + ii];
      s_b[jj][ii] = stage_b(j0 + jj, ii);
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kMxStepJ; kk += 4) {
      const double a = s_a[kk + kq][wave * 16 + col];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = MmT<double>::mfma(a, s_b[kk + kq][t * 16 + col], acc[t]);
    }
  }
}

// One workgroup per tile (bi, bj <= bi) of a group: sum over the tile of (C - L L^T)^2, twice for a tile below the diagonal.
__global__ __launch_bounds__(256) void mixed_cert_kernel(const MxGroup* __restrict__ grps, const MxWork* __restrict__ work,
                                                         const double4* __restrict__ smp, MxParams P, double* __restrict__ tile_sums) {
  typedef MmT<double>::v4 acc_t;
  __shared__ double s_a[kMxStepJ][kMxPitch];
  __shared__ double s_b[kMxStepJ][kMxPitch];
  __shared__ double4 s_si[kMxTile], s_sj[kMxTile];
  __shared__ double s_red[256];
  const MxWork wk = work[blockIdx.x];
  const MxGroup g = grps[wk.grp];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int i0 = wk.bi * kMxTile, j0 = wk.bj * kMxTile;
  if (tid < kMxTile) {
    const int i = i0 + tid < g.n ? i0 + tid : g.n - 1;
    s_si[tid] = smp[g.s_off + i];
  } else if (tid < 2 * kMxTile) {
    const int j = j0 + tid - kMxTile < g.n ? j0 + tid - kMxTile : g.n - 1;
    s_sj[tid - kMxTile] = smp[g.s_off + j];
  }
  acc_t acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = acc_t{0, 0, 0, 0};
  mx_tile_product(g, i0, s_a, s_b, [&](int j, int c) { return g.L[(long long)j * g.ldl + j0 + c]; }, acc);
  double sum = 0.0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ri = wave * 16 + MmT<double>::row_of(kq, r), cj = t * 16 + col;
      if (i0 + ri < g.n && j0 + cj < g.n) {
        const double diff = mixed_cov_elem(s_si[ri], s_sj[cj], P) - acc[t][r];
        sum += diff * diff;
      }
    }
  }
  s_red[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int x = 0; x < 256; ++x) tot += s_red[x];
    tile_sums[g.c_off + (long long)wk.bi * (wk.bi + 1) / 2 + wk.bj] = wk.bi == wk.bj ? tot : 2.0 * tot;
  }
}

// One workgroup per group: its tile sums in tile order (thread t takes tiles t, t + 256, ...; the 256 sums in thread order).
__global__ __launch_bounds__(256) void mixed_cert_sum_kernel(const MxGroup* __restrict__ grps, const double* __restrict__ tile_sums,
                                                             double* __restrict__ resid2) {
  __shared__ double s_red[256];
  const MxGroup g = grps[blockIdx.x];
  if (!g.L) return;  // a group that was not run has no tiles
  const long long nt = (long long)((g.n + kMxTile - 1) / kMxTile);
  const long long ntiles = nt * (nt + 1) / 2;
  double part = 0.0;
  for (long long x = threadIdx.x; x < ntiles; x += 256) part += tile_sums[g.c_off + x];
  s_red[threadIdx.x] = part;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int x = 0; x < 256; ++x) tot += s_red[x];
    resid2[blockIdx.x] = tot;
  }
}

// One workgroup per 64 x 64 tile of a group's V [n][r] = L [n][k] (U [k][r] diag(scale)).
template <typename T>
__global__ __launch_bounds__(256) void mixed_backmul_kernel(const MxGroup* __restrict__ grps, const MxWork* __restrict__ work,
                                                            const double* __restrict__ U, const double* __restrict__ scale, T* __restrict__ V) {
  typedef MmT<double>::v4 acc_t;
  __shared__ double s_a[kMxStepJ][kMxPitch];
  __shared__ double s_b[kMxStepJ][kMxPitch];
  const MxWork wk = work[blockIdx.x];
  const MxGroup g = grps[wk.grp];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int i0 = wk.bi * kMxTile, c0 = wk.bj * kMxTile;
  acc_t acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = acc_t{0, 0, 0, 0};
  mx_tile_product(g, i0, s_a, s_b,
                  [&](int j, int c) { return j < g.k && c0 + c < g.r ? U[g.u_off + (long long)j * g.r + c0 + c] * scale[g.sc_off + c0 + c] : 0.0; }, acc);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = i0 + wave * 16 + MmT<double>::row_of(kq, r);
    if (row >= g.n) continue;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int cc = c0 + t * 16 + col;
      if (cc < g.r) V[g.v_off + (long long)row * g.r + cc] = (T)acc[t][r];
    }
  }
}

}  // namespace calk
