// coeff_solve_kernels.hpp -- the foreground coefficients in closed form (cal_solver_solve_coeffs): one linear least-squares solve per
// fitting group.  With the gains held fixed, chi^2 = sum w |d - g_i conj(g_j) (A c)|^2 is quadratic in a group's coefficients c.
// Baseline b of group gamma has antennas (i, j) and the real row block A_b [nfreqs][nvec]; m = A c at the current coefficients:
//   G[b][f] = g_i[f] conj(g_j[f])       u[b][f] = w conj(G) (d - G m)   (complex)       q[b][f] = w |G|^2   (real)
//   N   = sum_{b in gamma} A_b^T diag(q_b) A_b     [nvec][nvec], real symmetric
//   rhs = sum_{b in gamma} A_b^T u_b               [nvec], complex (minus half the chi-square gradient)
//   (N + ridge (tr N / nvec) I) delta = rhs        c_new = c + damping delta
// Three kernels behind the model pass:
//   coeff_solve_rows_kernel   u_r, u_i over the two model planes, q into a third plane, all in T
//   coeff_gram_kernel         N (lower triangle) and rhs of every group on the matrix cores, in T, straight from the solver's basis tiles
//   coeff_chol_kernel         per group, in double: Cholesky of N + ridge, both substitutions, the masked damped update
// u, q, N and rhs are formed and accumulated in T in a fixed order (no atomics on reals: two calls give the same bits).
#pragma once
#include "multi_mfma_kernels.hpp"

namespace calk {

struct CsGroup {      // one fitting group as the two solve kernels see it
  int b0, b1;         // its baselines
  int nvec, coff;     // length and offset of its coefficient vector in the flat planes
  int fb_log2, slice; // channel-block width of its tiles; its time slice
  long long noff;     // element offset of its N ([nvec][nvec] T) in the chunk's scratch
  long long doff;     // element offset of its factor ([nvec + 2][nvec] doubles) in the chunk's double scratch
};
struct CsWork { int grp, bi, bj, pad; };  // one 64 x 64 block (bj <= bi) of a group's N

constexpr int kCsBlock = 64;   // rows / columns of N per workgroup: one 16-row tile per wave, four column tiles
constexpr int kCsChunk = 32;   // channels staged per step (tiles narrower than this: their own width)
constexpr int kCsPitch = 36;   // elements per LDS row: 16 rows x 4 channels of an MFMA operand land on 64 distinct banks (fp32)
constexpr int kCsMaxVec = 896;

// One wave per baseline row, four rows per block; a lane owns V = 16 / sizeof(T) adjacent channels per trip (16-byte loads).  u_r
// overwrites model_r, u_i model_i.  Channels [nfreqs, fpad) write zeros.  An autocorrelation row is a row like any other.
template <typename T>
__global__ __launch_bounds__(256) void coeff_solve_rows_kernel(T* __restrict__ model_r, T* __restrict__ model_i, T* __restrict__ q_rows,
                                                                const T* __restrict__ data_r, const T* __restrict__ data_i,
                                                                const T* __restrict__ wgts, const vec2_t<T>* __restrict__ gains,
                                                                const int2* __restrict__ bl_ant, int nbls, int nfreqs, int fpad) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
  if (b >= nbls) return;
  const int2 ant = bl_ant[b];
  const long long row = (long long)b * fpad;
  const vec2_t<T>* __restrict__ gi = gains + (long long)ant.x * fpad;
  const vec2_t<T>* __restrict__ gj = gains + (long long)ant.y * fpad;
  for (int f = lane * V; f < fpad; f += 64 * V) {  // fpad is a multiple of 8: whole vectors
    const vec_t mr = *reinterpret_cast<const vec_t*>(model_r + row + f);
    const vec_t mi = *reinterpret_cast<const vec_t*>(model_i + row + f);
    const vec_t dr = *reinterpret_cast<const vec_t*>(data_r + row + f);
    const vec_t di = *reinterpret_cast<const vec_t*>(data_i + row + f);
    const vec_t w = *reinterpret_cast<const vec_t*>(wgts + row + f);
    vec_t a2[2], b2[2];  // V channels of (re, im)
    a2[0] = *reinterpret_cast<const vec_t*>(gi + f);
    a2[1] = *reinterpret_cast<const vec_t*>(gi + f + V / 2);
    b2[0] = *reinterpret_cast<const vec_t*>(gj + f);
    b2[1] = *reinterpret_cast<const vec_t*>(gj + f + V / 2);
    vec_t ur, ui, q;
#pragma unroll
    for (int c = 0; c < V; ++c) {
      const T ax = a2[(2 * c) / V][(2 * c) % V], ay = a2[(2 * c) / V][(2 * c) % V + 1];
      const T bx = b2[(2 * c) / V][(2 * c) % V], by = b2[(2 * c) / V][(2 * c) % V + 1];
      const T Gr = ax * bx + ay * by, Gi = ay * bx - ax * by;  // g_i conj(g_j)
      const T rr = dr[c] - (Gr * mr[c] - Gi * mi[c]);          // d - G m
      const T ri = di[c] - (Gr * mi[c] + Gi * mr[c]);
      const bool live = f + c < nfreqs;
      ur[c] = live ? w[c] * (Gr * rr + Gi * ri) : (T)0;  // conj(G) r
      ui[c] = live ? w[c] * (Gr * ri - Gi * rr) : (T)0;
      q[c] = live ? w[c] * (Gr * Gr + Gi * Gi) : (T)0;
    }
    *reinterpret_cast<vec_t*>(model_r + row + f) = ur;
    *reinterpret_cast<vec_t*>(model_i + row + f) = ui;
    *reinterpret_cast<vec_t*>(q_rows + row + f) = q;
  }
}

// One workgroup per 64 x 64 block (bi, bj <= bi) of a group's N; wave w owns rows [16 w, 16 w + 16) of the block and up to four
// 16 x 16 accumulator tiles (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64, the reduction index is the channel), plus, in the blocks
// of column 0, a fifth whose columns 0 and 1 are rhs_r and rhs_i (operand columns u_r, u_i).  The band is walked in steps of up to
// kCsChunk channels: the step's piece of the tiles ([vector][channel], as the tiles store it) is staged into LDS twice, plain for the
// row operand and times q (summed first, see below) for the column operand.  Consecutive baselines of the group on one row block (the same tiles) are ONE
// walk: their q and u are summed in baseline order as the step is staged.  Folded tiles hold channels [0, nfreqs / 2): a second walk
// stages the mirror half, A[nfreqs - 1 - f][k] = (-1)^k A[f][k], against q and u of the mirrored channels.  Only tiles on or below
// the diagonal are computed and only elements on or below it are written.
template <typename T>
__global__ __launch_bounds__(256) void coeff_gram_kernel(const T* __restrict__ tiles, const long long* __restrict__ bl_tile,
                                                          const T* __restrict__ u_r, const T* __restrict__ u_i, const T* __restrict__ q_rows,
                                                          const CsGroup* __restrict__ grps, const CsWork* __restrict__ work,
                                                          T* __restrict__ nmat, T* __restrict__ rhs, int ncoef, int nfreqs, int fpad, int fold) {
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  typedef typename MmT<T>::v4 acc_t;
  __shared__ __attribute__((aligned(16))) T s_a[kCsBlock][kCsPitch];
  __shared__ __attribute__((aligned(16))) T s_b[kCsBlock][kCsPitch];
  __shared__ T s_q[kCsChunk], s_ur[kCsChunk], s_ui[kCsChunk];
  const CsWork wk = work[blockIdx.x];
  const CsGroup g = grps[wk.grp];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int nvec = g.nvec;
  const int k0 = wk.bi * kCsBlock, l0 = wk.bj * kCsBlock;
  const bool diag = wk.bi == wk.bj;
  const int fb = 1 << g.fb_log2;
  const int cw = fb < kCsChunk ? fb : kCsChunk;  // channels per step
  const int vpr = cw / V;                        // 16-byte pieces per staged row
  const int ntiles = (fold ? nfreqs / 2 : fpad) >> g.fb_log2;
  const bool wave_live = k0 + wave * 16 < nvec;
  acc_t acc[4], accr;
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = acc_t{0, 0, 0, 0};
  accr = acc_t{0, 0, 0, 0};
  // column tiles this wave computes: on or below the diagonal, and inside the matrix
  int njt = 0;
  if (wave_live) {
    njt = diag ? wave + 1 : 4;
    const int have = (nvec - l0 + 15) / 16;
    if (njt > have) njt = have;
  }
  for (int b = g.b0; b < g.b1;) {
    const long long tbase = bl_tile[b];
    int e = b + 1;
    while (e < g.b1 && bl_tile[e] == tbase) ++e;
    for (int mirror = 0; mirror <= fold; ++mirror) {
      for (int ct = 0; ct < ntiles; ++ct) {
        const T* __restrict__ tile = tiles + tbase + (long long)ct * nvec * fb;
        for (int s0 = 0; s0 < fb; s0 += cw) {
          const int c0 = ct * fb + s0;  // first channel of the step (of the tile's half band when folded)
          __syncthreads();              // the previous step's operands have been read
          if (tid < cw) {
            const int f = mirror ? nfreqs - 1 - (c0 + tid) : c0 + tid;
            T sq = 0, sr = 0, si = 0;
            for (int bb = b; bb < e; ++bb) {
              const long long o = (long long)bb * fpad + f;
              sq += q_rows[o];
              sr += u_r[o];
              si += u_i[o];
            }
            s_q[tid] = sq;
            s_ur[tid] = sr;
            s_ui[tid] = si;
          }
          __syncthreads();
          for (int idx = tid; idx < kCsBlock * vpr; idx += 256) {
            const int r = idx / vpr, c = (idx - r * vpr) * V;
            vec_t va, vb;
#pragma unroll
            for (int x = 0; x < V; ++x) va[x] = vb[x] = (T)0;
            if (k0 + r < nvec) {
              va = *reinterpret_cast<const vec_t*>(tile + (long long)(k0 + r) * fb + s0 + c);
              if (mirror && ((k0 + r) & 1)) va = -va;
            }
            if (diag) vb = va;
            else if (l0 + r < nvec) {
              vb = *reinterpret_cast<const vec_t*>(tile + (long long)(l0 + r) * fb + s0 + c);
              if (mirror && ((l0 + r) & 1)) vb = -vb;
            }
#pragma unroll
            for (int x = 0; x < V; ++x) vb[x] *= s_q[c + x];  // the column operand is q A
            *reinterpret_cast<vec_t*>(&s_a[r][c]) = va;
            *reinterpret_cast<vec_t*>(&s_b[r][c]) = vb;
          }
          __syncthreads();
          if (njt > 0) {
            for (int kk = 0; kk < cw; kk += 4) {
              const T a = s_a[wave * 16 + col][kk + kq];
#pragma unroll
              for (int t = 0; t < 4; ++t)
                if (t < njt) acc[t] = MmT<T>::mfma(a, s_b[t * 16 + col][kk + kq], acc[t]);
              if (wk.bj == 0) {
                const T ub = col == 0 ? s_ur[kk + kq] : col == 1 ? s_ui[kk + kq] : (T)0;
                accr = MmT<T>::mfma(a, ub, accr);
              }
            }
          }
        }
      }
    }
    b = e;
  }
  if (njt == 0) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = k0 + wave * 16 + MmT<T>::row_of(kq, r);
    if (row >= nvec) continue;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int cc = l0 + t * 16 + col;
      if (t < njt && cc <= row) nmat[g.noff + (long long)row * nvec + cc] = acc[t][r];
    }
    if (wk.bj == 0 && col < 2) rhs[(long long)col * ncoef + g.coff + row] = accr[r];
  }
}

// One workgroup per group, everything in double.  The lower triangle of N (+ the ridge on its diagonal) and, as rows nvec and
// nvec + 1, the two right-hand sides form one [nvec + 2][ld] matrix M, in LDS when it fits `lds_doubles` and in the chunk's
// L2-resident scratch otherwise.  Left-looking Cholesky by columns: column j of every row i >= j (the right-hand-side rows included,
// which is the forward substitution) takes its dot product with row j, then the column is divided by the pivot's root.  Back
// substitution by columns, the solution of both right-hand sides collected in LDS.  A group is singular when tr N <= 0 or a pivot is
// <= 0 or not finite: it leaves its coefficients alone and counts in counts[1]; a solved group counts in counts[0]; the groups of a
// slice whose mask byte is 0 do neither.  The update c + damping delta is rounded to T once.
template <typename T>
__global__ __launch_bounds__(256) void coeff_chol_kernel(const T* __restrict__ nmat, const T* __restrict__ rhs, double* __restrict__ dscr,
                                                          const CsGroup* __restrict__ grps, const int* __restrict__ order, T* __restrict__ c_r,
                                                          T* __restrict__ c_i, int ncoef, const unsigned char* __restrict__ slice_mask,
                                                          double damping, double ridge, int* __restrict__ counts, int lds_doubles) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double s_m[];
  __shared__ double s_x[2][kCsMaxVec];
  __shared__ double s_red[256];
  const CsGroup g = grps[order[blockIdx.x]];
  if (slice_mask && !slice_mask[g.slice]) return;
  const int tid = threadIdx.x;
  const int n = g.nvec;
  const bool in_lds = (long long)(n + 2) * (n | 1) <= lds_doubles;
  const int ld = in_lds ? (n | 1) : n;  // (odd pitch: the rows a column step reads side by side lie on different banks)
  double* M = in_lds ? s_m : dscr + g.doff;
  const T* __restrict__ Ng = nmat + g.noff;
  // the trace, in a fixed order
  double part = 0;
  for (int k = tid; k < n; k += 256) part += (double)Ng[(long long)k * n + k];
  s_red[tid] = part;
  __syncthreads();
  if (tid == 0) {
    double tr = 0;
    for (int k = 0; k < 256; ++k) tr += s_red[k];
    s_red[0] = tr;
  }
  __syncthreads();
  const double tr = s_red[0];
  if (!(tr > 0.0) || !isfinite(tr)) {
    if (tid == 0) atomicAdd(counts + 1, 1);
    return;
  }
  const double shift = ridge * (tr / n);
  for (int idx = tid; idx < n * n; idx += 256) {
    const int i = idx / n, k = idx - i * n;
    if (k <= i) M[(long long)i * ld + k] = (double)Ng[idx] + (k == i ? shift : 0.0);
  }
  for (int k = tid; k < n; k += 256) {
    M[(long long)n * ld + k] = (double)rhs[g.coff + k];
    M[(long long)(n + 1) * ld + k] = (double)rhs[(long long)ncoef + g.coff + k];
  }
  __syncthreads();
  for (int j = 0; j < n; ++j) {
    const double* __restrict__ Lj = M + (long long)j * ld;
    for (int i = j + tid; i < n + 2; i += 256) {
      double* Li = M + (long long)i * ld;
      double s = Li[j];
      for (int k = 0; k < j; ++k) s -= Li[k] * Lj[k];
      Li[j] = s;
    }
    __syncthreads();
    const double d = M[(long long)j * ld + j];  // the same value in every thread: the branch is uniform
    if (!(d > 0.0) || !isfinite(d)) {
      if (tid == 0) atomicAdd(counts + 1, 1);
      return;
    }
    __syncthreads();  // every thread has read the pivot
    const double root = sqrt(d);
    for (int i = j + 1 + tid; i < n + 2; i += 256) M[(long long)i * ld + j] /= root;
    if (tid == 0) M[(long long)j * ld + j] = root;
    __syncthreads();
  }
  // L^T x = y for the two rows y = M[n], M[n + 1]
  double* yr = M + (long long)n * ld;
  double* yi = M + (long long)(n + 1) * ld;
  for (int j = n - 1; j >= 0; --j) {
    const double* __restrict__ Lj = M + (long long)j * ld;
    const double xr = yr[j] / Lj[j], xi = yi[j] / Lj[j];
    for (int k = tid; k < j; k += 256) {
      yr[k] -= Lj[k] * xr;
      yi[k] -= Lj[k] * xi;
    }
    if (tid == 0) {
      s_x[0][j] = xr;
      s_x[1][j] = xi;
    }
    __syncthreads();
  }
  for (int k = tid; k < n; k += 256) {
    c_r[g.coff + k] = (T)((double)c_r[g.coff + k] + damping * s_x[0][k]);
    c_i[g.coff + k] = (T)((double)c_i[g.coff + k] + damping * s_x[1][k]);
  }
  if (tid == 0) atomicAdd(counts, 1);
}

}  // namespace calk
