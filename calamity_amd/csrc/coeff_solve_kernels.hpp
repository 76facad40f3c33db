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
// u, q, N and rhs are formed and accumulated in T in a fixed order (no atomics on reals: two calls give the same bits).  The Gram
// blocks and the factorisation are the shared core of normal_solve.hpp; the two kernels here fetch its operands and write its result.
#pragma once
#include "normal_solve.hpp"
#include "row_walk.hpp"

namespace calk {

struct CsGroup {      // one fitting group as the two solve kernels see it
  int b0, b1;         // its baselines
  int nvec, coff;     // length and offset of its coefficient vector in the flat planes
  int fb_log2, slice; // channel-block width of its tiles; its time slice
  long long noff;     // element offset of its N ([nvec][nvec] T) in the chunk's scratch
  long long doff;     // element offset of its factor ([nvec + 2][nvec] doubles) in the chunk's double scratch
};
struct CsWork { int grp, bi, bj, pad; };  // one 64 x 64 block (bj <= bi) of a group's N

// One wave per baseline row, four rows per block; a lane owns V = 16 / sizeof(T) adjacent channels per trip (16-byte loads).  u_r
// overwrites model_r, u_i model_i.  Channels [nfreqs, fpad) write zeros.  An autocorrelation row is a row like any other.
template <typename T>
__global__ __launch_bounds__(256) void coeff_solve_rows_kernel(T* __restrict__ model_r, T* __restrict__ model_i, T* __restrict__ q_rows,
                                                                const T* __restrict__ data_r, const T* __restrict__ data_i,
                                                                const T* __restrict__ wgts, const vec2_t<T>* __restrict__ gains,
                                                                const int2* __restrict__ bl_ant, int nbls, int nfreqs, int fpad) {
#pragma clang fp contract(off)
  constexpr int V = RowWalk<T>::V;
  typedef typename RowWalk<T>::vec_t vec_t;
  RowWalk<T> R;
  if (!R.begin(bl_ant, nbls, fpad)) return;
  GainPair<T> gp(gains, R.ant, fpad);
  for (int f = R.lane * V; f < fpad; f += 64 * V) {  // fpad is a multiple of 8: whole vectors
    const vec_t mr = R.load(model_r, f), mi = R.load(model_i, f);
    const vec_t dr = R.load(data_r, f), di = R.load(data_i, f);
    const vec_t w = R.load(wgts, f);
    gp.load(f);
    vec_t ur, ui, q;
#pragma unroll
    for (int c = 0; c < V; ++c) {
      const auto g = gp.at(c);
      const T Gr = g.Gr, Gi = g.Gi;                            // g_i conj(g_j)
      const T rr = dr[c] - (Gr * mr[c] - Gi * mi[c]);          // d - G m
      const T ri = di[c] - (Gr * mi[c] + Gi * mr[c]);
      const bool live = f + c < nfreqs;
      ur[c] = live ? w[c] * (Gr * rr + Gi * ri) : (T)0;  // conj(G) r
      ui[c] = live ? w[c] * (Gr * ri - Gi * rr) : (T)0;
      q[c] = live ? w[c] * (Gr * Gr + Gi * Gi) : (T)0;
    }
    R.store(model_r, f, ur);
    R.store(model_i, f, ui);
    R.store(q_rows, f, q);
  }
}

// One workgroup per 64 x 64 block (bi, bj <= bi) of a group's N (the Gram core of normal_solve.hpp; the operand columns of rhs are
// u_r, u_i).  The band is walked in steps of up to kNsChunk channels (tiles narrower than this: their own width): a step's piece of
// the tiles ([vector][channel], as the tiles store it) is the operand, q its weight.  Consecutive baselines of the group on one row
// block (the same tiles) are ONE walk: their q and u are summed in baseline order as the step is staged.  Folded tiles hold channels
// [0, nfreqs / 2): a second walk stages the mirror half, A[nfreqs - 1 - f][k] = (-1)^k A[f][k], against q and u of the mirrored
// channels.
template <typename T>
__global__ __launch_bounds__(256) void coeff_gram_kernel(const T* __restrict__ tiles, const long long* __restrict__ bl_tile,
                                                          const T* __restrict__ u_r, const T* __restrict__ u_i, const T* __restrict__ q_rows,
                                                          const CsGroup* __restrict__ grps, const CsWork* __restrict__ work,
                                                          T* __restrict__ nmat, T* __restrict__ rhs, int ncoef, int nfreqs, int fpad, int fold) {
  constexpr int V = 16 / (int)sizeof(T);
  typedef ns_vec_t<T> vec_t;
  typedef typename MmT<T>::v4 acc_t;
  __shared__ __attribute__((aligned(16))) T s_a[kNsBlock][kNsPitch];
  __shared__ __attribute__((aligned(16))) T s_b[kNsBlock][kNsPitch];
  __shared__ T s_v[3][kNsChunk];  // the step's sum q, sum u_r, sum u_i
  const CsWork wk = work[blockIdx.x];
  const CsGroup g = grps[wk.grp];
  const int tid = threadIdx.x;
  const int nvec = g.nvec;
  const int k0 = wk.bi * kNsBlock, l0 = wk.bj * kNsBlock;
  const bool diag = wk.bi == wk.bj;
  const int fb = 1 << g.fb_log2;
  const int cw = fb < kNsChunk ? fb : kNsChunk;  // channels per step
  const int ntiles = (fold ? nfreqs / 2 : fpad) >> g.fb_log2;
  acc_t acc[4], accr;
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = acc_t{0, 0, 0, 0};
  accr = acc_t{0, 0, 0, 0};
  const int njt = normal_gram_njt(nvec, k0, l0, diag);
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
            s_v[0][tid] = sq;
            s_v[1][tid] = sr;
            s_v[2][tid] = si;
          }
          normal_gram_step<T>(s_a, s_b, s_v, cw, k0, l0, diag, njt, wk.bj == 0,
                              [&](int row, int c) {
                                vec_t v;
#pragma unroll
                                for (int x = 0; x < V; ++x) v[x] = (T)0;
                                if (row < nvec) {
                                  v = *reinterpret_cast<const vec_t*>(tile + (long long)row * fb + s0 + c);
                                  if (mirror && (row & 1)) v = -v;
                                }
                                return v;
                              },
                              acc, accr);
        }
      }
    }
    b = e;
  }
  if (njt == 0) return;
  normal_gram_store<T>(nmat + g.noff, nvec, k0, l0, njt, wk.bj == 0, acc, accr,
                       [&](int col, int row) { return rhs + (long long)col * ncoef + g.coff + row; });
}

// One workgroup per group: normal_chol_solve of normal_solve.hpp on the group's N and rhs, its [nvec + 2][ld] matrix M in LDS when
// it fits `lds_doubles` and in the chunk's L2-resident scratch otherwise.  A singular group leaves its coefficients alone and counts
// in counts[1]; a solved group counts in counts[0]; the groups of a slice whose mask byte is 0 do neither.  The update
// c + damping delta is rounded to T once.
template <typename T>
__global__ __launch_bounds__(256) void coeff_chol_kernel(const T* __restrict__ nmat, const T* __restrict__ rhs, double* __restrict__ dscr,
                                                          const CsGroup* __restrict__ grps, const int* __restrict__ order, T* __restrict__ c_r,
                                                          T* __restrict__ c_i, int ncoef, const unsigned char* __restrict__ slice_mask,
                                                          double damping, double ridge, int* __restrict__ counts, int lds_doubles) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double s_m[];
  __shared__ double s_red[256];
  const CsGroup g = grps[order[blockIdx.x]];
  if (slice_mask && !slice_mask[g.slice]) return;
  const int tid = threadIdx.x;
  const int n = g.nvec;
  const bool in_lds = (long long)(n + 2) * (n | 1) <= lds_doubles;
  const int ld = in_lds ? (n | 1) : n;  // (odd pitch: the rows a column step reads side by side lie on different banks)
  double* M = in_lds ? s_m : dscr + g.doff;
  if (!normal_chol_solve(M, ld, n, nmat + g.noff, rhs + g.coff, rhs + (long long)ncoef + g.coff, ridge, s_red)) {
    if (tid == 0) atomicAdd(counts + 1, 1);
    return;
  }
  const double* xr = M + (long long)n * ld;
  const double* xi = M + (long long)(n + 1) * ld;
  for (int k = tid; k < n; k += 256) {
    c_r[g.coff + k] = (T)((double)c_r[g.coff + k] + damping * xr[k]);
    c_i[g.coff + k] = (T)((double)c_i[g.coff + k] + damping * xi[k]);
  }
  if (tid == 0) atomicAdd(counts, 1);
}

}  // namespace calk
