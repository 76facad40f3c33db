// solve_plan.hpp -- what the closed-form calls (solve_gains, solve_coeffs, solve_gain_coeffs, solve_gain_time_coeffs, fit_errors,
// gain_basis_errors) decide
// before they launch, on the host alone, from what plan_problem() (problem_plan.hpp) yields; the antenna lists without autocorrelations
// are its antenna_lists.  No HIP or RCCL runtime call and no solver: SolverT uploads these plans at the first call that needs them;
// cal_debug_solve_plan returns them as bytes (tests/test_solve_plan_host.py).  A group's result does not depend on its chunk, but the
// order of the groups and of the block pairs is the order the kernels work in: the stable sort and the loops below are part of the plan.
#pragma once
#include "problem_plan.hpp"
#include "fit_error_kernels.hpp"
#include "gain_time_basis_kernels.hpp"

namespace {

constexpr int64_t kCsScratchDefault = 256ll << 20;  // bytes of scratch a chunk may take (one group, one row alone may take more)
constexpr int kCsLdsDoubles = 16384;                // 128 KB: a factor of up to 126 vectors stays in LDS

// dynamic LDS of a Cholesky launch whose largest system has n unknowns: [n + 2] rows of n | 1 doubles, or the cap (the factor in scratch)
inline bool chol_in_lds(int n) { return (long long)(n + 2) * (n | 1) <= kCsLdsDoubles; }
inline size_t chol_lds_bytes(int n) { return (size_t)std::min<long long>((long long)(n + 2) * (n | 1), kCsLdsDoubles) * sizeof(double); }

// positions of a chunk of groups in order / work / lwork (l0 == l1 where the plan has no leverage work); dynamic LDS of its factor launch
struct GroupChunk { int g0, g1, w0, w1, l0, l1; size_t lds; };

struct GroupPlan {
  std::vector<int> order;         // groups heaviest first (as everywhere: the tail of a launch is made of the lightest)
  std::vector<CsWork> work;       // the Gram kernel's 64 x 64 block pairs, chunk by chunk
  std::vector<long long> xoff;    // [ngrps] element offset of a group's extra elements (fit_errors: W) in the chunk's third scratch; empty without any
  std::vector<FeWork> lwork;      // fit_errors: the leverage kernel's work (plan_leverage_work)
  std::vector<GroupChunk> chunks;
  long long n_max = 0, d_max = 0, x_max = 0;  // elements the three scratch buffers need: N (T), the factor (double), the extra (T)
  int npieces = 0;
};

// The groups of `grp` (the planner's cs_grp) in `order`, cut into chunks whose N (T), extra elements (T; extra[g] of group g, none where
// the vector is empty) and factor (double) stay under `bound` bytes -- a group that alone needs more is a chunk of its own.  Every
// chunk reuses the scratch buffers from offset 0: the offsets are written into the groups' noff / doff and into xoff.
inline GroupPlan plan_group_chunks(std::vector<CsGroup>& grp, size_t elem, int64_t bound, const std::vector<long long>& extra) {
  GroupPlan P;
  const int ngrps = (int)grp.size();
  std::vector<int> order(ngrps);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return grp[a].nvec > grp[b].nvec; });
  std::vector<CsWork> work;
  std::vector<long long> xoff(extra.size(), 0);
  for (int p = 0; p < ngrps;) {
    long long noff = 0, doff = 0, xo = 0;
    int max_nvec = 0;
    GroupChunk ch{p, p, (int)work.size(), 0, 0, 0, 0};
    for (; p < ngrps; ++p) {
      CsGroup& g = grp[order[p]];
      const long long nn = (long long)g.nvec * g.nvec, dd = (long long)(g.nvec + 2) * g.nvec, xx = extra.empty() ? 0 : extra[order[p]];
      if (p > ch.g0 && (noff + nn + xo + xx) * (long long)elem + (doff + dd) * 8 > bound) break;
      g.noff = noff;
      g.doff = doff;
      if (!extra.empty()) xoff[order[p]] = xo;
      noff += nn;
      doff += dd;
      xo += xx;
      max_nvec = std::max(max_nvec, g.nvec);
      const int nb = (g.nvec + kNsBlock - 1) / kNsBlock;
      for (int bi = 0; bi < nb; ++bi)
        for (int bj = 0; bj <= bi; ++bj) work.push_back(CsWork{order[p], bi, bj, 0});
    }
    ch.g1 = p;
    ch.w1 = (int)work.size();
    ch.lds = chol_lds_bytes(max_nvec);
    P.chunks.push_back(ch);
    P.n_max = std::max(P.n_max, noff);
    P.d_max = std::max(P.d_max, doff);
    P.x_max = std::max(P.x_max, xo);
  }
  P.order = std::move(order);
  P.work = std::move(work);
  P.xoff = std::move(xoff);
  return P;
}

// fit_errors: W (padded to whole 16 x 16 tiles, T) is counted in a chunk's bytes, so its chunks are cut elsewhere than solve_coeffs'
inline std::vector<long long> fit_error_extra(const std::vector<CsGroup>& cs_grp) {
  std::vector<long long> x(cs_grp.size());
  for (size_t g = 0; g < x.size(); ++g) x[g] = (long long)fe_pad(cs_grp[g].nvec) * fe_pad(cs_grp[g].nvec);
  return x;
}

// The leverage kernel's work of every chunk: every run of a group's baselines on one row block (equal bl_tile) x every kFePiece channels
// of the band tiles_cover channels wide (the half band where the problem folds).
inline void plan_leverage_work(GroupPlan& P, const std::vector<CsGroup>& grp, const std::vector<long long>& bl_tile, int tiles_cover) {
  P.npieces = (tiles_cover + kFePiece - 1) / kFePiece;
  for (GroupChunk& ch : P.chunks) {
    ch.l0 = (int)P.lwork.size();
    for (int p = ch.g0; p < ch.g1; ++p) {
      const CsGroup& g = grp[P.order[p]];
      for (int b = g.b0; b < g.b1;) {
        int e = b + 1;
        while (e < g.b1 && bl_tile[e] == bl_tile[b]) ++e;
        for (int piece = 0; piece < P.npieces; ++piece) P.lwork.push_back(FeWork{P.order[p], b, e, piece});
        b = e;
      }
    }
    ch.l1 = (int)P.lwork.size();
  }
}

// solve_gain_coeffs (L == 0) and solve_gain_time_coeffs: what one row of a chunk -- an antenna row, or an antenna over all its times --
// takes in the call's scratch buffers, and how many rows a chunk holds.  K: vectors of the frequency basis (0: none), L: of the time
// basis, Tn: times.  The system of a row has n = K, or L K, unknowns; without a frequency basis the channels are solved one by one.
struct RowChunks {
  int n;
  long long m_row, n_row;  // T elements per row: M_{t,a} of every time (time basis over a frequency basis), N_a
  long long d_row;         // doubles per row: the factor where it leaves LDS, or the channel systems beyond kTimeTile vectors
  bool in_lds;
  size_t lds;              // dynamic LDS of the Cholesky launch
  int rows;                // rows per chunk: what stays under the bound, at least one
  long long x_row;         // T elements per row beyond the solves' own (gain_basis_errors: W); 0 for the solves
};
// gain_basis_errors: W of a row (padded to whole 16 x 16 tiles, T) is counted in a chunk's bytes, so its chunks are cut elsewhere than
// the solves'; the channel systems of a time basis alone keep no W
inline long long gain_error_extra(int K, int L) {
  const long long np = K > 0 ? fe_pad((L > 0 ? L : 1) * K) : 0;
  return np * np;
}
inline RowChunks plan_row_chunks(int K, int L, int Tn, int nfreqs, size_t elem, int64_t bound, int nrows, long long extra = 0) {
  RowChunks r{};
  r.n = (L > 0 ? L : 1) * K;
  r.in_lds = chol_in_lds(r.n);
  r.lds = chol_lds_bytes(r.n);
  if (K > 0) {
    r.m_row = L > 0 ? (long long)Tn * K * K : 0;
    r.n_row = (long long)r.n * r.n;
    r.d_row = r.in_lds ? 0 : (long long)(r.n + 2) * r.n;
  } else {
    r.d_row = L <= kTimeTile ? 0 : (long long)nfreqs * (L * (L + 1) / 2 + 2 * L);
  }
  r.x_row = extra;
  const long long row_bytes = std::max<long long>(1, (r.m_row + r.n_row + r.x_row) * (long long)elem + r.d_row * 8);
  r.rows = (int)std::max<long long>(1, std::min<long long>(nrows, bound / row_bytes));
  return r;
}

}  // namespace
