// plan_sanitize.hip -- the set-up planner (calamity_amd/csrc/problem_plan.hpp), the planner of the closed-form calls
// (calamity_amd/csrc/solve_plan.hpp), of the post-fit reports (calamity_amd/csrc/report_plan.hpp), the step's shape (calamity_amd/csrc/step_plan.hpp) and the two-loop recursion of L-BFGS on
// coefficients (calamity_amd/csrc/lbfgs_core.hpp) under the host sanitizers, with no device and no interpreter: four problems built in code (folded STREAM, heads of baselines that share tiles, forced dense, multi-baseline runs),
// planned for fp32 and fp64; the closed-form plans, the delay-spectrum plan, the cross-spectrum plan, the delay / fringe-rate plan and the plan of the redundant averages (each with its refusals) at the default scratch bound and at a bound of 1 byte, the degeneracy plan in both modes,
// the caller's arrays of exactly the sizes the planners may read; plan_step over its whole input
// table; lbfgs_two_loop on Gram matrices of 0 .. 16 pairs held in arrays of exactly the sizes it may touch.  Exits non-zero on a planner error or an inconsistent plan; the sanitizers abort on a finding.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -o plan_sanitize tools/plan_sanitize.hip && ./plan_sanitize
#include "../calamity_amd/csrc/solve_plan.hpp"
#include "../calamity_amd/csrc/step_plan.hpp"
#include "../calamity_amd/csrc/report_plan.hpp"
#include "../calamity_amd/csrc/lbfgs_core.hpp"

#include <cstdint>
#include <limits>

namespace {

struct Case {
  const char* name;
  int nants, nfreqs, nslices, layout, kernel_path;
  std::vector<int> nvec, nrowblk;          // per basis block
  std::vector<int> grp_basis, grp_nbl;     // per group
  std::vector<int> rowblk, alias;          // per baseline (empty: none)
};

template <typename T>
int run(const Case& c) {
  const int nbasis = (int)c.nvec.size(), ngrps = (int)c.grp_basis.size();
  std::vector<int64_t> off(nbasis + 1, 0);
  for (int u = 0; u < nbasis; ++u) off[u + 1] = off[u] + (int64_t)c.nvec[u] * c.nrowblk[u] * c.nfreqs;
  // mirror-symmetric blocks, A[F-1-f][k] = (-1)^k A[f][k] exactly: a single-row-block STREAM problem folds in both dtypes
  std::vector<T> data((size_t)off[nbasis]);
  uint32_t seed = 12345u;
  for (int u = 0; u < nbasis; ++u)
    for (int r = 0; r < c.nrowblk[u]; ++r)
      for (int f = 0; f < c.nfreqs; ++f)
        for (int k = 0; k < c.nvec[u]; ++k) {
          T* blk = data.data() + off[u] + (size_t)r * c.nfreqs * c.nvec[u];
          if (f < (c.nfreqs + 1) / 2) {
            seed = seed * 1664525u + 1013904223u;
            blk[(size_t)f * c.nvec[u] + k] = (T)((seed >> 8) * (1.0 / 16777216.0) - 0.5);
          } else {
            const T m = blk[(size_t)(c.nfreqs - 1 - f) * c.nvec[u] + k];
            blk[(size_t)f * c.nvec[u] + k] = (k & 1) ? -m : m;
          }
        }
  std::vector<int> start(ngrps + 1, 0);
  for (int g = 0; g < ngrps; ++g) start[g + 1] = start[g] + c.grp_nbl[g];
  const int nbls = start[ngrps], nas = c.nants / c.nslices;
  // baselines listed slice by slice: group g lies in slice g * nslices / ngrps, its baselines walk that slice's antenna pairs
  std::vector<int> a0(nbls), a1(nbls);
  for (int g = 0; g < ngrps; ++g)
    for (int b = start[g]; b < start[g + 1]; ++b) {
      const int t = (int)((long long)g * c.nslices / ngrps);
      a0[b] = t * nas + b % nas;
      a1[b] = t * nas + (b % nas + 1 + (b / nas) % (nas - 1)) % nas;
    }
  cal_problem_desc d{};
  d.nants = c.nants; d.nfreqs = c.nfreqs; d.ngrps = ngrps; d.nbls = nbls; d.nbasis = nbasis;
  d.basis_offset = off.data(); d.basis_nvec = c.nvec.data(); d.basis_nrowblk = c.nrowblk.data(); d.basis_data = data.data();
  d.grp_basis = c.grp_basis.data(); d.grp_bl_start = start.data(); d.bl_ant0 = a0.data(); d.bl_ant1 = a1.data();
  d.bl_rowblk = c.rowblk.empty() ? nullptr : c.rowblk.data();
  d.bl_alias = c.alias.empty() ? nullptr : c.alias.data();
  d.layout = c.layout; d.kernel_path = c.kernel_path; d.nslices = c.nslices;
  ProblemPlan<T> p;
  const int rc = plan_problem(&d, p);
  if (rc != CAL_OK) {
    fprintf(stderr, "%s (%d-byte reals): planner error %d: %s\n", c.name, (int)sizeof(T), rc, g_err.c_str());
    return 1;
  }
  printf("%-12s %d-byte reals: fpad %d, %d items (%d simple, %d plain), fold %d, gc_direct %d, %d runs, %d heads (%d matrix-core, grid %d), dense %d: %d panels, grid %d\n",
         c.name, (int)sizeof(T), p.fpad, p.nitems, p.nitems_simple, p.nitems_plain, (int)p.fold, (int)p.gc_direct, (int)p.runs.size(), p.nheads, p.nheads_mfma,
         p.mm_grid, (int)p.mf_ok, p.mf_npanels, p.mf_grid);
  // the plans of the closed-form calls: one chunk at the default bound; at 1 byte every group, every row a chunk of its own
  std::vector<int> ptr;
  std::vector<int2> ent;
  antenna_lists(p.nants, p.bl_ant, true, ptr, ent);
  int bad = ptr[p.nants] > 2 * p.nbls || ent.empty();
  for (const int64_t bound : {kCsScratchDefault, (int64_t)1}) {
    std::vector<CsGroup> grp = p.cs_grp;
    const GroupPlan cs = plan_group_chunks(grp, sizeof(T), bound, {});
    GroupPlan fe = plan_group_chunks(grp, sizeof(T), bound, fit_error_extra(grp));
    plan_leverage_work(fe, grp, p.bl_tile, p.fold ? p.nfreqs / 2 : p.fpad);
    const RowChunks rf = plan_row_chunks(150, 0, 0, p.nfreqs, sizeof(T), bound, p.nants);
    const RowChunks rt = plan_row_chunks(20, 9, p.nslices, p.nfreqs, sizeof(T), bound, p.na_slice);
    const RowChunks rc = plan_row_chunks(0, 9, p.nslices, p.nfreqs, sizeof(T), bound, p.na_slice);
    const size_t want = bound == 1 ? (size_t)p.ngrps : 1;
    bad += cs.chunks.size() != want || fe.chunks.size() != want || cs.chunks.back().g1 != p.ngrps || fe.chunks.back().g1 != p.ngrps ||
           fe.chunks.back().l1 != (int)fe.lwork.size() || cs.chunks.back().w1 != (int)cs.work.size() || rf.rows < 1 || rt.rows < 1 || rc.rows < 1;
    printf("%-12s   bound %lld: %zu / %zu chunks, %zu Gram blocks, %zu leverage items in %d pieces, scratch %lld + %lld + %lld elements; rows per chunk %d, %d, %d\n",
           c.name, (long long)bound, cs.chunks.size(), fe.chunks.size(), cs.work.size(), fe.lwork.size(), fe.npieces, fe.n_max, fe.d_max, fe.x_max, rf.rows,
           rt.rows, rc.rows);
  }
  if (bad) fprintf(stderr, "%s (%d-byte reals): the closed-form plans are inconsistent\n", c.name, (int)sizeof(T));
  // the plans of the post-fit reports: 37 delays, rows dealt over three of four bins and every seventh left out; one chunk, then one per row
  const int nd = 37, nbins = 4;
  std::vector<T> op_r((size_t)p.nfreqs * nd, (T)1), op_i(op_r);
  std::vector<double> norm_f(p.nfreqs, 1.0), antpos(2 * (size_t)p.na_slice), freqs(p.nfreqs);
  std::vector<int> bin_of_bl(p.nbls);
  for (int b = 0; b < p.nbls; ++b) bin_of_bl[b] = b % 7 == 3 ? -1 : b % (nbins - 1);
  for (size_t k = 0; k < antpos.size(); ++k) antpos[k] = 14.6 * (double)((k * 7) % 11);
  for (int f = 0; f < p.nfreqs; ++f) freqs[f] = 100e6 + 400e3 * f;
  const cal_delay_spectrum_desc sd{nd, 7, 0, nbins, bin_of_bl.data(), op_r.data(), op_i.data(), norm_f.data()};
  int rbad = 0;
  for (const int64_t bound : {kCsScratchDefault, (int64_t)1}) {
    DelaySpectrumPlan<T> P;
    rbad += plan_delay_spectrum(p.nbls, p.nfreqs, p.fpad, &sd, bound, true, P) != CAL_OK || P.nchunks != (bound == 1 ? p.nbls : 1);
    int rows = 0;
    for (size_t k = 0; k < P.chunk_ptr.size(); k += 2) rows += P.chunk_ptr[k + 1] - P.chunk_ptr[k];
    rbad += rows != (int)P.bin_ent.size() || P.bin_ent.size() != (size_t)(p.nbls - (p.nbls + 3) / 7);
  }
  // the cross spectrum's plan: a pair per row (row b with row (b + 5) % nbls), scales and bins of exactly npairs entries; then its refusals
  {
    const int np = p.nbls;
    std::vector<int32_t> pairs(2 * (size_t)np), bin_of_pair(np);
    std::vector<double> scale(2 * (size_t)np, 1.5);
    for (int k = 0; k < np; ++k) pairs[2 * k] = k, pairs[2 * k + 1] = (k + 5) % np, bin_of_pair[k] = k % 7 == 3 ? -1 : k % (nbins - 1);
    cal_delay_cross_desc cd{nd, 7, 0, np, pairs.data(), scale.data(), 3, nbins, bin_of_pair.data(), op_r.data(), op_i.data(), norm_f.data()};
    for (const int64_t bound : {kCsScratchDefault, (int64_t)1}) {
      DelayCrossPlan<T> P;
      rbad += plan_delay_cross(p.nbls, p.nfreqs, p.fpad, &cd, bound, P) != CAL_OK || P.nchunks != (bound == 1 ? np : 1) || P.scale.size() != 2 * (size_t)np;
      int n = 0;
      for (size_t k = 0; k < P.chunk_ptr.size(); k += 2) n += P.chunk_ptr[k + 1] - P.chunk_ptr[k];
      rbad += n != (int)P.bin_ent.size() || P.bin_ent.size() != (size_t)(np - (np + 3) / 7) || P.n_x != (size_t)3 * 4 * P.cpairs * P.xpitch;
    }
    DelayCrossPlan<T> R;
    pairs[2 * (size_t)np - 1] = p.nbls;  // a row past the last
    rbad += plan_delay_cross(p.nbls, p.nfreqs, p.fpad, &cd, kCsScratchDefault, R) != CAL_ERR_INVALID;
    pairs[2 * (size_t)np - 1] = 0;
    scale[1] = std::numeric_limits<double>::infinity();
    rbad += plan_delay_cross(p.nbls, p.nfreqs, p.fpad, &cd, kCsScratchDefault, R) != CAL_ERR_INVALID;
    cd.scale = nullptr;  // no scales: ones
    cd.stats = 4;
    rbad += plan_delay_cross(p.nbls, p.nfreqs, p.fpad, &cd, kCsScratchDefault, R) != CAL_ERR_INVALID;
    cd.stats = 2;
    rbad += plan_delay_cross(p.nbls, p.nfreqs, p.fpad, &cd, kCsScratchDefault, R) != CAL_OK || R.nstat != 1 || R.scale[1] != 1.0;
  }
  // the delay / fringe-rate plan: a group of three rows per row (b, (b + 5) % nbls, b again: a repeat), scales of exactly ngroups ntimes
  // entries, opt of exactly ntimes nrates, bins of exactly ngroups; both bounds; then its refusals
  {
    const int ng = p.nbls, nt = 3, nr = 2;
    std::vector<int32_t> rows((size_t)ng * nt), bin_of_group(ng);
    std::vector<double> scale((size_t)ng * nt, 1.5), opt_r((size_t)nt * nr, 0.5), opt_i((size_t)nt * nr, -0.25);
    for (int k = 0; k < ng; ++k) rows[3 * k] = k, rows[3 * k + 1] = (k + 5) % ng, rows[3 * k + 2] = k, bin_of_group[k] = k % 7 == 3 ? -1 : k % (nbins - 1);
    cal_delay_fringe_desc fd{nd, 7, 0, ng, nt, nr, rows.data(), scale.data(), nbins, bin_of_group.data(), op_r.data(), op_i.data(), norm_f.data(),
                             opt_r.data(), opt_i.data()};
    for (const int64_t bound : {kCsScratchDefault, (int64_t)1}) {
      DelayFringePlan<T> P;
      rbad += plan_delay_fringe(p.nbls, p.nfreqs, p.fpad, &fd, bound, P) != CAL_OK || P.nchunks != (bound == 1 ? ng : 1) || P.cgroups != (bound == 1 ? 1 : ng) ||
              P.scale.size() != (size_t)ng * nt || P.opt.size() != 2 * (size_t)nt * nr || P.opt[0] != 0.5 || P.opt[(size_t)nt * nr] != -0.25;
      int n = 0;
      for (size_t k = 0; k < P.chunk_ptr.size(); k += 2) n += P.chunk_ptr[k + 1] - P.chunk_ptr[k];
      rbad += n != (int)P.bin_ent.size() || P.bin_ent.size() != (size_t)(ng - (ng + 3) / 7) || P.n_x != (size_t)3 * 2 * P.cgroups * nt * P.xpitch ||
              P.n_y != (size_t)3 * 2 * P.cgroups * nt * nd || P.n_pow != (size_t)3 * P.cgroups * nr * nd;
    }
    DelayFringePlan<T> R;
    rows[(size_t)ng * nt - 1] = p.nbls;  // a row past the last
    rbad += plan_delay_fringe(p.nbls, p.nfreqs, p.fpad, &fd, kCsScratchDefault, R) != CAL_ERR_INVALID;
    rows[(size_t)ng * nt - 1] = 0;
    scale[1] = std::numeric_limits<double>::infinity();
    rbad += plan_delay_fringe(p.nbls, p.nfreqs, p.fpad, &fd, kCsScratchDefault, R) != CAL_ERR_INVALID;
    fd.scale = nullptr;  // no scales: ones
    opt_i[(size_t)nt * nr - 1] = std::numeric_limits<double>::quiet_NaN();
    rbad += plan_delay_fringe(p.nbls, p.nfreqs, p.fpad, &fd, kCsScratchDefault, R) != CAL_ERR_INVALID;
    opt_i[(size_t)nt * nr - 1] = 0.0;
    for (const int bad_nt : {0, 65}) {
      fd.ntimes = bad_nt;
      rbad += plan_delay_fringe(p.nbls, p.nfreqs, p.fpad, &fd, kCsScratchDefault, R) != CAL_ERR_INVALID;
    }
    fd.ntimes = nt;
    for (const int bad_nr : {0, 65}) {
      fd.nrates = bad_nr;
      rbad += plan_delay_fringe(p.nbls, p.nfreqs, p.fpad, &fd, kCsScratchDefault, R) != CAL_ERR_INVALID;
    }
    fd.nrates = nr;
    fd.ngroups = 0;
    rbad += plan_delay_fringe(p.nbls, p.nfreqs, p.fpad, &fd, kCsScratchDefault, R) != CAL_ERR_INVALID;
    fd.ngroups = ng;
    bin_of_group[ng - 1] = nbins;  // a bin past the last
    rbad += plan_delay_fringe(p.nbls, p.nfreqs, p.fpad, &fd, kCsScratchDefault, R) != CAL_ERR_INVALID;
    bin_of_group[ng - 1] = -1;
    fd.what = 4;
    rbad += plan_delay_fringe(p.nbls, p.nfreqs, p.fpad, &fd, kCsScratchDefault, R) != CAL_OK || R.nq != 1 || R.scale[1] != 1.0;
  }
  // the plan of the redundant averages: a group of two sets per row (k % 4 members and one, the first group's first set empty), member
  // arrays of exactly nmembers entries and a set_ptr of exactly ngroups ntimes + 1; both bounds; then its refusals
  {
    const int ng = p.nbls, nt = 2, nr = 2;
    std::vector<int64_t> set_ptr(1, 0);
    std::vector<int32_t> member_row, bin_of_group(ng);
    for (int k = 0; k < ng; ++k) {
      for (int j = 0; j < k % 4; ++j) member_row.push_back((k + 3 * j) % ng);
      set_ptr.push_back((int64_t)member_row.size());
      member_row.push_back(k);
      set_ptr.push_back((int64_t)member_row.size());
      bin_of_group[k] = k % 7 == 3 ? -1 : k % (nbins - 1);
    }
    const int64_t nm = (int64_t)member_row.size();
    std::vector<double> wgt((size_t)nm, 0.75), scale((size_t)ng * nt, 1.5), opt_r((size_t)nt * nr, 0.5), opt_i((size_t)nt * nr, -0.25);
    std::vector<uint8_t> cj((size_t)nm, 0);
    cj[nm - 1] = 1;
    cal_delay_coherent_desc kd{nd, 7, 1, ng, nt, nr, set_ptr.data(), member_row.data(), wgt.data(), cj.data(), 1, scale.data(), nbins, bin_of_group.data(),
                               op_r.data(), op_i.data(), norm_f.data(), opt_r.data(), opt_i.data(), nm};
    for (const int64_t bound : {kCsScratchDefault, (int64_t)1}) {
      DelayCoherentPlan<T> P;
      rbad += plan_delay_coherent(p.nbls, p.nfreqs, p.fpad, &kd, bound, P) != CAL_OK || P.F.nchunks != (bound == 1 ? ng : 1) || P.F.cgroups != (bound == 1 ? 1 : ng) ||
              P.set_ptr.size() != (size_t)ng * nt + 1 || P.member_row.size() != (size_t)nm || P.member_wgt[0] != 0.75 || P.member_conj[nm - 1] != 1 ||
              P.chunk_members.size() != 2 * (size_t)P.F.nchunks || P.chunk_members[0] != 0 || P.chunk_members.back() != nm ||
              P.n_mask != (size_t)P.F.cgroups * nt * P.F.xpitch || P.nspans < 1;
      for (int c = 1; c < P.F.nchunks; ++c) rbad += P.chunk_members[2 * c] != P.chunk_members[2 * c - 1];
    }
    DelayCoherentPlan<T> R;
    auto refused = [&]() { return plan_delay_coherent(p.nbls, p.nfreqs, p.fpad, &kd, kCsScratchDefault, R) != CAL_ERR_INVALID; };
    member_row[nm - 1] = p.nbls;  // a row past the last
    rbad += refused();
    member_row[nm - 1] = 0;
    wgt[1] = -1.0;
    rbad += refused();
    wgt[1] = std::numeric_limits<double>::quiet_NaN();
    rbad += refused();
    kd.member_wgt = nullptr;  // no coefficients: ones
    cj[0] = 2;
    rbad += refused();
    kd.member_conj = nullptr;  // no flags: none
    set_ptr[0] = 1;
    rbad += refused();
    set_ptr[0] = 0;
    std::swap(set_ptr[2], set_ptr[3]);  // (set_ptr[3] > set_ptr[2]: group 1 has a member in its first set) it falls
    rbad += refused();
    std::swap(set_ptr[2], set_ptr[3]);
    kd.nmembers = nm - 1;
    rbad += refused();
    kd.nmembers = ((int64_t)1 << 30) + 1;
    rbad += refused();
    kd.nmembers = nm;
    for (const int bad_w : {-1, 2}) {
      kd.weighting = bad_w;
      rbad += refused();
    }
    kd.weighting = 0;
    for (const int bad_nt : {0, 65}) {
      kd.ntimes = bad_nt;
      rbad += refused();
    }
    kd.ntimes = nt;
    kd.set_ptr = nullptr;
    rbad += refused();
    kd.set_ptr = set_ptr.data();
    kd.what = 4;
    rbad += plan_delay_coherent(p.nbls, p.nfreqs, p.fpad, &kd, kCsScratchDefault, R) != CAL_OK || R.F.nq != 1 || R.member_wgt[1] != 1.0 || R.member_conj[0] != 0;
  }
  for (const bool band : {false, true}) {
    DegeneracyPlan P;
    rbad += plan_degeneracies(p.bl_ant, p.nants, p.nslices, p.nfreqs, p.fpad, band, antpos.data(), band ? freqs.data() : nullptr, P) != CAL_OK ||
            P.segs.empty() || P.segs.back().e1 != p.nbls || P.pack_geo().size() != P.geo_maxd() + p.nslices || P.pack_idx().size() != P.idx_segs() + 4 * (size_t)P.nseg;
  }
  if (rbad) fprintf(stderr, "%s (%d-byte reals): the report plans are inconsistent: %s\n", c.name, (int)sizeof(T), g_err.c_str());
  return bad || rbad ? 1 : 0;
}

// plan_step over every combination of its inputs (2^13 flag settings x 4 launch modes), through the layouts of cal_debug_step_shape:
// the loop bookkeeping and the partial coefficient-gradient sums of a step happen exactly once
int walk_step_shapes() {
  int bad = 0, replays = 0, tails = 0;
  for (int mode = CAL_LAUNCH_AUTO; mode <= CAL_LAUNCH_GRAPH; ++mode)
    for (int bits = 0; bits < (1 << 13); ++bits) {
      int32_t in[14], out[kStepShape];
      for (int i = 0, k = 0; i < 14; ++i) in[i] = i == 7 ? mode : (bits >> k++) & 1;
      const StepShape s = plan_step(step_inputs_from(in));
      step_shape_to(s, out);
      const bool own = s.update == UPDATE_FUSED || s.update == UPDATE_TAIL;
      bad += s.finalize == own || (s.partial_reduce && own) || (s.update != UPDATE_NONE) != (in[10] != 0) || out[7] != (s.Rk ? 3 : 1) || out[9] != s.update;
      replays += s.replay;
      tails += s.tail1;
    }
  printf("step shapes   %d inputs: %d with the one-launch tail, %d replayed from a graph\n", 4 << 13, tails, replays);
  if (bad) fprintf(stderr, "plan_step: %d inconsistent shapes\n", bad);
  return bad ? 1 : 0;
}

// lbfgs_two_loop for p = 0 .. kLbfgsMaxHistory pairs of positive curvature (y = H s, H diagonal and positive) in dimension 40, the vectors
// held in a permuted order behind idx: every array has exactly the size the function may touch, the slope must be finite and negative,
// and d = sum delta_j b_j must give that slope again
int walk_lbfgs() {
  int bad = 0;
  uint32_t seed = 777u;
  auto rnd = [&]() {
    seed = seed * 1664525u + 1013904223u;
    return (seed >> 8) * (1.0 / 16777216.0) - 0.5;
  };
  const int dim = 40;
  for (int p = 0; p <= calk::kLbfgsMaxHistory; ++p) {
    const int n = 2 * p + 1;
    std::vector<std::vector<double>> b(n, std::vector<double>(dim));
    std::vector<double> h(dim);
    for (double& x : h) x = 0.5 + (rnd() + 0.5);
    for (int i = 0; i < p; ++i)
      for (int k = 0; k < dim; ++k) {
        b[i][k] = rnd();
        b[p + i][k] = h[k] * b[i][k];
      }
    for (int k = 0; k < dim; ++k) b[2 * p][k] = rnd();
    std::vector<int> idx(n);
    for (int j = 0; j < n; ++j) idx[j] = (j * 7 + 3) % n;  // a permutation: gcd(7, n) = 1 for every odd n <= 33 but 7 and 21 ...
    if (n % 7 == 0)
      for (int j = 0; j < n; ++j) idx[j] = n - 1 - j;        // ... which get the reversal
    std::vector<double> gram((size_t)n * n), delta(n), alpha(p);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        double acc = 0;
        for (int k = 0; k < dim; ++k) acc += b[i][k] * b[j][k];
        gram[(size_t)idx[i] * n + idx[j]] = acc;
      }
    const double slope = calk::lbfgs_two_loop(p, gram.data(), n, idx.data(), delta.data(), alpha.data());
    double again = 0;
    for (int k = 0; k < dim; ++k) {
      double d = 0;
      for (int j = 0; j < n; ++j) d += delta[j] * b[j][k];
      again += d * b[2 * p][k];
    }
    bad += !(slope < 0.0) || !std::isfinite(slope) || std::fabs(again - slope) > 1e-10 * std::fabs(slope);
  }
  printf("lbfgs         0 .. %d pairs: the slopes are negative and those of the combined vectors\n", calk::kLbfgsMaxHistory);
  if (bad) fprintf(stderr, "lbfgs_two_loop: %d inconsistent directions\n", bad);
  return bad ? 1 : 0;
}

std::vector<int> cycle(int n, int m) {
  std::vector<int> v(n);
  for (int i = 0; i < n; ++i) v[i] = i % m;
  return v;
}

}  // namespace

int main() {
  std::vector<Case> cases;
  // folded STREAM: 45 single-baseline groups, tile widths from 128 down to 16, the widest block cut into several items
  cases.push_back({"fold", 10, 256, 1, CAL_LAYOUT_STREAM, CAL_PATH_AUTO, {12, 60, 120, 200, 230}, {1, 1, 1, 1, 1}, cycle(45, 5), std::vector<int>(45, 1), {}, {}});
  // heads: 3 slices of 70 single-baseline groups that share tiles; 66 heads for the matrix-core kernel, the 230-vector blocks beside it
  {
    Case c{"alias", 39, 256, 3, CAL_LAYOUT_STREAM, CAL_PATH_AUTO, {8, 33, 100, 224, 230}, {1, 1, 1, 1, 1}, {}, std::vector<int>(210, 1), {}, {}};
    for (int t = 0; t < 3; ++t)
      for (int g = 0; g < 70; ++g) {
        c.grp_basis.push_back(g < 66 ? g % 4 : 4);
        c.alias.push_back(t == 0 ? -1 : g);
      }
    cases.push_back(c);
  }
  // forced dense (fp32: split-bf16 operands; fp64: the fp64 matrix-core kernel), 2 slices, odd baseline counts per block
  cases.push_back({"dense", 26, 256, 2, CAL_LAYOUT_SHARED, CAL_PATH_DENSE, {20, 45, 77, 130, 200}, {1, 1, 1, 1, 1}, cycle(150, 5), std::vector<int>(150, 1), {}, {}});
  // multi-baseline groups over two row blocks, one run longer than kRunMax
  {
    Case c{"runs", 30, 96, 1, CAL_LAYOUT_STREAM, CAL_PATH_AUTO, {5, 12, 30, 7, 9}, {2, 2, 2, 2, 2}, {0, 1, 2, 3, 4}, {1, 3, 20, 70, 300}, {}, {}};
    for (int g = 0; g < 5; ++g)
      for (int b = 0; b < c.grp_nbl[g]; ++b) c.rowblk.push_back(g == 4 ? (b < 290 ? 0 : 1) : (b / 3) % 2);
    cases.push_back(c);
  }
  int bad = 0;
  for (const Case& c : cases) bad += run<float>(c) + run<double>(c);
  bad += walk_step_shapes();
  bad += walk_lbfgs();
  return bad ? 1 : 0;
}
