// report_plan.hpp -- what the post-fit reports cal_solver_delay_spectrum, cal_solver_delay_cross_spectrum, cal_solver_delay_fringe_spectrum,
// cal_solver_delay_coherent_spectrum, cal_solver_delay_transfer and cal_solver_fix_degeneracies decide
// before they launch, on the host alone: the rows of every bin and of every slice, how they are cut into chunks and segments, and the padded images the kernels read.
// No HIP or RCCL runtime call and no solver: SolverT uploads these plans at every call; cal_debug_report_plan returns them as bytes
// (tests/test_report_plan_host.py).  dspec_bin_kernel adds a bin's rows, and degen_sum_kernel a slice's segments, in the order written
// here, in double and without atomics: ascending rows, cut where the loops below cut them.  That order is what "two calls give the same
// bits, a slice of a batch the bits of the same slice alone" rests on, so it is part of the plan.
#pragma once
#include "problem_plan.hpp"
#include "solve_plan.hpp"
#include "delay_spectrum_kernels.hpp"
#include "delay_cross_kernels.hpp"
#include "delay_fringe_kernels.hpp"
#include "delay_coherent_kernels.hpp"
#include "delay_transfer_kernels.hpp"
#include "degeneracy_kernels.hpp"

namespace {

// ---- cal_solver_delay_spectrum ----------------------------------------------------------------------------------------------------
template <typename T>
struct DelaySpectrumPlan {
  int nq = 0;                  // quantities asked for: the bits of `what`
  int xpitch = 0, ndpad = 0;   // row pitch of the masked planes, columns of the operator image
  int crows = 0, nchunks = 0;  // rows per chunk (the last may hold fewer)
  std::vector<int> bin_ent;    // the sorted row list of every bin, one after the other (CSR, like ant_ent)
  std::vector<int> chunk_ptr;  // [nchunks][nbins][2]: a bin's piece of a chunk as positions in bin_ent
  std::vector<T> image;        // [re, im][xpitch][ndpad]: the operator, zero beyond nfreqs and ndelays
  std::vector<double> norm_f;  // [xpitch], zero beyond nfreqs
  size_t n_x = 0, n_pow = 0, n_out = 0;  // elements of ds_x (T), of ds_pow (double; 0 without power) and of ds_out (norm_bl | power_bin | count_bin)
};

// The sorted row list of every bin, one after the other (CSR: bin n's rows are bin_ent[bin_ptr[n] .. bin_ptr[n + 1])), ascending in b.
inline int plan_bin_lists(const char* who, int nbls, int nbins, const int32_t* bin_of_bl, std::vector<int>& bin_ptr, std::vector<int>& bin_ent) {
  bin_ptr.assign(nbins + 1, 0);
  for (int b = 0; b < nbls && nbins; ++b) {
    const int n = bin_of_bl[b];
    if (n < -1 || n >= nbins) return fail(CAL_ERR_INVALID, "%s: bin_of_bl[%d] = %d lies outside [-1, %d)", who, b, n, nbins);
    if (n >= 0) ++bin_ptr[n + 1];
  }
  if (nbins) {
    for (int n = 0; n < nbins; ++n) bin_ptr[n + 1] += bin_ptr[n];
    bin_ent.resize(bin_ptr[nbins]);
    std::vector<int> fill(bin_ptr.begin(), bin_ptr.end() - 1);
    for (int b = 0; b < nbls; ++b)
      if (bin_of_bl[b] >= 0) bin_ent[fill[bin_of_bl[b]]++] = b;
  }
  return CAL_OK;
}
// The operator as the kernels read it: [re, im][xpitch][ndpad], zero beyond nfreqs and nd.
template <typename T>
void plan_operator_image(int nfreqs, int nd, int xpitch, int ndpad, const void* op_r, const void* op_i, std::vector<T>& image) {
  image.assign((size_t)2 * xpitch * ndpad, (T)0);
  for (int part = 0; part < 2; ++part) {
    const T* src = static_cast<const T*>(part ? op_i : op_r);
    for (int f = 0; f < nfreqs; ++f) std::copy(src + (size_t)f * nd, src + (size_t)(f + 1) * nd, image.begin() + ((size_t)part * xpitch + f) * ndpad);
  }
}

// A chunk's scratch -- the masked planes in T and, with_power, its power in double -- stays under `bound` bytes (never less than one row);
// the chunks are cut at multiples of the transform's kDsRows where that fits.  d: ndelays, what, nbins, bin_of_bl, op_r, op_i, norm_f.
template <typename T>
int plan_delay_spectrum(int nbls, int nfreqs, int fpad, const cal_delay_spectrum_desc* d, int64_t bound, bool with_power, DelaySpectrumPlan<T>& P) {
  const int nd = d->ndelays, nbins = d->nbins;
  P.nq = (d->what & 1) + (d->what >> 1 & 1) + (d->what >> 2 & 1);
  if ((long long)P.nq * nbins * nd + nbins > (1ll << 31) - 1) return fail(CAL_ERR_INVALID, "delay_spectrum: nbins = %d is too many", nbins);
  std::vector<int> bin_ptr;
  CAL_TRY(plan_bin_lists("delay_spectrum", nbls, nbins, d->bin_of_bl, bin_ptr, P.bin_ent));
  P.xpitch = ds_xpitch(fpad);
  P.ndpad = ds_ndpad(nd);
  const size_t row_bytes = (size_t)P.nq * 2 * P.xpitch * sizeof(T) + (with_power ? (size_t)P.nq * nd * sizeof(double) : 0);
  long long crows = std::max<long long>(1, bound / (long long)row_bytes);
  if (crows > kDsRows) crows -= crows % kDsRows;
  crows = std::min<long long>(crows, nbls);
  P.crows = (int)crows;
  P.nchunks = (int)((nbls + crows - 1) / crows);
  P.chunk_ptr.resize((size_t)P.nchunks * nbins * 2);
  for (int c = 0; c < P.nchunks && nbins; ++c) {
    const long long b0 = c * crows, b1 = std::min<long long>(nbls, b0 + crows);
    for (int n = 0; n < nbins; ++n) {
      const int* e0 = P.bin_ent.data() + bin_ptr[n];
      const int* e1 = P.bin_ent.data() + bin_ptr[n + 1];
      P.chunk_ptr[((size_t)c * nbins + n) * 2] = (int)(std::lower_bound(e0, e1, (int)b0) - P.bin_ent.data());
      P.chunk_ptr[((size_t)c * nbins + n) * 2 + 1] = (int)(std::lower_bound(e0, e1, (int)b1) - P.bin_ent.data());
    }
  }
  plan_operator_image<T>(nfreqs, nd, P.xpitch, P.ndpad, d->op_r, d->op_i, P.image);
  P.norm_f.assign((size_t)P.xpitch, 0.0);
  std::copy(d->norm_f, d->norm_f + nfreqs, P.norm_f.begin());
  P.n_x = (size_t)P.nq * 2 * crows * P.xpitch;
  P.n_pow = with_power ? (size_t)P.nq * crows * nd : 0;
  P.n_out = (size_t)nbls + (size_t)P.nq * nbins * nd + nbins;
  return CAL_OK;
}

// ---- cal_solver_delay_cross_spectrum -----------------------------------------------------------------------------------------------
template <typename T>
struct DelayCrossPlan {
  int nq = 0, nstat = 0;        // quantities and statistics asked for: the bits of `what` and of `stats`
  int xpitch = 0, ndpad = 0;    // row pitch of the masked planes, columns of the operator image
  int cpairs = 0, nchunks = 0;  // pairs per chunk (the last may hold fewer)
  std::vector<int> bin_ent;     // the sorted pair list of every bin, one after the other (plan_bin_lists)
  std::vector<int> chunk_ptr;   // [nchunks][nbins][2]: a bin's piece of a chunk as positions in bin_ent
  std::vector<T> image;         // [re, im][xpitch][ndpad]: the operator, zero beyond nfreqs and ndelays
  std::vector<double> norm_f;   // [xpitch], zero beyond nfreqs
  std::vector<double> scale;    // [npairs][2]: the description's, or ones
  size_t n_x = 0, n_pow = 0, n_out = 0;  // elements of ds_x (T), of ds_pow (double) and of ds_out (norm_pair | cross_bin | diff_bin | count_bin)
};

// A chunk of pairs' scratch -- the masked planes of both sides in T and its nstat statistics in double -- stays under `bound` bytes (never
// less than one pair); the chunks are cut at multiples of the transform's kDcPairs where that fits.  Everything of the description that
// can be refused on the host is refused here: npairs, the rows of the pairs, stats, the scales, the bins.
template <typename T>
int plan_delay_cross(int nbls, int nfreqs, int fpad, const cal_delay_cross_desc* d, int64_t bound, DelayCrossPlan<T>& P) {
  const int nd = d->ndelays, nbins = d->nbins, np = d->npairs;
  if (np < 1) return fail(CAL_ERR_INVALID, "delay_cross_spectrum: npairs = %d (at least 1)", np);
  if (!d->pairs) return fail(CAL_ERR_INVALID, "delay_cross_spectrum: null pairs");
  if ((d->stats & 3) == 0 || (d->stats & ~3)) return fail(CAL_ERR_INVALID, "delay_cross_spectrum: stats = %d: bits 0 (cross), 1 (diff), at least one", d->stats);
  for (int p = 0; p < np; ++p)
    for (int s = 0; s < 2; ++s) {
      const int b = d->pairs[2 * (size_t)p + s];
      if (b < 0 || b >= nbls) return fail(CAL_ERR_INVALID, "delay_cross_spectrum: pairs[%d][%d] = %d lies outside [0, %d)", p, s, b, nbls);
    }
  P.scale.assign(2 * (size_t)np, 1.0);
  if (d->scale) {
    for (size_t k = 0; k < 2 * (size_t)np; ++k)
      if (!std::isfinite(d->scale[k])) return fail(CAL_ERR_INVALID, "delay_cross_spectrum: scale[%d][%d] is not finite", (int)(k / 2), (int)(k % 2));
    std::copy(d->scale, d->scale + 2 * (size_t)np, P.scale.begin());
  }
  P.nq = (d->what & 1) + (d->what >> 1 & 1) + (d->what >> 2 & 1);
  P.nstat = (d->stats & 1) + (d->stats >> 1 & 1);
  if ((long long)P.nstat * P.nq * nbins * nd + nbins > (1ll << 31) - 1) return fail(CAL_ERR_INVALID, "delay_cross_spectrum: nbins = %d is too many", nbins);
  for (int p = 0; p < np && nbins; ++p)
    if (d->bin_of_pair[p] < -1 || d->bin_of_pair[p] >= nbins)
      return fail(CAL_ERR_INVALID, "delay_cross_spectrum: bin_of_pair[%d] = %d lies outside [-1, %d)", p, d->bin_of_pair[p], nbins);
  std::vector<int> bin_ptr;
  CAL_TRY(plan_bin_lists("delay_cross_spectrum", np, nbins, d->bin_of_pair, bin_ptr, P.bin_ent));
  P.xpitch = ds_xpitch(fpad);
  P.ndpad = ds_ndpad(nd);
  const size_t pair_bytes = (size_t)P.nq * 2 * 2 * P.xpitch * sizeof(T) + (size_t)P.nstat * P.nq * nd * sizeof(double);
  long long cpairs = std::max<long long>(1, bound / (long long)pair_bytes);
  if (cpairs > kDcPairs) cpairs -= cpairs % kDcPairs;
  cpairs = std::min<long long>(cpairs, np);
  P.cpairs = (int)cpairs;
  P.nchunks = (int)((np + cpairs - 1) / cpairs);
  P.chunk_ptr.resize((size_t)P.nchunks * nbins * 2);
  for (int c = 0; c < P.nchunks && nbins; ++c) {
    const long long p0 = c * cpairs, p1 = std::min<long long>(np, p0 + cpairs);
    for (int n = 0; n < nbins; ++n) {
      const int* e0 = P.bin_ent.data() + bin_ptr[n];
      const int* e1 = P.bin_ent.data() + bin_ptr[n + 1];
      P.chunk_ptr[((size_t)c * nbins + n) * 2] = (int)(std::lower_bound(e0, e1, (int)p0) - P.bin_ent.data());
      P.chunk_ptr[((size_t)c * nbins + n) * 2 + 1] = (int)(std::lower_bound(e0, e1, (int)p1) - P.bin_ent.data());
    }
  }
  plan_operator_image<T>(nfreqs, nd, P.xpitch, P.ndpad, d->op_r, d->op_i, P.image);
  P.norm_f.assign((size_t)P.xpitch, 0.0);
  std::copy(d->norm_f, d->norm_f + nfreqs, P.norm_f.begin());
  P.n_x = (size_t)P.nq * 2 * 2 * cpairs * P.xpitch;
  P.n_pow = (size_t)P.nstat * P.nq * cpairs * nd;
  P.n_out = (size_t)np + (size_t)P.nstat * P.nq * nbins * nd + nbins;
  return CAL_OK;
}

// ---- cal_solver_delay_fringe_spectrum ----------------------------------------------------------------------------------------------
template <typename T>
struct DelayFringePlan {
  int nq = 0;                    // quantities asked for: the bits of `what`
  int xpitch = 0, ndpad = 0;     // row pitch of the masked planes, columns of the operator image
  int cgroups = 0, nchunks = 0;  // whole groups per chunk (the last may hold fewer)
  std::vector<int> bin_ent;      // the sorted group list of every bin, one after the other (plan_bin_lists)
  std::vector<int> chunk_ptr;    // [nchunks][nbins][2]: a bin's piece of a chunk as positions in bin_ent
  std::vector<T> image;          // [re, im][xpitch][ndpad]: the operator, zero beyond nfreqs and ndelays
  std::vector<double> norm_f;    // [xpitch], zero beyond nfreqs
  std::vector<double> scale;     // [ngroups][ntimes]: the description's, or ones
  std::vector<double> opt;       // opt_r | opt_i, [ntimes][nrates] each
  size_t n_x = 0, n_y = 0, n_pow = 0, n_out = 0;  // elements of ds_x (T), of Y and of the power (both in ds_pow, double) and of ds_out
                                                  // (norm_grp | power_bin | count_bin)
};

// A chunk of whole groups' scratch -- per group nq 2 T xpitch elements of T for the masked planes, nq 2 T ndelays doubles of Y and
// nq nrates ndelays doubles of power -- stays under `bound` bytes (never less than one group).  Everything of the description that can
// be refused on the host is refused here: ngroups, ntimes, nrates, the rows, the scales, opt, the bins.
// plan_fringe_core is the rule itself, shared with plan_delay_coherent below: `rows(0)` refuses what stands in for the rows when it is
// null, `rows(1)` its contents, at the places the fringe call has always refused them; `extra` bytes per group are added to the scratch.
template <typename T, typename Rows>
int plan_fringe_core(const char* who, int nfreqs, int fpad, const cal_delay_fringe_desc* d, Rows rows, size_t extra, int64_t bound, DelayFringePlan<T>& P) {
  const int nd = d->ndelays, nbins = d->nbins, ng = d->ngroups, nt = d->ntimes, nr = d->nrates;
  if (ng < 1) return fail(CAL_ERR_INVALID, "%s: ngroups = %d (at least 1)", who, ng);
  if (nt < 1 || nt > 64) return fail(CAL_ERR_INVALID, "%s: ntimes = %d lies outside [1, 64]", who, nt);
  if (nr < 1 || nr > 64) return fail(CAL_ERR_INVALID, "%s: nrates = %d lies outside [1, 64]", who, nr);
  CAL_TRY(rows(0));
  if (!d->opt_r || !d->opt_i) return fail(CAL_ERR_INVALID, "%s: null opt", who);
  const size_t nrow = (size_t)ng * nt;
  if (nrow > (size_t)(1u << 30)) return fail(CAL_ERR_INVALID, "%s: ngroups ntimes = %lld is too many", who, (long long)nrow);
  CAL_TRY(rows(1));
  P.scale.assign(nrow, 1.0);
  if (d->scale) {
    for (size_t k = 0; k < nrow; ++k)
      if (!std::isfinite(d->scale[k])) return fail(CAL_ERR_INVALID, "%s: scale[%d][%d] is not finite", who, (int)(k / nt), (int)(k % nt));
    std::copy(d->scale, d->scale + nrow, P.scale.begin());
  }
  const size_t nopt = (size_t)nt * nr;
  for (size_t k = 0; k < nopt; ++k)
    if (!std::isfinite(d->opt_r[k]) || !std::isfinite(d->opt_i[k]))
      return fail(CAL_ERR_INVALID, "%s: opt[%d][%d] is not finite", who, (int)(k / nr), (int)(k % nr));
  P.opt.resize(2 * nopt);
  std::copy(d->opt_r, d->opt_r + nopt, P.opt.begin());
  std::copy(d->opt_i, d->opt_i + nopt, P.opt.begin() + nopt);
  P.nq = (d->what & 1) + (d->what >> 1 & 1) + (d->what >> 2 & 1);
  if ((long long)P.nq * nbins * nr * nd + nbins > (1ll << 31) - 1) return fail(CAL_ERR_INVALID, "%s: nbins = %d is too many", who, nbins);
  for (int g = 0; g < ng && nbins; ++g)
    if (d->bin_of_group[g] < -1 || d->bin_of_group[g] >= nbins)
      return fail(CAL_ERR_INVALID, "%s: bin_of_group[%d] = %d lies outside [-1, %d)", who, g, d->bin_of_group[g], nbins);
  std::vector<int> bin_ptr;
  CAL_TRY(plan_bin_lists(who, ng, nbins, d->bin_of_group, bin_ptr, P.bin_ent));
  P.xpitch = ds_xpitch(fpad);
  P.ndpad = ds_ndpad(nd);
  const size_t group_bytes = (size_t)P.nq * 2 * nt * P.xpitch * sizeof(T) + (size_t)P.nq * 2 * nt * nd * sizeof(double) + (size_t)P.nq * nr * nd * sizeof(double) + extra;
  long long cgroups = std::max<long long>(1, bound / (long long)group_bytes);
  cgroups = std::min<long long>(cgroups, ng);  // (ngroups ntimes fits an int: so do a chunk's rows)
  P.cgroups = (int)cgroups;
  P.nchunks = (int)((ng + cgroups - 1) / cgroups);
  P.chunk_ptr.resize((size_t)P.nchunks * nbins * 2);
  for (int c = 0; c < P.nchunks && nbins; ++c) {
    const long long g0 = c * cgroups, g1 = std::min<long long>(ng, g0 + cgroups);
    for (int n = 0; n < nbins; ++n) {
      const int* e0 = P.bin_ent.data() + bin_ptr[n];
      const int* e1 = P.bin_ent.data() + bin_ptr[n + 1];
      P.chunk_ptr[((size_t)c * nbins + n) * 2] = (int)(std::lower_bound(e0, e1, (int)g0) - P.bin_ent.data());
      P.chunk_ptr[((size_t)c * nbins + n) * 2 + 1] = (int)(std::lower_bound(e0, e1, (int)g1) - P.bin_ent.data());
    }
  }
  plan_operator_image<T>(nfreqs, nd, P.xpitch, P.ndpad, d->op_r, d->op_i, P.image);
  P.norm_f.assign((size_t)P.xpitch, 0.0);
  std::copy(d->norm_f, d->norm_f + nfreqs, P.norm_f.begin());
  P.n_x = (size_t)P.nq * 2 * cgroups * nt * P.xpitch;
  P.n_y = (size_t)P.nq * 2 * cgroups * nt * nd;
  P.n_pow = (size_t)P.nq * cgroups * nr * nd;
  P.n_out = (size_t)ng + (size_t)P.nq * nbins * nr * nd + nbins;
  return CAL_OK;
}

template <typename T>
int plan_delay_fringe(int nbls, int nfreqs, int fpad, const cal_delay_fringe_desc* d, int64_t bound, DelayFringePlan<T>& P) {
  const int nt = d->ntimes;
  const size_t nrow = (size_t)d->ngroups * nt;
  return plan_fringe_core<T>("delay_fringe_spectrum", nfreqs, fpad, d, [&](int contents) -> int {
    if (!contents) return d->rows ? (int)CAL_OK : fail(CAL_ERR_INVALID, "delay_fringe_spectrum: null rows");
    for (size_t k = 0; k < nrow; ++k)
      if (d->rows[k] < 0 || d->rows[k] >= nbls)
        return fail(CAL_ERR_INVALID, "delay_fringe_spectrum: rows[%d][%d] = %d lies outside [0, %d)", (int)(k / nt), (int)(k % nt), d->rows[k], nbls);
    return CAL_OK;
  }, 0, bound, P);
}

// ---- cal_solver_delay_coherent_spectrum --------------------------------------------------------------------------------------------
// The fringe plan over the averaged planes (F: the same chunks of whole groups, bins, images, scales and opt), the member lists as they
// are uploaded once per call, and every chunk's range of members.
template <typename T>
struct DelayCoherentPlan {
  DelayFringePlan<T> F;
  std::vector<long long> set_ptr;       // [ngroups ntimes + 1]
  std::vector<int> member_row;          // [nmembers]
  std::vector<double> member_wgt;       // [nmembers]: the description's, or ones
  std::vector<unsigned char> member_conj;  // [nmembers]: the description's, or zeros
  std::vector<int64_t> chunk_members;   // [nchunks][2]: the chunk's members as positions in the member arrays
  int nspans = 0;                       // spans of 64 V channels of a row of the averaged planes
  size_t n_mask = 0;                    // bytes of a chunk's set masks
};

// plan_fringe_core with the sets in the place of the rows, and a group's set masks (ntimes pitch bytes) counted into its scratch.
// Refused here as well: a set_ptr that does not start at 0, falls, or does not end at nmembers; a member row outside [0, nbls); a
// coefficient that is negative or not finite; a member_conj other than 0 or 1; a weighting other than 0 or 1; nmembers above 2^30.
template <typename T>
int plan_delay_coherent(int nbls, int nfreqs, int fpad, const cal_delay_coherent_desc* d, int64_t bound, DelayCoherentPlan<T>& P) {
  const char* who = "delay_coherent_spectrum";
  const cal_delay_fringe_desc fd{d->ndelays, d->what, d->calibrated, d->ngroups, d->ntimes, d->nrates, nullptr, d->scale, d->nbins, d->bin_of_group,
                                 d->op_r, d->op_i, d->norm_f, d->opt_r, d->opt_i};
  const int nt = d->ntimes;
  const int64_t nm = d->nmembers;
  const size_t nsets = (size_t)std::max(d->ngroups, 0) * (size_t)std::max(nt, 0);
  const size_t mask_bytes = (size_t)std::max(nt, 0) * ds_xpitch(fpad);
  CAL_TRY(plan_fringe_core<T>(who, nfreqs, fpad, &fd, [&](int contents) -> int {
    if (!contents) {
      if (d->weighting != 0 && d->weighting != 1) return fail(CAL_ERR_INVALID, "%s: weighting = %d (0: the coefficients, 1: coefficients times weights)", who, d->weighting);
      if (nm < 0 || nm > (int64_t)1 << 30) return fail(CAL_ERR_INVALID, "%s: nmembers = %lld lies outside [0, 2^30]", who, (long long)nm);
      if (!d->set_ptr) return fail(CAL_ERR_INVALID, "%s: null set_ptr", who);
      if (nm > 0 && !d->member_row) return fail(CAL_ERR_INVALID, "%s: null member_row", who);
      return CAL_OK;
    }
    if (d->set_ptr[0] != 0) return fail(CAL_ERR_INVALID, "%s: set_ptr[0] = %lld (it starts at 0)", who, (long long)d->set_ptr[0]);
    for (size_t v = 0; v < nsets; ++v)
      if (d->set_ptr[v + 1] < d->set_ptr[v])
        return fail(CAL_ERR_INVALID, "%s: set_ptr[%lld] = %lld falls below set_ptr[%lld] = %lld", who, (long long)v + 1, (long long)d->set_ptr[v + 1], (long long)v,
                    (long long)d->set_ptr[v]);
    if (d->set_ptr[nsets] != nm)
      return fail(CAL_ERR_INVALID, "%s: set_ptr ends at %lld, not at nmembers = %lld", who, (long long)d->set_ptr[nsets], (long long)nm);
    for (int64_t k = 0; k < nm; ++k) {
      if (d->member_row[k] < 0 || d->member_row[k] >= nbls)
        return fail(CAL_ERR_INVALID, "%s: member_row[%lld] = %d lies outside [0, %d)", who, (long long)k, d->member_row[k], nbls);
      if (d->member_wgt && !(std::isfinite(d->member_wgt[k]) && d->member_wgt[k] >= 0.0))
        return fail(CAL_ERR_INVALID, "%s: member_wgt[%lld] is negative or not finite", who, (long long)k);
      if (d->member_conj && d->member_conj[k] > 1) return fail(CAL_ERR_INVALID, "%s: member_conj[%lld] = %d (0 or 1)", who, (long long)k, (int)d->member_conj[k]);
    }
    return CAL_OK;
  }, mask_bytes, bound, P.F));
  P.set_ptr.assign(d->set_ptr, d->set_ptr + nsets + 1);
  P.member_row.assign(d->member_row, d->member_row + nm);
  P.member_wgt.assign((size_t)nm, 1.0);
  if (d->member_wgt) std::copy(d->member_wgt, d->member_wgt + nm, P.member_wgt.begin());
  P.member_conj.assign((size_t)nm, 0);
  if (d->member_conj) std::copy(d->member_conj, d->member_conj + nm, P.member_conj.begin());
  P.chunk_members.resize((size_t)P.F.nchunks * 2);
  for (int c = 0; c < P.F.nchunks; ++c) {
    const long long g0 = (long long)c * P.F.cgroups, g1 = std::min<long long>(d->ngroups, g0 + P.F.cgroups);
    P.chunk_members[2 * c] = P.set_ptr[(size_t)g0 * nt];
    P.chunk_members[2 * c + 1] = P.set_ptr[(size_t)g1 * nt];
  }
  constexpr int V = 16 / (int)sizeof(T);
  P.nspans = (P.F.xpitch + 64 * V - 1) / (64 * V);
  P.n_mask = (size_t)P.F.cgroups * mask_bytes;
  return CAL_OK;
}

// ---- cal_solver_delay_transfer -----------------------------------------------------------------------------------------------------
// positions of a chunk of groups in order / work (plan_group_chunks' chunk), in runs and in rows; dynamic LDS of its factor launch
struct TransferChunk { int g0, g1, w0, w1, r0, r1, q0, q1; long long lds; };
template <typename T>
struct DelayTransferPlan {
  int xpitch = 0, ndpad = 0, npieces = 0;
  std::vector<CsGroup> grp;         // the groups with this plan's offsets
  GroupPlan G;                      // order, Gram work, xoff (a group's W, then S of its runs, in the chunk's third scratch)
  std::vector<DtRun> runs;          // chunk by chunk: every run of a group's baselines on one row block
  std::vector<DtRow> rows;          // chunk by chunk: the rows of its groups
  std::vector<TransferChunk> chunks;
  std::vector<int> bin_ent;         // the sorted row list of every bin (plan_bin_lists)
  std::vector<int> bin_ptr2;        // [nbins][2]: a bin's list as positions in bin_ent (what dspec_bin_kernel reads for ONE chunk of all rows)
  std::vector<T> image;             // [re, im][xpitch][ndpad]
  size_t n_rows_out = 0;            // elements of absorbed (and of noise): nbls ndelays doubles
  size_t n_out = 0;                 // valid | absorbed_bin | count_bin
};

// The groups are cut into chunks by plan_group_chunks' rule: N, W and S (T) and the factor (double) of a chunk stay under `bound` bytes,
// never less than one group.  S of a run is [fe_pad(nvec)][xpitch].  The rows of absorbed and noise are kept whole ([nbls][ndelays]
// doubles, outside the bound): the bins add their rows in ascending order, which is not the order of the chunks (heaviest group first).
template <typename T>
int plan_delay_transfer(const std::vector<CsGroup>& cs_grp, const std::vector<long long>& bl_tile, int nbls, int nfreqs, int fpad, bool fold,
                        const cal_delay_transfer_desc* d, int64_t bound, DelayTransferPlan<T>& P) {
  const int nd = d->ndelays, nbins = d->nbins;
  if ((long long)nbins * nd + nbins > (1ll << 31) - 1) return fail(CAL_ERR_INVALID, "delay_transfer: nbins = %d is too many", nbins);
  std::vector<int> bin_ptr;
  CAL_TRY(plan_bin_lists("delay_transfer", nbls, nbins, d->bin_of_bl, bin_ptr, P.bin_ent));
  P.bin_ptr2.resize((size_t)nbins * 2);
  for (int n = 0; n < nbins; ++n) P.bin_ptr2[2 * (size_t)n] = bin_ptr[n], P.bin_ptr2[2 * (size_t)n + 1] = bin_ptr[n + 1];
  P.xpitch = ds_xpitch(fpad);
  P.ndpad = ds_ndpad(nd);
  P.npieces = ((fold ? nfreqs / 2 : fpad) + kFePiece - 1) / kFePiece;
  P.grp = cs_grp;
  const int ngrps = (int)P.grp.size();
  auto runs_of = [&](const CsGroup& g, auto fn) {
    for (int b = g.b0; b < g.b1;) {
      int e = b + 1;
      while (e < g.b1 && bl_tile[e] == bl_tile[b]) ++e;
      fn(b, e);
      b = e;
    }
  };
  std::vector<long long> extra(ngrps);
  for (int gi = 0; gi < ngrps; ++gi) {
    const long long np = fe_pad(P.grp[gi].nvec);
    long long nruns = 0;
    runs_of(P.grp[gi], [&](int, int) { ++nruns; });
    extra[gi] = np * np + nruns * np * P.xpitch;
  }
  P.G = plan_group_chunks(P.grp, sizeof(T), bound, extra);
  for (const GroupChunk& ch : P.G.chunks) {
    TransferChunk tc{ch.g0, ch.g1, ch.w0, ch.w1, (int)P.runs.size(), 0, (int)P.rows.size(), 0, (long long)ch.lds};
    for (int p = ch.g0; p < ch.g1; ++p) {
      const int gi = P.G.order[p];
      const CsGroup& g = P.grp[gi];
      const long long np = fe_pad(g.nvec);
      long long soff = P.G.xoff[gi] + np * np;
      runs_of(g, [&](int b, int e) {
        P.runs.push_back(DtRun{soff, gi, b, e, 0});
        for (int bb = b; bb < e; ++bb) P.rows.push_back(DtRow{soff, bb, gi});
        soff += np * P.xpitch;
      });
    }
    tc.r1 = (int)P.runs.size();
    tc.q1 = (int)P.rows.size();
    P.chunks.push_back(tc);
  }
  plan_operator_image<T>(nfreqs, nd, P.xpitch, P.ndpad, d->op_r, d->op_i, P.image);
  P.n_rows_out = (size_t)nbls * nd;
  P.n_out = (size_t)nbls + (size_t)nbins * nd + nbins;
  return CAL_OK;
}

// ---- cal_solver_fix_degeneracies --------------------------------------------------------------------------------------------------
struct DegeneracyPlan {
  std::vector<double> d_b;    // [nbls][2]: r_i - r_j of a row's own antennas
  std::vector<double> pos;    // [na][2]: one slice's antenna positions
  std::vector<double> ratio;  // [fpad]: nu_f / nu_ref (band mode) or 1, zero beyond nfreqs
  std::vector<double> maxd;   // [nsl]: the slice's longest |d_b|
  std::vector<int> ent;       // the row list of every slice, one after the other, each ascending
  std::vector<int> segptr;    // [nsl + 1]: a slice's first segment
  std::vector<DgSeg> segs;    // every kDgSeg rows of a slice's list
  int nseg = 0;
  // The two blobs the kernels read, dg_geo (doubles) and dg_idx (ints): where every array starts, and the arrays packed in that order.
  size_t geo_pos() const { return d_b.size(); }
  size_t geo_ratio() const { return geo_pos() + pos.size(); }
  size_t geo_maxd() const { return geo_ratio() + ratio.size(); }
  size_t idx_segptr() const { return ent.size(); }
  size_t idx_segs() const { return idx_segptr() + segptr.size(); }
  std::vector<double> pack_geo() const {
    std::vector<double> v(d_b);
    for (const std::vector<double>* a : {&pos, &ratio, &maxd}) v.insert(v.end(), a->begin(), a->end());
    return v;
  }
  std::vector<int> pack_idx() const {
    static_assert(sizeof(DgSeg) == 4 * sizeof(int), "a segment is four ints of dg_idx");
    std::vector<int> v(ent);
    v.insert(v.end(), segptr.begin(), segptr.end());
    const int* s = reinterpret_cast<const int*>(segs.data());
    v.insert(v.end(), s, s + 4 * segs.size());
    return v;
  }
};

// bl_ant: the plan's rows; nsl slices of na = nants / nsl antennas each (joint time-basis layout: antenna row t na + a is slice t, antenna a);
// band: Phi(f) = (nu_f / nu_ref) Phi_0 with nu_ref the mean of freqs (read only then); antpos [na][2].
inline int plan_degeneracies(const std::vector<int2>& bl_ant, int nants, int nsl, int nfreqs, int fpad, bool band, const double* antpos,
                             const double* freqs, DegeneracyPlan& P) {
  const int nbls = (int)bl_ant.size(), na = nants / nsl;
  for (int k = 0; k < 2 * na; ++k)
    if (!std::isfinite(antpos[k])) return fail(CAL_ERR_INVALID, "fix_degeneracies: antenna position %d is not finite", k / 2);
  P.pos.assign(antpos, antpos + 2 * (size_t)na);
  P.ratio.assign((size_t)fpad, 0.0);
  std::fill(P.ratio.begin(), P.ratio.begin() + nfreqs, 1.0);
  if (band) {
    double mean = 0.0;
    for (int f = 0; f < nfreqs; ++f) mean += freqs[f];
    mean /= nfreqs;
    if (!std::isfinite(mean) || mean == 0.0) return fail(CAL_ERR_INVALID, "fix_degeneracies: the mean of freqs must be finite and not zero");
    for (int f = 0; f < nfreqs; ++f) P.ratio[f] = freqs[f] / mean;
  }
  P.d_b.assign(2 * (size_t)nbls, 0.0);
  P.maxd.assign((size_t)nsl, 0.0);
  std::vector<int> cnt(nsl + 1, 0);
  for (int b = 0; b < nbls; ++b) {
    const int2 a = bl_ant[b];
    const int t = a.x / na;
    if (a.y / na != t) return fail(CAL_ERR_INVALID, "fix_degeneracies: baseline row %d joins antennas of two slices (%d, %d; %d antennas per slice)", b, a.x, a.y, na);
    ++cnt[t + 1];
    const int i = a.x % na, j = a.y % na;
    const double de = P.pos[2 * i] - P.pos[2 * j], dn = P.pos[2 * i + 1] - P.pos[2 * j + 1];
    P.d_b[2 * (size_t)b] = de;
    P.d_b[2 * (size_t)b + 1] = dn;
    P.maxd[t] = std::max(P.maxd[t], std::sqrt(de * de + dn * dn));
  }
  for (int t = 0; t < nsl; ++t) cnt[t + 1] += cnt[t];
  P.ent.resize(nbls);
  std::vector<int> fill(cnt.begin(), cnt.end() - 1);
  for (int b = 0; b < nbls; ++b) P.ent[fill[bl_ant[b].x / na]++] = b;
  P.segptr.resize(nsl + 1);
  for (int t = 0; t < nsl; ++t) {
    P.segptr[t] = (int)P.segs.size();
    for (int e = cnt[t]; e < cnt[t + 1]; e += kDgSeg) P.segs.push_back(DgSeg{t, e, std::min(e + kDgSeg, cnt[t + 1]), 0});
  }
  P.segptr[nsl] = P.nseg = (int)P.segs.size();
  return CAL_OK;
}

}  // namespace
