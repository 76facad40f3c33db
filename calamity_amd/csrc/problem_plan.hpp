// problem_plan.hpp -- everything set_problem decides about a problem, on the host alone: plan_problem() turns a cal_problem_desc into a
// ProblemPlan<T>.  No HIP or RCCL runtime call and no solver: the kernel headers are included for their constants, record types and
// LDS-size functions.  SolverT::set_problem_local uploads the plan; cal_debug_plan returns it as bytes (tests/test_plan_host.py).
// Item and panel order decide the order of floating-point partial sums: every stable sort, map walk and first minimum is part of the result.
#pragma once
#include "../../include/calamity_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <map>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

#include "fit_kernels.hpp"
#include "dense_kernels.hpp"
#include "split_kernels.hpp"
#include "split2_kernels.hpp"
#include "dense64_kernels.hpp"
#include "multi_mfma_kernels.hpp"
#include "coeff_solve_kernels.hpp"

namespace {

using namespace calk;

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
#define CAL_TRY(expr)      \
  do {                     \
    int _r = (expr);       \
    if (_r != CAL_OK) return _r; \
  } while (0)

// Mirror symmetry of one basis block, row-major [nfreqs][nvec]: A[F-1-f][k] = (-1)^k A[f][k] (discrete prolate spheroidal
// sequences centred on zero delay alternate between symmetric and antisymmetric vectors).  Host only.  Returns false for a block
// with a non-finite element; otherwise the largest |A[F-1-f][k] - (-1)^k A[f][k]| and the largest |A|.
template <typename T>
bool mirror_residual(const T* a, int nfreqs, int nvec, double* resid, double* amax) {
  double r = 0, m = 0;
  for (long long i = 0; i < (long long)nfreqs * nvec; ++i) {
    const double x = std::fabs((double)a[i]);
    if (!std::isfinite(x)) return false;
    m = std::max(m, x);
  }
  for (int f = 0; f < nfreqs / 2; ++f) {
    const T* lo = a + (long long)f * nvec;
    const T* hi = a + (long long)(nfreqs - 1 - f) * nvec;
    for (int k = 0; k < nvec; ++k) r = std::max(r, std::fabs((double)hi[k] - ((k & 1) ? -(double)lo[k] : (double)lo[k])));
  }
  *resid = r;
  *amax = m;
  return true;
}
// The streaming kernel may read channels [0, F/2) of such a block alone (fit_kernels.hpp: process_item, FOLD) when the mirror
// half carries no information of its own: in fp32 when no element differs from its mirror partner by more than half a unit in
// the last place of the block's largest element -- what the cast of an fp64 basis to fp32 leaves behind -- and in fp64 when the
// halves agree exactly.  fb: the block's tile width; the band's half must consist of whole tiles.
template <typename T>
bool block_foldable(const T* a, int nfreqs, int nvec, int nrowblk, int fb, double* resid, double* amax) {
  *resid = *amax = 0;
  if (nrowblk != 1 || nfreqs < 2 || (nfreqs & 1) || fb <= 0 || (nfreqs / 2) % fb != 0) return false;
  if (!mirror_residual(a, nfreqs, nvec, resid, amax)) return false;
  if (sizeof(T) == 4) return *resid <= 0.5 * 1.1920928955078125e-07 * *amax;
  return *resid == 0.0;
}

template <typename T>
int choose_fb(int nvec, int nfreqs) {
  // widest channel block whose tile (nvec x FB) still fits the staging budget; never wider than the band needs
  int cap = FbSet<T>::fb_min;
  while (cap < FbSet<T>::fb_max && cap < nfreqs) cap *= 2;
  for (int fb = std::min(cap, FbSet<T>::fb_max); fb >= FbSet<T>::fb_min; fb /= 2)
    if ((long long)nvec * fb * (long long)sizeof(T) <= kTileBytes) return fb;
  return -1;
}
// f(std::integral_constant<int, FB>) for the tile width fb, one of the five the general kernels are instantiated for
template <typename T, typename F>
auto with_fb(int fb, F&& f) {
  constexpr int M = FbSet<T>::fb_max;
  if (fb == M) return f(std::integral_constant<int, M>{});
  if (fb == M / 2) return f(std::integral_constant<int, M / 2>{});
  if (fb == M / 4) return f(std::integral_constant<int, M / 4>{});
  if (fb == M / 8) return f(std::integral_constant<int, M / 8>{});
  return f(std::integral_constant<int, M / 16>{});
}

// The loss partials of every time slice: entries ptr[t] .. ptr[t + 1] of idx are the records (items or panels) of slice t, in record order.
template <typename R>
void slice_partial_index(const std::vector<R>& records, int nslices, std::vector<int>& ptr, std::vector<int>& idx) {
  ptr.assign(nslices + 1, 0);
  idx.assign(records.size(), 0);
  for (const R& r : records) ptr[r.slice + 1]++;
  for (int t = 0; t < nslices; ++t) ptr[t + 1] += ptr[t];
  std::vector<int> fill(ptr.begin(), ptr.end() - 1);
  for (size_t q = 0; q < records.size(); ++q) idx[fill[records[q].slice]++] = (int)q;
}

// XCD-affine dispatch: workgroups are dealt round-robin over the 8 XCDs (b and b + 8 share one), so workgroup b takes entry b / 8 of
// list b % 8.  Entry i (cost[i]) belongs to group[i] (0 .. ngroups - 1); a whole group goes to ONE of the 8 lists, groups dealt
// longest-processing-time first (heaviest group first, each to the list with the least load so far -- the first such list) so the lists
// carry equal cost.  together: a list holds its groups one after the other, each in entry order; otherwise its entries heaviest first.
// Returns the interleaved slot map: entry indices, -1 where a list is shorter than the longest.
inline std::vector<int> deal_over_xcds(const std::vector<int>& group, int ngroups, const std::vector<double>& cost, bool together) {
  const int n = (int)group.size();
  std::vector<double> gcost(ngroups, 0.0);
  std::vector<std::vector<int>> of_group(ngroups);
  for (int i = 0; i < n; ++i) {
    gcost[group[i]] += cost[i];
    of_group[group[i]].push_back(i);
  }
  std::vector<int> border(ngroups);
  std::iota(border.begin(), border.end(), 0);
  std::stable_sort(border.begin(), border.end(), [&](int a, int b) { return gcost[a] > gcost[b]; });
  double load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<int> list_of(ngroups);
  std::vector<std::vector<int>> lists(8);
  for (int k : border) {
    const int x = (int)(std::min_element(load, load + 8) - load);
    list_of[k] = x;
    load[x] += gcost[k];
    if (together) lists[x].insert(lists[x].end(), of_group[k].begin(), of_group[k].end());
  }
  if (!together)
    for (int i = 0; i < n; ++i) lists[list_of[group[i]]].push_back(i);
  size_t longest = 0;
  for (auto& l : lists) {
    if (!together) std::stable_sort(l.begin(), l.end(), [&](int a, int b) { return cost[a] > cost[b]; });
    longest = std::max(longest, l.size());
  }
  std::vector<int> slots(8 * longest, -1);
  for (int x = 0; x < 8; ++x)
    for (size_t j = 0; j < lists[x].size(); ++j) slots[j * 8 + x] = lists[x][j];
  return slots;
}

// Per-antenna CSR of (baseline, role, other antenna), in baseline order: a fixed summation order.  skip_autos: without the
// autocorrelation rows (the lists of gain_solve_ant_kernel; solve_plan.hpp).  ent is never empty (one spare entry).
inline void antenna_lists(int nants, const std::vector<int2>& bl_ant, bool skip_autos, std::vector<int>& ptr, std::vector<int2>& ent) {
  const int nbls = (int)bl_ant.size();
  auto skip = [&](int b) { return skip_autos && bl_ant[b].x == bl_ant[b].y; };
  ptr.assign(nants + 1, 0);
  for (int b = 0; b < nbls; ++b) {
    if (skip(b)) continue;
    ptr[bl_ant[b].x + 1]++;
    ptr[bl_ant[b].y + 1]++;
  }
  for (int a = 0; a < nants; ++a) ptr[a + 1] += ptr[a];
  ent.assign((size_t)std::max(1, ptr[nants]), int2{});
  std::vector<int> fill(ptr.begin(), ptr.end() - 1);
  for (int b = 0; b < nbls; ++b) {
    if (skip(b)) continue;
    ent[fill[bl_ant[b].x]++] = make_int2(b * 2 + 0, bl_ant[b].y);
    ent[fill[bl_ant[b].y]++] = make_int2(b * 2 + 1, bl_ant[b].x);
  }
}

// What set-up decides about a problem and the solver keeps (SolverT derives from it; a communicator may still change mf_ok,
// steps_per_sync and lamb_ok: agree_problem).
struct PlanScalars {
  int nants = 0, nfreqs = 0, fpad = 0, ngrps = 0, nbls = 0, ncoef = 0, nitems = 0, layout = 0;
  // time slices (cal_problem_desc::nslices): independent fits held together; slice t owns antennas [t na_slice, (t + 1) na_slice),
  // a contiguous run of the coefficient planes, its own loop state (state[par][t]), reduced sums (scal[4 t ..]) and loss history
  int nslices = 1, na_slice = 0;
  bool fold = false;        // the single-baseline items read folded tiles: channels [0, nfreqs / 2) of a mirror-symmetric basis (process_item, FOLD)
  bool small_loads = false; // every single-baseline item's tile fits kSmallLoads loads per thread: the narrow instance of fused_basis_kernel serves the loss / gradient passes
  int nitems_simple = 0;   // items [0, nitems_simple) are single-baseline groups (fused_basis_kernel), the rest multi-baseline (fused_group_kernel)
  int nitems_plain = 0;    // items [0, nitems_plain) of those are not covered by a head item of the multi-slice kernels
  bool gc_direct = true;   // every group is one item: the kernels write the coefficient gradient itself, no partials to sum
  long long gcp_len = 0;   // reals per plane of the coefficient-gradient partials
  double basis_bytes = 0;  // basis bytes a pass reads
  size_t lds_bytes = 0, lds_group_bytes = 0, lds_multi_bytes = 0, lds_multi_mfma_bytes = 0;  // dynamic LDS of the general kernels' launches
  int nheads = 0, nheads_mfma = 0;             // heads[0 .. nheads_mfma): fused_multi_mfma_kernel (at most kMmMaxVec vectors); the rest: fused_multi_kernel
  bool heads_one_pass_local = false;           // the regularised step of the heads in ONE pass, as this rank's own heads allow (a communicator may clear heads_one_pass: agree_problem)
  int mm_grid = 0;                             // workgroups of the matrix-core multi-slice launch: its head list is dealt over the 8 XCDs (-1: empty slot)
  // dense (MFMA) path of the SHARED layout, one baseline per fitting group
  bool mf_ok = false;
  bool mf_split = false;                       // fp32: the split-bf16 kernel (split_kernels.hpp: super-panels of 4 panels) instead of fused_dense_kernel
  bool mf_split2 = false;                      // ... in its one-image form (split2_kernels.hpp)
  int mf_npanels = 0, mf_grid = 0;             // panel records; workgroups of the dense launch (slots of the panel map)
  size_t mf_lds_grad[2] = {0, 0}, mf_lds_loss[2] = {0, 0};  // per launch class
  int steps_per_sync = 1;                      // train steps enqueued between two host synchronisations of run()
  int lamb_nvar = 0, lamb_ncvar = 0;
  bool lamb_ok = true;
};

template <typename T>
struct ProblemPlan : PlanScalars {
  int nbasis = 0;
  // ---- what is uploaded
  std::vector<int> fb_u;                 // [nbasis] tile width of every basis block
  std::vector<long long> uoff;           // [nbasis + 1] element offsets of the retiled unique blocks
  long long tiles_elems = 0;             // elements of the tile buffer in front of its zeroed pad
  std::vector<long long> bl_tile;        // [nbls] element offset of every baseline's first tile
  std::vector<CopyJob> jobs;             // STREAM layout: unique block -> the baselines' own tiles
  std::vector<int> grp_coff, slice_coff, slice_cblk;
  std::vector<LambVar> lamb_vars;
  std::vector<int> lamb_cvar_ptr, lamb_cvar_slice, lamb_cvar_id;
  std::vector<int2> runs, bl_ant;
  std::vector<Item> items;               // in launch order
  std::vector<int> item_goff, grp_item_ptr, coef_grp;  // (item_goff in the order the items were cut: group by group; coef_grp only if !gc_direct)
  std::vector<int> slice_ipart_ptr, slice_ipart_idx, slice_ppart_ptr, slice_ppart_idx;  // nslices > 1
  std::vector<Member> members;
  std::vector<PanelItem> panels;
  std::vector<int> heads, panel_map, ant_ptr;  // (heads, panel_map: -1 marks an empty slot of the XCD deal)
  std::vector<long long> op_off;         // dense path: [nbasis + 1] BYTE offsets of the blocks' packed operands (the pack kernels)
  std::vector<CsGroup> cs_grp;
  std::vector<int2> ant_ent;
  // ---- passed from phase to phase
  bool want_mfma = false, want_split = false;
  int ftile = 0;                         // channels a baseline's tiles cover
  std::vector<int> grp_slice, grp_of_bl, alias_root, grp_run0, set_cap, order;
  std::vector<char> basis_used, in_alias_set, item_multi;
  std::vector<long long> item_cost;
  std::vector<std::vector<int>> alias_sets;

  int validate(const cal_problem_desc* d) {
    if (!d || d->nants <= 0 || d->nfreqs <= 0 || d->ngrps <= 0 || d->nbls <= 0 || d->nbasis <= 0)
      return fail(CAL_ERR_INVALID, "set_problem: non-positive dimension");
    if (!d->basis_offset || !d->basis_nvec || !d->basis_nrowblk || !d->basis_data || !d->grp_basis || !d->grp_bl_start ||
        !d->bl_ant0 || !d->bl_ant1)
      return fail(CAL_ERR_INVALID, "set_problem: null pointer in problem description");
    if (d->layout != CAL_LAYOUT_STREAM && d->layout != CAL_LAYOUT_SHARED) return fail(CAL_ERR_INVALID, "set_problem: bad layout");
    if (d->grp_bl_start[0] != 0 || d->grp_bl_start[d->ngrps] != d->nbls)
      return fail(CAL_ERR_INVALID, "set_problem: grp_bl_start must run from 0 to nbls");
    nants = d->nants; nfreqs = d->nfreqs; ngrps = d->ngrps; nbls = d->nbls; nbasis = d->nbasis; layout = d->layout;
    fb_u.assign(nbasis, 0);
    int fb_used_max = 0;
    for (int u = 0; u < nbasis; ++u) {
      if (d->basis_nvec[u] <= 0 || d->basis_nrowblk[u] <= 0) return fail(CAL_ERR_INVALID, "set_problem: empty basis block %d", u);
      const long long want = (long long)d->basis_nvec[u] * d->basis_nrowblk[u] * nfreqs;
      if (d->basis_offset[u + 1] - d->basis_offset[u] != want)
        return fail(CAL_ERR_INVALID, "set_problem: basis block %d has %lld elements, expected %lld", u,
                    (long long)(d->basis_offset[u + 1] - d->basis_offset[u]), want);
      fb_u[u] = choose_fb<T>(d->basis_nvec[u], nfreqs);
      if (fb_u[u] < 0)
        return fail(CAL_ERR_UNSUPPORTED, "set_problem: basis block %d has %d vectors; at most %d are supported for this dtype", u,
                    d->basis_nvec[u], (int)(kTileBytes / sizeof(T) / FbSet<T>::fb_min));
      fb_used_max = std::max(fb_used_max, fb_u[u]);
    }
    // Row padding is a function of nfreqs alone (never of this rank's basis blocks or kernel choice): every rank of a
    // sharded fit must lay the gains out identically and all-reduce the same number of reals.  pw = min(128,
    // next_pow2(nfreqs)) is a multiple of every tile width in use and, for nfreqs > 64, of the dense kernel's chunk.
    int pw = 8;
    while (pw < 128 && pw < nfreqs) pw *= 2;
    if (fb_used_max > pw) return fail(CAL_ERR_INVALID, "set_problem: internal error: tile width %d exceeds the row padding %d", fb_used_max, pw);
    fpad = (nfreqs + pw - 1) / pw * pw;
    if (d->kernel_path != CAL_PATH_AUTO && d->kernel_path != CAL_PATH_GENERAL && d->kernel_path != CAL_PATH_DENSE && d->kernel_path != CAL_PATH_DENSE_F32 &&
        d->kernel_path != CAL_PATH_DENSE_SPLIT1 && d->kernel_path != CAL_PATH_GENERAL_FULL)
      return fail(CAL_ERR_INVALID, "set_problem: bad kernel_path %d", d->kernel_path);
    if (d->kernel_path == CAL_PATH_DENSE_F32 && !std::is_same<T, float>::value)
      return fail(CAL_ERR_UNSUPPORTED, "set_problem: CAL_PATH_DENSE_F32 is the fp32 kernel on v_mfma_f32_32x32x2_f32; this solver is fp64");
    if (d->kernel_path == CAL_PATH_DENSE_SPLIT1 && !std::is_same<T, float>::value)
      return fail(CAL_ERR_UNSUPPORTED, "set_problem: CAL_PATH_DENSE_SPLIT1 is an fp32 kernel (split-bf16 operands); this solver is fp64");
    const bool forced_dense = d->kernel_path == CAL_PATH_DENSE || d->kernel_path == CAL_PATH_DENSE_F32 || d->kernel_path == CAL_PATH_DENSE_SPLIT1;
    want_split = std::is_same<T, float>::value && d->kernel_path != CAL_PATH_DENSE_F32;
    for (int u = 0; u < nbasis && want_split; ++u) want_split = d->basis_nvec[u] <= kSplitMaxNvec;  // (wider blocks: the f32 kernel, up to 256 vectors)
    // dense (matrix-core) path: eligibility, then -- for CAL_PATH_AUTO -- whether the problem fills the chip
    bool dense_ok = layout == CAL_LAYOUT_SHARED && fpad % kChunk == 0;
    for (int g = 0; g < ngrps && dense_ok; ++g) dense_ok = (d->grp_bl_start[g + 1] - d->grp_bl_start[g]) == 1;
    for (int u = 0; u < nbasis && dense_ok; ++u) dense_ok = d->basis_nrowblk[u] == 1 && d->basis_nvec[u] <= DenseCfg<T>::max_nvec;
    // the dense kernels address the per-sample arrays with 32-bit BYTE offsets; the widest sample is one (re, im) pair
    if ((long long)(nbls + 2) * fpad * 2 * (long long)sizeof(T) >= (1LL << 32)) dense_ok = false;
    // ... and its packed operands (two MFMA-native copies of every unique block) with 32-bit byte offsets from one base
    long long dense_op_elems = 0;
    for (int u = 0; u < nbasis && dense_ok; ++u)  // kilobyte positions: forward + adjoint (the same count for both dtypes' layouts up to padding)
      dense_op_elems += want_split ? std::max(split_stream_bytes(fpad, d->basis_nvec[u], (d->basis_nvec[u] + 31) / 32), split2_stream_bytes(fpad, d->basis_nvec[u])) / 4
                        : std::is_same<T, float>::value
                            ? (long long)(fpad / 32) * ((d->basis_nvec[u] + 7) / 8) * 256 + (long long)(fpad / 32) * ((d->basis_nvec[u] + 31) / 32) * 4 * 256
                            : (long long)(fpad / 16) * ((d->basis_nvec[u] + 7) / 8) * 128 + (long long)(fpad / 16) * ((d->basis_nvec[u] + 15) / 16) * 2 * 128;
    if (dense_op_elems * (long long)(want_split ? 4 : sizeof(T)) >= (1LL << 32)) dense_ok = false;
    if (forced_dense && !dense_ok)
      return fail(CAL_ERR_UNSUPPORTED, "set_problem: CAL_PATH_DENSE needs the SHARED layout, one baseline per fitting group, "
                  "basis_nvec <= %d and nfreqs > 64", DenseCfg<T>::max_nvec);
    // a panel of 16 baselines occupies one CU for 60-70 us whatever the problem size; below ~2000 baselines the panels do
    // not fill the chip and the general kernel (one workgroup per baseline) is 2-3x faster (HERA-37 fp32: 25 vs 71 us)
    // (with a communicator the ranks then agree on ONE path -- the exchange payload of the "sum" regulariser differs between
    // the two -- in set_problem, behind all the rank-local work)
    want_mfma = dense_ok && d->kernel_path != CAL_PATH_GENERAL && d->kernel_path != CAL_PATH_GENERAL_FULL && (forced_dense || nbls >= 2048);
    for (int b = 0; b < d->nbls; ++b) {
      if (d->bl_ant0[b] < 0 || d->bl_ant0[b] >= nants || d->bl_ant1[b] < 0 || d->bl_ant1[b] >= nants)
        return fail(CAL_ERR_INVALID, "set_problem: baseline %d has an antenna index outside [0, %d)", b, nants);
    }
    return CAL_OK;
  }

  // ---- time slices: independent fits over disjoint antenna ranges, listed slice by slice
  int time_slices(const cal_problem_desc* d) {
    const int NSL = d->nslices > 1 ? d->nslices : 1;
    if (NSL > CAL_MAX_SLICES) return fail(CAL_ERR_UNSUPPORTED, "set_problem: %d time slices; at most %d are supported", NSL, CAL_MAX_SLICES);
    if (nants % NSL != 0) return fail(CAL_ERR_INVALID, "set_problem: nants = %d is not a multiple of nslices = %d", nants, NSL);
    const int nas = nants / NSL;
    grp_slice.assign(ngrps, 0);
    if (NSL > 1) {
      std::vector<char> seen(NSL, 0);
      for (int g = 0; g < ngrps; ++g) {
        const int b0 = d->grp_bl_start[g], b1 = d->grp_bl_start[g + 1];
        if (b0 < 0 || b1 > nbls || b1 <= b0) return fail(CAL_ERR_INVALID, "set_problem: group %d has no baselines", g);
        const int t = d->bl_ant0[b0] / nas;
        for (int b = b0; b < b1; ++b)
          if (d->bl_ant0[b] / nas != t || d->bl_ant1[b] / nas != t)
            return fail(CAL_ERR_INVALID, "set_problem: baseline %d of group %d leaves time slice %d (antennas %d, %d; %d antennas per slice)", b, g, t,
                        d->bl_ant0[b], d->bl_ant1[b], nas);
        if (g > 0 && t < grp_slice[g - 1]) return fail(CAL_ERR_INVALID, "set_problem: fitting groups must be listed slice by slice (group %d)", g);
        grp_slice[g] = t;
        seen[t] = 1;
      }
      for (int t = 0; t < NSL; ++t)
        if (!seen[t]) return fail(CAL_ERR_INVALID, "set_problem: time slice %d has no fitting group", t);
    }
    nslices = NSL;
    na_slice = nas;
    return CAL_OK;
  }

  // ---- groups, coefficient offsets, the optimizer's variables
  int groups_and_variables(const cal_problem_desc* d) {
    grp_coff.assign(ngrps + 1, 0);
    grp_of_bl.assign(nbls, 0);
    for (int g = 0; g < ngrps; ++g) {
      const int u = d->grp_basis[g];
      if (u < 0 || u >= nbasis) return fail(CAL_ERR_INVALID, "set_problem: group %d points at basis %d", g, u);
      if (d->grp_bl_start[g + 1] <= d->grp_bl_start[g]) return fail(CAL_ERR_INVALID, "set_problem: group %d has no baselines", g);
      grp_coff[g + 1] = grp_coff[g] + d->basis_nvec[u];
      for (int b = d->grp_bl_start[g]; b < d->grp_bl_start[g + 1]; ++b) {
        grp_of_bl[b] = g;
        const int rb = d->bl_rowblk ? d->bl_rowblk[b] : 0;
        if (rb < 0 || rb >= d->basis_nrowblk[u]) return fail(CAL_ERR_INVALID, "set_problem: baseline %d row block %d out of range", b, rb);
      }
    }
    ncoef = grp_coff[ngrps];
    slice_coff.assign(nslices + 1, ncoef);
    for (int g = ngrps - 1; g >= 0; --g) slice_coff[grp_slice[g]] = grp_coff[g];  // first group of every slice
    slice_coff[0] = 0;
    // the optimizer's variables (LAMB): a new coefficient variable wherever the (slice, grp_var) of the groups changes
    lamb_ok = true;
    std::vector<int>& cptr = lamb_cvar_ptr;
    for (int g = 0; g < ngrps; ++g) {
      const int var = d->grp_var ? d->grp_var[g] : 0;
      if (var < 0) return fail(CAL_ERR_INVALID, "set_problem: grp_var[%d] = %d is negative", g, var);
      // (groups of one variable scattered over a slice: fine for every element-wise optimizer; LAMB is refused in set_optimizer)
      if (g > 0 && grp_slice[g] == grp_slice[g - 1] && d->grp_var && var < d->grp_var[g - 1]) lamb_ok = false;
      if (g == 0 || grp_slice[g] != grp_slice[g - 1] || (d->grp_var && var != d->grp_var[g - 1])) {
        cptr.push_back(grp_coff[g]);
        lamb_cvar_slice.push_back(grp_slice[g]);
        lamb_cvar_id.push_back(var);
      }
    }
    lamb_ncvar = (int)cptr.size();
    cptr.push_back(ncoef);
    lamb_nvar = 2 * nslices + 2 * lamb_ncvar;
    for (int t = 0; t < nslices; ++t)
      for (int c = 0; c < 2; ++c) lamb_vars.push_back(LambVar{(long long)t * na_slice * fpad * 2 + c, (long long)na_slice * fpad, 2, 0});
    for (int plane = 0; plane < 2; ++plane)
      for (int k = 0; k < lamb_ncvar; ++k) lamb_vars.push_back(LambVar{(long long)plane * ncoef + cptr[k], (long long)(cptr[k + 1] - cptr[k]), 1, 1});
    // coefficient blocks of step_tail_kernel: every slice gets its own (a block works for ONE slice's decisions)
    slice_cblk.assign(nslices + 1, 0);
    for (int t = 0; t < nslices; ++t) {
      const long long nb = (2LL * (slice_coff[t + 1] - slice_coff[t]) + 255) / 256;
      slice_cblk[t + 1] = slice_cblk[t] + (int)std::max<long long>(1, std::min<long long>(nb, std::max(1, 4096 / nslices)));
    }
    // the groups as the kernels of solve_coeffs see them
    cs_grp.assign(ngrps, CsGroup{});
    for (int g = 0; g < ngrps; ++g) {
      const int u = d->grp_basis[g];
      int lg = 0;
      while ((1 << lg) < fb_u[u]) ++lg;
      cs_grp[g] = CsGroup{d->grp_bl_start[g], d->grp_bl_start[g + 1], d->basis_nvec[u], grp_coff[g], lg, grp_slice[g], 0, 0};
    }
    return CAL_OK;
  }

  int aliases_and_fold(const cal_problem_desc* d) {
    // ---- baselines that read another baseline's tiles (STREAM layout): the same physical baseline in several time slices
    alias_root.assign(nbls, -1);  // -1: owns its tiles
    if (d->bl_alias && layout == CAL_LAYOUT_STREAM) {
      for (int b = 0; b < nbls; ++b) {
        const int r = d->bl_alias[b];
        if (r < 0 || r == b) continue;
        if (r >= nbls || (d->bl_alias[r] >= 0 && d->bl_alias[r] != r))
          return fail(CAL_ERR_INVALID, "set_problem: bl_alias[%d] = %d must name a baseline that owns its tiles", b, r);
        const int g = grp_of_bl[b], gr = grp_of_bl[r];
        if (d->grp_basis[g] != d->grp_basis[gr] || (d->bl_rowblk ? d->bl_rowblk[b] != d->bl_rowblk[r] : false))
          return fail(CAL_ERR_INVALID, "set_problem: bl_alias[%d] = %d: the two baselines use different basis rows", b, r);
        if (d->grp_bl_start[g + 1] - d->grp_bl_start[g] != 1 || d->grp_bl_start[gr + 1] - d->grp_bl_start[gr] != 1)
          return fail(CAL_ERR_INVALID, "set_problem: bl_alias is for single-baseline fitting groups (baseline %d)", b);
        alias_root[b] = r;
      }
    }
    // ---- folded tiles: decided once per problem, from the description and the dtype alone (never from the communicator, the
    // launch mode or the device: solvers that are compared bit for bit must take the same form).  The streaming layout, every
    // item served by fused_basis_kernel (single-baseline groups, no shared tiles: the multi-slice and the group kernels keep
    // full tiles) and every basis block in use mirror-symmetric; CAL_PATH_GENERAL_FULL keeps the full tiles.
    fold = layout == CAL_LAYOUT_STREAM && d->kernel_path != CAL_PATH_GENERAL_FULL;
    for (int g = 0; g < ngrps && fold; ++g) fold = d->grp_bl_start[g + 1] - d->grp_bl_start[g] == 1;
    for (int b = 0; b < nbls && fold; ++b) fold = alias_root[b] < 0;
    basis_used.assign(nbasis, 0);
    for (int g = 0; g < ngrps; ++g) basis_used[d->grp_basis[g]] = 1;
    for (int u = 0; u < nbasis && fold; ++u) {
      double resid, amax;
      if (basis_used[u])
        fold = block_foldable(static_cast<const T*>(d->basis_data) + d->basis_offset[u], nfreqs, d->basis_nvec[u], d->basis_nrowblk[u], fb_u[u], &resid, &amax);
    }
    ftile = fold ? nfreqs / 2 : fpad;
    lds_bytes = 0;
    for (int u = 0; u < nbasis; ++u)
      lds_bytes = std::max(lds_bytes, with_fb<T>(fb_u[u], [&](auto fb) { return TileCfg<T, decltype(fb)::value>::lds_bytes(fold); }));
    in_alias_set.assign(nbls, 0);
    const bool multi_ok = (long long)(nbls + 1) * fpad < (1LL << 31) && (long long)nants * fpad < (1LL << 31);  // the multi kernel's 32-bit sample offsets
    for (int b = 0; b < nbls; ++b)
      if (alias_root[b] >= 0 && multi_ok) in_alias_set[b] = in_alias_set[alias_root[b]] = 1;  // (slices_share_heads: see head_items)
    return CAL_OK;
  }

  // ---- unique basis blocks -> tile-major device layout, and where every baseline's tiles lie in it
  void tile_layout(const cal_problem_desc* d) {
    uoff.assign(nbasis + 1, 0);
    // (folded: the lower half band of the blocks in use -- one row block each -- verbatim; the others are not needed)
    for (int u = 0; u < nbasis; ++u)
      uoff[u + 1] = uoff[u] + (fold ? (basis_used[u] ? (long long)ftile * d->basis_nvec[u] : 0LL) : (long long)d->basis_nrowblk[u] * fpad * d->basis_nvec[u]);
    bl_tile.assign(nbls, 0);
    bl_ant.resize(nbls);
    for (int b = 0; b < nbls; ++b) bl_ant[b] = make_int2(d->bl_ant0[b], d->bl_ant1[b]);
    if (layout == CAL_LAYOUT_SHARED) {
      for (int b = 0; b < nbls; ++b) {
        const int u = d->grp_basis[grp_of_bl[b]];
        const int rb = d->bl_rowblk ? d->bl_rowblk[b] : 0;
        bl_tile[b] = uoff[u] + (long long)rb * fpad * d->basis_nvec[u];
      }
      tiles_elems = uoff[nbasis];
      basis_bytes = (double)uoff[nbasis] / fpad * nfreqs * sizeof(T);
    } else {
      // every baseline owns its tiles, except that consecutive baselines of one group with the same row block (a
      // redundant set: one forward product for all of them) share one copy
      jobs.reserve(nbls);
      long long off = 0;
      for (int b = 0; b < nbls; ++b) {
        const int u = d->grp_basis[grp_of_bl[b]];
        const int rb = d->bl_rowblk ? d->bl_rowblk[b] : 0;
        const long long n = (long long)ftile * d->basis_nvec[u];
        const bool alias = b > 0 && grp_of_bl[b - 1] == grp_of_bl[b] && (d->bl_rowblk ? d->bl_rowblk[b - 1] : 0) == rb;
        if (alias) {
          bl_tile[b] = bl_tile[b - 1];
          continue;
        }
        if (alias_root[b] >= 0) continue;  // filled in below, once its owner's offset is known (the owner may come later)
        jobs.push_back(CopyJob{uoff[u] + (long long)rb * n, off, n});
        bl_tile[b] = off;
        off += n;
      }
      for (int b = 0; b < nbls; ++b)
        if (alias_root[b] >= 0) bl_tile[b] = bl_tile[alias_root[b]];
      tiles_elems = off;
      basis_bytes = fold ? (double)off * sizeof(T) : (double)off / fpad * nfreqs * sizeof(T);
    }
    // ~ tens of milliseconds of GPU time between two host synchronisations of run(); the same on every rank, or ranks
    // would notice a tolerance stop after different step counts and issue different numbers of all-reduces
    steps_per_sync = (int)std::max(1.0, std::min(256.0, 2.0e11 / ((double)basis_bytes + 1.0)));
  }

  // Panels of the dense kernels: the baselines of one (basis block, time slice) -- a panel never mixes slices: one loop state, one alpha
  // per panel -- cut into work items of `per` panel records with width(nvec) baselines each (the other slots padding), widest blocks first.
  // unit: bytes per element of PanelItem::a_kf4; cost(nvec, width): an item's time on a CU.
  // Then the XCD-affine dispatch of the launch (dense_kernels.hpp: fused_dense_kernel): all panels of a basis block on one of the 8 lists
  // (deal_over_xcds), inside a list the heaviest first: the hardware dispatches workgroups in index order, so the tail of the pass is made
  // of the lightest.  cost and the map count items, not records.
  template <typename Width, typename Cost>
  void build_panels(const cal_problem_desc* d, int per, int unit, Width width, Cost cost) {
    std::vector<std::vector<int>> by_u((size_t)nbasis * nslices);
    for (int b = 0; b < nbls; ++b) by_u[(size_t)d->grp_basis[grp_of_bl[b]] * nslices + grp_slice[grp_of_bl[b]]].push_back(b);
    std::vector<int> uorder((size_t)nbasis * nslices);
    std::iota(uorder.begin(), uorder.end(), 0);
    std::stable_sort(uorder.begin(), uorder.end(), [&](int a, int b) { return d->basis_nvec[a / nslices] > d->basis_nvec[b / nslices]; });
    std::vector<double> h_cost;
    for (int us : uorder) {
      const int u = us / nslices;
      const int nv = d->basis_nvec[u], w = width(nv);
      for (size_t i = 0; i < by_u[us].size(); i += (size_t)w * per) {
        for (int r = 0; r < per; ++r) {
          PanelItem pi{};
          pi.slice = us % nslices;
          for (int k = 0; k < kPanel; ++k) {
            const size_t at = i + (size_t)r * w + k;
            const int b = k < w && at < by_u[us].size() ? by_u[us][at] : -1;
            pi.bl[k] = b;
            pi.coff[k] = b >= 0 ? grp_coff[grp_of_bl[b]] : 0;
            pi.ant[k] = b >= 0 ? make_int2(d->bl_ant0[b], d->bl_ant1[b]) : make_int2(0, 0);
          }
          pi.a_kf4 = op_off[u] / unit;
          pi.a_fk4 = 0;
          pi.nvec = nv;
          if (sizeof(T) == 4) {
            pi.nvp2 = (nv + 15) / 16 * 16;
            pi.nvp32 = (nv + 31) / 32 * 32;
          }
          pi.tile0 = 0;  // (split-bf16 kernel: kSplitNT = 8 vector tiles, a whole block, fit one item since it runs one workgroup per CU)
          panels.push_back(pi);
        }
        h_cost.push_back(cost(nv, w));
      }
    }
    const int n = (int)panels.size() / per;
    // KNOWN ISSUE ("panel keys"): item i is looked up by the key of record i * per but a new block registers the key of record
    // i, so with per > 1 most items miss the lookup and become "blocks" of their own: the block-to-XCD affinity is then mostly not what
    // runs.  Kept as it is -- the map decides the dispatch of the headline kernel; changing it needs its own A/B measurement.
    std::vector<long long> keys;
    std::vector<int> blk(n);
    for (int i = 0; i < n; ++i) {
      size_t k = std::find(keys.begin(), keys.end(), panels[(size_t)i * per].a_kf4) - keys.begin();
      if (k == keys.size()) keys.push_back(panels[i].a_kf4);
      blk[i] = (int)k;
    }
    panel_map = deal_over_xcds(blk, (int)keys.size(), h_cost, false);
    mf_npanels = (int)panels.size();
    mf_grid = (int)panel_map.size();
    if (nslices > 1) slice_partial_index(panels, nslices, slice_ppart_ptr, slice_ppart_idx);  // the loss partials (one per panel), in panel order
    mf_ok = true;
  }

  // ---- the dense (matrix-core) path of the SHARED layout: which kernel, where every block's packed operands lie, the panels
  void dense_panels(const cal_problem_desc* d) {
    mf_ok = mf_split = mf_split2 = false;
    if (!want_mfma) return;
    op_off.assign(nbasis + 1, 0);
    if constexpr (std::is_same<T, float>::value) {
      if (want_split) {
        // split-bf16 operands (split_kernels.hpp): super-panels of kSpWaves panels (64 baselines) with the same basis block and slice;
        // the one-image form (split2_kernels.hpp) unless the first one is asked for by name
        const bool v2 = d->kernel_path != CAL_PATH_DENSE_SPLIT1;
        for (int u = 0; u < nbasis; ++u)
          op_off[u + 1] = op_off[u] + (v2 ? split2_stream_bytes(fpad, d->basis_nvec[u]) : split_stream_bytes(fpad, d->basis_nvec[u], (d->basis_nvec[u] + 31) / 32));
        // an item's time on a CU: per channel-block pair two element stages + its groups of 24 MFMAs
        build_panels(d, kSpWaves, 4, [](int) { return kPanel; },
                     [&](int nv, int) { return (fpad / 64) * (3000.0 + 900.0 * split_groups_per_pair(nv, (nv + 31) / 32)); });
        mf_lds_grad[0] = mf_lds_loss[0] = v2 ? (size_t)kS2Lds : split_lds_bytes();
        mf_split = true;
        mf_split2 = v2;
        return;
      }
      // v_mfma_f32_32x32x2_f32 (dense_kernels.hpp): panels of kPanel baselines.  Panels of more than four vector tiles and the rest are
      // two bodies of ONE launch.
      // Per-XCD panel lists (all panels of a basis block on one XCD, its packed operands L2-resident there: the L2 hit
      // rate of the operand requests is only 55-65 % without them) measured 3-5 % SLOWER with every generation of this
      // kernel: panels of one block then walk the same lines in step.
      int nvec_max = 0;
      for (int u = 0; u < nbasis; ++u) {
        nvec_max = std::max(nvec_max, d->basis_nvec[u]);
        op_off[u + 1] = op_off[u] + (long long)(fpad / 32) * ((d->basis_nvec[u] + 7) / 8 + (d->basis_nvec[u] + 31) / 32 * 4) * 256 * (long long)sizeof(float);
      }
      // a panel's time on a CU: a fixed part (prologue, element stage, epilogue) + its MFMA positions (stamps of the HERA-350 pass)
      build_panels(d, 1, 4, [](int) { return kPanel; },
                   [&](int nv, int) { return 60e3 + 600.0 * (fpad / kChunk) * ((nv + 7) / 8 + (nv + 31) / 32 * 4); });
      // one launch serves both panel classes (up to 4 / up to 8 vector tiles): the larger of their LDS footprints
      mf_lds_grad[0] = std::max(dense_lds_bytes(nvec_max, true, nvec_max > 128 ? 8 : 4), dense_lds_bytes(std::min(nvec_max, 128), true, 4));
      mf_lds_loss[0] = std::max(dense_lds_bytes(nvec_max, false, nvec_max > 128 ? 8 : 4), dense_lds_bytes(std::min(nvec_max, 128), false, 4));
    } else {
      // double precision: v_mfma_f64_16x16x4_f64 (dense64_kernels.hpp).  Two panel classes (bodies of one launch): blocks
      // of more than 128 vectors with panels of 8 baselines (one column tile, 16 gradient tiles), the rest with panels of 16
      int nvec_a = 0, nvec_b = 0;
      for (int u = 0; u < nbasis; ++u) {
        const int nv = d->basis_nvec[u];
        (nv > 128 ? nvec_a : nvec_b) = std::max(nv > 128 ? nvec_a : nvec_b, nv);
        op_off[u + 1] = op_off[u] + (long long)(fpad / kCB64) * ((nv + 7) / 8 + (nv + kVT64 - 1) / kVT64 * 2) * 128 * (long long)sizeof(double);
      }
      build_panels(d, 1, 8, [](int nv) { return nv > 128 ? 8 : 16; },
                   [&](int nv, int w) { return 60e3 + 300.0 * (w / 8) * (fpad / (4 * kCB64)) * ((nv + 7) / 8 + (nv + kVT64 - 1) / kVT64 * 2); });
      mf_lds_grad[0] = std::max(dense64_lds_bytes(nvec_a, 1, true), dense64_lds_bytes(nvec_b, 2, true));
      mf_lds_loss[0] = std::max(dense64_lds_bytes(nvec_a, 1, false), dense64_lds_bytes(nvec_b, 2, false));
    }
  }

  // which head items fused_multi_mfma_kernel takes: blocks of at most kMmMaxVec vectors, rows padded to a multiple of 128 channels (any
  // band of more than 64: its waves take an even number of 16-channel strips each)
  bool mfma_head_shape(const Item& q) const { return q.nvec <= kMmMaxVec && (1 << q.fb_log2) >= kMmStrip && fpad % 128 == 0; }

  void runs_and_items(const cal_problem_desc* d) {
    // ---- runs of the multi-baseline groups: consecutive baselines with the same row block, cut to kRunMax
    grp_run0.assign(ngrps + 1, 0);
    int nsimple_grps = 0;
    for (int g = 0; g < ngrps; ++g) {
      const int s0 = d->grp_bl_start[g], s1 = d->grp_bl_start[g + 1];
      grp_run0[g] = (int)runs.size();
      if (s1 - s0 == 1) {
        ++nsimple_grps;
        continue;
      }
      int lo = s0;
      for (int b = s0 + 1; b <= s1; ++b) {
        const bool cut = b == s1 || (d->bl_rowblk && d->bl_rowblk[b] != d->bl_rowblk[lo]) || b - lo == kRunMax;
        if (cut) {
          runs.push_back(make_int2(lo, b));
          lo = b;
        }
      }
    }
    grp_run0[ngrps] = (int)runs.size();

    // ---- work items: whole groups when that already fills the chip, otherwise split along tiles
    long long total_tiles = 0;
    for (int g = 0; g < ngrps; ++g)
      if (d->grp_bl_start[g + 1] - d->grp_bl_start[g] == 1) total_tiles += ftile / fb_u[d->grp_basis[g]];  // (folded tiles where the problem folds)
    // one item per group when the groups alone fill the chip (256 CUs x ~4 resident workgroups, several waves of them);
    // otherwise split groups along their tiles (partial coefficient gradients are summed by coeff_partial_reduce_kernel)
    // With at least one group per CU an item is never smaller than 1024 channels of its group (8 tiles of the widest fp32
    // shape, 16 of the widest fp64 one): a group of up to 56 vectors is then ONE item -- no partial coefficient gradients,
    // no second launch to sum them -- and only wider groups (narrower tiles) are cut, which also evens the items out.
    // Measured at HERA-37 (666 groups): fp64 76 -> 61 us per step, fp32 45 -> 42; cutting every group into 4-tile items
    // (the earlier rule) bought parallelism the chip did not need and paid a prologue and a reduction for it.
    const long long target_items = 8192;
    const bool groups_fill_chip = nsimple_grps >= 2048;
    const long long min_tiles = nsimple_grps >= 256 ? 1024 / FbSet<T>::fb_max : 4;
    const long long tiles_per_item = groups_fill_chip ? std::max<long long>(64, 4 * total_tiles / std::max(1, nsimple_grps))
                                                      : std::max<long long>(min_tiles, total_tiles / target_items);
    std::vector<Item> h_items;
    grp_item_ptr.assign(ngrps + 1, 0);
    gc_direct = true;
    lds_group_bytes = 0;
    for (int g = 0; g < ngrps; ++g) {
      const int u = d->grp_basis[g];
      const int ntpb = ftile / fb_u[u];
      int fl = 0;
      while ((1 << fl) < fb_u[u]) ++fl;
      Item it{};
      it.nvec = d->basis_nvec[u];
      it.coff = grp_coff[g];
      it.fb_log2 = fl;
      it.slice = grp_slice[g];
      if (d->grp_bl_start[g + 1] - d->grp_bl_start[g] == 1) {
        const long long nt = ntpb;
        // (a baseline that shares tiles stays ONE item: the multi kernel writes the whole coefficient gradient of its group)
        const int nparts = in_alias_set[d->grp_bl_start[g]] ? 1 : (int)std::max<long long>(1, (nt + tiles_per_item - 1) / tiles_per_item);
        if (nparts > 1) gc_direct = false;
        for (int k = 0; k < nparts; ++k) {
          it.bl0 = d->grp_bl_start[g];
          it.tile0 = (int)(nt * k / nparts);
          it.tile1 = (int)(nt * (k + 1) / nparts);
          it.tile_first = bl_tile[it.bl0];
          it.ant_first = make_int2(d->bl_ant0[it.bl0], d->bl_ant1[it.bl0]);
          h_items.push_back(it);
          item_cost.push_back((long long)(it.tile1 - it.tile0) * it.nvec * fb_u[u]);
          item_multi.push_back(0);
        }
      } else {
        // units = (run, channel block), run-major; a unit costs one tile (load, forward, adjoint: about 8 batches' worth)
        // plus one batch of the per-channel stage per kThreads / FB baselines.  Items are cut at ~96 batch equivalents
        // so that a big redundant set is spread over many workgroups (their partial coefficient gradients are summed).
        lds_group_bytes = std::max(lds_group_bytes, with_fb<T>(fb_u[u], [](auto fb) { return group_lds_bytes<T, decltype(fb)::value>(); }));
        const int bpt = kThreads / fb_u[u];
        const int r0 = grp_run0[g], r1 = grp_run0[g + 1];
        const long long budget = 96;
        long long cost = 0;
        int unit_lo = 0, nparts = 0;
        const int nunits = (r1 - r0) * ntpb;
        for (int uu = 0; uu < nunits; ++uu) {
          const int2 rn = runs[r0 + uu / ntpb];
          cost += 8 + (rn.y - rn.x + bpt - 1) / bpt;
          if (cost >= budget || uu + 1 == nunits) {
            it.bl0 = r0;
            it.tile0 = unit_lo;
            it.tile1 = uu + 1;
            h_items.push_back(it);
            item_cost.push_back(cost * 1024);  // same scale as nvec x FB of a full tile, roughly
            item_multi.push_back(1);
            unit_lo = uu + 1;
            cost = 0;
            ++nparts;
          }
        }
        if (nparts > 1) gc_direct = false;
      }
      grp_item_ptr[g + 1] = (int)h_items.size();
    }
    nitems = (int)h_items.size();
    small_loads = true;
    for (const Item& q : h_items) {
      const int lpr = (1 << q.fb_log2) / (16 / (int)sizeof(T));  // lanes per tile row; a load covers kThreads / lpr rows
      if (q.nvec > kSmallLoads * (kThreads / lpr)) small_loads = false;
    }
    // single-baseline items first, then the multi-baseline ones (two launches); inside each class heaviest first: the
    // hardware dispatches workgroups in index order, so the tail is made of the lightest items
    // (among the single-baseline items those that a head item of the multi-slice kernels covers come last: the loss and gradient
    // passes launch fused_basis_kernel over the plain ones only)
    alias_sets.assign(nbls, {});
    for (int b = 0; b < nbls; ++b)
      if (in_alias_set[b]) alias_sets[alias_root[b] >= 0 ? alias_root[b] : b].push_back(b);
    // members per head item: the matrix-core kernel takes 8 in both precisions (16 MFMA columns), fused_multi_kernel
    // MultiCfg<T>::nb_max (its gradient accumulators live in registers: 4 in fp64)
    set_cap.assign(nbls, MultiCfg<T>::nb_max);
    for (int q = 0; q < nitems; ++q)
      if (!item_multi[q] && mfma_head_shape(h_items[q])) set_cap[h_items[q].bl0] = kMmMembers;
    std::vector<char> bl_covered(nbls, 0);
    for (int r = 0; r < nbls; ++r)
      for (size_t i = 0; i < alias_sets[r].size(); i += set_cap[r]) {
        const size_t n = std::min<size_t>(set_cap[r], alias_sets[r].size() - i);
        if (n >= 2)
          for (size_t k = 0; k < n; ++k) bl_covered[alias_sets[r][i + k]] = 1;
      }
    auto item_class = [&](int q) { return item_multi[q] ? 2 : (bl_covered[h_items[q].bl0] ? 1 : 0); };
    order.resize(nitems);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
      if (item_class(a) != item_class(b)) return item_class(a) < item_class(b);
      return item_cost[a] > item_cost[b];
    });
    nitems_simple = 0;
    nitems_plain = 0;
    for (int q = 0; q < nitems; ++q) {
      nitems_simple += item_multi[q] ? 0 : 1;
      nitems_plain += item_class(q) == 0 ? 1 : 0;
    }
    item_goff.assign(nitems, 0);
    gcp_len = 0;
    if (gc_direct) {
      for (int q = 0; q < nitems; ++q) item_goff[q] = h_items[q].coff;
      gcp_len = ncoef;
    } else {
      for (int q = 0; q < nitems; ++q) {
        item_goff[q] = (int)gcp_len;
        gcp_len += h_items[q].nvec;
      }
      coef_grp.assign(ncoef, 0);
      for (int g = 0; g < ngrps; ++g)
        for (int n = grp_coff[g]; n < grp_coff[g + 1]; ++n) coef_grp[n] = g;
    }
    items.resize(nitems);
    for (int q = 0; q < nitems; ++q) {
      items[q] = h_items[order[q]];
      items[q].goff = item_goff[order[q]];
      items[q].role_n = 0;
      items[q].member0 = 0;
    }
    // the loss partials (one per item) of every time slice, in item order
    if (nslices > 1) slice_partial_index(items, nslices, slice_ipart_ptr, slice_ipart_idx);
  }

  // ---- sets of baselines that share tiles -> head items with member lists (at most set_cap baselines each)
  void head_items(const cal_problem_desc* d) {
    std::vector<Item>& sorted = items;
    std::vector<int> item_of_bl(nbls, -1);
    for (int q = 0; q < nitems; ++q)
      if (!item_multi[order[q]]) item_of_bl[sorted[q].bl0] = q;
    const std::vector<std::vector<int>>& sets = alias_sets;
    std::vector<int>& h_heads = heads;
    for (int r = 0; r < nbls; ++r) {
      const int NBM = set_cap[r];
      for (size_t i = 0; i < sets[r].size(); i += NBM) {
        const int n = (int)std::min<size_t>(NBM, sets[r].size() - i);
        if (n < 2) continue;  // a lone baseline runs as an ordinary item
        const int head = item_of_bl[sets[r][i]];
        sorted[head].role_n = (n << 2) | 1;
        sorted[head].member0 = (int)members.size();
        h_heads.push_back(head);
        for (int k = 0; k < n; ++k) {
          const int b = sets[r][i + k], q = item_of_bl[b];
          if (k > 0) sorted[q].role_n = 2;
          Member m{};
          m.bl = b;
          m.coff = sorted[q].coff;
          m.goff = sorted[q].goff;
          m.ant0 = d->bl_ant0[b];
          m.ant1 = d->bl_ant1[b];
          m.slice = sorted[q].slice;
          m.item = q;
          members.push_back(m);
        }
      }
    }
    // the matrix-core form first, each list heaviest first
    auto on_mfma = [&](int head) { return mfma_head_shape(sorted[head]); };
    std::stable_sort(h_heads.begin(), h_heads.end(), [&](int a, int b) {
      const bool ma = on_mfma(a), mb = on_mfma(b);
      if (ma != mb) return ma;
      return (long long)sorted[a].nvec * (sorted[a].role_n >> 2) > (long long)sorted[b].nvec * (sorted[b].role_n >> 2);
    });
    nheads_mfma = 0;
    lds_multi_bytes = lds_multi_mfma_bytes = 0;
    for (int head : h_heads) {
      if (on_mfma(head)) {
        ++nheads_mfma;
        lds_multi_mfma_bytes = std::max(lds_multi_mfma_bytes, multi_mfma_lds_bytes<T>(sorted[head].nvec));
      } else {
        lds_multi_bytes = std::max(lds_multi_bytes, with_fb<T>(1 << sorted[head].fb_log2, [](auto fb) { return multi_lds_bytes<T, decltype(fb)::value>(); }));
      }
    }
    nheads = (int)h_heads.size();
    // the "sum" regulariser over heads: one pass with two adjoint sets when every head is on the matrix-core kernel and narrow enough
    // for it (multi_mfma_kernels.hpp, REG == 2); else a loss pass for the slices' sums in front of the gradient pass (enqueue_pass)
    heads_one_pass_local = nheads > 0 && nheads == nheads_mfma;
    for (int head : h_heads) heads_one_pass_local = heads_one_pass_local && sorted[head].nvec <= kMmMaxVecOnePass<T>;
    // XCD-affine, antenna-grouped dispatch of the matrix-core heads: a head reads 2 gain rows per member (8 slices x 2 x 8 KB of a
    // 1024-channel band) -- a fifth of its bytes, 1.0 GB per pass of an 8-GPU rank's share against 23 MB of distinct gains, because
    // with the heads in cost order nothing a workgroup brings into its XCD's L2 is wanted by its neighbours (hit rate 17 %).
    // Every first antenna -- all heads whose baseline starts at it -- goes to ONE of the 8 lists (deal_over_xcds), heaviest antenna
    // groups first in a list, heaviest head first in a group.  The ant0 rows of a group then stay in that XCD's L2 for the whole group.
    mm_grid = nheads_mfma;
    if (nheads_mfma >= 64) {
      std::map<int, int> group_of_ant;  // groups numbered by ascending first antenna
      for (int i = 0; i < nheads_mfma; ++i) group_of_ant[sorted[h_heads[i]].ant_first.x] = 0;
      int ngroups = 0;
      for (auto& kv : group_of_ant) kv.second = ngroups++;
      std::vector<int> group(nheads_mfma);
      std::vector<double> cost(nheads_mfma);
      for (int i = 0; i < nheads_mfma; ++i) {  // (already heaviest first)
        group[i] = group_of_ant[sorted[h_heads[i]].ant_first.x];
        cost[i] = (double)sorted[h_heads[i]].nvec * (sorted[h_heads[i]].role_n >> 2) + 64.0;
      }
      std::vector<int> dealt = deal_over_xcds(group, ngroups, cost, true);
      mm_grid = (int)dealt.size();
      for (int& s : dealt)
        if (s >= 0) s = h_heads[s];
      dealt.insert(dealt.end(), h_heads.begin() + nheads_mfma, h_heads.end());
      h_heads.swap(dealt);
    }
  }

};

// The checks run in this order: the first failure is the one reported (fail(): cal_last_error).
template <typename T>
int plan_problem(const cal_problem_desc* d, ProblemPlan<T>& p) {
  p = ProblemPlan<T>{};
  CAL_TRY(p.validate(d));
  CAL_TRY(p.time_slices(d));
  CAL_TRY(p.groups_and_variables(d));
  CAL_TRY(p.aliases_and_fold(d));
  p.tile_layout(d);
  p.dense_panels(d);
  p.runs_and_items(d);
  p.head_items(d);
  antenna_lists(p.nants, p.bl_ant, false, p.ant_ptr, p.ant_ent);
  return CAL_OK;
}

}  // namespace
