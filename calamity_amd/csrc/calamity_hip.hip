// calamity_hip.hip -- C-ABI (include/calamity_hip.h) and host orchestration of the gfx950 fit kernels.
// No PyTorch, no TensorFlow, no CPU fallback: every compute entry point launches the HIP kernels of fit_kernels.hpp.
#include "../../include/calamity_hip.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

#include "fit_kernels.hpp"
#include "dense_kernels.hpp"
#include "split_kernels.hpp"
#include "split2_kernels.hpp"
#include "dense64_kernels.hpp"
#include "multi_mfma_kernels.hpp"
#include "gain_basis_kernels.hpp"
#include "gain_time_basis_kernels.hpp"
#include "fit_quality_kernels.hpp"
#include "robust_weight_kernels.hpp"
#include "gain_solve_kernels.hpp"
#include "coeff_solve_kernels.hpp"
#include "fit_error_kernels.hpp"
#include "gain_error_kernels.hpp"
#include "delay_spectrum_kernels.hpp"
#include "delay_cross_kernels.hpp"
#include "delay_fringe_kernels.hpp"
#include "delay_coherent_kernels.hpp"
#include "delay_transfer_kernels.hpp"
#include "degeneracy_kernels.hpp"
#include "gain_basis_solve_kernels.hpp"
#include "gain_time_solve_kernels.hpp"
#include "gauss_newton_kernels.hpp"
#include "lbfgs_kernels.hpp"
#include "mixed_comps_kernels.hpp"
#include "solve_plan.hpp"  // (and problem_plan.hpp)
#include "step_plan.hpp"
#include "report_plan.hpp"
#include <cstdlib>
#include <dlfcn.h>
#include <type_traits>

using namespace calk;

namespace {

#define HIP_TRY(expr)                                                                                          \
  do {                                                                                                         \
    hipError_t _e = (expr);                                                                                    \
    if (_e != hipSuccess) return fail(CAL_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)
#define NCCL_TRY(expr)                                                                                         \
  do {                                                                                                         \
    ncclResult_t _e = (expr);                                                                                  \
    if (_e != ncclSuccess) return fail(CAL_ERR_RCCL, "%s failed: %s (%s:%d)", #expr, ncclGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)

// Zero fills of new allocations run on a non-blocking utility stream of the current device, never on the legacy stream: a
// hipMemset there synchronises with every other stream, and HIP refuses it ("operation would make the legacy stream depend on
// a capturing ... stream") while ANOTHER thread's solver captures its step graph -- which is what parallel_fits does.
static hipError_t zero_fill(void* p, size_t n) {
  static std::mutex mu;
  static std::map<int, hipStream_t> streams;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  hipStream_t st;
  {
    std::lock_guard<std::mutex> lock(mu);
    auto it = streams.find(dev);
    if (it == streams.end()) {
      e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
      if (e != hipSuccess) return e;
      streams[dev] = st;
    } else {
      st = it->second;
    }
  }
  e = hipMemsetAsync(p, 0, n, st);
  if (e != hipSuccess) return e;
  return hipStreamSynchronize(st);
}

// A solver counts its device memory (memory_bytes) over the DevBufs it is made of, without a list to keep: DevBufRegistry is SolverT's
// first base class, and every DevBuf constructed on this thread between its constructor and the body of SolverT's, which clears
// g_registering -- the solver's members, all of them -- enters its list.  A DevBuf made at any other time (a local of a member function)
// belongs to nobody.
struct DevBuf;
thread_local std::vector<const DevBuf*>* g_registering = nullptr;
struct DevBufRegistry {
  std::vector<const DevBuf*> bufs;
  DevBufRegistry() { g_registering = &bufs; }
};

struct DevBuf {  // owning device allocation
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() {
    if (g_registering) g_registering->push_back(this);
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  int alloc(size_t n, bool zero = true) {
    release();
    if (n == 0) n = 16;
    hipError_t e = hipMalloc(&p, n);
    if (e != hipSuccess) {
      p = nullptr;
      return fail(CAL_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", n, hipGetErrorString(e));
    }
    bytes = n;
    if (zero) {
      // complete before this returns: the solver works on its own non-blocking stream, and an unfinished fill could land on top
      // of a later upload
      e = zero_fill(p, n);
      if (e != hipSuccess) return fail(CAL_ERR_HIP, "zero fill of a new allocation failed: %s", hipGetErrorString(e));
    }
    return CAL_OK;
  }
  // at least n bytes: a new allocation only when there is none or it is too small (it never shrinks)
  int reserve(size_t n, bool zero = true) { return p && bytes >= n ? (int)CAL_OK : alloc(n, zero); }
  template <typename U> U* as() const { return reinterpret_cast<U*>(p); }
};

// roctx ranges around the chunks of a PROFILED run (n_profile_steps of the reference wraps its profiled steps in
// tf.profiler.experimental.Trace, calibration.py:681-687): rocprofv3 --marker-trace then shows "calamity: train steps [a, b)"
// over the kernels of each chunk.  The marker library is looked up at run time; without it the ranges are no-ops.
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    for (const char* name : {"librocprofiler-sdk-roctx.so", "libroctx64.so"}) {
      if (void* h = dlopen(name, RTLD_NOW | RTLD_LOCAL)) {
        push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (push && pop) return;
        push = nullptr;
        pop = nullptr;
      }
    }
  }
};
inline Roctx& roctx() {
  static Roctx r;
  return r;
}

inline int grid_for(long long n, int block = 256, int cap = 16384) {
  long long g = (n + block - 1) / block;
  return (int)std::max<long long>(1, std::min<long long>(g, cap));
}


}  // namespace

// ================================================================================================================
struct cal_solver {
  virtual ~cal_solver() {}
  int device = 0;
  int dtype = CAL_F32;
  virtual int set_problem(const cal_problem_desc* d) = 0;
  virtual int set_data(const void* dr, const void* di, const void* w) = 0;
  virtual int set_regularization(int mode, const double* pr, const double* pi, bool per_slice) = 0;
  virtual int slice_count() = 0;
  virtual int get_slice_losses(double* out) = 0;
  virtual int set_optimizer(const cal_optimizer_desc* d) = 0;
  virtual int set_params(const void* g_r, const void* g_i, const void* c_r, const void* c_i) = 0;
  virtual int get_params(int which, void* g_r, void* g_i, void* c_r, void* c_i) = 0;
  virtual int get_moments(void* gm_r, void* gm_i, void* gv_r, void* gv_i, void* cm_r, void* cm_i, void* cv_r, void* cv_i,
                          int64_t* t) = 0;
  virtual int set_moments(const void* gm_r, const void* gm_i, const void* gv_r, const void* gv_i, const void* cm_r,
                          const void* cm_i, const void* cv_r, const void* cv_i, int64_t t) = 0;
  virtual int eval(bool grads, double* loss, void* gg_r, void* gg_i, void* gc_r, void* gc_i) = 0;
  virtual int run(const cal_run_desc* r, double* losses_out, cal_run_result* res, bool per_slice) = 0;
  virtual int model(void* mr, void* mi, bool with_gains) = 0;
  virtual int fit_quality(const void* g_r, const void* g_i, double* chisq_ant, double* wsum_ant, double* chisq_bl, double* wsum_bl) = 0;
  virtual int robust_weights(const cal_robust_desc* d, double* scale_bl, double* ndown_bl) = 0;
  virtual int delay_spectrum(const cal_delay_spectrum_desc* d, const void* g_r, const void* g_i, double* power_bl, double* norm_bl, double* power_bin,
                             double* count_bin) = 0;
  virtual int set_delay_spectrum_scratch(int64_t bytes) = 0;
  virtual int delay_cross_spectrum(const cal_delay_cross_desc* d, const void* g_r, const void* g_i, double* cross_pair, double* diff_pair, double* norm_pair,
                                   double* cross_bin, double* diff_bin, double* count_bin) = 0;
  virtual int delay_fringe_spectrum(const cal_delay_fringe_desc* d, const void* g_r, const void* g_i, double* power_grp, double* norm_grp, double* power_bin,
                                    double* count_bin) = 0;
  virtual int delay_coherent_spectrum(const cal_delay_coherent_desc* d, const void* g_r, const void* g_i, double* power_grp, double* norm_grp, double* power_bin,
                                      double* count_bin) = 0;
  virtual int delay_transfer(const cal_delay_transfer_desc* d, const void* g_r, const void* g_i, double* absorbed_bl, double* noise_bl, double* absorbed_bin,
                             double* count_bin, cal_fit_errors_counts* counts) = 0;
  virtual int set_delay_transfer_scratch(int64_t bytes) = 0;
  virtual int fix_degeneracies(const cal_degeneracy_desc* d, double* params, double* nsamp, double* last_step, void* out_g_r, void* out_g_i, void* out_m_r,
                               void* out_m_i) = 0;
  virtual int get_weights(void* out, int which) = 0;
  virtual int solve_gains(const cal_gain_solve_desc* d) = 0;
  virtual int hold_slices(const uint8_t* mask) = 0;
  virtual int solve_coeffs(const cal_coeff_solve_desc* d, cal_coeff_solve_result* res) = 0;
  virtual int set_coeff_solve_scratch(int64_t bytes) = 0;
  virtual int fit_errors(double ridge, double* coeff_var, double* model_var, double* leverage_bl, double* nsamp_bl, double* gain_var,
                         cal_fit_errors_counts* counts) = 0;
  virtual int gain_basis_errors(double ridge, double* gain_var, double* y_var, double* gain_dof, cal_fit_errors_counts* counts) = 0;
  virtual int solve_gain_coeffs(const cal_gain_coeff_solve_desc* d, cal_gain_coeff_solve_result* res) = 0;
  virtual int normal_product(const void* p_g_r, const void* p_g_i, const void* p_c_r, const void* p_c_i, void* out_g_r, void* out_g_i, void* out_c_r,
                             void* out_c_i) = 0;
  virtual int gauss_newton_step(const cal_gauss_newton_desc* d, cal_gauss_newton_result* res) = 0;
  virtual int lbfgs(const cal_lbfgs_desc* d, double* losses_out, cal_lbfgs_result* res) = 0;
  virtual int solve_gain_time_coeffs(const cal_gain_time_solve_desc* d, cal_gain_time_solve_result* res) = 0;
  virtual int get_gain_coeff_moments(void* ym_r, void* ym_i, void* yv_r, void* yv_i, void* cm_r, void* cm_i, void* cv_r, void* cv_i, int64_t* t) = 0;
  virtual int init_coeffs(const void* sr, const void* si) = 0;
  virtual int synchronize() = 0;
  virtual int timing_enable(int e) = 0;
  virtual int timing_get(cal_kernel_timing* out) = 0;
  virtual int memory_bytes(int64_t* b) = 0;
  virtual int comm_init(const void* id, int rank, int nranks) = 0;
  virtual int set_launch_mode(int mode) = 0;
  virtual int set_exchange_hook(cal_exchange_fn fn, void* ctx, int rank, int nranks) = 0;
  virtual int comm_size(int* nranks_seen) = 0;
  virtual int set_gain_basis(const void* basis, int nvec) = 0;
  virtual int set_gain_time_basis(const void* basis_t, int ntimes, int nvec_t) = 0;
  virtual int get_gain_coeffs(int which, void* y_r, void* y_i) = 0;
  virtual int eval_gain_coeff_grads(double* loss, void* gy_r, void* gy_i) = 0;
};

template <typename T>
struct SolverT final : DevBufRegistry, cal_solver, PlanScalars {  // PlanScalars (problem_plan.hpp): what set-up decided about the problem
  using T2 = vec2_t<T>;
  hipStream_t stream = nullptr;
  // Synchronous copies go through the solver's OWN (non-blocking) stream, never the legacy stream: a copy there synchronises with
  // every other stream, and HIP refuses it ("operation would make the legacy stream depend on a capturing ... stream") while ANOTHER
  // thread's solver captures its step graph -- parallel_fits, the workers of a SliceBatchFitter.
  hipError_t copy_sync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, stream);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(stream);
  }
  bool has_problem = false, has_data = false, has_gains = false, has_coef = false, has_opt = false;
  // time slices
  DevBuf slice_coff, slice_ipart_ptr, slice_ipart_idx, slice_ppart_ptr, slice_ppart_idx, slice_cblk;
  std::vector<int> h_slice_coff, h_slice_cblk;
  std::vector<int> h_grp_coff;
  // device buffers
  DevBuf tiles, bl_tile, bl_ant, runs, items, ant_ptr, ant_ent, coef_grp, grp_coff, grp_item_ptr, item_goff;
  DevBuf data_r, data_i, wgts;
  DevBuf gains, gains_m, gains_v, gains_snap;  // [nants][fpad] T2
  DevBuf gains_alt;                            // one-launch tail (step_tail_kernel): gains are read from one buffer and written to the other; `gains` is always the current one
  DevBuf coef, coef_m, coef_v, coef_snap;      // [2][ncoef] T (r plane then i plane)
  DevBuf q0, q1, comm;                         // comm: r0 | r1 | r2 (gain gradient parts), contiguous for the all-reduce
  DevBuf scal;                                 // [nslices] x 4 doubles: loss, s_r, s_i, spare
  DevBuf gcp0, gcp1, gc0, gc1;                 // coefficient-gradient partials and (multi-item groups) their sums
  DevBuf part, state, losses, scratch, model_buf;
  DevBuf gs_out, gs_ptr, gs_ent, gs_mask;      // solve_gains: num_r | num_i | den ([3][nants][nfreqs] doubles, the exchange payload); the antenna lists without autocorrelations; [nslices] mask bytes
  // what the plans of the closed-form calls are made from (solve_plan.hpp), as set_problem's plan held it on the host
  std::vector<CsGroup> h_cs_grp;
  std::vector<long long> h_bl_tile;
  std::vector<int2> h_bl_ant;
  // solve_coeffs (coeff_solve_kernels.hpp): the groups with its plan's offsets, order, work list and chunks (the first call), N of a
  // chunk of groups in T (cs_n) and its factor in double (cs_d), rhs [2][ncoef] T, the two counters
  DevBuf cs_grp, cs_order, cs_work, cs_n, cs_d, cs_rhs, cs_cnt;
  std::vector<GroupChunk> cs_chunks;
  int64_t cs_bound = kCsScratchDefault;        // bytes of scratch a chunk of any closed-form call may take (set_coeff_solve_scratch)
  // fit_errors (fit_error_kernels.hpp): a plan of its own (the chunks also hold W, so they are cut elsewhere than solve_coeffs'): the
  // groups with this plan's offsets, order, Gram work list, W offsets, the leverage kernel's work list; per chunk N (fe_n), the factor
  // (fe_d) and W (fe_w); rhs of the Gram kernel (unused), ok [ngrps] ints + the two counters (fe_ok), the partial sums
  // [nbls][slots] (fe_part), the outputs coeff_var | leverage_bl | nsamp_bl (fe_out) and, only when asked for, model_var (fe_mv)
  DevBuf fe_grp, fe_order, fe_work, fe_woff, fe_lwork, fe_n, fe_d, fe_w, fe_rhs, fe_ok, fe_part, fe_out, fe_mv;
  std::vector<GroupChunk> fe_chunks;
  int fe_npieces = 0;
  // The projected gain systems of solve_gain_coeffs, solve_gain_time_coeffs and gain_basis_errors (gain_basis_solve_kernels.hpp,
  // gain_time_solve_kernels.hpp, gain_error_kernels.hpp), one set for the three (reserve_gain_systems sizes it from a call's RowChunks,
  // enqueue_gain_systems fills it), per chunk of rows (antenna rows; antennas under a time basis): M_{t,a} [T][ca][K][K] T of a time
  // basis over a frequency basis (pg_m), N_a [ca][n][n] T (pg_n) and under both bases rhs_a [ca][2][n] T (pg_rhsa), the factor in double
  // where it leaves LDS or, without a frequency basis, the channel systems beyond kTimeTile vectors (pg_d); the per-row right-hand sides
  // [nants][2][K] T (pg_rhs) and the two counters of a sweep (pg_cnt).  The chunks share cs_bound.
  DevBuf pg_m, pg_n, pg_rhsa, pg_d, pg_rhs, pg_cnt;
  // gain_basis_errors' own, beside the set above: W [rows][np][np] T (gbe_w), ok [y_rows] and the two counters (gbe_ok), the outputs
  // gain_var | y_var | gain_dof | the channels' dof of a time basis alone, doubles (gbe_out)
  DevBuf gbe_w, gbe_ok, gbe_out;
  std::vector<uint8_t> held;                   // hold_slices: [nslices], 1 = the slice enters every later run as stopped (empty: none)
  DevBuf fq_out, fq_gains;                     // fit_quality: chisq_ant | wsum_ant ([nants][nfreqs] doubles each, the exchange payload) | chisq_bl | wsum_bl; gains given for one evaluation
  DevBuf rw_w0, rw_out;                        // robust_weights: w0, the weights as set_data gave them (first call after a set_data); scale_bl | ndown_bl ([nbls] doubles each)
  bool rw_w0_valid = false;
  // delay_spectrum (delay_spectrum_kernels.hpp): the operator image and norm_f of a call, the bins' sorted row lists and their pieces per chunk;
  // a chunk's masked planes in T (ds_x) and power in double (ds_pow); norm_bl | power_bin | count_bin (ds_out; the last two are the exchange payload)
  DevBuf ds_op, ds_normf, ds_ent, ds_ptr, ds_x, ds_pow, ds_out;
  int64_t ds_bound = kCsScratchDefault;        // bytes of scratch a chunk of rows may take (set_delay_spectrum_scratch)
  // delay_cross_spectrum (delay_cross_kernels.hpp) reuses them all, with chunks of pairs; the pairs and their scales of a call
  DevBuf dc_pairs, dc_scale;
  // delay_fringe_spectrum (delay_fringe_kernels.hpp) reuses them all as well, with chunks of whole groups: the rows of the groups in
  // dc_pairs, their scales in dc_scale, Y and then the power in ds_pow; opt_r | opt_i of a call
  DevBuf df_opt;
  // delay_coherent_spectrum (delay_coherent_kernels.hpp) reuses those of the fringe call from the averaged planes on; the member lists
  // of a call (set_ptr, rows, coefficients, conjugation flags) and a chunk's set masks
  DevBuf dk_ptr, dk_row, dk_wgt, dk_conj, dk_mask;
  // delay_transfer (delay_transfer_kernels.hpp): the plan of a call (groups, order, Gram work, W offsets, runs, rows, the bins' lists and
  // the operator image); per chunk N (dt_n), the factor (dt_d) and W | S (dt_x); rhs of the Gram kernel (unused), coeff_var of the factor
  // kernel (unused), ok [ngrps] ints + the two counters; absorbed and noise [nbls][ndelays]; valid | absorbed_bin | count_bin (dt_out; the
  // last two are the exchange payload)
  DevBuf dt_grp, dt_order, dt_work, dt_woff, dt_runs, dt_rows, dt_ent, dt_ptr, dt_op, dt_n, dt_d, dt_x, dt_rhs, dt_cv, dt_ok, dt_abs, dt_noise, dt_out;
  int64_t dt_bound = kCsScratchDefault;        // bytes of scratch a chunk of groups may take (set_delay_transfer_scratch)
  // fix_degeneracies (degeneracy_kernels.hpp): the reference planes, then z0 ([2][nbls][fpad] T); the reference's weights when given
  // ([nbls][fpad] T); d_b | the slice's antenna positions | nu_f / nu_ref | the slices' longest |d_b| (doubles); the slices' row lists |
  // first segments | segments (ints); the segments' partial sums ([8][nseg][fpad] doubles); the channels' state ([14][nsl][fpad] + [nsl][2]
  // doubles); g' and gref ([nants][fpad] T2 each)
  DevBuf dg_z, dg_w, dg_geo, dg_idx, dg_part, dg_st, dg_gout, dg_gref;
  // normal_product / gauss_newton_step (gauss_newton_kernels.hpp), vectors over the flat parameter space (gn_np() elements): the direction s, the
  // gradient of G m and the saved parameters in T; the solution x, the residual, N s and D in double.  gn_m: m = A c, gn_sd: the data planes while
  // they are substituted ([2][nbls][fpad] T each); gn_rows: the rows' sums (3 nbls doubles); the dot products' partials, the slices' scalars and
  // damping, the groups as gn_precond_coeff_kernel sees them, the first baseline row of every slice ([nslices + 1] ints)
  DevBuf gn_s, gn_g0, gn_save, gn_x, gn_res, gn_ns, gn_D, gn_m, gn_sd, gn_rows, gn_part, gn_scal, gn_lam, gn_grp, gn_rowptr;
  // lbfgs (lbfgs_kernels.hpp): 2 history + 4 vectors of T over the variable space (the ring of history + 1 slots of (s, y), x_k, g_k), the
  // dot products' block partials and sums, the slices' state, their recorded losses, the integer the host reads per trial round
  DevBuf lb_vec, lb_part, lb_dots, lb_state, lb_losses, lb_count;
  DevBuf members, heads;                       // baselines that share tiles (bl_alias): member lists of the head items, head item indices
  bool heads_one_pass = false;                 // the regularised step of the heads in ONE pass (all of them on fused_multi_mfma_kernel<.., REG = 2>)
  bool reg_prepass = false;                    // the regularised gradient pass is preceded by a loss pass and the slices' alpha (enqueue_pass);
                                               // with a communicator agreed over the ranks: if one rank needs it, every rank runs it
  // dense (MFMA) path of the SHARED layout, fp32, one baseline per fitting group
  DevBuf mf_ops, mf_panels;                    // mf_ops: every basis block's packed MFMA operands (see mfma_pack_kernel / mfma_pack64_kernel)
  DevBuf mf_map;                               // [mf_grid] workgroup -> panel (-1: empty slot): XCD-affine dispatch of the dense launch
  // small problems: a train step is two launches (fused pass, step_tail_kernel), replayed kGraphSteps at a time from a hipGraph (step_plan.hpp)
  int launch_mode = CAL_LAUNCH_AUTO;
  hipGraphExec_t graph_exec = nullptr;
  struct GraphKey {
    int optimizer, freeze, reg, losses_cap, st_par, tail, nsteps;
    const void *gains, *snap, *losses;
    const void *y, *ysnap;  // gain basis: the coefficient arrays the captured update and gain_expand_kernel work on (null without one)
    const void *tz, *tpf;   // time basis over a frequency basis: what the two time kernels hand to / take from the frequency kernels
    bool operator==(const GraphKey& o) const {
      return optimizer == o.optimizer && freeze == o.freeze && reg == o.reg && losses_cap == o.losses_cap && st_par == o.st_par && tail == o.tail &&
             nsteps == o.nsteps && gains == o.gains && snap == o.snap && losses == o.losses && y == o.y && ysnap == o.ysnap && tz == o.tz && tpf == o.tpf;
    }
  } graph_key{};
  DevBuf agree_buf;
  DevState* h_state = nullptr;                 // pinned mirror: [nslices]
  int h_state_cap = 0;
  int st_par = 0;                              // which half of `state` ([2][nslices]) is current
  DevState* st_cur() { return state.as<DevState>() + (size_t)st_par * nslices; }
  DevState* st_nxt() { return state.as<DevState>() + (size_t)(st_par ^ 1) * nslices; }
  std::vector<double> prior_r_t, prior_i_t;    // per slice
  // which slice every kernel's work belongs to (fit_kernels.hpp: SliceMap); the loss partials are per item (general kernels) or
  // per panel (dense kernels)
  SliceMap smap(bool panels) const {
    SliceMap m{};
    m.coff = slice_coff.as<int>();
    m.nslices = nslices;
    m.na_slice = na_slice;
    if (nslices > 1) {
      m.part_ptr = (panels ? slice_ppart_ptr : slice_ipart_ptr).template as<int>();
      m.part_idx = (panels ? slice_ppart_idx : slice_ipart_idx).template as<int>();
    }
    return m;
  }
  // settings
  cal_optimizer_desc opt{CAL_OPT_ADAMAX, 1e-3, 0.9, 0.999, 1e-7, 0.9, 0.0, 0.1, 0, 0, -0.5, 0.0, 0.0, 0.0, 0.0, 0.0};
  // LAMB: the optimizer's variables (g_r, g_i of every slice; the coefficient runs of every (slice, cal_problem_desc::grp_var) per plane)
  DevBuf lamb_vars, lamb_cvar_ptr, lamb_partial, lamb_ratio;
  // ... over several ranks: a coefficient variable (slice t, grp_var w) is spread over the ranks that own its groups -> its two sums of
  // squares are all-reduced in slot t * lamb_nv + w of lamb_glob (the gain variables are replicated: every rank already holds their norms)
  DevBuf lamb_glob, lamb_slot;
  std::vector<int> lamb_cvar_slice, lamb_cvar_id;
  int lamb_nv = 0;
  int reg = CAL_REG_NONE;
  // gain basis (set_gain_basis; gain_basis_kernels.hpp): gains = gb_g0 + B y.  The optimizer's gain variables are then y ([nants][gb_kpad]
  // (re, im), like the gains with row length gb_kpad), its gradient the projected planes gb_proj (p0 | p1 | p2, contiguous for the all-reduce)
  int gb_nvec = 0, gb_kpad = 0;
  DevBuf gb_B, gb_Bt;                          // [fpad][gb_kpad] and [gb_kpad][fpad], zero-padded
  DevBuf gb_g0, gb_y, gb_ym, gb_yv, gb_ysnap, gb_proj;
  bool gb_on() const { return gb_nvec > 0; }
  // gain time basis (set_gain_time_basis; gain_time_basis_kernels.hpp): the solver's nants = tb_T tb_na rows are tb_T times of tb_na antennas,
  // gains = gb_g0 + Bt (x) (B) y.  y, its moments, snapshot and gradient planes live in the gb_ buffers above, [tb_na][tb_L][W] complex with
  // W = gb_kpad or, without a frequency basis, fpad.  With both bases tb_pf holds gain_project_kernel's planes ([3][nants][gb_kpad]) and
  // tb_z what gain_expand_kernel expands ([nants][gb_kpad]).
  int tb_T = 0, tb_L = 0, tb_lpad = 0, tb_tpad = 0, tb_na = 0;
  DevBuf tb_B, tb_Bt;                          // [tb_T][tb_lpad] and [tb_L][tb_tpad], zero-padded
  DevBuf tb_z, tb_pf;
  bool tb_on() const { return tb_L > 0; }
  bool yb_on() const { return gb_on() || tb_on(); }                 // the optimizer's gain variables are y
  int y_w() const { return gb_on() ? gb_kpad : fpad; }               // W
  int y_cols() const { return gb_on() ? gb_nvec : nfreqs; }          // ... and its unpadded length
  int y_rows() const { return tb_on() ? tb_na : nants; }
  long long y_row() const { return (long long)(tb_on() ? tb_L : 1) * y_w(); }  // complex elements per row of y
  // timing
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
  size_t ev_used = 0;
  long long t_launches = 0;
  double t_total_ms = 0;
  // comm
  ncclComm_t nccl = nullptr;
  int nranks = 1, rank = 0;
  // caller-supplied exchange (cal_solver_set_exchange_hook): the same buffers and counts RCCL would reduce, staged through
  // pinned host memory and reduced by the callback
  cal_exchange_fn hook = nullptr;
  void* hook_ctx = nullptr;
  void* hook_buf = nullptr;
  size_t hook_bytes = 0;
  bool comm_on() const { return nccl != nullptr || hook != nullptr; }

  SolverT() { g_registering = nullptr; }  // every member DevBuf is in bufs by now
  ~SolverT() override {
    (void)hipSetDevice(device);
    if (nccl) (void)ncclCommDestroy(nccl);
    if (hook_buf) (void)hipHostFree(hook_buf);
    if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
    for (auto& e : ev_pool) {
      (void)hipEventDestroy(e.first);
      (void)hipEventDestroy(e.second);
    }
    if (h_state) (void)hipHostFree(h_state);
    if (stream) (void)hipStreamDestroy(stream);
  }

  int init() {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    CAL_TRY(size_state(1));
    return CAL_OK;
  }
  // loop state, reduced sums and their host mirror for n time slices (a new problem may change the count)
  int size_state(int n) {
    if (n > h_state_cap) {
      if (h_state) (void)hipHostFree(h_state);
      h_state = nullptr;
      h_state_cap = 0;
      HIP_TRY(hipHostMalloc((void**)&h_state, (size_t)n * sizeof(DevState), hipHostMallocDefault));
      h_state_cap = n;
    }
    memset(h_state, 0, (size_t)n * sizeof(DevState));
    CAL_TRY(state.alloc(2 * (size_t)n * sizeof(DevState)));  // double-buffered: see step_update_kernel
    CAL_TRY(scal.alloc(4 * (size_t)n * sizeof(double)));
    st_par = 0;
    prior_r_t.assign(n, 0.0);
    prior_i_t.assign(n, 0.0);
    for (int t = 0; t < n; ++t) reset_loop_state(h_state[t]);
    return CAL_OK;
  }
  static void reset_loop_state(DevState& h) {  // a new fit begins: loop state of calibration.py:573-574
    h.t = 0;
    h.b1t = h.b2t = 1.0;
    h.nadam_sched = 1.0;
    h.min_loss = 9e99;
    h.prev_loss = 0;
    h.n_recorded_total = 0;
    h.nonfinite = 0;
  }

  // ------------------------------------------------------------------------------------------------------------
  // With a communicator attached, every decision a rank takes from its OWN shard and that changes what it exchanges must
  // be taken by all ranks together -- and a rank whose set-up fails must not leave the others waiting in a collective.
  // So the rank-local part (validation, eligibility, every allocation and upload: set_problem_local) contains no collective
  // at all, and ONE agreement follows it on every path, failure included: the minimum over ranks of
  // {set-up ok ? kernel plan : -1, steps per host synchronisation, ...} (agree_problem).  A negative minimum fails the call
  // on every rank; a rank that built the dense path while another could not drops back to the general kernels (same buffers);
  // ranks whose problems differ in shape (nants, fpad, nslices, dtype) all fail with CAL_ERR_INVALID.
  int set_problem(const cal_problem_desc* d) override {
    const int rc = set_problem_local(d);
    if (!comm_on()) return rc;
    return agree_problem(rc);
  }
  // the agreement: FOUR ints, minimum over the ranks (the exchange a set-up issues, pinned by tests/test_gpu_exchange_hook.py):
  //   v[0] = set-up failed ? -1 : 4 * shape + plan, plan = 0: general kernels with the loss pre-pass of the regularised step,
  //          1: general kernels without it, 2: dense kernels built.  The plans form a chain -- heads (STREAM layout) and the dense
  //          kernels (SHARED layout) exclude each other, so "dense built" implies "no pre-pass" -- and the minimum of a chain is
  //          both "every rank built the dense kernels" and "no rank needs the pre-pass"
  //   v[1] = steps per host synchronisation (1 .. 256)
  //   v[2] = LAMB possible ? -(variables per slice) : -2^30
  //   v[3] = -shape
  // shape (< 2^27) = (nslices - 1) << 19 | f64 << 18 | 18-bit hash of (nants, fpad): min(shape) == -min(-shape) only if every
  // rank holds the same one (nslices and dtype compared exactly, nants and fpad through the hash)
  static int shape_code(int na, int fp, int nsl) {
    uint32_t h = 2166136261u;  // FNV-1a over the two words
    for (uint32_t w : {(uint32_t)na, (uint32_t)fp})
      for (int k = 0; k < 4; ++k) h = (h ^ ((w >> (8 * k)) & 0xffu)) * 16777619u;
    return (nsl - 1) << 19 | (sizeof(T) == 8 ? 1 : 0) << 18 | (int)((h ^ (h >> 18)) & 0x3ffffu);
  }
  int agree_problem(int rc) {
    const std::string msg = g_err;
    int local_nv = 0;
    for (int w : lamb_cvar_id) local_nv = std::max(local_nv, w + 1);
    const bool ok = rc == CAL_OK;
    const int shape = ok ? shape_code(nants, fpad, nslices) : 0;
    const int plan = mf_ok ? 2 : (nheads == 0 || heads_one_pass_local) ? 1 : 0;
    int v[4] = {ok ? 4 * shape + plan : -1, ok ? steps_per_sync : (1 << 30), ok && lamb_ok ? -local_nv : -(1 << 30), -shape};
    const int arc = agree_ints(v, 4, CAL_XCHG_MIN);
    if (arc != CAL_OK) {
      has_problem = false;
      return arc;
    }
    if (rc != CAL_OK) {
      g_err = msg;
      return rc;
    }
    if (v[0] < 0) {
      has_problem = false;
      return fail(CAL_ERR_STATE, "set_problem failed on another rank of the communicator");
    }
    const int lo = v[0] >> 2, hi = -v[3];
    if (lo != hi) {
      has_problem = false;
      const char* what = (lo >> 19) != (hi >> 19) ? "nslices" : ((lo >> 18) & 1) != ((hi >> 18) & 1) ? "the fit dtype" : "nants or fpad";
      return fail(CAL_ERR_INVALID, "set_problem: the ranks of the communicator disagree on %s (this rank: nants %d, fpad %d, nslices %d, %d-byte reals)",
                  what, nants, fpad, nslices, (int)sizeof(T));
    }
    const int agreed_plan = v[0] & 3;
    if (agreed_plan < 2) mf_ok = false;
    // the "sum" regulariser over heads: a rank that runs the loss pre-pass exchanges the slices' sums once more per step, so if
    // one rank needs it every rank runs it (its heads then take the two-pass form, REG == 1, and its S partials join the sum)
    heads_one_pass = heads_one_pass_local && agreed_plan >= 1;
    reg_prepass = agreed_plan == 0;
    steps_per_sync = v[1];
    lamb_ok = lamb_ok && v[2] > -(1 << 30);
    lamb_nv = lamb_ok ? -v[2] : 0;
    if (lamb_ok) {
      std::vector<int> slot(std::max(lamb_ncvar, 1), 0);
      for (int k = 0; k < lamb_ncvar; ++k) slot[k] = lamb_cvar_slice[k] * lamb_nv + lamb_cvar_id[k];
      CAL_TRY(upload(lamb_slot, slot));
      CAL_TRY(lamb_glob.alloc((size_t)std::max(1, 2 * nslices * lamb_nv) * 2 * sizeof(double)));
    }
    return CAL_OK;
  }
  // Set-up is three steps: reset, plan (problem_plan.hpp: every decision, on the host alone), upload.
  int set_problem_local(const cal_problem_desc* d) {
    HIP_TRY(hipSetDevice(device));
    has_problem = has_data = has_gains = has_coef = false;
    rw_w0_valid = false;
    drop_graph();
    release_gain_basis();  // a new problem fits per channel until a basis is set again
    ProblemPlan<T> p;
    CAL_TRY(plan_problem(d, p));
    return upload_plan(d, p);
  }
  // allocation of max(v.size(), min_count) elements (not zeroed) + synchronous copy on the solver's stream
  template <typename X>
  int upload(DevBuf& b, const std::vector<X>& v, size_t min_count = 0, bool sync = true) {
    CAL_TRY(b.alloc(std::max(v.size(), min_count) * sizeof(X), false));
    if (v.empty()) return CAL_OK;
    HIP_TRY(hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(X), hipMemcpyHostToDevice, stream));
    if (sync) HIP_TRY(hipStreamSynchronize(stream));
    return CAL_OK;
  }
  int upload_plan(const cal_problem_desc* d, const ProblemPlan<T>& p) {
    static_cast<PlanScalars&>(*this) = p;
    local_reg_plan();
    lamb_cvar_slice = p.lamb_cvar_slice; lamb_cvar_id = p.lamb_cvar_id;
    h_grp_coff = p.grp_coff; h_slice_coff = p.slice_coff; h_slice_cblk = p.slice_cblk; h_cs_grp = p.cs_grp; h_bl_tile = p.bl_tile; h_bl_ant = p.bl_ant;
    CAL_TRY(size_state(nslices));
    CAL_TRY(upload(slice_coff, p.slice_coff));
    CAL_TRY(upload(lamb_vars, p.lamb_vars));
    CAL_TRY(upload(lamb_cvar_ptr, p.lamb_cvar_ptr));
    CAL_TRY(lamb_partial.alloc((size_t)lamb_nvar * kLambSeg * 2 * sizeof(double)));
    CAL_TRY(lamb_ratio.alloc((size_t)lamb_nvar * sizeof(double)));

    // ---- unique basis blocks -> tile-major device layout
    DevBuf raw, utiles;
    const size_t raw_bytes = (size_t)d->basis_offset[p.nbasis] * sizeof(T);
    CAL_TRY(raw.alloc(raw_bytes, false));
    HIP_TRY(hipMemcpyAsync(raw.p, d->basis_data, raw_bytes, hipMemcpyHostToDevice, stream));
    // (+ a zeroed pad: fused_multi_mfma_kernel reads on past the last rows of a tile, against zero coefficients)
    CAL_TRY(utiles.alloc(((size_t)p.uoff.back() + kMmTilePadElems) * sizeof(T), false));
    HIP_TRY(hipMemsetAsync(utiles.as<T>() + p.uoff.back(), 0, kMmTilePadElems * sizeof(T), stream));
    for (int u = 0; u < p.nbasis; ++u) {
      const long long n = p.uoff[u + 1] - p.uoff[u];
      if (n == 0) continue;
      // (folded: channels [0, nfreqs / 2) of the block's only row block: whole tiles, no padding)
      hipLaunchKernelGGL(retile_kernel<T>, dim3(grid_for(n)), dim3(256), 0, stream, raw.as<T>() + d->basis_offset[u], utiles.as<T>() + p.uoff[u],
                         fold ? p.ftile : nfreqs, fold ? p.ftile : fpad, d->basis_nvec[u], fold ? 1 : d->basis_nrowblk[u], p.fb_u[u]);
    }
    HIP_TRY(hipGetLastError());
    if (layout == CAL_LAYOUT_SHARED) {  // the baselines read the unique blocks themselves
      HIP_TRY(hipStreamSynchronize(stream));
      tiles.release();
      tiles.p = utiles.p; tiles.bytes = utiles.bytes;
      utiles.p = nullptr; utiles.bytes = 0;
    } else {
      CAL_TRY(tiles.alloc(((size_t)p.tiles_elems + kMmTilePadElems) * sizeof(T), false));
      HIP_TRY(hipMemsetAsync(tiles.as<T>() + p.tiles_elems, 0, kMmTilePadElems * sizeof(T), stream));
      DevBuf djobs;
      CAL_TRY(upload(djobs, p.jobs, 0, false));
      hipLaunchKernelGGL(tile_copy_kernel<T>, dim3((unsigned)p.jobs.size()), dim3(256), 0, stream, utiles.as<T>(), tiles.as<T>(), djobs.as<CopyJob>());
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipStreamSynchronize(stream));
    }
    // ---- dense path: every block's packed MFMA operands, the panel records, the workgroup -> panel map
    if (p.mf_ok) {
      CAL_TRY(mf_ops.alloc((size_t)p.op_off.back(), false));
      for (int u = 0; u < p.nbasis; ++u) {
        unsigned char* dst = mf_ops.as<unsigned char>() + p.op_off[u];
        const long long bytes = p.op_off[u + 1] - p.op_off[u];
        if constexpr (std::is_same<T, float>::value) {
          const float* src = raw.as<float>() + d->basis_offset[u];
          const int nv = d->basis_nvec[u];
          if (mf_split2)
            hipLaunchKernelGGL(split2_pack_kernel, dim3(grid_for((long long)fpad * 256)), dim3(256), 0, stream, src, dst, nfreqs, fpad, nv);
          else if (mf_split)
            hipLaunchKernelGGL(split_pack_kernel, dim3(grid_for(bytes / 6)), dim3(256), 0, stream, src, reinterpret_cast<unsigned short*>(dst), nfreqs, fpad,
                               nv, 0, (nv + 31) / 32);
          else
            hipLaunchKernelGGL(mfma_pack_kernel, dim3(grid_for(bytes / 4)), dim3(256), 0, stream, src, reinterpret_cast<float*>(dst), nfreqs, fpad, nv,
                               (nv + 31) / 32 * 32);
        } else {
          hipLaunchKernelGGL(mfma_pack64_kernel, dim3(grid_for(bytes / 8)), dim3(256), 0, stream, raw.as<double>() + d->basis_offset[u],
                             reinterpret_cast<double*>(dst), nfreqs, fpad, d->basis_nvec[u]);
        }
      }
      HIP_TRY(hipGetLastError());
      if (nslices > 1) {
        CAL_TRY(upload(slice_ppart_ptr, p.slice_ppart_ptr, 0, false));
        CAL_TRY(upload(slice_ppart_idx, p.slice_ppart_idx, 0, false));
        HIP_TRY(hipStreamSynchronize(stream));
      }
      CAL_TRY(upload(mf_panels, p.panels, 0, false));
      CAL_TRY(upload(mf_map, p.panel_map, 0, false));
      HIP_TRY(hipStreamSynchronize(stream));
    }
    raw.release();
    CAL_TRY(upload(bl_tile, p.bl_tile));
    release_coeff_solve();
    CAL_TRY(upload(bl_ant, p.bl_ant));
    CAL_TRY(upload(runs, p.runs, 1));
    if (nslices > 1) {
      CAL_TRY(upload(slice_ipart_ptr, p.slice_ipart_ptr));
      CAL_TRY(upload(slice_ipart_idx, p.slice_ipart_idx));
      CAL_TRY(upload(slice_cblk, p.slice_cblk));
    }
    members.release();
    heads.release();
    if (nheads > 0) {
      CAL_TRY(upload(members, p.members));
      CAL_TRY(upload(heads, p.heads));
    }
    // the dynamic LDS every kernel of this problem may ask for
    constexpr bool f32 = std::is_same<T, float>::value;
    const bool multi = nheads > nheads_mfma, mm = nheads > 0 && nheads_mfma > 0;
    const struct { bool on; const void* fn; size_t lds; } attrs[] = {
        {mf_ok && mf_split2, reinterpret_cast<const void*>(&fused_dense_split2_kernel<true>), mf_lds_grad[0]},
        {mf_ok && mf_split2, reinterpret_cast<const void*>(&fused_dense_split2_kernel<false>), mf_lds_loss[0]},
        {mf_ok && mf_split && !mf_split2, reinterpret_cast<const void*>(&fused_dense_split_kernel<true>), mf_lds_grad[0]},
        {mf_ok && mf_split && !mf_split2, reinterpret_cast<const void*>(&fused_dense_split_kernel<false>), mf_lds_loss[0]},
        {mf_ok && f32 && !mf_split, reinterpret_cast<const void*>(&fused_dense_kernel<true>), mf_lds_grad[0]},
        {mf_ok && f32 && !mf_split, reinterpret_cast<const void*>(&fused_dense_kernel<false>), mf_lds_loss[0]},
        {mf_ok && !f32, reinterpret_cast<const void*>(&fused_dense64_kernel<true>), mf_lds_grad[0]},
        {mf_ok && !f32, reinterpret_cast<const void*>(&fused_dense64_kernel<false>), mf_lds_loss[0]},
        {multi, reinterpret_cast<const void*>(&fused_multi_kernel<T, MODE_GRAD, false>), lds_multi_bytes},
        {multi, reinterpret_cast<const void*>(&fused_multi_kernel<T, MODE_LOSS, false>), lds_multi_bytes},
        {multi, reinterpret_cast<const void*>(&fused_multi_kernel<T, MODE_GRAD, true>), lds_multi_bytes},
        {multi, reinterpret_cast<const void*>(&fused_multi_kernel<T, MODE_LOSS, true>), lds_multi_bytes},
        {mm, reinterpret_cast<const void*>(&fused_multi_mfma_kernel<T, MODE_GRAD, 0>), lds_multi_mfma_bytes},
        {mm, reinterpret_cast<const void*>(&fused_multi_mfma_kernel<T, MODE_LOSS, 0>), lds_multi_mfma_bytes},
        {mm, reinterpret_cast<const void*>(&fused_multi_mfma_kernel<T, MODE_GRAD, 1>), lds_multi_mfma_bytes},
        {mm, reinterpret_cast<const void*>(&fused_multi_mfma_kernel<T, MODE_LOSS, 1>), lds_multi_mfma_bytes},
        {mm, reinterpret_cast<const void*>(&fused_multi_mfma_kernel<T, MODE_GRAD, 2>), lds_multi_mfma_bytes},
    };
    for (const auto& a : attrs)
      if (a.on) HIP_TRY(hipFuncSetAttribute(a.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.lds));
    CAL_TRY(upload(items, p.items));
    if (!gc_direct) {
      CAL_TRY(upload(coef_grp, p.coef_grp));
      CAL_TRY(upload(grp_coff, p.grp_coff));
      CAL_TRY(upload(grp_item_ptr, p.grp_item_ptr));
      CAL_TRY(upload(item_goff, p.item_goff));
      CAL_TRY(gc0.alloc(2 * (size_t)ncoef * sizeof(T)));
    }
    CAL_TRY(upload(ant_ptr, p.ant_ptr));
    CAL_TRY(upload(ant_ent, p.ant_ent));

    for (DevBuf* b : {&gains_snap, &gains_alt, &coef_snap, &q1, &gcp1, &gc1, &model_buf, &scratch, &fq_out, &fq_gains, &gs_out, &gs_ptr, &gs_ent, &gs_mask, &cs_rhs, &rw_w0, &rw_out, &ds_op, &ds_normf, &ds_ent, &ds_ptr, &ds_x, &ds_pow, &ds_out, &dc_pairs, &dc_scale, &df_opt, &dk_ptr, &dk_row, &dk_wgt, &dk_conj, &dk_mask, &dt_grp, &dt_order, &dt_work, &dt_woff, &dt_runs, &dt_rows, &dt_ent, &dt_ptr, &dt_op, &dt_n, &dt_d, &dt_x, &dt_rhs, &dt_cv, &dt_ok, &dt_abs, &dt_noise, &dt_out, &dg_z, &dg_w, &dg_geo, &dg_idx, &dg_part, &dg_st, &dg_gout, &dg_gref,
                       &gn_s, &gn_g0, &gn_save, &gn_x, &gn_res, &gn_ns, &gn_D, &gn_m, &gn_sd, &gn_rows, &gn_part, &gn_scal, &gn_lam, &gn_grp, &gn_rowptr,
                       &lb_vec, &lb_part, &lb_dots, &lb_state, &lb_losses, &lb_count})
      b->release();
    // ---- state arrays
    const size_t rowbytes = (size_t)(nbls + 1) * fpad * sizeof(T);  // + one all-zero spare row (padding slots of the dense path)
    const size_t gbytes = (size_t)nants * fpad * sizeof(T2), cbytes = 2 * (size_t)ncoef * sizeof(T);
    // (coef + 256: the split-bf16 kernel reads whole pairs of 16-vector steps, up to 31 reals past the last group's coefficients)
    const std::pair<DevBuf*, size_t> zeroed[] = {{&data_r, rowbytes}, {&data_i, rowbytes}, {&wgts, rowbytes}, {&gains, gbytes}, {&gains_m, gbytes}, {&gains_v, gbytes},
                                                 {&coef, cbytes + 256}, {&coef_m, cbytes}, {&coef_v, cbytes}, {&q0, (size_t)(nbls + 1) * fpad * sizeof(T2)}, {&comm, 3 * gbytes},
                                                 {&gcp0, 2 * (size_t)gcp_len * sizeof(T)}, {&part, (size_t)std::max(nitems, mf_npanels) * 4 * sizeof(double)}};
    for (const auto& z : zeroed) CAL_TRY(z.first->alloc(z.second));
    held.clear();
    has_problem = true;
    reg = CAL_REG_NONE;
    return CAL_OK;
  }

  // one in-place all-reduce over the ranks of the job, on the solver's stream: RCCL, or the caller's exchange hook (the
  // stream is drained, the buffer staged through pinned host memory, reduced by the callback and copied back)
  int all_reduce(void* dev, size_t count, int dtype_code, int op) {
    if (nccl) {
      const ncclDataType_t dt = dtype_code == CAL_XCHG_F32 ? ncclFloat : dtype_code == CAL_XCHG_F64 ? ncclDouble : ncclInt32;
      NCCL_TRY(ncclAllReduce(dev, dev, count, dt, op == CAL_XCHG_MIN ? ncclMin : ncclSum, nccl, stream));
      return CAL_OK;
    }
    if (!hook) return CAL_OK;
    const size_t bytes = count * (dtype_code == CAL_XCHG_F64 ? 8 : 4);
    if (hook_bytes < bytes) {
      if (hook_buf) (void)hipHostFree(hook_buf);
      hook_buf = nullptr;
      hook_bytes = 0;
      HIP_TRY(hipHostMalloc(&hook_buf, bytes, hipHostMallocDefault));
      hook_bytes = bytes;
    }
    HIP_TRY(hipMemcpyAsync(hook_buf, dev, bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const int rc = hook(hook_ctx, hook_buf, (int64_t)count, dtype_code, op);
    if (rc != 0) return fail(CAL_ERR_RCCL, "the exchange hook returned %d", rc);
    HIP_TRY(hipMemcpyAsync(dev, hook_buf, bytes, hipMemcpyHostToDevice, stream));
    return CAL_OK;
  }
  // how the regularised step runs as far as this rank's own problem goes (no communicator; agree_problem may change it)
  void local_reg_plan() {
    heads_one_pass = heads_one_pass_local;
    reg_prepass = nheads > 0 && !heads_one_pass_local;
  }
  // a few ints reduced over the ranks of the communicator: the minimum (set-up decisions that every rank must take identically) or the sum
  int agree_ints(int* v, int n, int op) {
    if (!comm_on()) return CAL_OK;
    CAL_TRY(agree_buf.reserve((size_t)n * sizeof(int)));
    HIP_TRY(hipMemcpyAsync(agree_buf.p, v, n * sizeof(int), hipMemcpyHostToDevice, stream));
    CAL_TRY(all_reduce(agree_buf.p, n, CAL_XCHG_I32, op));
    HIP_TRY(hipMemcpyAsync(v, agree_buf.p, n * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return CAL_OK;
  }

  // ---- padded copies ------------------------------------------------------------------------------------------
  int ensure_scratch(size_t bytes) {
    CAL_TRY(scratch.reserve(bytes, false));
    return CAL_OK;
  }
  // host [rows][nfreqs] -> device [rows][fpad] * stride + off
  int upload_rows(const void* src, T* dst, long long rows, int stride, int off) { return upload_rows(src, dst, rows, stride, off, nfreqs, fpad); }
  int download_rows(void* dst, const T* src, long long rows, int stride, int off) { return download_rows(dst, src, rows, stride, off, nfreqs, fpad); }
  // (rows of nfreqs elements padded to fpad: the gains and per-baseline arrays; the gain-basis coefficients bring their own two lengths)
  int upload_rows(const void* src, T* dst, long long rows, int stride, int off, int nfreqs, int fpad) {
    const size_t bytes = (size_t)rows * nfreqs * sizeof(T);
    if (stride == 1 && fpad == nfreqs) {
      HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
      HIP_TRY(hipStreamSynchronize(stream));
      return CAL_OK;
    }
    CAL_TRY(ensure_scratch(bytes));
    HIP_TRY(hipMemcpyAsync(scratch.p, src, bytes, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(pad_rows_kernel<T>, dim3(grid_for(rows * fpad)), dim3(256), 0, stream, scratch.as<T>(), dst, rows, nfreqs, fpad,
                       stride, off);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return CAL_OK;
  }
  int download_rows(void* dst, const T* src, long long rows, int stride, int off, int nfreqs, int fpad) {
    const size_t bytes = (size_t)rows * nfreqs * sizeof(T);
    if (stride == 1 && fpad == nfreqs) {
      HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
      return CAL_OK;
    }
    CAL_TRY(ensure_scratch(bytes));
    hipLaunchKernelGGL(unpad_rows_kernel<T>, dim3(grid_for(rows * nfreqs)), dim3(256), 0, stream, src, scratch.as<T>(), rows, nfreqs,
                       fpad, stride, off);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(dst, scratch.p, bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return CAL_OK;
  }

  int set_data(const void* dr, const void* di, const void* w) override {
    HIP_TRY(hipSetDevice(device));
    if (!has_problem) return fail(CAL_ERR_STATE, "set_data before set_problem");
    if (!dr || !di || !w) return fail(CAL_ERR_INVALID, "set_data: null pointer");
    CAL_TRY(upload_rows(dr, data_r.as<T>(), nbls, 1, 0));
    CAL_TRY(upload_rows(di, data_i.as<T>(), nbls, 1, 0));
    CAL_TRY(upload_rows(w, wgts.as<T>(), nbls, 1, 0));
    rw_w0_valid = false;  // robust_weights: the next call takes w0 from these
    has_data = true;
    return CAL_OK;
  }

  int set_regularization(int mode, const double* pr, const double* pi, bool per_slice) override {
    HIP_TRY(hipSetDevice(device));
    if (!has_problem) return fail(CAL_ERR_STATE, "set_regularization before set_problem");
    if (mode != CAL_REG_NONE && mode != CAL_REG_SUM) return fail(CAL_ERR_INVALID, "set_regularization: unknown mode %d", mode);
    if (!pr || !pi) return fail(CAL_ERR_INVALID, "set_regularization: null priors");
    if (mode != reg && nheads > 0) HIP_TRY(hipMemsetAsync(part.p, 0, part.bytes, stream));  // member items write their slot only in the regularised form
    if (mode != reg) drop_graph();
    reg = mode;
    for (int t = 0; t < nslices; ++t) {
      prior_r_t[t] = pr[per_slice ? t : 0];
      prior_i_t[t] = pi[per_slice ? t : 0];
    }
    if (reg == CAL_REG_SUM) {
      if (!q1.p) CAL_TRY(q1.alloc((size_t)(nbls + 1) * fpad * sizeof(T2)));
      if (!gcp1.p) CAL_TRY(gcp1.alloc(2 * (size_t)gcp_len * sizeof(T)));
      if (!gc_direct && !gc1.p) CAL_TRY(gc1.alloc(2 * (size_t)ncoef * sizeof(T)));
    }
    return CAL_OK;
  }
  int slice_count() override { return nslices; }
  int get_slice_losses(double* out) override {
    if (!has_problem) return fail(CAL_ERR_STATE, "get_slice_losses before set_problem");
    if (!out) return fail(CAL_ERR_INVALID, "get_slice_losses: null");
    for (int t = 0; t < nslices; ++t) out[t] = h_state[t].loss;
    return CAL_OK;
  }

  int set_optimizer(const cal_optimizer_desc* d) override {
    HIP_TRY(hipSetDevice(device));
    if (!has_problem) return fail(CAL_ERR_STATE, "set_optimizer before set_problem");
    if (!d) return fail(CAL_ERR_INVALID, "set_optimizer: null");
    if (d->optimizer < CAL_OPT_ADAM || d->optimizer > CAL_OPT_LAMB)
      return fail(CAL_ERR_INVALID, "set_optimizer: unknown optimizer id %d", d->optimizer);
    if (d->optimizer == CAL_OPT_LAMB && yb_on())
      return fail(CAL_ERR_UNSUPPORTED, "set_optimizer: LAMB is not supported while a gain basis is set (its per-variable norms are defined over the "
                  "per-channel gains); detach the basis (nvec = 0) or choose another optimizer");
    if (d->optimizer == CAL_OPT_LAMB && !lamb_ok)
      return fail(CAL_ERR_UNSUPPORTED, "set_optimizer: LAMB takes one trust ratio per variable; the groups of a variable (cal_problem_desc::grp_var) must be "
                  "contiguous inside a time slice");
    opt = *d;
    HIP_TRY(hipMemsetAsync(gains_m.p, 0, gains_m.bytes, stream));
    HIP_TRY(hipMemsetAsync(coef_m.p, 0, coef_m.bytes, stream));
    if ((d->optimizer == CAL_OPT_ADAGRAD || d->optimizer == CAL_OPT_FTRL) && d->initial_accumulator_value != 0.0) {
      // Adagrad's / Ftrl's accumulator starts at initial_accumulator_value (Keras default 0.1)
      hipLaunchKernelGGL(fill_kernel<T>, dim3(grid_for((long long)(gains_v.bytes / sizeof(T)))), dim3(256), 0, stream, gains_v.as<T>(),
                         (long long)(gains_v.bytes / sizeof(T)), (T)d->initial_accumulator_value);
      hipLaunchKernelGGL(fill_kernel<T>, dim3(grid_for((long long)(coef_v.bytes / sizeof(T)))), dim3(256), 0, stream, coef_v.as<T>(),
                         (long long)(coef_v.bytes / sizeof(T)), (T)d->initial_accumulator_value);
      if (yb_on())
        hipLaunchKernelGGL(fill_kernel<T>, dim3(grid_for((long long)(gb_yv.bytes / sizeof(T)))), dim3(256), 0, stream, gb_yv.as<T>(),
                           (long long)(gb_yv.bytes / sizeof(T)), (T)d->initial_accumulator_value);
      HIP_TRY(hipGetLastError());
    } else {
      HIP_TRY(hipMemsetAsync(gains_v.p, 0, gains_v.bytes, stream));
      HIP_TRY(hipMemsetAsync(coef_v.p, 0, coef_v.bytes, stream));
      if (yb_on()) HIP_TRY(hipMemsetAsync(gb_yv.p, 0, gb_yv.bytes, stream));
    }
    if (yb_on()) HIP_TRY(hipMemsetAsync(gb_ym.p, 0, gb_ym.bytes, stream));
    drop_graph();
    for (int t = 0; t < nslices; ++t) reset_loop_state(h_state[t]);  // a new fit begins
    held.clear();
    has_opt = true;
    HIP_TRY(hipStreamSynchronize(stream));
    return CAL_OK;
  }

  int set_params(const void* g_r, const void* g_i, const void* c_r, const void* c_i) override {
    HIP_TRY(hipSetDevice(device));
    if (!has_problem) return fail(CAL_ERR_STATE, "set_params before set_problem");
    if (g_r) CAL_TRY(upload_rows(g_r, gains.as<T>(), nants, 2, 0));
    if (g_i) CAL_TRY(upload_rows(g_i, gains.as<T>(), nants, 2, 1));
    if ((g_r || g_i) && yb_on()) CAL_TRY(rebase_gain_basis());  // the fit now starts from these gains: g0 := gains, y := 0
    if (c_r) HIP_TRY(copy_sync(coef.as<T>(), c_r, (size_t)ncoef * sizeof(T), hipMemcpyHostToDevice));
    if (c_i) HIP_TRY(copy_sync(coef.as<T>() + ncoef, c_i, (size_t)ncoef * sizeof(T), hipMemcpyHostToDevice));
    if (g_r && g_i) has_gains = true;
    if (c_r && c_i) has_coef = true;
    return CAL_OK;
  }

  int get_params(int which, void* g_r, void* g_i, void* c_r, void* c_i) override {
    HIP_TRY(hipSetDevice(device));
    if (!has_problem) return fail(CAL_ERR_STATE, "get_params before set_problem");
    const T* g = gains.as<T>();
    const T* c = coef.as<T>();
    if (which == 1) {
      if (!gains_snap.p) return fail(CAL_ERR_STATE, "get_params(which=1): no use_min snapshot was taken");
      if (yb_on()) {
        // the snapshot of a basis fit is y's: the gains it stands for are expanded into gains_snap (which no kernel writes while a basis is set)
        if (!gb_ysnap.p) return fail(CAL_ERR_STATE, "get_params(which=1): no use_min snapshot was taken since the gain basis was set");
        CAL_TRY(enqueue_expand(gb_ysnap.as<T2>(), gains_snap.as<T2>()));
      }
      g = gains_snap.as<T>();
      c = coef_snap.as<T>();
    } else if (which != 0) {
      return fail(CAL_ERR_INVALID, "get_params: which must be 0 or 1");
    }
    HIP_TRY(hipStreamSynchronize(stream));
    if (g_r) CAL_TRY(download_rows(g_r, g, nants, 2, 0));
    if (g_i) CAL_TRY(download_rows(g_i, g, nants, 2, 1));
    if (c_r) HIP_TRY(copy_sync(c_r, c, (size_t)ncoef * sizeof(T), hipMemcpyDeviceToHost));
    if (c_i) HIP_TRY(copy_sync(c_i, c + ncoef, (size_t)ncoef * sizeof(T), hipMemcpyDeviceToHost));
    return CAL_OK;
  }

  int get_moments(void* gm_r, void* gm_i, void* gv_r, void* gv_i, void* cm_r, void* cm_i, void* cv_r, void* cv_i,
                  int64_t* t) override {
    HIP_TRY(hipSetDevice(device));
    if (!has_problem) return fail(CAL_ERR_STATE, "get_moments before set_problem");
    if (tb_on()) return fail(CAL_ERR_UNSUPPORTED, "get_moments: checkpoint / resume of a fit with a gain time basis is not supported");
    if (gb_on()) return fail(CAL_ERR_UNSUPPORTED, "get_moments: checkpoint / resume of a fit with a gain basis is not supported");
    HIP_TRY(hipStreamSynchronize(stream));
    if (t && nslices > 1) {
      // every slice counts its own updates (slices stop on their own and then freeze): ONE t only describes a solver whose slices agree
      for (int sl = 1; sl < nslices; ++sl)
        if (h_state[sl].t != h_state[0].t)
          return fail(CAL_ERR_STATE, "get_moments: the %d time slices of this solver have applied different numbers of updates (slice 0: %lld, slice %d: %lld); "
                      "one iteration count cannot resume them bit for bit", nslices, (long long)h_state[0].t, sl, (long long)h_state[sl].t);
    }
    if (gm_r) CAL_TRY(download_rows(gm_r, gains_m.as<T>(), nants, 2, 0));
    if (gm_i) CAL_TRY(download_rows(gm_i, gains_m.as<T>(), nants, 2, 1));
    if (gv_r) CAL_TRY(download_rows(gv_r, gains_v.as<T>(), nants, 2, 0));
    if (gv_i) CAL_TRY(download_rows(gv_i, gains_v.as<T>(), nants, 2, 1));
    const size_t cb = (size_t)ncoef * sizeof(T);
    if (cm_r) HIP_TRY(copy_sync(cm_r, coef_m.as<T>(), cb, hipMemcpyDeviceToHost));
    if (cm_i) HIP_TRY(copy_sync(cm_i, coef_m.as<T>() + ncoef, cb, hipMemcpyDeviceToHost));
    if (cv_r) HIP_TRY(copy_sync(cv_r, coef_v.as<T>(), cb, hipMemcpyDeviceToHost));
    if (cv_i) HIP_TRY(copy_sync(cv_i, coef_v.as<T>() + ncoef, cb, hipMemcpyDeviceToHost));
    if (t) *t = h_state->t;
    return CAL_OK;
  }

  int set_moments(const void* gm_r, const void* gm_i, const void* gv_r, const void* gv_i, const void* cm_r, const void* cm_i,
                  const void* cv_r, const void* cv_i, int64_t t) override {
    HIP_TRY(hipSetDevice(device));
    if (!has_problem) return fail(CAL_ERR_STATE, "set_moments before set_problem");
    if (tb_on()) return fail(CAL_ERR_UNSUPPORTED, "set_moments: checkpoint / resume of a fit with a gain time basis is not supported");
    if (gb_on()) return fail(CAL_ERR_UNSUPPORTED, "set_moments: checkpoint / resume of a fit with a gain basis is not supported");
    if (t < 0) return fail(CAL_ERR_INVALID, "set_moments: negative iteration count");
    if (gm_r) CAL_TRY(upload_rows(gm_r, gains_m.as<T>(), nants, 2, 0));
    if (gm_i) CAL_TRY(upload_rows(gm_i, gains_m.as<T>(), nants, 2, 1));
    if (gv_r) CAL_TRY(upload_rows(gv_r, gains_v.as<T>(), nants, 2, 0));
    if (gv_i) CAL_TRY(upload_rows(gv_i, gains_v.as<T>(), nants, 2, 1));
    const size_t cb = (size_t)ncoef * sizeof(T);
    if (cm_r) HIP_TRY(copy_sync(coef_m.as<T>(), cm_r, cb, hipMemcpyHostToDevice));
    if (cm_i) HIP_TRY(copy_sync(coef_m.as<T>() + ncoef, cm_i, cb, hipMemcpyHostToDevice));
    if (cv_r) HIP_TRY(copy_sync(coef_v.as<T>(), cv_r, cb, hipMemcpyHostToDevice));
    if (cv_i) HIP_TRY(copy_sync(coef_v.as<T>() + ncoef, cv_i, cb, hipMemcpyHostToDevice));
    // beta^t as the device keeps it: a running product, one factor per update (pow() differs from it in the last bits, and a
    // resumed fit must continue bit for bit).  Uses the betas of the optimizer set so far: set_optimizer comes first.
    double b1t = 1.0, b2t = 1.0, sched = 1.0;
    for (int64_t k = 0; k < t; ++k) {
      b1t *= opt.beta_1;
      b2t *= opt.beta_2;
    }
    if (opt.optimizer == CAL_OPT_NADAM && t > 0) {
      // Nadam's momentum schedule is a running product of pow() terms: rebuilt by the DEVICE's pow (advance_state's), whose last
      // bits differ from the host's -- a resumed fit continues bit for bit
      hipLaunchKernelGGL(nadam_sched_kernel, dim3(1), dim3(1), 0, stream, opt.beta_1, (long long)t, scal.as<double>());
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(&sched, scal.p, sizeof(double), hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
    }
    for (int sl = 0; sl < nslices; ++sl) {
      h_state[sl].t = t;
      h_state[sl].b1t = b1t;
      h_state[sl].b2t = b2t;
      h_state[sl].nadam_sched = sched;
    }
    return CAL_OK;
  }

  // ---- one pass of the hot path -------------------------------------------------------------------------------
  template <typename A> A pass_args() {  // what the argument structs of the general and of the dense kernels share
    A a{};
    a.data_r = data_r.as<T>();
    a.data_i = data_i.as<T>();
    a.wgts = wgts.as<T>();
    a.gains = gains.as<T2>();
    a.c_r = coef.as<T>();
    a.c_i = coef.as<T>() + ncoef;
    a.q0 = q0.as<T2>();
    a.part = part.as<double>();
    a.state = st_cur();
    a.nslices = nslices;
    a.fpad = fpad;
    a.nbls = nbls;
    return a;
  }
  FusedArgs<T> fused_args() {
    FusedArgs<T> a = pass_args<FusedArgs<T>>();
    a.tiles = tiles.as<T>();
    a.bl_tile = bl_tile.as<long long>();
    a.bl_ant = bl_ant.as<int2>();
    a.items = items.as<Item>();
    a.q1 = q1.as<T2>();
    a.gcp0_r = gcp0.as<T>();
    a.gcp0_i = gcp0.as<T>() + gcp_len;
    a.gcp1_r = gcp1.as<T>();
    a.gcp1_i = gcp1.p ? gcp1.as<T>() + gcp_len : nullptr;
    a.runs = runs.as<int2>();
    a.stream_once = layout == CAL_LAYOUT_STREAM ? 1 : 0;
    a.members = members.as<Member>();
    a.heads = nheads > 0 ? heads.as<int>() : nullptr;
    a.nfreqs = nfreqs;
    return a;
  }
  // ... pointed at the first two planes of model_buf ([planes][nbls][fpad]): model(), model_pass()
  FusedArgs<T> model_args() {
    FusedArgs<T> a = fused_args();
    a.model_r = model_buf.as<T>();
    a.model_i = model_buf.as<T>() + (size_t)nbls * fpad;
    return a;
  }
  using DenseArgs = typename std::conditional<std::is_same<T, float>::value, MfmaArgs, Dense64Args>::type;
  DenseArgs dense_args() {
    DenseArgs m = pass_args<DenseArgs>();
    m.ops = mf_ops.as<T>();
    m.panels = mf_panels.as<PanelItem>();
    m.gc_r = grad_c0();
    m.gc_i = grad_c0() + ncoef;
    m.slot_map = mf_map.as<int>();
    return m;
  }
  // The shape of a pass or train step (step_plan.hpp) for the solver as it stands.  nsteps: of the run, for the replay rule alone.
  StepShape step_shape(PassAsk ask, int nsteps = 0) const {
    return plan_step(StepInputs{mf_ok, reg == CAL_REG_SUM, reg_prepass, gc_direct, comm_on(), yb_on(), 2LL * nants * fpad + 2LL * ncoef <= (1LL << 20), launch_mode,
                                opt.optimizer == CAL_OPT_LAMB, ask, timing, nsteps >= kGraphMinSteps});
  }

  // ---- one launcher per kernel ---------------------------------------------------------------------------------
  using FusedFn = void (*)(const FusedArgs<T>);
  static FusedFn pick(bool with_reg, FusedFn reg, FusedFn plain) { return with_reg ? reg : plain; }
  // fused_basis_kernel<T, MODE, REG, L, FOLD> (folded tiles: every item of the problem is one, set_problem)
  template <int MODE, int L> FusedFn basis_kernel(bool with_reg) const {
    return fold ? pick(with_reg, fused_basis_kernel<T, MODE, true, L, true>, fused_basis_kernel<T, MODE, false, L, true>)
                : pick(with_reg, fused_basis_kernel<T, MODE, true, L, false>, fused_basis_kernel<T, MODE, false, L, false>);
  }
  // LDS buffer of gbar_G rows (MODE_GRAD); the narrowest tiles have the longest offset table
  static constexpr size_t kQLdsMax1 = TileCfg<T, FbSet<T>::fb_min>::q_lds_bytes(false);
  static constexpr size_t kQLdsMax2 = TileCfg<T, FbSet<T>::fb_min>::q_lds_bytes(true);
  template <int MODE> void launch_fused(FusedArgs<T> a, bool with_reg) {  // a.item_base = 0, as fused_args leaves it
    constexpr bool kPass = MODE == MODE_LOSS || MODE == MODE_GRAD;  // the passes with a multi-slice form and a narrow instance
    // they leave the covered items to the multi-slice form (fused_basis_kernel would return at once for each of them)
    const int nsimple = (kPass && nheads > 0) ? nitems_plain : nitems_simple;
    if (nsimple > 0) {
      FusedFn k = basis_kernel<MODE, kMaxLoads>(with_reg);
      if constexpr (kPass)
        if (small_loads) k = basis_kernel<MODE, kSmallLoads>(with_reg);
      const size_t lds = lds_bytes + (MODE == MODE_GRAD ? (with_reg ? kQLdsMax2 : kQLdsMax1) : 0);
      hipLaunchKernelGGL(k, dim3(nsimple), dim3(kThreads), lds, stream, a);
    }
    if constexpr (kPass) {
      // baselines that share tiles (skipped by the launch above): one workgroup per set.  With the regulariser these kernels take
      // the two-pass form (loss pass: S; gradient pass: alpha of each member's slice from the state) -- enqueue_pass orders the passes
      if (nheads > 0) {
        if (nheads_mfma > 0) {
          FusedFn k = pick(with_reg, fused_multi_mfma_kernel<T, MODE, 1>, fused_multi_mfma_kernel<T, MODE, 0>);
          if (with_reg && MODE == MODE_GRAD && heads_one_pass) k = fused_multi_mfma_kernel<T, MODE_GRAD, 2>;
          hipLaunchKernelGGL(k, dim3(mm_grid), dim3(kThreads), lds_multi_mfma_bytes, stream, a);
        }
        if (nheads > nheads_mfma) {
          FusedArgs<T> b = a;
          b.heads = a.heads + mm_grid;
          const FusedFn km = pick(with_reg, fused_multi_kernel<T, MODE, true>, fused_multi_kernel<T, MODE, false>);
          hipLaunchKernelGGL(km, dim3(nheads - nheads_mfma), dim3(kThreads), lds_multi_bytes, stream, b);
        }
      }
    }
    if (nitems > nitems_simple) {
      a.item_base = nitems_simple;
      const FusedFn kg = pick(with_reg, fused_group_kernel<T, MODE, true>, fused_group_kernel<T, MODE, false>);
      hipLaunchKernelGGL(kg, dim3(nitems - nitems_simple), dim3(kThreads), lds_group_bytes, stream, a);
    }
  }
  // the dense pass: fp64 its own kernel; fp32 the split-operand kernels where set-up chose them
  template <bool GRAD> void launch_dense(const DenseArgs& m) {
    void (*k)(DenseArgs);
    if constexpr (std::is_same<T, float>::value) k = !mf_split ? fused_dense_kernel<GRAD> : mf_split2 ? fused_dense_split2_kernel<GRAD> : fused_dense_split_kernel<GRAD>;
    else k = fused_dense64_kernel<GRAD>;
    hipLaunchKernelGGL(k, dim3(mf_grid), dim3(kDenseThreads), (GRAD ? mf_lds_grad : mf_lds_loss)[0], stream, m);
  }
  T* grad_c0() { return gc_direct ? gcp0.as<T>() : gc0.as<T>(); }
  T* grad_c1() { return gc_direct ? gcp1.as<T>() : gc1.as<T>(); }
  // blocks of the per-antenna reduction (gain_grad_kernel, step_tail_kernel): one per antenna and 64 lanes of 16 bytes
  int gain_blocks() const {
    const int cpl = 16 / (int)sizeof(T2) > 0 ? 16 / (int)sizeof(T2) : 1;
    return nants * ((fpad + 64 * cpl - 1) / (64 * cpl));
  }
  // gain_grad_kernel: the per-antenna reduction into r0 (REG: r1, r2 too) and, in one block per slice, its n_parts loss partials summed.
  // nants_or_0 = 0: the partial sums alone (no antenna work)
  template <bool REG> void launch_gain_grad(int blocks, T2* r0, T2* r1, T2* r2, int nants_or_0, int n_parts, const SliceMap& sm) {
    hipLaunchKernelGGL((gain_grad_kernel<T, REG>), dim3(blocks), dim3(256), 0, stream, q0.as<T2>(), q1.as<T2>(), gains.as<T2>(), ant_ptr.as<int>(),
                       ant_ent.as<int2>(), r0, r1, r2, nants_or_0, fpad, part.as<double>(), n_parts, scal.as<double>(), st_cur(), sm);
  }
  // coeff_partial_reduce_kernel: gc = the sums of the partials gcp of multi-item groups
  void launch_partial_reduce(const DevBuf& gcp, const DevBuf& gc, const SliceMap& sm) {
    hipLaunchKernelGGL(coeff_partial_reduce_kernel<T>, dim3((ncoef + 255) / 256), dim3(256), 0, stream, gcp.as<T>(), gcp.as<T>() + gcp_len, gc.as<T>(),
                       gc.as<T>() + ncoef, coef_grp.as<int>(), grp_coff.as<int>(), grp_item_ptr.as<int>(), item_goff.as<int>(), ncoef, st_cur(), sm);
  }
  // ... or the same sums taken by the update itself (step_update_kernel, step_tail_kernel)
  PartialSum<T> partial_sum(const DevBuf& gcp) {
    return PartialSum<T>{gcp.as<T>(), gcp.p ? gcp.as<T>() + gcp_len : nullptr, coef_grp.as<int>(), grp_coff.as<int>(), grp_item_ptr.as<int>(), item_goff.as<int>(), ncoef};
  }
  // Behind a loss pass whose gradient pass needs alpha = 2 (S - P) of every slice (dense path with the regulariser; baselines that share
  // tiles): the slices' sums -- with a communicator over the ranks, also on a rank whose own heads would not need it: its partials are part
  // of the sums --, then alpha into the state
  int enqueue_alpha_prepass(int n_parts, const SliceMap& sm) {
    launch_gain_grad<false>(nslices, comm.as<T2>(), comm.as<T2>(), comm.as<T2>(), 0, n_parts, sm);
    if (comm_on()) CAL_TRY(all_reduce(scal.p, 4 * (size_t)nslices, CAL_XCHG_F64, CAL_XCHG_SUM));
    hipLaunchKernelGGL(alpha_kernel, dim3((nslices + 63) / 64), dim3(64), 0, stream, st_cur(), scal.as<double>(), nslices);
    return CAL_OK;
  }
  // the time kernels' view of y and of the gradient planes: rows of time_row() reals, the tb_na antennas' 16-byte vectors in blocks of 256
  int time_row() const { return 2 * y_w(); }
  unsigned time_blocks() const { return (unsigned)(((long long)tb_na * (time_row() / (16 / (int)sizeof(T))) + 255) / 256); }
  // the gain-gradient planes at r0 onto the basis, into gb_proj
  int enqueue_project(int planes, T2* r0, const SliceMap& sm) {
    const DevState* st = st_cur();
    if (gb_on())
      hipLaunchKernelGGL((gain_project_kernel<T>), dim3(nants, planes), dim3(256), 0, stream, r0, gb_B.as<T>(), (tb_on() ? tb_pf : gb_proj).template as<T>(),
                         nants, fpad, gb_kpad, st, sm);
    if (tb_on()) {
      // the contraction over time, of the frequency-projected planes or of the per-channel ones
      hipLaunchKernelGGL((gain_time_project_kernel<T>), dim3(time_blocks(), (tb_L + kTimeTile - 1) / kTimeTile, planes), dim3(256), 0, stream,
                         gb_on() ? tb_pf.as<T>() : reinterpret_cast<const T*>(r0), tb_B.as<T>(), gb_proj.as<T>(), tb_na, tb_T, tb_L, tb_lpad, time_row(),
                         (size_t)nants * time_row());
    }
    HIP_TRY(hipGetLastError());
    return CAL_OK;
  }
  // a timed pass begins: the next pair of events of the pool, the first recorded now, *end behind the pass (enqueue_pass)
  int begin_timed_pass(hipEvent_t* end) {
    if (ev_used == ev_pool.size()) {
      hipEvent_t x, y;
      HIP_TRY(hipEventCreate(&x));
      HIP_TRY(hipEventCreate(&y));
      ev_pool.push_back({x, y});
    }
    *end = ev_pool[ev_used].second;
    HIP_TRY(hipEventRecord(ev_pool[ev_used++].first, stream));
    return CAL_OK;
  }

  // enqueue: loss (+ gradients) of the current parameters in the shape `s` (step_shape); leaves loss in state, final gradients in
  // comm[0] / grad_c0(), or with s.proj the gain gradient in gb_proj: the planes are projected BEFORE the exchange, which then carries
  // planes x 2 nants gb_kpad reals instead of planes x 2 nants fpad.  With s.tail1 the caller follows up with step_tail_kernel
  // (enqueue_step), which does everything behind the fused pass.
  int enqueue_pass(const StepShape& s, int losses_cap) {
    DevState* st = st_cur();
    hipEvent_t e1 = nullptr;
    if (timing) CAL_TRY(begin_timed_pass(&e1));
    const int n_parts = s.dense ? mf_npanels : nitems;
    const SliceMap sm = smap(s.dense);
    if (s.dense) {
      DenseArgs m = dense_args();
      if (s.two_pass) {
        launch_dense<false>(m);
        CAL_TRY(enqueue_alpha_prepass(n_parts, sm));
        m.use_alpha = 1;
      }
      if (s.grads) launch_dense<true>(m); else launch_dense<false>(m);
    } else {
      const FusedArgs<T> a = fused_args();
      if (s.prepass) {
        launch_fused<MODE_LOSS>(a, true);
        CAL_TRY(enqueue_alpha_prepass(n_parts, sm));
      }
      if (s.grads) launch_fused<MODE_GRAD>(a, s.reg); else launch_fused<MODE_LOSS>(a, s.reg);
    }
    if (timing) HIP_TRY(hipEventRecord(e1, stream));
    if (s.tail1) {
      HIP_TRY(hipGetLastError());
      return CAL_OK;
    }
    const size_t gn = (size_t)nants * fpad;
    T2* r0 = comm.as<T2>();
    T2* r1 = r0 + gn;
    T2* r2 = r1 + gn;
    if (s.partial_reduce) {
      launch_partial_reduce(gcp0, gc0, sm);
      if (s.Rk) launch_partial_reduce(gcp1, gc1, sm);
    }
    if (!s.grads) launch_gain_grad<false>(nslices, r0, r1, r2, 0, n_parts, sm);  // loss only: just the partial-sum blocks
    else if (s.Rk) launch_gain_grad<true>(gain_blocks() + nslices, r0, r1, r2, nants, n_parts, sm);
    else launch_gain_grad<false>(gain_blocks() + nslices, r0, r1, r2, nants, n_parts, sm);
    if (s.proj) CAL_TRY(enqueue_project(s.planes, r0, sm));
    const size_t xn = s.proj ? (size_t)y_rows() * y_row() : gn;  // complex elements per plane of the gain gradient from here on
    T2* x0 = s.proj ? gb_proj.as<T2>() : r0;
    if (comm_on()) {
      // the one exchange step of the sharded fit: sum gain-gradient parts and loss scalars over ranks
      // (issued for a 1-rank communicator too, so the path can be exercised on a single GPU)
      const int gdt = sizeof(T) == 4 ? CAL_XCHG_F32 : CAL_XCHG_F64;
      if (nccl) NCCL_TRY(ncclGroupStart());
      int rc = CAL_OK;
      if (s.grads) rc = all_reduce(x0, (size_t)s.planes * xn * 2, gdt, CAL_XCHG_SUM);
      if (rc == CAL_OK) rc = all_reduce(scal.p, 4 * (size_t)nslices, CAL_XCHG_F64, CAL_XCHG_SUM);
      if (nccl) NCCL_TRY(ncclGroupEnd());
      CAL_TRY(rc);
    }
    if (s.finalize)
      hipLaunchKernelGGL(finalize_kernel, dim3((nslices + 63) / 64), dim3(64), 0, stream, st, scal.as<double>(), losses.as<double>(), losses_cap,
                         s.update != UPDATE_NONE ? 1 : 0, nslices);
    if (s.grads && s.Rk) {
      hipLaunchKernelGGL(combine_gain_kernel<T>, dim3((int)((xn + 255) / 256)), dim3(256), 0, stream, x0, x0 + xn, x0 + 2 * xn, (int)xn, st, sm,
                         s.proj ? (int)y_row() : fpad);
      hipLaunchKernelGGL(combine_coeff_kernel<T>, dim3((ncoef + 255) / 256), dim3(256), 0, stream, grad_c0(), grad_c0() + ncoef,
                         grad_c1(), grad_c1() + ncoef, ncoef, st, sm);
    }
    HIP_TRY(hipGetLastError());
    return CAL_OK;
  }

  int enqueue_tail(const StepShape& s, bool freeze_model, int losses_cap) {
    TailArgs<T> a{};
    a.q0 = q0.as<T2>();
    a.q1 = q1.as<T2>();
    a.gains_in = gains.as<T2>();
    a.gains_out = gains_alt.as<T2>();
    a.gains_m = gains_m.as<T>();
    a.gains_v = gains_v.as<T>();
    a.gains_snap = gains_snap.p ? gains_snap.as<T>() : gains_alt.as<T>();  // only written when use_min found a new minimum
    a.ant_ptr = ant_ptr.as<int>();
    a.ant_ent = ant_ent.as<int2>();
    a.coef = AdamSet<T>{coef.as<T>(), gcp0.as<T>(), coef_m.as<T>(), coef_v.as<T>(), coef_snap.p ? coef_snap.as<T>() : coef.as<T>(),
                        freeze_model ? 0LL : 2LL * ncoef};
    a.coef_g1 = gcp1.as<T>();
    if (s.partials) {
      a.ps0 = partial_sum(gcp0);
      a.ps1 = partial_sum(gcp1);
    }
    a.part = part.as<double>();
    a.nparts = nitems;
    a.nants = nants;
    a.fpad = fpad;
    a.nblk_gain = gain_blocks();
    a.in = st_cur();
    a.out = st_nxt();
    a.losses = losses.as<double>();
    a.losses_cap = losses_cap;
    a.M = smap(false);
    a.cblk_ptr = nslices > 1 ? slice_cblk.as<int>() : nullptr;
    a.ncoef = ncoef;
    const long long nblk_c = freeze_model ? 0 : h_slice_cblk[nslices];
    if (s.reg) hipLaunchKernelGGL((step_tail_kernel<T, true>), dim3((unsigned)(a.nblk_gain + nblk_c)), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((step_tail_kernel<T, false>), dim3((unsigned)(a.nblk_gain + nblk_c)), dim3(256), 0, stream, a);
    st_par ^= 1;
    std::swap(gains.p, gains_alt.p);  // the buffer just written is the current one
    HIP_TRY(hipGetLastError());
    return CAL_OK;
  }
  // the optimizer's gain variables, with a gain basis y (the same kernels on flat arrays of another row length), and that row length
  AdamSet<T> gain_set() {
    if (yb_on()) return AdamSet<T>{gb_y.as<T>(), gb_proj.as<T>(), gb_ym.as<T>(), gb_yv.as<T>(), gb_ysnap.p ? gb_ysnap.as<T>() : gb_y.as<T>(), 2LL * y_rows() * y_row()};
    return AdamSet<T>{gains.as<T>(), comm.as<T>(), gains_m.as<T>(), gains_v.as<T>(), gains_snap.p ? gains_snap.as<T>() : gains.as<T>(), 2LL * nants * fpad};
  }
  int gain_row() const { return yb_on() ? (int)y_row() : fpad; }
  int enqueue_update(const StepShape& s, bool freeze_model, int losses_cap) {
    DevState* st = st_cur();
    const AdamSet<T> ga = gain_set();
    const AdamSet<T> ca{coef.as<T>(), grad_c0(), coef_m.as<T>(), coef_v.as<T>(), coef_snap.p ? coef_snap.as<T>() : coef.as<T>(), freeze_model ? 0LL : 2LL * ncoef};
    const int nblk_a = (int)((ga.n + 255) / 256), nblk_b = (int)((ca.n + 255) / 256);
    if (s.update == UPDATE_FUSED) {
      // the common path: finalize + update (+ the partial coefficient-gradient sums of split groups) as one launch
      PartialSum<T> ps{};
      if (s.partials && !freeze_model) ps = partial_sum(gcp0);
      const unsigned nb = (unsigned)std::max(1, std::min(nblk_a + nblk_b, 16384));
      hipLaunchKernelGGL((step_update_kernel<T>), dim3(nb), dim3(256), (size_t)nslices * sizeof(SliceStep<T>), stream, ga, ca, ps, st, st_nxt(),
                         scal.as<double>(), losses.as<double>(), losses_cap, smap(s.dense), gain_row(), ncoef);
      st_par ^= 1;
    } else if (s.update == UPDATE_LAMB) {
      // moments + u (in place of the gradients), per-variable norms, trust ratios, parameters.  (With a frozen model the
      // coefficient variables are not touched: their set is empty and their ratios are never read.)
      T* ua = comm.as<T>();
      T* ub = grad_c0();
      hipLaunchKernelGGL((lamb_moments_kernel<T>), dim3((unsigned)(nblk_a + nblk_b)), dim3(256), 0, stream, ga, ca, nblk_a, st, smap(s.dense), fpad, ncoef, ua, ub);
      hipLaunchKernelGGL((lamb_norm_kernel<T>), dim3((unsigned)(lamb_nvar * kLambSeg)), dim3(256), 0, stream, lamb_vars.as<LambVar>(), gains.as<T>(), ua,
                         coef.as<T>(), ub, lamb_partial.as<double>());
      const double* glob = nullptr;
      if (comm_on() && !freeze_model) {
        // a coefficient variable's groups are spread over the ranks: its sums of squares are summed over them (a few doubles per slice)
        const size_t nglob = (size_t)2 * nslices * lamb_nv * 2;
        HIP_TRY(hipMemsetAsync(lamb_glob.p, 0, nglob * sizeof(double), stream));
        hipLaunchKernelGGL(lamb_fold_kernel, dim3((2 * lamb_ncvar + 63) / 64), dim3(64), 0, stream, lamb_partial.as<double>(), lamb_glob.as<double>(),
                           lamb_slot.as<int>(), 2 * nslices, lamb_ncvar, nslices * lamb_nv);
        CAL_TRY(all_reduce(lamb_glob.p, nglob, CAL_XCHG_F64, CAL_XCHG_SUM));
        glob = lamb_glob.as<double>();
      }
      hipLaunchKernelGGL(lamb_ratio_kernel, dim3((lamb_nvar + 63) / 64), dim3(64), 0, stream, lamb_partial.as<double>(), lamb_ratio.as<double>(), lamb_nvar,
                         glob, lamb_slot.as<int>(), 2 * nslices, lamb_ncvar, nslices * lamb_nv);
      hipLaunchKernelGGL((lamb_apply_kernel<T>), dim3((unsigned)(nblk_a + nblk_b)), dim3(256), 0, stream, ga, ca, nblk_a, st, smap(s.dense), fpad, ncoef, ua, ub,
                         lamb_ratio.as<double>(), lamb_cvar_ptr.as<int>(), lamb_ncvar);
    } else {
      constexpr long long per = 256LL * kAdamVec<T>;  // elements per block
      const int va = (int)((ga.n + per - 1) / per), vb = (int)((ca.n + per - 1) / per);
      hipLaunchKernelGGL((adam2_kernel<T>), dim3((unsigned)(va + vb)), dim3(256), 0, stream, ga, ca, va, st, smap(s.dense), gain_row(), ncoef);
    }
    HIP_TRY(hipGetLastError());
    // with a gain basis the gains are rebuilt from y
    return s.expand ? enqueue_expand(gb_y.as<T2>(), gains.as<T2>()) : (int)CAL_OK;
  }
  // one train step: the pass, then its one-launch tail or its update
  int enqueue_step(const StepShape& s, bool freeze_model, int cap) {
    CAL_TRY(enqueue_pass(s, cap));
    return s.tail1 ? enqueue_tail(s, freeze_model, cap) : enqueue_update(s, freeze_model, cap);
  }
  // dst = g0 + B src (src: y or its use_min snapshot); with a time basis dst = g0 + Bt (x) B src
  int enqueue_expand(const T2* src, T2* dst) {
    constexpr int per = 256 * (16 / (int)sizeof(T));  // channels per block
    if (tb_on()) {
      hipLaunchKernelGGL((gain_time_expand_kernel<T>), dim3(time_blocks(), (tb_T + kTimeTile - 1) / kTimeTile), dim3(256), 0, stream,
                         gb_on() ? nullptr : gb_g0.as<T>(), tb_Bt.as<T>(), reinterpret_cast<const T*>(src),
                         gb_on() ? tb_z.as<T>() : reinterpret_cast<T*>(dst), tb_na, tb_T, tb_L, tb_tpad, time_row());
      src = tb_z.as<T2>();
    }
    if (gb_on())
      hipLaunchKernelGGL((gain_expand_kernel<T>), dim3((fpad + per - 1) / per, nants), dim3(256), 0, stream, gb_g0.as<T2>(), gb_Bt.as<T>(), src, dst, fpad, gb_kpad);
    HIP_TRY(hipGetLastError());
    return CAL_OK;
  }
  void release_gain_basis() {
    gb_nvec = gb_kpad = 0;
    tb_T = tb_L = tb_lpad = tb_tpad = tb_na = 0;
    for (DevBuf* b : {&gb_B, &gb_Bt, &gb_g0, &gb_y, &gb_ym, &gb_yv, &gb_ysnap, &gb_proj, &tb_B, &tb_Bt, &tb_z, &tb_pf}) b->release();
    release_gain_systems();
  }
  void release_gain_systems() {  // the scratch of the two basis sweeps and of gain_basis_errors: sized again by the next call
    for (DevBuf* b : {&pg_m, &pg_n, &pg_rhsa, &pg_d, &pg_rhs, &pg_cnt, &gbe_w, &gbe_ok, &gbe_out}) b->release();
  }
  // the fit starts from the gains the solver holds now: g0 := gains, y := 0 (and its snapshot with it)
  int rebase_gain_basis() {
    HIP_TRY(hipMemcpyAsync(gb_g0.p, gains.p, gains.bytes, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemsetAsync(gb_y.p, 0, gb_y.bytes, stream));
    if (gb_ysnap.p) HIP_TRY(hipMemsetAsync(gb_ysnap.p, 0, gb_ysnap.bytes, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return CAL_OK;
  }
  // after either setter changed its basis: the y arrays in the shape the two bases now give them, g0 := gains, y := 0, moments and t zeroed
  int reshape_gain_coeffs() {
    for (DevBuf* b : {&gb_g0, &gb_y, &gb_ym, &gb_yv, &gb_ysnap, &gb_proj, &tb_z, &tb_pf}) b->release();
    release_gain_systems();
    if (yb_on()) {
      const size_t ybytes = (size_t)y_rows() * y_row() * sizeof(T2);
      CAL_TRY(gb_g0.alloc(gains.bytes, false));
      CAL_TRY(gb_y.alloc(ybytes));
      CAL_TRY(gb_ym.alloc(ybytes));
      CAL_TRY(gb_yv.alloc(ybytes));
      CAL_TRY(gb_proj.alloc(3 * ybytes));
      if (gb_on() && tb_on()) {
        CAL_TRY(tb_z.alloc((size_t)nants * gb_kpad * sizeof(T2)));
        CAL_TRY(tb_pf.alloc(3 * (size_t)nants * gb_kpad * sizeof(T2)));
      }
      CAL_TRY(rebase_gain_basis());
    }
    if (has_opt) {
      // moments and iteration count start over, exactly as set_optimizer leaves them (of y, of the gains, of the coefficients)
      const cal_optimizer_desc same = opt;
      CAL_TRY(set_optimizer(&same));
    }
    return CAL_OK;
  }
  // the device copies of a basis and of its transpose
  int upload_basis_pair(DevBuf& d, DevBuf& dt, const std::vector<T>& h, const std::vector<T>& ht) {
    CAL_TRY(d.alloc(h.size() * sizeof(T), false));
    CAL_TRY(dt.alloc(ht.size() * sizeof(T), false));
    HIP_TRY(copy_sync(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    HIP_TRY(copy_sync(dt.p, ht.data(), ht.size() * sizeof(T), hipMemcpyHostToDevice));
    return CAL_OK;
  }
  // a setter that failed half way (an allocation, a copy) must not leave one basis on with y arrays in the shape of another
  // configuration: BOTH bases go, the fit is per channel from the gains as they stand, and the caller gets the error
  int detach_bases_after(int rc) {
    if (rc != CAL_OK) release_gain_basis();
    return rc;
  }
  int set_gain_basis(const void* basis, int nvec) override {
    HIP_TRY(hipSetDevice(device));
    if (!has_problem) return fail(CAL_ERR_STATE, "set_gain_basis before set_problem");
    if (nvec < 0 || nvec > nfreqs) return fail(CAL_ERR_INVALID, "set_gain_basis: nvec = %d; a basis has 1 .. nfreqs = %d vectors (0 detaches it)", nvec, nfreqs);
    if (nvec > 0 && !basis) return fail(CAL_ERR_INVALID, "set_gain_basis: null basis");
    if (nvec == 0 && !gb_on()) return CAL_OK;  // nothing to detach: the fit goes on as it stands, moments included
    if (nvec > 0 && has_opt && opt.optimizer == CAL_OPT_LAMB)
      return fail(CAL_ERR_UNSUPPORTED, "set_gain_basis: LAMB is not supported with a gain basis (its per-variable norms are defined over the per-channel gains)");
    HIP_TRY(hipStreamSynchronize(stream));
    if (nvec == 0) {
      // back to the per-channel fit (or the one smooth in time only), from the gains as they stand
      drop_graph();
      gb_nvec = gb_kpad = 0;
      gb_B.release();
      gb_Bt.release();
    } else {
      const T* b = static_cast<const T*>(basis);
      for (long long i = 0; i < (long long)nfreqs * nvec; ++i)
        if (!std::isfinite((double)b[i])) return fail(CAL_ERR_INVALID, "set_gain_basis: the basis has a non-finite element");
      drop_graph();
      const int kpad = (nvec + kGainBasisPad - 1) / kGainBasisPad * kGainBasisPad;
      std::vector<T> hB((size_t)fpad * kpad, (T)0), hBt((size_t)kpad * fpad, (T)0);
      for (int f = 0; f < nfreqs; ++f)
        for (int k = 0; k < nvec; ++k) hB[(size_t)f * kpad + k] = hBt[(size_t)k * fpad + f] = b[(size_t)f * nvec + k];
      gb_nvec = gb_kpad = 0;
      const int rc = upload_basis_pair(gb_B, gb_Bt, hB, hBt);
      if (rc != CAL_OK) return detach_bases_after(rc);
      gb_nvec = nvec;
      gb_kpad = kpad;
    }
    return detach_bases_after(reshape_gain_coeffs());
  }
  int set_gain_time_basis(const void* basis_t, int ntimes, int nvec_t) override {
    HIP_TRY(hipSetDevice(device));
    if (!has_problem) return fail(CAL_ERR_STATE, "set_gain_time_basis before set_problem");
    if (nvec_t < 0) return fail(CAL_ERR_INVALID, "set_gain_time_basis: nvec_t = %d is negative (0 detaches the time basis)", nvec_t);
    if (nvec_t == 0) {
      if (!tb_on()) return CAL_OK;  // nothing to detach: the fit goes on as it stands, moments included
      HIP_TRY(hipStreamSynchronize(stream));
      drop_graph();
      tb_T = tb_L = tb_lpad = tb_tpad = tb_na = 0;
      tb_B.release();
      tb_Bt.release();
      return detach_bases_after(reshape_gain_coeffs());
    }
    if (nslices > 1)
      return fail(CAL_ERR_UNSUPPORTED, "set_gain_time_basis: the solver holds %d time slices that stop on their own, which contradicts variables shared "
                  "between them; build the times as one fit (nslices <= 1, nants = ntimes x antennas)", nslices);
    if (ntimes <= 0 || nants % ntimes != 0)
      return fail(CAL_ERR_INVALID, "set_gain_time_basis: nants = %d is not a multiple of ntimes = %d (antenna a at time t is row t * (nants / ntimes) + a)", nants,
                  ntimes);
    if (nvec_t > ntimes) return fail(CAL_ERR_INVALID, "set_gain_time_basis: nvec_t = %d; a time basis has 1 .. ntimes = %d vectors (0 detaches it)", nvec_t, ntimes);
    if (!basis_t) return fail(CAL_ERR_INVALID, "set_gain_time_basis: null basis");
    if (has_opt && opt.optimizer == CAL_OPT_LAMB)
      return fail(CAL_ERR_UNSUPPORTED, "set_gain_time_basis: LAMB is not supported with a gain time basis (its per-variable norms are defined over the "
                  "per-channel gains)");
    const T* b = static_cast<const T*>(basis_t);
    for (long long i = 0; i < (long long)ntimes * nvec_t; ++i)
      if (!std::isfinite((double)b[i])) return fail(CAL_ERR_INVALID, "set_gain_time_basis: the basis has a non-finite element");
    HIP_TRY(hipStreamSynchronize(stream));
    drop_graph();
    const int lpad = (nvec_t + kTimeTile - 1) / kTimeTile * kTimeTile, tpad = (ntimes + kTimeTile - 1) / kTimeTile * kTimeTile;
    std::vector<T> hB((size_t)ntimes * lpad, (T)0), hBt((size_t)nvec_t * tpad, (T)0);
    for (int t = 0; t < ntimes; ++t)
      for (int l = 0; l < nvec_t; ++l) hB[(size_t)t * lpad + l] = hBt[(size_t)l * tpad + t] = b[(size_t)t * nvec_t + l];
    tb_T = tb_L = tb_lpad = tb_tpad = tb_na = 0;
    const int rc = upload_basis_pair(tb_B, tb_Bt, hB, hBt);
    if (rc != CAL_OK) return detach_bases_after(rc);
    tb_T = ntimes;
    tb_L = nvec_t;
    tb_lpad = lpad;
    tb_tpad = tpad;
    tb_na = nants / ntimes;
    return detach_bases_after(reshape_gain_coeffs());
  }
  int get_gain_coeffs(int which, void* y_r, void* y_i) override {
    HIP_TRY(hipSetDevice(device));
    if (!yb_on()) return fail(CAL_ERR_STATE, "get_gain_coeffs: no gain basis is set (cal_solver_set_gain_basis, cal_solver_set_gain_time_basis)");
    if (which != 0 && which != 1) return fail(CAL_ERR_INVALID, "get_gain_coeffs: which must be 0 or 1");
    if (which == 1 && !gb_ysnap.p) return fail(CAL_ERR_STATE, "get_gain_coeffs(which=1): no use_min snapshot was taken since the gain basis was set");
    HIP_TRY(hipStreamSynchronize(stream));
    return download_y(y_r, y_i, which == 1 ? gb_ysnap.as<T>() : gb_y.as<T>());
  }
  int download_y(void* y_r, void* y_i, const T* src) {  // the two planes of an array in the shape of y (null: not asked for)
    const long long rows = y_rows() * (y_row() / y_w());
    if (y_r) CAL_TRY(download_rows(y_r, src, rows, 2, 0, y_cols(), y_w()));
    if (y_i) CAL_TRY(download_rows(y_i, src, rows, 2, 1, y_cols(), y_w()));
    return CAL_OK;
  }
  // the optimizer's slots of a fit with a gain basis, read only (get_moments / set_moments stay refused there: no resume): the y slots
  // in the shape of get_gain_coeffs, the coefficient slots, and every slice's own update count
  int get_gain_coeff_moments(void* ym_r, void* ym_i, void* yv_r, void* yv_i, void* cm_r, void* cm_i, void* cv_r, void* cv_i, int64_t* t) override {
    HIP_TRY(hipSetDevice(device));
    if (!yb_on()) return fail(CAL_ERR_STATE, "get_gain_coeff_moments: no gain basis is set (cal_solver_set_gain_basis, cal_solver_set_gain_time_basis)");
    if (!has_opt) return fail(CAL_ERR_STATE, "get_gain_coeff_moments: no optimizer is set (cal_solver_set_optimizer)");
    HIP_TRY(hipStreamSynchronize(stream));
    CAL_TRY(download_y(ym_r, ym_i, gb_ym.as<T>()));
    CAL_TRY(download_y(yv_r, yv_i, gb_yv.as<T>()));
    const size_t cb = (size_t)ncoef * sizeof(T);
    if (cm_r) HIP_TRY(copy_sync(cm_r, coef_m.as<T>(), cb, hipMemcpyDeviceToHost));
    if (cm_i) HIP_TRY(copy_sync(cm_i, coef_m.as<T>() + ncoef, cb, hipMemcpyDeviceToHost));
    if (cv_r) HIP_TRY(copy_sync(cv_r, coef_v.as<T>(), cb, hipMemcpyDeviceToHost));
    if (cv_i) HIP_TRY(copy_sync(cv_i, coef_v.as<T>() + ncoef, cb, hipMemcpyDeviceToHost));
    if (t)
      for (int sl = 0; sl < nslices; ++sl) t[sl] = h_state[sl].t;
    return CAL_OK;
  }
  int eval_gain_coeff_grads(double* loss, void* gy_r, void* gy_i) override {
    HIP_TRY(hipSetDevice(device));
    CAL_TRY(ready());
    if (!yb_on()) return fail(CAL_ERR_STATE, "eval_gain_coeff_grads: no gain basis is set (cal_solver_set_gain_basis, cal_solver_set_gain_time_basis)");
    CAL_TRY(eval_pass(kProjectedGradPass, loss));
    return download_y(gy_r, gy_i, gb_proj.as<T>());
  }

  void drop_graph() {
    if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
    graph_exec = nullptr;
  }
  // kGraphSteps train steps (fused pass + one-launch tail each) captured once per configuration and replayed.  Everything a
  // step reads that changes between steps lives in device memory (loop state, parameters, moments); what is baked into the
  // captured launches -- buffer pointers, optimizer, frozen model, regulariser, loss-history capacity, which halves of the
  // double-buffered state and gains are current -- is the key.  kGraphSteps is even, so a replay leaves both double buffers
  // where it found them and the same graph serves the next replay.
  // s.tail1: the two-launch form of small problems (fused pass + step_tail_kernel); else the kernels of a large problem's step (fused / dense
  // pass(es), gain_grad_kernel, finalize_kernel, the update): a host whose cores are busy elsewhere then pays ONE launch per `nsteps` steps
  // instead of four or five per step (measured on shared boxes: 2.4-3.2 ms per step of a 0.6-ms kernel while the host was contended).
  int replay_steps(const StepShape& s, bool freeze_model, int cap, int nsteps) {
    const GraphKey key{opt.optimizer, freeze_model ? 1 : 0, reg, cap, st_par, s.tail1 ? 1 : 0, nsteps, gains.p, gains_snap.p, losses.p, gb_y.p, gb_ysnap.p, tb_z.p, tb_pf.p};
    if (!graph_exec || !(key == graph_key)) {
      drop_graph();
      hipGraph_t graph = nullptr;
      // enqueue_tail flips the double-buffer parities on the HOST for every captured step; nothing has run on the device until the
      // graph is launched, so they are put back when the capture ends (a failure after an odd number of captured steps would otherwise
      // leave the host pointing at the stale halves)
      const int par0 = st_par;
      void* const gains0 = gains.p;
      void* const alt0 = gains_alt.p;
      auto undo = [&]() {
        st_par = par0;
        gains.p = gains0;
        gains_alt.p = alt0;
      };
      HIP_TRY(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
      int rc = CAL_OK;
      for (int k = 0; k < nsteps && rc == CAL_OK; ++k) rc = enqueue_step(s, freeze_model, cap);
      const hipError_t e = hipStreamEndCapture(stream, &graph);
      undo();  // on every path (after an even number of steps: the same values; said explicitly: the launch below is what moves the device)
      if (rc != CAL_OK) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
      }
      if (e != hipSuccess) return fail(CAL_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
      const hipError_t ei = hipGraphInstantiate(&graph_exec, graph, nullptr, nullptr, 0);
      (void)hipGraphDestroy(graph);
      if (ei != hipSuccess) {
        graph_exec = nullptr;
        return fail(CAL_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(ei));
      }
      graph_key = key;
    }
    HIP_TRY(hipGraphLaunch(graph_exec, stream));
    return CAL_OK;
  }
  int set_launch_mode(int mode) override {
    if (mode != CAL_LAUNCH_AUTO && mode != CAL_LAUNCH_KERNELS && mode != CAL_LAUNCH_ONE_TAIL && mode != CAL_LAUNCH_GRAPH)
      return fail(CAL_ERR_INVALID, "set_launch_mode: unknown mode %d", mode);
    launch_mode = mode;
    return CAL_OK;
  }

  int push_state() {
    for (int t = 0; t < nslices; ++t) {
      DevState& h = h_state[t];
      h.lr = opt.learning_rate;
      h.beta1 = opt.beta_1;
      h.beta2 = opt.beta_2;
      h.eps = opt.epsilon;
      h.opt = opt.optimizer;
      h.nesterov = opt.nesterov;
      h.momentum = opt.momentum;
      h.rho = opt.rho;
      h.ftrl[0] = opt.optimizer == CAL_OPT_LAMB ? opt.weight_decay_rate : opt.learning_rate_power;
      h.ftrl[1] = opt.l1_regularization_strength;
      h.ftrl[2] = opt.l2_regularization_strength + opt.beta / (2.0 * opt.learning_rate);
      h.ftrl[3] = opt.l2_shrinkage_regularization_strength;
      h.reg = reg == CAL_REG_SUM;
      h.f32 = std::is_same<T, float>::value ? 1 : 0;
      h.prior_r = prior_r_t[t];
      h.prior_i = prior_i_t[t];
    }
    HIP_TRY(hipMemcpyAsync(st_cur(), h_state, (size_t)nslices * sizeof(DevState), hipMemcpyHostToDevice, stream));
    return CAL_OK;
  }
  int pull_state() {
    HIP_TRY(hipMemcpyAsync(h_state, st_cur(), (size_t)nslices * sizeof(DevState), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return CAL_OK;
  }
  void begin_pass_state() {  // a one-off pass (loss, gradients, model, initial coefficients): no slice is stopped
    for (int t = 0; t < nslices; ++t) h_state[t].done = h_state[t].done_after = 0;
  }
  int collect_timing() {
    for (size_t i = 0; i < ev_used; ++i) {
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, ev_pool[i].first, ev_pool[i].second));
      t_total_ms += ms;
      ++t_launches;
    }
    ev_used = 0;
    return CAL_OK;
  }
  int ready() {
    if (!has_problem) return fail(CAL_ERR_STATE, "no problem set (cal_solver_set_problem)");
    if (!has_data) return fail(CAL_ERR_STATE, "no data set (cal_solver_set_data)");
    if (!has_gains || !has_coef) return fail(CAL_ERR_STATE, "gains and coefficients must both be set (cal_solver_set_params)");
    return CAL_OK;
  }

  // what the one-off evaluations share: no slice is stopped, one pass, the loop state back on the host, the timing
  int eval_pass(PassAsk ask, double* loss) {
    begin_pass_state();
    CAL_TRY(push_state());
    CAL_TRY(enqueue_pass(step_shape(ask), 0));
    CAL_TRY(pull_state());
    if (timing) CAL_TRY(collect_timing());
    if (loss) {  // several time slices: the sum of their losses (cal_solver_get_slice_losses has each)
      double tot = 0;
      for (int t = 0; t < nslices; ++t) tot += h_state[t].loss;
      *loss = tot;
    }
    return CAL_OK;
  }
  int eval(bool grads, double* loss, void* gg_r, void* gg_i, void* gc_r, void* gc_i) override {
    HIP_TRY(hipSetDevice(device));
    CAL_TRY(ready());
    CAL_TRY(eval_pass(grads ? kGradPass : kLossPass, loss));
    if (grads) {
      if (gg_r) CAL_TRY(download_rows(gg_r, comm.as<T>(), nants, 2, 0));
      if (gg_i) CAL_TRY(download_rows(gg_i, comm.as<T>(), nants, 2, 1));
      if (gc_r) HIP_TRY(copy_sync(gc_r, grad_c0(), (size_t)ncoef * sizeof(T), hipMemcpyDeviceToHost));
      if (gc_i) HIP_TRY(copy_sync(gc_i, grad_c0() + ncoef, (size_t)ncoef * sizeof(T), hipMemcpyDeviceToHost));
    }
    return CAL_OK;
  }

  int run(const cal_run_desc* r, double* losses_out, cal_run_result* res, bool per_slice) override {
    HIP_TRY(hipSetDevice(device));
    CAL_TRY(ready());
    if (!has_opt) return fail(CAL_ERR_STATE, "no optimizer set (cal_solver_set_optimizer)");
    if (!r || r->nsteps < 0) return fail(CAL_ERR_INVALID, "run: bad run description");
    if (!per_slice && nslices > 1)
      return fail(CAL_ERR_STATE, "run: the solver holds %d time slices, each with its own losses and stopping test: use cal_solver_run_slices", nslices);
    const int nres = per_slice ? nslices : 1;
    if (res) memset(res, 0, sizeof(*res) * nres);
    if (r->nsteps == 0) return CAL_OK;
    if (r->use_min && !gains_snap.p) {
      CAL_TRY(gains_snap.alloc(gains.bytes));
      CAL_TRY(coef_snap.alloc(coef.bytes));
    }
    if (r->use_min && yb_on() && !gb_ysnap.p) CAL_TRY(gb_ysnap.alloc(gb_y.bytes));
    const size_t lbytes = (size_t)nslices * r->nsteps * sizeof(double);
    if (r->record) CAL_TRY(losses.reserve(lbytes));
    if (!losses.p) CAL_TRY(losses.alloc((size_t)nslices * sizeof(double)));
    for (int t = 0; t < nslices; ++t) {
      DevState& h = h_state[t];
      h.done = held.empty() ? 0 : held[t];  // (cal_solver_hold_slices: a slice that ended its loop in an earlier call of a chunked run)
      h.done_after = 0;
      h.n_recorded = 0;
      h.nupdates = 0;
      h.improved = 0;
      h.nonfinite = 0;
      h.record = r->record ? 1 : 0;
      h.use_min = r->use_min ? 1 : 0;
      h.tol = r->tol;
    }
    CAL_TRY(push_state());
    // steps are enqueued in chunks; the device decides when the loop of a slice ends (finalize_kernel) and later steps of a
    // chunk fall through at once for it, so the host only synchronises once per chunk instead of once per step (:701)
    const int chunk = steps_per_sync;
    const int cap = r->record ? r->nsteps : 0;
    // the shape of every step of this call: its kernels, its update, launched one by one or replayed from a graph (step_plan.hpp)
    const StepShape shape = step_shape(train_step(yb_on()), r->nsteps);
    if (shape.tail1 && !gains_alt.p) CAL_TRY(gains_alt.alloc(gains.bytes));
    const int gsteps = shape.tail1 ? kGraphSteps : std::min(kGraphStepsLarge, chunk & ~1);  // even: the double-buffered loop state ends a replay where it began
    int issued = 0;
    while (issued < r->nsteps) {
      const int n = std::min(chunk, r->nsteps - issued);
      const bool mark = timing && roctx().push;
      if (mark) {
        char label[96];
        snprintf(label, sizeof(label), "calamity: train steps [%d, %d)%s", issued, issued + n, r->record ? "" : " (unrecorded)");
        roctx().push(label);
      }
      int s = 0;
      if (shape.replay)
        for (; gsteps >= 2 && s + gsteps <= n; s += gsteps) CAL_TRY(replay_steps(shape, r->freeze_model != 0, cap, gsteps));
      for (; s < n; ++s) CAL_TRY(enqueue_step(shape, r->freeze_model != 0, cap));
      issued += n;
      const int prc = pull_state();
      if (mark) roctx().pop();
      CAL_TRY(prc);
      if (timing) CAL_TRY(collect_timing());
      bool all_over = true;
      for (int t = 0; t < nslices; ++t) all_over = all_over && (h_state[t].done || h_state[t].done_after || h_state[t].nonfinite);
      if (all_over) break;
    }
    int bad = -1;
    for (int t = 0; t < nslices; ++t) {
      const DevState& h = h_state[t];
      if (res && t < nres) {
        res[t].nrecorded = h.n_recorded;
        res[t].stopped = (h.done || h.done_after) && !h.nonfinite ? 1 : 0;
        res[t].nupdates = h.nupdates;
        res[t].nonfinite = h.nonfinite ? 1 : 0;
      }
      if (r->record && losses_out && h.n_recorded > 0)
        HIP_TRY(copy_sync(losses_out + (size_t)t * r->nsteps, losses.as<double>() + (size_t)t * cap,
                          (size_t)std::min(h.n_recorded, r->nsteps) * sizeof(double), hipMemcpyDeviceToHost));
      if (h.nonfinite && bad < 0) bad = t;
    }
    if (bad >= 0) {
      if (nslices > 1) return fail(CAL_ERR_NONFINITE, "loss of time slice %d became non-finite after %d updates", bad, h_state[bad].nupdates);
      return fail(CAL_ERR_NONFINITE, "loss became non-finite after %d updates", h_state[bad].nupdates);
    }
    return CAL_OK;
  }

  int model(void* mr, void* mi, bool with_gains) override {
    HIP_TRY(hipSetDevice(device));
    if (!has_problem || !has_coef) return fail(CAL_ERR_STATE, "model: problem and coefficients must be set");
    if (with_gains && !has_gains) return fail(CAL_ERR_STATE, "data_model: the gains must be set");
    if (!mr || !mi) return fail(CAL_ERR_INVALID, "model: null output");
    const size_t rowbytes = (size_t)nbls * fpad * sizeof(T);
    CAL_TRY(model_buf.reserve(2 * rowbytes));
    begin_pass_state();
    CAL_TRY(push_state());
    const FusedArgs<T> a = model_args();
    launch_fused<MODE_MODEL>(a, false);
    if (with_gains)
      hipLaunchKernelGGL(apply_gains_kernel<T>, dim3(grid_for((long long)nbls * fpad)), dim3(256), 0, stream, a.model_r, a.model_i, gains.as<T2>(),
                         bl_ant.as<int2>(), (long long)nbls, fpad);
    HIP_TRY(hipGetLastError());
    CAL_TRY(download_rows(mr, a.model_r, nbls, 1, 0));
    CAL_TRY(download_rows(mi, a.model_i, nbls, 1, 0));
    return CAL_OK;
  }

  // ---- what fit_quality and the closed-form solves share --------------------------------------------------------------
  int require_set(const char* who, bool need_gains) {
    if (!has_problem) return fail(CAL_ERR_STATE, "%s: no problem set (cal_solver_set_problem)", who);
    if (!has_data) return fail(CAL_ERR_STATE, "%s: no data set (cal_solver_set_data)", who);
    if (!has_coef) return fail(CAL_ERR_STATE, "%s: the coefficients must be set (cal_solver_set_params)", who);
    if (need_gains && !has_gains) return fail(CAL_ERR_STATE, "%s: the gains must be set (cal_solver_set_params)", who);
    return CAL_OK;
  }
  // the gains a post-fit report reads: the solver's, or the planes given for this call alone ([nants][nfreqs]), uploaded into fq_gains
  int report_gains(const char* who, const void* g_r, const void* g_i, const T2** g) {
    if ((g_r == nullptr) != (g_i == nullptr)) return fail(CAL_ERR_INVALID, "%s: give both g_r and g_i, or neither", who);
    if (!g_r && !has_gains) return fail(CAL_ERR_STATE, "%s: the gains must be set (cal_solver_set_params) or given", who);
    *g = gains.as<T2>();
    if (!g_r) return CAL_OK;
    CAL_TRY(fq_gains.reserve((size_t)nants * fpad * sizeof(T2)));
    CAL_TRY(upload_rows(g_r, fq_gains.as<T>(), nants, 2, 0));
    CAL_TRY(upload_rows(g_i, fq_gains.as<T>(), nants, 2, 1));
    *g = fq_gains.as<T2>();
    return CAL_OK;
  }
  // a call's plan array on the device (the buffers are kept between calls: a fit asks for the same sizes for every slice); an empty
  // array is copied only where copy_empty says so
  template <typename X>
  int put(DevBuf& b, const std::vector<X>& v, bool copy_empty) {
    const size_t bytes = v.size() * sizeof(X);
    CAL_TRY(b.reserve(bytes, false));
    if (bytes || copy_empty) HIP_TRY(copy_sync(b.p, v.data(), bytes, hipMemcpyHostToDevice));
    return CAL_OK;
  }
  // an output the caller may leave out: n doubles to the host, on the stream
  int give(double* host, const double* dev, size_t n) {
    if (host) HIP_TRY(hipMemcpyAsync(host, dev, n * sizeof(double), hipMemcpyDeviceToHost, stream));
    return CAL_OK;
  }
  // The model pass of model() into model_buf ([planes][nbls][fpad]), then rows(model_r, model_i, q_rows) launches what turns the planes
  // into the call's own rows (q_rows: the third plane, null when two are asked for).  The host mirror of the loop state is put back and
  // pushed again afterwards: the pass clears the slices' stop flags for itself.
  template <typename Rows>
  int model_pass(int planes, Rows rows) {
    const size_t plane = (size_t)nbls * fpad;
    CAL_TRY(model_buf.reserve(planes * plane * sizeof(T)));
    PassGuard G;
    CAL_TRY(pass_begin(G));
    const FusedArgs<T> a = model_args();
    launch_fused<MODE_MODEL>(a, false);
    rows(a.model_r, a.model_i, planes == 3 ? model_buf.as<T>() + 2 * plane : nullptr);
    HIP_TRY(hipGetLastError());
    return pass_restore_state(G);
  }
  // The loop state around one-off passes: pass_begin saves the host mirror, clears the stop flags and pushes; pass_restore_state puts it
  // back and pushes again.  A Gauss-Newton or L-BFGS call holds one guard over all its passes, with what it has substituted: pass_end.
  struct PassGuard {
    bool data = false, coefs = false;
    std::vector<DevState> saved;
  };
  int pass_begin(PassGuard& G) {
    G.saved.assign(h_state, h_state + nslices);
    begin_pass_state();
    return push_state();
  }
  int pass_restore_state(const PassGuard& G) {
    std::copy(G.saved.begin(), G.saved.end(), h_state);
    return push_state();
  }

  // ---- the two launch shapes of the post-fit kernels: every row kernel and antenna kernel goes through these ---------------
  struct RowPlanes { T *u_r = nullptr, *u_i = nullptr, *q = nullptr; };  // the three planes of model_buf behind a rows kernel
  template <typename K, typename... A>
  void launch_rows(K kern, size_t lds, A... a) {  // one wave per baseline row, four rows per block (row_walk.hpp)
    hipLaunchKernelGGL(kern, dim3((nbls + 3) / 4), dim3(256), lds, stream, a...);
  }
  template <typename K, typename... A>
  void launch_ants(K kern, A... a) {  // block = (antenna, 64 V channels), channel-block major
    constexpr int V = 16 / (int)sizeof(T);
    const int cblocks = (fpad + 64 * V - 1) / (64 * V);
    hipLaunchKernelGGL(kern, dim3(nants * cblocks), dim3(256), 0, stream, a...);
  }
  void launch_gn_data(const T* jp_r, const T* jp_i, const GnScal* scal) {  // G m (+ s_t J p) from gn_m into the data planes
    launch_rows(gn_data_kernel<T>, 0, gn_m.as<T>(), gn_m.as<T>() + (size_t)nbls * fpad, jp_r, jp_i, gains.as<T2>(), bl_ant.as<int2>(), scal, na_slice,
                data_r.as<T>(), data_i.as<T>(), nbls, nfreqs, fpad);
  }
  // a call's slice mask on the device (gs_mask); *dev is null where the call has none
  int upload_slice_mask(const uint8_t* host, const unsigned char** dev) {
    *dev = nullptr;
    if (!host) return CAL_OK;
    CAL_TRY(gs_mask.reserve((size_t)nslices, false));
    HIP_TRY(copy_sync(gs_mask.p, host, (size_t)nslices, hipMemcpyHostToDevice));
    *dev = gs_mask.as<unsigned char>();
    return CAL_OK;
  }
  // fn(t, t1) for every run [t, t1) of neighbouring selected slices (no mask: one run of all)
  template <typename Fn>
  int for_selected_slice_runs(const uint8_t* mask, Fn fn) {
    for (int t = 0; t < nslices;) {
      if (mask && !mask[t]) {
        ++t;
        continue;
      }
      int t1 = t + 1;
      while (t1 < nslices && (!mask || mask[t1])) ++t1;
      CAL_TRY(fn(t, t1));
      t = t1;
    }
    return CAL_OK;
  }
  // what set_optimizer leaves in n reals of the moment slots m and v from element off on
  int reset_moment_slots(DevBuf& m, DevBuf& v, size_t off, size_t n) {
    HIP_TRY(hipMemsetAsync(m.as<T>() + off, 0, n * sizeof(T), stream));
    if ((opt.optimizer == CAL_OPT_ADAGRAD || opt.optimizer == CAL_OPT_FTRL) && opt.initial_accumulator_value != 0.0)
      hipLaunchKernelGGL(fill_kernel<T>, dim3(grid_for((long long)n)), dim3(256), 0, stream, v.as<T>() + off, (long long)n,
                         (T)opt.initial_accumulator_value);
    else
      HIP_TRY(hipMemsetAsync(v.as<T>() + off, 0, n * sizeof(T), stream));
    return CAL_OK;
  }
  // ... in the slots of the selected slices (no mask: all), one run of neighbouring slices at a time: gain_reals reals of the gain slots
  // gain_m, gain_v per slice (0: none of them) and, with_coeffs, the slice's run of both coefficient planes
  int reset_slice_moments(const uint8_t* mask, DevBuf& gain_m, DevBuf& gain_v, size_t gain_reals, bool with_coeffs) {
    CAL_TRY(for_selected_slice_runs(mask, [&](int t, int t1) {
      if (gain_reals) CAL_TRY(reset_moment_slots(gain_m, gain_v, (size_t)t * gain_reals, (size_t)(t1 - t) * gain_reals));
      const size_t n = with_coeffs ? (size_t)(h_slice_coff[t1] - h_slice_coff[t]) : 0;
      for (int plane = 0; plane < 2 && n > 0; ++plane) CAL_TRY(reset_moment_slots(coef_m, coef_v, (size_t)plane * ncoef + h_slice_coff[t], n));
      return (int)CAL_OK;
    }));
    HIP_TRY(hipGetLastError());
    return CAL_OK;
  }

  // cal_solver_fit_quality: the model pass of model(), then quality_rows_kernel and quality_ant_kernel (fit_quality_kernels.hpp).
  int fit_quality(const void* g_r, const void* g_i, double* chisq_ant, double* wsum_ant, double* chisq_bl, double* wsum_bl) override {
    HIP_TRY(hipSetDevice(device));
    CAL_TRY(require_set("fit_quality", false));
    const T2* g = nullptr;
    CAL_TRY(report_gains("fit_quality", g_r, g_i, &g));
    const size_t nant_out = (size_t)nants * nfreqs;
    const size_t out_bytes = (2 * nant_out + 2 * (size_t)nbls) * sizeof(double);
    CAL_TRY(fq_out.reserve(out_bytes));
    double* o_ca = fq_out.as<double>();
    double* o_wa = o_ca + nant_out;
    double* o_cb = o_wa + nant_out;
    double* o_wb = o_cb + nbls;
    CAL_TRY(model_pass(2, [&](T* model_r, T* model_i, T*) {
      launch_rows(quality_rows_kernel<T>, 0, model_r, model_i, data_r.as<T>(), data_i.as<T>(), wgts.as<T>(), g, bl_ant.as<int2>(), nbls, nfreqs,
                  fpad, o_cb, o_wb);
      launch_ants(quality_ant_kernel<T>, model_r, wgts.as<T>(), ant_ptr.as<int>(), ant_ent.as<int2>(), nants, nfreqs, fpad, o_ca, o_wa);
    }));
    // the antenna planes of every rank's baselines add up to the array's: ONE all-reduce of 2 nants nfreqs doubles
    if (comm_on()) CAL_TRY(all_reduce(o_ca, 2 * nant_out, CAL_XCHG_F64, CAL_XCHG_SUM));
    CAL_TRY(give(chisq_ant, o_ca, nant_out));
    CAL_TRY(give(wsum_ant, o_wa, nant_out));
    CAL_TRY(give(chisq_bl, o_cb, (size_t)nbls));
    CAL_TRY(give(wsum_bl, o_wb, (size_t)nbls));
    HIP_TRY(hipStreamSynchronize(stream));
    return CAL_OK;
  }

  // cal_solver_delay_spectrum: the model pass of model(), then per chunk of rows dspec_rows_kernel, dspec_transform_kernel and
  // dspec_bin_kernel (delay_spectrum_kernels.hpp).  A chunk's scratch -- the masked planes in T and, when power_bl or bins are asked
  // for, its power in double -- stays under ds_bound; the chunks are cut at multiples of the transform's 128 rows where that fits.
  int delay_spectrum(const cal_delay_spectrum_desc* d, const void* g_r, const void* g_i, double* power_bl, double* norm_bl, double* power_bin,
                     double* count_bin) override {
    HIP_TRY(hipSetDevice(device));
    if (!d) return fail(CAL_ERR_INVALID, "delay_spectrum: null description");
    CAL_TRY(require_set("delay_spectrum", false));
    const T2* g = nullptr;
    CAL_TRY(report_gains("delay_spectrum", g_r, g_i, &g));
    if (d->ndelays < 1 || d->ndelays > 4096) return fail(CAL_ERR_INVALID, "delay_spectrum: ndelays = %d lies outside [1, 4096]", d->ndelays);
    if ((d->what & 7) == 0 || (d->what & ~7)) return fail(CAL_ERR_INVALID, "delay_spectrum: what = %d: bits 0 (data), 1 (model), 2 (residual), at least one", d->what);
    if (d->calibrated != 0 && d->calibrated != 1) return fail(CAL_ERR_INVALID, "delay_spectrum: calibrated = %d (0 or 1)", d->calibrated);
    if (!d->op_r || !d->op_i || !d->norm_f) return fail(CAL_ERR_INVALID, "delay_spectrum: null operator or norm_f");
    if (d->nbins < 0) return fail(CAL_ERR_INVALID, "delay_spectrum: nbins = %d", d->nbins);
    if ((d->nbins == 0) != (d->bin_of_bl == nullptr)) return fail(CAL_ERR_INVALID, "delay_spectrum: bin_of_bl goes with nbins > 0, and only with it");
    if (d->nbins == 0 && (power_bin || count_bin)) return fail(CAL_ERR_INVALID, "delay_spectrum: binned outputs need nbins > 0");
    const bool with_power = power_bl != nullptr || d->nbins > 0;
    DelaySpectrumPlan<T> P;  // the bins' rows, the chunks, the operator image (report_plan.hpp)
    CAL_TRY(plan_delay_spectrum(nbls, nfreqs, fpad, d, ds_bound, with_power, P));
    const int nd = d->ndelays, nbins = d->nbins, nq = P.nq, xpitch = P.xpitch, ndpad = P.ndpad, crows = P.crows;
    CAL_TRY(put(ds_op, P.image, false));
    CAL_TRY(put(ds_normf, P.norm_f, false));
    if (nbins) {
      CAL_TRY(put(ds_ent, P.bin_ent, false));
      CAL_TRY(put(ds_ptr, P.chunk_ptr, false));
    }
    CAL_TRY(ds_out.reserve(P.n_out * sizeof(double)));
    CAL_TRY(ds_x.reserve(P.n_x * sizeof(T), false));
    if (with_power) CAL_TRY(ds_pow.reserve(P.n_pow * sizeof(double), false));
    const size_t nbin_out = P.n_out - nbls;  // power_bin | count_bin: the exchange payload
    double* o_norm = ds_out.as<double>();
    double* o_pbin = o_norm + nbls;
    double* o_cbin = o_pbin + (size_t)nq * nbins * nd;
    hipError_t copy_err = hipSuccess;
    CAL_TRY(model_pass(2, [&](T* model_r, T* model_i, T*) {
      for (int c = 0; c < P.nchunks; ++c) {
        const long long b0 = (long long)c * crows;
        const int nr = (int)std::min<long long>(crows, nbls - b0);
        const size_t off = (size_t)b0 * fpad;
        hipLaunchKernelGGL(dspec_rows_kernel<T>, dim3((nr + 3) / 4), dim3(256), 0, stream, model_r + off, model_i + off, data_r.as<T>() + off,
                           data_i.as<T>() + off, wgts.as<T>() + off, g, bl_ant.as<int2>() + b0, ds_normf.as<double>(), nr, nfreqs, fpad, xpitch,
                           d->what, d->calibrated, ds_x.as<T>(), o_norm + b0);
        if (!with_power) continue;
        hipLaunchKernelGGL(dspec_transform_kernel<T>, dim3((nr + kDsRows - 1) / kDsRows, ndpad / kDsCols, nq), dim3(256), 0, stream, ds_x.as<T>(),
                           ds_op.as<T>(), o_norm + b0, nr, xpitch, nd, ndpad, ds_pow.as<double>());
        if (nbins)
          hipLaunchKernelGGL(dspec_bin_kernel, dim3(nbins, (nd + 255) / 256, nq), dim3(256), 0, stream, ds_pow.as<double>(), o_norm + b0,
                             ds_ptr.as<int>() + (size_t)c * nbins * 2, ds_ent.as<int>(), (int)b0, nr, nd, nbins, c == 0 ? 1 : 0, o_pbin, o_cbin);
        for (int q = 0; q < nq && power_bl && copy_err == hipSuccess; ++q)  // (the stream orders the copy before the next chunk's kernels)
          copy_err = hipMemcpyAsync(power_bl + ((size_t)q * nbls + b0) * nd, ds_pow.as<double>() + (size_t)q * nr * nd, (size_t)nr * nd * sizeof(double),
                                    hipMemcpyDeviceToHost, stream);
      }
    }));
    HIP_TRY(copy_err);
    // the bins of every rank's rows add up to the array's: ONE all-reduce of nwhat nbins ndelays + nbins doubles
    if (nbins && comm_on()) CAL_TRY(all_reduce(o_pbin, nbin_out, CAL_XCHG_F64, CAL_XCHG_SUM));
    CAL_TRY(give(norm_bl, o_norm, (size_t)nbls));
    CAL_TRY(give(power_bin, o_pbin, (size_t)nq * nbins * nd));
    CAL_TRY(give(count_bin, o_cbin, (size_t)nbins));
    HIP_TRY(hipStreamSynchronize(stream));
    return CAL_OK;
  }
  int set_delay_spectrum_scratch(int64_t bytes) override {
    if (bytes < 0) return fail(CAL_ERR_INVALID, "set_delay_spectrum_scratch: negative bound");
    ds_bound = bytes == 0 ? kCsScratchDefault : bytes;
    for (DevBuf* b : {&ds_x, &ds_pow}) b->release();
    return CAL_OK;
  }

  // cal_solver_delay_cross_spectrum: the model pass of model(), then per chunk of pairs dcross_rows_kernel, dcross_transform_kernel
  // (delay_cross_kernels.hpp) and dspec_bin_kernel as it is, over pairs instead of rows and with nstat nq planes.  The buffers are
  // those of delay_spectrum and the bound is ds_bound; the chunks are cut at multiples of the transform's 64 pairs where that fits.
  int delay_cross_spectrum(const cal_delay_cross_desc* d, const void* g_r, const void* g_i, double* cross_pair, double* diff_pair, double* norm_pair,
                           double* cross_bin, double* diff_bin, double* count_bin) override {
    HIP_TRY(hipSetDevice(device));
    if (!d) return fail(CAL_ERR_INVALID, "delay_cross_spectrum: null description");
    CAL_TRY(require_set("delay_cross_spectrum", false));
    const T2* g = nullptr;
    CAL_TRY(report_gains("delay_cross_spectrum", g_r, g_i, &g));
    if (d->ndelays < 1 || d->ndelays > 4096) return fail(CAL_ERR_INVALID, "delay_cross_spectrum: ndelays = %d lies outside [1, 4096]", d->ndelays);
    if ((d->what & 7) == 0 || (d->what & ~7))
      return fail(CAL_ERR_INVALID, "delay_cross_spectrum: what = %d: bits 0 (data), 1 (model), 2 (residual), at least one", d->what);
    if (d->calibrated != 0 && d->calibrated != 1) return fail(CAL_ERR_INVALID, "delay_cross_spectrum: calibrated = %d (0 or 1)", d->calibrated);
    if (!d->op_r || !d->op_i || !d->norm_f) return fail(CAL_ERR_INVALID, "delay_cross_spectrum: null operator or norm_f");
    if (d->nbins < 0) return fail(CAL_ERR_INVALID, "delay_cross_spectrum: nbins = %d", d->nbins);
    if ((d->nbins == 0) != (d->bin_of_pair == nullptr)) return fail(CAL_ERR_INVALID, "delay_cross_spectrum: bin_of_pair goes with nbins > 0, and only with it");
    if (d->nbins == 0 && (cross_bin || diff_bin || count_bin)) return fail(CAL_ERR_INVALID, "delay_cross_spectrum: binned outputs need nbins > 0");
    if (!(d->stats & 1) && (cross_pair || cross_bin)) return fail(CAL_ERR_INVALID, "delay_cross_spectrum: cross outputs need bit 0 of stats (stats = %d)", d->stats);
    if (!(d->stats & 2) && (diff_pair || diff_bin)) return fail(CAL_ERR_INVALID, "delay_cross_spectrum: diff outputs need bit 1 of stats (stats = %d)", d->stats);
    DelayCrossPlan<T> P;  // the refusals of pairs, stats and scales; the bins' pairs, the chunks, the operator image (report_plan.hpp)
    CAL_TRY(plan_delay_cross(nbls, nfreqs, fpad, d, ds_bound, P));
    const int nd = d->ndelays, nbins = d->nbins, np = d->npairs, nq = P.nq, nstat = P.nstat, xpitch = P.xpitch, ndpad = P.ndpad, cpairs = P.cpairs;
    CAL_TRY(put(ds_op, P.image, false));
    CAL_TRY(put(ds_normf, P.norm_f, false));
    CAL_TRY(put(dc_scale, P.scale, false));
    CAL_TRY(dc_pairs.reserve(2 * (size_t)np * sizeof(int32_t), false));
    HIP_TRY(copy_sync(dc_pairs.p, d->pairs, 2 * (size_t)np * sizeof(int32_t), hipMemcpyHostToDevice));
    if (nbins) {
      CAL_TRY(put(ds_ent, P.bin_ent, false));
      CAL_TRY(put(ds_ptr, P.chunk_ptr, false));
    }
    CAL_TRY(ds_out.reserve(P.n_out * sizeof(double)));
    CAL_TRY(ds_x.reserve(P.n_x * sizeof(T), false));
    CAL_TRY(ds_pow.reserve(P.n_pow * sizeof(double), false));
    const size_t nbin_stat = (size_t)nq * nbins * nd;   // one statistic's bins
    const size_t nbin_out = P.n_out - np;                // cross_bin | diff_bin | count_bin: the exchange payload
    double* o_norm = ds_out.as<double>();
    double* o_sbin = o_norm + np;
    double* o_cbin = o_sbin + (size_t)nstat * nbin_stat;
    double* pair_out[2] = {cross_pair, diff_pair};
    hipError_t copy_err = hipSuccess;
    CAL_TRY(model_pass(2, [&](T* model_r, T* model_i, T*) {
      for (int c = 0; c < P.nchunks; ++c) {
        const long long p0 = (long long)c * cpairs;
        const int nc = (int)std::min<long long>(cpairs, np - p0);
        hipLaunchKernelGGL(dcross_rows_kernel<T>, dim3((nc + 3) / 4), dim3(256), 0, stream, model_r, model_i, data_r.as<T>(), data_i.as<T>(), wgts.as<T>(), g,
                           bl_ant.as<int2>(), dc_pairs.as<int2>() + p0, ds_normf.as<double>(), nc, nfreqs, fpad, xpitch, d->what, d->calibrated,
                           ds_x.as<T>(), o_norm + p0);
        hipLaunchKernelGGL(dcross_transform_kernel<T>, dim3((nc + kDcPairs - 1) / kDcPairs, ndpad / kDsCols, nq), dim3(256), 0, stream, ds_x.as<T>(),
                           ds_op.as<T>(), o_norm + p0, dc_scale.as<double>() + 2 * p0, nc, xpitch, nd, ndpad, d->stats, ds_pow.as<double>());
        if (nbins)
          hipLaunchKernelGGL(dspec_bin_kernel, dim3(nbins, (nd + 255) / 256, nstat * nq), dim3(256), 0, stream, ds_pow.as<double>(), o_norm + p0,
                             ds_ptr.as<int>() + (size_t)c * nbins * 2, ds_ent.as<int>(), (int)p0, nc, nd, nbins, c == 0 ? 1 : 0, o_sbin, o_cbin);
        int slot = 0;
        for (int st = 0; st < 2; ++st) {
          if (!(d->stats >> st & 1)) continue;
          for (int q = 0; q < nq && pair_out[st] && copy_err == hipSuccess; ++q)  // (the stream orders the copy before the next chunk's kernels)
            copy_err = hipMemcpyAsync(pair_out[st] + ((size_t)q * np + p0) * nd, ds_pow.as<double>() + ((size_t)slot * nq + q) * nc * nd,
                                      (size_t)nc * nd * sizeof(double), hipMemcpyDeviceToHost, stream);
          ++slot;
        }
      }
    }));
    HIP_TRY(copy_err);
    // the bins of every rank's pairs add up to the array's: ONE all-reduce of nstat nwhat nbins ndelays + nbins doubles
    if (nbins && comm_on()) CAL_TRY(all_reduce(o_sbin, nbin_out, CAL_XCHG_F64, CAL_XCHG_SUM));
    CAL_TRY(give(norm_pair, o_norm, (size_t)np));
    CAL_TRY(give(cross_bin, o_sbin, nbin_stat));
    CAL_TRY(give(diff_bin, o_sbin + ((d->stats & 1) ? nbin_stat : 0), nbin_stat));
    CAL_TRY(give(count_bin, o_cbin, (size_t)nbins));
    HIP_TRY(hipStreamSynchronize(stream));
    return CAL_OK;
  }

  // cal_solver_delay_fringe_spectrum: the model pass of model(), then per chunk of whole groups dfringe_rows_kernel,
  // dfringe_transform_kernel, dfringe_time_kernel (delay_fringe_kernels.hpp) and dspec_bin_kernel as it is, over groups instead of rows
  // and with nrates ndelays columns.  The buffers are those of delay_spectrum and the bound is ds_bound.
  int delay_fringe_spectrum(const cal_delay_fringe_desc* d, const void* g_r, const void* g_i, double* power_grp, double* norm_grp, double* power_bin,
                            double* count_bin) override {
    HIP_TRY(hipSetDevice(device));
    if (!d) return fail(CAL_ERR_INVALID, "delay_fringe_spectrum: null description");
    CAL_TRY(require_set("delay_fringe_spectrum", false));
    const T2* g = nullptr;
    CAL_TRY(report_gains("delay_fringe_spectrum", g_r, g_i, &g));
    if (d->ndelays < 1 || d->ndelays > 4096) return fail(CAL_ERR_INVALID, "delay_fringe_spectrum: ndelays = %d lies outside [1, 4096]", d->ndelays);
    if ((d->what & 7) == 0 || (d->what & ~7))
      return fail(CAL_ERR_INVALID, "delay_fringe_spectrum: what = %d: bits 0 (data), 1 (model), 2 (residual), at least one", d->what);
    if (d->calibrated != 0 && d->calibrated != 1) return fail(CAL_ERR_INVALID, "delay_fringe_spectrum: calibrated = %d (0 or 1)", d->calibrated);
    if (!d->op_r || !d->op_i || !d->norm_f) return fail(CAL_ERR_INVALID, "delay_fringe_spectrum: null operator or norm_f");
    if (d->nbins < 0) return fail(CAL_ERR_INVALID, "delay_fringe_spectrum: nbins = %d", d->nbins);
    if ((d->nbins == 0) != (d->bin_of_group == nullptr)) return fail(CAL_ERR_INVALID, "delay_fringe_spectrum: bin_of_group goes with nbins > 0, and only with it");
    if (d->nbins == 0 && (power_bin || count_bin)) return fail(CAL_ERR_INVALID, "delay_fringe_spectrum: binned outputs need nbins > 0");
    DelayFringePlan<T> P;  // the refusals of groups, rows, scales and opt; the bins' groups, the chunks, the operator image (report_plan.hpp)
    CAL_TRY(plan_delay_fringe(nbls, nfreqs, fpad, d, ds_bound, P));
    const int ng = d->ngroups, nt = d->ntimes;
    FringeRun R;
    CAL_TRY(fringe_begin(d->ndelays, d->nbins, ng, nt, d->nrates, P, power_grp, R));
    CAL_TRY(dc_pairs.reserve((size_t)ng * nt * sizeof(int32_t), false));
    HIP_TRY(copy_sync(dc_pairs.p, d->rows, (size_t)ng * nt * sizeof(int32_t), hipMemcpyHostToDevice));
    CAL_TRY(model_pass(2, [&](T* model_r, T* model_i, T*) {
      for (int c = 0; c < P.nchunks; ++c) {
        const long long g0 = (long long)c * P.cgroups;
        const int nc = (int)std::min<long long>(P.cgroups, ng - g0);
        hipLaunchKernelGGL(dfringe_rows_kernel<T>, dim3((nc + 3) / 4), dim3(256), 0, stream, model_r, model_i, data_r.as<T>(), data_i.as<T>(), wgts.as<T>(), g,
                           bl_ant.as<int2>(), dc_pairs.as<int>() + g0 * nt, ds_normf.as<double>(), nc, nt, nfreqs, fpad, P.xpitch, d->what, d->calibrated,
                           ds_x.as<T>(), R.o_norm + g0);
        fringe_chunk_tail(R, c, g0, nc);
      }
    }));
    return fringe_end(R, norm_grp, power_bin, count_bin);
  }

  // What cal_solver_delay_fringe_spectrum and cal_solver_delay_coherent_spectrum share from the masked planes x on: the plan's arrays
  // on the device and the outputs' places (fringe_begin), per chunk dfringe_transform_kernel, dfringe_time_kernel, dspec_bin_kernel and
  // the copies of the per-group power (fringe_chunk_tail; the chunk's x in ds_x and its norm_grp are there), then the all-reduce of the
  // bins and the outputs (fringe_end).
  struct FringeRun {
    int nd, nbins, ng, nt, nr, nq, xpitch, ndpad, ncols;
    size_t nbin_out, time_lds;
    double *o_norm, *o_pbin, *o_cbin, *y, *pw, *power_grp;
    const double *opt_r, *opt_i;
    hipError_t copy_err;
  };
  int fringe_begin(int nd, int nbins, int ng, int nt, int nr, const DelayFringePlan<T>& P, double* power_grp, FringeRun& R) {
    CAL_TRY(put(ds_op, P.image, false));
    CAL_TRY(put(ds_normf, P.norm_f, false));
    CAL_TRY(put(dc_scale, P.scale, false));
    CAL_TRY(put(df_opt, P.opt, false));
    if (nbins) {
      CAL_TRY(put(ds_ent, P.bin_ent, false));
      CAL_TRY(put(ds_ptr, P.chunk_ptr, false));
    }
    CAL_TRY(ds_out.reserve(P.n_out * sizeof(double)));
    CAL_TRY(ds_x.reserve(P.n_x * sizeof(T), false));
    CAL_TRY(ds_pow.reserve((P.n_y + P.n_pow) * sizeof(double), false));
    R.nd = nd, R.nbins = nbins, R.ng = ng, R.nt = nt, R.nr = nr, R.nq = P.nq, R.xpitch = P.xpitch, R.ndpad = P.ndpad;
    R.ncols = nr * nd;               // columns of a group's power: [nrates][ndelays]
    R.nbin_out = P.n_out - ng;       // power_bin | count_bin: the exchange payload
    R.o_norm = ds_out.as<double>();
    R.o_pbin = R.o_norm + ng;
    R.o_cbin = R.o_pbin + (size_t)P.nq * nbins * R.ncols;
    R.y = ds_pow.as<double>();
    R.pw = R.y + P.n_y;
    R.opt_r = df_opt.as<double>();
    R.opt_i = R.opt_r + (size_t)nt * nr;
    R.time_lds = (size_t)nt * 2 * kDfCols * sizeof(double);
    R.power_grp = power_grp;
    R.copy_err = hipSuccess;
    return CAL_OK;
  }
  void fringe_chunk_tail(FringeRun& R, int c, long long g0, int nc) {
    const int nrows = nc * R.nt, nd = R.nd, nq = R.nq, nbins = R.nbins, ncols = R.ncols;
    hipLaunchKernelGGL(dfringe_transform_kernel<T>, dim3((nrows + kDsRows - 1) / kDsRows, R.ndpad / kDsCols, nq), dim3(256), 0, stream, ds_x.as<T>(),
                       ds_op.as<T>(), dc_scale.as<double>() + g0 * R.nt, nrows, R.xpitch, nd, R.ndpad, R.y);
    hipLaunchKernelGGL(dfringe_time_kernel, dim3(nc, (nd + kDfCols - 1) / kDfCols, nq), dim3(256), R.time_lds, stream, R.y, R.opt_r, R.opt_i, R.o_norm + g0, nc,
                       R.nt, R.nr, nd, R.pw);
    if (nbins)
      hipLaunchKernelGGL(dspec_bin_kernel, dim3(nbins, (ncols + 255) / 256, nq), dim3(256), 0, stream, R.pw, R.o_norm + g0,
                         ds_ptr.as<int>() + (size_t)c * nbins * 2, ds_ent.as<int>(), (int)g0, nc, ncols, nbins, c == 0 ? 1 : 0, R.o_pbin, R.o_cbin);
    for (int q = 0; q < nq && R.power_grp && R.copy_err == hipSuccess; ++q)  // (the stream orders the copy before the next chunk's kernels)
      R.copy_err = hipMemcpyAsync(R.power_grp + ((size_t)q * R.ng + g0) * ncols, R.pw + (size_t)q * nc * ncols, (size_t)nc * ncols * sizeof(double),
                                  hipMemcpyDeviceToHost, stream);
  }
  int fringe_end(FringeRun& R, double* norm_grp, double* power_bin, double* count_bin) {
    HIP_TRY(R.copy_err);
    // the bins of every rank's groups add up to the array's: ONE all-reduce of nwhat nbins nrates ndelays + nbins doubles
    if (R.nbins && comm_on()) CAL_TRY(all_reduce(R.o_pbin, R.nbin_out, CAL_XCHG_F64, CAL_XCHG_SUM));
    CAL_TRY(give(norm_grp, R.o_norm, (size_t)R.ng));
    CAL_TRY(give(power_bin, R.o_pbin, (size_t)R.nq * R.nbins * R.ncols));
    CAL_TRY(give(count_bin, R.o_cbin, (size_t)R.nbins));
    HIP_TRY(hipStreamSynchronize(stream));
    return CAL_OK;
  }

  // cal_solver_delay_coherent_spectrum: the model pass of model(), then per chunk of whole groups dcoherent_rows_kernel and
  // dcoherent_mask_kernel (delay_coherent_kernels.hpp) for the averaged planes, and the fringe call's tail as it is.  The member lists
  // are uploaded once; the buffers are those of delay_spectrum and the bound is ds_bound.
  int delay_coherent_spectrum(const cal_delay_coherent_desc* d, const void* g_r, const void* g_i, double* power_grp, double* norm_grp, double* power_bin,
                              double* count_bin) override {
    HIP_TRY(hipSetDevice(device));
    if (!d) return fail(CAL_ERR_INVALID, "delay_coherent_spectrum: null description");
    CAL_TRY(require_set("delay_coherent_spectrum", false));
    const T2* g = nullptr;
    CAL_TRY(report_gains("delay_coherent_spectrum", g_r, g_i, &g));
    if (d->ndelays < 1 || d->ndelays > 4096) return fail(CAL_ERR_INVALID, "delay_coherent_spectrum: ndelays = %d lies outside [1, 4096]", d->ndelays);
    if ((d->what & 7) == 0 || (d->what & ~7))
      return fail(CAL_ERR_INVALID, "delay_coherent_spectrum: what = %d: bits 0 (data), 1 (model), 2 (residual), at least one", d->what);
    if (d->calibrated != 0 && d->calibrated != 1) return fail(CAL_ERR_INVALID, "delay_coherent_spectrum: calibrated = %d (0 or 1)", d->calibrated);
    if (!d->op_r || !d->op_i || !d->norm_f) return fail(CAL_ERR_INVALID, "delay_coherent_spectrum: null operator or norm_f");
    if (d->nbins < 0) return fail(CAL_ERR_INVALID, "delay_coherent_spectrum: nbins = %d", d->nbins);
    if ((d->nbins == 0) != (d->bin_of_group == nullptr)) return fail(CAL_ERR_INVALID, "delay_coherent_spectrum: bin_of_group goes with nbins > 0, and only with it");
    if (d->nbins == 0 && (power_bin || count_bin)) return fail(CAL_ERR_INVALID, "delay_coherent_spectrum: binned outputs need nbins > 0");
    DelayCoherentPlan<T> P;  // every other refusal; the fringe plan over the averaged planes, the member lists (report_plan.hpp)
    CAL_TRY(plan_delay_coherent(nbls, nfreqs, fpad, d, ds_bound, P));
    const int ng = d->ngroups, nt = d->ntimes;
    FringeRun R;
    CAL_TRY(fringe_begin(d->ndelays, d->nbins, ng, nt, d->nrates, P.F, power_grp, R));
    CAL_TRY(put(dk_ptr, P.set_ptr, false));
    CAL_TRY(put(dk_row, P.member_row, false));
    CAL_TRY(put(dk_wgt, P.member_wgt, false));
    CAL_TRY(put(dk_conj, P.member_conj, false));
    CAL_TRY(dk_mask.reserve(P.n_mask, false));
    CAL_TRY(model_pass(2, [&](T* model_r, T* model_i, T*) {
      for (int c = 0; c < P.F.nchunks; ++c) {
        const long long g0 = (long long)c * P.F.cgroups;
        const int nc = (int)std::min<long long>(P.F.cgroups, ng - g0);
        const long long nwaves = (long long)nc * nt * P.nspans;
        hipLaunchKernelGGL(dcoherent_rows_kernel<T>, dim3((unsigned)((nwaves + 3) / 4)), dim3(256), 0, stream, model_r, model_i, data_r.as<T>(), data_i.as<T>(),
                           wgts.as<T>(), g, bl_ant.as<int2>(), dk_ptr.as<long long>() + g0 * nt, dk_row.as<int>(), dk_wgt.as<double>(),
                           dk_conj.as<unsigned char>(), nc * nt, P.nspans, nfreqs, fpad, P.F.xpitch, d->what, d->calibrated, d->weighting, ds_x.as<T>(),
                           dk_mask.as<unsigned char>());
        hipLaunchKernelGGL(dcoherent_mask_kernel<T>, dim3((nc + 3) / 4), dim3(256), 0, stream, dk_mask.as<unsigned char>(), ds_normf.as<double>(), nc, nt,
                           P.F.xpitch, 2 * P.F.nq, ds_x.as<T>(), R.o_norm + g0);
        fringe_chunk_tail(R, c, g0, nc);
      }
    }));
    return fringe_end(R, norm_grp, power_bin, count_bin);
  }

  // cal_solver_delay_transfer: the model pass of model() and coeff_solve_rows_kernel for q (at the call's gains), then per chunk of
  // groups coeff_gram_kernel and fit_error_factor_kernel (both as they are; rhs and coeff_var are not used), dtransfer_basis_kernel and
  // dtransfer_power_kernel (delay_transfer_kernels.hpp), then dspec_bin_kernel (as it is) once over all rows.  The plan
  // (report_plan.hpp) is made and uploaded at every call; fit_errors' and solve_coeffs' own plans stay where they are.
  int delay_transfer(const cal_delay_transfer_desc* d, const void* g_r, const void* g_i, double* absorbed_bl, double* noise_bl, double* absorbed_bin,
                     double* count_bin, cal_fit_errors_counts* counts) override {
    HIP_TRY(hipSetDevice(device));
    if (!d) return fail(CAL_ERR_INVALID, "delay_transfer: null description");
    CAL_TRY(require_set("delay_transfer", false));
    if ((g_r == nullptr) != (g_i == nullptr)) return fail(CAL_ERR_INVALID, "delay_transfer: give both g_r and g_i, or neither");
    if (!g_r && !has_gains) return fail(CAL_ERR_STATE, "delay_transfer: the gains must be set (cal_solver_set_params) or given");
    if (d->ndelays < 1 || d->ndelays > 4096) return fail(CAL_ERR_INVALID, "delay_transfer: ndelays = %d lies outside [1, 4096]", d->ndelays);
    if (d->calibrated != 0 && d->calibrated != 1) return fail(CAL_ERR_INVALID, "delay_transfer: calibrated = %d (0 or 1)", d->calibrated);
    if (!(d->ridge >= 0.0) || !std::isfinite(d->ridge)) return fail(CAL_ERR_INVALID, "delay_transfer: ridge = %g must be finite and >= 0", d->ridge);
    if (!d->op_r || !d->op_i) return fail(CAL_ERR_INVALID, "delay_transfer: null operator");
    if (d->nbins < 0) return fail(CAL_ERR_INVALID, "delay_transfer: nbins = %d", d->nbins);
    if ((d->nbins == 0) != (d->bin_of_bl == nullptr)) return fail(CAL_ERR_INVALID, "delay_transfer: bin_of_bl goes with nbins > 0, and only with it");
    if (d->nbins == 0 && (absorbed_bin || count_bin)) return fail(CAL_ERR_INVALID, "delay_transfer: binned outputs need nbins > 0");
    DelayTransferPlan<T> P;  // the chunks of groups, their runs and rows, the bins' rows, the operator image (report_plan.hpp)
    CAL_TRY(plan_delay_transfer(h_cs_grp, h_bl_tile, nbls, nfreqs, fpad, fold, d, dt_bound, P));
    const T2* g = nullptr;
    CAL_TRY(report_gains("delay_transfer", g_r, g_i, &g));
    const int nd = d->ndelays, nbins = d->nbins, xpitch = P.xpitch, ndpad = P.ndpad;
    CAL_TRY(put(dt_grp, P.grp, false));
    CAL_TRY(put(dt_order, P.G.order, false));
    CAL_TRY(put(dt_work, P.G.work, false));
    CAL_TRY(put(dt_woff, P.G.xoff, false));
    CAL_TRY(put(dt_runs, P.runs, false));
    CAL_TRY(put(dt_rows, P.rows, false));
    CAL_TRY(put(dt_op, P.image, false));
    if (nbins) {
      CAL_TRY(put(dt_ent, P.bin_ent, false));
      CAL_TRY(put(dt_ptr, P.bin_ptr2, false));
    }
    CAL_TRY(dt_n.reserve((size_t)P.G.n_max * sizeof(T), false));
    CAL_TRY(dt_d.reserve((size_t)P.G.d_max * sizeof(double), false));
    CAL_TRY(dt_x.reserve((size_t)P.G.x_max * sizeof(T), false));
    CAL_TRY(dt_rhs.reserve(2 * (size_t)ncoef * sizeof(T)));
    CAL_TRY(dt_cv.reserve((size_t)ncoef * sizeof(double), false));
    CAL_TRY(dt_ok.reserve(((size_t)ngrps + 2) * sizeof(int)));
    CAL_TRY(dt_out.reserve(P.n_out * sizeof(double)));
    const bool want_abs = absorbed_bl != nullptr || nbins > 0;
    if (want_abs) CAL_TRY(dt_abs.reserve(P.n_rows_out * sizeof(double), false));
    if (noise_bl) CAL_TRY(dt_noise.reserve(P.n_rows_out * sizeof(double), false));
    CAL_TRY(allow_chol_lds(&fit_error_factor_kernel<T>));
    double* o_valid = dt_out.as<double>();
    double* o_abin = o_valid + nbls;
    double* o_cbin = o_abin + (size_t)nbins * nd;
    int* ok = dt_ok.as<int>();
    int* dcnt = ok + ngrps;
    int cnt[2] = {0, 0};
    RowPlanes R;
    CAL_TRY(coeff_planes(R, g));
    HIP_TRY(hipMemsetAsync(dt_ok.p, 0, ((size_t)ngrps + 2) * sizeof(int), stream));
    HIP_TRY(hipMemsetAsync(o_valid, 0, (size_t)nbls * sizeof(double), stream));
    for (const TransferChunk& ch : P.chunks) {
      // S is zero where the basis kernel writes nothing (the channels [nfreqs, xpitch)); W is written whole
      HIP_TRY(hipMemsetAsync(dt_x.p, 0, (size_t)P.G.x_max * sizeof(T), stream));
      hipLaunchKernelGGL(coeff_gram_kernel<T>, dim3(ch.w1 - ch.w0), dim3(256), 0, stream, tiles.as<T>(), bl_tile.as<long long>(), R.u_r, R.u_i, R.q,
                         dt_grp.as<CsGroup>(), dt_work.as<CsWork>() + ch.w0, dt_n.as<T>(), dt_rhs.as<T>(), ncoef, nfreqs, fpad, fold ? 1 : 0);
      hipLaunchKernelGGL(fit_error_factor_kernel<T>, dim3(ch.g1 - ch.g0), dim3(256), (size_t)ch.lds, stream, dt_n.as<T>(), dt_d.as<double>(),
                         dt_grp.as<CsGroup>(), dt_order.as<int>() + ch.g0, dt_woff.as<long long>(), dt_x.as<T>(), dt_cv.as<double>(), ok, d->ridge,
                         dcnt, kCsLdsDoubles);
      if (ch.r1 > ch.r0)
        hipLaunchKernelGGL(dtransfer_basis_kernel<T>, dim3((unsigned)(ch.r1 - ch.r0) * P.npieces), dim3(256), 0, stream, tiles.as<T>(),
                           bl_tile.as<long long>(), dt_grp.as<CsGroup>(), dt_woff.as<long long>(), ok, dt_runs.as<DtRun>() + ch.r0, dt_x.as<T>(), nfreqs,
                           fpad, xpitch, fold ? 1 : 0, P.npieces);
      if (ch.q1 > ch.q0)
        hipLaunchKernelGGL(dtransfer_power_kernel<T>, dim3((unsigned)(ch.q1 - ch.q0) * (ndpad / kDsCols)), dim3(256), 0, stream, dt_x.as<T>(),
                           dt_op.as<T>(), wgts.as<T>(), g, bl_ant.as<int2>(), dt_grp.as<CsGroup>(), ok, dt_rows.as<DtRow>() + ch.q0, nfreqs, fpad, xpitch,
                           nd, ndpad, d->calibrated, want_abs ? dt_abs.as<double>() : nullptr, noise_bl ? dt_noise.as<double>() : nullptr, o_valid);
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(cnt, dcnt, 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
    if (nbins) {
      hipLaunchKernelGGL(dspec_bin_kernel, dim3(nbins, (nd + 255) / 256, 1), dim3(256), 0, stream, dt_abs.as<double>(), o_valid, dt_ptr.as<int>(),
                         dt_ent.as<int>(), 0, nbls, nd, nbins, 1, o_abin, o_cbin);
      HIP_TRY(hipGetLastError());
      // the bins of every rank's rows add up to the array's: ONE all-reduce of nbins ndelays + nbins doubles
      if (comm_on()) CAL_TRY(all_reduce(o_abin, (size_t)nbins * nd + nbins, CAL_XCHG_F64, CAL_XCHG_SUM));
    }
    CAL_TRY(give(absorbed_bl, dt_abs.as<double>(), P.n_rows_out));
    CAL_TRY(give(noise_bl, dt_noise.as<double>(), P.n_rows_out));
    CAL_TRY(give(absorbed_bin, o_abin, (size_t)nbins * nd));
    CAL_TRY(give(count_bin, o_cbin, (size_t)nbins));
    HIP_TRY(hipStreamSynchronize(stream));
    if (counts) {
      counts->nsolved = cnt[0];
      counts->nsingular = cnt[1];
    }
    return CAL_OK;
  }
  int set_delay_transfer_scratch(int64_t bytes) override {
    if (bytes < 0) return fail(CAL_ERR_INVALID, "set_delay_transfer_scratch: negative bound");
    dt_bound = bytes == 0 ? kCsScratchDefault : bytes;
    for (DevBuf* b : {&dt_n, &dt_d, &dt_x}) b->release();
    return CAL_OK;
  }

  // cal_solver_fix_degeneracies: the model pass of model(), then the six kernels of degeneracy_kernels.hpp.  The rows of every slice and their
  // segments, d_b and the longest |d_b| are planned on the host from the plan's bl_ant and the caller's positions; nothing is read back to plan.
  // m stays in the model planes (model_buf) for the whole call -- no other pass runs in between -- and m' overwrites it there at the end.
  int fix_degeneracies(const cal_degeneracy_desc* d, double* params, double* nsamp, double* last_step, void* out_g_r, void* out_g_i, void* out_m_r,
                       void* out_m_i) override {
    HIP_TRY(hipSetDevice(device));
    if (!d) return fail(CAL_ERR_INVALID, "fix_degeneracies: null description");
    CAL_TRY(require_set("fix_degeneracies", false));
    const T2* g = nullptr;
    CAL_TRY(report_gains("fix_degeneracies", d->g_r, d->g_i, &g));
    if (comm_on() && nranks > 1)
      return fail(CAL_ERR_STATE, "fix_degeneracies: a communicator or exchange hook of %d ranks is set: the channel sums over the baselines would need an "
                  "all-reduce per iteration, which is not implemented", nranks);
    if (d->mode != CAL_DEGEN_CHANNEL && d->mode != CAL_DEGEN_BAND) return fail(CAL_ERR_INVALID, "fix_degeneracies: mode = %d (CAL_DEGEN_CHANNEL or CAL_DEGEN_BAND)", d->mode);
    if (d->iters < 1) return fail(CAL_ERR_INVALID, "fix_degeneracies: iters = %d (at least 1)", d->iters);
    if (!d->ref_r || !d->ref_i) return fail(CAL_ERR_INVALID, "fix_degeneracies: null reference planes");
    if (!d->antpos) return fail(CAL_ERR_INVALID, "fix_degeneracies: null antenna positions");
    if ((d->gref_r == nullptr) != (d->gref_i == nullptr)) return fail(CAL_ERR_INVALID, "fix_degeneracies: give both gref_r and gref_i, or neither");
    if ((out_g_r == nullptr) != (out_g_i == nullptr) || (out_m_r == nullptr) != (out_m_i == nullptr))
      return fail(CAL_ERR_INVALID, "fix_degeneracies: the outputs come in (re, im) pairs");
    const bool band = d->mode == CAL_DEGEN_BAND;
    if (band && !d->freqs) return fail(CAL_ERR_INVALID, "fix_degeneracies: CAL_DEGEN_BAND needs freqs");
    const int nsl = tb_on() ? tb_T : nslices, na = nants / nsl;  // joint time-basis layout: antenna row t na + a is slice t, antenna a
    DegeneracyPlan P;  // d_b, the slices' rows and their segments (report_plan.hpp)
    CAL_TRY(plan_degeneracies(h_bl_ant, nants, nsl, nfreqs, fpad, band, d->antpos, d->freqs, P));
    const int nseg = P.nseg;
    CAL_TRY(put(dg_geo, P.pack_geo(), true));
    CAL_TRY(put(dg_idx, P.pack_idx(), true));
    const size_t plane = (size_t)nbls * fpad, splane = (size_t)nsl * fpad;
    const size_t st_count = kDgPlanes * splane + 2 * (size_t)nsl;
    CAL_TRY(dg_z.reserve(2 * plane * sizeof(T)));
    CAL_TRY(dg_part.reserve((size_t)kDgFirstSums * nseg * fpad * sizeof(double), false));
    CAL_TRY(dg_st.reserve(st_count * sizeof(double), false));
    T* z_r = dg_z.as<T>();
    T* z_i = z_r + plane;
    CAL_TRY(upload_rows(d->ref_r, z_r, nbls, 1, 0));
    CAL_TRY(upload_rows(d->ref_i, z_i, nbls, 1, 0));
    const T* w = wgts.as<T>();
    if (d->ref_w) {
      CAL_TRY(dg_w.reserve(plane * sizeof(T)));
      CAL_TRY(upload_rows(d->ref_w, dg_w.as<T>(), nbls, 1, 0));
      w = dg_w.as<T>();
    }
    const size_t gbytes = (size_t)nants * fpad * sizeof(T2);
    if (d->gref_r) {
      CAL_TRY(dg_gref.reserve(gbytes));
      CAL_TRY(upload_rows(d->gref_r, dg_gref.as<T>(), nants, 2, 0));
      CAL_TRY(upload_rows(d->gref_i, dg_gref.as<T>(), nants, 2, 1));
    }
    if (out_g_r) CAL_TRY(dg_gout.reserve(gbytes));
    const double* geo = dg_geo.as<double>();
    const double2* dv = reinterpret_cast<const double2*>(geo);
    const double2* pos = reinterpret_cast<const double2*>(geo + P.geo_pos());
    const double* ratio = geo + P.geo_ratio();
    const double* maxd = geo + P.geo_maxd();
    const int* ent = dg_idx.as<int>();
    const int* segptr = ent + P.idx_segptr();
    const DgSeg* segs = reinterpret_cast<const DgSeg*>(ent + P.idx_segs());
    double* st = dg_st.as<double>();
    double* part = dg_part.as<double>();
    T *m_r = nullptr, *m_i = nullptr;
    hipError_t memset_err = hipSuccess;
    CAL_TRY(model_pass(2, [&](T* model_r, T* model_i, T*) {
      m_r = model_r, m_i = model_i;
      memset_err = hipMemsetAsync(st, 0, st_count * sizeof(double), stream);
      if (memset_err != hipSuccess) return;
      launch_rows(degen_rows_kernel<T>, 0, model_r, model_i, z_r, z_i, w, bl_ant.as<int2>(), nbls, nfreqs, fpad);
      const dim3 sum_grid(nseg, (nfreqs + 255) / 256), solve_grid((nfreqs + 63) / 64, nsl);
      for (int it = 0; it <= d->iters; ++it) {  // iters steps, then the amplitude at the last Phi
        const int first = it == 0, last = it == d->iters;
        if (first)
          hipLaunchKernelGGL((degen_sum_kernel<T, true>), sum_grid, dim3(256), 0, stream, z_r, z_i, model_r, model_i, w, ent, segs, dv, st, nsl, nfreqs, fpad,
                             nseg, part);
        else
          hipLaunchKernelGGL((degen_sum_kernel<T, false>), sum_grid, dim3(256), 0, stream, z_r, z_i, model_r, model_i, w, ent, segs, dv, st, nsl, nfreqs, fpad,
                             nseg, part);
        hipLaunchKernelGGL(degen_solve_kernel, solve_grid, dim3(64, kDgParts), 0, stream, part, segptr, ratio, maxd, band ? 1 : 0, 0, first, last, nsl, nfreqs, fpad, nseg, st);
        if (band)
          hipLaunchKernelGGL(degen_solve_kernel, dim3(nsl), dim3(256), 0, stream, part, segptr, ratio, maxd, 1, 1, first, last, nsl, nfreqs, fpad, nseg, st);
      }
      if (d->gref_r)
        hipLaunchKernelGGL(degen_phase_kernel<T>, solve_grid, dim3(64), 0, stream, g, dg_gref.as<T2>(), w, ant_ptr.as<int>(), ant_ent.as<int2>(), pos, nsl, na,
                           nfreqs, fpad, st);
      if (out_g_r)
        hipLaunchKernelGGL(degen_apply_gains_kernel<T>, dim3(grid_for((long long)nants * fpad)), dim3(256), 0, stream, g, pos, st, nsl, na, nants, nfreqs, fpad,
                           dg_gout.as<T2>());
      if (out_m_r) launch_rows(degen_apply_rows_kernel<T>, 0, model_r, model_i, bl_ant.as<int2>(), dv, st, nsl, na, nbls, nfreqs, fpad);
    }));
    HIP_TRY(memset_err);
    std::vector<double> h_st(kDgPlanes * splane);
    HIP_TRY(copy_sync(h_st.data(), st, h_st.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int t = 0; t < nsl; ++t)
      for (int f = 0; f < nfreqs; ++f) {
        const size_t sf = (size_t)t * fpad + f, o = (size_t)t * nfreqs + f;
        if (params) {
          params[4 * o + 0] = h_st[DG_ETA * splane + sf];
          params[4 * o + 1] = h_st[DG_PSI * splane + sf];
          params[4 * o + 2] = h_st[DG_PE * splane + sf];
          params[4 * o + 3] = h_st[DG_PN * splane + sf];
        }
        if (nsamp) nsamp[o] = h_st[DG_CNT * splane + sf];
        if (last_step) last_step[o] = h_st[DG_STEP * splane + sf];
      }
    if (out_g_r) {
      CAL_TRY(download_rows(out_g_r, dg_gout.as<T>(), nants, 2, 0));
      CAL_TRY(download_rows(out_g_i, dg_gout.as<T>(), nants, 2, 1));
    }
    if (out_m_r) {
      CAL_TRY(download_rows(out_m_r, m_r, nbls, 1, 0));
      CAL_TRY(download_rows(out_m_i, m_i, nbls, 1, 0));
    }
    return CAL_OK;
  }

  // cal_solver_robust_weights: the model pass of model(), then robust_rows_kernel (robust_weight_kernels.hpp) over the weight plane in place.
  // Nothing leaves a baseline row: no exchange under a communicator.
  int robust_weights(const cal_robust_desc* d, double* scale_bl, double* ndown_bl) override {
    HIP_TRY(hipSetDevice(device));
    if (!d) return fail(CAL_ERR_INVALID, "robust_weights: null description");
    CAL_TRY(require_set("robust_weights", true));
    if (d->kind != CAL_ROBUST_NONE && d->kind != CAL_ROBUST_HUBER && d->kind != CAL_ROBUST_CAUCHY && d->kind != CAL_ROBUST_CLIP)
      return fail(CAL_ERR_INVALID, "robust_weights: unknown kind %d", d->kind);
    if (!(d->threshold > 0.0) || !std::isfinite(d->threshold)) return fail(CAL_ERR_INVALID, "robust_weights: threshold = %g must be finite and > 0", d->threshold);
    CAL_TRY(rw_out.reserve(2 * (size_t)nbls * sizeof(double)));
    double* o_scale = rw_out.as<double>();
    double* o_ndown = o_scale + nbls;
    HIP_TRY(hipMemsetAsync(o_scale, 0, 2 * (size_t)nbls * sizeof(double), stream));  // rows of unselected slices report 0
    if (d->kind != CAL_ROBUST_NONE || rw_w0_valid) {  // (kind NONE before any reweighting: the weights are w0 already)
      if (!rw_w0_valid) {
        CAL_TRY(rw_w0.reserve(wgts.bytes, false));
        HIP_TRY(hipMemcpyAsync(rw_w0.p, wgts.p, wgts.bytes, hipMemcpyDeviceToDevice, stream));
        rw_w0_valid = true;
      }
      const unsigned char* mask = nullptr;
      CAL_TRY(upload_slice_mask(d->slice_mask, &mask));
      static_assert(kRobustRows == 4, "robust_rows_kernel walks the rows like the other row kernels");
      const bool lds = fpad <= robust_lds_fpad<T>();
      auto launch = [&](T* model_r, T* model_i) {
        launch_rows(lds ? robust_rows_kernel<T, true> : robust_rows_kernel<T, false>, lds ? (size_t)kRobustRows * fpad * sizeof(T) : 0, model_r,
                    model_i, data_r.as<T>(), data_i.as<T>(), rw_w0.as<T>(), wgts.as<T>(), gains.as<T2>(), bl_ant.as<int2>(), mask, na_slice, nbls,
                    nfreqs, fpad, d->kind, d->threshold, o_scale, o_ndown);
      };
      if (d->kind == CAL_ROBUST_NONE) {
        launch(nullptr, nullptr);
        HIP_TRY(hipGetLastError());
      } else {
        CAL_TRY(model_pass(2, [&](T* model_r, T* model_i, T*) { launch(model_r, model_i); }));
      }
    }
    CAL_TRY(give(scale_bl, o_scale, (size_t)nbls));
    CAL_TRY(give(ndown_bl, o_ndown, (size_t)nbls));
    HIP_TRY(hipStreamSynchronize(stream));
    return CAL_OK;
  }
  int get_weights(void* out, int which) override {
    HIP_TRY(hipSetDevice(device));
    if (!has_problem || !has_data) return fail(CAL_ERR_STATE, "get_weights: problem and data must be set");
    if (!out) return fail(CAL_ERR_INVALID, "get_weights: null output");
    if (which != 0 && which != 1) return fail(CAL_ERR_INVALID, "get_weights: which = %d (0: current, 1: w0)", which);
    return download_rows(out, which == 1 && rw_w0_valid ? rw_w0.as<T>() : wgts.as<T>(), nbls, 1, 0);
  }

  // cal_solver_hold_slices: slices that enter every later run as stopped (a chunked loop keeps the slices that met the tolerance in
  // an earlier chunk as they are); NULL or all zeros: none.  set_optimizer and set_problem clear it.
  int hold_slices(const uint8_t* mask) override {
    if (!has_problem) return fail(CAL_ERR_STATE, "hold_slices before set_problem");
    held.clear();
    if (mask && std::any_of(mask, mask + nslices, [](uint8_t m) { return m != 0; })) {
      held.resize(nslices);
      for (int t = 0; t < nslices; ++t) held[t] = mask[t] ? 1 : 0;
    }
    return CAL_OK;
  }

  // ---- the steps the closed-form solves are made of --------------------------------------------------------------------
  // what every solve call checks first, behind its description (ridge: null where the call has none)
  int check_solve_call(const char* who, const char* count_name, int count, const char* unit, double damping, const double* ridge) {
    CAL_TRY(require_set(who, true));
    if (count < 1) return fail(CAL_ERR_INVALID, "%s: %s = %d, at least one %s", who, count_name, count, unit);
    if (!(damping > 0.0 && damping <= 1.0)) return fail(CAL_ERR_INVALID, "%s: damping = %g lies outside (0, 1]", who, damping);
    if (ridge && (!(*ridge >= 0.0) || !std::isfinite(*ridge))) return fail(CAL_ERR_INVALID, "%s: ridge = %g must be finite and >= 0", who, *ridge);
    return CAL_OK;
  }
  int check_moment_reset(const char* who, int reset, const char* flag) {
    if (reset && !has_opt) return fail(CAL_ERR_STATE, "%s: %s without an optimizer (cal_solver_set_optimizer)", who, flag);
    return CAL_OK;
  }
  // what the antenna sweeps work on: the per-antenna lists without the autocorrelation rows (problem_plan.hpp; uploaded at the first
  // call of a problem) and their output planes
  int gain_sweep_setup() {
    if (!gs_ptr.p) {
      std::vector<int> ptr;
      std::vector<int2> ent;
      antenna_lists(nants, h_bl_ant, true, ptr, ent);
      CAL_TRY(upload(gs_ent, ent));
      CAL_TRY(upload(gs_ptr, ptr));
    }
    return gs_out.reserve(3 * (size_t)nants * nfreqs * sizeof(double));
  }
  template <typename Kern>
  int allow_chol_lds(Kern* kern) {  // a factor kernel may ask for kCsLdsDoubles of dynamic LDS
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kCsLdsDoubles * (int)sizeof(double)));
    return CAL_OK;
  }
  // the model pass of model(), then gain_solve_rows_kernel: the planes the antenna sweeps read.  before(P) sees the model planes
  // (P.u_r, P.u_i) before the rows kernel overwrites them.
  template <typename Before = void (*)(const RowPlanes&)>
  int gain_planes(RowPlanes& P, Before before = [](const RowPlanes&) {}) {
    return model_pass(3, [&](T* model_r, T* model_i, T* third) {
      P = RowPlanes{model_r, model_i, third};
      before(P);
      launch_rows(gain_solve_rows_kernel<T>, 0, P.u_r, P.u_i, P.q, data_r.as<T>(), data_i.as<T>(), wgts.as<T>(), bl_ant.as<int2>(), nbls, nfreqs, fpad);
    });
  }
  // the model pass of model(), then coeff_solve_rows_kernel: the planes the Gram kernel reads
  // (g: the gains of a report call that was given its own, report_gains; null: the solver's)
  int coeff_planes(RowPlanes& P, const T2* g = nullptr) {
    return model_pass(3, [&](T* model_r, T* model_i, T* third) {
      P = RowPlanes{model_r, model_i, third};
      launch_rows(coeff_solve_rows_kernel<T>, 0, P.u_r, P.u_i, P.q, data_r.as<T>(), data_i.as<T>(), wgts.as<T>(), g ? g : gains.as<T2>(), bl_ant.as<int2>(),
                  nbls, nfreqs, fpad);
    });
  }
  // One antenna sweep: gain_solve_ant_kernel into gs_out (num_r | num_i | den), then the exchange of its last `nplanes` planes.  The
  // planes of every rank's baselines add up to the array's: ONE all-reduce of nplanes nants nfreqs doubles per sweep.
  int antenna_sweep(const RowPlanes& P, int nplanes) {
    const size_t nant_out = (size_t)nants * nfreqs;
    launch_ants(gain_solve_ant_kernel<T>, P.u_r, P.u_i, P.q, gains.as<T2>(), gs_ptr.as<int>(), gs_ent.as<int2>(), nants, nfreqs, fpad,
                gs_out.as<double>());
    HIP_TRY(hipGetLastError());
    if (comm_on()) CAL_TRY(all_reduce(gs_out.as<double>() + (3 - nplanes) * nant_out, nplanes * nant_out, CAL_XCHG_F64, CAL_XCHG_SUM));
    return CAL_OK;
  }
  // The end of a solve call: its two counters (cnt: null where it has none), what set_optimizer leaves in the moment slots the call
  // has solved -- reset_moments() -- then the stream drained and the result filled in.
  template <typename Res, typename Reset>
  int finish_solve(const DevBuf* cnt, Res* res, int reset, Reset reset_moments) {
    int counts[2] = {0, 0};
    if (cnt) HIP_TRY(hipMemcpyAsync(counts, cnt->p, 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
    if (reset) {
      CAL_TRY(reset_moments());
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(stream));
    if (res) {
      res->nsolved = counts[0];
      res->nsingular = counts[1];
    }
    return CAL_OK;
  }

  // cal_solver_solve_gains: the model pass of model(), gain_solve_rows_kernel once, then per sweep gain_solve_ant_kernel, the exchange of
  // its three planes and gain_solve_apply_kernel (gain_solve_kernels.hpp).
  int solve_gains(const cal_gain_solve_desc* d) override {
    HIP_TRY(hipSetDevice(device));
    if (!d) return fail(CAL_ERR_INVALID, "solve_gains: null description");
    CAL_TRY(check_solve_call("solve_gains", "nsweeps", d->nsweeps, "sweep", d->damping, nullptr));
    if (yb_on())
      return fail(CAL_ERR_UNSUPPORTED, "solve_gains: a gain basis is set (cal_solver_set_gain_basis, cal_solver_set_gain_time_basis): the closed form solves "
                  "free per-channel gains, and projecting them onto a basis is not implemented here; cal_solver_solve_gain_coeffs solves the coefficients of a "
                  "frequency basis, or detach the basis (nvec = 0) first");
    CAL_TRY(check_moment_reset("solve_gains", d->reset_gain_moments, "reset_gain_moments"));
    CAL_TRY(gain_sweep_setup());
    const unsigned char* mask = nullptr;
    CAL_TRY(upload_slice_mask(d->slice_mask, &mask));
    RowPlanes P;
    CAL_TRY(gain_planes(P));
    for (int k = 0; k < d->nsweeps; ++k) {
      CAL_TRY(antenna_sweep(P, 3));
      hipLaunchKernelGGL(gain_solve_apply_kernel<T>, dim3(grid_for((long long)nants * nfreqs)), dim3(256), 0, stream, gains.as<T2>(), gs_out.as<double>(),
                         mask, na_slice, nants, nfreqs, fpad, d->damping);
      HIP_TRY(hipGetLastError());
    }
    const size_t per = (size_t)na_slice * fpad * 2;  // reals of the gain slots per slice
    return finish_solve(nullptr, (cal_coeff_solve_result*)nullptr, d->reset_gain_moments,
                        [&] { return reset_slice_moments(d->slice_mask, gains_m, gains_v, per, false); });
  }

  // ---- cal_solver_normal_product / cal_solver_gauss_newton_step (gauss_newton_kernels.hpp) -----------------------
  // N p = J^H W J p through the solver's own passes: the model pass on substituted coefficients gives A dc, the gradient pass on substituted
  // data planes gives J^H W y.  Both are substituted by copying in place and back (the idiom of robust_weights), so every kernel family
  // reads the substituted operands through the pointers it always reads and no recorded step graph goes stale.
  size_t gn_go() const { return 2 * (size_t)nants * fpad; }
  size_t gn_np() const { return gn_go() + 2 * (size_t)ncoef; }
  GnSpace gn_space() const {
    GnSpace S{};
    S.coff = slice_coff.as<int>();
    S.na_slice = na_slice;
    S.nfreqs = nfreqs;
    S.fpad = fpad;
    S.ncoef = ncoef;
    S.go = (long long)gn_go();
    return S;
  }
  int gn_check(const char* who) {
    CAL_TRY(require_set(who, true));
    if (yb_on())
      return fail(CAL_ERR_UNSUPPORTED, "%s: a gain basis is set (cal_solver_set_gain_basis, cal_solver_set_gain_time_basis): the optimizer's gain variables are "
                  "then the basis coefficients y, and the Gauss-Newton matrix projected on them is not implemented; detach the basis (nvec = 0) first", who);
    if (comm_on())
      return fail(CAL_ERR_UNSUPPORTED, "%s: a communicator or exchange hook is set: the per-slice scalars of the product and of conjugate gradients would "
                  "need an exchange over the ranks, which is not implemented", who);
    return CAL_OK;
  }
  int gn_alloc(bool cg) {
    const size_t np = gn_np(), plane = (size_t)nbls * fpad;
    CAL_TRY(gn_s.reserve(np * sizeof(T)));
    CAL_TRY(gn_g0.reserve(np * sizeof(T)));
    CAL_TRY(gn_save.reserve(np * sizeof(T)));
    CAL_TRY(gn_ns.reserve(np * sizeof(double)));
    CAL_TRY(gn_m.reserve(2 * plane * sizeof(T)));
    CAL_TRY(gn_sd.reserve(2 * plane * sizeof(T)));
    CAL_TRY(gn_rows.reserve(3 * (size_t)nbls * sizeof(double)));
    CAL_TRY(gn_part.reserve((size_t)nslices * kGnBlocks * sizeof(double)));
    CAL_TRY(gn_scal.reserve((size_t)nslices * sizeof(GnScal)));
    if (!gn_rowptr.p) {
      // the groups are listed slice by slice and a group's rows are contiguous: so are a slice's rows
      std::vector<int> ptr(nslices + 1, nbls);
      for (int k = ngrps - 1; k >= 0; --k) ptr[h_cs_grp[k].slice] = std::min(ptr[h_cs_grp[k].slice], h_cs_grp[k].b0);
      for (int t = nslices - 1; t >= 0; --t) ptr[t] = std::min(ptr[t], ptr[t + 1]);
      CAL_TRY(upload(gn_rowptr, ptr));
    }
    if (!cg) return CAL_OK;
    CAL_TRY(gn_x.reserve(np * sizeof(double)));
    CAL_TRY(gn_res.reserve(np * sizeof(double)));
    CAL_TRY(gn_D.reserve(np * sizeof(double)));
    CAL_TRY(gn_lam.reserve((size_t)nslices * sizeof(double)));
    if (!gn_grp.p) {
      std::vector<GnGroup> g(ngrps);
      for (int k = 0; k < ngrps; ++k) g[k] = GnGroup{h_cs_grp[k].b0, h_cs_grp[k].b1, h_cs_grp[k].coff, h_cs_grp[k].nvec};
      CAL_TRY(upload(gn_grp, g));
    }
    return CAL_OK;
  }
  int gn_restore_data(PassGuard& G) {
    if (!G.data) return CAL_OK;
    const size_t plane = (size_t)nbls * fpad;
    HIP_TRY(hipMemcpyAsync(data_r.p, gn_sd.p, plane * sizeof(T), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(data_i.p, gn_sd.as<T>() + plane, plane * sizeof(T), hipMemcpyDeviceToDevice, stream));
    G.data = false;
    return CAL_OK;
  }
  int gn_restore_coefs(PassGuard& G) {
    if (!G.coefs) return CAL_OK;
    HIP_TRY(hipMemcpyAsync(coef.p, gn_save.as<T>() + gn_go(), 2 * (size_t)ncoef * sizeof(T), hipMemcpyDeviceToDevice, stream));
    G.coefs = false;
    return CAL_OK;
  }
  // data, coefficients and loop state back as the call found them -- on every path out of a call, failures included
  int pass_end(PassGuard& G, int rc, const char* who) {
    const std::string msg = g_err;
    int rc2 = gn_restore_data(G);
    if (rc2 == CAL_OK) rc2 = gn_restore_coefs(G);
    std::copy(G.saved.begin(), G.saved.end(), h_state);
    if (rc2 == CAL_OK) rc2 = push_state();
    if (rc2 == CAL_OK && hipStreamSynchronize(stream) != hipSuccess) rc2 = fail(CAL_ERR_HIP, "%s: hipStreamSynchronize failed", who);
    if (timing && rc2 == CAL_OK) rc2 = collect_timing();
    if (rc != CAL_OK) {
      g_err = msg;
      return rc;
    }
    return rc2;
  }
  // the gradient pass on the data planes as they stand; dst (may be null): the flat copy of the four planes
  int gn_grad_pass(T* dst) {
    CAL_TRY(enqueue_pass(step_shape(kGradPass), 0));
    if (dst) {
      HIP_TRY(hipMemcpyAsync(dst, comm.p, gn_go() * sizeof(T), hipMemcpyDeviceToDevice, stream));
      HIP_TRY(hipMemcpyAsync(dst + gn_go(), grad_c0(), 2 * (size_t)ncoef * sizeof(T), hipMemcpyDeviceToDevice, stream));
    }
    return CAL_OK;
  }
  // m = A c into gn_m (with_precond: D into gn_D from the same model pass), then the data planes saved and replaced by G m and the gradient
  // of that into gn_g0
  int gn_linearize(PassGuard& G, bool with_precond) {
    const size_t plane = (size_t)nbls * fpad;
    hipError_t ce = hipSuccess;
    const auto keep_model = [&](const RowPlanes& M) {  // (the imaginary plane follows the real one)
      ce = hipMemcpyAsync(gn_m.p, M.u_r, 2 * plane * sizeof(T), hipMemcpyDeviceToDevice, stream);
    };
    if (with_precond) {
      CAL_TRY(gain_sweep_setup());
      RowPlanes P;
      CAL_TRY(gain_planes(P, keep_model));
      HIP_TRY(ce);
      CAL_TRY(antenna_sweep(P, 3));  // (gn_check has refused a communicator: no exchange)
      hipLaunchKernelGGL(gn_precond_gain_kernel, dim3(grid_for((long long)nants * fpad)), dim3(256), 0, stream,
                         gs_out.as<double>() + 2 * (size_t)nants * nfreqs, gn_D.as<double>(), nants, nfreqs, fpad);
      double* rowq = gn_rows.as<double>() + 2 * (size_t)nbls;
      launch_rows(gn_precond_rows_kernel<T>, 0, gains.as<T2>(), wgts.as<T>(), bl_ant.as<int2>(), nbls, nfreqs, fpad, rowq);
      hipLaunchKernelGGL(gn_precond_coeff_kernel, dim3((ngrps + 255) / 256), dim3(256), 0, stream, rowq, gn_grp.as<GnGroup>(), ngrps, ncoef,
                         gn_D.as<double>() + gn_go());
      HIP_TRY(hipGetLastError());
    } else {
      CAL_TRY(model_pass(2, [&](T* model_r, T* model_i, T*) { keep_model(RowPlanes{model_r, model_i, nullptr}); }));
      HIP_TRY(ce);
    }
    HIP_TRY(hipMemcpyAsync(gn_sd.p, data_r.p, plane * sizeof(T), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(gn_sd.as<T>() + plane, data_i.p, plane * sizeof(T), hipMemcpyDeviceToDevice, stream));
    G.data = true;
    launch_gn_data(nullptr, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    return gn_grad_pass(gn_g0.as<T>());
  }
  // gn_ns = N s (+ lambda D s with D) for the direction in gn_s, and the partials of s . gn_ns; the coefficients are put back before it returns,
  // the data planes stay substituted
  int gn_product(PassGuard& G, const double* D) {
    const size_t plane = (size_t)nbls * fpad, cb = 2 * (size_t)ncoef * sizeof(T);
    HIP_TRY(hipMemcpyAsync(gn_save.as<T>() + gn_go(), coef.p, cb, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(coef.p, gn_s.as<T>() + gn_go(), cb, hipMemcpyDeviceToDevice, stream));
    G.coefs = true;
    CAL_TRY(model_pass(2, [&](T* model_r, T* model_i, T*) {
      launch_rows(gn_tangent_rows_kernel<T>, 0, gn_m.as<T>(), gn_m.as<T>() + plane, model_r, model_i, gains.as<T2>(), gn_s.as<T2>(), wgts.as<T>(),
                  bl_ant.as<int2>(), nbls, nfreqs, fpad, gn_rows.as<double>());
    }));
    CAL_TRY(gn_restore_coefs(G));
    hipLaunchKernelGGL(gn_scale_kernel, dim3(nslices), dim3(256), 0, stream, gn_rows.as<double>(), gn_rowptr.as<int>(), gn_scal.as<GnScal>());
    launch_gn_data(model_buf.as<T>(), model_buf.as<T>() + plane, gn_scal.as<GnScal>());
    HIP_TRY(hipGetLastError());
    CAL_TRY(gn_grad_pass(nullptr));
    hipLaunchKernelGGL(gn_diff_kernel<T>, dim3(kGnBlocks, nslices), dim3(256), 0, stream, gn_space(), comm.as<T>(), grad_c0(), gn_g0.as<T>(), gn_s.as<T>(), D,
                       gn_scal.as<GnScal>(), gn_ns.as<double>(), gn_part.as<double>());
    HIP_TRY(hipGetLastError());
    return CAL_OK;
  }

  int normal_product(const void* p_g_r, const void* p_g_i, const void* p_c_r, const void* p_c_i, void* out_g_r, void* out_g_i, void* out_c_r,
                     void* out_c_i) override {
    HIP_TRY(hipSetDevice(device));
    if (!p_g_r || !p_g_i || !p_c_r || !p_c_i || !out_g_r || !out_g_i || !out_c_r || !out_c_i) return fail(CAL_ERR_INVALID, "normal_product: null pointer");
    CAL_TRY(gn_check("normal_product"));
    CAL_TRY(gn_alloc(false));
    const size_t cb = (size_t)ncoef * sizeof(T);
    CAL_TRY(upload_rows(p_g_r, gn_s.as<T>(), nants, 2, 0));
    CAL_TRY(upload_rows(p_g_i, gn_s.as<T>(), nants, 2, 1));
    HIP_TRY(copy_sync(gn_s.as<T>() + gn_go(), p_c_r, cb, hipMemcpyHostToDevice));
    HIP_TRY(copy_sync(gn_s.as<T>() + gn_go() + ncoef, p_c_i, cb, hipMemcpyHostToDevice));
    std::vector<GnScal> sc(nslices);
    for (auto& x : sc) {
      x = GnScal{};
      x.scale = 1.0;
    }
    HIP_TRY(copy_sync(gn_scal.p, sc.data(), sc.size() * sizeof(GnScal), hipMemcpyHostToDevice));
    PassGuard G;
    int rc = pass_begin(G);
    if (rc == CAL_OK) rc = gn_linearize(G, false);
    if (rc == CAL_OK) rc = gn_product(G, nullptr);
    if (rc == CAL_OK) {
      T* out = gn_g0.as<T>();  // (the gradient of G m has served)
      hipLaunchKernelGGL(gn_round_kernel<T>, dim3(grid_for((long long)gn_np())), dim3(256), 0, stream, gn_ns.as<double>(), out, (long long)gn_np());
      if (hipGetLastError() != hipSuccess) rc = fail(CAL_ERR_HIP, "normal_product: launch failed");
    }
    CAL_TRY(pass_end(G, rc, "normal_product"));
    const T* out = gn_g0.as<T>();
    CAL_TRY(download_rows(out_g_r, out, nants, 2, 0));
    CAL_TRY(download_rows(out_g_i, out, nants, 2, 1));
    HIP_TRY(copy_sync(out_c_r, out + gn_go(), cb, hipMemcpyDeviceToHost));
    HIP_TRY(copy_sync(out_c_i, out + gn_go() + ncoef, cb, hipMemcpyDeviceToHost));
    return CAL_OK;
  }

  int gauss_newton_step(const cal_gauss_newton_desc* d, cal_gauss_newton_result* res) override {
    HIP_TRY(hipSetDevice(device));
    if (!d || !res) return fail(CAL_ERR_INVALID, "gauss_newton_step: null description or results");
    if (d->ncg < 1) return fail(CAL_ERR_INVALID, "gauss_newton_step: ncg = %d, at least one iteration", d->ncg);
    if (!(d->cg_tol >= 0.0) || !std::isfinite(d->cg_tol)) return fail(CAL_ERR_INVALID, "gauss_newton_step: cg_tol = %g must be finite and >= 0", d->cg_tol);
    if (!d->lambda) return fail(CAL_ERR_INVALID, "gauss_newton_step: null lambda");
    CAL_TRY(gn_check("gauss_newton_step"));
    for (int t = 0; t < nslices; ++t)
      if (!(d->lambda[t] >= 0.0) || !std::isfinite(d->lambda[t]))
        return fail(CAL_ERR_INVALID, "gauss_newton_step: lambda[%d] = %g must be finite and >= 0", t, d->lambda[t]);
    if (d->reset_moments && !has_opt) return fail(CAL_ERR_STATE, "gauss_newton_step: reset_moments without an optimizer (cal_solver_set_optimizer)");
    CAL_TRY(gn_alloc(true));
    const unsigned char* mask = nullptr;
    CAL_TRY(upload_slice_mask(d->slice_mask, &mask));
    HIP_TRY(copy_sync(gn_lam.p, d->lambda, (size_t)nslices * sizeof(double), hipMemcpyHostToDevice));
    std::vector<double> before(nslices), after(nslices);
    std::vector<GnScal> sc(nslices);
    std::vector<uint8_t> accepted(nslices, 0);
    const GnSpace S = gn_space();
    const dim3 vgrid(kGnBlocks, nslices), sgrid((nslices + 63) / 64);
    GnScal* scal_d = gn_scal.as<GnScal>();
    double *x = gn_x.as<double>(), *r = gn_res.as<double>(), *ns = gn_ns.as<double>(), *D = gn_D.as<double>(), *part = gn_part.as<double>();
    T* s = gn_s.as<T>();
    PassGuard G;
    auto body = [&]() -> int {
      // the gradient at the data (its loss is the loss before the step), the linearisation, the right-hand side
      CAL_TRY(gn_grad_pass(s));
      CAL_TRY(pull_state());
      for (int t = 0; t < nslices; ++t) before[t] = h_state[t].loss;
      CAL_TRY(gn_linearize(G, true));
      hipLaunchKernelGGL(gn_rhs_kernel<T>, vgrid, dim3(256), 0, stream, S, s, s + gn_go(), gn_g0.as<T>(), r);
      hipLaunchKernelGGL(gn_init_kernel<T>, vgrid, dim3(256), 0, stream, S, r, D, x, s, part);
      hipLaunchKernelGGL(gn_scalar0_kernel, sgrid, dim3(64), 0, stream, scal_d, part, kGnBlocks, nslices, mask, gn_lam.as<double>(), d->cg_tol);
      HIP_TRY(hipGetLastError());
      for (int it = 0; it < d->ncg; ++it) {  // the host reads no scalar in here: a frozen slice's kernels return at once
        CAL_TRY(gn_product(G, D));
        hipLaunchKernelGGL(gn_scalar1_kernel, sgrid, dim3(64), 0, stream, scal_d, part, kGnBlocks, nslices);
        hipLaunchKernelGGL(gn_update1_kernel<T>, vgrid, dim3(256), 0, stream, S, scal_d, s, ns, D, x, r, part);
        hipLaunchKernelGGL(gn_scalar2_kernel, sgrid, dim3(64), 0, stream, scal_d, part, kGnBlocks, nslices);
        hipLaunchKernelGGL(gn_update2_kernel<T>, vgrid, dim3(256), 0, stream, S, scal_d, r, D, s);
        HIP_TRY(hipGetLastError());
      }
      CAL_TRY(gn_restore_data(G));
      // the trial parameters of the selected slices, their loss, and the rejected slices back bit for bit
      HIP_TRY(hipMemcpyAsync(gn_save.p, gains.p, gn_go() * sizeof(T), hipMemcpyDeviceToDevice, stream));
      HIP_TRY(hipMemcpyAsync(gn_save.as<T>() + gn_go(), coef.p, 2 * (size_t)ncoef * sizeof(T), hipMemcpyDeviceToDevice, stream));
      hipLaunchKernelGGL(gn_apply_kernel<T>, vgrid, dim3(256), 0, stream, S, mask, x, gains.as<T>(), coef.as<T>());
      HIP_TRY(hipGetLastError());
      CAL_TRY(enqueue_pass(step_shape(kLossPass), 0));
      HIP_TRY(hipMemcpyAsync(sc.data(), scal_d, sc.size() * sizeof(GnScal), hipMemcpyDeviceToHost, stream));
      CAL_TRY(pull_state());
      std::vector<uint8_t> rejected(nslices, 0);
      for (int t = 0; t < nslices; ++t) {
        after[t] = h_state[t].loss;
        const bool sel = !d->slice_mask || d->slice_mask[t];
        accepted[t] = sel && std::isfinite(after[t]) && after[t] < before[t] ? 1 : 0;
        rejected[t] = sel && !accepted[t] ? 1 : 0;
      }
      const size_t ng = 2 * (size_t)na_slice * fpad;  // gain reals per slice
      CAL_TRY(for_selected_slice_runs(rejected.data(), [&](int t, int t1) {
        HIP_TRY(hipMemcpyAsync(gains.as<T>() + (size_t)t * ng, gn_save.as<T>() + (size_t)t * ng, (size_t)(t1 - t) * ng * sizeof(T), hipMemcpyDeviceToDevice, stream));
        const size_t n = (size_t)(h_slice_coff[t1] - h_slice_coff[t]);
        for (int plane = 0; plane < 2 && n > 0; ++plane) {
          const size_t off = (size_t)plane * ncoef + h_slice_coff[t];
          HIP_TRY(hipMemcpyAsync(coef.as<T>() + off, gn_save.as<T>() + gn_go() + off, n * sizeof(T), hipMemcpyDeviceToDevice, stream));
        }
        return (int)CAL_OK;
      }));
      // what set_optimizer leaves in the gain and coefficient slots, for the accepted slices
      if (d->reset_moments) CAL_TRY(reset_slice_moments(accepted.data(), gains_m, gains_v, ng, true));
      return CAL_OK;
    };
    int rc = pass_begin(G);
    if (rc == CAL_OK) rc = body();
    CAL_TRY(pass_end(G, rc, "gauss_newton_step"));
    for (int t = 0; t < nslices; ++t) {
      const bool sel = !d->slice_mask || d->slice_mask[t];
      res[t].loss_before = before[t];
      res[t].loss_after = sel ? after[t] : before[t];
      res[t].cg_residual = sc[t].resid;
      res[t].cg_iters = sc[t].iters;
      res[t].accepted = accepted[t];
    }
    return CAL_OK;
  }

  // ---- cal_solver_lbfgs (lbfgs_kernels.hpp) ------------------------------------------------------------------------
  // L-BFGS over the optimizer's own variables (gain_set(): the gains or y; the coefficient planes): the gradient and the loss come from the
  // passes every layout and kernel path already has, so a gain basis, a time gain basis and a frozen model all work.  The slices' scalars
  // stay on the device; the host reads one integer per trial round of the line search (how many slices still search) and nothing else
  // inside the loop.
  int lbfgs(const cal_lbfgs_desc* d, double* losses_out, cal_lbfgs_result* res) override {
    HIP_TRY(hipSetDevice(device));
    if (!d || !res) return fail(CAL_ERR_INVALID, "lbfgs: null description or results");
    if (d->nsteps < 1) return fail(CAL_ERR_INVALID, "lbfgs: nsteps = %d, at least one iteration", d->nsteps);
    if (d->history < 1 || d->history > kLbfgsMaxHistory) return fail(CAL_ERR_INVALID, "lbfgs: history = %d is outside [1, %d]", d->history, kLbfgsMaxHistory);
    if (d->max_ls < 1) return fail(CAL_ERR_INVALID, "lbfgs: max_ls = %d, at least one trial", d->max_ls);
    if (!(d->c1 > 0.0 && d->c1 < 1.0)) return fail(CAL_ERR_INVALID, "lbfgs: c1 = %g is outside (0, 1)", d->c1);
    if (!(d->shrink > 0.0 && d->shrink < 1.0)) return fail(CAL_ERR_INVALID, "lbfgs: shrink = %g is outside (0, 1)", d->shrink);
    if (!(d->ftol >= 0.0) || !std::isfinite(d->ftol)) return fail(CAL_ERR_INVALID, "lbfgs: ftol = %g must be finite and >= 0", d->ftol);
    if (!(d->curvature_eps >= 0.0) || !std::isfinite(d->curvature_eps))
      return fail(CAL_ERR_INVALID, "lbfgs: curvature_eps = %g must be finite and >= 0", d->curvature_eps);
    CAL_TRY(require_set("lbfgs", true));
    if (comm_on())
      return fail(CAL_ERR_UNSUPPORTED, "lbfgs: a communicator or exchange hook is set: the dot products of the history and the line search's scalars would "
                  "need an exchange over the ranks, which is not implemented");
    if (d->reset_moments && !has_opt) return fail(CAL_ERR_STATE, "lbfgs: reset_moments without an optimizer (cal_solver_set_optimizer)");
    const bool frozen = d->freeze_model != 0;
    const AdamSet<T> ga = gain_set();
    const long long go = ga.n, np = go + 2LL * ncoef;
    LbSpace S{};
    S.coff = slice_coff.as<int>();
    S.ngs = go / nslices;
    S.go = go;
    S.ncoef = ncoef;
    S.w = yb_on() ? y_w() : fpad;
    S.cols = yb_on() ? y_cols() : nfreqs;
    S.freeze = frozen ? 1 : 0;
    S.nslot = d->history + 1;
    const LbParams P{d->nsteps, d->history, d->max_ls, d->c1, d->shrink, d->ftol, d->curvature_eps};
    const size_t nloss = (size_t)nslices * (d->nsteps + 1);
    CAL_TRY(lb_vec.reserve((size_t)(2 * S.nslot + 2) * np * sizeof(T)));
    CAL_TRY(lb_part.reserve((size_t)nslices * kLbDots * kLbBlocks * sizeof(double)));
    CAL_TRY(lb_dots.reserve((size_t)nslices * kLbDots * sizeof(double)));
    CAL_TRY(lb_state.reserve((size_t)nslices * sizeof(LbState)));
    CAL_TRY(lb_losses.reserve(nloss * sizeof(double)));
    CAL_TRY(lb_count.reserve(sizeof(int)));
    std::vector<LbState> hs(nslices);
    for (int t = 0; t < nslices; ++t) {
      std::memset(&hs[t], 0, sizeof(LbState));
      if (d->slice_mask && !d->slice_mask[t]) {
        hs[t].done = 1;
        hs[t].status = 4;
      }
    }
    std::vector<double> hl(nloss, std::numeric_limits<double>::quiet_NaN());
    HIP_TRY(copy_sync(lb_state.p, hs.data(), hs.size() * sizeof(LbState), hipMemcpyHostToDevice));
    HIP_TRY(copy_sync(lb_losses.p, hl.data(), nloss * sizeof(double), hipMemcpyHostToDevice));
    constexpr int V = 16 / (int)sizeof(T);
    const LbView<T> x{ga.p, coef.as<T>()};
    const LbView<T> g{const_cast<T*>(ga.g), grad_c0()};
    T* vec = lb_vec.as<T>();
    LbState* st = lb_state.as<LbState>();
    double *part = lb_part.as<double>(), *dots = lb_dots.as<double>(), *losses_d = lb_losses.as<double>();
    const dim3 vgrid(kLbBlocks, nslices), rgrid(nslices, (kLbDots + 3) / 4);
    const StepShape grad_shape = step_shape(yb_on() ? kProjectedGradPass : kGradPass), loss_shape = step_shape(kLossPass);
    // the gradient pass at the point the solver holds, then the pair (or the start), the sums, the iteration's end and the next direction
    auto advance = [&](int init) -> int {
      CAL_TRY(enqueue_pass(grad_shape, 0));
      hipLaunchKernelGGL(lbfgs_pair_kernel<T>, vgrid, dim3(256), 0, stream, S, x, g, vec, np, st, part, init);
      hipLaunchKernelGGL(lbfgs_reduce_kernel<V>, rgrid, dim3(256), 0, stream, S, st, part, dots, init);
      hipLaunchKernelGGL(lbfgs_coeff_kernel, dim3(nslices), dim3(64), 0, stream, st, dots, st_cur(), losses_d, P, init);
      HIP_TRY(hipGetLastError());
      return CAL_OK;
    };
    PassGuard G;
    auto body = [&]() -> int {
      CAL_TRY(advance(1));
      for (int k = 0; k < d->nsteps; ++k) {
        hipLaunchKernelGGL(lbfgs_direction_kernel<T>, vgrid, dim3(256), 0, stream, S, vec, np, st);
        int n = 1;
        // a search takes at most max_ls trials, twice where it starts over along the gradient
        for (int r = 0; r < 2 * d->max_ls && n > 0; ++r) {
          hipLaunchKernelGGL(lbfgs_trial_kernel<T>, vgrid, dim3(256), 0, stream, S, x, vec, np, st);
          HIP_TRY(hipGetLastError());
          if (yb_on()) CAL_TRY(enqueue_expand(gb_y.as<T2>(), gains.as<T2>()));
          CAL_TRY(enqueue_pass(loss_shape, 0));
          hipLaunchKernelGGL(lbfgs_armijo_kernel, dim3(1), dim3(256), 0, stream, st, st_cur(), nslices, P, lb_count.as<int>());
          HIP_TRY(hipGetLastError());
          HIP_TRY(hipMemcpyAsync(&n, lb_count.p, sizeof(int), hipMemcpyDeviceToHost, stream));  // the one readback of the loop
          HIP_TRY(hipStreamSynchronize(stream));
        }
        if (n > 0) return fail(CAL_ERR_HIP, "lbfgs: the line search did not end within %d rounds", 2 * d->max_ls);
        hipLaunchKernelGGL(lbfgs_restore_kernel<T>, vgrid, dim3(256), 0, stream, S, x, vec, np, st);
        HIP_TRY(hipGetLastError());
        if (yb_on()) CAL_TRY(enqueue_expand(gb_y.as<T2>(), gains.as<T2>()));
        if (n < 0) break;  // every slice is done
        CAL_TRY(advance(0));
      }
      HIP_TRY(hipMemcpyAsync(hs.data(), st, hs.size() * sizeof(LbState), hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipMemcpyAsync(hl.data(), losses_d, nloss * sizeof(double), hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
      if (d->reset_moments) {
        // what set_optimizer leaves in the slots of the variables that moved
        std::vector<uint8_t> moved(nslices);
        for (int t = 0; t < nslices; ++t) moved[t] = hs[t].ever_moved ? 1 : 0;
        CAL_TRY(reset_slice_moments(moved.data(), yb_on() ? gb_ym : gains_m, yb_on() ? gb_yv : gains_v, (size_t)S.ngs, !frozen));
      }
      return CAL_OK;
    };
    int rc = pass_begin(G);
    if (rc == CAL_OK) rc = body();
    CAL_TRY(pass_end(G, rc, "lbfgs"));
    for (int t = 0; t < nslices; ++t) {
      const double f0 = hs[t].status == 4 ? std::numeric_limits<double>::quiet_NaN() : hl[(size_t)t * (d->nsteps + 1)];
      res[t].loss_before = hs[t].status == 3 ? std::numeric_limits<double>::quiet_NaN() : f0;
      res[t].loss_after = hs[t].status >= 3 ? res[t].loss_before : hs[t].f;
      res[t].iters = hs[t].iters;
      res[t].evals = hs[t].evals;
      res[t].pairs_dropped = hs[t].dropped;
      res[t].status = hs[t].status;
    }
    if (losses_out) std::copy(hl.begin(), hl.end(), losses_out);
    return CAL_OK;
  }

  // ---- cal_solver_solve_coeffs ----------------------------------------------------------------------------------
  void release_coeff_solve() {  // the plan of a problem / a scratch bound: rebuilt by the next call
    cs_chunks.clear();
    for (DevBuf* b : {&cs_grp, &cs_order, &cs_work, &cs_n, &cs_d, &cs_cnt, &fe_grp, &fe_order, &fe_work, &fe_woff, &fe_lwork, &fe_n, &fe_d, &fe_w, &fe_rhs, &fe_ok, &fe_part, &fe_out, &fe_mv}) b->release();
    fe_chunks.clear();
  }
  int set_coeff_solve_scratch(int64_t bytes) override {
    if (bytes < 0) return fail(CAL_ERR_INVALID, "set_coeff_solve_scratch: negative bound");
    cs_bound = bytes == 0 ? kCsScratchDefault : bytes;
    release_coeff_solve();
    release_gain_systems();
    return CAL_OK;
  }
  // The plan of solve_plan.hpp for this problem and bound, uploaded at the first call.  Every chunk reuses the two scratch buffers from
  // offset 0; a group's result does not depend on the chunk it falls into.
  int build_coeff_solve_plan() {
    if (!cs_chunks.empty()) return CAL_OK;
    const GroupPlan P = plan_group_chunks(h_cs_grp, sizeof(T), cs_bound, {});  // (its offsets land in h_cs_grp; nothing else reads them)
    CAL_TRY(upload(cs_grp, h_cs_grp));
    CAL_TRY(upload(cs_order, P.order));
    CAL_TRY(upload(cs_work, P.work));
    CAL_TRY(cs_n.alloc((size_t)P.n_max * sizeof(T), false));
    CAL_TRY(cs_d.alloc((size_t)P.d_max * sizeof(double), false));
    CAL_TRY(cs_cnt.alloc(2 * sizeof(int)));
    CAL_TRY(allow_chol_lds(&coeff_chol_kernel<T>));
    cs_chunks = P.chunks;
    return CAL_OK;
  }

  // cal_solver_solve_coeffs: per iteration the model pass of model(), coeff_solve_rows_kernel, then per chunk of groups
  // coeff_gram_kernel and coeff_chol_kernel (coeff_solve_kernels.hpp).  Every group is owned by one rank: no exchange.
  int solve_coeffs(const cal_coeff_solve_desc* d, cal_coeff_solve_result* res) override {
    HIP_TRY(hipSetDevice(device));
    if (!d) return fail(CAL_ERR_INVALID, "solve_coeffs: null description");
    CAL_TRY(check_solve_call("solve_coeffs", "niters", d->niters, "iteration", d->damping, &d->ridge));
    CAL_TRY(check_moment_reset("solve_coeffs", d->reset_coeff_moments, "reset_coeff_moments"));
    CAL_TRY(build_coeff_solve_plan());
    CAL_TRY(cs_rhs.reserve(2 * (size_t)ncoef * sizeof(T)));
    const unsigned char* mask = nullptr;
    CAL_TRY(upload_slice_mask(d->slice_mask, &mask));
    for (int it = 0; it < d->niters; ++it) {
      RowPlanes P;
      CAL_TRY(coeff_planes(P));
      HIP_TRY(hipMemsetAsync(cs_cnt.p, 0, 2 * sizeof(int), stream));
      for (const GroupChunk& ch : cs_chunks) {
        hipLaunchKernelGGL(coeff_gram_kernel<T>, dim3(ch.w1 - ch.w0), dim3(256), 0, stream, tiles.as<T>(), bl_tile.as<long long>(), P.u_r,
                           P.u_i, P.q, cs_grp.as<CsGroup>(), cs_work.as<CsWork>() + ch.w0, cs_n.as<T>(), cs_rhs.as<T>(), ncoef, nfreqs, fpad,
                           fold ? 1 : 0);
        hipLaunchKernelGGL(coeff_chol_kernel<T>, dim3(ch.g1 - ch.g0), dim3(256), ch.lds, stream, cs_n.as<T>(), cs_rhs.as<T>(), cs_d.as<double>(),
                           cs_grp.as<CsGroup>(), cs_order.as<int>() + ch.g0, coef.as<T>(), coef.as<T>() + ncoef, ncoef, mask, d->damping, d->ridge,
                           cs_cnt.as<int>(), kCsLdsDoubles);
        HIP_TRY(hipGetLastError());
      }
    }
    return finish_solve(&cs_cnt, res, d->reset_coeff_moments, [&] { return reset_slice_moments(d->slice_mask, coef_m, coef_v, 0, true); });
  }

  // ---- cal_solver_fit_errors -------------------------------------------------------------------------------------
  // solve_coeffs' plan with W counted in a chunk's bytes, and per chunk the leverage kernel's work (solve_plan.hpp).
  int build_fit_error_plan() {
    if (!fe_chunks.empty()) return CAL_OK;
    std::vector<CsGroup> grp = h_cs_grp;  // (solve_coeffs' offsets stay where they are)
    GroupPlan P = plan_group_chunks(grp, sizeof(T), cs_bound, fit_error_extra(grp));
    plan_leverage_work(P, grp, h_bl_tile, fold ? nfreqs / 2 : fpad);
    CAL_TRY(upload(fe_grp, grp));
    CAL_TRY(upload(fe_order, P.order));
    CAL_TRY(upload(fe_work, P.work));
    CAL_TRY(upload(fe_woff, P.xoff));
    CAL_TRY(upload(fe_lwork, P.lwork));
    CAL_TRY(fe_n.alloc((size_t)P.n_max * sizeof(T), false));
    CAL_TRY(fe_d.alloc((size_t)P.d_max * sizeof(double), false));
    CAL_TRY(fe_w.alloc((size_t)P.x_max * sizeof(T), false));
    CAL_TRY(fe_rhs.alloc(2 * (size_t)ncoef * sizeof(T)));
    CAL_TRY(fe_ok.alloc(((size_t)ngrps + 2) * sizeof(int)));
    CAL_TRY(fe_part.alloc((size_t)nbls * (fold ? 2 : 1) * P.npieces * sizeof(double)));
    CAL_TRY(fe_out.alloc(((size_t)ncoef + 2 * (size_t)nbls) * sizeof(double)));
    CAL_TRY(allow_chol_lds(&fit_error_factor_kernel<T>));
    fe_npieces = P.npieces;
    fe_chunks = P.chunks;
    return CAL_OK;
  }

  // cal_solver_fit_errors: the model pass of model() and coeff_solve_rows_kernel for q, then per chunk of groups coeff_gram_kernel (as
  // it is; its rhs is not used), fit_error_factor_kernel and fit_error_leverage_kernel, then fit_error_rows_kernel; for gain_var the
  // model pass once more with gain_solve_rows_kernel, gain_solve_ant_kernel and the exchange of its den plane.
  int fit_errors(double ridge, double* coeff_var, double* model_var, double* leverage_bl, double* nsamp_bl, double* gain_var,
                 cal_fit_errors_counts* counts) override {
    HIP_TRY(hipSetDevice(device));
    CAL_TRY(require_set("fit_errors", true));
    if (!(ridge >= 0.0) || !std::isfinite(ridge)) return fail(CAL_ERR_INVALID, "fit_errors: ridge = %g must be finite and >= 0", ridge);
    if (gain_var && yb_on())
      return fail(CAL_ERR_UNSUPPORTED, "fit_errors: gain_var with a gain basis set (cal_solver_set_gain_basis, cal_solver_set_gain_time_basis): the variance of "
                  "a basis gain is b_f^T N_a^-1 b_f with the projected N_a, which is not implemented here; pass gain_var = NULL (the coefficient "
                  "outputs use the expanded gains), or detach the basis (nvec = 0) first");
    const bool want_lev = model_var || leverage_bl;
    const bool want_coef = coeff_var || want_lev;
    int cnt[2] = {0, 0};
    if (want_coef || nsamp_bl) {
      CAL_TRY(build_fit_error_plan());
      const int nslot = (fold ? 2 : 1) * fe_npieces;
      double* o_cv = fe_out.as<double>();
      double* o_lev = o_cv + ncoef;
      double* o_ns = o_lev + nbls;
      int* ok = fe_ok.as<int>();
      int* dcnt = ok + ngrps;
      const size_t mv_bytes = (size_t)nbls * nfreqs * sizeof(double);
      if (model_var) CAL_TRY(fe_mv.reserve(mv_bytes, false));
      if (want_coef) {
        RowPlanes P;
        CAL_TRY(coeff_planes(P));
        // a singular group keeps zeros
        HIP_TRY(hipMemsetAsync(fe_ok.p, 0, ((size_t)ngrps + 2) * sizeof(int), stream));
        HIP_TRY(hipMemsetAsync(o_cv, 0, ((size_t)ncoef + (size_t)nbls) * sizeof(double), stream));
        if (want_lev) HIP_TRY(hipMemsetAsync(fe_part.p, 0, (size_t)nbls * nslot * sizeof(double), stream));
        if (model_var) HIP_TRY(hipMemsetAsync(fe_mv.p, 0, mv_bytes, stream));
        for (const GroupChunk& ch : fe_chunks) {
          hipLaunchKernelGGL(coeff_gram_kernel<T>, dim3(ch.w1 - ch.w0), dim3(256), 0, stream, tiles.as<T>(), bl_tile.as<long long>(), P.u_r,
                             P.u_i, P.q, fe_grp.as<CsGroup>(), fe_work.as<CsWork>() + ch.w0, fe_n.as<T>(), fe_rhs.as<T>(), ncoef, nfreqs, fpad,
                             fold ? 1 : 0);
          hipLaunchKernelGGL(fit_error_factor_kernel<T>, dim3(ch.g1 - ch.g0), dim3(256), ch.lds, stream, fe_n.as<T>(), fe_d.as<double>(),
                             fe_grp.as<CsGroup>(), fe_order.as<int>() + ch.g0, fe_woff.as<long long>(), fe_w.as<T>(), o_cv, ok, ridge, dcnt,
                             kCsLdsDoubles);
          if (want_lev && ch.l1 > ch.l0)
            hipLaunchKernelGGL(fit_error_leverage_kernel<T>, dim3(ch.l1 - ch.l0), dim3(256), 0, stream, tiles.as<T>(), bl_tile.as<long long>(),
                               P.q, fe_grp.as<CsGroup>(), fe_woff.as<long long>(), ok, fe_lwork.as<FeWork>() + ch.l0, fe_w.as<T>(),
                               model_var ? fe_mv.as<double>() : nullptr, fe_part.as<double>(), nfreqs, fpad, fold ? 1 : 0, fe_npieces);
          HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(cnt, dcnt, 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
      }
      if (leverage_bl || nsamp_bl) {
        launch_rows(fit_error_rows_kernel<T>, 0, fe_part.as<double>(), wgts.as<T>(), nbls, nfreqs, fpad, nslot, leverage_bl ? o_lev : nullptr,
                    nsamp_bl ? o_ns : nullptr);
        HIP_TRY(hipGetLastError());
      }
      if (coeff_var) HIP_TRY(hipMemcpyAsync(coeff_var, o_cv, (size_t)ncoef * sizeof(double), hipMemcpyDeviceToHost, stream));
      if (model_var) HIP_TRY(hipMemcpyAsync(model_var, fe_mv.p, mv_bytes, hipMemcpyDeviceToHost, stream));
      if (leverage_bl) HIP_TRY(hipMemcpyAsync(leverage_bl, o_lev, (size_t)nbls * sizeof(double), hipMemcpyDeviceToHost, stream));
      if (nsamp_bl) HIP_TRY(hipMemcpyAsync(nsamp_bl, o_ns, (size_t)nbls * sizeof(double), hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
    }
    if (gain_var) {
      CAL_TRY(gain_sweep_setup());
      RowPlanes P;
      CAL_TRY(gain_planes(P));
      CAL_TRY(antenna_sweep(P, 1));  // of the three planes only den is wanted, and exchanged
      const size_t nant_out = (size_t)nants * nfreqs;
      HIP_TRY(copy_sync(gain_var, gs_out.as<double>() + 2 * nant_out, nant_out * sizeof(double), hipMemcpyDeviceToHost));
      for (size_t k = 0; k < nant_out; ++k) gain_var[k] = gain_var[k] > 0.0 ? 1.0 / gain_var[k] : 0.0;
    }
    if (counts) {
      counts->nsolved = cnt[0];
      counts->nsingular = cnt[1];
    }
    return CAL_OK;
  }

  // ---- the projected gain systems: solve_gain_coeffs, solve_gain_time_coeffs, gain_basis_errors ------------------
  // The pg_ set for the chunks of rc; the buffers only grow.  No call can read what another left behind: gain_basis_gram_kernel and
  // gain_time_kron_kernel write every element of every row that a factor or Kronecker kernel of the same chunk then reads (N_a and M_{t,a}
  // on and below the diagonal, which is all the readers touch; both rhs rows), rows of a masked slice are skipped by the Gram and the
  // factor kernel alike, the factor in pg_d is written (normal_chol_load, ChanSystem::zero) before it is read, and a sweep zeroes the
  // counters itself.  pg_rhs and pg_cnt are zero-filled when allocated, as they always were.
  int reserve_gain_systems(const RowChunks& rc) {
    if (rc.m_row) {
      CAL_TRY(pg_m.reserve((size_t)rc.rows * rc.m_row * sizeof(T), false));
      CAL_TRY(pg_rhsa.reserve(2 * (size_t)rc.rows * rc.n * sizeof(T), false));
    }
    if (rc.n_row) {
      CAL_TRY(pg_n.reserve((size_t)rc.rows * rc.n_row * sizeof(T), false));
      CAL_TRY(pg_rhs.reserve(2 * (size_t)nants * gb_nvec * sizeof(T)));
      CAL_TRY(allow_chol_lds(&gain_basis_chol_kernel<T>));
    }
    CAL_TRY(pg_d.reserve(std::max<size_t>(8, (size_t)rc.rows * rc.d_row * sizeof(double)), false));
    return pg_cnt.reserve(2 * sizeof(int));
  }
  // Enqueues the projected normal matrices of rows [a0, a0 + ca) (antenna rows; antennas under a time basis) and their right-hand
  // sides: without a time basis gain_basis_gram_kernel into pg_n; with both bases the Gram of the rows of every time into pg_m
  // ([t][rel][K][K]: one launch over all rows when the chunk holds every antenna, their rows then lie side by side; else one per
  // time), then gain_time_kron_kernel into pg_n and pg_rhsa.  mask: the slice mask of solve_gain_coeffs, null otherwise.
  void enqueue_gain_systems(int a0, int ca, const unsigned char* mask) {
    const int K = gb_nvec, nb = (K + kNsBlock - 1) / kNsBlock, npairs = nb * (nb + 1) / 2;
    auto gram = [&](int row0, int rows, T* nmat) {
      hipLaunchKernelGGL(gain_basis_gram_kernel<T>, dim3((unsigned)rows * npairs), dim3(256), 0, stream, gb_Bt.as<T>(), gs_out.as<double>(), gains.as<T2>(),
                         nmat, pg_rhs.as<T>(), mask, na_slice, row0, npairs, K, gb_kpad, nants, nfreqs, fpad);
    };
    if (!tb_on()) return gram(a0, ca, pg_n.as<T>());
    const int na = tb_na, Tn = tb_T, L = tb_L;
    if (ca == na) gram(0, nants, pg_m.as<T>());
    else
      for (int t = 0; t < Tn; ++t) gram(t * na + a0, ca, pg_m.as<T>() + (size_t)t * ca * K * K);
    hipLaunchKernelGGL(gain_time_kron_kernel<T>, dim3((unsigned)ca * L, (L + kTimeTile - 1) / kTimeTile), dim3(256), 0, stream, pg_m.as<T>(),
                       pg_rhs.as<T>(), tb_B.as<T>(), pg_n.as<T>(), pg_rhsa.as<T>(), a0, ca, na, Tn, L, tb_lpad, K);
  }

  // cal_solver_gain_basis_errors: fit_errors' sequence for gain_var (the model pass, gain_solve_rows_kernel, gain_solve_ant_kernel and
  // the exchange of its den plane), then per chunk of rows enqueue_gain_systems (the kernels of the sweeps as they are),
  // gain_error_factor_kernel and gain_error_var_kernel; a time basis alone runs
  // gain_time_chan_var_kernel and gain_error_dof_kernel instead (gain_error_kernels.hpp).  The chunks count W (solve_plan.hpp).  y is
  // replicated and den is summed over the ranks, so every rank computes the same planes: no collective beyond antenna_sweep's own.
  int gain_basis_errors(double ridge, double* gain_var, double* y_var, double* gain_dof, cal_fit_errors_counts* counts) override {
    HIP_TRY(hipSetDevice(device));
    CAL_TRY(require_set("gain_basis_errors", true));
    if (!(ridge >= 0.0) || !std::isfinite(ridge)) return fail(CAL_ERR_INVALID, "gain_basis_errors: ridge = %g must be finite and >= 0", ridge);
    if (!yb_on())
      return fail(CAL_ERR_STATE, "gain_basis_errors: no gain basis is set (cal_solver_set_gain_basis, cal_solver_set_gain_time_basis); cal_solver_fit_errors "
                  "gives gain_var = 1 / den of free per-channel gains");
    CAL_TRY(gain_sweep_setup());
    const int K = gb_nvec, L = tb_on() ? tb_L : 0, Tn = tb_on() ? tb_T : 1, na = y_rows(), Lr = tb_on() ? tb_L : 1;
    const int n = Lr * (gb_on() ? K : 1), np = fe_pad(n);
    const RowChunks rc = plan_row_chunks(K, L, Tn, nfreqs, sizeof(T), cs_bound, na, gain_error_extra(K, L));
    const size_t nant_out = (size_t)nants * nfreqs;
    const size_t n_yvar = (size_t)na * Lr * (gb_on() ? K : nfreqs);
    const size_t n_chan = gb_on() ? 0 : (size_t)na * nfreqs;  // the channels' dof of a time basis alone
    CAL_TRY(reserve_gain_systems(rc));
    if (gb_on()) {
      CAL_TRY(gbe_w.reserve((size_t)rc.rows * rc.x_row * sizeof(T), false));
      CAL_TRY(allow_chol_lds(&gain_error_factor_kernel<T>));
    }
    CAL_TRY(gbe_ok.reserve(((size_t)na + 2) * sizeof(int)));
    CAL_TRY(gbe_out.reserve((nant_out + n_yvar + (size_t)na + n_chan) * sizeof(double), false));
    double* o_gv = gbe_out.as<double>();
    double* o_yv = o_gv + nant_out;
    double* o_dof = o_yv + n_yvar;
    double* o_chan = o_dof + na;
    int* ok = gbe_ok.as<int>();
    int* dcnt = ok + na;
    RowPlanes P;
    CAL_TRY(gain_planes(P));
    CAL_TRY(antenna_sweep(P, 1));  // of the three planes only den is wanted, and exchanged
    // a singular system keeps zeros
    HIP_TRY(hipMemsetAsync(gbe_ok.p, 0, ((size_t)na + 2) * sizeof(int), stream));
    HIP_TRY(hipMemsetAsync(gbe_out.p, 0, (nant_out + n_yvar + (size_t)na + n_chan) * sizeof(double), stream));
    const int npieces = (nfreqs + kFePiece - 1) / kFePiece;
    for (int a0 = 0; a0 < na; a0 += rc.rows) {
      const int ca = std::min(rc.rows, na - a0);
      if (gb_on()) {
        enqueue_gain_systems(a0, ca, nullptr);  // (the right-hand sides it also forms go nowhere anyone reads)
        hipLaunchKernelGGL(gain_error_factor_kernel<T>, dim3(ca), dim3(256), rc.lds, stream, pg_n.as<T>(), pg_d.as<double>(), gbe_w.as<T>(),
                           y_var ? o_yv : nullptr, gain_dof ? o_dof : nullptr, ok, a0, n, ridge, dcnt, kCsLdsDoubles);
        if (gain_var)
          hipLaunchKernelGGL(gain_error_var_kernel<T>, dim3((unsigned)Tn * ca * npieces), dim3(256), 0, stream, gbe_w.as<T>(), gb_Bt.as<T>(),
                             tb_on() ? tb_B.as<T>() : (const T*)nullptr, ok, o_gv, a0, ca, na, Lr, tb_lpad, K, nfreqs, fpad, npieces);
      } else {
        const unsigned blocks = (unsigned)(((long long)ca * nfreqs + 255) / 256);
        auto* chan = L <= kTimeTile ? gain_time_chan_var_kernel<T, kTimeTile> : gain_time_chan_var_kernel<T, 0>;  // the channel systems in registers, or in pg_d
        hipLaunchKernelGGL(chan, dim3(blocks), dim3(256), 0, stream, gs_out.as<double>(), tb_B.as<T>(), pg_d.as<double>(), y_var ? o_yv : nullptr,
                           gain_var ? o_gv : nullptr, gain_dof ? o_chan : nullptr, a0, ca, na, Tn, L, tb_lpad, nfreqs, ridge, dcnt);
      }
      HIP_TRY(hipGetLastError());
    }
    if (!gb_on() && gain_dof) {
      hipLaunchKernelGGL(gain_error_dof_kernel, dim3((na + 255) / 256), dim3(256), 0, stream, o_chan, o_dof, na, nfreqs);
      HIP_TRY(hipGetLastError());
    }
    int cnt[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(cnt, dcnt, 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
    if (gain_var) HIP_TRY(hipMemcpyAsync(gain_var, o_gv, nant_out * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (y_var) HIP_TRY(hipMemcpyAsync(y_var, o_yv, n_yvar * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (gain_dof) HIP_TRY(hipMemcpyAsync(gain_dof, o_dof, (size_t)na * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (counts) {
      counts->nsolved = cnt[0];
      counts->nsingular = cnt[1];
    }
    return CAL_OK;
  }

  // cal_solver_solve_gain_coeffs: solve_gains' sequence up to the exchanged planes, then per chunk of antenna rows enqueue_gain_systems
  // (gain_basis_gram_kernel) and gain_basis_chol_kernel (gain_basis_solve_kernels.hpp), then the gains of the selected slices rebuilt from y.  Every chunk of a
  // sweep reads the old gains: they are rebuilt behind the last one.  y is replicated and the planes are summed over the ranks, so
  // every rank computes the same update: no collective beyond solve_gains' own.
  int solve_gain_coeffs(const cal_gain_coeff_solve_desc* d, cal_gain_coeff_solve_result* res) override {
    HIP_TRY(hipSetDevice(device));
    if (!d) return fail(CAL_ERR_INVALID, "solve_gain_coeffs: null description");
    CAL_TRY(check_solve_call("solve_gain_coeffs", "nsweeps", d->nsweeps, "sweep", d->damping, &d->ridge));
    if (tb_on())
      return fail(CAL_ERR_UNSUPPORTED, "solve_gain_coeffs: a gain time basis is set (cal_solver_set_gain_time_basis): its coefficients couple the times of an "
                  "antenna, a joint (l, k) system this call does not solve; detach the time basis (nvec_t = 0) first");
    if (!gb_on()) return fail(CAL_ERR_STATE, "solve_gain_coeffs: no frequency gain basis is set (cal_solver_set_gain_basis); cal_solver_solve_gains solves free per-channel gains");
    CAL_TRY(check_moment_reset("solve_gain_coeffs", d->reset_gain_moments, "reset_gain_moments"));
    CAL_TRY(gain_sweep_setup());
    // chunks of antenna rows whose N_a (T) and factor (double, only where it does not fit LDS) stay under cs_bound (solve_plan.hpp)
    const int K = gb_nvec;
    const RowChunks rc = plan_row_chunks(K, 0, 0, nfreqs, sizeof(T), cs_bound, nants);
    CAL_TRY(reserve_gain_systems(rc));
    const unsigned char* mask = nullptr;
    CAL_TRY(upload_slice_mask(d->slice_mask, &mask));
    RowPlanes P;
    CAL_TRY(gain_planes(P));
    for (int k = 0; k < d->nsweeps; ++k) {
      CAL_TRY(antenna_sweep(P, 3));
      HIP_TRY(hipMemsetAsync(pg_cnt.p, 0, 2 * sizeof(int), stream));
      for (int a0 = 0; a0 < nants; a0 += rc.rows) {
        const int nr = std::min(rc.rows, nants - a0);
        enqueue_gain_systems(a0, nr, mask);
        hipLaunchKernelGGL(gain_basis_chol_kernel<T>, dim3(nr), dim3(256), rc.lds, stream, pg_n.as<T>(), pg_rhs.as<T>(), pg_d.as<double>(),
                           gb_y.as<T2>(), mask, na_slice, a0, a0, 1, K, gb_kpad, d->damping, d->ridge, pg_cnt.as<int>(), kCsLdsDoubles);
        HIP_TRY(hipGetLastError());
      }
      // gains = g0 + B y for the selected slices (runs of neighbouring slices in one launch each): the others keep their bits
      constexpr int per = 256 * (16 / (int)sizeof(T));  // channels per block of gain_expand_kernel
      CAL_TRY(for_selected_slice_runs(d->slice_mask, [&](int t, int t1) {
        const size_t r0 = (size_t)t * na_slice;
        hipLaunchKernelGGL((gain_expand_kernel<T>), dim3((fpad + per - 1) / per, (t1 - t) * na_slice), dim3(256), 0, stream, gb_g0.as<T2>() + r0 * fpad,
                           gb_Bt.as<T>(), gb_y.as<T2>() + r0 * gb_kpad, gains.as<T2>() + r0 * fpad, fpad, gb_kpad);
        return (int)CAL_OK;
      }));
      HIP_TRY(hipGetLastError());
    }
    const size_t yper = (size_t)na_slice * gb_kpad * 2;  // reals of the y slots per slice
    return finish_solve(&pg_cnt, res, d->reset_gain_moments, [&] { return reset_slice_moments(d->slice_mask, gb_ym, gb_yv, yper, false); });
  }

  // cal_solver_solve_gain_time_coeffs: solve_gain_coeffs' sequence up to the exchanged planes, then per chunk of antennas either
  // enqueue_gain_systems (gain_basis_gram_kernel on every row of the chunk: M_{t,a} and B^T r; gain_time_kron_kernel) and
  // gain_basis_chol_kernel over the L blocks of an antenna, or, without a
  // frequency basis, gain_time_chan_kernel (gain_time_solve_kernels.hpp); then the gains rebuilt from y.  Every chunk of a sweep reads
  // the old gains.  y is replicated and the planes are summed over the ranks: no collective beyond solve_gains' own.
  int solve_gain_time_coeffs(const cal_gain_time_solve_desc* d, cal_gain_time_solve_result* res) override {
    HIP_TRY(hipSetDevice(device));
    if (!d) return fail(CAL_ERR_INVALID, "solve_gain_time_coeffs: null description");
    CAL_TRY(check_solve_call("solve_gain_time_coeffs", "nsweeps", d->nsweeps, "sweep", d->damping, &d->ridge));
    if (!tb_on())
      return fail(CAL_ERR_STATE, "solve_gain_time_coeffs: no gain time basis is set (cal_solver_set_gain_time_basis); cal_solver_solve_gain_coeffs solves the "
                  "coefficients of a frequency basis alone, cal_solver_solve_gains free per-channel gains");
    CAL_TRY(check_moment_reset("solve_gain_time_coeffs", d->reset_gain_moments, "reset_gain_moments"));
    CAL_TRY(gain_sweep_setup());
    const int K = gb_nvec, L = tb_L, Tn = tb_T, na = tb_na;
    // chunks of antennas whose buffers stay under cs_bound (solve_plan.hpp)
    const RowChunks rc = plan_row_chunks(K, L, Tn, nfreqs, sizeof(T), cs_bound, na);
    CAL_TRY(reserve_gain_systems(rc));
    RowPlanes P;
    CAL_TRY(gain_planes(P));
    for (int k = 0; k < d->nsweeps; ++k) {
      CAL_TRY(antenna_sweep(P, 3));
      HIP_TRY(hipMemsetAsync(pg_cnt.p, 0, 2 * sizeof(int), stream));
      for (int a0 = 0; a0 < na; a0 += rc.rows) {
        const int ca = std::min(rc.rows, na - a0);
        if (gb_on()) {
          enqueue_gain_systems(a0, ca, nullptr);
          hipLaunchKernelGGL(gain_basis_chol_kernel<T>, dim3(ca), dim3(256), rc.lds, stream, pg_n.as<T>(), pg_rhsa.as<T>(), pg_d.as<double>(),
                             gb_y.as<T2>(), (const unsigned char*)nullptr, na_slice, a0, 0, L, K, gb_kpad, d->damping, d->ridge, pg_cnt.as<int>(),
                             kCsLdsDoubles);
        } else {
          const unsigned blocks = (unsigned)(((long long)ca * nfreqs + 255) / 256);
          auto* chan = L <= kTimeTile ? gain_time_chan_kernel<T, kTimeTile> : gain_time_chan_kernel<T, 0>;  // the channel systems in registers, or in pg_d
          hipLaunchKernelGGL(chan, dim3(blocks), dim3(256), 0, stream, gs_out.as<double>(), gains.as<T2>(), tb_B.as<T>(), gb_y.as<T2>(),
                             pg_d.as<double>(), a0, ca, na, Tn, L, tb_lpad, nfreqs, fpad, d->damping, d->ridge, pg_cnt.as<int>());
        }
        HIP_TRY(hipGetLastError());
      }
      CAL_TRY(enqueue_expand(gb_y.as<T2>(), gains.as<T2>()));  // gains = g0 + Bt (x) (B) y, behind the last chunk
    }
    // (the times of an antenna share its coefficients: no slice mask, every y slot)
    return finish_solve(&pg_cnt, res, d->reset_gain_moments, [&] { return reset_moment_slots(gb_ym, gb_yv, 0, 2 * (size_t)y_rows() * (size_t)y_row()); });
  }

  int init_coeffs(const void* sr, const void* si) override {
    HIP_TRY(hipSetDevice(device));
    if (!has_problem || !has_data) return fail(CAL_ERR_STATE, "init_coeffs: problem and data (weights) must be set");
    if (!sr || !si) return fail(CAL_ERR_INVALID, "init_coeffs: null source");
    const size_t rowbytes = (size_t)nbls * fpad * sizeof(T);
    CAL_TRY(model_buf.reserve(2 * rowbytes));
    T* s_r = model_buf.as<T>();
    T* s_i = s_r + (size_t)nbls * fpad;
    CAL_TRY(upload_rows(sr, s_r, nbls, 1, 0));
    CAL_TRY(upload_rows(si, s_i, nbls, 1, 0));
    begin_pass_state();
    CAL_TRY(push_state());
    FusedArgs<T> a = fused_args();
    a.data_r = s_r;
    a.data_i = s_i;
    launch_fused<MODE_INIT>(a, false);
    if (!gc_direct) launch_partial_reduce(gcp0, gc0, smap(false));
    HIP_TRY(hipGetLastError());
    // A^T b becomes the coefficient vector (orthonormal-column bases; the host applies the Gram solve otherwise)
    HIP_TRY(hipMemcpyAsync(coef.p, grad_c0(), 2 * (size_t)ncoef * sizeof(T), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    has_coef = true;
    return CAL_OK;
  }

  int synchronize() override {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamSynchronize(stream));
    return CAL_OK;
  }
  int timing_enable(int e) override {
    timing = e != 0;
    t_launches = 0;
    t_total_ms = 0;
    ev_used = 0;
    return CAL_OK;
  }
  int timing_get(cal_kernel_timing* out) override {
    if (!out) return fail(CAL_ERR_INVALID, "timing_get: null");
    if (!has_problem) return fail(CAL_ERR_STATE, "timing_get before set_problem");
    out->launches = t_launches;
    out->total_ms = t_total_ms;
    // B_step = s [F sum nvec (A) + 3 F Nbl (d_r, d_i, w) + 2 sum nvec (c) + 2 Na F (g)] + s [10 sum nvec + 10 Na F]
    const double s = sizeof(T);
    out->basis_bytes_per_launch = basis_bytes;
    out->algorithmic_bytes_per_launch =
        basis_bytes + s * (3.0 * nfreqs * nbls + 2.0 * ncoef + 2.0 * nants * nfreqs) + s * (10.0 * ncoef + 10.0 * nants * nfreqs);
    // forward A c and adjoint A^T gbar_v, complex x real: 4 + 4 flops per (channel, vector); the dense path's regularised step
    // runs the forward twice (loss-only pass for S, then the gradient pass) inside the timed region
    // (folded tiles: half the channels are multiplied, like half the basis bytes are read)
    out->flops_per_launch = ((mf_ok && reg == CAL_REG_SUM) ? 12.0 : 8.0) * (fold ? nfreqs / 2 : nfreqs) * (double)ncoef;
    out->basis_folded = fold ? 1 : 0;
    out->reserved = 0;
    out->kernel_path = mf_ok ? ((mf_split || !std::is_same<T, float>::value) ? (mf_split && !mf_split2 ? CAL_PATH_DENSE_SPLIT1 : CAL_PATH_DENSE) : CAL_PATH_DENSE_F32) : CAL_PATH_GENERAL;
    // the dense kernels are written for two workgroups per CU (160 KB of LDS): a basis block of ~250 vectors needs more than
    // 80 KB for its coefficient panel + rings and runs one
    out->dense_wg_per_cu = mf_ok ? (mf_lds_grad[0] * 2 <= 160 * 1024 ? 2 : 1) : 0;
    return CAL_OK;
  }
  int memory_bytes(int64_t* b) override {
    if (!b) return fail(CAL_ERR_INVALID, "memory_bytes: null");
    *b = 0;
    for (const DevBuf* d : bufs) *b += (int64_t)d->bytes;  // every DevBuf member (DevBufRegistry)
    return CAL_OK;
  }
  int comm_init(const void* id, int rk, int nr) override {
    HIP_TRY(hipSetDevice(device));
    if (!id || nr < 1 || rk < 0 || rk >= nr) return fail(CAL_ERR_INVALID, "comm_init: bad rank/nranks");
    if (nccl) {
      (void)ncclCommDestroy(nccl);
      nccl = nullptr;
    }
    ncclUniqueId uid;
    static_assert(sizeof(ncclUniqueId) <= CAL_COMM_ID_BYTES, "unique id does not fit");
    memcpy(&uid, id, sizeof(uid));
    NCCL_TRY(ncclCommInitRank(&nccl, nr, uid, rk));
    hook = nullptr;
    return joined(rk, nr);
  }
  int set_exchange_hook(cal_exchange_fn fn, void* ctx, int rk, int nr) override {
    HIP_TRY(hipSetDevice(device));
    if (fn && (nr < 1 || rk < 0 || rk >= nr)) return fail(CAL_ERR_INVALID, "set_exchange_hook: bad rank/nranks");
    if (nccl) {
      (void)ncclCommDestroy(nccl);
      nccl = nullptr;
    }
    hook = fn;
    hook_ctx = ctx;
    if (!fn) {
      nranks = 1;
      rank = 0;
      local_reg_plan();
      return CAL_OK;
    }
    return joined(rk, nr);
  }
  // how many ranks actually take part in the exchange: every rank contributes 1 to an all-reduce (1 without a communicator)
  int comm_size(int* nranks_seen) override {
    HIP_TRY(hipSetDevice(device));
    if (!nranks_seen) return fail(CAL_ERR_INVALID, "comm_size: null");
    *nranks_seen = 1;
    return agree_ints(nranks_seen, 1, CAL_XCHG_SUM);  // (no communicator: stays 1)
  }
  int joined(int rk, int nr) {
    nranks = nr;
    rank = rk;
    drop_graph();
    if (has_problem) {
      // a problem set before the communicator existed: agree now (fpad is rank-independent by construction; a rank
      // that chose the dense path falls back to the general kernel, which runs on the same buffers)
      CAL_TRY(agree_problem(CAL_OK));
    }
    return CAL_OK;
  }
};

namespace {
template <typename T>
int weighted_square_error(int64_t n, const void* const src[5], double* out) {
  hipStream_t st;
  HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  T* dev = nullptr;
  double* part = nullptr;
  const int nblk = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 2048));
  int rc = CAL_OK;
  auto step = [&](hipError_t e, const char* what) {
    if (rc == CAL_OK && e != hipSuccess) rc = fail(CAL_ERR_HIP, "cal_weighted_square_error: %s failed: %s", what, hipGetErrorString(e));
  };
  step(hipMalloc((void**)&dev, 5 * (size_t)n * sizeof(T)), "hipMalloc");
  step(hipMalloc((void**)&part, (size_t)(nblk + 1) * sizeof(double)), "hipMalloc");
  for (int k = 0; k < 5 && rc == CAL_OK; ++k) step(hipMemcpyAsync(dev + (size_t)k * n, src[k], (size_t)n * sizeof(T), hipMemcpyHostToDevice, st), "upload");
  if (rc == CAL_OK) {
    hipLaunchKernelGGL(square_error_kernel<T>, dim3(nblk), dim3(256), 0, st, dev, dev + n, dev + 2 * n, dev + 3 * n, dev + 4 * n, (long long)n, part);
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, st, part, nblk, part + nblk);
    step(hipGetLastError(), "launch");
    step(hipMemcpyAsync(out, part + nblk, sizeof(double), hipMemcpyDeviceToHost, st), "download");
    step(hipStreamSynchronize(st), "synchronize");
  }
  (void)hipFree(dev);
  (void)hipFree(part);
  (void)hipStreamDestroy(st);
  return rc;
}

}  // namespace

// ================================================================================================================
// cal_debug_plan: the host planner's arrays as bytes
namespace {
template <typename X>
int plan_bytes(const std::vector<X>& v, void* out, int64_t cap, int64_t* bytes, const char* who = "cal_debug_plan") {
  *bytes = (int64_t)(v.size() * sizeof(X));
  if (*bytes > cap) return fail(CAL_ERR_INVALID, "%s: the array has %lld bytes, the buffer %lld", who, (long long)*bytes, (long long)cap);
  if (*bytes) memcpy(out, v.data(), (size_t)*bytes);
  return CAL_OK;
}
template <typename T>
int debug_plan(const cal_problem_desc* d, int what, void* out, int64_t cap, int64_t* bytes) {
  ProblemPlan<T> p;
  CAL_TRY(plan_problem(d, p));
  switch (what) {
    case 0: {
      std::vector<int64_t> v = {p.fpad, p.ncoef, p.nslices, p.na_slice, p.fold, p.small_loads, p.nitems, p.nitems_simple, p.nitems_plain, p.gc_direct, p.gcp_len, 0,
                                p.steps_per_sync, (int64_t)p.lds_bytes, (int64_t)p.lds_group_bytes, (int64_t)p.lds_multi_bytes, (int64_t)p.lds_multi_mfma_bytes,
                                p.mf_ok, p.mf_split, p.mf_split2, p.mf_npanels, p.mf_grid, (int64_t)p.mf_lds_grad[0], (int64_t)p.mf_lds_loss[0], p.nheads, p.nheads_mfma,
                                p.heads_one_pass_local, p.mm_grid, p.lamb_ok, p.lamb_nvar, p.lamb_ncvar};
      memcpy(&v[11], &p.basis_bytes, sizeof(double));
      return plan_bytes(v, out, cap, bytes);
    }
    case 1: return plan_bytes(p.fb_u, out, cap, bytes);
    case 2: return plan_bytes(p.uoff, out, cap, bytes);
    case 3: return plan_bytes(p.bl_tile, out, cap, bytes);
    case 4: return plan_bytes(p.jobs, out, cap, bytes);
    case 5: return plan_bytes(p.grp_coff, out, cap, bytes);
    case 6: return plan_bytes(p.slice_coff, out, cap, bytes);
    case 7: return plan_bytes(p.slice_cblk, out, cap, bytes);
    case 8: return plan_bytes(p.lamb_vars, out, cap, bytes);
    case 9: return plan_bytes(p.lamb_cvar_ptr, out, cap, bytes);
    case 10: return plan_bytes(p.lamb_cvar_slice, out, cap, bytes);
    case 11: return plan_bytes(p.lamb_cvar_id, out, cap, bytes);
    case 12: return plan_bytes(p.runs, out, cap, bytes);
    case 13: return plan_bytes(p.items, out, cap, bytes);
    case 14: return plan_bytes(p.item_goff, out, cap, bytes);
    case 15: return plan_bytes(p.grp_item_ptr, out, cap, bytes);
    case 16: return plan_bytes(p.coef_grp, out, cap, bytes);
    case 17: return plan_bytes(p.slice_ipart_ptr, out, cap, bytes);
    case 18: return plan_bytes(p.slice_ipart_idx, out, cap, bytes);
    case 19: return plan_bytes(p.slice_ppart_ptr, out, cap, bytes);
    case 20: return plan_bytes(p.slice_ppart_idx, out, cap, bytes);
    case 21: return plan_bytes(p.members, out, cap, bytes);
    case 22: return plan_bytes(p.heads, out, cap, bytes);
    case 23: return plan_bytes(p.panels, out, cap, bytes);
    case 24: return plan_bytes(p.panel_map, out, cap, bytes);
    case 25: return plan_bytes(p.op_off, out, cap, bytes);
    case 26: return plan_bytes(p.cs_grp, out, cap, bytes);
    case 27: return plan_bytes(p.ant_ptr, out, cap, bytes);
    case 28: return plan_bytes(p.ant_ent, out, cap, bytes);
  }
  return fail(CAL_ERR_INVALID, "cal_debug_plan: what = %d", what);
}
// cal_debug_solve_plan: the arrays of solve_plan.hpp as bytes
template <typename T>
int debug_solve_plan(const cal_problem_desc* d, int64_t bound, int what, void* out, int64_t cap, int64_t* bytes) {
  const char* who = "cal_debug_solve_plan";
  auto give = [&](const auto& v) { return plan_bytes(v, out, cap, bytes, who); };
  ProblemPlan<T> p;
  CAL_TRY(plan_problem(d, p));
  if (what == 20 || what == 21) {
    std::vector<int> ptr;
    std::vector<int2> ent;
    antenna_lists(p.nants, p.bl_ant, true, ptr, ent);
    return what == 20 ? give(ptr) : give(ent);
  }
  if (what == 30) {
    const int64_t* in = static_cast<const int64_t*>(out);
    if (cap < 24 || in[0] < 0 || in[1] < 0 || in[0] + in[1] == 0 || (in[1] > 0 && (in[2] < 1 || p.nants % in[2] != 0)))
      return fail(CAL_ERR_INVALID, "%s: what = 30 takes K, L, T (K + L > 0; T divides nants) in the first 24 bytes of out", who);
    const int K = (int)in[0], L = (int)in[1], Tn = (int)in[2];
    const RowChunks r = plan_row_chunks(K, L, Tn, p.nfreqs, sizeof(T), bound, L > 0 ? p.nants / Tn : p.nants);
    return give(std::vector<int64_t>{r.rows, r.in_lds, (int64_t)r.lds, r.n, r.m_row, r.n_row, r.d_row});
  }
  if (what == 31) {  // gain_basis_errors: the same rows with W counted
    const int64_t* in = static_cast<const int64_t*>(out);
    if (cap < 24 || in[0] < 0 || in[1] < 0 || in[0] + in[1] == 0 || (in[1] > 0 && (in[2] < 1 || p.nants % in[2] != 0)))
      return fail(CAL_ERR_INVALID, "%s: what = 31 takes K, L, T (K + L > 0; T divides nants) in the first 24 bytes of out", who);
    const int K = (int)in[0], L = (int)in[1], Tn = (int)in[2];
    const RowChunks r = plan_row_chunks(K, L, Tn, p.nfreqs, sizeof(T), bound, L > 0 ? p.nants / Tn : p.nants, gain_error_extra(K, L));
    return give(std::vector<int64_t>{r.rows, r.in_lds, (int64_t)r.lds, r.n, r.m_row, r.n_row, r.d_row, r.x_row});
  }
  if (what < 0 || what >= 20 || what % 10 > 6) return fail(CAL_ERR_INVALID, "%s: what = %d", who, what);
  const bool fe = what >= 10;
  GroupPlan P = plan_group_chunks(p.cs_grp, sizeof(T), bound, fe ? fit_error_extra(p.cs_grp) : std::vector<long long>{});
  if (fe) plan_leverage_work(P, p.cs_grp, p.bl_tile, p.fold ? p.nfreqs / 2 : p.fpad);
  switch (what % 10) {
    case 0: return give(std::vector<int64_t>{P.n_max, P.d_max, P.x_max, P.npieces, (int64_t)P.chunks.size()});
    case 1: return give(p.cs_grp);
    case 2: return give(P.order);
    case 3: return give(P.work);
    case 4: return give(P.chunks);
    case 5: return give(P.xoff);
  }
  return give(P.lwork);
}
// cal_debug_delay_coherent_plan: plan_delay_coherent's arrays as bytes
template <typename T>
int debug_delay_coherent_plan(const cal_problem_desc* d, const cal_delay_coherent_desc* x, int64_t scratch_bytes, int what, void* out, int64_t cap, int64_t* bytes) {
  const char* who = "cal_debug_delay_coherent_plan";
  auto give = [&](const auto& v) { return plan_bytes(v, out, cap, bytes, who); };
  ProblemPlan<T> p;
  CAL_TRY(plan_problem(d, p));
  if (what < 70 || what > 77) return fail(CAL_ERR_INVALID, "%s: what = %d", who, what);
  if (x->ndelays < 1 || (x->what & 7) == 0 || (x->what & ~7) || x->nbins < 0 || (x->nbins == 0) != (x->bin_of_group == nullptr) || !x->op_r || !x->op_i ||
      !x->norm_f || scratch_bytes < 0)
    return fail(CAL_ERR_INVALID, "%s: what = %d takes a description cal_solver_delay_coherent_spectrum would plan for, and a bound >= 0", who, what);
  DelayCoherentPlan<T> P;
  CAL_TRY(plan_delay_coherent(p.nbls, p.nfreqs, p.fpad, x, scratch_bytes == 0 ? kCsScratchDefault : scratch_bytes, P));
  const DelayFringePlan<T>& F = P.F;
  switch (what) {
    case 70:
      return give(std::vector<int64_t>{F.nq, F.xpitch, F.ndpad, F.cgroups, F.nchunks, (int64_t)F.n_x, (int64_t)(F.n_y + F.n_pow), (int64_t)F.n_out,
                                       (int64_t)P.n_mask, P.nspans});
    case 71: return give(F.bin_ent);
    case 72: return give(F.chunk_ptr);
    case 73: return give(F.image);
    case 74: return give(F.norm_f);
    case 75: return give(F.scale);
    case 76: return give(F.opt);
  }
  return give(P.chunk_members);
}

// cal_debug_report_plan: the arrays of report_plan.hpp as bytes
template <typename T>
int debug_report_plan(const cal_problem_desc* d, const cal_report_plan_desc* r, int what, void* out, int64_t cap, int64_t* bytes) {
  const char* who = "cal_debug_report_plan";
  auto give = [&](const auto& v) { return plan_bytes(v, out, cap, bytes, who); };
  ProblemPlan<T> p;
  CAL_TRY(plan_problem(d, p));
  if (what >= 0 && what <= 4) {
    const cal_delay_spectrum_desc* s = r->spectrum;
    if (!s || s->ndelays < 1 || (s->what & 7) == 0 || (s->what & ~7) || s->nbins < 0 || (s->nbins == 0) != (s->bin_of_bl == nullptr) || !s->op_r || !s->op_i ||
        !s->norm_f || r->scratch_bytes < 0)
      return fail(CAL_ERR_INVALID, "%s: what = %d takes a spectrum description cal_solver_delay_spectrum would plan for, and a bound >= 0", who, what);
    DelaySpectrumPlan<T> P;
    CAL_TRY(plan_delay_spectrum(p.nbls, p.nfreqs, p.fpad, s, r->scratch_bytes == 0 ? kCsScratchDefault : r->scratch_bytes, r->with_power_bl != 0 || s->nbins > 0, P));
    switch (what) {
      case 0: return give(std::vector<int64_t>{P.nq, P.xpitch, P.ndpad, P.crows, P.nchunks, (int64_t)P.n_x, (int64_t)P.n_pow, (int64_t)P.n_out});
      case 1: return give(P.bin_ent);
      case 2: return give(P.chunk_ptr);
      case 3: return give(P.image);
    }
    return give(P.norm_f);
  }
  if (what >= 10 && what <= 19) {
    const cal_degeneracy_desc* g = r->degeneracy;
    const int nsl = r->nslices ? r->nslices : p.nslices;
    if (!g || (g->mode != CAL_DEGEN_CHANNEL && g->mode != CAL_DEGEN_BAND) || !g->antpos || (g->mode == CAL_DEGEN_BAND && !g->freqs) || nsl < 1 || p.nants % nsl != 0)
      return fail(CAL_ERR_INVALID, "%s: what = %d takes a mode, antpos, freqs for CAL_DEGEN_BAND, and a number of slices that divides nants", who, what);
    DegeneracyPlan P;
    CAL_TRY(plan_degeneracies(p.bl_ant, p.nants, nsl, p.nfreqs, p.fpad, g->mode == CAL_DEGEN_BAND, g->antpos, g->freqs, P));
    switch (what) {
      case 10: return give(std::vector<int64_t>{P.nseg, (int64_t)P.geo_pos(), (int64_t)P.geo_ratio(), (int64_t)P.geo_maxd(), (int64_t)P.idx_segptr(), (int64_t)P.idx_segs()});
      case 11: return give(P.d_b);
      case 12: return give(P.pos);
      case 13: return give(P.ratio);
      case 14: return give(P.maxd);
      case 15: return give(P.ent);
      case 16: return give(P.segptr);
      case 17: return give(P.segs);
      case 18: return give(P.pack_geo());
    }
    return give(P.pack_idx());
  }
  if (what >= 40 && what <= 48) {
    const cal_delay_transfer_desc* t = r->transfer;
    if (!t || t->ndelays < 1 || t->nbins < 0 || (t->nbins == 0) != (t->bin_of_bl == nullptr) || !t->op_r || !t->op_i || r->scratch_bytes < 0)
      return fail(CAL_ERR_INVALID, "%s: what = %d takes a transfer description cal_solver_delay_transfer would plan for, and a bound >= 0", who, what);
    DelayTransferPlan<T> P;
    CAL_TRY(plan_delay_transfer(p.cs_grp, p.bl_tile, p.nbls, p.nfreqs, p.fpad, p.fold, t, r->scratch_bytes == 0 ? kCsScratchDefault : r->scratch_bytes, P));
    switch (what) {
      case 40: return give(std::vector<int64_t>{P.xpitch, P.ndpad, P.npieces, P.G.n_max, P.G.d_max, P.G.x_max, (int64_t)P.chunks.size(), (int64_t)P.runs.size(),
                                                (int64_t)P.rows.size(), (int64_t)P.n_rows_out, (int64_t)P.n_out});
      case 41: return give(P.grp);
      case 42: return give(P.G.order);
      case 43: return give(P.chunks);
      case 44: return give(P.G.xoff);
      case 45: return give(P.runs);
      case 46: return give(P.rows);
      case 47: return give(P.bin_ent);
    }
    return give(P.bin_ptr2);
  }
  if (what >= 60 && what <= 65) {
    const cal_delay_cross_desc* x = r->cross;
    if (!x || x->ndelays < 1 || (x->what & 7) == 0 || (x->what & ~7) || x->nbins < 0 || (x->nbins == 0) != (x->bin_of_pair == nullptr) || !x->op_r || !x->op_i ||
        !x->norm_f || r->scratch_bytes < 0)
      return fail(CAL_ERR_INVALID, "%s: what = %d takes a cross description cal_solver_delay_cross_spectrum would plan for, and a bound >= 0", who, what);
    DelayCrossPlan<T> P;
    CAL_TRY(plan_delay_cross(p.nbls, p.nfreqs, p.fpad, x, r->scratch_bytes == 0 ? kCsScratchDefault : r->scratch_bytes, P));
    switch (what) {
      case 60: return give(std::vector<int64_t>{P.nq, P.nstat, P.xpitch, P.ndpad, P.cpairs, P.nchunks, (int64_t)P.n_x, (int64_t)P.n_pow, (int64_t)P.n_out});
      case 61: return give(P.bin_ent);
      case 62: return give(P.chunk_ptr);
      case 63: return give(P.image);
      case 64: return give(P.norm_f);
    }
    return give(P.scale);
  }
  if (what >= 70 && what <= 76) {
    const cal_delay_fringe_desc* x = r->fringe;
    if (!x || x->ndelays < 1 || (x->what & 7) == 0 || (x->what & ~7) || x->nbins < 0 || (x->nbins == 0) != (x->bin_of_group == nullptr) || !x->op_r || !x->op_i ||
        !x->norm_f || r->scratch_bytes < 0)
      return fail(CAL_ERR_INVALID, "%s: what = %d takes a fringe description cal_solver_delay_fringe_spectrum would plan for, and a bound >= 0", who, what);
    DelayFringePlan<T> P;
    CAL_TRY(plan_delay_fringe(p.nbls, p.nfreqs, p.fpad, x, r->scratch_bytes == 0 ? kCsScratchDefault : r->scratch_bytes, P));
    switch (what) {
      case 70: return give(std::vector<int64_t>{P.nq, P.xpitch, P.ndpad, P.cgroups, P.nchunks, (int64_t)P.n_x, (int64_t)(P.n_y + P.n_pow), (int64_t)P.n_out});
      case 71: return give(P.bin_ent);
      case 72: return give(P.chunk_ptr);
      case 73: return give(P.image);
      case 74: return give(P.norm_f);
      case 75: return give(P.scale);
    }
    return give(P.opt);
  }
  return fail(CAL_ERR_INVALID, "%s: what = %d", who, what);
}
}  // namespace

// ================================================================================================================
// cal_mixed_comps_*, cal_simple_cov_matrix: the kernels of mixed_comps_kernels.hpp
namespace {
int mx_use_device(int device, const char* who) {
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return fail(CAL_ERR_HIP, "no usable HIP device (%s); this library has no CPU fallback", e == hipSuccess ? "0 devices" : hipGetErrorString(e));
  if (device < 0 || device >= ndev) return fail(CAL_ERR_INVALID, "%s: device %d out of range [0, %d)", who, device, ndev);
  HIP_TRY(hipSetDevice(device));
  return CAL_OK;
}
// (u, v, w, nu) of every sample of nbls baselines on nfreqs channels, baseline-major, appended to `out`: pts = uvw * (nu / 3e8) as
// simple_cov_matrix forms it
int mx_samples(const char* who, int64_t nbls, const double* uvw, int32_t nfreqs, const double* freqs, std::vector<double>& out) {
  for (int64_t x = 0; x < nbls * 3; ++x)
    if (!std::isfinite(uvw[x])) return fail(CAL_ERR_INVALID, "%s: uvw is not finite", who);
  for (int32_t f = 0; f < nfreqs; ++f)
    if (!std::isfinite(freqs[f])) return fail(CAL_ERR_INVALID, "%s: freqs is not finite", who);
  size_t o = out.size();
  out.resize(o + (size_t)nbls * nfreqs * 4);
  for (int64_t a = 0; a < nbls; ++a)
    for (int32_t f = 0; f < nfreqs; ++f) {
      const double s = freqs[f] / 3e8;
      out[o++] = uvw[3 * a] * s;
      out[o++] = uvw[3 * a + 1] * s;
      out[o++] = uvw[3 * a + 2] * s;
      out[o++] = freqs[f];
    }
  return CAL_OK;
}
bool mx_params_ok(double ant_dly, double horizon, double offset, double min_dly) {
  return std::isfinite(ant_dly) && std::isfinite(horizon) && std::isfinite(offset) && std::isfinite(min_dly);
}
long long mx_group_bytes(int ldl, int nblk, int cap) {  // a group's share of a chunk's scratch at rank cap `cap`
  return (long long)ldl * ((cap + 15) / 16 * 16) * 8 + (long long)ldl * 8 + 2ll * nblk * (long long)sizeof(MxPart) + (long long)cap * 4;
}
struct MxEvents {
  hipEvent_t e[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  ~MxEvents() {
    for (hipEvent_t x : e)
      if (x) (void)hipEventDestroy(x);
  }
  int create() {
    for (hipEvent_t& x : e) HIP_TRY(hipEventCreate(&x));
    return CAL_OK;
  }
};
constexpr int kMxStepsPerRead = 32;  // steps enqueued between two reads of the chunk's count of finished groups
}  // namespace

struct cal_mixed_comps {
  int device = 0;
  hipStream_t st = nullptr;
  MxParams P{};
  double tol = 0;
  std::vector<MxGroup> grps;                 // every group of the call, L the compact factor
  std::vector<std::unique_ptr<DevBuf>> Lc;   // [ldl][kpad] per group
  std::vector<std::vector<int>> piv;
  std::vector<int> status, chunk;  // chunk: the chunk a group was factored in
  std::vector<double> maxd, resid_fro, G;
  DevBuf samples, dev_grps;
  double ms[3] = {0, 0, 0};  // factor, Gram, certificate
  ~cal_mixed_comps() {
    if (st) (void)hipStreamDestroy(st);
  }

  int upload_groups() {
    CAL_TRY(dev_grps.reserve(grps.size() * sizeof(MxGroup), false));
    HIP_TRY(hipMemcpyAsync(dev_grps.p, grps.data(), grps.size() * sizeof(MxGroup), hipMemcpyHostToDevice, st));
    return CAL_OK;
  }

  int run(const cal_mixed_comps_desc* d) {
    const char* who = "cal_mixed_comps_create";
    const int ng = d->ngroups;
    const int64_t bound = d->scratch_bytes == 0 ? kCsScratchDefault : d->scratch_bytes;
    P = MxParams{d->ant_dly, d->horizon, d->offset, d->min_dly};
    tol = d->tol;
    // a group's channels: all nfreqs of them, or its own piece [grp_freq_start[g], grp_freq_start[g + 1]) of freqs
    auto f0 = [&](int g) { return d->grp_freq_start ? d->grp_freq_start[g] : 0; };
    auto f1 = [&](int g) { return d->grp_freq_start ? d->grp_freq_start[g + 1] : d->nfreqs; };
    std::vector<double> smp;
    std::vector<long long> s_off(ng + 1, 0);
    for (int g = 0; g < ng; ++g) {
      const int64_t nb = (int64_t)d->grp_bl_start[g + 1] - d->grp_bl_start[g];
      if (nb <= 0 || d->grp_bl_start[0] != 0) return fail(CAL_ERR_INVALID, "%s: grp_bl_start must start at 0 and ascend", who);
      if (f0(g) < 0 || f1(g) <= f0(g) || f1(g) > d->nfreqs) return fail(CAL_ERR_INVALID, "%s: grp_freq_start must ascend within [0, nfreqs]", who);
      if (nb * (f1(g) - f0(g)) > (1 << 22)) return fail(CAL_ERR_INVALID, "%s: a group holds at most 2^22 samples", who);
      CAL_TRY(mx_samples(who, nb, d->uvw + 3 * (size_t)d->grp_bl_start[g], f1(g) - f0(g), d->freqs + f0(g), smp));
      s_off[g + 1] = (long long)(smp.size() / 4);
    }
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    CAL_TRY(samples.alloc(smp.size() * sizeof(double), false));
    HIP_TRY(hipMemcpyAsync(samples.p, smp.data(), smp.size() * sizeof(double), hipMemcpyHostToDevice, st));
    grps.assign(ng, MxGroup{});
    Lc.resize(ng);
    piv.resize(ng);
    status.assign(ng, MX_NOT_RUN);
    chunk.assign(ng, 0);
    maxd.assign(ng, 0.0);
    resid_fro.assign(ng, 0.0);
    for (int g = 0; g < ng; ++g) {
      MxGroup& q = grps[g];
      q.n = (int)(s_off[g + 1] - s_off[g]);
      q.ldl = (q.n + 63) / 64 * 64;
      q.nblk = (q.n + kMxRows - 1) / kMxRows;
      q.s_off = s_off[g];
      // what the group asks of the bound: a third of its order (the ranks of these matrices stay below a quarter); what it gets alone
      // in a chunk when that does not fit: the columns the bound holds, in sixteens
      q.cap = std::min(std::min(q.n, kMxMaxCap), std::max(64, (q.n + 2) / 3));
      if (mx_group_bytes(q.ldl, q.nblk, q.cap) > bound) {
        const long long fixed = mx_group_bytes(q.ldl, q.nblk, 0);
        const long long cols = bound > fixed ? (bound - fixed) / ((long long)q.ldl * 8 + 4) : 0;
        q.cap = (int)std::min<long long>(q.cap, cols / 16 * 16);
      }
    }
    MxEvents ev;
    CAL_TRY(ev.create());
    HIP_TRY(hipEventRecord(ev.e[0], st));
    DevBuf scratch, d_work, d_state;
    int nchunks = 0;
    for (int g0 = 0; g0 < ng;) {
      // the chunk: consecutive groups while their shares fit the bound (a group alone always fits: its cap was cut to it)
      int g1 = g0;
      long long bytes = 0;
      while (g1 < ng && (g1 == g0 || bytes + mx_group_bytes(grps[g1].ldl, grps[g1].nblk, grps[g1].cap) <= bound)) {
        bytes += mx_group_bytes(grps[g1].ldl, grps[g1].nblk, grps[g1].cap);
        ++g1;
      }
      std::vector<int> run_g;  // groups of the chunk that have a column to compute
      for (int g = g0; g < g1; ++g) chunk[g] = nchunks;
      ++nchunks;
      for (int g = g0; g < g1; ++g)
        if (grps[g].cap >= 1) run_g.push_back(g);
      if (!run_g.empty()) {
        CAL_TRY(scratch.reserve((size_t)bytes + 256 * run_g.size(), false));
        HIP_TRY(hipMemsetAsync(scratch.p, 0, scratch.bytes, st));
        std::vector<MxGroup> cg;
        std::vector<int2> work;
        char* base = scratch.as<char>();
        size_t off = 0;
        int maxcap = 0;
        auto take = [&](size_t nbytes) {
          char* ptr = base + off;
          off += (nbytes + 63) / 64 * 64;
          return ptr;
        };
        for (int g : run_g) {
          MxGroup q = grps[g];
          q.L = reinterpret_cast<double*>(take((size_t)q.ldl * ((q.cap + 15) / 16 * 16) * 8));
          q.d = reinterpret_cast<double*>(take((size_t)q.ldl * 8));
          maxcap = std::max(maxcap, q.cap);
          for (int b = 0; b < q.nblk; ++b) work.push_back(int2{(int)cg.size(), b});
          cg.push_back(q);
        }
        for (MxGroup& q : cg) q.part = reinterpret_cast<MxPart*>(take(2 * (size_t)q.nblk * sizeof(MxPart)));  // two buffers, by step parity
        for (MxGroup& q : cg) q.piv = reinterpret_cast<int*>(take((size_t)q.cap * 4));
        if (off > scratch.bytes) return fail(CAL_ERR_STATE, "%s: the chunk's plan (%zu bytes) exceeds its scratch (%zu)", who, off, scratch.bytes);
        const int nc = (int)cg.size();
        CAL_TRY(d_work.reserve(work.size() * sizeof(int2) + cg.size() * sizeof(MxGroup), false));
        CAL_TRY(d_state.reserve(nc * sizeof(MxState) + 64, false));
        MxGroup* dg = reinterpret_cast<MxGroup*>(d_work.as<char>() + work.size() * sizeof(int2));
        HIP_TRY(hipMemcpyAsync(d_work.p, work.data(), work.size() * sizeof(int2), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(dg, cg.data(), cg.size() * sizeof(MxGroup), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(d_state.p, 0, d_state.bytes, st));
        MxState* dstate = d_state.as<MxState>();
        int* dn = reinterpret_cast<int*>(d_state.as<char>() + (size_t)nc * sizeof(MxState));
        const dim3 grid((unsigned)work.size());
        hipLaunchKernelGGL(mixed_init_kernel, grid, dim3(256), 0, st, dg, d_work.as<int2>(), samples.as<double4>(), P);
        int ndone = 0;
        for (int step = 0; step <= maxcap && ndone < nc;) {  // step == cap is the launch that records a group at its cap
          const int to = std::min(maxcap + 1, step + kMxStepsPerRead);
          for (; step < to; ++step)
            hipLaunchKernelGGL(mixed_step_kernel, grid, dim3(256), (size_t)maxcap * 8, st, dg, d_work.as<int2>(), samples.as<double4>(), dstate, dn, P, tol,
                               step);
          HIP_TRY(hipGetLastError());
          HIP_TRY(hipMemcpyAsync(&ndone, dn, sizeof(int), hipMemcpyDeviceToHost, st));
          HIP_TRY(hipStreamSynchronize(st));
        }
        if (ndone != nc) return fail(CAL_ERR_STATE, "%s: %d of %d groups finished within their caps", who, ndone, nc);
        std::vector<MxState> hs(nc);
        HIP_TRY(hipMemcpyAsync(hs.data(), dstate, nc * sizeof(MxState), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int c = 0; c < nc; ++c) {
          const int g = run_g[c];
          MxGroup& q = grps[g];
          q.k = hs[c].k;
          q.kpad = std::max(16, (q.k + 15) / 16 * 16);
          if (q.k < 0 || q.k > q.cap) return fail(CAL_ERR_STATE, "%s: group %d reports rank %d at cap %d", who, g, q.k, q.cap);
          status[g] = hs[c].status;
          maxd[g] = hs[c].maxd;
          Lc[g] = std::make_unique<DevBuf>();
          // (column-major: the first kpad columns are one piece; kpad <= the cap rounded up to 16, and columns [k, kpad) were never written)
          const size_t lbytes = (size_t)q.ldl * std::min(q.kpad, (q.cap + 15) / 16 * 16) * 8;
          CAL_TRY(Lc[g]->alloc((size_t)q.ldl * q.kpad * 8, true));
          HIP_TRY(hipMemcpyAsync(Lc[g]->p, cg[c].L, lbytes, hipMemcpyDeviceToDevice, st));
          piv[g].resize(q.k);
          if (q.k) HIP_TRY(hipMemcpyAsync(piv[g].data(), cg[c].piv, (size_t)q.k * 4, hipMemcpyDeviceToHost, st));
          q.L = Lc[g]->as<double>();
        }
        HIP_TRY(hipStreamSynchronize(st));
      }
      g0 = g1;
    }
    scratch.release();
    HIP_TRY(hipEventRecord(ev.e[1], st));
    // G of every factored group in one launch, one buffer, one download; then the certificate the same way
    std::vector<MxWork> gw, cw;
    long long g_total = 0, c_total = 0;
    for (int g = 0; g < ng; ++g) {
      MxGroup& q = grps[g];
      q.d = nullptr;
      q.part = nullptr;
      q.piv = nullptr;
      q.g_off = g_total;
      q.c_off = c_total;
      if (status[g] == MX_NOT_RUN) continue;
      g_total += (long long)q.k * q.k;
      const int nb = (q.k + kNsBlock - 1) / kNsBlock, nt = (q.n + kMxTile - 1) / kMxTile;
      for (int bi = 0; bi < nb; ++bi)
        for (int bj = 0; bj <= bi; ++bj) gw.push_back(MxWork{g, bi, bj});
      for (int bi = 0; bi < nt; ++bi)
        for (int bj = 0; bj <= bi; ++bj) cw.push_back(MxWork{g, bi, bj});
      c_total += (long long)nt * (nt + 1) / 2;
    }
    CAL_TRY(upload_groups());
    G.assign((size_t)g_total, 0.0);
    std::vector<double> r2(ng, 0.0);
    DevBuf d_G, d_c, d_r2;
    CAL_TRY(d_G.alloc((size_t)g_total * 8, true));
    CAL_TRY(d_c.alloc((size_t)c_total * 8, true));
    CAL_TRY(d_r2.alloc((size_t)ng * 8, true));
    HIP_TRY(hipEventRecord(ev.e[2], st));
    if (!gw.empty()) {
      CAL_TRY(d_work.reserve(gw.size() * sizeof(MxWork), false));
      HIP_TRY(hipMemcpyAsync(d_work.p, gw.data(), gw.size() * sizeof(MxWork), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(mixed_gram_kernel, dim3((unsigned)gw.size()), dim3(256), 0, st, dev_grps.as<MxGroup>(), d_work.as<MxWork>(), d_G.as<double>());
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ev.e[3], st));
    HIP_TRY(hipStreamSynchronize(st));  // (d_work is reused)
    HIP_TRY(hipEventRecord(ev.e[4], st));
    if (!cw.empty()) {
      CAL_TRY(d_work.reserve(cw.size() * sizeof(MxWork), false));
      HIP_TRY(hipMemcpyAsync(d_work.p, cw.data(), cw.size() * sizeof(MxWork), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(mixed_cert_kernel, dim3((unsigned)cw.size()), dim3(256), 0, st, dev_grps.as<MxGroup>(), d_work.as<MxWork>(), samples.as<double4>(), P,
                         d_c.as<double>());
      hipLaunchKernelGGL(mixed_cert_sum_kernel, dim3(ng), dim3(256), 0, st, dev_grps.as<MxGroup>(), d_c.as<double>(), d_r2.as<double>());
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ev.e[5], st));
    if (g_total) HIP_TRY(hipMemcpyAsync(G.data(), d_G.p, (size_t)g_total * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(r2.data(), d_r2.p, (size_t)ng * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int g = 0; g < ng; ++g) {
      resid_fro[g] = status[g] == MX_NOT_RUN ? 0.0 : std::sqrt(r2[g]);
      if (status[g] == MX_NOT_RUN) continue;
      // normal_gram_store leaves the lower triangle: mirror it
      double* Gg = G.data() + grps[g].g_off;
      const int k = grps[g].k;
      for (int i = 0; i < k; ++i)
        for (int j = i + 1; j < k; ++j) Gg[(size_t)i * k + j] = Gg[(size_t)j * k + i];
    }
    for (int x = 0; x < 3; ++x) {
      float t = 0;
      HIP_TRY(hipEventElapsedTime(&t, ev.e[2 * x], ev.e[2 * x + 1]));
      ms[x] = t;
    }
    return CAL_OK;
  }

  template <typename T>
  int vectors(const int32_t* nkeep, const double* U, const double* scale, void* V, double* ms_out) {
    const int ng = (int)grps.size();
    std::vector<MxWork> work;
    long long u_total = 0, s_total = 0, v_total = 0;
    for (int g = 0; g < ng; ++g) {
      MxGroup& q = grps[g];
      if (nkeep[g] < 0 || nkeep[g] > q.k || (nkeep[g] > 0 && status[g] == MX_NOT_RUN))
        return fail(CAL_ERR_INVALID, "cal_mixed_comps_vectors: group %d keeps %d of %d vectors", g, nkeep[g], q.k);
      q.r = nkeep[g];
      q.u_off = u_total;
      q.sc_off = s_total;
      q.v_off = v_total;
      u_total += (long long)q.k * q.r;
      s_total += q.r;
      v_total += (long long)q.n * q.r;
      if (q.r == 0) continue;
      for (int bi = 0; bi < (q.n + kMxTile - 1) / kMxTile; ++bi)
        for (int bj = 0; bj < (q.r + kMxTile - 1) / kMxTile; ++bj) work.push_back(MxWork{g, bi, bj});
    }
    if (ms_out) *ms_out = 0.0;
    if (work.empty()) return CAL_OK;
    CAL_TRY(upload_groups());
    DevBuf d_u, d_v, d_work;
    MxEvents ev;
    CAL_TRY(ev.create());
    CAL_TRY(d_u.alloc((size_t)(u_total + s_total) * 8, false));
    CAL_TRY(d_v.alloc((size_t)v_total * sizeof(T), false));
    CAL_TRY(d_work.alloc(work.size() * sizeof(MxWork), false));
    HIP_TRY(hipMemcpyAsync(d_u.p, U, (size_t)u_total * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_u.as<double>() + u_total, scale, (size_t)s_total * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_work.p, work.data(), work.size() * sizeof(MxWork), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(ev.e[0], st));
    hipLaunchKernelGGL(mixed_backmul_kernel<T>, dim3((unsigned)work.size()), dim3(256), 0, st, dev_grps.as<MxGroup>(), d_work.as<MxWork>(), d_u.as<double>(),
                       d_u.as<double>() + u_total, d_v.as<T>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.e[1], st));
    HIP_TRY(hipMemcpyAsync(V, d_v.p, (size_t)v_total * sizeof(T), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, ev.e[0], ev.e[1]));
    if (ms_out) *ms_out = t;
    return CAL_OK;
  }
};

extern "C" {

int cal_mixed_comps_create(cal_mixed_comps** out, int device, const cal_mixed_comps_desc* d) {
  const char* who = "cal_mixed_comps_create";
  if (!out) return fail(CAL_ERR_INVALID, "%s: null handle pointer", who);
  *out = nullptr;
  if (!d || d->ngroups < 1 || d->nfreqs < 1 || !d->grp_bl_start || !d->uvw || !d->freqs) return fail(CAL_ERR_INVALID, "%s: the description needs groups, uvw and freqs", who);
  if (!mx_params_ok(d->ant_dly, d->horizon, d->offset, d->min_dly)) return fail(CAL_ERR_INVALID, "%s: ant_dly, horizon, offset and min_dly must be finite", who);
  if (!(d->tol > 0.0) || !std::isfinite(d->tol)) return fail(CAL_ERR_INVALID, "%s: tol must be finite and > 0", who);
  if (d->scratch_bytes < 0) return fail(CAL_ERR_INVALID, "%s: negative scratch bound", who);
  CAL_TRY(mx_use_device(device, who));
  std::unique_ptr<cal_mixed_comps> h(new cal_mixed_comps());
  h->device = device;
  CAL_TRY(h->run(d));
  *out = h.release();
  return CAL_OK;
}

int cal_mixed_comps_destroy(cal_mixed_comps* h) {
  if (!h) return fail(CAL_ERR_INVALID, "cal_mixed_comps_destroy: null handle");
  (void)hipSetDevice(h->device);
  delete h;
  return CAL_OK;
}

int cal_mixed_comps_info(cal_mixed_comps* h, int32_t* rank, int32_t* status, int32_t* chunk, double* max_d, double* resid_fro, double* times_ms) {
  if (!h) return fail(CAL_ERR_INVALID, "cal_mixed_comps_info: null handle");
  for (size_t g = 0; g < h->grps.size(); ++g) {
    if (rank) rank[g] = h->grps[g].k;
    if (status) status[g] = h->status[g];
    if (chunk) chunk[g] = h->chunk[g];
    if (max_d) max_d[g] = h->maxd[g];
    if (resid_fro) resid_fro[g] = h->resid_fro[g];
  }
  if (times_ms) memcpy(times_ms, h->ms, sizeof(h->ms));
  return CAL_OK;
}

int cal_mixed_comps_gram(cal_mixed_comps* h, double* G, int64_t cap_doubles) {
  if (!h || !G) return fail(CAL_ERR_INVALID, "cal_mixed_comps_gram: null argument");
  if ((int64_t)h->G.size() > cap_doubles) return fail(CAL_ERR_INVALID, "cal_mixed_comps_gram: G has %lld doubles, the buffer %lld", (long long)h->G.size(), (long long)cap_doubles);
  if (!h->G.empty()) memcpy(G, h->G.data(), h->G.size() * 8);
  return CAL_OK;
}

int cal_mixed_comps_vectors(cal_mixed_comps* h, int dtype, const int32_t* nkeep, const double* U, const double* scale, void* V, double* ms) {
  if (!h || !nkeep || !U || !scale || !V) return fail(CAL_ERR_INVALID, "cal_mixed_comps_vectors: null argument");
  if (dtype != CAL_F32 && dtype != CAL_F64) return fail(CAL_ERR_INVALID, "cal_mixed_comps_vectors: unknown dtype %d", dtype);
  HIP_TRY(hipSetDevice(h->device));
  return dtype == CAL_F32 ? h->vectors<float>(nkeep, U, scale, V, ms) : h->vectors<double>(nkeep, U, scale, V, ms);
}

int cal_mixed_comps_factor(cal_mixed_comps* h, int32_t group, double* L, int32_t* pivots) {
  if (!h || group < 0 || group >= (int32_t)h->grps.size()) return fail(CAL_ERR_INVALID, "cal_mixed_comps_factor: no such group");
  const MxGroup& q = h->grps[group];
  if (h->status[group] == MX_NOT_RUN || q.k == 0) return CAL_OK;
  HIP_TRY(hipSetDevice(h->device));
  if (L) {  // (on the handle's stream, not the legacy one: see cal_simple_cov_matrix)
    HIP_TRY(hipMemcpy2DAsync(L, (size_t)q.n * 8, q.L, (size_t)q.ldl * 8, (size_t)q.n * 8, (size_t)q.k, hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
  }
  if (pivots) memcpy(pivots, h->piv[group].data(), (size_t)q.k * 4);
  return CAL_OK;
}

int cal_simple_cov_matrix(int device, int32_t nbls, const double* uvw, int32_t nfreqs, const double* freqs, double ant_dly, double horizon, double offset,
                          double min_dly, double* C) {
  const char* who = "cal_simple_cov_matrix";
  if (nbls < 1 || nfreqs < 1 || !uvw || !freqs || !C) return fail(CAL_ERR_INVALID, "%s: bad argument", who);
  if (!mx_params_ok(ant_dly, horizon, offset, min_dly)) return fail(CAL_ERR_INVALID, "%s: ant_dly, horizon, offset and min_dly must be finite", who);
  const int64_t n = (int64_t)nbls * nfreqs;
  if (n > 46340) return fail(CAL_ERR_INVALID, "%s: %lld samples: the dense matrix is for orders up to 46340", who, (long long)n);
  CAL_TRY(mx_use_device(device, who));
  std::vector<double> smp;
  CAL_TRY(mx_samples(who, nbls, uvw, nfreqs, freqs, smp));
  DevBuf d_s, d_c;
  CAL_TRY(d_s.alloc(smp.size() * 8, false));
  CAL_TRY(d_c.alloc((size_t)n * n * 8, false));
  hipStream_t st;  // (its own stream: the legacy stream would synchronise with a solver that captures a graph on another thread)
  HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  int rc = CAL_OK;
  auto step = [&](hipError_t e, const char* what) {
    if (rc == CAL_OK && e != hipSuccess) rc = fail(CAL_ERR_HIP, "%s: %s failed: %s", who, what, hipGetErrorString(e));
  };
  step(hipMemcpyAsync(d_s.p, smp.data(), smp.size() * 8, hipMemcpyHostToDevice, st), "upload");
  if (rc == CAL_OK) {
    hipLaunchKernelGGL(mixed_dense_kernel, dim3(grid_for(n * n)), dim3(256), 0, st, d_s.as<double4>(), (int)n, MxParams{ant_dly, horizon, offset, min_dly},
                       d_c.as<double>());
    step(hipGetLastError(), "launch");
    step(hipMemcpyAsync(C, d_c.p, (size_t)n * n * 8, hipMemcpyDeviceToHost, st), "download");
    step(hipStreamSynchronize(st), "synchronize");
  }
  (void)hipStreamDestroy(st);
  return rc;
}


#ifdef CAL_STAMP
int cal_debug_read_split_stamps(void* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(calk::g_split_stamps), sizeof(calk::g_split_stamps)); }
int cal_debug_read_stamps(void* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(calk::g_dense_stamps), sizeof(calk::g_dense_stamps)); }
#endif
const char* cal_last_error(void) { return g_err.c_str(); }
const char* cal_version(void) { return "calamity_hip 0.1 (gfx950)"; }

int cal_basis_foldable(int dtype, const void* block, int32_t nfreqs, int32_t nvec, int32_t nrowblk, double* max_residual, double* max_abs) {
  if (!block || nfreqs <= 0 || nvec <= 0 || nrowblk <= 0 || (dtype != CAL_F32 && dtype != CAL_F64)) return fail(CAL_ERR_INVALID, "cal_basis_foldable: bad argument");
  double resid = 0, amax = 0;
  bool ok;
  if (dtype == CAL_F32) ok = block_foldable(static_cast<const float*>(block), nfreqs, nvec, nrowblk, choose_fb<float>(nvec, nfreqs), &resid, &amax);
  else ok = block_foldable(static_cast<const double*>(block), nfreqs, nvec, nrowblk, choose_fb<double>(nvec, nfreqs), &resid, &amax);
  if (max_residual) *max_residual = resid;
  if (max_abs) *max_abs = amax;
  return ok ? 1 : 0;
}

int cal_debug_plan(int dtype, const cal_problem_desc* d, int what, void* out, int64_t cap_bytes, int64_t* bytes) {
  if (!out || !bytes || cap_bytes < 0 || (dtype != CAL_F32 && dtype != CAL_F64)) return fail(CAL_ERR_INVALID, "cal_debug_plan: bad argument");
  return dtype == CAL_F32 ? debug_plan<float>(d, what, out, cap_bytes, bytes) : debug_plan<double>(d, what, out, cap_bytes, bytes);
}

int cal_debug_solve_plan(int dtype, const cal_problem_desc* d, int64_t scratch_bytes, int what, void* out, int64_t cap_bytes, int64_t* bytes) {
  if (!out || !bytes || cap_bytes < 0 || (dtype != CAL_F32 && dtype != CAL_F64)) return fail(CAL_ERR_INVALID, "cal_debug_solve_plan: bad argument");
  if (scratch_bytes < 0) return fail(CAL_ERR_INVALID, "cal_debug_solve_plan: negative bound");
  const int64_t bound = scratch_bytes == 0 ? kCsScratchDefault : scratch_bytes;  // as in set_coeff_solve_scratch
  return dtype == CAL_F32 ? debug_solve_plan<float>(d, bound, what, out, cap_bytes, bytes) : debug_solve_plan<double>(d, bound, what, out, cap_bytes, bytes);
}

int cal_debug_delay_coherent_plan(int dtype, const cal_problem_desc* d, const cal_delay_coherent_desc* desc, int64_t scratch_bytes, int what, void* out,
                                  int64_t cap_bytes, int64_t* bytes) {
  if (!desc || !out || !bytes || cap_bytes < 0 || (dtype != CAL_F32 && dtype != CAL_F64)) return fail(CAL_ERR_INVALID, "cal_debug_delay_coherent_plan: bad argument");
  return dtype == CAL_F32 ? debug_delay_coherent_plan<float>(d, desc, scratch_bytes, what, out, cap_bytes, bytes)
                          : debug_delay_coherent_plan<double>(d, desc, scratch_bytes, what, out, cap_bytes, bytes);
}
int cal_debug_report_plan(int dtype, const cal_problem_desc* d, const cal_report_plan_desc* r, int what, void* out, int64_t cap_bytes, int64_t* bytes) {
  if (!r || !out || !bytes || cap_bytes < 0 || (dtype != CAL_F32 && dtype != CAL_F64)) return fail(CAL_ERR_INVALID, "cal_debug_report_plan: bad argument");
  return dtype == CAL_F32 ? debug_report_plan<float>(d, r, what, out, cap_bytes, bytes) : debug_report_plan<double>(d, r, what, out, cap_bytes, bytes);
}

int cal_debug_step_shape(const int32_t* inputs, int32_t* shape) {
  if (!inputs || !shape || inputs[7] < CAL_LAUNCH_AUTO || inputs[7] > CAL_LAUNCH_GRAPH) return fail(CAL_ERR_INVALID, "cal_debug_step_shape: bad argument");
  step_shape_to(plan_step(step_inputs_from(inputs)), shape);
  return CAL_OK;
}

int cal_device_count(int* count) {
  if (!count) return fail(CAL_ERR_INVALID, "cal_device_count: null");
  *count = 0;
  HIP_TRY(hipGetDeviceCount(count));
  return CAL_OK;
}

int cal_device_info(int device, char* name, size_t name_len, int64_t* total_mem_bytes, int32_t* compute_units) {
  hipDeviceProp_t p;
  HIP_TRY(hipGetDeviceProperties(&p, device));
  if (name && name_len) snprintf(name, name_len, "%s (%s)", p.name, p.gcnArchName);
  if (total_mem_bytes) *total_mem_bytes = (int64_t)p.totalGlobalMem;
  if (compute_units) *compute_units = p.multiProcessorCount;
  return CAL_OK;
}

int cal_weighted_square_error(int device, int dtype, int64_t n, const void* model_r, const void* model_i, const void* data_r, const void* data_i,
                              const void* wgts, double* out) {
  if (!model_r || !model_i || !data_r || !data_i || !wgts || !out) return fail(CAL_ERR_INVALID, "cal_weighted_square_error: null argument");
  if (n < 0) return fail(CAL_ERR_INVALID, "cal_weighted_square_error: n = %lld", (long long)n);
  *out = 0.0;
  if (n == 0) return CAL_OK;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return fail(CAL_ERR_HIP, "no usable HIP device (%s); this library has no CPU fallback", e == hipSuccess ? "0 devices" : hipGetErrorString(e));
  if (device < 0 || device >= ndev) return fail(CAL_ERR_INVALID, "cal_weighted_square_error: device %d out of range [0, %d)", device, ndev);
  HIP_TRY(hipSetDevice(device));
  const void* const src[5] = {model_r, model_i, data_r, data_i, wgts};
  if (dtype == CAL_F32) return weighted_square_error<float>(n, src, out);
  if (dtype == CAL_F64) return weighted_square_error<double>(n, src, out);
  return fail(CAL_ERR_INVALID, "cal_weighted_square_error: unknown dtype %d", dtype);
}

int cal_device_stream_peak(int device, size_t bytes, int reps, double* read_gbps, double* copy_gbps) {
  if (bytes < (64u << 20) || reps < 1) return fail(CAL_ERR_INVALID, "cal_device_stream_peak: need >= 64 MiB and >= 1 repetition");
  HIP_TRY(hipSetDevice(device));
  const size_t n = bytes / 16;  // float4 elements
  void *src = nullptr, *dst = nullptr;
  float* sink = nullptr;
  hipEvent_t e0, e1;
  HIP_TRY(hipMalloc(&src, n * 16));
  if (hipMalloc(&dst, n * 16) != hipSuccess) { (void)hipFree(src); return fail(CAL_ERR_HIP, "cal_device_stream_peak: out of device memory"); }
  HIP_TRY(hipMalloc((void**)&sink, 1 << 20));
  HIP_TRY(hipMemset(src, 0, n * 16));
  HIP_TRY(hipMemset(dst, 0, n * 16));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  hipDeviceProp_t p;
  HIP_TRY(hipGetDeviceProperties(&p, device));
  const int grid = p.multiProcessorCount * 8;
  double best_r = 0, best_c = 0;
  for (int r = 0; r < reps + 1; ++r) {  // first launch of each kernel is a warm-up
    float ms = 0;
    HIP_TRY(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(stream_read_kernel, dim3(grid), dim3(256), 0, 0, (const f4_t*)src, n, sink);
    HIP_TRY(hipEventRecord(e1, 0));
    HIP_TRY(hipEventSynchronize(e1));
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    if (r > 0) best_r = std::max(best_r, (double)(n * 16) / (ms * 1e-3) / 1e9);
    HIP_TRY(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(stream_copy_kernel, dim3(grid), dim3(256), 0, 0, (const f4_t*)src, (f4_t*)dst, n);
    HIP_TRY(hipEventRecord(e1, 0));
    HIP_TRY(hipEventSynchronize(e1));
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    if (r > 0) best_c = std::max(best_c, (double)(2 * n * 16) / (ms * 1e-3) / 1e9);
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipFree(src);
  (void)hipFree(dst);
  (void)hipFree(sink);
  if (read_gbps) *read_gbps = best_r;
  if (copy_gbps) *copy_gbps = best_c;
  return CAL_OK;
}

int cal_device_busy_clock_mhz(int device, double* mhz) {
  if (!mhz) return fail(CAL_ERR_INVALID, "cal_device_busy_clock_mhz: null");
  HIP_TRY(hipSetDevice(device));
  long long* out = nullptr;
  float* sink = nullptr;
  HIP_TRY(hipMalloc((void**)&out, 2 * sizeof(long long)));
  HIP_TRY(hipMalloc((void**)&sink, 64));
  hipDeviceProp_t p;
  HIP_TRY(hipGetDeviceProperties(&p, device));
  int wall_khz = 0;
  HIP_TRY(hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, device));
  long long h[2] = {0, 0};
  for (int rep = 0; rep < 3; ++rep) {  // the last repetition is measured at the clock the load has settled on
    hipLaunchKernelGGL(busy_clock_kernel, dim3(p.multiProcessorCount * 8), dim3(256), 0, 0, out, 400000, sink);
    HIP_TRY(hipDeviceSynchronize());
  }
  HIP_TRY(hipMemcpy(h, out, sizeof(h), hipMemcpyDeviceToHost));
  (void)hipFree(out);
  (void)hipFree(sink);
  if (h[1] <= 0 || wall_khz <= 0) return fail(CAL_ERR_HIP, "cal_device_busy_clock_mhz: no wall-clock counter");
  *mhz = (double)h[0] / ((double)h[1] / (wall_khz * 1e3)) / 1e6;
  return CAL_OK;
}

int cal_solver_create(cal_solver** out, int device, int dtype) {
  if (!out) return fail(CAL_ERR_INVALID, "cal_solver_create: null");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(CAL_ERR_HIP, "no usable HIP device (%s); this library has no CPU fallback", e == hipSuccess ? "0 devices" : hipGetErrorString(e));
  if (device < 0 || device >= n) return fail(CAL_ERR_INVALID, "cal_solver_create: device %d out of range [0, %d)", device, n);
  std::unique_ptr<cal_solver> s;
  if (dtype == CAL_F32) {
    auto* p = new SolverT<float>();
    s.reset(p);
    p->device = device;
    p->dtype = dtype;
    CAL_TRY(p->init());
  } else if (dtype == CAL_F64) {
    auto* p = new SolverT<double>();
    s.reset(p);
    p->device = device;
    p->dtype = dtype;
    CAL_TRY(p->init());
  } else {
    return fail(CAL_ERR_INVALID, "cal_solver_create: unknown dtype %d", dtype);
  }
  *out = s.release();
  return CAL_OK;
}

int cal_solver_destroy(cal_solver* s) {
  delete s;
  return CAL_OK;
}

#define NEED(s) \
  if (!(s)) return fail(CAL_ERR_INVALID, "%s: null solver handle", __func__)

int cal_solver_set_problem(cal_solver* s, const cal_problem_desc* d) { NEED(s); return s->set_problem(d); }
int cal_solver_set_data(cal_solver* s, const void* dr, const void* di, const void* w) { NEED(s); return s->set_data(dr, di, w); }
int cal_solver_set_regularization(cal_solver* s, int mode, double pr, double pi) { NEED(s); return s->set_regularization(mode, &pr, &pi, false); }
int cal_solver_set_regularization_slices(cal_solver* s, int mode, const double* pr, const double* pi) { NEED(s); return s->set_regularization(mode, pr, pi, true); }
int cal_solver_get_slice_losses(cal_solver* s, double* losses) { NEED(s); return s->get_slice_losses(losses); }
int cal_solver_set_optimizer(cal_solver* s, const cal_optimizer_desc* d) { NEED(s); return s->set_optimizer(d); }
int cal_solver_set_params(cal_solver* s, const void* g_r, const void* g_i, const void* c_r, const void* c_i) {
  NEED(s);
  return s->set_params(g_r, g_i, c_r, c_i);
}
int cal_solver_get_params(cal_solver* s, int which, void* g_r, void* g_i, void* c_r, void* c_i) {
  NEED(s);
  return s->get_params(which, g_r, g_i, c_r, c_i);
}
int cal_solver_get_moments(cal_solver* s, void* gm_r, void* gm_i, void* gv_r, void* gv_i, void* cm_r, void* cm_i, void* cv_r,
                           void* cv_i, int64_t* t) {
  NEED(s);
  return s->get_moments(gm_r, gm_i, gv_r, gv_i, cm_r, cm_i, cv_r, cv_i, t);
}
int cal_solver_set_moments(cal_solver* s, const void* gm_r, const void* gm_i, const void* gv_r, const void* gv_i, const void* cm_r,
                           const void* cm_i, const void* cv_r, const void* cv_i, int64_t t) {
  NEED(s);
  return s->set_moments(gm_r, gm_i, gv_r, gv_i, cm_r, cm_i, cv_r, cv_i, t);
}
int cal_solver_eval_loss(cal_solver* s, double* loss) { NEED(s); return s->eval(false, loss, nullptr, nullptr, nullptr, nullptr); }
int cal_solver_eval_grads(cal_solver* s, double* loss, void* gg_r, void* gg_i, void* gc_r, void* gc_i) {
  NEED(s);
  return s->eval(true, loss, gg_r, gg_i, gc_r, gc_i);
}
int cal_solver_run(cal_solver* s, const cal_run_desc* r, double* losses_out, cal_run_result* res) { NEED(s); return s->run(r, losses_out, res, false); }
int cal_solver_run_slices(cal_solver* s, const cal_run_desc* r, double* losses_out, cal_run_result* res) { NEED(s); return s->run(r, losses_out, res, true); }
int cal_solver_model(cal_solver* s, void* mr, void* mi) { NEED(s); return s->model(mr, mi, false); }
int cal_solver_data_model(cal_solver* s, void* mr, void* mi) { NEED(s); return s->model(mr, mi, true); }
int cal_solver_solve_gains(cal_solver* s, const cal_gain_solve_desc* desc) { NEED(s); return s->solve_gains(desc); }
int cal_solver_hold_slices(cal_solver* s, const uint8_t* mask) { NEED(s); return s->hold_slices(mask); }
int cal_solver_normal_product(cal_solver* s, const void* p_g_r, const void* p_g_i, const void* p_c_r, const void* p_c_i, void* out_g_r, void* out_g_i,
                              void* out_c_r, void* out_c_i) {
  NEED(s);
  return s->normal_product(p_g_r, p_g_i, p_c_r, p_c_i, out_g_r, out_g_i, out_c_r, out_c_i);
}
int cal_solver_gauss_newton_step(cal_solver* s, const cal_gauss_newton_desc* desc, cal_gauss_newton_result* results) { NEED(s); return s->gauss_newton_step(desc, results); }
int cal_solver_lbfgs(cal_solver* s, const cal_lbfgs_desc* desc, double* losses_out, cal_lbfgs_result* results) { NEED(s); return s->lbfgs(desc, losses_out, results); }
int cal_debug_lbfgs_coefficients(int32_t npairs, const double* gram, double* delta, double* slope) {
  if (npairs < 0 || npairs > kLbfgsMaxHistory) return fail(CAL_ERR_INVALID, "cal_debug_lbfgs_coefficients: npairs = %d is outside [0, %d]", npairs, kLbfgsMaxHistory);
  if (!gram || !delta || !slope) return fail(CAL_ERR_INVALID, "cal_debug_lbfgs_coefficients: null pointer");
  int idx[kLbfgsMaxBasis];
  double alpha[kLbfgsMaxHistory];
  for (int j = 0; j <= 2 * npairs; ++j) idx[j] = j;
  *slope = lbfgs_two_loop(npairs, gram, 2 * npairs + 1, idx, delta, alpha);
  return CAL_OK;
}
int cal_solver_solve_coeffs(cal_solver* s, const cal_coeff_solve_desc* desc, cal_coeff_solve_result* result) { NEED(s); return s->solve_coeffs(desc, result); }
int cal_solver_gain_basis_errors(cal_solver* s, double ridge, double* gain_var, double* y_var, double* gain_dof, cal_fit_errors_counts* counts) {
  NEED(s);
  return s->gain_basis_errors(ridge, gain_var, y_var, gain_dof, counts);
}
int cal_solver_set_coeff_solve_scratch(cal_solver* s, int64_t bytes) { NEED(s); return s->set_coeff_solve_scratch(bytes); }
int cal_solver_fit_errors(cal_solver* s, double ridge, double* coeff_var, double* model_var, double* leverage_bl, double* nsamp_bl, double* gain_var,
                          cal_fit_errors_counts* counts) {
  NEED(s);
  return s->fit_errors(ridge, coeff_var, model_var, leverage_bl, nsamp_bl, gain_var, counts);
}
int cal_solver_get_gain_coeff_moments(cal_solver* s, void* ym_r, void* ym_i, void* yv_r, void* yv_i, void* cm_r, void* cm_i, void* cv_r, void* cv_i, int64_t* t) {
  NEED(s);
  return s->get_gain_coeff_moments(ym_r, ym_i, yv_r, yv_i, cm_r, cm_i, cv_r, cv_i, t);
}
int cal_solver_solve_gain_coeffs(cal_solver* s, const cal_gain_coeff_solve_desc* desc, cal_gain_coeff_solve_result* result) { NEED(s); return s->solve_gain_coeffs(desc, result); }
int cal_solver_solve_gain_time_coeffs(cal_solver* s, const cal_gain_time_solve_desc* desc, cal_gain_time_solve_result* result) { NEED(s); return s->solve_gain_time_coeffs(desc, result); }
int cal_solver_fit_quality(cal_solver* s, const void* g_r, const void* g_i, double* chisq_ant, double* wsum_ant, double* chisq_bl, double* wsum_bl) {
  NEED(s);
  return s->fit_quality(g_r, g_i, chisq_ant, wsum_ant, chisq_bl, wsum_bl);
}
int cal_solver_delay_spectrum(cal_solver* s, const cal_delay_spectrum_desc* desc, const void* g_r, const void* g_i, double* power_bl, double* norm_bl,
                              double* power_bin, double* count_bin) {
  NEED(s);
  return s->delay_spectrum(desc, g_r, g_i, power_bl, norm_bl, power_bin, count_bin);
}
int cal_solver_set_delay_spectrum_scratch(cal_solver* s, int64_t bytes) { NEED(s); return s->set_delay_spectrum_scratch(bytes); }
int cal_solver_delay_cross_spectrum(cal_solver* s, const cal_delay_cross_desc* desc, const void* g_r, const void* g_i, double* cross_pair, double* diff_pair,
                                    double* norm_pair, double* cross_bin, double* diff_bin, double* count_bin) {
  NEED(s);
  return s->delay_cross_spectrum(desc, g_r, g_i, cross_pair, diff_pair, norm_pair, cross_bin, diff_bin, count_bin);
}
int cal_solver_delay_fringe_spectrum(cal_solver* s, const cal_delay_fringe_desc* desc, const void* g_r, const void* g_i, double* power_grp, double* norm_grp,
                                     double* power_bin, double* count_bin) {
  NEED(s);
  return s->delay_fringe_spectrum(desc, g_r, g_i, power_grp, norm_grp, power_bin, count_bin);
}
int cal_solver_delay_coherent_spectrum(cal_solver* s, const cal_delay_coherent_desc* desc, const void* g_r, const void* g_i, double* power_grp, double* norm_grp,
                                       double* power_bin, double* count_bin) {
  NEED(s);
  return s->delay_coherent_spectrum(desc, g_r, g_i, power_grp, norm_grp, power_bin, count_bin);
}
int cal_solver_delay_transfer(cal_solver* s, const cal_delay_transfer_desc* desc, const void* g_r, const void* g_i, double* absorbed_bl, double* noise_bl,
                              double* absorbed_bin, double* count_bin, cal_fit_errors_counts* counts) {
  NEED(s);
  return s->delay_transfer(desc, g_r, g_i, absorbed_bl, noise_bl, absorbed_bin, count_bin, counts);
}
int cal_solver_set_delay_transfer_scratch(cal_solver* s, int64_t bytes) { NEED(s); return s->set_delay_transfer_scratch(bytes); }
int cal_solver_fix_degeneracies(cal_solver* s, const cal_degeneracy_desc* desc, double* params, double* nsamp, double* last_step, void* out_g_r,
                                void* out_g_i, void* out_m_r, void* out_m_i) {
  NEED(s);
  return s->fix_degeneracies(desc, params, nsamp, last_step, out_g_r, out_g_i, out_m_r, out_m_i);
}
int cal_solver_robust_weights(cal_solver* s, const cal_robust_desc* desc, double* scale_bl, double* ndown_bl) { NEED(s); return s->robust_weights(desc, scale_bl, ndown_bl); }
int cal_solver_get_weights(cal_solver* s, void* out, int which) { NEED(s); return s->get_weights(out, which); }
int cal_solver_init_coeffs(cal_solver* s, const void* sr, const void* si) { NEED(s); return s->init_coeffs(sr, si); }
int cal_solver_synchronize(cal_solver* s) { NEED(s); return s->synchronize(); }
int cal_solver_set_launch_mode(cal_solver* s, int mode) { NEED(s); return s->set_launch_mode(mode); }
int cal_solver_timing_enable(cal_solver* s, int e) { NEED(s); return s->timing_enable(e); }
int cal_solver_timing_get(cal_solver* s, cal_kernel_timing* out) { NEED(s); return s->timing_get(out); }
int cal_solver_memory_bytes(cal_solver* s, int64_t* b) { NEED(s); return s->memory_bytes(b); }

int cal_comm_unique_id(void* id_out) {
  if (!id_out) return fail(CAL_ERR_INVALID, "cal_comm_unique_id: null");
  ncclUniqueId uid;
  NCCL_TRY(ncclGetUniqueId(&uid));
  memset(id_out, 0, CAL_COMM_ID_BYTES);
  memcpy(id_out, &uid, sizeof(uid));
  return CAL_OK;
}
int cal_solver_comm_init(cal_solver* s, const void* id, int rank, int nranks) { NEED(s); return s->comm_init(id, rank, nranks); }
int cal_solver_set_exchange_hook(cal_solver* s, cal_exchange_fn fn, void* ctx, int rank, int nranks) { NEED(s); return s->set_exchange_hook(fn, ctx, rank, nranks); }
int cal_solver_comm_size(cal_solver* s, int* nranks_seen) { NEED(s); return s->comm_size(nranks_seen); }
int cal_solver_set_gain_basis(cal_solver* s, const void* basis, int32_t nvec) { NEED(s); return s->set_gain_basis(basis, nvec); }
int cal_solver_set_gain_time_basis(cal_solver* s, const void* basis_t, int32_t ntimes, int32_t nvec_t) { NEED(s); return s->set_gain_time_basis(basis_t, ntimes, nvec_t); }
int cal_solver_get_gain_coeffs(cal_solver* s, int which, void* y_r, void* y_i) { NEED(s); return s->get_gain_coeffs(which, y_r, y_i); }
int cal_solver_eval_gain_coeff_grads(cal_solver* s, double* loss, void* gy_r, void* gy_i) { NEED(s); return s->eval_gain_coeff_grads(loss, gy_r, gy_i); }

}  // extern "C"
