/* calamity_hip.h -- C-ABI of the MI355X (gfx950) gain + foreground gradient-descent fitter.
 *
 * The reference (aewallwi/calamity) has no FFI: its seam is the Python function
 *   fit_gains_and_foregrounds(...)            /root/reference/calamity/calibration.py:447-738
 * whose arithmetic is issued as TensorFlow ops (fg_model/data_model/mse/mse_chunked[_sum_regularized],
 * calibration.py:1587-1656; tf.GradientTape :664-666; tf.optimizers.* apply_gradients :667).  The entry
 * points below are what a ctypes binding for that seam needs; each one cites the reference code it
 * replaces.  INTEGRATION.md shows the reference-side binding.
 *
 * Conventions
 *  - every function returns 0 on success and a negative cal_status on failure; cal_last_error() returns a
 *    thread-local message.  Nothing throws across the boundary.
 *  - all host pointers are caller-owned, C-contiguous, and are only read/written inside the call.
 *  - "real" arrays (void*) are float when the solver was created with CAL_F32 and double with CAL_F64.
 *  - the library owns every byte of device memory.  One handle is not re-entrant; distinct handles may be
 *    driven from distinct threads.
 *  - there is NO CPU fallback: without a usable HIP device cal_solver_create() fails.
 */
#ifndef CALAMITY_HIP_H
#define CALAMITY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cal_solver cal_solver;

enum cal_status {
  CAL_OK = 0,
  CAL_ERR_INVALID = -1, /* bad argument / inconsistent problem description */
  CAL_ERR_HIP = -2,     /* HIP runtime failure */
  CAL_ERR_RCCL = -3,    /* RCCL failure */
  CAL_ERR_STATE = -4,   /* call made in the wrong state (e.g. run before set_problem) */
  CAL_ERR_UNSUPPORTED = -5,
  CAL_ERR_NONFINITE = -6 /* loss became NaN/Inf; parameters are left as they were at that step */
};

enum cal_dtype { CAL_F32 = 0, CAL_F64 = 1 };                 /* dtype kwarg, calibration.py:464, :974 */
enum cal_optimizer { /* OPTIMIZERS, calibration.py:17-27: the whole table */
  CAL_OPT_ADAM = 0, CAL_OPT_ADAMAX = 1, CAL_OPT_SGD = 2, CAL_OPT_RMSPROP = 3, CAL_OPT_ADAGRAD = 4, CAL_OPT_NADAM = 5, CAL_OPT_ADADELTA = 6,
  CAL_OPT_FTRL = 7, CAL_OPT_LAMB = 8 /* tensorflow_addons.optimizers.LAMB, :26.  One trust ratio per VARIABLE (cal_problem_desc::grp_var);
                                        with a communicator attached the per-variable norms are summed over the ranks before the ratio */
};
enum cal_regularization { CAL_REG_NONE = 0, CAL_REG_SUM = 1 }; /* model_regularization, calibration.py:619-661 */
enum cal_layout {
  CAL_LAYOUT_STREAM = 0, /* every baseline owns its basis tiles in HBM (the reference's per-baseline tensor,
                            calibration.py:167-184, minus the zero padding): HBM-streaming kernel */
  CAL_LAYOUT_SHARED = 1  /* baselines alias the unique basis blocks (one per distinct delay, the operator_cache
                            of modeling.py:291-301): cache-resident basis */
};
enum cal_kernel_path {
  CAL_PATH_AUTO = 0,    /* dense kernel when the problem is eligible and large enough to fill the chip, else general */
  CAL_PATH_GENERAL = 1, /* register-direct streaming / group kernels (any dtype, layout, group shape).  STREAM layout: like
                           CAL_PATH_AUTO it reads only channels [0, nfreqs / 2) of a basis whose blocks are all mirror-symmetric
                           (cal_basis_foldable) when every fitting group has one baseline and no baseline shares tiles */
  CAL_PATH_DENSE = 2,   /* matrix-core kernel wherever the problem is eligible (SHARED layout, one baseline per fitting
                           group, basis_nvec <= 256, nfreqs > 64); CAL_ERR_UNSUPPORTED when it is not.  fp32: the split-bf16
                           kernel (six v_mfma_f32_32x32x16_bf16 per fp32 product block, four panels of a workgroup on one
                           operand image per unit of channels, read row-wise by the forward and transposed by the adjoint
                           product); fp64: v_mfma_f64_16x16x4_f64 */
  CAL_PATH_DENSE_F32 = 3, /* fp32 only: the dense kernel on v_mfma_f32_32x32x2_f32 (one panel per workgroup) that CAL_PATH_DENSE
                            ran before the split-bf16 kernel replaced it; kept for A/B measurements and as the accuracy yardstick */
  CAL_PATH_DENSE_SPLIT1 = 4, /* fp32 only: the first split-bf16 kernel (two packed operand streams through an LDS ring, coefficient
                            panels in LDS), which CAL_PATH_DENSE ran until the one-image form replaced it; kept for A/B measurements */
  CAL_PATH_GENERAL_FULL = 5 /* CAL_PATH_GENERAL that always keeps and streams the full band of every basis block: the comparator of
                               the folded form in tests and A/B measurements */
};

enum cal_launch_mode {
  CAL_LAUNCH_AUTO = 0,     /* the fastest form for the problem: large problems one launch per kernel; problems whose step is tens of
                              microseconds (no communicator, general kernels, at most 2^20 parameters) a two-launch step replayed
                              from a hipGraph, 16 steps per replay */
  CAL_LAUNCH_KERNELS = 1,  /* every kernel its own launch at every problem size (per-antenna reduction, loop bookkeeping, regulariser
                              fold, update: finalize_kernel + adam2_kernel, never the fused step_update_kernel / step_tail_kernel) */
  CAL_LAUNCH_ONE_TAIL = 2, /* small problems: fused pass + ONE tail launch per step, launched one by one (no graph) */
  CAL_LAUNCH_GRAPH = 3     /* as AUTO where the two-launch step applies */
};

/* Ragged description of one fit (replaces the zero-padded chunk tensors built by
 * tensorize_fg_model_comps_dict / tensorize_data, calibration.py:104-310).
 * A fitting group g shares ONE coefficient vector of basis_nvec[grp_basis[g]] complex numbers; its baselines are
 * bl in [grp_bl_start[g], grp_bl_start[g+1]).  Basis block u is row-major
 * [basis_nrowblk[u] * nfreqs][basis_nvec[u]] starting at basis_data + basis_offset[u] elements
 * ("Nfreqs x Ncomponents", modeling.py:288-289); baseline bl uses rows
 * [bl_rowblk[bl] * nfreqs, (bl_rowblk[bl] + 1) * nfreqs).  Consecutive baselines of a group with the same row block
 * (a redundant set, use_redundancy=True) share one forward / adjoint product on the device.
 * Limits: basis_nvec <= 896 (CAL_ERR_UNSUPPORTED beyond); all index arrays are validated (CAL_ERR_INVALID).
 * Device rows are padded to a multiple of min(128, next_pow2(nfreqs)) channels: a function of nfreqs alone, so every
 * rank of a sharded fit uses the same gain layout and all-reduce count. */
typedef struct cal_problem_desc {
  int32_t nants;
  int32_t nfreqs;
  int32_t ngrps;
  int32_t nbls;
  int32_t nbasis;
  const int64_t* basis_offset;   /* [nbasis + 1] */
  const int32_t* basis_nvec;     /* [nbasis] */
  const int32_t* basis_nrowblk;  /* [nbasis] */
  const void* basis_data;        /* real */
  const int32_t* grp_basis;      /* [ngrps] */
  const int32_t* grp_bl_start;   /* [ngrps + 1] */
  const int32_t* bl_ant0;        /* [nbls]  corr_inds[..][..][bl][0], calibration.py:176-177 */
  const int32_t* bl_ant1;        /* [nbls] */
  const int32_t* bl_rowblk;      /* [nbls] */
  int32_t layout;                /* cal_layout */
  int32_t kernel_path;           /* cal_kernel_path; with a communicator attached the ranks agree on one path */
  const int32_t* bl_alias;       /* [nbls] or NULL.  STREAM layout: baseline b reads the basis tiles of baseline bl_alias[b] (which
                                    owns its tiles: bl_alias of it is -1 or itself) instead of holding a copy -- the same physical
                                    baseline in the time slices one solver fits together (calibration.py:1160-1167 fits them one after
                                    another).  Both must be single-baseline groups on the same basis rows.  Such baselines are
                                    processed together: their tiles are read ONCE per pass for all of them. */
  int32_t nslices;               /* 0 or 1: one fit.  T > 1: the solver holds T independent fits -- the (polarization, time) slices that
                                    calibrate_and_model_tensor fits one after another (calibration.py:1160-1167) -- over the same kind of
                                    array: nants = T * (antennas of one slice), slice t owns antennas [t nants / T, (t + 1) nants / T), a
                                    baseline's two antennas and all baselines of a fitting group lie in ONE slice, groups are listed slice
                                    by slice, every slice has at least one group; T <= CAL_MAX_SLICES.  Each slice keeps its own loss,
                                    regulariser sums and priors, tolerance stop, use_min snapshot and optimizer iteration count
                                    (cal_solver_run_slices); a stopped slice's parameters freeze while the others go on. */
  int32_t reserved;
  const int32_t* grp_var;        /* [ngrps] or NULL: which optimizer VARIABLE a group's coefficients belong to -- the chunk of the reference's
                                    fg_r[chunk] / fg_i[chunk] tensors (calibration.py:596-603).  Only a layer-wise optimizer (LAMB: one trust
                                    ratio per variable) looks at it; groups of a variable are contiguous inside a time slice.  NULL: the
                                    coefficients of a slice are one variable per component. */
} cal_problem_desc;
#define CAL_MAX_SLICES 256

typedef struct cal_optimizer_desc { /* **opt_kwargs -> tf.optimizers.X(...), calibration.py:571; semantics: Keras OptimizerV2
                                     * (TensorFlow 2.4 - 2.10), formulae in fit_kernels.hpp: optimizer_step */
  int32_t optimizer;              /* cal_optimizer */
  double learning_rate;           /* Keras defaults: 1e-3 (SGD: 1e-2) */
  double beta_1;                  /* Adam, Adamax, Nadam: 0.9 */
  double beta_2;                  /* 0.999 */
  double epsilon;                 /* 1e-7 */
  double rho;                     /* RMSprop 0.9, Adadelta 0.95 */
  double momentum;                /* SGD, RMSprop: 0 */
  double initial_accumulator_value; /* Adagrad: 0.1 */
  int32_t nesterov;               /* SGD */
  int32_t reserved;
  /* Ftrl (initial_accumulator_value above: 0.1) */
  double learning_rate_power;                  /* -0.5 */
  double l1_regularization_strength;           /* 0 */
  double l2_regularization_strength;           /* 0 */
  double l2_shrinkage_regularization_strength; /* 0 */
  double beta;                                 /* 0 */
  double weight_decay_rate;                    /* LAMB: 0 (epsilon defaults to 1e-6 there) */
} cal_optimizer_desc;

typedef struct cal_run_desc { /* loop controls of fit_gains_and_foregrounds, calibration.py:457-461 */
  int32_t nsteps;           /* number of train steps to issue at most */
  int32_t record;           /* 0: unrecorded updates (profile steps :681-687 and the "graph build" step :693);
                               1: recorded steps of the main loop :699-717 */
  int32_t use_min;          /* :702-710 */
  int32_t freeze_model;     /* :598-603 */
  double tol;               /* :712 (only consulted when record != 0) */
} cal_run_desc;

typedef struct cal_run_result {
  int32_t nrecorded; /* losses written to losses_out by this call */
  int32_t stopped;   /* 1 if the tolerance test ended the loop */
  int32_t nupdates;  /* optimizer updates applied by this call */
  int32_t nonfinite; /* 1 if the loss became NaN/Inf (the call then returns CAL_ERR_NONFINITE) */
} cal_run_result;

typedef struct cal_kernel_timing { /* HIP-event timing of the dominant kernel of a pass: the fused basis-streaming kernel or the dense kernel (bench.py roofline) */
  int64_t launches;
  double total_ms;
  double algorithmic_bytes_per_launch; /* SURVEY.md 8(d) B_step figure restated for this problem */
  double basis_bytes_per_launch;
  double flops_per_launch;             /* 8 F sum nvec: forward A c and adjoint A^T gbar_v, complex x real (12: the dense path's
                                          regularised step times its loss-only pass too) */
  int32_t kernel_path;                 /* CAL_PATH_GENERAL or CAL_PATH_DENSE: the family the timed launches belong to */
  int32_t dense_wg_per_cu;             /* dense path: workgroups per CU its LDS footprint allows (2 is what the kernels are tuned for) */
  int32_t basis_folded;                /* 1: the streaming kernel reads half the band of a mirror-symmetric basis (cal_basis_foldable); the
                                          byte and flop figures above count what that pass reads and multiplies */
  int32_t reserved;
} cal_kernel_timing;

const char* cal_last_error(void);
const char* cal_version(void);
int cal_device_count(int* count);
/* Host only (no device is touched).  Whether the streaming kernel may keep just channels [0, nfreqs / 2) of the basis block
 * `block` (row-major [nrowblk * nfreqs][nvec], dtype CAL_F32 / CAL_F64): one row block, nfreqs even, nfreqs / 2 a whole number of
 * the block's channel tiles, and mirror symmetry with alternating sign in the block's own vector order,
 * A[nfreqs-1-f][k] = (-1)^k A[f][k] -- what modeling.dpss_windows delivers.  CAL_F32: no element may differ from its mirror partner by
 * more than half a unit in the last place of the block's largest element (the trace of the cast from fp64); CAL_F64: the two
 * halves agree exactly.  Returns 1 / 0, or a negative cal_status.  max_residual, max_abs (either may be NULL): the largest
 * |A[nfreqs-1-f][k] - (-1)^k A[f][k]| and the largest |A| of the block (zeros where the shape already rules folding out). */
int cal_basis_foldable(int dtype, const void* block, int32_t nfreqs, int32_t nvec, int32_t nrowblk, double* max_residual, double* max_abs);
/* Host only (no device is touched): runs the planner of cal_solver_set_problem on `d` for a solver of `dtype` and copies plan array `what`
 * to `out` as raw bytes (*bytes of them; CAL_ERR_INVALID if cap_bytes is too small).  Returns the planner's cal_status -- the code and
 * message cal_solver_set_problem would give -- when the problem is refused.  For tests (tests/test_plan_host.py).
 * what = 0: 31 scalars, 8 bytes each, int64 except [11]: fpad, ncoef, nslices, na_slice, fold, small_loads, nitems, nitems_simple, nitems_plain,
 *   gc_direct, gcp_len, basis_bytes (double), steps_per_sync, the dynamic LDS of fused_basis / fused_group / fused_multi / fused_multi_mfma, mf_ok,
 *   mf_split, mf_split2, mf_npanels, mf_grid, the dense launch's LDS (gradient, loss), nheads, nheads_mfma, heads_one_pass_local, mm_grid, lamb_ok,
 *   lamb_nvar, lamb_ncvar.
 * 1 fb (int32 per basis block), 2 tile offsets of the blocks (int64), 3 bl_tile (int64), 4 copy jobs (3 int64 each), 5 grp_coff, 6 slice_coff,
 * 7 slice_cblk, 8 LAMB variables (LambVar), 9 / 10 / 11 the coefficient variables' first coefficients, slices and grp_var ids, 12 runs (int2),
 * 13 items in launch order (Item), 14 item_goff, 15 grp_item_ptr, 16 coef_grp (empty when every group is one item), 17 / 18 and 19 / 20 the slices'
 * loss-partial index (ptr, idx) over items and over panels (empty with one slice), 21 members (Member), 22 heads, 23 panels (PanelItem),
 * 24 the panel map, 25 byte offsets of the blocks' packed operands, 26 CsGroup per group, 27 / 28 the antenna CSR (ptr; int2 entries).
 * Records are the structs of the kernel headers; int32 where nothing else is said. */
int cal_debug_plan(int dtype, const cal_problem_desc* d, int what, void* out, int64_t cap_bytes, int64_t* bytes);
/* Host only, like cal_debug_plan: what the closed-form calls plan at their first call (csrc/solve_plan.hpp) for the problem `d`, a solver of
 * `dtype` and the bound of cal_solver_set_coeff_solve_scratch (0: the default; negative: CAL_ERR_INVALID).  For tests
 * (tests/test_solve_plan_host.py).  what = 0 .. 6: the plan of cal_solver_solve_coeffs, 10 .. 16: of cal_solver_fit_errors --
 *   + 0: int64 n_max, d_max, x_max (elements of the N, factor and W scratch), npieces, number of chunks; + 1: CsGroup per group with the
 *   plan's offsets; + 2: order; + 3: Gram work (CsWork); + 4: chunks (int32 g0, g1, w0, w1, l0, l1, then the dynamic LDS as int64);
 *   + 5: W offsets (int64 per group); + 6: leverage work (FeWork).  The last two and npieces are empty / 0 for solve_coeffs.
 * 20 / 21: the antenna lists without autocorrelations (ptr; int2 entries).
 * 30: the row chunks of cal_solver_solve_gain_coeffs (L = 0) and cal_solver_solve_gain_time_coeffs.  On entry `out` holds int64 K, L, T
 *   (vectors of the frequency basis, of the time basis, times; nants must be a multiple of T); on return int64 rows per chunk, in_lds,
 *   the Cholesky launch's LDS bytes, unknowns per row, elements per row of M and N (dtype) and of the double scratch.
 * 31: the row chunks of cal_solver_gain_basis_errors, in and out as 30 plus an eighth number: elements per row of W (dtype). */
int cal_debug_solve_plan(int dtype, const cal_problem_desc* d, int64_t scratch_bytes, int what, void* out, int64_t cap_bytes, int64_t* bytes);
/* Host only, like cal_debug_plan: what cal_solver_delay_spectrum and cal_solver_fix_degeneracies plan before they launch
 * (csrc/report_plan.hpp) for the problem `d` and a solver of `dtype`.  For tests (tests/test_report_plan_host.py).  The call is described
 * by `r` (NULL: CAL_ERR_INVALID); the planner's own refusals come back with the code and message the solver's call would give.
 * what = 0 .. 4: the plan of cal_solver_delay_spectrum for r->spectrum (ndelays, what, nbins, bin_of_bl, op_r, op_i, norm_f are read; the
 *   operator in `dtype`), the bound r->scratch_bytes of cal_solver_set_delay_spectrum_scratch (0: the default) and with_power_bl (power_bl
 *   is asked for; bins ask for the power anyway) --
 *   0: int64 nwhat, the row pitch of the masked planes, the columns of the operator image, rows per chunk, chunks, the elements of the
 *   chunk's planes (dtype), of its power (double) and of norm_bl | power_bin | count_bin; 1: the bins' sorted row lists, one after the
 *   other; 2: [chunks][nbins][2] a bin's piece of a chunk as positions in 1; 3: the operator image [re, im][pitch][columns] (dtype);
 *   4: norm_f padded to the pitch (double).
 * what = 10 .. 19: the plan of cal_solver_fix_degeneracies for r->degeneracy (mode, antpos and, for CAL_DEGEN_BAND, freqs are read) over
 *   r->nslices slices (0: the problem's nslices; the ntimes of a joint time-basis layout otherwise: it must divide nants) --
 *   10: int64 segments, then the first double of antpos, ratio and maxd in blob 18 and the first int of 16 and 17 in blob 19;
 *   11: d_b [nbls][2]; 12: antpos; 13: nu_f / nu_ref [fpad]; 14: the slices' longest |d_b| (11 .. 14 double); 15: the slices' row lists,
 *   one after the other; 16: a slice's first segment [slices + 1]; 17: the segments (DgSeg); 18 / 19: the two blobs as the device holds
 *   them, 11 | 12 | 13 | 14 (double) and 15 | 16 | 17 (int32).
 * what = 40 .. 48: the plan of cal_solver_delay_transfer for r->transfer (ndelays, nbins, bin_of_bl, op_r, op_i are read) and the bound
 *   r->scratch_bytes of cal_solver_set_delay_transfer_scratch (0: the default) --
 *   40: int64 the row pitch of S, the columns of the operator image, the 64-channel pieces of the band, the elements of the chunk's N
 *   (dtype), factor (double) and W | S (dtype) scratch, chunks, runs, rows, the elements of absorbed_bl and of valid | absorbed_bin |
 *   count_bin; 41: CsGroup per group with the plan's offsets; 42: order; 43: chunks (int32 g0, g1, w0, w1, r0, r1, q0, q1 -- positions
 *   in 42, in the Gram work, in 45 and in 46 -- then the dynamic LDS as int64); 44: int64 per group, the offset of its W in the third
 *   scratch (S of its runs follows); 45: runs (int64 offset of S, int32 group, b0, b1, 0); 46: rows (int64 offset of S, int32 row,
 *   group); 47: the bins' sorted row lists; 48: [nbins][2] a bin's list as positions in 47.
 * what = 60 .. 65: the plan of cal_solver_delay_cross_spectrum for r->cross (every field is read; the operator in `dtype`) and the bound
 *   r->scratch_bytes of cal_solver_set_delay_spectrum_scratch (0: the default) --
 *   60: int64 nwhat, nstat, the row pitch of the masked planes, the columns of the operator image, pairs per chunk, chunks, the elements
 *   of the chunk's planes (dtype), of its statistics (double) and of norm_pair | cross_bin | diff_bin | count_bin; 61: the bins' sorted
 *   pair lists, one after the other; 62: [chunks][nbins][2] a bin's piece of a chunk as positions in 61; 63: the operator image
 *   [re, im][pitch][columns] (dtype); 64: norm_f padded to the pitch (double); 65: the scales [npairs][2] (double; ones for NULL).
 * what = 70 .. 76: the plan of cal_solver_delay_fringe_spectrum for r->fringe (every field is read; the operator in `dtype`) and the
 *   bound r->scratch_bytes of cal_solver_set_delay_spectrum_scratch (0: the default) --
 *   70: int64 nwhat, the row pitch of the masked planes, the columns of the operator image, groups per chunk, chunks, the elements of
 *   the chunk's planes (dtype), of its Y and power (double) and of norm_grp | power_bin | count_bin; 71: the bins' sorted group lists,
 *   one after the other; 72: [chunks][nbins][2] a bin's piece of a chunk as positions in 71; 73: the operator image
 *   [re, im][pitch][columns] (dtype); 74: norm_f padded to the pitch (double); 75: the scales [ngroups][ntimes] (double; ones for NULL);
 *   76: opt_r | opt_i, [ntimes][nrates] each (double). */
typedef struct cal_report_plan_desc {
  const struct cal_delay_spectrum_desc* spectrum;
  const struct cal_degeneracy_desc* degeneracy;
  int64_t scratch_bytes;
  int32_t with_power_bl;
  int32_t nslices;
  const struct cal_delay_transfer_desc* transfer; /* what = 40 .. 48 only */
  const struct cal_delay_cross_desc* cross;       /* what = 60 .. 65 only */
  const struct cal_delay_fringe_desc* fringe;     /* what = 70 .. 76 only */
} cal_report_plan_desc;
int cal_debug_report_plan(int dtype, const cal_problem_desc* d, const cal_report_plan_desc* r, int what, void* out, int64_t cap_bytes, int64_t* bytes);
/* Host only, like cal_debug_plan: the shape of one pass or train step (csrc/step_plan.hpp) -- which kernels follow the fused or dense pass,
 * the form of the update, whether a run replays its steps from a graph.  For tests (tests/test_step_plan_host.py).
 * inputs, 14 int32 (flags 0 / 1 but [7]): the dense path serves the pass, the regulariser is "sum", the regularised gradient pass needs the
 *   loss pre-pass, every group is one item (gc_direct), a communicator or exchange hook is set, a gain basis is set, 2 nants fpad + 2 ncoef
 *   <= 2^20, [7] the cal_launch_mode, the optimizer is LAMB, the pass is asked for gradients, for the update, for the projection on the gain
 *   basis, kernel timing is on, the run has at least 256 steps.  Every combination has a shape (CAL_ERR_INVALID: a null, an unknown mode).
 * shape, 13 int32: the general kernels' two-adjoint-set regulariser, the dense two-pass form, the general alpha pre-pass, step_tail_kernel
 *   behind the pass, step_update_kernel, coeff_partial_reduce_kernel runs, finalize_kernel runs, gain-gradient planes (1 or 3), the planes
 *   are projected, the update (0 none, 1 tail, 2 fused, 3 LAMB, 4 adam2), the gains are expanded from y afterwards, the steps are replayed
 *   from a graph, the pass leaves per-item partials of the coefficient gradient. */
int cal_debug_step_shape(const int32_t* inputs, int32_t* shape);
int cal_device_info(int device, char* name, size_t name_len, int64_t* total_mem_bytes, int32_t* compute_units);
/* Measured streaming peaks of the device (no reference counterpart; BASELINE.md section 3 asks for the roofline against a
 * stream kernel measured on the box next to the nominal 8 TB/s): a read-only sweep (16-byte non-temporal loads, the
 * access pattern of the fit's tile stream) and a copy, each over `bytes` of HBM, best of `reps` launches, in GB/s. */
int cal_device_stream_peak(int device, size_t bytes, int reps, double* read_gbps, double* copy_gbps);
/* Shader clock the device sustains while every CU is busy with vector FMAs for a few milliseconds (MHz): boxes of the
 * same model differ in the clock they hold under load, and compute-side kernel times scale with it. */
int cal_device_busy_clock_mhz(int device, double* mhz);
/* mse, calibration.py:1608-1609, on its own: sum over n samples of w ((d_r - m_r)^2 + (d_i - m_i)^2) for five host arrays of n
 * reals of type dtype (CAL_F32 / CAL_F64), evaluated on `device` (products in dtype as the reference's graph does, partial sums
 * in double, fixed order).  The fit itself never materialises a model: this is the reference's building block under its own name. */
int cal_weighted_square_error(int device, int dtype, int64_t n, const void* model_r, const void* model_i, const void* data_r,
                              const void* data_i, const void* wgts, double* out);

/* The joint-covariance modeling vectors of fitting groups, simple_cov.py:7-189 (the reference's use_tensorflow=True path), without the
 * dense eigenproblem (csrc/mixed_comps_kernels.hpp).  Per group of Nbls baselines, n = Nbls nfreqs samples, baseline-major:
 *   C[(a,i)][(b,j)] = sinc(2 max(min_dly dnu, horizon |u_a(nu_i) - u_b(nu_j)| + offset dnu)) sinc(2 ant_dly dnu), u = uvw nu / 3e8, dnu in GHz;
 *   diagonally pivoted Cholesky C ~ L L^T (argmax of the running diagonal, ties to the lowest index), stopped when the largest
 *   remaining diagonal is below tol (status 0, "ok") or at the group's rank cap (status 1); G = L^T L [k][k]; the certificate
 *   resid_fro = ||C - L L^T||_F over the whole matrix.  The caller takes the eigenpairs of G (lambda, U) and asks for
 *   V = L U diag(scale), scale = lambda^-1/2: orthonormal eigenvectors of L L^T.  All of it in double, on `device`; all sums in a
 *   fixed order.
 * Groups are factored in chunks of consecutive groups whose scratch fits scratch_bytes (0: 256 MiB; negative: CAL_ERR_INVALID).  A
 * group asks for min(n, 6144, max(64, ceil(n / 3))) columns; one that does not fit the bound even alone gets the columns the bound holds
 * (in sixteens) as its rank cap, and status 2 ("not run", rank 0) when that is none.  The factors (n rounded up to 64, times the rank
 * rounded up to 16, doubles per group) stay on the device until the handle is destroyed. */
typedef struct cal_mixed_comps_desc {
  int32_t ngroups;
  int32_t nfreqs;
  const int32_t* grp_bl_start; /* [ngroups + 1]: the baselines of group g are rows [grp_bl_start[g], grp_bl_start[g + 1]) of uvw */
  const double* uvw;           /* [grp_bl_start[ngroups]][3] metres */
  const double* freqs;         /* [nfreqs] Hz */
  const int32_t* grp_freq_start; /* NULL: every group has all nfreqs channels; else [ngroups + 1]: group g has channels
                                    [grp_freq_start[g], grp_freq_start[g + 1]) of freqs (groups of different bands in one call) */
  double ant_dly, horizon, offset, min_dly;
  double tol;                  /* > 0 */
  int64_t scratch_bytes;
} cal_mixed_comps_desc;
typedef struct cal_mixed_comps cal_mixed_comps;
/* Factors every group, forms every G and every certificate; CAL_ERR_HIP without a device (there is no CPU fallback). */
int cal_mixed_comps_create(cal_mixed_comps** out, int device, const cal_mixed_comps_desc* desc);
int cal_mixed_comps_destroy(cal_mixed_comps* h);
/* Per group (any pointer may be NULL): rank k, status, the chunk it was factored in (0, 1, ... in group order), the largest running
 * diagonal at the end, resid_fro; times_ms [3]: the factorisations, the Gram launch and the certificate launches of the create call
 * (HIP events). */
int cal_mixed_comps_info(cal_mixed_comps* h, int32_t* rank, int32_t* status, int32_t* chunk, double* max_d, double* resid_fro, double* times_ms);
/* G of every group, one after the other ([k][k] each, symmetric, both triangles), sum k^2 <= cap_doubles doubles. */
int cal_mixed_comps_gram(cal_mixed_comps* h, double* G, int64_t cap_doubles);
/* V = L U diag(scale) of every group in one upload, one launch, one download: nkeep [ngroups] (0: the group is skipped), U the
 * groups' [k][nkeep] one after the other, scale their [nkeep], V their [n][nkeep] in dtype (CAL_F32 / CAL_F64).  ms (may be NULL): the launch. */
int cal_mixed_comps_vectors(cal_mixed_comps* h, int dtype, const int32_t* nkeep, const double* U, const double* scale, void* V, double* ms);
/* For tests: L of one group as [k][n] (column m of L is row m) and its k pivots (either may be NULL). */
int cal_mixed_comps_factor(cal_mixed_comps* h, int32_t group, double* L, int32_t* pivots);
/* The dense C [n][n] of one group, n = nbls nfreqs <= 46340, by the same element function. */
int cal_simple_cov_matrix(int device, int32_t nbls, const double* uvw, int32_t nfreqs, const double* freqs, double ant_dly, double horizon,
                          double offset, double min_dly, double* C);

/* tf.device / GPU selection of read_calibrate_and_model_dpss, calibration.py:1741-1753, :1796-1804 */
int cal_solver_create(cal_solver** out, int device, int dtype);
int cal_solver_destroy(cal_solver* s);

/* tensorize_fg_model_comps_dict, calibration.py:104-190 (called once per dataset, :1143-1152) */
int cal_solver_set_problem(cal_solver* s, const cal_problem_desc* desc);
/* tensorize_data, calibration.py:193-310 (per pol/time): [nbls][nfreqs] real each; weights already normalised */
int cal_solver_set_data(cal_solver* s, const void* data_r, const void* data_i, const void* wgts);
/* model_regularization="sum": priors of calibration.py:619-625; mode = cal_regularization */
int cal_solver_set_regularization(cal_solver* s, int mode, double prior_r_sum, double prior_i_sum);
/* the same with one pair of priors per time slice (cal_problem_desc::nslices): prior_*_sum [nslices] */
int cal_solver_set_regularization_slices(cal_solver* s, int mode, const double* prior_r_sum, const double* prior_i_sum);
int cal_solver_set_optimizer(cal_solver* s, const cal_optimizer_desc* desc); /* also zeroes moments and t */

/* tf.Variable(g_r), ... calibration.py:596-603.  gains [nants][nfreqs]; coefficients flat in group order,
 * sum_g nvec_g reals each.  Any pointer may be NULL to leave that array untouched. */
int cal_solver_set_params(cal_solver* s, const void* g_r, const void* g_i, const void* c_r, const void* c_i);
/* .value() snapshots, calibration.py:706-710, :724-728.  which = 0: current parameters; 1: use_min snapshot */
int cal_solver_get_params(cal_solver* s, int which, void* g_r, void* g_i, void* c_r, void* c_i);
/* optimizer slots (checkpoint / resume; no counterpart in the reference): m and v (Adam) / u (Adamax).  A fit resumed with
 * set_params + set_moments (after set_optimizer, whose betas the bias corrections are rebuilt from) continues bit for bit.
 * The two slots per parameter, (m, v): Adam / Nadam first and second moment; Adamax (m, u); SGD (momentum accumulator, unused);
 * RMSprop (momentum accumulator, mean square); Adagrad (unused, accumulator); Adadelta (accumulated updates, accumulated gradients);
 * Ftrl (linear, accumulator); LAMB (first, second moment).  Several time slices (cal_problem_desc::nslices): t is the count every
 * slice shares; get_moments fails with CAL_ERR_STATE when the slices have applied different numbers of updates (they stop on their own). */
int cal_solver_get_moments(cal_solver* s, void* gm_r, void* gm_i, void* gv_r, void* gv_i, void* cm_r, void* cm_i,
                           void* cv_r, void* cv_i, int64_t* t);
int cal_solver_set_moments(cal_solver* s, const void* gm_r, const void* gm_i, const void* gv_r, const void* gv_i,
                           const void* cm_r, const void* cm_i, const void* cv_r, const void* cv_i, int64_t t);

/* loss_function() alone: mse_chunked / mse_chunked_sum_regularized, calibration.py:1612-1656 */
int cal_solver_eval_loss(cal_solver* s, double* loss); /* several time slices: the sum of their losses */
/* the loss of every time slice as of the last cal_solver_eval_loss / cal_solver_eval_grads: losses [nslices] */
int cal_solver_get_slice_losses(cal_solver* s, double* losses);
/* tape.gradient(loss, vars), calibration.py:664-666, without the update (parity tests) */
int cal_solver_eval_grads(cal_solver* s, double* loss, void* gg_r, void* gg_i, void* gc_r, void* gc_i);
/* train_step() x nsteps with the loop semantics of calibration.py:681-717; losses_out: [nsteps] doubles or NULL */
int cal_solver_run(cal_solver* s, const cal_run_desc* run, double* losses_out, cal_run_result* result);
/* The same loop for every time slice of the solver at once (cal_problem_desc::nslices; the time loop of calibration.py:1160-1167,
 * :1244-1269 as ONE batch): each train step advances every slice that has not stopped; slice t records its own losses
 * (losses_out [nslices][run->nsteps], row t holds results[t].nrecorded values), applies the tolerance test of :712-717 and the
 * use_min bookkeeping of :702-710 to ITS loss, and stops on its own -- its gains and coefficients then stay as they are.
 * cal_solver_get_params(which = 1) holds every slice's own minimum.  results: [nslices].  A non-finite loss stops that slice
 * only; the call then returns CAL_ERR_NONFINITE after the other slices have finished (results[t].nonfinite tells which). */
int cal_solver_run_slices(cal_solver* s, const cal_run_desc* run, double* losses_out, cal_run_result* results);
/* yield_fg_model_array, calibration.py:402-444, per baseline instead of a nants x nants cube: [nbls][nfreqs] */
int cal_solver_model(cal_solver* s, void* model_r, void* model_i);
/* data_model, calibration.py:1593-1605: the foreground model of every baseline times its antennas' current gains,
 * g_ant0 conj(g_ant1) (A c): [nbls][nfreqs] (gains and coefficients must be set) */
int cal_solver_data_model(cal_solver* s, void* model_r, void* model_i);
/* Where the residual power of the fit sits (no counterpart in the reference, which reports one loss per slice and fills the gain
 * object's quality_array with zeros, cal_utils.py:48): mse, calibration.py:1608-1609, kept per baseline and per (antenna, channel)
 * instead of summed to one number.  In solver units, for baseline b with antennas (i, j) and channel f:
 *   w = the weights of cal_solver_set_data, m = A c with the current coefficients, g = the gains the quality is evaluated at,
 *   e[b][f] = w[b][f] |d[b][f] - g_i[f] conj(g_j[f]) m[b][f]|^2
 *   chisq_bl[b] = sum_f e[b][f],  wsum_bl[b] = sum_f w[b][f]                                       [nbls]
 *   chisq_ant[a][f] = sum over the baselines b that hold a of e[b][f],  wsum_ant[a][f] likewise of w   [nants][nfreqs]
 * An autocorrelation baseline (ant0 == ant1) counts ONCE for its antenna.  sum_b chisq_bl is the unregularised loss; without
 * autocorrelations sum_a chisq_ant[a][f] = 2 sum_b e[b][f].  All four outputs are double for both dtypes: products are formed in
 * the solver's dtype as the loss kernels form them, sums are taken in double in a fixed order (no float atomics): two calls give
 * the same bits.  Any output pointer may be NULL.
 *   g_r, g_i: [nants][nfreqs] real (solver dtype), or both NULL.  NULL: the solver's current full gains (the expanded g, whatever
 *   gain bases are set).  Given: uploaded to a buffer of their own and used for this evaluation only -- the solver's gains, g0, y,
 *   moments and t are not touched.
 * Problem, data and coefficients must be set, gains set or given (CAL_ERR_STATE otherwise).  Works for every layout and kernel
 * path, fitting groups of several baselines, bl_alias, nslices > 1 and the joint time-basis layout (antenna row t Na + a is simply
 * a row; slices that have stopped are evaluated like the others).  It runs the model pass of cal_solver_model and leaves everything
 * a later cal_solver_run reads as it found it: a run continued after this call is bit-identical to one without it.
 * Under a communicator or exchange hook chisq_ant | wsum_ant are summed over the ranks in ONE all-reduce of 2 nants nfreqs doubles
 * (CAL_XCHG_F64, CAL_XCHG_SUM), whichever outputs are asked for: every rank returns identical planes.  chisq_bl and wsum_bl stay
 * the rank's own baselines. */
int cal_solver_fit_quality(cal_solver* s, const void* g_r, const void* g_i, double* chisq_ant, double* wsum_ant, double* chisq_bl,
                           double* wsum_bl);
/* Downweight outliers from the residual (no counterpart in the reference, which minimises a plain weighted chi-square): one round of
 * iteratively reweighted least squares.  The call rewrites the ONE weight plane that every kernel path, cal_solver_fit_quality, the
 * closed-form solves and the six post-fit reports (cal_solver_fit_errors, cal_solver_gain_basis_errors, cal_solver_delay_spectrum,
 * cal_solver_delay_cross_spectrum, cal_solver_delay_transfer, and cal_solver_fix_degeneracies where its ref_w is NULL: given reference weights replace the plane, which
 * is then not read) read, in place: no fit kernel changes and no recorded step graph goes stale.  With w0 the weights as
 * cal_solver_set_data gave them, (i, j) the antennas of baseline row b, m = A c at the solver's coefficients, g the solver's gains:
 *   e[b][f]  = w0[b][f] |d[b][f] - g_i[f] conj(g_j[f]) m[b][f]|^2     (products in the solver's dtype, in cal_solver_fit_quality's order)
 *   S_b      = { f < nfreqs : w0[b][f] > 0 },  n_b = |S_b|
 *   med_b    = the ((n_b + 1) // 2)-th smallest of e[b][S_b]          (the lower median: an element of the row, never an average)
 *   scale_b  = med_b / ln 2
 *   z2       = e / scale_b                                            (scale_b, z2 and psi in double)
 *   huber  : psi = 1 if z2 <= k^2 else k / sqrt(z2)
 *   cauchy : psi = 1 / (1 + z2 / k^2)
 *   clip   : psi = 1 if z2 <= k^2 else 0
 *   w[b][f]  = w0[b][f] * psi                                         (rounded once to the solver's dtype)
 * scale_b = med_b / ln 2 because w |r|^2 of complex Gaussian residuals is exponentially distributed, whose median is ln 2 times its
 * mean; k = threshold is in sigma (for that law P(z2 > 9) = e^-9 ~ 1.2e-4).  Rows with n_b = 0 or med_b = 0 keep w = w0 and report
 * scale 0; autocorrelation rows are rows like any other; channels outside S_b and the padding keep their bits.  The scale is per
 * baseline row: nothing leaves the row, so a sharded fit issues NO collective under a communicator or exchange hook.  Every call starts
 * from w0, never from the previous w; the weights are not renormalised, so losses before and after a call are under different weights
 * and are not comparable.  The median is exact (a bisection on the IEEE bit pattern of e, integer counts): two calls give the same bits.
 * Non-finite samples of S_b (w0 > 0, data not finite) take what the lines above give literally.  A NaN in e orders above every number,
 * +inf included: a row in which fewer than n_b - (n_b + 1) // 2 + 1 samples are NaN has a number for its median, and a row whose
 * median is a NaN (or zero) keeps w = w0 and reports scale 0, count 0.  Behind a finite scale a NaN sample has z2 = NaN, for which both
 * comparisons are false: psi is NaN under HUBER and CAUCHY (the weight becomes NaN and the sample is not counted in ndown_bl) and 0
 * under CLIP (weight w0 * 0 = 0; counted, so under CLIP ndown_bl stays the number of weights the call set to zero).  An infinite
 * sample has psi = 0 under all three kinds and is counted.  The finite samples of such a row are weighted as in any other row.
 *   kind: CAL_ROBUST_NONE copies w0 back for the selected slices (and frees nothing); HUBER, CAUCHY, CLIP as above; anything else, or a
 *   threshold that is not finite and > 0, is CAL_ERR_INVALID.  Problem, data, coefficients and gains must be set (CAL_ERR_STATE).
 *   slice_mask: [nslices] bytes or NULL (all slices): the rows of a slice whose byte is 0 (slice of a row = its first antenna row /
 *   antennas per slice) keep their bits, in the weights and in both outputs' device copies (the outputs report 0 for them).
 *   scale_bl, ndown_bl: [nbls] doubles each, either may be NULL: scale_b, and the number of samples of S_b with psi < 1.
 * w0 lives in a device plane of its own, allocated and copied from the weights by the first call after a cal_solver_set_data;
 * cal_solver_set_data and cal_solver_set_problem invalidate it, so a fit that never calls this pays no memory for it.  Works for every
 * layout and kernel path, fitting groups of several baselines, bl_alias, nslices > 1, the joint time-basis layout and with gain bases
 * attached.  It runs the model pass of cal_solver_model and, like cal_solver_fit_quality, puts the loop state back: a run continued
 * after a call with an all-zero mask is bit-identical to one without the call. */
enum { CAL_ROBUST_NONE = 0, CAL_ROBUST_HUBER = 1, CAL_ROBUST_CAUCHY = 2, CAL_ROBUST_CLIP = 3 };
typedef struct cal_robust_desc {
  int kind; /* CAL_ROBUST_NONE | HUBER | CAUCHY | CLIP */
  double threshold;
  const uint8_t* slice_mask;
} cal_robust_desc;
int cal_solver_robust_weights(cal_solver* s, const cal_robust_desc* desc, double* scale_bl, double* ndown_bl);
/* The weight plane: which = 0 the weights every kernel reads now, which = 1 w0 (the weights of cal_solver_set_data; equal to the
 * current ones until cal_solver_robust_weights has run).  out: [nbls][nfreqs] in the solver's dtype. */
int cal_solver_get_weights(cal_solver* s, void* out, int which);
/* The gains in closed form (no counterpart in the reference, which moves them by first-order descent only): damped StefCal sweeps
 * (Salvini & Wijnholds 2014).  With the foreground model m = A c held fixed at the solver's coefficients, the chi-square
 * sum w |d - g_i conj(g_j) m|^2 is linear least squares in one antenna's gain while the others are held fixed, with a closed-form
 * minimiser per (antenna, channel).  Baseline b has antennas (i, j) = (bl_ant0, bl_ant1); d, w are the solver's data and weights, g
 * its gains:
 *   P[b][f] = w d conj(m)        (complex)        Q[b][f] = w |m|^2        (real)
 *   role 0 (a == i):  num[a][f] += P g_j              den[a][f] += Q |g_j|^2
 *   role 1 (a == j):  num[a][f] += conj(P) g_i        den[a][f] += Q |g_i|^2
 *   g_new[a][f] = (1 - damping) g[a][f] + damping num/den    where den > 0, else g[a][f] unchanged
 * An autocorrelation row (i == j) enters neither sum (its model is quadratic in one gain).  All antennas are updated from the OLD
 * gains (a Jacobi sweep); damping = 0.5 is StefCal's averaging (damping = 1 stalls on this project's test problems).  Products are
 * formed in the solver's dtype; num and den are accumulated in double in a fixed order (no float atomics: two calls give the same
 * bits), and the update is evaluated in double and rounded once.  The sweeps minimise the chi-square term alone: the "sum"
 * regulariser is not part of the closed form.
 *   nsweeps >= 1 and 0 < damping <= 1 (CAL_ERR_INVALID otherwise); problem, data, coefficients and gains must be set (CAL_ERR_STATE).
 *   slice_mask: [nslices] bytes or NULL (all slices): the gains of a slice whose byte is 0 keep their bits.
 *   reset_gain_moments = 1: the optimizer's gain slots of the selected slices go back to what cal_solver_set_optimizer initialises
 *   them to (stale momentum after a jump in the gains is harmful); iteration counts and the coefficient slots stay.  Needs an
 *   optimizer (CAL_ERR_STATE).
 * With a frequency or time gain basis attached the call fails with CAL_ERR_UNSUPPORTED (projecting the solved gains onto a basis is
 * not implemented here; cal_solver_solve_gain_coeffs solves the coefficients of a frequency basis).  Works for every layout and kernel path, fitting groups of several baselines, bl_alias and nslices > 1: it runs
 * the model pass of cal_solver_model once, then one pass over (b, f) for P and Q, then per sweep one walk of the antennas' baseline
 * lists.  Like cal_solver_fit_quality it puts the loop state back: a run continued after a call with an all-zero mask is
 * bit-identical to one without the call.  Under a communicator or exchange hook every sweep sums num_r | num_i | den over the ranks in
 * ONE all-reduce of 3 nants nfreqs doubles (CAL_XCHG_F64, CAL_XCHG_SUM), and every rank applies the same update. */
typedef struct cal_gain_solve_desc {
  int32_t nsweeps;
  int32_t reset_gain_moments;
  double damping;
  const uint8_t* slice_mask;
} cal_gain_solve_desc;
int cal_solver_solve_gains(cal_solver* s, const cal_gain_solve_desc* desc);
/* Slices that enter every later cal_solver_run / cal_solver_run_slices as already stopped (mask [nslices] bytes, 1 = held; NULL or
 * all zeros: none): a loop issued in several calls keeps a slice that met the tolerance in an earlier call as it is, as one call
 * would.  A held slice reports stopped = 1 and records nothing.  cal_solver_set_optimizer and cal_solver_set_problem clear it. */
int cal_solver_hold_slices(cal_solver* s, const uint8_t* mask);
/* Joint Gauss-Newton steps over gains and coefficients together (no counterpart in the reference): the descent loop is first-order and the
 * closed forms above are block-wise, so alternated they stall in the valley where gains and foregrounds trade against each other.  The joint
 * matrix N = J^H W J is far too large to form and cheap to apply.  Baseline row b has antennas (i, j); d, w are the solver's data and current
 * weights, g its gains, c its coefficients, m = A c what cal_solver_model returns, G = g_i conj(g_j).  grad(d') means the four planes
 * cal_solver_eval_grads returns at the solver's current parameters when the data are d'.  A direction p = (dg [nants][nfreqs], dc [ncoef]) is
 * complex, held as (re, im) planes like the parameters:
 *   (J p)[b][f] = (dg_i conj(g_j) + g_i conj(dg_j)) m + G (A dc)        autocorrelation rows included, by the same formula
 *   N p  = J^H W J p := -1/2 ( grad(G m + J p) - grad(G m) )            four planes, laid out like the gradient
 *   rhs  = J^H W r   := -1/2 ( grad(d)         - grad(G m) )            r = d - G m
 * grad(G m) is zero without the regulariser and the regulariser's own gradient with "sum" (it does not depend on the data): N and rhs are
 * those of the chi-square term alone in both modes, as in every closed form above.  On the device it also cancels the rounding difference
 * between the model pass and the fused pass; it is computed once per call.  In fp32 those two passes round m differently by about 1e-7 |m| and
 * a direction of conjugate gradients near convergence makes J p smaller than that, so the pass evaluates grad(G m + s_t J p) and divides by
 * s_t, one scale per slice: s_t = sqrt(sum w |G m|^2 / sum w |J p|^2) over the slice's rows (sums in double, fixed order; 1 where either is 0).
 * cal_solver_normal_product returns N p in the solver's dtype: p_* and out_* are [nants][nfreqs] and [ncoef] like cal_solver_set_params.
 * cal_solver_gauss_newton_step solves (N + lambda_t D) p = rhs per slice (N is block-diagonal over the slices) by at most ncg iterations of
 * conjugate gradients preconditioned with the diagonal D, from p = 0 (which never moves along a null direction of N: the flux-scale degeneracy
 * stays out of the step):
 *   D_g[a][f] = den_a[f] of cal_solver_solve_gains at the current parameters (autocorrelations left out)
 *   D_c[k]    = sum_{b in gamma} (1 / nfreqs) sum_f w |G|^2 for every coefficient k of group gamma
 *   entries <= 0 or non-finite become 1
 * Each slice has its own alpha_t, beta_t on the device; it freezes once sqrt(rz_t / rz0_t) <= cg_tol, or once s . N s <= 0 or a non-finite
 * scalar appears.  The trial parameters are g + dg, c + dc; the slice's loss there is evaluated as cal_solver_eval_loss does (regulariser
 * included when set) and the slice is accepted iff that loss is finite and strictly below its loss before the step.  A rejected slice, and a
 * slice whose mask byte is 0, keeps the bits of its gains and coefficients.  Nothing else the fit reads differs after the call (data, weights,
 * w0, regulariser, loop state, t, any recorded step graph; the moments unless reset_moments): a run continued after a call with an all-zero
 * mask is bit-identical to one without it.  Dot products run in double in a fixed order: two calls give the same bits.
 * Passes per step: 1 model pass of c, ncg model passes of directions, ncg + 2 gradient passes, 1 loss pass.  The substituted operands are
 * copied into the solver's own data and coefficient planes and back, so every layout and kernel path, folded tiles, groups of several
 * baselines, bl_alias and nslices > 1 work, regulariser on or off.
 *   CAL_ERR_INVALID: null pointers, ncg < 1, cg_tol or a lambda negative or not finite.  CAL_ERR_STATE: problem, data, coefficients or gains
 *   not set; reset_moments without an optimizer.  CAL_ERR_UNSUPPORTED: a frequency or time gain basis is attached (the variables there are y;
 *   the projected step is not implemented), or a communicator or exchange hook is set (the per-slice scalars would need an exchange). */
int cal_solver_normal_product(cal_solver* s, const void* p_g_r, const void* p_g_i, const void* p_c_r, const void* p_c_i,
                              void* out_g_r, void* out_g_i, void* out_c_r, void* out_c_i);      /* N p, solver dtype */
typedef struct cal_gauss_newton_desc {
  int32_t ncg;               /* >= 1 */
  int32_t reset_moments;     /* accepted slices: gain and coefficient slots back to what cal_solver_set_optimizer leaves */
  double cg_tol;             /* >= 0, finite */
  const double* lambda;      /* [nslices], each finite and >= 0 */
  const uint8_t* slice_mask; /* [nslices] or NULL */
} cal_gauss_newton_desc;
typedef struct cal_gauss_newton_result { double loss_before, loss_after, cg_residual; int32_t cg_iters, accepted; } cal_gauss_newton_result;
int cal_solver_gauss_newton_step(cal_solver* s, const cal_gauss_newton_desc* desc, cal_gauss_newton_result* results /* [nslices] */);
/* Quasi-Newton fits (no counterpart in the reference): L-BFGS with a backtracking Armijo line search over the optimizer's own variables,
 * per slice -- its gains (or, with a frequency or time gain basis, its rows of y) and its run of both coefficient planes; with freeze_model
 * the gains alone.  It needs only what every layout and kernel path already produces, the loss and its gradient with respect to those
 * variables, so gain bases and a frozen model are supported where cal_solver_gauss_newton_step refuses them.  Padding (channels past nfreqs,
 * basis padding) takes part in no sum; the inner product is the real one over the (re, im) planes; the slices' scalars stay on the device in
 * double and every sum runs in double in a fixed order (no atomics): two calls give the same bits, and a slice of a batch the bits of the
 * same slice alone.
 *   start       f_0, g_0 from one gradient pass.  f_0 not finite, or |g_0| zero or not finite: status 3, nothing is written.
 *   direction   no stored pair: d = -g_k, t = min(1, 1 / |g_k|).  Else the two-loop recursion over the stored pairs with
 *               gamma = s . y / y . y of the newest pair, t = 1.  slope = g_k . d; slope >= 0 or not finite: the pairs are dropped, d = -g_k.
 *   search      at most max_ls trials x_k + t d (computed in double from the stored values, rounded once to the solver's dtype; with a
 *               basis the gains are expanded from y), one loss pass each, regulariser included; accepted iff the trial loss is finite and
 *               <= f_k + c1 t slope, else t *= shrink.  No trial accepted: with pairs stored they are dropped and the same iteration
 *               searches again along -g_k (its trials count in evals); with none the slice gets the bits of x_k back, status 2.
 *   pair        one gradient pass at the accepted point gives g_{k+1} and the recorded loss f_{k+1}; s = x_{k+1} - x_k, y = g_{k+1} - g_k
 *               (stored in the solver's dtype) enter the ring of `history` pairs iff s . y is finite and > curvature_eps sqrt(s.s y.y).
 *   stop        status 1 once ftol > 0 and f_k - f_{k+1} <= ftol |f_k|; status 0 after nsteps iterations; status 4: mask byte 0, never written.
 * pairs_dropped counts the pairs the curvature test kept out and the pairs thrown away when a direction or a search failed.
 * Passes: 1 + iters gradient passes and evals loss passes.  The host reads one integer per trial round (how many slices still search).
 * Data, weights, w0, regulariser, loop state, t and any recorded step graph stay as found on every path out of the call; so do the moments
 * unless reset_moments: then the slots of the variables of the slices that moved are what cal_solver_set_optimizer leaves.
 * Device memory: 2 history + 4 vectors in the solver's dtype over the variable space (counted by cal_solver_memory_bytes).
 *   CAL_ERR_INVALID: null desc or results, nsteps < 1, history outside [1, 16], max_ls < 1, c1 or shrink outside (0, 1), ftol or
 *   curvature_eps negative or not finite.  CAL_ERR_STATE: problem, data, coefficients or gains not set; reset_moments without an optimizer.
 *   CAL_ERR_UNSUPPORTED: a communicator or exchange hook is set (the dot products would need an exchange). */
typedef struct cal_lbfgs_desc {
  int32_t nsteps;            /* >= 1 iterations */
  int32_t history;           /* 1 .. 16 stored pairs */
  int32_t max_ls;            /* >= 1 trials per search */
  int32_t freeze_model;      /* the coefficients are no variables and keep their bits */
  int32_t reset_moments;
  int32_t reserved;
  double c1, shrink;         /* each in (0, 1) */
  double ftol;               /* >= 0; 0: no loss test */
  double curvature_eps;      /* >= 0 */
  const uint8_t* slice_mask; /* [nslices] or NULL */
} cal_lbfgs_desc;
typedef struct cal_lbfgs_result { double loss_before, loss_after; int32_t iters, evals, pairs_dropped, status; } cal_lbfgs_result;
int cal_solver_lbfgs(cal_solver* s, const cal_lbfgs_desc* desc, double* losses_out /* [nslices][nsteps + 1], NaN past iters, may be NULL */,
                     cal_lbfgs_result* results /* [nslices] */);
/* Host only, no device: the coefficients of the L-BFGS direction from the Gram matrix gram [2 npairs + 1][2 npairs + 1] of
 * b = [s_1 .. s_p (oldest first), y_1 .. y_p, g]: delta [2 npairs + 1] with d = sum_j delta_j b_j, and *slope = g . d.  The function the
 * device runs (lbfgs_core.hpp).  npairs in [0, 16]. */
int cal_debug_lbfgs_coefficients(int32_t npairs, const double* gram, double* delta, double* slope);
/* The foreground coefficients in closed form (no counterpart in the reference): the other half of alternating least squares next to
 * cal_solver_solve_gains.  With the gains held fixed the chi-square sum w |d - g_i conj(g_j) (A c)|^2 is linear least squares in the
 * coefficients and separates by fitting group.  Group gamma has nvec complex coefficients c; its baselines b have antennas (i, j) and
 * the real row block A_b [nfreqs][nvec] of the group's basis; d, w are the solver's data and weights, g its full (expanded) gains,
 * m = A c at the solver's current coefficients:
 *   G[b][f] = g_i[f] conj(g_j[f])
 *   u[b][f] = w conj(G) (d - G m)          (complex)
 *   q[b][f] = w |G|^2                      (real)
 *   N   = sum_{b in gamma} A_b^T diag(q_b) A_b   [nvec][nvec], real symmetric
 *   rhs = sum_{b in gamma} A_b^T u_b             [nvec], complex
 *   N_r = N + ridge (tr N / nvec) I
 *   N_r delta = rhs                              (one factorisation, two right-hand sides: re, im)
 *   c_new = c + damping delta
 * rhs is minus half the chi-square gradient with respect to c: with ridge = 0 and damping = 1 the step lands on the minimiser; with
 * ridge > 0 it is a Levenberg step whose fixed point is still the exact minimiser.  Baselines of a group that share a row block
 * share A: their q and u are summed first.  An autocorrelation row is an ordinary row (the model is linear in c).  The solve
 * minimises the chi-square term alone: the "sum" regulariser is not part of it.
 * Precision: u, q, N and rhs are formed and accumulated in the solver's dtype in a fixed order (no atomics on reals: two calls give the
 * same bits; N and rhs on v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64); the Cholesky factorisation of N_r, the substitutions
 * and the update are evaluated in double for both dtypes, and the update is rounded to the solver's dtype once.
 * A group is singular when tr N <= 0 (wholly flagged) or a pivot is <= 0 or not finite: it keeps the bits of its coefficients and is
 * counted in nsingular.  Suggested values: damping = 1, ridge = 1e-6 (flagged band edges take cond(N) to 1e8, beyond an fp32 Gram),
 * niters = 1; every iteration repeats the whole sequence from the current coefficients (in fp32 a second one is iterative
 * refinement).  result (may be NULL) counts the groups of the LAST iteration; groups of unselected slices count in neither field.
 *   niters >= 1, 0 < damping <= 1, ridge >= 0 and finite (CAL_ERR_INVALID otherwise); problem, data, coefficients and gains must be
 *   set, and reset_coeff_moments needs an optimizer (CAL_ERR_STATE).
 *   slice_mask: [nslices] bytes or NULL (all slices): the coefficients of a slice whose byte is 0 keep their bits.
 *   reset_coeff_moments = 1: the optimizer's coefficient slots of the selected slices go back to what cal_solver_set_optimizer
 *   initialises them to; iteration counts and the gain slots stay.
 * Gains, gain coefficients of a gain basis (y, g0), gain moments, t and iteration counts are never touched: unlike
 * cal_solver_solve_gains the call works with a frequency and / or time gain basis attached (it reads the expanded gains).  Works for
 * every layout and kernel path, folded and full tiles, fitting groups of several baselines, bl_alias, nslices > 1 and the joint
 * time-basis layout: it runs the model pass of cal_solver_model, one pass over (b, f) for u and q, then per group the Gram product
 * straight from the solver's basis tiles and the factorisation.  The groups are worked through heaviest first in chunks whose
 * scratch (N in the solver's dtype plus its factor in double) stays under 256 MiB -- never less than the largest group needs.
 * Like cal_solver_fit_quality it puts the loop state back: a run continued after a call with an all-zero mask is bit-identical to
 * one without the call.  Under a communicator or exchange hook the call issues NO collective: every fitting group belongs to one
 * rank, and the gains are replicated. */
typedef struct cal_coeff_solve_desc {
  int32_t niters;               /* >= 1 */
  int32_t reset_coeff_moments;
  double damping;               /* (0, 1] */
  double ridge;                 /* >= 0 */
  const uint8_t* slice_mask;    /* [nslices] or NULL */
} cal_coeff_solve_desc;
typedef struct cal_coeff_solve_result { int32_t nsolved; int32_t nsingular; } cal_coeff_solve_result; /* of the last iteration */
int cal_solver_solve_coeffs(cal_solver* s, const cal_coeff_solve_desc* desc, cal_coeff_solve_result* result);
/* The scratch bound of cal_solver_solve_coeffs in bytes (0: the default, 256 MiB).  The coefficients do not depend on it: tests use
 * it to send a small problem through several chunks. */
int cal_solver_set_coeff_solve_scratch(cal_solver* s, int64_t bytes);
/* The errors of a fit (no counterpart in the reference): the inverses of the curvature matrices that cal_solver_solve_coeffs and
 * cal_solver_solve_gains build.  In their notation -- baseline row b of fitting group gamma has antennas (i, j) and row block
 * A_b [nfreqs][nvec], a_{b,f} is row f of A_b, d, w are the solver's data and current weights, g its full (expanded) gains, m = A c at
 * the current coefficients:
 *   G[b][f]   = g_i[f] conj(g_j[f])          q[b][f] = w |G|^2
 *   N_gamma   = sum_{b in gamma} A_b^T diag(q_b) A_b      N_r = N_gamma + ridge (tr N_gamma / nvec) I      L L^T = N_r
 *   coeff_var[k]    = (N_r^-1)[k][k]                               [ncoef]           (re and im of c_k each have this variance / 2)
 *   model_var[b][f] = a_{b,f}^T N_r^-1 a_{b,f} = |L^-1 a_{b,f}|^2  [nbls][nfreqs]    (variance of m = A c, before the gains)
 *   lev[b][f]       = q[b][f] model_var[b][f]                      in [0, 1]
 *   leverage_bl[b]  = sum_f lev[b][f]                              [nbls]            (the parameters the model spent on row b)
 *   nsamp_bl[b]     = #{f : w[b][f] != 0}                          [nbls]            (an integer, returned as a double)
 *   gain_var[a][f]  = 1 / den_a[f], den_a = sum_b w |m|^2 |g_other|^2 as in cal_solver_solve_gains (autocorrelations left out);
 *                     0 where den_a <= 0                           [nants][nfreqs]
 * All outputs are doubles and variances for unit noise scale: exact where the weights are inverse noise variances 1 / E|n|^2.  They
 * are CONDITIONAL errors: the gains are held fixed for the coefficients and the model, the model and the other gains for a gain.
 * That is the block diagonal of the Gauss-Newton matrix; it ignores the gain-foreground covariance and with it the degeneracies,
 * so these are lower bounds.  With ridge = 0 and N of full rank, sum_{b in gamma} leverage_bl[b] = nvec.
 * N is formed in the solver's dtype on the matrix cores (coeff_gram_kernel as it is), factorised in double with
 * cal_solver_solve_coeffs' trace, ridge and singularity tests; W = L^-1 is rounded to the solver's dtype once and |W a|^2 runs on
 * the matrix cores, its squares summed in double.  A group that is singular by those tests keeps zeros in coeff_var, model_var and
 * leverage_bl and counts in nsingular.  Channels [nfreqs, fpad) never contribute.  Everything is summed in a fixed order: two calls
 * give the same bits.
 *   Any output pointer may be NULL.  Without model_var and leverage_bl the per-sample kernel is not launched; without coeff_var
 *   too nothing of the coefficient part runs; without gain_var the antenna part does not run.  counts may be NULL.
 *   ridge >= 0 and finite (CAL_ERR_INVALID); problem, data, coefficients and gains must be set (CAL_ERR_STATE).
 * Works with nslices > 1, bl_alias, groups of several baselines on several row blocks, both layouts, every kernel path and folded
 * tiles.  The coefficient outputs work with a frequency or time gain basis attached (the expanded gains are read); gain_var then
 * fails with CAL_ERR_UNSUPPORTED: the variance of a basis gain is b_f^T N_a^-1 b_f with the projected N_a, which is not computed here
 * but by cal_solver_gain_basis_errors below.
 * The groups are worked through in chunks under the bound of cal_solver_set_coeff_solve_scratch (N, the factor in double and W).
 * Like cal_solver_fit_quality it puts the loop state back: a run continued after the call is bit-identical to one without it.
 * Under a communicator or exchange hook every fitting group belongs to one rank and each rank fills its own rows: the coefficient
 * outputs need no exchange.  den is summed over the ranks in ONE all-reduce of nants nfreqs doubles (CAL_XCHG_F64, CAL_XCHG_SUM),
 * issued only when gain_var is asked for. */
typedef struct cal_fit_errors_counts { int32_t nsolved; int32_t nsingular; } cal_fit_errors_counts;
int cal_solver_fit_errors(cal_solver* s, double ridge, double* coeff_var, double* model_var, double* leverage_bl, double* nsamp_bl,
                          double* gain_var, cal_fit_errors_counts* counts);
/* The error bars of gains confined to a basis (no counterpart in the reference): the inverse of the projected curvature matrix that
 * cal_solver_solve_gain_coeffs and cal_solver_solve_gain_time_coeffs build, at the solver's current parameters.  In their notation
 * (den[row][f] of cal_solver_solve_gains, autocorrelations left out, summed over the ranks; shift = ridge tr N / n); conditional on the
 * other antennas and the model like gain_var of cal_solver_fit_errors, which B = I reproduces (1 / den):
 *   frequency basis B [nfreqs][K], per antenna row a (n = K):
 *     N_a = B^T diag(den_a) B     N_r = N_a + shift I     L L^T = N_r     W = L^-1
 *     y_var[a][k]    = sum_i W[i][k]^2                        (variance of the complex y_k)
 *     gain_var[a][f] = |W b_f|^2 = b_f^T N_r^-1 b_f           (b_f: row f of B), every f < nfreqs, flagged channels included
 *     gain_dof[a]    = n - shift sum_k y_var[a][k]            (= tr(N_a N_r^-1): complex parameters spent)
 *   time x frequency basis Bt [T][L], per antenna a, n = L K, index l K + k, N_a[(l,k),(l',k')] = sum_t Bt[t,l] Bt[t,l'] M_{t,a}[k,k']:
 *     gain_var[t Na + a][f] = |W (Bt[t,:] (x) b_f)|^2         y_var[a][l][k] = sum_i W[i][l K + k]^2        gain_dof[a] as above
 *   time basis alone, per (antenna, channel), L x L:
 *     N_{a,f}[l,l'] = sum_t Bt[t,l] Bt[t,l'] den[t,a,f]       y_var[a][l][f] = (N_r^-1)[l][l]
 *     gain_var[t Na + a][f] = Bt[t,:] N_r^-1 Bt[t,:]^T        gain_dof[a] = sum over the solved f of (L - shift_f sum_l y_var[a][l][f])
 * Outputs, all doubles, variances for unit noise scale, any may be NULL (its work is skipped): gain_var [nants][nfreqs];
 * y_var [y_rows][L or 1][K, or nfreqs without a frequency basis], unpadded; gain_dof [y_rows] (y_rows: nants, or Na under a time basis).
 * A system (an antenna row, an antenna, or an (antenna, channel) pair under a time basis alone) that is singular by the solves' tests
 * (tr <= 0, a pivot <= 0, or not finite) leaves zeros in all its outputs and counts in nsingular, a solved one in nsolved.  N is formed
 * in the solver's dtype (the solves' kernels as they are), factorised in double; W is rounded to the solver's dtype once and |W x|^2
 * runs on the matrix cores, its squares summed in double; the time basis alone runs in double throughout.  Every sum has a fixed order:
 * two calls give the same bits.  The rows are worked through in chunks under the bound of cal_solver_set_coeff_solve_scratch (the
 * solves' buffers and W); the results do not depend on it.
 *   ridge >= 0 and finite (CAL_ERR_INVALID); problem, data, coefficients and gains must be set, and a gain basis
 *   (cal_solver_set_gain_basis, cal_solver_set_gain_time_basis): CAL_ERR_STATE without one -- cal_solver_fit_errors gives gain_var of free gains.
 * y, the gains, the optimizer's slots and the loop state are untouched: a run continued after the call is bit-identical to one without
 * it.  y is replicated and den is summed over the ranks in ONE all-reduce of nants nfreqs doubles (CAL_XCHG_F64, CAL_XCHG_SUM), so
 * every rank computes the same planes. */
int cal_solver_gain_basis_errors(cal_solver* s, double ridge, double* gain_var, double* y_var, double* gain_dof, cal_fit_errors_counts* counts);
/* Where the power of data, model and residual sits in DELAY (no counterpart in the reference): the transform along frequency of
 * every baseline row as one complex matrix product against a small operator shared by all rows, from the planes the solver holds.
 * For baseline row b with antennas (i, j) and channel f, in solver units:
 *   w = the weight plane as the solver holds it now, m = A c with the current coefficients, g = the gains of this call,
 *   G[b][f]    = g_i[f] conj(g_j[f])                 mask[b][f] = (w[b][f] != 0)
 *   q[b][f]    = d, G m, d - G m                     (calibrated = 0: data, model, residual, bits 0, 1, 2 of `what`)
 *              = d / G, m, d / G - m                 (calibrated = 1; all three zero where |G|^2 == 0)
 *   x_q[b][f]  = mask q[b][f]                        formed in the solver's dtype, in the order the loss kernels form them
 *   X_q[b][k]  = sum_f x_q[b][f] (op_r + i op_i)[f][k]                            k < ndelays
 *   norm_bl[b] = sum_f mask norm_f[f]                                             [nbls]
 *   power_bl[q][b][k]  = |X_q[b][k]|^2 / norm_bl[b]; 0 where norm_bl[b] == 0      [nwhat][nbls][ndelays]
 *   power_bin[q][n][k] = sum of power_bl[q][b][k] over the rows b with bin_of_bl[b] == n and norm_bl[b] > 0,
 *                        taken in ascending b                                     [nwhat][nbins][ndelays]
 *   count_bin[n]       = the number of such rows (an integer, returned as a double)   [nbins]
 * nwhat is the number of bits set in `what`; the quantities asked for are stored in the order data, model, residual.  op is any
 * operator [nfreqs][ndelays] -- a tapered DFT (modeling.delay_transform), a least-squares or DPSS spectral estimator -- with the taper
 * folded in; norm_f is what an unflagged channel adds to a row's normalisation (the taper squared).  A row that is flagged throughout
 * has power 0 and enters no bin.
 * The products run on the matrix cores in the solver's dtype (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64); |X|^2, the division
 * and every sum over rows are taken in double in a fixed order, no float atomics: two calls give the same bits.  All outputs are
 * doubles; any output pointer may be NULL (power_bin and count_bin need nbins > 0).
 *   g_r, g_i: as in cal_solver_fit_quality -- [nants][nfreqs] or both NULL; NULL: the solver's current full gains, whatever gain
 *   bases are set; given gains are used for this call only.
 * Errors: CAL_ERR_STATE when problem, data or coefficients are not set, or the gains neither set nor given; CAL_ERR_INVALID for a
 * null description, a `what` without a bit of 1 | 2 | 4 (or with others), ndelays outside [1, 4096], a `calibrated` other than 0 or
 * 1, nbins < 0, a bin_of_bl that is NULL with nbins > 0 (or given with nbins == 0) or holds an index outside [-1, nbins), a null
 * operator or norm_f.
 * Works for every layout and kernel path, fitting groups of several baselines, bl_alias, nslices > 1 and the joint time-basis layout:
 * a row is a row, and the caller's bin_of_bl decides what is averaged with what.  It runs the model pass of cal_solver_model and, like
 * cal_solver_fit_quality, puts the loop state back: a run continued after the call is bit-identical to one without it.
 * The rows are worked through in chunks whose scratch -- the masked planes in the solver's dtype and, when power_bl or bins are asked
 * for, the chunk's power in double -- stays under the bound of cal_solver_set_delay_spectrum_scratch (never less than one row).  The
 * result does not depend on the chunks by a bit; the full [nwhat][nbls][ndelays] array never exists on the device.
 * Under a communicator or exchange hook power_bin | count_bin are summed over the ranks in ONE all-reduce of
 * nwhat nbins ndelays + nbins doubles (CAL_XCHG_F64, CAL_XCHG_SUM), whichever outputs are asked for (nbins == 0: none); power_bl and
 * norm_bl stay the rank's own rows. */
typedef struct cal_delay_spectrum_desc {
  int32_t ndelays;          /* columns of the operator, 1 <= ndelays <= 4096 */
  int32_t what;             /* bit 0: data, bit 1: model, bit 2: residual; at least one */
  int32_t calibrated;       /* 0: d, G m, d - G m (G = g_i conj(g_j)); 1: d / G, m, d / G - m, zero where |G|^2 == 0 */
  int32_t nbins;            /* 0: no binned output */
  const int32_t* bin_of_bl; /* [nbls] in [-1, nbins): -1 leaves the row out; NULL iff nbins == 0 */
  const void* op_r;         /* [nfreqs][ndelays], solver dtype: the transform along frequency, taper folded in */
  const void* op_i;
  const double* norm_f;     /* [nfreqs]: what an unflagged channel adds to the row's normalisation (the taper squared) */
} cal_delay_spectrum_desc;
int cal_solver_delay_spectrum(cal_solver* s, const cal_delay_spectrum_desc* desc, const void* g_r, const void* g_i, double* power_bl,
                              double* norm_bl, double* power_bin, double* count_bin);
/* The scratch bound of cal_solver_delay_spectrum in bytes (0: the default, 256 MiB; negative: CAL_ERR_INVALID).  The outputs do not
 * depend on it: tests use it to send a small problem through several chunks.  cal_solver_delay_cross_spectrum shares it. */
int cal_solver_set_delay_spectrum_scratch(cal_solver* s, int64_t bytes);
/* Delay power that noise does not bias: the cross power of two rows that see the same sky with independent noise -- two adjacent
 * integrations of one baseline, as rows of one solver (nslices > 1, bl_alias, the joint time-basis layout) -- and the power of their
 * half difference, the noise spectrum measured from the data.  cal_solver_delay_spectrum's |X|^2 of a residual is signal plus the
 * full noise power; here the sky, slow in time, survives the product and the noise averages to zero.  Notation of
 * cal_solver_delay_spectrum: row b, G, m, w and the quantities q = data, model, residual (calibrated or not), formed in the solver's
 * dtype exactly as there.  For pair p = (b0, b1) = pairs[p] with scales (a0, a1) = scale[p]:
 *   mask_p[f]      = (w[b0][f] != 0) && (w[b1][f] != 0)            the COMMON mask: two rows flagged differently leak foregrounds
 *                                                                  differently, and the leakage would not cancel
 *   x_q[p][s][f]   = mask_p q[b_s][f]                              s = 0, 1
 *   X_q[p][s][k]   = sum_f x_q[p][s][f] (op_r + i op_i)[f][k]
 *   norm_pair[p]   = sum_f mask_p norm_f[f]                                                         [npairs]
 *   Y_s            = a_s X_q[p][s][k]                              in double, after the matrix product
 *   cross[q][p][k] = (Re Y_0 Re Y_1 + Im Y_0 Im Y_1) / norm_pair[p]     0 where norm_pair[p] == 0   [nwhat][npairs][ndelays], signed
 *   diff[q][p][k]  = ((Re Y_0 - Re Y_1)^2 + (Im Y_0 - Im Y_1)^2) / (2 norm_pair[p])                 [nwhat][npairs][ndelays], >= 0
 *   cross_bin / diff_bin [q][n][k] = the sum over the pairs p with bin_of_pair[p] == n and norm_pair[p] > 0, in ascending p
 *                                                                                                   [nwhat][nbins][ndelays]
 *   count_bin[n]   = their number                                                                   [nbins]
 * The scales put both sides into common units before they are combined (a caller that divides every slice by its own rms passes the
 * rms values); NULL: ones.  A pair may join any two rows, (b, b) included: with unit scales its diff is exactly 0 and its cross is
 * cal_solver_delay_spectrum's power_bl[b] to the bit.  With independent noise of equal variance on both sides the expectation of cross
 * is that of the common signal alone and the expectation of diff is the noise power of one side.
 * The products run on the matrix cores in the solver's dtype, by the loop of cal_solver_delay_spectrum; scaling, products, the division
 * and every sum over pairs are taken in double in a fixed order, no float atomics: two calls give the same bits, and so do two
 * chunkings.  All outputs are doubles; any output pointer may be NULL.
 *   g_r, g_i: as in cal_solver_delay_spectrum -- NULL: the solver's current full gains; given gains are used for this call only.
 * Errors, before any launch: those of cal_solver_delay_spectrum (CAL_ERR_STATE when problem, data or coefficients are not set, or the
 * gains neither set nor given; CAL_ERR_INVALID for a null description, a bad `what`, ndelays, `calibrated`, nbins, bin_of_pair, a
 * null operator or norm_f); CAL_ERR_INVALID for npairs < 1, null pairs, a row index outside [0, nbls), a `stats` without a bit of
 * 1 | 2 (or with others), a scale that is not finite, cross_pair / cross_bin without bit 0 or diff_pair / diff_bin without bit 1,
 * binned outputs with nbins == 0.
 * Works for every layout and kernel path, fitting groups of several baselines, bl_alias, nslices > 1 and the joint time-basis layout.
 * A post-fit pass: it runs the model pass of cal_solver_model and puts the loop state back; a run continued after the call is
 * bit-identical to one without it.
 * The pairs are worked through in chunks whose scratch -- the masked planes of both sides in the solver's dtype and the chunk's
 * statistics in double -- stays under the bound of cal_solver_set_delay_spectrum_scratch (never less than one pair; cut at multiples
 * of 64 pairs where that fits); the device buffers of cal_solver_delay_spectrum are reused.  The result does not depend on the chunks
 * by a bit.
 * Under a communicator or exchange hook cross_bin | diff_bin | count_bin (those of the bits set) are summed over the ranks in ONE
 * all-reduce of nstat nwhat nbins ndelays + nbins doubles (CAL_XCHG_F64, CAL_XCHG_SUM), whichever outputs are asked for (nbins == 0:
 * none); the per-pair outputs stay the rank's own. */
typedef struct cal_delay_cross_desc {
  int32_t ndelays;            /* columns of the operator, 1 <= ndelays <= 4096 */
  int32_t what;               /* bit 0: data, bit 1: model, bit 2: residual; at least one */
  int32_t calibrated;         /* as in cal_delay_spectrum_desc */
  int32_t npairs;             /* >= 1 */
  const int32_t* pairs;       /* [npairs][2]: any two rows of the solver, each in [0, nbls) */
  const double* scale;        /* [npairs][2], finite; NULL: ones */
  int32_t stats;              /* bit 0: cross, bit 1: diff; at least one */
  int32_t nbins;              /* 0: no binned output */
  const int32_t* bin_of_pair; /* [npairs] in [-1, nbins): -1 leaves the pair out; NULL iff nbins == 0 */
  const void* op_r;           /* [nfreqs][ndelays], solver dtype: the transform along frequency, taper folded in */
  const void* op_i;
  const double* norm_f;       /* [nfreqs]: what a channel unflagged on both sides adds to the pair's normalisation */
} cal_delay_cross_desc;
int cal_solver_delay_cross_spectrum(cal_solver* s, const cal_delay_cross_desc* desc, const void* g_r, const void* g_i, double* cross_pair,
                                    double* diff_pair, double* norm_pair, double* cross_bin, double* diff_bin, double* count_bin);
/* The delay / fringe-rate plane: the delay transform of T rows that are one baseline at T integrations, and then a transform ALONG
 * time.  cal_solver_delay_spectrum, cal_solver_delay_transfer and cal_solver_delay_cross_spectrum treat time as a label; along time,
 * cross-talk and other instrument-locked residuals sit at fringe rate 0, the sky at the fringe rate its baseline gives it, and noise
 * is white.  The rate-0 row is the coherent time average every power-spectrum pipeline takes before squaring; the cross and
 * half-difference powers of cal_solver_delay_cross_spectrum are the two fringe-rate channels of a window of two.  Notation of
 * cal_solver_delay_spectrum: row b, G, m, w and the quantities q = data, model, residual (calibrated or not), formed in the solver's
 * dtype exactly as there.  A group g is an ordered list of T = ntimes rows rows[g][0 .. T) -- any rows of the solver, repeats
 * allowed; in practice one baseline at T consecutive integrations (nslices > 1, bl_alias, the joint time-basis layout) -- with scales
 * a[g][t] = scale[g][t]:
 *   mask_g[f]         = AND over t of (w[rows[g][t]][f] != 0)          the COMMON mask of all T rows: rows flagged differently leak
 *                                                                     foregrounds differently
 *   x_q[g][t][f]      = mask_g[f] q[rows[g][t]][f]
 *   X_q[g][t][k]      = sum_f x_q[g][t][f] (op_r + i op_i)[f][k]      matrix cores, solver dtype, the loop of cal_solver_delay_spectrum
 *   Y_t               = a[g][t] X_q[g][t][k]                          in double, after the matrix product
 *   Z_q[g][r][k]      = sum_t (opt_r + i opt_i)[t][r] Y_t             complex, in double
 *   norm_grp[g]       = sum_f mask_g[f] norm_f[f]                                                      [ngroups]
 *   power_grp[q][g][r][k] = (Re Z^2 + Im Z^2) / norm_grp[g]     0 where norm_grp[g] == 0               [nwhat][ngroups][nrates][ndelays]
 *   power_bin[q][n][r][k] = the sum over the groups g with bin_of_group[g] == n and norm_grp[g] > 0, in ascending g
 *                                                                                                      [nwhat][nbins][nrates][ndelays]
 *   count_bin[n]      = their number                                                                   [nbins]
 * The order of operations for Z is part of the definition: the accumulators start at zero and, for t ascending,
 * re += (opt_r yr - opt_i yi) and im += (opt_r yi + opt_i yr), without contraction.  Hence, to the bit: ntimes = 1 with opt = [[1]]
 * and unit scale gives cal_solver_delay_spectrum's power_bl of the row; ntimes = 2 with opt = [[1, 1], [1, -1]] gives at rate 1 twice
 * cal_solver_delay_cross_spectrum's diff of the same pairs.
 * opt is any complex operator [ntimes][nrates] given in double: the caller folds the taper along time and its normalisation into
 * it; there is no norm_t.  The scales put the rows into common units (a caller that divides every slice by its own rms passes the rms
 * values); NULL: ones.
 * The mask is common: a group with one row flagged throughout has norm_grp == 0, power 0, and enters no bin.
 * Scaling, the sum over time, the division and every sum over groups are taken in double in a fixed order, no float atomics: two calls
 * give the same bits, and so do two chunkings.  All outputs are doubles; any output pointer may be NULL.
 *   g_r, g_i: as in cal_solver_delay_spectrum -- NULL: the solver's current full gains; given gains are used for this call only.
 * Errors, before any launch: those of cal_solver_delay_spectrum (CAL_ERR_STATE when problem, data or coefficients are not set, or the
 * gains neither set nor given; CAL_ERR_INVALID for a null description, a bad `what`, ndelays, `calibrated`, nbins, bin_of_group, a
 * null operator or norm_f); CAL_ERR_INVALID for ngroups < 1, ntimes or nrates outside [1, 64], null rows or opt, a row outside
 * [0, nbls), a scale or operator entry that is not finite, a bin outside [-1, nbins), binned outputs with nbins == 0.
 * Works for every layout and kernel path, fitting groups of several baselines, bl_alias, nslices > 1 and the joint time-basis layout.
 * A post-fit pass: it runs the model pass of cal_solver_model and puts the loop state back; a run continued after the call is
 * bit-identical to one without it.  It reads the ONE weight plane the other reports read, the one cal_solver_robust_weights rewrites,
 * not the weights as set.
 * The groups are worked through in chunks of whole groups whose scratch -- per group nwhat 2 ntimes pitch elements of the solver's dtype
 * for the masked planes, nwhat 2 ntimes ndelays doubles of Y and nwhat nrates ndelays doubles of power -- stays under the bound of
 * cal_solver_set_delay_spectrum_scratch (never less than one group); the device buffers of cal_solver_delay_spectrum are reused.  The
 * result does not depend on the chunks by a bit.
 * Under a communicator or exchange hook power_bin | count_bin are summed over the ranks in ONE all-reduce of
 * nwhat nbins nrates ndelays + nbins doubles (CAL_XCHG_F64, CAL_XCHG_SUM), whichever outputs are asked for (nbins == 0: none); the
 * per-group outputs stay the rank's own. */
typedef struct cal_delay_fringe_desc {
  int32_t ndelays;             /* columns of the operator, 1 <= ndelays <= 4096 */
  int32_t what;                /* bit 0: data, bit 1: model, bit 2: residual; at least one */
  int32_t calibrated;          /* as in cal_delay_spectrum_desc */
  int32_t ngroups;             /* >= 1 */
  int32_t ntimes;              /* rows of a group, 1 <= ntimes <= 64 */
  int32_t nrates;              /* columns of opt, 1 <= nrates <= 64 */
  const int32_t* rows;         /* [ngroups][ntimes]: rows of the solver, each in [0, nbls), repeats allowed */
  const double* scale;         /* [ngroups][ntimes], finite; NULL: ones */
  int32_t nbins;               /* 0: no binned output */
  const int32_t* bin_of_group; /* [ngroups] in [-1, nbins): -1 leaves the group out; NULL iff nbins == 0 */
  const void* op_r;            /* [nfreqs][ndelays], solver dtype: the transform along frequency, taper folded in */
  const void* op_i;
  const double* norm_f;        /* [nfreqs]: what a channel unflagged in all rows adds to the group's normalisation */
  const double* opt_r;         /* [ntimes][nrates], finite: the transform along time, taper and normalisation folded in */
  const double* opt_i;
} cal_delay_fringe_desc;
int cal_solver_delay_fringe_spectrum(cal_solver* s, const cal_delay_fringe_desc* desc, const void* g_r, const void* g_i, double* power_grp,
                                     double* norm_grp, double* power_bin, double* count_bin);
/* Delay / fringe-rate power of redundant averages: the coherent sum.  cal_solver_delay_spectrum, cal_solver_delay_cross_spectrum and
 * cal_solver_delay_fringe_spectrum square ONE baseline row at a time and reach a baseline-length bin only as a mean of powers, an
 * incoherent average.  A power-spectrum pipeline for a redundant array adds the calibrated visibilities of a redundant group first,
 * then transforms and squares: noise power then falls as 1 / N in the group size.  The notation is that of
 * cal_solver_delay_fringe_spectrum: row b, G, m, w and the quantities q = data, model, residual (calibrated or not), formed in the
 * solver's dtype exactly as there, under the row's own mask (w[b][f] != 0).
 * A group g has T = ntimes SETS.  Set v = g T + t holds the members k in [set_ptr[v], set_ptr[v + 1]).  Each member has a row
 * member_row[k] in [0, nbls), repeats allowed; a coefficient omega_k = member_wgt[k], finite and >= 0 (NULL: ones); a flag
 * member_conj[k] in {0, 1} (NULL: none).
 *   u_k[f]      = omega_k                        (weighting = 0)
 *               = omega_k (double) w[b_k][f]     (weighting = 1)
 *                 both taken as 0 where w[b_k][f] == 0
 *   den_v[f]    = sum_k u_k[f]                   in double, k ascending from 0
 *   xbar_q[v][f]= ( sum_k u_k[f] c_k(q[b_k][f]) ) / den_v[f]
 *                 c_k negates Im where member_conj[k]
 *                 re and im are summed separately, in double, k ascending from 0,
 *                 acc += u * (double) q with contraction off
 *                 then divided, then rounded ONCE to the solver's dtype
 *                 0 where den_v[f] == 0
 *   mask_v[f]   = den_v[f] > 0
 *   mask_g[f]   = AND over t of mask_(g,t)[f]
 *   x_q[g][t][f]= mask_g[f] ? xbar_q[g T + t][f] : 0
 * From x_q on, everything is cal_solver_delay_fringe_spectrum's definition, word for word: X = x op on the matrix cores by the same
 * loop, Y_t = scale[g][t] X in double, Z = sum_t opt Y_t in the stated order, norm_grp = sum_f mask_g norm_f, power = |Z|^2 / norm_grp,
 * the bins and count_bin.  Outputs: power_grp [nwhat][ngroups][nrates][ndelays], norm_grp [ngroups], power_bin
 * [nwhat][nbins][nrates][ndelays], count_bin [nbins]; all doubles, any of them may be NULL.  An empty set gives its group norm_grp == 0,
 * power 0 and no bin.
 * Hence, to the bit: (a) sets of one member with unit coefficient, no conjugation and weighting = 0 give
 * cal_solver_delay_fringe_spectrum on rows[g][t] = that member (1.0 q / 1.0 is exact); (b) a set that holds one row twice gives the
 * bits of that row once; (c) with ntimes = 1 and opt = [[1]], singleton sets all conjugated and the operator conj(op) give the bits of
 * the unconjugated sets with op (every product of the complex transform changes sign or keeps it as a whole, and IEEE rounding is
 * sign-symmetric); two calls give the same bits, and so does any scratch bound.
 * set_ptr is int64 [ngroups ntimes + 1]; it starts at 0, never falls and ends at nmembers.
 * Errors, before any launch: those of cal_solver_delay_fringe_spectrum (with set_ptr and member_row in the place of rows);
 * CAL_ERR_INVALID for a set_ptr that does not start at 0, falls, or does not end at nmembers, a member row outside [0, nbls), a
 * coefficient that is negative or not finite, a member_conj other than 0 or 1, a weighting other than 0 or 1, nmembers above 2^30.
 * Works for every layout and kernel path, bl_alias, nslices > 1 and the joint time-basis layout.  A post-fit pass like
 * cal_solver_delay_fringe_spectrum: it puts the loop state back, and it reads the ONE weight plane cal_solver_robust_weights rewrites.
 * The groups are worked through in chunks of whole groups whose scratch -- the fringe call's per group over the averaged planes, plus
 * ntimes pitch bytes of set masks -- stays under the bound of cal_solver_set_delay_spectrum_scratch (never less than one group); the
 * member lists are uploaded once per call; the device buffers of cal_solver_delay_spectrum are reused.
 * Under a communicator or exchange hook power_bin | count_bin are summed over the ranks in ONE all-reduce of
 * nwhat nbins nrates ndelays + nbins doubles (CAL_XCHG_F64, CAL_XCHG_SUM), whichever outputs are asked for (nbins == 0: none); the
 * per-group outputs stay the rank's own, and the caller keeps a group's rows on one rank. */
typedef struct cal_delay_coherent_desc {
  int32_t ndelays;             /* as in cal_delay_fringe_desc */
  int32_t what;
  int32_t calibrated;
  int32_t ngroups;             /* >= 1 */
  int32_t ntimes;              /* sets of a group, 1 <= ntimes <= 64 */
  int32_t nrates;              /* columns of opt, 1 <= nrates <= 64 */
  const int64_t* set_ptr;      /* [ngroups ntimes + 1]: set v's members are [set_ptr[v], set_ptr[v + 1]) */
  const int32_t* member_row;   /* [nmembers]: rows of the solver, each in [0, nbls), repeats allowed */
  const double* member_wgt;    /* [nmembers], finite and >= 0; NULL: ones */
  const uint8_t* member_conj;  /* [nmembers], 0 or 1; NULL: none */
  int32_t weighting;           /* 0: u = omega; 1: u = omega w */
  const double* scale;         /* [ngroups][ntimes], finite; NULL: ones */
  int32_t nbins;               /* 0: no binned output */
  const int32_t* bin_of_group; /* [ngroups] in [-1, nbins); NULL iff nbins == 0 */
  const void* op_r;            /* [nfreqs][ndelays], solver dtype */
  const void* op_i;
  const double* norm_f;        /* [nfreqs] */
  const double* opt_r;         /* [ntimes][nrates], finite */
  const double* opt_i;
  int64_t nmembers;            /* 0 <= nmembers <= 2^30 */
} cal_delay_coherent_desc;
int cal_solver_delay_coherent_spectrum(cal_solver* s, const cal_delay_coherent_desc* desc, const void* g_r, const void* g_i, double* power_grp,
                                       double* norm_grp, double* power_bin, double* count_bin);
/* Host only, like cal_debug_report_plan: the plan of cal_solver_delay_coherent_spectrum for `desc` (every field is read; the operator
 * in `dtype`) under the bound scratch_bytes of cal_solver_set_delay_spectrum_scratch (0: the default), as bytes.  The selectors mirror
 * 70 .. 76 of cal_debug_report_plan --
 *   70: int64 nwhat, the row pitch of the averaged planes, the columns of the operator image, groups per chunk, chunks, the elements
 *   of the chunk's planes (dtype), of its Y and power (double), of norm_grp | power_bin | count_bin, the bytes of the chunk's set
 *   masks and the spans of a row; 71: the bins' sorted group lists; 72: [chunks][nbins][2] a bin's piece of a chunk as positions in 71;
 *   73: the operator image [re, im][pitch][columns] (dtype); 74: norm_f padded to the pitch (double); 75: the scales [ngroups][ntimes]
 *   (double; ones for NULL); 76: opt_r | opt_i (double); 77: int64 [chunks][2], the chunk's members as positions in the member arrays. */
int cal_debug_delay_coherent_plan(int dtype, const cal_problem_desc* d, const cal_delay_coherent_desc* desc, int64_t scratch_bytes, int what, void* out,
                                  int64_t cap_bytes, int64_t* bytes);
/* The signal loss of the fit in delay space: the share of the power at every delay that the coefficient fit itself removes.  The
 * foreground basis absorbs every component of the data in its span -- noise and cosmological signal as well as foregrounds -- so a
 * residual delay spectrum (cal_solver_delay_spectrum) is biased low near the edge of the basis; this is the factor that undoes it.
 * Notation of cal_solver_fit_errors and cal_solver_delay_spectrum: row b of fitting group gamma has antennas (i, j) and the basis rows
 * a_{b,f}; G = g_i conj(g_j), q = w |G|^2, mask = (w != 0);
 *   N_gamma = sum_{b in gamma} A_b^T diag(q_b) A_b    N_r = N_gamma + ridge (tr N_gamma / nvec) I    L L^T = N_r   (cal_solver_fit_errors')
 *                    calibrated = 0 (d - G m)      calibrated = 1 (d / G - m)
 *   s[b][f]     =    mask G                        mask                       (0 where |G|^2 == 0)
 *   v[b][f]     =    mask / w                      mask / q                   (0 where |G|^2 == 0)
 *   U[b][k]           = sum_f (op_r + i op_i)[f][k] s[b][f] a_{b,f}           complex, nvec numbers
 *   num[b][k]         = |L^-1 U[b][k]|^2
 *   noise_bl[b][k]    = sum_f v[b][f] |op[f][k]|^2                            [nbls][ndelays]
 *   absorbed_bl[b][k] = num / noise_bl; 0 where noise_bl == 0 or the group is singular      [nbls][ndelays], in [0, 1]
 *   absorbed_bin[n][k] = sum of absorbed_bl[b][k] over the rows b with bin_of_bl[b] == n, an unflagged sample and a factored group,
 *                        taken in ascending b                                 [nbins][ndelays]
 *   count_bin[n]      = the number of such rows (an integer, returned as a double)          [nbins]
 * Meaning: with the gains held fixed (the conditional view of cal_solver_fit_errors: a lower bound on the loss), noise of variance
 * 1 / w on the unflagged samples and the coefficients at their weighted least-squares optimum, noise_bl is the expected delay power of
 * the masked data at delay k, as cal_solver_delay_spectrum masks them, and noise_bl - num that of the masked residual -- for groups of
 * several baselines too.  Exact at ridge = 0 (a ridge only lowers num), and for any input whose variance is proportional to 1 / w:
 * 1 - absorbed_bin / count_bin is the transfer of a signal that is white in delay wherever the weights are uniform over the unflagged
 * samples.  With the unshifted rectangular DFT of all nfreqs delays, sum_k num[b][k] = nfreqs sum_f mask |G|^2 model_var[b][f].
 * The two products -- S = L^-1 A^T per run of a group's baselines, then (S diag(s_b)) op per baseline row, real times complex -- run on
 * the matrix cores in the solver's dtype (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64); the squares, noise_bl, the division and
 * every sum over vectors and rows are taken in double in a fixed order, no float atomics: two calls give the same bits.  All outputs
 * are doubles; any output pointer may be NULL (absorbed_bin and count_bin need nbins > 0).  counts (may be NULL): the groups factored
 * and the singular ones, as in cal_solver_fit_errors; the rows of a singular group and the rows without an unflagged sample are zero
 * and enter no bin.
 *   g_r, g_i: as in cal_solver_delay_spectrum -- NULL: the solver's current full gains, whatever gain bases are set; given gains are
 *   used for this call only (q and N are formed from them too).
 * Errors, before any launch: CAL_ERR_STATE when problem, data or coefficients are not set, or the gains neither set nor given;
 * CAL_ERR_INVALID for a null description, ndelays outside [1, 4096], a `calibrated` other than 0 or 1, a ridge that is negative or not
 * finite, nbins < 0, a bin_of_bl that is NULL with nbins > 0 (or given with nbins == 0) or holds an index outside [-1, nbins), a null
 * operator, binned outputs with nbins == 0.
 * Works for every layout and kernel path, folded and full tiles, fitting groups of several baselines on several row blocks, bl_alias
 * and nslices > 1.  A post-fit pass like cal_solver_fit_errors: it runs the model pass of cal_solver_model and puts the loop state
 * back; nothing a later cal_solver_run reads changes, and a run continued after the call is bit-identical to one without it.
 * The groups are worked through in chunks (heaviest first) whose scratch -- N, L^-1 and S in the solver's dtype and the factor in
 * double -- stays under the bound of cal_solver_set_delay_transfer_scratch (never less than one group).  The result does not depend on
 * the chunks by a bit.  The rows of absorbed_bl (and of noise_bl when asked for) are kept whole on the device, nbls ndelays doubles
 * each: the bins add their rows in ascending order, which is not the order of the chunks.
 * Under a communicator or exchange hook absorbed_bin | count_bin are summed over the ranks in ONE all-reduce of nbins ndelays + nbins
 * doubles (CAL_XCHG_F64, CAL_XCHG_SUM), whichever outputs are asked for (nbins == 0: none); a group belongs to one rank, so the per-row
 * outputs stay the rank's own rows. */
typedef struct cal_delay_transfer_desc {
  int32_t ndelays;          /* columns of the operator, 1 <= ndelays <= 4096 */
  int32_t calibrated;       /* 0: the loss of d - G m; 1: of d / G - m */
  int32_t nbins;            /* 0: no binned output */
  const int32_t* bin_of_bl; /* [nbls] in [-1, nbins): -1 leaves the row out; NULL iff nbins == 0 */
  const void* op_r;         /* [nfreqs][ndelays], solver dtype: the transform along frequency, taper folded in */
  const void* op_i;
  double ridge;             /* of the factorisation, as in cal_solver_fit_errors: finite, >= 0 */
} cal_delay_transfer_desc;
int cal_solver_delay_transfer(cal_solver* s, const cal_delay_transfer_desc* desc, const void* g_r, const void* g_i, double* absorbed_bl,
                              double* noise_bl, double* absorbed_bin, double* count_bin, cal_fit_errors_counts* counts);
/* The scratch bound of cal_solver_delay_transfer in bytes (0: the default, 256 MiB; negative: CAL_ERR_INVALID).  The outputs do not
 * depend on it: tests use it to send a small problem through several chunks. */
int cal_solver_set_delay_transfer_scratch(cal_solver* s, int64_t bytes);
/* Fix the gain degeneracies against a reference (sky) model after a fit (the reference computes one band-wide amplitude on the host and
 * never applies its phase).  A fit constrains only g_i conj(g_j) m_b; per slice t and channel f an amplitude eta, a phase psi and a
 * phase gradient across the array Phi = (Phi_e, Phi_n) (rad / m; a shift of the sky) are free because the model absorbs them.  Baseline
 * row b has antennas (i, j); r_a = antpos[a] (east, north, metres), d_b = r_i - r_j from the row's own (ant0, ant1) -- a row stored
 * conjugated needs nothing special, an autocorrelation row has d_b = 0; m = A c at the solver's coefficients (cal_solver_model), s =
 * ref_r + i ref_i the reference visibility, w = ref_w or, with NULL, the weight plane the solver reads now; g the given gains or the
 * solver's full gains, as in cal_solver_fit_quality.  In solver units:
 *   z0_b = w conj(m_b) s_b               products in the solver's dtype; only samples with w > 0 count, here and below
 *   Q    = sum_b w |m_b|^2               H = sum_b |z0_b| d_b d_b^T  (2 x 2, formed once)
 *   Phi  = 0;  iters times:  z_b = z0_b e^{-i Phi.d_b},  q = sum_b Im(z_b) d_b,  Phi += H^+ q
 *   e^{2 eta} = max(sum_b Re z_b, 0) / Q                      z_b at the last Phi
 *   H^+ q: the inverse where det H > 1e-12 (tr H / 2)^2; else (a linear array) the step along H's dominant eigenvector alone
 *   psi  = arg sum_a g_a e^{-i Phi.r_a} conj(gref_a)          over the antennas that have a cross-correlation row with w > 0 at f, in
 *                                                             ascending antenna order; 0 without gref
 *   m'_b = m_b e^{2 eta} e^{i Phi.d_b}                        g'_a = g_a e^{-eta} e^{-i (Phi.r_a + psi)}
 * so that g'_i conj(g'_j) m'_b = g_i conj(g_j) m_b.  The iteration is a chord method whose matrix is the Hessian at a noise-free solution:
 * it converges from tilts up to about pi / 2 on the longest baseline (1e-15 rad after 4 iterations from 1.5 rad); last_step = |H^+ q| of the
 * last iteration times the slice's longest |d_b|, in radians, tells a fit that did not settle.
 * A channel with Q = 0, tr H = 0 or sum Re z <= 0 keeps the identity (eta = psi = Phi = 0, m' = m, g' = g bit for bit) and reports 0 samples.
 * CAL_DEGEN_CHANNEL: every channel on its own.  CAL_DEGEN_BAND: one amplitude and one sky shift per slice, Phi(f) = (nu_f / nu_ref) Phi_0
 * with nu_ref the mean of freqs: q_0 = sum_f (nu_f / nu_ref) q(f), H_0 = sum_f (nu_f / nu_ref)^2 H(f), e^{2 eta} = sum_f sum_b Re z_b /
 * sum_f Q(f), over the channels with Q(f) > 0 and tr H(f) > 0 in ascending order (the others keep the identity); psi stays per channel.
 * Arithmetic: every sum over baselines, antennas and channels is taken in double in an order the problem alone decides -- a slice's rows in
 * ascending order, cut into segments of 128 rows, the segments' sums added in eight runs of neighbours, each in ascending order, and the
 * runs in ascending order; no float atomics -- so two calls give the
 * same bits and a slice of a batch the bits of the same slice alone.  sincos, the 2 x 2 solve, eta and the factors applied are in double;
 * m' and g' are rounded once to the solver's dtype.
 * Slices: t runs over nslices or, in the joint time-basis layout, over the ntimes of cal_solver_set_gain_time_basis (antenna row t Na + a is
 * slice t, antenna a); antpos holds one slice's antennas.  Works for every layout and kernel path, fitting groups of several baselines,
 * bl_alias and attached gain bases (g' is an output and need not lie in the basis).  Nothing the fit reads changes (gains, g0, y,
 * coefficients, moments, t, weights, loop state): a run continued after the call is bit-identical to one without it.
 * Device memory (counted by cal_solver_memory_bytes, kept until cal_solver_set_problem): two planes [nbls][fpad] of the solver's dtype
 * (the reference, overwritten by z0), a third when ref_w is given, 8 ceil(rows / 128) fpad doubles of partial sums, g' and gref
 * [nants][fpad] complex, and per-channel state of 14 nslices fpad doubles; m itself stays in the model planes of cal_solver_model and m'
 * overwrites it there.
 *   CAL_ERR_STATE: problem, data or coefficients not set, gains neither set nor given; a communicator or exchange hook of more than one
 *   rank (the channel sums would need an all-reduce per iteration, which is not implemented).  CAL_ERR_INVALID: a null description, an
 *   unknown mode, iters < 1, null ref_r / ref_i / antpos, CAL_DEGEN_BAND without freqs (or with a mean that is zero or not finite), a
 *   position that is not finite, half a (re, im) pair, a row that joins antennas of two slices. */
enum { CAL_DEGEN_CHANNEL = 0, CAL_DEGEN_BAND = 1 };
typedef struct cal_degeneracy_desc {
  int mode;                     /* CAL_DEGEN_CHANNEL | CAL_DEGEN_BAND */
  int32_t iters;                /* >= 1 */
  const void *ref_r, *ref_i;    /* [nbls][nfreqs], solver dtype, the solver's row order */
  const void* ref_w;            /* same shape, or NULL: the solver's weights */
  const double* antpos;         /* [nants_per_slice][2] east, north in metres */
  const double* freqs;          /* [nfreqs], needed for CAL_DEGEN_BAND */
  const void *g_r, *g_i;        /* [nants][nfreqs] or both NULL (as cal_solver_fit_quality) */
  const void *gref_r, *gref_i;  /* [nants][nfreqs] or both NULL: psi = 0 */
} cal_degeneracy_desc;
int cal_solver_fix_degeneracies(cal_solver* s, const cal_degeneracy_desc* desc,
                                double* params /* [nslices][nfreqs][4]: eta, psi, Phi_e, Phi_n */,
                                double* nsamp /* [nslices][nfreqs] samples with w > 0 */, double* last_step /* [nslices][nfreqs] */,
                                void* out_g_r, void* out_g_i /* [nants][nfreqs] */, void* out_m_r, void* out_m_i /* [nbls][nfreqs] */);
/* The coefficients of a frequency gain basis in closed form (no counterpart in the reference): the damped StefCal sweeps of
 * cal_solver_solve_gains projected on the basis g = g0 + B y of cal_solver_set_gain_basis.  With the other antennas held fixed the
 * chi-square is quadratic in one antenna's y.  num, den are exactly cal_solver_solve_gains': the model pass, then P, Q, then the
 * per-antenna sums from the OLD gains, autocorrelations left out.  For antenna row a (one antenna of one slice), g_a the solver's
 * current expanded gains, B [nfreqs][K] the attached basis:
 *   r_a[f]  = num_a[f] - den_a[f] g_a[f]                 (complex; minus half the chi-square gradient w.r.t. g_a)
 *   N_a     = B^T diag(den_a) B                          [K][K], real symmetric
 *   rhs_a   = B^T r_a                                    [K], complex
 *   (N_a + ridge (tr N_a / K) I) delta_a = rhs_a         (one factorisation, two right-hand sides: re, im)
 *   y_a    <- y_a + damping delta_a                      then gains = g0 + B y for the whole array
 * Every antenna is solved from the old gains (a Jacobi sweep); the gains are rebuilt once per sweep, after every row has been solved.
 * B = I, ridge = 0 is the update of cal_solver_solve_gains; damping = 1, ridge = 0 lands on the exact per-antenna minimiser.  Unlike
 * the per-channel sweep a channel with den = 0 of a non-singular antenna does move: the basis interpolates across it.  The sweeps
 * minimise the chi-square term alone: the "sum" regulariser is not part of them.
 * Precision: r_a is evaluated in double from the double num / den planes and rounded to the solver's dtype once; N_a and rhs_a are
 * formed and accumulated in the solver's dtype in a fixed order (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64; no atomics on reals:
 * two calls give the same bits); the Cholesky factorisation, both substitutions and the update of y run in double for both dtypes,
 * and the update is rounded once.
 * A row is singular when tr N_a <= 0 (no unflagged cross-correlation) or a pivot is <= 0 or not finite: it keeps the bits of its y and
 * counts in nsingular.  result (may be NULL) counts the antenna rows of the LAST sweep; rows of unselected slices count in neither
 * field.  Suggested values: damping = 0.5, ridge = 1e-6.
 *   nsweeps >= 1, 0 < damping <= 1, ridge >= 0 and finite (CAL_ERR_INVALID otherwise); problem, data, coefficients, gains and a
 *   frequency gain basis must be set, and reset_gain_moments needs an optimizer (CAL_ERR_STATE).  With a gain TIME basis attached the
 *   call returns CAL_ERR_UNSUPPORTED: its variables couple the times of an antenna, a joint (l, k) system that is a different solve.
 *   slice_mask: [nslices] bytes or NULL (all slices): the y rows and the gains of a slice whose byte is 0 keep their bits.
 *   reset_gain_moments = 1: the optimizer's y slots of the selected slices go back to what cal_solver_set_optimizer initialises them
 *   to (Adagrad's / Ftrl's initial_accumulator_value included).
 * g0, the y snapshot of use_min, coefficients, their slots, t and iteration counts are never touched.  Works for every K the basis
 * setter accepts, every layout and kernel path, fitting groups of several baselines, bl_alias and nslices > 1 (it reuses the model
 * pass).  The antenna rows are worked through in chunks whose scratch (N_a in the solver's dtype, plus its factor in double where
 * (K + 2) rows do not fit LDS) stays under the bound of cal_solver_set_coeff_solve_scratch; every chunk of a sweep reads the old gains.
 * Like cal_solver_solve_gains it puts the loop state back (a run continued after a call with an all-zero mask is bit-identical to one
 * without the call) and issues ONE all-reduce of 3 nants nfreqs doubles per sweep under a communicator or exchange hook: y is
 * replicated, so every rank then computes the same update, bit for bit. */
typedef struct cal_gain_coeff_solve_desc {
  int32_t nsweeps;              /* >= 1 */
  int32_t reset_gain_moments;
  double damping;               /* (0, 1] */
  double ridge;                 /* >= 0 */
  const uint8_t* slice_mask;    /* [nslices] or NULL */
} cal_gain_coeff_solve_desc;
typedef struct cal_gain_coeff_solve_result { int32_t nsolved; int32_t nsingular; } cal_gain_coeff_solve_result; /* antenna rows of the last sweep */
int cal_solver_solve_gain_coeffs(cal_solver* s, const cal_gain_coeff_solve_desc* desc, cal_gain_coeff_solve_result* result);
/* Damped StefCal sweeps taken jointly over the times of a fit with a gain TIME basis (cal_solver_set_gain_time_basis),
 *   g[t] = g0[t] + sum_l Bt[t,l] z_l,   z_l = B y_l with a frequency basis, y_l without one.
 * State: nslices <= 1, nants = T Na, row t Na + a is antenna a at time t; y is [Na][L][W] complex, W = kpad with a frequency basis and
 * fpad without.  num, den are cal_solver_solve_gains' per-row sums from the OLD gains, autocorrelations left out (the model pass, P, Q,
 * the per-antenna sums, the all-reduce of 3 nants nfreqs doubles under a communicator or hook), r[row][f] = num - den g in double.
 * With a frequency basis (n = L K, index l K + k), M_{t,a} = B^T diag(den_{t,a}) B exactly as cal_solver_solve_gain_coeffs forms it:
 *   N_a[(l,k),(l',k')] = sum_t Bt[t,l] Bt[t,l'] M_{t,a}[k,k']          rhs_a[(l,k)] = sum_t Bt[t,l] (B^T r_{t,a})[k]
 *   (N_a + ridge (tr N_a / n) I) delta_a = rhs_a                        y_a <- y_a + damping delta_a
 * Every antenna is solved from the old gains (a Jacobi sweep); the gains are rebuilt once per sweep.  An antenna is singular when
 * tr N_a <= 0 (no unflagged cross-correlation at any time) or a pivot is <= 0 or not finite: it keeps the bits of its y and of its
 * gains.  An antenna flagged wholly at some times but not all IS solved, and its gains at the flagged times move: the time basis
 * interpolates; the same holds for a flagged channel.
 * Without a frequency basis the system decouples per (antenna, channel), L x L each, everything in double from the double planes:
 *   N_{a,f}[l,l'] = sum_t Bt[t,l] Bt[t,l'] den[t,a,f]                   rhs_{a,f}[l] = sum_t Bt[t,l] r[t,a,f]
 *   (N_{a,f} + ridge (tr N_{a,f} / L) I) delta = rhs                    y[a][:][f] <- y[a][:][f] + damping delta
 * and a system with tr <= 0 or a bad pivot keeps the bits of y[a][:][f].
 * result (may be NULL) counts the systems of the LAST sweep: antennas with a frequency basis, (antenna, channel) pairs without one.
 * T = 1, Bt = [[1]] with a frequency basis gives the bits of cal_solver_solve_gain_coeffs on a solver without the time basis;
 * Bt = I, ridge = 0 is its sweep per time (with a ridge they differ: the joint trace runs over all times); damping = 1, ridge = 0
 * lands on the exact per-antenna minimiser.  The "sum" regulariser is not part of the sweeps.
 * Precision: M_{t,a} and B^T r are in the solver's dtype; the sums over t run in double in ascending t and are rounded to the dtype once
 * on store; the factorisation, the substitutions and the update of y run in double, the update is rounded once.  Every sum of reals has
 * a fixed order, atomics only on the two integer counters: two calls give the same bits.  Suggested: damping = 0.5, ridge = 1e-6.
 *   nsweeps >= 1, 0 < damping <= 1, ridge >= 0 and finite (CAL_ERR_INVALID otherwise); problem, data, coefficients, gains and a gain
 *   time basis must be set, and reset_gain_moments needs an optimizer (CAL_ERR_STATE).
 *   reset_gain_moments = 1: the optimizer's y slots go back to what cal_solver_set_optimizer leaves there.
 * g0, the y snapshot of use_min, coefficients, their slots, t and iteration counts are never touched; the loop state is put back around
 * the model pass.  The antennas are worked in chunks whose buffers (the M, N_a, the factor where it leaves LDS, or the channel scratch
 * beyond 8 time vectors) stay under the bound of cal_solver_set_coeff_solve_scratch, never less than one antenna; every chunk of a sweep
 * reads the old gains.  There is no slice mask: it is one joint fit. */
typedef struct cal_gain_time_solve_desc {
  int32_t nsweeps;              /* >= 1 */
  int32_t reset_gain_moments;
  double damping;               /* (0, 1] */
  double ridge;                 /* >= 0 */
} cal_gain_time_solve_desc;
typedef struct cal_gain_time_solve_result { int32_t nsolved; int32_t nsingular; } cal_gain_time_solve_result; /* systems of the last sweep */
int cal_solver_solve_gain_time_coeffs(cal_solver* s, const cal_gain_time_solve_desc* desc, cal_gain_time_solve_result* result);
/* The optimizer's slots of a fit with a gain basis, read only (cal_solver_get_moments / cal_solver_set_moments stay refused there:
 * this is no checkpoint): ym_*, yv_* the first and second slot of y in the shape of cal_solver_get_gain_coeffs, cm_*, cv_* those of
 * the coefficients [ncoeffs], t [nslices] every slice's own count of applied updates.  Any pointer may be NULL.  CAL_ERR_STATE without
 * a gain basis or without an optimizer. */
int cal_solver_get_gain_coeff_moments(cal_solver* s, void* ym_r, void* ym_i, void* yv_r, void* yv_i, void* cm_r, void* cm_i, void* cv_r,
                                      void* cv_i, int64_t* t);
/* tensorize_fg_coeffs, calibration.py:828-913: per group least squares of src on the basis with samples of zero
 * weight zeroed; the result becomes the current coefficients.  src_*: [nbls][nfreqs] real. */
int cal_solver_init_coeffs(cal_solver* s, const void* src_r, const void* src_i);

int cal_solver_synchronize(cal_solver* s);
/* How cal_solver_run issues a train step (cal_launch_mode).  Every mode computes the same numbers, bit for bit: the python
 * loop of calibration.py:699-717 pays a host synchronisation per step (:701); here the choice is only how many launches a
 * step costs. */
int cal_solver_set_launch_mode(cal_solver* s, int mode);
int cal_solver_timing_enable(cal_solver* s, int enable);
int cal_solver_timing_get(cal_solver* s, cal_kernel_timing* out);
int cal_solver_memory_bytes(cal_solver* s, int64_t* device_bytes);

/* Baseline-sharded data parallelism (no counterpart in the reference, which is single-device,
 * calibration.py:1796-1804): one process per GPU, one RCCL all-reduce of the per-antenna gain gradients and the
 * loss scalars per step.  id: CAL_COMM_ID_BYTES bytes produced on rank 0 and shared out of band. */
#define CAL_COMM_ID_BYTES 128
int cal_comm_unique_id(void* id_out);
int cal_solver_comm_init(cal_solver* s, const void* id, int rank, int nranks);
/* The same exchange through a transport of the caller's (MPI, gloo, ...; and the vehicle of the two-ranks-on-one-GPU tests:
 * RCCL refuses two ranks on one device).  Wherever the library would call ncclAllReduce -- the set-up agreement, the gain
 * gradients and the loss scalars of every step -- it drains its stream, hands the callback the SAME buffer and element
 * count staged in pinned host memory, and expects it reduced in place over the nranks callers (0 = success), then copies it
 * back.  Replaces a communicator of cal_solver_comm_init and vice versa; fn = NULL detaches. */
enum cal_exchange_dtype { CAL_XCHG_F32 = 0, CAL_XCHG_F64 = 1, CAL_XCHG_I32 = 2 };
enum cal_exchange_op { CAL_XCHG_SUM = 0, CAL_XCHG_MIN = 1 };
typedef int (*cal_exchange_fn)(void* ctx, void* host_buf, int64_t count, int dtype, int op);
int cal_solver_set_exchange_hook(cal_solver* s, cal_exchange_fn fn, void* ctx, int rank, int nranks);
/* How many ranks take part in the solver's exchange, COUNTED by the exchange itself: every rank adds 1 in an all-reduce over the
 * communicator / hook (1 without either).  A launcher's rank count is a claim; this is what the data path sees (bench.py reports it). */
int cal_solver_comm_size(cal_solver* s, int* nranks_seen);

/* Gains that are smooth in frequency WHILE they are fitted (no counterpart in the reference, whose gains are free per channel,
 * calibration.py:596-599):  g_a(f) = g0_a(f) + sum_k B(f, k) y_a(k)  with one real basis B shared by every antenna and time
 * slice.  g0 are the gains the solver holds when the basis is set (or is given afterwards: cal_solver_set_params with gains sets
 * g0 to them and y to 0), so the fit starts exactly where the per-channel fit starts and only the CORRECTION lies in span(B).
 * The optimizer's gain variables are y_r, y_i [nants][nvec] (chain rule: grad y = grad g @ B); loss, coefficients and loop
 * semantics are unchanged, use_min snapshots y.  Under a communicator or exchange hook the PROJECTED gradient is exchanged:
 * planes x 2 nants kpad reals per step instead of planes x 2 nants fpad, kpad = nvec rounded up to a multiple of 8 (planes = 3
 * with the "sum" regulariser on the general kernels, else 1).
 *   basis: real (solver dtype) [nfreqs][nvec] row-major, 1 <= nvec <= nfreqs; call after set_problem (a new problem detaches
 *   the basis).  Moments and t are zeroed as by set_optimizer.  nvec = 0 detaches: the fit is per channel again, from the gains
 *   as they stand.
 * cal_solver_get_params keeps returning the full gains [nants][nfreqs]; cal_solver_eval_grads the per-channel gradient.
 * While a basis is set: the optimizer LAMB (set_optimizer / set_gain_basis) and cal_solver_get_moments / set_moments
 * (checkpoint / resume) fail with CAL_ERR_UNSUPPORTED; a train step always runs kernel by kernel (CAL_LAUNCH_ONE_TAIL falls
 * back to that form; CAL_LAUNCH_GRAPH replays the kernel-by-kernel step, the two basis kernels included). */
int cal_solver_set_gain_basis(cal_solver* s, const void* basis, int32_t nvec);
/* y [nants][nvec] real each; which as in cal_solver_get_params.  While a time basis is set (cal_solver_set_gain_time_basis):
 * [Na][L][nvec], or [Na][L][nfreqs] without a frequency basis */
int cal_solver_get_gain_coeffs(cal_solver* s, int which, void* y_r, void* y_i);
/* loss and its gradient with respect to y (the projected gain gradient): gy_* [nants][nvec] (parity tests); while a time basis
 * is set the gradient contracted over the times as well, in the shape cal_solver_get_gain_coeffs then has */
int cal_solver_eval_gain_coeff_grads(cal_solver* s, double* loss, void* gy_r, void* gy_i);

/* Gains that are smooth in TIME while they are fitted.  The solver holds T time slices as ONE fit with one loop state (nslices <= 1,
 * nants = T Na, antenna a at time t is row t Na + a: what distributed.batch_time_slices(per_slice=False) builds) and
 *   g[t Na + a](f) = g0[t Na + a](f) + sum_l Bt(t, l) z_a,l(f),    Bt real [T][L], 1 <= L <= T,
 *   z_a,l(f) = sum_k B(f, k) y_a(l, k) while a frequency basis is set too, y_a(l, f) without one (free per channel, smooth in time).
 * The optimizer's gain variables are y_r, y_i [Na][L][W], W = kpad or fpad on the device, nvec or nfreqs at this interface.  Chain
 * rule: grad y_a(l, .) = sum_t Bt(t, l) p[t Na + a](.), p the (frequency-projected) gain-gradient row, and the same for every plane.
 * Loss, coefficients and loop semantics are unchanged; use_min snapshots y.  Under a communicator or exchange hook the
 * time-projected planes are exchanged: planes x 2 Na L W reals per step (plus the loss scalars as before), W = kpad with a frequency
 * basis, else fpad.
 *   basis_t: real (solver dtype) [ntimes][nvec_t] row-major; call after set_problem.  Independent of cal_solver_set_gain_basis and
 *   callable in either order: each setter sets g0 := the current gains, y := 0 and zeroes moments and t.  nvec_t = 0 detaches the
 *   time basis only; a new set_problem detaches both.  A setter (this one or cal_solver_set_gain_basis) that fails half way, in an
 *   allocation or a copy, detaches BOTH bases before it returns the error: the fit is per channel from the gains as they stand.
 * Fails with CAL_ERR_UNSUPPORTED for a solver of several slices (nslices > 1) and for LAMB (here and in set_optimizer), with
 * CAL_ERR_INVALID when nants % ntimes != 0, nvec_t > ntimes or the basis has a non-finite entry.  While it is set,
 * cal_solver_get_moments / set_moments fail with CAL_ERR_UNSUPPORTED, cal_solver_get_gain_coeffs and
 * cal_solver_eval_gain_coeff_grads return [Na][L][nvec] (or [Na][L][nfreqs]), get_params and eval_grads are unchanged, and a train
 * step runs kernel by kernel as with the frequency basis (CAL_LAUNCH_GRAPH replays that step, the time kernels included). */
int cal_solver_set_gain_time_basis(cal_solver* s, const void* basis_t, int32_t ntimes, int32_t nvec_t);

#ifdef __cplusplus
}
#endif
#endif /* CALAMITY_HIP_H */
