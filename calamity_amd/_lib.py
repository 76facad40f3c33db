"""ctypes binding of libcalamity_hip.so (include/calamity_hip.h).  No torch, no TensorFlow.

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C calamity_amd/csrc``.  Loading fails loudly
when it is missing: the product has no CPU fallback.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libcalamity_hip.so")  # the one shipped build; experiment harnesses (tools/) assign this attribute before load()

CAL_F32, CAL_F64 = 0, 1
CAL_OPT_ADAM, CAL_OPT_ADAMAX, CAL_OPT_SGD, CAL_OPT_RMSPROP, CAL_OPT_ADAGRAD, CAL_OPT_NADAM, CAL_OPT_ADADELTA, CAL_OPT_FTRL, CAL_OPT_LAMB = range(9)
CAL_REG_NONE, CAL_REG_SUM = 0, 1
CAL_LAYOUT_STREAM, CAL_LAYOUT_SHARED = 0, 1
CAL_PATH_AUTO, CAL_PATH_GENERAL, CAL_PATH_DENSE, CAL_PATH_DENSE_F32, CAL_PATH_DENSE_SPLIT1, CAL_PATH_GENERAL_FULL = 0, 1, 2, 3, 4, 5
CAL_LAUNCH_AUTO, CAL_LAUNCH_KERNELS, CAL_LAUNCH_ONE_TAIL, CAL_LAUNCH_GRAPH = 0, 1, 2, 3
CAL_COMM_ID_BYTES = 128
CAL_MAX_SLICES = 256
CAL_ERR_INVALID, CAL_ERR_STATE, CAL_ERR_UNSUPPORTED, CAL_ERR_NONFINITE = -1, -4, -5, -6


class ProblemDesc(C.Structure):
    _fields_ = [
        ("nants", C.c_int32),
        ("nfreqs", C.c_int32),
        ("ngrps", C.c_int32),
        ("nbls", C.c_int32),
        ("nbasis", C.c_int32),
        ("basis_offset", C.c_void_p),
        ("basis_nvec", C.c_void_p),
        ("basis_nrowblk", C.c_void_p),
        ("basis_data", C.c_void_p),
        ("grp_basis", C.c_void_p),
        ("grp_bl_start", C.c_void_p),
        ("bl_ant0", C.c_void_p),
        ("bl_ant1", C.c_void_p),
        ("bl_rowblk", C.c_void_p),
        ("layout", C.c_int32),
        ("kernel_path", C.c_int32),
        ("bl_alias", C.c_void_p),
        ("nslices", C.c_int32),
        ("reserved", C.c_int32),
        ("grp_var", C.c_void_p),
    ]


class OptimizerDesc(C.Structure):
    _fields_ = [
        ("optimizer", C.c_int32),
        ("learning_rate", C.c_double),
        ("beta_1", C.c_double),
        ("beta_2", C.c_double),
        ("epsilon", C.c_double),
        ("rho", C.c_double),
        ("momentum", C.c_double),
        ("initial_accumulator_value", C.c_double),
        ("nesterov", C.c_int32),
        ("reserved", C.c_int32),
        ("learning_rate_power", C.c_double),
        ("l1_regularization_strength", C.c_double),
        ("l2_regularization_strength", C.c_double),
        ("l2_shrinkage_regularization_strength", C.c_double),
        ("beta", C.c_double),
        ("weight_decay_rate", C.c_double),
    ]


class RunDesc(C.Structure):
    _fields_ = [
        ("nsteps", C.c_int32),
        ("record", C.c_int32),
        ("use_min", C.c_int32),
        ("freeze_model", C.c_int32),
        ("tol", C.c_double),
    ]


class GainSolveDesc(C.Structure):
    _fields_ = [("nsweeps", C.c_int32), ("reset_gain_moments", C.c_int32), ("damping", C.c_double), ("slice_mask", C.c_void_p)]


class RobustDesc(C.Structure):
    """cal_robust_desc: kind (ROBUST_KINDS), threshold k in sigma, slice_mask [nslices] bytes or NULL.  With w0 the weights of set_data:
    e = w0 |d - g_i conj(g_j) (A c)|^2, med_b the ((n_b + 1) // 2)-th smallest e over the row's samples with w0 > 0, scale_b = med_b / ln 2,
    z2 = e / scale_b; huber psi = 1 if z2 <= k^2 else k / sqrt(z2), cauchy psi = 1 / (1 + z2 / k^2), clip psi = 1 if z2 <= k^2 else 0;
    w = w0 psi (include/calamity_hip.h: cal_solver_robust_weights)."""
    _fields_ = [("kind", C.c_int), ("threshold", C.c_double), ("slice_mask", C.c_void_p)]


ROBUST_KINDS = {"none": 0, "huber": 1, "cauchy": 2, "clip": 3}


class DelaySpectrumDesc(C.Structure):
    """cal_delay_spectrum_desc (include/calamity_hip.h: cal_solver_delay_spectrum): ndelays columns of the operator op_r + i op_i
    ([nfreqs][ndelays], solver dtype), what (DELAY_SPECTRUM_WHAT bits), calibrated 0 / 1, nbins and bin_of_bl [nbls] int32 in
    [-1, nbins) (NULL iff nbins == 0), norm_f [nfreqs] float64."""
    _fields_ = [("ndelays", C.c_int32), ("what", C.c_int32), ("calibrated", C.c_int32), ("nbins", C.c_int32), ("bin_of_bl", C.c_void_p),
                ("op_r", C.c_void_p), ("op_i", C.c_void_p), ("norm_f", C.c_void_p)]


DELAY_SPECTRUM_WHAT = {"data": 1, "model": 2, "resid": 4}


DELAY_CROSS_STATS = {"cross": 1, "diff": 2}


class DelayCrossDesc(C.Structure):
    """cal_delay_cross_desc (include/calamity_hip.h: cal_solver_delay_cross_spectrum): ndelays, what and calibrated as in
    DelaySpectrumDesc; npairs, pairs [npairs][2] int32 (rows of the solver), scale [npairs][2] float64 (NULL: ones), stats
    (DELAY_CROSS_STATS bits), nbins and bin_of_pair [npairs] int32 in [-1, nbins) (NULL iff nbins == 0), the operator and norm_f."""
    _fields_ = [("ndelays", C.c_int32), ("what", C.c_int32), ("calibrated", C.c_int32), ("npairs", C.c_int32), ("pairs", C.c_void_p),
                ("scale", C.c_void_p), ("stats", C.c_int32), ("nbins", C.c_int32), ("bin_of_pair", C.c_void_p), ("op_r", C.c_void_p),
                ("op_i", C.c_void_p), ("norm_f", C.c_void_p)]


class DelayFringeDesc(C.Structure):
    """cal_delay_fringe_desc (include/calamity_hip.h: cal_solver_delay_fringe_spectrum): ndelays, what and calibrated as in
    DelaySpectrumDesc; ngroups, ntimes, nrates, rows [ngroups][ntimes] int32 (rows of the solver), scale [ngroups][ntimes] float64
    (NULL: ones), nbins and bin_of_group [ngroups] int32 in [-1, nbins) (NULL iff nbins == 0), the operator and norm_f, and the
    transform along time opt_r, opt_i [ntimes][nrates] float64."""
    _fields_ = [("ndelays", C.c_int32), ("what", C.c_int32), ("calibrated", C.c_int32), ("ngroups", C.c_int32), ("ntimes", C.c_int32),
                ("nrates", C.c_int32), ("rows", C.c_void_p), ("scale", C.c_void_p), ("nbins", C.c_int32), ("bin_of_group", C.c_void_p),
                ("op_r", C.c_void_p), ("op_i", C.c_void_p), ("norm_f", C.c_void_p), ("opt_r", C.c_void_p), ("opt_i", C.c_void_p)]


class DelayCoherentDesc(C.Structure):
    """cal_delay_coherent_desc (include/calamity_hip.h: cal_solver_delay_coherent_spectrum): the fields of DelayFringeDesc with ``rows``
    replaced by the ragged sets -- set_ptr [ngroups ntimes + 1] int64, member_row [nmembers] int32, member_wgt [nmembers] float64 (NULL:
    ones), member_conj [nmembers] uint8 (NULL: none), weighting 0 / 1 -- and nmembers at the end."""
    _fields_ = [("ndelays", C.c_int32), ("what", C.c_int32), ("calibrated", C.c_int32), ("ngroups", C.c_int32), ("ntimes", C.c_int32),
                ("nrates", C.c_int32), ("set_ptr", C.c_void_p), ("member_row", C.c_void_p), ("member_wgt", C.c_void_p), ("member_conj", C.c_void_p),
                ("weighting", C.c_int32), ("scale", C.c_void_p), ("nbins", C.c_int32), ("bin_of_group", C.c_void_p), ("op_r", C.c_void_p),
                ("op_i", C.c_void_p), ("norm_f", C.c_void_p), ("opt_r", C.c_void_p), ("opt_i", C.c_void_p), ("nmembers", C.c_int64)]


class DelayTransferDesc(C.Structure):
    """cal_delay_transfer_desc (include/calamity_hip.h: cal_solver_delay_transfer): ndelays columns of the operator op_r + i op_i
    ([nfreqs][ndelays], solver dtype), calibrated 0 / 1, nbins and bin_of_bl [nbls] int32 in [-1, nbins) (NULL iff nbins == 0), the
    ridge of the factorisation (cal_solver_fit_errors')."""
    _fields_ = [("ndelays", C.c_int32), ("calibrated", C.c_int32), ("nbins", C.c_int32), ("bin_of_bl", C.c_void_p), ("op_r", C.c_void_p),
                ("op_i", C.c_void_p), ("ridge", C.c_double)]


class DegeneracyDesc(C.Structure):
    """cal_degeneracy_desc (include/calamity_hip.h: cal_solver_fix_degeneracies): mode (DEGENERACY_MODES), iters >= 1, the reference
    planes ref_r, ref_i and their weights ref_w (NULL: the solver's) [nbls][nfreqs] in the solver's dtype, antpos [nants per slice][2]
    and freqs [nfreqs] float64, the gains g and the reference gains gref [nants][nfreqs] (each pair may be NULL)."""
    _fields_ = [("mode", C.c_int), ("iters", C.c_int32), ("ref_r", C.c_void_p), ("ref_i", C.c_void_p), ("ref_w", C.c_void_p),
                ("antpos", C.c_void_p), ("freqs", C.c_void_p), ("g_r", C.c_void_p), ("g_i", C.c_void_p), ("gref_r", C.c_void_p),
                ("gref_i", C.c_void_p)]


DEGENERACY_MODES = {"channel": 0, "band": 1}


class ReportPlanDesc(C.Structure):
    """cal_report_plan_desc (include/calamity_hip.h: cal_debug_report_plan): the call whose host plan is asked for -- a spectrum
    description with its scratch bound and whether power_bl is wanted, a degeneracy description with the number of slices
    (0: the problem's), or a transfer description with its scratch bound."""
    _fields_ = [("spectrum", C.POINTER(DelaySpectrumDesc)), ("degeneracy", C.POINTER(DegeneracyDesc)), ("scratch_bytes", C.c_int64),
                ("with_power_bl", C.c_int32), ("nslices", C.c_int32), ("transfer", C.POINTER(DelayTransferDesc))]


class CrossReportPlanDesc(ReportPlanDesc):
    """cal_report_plan_desc with its last field, read for the selectors 60 .. 65 only: a cross description, planned under scratch_bytes
    (the spectrum's bound)."""
    _fields_ = [("cross", C.POINTER(DelayCrossDesc))]


class FringeReportPlanDesc(CrossReportPlanDesc):
    """cal_report_plan_desc with its last field, read for the selectors 70 .. 76 only: a fringe description, planned under
    scratch_bytes (the spectrum's bound)."""
    _fields_ = [("fringe", C.POINTER(DelayFringeDesc))]


class CoeffSolveDesc(C.Structure):
    _fields_ = [("niters", C.c_int32), ("reset_coeff_moments", C.c_int32), ("damping", C.c_double), ("ridge", C.c_double), ("slice_mask", C.c_void_p)]


class CoeffSolveResult(C.Structure):
    _fields_ = [("nsolved", C.c_int32), ("nsingular", C.c_int32)]


class FitErrorsCounts(C.Structure):
    _fields_ = [("nsolved", C.c_int32), ("nsingular", C.c_int32)]


class GainCoeffSolveDesc(C.Structure):
    _fields_ = [("nsweeps", C.c_int32), ("reset_gain_moments", C.c_int32), ("damping", C.c_double), ("ridge", C.c_double), ("slice_mask", C.c_void_p)]


class GainCoeffSolveResult(C.Structure):
    _fields_ = [("nsolved", C.c_int32), ("nsingular", C.c_int32)]


class GainTimeSolveDesc(C.Structure):
    _fields_ = [("nsweeps", C.c_int32), ("reset_gain_moments", C.c_int32), ("damping", C.c_double), ("ridge", C.c_double)]


class GainTimeSolveResult(C.Structure):
    _fields_ = [("nsolved", C.c_int32), ("nsingular", C.c_int32)]


class GaussNewtonDesc(C.Structure):
    """cal_gauss_newton_desc: at most ``ncg`` iterations of conjugate gradients on (N + lambda_t D) p = rhs per slice, stopped at
    sqrt(rz / rz0) <= cg_tol; lambda [nslices] doubles, slice_mask [nslices] bytes or NULL (include/calamity_hip.h)."""
    _fields_ = [("ncg", C.c_int32), ("reset_moments", C.c_int32), ("cg_tol", C.c_double), ("lambda", C.c_void_p), ("slice_mask", C.c_void_p)]


class GaussNewtonResult(C.Structure):
    _fields_ = [("loss_before", C.c_double), ("loss_after", C.c_double), ("cg_residual", C.c_double), ("cg_iters", C.c_int32), ("accepted", C.c_int32)]


class LbfgsDesc(C.Structure):
    """cal_lbfgs_desc: ``nsteps`` iterations of L-BFGS with ``history`` stored pairs and a backtracking Armijo search of at most
    ``max_ls`` trials (``c1``, ``shrink``); slice_mask [nslices] bytes or NULL (include/calamity_hip.h)."""
    _fields_ = [("nsteps", C.c_int32), ("history", C.c_int32), ("max_ls", C.c_int32), ("freeze_model", C.c_int32), ("reset_moments", C.c_int32),
                ("reserved", C.c_int32), ("c1", C.c_double), ("shrink", C.c_double), ("ftol", C.c_double), ("curvature_eps", C.c_double),
                ("slice_mask", C.c_void_p)]


class LbfgsResult(C.Structure):
    _fields_ = [("loss_before", C.c_double), ("loss_after", C.c_double), ("iters", C.c_int32), ("evals", C.c_int32), ("pairs_dropped", C.c_int32),
                ("status", C.c_int32)]


class MixedCompsDesc(C.Structure):
    """cal_mixed_comps_desc (include/calamity_hip.h: cal_mixed_comps_create): grp_bl_start [ngroups + 1] int32 into uvw [.][3] float64,
    freqs [nfreqs] float64, grp_freq_start NULL (every group has all channels) or [ngroups + 1] int32 into freqs, the four parameters of
    simple_cov_matrix, tol > 0, the scratch bound in bytes (0: 256 MiB)."""
    _fields_ = [("ngroups", C.c_int32), ("nfreqs", C.c_int32), ("grp_bl_start", C.c_void_p), ("uvw", C.c_void_p), ("freqs", C.c_void_p),
                ("grp_freq_start", C.c_void_p), ("ant_dly", C.c_double), ("horizon", C.c_double), ("offset", C.c_double), ("min_dly", C.c_double), ("tol", C.c_double),
                ("scratch_bytes", C.c_int64)]


MIXED_COMPS_STATUS = ("ok", "rank cap", "not run")


class RunResult(C.Structure):
    _fields_ = [("nrecorded", C.c_int32), ("stopped", C.c_int32), ("nupdates", C.c_int32), ("nonfinite", C.c_int32)]


class KernelTiming(C.Structure):
    _fields_ = [
        ("launches", C.c_int64),
        ("total_ms", C.c_double),
        ("algorithmic_bytes_per_launch", C.c_double),
        ("basis_bytes_per_launch", C.c_double),
        ("flops_per_launch", C.c_double),
        ("kernel_path", C.c_int32),
        ("dense_wg_per_cu", C.c_int32),
        ("basis_folded", C.c_int32),
        ("reserved", C.c_int32),
    ]


# every symbol include/calamity_hip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "cal_last_error": (C.c_char_p, []),
    "cal_version": (C.c_char_p, []),
    "cal_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "cal_basis_foldable": (C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "cal_debug_plan": (C.c_int, [C.c_int, C.POINTER(ProblemDesc), C.c_int, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "cal_debug_solve_plan": (C.c_int, [C.c_int, C.POINTER(ProblemDesc), C.c_int64, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "cal_debug_delay_coherent_plan": (C.c_int, [C.c_int, C.POINTER(ProblemDesc), C.POINTER(DelayCoherentDesc), C.c_int64, C.c_int, _P, C.c_int64,
                                               C.POINTER(C.c_int64)]),
    "cal_debug_report_plan": (C.c_int, [C.c_int, C.POINTER(ProblemDesc), C.POINTER(ReportPlanDesc), C.c_int, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "cal_debug_step_shape": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "cal_device_info": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "cal_device_stream_peak": (C.c_int, [C.c_int, C.c_size_t, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "cal_device_busy_clock_mhz": (C.c_int, [C.c_int, C.POINTER(C.c_double)]),
    "cal_solver_create": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int]),
    "cal_solver_destroy": (C.c_int, [_P]),
    "cal_solver_set_problem": (C.c_int, [_P, C.POINTER(ProblemDesc)]),
    "cal_solver_set_data": (C.c_int, [_P, _P, _P, _P]),
    "cal_solver_set_regularization": (C.c_int, [_P, C.c_int, C.c_double, C.c_double]),
    "cal_solver_set_regularization_slices": (C.c_int, [_P, C.c_int, _P, _P]),
    "cal_solver_set_optimizer": (C.c_int, [_P, C.POINTER(OptimizerDesc)]),
    "cal_solver_set_params": (C.c_int, [_P, _P, _P, _P, _P]),
    "cal_solver_get_params": (C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    "cal_solver_get_moments": (C.c_int, [_P] + [_P] * 8 + [C.POINTER(C.c_int64)]),
    "cal_solver_set_moments": (C.c_int, [_P] + [_P] * 8 + [C.c_int64]),
    "cal_solver_eval_loss": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "cal_solver_eval_grads": (C.c_int, [_P, C.POINTER(C.c_double), _P, _P, _P, _P]),
    "cal_solver_get_slice_losses": (C.c_int, [_P, _P]),
    "cal_solver_run": (C.c_int, [_P, C.POINTER(RunDesc), _P, C.POINTER(RunResult)]),
    "cal_solver_run_slices": (C.c_int, [_P, C.POINTER(RunDesc), _P, C.POINTER(RunResult)]),
    "cal_solver_model": (C.c_int, [_P, _P, _P]),
    "cal_solver_data_model": (C.c_int, [_P, _P, _P]),
    "cal_solver_fit_quality": (C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "cal_solver_solve_gains": (C.c_int, [_P, C.POINTER(GainSolveDesc)]),
    "cal_solver_hold_slices": (C.c_int, [_P, _P]),
    "cal_solver_normal_product": (C.c_int, [_P] + [_P] * 8),
    "cal_solver_gauss_newton_step": (C.c_int, [_P, C.POINTER(GaussNewtonDesc), C.POINTER(GaussNewtonResult)]),
    "cal_solver_lbfgs": (C.c_int, [_P, C.POINTER(LbfgsDesc), _P, C.POINTER(LbfgsResult)]),
    "cal_debug_lbfgs_coefficients": (C.c_int, [C.c_int32, _P, _P, C.POINTER(C.c_double)]),
    "cal_solver_robust_weights": (C.c_int, [_P, C.POINTER(RobustDesc), _P, _P]),
    "cal_solver_delay_spectrum": (C.c_int, [_P, C.POINTER(DelaySpectrumDesc), _P, _P, _P, _P, _P, _P]),
    "cal_solver_set_delay_spectrum_scratch": (C.c_int, [_P, C.c_int64]),
    "cal_solver_delay_cross_spectrum": (C.c_int, [_P, C.POINTER(DelayCrossDesc), _P, _P, _P, _P, _P, _P, _P, _P]),
    "cal_solver_delay_fringe_spectrum": (C.c_int, [_P, C.POINTER(DelayFringeDesc), _P, _P, _P, _P, _P, _P]),
    "cal_solver_delay_coherent_spectrum": (C.c_int, [_P, C.POINTER(DelayCoherentDesc), _P, _P, _P, _P, _P, _P]),
    "cal_solver_delay_transfer": (C.c_int, [_P, C.POINTER(DelayTransferDesc), _P, _P, _P, _P, _P, _P, C.POINTER(FitErrorsCounts)]),
    "cal_solver_set_delay_transfer_scratch": (C.c_int, [_P, C.c_int64]),
    "cal_solver_fix_degeneracies": (C.c_int, [_P, C.POINTER(DegeneracyDesc), _P, _P, _P, _P, _P, _P, _P]),
    "cal_solver_get_weights": (C.c_int, [_P, _P, C.c_int]),
    "cal_solver_solve_coeffs": (C.c_int, [_P, C.POINTER(CoeffSolveDesc), C.POINTER(CoeffSolveResult)]),
    "cal_solver_set_coeff_solve_scratch": (C.c_int, [_P, C.c_int64]),
    "cal_solver_fit_errors": (C.c_int, [_P, C.c_double, _P, _P, _P, _P, _P, C.POINTER(FitErrorsCounts)]),
    "cal_solver_gain_basis_errors": (C.c_int, [_P, C.c_double, _P, _P, _P, C.POINTER(FitErrorsCounts)]),
    "cal_solver_solve_gain_coeffs": (C.c_int, [_P, C.POINTER(GainCoeffSolveDesc), C.POINTER(GainCoeffSolveResult)]),
    "cal_solver_solve_gain_time_coeffs": (C.c_int, [_P, C.POINTER(GainTimeSolveDesc), C.POINTER(GainTimeSolveResult)]),
    "cal_solver_get_gain_coeff_moments": (C.c_int, [_P] + [_P] * 8 + [C.POINTER(C.c_int64)]),
    "cal_weighted_square_error": (C.c_int, [C.c_int, C.c_int, C.c_int64, _P, _P, _P, _P, _P, C.POINTER(C.c_double)]),
    "cal_mixed_comps_create": (C.c_int, [C.POINTER(_P), C.c_int, C.POINTER(MixedCompsDesc)]),
    "cal_mixed_comps_destroy": (C.c_int, [_P]),
    "cal_mixed_comps_info": (C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "cal_mixed_comps_gram": (C.c_int, [_P, _P, C.c_int64]),
    "cal_mixed_comps_vectors": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.POINTER(C.c_double)]),
    "cal_mixed_comps_factor": (C.c_int, [_P, C.c_int32, _P, _P]),
    "cal_simple_cov_matrix": (C.c_int, [C.c_int, C.c_int32, _P, C.c_int32, _P, C.c_double, C.c_double, C.c_double, C.c_double, _P]),
    "cal_solver_init_coeffs": (C.c_int, [_P, _P, _P]),
    "cal_solver_synchronize": (C.c_int, [_P]),
    "cal_solver_set_launch_mode": (C.c_int, [_P, C.c_int]),
    "cal_solver_timing_enable": (C.c_int, [_P, C.c_int]),
    "cal_solver_timing_get": (C.c_int, [_P, C.POINTER(KernelTiming)]),
    "cal_solver_memory_bytes": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "cal_comm_unique_id": (C.c_int, [_P]),
    "cal_solver_comm_init": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "cal_solver_set_exchange_hook": (C.c_int, [_P, _P, _P, C.c_int, C.c_int]),
    "cal_solver_comm_size": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "cal_solver_set_gain_basis": (C.c_int, [_P, _P, C.c_int32]),
    "cal_solver_set_gain_time_basis": (C.c_int, [_P, _P, C.c_int32, C.c_int32]),
    "cal_solver_get_gain_coeffs": (C.c_int, [_P, C.c_int, _P, _P]),
    "cal_solver_eval_gain_coeff_grads": (C.c_int, [_P, C.POINTER(C.c_double), _P, _P]),
}

EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int)  # cal_exchange_fn
CAL_XCHG_F32, CAL_XCHG_F64, CAL_XCHG_I32 = 0, 1, 2
CAL_XCHG_SUM, CAL_XCHG_MIN = 0, 1

_lib = None


class CalamityHipError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"calamity_hip error {code}: {message}")
        self.code = code


def load():
    """Load the shared library (once) and declare every prototype.  Raises if the build is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C calamity_amd/csrc`.  calamity_amd has no CPU fallback."
        )
    # RCCL between processes / devices shares buffers by IPC handles; hosts whose driver only supports dmabuf IPC need the legacy
    # mode off BEFORE the HSA runtime starts (first HIP call), else communicator set-up fails with "hipIpcGetMemHandle: invalid argument"
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(code):
    if code != 0:
        raise CalamityHipError(code, load().cal_last_error().decode("utf-8", "replace"))


def device_count():
    n = C.c_int(0)
    check(load().cal_device_count(C.byref(n)))
    return n.value


def device_info(device=0):
    name = C.create_string_buffer(256)
    mem = C.c_int64(0)
    cus = C.c_int32(0)
    check(load().cal_device_info(device, name, 256, C.byref(mem), C.byref(cus)))
    return dict(name=name.value.decode(), total_mem_bytes=mem.value, compute_units=cus.value)


def stream_peak(device=0, nbytes=4 << 30, reps=5):
    """Measured streaming peaks of the device in GB/s: (read-only sweep, copy)."""
    rd, cp = C.c_double(0.0), C.c_double(0.0)
    check(load().cal_device_stream_peak(device, nbytes, reps, C.byref(rd), C.byref(cp)))
    return rd.value, cp.value


def busy_clock_mhz(device=0):
    """Shader clock (MHz) the device holds while all CUs run vector FMAs."""
    mhz = C.c_double(0.0)
    check(load().cal_device_busy_clock_mhz(device, C.byref(mhz)))
    return mhz.value
