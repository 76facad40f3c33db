#!/usr/bin/env python3
"""Build-time guard (called by the Makefile with hipcc's -Rpass-analysis=kernel-resource-usage remarks on stdin).

The dense kernels consume their LDS-DMA operand ring behind COUNTED `s_waitcnt vmcnt(N)`: every vector-memory operation of
a wave is in that count, and register spills are vector-memory operations (scratch).  A spilling build would therefore not
just be slower, it would read ring slots before they have landed.  So: no scratch, no spills, in any kernel whose name
contains `fused_dense`; and two waves per SIMD where the kernels are written for two.
`fused_multi_mfma_kernel<float>` sits at 245 of the 256 registers two waves per SIMD leave it (the double instance has a
CU to itself): no scratch and no spilled VGPRs there either (a few SGPR spills into lanes of a VGPR are tolerated: they sit outside its job loop).
`fused_basis_kernel`: no scratch in any instance; four waves per SIMD in the fp32 gradient instances with full and with folded tiles.
`gain_project_kernel`, `gain_expand_kernel` (gain_basis_kernels.hpp), `gain_time_project_kernel`, `gain_time_expand_kernel`
(gain_time_basis_kernels.hpp), `quality_rows_kernel`, `quality_ant_kernel` (fit_quality_kernels.hpp), `robust_rows_kernel` (robust_weight_kernels.hpp, both
instances of both dtypes), `gain_solve_rows_kernel`, `gain_solve_ant_kernel`,
`gain_solve_apply_kernel` (gain_solve_kernels.hpp), `coeff_solve_rows_kernel`, `coeff_gram_kernel`, `coeff_chol_kernel`
(coeff_solve_kernels.hpp), `gain_basis_gram_kernel`, `gain_basis_chol_kernel` (gain_basis_solve_kernels.hpp; both pairs are built on the
shared Gram and Cholesky core of normal_solve.hpp; the second is the factor step of the time-basis solve too), `gain_time_kron_kernel`,
`gain_time_chan_kernel` (gain_time_solve_kernels.hpp, both instances), `fit_error_factor_kernel`, `fit_error_leverage_kernel`, `fit_error_rows_kernel` (fit_error_kernels.hpp),
`gain_error_factor_kernel`, `gain_error_var_kernel`, `gain_time_chan_var_kernel`, `gain_error_dof_kernel` (gain_error_kernels.hpp), every `gn_*_kernel`
(gauss_newton_kernels.hpp), every `lbfgs_*_kernel` (lbfgs_kernels.hpp): no scratch, no spilled VGPRs.
`dspec_rows_kernel`, `dspec_transform_kernel`, `dspec_bin_kernel` (delay_spectrum_kernels.hpp), both dtypes: no scratch, no spilled VGPRs, and
two waves per SIMD in the transform kernel.
`dcross_rows_kernel`, `dcross_transform_kernel` (delay_cross_kernels.hpp), both dtypes: no scratch, no spilled VGPRs, and two waves per
SIMD in the transform kernel.
`dfringe_rows_kernel`, `dfringe_transform_kernel` (both dtypes), `dfringe_time_kernel` (delay_fringe_kernels.hpp): no scratch, no spilled
VGPRs, two waves per SIMD in the transform kernel and in the time kernel (two workgroups of four waves per CU at 64 times).
`dcoherent_rows_kernel`, `dcoherent_mask_kernel` (delay_coherent_kernels.hpp), both dtypes: no scratch, no spilled VGPRs.
`dtransfer_basis_kernel`, `dtransfer_power_kernel` (delay_transfer_kernels.hpp), both dtypes: no scratch, no spilled VGPRs, and two waves
per SIMD in the power kernel.
`degen_rows_kernel`, `degen_sum_kernel`, `degen_solve_kernel`, `degen_phase_kernel`, `degen_apply_gains_kernel`, `degen_apply_rows_kernel`
(degeneracy_kernels.hpp), both dtypes: no scratch, no spilled VGPRs.
`mixed_dense_kernel`, `mixed_init_kernel`, `mixed_step_kernel`, `mixed_gram_kernel`, `mixed_cert_kernel`, `mixed_cert_sum_kernel`,
`mixed_backmul_kernel` (mixed_comps_kernels.hpp): no scratch, no spilled VGPRs."""
import re
import sys

cur, bad, seen = None, [], 0
for line in sys.stdin:
    m = re.search(r"remark:\s+Function Name: (\S+)", line)
    if m:
        cur = m.group(1)
        seen += "fused_dense" in cur
        continue
    if cur is not None and "fused_multi_mfma" in cur:
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and m.group(1).startswith("Occupancy"):
            inst = re.search(r"fused_multi_mfma_kernelI([fd])Li(\d)ELi(\d)E", cur)  # <T, MODE, REG>
            one_wg = inst is None or inst.group(1) == "d" or inst.group(3) == "2"  # (double, and the one-pass regularised form: one workgroup per CU by design)
            if int(m.group(2)) < 2 and not one_wg:
                bad.append(f"{cur}: occupancy {m.group(2)} waves/SIMD (< 2)")
        elif m and int(m.group(2)) != 0:
            bad.append(f"{cur}: {m.group(1)} = {m.group(2)}")
        continue
    if cur is not None and "fused_basis_kernel" in cur:
        # the streaming kernel's headline instances (fp32, gradient pass, no regulariser, full and folded tiles) hide HBM latency with
        # four workgroups per CU: four waves per SIMD and no scratch; no instance of the kernel may use scratch at all
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and m.group(1).startswith("Occupancy"):
            if re.search(r"fused_basis_kernelIfLi1ELb0ELi7ELb[01]E", cur) and int(m.group(2)) < 4:
                bad.append(f"{cur}: occupancy {m.group(2)} waves/SIMD (< 4)")
        elif m and int(m.group(2)) != 0:
            bad.append(f"{cur}: {m.group(1)} = {m.group(2)}")
        continue
    if cur is not None and any(k in cur for k in ("gain_project_kernel", "gain_expand_kernel", "gain_time_project_kernel", "gain_time_expand_kernel",
                                             "quality_rows_kernel", "quality_ant_kernel", "robust_rows_kernel", "gain_solve_rows_kernel", "gain_solve_ant_kernel",
                                             "gain_solve_apply_kernel", "coeff_solve_rows_kernel", "coeff_gram_kernel", "coeff_chol_kernel",
                                             "gain_basis_gram_kernel", "gain_basis_chol_kernel", "gain_time_kron_kernel",
                                             "gain_time_chan_kernel", "fit_error_factor_kernel", "fit_error_leverage_kernel", "fit_error_rows_kernel",
                                             "gain_error_factor_kernel", "gain_error_var_kernel", "gain_time_chan_var_kernel", "gain_error_dof_kernel",
                                             "gn_tangent_rows_kernel", "gn_scale_kernel", "gn_data_kernel", "gn_precond_rows_kernel", "gn_precond_gain_kernel",
                                             "gn_precond_coeff_kernel", "gn_rhs_kernel", "gn_init_kernel", "gn_scalar0_kernel", "gn_diff_kernel",
                                             "gn_scalar1_kernel", "gn_update1_kernel", "gn_scalar2_kernel", "gn_update2_kernel", "gn_apply_kernel",
                                             "gn_round_kernel", "lbfgs_pair_kernel", "lbfgs_reduce_kernel", "lbfgs_coeff_kernel", "lbfgs_direction_kernel",
                                             "lbfgs_trial_kernel", "lbfgs_armijo_kernel", "lbfgs_restore_kernel")):
        # the kernels around the update of a gain-basis fit, the two of the fit-quality pass, the one of the robust reweighting, the three of the gain solve, the three
        # of the coefficient solve, the two of the gain-coefficient solve, the two of the time-basis solve beside them, the three of the fit errors, the four of the basis-gain errors, those of the
        # Gauss-Newton step and those of L-BFGS keep their accumulators in registers: no scratch
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and int(m.group(2)) != 0:
            bad.append(f"{cur}: {m.group(1)} = {m.group(2)}")
        continue
    if cur is not None and any(k in cur for k in ("dspec_rows_kernel", "dspec_transform_kernel", "dspec_bin_kernel")):
        # the three of the delay spectrum: no scratch, no spilled VGPRs; the transform keeps 2 x 8 accumulator tiles per wave and is
        # written for two waves per SIMD in both dtypes
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and m.group(1).startswith("Occupancy"):
            if "dspec_transform_kernel" in cur and int(m.group(2)) < 2:
                bad.append(f"{cur}: occupancy {m.group(2)} waves/SIMD (< 2)")
        elif m and int(m.group(2)) != 0:
            bad.append(f"{cur}: {m.group(1)} = {m.group(2)}")
        continue
    if cur is not None and any(k in cur for k in ("dcross_rows_kernel", "dcross_transform_kernel")):
        # the two of the delay cross spectrum: no scratch, no spilled VGPRs; the transform runs the spectrum's loop (2 x 8 accumulator tiles
        # per wave) and keeps its two waves per SIMD in both dtypes
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and m.group(1).startswith("Occupancy"):
            if "dcross_transform_kernel" in cur and int(m.group(2)) < 2:
                bad.append(f"{cur}: occupancy {m.group(2)} waves/SIMD (< 2)")
        elif m and int(m.group(2)) != 0:
            bad.append(f"{cur}: {m.group(1)} = {m.group(2)}")
        continue
    if cur is not None and any(k in cur for k in ("dfringe_rows_kernel", "dfringe_transform_kernel", "dfringe_time_kernel")):
        # the three of the delay / fringe-rate spectrum: no scratch, no spilled VGPRs; the transform runs the spectrum's loop and keeps its
        # two waves per SIMD in both dtypes; the time kernel's LDS admits two workgroups per CU at 64 times, and its registers must too
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and m.group(1).startswith("Occupancy"):
            if ("dfringe_transform_kernel" in cur or "dfringe_time_kernel" in cur) and int(m.group(2)) < 2:
                bad.append(f"{cur}: occupancy {m.group(2)} waves/SIMD (< 2)")
        elif m and int(m.group(2)) != 0:
            bad.append(f"{cur}: {m.group(1)} = {m.group(2)}")
        continue
    if cur is not None and any(k in cur for k in ("dcoherent_rows_kernel", "dcoherent_mask_kernel")):
        # the two in front of the coherent spectrum: a set's sums in double stay in registers (28 doubles per lane in fp32): no scratch, no
        # spilled VGPRs
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and int(m.group(2)) != 0:
            bad.append(f"{cur}: {m.group(1)} = {m.group(2)}")
        continue
    if cur is not None and any(k in cur for k in ("dtransfer_basis_kernel", "dtransfer_power_kernel")):
        # the two of the delay transfer: no scratch, no spilled VGPRs; the power kernel keeps 2 x 8 accumulator tiles per wave, as the
        # spectrum's transform does, and is written for two waves per SIMD in both dtypes
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and m.group(1).startswith("Occupancy"):
            if "dtransfer_power_kernel" in cur and int(m.group(2)) < 2:
                bad.append(f"{cur}: occupancy {m.group(2)} waves/SIMD (< 2)")
        elif m and int(m.group(2)) != 0:
            bad.append(f"{cur}: {m.group(1)} = {m.group(2)}")
        continue
    if cur is not None and any(k in cur for k in ("degen_rows_kernel", "degen_sum_kernel", "degen_solve_kernel", "degen_phase_kernel",
                                             "degen_apply_gains_kernel", "degen_apply_rows_kernel")):
        # the six of the degeneracy fix keep their sums, and the double-precision sincos its argument reduction, in registers
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and int(m.group(2)) != 0:
            bad.append(f"{cur}: {m.group(1)} = {m.group(2)}")
        continue
    if cur is not None and any(k in cur for k in ("mixed_dense_kernel", "mixed_init_kernel", "mixed_step_kernel", "mixed_gram_kernel",
                                             "mixed_cert_kernel", "mixed_cert_sum_kernel", "mixed_backmul_kernel")):
        # the seven of the mixed-model components (mixed_comps_kernels.hpp): the double-precision sinpi of the covariance element and the
        # four accumulator tiles of the tile products stay in registers
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and int(m.group(2)) != 0:
            bad.append(f"{cur}: {m.group(1)} = {m.group(2)}")
        continue
    if cur is None or "fused_dense" not in cur:
        continue
    m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill|Occupancy \[waves/SIMD\]): (\d+)", line)
    if not m:
        continue
    key, val = m.group(1), int(m.group(2))
    if key.startswith("Occupancy"):
        if val < 2 and "fused_dense_split" not in cur:  # (the split-bf16 kernel runs one workgroup per CU by design: split_kernels.hpp)
            bad.append(f"{cur}: occupancy {val} waves/SIMD (< 2)")
    elif val != 0 and not (key.startswith("SGPRs Spill") and "fused_dense_split" in cur):
        # (SGPR spills of the split-bf16 kernel go into lanes of a VGPR -- it has 512 -- not to scratch: ScratchSize stays checked)
        bad.append(f"{cur}: {key} = {val}")
if seen == 0:
    bad.append("no fused_dense kernel found in the compiler's resource remarks")
if bad:
    sys.stderr.write("check_resources: the dense kernels must not spill (scratch traffic breaks their counted waits), the streaming kernel must keep its occupancy:\n  " + "\n  ".join(bad) + "\n")
    sys.exit(1)
print(f"check_resources: {seen} dense kernels, no scratch, no spills")
