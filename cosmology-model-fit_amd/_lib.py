"""
ctypes binding of the gfx950 shared library (csrc/ -> libcosmofit_hip.so) behind include/cosmofit.h.

There is no CPU implementation behind this module: if the library is missing or no MI355X is
visible, every operation raises (``CosmofitError``), it never falls back.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# COSMOFIT_LIB: another build of the same sources (tools/build_variant.sh: tuning / debug variants for A/B timing)
LIB_PATH = os.environ.get("COSMOFIT_LIB") or os.path.join(_HERE, "libcosmofit_hip.so")
CSRC = os.path.join(_HERE, "csrc")

CF_ABI_VERSION = 11
CF_P_NSLOTS = 15
SLOTS = ("offset", "H0", "Om", "obh2", "och2", "w0", "wa", "v", "rd", "fcc", "lin", "v2", "v3", "s8", "fs8err")

# enums of include/cosmofit.h
CF_EZ_LATE_FLAT, CF_EZ_PHYSICAL = 0, 1
CF_FDE_LCDM, CF_FDE_WCDM, CF_FDE_THAWING, CF_FDE_CPL = 0, 1, 2, 3
CF_OUT_CHI2, CF_OUT_LOGL, CF_OUT_LOGP = 0, 1, 2
CF_SOLVE_BLOCKED_TRSM, CF_SOLVE_INVERSE_GEMM, CF_SOLVE_AUTO = 0, 1, 2
SOLVE_MODES = {"blocked": CF_SOLVE_BLOCKED_TRSM, "inverse": CF_SOLVE_INVERSE_GEMM, "auto": CF_SOLVE_AUTO}
CF_CMB_NONE = 0
STATUS = {0: "CF_OK", -1: "CF_ERR_INVALID", -2: "CF_ERR_NO_DEVICE", -3: "CF_ERR_HIP", -4: "CF_ERR_NOT_POSDEF",
          -5: "CF_ERR_UNSUPPORTED", -6: "CF_ERR_ILL_CONDITIONED"}


class CosmofitError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{STATUS.get(code, code)}: {msg}")
        self.code = code


class cf_param(C.Structure):
    _fields_ = [("idx", C.c_int32), ("_pad", C.c_int32), ("scale", C.c_double), ("fixed", C.c_double)]


class cf_gauss_prior(C.Structure):
    _fields_ = [("idx", C.c_int32), ("_pad", C.c_int32), ("mean", C.c_double), ("sigma", C.c_double)]


class cf_desc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("struct_size", C.c_int32), ("device", C.c_int32), ("ndim", C.c_int32),
        ("ez_model", C.c_int32), ("fde", C.c_int32), ("n_grid", C.c_int32), ("_pad0", C.c_int32),
        ("z_max", C.c_double), ("c_km_s", C.c_double),
        ("param", cf_param * CF_P_NSLOTS),
        ("n_sn", C.c_int64),
        ("sn_z_cmb", C.c_void_p), ("sn_z_hel", C.c_void_p), ("sn_obs", C.c_void_p), ("sn_step", C.c_void_p),
        ("sn_z_turn", C.c_double),
        ("sn_chol", C.c_void_p), ("sn_chol_ld", C.c_int64),
        ("n_bao", C.c_int32), ("bao_dh_mode", C.c_int32), ("rd_mode", C.c_int32), ("_pad1", C.c_int32),
        ("bao_z", C.c_void_p), ("bao_val", C.c_void_p), ("bao_qty", C.c_void_p), ("bao_inv_cov", C.c_void_p),
        ("rd_fit", C.c_double * 11),
        ("cmb_mode", C.c_int32), ("n_gl", C.c_int32),
        ("gl_x", C.c_void_p), ("gl_w", C.c_void_p),
        ("cmb_prior", C.c_double * 3), ("cmb_inv_cov", C.c_double * 9),
        ("zstar_fit", C.c_double * 11), ("o_gamma_h2", C.c_double),
        ("or_h2", C.c_double), ("omnu_h2", C.c_double), ("nu_m0", C.c_double), ("nu_rho0", C.c_double),
        ("nu_qs_sq", C.c_double * 5), ("nu_ws", C.c_double * 5),
        ("bounds", C.c_void_p),
        ("n_gauss", C.c_int32), ("cpl_wall", C.c_int32),
        ("gauss", C.c_void_p),
        ("n_chi2_gauss", C.c_int32), ("_pad2", C.c_int32),
        ("chi2_gauss", C.c_void_p),
        ("sn_fixed_mu", C.c_void_p),
        ("n_cc", C.c_int32), ("_pad3", C.c_int32),
        ("cc_z", C.c_void_p), ("cc_h", C.c_void_p), ("cc_inv_cov", C.c_void_p),
        ("cc_logdet", C.c_double),
        ("solve_mode", C.c_int32), ("_pad4", C.c_int32),
        ("probe_limit", C.c_double),
        ("n_devices", C.c_int32), ("_pad5", C.c_int32), ("devices", C.c_void_p),
        ("om_mode", C.c_int32), ("rd_wm_mode", C.c_int32), ("sn_lin_coef", C.c_void_p), ("sn_dir", C.c_void_p),
        ("n_fs8", C.c_int32), ("fs8_steps", C.c_int32),
        ("fs8_z", C.c_void_p), ("fs8_val", C.c_void_p), ("fs8_inv_cov", C.c_void_p), ("fs8_fid", C.c_void_p),
        ("logl_const", C.c_double), ("fs8_a_init", C.c_double),
        ("sn_vel_mode", C.c_int32), ("cc_f_mode", C.c_int32), ("prior_norm_mode", C.c_int32), ("fs8_n_agrid", C.c_int32),
    ]


CF_NS_MAX_NDIM = 16
CF_NS_UNIFORM, CF_NS_NORMAL = 0, 1


class cf_ns_prior(C.Structure):
    _fields_ = [("ndim", C.c_int32), ("_pad", C.c_int32), ("kind", C.c_int32 * CF_NS_MAX_NDIM),
                ("a", C.c_double * CF_NS_MAX_NDIM), ("b", C.c_double * CF_NS_MAX_NDIM)]


CF_QSR_BAO_NONE, CF_QSR_BAO_QUAD = 0, 1

CF_MARG_MAX_NDIM, CF_MARG_MAX_BINS, CF_MARG_MAX_PAIRS, CF_MARG_MAX_SEGMENTS, CF_MARG_NOT_COUNTED = 16, 128, 256, 65536, 255

CF_KDE_MAX_NDIM, CF_KDE_TILE, CF_KDE_SLICE, CF_KDE_QUERY_BLOCK, CF_KDE_SPLIT_BELOW_BLOCKS = 8, 256, 2048, 512, 512

CF_OPT_MAX_NDIM, CF_OPT_MAX_TRIALS = 16, 8
CF_OPT_RUNNING, CF_OPT_CONVERGED, CF_OPT_NOISE_FLOOR, CF_OPT_ITER_CAP, CF_OPT_NONFINITE_START, CF_OPT_NONFINITE_STENCIL = range(6)
CF_OPT_NEED_RESET, CF_OPT_HAS_PAIR, CF_OPT_FRESH, CF_OPT_HAS_STEP = 1, 2, 4, 8


class cf_opt_params(C.Structure):
    _fields_ = [("ndim", C.c_int32), ("n_free", C.c_int32), ("free_idx", C.c_int32 * CF_OPT_MAX_NDIM),
                ("lo", C.c_double * CF_OPT_MAX_NDIM), ("width", C.c_double * CF_OPT_MAX_NDIM), ("h", C.c_double),
                ("delta", C.c_double), ("c1", C.c_double), ("gtol", C.c_double), ("gtol_rel", C.c_double),
                ("n_trials", C.c_int32), ("max_iter", C.c_int32)]


class cf_opt_state(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ("u", "f", "g", "g_prev", "s", "hinv", "d", "gnorm", "form", "status", "n_iter",
                                                "flags")]


class cf_qsr_ext(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("n_grid", C.c_int32), ("n_qsr", C.c_int64),
        ("qsr_z", C.c_void_p), ("qsr_mu", C.c_void_p), ("qsr_sigma", C.c_void_p),
        ("qsr_offset", cf_param), ("qsr_scatter", cf_param),
        ("fde_n", C.c_double), ("fde_k", C.c_double), ("fde_p", C.c_double),
        ("qsr_z_top", C.c_double), ("sn_z_top", C.c_double),
        ("sn_zhel", C.c_int32), ("bao_mode", C.c_int32), ("n_bao", C.c_int32), ("_pad", C.c_int32),
        ("bao_z", C.c_void_p), ("bao_val", C.c_void_p), ("bao_qty", C.c_void_p), ("bao_inv_cov", C.c_void_p),
    ]


CF_DQ_MAX, CF_CURVE_MAX_NZ = 32, 4096
# cf_derived_code / cf_curve_code of include/cosmofit.h by the names derived.Spec takes
DERIVED_CODES = {"H0": 0, "h": 1, "Om": 2, "omh2": 3, "obh2": 4, "och2": 5, "w0": 6, "wa": 7, "q0": 8, "j0": 9, "S8": 10, "rd": 11,
                 "z_star": 12, "r_drag": 13, "z_drag": 14, "z_eq": 15, "H@": 16,
                 "rs_star": 32, "DM_star": 33, "theta_star100": 34, "R": 35, "lA": 36}
CURVE_CODES = {"H": 0, "DM": 1, "DV_rd": 2, "DM_rd": 3, "DH_rd": 4, "F_AP": 5, "mu": 6}


class cf_derived_consts(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("has_rdrag_fit", C.c_int32), ("zdrag_fit", C.c_double * 10),
                ("rdrag_fit", C.c_double * 11), ("zeq_or_h2", C.c_double)]


CF_GP_NDIM, CF_GP_MAX_N, CF_GP_MAX_NZ = 4, 64, 65536


class cf_gp_desc(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("n", C.c_int32), ("_pad", C.c_int32),
                ("z", C.c_void_p), ("y", C.c_void_p), ("cov", C.c_void_p), ("bounds", C.c_void_p)]


class cf_gp_info(C.Structure):
    _fields_ = [("n", C.c_int32), ("device", C.c_int32), ("ld", C.c_int32), ("lds_bytes", C.c_int32),
                ("failed_factorizations", C.c_int64)]


CF_FIELD_MAX_NQ, CF_FIELD_MAX_NDIM, CF_FIELD_NPAR, CF_FIELD_NSCALAR, CF_FIELD_LAUNCH_ROWS = 4096, 64, 4, 5, 1 << 22
CF_FIELD_OK, CF_FIELD_PHANTOM, CF_FIELD_BAD = 0, 1, 2
FIELD_PARS = ("H0", "Om", "w0", "wa")
FIELD_SCALARS = ("phi_today", "t_today", "hubble_time", "phi_max", "t_max")
FIELD_OUTPUTS = ("phi_a", "t_a", "w_a", "K_a", "V_a", "phi_grid", "a_phi", "V_phi", "t_grid", "a_t", "phi_t")


class cf_field_desc(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("fde", C.c_int32), ("n_a", C.c_int32), ("ndim", C.c_int32), ("n_par", C.c_int32),
                ("_pad", C.c_int32), ("a_min", C.c_double), ("a_max", C.c_double), ("orh2", C.c_double),
                ("par", cf_param * CF_FIELD_NPAR)]


class cf_field_queries(C.Structure):
    _fields_ = [("a_q", C.c_void_p), ("phi_q", C.c_void_p), ("t_q", C.c_void_p), ("n_aq", C.c_int32), ("n_phi", C.c_int32),
                ("n_t", C.c_int32), ("_pad", C.c_int32)]


class cf_field_out(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in FIELD_OUTPUTS + ("scalars", "status")]


CF_RB_SN, CF_RB_BAO = 0, 1
CF_RS_NCOL, CF_RESID_MAX_THR, CF_RESID_CHUNK = 10, 4, 4096
RESID_BLOCKS = {"sn": CF_RB_SN, "bao": CF_RB_BAO}
# cf_resid_col of include/cosmofit.h, in column order
RESID_COLUMNS = ("mean", "std", "ss_res", "rmsd", "ss_tot", "r2", "skew", "kurtosis", "max_pull", "max_pull_index")
# the ten chi2_blocks columns of cf_eval_parts / cf_resid_device
CHI2_BLOCK_COLUMNS = ("chi2_sn", "chi2_bao", "chi2_cmb", "cmb_v0", "cmb_v1", "cmb_v2", "chi2_cc", "chi2_fs8", "z_star", "r_drag")


class cf_resid_acc(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n", C.c_int32), ("n_thr", C.c_int32), ("_pad", C.c_int32),
                ("w_sum", C.c_void_p), ("mean", C.c_void_p), ("m2", C.c_void_p), ("exceed", C.c_void_p),
                ("n_used", C.c_void_p), ("n_skipped", C.c_void_p)]


CF_MOCK_CHUNK = 4096


class cf_mock_set(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_mocks", C.c_int32), ("n_sn", C.c_int32), ("n_bao", C.c_int32),
                ("n_cmb", C.c_int32), ("_pad", C.c_int32),
                ("g_sn", C.c_void_p), ("g_bao", C.c_void_p), ("g_cmb", C.c_void_p), ("c", C.c_void_p)]


CF_INFL_NCOL, CF_INFL_CHUNK = 5, 4096
# cf_infl_col of include/cosmofit.h, in column order
INFL_COLUMNS = ("chi2", "max_z", "max_z_index", "max_drop", "max_drop_index")


class cf_infl_out(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("_pad", C.c_int32),
                ("g", C.c_void_p), ("contrib", C.c_void_p), ("z", C.c_void_p), ("loo", C.c_void_p), ("sample", C.c_void_p)]


CF_CSCALE_MAX_S, CF_CSCALE_CHUNK = 16, 4096
CF_MARG_MAX_M, CF_MARG_CHUNK, CF_MARG_SLICE = 16, 4096, 256
CF_MARG_PROFILE, CF_MARG_MARGINAL = 0, 1
CF_SCAN_CHUNK, CF_SCAN_TILE, CF_SCAN_MAX_K = 4096, 64, (1 << 24) - 1


CF_BRIDGE_MAX_NDIM, CF_BRIDGE_SLICE, CF_BRIDGE_RESULT_DOUBLES = 16, 2048, 8
# cf_bridge_result of include/cosmofit.h, in index order, and cf_bridge_status
BRIDGE_RESULT = ("log_r", "n_iter", "status", "mean_f1", "var_f1", "mean_f2", "var_f2", "r")
CF_BRIDGE_CONVERGED, CF_BRIDGE_ITER_CAP, CF_BRIDGE_NONFINITE = range(3)


CF_GROUP_MAX_GROUPS, CF_GROUP_MAX_M, CF_GROUP_MAX_BYTES = 1024, 1024, 256 << 20
CF_RW_SLICE, CF_RW_MAX_NCOL, CF_RW_MAX_G, CF_RW_MEAN = 2048, 16, 4096, 8
# cf_rw_slot of include/cosmofit.h, in slot order; the moments follow from CF_RW_MEAN on
RW_SLOTS = ("lmax", "sum_w", "sum_w2", "max_w", "n_used", "n_skipped", "sum_w0", "sum_w0_sq")


def rw_ncol(ncol: int) -> int:
    """CF_RW_NCOL(ncol): doubles per column record of cf_reweight_device."""
    return 8 + ncol + ncol * (ncol + 1) // 2


class cf_info(C.Structure):
    _fields_ = [
        ("n_sn", C.c_int64), ("n_sn_pad", C.c_int64), ("packed_chol_bytes", C.c_int64),
        ("workspace_bytes", C.c_int64), ("max_walkers", C.c_int64), ("nonfinite_count", C.c_int64),
        ("device", C.c_int32), ("cu_count", C.c_int32), ("gcn_arch", C.c_char * 64),
        ("pack_probe_rel", C.c_double), ("solve_mode", C.c_int32), ("n_devices", C.c_int32),
        ("devices", C.c_int32 * 16),
    ]


# every symbol include/cosmofit.h declares: name -> (restype, argtypes)
_VP, _I64, _I32 = C.c_void_p, C.c_int64, C.c_int32
EXPORTS = {
    "cf_device_count": (C.c_int, []),
    "cf_last_error": (C.c_char_p, []),
    "cf_abi_version": (C.c_int, []),
    "cf_create": (C.c_int, [C.POINTER(cf_desc), C.POINTER(_VP)]),
    "cf_destroy": (None, [_VP]),
    "cf_get_info": (C.c_int, [_VP, C.POINTER(cf_info)]),
    "cf_eval": (C.c_int, [_VP, _VP, _I64, _VP, _I32]),
    "cf_split_rows": (None, [_I64, _I32, _I32, C.POINTER(_I64), C.POINTER(_I64)]),
    "cf_eval_device": (C.c_int, [_VP, _VP, _I64, _VP, _I32, _VP]),
    "cf_eval_parts": (C.c_int, [_VP, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP]),
    "cf_eval_table": (C.c_int, [_VP, _VP, _I64, _VP, _VP]),
    "cf_eval_bao_at": (C.c_int, [_VP, _VP, _VP, _VP, _I64, _VP]),
    "cf_eval_hz": (C.c_int, [_VP, _VP, _VP, _I64, _VP]),
    "cf_eval_fs8_at": (C.c_int, [_VP, _VP, _VP, _I64, _VP]),
    "cf_last_kernel_ms": (C.c_int, [_VP, C.POINTER(C.c_float * 2)]),
    "cf_enable_timing": (C.c_int, [_VP, C.c_int]),
    "cf_set_timing_stride": (C.c_int, [_VP, C.c_int]),
    "cf_timed_calls": (C.c_int64, [_VP]),
    "cf_kernel_ms": (C.c_int, [_VP, _I64, C.POINTER(C.c_float * 2)]),
    "cf_kernel_ms3": (C.c_int, [_VP, _I64, C.POINTER(C.c_float * 3)]),
    "cf_walker_form": (C.c_int, [_VP, _I64]),
    "cf_walker_levels": (C.c_int, [_VP, C.POINTER(C.c_int32 * 8)]),
    "cf_solve_form": (C.c_int, [_I64, _I64, C.POINTER(C.c_int32 * 10)]),
    "cf_solve_frag_order": (C.c_int, [_VP, _I64]),
    "cf_small_blocks_form": (C.c_int, [_VP, _I64]),
    "cf_last_residuals": (C.c_int, [_VP, _I64, _VP, C.POINTER(C.c_int32)]),
    "cf_interp_hermite": (C.c_int, [_VP, _I64, _VP, _VP, _VP, _I64, _VP]),
    "cf_interp_pchip": (C.c_int, [_VP, _I64, _VP, _VP, _I64, _VP]),
    "cf_solve_triangular": (C.c_int, [_VP, _I64, _I64, _VP, _I64, _VP]),
    "cf_selftest_invpack_host": (C.c_int, [_VP, _I64, _I64, _VP, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "cf_selftest_log10": (C.c_int, [_VP, _I64, _VP]),
    "cf_selftest_log10_tab": (C.c_int, [_VP, _I64, _VP]),
    "cf_selftest_exp_tab": (C.c_int, [_VP, _I64, _VP]),
    "cf_selftest_pos_ops": (C.c_int, [_VP, _VP, _I64, _VP]),
    "cf_ens_active_count": (_I64, [C.c_uint64, _I32, _I32, _I64, _I64]),
    "cf_ens_comp_count": (_I64, [C.c_uint64, _I32, _I32, _I64]),
    "cf_ens_active_set": (C.c_int, [C.c_uint64, _I32, _I32, _I64, _I64, _VP, _VP, _VP]),
    "cf_ens_kde_prepare": (C.c_int, [_VP, _I64, _I32, _I32, _I32, C.c_uint64, _VP, _VP, _VP]),
    "cf_ens_propose": (C.c_int, [_I32, _VP, _I64, _I32, _I32, _I32, C.c_uint64, _VP, _I64, C.c_uint64, C.c_double,
                                 C.c_double, _VP, _VP, _VP, _VP, _VP]),
    "cf_ens_accept": (C.c_int, [_VP, _VP, _I64, C.c_int32, C.c_uint64, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "cf_ens_accept_record": (C.c_int, [_VP, _VP, _I64, C.c_int32, C.c_uint64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                       _VP]),
    "cf_chain_mean": (C.c_int, [_VP, _I64, _I64, _VP, _VP]),
    "cf_chain_lagsum": (C.c_int, [_VP, _VP, _I64, _I64, _I64, _I32, _VP, _VP]),
    "cf_chain_acf_mean": (C.c_int, [_VP, _VP, _I64, _I32, _I32, _VP, _VP]),
    "cf_marg_bin": (C.c_int, [_VP, _I64, _I32, _VP, _I32, _VP, _VP]),
    "cf_marg_hist": (C.c_int, [_VP, _VP, C.c_double, _I64, _I32, _I32, _VP, _I32, _VP, _VP, _I32, _VP]),
    "cf_kde_sum_device": (C.c_int, [_VP, _VP, _I64, _I32, _VP, _I64, _I64, _VP, _VP, _VP]),
    "cf_ns_prior_draw": (C.c_int, [_VP, _I64, C.c_uint64, _VP, _VP, _VP]),
    "cf_ns_transform": (C.c_int, [_VP, _VP, _I64, _VP, _VP]),
    "cf_ns_walk_start": (C.c_int, [_VP, _VP, _VP, _I64, _I32, _I64, C.c_uint64, _VP, _VP, _VP, _VP]),
    "cf_ns_propose": (C.c_int, [_VP, _VP, _I64, _I64, C.c_uint64, C.c_double, C.c_double, _VP, _VP, _VP, _VP, _VP, _VP]),
    "cf_ns_accept": (C.c_int, [_I64, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "cf_selftest_pack_host": (C.c_int, [_VP, _I64, _I64, _VP, C.POINTER(C.c_double), C.POINTER(_I64)]),
    "cf_create_quasar": (C.c_int, [C.POINTER(cf_desc), C.POINTER(cf_qsr_ext), C.POINTER(_VP)]),
    "cf_qsr_eval_parts": (C.c_int, [_VP, _VP, _I64, _VP, _VP, _VP, _VP]),
    "cf_opt_starts": (C.c_int, [C.POINTER(cf_opt_params), _I64, _VP, C.c_uint64, _I32, _VP, _VP, _VP]),
    "cf_opt_stencil": (C.c_int, [C.POINTER(cf_opt_params), C.POINTER(cf_opt_state), _VP, _I64, _VP, _VP]),
    "cf_opt_direction": (C.c_int, [C.POINTER(cf_opt_params), C.POINTER(cf_opt_state), _VP, _I64, _VP, _VP, _VP]),
    "cf_opt_accept": (C.c_int, [C.POINTER(cf_opt_params), C.POINTER(cf_opt_state), _VP, _I64, _VP, _VP]),
    "cf_opt_compact": (C.c_int, [_VP, _I64, _VP, _VP, _VP, _VP]),
    "cf_derived_device": (C.c_int, [_VP, _VP, _I64, _VP, _VP, _I32, _VP, _VP, _VP]),
    "cf_curves_device": (C.c_int, [_VP, _VP, _I64, _I32, _VP, _I32, _VP, _VP]),
    "cf_derived": (C.c_int, [_VP, _VP, _I64, _VP, _VP, _I32, _VP, _VP]),
    "cf_curves": (C.c_int, [_VP, _VP, _I64, _I32, _VP, _I32, _VP]),
    "cf_gp_create": (C.c_int, [C.POINTER(cf_gp_desc), C.POINTER(_VP)]),
    "cf_gp_destroy": (None, [_VP]),
    "cf_gp_get_info": (C.c_int, [_VP, C.POINTER(cf_gp_info)]),
    "cf_gp_mll_device": (C.c_int, [_VP, _VP, _I64, _VP, _VP, _VP]),
    "cf_gp_predict_device": (C.c_int, [_VP, _VP, _I64, _VP, _I32, C.c_double, _VP, _VP]),
    "cf_gp_mll": (C.c_int, [_VP, _VP, _I64, _VP, _VP]),
    "cf_gp_predict": (C.c_int, [_VP, _VP, _I64, _VP, _I32, C.c_double, _VP]),
    "cf_field_launch_count": (_I64, [_I64]),
    "cf_field_launch_range": (None, [_I64, _I64, C.POINTER(_I64), C.POINTER(_I64)]),
    "cf_field_device": (C.c_int, [C.POINTER(cf_field_desc), _VP, _I64, C.POINTER(cf_field_queries), C.POINTER(cf_field_out), _VP]),
    "cf_field": (C.c_int, [C.POINTER(cf_field_desc), _VP, _I64, C.POINTER(cf_field_queries), C.POINTER(cf_field_out)]),
    "cf_resid_device": (C.c_int, [_VP, _VP, _I64, _VP, _I32, _VP, _I32, _VP, _VP, C.POINTER(cf_resid_acc), _VP]),
    "cf_resid": (C.c_int, [_VP, _VP, _I64, _VP, _I32, _VP, _I32, _VP, _VP, C.POINTER(cf_resid_acc)]),
    "cf_resid_check_args": (C.c_int, [_I64, _I32, _I32, _I32, _VP, _I64, _I32, _VP, _I32, _VP, _VP, C.POINTER(cf_resid_acc)]),
    "cf_resid_sigma": (C.c_int, [_VP, _I32, _VP]),
    "cf_resid_set_chunk": (C.c_int, [_VP, _I64]),
    "cf_mock_eval_device": (C.c_int, [_VP, C.POINTER(cf_mock_set), _VP, _I64, _VP, _I32, _VP, _VP, _VP]),
    "cf_mock_eval": (C.c_int, [_VP, C.POINTER(cf_mock_set), _VP, _I64, _VP, _I32, _VP, _VP]),
    "cf_mock_check_args": (C.c_int, [_I64, _I32, _I32, _I32, _I32, C.POINTER(cf_mock_set), _VP, _I64, _VP, _I32, _VP]),
    "cf_mock_set_chunk": (C.c_int, [_VP, _I64]),
    "cf_mock_normals": (C.c_int, [C.c_uint64, _I64, _I64, _I32, _VP, _VP]),
    "cf_prec_create": (C.c_int, [_VP, _I64, _I64, _I32, C.POINTER(_VP)]),
    "cf_prec_create_inv": (C.c_int, [_VP, _I64, _I64, _I32, C.POINTER(_VP)]),
    "cf_prec_destroy": (None, [_VP]),
    "cf_prec_diag": (C.c_int, [_VP, _VP]),
    "cf_prec_apply_device": (C.c_int, [_VP, _VP, _I64, _I64, _VP, _I64, _VP]),
    "cf_selftest_prec_host": (C.c_int, [_VP, _I64, _I64, _VP, _VP]),
    "cf_infl_device": (C.c_int, [_VP, _VP, _VP, _I64, _VP, _I32, _VP, _I32, C.POINTER(cf_infl_out), C.POINTER(cf_resid_acc),
                                 C.POINTER(cf_resid_acc), _VP]),
    "cf_infl": (C.c_int, [_VP, _VP, _VP, _I64, _VP, _I32, _VP, _I32, C.POINTER(cf_infl_out), C.POINTER(cf_resid_acc),
                          C.POINTER(cf_resid_acc)]),
    "cf_infl_check_args": (C.c_int, [_I64, _I32, _I32, _I32, _I32, _I32, _I64, _I32, _VP, _I64, _I32, _VP, _I32,
                                     C.POINTER(cf_infl_out), C.POINTER(cf_resid_acc), C.POINTER(cf_resid_acc)]),
    "cf_infl_set_chunk": (C.c_int, [_VP, _I64]),
    "cf_cscale_create": (C.c_int, [_VP, _I64, _I64, _VP, _I32, C.POINTER(_VP)]),
    "cf_cscale_destroy": (None, [_VP]),
    "cf_cscale_look": (C.c_int, [_VP, C.POINTER(_I64), C.POINTER(_I32)]),
    "cf_cscale_apply_device": (C.c_int, [_VP, _VP, _I64, _I64, _VP, _I32, _VP, _VP, _VP, _VP]),
    "cf_cscale_eval_device": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I64, _I32, _VP, _VP, _VP]),
    "cf_cscale_eval": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I64, _I32, _VP, _VP]),
    "cf_cscale_check_args": (C.c_int, [_I64, _I32, _I32, _I32, _I32, _I64, _I32, _VP, _VP, _I32, _I64, _I32, _VP, _VP]),
    "cf_cscale_set_chunk": (C.c_int, [_VP, _I64]),
    "cf_selftest_cscale_host": (C.c_int, [_VP, _VP, _I64, _VP, _I32, _VP, _VP]),
    "cf_marg_create": (C.c_int, [_VP, _VP, _VP, _I64, _I32, C.c_double, C.c_double, _I32, C.POINTER(_VP)]),
    "cf_marg_destroy": (None, [_VP]),
    "cf_marg_info": (C.c_int, [_VP, C.POINTER(_I64), C.POINTER(_I32), C.POINTER(_I32), C.POINTER(C.c_double),
                               C.POINTER(C.c_double)]),
    "cf_marg_apply_device": (C.c_int, [_VP, _VP, _I64, _I64, _VP, _VP, _VP, _VP, _VP]),
    "cf_marg_eval_device": (C.c_int, [_VP, _VP, _VP, _I64, _I32, _I32, _VP, _VP, _VP, _VP]),
    "cf_marg_eval": (C.c_int, [_VP, _VP, _VP, _I64, _I32, _I32, _VP, _VP, _VP]),
    "cf_marg_check_args": (C.c_int, [_I64, _I32, _I32, _I32, _I32, _I64, _I32, _VP, _I64, _I32, _I32, _VP, _VP]),
    "cf_marg_set_chunk": (C.c_int, [_VP, _I64]),
    "cf_selftest_marg_host": (C.c_int, [_VP, _I32, _VP, _VP, _I32, _VP, C.c_double, C.c_double, C.c_double, _I32, _I32, _VP, _VP,
                                        _VP, _VP]),
    "cf_scan_create": (C.c_int, [_VP, _I64, _I64, _I64, _VP, _I32, C.POINTER(_VP)]),
    "cf_scan_destroy": (None, [_VP]),
    "cf_scan_info": (C.c_int, [_VP, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(_I32), C.POINTER(_I64)]),
    "cf_scan_apply_device": (C.c_int, [_VP, _VP, _I64, _I64, _I32, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _VP]),
    "cf_scan_eval_device": (C.c_int, [_VP, _VP, _VP, _I64, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _VP]),
    "cf_scan_eval": (C.c_int, [_VP, _VP, _VP, _I64, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP]),
    "cf_scan_check_args": (C.c_int, [_I64, _I32, _I32, _I32, _I32, _I64, _I64, _I32, _VP, _I64, _I32, _I32, _VP, _I64]),
    "cf_scan_set_chunk": (C.c_int, [_VP, _I64]),
    "cf_selftest_scan_host": (C.c_int, [_VP, _I64, _I64, _I64, _VP, _I32, _VP, _VP, _VP, _VP, _VP]),
    "cf_bridge_forward": (C.c_int, [_VP, _I64, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "cf_bridge_points": (C.c_int, [_VP, _I64, _I32, _VP, _VP, _VP, _VP, _I32, _VP, _VP, _VP]),
    "cf_bridge_draw": (C.c_int, [C.c_uint64, _I64, _I64, _I32, _VP, _VP]),
    "cf_bridge_solve": (C.c_int, [_VP, _I64, _VP, _I64, C.c_double, C.c_double, C.c_double, C.c_double, _I32, _VP, _VP, _VP]),
    "cf_group_create": (C.c_int, [_VP, _I32, _VP, _VP, C.POINTER(_VP)]),
    "cf_group_destroy": (None, [_VP]),
    "cf_group_info": (C.c_int, [_VP, _VP, _VP, _VP]),
    "cf_group_check_args": (C.c_int, [_I64, _VP, _I32, _VP, _VP]),
    "cf_selftest_group_host": (C.c_int, [_VP, _I64, _I64, _I64, _VP, _VP]),
    "cf_group_quad_check_args": (C.c_int, [_I64, _I32, _VP, _I64, _I64, _VP, _I64]),
    "cf_group_quad_device": (C.c_int, [_VP, _VP, _I64, _I64, _VP, _I64, _VP]),
    "cf_reweight_check_args": (C.c_int, [_VP, _I64, _I64, _I32, _VP, _I64, _I32, _VP, _VP]),
    "cf_reweight_device": (C.c_int, [_VP, _I64, _I64, _I32, _VP, _VP, _I64, _I32, _VP, _VP, _VP]),
    "cf_rep_check_args": (C.c_int, [_I64, _I64, _I32, _I32, _I32, _I32, _I32]),
    "cf_rep_key": (C.c_uint64, [C.c_uint64, C.c_uint64, _I32, _I32]),
    "cf_rep_kde_prepare": (C.c_int, [_VP, _I64, _I64, _I32, _I32, _I32, _VP, C.c_uint64, _I32, _VP, _VP, _VP]),
    "cf_rep_propose": (C.c_int, [_I32, _VP, _I64, _I64, _I32, _I32, _I32, _VP, C.c_uint64, _I32, C.c_double, C.c_double, _VP, _VP,
                                 _VP, _VP, _VP]),
    "cf_rep_accept_record": (C.c_int, [_VP, _VP, _VP, _I64, _I64, _I32, _I32, _I32, _VP, C.c_uint64, _I32, _VP, _VP, _VP, _VP, _VP,
                                       _VP, _VP, _VP, _VP, _VP]),
    "cf_rep_swap": (C.c_int, [_VP, _VP, _I64, _I32, _I64, _I32, _VP, _VP, C.c_uint64, _I32, _VP, _VP]),
}


def build(force: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 into libcosmofit_hip.so (in-tree)."""
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", CSRC], check=True, stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64 / libhsa-runtime64 (same
    SONAME as /opt/rocm's); if both copies get loaded the second one sees no GPU.  bench.py and the
    tests use torch for device tensors and torch.distributed, so when torch is installed we bind to
    ITS runtime (whichever of the two is imported first); without torch the RUNPATH (/opt/rocm) applies."""
    import importlib.util

    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is not None and spec.origin:
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)


def lib():
    """Load the shared library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CosmofitError(-2, f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                    "(hipcc --offload-arch=gfx950); there is no CPU implementation to fall back to")
        _preload_hip_runtime()
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in EXPORTS.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        if L.cf_abi_version() != CF_ABI_VERSION:
            raise CosmofitError(-1, "libcosmofit_hip.so ABI version mismatch; rebuild it")
        _lib = L
    return _lib


def check(rc: int):
    if rc != 0:
        raise CosmofitError(rc, lib().cf_last_error().decode(errors="replace"))
