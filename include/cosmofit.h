/*
 * cosmofit.h — C-ABI of the MI355X (gfx950) batched cosmological log-likelihood engine.
 *
 * This is the drop-in boundary for ONE hot path of franciscotln/cosmology-model-fit:
 * the per-walker chi^2 / log-likelihood that emcee / nautilus call through
 * `log_probability(theta)` or `log_probs_vectorized(Theta[W,ndim])`.
 * Plain C types only (pointers + sizes); loadable with ctypes.
 *
 * Reference interfaces each entry point replaces (paths relative to the reference repo):
 *   cf_create            module-level data set-up        sn/pantheon.py:10-19, bao/desi_cmb_des5y.py:14-22
 *   cf_eval              chi_squared / log_likelihood /
 *                        log_probability / *_vectorized  sn/pantheon.py:57-97, bao/desi.py:63-106,
 *                                                        bao/desi_cmb.py:137-143, bao/desi_cmb_des5y.py:138-145
 *   cf_eval_device       the same on device-resident Theta (on-device ensemble; replaces the
 *                        emcee pool.map dispatch          sn/pantheon.py:119-125)
 *   cf_eval_parts        DM_z / mu_theory / mu_corr accessors used by the post-fit plots
 *                                                        sn/pantheon.py:34-54,152-155
 *   cf_eval_table        the (cum_dm, dh_grid) pair inside DM_z / DM_grid  sn/pantheon.py:35-39, bao/desi_cmb_des5y.py:60-66
 *   cf_eval_bao_at       bao_theory(z, qty, params) at ARBITRARY redshifts (post-fit plots)  bao/desi.py:38-56, bao/plot_predictions.py:24-45
 *   cf_eval_hz           H_z(z, params) at arbitrary redshifts (post-fit plots)             ohd/cc.py:95-96, ohd/plot_predictions.py:7-32
 *   cf_eval_fs8_at       fs8_theory(a, params) at arbitrary scale factors (post-fit plots) fs8/fs8.py:84-98,221-226
 *   cf_resid_device      the residual block after the fit: R^2, RMSD, skewness, kurtosis of the residuals, their plot against
 *                        sqrt(diag(cov)) -- for every row of a device chain    sn/pantheon.py:150-201, bao/desi_fs_lya.py:96-141
 *   cf_mock_eval_device  the same likelihood on per-row mock data sets: the Monte-Carlo calibration of the Delta chi^2
 *                        significances the scripts quote  sn/union3_1.py:145-161, sn/pantheon_dipole.py:172
 *   cf_interp_hermite    interp_hermite                   interpolator.py:117-119
 *   cf_interp_pchip      interp_pchip                     interpolator.py:111-114
 *   cf_solve_triangular  solve_triangular (returns y.y)   solve_triangular.py:5-14
 *
 * Error convention: every function returns 0 on success, a negative cf_status otherwise;
 * the message is available through cf_last_error() (thread-local). Nothing throws across
 * the ABI. Numerical convention: theta outside the strict prior box -> -inf for CF_OUT_LOGP
 * (sn/pantheon.py:82-83); a non-finite chi^2 for an in-box theta -> -inf (never NaN: emcee
 * raises ValueError on NaN) and is counted in cf_info.nonfinite_count.
 *
 * Threading: one caller per handle at a time (the reference callers are single-threaded per
 * process). Different handles may be used from different threads.
 *
 * Current device: a handle lives on the device(s) named at cf_create; every function taking a handle
 * switches the calling thread to that device for its own HIP calls and restores the thread's previous
 * current device before it returns. The cf_ens_* functions take device pointers and a stream and launch
 * on the calling thread's current device, which must be the one those belong to.
 */
#ifndef COSMOFIT_H
#define COSMOFIT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CF_ABI_VERSION 11

typedef struct cf_handle cf_handle;

enum cf_status {
  CF_OK = 0,
  CF_ERR_INVALID = -1,   /* bad descriptor / argument */
  CF_ERR_NO_DEVICE = -2, /* no HIP device visible */
  CF_ERR_HIP = -3,       /* a HIP runtime call failed */
  CF_ERR_NOT_POSDEF = -4,/* a zero / negative / non-finite pivot in L */
  CF_ERR_UNSUPPORTED = -5,
  CF_ERR_ILL_CONDITIONED = -6 /* the blocked solve would lose more than 1e-11 relative on this factor */
};

/* Expansion-rate family (a2-a4). */
enum cf_ez_model {
  /* H = H0 * sqrt(Om*(1+z)^3 + (1-Om)*f_DE(z))            sn/pantheon.py:28-31, bao/desi.py:32-35 */
  CF_EZ_LATE_FLAT = 0,
  /* H = H0 * sqrt(Or*zp1^4 + Obc*zp1^3 + Ode*f_DE + Onu*Omnu_z(z)), densities = omega/h^2,
     Ode = 1-Obc-Or-Onu                                   bao/desi_cmb_des5y.py:34-54 */
  CF_EZ_PHYSICAL = 1
};

/* Dark-energy density ratio f_DE(z) (SURVEY section 2 "f_DE(z)"). */
enum cf_fde {
  CF_FDE_LCDM = 0,    /* 1 */
  CF_FDE_WCDM = 1,    /* zp1^(3(1+w0))                        sn/pantheon_and_sh0es.py:26-28 */
  CF_FDE_THAWING = 2, /* (2 zp1^3 / (1+w0+(1-w0) zp1^3))^2    bao/desi.py:26-28 */
  CF_FDE_CPL = 3      /* zp1^(3(1+w0+wa)) exp(-3 wa z/zp1)    bao/desi_fs_lya_cmb.py:19-22 */
};

/* Physical-parameter slots. Each slot is either read from theta[idx]*scale or fixed. */
enum cf_param_slot {
  CF_P_OFFSET = 0, /* M (absolute magnitude) or delta-M offset, subtracted from the SN residual */
  CF_P_H0 = 1,     /* km/s/Mpc; use scale=100 when the sampler parameter is h */
  CF_P_OM = 2,     /* Omega_m (CF_EZ_LATE_FLAT) */
  CF_P_OBH2 = 3,   /* omega_b (CF_EZ_PHYSICAL) */
  CF_P_OCH2 = 4,   /* omega_c (CF_EZ_PHYSICAL) */
  CF_P_W0 = 5,
  CF_P_WA = 6,
  CF_P_V = 7,      /* peculiar-velocity step amplitude in units of 100 km/s (mu_corr) */
  CF_P_RD = 8,     /* sound horizon in Mpc when fixed or free (BAO block) */
  CF_P_FCC = 9,    /* error-rescale factor of the cosmic-chronometer block (default: fixed 1) */
  CF_P_LIN = 10,   /* amplitude of the per-SN linear magnitude term sn_lin_coef[i] (bulk-flow correction of M,
                      bao/desi_cmb_pantheon_H0trgb.py:102-106) */
  CF_P_V2 = 11,    /* second and third velocity components (x 100 km/s) of a direction-dependent peculiar velocity: */
  CF_P_V3 = 12,    /*   v_los,i = n_i . (V, V2, V3)                     sn/pantheon_dipole_xyz.py:50-60 */
  CF_P_S8 = 13,    /* sigma_8(z = 0) of the growth-rate block          fs8/fs8.py:84-98 */
  CF_P_FS8ERR = 14,/* error-rescale factor f_err of the growth-rate block (default: fixed 1)  fs8/fs8.py:116-125 */
  CF_P_NSLOTS = 15
};

typedef struct cf_param {
  int32_t idx;   /* index into theta, or -1 when the slot is fixed / unused */
  int32_t _pad;
  double scale;  /* value = theta[idx]*scale  (scale is applied as `scale*theta`, cf. `100 * h`) */
  double fixed;  /* value when idx < 0 */
} cf_param;

/* BAO quantity codes (bao/desi_cmb_des5y.py:69-79). */
enum cf_bao_qty { CF_BAO_DV = 0, CF_BAO_DM = 1, CF_BAO_DH = 2, CF_BAO_FAP = 3 };

enum cf_bao_dh_mode {
  CF_BAO_DH_PCHIP = 0, /* DH interpolated from the grid with PCHIP  bao/desi_cmb_des5y.py:88 */
  CF_BAO_DH_EXACT = 1  /* DH = c/H(z) evaluated at the datum       bao/desi_cmb.py:54-56 */
};

enum cf_rd_mode {
  CF_RD_PARAM = 0,  /* from slot CF_P_RD (fixed constant or free parameter) */
  CF_RD_FIT = 1     /* r_drag(omega_b, omega_m) fitting formula, coefficients in cf_desc.rd_fit */
};

enum cf_cmb_mode {
  CF_CMB_NONE = 0,
  CF_CMB_R_LA_WB = 1,   /* (R, l_A, omega_b) 3-vector x 3x3 inverse cov   bao/desi_cmb_des5y.py:126-129 */
  CF_CMB_LA_ONLY = 2,   /* only the l_A component                        bao/desi_des5y_bbn_theta_star.py:110-111 */
  CF_CMB_THETA_WB_WM = 3 /* (100 theta*, omega_b, omega_m)               cmb/data_early_lcdm_compression.py:198-207 */
};

/* How chi^2 = || L^-1 Delta ||^2 is evaluated (both on FP64 matrix cores; solve_triangular.py:5-14). */
enum cf_solve_mode {
  CF_SOLVE_BLOCKED_TRSM = 0, /* blocked forward substitution, one workgroup per 16-walker panel: 256-row block rows,
                                diagonal blocks through their host-computed inverses */
  CF_SOLVE_INVERSE_GEMM = 1, /* triangular GEMM against X = L^-1 (inverted once on the host in extended precision,
                                probed against row-by-row substitution at cf_create): no dependency between row
                                blocks, so the matrix cores stay busy for large batches and a batch of 1..2048
                                walkers (log_evidence.py:20-46, small emcee ensembles) spreads over the whole chip */
  CF_SOLVE_AUTO = 2          /* CF_SOLVE_INVERSE_GEMM when its probe passes (<= 1e-11 relative), otherwise
                                CF_SOLVE_BLOCKED_TRSM; cf_info.solve_mode tells which one is in effect */
};

/* Output selector for cf_eval*. */
enum cf_out {
  CF_OUT_CHI2 = 0, /* chi^2 */
  CF_OUT_LOGL = 1, /* -0.5 chi^2                                  (nautilus: likelihood only) */
  CF_OUT_LOGP = 2  /* log prior + log L, -inf outside the box     (emcee log_probability) */
};

typedef struct cf_gauss_prior {
  int32_t idx;   /* theta index */
  int32_t _pad;
  double mean;
  double sigma;  /* term: -0.5*(theta[idx]-mean)^2/sigma^2        sn/pantheon.py:85
                    zero or not finite: refused by cf_create (CF_ERR_INVALID) */
} cf_gauss_prior;

/*
 * Immutable likelihood descriptor. All arrays are host pointers, copied at cf_create and
 * free to be released as soon as it returns.
 */
typedef struct cf_desc {
  int32_t abi_version;  /* CF_ABI_VERSION */
  int32_t struct_size;  /* sizeof(cf_desc) as seen by the caller */
  int32_t device;       /* HIP device ordinal */
  int32_t ndim;         /* length of one theta row */

  int32_t ez_model;     /* cf_ez_model */
  int32_t fde;          /* cf_fde */
  int32_t n_grid;       /* G, points of the uniform z grid (4000 in every reference script) */
  int32_t _pad0;
  double z_max;         /* grid = linspace(0, z_max, G)            sn/pantheon.py:16 */
  double c_km_s;        /* speed of light in km/s                  sn/pantheon.py:12 */

  cf_param param[CF_P_NSLOTS];

  /* ---- SN block (may be absent: n_sn = 0) ---- */
  int64_t n_sn;
  const double* sn_z_cmb;   /* [n_sn] */
  const double* sn_z_hel;   /* [n_sn] */
  const double* sn_obs;     /* [n_sn] m_b or mu */
  const double* sn_step;    /* [n_sn] per-SN sign/weight s_i multiplying 100*v/c in z_cosmo; NULL -> use z_turn */
  double sn_z_turn;         /* s_i = +1 if z_cmb <= z_turn else -1     sn/pantheon.py:46 */
  const double* sn_chol;    /* [n_sn*ld] row-major lower Cholesky factor; ONLY L[i][j<=i] is read
                               (cho_factor leaves garbage above the diagonal, sn/pantheon.py:14) */
  int64_t sn_chol_ld;       /* row stride of sn_chol in elements (>= n_sn) */

  /* ---- BAO block (n_bao = 0 -> absent) ---- */
  int32_t n_bao;
  int32_t bao_dh_mode;      /* cf_bao_dh_mode */
  int32_t rd_mode;          /* cf_rd_mode */
  int32_t _pad1;
  const double* bao_z;      /* [n_bao] */
  const double* bao_val;    /* [n_bao] */
  const int32_t* bao_qty;   /* [n_bao] cf_bao_qty */
  const double* bao_inv_cov;/* [n_bao*n_bao] row-major explicit inverse */
  double rd_fit[11];        /* r_drag coefficients b, m, a1..a9     cmb/data_planck_act_compression.py:102-124 */

  /* ---- compressed-CMB block ---- */
  int32_t cmb_mode;         /* cf_cmb_mode */
  int32_t n_gl;             /* Gauss-Legendre nodes (100) */
  const double* gl_x;       /* [n_gl] nodes on [-1,1]   (np.polynomial.legendre.leggauss) */
  const double* gl_w;       /* [n_gl] weights */
  double cmb_prior[3];
  double cmb_inv_cov[9];
  double zstar_fit[11];     /* z_star: s1, s2, b, m, then e0, c1, e1, e2, c2, e3, e4 of
                               wm^e0 + s1 c1 wb^e1 wm^e2 + s2 c2 wm^e3 wb^e4 (wb, wm raised to b, m first)
                               cmb/data_planck_act_compression.py:86-99 */
  double o_gamma_h2;        /* photon density for R_b                 cmb/...:29 */

  /* ---- radiation + massive neutrino constants (CF_EZ_PHYSICAL) ---- */
  double or_h2;             /* cmb.Or_h2 */
  double omnu_h2;           /* cmb.Omnu_h2 */
  double nu_m0;             /* m0 */
  double nu_rho0;           /* rho0 */
  double nu_qs_sq[5];       /* qs**2 */
  double nu_ws[5];          /* weights */

  /* ---- priors (CF_OUT_LOGP only) ---- */
  const double* bounds;     /* [ndim*2] (lo,hi) strict box; NULL -> no box */
  int32_t n_gauss;
  int32_t cpl_wall;         /* 1: w0+wa >= 0 -> -1e8             bao/desi_fs_lya_cmb.py:118-121 */
  const cf_gauss_prior* gauss; /* [n_gauss] Gaussian terms added to the log-prior */
  /* Gaussian terms added to chi^2 itself (e.g. BBN omega_b, bao/desi_des5y_bbn_theta_star.py:139) */
  int32_t n_chi2_gauss;
  int32_t _pad2;
  const cf_gauss_prior* chi2_gauss;

  /* ---- SN block extension: fixed distance moduli (SH0ES Cepheid hosts) ---- */
  const double* sn_fixed_mu; /* [n_sn] or NULL; entry NaN -> mu_theory, else this value replaces
                                25 + 5 log10((1+z_hel) DM)          sn/pantheon_and_sh0es.py:63-69 */

  /* ---- cosmic-chronometer block (n_cc = 0 -> absent)  bao/desi_union3_cc_theta_star.py:129-139 ----
   * chi2_cc = (H_obs - H(z))^T inv_cov (H_obs - H(z)) * f_cc^2 and
   * log L -= 0.5 * (n_cc ln(2 pi) + logdet - 2 n_cc ln f_cc) */
  int32_t n_cc;
  int32_t _pad3;
  const double* cc_z;       /* [n_cc] */
  const double* cc_h;       /* [n_cc] km/s/Mpc */
  const double* cc_inv_cov; /* [n_cc*n_cc] */
  double cc_logdet;         /* ln det of the CC covariance */

  int32_t solve_mode;       /* cf_solve_mode */
  int32_t _pad4;
  double probe_limit;       /* acceptance limit of the create-time accuracy probe of the packed factor (relative chi^2
                               discrepancy against row-by-row substitution on three probe vectors); 0 = the default 1e-11.
                               A smaller value makes CF_SOLVE_AUTO fall back to the blocked solve earlier. */

  /* ---- several GPUs behind one handle (the sampler stays in ONE host process, sn/pantheon.py:119-125) ----
   * n_devices = 0: the single ordinal `device`.  n_devices > 0: `devices[n_devices]` HIP ordinals; the data and the
   * packed factor are replicated on each at cf_create, cf_eval splits the rows of theta contiguously over them (one
   * host thread + one stream per device, disjoint slices of `out`), results are bit-identical to one device.
   * n_devices = -1: every visible device.  An ordinal may repeat (two replicas on one GPU).  cf_eval_device needs a
   * single-device handle. */
  int32_t n_devices;
  int32_t _pad5;
  const int32_t* devices;

  /* ---- parameterisation variants of the scripts ("Physics variants") ---- */
  int32_t om_mode;          /* 0: Omega_m = slot CF_P_OM; 1: slot CF_P_OM is omega_m = Omega_m h^2 and
                               Omega_m = omega_m / (H0/100)^2          bao/desi_omh2.py:18-20 */
  int32_t rd_wm_mode;       /* matter density handed to the r_drag fit (CF_RD_FIT): 0 = omega_b + omega_c + omega_nu (physical
                               densities, bao/desi_cmb_des5y.py:84-85); 1 = Omega_m (H0/100)^2 of the late-time flat model with
                               omega_b from slot CF_P_OBH2                bao/desi_bbn.py:46-60 */
  const double* sn_lin_coef;/* [n_sn] or NULL: the SN offset becomes offset + theta_LIN * sn_lin_coef[i]; with
                               sn_lin_coef[i] = 100 (5/ln 10) / (c z_cmb,i) this is the linearised bulk-flow magnitude
                               term                                    bao/desi_cmb_pantheon_H0trgb.py:102-106 */
  const double* sn_dir;     /* [n_sn*3] or NULL: unit vectors n_i; then the peculiar velocity of SN i is
                               100 * (n_i . (V, V2, V3)) * sn_step[i] km/s (sn_step = attenuation x survey mask)
                                                                       sn/pantheon_dipole_xyz.py:50-60 */

  /* ---- growth-rate block f sigma_8(z) (n_fs8 = 0 -> absent)  fs8/fs8.py:64-125, bao/desi_cmb_union3_fs8.py:147-207 ----
   * delta'' = -(3/a + E'/E) delta' + (3/2) Omega_m delta / (a^5 E^2) from a_init (delta = a, delta' = 1) to a = 1, with
   * Omega_m = slot OM (CF_EZ_LATE_FLAT) or (omega_b + omega_c)/h^2 (CF_EZ_PHYSICAL);
   * theory_k = (sigma_8 / delta(1)) a_k delta'(a_k) / q_k,  q_k = H(z_k) D_M(z_k) / fs8_fid[k]  (Alcock-Paczynski);
   * chi2_fs8 = f_err^2 (val - theory)^T inv_cov (val - theory)  and  log L += n_fs8 ln f_err.
   * The reference integrates with scipy's adaptive RK45 at rtol = 1e-6; here a fixed-step RK4 in ln a: fs8_steps steps, rounded
   * up to 256, 512, 1024 (0 = default) or 2048 (256 lanes per walker, 1-8 steps per lane; the ODE is linear, so the steps are
   * 2 x 2 matrices combined by a parallel scan): the two agree to the reference's own integration error (~1e-6 relative on theory);
   * against the reference's equation integrated to convergence the default leaves < 1e-9 on the theory (fs8_n_agrid below). */
  int32_t n_fs8;
  int32_t fs8_steps;
  const double* fs8_z;      /* [n_fs8] */
  const double* fs8_val;    /* [n_fs8] */
  const double* fs8_inv_cov;/* [n_fs8*n_fs8] */
  const double* fs8_fid;    /* [n_fs8] H_fid(z_k) D_M,fid(z_k) in the units H(z) D_M(z) has for this descriptor */
  double logl_const;        /* constant added to log L (CF_OUT_LOGL / CF_OUT_LOGP): Gaussian normalisations a script keeps in its
                               log-likelihood, e.g. -0.5 (N ln 2 pi + logdet) of the growth-rate block, fs8/fs8_cmb.py:20,181-183 */
  double fs8_a_init;        /* 10^-2.15 (fs8/fs8.py:79), 10^-2.7 (bao/desi_cmb_union3_fs8.py:168), 1/201 (ohd/cc_fs8.py:86-87) */

  /* ---- further per-script conventions ---- */
  int32_t sn_vel_mode;      /* 0: z_cosmo = -1 + (1 + z_cmb) / (1 + z_pec)                         sn/pantheon.py:43-48
                               1: z_cosmo = max((1 + z_cmb) (1 + z_pec) - 1, 1e-8)                 bao/desi_pantheon_cc.py:84-90 */
  int32_t cc_f_mode;        /* 0: chi2_cc * f_cc^2, log L += n_cc ln f_cc  (f_cc divides the errors, bao/desi_union3_cc_theta_star.py:129-139)
                               1: chi2_cc * f_cc^-2, log L -= n_cc ln f_cc (f_cc multiplies them)   ohd/cc_pantheon.py:64,92 */
  int32_t prior_norm_mode;  /* 0: log prior inside the box = -sum log(hi - lo) (sn/pantheon.py:77); 1: 0.0 (ohd/cc_cmb.py:70-73) */
  int32_t fs8_n_agrid;      /* growth block: 0 = delta'(a_k) read from the integration directly; N >= 4 = as the scripts do, by interp_pchip
                             * of delta' sampled on a_span = np.logspace(log10 fs8_a_init, 0, N) (fs8/fs8.py:79-98: N = 1000;
                             * bao/desi_cmb_union3_fs8.py:169: 2500; ohd/cc_fs8.py:87: 1000; fs8/fs8_cmb.py:129: 5000) */
} cf_desc;

typedef struct cf_info {
  int64_t n_sn;
  int64_t n_sn_pad;        /* rows after padding to the 16-row MFMA tile */
  int64_t packed_chol_bytes;
  int64_t workspace_bytes; /* current device workspace (grows with W) */
  int64_t max_walkers;     /* walkers the current workspace holds */
  int64_t nonfinite_count; /* in-box evaluations whose chi^2 was not finite since create */
  int32_t device;
  int32_t cu_count;
  char gcn_arch[64];
  double pack_probe_rel;   /* |chi2(packed streams) - chi2(row-by-row substitution)| / chi2 on a probe vector,
                              measured on the host at cf_create (refused above 1e-11) */
  int32_t solve_mode;      /* cf_solve_mode in effect (never CF_SOLVE_AUTO) */
  int32_t n_devices;       /* replicas behind this handle (1 unless cf_desc.n_devices asked for more) */
  int32_t devices[16];     /* their HIP ordinals (the first 16) */
} cf_info;

int cf_device_count(void);
const char* cf_last_error(void);
int cf_abi_version(void);

int cf_create(const cf_desc* desc, cf_handle** out);
void cf_destroy(cf_handle* h);
int cf_get_info(cf_handle* h, cf_info* info);

/* Host buffers. theta: [W*ndim] C-order float64; out: [W] float64. Synchronous.  A handle created over several
 * devices (cf_desc.n_devices) splits the rows as cf_split_rows says, one host thread and one stream per device; this is
 * what lets a sampler that lives in one host process (emcee / nautilus with a vectorised callback, sn/pantheon.py:119-125,
 * bao/desi.py:100-129) use every GPU of the node. */
int cf_eval(cf_handle* h, const double* theta, int64_t W, double* out, int32_t out_kind);

/* Rows [*begin, *end) of a W-walker batch that replica k of n evaluates: contiguous, whole 32-walker panels, sizes
 * differing by at most one panel.  Pure host arithmetic (no device needed). */
void cf_split_rows(int64_t W, int32_t n, int32_t k, int64_t* begin, int64_t* end);

/* Device buffers on the handle's device; asynchronous on `hip_stream` (a hipStream_t; NULL = HIP's
 * default stream, which is what torch.cuda.current_stream().cuda_stream reports as 0), ordered like any
 * other work on that stream. Grows the workspace if needed (then it synchronises once).
 * A handle owns ONE workspace (residual rows, chi^2 shares, arrival counters): evaluations of one handle are
 * ordered with respect to each other by the library -- on one stream by that stream; when an evaluation arrives on a
 * DIFFERENT stream than the handle's previous one (cf_eval and the accessors run on a stream the handle owns), the
 * library first waits ON THE HOST until the previous evaluation has drained (hipDeviceSynchronize if that one ran on
 * a caller's stream: the caller's stream handle is never passed back to HIP, so it may be destroyed at any time after
 * the call that used it).  Hence: calls that stay on one stream are purely asynchronous and capturable into a
 * hipGraph; the FIRST call after a stream switch blocks the host and is illegal while `hip_stream` is capturing.
 * For concurrent evaluations create one handle per stream. */
int cf_eval_device(cf_handle* h, const double* d_theta, int64_t W, double* d_out,
                   int32_t out_kind, void* hip_stream);

/* Intermediates for plots/tests. Any output pointer may be NULL. Host buffers.
 *   dm_obs [W*n_sn]  DM(z_cmb)           sn/pantheon.py:58
 *   mu_corr[W*n_sn]                      sn/pantheon.py:43-49
 *   delta  [W*n_sn]  residual vector     sn/pantheon.py:59-60
 *   chi2_blocks[W*10] (chi2_sn, chi2_bao, chi2_cmb, cmb distance vector[3], chi2_cc, chi2_fs8, z_star, r_drag: the two
 *                     fitting formulae as the blocks evaluated them, 0 where no block needs them;
 *                     cmb/data_planck_act_compression.py:86-124, the blobs of cmb/cmb.py:45-58)
 *                                        bao/desi_cmb_des5y.py:126-141, cmb/data_planck_act_compression.py:200-212
 *   bao_theory[W*n_bao]                  bao/desi_cmb_des5y.py:82-100
 *   fs8_theory[W*n_fs8]                  fs8_theory(a, theta) before the Alcock-Paczynski division, fs8/fs8.py:84-98 */
int cf_eval_parts(cf_handle* h, const double* theta, int64_t W, double* dm_obs, double* mu_corr,
                  double* delta, double* chi2_blocks, double* bao_theory, double* fs8_theory);

/* The distance table of W <= 4096 walkers on the reference's grid z_grid = linspace(0, z_max, G): cum_dm[W*G] (the
 * cumulative trapezoid of c/H) and dh[W*G] (c/H at the nodes), host buffers -- the pair that DM_z(params, z) of the
 * scripts hands to interp_hermite (sn/pantheon.py:34-40, bao/desi_cmb_des5y.py:60-66), for the post-fit plots that
 * evaluate distances at arbitrary redshifts (sn/pantheon.py:152-155). */
int cf_eval_table(cf_handle* h, const double* theta, int64_t W, double* cum_dm, double* dh);

/* bao_theory(z, qty, params) of the scripts for ONE theta at n arbitrary (redshift, quantity code) pairs -- what the post-fit
 * block hands to plot_bao_predictions as a smooth curve (bao/plot_predictions.py:24-45, bao/desi.py:38-56, :204-211): the
 * handle's own E(z) model, D_H convention (PCHIP or c / H) and sound horizon (slot, fixed or fitted), evaluated by the same
 * kernels as the BAO block of the likelihood.  qty: 0 D_V / r_d, 1 D_M / r_d, 2 D_H / r_d, 3 F_AP.  Host buffers. */
int cf_eval_bao_at(cf_handle* h, const double* theta, const double* z, const int32_t* qty, int64_t n, double* out);

/* H_z(z, params) of the scripts in km/s/Mpc for ONE theta at n arbitrary redshifts: the curve and the residuals of
 * plot_cc_predictions (ohd/plot_predictions.py:7-32, ohd/cc.py:95-101, bao/desi_cc.py:193-199).  Host buffers. */
int cf_eval_hz(cf_handle* h, const double* theta, const double* z, int64_t n, double* out);

/* fs8_theory(a, params) of the growth-rate scripts -- f sigma_8 before the Alcock-Paczynski division -- for ONE theta at n
 * arbitrary redshifts z = 1 / a - 1 with a_init <= a <= 1: the smooth curve of fs8/plot_predictions.py:7-32
 * (fs8/fs8.py:221-226).  The handle must have a growth-rate block (its a_init, E(z) model and sigma_8 slot are used). */
int cf_eval_fs8_at(cf_handle* h, const double* theta, const double* z, int64_t n, double* out);

/* Per-kernel timing with HIP events recorded on the stream the kernels are launched on.
 * cf_enable_timing(h, slots): keep events for the last `slots` evaluation calls (0 = off, the
 * default) and reset the call counter.  cf_kernel_ms(h, call, t): t[0] = distance + residual
 * kernel (and the small-blocks kernel of a joint likelihood), t[1] = solve + chi^2 kernel of evaluation number `call` (0-based since
 * cf_enable_timing); waits for that call.  cf_last_kernel_ms = the most recent call. */
int cf_enable_timing(cf_handle* h, int slots);
/* record the events on every `stride`-th evaluation only (default 1): sampled timing of a long loop */
int cf_set_timing_stride(cf_handle* h, int stride);
int64_t cf_timed_calls(cf_handle* h);
int cf_kernel_ms(cf_handle* h, int64_t call, float t[2]);
/* the same with the per-walker stage split: t[0] = walker_kernel, t[1] = small-block (+ growth) kernels, t[2] = solve kernel */
int cf_kernel_ms3(cf_handle* h, int64_t call, float t[3]);
int cf_last_kernel_ms(cf_handle* h, float t[2]);
/* Which form of the per-walker kernel cf_eval / cf_eval_device run for a batch of W walkers: 0 = one workgroup per walker,
 * 1 = streaming (one wave per walker, large batches; the same bits), 2 = the generic kernel.  Negative: an error code.
 * CF_TUNE walker_stream=0|1 forces the choice between 0 and 1 where both are allowed. */
int cf_walker_form(cf_handle* h, int64_t W);
/* The wave priority (0 .. 3) the streaming form takes at the top of each of its at most eight grid segments, as in effect for
 * this handle: it falls from 3 to 0 as the share of a walker's work already done rises (a function of the SNe per segment alone),
 * so that the waves sharing a SIMD finish together; no result depends on it.  All zeros under CF_TUNE walker_level=0, for a grid
 * of one segment and for data the streaming form does not take.  The table goes with batches of at most one round of the chip
 * (16 walkers per CU: 4096 on 256 CUs); a larger batch runs every wave at priority 0.  An unknown CF_TUNE key is silently
 * ignored: this is how to see that the key took effect. */
int cf_walker_levels(cf_handle* h, int32_t out[8]);
/* The launch-time form of the inverse-GEMM solve (CF_SOLVE_INVERSE_GEMM only; the blocked solve has one form) for a batch of W
 * walkers over an SN factor of n_sn rows: a pure function of n_sn, W and the process's CF_TUNE -- no handle, no device -- computed
 * by the helpers the launch itself uses.  out[0] kernel (0 small-batch, 1 throughput), [1] walkers per panel (16 or 32), [2] tiles
 * per workgroup of the small-batch kernel (1 or 2; 0 for throughput), [3] row blocks of 64 rows, [4] 16-row tiles of the last row
 * block that hold rows of the factor (1..4; only the throughput kernel skips the others), [5] row-block levels worked as half
 * units, [6] panel groups, [7] panels per group, [8] snake order of the row blocks (0 / 1), [9] workgroups launched.  [5]..[8]
 * are 0, 1, the number of panels, 0 for the small-batch kernel.  An unknown CF_TUNE key is silently ignored: this is how to see
 * that a key took effect.  n_sn in 1..2^20, W >= 1, otherwise CF_ERR_INVALID. */
int cf_solve_form(int64_t n_sn, int64_t W, int32_t out[10]);
/* 1: the per-walker stage writes the residuals of a batch of W walkers in the small-batch solve kernel's fragment order, 0: in
 * walker rows (every batch of the throughput solve kernel; likelihoods that take the generic per-walker kernel; CF_TUNE
 * small_frag=0).  A property of the handle; the result is the same bits either way.  Negative: an error code. */
int cf_solve_frag_order(cf_handle* h, int64_t W);
/* The launch form of the small-blocks kernel (z* / r_drag fits, compressed CMB, cosmic chronometers, BAO) for a batch of W
 * walkers under the process's CF_TUNE: lanes per walker + 256 * waves per walker -- 272 = sixteen lanes (W > sb_wide_max, default
 * 2048), 320 = one wave (only with sb_roles_max below W), 576 = two waves (the default up to 2048 walkers); the same bits in all
 * three.  0: the handle has none of these blocks (or is a quasar handle).  Negative: an error code (null handle, W < 1). */
int cf_small_blocks_form(cf_handle* h, int64_t W);
/* Debug query: the SN residual buffer as the per-walker kernel of the handle's most recent evaluation left it (the solve only reads
 * it).  Waits for the handle's stream, then copies the first ceil(W / 16) * 16 * n_ld doubles to `out`, raw, and sets *layout to the
 * layout that evaluation was launched with: 0 = walker rows (walker w at w * n_ld; rows n_sn .. n_ld - 1 are zero padding), 1 = the
 * small-batch solve's fragment order, where element (w, i) sits at
 *   (w >> 4) * 16 * n_ld + (i >> 3) * 128 + ((i >> 1) & 3) * 32 + 2 * (w & 15) + (i & 1).
 * n_ld = n_sn rounded up to a multiple of 64.  CF_ERR_INVALID: a null argument, a handle without an SN block, a W that is not the
 * batch size of the last evaluation (or no evaluation yet); CF_ERR_UNSUPPORTED: a handle on several devices, a quasar handle. */
int cf_last_residuals(cf_handle* h, int64_t W, double* out, int32_t* layout);

/* ---- stand-alone operators with the reference's signatures (host buffers) ---- */
/* out[k] = Hermite(xq[k]; x, y, y_prime), linear extrapolation outside   interpolator.py:117-119 */
int cf_interp_hermite(const double* xq, int64_t nq, const double* x, const double* y,
                      const double* y_prime, int64_t n, double* out);
/* out[k] = PCHIP(xq[k]; x, y), clamped outside                             interpolator.py:111-114 */
int cf_interp_pchip(const double* xq, int64_t nq, const double* x, const double* y, int64_t n,
                    double* out);
/* out[w] = || L^-1 b_w ||^2 for nrhs right-hand sides b[nrhs*n] (row w = b_w)  solve_triangular.py:5-14 */
int cf_solve_triangular(const double* L, int64_t n, int64_t ld, const double* b, int64_t nrhs,
                        double* out);

/* Host-only self-test of the factor packing (validates the fragment streams the solve kernel
 * consumes by replaying them for one right-hand side).  For the CPU test-suite; no evaluation
 * entry point ever calls it. */
int cf_selftest_pack_host(const double* L, int64_t n, int64_t ld, const double* b, double* chi2_out,
                          int64_t* packed_bytes);

/* The same for the inverse-GEMM packing (explicit inverse); probe_out (may be NULL) receives the value
 * cf_create compares with 1e-11. */
int cf_selftest_invpack_host(const double* L, int64_t n, int64_t ld, const double* b, double* chi2_out,
                             double* probe_out);

/* Device self-tests of the two in-kernel log10 routines: out[k] = log10(x[k]).  cf_selftest_log10: the <= 1 ulp
 * routine of the accessor / calibrator paths (mu_corr = 5 log10 of a ratio near 1); cf_selftest_log10_tab: the
 * table-driven routine of the production SN loop (absolute error ~2e-16 max(1, |log10 x|)). */
int cf_selftest_log10(const double* x, int64_t n, double* out);
int cf_selftest_log10_tab(const double* x, int64_t n, double* out);
/* The table-driven exp of the wCDM / CPL table build (|x| < ~700, no special cases): out[k] = exp(x[k]), <= 1.5 ulp. */
int cf_selftest_exp_tab(const double* x, int64_t n, double* out);
/* sqrt / quotient of the compressed-CMB Gauss-Legendre nodes (positive, finite, normal operands: the library routines' instruction
 * sequences without their exponent scaling and class selects): out[4 k .. 4 k + 3] = {sqrt_pos(a[k]), the library's sqrt(a[k]),
 * div_pos(a[k], b[k]), the library's a[k] / b[k]}, all on the device -- the pairs must be the same bits. */
int cf_selftest_pos_ops(const double* a, const double* b, int64_t n, double* out);

/* ---- Device-resident ensemble moves (the sampler side of sn/pantheon.py:108-125: emcee with KDEMove 30 % +
 * DEMove 70 %, StretchMove by default elsewhere).  All pointers are device pointers on the current device, all
 * calls are asynchronous on `hip_stream`.
 * Splits (emcee's RedBlueMove: `nsplits` sets updated in turn, each proposing from the union of the others): n_splits = 2 for
 * the stretch and KDE moves, 3 for the DE move (emcee's DEMove sets nsplits = 3).  Walkers are taken in consecutive groups of
 * n_splits: walker n_splits c + b belongs to split perm_c[b], where perm_c is the identity for split_key = 0 (fixed classes
 * index mod n_splits) and otherwise a counter-based random permutation of (split_key, c) -- the splits are re-drawn every step
 * (emcee shuffles its index array) while every split still holds one member of every group, so every process keeps its fair
 * share of each split.  d_all_pos [w_total * ndim] holds every walker's position (after the all-gather of a sharded
 * ensemble), d_ids [n_active] the global indices of the active walkers this process owns, and the complementary set of
 * split `split` is every walker of the other splits in ascending index order.  Random numbers are counter-based: key0 = the
 * 64-bit key of stream 0 for this (seed, step, split) (cosmology-model-fit_amd/ensemble.py: stream_key), so a chain does not
 * depend on how the walkers are sharded over processes.
 *   cf_ens_active_count / cf_ens_comp_count: HOST functions (no device needed): the number of walkers of split `split` in the
 *     shard [shard_start, shard_stop), and the size of its complementary set in an ensemble of w_total walkers; -1 on bad arguments.
 *   cf_ens_active_set: the active walkers of split `split` that the shard [shard_start, shard_stop) owns, ascending:
 *     d_ids [cf_ens_active_count] global indices, d_local_idx = d_ids - shard_start.
 *   cf_ens_kde_prepare: Silverman-bandwidth Gaussian KDE of the complementary set: d_params [2 ndim^2 + 1] =
 *     {chol (lower), inv(chol)^T, log normalisation}, d_wc [cf_ens_comp_count * ndim] = whitened complementary positions.
 *     CF_ERR_INVALID, before anything is launched, when cf_ens_comp_count <= ndim (the covariance would be singular).
 *   cf_ens_propose: kind 0 stretch (scale a), 1 differential evolution (gamma0 = 2.38 / sqrt(2 ndim), jitter de_sigma),
 *     2 KDE independence proposal; d_y [n_active * ndim], d_log_factor [n_active] = log Hastings factor.
 *   cf_ens_accept: accept with probability min(1, exp(log_factor + lp_new - lp_old)) (NaN never accepts); updates
 *     d_x_local / d_logp_local at d_local_idx [n_active] and adds the number of accepted moves to *d_n_accepted. */
int64_t cf_ens_active_count(uint64_t split_key, int32_t n_splits, int32_t split, int64_t shard_start, int64_t shard_stop);
int64_t cf_ens_comp_count(uint64_t split_key, int32_t n_splits, int32_t split, int64_t w_total);
int cf_ens_active_set(uint64_t split_key, int32_t n_splits, int32_t split, int64_t shard_start, int64_t shard_stop,
                      int64_t* d_ids, int64_t* d_local_idx, void* hip_stream);
int cf_ens_kde_prepare(const double* d_all_pos, int64_t w_total, int32_t ndim, int32_t n_splits, int32_t split,
                       uint64_t split_key, double* d_params, double* d_wc, void* hip_stream);
int cf_ens_propose(int32_t kind, const double* d_all_pos, int64_t w_total, int32_t ndim, int32_t n_splits, int32_t split,
                   uint64_t split_key, const int64_t* d_ids, int64_t n_active, uint64_t key0, double a, double de_sigma,
                   const double* d_kde_params, const double* d_kde_wc, double* d_y, double* d_log_factor,
                   void* hip_stream);
int cf_ens_accept(const int64_t* d_ids, const int64_t* d_local_idx, int64_t n_active, int32_t ndim, uint64_t key0,
                  const double* d_y, const double* d_lp_new, const double* d_log_factor, double* d_x_local,
                  double* d_logp_local, uint64_t* d_n_accepted, void* hip_stream);
/* cf_ens_accept_record: cf_ens_accept (same d_x_local / d_logp_local / *d_n_accepted bits) that also records the step for
 * a chain.  For every active walker it writes the walker's row after the accept to d_chain_slot [W_local * ndim] and its
 * log P to d_logp_slot [W_local] at its local index, and adds its accept bit (0 / 1) to d_walker_accepted [W_local].
 * Every walker is active in exactly one split of a step and no later split of the step moves it, so the accepts of one
 * step's splits write every slot row once: the end-of-step state.  d_chain_slot and d_logp_slot are both null (count
 * only) or both set; d_walker_accepted may be null (no per-walker counts). */
int cf_ens_accept_record(const int64_t* d_ids, const int64_t* d_local_idx, int64_t n_active, int32_t ndim, uint64_t key0,
                         const double* d_y, const double* d_lp_new, const double* d_log_factor, double* d_x_local,
                         double* d_logp_local, uint64_t* d_n_accepted, double* d_chain_slot, double* d_logp_slot,
                         int64_t* d_walker_accepted, void* hip_stream);

/* ---- Replica ensembles (csrc/cosmofit_replica.hip): R independent ensembles of w walkers each, stepped together by the
 * launches of one split update, with an optional inverse temperature per replica and swaps between the rungs of a ladder.
 * All pointers are device pointers on the current device, all launches are asynchronous on `hip_stream`.
 * Layout: d_pos [R * w * ndim], global row r w + l (replica r, local walker l); d_l [R * w] the walkers' log P (the
 * log-LIKELIHOOD in a tempered run).  w is a multiple of n_splits, so every replica has n_act = w / n_splits active walkers per
 * split and nc = w - n_act complementary ones; active row i = r n_act + m is the member of local group m of replica r that
 * belongs to `split`.  Partners come from the walker's own replica only.
 * Random numbers: d_base [R], base_r = mix(seeds[r] * 0x9E3779B97F4A7C15 + 0x5851F42D4C957F2D) (splitmix64 finaliser), uploaded
 * once; the kernels form the keys of ensemble.py's stream_key(seeds[r], step, split, stream) = mix(base_r ^ step) + (split << 8)
 * + stream themselves (no per-step upload), the counter is the local index l, and the split key is stream 254 of (step, 0), or 0
 * for randomize = 0.  Replica r is therefore, bit for bit, the chain of a stand-alone ensemble (cf_ens_*) with seed seeds[r]: the
 * per-element arithmetic and the reduction orders are the same device code.
 *   cf_rep_check_args: HOST function (no device needed), the refusals every entry point applies before it launches: R >= 1,
 *     w even and >= 4, w divisible by n_splits, nc > ndim for kind 2 (KDE), ndim in 1..16, R w < 2^31; T = 0 (no tempering) or
 *     the rungs of a ladder (R a multiple of T, has_bounds required).  CF_ERR_INVALID with the reason in cf_last_error.
 *   cf_rep_key: HOST function, the 64-bit key the kernels form from (base, step, split, stream).
 *   cf_rep_kde_prepare: one 256-thread workgroup per replica; d_params [R * (2 ndim^2 + 1)], d_wc [R * nc * ndim], per replica
 *     as cf_ens_kde_prepare.
 *   cf_rep_propose: kind as cf_ens_propose; d_y [R * n_act * ndim], d_log_factor [R * n_act]; for the KDE move the log-factor
 *     kernel follows in the same call.
 *   cf_rep_accept_record: accept with probability min(1, exp((log_factor + beta l_new) - beta l_old)), beta = d_beta[r] (null:
 *     1, which is cf_ens_accept's expression to the bit); NaN never accepts; with d_lo / d_hi [ndim] (both null: no box) a
 *     proposal that is not strictly inside the box never accepts.  d_beta needs the box.  Adds the accepted moves of replica r to
 *     d_n_accepted[r]; d_chain_slot [R * w * ndim] / d_l_slot [R * w] / d_walker_accepted [R * w] as in cf_ens_accept_record
 *     (slots both null or both set, counts may be null).
 *   cf_rep_swap: R = C T replicas, r = c T + t: for every ladder c and every rung t = parity, parity + 2, ... with t + 1 < T,
 *     walker l of rung t and walker l of rung t + 1 exchange rows and d_l exactly when
 *     log u < (beta_t - beta_{t+1}) (l_{t+1,l} - l_{t,l}), u = the uniform of (stream_key(seeds[c T + t], step, 0, 253), counter
 *     l), d_beta [R]; a NaN difference never swaps.  Adds the accepted swaps to d_n_swapped [C * (T - 1)] at c (T - 1) + t. */
int cf_rep_check_args(int64_t R, int64_t w, int32_t ndim, int32_t n_splits, int32_t kind, int32_t T, int32_t has_bounds);
uint64_t cf_rep_key(uint64_t base, uint64_t step, int32_t split, int32_t stream);
int cf_rep_kde_prepare(const double* d_pos, int64_t R, int64_t w, int32_t ndim, int32_t n_splits, int32_t split,
                       const uint64_t* d_base, uint64_t step, int32_t randomize, double* d_params, double* d_wc, void* hip_stream);
int cf_rep_propose(int32_t kind, const double* d_pos, int64_t R, int64_t w, int32_t ndim, int32_t n_splits, int32_t split,
                   const uint64_t* d_base, uint64_t step, int32_t randomize, double a, double de_sigma, const double* d_params,
                   const double* d_wc, double* d_y, double* d_log_factor, void* hip_stream);
int cf_rep_accept_record(const double* d_y, const double* d_l_new, const double* d_log_factor, int64_t R, int64_t w, int32_t ndim,
                         int32_t n_splits, int32_t split, const uint64_t* d_base, uint64_t step, int32_t randomize,
                         const double* d_beta, const double* d_lo, const double* d_hi, double* d_pos, double* d_l,
                         uint64_t* d_n_accepted, double* d_chain_slot, double* d_l_slot, int64_t* d_walker_accepted,
                         void* hip_stream);
int cf_rep_swap(double* d_pos, double* d_l, int64_t C, int32_t T, int64_t w, int32_t ndim, const double* d_beta,
                const uint64_t* d_base, uint64_t step, int32_t parity, uint64_t* d_n_swapped, void* hip_stream);

/* ---- chain statistics (csrc/cosmofit_chain.hip): emcee's integrated autocorrelation time by direct lag sums ----------------
 * A chain is [n_t, n_s] float64 in device memory, n_s = n_walkers * ndim series side by side (row t holds every series at
 * step t: an emcee chain [n_t, n_w, ndim] as it lies in memory).  Every sum runs in a fixed order (no atomics), so the
 * results are a deterministic function of the chain.
 *   cf_chain_mean: d_mean [n_s] = per-series mean over t.
 *   cf_chain_lagsum: d_out [nlag * n_s], row j = sum_{t < n_t - tau} (x_t - m)(x_{t + tau} - m) at tau = lag0 + j
 *     (a lag >= n_t gives 0).
 *   cf_chain_acf_mean: d_f [nlag * ndim], f[j][d] = (sum over w = 0 .. n_w - 1, ascending, of
 *     d_lagsum[j][w ndim + d] / d_c0[w ndim + d]) / n_w, d_c0 = the lag-0 row. */
int cf_chain_mean(const double* d_x, int64_t n_t, int64_t n_s, double* d_mean, void* hip_stream);
int cf_chain_lagsum(const double* d_x, const double* d_mean, int64_t n_t, int64_t n_s, int64_t lag0, int32_t nlag,
                    double* d_out, void* hip_stream);
int cf_chain_acf_mean(const double* d_lagsum, const double* d_c0, int64_t n_w, int32_t ndim, int32_t nlag, double* d_f,
                      void* hip_stream);

/* ---- marginals (csrc/cosmofit_marginals.hip): the histograms behind a corner plot ------------------------------------------
 * Samples are [n, ndim] float64 in device memory, row-major and contiguous (a flat chain, or weighted posterior points).
 * Limits of both entries: 1 <= n <= 2^31 - 1, 1 <= ndim <= CF_MARG_MAX_NDIM, 1 <= nbins <= CF_MARG_MAX_BINS; anything else
 * returns CF_ERR_INVALID before anything is launched.
 *   cf_marg_bin: d_idx [n * ndim] uint8 = numpy's bin of every value in its column's edges, d_edges [ndim * (nbins + 1)]
 *     float64 in device memory (made on the host by np.linspace(lo, hi, nbins + 1) per column and uploaded, so that they have
 *     numpy's bits; increasing).  Bin i iff edges[i] <= x < edges[i + 1]; the last bin also takes x == edges[nbins]; every
 *     other value (below, above, NaN, +-inf) gets CF_MARG_NOT_COUNTED.  This is np.histogram's and np.histogram2d's rule,
 *     reproduced exactly: the bin is guessed with one multiply and corrected by comparisons with the edges themselves.
 *   cf_marg_hist: from d_idx, the ndim 1-D histograms d_h1 [ndim * nbins] and, for the host list pairs [npairs * 2]
 *     (0 <= npairs <= CF_MARG_MAX_PAIRS, columns in 0 .. ndim - 1, repeats allowed), the 2-D histograms d_h2
 *     [npairs * nbins * nbins]: H[p][i][j] = rows with column pairs[2p] in bin i and column pairs[2p + 1] in bin j
 *     (np.histogram2d's orientation); a row counts if both indices are < nbins.  d_h2 may be null if npairs = 0.
 *     d_w = null: int64 counts.  d_w [n] (weights >= 0, finite; w_max = their maximum > 0, both checked by the caller):
 *     int64 fixed-point sums of q = rint(w / w_max * 2^s), s = 62 - ceil(log2 n), so that no sum can overflow; the caller
 *     multiplies by w_max / 2^s.  All sums are integer sums (LDS and global integer atomics): the same input gives the same
 *     bits on every run, for every n_segments and for every order of the rows.  n_segments (0 .. CF_MARG_MAX_SEGMENTS) is
 *     the number of row segments the work is cut into, one workgroup per (pair, segment); 0 lets the library choose. */
#define CF_MARG_MAX_NDIM 16
#define CF_MARG_MAX_BINS 128
#define CF_MARG_MAX_PAIRS 256
#define CF_MARG_MAX_SEGMENTS 65536
#define CF_MARG_NOT_COUNTED 255
int cf_marg_bin(const double* d_x, int64_t n, int32_t ndim, const double* d_edges, int32_t nbins, uint8_t* d_idx,
                void* hip_stream);
int cf_marg_hist(const uint8_t* d_idx, const double* d_w, double w_max, int64_t n, int32_t ndim, int32_t nbins,
                 const int32_t* pairs, int32_t npairs, int64_t* d_h1, int64_t* d_h2, int32_t n_segments, void* hip_stream);

/* ---- kernel density sums (csrc/cosmofit_kde.hip; the driver is cosmology-model-fit_amd/tension.py) -----------------------
 * All-pairs isotropic Gaussian kernel sums on already whitened points, everything float64 in device memory, row-major:
 *   out[i] = sum over j != self(i) of  w_j exp(-0.5 |q_i - y_j|^2),     sq[i] = the sum of the squares of the same terms
 * d_y [n * ndim] samples, d_w [n] weights (null: all 1), d_q [m * ndim] queries, d_out [m], d_sq [m] (null: not wanted).
 * self_offset = -1: every sample counts.  self_offset >= 0: query i IS sample self_offset + i and that one term is left out
 * inside the loop (exact leave-one-out; nothing is subtracted afterwards).
 * Order of summation: slices of CF_KDE_SLICE consecutive samples, ascending j within a slice, then the slices ascending; so
 * the bits of a row depend on the samples, the weights, the query and self(i) only (not on m, the row's position, the stream
 * or repetition).  Samples are staged CF_KDE_TILE at a time.  A query further than ~37 units from every sample gives exactly
 * 0.0 (exp underflows; no rescaling); a NaN or infinite query coordinate gives NaN in that row only.  Samples and weights
 * must be finite (the caller checks).  CF_ERR_INVALID, before anything is launched, for: ndim outside 1 .. CF_KDE_MAX_NDIM,
 * n < 1, m < 1, a null d_y / d_q / d_out, self_offset < -1, self_offset + m > n.  Device pointers only; the current device. */
#define CF_KDE_MAX_NDIM 8
#define CF_KDE_TILE 256
#define CF_KDE_SLICE 2048
/* launch geometry, stated for tests and tools (it never changes a bit of a result): a workgroup owns CF_KDE_QUERY_BLOCK
 * queries; calls with fewer than CF_KDE_SPLIT_BELOW_BLOCKS query blocks give every slice a workgroup of its own */
#define CF_KDE_QUERY_BLOCK 512
#define CF_KDE_SPLIT_BELOW_BLOCKS 512
int cf_kde_sum_device(const double* d_y, const double* d_w, int64_t n, int32_t ndim, const double* d_q, int64_t m,
                      int64_t self_offset, double* d_out, double* d_sq, void* hip_stream);

/* ---- nested sampling (csrc/cosmofit_nested.hip; the driver is cosmology-model-fit_amd/nested.py) -------------------------
 * Classic nested sampling with batch deletion on a device-resident live set: the per-step work of the constrained
 * differential-evolution walk that replaces the dead points.  Points live in the unit cube; theta = T(u) is the prior
 * transform of cf_ns_prior: lo + u (hi - lo) for CF_NS_UNIFORM (a = lo, b = hi), loc + scale * Phi^-1(u) for CF_NS_NORMAL
 * (a = loc, b = scale).  Arrays are row-major [rows * ndim] float64 device pointers on the current device; every call is
 * asynchronous on `hip_stream`.  Random numbers are the ensemble's counter-based generator: `key` is the 64-bit key of stream
 * 0 for (seed, iteration, walk step) (nested.py: ns_key), stream s has key + s, the counter is the row index.
 *   cf_ns_prior_draw: u[i][k] uniform in (0, 1) from stream k, theta = T(u), for i < n.
 *   cf_ns_transform: theta = T(u) for n rows.
 *   cf_ns_walk_start: walker i < m starts at survivor j = floor(U(stream 0, i) * n_surv): copies its u, theta, log L.
 *   cf_ns_propose: partners a != b of the survivor set (streams 0 and 1), u' = u + gamma (u_a - u_b) + sigma N_k (normal k
 *     from streams 2 + 2k, 3 + 2k); d_ok[i] = 1 and d_ptheta = T(u') if u' lies in the open cube, else d_ok[i] = 0 and
 *     d_ptheta = the walker's current theta (the likelihood never sees a point outside the prior).
 *   cf_ns_accept: walker i takes the proposal iff d_ok[i] and d_plogl[i] is finite and > *d_lstar; d_counts[0..2] +=
 *     accepted, out-of-cube and non-finite proposals (integer atomics only). */
#define CF_NS_MAX_NDIM 16
enum { CF_NS_UNIFORM = 0, CF_NS_NORMAL = 1 };
typedef struct cf_ns_prior {
  int32_t ndim;                   /* 1 .. CF_NS_MAX_NDIM */
  int32_t _pad;
  int32_t kind[CF_NS_MAX_NDIM];   /* CF_NS_UNIFORM / CF_NS_NORMAL */
  double a[CF_NS_MAX_NDIM];       /* lo / loc */
  double b[CF_NS_MAX_NDIM];       /* hi / scale */
} cf_ns_prior;

int cf_ns_prior_draw(const cf_ns_prior* prior, int64_t n, uint64_t key, double* d_u, double* d_theta, void* hip_stream);
int cf_ns_transform(const cf_ns_prior* prior, const double* d_u, int64_t n, double* d_theta, void* hip_stream);
int cf_ns_walk_start(const double* d_su, const double* d_stheta, const double* d_slogl, int64_t n_surv, int32_t ndim, int64_t m,
                     uint64_t key, double* d_wu, double* d_wtheta, double* d_wlogl, void* hip_stream);
int cf_ns_propose(const cf_ns_prior* prior, const double* d_su, int64_t n_surv, int64_t m, uint64_t key, double gamma,
                  double sigma, const double* d_wu, const double* d_wtheta, double* d_pu, double* d_ptheta, int32_t* d_ok,
                  void* hip_stream);
int cf_ns_accept(int64_t m, int32_t ndim, const double* d_lstar, const double* d_pu, const double* d_ptheta,
                 const int32_t* d_ok, const double* d_plogl, double* d_wu, double* d_wtheta, double* d_wlogl,
                 uint64_t* d_counts, void* hip_stream);

/* ---- quasar Hubble-diagram likelihoods (csrc/cosmofit_quasar.hip; the recipes are cosmology-model-fit_amd/quasars.py) ----
 * The quasars/qsr_*.py scripts: Risaliti-Lusso quasars as standard candles with a free intrinsic scatter, alone or joint
 * with SNe and BAO, on an older distance algorithm than the other scripts:
 *   E^2 = Om (1+z)^3 + (1 - Om) f_DE,  f_DE = (n X / (1 + (n - 1) X))^(p (1 + w0)),  X = (1+z)^k;
 *   I(z) = np.interp(z, grid, cumulative_trapezoid(1 / E, grid, initial=0)), grid = linspace(0, top, n_grid);
 *   mu(z) = 25 + 5 log10((1 + z') (c / H0) I(z)),  z' = z, or z_hel for the SN block when sn_zhel = 1;
 *   chi2_q = sum delta^2 / (sigma^2 + s^2),  delta = mu_obs - dM_qsr - mu(z),  log L -= 0.5 sum ln(sigma^2 + s^2);
 *   the SN block is the descriptor's: residual obs - offset - mu(z_cmb), chi2 through its Cholesky factor;
 *   BAO (bao_mode = CF_QSR_BAO_QUAD): D_M(z_i) = c / H0 x the trapezoid of 1 / E on linspace(0, z_i, n_grid) of its own,
 *   D_H = c / H(z_i), D_V = (z D_H D_M^2)^(1/3), all over r_d (slot CF_P_RD); chi2_bao = Delta^T inv_cov Delta.
 * cf_create_quasar takes an ordinary cf_desc for what the scripts share with the rest (ndim, device, c_km_s, slots CF_P_OM,
 * CF_P_W0, CF_P_H0, CF_P_OFFSET (SN offset), CF_P_RD, the SN block, bounds, solve_mode; ez_model CF_EZ_LATE_FLAT, fde, n_grid
 * and z_max are not used by the quasar path, n_bao / cmb / cc / fs8 must be absent) plus this extension.  The result is an
 * ordinary handle: cf_eval, cf_eval_device, timing and cf_destroy work on it; cf_eval_parts, cf_eval_table, cf_eval_bao_at,
 * cf_eval_hz and cf_eval_fs8_at refuse it (CF_ERR_UNSUPPORTED), cf_qsr_eval_parts is its accessor.
 *   CF_OUT_CHI2 = chi2_sn + chi2_q + chi2_bao ("chi squared total" of the scripts), CF_OUT_LOGL = the script's log_likelihood,
 *   CF_OUT_LOGP = its log_posterior (strict box, 0 inside: prior_norm_mode = 1).
 * One device only: a descriptor with n_devices != 0 is refused with CF_ERR_UNSUPPORTED. */
enum cf_qsr_bao_mode { CF_QSR_BAO_NONE = 0, CF_QSR_BAO_QUAD = 1 };
#define CF_QSR_MAX_QSR 65536
typedef struct cf_qsr_ext {
  int32_t struct_size;      /* sizeof(cf_qsr_ext) as seen by the caller */
  int32_t n_grid;           /* nodes of every linspace grid (3000 in the scripts), 16 .. 8192 */
  int64_t n_qsr;            /* 1 .. CF_QSR_MAX_QSR */
  const double* qsr_z;      /* [n_qsr] */
  const double* qsr_mu;     /* [n_qsr] observed distance moduli */
  const double* qsr_sigma;  /* [n_qsr] */
  cf_param qsr_offset;      /* dM_qsr */
  cf_param qsr_scatter;     /* s */
  double fde_n, fde_k, fde_p;  /* (n, k, p) of f_DE */
  double qsr_z_top;         /* top of the quasar grid (max z_qsr in every script) */
  double sn_z_top;          /* top of a separate SN grid (max z_sn), or 0: the SN block reads the quasar grid */
  int32_t sn_zhel;          /* 1: the SN luminosity distance takes (1 + z_hel) */
  int32_t bao_mode;         /* cf_qsr_bao_mode */
  int32_t n_bao;            /* 0 .. 64 */
  int32_t _pad;
  const double* bao_z;      /* [n_bao] */
  const double* bao_val;    /* [n_bao] */
  const int32_t* bao_qty;   /* [n_bao] CF_BAO_DV / CF_BAO_DM / CF_BAO_DH */
  const double* bao_inv_cov;/* [n_bao * n_bao] row-major inverse covariance */
} cf_qsr_ext;

int cf_create_quasar(const cf_desc* desc, const cf_qsr_ext* ext, cf_handle** out);
/* Per-block results of a quasar handle for W host rows, computed by the same kernels as cf_eval.  Any output may be NULL.
 *   chi2_blocks [W * 3]  (chi2_sn, chi2_q, chi2_bao), 0 for an absent block
 *   mu_sn [W * n_sn], mu_qsr [W * n_qsr]  mu at the SN and quasar redshifts;  bao_theory [W * n_bao]  the BAO predictions */
int cf_qsr_eval_parts(cf_handle* h, const double* theta, int64_t W, double* chi2_blocks, double* mu_sn, double* mu_qsr,
                      double* bao_theory);

/* ---- batched box-constrained maximization (csrc/cosmofit_opt.hip; the driver is cosmology-model-fit_amd/optimize.py) -----
 * B independent problems maximise one objective f(theta) inside a box.  A problem lives in box-scaled coordinates
 * u = (theta - lo) / width, u in [delta, 1 - delta]; theta = lo + u width is every row the objective sees.  The n_free
 * coordinates free_idx move (common to all problems); the others keep each problem's start value.  Per iteration:
 *   cf_opt_stencil: for every active problem a (problem d_active[a]) the 2 n_free rows d_rows [(a 2 n_free + 2 j + side) * ndim]:
 *     free slot j perturbed by u +- h (central form 0), u + h, u + 2h (forward form +1, within 2h of the lower face) or
 *     u - h, u - 2h (backward form -1, within 2h of the upper face); writes the forms.
 *   cf_opt_direction: 16 lanes per problem from the stencil values d_fs: the gradient g (free slots), the projected gradient
 *     (a slot at a face with g pointing out of the box is held at 0), its max norm; status CF_OPT_NONFINITE_STENCIL if a
 *     stencil value is not finite, CF_OPT_CONVERGED if the norm <= gtol + gtol_rel |f|; else the BFGS update of H^-1 on -f
 *     (y = g_prev - g zeroed on the held slots; skipped when s.y <= 0 or (s.y)^2 <= 1e-20 |s|^2 |y|^2), d = H^-1 pg
 *     (held slots 0), a reset to sigma I when flagged or when pg.d <= 0 (sigma: the largest move 0.1, or min(0.1, 4 max|s|)
 *     once a step was taken; after a failed search at most 4^-K max|d| of the failed direction), and the K trial rows
 *     d_trials [(a K + k) * ndim] = P(u + 4^-k d) (P clamps to [delta, 1 - delta]; a finished problem gets K copies of u).
 *   cf_opt_accept: one thread per problem from the trial values d_ft: the first k with f_k >= f + c1 g.(u_k - u), else the
 *     best finite f_k; a trial counts only if f_k > f + 4 eps |f|; else a reset next iteration (CF_OPT_NOISE_FLOOR if H^-1
 *     was fresh from a reset after a failed search); n_iter += 1, CF_OPT_ITER_CAP at max_iter.
 *   cf_opt_compact: one workgroup: the still-running problems of d_active in order into d_next, their number into *d_count.
 * cf_opt_starts: u for n rows: a free coordinate uniform in [delta, 1 - delta] from stream c (the coordinate) at counter b
 *   (the row) of the ensemble's counter-based generator under `key` (optimize.py: opt_key) when `random`, else
 *   clamp((x0 - lo) / width); a fixed coordinate always from d_x0 [n * ndim]; d_theta = lo + u width.
 * Per-problem state (cf_opt_state): row-major float64 device arrays, problem b at b * ndim (u), b * 16 (g, g_prev, s, d,
 * form), b * 256 (hinv, row i of H^-1 at 16 i) and b (f, gnorm, status, n_iter, flags).  Every call is asynchronous on
 * `hip_stream`; sums run in index order and there are no float atomics, so a problem's bits do not depend on the batch. */
#define CF_OPT_MAX_NDIM 16
#define CF_OPT_MAX_TRIALS 8
enum cf_opt_status {
  CF_OPT_RUNNING = 0,
  CF_OPT_CONVERGED = 1,         /* projected, box-scaled gradient <= gtol + gtol_rel |f| */
  CF_OPT_NOISE_FLOOR = 2,       /* no ascent after a reset of H^-1: converged at the finite-difference noise floor */
  CF_OPT_ITER_CAP = 3,
  CF_OPT_NONFINITE_START = 4,   /* f of the start is not finite (set by the driver; the problem never moves) */
  CF_OPT_NONFINITE_STENCIL = 5
};
enum cf_opt_flag { CF_OPT_NEED_RESET = 1, CF_OPT_HAS_PAIR = 2, CF_OPT_FRESH = 4, CF_OPT_HAS_STEP = 8 };
typedef struct cf_opt_params {
  int32_t ndim;                        /* 1 .. CF_OPT_MAX_NDIM */
  int32_t n_free;                      /* 1 .. ndim */
  int32_t free_idx[CF_OPT_MAX_NDIM];   /* ascending theta indices of the free coordinates */
  double lo[CF_OPT_MAX_NDIM];
  double width[CF_OPT_MAX_NDIM];       /* hi - lo > 0 */
  double h;                            /* stencil step in u, (0, 0.01] */
  double delta;                        /* margin of u, (0, 1e-3] */
  double c1;                           /* Armijo constant, (0, 1) */
  double gtol;                         /* convergence: max |projected g| <= gtol + gtol_rel |f| */
  double gtol_rel;
  int32_t n_trials;                    /* K, 1 .. CF_OPT_MAX_TRIALS */
  int32_t max_iter;                    /* >= 1 */
} cf_opt_params;
typedef struct cf_opt_state {
  double* u;       /* [B * ndim] */
  double* f;       /* [B] */
  double* g;       /* [B * 16] gradient at u (free slots) */
  double* g_prev;  /* [B * 16] gradient before the last accepted step */
  double* s;       /* [B * 16] last accepted step in u */
  double* hinv;    /* [B * 256] */
  double* d;       /* [B * 16] direction */
  double* gnorm;   /* [B] max |projected g| */
  int8_t* form;    /* [B * 16] stencil forms */
  int32_t* status; /* [B] cf_opt_status */
  int32_t* n_iter; /* [B] */
  int32_t* flags;  /* [B] cf_opt_flag bits */
} cf_opt_state;

int cf_opt_starts(const cf_opt_params* params, int64_t n, const double* d_x0, uint64_t key, int32_t random, double* d_u,
                  double* d_theta, void* hip_stream);
int cf_opt_stencil(const cf_opt_params* params, const cf_opt_state* state, const int32_t* d_active, int64_t n_active,
                   double* d_rows, void* hip_stream);
int cf_opt_direction(const cf_opt_params* params, const cf_opt_state* state, const int32_t* d_active, int64_t n_active,
                     const double* d_fs, double* d_trials, void* hip_stream);
int cf_opt_accept(const cf_opt_params* params, const cf_opt_state* state, const int32_t* d_active, int64_t n_active,
                  const double* d_ft, void* hip_stream);
int cf_opt_compact(const int32_t* d_active, int64_t n_active, const int32_t* d_status, int32_t* d_next, int32_t* d_count,
                   void* hip_stream);

/* ---- derived parameters and prediction curves of posterior samples (csrc/cosmofit_derived.hip; the driver is
 * cosmology-model-fit_amd/derived.py) -----------------------------------------------------------------------------------------
 * What the post-fit blocks of the scripts do first with their samples: add columns.  Rows are d_theta [S * ndim] float64,
 * row-major, in device memory on the handle's device (a flat chain, or the weighted nested posterior); the model, the slot
 * mapping (cf_param, om_mode, rd_mode, rd_wm_mode), the fit coefficients, the Gauss-Legendre nodes and the neutrino constants
 * are the handle's.  One thread per row for the scalar quantities, one workgroup (and one distance table in LDS) per row for
 * the curves; every sum runs in a fixed order, so a row's values depend neither on S, nor on the row's position, nor on the
 * launch geometry.  A non-finite theta entry gives NaN in the columns that read it and touches no other row; there is no box
 * check.  A quantity whose slot or block the handle lacks is CF_ERR_INVALID with the quantity's name in the message.
 *
 * Scalar quantities (cf_derived_code, one `arg` each, 0 unless stated).  With h = H0 / 100, wb / wc = slots CF_P_OBH2 /
 * CF_P_OCH2, wnu = cf_desc.omnu_h2:
 *   CF_DQ_H0, CF_DQ_H          slot CF_P_H0, and H0 / 100
 *   CF_DQ_OM                   CF_EZ_PHYSICAL: (wb + wc + wnu) / h^2                       bao/desi_cmb.py:196-197
 *                              CF_EZ_LATE_FLAT: slot CF_P_OM, or slot / h^2 with om_mode = 1  bao/desi_omh2.py:18-20
 *   CF_DQ_OMH2                 wb + wc + wnu, or Omega_m h^2                               bao/desi_cmb.py:196, bao/desi_union3_bbn.py:175
 *   CF_DQ_OBH2, CF_DQ_OCH2     the slots
 *   CF_DQ_W0, CF_DQ_WA         the slots; CF_FDE_THAWING: wa = -1.5 (1 - w0^2)             bao/desi_union3_bbn.py:320
 *   CF_DQ_Q0                   Om / 2 + (1 + 3 w0) (1 - Om) / 2                            bao/desi_cmb_union3_fs8.py:238-240
 *   CF_DQ_J0                   1 + 1.5 (1 - Om) (3 w0 (1 + w0) + wa)                       bao/desi_cmb_union3_fs8.py:243-245
 *   CF_DQ_S8                   sigma_8 (Om / 0.3)^0.5, sigma_8 = slot CF_P_S8              bao/desi_cmb_union3_fs8.py:284
 *   CF_DQ_RD                   what the BAO block divides by: slot CF_P_RD, or the r_drag fit (CF_RD_FIT)  bao/desi_cmb.py:81-82
 *   CF_DQ_Z_STAR               z_star(wb, wb + wc + wnu), cf_desc.zstar_fit                cmb/data_planck_act_compression.py:86-99
 *   CF_DQ_R_DRAG               r_drag(wb, wm): cf_desc.rd_fit (CF_RD_FIT) or cf_derived_consts.rdrag_fit   cmb/...:102-124
 *   CF_DQ_Z_DRAG               z_drag(wb, wm), cf_derived_consts.zdrag_fit                 cmb/data_planck_act_compression.py:127-138
 *                              (wm of both: wb + wc + wnu, or Omega_m h^2 with rd_wm_mode = 1, bao/desi_bbn.py:46-60)
 *   CF_DQ_Z_EQ                 -1 + (wb + wc) / arg, arg = Omega_r h^2 (0: cf_derived_consts.zeq_or_h2)   cmb/cmb.py:134-137
 *   CF_DQ_H_AT                 H(arg) in km/s/Mpc, arg = z                                 ohd/cc.py:95-96
 * Gauss-Legendre quantities (the handle has a compressed-CMB block, hence nodes): the integrands, the node order and the z*
 * of cmb_distances, cmb/data_planck_act_compression.py:160-212
 *   CF_DQ_RS_STAR              r_s(z*) in Mpc                                              :183-197
 *   CF_DQ_DM_STAR              D_M(z*) in Mpc                                              :160-172
 *   CF_DQ_THETA_STAR100        100 r_s(z*) / D_M(z*)                                       cmb/cmb.py:56,63
 *   CF_DQ_R                    100 sqrt(wb + wc + wnu) D_M(z*) / c                         :210
 *   CF_DQ_LA                   pi D_M(z*) / r_s(z*)                                        :211
 *
 * Curves (cf_curve_code) at d_z [nz]: distances from the row's own n_grid-node trapezoid table and cubic Hermite with linear
 * extrapolation beyond the grid (DM_z of the scripts, bao/desi_cmb.py:59-65), D_H by cf_desc.bao_dh_mode, r_d as CF_DQ_RD:
 *   CF_CURVE_H  H(z)   CF_CURVE_DM  D_M(z)   CF_CURVE_DV_RD / _DM_RD / _DH_RD / _FAP  bao_theory(z, qty, params) (bao/desi.py:38-56)
 *   CF_CURVE_MU  25 + 5 log10((1 + z) D_M(z))  (sn/pantheon.py:52-54)
 * A non-finite z gives NaN.
 *
 * cf_derived_device / cf_curves_device: d_out [S * n_q] / [S * nz] float64, row-major; asynchronous on `hip_stream`, ordered
 * like any other work on that stream (they use no workspace of the handle, so they are never the stream switch of
 * cf_eval_device's contract and may be captured); a single-device handle; S = 0 is a no-op; 1 <= n_q <= CF_DQ_MAX,
 * 1 <= nz <= CF_CURVE_MAX_NZ.  `consts` may be NULL when no requested quantity reads it.  cf_derived / cf_curves: the same on
 * host buffers, synchronous. */
#define CF_DQ_MAX 32
#define CF_CURVE_MAX_NZ 4096
enum cf_derived_code {
  CF_DQ_H0 = 0, CF_DQ_H = 1, CF_DQ_OM = 2, CF_DQ_OMH2 = 3, CF_DQ_OBH2 = 4, CF_DQ_OCH2 = 5, CF_DQ_W0 = 6, CF_DQ_WA = 7,
  CF_DQ_Q0 = 8, CF_DQ_J0 = 9, CF_DQ_S8 = 10, CF_DQ_RD = 11, CF_DQ_Z_STAR = 12, CF_DQ_R_DRAG = 13, CF_DQ_Z_DRAG = 14,
  CF_DQ_Z_EQ = 15, CF_DQ_H_AT = 16,
  CF_DQ_RS_STAR = 32, CF_DQ_DM_STAR = 33, CF_DQ_THETA_STAR100 = 34, CF_DQ_R = 35, CF_DQ_LA = 36
};
enum cf_curve_code {
  CF_CURVE_H = 0, CF_CURVE_DM = 1, CF_CURVE_DV_RD = 2, CF_CURVE_DM_RD = 3, CF_CURVE_DH_RD = 4, CF_CURVE_FAP = 5, CF_CURVE_MU = 6
};
typedef struct cf_derived_consts {
  int32_t struct_size;   /* sizeof(cf_derived_consts) as seen by the caller */
  int32_t has_rdrag_fit; /* 1: rdrag_fit is set (only read by CF_DQ_R_DRAG on a handle without CF_RD_FIT) */
  double zdrag_fit[10];  /* s1, s2, b, m, then c1, e1, e2, c2, e3, e4 of (1 + s1 c1 wb^e1 wm^e2 + s2 c2 wm^e3) wm^e4
                            (wb, wm raised to b, m first)          cmb/data_planck_act_compression.py:127-138 */
  double rdrag_fit[11];  /* b, m, a1..a9 as cf_desc.rd_fit */
  double zeq_or_h2;      /* Omega_r h^2 of z_eq: cmb.Omega_r_h2(), N_eff = 3.044     cmb/cmb.py:135 */
} cf_derived_consts;

int cf_derived_device(cf_handle* h, const double* d_theta, int64_t S, const int32_t* codes, const double* args, int32_t n_q,
                      const cf_derived_consts* consts, double* d_out, void* hip_stream);
int cf_curves_device(cf_handle* h, const double* d_theta, int64_t S, int32_t code, const double* d_z, int32_t nz, double* d_out,
                     void* hip_stream);
int cf_derived(cf_handle* h, const double* theta, int64_t S, const int32_t* codes, const double* args, int32_t n_q,
               const cf_derived_consts* consts, double* out);
int cf_curves(cf_handle* h, const double* theta, int64_t S, int32_t code, const double* z, int32_t nz, double* out);

/* ---- Gaussian-process reconstruction of H(z) (csrc/cosmofit_gp.hip; the driver is cosmology-model-fit_amd/gp.py) -------------
 * The model of ohd/cc_gp.py:14-41 with ohd/gp_lib.py:55-68: data z [n], y [n], a symmetric covariance C [n, n]; hyperparameters
 * theta = (m, s_f^2, l, s) = constant mean, output scale, length scale, noise scale, in natural form (a box replaces gpytorch's
 * constraints):
 *   K_ij = s_f^2 exp(-(z_i - z_j)^2 / (2 l^2)) + s C_ij,   r = y - m,   K = L L^T
 *   log ML = -1/2 r^T K^-1 r - sum_i log L_ii - (n / 2) log 2 pi        (the whole marginal likelihood, not a per-datum loss)
 * and at a test redshift z*, with k* = k(z, z*), dk* = d k(z, z*) / d z*, v = L^-1 k*, u = L^-1 dk*, w = L^-1 r:
 *   [0] mean = m + v . w            [1] var = s_f^2 - v . v + s noise           (`noise`: test_noise of cc_gp.py:76-79)
 *   [2] dmean = u . w               [3] dvar = s_f^2 / l^2 - u . u               [4] cov(value, derivative) = -v . u
 * All arithmetic is float64 and the kernels work on whatever (y, C) they are given (gp.py normalises as the script does).
 *
 * cf_gp_create validates before its first HIP call (1 <= n <= CF_GP_MAX_N, non-null pointers, finite data, C symmetric to 1e-12
 * relative, bounds [4][2] finite with lo < hi and lo >= 0 for s_f^2, l, s) and copies everything to the device.
 *
 * cf_gp_mll_device: d_theta [W * 4] -> d_out [W], and d_parts [W * 2] = (r^T K^-1 r, log|K|) when not NULL.  Asynchronous on
 * `hip_stream`, one wave per row, K built and factored in LDS.  A row with an entry not strictly inside the box (NaN and +-inf
 * included) is -inf without being evaluated (its parts are NaN); a pivot <= 0 or non-finite is -inf, NaN parts, and one count
 * in cf_gp_info.failed_factorizations; the value is never NaN.
 *
 * cf_gp_predict_device: d_theta [S * 4], d_zstar [nz] -> d_out [S * nz * 5], the five quantities above.  One workgroup per row:
 * factor once, then every test point.  A row outside the box or with a failed factorisation is NaN in that row only; a
 * non-finite z* is NaN at that point only.  1 <= nz <= CF_GP_MAX_NZ, noise finite and >= 0.
 *
 * Every sum runs in index order: a row's bits depend neither on W / S, nor on the row's position, nor on the launch geometry.
 * Zero rows is a no-op; up to 2^31 - 1 rows per call, launched as grids of at most 2^22 rows one after the other on the stream.
 * cf_gp_mll / cf_gp_predict: the same on host buffers, synchronous. */
#define CF_GP_NDIM 4
#define CF_GP_MAX_N 64
#define CF_GP_MAX_NZ 65536
typedef struct cf_gp cf_gp;
typedef struct cf_gp_desc {
  int32_t struct_size; /* sizeof(cf_gp_desc) as seen by the caller */
  int32_t device;
  int32_t n;
  int32_t _pad;
  const double* z;      /* [n] */
  const double* y;      /* [n] */
  const double* cov;    /* [n * n] row-major */
  const double* bounds; /* [4 * 2]: (lo, hi) of m, s_f^2, l, s */
} cf_gp_desc;
typedef struct cf_gp_info {
  int32_t n, device;
  int32_t ld;        /* leading dimension of K in LDS (doubles) */
  int32_t lds_bytes; /* dynamic LDS of one row */
  int64_t failed_factorizations; /* rows of cf_gp_mll_device / cf_gp_mll whose factorisation met a pivot <= 0 or non-finite */
} cf_gp_info;

int cf_gp_create(const cf_gp_desc* desc, cf_gp** out);
void cf_gp_destroy(cf_gp* gp);
int cf_gp_get_info(cf_gp* gp, cf_gp_info* info); /* waits for the device */
int cf_gp_mll_device(cf_gp* gp, const double* d_theta, int64_t W, double* d_out, double* d_parts, void* hip_stream);
int cf_gp_predict_device(cf_gp* gp, const double* d_theta, int64_t S, const double* d_zstar, int32_t nz, double noise,
                         double* d_out, void* hip_stream);
int cf_gp_mll(cf_gp* gp, const double* theta, int64_t W, double* out, double* parts);
int cf_gp_predict(cf_gp* gp, const double* theta, int64_t S, const double* zstar, int32_t nz, double noise, double* out);

/* ---- Quintessence reconstruction (csrc/cosmofit_field.hip; the driver is cosmology-model-fit_amd/quintessence.py) ------------
 * field.py for every row of a chain.  On a = linspace(a_min, a_max, n_a), with h = H0 / 100, Or = orh2 / h^2 and
 *   E^2(a) = Om a^-3 + Or a^-4 + (1 - Om - Or) rho_de(a)                                        field.py:23-26
 *   CF_FDE_THAWING  1 + w = 2 (1 + w0) a^3 / D,  rho_de = 4 / D^2,  D = (1 + w0) a^3 + 1 - w0     :19-21
 *   CF_FDE_WCDM     1 + w = 1 + w0,               rho_de = a^(-3 (1 + w0))
 *   CF_FDE_CPL      1 + w = 1 + w0 + wa (1 - a),  rho_de = a^(-3 (1 + w0 + wa)) exp(-3 wa (1 - a))
 * (CF_FDE_LCDM has no field and is refused) the row's tables are the cumulative trapezoids (scipy's, initial = 0)
 *   phi(a) of sqrt((1 + w) rho_de) / (a H0 E)   :40-42      t(a) of 1 / (a E), times 9.77813 / h Gyr   :97-104
 * 1 + w is formed directly, not as 1 + (-1 + x) as the script has it: below a ~ 0.01 the device values are the more accurate
 * ones (the script's phi differs by up to 1.6e-6 relative at its first nodes, 4e-15 of the row's largest phi).
 *
 * Queries, each set optional, every output pointer optional (NULL: that part is skipped), outputs row-major [S, n]:
 *   a_q [n_aq]     phi_a, t_a: np.interp on the a grid (clamped outside); w_a, K_a = (1 + w) rho_de / 2, V_a = (1 - w) rho_de / 2
 *                  analytic at a_q                                                                :31-32,68,105
 *   phi_q [n_phi]  a_phi = interp1d(phi, a, linear, extrapolate)(phi_q), V_phi = V(a_phi)            :44-48
 *                  phi_q = NULL with n_phi >= 1: every row's own linspace(phi[0], phi[n_a - 1], n_phi), written to phi_grid
 *   t_q [n_t]      a_t = interp1d(t, a, linear, extrapolate)(t_q), phi_t = np.interp(t_q, t, phi), t in Gyr   :108-114
 *                  t_q = NULL with n_t >= 1: every row's own linspace(t[min(10, n_a - 1)], min(1.5 t_today, 0.95 t[n_a - 1]),
 *                  n_t), written to t_grid
 *   scalars [S, CF_FIELD_NSCALAR] (cf_field_scalar), status [S] (cf_field_status)
 * A NaN query gives NaN at that point only.  Status of a row: CF_FIELD_OK; CF_FIELD_PHANTOM when 1 + w < 0 at a node (phi_a,
 * phi_grid, a_phi, V_phi, phi_t, phi_today and phi_max are NaN, the rest is computed); CF_FIELD_BAD for a non-finite parameter,
 * H0 <= 0, or E^2 <= 0 / non-finite at a node (everything is NaN).  A bad row never touches its neighbours.
 *
 * The parameters H0, Om, w0 and (CF_FDE_CPL only, n_par = 4, otherwise n_par = 3) wa come from theta[idx] * scale or are fixed.
 * Validated before the first HIP call (CF_ERR_INVALID): struct_size, fde, 16 <= n_a <= 8192, finite 0 < a_min < 1 < a_max,
 * orh2 finite >= 0, 1 <= ndim <= CF_FIELD_MAX_NDIM, columns < ndim, n_par, 0 <= S <= CF_FIELD_MAX_ROWS, at most
 * CF_FIELD_MAX_NQ points per set, an output whose query set is empty.  S = 0 is a no-op.
 *
 * cf_field_device: one 512-thread workgroup per row (grids of at most CF_FIELD_LAUNCH_ROWS rows), the row's {phi, t} table in LDS (16 n_a + 8 KB); asynchronous on
 * `hip_stream` on the current device, ordered like any other work on that stream, no workspace, may be captured.  Every sum
 * runs in an order fixed by n_a alone: a row's bits depend neither on S, nor on its position, nor on the grid of the launch.
 * cf_field: the same on host buffers, synchronous, on the current device. */
#define CF_FIELD_MAX_NQ 4096
#define CF_FIELD_MAX_NDIM 64
#define CF_FIELD_MAX_ROWS 2147483647
#define CF_FIELD_LAUNCH_ROWS 4194304 /* rows (workgroups) per grid: 2^31 threads at 512 per workgroup */
#define CF_FIELD_NPAR 4
#define CF_FIELD_NSCALAR 5
enum cf_field_par { CF_FIELD_P_H0 = 0, CF_FIELD_P_OM = 1, CF_FIELD_P_W0 = 2, CF_FIELD_P_WA = 3 };
enum cf_field_scalar {
  CF_FIELD_PHI_TODAY = 0, CF_FIELD_T_TODAY = 1 /* Gyr */, CF_FIELD_HUBBLE_TIME = 2 /* Gyr */, CF_FIELD_PHI_MAX = 3,
  CF_FIELD_T_MAX = 4 /* Gyr */
};
enum cf_field_status { CF_FIELD_OK = 0, CF_FIELD_PHANTOM = 1, CF_FIELD_BAD = 2 };
typedef struct cf_field_desc {
  int32_t struct_size; /* sizeof(cf_field_desc) as seen by the caller */
  int32_t fde;         /* CF_FDE_WCDM | CF_FDE_THAWING | CF_FDE_CPL */
  int32_t n_a;
  int32_t ndim;        /* doubles per row of theta */
  int32_t n_par;       /* 3: H0, Om, w0; 4: and wa (CF_FDE_CPL) */
  int32_t _pad;
  double a_min, a_max;
  double orh2;         /* Omega_r h^2 (field.py:10: 4.1835e-05) */
  cf_param par[CF_FIELD_NPAR];
} cf_field_desc;
typedef struct cf_field_queries {
  const double* a_q;
  const double* phi_q; /* NULL with n_phi >= 1: the rows' own grids */
  const double* t_q;   /* NULL with n_t >= 1: the rows' own grids */
  int32_t n_aq, n_phi, n_t, _pad;
} cf_field_queries;
typedef struct cf_field_out {
  double *phi_a, *t_a, *w_a, *K_a, *V_a; /* [S, n_aq] */
  double *phi_grid, *a_phi, *V_phi;      /* [S, n_phi] */
  double *t_grid, *a_t, *phi_t;          /* [S, n_t] */
  double* scalars;                       /* [S, CF_FIELD_NSCALAR] */
  int32_t* status;                       /* [S] */
} cf_field_out;

/* How cf_field_device cuts S rows into grids: cf_field_launch_count(S) launches one after the other on the stream, launch k over
 * the rows [begin, end) of cf_field_launch_range (at most CF_FIELD_LAUNCH_ROWS each; k out of range: the empty range [S, S)).
 * Host arithmetic, no device needed. */
int64_t cf_field_launch_count(int64_t S);
void cf_field_launch_range(int64_t S, int64_t k, int64_t* begin, int64_t* end);
int cf_field_device(const cf_field_desc* desc, const double* d_theta, int64_t S, const cf_field_queries* queries,
                    const cf_field_out* out, void* hip_stream);
int cf_field(const cf_field_desc* desc, const double* theta, int64_t S, const cf_field_queries* queries, const cf_field_out* out);

/* ---- Fit report: residual statistics of every chain sample (csrc/cosmofit_resid.hip; the driver is
 * cosmology-model-fit_amd/fit_report.py) ---------------------------------------------------------------------------------------
 * The block every main() of the scripts ends with (sn/pantheon.py:150-201, bao/desi_fs_lya.py:96-141, sn/plotting.py:46-71),
 * for every row of d_theta [S * ndim] instead of the one central theta.  The residual rows are those of the accessor path
 * (cf_eval_parts: the reference's exact sequence, every SN variant), evaluated in chunks of at most CF_RESID_CHUNK rows into
 * the handle's workspace and reduced there by two kernels; the likelihood is evaluated once per row.
 *
 * block = CF_RB_SN:  r_i = the row's residual vector, y_i = obs_i - mu_corr_i (`corrected_mags`), n = n_sn,
 *                    sigma_i = sqrt(C_ii), C_ii = sum_{j <= i} L_ij^2 of the Cholesky factor given to cf_create
 * block = CF_RB_BAO: r_i = val_i - bao_theory_i, y_i = val_i, n = n_bao, sigma_i = sqrt of the diagonal of inverse(bao_inv_cov)
 * (sigma is computed on the host at cf_create and uploaded at the first call; cf_resid_sigma copies it out).
 *
 * d_sample [S * CF_RS_NCOL] (cf_resid_col), with m_k = (1 / n) sum_i (r_i - mean)^k:
 *   mean, std = sqrt(m_2) (scipy.stats.norm.fit), ss_res = sum r^2, rmsd = sqrt(ss_res / n), ss_tot = sum (y - mean(y))^2,
 *   r2 = 1 - ss_res / ss_tot, skew = m_3 / m_2^1.5, kurtosis = m_4 / m_2^2 - 3 (scipy.stats.skew / kurtosis: biased, Fisher),
 *   max_pull = max_i |r_i| / sigma_i and its index i (np.argmax's rule: the first NaN, else the first maximum).
 *   Two passes, every sum as lane-strided partials and a fixed butterfly: a row's bits depend neither on S, nor on its position,
 *   nor on the chunking, nor on device / host pointers.  Plain IEEE: n = 1 or m_2 = 0 give NaN where numpy does; a non-finite
 *   theta entry gives NaN in that row only.
 * d_chi2_blocks [S * 10]: the chi2_blocks columns of cf_eval_parts.
 * acc: running per-datum state over the rows, device arrays the caller owns and zeroes before the first call.  For datum i,
 *   rows in order, a row is SKIPPED (n_skipped[i] += 1) when its weight is <= 0 or not finite or r_i is not finite; otherwise
 *   (n_used[i] += 1), with w = d_w[s] (1 when d_w is NULL), West's update
 *     W' = w_sum + w;  d = r_i - mean;  mean += (w d) / W';  m2 += (w d) (r_i - mean);  w_sum = W';
 *     exceed[k * n + i] += w  if |r_i| > thresholds[k] * sigma_i
 *   (Welford's for unit weights; variance = m2 / w_sum).  The accumulation is sequential in global row order: the same bits
 *   for every chunk size and for every split of a chain into consecutive calls.
 * d_w: NULL or [S].  thresholds: host array [n_thr], finite and >= 0, 0 <= n_thr <= CF_RESID_MAX_THR; only read with acc.
 * Any of d_sample, d_chi2_blocks, acc may be NULL, not all three.
 *
 * Checks, all before the first HIP call (cf_resid_check_args states them without a handle): a quasar handle or a handle over
 * several devices is CF_ERR_UNSUPPORTED; a block the handle lacks, S < 0 or > 2^31 - 1, n_thr out of range, a non-finite
 * threshold, an acc whose struct_size / n / n_thr do not match or with a null array, no output at all, and (S > 0) a null
 * d_theta are CF_ERR_INVALID.  S = 0 is a no-op.  The cosmic-chronometer and growth-rate blocks are not covered: the accessor
 * path does not export their theory vectors.
 *
 * Stream contract: cf_resid_device evaluates into the handle's ONE workspace, so it obeys the contract of cf_eval_device
 * (ordered with the handle's other evaluations, the first call after a stream switch blocks the host), NOT the independent,
 * capturable one of cf_derived_device; the first call, and a call that has to grow the workspace, synchronise.
 * cf_resid: the same on host buffers (acc's arrays host arrays too), synchronous, same bits. */
#define CF_RB_SN 0
#define CF_RB_BAO 1
#define CF_RS_NCOL 10
#define CF_RESID_MAX_THR 4
#define CF_RESID_CHUNK 4096
enum cf_resid_col {
  CF_RS_MEAN = 0, CF_RS_STD = 1, CF_RS_SS_RES = 2, CF_RS_RMSD = 3, CF_RS_SS_TOT = 4, CF_RS_R2 = 5, CF_RS_SKEW = 6, CF_RS_KURT = 7,
  CF_RS_MAX_PULL = 8, CF_RS_MAX_PULL_IDX = 9
};
typedef struct cf_resid_acc {
  int32_t struct_size; /* sizeof(cf_resid_acc) as seen by the caller */
  int32_t n;           /* data of the block */
  int32_t n_thr;       /* rows of exceed */
  int32_t _pad;
  double* w_sum;       /* [n] weight of the used rows */
  double* mean;        /* [n] */
  double* m2;          /* [n] sum of w (r - mean)^2 */
  double* exceed;      /* [n_thr * n] weight beyond each threshold (may be NULL when n_thr = 0) */
  int64_t* n_used;     /* [n] */
  int64_t* n_skipped;  /* [n] */
} cf_resid_acc;

int cf_resid_device(cf_handle* h, const double* d_theta, int64_t S, const double* d_w, int32_t block, const double* thresholds,
                    int32_t n_thr, double* d_sample, double* d_chi2_blocks, cf_resid_acc* acc, void* hip_stream);
int cf_resid(cf_handle* h, const double* theta, int64_t S, const double* w, int32_t block, const double* thresholds, int32_t n_thr,
             double* sample, double* chi2_blocks, cf_resid_acc* acc);
/* The argument rules above as host arithmetic on the facts of a handle (its n_sn, n_bao, whether it is a quasar handle, its
 * number of devices): what cf_resid_device returns before it touches the device.  No handle and no device needed. */
int cf_resid_check_args(int64_t n_sn, int32_t n_bao, int32_t is_quasar, int32_t n_devices, const void* theta, int64_t S, int32_t block,
                        const double* thresholds, int32_t n_thr, const void* sample, const void* chi2_blocks, const cf_resid_acc* acc);
/* sigma_i of a block into the host array out [n]; CF_ERR_INVALID for a block the handle lacks.  No HIP call. */
int cf_resid_sigma(cf_handle* h, int32_t block, double* out);
/* Rows per chunk of the following cf_resid_device / cf_resid calls of this handle, 1 .. 65536; 0 restores CF_RESID_CHUNK.
 * The results do not depend on it: it exists so that tests can cross chunk boundaries with few rows. */
int cf_resid_set_chunk(cf_handle* h, int64_t rows);

/* ---- Mock-data ensembles: one likelihood whose DATA differ per row (csrc/cosmofit_mock.hip; the driver is
 * cosmology-model-fit_amd/mocks.py) --------------------------------------------------------------------------------------------
 * The reference reads every Delta chi^2 through Wilks' theorem (sn/pantheon_dipole.py:172, sn/union3_1.py:145-161); calibrating
 * that by simulation needs thousands of data sets fitted under one handle.  All data enter the residual linearly (SN obs - ...,
 * BAO val - theory, CMB prior - distances), so for the data `data + d_k` of mock k
 *     chi2_k(theta) = (r + d_k)^T C^-1 (r + d_k) = chi2(theta) + 2 r(theta) . g_k + c_k,   g_k = C^-1 d_k,  c_k = d_k . g_k
 * and a mock costs one dot product of the residual row the accessor path already forms with a row of g.
 *
 * Value of row s, k = d_mock[s]:  x_b = sum_i r_{b,i}(theta_s) g_b[k n_b + i] for every shifted block b (SN, BAO, CMB, in that
 * order; r_cmb = cmb_prior - the CMB theory vector), shift = 2 sum_b x_b + c[k];
 *   g_b and c must be formed with the matrix of the block's quadratic form AS THE HANDLE EVALUATES IT, symmetrised: a handle
 *   with cmb_mode 2 uses the l_A entry cmb_inv_cov[1][1] alone, so its g_cmb has zeros in columns 0 and 2 and c counts d[1] only;
 *   d_out[s] = base + shift (CF_OUT_CHI2) or base - shift / 2 (CF_OUT_LOGL, CF_OUT_LOGP), base = what cf_eval_device defines
 *   for out_kind on this handle (priors, walls, unshifted blocks included), evaluated through the accessor path;
 *   d_cross[3 s + b] = x_b (0 for a block not shifted; d_cross may be NULL).
 *   k < 0: the observed data, d_out = base (x_b = 0).  k >= n_mocks: NaN in that row, nothing is read out of bounds.  A row
 *   whose base is -inf stays -inf.  A non-finite theta entry gives what cf_eval_device gives for it, in that row only.
 * One wave per row; every sum as lane-strided partials and a fixed butterfly: a row's bits depend on (theta, k) only -- not on
 * S, the row's position, the chunking (cf_mock_set_chunk) or device / host pointers.
 *
 * Checks, all before the first HIP call (cf_mock_check_args states them without a handle): a quasar handle or a handle over
 * several devices is CF_ERR_UNSUPPORTED; a null set, a struct_size mismatch, n_mocks < 1, an n_* that is neither 0 nor the
 * handle's (n_cmb: 3 with a CMB block), a null array of a shifted block or a null c, no shifted block at all, a bad out_kind,
 * S < 0 or > 2^31 - 1, and (S > 0) a null theta, mock or out are CF_ERR_INVALID.  S = 0 is a no-op.
 * Stream contract: that of cf_resid_device (the handle's ONE workspace).
 * cf_mock_eval: the same on host buffers (the set's arrays host arrays too), synchronous, same bits. */
typedef struct cf_mock_set {          /* arrays are the caller's, device memory (host memory for cf_mock_eval) */
  int32_t struct_size, n_mocks;       /* n_mocks >= 1 */
  int32_t n_sn, n_bao, n_cmb;         /* 0: block not shifted; else the handle's n_sn / n_bao / 3 */
  int32_t _pad;
  const double* g_sn;                 /* [n_mocks * n_sn]  C_sn^-1 d_k */
  const double* g_bao;                /* [n_mocks * n_bao] bao_inv_cov d_k */
  const double* g_cmb;                /* [n_mocks * 3]     cmb_inv_cov d_k; cmb_mode 2 (l_A alone): (0, cmb_inv_cov[1][1] d_k[1], 0) */
  const double* c;                    /* [n_mocks] sum over the shifted blocks of d_k . g_k */
} cf_mock_set;
#define CF_MOCK_CHUNK 4096
int cf_mock_eval_device(cf_handle* h, const cf_mock_set* set, const double* d_theta, int64_t S, const int32_t* d_mock,
                        int32_t out_kind, double* d_out, double* d_cross, void* hip_stream);
int cf_mock_eval(cf_handle* h, const cf_mock_set* set, const double* theta, int64_t S, const int32_t* mock, int32_t out_kind,
                 double* out, double* cross);
/* The argument rules above as host arithmetic on the facts of a handle (its n_sn, n_bao, whether it has a CMB block, whether it
 * is a quasar handle, its number of devices).  No handle and no device needed. */
int cf_mock_check_args(int64_t n_sn, int32_t n_bao, int32_t has_cmb, int32_t is_quasar, int32_t n_devices, const cf_mock_set* set,
                       const void* theta, int64_t S, const void* mock, int32_t out_kind, const void* out);
/* Rows per chunk of the following cf_mock_eval_device / cf_mock_eval calls of this handle, 1 .. 65536; 0 restores
 * CF_MOCK_CHUNK.  The results do not depend on it. */
int cf_mock_set_chunk(cf_handle* h, int64_t rows);
/* Standard normals of a mock set on the device: d_out[(k - k0) n + i] = the ensemble generator's normal (Box-Muller from streams
 * 0 and 1 of `key`, counter k n + i) for k0 <= k < k0 + K, i < n.  A value depends on (key, k, i) only, so a set can be drawn
 * in pieces.  CF_ERR_INVALID: k0 < 0, K < 0, n < 1, (k0 + K) n > 2^62, a null d_out with K > 0.  K = 0 is a no-op. */
int cf_mock_normals(uint64_t key, int64_t k0, int64_t K, int32_t n, double* d_out, void* hip_stream);

/* ---- Which data carry a chi^2: per-datum attribution and leave-one-out residuals (csrc/cosmofit_infl.hip; the driver is
 * cosmology-model-fit_amd/influence.py) ----------------------------------------------------------------------------------------
 * The reference reads a Delta chi^2 between two models as a statement about individual data (README: the supernovae on either side
 * of z_turn).  With a dense covariance the raw pull r_i / sqrt(C_ii) of the fit report is no test statistic; what is one comes
 * from a single vector per row, g = K r with K = C^-1 the precision matrix of the block:
 *   contrib_i = r_i g_i            sum_i contrib_i = chi^2, so contrib_i(theta_A) - contrib_i(theta_B) splits a Delta chi^2 exactly
 *   loo_i     = g_i / K_ii         datum i minus its prediction from all the others; its error is 1 / sqrt(K_ii)
 *   z_i       = g_i / sqrt(K_ii)   the z-score of that leave-one-out residual
 *   chi^2 without datum i = chi^2 - g_i^2 / K_ii (no refit of the covariance).
 *
 * cf_prec: K on one device.  cf_prec_create reads the LOWER triangle of the Cholesky factor L [n x n, row pitch ld] and forms
 * K = Linv^T Linv on the host in extended precision from the extended-precision columns of the inverse (forward substitution
 * with compensated sums; Linv is not rounded to double in between; K is rounded once).  cf_prec_create_inv takes the precision matrix itself [n x n, row pitch ld] (the BAO
 * block's inverse covariance) and symmetrises it, (A + A^T) / 2; a datum whose diagonal entry is 0 is one the likelihood ignores
 * (its row and column are zero): g, contrib, z and loo are 0 there.  Both upload K (zero-padded to a multiple of 16), diag K and
 * 1 / sqrt(diag K).  cf_prec_diag copies diag K out [n] (no HIP call).  CF_ERR_INVALID: a null argument, n < 1 or > 32768,
 * ld < n; CF_ERR_NOT_POSDEF: a factor with a diagonal entry that is not finite and > 0, an inverse covariance with a non-finite
 * entry or a negative diagonal entry; CF_ERR_NO_DEVICE without a device.
 *
 * cf_prec_apply_device: the bare product d_g[s * g_pitch + j] = sum_i d_rows[s * pitch + i] K_ij for s < S, j < n on FP64 matrix
 * cores; columns >= n and rows >= S of d_rows are never read, columns >= n of d_g never written.  The k loop is ascending with one
 * accumulator per output, so a row of d_g depends on its row of d_rows and on K only: not on S, the row's position or the stream.
 * A NaN or inf in a row stays in that row.  CF_ERR_INVALID: a null argument (S > 0), S < 0 or > 2^31 - 1, pitch or g_pitch < n.
 *
 * cf_infl_device: for every row of d_theta [S * ndim] the residual row of the accessor path (as cf_resid_device: chunks of at
 * most CF_INFL_CHUNK rows into the handle's workspace), g = K r, and from it
 *   out->g, contrib, z, loo [S * n] (each may be NULL), out->sample [S * CF_INFL_NCOL] (may be NULL; cf_infl_col):
 *     chi2 = sum_i r_i g_i (lane-strided partials and a fixed butterfly), max_z = max_i |z_i| and its index, max_drop =
 *     max_i g_i^2 / K_ii and its index (np.argmax's rule: the first NaN, else the first maximum);
 *   acc_z: the running per-datum state of cf_resid_device (West's update, thresholds in units of sigma = 1) over the z rows;
 *   acc_contrib: the same over the contrib rows, without thresholds (its n_thr must be 0).
 *   A row's bits depend on theta only: not on S, its position, the chunking (cf_infl_set_chunk) or device / host pointers; the
 *   accumulators give the same bits for every split of a chain into consecutive calls.  A non-finite theta entry gives NaN in
 *   that row only, and the accumulators skip it.
 * block: CF_RB_SN (r = the row's residual vector) or CF_RB_BAO (r = val - bao_theory).  d_w: NULL or [S], read by the accumulators.
 *
 * Checks, all before the first HIP call (cf_infl_check_args states them without a handle), all CF_ERR_INVALID: a quasar handle,
 * a handle over several devices, a block the handle lacks, a null cf_prec, prec_n that is not the block's n, a cf_prec on
 * another device than the handle, S < 0 or > 2^31 - 1, n_thr outside 0 .. CF_RESID_MAX_THR, a non-finite or negative threshold,
 * an out whose struct_size does not match, an accumulator whose struct_size / n / n_thr do not match or with a null array,
 * no output at all, and (S > 0) a null d_theta.  S = 0 is a no-op.
 * Stream contract: that of cf_resid_device (the handle's ONE workspace).
 * cf_infl: the same on host buffers (the accumulators' arrays host arrays too), synchronous, same bits. */
#define CF_INFL_NCOL 5
#define CF_INFL_CHUNK 4096
enum cf_infl_col { CF_IS_CHI2 = 0, CF_IS_MAX_Z = 1, CF_IS_MAX_Z_IDX = 2, CF_IS_MAX_DROP = 3, CF_IS_MAX_DROP_IDX = 4 };
typedef struct cf_prec cf_prec;
typedef struct cf_infl_out {
  int32_t struct_size; /* sizeof(cf_infl_out) as seen by the caller */
  int32_t _pad;
  double* g;           /* [S * n] K r */
  double* contrib;     /* [S * n] r_i g_i */
  double* z;           /* [S * n] g_i / sqrt(K_ii) */
  double* loo;         /* [S * n] g_i / K_ii */
  double* sample;      /* [S * CF_INFL_NCOL] */
} cf_infl_out;

int cf_prec_create(const double* L, int64_t n, int64_t ld, int32_t device, cf_prec** out);
int cf_prec_create_inv(const double* inv_cov, int64_t n, int64_t ld, int32_t device, cf_prec** out);
void cf_prec_destroy(cf_prec* p);
int cf_prec_diag(cf_prec* p, double* out_n);
int cf_prec_apply_device(cf_prec* p, const double* d_rows, int64_t pitch, int64_t S, double* d_g, int64_t g_pitch, void* hip_stream);
/* The host half of cf_prec_create alone: K [n * n] and diag K [n] (either may be NULL) of the factor L.  No device needed. */
int cf_selftest_prec_host(const double* L, int64_t n, int64_t ld, double* K_out, double* kdiag_out);
int cf_infl_device(cf_handle* h, cf_prec* prec, const double* d_theta, int64_t S, const double* d_w, int32_t block,
                   const double* thresholds, int32_t n_thr, cf_infl_out* out, cf_resid_acc* acc_z, cf_resid_acc* acc_contrib,
                   void* hip_stream);
int cf_infl(cf_handle* h, cf_prec* prec, const double* theta, int64_t S, const double* w, int32_t block, const double* thresholds,
            int32_t n_thr, cf_infl_out* out, cf_resid_acc* acc_z, cf_resid_acc* acc_contrib);
/* The argument rules above as host arithmetic on the facts of a handle (its n_sn, n_bao, whether it is a quasar handle, its
 * number of devices, its device) and of a cf_prec (has_prec: non-null; its n and device).  No handle and no device needed. */
int cf_infl_check_args(int64_t n_sn, int32_t n_bao, int32_t is_quasar, int32_t n_devices, int32_t handle_device, int32_t has_prec,
                       int64_t prec_n, int32_t prec_device, const void* theta, int64_t S, int32_t block, const double* thresholds,
                       int32_t n_thr, const cf_infl_out* out, const cf_resid_acc* acc_z, const cf_resid_acc* acc_contrib);
/* Rows per chunk of the following cf_infl_device / cf_infl calls of this handle, 1 .. 65536; 0 restores CF_INFL_CHUNK.  The
 * results do not depend on it: it exists so that tests can cross chunk boundaries with few rows. */
int cf_infl_set_chunk(cf_handle* h, int64_t rows);

/* ---- A free amplitude on the SN covariance: C(s) = C0 + s C1 (csrc/cosmofit_cscale.hip; the driver is
 * cosmology-model-fit_amd/covscale.py) -----------------------------------------------------------------------------------------
 * The handle holds ONE Cholesky factor, C0 = L0 L0^T, fixed at cf_create.  One scalar amplitude on a second matrix needs no new
 * factor: with A = L0^-1 C1 L0^-T = Q diag(lambda) Q^T and T = Q^T L0^-1 (both formed once, on the host, by the caller:
 * covscale.decompose), a residual row r gives y = T r and
 *   quad(s)   = r^T C(s)^-1 r      = sum_k y_k^2 / (1 + s lambda_k)
 *   logdet(s) = ln|C(s)| - ln|C0|  = sum_k log1p(s lambda_k)
 * valid while 1 + s lambda_k > 0 for every k.  C1: the identity (intrinsic scatter, s = sigma_int^2), a 0/1 diagonal (the scatter
 * of one survey or redshift range), a systematics matrix, any symmetric matrix (negative eigenvalues only bound s).
 *
 * cf_cscale: T and lambda on one device.  cf_cscale_create reads T [n x n, row pitch ld] and lambda [n] and uploads M = T^T,
 * zero-padded to a multiple of 16, and lambda.  CF_ERR_INVALID: a null argument, n < 1 or > 32768, ld < n, a non-finite entry of
 * T or lambda; CF_ERR_NO_DEVICE without a device.  cf_cscale_look reports n and the device (either pointer may be NULL).
 *
 * cf_cscale_apply_device: the kernels alone, on caller-supplied rows.  For row s < S and j < n_s, with amplitude
 * d_s[s * n_s + j], it writes d_quad[s * n_s + j] and d_logdet[s * n_s + j] (either may be NULL); d_y is [S * n] = T r, or NULL
 * to never store y (the product Y = R M runs on FP64 matrix cores and the first reduction of quad is fused into its epilogue).
 * Columns >= n and rows >= S of d_rows (row pitch `pitch` >= n) are never read: a select, not a product with zero.
 * 1 <= n_s <= CF_CSCALE_MAX_S.  CF_ERR_INVALID: a null cf_cscale, S < 0 or > 2^31 - 1, n_s out of range, pitch < n, no output at
 * all, and (S > 0) null rows or amplitudes.  S = 0 is a no-op.
 *
 * cf_cscale_eval_device: for every row of d_theta [S * ndim] the residual row of the accessor path (as cf_infl_device: chunks of
 * at most CF_CSCALE_CHUNK rows into the handle's workspace), then the product and the row kernel.  d_out [S * n_s] by out_kind:
 *   CF_OUT_CHI2              the engine's chi^2 of the row with its SN term replaced by quad: (chi2 - chi2_SN(C0)) + quad
 *   CF_OUT_LOGL / CF_OUT_LOGP  the engine's own value of that kind plus 0.5 chi2_SN(C0) - 0.5 (quad + logdet)
 * chi2_SN(C0) is the SN chi^2 the engine computed for that row, so every other block, constant and prior term stays what the
 * engine makes it.  d_parts: NULL, or [S * n_s * 2] holding (quad, logdet).
 *
 * Domain and special values, per (row, j), never leaking to a neighbour: 1 + s lambda_k <= 0 for any k gives NaN in quad and
 * logdet, -inf in d_out for LOGL / LOGP and NaN for CHI2; a non-finite s or a non-finite theta entry gives NaN in that row's
 * outputs only; where the engine's own LOGL / LOGP is -inf (outside the prior box, a non-finite chi^2) d_out is -inf; s = 0
 * gives logdet exactly 0.0 and quad = sum_k y_k^2 in the kernel's order; a zero row gives exact zeros.
 *
 * Determinism: the outputs for (row, s_j) depend on that row's theta (its residual row), on s_j, on T and on lambda only -- not
 * on S or the row's position, not on n_s or the other amplitudes of the row, not on the chunking (cf_cscale_set_chunk), device or
 * host pointers, the stream or repetition.  One accumulator per element of y, an ascending k loop over ceil(n / 32) * 32 columns,
 * quad summed per 32-column slab in a fixed lane order and the slabs in ascending order, logdet as 64 lane-strided partials and
 * a fixed butterfly; no atomics.
 *
 * Checks of the eval entry points, all before the first HIP call (cf_cscale_check_args states them without a handle), all
 * CF_ERR_INVALID: a quasar handle, a handle over several devices, no SN block, a null cf_cscale, a cf_cscale whose n is not n_sn
 * or that lives on another device, S < 0 or > 2^31 - 1, n_s out of range, an out_kind that is none of the three, no output at
 * all, and (S > 0) a null d_theta or d_s.  S = 0 is a no-op.
 * Stream contract: that of cf_resid_device (the handle's ONE workspace); a cf_cscale has ONE scratch for the slab partials, so a
 * call on another stream than the previous call on the same cf_cscale first waits, on the host, for the device.
 * cf_cscale_eval: the same on host buffers, synchronous, same bits. */
#define CF_CSCALE_MAX_S 16
#define CF_CSCALE_CHUNK 4096
typedef struct cf_cscale cf_cscale;
int cf_cscale_create(const double* T, int64_t n, int64_t ld, const double* lambda, int32_t device, cf_cscale** out);
void cf_cscale_destroy(cf_cscale* p);
int cf_cscale_look(const cf_cscale* p, int64_t* n, int32_t* device);
int cf_cscale_apply_device(cf_cscale* p, const double* d_rows, int64_t pitch, int64_t S, const double* d_s, int32_t n_s,
                           double* d_quad, double* d_logdet, double* d_y, void* hip_stream);
int cf_cscale_eval_device(cf_handle* h, cf_cscale* p, const double* d_theta, const double* d_s, int32_t n_s, int64_t S,
                          int32_t out_kind, double* d_out, double* d_parts, void* hip_stream);
int cf_cscale_eval(cf_handle* h, cf_cscale* p, const double* theta, const double* s, int32_t n_s, int64_t S, int32_t out_kind,
                   double* out, double* parts);
/* The argument rules above as host arithmetic on the facts of a handle (its n_sn, whether it is a quasar handle, its number of
 * devices, its device) and of a cf_cscale (has_cscale: non-null; its n and device).  No handle and no device needed. */
int cf_cscale_check_args(int64_t n_sn, int32_t is_quasar, int32_t n_devices, int32_t handle_device, int32_t has_cscale,
                         int64_t cscale_n, int32_t cscale_device, const void* theta, const void* s, int32_t n_s, int64_t S,
                         int32_t out_kind, const void* out, const void* parts);
/* Rows per chunk of the following cf_cscale_eval_device / cf_cscale_eval calls of this handle, 1 .. 65536; 0 restores
 * CF_CSCALE_CHUNK.  The results do not depend on it: it exists so that tests can cross chunk boundaries with few rows. */
int cf_cscale_set_chunk(cf_handle* h, int64_t rows);
/* The arithmetic of the row kernel and of the product's epilogue compiled for the host, in the same order of operations (one
 * __host__ __device__ function per term, shared with the kernels): quad [n_s] and logdet [n_s] (either may be NULL) of one row
 * y [n] for the amplitudes s [n_s], with the domain rule.  No device needed. */
int cf_selftest_cscale_host(const double* y, const double* lambda, int64_t n, const double* s, int32_t n_s, double* quad,
                            double* logdet);

/* ---- Linear SN nuisance parameters in closed form (csrc/cosmofit_marg.hip; the driver is
 * cosmology-model-fit_amd/nuisance.py) -----------------------------------------------------------------------------------------
 * SN residual r(theta, alpha) = r0(theta) - A alpha: r0 is the handle's own residual row (the marginalised slots fixed in its
 * descriptor), A [n, m] constant templates (a column of ones: the absolute magnitude; a 0/1 mask: a per-survey offset;
 * sn_lin_coef: the bulk-flow amplitude), 1 <= m <= CF_MARG_MAX_M, and on alpha_j a prior N(mu_j, sigma_j) or a flat one.  With
 * P = diag(1 / sigma_j^2) (0 where flat), K = C^-1 A, F = A^T K + P = L_F L_F^T, all formed once on the host (nuisance.project):
 *   Wt = K L_F^-T [n, m],  ct = L_F^-1 P mu [m],  U = L_F^T [m, m],  pmu = mu^T P mu
 *   t = Wt^T r0 + ct,   q = sum_j t_j^2 (ascending j),   alpha = U^-1 (t + xi)   (xi = 0: the conditional mean alpha_hat;
 *   xi ~ N(0, I): a draw from p(alpha | theta, data), whose covariance is F^-1)
 *   CF_OUT_CHI2:               chi2_prof = (e + pmu) - q, the minimum over alpha with the prior penalty, in both modes
 *   CF_OUT_LOGL / CF_OUT_LOGP:  (e + 0.5 q) - 0.5 pmu, and + log_norm in mode CF_MARG_MARGINAL (the integral over alpha)
 * where e is the handle's own value of that kind.  e = -inf stays -inf and a NaN e gives NaN; in both cases the row of alpha is
 * NaN, whatever the workspace holds.  A row whose projection t is not finite (a NaN or an inf among its residuals) has NaN in t,
 * q, alpha and the value.
 *
 * cf_marg: Wt (zero-padded to 16 columns), ct and U on one device.  cf_marg_create reads Wt [n * m, row-major], ct [m] and the
 * upper triangle of U [m * m, row-major].  CF_ERR_INVALID: a null argument, n < 1 or > 32768, m outside 1 .. CF_MARG_MAX_M, a
 * non-finite entry, pmu or log_norm, a diagonal entry of U that is not > 0; CF_ERR_NO_DEVICE without a device.  cf_marg_info
 * reports what the object holds (any pointer may be NULL).
 *
 * cf_marg_apply_device: the kernels alone, on caller-supplied rows d_rows [S rows, pitch >= n]: d_t [S * m], d_q [S], d_alpha
 * [S * m] (any may be NULL, not all); d_xi [S * m] or NULL.  Columns >= n and rows >= S are never read: a select, not a product
 * with zero.  CF_ERR_INVALID: a null cf_marg, S < 0 or > 2^31 - 1, pitch < n, no output at all, (S > 0) null rows.
 *
 * cf_marg_eval_device: for every row of d_theta [S * ndim] the residual row of the accessor path (chunks of at most
 * CF_MARG_CHUNK rows into the handle's workspace, as cf_mock_eval_device), then the product T = R Wt on FP64 matrix cores (a wave
 * owns 16 rows and one slice of CF_MARG_SLICE columns; the slice partials are summed in ascending order) and the row kernel.
 * d_out [S] and d_alpha [S * m]: either may be NULL, not both.  d_xi [S * m] or NULL.
 * Determinism: a row's outputs depend on its theta (its residual row), its xi and the cf_marg only -- not on S, the row's
 * position, the chunking (cf_marg_set_chunk), device or host pointers, the stream, repetition or which outputs are asked for.
 * Checks, all before the first HIP call (cf_marg_check_args states them without a handle), all CF_ERR_INVALID: a quasar handle,
 * a handle over several devices, no SN block, a null cf_marg, a cf_marg whose n is not n_sn or that lives on another device, a
 * bad out_kind or mode, S < 0 or > 2^31 - 1, no output at all, (S > 0) a null d_theta.  S = 0 is a no-op.
 * Stream contract: that of cf_resid_device (the handle's ONE workspace); a cf_marg has ONE scratch for the slice partials, so a
 * call on another stream than the previous call on the same cf_marg first waits, on the host, for the device.
 * cf_marg_eval: the same on host buffers, synchronous, same bits. */
#define CF_MARG_MAX_M 16
#define CF_MARG_CHUNK 4096
#define CF_MARG_SLICE 256
#define CF_MARG_PROFILE 0
#define CF_MARG_MARGINAL 1
typedef struct cf_marg cf_marg;
int cf_marg_create(const double* Wt, const double* ct, const double* U, int64_t n, int32_t m, double pmu, double log_norm,
                   int32_t device, cf_marg** out);
void cf_marg_destroy(cf_marg* p);
int cf_marg_info(const cf_marg* p, int64_t* n, int32_t* m, int32_t* device, double* pmu, double* log_norm);
int cf_marg_apply_device(cf_marg* p, const double* d_rows, int64_t pitch, int64_t S, const double* d_xi, double* d_t, double* d_q,
                         double* d_alpha, void* hip_stream);
int cf_marg_eval_device(cf_handle* h, cf_marg* p, const double* d_theta, int64_t S, int32_t out_kind, int32_t mode,
                        const double* d_xi, double* d_out, double* d_alpha, void* hip_stream);
int cf_marg_eval(cf_handle* h, cf_marg* p, const double* theta, int64_t S, int32_t out_kind, int32_t mode, const double* xi,
                 double* out, double* alpha);
/* The argument rules above as host arithmetic on the facts of a handle (its n_sn, whether it is a quasar handle, its number of
 * devices, its device) and of a cf_marg (has_marg: non-null; its n and device).  No handle and no device needed. */
int cf_marg_check_args(int64_t n_sn, int32_t is_quasar, int32_t n_devices, int32_t handle_device, int32_t has_marg, int64_t marg_n,
                       int32_t marg_device, const void* theta, int64_t S, int32_t out_kind, int32_t mode, const void* out,
                       const void* alpha);
/* Rows per chunk of the following cf_marg_eval_device / cf_marg_eval calls of this handle, 1 .. 65536; 0 restores
 * CF_MARG_CHUNK.  The results do not depend on it: it exists so that tests can cross chunk boundaries with few rows. */
int cf_marg_set_chunk(cf_handle* h, int64_t rows);
/* The arithmetic of the row kernel compiled for the host, in the same order of operations (one __host__ __device__ function per
 * step, shared with the kernel): from one row's slice partials part [n_slice * 16] (entry b * 16 + j: slice b, component j),
 * t [m], q, alpha [m] and the value of (out_kind, mode) for the engine value e (any output may be NULL).  No device needed. */
int cf_selftest_marg_host(const double* part, int32_t n_slice, const double* ct, const double* U, int32_t m, const double* xi,
                          double pmu, double log_norm, double e, int32_t out_kind, int32_t mode, double* t, double* q,
                          double* alpha, double* value);

/* ---- Bridge-sampling evidence (csrc/cosmofit_bridge.hip; the driver is cosmology-model-fit_amd/evidence.py) ----------------
 * ln Z of a posterior in a finite box from a chain and draws of a Gaussian fitted to it in unbounded coordinates (Meng & Wong
 * 1996; Gronau et al. 2017).  Everything is float64, row-major, device pointers on the current device, asynchronous on
 * `hip_stream` (cf_bridge_solve excepted, see there); lo, hi [ndim], mean [ndim] and chol [ndim * ndim, row-major, the lower triangle is read] are small HOST arrays
 * copied into the kernel arguments.
 *   u = (theta - lo) / (hi - lo),  phi = log u - log1p(-u),  z = R^-1 (phi - mean) by forward substitution in index order
 *   log J(theta) = sum_k [log(hi_k - lo_k) + log u_k + log1p(-u_k)] in index order
 *   back: u = 1 / (1 + e^-phi), theta = lo + (hi - lo) u, log J = sum_k [log(hi_k - lo_k) - |phi_k| - 2 log1p(e^-|phi_k|)],
 *   finite when u rounds to 0 or 1 (theta may then equal a face; it never leaves [lo, hi]: above the middle of the box it is
 *   formed as hi - (hi - lo) (1 - u)).  Going forward 1 - u is formed as (hi - theta) / (hi - lo),
 *   which keeps phi and log J good to a few ulp next to the upper face.
 * cf_bridge_forward: d_theta [n * ndim] -> d_z [n * ndim], d_log_jac [n].  A row with a coordinate not strictly inside the
 *   box (theta <= lo or theta >= hi), or NaN, gets NaN in its own z row and log J, and nowhere else.
 * cf_bridge_points: d_z [n * ndim] -> d_theta = T^-1(mean + R z) (mirror = 0) or T^-1(mean - R z) (mirror = 1), and its log J.
 * cf_bridge_draw: d_z[row * ndim + k] = the ensemble generator's normal (Box-Muller from streams 2k and 2k + 1 of `key`, counter
 *   first + row): a row's bits depend on (key, first + row, ndim) only, so a set can be drawn in pieces.
 * A row of the three depends on that row and the arguments only: not on n, its position, the stream or repetition.
 * cf_bridge_solve: with x = l - lstar, e = exp(-|x|) (no exponential of a positive number is taken), r_0 = 1,
 *     r_{t+1} = mean_j A(x_2j) / mean_i B(x_1i),   A(x) = 1 / (s1 + s2 r e) for x >= 0, else e / (s1 e + s2 r),
 *                                                  B(x) = e / (s1 + s2 r e) for x >= 0, else 1 / (s1 e + s2 r),
 *   until |r_{t+1} - r_t| <= tol r_{t+1} (CF_BRIDGE_CONVERGED) or max_iter updates (CF_BRIDGE_ITER_CAP); then, at the last r,
 *   f_1j = A(x_2j) and f_2i = r B(x_1i) (= p / (s1 p + s2) and 1 / (s1 p + s2) with p = e^x / r): d_f2 [n1] gets the f_2 series
 *   and d_result [CF_BRIDGE_RESULT_DOUBLES] the record indexed by cf_bridge_result (variances with n - 1; 0 for n = 1).
 *   l_2 = -inf contributes 0.  NaN or +inf in either vector, -inf in l_1, or an r that is not finite and > 0 (every draw
 *   outside the box) give CF_BRIDGE_NONFINITE; in the first case nothing is iterated and the record and d_f2 are NaN.
 *   One launch triple per iteration (slice partials of l2, of l1, a one-thread step) behind a device-side done flag that turns
 *   later launches into no-ops; the call enqueues batches of 16 iterations and reads the flag between them, so it returns after
 *   the last iteration has run (it synchronises `hip_stream`); the record is written by the last launch and read by the caller
 *   once.  No workgroup waits on another.  State and partials live in a stream-ordered workspace of the call.
 *   Order of summation: slices of CF_BRIDGE_SLICE consecutive terms, ascending within a slice, then the slices ascending (the
 *   cf_kde_sum_device contract), so the record's bits depend on the inputs only.  No float atomics.
 * CF_ERR_INVALID, before anything is launched: ndim outside 1 .. CF_BRIDGE_MAX_NDIM, n < 1 (n1, n2), a null pointer, a
 *   non-finite or empty box, a non-finite mean or factor, a non-positive diagonal of chol, mirror not 0 / 1, first < 0, a
 *   non-finite lstar, s1 or s2 not finite and > 0, tol not finite and >= 0, max_iter < 1. */
#define CF_BRIDGE_MAX_NDIM 16
#define CF_BRIDGE_SLICE 2048
#define CF_BRIDGE_RESULT_DOUBLES 8
enum cf_bridge_result { CF_BR_LOG_R = 0, CF_BR_N_ITER = 1, CF_BR_STATUS = 2, CF_BR_MEAN_F1 = 3, CF_BR_VAR_F1 = 4,
                        CF_BR_MEAN_F2 = 5, CF_BR_VAR_F2 = 6, CF_BR_R = 7 };
enum cf_bridge_status { CF_BRIDGE_CONVERGED = 0, CF_BRIDGE_ITER_CAP = 1, CF_BRIDGE_NONFINITE = 2 };
int cf_bridge_forward(const double* d_theta, int64_t n, int32_t ndim, const double* lo, const double* hi, const double* mean,
                      const double* chol, double* d_z, double* d_log_jac, void* hip_stream);
int cf_bridge_points(const double* d_z, int64_t n, int32_t ndim, const double* lo, const double* hi, const double* mean,
                     const double* chol, int32_t mirror, double* d_theta, double* d_log_jac, void* hip_stream);
int cf_bridge_draw(uint64_t key, int64_t first, int64_t n, int32_t ndim, double* d_z, void* hip_stream);
int cf_bridge_solve(const double* d_l1, int64_t n1, const double* d_l2, int64_t n2, double lstar, double s1, double s2, double tol,
                    int32_t max_iter, double* d_result, double* d_f2, void* hip_stream);

/* ---- Leave-group-out fits (csrc/cosmofit_group.hip; the driver is cosmology-model-fit_amd/leaveout.py) ----------------------
 * With K = C^-1, g = K r (the g rows of cf_infl_device / cf_prec_apply_device) and a group B of m data,
 *   q_B = g_B^T (K_BB)^-1 g_B >= 0,   chi^2 of the data without B = chi^2 - q_B   (exactly; no refit of the covariance):
 * q_B is the chi^2 of the leave-group-out residual e_B = K_BB^-1 g_B = r_B - C_BA C_AA^-1 r_A, whose covariance is K_BB^-1 (m
 * degrees of freedom); g_i^2 / K_ii of cf_infl_device is the case m = 1.  The posterior without B is the chain reweighted by
 * exp(+q_B / 2).
 *
 * cf_group: a list of groups over the n data of a cf_prec, on its device.  Group b holds idx[offsets[b] .. offsets[b + 1]):
 * distinct indices in any order; groups may overlap.  cf_group_create reads K once (a synchronous copy back of the rows named),
 * factors K_BB = L_B L_B^T on the host in long double with compensated sums, inverts the factor in the same precision, rounds once
 * and uploads X_B = L_B^-1 (lower triangular, row-major, zero-padded to a pitch of m rounded up to 16) and the index lists.
 * CF_ERR_INVALID, naming the group: n_groups outside 1 .. CF_GROUP_MAX_GROUPS, a group that is empty or holds more than
 * CF_GROUP_MAX_M data, an index outside 0 .. n - 1 or named twice in a group, a datum with K_ii = 0 (one the likelihood ignores),
 * all factors together beyond CF_GROUP_MAX_BYTES, a non-positive pivot (group and column).  cf_group_check_args states the
 * argument rules without a device (kdiag [n] may be NULL: then no datum is taken as ignored).
 * cf_group_info: out6 = {n, n_groups, device, largest m, indices held, bytes held on the device}; m_out, pitch_out [n_groups]
 * (either may be NULL) the size and the padded pitch of every group.
 * cf_selftest_group_host: the host half alone for one group of m data of K [n x n, row pitch ld; only the LOWER triangle is
 * read]: X_out [m * m] row-major, zeros above the diagonal.  No device needed.
 *
 * cf_group_quad_device: d_q[s * q_pitch + b] = q_b of row s of d_g [S rows at pitch g_pitch >= n], for s < S and every group b,
 * on FP64 matrix cores, asynchronous on `hip_stream`.  The bits of an element depend on its row of g and on its group only: not
 * on S, the row's position, the other groups, or the stream.  Rows >= S and columns no group names are never read.  A non-finite
 * g_i gives NaN in q[s, b] for exactly the groups that hold datum i.  q >= 0; a zero row gives +0.0.  CF_ERR_INVALID before
 * anything is launched (cf_group_quad_check_args states it without a device): S outside 0 .. CF_GROUP_MAX_ROWS, g_pitch < n,
 * q_pitch < n_groups, a null pointer with S > 0.
 *
 * cf_reweight_device: the importance summary of log-weights d_lw [S rows at pitch lw_pitch >= G] over the columns d_x [S rows at
 * pitch x_pitch >= ncol] with base weights d_w0 [S] (NULL: ones).  Per column b of lw the record d_out[b * CF_RW_NCOL(ncol) + ..]
 * (cf_rw_slot): lmax = the largest lw of the used rows whose base weight is > 0 (a row of base weight 0 has weight 0 whatever its
 * lw: a nested run's early points, of weight exp(-40000) = 0, must not set the scale of all the others); with
 * w = w0 exp(lw - lmax): sum w, sum w^2, the largest w, n_used, n_skipped, sum w0 and sum w0^2 over the used rows; from
 * CF_RW_MEAN on sum w (x_i - pivot_i) [ncol], then the upper triangle of sum w (x_i - pivot_i)(x_j - pivot_j), rows i ascending,
 * j = i .. ncol - 1.  pivot [ncol] is a HOST array (the base chain's mean keeps the second moments free of cancellation).  A row
 * is skipped for column b, and counted, when lw[s, b] is NaN or +inf, when any x[s, :] is non-finite, or when w0[s] is not a
 * finite number >= 0; lw = -inf is weight 0 and counts as used.  A column without a used row of positive base weight has
 * lmax = -inf and zero sums.  Order of summation: slices of CF_RW_SLICE consecutive rows, ascending within a slice from 0.0, then
 * the slices ascending (the cf_kde_sum_device contract); the bits of a record depend on its column of lw and on w0, x, pivot
 * only, not on the other columns or the stream.  The only exponential is of a number <= 0.
 * CF_ERR_INVALID before anything is launched (cf_reweight_check_args): a null pointer, S outside 1 .. CF_RW_MAX_ROWS, G outside
 * 1 .. CF_RW_MAX_G, ncol outside 1 .. CF_RW_MAX_NCOL, a pitch below its width, a non-finite pivot, partial sums beyond
 * CF_RW_MAX_WORKSPACE bytes. */
#define CF_GROUP_MAX_GROUPS 1024
#define CF_GROUP_MAX_M 1024
#define CF_GROUP_MAX_BYTES ((int64_t)256 << 20)
#define CF_GROUP_MAX_ROWS ((int64_t)1 << 32)
#define CF_RW_SLICE 2048
#define CF_RW_MAX_NCOL 16
#define CF_RW_MAX_G 4096
#define CF_RW_MAX_ROWS ((int64_t)1 << 31)
#define CF_RW_MAX_WORKSPACE ((int64_t)1 << 30)
#define CF_RW_NCOL(ncol) (8 + (ncol) + (ncol) * ((ncol) + 1) / 2)
enum cf_rw_slot { CF_RW_LMAX = 0, CF_RW_SUM_W = 1, CF_RW_SUM_W2 = 2, CF_RW_MAX_W = 3, CF_RW_N_USED = 4, CF_RW_N_SKIPPED = 5,
                  CF_RW_SUM_W0 = 6, CF_RW_SUM_W0_SQ = 7, CF_RW_MEAN = 8 };
typedef struct cf_group cf_group;
int cf_group_create(cf_prec* prec, int32_t n_groups, const int64_t* offsets, const int32_t* idx, cf_group** out);
void cf_group_destroy(cf_group* g);
int cf_group_info(cf_group* g, int64_t* out6, int64_t* m_out, int64_t* pitch_out);
int cf_group_check_args(int64_t n, const double* kdiag, int32_t n_groups, const int64_t* offsets, const int32_t* idx);
int cf_selftest_group_host(const double* K, int64_t n, int64_t ld, int64_t m, const int32_t* idx, double* X_out);
int cf_group_quad_check_args(int64_t n, int32_t n_groups, const void* d_g, int64_t g_pitch, int64_t S, const void* d_q,
                             int64_t q_pitch);
int cf_group_quad_device(cf_group* g, const double* d_g, int64_t g_pitch, int64_t S, double* d_q, int64_t q_pitch, void* hip_stream);
int cf_reweight_check_args(const void* d_lw, int64_t lw_pitch, int64_t S, int32_t G, const void* d_x, int64_t x_pitch, int32_t ncol,
                           const double* pivot, const void* d_out);
int cf_reweight_device(const double* d_lw, int64_t lw_pitch, int64_t S, int32_t G, const double* d_w0, const double* d_x,
                       int64_t x_pitch, int32_t ncol, const double* pivot, double* d_out, void* hip_stream);

/* ---- Template scans (csrc/cosmofit_scan.hip; the driver is cosmology-model-fit_amd/scan.py) ---------------------------------
 * K candidate templates a_k on top of a base model A0 [n, m0] of the SN residual.  With K' the SN precision matrix deflated by
 * the base (K' = C^-1 - Wt Wt^T, Wt of nuisance.project), g_k = K' a_k, F_k = a_k^T g_k + 1 / sigma_k^2 and
 * v_k = g_k / sqrt(F_k), all formed once on the host (scan.prepare), a residual row r0 gives
 *   s_k = v_k^T r0                     the signed z-score of candidate k given the base
 *   dchi2_k = s_k^2                    what fitting a_k as well would take off the profiled chi^2
 *   statistic: s^2 (sign 0), max(s, 0)^2 (sign +1), max(-s, 0)^2 (sign -1)
 * cf_scan: V [n, K] (column k: v_k) and the live flags on one device.  cf_scan_create reads V [n rows at pitch ld >= K] and
 * live [K] (NULL: all live); the column of a candidate that is not live is stored as zero, so its score is exactly 0.0, and it
 * never wins a row.  V is zero-padded to multiples of the kernel's tile in both directions.  CF_ERR_INVALID: a null argument,
 * n outside 1 .. 32768, K outside 1 .. 2^24 - 1, ld < K, a non-finite entry; CF_ERR_NO_DEVICE without a device.  cf_scan_info
 * reports n, K, the device and the number of live candidates (any pointer may be NULL).
 *
 * cf_scan_apply_device: the kernels alone on caller-supplied rows d_rows [S rows, pitch >= n]; columns >= n and rows >= S are
 * never read (a select, not a product with zero).  Z = R V on FP64 matrix cores (one accumulator per output, ascending k loop, no
 * split-k, no atomics) with the reductions fused behind it, so Z reaches memory only when d_map is given.  Outputs, any may be
 * NULL, not all:
 *   d_best [S], d_best_k [S] (int32), d_s_best [S]: the largest statistic of the row over the live candidates, its candidate
 *     (ties: the smallest k) and the signed score there; a row with a score that is not finite has NaN, -1, NaN, as has a row of
 *     an object without a live candidate;
 *   d_map [S rows at map_pitch >= K]: the scores s_k;
 *   d_colacc [2 K + 1]: RUNNING accumulators the call adds to: (sum w s_k, sum w s_k^2) at 2 k, 2 k + 1 and sum w at 2 K, with
 *     w = d_w [S] (NULL: ones).  Blocks of CF_SCAN_TILE rows are summed in ascending order from 0.0, then added in ascending order.
 * Determinism: the score of (row, k) depends on that row's residuals and column k of V only -- not on S, the row's position, the
 * chunking, the stream, the pointer kind, sign, which outputs are asked for or which other candidates there are; best is the
 * maximum of the statistics of the scores d_map would hold.  The accumulators have the same bits for the same cut of a chain into
 * calls (and chunks) and differ by rounding across cuts.
 * CF_ERR_INVALID: a null cf_scan, S < 0 or > 2^31 - 1, pitch < n, sign outside -1 .. 1, no output at all, map_pitch < K with a
 * map, (S > 0) null rows.
 *
 * cf_scan_eval_device: for every row of d_theta [S * ndim] the residual row of the accessor path (chunks of at most
 * CF_SCAN_CHUNK rows into the handle's workspace, as cf_marg_eval_device), the handle's own chi^2 to d_chi2 [S] (may be NULL) and
 * the kernels above behind it on the same stream.  Checks, all before the first HIP call (cf_scan_check_args states them without
 * a handle: n_outputs counts the non-null outputs, d_chi2 included), all CF_ERR_INVALID: a quasar handle, a handle over several
 * devices, no SN block, a null cf_scan, a cf_scan whose n is not n_sn or that lives on another device, a bad sign, S out of
 * range, no output, a map pitch below K, (S > 0) a null d_theta.  S = 0 is a no-op.  Stream contract: that of
 * cf_marg_eval_device; a cf_scan has ONE scratch, so a call on another stream than the previous call on the same cf_scan first
 * waits, on the host, for the device.  cf_scan_eval: the same on host buffers, synchronous, same bits (colacc is read and
 * written). */
#define CF_SCAN_CHUNK 4096
#define CF_SCAN_TILE 64
#define CF_SCAN_MAX_K (((int64_t)1 << 24) - 1)
typedef struct cf_scan cf_scan;
int cf_scan_create(const double* V, int64_t n, int64_t K, int64_t ld, const uint8_t* live, int32_t device, cf_scan** out);
void cf_scan_destroy(cf_scan* p);
int cf_scan_info(const cf_scan* p, int64_t* n, int64_t* K, int32_t* device, int64_t* n_live);
int cf_scan_apply_device(cf_scan* p, const double* d_rows, int64_t pitch, int64_t S, int32_t sign, const double* d_w, double* d_best,
                         int32_t* d_best_k, double* d_s_best, double* d_map, int64_t map_pitch, double* d_colacc, void* hip_stream);
int cf_scan_eval_device(cf_handle* h, cf_scan* p, const double* d_theta, int64_t S, int32_t sign, const double* d_w, double* d_chi2,
                        double* d_best, int32_t* d_best_k, double* d_s_best, double* d_map, int64_t map_pitch, double* d_colacc,
                        void* hip_stream);
int cf_scan_eval(cf_handle* h, cf_scan* p, const double* theta, int64_t S, int32_t sign, const double* w, double* chi2, double* best,
                 int32_t* best_k, double* s_best, double* map, int64_t map_pitch, double* colacc);
int cf_scan_check_args(int64_t n_sn, int32_t is_quasar, int32_t n_devices, int32_t handle_device, int32_t has_scan, int64_t scan_n,
                       int64_t scan_K, int32_t scan_device, const void* theta, int64_t S, int32_t sign, int32_t n_outputs,
                       const void* map, int64_t map_pitch);
/* Rows per chunk of the following cf_scan_eval_device / cf_scan_eval calls of this handle, 1 .. 65536; 0 restores CF_SCAN_CHUNK.
 * No score or row output depends on it; the column accumulators depend on it by rounding only. */
int cf_scan_set_chunk(cf_handle* h, int64_t rows);
/* The two reductions compiled for the host from a given map [S rows at pitch >= K] (the steps are __host__ __device__ functions
 * shared with the kernels: the statistic of a score, the comparison with its tie rule, a row's step of a block's column sums):
 * best, best_k, s_best [S] and colacc [2 K + 1] (read and written); any output may be NULL; live [K] or NULL.  No device needed. */
int cf_selftest_scan_host(const double* map, int64_t S, int64_t K, int64_t pitch, const uint8_t* live, int32_t sign, const double* w,
                          double* best, int32_t* best_k, double* s_best, double* colacc);

#ifdef __cplusplus
}
#endif
#endif /* COSMOFIT_H */
