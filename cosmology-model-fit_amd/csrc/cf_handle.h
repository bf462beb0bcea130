// cf_handle.h — the handle as every translation unit of the library sees it, and the engine services (cosmofit_api.hip) the
// feature files build on.  Private, host code only: nothing here reaches a kernel or the ABI.
#pragma once
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "cf_host.h"
#include "cf_pack.h"
#include "cosmofit_device.h"

struct PackedFactor {
  DevBuf frags, upd_off, diag_off;
  cf_dev_pack dev{};
  int64_t n = 0, n_pad = 0, bytes = 0;
  int upload(const cf_host_pack& hp) {
    n = hp.n;
    n_pad = hp.n_pad;
    bytes = (int64_t)(hp.frags.size() * sizeof(cf_d2));
    if (frags.ensure(hp.frags.size() * sizeof(cf_d2) + 16)) return CF_ERR_HIP;
    if (upd_off.ensure(hp.upd_off.size() * 8)) return CF_ERR_HIP;
    if (diag_off.ensure(hp.diag_off.size() * 8)) return CF_ERR_HIP;
    HIP_TRY(hipMemcpy(frags.p, hp.frags.data(), hp.frags.size() * sizeof(cf_d2), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(upd_off.p, hp.upd_off.data(), hp.upd_off.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(diag_off.p, hp.diag_off.data(), hp.diag_off.size() * 8, hipMemcpyHostToDevice));
    dev.frags = frags.as<const cf_d2>();
    dev.upd_off = upd_off.as<const int64_t>();
    dev.diag_off = diag_off.as<const int64_t>();
    dev.n_blocks = hp.n_blocks;
    dev.ksplit = hp.ksplit;
    dev.tclasses = hp.tclasses;
    return 0;
  }
};

struct InversePack {
  DevBuf frags, off;
  cf_dev_invpack dev{};
  int64_t bytes = 0;
  int upload(const cf_host_invpack& hp) {
    bytes = (int64_t)(hp.frags.size() * sizeof(cf_d2));
    if (frags.ensure(hp.frags.size() * sizeof(cf_d2))) return CF_ERR_HIP;
    if (off.ensure(hp.off.size() * 8)) return CF_ERR_HIP;
    HIP_TRY(hipMemcpy(frags.p, hp.frags.data(), hp.frags.size() * sizeof(cf_d2), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(off.p, hp.off.data(), hp.off.size() * 8, hipMemcpyHostToDevice));
    dev.frags = frags.as<const cf_d2>();
    dev.off = off.as<const int64_t>();
    dev.n_rowblocks = hp.n_rowblocks;
    return 0;
  }
};

// Pinned host staging: pageable caller buffers make hipMemcpyAsync go through the runtime's own
// bounce buffers; a handle-owned pinned block keeps the host round trip of a small batch short.
struct PinnedBuf {
  void* p = nullptr;
  size_t bytes = 0;
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
  int ensure(size_t need) {
    if (need <= bytes) return 0;
    if (p) { (void)hipHostFree(p); p = nullptr; bytes = 0; }
    HIP_TRY(hipHostMalloc(&p, need, hipHostMallocDefault));
    bytes = need;
    return 0;
  }
};

struct cf_qsr_state;  // cosmofit_quasar.hip

// A host thread that evaluates one replica's slice of a multi-device cf_eval (one per replica beyond the first).
struct cf_worker {
  std::thread th;
  std::mutex m;
  std::condition_variable cv;
  bool has_job = false, done = false, quit = false;
  const double* theta = nullptr;
  double* out = nullptr;
  int64_t W = 0;
  int out_kind = 0, rc = 0;
  std::string err;
};

struct cf_handle {
  int device = 0;
  int solve_mode = 0;
  PinnedBuf stage_in, stage_out;
  InversePack ipack;
  DevBuf partial, arrivals;  // inverse-GEMM solve: chi^2 shares per (row block, walker); arrival counters per panel
  DevBuf partial4;           // small-batch solve: shares per (panel, row block, tile, walker), CF_SMALL_MAX_PANELS panels
  DevBuf epi;                // device copy of `epi_host`: what the solve kernels' last arrivers read of the prior / output epilogue
  cf_epilogue epi_host{};
  hipStream_t stream = nullptr;  // host-buffer evaluations (cf_eval, cf_eval_parts)
  // the ONE workspace is shared by every evaluation of this handle: an evaluation launched on a different stream
  // than the previous one first waits (on the host) for that stream
  hipStream_t last_stream = nullptr;
  bool has_last = false;
  // what cf_last_residuals reports: the batch size of the most recent evaluation and the layout its per-walker kernel was
  // launched with (0 walker rows, 1 the small-batch solve's fragment order); -1 / 0 before the first evaluation
  int64_t last_W = -1;
  int last_layout = 0;
  // timing ring: per evaluation 4 events (before the walker kernel, behind it, behind the small-block / growth kernels, behind the solve)
  std::vector<hipEvent_t> ev;
  int timing_slots = 0, timing_stride = 1;
  int64_t timed_calls = 0, eval_calls = 0;
  cf_dev_desc d{};
  PackedFactor pack;
  DevBuf z_cmb, z_hel, obs, sn_step, sn_rec, log10_tab;
  DevBuf stream_rec, stream_row;  // the SN records in segment order and their rows (walker_stream_kernel: cf_stream_pack.h)
  cf_stream_args sargs{};         // rec == null: the data do not fit the streaming form
  DevBuf bao_z, bao_val, bao_inv_cov, bao_qty, gl_x, gl_w, fixed_mu, cc_z, cc_h, cc_inv_cov, nu_grid, ln_grid, nu_sw, ln_sw, exp2_tab, sn_lin, sn_dir;
  DevBuf theta, out, delta, ypk, chi2_extra, nonfinite;
  DevBuf fs8_z, fs8_val, fs8_inv_cov, fs8_fid, fs8_step_of, fs8_order, fs8_tab, fs8_pts;
  DevBuf bao_nodes, bao_base;  // [max_walkers][n_bao][CF_BAO_NODES] table nodes for small_blocks_kernel; first node per datum
  PinnedBuf done_flags;           // [CF_DONE_FLAGS] words the evaluation's last kernel sets as each panel's results reach the staging block
  unsigned long long done_seq = 0;
  int done_armed = 0;             // panels whose word the current synchronous call waits for (0: wait for the stream)
  bool theta_on_host = false;     // set around a zero-copy evaluation: theta is the pinned staging block (reads cross the host link)
  bool has_small_blocks = false;  // BAO and / or CMB block present
  bool has_growth = false;        // growth-rate block present
  cf_qsr_state* qsr = nullptr;    // a quasar likelihood (cf_create_quasar): its per-walker kernel replaces walker_kernel
  int64_t max_walkers = 0;
  double pack_probe_rel = 0.0;
  int cu_count = 0;
  char arch[64] = {0};
  // replicas on further devices (owned by the primary handle) and their worker threads
  std::vector<cf_handle*> peers;
  std::vector<std::unique_ptr<cf_worker>> workers;
  std::mutex mu;
  // fit report (cf_resid_device): sqrt(C_ii) of the SN / BAO data, computed on the host at cf_create and uploaded at the first
  // call; per-chunk outputs of the accessor path (mu_corr, bao_theory, the chi^2 shares); rows per chunk (0: CF_RESID_CHUNK)
  std::vector<double> sigma_sn_host, sigma_bao_host;
  DevBuf sigma_sn, sigma_bao, r_mc, r_bt, r_blk, r_snb, r_fsb;
  bool sigma_uploaded = false;
  int64_t resid_rows = 0, resid_chunk = 0;
  int64_t mock_chunk = 0;  // rows per chunk of cf_mock_eval_device (0: CF_MOCK_CHUNK); it shares the fit report's chunk buffers
  // attribution (cf_infl_device): per-chunk g = K r and the contrib / z rows the caller did not ask for but an accumulator reads,
  // each [rows][n] and allocated when first needed; rows per chunk (0: CF_INFL_CHUNK).  The residual rows are the fit report's.
  DevBuf i_g, i_contrib, i_z;
  int64_t infl_chunk = 0;
  int64_t cscale_chunk = 0;  // rows per chunk of cf_cscale_eval_device (0: CF_CSCALE_CHUNK); residual rows and chi^2 shares are the fit report's
  int64_t marg_chunk = 0;  // rows per chunk of cf_marg_eval_device (0: CF_MARG_CHUNK); it shares the fit report's chunk buffers
  int64_t scan_chunk = 0;  // rows per chunk of cf_scan_eval_device (0: CF_SCAN_CHUNK); it shares the fit report's chunk buffers
};

// An entry point's hold on its handle: h->mu locked and the handle's device current (cf_host.h: DeviceScope) until it returns.
// The helpers that need both take a `const HandleScope&` and reach the handle through it.
struct HandleScope {
  cf_handle* const h;
  std::lock_guard<std::mutex> lock;
  DeviceScope on_device;
  const hipError_t err;
  explicit HandleScope(cf_handle* handle) : h(handle), lock(h->mu), on_device(h->device), err(on_device.err) {}
};

// Host-side preparation shared by the replicas of a multi-device handle: the factor is packed (and, for the
// inverse-GEMM solve, inverted in extended precision) once, then uploaded to every device.
struct HostPrep {
  bool packed = false;
  int solve_mode = 0;
  double probe_rel = 0.0;
  cf_host_invpack ip;
  cf_host_pack hp;
};

// n values to the device: `b` grows to hold them, and `dev` (a descriptor field as a rule) becomes its typed pointer.
template <class T>
int upload(DevBuf& b, const T* src, int64_t n) {
  if (b.ensure((size_t)n * sizeof(T))) return CF_ERR_HIP;
  HIP_TRY(hipMemcpy(b.p, src, (size_t)n * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}
template <class T>
int upload(DevBuf& b, const T* src, int64_t n, const T*& dev) {
  if (int rc = upload(b, src, n)) return rc;
  dev = b.as<const T>();
  return 0;
}

// cosmofit_api.hip.  The workspace for W walkers; one evaluation of W walkers ordered on `st` (a mucorr_out buffer selects the
// accessor form of the per-walker kernel); rows per chunk of one of the loops over the workspace (cf_*_set_chunk); cf_create's
// descriptor checks and one handle on one device.  Hidden: private to the library, and called directly as when they were static.
#pragma GCC visibility push(hidden)
int ensure_workspace(cf_handle* h, int64_t W);
int launch_path(cf_handle* h, const double* d_theta, int64_t W, double* d_out, int out_kind, hipStream_t st, double* dm_out,
                double* mucorr_out, double* blocks_out, double* bao_out, double* chi2_sn_out = nullptr,
                double* fs8_block_out = nullptr, double* fs8_theory_out = nullptr);
int set_chunk(cf_handle* h, int64_t cf_handle::*field, int64_t rows, const char* fn);
int validate_desc(const cf_desc* c);
int create_one(const cf_desc* c, int device, HostPrep& prep, cf_handle** out);

// cosmofit_quasar.hip.  The per-walker kernel of a quasar handle (launch_eval) and the end of its tables (cf_destroy).
int cf_qsr_launch(const cf_qsr_state* q, const double* theta, int64_t W, double* delta, double* extra, int out_kind, double* th_copy,
                  hipStream_t st);
void cf_qsr_free(cf_qsr_state* q);
#pragma GCC visibility pop
