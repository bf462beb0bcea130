#!/usr/bin/env python3
"""In-kernel timeline of the streaming per-walker kernel from the DIAGNOSTIC build (tools/build_variant.sh walkerdiag -DCF_DIAG_WALKER):
    COSMOFIT_LIB=$PWD/cosmology-model-fit_amd/libcosmofit_hip_walkerdiag.so python tools/walker_timeline.py [--per-simd N] [W]
Every wave (= walker) of walker_stream_kernel leaves the shader clock at its first instruction, behind each segment's table build
and behind its last store, the 100 MHz real-time counter at both ends and its hardware slot.  Printed for the LAST dispatch of a
run of back-to-back evaluations (flat LambdaCDM, 1701 SNe, W = 4096 walkers by default): per SIMD the end times of its waves as
fractions of the dispatch; over all SIMDs how many of a SIMD's waves are alive against time, the time spent at 4 / 3 / 2 / 1
alive, the spread of the finish times inside a SIMD, and when the waves pass each segment.  CF_TUNE (walker_level=0|1) applies
as in any run; the table in effect is printed."""
import ctypes as C, importlib, os, sys, time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

pkg = importlib.import_module("cosmology-model-fit_amd")
lib = pkg._lib.lib()
lib.cf_debug_walker_clock.argtypes = [C.c_void_p]
MAX_W, SLOTS = 8192, 16  # CF_WALKER_DIAG_MAX, CF_WALKER_DIAG_SLOTS of csrc/cosmofit_kernels.hip
args = sys.argv[1:]
per_simd = 32
if "--per-simd" in args:
    k = args.index("--per-simd")
    per_simd = int(args[k + 1])
    del args[k:k + 2]
W = int(args[0]) if args else 4096
assert W <= MAX_W, "the stamp buffer holds 8192 walkers"

syn = pkg.synthetic.pantheon_like(n_sn=1701, seed=0)
lk = pkg.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"])
import torch

th = torch.from_numpy(pkg.synthetic.walkers(pkg.sn_pantheon.bounds, W, seed=0)).cuda()
out = torch.empty(W, dtype=torch.float64, device="cuda")
st = torch.cuda.current_stream().cuda_stream
assert lk.engine.walker_form(W) == 1, "this batch does not take the streaming form (CF_TUNE walker_stream=1 forces it)"
t0 = time.perf_counter()
while time.perf_counter() - t0 < 2.0:  # the sustained clock, not the ramp
    for _ in range(32):
        lk.engine.eval_device(th.data_ptr(), W, out.data_ptr(), pkg.CF_OUT_LOGP, st)
    torch.cuda.synchronize()
buf = np.zeros(MAX_W * SLOTS, dtype=np.uint64)
assert lib.cf_debug_walker_clock(buf.ctypes.data) == 0
b = buf.reshape(MAX_W, SLOTS).astype(np.int64)[:W]
levels = lk.engine.walker_levels()
lk.engine.close()

n_seg = int((b[0, 1:9] > 0).sum())
rt0 = b[:, 11].min()
start, end = (b[:, 11] - rt0) / 100.0, (b[:, 12] - rt0) / 100.0  # us on the real-time counter, common to the chip
span = end.max()
life = np.maximum(b[:, 9] - b[:, 0], 1)  # shader cycles
clk = life / np.maximum(b[:, 12] - b[:, 11], 1) * 0.1  # GHz
hw = b[:, 10]
# a SIMD: XCC_ID, [se_id 15:13, sh_id 12, cu_id 11:8] and simd_id 5:4 of HW_ID
simd = ((hw >> 32) & 0xf) * 4096 * 4 + ((hw >> 8) & 0xff) * 4 + ((hw >> 4) & 3)
ids, inv = np.unique(simd, return_inverse=True)
counts = np.bincount(inv)
q = lambda x: "min %.3f  p10 %.3f  median %.3f  p90 %.3f  max %.3f" % tuple(np.percentile(x, [0, 10, 50, 90, 100]))
print(f"W = {W}: {W} waves on {len(ids)} SIMDs (waves per SIMD: min {counts.min()} max {counts.max()}), {n_seg} segments, levels in effect {levels}")
print(f"  dispatch span (first wave's first instruction -> last wave's last store): {span:.2f} us;  shader clock [GHz]: {q(clk)}")
print(f"  wave start [fraction of the span]: {q(start / span)}")
print(f"  wave end   [fraction of the span]: {q(end / span)}")
print(f"  wave life  [fraction of the span]: {q((end - start) / span)}")

# per SIMD: the waves' ends, sorted
order = np.lexsort((end, inv))
ends_by_simd = np.split(end[order] / span, np.cumsum(counts)[:-1])
starts_by_simd = np.split(start[order] / span, np.cumsum(counts)[:-1])
print(f"  per SIMD, the end of each of its waves as a fraction of the span (first {min(per_simd, len(ids))} SIMDs of {len(ids)}; --per-simd N for more):")
for i in range(min(per_simd, len(ids))):
    h = int(ids[i])
    print(f"    xcc {h // 16384} cu 0x{(h // 4) % 4096:02x} simd {h % 4}: " + "  ".join(f"{e:.3f}" for e in ends_by_simd[i]))
full = [e for e in ends_by_simd if len(e) == 4]
if full:
    e4 = np.array(full)
    print(f"  SIMDs with four waves ({len(full)}): mean end of the 1st / 2nd / 3rd / 4th wave to finish: " + " / ".join(f"{v:.3f}" for v in e4.mean(axis=0))
          + "   (finishing one after another at equal rates would give 0.25 / 0.50 / 0.75 / 1.00 of the SIMD's own end)")
    print(f"  the same as fractions of the SIMD's OWN last end: " + " / ".join(f"{v:.3f}" for v in (e4 / e4[:, 3:4]).mean(axis=0)))
    print(f"  spread of the finish times inside a SIMD (last - first end) [fraction of the span]: {q(e4[:, 3] - e4[:, 0])}")
    print(f"  median spread: {np.median(e4[:, 3] - e4[:, 0]) * span:.2f} us = {np.median(e4[:, 3] - e4[:, 0]):.3f} of the span")

# waves alive per SIMD against time: an event sweep per SIMD, summed into time spent at each count
T = np.zeros(8)  # SIMD-time [us] at k alive
grid = np.linspace(0.0, span, 41)
alive_grid = np.zeros((len(ids), len(grid)))
for i in range(len(ids)):
    s_, e_ = starts_by_simd[i] * span, ends_by_simd[i] * span
    ev = np.concatenate([np.stack([s_, np.ones_like(s_)], 1), np.stack([e_, -np.ones_like(e_)], 1), [[0.0, 0.0], [span, 0.0]]])
    ev = ev[np.argsort(ev[:, 0], kind="stable")]
    alive = np.cumsum(ev[:, 1])[:-1]
    np.add.at(T, np.clip(alive.astype(int), 0, 7), np.diff(ev[:, 0]))
    alive_grid[i] = (s_[None, :] <= grid[:, None]).sum(1) - (e_[None, :] <= grid[:, None]).sum(1)
tot = T.sum()
print("  share of SIMD-time at k waves alive: " + "  ".join(f"{k}: {100 * T[k] / tot:.1f} %" for k in range(5)) +
      (f"  >4: {100 * T[5:].sum() / tot:.1f} %" if T[5:].sum() > 0 else ""))
print(f"  mean waves alive per SIMD over the span: {(T * np.arange(8)).sum() / tot:.2f}")
print("  waves alive per SIMD against time (fraction of the span: mean over SIMDs | share of SIMDs at 4 / 3 / 2 / 1 / 0):")
for j in range(0, len(grid), 2):
    a = alive_grid[:, j]
    print(f"    {grid[j] / span:.2f}: {a.mean():.2f} | " + " / ".join(f"{100 * np.mean(a == k):3.0f}" for k in (4, 3, 2, 1, 0)))

# when the waves pass each segment's table build, as a fraction of the wave's own life (in shader cycles) and of the span
seg = (b[:, 1:1 + n_seg] - b[:, 0:1]) / life[:, None]
print("  table of segment s built at [fraction of the wave's own life], median over waves: " + "  ".join(f"{np.median(seg[:, s]):.3f}" for s in range(n_seg)))
seg_t = (start[:, None] + seg * (end - start)[:, None]) / span
for s in range(n_seg):
    print(f"    segment {s} built [fraction of the span]: {q(seg_t[:, s])}")
# within a SIMD: how far apart its waves are in WORK done at the moment the first of them ends (1 = a whole walker)
if full:
    lag = []
    for i in range(len(ids)):
        if counts[i] != 4:
            continue
        idx = order[np.sum(counts[:i]):np.sum(counts[:i]) + 4]
        t_first = end[idx[0]]
        for w in idx[1:]:
            tt = np.concatenate([[start[w]], start[w] + seg[w] * (end[w] - start[w]), [end[w]]])
            # share of own life as a proxy of the work done
            lag.append(1.0 - np.interp(t_first, tt, np.concatenate([[0.0], seg[w], [1.0]])))
    print(f"  when a SIMD's first wave ends, share of their own life the other three still have ahead: {q(np.array(lag))}")
