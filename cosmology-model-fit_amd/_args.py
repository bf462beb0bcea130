"""
The argument layer of the Python front ends: what every feature module does to its inputs before it calls the library.

Every check follows one rule: shape and type first, the device last, so that a wrong argument is reported the same with and
without a GPU.  torch is imported where a function needs it, so host-only modules (``interpolator``, ``engine``) can use ``ptr``
without it.
"""
from __future__ import annotations

import ctypes as C


def ptr(a):
    """A contiguous numpy array as ``c_void_p`` (None stays None)."""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def stream_of(device) -> int:
    """The raw handle of torch's current stream on `device`."""
    import torch

    return torch.cuda.current_stream(device).cuda_stream


def require_gpu(who: str):
    """(_lib, the loaded library), or CosmofitError when no GPU is visible.  who: "optimize.maximize", "evidence.bridge", ..."""
    import torch

    from . import _lib as L

    lib = L.lib()  # raises if the HIP library is missing
    if lib.cf_device_count() < 1 or not torch.cuda.is_available():
        raise L.CosmofitError(-2, f"{who} runs in the library's HIP kernels: no GPU is visible (there is no tensor fallback)")
    return L, lib


def float64_tensor(x, what: str):
    """The first two checks of every sample argument: a torch tensor, of float64."""
    import torch

    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{what} takes a tensor on an MI355X (there is no CPU implementation to fall back to)")
    if x.dtype != torch.float64:
        raise ValueError(f"{what} takes float64")
    return x


def on_device(x, what: str):
    """A float64 tensor that lives on a GPU, as it is."""
    import torch

    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError(f"{what} takes a tensor on an MI355X (there is no CPU implementation to fall back to)")
    return float64_tensor(x, what)


def sample_rows(samples, ndim: int, what: str):
    """samples as contiguous float64 rows [n, ndim] on a GPU."""
    samples = float64_tensor(samples, what)
    if samples.dim() != 2 or samples.shape[1] != ndim:
        raise ValueError(f"{what} takes samples [n, {ndim}]")
    if samples.shape[0] > 2**31 - 1:
        raise ValueError(f"{what} takes at most 2^31 - 1 rows")
    return on_device(samples, what).contiguous()


def row_weights(weights, x, what: str):
    """One weight per row of x, finite and >= 0, on the samples' device (a row of weight 0 is skipped and counted); None
    stays None."""
    import torch

    if weights is None:
        return None
    if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float64:
        raise ValueError(f"{what} takes the weights as a float64 tensor")
    if weights.dim() != 1 or weights.shape[0] != x.shape[0]:
        raise ValueError("weights must be [n], one per sample")
    if weights.device != x.device:
        raise ValueError("weights must be on the device of the samples")
    w = weights.contiguous()
    if w.shape[0] and not bool((torch.isfinite(w) & (w >= 0)).all()):
        raise ValueError("weights must be finite and >= 0")
    return w


NO_ACCESSOR_PATH = "no accessor path to take the residuals from"


def single_device_engine(engine, what: str, quasar_reason: str = NO_ACCESSOR_PATH) -> dict:
    """The engine gate of the features that read an engine's accessor path: ``engine.model_info`` of a LikelihoodEngine that
    is no quasar engine (quasar_reason: what such an engine lacks) and lives on one device."""
    info = getattr(engine, "model_info", None)
    if info is None:
        raise ValueError(f"{what} takes a LikelihoodEngine (or a likelihood mirror's .engine)")
    if info["quasar"]:
        raise ValueError(f"{what}: a quasar engine has {quasar_reason}")
    if info["multi_device"]:
        raise ValueError(f"{what}: the engine spans several devices; use one engine per device")
    return info
