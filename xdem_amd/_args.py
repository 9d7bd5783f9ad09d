"""The one place an array becomes an argument of ``libxdemhip``: the ctypes pointer types, what a NumPy array or a torch tensor is
to the library (address, ``F32`` / ``F64`` code, ``HOST`` / ``DEVICE`` memory space), and the few ways a raster is made readable for
it (DESIGN.md has the table of which call site promotes to what and which refuses).  Plain functions over ``_lib``, NumPy and --
imported where a tensor is at hand -- torch.

An address is a bare integer: whoever takes one with ``ptr`` keeps the array alive until the call has returned.  The typed pointers
of ``dp`` .. ``u64p`` hold a NumPy array themselves (``ctypes.data_as`` keeps a reference) but NOT a tensor: a tensor's address is cast,
nothing is held, and the caller keeps the tensor alive as it does for ``ptr``."""
from __future__ import annotations

import contextlib
import ctypes
import warnings
from typing import NamedTuple

import numpy as np

from . import _lib

DP = ctypes.POINTER(ctypes.c_double)
IP = ctypes.POINTER(ctypes.c_int)
I64P = ctypes.POINTER(ctypes.c_int64)
I32P = ctypes.POINTER(ctypes.c_int32)
U64P = ctypes.POINTER(ctypes.c_uint64)
FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


# ---- what an array is to the library ------------------------------------------------------------------------------------------------
def is_tensor(x) -> bool:
    """A torch tensor (or anything that answers ``is_cuda``).  The sites that asked ``type(x).__module__.startswith("torch")`` before --
    ``stats._Input``, the volume inputs, ``convolution`` -- answer differently for one kind of input only: a Tensor subclass defined
    outside torch was taken for host data there and is a tensor here."""
    return hasattr(x, "is_cuda")


def np_dtype(x) -> np.dtype:
    """The NumPy dtype of an array, a tensor or a dtype of either kind."""
    if not isinstance(x, (np.dtype, type, str)):
        x = getattr(x, "dtype", x)
        if str(x).startswith("torch."):
            return np.dtype(str(x)[6:])
    return np.dtype(x)


def code(x) -> int:
    return _lib.F32 if np_dtype(x) == np.float32 else _lib.F64


def ptr(x):
    """The address of an array's or a tensor's first element; None stays None."""
    if x is None:
        return None
    return x.data_ptr() if is_tensor(x) else x.ctypes.data


def space(x) -> int:
    return _lib.DEVICE if is_tensor(x) else _lib.HOST


def _typed(pointer_type):
    def typed(a):
        if a is None:
            return None
        return ctypes.cast(a.data_ptr(), pointer_type) if is_tensor(a) else a.ctypes.data_as(pointer_type)
    return typed


dp, ip, i64p, i32p, u64p, chars = (_typed(t) for t in (DP, IP, I64P, I32P, U64P, ctypes.c_char_p))


def c_doubles(values):
    """A sequence of numbers as the library's ``const double*``."""
    return dp(np.ascontiguousarray(values, dtype=np.float64))


def same_space(x, like):
    """``x`` where ``like`` lives: uploaded to its device, fetched to the host, or as it is."""
    if is_tensor(like) and not is_tensor(x):
        import torch

        return torch.from_numpy(x).to(like.device)
    if not is_tensor(like) and is_tensor(x):
        return x.cpu().numpy()
    return x


def synchronize_torch(t) -> None:
    """Wait for the current torch stream of ``t``'s device: what ``t`` holds is complete before the library reads it on its own stream."""
    import torch

    torch.cuda.current_stream(t.device).synchronize()


@contextlib.contextmanager
def torch_stream_scope(ctx, x, reset: bool = False):
    """The body of a one-call wrapper around its library call.  For a tensor ``x``: the context's call lock held and its stream set to
    the current torch stream of ``x``'s device, so that the call is ordered among the caller's work without a host synchronisation;
    ``reset`` puts the context's own stream back afterwards.  For a host array: nothing."""
    if not is_tensor(x):
        yield
        return
    import torch

    with ctx.call_lock:
        ctx.set_stream(torch.cuda.current_stream(x.device).cuda_stream)
        try:
            yield
        finally:
            if reset:
                ctx.set_stream(None)


# ---- a float raster the library can read --------------------------------------------------------------------------------------------
def nan_filled(a):
    """A masked array with NaN in its masked cells, anything else as an array as it is; None stays None."""
    if a is None:
        return None
    return np.asarray(a.filled(np.nan) if isinstance(a, np.ma.MaskedArray) else a)


def host_float(a, default=np.float32) -> np.ndarray:
    """A C-contiguous float32 / float64 host array: masked cells NaN, any other dtype promoted to ``default``; an input that
    qualifies already is returned itself."""
    a = np.ascontiguousarray(nan_filled(a))
    return a if a.dtype in FLOATS else a.astype(default)


def device_float(t, what: str, ndim: int | None = 2):
    """``t`` if it is a contiguous float32 / float64 CUDA tensor of ``ndim`` dimensions (None: any); ValueError(``what``) otherwise."""
    import torch

    if not (t.is_cuda and t.is_contiguous() and t.dtype in (torch.float32, torch.float64) and (ndim is None or t.dim() == ndim)):
        raise ValueError(what)
    return t


def flat_float(x, what: str):
    """A raster as the volume passes read it: a flat contiguous float32 / float64 array or CUDA tensor, masked cells NaN.  A tensor of
    another dtype or layout is converted, not refused -- only a host tensor is (``what`` names the argument).  Integer rasters become
    float32, as geoutils' get_array_and_mask makes them."""
    if is_tensor(x):
        import torch

        if not x.is_cuda:
            raise ValueError(f"{what}: a tensor input must live on the GPU (pass host data as a NumPy array)")
        if x.dtype not in (torch.float32, torch.float64):
            x = x.to(torch.float32)
        return x.contiguous().reshape(-1)
    if isinstance(x, np.ma.MaskedArray):   # (an integer raster cannot hold the NaN of its masked cells: promoted first)
        data = np.array(x.data, dtype=x.dtype if x.dtype in FLOATS else np.float32)
        data[np.ma.getmaskarray(x)] = np.nan
        x = data
    return host_float(x).reshape(-1)


def flat_mask(m, like):
    """A mask as flat uint8, non-zero = set, where ``like`` lives."""
    m = m.contiguous().reshape(-1) if is_tensor(m) else np.asarray(m).reshape(-1).astype(bool)
    return mask_u8(m, like, nonzero=True)


def mask_u8(m, like, nonzero: bool = False):
    """A mask as contiguous uint8 where ``like`` lives.  The values are cast as they are -- the masks next to a raster pair -- or, with
    ``nonzero``, every non-zero value becomes 1 (the statistics and the volumes)."""
    if is_tensor(like):
        import torch

        t = m if is_tensor(m) else torch.from_numpy(np.ascontiguousarray(m, dtype=bool if nonzero else np.uint8))
        return (t != 0 if nonzero else t).to(device=like.device, dtype=torch.uint8).contiguous()
    a = m.cpu().numpy() if is_tensor(m) else m
    if nonzero:
        return np.ascontiguousarray(np.asarray(a, dtype=bool)).view(np.uint8)
    return np.ascontiguousarray(a, dtype=np.uint8)


def plane_in_space(plane, device):
    """A float32 / float64 plane where a call reads it: on ``device`` (a torch device: a contiguous CUDA tensor, uploaded or moved
    if need be, the current stream synchronised) or, with ``device`` None, on the host (a contiguous NumPy array).  Other dtypes
    become float64.  Returns (pointer, dtype code, shape, the array to keep alive)."""
    if device is not None:
        import torch

        if is_tensor(plane):
            t = plane
        else:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", UserWarning)   # (a read-only array is only read)
                t = torch.from_numpy(np.ascontiguousarray(nan_filled(plane)))
        if t.dtype not in (torch.float32, torch.float64):
            t = t.to(torch.float64)
        t = t.to(device).contiguous()
        synchronize_torch(t)
    else:
        t = host_float(plane.cpu().numpy() if is_tensor(plane) else plane, np.float64)
    return ptr(t), code(t), tuple(t.shape), t


class RasterPair(NamedTuple):
    ref: int                 # pointers for the library's create call
    tba: int
    inlier: int | None
    dtype: np.dtype
    code: int                # _lib.F32 / _lib.F64
    shape: tuple
    memspace: int            # _lib.HOST / _lib.DEVICE
    keep: tuple              # the arrays the pointers point into: alive at least until the create call returns


def raster_pair(ref, tba, inlier_mask) -> RasterPair:
    """Two rasters on one grid and an optional inlier mask, as a plan's create call takes them.  ``ref`` / ``tba``: 2-D arrays
    (promoted to float64 if either is float64, else to float32, when their dtypes differ or are not float), or contiguous 2-D float32 /
    float64 CUDA tensors of one dtype, never copied (the plan keeps them alive; the current torch stream is synchronised).  The mask
    goes as uint8: next to device rasters a host mask is uploaded and a device mask converted, on the rasters' device."""
    if is_tensor(ref):
        refused = "device inputs must be contiguous 2D float32 / float64 CUDA tensors of the same shape and dtype"
        device_float(ref, refused)
        device_float(tba, refused)
        if ref.dtype != tba.dtype or ref.shape != tba.shape:
            raise ValueError(refused)
        inl = None if inlier_mask is None else mask_u8(inlier_mask, ref)
        synchronize_torch(ref)
    else:
        ref, tba = np.ascontiguousarray(ref), np.ascontiguousarray(tba)
        if ref.shape != tba.shape or ref.ndim != 2:
            raise ValueError("ref and tba must be 2D arrays of the same shape")
        if ref.dtype != tba.dtype or ref.dtype not in FLOATS:
            dt = np.float64 if np.float64 in (ref.dtype, tba.dtype) else np.float32
            ref, tba = ref.astype(dt), tba.astype(dt)
        inl = None if inlier_mask is None else mask_u8(inlier_mask, ref)
    return RasterPair(ptr(ref), ptr(tba), ptr(inl), np_dtype(ref), code(ref), tuple(ref.shape), space(ref), (ref, tba, inl))
