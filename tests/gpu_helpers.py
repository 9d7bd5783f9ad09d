"""Helpers shared by the GPU tests that call the C ABI with the caller's device memory (``XDEMHIP_DEVICE``)."""
import ctypes

import numpy as np

DP = ctypes.POINTER(ctypes.c_double)


def _dev(a):
    """A device copy of a NumPy array, complete before the library's own stream reads it."""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _dev_empty(shape, dtype):
    import torch

    return torch.empty(shape, dtype=torch.float32 if np.dtype(dtype) == np.float32 else torch.float64, device="cuda")


def _back(ctx, t):
    ctx.synchronize()   # the library launches on its own stream
    return t.cpu().numpy()


def _with_nans(rng, a, k):
    a = a.copy()
    a.reshape(-1)[rng.choice(a.size, k, replace=False)] = np.nan
    return a
