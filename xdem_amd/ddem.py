"""``xdem.dDEM``: a difference of two DEMs with its time span and, once its voids are filled, the filled array (xdem/ddem.py:81-269).

Upstream's dDEM is a geoutils Raster that takes over the ``__dict__`` of the raster it is made from; this one does the same with an
``xdem_amd.DEM``, so it has that DEM's ``data``, ``transform``, ``crs``, ``nodata``, ``res`` and ``shape``.  ``data`` is a host array, a
masked array or a device tensor; ``filled_data`` comes back in the memspace of ``data``.

Of ``interpolate``'s three methods "regional_hypsometric" runs on the device (``xdem_amd.volume.hypsometric_interpolation``); "idw" and
"local_hypsometric" end in GDAL's ``fillnodata`` upstream and are refused.  A ``DEMCollection`` fills all its
dDEMs in one batched pass instead of calling ``interpolate`` on each (xdem_amd/demcollection.py).
"""
from __future__ import annotations

from typing import Any

import numpy as np

from . import volume
from ._args import is_tensor
from .dem import DEM
from .vector import Vector

_GDAL_METHODS = ("idw", "local_hypsometric")


def _has_voids(data) -> bool:
    """A masked or a non-finite pixel: what a fill fills.  (Upstream's test in ``filled_data``, ddem.py:128, looks for NaN and the
    mask and lets an infinity pass; here an infinity is a void on every route, as the stack's subtraction pass counts it.)"""
    if is_tensor(data):
        return not bool(data.isfinite().all().item())
    if isinstance(data, np.ma.MaskedArray) and np.any(np.ma.getmaskarray(data)):
        return True
    return not bool(np.all(np.isfinite(np.asarray(data))))


def raster_of(data, transform, crs=None, nodata=None) -> DEM:
    """A DEM around `data` as it is -- a device tensor stays one (``DEM(...)`` itself makes a host array of what it gets)."""
    if not is_tensor(data):
        return DEM.from_array(data, transform, crs, nodata)
    if data.ndim != 2:
        raise ValueError("DEM data must be 2D")
    dem = DEM.__new__(DEM)
    dem.data = data
    dem.transform = tuple(float(v) for v in ((transform.a, transform.b, transform.c, transform.d, transform.e, transform.f)
                                             if hasattr(transform, "a") else transform))
    dem.crs, dem.nodata = crs, nodata
    return dem


def mask_as_array(mask, like=None) -> Any:
    """A mask given as an array, a tensor, a DEM of a mask or a Vector, as a boolean array / tensor.  For a DEM upstream's rule
    (ddem.py:70-72): the true value is the raster's maximum, unless that is 0 or False.  A Vector is burnt into the grid of the
    raster `like` on the GPU (``Vector.create_mask``), in the memspace of that raster's data."""
    if isinstance(mask, Vector):
        if like is None:
            raise ValueError("a Vector mask needs the raster it is burnt into")
        return mask.create_mask(like, device=is_tensor(like.data))
    if isinstance(mask, DEM):
        data = mask.data
        if is_tensor(data):
            top = data[~data.isnan()].max() if data.is_floating_point() else data.max()
            return data == (top if top.item() not in (0, False) else True)
        top = np.nanmax(data)
        return np.asarray(data == (top if top not in [0, False] else True)).squeeze()
    if is_tensor(mask) or isinstance(mask, np.ndarray):
        return mask
    raise TypeError(f"Raster has invalid type: {type(mask)}. Expected one of: ['xdem_amd.DEM', 'numpy.ndarray', 'torch.Tensor']")


class dDEM(DEM):
    """A difference-DEM object."""

    def __init__(self, raster: DEM, start_time: np.datetime64, end_time: np.datetime64, error: Any | None = None):
        self.__dict__ = raster.__dict__   # (as upstream: the dDEM takes over the raster's state)
        self.start_time = start_time
        self.end_time = end_time
        self.error = error
        self._filled_data = None
        self._fill_method = ""
        self._known_voids = None   # (array object, has voids, the tensor's version then): set by a DEMCollection, whose subtraction pass counted them

    def __str__(self) -> str:
        return f"dDEM from {self.start_time} to {self.end_time}.\n\n{super().__str__()}"

    def copy(self, new_array=None) -> "dDEM":
        if new_array is None:
            new_array = self.data.clone() if is_tensor(self.data) else self.data.copy()
        return dDEM.from_array(new_array, self.transform, self.crs, self.start_time, self.end_time)

    @property
    def filled_data(self):
        """The filled array if there is one, else the data if it has no void, else None."""
        if self._filled_data is not None:
            return self._filled_data
        known = self._known_voids
        if known is not None and known[0] is self.data and known[2] == getattr(self.data, "_version", 0):
            voids = known[1]
        else:
            voids = _has_voids(self.data)
        if voids:
            return None
        return self.data if is_tensor(self.data) else np.asarray(self.data)

    @filled_data.setter
    def filled_data(self, array) -> None:
        size = array.numel() if is_tensor(array) else np.size(array)
        data_size = self.data.numel() if is_tensor(self.data) else self.data.size
        assert data_size == size, f"Array shape '{tuple(array.shape)}' differs from the data shape '{tuple(self.data.shape)}'"
        self._filled_data = array.reshape(tuple(self.data.shape)) if is_tensor(array) else np.asarray(array).reshape(self.data.shape)

    @property
    def fill_method(self) -> str:
        """The fill method used for the filled_data (upstream never sets it: it stays "")."""
        return self._fill_method

    @property
    def time(self) -> np.timedelta64:
        return self.end_time - self.start_time

    @classmethod
    def from_array(cls, data, transform, crs, start_time: np.datetime64, end_time: np.datetime64, nodata=None, error: float = None) -> "dDEM":
        return cls(raster_of(data, transform, crs, nodata), start_time=start_time, end_time=end_time, error=error)

    def interpolate(self, method: str = "idw", reference_elevation=None, mask=None):
        """Fill the voids with `method` and return ``filled_data``.

        "regional_hypsometric": the dDEM's median per 50 m elevation bin of `reference_elevation` (an array, a tensor or a DEM on this
        grid) over `mask` (a boolean array, a DEM of a mask or a Vector), evaluated at the voids inside the mask.  "idw" and "local_hypsometric"
        are GDAL's fillnodata upstream and raise NotImplementedError here."""
        if reference_elevation is not None:
            ref_data = reference_elevation.data if isinstance(reference_elevation, (DEM, np.ma.MaskedArray)) else reference_elevation
            assert tuple(ref_data.shape) == tuple(self.data.shape), (
                f"'reference_elevation' shape ({tuple(ref_data.shape)})" f" different from 'self' ({tuple(self.data.shape)})"
            )
        if method in _GDAL_METHODS:
            raise NotImplementedError(f"Interpolation method '{method}' ends in GDAL's fillnodata upstream, which has no counterpart "
                                      "here; use 'regional_hypsometric'.")
        if method != "regional_hypsometric":
            raise NotImplementedError(f"Interpolation method '{method}' not supported")
        assert reference_elevation is not None
        assert mask is not None
        mask_array = mask_as_array(mask, self).reshape(tuple(self.data.shape))
        ref = reference_elevation.data if isinstance(reference_elevation, DEM) else reference_elevation
        filled = volume.hypsometric_interpolation(self.data, ref, mask=mask_array)
        self.filled_data = filled.data if isinstance(filled, np.ma.MaskedArray) else filled
        return self.filled_data
