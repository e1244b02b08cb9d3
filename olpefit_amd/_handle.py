"""What the wrappers of the library's fold objects share: the lifetime of a ctypes handle,
array pointers and the reading of a saved ``.npz``."""
from __future__ import annotations

import numpy as np

from . import _lib


class Handle:
    """A ctypes handle ``_h`` of the loaded library ``_lib``, freed once by the library
    function named ``_destroy``: by ``close()``, on leaving a ``with`` block, or with the
    object.  A subclass sets ``_lib``, then ``_h`` once its create call has succeeded."""

    _destroy: str
    _h = None

    def close(self):
        if self._h:
            getattr(self._lib, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _pd(a):
    return a.ctypes.data_as(_lib._pd)


def _u64(a):
    return a.ctypes.data_as(_lib._pu64)


def load_npz(path):
    """What the ``save`` of ``Corner``, ``Residuals`` or ``Autocorr`` wrote, as a dict of
    arrays."""
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}
