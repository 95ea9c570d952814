"""Wavelets for the convolutional modelling operators (host NumPy, as
pylops.utils.wavelets: a wavelet is a handful of taps built once)."""
import numpy as np


def ricker(t, f0: float = 10.0):
    """Ricker wavelet w = (1 - 2 (pi f0 t)^2) exp(-(pi f0 t)^2) on the
    symmetric axis built from the non-negative ``t`` (t[0] == 0):
    returns (w, t_full, wcenter) with len(w) == 2 len(t) - 1 and the
    peak w[wcenter] == 1."""
    t = np.asarray(t, dtype=np.float64)
    if t.ndim != 1 or t.size < 1:
        raise ValueError("ricker: t must be a non-empty 1-D axis")
    t_full = np.concatenate((-t[:0:-1], t))
    a = (np.pi * f0 * t_full) ** 2
    w = (1.0 - 2.0 * a) * np.exp(-a)
    return w, t_full, int(np.argmax(np.abs(w)))
