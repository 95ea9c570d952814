"""Kirchhoff demigration / migration local operators — pylops'
waveeqprocessing.Kirchhoff (kinematic: dynamic=False, wavfilter=False) and
the LSM wrapper the reference's least-squares-migration tutorial places
inside MPIVStack, on the HIP kernels of csrc/kirchhoff.hip (pam_kirch) and
csrc/conv1d.hip (pam_conv1d, the wavelet stage).

pylops is not vendored, so the convention is restated in include/pam.h and
locked by tests/kirchref.py: with the traveltimes in samples,
q = trav_srcs[i, is] / dt + trav_recs[i, ir] / dt, it = floor(q),
w = q - it, the pair of trace (is, ir) and image point i contributes iff
0 <= it < nt - 1, and then
    forward  d[is, ir, it] += m[i] (1 - w);  d[is, ir, it + 1] += m[i] w
    adjoint  m[i] += (1 - w) d[is, ir, it] + w d[is, ir, it + 1]
followed (forward) or preceded (adjoint) by the convolution of every trace
with the wavelet."""
import numpy as np
import torch

from . import kernels
from .convolve import Convolve1DLocal
from .distributedarray import as_torch_dtype
from .localops import LocalOperator


def _grid(z, x, y):
    """(ni, ndim) coordinates of the image points, (y,) x, z order, the
    model flattened in C order over ((ny,) nx, nz)."""
    axes = [np.asarray(a, dtype=np.float64).ravel()
            for a in ((x, z) if y is None else (y, x, z))]
    mesh = np.meshgrid(*axes, indexing="ij")
    return np.stack([g.ravel() for g in mesh], axis=1)


def traveltime_table(z, x, srcs, recs, vel, y=None):
    """Straight-ray traveltimes for a constant velocity ``vel``:
    sqrt(dx^2 (+ dy^2) + dz^2) / vel from every source / receiver to every
    image point.  ``srcs`` (2, ns) holds (x, z) rows — (3, ns): (y, x, z)
    when ``y`` is given — and ``recs`` likewise.  Returns float64 arrays
    (trav_srcs (ni, ns), trav_recs (ni, nr)), pylops' layout, the image
    points flattened in C order over ((ny,) nx, nz).  Construction-time
    work on the host."""
    if np.ndim(vel) != 0:
        raise ValueError("analytic traveltimes need one constant velocity; "
                         "pass tables with mode='byot' for anything else")
    pts = _grid(z, x, y)
    out = []
    for name, pos in (("srcs", srcs), ("recs", recs)):
        pos = np.asarray(pos, dtype=np.float64)
        if pos.ndim != 2 or pos.shape[0] != pts.shape[1]:
            raise ValueError(f"{name} must have shape ({pts.shape[1]}, n), "
                             f"got {pos.shape}")
        dist2 = np.zeros((pts.shape[0], pos.shape[1]))
        for c in range(pts.shape[1]):
            dist2 += (pts[:, c:c + 1] - pos[c][None, :]) ** 2
        out.append(np.sqrt(dist2) / float(vel))
    return out[0], out[1]


class KirchhoffLocal(LocalOperator):
    """Kinematic Kirchhoff demigration (matvec) and migration (rmatvec) of
    shape (ns * nr * nt, ni) — pylops Kirchhoff with dynamic=False and
    wavfilter=False: the reflectivity on the (``x``, ``z``) grid — with
    ``y``: (y, x, z) — flattened in C order, is spread along the
    source-point-receiver traveltimes into ns * nr traces on the time axis
    ``t`` (it must start at 0; only t[1] - t[0] is used) with linear
    interpolation, then every trace is convolved with ``wav`` centred at
    ``wavcenter``.  ``wav=None`` is an extension: the bare spread.

    ``mode="analytic"`` builds straight-ray tables for the constant
    velocity ``vel`` (traveltime_table); ``mode="byot"`` takes
    ``trav = (trav_srcs (ni, ns), trav_recs (ni, nr))`` in seconds, NumPy
    arrays or tensors.  The tables are converted once, here, to samples
    and to the trace-major layout of pam_kirch (``qs`` (ns, ni), ``qr``
    (nr, ni)) and move to the device of the first vector.

    matvec = conv o spread, rmatvec = gather o conv^T: two launches each
    way.  The migration (gather) is reproducible bit for bit.  The
    demigration (spread) accumulates each trace in LDS with float adds
    whose order depends on the schedule: it equals the exact sum within
    rounding, (n + 2) eps sum|m_i| weight for a sample with n
    contributions, but its last bits are not pinned."""

    def __init__(self, z, x, t, srcs, recs, vel=None, wav=None,
                 wavcenter: int = 0, y=None, mode: str = "analytic",
                 trav=None, dtype="float64", dynamic: bool = False,
                 wavfilter: bool = False):
        if dynamic:
            raise NotImplementedError(
                "dynamic=True (amplitude and obliquity weights) needs "
                "amplitude tables and angle apertures this kinematic "
                "kernel does not carry")
        if wavfilter:
            raise NotImplementedError(
                "wavfilter=True (the half-derivative wavelet filter) is "
                "not applied here: filter the wavelet on the host and "
                "pass the result as wav")
        if mode == "eikonal":
            raise NotImplementedError(
                "mode='eikonal' needs an eikonal solver this project does "
                "not carry: compute the tables elsewhere and pass them "
                "with mode='byot', trav=(trav_srcs, trav_recs)")
        if mode not in ("analytic", "byot"):
            raise ValueError(f"mode must be 'analytic' or 'byot', got "
                             f"{mode!r}")
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype("float64"), np.dtype("float32")):
            raise TypeError(f"KirchhoffLocal is real: dtype float64 or "
                            f"float32, got {self.dtype}")
        tdt = as_torch_dtype(self.dtype)
        t = np.asarray(t, dtype=np.float64).ravel()
        if t.size < 2 or not t[1] > t[0]:
            raise ValueError("t needs at least two increasing samples")
        self.nt, self.dt = int(t.size), float(t[1] - t[0])
        axes = (x, z) if y is None else (y, x, z)
        self.dims = tuple(int(np.size(a)) for a in axes)
        ni = int(np.prod(self.dims))
        if mode == "analytic":
            if vel is None:
                raise ValueError("mode='analytic' needs vel")
            trav = traveltime_table(z, x, srcs, recs, vel, y=y)
        elif trav is None or len(trav) != 2:
            raise ValueError("mode='byot' needs trav=(trav_srcs, trav_recs)")
        tabs = []
        for name, tab in zip(("trav_srcs", "trav_recs"), trav):
            if isinstance(tab, torch.Tensor):
                tab = tab.detach().cpu().numpy()
            tab = np.asarray(tab, dtype=np.float64)
            if tab.ndim != 2 or tab.shape[0] != ni or tab.shape[1] < 1:
                raise ValueError(f"{name} must have shape ({ni}, n), got "
                                 f"{tab.shape}")
            # samples, trace-major: q[is, i] = trav[i, is] / dt
            tabs.append(torch.from_numpy(
                np.ascontiguousarray(tab.T / self.dt)).to(tdt))
        self.qs, self.qr = tabs
        self.ns, self.nr, self.ni = self.qs.shape[0], self.qr.shape[0], ni
        self.shape = (self.ns * self.nr * self.nt, ni)
        self.conv = None
        if wav is not None:
            self.conv = Convolve1DLocal((self.ns * self.nr, self.nt), wav,
                                        offset=wavcenter, axis=-1,
                                        dtype=self.dtype)

    def _tables(self, device):
        if self.qs.device != device:
            self.qs, self.qr = self.qs.to(device), self.qr.to(device)
        return self.qs, self.qr

    def matvec(self, x):
        d = torch.empty((self.ns, self.nr, self.nt), dtype=x.dtype,
                        device=x.device)
        kernels.kirchhoff(d, x.reshape(-1), *self._tables(x.device), False)
        d = d.view(-1)
        return d if self.conv is None else self.conv.matvec(d)

    def rmatvec(self, x):
        if self.conv is not None:
            x = self.conv.rmatvec(x)
        m = torch.empty(self.ni, dtype=x.dtype, device=x.device)
        kernels.kirchhoff(x.reshape(self.ns, self.nr, self.nt), m,
                          *self._tables(x.device), True)
        return m


class LSMLocal:
    """pylops.waveeqprocessing.LSM's constructor: ``Demop`` is the
    KirchhoffLocal demigration operator, so that
    ``MPIVStack(ops=[lsm.Demop])`` ports line for line.  Further keywords
    (trav, dtype) go to KirchhoffLocal."""

    def __init__(self, z, x, t, srcs, recs, vel, wav, wavcenter, y=None,
                 mode: str = "analytic", **kwargs):
        self.y, self.x, self.z = y, x, z
        self.Demop = KirchhoffLocal(z, x, t, srcs, recs, vel, wav, wavcenter,
                                    y=y, mode=mode, **kwargs)
