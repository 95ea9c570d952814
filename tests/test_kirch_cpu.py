"""What pam_kirch and its layers promise without a GPU: the C entry point
refuses bad arguments before launching, the host-side queries, the launch
layer's check order on CPU tensors, the operators' validation, the
traveltime tables and the public names."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pylops_mpi_amd as pm
from pylops_mpi_amd import _ffi, kernels

EARG, EDTYPE = -1, -2
F64, F32, C128, C64 = _ffi.F64, _ffi.F32, _ffi.C128, _ffi.C64
ENV = ("PAM_KIRCH_WINDOW", "PAM_KIRCH_SPLIT", "PAM_KIRCH_STAGE")


@pytest.fixture(scope="module")
def lib():
    if not _ffi.available():
        pytest.skip("libpam.so not built (run __graft_entry__.build())")
    return _ffi.lib()


@pytest.fixture
def env():
    """env(NAME, value) sets one of the PAM_KIRCH_* selectors (None
    removes it); all are restored afterwards."""
    old = {k: os.environ.pop(k, None) for k in ENV}

    def set_(name, v):
        assert name in ENV
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(v)
    yield set_
    for k, v in old.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


# ------------------------------------------------------------------- C ABI
def test_abi_refuses_bad_arguments(lib, env):
    """Only argument sets that must be refused are passed, so nothing can
    launch; the pointers are placeholders that are never dereferenced."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    good = dict(adjoint=0, m=p, d=p + 64, qs=p + 256, qr=p + 320, ws=None,
                ns=1, nr=1, ni=2, nt=4, dtype=F64)

    def call(**kw):
        a = {**good, **kw}
        return lib.pam_kirch(None, a["adjoint"], a["m"], a["d"], a["qs"],
                             a["qr"], a["ws"], a["ns"], a["nr"], a["ni"],
                             a["nt"], a["dtype"])

    for adjoint in (0, 1):
        for name in ("ns", "nr", "ni"):
            for bad in (0, -3):
                assert call(adjoint=adjoint, **{name: bad}) == EARG
        for nt in (1, 0, -2):
            assert call(adjoint=adjoint, nt=nt) == EARG
        for name in ("m", "d", "qs", "qr"):
            assert call(adjoint=adjoint, **{name: None}) == EARG
        # m inside d, d inside m, the same pointer
        assert call(adjoint=adjoint, m=p + 64) == EARG
        assert call(adjoint=adjoint, m=p + 64 + 24) == EARG
        assert call(adjoint=adjoint, d=p + 8) == EARG
        for dtype in (C128, C64, 9, -1):
            assert call(adjoint=adjoint, dtype=dtype) == EDTYPE
        assert call(adjoint=adjoint, ni=0, dtype=C128) == EARG
    # a split adjoint needs its workspace
    env("PAM_KIRCH_SPLIT", 1)
    ntr = 2 * lib.pam_kirch_chunk(1000, 1, 2, 4, F64) + 1
    assert lib.pam_kirch_ws_elems(1, ntr, 1, 2, 4, F64) == 3 * 2
    big = (ctypes.c_double * (ntr * 4 + 8))()
    assert call(adjoint=1, ns=ntr, d=ctypes.addressof(big)) == EARG
    assert list(buf) == [0.0] * 64


def test_queries(lib, env):
    for fn in (lib.pam_kirch_chunk, lib.pam_kirch_variant,
               lib.pam_kirch_window):
        assert fn(2, 3, 10, 8, C128) == EDTYPE
        for bad in ((0, 3, 10, 8), (2, 0, 10, 8), (2, 3, 0, 8),
                    (2, 3, 10, 1)):
            assert fn(*bad, F64) == EARG
    assert lib.pam_kirch_ws_elems(0, 2, 3, 10, 1, F64) == EARG
    assert lib.pam_kirch_ws_elems(1, 2, 3, 10, 8, C64) == EDTYPE
    P = lib.pam_kirch_points()
    assert P > 0 and P % 64 == 0 and kernels.kirchhoff_points() == P
    for dt, size in ((F64, 8), (F32, 4)):
        # few traces: one chunk and no workspace
        assert lib.pam_kirch_chunk(2, 3, 10, 8, dt) == 6
        assert lib.pam_kirch_ws_elems(1, 2, 3, 10, 8, dt) == 0
        assert lib.pam_kirch_ws_elems(0, 2, 3, 10, 8, dt) == 0
        # many traces on few points: split into chunks of a fixed size
        c = lib.pam_kirch_chunk(100, 100, 10, 8, dt)
        assert 0 < c < 10000
        assert lib.pam_kirch_chunk(50, 7, 1000, 20, dt) == c
        assert lib.pam_kirch_ws_elems(1, 100, 100, 10, 8, dt) == \
            -(-10000 // c) * 10
        assert lib.pam_kirch_chunk(1, c, 10, 8, dt) == c        # one chunk
        assert lib.pam_kirch_ws_elems(1, 1, c, 10, 8, dt) == 0
        assert lib.pam_kirch_ws_elems(1, 1, c + 1, 10, 8, dt) == 20
        # points that fill the chip on their own: no split
        ni = 4096 * P
        assert lib.pam_kirch_chunk(100, 100, ni, 8, dt) == 10000
        assert lib.pam_kirch_ws_elems(1, 100, 100, ni, 8, dt) == 0
        env("PAM_KIRCH_SPLIT", 1)
        assert lib.pam_kirch_chunk(100, 100, ni, 8, dt) == c
        env("PAM_KIRCH_SPLIT", 0)
        assert lib.pam_kirch_chunk(100, 100, 10, 8, dt) == 10000
        assert lib.pam_kirch_ws_elems(1, 100, 100, 10, 8, dt) == 0
        env("PAM_KIRCH_SPLIT", None)
        # the window: the trace, or less; never beyond the LDS budget (the
        # window is kept in float64 for either dtype)
        wmax = 65536 // 8
        assert lib.pam_kirch_window(100, 100, 10, 651, dt) == 651
        w = lib.pam_kirch_window(2, 3, 10, 651, dt)
        assert 0 < w < 651
        assert lib.pam_kirch_window(2, 3, 10, 2, dt) == 2
        assert lib.pam_kirch_window(100, 100, 10, 10 * wmax, dt) == wmax
        for forced, nt, want in ((5, 651, 5), (5, 3, 3), (1, 651, 1),
                                 (wmax, 10 * wmax, wmax)):
            env("PAM_KIRCH_WINDOW", forced)
            assert lib.pam_kirch_window(100, 100, 10, nt, dt) == want
        for junk in ("0", "-4", "", str(wmax + 1)):
            env("PAM_KIRCH_WINDOW", junk)
            assert lib.pam_kirch_window(2, 3, 10, 651, dt) == w
        env("PAM_KIRCH_WINDOW", None)
        budget = 65536 // size
        # the adjoint's body: forced either way; staged needs the trace to
        # fit
        auto = lib.pam_kirch_variant(2, 3, 10, 651, dt)
        assert auto in (0, 1)
        for v in (0, 1):
            env("PAM_KIRCH_STAGE", v)
            assert lib.pam_kirch_variant(2, 3, 10, 651, dt) == v
            assert lib.pam_kirch_variant(2, 3, 10, budget, dt) == v
            assert lib.pam_kirch_variant(2, 3, 10, budget + 1, dt) == 0
        env("PAM_KIRCH_STAGE", 7)
        assert lib.pam_kirch_variant(2, 3, 10, 651, dt) == auto
        env("PAM_KIRCH_STAGE", None)


# ------------------------------------------------------------ launch layer
def _block(dtype=torch.float64):
    d = torch.full((2, 3, 8), -1.0, dtype=dtype)
    m = torch.full((5,), -1.0, dtype=dtype)
    qs = torch.ones((2, 5), dtype=dtype)
    qr = torch.ones((3, 5), dtype=dtype)
    return d, m, qs, qr


def test_launch_layer_checks_in_order(lib, env):
    d, m, qs, qr = _block()
    # dtypes first — even when the shapes are wrong too
    with pytest.raises(TypeError, match="pam_kirch"):
        kernels.kirchhoff(d.to(torch.complex128), m, qs, qr, False)
    with pytest.raises(TypeError, match="pam_kirch"):
        kernels.kirchhoff(d.to(torch.int32), m, qs, qr, True)
    for i in (1, 2, 3):
        args = [d, m, qs, qr]
        args[i] = args[i].to(torch.float32)[:1]
        with pytest.raises(TypeError, match="pam_kirch"):
            kernels.kirchhoff(*args, False)
    # then shapes
    with pytest.raises(ValueError):
        kernels.kirchhoff(d.view(-1), m, qs, qr, False)        # rank
    with pytest.raises(ValueError, match="pam_kirch"):
        kernels.kirchhoff(d, m, qs[:1], qr, False)
    with pytest.raises(ValueError, match="pam_kirch"):
        kernels.kirchhoff(d, m, qs, qr[:, :4], True)
    with pytest.raises(ValueError, match="pam_kirch.*nt >= 2"):
        kernels.kirchhoff(d[:, :, :1], m, qs, qr, True)
    # then the output's layout: never copied
    dt_ = torch.full((2, 8, 3), -1.0, dtype=torch.float64).transpose(1, 2)
    with pytest.raises(ValueError, match="pam_kirch.*contiguous"):
        kernels.kirchhoff(dt_, m, qs, qr, False)
    mt = torch.full((10,), -1.0, dtype=torch.float64)[::2]
    with pytest.raises(ValueError, match="pam_kirch.*contiguous"):
        kernels.kirchhoff(d, mt, qs, qr, True)
    # and the device last (a strided INPUT is fine)
    for args in ((d, m, qs, qr, False), (d, m, qs, qr, True),
                 (d, mt, qs, qr, False), (dt_, m, qs, qr, True)):
        with pytest.raises(RuntimeError, match="no CPU compute path"):
            kernels.kirchhoff(*args)
    assert torch.all(d == -1.0) and torch.all(m == -1.0)
    assert torch.all(dt_ == -1.0) and torch.all(mt == -1.0)
    # query wrappers: same checks, answers of the C queries
    assert kernels.kirchhoff_chunk(d, m, qs, qr) == 6
    assert kernels.kirchhoff_window(d, m, qs, qr) == 8
    env("PAM_KIRCH_WINDOW", 3)
    assert kernels.kirchhoff_window(d, m, qs, qr) == 3
    env("PAM_KIRCH_STAGE", 1)
    assert kernels.kirchhoff_variant(d, m, qs, qr) == kernels.KIRCH_STAGED
    env("PAM_KIRCH_STAGE", 0)
    assert kernels.kirchhoff_variant(d, m, qs, qr) == kernels.KIRCH_GATHER
    with pytest.raises(TypeError, match="pam_kirch"):
        kernels.kirchhoff_chunk(d.to(torch.complex64), m, qs, qr)


# --------------------------------------------------------------- operators
def test_public_names():
    for name in ("KirchhoffLocal", "LSMLocal", "traveltime_table"):
        assert hasattr(pm, name), name
    assert issubclass(pm.KirchhoffLocal, pm.LocalOperator)


def geometry(three_d=False):
    x, z = np.arange(5) * 4.0, np.arange(4) * 3.0
    y = np.arange(3) * 5.0 if three_d else None
    srcs = np.array([[2.0, 9.0, 15.0], [1.0, 1.0, 2.0]])
    recs = np.array([[0.0, 16.0], [0.5, 0.5]])
    if three_d:
        srcs = np.vstack([[1.0, 4.0, 9.0], srcs])
        recs = np.vstack([[2.0, 7.0], recs])
    return z, x, y, srcs, recs


@pytest.mark.parametrize("three_d", (False, True))
def test_traveltime_table(three_d):
    z, x, y, srcs, recs = geometry(three_d)
    vel = 1500.0
    ts, tr = pm.traveltime_table(z, x, srcs, recs, vel, y=y)
    ni = x.size * z.size * (y.size if three_d else 1)
    assert ts.shape == (ni, 3) and tr.shape == (ni, 2)
    assert ts.dtype == tr.dtype == np.float64
    for tab, pos in ((ts, srcs), (tr, recs)):
        for i in range(ni):
            if three_d:
                iy, ix, iz = np.unravel_index(i, (3, 5, 4))
                p = np.array([y[iy], x[ix], z[iz]])
            else:
                ix, iz = np.unravel_index(i, (5, 4))
                p = np.array([x[ix], z[iz]])
            want = np.sqrt(((p[:, None] - pos) ** 2).sum(axis=0)) / vel
            np.testing.assert_allclose(tab[i], want, rtol=1e-15, atol=0)
    with pytest.raises(ValueError, match="constant velocity"):
        pm.traveltime_table(z, x, srcs, recs, np.full((5, 4), vel), y=y)
    with pytest.raises(ValueError, match="srcs"):
        pm.traveltime_table(z, x, srcs[:1], recs, vel, y=y)


def test_kirchhoff_validation():
    z, x, _, srcs, recs = geometry()
    t = np.arange(40) * 0.004
    wav, _, wavc = pm.ricker(t[:5], f0=20)
    op = pm.KirchhoffLocal(z, x, t, srcs, recs, 1000.0, wav, wavc)
    assert op.shape == (3 * 2 * 40, 20) and op.dims == (5, 4)
    assert (op.ns, op.nr, op.ni, op.nt) == (3, 2, 20, 40)
    assert op.dtype == np.float64 and op.qs.dtype == torch.float64
    assert op.qs.shape == (3, 20) and op.qr.shape == (2, 20)
    assert op.qs.is_contiguous() and op.qr.is_contiguous()
    assert isinstance(op.conv, pm.Convolve1DLocal)
    assert op.conv.dims == (6, 40) and op.conv.offset == wavc
    # the tables: seconds / dt, transposed
    ts, tr = pm.traveltime_table(z, x, srcs, recs, 1000.0)
    assert np.array_equal(op.qs.numpy(), ts.T / 0.004)
    assert np.array_equal(op.qr.numpy(), tr.T / 0.004)
    # byot: arrays or tensors, same tables; float32 casts them once
    for trav in ((ts, tr), (torch.from_numpy(ts), torch.from_numpy(tr))):
        by = pm.KirchhoffLocal(z, x, t, srcs, recs, mode="byot", trav=trav,
                               dtype="float32")
        assert by.conv is None and by.dtype == np.float32
        assert torch.equal(by.qs, op.qs.to(torch.float32))
        assert torch.equal(by.qr, op.qr.to(torch.float32))
    op3 = pm.KirchhoffLocal(*geometry(True)[:2], t, *geometry(True)[3:],
                            vel=2000.0, y=geometry(True)[2])
    assert op3.dims == (3, 5, 4) and op3.shape == (240, 60)
    lsm = pm.LSMLocal(z, x, t, srcs, recs, 1000.0, wav, wavc)
    assert isinstance(lsm.Demop, pm.KirchhoffLocal)
    assert lsm.Demop.shape == op.shape
    assert torch.equal(lsm.Demop.qs, op.qs)

    for kw, word in ((dict(mode="eikonal"), "eikonal solver"),
                     (dict(dynamic=True), "amplitude"),
                     (dict(wavfilter=True), "filter")):
        with pytest.raises(NotImplementedError, match=word):
            pm.KirchhoffLocal(z, x, t, srcs, recs, 1000.0, wav, wavc, **kw)
    with pytest.raises(NotImplementedError, match="byot"):
        pm.LSMLocal(z, x, t, srcs, recs, 1000.0, wav, wavc, mode="eikonal")
    with pytest.raises(ValueError, match="mode"):
        pm.KirchhoffLocal(z, x, t, srcs, recs, 1000.0, mode="ray")
    with pytest.raises(ValueError, match="vel"):
        pm.KirchhoffLocal(z, x, t, srcs, recs)
    with pytest.raises(ValueError, match="byot"):
        pm.KirchhoffLocal(z, x, t, srcs, recs, mode="byot")
    with pytest.raises(ValueError, match="trav_srcs"):
        pm.KirchhoffLocal(z, x, t, srcs, recs, mode="byot",
                          trav=(ts[:-1], tr))
    with pytest.raises(ValueError, match="trav_recs"):
        pm.KirchhoffLocal(z, x, t, srcs, recs, mode="byot",
                          trav=(ts, tr.ravel()))
    with pytest.raises(ValueError, match="t needs"):
        pm.KirchhoffLocal(z, x, t[:1], srcs, recs, 1000.0)
    with pytest.raises(TypeError, match="real"):
        pm.KirchhoffLocal(z, x, t, srcs, recs, 1000.0, dtype="complex128")
    # no CPU compute path: the apply fails loudly, never falls back
    with pytest.raises(RuntimeError, match="no CPU compute path"):
        op.matvec(torch.zeros(20, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU compute path"):
        op.rmatvec(torch.zeros(240, dtype=torch.float64))
