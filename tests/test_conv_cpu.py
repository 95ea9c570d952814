"""What pam_conv1d and its layers promise without a GPU: the C entry
point refuses bad arguments before launching, the host-side variant and
tile queries, the launch layer's check order on CPU tensors, the
operators' validation and public names, and the Ricker wavelet."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pylops_mpi_amd as pm
from pylops_mpi_amd import _ffi, kernels

EARG, EDTYPE, EOP = -1, -2, -3
F64, F32, C128 = _ffi.F64, _ffi.F32, _ffi.C128


@pytest.fixture(scope="module")
def lib():
    if not _ffi.available():
        pytest.skip("libpam.so not built (run __graft_entry__.build())")
    return _ffi.lib()


@pytest.fixture
def variant_env():
    old = os.environ.pop("PAM_CONV_VARIANT", None)
    yield lambda v: (os.environ.__setitem__("PAM_CONV_VARIANT", str(v))
                     if v is not None
                     else os.environ.pop("PAM_CONV_VARIANT", None))
    os.environ.pop("PAM_CONV_VARIANT", None)
    if old is not None:
        os.environ["PAM_CONV_VARIANT"] = old


# ------------------------------------------------------------------- C ABI
def test_abi_refuses_bad_arguments(lib):
    """Only argument sets that must be refused are passed, so nothing can
    launch; the pointers are placeholders that are never dereferenced."""
    buf = (ctypes.c_double * 4)()
    p = ctypes.addressof(buf)
    good = dict(adjoint=0, x=p, y=p + 8, h=p + 16, batch=1, d=2, m=1, nh=2,
                offset=0, deriv=0, dtype=F64)

    def call(**kw):
        a = {**good, **kw}
        return lib.pam_conv1d(None, a["adjoint"], a["x"], a["y"], a["h"],
                              a["batch"], a["d"], a["m"], a["nh"],
                              a["offset"], a["deriv"], a["dtype"])

    for name in ("batch", "d", "m", "nh"):
        for bad in (0, -3):
            assert call(**{name: bad}) == EARG, (name, bad)
    for off in (-1, 2, 7):
        assert call(offset=off) == EARG, off
    for name in ("x", "y", "h"):
        assert call(**{name: None}) == EARG, name
    for deriv in (-1, 3):
        assert call(deriv=deriv) == EOP, deriv
    for dtype in (C128, 3, 9, -1):
        assert call(dtype=dtype) == EDTYPE, dtype
    # the documented precedence: argument, then op, then dtype
    assert call(d=0, deriv=5, dtype=9) == EARG
    assert call(deriv=5, dtype=9) == EOP
    assert list(buf) == [0.0] * 4


def test_queries_refuse_bad_arguments(lib):
    assert lib.pam_conv1d_variant(C128, 8, 8, 3) == EDTYPE
    for d, m, nh in ((0, 8, 3), (8, 0, 3), (8, 8, 0)):
        assert lib.pam_conv1d_variant(F64, d, m, nh) == EARG
    assert lib.pam_conv1d_tile_d(2, C128, 3) == EDTYPE
    assert lib.pam_conv1d_tile_d(2, F64, 0) == EARG
    assert lib.pam_conv1d_tile_m(2, 7) == EDTYPE


@pytest.mark.parametrize("dt", (F64, F32))
def test_variant_query_honours_the_environment(lib, variant_env, dt):
    d, m, nh = 300, 100, 41
    for v in (0, 1, 2):
        variant_env(v)
        assert lib.pam_conv1d_variant(dt, d, m, nh) == v
        assert lib.pam_conv1d_variant(dt, d, 1, nh) == v
    # re-read on every call: no restart, no cache
    variant_env(2)
    assert lib.pam_conv1d_variant(dt, d, m, nh) == 2
    variant_env(0)
    assert lib.pam_conv1d_variant(dt, d, m, nh) == 0
    # anything else selects nothing: the automatic choice, a valid code
    variant_env(None)
    auto = lib.pam_conv1d_variant(dt, d, m, nh)
    assert auto in (0, 1, 2)
    for junk in ("7", "-2", ""):
        variant_env(junk)
        assert lib.pam_conv1d_variant(dt, d, m, nh) == auto


@pytest.mark.parametrize("dt", (F64, F32))
def test_variant_query_reports_the_lds_fallback(lib, variant_env, dt):
    """The trace kernel stages (nh + 1) * m samples of halo, the column
    kernel nh + 1 rows of tile_m: past 64 KiB of LDS both report 0."""
    size = 8 if dt == F64 else 4
    variant_env(1)
    assert lib.pam_conv1d_variant(dt, 64, 8, 41) == 1
    assert lib.pam_conv1d_variant(dt, 64, 65536 // size, 41) == 0
    assert lib.pam_conv1d_variant(dt, 64, 64, 65536 // size) == 0
    assert lib.pam_conv1d_variant(dt, 64, 2000, 41) == 0     # 84000 samples
    variant_env(2)
    assert lib.pam_conv1d_variant(dt, 64, 2000, 41) == 2     # m is tiled
    assert lib.pam_conv1d_variant(dt, 64, 2000, 65536 // size) == 0
    assert lib.pam_conv1d_tile_d(2, dt, 65536 // size) == 0
    # the automatic choice never lands on a kernel that does not fit
    variant_env(None)
    assert lib.pam_conv1d_variant(dt, 64, 2000, 65536 // size) == 0
    # the tiled kernels index one batch in 32 bits
    variant_env(2)
    assert lib.pam_conv1d_variant(dt, 1 << 20, 1 << 12, 3) == 0
    variant_env(1)
    assert lib.pam_conv1d_variant(dt, 1 << 31, 1, 3) == 0


@pytest.mark.parametrize("dt", (F64, F32))
def test_tile_queries(lib, dt):
    for nh in (1, 3, 41):
        assert lib.pam_conv1d_tile_d(0, dt, nh) == 0
        assert lib.pam_conv1d_tile_m(0, dt) == 0
        for v in (1, 2):
            assert lib.pam_conv1d_tile_d(v, dt, nh) > 0
            assert lib.pam_conv1d_tile_m(v, dt) > 0
    size = 8 if dt == F64 else 4
    for nh in (1, 41, 200):
        td, tm = kernels.conv1d_tile(
            2, torch.float64 if dt == F64 else torch.float32, nh)
        assert td == 0 or (td + nh + 1) * tm * size <= 65536
        assert (td == 0) == (nh == 200 and dt == F64)
    assert kernels.conv1d_tile(0, torch.float32, 5) == (0, 0)
    assert kernels.conv1d_tile(2, torch.complex64, 5) == \
        kernels.conv1d_tile(2, torch.float32, 5)


# ------------------------------------------------------------ launch layer
def _block(dtype=torch.float64):
    x = torch.arange(24, dtype=dtype).reshape(2, 4, 3)
    y = torch.full((2, 4, 3), -1.0, dtype=dtype)
    h = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    return y, x, h


def test_launch_layer_checks_in_order():
    y, x, h = _block()
    # dtypes first — even when the shapes are wrong too
    with pytest.raises(TypeError, match="pam_conv1d.*complex taps"):
        kernels.conv1d(y, x, h.to(torch.complex128), False, 0)
    with pytest.raises(TypeError, match="pam_conv1d"):
        kernels.conv1d(y, x.to(torch.float32)[:1], h, False, 9)
    with pytest.raises(TypeError, match="pam_conv1d"):
        kernels.conv1d(y, x, h.to(torch.float32), False, 0)
    yc = torch.full((2, 4, 3), -1.0, dtype=torch.complex64)
    with pytest.raises(TypeError, match="pam_conv1d"):     # wants float32
        kernels.conv1d(yc, yc.clone(), h, False, 0)
    # then shapes and scalars
    with pytest.raises(ValueError, match="pam_conv1d"):
        kernels.conv1d(y, x[:1], h, False, 0)
    with pytest.raises(ValueError):
        kernels.conv1d(y.view(-1), x.view(-1), h, False, 0)   # rank
    with pytest.raises(ValueError, match="1-D"):
        kernels.conv1d(y, x, h.reshape(1, 3), False, 0)
    for off in (-1, 3):
        with pytest.raises(ValueError, match="offset"):
            kernels.conv1d(y, x, h, False, off)
    for deriv in (-1, 3):
        with pytest.raises(ValueError, match="deriv"):
            kernels.conv1d(y, x, h, True, 0, deriv)
    # then the output's layout: never copied
    yt = torch.full((2, 3, 4), -1.0, dtype=torch.float64).transpose(1, 2)
    with pytest.raises(ValueError, match="pam_conv1d.*contiguous"):
        kernels.conv1d(yt, x, h, False, 0)
    assert torch.all(yt == -1.0)
    # and the device last
    for args in ((y, x, h, False, 1), (y, x, h, True, 2, 1),
                 (y, x.transpose(1, 2).reshape(2, 4, 3), h, False, 0, 2),
                 (yc, yc.clone(), h.to(torch.float32), True, 0)):
        with pytest.raises(RuntimeError, match="no CPU compute path"):
            kernels.conv1d(*args)
    assert torch.all(y == -1.0) and torch.all(yc == -1.0)


def test_variant_wrapper(lib, variant_env):
    _, x, _ = _block()
    variant_env(1)
    assert kernels.conv1d_variant(x, 3) == kernels.CONV_TRACE == 1
    variant_env(2)
    assert kernels.conv1d_variant(x, 3) == kernels.CONV_COLUMN == 2
    variant_env(0)
    assert kernels.conv1d_variant(x.to(torch.complex64), 3) == \
        kernels.CONV_PLAIN == 0


# --------------------------------------------------------------- operators
def test_public_names():
    for name in ("Convolve1DLocal", "PoststackLinearModellingLocal",
                 "ricker", "wavelets"):
        assert hasattr(pm, name), name
    assert pm.wavelets.ricker is pm.ricker
    assert issubclass(pm.Convolve1DLocal, pm.LocalOperator)
    assert issubclass(pm.PoststackLinearModellingLocal, pm.LocalOperator)


def test_convolve1d_validation():
    h = np.arange(1.0, 6.0)
    op = pm.Convolve1DLocal((4, 7, 3), h, offset=2, axis=1)
    assert op.shape == (84, 84) and (op.batch, op.d, op.m) == (4, 7, 3)
    assert op.dtype == np.float64 and op.h.dtype == torch.float64
    op = pm.Convolve1DLocal(9, torch.ones(2), offset=1, dtype="float32")
    assert (op.batch, op.d, op.m) == (1, 9, 1) and op.h.dtype == torch.float32
    op = pm.Convolve1DLocal((5, 6), h, axis=-1, dtype="complex64")
    assert op.h.dtype == torch.float32 and (op.batch, op.d, op.m) == (5, 6, 1)
    with pytest.raises(ValueError, match="1-D"):
        pm.Convolve1DLocal((4, 7), np.ones((2, 3)))
    for off in (-1, 5):
        with pytest.raises(ValueError, match="offset"):
            pm.Convolve1DLocal((4, 7), h, offset=off)
    for axis in (2, -3):
        with pytest.raises(ValueError, match="axis"):
            pm.Convolve1DLocal((4, 7), h, axis=axis)
    with pytest.raises(TypeError):
        pm.Convolve1DLocal((4, 7), h.astype(np.complex128))
    # no CPU compute path: the apply fails loudly, never falls back
    op = pm.Convolve1DLocal((4, 7), h, offset=2)
    with pytest.raises(RuntimeError, match="no CPU compute path"):
        op.matvec(torch.zeros(28, dtype=torch.float64))


def test_poststack_validation():
    wav = np.arange(1.0, 8.0)
    op = pm.PoststackLinearModellingLocal(wav, 30, spatdims=(5, 4))
    assert op.dims == (30, 5, 4) and (op.batch, op.d, op.m) == (1, 30, 20)
    assert op.offset == 3 and op.kind == "centered" and op.fused
    op = pm.PoststackLinearModellingLocal(wav, 30, spatdims=(5, 4), axis=-1,
                                          kind="forward", fused=False)
    assert op.dims == (5, 4, 30) and (op.batch, op.d, op.m) == (20, 30, 1)
    op = pm.PoststackLinearModellingLocal(wav, 30, spatdims=(5, 4), axis=1)
    assert op.dims == (5, 30, 4) and (op.batch, op.d, op.m) == (5, 30, 4)
    op = pm.PoststackLinearModellingLocal(wav[:6], 30, dtype="float32")
    assert op.dims == (30,) and op.offset == 3 and op.shape == (30, 30)
    assert pm.PoststackLinearModellingLocal(wav, 30, 8).dims == (30, 8)
    with pytest.raises(NotImplementedError, match="DenseLocal"):
        pm.PoststackLinearModellingLocal(wav, 30, explicit=True)
    with pytest.raises(NotImplementedError, match="DenseLocal"):
        pm.PoststackLinearModellingLocal(np.ones((30, 7)), 30)
    with pytest.raises(NotImplementedError, match="kind"):
        pm.PoststackLinearModellingLocal(wav, 30, kind="backward")
    with pytest.raises(ValueError, match="axis"):
        pm.PoststackLinearModellingLocal(wav, 30, spatdims=(5,), axis=2)


# ------------------------------------------------------------------ ricker
def test_ricker():
    t = np.arange(21) * 0.004
    w, tf, c = pm.ricker(t, f0=20)
    assert w.shape == tf.shape == (41,) and c == 20
    assert w[c] == 1.0 and np.all(np.abs(np.delete(w, c)) < 1.0)
    assert np.array_equal(w, w[::-1]) and np.array_equal(tf, -tf[::-1])
    assert np.array_equal(tf[c:], t)
    a = (np.pi * 20 * tf) ** 2
    np.testing.assert_allclose(w, (1 - 2 * a) * np.exp(-a), rtol=1e-15)
    w1, t1, c1 = pm.ricker(np.zeros(1))
    assert w1.tolist() == [1.0] and c1 == 0
    assert pm.ricker(t)[0].shape == (41,)        # f0 defaults to 10
