"""pam_kirch kernel by kernel against the NumPy loops of tests/kirchref.py
(themselves checked in tests/test_kirchref_cpu.py), then the operators.

Every operand sits in a larger, sentinel-filled device buffer
(primref.Placed), 16-byte aligned or one element off it; after a launch
the guards must hold the sentinel and the inputs their uploaded bits.

Adjoint (gather): equal to gather_ref bit for bit (primref.same: +-0
equal) for both bodies (samples from global memory / trace staged in LDS)
and with the traces split into chunks or not, the chunk read from the
query.  Forward (spread): LDS float adds make the order of a sample's sum
depend on the schedule, so
    |got - spread_ref| <= (n + 2) * eps_T * spread_ref(|m|)   per sample,
n the sample's contribution count and spread_ref(|m|) in float64 — the
bound of a sum of n rounded products in any order — and samples without a
contribution are exactly 0.

Shapes: ni in {1, 63, 64, 65, P-1, P, P+1, 2P+3}, P the points of one
workgroup; nt in {2, 3, 64, 65}, W-1, W, W+1, 2W+1 around a forced window
W and one trace longer than the LDS budget; (ns, nr) in {(1,1), (1,3),
(2,2), (3,1)} and trace counts C-1, C, C+1, 2C, 2C+1 around the chunk C."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import convref as cr
import kirchref as kr
import primref as pr
from primref import Placed
import pylops_mpi_amd as pm
from pylops_mpi_amd import kernels

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"f64": np.float64, "f32": np.float32}
TORCH = {"f64": torch.float64, "f32": torch.float32}
ENV = ("PAM_KIRCH_WINDOW", "PAM_KIRCH_SPLIT", "PAM_KIRCH_STAGE")
KINDS = ("random", "collide", "own", "skip")
ALIGNS = ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0),
          (0, 0, 0, 1), (1, 1, 1, 1))        # d, m, qs, qr
SMALL_TR = ((1, 1), (1, 3), (2, 2), (3, 1))
NTS = (2, 3, 64, 65)


@pytest.fixture(scope="module", autouse=True)
def _init():
    from pylops_mpi_amd.comm import init_default_comm
    init_default_comm(torch.device("cuda:0"))


@pytest.fixture
def force():
    """force(window=, split=, stage=) selects the launch plan for the calls
    that follow (None: automatic); the environment is restored afterwards."""
    old = {k: os.environ.pop(k, None) for k in ENV}

    def set_(window=None, split=None, stage=None):
        for k, v in zip(ENV, (window, split, stage)):
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
    yield set_
    for k, v in old.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def fixed_chunk():
    """The chunk C of a split gather: 1000 traces on one point, with the
    split forced on for the length of the query."""
    d = torch.empty((1000, 1, 2), dtype=torch.float64, device="meta")
    m = torch.empty((1,), dtype=torch.float64, device="meta")
    q = torch.empty((1000, 1), dtype=torch.float64, device="meta")
    old = os.environ.get("PAM_KIRCH_SPLIT")
    os.environ["PAM_KIRCH_SPLIT"] = "1"
    try:
        return kernels.kirchhoff_chunk(d, m, q, q[:1])
    finally:
        if old is None:
            os.environ.pop("PAM_KIRCH_SPLIT")
        else:
            os.environ["PAM_KIRCH_SPLIT"] = old


def ni_values():
    P = kernels.kirchhoff_points()
    return (1, 63, 64, 65, P - 1, P, P + 1, 2 * P + 3)


def tables(kind, ns, nr, ni, nt, dtype, seed, edges=()):
    """qs (ns, ni), qr (nr, ni) in samples.
    random: sums spread over [-2, nt + 2);
    collide: every pair of every trace on one sample pair;
    own: image point i on sample i mod (nt - 1), shifted per trace;
    skip: random with q = -0.5, nt - 1, one ulp below nt - 1, an exact
      integer, NaN and +inf planted at the first points of every trace.
    ``edges``: window starts t0; a pair with it = t0 - 1, it + 1 = t0 is
    planted for each (it straddles the window edge)."""
    T = dtype
    rng = np.random.default_rng([seed, ns, nr, ni, nt])
    if kind == "collide":
        qs = np.full((ns, ni), (nt - 2) // 2, dtype=T)
        qr = np.full((nr, ni), 0.25, dtype=T)
    elif kind == "own":
        qs = np.tile((np.arange(ni) % (nt - 1)).astype(T), (ns, 1))
        qr = np.full((nr, ni), 0.5, dtype=T)
        if nt > 2:
            qs = (qs + np.arange(ns)[:, None].astype(T)) % T(nt - 1)
    else:
        qs = rng.uniform(-1.0, (nt + 2) / 2.0, (ns, ni)).astype(T)
        qr = rng.uniform(-1.0, (nt + 2) / 2.0, (nr, ni)).astype(T)
    planted = []
    if kind == "skip":
        planted += [T(-0.5), T(nt - 1), np.nextafter(T(nt - 1), T(0)),
                    T(min(1, nt - 2)), T(np.nan), T(np.inf)]
    planted += [T(t0 - 0.5) for t0 in edges if 1 <= t0 < nt]
    for j, q in enumerate(planted[:ni]):
        i = (j * 7) % ni if ni > 7 * len(planted) else j
        qs[:, i] = q
        qr[:, i] = 0
    return qs, qr


def model(n, dtype, seed):
    rng = np.random.default_rng([seed, n])
    x = rng.standard_normal(n).astype(dtype)
    if n >= 16:
        x[(np.arange(4) * 37 + seed) % n] = [0.0, -0.0, 0.0, -0.0]
    return x


def launch(adjoint, dval, mval, qs, qr, align):
    """One guarded launch -> the output's value; asserts guards and
    inputs.  The output operand is uploaded as sentinels."""
    ns, nr, nt = dval.shape
    ni = mval.size
    if adjoint:
        mval = np.full(ni, pr.SENTINEL, dtype=mval.dtype)
    else:
        dval = np.full(dval.shape, pr.SENTINEL, dtype=dval.dtype)
    pd, pmod = Placed(dval, align[0]), Placed(mval, align[1])
    pqs, pqr = Placed(qs, align[2]), Placed(qr, align[3])
    kernels.kirchhoff(pd.tensor.view(ns, nr, nt), pmod.tensor,
                      pqs.tensor.view(ns, ni), pqr.tensor.view(nr, ni),
                      adjoint)
    out, inp = (pmod, pd) if adjoint else (pd, pmod)
    full = out.fetch()
    assert out.guards_intact(full), "guard overwritten"
    assert inp.untouched() and pqs.untouched() and pqr.untouched(), \
        "input changed"
    return out.value(full)


def diff(got, want):
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    return (f"{bad.size} of {got.size} differ, first at {bad[:4]}: got "
            f"{got[bad[:4]]}, want {want[bad[:4]]}")


# ---------------------------------------------------------------- adjoint
def check_gather(force, dname, ns, nr, ni, nt, kind, align, seed, split,
                 stage, expect_stage=None):
    T = DT[dname]
    qs, qr = tables(kind, ns, nr, ni, nt, T, seed)
    d = model(ns * nr * nt, T, seed + 1).reshape(ns, nr, nt)
    force(split=split, stage=stage)
    meta = [torch.empty(s, dtype=TORCH[dname], device="meta")
            for s in ((ns, nr, nt), (ni,), (ns, ni), (nr, ni))]
    chunk = kernels.kirchhoff_chunk(*meta)
    C = fixed_chunk()
    if split == 1:
        assert chunk == (C if ns * nr > C else ns * nr)
    elif split == 0:
        assert chunk == ns * nr
    assert chunk in (C, ns * nr)
    if stage is not None:
        want_stage = stage if expect_stage is None else expect_stage
        assert kernels.kirchhoff_variant(*meta) == want_stage
    got = launch(True, d, np.zeros(ni, dtype=T), qs, qr, align)
    want = kr.gather_ref(d, qs, qr, chunk)
    msg = (f"{dname} ns={ns} nr={nr} ni={ni} nt={nt} {kind} align={align} "
           f"split={split} stage={stage} chunk={chunk}")
    assert pr.same(got, want), f"{msg}: {diff(got, want)}"


@pytest.mark.parametrize("dname", list(DT))
def test_gather_matches_reference_bit_for_bit(force, dname):
    """Every (ni, nt, traces) on an edge, the table kinds, alignments and
    the two bodies rotating; a handful of traces is one chunk whatever the
    plan says."""
    for n, (ni, nt, (ns, nr)) in enumerate(itertools.product(
            ni_values(), NTS, SMALL_TR)):
        check_gather(force, dname, ns, nr, ni, nt, KINDS[n % 4],
                     ALIGNS[n % 6], n % 3, (None, 0, 1)[n % 3], n % 2)


@pytest.mark.parametrize("dname", list(DT))
def test_gather_with_every_split_of_the_launch_plan(force, dname):
    """Trace counts around the chunk C: the automatic plan, and both
    bodies with the traces split and unsplit."""
    C, P = fixed_chunk(), kernels.kirchhoff_points()
    traces = ((1, C - 1), (C, 1), (1, C + 1), (2, C), (2 * C + 1, 1))
    plans = ((None, None), (0, 0), (0, 1), (1, 0), (1, 1))
    for n, ((ns, nr), ni, nt) in enumerate(itertools.product(
            traces, (1, 65, P + 1), (3, 65))):
        for split, stage in plans:
            check_gather(force, dname, ns, nr, ni, nt, KINDS[n % 4],
                         ALIGNS[n % 6], n % 3, split, stage)


@pytest.mark.parametrize("dname", list(DT))
def test_gather_of_a_trace_beyond_the_lds_budget(force, dname):
    """Staging is refused (the query says so) and the result is right."""
    nt = 65536 // np.dtype(DT[dname]).itemsize + 1
    check_gather(force, dname, 1, 2, 65, nt, "random", ALIGNS[0], 0, None,
                 1, expect_stage=0)
    check_gather(force, dname, 1, 2, 65, nt - 1, "skip", ALIGNS[5], 1, None,
                 1, expect_stage=1)


# ---------------------------------------------------------------- forward
def check_spread(force, dname, ns, nr, ni, nt, kind, align, seed,
                 window=None, straddle=False):
    T = DT[dname]
    force(window=window)
    meta = [torch.empty(s, dtype=TORCH[dname], device="meta")
            for s in ((ns, nr, nt), (ni,), (ns, ni), (nr, ni))]
    W = kernels.kirchhoff_window(*meta)
    if window is not None:
        assert W == min(window, nt)
    edges = range(W, nt, W) if straddle else ()
    qs, qr = tables(kind, ns, nr, ni, nt, T, seed, edges)
    m = model(ni, T, seed + 2)
    got = launch(False, np.zeros((ns, nr, nt), dtype=T), m, qs, qr,
                 align).reshape(ns, nr, nt)
    want = kr.spread_ref(m, qs, qr, nt)
    bound = kr.spread_bound(m, qs, qr, nt)
    count = kr.spread_count(qs, qr, nt)
    msg = (f"{dname} ns={ns} nr={nr} ni={ni} nt={nt} {kind} align={align} "
           f"W={W}")
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    worst = np.max(err - bound)
    print(f"{msg}: max err {err.max():.3e}, max (err - bound) {worst:.3e}, "
          f"max count {count.max()}")
    assert np.all(err <= bound), f"{msg}: {np.argwhere(err > bound)[:4]}"
    assert np.all(got[count == 0] == 0), f"{msg}: untouched sample not 0"
    return got


@pytest.mark.parametrize("dname", list(DT))
def test_spread_within_the_rounding_bound(force, dname):
    for n, (ni, nt, (ns, nr)) in enumerate(itertools.product(
            ni_values(), NTS, SMALL_TR)):
        check_spread(force, dname, ns, nr, ni, nt, KINDS[n % 4],
                     ALIGNS[n % 6], n % 3)


@pytest.mark.parametrize("dname", list(DT))
@pytest.mark.parametrize("W", (1, 5, 16))
def test_spread_in_forced_windows(force, dname, W):
    """nt on either side of the window and past two windows; a pair that
    straddles every window edge is planted."""
    P = kernels.kirchhoff_points()
    nts = sorted({W - 1, W, W + 1, 2 * W + 1} - {0, 1})
    for n, (nt, ni, (ns, nr)) in enumerate(itertools.product(
            nts, (1, 65, P + 1), ((1, 1), (2, 2)))):
        check_spread(force, dname, ns, nr, ni, nt, KINDS[n % 4],
                     ALIGNS[n % 6], n % 3, window=W, straddle=True)


@pytest.mark.parametrize("dname", list(DT))
def test_spread_of_a_trace_beyond_the_lds_budget(force, dname):
    """Windows of the budget's size — what the automatic plan gives a
    long trace when there are traces enough to fill the chip
    (tests/test_kirch_cpu.py), forced here on two traces — and a window
    one sample beyond it, which is refused: the automatic, shorter one."""
    budget = 65536 // 8         # the window is float64 for either dtype
    check_spread(force, dname, 1, 2, 300, budget + 5, "random", ALIGNS[0],
                 0, window=budget, straddle=True)
    force(window=budget + 1)
    meta = [torch.empty(s, dtype=TORCH[dname], device="meta")
            for s in ((1, 2, budget + 5), (300,), (1, 300), (2, 300))]
    assert kernels.kirchhoff_window(*meta) < budget


@pytest.mark.parametrize("dname", list(DT))
def test_spread_of_a_maximum_collision_twice(force, dname):
    """Every point of 2 x 3 traces on one sample pair, run twice; whether
    the two runs agree bit for bit is printed, not asserted
    (profiles/kirchhoff.log records what a run showed)."""
    runs = [check_spread(force, dname, 2, 3, 4099, 64, "collide", ALIGNS[0],
                         3) for _ in range(2)]
    print(f"collision spread {dname} run twice: bits "
          f"{'identical' if pr.same(runs[0], runs[1]) else 'DIFFER'}")


# --------------------------------------------------------------- operators
def dev(a):
    return torch.as_tensor(a, device="cuda:0")


def small_operator(dtype="float64", wavelet=True):
    """11 x 9 model, 2 x 3 traces, nt = 40: events between samples 8 and
    32 at 1000 m/s, dt = 4 ms."""
    x, z = np.arange(11) * 4.0, 8.0 + np.arange(9) * 4.0
    t = np.arange(40) * 0.004
    srcs = np.array([[6.0, 30.0], [2.0, 2.0]])
    recs = np.array([[4.0, 20.0, 36.0], [3.0, 3.0, 3.0]])
    wav, _, wavc = pm.ricker(t[:4], f0=40)
    if not wavelet:
        wav = None
    return pm.KirchhoffLocal(z, x, t, srcs, recs, 1000.0, wav, wavc,
                             dtype=dtype)


@pytest.mark.parametrize("dname", list(DT))
def test_operator_against_the_reference(force, dname):
    """KirchhoffLocal (analytic, with a wavelet).  Forward: conv1d_ref o
    spread_ref; the convolution is linear, so a spread within B of its
    reference gives a convolved trace within conv(|h|, B) of it, plus the
    two convolutions' own rounding, nh * eps * conv(|h|, spread_ref(|m|))
    (nh rounded products and sums each, on inputs that differ in the last
    bits).  Adjoint: conv1d and the gather are both pinned, so gather_ref
    o conv1d_ref bit for bit."""
    force()
    T = DT[dname]
    op = small_operator(np.dtype(T).name)
    qs, qr = op.qs.numpy().copy(), op.qr.numpy().copy()
    assert qs.dtype == T
    h = op.conv.h.numpy().copy()
    rng = np.random.default_rng(5)
    m = rng.standard_normal(op.ni).astype(T)
    ntr, nt = op.ns * op.nr, op.nt
    got = op.matvec(dev(m)).cpu().numpy().reshape(1, ntr, nt)
    s = kr.spread_ref(m, qs, qr, nt).reshape(ntr, nt, 1)
    want = cr.conv1d_ref(s, h, op.conv.offset, False).reshape(1, ntr, nt)
    habs = np.abs(h).astype(np.float64)
    B = kr.spread_bound(m, qs, qr, nt).reshape(ntr, nt, 1)
    S = kr.spread_ref(np.abs(m), qs, qr, nt,
                      acc=np.float64).reshape(ntr, nt, 1)
    eps = float(np.finfo(T).eps)
    bound = (cr.conv1d_ref(B, habs, op.conv.offset, False)
             + h.size * eps * cr.conv1d_ref(S, habs, op.conv.offset, False))
    err = np.abs(got.astype(np.float64).ravel()
                 - want.astype(np.float64).ravel())
    print(f"{dname}: max err {err.max():.3e}, max bound {bound.max():.3e}")
    assert np.count_nonzero(want) > want.size // 4
    assert np.all(err <= bound.ravel())

    d = rng.standard_normal((op.ns, op.nr, nt)).astype(T)
    gotm = op.rmatvec(dev(d.ravel())).cpu().numpy()
    ct = cr.conv1d_ref(d.reshape(ntr, nt, 1), h, op.conv.offset,
                       True).reshape(op.ns, op.nr, nt)
    wantm = kr.gather_ref(ct, qs, qr)       # 6 traces: one chunk
    assert pr.same(gotm, wantm), diff(gotm, wantm)
    assert np.count_nonzero(wantm) == wantm.size
    assert op.qs.is_cuda                    # the tables moved once

    bare = small_operator(np.dtype(T).name, wavelet=False)
    gotb = bare.matvec(dev(m)).cpu().numpy().reshape(op.ns, op.nr, nt)
    assert np.all(np.abs(gotb.astype(np.float64) - s.reshape(gotb.shape))
                  <= B.reshape(gotb.shape))
    assert pr.same(bare.rmatvec(dev(d.ravel())).cpu().numpy(),
                   kr.gather_ref(d, qs, qr))


def test_dottest_through_vstack(force):
    force()
    rng = np.random.default_rng(6)
    for wavelet in (True, False):
        op = small_operator(wavelet=wavelet)
        Op = pm.MPIVStack(ops=[op])
        assert Op.shape == op.shape
        u = pm.DistributedArray.to_dist(
            dev(rng.standard_normal(op.shape[1])),
            partition=pm.Partition.BROADCAST)
        v = pm.DistributedArray.to_dist(dev(rng.standard_normal(op.shape[0])))
        assert pm.dottest(Op, u, v, rtol=1e-10)


def test_cgls_lowers_the_cost_monotonically(force):
    force()
    op = small_operator()
    Op = pm.MPIVStack(ops=[op])
    refl = np.zeros((11, 9))
    refl[:, 3], refl[:, 6] = -1.0, 0.5
    m = pm.DistributedArray.to_dist(dev(refl.ravel()),
                                    partition=pm.Partition.BROADCAST)
    d = Op @ m
    x0 = pm.DistributedArray(Op.shape[1], partition=pm.Partition.BROADCAST)
    x0[:] = 0
    cost = np.asarray(pm.cgls(Op, d, x0=x0, niter=10, tol=0.0)[5])
    assert cost.size == 11 and cost[0] > 0
    assert np.all(np.diff(cost) <= 0), cost
    assert cost[-1] < cost[0]


def test_example_runs_at_a_reduced_size():
    env = {k: v for k, v in os.environ.items() if k not in ENV}
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "examples", "lsm.py"), "--nx",
         "21", "--nz", "16", "--nr", "3", "--ns", "2", "--nt", "80",
         "--ntwav", "5", "--niter", "5"],
        capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cgls x5" in out.stdout and "9-tap ricker" in out.stdout
