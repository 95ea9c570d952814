"""The stencil family kernel by kernel — pam_fd_apply's row-parallel, band
and rolling kernels, pam_fd_serial and pam_nsconv — against the NumPy
restatement of tests/stencilref.py, every comparison bit for bit.

Operands.  Every operand is a primref.Placed view: inside a guarded
buffer, 16-byte aligned or one element off.  After each launch the guards
of y hold the sentinel, the rows of y outside [rbegin, rend) hold FILL, and
x / gf / gb hold the bits that were uploaded.  (A complex128 block one REAL
off has no torch view, so the complex128 cases are aligned; complex64 runs
both ways.)

Blocks.  A global [N, m] array is launched whole, or as the block a rank
would see: the first block (gb only), a middle block (both planes), the last
block (gf only), or a row sub-range of a middle block.  The planes are the
w global rows before and after the block; where those rows lie outside the
global array they are NaN, which a kernel that masks a term by multiplying
with zero, or reads a row its mask excludes, turns into a wrong result.

Data.  Standard normals; from 500 columns on a few +-0, denormals and +-inf
are sprinkled in (inf - inf and 0 * inf are NaN in kernel and reference
alike; primref.same compares them slot by slot).

No launch in this file passes an axis shorter than stencilref.fd_min_rows:
those inputs are rejected (include/pam.h) and only the error return is
observed, in test_argument_errors.

The kernels whose selectors are read once per process run in fresh child
processes, last in the file."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import primref as pr
import stencilref as sr
from primref import Placed, same
from pylops_mpi_amd import _ffi, kernels

pytestmark = pytest.mark.gpu

NP = {"f64": np.float64, "f32": np.float32}
CNP = {"f64": np.complex128, "f32": np.complex64}
LANES = {"f64": 2, "f32": 4}                 # elements per 16 bytes
FILL = 7.0                                   # rows a launch must not store
COEFF = 1.0 / 1.5                            # inexact in both types
OPS = sr.OPS
CLASS_OPS = (4, 5, 7, 12)    # one op per (term count, halo width) class
ALIGNED = dict(x=0, y=0, gf=0, gb=0)


# -------------------------------------------------------------------- data
def normals(shape, dt, seed):
    """Standard normals; with >= 500 columns a few special values."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape).astype(dt)
    if shape[-1] >= 500:
        tiny = np.finfo(dt).smallest_subnormal
        flat = a.reshape(-1)
        spots = rng.choice(flat.size, size=12, replace=False)
        flat[spots] = np.array([0.0, -0.0, 3 * tiny, -5 * tiny, np.inf,
                                -np.inf] * 2, dtype=dt)
    return a


def ghost(G, lo, w):
    """Rows [lo, lo + w) of the global array; NaN where there is none."""
    out = np.full((w, G.shape[1]), np.nan, dtype=G.dtype)
    for k in range(w):
        if 0 <= lo + k < G.shape[0]:
            out[k] = G[lo + k]
    return out


def view2(p, rows):
    return None if p is None else p.tensor.view(rows, -1)


# --------------------------------------------------------- pam_fd_apply
def run_block(G, s, nloc, rb, re, ops, edges, variant, off, tag, fails,
              cplx=None):
    """Rows [rb, re) of the block G[s:s+nloc] of the global array G, every
    op in ``ops`` and edge in ``edges`` that is defined for N, on the kernel
    ``variant``; failures are appended to ``fails``.  ``cplx``: the complex
    dtype the real array G stands for (columns are (re, im) pairs)."""
    N, m = G.shape
    T = G.dtype.type
    as_op = (lambda a: a) if cplx is None else \
        (lambda a: np.ascontiguousarray(a).view(cplx))
    xs = G[s:s + nloc]
    x = Placed(as_op(xs), off["x"])
    planes = {}
    for w in (1, 2):
        gf = ghost(G, s - w, w) if s > 0 else None
        gb = ghost(G, s + nloc, w) if s + nloc < N else None
        planes[w] = (gf, gb,
                     None if gf is None else Placed(as_op(gf), off["gf"]),
                     None if gb is None else Placed(as_op(gb), off["gb"]))
    xt = view2(x, nloc)
    for op in ops:
        w = sr.HALO[op]
        gf, gb, pgf, pgb = planes[w]
        gft, gbt = view2(pgf, w), view2(pgb, w)
        for edge in edges:
            if N < sr.fd_min_rows(op, edge):
                continue                      # rejected input: never launched
            what = f"{tag} op={op} edge={edge} N={N} m={m} block=[{s}," \
                   f"{s + nloc}) rows=[{rb},{re}) off={off}"
            yfill = np.full((nloc, m), FILL, dtype=T)
            y = Placed(as_op(yfill), off["y"])
            yt = view2(y, nloc)
            got_variant = kernels.fd_variant(yt, xt, gft, gbt, rb, re)
            if got_variant != variant:
                fails.append(f"{what}: variant {got_variant} != {variant}")
                continue
            kernels.fd_apply(yt, xt, gft, gbt, op, edge, s, N, rb, re, COEFF)
            want = yfill.copy()
            want[rb:re] = sr.fd_rows(xs, op, edge, COEFF, s, N, gf, gb, rb,
                                     re)
            full = y.fetch()
            got = pr.rview(y.value(full)).reshape(nloc, m)
            if not y.guards_intact(full):
                fails.append(f"{what}: guards of y overwritten")
            elif not same(got, want):
                bad = np.argwhere(~((got == want)
                                    | (np.isnan(got) & np.isnan(want))))
                fails.append(f"{what}: {len(bad)} wrong, first at "
                             f"{bad[0].tolist()}: {got[tuple(bad[0])]!r} != "
                             f"{want[tuple(bad[0])]!r}")
    for p in [x] + [q for v in planes.values() for q in v[2:]]:
        if p is not None and not p.untouched():
            fails.append(f"{tag} N={N} m={m} block=[{s},{s + nloc}): an "
                         f"input was written")


def block_sets(N, sets):
    """(name, s, nloc, rb, re) of the global length N: whole array, first,
    middle and last block, and rows [1, nloc-2) of the middle block."""
    h = 2 if N >= 5 else 1
    out = []
    if "whole" in sets:
        out.append(("whole", 0, N, 0, N))
    if "first" in sets and N >= 2:
        out.append(("first", 0, max(1, N // 2), 0, max(1, N // 2)))
    if "last" in sets and N >= 2:
        out.append(("last", N // 2, N - N // 2, 0, N - N // 2))
    if N >= 3:
        nloc = N - 2 * h
        if "middle" in sets:
            out.append(("middle", h, nloc, 0, nloc))
        if "sub" in sets and nloc >= 4:
            out.append(("sub", h, nloc, 1, nloc - 2))
    return out


ALL_SETS = ("whole", "first", "middle", "last", "sub")
ROW_COLS = {"f64": (1, 3, 4, 6, 518, 1029), "f32": (1, 3, 8, 12, 1036, 2058)}


def offsets(k, has_gf=False, has_gb=False):
    """One operand of those the launch has (x, y and the planes), the k-th
    in turn, one element off 16-byte alignment."""
    have = ["x", "y"] + ["gf"] * has_gf + ["gb"] * has_gb
    return {name: int(name == have[k % len(have)]) for name in ALIGNED}


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("lanes", [False, True])
@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_row_kernel(monkeypatch, dname, lanes, edge):
    """All 14 ops, N = 1 (or the op's minimum) .. 9, every block set.
    lanes: 16-byte aligned operands and m a multiple of the lane count;
    otherwise one element per lane — m no such multiple, or one operand
    (each of the four in turn) one element off."""
    monkeypatch.setenv("PAM_FD_BAND", "-1")
    fails, k = [], 0
    for m in ROW_COLS[dname]:
        if lanes and m % LANES[dname]:
            continue
        for N in range(1, 10):
            G = normals((N, m), NP[dname], 100 * m + N)
            for name, s, nloc, rb, re in block_sets(N, ALL_SETS):
                if lanes or (m % LANES[dname] and k % 2):
                    off = ALIGNED
                else:
                    off = offsets(k // 2, s > 0, s + nloc < N)
                k += 1
                run_block(G, s, nloc, rb, re, OPS, (edge,), kernels.FD_ROW,
                          off, f"row {dname} {name}", fails)
    assert not fails, (len(fails), fails[:6])


def band_cases(RT):
    """(N, s, nloc, rb, re): the row counts of test_gpu_fd_band as a whole
    array and as first, middle and last block, and sub-ranges of the
    largest middle block that start and end mid-band."""
    from test_gpu_fd_band import row_counts
    out = []
    for nloc in row_counts(RT):
        out += [(nloc, 0, nloc, 0, nloc), (nloc + 3, 0, nloc, 0, nloc),
                (nloc + 4, 2, nloc, 0, nloc), (nloc + 3, 3, nloc, 0, nloc)]
    nloc = 3 * RT + 2
    out += [(nloc + 4, 2, nloc, rb, re)
            for rb, re in ((0, 1), (1, nloc - 1), (RT - 1, 2 * RT + 1),
                           (nloc - 1, nloc), (2, 2 + RT), (RT + 1, RT + 3))]
    return out


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_band_kernel(monkeypatch, dname, edge):
    """The band kernel against stencilref (not against the row kernel):
    one partial column block, and two blocks and a tail."""
    monkeypatch.setenv("PAM_FD_BAND", "1")
    RT = kernels.fd_band_rows()
    fails = []
    for mv in (3, 2 * 256 + 3):
        m = mv * LANES[dname]
        for N, s, nloc, rb, re in band_cases(RT):
            G = normals((N, m), NP[dname], 7 * N + s + mv)
            run_block(G, s, nloc, rb, re, OPS, (edge,), kernels.FD_BAND,
                      ALIGNED, f"band {dname}", fails)
    assert not fails, (len(fails), fails[:6])


@pytest.mark.parametrize("band", ["-1", "1"])
@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_complex_blocks(monkeypatch, dname, band):
    """complex128 / complex64 through kernels.fd_apply: the real view with
    doubled columns, an odd and an even column count."""
    monkeypatch.setenv("PAM_FD_BAND", band)
    fails = []
    offs = [ALIGNED] if dname == "f64" else [ALIGNED, offsets(0), offsets(1)]
    for m in (3, 4):
        for N in (3, 4, 9):
            G = normals((N, 2 * m), NP[dname], 50 + N + m)
            for name, s, nloc, rb, re in block_sets(N, ("whole", "middle")):
                for off in offs:
                    # complex64: one element off is 8 bytes, no 16-B lanes
                    lanes16 = off is ALIGNED and (2 * m) % LANES[dname] == 0
                    variant = kernels.FD_BAND if band == "1" and lanes16 \
                        else kernels.FD_ROW
                    run_block(G, s, nloc, rb, re, CLASS_OPS, (False, True),
                              variant, off, f"complex {dname} {name}", fails,
                              cplx=CNP[dname])
    assert not fails, (len(fails), fails[:6])


# -------------------------------------------------------- pam_fd_serial
def run_serial(x, ops, edges, off, tag, fails, cplx=None):
    """pam_fd_serial on the real [batch, d, m] array x (standing for the
    complex dtype ``cplx`` if given), x and y placed at off = (x, y); first
    and last batch are reported separately — a wrong batch base shows
    there."""
    batch, d, m = x.shape
    as_op = (lambda a: a) if cplx is None else \
        (lambda a: np.ascontiguousarray(a).view(cplx))
    px = Placed(as_op(x), off[0])
    xt = px.tensor.view(batch, d, -1)
    for op in ops:
        for edge in edges:
            if d < sr.fd_min_rows(op, edge):
                continue                      # rejected input: never launched
            what = f"{tag} op={op} edge={edge} shape={x.shape} off={off}"
            py = Placed(as_op(np.full(x.shape, FILL, dtype=x.dtype)), off[1])
            kernels.fd_serial(py.tensor.view(batch, d, -1), xt, op, edge,
                              COEFF)
            want = sr.fd_serial_ref(x, op, edge, COEFF)
            full = py.fetch()
            got = pr.rview(py.value(full)).reshape(x.shape)
            if not py.guards_intact(full):
                fails.append(f"{what}: guards of y overwritten")
            for b in sorted({0, batch - 1}):
                if not same(got[b], want[b]):
                    fails.append(f"{what}: batch {b} wrong")
            if not same(got, want):
                fails.append(f"{what}: wrong")
    if not px.untouched():
        fails.append(f"{tag} shape={x.shape}: x was written")


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_fd_serial(dname, edge):
    fails, k = [], 0
    for batch, m in ((1, 1), (3, 1), (1, 5), (2, 3)):
        for d in range(1, 10):
            x = normals((batch, d, m), NP[dname], 11 * d + batch + m)
            run_serial(x, OPS, (edge,), (k % 2, k // 2 % 2),
                       f"serial {dname}", fails)
            k += 1
    assert not fails, (len(fails), fails[:6])


@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_fd_serial_complex(dname):
    fails = []
    off1 = 0 if dname == "f64" else 1       # complex128: aligned only
    for k, (batch, d, m) in enumerate(((2, 3, 3), (3, 9, 2), (1, 4, 1))):
        x = normals((batch, d, 2 * m), NP[dname], 70 + k)
        run_serial(x, CLASS_OPS, (False, True),
                   ((k % 2) * off1, ((k + 1) % 2) * off1),
                   f"serial c{dname}", fails, cplx=CNP[dname])
    assert not fails, (len(fails), fails[:6])


def test_fd_serial_stride_loop():
    """One launch just over the grid cap of 4096 blocks x 256 threads: every
    thread of the first blocks takes a second pass of the stride loop."""
    x = normals((3, 7, 50000), np.float32, 80)
    assert x.size > 4096 * 256
    fails = []
    run_serial(x, CLASS_OPS, (True,), (0, 0), "serial stride", fails)
    assert not fails, fails[:6]


# ----------------------------------------------------------- pam_nsconv
OH, DH = 3.0, 5.5    # anchors 3, 8.5, 14, 19.5: samples 3 and 14 sit on one


def run_nsconv(x, hs, off, tag, fails):
    batch, d, m = x.shape
    px, ph = Placed(x, off), Placed(hs, 1 - off)
    for forward in (True, False):
        what = f"{tag} forward={forward} shape={x.shape} hs={hs.shape} " \
               f"off={off}"
        py = Placed(np.full(x.shape, FILL, dtype=x.dtype), off)
        kernels.nsconv(py.tensor.view(x.shape), px.tensor.view(x.shape),
                       ph.tensor.view(hs.shape), forward, OH, DH)
        want = sr.nsconv_ref(x, hs, OH, DH, forward)
        full = py.fetch()
        got = py.value(full).reshape(x.shape)
        if not py.guards_intact(full):
            fails.append(f"{what}: guards of y overwritten")
        elif not same(got, want):
            fails.append(f"{what}: wrong")
    if not (px.untouched() and ph.untouched()):
        fails.append(f"{tag}: an input was written")


@pytest.mark.parametrize("hsize", [1, 3, 7])
@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_nsconv(dname, hsize):
    """Forward and adjoint; 1, 2 and 4 anchor filters, so that samples fall
    before the first anchor (0..2), on an anchor (3, 14; weight 0), between
    two, and after the last; axes shorter than the filter."""
    fails, k = [], 0
    rng = np.random.default_rng(90 + hsize)
    for nf in (1, 2, 4):
        hs = rng.standard_normal((nf, hsize)).astype(NP[dname])
        for d in sorted({1, 2, max(hsize - 1, 1), 24}):
            for batch, m in ((1, 1), (3, 1), (1, 4), (2, 3)):
                x = normals((batch, d, m), NP[dname], k)
                run_nsconv(x, hs, k % 2, f"nsconv {dname}", fails)
                k += 1
    assert not fails, (len(fails), fails[:6])


def test_nsconv_stride_loop():
    """One launch over the grid cap (4096 blocks x 256 threads)."""
    x = normals((3, 7, 50000), np.float32, 81)
    assert x.size > 4096 * 256
    hs = np.random.default_rng(82).standard_normal((2, 3)).astype(np.float32)
    fails = []
    run_nsconv(x, hs, 0, "nsconv stride", fails)
    assert not fails, fails


# ------------------------------------------------------ argument errors
def test_argument_errors():
    """PAM_EOP, PAM_EDTYPE and PAM_EARG come back before anything is
    launched: the output keeps every bit.  The axis-too-short inputs are
    observed here, through the error return, and nowhere else."""
    lib = _ffi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    EARG, EDTYPE, EOP = -1, -2, -3
    x = Placed(normals((1, 3, 4), np.float64, 1))
    y = Placed(np.full(12, FILL))

    def apply(op=4, edge=0, nloc=3, m=4, row0=0, nglob=3, rb=0, re=3,
              dtype=_ffi.F64):
        return lib.pam_fd_apply(stream, op, edge, x.ptr, None, None, y.ptr,
                                nloc, m, row0, nglob, rb, re, 1.0, dtype)

    def serial(op=4, edge=0, batch=1, d=3, m=4, dtype=_ffi.F64):
        return lib.pam_fd_serial(stream, op, edge, x.ptr, y.ptr, batch, d, m,
                                 1.0, dtype)

    for fn in (apply, serial):
        assert fn(op=-1) == EOP and fn(op=14) == EOP
        assert fn(dtype=_ffi.C128) == EDTYPE and fn(dtype=_ffi.C64) == EDTYPE
        assert fn(m=0) == EARG and fn(m=-4) == EARG
    assert apply(re=4) == EARG and apply(rb=-1) == EARG
    assert apply(nloc=-1, re=-1) == EARG
    assert serial(batch=0) == EARG and serial(d=0) == EARG
    for op in OPS:
        for n in range(1, sr.fd_min_rows(op, True)):
            # a whole array, and a one-row block of so short a global axis
            assert apply(op=op, edge=1, nloc=n, nglob=n, re=n) == EARG
            assert apply(op=op, edge=1, nloc=1, nglob=n, re=1) == EARG
            assert apply(op=op, edge=1, nloc=0, nglob=n, re=0) == EARG
            assert serial(op=op, edge=1, d=n) == EARG
            assert serial(op=op, edge=1, d=n, batch=3, m=1) == EARG
    torch.cuda.synchronize()
    assert y.untouched() and x.untouched()
    # the same through the tensor layer
    yt, xt = y.tensor.view(3, 4), x.tensor.view(3, 4)
    with pytest.raises(ValueError, match="at least 3"):
        kernels.fd_apply(yt[:2], xt[:2], None, None, 12, True, 0, 2, 0, 2,
                         1.0)
    with pytest.raises(ValueError, match="at least 2"):
        kernels.fd_serial(yt.view(3, 1, 4), xt.view(3, 1, 4), 5, True, 1.0)
    torch.cuda.synchronize()
    assert y.untouched() and x.untouched()


# ------------------------------------- kernels behind once-read selectors
def run_row_capped():
    """For a process started with PAM_FD_GY=2 PAM_FD_CAP=4: the row kernel
    with fewer block-rows than rows and 11 column blocks on at most 4 (one
    row) or 2 (more rows; then a 4x-unrolled trip, single trips and a
    partial last block per row) -> list of failures."""
    os.environ["PAM_FD_BAND"] = "-1"
    fails = []
    for dname in ("f64", "f32"):
        m = (10 * 256 + 37) * LANES[dname]
        for nloc in (1, 5, 9):
            for N, s in ((nloc, 0), (nloc + 8, 4)):    # whole, middle
                G = normals((N, m), NP[dname], 3 * N + s)
                run_block(G, s, nloc, 0, nloc, CLASS_OPS, (False, True),
                          kernels.FD_ROW, ALIGNED, f"capped {dname}", fails)
        # one element per lane under the same caps
        G = normals((13, m + 1), NP[dname], 17)
        run_block(G, 4, 5, 0, 5, CLASS_OPS, (True,), kernels.FD_ROW,
                  ALIGNED, f"capped scalar {dname}", fails)
    return fails


ROLL_COLS = {"f64": (2, 4, 6, 8, 4102), "f32": (4, 8, 12, 8204)}


def run_roll_forced(dname):
    """For a process started with PAM_FD_ROLL=1 and PAM_FD_BAND unset: the
    rolling kernel at 16- and 32-byte lanes, one and two column blocks (the
    second with chains that own no column), 1 .. 33 rows -> list of
    failures."""
    fails = []
    for m in ROLL_COLS[dname]:
        for nloc in (1, 2, 3, 5, 17, 33):
            cases = [(nloc, 0, 0, nloc), (nloc + 3, 0, 0, nloc),
                     (nloc + 4, 2, 0, nloc), (nloc + 3, 3, 0, nloc)]
            if nloc >= 5:
                cases.append((nloc + 4, 2, 1, nloc - 2))
            for N, s, rb, re in cases:
                G = normals((N, m), NP[dname], N + s + m)
                run_block(G, s, nloc, rb, re, OPS, (False, True),
                          kernels.FD_ROLL, ALIGNED, f"roll {dname}", fails)
    return fails


DONE = "stencil child compared everything:"
CHILD = """
import sys
sys.path[:0] = [{tests!r}, {root!r}]
import test_gpu_stencil as t
bad = t.{call}
print(t.DONE, len(bad), "failures")
print("\\n".join(bad[:20]))
sys.exit(1 if bad else 0)
"""


def in_child(call, **env):
    """Run the call ``call`` of this module in a fresh interpreter with
    ``env`` set.  A child that does not get to report its comparisons —
    killed by a signal, stopped by a device error, or out of time — ends the
    session: nothing more is started on the device after a fault."""
    tests = os.path.dirname(os.path.abspath(__file__))
    full = {k: v for k, v in os.environ.items()
            if not k.startswith("PAM_FD_")}
    full.update(env)
    cmd = [sys.executable, "-c",
           CHILD.format(tests=tests, root=os.path.dirname(tests), call=call)]
    try:
        r = subprocess.run(cmd, env=full, timeout=300, capture_output=True,
                           text=True)
    except subprocess.TimeoutExpired:
        pytest.exit(f"{call}: the child process hung; nothing more is run on "
                    f"the device", returncode=1)
    # the child either reports its comparisons (the DONE line, exit 0 or 1)
    # or it ended some other way: a signal, an abort, or an exception on
    # the way — a HIP error such as an illegal memory access arrives as one
    done = r.returncode in (0, 1) and DONE in r.stdout
    if not done:
        pytest.exit(f"{call}: the child process did not finish "
                    f"({r.returncode}); nothing more is run on the device\n"
                    f"{r.stdout[-1000:]}\n{r.stderr[-2000:]}", returncode=1)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:],
                               r.stderr[-2000:])


def test_row_kernel_under_grid_caps():
    """PAM_FD_GY / PAM_FD_CAP are read once per process: the row kernel's
    row-stride loop, column-stride loop and 4x-unrolled trips at a small
    shape."""
    in_child("run_row_capped()", PAM_FD_GY="2", PAM_FD_CAP="4")


@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_roll_kernel_forced(dname):
    """PAM_FD_ROLL is read once per process: the rolling kernel at small
    shapes, against stencilref."""
    in_child(f"run_roll_forced({dname!r})", PAM_FD_ROLL="1")
