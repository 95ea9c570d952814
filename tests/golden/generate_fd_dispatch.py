"""Generate the stencil dispatch-table fixture fd_dispatch.json.

pam_fd_variant(dtype, m, nrows, aligned16) is a pure host query — libpam.so
loads without a GPU — reporting the kernel a stencil launch uses:
0 row-parallel, 1 rolling window, 2 row band.  The table pins the automatic
rule (no PAM_* variable set) over a fixed grid, so that a change to the
launch code that is meant to keep the dispatch can prove it did: generate
the table from the build BEFORE the change, commit it, and
tests/test_fd_dispatch.py asserts the build after it reproduces it.

Grid: both dtypes; aligned 0 and 1; m just below, at and just above the
2.5 MiB and 4 MiB row thresholds with m % 4 of 0, 2 and 1; row counts
around the band kernel's 16-row floor and the 1024-row raggedness rule.

Run from the repo root:
    python tests/golden/generate_fd_dispatch.py [path/to/libpam.so]
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "fd_dispatch.json")
DEFAULT_LIB = os.path.join(HERE, "..", "..", "pylops_mpi_amd", "libpam.so")

DTYPES = {0: 8, 1: 4}           # PAM_F64, PAM_F32 -> element bytes
NROWS = [0, 1, 15, 16, 17, 1023, 1024, 1025, 1536]
ROW_THRESHOLDS = [5 << 19, 4 << 20]   # 2.5 MiB, 4 MiB of row


def columns(esize):
    """m % 4 == 0, 2, 1 just below and just above each threshold, and the
    threshold itself."""
    out = []
    for nbytes in ROW_THRESHOLDS:
        t = nbytes // esize
        assert t % 4 == 0
        out += [t - 4, t - 2, t - 3, t, t + 4, t + 2, t + 1]
    return out


def cases():
    """[(dtype, aligned16, m)] — one table row each, NROWS entries wide."""
    return [(dt, al, m) for dt, esize in DTYPES.items() for al in (0, 1)
            for m in columns(esize)]


def table(lib):
    for name in sorted(os.environ):
        assert not name.startswith("PAM_"), f"{name} is set"
    fn = lib.pam_fd_variant
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int]
    return [{"dtype": dt, "aligned16": al, "m": m,
             "variant": [fn(dt, m, n, al) for n in NROWS]}
            for dt, al, m in cases()]


def main():
    lib = ctypes.CDLL(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_LIB)
    rows = table(lib)
    with open(OUT, "w") as f:
        f.write('{"nrows": %s,\n "rows": [\n  ' % json.dumps(NROWS))
        f.write(",\n  ".join(json.dumps(r) for r in rows))
        f.write("\n ]}\n")
    print(f"wrote {OUT}: {len(rows)} rows x {len(NROWS)} row counts")


if __name__ == "__main__":
    main()
