"""The stencil launch plan's automatic rule, against a table recorded from
the build before the plan was rewritten (tests/golden/fd_dispatch.json,
tests/golden/generate_fd_dispatch.py).  Runs without a GPU:
pam_fd_variant is a host-side query."""
import ctypes
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LIB = os.path.join(ROOT, "pylops_mpi_amd", "libpam.so")


def _generator():
    spec = importlib.util.spec_from_file_location(
        "generate_fd_dispatch", os.path.join(GOLDEN,
                                             "generate_fd_dispatch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "fd_dispatch.json")) as f:
        return json.load(f)


def test_fixture_covers_the_grid(golden):
    gen = _generator()
    assert golden["nrows"] == gen.NROWS == [0, 1, 15, 16, 17, 1023, 1024,
                                            1025, 1536]
    assert [(r["dtype"], r["aligned16"], r["m"]) for r in golden["rows"]] \
        == gen.cases()
    for dt, esize in ((0, 8), (1, 4)):
        ms = {r["m"] for r in golden["rows"] if r["dtype"] == dt}
        for nbytes in (2621440, 4194304):
            t = nbytes // esize
            assert {t - 4, t - 3, t - 2, t, t + 1, t + 2, t + 4} <= ms
    # every kernel appears, so the table can tell them apart
    seen = {v for r in golden["rows"] for v in r["variant"]}
    assert seen == {0, 1, 2}


def test_dispatch_table_reproduced(golden, monkeypatch):
    for name in list(os.environ):
        if name.startswith("PAM_"):
            monkeypatch.delenv(name)
    got = _generator().table(ctypes.CDLL(LIB))
    assert len(got) == len(golden["rows"])
    for g, w in zip(got, golden["rows"]):
        assert g == w, (g, w)
