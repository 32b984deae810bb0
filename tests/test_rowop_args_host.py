"""The row-operation family accepts and refuses exactly the argument lists on record (tests/rowop_args.py builds the grid; tests/rowop_args_expected.json is
the record of the library before its host layer moved onto lpi_amd/csrc/dispatch.h and the shared per-op predicates).  No GPU is needed: a refused call returns
before any launch, an accepted one counts its launch and, without a device, fails in the runtime."""
import json
import os
import re

import pytest
import torch

import rowop_args as G
from lpi_amd import _lib

CSRC = os.path.join(G.REPO, "lpi_amd", "csrc")


@pytest.fixture(scope="module")
def grid():
    with open(G.EXPECTED) as f:
        rec = json.load(f)
    cases = G.cases()
    want = []
    seen = {}
    for name, _, _ in cases:
        i = seen.get(name, 0)
        assert name in rec and i < len(rec[name]), f"{name}: the grid has more tuples than the record: record it again (tests/rowop_args.py)"
        want.append(rec[name][i])
        seen[name] = i + 1
    assert seen == {k: len(v) for k, v in rec.items()}, "the grid and the record list different tuples: record it again (tests/rowop_args.py)"
    return cases, want


def test_grid_covers_every_entry_point(grid):
    """Every lpi_* function the two row sources define is bound (_lib.SIGNATURES) and in the grid, lpi_row_jobs with each of its ten ops; every name has at
    least one accepted and one refused tuple.  lpi_rowstat_guard alone is exempt (it asks the runtime about its pointer)."""
    cases, want = grid
    exported = set()
    for src in ("rowops.hip", "mx8_rows.hip"):
        with open(os.path.join(CSRC, src)) as f:
            exported |= set(re.findall(r'^extern "C" \w+ (lpi_\w+)\(', f.read(), re.M))
    assert "lpi_scatter_add_rows" in exported and "lpi_row_jobs" in exported and len(exported) >= 34
    assert exported <= set(_lib.SIGNATURES)
    names = {c[0] for c in cases}
    assert exported - G.EXEMPT <= names, sorted(exported - G.EXEMPT - names)
    ops = {k for k in vars(_lib) if k.startswith("ROWOP_")}
    assert len(ops) == 10 and {"job:" + k[len("ROWOP_"):] for k in ops} <= names
    for name in names:
        classes = {bool(w[1]) for c, w in zip(cases, want) if c[0] == name}
        assert classes == {True, False}, f"{name}: the grid needs an accepted and a refused tuple"


def test_refused_lists_stay_refused(grid):
    """Same code, and not one launch over the whole class."""
    cases, want = grid
    n0 = _lib.launch_count()
    bad = []
    for (name, label, thunk), (rc, launches) in zip(cases, want):
        if launches == 0:
            got = int(thunk())
            if got != rc:
                bad.append((name, label, got, rc))
            assert _lib.launch_count() == n0, f"{name} [{label}] launched: it is refused on record (code {rc})"      # stop at the first: nothing more on made-up addresses
    assert not bad, bad[:20]


def test_accepted_lists_stay_accepted(grid):
    """Same code and launch count per tuple.  Only without a device: with one, the accepted lists would launch kernels on made-up addresses."""
    if torch.cuda.device_count() != 0:
        pytest.skip("a GPU is present: the accepted argument lists would launch on made-up addresses (this class is replayed on machines without one)")
    cases, want = grid
    bad = []
    for (name, label, thunk), (rc, launches) in zip(cases, want):
        if launches:
            n0 = _lib.launch_count()
            got = [int(thunk()), _lib.launch_count() - n0]
            if got != [rc, launches]:
                bad.append((name, label, got, [rc, launches]))
    assert not bad, bad[:20]
