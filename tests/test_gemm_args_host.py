"""The GEMM family accepts and refuses exactly the argument lists on record, and sends every accepted one to the kernel on record (tests/gemm_args.py builds
the grid; tests/gemm_args_expected.json is the record of the library before its host layer moved onto one call struct and one typed pick,
lpi_amd/csrc/gemm_host.h).  Only without a GPU: a refused call returns before any launch, an accepted one fails in the runtime with its no-device code — with a
device, a regression that accepted a recorded refusal would launch on made-up addresses, so the whole module is skipped there (refusal and kernel choice on a
device: tests/test_gemm_strides_gpu.py, on real buffers)."""
import os
import re

import pytest
import torch

import gemm_args as G
from lpi_amd import _lib

CSRC = os.path.join(G.REPO, "lpi_amd", "csrc")
SOURCES = ("gemm.hip", "gemm256.hip", "gemm256p.hip", "gemm256x128.hip", "gemm_rows.hip", "gemm_mx8.hip")
ENTRY_POINTS = {"lpi_gemm_nt", "lpi_gemm_nt_grouped", "lpi_gemm_nt_rows", "lpi_gemm_nt_rows_supported", "lpi_gemm_ln_supported", "lpi_gemm_nt_mx8", "lpi_gemm_mx8_ok",
                "lpi_gemm_nt_mx8_256", "lpi_gemm_mx8_256_ok"}

pytestmark = pytest.mark.skipif(torch.cuda.device_count() != 0, reason="a GPU is present: the argument lists point at made-up addresses (replayed on machines without one)")


@pytest.fixture(scope="module")
def grid():
    src, rec = G.load_record()
    assert re.match(r"[0-9a-f]{7,40} ", src), "the record names the commit it was made from"
    cases = G.cases()
    want = []
    seen = {}
    for name, _, _ in cases:
        i = seen.get(name, 0)
        assert name in rec and i < len(rec[name]), f"{name}: the grid has more tuples than the record: record it again (tests/gemm_args.py)"
        want.append(rec[name][i])
        seen[name] = i + 1
    assert seen == {k: len(v) for k, v in rec.items()}, "the grid and the record list different tuples: record it again (tests/gemm_args.py)"
    return cases, want


def test_grid_covers_every_entry_point(grid):
    """Every extern "C" function of the six sources (but the two that only read thread state back) is bound (_lib.SIGNATURES) and in the grid, with at least one
    accepted and one refused tuple; every kernel the family attributes a launch to is chosen by some accepted tuple."""
    cases, want = grid
    exported = set()
    for src in SOURCES:
        with open(os.path.join(CSRC, src)) as f:
            exported |= set(re.findall(r'^extern "C" \w+ (lpi_\w+)\(', f.read(), re.M))
    assert exported - {"lpi_gemm_last_grouped", "lpi_gemm_stamps_read"} == ENTRY_POINTS, sorted(exported)      # (the stamps reader: diagnostic builds only)
    assert exported - {"lpi_gemm_stamps_read"} <= set(_lib.SIGNATURES)
    names = {c[0] for c in cases}
    assert names == ENTRY_POINTS, sorted(ENTRY_POINTS ^ names)
    for name in names:
        classes = {G.accepted(name, w[0]) for c, w in zip(cases, want) if c[0] == name}
        assert classes == {True, False}, f"{name}: the grid needs an accepted and a refused tuple"
    refused = [w for c, w in zip(cases, want) if not G.accepted(c[0], w[0])]
    assert all(w[1] == 0 and w[2] == _lib.GEMM_K_ROWS and w[3] == 0 for w in refused), "a refused list has launched nothing and chosen no kernel"
    chosen = {w[2] for c, w in zip(cases, want) if c[0] not in G.PREDICATES and G.accepted(c[0], w[0])}
    assert chosen == {_lib.GEMM_K_128, _lib.GEMM_K_256, _lib.GEMM_K_256_TAIL, _lib.GEMM_K_256X128, _lib.GEMM_K_ROWS, _lib.GEMM_K_MX8, _lib.GEMM_K_X3, _lib.GEMM_K_MX8_256}


def test_refused_lists_stay_refused(grid):
    """Same code, no kernel chosen, and not one launch over the whole class."""
    cases, want = grid
    lib = _lib.load()
    bad = []
    for (name, label, thunk), w in zip(cases, want):
        if not G.accepted(name, w[0]):
            got = G.run_one(lib, thunk)
            if got != w:
                bad.append((name, label, got, w))
            assert got[1] == 0, f"{name} [{label}] launched: it is refused on record (code {w[0]})"      # stop at the first: nothing more on made-up addresses
    assert not bad, (len(bad), bad[:20])


def test_accepted_lists_stay_accepted(grid):
    """Same code, launch count, kernel and grouped flag per tuple."""
    cases, want = grid
    lib = _lib.load()
    bad = []
    for (name, label, thunk), w in zip(cases, want):
        if G.accepted(name, w[0]):
            got = G.run_one(lib, thunk)
            if got != w:
                bad.append((name, label, got, w))
    assert not bad, (len(bad), bad[:20])


def test_tuning_keys_are_restored(grid):
    """The grid sets tuning keys for single calls (gemm_args.TUNINGS): every key is back at its default afterwards."""
    cases, _ = grid
    lib = _lib.load()
    before = [lib.lpi_get_tuning(k) for k in range(16)]
    assert {k for k, _ in G.TUNINGS} == {0, 1, 2, 4, 5, 6, 8, 14, 15}
    n = 0
    for name, label, thunk in cases:
        if " key " in label and label.endswith(": good"):
            thunk()
            n += 1
    assert n >= len(G.TUNINGS) and [lib.lpi_get_tuning(k) for k in range(16)] == before
