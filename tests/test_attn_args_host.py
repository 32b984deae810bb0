"""The attention family accepts and refuses exactly the argument lists on record (tests/attn_args.py builds the grid; tests/attn_args_expected.json is the
record of the library before its host layer moved onto one call struct, the shared predicates and lpi_amd/csrc/dispatch.h).  Only without a GPU: a refused
call returns before any launch, an accepted one fails in the runtime with its no-device code — with a device, a regression that accepted a recorded refusal
would launch on made-up addresses, so the whole module is skipped there (refusal on a device: tests/test_attn_strides_gpu.py, on real buffers)."""
import json
import os
import re

import pytest
import torch

import attn_args as G
from lpi_amd import _lib

CSRC = os.path.join(G.REPO, "lpi_amd", "csrc")
SOURCES = ("attention.hip", "attn_pooled.hip", "attn_hd.hip")

pytestmark = pytest.mark.skipif(torch.cuda.device_count() != 0, reason="a GPU is present: the argument lists point at made-up addresses (replayed on machines without one)")


@pytest.fixture(scope="module")
def grid():
    with open(G.EXPECTED) as f:
        rec = json.load(f)
    assert re.match(r"[0-9a-f]{7,40} ", rec.pop("recorded_from")), "the record names the commit it was made from"
    cases = G.cases()
    want = []
    seen = {}
    for name, _, _ in cases:
        i = seen.get(name, 0)
        assert name in rec and i < len(rec[name]), f"{name}: the grid has more tuples than the record: record it again (tests/attn_args.py)"
        want.append(rec[name][i])
        seen[name] = i + 1
    assert seen == {k: len(v) for k, v in rec.items()}, "the grid and the record list different tuples: record it again (tests/attn_args.py)"
    return cases, want


def test_grid_covers_every_entry_point(grid):
    """Every extern "C" function of the three sources is bound (_lib.SIGNATURES) and in the grid, with at least one accepted and one refused tuple."""
    cases, want = grid
    exported = set()
    for src in SOURCES:
        with open(os.path.join(CSRC, src)) as f:
            exported |= set(re.findall(r'^extern "C" \w+ (lpi_\w+)\(', f.read(), re.M))
    assert "lpi_attn_bwd_layout" in exported and "lpi_attn_pooled_bwd_desc" in exported and "lpi_attn_hd_supported" in exported and len(exported) == 22
    assert exported <= set(_lib.SIGNATURES)
    names = {c[0] for c in cases}
    assert exported == names, sorted(exported ^ names)
    for name in names:
        classes = {G.accepted(name, w[0]) for c, w in zip(cases, want) if c[0] == name}
        assert classes == {True, False}, f"{name}: the grid needs an accepted and a refused tuple"
    assert all(w[1] == 0 for c, w in zip(cases, want) if not G.accepted(c[0], w[0])), "a refused list has launched nothing"


def test_refused_lists_stay_refused(grid):
    """Same code, and not one launch over the whole class."""
    cases, want = grid
    n0 = _lib.launch_count()
    bad = []
    for (name, label, thunk), (rc, launches) in zip(cases, want):
        if not G.accepted(name, rc):
            got = int(thunk())
            if got != rc:
                bad.append((name, label, got, rc))
            assert _lib.launch_count() == n0, f"{name} [{label}] launched: it is refused on record (code {rc})"      # stop at the first: nothing more on made-up addresses
    assert not bad, (len(bad), bad[:20])


def test_accepted_lists_stay_accepted(grid):
    """Same code and launch count per tuple."""
    cases, want = grid
    bad = []
    for (name, label, thunk), (rc, launches) in zip(cases, want):
        if G.accepted(name, rc):
            n0 = _lib.launch_count()
            got = [int(thunk()), _lib.launch_count() - n0]
            if got != [rc, launches]:
                bad.append((name, label, got, [rc, launches]))
    assert not bad, (len(bad), bad[:20])


def test_tuning_keys_are_restored(grid):
    """The grid sets tuning keys 3, 7 and 13 for single calls: every key is back at its default afterwards."""
    cases, _ = grid
    lib = _lib.load()
    before = [lib.lpi_get_tuning(k) for k in range(16)]
    for name, label, thunk in cases:
        if " key " in label and label.endswith(": good"):
            thunk()
    assert [lib.lpi_get_tuning(k) for k in range(16)] == before
