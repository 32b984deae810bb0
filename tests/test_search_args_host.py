"""The streamed search accepts and refuses exactly the argument lists on record, and its two workspace functions answer what is on record
(tests/search_args.py builds the grid; tests/search_args_expected.json is the record of the library before its host layer moved onto one call struct,
SearchCall in lpi_amd/csrc/search_tile.h).  Only without a GPU: a refused call returns before any launch, an accepted one fails in the runtime with its
no-device code -- with a device, a regression that accepted a recorded refusal would launch on made-up addresses, so the whole module is skipped there
(results on a device: the tests/test_search*_gpu.py modules, on real buffers)."""
import os
import re

import pytest
import torch

import search_args as S
from lpi_amd import _lib

CSRC = os.path.join(S.REPO, "lpi_amd", "csrc")
SOURCES = ("search.hip", "search16.hip", "search_mx8.hip", "search_mx4.hip", "search_wide.hip", "search_rerank.hip")
LAUNCHING = {"lpi_search_topk", "lpi_search_rank", "lpi_search_topk_t", "lpi_search_rank_t", "lpi_search_topk_mx8", "lpi_search_rank_mx8", "lpi_search_topk_mx4",
             "lpi_search_topk_wide_mx4", "lpi_search_topk_wide", "lpi_search_topk_wide_t", "lpi_search_topk_wide_mx8", "lpi_search_rerank", "lpi_search_rerank_t"}

pytestmark = pytest.mark.skipif(torch.cuda.device_count() != 0, reason="a GPU is present: the argument lists point at made-up addresses (replayed on machines without one)")


@pytest.fixture(scope="module")
def grid():
    src, rec, tables = S.load_record()
    assert re.match(r"[0-9a-f]{7,40}\b", src), "the record names the commit it was made from"
    cases = S.cases()
    want = []
    seen = {}
    for name, _, _ in cases:
        i = seen.get(name, 0)
        assert name in rec and i < len(rec[name]), f"{name}: the grid has more tuples than the record: record it again (tests/search_args.py)"
        want.append(rec[name][i])
        seen[name] = i + 1
    assert seen == {k: len(v) for k, v in rec.items()}, "the grid and the record list different tuples: record it again (tests/search_args.py)"
    return cases, want, tables


def test_grid_covers_every_entry_point(grid):
    """Every extern "C" function of the six sources is bound (_lib.SIGNATURES) and in the grid: the launching ones each with an accepted and a refused tuple,
    the two workspace functions each with a table that holds sizes and refusals."""
    cases, want, tables = grid
    exported = set()
    for src in SOURCES:
        with open(os.path.join(CSRC, src)) as f:
            exported |= set(re.findall(r'^extern "C" \w+ (lpi_\w+)\(', f.read(), re.M))
    assert exported == LAUNCHING | set(S.WORKSPACES), sorted(exported)
    assert exported <= set(_lib.SIGNATURES)
    names = {c[0] for c in cases}
    assert names == LAUNCHING, sorted(LAUNCHING ^ names)
    for name in names:
        classes = {S.accepted(w[0]) for c, w in zip(cases, want) if c[0] == name}
        assert classes == {True, False}, f"{name}: the grid needs an accepted and a refused tuple"
    assert set(tables) == set(S.WORKSPACES)
    for name, values in tables.items():
        assert len(values) == len(S.WS_NQ) * len(S.WS_NG) * len(S.WS_K[name]) and S.EINVAL in values and max(values) > 0, name


def test_refused_lists_stay_refused(grid):
    """Same code, and not one launch over the whole class."""
    cases, want, _ = grid
    bad = []
    for (name, label, thunk), w in zip(cases, want):
        if not S.accepted(w[0]):
            assert w[1] == 0, (name, label, w)
            got = S.run_one(thunk)
            if got != w:
                bad.append((name, label, got, w))
            assert got[1] == 0, f"{name} [{label}] launched: it is refused on record (code {w[0]})"      # stop at the first: nothing more on made-up addresses
    assert not bad, (len(bad), bad[:20])


def test_accepted_lists_stay_accepted(grid):
    """Same code and launch count per tuple."""
    cases, want, _ = grid
    bad = []
    for (name, label, thunk), w in zip(cases, want):
        if S.accepted(w[0]):
            got = S.run_one(thunk)
            if got != w:
                bad.append((name, label, got, w))
    assert not bad, (len(bad), bad[:20])


def test_workspace_tables_match_the_record(grid):
    _, _, tables = grid
    got = S.workspace_tables()
    for name in S.WORKSPACES:
        keys = [(nq, ng, k) for nq in S.WS_NQ for ng in S.WS_NG for k in S.WS_K[name]]
        bad = [(key, g, w) for key, g, w in zip(keys, got[name], tables[name]) if g != w]
        assert not bad, (name, len(bad), bad[:20])
