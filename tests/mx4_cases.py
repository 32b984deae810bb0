"""Test data shared by tests/test_search_mx4_host.py (the premise, on the CPU) and tests/test_search_mx4_gpu.py: MX-FP4 rows built on the host whose scores
are exact in every summation order, with many exact ties."""
import functools

import numpy as np
import torch

import mx4_emulate as MX4

KS = [(1, False), (16, False), (17, True), (100, True), (256, True)]      # (k, wide entry point) of the GPU tests; k is capped at ng


@functools.lru_cache(maxsize=None)
def int_case(nq, ng, E, seed):
    """Codes and scale bytes built on the host.  Nibbles: 3 % are +-1 (codes 2 and 10), the rest 0; scale bytes uniform in 125 .. 129 per (row, block).  A
    product is +-2^s with -4 <= s <= 4, so every partial sum is a multiple of 2^-4 below 2^14: exact in f32 in every order, and the f64 product of the
    dequantised rows is the exact score.  Two of every three gallery rows are copies (codes and scales) of rows of the first third, so most rows' best
    scores come in exact ties whatever the nibbles do: the order inside a tie is the index order, descending.  Computed once per shape."""
    gen = torch.Generator().manual_seed(seed)

    def rows(n):
        c = torch.where(torch.rand(n, E, generator=gen) < 0.03, torch.where(torch.rand(n, E, generator=gen) < 0.5, 2, 10), 0).to(torch.uint8)
        return MX4.pack(c), (125 + torch.randint(0, 5, (n, E // 32), generator=gen)).to(torch.uint8)

    qc, qs = rows(nq)
    gc, gs = rows(ng)
    base = max(1, ng // 3)
    src = torch.randint(0, base, (ng - base,), generator=gen)
    gc[base:], gs[base:] = gc[src], gs[src]
    s = (MX4.dequantize(qc, qs) @ MX4.dequantize(gc, gs).t()).numpy()
    assert np.abs(s).max() < 2 ** 14 and np.array_equal(s * 16, np.round(s * 16))
    key = np.round(s * 16).astype(np.int64) * ng + np.arange(ng, dtype=np.int64)[None, :]      # monotone in (value, then index): a row's keys are distinct
    order = np.argsort(-key, axis=1, kind="stable")
    return qc, qs, gc, gs, s, order


def tie_shares(s, order):
    """k -> the share of rows whose scores at positions k - 1 and k of the sorted row are equal: the list's end falls inside a tie"""
    srt = np.take_along_axis(s, order, 1)
    return {k: float((srt[:, k - 1] == srt[:, k]).mean()) for k, _ in KS}
