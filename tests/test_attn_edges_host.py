"""tests/attn_edges.py held to its own claims on the CPU (conditions, not measurements):
  * an honest kernel — f64 with the counted roundings applied (attn_edges.emulate) — stays inside the per-element bars for every arm, length class, operand type
    and kernel class, causal and not;
  * each mutant of the reference leaves the bars by a factor of ten or more on the arm that was built for it;
  * the phantom-key mutant PASSES the relerr bars the attention tests had so far, on their own random data at L = 213: the hole tests/test_attn_edges_gpu.py closes.
"""
import functools

import pytest
import torch

import attn_edges as AE

TYPES = [torch.float32, torch.bfloat16, torch.float16]
TID = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
LENGTHS = [1, 2, 17, 33, 65, 97, 225, 289]      # one per tile class: below a 16-row tile, one past a 16 / 32 / 64-row edge, three tiles, past 224, past 288
OUTS = ("ctx", "lse", "dq", "dk", "dv")


@functools.lru_cache(maxsize=None)
def case(arm, n, td, causal, seed=3):
    sl = AE.make(arm, n, seed, td, causal=causal)
    al = AE.causal_mask(n, n, causal=causal)
    R = AE.attend(sl["q"], sl["k"], sl["v"], al, sl["dctx"])
    return sl, al, R, AE.bars(R, td, exact_bf16=AE.is_bf16(sl["q"], sl["k"], sl["v"]))


def ratios(got, R, B, outs=OUTS):
    return {o: AE.worst(got[o], R[o], B[o]) for o in outs}


@pytest.mark.parametrize("td", TYPES, ids=TID.get)
@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("arm", AE.ARMS)
def test_honest_kernel_stays_inside_the_bars(arm, causal, td):
    for n in LENGTHS + ([1024] if arm == "staircase" and not causal else []):
        sl, al, R, B = case(arm, n, td, causal)
        r = ratios(AE.emulate(sl["q"], sl["k"], sl["v"], al, sl["dctx"], td), R, B)
        assert max(r.values()) < 1.0, (arm, n, causal, r)


@pytest.mark.parametrize("td", TYPES, ids=TID.get)
@pytest.mark.parametrize("arm", ["random", "negative", "match"])
def test_honest_pooled_kernel_stays_inside_the_bars(arm, td):
    """One query row (attn_pooled.hip): keys <= idx under the causal mask, all keys without."""
    n = 77
    for causal in (0, 1):
        sl = AE.make(arm, n, 5, td, causal=causal)
        for idx in (0, 1, 16, 32, n - 2, n - 1):
            al = AE.causal_mask(n, n, causal=causal)[idx:idx + 1]
            q, d = sl["q"][idx:idx + 1], sl["dctx"][idx:idx + 1]
            R = AE.attend(q, sl["k"], sl["v"], al, d)
            B = AE.bars(R, td, AE.POOLED)
            r = ratios(AE.emulate(q, sl["k"], sl["v"], al, d, td, AE.POOLED), R, B)
            assert max(r.values()) < 1.0, (arm, causal, idx, r)
            if causal:
                assert float(R["dk"][idx + 1:].abs().max() if idx + 1 < n else 0.0) == 0.0      # behind the causal limit: exact zeros in the reference too


# ---- the mutants ----------------------------------------------------------------------------------------------------------------------------------------------------
def mutant_ratio(arm, n, td, causal, outs, **kw):
    sl, al, R, B = case(arm, n, td, causal)
    al = kw.pop("allowed", al)
    M = AE.attend(sl["q"], sl["k"], sl["v"], al, sl["dctx"], **kw)
    return max(ratios(M, R, B, outs).values())


@pytest.mark.parametrize("td", TYPES, ids=TID.get)
def test_mutants_leave_the_bars_by_ten(td):
    z = torch.zeros(1, AE.HD, dtype=AE.F64)
    for n in (1, 17, 77, 213, 273):
        # a phantom zero key behind L (a zero-filled LDS row that keeps its score 0)
        assert mutant_ratio("negative", n, td, 0, ("ctx", "lse"), extra_k=z, extra_v=z) >= 10.0, n
    for n in (2, 33, 77, 213, 289):
        full = AE.causal_mask(n, n, causal=False)
        drop = full.clone()
        drop[:, -1] = False
        assert mutant_ratio("match", n, td, 0, ("ctx",), allowed=drop) >= 10.0, n                                   # the last key dropped
        w = torch.ones(n)
        w[-1] = 0.0
        assert mutant_ratio("match", n, td, 0, ("dv",), dkv_weight=w) >= 10.0, n                                    # the last query dropped in the dK / dV sums
        if n <= 288:
            for arm, shift in (("forbidden", +1), ("forbidden", -1)) + ((("match", -1),) if n >= 33 else ()):      # the causal mask shifted by one; `match` has
                assert mutant_ratio(arm, n, td, 1, ("ctx",), allowed=AE.causal_mask(n, n, shift=shift)) >= 10.0, (arm, n, shift)      # the diagonal decisive


@pytest.mark.parametrize("td", TYPES, ids=TID.get)
def test_ragged_neighbour_mutant(td):
    """A ragged sample that reads one key of its neighbour (non-causal: under the causal mask a key behind the sample's end is masked anyway).  The `negative`
    arm alternates its sign from sample to sample, so the neighbour's key scores +20 where the sample's own score -20."""
    for n in (1, 16, 33, 59):
        own, nb = AE.make("negative", n, 10, td), AE.make("negative", 4, 11, td, sign=-1.0)
        al = AE.causal_mask(n, n, causal=False)
        R = AE.attend(own["q"], own["k"], own["v"], al, own["dctx"])
        M = AE.attend(own["q"], own["k"], own["v"], al, own["dctx"], extra_k=nb["k"][:1], extra_v=nb["v"][:1])
        assert AE.worst(M["ctx"], R["ctx"], AE.bars(R, td)["ctx"]) >= 10.0, n


@pytest.mark.parametrize("td", TYPES, ids=TID.get)
def test_rows_needed_rounded_down_mutant(td):
    """rows_needed rounded DOWN to a 32-row block: the rows between stay unwritten (zeros here)."""
    n = 77
    sl, al, R, B = case("random", n, td, 1)
    for need in (1, 17, 31, 33, n - 1):
        lo = need // 32 * 32
        r = {}
        for o in ("dq", "dk", "dv"):
            got = R[o].clone()
            got[lo:] = 0.0
            r[o] = AE.worst(got[:need], R[o][:need], B[o][:need])
        assert max(r.values()) >= 10.0, (need, r)      # (dq of position 0 is 0 under the causal mask — one key —, so need = 1 shows in dv)


@pytest.mark.parametrize("td,n", [(torch.float16, 97), (torch.bfloat16, 1024), (torch.float32, 1024)], ids=["f16-97", "bf16-1024", "f32-1024"])
def test_frozen_maximum_mutant(td, n):
    """A running maximum that never moves after the first tile: scale-free while nothing overflows, so it shows where the staircase has climbed past the type's
    range — two tiles for an f16 P, 16 for f32 / bf16 (the long kernels' lengths)."""
    sl, al, R, B = case("staircase", n, td, 0)
    got = AE.emulate(sl["q"], sl["k"], sl["v"], al, sl["dctx"], td, frozen_max=True)
    assert AE.worst(got["ctx"], R["ctx"], B["ctx"]) >= 10.0


def test_phantom_key_passes_the_old_bars():
    """The hole: ONE padded key that keeps its score 0 moves ctx and lse of the existing random data at L = 213 by a few 1e-3 of max |ref| — green under the
    bf16 bars (2e-2) every attention test had, red by more than ten times under the per-element bars on the `negative` arm (test_mutants_leave_the_bars_by_ten)."""
    td, n = torch.bfloat16, 213
    sl, al, R, B = case("random", n, td, 0)
    z = torch.zeros(1, AE.HD, dtype=AE.F64)
    M = AE.attend(sl["q"], sl["k"], sl["v"], al, sl["dctx"], extra_k=z, extra_v=z)
    e_ctx, e_lse = AE.relerr(AE.rt(M["ctx"], td), R["ctx"]), AE.relerr(M["lse"], R["lse"])
    print(f"phantom key, random arm, bf16, L = 213: ctx relerr {e_ctx:.2e}, lse relerr {e_lse:.2e}")
    assert e_ctx < AE.OLD_CTX[td] and e_lse < AE.OLD_LSE[td]
    for o in ("dq", "dk", "dv"):
        assert AE.relerr(M[o], R[o]) < AE.OLD_GRAD[td], o


@pytest.mark.parametrize("td", [torch.bfloat16, torch.float16], ids=TID.get)
def test_spool_bar_and_phantom_row(td):
    """attn_stream.hip: an honest forward stays inside the derived ctx bar on both arms; a phantom zero row takes the row on the `negative` arm (every real row
    scores about -20 below it) and leaves the bar by ten times or more."""
    for L in (1, 2, 33, 225, 288):
        for arm in ("random", "negative"):
            c = AE.spool_case(arm, 2, L, 2, td)
            ref = AE.spool_reference(c, td)
            assert AE.worst(AE.spool_emulate(c, td), ref["ctx"], ref["ctx_bar"]) < 1.0, (arm, L)
        mut = AE.spool_reference(AE.spool_with_phantom(c), td)["ctx"]
        assert AE.worst(mut, ref["ctx"], ref["ctx_bar"]) >= 10.0, L
        assert AE.relerr(mut, ref["ctx"]) > 10 * 1e-2, L      # and the relerr bar of the kernel's existing test by ten times as well
