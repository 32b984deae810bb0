"""tests/strided.py can fail: a plain numpy "GEMM with explicit leading dimensions" with four deliberate addressing mistakes, each of which the
helper's checks (or a NaN in the result) catch, and the correct call, which passes them; 1-byte operands (MX-FP8 bytes); rows a call must leave alone.  No GPU."""
import numpy as np
import pytest
import torch

import strided as S

M, N, K = 8, 16, 24
LDA, LDB, LDC, LDR = K + 16, K + 32, N + 4, N + 12      # all different from each other and from the widths; ldc = N + 4: an 8-byte row end (fp16)
COL0 = 8                                                 # 16 bytes of fp16


def np_gemm(a, lda, b, ldb, c, ldc, r, ldr, bug=None):
    """C[M, N] = A[M, K] . B[N, K]^T + R[M, N] on FLAT arrays that start at each operand's first element.  bug: one of the four mistakes."""
    ld_a = K if bug == "K for lda" else lda
    ld_c = ldr if bug == "ldr for C" else ldc
    ld_r = ldc if bug == "ldc for the residual" else ldr
    bm = np.stack([b[n * ldb:n * ldb + K] for n in range(N)]).astype(np.float64)
    for m in range(M):
        row = bm @ a[m * ld_a:m * ld_a + K].astype(np.float64) + r[m * ld_r:m * ld_r + N].astype(np.float64)
        if bug == "16-byte store":      # a lane owns four columns (8 bytes of fp16) but stores 16 bytes: the last group of a row runs 8 bytes over its end
            for j in range(0, N, 4):
                c[m * ld_c + j:m * ld_c + j + 8] = np.concatenate([row[j:j + 4], np.zeros(4)]).astype(c.dtype)
        else:
            c[m * ld_c:m * ld_c + N] = row.astype(c.dtype)


def run(bug):
    g = torch.Generator().manual_seed(1)
    av, bv, rv = (torch.randn(M, K, generator=g).half(), torch.randn(N, K, generator=g).half(), torch.randn(M, N, generator=g).half())
    elems = S.arena_bytes(max_rows=max(M, N), max_ld=max(LDA, LDB, LDC, LDR), max_esz=2, col0=COL0) // 2
    ops = dict(A=S.operand(M, K, LDA, torch.float16, COL0, elems, av), B=S.operand(N, K, LDB, torch.float16, COL0, elems, bv),
               R=S.operand(M, N, LDR, torch.float16, COL0, elems, rv), C=S.operand(M, N, LDC, torch.float16, COL0, elems))
    flat = {k: o.arena.numpy()[COL0:] for k, o in ops.items()}      # shares the arena's memory
    np_gemm(flat["A"], LDA, flat["B"], LDB, flat["C"], LDC, flat["R"], LDR, bug)
    ref = av.double() @ bv.double().t() + rv.double()
    return ops, ref


def caught(ops, ref):
    """The GPU tests' assertions: pads intact on every operand, every output element written, no NaN, the reference met.  -> the first that fails."""
    try:
        for k, o in ops.items():
            S.check_pads(k, o)
        S.check_written("C", ops["C"])
    except AssertionError as e:
        return str(e)
    got = ops["C"].t.double()
    if bool(torch.isnan(got).any()):
        return "NaN in the result"
    if float((got - ref).abs().max()) > 2e-3 * float(ref.abs().max()):
        return "reference missed"
    return None


def test_operand_layout():
    elems = S.arena_bytes(M, LDC, 4, col0=8) // 4
    o = S.operand(M, N, LDC, torch.float32, 4, elems)
    assert o.t.shape == (M, N) and o.t.stride() == (LDC, 1) and o.t.data_ptr() == o.arena.data_ptr() + 16
    raw = S.bits(o.arena)
    assert int(o.inside.sum()) == M * N and bool((raw[o.inside] == S.UNWRITTEN[torch.float32]).all()) and bool((raw[~o.inside] == S.PAD[torch.float32]).all())
    assert bool(torch.isnan(o.arena).all()) and S.PAD[torch.float32] != S.UNWRITTEN[torch.float32]
    vals = torch.arange(M * N, dtype=torch.float32).reshape(M, N)
    i = S.operand(M, N, LDC, torch.bfloat16, 8, 2 * elems, vals)
    assert torch.equal(i.t.float(), vals.bfloat16().float()) and bool(torch.isnan(i.arena[~i.inside]).all()) and i.arena[8] == 0 and i.arena[8 + LDC] == N
    with pytest.raises(AssertionError):      # an arena that is not sized for the view
        S.operand(M, N, LDC, torch.float32, 4, 4 + (M - 1) * LDC + N - 1)
    with pytest.raises(AssertionError):      # "never written" is visible
        S.check_written("C", o)
    o.arena[0] = 1.0
    with pytest.raises(AssertionError):      # ... and so is a write in front of the view
        S.check_pads("C", o)


def test_the_correct_gemm_passes():
    ops, ref = run(None)
    assert caught(ops, ref) is None


@pytest.mark.parametrize("bug,how", [("ldr for C", "outside the operand's footprint"), ("ldc for the residual", "NaN in the result"), ("K for lda", "NaN in the result"),
                                     ("16-byte store", "outside the operand's footprint")])
def test_each_wrong_gemm_is_caught(bug, how):
    ops, ref = run(bug)
    msg = caught(ops, ref)
    assert msg is not None and how in msg, (bug, msg)


def test_one_byte_operands_and_kept_rows():
    """strided.py on torch.uint8 (the MX-FP8 element and scale bytes): PAD 0x7F, UNWRITTEN 0xFF, compared as bytes; in_out + check_kept on the rows a call does not own."""
    n = S.arena_bytes(13, 168, 4, 4)
    q = S.operand(13, 160, 168, torch.uint8, 4, n)
    assert q.t.dtype == torch.uint8 and q.t.stride() == (168, 1) and q.t.data_ptr() == q.arena.data_ptr() + 4
    assert bool((q.arena[q.inside] == 0xFF).all()) and bool((q.arena[~q.inside] == 0x7F).all())
    with pytest.raises(AssertionError, match="never written"):
        S.check_written("q", q)
    q.t[:] = 0x38
    q.t[3, 5] = 0x7F      # an element byte that equals PAD is a written value like any other
    S.check_written("q", q), S.check_pads("q", q)
    q.arena[4 + 160] = 0
    with pytest.raises(AssertionError, match="outside the operand's footprint"):
        S.check_pads("q", q)
    sc = S.operand(13, 5, 8, torch.uint8, 3, n, torch.full((13, 5), 127, dtype=torch.uint8))
    assert not sc.output and bool((sc.t == 127).all())
    sc.t[0, 0] = 126
    with pytest.raises(AssertionError, match="an input operand was written"):
        S.check_pads("scales", sc)
    vals = torch.arange(13 * 8, dtype=torch.float32).reshape(13, 8)
    s = S.must_write(S.in_out(S.operand(13, 8, 12, torch.float32, 4, n // 4, vals)), rows=[2, 5])
    s.t[2] += 1
    s.t[5] += 1
    S.check_pads("stream", s), S.check_written("stream", s), S.check_kept("stream", s)
    s.t[6, 0] = -1.0
    with pytest.raises(AssertionError, match="does not own"):
        S.check_kept("stream", s)


def test_int32_operands_carry_sentinels_no_label_rank_or_index_can_equal():
    """strided.py on torch.int32 (labels, ranks, top-k indices, the `changed` flag): PAD and UNWRITTEN are negative, differ from each other, from -1 (the padding of a
    ground-truth list) and from 0x7fffffff (the rank of a row without ground truth); a written 0 counts as written; pads and inputs are compared as integers."""
    pad, unw = S.PAD[torch.int32], S.UNWRITTEN[torch.int32]
    assert pad < -1 and unw < -1 and pad != unw and -2 ** 31 <= min(pad, unw) and 0x7fffffff not in (pad, unw)
    n = S.arena_bytes(7, 8, 4, 3) // 4
    lab = S.operand(7, 1, 1, torch.int32, 3, n)
    assert lab.t.dtype == torch.int32 and lab.t.data_ptr() == lab.arena.data_ptr() + 12
    assert bool((lab.arena[lab.inside] == unw).all()) and bool((lab.arena[~lab.inside] == pad).all())
    with pytest.raises(AssertionError, match="never written"):
        S.check_written("labels", lab)
    lab.t[:, 0] = torch.tensor([0, 1, 0, 4, 0x7fffffff, -1, 2], dtype=torch.int32)
    S.check_written("labels", lab), S.check_pads("labels", lab)
    lab.arena[3 + 7] = 0      # one label too many
    with pytest.raises(AssertionError, match="outside the operand's footprint"):
        S.check_pads("labels", lab)
    gt = S.operand(7, 2, 5, torch.int32, 1, n, torch.tensor([[3, -1]] * 7, dtype=torch.int32))
    assert not gt.output and bool((gt.t[:, 1] == -1).all()) and gt.arena[1 + 2] == pad
    gt.t[2, 1] = 4
    with pytest.raises(AssertionError, match="an input operand was written"):
        S.check_pads("gt", gt)
    flag = S.in_out(S.region(torch.tensor([3]), torch.int32, n, torch.tensor([0], dtype=torch.int32)))
    S.check_written("changed", flag), S.check_pads("changed", flag), S.check_kept("changed", flag)      # a flag left at 0 is a value, not "unwritten"
    S.must_write(flag, none=True)
    flag.arena[3] = 1
    with pytest.raises(AssertionError, match="does not own"):
        S.check_kept("changed", flag)
