"""tests/attn_arms.py can fail: a plain torch attention forward + backward (and a pooled backward) that does its own address arithmetic on the flat arenas of
tests/strided.py — base offset, ldqkv, ldctx, lddctx, lddqkv, the head step and the q | k | v step are its arguments — with six deliberate addressing
mistakes.  The correct version passes `check_arms` and the f64 reference; each mistake turns the case red with the message it is meant to produce; and every
address a mistake touches stays inside its arena (the arena sizing rule of strided.py, attn_arms.case_bytes).  No GPU."""
import pytest
import torch

import attn_arms as AA
import strided as S

B, L, H, HD = 2, 21, 2, 64
D, M, LP = H * HD, B * L, 32      # LP: L rounded up to the 32-row tile of the kernels
TD = torch.bfloat16               # 2-byte operands: a 16-byte store is 8 elements
LDS = dict(ldqkv=3 * D + 32, lddqkv=3 * D + 64, ldctx=D + 8, lddctx=D + 16)      # "tier1" of test_attn_strides_gpu.py
BASE = 8                          # 16 bytes


class Flat:
    """A flat arena addressed by element index from the operand's base pointer; remembers the largest address it was asked for."""

    def __init__(self, rec, base):
        self.a, self.base, self.hi = rec.arena, base, -1

    def _ix(self, idx):
        idx = self.base + torch.as_tensor(idx, dtype=torch.int64)
        self.hi = max(self.hi, int(idx.max()))
        assert int(idx.min()) >= 0 and self.hi < self.a.numel(), "an address left the arena: the sizing rule is broken"
        return idx

    def ld(self, idx):
        return self.a[self._ix(idx)].double()

    def st(self, idx, val):
        self.a[self._ix(idx)] = val.to(self.a.dtype)


def tile(rows, ld, col, n=HD):
    """element indices of an [len(rows), n] tile at column `col` of a matrix with row stride ld"""
    return torch.as_tensor(rows)[:, None] * ld + col + torch.arange(n)[None, :]


def flat_attention(f, ldqkv, ldctx, lddctx, lddqkv, hstep, vstep, bug=None):
    """softmax(q k^T / 8) v and its backward for B x H heads on the Flat arenas f = {qkv, ctx, lse, dctx, delta, dqkv}: element (row, head h, which, c) of qkv at
    row * ldqkv + h * hstep + which * vstep + c, (row, h, c) of ctx at row * ldctx + h * 64 + c, lse / delta [B, H, L]."""
    ld_ctx_store = H * HD if bug == "a" else ldctx
    ld_dqkv_store = ldqkv if bug == "b" else lddqkv
    kstep = ldqkv // 3 if bug == "c" else vstep
    lse_rows = LP if bug == "e" else L
    for b in range(B):
        for h in range(H):
            rows = b * L + torch.arange(L)
            q, k, v = f["qkv"].ld(tile(rows, ldqkv, h * hstep)), f["qkv"].ld(tile(rows, ldqkv, h * hstep + kstep)), f["qkv"].ld(tile(rows, ldqkv, h * hstep + 2 * vstep))
            s = q @ k.t() / 8.0
            p = torch.softmax(s, -1)
            o = p @ v
            f["ctx"].st(tile(rows, ld_ctx_store, h * HD), o)
            if bug == "d":      # the row's last 16-byte store starts 8 bytes before the row's end (only the last head's reaches a pad)
                over = torch.cat([o[:, -4:], torch.zeros(L, 4, dtype=torch.float64)], 1)
                f["ctx"].st(tile(rows, ld_ctx_store, h * HD + HD - 4, 8), over)
            lse = torch.logsumexp(s, -1)
            f["lse"].st((b * H + h) * L + torch.arange(lse_rows), torch.cat([lse, torch.zeros(lse_rows - L, dtype=torch.float64)]))
    for b in range(B):
        for h in range(H):
            rows = b * L + torch.arange(L)
            q, k, v = f["qkv"].ld(tile(rows, ldqkv, h * hstep)), f["qkv"].ld(tile(rows, ldqkv, h * hstep + kstep)), f["qkv"].ld(tile(rows, ldqkv, h * hstep + 2 * vstep))
            o, do = f["ctx"].ld(tile(rows, ldctx, h * HD)), f["dctx"].ld(tile(rows, lddctx, h * HD))
            p = torch.exp(q @ k.t() / 8.0 - f["lse"].ld((b * H + h) * L + torch.arange(L))[:, None])
            delta = (o * do).sum(1)
            f["delta"].st((b * H + h) * L + torch.arange(L), delta)
            ds = p * (do @ v.t() - delta[:, None]) / 8.0
            for which, g in enumerate((ds @ k, ds.t() @ q, p.t() @ do)):
                f["dqkv"].st(tile(rows, ld_dqkv_store, h * hstep + which * vstep), g)


def flat_pooled_bwd(f, ldqkv, lddctx, lddqkv, bug=None):
    """The pooled form's backward for query row 0 of every sample (non-causal): dK, dV into columns d..3d of all L rows; the q columns stay untouched."""
    for b in range(B):
        for h in range(H):
            rows = b * L + torch.arange(L)
            q = f["qkv"].ld(tile(rows[:1], ldqkv, h * HD))
            k, v = f["qkv"].ld(tile(rows, ldqkv, D + h * HD)), f["qkv"].ld(tile(rows, ldqkv, 2 * D + h * HD))
            do = f["dctx"].ld(tile(rows[:1], lddctx, h * HD))
            p = torch.softmax(q @ k.t() / 8.0, -1)
            dp = do @ v.t()
            ds = p * (dp - (p * dp).sum()) / 8.0
            f["dqkv"].st(tile(rows, lddqkv, D + h * HD), ds.t() @ q)
            f["dqkv"].st(tile(rows, lddqkv, 2 * D + h * HD), p.t() @ do)
            if bug == "f":
                f["dqkv"].st(tile(rows, lddqkv, h * HD), torch.zeros(L, HD, dtype=torch.float64))


def values():
    g = torch.Generator().manual_seed(5)
    return (torch.randn(M, 3 * D, generator=g) * 0.7).to(TD), torch.randn(M, D, generator=g).to(TD)


def build(strided, pooled=False):
    """-> ({name: Record}, {name: Flat}, the leading dimensions) of one arm; every arena has case_bytes() bytes."""
    qkv, dctx = values()
    ld = LDS if strided else dict(ldqkv=3 * D, lddqkv=3 * D, ldctx=D, lddctx=D)
    base = BASE if strided else 0
    nbytes = AA.case_bytes(M, LDS.values(), [BASE])

    def op(cols, ldname, fill=None, col=0):      # (the tight arm's arenas have the same size: a mistake must not leave them either)
        return S.operand(M, cols, ld[ldname], TD, base + col, nbytes // 2, fill, "cpu")

    def stat():
        return S.region(base + torch.arange(B * H * L), torch.float32, nbytes // 4, None, "cpu")

    if pooled:      # dqkv's footprint is the K and V columns: the q columns are pads
        ops = dict(qkv=op(3 * D, "ldqkv", qkv), dctx=op(D, "lddctx", dctx), dqkv=op(2 * D, "lddqkv", None, D))
    else:
        ops = dict(qkv=op(3 * D, "ldqkv", qkv), dctx=op(D, "lddctx", dctx), ctx=op(D, "ldctx"), lse=stat(), delta=S.must_write(stat(), none=True), dqkv=op(3 * D, "lddqkv"))
    return ops, {k: Flat(o, base) for k, o in ops.items()}, ld


def reference(qkv, dctx):
    x = qkv.double().requires_grad_(True)
    q, k, v = x.reshape(B, L, 3, H, HD).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / 8.0
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(M, D)
    o.backward(dctx.double())
    return o.detach(), torch.logsumexp(s, -1).detach(), x.grad


def run(bug, pooled=False):
    """Both arms under the same (possibly wrong) address arithmetic -> the first failing assertion's text, or None; and the arenas' largest addresses."""
    arms = []
    for strided in (True, False):
        ops, f, ld = build(strided, pooled)
        if pooled:
            flat_pooled_bwd(f, ld["ldqkv"], ld["lddctx"], ld["lddqkv"], bug)
        else:
            flat_attention(f, ld["ldqkv"], ld["ldctx"], ld["lddctx"], ld["lddqkv"], HD, D, bug)
        arms.append((ops, f))
    try:
        AA.check_arms(f"bug {bug}", arms[0][0], arms[1][0])
    except AssertionError as e:
        return str(e), arms
    return None, arms


def test_the_correct_attention_passes_and_meets_the_reference():
    msg, arms = run(None)
    assert msg is None, msg
    ti = arms[1][0]
    qkv, dctx = values()
    o, lse, g = reference(qkv, dctx)
    rel = lambda got, ref: float((got.double() - ref).abs().max() / ref.abs().max())  # noqa: E731
    assert rel(ti["ctx"].t, o) < 2e-2 and rel(ti["dqkv"].t, g) < 4e-2      # bf16 stores of exact f64 arithmetic
    assert rel(ti["lse"].arena[ti["lse"].inside].reshape(B, H, L), lse) < 1e-5
    msg, _ = run(None, pooled=True)
    assert msg is None, msg


@pytest.mark.parametrize("bug,pooled,how", [
    ("a", False, "ctx (strided arm): "),                                     # ctx stored with H*64 as the row stride: pads written
    ("b", False, "dqkv (strided arm): "),                                    # dqkv stored with ldqkv
    ("c", False, "the strided arm differs from the tight arm"),              # k columns taken at ldqkv / 3: other values, or a pad's NaN, in every output
    ("d", False, "ctx (strided arm): "),                                     # a 16-byte store over the row's end
    ("e", False, "lse (strided arm): "),                                     # lse written for Lp rows: behind [B, H, L]
    ("f", True, "dqkv (strided arm): "),                                     # the pooled backward writes the q columns
])
def test_each_wrong_attention_is_caught(bug, pooled, how):
    msg, arms = run(bug, pooled)
    assert msg is not None and how in msg, (bug, msg)
    if bug != "c":
        assert "outside the operand's footprint were written" in msg, (bug, msg)
    # the sizing rule: the wrong addresses stayed inside every arena of both arms (Flat asserts it on every access; here the strided arm's numbers)
    for name, f in arms[0][1].items():
        assert 0 <= f.hi < f.a.numel(), name
    if bug in "ade":
        f = arms[0][1]["ctx" if bug != "e" else "lse"]
        inside = arms[0][0]["ctx" if bug != "e" else "lse"].inside.nonzero()
        assert (f.hi > int(inside.max())) == (bug != "a")      # d, e ran over the footprint's end and still inside the arena; a wrote between the rows


def test_may_be_written_rows_are_neither_pads_nor_musts():
    """strided.must_write: rows behind `rows_needed` may be written or left; rows before it must be written; delta (nothing must) is held to its pads alone."""
    n = AA.case_bytes(M, [D + 8], [BASE]) // 2
    for wrote in (5, M):
        o = S.must_write(S.operand(M, D, D + 8, TD, BASE, n), 5)
        o.t[:wrote] = 1.0
        S.check_pads("o", o), S.check_written("o", o)
        assert int(o.must.sum()) == 5 * D
    o = S.must_write(S.operand(M, D, D + 8, TD, BASE, n), [0, 1, 2, 30, 31])      # the first rows of two samples
    o.t[:3] = 1.0
    with pytest.raises(AssertionError, match="never written"):
        S.check_written("o", o)
    o.t[30:32] = 1.0
    S.check_written("o", o)
    o.arena[BASE + D] = 1.0
    with pytest.raises(AssertionError, match="outside the operand's footprint"):
        S.check_pads("o", o)
    d = S.must_write(S.region(BASE + torch.arange(B * H * L), torch.float32, n // 2), none=True)
    S.check_written("delta", d), S.check_pads("delta", d)
    d.arena[BASE + B * H * L] = 0.0
    with pytest.raises(AssertionError, match="outside the operand's footprint"):
        S.check_pads("delta", d)
