"""tests/arms.py and tests/strided.py can fail on the row-operation family: a plain torch LayerNorm forward + backward over mapped rows, a batch-row gather and a
transpose that do their own address arithmetic on the flat arenas of tests/strided.py — base offset, ldx, ldy, lddy, lddx, ldcast, ld_src, ld_dst, lds, ldd are their
arguments — with seven deliberate addressing mistakes.  The correct versions pass `check_arms` (kept = True) and the f64 reference; each mistake turns the case red with
the message it is meant to produce; and every address a mistake touches stays inside its arena (the arena sizing rule of strided.py).  No GPU."""
import pytest
import torch

import arms as A
import strided as S

B, L, P, ROW0, D = 3, 7, 2, 1, 16
ROWS = B * L
MROWS = [b * L + ROW0 + p for b in range(B) for p in range(P)]      # the rows of the stream the backward owns
TC = torch.bfloat16                                                # the cast copy: a 16-byte store is 8 elements
LDS = dict(ldx=D + 4, ldy=D + 8, lddy=D + 12, lddx=D + 16, ldcast=D + 20, ld_src=D + 24, ld_dst=D + 28, lds=D + 3, ldd=ROWS + 5)
BASE = 4
NBYTES = S.arena_bytes(ROWS, max(LDS.values()), 4, BASE)           # the largest row count, leading dimension, element size and base of the case


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


def row(r, ld, n=D):
    return r * ld + torch.arange(n)


def flat_layernorm(f, gam, ld, bug=None):
    """y = LN(x) for every row of the stream, then dx (f32, in/out) += LN'(dy) and its bf16 copy for the mapped rows: dy is compact [B P, d]."""
    ldx_fwd = ld["ldy"] if bug == "ldy for ldx" else ld["ldx"]
    ld_y_store = D if bug == "d for ld in a store" else ld["ldy"]
    ld_cast_store = ld["lddx"] if bug == "lddx for ldcast" else ld["ldcast"]
    for r in range(ROWS):
        x = f["x"].ld(row(r, ldx_fwd))
        mu, rs = x.mean(), 1 / torch.sqrt(x.var(unbiased=False) + 1e-5)
        f["mean"].st([r], mu[None]), f["rstd"].st([r], rs[None])
        f["y"].st(row(r, ld_y_store), (x - mu) * rs * gam)
    for crow, r in enumerate(MROWS):
        srow = crow if bug == "compact row for mapped row" else r
        x, g = f["x"].ld(row(srow, ld["ldx"])), f["dy"].ld(row(crow, ld["lddy"])) * gam
        mu, rs = f["mean"].ld([srow])[0], f["rstd"].ld([srow])[0]
        xh = (x - mu) * rs
        t = (g - g.mean() - xh * (g * xh).mean()) * rs + f["dx"].ld(row(srow, ld["lddx"]))
        f["dx"].st(row(srow, ld["lddx"]), t)
        f["cast"].st(row(srow, ld_cast_store), t)
        if bug == "16-byte store 8 bytes before the row's end":      # a lane owns the row's last four bf16 (8 bytes) but stores eight
            f["cast"].st(row(srow, ld_cast_store, 8) + D - 4, torch.cat([t[-4:], torch.zeros(4, dtype=torch.float64)]))


def flat_gather(f, ld, bug=None):
    ld_store = ld["ld_src"] if bug == "ld_src for ld_dst" else ld["ld_dst"]
    for crow, r in enumerate(MROWS):
        f["dst"].st(row(crow, ld_store), f["src"].ld(row(r, ld["ld_src"])))


def flat_transpose(f, ld, bug=None):
    ld_store = ld["lds"] if bug == "a transpose writing at lds" else ld["ldd"]
    for r in range(ROWS):
        f["tdst"].st(torch.arange(D) * ld_store + r, f["tsrc"].ld(row(r, ld["lds"])))


def values():
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(x=r(ROWS, D) * 2 + 0.3, dy=r(B * P, D), dx0=r(ROWS, D), gam=(1 + 0.1 * r(D)).double(), src=r(ROWS, D), tsrc=r(ROWS, D))


def build(strided):
    v = values()
    ld = LDS if strided else dict(ldx=D, ldy=D, lddy=D, lddx=D, ldcast=D, ld_src=D, ld_dst=D, lds=D, ldd=ROWS)
    base = BASE if strided else 0

    def op(rows, cols, ldname, td=torch.float32, fill=None):      # (the tight arm's arenas have the same size: a mistake must not leave them either)
        return S.operand(rows, cols, ld[ldname], td, base, NBYTES // (4 if td == torch.float32 else 2), fill, "cpu")

    def stat():
        return S.region(base + torch.arange(ROWS), torch.float32, NBYTES // 4, None, "cpu")

    ops = dict(x=op(ROWS, D, "ldx", fill=v["x"]), y=op(ROWS, D, "ldy"), mean=stat(), rstd=stat(), dy=op(B * P, D, "lddy", fill=v["dy"]),
               dx=S.must_write(S.in_out(op(ROWS, D, "lddx", fill=v["dx0"])), rows=MROWS), cast=S.must_write(op(ROWS, D, "ldcast", TC), rows=MROWS),
               src=op(ROWS, D, "ld_src", fill=v["src"]), dst=op(B * P, D, "ld_dst"), tsrc=op(ROWS, D, "lds", fill=v["tsrc"]), tdst=op(D, ROWS, "ldd"))
    return ops, {k: Flat(o, base) for k, o in ops.items()}, ld, v


def run(bug):
    """Both arms under the same (possibly wrong) address arithmetic -> the first failing assertion's text, or None; and the arms."""
    arms = []
    for strided in (True, False):
        ops, f, ld, v = build(strided)
        flat_layernorm(f, v["gam"], ld, bug)
        flat_gather(f, ld, bug)
        flat_transpose(f, ld, bug)
        arms.append((ops, f))
    try:
        A.check_arms(f"bug {bug}", arms[0][0], arms[1][0], kept=True)
    except AssertionError as e:
        return str(e), arms
    return None, arms


def test_the_correct_row_operations_pass_and_meet_the_reference():
    msg, arms = run(None)
    assert msg is None, msg
    t, v = arms[1][0], values()
    xr = v["x"].double().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xr, (D,), v["gam"], None, 1e-5)
    g = torch.zeros(ROWS, D, dtype=torch.float64)
    g[MROWS] = v["dy"].double()
    y.backward(g)
    rel = lambda got, ref: float((got.double() - ref).abs().max() / ref.abs().max())  # noqa: E731
    assert rel(t["y"].t, y.detach()) < 1e-6                                           # f32 stores of f64 arithmetic
    want = (v["dx0"].double() + xr.grad)[MROWS]
    assert rel(t["dx"].t[MROWS], want) < 1e-6 and rel(t["cast"].t[MROWS], want) < 8e-3      # ... and their bf16 rounding
    assert torch.equal(t["dst"].t, v["src"][MROWS]) and torch.equal(t["tdst"].t, v["tsrc"].t())
    assert torch.equal(t["dx"].t[0], v["dx0"][0])                                     # a row the backward does not own


@pytest.mark.parametrize("bug,how", [
    ("ldy for ldx", "the strided arm differs from the tight arm"),                        # x read at the wrong stride: other values, or a pad's NaN, in y
    ("lddx for ldcast", "cast (strided arm): "),                                          # the cast copy stored with the f32 stream's stride: pads written
    ("compact row for mapped row", "footprint elements the call does not own were written"),   # the stream touched at rows 0 .. B P - 1
    ("d for ld in a store", "y (strided arm): "),                                         # y stored tight into a strided view
    ("16-byte store 8 bytes before the row's end", "cast (strided arm): "),               # four elements too many behind every mapped row
    ("ld_src for ld_dst", "dst (strided arm): "),                                         # the gather's compact rows stored at the source's stride
    ("a transpose writing at lds", "tdst (strided arm): "),                               # dst rows at the source's stride
])
def test_each_wrong_row_operation_is_caught(bug, how):
    msg, arms = run(bug)
    assert msg is not None and how in msg, (bug, msg)
    if bug not in ("ldy for ldx", "compact row for mapped row"):
        assert "outside the operand's footprint were written" in msg, (bug, msg)
    # the sizing rule: the wrong addresses stayed inside every arena of both arms (Flat asserts it on every access; here the numbers)
    for ops, fl in arms:
        for name, f in fl.items():
            assert 0 <= f.hi < f.a.numel(), (bug, name)
    if bug in ("lddx for ldcast", "16-byte store 8 bytes before the row's end", "ld_src for ld_dst"):
        name = "dst" if bug == "ld_src for ld_dst" else "cast"
        changed = (S.bits(arms[0][0][name].arena) != arms[0][0][name].before) & ~arms[0][0][name].inside
        assert int(changed.sum()) > 0 and int(changed.nonzero().max()) < arms[0][0][name].arena.numel()

