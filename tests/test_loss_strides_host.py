"""tests/arms.py and tests/strided.py can fail on the loss / prompt / k-means / interaction family: plain torch restatements of the address arithmetic of five of its kernels
— the contrastive loss's column log-sum-exp and gradient (ld, lddl), a k-means column pass in column blocks (ldx, an E tail), the interaction backward's two row
gradients (ldgv, ldgt, lddv, lddt, cleared first), the two-stack `t` pass of the prompt backward (both stacks' rows in one grid) — on the flat arenas of tests/strided.py,
with six deliberate addressing mistakes typical of the family.  The correct versions pass `check_arms` and the f64 reference; each mistake turns the case red with the
message it is meant to produce; and every address a mistake touches stays inside its arena (the arena sizing rule of strided.py).  No GPU."""
import pytest
import torch

import arms as A
import strided as S

N, E, BLK = 5, 11, 8                 # the loss matrix is N x N; E columns walked in blocks of BLK (the kernels: 64): a tail of 3
DV, DT, ROWS, R = 6, 9, 3, 2         # interaction widths; the prompt backward: ROWS = Lyr P rows per stack, rank R
LDS = dict(ld=N + 1, lddl=N + 3, ldx=E + 3, ldgv=DV + 9, ldgt=DT + 11, lddv=DV + 13, lddt=DT + 15)
BASE = 3
NBYTES = S.arena_bytes(2 * ROWS, max(LDS.values()), 4, BASE)      # the largest row count (the two-stack grid's 2 ROWS > N), leading dimension and base of the case


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


def flat_clip(f, ld, bug):
    """col_lse[j] = logsumexp_i x[i, j] (a column walk); dlogits[i, j] = softmax_col(x)[i, j] at lddl"""
    ld_walk = N if bug == "n for ld in a column walk" else ld["ld"]
    ld_store = ld["ld"] if bug == "ld for lddl" else ld["lddl"]
    cols = torch.stack([f["x"].ld(torch.arange(N) * ld_walk + j) for j in range(N)])      # [j, i]
    lse = torch.logsumexp(cols, 1)
    f["col_lse"].st(torch.arange(N), lse)
    for i in range(N):
        row = f["x"].ld(i * ld["ld"] + torch.arange(N))
        f["dlogits"].st(i * ld_store + torch.arange(N), torch.exp(row - lse))


def flat_colstats(f, ld, bug):
    """colsum[e] = sum_i x[i, e], in blocks of BLK columns: the last block is partial"""
    for b in range(0, E, BLK):
        e = b + torch.arange(min(BLK, E - b))
        s = torch.stack([f["X"].ld(i * ld["ldx"] + e) for i in range(N)]).sum(0)
        if bug == "a column tail written past E":      # the loads are guarded (a lane behind E adds nothing), the store is not
            e, s = b + torch.arange(BLK), torch.cat([s, torch.zeros(BLK - len(e), dtype=torch.float64)])
        f["colsum"].st(e, s)


def flat_interact_bwd(f, ld, bug):
    """dxv / dxt cleared (one 2-D memset each), then dxv += 2 g_out_v, dxt += 3 g_out_t: the kernels' accumulation into a cleared strided footprint"""
    if bug == "a memset of N*Dv contiguous floats on a strided dxv":
        f["dxv"].st(torch.arange(N * DV), torch.zeros(N * DV))
    else:
        for n in range(N):
            f["dxv"].st(n * ld["lddv"] + torch.arange(DV), torch.zeros(DV))
    ld_t = ld["lddv"] if bug == "lddv for lddt" else ld["lddt"]
    for n in range(N):
        f["dxt"].st(n * ld_t + torch.arange(DT), torch.zeros(DT))
    for n in range(N):
        iv, it = n * ld["lddv"] + torch.arange(DV), n * ld_t + torch.arange(DT)
        f["dxv"].st(iv, f["dxv"].ld(iv) + 2 * f["gv"].ld(n * ld["ldgv"] + torch.arange(DV)))
        f["dxt"].st(it, f["dxt"].ld(it) + 3 * f["gt"].ld(n * ld["ldgt"] + torch.arange(DT)))


def flat_t2(f, bug):
    """t[row, k] = sum_d dout[row, d] d3[d, k] for both stacks in ONE grid of 2 ROWS rows: rows [ROWS, 2 ROWS) are the textual stack's rows [0, ROWS)"""
    for row in range(2 * ROWS):
        vis = row < ROWS
        rr = row if vis or bug == "the second stack's rows indexed without - rows" else row - ROWS
        D, dout, d3, t = (DV, f["doutv"], f["d3v"], f["tv"]) if vis else (DT, f["doutt"], f["d3t"], f["tt"])
        g = dout.ld(rr * D + torch.arange(D))
        w = torch.stack([d3.ld(torch.arange(D) * R + k) for k in range(R)])
        t.st(rr * R + torch.arange(R), w @ g)


def values():
    g = torch.Generator().manual_seed(11)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(x=r(N, N) * 3, X=r(N, E), gv=r(N, DV), gt=r(N, DT), doutv=r(ROWS, DV), doutt=r(ROWS, DT), d3v=r(DV, R), d3t=r(DT, R))


def build(strided):
    v = values()
    ld = LDS if strided else dict(ld=N, lddl=N, ldx=E, ldgv=DV, ldgt=DT, lddv=DV, lddt=DT)
    base = BASE if strided else 0

    def op(rows, cols, ldname=None, fill=None):      # ldname None: a dense operand (ld = cols in both arms, the base offset in the strided one); the tight arm's arenas have the same size
        return S.operand(rows, cols, ld[ldname] if ldname else cols, torch.float32, base, NBYTES // 4, fill, "cpu")
    ops = dict(x=op(N, N, "ld", v["x"]), col_lse=op(1, N), dlogits=op(N, N, "lddl"), X=op(N, E, "ldx", v["X"]), colsum=op(1, E),
               gv=op(N, DV, "ldgv", v["gv"]), gt=op(N, DT, "ldgt", v["gt"]), dxv=op(N, DV, "lddv"), dxt=op(N, DT, "lddt"),
               doutv=op(ROWS, DV, None, v["doutv"]), doutt=op(ROWS, DT, None, v["doutt"]), d3v=op(DV, R, None, v["d3v"]), d3t=op(DT, R, None, v["d3t"]),
               tv=op(ROWS, R), tt=op(ROWS, R))
    return ops, {k: Flat(o, base) for k, o in ops.items()}, ld, v


def run(bug):
    """Both arms under the same (possibly wrong) address arithmetic -> the first failing assertion's text, or None; and the arms."""
    arms = []
    for strided in (True, False):
        ops, f, ld, _ = build(strided)
        flat_clip(f, ld, bug), flat_colstats(f, ld, bug), flat_interact_bwd(f, ld, bug), flat_t2(f, bug)
        arms.append((ops, f))
    try:
        A.check_arms(f"bug {bug}", arms[0][0], arms[1][0])
    except AssertionError as e:
        return str(e), arms
    return None, arms


def test_the_correct_address_arithmetic_passes_and_meets_the_reference():
    msg, arms = run(None)
    assert msg is None, msg
    t, v = arms[1][0], {k: x.double() for k, x in values().items()}
    rel = lambda got, ref: float((got.double() - ref).abs().max() / ref.abs().max())  # noqa: E731
    assert rel(t["col_lse"].t[0], torch.logsumexp(v["x"], 0)) < 1e-6 and rel(t["dlogits"].t, torch.softmax(v["x"], 0)) < 1e-6      # f32 stores of f64 arithmetic
    assert rel(t["colsum"].t[0], v["X"].sum(0)) < 1e-6
    assert torch.equal(t["dxv"].t, 2 * values()["gv"]) and torch.equal(t["dxt"].t, 3 * values()["gt"])
    assert rel(t["tv"].t, v["doutv"] @ v["d3v"]) < 1e-6 and rel(t["tt"].t, v["doutt"] @ v["d3t"]) < 1e-6


@pytest.mark.parametrize("bug,how", [
    ("ld for lddl", "dlogits (strided arm): "),                                            # the gradient stored at the logits' stride: pads written
    ("n for ld in a column walk", "col_lse: the strided arm differs from the tight arm"),  # other rows' values, or a pad's NaN, in a column's log-sum-exp
    ("lddv for lddt", "dxt (strided arm): "),                                              # the textual gradient rows at the visual stride
    ("a memset of N*Dv contiguous floats on a strided dxv", "dxv (strided arm): "),        # the pads between the first rows cleared, the last rows never
    ("a column tail written past E", "colsum (strided arm): "),                            # a whole column block stored where the last one is partial
    ("the second stack's rows indexed without - rows", "tt (strided arm): 6 of 6 output elements were never written"),      # the textual t rows land behind tt's end
])
def test_each_wrong_address_is_caught(bug, how):
    msg, arms = run(bug)
    assert msg is not None and how in msg, (bug, msg)
    quiet = ("n for ld in a column walk", "the second stack's rows indexed without - rows")
    # (the second: what lands behind tt's end was computed from doutt's pads, NaN with the pad's own payload, so those pads keep their bits; tt itself stays unwritten)
    if bug not in quiet:
        assert "outside the operand's footprint were written" in msg, (bug, msg)
    # the sizing rule: the wrong addresses stayed inside every arena of both arms (Flat asserts it on every access; here the numbers)
    for ops, fl in arms:
        for name, f in fl.items():
            assert 0 <= f.hi < f.a.numel(), (bug, name)
    if bug not in quiet:
        name = how.split(" ")[0]
        rec = arms[0][0][name]
        changed = (S.bits(rec.arena) != rec.before) & ~rec.inside
        assert int(changed.sum()) > 0 and int(changed.nonzero().max()) < rec.arena.numel()
    if bug == "a memset of N*Dv contiguous floats on a strided dxv":      # ... and the rows the contiguous memset never reached still hold NaN: the second thing that would show
        assert bool(torch.isnan(arms[0][0]["dxv"].t[-1]).all())
