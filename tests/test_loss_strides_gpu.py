"""The loss / prompt / k-means / ranking / interaction family (loss.hip, interact.hip) held to its leading dimensions, its write bounds and its edges on a real MI355X:
lpi_clip_loss_fwd_bwd / _local_grad / _local, lpi_ce_rows_fwd_bwd, lpi_sum_scaled, lpi_prompt_cp_fwd / _bwd / _fwd2 / _bwd2, lpi_align_loss_fwd_bwd(2),
lpi_nt_bxent_fwd_bwd, the four lpi_kmeans_* passes, lpi_l1_task_id, lpi_retrieval_rank, lpi_topk, lpi_interact_fwd / _bwd (raw, ten leading dimensions), lpi_sgd_step.

Every case is an OP: a function that builds its operands on an `Arm` and returns (run, check).  It runs twice: the STRIDED arm on tests/strided.py views (base pointer 1 or 3
elements into its arena, every leading dimension of the case width + 1, + 3, + 5, ... — these kernels move one f32 per lane, so odd steps are legal —, NaN in every pad,
large negative integers in the pads of int32 operands), the TIGHT arm on contiguous copies.  Dense operands (factors, keys, centres, scratch, statistics) live in arenas
too: base offset, pads behind their end.  Asserted per case (tests/arms.py; tests/test_loss_strides_host.py proves that these assertions catch a wrong address):
  * the launch count, the same in both arms;
  * every must-be-written output of the strided arm equals the tight arm's bit for bit; no pad of any operand, inputs included, changed; every must-be-written
    element was written (scratch has no must-be-written part: only its pads are checked);
  * the tight arm meets an f64 reference of the operation.
Every arena of a case has strided.arena_bytes(largest row count, largest leading dimension, 4 bytes, base) bytes, so a kernel that applies any stride of the case to any
pointer of the case fails an assertion and never leaves an allocation.

Bars.  Where the kernel's existing test has a bar it is used and named at the constant below (the two-stack prompt backward: the per-stack bar AND, for the four
gradients no existing test holds to f64, the derived one).  Where there is none the bar is derived per output element from the f64
reference: a fixed-order f32 sum of m addends is held to (m + 2) 2^-23 sum |addend| (`sum_bar`).  The INTEGER arm runs the k-means passes, lpi_l1_task_id, the rank /
top-k kernels and the prompt kernels on integer-valued data (-3 .. 3), where every f32 sum is exact: equality with the integer reference, which decides the tie rules
(first minimum, lower task, later index) without a margin; a centre mean, the quotient of two exact integers, to 1 ulp.  Every figure is printed beside its bar
(pytest -s); the last test prints the worst per bar.

What this file found (fixed in loss.hip with it): lpi_prompt_cp_bwd2's g1 differed from the per-stack launches in the last bit at r = 3 (an FMA contracted in one
kernel and not in the other); lpi_align_loss_fwd_bwd's value without gradient buffers differed in the last bit from the value with them and from the two-launch form
(another summation order of the row means at D > 64).

lpi_nt_bxent_fwd_bwd at D = 1: every cosine is +-1 whatever X holds, so the true gradient is identically zero and an error relative to max |reference| has no scale
there; with accumulate = 0 the overwritten dx_row is held to the same relative bar on the scale of the two cancelling addends the kernel forms it from (an absolute
bound from the f64 reference's dL/dcos, see op_task_loss); with accumulate = 1 the reference is the prefilled dx_row.  lpi_kmeans_update's "counts is written once": counts has exactly k values, all
written, exact, nothing behind them (the column-chunk-0 blocks own them; a second chunk writing them too would show only as a race, not asserted here).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import arms as A  # noqa: E402
import strided as S  # noqa: E402
from lpi_amd import _lib  # noqa: E402
from lpi_amd._lib import call  # noqa: E402
from poison import relerr, same_bits  # noqa: E402

DEV = "cuda:0"
I32 = torch.int32
U = 2.0 ** -23
# The bars, each from the existing test of the kernel (relerr = max |got - ref| / max |ref|, tests/poison.py; "loss" bars: |got - ref| < bar max(1, |ref|)):
CLIP_LOSS_BAR, CLIP_GRAD_BAR = 1e-5, 5e-5       # tests/test_kernels_gpu.py test_clip_loss (loss and logits 1e-5: the lse vectors are held to it too; gradients 5e-5)
CE_LOSS_BAR, CE_GRAD_BAR = 2e-5, 2e-4           # tests/test_dead_memory_gpu.py test_ce_rows_reads_inside_n_and_writes_inside_its_block (test_clip_loss_modes_of_gather_features)
CP_OUT_BAR, CP_GRAD_BAR = 1e-6, 1e-5            # tests/test_kernels_gpu.py test_prompt_cp_fwd_bwd; the shared factor of the two-stack form: tests/test_round4_gpu.py
ALIGN_LOSS_BAR, ALIGN_GRAD_BAR = 2e-5, 5e-5     # tests/test_kernels_gpu.py test_align_loss
TASK_LOSS_BAR, TASK_GRAD_BAR = 1e-5, 1e-4       # tests/test_kernels_gpu.py test_nt_bxent_task_loss
INTERACT_OUT_BAR, INTERACT_GRAD_BAR = 2e-5, 1e-4   # tests/test_plugin_gpu.py test_interact_kernels_vs_f64 (outputs: the statistics are held to it too; every gradient)
SGD_BAR = 1e-6                                  # tests/test_kernels_gpu.py test_sgd_step_kernel_matches_torch_sgd: max |p - p_ref|
L1_DIST_CAP = 1e-3                              # tests/test_kernels_gpu.py test_l1_task_id_kernel: the derived bar is never looser than this
WORST = {}                                      # what -> (worst figure, bar): printed by the last test


def stream():
    return torch.cuda.current_stream().cuda_stream


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def ints(*shape, seed=0):
    return torch.randint(-3, 4, shape, generator=torch.Generator().manual_seed(seed)).float()


def note(what, e, bar):
    print(f"{what}: {e:.3e} (bar {bar:g})")
    WORST[what] = (max(e, WORST.get(what, (0.0, bar))[0]), bar)


def held(what, got, ref, bar):
    """relerr beside ITS bar (pytest -s shows it), then assert."""
    e = relerr(got, ref)
    note(what, e, bar)
    assert e < bar, (what, e, bar)


def held_loss(what, got, ref, bar):
    e = abs(float(got.reshape(-1)[0]) - float(ref)) / max(1.0, abs(float(ref)))
    note(what, e, bar)
    assert e < bar, (what, e, bar)


def held_abs(what, got, ref, bar):
    e = float((got.double().cpu() - ref.double().cpu()).abs().max())
    note(what, e, bar)
    assert e < bar, (what, e, bar)


def sum_bar(m, sum_abs):
    """A fixed-order f32 sum of m addends: (m + 2) 2^-23 sum |addend|, per output element, from the f64 reference."""
    return (m + 2) * U * sum_abs.double()


def held_elem(what, got, ref, bar):
    """Per-element bars (a tensor): the worst |got - ref| / bar is printed as a fraction of 1; where the bar is 0 the value must be exact."""
    err, bar = (got.double().cpu() - ref.double().cpu()).abs(), bar.double().cpu().expand_as(ref)
    frac = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    e = float(frac.max())
    note(what + " (fraction of the derived bar)", e, 1.0)
    assert e <= 1.0, (what, e)


def exact(what, got, ref):
    got, ref = got.cpu(), ref.cpu()
    assert got.shape == ref.shape and bool((got.double() == ref.double()).all()), (what, int((got.double() != ref.double()).sum()), "values differ")


class Arm:
    """One arm's operands as strided.Records: .ops[name].  `mat` takes the STRIDED arm's leading dimension (None: a dense operand, ld = cols in both arms); the tight arm
    gets ld = cols, base 0.  Every arena has strided.arena_bytes(max_rows, max_ld, 4, base) bytes: `mat` refuses an operand the sizing did not count."""

    def __init__(self, strided, max_rows, max_ld, base):
        self.strided, self.max_rows, self.max_ld, self.base, self.ops, self.keep = strided, max_rows, max_ld, base, {}, []
        self.nelem = S.arena_bytes(max_rows, max_ld, 4, base) // 4

    def ld(self, cols, ld):
        return ld if self.strided else cols

    def mat(self, name, rows, cols, ld=None, fill=None, in_out=False, td=torch.float32, none=False, keep=False):
        """none: contents unspecified (scratch): only the pads are checked.  keep: the call must leave the whole footprint alone (strided.check_kept)."""
        lds = cols if ld is None else ld
        assert rows <= self.max_rows and cols <= lds <= self.max_ld and name not in self.ops, (name, rows, cols, lds)
        if fill is not None:
            fill = fill.reshape(rows, cols)
        rec = S.operand(rows, cols, self.ld(cols, lds), td, self.base if self.strided else 0, self.nelem, fill, DEV)
        if in_out:
            S.in_out(rec)
        if none or keep:
            S.must_write(rec, none=True)
        if keep:
            self.keep.append(name)
        self.ops[name] = rec
        return rec.t

    def flat(self, name, n, none=False):
        """an output vector of n floats that is no matrix (the interaction's `grads` and workspace): a strided.region at the base, anywhere inside the case's arena size"""
        base = self.base if self.strided else 0
        assert base + n <= self.nelem and name not in self.ops, (name, n)
        rec = S.region(base + torch.arange(n), torch.float32, self.nelem, None, DEV)
        if none:
            S.must_write(rec, none=True)
        self.ops[name] = rec
        return rec.t[base:base + n]

    def got(self, name):
        rec = self.ops[name]
        return (rec.t if rec.t.dim() == 2 else rec.arena[rec.inside]).cpu()


def run_arms(label, op, max_rows, max_ld, base, launches, **kw):
    """op(arm, **kw) -> (run, check): builds the operands; run() issues the call(s); check(arm) holds the tight arm to f64.  -> (strided arm, tight arm)"""
    arms = []
    for strided in (True, False):
        arm = Arm(strided, max_rows, max_ld, base)
        run, check = op(arm, **kw)
        torch.cuda.synchronize()
        n0 = _lib.launch_count()
        run()
        torch.cuda.synchronize()
        assert _lib.launch_count() - n0 == launches, (label, "strided" if strided else "tight", _lib.launch_count() - n0, launches)
        arms.append((arm, check))
    A.check_arms(label, arms[0][0].ops, arms[1][0].ops, torch.cuda.synchronize)
    for arm, _ in arms:
        for k in arm.keep:
            S.check_kept(f"{label} {k}", arm.ops[k])
    arms[1][1](arms[1][0])
    return arms[0][0], arms[1][0]


def same_outputs(label, a, b, names):
    """two forms of one operation, both on strided operands: bit for bit"""
    for k in names:
        x, y = a.got(k), b.got(k)
        assert same_bits(x, y), f"{label} {k}: the two forms differ in {int((S.bits(x) != S.bits(y)).sum())} of {y.numel()} values"


# ---- the contrastive loss family ---------------------------------------------------------------------------------------------------------------------------------------
CLIP_N = [1, 5, 15, 17, 65, 130, 257]      # < 16 rows per column block; the 16- and 4-row block tails; the 64-column tail; a second 256-column block
UP = 0.7


def windows(n):
    return sorted({(0, n), (n - 1, 1), (n // 3, max(1, n // 2))})


def clip_ref(x):
    n = x.shape[0]
    rl, cl = torch.logsumexp(x, 1), torch.logsumexp(x, 0)
    d = (torch.softmax(x, 1) + torch.softmax(x, 0) - 2 * torch.eye(n, dtype=torch.float64)) * (UP / (2 * n))
    return (0.5 * (rl + cl) - x.diag()).mean(), rl, cl, d


def op_clip(arm, n, form, r0=0, nloc=0):
    """form: "dlogits" / "value" (lpi_clip_loss_fwd_bwd), "four" (+ lpi_clip_loss_local_grad), "two" / "two value" (lpi_clip_loss_local)"""
    x = rnd(n, n, seed=n) * 3      # the values of test_clip_loss_local_two_launches_equal_the_four
    X = arm.mat("logits", n, n, n + 1, x)
    ld = arm.ld(n, n + 1)
    loss, rl, cl = arm.mat("loss", 1, 1), arm.mat("row_lse", 1, n), arm.mat("col_lse", 1, n)
    DL = arm.mat("dlogits", n, n, n + 3) if form == "dlogits" else None
    G, GT = (arm.mat("g", nloc, n, n + 5), arm.mat("gt", nloc, n, n + 5)) if form in ("four", "two") else (None, None)
    ldg = arm.ld(n, n + 5)

    def run():
        if form in ("dlogits", "value", "four"):
            call("lpi_clip_loss_fwd_bwd", n, X, ld, UP, loss, DL, arm.ld(n, n + 3) if DL is not None else 0, rl, cl, stream())
        if form == "four":
            call("lpi_clip_loss_local_grad", n, X, ld, rl, cl, UP, r0, nloc, G, GT, ldg, stream())
        if form == "two":
            call("lpi_clip_loss_local", n, X, ld, UP, r0, nloc, loss, rl, cl, G, GT, ldg, stream())
        if form == "two value":
            call("lpi_clip_loss_local", n, X, ld, UP, 0, 0, loss, rl, cl, None, None, 0, stream())

    def check(t):
        lref, rref, cref, dref = clip_ref(x.double())
        held_loss("clip loss", t.got("loss"), lref, CLIP_LOSS_BAR)
        held("clip row_lse", t.got("row_lse")[0], rref, CLIP_LOSS_BAR)
        held("clip col_lse", t.got("col_lse")[0], cref, CLIP_LOSS_BAR)
        if DL is not None:
            held("clip dlogits", t.got("dlogits"), dref, CLIP_GRAD_BAR)
        if G is not None:
            held("clip g (local rows)", t.got("g"), dref[r0:r0 + nloc], CLIP_GRAD_BAR)
            held("clip gt (local columns)", t.got("gt"), dref[:, r0:r0 + nloc].t(), CLIP_GRAD_BAR)
    return run, check


@pytest.mark.parametrize("n", CLIP_N)
def test_clip_loss(n):
    """ld = n + 1, lddl = n + 3, ldg = n + 5.  The two-launch form equals the four-launch form bit for bit, with gradients and value only."""
    base = 1 if n % 2 else 3
    size = (n, n + 5, base)
    run_arms(f"clip dlogits {n}", op_clip, *size, 4, n=n, form="dlogits")
    v4, _ = run_arms(f"clip value {n}", op_clip, *size, 3, n=n, form="value")
    v2, _ = run_arms(f"clip local value {n}", op_clip, *size, 2, n=n, form="two value")
    same_outputs(f"clip value {n}", v2, v4, ("loss", "row_lse", "col_lse"))
    for r0, nloc in windows(n):
        a, _ = run_arms(f"clip four {n} [{r0}, {r0 + nloc})", op_clip, *size, 4, n=n, form="four", r0=r0, nloc=nloc)
        b, _ = run_arms(f"clip two {n} [{r0}, {r0 + nloc})", op_clip, *size, 2, n=n, form="two", r0=r0, nloc=nloc)
        same_outputs(f"clip local {n} [{r0}, {r0 + nloc})", b, a, ("loss", "row_lse", "col_lse", "g", "gt"))


def op_ce_rows(arm, n, label0, rows, mode):
    """mode: "out" (dlogits at lddl = n + 3), "in" (dlogits == logits: the gradient overwrites the block), "null" (losses only)"""
    x = rnd(rows, n, seed=n + 7 * rows) * 3
    X = arm.mat("logits", rows, n, n + 1, x, in_out=(mode == "in"))
    ld = arm.ld(n, n + 1)
    LR = arm.mat("loss_rows", 1, rows)
    DL = arm.mat("dlogits", rows, n, n + 3) if mode == "out" else X if mode == "in" else None
    lddl = arm.ld(n, n + 3) if mode == "out" else ld

    def run():
        call("lpi_ce_rows_fwd_bwd", rows, n, X, ld, label0, UP, LR, DL, lddl, stream())

    def check(t):
        x64, lab = x.double(), torch.arange(rows) + label0
        held("ce_rows loss_rows", t.got("loss_rows")[0], torch.logsumexp(x64, 1) - x64[torch.arange(rows), lab], CE_LOSS_BAR)
        if DL is not None:
            held("ce_rows dlogits", t.got("dlogits" if mode == "out" else "logits"), UP * (torch.softmax(x64, 1) - torch.nn.functional.one_hot(lab, n).double()), CE_GRAD_BAR)
    return run, check


@pytest.mark.parametrize("n", CLIP_N)
def test_ce_rows_in_place_out_of_place_and_losses_only(n):
    for r0, nloc in windows(n):
        size = (nloc, n + 3, 3 if n % 2 else 1)
        o, _ = run_arms(f"ce_rows out {n} [{r0}, {r0 + nloc})", op_ce_rows, *size, 1, n=n, label0=r0, rows=nloc, mode="out")
        i, _ = run_arms(f"ce_rows in place {n} [{r0}, {r0 + nloc})", op_ce_rows, *size, 1, n=n, label0=r0, rows=nloc, mode="in")
        z, _ = run_arms(f"ce_rows dlogits NULL {n} [{r0}, {r0 + nloc})", op_ce_rows, *size, 1, n=n, label0=r0, rows=nloc, mode="null")
        assert same_bits(i.got("logits"), o.got("dlogits")) and same_bits(i.got("loss_rows"), o.got("loss_rows")) and same_bits(z.got("loss_rows"), o.got("loss_rows"))


def op_sum_scaled(arm, n, with_b):
    a, b = rnd(n, seed=n), rnd(n, seed=n + 1)
    Av, Bv, out = arm.mat("a", 1, n, fill=a), arm.mat("b", 1, n, fill=b) if with_b else None, arm.mat("out", 1, 1)

    def run():
        call("lpi_sum_scaled", n, Av, Bv, 0.37, out, stream())

    def check(t):
        add = a.double() + (b.double() if with_b else 0)
        held_elem("sum_scaled", t.got("out").reshape(1), (0.37 * add.sum()).reshape(1), 0.37 * sum_bar(n, add.abs().sum()).reshape(1))
    return run, check


@pytest.mark.parametrize("with_b", [False, True], ids=["b NULL", "b"])
@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_sum_scaled(n, with_b):
    run_arms(f"sum_scaled {n}", op_sum_scaled, 1, n, 3, 1, n=n, with_b=with_b)


# ---- prompt CP ----------------------------------------------------------------------------------------------------------------------------------------------------------
CP_LP = [(1, 1), (3, 3), (2, 9)]                          # Lyr P = 1, 9, 18: no multiple of 4 (one workgroup of cp_bwd_t2_kernel holds both stacks' waves); below and above 16
CP_D = [(1, 63), (63, 65), (65, 130), (130, 1)]           # (Dv, Dt): one column, the 64-column tail on either side, a third column block
CP_R = [1, 3, 16]
CP_NAMES = ("g1", "g2v", "g2t", "g3v", "g3t")


def cp_values(Lyr, P, Dv, Dt, r, integer):
    """float: positive on average (0.5 + 0.25 randn; dout 1 + 0.5 randn), so that no output of a one-element shape is a cancelled sum; integer: -3 .. 3, scale = r (sc = 1)"""
    sd = 1000 * Lyr + 100 * P + r
    if integer:
        f = lambda *s, k: ints(*s, seed=sd + k)  # noqa: E731
        return dict(d1=f(Lyr, r, k=1), d2v=f(P, r, k=2), d2t=f(P, r, k=3), d3v=f(Dv, r, k=4), d3t=f(Dt, r, k=5), doutv=f(Lyr * P, Dv, k=6), doutt=f(Lyr * P, Dt, k=7),
                    g10=f(Lyr, r, k=8), scale=float(r))
    f = lambda *s, k: 0.5 + 0.25 * rnd(*s, seed=sd + k)  # noqa: E731
    return dict(d1=f(Lyr, r, k=1), d2v=f(P, r, k=2), d2t=f(P, r, k=3), d3v=f(Dv, r, k=4), d3t=f(Dt, r, k=5), doutv=2 * f(Lyr * P, Dv, k=6), doutt=2 * f(Lyr * P, Dt, k=7),
                g10=f(Lyr, r, k=8), scale=2.0)


def cp_ref(v, Lyr, P, r):
    """f64: both outputs and the five gradients (g1 = the visual stack's + the textual stack's)"""
    q = {k: (t.double().requires_grad_(True) if k.startswith("d") and not k.startswith("dout") else t.double()) for k, t in v.items() if k != "scale"}
    sc = v["scale"] / r
    ov = torch.einsum("lr,pr,dr->lpd", q["d1"], q["d2v"], q["d3v"]) * sc
    ot = torch.einsum("lr,pr,dr->lpd", q["d1"], q["d2t"], q["d3t"]) * sc
    gv = torch.autograd.grad(ov, [q["d1"], q["d2v"], q["d3v"]], q["doutv"].reshape(ov.shape), retain_graph=True)
    gt = torch.autograd.grad(ot, [q["d1"], q["d2t"], q["d3t"]], q["doutt"].reshape(ot.shape))
    # sum |addend| per element of g2 (Lyr D addends: the D of the scratch t, then the Lyr of g2) and of g3 (Lyr P addends): the derived bars of the two-stack form
    a = {k: t.detach().abs() for k, t in q.items()}
    sums = {}
    for sfx in ("v", "t"):
        do = a["dout" + sfx].reshape(Lyr, P, -1)
        sums["g2" + sfx] = (do.shape[-1] * Lyr, sc * torch.einsum("lpd,dr,lr->pr", do, a["d3" + sfx], a["d1"]))
        sums["g3" + sfx] = (Lyr * P, sc * torch.einsum("lpd,lr,pr->dr", do, a["d1"], a["d2" + sfx]))
    return dict(outv=ov.detach().reshape(Lyr * P, -1), outt=ot.detach().reshape(Lyr * P, -1), g1v=gv[0], g1t=gt[0], g1=gv[0] + gt[0], g2v=gv[1], g2t=gt[1], g3v=gv[2], g3t=gt[2],
                sums=sums)


def cp_check(names, ref, integer, bars, derived=False):
    """derived: the two-stack backward — g2v, g2t, g3v, g3t have no f64 bar in an existing test: (m + 2) 2^-23 sum |addend| per element, besides the per-stack bar"""
    def check(t):
        for k in names:
            if integer:
                exact(f"prompt CP {k} (integers)", t.got(k), ref[k])
                continue
            held(f"prompt CP {k}", t.got(k), ref[k], bars(k))
            if derived and k in ref["sums"]:
                held_elem(f"prompt CP two-stack {k}", t.got(k), ref[k], sum_bar(*ref["sums"][k]))
    return check


def op_cp_fwd(arm, Lyr, P, Dv, Dt, r, v, ref, both, integer):
    """both: lpi_prompt_cp_fwd2 (one launch); else lpi_prompt_cp_fwd per stack (two)"""
    d1, d2v, d2t, d3v, d3t = (arm.mat(k, v[k].shape[0], v[k].shape[1], fill=v[k]) for k in ("d1", "d2v", "d2t", "d3v", "d3t"))
    ov, ot = arm.mat("outv", Lyr * P, Dv), arm.mat("outt", Lyr * P, Dt)

    def run():
        if both:
            call("lpi_prompt_cp_fwd2", Lyr, P, Dv, Dt, r, d1, d2v, d2t, d3v, d3t, v["scale"], ov, ot, stream())
        else:
            call("lpi_prompt_cp_fwd", Lyr, P, Dv, r, d1, d2v, d3v, v["scale"], ov, stream())
            call("lpi_prompt_cp_fwd", Lyr, P, Dt, r, d1, d2t, d3t, v["scale"], ot, stream())
    return run, cp_check(("outv", "outt"), ref, integer, lambda k: CP_OUT_BAR)


def op_cp_bwd(arm, Lyr, P, Dv, Dt, r, v, ref, both, integer):
    """both: lpi_prompt_cp_bwd2 (two launches); else lpi_prompt_cp_bwd for the visual stack (g1 overwritten), then the textual one (g1 accumulated): six launches"""
    d1, d2v, d2t, d3v, d3t, dov, dot = (arm.mat(k, v[k].shape[0], v[k].shape[1], fill=v[k]) for k in ("d1", "d2v", "d2t", "d3v", "d3t", "doutv", "doutt"))
    g1, g2v, g2t, g3v, g3t = arm.mat("g1", Lyr, r), arm.mat("g2v", P, r), arm.mat("g2t", P, r), arm.mat("g3v", Dv, r), arm.mat("g3t", Dt, r)
    scr = arm.mat("scratch", 2 * Lyr * P, r, none=True)

    def run():
        if both:
            call("lpi_prompt_cp_bwd2", Lyr, P, Dv, Dt, r, d1, d2v, d2t, d3v, d3t, v["scale"], dov, dot, g1, g2v, g2t, g3v, g3t, scr, stream())
        else:
            call("lpi_prompt_cp_bwd", Lyr, P, Dv, r, d1, d2v, d3v, v["scale"], dov, g1, g2v, g3v, 0, scr, stream())
            call("lpi_prompt_cp_bwd", Lyr, P, Dt, r, d1, d2t, d3t, v["scale"], dot, g1, g2t, g3t, 1, scr[Lyr * P:], stream())
    return run, cp_check(CP_NAMES, ref, integer, lambda k: CP_GRAD_BAR, derived=both)


def op_cp_bwd_one(arm, Lyr, P, Dv, Dt, r, v, ref, acc, integer):
    """one stack (the textual one), accumulate_g1 = acc into a prefilled g1"""
    d1, d2t, d3t, dot = (arm.mat(k, v[k].shape[0], v[k].shape[1], fill=v[k]) for k in ("d1", "d2t", "d3t", "doutt"))
    g1 = arm.mat("g1", Lyr, r, fill=v["g10"] if acc else None, in_out=bool(acc))
    g2t, g3t, scr = arm.mat("g2t", P, r), arm.mat("g3t", Dt, r), arm.mat("scratch", Lyr * P, r, none=True)

    def run():
        call("lpi_prompt_cp_bwd", Lyr, P, Dt, r, d1, d2t, d3t, v["scale"], dot, g1, g2t, g3t, acc, scr, stream())
    one = dict(ref, g1=ref["g1t"] + (v["g10"].double() if acc else 0))
    return run, cp_check(("g1", "g2t", "g3t"), one, integer, lambda k: CP_GRAD_BAR)


CP_CASES = [(lp + d + (CP_R[(i + j) % 3],)) for i, lp in enumerate(CP_LP) for j, d in enumerate(CP_D)]      # every (Lyr, P) x (Dv, Dt); every r with every (Lyr, P)


@pytest.mark.parametrize("integer", [False, True], ids=["float", "integers"])
@pytest.mark.parametrize("Lyr,P,Dv,Dt,r", CP_CASES)
def test_prompt_cp(Lyr, P, Dv, Dt, r, integer):
    """All five factor gradients and both outputs against f64 einsum; the two-stack forms against the per-stack launches, bit for bit."""
    v = cp_values(Lyr, P, Dv, Dt, r, integer)
    ref = cp_ref(v, Lyr, P, r)
    kw = dict(Lyr=Lyr, P=P, Dv=Dv, Dt=Dt, r=r, v=v, ref=ref, integer=integer)
    size = (max(2 * Lyr * P, Dv, Dt), max(Dv, Dt, r), 1 if r % 2 else 3)
    label = f"prompt CP ({Lyr}, {P}, {Dv}, {Dt}, r {r})"
    f1, _ = run_arms(label + " fwd per stack", op_cp_fwd, *size, 2, both=False, **kw)
    f2, _ = run_arms(label + " fwd2", op_cp_fwd, *size, 1, both=True, **kw)
    same_outputs(label + " fwd2", f2, f1, ("outv", "outt"))
    b1, _ = run_arms(label + " bwd per stack", op_cp_bwd, *size, 6, both=False, **kw)
    b2, _ = run_arms(label + " bwd2", op_cp_bwd, *size, 2, both=True, **kw)
    same_outputs(label + " bwd2", b2, b1, CP_NAMES)
    for acc in (0, 1):
        run_arms(label + f" bwd accumulate_g1 = {acc}", op_cp_bwd_one, *size, 3, acc=acc, **kw)


# ---- alignment loss ------------------------------------------------------------------------------------------------------------------------------------------------------
def op_align(arm, Lyr, P, Dv, Dt, grads, two):
    """two: lpi_align_loss_fwd_bwd2 (two launches); else lpi_align_loss_fwd_bwd (three with gradients, one without).  Values: row means / temp of order 0.3 at every width,
    as test_align_loss has them at 768 / 512."""
    nr = Lyr * P
    vis, txt = rnd(nr, Dv, seed=Lyr + Dv) * 0.003 * Dv ** 0.5 + 0.001, rnd(nr, Dt, seed=P + Dt) * 0.003 * Dt ** 0.5 - 0.001
    V, T, loss = arm.mat("vis", nr, Dv, fill=vis), arm.mat("txt", nr, Dt, fill=txt), arm.mat("loss", 1, 1)
    DV, DT = (arm.mat("dvis", nr, Dv), arm.mat("dtxt", nr, Dt)) if grads else (None, None)
    scr = arm.mat("scratch", nr, 2, none=True) if two else None

    def run():
        if two:
            call("lpi_align_loss_fwd_bwd2", Lyr, P, Dv, Dt, V, T, 0.01, 0.1, loss, DV, DT, scr, stream())
        else:
            call("lpi_align_loss_fwd_bwd", Lyr, P, Dv, Dt, V, T, 0.01, 0.1, loss, DV, DT, stream())

    def check(t):
        v, x = vis.double().reshape(Lyr, P, Dv).requires_grad_(True), txt.double().reshape(Lyr, P, Dt).requires_grad_(True)
        Sm = (v.mean(-1) / 0.01) @ (x.mean(-1) / 0.01).t()
        lab = torch.arange(Lyr)
        ref = 0.1 * (torch.nn.functional.cross_entropy(Sm, lab) + torch.nn.functional.cross_entropy(Sm.t(), lab)) / 2
        ref.backward()
        held_loss("alignment loss", t.got("loss"), ref.detach(), ALIGN_LOSS_BAR)
        if grads and Lyr > 1:      # (Lyr = 1: a 1 x 1 softmax, the gradient is identically zero)
            held("alignment dvis", t.got("dvis"), v.grad.reshape(nr, Dv), ALIGN_GRAD_BAR)
            held("alignment dtxt", t.got("dtxt"), x.grad.reshape(nr, Dt), ALIGN_GRAD_BAR)
        elif grads:
            exact("alignment dvis (Lyr = 1)", t.got("dvis"), torch.zeros(nr, Dv)), exact("alignment dtxt (Lyr = 1)", t.got("dtxt"), torch.zeros(nr, Dt))
    return run, check


def align_case(Lyr, P, Dv, Dt, grads):
    size = (Lyr * P, max(Dv, Dt, 2), 3 if Dv % 2 else 1)
    label = f"alignment ({Lyr}, {P}, {Dv}, {Dt}) {'with' if grads else 'without'} gradients"
    a, _ = run_arms(label, op_align, *size, 3 if grads else 1, Lyr=Lyr, P=P, Dv=Dv, Dt=Dt, grads=grads, two=False)
    b, _ = run_arms(label + " two launches", op_align, *size, 2, Lyr=Lyr, P=P, Dv=Dv, Dt=Dt, grads=grads, two=True)
    same_outputs(label, b, a, ("loss", "dvis", "dtxt") if grads else ("loss",))


@pytest.mark.parametrize("grads", [True, False], ids=["gradients", "value"])
@pytest.mark.parametrize("Dv,Dt", [(1, 255), (255, 257), (257, 300), (300, 1)])
@pytest.mark.parametrize("Lyr,P", [(1, 1), (2, 3), (9, 16)])
def test_alignment_loss_both_forms(Lyr, P, Dv, Dt, grads):
    align_case(Lyr, P, Dv, Dt, grads)


def test_alignment_loss_at_the_largest_prompt_count_its_lds_check_accepts():
    """lpi_align_loss_fwd_bwd keeps 4 Lyr P + 2 Lyr^2 + 2 Lyr floats in LDS and refuses more than 64 KB: at Lyr = 2 that is P <= 2046 (16380 floats); P = 2047 is refused
    before any launch."""
    align_case(2, 2046, 3, 1, True)
    z = torch.zeros(2 * 2047 * 3, device=DEV)
    n0 = _lib.launch_count()
    with pytest.raises(_lib.LpiError):
        call("lpi_align_loss_fwd_bwd", 2, 2047, 3, 1, z, z, 0.01, 0.1, z, None, None, stream())
    assert _lib.launch_count() == n0


# ---- task loss -----------------------------------------------------------------------------------------------------------------------------------------------------------
def task_target(T):
    tgt = torch.eye(T, dtype=I32)      # the diagonal is every row's positive; T = 2: the other entry its negative
    if T > 2:
        for i in range(0, T - 1, 2):
            tgt[i, i + 1] = tgt[i + 1, i] = 1      # pairs of similar tasks; every row keeps at least T - 2 negatives
    return tgt


def op_task_loss(arm, T, D, row, acc):
    X = rnd(T, D, seed=T + D)
    for i in range(0, T - 1, 2):
        X[i + 1] = X[i] + 0.05 * rnd(D, seed=T + D + i + 1)      # a similar pair, as in test_nt_bxent_task_loss: the sigmoid is not saturated everywhere
    tgt, dx0 = task_target(T), rnd(D, seed=3 * T + D)
    Xd, Td = arm.mat("X", T, D, fill=X), arm.mat("target", T, T, fill=tgt, td=I32)
    loss, scr = arm.mat("loss", 1, 1), arm.mat("scratch", 2 * T, T, none=True)
    DX = arm.mat("dx_row", 1, D, fill=dx0 if (acc or row < 0) else None, in_out=bool(acc or row < 0), keep=row < 0)      # row < 0: forward only, dx_row keeps its bits

    def run():
        call("lpi_nt_bxent_fwd_bwd", T, D, row, Xd, Td, 0.5, 0.8, loss, DX, acc, scr, stream())

    def check(t):
        Xr = X.double().requires_grad_(True)
        xn = Xr / Xr.norm(dim=-1, keepdim=True)
        cos = xn @ xn.t()
        cos.retain_grad()
        cs = cos.masked_fill(torch.eye(T, dtype=torch.bool), float("inf"))
        el = torch.nn.functional.binary_cross_entropy_with_logits((cs / 0.5).sigmoid(), tgt.double(), reduction="none")
        pos = tgt.bool()
        ref = 0.8 * ((el * pos).sum(1) / pos.sum(1) + (el * ~pos).sum(1) / (~pos).sum(1)).mean()
        assert bool(torch.isfinite(ref))
        ref.backward()
        held_loss("task loss", t.got("loss"), ref.detach(), TASK_LOSS_BAR)
        if row >= 0 and D == 1 and not acc:
            # one column: every cosine is +-1 whatever X holds, the true gradient is identically zero and max |reference| is no scale.  The kernel forms it as
            # sum_j w_j (x_j / (|x_r| |x_j|) - cos_rj x_r / |x_r|^2), w_j = dL/dcos_rj + dL/dcos_jr: two addends of size |w_j| / |x_r| that cancel.  The same relative
            # bar on the scale of those addends (from the f64 reference's dL/dcos), as an absolute bound.
            w = (cos.grad[row] + cos.grad[:, row]).abs().sum()
            assert float(Xr.grad[row].abs().max()) < 1e-12 * float(w / X[row].abs().double().max())      # the reference agrees: zero up to f64 rounding
            held_elem("task loss dx_row at D = 1, overwritten", t.got("dx_row")[0], torch.zeros(1), TASK_GRAD_BAR * (2 * w / X[row].abs().double().max()).detach().reshape(1))
        elif row >= 0:
            held("task loss dx_row", t.got("dx_row")[0], Xr.grad[row] + (dx0.double() if acc else 0), TASK_GRAD_BAR)
    return run, check


@pytest.mark.parametrize("D", [1, 255, 257, 300])
@pytest.mark.parametrize("T", [2, 5, 32])
def test_task_loss(T, D):
    for row in (0, T - 1, -1):
        for acc in (0, 1):
            run_arms(f"task loss T {T} D {D} row {row} accumulate {acc}", op_task_loss, 2 * T, max(D, T), 1 if T % 2 else 3, 3 if row >= 0 else 2, T=T, D=D, row=row, acc=acc)


# ---- k-means passes ------------------------------------------------------------------------------------------------------------------------------------------------------
KM = [(1, 1, 1), (5, 63, 3), (15, 65, 5), (17, 130, 3), (37, 130, 5), (37, 1, 1), (15, 63, 1), (5, 65, 5)]      # (n, E, k): n < 16, n % 4 != 0, E tails, two column blocks


def km_x(n, E, integer):
    return ints(n, E, seed=n + E) if integer else rnd(n, E, seed=n + E)


def op_km_sqdist(arm, n, E, nc, integer):
    x = km_x(n, E, integer)
    cand = (torch.arange(nc) * 5 + n - 1) % n
    X, Cd, out = arm.mat("X", n, E, E + 3, x), arm.mat("cand", 1, nc, fill=cand, td=I32), arm.mat("out", nc, n)

    def run():
        call("lpi_kmeans_sqdist", n, E, nc, X, arm.ld(E, E + 3), Cd, out, stream())

    def check(t):
        d2 = (x.double()[None] - x.double()[cand][:, None]) ** 2
        if integer:
            exact("kmeans_sqdist (integers)", t.got("out"), d2.sum(-1))
        else:
            held_elem("kmeans_sqdist", t.got("out"), d2.sum(-1), sum_bar(E, d2.sum(-1)))
    return run, check


def km_centres(k, E, x, integer):
    c = ints(k, E, seed=k + E + 50) if integer else rnd(k, E, seed=k + E + 50)
    if integer:
        c[0] = x[0]              # a point ON a centre: distance 0
        if k > 1:
            c[1] = c[0]          # two identical centres: the lower index takes every point they are nearest to
    return c


def op_km_assign(arm, n, E, k, integer, mindist, preset="none"):
    """preset: "none" (labels hold k: every label is written), "answer" (nothing moves: changed stays 0), "one wrong" (changed = 1)"""
    x = km_x(n, E, integer)
    c = km_centres(k, E, x, integer)
    d2 = ((x.double()[:, None] - c.double()[None]) ** 2).sum(-1)
    ans = torch.from_numpy(np.argmin(d2.numpy(), axis=1).astype(np.int32))      # numpy: the FIRST minimum
    lab0 = torch.full((n,), k, dtype=I32) if preset == "none" else ans.clone()
    if preset == "one wrong":
        lab0[n // 2] = (ans[n // 2] + 1) % (k + 1)
    X, C = arm.mat("X", n, E, E + 3, x), arm.mat("centers", k, E, fill=c)
    L = arm.mat("labels", 1, n, fill=lab0, in_out=True, td=I32)
    CH = arm.mat("changed", 1, 1, fill=torch.zeros(1, dtype=I32), in_out=True, td=I32)
    MD = arm.mat("mindist", 1, n) if mindist else None

    def run():
        call("lpi_kmeans_assign", n, E, k, X, arm.ld(E, E + 3), C, L, CH, MD, stream())

    def check(t):
        best = d2.min(1)[0]
        assert int(t.got("changed")) == (0 if preset == "answer" else 1)
        if integer:
            exact("kmeans_assign labels (integers)", t.got("labels")[0], ans)
            assert k == 1 or not bool((t.got("labels") == 1).any()), "a point took the higher of two identical centres"
            if mindist:
                exact("kmeans_assign mindist (integers)", t.got("mindist")[0], best)
        else:
            bar = sum_bar(E, best)
            srt = d2.sort(1)[0]
            safe = (srt[:, 1] - srt[:, 0] > 2 * sum_bar(E, srt[:, 1])) if k > 1 else torch.ones(n, dtype=torch.bool)
            assert int(safe.sum()) >= n - 1 and torch.equal(t.got("labels")[0][safe], ans[safe])
            if mindist:
                held_elem("kmeans_assign mindist", t.got("mindist")[0], best, bar)
    return run, check


def op_km_update(arm, n, E, k, integer):
    x = km_x(n, E, integer)
    lab = (torch.arange(n) * 3 % max(1, k - 1)).to(I32)      # k > 1: cluster k - 1 has no point
    X, L = arm.mat("X", n, E, E + 3, x), arm.mat("labels", 1, n, fill=lab, td=I32)
    NC, CN = arm.mat("new_centers", k, E), arm.mat("counts", 1, k)

    def run():
        call("lpi_kmeans_update", n, E, k, X, arm.ld(E, E + 3), L, NC, CN, stream())

    def check(t):
        cnt = torch.stack([(lab == c).sum() for c in range(k)]).double()
        sums = torch.stack([x.double()[lab == c].sum(0) for c in range(k)])
        sabs = torch.stack([x.double()[lab == c].abs().sum(0) for c in range(k)])
        mean = sums / cnt.clamp_min(1)[:, None]
        exact("kmeans_update counts", t.got("counts")[0], cnt)
        if k > 1:
            assert float(cnt[k - 1]) == 0 and bool((t.got("new_centers")[k - 1] == 0).all()), "the empty cluster's centre is not zero"
        if integer:      # an exact integer sum divided by an exact count: the f32 quotient, to 1 ulp
            held_elem("kmeans_update new_centers (integers; 1 ulp)", t.got("new_centers"), mean, U * mean.abs())
        else:
            held_elem("kmeans_update new_centers", t.got("new_centers"), mean, sum_bar(cnt[:, None], sabs / cnt.clamp_min(1)[:, None]))
    return run, check


def op_km_colstats(arm, n, E, integer, center):
    x = km_x(n, E, integer)
    c = (ints(E, seed=E + 9) if integer else x.mean(0) + 0.01 * rnd(E, seed=E + 9)) if center else None
    X, C = arm.mat("X", n, E, E + 3, x), arm.mat("center", 1, E, fill=c) if center else None
    CS, CQ = arm.mat("colsum", 1, E), arm.mat("colsq", 1, E)

    def run():
        call("lpi_kmeans_colstats", n, E, X, arm.ld(E, E + 3), C, CS, CQ, stream())

    def check(t):
        v = x.double() - (c.double() if center else 0)
        if integer:
            exact("kmeans_colstats colsum (integers)", t.got("colsum")[0], v.sum(0)), exact("kmeans_colstats colsq (integers)", t.got("colsq")[0], (v * v).sum(0))
        else:
            held_elem("kmeans_colstats colsum", t.got("colsum")[0], v.sum(0), sum_bar(n, v.abs().sum(0)))
            held_elem("kmeans_colstats colsq", t.got("colsq")[0], (v * v).sum(0), sum_bar(n, (v * v).sum(0)))
    return run, check


@pytest.mark.parametrize("integer", [False, True], ids=["float", "integers"])
@pytest.mark.parametrize("n,E,k", KM)
def test_kmeans_passes_each_on_its_own(n, E, k, integer):
    size = (max(n, k), max(E + 3, n), 1 if E % 2 else 3)
    label = f"kmeans ({n}, {E}, {k})"
    run_arms(label + " sqdist", op_km_sqdist, *size, 1, n=n, E=E, nc=k, integer=integer)
    for mindist in (True, False):
        run_arms(label + f" assign mindist {mindist}", op_km_assign, *size, 1, n=n, E=E, k=k, integer=integer, mindist=mindist)
    run_arms(label + " update", op_km_update, *size, 1, n=n, E=E, k=k, integer=integer)
    for center in (True, False):
        run_arms(label + f" colstats center {center}", op_km_colstats, *size, 1, n=n, E=E, integer=integer, center=center)
    if integer:      # the exact answer is known: labels pre-set to it leave `changed` 0; one wrong label sets it
        run_arms(label + " assign, labels hold the answer", op_km_assign, *size, 1, n=n, E=E, k=k, integer=True, mindist=True, preset="answer")
        run_arms(label + " assign, one wrong label", op_km_assign, *size, 1, n=n, E=E, k=k, integer=True, mindist=False, preset="one wrong")


# ---- task id, ranking, top-k ---------------------------------------------------------------------------------------------------------------------------------------------
def op_task_id(arm, n, E, integer, dist, T=3, C=2):
    f = ints(n, E, seed=n + E) if integer else rnd(n, E, seed=n + E)
    keys = ints(T, C, E, seed=E + 3) if integer else rnd(T, C, E, seed=E + 3)
    if integer:
        keys[1] = keys[0]      # two tasks with the same key set: the lower one wins wherever they are nearest
        keys[0, 1], keys[1, 1] = f[0], f[0]
    F, K = arm.mat("feat", n, E, E + 1, f), arm.mat("keys", T * C, E, fill=keys)
    sel, DS = arm.mat("sel", 1, n, td=I32), arm.mat("dist", n, T) if dist else None

    def run():
        call("lpi_l1_task_id", n, E, T, C, F, arm.ld(E, E + 1), K, sel, DS, stream())

    def check(t):
        l1 = (f.double()[:, None, None] - keys.double()[None]).abs().sum(-1)      # [n, T, C]
        d = l1.min(2)[0]
        ans = torch.from_numpy(np.argmin(d.numpy(), axis=1).astype(np.int32))
        if integer:
            exact("l1_task_id sel (integers)", t.got("sel")[0], ans)
            assert not bool((t.got("sel") == 1).any()) and int(t.got("sel")[0, 0]) == 0, "the higher of two identical tasks won"
            if dist:
                exact("l1_task_id dist (integers)", t.got("dist"), d)
        else:
            bar = sum_bar(E, d).clamp_max(L1_DIST_CAP)
            srt = d.sort(1)[0]
            safe = srt[:, 1] - srt[:, 0] > 2 * sum_bar(E, srt[:, 1])
            assert int(safe.sum()) >= n - 1 and torch.equal(t.got("sel")[0][safe], ans[safe])
            if dist:
                held_elem("l1_task_id dist", t.got("dist"), d, bar)
    return run, check


@pytest.mark.parametrize("integer", [False, True], ids=["float", "integers"])
@pytest.mark.parametrize("n,E", [(1, 1), (5, 63), (37, 65), (5, 130), (37, 130), (37, 1)])
def test_l1_task_id(n, E, integer):
    for dist in (True, False):
        run_arms(f"l1_task_id ({n}, {E}) dist {dist}", op_task_id, max(n, 6), max(E + 1, 3, n), 3 if E % 2 else 1, 1, n=n, E=E, integer=integer, dist=dist)


NR = 7      # two workgroups of four rows, the second partial


def rank_scores(nc):
    """row 0 random; 1 all equal; 2 random with -inf in every third column; 3 a tie between column c0 and its 64-distant neighbour (the same lane; nc <= 64: first and
    last column); 4 integers -3 .. 3 (ties everywhere); 5 integers with -inf mixed in; 6 -inf but one column.  gt: three per row, padded with -1; row 3's first is c0."""
    s = rnd(NR, nc, seed=nc)
    s[1] = 0.5
    s[2, ::3] = float("-inf")
    c0, c1 = ((nc - 65) // 2, (nc - 65) // 2 + 64) if nc > 64 else (0, nc - 1)
    s[3, c1] = s[3, c0]
    s[4] = ints(nc, seed=nc + 1)
    s[5] = ints(nc, seed=nc + 2)
    s[5, 1::4] = float("-inf")
    s[6] = float("-inf")
    s[6, nc // 2] = 1.0
    gt = torch.full((NR, 3), -1, dtype=I32)
    gt[:, 0] = torch.tensor([nc - 1, nc // 2, 0, c0, nc // 3, min(1, nc - 1), nc // 2])
    gt[0, 1], gt[4, 2], gt[5, 2], gt[6, 1] = 0, nc - 1, nc // 2, 0
    return s, gt


def order(row):
    return np.argsort(row.numpy(), kind="stable")[::-1]      # the reference of test_retrieval_rank_and_topk: later index first among equal scores


def op_rank(arm, nc):
    s, gt = rank_scores(nc)
    Sd, G, R = arm.mat("scores", NR, nc, nc + 1, s), arm.mat("gt", NR, 3, fill=gt, td=I32), arm.mat("rank", 1, NR, td=I32)

    def run():
        call("lpi_retrieval_rank", NR, nc, Sd, arm.ld(nc, nc + 1), G, 3, R, stream())

    def check(t):
        ref = [min(int(np.where(order(s[i]) == j)[0][0]) for j in gt[i].tolist() if j >= 0) for i in range(NR)]
        assert t.got("rank")[0].tolist() == ref, (t.got("rank")[0].tolist(), ref)
    return run, check


def op_topk(arm, nc, k, val):
    s, _ = rank_scores(nc)
    Sd, IX, VL = arm.mat("scores", NR, nc, nc + 1, s), arm.mat("idx", NR, k, td=I32), arm.mat("val", NR, k) if val else None

    def run():
        call("lpi_topk", NR, nc, k, Sd, arm.ld(nc, nc + 1), IX, VL, stream())

    def check(t):
        refi = np.stack([order(s[i])[:k] for i in range(NR)])
        assert (t.got("idx").numpy() == refi).all(), (t.got("idx"), refi)
        if val:
            exact("topk val", t.got("val"), torch.gather(s, 1, torch.from_numpy(refi.copy()).long()))
    return run, check


@pytest.mark.parametrize("nc", [1, 5, 63, 65, 130])
def test_retrieval_rank_and_topk(nc):
    size = (NR, max(nc + 1, NR), 1 if nc % 2 else 3)
    run_arms(f"retrieval_rank {nc}", op_rank, *size, 1, nc=nc)
    for k, val in ((1, True), (1, False), (nc, True), (nc, False)):
        run_arms(f"topk {nc} k {k} val {val}", op_topk, *size, 1, nc=nc, k=k, val=val)


# ---- interaction ---------------------------------------------------------------------------------------------------------------------------------------------------------
IP = ("dim_1_v2t", "dim_2_v2t", "dim_3_v2t", "dim_1_t2v", "dim_2_t2v", "dim_3_t2v", "visual_norm.weight", "visual_norm.bias", "textual_norm.weight", "textual_norm.bias")
MIX, EPS = 0.1, 1e-5


def interact_values(N, Dv, Dt, R, Lyr):
    gen = torch.Generator().manual_seed(N * 7 + R + Dv)
    rn = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    p = {"dim_1_v2t": rn(Lyr, R), "dim_2_v2t": rn(Dv + 1, R) * 0.2, "dim_3_v2t": rn(Dt, R), "dim_1_t2v": rn(Lyr, R), "dim_2_t2v": rn(Dt + 1, R) * 0.2, "dim_3_t2v": rn(Dv, R),
         "visual_norm.weight": 1 + 0.1 * rn(Dv), "visual_norm.bias": 0.1 * rn(Dv), "textual_norm.weight": 1 + 0.1 * rn(Dt), "textual_norm.bias": 0.1 * rn(Dt)}      # test_interact_kernels_vs_f64
    return p, rn(N, Dv), rn(N, Dt), rn(N, Dv), rn(N, Dt)


def interact_ref(p, xv, xt, wv, wt, layer):
    from oracle import lpi_oracle as O
    p64 = {k: v.double().requires_grad_(True) for k, v in p.items()}
    a, b = xv.double().requires_grad_(True), xt.double().requires_grad_(True)
    vr, tr = O.interact(p64, a, b, layer)
    ((vr * wv.double()).sum() + (tr * wt.double()).sum()).backward()

    def mixed(d1, d2, d3, xin, xout):      # the row a LayerNorm sees: its mean and rstd are what `stat` keeps
        m = torch.einsum("r,ir,jr->ij", d1[layer], d2, d3) / d1.shape[1]
        u = (1 - MIX) * xout + MIX * (xin @ m[:-1] + m[-1:])
        return u.mean(1), 1 / torch.sqrt(u.var(1, unbiased=False) + EPS)
    with torch.no_grad():
        sv = mixed(p64["dim_1_t2v"], p64["dim_2_t2v"], p64["dim_3_t2v"], b, a)
        st = mixed(p64["dim_1_v2t"], p64["dim_2_v2t"], p64["dim_3_v2t"], a, b)
    g = {k: v.grad for k, v in p64.items()}

    def side(d, out):      # dd3 | dd2 | dd1 row `layer` | dgamma | dbeta (include/lpi_hip.h)
        return torch.cat([g[f"dim_3_{d}"].reshape(-1), g[f"dim_2_{d}"].reshape(-1), g[f"dim_1_{d}"][layer], g[f"{out}_norm.weight"], g[f"{out}_norm.bias"]])
    return dict(out_v=vr.detach(), out_t=tr.detach(), stat=torch.stack([sv[0], sv[1], st[0], st[1]]), dxv=a.grad, dxt=b.grad, v2t=side("v2t", "textual"), t2v=side("t2v", "visual"))


def interact_operands(arm, N, Dv, Dt, R, Lyr, p, xv, xt):
    XV, XT = arm.mat("xv", N, Dv, Dv + 1, xv), arm.mat("xt", N, Dt, Dt + 3, xt)
    ps = [arm.mat(k, p[k].reshape(-1, R).shape[0] if p[k].dim() == 2 else 1, R if p[k].dim() == 2 else p[k].numel(), fill=p[k]) for k in IP]
    return XV, arm.ld(Dv, Dv + 1), XT, arm.ld(Dt, Dt + 3), ps


def op_interact_fwd(arm, N, Dv, Dt, R, Lyr, layer, vals, ref):
    p, xv, xt, _, _ = vals
    XV, ldv, XT, ldt, ps = interact_operands(arm, N, Dv, Dt, R, Lyr, p, xv, xt)
    OV, OT, ST = arm.mat("out_v", N, Dv, Dv + 5), arm.mat("out_t", N, Dt, Dt + 7), arm.mat("stat", 4, N)

    def run():
        call("lpi_interact_fwd", N, Dv, Dt, R, Lyr, layer, XV, ldv, XT, ldt, *ps, MIX, EPS, OV, arm.ld(Dv, Dv + 5), OT, arm.ld(Dt, Dt + 7), ST, stream())

    def check(t):
        for k in ("out_v", "out_t", "stat"):
            held(f"interact {k}", t.got(k), ref[k], INTERACT_OUT_BAR)
    return run, check


def op_interact_bwd(arm, N, Dv, Dt, R, Lyr, layer, vals, ref, nws):
    """dxv / dxt are OUTPUTS that hold UNWRITTEN: lpi_interact_bwd clears the strided footprint (hipMemset2DAsync; the tight arm: one hipMemsetAsync) and the kernel adds into it"""
    p, xv, xt, wv, wt = vals
    XV, ldv, XT, ldt, ps = interact_operands(arm, N, Dv, Dt, R, Lyr, p, xv, xt)
    GV, GT = arm.mat("g_out_v", N, Dv, Dv + 9, wv), arm.mat("g_out_t", N, Dt, Dt + 11, wt)
    DXV, DXT = arm.mat("dxv", N, Dv, Dv + 13), arm.mat("dxt", N, Dt, Dt + 15)
    la, lb = Dt * R + (Dv + 1) * R + R + 2 * Dt, Dv * R + (Dt + 1) * R + R + 2 * Dv
    GR, WS = arm.flat("grads", la + lb), arm.flat("workspace", nws, none=True)

    def run():
        call("lpi_interact_bwd", N, Dv, Dt, R, Lyr, layer, XV, ldv, XT, ldt, *ps, MIX, EPS, GV, arm.ld(Dv, Dv + 9), GT, arm.ld(Dt, Dt + 11), DXV, arm.ld(Dv, Dv + 13), DXT,
             arm.ld(Dt, Dt + 15), GR, WS, stream())

    def check(t):
        held("interact dxv", t.got("dxv"), ref["dxv"], INTERACT_GRAD_BAR), held("interact dxt", t.got("dxt"), ref["dxt"], INTERACT_GRAD_BAR)
        got = t.got("grads")
        floor = 1e-9 * float(torch.cat([ref["v2t"], ref["t2v"]]).abs().max())
        for name, g, r, Din, Dout in (("v2t", got[:la], ref["v2t"], Dv, Dt), ("t2v", got[la:], ref["t2v"], Dt, Dv)):
            cuts = [0, Dout * R, Dout * R + (Din + 1) * R, Dout * R + (Din + 1) * R + R, Dout * R + (Din + 1) * R + R + Dout, len(r)]
            for part, lo, hi in zip(("dd3", "dd2", "dd1", "dgamma", "dbeta"), cuts[:-1], cuts[1:]):
                if float(r[lo:hi].abs().max()) > floor:
                    held(f"interact {part}", g[lo:hi], r[lo:hi], INTERACT_GRAD_BAR)
                else:      # a LayerNorm over ONE column has no gradient: zero in exact arithmetic (f64 leaves rounding dust); held to the same bar on the floor's scale
                    assert float(g[lo:hi].abs().max()) <= INTERACT_GRAD_BAR * floor, (name, part)
    return run, check


@pytest.mark.parametrize("N,Dv,Dt,R,Lyr,layer", [(1, 72, 260, 1, 2, 0), (5, 1024, 255, 3, 4, 3), (257, 72, 260, 8, 3, 2), (257, 257, 1, 1, 2, 0), (5, 257, 1, 8, 9, 8),
                                                 (257, 1024, 255, 3, 1, 0)])
def test_interact_raw_with_ten_leading_dimensions(N, Dv, Dt, R, Lyr, layer):
    """N = 257: two rows per workgroup, the last workgroup partial.  ldv, ldt, ldov, ldot, ldgv, ldgt, lddv, lddt = width + 1, 3, 5, 7, 9, 11, 13, 15."""
    vals = interact_values(N, Dv, Dt, R, Lyr)
    ref = interact_ref(*vals, layer)
    nws = int(_lib.load().lpi_interact_workspace_floats(N, Dv, Dt, R))
    G = -(-N // max(1, (N + 255) // 256))
    assert nws == G * (2 * (Dv + Dt) * R + 4 * R + 2 * (Dv + Dt))      # per-workgroup partials of both directions
    label = f"interact ({N}, {Dv}, {Dt}, R {R}, layer {layer} of {Lyr})"
    rows = max(N, Dv + 1, Dt + 1, Lyr, 4, -(-nws // (max(Dv, Dt) + 15)), -(-(nws // G) // (max(Dv, Dt) + 15)))      # (the workspace and `grads`, seen as rows of the widest leading dimension, count too)
    size = (rows, max(Dv, Dt) + 15, 1 if N % 2 else 3)
    run_arms(label + " fwd", op_interact_fwd, *size, 1, N=N, Dv=Dv, Dt=Dt, R=R, Lyr=Lyr, layer=layer, vals=vals, ref=ref)
    run_arms(label + " bwd", op_interact_bwd, *size, 2, N=N, Dv=Dv, Dt=Dt, R=R, Lyr=Lyr, layer=layer, vals=vals, ref=ref, nws=nws)


# ---- SGD -----------------------------------------------------------------------------------------------------------------------------------------------------------------
def op_sgd(arm, n, first):
    p, g, b = rnd(n, seed=n), rnd(n, seed=n + 1) * 1e-3, rnd(n, seed=n + 2) * 1e-2
    Pv, Gv, Bv = arm.mat("param", 1, n, fill=p, in_out=True), arm.mat("grad", 1, n, fill=g), arm.mat("momentum_buf", 1, n, fill=b, in_out=True)

    def run():
        call("lpi_sgd_step", n, Pv, Gv, Bv, 0.05, 0.9, 2e-4, first, stream())

    def check(t):
        d = g.double() + 2e-4 * p.double()
        nb = d if first else 0.9 * b.double() + d
        held_abs("sgd momentum_buf", t.got("momentum_buf")[0], nb, SGD_BAR), held_abs("sgd param", t.got("param")[0], p.double() - 0.05 * nb, SGD_BAR)
    return run, check


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("n", [1, 255, 257])
def test_sgd_step(n, first):
    run_arms(f"sgd {n} first {first}", op_sgd, 1, n, 3, 1, n=n, first=first)


# ---- what the checks refuse ----------------------------------------------------------------------------------------------------------------------------------------------
def test_what_the_host_checks_refuse_launches_nothing_and_writes_nothing():
    """Library version 619.  Every refusal of loss.hip and interact.hip as a case (each leading dimension, range and size rule by hand; every required pointer as NULL and
    every count as 0 generated from the argument lists): LPI_EINVAL, the launch counter stays put, every output arena keeps its bits; then every
    argument list a refusal was derived from launches.  New in 619: lpi_clip_loss_fwd_bwd checks lddl before its first launch (it had written row_lse, col_lse and loss by
    then); lpi_ce_rows_fwd_bwd refuses dlogits == logits with lddl != ld; lpi_align_loss_fwd_bwd refuses one gradient pointer without the other (as the two-launch form always
    did); the lpi_prompt_cp_* calls refuse Lyr P r or D r beyond int (their kernels index with int) and, like lpi_sgd_step and lpi_copy_rows, an element count
    whose one-thread-per-element grid does not fit; lpi_interact_workspace_floats refuses what lpi_interact_fwd refuses."""
    lib = _lib.load()
    s, E = stream(), -22
    nel = S.arena_bytes(64, 1100, 4, 1) // 4
    outs = []

    def O(td=torch.float32):      # an output arena of its own; the pointer is one element in
        rec = S.operand(1, nel - 2, nel - 2, td, 1, nel, None, DEV)
        outs.append(rec)
        return rec.t.data_ptr()
    zin = torch.zeros(nel, device=DEV)
    iin = torch.zeros(nel, dtype=I32, device=DEV)
    Z, Zi = zin.data_ptr(), iin.data_ptr()
    n = 5
    cases = []      # (function, good arguments {name: value}, [(name, bad value)], launches of the good list)
    clip = dict(n=n, x=Z, ld=n + 1, up=1.0, loss=O(), dl=O(), lddl=n + 3, rl=O(), cl=O(), s=s)
    cases.append((lib.lpi_clip_loss_fwd_bwd, clip, [("lddl", n - 1), ("ld", n - 1), ("n", 0), ("x", None), ("loss", None), ("rl", None), ("cl", None)], 4))
    lg = dict(n=n, x=Z, ld=n + 1, rl=Z, cl=Z, up=1.0, r0=1, nloc=3, g=O(), gt=O(), ldg=n + 5, s=s)
    cases.append((lib.lpi_clip_loss_local_grad, lg, [("ldg", n - 1), ("ld", n - 1), ("r0", -1), ("nloc", 0), ("nloc", 5), ("g", None), ("gt", None), ("rl", None), ("n", 0)], 1))
    lc = dict(n=n, x=Z, ld=n + 1, up=1.0, r0=1, nloc=3, loss=O(), rl=O(), cl=O(), g=O(), gt=O(), ldg=n + 5, s=s)
    cases.append((lib.lpi_clip_loss_local, lc, [("ldg", n - 1), ("ld", n - 1), ("r0", -1), ("nloc", 0), ("nloc", 5), ("g", None), ("gt", None), ("loss", None), ("n", 0)], 2))
    ce = dict(rows=3, n=n, x=Z, ld=n + 1, label0=2, up=1.0, lr=O(), dl=O(), lddl=n + 3, s=s)
    cases.append((lib.lpi_ce_rows_fwd_bwd, ce, [("lddl", n - 1), ("ld", n - 1), ("label0", 3), ("label0", -1), ("rows", 0), ("dl", Z), ("lr", None), ("x", None)], 1))
    cases.append((lib.lpi_sum_scaled, dict(n=n, a=Z, b=Z, sc=1.0, out=O(), s=s), [("n", 0), ("a", None), ("out", None)], 1))
    cases.append((lib.lpi_sgd_step, dict(n=n, p=O(), g=Z, b=O(), lr=0.1, m=0.9, wd=0.0, first=0, s=s), [("n", 0), ("p", None), ("g", None), ("b", None)], 1))
    l1 = dict(n=n, E=7, T=2, C=2, f=Z, ldf=8, keys=Z, sel=O(I32), dist=O(), s=s)
    cases.append((lib.lpi_l1_task_id, l1, [("ldf", 6), ("E", 0), ("T", 0), ("C", 0), ("n", 0), ("f", None), ("keys", None), ("sel", None)], 1))
    cpf = dict(Lyr=2, P=3, D=7, r=3, d1=Z, d2=Z, d3=Z, sc=1.0, out=O(), s=s)
    cases.append((lib.lpi_prompt_cp_fwd, cpf, [("r", 17), ("r", 0), ("D", 0), ("Lyr", 0), ("P", 0), ("d3", None), ("out", None), ("Lyr", 1 << 30), ("D", 1 << 30)], 1))
    cpf2 = dict(Lyr=2, P=3, Dv=7, Dt=5, r=3, d1=Z, d2v=Z, d2t=Z, d3v=Z, d3t=Z, sc=1.0, ov=O(), ot=O(), s=s)
    cases.append((lib.lpi_prompt_cp_fwd2, cpf2, [("r", 17), ("Dt", 0), ("Dv", 0), ("ot", None), ("d2t", None), ("P", 1 << 30), ("Dt", 1 << 30)], 1))
    cpb = dict(Lyr=2, P=3, D=7, r=3, d1=Z, d2=Z, d3=Z, sc=1.0, dout=Z, g1=O(), g2=O(), g3=O(), acc=0, scr=O(), s=s)
    cases.append((lib.lpi_prompt_cp_bwd, cpb, [("r", 17), ("D", 0), ("g1", None), ("g2", None), ("g3", None), ("scr", None), ("dout", None), ("Lyr", 1 << 30), ("D", 1 << 30)], 3))
    cpb2 = dict(Lyr=2, P=3, Dv=7, Dt=5, r=3, d1=Z, d2v=Z, d2t=Z, d3v=Z, d3t=Z, sc=1.0, dov=Z, dot=Z, g1=O(), g2v=O(), g2t=O(), g3v=O(), g3t=O(), scr=O(), s=s)
    cases.append((lib.lpi_prompt_cp_bwd2, cpb2, [("r", 17), ("Dt", 0), ("g3t", None), ("scr", None), ("dot", None), ("Lyr", 1 << 30), ("Dv", 1 << 30)], 2))
    al = dict(Lyr=2, P=3, Dv=7, Dt=5, vis=Z, txt=Z, temp=0.01, w=0.1, loss=O(), dv=O(), dt=O(), s=s)
    cases.append((lib.lpi_align_loss_fwd_bwd, al, [("dv", None), ("dt", None), ("temp", 0.0), ("P", 2047), ("Lyr", 0), ("Dv", 0), ("loss", None), ("vis", None)], 3))
    al2 = dict(al, scr=O(), s=s)
    al2 = {k: al2[k] for k in ("Lyr", "P", "Dv", "Dt", "vis", "txt", "temp", "w", "loss", "dv", "dt", "scr", "s")}
    cases.append((lib.lpi_align_loss_fwd_bwd2, al2, [("dv", None), ("dt", None), ("temp", 0.0), ("P", 4100), ("scr", None), ("Dt", 0), ("loss", None)], 2))
    bx = dict(T=4, D=7, row=1, X=Z, tgt=Zi, temp=0.5, w=1.0, loss=O(), dx=O(), acc=0, scr=O(), s=s)
    cases.append((lib.lpi_nt_bxent_fwd_bwd, bx, [("row", 4), ("T", 33), ("T", 0), ("D", 0), ("temp", 0.0), ("scr", None), ("loss", None), ("tgt", None), ("X", None)], 3))
    cases.append((lib.lpi_kmeans_sqdist, dict(n=n, E=7, nc=2, X=Z, ldx=10, cand=Zi, out=O(), s=s), [("ldx", 6), ("nc", 0), ("E", 0), ("n", 0), ("cand", None), ("out", None)], 1))
    ka = dict(n=n, E=7, k=2, X=Z, ldx=10, c=Z, lab=O(I32), ch=O(I32), md=O(), s=s)
    cases.append((lib.lpi_kmeans_assign, ka, [("ldx", 6), ("k", 0), ("E", 0), ("n", 0), ("c", None), ("lab", None), ("ch", None)], 1))
    ku = dict(n=n, E=7, k=2, X=Z, ldx=10, lab=Zi, nc=O(), cnt=O(), s=s)
    cases.append((lib.lpi_kmeans_update, ku, [("ldx", 6), ("k", 0), ("E", 0), ("n", 0), ("lab", None), ("nc", None), ("cnt", None)], 1))
    cases.append((lib.lpi_kmeans_colstats, dict(n=n, E=7, X=Z, ldx=10, c=None, cs=O(), cq=O(), s=s), [("ldx", 6), ("E", 0), ("n", 0), ("X", None), ("cs", None), ("cq", None)], 1))
    rk = dict(nr=3, nc=n, sc=Z, ld=n + 1, gt=Zi, gpr=2, rank=O(I32), s=s)
    cases.append((lib.lpi_retrieval_rank, rk, [("ld", n - 1), ("gpr", 0), ("nc", 0), ("nr", 0), ("gt", None), ("rank", None), ("sc", None)], 1))
    tk = dict(nr=3, nc=n, k=n, sc=Z, ld=n + 1, idx=O(I32), val=O(), s=s)
    cases.append((lib.lpi_topk, tk, [("ld", n - 1), ("k", n + 1), ("k", 0), ("nc", 0), ("nr", 0), ("idx", None), ("sc", None)], 1))
    par = {f"p{i}": Z for i in range(10)}
    ifw = dict(N=n, Dv=9, Dt=7, R=3, Lyr=2, layer=1, xv=Z, ldv=10, xt=Z, ldt=10, **par, mix=0.1, eps=1e-5, ov=O(), ldov=14, ot=O(), ldot=16, stat=O(), s=s)
    cases.append((lib.lpi_interact_fwd, ifw, [("ldv", 8), ("ldt", 6), ("ldov", 8), ("ldot", 6), ("R", 9), ("R", 0), ("Dv", 1025), ("Dt", 1025), ("layer", 2), ("layer", -1), ("N", 0),
                                              ("p3", None), ("stat", None), ("ot", None)], 1))
    nws = lib.lpi_interact_workspace_floats(n, 9, 7, 3)
    assert 0 < nws < nel - 2
    ibw = dict(N=n, Dv=9, Dt=7, R=3, Lyr=2, layer=1, xv=Z, ldv=10, xt=Z, ldt=10, **par, mix=0.1, eps=1e-5, gv=Z, ldgv=18, gt=Z, ldgt=18, dxv=O(), lddv=22, dxt=O(), lddt=22,
               grads=O(), ws=O(), s=s)
    cases.append((lib.lpi_interact_bwd, ibw, [("ldv", 8), ("ldt", 6), ("ldgv", 8), ("ldgt", 6), ("lddv", 8), ("lddt", 6), ("R", 9), ("Dv", 1025), ("layer", 2), ("N", 0),
                                              ("p9", None), ("dxv", None), ("dxt", None), ("grads", None), ("ws", None)], 2))
    # sizes whose one-thread-per-element grid would not fit 2^31 - 1 workgroups of 256 while every int index still fits (619; nothing is touched: refused first)
    big = dict(Lyr=1 << 14, P=1 << 15, r=1)
    cases[[c[0] for c in cases].index(lib.lpi_prompt_cp_fwd)][2].append((None, dict(big, D=1 << 30)))
    cases[[c[0] for c in cases].index(lib.lpi_prompt_cp_fwd2)][2].append((None, dict(big, Dv=1 << 29, Dt=1 << 29)))
    cases[[c[0] for c in cases].index(lib.lpi_sgd_step)][2].append(("n", 1 << 40))
    cases.append((lib.lpi_copy_rows, dict(rows=3, cols=n, src=Z, lds=n + 1, dst=O(), ldd=n + 3, s=s), [("lds", n - 1), ("ldd", n - 1), (None, dict(rows=1 << 30, cols=1 << 30, lds=1 << 30, ldd=1 << 30))], 1))
    # ... and EVERY required pointer as NULL, every count as 0 (whatever the lists above already hold)
    optional = {"lpi_clip_loss_fwd_bwd": {"dl"}, "lpi_ce_rows_fwd_bwd": {"dl"}, "lpi_sum_scaled": {"b"}, "lpi_l1_task_id": {"dist"}, "lpi_nt_bxent_fwd_bwd": {"dx"},
                "lpi_kmeans_assign": {"md"}, "lpi_kmeans_colstats": {"c"}, "lpi_topk": {"val"}}
    counts = {"n", "rows", "E", "T", "C", "Lyr", "P", "D", "Dv", "Dt", "r", "R", "N", "nc", "k", "nr", "gpr", "cols"}
    for fn, good, bads, _ in cases:
        have = {(k, v) for k, v in bads if k is not None and (v is None or v == 0)}
        for k, v in good.items():
            is_ptr = k != "s" and (v is None or (isinstance(v, int) and v > (1 << 32)))
            if is_ptr and v is not None and k not in optional.get(fn.__name__, set()) and (k, None) not in have:
                bads.append((k, None))
            if k in counts and (k, 0) not in have:
                bads.append((k, 0))
    n0 = _lib.launch_count()
    refused = 0
    for fn, good, bads, _ in cases:
        for k, v in bads:
            args = dict(good, **(v if k is None else {k: v}))
            assert len(args) == len(good), (fn.__name__, k)
            assert fn(*args.values()) == E, (fn.__name__, k, v)
            refused += 1
    for bad in ((0, 9, 7, 3), (n, 0, 7, 3), (n, 9, 0, 3), (n, 9, 7, 0), (n, 9, 7, 9), (n, 1025, 7, 3), (n, 9, 1025, 3)):      # the sizes lpi_interact_fwd refuses have no workspace
        assert lib.lpi_interact_workspace_floats(*bad) == E, bad
        refused += 1
    torch.cuda.synchronize()
    assert _lib.launch_count() == n0, "a refused call launched a kernel"
    for i, rec in enumerate(outs):
        assert torch.equal(S.bits(rec.arena), rec.before), f"a refused call wrote output arena {i}"
    print(f"{refused} refusals, {len(outs)} output arenas untouched")
    for fn, good, _, launches in cases:      # every argument list the refusals started from launches
        n1 = _lib.launch_count()
        assert fn(*good.values()) == 0, fn.__name__
        assert _lib.launch_count() - n1 == launches, (fn.__name__, _lib.launch_count() - n1, launches)
    torch.cuda.synchronize()
    for rec in outs:
        S.check_pads("an output arena of the refusal test", rec)      # element 0 and the last one are pads: the good calls stayed inside


def test_zz_the_worst_figure_beside_each_bar():
    """Runs last (file order): what `held` and its kin recorded, one line per bar — the figures of the commit message."""
    for what, (e, bar) in sorted(WORST.items()):
        print(f"WORST {what}: {e:.3e} (bar {bar:g})")
