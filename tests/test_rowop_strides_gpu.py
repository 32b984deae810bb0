"""The row-operation family held to its leading dimensions and its write bounds on a real MI355X: every entry point of rowops.hip and mx8_rows.hip that takes a
row stride (lpi_layernorm_fwd / _bwd / _bwd_rows(_varlen) / _fwd_pair / _bwd_pair, lpi_l2norm_*, lpi_pool_ln_*, lpi_gather_batch_rows(_varlen), lpi_scatter_add_rows,
lpi_patchify(_u8), lpi_vis_assemble_fwd, lpi_transpose(2), lpi_ln_stats_finalize_pair, every lpi_row_jobs op, lpi_mx8_quantize, lpi_layernorm_mx8_fwd) and lpi_copy_rows.

Every case is an OP: a function that builds its operands on an `Arm` and returns the call(s).  It runs twice: the STRIDED arm on tests/strided.py views (base pointer
`base` elements into its arena, every leading dimension of the case different from the width and from every other one, NaN in every pad), the TIGHT arm on contiguous
copies of the same values.  Asserted per case (tests/arms.py; tests/test_rowop_strides_host.py proves that these assertions catch a wrong stride):
  * the launch count is what the dispatch implies (1; 2 for a LayerNorm pair off the fused path and for lpi_vis_assemble_bwd), the same in both arms;
  * every must-be-written output of the strided arm equals the tight arm's bit for bit; no pad of any operand, inputs included, changed; every must-be-written
    element was written; the rows of a stream that a mapped-row kernel does not own kept their bits (strided.check_kept);
  * the tight arm meets the f64 reference at the bar of the kernel's existing test (each bar names its source where it is used; none is new).
Every arena of a case has strided.arena_bytes(largest row count — the full B x L stream for the mapped forms —, largest leading dimension, 4 bytes, largest base)
bytes, so a kernel that applies any stride of the case to any pointer of the case fails an assertion and never leaves an allocation.

Shapes: 13 rows (a partial last block at 4 and at 8 rows per block); d = 132 (the 4-element kernels: both arms on the same kernel), 136 and 520 (the half-wave 16-byte
kernels of the 2-byte types; chunk bounds 1 and 3, last chunk partial), 1032 (chunk bound 8, f32).  Mapped forms: B = 3, L = 7, P = 2, row0 = 1; ragged: row_start =
[0, 5, 12, 19], the rows behind row_start[B] are pads.  Leading dimensions: width + 4, + 8, + 12, ... elements with base 4 for the 4-element kernels — the smallest
steps their checks accept (include/lpi_hip.h, "Leading dimensions and alignment of the row operations") —, width + 8, + 16, ... with base 8 for the half-wave kernels
(again the smallest); odd steps and base 1 where a lane moves one element (transposes, copies, scale bytes).  What the checks refuse is tested to launch nothing.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import arms as A  # noqa: E402
import mx8_emulate as MX  # noqa: E402
import strided as S  # noqa: E402
from lpi_amd import _lib  # noqa: E402
from lpi_amd._lib import BF16, F16, F32, call  # noqa: E402
from poison import relerr, same_bits  # noqa: E402

DEV = "cuda:0"
TD = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
ROWS = 13
MB, ML, MP, MROW0 = 3, 7, 2, 1                      # the mapped forms
ROW_START = [0, 5, 12, 19]
# The bars (relerr = max |got - ref| / max |ref|, tests/poison.py), each from the existing test of the kernel:
TOL = {F32: 2e-5, BF16: 2e-2}                       # tests/test_kernels_gpu.py TOL: test_layernorm_fwd_bwd (y and the cast copy), the f32 kernels
LN_Y_BAR = {(F32, F32): 2e-5, (F32, BF16): 2e-2,    # test_layernorm_fwd_bwd
            (F16, BF16): 8e-3,                      # test_fp16_residual_stream_kernels
            (F16, F16): 2e-3, (F32, F16): 2e-3}     # test_layernorm_f16_output_and_pooled_attention_f16 (the f16 operand's rounding)
STAT_BAR = 1e-5                                     # test_fp16_residual_stream_kernels, test_layernorm_mx8: mean / rstd
DX_BAR = 2e-5                                       # test_layernorm_fwd_bwd: the f32 gradient stream
STREAM16_BAR = 1e-2                                 # test_layernorm_bwd_bf16_gradient_stream, test_fp16_residual_stream_kernels: the bf16 stream (dx = NULL)
SCATTER_BAR = {F32: 1e-6, BF16: 8e-3}               # test_scatter_add_rows


def stream():
    return torch.cuda.current_stream().cuda_stream


def esz(td):
    return 1 if td == torch.uint8 else 4 if td == torch.float32 else 2


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def held(what, dt, got, ref, bar):
    """Print the figure beside ITS bar (pytest -s shows it), then assert."""
    e = relerr(got, ref)
    print(f"{what} [{NAME.get(dt, dt)}]: {e:.3e} (bar {bar:g})")
    assert e < bar, (what, NAME.get(dt, dt), e, bar)


class Arm:
    """One arm's operands as strided.Records: .ops[name].  `mat` / `vec` take the STRIDED arm's leading dimension and base; the tight arm gets ld = cols, base 0.
    Every arena has `nbytes` bytes = strided.arena_bytes(max_rows, max_ld, 4, max_base): `mat` refuses an operand the sizing did not count."""

    def __init__(self, strided, max_rows, max_ld, base):
        self.strided, self.max_rows, self.max_ld, self.base, self.ops = strided, max_rows, max_ld, base, {}
        self.nbytes = S.arena_bytes(max_rows, max_ld, 4, base)

    def ld(self, cols, ld):
        return ld if self.strided else cols

    def mat(self, name, rows, cols, ld, td, fill=None, in_out=False, base=None):
        base = self.base if base is None else base
        assert rows <= self.max_rows and cols <= ld <= self.max_ld and base <= self.base and name not in self.ops, name
        rec = S.operand(rows, cols, self.ld(cols, ld), td, base if self.strided else 0, self.nbytes // esz(td), fill, DEV)
        self.ops[name] = S.in_out(rec) if in_out else rec
        return rec.t

    def vec(self, name, n, fill=None, td=torch.float32, base=None, misalign=0):
        """n elements at `base`: gamma / beta (inputs), mean / rstd / inv_norm (region outputs of exactly n values).  -> the tensor the kernel is handed.
        misalign (an input): the values start `misalign` elements behind `base` in BOTH arms, so the tight arm's pointer is off its alignment too; the
        elements in front of them belong to the footprint and hold a copy of the first values."""
        base = (self.base if base is None else base) if self.strided else 0
        assert name not in self.ops and base <= self.base and (misalign == 0 or fill is not None), name
        if misalign:
            fill = torch.cat([fill[:misalign], fill])
        rec = S.region(base + torch.arange(n + misalign), td, self.nbytes // esz(td), fill, DEV)
        self.ops[name] = rec
        return rec.t[base + misalign:base + misalign + n]

    def rows_only(self, name, rows):
        S.must_write(self.ops[name], rows=rows)

    def got(self, name):
        return self.ops[name].t if self.ops[name].t.dim() == 2 else self.ops[name].arena[self.ops[name].inside]


def run_arms(label, op, max_rows, max_ld, base, launches=1, **kw):
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
    A.check_arms(label, arms[0][0].ops, arms[1][0].ops, torch.cuda.synchronize, kept=True)
    arms[1][1](arms[1][0])
    return arms[0][0], arms[1][0]


def run_each_arm(label, op, max_rows, max_ld, base, launches, **kw):
    """For a case whose leading dimensions put the two arms on DIFFERENT kernels: launches = (strided, tight); each arm is held to its pads, its written
    elements and the f64 bars, and the arms are NOT compared bit for bit.  -> (strided arm, tight arm)"""
    arms = []
    for strided, want in zip((True, False), launches):
        arm = Arm(strided, max_rows, max_ld, base)
        run, check = op(arm, **kw)
        torch.cuda.synchronize()
        n0 = _lib.launch_count()
        run()
        torch.cuda.synchronize()
        assert _lib.launch_count() - n0 == want, (label, "strided" if strided else "tight", _lib.launch_count() - n0, want)
        for name, o in arm.ops.items():
            S.check_pads(f"{label} {name}", o)
            if o.output:
                S.check_written(f"{label} {name}", o), S.check_kept(f"{label} {name}", o)
        check(arm)
        arms.append(arm)
    return arms


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------------------------------------
def ln_values(rows, d, xdt, seed=5):
    x = (rnd(rows, d, seed=seed) * 2 + 0.3) if xdt == F32 else (rnd(rows, d, seed=seed) * 3 + 0.5).half()      # the existing tests' inputs
    return x, 1 + 0.1 * rnd(d, seed=seed + 1), 0.05 * rnd(d, seed=seed + 2)


def stats64(x):
    x = x.double()
    return x.mean(1), 1 / torch.sqrt(x.var(1, unbiased=False) + 1e-5)


def op_ln_fwd(arm, xdt, ydt, d, u, rows=ROWS, tag="", k=0, ldx=None, ldy=None):
    """lpi_layernorm_fwd; ydt None: statistics only.  u: 4 (4-element kernels) or 8 (half-wave); k shifts the leading dimensions (pairs: all four different)."""
    x, gam, bet = ln_values(rows, d, xdt, seed=5 + 10 * k)
    X = arm.mat(tag + "x", rows, d, ldx or d + u * (1 + 2 * k), TD[xdt], x)
    G, Bt = (arm.vec(tag + "gamma", d, gam), arm.vec(tag + "beta", d, bet)) if ydt is not None else (None, None)
    Y = arm.mat(tag + "y", rows, d, ldy or d + u * (2 + 2 * k), TD[ydt]) if ydt is not None else None
    mean, rstd = arm.vec(tag + "mean", rows), arm.vec(tag + "rstd", rows)
    args = (rows, d, X, X.stride(0), G, Bt, Y, Y.stride(0) if Y is not None else 0, mean, rstd)

    def run():
        call("lpi_layernorm_fwd", ydt if ydt is not None else BF16, xdt, *args, stream())

    def check(t):
        m, r = stats64(x)
        held("layernorm mean", xdt, t.got(tag + "mean"), m, STAT_BAR)
        held("layernorm rstd", xdt, t.got(tag + "rstd"), r, STAT_BAR)
        if ydt is not None:
            ref = torch.nn.functional.layer_norm(x.double(), (d,), gam.double(), bet.double(), 1e-5)
            held("layernorm y", ydt, t.got(tag + "y"), ref, LN_Y_BAR[(xdt, ydt)])
    run.args, run.dts = args, (ydt if ydt is not None else BF16, xdt)
    return run, check


LNF4 = [(F32, F32, 132), (F32, F32, 136), (F32, F32, 520), (F32, F32, 1032), (F32, BF16, 132), (F32, BF16, 520), (F32, F16, 132), (F32, F16, 520),
        (F16, BF16, 132), (F16, F16, 132)]
LNF8 = [(F16, BF16, 136), (F16, BF16, 520), (F16, F16, 136), (F16, F16, 520), (F16, None, 136), (F16, None, 520)]


@pytest.mark.parametrize("xdt,ydt,d,u", [c + (4,) for c in LNF4] + [c + (8,) for c in LNF8], ids=lambda v: NAME.get(v, str(v)) if v is None or v < 3 else str(v))
def test_layernorm_forward(xdt, ydt, d, u):
    run_arms(f"ln_fwd {NAME[xdt]} -> {NAME.get(ydt, 'statistics')} {d}", op_ln_fwd, ROWS, d + 2 * u, u, xdt=xdt, ydt=ydt, d=d, u=u)


@pytest.mark.parametrize("ydt", [BF16, F16], ids=["bf16", "f16"])
def test_a_leading_dimension_of_4_mod_8_moves_the_fp16_stream_to_the_4_element_kernel(ydt):
    """d = 136, f16 stream: ldx = d + 4 fails the half-wave kernel's condition, so the STRIDED arm runs ln_fwd_kernel and the tight arm ln_fwd_h16_kernel.  The strided
    arm is held to the f64 bar, not to the tight arm's bits; whether the two kernels' bits agree is printed (an observation, recorded in DESIGN.md), not asserted."""
    d = 136
    outs = run_each_arm(f"ln_fwd 4 mod 8 {NAME[ydt]}", op_ln_fwd, ROWS, d + 8, 4, (1, 1), xdt=F16, ydt=ydt, d=d, u=4)
    for kk in ("y", "mean", "rstd"):
        s, t = outs[0].got(kk).contiguous(), outs[1].got(kk).contiguous()
        print(f"OBSERVATION 4-element vs half-wave kernel, {NAME[ydt]} {kk}: {int((S.bits(s) != S.bits(t)).sum())} of {t.numel()} values differ in their bits")


KINDS = dict(FFF=(F32, F32, F32), FFB=(F32, F32, BF16), FBB=(F32, BF16, BF16), FBF=(F32, BF16, F32), HBB=(F16, BF16, BF16), H16=(F16, BF16, BF16))      # x, dy, cast


def mapped_rows(ragged):
    starts = ROW_START[:MB] if ragged else [b * ML for b in range(MB)]
    return [s + MROW0 + p for s in starts for p in range(MP)], (ROW_START[MB] if ragged else MB * ML)


def op_ln_bwd(arm, kind, d, mode, acc, mapped=None, tag="", k=0, job=False, lds=None):
    """lpi_layernorm_bwd (mapped None) / lpi_layernorm_bwd_rows (mapped "uniform") / _rows_varlen ("ragged").  mode: "both" (dx and dx_cast), "dx", "cast" (dx = NULL:
    the cast copy is the gradient stream).  job: lddx == ldcast (LPI_ROWOP_LN_BWD has the one ld_c for both)."""
    xdt, dydt, cdt = KINDS[kind]
    u = 8 if kind == "H16" else 4
    if mapped:
        mrows, srows = mapped_rows(mapped == "ragged")
        rows = MB * MP
    else:
        rows = srows = ROWS
        mrows = list(range(rows))
    xs, gam, _ = ln_values(srows, d, xdt, seed=5 + 10 * k)
    dy = rnd(rows, d, seed=8 + 10 * k).to(TD[dydt])
    dx0 = rnd(srows, d, seed=9 + 10 * k)
    m, r = stats64(xs)
    dead = torch.ones(srows, dtype=torch.bool)
    dead[mrows] = False
    xin, m_in, r_in = xs.clone(), m.float(), r.float()
    xin[dead], m_in[dead], r_in[dead] = float("nan"), float("nan"), float("nan")      # the rows a mapped call does not own: read into a result they show
    lds = list(lds) if lds else [d + u * (i + 1 + 4 * k) for i in range(4)]      # lddy, ldx, lddx, ldcast
    if job:
        lds[3] = lds[2]
    DY = arm.mat(tag + "dy", rows, d, lds[0], TD[dydt], dy)
    X = arm.mat(tag + "x", srows, d, lds[1], TD[xdt], xin)
    G, MEAN, RSTD = arm.vec(tag + "gamma", d, gam), arm.vec(tag + "mean", srows, m_in), arm.vec(tag + "rstd", srows, r_in)
    DX = CAST = None
    if mode != "cast":
        DX = arm.mat(tag + "dx", srows, d, lds[2], torch.float32, dx0 if acc else None, in_out=bool(acc))
        arm.rows_only(tag + "dx", mrows)
    if mode != "dx":
        cast_in = mode == "cast" and acc      # with dx present the cast copy is written, never read
        CAST = arm.mat(tag + "cast", srows, d, lds[3], TD[cdt], dx0.to(TD[cdt]) if cast_in else None, in_out=bool(cast_in))
        arm.rows_only(tag + "cast", mrows)
    tail = (DY, DY.stride(0), X, X.stride(0), G, MEAN, RSTD, DX, arm.ld(d, lds[2]), CAST, arm.ld(d, lds[3]), acc)
    rs = torch.tensor(ROW_START, dtype=torch.int32, device=DEV) if mapped == "ragged" else None      # (row_start / idx: int32 inputs no kernel writes; plain tensors)

    def run():
        if mapped == "ragged":
            call("lpi_layernorm_bwd_rows_varlen", dydt, cdt, xdt, MB, ML, rs, MROW0, MP, d, *tail, stream())
        elif mapped:
            call("lpi_layernorm_bwd_rows", dydt, cdt, xdt, MB, ML, MROW0, MP, d, *tail, stream())
        else:
            call("lpi_layernorm_bwd", dydt, cdt, xdt, rows, d, *tail, stream())

    def check(t):
        xr = xs[mrows].double().requires_grad_(True)
        torch.nn.functional.layer_norm(xr, (d,), gam.double(), None, 1e-5).backward(dy.double())
        if DX is not None:
            held("layernorm dx", F32, t.got(tag + "dx")[mrows], xr.grad + (dx0[mrows].double() if acc else 0), DX_BAR)
        if CAST is not None:
            base = (dx0 if mode == "both" else dx0.to(TD[cdt]))[mrows].double() if acc else 0
            bar = TOL[cdt] if mode == "both" or cdt == F32 else STREAM16_BAR
            held("layernorm dx_cast" if mode == "both" else "layernorm gradient stream", cdt, t.got(tag + "cast")[mrows], xr.grad + base, bar)
    run.tail, run.dts, run.rows = tail, (dydt, cdt, xdt), rows
    return run, check


LNB = [(kind, 132, mode, acc) for kind in ("FFF", "FFB", "FBB", "FBF", "HBB") for mode in (("both", "dx", "cast") if kind == "FFF" else ("both", "cast")) for acc in (0, 1)]
LNB += [("H16", 136, "cast", 0), ("H16", 136, "cast", 1), ("H16", 520, "cast", 1), ("FFF", 1032, "both", 1), ("FBB", 520, "both", 1)]


@pytest.mark.parametrize("kind,d,mode,acc", LNB)
def test_layernorm_backward(kind, d, mode, acc):
    u = 8 if kind == "H16" else 4
    run_arms(f"ln_bwd {kind} {d} {mode} acc={acc}", op_ln_bwd, ROWS, d + 4 * u, u, kind=kind, d=d, mode=mode, acc=acc)


@pytest.mark.parametrize("mapped", ["uniform", "ragged"])
@pytest.mark.parametrize("kind,d,mode,acc", [("FFF", 132, "dx", 1), ("FBB", 132, "both", 0), ("HBB", 132, "cast", 1), ("H16", 136, "cast", 1), ("H16", 136, "cast", 0)])
def test_layernorm_backward_of_mapped_rows(kind, d, mode, acc, mapped):
    """compact dy at lddy; x, the statistics and the gradient stream at the mapped rows of the full stream (ldx / lddx / ldcast); every other stream row keeps its bits."""
    u = 8 if kind == "H16" else 4
    run_arms(f"ln_bwd_rows {kind} {mode} acc={acc} {mapped}", op_ln_bwd, MB * ML, d + 4 * u, u, kind=kind, d=d, mode=mode, acc=acc, mapped=mapped)


def op_ln_fwd_pair(arm, ydt, d0, d1, u1, ldx1=None, ldy1=None):
    r0, c0 = op_ln_fwd(arm, F16, ydt, d0, 8, rows=ROWS, tag="p0.", k=0)
    r1, c1 = op_ln_fwd(arm, F16, ydt, d1, u1, rows=9, tag="p1.", k=1, ldx=ldx1, ldy=ldy1)      # (the tight arm takes ld = d whatever is asked for)

    def run():
        _lib.layernorm_fwd_pair(r0.dts[0], F16, r0.args, r1.args, stream())
    return run, lambda t: (c0(t), c1(t))


@pytest.mark.parametrize("ydt", [BF16, F16, None], ids=["bf16", "f16", "statistics"])
def test_layernorm_forward_pair_on_the_fused_path_is_one_launch(ydt):
    run_arms(f"ln_fwd_pair {ydt}", op_ln_fwd_pair, ROWS, 520 + 32, 8, ydt=ydt, d0=520, d1=136, u1=8)


def test_layernorm_forward_pair_off_the_fused_path_is_two_launches():
    """problem 1: d = 132 with ldx = 140 (4 mod 8) -> no fused launch; both arms run problem 1 on the 4-element kernel (d % 8 != 0), problem 0 on the half-wave one."""
    run_arms("ln_fwd_pair 2 launches", op_ln_fwd_pair, ROWS, 520 + 32, 8, launches=2, ydt=BF16, d0=520, d1=132, u1=4, ldx1=140)


def op_ln_bwd_pair(arm, d1, kind1, lds1=None):
    r0, c0 = op_ln_bwd(arm, "H16", 520, "cast", 1, tag="p0.", k=0)
    r1, c1 = op_ln_bwd(arm, kind1, d1, "cast", 0, tag="p1.", k=1, lds=lds1)

    def run():
        _lib.layernorm_bwd_pair(BF16, BF16, F16, (r0.rows, 520) + r0.tail, (r1.rows, d1) + r1.tail, stream())
    return run, lambda t: (c0(t), c1(t))


@pytest.mark.parametrize("d1,kind1,launches", [(136, "H16", 1), (132, "HBB", 2)])
def test_layernorm_backward_pair(d1, kind1, launches):
    """(136, H16): both problems on the half-wave kernel, one launch.  (132, HBB): d = 132 is no multiple of 8, which pushes problem 1 (and with it the pair) off it: two launches."""
    run_arms(f"ln_bwd_pair {d1}", op_ln_bwd_pair, ROWS, 520 + 8 * 8, 8, launches=launches, d1=d1, kind1=kind1)


@pytest.mark.parametrize("which", ["ldx", "ldy", "lddy", "ldx (backward)", "ldcast"])
def test_one_leading_dimension_of_4_mod_8_takes_a_pair_off_the_fused_path(which):
    """d = 136 in problem 1, every pointer 16-byte aligned, every leading dimension a multiple of 8 but ONE (4 mod 8): that term alone decides the pair's dispatch.
    The strided arm runs two launches (problem 1 on the 4-element kernel), the tight arm the one fused launch: different kernels, so each arm is held to its pads
    and the f64 bars, not to the other's bits.  A pair dispatch that ignored ldx, ldy, lddy or ldcast would launch once and fail the count."""
    d = 136
    if which in ("ldx", "ldy"):
        ld = dict(ldx1=160, ldy1=168)
        ld[which + "1"] += 4
        run_each_arm(f"ln_fwd_pair {which} 4 mod 8", op_ln_fwd_pair, ROWS, 520 + 32, 8, (2, 1), ydt=BF16, d0=520, d1=d, u1=8, **ld)
    else:
        lds = [d + 40, d + 48, d + 56, d + 64]      # lddy, ldx, lddx (dx = NULL: only its low bits are looked at), ldcast
        lds[{"lddy": 0, "ldx (backward)": 1, "ldcast": 3}[which]] += 4
        run_each_arm(f"ln_bwd_pair {which} 4 mod 8", op_ln_bwd_pair, ROWS, 520 + 8 * 8, 8, (2, 1), d1=d, kind1="HBB", lds1=lds)


# ---- L2 norm, pooled heads, gather / scatter --------------------------------------------------------------------------------------------------------------------------
def op_l2norm_fwd(arm, k=0, E=132, B=ROWS):
    x = rnd(B, E, seed=3 + k)
    X, Y, INV = arm.mat("x", B, E, E + 4 + 12 * k, torch.float32, x), arm.mat("y", B, E, E + 8 + 12 * k, torch.float32), arm.vec("inv", B)

    def run():
        call("lpi_l2norm_fwd", B, E, X, X.stride(0), Y, Y.stride(0), INV, stream())

    def check(t):      # no f64 test of its own exists (test_round4_gpu.py compares launches): the f32 bar of tests/test_kernels_gpu.py
        n = x.double().norm(dim=1, keepdim=True)
        held("l2norm y", F32, t.got("y"), x.double() / n, TOL[F32])
        held("l2norm inv_norm", F32, t.got("inv"), 1 / n[:, 0], TOL[F32])
    run.job = lambda: _lib.row_job(_lib.ROWOP_L2NORM_FWD, B=B, d=E, a=X, ld_a=X.stride(0), out=Y, ld_c=Y.stride(0), mean=INV)
    return run, check


def op_l2norm_bwd(arm, k=0, E=132, B=ROWS, copy=False):
    x, dy = rnd(B, E, seed=3 + k), rnd(B, E, seed=23 + k)
    n = x.double().norm(dim=1, keepdim=True)
    y = (x.double() / n).float()
    Y, DY = arm.mat("y", B, E, E + 4 + 12 * k, torch.float32, y), arm.mat("dy", B, E, E + 8 + 12 * k, torch.float32, dy)
    INV, DX = arm.vec("inv", B, (1 / n[:, 0]).float()), arm.mat("dx", B, E, E + 12 + 12 * k, torch.float32)
    DX16 = arm.mat("dx16", B, E, E + 12 + 12 * k, torch.bfloat16) if copy else None      # the job's bf16 copy: the same row stride as dx

    def run():
        call("lpi_l2norm_bwd", B, E, Y, Y.stride(0), DY, DY.stride(0), INV, DX, DX.stride(0), stream())

    def check(t):
        yy, g = y.double(), dy.double()
        held("l2norm dx", F32, t.got("dx"), (g - yy * (yy * g).sum(1, keepdim=True)) / n, TOL[F32])
    run.job = lambda: _lib.row_job(_lib.ROWOP_L2NORM_BWD, B=B, d=E, a=Y, ld_a=Y.stride(0), b=DY, ld_b=DY.stride(0), mean_in=INV, out=DX, ld_c=DX.stride(0), out2=DX16,
                                   dt_b=BF16)
    return run, check


def test_l2norm():
    run_arms("l2norm_fwd", op_l2norm_fwd, ROWS, 132 + 12, 4)
    run_arms("l2norm_bwd", op_l2norm_bwd, ROWS, 132 + 12, 4)


POOL_IDX = [0, 6, 3]


def pool_index(how):
    """-> (L argument, idx tensor or None, the pooled rows of the [MB * ML, d] stream)"""
    if how == "cls":
        return ML, None, [b * ML for b in range(MB)]
    rows = [b * ML + i for b, i in enumerate(POOL_IDX)]
    if how == "relative":
        return ML, torch.tensor(POOL_IDX, dtype=torch.int32, device=DEV), rows
    return 0, torch.tensor(rows, dtype=torch.int32, device=DEV), rows


def op_pool_ln_fwd(arm, xdt=F32, ydt=F32, how="relative", d=132, k=0, raw=False):
    x, gam, bet = ln_values(MB * ML, d, xdt, seed=20 + k)
    L, idx, prow = pool_index(how)
    X = arm.mat("x", MB * ML, d, d, TD[xdt], x)      # the stream has no row stride of its own: [B L, d] at an offset base
    G, Bt = arm.vec("gamma", d, gam), arm.vec("beta", d, bet)
    Y, MEAN, RSTD = arm.mat("y", MB, d, d + 4 + 4 * k, TD[ydt]), arm.vec("mean", MB), arm.vec("rstd", MB)
    RAW = arm.mat("raw", MB, d, d, torch.float32) if raw else None

    def run():
        call("lpi_pool_ln_fwd", ydt, xdt, MB, L, d, X, idx, G, Bt, Y, Y.stride(0), MEAN, RSTD, stream())
        if raw:
            call("lpi_gather_rows", xdt, MB, L, d, X, idx, RAW, stream())

    def check(t):      # tests/test_dead_memory_gpu.py piece_pool_ln_fwd: 2e-5 / 8e-3 / 2e-3 by output type (= LN_Y_BAR), statistics 1e-5
        xp = x[prow].double()
        m, r = stats64(xp)
        held("pool_ln y", ydt, t.got("y"), torch.nn.functional.layer_norm(xp, (d,), gam.double(), bet.double(), 1e-5), LN_Y_BAR[(xdt, ydt)])
        held("pool_ln mean", xdt, t.got("mean"), m, STAT_BAR)
        held("pool_ln rstd", xdt, t.got("rstd"), r, STAT_BAR)
    run.job = lambda: _lib.row_job(_lib.ROWOP_POOL_LN_FWD, B=MB, L=L, d=d, dt_a=xdt, dt_b=ydt, a=X, idx=idx, gamma=G, beta=Bt, out=Y, ld_c=Y.stride(0), mean=MEAN, rstd=RSTD,
                                   out2=RAW)
    return run, check


def op_pool_ln_bwd(arm, cdt=BF16, how="relative", d=132, k=0):
    x, gam, _ = ln_values(MB * ML, d, F32, seed=23 + k)
    dy = rnd(MB, d, seed=25 + k)
    L, idx, prow = pool_index(how)
    m, r = stats64(x[prow])
    DY, X = arm.mat("dy", MB, d, d + 4 + 4 * k, torch.float32, dy), arm.mat("x", MB * ML, d, d, torch.float32, x)
    G, MEAN, RSTD = arm.vec("gamma", d, gam), arm.vec("mean", MB, m.float()), arm.vec("rstd", MB, r.float())
    DX, CAST = arm.mat("dx", MB * ML, d, d, torch.float32), arm.mat("cast", MB * ML, d, d, TD[cdt])
    arm.rows_only("dx", prow), arm.rows_only("cast", prow)

    def run():
        call("lpi_pool_ln_bwd", cdt, MB, L, d, DY, DY.stride(0), X, idx, G, MEAN, RSTD, DX, CAST, stream())

    def check(t):      # tests/test_dead_memory_gpu.py piece_pool_ln_bwd (test_layernorm_fwd_bwd): dx 2e-5, the cast copy TOL
        xr = x[prow].double().requires_grad_(True)
        torch.nn.functional.layer_norm(xr, (d,), gam.double(), None, 1e-5).backward(dy.double())
        held("pool_ln dx", F32, t.got("dx")[prow], xr.grad, DX_BAR)
        held("pool_ln dx_cast", cdt, t.got("cast")[prow], xr.grad, TOL[cdt])
    run.job = lambda: _lib.row_job(_lib.ROWOP_POOL_LN_BWD, B=MB, L=L, d=d, dt_b=cdt, a=DY, ld_a=DY.stride(0), b=X, idx=idx, gamma=G, mean_in=MEAN, rstd_in=RSTD, out=DX,
                                   out2=CAST)
    return run, check


@pytest.mark.parametrize("how", ["cls", "relative", "absolute"])
def test_pooled_layernorm(how):
    run_arms(f"pool_ln_fwd f32 {how}", op_pool_ln_fwd, MB * ML, 132 + 4, 4, how=how)
    run_arms(f"pool_ln_fwd f16->bf16 {how}", op_pool_ln_fwd, MB * ML, 132 + 4, 4, how=how, xdt=F16, ydt=BF16)
    run_arms(f"pool_ln_bwd {how}", op_pool_ln_bwd, MB * ML, 132 + 4, 4, how=how, cdt=BF16 if how != "cls" else F32)


def op_gather(arm, dt=BF16, ragged=False, cols=136, k=0):
    mrows, srows = mapped_rows(ragged)
    src = rnd(srows, cols, seed=9 + k).to(TD[dt])
    u = 16 // esz(TD[dt])
    SRC, DST = arm.mat("src", srows, cols, cols + u * (1 + 2 * k), TD[dt], src), arm.mat("dst", MB * MP, cols, cols + u * (2 + 2 * k), TD[dt])
    rs = torch.tensor(ROW_START, dtype=torch.int32, device=DEV) if ragged else None

    def run():
        if ragged:
            call("lpi_gather_batch_rows_varlen", dt, MB, ML, rs, MROW0, MP, cols, SRC, SRC.stride(0), DST, DST.stride(0), stream())
        else:
            call("lpi_gather_batch_rows", dt, MB, ML, MROW0, MP, cols, SRC, SRC.stride(0), DST, DST.stride(0), stream())

    def check(t):      # test_row_kernels_varlen: a copy, bit for bit
        assert same_bits(t.got("dst").contiguous().cpu(), src[mrows].contiguous())
    run.job = lambda: _lib.row_job(_lib.ROWOP_GATHER_BATCH_ROWS, B=MB, L=ML, row_start=rs, row0=MROW0, P=MP, d=cols // u, a=SRC, ld_a=SRC.stride(0) // u, out=DST,
                                   ld_c=DST.stride(0) // u)
    return run, check


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_gather_batch_rows(dt, ragged):
    u = 16 // esz(TD[dt])
    run_arms("gather_batch_rows", op_gather, MB * ML, 136 + 2 * u, u, dt=dt, ragged=ragged)


def op_scatter_add(arm, dt=BF16, how="relative", d=132, k=0):
    L, idx, prow = pool_index(how)
    dst0, src = rnd(MB * ML, d, seed=31 + k).to(TD[dt]), rnd(MB, d, seed=32 + k).to(TD[dt])
    SRC = arm.mat("src", MB, d, d + 4 + 8 * k, TD[dt], src)
    DST = arm.mat("dst", MB * ML, d, d + 8 + 8 * k, TD[dt], dst0, in_out=True)
    arm.rows_only("dst", prow)

    def run():
        call("lpi_scatter_add_rows", dt, MB, L, d, SRC, SRC.stride(0), idx, DST, DST.stride(0), stream())

    def check(t):
        held("scatter_add", dt, t.got("dst")[prow], dst0[prow].double() + src.double(), SCATTER_BAR[dt])
    run.job = lambda: _lib.row_job(_lib.ROWOP_SCATTER_ADD, B=MB, L=L, d=d, dt_a=dt, a=SRC, ld_a=SRC.stride(0), idx=idx, out=DST, ld_c=DST.stride(0))
    return run, check


@pytest.mark.parametrize("how", ["cls", "relative", "absolute"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_scatter_add_rows(dt, how):
    run_arms("scatter_add_rows", op_scatter_add, MB * ML, 132 + 8, 4, dt=dt, how=how)


# ---- vision front end -------------------------------------------------------------------------------------------------------------------------------------------------
def op_patchify(arm, dt, u8=False, vector=True):
    B, R, ps = 2, 8, 4
    G, K = R // ps, 3 * ps * ps
    Kp = 64      # K = 48 rounded up to the 128-byte block of either element size (32 f32 / 64 two-byte elements)
    pix = torch.randint(0, 256, (B, 3, R, R), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    lut = torch.stack([(torch.arange(256).float() / 255 - m) / s for m, s in ((0.48, 0.27), (0.46, 0.26), (0.41, 0.28))])
    img = torch.stack([lut[c][pix[:, c].long()] for c in range(3)], 1)
    if u8:
        IMG = arm.vec("image", pix.numel(), pix.reshape(-1), torch.uint8, base=4)
        LUT = arm.vec("lut", 768, lut.reshape(-1))
    else:
        IMG = arm.vec("image", img.numel(), img.reshape(-1), misalign=0 if vector else 1)      # one element off 16 bytes in both arms -> the scalar image path
    COLS = arm.mat("cols", B * G * G, Kp, Kp + 4, TD[dt])

    def run():
        if u8:
            call("lpi_patchify_u8", dt, B, R, ps, IMG, LUT, COLS, COLS.stride(0), stream())
        else:
            call("lpi_patchify", dt, B, R, ps, IMG, COLS, COLS.stride(0), stream())

    def check(t):      # an im2col moves values: equality with the rounded pixels, zeros in columns K .. Kp (test_uint8_pixels_give_the_f32_pipelines_features_bit_for_bit)
        ref = torch.zeros(B * G * G, Kp)
        ref[:, :K] = img.reshape(B, 3, G, ps, G, ps).permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, K)
        assert same_bits(t.got("cols").contiguous().cpu(), ref.to(TD[dt]))
    return run, check


@pytest.mark.parametrize("path", ["vector", "scalar", "u8"])
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_patchify(dt, path):
    """ldcols = Kp + 4; the zero columns K .. Kp are part of the footprint.  The scalar image path is taken by an image that is not 16-byte aligned: the tight arm's image
    sits at base 0 and would take the vector path, so this case starts it one element later in BOTH arms (Arm.vec, misalign; the columns are what the arms differ in)."""
    run_arms(f"patchify {path}", op_patchify, 16, 68, 4, dt=dt, u8=path == "u8", vector=path != "scalar")


def op_vis_assemble(arm, xdt, stats):
    B, G2, P, d = 2, 4, 2, 132
    L = 1 + P + G2
    pe, cls, pos, pr = rnd(B * G2, d, seed=1) * 2, rnd(d, seed=2), rnd(1 + G2, d, seed=3), rnd(B * P, d, seed=4)
    gam, bet = 1 + 0.2 * rnd(d, seed=5), 0.1 * rnd(d, seed=6)
    PE = arm.mat("patch_emb", B * G2, d, d + 4, torch.float32, pe)
    CLS, POS, PR = arm.vec("cls", d, cls), arm.vec("pos", (1 + G2) * d, pos.reshape(-1)), arm.vec("prompt0", B * P * d, pr.reshape(-1))
    G, Bt = arm.vec("gamma", d, gam), arm.vec("beta", d, bet)
    X0, MEAN, RSTD = arm.mat("x0", B * L, d, d, TD[xdt]), arm.vec("mean", B * L), arm.vec("rstd", B * L)
    OM, OR = (arm.vec("out_mean", B * L), arm.vec("out_rstd", B * L)) if stats else (None, None)

    def run():
        call("lpi_vis_assemble_fwd", xdt, B, G2, P, d, PE, PE.stride(0), CLS, POS, PR, P * d, G, Bt, X0, MEAN, RSTD, OM, OR, stream())

    def check(t):
        pre = torch.cat([torch.cat([(cls + pos[0])[None], pr[b * P:(b + 1) * P], pe[b * G2:(b + 1) * G2] + pos[1:]]) for b in range(B)]).double()
        m, r = stats64(pre)
        ref = torch.nn.functional.layer_norm(pre, (d,), gam.double(), bet.double(), 1e-5)
        held("vis_assemble x0", xdt, t.got("x0"), ref, LN_Y_BAR[(F32, xdt)])      # an f32 row through LayerNorm into x_dtype: the LayerNorm bars
        held("vis_assemble mean", F32, t.got("mean"), m, STAT_BAR)
        held("vis_assemble rstd", F32, t.got("rstd"), r, STAT_BAR)
        if stats:      # test_row_kernels_leave_the_layernorm_statistics_of_the_rows_they_write: close() = 2e-6 of max(1, |mean|), rstd to 2e-6 relative
            sm, sr = stats64(t.got("x0").cpu())
            assert float((t.got("out_mean").cpu().double() - sm).abs().max()) <= 2e-6 * max(1.0, float(sm.abs().max()))
            assert float((t.got("out_rstd").cpu().double() / sr - 1).abs().max()) <= 2e-6
    return run, check


@pytest.mark.parametrize("stats", [False, True], ids=["", "row statistics"])
@pytest.mark.parametrize("xdt", [F32, F16], ids=["f32", "f16"])
def test_vis_assemble_forward(xdt, stats):
    run_arms("vis_assemble_fwd", op_vis_assemble, 14, 136, 4, xdt=xdt, stats=stats)


# ---- one element per lane: transposes, copies, the statistics finalize ----------------------------------------------------------------------------------------------
def op_transpose(arm, dt, pair):
    shapes = [(37, 45), (21, 50)] if pair else [(37, 45)]
    srcs = [rnd(r, c, seed=40 + i).to(TD[dt]) for i, (r, c) in enumerate(shapes)]
    args = []
    for i, ((r, c), s) in enumerate(zip(shapes, srcs)):
        SRC, DST = arm.mat(f"src{i}", r, c, c + 3 + 10 * i, TD[dt], s), arm.mat(f"dst{i}", c, r, r + 5 + 10 * i, TD[dt])
        args += [r, c, SRC, SRC.stride(0), DST, DST.stride(0)]

    def run():
        call("lpi_transpose2" if pair else "lpi_transpose", dt, *args, stream())

    def check(t):      # test_transpose_pair: equality
        for i, s in enumerate(srcs):
            assert same_bits(t.got(f"dst{i}").contiguous().cpu(), s.t().contiguous())
    return run, check


def test_transposes():
    for dt in (F32, BF16):
        run_arms("transpose", op_transpose, 50, 63, 1, dt=dt, pair=False)
    run_arms("transpose2", op_transpose, 50, 63, 1, dt=F32, pair=True)


def op_copy_rows(arm):
    src = rnd(ROWS, 45, seed=3)
    SRC, DST = arm.mat("src", ROWS, 45, 52, torch.float32, src), arm.mat("dst", ROWS, 45, 49, torch.float32)

    def run():
        call("lpi_copy_rows", ROWS, 45, SRC, SRC.stride(0), DST, DST.stride(0), stream())
    return run, lambda t: same_bits(t.got("dst").contiguous().cpu(), src) or pytest.fail("copy_rows")      # test_copy_rows_and_score_matrix: equality


def test_copy_rows():
    run_arms("copy_rows", op_copy_rows, ROWS, 52, 1)


def op_stats_finalize_pair(arm):
    probs = [(ROWS, 256, 17), (9, 128, 12)]      # rows, d, ld of the slot buffer [2 d / 128, ld]: ld0 != ld1, both > rows
    xs = [(rnd(r, d, seed=50 + i) * 3 + 0.7).half() for i, (r, d, _) in enumerate(probs)]
    args = []
    for i, ((r, d, ld), x) in enumerate(zip(probs, xs)):
        blocks = x.float().reshape(r, d // 128, 128)
        part = torch.stack([blocks.sum(2), (blocks * blocks).sum(2)], 2).reshape(r, 2 * (d // 128)).t().contiguous()      # slot 2 j: sums, 2 j + 1: sums of squares
        PART = arm.mat(f"part{i}", 2 * (d // 128), r, ld, torch.float32, part)
        args += [r, d, PART, PART.stride(0), arm.vec(f"mean{i}", r), arm.vec(f"rstd{i}", r)]

    def run():
        call("lpi_ln_stats_finalize_pair", *args, 1e-5, stream())

    def check(t):      # test_gemm_residual_epilogue_with_row_statistics: |mean - ref| < 1e-5, |rstd std - 1| < 2e-5
        for i, x in enumerate(xs):
            xd = x.double()
            assert float((t.got(f"mean{i}").cpu().double() - xd.mean(1)).abs().max()) < 1e-5
            assert float((t.got(f"rstd{i}").cpu().double() * xd.std(1, unbiased=False).clamp_min(1e-3) - 1).abs().max()) < 2e-5
    return run, check


def test_ln_stats_finalize_pair():
    run_arms("ln_stats_finalize_pair", op_stats_finalize_pair, ROWS, 17, 1)


# ---- MX-FP8 rows ------------------------------------------------------------------------------------------------------------------------------------------------------
def op_mx8_quantize(arm, xdt, K=160):
    x = (rnd(ROWS, K, seed=K) * torch.exp(rnd(ROWS, 1, seed=K + 1))).to(TD[xdt])
    x[3, 64:96] = 0.0
    X = arm.mat("x", ROWS, K, K + 4, TD[xdt], x)
    Q = arm.mat("q", ROWS, K, K + 8, torch.uint8, base=4)
    SC = arm.mat("scales", ROWS, K // 32, K // 32 + 3, torch.uint8, base=3)      # scale bytes are stored one at a time: any step, any pointer

    def run():
        call("lpi_mx8_quantize", xdt, ROWS, K, X, X.stride(0), Q, Q.stride(0), SC, SC.stride(0), stream())

    def check(t):      # tests/test_mx8_gpu.py test_quantize_bit_for_bit: equality with the CPU restatement of the format
        qr, sr = MX.quantize(x)
        assert torch.equal(t.got("scales").cpu(), sr) and torch.equal(t.got("q").cpu(), qr)
    return run, check


def op_ln_mx8(arm, xdt, d):
    x = (rnd(ROWS, d, seed=d) * torch.exp(0.5 * rnd(ROWS, 1, seed=d + 1)) + rnd(ROWS, 1, seed=d + 2)).to(TD[xdt])
    x[::7, 3] *= 40.0
    gam, bet = 1.0 + 0.2 * rnd(d, seed=3), 0.1 * rnd(d, seed=4)
    X, G, Bt = arm.mat("x", ROWS, d, d + 4, TD[xdt], x), arm.vec("gamma", d, gam), arm.vec("beta", d, bet)
    Q, SC = arm.mat("q", ROWS, d, d + 8, torch.uint8, base=4), arm.mat("scales", ROWS, d // 32, d // 32 + 3, torch.uint8, base=3)
    MEAN, RSTD = arm.vec("mean", ROWS), arm.vec("rstd", ROWS)

    def run():
        call("lpi_layernorm_mx8_fwd", xdt, ROWS, d, X, X.stride(0), G, Bt, Q, Q.stride(0), SC, SC.stride(0), MEAN, RSTD, stream())

    def check(t):      # tests/test_mx8_gpu.py test_layernorm_mx8: statistics 1e-5, no element outside the format's bound (widened by 2e-6 |y|)
        m, r = stats64(x)
        y = (x.double() - m[:, None]) * r[:, None] * gam.double() + bet.double()
        held("layernorm_mx8 mean", xdt, t.got("mean"), m, STAT_BAR)
        held("layernorm_mx8 rstd", xdt, t.got("rstd"), r, STAT_BAR)
        assert MX.bound_violations(y, t.got("q").contiguous(), t.got("scales").contiguous(), widen=2e-6 * y.abs()) == 0
    return run, check


@pytest.mark.parametrize("xdt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_mx8_quantize(xdt):
    run_arms("mx8_quantize", op_mx8_quantize, ROWS, 168, 4, xdt=xdt)


@pytest.mark.parametrize("d", [160, 544])
@pytest.mark.parametrize("xdt", [F32, F16], ids=["f32", "f16"])
def test_layernorm_mx8(xdt, d):
    run_arms("layernorm_mx8_fwd", op_ln_mx8, ROWS, d + 8, 4, xdt=xdt, d=d)


# ---- lpi_row_jobs -----------------------------------------------------------------------------------------------------------------------------------------------------
def op_job_ln_bwd(arm, k=0, kind="FBB"):
    run, check = op_ln_bwd(arm, kind, 132, "both", 1, k=k, job=True)
    dy, lddy, x, ldx, g, mean, rstd, dx, lddx, cast, ldcast, acc = run.tail
    assert lddx == ldcast      # out and out2 share ld_c (include/lpi_hip.h)
    run.job = lambda: _lib.row_job(_lib.ROWOP_LN_BWD, B=ROWS, d=132, dt_a=run.dts[0], dt_b=run.dts[1], a=dy, ld_a=lddy, b=x, ld_b=ldx, gamma=g, mean_in=mean,
                                   rstd_in=rstd, out=dx, out2=cast, ld_c=lddx, flag=acc)
    return run, check


def op_job_ln_bwd_rows_h16(arm, k=0, ragged=True):
    run, check = op_ln_bwd(arm, "H16", 136, "cast", 1, mapped="ragged" if ragged else "uniform", k=k)
    dy, lddy, x, ldx, g, mean, rstd, dx, lddx, cast, ldcast, acc = run.tail
    rs = torch.tensor(ROW_START, dtype=torch.int32, device=DEV) if ragged else None
    run.job = lambda: _lib.row_job(_lib.ROWOP_LN_BWD_ROWS_H16, B=MB, L=ML, row_start=rs, row0=MROW0, P=MP, d=136, a=dy, ld_a=lddy, b=x, ld_b=ldx, gamma=g, mean_in=mean,
                                   rstd_in=rstd, out2=cast, ld_c=ldcast, flag=acc)
    return run, check


def op_job_prompt_add(arm, k=0, xdt=F16, d=132):
    """PROMPT_ADD and VIS_PROMPT_ROWS_BWD take no leading dimension (the stream is [B L, d]): here for the offset base pointers and the rows they must not touch."""
    mrows, srows = mapped_rows(True)
    x0 = (rnd(srows, d, seed=60 + k) * 2).to(TD[xdt])
    pr = rnd(MP, d, seed=61 + k)
    X = arm.mat("x", srows, d, d, TD[xdt], x0, in_out=True)
    arm.rows_only("x", mrows)
    PR, OM, OR = arm.vec("prompt", MP * d, pr.reshape(-1)), arm.vec("out_mean", srows), arm.vec("out_rstd", srows)
    S.must_write(arm.ops["out_mean"], index=[(arm.base if arm.strided else 0) + r for r in mrows])
    S.must_write(arm.ops["out_rstd"], index=[(arm.base if arm.strided else 0) + r for r in mrows])
    rs = torch.tensor(ROW_START, dtype=torch.int32, device=DEV)

    def run():
        call("lpi_prompt_add_varlen", xdt, MB, ML, rs, MP, d, X, PR, 0, OM, OR, stream())

    def check(t):      # test_fp16_residual_stream_kernels: the stored rows equal the rounded sum
        ref = (x0[mrows].float() + pr.repeat(MB, 1)).to(TD[xdt])
        assert same_bits(t.got("x")[mrows].contiguous().cpu(), ref)
    run.job = lambda: _lib.row_job(_lib.ROWOP_PROMPT_ADD, B=MB, L=ML, row_start=rs, P=MP, d=d, dt_a=xdt, out=X, a=PR, bstride=0, mean=OM, rstd=OR)
    return run, check


def op_job_vis_prompt_rows_bwd(arm, k=0, dt=BF16, d=132):
    mrows, srows = mapped_rows(False)
    G2 = ML - 1 - MP
    dx0, pr, gam = rnd(srows, d, seed=70 + k).to(TD[dt]), rnd(MP, d, seed=71 + k), 1 + 0.1 * rnd(d, seed=72 + k)
    m, r = stats64(pr.repeat(MB, 1))
    mean, rstd = torch.full((srows,), float("nan")), torch.full((srows,), float("nan"))
    mean[mrows], rstd[mrows] = m.float(), r.float()
    DX = arm.mat("dx0", srows, d, d, TD[dt], dx0, in_out=True)
    arm.rows_only("dx0", mrows)
    PR, G, MEAN, RSTD = arm.vec("prompt0", MP * d, pr.reshape(-1)), arm.vec("gamma", d, gam), arm.vec("mean", srows, mean), arm.vec("rstd", srows, rstd)
    DP = arm.mat("dprompt", MP, d, d, torch.float32)      # the single-op entry point's batch sum (its second launch); the job has the LayerNorm part alone

    def run():
        call("lpi_vis_assemble_bwd", dt, MB, G2, MP, d, DX, PR, 0, G, MEAN, RSTD, DP, stream())

    def check(t):      # LN' of the prompt rows: the gradient stream's bars (TOL)
        xr = pr.repeat(MB, 1).double().requires_grad_(True)
        torch.nn.functional.layer_norm(xr, (d,), gam.double(), None, 1e-5).backward(dx0[mrows].double())
        held("vis_prompt_rows_bwd", dt, t.got("dx0")[mrows], xr.grad, TOL[dt])
        # dprompt[p] = the f32 sum over the batch of the rows as stored: the f32 bar of tests/test_kernels_gpu.py
        held("vis_assemble_bwd dprompt", F32, t.got("dprompt"), t.got("dx0")[mrows].double().cpu().reshape(MB, MP, d).sum(0), TOL[F32])
    run.job = lambda: _lib.row_job(_lib.ROWOP_VIS_PROMPT_ROWS_BWD, B=MB, L=ML, P=MP, d=d, dt_a=dt, out=DX, a=PR, bstride=0, gamma=G, mean_in=MEAN, rstd_in=RSTD)
    return run, check


# op, keyword arguments, (max_rows, max_ld, base) at k <= 3, launches of the single-op form
JOBS = {
    "POOL_LN_FWD": (op_pool_ln_fwd, dict(xdt=F16, ydt=BF16, raw=True), (MB * ML, 132 + 16, 4), 2),
    "L2NORM_FWD": (op_l2norm_fwd, {}, (ROWS, 132 + 48, 4), 1),
    "L2NORM_BWD": (op_l2norm_bwd, dict(copy=True), (ROWS, 132 + 48, 4), 1),
    "POOL_LN_BWD": (op_pool_ln_bwd, {}, (MB * ML, 132 + 16, 4), 1),
    "LN_BWD": (op_job_ln_bwd, {}, (ROWS, 132 + 64, 4), 1),
    "SCATTER_ADD": (op_scatter_add, {}, (MB * ML, 132 + 32, 4), 1),
    "GATHER_BATCH_ROWS": (op_gather, dict(ragged=True), (MB * ML, 136 + 64, 8), 1),
    "PROMPT_ADD": (op_job_prompt_add, {}, (MB * ML, 132, 4), 1),
    "LN_BWD_ROWS_H16": (op_job_ln_bwd_rows_h16, {}, (MB * ML, 136 + 128, 8), 1),
    "VIS_PROMPT_ROWS_BWD": (op_job_vis_prompt_rows_bwd, {}, (MB * ML, 132, 4), 2),
}


def single_and_job(names, label):
    """Each op of `names` twice on STRIDED operands (op k with its own leading dimensions): the single-op entry points on one set, ONE lpi_row_jobs launch on the other."""
    sets = ([], [])
    for which in (0, 1):
        for k, name in enumerate(names):
            op, kw, size, _ = JOBS[name]
            arm = Arm(True, *size)
            run, _ = op(arm, k=k, **kw)
            sets[which].append((arm, run))
    torch.cuda.synchronize()
    n0 = _lib.launch_count()
    for arm, run in sets[0]:
        run()
    torch.cuda.synchronize()
    assert _lib.launch_count() - n0 == sum(JOBS[n][3] for n in names)
    jobs = [run.job() for _, run in sets[1]]
    lds = [(j.ld_a, j.ld_b, j.ld_c) for j in jobs]
    n0 = _lib.launch_count()
    _lib.row_jobs(jobs, stream())
    torch.cuda.synchronize()
    assert _lib.launch_count() - n0 == 1
    for (a0, _), (a1, _), name in zip(sets[0], sets[1], names):
        if name == "L2NORM_BWD":      # the bf16 copy exists in the job alone (the single-op form is lpi_cast behind it): written, inside its rows, = the cast of dx
            c = a1.ops.pop("dx16")
            S.check_pads("L2NORM_BWD dx16", c), S.check_written("L2NORM_BWD dx16", c)
            assert same_bits(c.t.contiguous(), a1.ops["dx"].t.to(torch.bfloat16).contiguous())
            a0.ops.pop("dx16")
        if name == "VIS_PROMPT_ROWS_BWD":      # dprompt is written by the single-op form alone (lpi_vis_assemble_bwd's batch sum): written, inside its rows
            c = a0.ops.pop("dprompt")
            S.check_pads("VIS_PROMPT_ROWS_BWD dprompt", c), S.check_written("VIS_PROMPT_ROWS_BWD dprompt", c)
            S.check_pads("VIS_PROMPT_ROWS_BWD dprompt (row-job arm: untouched)", a1.ops.pop("dprompt"))
        A.check_arms(f"{label} {name}", a0.ops, a1.ops, torch.cuda.synchronize, names=("single-op", "row-job"), kept=True)
    return lds


@pytest.mark.parametrize("name", list(JOBS))
def test_each_row_job_equals_its_single_op_entry_point_on_strided_operands(name):
    single_and_job([name], "row job")
    op, kw, size, launches = JOBS[name]
    kw = {k: v for k, v in kw.items() if k != "copy"}      # (the bf16 copy of L2NORM_BWD exists in the job alone)
    run_arms(f"single {name}", op, *size, launches=launches, **kw)      # ... and the single-op form against the tight arm and f64


def test_four_row_jobs_in_one_launch_each_with_its_own_leading_dimensions():
    lds = single_and_job(["SCATTER_ADD", "L2NORM_BWD", "LN_BWD", "LN_BWD_ROWS_H16"], "four jobs")
    used = [v for t in lds for v in t if v]
    assert len(used) == len(set(used)) == 11, lds      # every job's ld_a / ld_b / ld_c differs from every other job's (SCATTER_ADD has no ld_b)
    single_and_job(["POOL_LN_FWD", "L2NORM_FWD", "POOL_LN_BWD", "GATHER_BATCH_ROWS"], "four jobs")


# ---- what the checks refuse -------------------------------------------------------------------------------------------------------------------------------------------
def test_strides_and_pointers_the_row_kernels_cannot_take_are_refused_before_any_launch():
    """Library version 618: a row moved four elements at a time needs its pointer aligned to that access (16 bytes f32, 8 bytes 2-byte types) and a leading dimension
    that covers the width; gamma / beta and every other f32x4 vector 16 bytes; lpi_scatter_add_rows the same rule (f32 rows were held to 8 bytes).  Each refusal launches nothing; the unmodified argument lists launch."""
    lib = _lib.load()
    keep = []      # every tensor whose address goes into an argument list lives until the final synchronize: no list holds a freed block, no two operands share one

    def P(t):
        if t is None:
            return None
        keep.append(t)
        return t.data_ptr()
    z = lambda *s, td=torch.float32: torch.zeros(*s, device=DEV, dtype=td)  # noqa: E731
    d, R = 132, ROWS
    x, y, g, b, st = z(R, 160), z(R, 160), z(d + 4), z(d + 4), z(2, R)      # wide enough for every leading dimension below
    xh, yb = z(R, 160, td=torch.float16), z(R, 160, td=torch.bfloat16)
    idx = torch.zeros(R, dtype=torch.int32, device=DEV)
    s = stream()
    E = -22

    def variants(good, bad):
        """good: {name: value}; bad: [(name, value)] each replacing one argument -> the argument tuples"""
        return [tuple(dict(good, **{k: v}).values()) for k, v in bad]

    cases = []      # (function, good argument tuple, bad argument tuples, launches of the good one)
    fwd = dict(dt=F32, xdt=F32, rows=R, d=d, x=P(x), ldx=d + 8, g=P(g), b=P(b), y=P(y), ldy=d + 8, m=P(st[0]), r=P(st[1]), s=s)
    cases.append((lib.lpi_layernorm_fwd, fwd, [("x", P(x) + 4), ("y", P(y) + 8), ("g", P(g) + 4), ("b", P(b) + 8), ("ldx", d - 4), ("ldy", d - 4), ("ldy", d + 2)], 1))
    fwdh = dict(fwd, dt=BF16, xdt=F16, x=P(xh), y=P(yb))
    cases.append((lib.lpi_layernorm_fwd, fwdh, [("x", P(xh) + 4), ("y", P(yb) + 2), ("y", P(yb) + 4), ("ldy", d - 4)], 1))
    st136 = dict(fwdh, d=136, ldx=144, g=None, b=None, y=None, ldy=0)
    cases.append((lib.lpi_layernorm_fwd, st136, [("ldx", 128), ("x", P(xh) + 8)], 1))
    bwd = dict(dy=F32, c=F32, xdt=F32, rows=R, d=d, pdy=P(y), lddy=d + 8, x=P(x), ldx=d + 8, g=P(g), m=P(st[0]), r=P(st[1]), dx=P(z(R, d + 8)), lddx=d + 8,
               cast=P(z(R, d + 8)), ldcast=d + 8, acc=0, s=s)
    cases.append((lib.lpi_layernorm_bwd, bwd, [("pdy", P(y) + 4), ("x", P(x) + 8), ("g", P(g) + 4), ("dx", bwd["dx"] + 4), ("cast", bwd["cast"] + 8), ("lddy", d - 4),
                                               ("ldx", d - 4), ("lddx", d - 4), ("ldcast", d - 4)], 1))
    rows = dict(dy=F32, c=F32, xdt=F32, B=MB, L=ML, row0=1, P=MP, d=d, pdy=P(y), lddy=d + 8, x=P(z(MB * ML, d + 8)), ldx=d + 8, g=P(g), m=P(z(MB * ML)), r=P(z(MB * ML)),
                dx=P(z(MB * ML, d + 8)), lddx=d + 8, cast=None, ldcast=d + 8, acc=0, s=s)
    cases.append((lib.lpi_layernorm_bwd_rows, rows, [("lddx", d - 4), ("g", P(g) + 8), ("pdy", P(y) + 4)], 1))
    rs3 = torch.tensor(ROW_START, dtype=torch.int32, device=DEV)
    rowsv = dict(dy=BF16, c=BF16, xdt=F32, B=MB, L=ML, rs=P(rs3), row0=1, P=MP, d=d, pdy=P(yb), lddy=d + 8, x=P(z(MB * ML, d + 8)), ldx=d + 8, g=P(g), m=P(z(MB * ML)),
                 r=P(z(MB * ML)), dx=None, lddx=d + 8, cast=P(z(MB * ML, d + 8, td=torch.bfloat16)), ldcast=d + 8, acc=0, s=s)
    cases.append((lib.lpi_layernorm_bwd_rows_varlen, rowsv, [("ldcast", d - 4), ("cast", rowsv["cast"] + 4), ("pdy", P(yb) + 4), ("x", rowsv["x"] + 8), ("g", P(g) + 4),
                                                             ("ldx", d - 4)], 1))
    padd = dict(xdt=F16, B=2, L=6, P=2, d=d, x=P(z(12, d, td=torch.float16)), pr=P(z(2, d + 4)), pbs=0, om=None, orr=None, s=s)
    cases.append((lib.lpi_prompt_add, padd, [("x", padd["x"] + 4), ("pr", padd["pr"] + 4)], 1))
    rs2 = torch.tensor([0, 5, 11], dtype=torch.int32, device=DEV)
    paddv = dict(xdt=F32, B=2, L=6, rs=P(rs2), P=2, d=d, x=P(z(12, d)), pr=P(z(2, d + 4)), pbs=0, om=None, orr=None, s=s)
    cases.append((lib.lpi_prompt_add_varlen, paddv, [("x", paddv["x"] + 8), ("pr", paddv["pr"] + 8)], 1))
    vab = dict(dt=BF16, B=2, G2=3, P=2, d=d, dx0=P(z(12, d, td=torch.bfloat16)), pr=P(z(2, d + 4)), pbs=0, g=P(g), m=P(z(12)), r=P(z(12)), dp=P(z(2, d + 4)), s=s)
    cases.append((lib.lpi_vis_assemble_bwd, vab, [("dx0", vab["dx0"] + 4), ("pr", vab["pr"] + 4), ("g", P(g) + 8), ("dp", vab["dp"] + 4)], 2))      # LN' + the batch sum
    l2f = dict(B=R, E=d, x=P(x), ldx=d + 8, y=P(y), ldy=d + 8, inv=P(st[0]), s=s)
    cases.append((lib.lpi_l2norm_fwd, l2f, [("x", P(x) + 4), ("y", P(y) + 8), ("ldx", d - 4), ("ldy", d - 4)], 1))
    l2b = dict(B=R, E=d, y=P(y), ldy=d + 8, dy=P(x), lddy=d + 8, inv=P(st[0]), dx=P(z(R, d + 8)), lddx=d + 8, s=s)
    cases.append((lib.lpi_l2norm_bwd, l2b, [("y", P(y) + 4), ("dy", P(x) + 4), ("dx", l2b["dx"] + 8), ("lddx", d - 4), ("lddy", d - 4), ("ldy", d - 4)], 1))
    plf = dict(dt=BF16, xdt=F16, B=R, L=1, d=d, x=P(xh), idx=None, g=P(g), b=P(b), y=P(yb), ldy=d + 8, m=P(st[0]), r=P(st[1]), s=s)
    cases.append((lib.lpi_pool_ln_fwd, plf, [("x", P(xh) + 4), ("y", P(yb) + 4), ("g", P(g) + 4), ("b", P(b) + 4), ("ldy", d - 4)], 1))
    plb = dict(c=BF16, B=R, L=1, d=d, dy=P(y), lddy=d + 8, x=P(x), idx=None, g=P(g), m=P(st[0]), r=P(st[1]), dx=P(z(R, d + 8)), cast=P(yb), s=s)
    cases.append((lib.lpi_pool_ln_bwd, plb, [("dy", P(y) + 4), ("x", P(x) + 4), ("g", P(g) + 8), ("dx", plb["dx"] + 4), ("cast", P(yb) + 4), ("lddy", d - 4)], 1))
    sca = dict(dt=F32, B=R, L=1, d=d, src=P(x), lds=d + 8, idx=None, dst=P(y), ldd=d + 8, s=s)      # f32 rows are moved 16 bytes at a time: up to 617 held to 8 only
    cases.append((lib.lpi_scatter_add_rows, sca, [("ldd", d + 2), ("lds", d + 6), ("src", P(x) + 8), ("dst", P(y) + 8), ("ldd", d - 4)], 1))
    img, cols = z(2, 3, 8, 8), z(8, 72, td=torch.bfloat16)
    pat = dict(dt=BF16, B=2, R=8, ps=4, img=P(img), cols=P(cols), ld=68, s=s)
    cases.append((lib.lpi_patchify, pat, [("cols", P(cols) + 4), ("cols", P(cols) + 2), ("ld", 60), ("ld", 66)], 1))
    patu = dict(dt=F32, B=2, R=8, ps=4, img=P(torch.zeros(2, 3, 8, 8, dtype=torch.uint8, device=DEV)), lut=P(z(768)), cols=P(z(8, 72)), ld=68, s=s)
    cases.append((lib.lpi_patchify_u8, patu, [("cols", patu["cols"] + 8), ("ld", 60)], 1))
    pe, pos, pr, x0, cls = z(8, d + 8), z(5, d), z(2, d + 4), z(14, d + 4), z(d + 4)
    vis = dict(xdt=F32, B=2, G2=4, P=2, d=d, pe=P(pe), ldpe=d + 8, cls=P(cls), pos=P(pos), pr=P(pr), pbs=0, g=P(g), b=P(b), x0=P(x0), m=P(z(14)), r=P(z(14)), om=None, orr=None, s=s)
    cases.append((lib.lpi_vis_assemble_fwd, vis, [("pe", P(pe) + 4), ("ldpe", d - 4), ("cls", P(cls) + 4), ("pos", P(pos) + 8), ("pr", P(pr) + 4), ("g", P(g) + 4), ("b", P(b) + 4),
                                                   ("x0", P(x0) + 4)], 1))
    n0 = _lib.launch_count()
    for fn, good, bads, _ in cases:
        for a in variants(good, bads):
            assert fn(*a) == E, (fn.__name__, a)
    # the pair: BOTH problems are checked before the first launch (off the fused path a pair is two launches)
    ok = (R, d, x, d + 8, g, b, y, d + 8, st[0], st[1])
    for bad in ((R, d, x, d + 8, g[1:], b, y, d + 8, st[0], st[1]), (R, d, x, d + 8, g, b, y, d - 4, st[0], st[1])):
        with pytest.raises(_lib.LpiError):
            _lib.layernorm_fwd_pair(F32, F32, ok, bad, s)
    okb = (R, d, y, d + 8, x, d + 8, g, st[0], st[1], z(R, d + 8), d + 8, None, d + 8, 0)
    with pytest.raises(_lib.LpiError):
        _lib.layernorm_bwd_pair(F32, F32, F32, okb, okb[:10] + (d - 4,) + okb[11:], s)
    # row jobs: the same rules per op
    inv = st[0]
    good_jobs = dict(
        l2f=dict(op=_lib.ROWOP_L2NORM_FWD, B=R, d=d, a=x, ld_a=d + 8, out=y, ld_c=d + 8, mean=inv),
        l2b=dict(op=_lib.ROWOP_L2NORM_BWD, B=R, d=d, a=y, ld_a=d + 8, b=x, ld_b=d + 8, mean_in=inv, out=z(R, d + 8), ld_c=d + 8, out2=yb, dt_b=BF16),
        plf=dict(op=_lib.ROWOP_POOL_LN_FWD, B=R, L=1, d=d, dt_a=F16, dt_b=BF16, a=xh, gamma=g, beta=b, out=yb, ld_c=d + 8, mean=st[0], rstd=st[1], out2=z(R, d)),
        plb=dict(op=_lib.ROWOP_POOL_LN_BWD, B=R, L=1, d=d, dt_b=BF16, a=y, ld_a=d + 8, b=x, gamma=g, mean_in=st[0], rstd_in=st[1], out=z(R, d), out2=yb),
        lnb=dict(op=_lib.ROWOP_LN_BWD, B=R, d=d, dt_a=F32, dt_b=F32, a=y, ld_a=d + 8, b=x, ld_b=d + 8, gamma=g, mean_in=st[0], rstd_in=st[1], out=z(R, d + 8), out2=z(R, d + 8),
                 ld_c=d + 8, flag=0),
        sadd=dict(op=_lib.ROWOP_SCATTER_ADD, B=R, L=1, d=d, dt_a=F32, a=x, ld_a=d + 8, out=y, ld_c=d + 8),
        padd=dict(op=_lib.ROWOP_PROMPT_ADD, B=2, L=6, P=2, d=d, dt_a=F16, out=z(12, d, td=torch.float16), a=z(2, d + 4), bstride=0),
        vpr=dict(op=_lib.ROWOP_VIS_PROMPT_ROWS_BWD, B=2, L=6, P=2, d=d, dt_a=BF16, out=z(12, d, td=torch.bfloat16), a=z(2, d + 4), bstride=0, gamma=g, mean_in=z(12),
                 rstd_in=z(12)),
        h16=dict(op=_lib.ROWOP_LN_BWD_ROWS_H16, B=2, L=6, row0=1, P=2, d=136, a=z(4, 144, td=torch.bfloat16), ld_a=144, b=z(12, 144, td=torch.float16), ld_b=144, gamma=g,
                 mean_in=z(12), rstd_in=z(12), out2=z(12, 144, td=torch.bfloat16), ld_c=144, flag=0))
    off = lambda t, n: t.reshape(-1)[n:]  # noqa: E731
    bad_jobs = [("l2f", "a", off(x, 1)), ("l2f", "ld_c", d - 4), ("l2b", "out2", off(yb, 2)), ("l2b", "ld_b", d - 4), ("plf", "gamma", off(g, 1)), ("plf", "out", off(yb, 2)),
                ("plf", "ld_c", d - 4), ("plf", "out2", off(z(R, d + 4), 1)), ("plb", "b", off(x, 1)), ("plb", "gamma", off(g, 2)), ("plb", "ld_a", d - 4),
                ("lnb", "gamma", off(g, 1)), ("lnb", "ld_c", d - 4), ("lnb", "a", off(y, 1)), ("sadd", "ld_c", d + 2), ("sadd", "a", off(x, 2)), ("padd", "out", off(z(13, d, td=torch.float16), 2)),
                ("padd", "a", off(z(2, d + 4), 1)), ("vpr", "gamma", off(g, 1)), ("vpr", "a", off(z(2, d + 4), 2)), ("h16", "gamma", off(g, 1)), ("h16", "ld_c", 128),
                ("h16", "ld_a", 128)]
    for name, field, value in bad_jobs:
        kw = dict(good_jobs[name], **{field: value})
        with pytest.raises(_lib.LpiError):
            _lib.row_jobs([_lib.row_job(kw.pop("op"), **kw)], s)
    torch.cuda.synchronize()
    assert _lib.launch_count() == n0, "a refused call launched a kernel"
    # every argument list the refusals started from launches
    for fn, good, _, launches in cases:
        n1 = _lib.launch_count()
        assert fn(*good.values()) == 0, fn.__name__
        assert _lib.launch_count() - n1 == launches, fn.__name__
    n1 = _lib.launch_count()
    ok2 = ok[:6] + (z(R, 160),) + ok[7:8] + (z(R), z(R))      # the second problem writes buffers of its own
    okb2 = okb[:9] + (z(R, d + 8),) + okb[10:]
    _lib.layernorm_fwd_pair(F32, F32, ok, ok2, s)
    _lib.layernorm_bwd_pair(F32, F32, F32, okb, okb2, s)
    assert _lib.launch_count() - n1 == 4
    for name, kw in good_jobs.items():
        n1 = _lib.launch_count()
        kw = dict(kw)
        _lib.row_jobs([_lib.row_job(kw.pop("op"), **kw)], s)
        assert _lib.launch_count() - n1 == 1, name
    torch.cuda.synchronize()
    del keep      # ... only now

