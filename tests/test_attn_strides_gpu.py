"""The attention family held to its leading dimensions and its write bounds on a real MI355X: lpi_attn_fwd / _bwd and their _varlen / _prefix / _shared / _layout /
_one / _pair forms (attention.hip, attention4.hip, attn_long.hip), lpi_shared_kv_reduce, lpi_attn_pooled_* (attn_pooled.hip) and lpi_spool_attn_* (attn_stream.hip).

Every case runs its call sequence twice under the same tuning keys: the STRIDED arm on tests/strided.py views (every base pointer offset by 16 bytes or more, ldqkv,
lddqkv, ldctx, lddctx, ldq, lddq all different from each other and from the widths, NaN in every pad, lse / delta arenas whose footprint is exactly [B, H, L]), the
TIGHT arm on contiguous copies of the same values.  H = 2 throughout: the head step (64), the q | k | v step (H 64 = 128) and the row strides are different numbers.
Asserted in each case (tests/attn_arms.py; tests/test_attn_strides_host.py proves that these assertions catch a wrong stride):
  * each call launches as many kernels as the dispatch in the code implies (forward 1; f32 / key-3 two-pass backward 2; fused backward 1; streamed single-pass
    backward 1, or 2 at 224 < L <= 288; long backward 2; shared backward + 1 reduce; spool forward and backward 3 each), the same number in both arms;
  * every output of the strided arm equals the tight arm's bit for bit: ctx, lse, dq / dk / dv, dq of the pooled forms, dh;
  * no pad of any operand, inputs included, changed; every must-be-written output element was written.  Rows behind `rows_needed` may be left unwritten: they
    are neither must-be-written nor pads.  Rows >= row_start[B] up to the 256-rounded row count are pads.  delta's contents are unspecified: pads only;
  * the tight arm holds no NaN and meets the f64 CPU reference at the bar of the kernel's existing test (BARS below names each source).
Every arena of a case has attn_arms.case_bytes() bytes — the 256-rounded largest row count x the largest leading dimension x 4 bytes + the largest base offset —
so a kernel that applies any stride of the case to any pointer of the case fails an assertion and never leaves an allocation.

Leading dimensions: "tier1" = ldqkv 3d + 32, lddqkv 3d + 64, ldctx d + 8, lddctx d + 16, ldq d + 24, lddq d + 40 (spool: ldx d + 8, ldw d + 16, ldwt 3d + 24,
lddh d + 32, and d + 48 / d + 56 for its ctx / dctx so that they stay different from ldx / ldw); "min" = the smallest steps the argument checks of every entry
point of the case accept (include/lpi_hip.h, "Alignment of the attention operands"); "wide" = each matrix is the right two thirds of a [rows, 1.5 x width] buffer
(the engine's column blocks; there the leading dimensions of equally wide matrices coincide).  What the checks refuse is tested to launch nothing.
"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_arms as AA  # noqa: E402
import strided as S  # noqa: E402
from lpi_amd import _lib  # noqa: E402
from lpi_amd._lib import BF16, F16, F32, LpiError, call  # noqa: E402
from poison import relerr  # noqa: E402

DEV = "cuda:0"
TD = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
GD = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.bfloat16}      # gradients of the f16 mode are bf16 (test_attention_f16_forward_bf16_backward)
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
ALL, TWO = [F32, BF16, F16], [BF16, F16]
H, HD = 2, 64
D = H * HD
PRE = 17                       # shared prefix rows (tests/test_shared_prefix_gpu.py)
RAGGED = [59, 17, 32, 5]       # tests/test_dead_memory_gpu.py
DEFAULT_KEYS = {3: 0, 7: 0, 9: 0, 11: 0, 12: 0, 13: 0}
# The bars of the kernels' existing tests (relerr = max |got - ref| / max |ref|):
#   ctx / lse / gradients of the full attention: tests/test_kernels_gpu.py test_attention_fwd_bwd (f32, bf16), test_attention_f16_forward_bf16_backward (f16),
#   test_attention_varlen_fwd_bwd (ragged), test_attention_long_sequences_fwd_bwd (L > 288: bf16's bars for f16 too), as collected in tests/test_dead_memory_gpu.py;
#   pooled forms: test_attention_pooled_row_fwd_bwd, test_layernorm_f16_output_and_pooled_attention_f16;
#   spool: tests/test_round6_gpu.py test_last_block_attention_from_the_stream_against_f64 (ctx 1e-2, dq and dh 1.5e-2, inclusive).
CTX_BAR = {F32: 2e-5, BF16: 2e-2, F16: 3e-3}
LSE_BAR = {F32: 1e-5, BF16: 2e-2, F16: 3e-3}
GRAD_BAR = {F32: 5e-5, BF16: 4e-2, F16: 4e-2}
SPOOL_BAR = dict(ctx=1e-2, dq=1.5e-2, dh=1.5e-2)


def bars(dt, L):
    long_ = L > 288
    return (CTX_BAR[BF16] if long_ and dt == F16 else CTX_BAR[dt]), (LSE_BAR[BF16] if long_ and dt == F16 else LSE_BAR[dt]), GRAD_BAR[dt]


def stream():
    return torch.cuda.current_stream().cuda_stream


def esz(td):
    return 4 if td == torch.float32 else 2


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


class tuning:
    """Tuning keys set inside the block, every one of them restored after it (also when the block raises)."""

    def __init__(self, keys):
        self.keys = dict(keys)

    def __enter__(self):
        lib = _lib.load()
        self.old = {k: lib.lpi_get_tuning(k) for k in self.keys}
        for k, v in self.keys.items():
            assert lib.lpi_set_tuning(k, v) == 0

    def __exit__(self, *exc):
        for k, v in self.old.items():
            assert _lib.load().lpi_set_tuning(k, v) == 0


# ---- leading dimensions ---------------------------------------------------------------------------------------------------------------------------------------------
WIDTH = dict(ldqkv=3 * D, lddqkv=3 * D, ldctx=D, lddctx=D, ldq=D, lddq=D, ldqkv_t=3 * D, ldctx_t=D, ldx=D, ldw=D, ldwt=3 * D, lddh=D, lddqkv_any=3 * D)


def make_lds(ldset, group, dt):
    """-> {key: leading dimension in elements, "wide": bool}.  group: "full" (attention.hip / attention4.hip / attn_long.hip and the layout forms), "pooled", "spool"."""
    keys = dict(full=("ldqkv", "lddqkv", "ldctx", "lddctx", "ldqkv_t", "ldctx_t"), pooled=("ldqkv", "lddqkv", "ldctx", "lddctx", "ldq", "lddq"),
                spool=("ldx", "ldw", "ldwt", "lddh", "ldq", "lddq", "ldctx", "lddctx"))[group]
    if ldset == "wide":
        return dict({k: 3 * WIDTH[k] // 2 for k in keys}, wide=True, nudge=False)
    if ldset == "tier1":
        add = dict(ldqkv=32, lddqkv=64, ldctx=8, lddctx=16, ldq=24, lddq=40, ldqkv_t=96, ldctx_t=48, ldx=8, ldw=16, ldwt=24, lddh=32)
        if group == "spool":
            add.update(ldctx=48, lddctx=56)
        add = {k: add[k] for k in keys}
    else:
        assert ldset == "min"
        u, g = 16 // esz(TD[dt]), 16 // esz(GD[dt])
        if group == "full":
            # ldqkv / lddqkv / lddctx: whole 16-byte units (bad_attn, lpi_attn_bwd_prefix); ldctx: the forward wants 8 ELEMENTS for every type, the backward 16 bytes:
            # ctx is shared, so the stricter rule; the layout forms want 8 elements everywhere (2-byte types: the same numbers)
            add = dict(ldqkv=u, lddqkv=2 * g, ldctx=8, lddctx=g if g != 8 else 16, ldqkv_t=3 * u, ldctx_t=24)
        elif group == "pooled":
            # q, qkv, dctx are read four elements at a time and held to 16 bytes; ctx, dq and dqkv are stored one element at a time: any step (dqkv on a shared
            # prefix goes through lpi_shared_kv_reduce as well: 4 elements; elsewhere lddqkv_any, an odd step)
            add = dict(ldqkv=u, ldq=u, lddctx=2 * g, ldctx=1, lddq=3, lddqkv=4 if u != 4 else 8, lddqkv_any=5)
            keys = keys + ("lddqkv_any",)
        else:
            # x, Wqkv, WqkvT, q, dctx: 8 elements; dh: 4 elements (8-byte stores); ctx and dq are stored one element at a time
            add = dict(ldx=8, ldw=16, ldwt=8, ldq=24, lddctx=32, ldctx=1, lddq=3, lddh=4)
    assert set(add) == set(keys), (ldset, group)
    L = {k: WIDTH[k] + v for k, v in add.items()}
    per_width = {}
    for k, v in L.items():
        assert v != WIDTH[k] and v not in per_width.setdefault(WIDTH[k], set()), (ldset, group, k)      # pairwise different among equally wide matrices, and != width
        per_width[WIDTH[k]].add(v)
    assert len(set(L.values())) == len(L), L
    return dict(L, wide=False, nudge=ldset == "min")


class Arm:
    """The operands of one arm of a case as strided.Records: .ops[name]; .p[name] the pointer handed to the kernel, .ld[name] its leading dimension."""

    def __init__(self, L, nbytes):
        self.L, self.nbytes, self.ops, self.p, self.ld = L, nbytes, {}, {}, {}

    def mat(self, name, rows, key, td, fill=None, col=0, cols=None, bump=0, any_pointer=False):
        """A [rows, cols] block at column `col` of a matrix of WIDTH[key] columns (the pooled backward's dqkv: col = d, cols = 2d); the pointer is the matrix's.
        any_pointer: an operand that is stored one element at a time — in the "min" set its pointer sits ONE ELEMENT behind the 16-byte offset."""
        width = WIDTH[key]
        cols = width - col if cols is None else cols
        if self.L is None:
            ld, base = width, 0
        else:
            ld, base = self.L[key] + bump, (width // 2 if self.L["wide"] else 16 // esz(td)) + (1 if any_pointer and self.L["nudge"] else 0)
        rec = S.operand(rows, cols, ld, td, base + col, self.nbytes // esz(td), fill, DEV)
        self.ops[name], self.p[name], self.ld[name] = rec, rec.arena[base:], ld
        return rec

    def stat(self, name, n, fill=None, live=None, unspecified=False):
        """n floats (lse, delta, scratch, LayerNorm statistics) 16 bytes into an arena of the case's size; live: bool [n], what must be written."""
        base = 0 if self.L is None else 4
        rec = S.region(base + torch.arange(n), torch.float32, self.nbytes // 4, fill, DEV)
        if unspecified:
            S.must_write(rec, none=True)
        elif live is not None:
            S.must_write(rec, index=base + live.reshape(-1).nonzero()[:, 0])
        self.ops[name], self.p[name] = rec, rec.arena[base:]
        return rec

    def vals(self, name, shape=None):
        """The footprint's values of operand `name` on the CPU (row by row)."""
        o = self.ops[name]
        v = o.arena[o.inside].cpu()
        return v if shape is None else v.reshape(shape)


def case_bytes(rows, L):
    lds = [v for k, v in L.items() if k not in ("wide", "nudge")]
    return AA.case_bytes(rows, lds + [max(lds) + 64], [3 * D // 2 + D if L["wide"] else 9 + D])      # (+ 64: the pair's second problem; + D: a column-block footprint)


def launches(fn, want, label):
    n0 = _lib.launch_count()
    fn()
    got = _lib.launch_count() - n0
    assert got == want, f"{label}: {got} launches, the dispatch implies {want}"


def bwd_launches(dt, L, causal, ragged, keys):
    """lpi_attn_bwd_prefix's dispatch (attention.hip): long | f32 and key 3: two passes | streamed (attention4.hip; two key windows behind 224) | fused."""
    if L > 288:
        return 2
    if dt == F32 or keys.get(3, 0):
        return 2
    if not ragged and not causal and (keys.get(7, 0) == 5 or (keys.get(7, 0) == 0 and L > 160)):
        return 2 if L > 224 else 1
    Lp = (L + 31) // 32 * 32
    return 1 if 4 * Lp * 160 + 8 * Lp <= 160 * 1024 else 2      # bwd_launch: the fused kernel keeps four images of Lp rows in LDS


def held(label, name, got, ref, bar, inclusive=False):
    e = relerr(got, ref)
    print(f"{label} {name}: error {e:.3e} (bar {bar:g})")
    assert (e <= bar) if inclusive else (e < bar), (label, name, e, bar)
    return e


# ---- f64 references -------------------------------------------------------------------------------------------------------------------------------------------------
def seq_attention(x, rows, q_from, causal):
    """One sequence in f64: keys = the global rows `rows` (in position order) of x [R, 3d] (q | k | v, heads by 64), queries = positions q_from .. -> ctx [nq, d],
    lse [H, nq] (tests/test_kernels_gpu.py: attn_ref, per sequence)."""
    rows = torch.as_tensor(rows)
    n, nq = len(rows), len(rows) - q_from
    q = x[rows[q_from:], :D].reshape(nq, H, HD).transpose(0, 1)
    k, v = (x[rows, c * D:(c + 1) * D].reshape(n, H, HD).transpose(0, 1) for c in (1, 2))
    s = (q * 0.125) @ k.transpose(-1, -2)
    if causal:
        s = s + torch.full((nq, n), float("-inf"), dtype=torch.float64).triu_(1 + q_from)
    return (torch.softmax(s, -1) @ v).transpose(0, 1).reshape(nq, D), torch.logsumexp(s, -1)


def sequences(kind, B, L):
    """-> (the samples of a batch as (global rows, first query position), the row count, row_start or None, the longest sequence)."""
    if kind == "uniform":
        return [(list(range(b * L, (b + 1) * L)), 0) for b in range(B)], B * L, None, L
    lens = RAGGED if kind == "ragged" else [1, 7, 33, 60, 20]      # shared: the smallest two-head case of tests/test_shared_prefix_gpu.py
    pre = PRE if kind == "shared" else 0
    rs = [pre]
    for n in lens:
        rs.append(rs[-1] + n)
    own = [list(range(rs[b], rs[b + 1])) for b in range(len(lens))]
    if kind == "ragged":
        return [(r, 0) for r in own], rs[-1], rs, max(lens)
    return [(list(range(PRE)) + r, PRE) for r in own] + [(list(range(PRE)), 0)], rs[-1], rs, PRE + max(lens)      # sample index B = the shared sequence


@functools.lru_cache(maxsize=16)
def problem(dt, kind, B, L, causal):
    """Operands as stored and the f64 forward + backward of those: computed once per (type, batch), shared by the cases, never written."""
    seqs, M, rs, Lmax = sequences(kind, B, L)
    qkv = rnd(M, 3 * D, seed=11 + L, scale=0.7).to(TD[dt])
    dctx = rnd(M, D, seed=12 + L).to(GD[dt])
    x = qkv.double().requires_grad_(True)
    ctx, lse, live = torch.zeros(M, D, dtype=torch.float64), torch.zeros(len(seqs), H, Lmax, dtype=torch.float64), torch.zeros(len(seqs), H, Lmax, dtype=torch.bool)
    loss = 0.0
    for i, (rows, q_from) in enumerate(seqs):
        o, l_ = seq_attention(x, rows, q_from, causal)
        own = torch.as_tensor(rows[q_from:])
        ctx[own], lse[i, :, :len(own)], live[i, :, :len(own)] = o.detach(), l_.detach(), True
        loss = loss + (o * dctx[own].double()).sum()
    loss.backward()
    return dict(qkv=qkv, dctx=dctx, ctx=ctx, lse=lse, live=live, grad=x.grad, M=M, rs=rs, Lmax=Lmax, seqs=seqs, nb=len(seqs) - (kind == "shared"))


# ---- full attention: uniform, ragged, shared-prefix batches ---------------------------------------------------------------------------------------------------------
def full_arm(dt, kind, pb, causal, L, nbytes, keys, need, label):
    M, Lmax, B = pb["M"], pb["Lmax"], pb["nb"]
    a = Arm(L, nbytes)
    a.mat("qkv", M, "ldqkv", TD[dt], pb["qkv"]), a.mat("dctx", M, "lddctx", GD[dt], pb["dctx"]), a.mat("ctx", M, "ldctx", TD[dt]), a.mat("dqkv", M, "lddqkv", GD[dt])
    ns = pb["lse"].shape[0]
    a.stat("lse", ns * H * Lmax, live=pb["live"]), a.stat("delta", ns * H * Lmax, unspecified=True)
    rs = None if pb["rs"] is None else torch.tensor(pb["rs"], dtype=torch.int32, device=DEV)
    p, ld, st = a.p, a.ld, stream()
    nbwd = bwd_launches(dt, Lmax, causal, rs is not None, keys)
    if kind == "shared":
        a.stat("shared_dkv", B * PRE * 2 * D)
        launches(lambda: call("lpi_attn_fwd_shared", dt, B, Lmax, rs, PRE, H, p["qkv"], ld["qkv"], p["ctx"], ld["ctx"], p["lse"], st), 1, label + " forward")
        launches(lambda: call("lpi_attn_bwd_shared", dt, B, Lmax, rs, PRE, Lmax, H, p["qkv"], ld["qkv"], p["ctx"], ld["ctx"], p["dctx"], ld["dctx"], p["lse"], p["delta"],
                              p["dqkv"], ld["dqkv"], p["shared_dkv"], st), nbwd + 1, label + " backward + reduce")
    else:
        launches(lambda: call("lpi_attn_fwd_varlen", dt, B, Lmax, rs, H, p["qkv"], ld["qkv"], p["ctx"], ld["ctx"], p["lse"], causal, st) if rs is not None else
                 call("lpi_attn_fwd", dt, B, Lmax, H, p["qkv"], ld["qkv"], p["ctx"], ld["ctx"], p["lse"], causal, st), 1, label + " forward")
        launches(lambda: call("lpi_attn_bwd_varlen", dt, B, Lmax, rs, H, p["qkv"], ld["qkv"], p["ctx"], ld["ctx"], p["dctx"], ld["dctx"], p["lse"], p["delta"], p["dqkv"],
                              ld["dqkv"], causal, st) if rs is not None else
                 call("lpi_attn_bwd", dt, B, Lmax, H, p["qkv"], ld["qkv"], p["ctx"], ld["ctx"], p["dctx"], ld["dctx"], p["lse"], p["delta"], p["dqkv"], ld["dqkv"], causal, st),
                 nbwd, label + " backward")
    if need:      # the prefix form into a second gradient matrix: the first `need` positions of every sequence must be written, the rest may be
        part = a.mat("part", M, "lddqkv", GD[dt])
        S.must_write(part, prefix_rows(pb, need))
        a.stat("delta_p", ns * H * Lmax, unspecified=True)
        if kind == "shared":
            a.stat("shared_dkv_p", B * PRE * 2 * D)
            launches(lambda: call("lpi_attn_bwd_shared", dt, B, Lmax, rs, PRE, need, H, p["qkv"], ld["qkv"], p["ctx"], ld["ctx"], p["dctx"], ld["dctx"], p["lse"],
                                  p["delta_p"], p["part"], ld["part"], p["shared_dkv_p"], st), nbwd + 1, label + " backward, rows_needed")
        else:
            launches(lambda: call("lpi_attn_bwd_prefix", dt, B, Lmax, rs, need, H, p["qkv"], ld["qkv"], p["ctx"], ld["ctx"], p["dctx"], ld["dctx"], p["lse"], p["delta_p"],
                                  p["part"], ld["part"], causal, st), nbwd, label + " backward, rows_needed")
    return a


def prefix_rows(pb, need):
    """The global rows at positions < need of every sequence."""
    rows = set()
    for seq, q_from in pb["seqs"]:
        rows.update(seq[:need])
    return sorted(rows)


def full_case(dt, kind, B, L, causal, ldset, keys=None, need=0):
    keys = keys or {}
    pb = problem(dt, kind, B, L, causal)
    label = f"{kind} {NAME[dt]} B={B} L={pb['Lmax']} causal={causal} {ldset} keys={keys}"
    Ls = make_lds(ldset, "full", dt)
    nbytes = case_bytes(pb["M"], Ls)
    with tuning({**DEFAULT_KEYS, **keys}):
        st = full_arm(dt, kind, pb, causal, Ls, nbytes, keys, need, label)
        ti = full_arm(dt, kind, pb, causal, None, nbytes, keys, need, label)
    AA.check_arms(label, st.ops, ti.ops, torch.cuda.synchronize)
    cbar, lbar, gbar = bars(dt, pb["Lmax"])
    M = pb["M"]
    held(label, "ctx", ti.vals("ctx", (M, D)), pb["ctx"], cbar)
    held(label, "lse", ti.vals("lse", pb["lse"].shape)[pb["live"]], pb["lse"][pb["live"]], lbar)
    g = ti.vals("dqkv", (M, 3 * D))
    for i, name in enumerate(("dq", "dk", "dv")):
        held(label, name, g[:, i * D:(i + 1) * D], pb["grad"][:, i * D:(i + 1) * D], gbar)
    if need:
        rows = prefix_rows(pb, need)
        held(label, "rows_needed dqkv", ti.vals("part", (M, 3 * D))[rows], pb["grad"][rows], gbar)


UNIFORM = [(ALL, 2, 21, 0, {}), (ALL, 2, 77, 1, {}),                                  # one-head forward; f32 two-pass, 2-byte fused backward
           (TWO, 2, 77, 1, {3: 1}),                                                   # the two-pass kernels on 2-byte operands
           (ALL, 2, 213, 0, {}),                                                      # 2-byte: streamed single-pass backward (L > 160)
           ([BF16], 2, 213, 0, {7: 1}),                                               # the fused backward at L = 213
           (TWO, 2, 224, 0, {11: 1}), (TWO, 2, 273, 0, {11: 1}),                      # Lp = 224 instantiation | swizzled forward + two key windows; heads share a workgroup
           ([BF16], 1, 273, 0, {13: 1}),                                              # the padded (unswizzled) forward at 273
           (ALL, 1, 289, 0, {})]                                                      # attn_long.hip, the smallest long shape
UNIFORM_PARAMS = [pytest.param(dt, B, L, c, keys, "tier1", id=f"{NAME[dt]}-{B}x{L}-c{c}-{'-'.join(f'k{k}={v}' for k, v in keys.items()) or 'default'}-tier1")
                  for dts, B, L, c, keys in UNIFORM for dt in dts]
# min and wide once per kernel file: attention.hip (77, causal: all types), attention4.hip (213: 2-byte), attn_long.hip (289)
UNIFORM_PARAMS += [pytest.param(dt, B, L, c, {}, ldset, id=f"{NAME[dt]}-{B}x{L}-c{c}-default-{ldset}")
                   for ldset in ("min", "wide") for dts, B, L, c in ((ALL, 2, 77, 1), (TWO, 2, 213, 0), (ALL, 1, 289, 0)) for dt in dts]


@pytest.mark.parametrize("dt,B,L,causal,keys,ldset", UNIFORM_PARAMS)
def test_attention_uniform(dt, B, L, causal, keys, ldset):
    full_case(dt, "uniform", B, L, causal, ldset, keys)


RAGGED_PARAMS = [(dt, "tier1") for dt in ALL] + [(dt, ldset) for ldset in ("min", "wide") for dt in (F32, BF16)]      # min / wide once per kernel type


@pytest.mark.parametrize("dt,ldset", RAGGED_PARAMS, ids=[f"{NAME[t]}-{s}" for t, s in RAGGED_PARAMS])
def test_attention_ragged_and_prefix(dt, ldset):
    """lpi_attn_fwd_varlen / _bwd_varlen / _bwd_prefix (rows_needed = 17) on lengths [59, 17, 32, 5]: rows >= row_start[B] are pads, lse entries l >= L_b need not be written."""
    full_case(dt, "ragged", len(RAGGED), max(RAGGED), 1, ldset, need=17)


@pytest.mark.parametrize("dt", ALL, ids=[NAME[t] for t in ALL])
def test_attention_shared_prefix(dt):
    """lpi_attn_fwd_shared / lpi_attn_bwd_shared (+ lpi_shared_kv_reduce into the strided dqkv) on own lengths [1, 7, 33, 60, 20] behind 17 shared rows; once more with
    rows_needed = 17 + 3 positions."""
    full_case(dt, "shared", 5, 0, 1, "tier1", need=PRE + 3)


# ---- layout strides plus a loose row stride ---------------------------------------------------------------------------------------------------------------------------
def text_problem(dt):
    return problem(dt, "uniform", 3, 40, 1)


def layout_arm(dt, pb, tx, B, L, rows, Ls, nbytes, label):
    M = pb["M"]
    a = Arm(Ls, nbytes)
    grouped = pb["qkv"].reshape(M, 3, H, HD).permute(0, 2, 1, 3).reshape(M, 3 * D)      # [row][head][q | k | v][64]
    a.mat("qkv", M, "ldqkv", TD[dt], grouped), a.mat("dctx", M, "lddctx", torch.bfloat16, pb["dctx"]), a.mat("ctx", M, "ldctx", TD[dt]), a.mat("ctx_pair", M, "ldctx", TD[dt])
    a.mat("dqkv", M, "lddqkv", torch.bfloat16)
    a.stat("lse", B * H * L), a.stat("lse_pair", B * H * L), a.stat("delta", B * H * L, unspecified=True)
    Mt = tx["M"]
    a.mat("qkv_t", Mt, "ldqkv_t", TD[dt], tx["qkv"]), a.mat("ctx_t", Mt, "ldctx_t", TD[dt]), a.stat("lse_t", 3 * H * 40)
    if rows:
        S.must_write(a.ops["dqkv"], prefix_rows(pb, rows))
    p, ld, st = a.p, a.ld, stream()
    lay = (3 * HD, HD, HD)
    va = (B, L, None, H, p["qkv"], ld["qkv"], p["ctx"], ld["ctx"], p["lse"], 0, 0, lay)
    vb = (B, L, None, H, p["qkv"], ld["qkv"], p["ctx_pair"], ld["ctx_pair"], p["lse_pair"], 0, 0, lay)
    launches(lambda: _lib.attn_fwd_one(dt, va, st), 1, label + " lpi_attn_fwd_one")
    launches(lambda: _lib.attn_fwd_pair(dt, vb, (3, 40, None, H, p["qkv_t"], ld["qkv_t"], p["ctx_t"], ld["ctx_t"], p["lse_t"], 1, 0), st), 1, label + " lpi_attn_fwd_pair")
    lay6 = (ctypes.c_int32 * 6)(3 * HD, HD, 3 * HD, HD, HD, HD)
    launches(lambda: call("lpi_attn_bwd_layout", dt, B, L, rows, H, p["qkv"], ld["qkv"], p["ctx"], ld["ctx"], p["dctx"], ld["dctx"], p["lse"], p["delta"], p["dqkv"], ld["dqkv"],
                          ctypes.cast(lay6, ctypes.c_void_p), st), bwd_launches(dt, L, 0, False, {}), label + " lpi_attn_bwd_layout")
    return a


LAYOUT_PARAMS = [(dt, 2, L, "tier1", rows) for dt in TWO for L in (50, 213) for rows in (0, 17)] + [(BF16, 2, 213, "min", 0), (BF16, 2, 213, "wide", 0)]


@pytest.mark.parametrize("dt,B,L,ldset,rows", LAYOUT_PARAMS, ids=[f"{NAME[t]}-{B}x{L}-{s}-rows{r}" for t, B, L, s, r in LAYOUT_PARAMS])
def test_attention_layout_forms(dt, B, L, ldset, rows):
    """lpi_attn_fwd_one / lpi_attn_fwd_pair / lpi_attn_bwd_layout on the head-grouped order with a row stride of 3d + 8 k elements (fused backward at L = 50, streamed
    at 213); the pair's partner is a causal text problem (3, 40, 2) on strided operands of its own."""
    pb, tx = problem(dt, "uniform", B, L, 0), text_problem(dt)
    label = f"layout {NAME[dt]} B={B} L={L} rows_needed={rows} {ldset}"
    Ls = make_lds(ldset, "full", dt)
    nbytes = case_bytes(pb["M"], Ls)
    with tuning(DEFAULT_KEYS):
        st, ti = layout_arm(dt, pb, tx, B, L, rows, Ls, nbytes, label), layout_arm(dt, pb, tx, B, L, rows, None, nbytes, label)
    AA.check_arms(label, st.ops, ti.ops, torch.cuda.synchronize)
    cbar, lbar, gbar = bars(dt, L)
    M = pb["M"]
    for tag in ("", "_pair"):
        held(label, "ctx" + tag, ti.vals("ctx" + tag, (M, D)), pb["ctx"], cbar)
        held(label, "lse" + tag, ti.vals("lse" + tag, (B, H, L)), pb["lse"], lbar)
    held(label, "ctx_t", ti.vals("ctx_t", (tx["M"], D)), tx["ctx"], cbar)
    held(label, "lse_t", ti.vals("lse_t", (3, H, 40)), tx["lse"], lbar)
    g = ti.vals("dqkv", (M, H, 3, HD)).permute(0, 2, 1, 3).reshape(M, 3 * D)
    keep = prefix_rows(pb, rows) if rows else list(range(M))
    for i, name in enumerate(("dq", "dk", "dv")):
        held(label, name, g[keep, i * D:(i + 1) * D], pb["grad"][keep, i * D:(i + 1) * D], gbar)


# ---- pooled-row attention -------------------------------------------------------------------------------------------------------------------------------------------
POOLED = {"uniform_causal": ("uniform", 3, 77, 1, [0, 40, 76]), "uniform_token0": ("uniform", 2, 21, 0, None), "ragged": ("ragged", 4, 59, 1, [n - 1 for n in RAGGED]),
          "shared": ("shared", 5, 0, 1, [PRE + n - 1 for n in (1, 7, 33, 60, 20)])}


@functools.lru_cache(maxsize=8)
def pooled_problem(dt, form):
    """One query per sample (position idx[b]; None: 0), K and V from columns d..3d of qkv: f64 ctx, lse, dq and dK | dV (zero behind the causal mask)."""
    kind, B, L, causal, idx = POOLED[form]
    seqs, M, rs, Lmax = sequences(kind, B, L)
    seqs = seqs[:B]
    pos = idx if idx is not None else [0] * B
    qkv = rnd(M, 3 * D, seed=21 + M, scale=0.7).to(TD[dt])
    q, dctx = rnd(B, D, seed=22 + M).to(TD[dt]), rnd(B, D, seed=23 + M).to(GD[dt])
    x, qr = qkv.double().requires_grad_(True), q.double().requires_grad_(True)
    ctx, lse = [], []
    for b, (rows, _) in enumerate(seqs):
        keys = torch.as_tensor(rows[:pos[b] + 1] if causal else rows)
        k, v = (x[keys, c * D:(c + 1) * D].reshape(len(keys), H, HD) for c in (1, 2))
        s = torch.einsum("hc,nhc->hn", qr[b].reshape(H, HD), k) / 8.0
        ctx.append(torch.einsum("hn,nhc->hc", torch.softmax(s, -1), v).reshape(D))
        lse.append(torch.logsumexp(s, -1))
    ctx = torch.stack(ctx)
    (ctx * dctx.double()).sum().backward()
    return dict(kind=kind, B=B, Lmax=Lmax, causal=causal, idx=idx, M=M, rs=rs, qkv=qkv, q=q, dctx=dctx, ctx=ctx.detach(), lse=torch.stack(lse).detach(), dq=qr.grad,
                dkv=x.grad[:, D:])


def pooled_ops(a, dt, pb, tag="", bump=0):
    """The operands of one pooled problem in arm `a` -> the lpi_attn_pooled_desc fields."""
    B, M = pb["B"], pb["M"]
    m = lambda name, *args, **kw: a.mat(name + tag, *args, bump=bump, **kw)  # noqa: E731
    m("q", B, "ldq", TD[dt], pb["q"]), m("qkv", M, "ldqkv", TD[dt], pb["qkv"]), m("dctx", B, "lddctx", GD[dt], pb["dctx"])
    shared = pb["kind"] == "shared"
    free = not shared and a.L is not None and "lddqkv_any" in a.L      # "min": an odd row step and an element-aligned pointer where no reduce follows
    m("ctx", B, "ldctx", TD[dt], any_pointer=True), m("dq", B, "lddq", GD[dt], any_pointer=True)
    m("dqkv", M, "lddqkv_any" if free else "lddqkv", GD[dt], col=D, any_pointer=not shared)      # the q columns of dqkv are pads: "columns 0..d are untouched"
    a.stat("lse" + tag, B * H)
    if shared:
        a.stat("shared_dkv" + tag, B * PRE * 2 * D)
    g = lambda name: a.p[name + tag]  # noqa: E731
    return dict(B=B, L=pb["Lmax"], H=H, row_start=None if pb["rs"] is None else torch.tensor(pb["rs"], dtype=torch.int32, device=DEV), q=g("q"), ldq=a.ld["q" + tag],
                qkv=g("qkv"), ldqkv=a.ld["qkv" + tag], idx=None if pb["idx"] is None else torch.tensor(pb["idx"], dtype=torch.int32, device=DEV), ctx=g("ctx"),
                ldctx=a.ld["ctx" + tag], lse=g("lse"), dctx=g("dctx"), lddctx=a.ld["dctx" + tag], dq=g("dq"), lddq=a.ld["dq" + tag], dqkv=g("dqkv"), lddqkv=a.ld["dqkv" + tag],
                causal=pb["causal"], shared_rows=PRE if shared else 0, shared_dkv=g("shared_dkv") if shared else None)


def pooled_sanity(label, dt, ti, pb, tag=""):
    B, M = pb["B"], pb["M"]
    cbar, lbar, gbar = bars(dt, pb["Lmax"])
    held(label, "ctx" + tag, ti.vals("ctx" + tag, (B, D)), pb["ctx"], cbar)
    held(label, "lse" + tag, ti.vals("lse" + tag, (B, H)), pb["lse"], lbar)
    held(label, "dq" + tag, ti.vals("dq" + tag, (B, D)), pb["dq"], gbar)
    g = ti.vals("dqkv" + tag, (M, 2 * D))
    held(label, "dk" + tag, g[:, :D], pb["dkv"][:, :D], gbar)
    held(label, "dv" + tag, g[:, D:], pb["dkv"][:, D:], gbar)


def pooled_arm(dt, form, Ls, nbytes, label):
    a = Arm(Ls, nbytes)
    st = stream()
    if form == "pair":
        ts = [pooled_ops(a, dt, pooled_problem(dt, f), f"[{i}]", 64 * i) for i, f in enumerate(("uniform_causal", "uniform_token0"))]
        launches(lambda: _lib.attn_pooled_pair(dt, ts[0], ts[1], st), 1, label + " lpi_attn_pooled_fwd_pair")
        launches(lambda: _lib.attn_pooled_pair(dt, ts[0], ts[1], st, backward=True), 1, label + " lpi_attn_pooled_bwd_pair")
        return a
    pb = pooled_problem(dt, form)
    t = pooled_ops(a, dt, pb)
    if form == "shared":      # the descriptor form: the only single-problem form that takes the shared-prefix fields
        launches(lambda: _lib.attn_pooled_one(dt, t, st), 1, label + " lpi_attn_pooled_fwd_desc")
        launches(lambda: _lib.attn_pooled_one(dt, t, st, backward=True), 2, label + " lpi_attn_pooled_bwd_desc + reduce")
    elif form == "ragged":
        launches(lambda: call("lpi_attn_pooled_fwd_varlen", dt, t["B"], t["L"], t["row_start"], H, t["q"], t["ldq"], t["qkv"], t["ldqkv"], t["idx"], t["ctx"], t["ldctx"],
                              t["lse"], t["causal"], st), 1, label + " forward")
        launches(lambda: call("lpi_attn_pooled_bwd_varlen", dt, t["B"], t["L"], t["row_start"], H, t["q"], t["ldq"], t["qkv"], t["ldqkv"], t["idx"], t["dctx"], t["lddctx"],
                              t["lse"], t["dq"], t["lddq"], t["dqkv"], t["lddqkv"], t["causal"], st), 1, label + " backward")
    else:
        launches(lambda: call("lpi_attn_pooled_fwd", dt, t["B"], t["L"], H, t["q"], t["ldq"], t["qkv"], t["ldqkv"], t["idx"], t["ctx"], t["ldctx"], t["lse"], t["causal"], st),
                 1, label + " forward")
        launches(lambda: call("lpi_attn_pooled_bwd", dt, t["B"], t["L"], H, t["q"], t["ldq"], t["qkv"], t["ldqkv"], t["idx"], t["dctx"], t["lddctx"], t["lse"], t["dq"],
                              t["lddq"], t["dqkv"], t["lddqkv"], t["causal"], st), 1, label + " backward")
    return a


POOLED_PARAMS = [(f, "tier1") for f in ("uniform_causal", "uniform_token0", "ragged", "pair", "shared")] + [("uniform_causal", "min"), ("shared", "min"), ("ragged", "wide")]


@pytest.mark.parametrize("form,ldset", POOLED_PARAMS, ids=[f"{f}-{s}" for f, s in POOLED_PARAMS])
@pytest.mark.parametrize("dt", ALL, ids=[NAME[t] for t in ALL])
def test_attention_pooled(dt, form, ldset):
    """lpi_attn_pooled_fwd / _bwd, their _varlen, _pair and _desc (shared prefix + lpi_shared_kv_reduce) forms: six leading dimensions, all different; dqkv's footprint
    is its K and V columns, all L rows of every sample (zeros behind the mask)."""
    label = f"pooled {form} {NAME[dt]} {ldset}"
    Ls = make_lds(ldset, "pooled", dt)
    forms = ("uniform_causal", "uniform_token0") if form == "pair" else (form,)
    nbytes = case_bytes(max(pooled_problem(dt, f)["M"] for f in forms), Ls)
    with tuning(DEFAULT_KEYS):
        st, ti = pooled_arm(dt, form, Ls, nbytes, label), pooled_arm(dt, form, None, nbytes, label)
    AA.check_arms(label, st.ops, ti.ops, torch.cuda.synchronize)
    for i, f in enumerate(forms):
        pooled_sanity(label, dt, ti, pooled_problem(dt, f), f"[{i}]" if form == "pair" else "")


# ---- the last block's attention from the residual stream --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def spool_problem(dt):
    """tests/test_round6_gpu.py::test_last_block_attention_from_the_stream_against_f64 at B = 2, L = 21, H = 2 (d = 128)."""
    B, L = 2, 21
    M, td = B * L, TD[dt]
    g = torch.Generator().manual_seed(B * 1000 + L)
    x = (torch.randn(M, D, generator=g) * 1.3 + 0.4 * torch.randn(M, 1, generator=g)).half()
    gamma, beta = 1.0 + 0.1 * torch.randn(D, generator=g), 0.05 * torch.randn(D, generator=g)
    W = (torch.randn(3 * D, D, generator=g) * D ** -0.5).to(td)
    bq = 0.02 * torch.randn(3 * D, generator=g)
    q, dctx = torch.randn(B, D, generator=g).to(td), torch.randn(B, D, generator=g).bfloat16()
    x64 = x.double()
    mean, rstd = x64.mean(1), 1.0 / (x64.var(1, unbiased=False) + 1e-5).sqrt()
    h = ((x64 - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double()).requires_grad_(True)
    qr = q.double().requires_grad_(True)
    Wd, bd = W.double(), bq.double()
    k, v = (h @ Wd[D:2 * D].t() + bd[D:2 * D]).view(B, L, H, HD), (h @ Wd[2 * D:].t() + bd[2 * D:]).view(B, L, H, HD)
    s = torch.einsum("bhc,blhc->bhl", qr.view(B, H, HD), k) / 8.0
    ctx = torch.einsum("bhl,blhc->bhc", torch.softmax(s, -1), v).reshape(B, D)
    (ctx * dctx.double()).sum().backward()
    return dict(B=B, L=L, M=M, x=x, gamma=gamma, beta=beta, W=W, bq=bq, q=q, dctx=dctx, mean=mean.float(), rstd=rstd.float(), ctx=ctx.detach(), dq=qr.grad, dh=h.grad)


def spool_arm(dt, pb, Ls, nbytes, label):
    B, L, M, td = pb["B"], pb["L"], pb["M"], TD[dt]
    a = Arm(Ls, nbytes)
    a.mat("q", B, "ldq", td, pb["q"]), a.mat("W", 3 * D, "ldw", td, pb["W"]), a.mat("WT", D, "ldwt", td, pb["W"].t()), a.mat("x", M, "ldx", torch.float16, pb["x"])
    Wb = pb["W"].bfloat16()      # the backward's weight operands are bf16 whatever the forward's type
    a.mat("Wb", 3 * D, "ldw", torch.bfloat16, Wb), a.mat("WbT", D, "ldwt", torch.bfloat16, Wb.t()), a.mat("dctx", B, "lddctx", torch.bfloat16, pb["dctx"])
    a.mat("ctx", B, "ldctx", td, any_pointer=True), a.mat("dq", B, "lddq", torch.bfloat16, any_pointer=True), a.mat("dh", M, "lddh", torch.bfloat16)
    a.stat("mean", M, pb["mean"]), a.stat("rstd", M, pb["rstd"]), a.stat("lse", B * H), a.stat("scratch", 4 * B * H * D, unspecified=True)
    bq, gamma, beta = pb["bq"].to(DEV), pb["gamma"].to(DEV), pb["beta"].to(DEV)
    p, ld, st = a.p, a.ld, stream()
    launches(lambda: call("lpi_spool_attn_fwd", dt, B, L, H, p["q"], ld["q"], p["W"], ld["W"], p["WT"], ld["WT"], bq, p["x"], ld["x"], p["mean"], p["rstd"], gamma, beta,
                          p["scratch"], p["lse"], p["ctx"], ld["ctx"], st), 3, label + " forward")
    launches(lambda: call("lpi_spool_attn_bwd", B, L, H, p["Wb"], ld["Wb"], p["WbT"], ld["WbT"], p["x"], ld["x"], p["mean"], p["rstd"], gamma, p["scratch"], p["lse"],
                          p["dctx"], ld["dctx"], p["dq"], ld["dq"], p["dh"], ld["dh"], st), 3, label + " backward")
    return a


SPOOL_PARAMS = [(BF16, "tier1"), (F16, "tier1"), (BF16, "min"), (BF16, "wide")]


@pytest.mark.parametrize("dt,ldset", SPOOL_PARAMS, ids=[f"{NAME[t]}-{s}" for t, s in SPOOL_PARAMS])
def test_last_block_attention_from_the_stream(dt, ldset):
    """lpi_spool_attn_fwd / _bwd (attn_stream.hip) at B = 2, L = 21, H = 2, d = 128: ldx, ldw, ldwt, ldq, ldctx, lddctx, lddq, lddh all different."""
    assert _lib.load().lpi_spool_attn_supported(21, H, D) == 1
    pb = spool_problem(dt)
    label = f"spool {NAME[dt]} {ldset}"
    Ls = make_lds(ldset, "spool", dt)
    nbytes = case_bytes(3 * D, Ls)      # the weight has the most rows
    with tuning(DEFAULT_KEYS):
        st, ti = spool_arm(dt, pb, Ls, nbytes, label), spool_arm(dt, pb, None, nbytes, label)
    AA.check_arms(label, st.ops, ti.ops, torch.cuda.synchronize)
    held(label, "ctx", ti.vals("ctx", (pb["B"], D)), pb["ctx"], SPOOL_BAR["ctx"], inclusive=True)
    held(label, "dq", ti.vals("dq", (pb["B"], D)), pb["dq"], SPOOL_BAR["dq"], inclusive=True)
    held(label, "dh", ti.vals("dh", (pb["M"], D)), pb["dh"], SPOOL_BAR["dh"], inclusive=True)


# ---- what the argument checks refuse ---------------------------------------------------------------------------------------------------------------------------------
def test_strides_and_pointers_the_kernels_cannot_take_are_refused_before_any_launch():
    """Per entry-point group: ldqkv < 3d and ldctx < d; a leading dimension that is no whole number of 16-byte units where the code needs one; a base pointer offset
    by 8 bytes where 16 are required (4 where 8 are).  LpiError, and lpi_launch_count() does not move.  Then every helper's unmodified arguments are shown to launch.  (Written from the checks as they stand: include/lpi_hip.h,
    "Alignment of the attention operands".)"""
    B, L, M = 2, 21, 42
    st = stream()
    z = lambda n, td=torch.bfloat16: torch.zeros(n, device=DEV, dtype=td)  # noqa: E731
    big = 256 * (3 * D + 64)
    qkv, ctx, dctx, dqkv, q, dq = z(big), z(big), z(big), z(big), z(big), z(big)
    qkv32, ctx32 = z(big, torch.float32), z(big, torch.float32)
    lse, delta, scratch = z(4096, torch.float32), z(4096, torch.float32), z(65536, torch.float32)
    rs = torch.tensor([PRE, PRE + 10, PRE + 31], dtype=torch.int32, device=DEV)
    idx = torch.tensor([PRE + 9, PRE + 20], dtype=torch.int32, device=DEV)
    refused = []

    def no(fn, *args):
        with pytest.raises(LpiError):
            fn(*args)
        refused.append(args[0] if isinstance(args[0], str) else fn.__name__)

    def fwd(dt=BF16, qkv=qkv, ldqkv=3 * D, ctx=ctx, ldctx=D):
        return ("lpi_attn_fwd", dt, B, L, H, qkv, ldqkv, ctx, ldctx, lse, 0, st)

    def bwd(qkv=qkv, ldqkv=3 * D, ctx=ctx, ldctx=D, dctx=dctx, lddctx=D, dqkv=dqkv, lddqkv=3 * D, dt=BF16):
        return ("lpi_attn_bwd", dt, B, L, H, qkv, ldqkv, ctx, ldctx, dctx, lddctx, lse, delta, dqkv, lddqkv, 0, st)

    def fwd_sh(ldqkv=3 * D, ctx=ctx, ldctx=D):
        return ("lpi_attn_fwd_shared", BF16, B, PRE + 21, rs, PRE, H, qkv, ldqkv, ctx, ldctx, lse, st)

    def bwd_sh(ldqkv=3 * D, ldctx=D, lddctx=D, dqkv=dqkv, lddqkv=3 * D, sc=scratch):
        return ("lpi_attn_bwd_shared", BF16, B, PRE + 21, rs, PRE, PRE + 21, H, qkv, ldqkv, ctx, ldctx, dctx, lddctx, lse, delta, dqkv, lddqkv, sc, st)

    def red(dt=BF16, dqkv=dqkv, lddqkv=3 * D):
        return ("lpi_shared_kv_reduce", dt, B, PRE, H, scratch, dqkv, lddqkv, 0, st)

    def one(qkv=qkv, ldqkv=3 * D, ctx=ctx, ldctx=D, lay=(3 * HD, HD, HD)):
        return (BF16, (B, L, None, H, qkv, ldqkv, ctx, ldctx, lse, 0, 0, lay), st)

    def lay_bwd(ldqkv=3 * D, ldctx=D, lddctx=D, dqkv=dqkv, lddqkv=3 * D):
        lay6 = (ctypes.c_int32 * 6)(3 * HD, HD, 3 * HD, HD, HD, HD)
        return ("lpi_attn_bwd_layout", BF16, B, L, 0, H, qkv, ldqkv, ctx, ldctx, dctx, lddctx, lse, delta, dqkv, lddqkv, ctypes.cast(lay6, ctypes.c_void_p), st)

    def pooled(**kw):
        t = dict(B=B, L=L, H=H, row_start=None, q=q, ldq=D, qkv=qkv, ldqkv=3 * D, idx=None, ctx=ctx, ldctx=D, lse=lse, dctx=dctx, lddctx=D, dq=dq, lddq=D, dqkv=dqkv,
                 lddqkv=3 * D, causal=0, shared_rows=0, shared_dkv=None)
        t.update(kw)
        return t

    def pfwd(t):
        return ("lpi_attn_pooled_fwd", BF16, B, L, H, t["q"], t["ldq"], t["qkv"], t["ldqkv"], None, t["ctx"], t["ldctx"], lse, 0, st)

    def pbwd(t):
        return ("lpi_attn_pooled_bwd", BF16, B, L, H, t["q"], t["ldq"], t["qkv"], t["ldqkv"], None, t["dctx"], t["lddctx"], lse, t["dq"], t["lddq"], t["dqkv"], t["lddqkv"], 0, st)

    w, wt, x, dh = z(3 * D * (D + 64)), z(D * (3 * D + 64)), z(big, torch.float16), z(big)
    gamma, beta, bqkv = z(D + 8, torch.float32), z(D + 8, torch.float32), z(3 * D, torch.float32)

    def sfwd(q=q, ldq=D, ldw=D, ldwt=3 * D, x=x, ldx=D, ldctx=D, gamma=gamma, beta=beta, sc=scratch):
        return ("lpi_spool_attn_fwd", BF16, B, L, H, q, ldq, w, ldw, wt, ldwt, bqkv, x, ldx, lse, lse, gamma, beta, sc, lse, ctx, ldctx, st)

    def sbwd(x=x, ldx=D, dctx=dctx, lddctx=D, lddq=D, dh=dh, lddh=D, gamma=gamma, sc=scratch):
        return ("lpi_spool_attn_bwd", B, L, H, w, D, wt, 3 * D, x, ldx, lse, lse, gamma, sc, lse, dctx, lddctx, dq, lddq, dh, lddh, st)

    rs0 = torch.tensor([0, 21, 42], dtype=torch.int32, device=DEV)

    def varlen(name, **kw):      # the _varlen / _prefix forms called directly (the plain forms delegate to them)
        a = dict(ldqkv=3 * D, ldctx=D, lddctx=D, lddqkv=3 * D, ldq=D, lddq=D, qkv=qkv, dctx=dctx)
        a.update(kw)
        return {"lpi_attn_fwd_varlen": (name, BF16, B, L, rs0, H, a["qkv"], a["ldqkv"], ctx, a["ldctx"], lse, 1, st),
                "lpi_attn_bwd_varlen": (name, BF16, B, L, rs0, H, a["qkv"], a["ldqkv"], ctx, a["ldctx"], a["dctx"], a["lddctx"], lse, delta, dqkv, a["lddqkv"], 1, st),
                "lpi_attn_bwd_prefix": (name, BF16, B, L, rs0, 17, H, a["qkv"], a["ldqkv"], ctx, a["ldctx"], a["dctx"], a["lddctx"], lse, delta, dqkv, a["lddqkv"], 1, st),
                "lpi_attn_pooled_fwd_varlen": (name, BF16, B, L, rs0, H, q, a["ldq"], a["qkv"], a["ldqkv"], None, ctx, a["ldctx"], lse, 0, st),
                "lpi_attn_pooled_bwd_varlen": (name, BF16, B, L, rs0, H, q, a["ldq"], a["qkv"], a["ldqkv"], None, a["dctx"], a["lddctx"], lse, dq, a["lddq"], dqkv, a["lddqkv"],
                                               0, st)}[name]

    n0 = _lib.launch_count()
    # lpi_attn_fwd / _bwd (and through them the _varlen / _prefix forms): rows too short | rows that do not end on 16 bytes | pointers 8 bytes off
    for args in (fwd(ldqkv=3 * D - 8), fwd(ldctx=D - 8), fwd(ldqkv=3 * D + 4), fwd(ldctx=D + 4), fwd(F32, qkv32, 3 * D + 2, ctx32, D), fwd(F32, qkv32, 3 * D, ctx32, D + 4),
                 fwd(qkv=qkv[4:]), fwd(ctx=ctx[4:]),
                 bwd(ldqkv=3 * D - 8), bwd(ldctx=D - 8), bwd(lddctx=D - 8), bwd(lddqkv=3 * D - 8), bwd(ldqkv=3 * D + 4), bwd(ldctx=D + 4), bwd(lddctx=D + 4), bwd(lddqkv=3 * D + 4),
                 bwd(qkv=qkv[4:]), bwd(ctx=ctx[4:]), bwd(dctx=dctx[4:]), bwd(dqkv=dqkv[4:]),
                 # the shared-prefix forms and the reduce (4-element rows, 8-byte pointer for a 2-byte dqkv; 16 bytes for f32)
                 fwd_sh(ldqkv=3 * D - 8), fwd_sh(ldctx=D - 8), fwd_sh(ldqkv=3 * D + 4), fwd_sh(ldctx=D + 4), fwd_sh(ctx=ctx[4:]),
                 bwd_sh(ldqkv=3 * D - 8), bwd_sh(ldctx=D - 8), bwd_sh(lddctx=D + 4), bwd_sh(lddqkv=3 * D + 4), bwd_sh(dqkv=dqkv[4:]), bwd_sh(sc=scratch[2:]),
                 red(lddqkv=3 * D - 4), red(lddqkv=3 * D + 2), red(dqkv=dqkv[2:]), red(F32, ctx32[2:]),
                 # the layout backward: 8 elements everywhere
                 lay_bwd(ldqkv=HD - 8), lay_bwd(ldctx=HD - 8), lay_bwd(ldqkv=3 * D + 4), lay_bwd(ldctx=D + 4), lay_bwd(lddctx=D + 4), lay_bwd(lddqkv=3 * D + 4), lay_bwd(dqkv=dqkv[4:]),
                 # the pooled forms: q, qkv and dctx rows and pointers (ctx, dq, dqkv are stored one element at a time and take any step >= the width)
                 pfwd(pooled(ldqkv=3 * D - 8)), pfwd(pooled(ldctx=D - 8)), pfwd(pooled(ldq=D + 4)), pfwd(pooled(ldqkv=3 * D + 4)), pfwd(pooled(q=q[4:])), pfwd(pooled(qkv=qkv[4:])),
                 pbwd(pooled(ldqkv=3 * D - 8)), pbwd(pooled(lddqkv=3 * D - 8)), pbwd(pooled(lddq=D - 8)), pbwd(pooled(lddctx=D + 4)), pbwd(pooled(dctx=dctx[4:])),
                 # the last block from the stream: 8-element rows of x, W, W^T, q, dctx; 4-element rows and an 8-byte pointer for dh
                 sfwd(ldx=D - 8), sfwd(ldctx=D - 8), sfwd(ldx=D + 4), sfwd(ldq=D + 4), sfwd(ldw=D + 4), sfwd(ldwt=3 * D + 4), sfwd(x=x[4:]), sfwd(q=q[4:]),
                 sbwd(lddq=D - 8), sbwd(lddh=D - 8), sbwd(ldx=D + 4), sbwd(lddctx=D + 4), sbwd(lddh=D + 2), sbwd(dctx=dctx[4:]), sbwd(dh=dh[2:]),
                 # ... its scratch, gamma and beta are moved as f32x4: 16-byte pointers (since library version 617)
                 sfwd(sc=scratch[2:]), sfwd(gamma=gamma[2:]), sfwd(beta=beta[2:]), sbwd(sc=scratch[2:]), sbwd(gamma=gamma[2:]),
                 # the ragged and prefix forms, called directly
                 varlen("lpi_attn_fwd_varlen", ldqkv=3 * D + 4), varlen("lpi_attn_fwd_varlen", ldctx=D + 4), varlen("lpi_attn_fwd_varlen", qkv=qkv[4:]),
                 varlen("lpi_attn_bwd_varlen", lddqkv=3 * D + 4), varlen("lpi_attn_bwd_varlen", lddctx=D - 8), varlen("lpi_attn_bwd_varlen", dctx=dctx[4:]),
                 varlen("lpi_attn_bwd_prefix", lddqkv=3 * D + 4), varlen("lpi_attn_bwd_prefix", ldctx=D + 4), varlen("lpi_attn_bwd_prefix", dctx=dctx[4:]),
                 varlen("lpi_attn_pooled_fwd_varlen", ldq=D + 4), varlen("lpi_attn_pooled_fwd_varlen", ldctx=D - 8), varlen("lpi_attn_pooled_fwd_varlen", qkv=qkv[4:]),
                 varlen("lpi_attn_pooled_bwd_varlen", lddctx=D + 4), varlen("lpi_attn_pooled_bwd_varlen", lddq=D - 8), varlen("lpi_attn_pooled_bwd_varlen", dctx=dctx[4:])):
        no(call, *args)
    for a in (one(ldqkv=HD - 8), one(ldctx=HD - 8), one(ldqkv=3 * D + 4), one(ldctx=D + 4), one(lay=(3 * HD + 4, HD, HD)), one(qkv=qkv[4:]), one(ctx=ctx[4:])):
        no(_lib.attn_fwd_one, *a)
        no(_lib.attn_fwd_pair, a[0], a[1], (B, L, None, H, qkv, 3 * D, ctx, D, lse, 1, 0), st)
    sh = dict(row_start=rs, idx=idx, causal=1, shared_rows=PRE, shared_dkv=scratch, L=PRE + 21)
    for t in (pooled(ldq=D + 4), pooled(q=q[4:]), pooled(ldqkv=3 * D - 8), pooled(ldctx=D - 8), pooled(ldq=D + 4, **sh), pooled(qkv=qkv[4:], **sh)):
        no(_lib.attn_pooled_one, BF16, t, st)
        no(_lib.attn_pooled_pair, BF16, pooled(), t, st)
    # on a shared prefix dqkv and shared_dkv go through lpi_shared_kv_reduce BEHIND the pooled kernel: its conditions (4-element rows, an 8-byte dqkv, a 16-byte
    # shared_dkv) are refused before that kernel runs (since library version 617)
    shared_bad = (pooled(lddqkv=3 * D + 2, **sh), pooled(dqkv=dqkv[2:], **sh), pooled(**dict(sh, shared_dkv=scratch[2:])))
    for t in (pooled(lddctx=D + 4), pooled(dctx=dctx[4:]), pooled(lddq=D - 8), pooled(lddctx=D + 4, **sh), pooled(dctx=dctx[4:], **sh)) + shared_bad:
        no(lambda *a: _lib.attn_pooled_one(*a, backward=True), BF16, t, st)
        no(lambda *a: _lib.attn_pooled_pair(*a, backward=True), BF16, pooled(), t, st)
    torch.cuda.synchronize()
    assert _lib.launch_count() == n0, "a refused call launched a kernel"
    print(f"{len(refused)} calls refused, nothing launched")

    # Every helper's UNMODIFIED argument list is accepted and launches what the dispatch implies: none of the refusals above is owed to a wrong baseline.
    def yes(want, fn, *args):
        launches(lambda: fn(*args), want, f"accepted {args[0] if isinstance(args[0], str) else fn.__name__}")

    with tuning(DEFAULT_KEYS):
        pair_text = (B, L, None, H, qkv, 3 * D, ctx, D, lse, 1, 0)
        for want, args in ((1, fwd()), (1, bwd()), (1, fwd_sh()), (2, bwd_sh()), (1, red()), (1, lay_bwd()), (1, pfwd(pooled())), (1, pbwd(pooled())), (3, sfwd()), (3, sbwd()),
                           (1, varlen("lpi_attn_fwd_varlen")), (1, varlen("lpi_attn_bwd_varlen")), (1, varlen("lpi_attn_bwd_prefix")),
                           (1, varlen("lpi_attn_pooled_fwd_varlen")), (1, varlen("lpi_attn_pooled_bwd_varlen")),
                           # the smallest accepted steps: the forward wants ldctx in 8 ELEMENTS for f32 too; a pooled ctx takes any step
                           (1, fwd(ldqkv=3 * D + 8, ldctx=D + 8)), (1, fwd(F32, qkv32, 3 * D + 4, ctx32, D + 8)), (1, pfwd(pooled(ldctx=D + 1)))):
            yes(want, call, *args)
        yes(1, _lib.attn_fwd_one, *one())
        yes(1, _lib.attn_fwd_pair, BF16, one()[1], pair_text, st)
        for t, extra in ((pooled(), 0), (pooled(**sh), 1)):      # extra: the reduce behind a shared-prefix backward
            yes(1, _lib.attn_pooled_one, BF16, t, st)
            yes(1, _lib.attn_pooled_pair, BF16, pooled(), t, st)
            yes(1 + extra, lambda *a: _lib.attn_pooled_one(*a, backward=True), BF16, t, st)
            yes(1 + extra, lambda *a: _lib.attn_pooled_pair(*a, backward=True), BF16, pooled(), t, st)
    torch.cuda.synchronize()


# ---- the LDS set-up of every kernel instantiation ---------------------------------------------------------------------------------------------------------------------
def test_every_large_lds_kernel_launches_in_one_process():
    """Every kernel of attention.hip and attention4.hip that asks for more than the default 64 KiB of LDS is launched here, in one process, at a length whose image
    exceeds 64 KiB: the permission is set once per (kernel instantiation, device) by an LdsOnce beside each launch, and a kernel whose set-up were skipped (or
    taken for a neighbour's) fails its launch.  Outputs per element against the f64 reference and bars of tests/attn_edges.py, launch counts as the dispatch implies
    (the batches, bars and checks of tests/test_attn_edges_gpu.py, imported here at call time: that module imports this one).
      forward <T, causal> (+ swizzled <2-byte, non-causal>), two-pass backward (f32; key 3 = 1), streamed backward in two windows: L = 288, each dtype, causal and not
      fused backward <bf16 | f16-saved, causal and not>: L = 224 (causal; non-causal with key 7 = 1), where four images take 145 KiB
      streamed backward <bf16 | f16-saved>, tuned (L = 224) and generic in two windows (L = 273)
      ragged causal: L = 288 among shorter samples
      pair forward <T, C0, C1>: (288 non-causal, 77 causal) on the swizzled images, (77 causal, 77 causal)."""
    import test_attn_edges_gpu as E
    for dt in ALL:
        for causal in (0, 1):
            pb = E.batch(dt, "random", "uniform", (288, 288), causal)
            for keys in ({}, {3: 1}) if dt != F32 else ({},):
                E.check_full(pb, keys, arm="random")
        E.check_full(E.batch(dt, "match", "ragged", E.RAGGED["long"], 1), {}, arm="match")
    for dt in TWO:
        td = TD[dt]
        E.check_full(E.batch(dt, "random", "uniform", (224, 224), 1), {}, arm="random")          # fused, causal
        pb = E.batch(dt, "random", "uniform", (224, 224), 0)
        E.check_full(pb, {7: 1}, arm="random")                                                     # fused, non-causal
        E.check_full(pb, {}, arm="random")                                                         # streamed, the Lp = 224 configuration
        E.check_full(E.batch(dt, "random", "uniform", (273, 273), 0), {}, arm="random")           # streamed, two key windows
        vis, txt = E.batch(dt, "random", "uniform", (288, 288), 0), E.batch(dt, "random", "uniform", (77, 77), 1)
        for first in (vis, txt):
            a = [(pb, E.nan(pb["M"], D, td=td), E.nan(2, H, pb["Lmax"])) for pb in (first, txt)]
            label = f"random pair {NAME[dt]} L={first['Lmax']} + 77"
            with tuning(DEFAULT_KEYS):
                launches(lambda: _lib.attn_fwd_pair(dt, *[(2, pb["Lmax"], None, H, pb["qkv"], 3 * D, ctx, D, lse, pb["causal"], 0) for pb, ctx, lse in a], E.stream()), 1, label)
            torch.cuda.synchronize()
            for pb, ctx, lse in a:
                E.hold(label, f"attention fwd pair {NAME[dt]}", "ctx", ctx.cpu(), pb["ref"]["ctx"], pb["bar"]["ctx"], E.AE.OLD_CTX[td])
                E.hold(label, f"attention fwd pair {NAME[dt]}", "lse", lse.cpu(), pb["ref"]["lse"], pb["bar"]["lse"], E.AE.OLD_LSE[td])
