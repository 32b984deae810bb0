"""The attention family at its tile edges, per element, on adversarial masks (real MI355X): lpi_attn_fwd / _bwd and the _varlen / _prefix / _shared forms (attention.hip,
attention4.hip, attn_long.hip, attn_softmax.h), lpi_shared_kv_reduce, the pooled forms (attn_pooled.hip), lpi_spool_attn_fwd / _bwd (attn_stream.hip), and one case each of
the pair and layout forms.

Every output ELEMENT is held to the bar tests/attn_edges.py derives from the f64 reference (the roundings the kernels' code performs, counted there; nothing is taken
from a kernel's output), and the relerr bars of the existing tests stay as a second assertion (ctx, lse: every arm; gradients: the `random` arm).  The inputs are that module's arms: `negative` (a masked key that keeps
its zero score takes the whole row), `match` (every key and every query decides one row), `forbidden` (every masked pair scores above every allowed one), `staircase`
(rows of one wave cross ATTN_DEFER_THR tile after tile, or just do not), `random`.  Two samples x two heads with different data per (sample, head): a cross-sample or
cross-head mix-up shows.  Lengths: every 16 / 32-row tile edge, the dispatch's thresholds (224, 288, 1024) and their neighbours.  The tuning keys select every kernel
body the dispatch can reach by name; the launch counts are asserted (tests/test_attn_strides_gpu.py: tuning, launches, bwd_launches).  Outputs start as NaN: an
element nobody wrote fails.  A length the header documents as refused (causal or ragged behind 288) is asserted to raise and to launch nothing.
Each line "EDGE ..." printed is a measured worst |got - ref| / bar ("Tile edges and masks of the attention family").
"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_edges as AE  # noqa: E402
from lpi_amd import _lib  # noqa: E402
from lpi_amd._lib import BF16, F16, F32, LpiError, call  # noqa: E402
from test_attn_strides_gpu import bwd_launches, launches, tuning  # noqa: E402

DEV = "cuda:0"
TD = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
ALL = [F32, BF16, F16]
H, HD = 2, AE.HD
D = H * HD
DEFAULT_KEYS = {3: 0, 7: 0, 9: 0, 11: 0, 12: 0, 13: 0}
SHORT = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 223, 224, 225, 255, 256, 257, 287, 288]
LONG = [289, 303, 304, 305, 319, 320, 321, 383, 384, 385, 1023, 1024]
SUBSET = {17, 33, 97, 225, 257, 288, 305, 1023}      # one length per tile class for the `random`, `forbidden` and `staircase` arms


def stream():
    return torch.cuda.current_stream().cuda_stream


def nan(*shape, td=torch.float32):
    return torch.full(shape, float("nan"), dtype=td, device=DEV)


def hold(label, kernel, out, got, ref, bar, old=None, scale=None):
    """Per element inside the bar, no NaN; `old`: the relerr bar of the existing tests (max |got - ref| / max |ref| of the whole tensor) on top: for ctx and lse on
    every arm and type, for dq / dk / dv on the `random` arm, the data those bars were set for — the other arms make the gradients small on purpose (dS of a
    one-hot row cancels to nothing), so max |ref| is no scale for their errors.  scale: that max |ref| where `ref` is a few rows of the tensor (rows_needed = 1
    under the causal mask: dq of position 0 is 0).
    The `staircase` arm's scores reach 175 (|q . k| = 1400: ONE f32 rounding of such a product is 2^-24 * 1400 / 8 = 1e-5 of p), which 2e-5 of max |ctx| cannot
    hold for an f32 kernel of any order of summation: there the f32 ctx is held by its per-element bar alone (lse, absolute in the log domain, keeps the old bar)."""
    arm = label.split()[0]
    if (out not in ("ctx", "lse") and arm != "random") or (out == "ctx" and arm == "staircase" and kernel.endswith("f32")):
        old = None
    r = AE.worst(got, ref, bar)
    print(f"EDGE kernel={kernel} out={out} ratio={r:.4f} | {label}")
    assert r < 1.0, (label, kernel, out, r)
    if old is not None and ref.numel():
        e = AE.relerr(got, ref) if scale is None else float((got.double() - ref).abs().max()) / scale
        assert e < old, (label, kernel, out, "relerr", e, old)


# ---- a batch: sequences -> operands, reference, bars ----------------------------------------------------------------------------------------------------------------
def layout(kind, lens, pre=0):
    """-> [(global rows of the sequence's positions, first query position)], row count, row_start or None, longest sequence.  shared: own lengths `lens` behind `pre`
    shared rows; sequence index B is the shared sequence itself."""
    if kind == "uniform":
        L = lens[0]
        return [(list(range(b * L, (b + 1) * L)), 0) for b in range(len(lens))], len(lens) * L, None, L
    rs = [pre]
    for n in lens:
        rs.append(rs[-1] + n)
    own = [list(range(rs[b], rs[b + 1])) for b in range(len(lens))]
    if kind == "ragged":
        return [(r, 0) for r in own], rs[-1], rs, max(lens)
    sh = list(range(pre))
    return [(sh + r, pre) for r in own] + [(sh, 0)], rs[-1], rs, pre + max(lens)


@functools.lru_cache(maxsize=8)
def batch(dt, arm, kind, lens, causal, pre=0):
    """Operands as stored, the f64 reference and the per-element bars of one batch: computed once, shared by the tuning variants, never written."""
    td, gd = TD[dt], AE.grad_type(TD[dt])
    seqs, M, rs, Lmax = layout(kind, list(lens), pre)
    slices = []
    for b, (rows, q_from) in enumerate(seqs):
        shared_seq = kind == "shared" and b == len(seqs) - 1
        slices.append([AE.make(arm, len(rows), (900 + h) if shared_seq else 100 * b + 10 * h + len(rows), td, causal=causal, shared=0 if shared_seq else pre,
                               shared_seed=900 + h, sign=-1.0 if kind == "ragged" and b % 2 else 1.0) for h in range(H)])
    qkv, dctx = AE.pack(slices, [r for r, _ in seqs], M, H)
    exact = AE.is_bf16(qkv)
    ns = len(seqs)
    ref = dict(ctx=torch.zeros(M, D, dtype=AE.F64), lse=torch.zeros(ns, H, Lmax, dtype=AE.F64), dqkv=torch.zeros(M, 3 * D, dtype=AE.F64))
    bar = {k: torch.zeros_like(v) for k, v in ref.items()}
    live = torch.zeros(ns, H, Lmax, dtype=torch.bool)
    for b, (rows, q_from) in enumerate(seqs):
        r, own = torch.as_tensor(rows), torch.as_tensor(rows[q_from:])
        nq = len(own)
        for h, sl in enumerate(slices[b]):
            R = AE.attend(sl["q"][q_from:], sl["k"], sl["v"], AE.causal_mask(nq, len(rows), q_from, causal), sl["dctx"][q_from:])
            Bz = AE.bars(R, td, exact_bf16=exact)
            c = slice(h * HD, (h + 1) * HD)
            for dst, src in ((ref, R), (bar, Bz)):
                dst["ctx"][own, c], dst["lse"][b, h, :nq] = src["ctx"], src["lse"]
                dst["dqkv"][own, c] += src["dq"]
                dst["dqkv"][r, D + h * HD:D + (h + 1) * HD] += src["dk"]      # shared keys: the batch sum (lpi_shared_kv_reduce), bars add
                dst["dqkv"][r, 2 * D + h * HD:2 * D + (h + 1) * HD] += src["dv"]
            live[b, h, :nq] = True
    if kind == "shared":      # the reduce stores the sum once more on top of the shared sequence's own store: 2 u of the total
        bar["dqkv"][:pre, D:] += 2.0 * AE.U[gd] * ref["dqkv"][:pre, D:].abs()
    return dict(dt=dt, kind=kind, causal=causal, pre=pre, seqs=seqs, M=M, rs=rs, Lmax=Lmax, B=ns - (kind == "shared"), qkv=qkv.to(td).to(DEV), dctx=dctx.to(gd).to(DEV),
                ref=ref, bar=bar, live=live, slices=slices)


def fwd_body(dt, L, causal, ragged, keys):
    if L > 288:
        return "attn_long fwd"
    Lp = (L + 31) // 32 * 32
    sw = dt != F32 and not causal and not ragged and keys.get(13, 0) != 1 and 4 * Lp * 160 > 160 * 1024 and 4 * Lp * 128 <= 160 * 1024
    return "attention fwd swizzled" if sw else "attention fwd"


def bwd_body(dt, L, causal, ragged, keys):
    """Which backward the dispatch of lpi_attn_bwd_prefix runs (attention.hip), by name."""
    if L > 288:
        return "attn_long bwd"
    if dt == F32 or keys.get(3, 0):
        return "attention bwd two-pass"
    if not ragged and not causal and (keys.get(7, 0) == 5 or (keys.get(7, 0) == 0 and L > 160)):
        return "attention4 bwd streamed" + (" two windows" if L > 224 else "")
    Lp = (L + 31) // 32 * 32
    return "attention bwd fused" if 4 * Lp * 160 + 8 * Lp <= 160 * 1024 else "attention bwd two-pass"


# launches of each backward body: held against test_attn_strides_gpu.bwd_launches in run_full, so the two readings of the dispatch cannot drift apart unnoticed
BWD_LAUNCHES = {"attn_long bwd": 2, "attention bwd two-pass": 2, "attention4 bwd streamed": 1, "attention4 bwd streamed two windows": 2, "attention bwd fused": 1}


def variants(dt, L, causal, ragged):
    """Tuning keys that reach every kernel body the dispatch has for this case, one per distinct (forward, backward) body."""
    if L > 288 or dt == F32:
        return [{}]
    seen, out = set(), []
    for keys in ({}, {7: 1}, {7: 5}, {3: 1}, {13: 1}, {7: 5, 11: 1}):
        body = (fwd_body(dt, L, causal, ragged, keys), bwd_body(dt, L, causal, ragged, keys), keys.get(11, 0) if "streamed" in bwd_body(dt, L, causal, ragged, keys) else 0)
        if body not in seen:
            seen.add(body)
            out.append(keys)
    return out


def run_full(pb, keys, need=0):
    """Forward + backward of a batch under `keys` -> ctx, lse, dqkv on the CPU (outputs start as NaN), and the names of the bodies that ran."""
    dt, kind, causal, B, Lmax, M = pb["dt"], pb["kind"], pb["causal"], pb["B"], pb["Lmax"], pb["M"]
    td, gd = TD[dt], AE.grad_type(TD[dt])
    ns = B + (kind == "shared")
    ctx, dqkv, lse, delta = nan(M, D, td=td), nan(M, 3 * D, td=gd), nan(ns, H, Lmax), nan(ns, H, Lmax)
    rs = None if pb["rs"] is None else torch.tensor(pb["rs"], dtype=torch.int32, device=DEV)
    qkv, dctx, st = pb["qkv"], pb["dctx"], stream()
    label = f"{kind} {NAME[dt]} L={Lmax} causal={causal} keys={keys} need={need}"
    nb = BWD_LAUNCHES[bwd_body(dt, Lmax, causal, rs is not None, keys)]
    assert nb == bwd_launches(dt, Lmax, causal, rs is not None, keys), label
    with tuning({**DEFAULT_KEYS, **keys}):
        if kind == "shared":
            part = nan(B * pb["pre"] * 2 * D)
            launches(lambda: call("lpi_attn_fwd_shared", dt, B, Lmax, rs, pb["pre"], H, qkv, 3 * D, ctx, D, lse, st), 1, label + " forward")
            launches(lambda: call("lpi_attn_bwd_shared", dt, B, Lmax, rs, pb["pre"], need or Lmax, H, qkv, 3 * D, ctx, D, dctx, D, lse, delta, dqkv, 3 * D, part, st), nb + 1,
                     label + " backward + reduce")
        else:
            launches(lambda: call("lpi_attn_fwd_varlen", dt, B, Lmax, rs, H, qkv, 3 * D, ctx, D, lse, causal, st) if rs is not None else
                     call("lpi_attn_fwd", dt, B, Lmax, H, qkv, 3 * D, ctx, D, lse, causal, st), 1, label + " forward")
            if need:
                launches(lambda: call("lpi_attn_bwd_prefix", dt, B, Lmax, rs, need, H, qkv, 3 * D, ctx, D, dctx, D, lse, delta, dqkv, 3 * D, causal, st), nb, label + " backward")
            else:
                launches(lambda: call("lpi_attn_bwd_varlen", dt, B, Lmax, rs, H, qkv, 3 * D, ctx, D, dctx, D, lse, delta, dqkv, 3 * D, causal, st) if rs is not None else
                         call("lpi_attn_bwd", dt, B, Lmax, H, qkv, 3 * D, ctx, D, dctx, D, lse, delta, dqkv, 3 * D, causal, st), nb, label + " backward")
    torch.cuda.synchronize()
    return label, ctx.cpu(), lse.cpu(), dqkv.cpu(), fwd_body(dt, Lmax, causal, rs is not None, keys), bwd_body(dt, Lmax, causal, rs is not None, keys)


def check_full(pb, keys, need=0, arm=""):
    label, ctx, lse, dqkv, fb, bb = run_full(pb, keys, need)
    label = f"{arm} {label}"
    td = TD[pb["dt"]]
    ref, bar, live = pb["ref"], pb["bar"], pb["live"]
    long_f16 = pb["Lmax"] > 288 and td == torch.float16      # the existing long-sequence test holds f16 to bf16's bars
    old_c, old_l = (AE.OLD_CTX[torch.bfloat16], AE.OLD_LSE[torch.bfloat16]) if long_f16 else (AE.OLD_CTX[td], AE.OLD_LSE[td])
    tag = f"{fb} {NAME[pb['dt']]}"
    hold(label, tag, "ctx", ctx, ref["ctx"], bar["ctx"], old_c)
    hold(label, tag, "lse", lse[live], ref["lse"][live], bar["lse"][live], old_l)
    rows = list(range(pb["M"]))
    if need:      # the positions below rows_needed of every sequence are held to the bar; the rest may be left unwritten
        rows = sorted({r for seq, _ in pb["seqs"] for r in seq[:need]})
    tag = f"{bb} {NAME[pb['dt']]}"
    for i, name in enumerate(("dq", "dk", "dv")):
        c = slice(i * D, (i + 1) * D)
        hold(label, tag, name, dqkv[rows][:, c], ref["dqkv"][rows][:, c], bar["dqkv"][rows][:, c], AE.OLD_GRAD[td], scale=float(ref["dqkv"][:, c].abs().max()) + 1e-30)


# ---- uniform batches: every tile edge x every body ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", SHORT + LONG)
@pytest.mark.parametrize("dt", ALL, ids=[NAME[t] for t in ALL])
def test_uniform_lengths(dt, L):
    """lpi_attn_fwd / lpi_attn_bwd, causal and not.  `negative` and `match` at every length, the other arms at one length per tile class."""
    B = 1 if L > 512 else 2
    for causal in (0, 1):
        if L > 288 and causal:      # include/lpi_hip.h: "causal or ragged sequences of that length are refused with LPI_EINVAL" — asserted, and nothing launches
            z = torch.zeros(B * L, 3 * D, dtype=TD[dt], device=DEV)
            n0 = _lib.launch_count()
            with pytest.raises(LpiError):
                call("lpi_attn_fwd", dt, B, L, H, z, 3 * D, z, D, nan(B, H, L), 1, stream())
            with pytest.raises(LpiError):
                call("lpi_attn_bwd", dt, B, L, H, z, 3 * D, z, D, z, D, nan(B, H, L), nan(B, H, L), z, 3 * D, 1, stream())
            assert _lib.launch_count() == n0
            continue
        arms = ["negative", "match"]
        if L in SUBSET:
            arms += ["random"] + (["forbidden"] if causal else []) + (["staircase"] if L > 32 else [])
        for arm in arms:
            pb = batch(dt, arm, "uniform", (L,) * B, causal)
            for keys in variants(dt, L, causal, False):
                check_full(pb, keys, arm=arm)


# ---- ragged batches -------------------------------------------------------------------------------------------------------------------------------------------------
RAGGED = {"short": (59, 1, 2, 16, 17, 32, 33), "long": (1, 2, 16, 17, 32, 33, 59, 288)}      # fused backward | the two-pass kernels (four images of 288 rows do not fit)


@pytest.mark.parametrize("lens", list(RAGGED), ids=list(RAGGED))
@pytest.mark.parametrize("dt", ALL, ids=[NAME[t] for t in ALL])
def test_ragged_lengths(dt, lens):
    """lpi_attn_fwd_varlen / _bwd_varlen.  `forbidden` (causal), `match`, and non-causal `negative` with its sign alternating from sample to sample: a sample that
    reads one key of its neighbour gives it the whole row."""
    for causal, arms in ((1, ("forbidden", "match")), (0, ("match", "negative"))):
        for arm in arms:
            pb = batch(dt, arm, "ragged", RAGGED[lens], causal)
            for keys in ({}, {3: 1}) if dt != F32 and lens == "short" else ({},):
                check_full(pb, keys, arm=arm)
    n0 = _lib.launch_count()      # a ragged batch behind 288 is refused (include/lpi_hip.h)
    rs = torch.tensor([0, 289, 300], dtype=torch.int32, device=DEV)
    z = torch.zeros(300, 3 * D, dtype=TD[dt], device=DEV)
    g = torch.zeros(300, 3 * D, dtype=AE.grad_type(TD[dt]), device=DEV)
    with pytest.raises(LpiError):
        call("lpi_attn_fwd_varlen", dt, 2, 289, rs, H, z, 3 * D, z, D, nan(2, H, 289), 0, stream())
    with pytest.raises(LpiError):
        call("lpi_attn_bwd_varlen", dt, 2, 289, rs, H, z, 3 * D, z, D, g, D, nan(2, H, 289), nan(2, H, 289), g, 3 * D, 0, stream())
    with pytest.raises(LpiError):
        call("lpi_attn_bwd_prefix", dt, 2, 289, rs, 17, H, z, 3 * D, z, D, g, D, nan(2, H, 289), nan(2, H, 289), g, 3 * D, 0, stream())
    assert _lib.launch_count() == n0


# ---- rows_needed ----------------------------------------------------------------------------------------------------------------------------------------------------
PREFIX = {"uniform-causal-77": ("uniform", (77, 77), 1), "uniform-213": ("uniform", (213, 213), 0), "uniform-273": ("uniform", (273, 273), 0),
          "ragged-causal": ("ragged", RAGGED["short"], 1)}


@pytest.mark.parametrize("form", list(PREFIX), ids=list(PREFIX))
@pytest.mark.parametrize("dt", ALL, ids=[NAME[t] for t in ALL])
def test_rows_needed(dt, form):
    """lpi_attn_bwd_prefix: rows_needed at every 16 / 32-row edge, L - 1 and L; the positions below rows_needed are held to the bar (the rest may stay NaN)."""
    kind, lens, causal = PREFIX[form]
    L = max(lens)
    for arm in ("random", "match"):
        pb = batch(dt, arm, kind, lens, causal)
        for need in (1, 16, 17, 31, 32, 33, L - 1, L):
            for keys in variants(dt, L, causal, kind == "ragged"):
                if 13 not in keys:
                    check_full(pb, keys, need=need, arm=arm)


# ---- shared prefix --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", [1, 2, 16, 17, 32, 33])
@pytest.mark.parametrize("dt", ALL, ids=[NAME[t] for t in ALL])
def test_shared_prefix_lengths(dt, pre):
    """lpi_attn_fwd_shared / lpi_attn_bwd_shared + lpi_shared_kv_reduce's batch sum; own lengths include 1 and both sides of a tile edge."""
    for arm in ("forbidden", "match", "random"):
        pb = batch(dt, arm, "shared", (1, 7, 33, 60, 2, 31), 1, pre)
        check_full(pb, {}, arm=arm)
    pb = batch(dt, "random", "shared", (1, 7, 33, 60, 2, 31), 1, pre)
    check_full(pb, {}, need=pre + 3, arm="random")


# ---- pooled forms ---------------------------------------------------------------------------------------------------------------------------------------------------
POOL_LENS = (33, 40, 16, 17, 32, 59, 59, 59)
POOL_IDX = (0, 1, 15, 16, 31, 32, 57, 58)       # 0, 1, 15, 16, 31, 32, L - 2, L - 1


@pytest.mark.parametrize("form", ["varlen-causal", "varlen-token0", "desc-shared"])
@pytest.mark.parametrize("dt", ALL, ids=[NAME[t] for t in ALL])
def test_pooled_rows(dt, form):
    """lpi_attn_pooled_fwd_varlen / _bwd_varlen (causal with idx; token 0 without a mask) and the _desc form on a shared prefix of 17 rows.  dK / dV behind the causal
    limit are exact zeros."""
    td, gd = TD[dt], AE.grad_type(TD[dt])
    causal, pre = int(form != "varlen-token0"), 17 if form == "desc-shared" else 0
    B = len(POOL_LENS)
    idx = [0] * B if not causal else [i + (pre if i >= 15 else 0) for i in POOL_IDX] if pre else list(POOL_IDX)      # shared: positions on both sides of the prefix's end
    for arm in ("negative", "match", "random"):
        pb = batch(dt, arm, "shared" if pre else "ragged", POOL_LENS, causal, pre)
        M, Lmax = pb["M"], pb["Lmax"]
        q, dctx = torch.zeros(B, D, dtype=AE.F64), torch.zeros(B, D, dtype=AE.F64)
        ref = dict(ctx=torch.zeros(B, D, dtype=AE.F64), lse=torch.zeros(B, H, dtype=AE.F64), dq=torch.zeros(B, D, dtype=AE.F64), dkv=torch.zeros(M, 2 * D, dtype=AE.F64))
        bar = {k: torch.zeros_like(v) for k, v in ref.items()}
        dead = torch.ones(M, dtype=torch.bool)
        for b in range(B):
            rows = torch.as_tensor(pb["seqs"][b][0])
            n = len(rows)
            for h, sl in enumerate(pb["slices"][b]):
                c = slice(h * HD, (h + 1) * HD)
                q[b, c], dctx[b, c] = sl["q"][idx[b]], sl["dctx"][idx[b]]
                R = AE.attend(sl["q"][idx[b]:idx[b] + 1], sl["k"], sl["v"], AE.causal_mask(n, n, causal=causal)[idx[b]:idx[b] + 1], sl["dctx"][idx[b]:idx[b] + 1])
                Bz = AE.bars(R, td, AE.POOLED)
                for dst, src in ((ref, R), (bar, Bz)):
                    dst["ctx"][b, c], dst["lse"][b, h], dst["dq"][b, c] = src["ctx"][0], src["lse"][0], src["dq"][0]
                    dst["dkv"][rows, c] += src["dk"]
                    dst["dkv"][rows, D + h * HD:D + (h + 1) * HD] += src["dv"]
            dead[rows[:idx[b] + 1] if causal else rows] = False
        if pre:
            bar["dkv"][:pre] += 2.0 * AE.U[gd] * ref["dkv"][:pre].abs()      # the reduce's store
        ctx, lse, dq, dqkv = nan(B, D, td=td), nan(B, H), nan(B, D, td=gd), nan(M, 3 * D, td=gd)
        t = dict(B=B, L=Lmax, H=H, row_start=torch.tensor(pb["rs"], dtype=torch.int32, device=DEV), q=q.to(td).to(DEV), ldq=D, qkv=pb["qkv"], ldqkv=3 * D,
                 idx=torch.tensor(idx, dtype=torch.int32, device=DEV) if causal else None, ctx=ctx, ldctx=D, lse=lse, dctx=dctx.to(gd).to(DEV), lddctx=D, dq=dq, lddq=D,
                 dqkv=dqkv, lddqkv=3 * D, causal=causal, shared_rows=pre, shared_dkv=nan(B * pre * 2 * D) if pre else None)
        label, st = f"{arm} pooled {form} {NAME[dt]}", stream()
        with tuning(DEFAULT_KEYS):
            if pre:
                launches(lambda: _lib.attn_pooled_one(dt, t, st), 1, label + " forward")
                launches(lambda: _lib.attn_pooled_one(dt, t, st, backward=True), 2, label + " backward + reduce")
            else:
                launches(lambda: call("lpi_attn_pooled_fwd_varlen", dt, B, Lmax, t["row_start"], H, t["q"], D, t["qkv"], 3 * D, t["idx"], ctx, D, lse, causal, st), 1, label + " forward")
                launches(lambda: call("lpi_attn_pooled_bwd_varlen", dt, B, Lmax, t["row_start"], H, t["q"], D, t["qkv"], 3 * D, t["idx"], t["dctx"], D, lse, dq, D, dqkv, 3 * D, causal,
                                      st), 1, label + " backward")
        torch.cuda.synchronize()
        tag = f"attn_pooled {NAME[dt]}"
        hold(label, tag, "ctx", ctx.cpu(), ref["ctx"], bar["ctx"], AE.OLD_CTX[td])
        hold(label, tag, "lse", lse.cpu(), ref["lse"], bar["lse"], AE.OLD_LSE[td])
        hold(label, tag, "dq", dq.cpu(), ref["dq"], bar["dq"], AE.OLD_GRAD[td])
        g = dqkv.cpu()[:, D:]
        hold(label, tag, "dk", g[:, :D], ref["dkv"][:, :D], bar["dkv"][:, :D], AE.OLD_GRAD[td])
        hold(label, tag, "dv", g[:, D:], ref["dkv"][:, D:], bar["dkv"][:, D:], AE.OLD_GRAD[td])
        assert dead.any() == bool(causal) and bool((g[dead].double() == 0).all()), label + ": dK / dV behind the causal limit are exact zeros"
        assert bool(torch.isnan(dqkv.cpu()[:, :D].float()).all()), label + ": the q columns of dqkv are untouched"


# ---- pair and layout forms: held bit for bit to the single forms elsewhere; here once on the `negative` arm, so that the equality is not two equal mistakes -------
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_pair_and_layout_on_the_negative_arm(dt):
    td = TD[dt]
    L, Lt = 273, 33
    pb, tx = batch(dt, "negative", "uniform", (L, L), 0), batch(dt, "negative", "uniform", (Lt, Lt), 1)
    M = pb["M"]
    st = stream()
    # head-grouped order [row][head][q | k | v][64] (tests/test_attn_strides_gpu.py: layout_arm)
    grouped = pb["qkv"].reshape(M, 3, H, HD).permute(0, 2, 1, 3).reshape(M, 3 * D).contiguous()
    ctx, lse, ctx_t, lse_t, dqkv = nan(M, D, td=td), nan(2, H, L), nan(tx["M"], D, td=td), nan(2, H, Lt), nan(M, 3 * D, td=torch.bfloat16)
    lay = (3 * HD, HD, HD)
    lay6 = (ctypes.c_int32 * 6)(3 * HD, HD, 3 * HD, HD, HD, HD)
    label = f"negative pair + layout {NAME[dt]}"
    with tuning(DEFAULT_KEYS):
        launches(lambda: _lib.attn_fwd_pair(dt, (2, L, None, H, grouped, 3 * D, ctx, D, lse, 0, 0, lay), (2, Lt, None, H, tx["qkv"], 3 * D, ctx_t, D, lse_t, 1, 0), st), 1,
                 label + " lpi_attn_fwd_pair")
        launches(lambda: call("lpi_attn_bwd_layout", dt, 2, L, 0, H, grouped, 3 * D, ctx, D, pb["dctx"], D, lse, nan(2, H, L), dqkv, 3 * D, ctypes.cast(lay6, ctypes.c_void_p), st),
                 bwd_launches(dt, L, 0, False, {}), label + " lpi_attn_bwd_layout")
    torch.cuda.synchronize()
    hold(label, f"attention fwd pair {NAME[dt]}", "ctx", ctx.cpu(), pb["ref"]["ctx"], pb["bar"]["ctx"], AE.OLD_CTX[td])
    hold(label, f"attention fwd pair {NAME[dt]}", "lse", lse.cpu(), pb["ref"]["lse"], pb["bar"]["lse"], AE.OLD_LSE[td])
    hold(label, f"attention fwd pair {NAME[dt]}", "ctx", ctx_t.cpu(), tx["ref"]["ctx"], tx["bar"]["ctx"], AE.OLD_CTX[td])
    hold(label, f"attention fwd pair {NAME[dt]}", "lse", lse_t.cpu(), tx["ref"]["lse"], tx["bar"]["lse"], AE.OLD_LSE[td])
    g = dqkv.cpu().reshape(M, H, 3, HD).permute(0, 2, 1, 3).reshape(M, 3 * D)
    for i, name in enumerate(("dq", "dk", "dv")):
        c = slice(i * D, (i + 1) * D)
        hold(label, f"attention4 bwd layout {NAME[dt]}", name, g[:, c], pb["ref"]["dqkv"][:, c], pb["bar"]["dqkv"][:, c], AE.OLD_GRAD[td])


# ---- the last block's attention from the residual stream ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 31, 32, 33, 224, 225, 287, 288])
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_last_block_from_the_stream_lengths(dt, L):
    """lpi_spool_attn_fwd / _bwd (attn_stream.hip), d = 128, against the literal f64 evaluation (tests/test_round6_gpu.py) at the tile edges, one- and two-row
    sequences and both sides of 224 / 288.  ctx, dq and dh at the relerr bars of the kernel's existing test (1e-2, 1.5e-2, 1.5e-2, inclusive) on both arms, and ctx
    per element inside the bar attn_edges.spool_reference counts.  On the `negative` arm (every real row about -20 below a row of zeros, shaped through x and W_k)
    that bar is 2 .. 3 % of |ctx| and a padded row that kept a weight would take the row; on `random` it is loose at long L (tests/test_attn_edges_host.py).  A shape
    lpi_spool_attn_supported refuses is asserted to raise and to launch nothing."""
    td, B = TD[dt], 2
    for arm in ("random", "negative"):
        c = AE.spool_case(arm, B, L, H, td)
        dev = lambda t, ty: t.to(ty).to(DEV).contiguous()  # noqa: E731
        x, W, q, dctx = dev(c["x"], torch.float16), dev(c["W"], td), dev(c["q"], td), dev(c["dctx"], torch.bfloat16)
        WT, Wb = dev(c["W"].t(), td), dev(c["W"], torch.bfloat16)      # the backward's weight operands are bf16 whatever the forward's type
        WbT = dev(c["W"].to(torch.bfloat16).t(), torch.bfloat16)
        f32 = lambda name: dev(c[name], torch.float32)  # noqa: E731
        mean, rstd, gamma, beta, bq = f32("mean"), f32("rstd"), f32("gamma"), f32("beta"), f32("bq")
        ctx, dq, dh, lse, scratch = nan(B, D, td=td), nan(B, D, td=torch.bfloat16), nan(B * L, D, td=torch.bfloat16), nan(B, H), nan(4 * B * H * D)
        label, st = f"{arm} spool {NAME[dt]} L={L}", stream()
        fwd = lambda: call("lpi_spool_attn_fwd", dt, B, L, H, q, D, W, D, WT, 3 * D, bq, x, D, mean, rstd, gamma, beta, scratch, lse, ctx, D, st)  # noqa: E731
        bwd = lambda: call("lpi_spool_attn_bwd", B, L, H, Wb, D, WbT, 3 * D, x, D, mean, rstd, gamma, scratch, lse, dctx, D, dq, D, dh, D, st)  # noqa: E731
        if _lib.load().lpi_spool_attn_supported(L, H, D) != 1:
            n0 = _lib.launch_count()
            for fn in (fwd, bwd):
                with pytest.raises(LpiError):
                    fn()
            assert _lib.launch_count() == n0, label
            continue
        ref = AE.spool_reference(c, td)
        with tuning(DEFAULT_KEYS):
            launches(fwd, 3, label + " forward")
            launches(bwd, 3, label + " backward")
        torch.cuda.synchronize()
        e = {n: AE.relerr(t.cpu(), ref[n]) for n, t in (("ctx", ctx), ("dq", dq), ("dh", dh))}
        print(f"EDGE-RELERR {label} ctx={e['ctx']:.3e} dq={e['dq']:.3e} dh={e['dh']:.3e}")
        hold(label, f"attn_stream fwd {NAME[dt]}", "ctx", ctx.cpu(), ref["ctx"], ref["ctx_bar"])
        if L == 1:      # a softmax over one key has no gradient: the reference's dq is 0 and relerr has no scale; the absolute bar counted in spool_reference
            hold(label, f"attn_stream bwd {NAME[dt]}", "dq", dq.cpu(), ref["dq"], ref["dq_bar1"])
            e["dq"] = 0.0
        assert e["ctx"] <= 1e-2 and e["dq"] <= 1.5e-2 and e["dh"] <= 1.5e-2, (label, e)
