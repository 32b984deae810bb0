"""Inputs and f64 references for the attention tests at head widths that end in HALF a 16-column tile — 88 (OpenCLIP ViT-g/14) and 104 (ViT-bigG/14).  This is
tests/attn_hd_cases.py with the head width HD a parameter (a plain helper module: no fixtures, no pytest settings; CPU only): the same modes, shapes, bars and
`late` arm; a case (HD, shape, arm, mode) is computed once and shared by every test that needs it (functools.lru_cache) — the tensors it returns are never written.

Arms:
    late    N(0, 1) data with the long test's dominant late key (key L - 7 of sample 0, head 0 = 2.5 x query 5: forces the running-max rescale; L >= 8)
    tail8   q, k, v and dctx are ZERO in the columns 0 .. HD - 9 of every head; the last eight columns HD - 8 .. HD - 1 — the live half of the last tile — hold
            2 x N(0, 1) (qkv) and N(0, 1) (dctx), with the seeds of attn_hd_cases' `upper`: a kernel that drops, mis-pads or mis-masks the half tile sees
            all-zero scores, a uniform softmax and zero values
"""
import functools

import torch

from attn_hd_cases import BARS, MODES, SHAPES, bars, relerr, rnd, uniform_lse  # noqa: F401  (one set of bars, modes and shapes for the family)

WIDTHS = (88, 104)
TAIL8_SHAPES = [(2, 17, 2), (2, 129, 2), (1, 273, 2)]


def attn_ref(HD, qkv, B, L, H):
    """-> ctx [B L, H HD], lse [B, H, L], scores [B, H, L, L] (f64)"""
    d = H * HD
    q, k, v = qkv.double().reshape(B, L, 3, H, HD).permute(2, 0, 3, 1, 4)
    s = (q * HD ** -0.5) @ k.transpose(-1, -2)
    p = torch.softmax(s, -1)
    return (p @ v).transpose(1, 2).reshape(B * L, d), torch.logsumexp(s, -1), s


def raw_inputs(HD, B, L, H, arm):
    """f32 master data of a case: qkv [B L, 3 H HD], dctx [B L, H HD]"""
    d = H * HD
    qkv, dctx = rnd(B * L, 3 * d, seed=11), rnd(B * L, d, seed=12)
    if arm == "late":
        if L >= 8:
            qkv[L - 7, d:d + HD] = qkv[5, :HD] * 2.5          # key L - 7 matches query 5 of sample 0, head 0
    elif arm == "tail8":
        low = (torch.arange(d) % HD) < HD - 8
        qkv = qkv * 2.0
        dctx[:, low] = 0.0
        qkv[:, low.repeat(3)] = 0.0
    else:
        raise ValueError(arm)
    return qkv, dctx


@functools.lru_cache(maxsize=None)
def case(HD, B, L, H, arm, mode):
    """-> dict of CPU tensors: qkv, dctx (in the mode's types) and the f64 references ctx, lse, delta, dqkv, scores.  Shared: do not write to them."""
    _, td, tg = MODES[mode]
    scale = HD ** -0.5
    qkv, dctx = raw_inputs(HD, B, L, H, arm)
    qkv, dctx = qkv.to(td), dctx.to(tg)
    qr = qkv.double().requires_grad_(True)
    oref, lref, s = attn_ref(HD, qr, B, L, H)
    oref.backward(dctx.double())
    o = oref.detach()
    delta = (o * dctx.double()).view(B, L, H, HD).sum(-1).permute(0, 2, 1).contiguous()
    # the scale at which dq = scale dS k and dk = scale dS^T q are formed: |dS| <= |dP| + |delta| with dP = dctx v^T (attn_hd_cases.case)
    q, k, v = qkv.double().reshape(B, L, 3, H, HD).permute(2, 0, 3, 1, 4)
    dp = dctx.double().reshape(B, L, H, HD).transpose(1, 2) @ v.transpose(-1, -2)
    unit = scale * float(dp.abs().max())
    return {"qkv": qkv, "dctx": dctx, "ctx": o, "lse": lref.detach(), "delta": delta, "dqkv": qr.grad.detach(), "scores": s.detach(),
            "unit_dq": unit * float(k.abs().max()), "unit_dk": unit * float(q.abs().max())}


def tail8_premises(ref, L):
    """What makes `tail8` a test of the half tile, asserted on the f64 reference alone before any kernel result is looked at: every query's scores spread over
    the keys by more than 1, lse lies more than 1 off the uniform softmax's log L somewhere, and ctx is not small.  -> (spread, lse offset, max |ctx|)"""
    s = ref["scores"]
    spread = float((s.max(-1).values - s.min(-1).values).min())
    off = float((ref["lse"] - uniform_lse(L)).abs().max())
    top = float(ref["ctx"].abs().max())
    assert spread > 1.0, spread
    assert off > 1.0, off
    assert top > 0.5, top
    return spread, off, top


def errors(HD, mode, H, ctx, lse, delta, dqkv, ref):
    """relerr of each output tensor against the case's references: {name: error}"""
    d = H * HD
    e = {"ctx": relerr(ctx, ref["ctx"]), "lse": relerr(lse, ref["lse"]), "delta": relerr(delta, ref["delta"])}
    for name, sl in (("dq", slice(0, d)), ("dk", slice(d, 2 * d)), ("dv", slice(2 * d, 3 * d))):
        e[name] = relerr(dqkv[:, sl], ref["dqkv"][:, sl], ref.get("unit_" + name))
    return e


def head_cols(HD, H, h, parts=3):
    """column indices of head h in a [*, parts H HD] matrix"""
    d = H * HD
    return torch.cat([torch.arange(w * d + h * HD, w * d + (h + 1) * HD) for w in range(parts)])
