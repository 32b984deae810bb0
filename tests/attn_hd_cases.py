"""Inputs and f64 references for the 80-wide-head attention tests (a plain helper module: no fixtures, no pytest settings; CPU only).

The reference is `attn_ref` of tests/test_kernels_gpu.py with 80 for 64 and 80^-0.5 for 0.125, under f64 autograd, on the inputs ROUNDED to the mode's storage
types; a case (shape, arm, mode) is computed once and shared by every test that needs it (functools.lru_cache) — the tensors it returns are never written.

Arms:
    late    N(0, 1) data with the long test's dominant late key (key L - 7 of sample 0, head 0 = 2.5 x query 5: forces the running-max rescale; L >= 8)
    upper   q, k, v and dctx are ZERO in the columns 0 .. 63 of every head and 2 x N(0, 1) in 64 .. 79: a kernel that drops or mis-pads the last 16 columns
            sees all-zero scores, a uniform softmax and zero values
"""
import functools
import math

import torch

from lpi_amd._lib import BF16, F16, F32

HD = 80
SCALE = HD ** -0.5

# mode -> (dtype code, storage type of qkv / ctx, type of dctx / dqkv)
MODES = {"f32": (F32, torch.float32, torch.float32), "bf16": (BF16, torch.bfloat16, torch.bfloat16), "f16": (F16, torch.float16, torch.bfloat16)}

# both sides of every block edge a 16-, 32-, 64- or 128-row tiling can have, the two lengths the real towers use (257 + 16 prompts; ViT-L/14@336's 577),
# the boundary between the existing short and long families (289) and the envelope's end
SHAPES = [(2, 1, 1), (2, 15, 2), (1, 16, 1), (2, 17, 2), (1, 31, 1), (1, 32, 2), (2, 33, 1), (1, 127, 2), (1, 128, 1), (2, 129, 2), (1, 273, 2), (1, 289, 1),
          (1, 577, 1), (1, 1024, 1)]

# the project's own bars for the key-walking family (tests/test_kernels_gpu.py::test_attention_long_sequences_fwd_bwd): relerr = max |got - ref| / max |ref|
BARS = {"f32": {"ctx": 2e-5, "lse": 1e-5, "delta": 1e-5, "dq": 5e-5, "dk": 5e-5, "dv": 5e-5},
        "2byte": {"ctx": 2e-2, "lse": 2e-2, "delta": 2e-2, "dq": 4e-2, "dk": 4e-2, "dv": 4e-2}}


def bars(mode):
    return BARS["f32" if mode == "f32" else "2byte"]


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def relerr(got, ref, unit=None):
    """max |got - ref| / max |ref| (tests/test_kernels_gpu.py).  Where the reference is IDENTICALLY zero the quotient means nothing — at L = 1 the softmax is the
    constant 1, so dq = dk = 0 exactly while the kernel's dS = p (dP - delta) is round-off of the terms it subtracts — and the error is taken relative to `unit`,
    the magnitude of those terms (see case()): the same bar, on the scale the gradient is computed at.  Every other reference is measured as before."""
    got, ref = got.double().cpu(), ref.double().cpu()
    den = float(ref.abs().max())
    if unit is not None and den < 1e-9 * unit:
        den = unit
    return float((got - ref).abs().max() / (den + 1e-30))


def attn_ref(qkv, B, L, H):
    """-> ctx [B L, H 80], lse [B, H, L], scores [B, H, L, L] (f64)"""
    d = H * HD
    q, k, v = qkv.double().reshape(B, L, 3, H, HD).permute(2, 0, 3, 1, 4)
    s = (q * SCALE) @ k.transpose(-1, -2)
    p = torch.softmax(s, -1)
    return (p @ v).transpose(1, 2).reshape(B * L, d), torch.logsumexp(s, -1), s


def raw_inputs(B, L, H, arm):
    """f32 master data of a case: qkv [B L, 3 H 80], dctx [B L, H 80]"""
    d = H * HD
    qkv, dctx = rnd(B * L, 3 * d, seed=11), rnd(B * L, d, seed=12)
    if arm == "late":
        if L >= 8:
            qkv[L - 7, d:d + HD] = qkv[5, :HD] * 2.5          # key L - 7 matches query 5 of sample 0, head 0
    elif arm == "upper":
        low = (torch.arange(d) % HD) < 64
        qkv = qkv * 2.0
        dctx[:, low] = 0.0
        qkv[:, low.repeat(3)] = 0.0
    else:
        raise ValueError(arm)
    return qkv, dctx


@functools.lru_cache(maxsize=None)
def case(B, L, H, arm, mode):
    """-> dict of CPU tensors: qkv, dctx (in the mode's types) and the f64 references ctx, lse, delta, dqkv, scores.  Shared: do not write to them."""
    _, td, tg = MODES[mode]
    qkv, dctx = raw_inputs(B, L, H, arm)
    qkv, dctx = qkv.to(td), dctx.to(tg)
    qr = qkv.double().requires_grad_(True)
    oref, lref, s = attn_ref(qr, B, L, H)
    oref.backward(dctx.double())
    o = oref.detach()
    delta = (o * dctx.double()).view(B, L, H, HD).sum(-1).permute(0, 2, 1).contiguous()
    # the scale at which dq = scale dS k and dk = scale dS^T q are formed: |dS| <= |dP| + |delta| with dP = dctx v^T
    q, k, v = qkv.double().reshape(B, L, 3, H, HD).permute(2, 0, 3, 1, 4)
    dp = dctx.double().reshape(B, L, H, HD).transpose(1, 2) @ v.transpose(-1, -2)
    unit = SCALE * float(dp.abs().max())
    return {"qkv": qkv, "dctx": dctx, "ctx": o, "lse": lref.detach(), "delta": delta, "dqkv": qr.grad.detach(), "scores": s.detach(),
            "unit_dq": unit * float(k.abs().max()), "unit_dk": unit * float(q.abs().max())}


def errors(mode, H, ctx, lse, delta, dqkv, ref):
    """relerr of each output tensor against the case's references: {name: error}"""
    d = H * HD
    e = {"ctx": relerr(ctx, ref["ctx"]), "lse": relerr(lse, ref["lse"]), "delta": relerr(delta, ref["delta"])}
    for name, sl in (("dq", slice(0, d)), ("dk", slice(d, 2 * d)), ("dv", slice(2 * d, 3 * d))):
        e[name] = relerr(dqkv[:, sl], ref["dqkv"][:, sl], ref.get("unit_" + name))
    return e


def head_cols(H, h, parts=3):
    """column indices of head h in a [*, parts H 80] matrix"""
    d = H * HD
    return torch.cat([torch.arange(w * d + h * HD, w * d + (h + 1) * HD) for w in range(parts)])


def uniform_lse(L):
    return math.log(L)
