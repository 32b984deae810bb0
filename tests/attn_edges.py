"""Tile edges and masks of the attention family: the f64 reference, its per-element bars, the input arms and the reference's mutants (a plain helper module
next to attn_arms.py: CPU only, no fixtures, no pytest settings).  tests/test_attn_edges_gpu.py holds the HIP kernels to it, tests/test_attn_edges_host.py
proves on the CPU that an honest kernel stays inside the bars and that each mistake the arms were built for leaves them by a factor of ten or more.

ONE reference for every form.  A (sample, head) slice is q [nq, 64], k, v [nk, 64], an `allowed` matrix [nq, nk] and dctx [nq, 64]; `attend` returns ctx, lse,
P and dq / dk / dv in f64.  Causal, ragged, shared-prefix, rows_needed and pooled forms differ only in which rows are keys, which are queries and what
`allowed` holds (`causal_mask`).  Inputs arrive already rounded to the operand type.

BARS are per element and come from the reference, never from a kernel's output.  u = 2^-9 (bf16), 2^-12 (f16), 2^-24 (f32); one round-to-nearest store into a
type moves a value by at most 2 u of its magnitude (bf16 keeps 8 significant bits).  Counted roundings (lpi_amd/csrc):

  MFMA kernels (attention.hip attn_fwd_body, attn_walk.h, the 2-byte types):
    P -> operand type in mma_transposed (pack2_t, attention.hip; attn_walk.h pack2_t<TM>)                                2 u of every addend p_ij v_jc
    o * inv -> operand type in store_row16_t / Elem<T>::st4                                                               2 u of |ctx| <= sum_j P_ij |v_jc|
    the row sum lsum adds the UNROUNDED f32 p (attn_softmax.h: ps += s0 + s1 before the pack), 1 / ltot and o * inv are f32: in EPS below
                                                                                                               c_fwd = 4;  f32 operands: nothing is packed,
    the reciprocal and the product are one f32 rounding each: c_fwd = 2 (u = 2^-24)
  MFMA backwards (attn_bwd_fused_kernel, attn_bwd_dq_kernel / attn_bwd_dkv_kernel, attention4.hip, attn_walk.h; gradients bf16 for both 2-byte modes):
    dS = P (dP - delta) / 8 -> bf16, P -> bf16 in mma_transposed                                                          2 u of every addend
    dq / dk / dv -> bf16 in store_row_bf16_t                                                                              2 u of the sum      c_bwd = 4 (f32: 2)
    delta = rowsum(ctx * dctx) reads the STORED ctx (load_row_chunks of ctx in phase A): its error, c_fwd u_ctx sum_c (P |v|)_ic |dctx_ic| =: c_fwd u_ctx D_i,
    enters every dS_ij as P_ij D_i / 8 — NOT small beside |dS_ij| where dP - delta cancels (a one-hot row), so it is a term of its own
    f16 mode: q, k, v are converted to bf16 on their way into LDS (stage_rows4<T, SV16>, CV0 / CV1 of stage_rows2): exact for operands that are bf16 values
    (every arm but `random`); else 2^-8 of every factor, counted in `eps_bwd` (cv)
  pooled kernels (attn_pooled.hip): all arithmetic f32, one Elem<T>::st per output: c_fwd = c_bwd = 2, delta is recomputed in f32 (no stored ctx).

  EPS_i, the f32 arithmetic on row i's scores (relative error of an unnormalised p_ij): a 64-term f32 dot product (<= 64 * 2^-24 of sum_c |q_ic k_jc|), the scale,
  the fmaf with the reference point (|arg| <= |s| c + |m|) and v_exp_f32 / __expf (2 ulp), the f32 row sum over nk keys:
      EPS_i = 2^-24 (67 max_j sum_c |q_ic k_jc| / 8 + 10 + nk).
  A normalised P_ij carries 2 EPS_i (numerator and row sum).
  ctx bar (i, c) = (c_fwd u + 2 EPS_i) sum_j P_ij |v_jc|   (+ f16 operands: 2^-25 max_j P_ij sum_j |v_jc| — an f16 p below 2^-14 of the row's reference point is
                   subnormal and carries 2^-25 ABSOLUTE; the reference point never exceeds the row maximum, so the largest p is >= 1)
  lse bar (i)    = EPS_i + 3 * 2^-24 (max_j |s_ij| + 16 ln 2 + ln nk + |lse_i|) + 2^-21        (m + log2f(ltot)) * LN2: m sits up to 8 in the log2 domain below
                                                                                                the row maximum (ATTN_DEFER_THR), ltot <= 256 nk; log2f ~ 2^-21 absolute
  dq bar (i, c)  = c_bwd u_g sum_j |dS_ij| |k_jc| + sum_j P_ij (sum_c ctx bar_ic |dctx_ic|) / 8 |k_jc| + sum_j EPSB_i aDS_ij |k_jc|,
                   aDS_ij = P_ij (sum_c |dctx_ic v_jc| + D_i) / 8
  Every bar has the absolute floor 2^-120 (f32 underflow: far keys of the `forbidden` arm have p ~ e^-500).
  dk, dv: the same with the roles of the rows exchanged (dv has no delta term: addends P_ij dctx_ic).
  EPSB_i = 2 lse bar_i + 2 EPS_i + 2^-24 (64 + nq) (+ cv): the backward recomputes P from the forward's f32 lse.
"""
import math

import torch

F64 = torch.float64
HD = 64
U = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}
E32 = 2.0 ** -24
FLOOR = 2.0 ** -120      # f32 (and bf16) underflow: a p, dS or product below 2^-126 is flushed — an absolute floor under every bar (64 addends of 2^-126)
# kernel class -> counted constants (the module docstring says where each rounding was read)
MFMA = dict(name="mfma", c_fwd={2: 4, 4: 2}, c_bwd={2: 4, 4: 2}, stored_ctx=True, converts=True)
POOLED = dict(name="pooled", c_fwd={2: 2, 4: 2}, c_bwd={2: 2, 4: 2}, stored_ctx=False, converts=False)
# the bars every attention test had before this file (relerr = max |got - ref| / max |ref|), kept as a second assertion
OLD_CTX = {torch.float32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 3e-3}
OLD_LSE = {torch.float32: 1e-5, torch.bfloat16: 2e-2, torch.float16: 3e-3}
OLD_GRAD = {torch.float32: 5e-5, torch.bfloat16: 4e-2, torch.float16: 4e-2}


def esize(td):
    return 4 if td == torch.float32 else 2


def grad_type(td):
    """Gradients of the f16 mode are bf16."""
    return torch.float32 if td == torch.float32 else torch.bfloat16


def rt(x, td):
    """x rounded to `td`, back in f64."""
    return x.to(td).to(F64)


def relerr(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


# ---- masks ----------------------------------------------------------------------------------------------------------------------------------------------------------
def causal_mask(nq, nk, q_from=0, causal=True, shift=0):
    """allowed[i, j]: query i sits at position q_from + i, key j at position j.  shift: the MUTANTS' off-by-one (+1: one key of the future, -1: the diagonal
    lost; a row left without any key keeps key 0)."""
    if not causal:
        return torch.ones(nq, nk, dtype=torch.bool)
    i = torch.arange(nq)[:, None] + q_from
    j = torch.arange(nk)[None, :]
    a = j <= i + shift
    a[:, 0] |= ~a.any(1)
    return a


# ---- the reference --------------------------------------------------------------------------------------------------------------------------------------------------
def attend(q, k, v, allowed, dctx=None, extra_k=None, extra_v=None, dkv_weight=None):
    """f64 attention of one (sample, head) slice and its gradients.  extra_k / extra_v: keys every query sees behind the slice's own (mutants: a phantom zero key,
    a neighbour's key); dkv_weight [nq]: the weight of each query in the dK / dV sums (mutant: the last query dropped).  -> dict."""
    q, k, v = q.to(F64), k.to(F64), v.to(F64)
    nq, nk = q.shape[0], k.shape[0]
    if extra_k is not None:
        k, v = torch.cat([k, extra_k.to(F64)]), torch.cat([v, extra_v.to(F64)])
        allowed = torch.cat([allowed, torch.ones(nq, extra_k.shape[0], dtype=torch.bool)], 1)
    s = (q @ k.t()) * 0.125
    s = s.masked_fill(~allowed, float("-inf"))
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[:, None])
    R = dict(q=q, k=k, v=v, allowed=allowed, s=s, P=P, lse=lse, ctx=P @ v, nk=nk)
    if dctx is not None:
        dctx = dctx.to(F64)
        dP = dctx @ v.t()
        delta = (R["ctx"] * dctx).sum(-1)
        dS = P * (dP - delta[:, None]) * 0.125
        w = torch.ones(nq, dtype=F64) if dkv_weight is None else dkv_weight.to(F64)
        R.update(dctx=dctx, dS=dS, dq=dS @ k, dk=((dS * w[:, None]).t() @ q)[:nk], dv=((P * w[:, None]).t() @ dctx)[:nk])
    return R


def bars(R, td, kern=MFMA, exact_bf16=True):
    """The per-element bars of a reference result R for operand type td (module docstring) -> dict(ctx, lse[, dq, dk, dv])."""
    u, gd = U[td], grad_type(td)
    ug = U[gd]
    q, k, v, P, s, al = R["q"], R["k"], R["v"], R["P"], R["s"], R["allowed"]
    nq, nk = s.shape
    A = (q.abs() @ k.abs().t()).masked_fill(~al, 0.0).max(-1).values
    eps = E32 * (67.0 * A / 8.0 + 10.0 + nk)
    PV = P @ v.abs()
    c_fwd = kern["c_fwd"][esize(td)]
    smax = s.masked_fill(~al, 0.0).abs().max(-1).values
    ctx_bar = (c_fwd * u + 2.0 * eps)[:, None] * PV
    if td == torch.float16 and kern["name"] == "mfma":      # an f16 p below 2^-14 of the row's reference point is subnormal: 2^-25 absolute, the row maximum p >= 1
        ctx_bar = ctx_bar + 2.0 ** -25 * P.max(-1).values[:, None] * (al.to(F64) @ v.abs())
    ctx_bar = ctx_bar + FLOOR
    out = dict(ctx=ctx_bar,
               lse=eps + 3.0 * E32 * (smax + 16.0 * math.log(2.0) + math.log(nk) + R["lse"].abs()) + 2.0 ** -21)
    if "dctx" in R:
        dctx, dS = R["dctx"], R["dS"]
        c_bwd = kern["c_bwd"][esize(gd)]
        D = (PV * dctx.abs()).sum(-1)
        aDS = P * (dctx.abs() @ v.abs().t() + D[:, None]) * 0.125
        epsb = 2.0 * out["lse"] + 2.0 * eps + E32 * (64.0 + nq)
        if td == torch.float16 and kern["converts"] and not exact_bf16:
            epsb = epsb + 2.0 ** -8 * (2.0 * A / 8.0 + 1.0)      # q, k (scores) and v (dP) rounded to bf16
            c_bwd = c_bwd + 2                                     # and the k / q factor of every dq / dk addend
        dl = P * (ctx_bar * dctx.abs()).sum(-1)[:, None] * 0.125 if kern["stored_ctx"] else 0.0      # delta from the stored ctx: off by at most sum_c ctx bar |dctx|
        E = c_bwd * ug * dS.abs() + dl + epsb[:, None] * aDS      # what one dS_ij may be off by
        nk0 = R["nk"]
        out.update(dq=E @ k.abs() + FLOOR, dk=(E.t() @ q.abs())[:nk0] + FLOOR, dv=(((c_bwd * ug + epsb)[:, None] * P).t() @ dctx.abs())[:nk0] + FLOOR)
    return out


def worst(got, ref, bar):
    """max |got - ref| / bar; an element whose bar is 0 must be met exactly; NaN anywhere -> inf."""
    d = (got.to(F64) - ref.to(F64)).abs()
    if not bool(torch.isfinite(d).all()):
        return float("inf")
    r = torch.where(bar > 0, d / bar.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    return float(r.max()) if r.numel() else 0.0


# ---- an honest kernel, emulated: f64 with the counted roundings applied ---------------------------------------------------------------------------------------------
def emulate(q, k, v, allowed, dctx, td, kern=MFMA, frozen_max=False):
    """-> dict(ctx, lse, dq, dk, dv).  frozen_max: the MUTANT whose running maximum never moves after the first 32-key tile — p = exp2(.) in f32 against the
    first tile's maximum, as the kernel would compute it (it overflows where the scores climb)."""
    gd = grad_type(td)
    two, mf = esize(td) == 2, kern["name"] == "mfma"
    s = ((q @ k.t()) * 0.125).masked_fill(~allowed, float("-inf"))
    if frozen_max:
        m = s[:, :32].max(-1, keepdim=True).values
        p = torch.exp2(((s - m) * math.log2(math.e)).float()).double()
    else:
        m = s.max(-1, keepdim=True).values
        p = torch.exp(s - m)
    lsum = p.sum(-1, keepdim=True)
    pr = rt(p, td) if (two and mf) else p
    ctx = rt((pr @ v) / lsum, td)
    lse = rt((m + torch.log(lsum))[:, 0], torch.float32)
    qb, kb, vb = (rt(x, torch.bfloat16) for x in (q, k, v)) if (td == torch.float16 and kern["converts"]) else (q, k, v)
    Pb = torch.exp(((qb @ kb.t()) * 0.125).masked_fill(~allowed, float("-inf")) - lse[:, None])
    delta = ((ctx if kern["stored_ctx"] else Pb @ vb) * dctx).sum(-1)
    dS = Pb * (dctx @ vb.t() - delta[:, None]) * 0.125
    dSr, Pr = (rt(dS, gd), rt(Pb, gd)) if mf else (dS, Pb)
    return dict(ctx=ctx, lse=lse, dq=rt(dSr @ kb, gd), dk=rt(dSr.t() @ qb, gd), dv=rt(Pr.t() @ dctx, gd))


# ---- input arms -----------------------------------------------------------------------------------------------------------------------------------------------------
ARMS = ("random", "negative", "match", "forbidden", "staircase")


def _table(n, seed, shared, shared_seed, cols):
    own = torch.randn(n, cols, generator=torch.Generator().manual_seed(seed), dtype=F64)
    if shared:
        own[:shared] = torch.randn(shared, cols, generator=torch.Generator().manual_seed(shared_seed), dtype=F64)
    return own


def match_target(n, seed, causal):
    """pi: the key that dominates each query.  Non-causal: a seeded permutation (every key decisive for one row); causal: i, i - 1, 0 in turn."""
    if not causal:
        return torch.randperm(n, generator=torch.Generator().manual_seed(seed + 7))
    i = torch.arange(n)
    return torch.where(i % 3 == 0, i, torch.where(i % 3 == 1, (i - 1).clamp_min(0), torch.zeros_like(i)))


def make(arm, n, seed, td, causal=False, shared=0, shared_seed=1000, sign=1.0):
    """q, k, v (rounded to td) and dctx (rounded to the gradient type) of ONE (sample, head) slice of n positions, f64 [n, 64] each.  The first `shared` positions
    come from shared_seed alone (the shared prefix: the same rows in every sample).  Every arm but `random` holds bf16 values in q, k, v, so the f16 mode's
    conversion to bf16 in the backward is exact (`exact_bf16` of bars)."""
    T = _table(n, seed, shared, shared_seed, 4 * HD)
    q, k, v, dctx = (T[:, i * HD:(i + 1) * HD].clone() for i in range(4))
    pos = torch.arange(n, dtype=F64)
    if arm == "random":
        q, k, v = 0.7 * q, 0.7 * k, 0.7 * v
    elif arm == "negative":      # every score about -20: a key that should be masked and scores 0 takes the whole row
        q, k = 0.5 * q, 0.5 * k
        q[:, 0], k[:, 0] = 4.0 * sign, -40.0 * sign      # sign: alternated from sample to sample of a ragged batch, a neighbour's key then scores +20
    elif arm == "match":         # +-1 codes: score 16 at j = pi(i), N(0, 2^2) elsewhere
        code = torch.where(T[:, HD:2 * HD] >= 0, 1.0, -1.0).to(F64)
        k, q = code, 2.0 * code[match_target(n, seed, causal)]
    elif arm == "forbidden":     # score = 2 (j - i) exactly: every masked pair scores above every allowed one
        hi, lo = torch.div(pos, 16, rounding_mode="floor"), torch.remainder(pos, 16)
        q, k = torch.zeros(n, HD, dtype=F64), torch.zeros(n, HD, dtype=F64)
        q[:, 0], q[:, 1], q[:, 2], q[:, 3] = -256.0 * hi, -16.0 * lo, 16.0, 16.0
        k[:, 0], k[:, 1], k[:, 2], k[:, 3] = 1.0, 1.0, 16.0 * hi, lo
    elif arm == "staircase":     # score = g_i * (32-key tile of j): steps just below / above ATTN_DEFER_THR, rising and falling, mixed inside a wave's 32 rows
        lo_, hi_ = 5.4375, 5.65625      # bf16 values on either side of 8 ln 2 = 5.545
        blk, i = torch.div(pos, 32, rounding_mode="floor") % 4, pos.long()
        cyc = torch.tensor([lo_, hi_, -lo_, -hi_], dtype=F64)
        g = torch.where(blk == 0, torch.full_like(pos, lo_), torch.where(blk == 1, torch.where(pos % 2 == 0, lo_, hi_).to(F64),
                        torch.where(blk == 2, torch.full_like(pos, hi_), cyc[i % 4])))
        q, k = 0.25 * q, 0.25 * k
        q[:, 0], k[:, 0] = g, 8.0 * torch.div(pos, 32, rounding_mode="floor")
    else:
        raise ValueError(arm)
    if arm != "random":
        q, k, v = (rt(x, torch.bfloat16) for x in (q, k, v))
    return dict(q=rt(q, td), k=rt(k, td), v=rt(v, td), dctx=rt(dctx, grad_type(td)))


def is_bf16(*xs):
    return all(bool((rt(x, torch.bfloat16) == x).all()) for x in xs)


# ---- batches: [rows, 3 H 64] / [rows, H 64] matrices from slices ---------------------------------------------------------------------------------------------------
def pack(slices, rows, M, H):
    """slices[b][h] = make(...) of sample b; rows[b] = the global rows of its positions -> qkv [M, 3 H 64], dctx [M, H 64] (f64)."""
    qkv, dctx = torch.zeros(M, 3 * H * HD, dtype=F64), torch.zeros(M, H * HD, dtype=F64)
    for b, per_head in enumerate(slices):
        r = torch.as_tensor(rows[b])
        for h, sl in enumerate(per_head):
            for w, name in enumerate(("q", "k", "v")):
                qkv[r, (w * H + h) * HD:(w * H + h + 1) * HD] = sl[name]
            dctx[r, h * HD:(h + 1) * HD] = sl["dctx"]
    return qkv, dctx


# ---- the last block's attention from the residual stream (attn_stream.hip) ----------------------------------------------------------------------------------------
def spool_case(arm, B, L, H, td, seed=0):
    """Operands of lpi_spool_attn_fwd / _bwd as stored (x fp16, W and q in td, dctx bf16, the rest f32) -> dict.  `random`: the data of the kernel's existing test.
    `negative`: column 0 of x is an outlier in every row and W_k sends it against the (common) query direction, so every real row scores about -20 below a row
    of zeros — shaped through x and W_k, because the scores exist nowhere as an operand."""
    d = H * HD
    g = torch.Generator().manual_seed(1000 * B + L + seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    x = rn(B * L, d) * 1.3 + 0.4 * rn(B * L, 1)
    gamma, beta = 1.0 + 0.1 * rn(d), 0.05 * rn(d)
    W, bq = rn(3 * d, d) * d ** -0.5, 0.02 * rn(3 * d)
    q, dctx = rn(B, d), rn(B, d)
    if arm == "negative":
        u = rn(d)
        q = u[None, :] * (1.0 + 0.25 * torch.rand(B, 1, generator=g, dtype=F64))
        x[:, 0] = 40.0
        W[d:2 * d, 0] = -0.24 * u
    elif arm != "random":
        raise ValueError(arm)
    x = rt(x, torch.float16)
    mean, rstd = x.mean(1), 1.0 / (x.var(1, unbiased=False) + 1e-5).sqrt()
    return dict(B=B, L=L, H=H, x=x, gamma=rt(gamma, torch.float32), beta=rt(beta, torch.float32), W=rt(W, td), bq=rt(bq, torch.float32), q=rt(q, td),
                dctx=rt(dctx, torch.bfloat16), mean=rt(mean, torch.float32), rstd=rt(rstd, torch.float32))


def spool_reference(c, td):
    """f64 ctx, dq, dh of a spool_case (LayerNorm from the f32 statistics the kernel is given) and the per-element bar of ctx.  Counted in attn_stream.hip:
      qt = W_k^T q / 8 by MFMA on the stored operands, f32 out (headw_t_kernel): 64 f32 roundings of sum_c |W_k[c, j] q_c| / 8 =: aqt_j
      g = fp16(gamma o qt) (the gamma o vector image): 2^-11 of every term of a score; the score r (x . g - mu cg) in f32 over d terms
          es_l = 2^-11 sum_j |xhat_lj - xbar_j| |gamma_j qt_j| + 2^-24 (d + 72) (X_l + r_l |mu_l| G),  X_l = sum_j |xhat_lj gamma_j| aqt_j,  G = sum_j |gamma_j| aqt_j
          (xbar = sum_l p_l xhat_l: what all rows' scores have in common drops out of the softmax; the rounding of g is relative to |gamma qt|, not to aqt)
      p = __expf(S - lse): a normalised p_l carries ep_l = es_l + sum_m p_m es_m + 2^-22 (2 + |s_l - max s|)
      w = fp16(p r) (the weights table WT): 2^-11, and 2^-25 absolute below fp16's normal range
      hbar = gamma o (sum_l w_l x_l - zmu) + beta, f32 over L rows; hbar -> T into the A fragments and ctx -> T (headw_n_kernel): 2 u each, f32 over d terms."""
    B, L, H = c["B"], c["L"], c["H"]
    d, u = H * HD, U[td]
    mu, r = c["mean"], c["rstd"]
    xh = (c["x"] - mu[:, None]) * r[:, None]
    hln = (xh * c["gamma"] + c["beta"]).requires_grad_(True)
    qr = c["q"].clone().requires_grad_(True)
    W, bq, ga = c["W"], c["bq"], c["gamma"].abs()
    k, v = (hln @ W[d:2 * d].t() + bq[d:2 * d]).view(B, L, H, HD), (hln @ W[2 * d:].t() + bq[2 * d:]).view(B, L, H, HD)
    s = torch.einsum("bhc,blhc->bhl", qr.view(B, H, HD), k) / 8.0
    P = torch.softmax(s, -1)
    ctx = torch.einsum("bhl,blhc->bhc", P, v).reshape(B, d)
    (ctx * c["dctx"]).sum().backward()
    bar, dq_bar1 = torch.zeros(B, d, dtype=F64), torch.zeros(B, d, dtype=F64)
    with torch.no_grad():
        for b in range(B):
            rows = slice(b * L, (b + 1) * L)
            xa, rb, mb = xh[rows].abs(), r[rows], mu[rows].abs()
            for h in range(H):
                Wk, Wv, qh = W[d + h * HD:d + (h + 1) * HD], W[2 * d + h * HD:2 * d + (h + 1) * HD], c["q"][b, h * HD:(h + 1) * HD]
                aqt, qt = Wk.abs().t() @ qh.abs() / 8.0, (Wk.t() @ qh / 8.0).abs()
                p, sl = P[b, h], s[b, h]
                xc = (xh[rows] - p @ xh[rows]).abs()      # a score error common to all rows drops out of the softmax: rows centred on their p-weighted mean
                X, G = (xa * ga) @ aqt, float((ga * aqt).sum())
                es = 2.0 ** -11 * ((xc * ga) @ qt) + E32 * (d + 72) * (X + rb * mb * G)
                ep = es + float((p * es).sum()) + 2.0 ** -22 * (2.0 + (sl - sl.max()).abs())
                hbar = p @ hln[rows]
                # the errors of the normalised p sum to zero (centred rows again); the fp16 rounding of each weight does not (plain rows)
                Eh = ga * ((p * ep) @ xc + (p * 2.0 ** -11 + 2.0 ** -25 / rb) @ xa) + E32 * (L + 8) * ga * (p @ (xa + (rb * mb)[:, None]))
                if L == 1:      # one key: p = 1, dq = 0 exactly.  The backward recomputes the score in another order than the forward's lse: |1 - p| <= twice the f32 part
                    # of es (+ __expf), ds = p (1 - p) dp, dq = W_k (ds hln) / 8 through two bf16 roundings (dqt, dq: 1.02)
                    dp = float(c["dctx"][b, h * HD:(h + 1) * HD] @ (Wv @ hln[rows][0]))
                    dq_bar1[b, h * HD:(h + 1) * HD] = 1.02 * float(2.0 * E32 * (d + 72) * (X + rb * mb * G)[0] + 2.0 ** -22) * abs(dp) * (Wk.abs() @ hln[rows][0].abs()) / 8.0 + FLOOR
                bar[b, h * HD:(h + 1) * HD] = Wv.abs() @ (Eh + 2.0 * u * hbar.abs()) + E32 * (d + 8) * (Wv.abs() @ hbar.abs()) + 2.0 * u * ctx[b, h * HD:(h + 1) * HD].abs() + FLOOR
    return dict(ctx=ctx.detach(), dq=qr.grad, dh=hln.grad, ctx_bar=bar, dq_bar1=dq_bar1)


def spool_emulate(c, td):
    """An honest forward, f64 with the counted roundings: g -> fp16, w = p r -> fp16, hbar -> td, ctx -> td."""
    B, L, H = c["B"], c["L"], c["H"]
    d = H * HD
    out = torch.zeros(B, d, dtype=F64)
    for b in range(B):
        rows = slice(b * L, (b + 1) * L)
        x, mu, r = c["x"][rows], c["mean"][rows], c["rstd"][rows]
        for h in range(H):
            Wk, Wv, qh = c["W"][d + h * HD:d + (h + 1) * HD], c["W"][2 * d + h * HD:2 * d + (h + 1) * HD], c["q"][b, h * HD:(h + 1) * HD]
            g = rt(c["gamma"] * (Wk.t() @ qh / 8.0), torch.float16)
            w = rt(torch.softmax(r * (x @ g - mu * g.sum()), -1) * r, torch.float16)
            hbar = c["gamma"] * (w @ x - (w * mu).sum()) + c["beta"]
            out[b, h * HD:(h + 1) * HD] = rt(Wv @ rt(hbar, td) + c["bq"][2 * d + h * HD:2 * d + (h + 1) * HD], td)
    return out


def spool_with_phantom(c):
    """The MUTANT: every sample reads one row more — zeros, with statistics (0, 1) — as if a padded row of the 32-row tile kept a weight."""
    B, L, d = c["B"], c["L"], c["x"].shape[1]
    x, mean, rstd = torch.zeros(B, L + 1, d, dtype=F64), torch.zeros(B, L + 1, dtype=F64), torch.ones(B, L + 1, dtype=F64)
    x[:, :L], mean[:, :L], rstd[:, :L] = c["x"].view(B, L, d), c["mean"].view(B, L), c["rstd"].view(B, L)
    return dict(c, L=L + 1, x=x.reshape(-1, d), mean=mean.reshape(-1), rstd=rstd.reshape(-1))
