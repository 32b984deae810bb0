"""The 80-wide-head attention kernels alone (csrc/attn_hd.hip: csrc/attn_walk.h at head width 80) at ViT-H/14's vision shape — 256 samples x 16 heads, L = 273 (257 tokens + 16 prompts), bf16 —
beside the EXISTING 64-wide family at H x 64 and the same L, in the same process: forward and backward TFLOP/s of each, and the ratio.

At L = 273 the existing entry points run the one-workgroup short kernels (L <= 288; attention.hip / attention4.hip), not attn_long.hip — the same key-walking
family at head width 64 takes 288 < L <= 1024 only.  So a second pair is timed at L = 289, the shortest sequence that reaches attn_long.hip: the two
instantiations of attn_walk.h side by side.  The arms are INTERLEAVED (round by round: hd 80, 64-wide, hd 80, ...), every round on fresh random data, each call
timed by HIP events around a few repeats after a warm-up; the median over the rounds is reported and the spread (min .. max) beside it.

usage: python3 tools/probe/attn_hd_bench.py [--json OUT] [--rounds 7] [--batch 256]          (LPI_LIB selects a build)
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from lpi_amd import _lib  # noqa: E402
from lpi_amd._lib import BF16, call  # noqa: E402

DEV = "cuda:0"


def buffers(B, L, H, hd, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    d = H * hd
    r = lambda *s: torch.randn(*s, device=DEV, generator=g).bfloat16()  # noqa: E731
    return dict(qkv=r(B * L, 3 * d), dctx=r(B * L, d), ctx=torch.zeros(B * L, d, device=DEV, dtype=torch.bfloat16), lse=torch.zeros(B, H, L, device=DEV),
                delta=torch.zeros(B, H, L, device=DEV), dqkv=torch.zeros(B * L, 3 * d, device=DEV, dtype=torch.bfloat16), d=d)


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n      # us


def one_round(B, L, H, hd, seed, n):
    """-> (forward us, backward us) of one arm on fresh data"""
    s = torch.cuda.current_stream().cuda_stream
    b = buffers(B, L, H, hd, seed)
    d = b["d"]
    if hd == 64:
        fwd = lambda: call("lpi_attn_fwd", BF16, B, L, H, b["qkv"], 3 * d, b["ctx"], d, b["lse"], 0, s)  # noqa: E731
        bwd = lambda: call("lpi_attn_bwd", BF16, B, L, H, b["qkv"], 3 * d, b["ctx"], d, b["dctx"], d, b["lse"], b["delta"], b["dqkv"], 3 * d, 0, s)  # noqa: E731
    else:
        fwd = lambda: call("lpi_attn_hd_fwd", BF16, B, L, H, hd, b["qkv"], 3 * d, b["ctx"], d, b["lse"], s)  # noqa: E731
        bwd = lambda: call("lpi_attn_hd_bwd", BF16, B, L, H, hd, b["qkv"], 3 * d, b["ctx"], d, b["dctx"], d, b["lse"], b["delta"], b["dqkv"], 3 * d, s)  # noqa: E731
    return timed(fwd, n), timed(bwd, n)


def flops(B, L, H, hd):
    """algorithmic: forward = Q K^T and P V (2 products of 2 L L hd each per head); backward = 2.5 x that (five products: S, dP, dV, dQ, dK)"""
    fl = 4.0 * L * L * hd * H * B
    return fl, 2.5 * fl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_hd_bench.py measures on an MI355X: no GPU here, nothing is reported")
    _lib.load()
    B, H = a.batch, 16
    out = {"lib": os.environ.get("LPI_LIB", "default build"), "dtype": "bf16", "B": B, "H": H, "rounds": a.rounds, "repeats": a.repeats, "shapes": []}
    for L, what64 in ((273, "short kernels (attention.hip / attention4.hip): what lpi_attn_fwd / _bwd run at L <= 288"),
                      (289, "key-walking family at 64 (attn_long.hip): what lpi_attn_fwd / _bwd run at 288 < L <= 1024")):
        t = {80: ([], []), 64: ([], [])}
        for r in range(a.rounds):
            for hd in (80, 64):      # interleaved, fresh data every round
                f, b = one_round(B, L, H, hd, 1000 * L + 10 * r + (hd == 64), a.repeats)
                t[hd][0].append(f)
                t[hd][1].append(b)
        rec = {"L": L, "family_64": what64}
        for hd in (80, 64):
            ff, fb = flops(B, L, H, hd)
            for name, ts, fl in (("fwd", t[hd][0], ff), ("bwd", t[hd][1], fb)):
                med = statistics.median(ts)
                rec[f"hd{hd}_{name}"] = {"us_median": med, "us_min": min(ts), "us_max": max(ts), "tflops": fl / med / 1e6}
        for name in ("fwd", "bwd"):
            rec[f"ratio_{name}_tflops_hd80_over_64"] = rec[f"hd80_{name}"]["tflops"] / rec[f"hd64_{name}"]["tflops"]
        out["shapes"].append(rec)
        print(f"L = {L}, B x H = {B} x {H}, bf16; 64-wide arm: {what64}")
        for hd in (80, 64):
            f, b = rec[f"hd{hd}_fwd"], rec[f"hd{hd}_bwd"]
            print(f"  head width {hd}: forward {f['us_median']:.0f} us ({f['us_min']:.0f} .. {f['us_max']:.0f}) = {f['tflops']:.0f} TFLOP/s, "
                  f"backward {b['us_median']:.0f} us ({b['us_min']:.0f} .. {b['us_max']:.0f}) = {b['tflops']:.0f} TFLOP/s")
        print(f"  TFLOP/s ratio 80-wide / 64-wide: forward {rec['ratio_fwd_tflops_hd80_over_64']:.2f}, backward {rec['ratio_bwd_tflops_hd80_over_64']:.2f}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
