"""The key-walking attention kernels at the head widths behind lpi_attn_hd_fwd / _bwd side by side — 80 (ViT-H/14, csrc/attn_hd.hip), 88 (ViT-g/14,
csrc/attn_hd88.hip) and 104 (ViT-bigG/14, csrc/attn_hd104.hip) — at the models' vision shape: 64 samples x 16 heads, L = 273 (257 tokens + 16 prompts), bf16.
Forward and backward time and algorithmic TFLOP/s of each (a sibling of attn_hd_bench.py, whose buffers, timing and FLOP count it uses).  The arms are
INTERLEAVED round by round on fresh random data; the median over the rounds is reported and the spread (min .. max) beside it.  88 and 104 end the output side
in half a 16-column tile and pad the contraction to 96 / 128: the MFMA work per algorithmic FLOP is 96 / 88 and (112 + 128) / (2 x 104) of a whole-tile width's.

usage: python3 tools/probe/attn_hdx_bench.py [--json OUT] [--rounds 7] [--batch 64]          (LPI_LIB selects a build)
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from attn_hd_bench import flops, one_round  # noqa: E402
from lpi_amd import _lib  # noqa: E402

WIDTHS = (80, 88, 104)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--L", type=int, default=273)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_hdx_bench.py measures on an MI355X: no GPU here, nothing is reported")
    _lib.load()
    B, H, L = a.batch, 16, a.L
    t = {hd: ([], []) for hd in WIDTHS}
    for r in range(a.rounds):
        for hd in WIDTHS:      # interleaved, fresh data every round
            f, b = one_round(B, L, H, hd, 1000 * L + 10 * r + hd, a.repeats)
            t[hd][0].append(f)
            t[hd][1].append(b)
    out = {"lib": os.environ.get("LPI_LIB", "default build"), "dtype": "bf16", "B": B, "H": H, "L": L, "rounds": a.rounds, "repeats": a.repeats}
    print(f"L = {L}, B x H = {B} x {H}, bf16")
    for hd in WIDTHS:
        ff, fb = flops(B, L, H, hd)
        for name, ts, fl in (("fwd", t[hd][0], ff), ("bwd", t[hd][1], fb)):
            med = statistics.median(ts)
            out[f"hd{hd}_{name}"] = {"us_median": med, "us_min": min(ts), "us_max": max(ts), "tflops": fl / med / 1e6}
        f, b = out[f"hd{hd}_fwd"], out[f"hd{hd}_bwd"]
        print(f"  head width {hd}: forward {f['us_median']:.0f} us ({f['us_min']:.0f} .. {f['us_max']:.0f}) = {f['tflops']:.0f} TFLOP/s, "
              f"backward {b['us_median']:.0f} us ({b['us_min']:.0f} .. {b['us_max']:.0f}) = {b['tflops']:.0f} TFLOP/s")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
