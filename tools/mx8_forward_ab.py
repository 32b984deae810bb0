#!/usr/bin/env python3
"""EngineOptions.mx8_forward against the 2-byte forward, one process, one GPU, random non-zero data (synth weights and images, ViT-B/16, 256 pairs):

  rate    the forward-only encode (both towers in lock step + the cosine matrix, as bench.py --fwd-only runs it) in three arms — option off, on with
          mx8_tile256=False (the 128x128 MX kernel everywhere), on (the 256x256 MX kernel where the engine's rule sends it) — interleaved round by
          round in ONE process (boxes differ by several percent: only a same-box comparison means anything);
  gemm    HIP-event times of the four block GEMM shapes alone, bf16 kernel / MX 128x128 (lpi_gemm_nt_mx8) / MX 256x256 (lpi_gemm_nt_mx8_256) with the
          epilogues the engine uses, the three arms interleaved round by round, and the GB/s of the stand-alone quantiser and of LayerNorm -> MX;
  error   the features of the option (and of plain bf16 mode) against the f32 engine on the same inputs, and whether the two MX arms give the same bits.

    python tools/mx8_forward_ab.py [--batch 256] [--rounds 4] [--steps 10]

writes profiles/mx8_tile256_ab.json (profiles/mx8_forward_ab.json is the two-arm record of the run that introduced the option).  Every step is a child process under its own `timeout -k 10`; the first one that fails ends the run."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
DEV = "cuda:0"
MODEL = "ViT-B/16"


def _inputs(batch):
    import torch
    from lpi_amd import synth
    from lpi_amd.engine import PackedIds, trim_token_ids
    import numpy as np
    cfg = synth.CONFIGS[MODEL]
    img = torch.from_numpy(synth.images(batch, cfg.image_resolution)).to(DEV)
    ids = np.ascontiguousarray(trim_token_ids(synth.token_ids(batch)))
    fac = {k: torch.from_numpy(v).to(DEV) for k, v in synth.prompt_factors(9, 16, cfg.vision_width, cfg.transformer_width, r=4).items()}
    return cfg, img, ids, fac, PackedIds


def step_rate(a):
    import numpy as np
    import torch
    from lpi_amd import synth
    from lpi_amd.engine import DualEncoder, EngineOptions
    from lpi_amd.step import forward_loss
    cfg, img, ids, fac, PackedIds = _inputs(a.batch)
    sd = synth.clip_state_dict(cfg)
    pids = PackedIds(ids, 17).to(DEV)
    arms = {"off": EngineOptions(), "on_128": EngineOptions(mx8_forward=True, mx8_tile256=False), "on": EngineOptions(mx8_forward=True)}
    encs = {k: DualEncoder(cfg, sd, dtype="bf16", device=DEV, options=o) for k, o in arms.items()}

    def run(enc, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        ev[0].record()
        for i in range(n):
            with torch.no_grad():
                forward_loss(enc, img, pids, fac, 3)
            ev[i + 1].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]

    for k in arms:
        run(encs[k], 3)
    ms = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k in arms:
            ms[k].append(float(np.median(run(encs[k], a.steps))))
    rec = {k: {"median_ms_per_round": [round(v, 3) for v in ms[k]], "median_ms": round(float(np.median(ms[k])), 3),
               "pairs_per_s": round(a.batch / (1e-3 * float(np.median(ms[k]))), 1)} for k in arms}
    rec["speedup_on_over_off"] = round(rec["off"]["median_ms"] / rec["on"]["median_ms"], 4)
    rec["speedup_on_128_over_off"] = round(rec["off"]["median_ms"] / rec["on_128"]["median_ms"], 4)
    rec["speedup_on_over_on_128"] = round(rec["on_128"]["median_ms"] / rec["on"]["median_ms"], 4)
    rec["workload"] = f"{MODEL}, {a.batch} pairs, depth 3, r 4, packed text with 17 shared positions, forward-only encode + cosine matrix, bf16 mode"
    return rec


def step_gemm(a):
    import numpy as np
    import torch
    from lpi_amd import _lib
    from lpi_amd import engine as E
    from lpi_amd._lib import BF16, F16, MX8, call
    d = 768
    M = E._pad(a.batch * 213, 256)      # the vision tower's rows: 1 + 16 prompt + 196 patch tokens per image
    g = torch.Generator(device=DEV).manual_seed(0)
    st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731

    def timed(fn, n=10):
        for _ in range(3):
            fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        ev[0].record()
        for i in range(n):
            fn()
            ev[i + 1].record()
        torch.cuda.synchronize()
        return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(n)]))

    lib = _lib.load()
    out = {"M": M, "rounds": a.rounds, "launches_per_round": a.steps, "shapes": {}}
    for name, N, K, epi, res, cdt in (("in_proj", 3 * d, d, E.EPI_NONE, False, torch.bfloat16), ("out_proj", d, d, E.EPI_NONE, True, torch.float16),
                                      ("c_fc", 4 * d, d, E.EPI_QUICKGELU, False, torch.bfloat16), ("c_proj", d, 4 * d, E.EPI_NONE, True, torch.float16)):
        x = torch.randn(M, K, generator=g, device=DEV)
        w = torch.randn(N, K, generator=g, device=DEV) * 0.03
        bias = torch.randn(N, generator=g, device=DEV)
        r = torch.randn(M, N, generator=g, device=DEV).half() if res else None
        xb, wb = x.bfloat16(), w.bfloat16()
        c = torch.zeros(M, N, dtype=cdt, device=DEV)
        xq, xs = E.mx8_quantize(x)
        wq, wsc = E.mx8_quantize(w)
        mx_out = name == "c_fc"      # the engine's c_fc writes c_proj's MX operand
        cq = torch.zeros(M, N, dtype=torch.uint8, device=DEV) if mx_out else c
        cs = torch.zeros(M, N // 32, dtype=torch.uint8, device=DEV) if mx_out else None
        cd = MX8 if mx_out else (F16 if cdt == torch.float16 else BF16)

        def mx(entry):
            return lambda: call(entry, cd, M, N, K, xq, K, xs, K // 32, wq, K, wsc, K // 32, cq, N, cs, N // 32 if mx_out else 0, bias, r, N if res else 0,
                                epi, 1.0, st())
        arms = {"bf16": lambda: E.gemm(BF16, xb, wb, c, M, N, K, bias=bias, residual=r, epi=epi), "mx8_128": mx("lpi_gemm_nt_mx8"),
                "mx8_256": mx("lpi_gemm_nt_mx8_256")}
        ms, kinds = {k: [] for k in arms}, {}
        for _ in range(a.rounds):      # the arms interleaved round by round: a drift of the box falls on all three
            for k, fn in arms.items():
                ms[k].append(timed(fn, a.steps))
                kinds[k] = int(lib.lpi_gemm_last_kernel())
        fl = 2.0 * M * N * K
        rec = {"N": N, "K": K, "mx8_output": "mx8" if mx_out else str(cdt).split(".")[-1]}
        for k in arms:
            t = float(np.median(ms[k]))
            rec[k] = {"ms": round(t, 4), "ms_per_round": [round(v, 4) for v in ms[k]], "tflops": round(fl / t / 1e9, 1), "kernel": kinds[k]}
        rec["mx8_256_over_bf16"] = round(rec["bf16"]["ms"] / rec["mx8_256"]["ms"], 3)
        rec["mx8_256_over_mx8_128"] = round(rec["mx8_128"]["ms"] / rec["mx8_256"]["ms"], 3)
        rec["mx8_128_over_bf16"] = round(rec["bf16"]["ms"] / rec["mx8_128"]["ms"], 3)
        out["shapes"][name] = rec
    ctx = torch.randn(M, d, generator=g, device=DEV).bfloat16()
    q, s = E.mx8_quantize(ctx)
    t = timed(lambda: E.mx8_quantize(ctx, q, s))
    out["quantize_bf16"] = {"ms": round(t, 4), "GB_per_s": round(M * d * (2 + 1 + 1 / 32) / t / 1e6, 1)}
    xh = torch.randn(M, d, generator=g, device=DEV).half()
    gam, bet = torch.ones(d, device=DEV), torch.zeros(d, device=DEV)
    t = timed(lambda: call("lpi_layernorm_mx8_fwd", F16, M, d, xh, d, gam, bet, q, d, s, d // 32, None, None, st()))
    out["layernorm_mx8"] = {"ms": round(t, 4), "GB_per_s": round(M * d * (2 + 1 + 1 / 32) / t / 1e6, 1)}
    return out


def step_error(a):
    import numpy as np
    import torch
    from lpi_amd import synth
    from lpi_amd.engine import DualEncoder, EngineOptions
    from lpi_amd.step import forward_loss
    cfg, img, ids, fac, PackedIds = _inputs(a.batch)
    sd = synth.clip_state_dict(cfg)
    feats = {}
    for name, dtype, opts in (("f32", "f32", {}), ("bf16", "bf16", {}), ("mx8", "bf16", {"mx8_forward": True}),
                              ("mx8_128", "bf16", {"mx8_forward": True, "mx8_tile256": False})):
        enc = DualEncoder(cfg, sd, dtype=dtype, device=DEV, options=EngineOptions(**opts))
        with torch.no_grad():
            _, fi, ft, _, _ = forward_loss(enc, img, PackedIds(ids, 17).to(DEV), fac, 3)
        torch.cuda.synchronize()
        feats[name] = (fi.float().cpu().numpy(), ft.float().cpu().numpy())
        del enc
        torch.cuda.empty_cache()
    rec = {}
    for name in ("bf16", "mx8"):
        err = max(float(np.abs(g - r).max()) for g, r in zip(feats[name], feats["f32"]))
        cos = min(float(((g * r).sum(1) / (np.linalg.norm(g, axis=1) * np.linalg.norm(r, axis=1))).min()) for g, r in zip(feats[name], feats["f32"]))
        lg = [feats[n][0] @ feats[n][1].T for n in (name, "f32")]
        rec[name] = {"max_abs_feature_error": float(f"{err:.4g}"), "min_cosine": round(cos, 6), "max_abs_cosine_matrix_error": float(f"{np.abs(lg[0] - lg[1]).max():.4g}"),
                     "top1_i2t_agreement": round(float((lg[0].argmax(1) == lg[1].argmax(1)).mean()), 4)}
    rec["mx8_tile256_same_bits_as_128x128"] = bool(all(np.array_equal(g, r) for g, r in zip(feats["mx8"], feats["mx8_128"])))
    return rec


STEPS = {"rate": (step_rate, 600), "gemm": (step_gemm, 300), "error": (step_error, 600)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--step", choices=sorted(STEPS), help="(internal) run one step in this process and print its JSON record")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mx8_tile256_ab.json"))
    a = ap.parse_args()
    if a.step:
        print("MX8_AB " + json.dumps(STEPS[a.step][0](a)))
        return 0
    result = {"tool": "tools/mx8_forward_ab.py", "model": MODEL, "batch": a.batch}
    for name in ("gemm", "rate", "error"):
        cmd = ["timeout", "-k", "10", str(STEPS[name][1]), sys.executable, os.path.abspath(__file__), "--step", name, "--batch", str(a.batch),
               "--rounds", str(a.rounds), "--steps", str(a.steps)]
        p = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("MX8_AB ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            print(f"step {name} failed with exit status {p.returncode}: nothing further is started", file=sys.stderr)
            return 1
        result[name] = json.loads(lines[-1][len("MX8_AB "):])
        print(name, json.dumps(result[name]), flush=True)
    import torch
    result["device"] = torch.cuda.get_device_name(0)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
