#!/usr/bin/env python3
"""EngineOptions.erf_gelu against the default (QuickGELU in the c_fc epilogue), one process per step, one GPU, synthetic non-zero data (ViT-B/16, 256 pairs,
bf16 mode unless --dtype says otherwise):

  rate    the default training step (lpi_amd.step.train_step, depth 3, packed text with 17 shared positions: what bench.py times) and the forward-only
          encode (forward_loss under no_grad), option off and on, interleaved round by round in ONE process (boxes differ by several percent: only a
          same-box comparison means anything);
  kernel  HIP-event times at the vision tower's c_fc shape (54 528 x 3 072 at 256 pairs): lpi_gelu_erf_fwd with and without the saved derivative, in GB/s,
          next to the LayerNorm kernel's rate on the same rows; and c_fc as a plain GEMM against its QuickGELU form, unfolded (LPI_EPI_NONE against
          LPI_EPI_QUICKGELU) and with the LayerNorm fold (LPI_EPI_LN against LPI_EPI_LN_QUICKGELU), each with and without the saved derivative.

    python tools/erf_gelu_ab.py [--batch 256] [--rounds 4] [--steps 10] [--dtype bf16]

writes profiles/erf_gelu_ab.json.  Every step is a child process under its own `timeout -k 10`; the first one that fails ends the run."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
DEV = "cuda:0"
MODEL = "ViT-B/16"


def _timed(fn, n):
    import numpy as np
    import torch
    for _ in range(3):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    ev[0].record()
    for i in range(n):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(n)]))


def step_rate(a):
    import numpy as np
    import torch
    from lpi_amd import _lib, synth
    from lpi_amd.engine import DualEncoder, EngineOptions, PackedIds, trim_token_ids
    from lpi_amd.step import forward_loss, train_step
    cfg = synth.CONFIGS[MODEL]
    sd = synth.clip_state_dict(cfg)
    img = torch.from_numpy(synth.images(a.batch, cfg.image_resolution)).to(DEV)
    pids = PackedIds(np.ascontiguousarray(trim_token_ids(synth.token_ids(a.batch))), 17).to(DEV)
    fac_np = synth.prompt_factors(9, 16, cfg.vision_width, cfg.transformer_width, r=4)
    fac = {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in fac_np.items()}
    encs = {"off": DualEncoder(cfg, sd, dtype=a.dtype, device=DEV, options=EngineOptions()),
            "on": DualEncoder(cfg, sd, dtype=a.dtype, device=DEV, options=EngineOptions(erf_gelu=True))}

    def train(enc):
        for v in fac.values():
            v.grad = None
        train_step(enc, img, pids, fac, 3)

    def fwd(enc):
        with torch.no_grad():
            forward_loss(enc, img, pids, fac, 3)

    rec = {"workload": f"{MODEL}, {a.batch} pairs, depth 3, r 4, packed text with 17 shared positions, {a.dtype} mode", "launches": {}}
    for name, fn in (("train_step", train), ("forward_only", fwd)):
        ms = {k: [] for k in encs}
        for k, enc in encs.items():
            n0 = _lib.launch_count()
            fn(enc)
            torch.cuda.synchronize()
            rec["launches"][f"{name}.{k}"] = _lib.launch_count() - n0
        for _ in range(a.rounds):      # the arms interleaved round by round: a drift of the box falls on both
            for k, enc in encs.items():
                ms[k].append(_timed(lambda: fn(enc), a.steps))
        rec[name] = {k: {"median_ms_per_round": [round(v, 3) for v in ms[k]], "median_ms": round(float(np.median(ms[k])), 3)} for k in encs}
        rec[name]["on_minus_off_ms"] = round(rec[name]["on"]["median_ms"] - rec[name]["off"]["median_ms"], 3)
        rec[name]["on_over_off"] = round(rec[name]["on"]["median_ms"] / rec[name]["off"]["median_ms"], 4)
    return rec


def step_kernel(a):
    import numpy as np
    import torch
    from lpi_amd import _lib
    from lpi_amd import engine as E
    from lpi_amd._lib import BF16, F16, F32, call
    d = 768
    M = E._pad(a.batch * 213, 256)      # the vision tower's rows: 1 + 16 prompt + 196 patch tokens per image
    N = 4 * d
    g = torch.Generator(device=DEV).manual_seed(0)
    st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    lib = _lib.load()
    out = {"rows": M, "cols": N, "rounds": a.rounds, "launches_per_round": a.steps, "activation": {}, "c_fc": {}}
    # the activation kernel rewrites its input, and erfc branches on the argument's range: every timed launch gets the SAME fresh pre-activations (a copy
    # outside the timed interval), each launch between its own pair of events
    def timed_fresh(u, u0, fn, n):
        ts = []
        for i in range(n + 2):
            u.copy_(u0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    for name, tdt, code, acode, adt in (("bf16", torch.bfloat16, BF16, BF16, torch.bfloat16), ("f16", torch.float16, F16, BF16, torch.bfloat16),
                                        ("f32", torch.float32, F32, F32, torch.float32)):
        u0 = (3.0 * torch.randn(M, N, generator=g, device=DEV)).to(tdt)
        u = torch.empty_like(u0)
        aux = torch.empty(M, N, dtype=adt, device=DEV)
        esz, asz = u.element_size(), aux.element_size()
        rec = {}
        for arm, ax, nbytes in (("with_aux", aux, M * N * (2 * esz + asz)), ("no_aux", None, M * N * 2 * esz)):
            ms = [timed_fresh(u, u0, lambda: call("lpi_gelu_erf_fwd", code, acode, M, N, u, N, ax, N if ax is not None else 0, st()), a.steps)
                  for _ in range(a.rounds)]
            t = float(np.median(ms))
            rec[arm] = {"ms": round(t, 4), "ms_per_round": [round(v, 4) for v in ms], "bytes": nbytes, "GB_per_s": round(nbytes / t / 1e6, 1)}
        out["activation"][name] = rec
        del u, u0, aux
    # LayerNorm on the same rows (fp16 stream -> bf16 operand): the rate of a row kernel the step already runs
    xh = torch.randn(M, d, generator=g, device=DEV).half()
    y = torch.empty(M, d, dtype=torch.bfloat16, device=DEV)
    gam, bet = torch.ones(d, device=DEV), torch.zeros(d, device=DEV)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    ms = [_timed(lambda: call("lpi_layernorm_fwd", BF16, F16, M, d, xh, d, gam, bet, y, d, mean, rstd, st()), a.steps) for _ in range(a.rounds)]
    t = float(np.median(ms))
    out["layernorm_fwd"] = {"rows": M, "d": d, "ms": round(t, 4), "bytes": M * d * 4 + M * 8, "GB_per_s": round((M * d * 4 + M * 8) / t / 1e6, 1)}
    stat = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    ms = [_timed(lambda: call("lpi_layernorm_fwd", BF16, F16, M, d, xh, d, None, None, None, 0, stat[0], stat[1], st()), a.steps) for _ in range(a.rounds)]
    t = float(np.median(ms))
    out["layernorm_stats_only"] = {"rows": M, "d": d, "ms": round(t, 4), "bytes": M * d * 2 + M * 8, "GB_per_s": round((M * d * 2 + M * 8) / t / 1e6, 1)}
    # c_fc: plain against QuickGELU
    x = torch.randn(M, d, generator=g, device=DEV)
    w = torch.randn(N, d, generator=g, device=DEV) * 0.03
    bias = torch.randn(N, generator=g, device=DEV)
    c = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    aux = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    xb, wb, xf, wf = x.bfloat16(), w.bfloat16(), x.half(), w.half()
    lnblk = torch.zeros(2 * M + N, device=DEV)
    lnblk[M:2 * M] = 1.0      # mean 0 | rstd 1 | c1 0
    arms = {
        "plain": lambda: E.gemm(BF16, xb, wb, c, M, N, d, bias=bias),
        "quickgelu": lambda: E.gemm(BF16, xb, wb, c, M, N, d, bias=bias, epi=E.EPI_QUICKGELU),
        "quickgelu_aux": lambda: E.gemm(BF16, xb, wb, c, M, N, d, bias=bias, epi=E.EPI_QUICKGELU, aux=aux),
        "ln": lambda: E.gemm(F16, xf, wf, c, M, N, d, bias=bias, residual=lnblk, ldr=M, epi=E.EPI_LN),
        "ln_quickgelu": lambda: E.gemm(F16, xf, wf, c, M, N, d, bias=bias, residual=lnblk, ldr=M, epi=E.EPI_LN_QUICKGELU),
        "ln_quickgelu_aux": lambda: E.gemm(F16, xf, wf, c, M, N, d, bias=bias, residual=lnblk, ldr=M, epi=E.EPI_LN_QUICKGELU, aux=aux),
    }
    ms, kinds = {k: [] for k in arms}, {}
    for _ in range(a.rounds):
        for k, fn in arms.items():
            ms[k].append(_timed(fn, a.steps))
            kinds[k] = int(lib.lpi_gemm_last_kernel())
    for k in arms:
        t = float(np.median(ms[k]))
        out["c_fc"][k] = {"ms": round(t, 4), "ms_per_round": [round(v, 4) for v in ms[k]], "tflops": round(2.0 * M * N * d / t / 1e9, 1), "kernel": kinds[k]}
    act = out["activation"]["bf16"]
    out["c_fc"]["training_forward_ms"] = {"default": out["c_fc"]["ln_quickgelu_aux"]["ms"], "erf_gelu": round(out["c_fc"]["ln"]["ms"] + act["with_aux"]["ms"], 4)}
    out["c_fc"]["no_grad_forward_ms"] = {"default": out["c_fc"]["ln_quickgelu"]["ms"], "erf_gelu": round(out["c_fc"]["ln"]["ms"] + act["no_aux"]["ms"], 4)}
    return out


STEPS = {"rate": (step_rate, 420), "kernel": (step_kernel, 240)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "f16", "f32"))
    ap.add_argument("--step", choices=sorted(STEPS), help="(internal) run one step in this process and print its JSON record")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "erf_gelu_ab.json"))
    a = ap.parse_args()
    if a.step:
        print("ERF_AB " + json.dumps(STEPS[a.step][0](a)))
        return 0
    result = {"tool": "tools/erf_gelu_ab.py", "model": MODEL, "batch": a.batch, "dtype": a.dtype}
    for name in ("kernel", "rate"):
        cmd = ["timeout", "-k", "10", str(STEPS[name][1]), sys.executable, os.path.abspath(__file__), "--step", name, "--batch", str(a.batch),
               "--rounds", str(a.rounds), "--steps", str(a.steps), "--dtype", a.dtype]
        p = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("ERF_AB ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            print(f"step {name} failed with exit status {p.returncode}: nothing further is started", file=sys.stderr)
            return 1
        result[name] = json.loads(lines[-1][len("ERF_AB "):])
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
