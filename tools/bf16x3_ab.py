#!/usr/bin/env python3
"""EngineOptions.gemm_bf16x3 (operand code LPI_F32X3) against the exact f32 path, ONE process on one GPU (boxes differ by several percent: only a
same-process comparison means anything).  The comparator of every figure is the f32 arm of this process, which is the code without the option:

  gemm    HIP-event times of the four block GEMMs at the vision tower's rows (M = pad(batch * 213, 256); N x K = 2304x768, 768x768, 3072x768, 768x3072) with
          the epilogues the f32 forward uses, and of their dgrads; arms LPI_F32 / LPI_F32X3 interleaved, `--rounds` rounds of `--steps` launches, median of
          the rounds' medians; which kernel each arm launched; the error of both arms against the f64 product on a 512-row slice;
  step    the f32 training step (ViT-B/16, `--batch` pairs, depth 3, r 4: BASELINE.json configs[2]) with the option off and on, interleaved the same way;
          max |delta logit|, max |delta feature| and the factor-gradient relative error between the two arms; the step's GEMM time by kernel (bracketing
          events on every GEMM launch, in extra steps that are not timed as steps).

    python tools/bf16x3_ab.py [--batch 256] [--rounds 4] [--steps 10]

writes profiles/bf16x3_ab.json.  An error in either part ends the process: nothing further is started.  Run it under a time limit."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
DEV = "cuda:0"
MODEL = "ViT-B/16"


def _median_rounds(arms, rounds, steps):
    """arms: name -> callable.  Interleaved rounds of `steps` event-timed calls each.  -> name -> (median of the rounds' medians, the rounds' medians) in ms."""
    import numpy as np
    import torch
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
            ev[0].record()
            for i in range(steps):
                fn()
                ev[i + 1].record()
            torch.cuda.synchronize()
            ms[k].append(float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(steps)])))
    return {k: (float(np.median(v)), [round(x, 4) for x in v]) for k, v in ms.items()}


def part_gemm(a):
    import torch
    from lpi_amd import _lib
    from lpi_amd import engine as E
    from lpi_amd._lib import F32, F32X3, call
    d = 768
    M = E._pad(a.batch * 213, 256)      # the vision tower's rows: 1 + 16 prompt + 196 patch tokens per image
    g = torch.Generator(device=DEV).manual_seed(0)
    st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    lib = _lib.load()
    out = {"M": M, "tuning_key_1": int(lib.lpi_get_tuning(1)), "shapes": {}}
    # (name, N, K, epilogue, bias, residual, aux): the forward's four and their dgrads (B = the pre-transposed weight, no bias; d c_proj carries gelu')
    cases = (("in_proj", 3 * d, d, E.EPI_NONE, True, False, False), ("out_proj", d, d, E.EPI_NONE, True, True, False),
             ("c_fc", 4 * d, d, E.EPI_QUICKGELU, True, False, True), ("c_proj", d, 4 * d, E.EPI_NONE, True, True, False),
             ("d_in_proj", d, 3 * d, E.EPI_NONE, False, False, False), ("d_out_proj", d, d, E.EPI_NONE, False, False, False),
             ("d_c_fc", d, 4 * d, E.EPI_NONE, False, False, False), ("d_c_proj", 4 * d, d, E.EPI_DQUICKGELU, False, False, True))
    for name, N, K, epi, has_bias, has_res, has_aux in cases:
        x = torch.randn(M, K, generator=g, device=DEV)
        w = torch.randn(N, K, generator=g, device=DEV) * 0.03
        bias = torch.randn(N, generator=g, device=DEV) if has_bias else None
        r = torch.randn(M, N, generator=g, device=DEV) if has_res else None
        aux = (torch.rand(M, N, generator=g, device=DEV) if epi == E.EPI_DQUICKGELU else torch.zeros(M, N, device=DEV)) if has_aux else None
        c = torch.zeros(M, N, device=DEV)

        def launch(dt):
            call("lpi_gemm_nt", dt, F32, M, N, K, x, K, w, K, c, N, bias, r, N if has_res else 0, epi, aux, N if has_aux else 0, 1.0, st())

        kern, err = {}, {}
        ref = x[:512].double() @ w.double().t()      # error of the bare product on a slice, against f64 of the original operands
        c512 = torch.zeros(512, N, device=DEV)
        for arm, dt in (("f32", F32), ("x3", F32X3)):
            launch(dt)
            kern[arm] = int(lib.lpi_gemm_last_kernel())
            call("lpi_gemm_nt", dt, F32, 512, N, K, x, K, w, K, c512, N, None, None, 0, E.EPI_NONE, None, 0, 1.0, st())
            err[arm] = float((c512.double() - ref).abs().max() / ref.abs().max())
        t = _median_rounds({"f32": lambda: launch(F32), "x3": lambda: launch(F32X3)}, a.rounds, a.steps)
        fl = 2.0 * M * N * K
        out["shapes"][name] = {"N": N, "K": K, "f32_ms": round(t["f32"][0], 4), "x3_ms": round(t["x3"][0], 4), "f32_rounds_ms": t["f32"][1],
                               "x3_rounds_ms": t["x3"][1], "f32_tflops": round(fl / t["f32"][0] / 1e9, 1), "x3_tflops": round(fl / t["x3"][0] / 1e9, 1),
                               "speedup": round(t["f32"][0] / t["x3"][0], 3), "f32_kernel": kern["f32"], "x3_kernel": kern["x3"],
                               "f32_err_over_max_ref": float(f"{err['f32']:.3e}"), "x3_err_over_max_ref": float(f"{err['x3']:.3e}")}
        print(name, json.dumps(out["shapes"][name]), flush=True)
        del x, w, c, r, aux
    f32 = sum(v["f32_ms"] for v in out["shapes"].values())
    x3 = sum(v["x3_ms"] for v in out["shapes"].values())
    out["sum_f32_ms"], out["sum_x3_ms"], out["sum_speedup"] = round(f32, 3), round(x3, 3), round(f32 / x3, 3)
    return out


def part_step(a):
    import numpy as np
    import torch
    from lpi_amd import engine as E
    from lpi_amd import synth
    from lpi_amd.engine import DualEncoder, EngineOptions, PackedIds, trim_token_ids
    from lpi_amd.step import train_step
    cfg = synth.CONFIGS[MODEL]
    img = torch.from_numpy(synth.images(a.batch, cfg.image_resolution)).to(DEV)
    ids = PackedIds(np.ascontiguousarray(trim_token_ids(synth.token_ids(a.batch))), 17).to(DEV)
    sd = synth.clip_state_dict(cfg)
    encs, facs = {}, {}
    for arm, on in (("off", False), ("on", True)):
        encs[arm] = DualEncoder(cfg, sd, dtype="f32", device=DEV, options=EngineOptions(gemm_bf16x3=on))
        facs[arm] = {k: torch.from_numpy(v).to(DEV).requires_grad_(True)
                     for k, v in synth.prompt_factors(9, 16, cfg.vision_width, cfg.transformer_width, r=4).items()}

    def step(arm):
        for p in facs[arm].values():
            p.grad = None
        return train_step(encs[arm], img, ids, facs[arm], 3)

    res = {}
    for arm in encs:
        out = step(arm)
        torch.cuda.synchronize()
        res[arm] = {"img_f": out["img_f"].double().cpu(), "txt_f": out["txt_f"].double().cpu(),
                    "logits": (encs[arm].logit_scale_exp * out["img_f"] @ out["txt_f"].t()).double().cpu(),
                    "grads": {k: facs[arm][k].grad.double().cpu() for k in synth.PROMPT_NAMES}}
    off, on = res["off"], res["on"]
    cos = min(float((on["grads"][k].ravel() @ off["grads"][k].ravel()) / (on["grads"][k].norm() * off["grads"][k].norm())) for k in synth.PROMPT_NAMES)
    rec = {"workload": f"{MODEL}, {a.batch} pairs, depth 3, r 4, packed text with 17 shared positions, f32 mode train_step (BASELINE.json configs[2])",
           "max_abs_logit_delta": float(f"{(on['logits'] - off['logits']).abs().max():.4g}"),
           "max_abs_logit": float(f"{off['logits'].abs().max():.4g}"),
           "max_abs_feature_delta": float(f"{max((on[k] - off[k]).abs().max() for k in ('img_f', 'txt_f')):.4g}"),
           "factor_gradient_max_rel_error": float(f"{max(((on['grads'][k] - off['grads'][k]).abs().max() / off['grads'][k].abs().max()) for k in synth.PROMPT_NAMES):.4g}"),
           "factor_gradient_min_cosine": round(cos, 9),
           "top1_i2t_agreement": round(float((on["logits"].argmax(1) == off["logits"].argmax(1)).float().mean()), 4)}
    t = _median_rounds({"off": lambda: step("off"), "on": lambda: step("on")}, a.rounds, a.steps)
    for arm in ("off", "on"):
        rec[arm] = {"median_ms_per_round": t[arm][1], "median_ms": round(t[arm][0], 3), "pairs_per_s": round(a.batch / (1e-3 * t[arm][0]), 1)}
    rec["speedup_on_over_off"] = round(t["off"][0] / t["on"][0], 4)
    # where the GEMM time of a step goes, by kernel (LPI_GEMM_K_*): three profiled steps per arm, not timed as steps
    names = {0: "128x128", 1: "256x256", 2: "256x256_tail", 3: "256x128", 4: "rows", 5: "mx8", 6: "bf16x3"}
    for arm in ("off", "on"):
        E.GEMM_PROFILE = []
        try:
            for _ in range(3):
                step(arm)
            torch.cuda.synchronize()
            by = {}
            for e0, e1, fl, _, kind in E.GEMM_PROFILE:
                ms, n, f = by.get(kind, (0.0, 0, 0.0))
                by[kind] = (ms + e0.elapsed_time(e1), n + 1, f + fl)
        finally:
            E.GEMM_PROFILE = None
        rec[arm]["gemm_ms_per_step_by_kernel"] = {names[k]: {"ms": round(v[0] / 3, 3), "launches": v[1] // 3, "tflops": round(v[2] / v[0] / 1e9, 1)}
                                                  for k, v in sorted(by.items())}
        rec[arm]["gemm_ms_per_step"] = round(sum(v[0] for v in by.values()) / 3, 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--only", choices=("gemm", "step"))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bf16x3_ab.json"))
    a = ap.parse_args()
    if a.rounds < 4 or a.steps < 10:
        print("note: fewer than 4 rounds of 10 launches: a smoke run, not a measurement", file=sys.stderr)
    import torch
    from lpi_amd import _lib
    result = {"tool": "tools/bf16x3_ab.py", "model": MODEL, "batch": a.batch, "rounds": a.rounds, "steps": a.steps, "device": torch.cuda.get_device_name(0),
              "library_version": int(_lib.load().lpi_version())}
    for name, fn in (("gemm", part_gemm), ("step", part_step)):
        if a.only in (None, name):
            result[name] = fn(a)
            print(name, json.dumps(result[name]), flush=True)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
