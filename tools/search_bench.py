#!/usr/bin/env python3
"""The streamed search (lpi_amd.search: lpi_search_rank / lpi_search_topk, and their bf16 / f16 forms lpi_search_rank_t / lpi_search_topk_t) against the
matrix path (engine.score_matrix + lpi_retrieval_rank / lpi_topk),
ONE process on one GPU, arms interleaved: time (HIP events, median of `--rounds` rounds' medians of `--steps` calls) and the growth of
torch.cuda.max_memory_allocated over one call of each arm, at

  i2t    5 000 queries x 25 000 gallery rows x 512 (COCO's test split, images -> captions, 5 ground truths per row)
  t2i    25 000 x 5 000 x 512 (captions -> images, 1 ground truth per row)
  eval   both directions of the evaluation as SPrompts._evaluate_retrieval runs them (matrix: ONE score_matrix + two rank searches)
  train  123 287 x 616 767 x 512 (COCO's training split): three f32 matrices of it are 912 GB, so the matrix arm does not exist; one call of each
         streamed form, timed once.  --no-large skips it.

The matrix arm of i2t / t2i is what the path does for one direction: score_matrix (the padded GEMM output, its copy and its transpose) + one
lpi_retrieval_rank.  Rows unit-normalised Gaussian; ranks of the two arms are compared (they may differ where two scores lie within rounding: the GEMM
kernels sum K in another order) and the count is recorded.  The bf16 / f16 arms (`operands=`) search copies of the operands cast ONCE, outside the
timed region and before the peak is taken, as a gallery held in that type is; their ranks are compared with the f32 streamed arm's, which is the
baseline their time is read against in the same run (rounding the rows moves scores by up to 2u + u^2, so ranks differ: the count is a description).

    python tools/search_bench.py [--rounds 5] [--steps 5] [--no-large] [--mx8 | --wide | --rerank | --mx4]

writes profiles/search_stream_2byte.json (profiles/search_stream.json is the record of the f32 arms alone, before the 2-byte arms existed).

--mx8: the MX-FP8 arm (`operands="mx8"` on Mx8Rows quantised ONCE, outside the timed region and before the peak is taken, as a gallery held in that
format is) beside the f32 and bf16 streamed arms of the same run, and nothing else: rank and top-10 at i2t / t2i and, unless --no-large, at train.
Against the f32 streamed arm it records the rows whose rank differs and the mean overlap of the top-10 index sets (descriptions: MX rounding moves
scores).  It writes profiles/search_stream_mx8.json and leaves the other two records alone.

--wide: the wide top-k path (csrc/search_wide.hip) at k = 17, 100, 256 on f32, bf16 and MX-FP8 operands, the matrix path (score_matrix + lpi_topk, which
takes any k) at the same k and the narrow streamed top-16, interleaved, at i2t; each streamed arm once at train unless --no-large (the matrix does not
exist there).  Per arm: time, time relative to top-16 and to the matrix path, peak bytes.  It writes profiles/search_stream_wide.json only.

--rerank: the two-stage search (lpi_amd.search.topk_reranked: a coarse MX-FP8 or bf16 top-kc on operands held in that type, then csrc/search_rerank.hip
on the f32 rows) at k = 10 with kc = k, 2 k and 4 k, beside the f32 streamed top-10 (narrow) and top-17 (wide) of the same run, which are the parent's
unchanged code and the baseline, and the re-rank launch alone on a held candidate list; interleaved at i2t, each arm once at train unless --no-large.
Per arm: time, peak bytes, and the share of rows whose final (idx, val) equals the f32 top-10's bit for bit.  It writes
profiles/search_stream_rerank.json only.

--mx4: the two-stage search with an MX-FP4 coarse pass (coarse="mx4" on Mx4Rows quantised ONCE and held, csrc/search_mx4.hip) at kc = 64, 128 and 256, beside
the f32 streamed top-10 and the MX-FP8 two-stage search at kc = 40 of the same run, which are the parent's unchanged code and the baseline; k = 10,
interleaved at i2t (the record of this mode was taken with --rounds 3 --steps 3), each arm once at train unless --no-large.  Per arm: time, peak bytes
and the share of rows whose final (idx, val) equals the f32 top-10's bit for bit; and the gallery's bytes per type.  It writes
profiles/search_stream_mx4.json only.

An error ends the process: nothing further is started.  Run it under a time limit."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
DEV = "cuda:0"


def _unit(n, E, gen):
    import torch
    x = torch.randn(n, E, device=DEV, generator=gen)
    return x / x.norm(dim=1, keepdim=True)


def _median_rounds(arms, rounds, steps):
    import numpy as np
    import torch
    for fn in arms.values():
        for _ in range(2):
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
    return {k: {"ms": round(float(np.median(v)), 4), "rounds_ms": [round(x, 4) for x in v]} for k, v in ms.items()}


def _peak(fn):
    """Growth of max_memory_allocated over one call, from a state without cached workspaces or results."""
    import torch
    from lpi_amd import search
    search._WS.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def _overlap10(i_a, i_b):
    """Mean over the rows of |top-10 set a & top-10 set b| / 10."""
    return float((i_a[:, :, None] == i_b[:, None, :]).any(2).float().mean())


def _timed_once(fn):
    import torch
    from lpi_amd import search
    search._WS.clear()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return r, e0.elapsed_time(e1), int(torch.cuda.max_memory_allocated() - base)


def _mx8_arms(a, res, img, txt, gt_i, gt_t, gen):
    """--mx8: streamed f32 / bf16 / mx8, rank and top-10, interleaved in this process."""
    import torch
    from lpi_amd import search
    E = img.shape[1]
    for name, q, g, gt in (("i2t_5000x25000", img, txt, gt_i), ("t2i_25000x5000", txt, img, gt_t)):
        q2, g2 = q.bfloat16(), g.bfloat16()                          # cast / quantised once, outside the timed region
        q8, g8 = search.quantize_mx8(q), search.quantize_mx8(g)
        arms = {
            "streamed_rank": lambda q=q, g=g, gt=gt: search.gt_rank(q, g, gt),
            "streamed_rank_bf16": lambda q2=q2, g2=g2, gt=gt: search.gt_rank(q2, g2, gt, operands="bf16"),
            "streamed_rank_mx8": lambda q8=q8, g8=g8, gt=gt: search.gt_rank(q8, g8, gt, operands="mx8"),
            "streamed_top10": lambda q=q, g=g: search.topk(q, g, 10),
            "streamed_top10_bf16": lambda q2=q2, g2=g2: search.topk(q2, g2, 10, operands="bf16"),
            "streamed_top10_mx8": lambda q8=q8, g8=g8: search.topk(q8, g8, 10, operands="mx8"),
        }
        out = _median_rounds(arms, a.rounds, a.steps)
        for k, fn in arms.items():
            out[k]["peak_bytes"] = _peak(fn)
            out[k]["tflops"] = round(2.0 * q.shape[0] * g.shape[0] * E / (out[k]["ms"] * 1e-3) / 1e12, 2)
        rs, is_ = arms["streamed_rank"](), arms["streamed_top10"]()[0]
        for ops in ("bf16", "mx8"):
            out["rank_rows_differing_%s_vs_streamed_f32" % ops] = int((arms["streamed_rank_" + ops]() != rs).sum())
            out["top10_overlap_%s_vs_streamed_f32" % ops] = round(_overlap10(arms["streamed_top10_" + ops]()[0], is_), 4)
        out["rows"] = int(q.shape[0])
        out["gallery_bytes"] = {"f32": g.shape[0] * E * 4, "bf16": g.shape[0] * E * 2, "mx8": g8.nbytes}
        res["shapes"][name] = out
        print(name, json.dumps(out), flush=True)
    if a.no_large:
        return
    nq, ng = 123287, 616767
    del q, g, q2, g2, q8, g8, arms
    torch.cuda.empty_cache()
    q, g = _unit(nq, E, gen), _unit(ng, E, gen)
    gt = (torch.arange(nq, device=DEV, dtype=torch.int32)[:, None] * 5 + torch.arange(5, device=DEV, dtype=torch.int32)[None, :]).contiguous()
    q2, g2 = q.bfloat16(), g.bfloat16()
    q8, g8 = search.quantize_mx8(q), search.quantize_mx8(g)
    out, kept = {}, {}
    for k, fn in (("streamed_rank", lambda: search.gt_rank(q, g, gt)),
                  ("streamed_rank_bf16", lambda: search.gt_rank(q2, g2, gt, operands="bf16")),
                  ("streamed_rank_mx8", lambda: search.gt_rank(q8, g8, gt, operands="mx8")),
                  ("streamed_top10", lambda: search.topk(q, g, 10)),
                  ("streamed_top10_bf16", lambda: search.topk(q2, g2, 10, operands="bf16")),
                  ("streamed_top10_mx8", lambda: search.topk(q8, g8, 10, operands="mx8"))):
        r, ms, peak = _timed_once(fn)
        kept[k] = r if "rank" in k else r[0][:4096].clone()      # the quality figures of the top-10 form on the first 4 096 rows
        out[k] = {"ms": round(ms, 2), "calls_timed": 1, "peak_bytes": peak, "tflops": round(2.0 * nq * ng * E / (ms * 1e-3) / 1e12, 2)}
        del r
        print(k, json.dumps(out[k]), flush=True)
    for ops in ("bf16", "mx8"):
        out["rank_rows_differing_%s_vs_streamed_f32" % ops] = int((kept["streamed_rank_" + ops] != kept["streamed_rank"]).sum())
        out["top10_overlap_%s_vs_streamed_f32_first_4096_rows" % ops] = round(_overlap10(kept["streamed_top10_" + ops], kept["streamed_top10"]), 4)
    out["rows"] = nq
    out["gallery_bytes"] = {"f32": ng * E * 4, "bf16": ng * E * 2, "mx8": g8.nbytes}
    res["shapes"]["train_123287x616767"] = out
    print("train", json.dumps(out), flush=True)


def _wide_arms(a, res, img, txt, gen, matrix_topk, score_matrix):
    """--wide: streamed top-k on the wide path at k = 17, 100, 256 (f32 / bf16 / mx8 operands) against the matrix path (score_matrix + lpi_topk) and
    the narrow streamed top-16, interleaved in this process."""
    import torch
    from lpi_amd import _lib, search
    E = img.shape[1]
    KS = (17, 100, 256)
    q, g = img, txt
    q2, g2 = q.bfloat16(), g.bfloat16()                              # cast / quantised once, outside the timed region
    q8, g8 = search.quantize_mx8(q), search.quantize_mx8(g)
    arms = {"streamed_top16": lambda: search.topk(q, g, 16)}
    for k in KS:
        arms["streamed_top%d" % k] = lambda k=k: search.topk(q, g, k)
        arms["streamed_top%d_bf16" % k] = lambda k=k: search.topk(q2, g2, k, operands="bf16")
        arms["streamed_top%d_mx8" % k] = lambda k=k: search.topk(q8, g8, k, operands="mx8")
        arms["matrix_top%d" % k] = lambda k=k: matrix_topk(score_matrix(q, g)[0], k)
    out = _median_rounds(arms, a.rounds, a.steps)
    for name, fn in arms.items():
        out[name]["peak_bytes"] = _peak(fn)
    for k in KS:
        out["top%d_rows_differing_matrix_vs_streamed" % k] = int((arms["matrix_top%d" % k]()[0] != arms["streamed_top%d" % k]()[0]).any(1).sum())
        for ops in ("", "_bf16", "_mx8"):
            name = "streamed_top%d%s" % (k, ops)
            out[name]["vs_top16"] = round(out[name]["ms"] / out["streamed_top16"]["ms"], 3)
            out[name]["vs_matrix"] = round(out[name]["ms"] / out["matrix_top%d" % k]["ms"], 3)
    out["rows"] = int(q.shape[0])
    out["workspace_bytes"] = dict({"top16": int(_lib.load().lpi_search_workspace(q.shape[0], g.shape[0], 16))},
                                  **{"top%d" % k: int(_lib.load().lpi_search_wide_workspace(q.shape[0], g.shape[0], k)) for k in KS})
    out["score_matrix_bytes"] = q.shape[0] * g.shape[0] * 4
    res["shapes"]["i2t_5000x25000"] = out
    print("i2t_5000x25000", json.dumps(out), flush=True)
    if a.no_large:
        res["shapes"]["train_123287x616767"] = "not measured (--no-large)"
        return
    nq, ng = 123287, 616767
    del q, g, q2, g2, q8, g8, arms
    torch.cuda.empty_cache()
    q, g = _unit(nq, E, gen), _unit(ng, E, gen)
    q2, g2 = q.bfloat16(), g.bfloat16()
    q8, g8 = search.quantize_mx8(q), search.quantize_mx8(g)
    out = {}
    runs = [("streamed_top16", lambda: search.topk(q, g, 16))]
    for k in KS:
        runs += [("streamed_top%d" % k, lambda k=k: search.topk(q, g, k)),
                 ("streamed_top%d_bf16" % k, lambda k=k: search.topk(q2, g2, k, operands="bf16")),
                 ("streamed_top%d_mx8" % k, lambda k=k: search.topk(q8, g8, k, operands="mx8"))]
    for name, fn in runs:
        r, ms, peak = _timed_once(fn)
        del r
        out[name] = {"ms": round(ms, 2), "calls_timed": 1, "peak_bytes": peak, "tflops": round(2.0 * nq * ng * E / (ms * 1e-3) / 1e12, 2)}
        out[name]["vs_top16"] = round(ms / out["streamed_top16"]["ms"], 3)
        print(name, json.dumps(out[name]), flush=True)
    out["rows"] = nq
    out["matrix"] = "not measured: the score matrix would be %d bytes" % (nq * ng * 4)
    out["score_matrix_bytes"] = nq * ng * 4
    res["shapes"]["train_123287x616767"] = out
    print("train", json.dumps(out), flush=True)


def _rerank_arms(a, res, img, txt, gen):
    """--rerank: coarse top-kc (mx8 / bf16, operands held) + the f32 re-rank to k = 10 at kc = k, 2 k, 4 k, against the f32 streamed top-10 / top-17."""
    import torch
    from lpi_amd import search
    E, K = img.shape[1], 10
    KCS = (K, 2 * K, 4 * K)

    def build(q, g):
        held = {"mx8": (search.quantize_mx8(q), search.quantize_mx8(g)), "bf16": (q.bfloat16(), g.bfloat16())}      # once, outside the timed region
        arms = {"streamed_top10": lambda: search.topk(q, g, K), "streamed_top17": lambda: search.topk(q, g, 17)}
        for ops, (cq, cg) in held.items():
            for kc in KCS:
                arms["two_stage_%s_kc%d" % (ops, kc)] = lambda ops=ops, cq=cq, cg=cg, kc=kc: search.topk_reranked(
                    q, g, K, coarse=ops, candidates=kc, coarse_queries=cq, coarse_gallery=cg)
        return held, arms

    def same_rows(r, want):
        return round(float(((r[0] == want[0]) & (r[1].view(torch.int32) == want[1].view(torch.int32))).all(1).float().mean()), 4)

    q, g = img, txt
    held, arms = build(q, g)
    lists = {kc: search.topk(*held["mx8"], kc, operands="mx8")[0] for kc in KCS + (256,)}
    for kc in lists:
        arms["rerank_alone_kc%d" % kc] = lambda kc=kc: search.rerank(q, g, lists[kc], min(kc, K) if kc < 256 else 256)
    out = _median_rounds(arms, a.rounds, a.steps)
    want = arms["streamed_top10"]()
    for name, fn in arms.items():
        out[name]["peak_bytes"] = _peak(fn)
        out[name]["vs_streamed_top10"] = round(out[name]["ms"] / out["streamed_top10"]["ms"], 3)
        if name.startswith("two_stage"):
            out[name]["rows_equal_f32_top10"] = same_rows(fn(), want)
    out["rows"] = int(q.shape[0])
    out["gallery_bytes"] = {"f32": g.shape[0] * E * 4, "bf16": g.shape[0] * E * 2, "mx8": held["mx8"][1].nbytes}
    res["shapes"]["i2t_5000x25000"] = out
    print("i2t_5000x25000", json.dumps(out), flush=True)
    if a.no_large:
        res["shapes"]["train_123287x616767"] = "not measured (--no-large)"
        return
    nq, ng = 123287, 616767
    del q, g, held, arms, lists, want
    torch.cuda.empty_cache()
    q, g = _unit(nq, E, gen), _unit(ng, E, gen)
    held, arms = build(q, g)
    out, want = {}, None
    for name, fn in arms.items():
        r, ms, peak = _timed_once(fn)
        out[name] = {"ms": round(ms, 2), "calls_timed": 1, "peak_bytes": peak}
        if name == "streamed_top10":
            want = r
        out[name]["vs_streamed_top10"] = round(ms / out["streamed_top10"]["ms"], 3)
        if name.startswith("two_stage"):
            out[name]["rows_equal_f32_top10"] = same_rows(r, want)
        del r
        print(name, json.dumps(out[name]), flush=True)
    out["rows"] = nq
    out["gallery_bytes"] = {"f32": ng * E * 4, "bf16": ng * E * 2, "mx8": held["mx8"][1].nbytes}
    res["shapes"]["train_123287x616767"] = out
    print("train", json.dumps(out), flush=True)


def _mx4_arms(a, res, img, txt, gen):
    """--mx4: f32 top-10; MX-FP8 coarse (kc = 40) + f32 re-rank; MX-FP4 coarse (kc = 64, 128, 256) + f32 re-rank.  Coarse operands held."""
    import torch
    from lpi_amd import search
    E, K = img.shape[1], 10

    def build(q, g):
        q8, g8, q4, g4 = search.quantize_mx8(q), search.quantize_mx8(g), search.quantize_mx4(q), search.quantize_mx4(g)      # once, outside the timed region
        arms = {"streamed_top10": lambda: search.topk(q, g, K),
                "two_stage_mx8_kc40": lambda: search.topk_reranked(q, g, K, coarse="mx8", candidates=40, coarse_queries=q8, coarse_gallery=g8)}
        for kc in (64, 128, 256):
            arms["two_stage_mx4_kc%d" % kc] = lambda kc=kc: search.topk_reranked(q, g, K, coarse="mx4", candidates=kc, coarse_queries=q4, coarse_gallery=g4)
        return arms, {"f32": g.shape[0] * E * 4, "bf16": g.shape[0] * E * 2, "mx8": g8.nbytes, "mx4": g4.nbytes}

    def same_rows(r, want):
        return round(float(((r[0] == want[0]) & (r[1].view(torch.int32) == want[1].view(torch.int32))).all(1).float().mean()), 4)

    q, g = img, txt
    arms, gbytes = build(q, g)
    out = _median_rounds(arms, a.rounds, a.steps)
    want = arms["streamed_top10"]()
    for name, fn in arms.items():
        out[name]["peak_bytes"] = _peak(fn)
        out[name]["vs_streamed_top10"] = round(out[name]["ms"] / out["streamed_top10"]["ms"], 3)
        out[name]["rows_equal_f32_top10"] = same_rows(fn(), want)
    out["rows"] = int(q.shape[0])
    out["gallery_bytes"] = gbytes
    res["shapes"]["i2t_5000x25000"] = out
    print("i2t_5000x25000", json.dumps(out), flush=True)
    if a.no_large:
        res["shapes"]["train_123287x616767"] = "not measured (--no-large)"
        return
    nq, ng = 123287, 616767
    del q, g, arms, want
    torch.cuda.empty_cache()
    q, g = _unit(nq, E, gen), _unit(ng, E, gen)
    arms, gbytes = build(q, g)
    out, want = {}, None
    for name, fn in arms.items():
        r, ms, peak = _timed_once(fn)
        out[name] = {"ms": round(ms, 2), "calls_timed": 1, "peak_bytes": peak}
        if name == "streamed_top10":
            want = r
        out[name]["vs_streamed_top10"] = round(ms / out["streamed_top10"]["ms"], 3)
        out[name]["rows_equal_f32_top10"] = same_rows(r, want)
        del r
        print(name, json.dumps(out[name]), flush=True)
    out["rows"] = nq
    out["gallery_bytes"] = gbytes
    res["shapes"]["train_123287x616767"] = out
    print("train", json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-large", action="store_true")
    ap.add_argument("--mx8", action="store_true", help="the f32, bf16 and MX-FP8 streamed arms only -> profiles/search_stream_mx8.json")
    ap.add_argument("--wide", action="store_true", help="the wide top-k arms (k = 17, 100, 256) against the matrix path -> profiles/search_stream_wide.json")
    ap.add_argument("--rerank", action="store_true", help="the two-stage search (coarse mx8 / bf16 + f32 re-rank) against the f32 top-10 -> profiles/search_stream_rerank.json")
    ap.add_argument("--mx4", action="store_true", help="the two-stage search with an MX-FP4 coarse pass against f32 and MX-FP8 -> profiles/search_stream_mx4.json")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(REPO, "profiles", "search_stream_mx4.json" if a.mx4 else "search_stream_rerank.json" if a.rerank else "search_stream_wide.json" if a.wide
                             else "search_stream_mx8.json" if a.mx8 else "search_stream_2byte.json")
    import torch
    from lpi_amd import _lib, search
    from lpi_amd.engine import score_matrix
    gen = torch.Generator(device=DEV).manual_seed(0)
    E = 512
    TWO_BYTE = (("bf16", torch.bfloat16), ("f16", torch.float16))
    img, txt = _unit(5000, E, gen), _unit(25000, E, gen)
    gt_i = (torch.arange(5000, device=DEV, dtype=torch.int32)[:, None] * 5 + torch.arange(5, device=DEV, dtype=torch.int32)[None, :]).contiguous()
    gt_t = (torch.arange(25000, device=DEV, dtype=torch.int32) // 5).view(-1, 1).contiguous()
    txt[gt_i[:, 0].long()] = torch.nn.functional.normalize(img + 0.05 * torch.randn(5000, E, device=DEV, generator=gen), dim=1)      # some signal
    st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731

    def matrix_rank(s, gt):
        r = torch.empty(s.shape[0], dtype=torch.int32, device=DEV)
        _lib.call("lpi_retrieval_rank", s.shape[0], s.shape[1], s, s.shape[1], gt, gt.shape[1], r, st())
        return r

    def matrix_topk(s, k):
        idx = torch.empty(s.shape[0], k, dtype=torch.int32, device=DEV)
        val = torch.empty(s.shape[0], k, dtype=torch.float32, device=DEV)
        _lib.call("lpi_topk", s.shape[0], s.shape[1], k, s, s.shape[1], idx, val, st())
        return idx, val

    res = {"device": torch.cuda.get_device_name(0), "abi": int(_lib.load().lpi_version()), "rounds": a.rounds, "steps": a.steps, "E": E, "shapes": {}}
    if a.mx4:
        _mx4_arms(a, res, img, txt, gen)
    elif a.rerank:
        _rerank_arms(a, res, img, txt, gen)
    elif a.wide:
        _wide_arms(a, res, img, txt, gen, matrix_topk, score_matrix)
    elif a.mx8:
        _mx8_arms(a, res, img, txt, gt_i, gt_t, gen)
    if a.mx4 or a.rerank or a.wide or a.mx8:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print("wrote", a.out)
        return
    for name, q, g, gt in (("i2t_5000x25000", img, txt, gt_i), ("t2i_25000x5000", txt, img, gt_t)):
        arms = {
            "matrix_rank": lambda q=q, g=g, gt=gt: matrix_rank(score_matrix(q, g)[0], gt),
            "streamed_rank": lambda q=q, g=g, gt=gt: search.gt_rank(q, g, gt),
            "matrix_top10": lambda q=q, g=g: matrix_topk(score_matrix(q, g)[0], 10),
            "streamed_top10": lambda q=q, g=g: search.topk(q, g, 10),
        }
        for ops, tdt in TWO_BYTE:
            q2, g2 = q.to(tdt), g.to(tdt)      # cast once, outside the timed region
            arms["streamed_rank_" + ops] = lambda q2=q2, g2=g2, gt=gt, ops=ops: search.gt_rank(q2, g2, gt, operands=ops)
            arms["streamed_top10_" + ops] = lambda q2=q2, g2=g2, ops=ops: search.topk(q2, g2, 10, operands=ops)
        out = _median_rounds(arms, a.rounds, a.steps)
        for k, fn in arms.items():
            out[k]["peak_bytes"] = _peak(fn)
        rm, rs = arms["matrix_rank"](), arms["streamed_rank"]()
        im, _ = arms["matrix_top10"]()
        is_, _ = arms["streamed_top10"]()
        out["rank_rows_differing"] = int((rm != rs).sum())
        out["top10_rows_differing"] = int((im != is_).any(1).sum())
        for ops, _ in TWO_BYTE:
            out["rank_rows_differing_%s_vs_streamed_f32" % ops] = int((arms["streamed_rank_" + ops]() != rs).sum())
            out["top10_rows_differing_%s_vs_streamed_f32" % ops] = int((arms["streamed_top10_" + ops]()[0] != is_).any(1).sum())
        out["rows"] = int(q.shape[0])
        out["workspace_bytes"] = {"rank": int(_lib.load().lpi_search_workspace(q.shape[0], g.shape[0], 0)),
                                  "top10": int(_lib.load().lpi_search_workspace(q.shape[0], g.shape[0], 10))}
        res["shapes"][name] = out
        print(name, json.dumps(out), flush=True)

    def eval_matrix():
        s_i2t, s_t2i = score_matrix(img, txt)
        return matrix_rank(s_i2t, gt_i), matrix_rank(s_t2i, gt_t)

    def eval_streamed():
        return search.gt_rank(img, txt, gt_i), search.gt_rank(txt, img, gt_t)

    arms = {"matrix": eval_matrix, "streamed": eval_streamed}
    out = _median_rounds(arms, a.rounds, a.steps)
    for k, fn in arms.items():
        out[k]["peak_bytes"] = _peak(fn)
    res["shapes"]["eval_both_directions_5000x25000"] = out
    print("eval", json.dumps(out), flush=True)

    if not a.no_large:
        nq, ng = 123287, 616767
        del img, txt
        torch.cuda.empty_cache()
        q, g = _unit(nq, E, gen), _unit(ng, E, gen)
        gt = (torch.arange(nq, device=DEV, dtype=torch.int32)[:, None] * 5 + torch.arange(5, device=DEV, dtype=torch.int32)[None, :]).contiguous()
        out = {"matrix": {"exists": False, "bytes_needed_for_three_f32_matrices": 3 * nq * ng * 4}}
        large = [("streamed_rank", lambda: search.gt_rank(q, g, gt)), ("streamed_top10", lambda: search.topk(q, g, 10))]
        for ops, tdt in TWO_BYTE:
            q2, g2 = q.to(tdt), g.to(tdt)
            large += [("streamed_rank_" + ops, lambda q2=q2, g2=g2, ops=ops: search.gt_rank(q2, g2, gt, operands=ops)),
                      ("streamed_top10_" + ops, lambda q2=q2, g2=g2, ops=ops: search.topk(q2, g2, 10, operands=ops))]
        for k, fn in large:
            search._WS.clear()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn()
            e1.record()
            torch.cuda.synchronize()
            out[k] = {"ms": round(e0.elapsed_time(e1), 2), "calls_timed": 1, "peak_bytes": int(torch.cuda.max_memory_allocated() - base),
                      "tflops": round(2.0 * nq * ng * E / (e0.elapsed_time(e1) * 1e-3) / 1e12, 2)}
            del r
            print(k, json.dumps(out[k]), flush=True)
        out["operand_bytes"] = (nq + ng) * E * 4
        res["shapes"]["train_123287x616767"] = out
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
