#!/usr/bin/env python3
"""lpi_jpeg_decode_u8 of two builds of the library in one process, called in turn on the same 256-file baseline batch (640 x 480 q90 4:2:0, the files
of tools/decode_pipeline_bench.py): has a change made the baseline decode slower?  The protocol of profiles/filters_resample_ab.json: warm-up rounds,
then 40 timed calls of each (HIP events around the call: descriptor copy + clear + launches), interleaved round by round; median, p10 / p90 and
minimum; the parent against a second handle of itself (its own file copied, so that the loader maps it again) gives the run-to-run spread.  The
outputs and statuses of the two builds are compared byte for byte.  --progressive: the same protocol with lpi_jpeg_decode_u8_x and
LPI_JPEG_PROGRESSIVE on the 256-file progressive batch of the same pixels (Pillow's 10-scan script).

--layouts: no second build (a parent refuses the flag): this tree's lpi_jpeg_decode_u8_x with LPI_JPEG_LAYOUTS on a 256-file batch of each new
kind (4:4:0, 4:1:1, CMYK at 2x2: tools/decode_pipeline_bench.py layout_file) and on the baseline batch with and without the flag, interleaved round
by round under the same protocol; every status must be 0.  --only NAME[,NAME]: those batches alone (a rocprofv3 --kernel-trace --stats run
of one kind gives its per-kernel split).

usage: python3 tools/jpeg_decode_ab.py --parent PATH/liblpi_hip.so [--progressive] [--out FILE.json]   (the other build is this tree's)
       python3 tools/jpeg_decode_ab.py --layouts [--only 4:4:0] [--out FILE.json]"""
import argparse
import ctypes
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))


def bind(path):
    lib = ctypes.CDLL(path)
    P, L, I = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
    lib.lpi_jpeg_decode_u8.argtypes = [I, P, P, P, L, P, P, L, P, P, L, P]
    lib.lpi_jpeg_decode_u8.restype = I
    lib.lpi_jpeg_decode_workspace.argtypes = [I, P, P, P]
    lib.lpi_jpeg_decode_workspace.restype = I
    lib.lpi_jpeg_decode_u8_x.argtypes = [I, I, P, P, P, L, P, P, L, P, P, L, P]
    lib.lpi_jpeg_decode_u8_x.restype = I
    lib.lpi_jpeg_decode_workspace_x.argtypes = [I, I, P, P, P]
    lib.lpi_jpeg_decode_workspace_x.restype = I
    lib.lpi_version.restype = I
    return lib


def layouts(a):
    """--layouts: the new kinds beside the baseline batch, this tree's library only."""
    from decode_pipeline_bench import LAYOUT_KINDS, layout_file, write_folder
    from lpi_amd import _lib
    dev = torch.device("cuda:0")
    lib = bind(_lib.LIB_PATH)
    with tempfile.TemporaryDirectory() as root:
        write_folder(root, 256, 256, 1)
        base = [open(os.path.join(root, f"im{i}.jpg"), "rb").read() for i in range(256)]
    only = a.only.split(",") if a.only else None
    batches = {"baseline_flags0": (0, base), "baseline_flags4": (4, base)}
    for kind in LAYOUT_KINDS:
        if only is None or kind in only:
            rng = np.random.default_rng(0)
            batches[kind] = (4, [layout_file(rng, kind) for _ in range(256)])
    batches = {k: v for k, v in batches.items() if only is None or k in only}
    out_off = (np.arange(256, dtype=np.int64) * 640 * 480 * 3)
    out = torch.empty(256 * 640 * 480 * 3, dtype=torch.uint8, device=dev)
    status = torch.empty(256, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev)
    prep = {}
    for k, (flags, files) in batches.items():
        host = np.frombuffer(b"".join(files), np.uint8).copy()
        offs = np.concatenate(([0], np.cumsum([len(f) for f in files]))).astype(np.int64)
        v = ctypes.c_long(0)
        assert lib.lpi_jpeg_decode_workspace_x(flags, 256, host.ctypes.data, offs.ctypes.data, ctypes.addressof(v)) == 0, k
        prep[k] = (flags, host, offs, torch.from_numpy(host).to(dev), torch.empty(v.value, dtype=torch.uint8, device=dev))
    times, bad = {k: [] for k in prep}, {}
    for r in range(a.warmup + a.reps):
        for k, (flags, host, offs, src, ws) in prep.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            rc = lib.lpi_jpeg_decode_u8_x(flags, 256, host.ctypes.data, offs.ctypes.data, src.data_ptr(), src.numel(), out_off.ctypes.data, out.data_ptr(),
                                          out.numel(), status.data_ptr(), ws.data_ptr(), ws.numel(), s.cuda_stream)
            e1.record(s)
            e1.synchronize()
            assert rc == 0, (k, rc)
            if r >= a.warmup:
                times[k].append(1e3 * e0.elapsed_time(e1))
            if r == 0:
                bad[k] = int((status != 0).sum())
    rec = {"tool": "tools/jpeg_decode_ab.py --layouts", "batch": "256 files 640 x 480 q90 of each kind", "reps": a.reps, "warmup": a.warmup,
           "version": int(lib.lpi_version()), "statuses_not_ok": bad}
    for k, t in times.items():
        rec[k] = {"median_us": round(float(np.median(t)), 1), "p10_p90_us": [round(float(np.percentile(t, q)), 1) for q in (10, 90)],
                  "min_us": round(float(min(t)), 1), "file_MB": round(prep[k][1].size / 1e6, 2), "workspace_MB": round(prep[k][4].numel() / 1e6, 1)}
    assert not any(bad.values()), bad
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--layouts", action="store_true", help="the new kinds of LPI_JPEG_LAYOUTS beside the baseline batch, this tree's build only")
    ap.add_argument("--only", default=None, help="with --layouts: a comma list of baseline_flags0, baseline_flags4, 4:4:0, 4:1:1, cmyk")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--progressive", action="store_true", help="lpi_jpeg_decode_u8_x with LPI_JPEG_PROGRESSIVE on the progressive batch")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.layouts:
        return finish(layouts(a), a)
    if not a.parent:
        ap.error("--parent is required without --layouts")
    from decode_pipeline_bench import write_folder
    from lpi_amd import _lib
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as root:
        write_folder(root, 256, 256, 1, progressive=a.progressive)
        files = [open(os.path.join(root, f"im{i}.jpg"), "rb").read() for i in range(256)]
        twin = os.path.join(root, "parent_twin.so")
        shutil.copyfile(a.parent, twin)
        libs = {"parent": bind(a.parent), "parent2": bind(twin), "new": bind(_lib.LIB_PATH)}
    host = np.frombuffer(b"".join(files), np.uint8).copy()
    offs = np.concatenate(([0], np.cumsum([len(f) for f in files]))).astype(np.int64)
    out_off = (np.arange(256, dtype=np.int64) * 640 * 480 * 3)
    need = {}
    for k, lib in libs.items():
        v = ctypes.c_long(0)
        workspace = (lib.lpi_jpeg_decode_workspace_x, 1) if a.progressive else (lib.lpi_jpeg_decode_workspace,)
        assert workspace[0](*workspace[1:], 256, host.ctypes.data, offs.ctypes.data, ctypes.addressof(v)) == 0
        need[k] = v.value
    src = torch.from_numpy(host).to(dev)
    ws = torch.empty(max(need.values()), dtype=torch.uint8, device=dev)
    out = torch.empty(256 * 640 * 480 * 3, dtype=torch.uint8, device=dev)
    status = torch.empty(256, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev)
    times = {k: [] for k in libs}
    decode = {k: (lib.lpi_jpeg_decode_u8_x, 1) if a.progressive else (lib.lpi_jpeg_decode_u8,) for k, lib in libs.items()}
    digest = {}
    for r in range(a.warmup + a.reps):
        for k, lib in libs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            rc = decode[k][0](*decode[k][1:], 256, host.ctypes.data, offs.ctypes.data, src.data_ptr(), src.numel(), out_off.ctypes.data, out.data_ptr(),
                              out.numel(), status.data_ptr(), ws.data_ptr(), need[k], s.cuda_stream)
            e1.record(s)
            e1.synchronize()
            assert rc == 0, (k, rc)
            if r >= a.warmup:
                times[k].append(1e3 * e0.elapsed_time(e1))
            if r == 0:
                digest[k] = (out.cpu(), status.tolist())
    rec = {"tool": "tools/jpeg_decode_ab.py", "batch": f"256 {'progressive' if a.progressive else 'baseline'} files 640 x 480 q90 4:2:0", "file_MB": round(host.size / 1e6, 2), "reps": a.reps,
           "warmup": a.warmup, "versions": {k: int(lib.lpi_version()) for k, lib in libs.items()}, "workspace_bytes": need,
           "bits_equal_parent_new": bool(torch.equal(digest["parent"][0], digest["new"][0]) and digest["parent"][1] == digest["new"][1]),
           "statuses_not_ok": int(sum(1 for v in digest["new"][1] if v))}
    for k, t in times.items():
        rec[k] = {"median_us": round(float(np.median(t)), 1), "p10_p90_us": [round(float(np.percentile(t, q)), 1) for q in (10, 90)],
                  "min_us": round(float(min(t)), 1)}
    lo, hi = rec["parent"]["p10_p90_us"]
    rec["new_median_inside_parent_p10_p90"] = bool(lo <= rec["new"]["median_us"] <= hi)
    finish(rec, a)


def finish(rec, a):
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
