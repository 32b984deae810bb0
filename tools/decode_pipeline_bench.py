#!/usr/bin/env python3
"""pixel_format='u8' against 'decoded' and 'jpeg' on real COCO-format JPEGs (seeded synthetic 640 x 480 q90 images written to a temporary folder,
no restart markers):

  1. host ms per item of the datasets (decode or header walk + transform + hand-over), train (Coco) and eval (CocoEval, Resize(256) +
     CenterCrop(224)), one process;
  2. lpi_image_resample_u8 for a 256-image batch of those items: HIP events around the call (descriptor copy + launches), warm-up, median of 30;
  3. lpi_jpeg_decode_u8 for a 256-image batch of the 'jpeg' items: the file bytes already on the device, output at full size, HIP events around the
     call (descriptor copy + clear + launches), warm-up, median of 30; the GPU statuses, and the files outside the envelope (host fallbacks);
  4. the plugin loop (SPrompts.train_epoch, ViT-B/16 bf16, 256 pairs, BatchPipeline) over the folder: pairs/s with num_workers 0 / 8 / 14, in steady
     state: the untimed warm-up is longer than the DataLoader's prefetch queue (prefetch_factor 2 x workers batches), so the timed steps wait for
     batches the workers make while they are timed.

The decode's phases (per-kernel times): rocprofv3 --kernel-trace --stats -- python3 tools/decode_pipeline_bench.py --decode-only

--progressive: the same seeded pixels saved with progressive=True in a second folder.  Reports the host ms per item of 'jpeg' with jpeg_progressive
(the parser walks the whole file) beside the baseline folder's, lpi_jpeg_decode_u8_x on one 256-file progressive batch beside the baseline batch's
time from the same process, and the plugin loop's pairs/s of 'jpeg' with the key on, with the key off (Pillow decodes every file in the loader) and of
'u8'.  With --decode-only: the two decode timings only.

--layouts: a seeded folder that mixes the kinds LPI_JPEG_LAYOUTS adds (4:4:0, 4:1:1 and CMYK at 2x2 in turn, 640 x 480 q90: Pillow's files of the
same MCU with their frame headers rewritten, tests/jpeg_layouts.py).  Reports lpi_jpeg_decode_u8_x with the flag on one 256-file batch of each kind
and of the mix beside the baseline batch's time from the same process, the host ms per item and the plugin loop's pairs/s of 'jpeg' with
jpeg_layouts on, off (Pillow decodes every file in the loader) and of 'u8'.  With --decode-only: the decode timings only.

--filter bilinear | bicubic | box: the resampling filter of every dataset here (host transforms and GPU kernel alike; default bilinear).

usage: python3 tools/decode_pipeline_bench.py [--images 512] [--steps 16] [--workers 0,8,14] [--filter bilinear] [--decode-only] [--progressive | --layouts]
       [--out FILE.json]
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from torch.utils.data import DataLoader  # noqa: E402

from lpi_amd import imageops  # noqa: E402
from lpi_amd.retrieval.utils import data as D  # noqa: E402


def photo(rng, w=640, h=480, mode="RGB"):
    """Smooth-ish content (a JPEG of uniform noise decodes slower than a photo): low-resolution noise upsampled, plus a little grain."""
    from PIL import Image
    ch = len(mode)
    base = rng.integers(0, 256, (30, 40, ch), dtype=np.uint8)
    im = Image.fromarray(base, mode).resize((w, h), Image.BILINEAR)
    a = np.asarray(im).astype(np.int16) + rng.integers(-8, 9, (h, w, ch))
    return Image.fromarray(np.clip(a, 0, 255).astype(np.uint8), mode)


LAYOUT_KINDS = {"4:4:0": ("RGB", (1, 2)), "4:1:1": ("RGB", (4, 1)), "cmyk": ("CMYK", (2, 2))}


def layout_file(rng, kind):
    """One 640 x 480 q90 file of a kind of LAYOUT_KINDS: Pillow's file of the geometry with the same MCU (4:2:2 for 4:4:0, 4:2:0 for 4:1:1), at the
    size that has the MCU grid of 640 x 480, with its frame header rewritten (tests/jpeg_layouts.py says why that is a valid file)."""
    import io
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import jpeg_layouts as L
    mode, hv = LAYOUT_KINDS[kind]
    sh, sv = L.SOURCE[hv]
    buf = io.BytesIO()
    photo(rng, 8 * sh * -(-640 // (8 * hv[0])), 8 * sv * -(-480 // (8 * hv[1])), mode).save(buf, "JPEG", quality=90, subsampling=L.SUBSAMPLING[(sh, sv)])
    return L.reframe(buf.getvalue(), hv, 640, 480)


def write_annotations(root, n_files, n_train, n_val):
    train = [{"image": f"im{i % n_files}.jpg", "caption": f"a photo of a thing number {i}", "category": 11, "image_id": f"coco_{i}"} for i in range(n_train)]
    val = [{"image": f"im{i % n_files}.jpg", "caption": [f"first caption {i}", f"second caption {i}"], "category": 11, "image_id": i} for i in range(n_val)]
    json.dump(train, open(os.path.join(root, "train.json"), "w"))
    json.dump(val, open(os.path.join(root, "val.json"), "w"))


def write_layouts_folder(root, n_files, n_train, n_val, kinds=tuple(LAYOUT_KINDS)):
    """The seeded folder of --layouts: file i is of kind kinds[i % len(kinds)]."""
    rng = np.random.default_rng(0)
    for i in range(n_files):
        with open(os.path.join(root, f"im{i}.jpg"), "wb") as f:
            f.write(layout_file(rng, kinds[i % len(kinds)]))
    write_annotations(root, n_files, n_train, n_val)


def write_folder(root, n_files, n_train, n_val, progressive=False):
    kw = {"progressive": True} if progressive else {}
    rng = np.random.default_rng(0)
    for i in range(n_files):
        photo(rng).save(os.path.join(root, f"im{i}.jpg"), quality=90, **kw)
    write_annotations(root, n_files, n_train, n_val)


def host_ms(ds, n):
    torch.manual_seed(0)
    ds[0]
    t0 = time.perf_counter()
    for i in range(n):
        ds[i % len(ds)]
    return 1e3 * (time.perf_counter() - t0) / n


def kernel_us(ds, dev, reps=30, warm=5):
    torch.manual_seed(0)
    batch = D.collate_decoded([ds[i % len(ds)] for i in range(256)])[0]
    desc, nbytes = imageops.descriptors(batch)
    ws_bytes = imageops.workspace_bytes(desc, batch.size, batch.filter)
    stage = torch.empty(int(nbytes.sum()), dtype=torch.uint8, pin_memory=True)
    imageops.gather(batch, stage, nbytes, 8)
    src = stage.to(dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty((256, 3, batch.size, batch.size), dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev)
    times = []
    for r in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        imageops.launch(desc, src, int(nbytes.sum()), ws, ws_bytes, out, batch.size, s, batch.filter)
        e1.record(s)
        e1.synchronize()
        if r >= warm:
            times.append(1e3 * e0.elapsed_time(e1))
    return {"median_us": round(float(np.median(times)), 1), "p10_p90_us": [round(float(np.percentile(times, q)), 1) for q in (10, 90)],
            "source_MB": round(float(nbytes.sum()) / 1e6, 1), "workspace_MB": round(ws_bytes / 1e6, 2), "filter": batch.filter, "reps": reps,
            "warmup": warm}


def jpeg_decode(ds, root, dev, reps=30, warm=5, progressive=False, layouts=False):
    """lpi_jpeg_decode_u8 (progressive / layouts: lpi_jpeg_decode_u8_x with LPI_JPEG_PROGRESSIVE / LPI_JPEG_LAYOUTS) on one 256-image batch of
    'jpeg' items (bytes on the device, full-size output), and the folder's fallbacks."""
    torch.manual_seed(0)
    batch = D.collate_encoded([ds[i % len(ds)] for i in range(256)])[0]
    gpu = [i for i in range(len(batch)) if i not in batch.fallback]
    lo, hi = int(batch.offsets[gpu[0]]), int(batch.offsets[gpu[-1] + 1])
    host = batch.data.numpy()[lo:hi]
    offs = np.array([int(batch.offsets[i]) for i in gpu] + [hi], dtype=np.int64) - lo
    wh = batch.wh.numpy()[gpu]
    out_off = np.concatenate(([0], np.cumsum(wh[:, 0] * wh[:, 1] * 3)))
    src = torch.from_numpy(host.copy()).to(dev)
    ws_bytes = imageops.jpeg_workspace_bytes(host, offs, progressive, layouts)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(int(out_off[-1]), dtype=torch.uint8, device=dev)
    status = torch.empty(len(gpu), dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev)
    times, host_call = [], []
    for r in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        t0 = time.perf_counter()
        imageops.jpeg_launch(host, offs, src, out_off[:-1], out, status, ws, s, progressive, layouts)
        t1 = time.perf_counter()
        e1.record(s)
        e1.synchronize()
        if r >= warm:
            times.append(1e3 * e0.elapsed_time(e1))
            host_call.append(1e3 * (t1 - t0))
    # the host's share: the parse of every file for the workspace size (once per batch), and the decode call itself until it returns (parse again,
    # descriptor and scan tables built and copied from pageable memory, launches enqueued)
    t0 = time.perf_counter()
    for _ in range(10):
        imageops.jpeg_workspace_bytes(host, offs, progressive, layouts)
    ws_ms = 1e2 * (time.perf_counter() - t0)
    files = sorted(f for f in os.listdir(root) if f.endswith(".jpg"))
    outside = sum(1 for f in files if not (imageops.jpeg_info(open(os.path.join(root, f), "rb").read(), progressive, layouts) or (False,))[0])
    return {"median_us": round(float(np.median(times)), 1), "p10_p90_us": [round(float(np.percentile(times, q)), 1) for q in (10, 90)],
            "host_call_ms_median": round(float(np.median(host_call)), 3), "host_workspace_call_ms": round(ws_ms, 3), "files": len(gpu), "file_MB": round(hi / 1e6 - lo / 1e6, 2), "mean_file_KB": round((hi - lo) / len(gpu) / 1e3, 1),
            "output_MB": round(float(out_off[-1]) / 1e6, 1), "workspace_MB": round(ws_bytes / 1e6, 1), "gpu_status_not_ok": int((status != 0).sum()),
            "batch_fallbacks": len(batch.fallback), "folder_files": len(files), "folder_files_outside_envelope": outside, "reps": reps, "warmup": warm}


def loop_pairs_per_s(root, pf, workers, steps, warm, dev, filter="bilinear", jpeg_progressive=False, jpeg_layouts=False):
    from lpi_amd.retrieval.methods.sprompt import SPrompts
    args = json.load(open(os.path.join(REPO, "lpi_amd", "retrieval", "configs", "lpi", "coco_lpi.json")))
    args.update(device=[dev], compute_dtype="bf16", honor_prompt_depth=True, prompt_depth=3, batch_size=256, epochs=1, num_workers=workers,
                pixel_format=pf)
    m = SPrompts(args)
    m._network.update_fc(0)
    ds = D.Coco(image_root=root, ann_file=os.path.join(root, "train.json"), tasks=[0], pixel_format=pf, interpolation=filter,
                jpeg_progressive=jpeg_progressive, jpeg_layouts=jpeg_layouts)
    collate = D.collate_decoded if pf == "decoded" else (D.collate_encoded if pf == "jpeg" else (D.collate_keep_images if workers == 0 else None))
    loader = DataLoader(ds, batch_size=256, shuffle=False, num_workers=workers, collate_fn=collate, persistent_workers=False)
    opt, _ = m._setup_training()
    t = {}

    def on_step(i, b, o):
        if i == warm - 1:
            torch.cuda.synchronize()
            t[0] = time.perf_counter()
        if i == warm + steps - 1:
            torch.cuda.synchronize()
            t[1] = time.perf_counter()
            return True
        return False
    m.train_epoch(loader, opt, 0, None, on_step)
    del m
    return {"pairs_per_s": round(256 * steps / (t[1] - t[0]), 1), "timed_steps": steps, "warmup_steps": warm,
            "prefetch_queue_batches": 2 * workers if workers else 0}


def progressive_sections(a, rec, dev):
    """--progressive: a baseline and a progressive folder of the same seeded pixels."""
    workers = [int(x) for x in a.workers.split(",")]
    warm = {w: max(a.warmup, 2 * w + 2) for w in workers}
    rec["source"] = "640 x 480 q90 JPEG, progressive=True (Pillow's 10-scan script) beside the baseline files of the same pixels"
    with tempfile.TemporaryDirectory() as base, tempfile.TemporaryDirectory() as prog:
        n_train = 256 * ((0 if a.decode_only else a.steps + max(warm.values())) + 1)
        write_folder(base, a.images, 256, 256)
        write_folder(prog, a.images, n_train, 256, progressive=True)

        def sets(root, **kw):
            return (D.Coco(image_root=root, ann_file=os.path.join(root, "train.json"), tasks=[0], pixel_format="jpeg", interpolation=a.filter, **kw),
                    D.CocoEval(image_root=root, ann_file=os.path.join(root, "val.json"), tasks=[0], pixel_format="jpeg", interpolation=a.filter, **kw))
        b_tr, b_ev = sets(base)
        on_tr, on_ev = sets(prog, jpeg_progressive=True)
        off_tr, off_ev = sets(prog)
        rec["jpeg_decode_256"] = {"baseline_files": jpeg_decode(b_tr, base, dev), "progressive_files": jpeg_decode(on_tr, prog, dev, progressive=True)}
        print(json.dumps({"jpeg_decode_256": rec["jpeg_decode_256"]}), flush=True)
        if not a.decode_only:
            rec["host_ms_per_item"] = {"train_jpeg_baseline_files": round(host_ms(b_tr, a.host_items), 3),
                                       "eval_jpeg_baseline_files": round(host_ms(b_ev, a.host_items), 3),
                                       "train_jpeg_progressive_key_on": round(host_ms(on_tr, a.host_items), 3),
                                       "eval_jpeg_progressive_key_on": round(host_ms(on_ev, a.host_items), 3),
                                       "train_jpeg_progressive_key_off": round(host_ms(off_tr, min(a.host_items, 50)), 3),
                                       "eval_jpeg_progressive_key_off": round(host_ms(off_ev, min(a.host_items, 50)), 3)}
            rec["loop_pairs_per_s"] = {}
            for w in workers:
                for name, pf, key in (("jpeg_key_on", "jpeg", True), ("jpeg_key_off", "jpeg", False), ("u8", "u8", False)):
                    r = loop_pairs_per_s(prog, pf, w, a.steps, warm[w], dev, a.filter, jpeg_progressive=key)
                    rec["loop_pairs_per_s"][f"{name}_workers{w}"] = r
                    print(json.dumps({f"{name}_workers{w}": r}), flush=True)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def layouts_sections(a, rec, dev):
    """--layouts: the baseline folder, one folder per new kind (decode timings) and the folder that mixes them (host times and the loop)."""
    workers = [int(x) for x in a.workers.split(",")]
    warm = {w: max(a.warmup, 2 * w + 2) for w in workers}
    rec["source"] = "640 x 480 q90 JPEG: 4:4:0, 4:1:1 and CMYK 2x2 files in turn (frame headers rewritten) beside baseline 4:2:0 files"
    with tempfile.TemporaryDirectory() as base, tempfile.TemporaryDirectory() as mix:
        n_train = 256 * ((0 if a.decode_only else a.steps + max(warm.values())) + 1)
        write_folder(base, 256, 256, 256)
        write_layouts_folder(mix, a.images, n_train, 256)

        def sets(root, **kw):
            return (D.Coco(image_root=root, ann_file=os.path.join(root, "train.json"), tasks=[0], pixel_format="jpeg", interpolation=a.filter, **kw),
                    D.CocoEval(image_root=root, ann_file=os.path.join(root, "val.json"), tasks=[0], pixel_format="jpeg", interpolation=a.filter, **kw))
        b_tr, b_ev = sets(base)
        on_tr, on_ev = sets(mix, jpeg_layouts=True)
        off_tr, off_ev = sets(mix)
        rec["jpeg_decode_256"] = {"baseline_files": jpeg_decode(b_tr, base, dev), "baseline_files_with_the_flag": jpeg_decode(b_tr, base, dev, layouts=True)}
        for kind in LAYOUT_KINDS:
            with tempfile.TemporaryDirectory() as one:
                write_layouts_folder(one, 256, 256, 1, (kind,))
                rec["jpeg_decode_256"][kind] = jpeg_decode(sets(one, jpeg_layouts=True)[0], one, dev, layouts=True)
        rec["jpeg_decode_256"]["mixed"] = jpeg_decode(on_tr, mix, dev, layouts=True)
        print(json.dumps({"jpeg_decode_256": rec["jpeg_decode_256"]}), flush=True)
        if not a.decode_only:
            rec["host_ms_per_item"] = {"train_jpeg_baseline_files": round(host_ms(b_tr, a.host_items), 3),
                                       "eval_jpeg_baseline_files": round(host_ms(b_ev, a.host_items), 3),
                                       "train_jpeg_layouts_key_on": round(host_ms(on_tr, a.host_items), 3),
                                       "eval_jpeg_layouts_key_on": round(host_ms(on_ev, a.host_items), 3),
                                       "train_jpeg_layouts_key_off": round(host_ms(off_tr, min(a.host_items, 50)), 3),
                                       "eval_jpeg_layouts_key_off": round(host_ms(off_ev, min(a.host_items, 50)), 3)}
            rec["loop_pairs_per_s"] = {}
            for w in workers:
                for name, pf, key in (("jpeg_key_on", "jpeg", True), ("jpeg_key_off", "jpeg", False), ("u8", "u8", False)):
                    r = loop_pairs_per_s(mix, pf, w, a.steps, warm[w], dev, a.filter, jpeg_layouts=key)
                    rec["loop_pairs_per_s"][f"{name}_workers{w}"] = r
                    print(json.dumps({f"{name}_workers{w}": r}), flush=True)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2, help="untimed steps; at least prefetch_factor (2) x workers + 2 whatever this says")
    ap.add_argument("--workers", default="0,8,14")
    ap.add_argument("--host-items", type=int, default=200)
    ap.add_argument("--filter", default="bilinear", choices=list(imageops.FILTERS), help="Pillow resampling filter of the transforms and the kernel")
    ap.add_argument("--decode-only", action="store_true", help="write the folder and run section 3 only (for a rocprofv3 --kernel-trace run)")
    ap.add_argument("--progressive", action="store_true", help="the progressive folder: jpeg_progressive on / off / 'u8' (see above)")
    ap.add_argument("--layouts", action="store_true", help="the folder that mixes 4:4:0, 4:1:1 and CMYK files: jpeg_layouts on / off / 'u8' (see above)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from lpi_amd.synth_bpe import ensure_vocab
    ensure_vocab()
    dev = torch.device("cuda:0")
    rec = {"tool": "tools/decode_pipeline_bench.py", "source": "640 x 480 q90 JPEG", "batch": 256, "host_threads": torch.get_num_threads(),
           "filter": a.filter}
    if a.progressive:
        progressive_sections(a, rec, dev)
        return
    if a.layouts:
        layouts_sections(a, rec, dev)
        return
    with tempfile.TemporaryDirectory() as root:
        workers = [int(x) for x in a.workers.split(",")]
        warm = {w: max(a.warmup, 2 * w + 2) for w in workers}
        write_folder(root, a.images, 256 * (a.steps + max(warm.values()) + 1), 256)
        formats = ("u8", "decoded", "jpeg")
        tr = {pf: D.Coco(image_root=root, ann_file=os.path.join(root, "train.json"), tasks=[0], pixel_format=pf, interpolation=a.filter)
              for pf in formats}
        ev = {pf: D.CocoEval(image_root=root, ann_file=os.path.join(root, "val.json"), tasks=[0], pixel_format=pf, interpolation=a.filter)
              for pf in formats}
        if a.decode_only:
            rec["jpeg_decode_256"] = jpeg_decode(tr["jpeg"], root, dev)
            print(json.dumps(rec))
            return
        rec["host_ms_per_item"] = {f"{form}_{pf}": round(host_ms(ds[pf], a.host_items), 3) for form, ds in (("train", tr), ("eval", ev))
                                   for pf in formats}
        for form in ("train", "eval"):
            u, d = rec["host_ms_per_item"][f"{form}_u8"], rec["host_ms_per_item"][f"{form}_decoded"]
            rec[f"host_saving_{form}"] = round(1.0 - d / u, 3)
            rec[f"host_saving_{form}_jpeg"] = round(1.0 - rec["host_ms_per_item"][f"{form}_jpeg"] / u, 3)
        rec["kernel_256"] = {"train": kernel_us(tr["decoded"], dev), "eval": kernel_us(ev["decoded"], dev)}
        rec["jpeg_decode_256"] = jpeg_decode(tr["jpeg"], root, dev)
        print(json.dumps({"jpeg_decode_256": rec["jpeg_decode_256"]}), flush=True)
        rec["loop_pairs_per_s"] = {}
        for w in workers:
            for pf in formats:
                rec["loop_pairs_per_s"][f"{pf}_workers{w}"] = loop_pairs_per_s(root, pf, w, a.steps, warm[w], dev, a.filter)
                print(json.dumps({f"{pf}_workers{w}": rec["loop_pairs_per_s"][f"{pf}_workers{w}"]}), flush=True)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
