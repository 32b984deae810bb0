"""pixel_format='decoded': the crop / resize / centre crop / flip of the data transforms on the GPU (lpi_image_resample_u8_f, csrc/imageops.hip), with
Pillow's bilinear (the default), bicubic or box filter.

A DecodedBatch (lpi_amd.retrieval.utils.data) holds B decoded HWC uint8 images of their original sizes and a [B, 9] descriptor table; the kernel turns
them into the [B,3,S,S] uint8 CHW batch pixel_format='u8' delivers, byte for byte (Pillow 12's fixed-point resample with the batch's filter).  Every image consumer
goes through resample_decoded; lpi_amd.pipeline.BatchPipeline uses the pieces below with its own ring slots.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib

DESC = 12       # int64 fields of one image's kernel descriptor (include/lpi_hip.h LPI_RESAMPLE_DESC)
FILTERS = {"bilinear": 2, "bicubic": 3, "box": 4}      # LPI_FILTER_* = Pillow's Image.Resampling values


def filter_code(filter):
    """LPI_FILTER_* of a filter name (ValueError for a name the kernel does not restate: nearest, lanczos, hamming, ...)."""
    try:
        return FILTERS[filter]
    except (KeyError, TypeError):
        raise ValueError(f"filter must be 'bilinear', 'bicubic' or 'box', not {filter!r}") from None


def descriptors(batch):
    """(host [B, 12] int64 descriptor table {src_offset, w, h, x0, y0, x1, y1, rw, rh, ox, oy, flip}, per-image byte counts) of a DecodedBatch whose
    images are packed back to back in that order."""
    B = len(batch.pixels)
    params = np.asarray(batch.params, dtype=np.int64).reshape(B, -1)
    if params.shape[1] != 9:
        raise ValueError(f"a DecodedBatch's descriptor table is [B, 9], not {list(params.shape)}")
    nbytes = np.empty(B, dtype=np.int64)
    desc = np.empty((B, DESC), dtype=np.int64)
    for i, p in enumerate(batch.pixels):
        if p.dtype != torch.uint8 or p.dim() != 3 or p.shape[2] != 3:
            raise ValueError("DecodedBatch pixels must be HWC uint8 tensors with 3 channels")
        desc[i, 1], desc[i, 2] = int(p.shape[1]), int(p.shape[0])
        nbytes[i] = p.numel()
    desc[:, 0] = np.concatenate(([0], np.cumsum(nbytes)[:-1]))
    desc[:, 3:] = params
    return desc, nbytes


def gather(batch, dst, nbytes, threads=8):
    """The batch's pixels packed back to back into the host byte buffer dst (pinned, >= sum(nbytes) bytes) on `threads` threads (lpi_host_gather_v)."""
    rows = [p if p.is_contiguous() else p.contiguous() for p in batch.pixels]
    if any(p.is_cuda for p in rows):
        raise ValueError("DecodedBatch pixels are host tensors (the decoder's output)")
    n = len(rows)
    ptrs = (ctypes.c_void_p * n)(*[p.data_ptr() for p in rows])
    sizes = (ctypes.c_long * n)(*[int(b) for b in nbytes])
    rc = _lib.load().lpi_host_gather_v(dst.data_ptr(), ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(sizes, ctypes.c_void_p), n, int(threads))
    if rc != 0:
        raise _lib.LpiError(f"lpi_host_gather_v failed with code {rc}")


def workspace_bytes(desc, size, filter="bilinear"):
    """Device workspace lpi_image_resample_u8_f needs for the host descriptor table `desc` and the filter (LpiError on an invalid descriptor)."""
    code = filter_code(filter)
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    out = ctypes.c_long(0)
    rc = _lib.load().lpi_image_resample_workspace_f(code, int(desc.shape[0]), int(size), desc.ctypes.data, ctypes.addressof(out))
    if rc != 0:
        raise _lib.LpiError(f"lpi_image_resample_workspace_f failed with code {rc} (invalid descriptor)")
    return int(out.value)


def launch(desc, src, src_bytes, ws, ws_bytes, out, size, stream, filter="bilinear"):
    """lpi_image_resample_u8_f on `stream` (a torch.cuda.Stream): out[:B] from the packed sources src (device uint8) and the host descriptor table desc
    (pageable numpy: the call validates it and copies it into the workspace itself).  ws_bytes: workspace_bytes of the SAME filter."""
    code = filter_code(filter)
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    B = int(desc.shape[0])
    rc = _lib.load().lpi_image_resample_u8_f(code, B, int(size), desc.ctypes.data, src.data_ptr(), int(src_bytes), ws.data_ptr(), int(ws_bytes),
                                             out.data_ptr(), stream.cuda_stream)
    if rc != 0:
        raise _lib.LpiError(f"lpi_image_resample_u8_f failed with code {rc}" + (" (invalid argument)" if rc == -22 else ""))


def _batch_filter(batch, filter):
    """The filter of a resample call: the named one, else the batch's own; checked here, before anything is enqueued."""
    filter = getattr(batch, "filter", "bilinear") if filter is None else filter
    filter_code(filter)
    return filter


def resample_decoded(batch, size=None, device="cuda", stream=None, threads=8, filter=None):
    """DecodedBatch -> device [B,3,S,S] uint8 (CHW, contiguous): the batch pixel_format='u8' gives for the same images and draws, byte for byte.
    size: S (default: the batch's); stream: a torch.cuda.Stream (default: the device's current one) on which the copies and the kernels are enqueued
    — the result is ready in that stream's order; filter: 'bilinear' | 'bicubic' | 'box' (default: the batch's own, 'bilinear' unless its dataset
    said otherwise)."""
    size = int(batch.size if size is None else size)
    filter = _batch_filter(batch, filter)
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.LpiError("resample_decoded runs on an MI355X (device must be cuda:N)")
    stream = torch.cuda.current_stream(device) if stream is None else stream
    desc, nbytes = descriptors(batch)
    ws_bytes = workspace_bytes(desc, size, filter)          # validates before anything is copied
    total = int(nbytes.sum())
    stage = torch.empty(max(total, 1), dtype=torch.uint8, pin_memory=True)
    gather(batch, stage, nbytes, threads)
    with torch.cuda.stream(stream):
        src = stage.to(device, non_blocking=True)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        out = torch.empty((len(batch.pixels), 3, size, size), dtype=torch.uint8, device=device)
        launch(desc, src, total, ws, ws_bytes, out, size, stream, filter)
    return out


# ---------------------------------------------------------------------------------------------- pixel_format='jpeg' (lpi_jpeg_decode_u8, csrc/jpeg.hip)
JPEG_INFO = 8       # int64 fields lpi_jpeg_info fills (include/lpi_hip.h LPI_JPEG_INFO)
JPEG_INFO_X = 10    # ... and lpi_jpeg_info_x (LPI_JPEG_INFO_X: + {parsed as progressive, scans})
JPEG_PROGRESSIVE = 1        # LPI_JPEG_PROGRESSIVE: progressive files with a complete scan script are inside the envelope
JPEG_LAYOUTS = 4            # LPI_JPEG_LAYOUTS: baseline 4:4:0, 4:1:1, 1x4, RGB, CMYK and YCCK files are inside the envelope


def _flags(progressive=False, layouts=False):
    """The flags word of the lpi_jpeg_*_x calls: the public keywords are booleans, everything below them carries this word."""
    return (JPEG_PROGRESSIVE if progressive else 0) | (JPEG_LAYOUTS if layouts else 0)


def _batch_flags(batch):
    return _flags(getattr(batch, "progressive", False), getattr(batch, "layouts", False))


def _u8(data):
    """bytes / numpy / tensor -> a contiguous host uint8 numpy view."""
    if torch.is_tensor(data):
        return data.contiguous().numpy().reshape(-1).view(np.uint8)
    return np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data).reshape(-1).view(np.uint8)


def jpeg_info(data, progressive=False, layouts=False):
    """(gpu, width, height) of one file from its headers (lpi_jpeg_info_x: host only, it never touches the GPU, so forked loader workers may call it):
    gpu = the file is inside lpi_jpeg_decode_u8's envelope or, with progressive=True, inside that of LPI_JPEG_PROGRESSIVE (the parser then walks a
    progressive file to its end), with layouts=True inside that of LPI_JPEG_LAYOUTS (baseline 4:4:0, 4:1:1, 1x4, RGB, CMYK, YCCK).  None when the headers have a structural error; (False, 0, 0) for a file that is not a JPEG.  The envelope is
    decided there and only there."""
    a = _u8(data)
    info = (ctypes.c_long * JPEG_INFO_X)()
    rc = _lib.load().lpi_jpeg_info_x(_flags(progressive, layouts), a.ctypes.data if a.size else None, int(a.size), ctypes.addressof(info))
    if rc != 0:
        return None
    return bool(info[0]), int(info[1]), int(info[2])


def pil_decode(data):
    """Pillow's decode of one file's bytes: np.asarray(Image.open(f).convert("RGB")) as an HWC uint8 tensor — the yardstick and the fallback (files
    outside the envelope, and files whose GPU status is not OK).  Pillow's own exception propagates."""
    import io
    from PIL import Image
    with Image.open(io.BytesIO(_u8(data).tobytes())) as im:
        return torch.from_numpy(np.array(im.convert("RGB"), dtype=np.uint8))


def jpeg_workspace_bytes(host, offsets, progressive=False, layouts=False):
    """Device workspace lpi_jpeg_decode_u8_x needs for the files packed in host (uint8 numpy) at offsets ([n + 1] int64); LpiError when a file is
    outside the envelope (progressive: that of LPI_JPEG_PROGRESSIVE; layouts: that of LPI_JPEG_LAYOUTS) or has a structural error."""
    return _workspace_x(_flags(progressive, layouts), host, offsets)


def _workspace_x(flags, host, offsets):
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    out = ctypes.c_long(0)
    rc = _lib.load().lpi_jpeg_decode_workspace_x(int(flags), int(offsets.size - 1), host.ctypes.data, offsets.ctypes.data,
                                                 ctypes.addressof(out))
    if rc != 0:
        raise _lib.LpiError(f"lpi_jpeg_decode_workspace_x failed with code {rc} (a file outside the envelope or with a broken header)")
    return int(out.value)


def jpeg_launch(host, offsets, src, out_off, out, status, ws, stream, progressive=False, layouts=False):
    """lpi_jpeg_decode_u8_x on `stream`: the files of host / src (its device copy) at offsets into out at out_off (host int64), statuses into status;
    progressive: with LPI_JPEG_PROGRESSIVE, layouts: with LPI_JPEG_LAYOUTS (neither: flags = 0, which is lpi_jpeg_decode_u8)."""
    _launch_x(_flags(progressive, layouts), host, offsets, src, out_off, out, status, ws, stream)


def _launch_x(flags, host, offsets, src, out_off, out, status, ws, stream):
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    out_off = np.ascontiguousarray(out_off, dtype=np.int64)
    rc = _lib.load().lpi_jpeg_decode_u8_x(int(flags), int(offsets.size - 1), host.ctypes.data, offsets.ctypes.data,
                                          src.data_ptr(), int(src.numel()), out_off.ctypes.data, out.data_ptr(), int(out.numel()), status.data_ptr(),
                                          ws.data_ptr(), int(ws.numel()), stream.cuda_stream)
    if rc != 0:
        raise _lib.LpiError(f"lpi_jpeg_decode_u8_x failed with code {rc}" + (" (invalid argument)" if rc == -22 else ""))


class _Decoded:
    """Full-size pixels of an EncodedBatch on the device: `pixels` (uint8, the images packed HWC back to back), per image its (offset, w, h); `status`
    the pinned host copy of the GPU statuses, readable once the event `ready` has completed; `gpu` the batch indices the GPU decoded."""
    __slots__ = ("pixels", "offsets", "wh", "status", "gpu", "keep", "ready")


_SIDE = {}


def _side_stream(device):
    """The stream this module decodes on for callers that did not name one (one per device): waiting for a batch's statuses then waits for that batch
    only, not for the work the caller has queued on its own stream."""
    index = device.index if device.index is not None else torch.cuda.current_device()
    s = _SIDE.get(index)
    if s is None:
        s = _SIDE[index] = torch.cuda.Stream(device=torch.device("cuda", index))
    return s


def _fresh(device):     # the default buffer provider bufs(key, nbytes, 'pinned' | 'device'): a fresh tensor for every request
    return lambda key, n, where: torch.empty(max(int(n), 1), dtype=torch.uint8, **({"pin_memory": True} if where == "pinned" else {"device": device}))


def _issue_decode(batch, device, stream, bufs=None):
    """Enqueues on `stream`: the H2D copy of the batch's file bytes, lpi_jpeg_decode_u8 for its GPU files, the H2D copies of its host-decoded images, the
    D2H copy of the statuses.  bufs: a buffer provider (BatchPipeline's slots); fresh tensors by default."""
    bufs = bufs or _fresh(device)
    B = len(batch)
    wh = np.asarray(batch.wh, dtype=np.int64).reshape(B, 2)
    nbytes = wh[:, 0] * wh[:, 1] * 3
    offs = np.concatenate(([0], np.cumsum(nbytes)))
    total = int(offs[-1])
    gpu = [i for i in range(B) if i not in batch.fallback]
    data = batch.data if batch.data.is_pinned() else batch.data.pin_memory()
    host = data.numpy()
    file_off = np.asarray(batch.offsets, dtype=np.int64)
    d = _Decoded()
    d.wh, d.offsets, d.gpu = wh, offs[:-1], gpu
    d.keep = [data]
    with torch.cuda.stream(stream):
        d.pixels = bufs("pixels", total, "device")[:max(total, 1)]
        status_dev = bufs("status", 4 * max(B, 1), "device")[:4 * max(B, 1)].view(torch.int32)
        d.status = bufs("status_host", 4 * max(B, 1), "pinned")[:4 * max(B, 1)].view(torch.int32)
        if gpu:
            lo, hi = int(file_off[gpu[0]]), int(file_off[gpu[-1] + 1])
            sub_off = np.array([file_off[i] for i in gpu] + [hi], dtype=np.int64) - lo
            sub = host[lo:hi]
            src = bufs("src", hi - lo, "device")[:hi - lo]
            src.copy_(data[lo:hi], non_blocking=True)
            flags = _batch_flags(batch)
            ws_bytes = _workspace_x(flags, sub, sub_off)
            ws = bufs("ws", ws_bytes, "device")[:ws_bytes]
            _launch_x(flags, sub, sub_off, src, d.offsets[gpu], d.pixels, status_dev, ws, stream)
            d.status[:len(gpu)].copy_(status_dev[:len(gpu)], non_blocking=True)
        d.ready = torch.cuda.Event()
        d.ready.record(stream)
        for i, px in batch.fallback.items():
            d.pixels[int(offs[i]):int(offs[i + 1])].copy_(px.reshape(-1), non_blocking=True)
            d.keep.append(px)
    return d


def _redo_failed(batch, d, stream):
    """After the stream has passed the status copy: the files whose GPU status is not OK, decoded by Pillow (its pixels, or its exception) into their
    slots.  Returns how many."""
    bad = [i for k, i in enumerate(d.gpu) if int(d.status[k]) != 0]
    with torch.cuda.stream(stream):
        for i in bad:
            px = pil_decode(batch.file(i))
            w, h = (int(v) for v in d.wh[i])
            if tuple(px.shape) != (h, w, 3):
                raise _lib.LpiError(f"file {i}: Pillow decodes {tuple(px.shape)}, its header says {(h, w, 3)}")
            d.pixels[int(d.offsets[i]):int(d.offsets[i]) + h * w * 3].copy_(px.reshape(-1).pin_memory(), non_blocking=True)
    return len(bad)


def _work_streams(device, stream):
    """(the stream the caller reads the result on, the stream the decode runs on)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.LpiError("pixel_format='jpeg' decodes on an MI355X (device must be cuda:N)")
    stream = torch.cuda.current_stream(device) if stream is None else stream
    return device, stream, _side_stream(device)


def decode_jpeg(batch, device="cuda", stream=None):
    """EncodedBatch -> the full-size decoded images on the device, a list of B [h, w, 3] uint8 tensors (views of one buffer): for every file
    np.asarray(Image.open(f).convert("RGB")), byte for byte.  The decode runs on this module's side stream; the host waits for that batch's statuses
    only, and the result is ready in `stream`'s order (default: the device's current stream)."""
    device, stream, side = _work_streams(device, stream)
    d = _issue_decode(batch, device, side)
    d.ready.synchronize()
    _redo_failed(batch, d, side)
    stream.wait_stream(side)
    d.pixels.record_stream(stream)
    return [d.pixels[int(o):int(o) + int(w) * int(h) * 3].view(int(h), int(w), 3) for o, (w, h) in zip(d.offsets, d.wh)]


def _decode_resample(batch, size, filter, device, stream, bufs):
    """EncodedBatch -> device [B,3,S,S] uint8 on `stream`, buffers from bufs (as _issue_decode's): decode, resample, then the host waits for the
    statuses' copy (the resample may still run); a file whose GPU status is not OK is decoded again by Pillow and the batch resampled again."""
    B = len(batch)
    d = _issue_decode(batch, device, stream, bufs)
    desc = np.empty((B, DESC), dtype=np.int64)          # the resample descriptor table of the images as d.pixels packs them
    desc[:, 0], desc[:, 1:3], desc[:, 3:] = d.offsets, d.wh, np.asarray(batch.params, dtype=np.int64).reshape(B, -1)
    ws_bytes = workspace_bytes(desc, size, filter)
    with torch.cuda.stream(stream):
        ws, out = bufs("resample_ws", ws_bytes, "device"), bufs("out", B * 3 * size * size, "device")
    launch(desc, d.pixels, d.pixels.numel(), ws, ws_bytes, out, size, stream, filter)
    d.ready.synchronize()
    if _redo_failed(batch, d, stream):
        launch(desc, d.pixels, d.pixels.numel(), ws, ws_bytes, out, size, stream, filter)
    return out[:B * 3 * size * size].view(B, 3, size, size)


def resample_encoded(batch, size=None, device="cuda", stream=None, threads=8, filter=None):
    """EncodedBatch -> device [B,3,S,S] uint8 (CHW, contiguous): the batch resample_decoded (and pixel_format='u8') gives for the same images and
    draws, byte for byte.  The GPU decodes the files inside the envelope (lpi_jpeg_decode_u8), the worker already decoded the others (Pillow).  All
    of it runs on this module's side stream (_decode_resample): the host waits for this batch's statuses only, not for the work queued on `stream`;
    the result is ready in `stream`'s order (default: the device's current one).  threads: unused (the bytes arrive packed); filter: as resample_decoded's."""
    size = int(batch.size if size is None else size)
    filter = _batch_filter(batch, filter)
    device, stream, side = _work_streams(device, stream)
    out = _decode_resample(batch, size, filter, device, side, _fresh(device))
    stream.wait_stream(side)
    out.record_stream(stream)
    return out
