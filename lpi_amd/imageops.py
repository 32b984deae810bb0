"""pixel_format='decoded': the crop / bilinear resize / centre crop / flip of the data transforms on the GPU (lpi_image_resample_u8, csrc/imageops.hip).

A DecodedBatch (lpi_amd.retrieval.utils.data) holds B decoded HWC uint8 images of their original sizes and a [B, 9] descriptor table; the kernel turns
them into the [B,3,S,S] uint8 CHW batch pixel_format='u8' delivers, byte for byte (Pillow 12's fixed-point bilinear resample).  Every image consumer
goes through resample_decoded; lpi_amd.pipeline.BatchPipeline uses the pieces below with its own ring slots.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib

DESC = 12       # int64 fields of one image's kernel descriptor (include/lpi_hip.h LPI_RESAMPLE_DESC)


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


def workspace_bytes(desc, size):
    """Device workspace lpi_image_resample_u8 needs for the host descriptor table `desc` (LpiError on an invalid descriptor)."""
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    out = ctypes.c_long(0)
    rc = _lib.load().lpi_image_resample_workspace(int(desc.shape[0]), int(size), desc.ctypes.data, ctypes.addressof(out))
    if rc != 0:
        raise _lib.LpiError(f"lpi_image_resample_workspace failed with code {rc} (invalid descriptor)")
    return int(out.value)


def launch(desc, src, src_bytes, ws, ws_bytes, out, size, stream):
    """lpi_image_resample_u8 on `stream` (a torch.cuda.Stream): out[:B] from the packed sources src (device uint8) and the host descriptor table desc
    (pageable numpy: the call validates it and copies it into the workspace itself)."""
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    B = int(desc.shape[0])
    rc = _lib.load().lpi_image_resample_u8(B, int(size), desc.ctypes.data, src.data_ptr(), int(src_bytes), ws.data_ptr(), int(ws_bytes), out.data_ptr(),
                                           stream.cuda_stream)
    if rc != 0:
        raise _lib.LpiError(f"lpi_image_resample_u8 failed with code {rc}" + (" (invalid argument)" if rc == -22 else ""))


def resample_decoded(batch, size=None, device="cuda", stream=None, threads=8):
    """DecodedBatch -> device [B,3,S,S] uint8 (CHW, contiguous): the batch pixel_format='u8' gives for the same images and draws, byte for byte.
    size: S (default: the batch's); stream: a torch.cuda.Stream (default: the device's current one) on which the copies and the kernels are enqueued
    — the result is ready in that stream's order."""
    size = int(batch.size if size is None else size)
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.LpiError("resample_decoded runs on an MI355X (device must be cuda:N)")
    stream = torch.cuda.current_stream(device) if stream is None else stream
    desc, nbytes = descriptors(batch)
    ws_bytes = workspace_bytes(desc, size)          # validates before anything is copied
    total = int(nbytes.sum())
    stage = torch.empty(max(total, 1), dtype=torch.uint8, pin_memory=True)
    gather(batch, stage, nbytes, threads)
    with torch.cuda.stream(stream):
        src = stage.to(device, non_blocking=True)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        out = torch.empty((len(batch.pixels), 3, size, size), dtype=torch.uint8, device=device)
        launch(desc, src, total, ws, ws_bytes, out, size, stream)
    return out
