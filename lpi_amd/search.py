"""Streamed retrieval search (csrc/search.hip): the k best gallery rows, or the rank of the ground truth, of every query row without the score matrix.

``topk`` and ``gt_rank`` compute the scores ``queries @ gallery.T`` tile by tile on the matrix cores in the f32 mode's arithmetic and consume them from the
accumulators: memory is O(nq * k) instead of O(nq * ng).  A score's bits depend on its two rows only, so a gallery searched chunk by chunk
(``col_base`` / ``into``) gives the result of one call bit for bit.  ``operands="bf16"`` / ``"f16"`` searches 2-byte operands (csrc/search16.hip): a
tensor of that dtype is read in place, a score is the f32 sum in one fixed order of the exact products of the 2-byte values, and every property above
holds.  There is no fall-back: a shape outside the envelope (E a multiple of 16, of 32 for 2-byte operands, <= 1024; 1 <= k <= 16) raises."""
from __future__ import annotations

import torch

from . import _lib

_WS = {}      # device -> workspace tensor (grown on demand, contents do not survive a call)


def _f32_rows(t):
    """f32 with unit inner stride and a 16-byte row stride, as score_matrix casts / contiguises its operands."""
    if t.dim() != 2:
        raise ValueError("expected a [rows, E] tensor")
    if t.dtype != torch.float32 or t.stride(1) != 1 or t.stride(0) % 4 or t.stride(0) < t.shape[1] or t.data_ptr() % 16:
        t = t.float().contiguous()
    return t


_OPERANDS = {"bf16": (_lib.BF16, torch.bfloat16), "f16": (_lib.F16, torch.float16)}


def _operands(operands):
    """None | 'f32' -> None (the f32 entry points); 'bf16' | 'f16' -> (LPI code, torch dtype)."""
    if operands is None or operands == "f32":
        return None
    if not isinstance(operands, str) or operands not in _OPERANDS:
        raise ValueError(f"unknown operands {operands!r} (f32 | bf16 | f16)")
    return _OPERANDS[operands]


def _rows16(t, dtype):
    """`dtype` (2 bytes) with unit inner stride, a 16-byte row stride and a 16-byte aligned base: such a tensor is used in place, anything else is cast
    or made contiguous once."""
    if t.dim() != 2:
        raise ValueError("expected a [rows, E] tensor")
    if t.dtype != dtype or t.stride(1) != 1 or t.stride(0) % 8 or t.stride(0) < t.shape[1] or t.data_ptr() % 16:
        t = t.to(dtype).contiguous()
    return t


def _workspace(dev, nq, ng, k):
    need = int(_lib.load().lpi_search_workspace(nq, ng, k))
    if need <= 0:
        raise _lib.LpiError(f"lpi_search_workspace({nq}, {ng}, {k}) refused the shape")
    ws = _WS.get(dev)
    if ws is None or ws.numel() < need:
        _WS[dev] = None      # drop the old one first: the peak is one workspace, not two
        ws = _WS[dev] = torch.empty(need, dtype=torch.uint8, device=dev)
    return ws


def topk(queries, gallery, k, *, col_base=0, into=None, operands=None):
    """-> (idx int32 [nq, k], val f32 [nq, k]): per query row the k largest scores in the order (value descending, then index descending),
    lpi_topk's.  ``col_base`` is added to the indices.  ``into`` = the (idx, val) of earlier calls over other gallery chunks: the lists are merged in
    place and returned.  ``operands``: None | "f32" (anything not f32 is cast to f32) | "bf16" | "f16" (both operands end in that type; val stays f32)."""
    typed = _operands(operands)
    q, g = (_f32_rows(queries), _f32_rows(gallery)) if typed is None else (_rows16(queries, typed[1]), _rows16(gallery, typed[1]))
    nq, E = q.shape
    ng = g.shape[0]
    if g.shape[1] != E:
        raise ValueError(f"queries have {E} features, the gallery {g.shape[1]}")
    dev = q.device
    if into is None:
        idx = torch.empty(nq, k, dtype=torch.int32, device=dev)
        val = torch.empty(nq, k, dtype=torch.float32, device=dev)
    else:
        idx, val = into
        if (tuple(idx.shape) != (nq, k) or tuple(val.shape) != (nq, k) or idx.dtype != torch.int32 or val.dtype != torch.float32
                or not idx.is_contiguous() or not val.is_contiguous()):
            raise ValueError("into = (idx int32 [nq, k], val f32 [nq, k]), contiguous")
    ws = _workspace(dev, nq, ng, k)
    name, dt = ("lpi_search_topk", ()) if typed is None else ("lpi_search_topk_t", (typed[0],))
    _lib.call(name, *dt, nq, ng, E, q, q.stride(0), g, g.stride(0), int(k), int(col_base), 0 if into is None else 1, idx, val, ws,
              ws.numel(), torch.cuda.current_stream().cuda_stream)
    return idx, val


def gt_rank(queries, gallery, gt, *, operands=None):
    """-> rank int32 [nq]: lpi_retrieval_rank of the score matrix the two feature sets would give, over the ground-truth list ``gt`` int32 [nq] or
    [nq, gt_per_row] (entries < 0 are padding).  ``operands`` as in ``topk``."""
    typed = _operands(operands)
    q, g = (_f32_rows(queries), _f32_rows(gallery)) if typed is None else (_rows16(queries, typed[1]), _rows16(gallery, typed[1]))
    nq, E = q.shape
    ng = g.shape[0]
    if g.shape[1] != E:
        raise ValueError(f"queries have {E} features, the gallery {g.shape[1]}")
    dev = q.device
    gt = torch.as_tensor(gt).to(device=dev, dtype=torch.int32).reshape(nq, -1).contiguous()
    rank = torch.empty(nq, dtype=torch.int32, device=dev)
    ws = _workspace(dev, nq, ng, 0)
    name, dt = ("lpi_search_rank", ()) if typed is None else ("lpi_search_rank_t", (typed[0],))
    _lib.call(name, *dt, nq, ng, E, q, q.stride(0), g, g.stride(0), gt, gt.shape[1], rank, ws, ws.numel(),
              torch.cuda.current_stream().cuda_stream)
    return rank
