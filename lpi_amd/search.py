"""Streamed retrieval search (csrc/search.hip): the k best gallery rows, or the rank of the ground truth, of every query row without the score matrix.

``topk`` and ``gt_rank`` compute the scores ``queries @ gallery.T`` tile by tile on the matrix cores in the f32 mode's arithmetic and consume them from the
accumulators: memory is O(nq * k) instead of O(nq * ng).  A score's bits depend on its two rows only, so a gallery searched chunk by chunk
(``col_base`` / ``into``) gives the result of one call bit for bit.  ``operands="bf16"`` / ``"f16"`` searches 2-byte operands (csrc/search16.hip): a
tensor of that dtype is read in place, a score is the f32 sum in one fixed order of the exact products of the 2-byte values, and every property above
holds.  ``operands="mx8"`` searches MX-FP8 operands (csrc/search_mx8.hip): e4m3 bytes with one E8M0 scale byte per 32 elements, an ``Mx8Rows`` (what
``quantize_mx8`` returns), one byte per element plus the scales; an ``Mx8Rows`` is read in place, a float tensor is quantised once; a score is the f32
result of the block-scaled instruction chain over E in one fixed order, of the QUANTISED rows, and the properties above hold.  There is no fall-back:
a shape outside the envelope (E a multiple of 16, of 32 for 2-byte operands, of 128 for MX-FP8 and MX-FP4, <= 1024; 1 <= k <= 256) raises.

``operands="mx4"`` searches MX-FP4 operands (csrc/search_mx4.hip): e2m1 nibbles, two per byte, with the same scales, an ``Mx4Rows`` (what
``quantize_mx4`` returns), 0.53 bytes per element.  It is a COARSE type: ``topk`` and the coarse stage of ``topk_reranked`` take it, with every property
above (a score is the block-scaled chain over the quantised rows), but its scores are off by a few 1e-2 on unit rows, so ``gt_rank`` and ``rerank``
refuse it: an MX-FP4 list is a candidate list for ``rerank``, not a result.

``topk`` with k <= 16 keeps a sorted list per row in LDS (the narrow entry points).  17 <= k <= 256 goes to the wide entry points (csrc/search_wide.hip):
the same scores, bit for bit, in one sweep of the gallery; scores that beat a row's current k-th best are appended to a candidate buffer in the
workspace and selected down to k when it fills.  The workspace is ``lpi_search_wide_workspace`` bytes (256 or 512 pairs per gallery split and query
row: 264 MiB where the score matrix of 2048 x 1 048 576 would be 8 GiB), and every property above holds for every operand type.

``rerank`` is the second stage of a two-stage search (csrc/search_rerank.hip): the exact scores of a short candidate list per query row, with the bits
``topk`` of the same operand type gives those pairs, and the k best of them.  ``topk_reranked`` runs a coarse ``topk`` ("mx8" / "bf16") that
over-fetches a little and re-ranks its lists on the better operand: where the coarse list holds the f32 top k, the result IS ``topk``'s f32 result."""
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
    """None | 'f32' -> None (the f32 entry points); 'bf16' | 'f16' -> (LPI code, torch dtype); 'mx8' -> 'mx8'; 'mx4' -> 'mx4'."""
    if operands is None or operands == "f32":
        return None
    if operands == "mx8" or operands == "mx4":
        return operands
    if not isinstance(operands, str) or operands not in _OPERANDS:
        raise ValueError(f"unknown operands {operands!r} (f32 | bf16 | f16 | mx8 | mx4)")
    return _OPERANDS[operands]


class _MxRows:
    """Rows in one of the project's block-scaled formats (include/lpi_hip.h): ``codes`` uint8 [n, E / elements per byte] and ``scales`` uint8 [n, E / 32]
    (E8M0, one per 32 consecutive elements), as the search reads them in place: unit inner strides, a 16-byte row stride and base for the codes, a 4-byte
    row stride and base for the scales.  Immutable; ``rows[a:b]`` is a view of rows a..b-1 (a gallery searched in chunks with ``col_base`` / ``into``);
    ``shape`` is (n, E) in ELEMENTS.  A subclass states its ``operands`` name and the elements a code byte holds."""
    __slots__ = ("codes", "scales")
    _FMT, _PER_BYTE = None, 0

    def __init__(self, codes, scales):
        cls, per = type(self).__name__, self._PER_BYTE
        for name, t in (("codes", codes), ("scales", scales)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 2:
                raise ValueError(f"{cls}: {name} must be a uint8 tensor [rows, ...]")
        n, E = codes.shape[0], per * codes.shape[1]
        if E == 0 or E % 32 or tuple(scales.shape) != (n, E // 32):
            raise ValueError(f"{cls}: codes [n, {'E' if per == 1 else f'E / {per}'}] with E a multiple of 32 and scales [n, E / 32], "
                             f"got {tuple(codes.shape)} and {tuple(scales.shape)}")
        if codes.device != scales.device:
            raise ValueError(f"{cls}: codes and scales on different devices")
        for name, t, align in (("codes", codes, 16), ("scales", scales, 4)):
            if t.stride(1) != 1 or t.stride(0) % align or t.stride(0) < t.shape[1] or t.data_ptr() % align:
                raise ValueError(f"{cls}: {name} needs a unit inner stride and a row stride and base that are multiples of {align} bytes")
        object.__setattr__(self, "codes", codes)
        object.__setattr__(self, "scales", scales)

    def __setattr__(self, name, value):
        raise AttributeError(f"{type(self).__name__} is immutable")

    @property
    def shape(self):
        return torch.Size((self.codes.shape[0], self._PER_BYTE * self.codes.shape[1]))

    @property
    def device(self):
        return self.codes.device

    @property
    def nbytes(self):
        """The bytes of the codes and scales themselves (gaps of a strided view are not counted)."""
        n, E = self.shape
        return n * (E // self._PER_BYTE) + n * (E // 32)

    def __len__(self):
        return self.codes.shape[0]

    def __getitem__(self, rows):
        if not isinstance(rows, slice) or rows.step not in (None, 1):
            raise TypeError(f"{type(self).__name__}[a:b]: a slice of rows with step 1")
        return type(self)(self.codes[rows], self.scales[rows])


class Mx8Rows(_MxRows):
    """MX-FP8 rows: ``codes`` uint8 [n, E] (e4m3fn bytes) and their scales; what ``quantize_mx8`` returns and ``operands="mx8"`` reads."""
    __slots__ = ()
    _FMT, _PER_BYTE = "mx8", 1


class Mx4Rows(_MxRows):
    """MX-FP4 rows: ``codes`` uint8 [n, E / 2] (e2m1 nibbles, element 2 j in the low nibble of byte j) and their scales; what ``quantize_mx4`` returns and
    ``operands="mx4"`` reads.  A coarse operand: ``topk`` and the coarse stage of ``topk_reranked`` take it, ``gt_rank`` and ``rerank`` do not."""
    __slots__ = ()
    _FMT, _PER_BYTE = "mx4", 2


_MX = {cls._FMT: cls for cls in (Mx8Rows, Mx4Rows)}      # operands name -> rows class
_QUANT_DT = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}


def _quantize(x, fmt):
    """f32 / bf16 / f16 [n, E] on the device (E a multiple of 32) -> the rows class of `fmt`: one lpi_<fmt>_quantize launch."""
    if x.dim() != 2:
        raise ValueError("expected a [rows, E] tensor")
    if x.dtype not in _QUANT_DT:
        x = x.float()
    n, E = x.shape
    if n == 0 or E == 0 or E % 32:
        raise ValueError(f"quantize_{fmt}: [n, E] with n > 0 and E a positive multiple of 32, got {tuple(x.shape)}")
    if x.stride(1) != 1 or x.stride(0) % 4 or x.stride(0) < E or x.data_ptr() % (4 * x.element_size()):
        x = x.contiguous()
    codes = torch.empty(n, E // _MX[fmt]._PER_BYTE, dtype=torch.uint8, device=x.device)
    lds = (E // 32 + 3) // 4 * 4      # scale rows of whole dwords
    scales = torch.empty(n, lds, dtype=torch.uint8, device=x.device)[:, :E // 32]
    _lib.call(f"lpi_{fmt}_quantize", _QUANT_DT[x.dtype], n, E, x, x.stride(0), codes, codes.shape[1], scales, lds, torch.cuda.current_stream().cuda_stream)
    return _MX[fmt](codes, scales)


def quantize_mx8(x):
    """f32 / bf16 / f16 [n, E] on the device (E a multiple of 32) -> Mx8Rows: one lpi_mx8_quantize launch (bit for bit tests/mx8_emulate.quantize)."""
    return _quantize(x, "mx8")


def quantize_mx4(x):
    """f32 / bf16 / f16 [n, E] on the device (E a multiple of 32) -> Mx4Rows: one lpi_mx4_quantize launch (bit for bit tests/mx4_emulate.quantize)."""
    return _quantize(x, "mx4")


def _check_rows(queries, gallery, typed, message, block_scaled=True):
    """The "rows class and `operands` disagree" refusals, `message` filled in for the format: an operand of a rows class whose format is not `typed`, and,
    in a call that takes no block-scaled operands at all (block_scaled=False), such a `typed` itself."""
    for fmt, cls in _MX.items():
        rows = isinstance(queries, cls) or isinstance(gallery, cls)
        if (rows and typed != fmt) or (not block_scaled and typed == fmt):
            raise ValueError(message.format(fmt=fmt, cls=cls.__name__, bits=fmt[2]))


def _entry(form, typed, wide=False):
    """The entry point of `form` ('topk' | 'rank' | 'rerank') for `typed` (_operands): lpi_search_{form}[_wide]{'' | _t | _mx8 | _mx4}."""
    return f"lpi_search_{form}{'_wide' if wide else ''}{'' if typed is None else '_' + typed if typed in _MX else '_t'}"


def _lead(typed, nq, ng, E, q, g):
    """The arguments every entry point begins with, up to the gallery's."""
    if typed in _MX:
        return (nq, ng, E, q.codes, q.codes.stride(0), q.scales, q.scales.stride(0), g.codes, g.codes.stride(0), g.scales, g.scales.stride(0))
    return (() if typed is None else (typed[0],)) + (nq, ng, E, q, q.stride(0), g, g.stride(0))


def _prepare(queries, gallery, typed, form):
    """The operands as `typed` (_operands) wants them -> (nq, ng, device, the arguments of the entry point of `form` = 'topk' | 'rank' up to the gallery's)."""
    _check_rows(queries, gallery, typed, 'an {cls} operand is searched with operands="{fmt}"')
    if typed == "mx4" and form != "topk":
        raise ValueError('MX-FP4 ("mx4", an Mx4Rows) is a coarse top-k type: there is no rank form on its scores')
    if typed is None:
        q, g = _f32_rows(queries), _f32_rows(gallery)
    elif typed in _MX:
        q, g = (t if isinstance(t, _MX[typed]) else _quantize(t, typed) for t in (queries, gallery))
    else:
        q, g = _rows16(queries, typed[1]), _rows16(gallery, typed[1])
    nq, E = q.shape
    ng = g.shape[0]
    if g.shape[1] != E:
        raise ValueError(f"queries have {E} features, the gallery {g.shape[1]}")
    if typed in _MX and E % 128:
        raise ValueError(f"MX-FP{typed[2]} operands are searched with E a multiple of 128, not {E}")
    return nq, ng, q.device, _lead(typed, nq, ng, E, q, g)


def _rows16(t, dtype):
    """`dtype` (2 bytes) with unit inner stride, a 16-byte row stride and a 16-byte aligned base: such a tensor is used in place, anything else is cast
    or made contiguous once."""
    if t.dim() != 2:
        raise ValueError("expected a [rows, E] tensor")
    if t.dtype != dtype or t.stride(1) != 1 or t.stride(0) % 8 or t.stride(0) < t.shape[1] or t.data_ptr() % 16:
        t = t.to(dtype).contiguous()
    return t


_KNARROW = 16      # the narrow entry points' k range; above it, up to 256, the wide ones (search_wide.hip)


def _workspace(dev, nq, ng, k):
    fn = "lpi_search_wide_workspace" if k > _KNARROW else "lpi_search_workspace"
    need = int(getattr(_lib.load(), fn)(nq, ng, k))
    if need <= 0:
        raise _lib.LpiError(f"{fn}({nq}, {ng}, {k}) refused the shape")
    ws = _WS.get(dev)
    if ws is None or ws.numel() < need:
        _WS[dev] = None      # drop the old one first: the peak is one workspace, not two
        ws = _WS[dev] = torch.empty(need, dtype=torch.uint8, device=dev)
    return ws


def topk(queries, gallery, k, *, col_base=0, into=None, operands=None):
    """-> (idx int32 [nq, k], val f32 [nq, k]), 1 <= k <= 256: per query row the k largest scores in the order (value descending, then index
    descending), lpi_topk's.  ``col_base`` is added to the indices.  ``into`` = the (idx, val) of earlier calls over other gallery chunks: the lists are merged in
    place and returned.  ``operands``: None | "f32" (anything not f32 is cast to f32) | "bf16" | "f16" (both operands end in that type; val stays f32)
    | "mx8" (an Mx8Rows is read in place, a float tensor is quantised once; val = the scores of the quantised rows) | "mx4" (the same with an Mx4Rows:
    a coarse list, to be re-ranked)."""
    typed = _operands(operands)
    nq, ng, dev, lead = _prepare(queries, gallery, typed, "topk")
    if into is None:
        idx = torch.empty(nq, k, dtype=torch.int32, device=dev)
        val = torch.empty(nq, k, dtype=torch.float32, device=dev)
    else:
        idx, val = into
        if (tuple(idx.shape) != (nq, k) or tuple(val.shape) != (nq, k) or idx.dtype != torch.int32 or val.dtype != torch.float32
                or not idx.is_contiguous() or not val.is_contiguous()):
            raise ValueError("into = (idx int32 [nq, k], val f32 [nq, k]), contiguous")
    ws = _workspace(dev, nq, ng, k)
    _lib.call(_entry("topk", typed, wide=k > _KNARROW), *lead, int(k), int(col_base), 0 if into is None else 1, idx, val, ws, ws.numel(), torch.cuda.current_stream().cuda_stream)
    return idx, val


def gt_rank(queries, gallery, gt, *, operands=None):
    """-> rank int32 [nq]: lpi_retrieval_rank of the score matrix the two feature sets would give, over the ground-truth list ``gt`` int32 [nq] or
    [nq, gt_per_row] (entries < 0 are padding).  ``operands`` as in ``topk``, without "mx4": MX-FP4 scores are no basis for a metric."""
    typed = _operands(operands)
    nq, ng, dev, lead = _prepare(queries, gallery, typed, "rank")
    gt = torch.as_tensor(gt).to(device=dev, dtype=torch.int32).reshape(nq, -1).contiguous()
    rank = torch.empty(nq, dtype=torch.int32, device=dev)
    ws = _workspace(dev, nq, ng, 0)
    _lib.call(_entry("rank", typed), *lead, gt, gt.shape[1], rank, ws, ws.numel(), torch.cuda.current_stream().cuda_stream)
    return rank


_KWIDE = 256      # LPI_SEARCH_KWIDE: the longest list of topk and the longest candidate list of rerank


def rerank(queries, gallery, cand, k=None, *, operands=None):
    """-> (idx int32 [nq, k], val f32 [nq, k]): per query row the k best of the gallery rows listed in ``cand`` [nq, kc] (integer, kc <= 256; k defaults
    to kc), scored on the operands themselves, in ``topk``'s order.  An entry outside [0, ng) is padding (the -1 of a short list), an index that occurs
    several times in a row counts once (lists of several coarse passes may simply be concatenated), unfilled slots are (-1, -inf) and come last.
    ``val`` has the bits ``topk`` with the same ``operands`` returns for the pair, so a re-ranked list compares with ``==`` against a searched one.
    ``operands``: None | "f32" | "bf16" | "f16" with ``topk``'s in-place rules; MX-FP8 and MX-FP4 are not re-rank types (the second stage exists for the
    better operand).  An int32 ``cand`` with unit inner stride is read in place, a row-strided view included; anything else is converted once.  One launch,
    no workspace."""
    typed = _operands(operands)
    _check_rows(queries, gallery, typed, 'rerank scores f32 / bf16 / f16 operands: MX-FP{bits} ("{fmt}", an {cls}) is a coarse type, not a re-rank type',
                block_scaled=False)
    if not isinstance(cand, torch.Tensor) or cand.dim() != 2 or cand.dtype.is_floating_point or cand.dtype in (torch.bool, torch.complex64, torch.complex128):
        raise ValueError("cand = an integer tensor [nq, kc]")
    if queries.dim() != 2 or gallery.dim() != 2:
        raise ValueError("expected [rows, E] tensors")
    nq, E = queries.shape
    ng = gallery.shape[0]
    if gallery.shape[1] != E:
        raise ValueError(f"queries have {E} features, the gallery {gallery.shape[1]}")
    kc = cand.shape[1]
    if cand.shape[0] != nq:
        raise ValueError(f"cand has {cand.shape[0]} rows, the queries {nq}")
    if not 1 <= kc <= _KWIDE:
        raise ValueError(f"cand lists 1 .. {_KWIDE} candidates per row, not {kc}")
    k = kc if k is None else int(k)
    if not 1 <= k <= kc:
        raise ValueError(f"1 <= k <= kc = {kc}, not {k}")
    if typed is None:
        q, g = _f32_rows(queries), _f32_rows(gallery)
    else:
        q, g = _rows16(queries, typed[1]), _rows16(gallery, typed[1])
    dev = q.device
    if cand.dtype != torch.int32 or cand.stride(1) != 1 or cand.stride(0) < kc or cand.device != dev:
        if cand.dtype != torch.int32:      # an index that does not fit int32 must stay padding
            cand = torch.where((cand < 0) | (cand >= ng), torch.full_like(cand, -1), cand)
        cand = cand.to(device=dev, dtype=torch.int32).contiguous()
    idx = torch.empty(nq, k, dtype=torch.int32, device=dev)
    val = torch.empty(nq, k, dtype=torch.float32, device=dev)
    _lib.call(_entry("rerank", typed), *_lead(typed, nq, ng, E, q, g), cand, cand.stride(0), kc, k, idx, val, torch.cuda.current_stream().cuda_stream)
    return idx, val


def topk_reranked(queries, gallery, k, *, coarse="mx8", candidates=None, coarse_queries=None, coarse_gallery=None, operands=None):
    """Two-stage search -> (idx int32 [nq, k], val f32 [nq, k]): ``topk(coarse_queries or queries, coarse_gallery or gallery, candidates,
    operands=coarse)`` (the narrow kernels up to 16 candidates, the wide ones above), then ``rerank(queries, gallery, its idx, k, operands=operands)``.
    Where the coarse list of a row holds the row's exact top k, the row's result is ``topk(queries, gallery, k, operands=operands)``'s, bit for bit; a
    neighbour the coarse pass ranks below ``candidates`` is lost.  ``candidates`` defaults to min(ng, 256, max(4 k, 32)), a choice, not a measurement
    (DESIGN.md has what k, 2 k and 4 k recover), and must satisfy k <= candidates <= min(ng, 256).  With ``coarse="mx4"`` the default is
    min(ng, 256, max(16 k, 128)): a choice taken from a CPU emulation of the format on random unit rows ("MX-FP4 operands": at k = 10 the f32
    top 10 lay inside the MX-FP4 top 128 for every row tried, inside the top 64 for 98 - 100 %), to be revisited with the measured table: at
    123 287 x 616 767 random unit rows 128 candidates lost a neighbour on 0.18 % of the rows and 256 on none, so pass ``candidates=256`` where every
    row matters.
    ``coarse_gallery`` / ``coarse_queries``: the ``Mx8Rows`` (``quantize_mx8``), the ``Mx4Rows`` (``quantize_mx4``) or the 2-byte copy of the operand,
    held by the caller across calls; WITHOUT them the operand is quantised or cast again on every call, which for the gallery costs a pass over it and
    its coarse copy in memory each time.  A coarse gallery searched in chunks
    composes with ``rerank`` directly: ``topk(..., col_base=, into=)`` over the chunks, then one ``rerank`` on the whole exact gallery."""
    ctyped = _operands(coarse)      # an unknown name is refused here, before anything else
    if _operands(operands) in ("mx8", "mx4"):
        raise ValueError(f'the re-rank operands are f32 / bf16 / f16, not "{operands}"')
    ng = gallery.shape[0]
    k = int(k)
    top = min(ng, _KWIDE)
    if candidates is None:
        candidates = min(top, max(16 * k, 128) if ctyped == "mx4" else max(4 * k, 32))
    candidates = int(candidates)
    if not 1 <= k <= candidates <= top:
        raise ValueError(f"1 <= k <= candidates <= min(ng, {_KWIDE}) = {top}, not k = {k}, candidates = {candidates}")
    cq = queries if coarse_queries is None else coarse_queries
    cg = gallery if coarse_gallery is None else coarse_gallery
    if cq.shape[0] != queries.shape[0] or cg.shape[0] != ng:
        raise ValueError("the coarse operands have the rows of the exact ones")
    cidx, _ = topk(cq, cg, candidates, operands=coarse)
    return rerank(queries, gallery, cidx, k, operands=operands)
