"""Strided operands for kernel tests (a plain helper module: no fixtures, no pytest settings; works on the CPU and on the GPU).

A kernel that takes a leading dimension per operand is handed sub-matrix VIEWS: an offset base pointer and a row stride larger than the
width.  A test that passes contiguous tensors (ld == width, base == start of the allocation) cannot tell `ldc` from `ldr`, `lda` from `K`,
or a 16-byte store that runs over a row's end from one that does not.  Here every operand of a case lives in a flat ARENA of its own:

    operand(rows, cols, ld, dtype, col0, arena_elems, fill)   a [rows, cols] view with stride (ld, 1) whose first element is arena[col0]

    * every arena element OUTSIDE the view's footprint {col0 + r * ld + c} holds PAD, a NaN (set by bit pattern): read into a result it
      shows as NaN, written it shows in `check_pads`, which compares the arena's bits with those of before the call;
    * an INPUT (fill = a [rows, cols] tensor) holds its live values in the footprint;
    * an OUTPUT (fill = None) holds UNWRITTEN there, a second NaN with other bits: `check_written` finds what the kernel left out (1-byte operands,
      torch.uint8 = MX-FP8 element and scale bytes: PAD 0x7F, UNWRITTEN 0xFF; compared as bytes; torch.int32 = labels / ranks / indices: two negative sentinels).  `in_out` turns a filled operand into an output.  Where a
      call MAY leave a part of its output untouched (the rows behind `rows_needed` of an attention backward, a scratch block whose contents
      are unspecified), `must_write` narrows what `check_written` asks for: the rest of the footprint is neither a pad nor a must — unless the
      call must leave it alone (the rows of a stream it does not own): `check_kept` holds it to its earlier bits.

THE SAFETY RULE (arena sizing).  Within one test case EVERY arena has the same size in bytes, `arena_bytes(...)`, worked out from the
LARGEST row count, the LARGEST leading dimension and the LARGEST element size of ANY operand of that case, plus the base offset col0:

    bytes = (max_col0 + max_rows * max_ld) * max_esz + SLACK

so whichever leading dimension, row count or element size a wrong kernel applies to whichever pointer of the case — ldr for C, K for lda,
4-byte elements on a 2-byte operand, a 16-byte access at a row's last 8 bytes — the address stays inside that operand's own allocation.
A wrong kernel fails an assertion; it never faults.  (Operands that are not matrices — a statistics block, a slot buffer — use `region`
with an explicit index list and the same arena size.)
"""
import torch

from poison import bits

# NaNs, told apart by their payloads.  torch.uint8 carries the MX-FP8 operands (e4m3 element bytes, E8M0 scale bytes): PAD 0x7F is e4m3's NaN, UNWRITTEN 0xFF is
# the NaN of both formats, which neither an element code nor a scale byte of finite data can be — so `check_written` still tells "left out" from "written"
# torch.int32 carries labels, ranks, indices, counts and flags (the loss / k-means / ranking family): PAD and UNWRITTEN are two large NEGATIVE integers, which no label,
# rank (0 .. n_cols, or 0x7fffffff for "no ground truth"), index or the -1 that pads a ground-truth list can equal; compared as integers
PAD = {torch.float32: 0x7FC00BAD, torch.bfloat16: 0x7FC5, torch.float16: 0x7E05, torch.uint8: 0x7F, torch.int32: -0x5AD5AD00}
UNWRITTEN = {torch.float32: 0x7FC0F00D, torch.bfloat16: 0x7FCA, torch.float16: 0x7E0A, torch.uint8: 0xFF, torch.int32: -0x0F00D000}
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.uint8: torch.uint8, torch.int32: torch.int32}
SLACK = 64      # bytes behind the last row: a 16-byte access that starts inside the last row ends inside the arena


def arena_bytes(max_rows, max_ld, max_esz, col0=0):
    """The one arena size of a test case (see THE SAFETY RULE); col0 = the largest base offset of the case, in elements."""
    return (col0 + max_rows * max_ld) * max_esz + SLACK


class Record:
    """What `operand` / `region` return: .t the view (hand it to the kernel), .arena the flat allocation, .inside the footprint as a bool
    mask over the arena, .before the arena's bits after set-up, .output whether the footprint holds UNWRITTEN."""

    def __init__(self, t, arena, inside, output):
        self.t, self.arena, self.inside, self.output = t, arena, inside, output
        self.must = inside      # the part of an output's footprint the call MUST write (narrowed by `must_write`)
        self.before = bits(arena).clone()


def _arena(arena_elems, dtype, device):
    assert dtype in _INT, dtype
    return torch.full((arena_elems,), PAD[dtype], dtype=_INT[dtype], device=device).view(dtype)      # every pattern here fits its integer type


def region(index, dtype, arena_elems, fill=None, device="cpu"):
    """An arena of `arena_elems` elements whose footprint is the explicit element list `index` (int64, distinct): `fill` (as many values, in
    that order) or UNWRITTEN.  Returns a Record whose .t is the whole arena (the caller hands the kernel .t[first:])."""
    index = torch.as_tensor(index, dtype=torch.int64, device=device)
    assert index.numel() > 0 and int(index.min()) >= 0 and int(index.max()) < arena_elems, "the footprint leaves the arena: size every arena with arena_bytes()"
    arena = _arena(arena_elems, dtype, device)
    inside = torch.zeros(arena_elems, dtype=torch.bool, device=device)
    inside[index] = True
    assert int(inside.sum()) == index.numel(), "footprint elements overlap"
    if fill is None:
        arena.view(_INT[dtype])[index] = UNWRITTEN[dtype]
    else:
        arena[index] = fill.to(device=device, dtype=dtype).reshape(-1)
    return Record(arena, arena, inside, fill is None)


def operand(rows, cols, ld, dtype, col0, arena_elems, fill=None, device="cpu"):
    """A [rows, cols] view with stride(0) == ld, stride(1) == 1, first element arena[col0] (so data_ptr() is not the start of the allocation
    when col0 > 0).  fill: the [rows, cols] live values of an input; None for an output.  Returns a Record (.t is the view)."""
    assert ld >= cols and col0 >= 0
    assert col0 + (rows - 1) * ld + cols <= arena_elems, "the footprint leaves the arena: size every arena with arena_bytes()"
    arena = _arena(arena_elems, dtype, device)
    view = arena.as_strided((rows, cols), (ld, 1), col0)
    inside = torch.zeros(arena_elems, dtype=torch.bool, device=device)
    inside.as_strided((rows, cols), (ld, 1), col0).fill_(True)
    if fill is None:
        view.view(_INT[dtype]).fill_(UNWRITTEN[dtype])
    else:
        assert tuple(fill.shape) == (rows, cols), (tuple(fill.shape), rows, cols)
        view.copy_(fill.to(dtype))
    assert view.stride() == (ld, 1) and view.data_ptr() == arena.data_ptr() + col0 * arena.element_size()
    return Record(view, arena, inside, fill is None)


def in_out(rec):
    """An operand the call reads AND writes (a gradient stream it adds to): built with its live values as `fill`, then held as an output — its pads are
    checked, its footprint may change, `must_write` / `check_kept` say which part of it."""
    rec.output = True
    return rec


def must_write(rec, rows=None, none=False, index=None):
    """Narrow what `check_written` asks of the output `rec`.  Give one of:
        rows   an `operand` view: a count (the first rows) or a list of row indices;
        index  a `region`: the arena elements;
        none   True: nothing must be written (contents unspecified).
    The rest of the footprint may be written or left: neither `check_pads` nor `check_written` looks at it."""
    assert rec.output
    must = torch.zeros_like(rec.inside)
    if index is not None:
        must[torch.as_tensor(index, dtype=torch.int64, device=must.device)] = True
        assert not bool((must & ~rec.inside).any())
    elif not none:
        assert rec.t.dim() == 2
        r = torch.arange(rows) if isinstance(rows, int) else torch.as_tensor(rows, dtype=torch.int64)
        assert r.numel() > 0 and int(r.min()) >= 0 and int(r.max()) < rec.t.shape[0]
        col0 = (rec.t.data_ptr() - rec.arena.data_ptr()) // rec.arena.element_size()
        idx = col0 + r[:, None] * rec.t.stride(0) + torch.arange(rec.t.shape[1])[None, :]
        must[idx.reshape(-1).to(must.device)] = True
    rec.must = must
    return rec


def check_pads(name, rec):
    """Every arena element outside the footprint still has the bits it had before the call (integer compare: NaN payloads count)."""
    now = bits(rec.arena)
    changed = (now != rec.before) & ~rec.inside
    n = int(changed.sum())
    assert n == 0, f"{name}: {n} elements outside the operand's footprint were written (first at arena element {int(changed.nonzero()[0])})"
    if not rec.output:
        assert torch.equal(now, rec.before), f"{name}: an input operand was written"


def check_written(name, rec):
    """No must-be-written footprint element of an output still holds UNWRITTEN."""
    assert rec.output, name
    left = (bits(rec.arena) == UNWRITTEN[rec.arena.dtype]) & rec.must
    n = int(left.sum())
    assert n == 0, f"{name}: {n} of {int(rec.must.sum())} output elements were never written (first at arena element {int(left.nonzero()[0]) if n else -1})"


def check_kept(name, rec):
    """The footprint elements of an output that are NOT must-be-written still have the bits they had before the call: for a call that owns some rows of a
    larger matrix (the mapped rows of a stream) and must leave the others alone.  Not for outputs whose remaining part MAY be written (attn_arms)."""
    assert rec.output, name
    changed = (bits(rec.arena) != rec.before) & rec.inside & ~rec.must
    n = int(changed.sum())
    assert n == 0, f"{name}: {n} footprint elements the call does not own were written (first at arena element {int(changed.nonzero()[0]) if n else -1})"
