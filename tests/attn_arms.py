"""The strided-arm / tight-arm assertions of the attention family (a plain helper module next to strided.py: no fixtures, no pytest settings; works on the
CPU and on the GPU).  tests/test_attn_strides_gpu.py runs the HIP kernels through it, tests/test_attn_strides_host.py proves on CPU tensors that it catches
what it is meant to catch.

A case builds its operands twice as {name: strided.Record}: the STRIDED arm (offset base pointers, every leading dimension different from the widths and from
each other, NaN in every pad) and the TIGHT arm (contiguous copies of the same values), runs the same calls on both, and hands both to `check_arms`:

  * no pad of any operand changed, inputs included, and no input changed at all                         (strided.check_pads)
  * every must-be-written element of every output was written                                            (strided.check_written; strided.must_write narrows it)
  * the tight arm's must-be-written values hold no NaN
  * the strided arm's must-be-written values are the tight arm's bit for bit: a leading dimension changes no arithmetic.

An output whose contents are unspecified (`delta`) has an empty must-be-written part: only its pads are checked.  `case_bytes` is the arena sizing rule of
strided.py for an attention case: every arena of the case, lse / delta included, gets that many bytes.
"""
import torch

import strided as S
from poison import same_bits


def pad256(n):
    return (n + 255) // 256 * 256


def case_bytes(rows, lds, bases, max_esz=4):
    """One arena size for every operand of a case: the 256-rounded largest row count x the largest leading dimension x the largest element size (4: lse and
    delta are f32 in every case) + the largest base offset.  Whatever stride of the case a wrong kernel applies to whatever pointer of the case stays inside."""
    return S.arena_bytes(pad256(rows), max(lds), max_esz, max(bases))


def outputs(ops):
    return [k for k, o in ops.items() if o.output]


def check_arms(label, strided_ops, tight_ops, sync=None):
    if sync is not None:
        sync()
    for arm, ops in (("strided", strided_ops), ("tight", tight_ops)):
        for k, o in ops.items():
            S.check_pads(f"{label} {k} ({arm} arm)", o)
        for k in outputs(ops):
            S.check_written(f"{label} {k} ({arm} arm)", ops[k])
    assert outputs(strided_ops) == outputs(tight_ops) and outputs(tight_ops), label
    compared = 0
    for k in outputs(tight_ops):
        s, t = (o.arena[o.must] for o in (strided_ops[k], tight_ops[k]))      # the must-be-written values in address order = row by row in both arms
        assert s.numel() == t.numel(), f"{label} {k}: the arms' footprints differ"
        if t.numel() == 0:
            continue
        compared += 1
        assert not bool(torch.isnan(t.float()).any()), f"{label} {k}: NaN in the tight arm"
        assert same_bits(s, t), f"{label} {k}: the strided arm differs from the tight arm in {int((S.bits(s) != S.bits(t)).sum())} of {t.numel()} values"
    assert compared > 0, label
