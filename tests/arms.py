"""The two-arm assertions of the strided-view tests (a plain helper module next to strided.py: no fixtures, no pytest settings; works on the CPU and on the GPU).
tests/test_attn_strides_gpu.py (through attn_arms), tests/test_rowop_strides_gpu.py and tests/test_loss_strides_gpu.py run HIP kernels through it;
tests/test_attn_strides_host.py, tests/test_rowop_strides_host.py and tests/test_loss_strides_host.py prove on CPU tensors that it catches what it is meant to catch.

A case builds its operands twice as {name: strided.Record} and runs the same calls on both.  Usually the arms are the STRIDED one (offset base pointers, every
leading dimension different from the widths and from each other, NaN in every pad) and the TIGHT one (contiguous copies of the same values); `names` renames them
where a case compares something else (a single-op launch against the same op as a row job, both on strided operands).  `check_arms` asserts:

  * no pad of any operand changed, inputs included, and no input changed at all                         (strided.check_pads)
  * every must-be-written element of every output was written                                            (strided.check_written; strided.must_write narrows it)
  * kept = True: the rest of every output's footprint kept its bits                                     (strided.check_kept)
  * the second arm's must-be-written values hold no NaN
  * the first arm's must-be-written values are the second arm's bit for bit: a leading dimension changes no arithmetic.

An output whose contents are unspecified has an empty must-be-written part: only its pads are checked.
"""
import torch

import strided as S
from poison import same_bits


def outputs(ops):
    return [k for k, o in ops.items() if o.output]


def check_arms(label, strided_ops, tight_ops, sync=None, names=("strided", "tight"), kept=False):
    if sync is not None:
        sync()
    for arm, ops in zip(names, (strided_ops, tight_ops)):
        for k, o in ops.items():
            S.check_pads(f"{label} {k} ({arm} arm)", o)
        for k in outputs(ops):
            S.check_written(f"{label} {k} ({arm} arm)", ops[k])
            if kept:
                S.check_kept(f"{label} {k} ({arm} arm)", ops[k])
    assert outputs(strided_ops) == outputs(tight_ops) and outputs(tight_ops), label
    compared = 0
    for k in outputs(tight_ops):
        s, t = (o.arena[o.must] for o in (strided_ops[k], tight_ops[k]))      # the must-be-written values in address order = row by row in both arms
        assert s.numel() == t.numel(), f"{label} {k}: the arms' footprints differ"
        if t.numel() == 0:
            continue
        compared += 1
        assert not bool(torch.isnan(t.float()).any()), f"{label} {k}: NaN in the {names[1]} arm"
        assert same_bits(s, t), f"{label} {k}: the {names[0]} arm differs from the {names[1]} arm in {int((S.bits(s) != S.bits(t)).sum())} of {t.numel()} values"
    assert compared > 0, label
