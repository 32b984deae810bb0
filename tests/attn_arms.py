"""The strided-arm / tight-arm assertions of the attention family (a plain helper module next to strided.py: no fixtures, no pytest settings; works on the
CPU and on the GPU).  tests/test_attn_strides_gpu.py runs the HIP kernels through it, tests/test_attn_strides_host.py proves on CPU tensors that it catches
what it is meant to catch.  `check_arms` itself lives in tests/arms.py (the row-operation family uses it too) and is re-exported here.

A case builds its operands twice as {name: strided.Record}: the STRIDED arm (offset base pointers, every leading dimension different from the widths and from
each other, NaN in every pad) and the TIGHT arm (contiguous copies of the same values), runs the same calls on both, and hands both to `check_arms`:

  * no pad of any operand changed, inputs included, and no input changed at all                         (strided.check_pads)
  * every must-be-written element of every output was written                                            (strided.check_written; strided.must_write narrows it)
  * the tight arm's must-be-written values hold no NaN
  * the strided arm's must-be-written values are the tight arm's bit for bit: a leading dimension changes no arithmetic.

An output whose contents are unspecified (`delta`) has an empty must-be-written part: only its pads are checked.  `case_bytes` is the arena sizing rule of
strided.py for an attention case: every arena of the case, lse / delta included, gets that many bytes.
"""
import strided as S


def pad256(n):
    return (n + 255) // 256 * 256


def case_bytes(rows, lds, bases, max_esz=4):
    """One arena size for every operand of a case: the 256-rounded largest row count x the largest leading dimension x the largest element size (4: lse and
    delta are f32 in every case) + the largest base offset.  Whatever stride of the case a wrong kernel applies to whatever pointer of the case stays inside."""
    return S.arena_bytes(pad256(rows), max(lds), max_esz, max(bases))


from arms import check_arms, outputs  # noqa: E402,F401  (the generic assertions; kept importable from here)
