"""Dead-memory poisoning for kernel tests (a plain helper module: no fixtures, no pytest settings).

A kernel is handed memory it must not use: padded rows of an arena, rows behind a sample's length, the masked half of a causal
sequence, scratch whose contents are "unspecified".  With finite stale data a kernel that loads such memory and multiplies it by a
zero probability still passes every tolerance; with NaN it cannot (0 x NaN = NaN).  A case therefore runs twice:

    arm A   dead regions hold zeros (a fresh arena), preserved regions hold NaN
    arm B   dead regions hold NaN,                    preserved regions hold NaN

and `two_arms` asserts that the poisoned element count is > 0, that the live outputs of A and B are bit-identical, that preserved
regions still hold their fill in both arms, that arm A's live outputs hold no NaN, and that arm A meets the f64 reference the case
registered.  "Dead on read" = the header or the engine says the call does not use it; "preserved" = the call must not write it.

A case is a function `case(arm)` that builds its buffers, marks them through `arm`, and calls the kernel:

    arm.dead(t, mask)            fill t where mask is True (mask None: all of t): zeros in arm A, NaN in arm B
    arm.dead_index(t, mask, n)   integer indices: arm B replaces t[mask] by a DIFFERENT index that is still in [0, n); arm A keeps them
    arm.preserve(name, t, mask)  NaN in both arms; checked for bit-identity with that fill after the case returns
    arm.out(name, t, mask, ref=None, tol=None)   a live output (mask None: all live); ref: f64 tensor of t's shape (arm A is held to it)

Masks are bool tensors of t's shape, or of its leading dimensions (a row mask of a [rows, d] buffer).
"""
import torch

_INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float64: torch.int64}


def bits(t):
    """t's bit patterns as an integer tensor (floating types through an integer view; integer types as they are)."""
    t = t.contiguous()
    return t.view(_INT_VIEW[t.dtype]) if t.dtype in _INT_VIEW else t


def same_bits(a, b):
    """True if a and b hold the same bit patterns: NaN payloads compare equal to themselves, -0.0 differs from 0.0."""
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def full_mask(t, mask):
    """`mask` (None = everything; a bool tensor of t's shape or of its leading dimensions) as a bool tensor of t's shape on t's device."""
    if mask is None:
        return torch.ones(t.shape, dtype=torch.bool, device=t.device)
    mask = torch.as_tensor(mask, dtype=torch.bool).to(t.device)
    assert mask.shape == t.shape[:mask.dim()], (tuple(mask.shape), tuple(t.shape))
    return mask.reshape(mask.shape + (1,) * (t.dim() - mask.dim())).expand(t.shape)


def fill(t, mask, value):
    """t[mask] = value in place (f32 / bf16 / f16; value may be NaN); returns the number of elements written."""
    assert t.dtype in (torch.float32, torch.bfloat16, torch.float16), t.dtype
    m = full_mask(t, mask)
    t.masked_fill_(m, value)
    return int(m.sum())


def fill_nan(t, mask=None):
    return fill(t, mask, float("nan"))


def other_index(t, mask, n):
    """Integer index array: t[mask] = (t[mask] + 1 + (t[mask] % (n - 1))) % n — a DIFFERENT index, still in [0, n).  Returns the count."""
    assert not t.dtype.is_floating_point and n >= 2
    m = full_mask(t, mask)
    old = t[m]
    assert bool(((old >= 0) & (old < n)).all())
    new = (old + 1 + old % (n - 1)) % n
    t[m] = new
    return int(m.sum())


def relerr(got, ref):
    """max |got - ref| / max |ref| in f64 (the measure of tests/test_kernels_gpu.py)."""
    got, ref = got.double().cpu(), ref.double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


class Arm:
    def __init__(self, poison):
        self.poison = poison
        self.poisoned = 0          # dead elements filled (the same count in both arms)
        self.outs = {}             # name -> (live values [n], ref values [n] or None, tol, err)
        self._kept = []            # (name, tensor, mask, the fill's bits)

    def dead(self, t, mask=None, count=True):
        """count=False: a region that was counted before and is filled again (an output of the forward that is dead to the backward)."""
        n = fill(t, mask, float("nan") if self.poison else 0.0)
        self.poisoned += n if count else 0
        return t

    def dead_index(self, t, mask, n):
        if self.poison:
            self.poisoned += other_index(t, mask, n)
        else:
            self.poisoned += int(full_mask(t, mask).sum())
        return t

    def preserve(self, name, t, mask=None):
        m = full_mask(t, mask).clone()
        assert fill_nan(t, m) > 0, name
        self._kept.append((name, t, m, bits(t[m]).clone()))
        return t

    def out(self, name, t, mask=None, ref=None, tol=None, err=relerr):
        """err(got, ref) -> float on CPU tensors: the error measure the bar `tol` belongs to (default: relerr); tol == 0 asks for equality."""
        assert name not in self.outs, name
        m = full_mask(t, mask)
        self.outs[name] = (t[m].clone(), None if ref is None else ref.to(t.device)[m].double().cpu(), tol, err)

    def check_preserved(self):
        for name, t, m, before in self._kept:
            assert torch.equal(bits(t[m]), before), f"{name}: a preserved region was written (arm {'B' if self.poison else 'A'})"


def two_arms(case, label="", sync=None):
    """Run `case` with zeros and with NaN in its dead regions and hold it to the contract above.  Returns the poisoned element count."""
    arms = []
    for poison in (False, True):
        arm = Arm(poison)
        case(arm)
        if sync is not None:
            sync()
        arm.check_preserved()
        arms.append(arm)
    a, b = arms
    print(f"POISON {label}: {b.poisoned} dead elements poisoned, {sum(int(k[2].sum()) for k in b._kept)} preserved")
    assert b.poisoned > 0 and a.poisoned == b.poisoned, (label, a.poisoned, b.poisoned)
    assert a.outs.keys() == b.outs.keys() and len(a.outs) > 0
    for name, (va, ref, tol, err) in a.outs.items():
        vb = b.outs[name][0]
        assert va.numel() > 0, name
        if va.dtype.is_floating_point:
            assert not bool(torch.isnan(va).any()), f"{label} {name}: NaN in a live output with zeros in the dead regions"
        assert same_bits(va, vb), f"{label} {name}: the live output depends on dead memory ({int((bits(va) != bits(vb)).sum())} of {va.numel()} values differ)"
        if ref is not None:
            e = err(va.cpu(), ref)
            print(f"    {name}: error {e:.3e} (bar {tol:g})")
            assert (e <= tol) if tol == 0 else (e < tol), (label, name, e, tol)
    return b.poisoned
