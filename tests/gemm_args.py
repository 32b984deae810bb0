"""The argument grid of the GEMM family's HOST layer (lpi_amd/csrc/gemm.hip, gemm256.hip, gemm256p.hip, gemm256x128.hip, gemm_rows.hip, gemm_mx8.hip): which
argument lists each entry point accepts, which it refuses before any launch, and which kernel an accepted list is sent to.

The host code of this family never dereferences an operand pointer (the lpi_gemm_desc arrays are host memory and are real here), so the whole accept set can
be observed with made-up addresses, as tests/attn_args.py does for the attention family: a refused call returns LPI_EINVAL / LPI_ENOSYS and lpi_launch_count()
stays; an accepted call gets as far as the runtime, which, without a device, answers with its no-device code (100) — from the LDS set-up of the kernels that
need more than 64 KiB (no launch counted), or from the launch itself (counted).  Every launcher notes its kernel (lpi_gemm_last_kernel) BEFORE that set-up, so
the kernel chosen for an accepted list is on record too, with lpi_gemm_last_grouped.  The note is thread state that a refused call leaves alone: before every
tuple an ordinary few-row call (reset(), kernel LPI_GEMM_K_ROWS) puts it back to that known value, so a value left by the tuple before cannot pass for this one's.

cases() builds a deterministic grid.  Good lists: every built (dtype, c_dtype) pair with every epilogue it takes, with and without bias, residual and aux, at a
shape for each kernel (128-tile only; 256x256 one tile per workgroup; 256x128; persistent; the hybrid tail at 54528 x 768 = 639 tiles; weights above 3 MB with an
even and an odd N-tile count; a SIDE16 group whose summed N exceeds 8192; a grouped pair of 256 + 32 tiles and one a tile short; few-row calls of one and two
problems); LPI_F32X3; the LN-fold pairs and LPI_EPI_RES_ROWSTATS; each c_dtype of the two MX-FP8 entry points.  Every good list again under single tuning-key
changes (TUNINGS), set for the one call and restored.  Then every argument mutated one at a time (entry_points() says which good lists: not those that differ
from a mutated neighbour by a bias alone, or by a shape that takes the same way through the checks): pointers NULL / +2 / +4 / +8 bytes; leading dimensions 0, -1,
width - 4, +1, +2, +4, +8; M, N, K 0, -1 and plus or minus one, half and a quarter of a tile; every dtype and epilogue code from -1 to one past the header's
largest; count 0 .. 3; alpha 1 against 0.5; residual and aux present in only one problem of a pair (their pointer mutations).

Run as a script WITHOUT a GPU, this records (return code, launches, lpi_gemm_last_kernel, lpi_gemm_last_grouped) per tuple into tests/gemm_args_expected.json
(the distinct outcomes once, then a letter per tuple, one string per good list: load_record() reads it back):
    LPI_LIB=<build of the commit to record>/liblpi_hip.so python3 tests/gemm_args.py <hash of that commit>
The committed record is that of the library before the host layer moved onto one call struct and one typed pick (lpi_amd/csrc/gemm_host.h), with each
lpi_note_gemm_kernel call moved ahead of its lpi_ensure_lds as its only change.
"""
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from lpi_amd import _lib  # noqa: E402

EXPECTED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_args_expected.json")
F32, BF16, F16, MX8, F32X3 = 0, 1, 2, 3, 4
NAMES = {F32: "f32", BF16: "bf16", F16: "f16", MX8: "mx8", F32X3: "f32x3"}
NONE, QUICKGELU, DQUICKGELU, LN, LN_QUICKGELU, RES_ROWSTATS = range(6)
DT_CODES = range(-1, 7)       # one past LPI_MX4 = 5
EPI_CODES = range(-1, 7)      # one past LPI_EPI_RES_ROWSTATS = 5
REFUSED = (-22, -38)          # LPI_EINVAL, LPI_ENOSYS
PREDICATES = ("lpi_gemm_nt_rows_supported", "lpi_gemm_ln_supported", "lpi_gemm_mx8_ok", "lpi_gemm_mx8_256_ok")      # answer 1 / 0, launch nothing
DESC_FORMS = ("lpi_gemm_nt_grouped", "lpi_gemm_nt_rows")
# single tuning-key changes under which every good list is repeated: (key, value)
TUNINGS = ((0, 1 << 30), (1, 1), (2, -1), (2, 2), (4, 4), (5, 0), (6, 0), (8, 1), (14, 1), (15, -1), (15, 2), (15, 3))
PAIRS = ((F32, F32), (F32X3, F32), (BF16, BF16), (BF16, F32), (F16, F16), (F16, F32))      # the pairs with the three common epilogues; bf16 -> f16 beside them


def A(k):
    """the k-th made-up address: 4 KiB aligned, 16 MiB apart"""
    return 0x7E0000000000 + k * 0x1000000


def accepted(name, rc):
    """did the argument list pass the host checks?"""
    return rc == 1 if name in PREDICATES else rc not in REFUSED


# an argument: (name, kind, value[, width or tile]).  kinds: dt dtype code | epi epilogue code | p pointer | ld leading dimension of rows `width` wide |
# dim M, N or K with its tile | n count | a alpha | s: the NULL stream
def mutations(args):
    """(label, values) of every one-argument mutation of a good list"""
    for i, a in enumerate(args):
        name, kind, v = a[0], a[1], a[2]
        if kind == "dt":
            alt = list(DT_CODES)
        elif kind == "epi":
            alt = list(EPI_CODES)
        elif kind == "p":
            base = v or A(63)
            alt = ([0] if v else [base]) + [base + 2, base + 4, base + 8]
        elif kind == "ld":
            alt = [0, -1, a[3] - 4, v + 1, v + 2, v + 4, v + 8]
        elif kind == "dim":
            t = a[3]
            alt = [0, -1, v - t, v + t, v - t // 2, v + t // 2, v - t // 4, v + t // 4]
        elif kind == "n":
            alt = [0, 1, 2, 3]
        elif kind == "a":
            alt = [0.5 if v == 1.0 else 1.0]
        else:
            continue
        for m in dict.fromkeys(alt):
            if m != v:
                yield f"{name}={m if kind != 'p' else (m - (v or A(63)) if m else 'NULL')}", [x[2] for x in args[:i]] + [m] + [x[2] for x in args[i + 1:]]


S = ("stream", "s", None)


def prob(dt, cdt, epi, M, N, K, bias=0, res=0, aux=0, k=0, tile=256):
    """the fields of one lpi_gemm_desc, in its order.  Leading dimensions leave a tile and 16 elements of room, so that a grown M, N or K meets the shape rules
    and not its own row stride; ldr / ldaux count rows where the epilogue keeps per-row f32 values there (the LN block, the row statistics)."""
    bk = 32 if dt in (F32, F32X3) else 128 if dt == MX8 else 64
    o = k * 0x400000
    rw = M if epi in (LN, LN_QUICKGELU) else N
    aw = M if epi == RES_ROWSTATS else N
    return [("M", "dim", M, tile), ("N", "dim", N, tile), ("K", "dim", K, bk), ("A", "p", A(1) + o), ("lda", "ld", K + bk + 16, K), ("B", "p", A(2) + o), ("ldb", "ld", K + bk + 16, K),
            ("C", "p", A(3) + o), ("ldc", "ld", N + tile + 16, N), ("bias", "p", A(4) + o if bias else 0), ("residual", "p", A(5) + o if res else 0), ("ldr", "ld", rw + tile + 16, rw),
            ("aux", "p", A(6) + o if aux else 0), ("ldaux", "ld", aw + tile + 16, aw)]


def nt(dt, cdt, epi, M, N, K, alpha=1.0, **kw):
    """lpi_gemm_nt's argument list"""
    f = {x[0]: x for x in prob(dt, cdt, epi, M, N, K, **kw)}
    return [("dtype", "dt", dt), ("c_dtype", "dt", cdt)] + [f[n] for n in ("M", "N", "K", "A", "lda", "B", "ldb", "C", "ldc", "bias", "residual", "ldr")] + \
           [("epilogue", "epi", epi), f["aux"], f["ldaux"], ("alpha", "a", alpha), S]


def descs(dt, cdt, epi, probs, alpha=1.0):
    """lpi_gemm_nt_grouped's / lpi_gemm_nt_rows' argument list: the head, then the descriptors' fields as "<i>.<field>" """
    return [("dtype", "dt", dt), ("c_dtype", "dt", cdt), ("epilogue", "epi", epi), ("alpha", "a", alpha), ("count", "n", len(probs))] + \
           [(f"{i}.{x[0]}",) + tuple(x[1:]) for i, p in enumerate(probs) for x in p] + [S]


def mx(cdt, epi, M, N, K, bias=0, res=0):
    """lpi_gemm_nt_mx8's / lpi_gemm_nt_mx8_256's argument list"""
    f = {x[0]: x for x in prob(MX8, cdt, epi, M, N, K, bias, res)}
    return [("c_dtype", "dt", cdt), f["M"], f["N"], f["K"], f["A"], f["lda"], ("a_scales", "p", A(7)), ("ldas", "ld", K // 32 + 8, K // 32), f["B"], f["ldb"],
            ("b_scales", "p", A(8)), ("ldbs", "ld", K // 32 + 8, K // 32), f["C"], f["ldc"], ("c_scales", "p", A(9) if cdt == MX8 else 0), ("ldcs", "ld", N // 32 + 8, N // 32),
            f["bias"], f["residual"], f["ldr"], ("epilogue", "epi", epi), ("alpha", "a", 1.0), S]


def epilogue_lists(dt, cdt):
    """(label, epilogue, bias, residual, aux) of every epilogue the pair takes, with and without what it may carry"""
    if (dt, cdt) == (BF16, F16):
        return [(f"none bias={b} res", NONE, b, 1, 0) for b in (0, 1)]
    return [(f"none bias={b} res={r}", NONE, b, r, 0) for b in (0, 1) for r in (0, 1)] + [(f"quickgelu bias={b} aux={a}", QUICKGELU, b, 0, a) for b in (0, 1) for a in (0, 1)] + \
           [(f"dquickgelu bias={b}", DQUICKGELU, b, 0, 1) for b in (0, 1)]


# shapes that reach each kernel (256 CUs when no device answers): label, M, N, K, tile of M and N
SHAPES_2BYTE = (("128-tile", 128, 256, 128, 128), ("15 tiles", 1280, 768, 512, 256), ("256x128 16 tiles", 1024, 1024, 512, 256), ("256x128 159 tiles", 13568, 768, 512, 256),
                ("persistent 256 tiles", 4096, 4096, 512, 256), ("tail 639 tiles", 54528, 768, 768, 256), ("slices even", 8192, 2048, 1024, 256),
                ("slices odd", 8192, 2304, 768, 256))
MUTATED_SHAPES = ("256x128 16 tiles", "persistent 256 tiles", "1600 tiles")      # beside "128-tile"
SHAPES_4BYTE = (("128-tile", 128, 256, 128, 128), ("256 tiles", 4096, 4096, 256, 256), ("1600 tiles", 10240, 10240, 256, 256))


def entry_points():
    """name -> [(branch label, good argument list, mutate it?)]: every list is called as it is and under each of TUNINGS; the lists that differ from a mutated
    neighbour only by a bias, or by a shape that takes the same path through the checks, are not mutated again"""
    E = {}
    g = E.setdefault("lpi_gemm_nt", [])
    for dt, cdt in PAIRS + ((BF16, F16),):
        for sl, M, N, K, tile in (SHAPES_4BYTE if dt in (F32, F32X3) else SHAPES_2BYTE):
            for el, epi, b, r, a in epilogue_lists(dt, cdt):
                g.append((f"{NAMES[dt]}->{NAMES[cdt]} {sl} {el}", nt(dt, cdt, epi, M, N, K, bias=b, res=r, aux=a, tile=tile), sl == "128-tile" or (sl in MUTATED_SHAPES and not b)))
    for dt, cdt in ((F16, BF16), (F16, F16), (BF16, BF16)):      # the LN-fold pairs
        for sl, M, N, K in (("15 tiles", 1280, 768, 512), ("256 tiles", 4096, 4096, 512), ("tail 639 tiles", 54528, 768, 768)):
            g.append((f"{NAMES[dt]}->{NAMES[cdt]} {sl} ln", nt(dt, cdt, LN, M, N, K, bias=1, res=1), sl == "256 tiles"))
            g += [(f"{NAMES[dt]}->{NAMES[cdt]} {sl} ln_quickgelu aux={a}", nt(dt, cdt, LN_QUICKGELU, M, N, K, bias=1, res=1, aux=a), sl == "256 tiles") for a in (0, 1)]
    g.append(("f16->f16 128-tile ln", nt(F16, F16, LN, 128, 256, 128, bias=1, res=1, tile=128), True))      # no 256x256 shape: refused
    for dt in (BF16, F16):
        g += [(f"{NAMES[dt]}->f16 {sl} res_rowstats bias={b}", nt(dt, F16, RES_ROWSTATS, M, N, K, bias=b, res=1, aux=1), True) for sl, M, N, K in (("15 tiles", 1280, 768, 512), ("tail 639 tiles", 54528, 768, 768))
              for b in (0, 1)]

    g = E.setdefault("lpi_gemm_nt_grouped", [])
    big, small, short = (4096, 4096, 512), (2048, 1024, 512), (1792, 8192, 512)      # 256, 32 and 224 tiles; (7936, 256) = 31
    for dt, cdt in ((BF16, BF16), (BF16, F32), (F16, F16), (F16, F32), (BF16, F16), (F32, F32), (F32X3, F32)):
        for el, epi, b, r, a in epilogue_lists(dt, cdt):
            g.append((f"{NAMES[dt]}->{NAMES[cdt]} 256 + 32 tiles {el}", descs(dt, cdt, epi, [prob(dt, cdt, epi, *big, b, r, a), prob(dt, cdt, epi, *small, b, r, a, k=1)]), not b))
    g.append(("bf16 224 + 31 tiles none", descs(BF16, BF16, NONE, [prob(BF16, BF16, NONE, *short), prob(BF16, BF16, NONE, 7936, 256, 512, k=1)]), True))
    g.append(("bf16 224 + 32 tiles none", descs(BF16, BF16, NONE, [prob(BF16, BF16, NONE, *short), prob(BF16, BF16, NONE, *small, k=1)]), True))
    g.append(("bf16 side16 summed N 8704 dquickgelu", descs(BF16, BF16, DQUICKGELU, [prob(BF16, BF16, DQUICKGELU, 2048, 4352, 512, aux=1), prob(BF16, BF16, DQUICKGELU, 2048, 4352, 512, aux=1, k=1)]), True))
    g.append(("bf16 side16 summed N 8192 dquickgelu", descs(BF16, BF16, DQUICKGELU, [prob(BF16, BF16, DQUICKGELU, 2048, 4096, 512, aux=1), prob(BF16, BF16, DQUICKGELU, 2048, 4096, 512, aux=1, k=1)]), True))
    g.append(("bf16->f16 side16 summed N 8704 res", descs(BF16, F16, NONE, [prob(BF16, F16, NONE, 2048, 4352, 512, res=1), prob(BF16, F16, NONE, 2048, 4352, 512, res=1, k=1)]), True))
    for dt, cdt in ((F16, BF16), (F16, F16), (BF16, BF16)):
        g.append((f"{NAMES[dt]}->{NAMES[cdt]} 256 + 32 tiles ln", descs(dt, cdt, LN, [prob(dt, cdt, LN, *big, 1, 1), prob(dt, cdt, LN, *small, 1, 1, k=1)]), True))
        g += [(f"{NAMES[dt]}->{NAMES[cdt]} 256 + 32 tiles ln_quickgelu aux={a}", descs(dt, cdt, LN_QUICKGELU, [prob(dt, cdt, LN_QUICKGELU, *big, 1, 1, a), prob(dt, cdt, LN_QUICKGELU, *small, 1, 1, a, k=1)]), True)
              for a in (0, 1)]
    for dt in (BF16, F16):
        g.append((f"{NAMES[dt]}->f16 256 + 32 tiles res_rowstats", descs(dt, F16, RES_ROWSTATS, [prob(dt, F16, RES_ROWSTATS, *big, 1, 1, 1), prob(dt, F16, RES_ROWSTATS, *small, 1, 1, 1, k=1)]), True))
    g.append(("bf16 one problem", descs(BF16, BF16, NONE, [prob(BF16, BF16, NONE, *big)]), True))
    g.append(("bf16 three problems", descs(BF16, BF16, NONE, [prob(BF16, BF16, NONE, *big), prob(BF16, BF16, NONE, *small, k=1), prob(BF16, BF16, NONE, 128, 256, 128, k=2, tile=128)]), True))

    g = E.setdefault("lpi_gemm_nt_rows", [])
    for dt, cdt in ((F32, F32), (BF16, BF16), (BF16, F32), (F16, F16), (F16, F32)):
        for el, epi, b, r, a in epilogue_lists(dt, cdt):
            for n in (1, 2):
                g.append((f"{NAMES[dt]}->{NAMES[cdt]} count {n} {el}", descs(dt, cdt, epi, [prob(dt, cdt, epi, 64, 96, 256, b, r, a, k=i, tile=32) for i in range(n)]), not b and (n == 2 or epi == NONE)))

    shape = lambda M, N, K, tile, bk: [("M", "dim", M, tile), ("N", "dim", N, tile), ("K", "dim", K, bk)]      # noqa: E731
    E["lpi_gemm_nt_rows_supported"] = [(NAMES[dt], [("dtype", "dt", dt)] + shape(64, 96, 256, 32, 32 if dt == F32 else 64), True) for dt in (F32, BF16, F16)]
    E["lpi_gemm_ln_supported"] = [(NAMES[dt], [("dtype", "dt", dt)] + shape(1280, 768, 512, 256, 64), True) for dt in (BF16, F16)]
    E["lpi_gemm_mx8_ok"] = [("shape", shape(256, 384, 256, 128, 128), True)]
    E["lpi_gemm_mx8_256_ok"] = [("shape", shape(512, 768, 512, 256, 128), True)]
    for name, (M, N, K) in (("lpi_gemm_nt_mx8", (256, 384, 256)), ("lpi_gemm_nt_mx8_256", (512, 768, 512))):
        g = E.setdefault(name, [])
        for cdt in (F32, BF16, F16, MX8):
            g += [(f"->{NAMES[cdt]} {'quickgelu' if epi else 'none'} bias={b}", mx(cdt, epi, M, N, K, b), True) for epi in (NONE, QUICKGELU) for b in (0, 1)]
            if cdt in (F32, F16):
                g.append((f"->{NAMES[cdt]} none res", mx(cdt, NONE, M, N, K, 1, 1), True))
    return E


def _call(lib, name, names, values, tuning):
    """one call: descriptor fields ("<i>.<field>") go into a real array of four lpi_gemm_desc (the ones the list does not give repeat the last given, so a
    grown count reads host memory that is there); the tuning keys hold for this call alone"""
    head, fields = [], {}
    for k, v in zip(names, values):
        if name in DESC_FORMS and "." in k:
            fields.setdefault(int(k.split(".")[0]), []).append((k.split(".")[1], v))
        else:
            head.append(v)
    if name in DESC_FORMS:
        arr = (_lib.GemmDesc * 4)()
        for i in range(4):
            for f, v in fields[min(i, len(fields) - 1)]:
                setattr(arr[i], f, (v or None) if f in _PTR_FIELDS else v)
        head = head[:-1] + [ctypes.cast(arr, ctypes.c_void_p)] + head[-1:]      # ... descriptors, stream
    old = {k: lib.lpi_get_tuning(k) for k in tuning}
    for k, v in tuning.items():
        assert lib.lpi_set_tuning(k, v) == 0
    try:
        return getattr(lib, name)(*head)
    finally:
        for k, v in old.items():
            assert lib.lpi_set_tuning(k, v) == 0


_PTR_FIELDS = {"A", "B", "C", "bias", "residual", "aux"}


def cases():
    """[(entry point, tuple label, thunk)]: the thunk calls the library once and returns its code"""
    lib = _lib.load()
    out = []
    for name, branches in entry_points().items():
        for branch, args, mutate in branches:
            names = [a[0] for a in args]
            good = [a[2] for a in args]
            run = lambda v, t={}, name=name, names=names: _call(lib, name, names, v, t)      # noqa: E731
            out.append((name, f"{branch}: good", (lambda v=good, run=run: run(v))))
            if name not in PREDICATES:
                for k, val in TUNINGS:
                    out.append((name, f"{branch} key {k}={val}: good", (lambda v=good, run=run, t={k: val}: run(v, t))))
            for label, v in mutations(args) if mutate else ():
                out.append((name, f"{branch}: {label}", (lambda v=v, run=run: run(v))))
    for name in DESC_FORMS:
        out.append((name, "NULL descriptors", (lambda fn=getattr(lib, name): fn(BF16, BF16, NONE, 1.0, 2, None, None))))
    return out


def reset(lib):
    """lpi_gemm_last_kernel back to a known value (LPI_GEMM_K_ROWS) through an ordinary call: one few-row problem"""
    d = (_lib.GemmDesc * 1)()
    for f, v in (("M", 32), ("N", 32), ("K", 64), ("A", A(1)), ("lda", 64), ("B", A(2)), ("ldb", 64), ("C", A(3)), ("ldc", 32)):
        setattr(d[0], f, v)
    rc = lib.lpi_gemm_nt_rows(BF16, BF16, NONE, 1.0, 1, ctypes.cast(d, ctypes.c_void_p), None)
    assert rc not in REFUSED and lib.lpi_gemm_last_kernel() == _lib.GEMM_K_ROWS, rc


def run_one(lib, thunk):
    """[code, launches, last kernel, last grouped] of one tuple"""
    reset(lib)
    n0 = _lib.launch_count()
    rc = int(thunk())
    return [rc, _lib.launch_count() - n0, lib.lpi_gemm_last_kernel(), lib.lpi_gemm_last_grouped()]


LETTERS = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"


def branch_of(label):
    """the good list a tuple belongs to: its label without the tuning key and the mutation"""
    return label.split(":")[0].split(" key ")[0]


def load_record():
    """(recorded_from, {entry point: [[code, launches, last kernel, last grouped] per tuple, in the order of cases()]})"""
    with open(EXPECTED) as f:
        rec = json.load(f)
    src, outcomes = rec.pop("recorded_from"), rec.pop("outcomes")
    return src, {name: [outcomes[ch] for s in lists for ch in s] for name, lists in rec.items()}


def _lines(strings, width=280):
    """the strings as JSON list items, several short ones to a line"""
    out = []
    for s in strings:
        if out and len(out[-1]) + len(s) + 4 <= width:
            out[-1] += f', "{s}"'
        else:
            out.append(f'  "{s}"')
    return out


def main():
    import torch
    assert torch.cuda.device_count() == 0, "record on a machine without a GPU: the accepted lists would launch on made-up addresses"
    assert len(sys.argv) == 2, "usage: LPI_LIB=<library of the commit to record> python3 tests/gemm_args.py <hash of that commit>"
    lib = _lib.load()
    cs = cases()
    res = [run_one(lib, thunk) for _, _, thunk in cs]
    # the file: the distinct outcomes once, then per entry point one string per good list — a letter per tuple (the list itself, its tuning keys, its mutations)
    outcomes = sorted({tuple(r) for r in res})
    assert len(outcomes) <= len(LETTERS)
    rec, last = {}, None
    for (name, label, _), r in zip(cs, res):
        if (name, branch_of(label)) != last:
            rec.setdefault(name, []).append("")
            last = (name, branch_of(label))
        rec[name][-1] += LETTERS[outcomes.index(tuple(r))]
    with open(EXPECTED, "w") as f:
        f.write('{\n "recorded_from": ' + json.dumps(sys.argv[1] + " + each lpi_note_gemm_kernel moved ahead of its lpi_ensure_lds") + ",\n" +
                ' "outcomes": {' + ", ".join(f'"{LETTERS[i]}": {json.dumps(list(o))}' for i, o in enumerate(outcomes)) + "},\n" +
                ",\n".join(f' "{k}": [\n' + ",\n".join(_lines(v)) + "\n ]" for k, v in rec.items()) + "\n}\n")
    acc = sum(1 for (name, _, _), r in zip(cs, res) if accepted(name, r[0]))
    print(f"{len(cs)} tuples of {len(rec)} names recorded from {_lib.LIB_PATH}: {acc} accepted, {len(cs) - acc} refused")


if __name__ == "__main__":
    main()
