"""The argument grid of the attention family's HOST layer (lpi_amd/csrc/attention.hip, attn_pooled.hip, attn_hd.hip, and through them attention4.hip and
attn_long.hip): which argument lists each entry point accepts, and which it refuses before any launch.

The host code of this family never dereferences an operand pointer (descriptors and the `lay` array of lpi_attn_bwd_layout are host memory and are real here),
so the whole accept set can be observed with made-up addresses, as tests/rowop_args.py does for the row operations: a refused call returns LPI_EINVAL /
LPI_ENOSYS and lpi_launch_count() stays; an accepted call gets as far as the runtime, which, without a device, answers with its no-device code (100) — from
the LDS set-up of the kernels that need more than 64 KiB (no launch counted), or from the launch itself (counted).  cases() builds a deterministic grid: one
good argument list per dispatch branch (each dtype; causal or not; uniform, ragged, shared prefix; L = 50, 200, 224, 273, 288, 289, 600, 1024; an explicit
layout; tuning keys 3 = 1, 7 = 1, 7 = 5, 13 = 1, set for the one call and restored; head widths 80, 88, 104), then every argument mutated one at a time
(pointers NULL / +2 / +4 / +8 bytes; leading dimensions and counts 0, -1, width - 4, +1, +2, +4, +6; every dtype code from -1 to one past the largest of the
header; L 0, 1, 288, 289, 1024, 1025; shared_rows and rows_needed 0, -1, L - 1, L, L + 1; each layout stride 0, -8, +4; causal flipped; head_dim over the
multiples of 8 around the built ones).  tests/test_attn_args_host.py replays it against the built library.

Run as a script WITHOUT a GPU, this records (return code, launches) per tuple into tests/attn_args_expected.json:
    LPI_LIB=<build of the commit to record>/liblpi_hip.so python3 tests/attn_args.py <hash of that commit>
The committed record is that of the library before the host layer moved onto one call struct, the shared predicates and the typed dispatch
(lpi_amd/csrc/dispatch.h), with lpi_ensure_lds's no-device return code (common.h) as its only change.
"""
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from lpi_amd import _lib  # noqa: E402

EXPECTED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "attn_args_expected.json")
F32, BF16, F16 = 0, 1, 2
DTS = (("f32", F32), ("bf16", BF16), ("f16", F16))
DT_CODES = range(-1, 7)      # one past LPI_MX4 = 5
REFUSED = (-22, -38)         # LPI_EINVAL, LPI_ENOSYS
B, H = 2, 2


def A(k):
    """the k-th made-up address: 4 KiB aligned, 16 MiB apart"""
    return 0x7E0000000000 + k * 0x1000000


def accepted(name, rc):
    """did the argument list pass the host checks?  (lpi_attn_hd_supported answers 1 / 0 and launches nothing)"""
    return rc == 1 if name == "lpi_attn_hd_supported" else rc not in REFUSED


# an argument: (name, kind, value[, width]).  kinds: dt dtype code | p pointer | ld leading dimension of rows `width` wide | n count | L sequence length |
# sr shared_rows / rows_needed (edges from the list's own L) | st layout stride | c causal flag | hd head width | layp "the lay array is given" |
# i, s: passed as they are (flags, the NULL stream)
def mutations(args):
    """(label, values) of every one-argument mutation of a good list"""
    val = {a[0]: a[2] for a in args}
    for i, a in enumerate(args):
        name, kind, v = a[0], a[1], a[2]
        L = val.get(name[:name.rfind(".") + 1] + "L")      # "<i>." of a descriptor's field: its own L
        if kind == "dt":
            alt = list(DT_CODES)
        elif kind == "p":
            base = v or A(63)
            alt = ([0] if v else [base]) + [base + 2, base + 4, base + 8]
        elif kind == "ld":
            alt = [0, -1, a[3] - 4, v + 1, v + 2, v + 4, v + 6]
        elif kind == "n":
            alt = [0, -1, v + 1, v + 2, v + 4, v + 6]
        elif kind == "L":
            alt = [0, 1, 288, 289, 1024, 1025]
        elif kind == "sr":
            alt = [0, -1, L - 1, L, L + 1]
        elif kind == "st":
            alt = [0, -8, v + 4]
        elif kind == "c":
            alt = [1 - v]
        elif kind == "hd":
            alt = [0, 64, 72, 80, 88, 96, 104, 112]
        elif kind == "layp":
            alt = [0]
        else:
            continue
        for m in dict.fromkeys(alt):
            if m != v:
                yield f"{name}={m if kind != 'p' else (m - (v or A(63)) if m else 'NULL')}", [x[2] for x in args[:i]] + [m] + [x[2] for x in args[i + 1:]]


def P_(name, k, null=False):
    return (name, "p", 0 if null else A(k))


S = ("stream", "s", None)


def fwd(dt, L, causal=0, rs=False, shared=None, hd=None):
    """lpi_attn_fwd / _varlen / _shared / lpi_attn_hd_fwd"""
    w = H * (hd or 64)
    a = [("dtype", "dt", dt), ("B", "n", B), ("L", "L", L)]
    if rs is not None:
        a += [P_("row_start", 9, not rs)]
    if shared is not None:
        a += [("shared_rows", "sr", shared)]
    a += [("H", "n", H)] + ([("head_dim", "hd", hd)] if hd else []) + [P_("qkv", 1), ("ldqkv", "ld", 3 * w + 8, 3 * w), P_("ctx", 2), ("ldctx", "ld", w + 8, w), P_("lse", 3)]
    return a + ([("causal", "c", causal)] if shared is None and not hd else [])


def bwd(dt, L, causal=0, rs=False, shared=None, rows=None, hd=None, lay=None):
    """lpi_attn_bwd / _varlen / _prefix / _shared / _layout / lpi_attn_hd_bwd"""
    w = H * (hd or 64)
    a = [("dtype", "dt", dt), ("B", "n", B), ("L", "L", L)]
    if rs is not None:
        a += [P_("row_start", 9, not rs)]
    if shared is not None:
        a += [("shared_rows", "sr", shared)]
    if rows is not None:
        a += [("rows_needed", "sr", rows)]
    a += [("H", "n", H)] + ([("head_dim", "hd", hd)] if hd else [])
    lw, cw = (64, 64) if lay else (3 * w, w)      # an explicit layout: every leading dimension >= 64
    a += [P_("qkv", 1), ("ldqkv", "ld", 3 * w + 8, lw), P_("ctx", 2), ("ldctx", "ld", w + 8, cw), P_("dctx", 4), ("lddctx", "ld", w + 16, cw), P_("lse", 3), P_("delta", 5),
          P_("dqkv", 6), ("lddqkv", "ld", 3 * w + 16, lw)]
    if shared is not None:
        a += [P_("shared_dkv", 7)]
    if lay:
        a += [("lay", "layp", 1)] + [(f"lay.{i}", "st", v) for i, v in enumerate(lay)]
    return a + ([("causal", "c", causal)] if shared is None and not hd and not lay else [])


def fdesc(L, causal=0, rs=False, shared=0, lay=None, k=0):
    """the fields of one lpi_attn_fwd_desc"""
    w, o = H * 64, k * 0x400000
    return [("B", "n", B), ("L", "L", L), ("H", "n", H), ("row_start", "p", 0 if not rs else A(9) + o), ("qkv", "p", A(1) + o), ("ldqkv", "ld", 3 * w + 8, 64 if lay else 3 * w),
            ("ctx", "p", A(2) + o), ("ldctx", "ld", w + 8, 64 if lay else w), ("lse", "p", A(3) + o), ("causal", "c", causal), ("shared_rows", "sr", shared),
            ("qkv_hs", "st", lay[0] if lay else 0), ("qkv_vs", "st", lay[1] if lay else 0), ("ctx_hs", "st", lay[2] if lay else 0)]


def pdesc(L, causal=0, rs=False, shared=0, k=0, backward=False):
    """the fields of one lpi_attn_pooled_desc: the forward's or the backward's (the others stay zero)"""
    w, o = H * 64, k * 0x400000
    a = [("B", "n", B), ("L", "L", L), ("H", "n", H), ("row_start", "p", 0 if not rs else A(9) + o), ("q", "p", A(1) + o), ("ldq", "ld", w + 8, w), ("qkv", "p", A(2) + o),
         ("ldqkv", "ld", 3 * w + 8, 3 * w), ("idx", "p", A(3) + o)]
    if backward:
        a += [("lse", "p", A(5) + o), ("dctx", "p", A(6) + o), ("lddctx", "ld", w + 16, w), ("dq", "p", A(7) + o), ("lddq", "ld", w + 24, w), ("dqkv", "p", A(8) + o),
              ("lddqkv", "ld", 3 * w + 16, 3 * w)]
    else:
        a += [("ctx", "p", A(4) + o), ("ldctx", "ld", w + 8, w), ("lse", "p", A(5) + o)]
    a += [("causal", "c", causal), ("shared_rows", "sr", shared)]
    return a + ([("shared_dkv", "p", A(10) + o if shared else 0)] if backward else [])


def pooled(dt, L, causal, rs, backward):
    """lpi_attn_pooled_fwd / _bwd and their _varlen forms: the descriptor's fields in the order of the argument list"""
    d = {x[0]: x for x in pdesc(L, causal, bool(rs), backward=backward)}
    order = ["B", "L"] + (["row_start"] if rs is not None else []) + ["H", "q", "ldq", "qkv", "ldqkv", "idx"] + \
            (["dctx", "lddctx", "lse", "dq", "lddq", "dqkv", "lddqkv"] if backward else ["ctx", "ldctx", "lse"]) + ["causal"]
    return [("dtype", "dt", dt)] + [d[k] for k in order]


def pair(a, b):
    """two lists -> one, names prefixed by the descriptor index"""
    return [(f"{i}.{x[0]}",) + tuple(x[1:]) for i, l in enumerate((a, b)) for x in l]


PLANES = (200 * 64, H * 200 * 64, 200 * 64)      # head-blocked planes at L = 200 (include/lpi_hip.h, lpi_attn_fwd_desc): qkv_hs, qkv_vs, ctx_hs


def entry_points():
    """name -> [(branch label, good argument list, {tuning key: value})]"""
    E = {}
    T0 = {}
    E["lpi_attn_fwd"] = [(f"{n} L=50 causal={c}", fwd(dt, 50, c, None), T0) for n, dt in DTS for c in (0, 1)] + \
                        [(f"{n} L={L}", fwd(dt, L, 0, None), T0) for n, dt in DTS for L in (200, 224, 273, 288, 289, 600, 1024)] + \
                        [("bf16 L=288 causal", fwd(BF16, 288, 1, None), T0), ("bf16 L=273 key 13", fwd(BF16, 273, 0, None), {13: 1})]
    E["lpi_attn_fwd_varlen"] = [(f"{n} ragged causal={c}", fwd(dt, 50, c, True), T0) for n, dt in DTS for c in (0, 1)] + \
                               [("bf16 ragged L=273", fwd(BF16, 273, 0, True), T0), ("bf16 uniform L=600", fwd(BF16, 600, 0, False), T0)]
    E["lpi_attn_fwd_shared"] = [(f"{n} L={L}", fwd(dt, L, 1, True, 17), T0) for n, dt in DTS for L in (50, 288)]
    E["lpi_attn_bwd"] = [(f"{n} L=50 causal={c}", bwd(dt, 50, c, None), T0) for n, dt in DTS for c in (0, 1)] + \
                        [(f"{n} L={L}", bwd(dt, L, 0, None), T0) for n, dt in DTS for L in (200, 224, 273, 288, 289, 600, 1024)] + \
                        [(f"{n} L={L} key {k}={v}", bwd(dt, L, 0, None), {k: v}) for n, dt in DTS[1:] for L, k, v in ((200, 3, 1), (200, 7, 1), (50, 7, 5), (273, 3, 1), (288, 7, 5))] + \
                        [("bf16 L=288 causal", bwd(BF16, 288, 1, None), T0)]
    E["lpi_attn_bwd_varlen"] = [(f"{n} ragged causal={c}", bwd(dt, 50, c, True), T0) for n, dt in DTS for c in (0, 1)] + \
                               [("bf16 ragged L=200", bwd(BF16, 200, 0, True), T0), ("f16 uniform L=200", bwd(F16, 200, 0, False), T0)]
    E["lpi_attn_bwd_prefix"] = [(f"{n} L={L} rows 9", bwd(dt, L, 0, False, rows=9), T0) for n, dt in DTS for L in (50, 200, 273, 600)] + \
                               [("bf16 ragged causal rows 9", bwd(BF16, 50, 1, True, rows=9), T0), ("bf16 L=200 rows 9 key 3", bwd(BF16, 200, 0, False, rows=9), {3: 1})]
    E["lpi_attn_bwd_shared"] = [(f"{n} L={L}", bwd(dt, L, 1, True, 17, 30), T0) for n, dt in DTS for L in (50, 288)] + [("bf16 key 3", bwd(BF16, 50, 1, True, 17, 30), {3: 1})]
    E["lpi_attn_bwd_layout"] = [(f"{n} L={L}", bwd(dt, L, rs=None, rows=0, lay=(64, 128, 64, 128, 64, 64)), T0) for n, dt in DTS[1:] for L in (50, 200, 273, 288)] + \
                               [(f"bf16 L={L} key {k}={v}", bwd(BF16, L, rs=None, rows=9, lay=(64, 128, 64, 128, 64, 64)), {k: v}) for L, k, v in ((200, 3, 1), (200, 7, 1), (50, 7, 5))] + \
                               [("bf16 planes L=200", bwd(BF16, 200, rs=None, rows=0, lay=PLANES[:2] * 2 + (PLANES[2],) * 2), T0)]
    E["lpi_shared_kv_reduce"] = [(n, [("dtype", "dt", dt), ("B", "n", B), ("shared_rows", "n", 17), ("H", "n", H), P_("partial", 1), P_("dqkv", 2), ("lddqkv", "ld", 3 * H * 64 + 16, 3 * H * 64),
                                      ("accumulate", "i", 1)], T0) for n, dt in DTS]
    for hd in (80, 88, 104):
        E.setdefault("lpi_attn_hd_fwd", []).extend((f"{n} head_dim={hd} L={L}", fwd(dt, L, rs=None, hd=hd), T0) for n, dt in DTS for L in (50, 600))
        E.setdefault("lpi_attn_hd_bwd", []).extend((f"{n} head_dim={hd} L={L}", bwd(dt, L, rs=None, hd=hd), T0) for n, dt in DTS for L in (50, 600))
        E.setdefault("lpi_attn_hd_supported", []).append((f"head_dim={hd}", [("L", "L", 257), ("H", "n", 16), ("head_dim", "hd", hd)], T0))
    for back in (False, True):
        d = "bwd" if back else "fwd"
        E[f"lpi_attn_pooled_{d}"] = [(f"{n} causal={c}", pooled(dt, 50, c, None, back), T0) for n, dt in DTS for c in (0, 1)] + [("bf16 L=1024", pooled(BF16, 1024, 0, None, back), T0)]
        E[f"lpi_attn_pooled_{d}_varlen"] = [(f"{n} ragged", pooled(dt, 50, 1, True, back), T0) for n, dt in DTS] + [("bf16 uniform", pooled(BF16, 200, 0, False, back), T0)]
    return {k: [(n, a + ([] if k == "lpi_attn_hd_supported" else [S]), t) for n, a, t in v] for k, v in E.items()}


def desc_entry_points():
    """name -> [(branch label, [dtype] + the fields of its descriptor(s), {tuning key: value})]"""
    D = {}
    T0 = {}
    DT = lambda dt: [("dtype", "dt", dt)]      # noqa: E731
    one = lambda a: [("0." + x[0],) + tuple(x[1:]) for x in a]      # noqa: E731
    D["lpi_attn_fwd_pair"] = [(f"{n} vision + text", DT(dt) + pair(fdesc(200), fdesc(50, 1, True, k=1)), T0) for n, dt in DTS] + \
                             [(f"{n} L=273 + text", DT(dt) + pair(fdesc(273), fdesc(77, 1, True, k=1)), T0) for n, dt in DTS[1:]] + \
                             [("bf16 L=273 + text key 13", DT(BF16) + pair(fdesc(273), fdesc(77, 1, True, k=1)), {13: 1}),
                              ("bf16 causal + causal", DT(BF16) + pair(fdesc(77, 1), fdesc(77, 1, k=1)), T0), ("bf16 causal + not", DT(BF16) + pair(fdesc(77, 1), fdesc(50, 0, k=1)), T0),
                              ("bf16 not + not", DT(BF16) + pair(fdesc(288), fdesc(50, 0, k=1)), T0),
                              ("bf16 vision + shared prefix", DT(BF16) + pair(fdesc(200), fdesc(50, 1, True, 17, k=1)), T0),
                              ("f32 vision + shared prefix", DT(F32) + pair(fdesc(200), fdesc(50, 1, True, 17, k=1)), T0),
                              ("bf16 L=600 + text", DT(BF16) + pair(fdesc(600), fdesc(50, 1, True, k=1)), T0),
                              ("f16 planes + text", DT(F16) + pair(fdesc(200, lay=PLANES), fdesc(50, 1, True, k=1)), T0)]
    D["lpi_attn_fwd_one"] = [(f"{n} uniform", DT(dt) + one(fdesc(200)), T0) for n, dt in DTS] + \
                            [("bf16 ragged causal", DT(BF16) + one(fdesc(50, 1, True)), T0), ("bf16 shared prefix", DT(BF16) + one(fdesc(50, 1, True, 17)), T0),
                             ("bf16 L=600", DT(BF16) + one(fdesc(600)), T0), ("bf16 planes", DT(BF16) + one(fdesc(200, lay=PLANES)), T0),
                             ("f16 planes L=273", DT(F16) + one(fdesc(273, lay=(273 * 64, H * 273 * 64, 273 * 64))), T0)]
    for back in (False, True):
        d = "bwd" if back else "fwd"
        D[f"lpi_attn_pooled_{d}_pair"] = [(f"{n} vision + text", DT(dt) + pair(pdesc(200, backward=back), pdesc(50, 1, True, k=1, backward=back)), T0) for n, dt in DTS] + \
                                         [(f"{n} vision + shared prefix", DT(dt) + pair(pdesc(200, backward=back), pdesc(50, 1, True, 17, k=1, backward=back)), T0) for n, dt in DTS]
        D[f"lpi_attn_pooled_{d}_desc"] = [(f"{n} ragged", DT(dt) + one(pdesc(50, 1, True, backward=back)), T0) for n, dt in DTS] + \
                                         [(f"{n} shared prefix", DT(dt) + one(pdesc(50, 1, True, 17, backward=back)), T0) for n, dt in DTS] + \
                                         [("bf16 uniform L=1024", DT(BF16) + one(pdesc(1024, backward=back)), T0)]
    return D


_DESCS = {"lpi_attn_fwd_pair": _lib.AttnFwdDesc, "lpi_attn_fwd_one": _lib.AttnFwdDesc, "lpi_attn_pooled_fwd_pair": _lib.AttnPooledDesc, "lpi_attn_pooled_bwd_pair": _lib.AttnPooledDesc,
          "lpi_attn_pooled_fwd_desc": _lib.AttnPooledDesc, "lpi_attn_pooled_bwd_desc": _lib.AttnPooledDesc}


def _call(lib, fn, names, values, cls, tuning):
    """one call: descriptor fields ("<i>.<field>") and the lay array ("lay.<i>") go into real host memory; the tuning keys hold for this call alone"""
    head, lay, fields = [], [], {}
    for k, v in zip(names, values):
        if k.startswith("lay."):
            lay.append(v)
        elif cls is not None and "." in k:
            fields.setdefault(int(k.split(".")[0]), []).append((k.split(".")[1], v))
        else:
            head.append(v)
    if lay:
        arr = (ctypes.c_int32 * 6)(*lay)
        i = names.index("lay")
        head[i] = ctypes.cast(arr, ctypes.c_void_p) if head[i] else None
    if cls is not None:
        descs = (cls * len(fields))()
        for i, fs in fields.items():
            for f, v in fs:
                setattr(descs[i], f, (v or None) if f in _PTR_FIELDS else v)
        head = head[:-1] + [ctypes.cast(descs, ctypes.c_void_p)] + head[-1:]      # ... descriptors, stream
    old = {k: lib.lpi_get_tuning(k) for k in tuning}
    for k, v in tuning.items():
        assert lib.lpi_set_tuning(k, v) == 0
    try:
        return fn(*head)
    finally:
        for k, v in old.items():
            assert lib.lpi_set_tuning(k, v) == 0


_PTR_FIELDS = _lib._POOLED_PTRS | {"row_start", "qkv", "ctx", "lse"}


def cases():
    """[(entry point, tuple label, thunk)]: the thunk calls the library once and returns its code"""
    lib = _lib.load()
    out = []
    for table, desc in ((entry_points(), False), (desc_entry_points(), True)):
        for name, branches in table.items():
            fn, cls = getattr(lib, name), _DESCS[name] if desc else None
            for branch, args, tuning in branches:
                if desc:
                    args = args + [S]
                names = [a[0] for a in args]
                run = lambda v, fn=fn, names=names, cls=cls, tuning=tuning: _call(lib, fn, names, v, cls, tuning)      # noqa: E731
                out.append((name, f"{branch}: good", (lambda v=[a[2] for a in args], run=run: run(v))))
                for label, v in mutations(args):
                    out.append((name, f"{branch}: {label}", (lambda v=v, run=run: run(v))))
    for name in _DESCS:
        out.append((name, "NULL descriptors", (lambda fn=getattr(lib, name): fn(BF16, None, None))))
    return out


def run(case_list):
    """[(code, launches)] of the tuples, in order"""
    res = []
    for _, _, thunk in case_list:
        n0 = _lib.launch_count()
        rc = int(thunk())
        res.append([rc, _lib.launch_count() - n0])
    return res


def main():
    import torch
    assert torch.cuda.device_count() == 0, "record on a machine without a GPU: the accepted lists would launch on made-up addresses"
    assert len(sys.argv) == 2, "usage: LPI_LIB=<library of the commit to record> python3 tests/attn_args.py <hash of that commit>"
    cs = cases()
    res = run(cs)
    rec = {}
    for (name, _, _), r in zip(cs, res):
        rec.setdefault(name, []).append(r)
    with open(EXPECTED, "w") as f:
        f.write('{\n "recorded_from": ' + json.dumps(sys.argv[1] + " + the no-device return code of lpi_ensure_lds") + ",\n" +
                ",\n".join(f' "{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in rec.items()) + "\n}\n")
    acc = sum(1 for (name, _, _), r in zip(cs, res) if accepted(name, r[0]))
    print(f"{len(cs)} tuples of {len(rec)} names recorded from {_lib.LIB_PATH}: {acc} accepted, {len(cs) - acc} refused")


if __name__ == "__main__":
    main()
