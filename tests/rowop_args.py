"""The argument grid of the row-operation family's HOST layer (lpi_amd/csrc/rowops.hip, mx8_rows.hip): which argument lists each entry point and each
lpi_row_jobs op accepts, and which it refuses before any launch.

The host code of this family never dereferences an operand pointer, so the whole accept set can be observed with made-up addresses: a refused call returns
LPI_EINVAL / LPI_ENOSYS and lpi_launch_count() stays; an accepted call counts its launch(es) (without a device every launch then fails with HIP's
no-device code).  cases() builds a deterministic grid: one good argument list per dispatch branch of every entry point, then every argument mutated one at
a time (pointers NULL / +2 / +4 / +8 bytes; leading dimensions and counts 0, -1, width - 4, +1, +2, +4, +6; d 0, 2, 2048, 2052; every dtype argument each
code from -1 to one past the largest of the header; P, row0 and L to their edges).  tests/test_rowop_args_host.py replays it against the built library.

Run as a script WITHOUT a GPU, this records (return code, launches) per tuple into tests/rowop_args_expected.json:
    LPI_LIB=<build of the commit to record>/liblpi_hip.so python3 tests/rowop_args.py
The committed record is that of the library before the host layer moved onto the typed dispatch (lpi_amd/csrc/dispatch.h) and the shared per-op predicates.
"""
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from lpi_amd import _lib  # noqa: E402

EXPECTED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rowop_args_expected.json")
F32, BF16, F16 = 0, 1, 2
DT_CODES = range(-1, 6)      # one past LPI_F32X3 = 4
EXEMPT = {"lpi_rowstat_guard"}      # asks the runtime about its pointer


def A(k):
    """the k-th made-up address: 4 KiB aligned, 16 MiB apart"""
    return 0x7E0000000000 + k * 0x1000000


# an argument: (name, kind, value[, width]).  kinds: dt dtype code | p pointer | ld leading dimension of rows `width` wide | n count | d row width |
# P, row0, L rows of a sample (edges from the list's own L / P / row0) | l long stride | i, f, s: passed as they are (flags, floats, the NULL stream)
def mutations(args):
    """(label, values) of every one-argument mutation of a good list"""
    val = {a[0]: a[2] for a in args}
    for i, a in enumerate(args):
        name, kind, v = a[0], a[1], a[2]
        pre = name[:name.rfind(".") + 1]      # "<i>." of a descriptor's field: its own L / P / row0
        L, P, r0 = val.get(pre + "L"), val.get(pre + "P"), val.get(pre + "row0", 0)
        if kind == "dt":
            alt = [c for c in DT_CODES if c != v]
        elif kind == "p":
            base = v or A(63)
            alt = ([0] if v else [base]) + [base + 2, base + 4, base + 8]
        elif kind == "ld":
            alt = [0, -1, a[3] - 4, v + 1, v + 2, v + 4, v + 6]
        elif kind == "n":
            alt = [0, -1, v + 1, v + 2, v + 4, v + 6]
        elif kind == "d":
            alt = [0, 2, 2048, 2052]
        elif kind == "l":
            alt = [0, v + 1, v + 2, v + 4]
        elif kind == "P":
            alt = [0, -1, 1] + ([L, L - r0, L - r0 + 1] if L is not None else [])
        elif kind == "row0":
            alt = [-1, 0, L - P, L - P + 1, L]
        elif kind == "L":
            alt = [0, -1, 1, r0 + (P or 0), r0 + (P or 0) - 1, (P or 0) + 1]
        else:
            continue
        for m in dict.fromkeys(alt):
            if m != v:
                yield f"{name}={m if kind != 'p' else (m - (v or A(63)) if m else 'NULL')}", [x[2] for x in args[:i]] + [m] + [x[2] for x in args[i + 1:]]


def P_(name, k, null=False):
    return (name, "p", 0 if null else A(k))


S = ("stream", "s", None)


def ln_fwd(dt, xdt, d, ld, y=True, rows=10):
    return [("dtype", "dt", dt), ("x_dtype", "dt", xdt), ("rows", "n", rows), ("d", "d", d), P_("x", 1), ("ldx", "ld", ld, d), P_("gamma", 2), P_("beta", 3),
            P_("y", 4, not y), ("ldy", "ld", ld if y else 0, d), P_("mean", 5), P_("rstd", 6)]


def ln_bwd(dydt, cdt, xdt, d, ld, dx=True, cast=True, rows=10):
    return [("dy_dtype", "dt", dydt), ("cast_dtype", "dt", cdt), ("x_dtype", "dt", xdt), ("rows", "n", rows), ("d", "d", d), P_("dy", 1), ("lddy", "ld", ld, d),
            P_("x", 2), ("ldx", "ld", ld, d), P_("gamma", 3), P_("mean", 4), P_("rstd", 5), P_("dx", 6, not dx), ("lddx", "ld", ld, d), P_("dx_cast", 7, not cast),
            ("ldcast", "ld", ld, d), ("accumulate", "i", 1)]


def ln_bwd_rows(dydt, cdt, xdt, d, ld, dx, varlen, rs=False):
    a = ln_bwd(dydt, cdt, xdt, d, ld, dx)
    head = a[:3] + [("B", "n", 3), ("L", "L", 9)] + ([P_("row_start", 8, not rs)] if varlen else []) + [("row0", "row0", 2), ("P", "P", 4)]
    return head + a[4:]


LN_D = (264, 520, 776, 1032)      # one width in each of the NC = 2, 3, 4, 8 ranges (132 and 136: NC = 1)


def entry_points():
    """name -> list of (branch label, good argument list without the stream)"""
    E = {}
    E["lpi_layernorm_fwd"] = [("f32", ln_fwd(F32, F32, 132, 140)), ("f32->bf16", ln_fwd(BF16, F32, 132, 140)), ("f32->f16", ln_fwd(F16, F32, 132, 140)),
                              ("f16->bf16 half-wave", ln_fwd(BF16, F16, 136, 144)), ("f16->bf16 wave", ln_fwd(BF16, F16, 132, 140)),
                              ("f16->f16 half-wave", ln_fwd(F16, F16, 136, 144)), ("f16->f16 wave", ln_fwd(F16, F16, 132, 140)),
                              ("statistics only", ln_fwd(BF16, F16, 136, 144, y=False))] + [(f"f32 d={d}", ln_fwd(F32, F32, d, d + 8)) for d in LN_D] + \
                             [(f"half-wave d={d}", ln_fwd(BF16, F16, d, d + 8)) for d in LN_D]
    E["lpi_layernorm_bwd"] = [("half-wave", ln_bwd(BF16, BF16, F16, 136, 144, dx=False)), ("f16 x, no dx", ln_bwd(BF16, BF16, F16, 132, 140, dx=False)),
                              ("f16 x, dx", ln_bwd(BF16, BF16, F16, 136, 144)), ("fff", ln_bwd(F32, F32, F32, 132, 140)), ("ffb", ln_bwd(F32, BF16, F32, 132, 140)),
                              ("fbb", ln_bwd(BF16, BF16, F32, 132, 140)), ("fbf", ln_bwd(BF16, F32, F32, 132, 140)), ("fff no cast", ln_bwd(F32, F32, F32, 132, 140, cast=False))] + \
                             [(f"fff d={d}", ln_bwd(F32, F32, F32, d, d + 8)) for d in LN_D] + [(f"half-wave d={d}", ln_bwd(BF16, BF16, F16, d, d + 8, dx=False)) for d in LN_D]
    E["lpi_layernorm_bwd_rows_varlen"] = [("half-wave, row_start", ln_bwd_rows(BF16, BF16, F16, 136, 144, False, True, True)),
                                          ("fff uniform", ln_bwd_rows(F32, F32, F32, 132, 140, True, True))]
    E["lpi_layernorm_bwd_rows"] = [("half-wave", ln_bwd_rows(BF16, BF16, F16, 136, 144, False, False)), ("fbb", ln_bwd_rows(BF16, BF16, F32, 132, 140, True, False))]

    def patchify(dt, R, ps, u8):      # cols: [B * G * G, Kp], Kp = 3 ps^2 rounded up to 128 bytes
        K, bk = 3 * ps * ps, 32 if dt == F32 else 64
        Kp = (K + bk - 1) // bk * bk
        return [("dtype", "dt", dt), ("B", "n", 2), ("R", "n", R), ("ps", "n", ps), P_("image", 1)] + ([P_("lut", 2)] if u8 else []) + [P_("cols", 3), ("ldcols", "ld", Kp + 8, Kp)]
    E["lpi_patchify"] = [("f32 vec4", patchify(F32, 16, 4, False)), ("bf16 vec4", patchify(BF16, 16, 4, False)), ("f16 scalar", patchify(F16, 6, 2, False))]
    E["lpi_patchify_u8"] = [("f32", patchify(F32, 16, 4, True)), ("bf16", patchify(BF16, 16, 4, True)), ("f16", patchify(F16, 16, 4, True))]
    E["lpi_vis_assemble_fwd"] = [(n, [("x_dtype", "dt", dt), ("B", "n", 2), ("G2", "n", 4), ("P", "n", p), ("d", "d", 132), P_("patch_emb", 1), ("ldpe", "ld", 140, 132),
                                      P_("cls", 2), P_("pos", 3), P_("prompt0", 4, p == 0), ("prompt_bstride", "l", 264), P_("gamma", 5), P_("beta", 6), P_("x0", 7),
                                      P_("mean", 8), P_("rstd", 9), P_("out_mean", 10, not st), P_("out_rstd", 11, not st)])
                                 for n, dt, p, st in (("f32", F32, 2, False), ("f16 + statistics", F16, 2, True), ("no prompt", F32, 0, False))]

    def gbr(dt, cols, ld, varlen):
        return [("dtype", "dt", dt), ("B", "n", 3), ("L", "L", 9)] + ([P_("row_start", 8, True)] if varlen else []) + \
               [("row0", "row0", 2), ("P", "P", 4), ("cols", "ld", cols, cols + 4), P_("src", 1), ("ld_src", "ld", ld, cols), P_("dst", 2), ("ld_dst", "ld", ld, cols)]
    E["lpi_gather_batch_rows_varlen"] = [("f32", gbr(F32, 132, 140, True)), ("bf16", gbr(BF16, 136, 144, True))]
    E["lpi_gather_batch_rows"] = [("f16", gbr(F16, 136, 144, False))]

    def rsum(dt, varlen):
        return [("dtype", "dt", dt), ("B", "n", 3), ("L", "L", 9)] + ([P_("row_start", 8, True)] if varlen else []) + \
               [("row0", "row0", 2), ("P", "P", 4), ("d", "d", 132), P_("dx", 1), P_("out", 2), ("accumulate", "i", 0)]
    E["lpi_rows_sum_over_batch_varlen"] = [("f32", rsum(F32, True)), ("bf16", rsum(BF16, True))]
    E["lpi_rows_sum_over_batch"] = [("f32", rsum(F32, False))]
    E["lpi_vis_assemble_bwd"] = [(n, [("dtype", "dt", dt), ("B", "n", 2), ("G2", "n", 4), ("P", "n", 2), ("d", "d", 132), P_("dx0", 1), P_("prompt0", 2), ("prompt_bstride", "l", 264),
                                      P_("gamma", 3), P_("mean", 4), P_("rstd", 5), P_("dprompt", 6)]) for n, dt in (("f32", F32), ("bf16", BF16))]

    def txt(dt, form):
        a = [("x_dtype", "dt", dt), ("B", "n", 3), ("L", "L", 9)]
        if form == "shared":
            a += [P_("row_start", 8), ("shared_rows", "n", 3)]
        elif form == "varlen":
            a += [P_("row_start", 8, True)]
        a += [("P", "P", 2), ("d", "d", 132), P_("ids", 1), P_("tok_emb", 2), P_("pos", 3), P_("ctx", 4)]
        if form != "shared":
            a += [("ctx_bstride", "l", 264)]
        return a + [P_("x0", 5), P_("out_mean", 6, dt == F32), P_("out_rstd", 7, dt == F32)]
    E["lpi_txt_embed_fwd_shared"] = [("f16", txt(F16, "shared"))]
    E["lpi_txt_embed_fwd_varlen"] = [("f32", txt(F32, "varlen")), ("f16", txt(F16, "varlen"))]
    E["lpi_txt_embed_fwd"] = [("f32", txt(F32, "plain"))]

    def padd(dt, varlen):
        return [("x_dtype", "dt", dt), ("B", "n", 3), ("L", "L", 9)] + ([P_("row_start", 8, True)] if varlen else []) + \
               [("P", "P", 2), ("d", "d", 132), P_("x", 1), P_("prompt_l", 2), ("prompt_bstride", "l", 264), P_("out_mean", 3, dt == F32), P_("out_rstd", 4, dt == F32)]
    E["lpi_prompt_add_varlen"] = [("f32", padd(F32, True)), ("f16 + statistics", padd(F16, True))]
    E["lpi_prompt_add"] = [("f32", padd(F32, False))]
    E["lpi_pool_ln_fwd"] = [(f"{xdt}->{dt}" + ("" if L else " absolute rows"),
                             [("dtype", "dt", dt), ("x_dtype", "dt", xdt), ("B", "n", 5), ("L", "L", L), ("d", "d", 132), P_("x", 1), P_("idx", 2, idx is None), P_("gamma", 3),
                              P_("beta", 4), P_("y", 5), ("ldy", "ld", 140, 132), P_("mean", 6), P_("rstd", 7)])
                            for dt, xdt, L, idx in ((F32, F32, 9, 1), (BF16, F32, 9, None), (BF16, F16, 9, 1), (F16, F32, 9, 1), (F16, F16, 9, 1), (F32, F32, 0, 1))]
    E["lpi_pool_ln_bwd"] = [(n, [("cast_dtype", "dt", dt), ("B", "n", 5), ("L", "L", 9), ("d", "d", 132), P_("dy", 1), ("lddy", "ld", 140, 132), P_("x", 2), P_("idx", 3), P_("gamma", 4),
                                 P_("mean", 5), P_("rstd", 6), P_("dx", 7), P_("dx_cast", 8, not cast)]) for n, dt, cast in (("f32", F32, True), ("bf16", BF16, True), ("no cast", BF16, False))]
    E["lpi_gather_rows"] = [(n, [("x_dtype", "dt", dt), ("B", "n", 5), ("L", "L", 9), ("d", "d", 132), P_("src", 1), P_("idx", 2), P_("dst", 3)]) for n, dt in (("f32", F32), ("f16", F16))]
    E["lpi_scatter_rows"] = [(n, [("cast_dtype", "dt", dt), ("B", "n", 5), ("L", "L", 9), ("d", "d", 132), P_("src", 1), P_("idx", 2), P_("dst", 3, not dst), P_("dst_cast", 4)])
                             for n, dt, dst in (("f32", F32, True), ("bf16", BF16, True), ("cast only", BF16, False))]
    E["lpi_scatter_add_rows"] = [(n, [("dtype", "dt", dt), ("B", "n", 5), ("L", "L", L), ("d", "d", 132), P_("src", 1), ("ld_src", "ld", 140, 132), P_("idx", 2), P_("dst", 3),
                                      ("ld_dst", "ld", 144, 132)]) for n, dt, L in (("f32", F32, 9), ("bf16", BF16, 9), ("absolute rows", F32, 0))]
    E["lpi_l2norm_fwd"] = [("f32", [("B", "n", 5), ("E", "d", 132), P_("x", 1), ("ldx", "ld", 140, 132), P_("y", 2), ("ldy", "ld", 144, 132), P_("inv_norm", 3)])]
    E["lpi_l2norm_bwd"] = [("f32", [("B", "n", 5), ("E", "d", 132), P_("y", 1), ("ldy", "ld", 140, 132), P_("dy", 2), ("lddy", "ld", 144, 132), P_("inv_norm", 3), P_("dx", 4),
                                    ("lddx", "ld", 136, 132)])]
    E["lpi_ln_stats_finalize_pair"] = [(n, [("rows0", "n", 10), ("d0", "d", 256), P_("part0", 1), ("ld0", "ld", 12, 10), P_("mean0", 2), P_("rstd0", 3), ("rows1", "n", r1), ("d1", "d", 384),
                                            P_("part1", 4), ("ld1", "ld", 12, 10), P_("mean1", 5), P_("rstd1", 6), ("eps", "f", 1e-5)]) for n, r1 in (("two", 10), ("one", 0))]
    E["lpi_ln_stats_finalize"] = [("one", [("rows", "n", 10), ("d", "d", 256), P_("part", 1), ("ld", "ld", 12, 10), ("eps", "f", 1e-5), P_("mean", 2), P_("rstd", 3)])]
    E["lpi_eot_index"] = [("ids", [("B", "n", 5), ("L", "n", 9), P_("ids", 1), P_("idx", 2)])]
    E["lpi_cast"] = [(n, [("src_dtype", "dt", s), ("dst_dtype", "dt", t), ("n", "n", 1320), P_("src", 1), P_("dst", 2)]) for n, s, t in (("f32->bf16", F32, BF16), ("bf16->f32", BF16, F32), ("f32->f32", F32, F32))]
    E["lpi_transpose"] = [(n, [("dtype", "dt", dt), ("rows", "n", 33), ("cols", "n", 70), P_("src", 1), ("lds", "ld", 72, 70), P_("dst", 2), ("ldd", "ld", 36, 33)]) for n, dt in (("f32", F32), ("bf16", BF16))]
    E["lpi_transpose2"] = [("f32", [("dtype", "dt", F32), ("rows0", "n", 33), ("cols0", "n", 70), P_("src0", 1), ("lds0", "ld", 72, 70), P_("dst0", 2), ("ldd0", "ld", 36, 33),
                                    ("rows1", "n", 20), ("cols1", "n", 40), P_("src1", 3), ("lds1", "ld", 44, 40), P_("dst1", 4), ("ldd1", "ld", 24, 20)])]
    E["lpi_mx8_quantize"] = [(n, [("x_dtype", "dt", dt), ("rows", "n", 10), ("K", "d", 160), P_("x", 1), ("ldx", "ld", 168, 160), P_("q", 2), ("ldq", "ld", 164, 160), P_("scales", 3),
                                  ("lds", "ld", 7, 5 + 4)]) for n, dt in (("f32", F32), ("bf16", BF16), ("f16", F16))]
    E["lpi_layernorm_mx8_fwd"] = [(f"{dt} d={d}", [("x_dtype", "dt", dt), ("rows", "n", 10), ("d", "d", d), P_("x", 1), ("ldx", "ld", d + 8, d), P_("gamma", 2), P_("beta", 3), P_("q", 4),
                                                   ("ldq", "ld", d + 4, d), P_("scales", 5), ("lds", "ld", d // 32 + 2, d // 32 + 4), P_("mean", 6), P_("rstd", 7)])
                                  for dt, d in ((F32, 160), (F16, 160), (F32, 288), (F16, 544), (F32, 800))]
    return {k: [(n, a + [S]) for n, a in v] for k, v in E.items()}


# ---- the calls that take descriptors: fields of descriptor i are named "<i>.<field>" in the argument list
def _desc_call(fn, cls, names, values):
    """fn(leading scalars..., descriptors, NULL stream): the values named "<i>.<field>" fill descriptor i, the others lead the call"""
    arr = (cls * (1 + max(int(k.split(".")[0]) for k in names if "." in k)))()
    head = []
    for k, v in zip(names, values):
        if "." in k:
            i, f = k.split(".")
            setattr(arr[int(i)], f, v if f not in _PTRS or v else None)
        else:
            head.append(v)
    return fn(*head, ctypes.cast(arr, ctypes.c_void_p), None)


def pair(a, b):
    """two lists -> one, names prefixed by the descriptor index"""
    return [(f"{i}.{x[0]}",) + tuple(x[1:]) for i, l in enumerate((a, b)) for x in l]


def desc_entry_points():
    D = {}

    def fwd(d, ld, y=True, k=0):
        return [x if x[1] != "p" or not x[2] else (x[0], "p", x[2] + k * 0x400000) for x in ln_fwd(0, 0, d, ld, y)[2:]]

    def bwd(d, ld, dx, k=0):
        return [x if x[1] != "p" or not x[2] else (x[0], "p", x[2] + k * 0x400000) for x in ln_bwd(0, 0, 0, d, ld, dx)[3:]]
    D["lpi_layernorm_fwd_pair"] = [(n, [("dtype", "dt", dt), ("x_dtype", "dt", xdt)] + pair(fwd(d0, d0 + 8, y), fwd(d1, d1 + 8, y, 1)))
                                   for n, dt, xdt, d0, d1, y in (("fused bf16", BF16, F16, 136, 264, True), ("fused f16, narrow first", F16, F16, 136, 520, True),
                                                                 ("statistics only", BF16, F16, 776, 136, False), ("two launches (d % 8)", BF16, F16, 132, 264, True),
                                                                 ("two launches (f32)", F32, F32, 132, 264, True), ("two launches (d > 1024)", BF16, F16, 1032, 136, True))]
    D["lpi_layernorm_bwd_pair"] = [(n, [("dy_dtype", "dt", a), ("cast_dtype", "dt", b), ("x_dtype", "dt", c)] + pair(bwd(d0, d0 + 8, dx), bwd(d1, d1 + 8, dx, 1)))
                                   for n, a, b, c, d0, d1, dx in (("fused", BF16, BF16, F16, 264, 136, False), ("fused, narrow first", BF16, BF16, F16, 136, 776, False),
                                                                  ("two launches (dx)", BF16, BF16, F16, 136, 264, True), ("two launches (f32)", F32, F32, F32, 132, 264, True))]

    def rs(k, d, P):
        return [("B", "n", 3), ("L", "L", 9), ("row0", "row0", 2), ("P", "P", P), ("d", "d", d), ("accumulate", "i", 0), P_("row_start", 8, True), P_("dx", 1 + 2 * k), P_("out", 2 + 2 * k)]
    D["lpi_rows_sum_over_batch_pair"] = [(n, [("dtype", "dt", dt)] + pair(rs(0, 132, 4), rs(1, 264, 2))) for n, dt in (("f32", F32), ("bf16", BF16))]
    return D


def row_job_ops():
    """op name -> (op code, [(label, fields)]): fields as an argument list whose names are lpi_row_job members"""
    J = {}
    J["POOL_LN_FWD"] = (1, [(n, [("dt_a", "dt", xdt), ("dt_b", "dt", dt), ("B", "n", 5), ("L", "L", 9), ("d", "d", 132), P_("a", 1), P_("idx", 2), P_("gamma", 3), P_("beta", 4), P_("out", 5),
                                 ("ld_c", "ld", 140, 132), P_("mean", 6), P_("rstd", 7), P_("out2", 8, not o2)])
                            for n, xdt, dt, o2 in (("f32->f32", F32, F32, False), ("f32->bf16 + out2", F32, BF16, True), ("f16->bf16", F16, BF16, False), ("f32->f16", F32, F16, False),
                                                   ("f16->f16 + out2", F16, F16, True))])
    J["L2NORM_FWD"] = (2, [("f32", [("B", "n", 5), ("d", "d", 132), P_("a", 1), ("ld_a", "ld", 140, 132), P_("out", 2), ("ld_c", "ld", 144, 132), P_("mean", 3)])])
    J["L2NORM_BWD"] = (3, [(n, [("dt_b", "dt", dt), ("B", "n", 5), ("d", "d", 132), P_("a", 1), ("ld_a", "ld", 140, 132), P_("b", 2), ("ld_b", "ld", 144, 132), P_("mean_in", 3), P_("out", 4),
                                ("ld_c", "ld", 136, 132), P_("out2", 5, not o2)]) for n, dt, o2 in (("f32", F32, False), ("bf16 copy", BF16, True))])
    J["POOL_LN_BWD"] = (4, [(n, [("dt_b", "dt", dt), ("B", "n", 5), ("L", "L", 9), ("d", "d", 132), P_("a", 1), ("ld_a", "ld", 140, 132), P_("b", 2), P_("idx", 3), P_("gamma", 4), P_("mean_in", 5),
                                 P_("rstd_in", 6), P_("out", 7), P_("out2", 8, not o2)]) for n, dt, o2 in (("f32", F32, True), ("bf16", BF16, True), ("no cast", BF16, False))])
    J["LN_BWD"] = (5, [(n, [("dt_a", "dt", dt), ("dt_b", "dt", dt), ("B", "n", 5), ("d", "d", d), P_("a", 1), ("ld_a", "ld", d + 8, d), P_("b", 2), ("ld_b", "ld", d + 8, d), P_("gamma", 3),
                            P_("mean_in", 4), P_("rstd_in", 5), P_("out", 6, not dx), ("ld_c", "ld", d + 8, d), P_("out2", 7), ("flag", "i", 1)])
                       for n, dt, d, dx in [("bf16", BF16, 132, True), ("f32", F32, 132, True), ("bf16 no dx", BF16, 132, False)] + [(f"f32 d={d}", F32, d, True) for d in LN_D]])
    J["SCATTER_ADD"] = (6, [(n, [("dt_a", "dt", dt), ("B", "n", 5), ("L", "L", L), ("d", "d", 132), P_("a", 1), ("ld_a", "ld", 140, 132), P_("idx", 2), P_("out", 3), ("ld_c", "ld", 144, 132)])
                            for n, dt, L in (("f32", F32, 9), ("bf16", BF16, 9), ("absolute rows", F32, 0))])
    J["GATHER_BATCH_ROWS"] = (7, [("16-byte units", [("B", "n", 3), ("L", "L", 9), P_("row_start", 8, True), ("row0", "row0", 2), ("P", "P", 4), ("d", "ld", 33, 37), P_("a", 1), ("ld_a", "ld", 35, 33),
                                                     P_("out", 2), ("ld_c", "ld", 36, 33)])])
    J["PROMPT_ADD"] = (8, [(n, [("dt_a", "dt", dt), ("B", "n", 3), ("L", "L", 9), P_("row_start", 8, True), ("P", "P", 2), ("d", "d", 132), P_("out", 1), P_("a", 2), ("bstride", "l", 264),
                                P_("mean", 3, dt == F32), P_("rstd", 4, dt == F32)]) for n, dt in (("f32", F32), ("f16 + statistics", F16))])
    J["LN_BWD_ROWS_H16"] = (9, [(f"d={d}", [("B", "n", 3), ("L", "L", 9), P_("row_start", 8, d != 136), ("row0", "row0", 2), ("P", "P", 4), ("d", "d", d), P_("a", 1), ("ld_a", "ld", d + 8, d),
                                            P_("b", 2), ("ld_b", "ld", d + 8, d), P_("gamma", 3), P_("mean_in", 4), P_("rstd_in", 5), P_("out2", 6), ("ld_c", "ld", d + 16, d), ("flag", "i", 1)])
                                for d in (136, 264, 520, 776)])
    J["VIS_PROMPT_ROWS_BWD"] = (10, [(n, [("dt_a", "dt", dt), ("B", "n", 2), ("L", "n", 7), ("P", "n", 2), ("d", "d", 132), P_("out", 1), P_("a", 2), ("bstride", "l", 264), P_("gamma", 3),
                                          P_("mean_in", 4), P_("rstd_in", 5)]) for n, dt in (("f32", F32), ("bf16", BF16))])
    return J


_DESCS = {"lpi_layernorm_fwd_pair": (_lib.LnFwdDesc, 2), "lpi_layernorm_bwd_pair": (_lib.LnBwdDesc, 3), "lpi_rows_sum_over_batch_pair": (_lib.RowsSumDesc, 1)}
_PTRS = _lib._ROWJOB_PTRS | {"x", "y", "dy", "dx", "dx_cast"}


def cases():
    """[(entry point or 'job:<OP>', tuple label, thunk)]: the thunk calls the library once and returns its code"""
    lib = _lib.load()
    out = []

    def add(name, branch, args, run):
        out.append((name, f"{branch}: good", (lambda v=[a[2] for a in args]: run(v))))
        for label, v in mutations(args):
            out.append((name, f"{branch}: {label}", (lambda v=v: run(v))))
    for name, branches in entry_points().items():
        fn = getattr(lib, name)
        for branch, args in branches:
            add(name, branch, args, lambda v, fn=fn: fn(*v))
    for name, branches in desc_entry_points().items():
        cls, lead = _DESCS[name]
        for branch, args in branches:
            names = [a[0] for a in args]
            add(name, branch, args, lambda v, fn=getattr(lib, name), cls=cls, names=names: _desc_call(fn, cls, names, v))
    for op, (code, branches) in row_job_ops().items():
        for branch, args in branches:
            names = ["n", "0.op"] + ["0." + a[0] for a in args]
            add("job:" + op, branch, args, lambda v, code=code, names=names: _desc_call(lib.lpi_row_jobs, _lib.RowJob, names, [1, code] + v))
    # the job list itself: count, NULL list, an unknown op, a good job behind a bad one and the reverse (every job is checked before the launch)
    good = row_job_ops()["L2NORM_FWD"][1][0][1]
    names = ["n", "0.op"] + ["0." + a[0] for a in good] + ["1.op"] + ["1." + a[0] for a in good]
    v0 = [a[2] for a in good]
    for label, n, op0, op1, bad in (("two good jobs", 2, 2, 2, None), ("n = 0", 0, 2, 2, None), ("n = 5", 5, 2, 2, None), ("unknown op", 1, 11, 2, None), ("op 0", 1, 0, 2, None),
                                    ("second job bad", 2, 2, 2, 1), ("first job bad", 2, 2, 2, 0)):
        vals = [n, op0] + ([0] + v0[1:] if bad == 0 else v0) + [op1] + ([0] + v0[1:] if bad == 1 else v0)
        out.append(("lpi_row_jobs", label, (lambda vals=vals: _desc_call(lib.lpi_row_jobs, _lib.RowJob, names, vals))))
    out.append(("lpi_row_jobs", "NULL list", lambda: lib.lpi_row_jobs(1, None, None)))
    for name in _DESCS:
        lead = _DESCS[name][1]
        out.append((name, "NULL descriptors", (lambda fn=getattr(lib, name), lead=lead: fn(*([BF16] * lead), None, None))))
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
    cs = cases()
    res = run(cs)
    rec = {}
    for (name, _, _), r in zip(cs, res):
        rec.setdefault(name, []).append(r)
    with open(EXPECTED, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in rec.items()) + "\n}\n")
    print(f"{len(cs)} tuples of {len(rec)} names recorded from {_lib.LIB_PATH}: {sum(1 for r in res if r[1])} accepted, {sum(1 for r in res if not r[1])} refused")


if __name__ == "__main__":
    main()
