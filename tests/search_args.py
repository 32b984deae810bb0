"""The argument grid of the streamed search's HOST layer (lpi_amd/csrc/search.hip, search16.hip, search_mx8.hip, search_mx4.hip, search_wide.hip,
search_rerank.hip; the rules themselves are in search_tile.h): which argument lists each entry point accepts and which it refuses before any launch.

The host code of this family never dereferences an operand pointer, so the whole accept set can be observed with made-up addresses, as tests/gemm_args.py
does for the GEMM family: a refused call returns LPI_EINVAL and lpi_launch_count() stays; an accepted call gets as far as the runtime, which, without a
device, answers with its no-device code (100) -- from the LDS set-up of a sweep (no launch counted) or, for the re-rank kernel, which needs none, from the
launch itself (counted).

cases() builds a deterministic grid.  Good lists: each of the 13 launching entry points at a few shapes (SHAPES: an ordinary one, one of a row block plus two
rows and two gallery tiles plus an edge, one row against a gallery shorter than a list with E = 1024, the training split's), the list forms at the ends of
their k range with and without accumulate, the typed forms with every type they take.  Then every argument mutated one at a time: counts 0 and -1; E at every
multiple of 8 or 16 around each type's step, at 1024 and above it; each leading dimension short or misaligned; each pointer NULL or misaligned; scale
pointers and scale strides; k at 0, 1, 16 / 17, 256 / 257 and above ng (the workspace is then made large, so that the rule on k is what answers); col_base
at -1 and around 2^31 - ng; a workspace one byte short; gt_per_row, kc, ldc and the re-rank k at their edges; every dt code from -1 to one past LPI_MX4.
For the two workspace functions the grid is a table of inputs (WS_NQ x WS_NG x their k) with the value returned.

Run as a script WITHOUT a GPU, this records [return code, launches] per tuple and the two tables into tests/search_args_expected.json (the distinct outcomes
once, then a letter per tuple, one string per good list: load_record() reads it back):
    LPI_LIB=<build of the commit to record>/liblpi_hip.so python3 tests/search_args.py <hash of that commit>
The committed record is that of the library before the host layer moved onto one call struct (SearchCall, search_tile.h).
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from lpi_amd import _lib  # noqa: E402

EXPECTED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "search_args_expected.json")
F32, BF16, F16, MX8, MX4 = 0, 1, 2, 3, 5
NAMES = {F32: "f32", BF16: "bf16", F16: "f16", MX8: "mx8", MX4: "mx4"}
DT_CODES = range(-1, 7)      # one past LPI_MX4 = 5
EINVAL = -22
WORKSPACES = ("lpi_search_workspace", "lpi_search_wide_workspace")
SHAPES = ((300, 4133, 512), (130, 300, 128), (1, 10, 1024), (123287, 616767, 256))      # nq, ng, E
E_VALUES = (-1, 0, 8, 16, 24, 32, 48, 64, 96, 120, 128, 136, 192, 256, 384, 1024, 1032, 1040, 1056, 1152, 2048)
WS_NQ = (-1, 0, 1, 127, 128, 129, 300, 5000, 65536, 123287)
WS_NG = (-1, 0, 1, 127, 128, 129, 4133, 65407, 65536, 616767, 2**31 - 1)
WS_K = {"lpi_search_workspace": (-1, 0, 1, 5, 16, 17), "lpi_search_wide_workspace": (-1, 0, 1, 16, 17, 128, 129, 256, 257)}
BIG = 1 << 40                # a workspace size that is never the reason for a refusal


def A(k):
    """the k-th made-up address: 4 KiB aligned, 16 MiB apart"""
    return 0x7E0000000000 + k * 0x1000000


def accepted(rc):
    """did the argument list pass the host checks?"""
    return rc != EINVAL


def elem_bytes(dt):
    return {F32: 4, BF16: 2, F16: 2, MX8: 1, MX4: 1}[dt]      # MX-FP4: of a code byte, the unit of its leading dimensions


# an argument: (name, kind, value[, row width]).  kinds: dt type code | n count | E | p pointer | ld leading dimension of rows `width` wide | k list length |
# cb col_base | acc accumulate | wsb ws_bytes | gpr gt_per_row | kc, ldc, rk: the re-rank form's | s the NULL stream
def operands(dt, nq, ng, E, typed):
    """the arguments every entry point begins with: [dt,] nq, ng, E, Q, ldq, [q_scales, ldqs,] G, ldg, [g_scales, ldgs]; leading dimensions leave 16 bytes of
    room, so that a grown E meets its own rule first"""
    row = E // 2 if dt == MX4 else E
    pad = 16 // elem_bytes(dt)
    out = ([("dt", "dt", dt)] if typed else []) + [("nq", "n", nq), ("ng", "n", ng), ("E", "E", E), ("Q", "p", A(1)), ("ldq", "ld", row + pad, row)]
    if dt in (MX8, MX4):
        out += [("q_scales", "p", A(2)), ("ldqs", "ld", E // 32 + 4, E // 32)]
    out += [("G", "p", A(3)), ("ldg", "ld", row + pad, row)]
    if dt in (MX8, MX4):
        out += [("g_scales", "p", A(4)), ("ldgs", "ld", E // 32 + 4, E // 32)]
    return out


def list_form(lib, wide, nq, ng, k, acc):
    need = getattr(lib, WORKSPACES[wide])(nq, ng, k)
    return [("k", "k", k, ng), ("col_base", "cb", 7, ng), ("accumulate", "acc", acc), ("idx", "p", A(5)), ("val", "p", A(6)), ("ws", "p", A(7)), ("ws_bytes", "wsb", need),
            ("stream", "s", None)]


def rank_form(lib, nq, ng):
    return [("gt", "p", A(8)), ("gt_per_row", "gpr", 5), ("rank", "p", A(9)), ("ws", "p", A(7)), ("ws_bytes", "wsb", lib.lpi_search_workspace(nq, ng, 0)), ("stream", "s", None)]


def rerank_form(kc, k):
    return [("cand", "p", A(10)), ("ldc", "ldc", kc + 3, kc), ("kc", "kc", kc, k), ("k", "rk", k, kc), ("idx", "p", A(5)), ("val", "p", A(6)), ("stream", "s", None)]


def mutations(args):
    """(label, {name: value}) of every one-argument mutation of a good list (a mutated k takes a large ws_bytes with it)"""
    for a in args:
        name, kind, v = a[0], a[1], a[2]
        also = {}
        if kind == "dt":
            alt = list(DT_CODES)
        elif kind == "n":
            alt = [0, -1]
        elif kind == "E":
            alt = list(E_VALUES)
        elif kind == "p":
            alt = [0, v + 1, v + 2, v + 4, v + 8]
        elif kind == "ld":
            alt = [0, -1, a[3] - 4, a[3] - 1, a[3], v + 1, v + 2, v + 4, v + 8]
        elif kind == "k":
            alt, also = [-1, 0, 1, 16, 17, 256, 257, a[3], a[3] + 1], {"ws_bytes": BIG}
        elif kind == "cb":
            alt = [-1, 0, 2**31 - 1 - a[3], 2**31 - a[3], 2**31 - 1]
        elif kind == "acc":
            alt = [0, 1, 2, -1]
        elif kind == "wsb":
            alt = [v - 1, 0, -1, BIG]
        elif kind == "gpr":
            alt = [0, -1, 1]
        elif kind == "kc":
            alt = [0, -1, 1, a[3] - 1, a[3], 256, 257]
        elif kind == "ldc":
            alt = [0, -1, a[3] - 1, a[3], v + 1]
        elif kind == "rk":
            alt = [0, -1, 1, a[3], a[3] + 1]
        else:
            continue
        for m in dict.fromkeys(alt):
            if m != v:
                yield f"{name}={m if kind != 'p' else (m - v if m else 'NULL')}", dict(also, **{name: m})


def entry_points():
    """name -> [(label, good argument list)]"""
    lib = _lib.load()
    E = {}
    lists = (("lpi_search_topk", F32, 0, 0), ("lpi_search_topk_t", None, 1, 0), ("lpi_search_topk_mx8", MX8, 0, 0), ("lpi_search_topk_mx4", MX4, 0, 0),
             ("lpi_search_topk_wide", F32, 0, 1), ("lpi_search_topk_wide_t", None, 1, 1), ("lpi_search_topk_wide_mx8", MX8, 0, 1), ("lpi_search_topk_wide_mx4", MX4, 0, 1))
    for name, dt0, typed, wide in lists:
        g = E.setdefault(name, [])
        for dt in ((F32, BF16, F16) if typed else (dt0,)):
            for nq, ng, e in SHAPES:
                for k in ((1, 5, 16) if not wide else (1, 17, 100, 128, 129, 256)):
                    for acc in (0, 1):
                        if acc or k <= ng:
                            g.append((f"{NAMES[dt]} {nq}x{ng}x{e} k={k} acc={acc}", operands(dt, nq, ng, e, typed) + list_form(lib, wide, nq, ng, k, acc)))
    for name, dt0, typed in (("lpi_search_rank", F32, 0), ("lpi_search_rank_t", None, 1), ("lpi_search_rank_mx8", MX8, 0)):
        g = E.setdefault(name, [])
        for dt in ((F32, BF16, F16) if typed else (dt0,)):
            g += [(f"{NAMES[dt]} {nq}x{ng}x{e}", operands(dt, nq, ng, e, typed) + rank_form(lib, nq, ng)) for nq, ng, e in SHAPES]
    for name, typed in (("lpi_search_rerank", 0), ("lpi_search_rerank_t", 1)):
        g = E.setdefault(name, [])
        for dt in ((F32, BF16, F16) if typed else (F32,)):
            g += [(f"{NAMES[dt]} {nq}x{ng}x{e} kc={kc} k={k}", operands(dt, nq, ng, e, typed) + rerank_form(kc, k))
                  for nq, ng, e in SHAPES for kc, k in ((1, 1), (20, 10), (40, 40), (256, 10), (256, 256))]
    return E


def cases():
    """[(entry point, tuple label, thunk)]: the thunk calls the library once and returns its code"""
    lib = _lib.load()
    out = []
    for name, goods in entry_points().items():
        fn = getattr(lib, name)
        for label, args in goods:
            good = {a[0]: a[2] for a in args}
            run = lambda change={}, fn=fn, good=good: fn(*dict(good, **change).values())      # noqa: E731
            out.append((name, f"{label}: good", run))
            for m, change in mutations(args):
                out.append((name, f"{label}: {m}", (lambda run=run, change=change: run(change))))
    return out


def workspace_tables():
    """{workspace function: [value for every (nq, ng, k) of WS_NQ x WS_NG x WS_K[function], k fastest]}"""
    lib = _lib.load()
    return {name: [int(getattr(lib, name)(nq, ng, k)) for nq in WS_NQ for ng in WS_NG for k in WS_K[name]] for name in WORKSPACES}


def run_one(thunk):
    """[code, launches] of one tuple"""
    n0 = _lib.launch_count()
    rc = int(thunk())
    return [rc, _lib.launch_count() - n0]


LETTERS = "abcdefghijklmnopqrstuvwxyz"


def load_record():
    """(recorded_from, {entry point: [[code, launches] per tuple, in the order of cases()]}, {workspace function: [values]})"""
    with open(EXPECTED) as f:
        rec = json.load(f)
    src, outcomes, tables = rec.pop("recorded_from"), rec.pop("outcomes"), rec.pop("workspace_tables")
    return src, {name: [outcomes[ch] for s in lists for ch in s] for name, lists in rec.items()}, tables


def _lines(items, width=280):
    """the items (already JSON text) as list lines, several short ones to a line"""
    out = []
    for s in items:
        if out and len(out[-1]) + len(s) + 2 <= width:
            out[-1] += ", " + s
        else:
            out.append("  " + s)
    return out


def main():
    import torch
    assert torch.cuda.device_count() == 0, "record on a machine without a GPU: the accepted lists would launch on made-up addresses"
    assert len(sys.argv) == 2, "usage: LPI_LIB=<library of the commit to record> python3 tests/search_args.py <hash of that commit>"
    cs = cases()
    res = [run_one(thunk) for _, _, thunk in cs]
    outcomes = sorted({tuple(r) for r in res})
    rec, last = {}, None
    for (name, label, _), r in zip(cs, res):
        if (name, label.split(":")[0]) != last:
            rec.setdefault(name, []).append("")
            last = (name, label.split(":")[0])
        rec[name][-1] += LETTERS[outcomes.index(tuple(r))]
    with open(EXPECTED, "w") as f:
        f.write('{\n "recorded_from": ' + json.dumps(sys.argv[1]) + ",\n" +
                ' "outcomes": {' + ", ".join(f'"{LETTERS[i]}": {json.dumps(list(o))}' for i, o in enumerate(outcomes)) + "},\n" +
                ' "workspace_tables": {\n' + ",\n".join(f'  "{k}": [\n' + ",\n".join("  " + ln for ln in _lines(map(str, v))) + "\n  ]" for k, v in workspace_tables().items()) + "\n },\n" +
                ",\n".join(f' "{k}": [\n' + ",\n".join(_lines(f'"{s}"' for s in v)) + "\n ]" for k, v in rec.items()) + "\n}\n")
    acc = sum(1 for r in res if accepted(r[0]))
    print(f"{len(cs)} tuples of {len(rec)} names and two workspace tables recorded from {_lib.LIB_PATH}: {acc} accepted, {len(cs) - acc} refused")


if __name__ == "__main__":
    main()
