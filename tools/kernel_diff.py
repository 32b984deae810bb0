#!/usr/bin/env python3
"""Are the device functions of two builds the same, function by function?  (CPU tool: llvm-objdump / llvm-readelf on the gfx950 code objects inside
<build dir>/<name>.o, unbundled as tools/isa_count.py does.)

usage: python3 tools/kernel_diff.py BUILD_DIR_A BUILD_DIR_B [--objects rowops.o,mx8_rows.o,attn_pooled.o] [--json OUT] [--label-a TEXT] [--label-b TEXT]
                                                         [--rename REGEX=REPL ...]

For the UNION of the listed objects' code objects on each side (a function may move between the objects) it compares, by function name and whatever the order:
the set of names; each function's disassembly with addresses and raw bytes stripped; each kernel's metadata note (VGPRs, SGPRs, LDS, private segment, kernarg
size).  Prints every difference and exits 1 if there is any.  It compares text and knows nothing about particular instructions.
--rename REGEX=REPL (repeatable, applied in order with re.sub) rewrites the function names of BOTH sides and the <name+offset> labels inside the text before
comparing, so that a kernel whose name changed (a new template argument, another argument struct) meets its predecessor under one key.
"""
import argparse
import difflib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
META = {".vgpr_count": "vgprs", ".sgpr_count": "sgprs", ".group_segment_fixed_size": "lds", ".private_segment_fixed_size": "private_segment",
        ".kernarg_segment_size": "kernarg"}


def device_object(obj, tmp):
    """the gfx950 code object bundled in a host object file"""
    d = tempfile.mkdtemp(dir=tmp)
    shutil.copy(obj, d)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", os.path.basename(obj)], check=True, capture_output=True, cwd=d)
    dev = [p for p in os.listdir(d) if "amdgcn" in p and "gfx950" in p]
    assert len(dev) == 1, (obj, os.listdir(d))
    return os.path.join(d, dev[0])


def functions(dev):
    """name -> disassembly text of the symbol's own bytes (the padding up to the next function's alignment is not part of it); branch targets read
    <function+offset>, so the text does not depend on where the function lies"""
    syms = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-t", dev], check=True, capture_output=True, text=True).stdout
    end = {}
    for line in syms.splitlines():      # "0000000000001a00 g     F .text  0000000000000a5c [.protected] name"
        m = re.match(r"^([0-9a-f]+) .* F \.text\s+([0-9a-f]+) (?:\.\w+ )?(\S+)$", line)
        if m:
            end[m.group(3)] = int(m.group(1), 16) + int(m.group(2), 16)
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", dev], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        m = re.match(r"^\s+(\S.*?)\s*// ([0-9A-Fa-f]+):.*$", line)      # "<instruction>   // 000000001234: BF8C0000": the comment carries the address (and the bytes)
        if m and cur is not None and int(m.group(2), 16) < end[cur]:
            out[cur].append(m.group(1))
    return {k: "\n".join(v) for k, v in out.items()}


def metadata(dev):
    """kernel name -> the resource fields of its AMDGPU metadata note"""
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", dev], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in notes.splitlines():      # the note is YAML: a kernel is an item of amdhsa.kernels ("  - "), its own keys are indented by four
        m = re.match(r"^(  - |    )(\.[a-z_]+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        if m.group(2) == ".name":
            out[m.group(3).strip().strip("'\"")] = cur
        elif m.group(2) in META:
            cur[META[m.group(2)]] = int(m.group(3))
    return out


def side(build_dir, objects, tmp):
    fn, md = {}, {}
    for o in objects:
        dev = device_object(os.path.join(build_dir, o), tmp)
        for name, text in functions(dev).items():
            assert name not in fn, "defined twice: " + name
            fn[name] = text
        md.update(metadata(dev))
    return fn, md


def renamed(fn, md, rules):
    def r(name):
        for pat, repl in rules:
            name = re.sub(pat, repl, name)
        return name
    out = {r(k): re.sub(r"<([^>+]+)", lambda m: "<" + r(m.group(1)), v) for k, v in fn.items()}
    assert len(out) == len(fn), "--rename maps two functions to one name"
    return out, {r(k): v for k, v in md.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--objects", default="rowops.o,mx8_rows.o,attn_pooled.o")
    ap.add_argument("--json")
    ap.add_argument("--show", help="regex: print the text diff of the differing functions it matches")
    ap.add_argument("--label-a", default=None)
    ap.add_argument("--label-b", default=None)
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL")
    args = ap.parse_args()
    rules = [r.split("=", 1) for r in args.rename]
    objects = args.objects.split(",")
    tmp = tempfile.mkdtemp()
    try:
        fa, ma = side(args.a, objects, tmp)
        fb, mb = side(args.b, objects, tmp)
    finally:
        shutil.rmtree(tmp)
    (fa, ma), (fb, mb) = renamed(fa, ma, rules), renamed(fb, mb, rules)
    only_a, only_b = sorted(set(fa) - set(fb)), sorted(set(fb) - set(fa))
    differ = []
    for name in sorted(set(fa) & set(fb)):
        code, meta = fa[name] != fb[name], ma.get(name) != mb.get(name)
        if code or meta:
            differ.append({"name": name, "code_differs": code, "metadata_differs": meta, "instructions": [fa[name].count("\n") + 1, fb[name].count("\n") + 1],
                           "metadata_a": ma.get(name), "metadata_b": mb.get(name)})
    for n in only_a:
        print("only in A:", n)
    for n in only_b:
        print("only in B:", n)
    for d in differ:
        print(f"differs: {d['name']}\n    code {'differs' if d['code_differs'] else 'same'} ({d['instructions'][0]} -> {d['instructions'][1]} lines)  "
              f"metadata A {d['metadata_a']}  B {d['metadata_b']}")
        if args.show and re.search(args.show, d["name"]):
            print("\n".join(difflib.unified_diff(fa[d["name"]].splitlines(), fb[d["name"]].splitlines(), "A", "B", lineterm="", n=2)))
    print(f"{len(fa)} functions in A, {len(fb)} in B, {len(ma)} / {len(mb)} kernels with metadata; {len(only_a)} only in A, {len(only_b)} only in B, {len(differ)} differ")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"a": args.label_a or args.a, "b": args.label_b or args.b, "objects": objects, "rename": args.rename, "functions_a": len(fa), "functions_b": len(fb),
                       "only_in_a": only_a, "only_in_b": only_b, "differ": differ}, f, indent=1)
            f.write("\n")
    return 1 if only_a or only_b or differ else 0


if __name__ == "__main__":
    sys.exit(main())
