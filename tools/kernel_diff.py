#!/usr/bin/env python3
r"""Per-kernel machine-code comparison of two builds (CPU only):  tools/kernel_diff.py OLD NEW [--arch gfx950] [--list] [--rename REGEX=REPL]...

OLD / NEW are either two shared libraries (every gfx950 code object in their offload bundles is disassembled with llvm-objdump) or two
`hipcc --cuda-device-only -S` outputs of the same translation unit.  For every kernel symbol: identical, differs, or only in one side.  The
instruction text of WHOLE kernels is compared, local block labels renumbered in order of appearance; for a kernel that differs the VGPR / SGPR /
scratch / LDS figures of both sides are printed from the code-object metadata.  Exit status 1 if anything differs or is only in one side.
--rename pairs kernels whose (mangled) names changed: re.sub(REGEX, REPL) on NEW's names, e.g. for kernels that became instantiations of one template
  --rename 'g1qb_(\w+?)I10G1Q(\d)Stream(\w+?)S4_=g1q\2_\1I\3S3_'"""
import argparse
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
META = {"vgpr": ".vgpr_count", "sgpr": ".sgpr_count", "scratch": ".private_segment_fixed_size", "lds": ".group_segment_fixed_size"}


def metadata(text):
    """{kernel: {vgpr, sgpr, scratch, lds}} from the amdhsa.kernels YAML (the same text in a .s file and in `llvm-readelf --notes`)"""
    out = {}
    for entry in re.split(r"\n\s*- \.", text):
        name = re.search(r"(?:^|\n)\s*\.name:\s*'?([\w.$]+)'?", "\n." + entry)
        if not name or ".kernarg_segment_size:" not in entry:
            continue
        out[name.group(1)] = {k: int(m.group(1)) if (m := re.search(re.escape(v) + r":\s*(\d+)", entry)) else -1 for k, v in META.items()}
    return out


def normalise(lines):
    labels, body = {}, []
    for ln in lines:
        ln = re.split(r"\s*(?://|;)", ln, maxsplit=1)[0].strip()          # comments: addresses, encodings
        if not ln or (ln.startswith(".") and not re.match(r"\.LBB\d+_\d+:", ln)):      # assembler directives
            continue
        body.append(re.sub(r"\.LBB\d+_\d+|\bL\d+\b", lambda m: labels.setdefault(m.group(0), "@%d" % len(labels)), ln))
    return body


def from_asm(path):
    text = open(path).read()
    meta, code = metadata(text), {}
    for name in meta:
        m = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.S | re.M)
        if m:
            code[name] = normalise(m.group(1).splitlines())
    return code, meta


def from_library(path, arch):
    data, code, meta, at = open(path, "rb").read(), {}, {}, 0
    with tempfile.TemporaryDirectory() as tmp:
        while (at := data.find(MAGIC, at)) >= 0:
            (n,), p = struct.unpack_from("<Q", data, at + 24), at + 32
            for _ in range(n):
                off, size, tl = struct.unpack_from("<QQQ", data, p)
                triple, p = data[p + 24:p + 24 + tl].decode(), p + 24 + tl
                if arch not in triple or size == 0:
                    continue
                co = os.path.join(tmp, "co%d.o" % len(os.listdir(tmp)))
                open(co, "wb").write(data[at + off:at + off + size])
                m = metadata(subprocess.run([LLVM + "/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout)
                dis = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", "--symbolize-operands", co],
                                     capture_output=True, text=True, check=True).stdout
                for name, body in re.findall(r"^<(?!L\d+>)([\w.$]+)>:\n(.*?)(?=^<(?!L\d+>)[\w.$]+>:|\Z)", dis, re.S | re.M):
                    if name in m:
                        code[name] = normalise(body.splitlines())
                meta.update(m)
            at += len(MAGIC)
    return code, meta


def load(path, arch):
    return from_library(path, arch) if open(path, "rb").read(4) == b"\x7fELF" else from_asm(path)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--list", action="store_true", help="print the identical kernels too")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL", help="re.sub on NEW's kernel names before pairing")
    a = ap.parse_args()
    (co, mo), (cn, mn) = load(a.old, a.arch), load(a.new, a.arch)
    for pat, repl in (r.split("=", 1) for r in a.rename):
        cn, mn = ({re.sub(pat, repl, k): v for k, v in d.items()} for d in (cn, mn))
    same = [k for k in co if k in cn and co[k] == cn[k]]
    diff = [k for k in co if k in cn and co[k] != cn[k]]
    only = [(k, "old") for k in co if k not in cn] + [(k, "new") for k in cn if k not in co]
    if a.list:
        for k in same:
            print("identical    ", k)
    for k in diff:
        print("differs      ", k, "(%d -> %d instructions and labels)" % (len(co[k]), len(cn[k])))
        for side, m in (("old", mo[k]), ("new", mn[k])):
            print("    %s: VGPR %d  SGPR %d  scratch %d B  LDS %d B" % (side, m["vgpr"], m["sgpr"], m["scratch"], m["lds"]))
    for k, side in only:
        print("only in %s  " % side, k)
    print("%d kernels: %d identical, %d differ, %d only in one" % (len(same) + len(diff) + len(only), len(same), len(diff), len(only)))
    return 1 if diff or only else 0


if __name__ == "__main__":
    sys.exit(main())
