#!/usr/bin/env python3
"""One line per gfx950 kernel of the library: demangled name, instruction count, SHA-256 of the normalised instruction stream,
SHA-256 of the kernel's .amdhsa_* block.  Two trees whose tables are equal ship the same device code, whichever source file
each kernel lives in: the proof a refactor of csrc/ needs, and it needs no GPU.

The stream of a kernel is the listing from its label to its .Lfunc_end, with comments cut, blank lines, .p2align / .loc /
.cfi* lines and the asm statements' ;;#ASMSTART / ;;#ASMEND markers dropped, and every local label (.L...) renamed by order
of first appearance within the kernel.  The translation unit is not part of a line.

Usage: python tools/isa_digest.py [TREE] [--against TABLE]
TREE defaults to this repository; its fractal-renderer_amd/build.py gives SOURCES and the flags.  With --against the exit code
is 1 if a kernel is missing, new or different ('#' lines of TABLE are ignored)."""
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = re.compile(r"^\.(p2align|loc|cfi\w*)\b")
LABEL = re.compile(r"\.L[\w$.]+")


def normalise(lines):
    """-> (normalised text, instruction count) of one kernel's lines."""
    names, out, count = {}, [], 0
    for raw in lines:
        s = " ".join(raw.split(";", 1)[0].split("//", 1)[0].split())
        if not s or DROP.match(s):
            continue
        s = LABEL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), s)
        count += not (s.endswith(":") or s.startswith("."))
        out.append(s)
    return "\n".join(out), count


def kernels(lines):
    """-> {mangled symbol: (instruction count, stream digest, .amdhsa digest)} of one listing."""
    meta, k = {}, 0
    while k < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[k])
        if m:
            end = next(j for j in range(k, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
            block = [" ".join(x.split(";", 1)[0].split()) for x in lines[k + 1:end]]
            meta[m.group(1)] = hashlib.sha256("\n".join(b for b in block if b).encode()).hexdigest()
            k = end
        k += 1
    out = {}
    for k, line in enumerate(lines):
        sym = line.split(":", 1)[0]
        if sym not in meta or ":" not in line:
            continue
        end = next(j for j in range(k + 1, len(lines)) if lines[j].startswith(".Lfunc_end"))
        text, count = normalise(lines[k:end])
        out[sym] = (count, hashlib.sha256(text.encode()).hexdigest(), meta[sym])
    assert set(out) == set(meta), sorted(set(meta) ^ set(out))
    return out


def table(root):
    """Compile every source of the tree at `root` to a listing -> (sorted lines 'name\\tcount\\tstream\\tamdhsa', hipcc version)."""
    spec = importlib.util.spec_from_file_location("_fr_build_digest", os.path.join(root, "fractal-renderer_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    flags = [f for f in build.HIPCC_FLAGS if f not in ("-shared", "-fPIC", "-pthread")]  # as scan_asm_hazards.build_flags()
    hipcc, found = build.find_hipcc(), {}
    with tempfile.TemporaryDirectory() as td:
        for src in build.SOURCES:
            lst = os.path.join(td, src + ".s")
            subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "-o", lst, os.path.join(build.CSRC, src)], check=True, cwd=build.CSRC,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            new = kernels(open(lst).read().split("\n"))
            assert not set(new) & set(found), "a kernel in two translation units: %s" % sorted(set(new) & set(found))
            found.update(new)
    syms = sorted(found)
    filt = os.path.join(os.path.dirname(hipcc), "..", "llvm", "bin", "llvm-cxxfilt")
    names = subprocess.run([filt if os.path.exists(filt) else "c++filt"], input="\n".join(syms), capture_output=True, text=True, check=True).stdout.split("\n")
    version = [x for x in subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout.split("\n") if "version" in x]
    return sorted("%s\t%d\t%s\t%s" % (n, *found[s]) for n, s in zip(names, syms)), "; ".join(v.strip() for v in version)


def compare(lines, saved):
    """-> list of differences between two tables (lists of 'name\\t...' lines)."""
    a, b = ({x.split("\t", 1)[0]: x for x in t if x and not x.startswith("#")} for t in (saved, lines))
    return (["missing: " + n for n in sorted(set(a) - set(b))] + ["new: " + n for n in sorted(set(b) - set(a))]
            + ["different: %s\n  was %s\n  is  %s" % (n, a[n].split("\t", 1)[1], b[n].split("\t", 1)[1]) for n in sorted(set(a) & set(b)) if a[n] != b[n]])


def main(argv):
    against = argv[argv.index("--against") + 1] if "--against" in argv else None
    rest = [a for a in argv if a not in ("--against", against)]
    lines, version = table(os.path.abspath(rest[0]) if rest else HERE)
    print("# %d kernels; %s" % (len(lines), version))
    print("\n".join(lines))
    if against:
        diff = compare(lines, open(against).read().split("\n"))
        print("\n".join(diff) if diff else "# equal to %s" % against, file=sys.stderr)
        return 1 if diff else 0
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
