#!/usr/bin/env python3
"""Instruction mix of the loops of one kernel, read from the gfx950 assembly hipcc emits.

    python tools/ws_isa_mix.py quantum_compute_dft_amd/csrc/dft_api.hip "k_rho_ws<8, true, true>"

compiles the translation unit with the library's own flags (device side only, -S) into a temporary
directory, finds every loop of the named kernel (a label that a later branch jumps back to) and prints
the instruction classes per trip.  In the wave-specialised kernels the two role loops are the loops with
four s_barrier (4x unrolled: a trip is four sub-tiles): the one with the MFMAs belongs to the matrix
waves, the one with the buffer loads to the loader waves.  Those two are printed; --all prints every
loop (the compiler splits the partial last trip into loops of its own).  Next to a saturating
fp64-MFMA wave a loader wave issues about one vector instruction per 24 cycles and one scalar
instruction per 16, which is why the length of that stream matters.

CPU only: needs hipcc and c++filt, never touches a GPU.  `--asm FILE` reads an existing .s instead.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ["total", "SALU", "v_mov", "DPP", "f64 add/mul/fma", "other VALU", "MFMA", "buffer_load", "LDS", "global", "s_waitcnt", "s_barrier"]


def build_flags():
    """The library's compile flags (quantum_compute_dft_amd/build.py), minus what only an object file needs."""
    sys.path.insert(0, ROOT)
    try:
        from quantum_compute_dft_amd.build import FLAGS
    except Exception:
        FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form"]
    return [f for f in FLAGS if f not in ("-fPIC", "-Wall", "-Wno-unused-function")]


def compile_to_asm(src, out, extra):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc] + build_flags() + extra + ["-Wno-unused-command-line-argument", "--cuda-device-only", "-S", src, "-o", out]
    subprocess.run(cmd, check=True)


def kernels(asm_lines):
    """{mangled name: (first line, last line)} of every function body."""
    out, name, start = {}, None, 0
    for i, l in enumerate(asm_lines):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            name, start = m.group(1), i + 1
        elif name and l.startswith(".Lfunc_end"):
            out[name] = (start, i)
            name = None
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.splitlines()))


def instruction(line):
    """Mnemonic and operand text of an instruction line, or None for labels, directives and comments."""
    s = line.split(";")[0].strip()
    if not s or s.endswith(":") or s.startswith("."):
        return None
    parts = s.split(None, 1)
    return parts[0], (parts[1] if len(parts) > 1 else "")


def classify(op, args):
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op == "s_barrier":
        return "s_barrier"
    if op.startswith("s_"):
        return "SALU"
    if "mfma" in op:
        return "MFMA"
    if op.startswith("buffer_load"):
        return "buffer_load"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "global"
    if op.endswith("_dpp") or re.search(r"\b(row_|quad_perm|wave_|bank_mask|row_mask)", args):
        return "DPP"
    if op.startswith("v_mov_") or op.startswith("v_accvgpr"):
        return "v_mov"
    if re.match(r"v_(add|mul|fma)_f64", op):
        return "f64 add/mul/fma"
    return "other VALU"


def loops(body):
    """[(first, last)] index ranges into `body`: from a label to the last branch that jumps back to it."""
    labels = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = i
    span = {}
    for i, l in enumerate(body):
        ins = instruction(l)
        if ins and ins[0].startswith(("s_cbranch", "s_branch")):
            t = ins[1].strip()
            if t in labels and labels[t] < i:
                span[labels[t]] = max(span.get(labels[t], 0), i)
    return sorted(span.items())


def mix(body, first, last):
    c = dict.fromkeys(CLASSES, 0)
    for l in body[first:last + 1]:
        ins = instruction(l)
        if ins:
            c[classify(*ins)] += 1
            c["total"] += 1
    return c


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source", help=".hip translation unit (ignored with --asm)")
    ap.add_argument("kernel", help="substring of the demangled kernel name, e.g. 'k_rho_ws<8, true, true>'")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--min", type=int, default=32, help="skip loops shorter than this many instructions (default 32)")
    ap.add_argument("--barriers", type=int, default=4, help="s_barrier count of one trip of a role loop (default 4: the ring depth)")
    ap.add_argument("--all", action="store_true", help="print every loop, not only one trip of each role loop")
    ap.add_argument("--flag", action="append", default=[], help="extra compiler flag (repeatable)")
    a = ap.parse_args()

    with tempfile.TemporaryDirectory() as tmp:
        path = a.asm
        if not path:
            path = os.path.join(tmp, "unit.s")
            compile_to_asm(a.source, path, a.flag)
        with open(path) as fh:
            lines = fh.read().splitlines()
    ks = kernels(lines)
    names = demangle(list(ks))
    want = a.kernel.replace(" ", "")
    hits = [n for n in ks if want in names[n].replace(" ", "")]
    if not hits:
        sys.exit(f"no kernel matches {a.kernel!r}")
    for n in hits:
        first, last = ks[n]
        body = lines[first:last]
        print(names[n])
        print("  " + " | ".join(["loop (lines)".ljust(24), "role".ljust(7)] + [c.rjust(max(len(c), 5)) for c in CLASSES]))
        rows = []
        for lo, hi in loops(body):
            c = mix(body, lo, hi)
            if c["total"] < a.min:
                continue
            role = "mixed" if c["MFMA"] and c["buffer_load"] else "MFMA" if c["MFMA"] else "loader" if c["buffer_load"] else "-"
            rows.append((role, c, f"{body[lo].split(':')[0]} ({first + lo + 1}-{first + hi + 1})"))
        if not a.all:  # one trip of each role loop: exactly --barriers barriers, the longest such loop of the role
            keep = {}
            for role, c, tag in rows:
                if role not in ("MFMA", "loader") or c["s_barrier"] != a.barriers:
                    continue
                if role not in keep or c["total"] > keep[role][1]["total"]:
                    keep[role] = (role, c, tag)
            rows = [keep[r] for r in ("loader", "MFMA") if r in keep]
        for role, c, tag in rows:
            print("  " + " | ".join([tag.ljust(24), role.ljust(7)] + [str(c[k]).rjust(max(len(k), 5)) for k in CLASSES]))


if __name__ == "__main__":
    main()
