#!/usr/bin/env python
"""Per-kernel register / scratch / code-size table from the compiler alone.

Compiles the two device TUs (csrc/hip/*.hip) device-only with setup.py's
flags plus -Rpass-analysis=kernel-resource-usage and prints one markdown
table per file: VGPRs, VGPR/SGPR spills, ScratchSize, LDS, occupancy and
code size of every kernel.  No GPU needed.  Reads the compiler's resource
remarks and the code object's symbol sizes only.

A jump in ScratchSize with no change in spills is a private-memory slot
(a run-time-indexed local array or struct copy, e.g. the 128-byte BVH4 node
copy before the child words were selected from registers) — cheap to see
here, expensive to find on the GPU.

    python scripts/kernel_resources.py                # this tree
    python scripts/kernel_resources.py --root OTHER   # another checkout
    python scripts/kernel_resources.py --filter k_render
"""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

HIP_SOURCES = ["csrc/hip/pt_kernels.hip", "csrc/hip/wf_kernels.hip"]

FIELDS = [  # (remark label prefix, column)
    ("VGPRs:", "VGPR"),
    ("AGPRs:", "AGPR"),
    ("VGPRs Spill:", "VGPR spill"),
    ("SGPRs Spill:", "SGPR spill"),
    ("ScratchSize [bytes/lane]:", "scratch B/lane"),
    ("LDS Size [bytes/block]:", "LDS B"),
    ("Occupancy [waves/SIMD]:", "occ"),
]


def load_setup(root: Path):
    spec = importlib.util.spec_from_file_location("_hippt_setup", root / "setup.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def llvm_tool(hipcc: str, name: str) -> str:
    out = subprocess.run([hipcc, f"-print-prog-name={name}"],
                         capture_output=True, text=True).stdout.strip()
    if out and os.path.isfile(out):
        return out
    beside = Path(hipcc).resolve().parent.parent / "lib" / "llvm" / "bin" / name
    return str(beside) if beside.is_file() else name


def parse_remarks(text: str):
    """{mangled name: {column: int}} from kernel-resource-usage remarks."""
    res, cur = {}, None
    for line in text.splitlines():
        if "remark:" not in line:
            continue
        body = line.split("remark:", 1)[1]
        body = re.sub(r"\s*\[-Rpass-analysis=[^\]]*\]\s*$", "", body)
        # drop the "file:line:col:" location in front of the message
        body = re.sub(r"^\s*\S+:\d+:\d+:\s*", "", body).strip()
        if body.startswith("Function Name:"):
            cur = body.split(":", 1)[1].strip()
            res[cur] = {}
            continue
        if cur is None:
            continue
        for label, col in FIELDS:
            if body.startswith(label):
                val = body[len(label):].strip()
                if val.lstrip("-").isdigit():
                    res[cur][col] = int(val)
                break
    return res


def function_symbols(objdump: str, obj: Path, demangled: bool):
    """{address: (name, bytes)} for the function symbols of a code object
    (symbol table only)."""
    cmd = [objdump, "-t", str(obj)] + (["-C"] if demangled else [])
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
    syms = {}
    for line in out.splitlines():
        m = re.match(r"^([0-9a-f]{16})\s.{7}\s+(\.text\S*)\s+([0-9a-f]{16})\s+(.*)$", line)
        if m and "F" in line[17:24]:
            name = re.sub(r"^\.(hidden|protected|internal)\s+", "", m.group(4))
            syms[int(m.group(1), 16)] = (name, int(m.group(3), 16))
    return syms


def symbol_tables(objdump: str, obj: Path):
    """({mangled: bytes}, {mangled: demangled}) of the kernels' code."""
    raw = function_symbols(objdump, obj, False)
    nice = function_symbols(objdump, obj, True)
    sizes = {name: size for name, size in raw.values()}
    names = {raw[a][0]: nice[a][0] for a in raw if a in nice}
    return sizes, names


def short(name: str) -> str:
    name = re.sub(r"^void\s+", "", name).replace("hippt::", "")
    return re.sub(r"\(.*$", "", name)  # drop the parameter list


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent),
                    help="checkout to compile (default: this one)")
    ap.add_argument("--filter", default="", help="only kernels whose name contains this")
    args = ap.parse_args()
    root = Path(args.root).resolve()
    # flags always come from this tree's setup.py, so two checkouts compare
    # like for like
    setup = load_setup(Path(__file__).resolve().parent.parent)
    cflags, _ = setup.compile_flags()
    cflags = [f for f in cflags if f != "-fPIC" and not f.startswith("-fsanitize")
              and f != "-shared-libasan"]
    objdump = llvm_tool(setup.HIPCC, "llvm-objdump")
    cols = [c for _, c in FIELDS] + ["code B"]
    with tempfile.TemporaryDirectory() as tmp:
        jobs = []
        for src in HIP_SOURCES:
            obj = Path(tmp) / (Path(src).stem + ".co")
            cmd = [setup.HIPCC, "-x", "hip", "-c", str(root / src), "-o", str(obj),
                   "--cuda-device-only", "--no-gpu-bundle-output",
                   "-Rpass-analysis=kernel-resource-usage"] + cflags
            jobs.append((src, obj, subprocess.Popen(
                cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        for src, obj, p in jobs:
            log, _ = p.communicate()
            if p.returncode != 0:
                sys.stderr.write(log)
                raise SystemExit(f"hipcc failed on {src}")
            res = parse_remarks(log)
            sizes, names = symbol_tables(objdump, obj)
            names = {m: names.get(m, m) for m in res}
            print(f"### {src} ({setup.ARCH})\n")
            print("| kernel | " + " | ".join(cols) + " |")
            print("|---|" + "---|" * len(cols))
            for mangled in sorted(res, key=lambda m: short(names[m])):
                nice = short(names[mangled])
                if args.filter and args.filter not in nice:
                    continue
                row = dict(res[mangled])
                row["code B"] = sizes.get(mangled, "")
                print(f"| `{nice}` | " + " | ".join(str(row.get(c, "")) for c in cols) + " |")
            print()


if __name__ == "__main__":
    main()
