"""Do a GEMM kernel's prefetched operands stay in flight across its MFMAs?  (host only, no GPU)

For every gfx950 kernel of libunet_hip.so whose symbol matches --match, this reads the k-loop out of
`llvm-objdump -d` and prints, per run of vector-memory loads that precedes MFMAs inside the loop:

    loads   global_load instructions of the run (the next stage's operands)
    minwait the lowest vmcnt any s_waitcnt asks for between the run's first load and the next v_mfma
            ("-": no wait at all)
    drained loads of the run that such a wait forces to return before the MFMAs start

A run is healthy when drained == 0: every wait in front of the MFMAs leaves at least as many
vector-memory operations outstanding as the run has issued so far (vmcnt counts loads and stores in
issue order, so `vmcnt(n)` with n below the number issued since the run's first load waits for that
load).  DESIGN.md §4 has the rule this checks and how the compiler breaks it (loop-carried copies).

    python tools/kloop_waits.py                       # the rows and weight-gradient GEMMs
    python tools/kloop_waits.py --match 'gemm_rows_vecILi128ELi128ELi32E.*Lb1ELb1EEEv' --json
    python tools/kloop_waits.py --asm gemm_rows.s     # a `hipcc -S --cuda-device-only` listing instead

The k-loop is the set of instructions that lie on a control-flow cycle through a v_mfma (so a peeled
last stage, the prologue and the epilogue are outside it); an unconditional s_branch met while a run
is open is followed (the compiler may place a conditional load block out of line)."""
from __future__ import annotations

import argparse
import json
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "unet-image-segmentation_amd" / "unet_amd" / "libunet_hip.so"
LLVM = Path("/opt/rocm/lib/llvm/bin")
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
DEFAULT_MATCH = r"gemm_rows_vec|gemm_wgrad_vec"
# the split-precision rows kernels launch_rows' ten (operand mode, dropout, epilogue) triples instantiate
X6_ROWS = r"gemm_rows_vecILi128ELi128ELi32ELi\d+ELb[01]ELi\d+ELb1ELb1EEEv"


def tool(name):
    p = LLVM / name
    return str(p) if p.exists() else shutil.which(name)


def code_objects(lib: Path, outdir: str):
    """Writes every gfx950 code object of the library's fat binary to outdir; their paths."""
    objcopy = tool("llvm-objcopy")
    fat = os.path.join(outdir, "fat.bin")
    # (an explicit output file: without one objcopy rewrites the library in place)
    subprocess.run([objcopy, "--dump-section", f".hip_fatbin={fat}", str(lib), os.path.join(outdir, "lib.so")],
                   check=True, capture_output=True)
    blob = open(fat, "rb").read()
    out, pos = [], 0
    while (i := blob.find(BUNDLE_MAGIC, pos)) >= 0:
        (entries,) = struct.unpack_from("<Q", blob, i + 24)
        p = i + 32
        for _ in range(entries):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" not in triple or size == 0:
                continue
            elf = os.path.join(outdir, f"co{len(out)}.elf")
            open(elf, "wb").write(blob[i + off:i + off + size])
            out.append(elf)
        pos = i + len(BUNDLE_MAGIC)
    return out


class Ins:
    __slots__ = ("op", "args", "addr", "target")

    def __init__(self, op, args, addr, target):
        self.op, self.args, self.addr, self.target = op, args, addr, target


_OBJ_SYM = re.compile(r"^[0-9a-f]+ <(\S+)>:\s*$")
_OBJ_INS = re.compile(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):")
_ASM_SYM = re.compile(r"^(_Z\w+):")
_ASM_LABEL = re.compile(r"^(\.LBB\w+):")
_ASM_INS = re.compile(r"^\t([a-z]\w+)\s*(.*?)\s*(;.*)?$")


def parse_objdump(text: str, want):
    """{symbol: [Ins]} from `llvm-objdump -d`: branch targets from the instruction's own offset."""
    out, cur = {}, None
    for line in text.splitlines():
        m = _OBJ_SYM.match(line)
        if m:
            cur = out.setdefault(m.group(1), []) if want(m.group(1)) else None
            continue
        if cur is None:
            continue
        m = _OBJ_INS.match(line)
        if not m:
            continue
        op, args, addr = m.group(1), m.group(2), int(m.group(3), 16)
        target = None
        if op.startswith(("s_branch", "s_cbranch")):
            imm = int(args.split()[0], 0) & 0xFFFF
            target = addr + 4 + 4 * (imm - 0x10000 if imm & 0x8000 else imm)
        cur.append(Ins(op, args, addr, target))
    return out


def parse_asm(text: str, want):
    """The same from a compiler listing (`-S`): instruction index as address, labels resolved."""
    out, cur, labels, fix = {}, None, {}, []
    for line in text.splitlines():
        m = _ASM_SYM.match(line)
        if m:
            cur = out.setdefault(m.group(1), []) if want(m.group(1)) else None
            continue
        if cur is None:
            continue
        m = _ASM_LABEL.match(line)
        if m:
            labels[m.group(1)] = (id(cur), len(cur))
            continue
        if line.startswith("\t.") or line.startswith(".Lfunc_end"):
            if line.startswith(".Lfunc_end"):
                cur = None
            continue
        m = _ASM_INS.match(line)
        if not m:
            continue
        ins = Ins(m.group(1), m.group(2), len(cur), None)
        if ins.op.startswith(("s_branch", "s_cbranch")):
            fix.append((id(cur), ins, ins.args.split()[0]))
        cur.append(ins)
    for owner, ins, lab in fix:
        if lab in labels and labels[lab][0] == owner:
            ins.target = labels[lab][1]
    return out


def _vmcnt(ins):
    m = re.search(r"vmcnt\((\d+)\)", ins.args)
    return int(m.group(1)) if m else None


def _succ(code, at):
    """Successor instruction indices of every instruction (fall-through and branch target)."""
    out = []
    for i, ins in enumerate(code):
        nx = []
        if ins.op not in ("s_branch", "s_endpgm") and i + 1 < len(code):
            nx.append(i + 1)
        if ins.target is not None and ins.target in at:
            nx.append(at[ins.target])
        out.append(nx)
    return out


def _reach(start, edges):
    seen, todo = set(), list(edges[start])
    while todo:
        i = todo.pop()
        if i not in seen:
            seen.add(i)
            todo.extend(edges[i])
    return seen


def kloop(code):
    """The k-loop: the instructions (indices) that lie on a cycle through a v_mfma, or None.  The
    peeled last stage, the prologue and the epilogue are on no such cycle."""
    at = {ins.addr: i for i, ins in enumerate(code)}
    fwd = _succ(code, at)
    bwd = [[] for _ in code]
    for i, nx in enumerate(fwd):
        for j in nx:
            bwd[j].append(i)
    loop, done = set(), set()
    for m in (i for i, ins in enumerate(code) if ins.op.startswith("v_mfma")):
        if m in done:
            continue
        down = _reach(m, fwd)
        if m in down:
            scc = down & _reach(m, bwd)
            loop |= scc
            done |= scc
        done.add(m)
    return loop or None


def runs(code):
    """The load runs in front of MFMAs inside the k-loop: [{loads, minwait, drained}]."""
    loop = kloop(code)
    if loop is None:
        return []
    at = {ins.addr: i for i, ins in enumerate(code)}
    out, counted = [], set()
    for i in sorted(loop):
        if i in counted or not code[i].op.startswith(("global_load", "buffer_load", "flat_load")):
            continue
        # a run opens: walk forward (through unconditional branches) to the next MFMA
        loads = issued = drained = 0
        minwait = None
        j, seen = i, set()
        while j in loop and j not in seen:
            seen.add(j)
            ins = code[j]
            if ins.op.startswith("v_mfma"):
                break
            if ins.op.startswith(("global_load", "buffer_load", "flat_load")):
                counted.add(j)
                loads += 1
                issued += 1
            elif ins.op.startswith(("global_store", "buffer_store", "flat_store", "global_atomic")):
                issued += 1
            elif ins.op == "s_waitcnt":
                n = _vmcnt(ins)
                if n is not None:
                    minwait = n if minwait is None else min(minwait, n)
                    drained = max(drained, issued - n)
            if ins.op == "s_branch":
                j = at.get(ins.target, -1)
            else:
                j += 1
        if j in loop and code[j].op.startswith("v_mfma"):
            out.append({"loads": loads, "minwait": minwait, "drained": max(drained, 0)})
    return out


def table(lib=LIB, match=DEFAULT_MATCH, asm=None):
    """{kernel symbol: [run, ...]} for the matching kernels (those that have an MFMA k-loop)."""
    rx = re.compile(match)
    want = lambda s: bool(rx.search(s))  # noqa: E731
    kernels = {}
    if asm:
        kernels = parse_asm(open(asm).read(), want)
    else:
        objdump = tool("llvm-objdump")
        with tempfile.TemporaryDirectory() as d:
            for elf in code_objects(Path(lib), d):
                text = subprocess.run([objdump, "-d", "--no-show-raw-insn", elf], check=True, capture_output=True,
                                      text=True).stdout
                kernels.update(parse_objdump(text, want))
    return {name: runs(code) for name, code in sorted(kernels.items()) if kloop(code) is not None}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--lib", default=str(LIB))
    ap.add_argument("--asm", help="a compiler listing (.s) instead of the library")
    ap.add_argument("--match", default=DEFAULT_MATCH, help="regex over kernel symbols")
    ap.add_argument("--x6-rows", action="store_true", help="only the split-precision rows kernels of launch_rows")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    t = table(a.lib, X6_ROWS if a.x6_rows else a.match, a.asm)
    if a.json:
        print(json.dumps(t, indent=1))
        return 0
    print(f"{'loads':>5} {'minwait':>7} {'drained':>7}  kernel")
    for name, rs in t.items():
        if not rs:
            print(f"{'-':>5} {'-':>7} {'-':>7}  {name}  (no load run in front of the k-loop's MFMAs)")
        for r in rs:
            mw = "-" if r["minwait"] is None else str(r["minwait"])
            print(f"{r['loads']:>5} {mw:>7} {r['drained']:>7}  {name}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
