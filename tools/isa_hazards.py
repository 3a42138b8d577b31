#!/usr/bin/env python3
"""Wait-state audit of gfx950 device assembly: the hazards hipcc pads in its own code and not inside an `asm` string.

hipcc's hazard recogniser inserts `s_nop`s between a producer and a consumer that the hardware does not interlock; the text of an
inline-asm statement (between `;;#ASMSTART` and `;;#ASMEND` in the `-S` output) is opaque to it and gets none.  This reads the
assembly, follows every path forward from each producer — fall-through, branch targets, loop back-edges — and reports each
consumer reached before the rule's wait states are spent (`s_nop N` is N + 1 states, any other instruction 1, a label 0).

The rules are the ones of the CDNA3/CDNA4 ISA's "manually inserted wait states" table that apply to what the product's asm contains.
Each is held to the toolchain by a probe in tests/test_isa_hazards.py: a HIP kernel whose hipcc output pads that pair (so no rule is
stricter than hipcc), and the same pair written unpadded in an asm string (so the checker finds it).  Instructions for which no rule
here is calibrated — a VALU write of EXEC, a write of M0 — are reported by `uncovered()` when they appear inside an asm string.

    python tools/isa_hazards.py [--build] [file.s ...]     # --build: make -C voxelraytracing_amd/csrc asm into a temp dir
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from dataclasses import dataclass, field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "voxelraytracing_amd", "csrc")
PRODUCT_UNITS = ("vrt_kernels", "vrt_path", "vrt_accel", "vrt_lit", "vrt_denoise") # the translation units with kernels that ship in libvrt.so
EXPERIMENT_UNITS = ()   # none is left (csrc/experiments/ is deleted); the name stays for code written against this module that adds the two

_REG = re.compile(r"(?<![\w.])(v|s|a)(\d+)\b|(?<![\w.])(v|s|a)\[(\d+):(\d+)\]|\b(vcc|exec|vcc_lo|vcc_hi|exec_lo|exec_hi|m0|scc)\b")
_PAIRS = {"vcc": ("vcc_lo", "vcc_hi"), "exec": ("exec_lo", "exec_hi")}
# VOP3b: a vector destination and a scalar one (carry, or a scale's flag)
_VOP3B = re.compile(r"^v_(add|sub|subrev|addc|subb|subbrev)_co_u32|^v_div_scale_|^v_mad_(u64_u32|i64_i32)")
_VMEM = re.compile(r"^(buffer|global|flat|scratch|tbuffer)_")
_STORE = re.compile(r"^(buffer|global|flat|scratch|tbuffer)_store|^ds_write|^s_store|^s_buffer_store")
_TRANS = re.compile(r"^v_(exp|log|rcp|rsq|sqrt|sin|cos)(_legacy)?_f(16|32|64)|^v_rcp_iflag_f32|^v_(exp|log)_legacy_f32")
_READLANE = re.compile(r"^v_read(first)?lane_b32")
_WRITELANE = re.compile(r"^v_writelane_b32")
_LABEL = re.compile(r"^([.\w$]+):")


def _regs(text):
    """The 32-bit registers an operand string names: 'v3', 's4', 'vcc_lo', ... (s[4:5] -> s4 s5; vcc -> vcc_lo vcc_hi)."""
    out = []
    for m in _REG.finditer(text):
        if m.group(1):
            out.append(f"{m.group(1)}{m.group(2)}")
        elif m.group(3):
            out += [f"{m.group(3)}{i}" for i in range(int(m.group(4)), int(m.group(5)) + 1)]
        else:
            out += list(_PAIRS.get(m.group(6), (m.group(6),)))
    return out


def _is_sgpr(r):
    return r[0] == "s" and r[1:].isdigit() or r.startswith("vcc")


@dataclass
class Insn:
    idx: int
    line: int
    op: str
    text: str
    in_asm: bool
    defs: tuple = ()
    uses: tuple = ()          # every register read
    operands: tuple = ()      # the operand strings as written (uses by position)
    target: str = None        # a branch's label

    @property
    def is_valu(self):
        return self.op.startswith("v_")

    @property
    def is_vmem(self):
        return bool(_VMEM.match(self.op))

    def states(self):
        if self.op == "s_nop":
            return int(self.operands[0], 0) + 1
        return 1


def _split_operands(rest):
    ops, depth, cur = [], 0, ""
    for ch in rest:
        if ch == "[":
            depth += 1
        elif ch == "]":
            depth -= 1
        if ch == "," and depth == 0:
            ops.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        ops.append(cur.strip())
    return ops


def _decode(idx, line, op, rest, in_asm):
    operands = tuple(_split_operands(rest))
    defs, uses = [], []
    regs = [_regs(o) for o in operands]
    no_dst = (_STORE.match(op) or op.startswith(("s_cmp", "s_bitcmp", "s_cbranch", "s_branch", "s_waitcnt", "s_nop", "s_setprio",
                                                 "s_endpgm", "s_barrier", "s_sendmsg", "s_setpc", "s_trap", "s_sleep", "s_dcache")))
    if operands and not no_dst:
        defs += regs[0]
        uses_from = 1
        if _VOP3B.match(op) and len(operands) > 1 and all(_is_sgpr(r) for r in regs[1]) and regs[1]:
            defs += regs[1]
            uses_from = 2
        for r in regs[uses_from:]:
            uses += r
    else:
        for r in regs:
            uses += r
    if op.startswith("s_") and "saveexec" in op:
        defs += ["exec_lo", "exec_hi"]
        uses += ["exec_lo", "exec_hi"]
    if op.startswith("v_cmpx"):
        defs += ["exec_lo", "exec_hi"]
    if op.startswith("v_div_fmas"):
        uses += ["vcc_lo", "vcc_hi"]
    if op in ("s_cbranch_vccz", "s_cbranch_vccnz"):
        uses += ["vcc_lo", "vcc_hi"]
    target = operands[0] if op == "s_branch" or op.startswith("s_cbranch") else None
    return Insn(idx, line, op, f"{op} {rest}".strip(), in_asm, tuple(defs), tuple(uses), operands, target)


@dataclass
class Function:
    name: str
    insns: list = field(default_factory=list)
    labels: dict = field(default_factory=dict)   # label -> index of the next instruction


def parse(text):
    """The functions of one `-S` file: instructions with their registers, labels, and which lie inside an asm string."""
    funcs, fn, in_asm = [], None, False
    for ln, raw in enumerate(text.splitlines(), 1):
        s = raw.strip()
        if s.startswith(";;#ASMSTART"):
            in_asm = True
            continue
        if s.startswith(";;#ASMEND"):
            in_asm = False
            continue
        s = s.split(";", 1)[0].strip()
        if not s:
            continue
        m = _LABEL.match(s)
        if m:
            name = m.group(1)
            if not name.startswith("."):
                fn = Function(name)
                funcs.append(fn)
            elif fn is not None:
                fn.labels[name] = len(fn.insns)
            s = s[m.end():].strip()
            if not s:
                continue
        if fn is None or s.startswith("."):   # directives
            continue
        op, _, rest = s.partition(" ")
        if not re.match(r"^[a-z][a-z0-9_]*$", op):
            continue
        fn.insns.append(_decode(len(fn.insns), ln, op, rest.strip(), in_asm))
    return [f for f in funcs if f.insns]


def _successors(fn, i):
    ins = fn.insns[i]
    if ins.op in ("s_endpgm", "s_setpc_b64", "s_swappc_b64", "s_trap", "s_endpgm_saved"):
        return []
    out = []
    if ins.target is not None:
        t = fn.labels.get(ins.target)
        if t is not None:
            out.append(t)
        if ins.op == "s_branch":
            return out
    if i + 1 < len(fn.insns):
        out.append(i + 1)
    return out


# ---- the rules: (name, need, producer test -> the registers it hands on, consumer test(insn, reg) -> reads it in that role) ----
def _valu_sgpr_defs(p):
    return [r for r in p.defs if _is_sgpr(r)] if p.is_valu else []


def _lane_select(c):
    if _READLANE.match(c.op) and c.op != "v_readfirstlane_b32" and len(c.operands) > 2:
        return _regs(c.operands[2])
    if _WRITELANE.match(c.op) and len(c.operands) > 2:
        return _regs(c.operands[2])
    return []


@dataclass(frozen=True)
class Rule:
    name: str
    need: int
    what: str
    produces: object
    consumes: object


RULES = (
    Rule("valu_sgpr_valu", 2, "VALU writes an SGPR or VCC, a VALU reads it",
         _valu_sgpr_defs, lambda c, r: c.is_valu and r in c.uses and r not in _lane_select(c)),
    Rule("valu_sgpr_lanesel", 4, "VALU writes an SGPR, v_readlane/v_writelane takes it as the lane select",
         _valu_sgpr_defs, lambda c, r: r in _lane_select(c)),
    Rule("valu_sgpr_vmem", 5, "VALU writes an SGPR, a VMEM instruction reads it (address, descriptor, offset)",
         lambda p: [r for r in _valu_sgpr_defs(p) if r[0] == "s"], lambda c, r: c.is_vmem and r in c.uses),
    Rule("valu_vgpr_readlane", 1, "VALU writes a VGPR, v_readlane/v_readfirstlane reads it",
         lambda p: [r for r in p.defs if r[0] == "v" and r[1:].isdigit()] if p.is_valu else [],
         lambda c, r: bool(_READLANE.match(c.op)) and len(c.operands) > 1 and r in _regs(c.operands[1])),
    Rule("trans_valu", 1, "a transcendental VALU op writes a VGPR, a non-transcendental VALU reads it",
         lambda p: [r for r in p.defs if r[0] == "v" and r[1:].isdigit()] if _TRANS.match(p.op) else [],
         lambda c, r: c.is_valu and not _TRANS.match(c.op) and r in c.uses),
)


@dataclass
class Finding:
    rule: str
    function: str
    producer: Insn
    consumer: Insn
    found: int
    need: int

    @property
    def in_asm(self):
        return self.producer.in_asm or self.consumer.in_asm

    @property
    def violation(self):
        return self.found < self.need

    def __str__(self):
        where = "inline asm" if self.in_asm else "compiler code"
        return (f"[{self.rule}] {self.function}: {self.producer.text!r} (line {self.producer.line}) -> {self.consumer.text!r} "
                f"(line {self.consumer.line}): {self.found} wait state(s), needs {self.need} ({where})")


def scan(funcs, rules=RULES, horizon=None):
    """Every producer -> consumer pair of each rule met within `horizon` wait states (default: the rule's own count, i.e. the
    violations), the fewest states over all paths.  A path ends where any instruction writes the register again."""
    out = []
    for fn in funcs:
        for rule in rules:
            lim = rule.need if horizon is None else horizon
            for p in fn.insns:
                best = {}   # consumer -> the fewest states to it, over the producer's registers and all paths
                for reg in sorted(set(rule.produces(p))):
                    stack = [(s, 0) for s in _successors(fn, p.idx)]
                    seen = set()
                    while stack:
                        j, spent = stack.pop()
                        if (j, spent) in seen:
                            continue
                        seen.add((j, spent))
                        c = fn.insns[j]
                        if rule.consumes(c, reg) and (j not in best or spent < best[j]):
                            best[j] = spent
                        if reg in c.defs:
                            continue
                        spent += c.states()
                        if spent >= lim:
                            continue
                        stack += [(s, spent) for s in _successors(fn, j)]
                for j, spent in sorted(best.items()):
                    out.append(Finding(rule.name, fn.name, p, fn.insns[j], spent, rule.need))
    return out


def violations(funcs):
    return [f for f in scan(funcs) if f.violation]


def uncovered(funcs):
    """Instructions inside asm strings that no rule here is calibrated for: a VALU write of EXEC, any write of M0."""
    return [(fn.name, i) for fn in funcs for i in fn.insns
            if i.in_asm and ((i.is_valu and ("exec_lo" in i.defs or "exec_hi" in i.defs)) or "m0" in i.defs)]


def hipflags():
    """The Makefile's HIPFLAGS (one source of truth for the flags the product is compiled with)."""
    return subprocess.check_output(["make", "-s", "--no-print-directory", "-C", CSRC, "print-hipflags"], text=True).split()


def build_asm(outdir):
    """make asm: the device assembly of every translation unit with kernels, into outdir; {unit: path}."""
    subprocess.check_call(["make", "-s", "--no-print-directory", "-C", CSRC, "asm", f"ASMDIR={os.path.abspath(outdir)}"],
                          stdout=subprocess.DEVNULL)
    return {u: os.path.join(outdir, u + ".s") for u in PRODUCT_UNITS}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("files", nargs="*", help="-S output to scan")
    ap.add_argument("--build", action="store_true", help="build the product's assembly (make asm) and scan it")
    a = ap.parse_args(argv)
    files = {os.path.splitext(os.path.basename(f))[0]: f for f in a.files}
    tmp = None
    if a.build:
        tmp = tempfile.TemporaryDirectory()
        files.update(build_asm(tmp.name))
    if not files:
        ap.error("no assembly: name -S files or pass --build")
    failed = False
    for unit, path in files.items():
        with open(path) as f:
            funcs = parse(f.read())
        vs = violations(funcs)
        asm = [v for v in vs if v.in_asm]
        print(f"{unit}: {len(funcs)} functions, {sum(len(fn.insns) for fn in funcs)} instructions; "
              f"{len(asm)} violation(s) inside inline asm, {len(vs) - len(asm)} in compiler code")
        for v in vs:
            print("  " + str(v))
        for fname, i in uncovered(funcs):
            print(f"  [uncovered] {fname}: {i.text!r} (line {i.line}): no rule here is calibrated for it")
        failed |= bool(vs or uncovered(funcs))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
