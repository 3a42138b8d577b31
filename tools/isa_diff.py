"""tools/isa_diff.py — the gfx950 instruction streams of two builds of libvrt.so, kernel by kernel (no GPU).

    python tools/isa_diff.py OLD.so NEW.so [--rename NEW_REGEX=OLD_REPL ...] [--rename-file FILE]

Every kernel of OLD is looked up in NEW (after the --rename substitutions, applied to NEW's symbol names: a template argument
that a later build added with its old value as the default; --rename-file: one REGEX=REPL per line, # comments) and their bodies are compared instruction for instruction, with
what legitimately differs between two links left out: addresses, raw encodings, comments, symbolic branch labels.  Prints
one line per kernel that differs or is missing and a summary; exit status 1 if any kernel of OLD differs or is missing.
Under a kernel that differs, its hand-written march loops (vrt_march.h VRT_MARCH_LOOP: from `s_setprio 1` to `s_setprio 0`) are
compared on their own with the register numbers left out — the compiler allocates an asm statement's operands anew when the code
around it changes.  The disassembler's "..." for zero padding behind a function is not an instruction."""
import argparse
import os
import re
import struct
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def code_objects(path):
    """The gfx950 code objects of a HIP shared library's .hip_fatbin (one bundle per translation unit)."""
    data = open(path, "rb").read()
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    names = sec[shstrndx]
    fat = b""
    for s in sec:
        if data[names[4] + s[0]:data.index(b"\0", names[4] + s[0])] == b".hip_fatbin":
            fat = data[s[4]:s[4] + s[5]]
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    at = fat.find(magic)
    while at >= 0:
        count, = struct.unpack_from("<Q", fat, at + 24)
        q = at + 32
        for _ in range(count):
            off, size, tl = struct.unpack_from("<QQQ", fat, q)
            triple = fat[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            if "gfx950" in triple and size:
                yield fat[at + off:at + off + size]
        at = fat.find(magic, at + 24)


def kernels(path):
    """{symbol: [normalised instruction lines]} of every function in the library's gfx950 code objects."""
    out = {}
    for co in code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", f.name], capture_output=True,
                                  text=True, check=True).stdout
        cur = None
        for line in text.splitlines():
            m = re.match(r"^(?:[0-9a-f]+ )?<(\S+)>:$", line)
            if m:
                cur = out.setdefault(m.group(1), [])
                continue
            if cur is None:
                continue
            ins = re.sub(r"//.*$", "", line)
            ins = re.sub(r"<[^>]*>", "", ins).strip()
            if ins and ins != "...":   # ("...": the disassembler's word for zero padding behind a function, not an instruction)
                cur.append(" ".join(ins.split()))
    return out


def asm_loops(body):
    """The instruction sequences between `s_setprio 1` and `s_setprio 0`, register numbers left out."""
    out, cur = [], None
    for ins in body:
        if ins.startswith("s_setprio 1"):
            cur = []
        if cur is not None:
            cur.append(re.sub(r"\b[vs]\[?\d+(:\d+)?\]?", "R", ins))
        if ins.startswith("s_setprio 0") and cur is not None:
            out.append(cur)
            cur = None
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], help="REGEX=REPL applied to NEW's symbols before the lookup")
    ap.add_argument("--rename-file", help="a file of REGEX=REPL lines, applied after the --rename ones (blank lines and # comments skipped)")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    renames = list(a.rename)
    if a.rename_file:
        renames += [ln.strip() for ln in open(a.rename_file) if ln.strip() and not ln.lstrip().startswith("#")]
    subs = [r.split("=", 1) for r in renames]
    renamed = {}
    for sym, body in new.items():
        k = sym
        for pat, repl in subs:
            k = re.sub(pat, repl, k)
        renamed.setdefault(k, (sym, body))
    same = differ = missing = 0
    for sym, body in sorted(old.items()):
        if sym not in renamed:
            print(f"MISSING  {sym}")
            missing += 1
            continue
        nsym, nbody = renamed[sym]
        if nbody == body:
            same += 1
            continue
        differ += 1
        n = sum(1 for x, y in zip(body, nbody) if x != y) + abs(len(body) - len(nbody))
        print(f"DIFFERS  {sym} -> {nsym}: {len(body)} vs {len(nbody)} instructions, {n} lines differ")
        lo, ln = asm_loops(body), asm_loops(nbody)
        if lo or ln:
            print(f"         march loops (s_setprio 1 .. s_setprio 0), instructions: {[len(x) for x in lo]} vs {[len(x) for x in ln]}; "
                  f"{'the same sequences, register numbers left out' if lo == ln else 'THEY DIFFER'}")
    extra = sorted(s for s in new if s not in {renamed[k][0] for k in old if k in renamed})
    for s in extra:
        print(f"NEW      {s} ({len(new[s])} instructions)")
    print(f"{os.path.basename(a.old)} -> {os.path.basename(a.new)}: {len(old)} functions before, {same} identical, {differ} differ, "
          f"{missing} missing; {len(extra)} new")
    return 1 if differ or missing else 0


if __name__ == "__main__":
    sys.exit(main())
