"""Per-kernel diff of the gfx950 device code of two builds of the library: the
check that a refactor of a kernel's source leaves the machine code alone.

    python tools/isa_diff.py OLD.so NEW.so

For every kernel symbol of either library it compares the instruction text
(addresses and encodings stripped; a branch keeps its pc-relative operand and
its <kernel+offset> target, and a pc-relative literal that reaches read-only
data is replaced by the address it forms, or by the name of the out-of-line
device function it reaches, and the s_nop padding behind a kernel is dropped,
so a kernel that grew or a function that left does not mark the others) and
the scalar fields of the kernel's entry in the code object's metadata
note (VGPR/SGPR/AGPR counts, LDS, scratch, kernarg size, spills...).  Prints
the kernels added, removed and changed; exits 1 if there are any.  Runs on
the CPU with the ROCm llvm tools (the unbundling is isa_scan's)."""
import re
import subprocess
import sys

import isa_scan


def kernels(so: str) -> dict:
    """{kernel symbol: (instruction lines, {metadata field: value})}"""
    out = {}
    for co in isa_scan.code_objects(so):
        meta, cur = {}, None
        note = subprocess.run([f"{isa_scan.LLVM}/llvm-readelf", "--notes", co],
                              capture_output=True, text=True, check=True).stdout
        for line in note.splitlines():
            if line.startswith("  - "):  # the next entry of amdhsa.kernels
                cur, line = {}, "    " + line[4:]
            m = re.match(r"^    \.(\w+):\s+(\S+)$", line)
            if m and cur is not None:
                cur[m.group(1)] = m.group(2)
                if m.group(1) == "name":
                    meta[m.group(2)] = cur
        # a literal that reaches a function of the code object (a call of a
        # device function kept out of line) is named after it: the function
        # moves when the code object's other contents change size
        syms = subprocess.run([f"{isa_scan.LLVM}/llvm-readelf", "-sW", co],
                              capture_output=True, text=True, check=True).stdout
        funcs = {int(m.group(1), 16): m.group(2) for m in
                 re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+\d+\s+FUNC\s.*\s(\S+)$", syms, re.M)}
        for fn, lines in isa_scan.disassembly(co).items():
            text, pc = [], None
            for line in lines:
                insn, _, rest = line.partition("//")
                insn = insn.strip()
                if not insn:
                    continue
                addr, target = re.match(r"\s*([0-9A-F]+):", rest), re.search(r"<.+>$", rest)
                # s_getpc_b64 + s_add_u32 literal reaches data outside the kernel:
                # the literal moves with the kernel, the address it forms does not
                lit = re.match(r"(s_add_u32 .+, )(0x[0-9a-f]+)$", insn) if pc else None
                if lit:
                    to = (pc + int(lit.group(2), 16)) & 0xffffffff
                    insn = f"{lit.group(1)}<{funcs.get(to, hex(to))}>"
                pc = int(addr.group(1), 16) + 4 if insn.startswith("s_getpc_b64") and addr else None
                text.append(insn + (" " + target.group(0) if target else ""))
            while text and text[-1] in ("s_nop 0", "..."):  # the padding up to the next function
                text.pop()
            out[fn] = (text, meta.get(fn, {}))
    return out


def main(old_so: str, new_so: str) -> int:
    old, new = kernels(old_so), kernels(new_so)
    added, removed = sorted(set(new) - set(old)), sorted(set(old) - set(new))
    changed = sorted(fn for fn in set(old) & set(new) if old[fn] != new[fn])
    for what, fns in (("added", added), ("removed", removed)):
        for fn in fns:
            print(f"{what}: {fn}")
    for fn in changed:
        (ti, mi), (tj, mj) = old[fn], new[fn]
        fields = [f"{k} {mi.get(k)} -> {mj.get(k)}" for k in sorted(set(mi) | set(mj))
                  if mi.get(k) != mj.get(k)]
        first = next((n for n, (x, y) in enumerate(zip(ti, tj)) if x != y), min(len(ti), len(tj)))
        code = "" if ti == tj else f"{len(ti)} -> {len(tj)} instructions, first at {first}"
        print(f"changed: {fn}: " + "; ".join(filter(None, [code] + fields)))
    print(f"{len(old)} -> {len(new)} kernels: {len(added)} added, {len(removed)} removed, "
          f"{len(changed)} changed")
    return 1 if added or removed or changed else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
