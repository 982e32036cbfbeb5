#!/usr/bin/env python3
"""Per-symbol comparison of the gfx950 code of two builds of libcodae_hip.so (check_isa.py's disassemble / functions): the proof
a refactor asks for when it claims that the shipped kernels did not change.

Usage: python tools/isa_diff.py OLD.so NEW.so [--kernarg]
  default    a symbol differs when any mnemonic or operand does.  The literal of the s_add_u32 / s_addc_u32 pair behind an
             s_getpc_b64 (the pc-relative address of a global) is not compared: it moves with the code object's layout.
  --kernarg  also ignores the immediate offset of s_load_* instructions (a field left a by-value kernel argument struct and
             everything behind it moved); the mnemonic sequence must still be identical.
Prints the symbol counts, the symbols only one library has, and the symbols that differ (first differing instruction).
Exit code 0 = every common symbol is the same under the chosen rule."""
import re
import sys

from check_isa import disassemble, functions


def normalise(insns, kernarg):
    out, pc_rel = [], 0
    for _, op, args in insns:
        if op == "s_getpc_b64":
            pc_rel = 2
        elif pc_rel and op in ("s_add_u32", "s_addc_u32"):
            args = re.sub(r"(0x[0-9a-fA-F]+|\d+)\s*$", "LIT", args)
            pc_rel -= 1
        if kernarg and op.startswith("s_load_"):
            args = re.sub(r"(0x[0-9a-fA-F]+|\d+)\s*$", "OFF", args)
        out.append((op, args))
    return out


def main():
    kernarg = "--kernarg" in sys.argv
    old_lib, new_lib = [a for a in sys.argv[1:] if not a.startswith("--")]
    old, new = functions(disassemble(old_lib)), functions(disassemble(new_lib))
    pipe = lambda f: sum(1 for n in f if "gemm_bf16_pipe_kernel" in n)
    print("symbols: old %d, new %d; gemm_bf16_pipe_kernel instantiations: old %d, new %d" % (len(old), len(new), pipe(old), pipe(new)))
    for title, names in (("only in old", sorted(set(old) - set(new))), ("only in new", sorted(set(new) - set(old)))):
        print("%s: %d" % (title, len(names)))
        for n in names:
            print("    " + n)
    differing = 0
    for n in sorted(set(old) & set(new)):
        a, b = normalise(old[n], kernarg), normalise(new[n], kernarg)
        if a == b:
            continue
        differing += 1
        same_ops = [x[0] for x in a] == [x[0] for x in b]
        i = next((k for k, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        print("DIFFERS %s: %d vs %d instructions, mnemonic sequence %s; first at #%d: %s | %s" %
              (n, len(a), len(b), "same" if same_ops else "CHANGED", i, " ".join(a[i]) if i < len(a) else "-", " ".join(b[i]) if i < len(b) else "-"))
    print("common symbols: %d, differing (%s): %d" % (len(set(old) & set(new)), "operands but kernel-argument offsets" if kernarg else "any operand", differing))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
