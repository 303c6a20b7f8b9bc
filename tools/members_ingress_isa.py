"""Static instruction counts of ingress::k_update_members<R> (bourse_amd/csrc/members_ingress.hpp) in the shipped library.

tools/kernel_isa_counts.py::measure takes the kernels whose name starts with "k_" once "void bkd::" is stripped; this kernel
sits in a nested namespace, so it is not among them and profiles/kernel_isa_baseline.json keeps listing exactly the kernels
it listed.  The same disassembly (kernel_isa_counts.kernels_of / demangle) gives this kernel's counts and loop sizes, which
tests/test_members_ingress_isa.py compares with profiles/kernel_isa_members_ingress.json within the baseline's 3 %.
After an INTENDED change of the kernel:  python tools/members_ingress_isa.py --update

usage: members_ingress_isa.py [--update | --check] [--lib path]
"""
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_isa_counts as K  # noqa: E402

PROFILE = os.path.join(K.ROOT, "profiles", "kernel_isa_members_ingress.json")
PREFIX = "ingress::k_update_members<"


def disassemble(lib):
    """{demangled name: (counts + loops, instruction mnemonics)} of every ingress::k_update_members instantiation"""
    out = {}
    with tempfile.TemporaryDirectory(prefix="bourse_isa_") as tmp:
        for o in K.code_objects(lib, tmp):
            ks = K.kernels_of(o)
            names = K.demangle(sorted(ks))
            mine = {n: d for n, d in names.items() if d.startswith(PREFIX)}
            if not mine:
                continue
            txt = K.subprocess.run([K._tool("llvm-objdump"), "-d", o], check=True, capture_output=True, text=True).stdout
            cur, ops = None, {n: [] for n in mine}
            for line in txt.splitlines():
                m = K.SYM.match(line)
                if m:
                    if m.group(2).startswith("_Z"):
                        cur = m.group(2)
                    continue
                m = K.INS.match(line)
                if m and cur in ops:
                    ops[cur].append(m.group(1))
            for n, d in mine.items():
                out[d] = (ks[n], ops[n])
    return out


def measure(lib):
    return {d: v for d, (v, _) in sorted(disassemble(lib).items())}


def main(argv):
    lib = os.path.join(K.ROOT, "bourse_amd", "csrc", "libbourse_amd.so")
    if "--lib" in argv:
        lib = argv[argv.index("--lib") + 1]
    now = measure(lib)
    if "--update" in argv:
        json.dump({"_toolchain": K.toolchain(), "_tolerance": K.TOL,
                   "_how": "python tools/members_ingress_isa.py --update (after an intended kernel change); checked by "
                           "tests/test_members_ingress_isa.py",
                   "kernels": now}, open(PROFILE, "w"), indent=1, sort_keys=True)
        print(f"{len(now)} kernels -> {os.path.relpath(PROFILE, K.ROOT)}")
        return 0
    if "--check" in argv:
        base = json.load(open(PROFILE))
        bad = K.compare(base["kernels"], now, base.get("_tolerance", K.TOL))
        print("\n".join(bad + [f"{len(now)} kernels, {len(bad)} differences"]))
        return 1 if bad else 0
    for k, v in now.items():
        print(k, v["counts"], v["loops"][:10])
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
