"""Per kernel symbol: is the gfx950 machine code of a kernel file's object the same on both sides?

disasm_compare.py PARENT_CSRC TREE_CSRC FILE...   (csrc directories with build/ and build_f16/ in them)

Takes the .hip_fatbin section out of each object, unbundles the gfx950 code object, disassembles it without addresses and encodings
and compares the instruction text symbol by symbol.  One line per symbol and build; the last line counts the differing ones."""
import hashlib, os, re, subprocess, sys, tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def symbols(obj):
    with tempfile.TemporaryDirectory() as t:
        fat, co = os.path.join(t, "fatbin"), os.path.join(t, "co")
        subprocess.check_call([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(t, "unused.o")])
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               f"--input={fat}", f"--output={co}"])
        text = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^<(.+)>:$", line.strip())
        if m:
            name = m.group(1)
            out[name] = []
        elif name and line.strip():
            out[name].append(re.sub(r"\s*//.*$", "", line).strip())
    return out


def main():
    parent, tree, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    differing = total = 0
    for build in ("build", "build_f16"):
        for f in files:
            a, b = symbols(f"{parent}/{build}/{f}.o"), symbols(f"{tree}/{build}/{f}.o")
            for name in sorted(set(a) | set(b)):
                ia, ib = a.get(name), b.get(name)
                same = ia == ib
                total += 1
                differing += not same
                h = hashlib.sha256("\n".join(ib or []).encode()).hexdigest()[:12]
                print(f"{build}/{f}.o {name} instructions parent {len(ia) if ia is not None else 'absent'} tree "
                      f"{len(ib) if ib is not None else 'absent'} sha {h} {'same' if same else 'DIFFERENT'}")
    print(f"# {total} kernel symbols compared, differing: {differing}")


main()
