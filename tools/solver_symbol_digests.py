"""solver_symbol_digests.py PARENT_DIR CHANGE_DIR [OBJECT...]: per-kernel digests of the gfx950 code objects of the solver
objects (default vigo_solver.hip.o, vigo_solver_obs.o) in two build directories, the method of
profiles/axis_const_symbol_digests.tsv: llvm-objdump -d of the code object, addresses and encodings stripped, sha256 per
symbol.  Needs no GPU.  A kernel is matched by its demangled name, a trailing template argument that only the change
spells out (the MIXED = false of k_optimize / k_cost_grad) dropped.  Prints the table; exits 1 if a kernel of the parent is
missing from the change or differs.
solver_symbol_digests.py --figures OBJECT: the code-object figures of every kernel of one object instead (the notes of its
gfx950 code object): VGPRs, AGPRs, SGPRs, spilled VGPRs / SGPRs, scratch and static LDS bytes, instructions."""
import hashlib, os, re, subprocess, sys, tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def code_object(obj, notes=False):   # the gfx950 ELF inside the object's .hip_fatbin (build_id.py reads the same bundle)
    with tempfile.TemporaryDirectory() as d:
        fat, out = os.path.join(d, "fatbin"), os.path.join(d, "gfx950.co")
        subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", f"--output={out}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True)
        tool = [f"{LLVM}/llvm-readelf", "--notes", out] if notes else [f"{LLVM}/llvm-objdump", "-d", "-C", "--no-show-raw-insn", "--no-leading-addr", out]
        return subprocess.run(tool, check=True, capture_output=True, text=True).stdout


def figures(obj):
    fields = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
              ".group_segment_fixed_size")
    insns = {mangled_free: v[0] for mangled_free, v in kernels(obj).items()}
    print("# kernel\tVGPRs\tAGPRs\tSGPRs\tVGPR spills\tSGPR spills\tscratch B\tstatic LDS B\tinstructions")
    rows = []
    for block in code_object(obj, notes=True).split("  - .agpr_count")[1:]:
        block = ".agpr_count" + block
        get = lambda f: re.search(re.escape(f) + r":\s*(\S+)", block).group(1)
        name = subprocess.run(["c++filt", get(".name")], check=True, capture_output=True, text=True).stdout.strip()   # (binutils)
        name = re.sub(r"^void vigo::\(anonymous namespace\)::|\((vigo::SolveArgs|std::conditional<).*$", "", name)
        rows.append("\t".join([name] + [get(f) for f in fields] + [str(insns.get(name, "-"))]))
    print("\n".join(sorted(rows)))


def kernels(obj):   # demangled kernel name -> (instructions, digest)
    out, name, body = {}, None, []
    def close():
        if name and "k_" in name:
            out[name] = (len(body), hashlib.sha256("\n".join(body).encode()).hexdigest()[:16])
    for line in code_object(obj).splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.*)>:$", line)
        if m:
            close()
            # "void vigo::(anonymous namespace)::k_x<...>(vigo::SolveArgs, ...)" -> "k_x<...>"
            name, body = re.sub(r"^void vigo::\(anonymous namespace\)::|\((vigo::SolveArgs|std::conditional<).*$", "", m.group(1)), []
        elif name and line.strip() and line.strip() != "...":   # ("...": zero fill up to the next symbol's alignment, no code)
            body.append(re.sub(r"\s*//.*$", "", line).strip())   # (the comment holds the address and the encoding)
    close()
    return out


def key(name):   # the change's spelled-out default arguments
    return re.sub(r", false>$", ">", name) if name.startswith(("k_optimize<", "k_cost_grad<")) else name


def main():
    if sys.argv[1] == "--figures":
        return figures(sys.argv[2])
    parent, change = sys.argv[1], sys.argv[2]
    objs = sys.argv[3:] or ["vigo_solver.hip.o", "vigo_solver_obs.o"]
    bad = 0
    print("# object\tinstructions parent\tdigest parent\tinstructions change\tdigest change\tsame\tkernel")
    for o in objs:
        a = kernels(os.path.join(parent, o))
        b = kernels(os.path.join(change, o))
        if not set(a) <= set(b):     # (a parent from before MIXED: its names lack the argument)
            b = {key(k): v for k, v in b.items()}
        for name in sorted(a):
            got = b.get(name)
            same = got == a[name]
            bad += 0 if same else 1
            print(f"{o}\t{a[name][0]}\t{a[name][1]}\t{got[0] if got else '-'}\t{got[1] if got else '-'}\t{'yes' if same else 'NO'}\t{name}")
        for name in sorted(set(b) - set(a)):
            print(f"{o}\t-\t-\t{b[name][0]}\t{b[name][1]}\tnew\t{name}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
