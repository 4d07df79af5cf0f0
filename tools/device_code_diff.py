"""No GPU: do two sets of objects hold the same gfx950 kernels?  For a change that moves kernels between sources (or touches only
host code) every kernel must come out of the compiler as it went in.  usage: device_code_diff.py DIR_A DIR_B [--arch gfx950]

Each directory holds the objects of one tree: `hipcc --cuda-device-only -c` outputs (offload bundles), host objects with a .hip_fatbin
section, or bare code objects.  Compile both trees with the Makefile's flags and ONE fixed -cuid=<string>: the default compilation-unit
id is derived from the source path and lands in the bundle.  Per function symbol of the unbundled code objects the tool takes the
llvm-objdump -d text (instruction + encoding, addresses dropped) and per kernel its whole llvm-readelf --notes metadata entry (agpr /
sgpr / vgpr counts, spills, LDS, scratch, kernarg size and layout).  It compares whole bodies, whatever they contain.
Pass (exit 0): the union of A's symbols equals the union of B's, no symbol twice on one side, 0 bodies differ, all metadata equal."""
import hashlib, os, re, shutil, subprocess, sys, tempfile

BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def tool(name):
    p = shutil.which(name) or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", name)
    if not os.path.exists(p):
        sys.exit(f"{name} not found (PATH or $ROCM_PATH/llvm/bin)")
    return p


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(path, arch, tmp):
    """path of the bare gfx code object inside `path`, or None when the object has no device code"""
    with open(path, "rb") as f:
        head = f.read(len(BUNDLE_MAGIC))
    if head[:4] == b"\x7fELF" and "amdgpu" not in run(tool("llvm-readelf"), "-h", path).lower():   # a host object: its fat binary
        fat = os.path.join(tmp, os.path.basename(path) + ".hipfb")
        subprocess.run([tool("llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", path, os.devnull], capture_output=True)
        if not os.path.exists(fat) or os.path.getsize(fat) == 0:
            return None
        path, head = fat, BUNDLE_MAGIC
    if head != BUNDLE_MAGIC:
        return path
    targets = [t for t in run(tool("clang-offload-bundler"), "--list", "--type=o", f"--input={path}").split() if t.endswith(arch)]
    if not targets:
        return None
    co = os.path.join(tmp, os.path.basename(path) + ".co")
    run(tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--input={path}", f"--targets={targets[0]}", f"--output={co}")
    return co


SYM = re.compile(r"^[0-9a-f]+ <(.+)>:$")
ADDR = re.compile(r"// [0-9A-Fa-f]+: ")


def bodies(co):
    """symbol -> sha256 of its instruction text + encodings, addresses dropped"""
    out, name, lines = {}, None, []

    def close():
        if name:
            while lines and lines[-1] == "...":      # zero fill up to the next symbol's alignment: not part of the body
                lines.pop()
            out[name] = hashlib.sha256("\n".join(lines).encode()).hexdigest()

    for line in run(tool("llvm-objdump"), "-d", co).splitlines():
        m = SYM.match(line)
        if m:
            close()
            name, lines = m.group(1), []
        elif name and line.strip():
            lines.append(ADDR.sub("// ", line.strip()))
    close()
    return out


def metadata(co):
    """kernel name -> (its whole metadata entry as text, the headline fields)"""
    entries, in_kernels = [], False
    for line in run(tool("llvm-readelf"), "--notes", co).splitlines():
        if line.startswith("amdhsa.kernels:"):
            in_kernels = True
        elif in_kernels and line and not line.startswith(" "):
            in_kernels = False
        elif in_kernels:
            if line.startswith("  - "):
                entries.append([])
            entries[-1].append(line)
    named = {}
    for entry in entries:       # the kernel's own fields sit at the entry's first indentation level, its arguments deeper
        fields = dict(m.groups() for m in (re.match(r"^  [- ] (\.[a-z_]+):\s+(\S+)$", l) for l in entry) if m)
        named[fields[".name"]] = ("\n".join(entry), fields)
    return named


HEAD = [".agpr_count", ".sgpr_count", ".vgpr_count", ".sgpr_spill_count", ".vgpr_spill_count", ".group_segment_fixed_size",
        ".private_segment_fixed_size", ".kernarg_segment_size"]


def load(directory, arch, tmp):
    syms, meta, dup = {}, {}, []
    sub = tempfile.mkdtemp(dir=tmp)
    for fn in sorted(os.listdir(directory)):
        p = os.path.join(directory, fn)
        if not os.path.isfile(p) or not fn.endswith((".o", ".co", ".hipfb")):
            continue
        co = code_object(p, arch, sub)
        if co is None:
            continue
        b, m = bodies(co), metadata(co)
        dup += [f"{s} ({fn} and {syms[s][1]})" for s in b if s in syms]
        syms.update({s: (h, fn) for s, h in b.items()})
        meta.update(m)
        print(f"  {directory}/{fn}: {len(b)} symbols, {len(m)} kernels")
    return syms, meta, dup


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    arch = sys.argv[sys.argv.index("--arch") + 1] if "--arch" in sys.argv else "gfx950"
    if len(args) != 2:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        sa, ma, da = load(args[0], arch, tmp)
        sb, mb, db = load(args[1], arch, tmp)
    only_a, only_b = sorted(set(sa) - set(sb)), sorted(set(sb) - set(sa))
    differ = sorted(s for s in set(sa) & set(sb) if sa[s][0] != sb[s][0])
    meta_differ = sorted(k for k in set(ma) & set(mb) if ma[k][0] != mb[k][0])
    print(f"symbols A {len(sa)} B {len(sb)}; only in A {len(only_a)}, only in B {len(only_b)}, twice in A {len(da)}, twice in B {len(db)}, "
          f"bodies that differ {len(differ)}")
    print(f"kernel metadata (agpr / sgpr / vgpr / spills / LDS / scratch / kernarg): kernels A {len(ma)} B {len(mb)}, "
          f"equal {not meta_differ and set(ma) == set(mb)}")
    for title, names in (("only in A", only_a), ("only in B", only_b), ("twice in A", da), ("twice in B", db), ("body differs", differ)):
        for n in names:
            print(f"  {title}: {n}")
    for k in meta_differ:
        print(f"  metadata differs: {k}: " + ", ".join(f"{f} {ma[k][1].get(f)} -> {mb[k][1].get(f)}" for f in HEAD if ma[k][1].get(f) != mb[k][1].get(f)))
    ok = not (only_a or only_b or da or db or differ or meta_differ) and set(ma) == set(mb) and len(sa) > 0
    print("PASS" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
