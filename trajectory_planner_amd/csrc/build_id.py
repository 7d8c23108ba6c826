"""build_id.py SOLVER_OBJ... -- OTHER_OBJ...: prints vigo_build_id()'s "solver:<12 hex> all:<12 hex>", digests of the compiled
code (`solver` over the objects before `--`, `all` over all of them): each object's host .text* / .rodata* sections and its
gfx950 code object's .text, .rodata, .data and .note — never symbol or string tables, which carry the per-build __hip_cuid_."""
import hashlib, struct, sys

def sections(elf):   # (name, bytes) of each section of a 64-bit little-endian ELF
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    size, num, names = struct.unpack_from("<HHH", elf, 0x3A)
    sh = [struct.unpack_from("<IIQQQQ", elf, shoff + i * size) for i in range(num)]
    base = sh[names][4]
    return [(elf[base + n:elf.index(b"\0", base + n)], b"" if t == 8 else elf[o:o + sz]) for n, t, _, _, o, sz in sh]

def code_object(bundle, target=b"hipv4-amdgcn-amd-amdhsa--gfx950"):   # from an (uncompressed) clang offload bundle
    assert bundle.startswith(b"__CLANG_OFFLOAD_BUNDLE__"), "unsupported offload bundle format"
    pos = 32
    for _ in range(struct.unpack_from("<Q", bundle, 24)[0]):
        off, size, n = struct.unpack_from("<QQQ", bundle, pos)
        if bundle[pos + 24:pos + 24 + n] == target: return bundle[off:off + size]
        pos += 24 + n
    raise SystemExit("no gfx950 code object in the offload bundle")

def code(path):
    host = sections(open(path, "rb").read())
    dev = [s for n, b in host if n == b".hip_fatbin" for s in sections(code_object(b))]
    return b"".join(n + struct.pack("<Q", len(b)) + b for n, b in host if n.startswith((b".text", b".rodata"))) + b"".join(
        n + struct.pack("<Q", len(b)) + b for n, b in dev if n in (b".text", b".rodata", b".data", b".note"))

cut = sys.argv.index("--")
digest = lambda objs: hashlib.sha1(b"".join(code(o) for o in objs)).hexdigest()[:12]
print(f"solver:{digest(sys.argv[1:cut])} all:{digest(sys.argv[1:cut] + sys.argv[cut + 1:])}")
