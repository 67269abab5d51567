"""Hashes of the gfx950 device code of every source in csrc/Makefile's SRCS, to show that a host-side or
source-organisation change left the kernels byte for byte as they were:
  python tools/device_text.py hash <out.txt>       compile every source device-only, write "<source> <section> <sha256>"
  python tools/device_text.py hash-kernels <out.txt>   the same per kernel: "<mangled name> <size> <sha256>" for every FUNC symbol
                                                   of .text - its bytes and its <name>.kd descriptor without the 8-byte
                                                   kernel_code_entry_byte_offset - and no word about the source it came
                                                   from, so a kernel can be followed from one file to another
  python tools/device_text.py compare <a.txt> <b.txt>   exit 1 unless every pair of sections matches; for two per-kernel files:
                                                   unless the name sets are equal, no name occurs twice and every hash matches
Each source is compiled from inside csrc with relative paths (no path leaks into the code object) with the Makefile's
flags plus --offload-device-only --no-gpu-bundle-output; .text and .rodata are extracted with llvm-objcopy -O binary.
Two compiles of one source give identical sections (the ELF files themselves differ)."""
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "crank_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
SECTIONS = (".text", ".rodata")


def makefile():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    extra = {m.group(1) + ".hip": m.group(2).split() for m in re.finditer(r"^(\w+)\.o:\s*EXTRA\s*=\s*(.*)$", mk, re.M)}
    return srcs, flags, extra


def compile_device(src, flags, extra, tmp):
    elf = os.path.join(tmp, src + ".elf")
    subprocess.run([os.path.join(ROCM, "bin", "hipcc"), *flags, *extra.get(src, []), "--offload-device-only",
                    "--no-gpu-bundle-output", "-c", src, "-o", elf], check=True, cwd=CSRC)
    return elf


def hash_one(src, flags, extra, tmp):
    elf = compile_device(src, flags, extra, tmp)
    out = []
    for sec in SECTIONS:
        raw = elf + sec
        subprocess.run([os.path.join(ROCM, "llvm", "bin", "llvm-objcopy"), "-O", "binary", "--only-section=" + sec, elf, raw],
                       check=True)
        data = open(raw, "rb").read() if os.path.exists(raw) else b""
        out.append((src, sec, len(data), hashlib.sha256(data).hexdigest()))
    return out


def kernels_one(src, flags, extra, tmp):
    """(name, size, sha256) of every FUNC symbol of .text: the function's bytes, then its kernel descriptor (the OBJECT
    <name>.kd, 64 bytes) without bytes 16..23, the entry offset - the one field that says where in the file the code lies."""
    elf = compile_device(src, flags, extra, tmp)
    listing = subprocess.run([os.path.join(ROCM, "llvm", "bin", "llvm-readelf"), "-S", "-s", "-W", elf], check=True,
                             capture_output=True, text=True).stdout
    # "[ 7] .text PROGBITS <addr> <off> <size> ...": section index -> (name, address, file offset)
    secs = {int(m.group(1)): (m.group(2), int(m.group(3), 16), int(m.group(4), 16))
            for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+[0-9a-f]+", listing, re.M)}
    # "<num>: <value> <size> <type> <bind> <vis> <ndx> <name>" (.symtab and .dynsym list a global twice: same record)
    syms = {(m.group(3), m.group(5)): (int(m.group(1), 16), int(m.group(2)), m.group(4))
            for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+(\d+)\s+(\S+)$", listing, re.M)}
    raw = open(elf, "rb").read()

    def body(value, size, ndx):
        _, addr, off = secs[int(ndx)]
        return raw[off + value - addr:off + value - addr + size]

    out = []
    for (kind, name), (value, size, ndx) in sorted(syms.items()):
        if kind != "FUNC" or secs[int(ndx)][0] != ".text":
            continue
        data = body(value, size, ndx)
        kd = syms.get(("OBJECT", name + ".kd"))
        if kd:
            d = body(*kd)
            assert len(d) == 64, (name, len(d))
            data += d[:16] + d[24:]
        out.append((name, size, hashlib.sha256(data).hexdigest()))
    return out


def run_all(one, path, what):
    srcs, flags, extra = makefile()
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(int(os.environ.get("JOBS", "8"))) as ex:
        rows = [r for rs in ex.map(lambda s: one(s, flags, extra, tmp), srcs) for r in rs]
    with open(path, "w") as f:
        for r in sorted(rows) if what == "kernels" else rows:
            f.write(" ".join(str(x) for x in r) + "\n")
    print("wrote", path, len(rows), what)


def compare_kernels(a, b):
    ta, tb = ([l.split() for l in open(p) if l.strip()] for p in (a, b))
    bad = 0
    for p, t in ((a, ta), (b, tb)):
        names = [r[0] for r in t]
        for n in sorted({n for n in names if names.count(n) > 1}):
            print("TWICE in", p, n)
            bad += 1
    da, db = ({r[0]: r[1:] for r in t} for t in (ta, tb))
    for n in sorted(set(da) | set(db)):
        if da.get(n) != db.get(n):
            print("DIFFERS" if n in da and n in db else "ONLY IN " + (a if n in da else b), n, da.get(n), db.get(n))
            bad += 1
    print(f"{len([n for n in da if da[n] == db.get(n)])} of {len(da)} kernels identical, {len(db)} in {b}")
    return 1 if bad or not da else 0


def cmd_compare(a, b):
    if len(open(a).readline().split()) == 3:  # per-kernel lines have no source and no section
        return compare_kernels(a, b)
    ta, tb = ({tuple(l.split()[:2]): l.split()[2:] for l in open(p) if l.strip()} for p in (a, b))
    bad = [k for k in sorted(set(ta) | set(tb)) if ta.get(k) != tb.get(k)]
    for k in bad:
        print("DIFFERS", *k, ta.get(k), tb.get(k))
    print(f"{len(ta) - len([k for k in bad if k in ta])} of {len(ta)} sections identical")
    return 1 if bad or not ta else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "hash":
        run_all(hash_one, sys.argv[2], "sections")
    elif len(sys.argv) == 3 and sys.argv[1] == "hash-kernels":
        run_all(kernels_one, sys.argv[2], "kernels")
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(cmd_compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
