"""Hashes of the gfx950 device code of every source in csrc/Makefile's SRCS, to show that a host-side or
source-organisation change left the kernels byte for byte as they were:
  python tools/device_text.py hash <out.txt>       compile every source device-only, write "<source> <section> <sha256>"
  python tools/device_text.py compare <a.txt> <b.txt>   exit 1 unless every pair of sections matches
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


def hash_one(src, flags, extra, tmp):
    elf = os.path.join(tmp, src + ".elf")
    subprocess.run([os.path.join(ROCM, "bin", "hipcc"), *flags, *extra.get(src, []), "--offload-device-only",
                    "--no-gpu-bundle-output", "-c", src, "-o", elf], check=True, cwd=CSRC)
    out = []
    for sec in SECTIONS:
        raw = elf + sec
        subprocess.run([os.path.join(ROCM, "llvm", "bin", "llvm-objcopy"), "-O", "binary", "--only-section=" + sec, elf, raw],
                       check=True)
        data = open(raw, "rb").read() if os.path.exists(raw) else b""
        out.append((src, sec, len(data), hashlib.sha256(data).hexdigest()))
    return out


def cmd_hash(path):
    srcs, flags, extra = makefile()
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(int(os.environ.get("JOBS", "8"))) as ex:
        rows = [r for rs in ex.map(lambda s: hash_one(s, flags, extra, tmp), srcs) for r in rs]
    with open(path, "w") as f:
        for src, sec, n, h in rows:
            f.write(f"{src} {sec} {n} {h}\n")
    print("wrote", path, len(rows), "sections")


def cmd_compare(a, b):
    ta, tb = ({tuple(l.split()[:2]): l.split()[2:] for l in open(p) if l.strip()} for p in (a, b))
    bad = [k for k in sorted(set(ta) | set(tb)) if ta.get(k) != tb.get(k)]
    for k in bad:
        print("DIFFERS", *k, ta.get(k), tb.get(k))
    print(f"{len(ta) - len([k for k in bad if k in ta])} of {len(ta)} sections identical")
    return 1 if bad or not ta else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "hash":
        cmd_hash(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(cmd_compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
