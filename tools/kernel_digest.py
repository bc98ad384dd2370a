#!/usr/bin/env python3
"""kernel_digest.py OBJECT...: one sorted line per gfx950 kernel of the given host objects --
name, code size, VGPRs, SGPRs, LDS, scratch, VGPR / SGPR spills (from the code object's notes) and the sha256 of the
kernel's code bytes.  Two builds launch the same kernels exactly when `sort -u` of their digests agree; a name listed
twice is a kernel compiled into two objects.  Whole code objects cannot be compared: their file hashes differ between
two compilations of one source, while a kernel's bytes do not (the kernels reference nothing outside themselves)."""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
NOTE_KEYS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count",
             "sgpr_spill_count")


def tool(name, *args, cwd=None):
    return subprocess.run([os.path.join(LLVM, name), *args], cwd=cwd, check=True, capture_output=True, text=True).stdout


def digest(obj):
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(obj, os.path.join(tmp, "o"))
        tool("llvm-objdump", "--offloading", "o", cwd=tmp)  # writes o.<k>.<target> next to its input
        for co in sorted(f for f in os.listdir(tmp) if f.endswith("gfx950")):
            path = os.path.join(tmp, co)
            text = re.search(r"\] \.text\s+PROGBITS\s+([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+)", tool("llvm-readelf", "-S", path))
            addr, off, size = (int(x, 16) for x in text.groups())
            with open(path, "rb") as fh:
                code = fh.read()[off:off + size]
            funcs = {}
            for m in re.finditer(r"^\s*\d+: ([0-9a-f]+)\s+(\d+) FUNC\s.* (\S+)$", tool("llvm-readelf", "-s", path), re.M):
                funcs[m.group(3)] = (int(m.group(1), 16) - addr, int(m.group(2)))
            kernels, cur = [], None
            for line in tool("llvm-readelf", "--notes", path).splitlines():
                m = re.match(r"^(  - |    )\.(\w+):\s+(\S+)$", line)
                if m and m.group(1) == "  - ":
                    cur = {}
                    kernels.append(cur)
                if m and cur is not None:
                    cur[m.group(2)] = m.group(3)
            for k in kernels:
                at, n = funcs[k["name"]]
                yield " ".join([k["name"], str(n), *(k[key] for key in NOTE_KEYS), hashlib.sha256(code[at:at + n]).hexdigest()])


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    print("\n".join(sorted(line for obj in sys.argv[1:] for line in digest(obj))))
