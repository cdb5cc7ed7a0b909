"""Size and SHA-1 of the machine code of every kernel in the built library: the companion of tools/kernel_resources.sh for
"symbol by symbol the same bytes".  Two libraries hold the same code for a kernel when its line is the same in both outputs.

    python tools/kernel_code_hashes.py [clive2_amd/libclive2_amd.so] | sort > new.txt      # diff against the parent's
"""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def device_elf(lib):
    """the embedded gfx950 code object: the first ELF inside the file whose e_machine is 224 (AMDGPU)"""
    b = open(lib, "rb").read()
    i = b.find(b"\x7fELF", 1)
    while i != -1:
        if struct.unpack_from("<H", b, i + 18)[0] == 224:
            return b[i:]
        i = b.find(b"\x7fELF", i + 1)
    raise SystemExit(f"{lib}: no AMDGPU code object inside")


def main(argv):
    lib = argv[1] if len(argv) > 1 else os.path.join("clive2_amd", "libclive2_amd.so")
    co = device_elf(lib)
    with tempfile.TemporaryDirectory() as t:
        path = os.path.join(t, "k.co")
        with open(path, "wb") as f:
            f.write(co)
        sections = subprocess.run([READELF, "-S", "-W", path], capture_output=True, text=True, check=True).stdout
        symbols = subprocess.run([READELF, "-s", "-W", path], capture_output=True, text=True, check=True).stdout
    m = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", sections)
    addr, off = int(m.group(1), 16), int(m.group(2), 16)
    seen = set()
    for line in symbols.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC" and f[6] != "UND" and f[7] not in seen:      # .symtab repeats .dynsym
            seen.add(f[7])
            value, size = int(f[1], 16), int(f[2])
            code = co[off + value - addr: off + value - addr + size]
            print(f[7], size, hashlib.sha1(code).hexdigest())
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv))
