#!/usr/bin/env python3
"""Do two builds of libvilfusion_hip.so hold the same device code? Disassembles the gfx950 code objects of both and compares the instruction sequence of every
function symbol (addresses and encodings stripped). The check behind a refactor that must not move a kernel. Needs no GPU.

  python tools/dev_same_device_code.py OTHER.so [THIS.so]      # exit status 1 and the differing symbols if they differ
"""
import re
import subprocess
import sys
import tempfile

from kernel_resources import SO, code_objects

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def functions(path):
    """symbol -> its instructions, over every code object of the library"""
    out = {}
    for blob in code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob); f.flush()
            txt = subprocess.run([OBJDUMP, "-d", f.name], capture_output=True, text=True, check=True).stdout
        name = None
        for line in txt.splitlines():
            m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
            if m:
                name = m.group(1)
                assert name not in out, name
                out[name] = []
            elif name and line.strip():
                out[name].append(line.split("//")[0].strip())
    return out


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2] if len(sys.argv) > 2 else SO)
    bad = sorted(set(a) ^ set(b)) + sorted(n for n in set(a) & set(b) if a[n] != b[n])
    print(f"{len(a)} / {len(b)} symbols, {sum(map(len, a.values()))} / {sum(map(len, b.values()))} instructions, {len(bad)} differ" + "".join("\n  " + n for n in bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
