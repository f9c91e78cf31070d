#!/usr/bin/env python3
"""Per-kernel disassembly comparison of two builds of the library: which kernels compile to different instructions.

    python tools/kernel_disasm_diff.py OLD.so NEW.so

Each library's gfx950 code object is unbundled and disassembled (llvm-objdump); a kernel's instructions are compared after hexadecimal
immediates and symbolic targets are masked, so that PC-relative offsets to the constant tables (which move whenever the code object grows) do
not count.  Prints one line per kernel: "same" or "differs" with the instruction counts."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def kernels(lib):
    with tempfile.TemporaryDirectory() as t:
        fat, co = os.path.join(t, "fatbin"), os.path.join(t, "co")
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}",
                               f"--output={co}", "--unbundle"])
        text = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(?:\S+ )?<(\S+)>:", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        line = re.sub(r"//.*", "", line).strip()
        if cur and line:
            out[cur].append(re.sub(r"<[^>]*>", "", re.sub(r"0x[0-9a-fA-F]+", "X", line)))
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    for k in sorted(set(old) | set(new)):
        a, b = old.get(k), new.get(k)
        if a is None or b is None:
            print(f"{k:48s} {'new' if a is None else 'removed'}")
        else:
            print(f"{k:48s} {'same' if a == b else 'differs'} ({len(a)} -> {len(b)} instructions)")


if __name__ == "__main__":
    main()
