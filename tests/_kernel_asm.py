"""One file of yams_amd/csrc compiled to gfx950 assembly with the product flags (yams_amd.build.FLAGS; hipcc cross-compiles
without a GPU), split the way the resource tests read it.  Compiled once per source file and process."""
import collections
import functools
import os
import re
import subprocess
import tempfile

from yams_amd import build

KernelAsm = collections.namedtuple("KernelAsm", "kernels meta text")


@functools.lru_cache(maxsize=None)
def kernel_asm(src):
    """kernels: {mangled kernel name: the lines of its body up to the end of the function, comments cut off};
    meta: {mangled kernel name: {key: int}}, the integer fields of the kernel's entry in the amdhsa.kernels metadata;
    text: the assembly as the compiler wrote it."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        cmd = [build.HIPCC, *build.FLAGS, "--cuda-device-only", "-S", os.path.join(build.CSRC, src), "-o", out]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-3000:]
        text = open(out).read()
    kernels, meta, body, entry = {}, {}, None, None
    for line in text.splitlines():
        m = re.match(r"^(_ZN10yams_accel\w+):", line)
        if m:
            body = kernels[m.group(1)] = []
        elif line.startswith(".Lfunc_end"):      # (not the first s_endpgm: an early return has one of its own)
            body = None
        elif body is not None:
            body.append(line.split(";")[0])
        if line.startswith("  - ."):             # an entry of amdhsa.kernels (its arguments' entries are indented deeper)
            entry = {}
        m = re.match(r"^(?:  - |    )\.(\w+):\s+(\S+)$", line)
        if entry is None or not m:
            continue
        if m.group(1) == "name":
            meta[m.group(2)] = entry
        elif m.group(2).isdigit():
            entry[m.group(1)] = int(m.group(2))
    return KernelAsm(kernels, meta, text)
