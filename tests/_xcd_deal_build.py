"""Test infrastructure: builds tests/cpp/xcd_deal_test (plain g++, no GPU, no ROCm include path: yams_amd/csrc/xcd_deal.h is the
header the int8 sweep's kernels inline) with AddressSanitizer and UBSan.  The program has its own main."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_xcd_deal_test():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "xcd_deal_test")
    src = os.path.join(ROOT, "tests", "cpp", "xcd_deal_test.cpp")
    hdr = os.path.join(ROOT, "yams_amd", "csrc", "xcd_deal.h")
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in (src, hdr)):
        return exe
    # -ffp-contract=off, as the kernels are built
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("xcd_deal_test failed to compile:\n" + r.stdout.decode())
    return exe
