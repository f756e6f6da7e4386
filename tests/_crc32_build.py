"""Test infrastructure of the CRC-32 tests: compiles the stand-alone C++ programs under tests/cpp that go with
yams_amd/csrc/crc32_host.h and include/yams_accel/checksum.hpp.  Plain g++, no GPU, no ROCm include path."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fresh(exe, deps):
    return os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps)


def build_crc32_host_test():
    """tests/cpp/crc32_host_test.cpp with AddressSanitizer and UBSan: the program has its own main and walks the segment plan
    over heap blocks of exactly the granules a message touches.  Returns the executable."""
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "crc32_host_test")
    src = os.path.join(ROOT, "tests", "cpp", "crc32_host_test.cpp")
    if _fresh(exe, [src, os.path.join(ROOT, "yams_amd", "csrc", "crc32_host.h")]):
        return exe
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("crc32_host_test failed to compile:\n" + r.stdout.decode())
    return exe


def build_checksum_shell_test():
    """tests/cpp/checksum_shell_test.cpp: the driver of include/yams_accel/checksum.hpp (AccelCrc32 over the plugin's
    content_checksum_v1, dlopen at run time).  Built where a compiler is; the binary travels.  Returns the executable."""
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "checksum_shell_test")
    src = os.path.join(ROOT, "tests", "cpp", "checksum_shell_test.cpp")
    deps = [src, os.path.join(ROOT, "include", "yams_mi355x_accel.h"), os.path.join(ROOT, "include", "yams_accel", "checksum.hpp")]
    if _fresh(exe, deps):
        return exe
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-g", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                        "-ldl"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("checksum_shell_test failed to compile:\n" + r.stdout.decode())
    return exe
