"""Test infrastructure: builds tests/cpp/route_shell_test.cpp, the driver of include/yams_accel/topology_route.hpp
(AccelClusterRouter over a stand-in table, or over the real topology_route_v1 with --plugin).  Plain g++; the binary is
git-ignored and travels to the GPU box."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "route_shell_test.cpp")
CXX = os.environ.get("CXX", "g++")


def build_shell_test(sanitize=False):
    """sanitize=True: a stand-alone program under AddressSanitizer and UBSan (CPU only).  Returns the executable."""
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "route_shell_test_asan" if sanitize else "route_shell_test")
    deps = [SRC, os.path.join(ROOT, "include", "yams_mi355x_accel.h")] + \
        [os.path.join(ROOT, "include", "yams_accel", f) for f in ("topology_route.hpp", "plugin.hpp", "result.hpp")]
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
        return exe
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    r = subprocess.run([CXX, "-std=c++20", "-O1", "-ffp-contract=off", "-Wall", *extra, "-I" + os.path.join(ROOT, "include"), "-o", exe, SRC, "-ldl"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("route_shell_test failed to compile:\n" + r.stdout.decode())
    return exe
