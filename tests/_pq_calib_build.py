"""Test infrastructure of the PQ sum-order probe: compiles the stand-alone C++ programs under tests/cpp that go with
include/yams_accel/pq_calibration.hpp.  Plain g++, no GPU, no ROCm include path, no reference tree."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "_build")
CXX = os.environ.get("CXX", "g++")


def _fresh(exe, deps):
    return os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps)


def _run(cmd, what):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError(what + " failed to compile:\n" + r.stdout.decode())


def has_avx2():
    try:
        return "avx2" in open("/proc/cpuinfo").read()
    except OSError:
        return False


def build_pq_calibration_test():
    """tests/cpp/pq_calibration_test.cpp with AddressSanitizer and UBSan (the program has its own main), linked with the two
    hosts of tests/cpp/pq_host_avx2_{a,b}.cpp, which alone are compiled with -mavx2 (the program calls them only in its
    avx2 mode).  -O2 -ffast-math on the main program on purpose: the header's definitions must hold under the flags a host may
    build with.  Returns the executable."""
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "pq_calibration_test")
    src = os.path.join(ROOT, "tests", "cpp", "pq_calibration_test.cpp")
    hosts = [os.path.join(ROOT, "tests", "cpp", "pq_host_avx2_%s.cpp" % x) for x in "ab"]
    deps = [src, os.path.join(ROOT, "include", "yams_accel", "pq_calibration.hpp"), os.path.join(ROOT, "include", "yams_mi355x_accel.h")] + hosts
    if _fresh(exe, deps):
        return exe
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    objs = []
    for h in hosts:
        obj = os.path.join(OUT, os.path.basename(h)[:-4] + ".o")
        _run([CXX, "-std=c++17", "-O2", "-g", "-mavx2", "-Wall", "-Wextra", *san, "-c", h, "-o", obj], os.path.basename(h))
        objs.append(obj)
    _run([CXX, "-std=c++17", "-O2", "-ffast-math", "-g", "-Wall", "-Wextra", *san, "-I" + os.path.join(ROOT, "include"), "-o", exe, src, *objs],
         "pq_calibration_test")
    return exe


def build_pq_calibration_gpu_test(reference: str = "/root/reference"):
    """tests/cpp/pq_calibration_gpu_test.cpp: calibratePq / setPqSum / the default flag word of the adapters, on the device
    through the plugin (dlopen at run time).  Where the reference's headers exist it is compiled against them
    (-DYAMS_ACCEL_USE_HOST_TYPES) and drives AccelExactScanBackend; elsewhere it drives AccelVectorTable, which the backend
    forwards to.  The binary travels.  Returns (executable, "backend" | "table")."""
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "pq_calibration_gpu_test")
    src = os.path.join(ROOT, "tests", "cpp", "pq_calibration_gpu_test.cpp")
    host = os.path.isdir(os.path.join(reference, "include", "yams"))
    tag = os.path.join(OUT, "pq_calibration_gpu_test.kind")
    deps = [src, os.path.join(ROOT, "include", "yams_mi355x_accel.h")] + \
        [os.path.join(ROOT, "include", "yams_accel", f) for f in os.listdir(os.path.join(ROOT, "include", "yams_accel"))]
    if _fresh(exe, deps) and os.path.exists(tag) and (open(tag).read() == "backend" or not host):
        return exe, open(tag).read()
    cmd = [CXX, "-std=c++20", "-O1", "-g", "-Wall", "-Wno-unused-variable", "-I" + os.path.join(ROOT, "include")]
    if host:
        cmd += ["-DYAMS_ACCEL_USE_HOST_TYPES", "-I" + os.path.join(ROOT, "oracle", "shim"), "-I" + os.path.join(reference, "include")]
    _run(cmd + ["-o", exe, src, "-lpthread", "-ldl"], "pq_calibration_gpu_test")
    with open(tag, "w") as f:
        f.write("backend" if host else "table")
    return exe, "backend" if host else "table"
