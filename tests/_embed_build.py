"""Test infrastructure: builds tests/cpp/embed_oracle.cpp (our C++ restatement of the embedding model's pooling head, a shared
library for ctypes) and tests/cpp/embed_shell_test.cpp, the driver of include/yams_accel/embedding_pool.hpp (AccelEmbeddingPooler
over a stand-in table, or over the real embedding_pool_v1 with --plugin).  Plain g++ with -ffp-contract=off: the MEAN step's
multiply and add stay two roundings.  The binaries are git-ignored and travel to the GPU box."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
OUT = os.path.join(CPP, "_build")
CXX = os.environ.get("CXX", "g++")


def _fresh(target, deps):
    return os.path.exists(target) and all(os.path.getmtime(target) >= os.path.getmtime(d) for d in deps)


def build_oracle():
    """Returns the path of libembed_oracle.so."""
    os.makedirs(OUT, exist_ok=True)
    lib = os.path.join(OUT, "libembed_oracle.so")
    src = os.path.join(CPP, "embed_oracle.cpp")
    if _fresh(lib, [src]):
        return lib
    r = subprocess.run([CXX, "-std=c++20", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-o", lib, src],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("embed_oracle failed to compile:\n" + r.stdout.decode())
    return lib


def build_shell_test(sanitize=False):
    """sanitize=True: a stand-alone program under AddressSanitizer and UBSan (CPU only).  Returns the executable."""
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "embed_shell_test_asan" if sanitize else "embed_shell_test")
    src = os.path.join(CPP, "embed_shell_test.cpp")
    deps = [src, os.path.join(CPP, "embed_oracle.cpp"), os.path.join(ROOT, "include", "yams_mi355x_accel.h")] + \
        [os.path.join(ROOT, "include", "yams_accel", f) for f in ("embedding_pool.hpp", "plugin.hpp", "result.hpp")]
    if _fresh(exe, deps):
        return exe
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    r = subprocess.run([CXX, "-std=c++20", "-O1", "-ffp-contract=off", "-Wall", *extra, "-I" + os.path.join(ROOT, "include"), "-o", exe, src, "-ldl"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("embed_shell_test failed to compile:\n" + r.stdout.decode())
    return exe
