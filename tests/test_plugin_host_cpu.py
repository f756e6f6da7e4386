"""The plugin door's host logic (yams_amd/csrc/plugin_host.h: what plugin.cpp computes on the host around its device calls)
on the CPU: compiled with plain g++ under AddressSanitizer and UBSan into tests/cpp/plugin_host_test and run there — the
stripe dealing against the kernels' own global_row_id, the dealt allow-mask, the shard-local tie ranks, the PQ key ranking,
the permutation check, the hit packing, hex, the strict configuration reader, the owned result arrays (OwnedArrays, HitResult)
and the registry of a handle family (HandleTable) — the last also under ThreadSanitizer, from eight threads."""
import subprocess

import _cpp_build


def test_the_door_s_host_logic_under_asan_and_ubsan():
    exe = _cpp_build.build_plugin_host_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_the_handle_table_from_eight_threads_under_tsan():
    exe = _cpp_build.build_plugin_host_test_tsan()
    r = subprocess.run([exe, "--threads"], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "threads OK (0 failures" in r.stdout and "ThreadSanitizer" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
