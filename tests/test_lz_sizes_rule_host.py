"""The size rule of the first LZ77 stage (lzx::Size in jampack_amd/csrc/lz_expand.hpp, which k_lz77_sizes and jpk_lz77_size compile) on
the CPU under AddressSanitizer + UBSan: a stand-alone program (tests/lz_sizes_rule_host.cpp, linked with prestage.cpp) runs the host form
of the walk and jpk_lz77_size against jpk_lz77_decompress -- status and out_len -- on the crafted streams of lz_expand_cases.py and on
2000 random token streams of at most 4 KiB of output, each at out_cap = its exact size, its size - 1, 0 and a large cap.  No Python
extension; the sanitizer runtimes are linked statically and the binary is run directly in the unchanged environment."""
import os
import re
import subprocess

import lz_expand_cases as lzc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_size_rule_against_the_serial_decoder_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "lz_sizes_rule_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "lz_sizes_rule_host.cpp"),
                           os.path.join(ROOT, "jampack_amd", "csrc", "prestage.cpp"), "-o", exe])
    cases = lzc.valid_cases() + lzc.corrupt_cases()
    path = str(tmp_path / "cases.bin")
    open(path, "wb").write(lzc.pack(cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "all-ok 0" in r.stdout and "FAIL" not in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    # every valid crafted stream decodes at its size and at the large cap; the five streams that fail a check of the token walk are
    # corrupt at the large cap; every stream is over a capacity of 0 in its first token but two: "empty" has no byte to be over, and
    # "literals beyond the input" fails the check in front of the capacity check
    c = re.search(r"^crafted (\d+) ok (\d+) corrupt (\d+) capacity (\d+)$", r.stdout, re.M)
    assert c, r.stdout[-500:]
    n, ok, corrupt, capacity = (int(x) for x in c.groups())
    assert n == len(cases) and ok == len(lzc.valid_cases()) + 3 and corrupt == 5 and capacity == len(cases) - 2, r.stdout[-500:]
    # the random streams reach every outcome (a condition on the generator, not on the rule): streams that met it at one capacity at least
    m = re.search(r"^random 2000 ok (\d+) corrupt (\d+) capacity (\d+)$", r.stdout, re.M)
    assert m and all(int(x) >= 20 for x in m.groups()), r.stdout[-500:]
