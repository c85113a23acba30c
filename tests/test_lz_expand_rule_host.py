"""The rule of the parallel LZ77 expander (jampack_amd/csrc/lz_expand.hpp) on the CPU under AddressSanitizer + UBSan: a stand-alone
program (tests/lz_expand_rule_host.cpp, linked with prestage.cpp for jpk_lz77_decompress) runs the host form of plan and chase -- the
functions the kernels compile -- against the serial decoder's bytes, lengths and statuses on the crafted streams of lz_expand_cases.py
and on 2000 random token streams of at most 4 KiB of output.  No Python extension; the sanitizer runtimes are linked statically and the
binary is run directly in the unchanged environment."""
import os
import re
import subprocess

import lz_expand_cases as lzc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_and_chase_against_the_serial_decoder_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "lz_expand_rule_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "lz_expand_rule_host.cpp"),
                           os.path.join(ROOT, "jampack_amd", "csrc", "prestage.cpp"), "-o", exe])
    cases = lzc.valid_cases() + lzc.corrupt_cases()
    path = str(tmp_path / "cases.bin")
    open(path, "wb").write(lzc.pack(cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "all-ok 0" in r.stdout and "FAIL" not in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    c = re.search(r"^crafted (\d+) parallel (\d+) refused (\d+) over_cap (\d+) deep (\d+)$", r.stdout, re.M)
    want = [len(cases), sum(p == "parallel" for *_, p in cases), len(lzc.corrupt_cases()), 1, 1]
    assert c and [int(x) for x in c.groups()] == want, (r.stdout[-500:], want)
    # the random streams reach every way a block can go
    m = re.search(r"^random 2000 parallel (\d+) refused (\d+) over_cap (\d+) deep (\d+)$", r.stdout, re.M)
    assert m and all(int(x) >= 20 for x in m.groups()), r.stdout[-500:]
