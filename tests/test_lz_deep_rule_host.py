"""The deep rule of the parallel LZ77 expander (jampack_amd/csrc/lz_expand.hpp: lzx::deep_step, lzx::deep_seg_cap and the chase with
lzx::DEEP_CHASE hops, what k_lzd_plan / k_lzd_copy compile) on the CPU under AddressSanitizer + UBSan: a stand-alone program
(tests/lz_deep_rule_host.cpp, linked with prestage.cpp for jpk_lz77_decompress) runs plan and chase against the serial decoder's bytes,
lengths and statuses on the crafted streams of lz_deep_cases.py, on the valid and the hostile streams of lz_expand_cases.py and on 2000
random token streams, and holds every path against a model of its own.  No Python extension; the sanitizer runtimes are linked
statically and the binary is run directly in the unchanged environment."""
import os
import re
import subprocess

import lz_deep_cases as lzd
import lz_expand_cases as lzc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_model_gives_the_crafted_streams_the_paths_they_were_made_for():
    cases = lzd.valid_cases()
    want = lzd.expected_paths()
    assert {name: path for name, _, _, path in cases} == want
    # the depths are what the names say, and the two budget streams differ by one record at one prefix
    hops, per, slack = lzd.LIMITS
    for d in (9, 15, hops, hops + 1):
        assert lzc.shape(lzd.deep_chase(d))[1] == d and lzc.shape(lzd.generations(d))[1] == d
    assert lzc.shape(lzd.overlaps(3, hops))[1] == hops and lzc.shape(lzd.overlaps(17, hops))[1] == hops
    at, over = lzd.prefixes(lzd.budget(False)), lzd.prefixes(lzd.budget(True))
    assert at[1] == (4, 10) and 4 == 10 // per + slack and over[2] == (5, 14) and all(n <= op // per + slack for n, op in at)
    # the short input has more records than the old rule's cap and fewer than the new one's
    s = lzd.short_input()
    nrec = lzd.prefixes(s)[-1][0]
    assert nrec == 391 and nrec > lzc.seg_cap(len(s)) and lzc.path_of(s) == "serial"


def test_deep_plan_and_chase_against_the_serial_decoder_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "lz_deep_rule_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "lz_deep_rule_host.cpp"),
                           os.path.join(ROOT, "jampack_amd", "csrc", "prestage.cpp"), "-o", exe])
    old = [(name, s, cap, lzd.deep_path_of(s)) for name, s, cap, _ in lzc.valid_cases()]
    cases = lzd.valid_cases() + old + lzc.corrupt_cases()
    path = str(tmp_path / "cases.bin")
    open(path, "wb").write(lzc.pack(cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "all-ok 0" in r.stdout and "FAIL" not in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    assert "limits %d %d %d\n" % lzd.LIMITS in r.stdout, r.stdout[-500:]
    c = re.search(r"^crafted (\d+) parallel (\d+) refused (\d+) over (\d+) deep (\d+)$", r.stdout, re.M)
    assert c, r.stdout[-500:]
    total, par, refused, over, deep = (int(x) for x in c.groups())
    assert (total, par, refused) == (len(cases), sum(p == "parallel" for *_, p in cases), len(lzc.corrupt_cases())), r.stdout[-500:]
    assert over >= 2 and deep >= 3 and over + deep == sum(p == "serial" for *_, p in cases) - refused, r.stdout[-500:]
    # the random streams reach every way a block can go, and at most a quarter of them go the serial way
    m = re.search(r"^random 2000 parallel (\d+) refused (\d+) over (\d+) deep (\d+)$", r.stdout, re.M)
    assert m and all(int(x) >= 20 for x in m.groups()), r.stdout[-500:]
    assert int(m.group(1)) >= 1500, r.stdout[-500:]
