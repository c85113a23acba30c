"""The resync rule of damaged stock-CLI .jam archives (jrs::walk over jrs::HostSrc{..., cli = true} in jampack_amd/csrc/jam_resync.hpp,
which jam_archive.hip compiles for both recover entries) on the CPU under AddressSanitizer + UBSan: a stand-alone program
(tests/jam_resync_cli_rule_host.cpp, header only) compares it, under windows of 1 byte to 4 KiB and caps of 1 to 4 candidates, with a
brute-force walk of its own -- a frame may declare (int64_t)(BlockSize * 1.05) + 4096 bytes behind the trailer, a staged header is never
plausible -- on crafted damage and on 800 random archives.  No Python extension; the sanitizer runtimes are linked statically and the
binary is run directly in the unchanged environment."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_resync_rule_against_a_brute_force_walk_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "jam_resync_cli_rule_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "jam_resync_cli_rule_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "all-ok 0" in r.stdout and "FAIL" not in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    c = re.search(r"^crafted (\d+) frames (\d+) gaps (\d+) clean (\d+)$", r.stdout, re.M)
    assert c, r.stdout[-500:]
    n, frames, gaps, clean = (int(x) for x in c.groups())
    # no gap: undamaged, empty, the truncation at a frame edge, a declared trailer, and a declared BlockSize (both walks), BlockSize + 1, cap
    # and 2 MiB + 1 at BlockSize 2 MiB (the stock-CLI walk only); every other case has one gap at least
    assert n == 66 and clean == 9 and gaps >= n - clean and frames >= 3 * n, r.stdout[-500:]
    # the random archives reach every outcome (a condition on the generator, not on the rule)
    m = re.search(r"^random (\d+) frames (\d+) gaps (\d+) clean (\d+)$", r.stdout, re.M)
    assert m and int(m.group(1)) >= 500 and int(m.group(2)) >= 500 and int(m.group(3)) >= 500 and int(m.group(4)) >= 20, r.stdout[-500:]
