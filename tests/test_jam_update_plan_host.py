"""The plan of an archive update (jampack_amd/csrc/jam_update_plan.hpp, which jam_archive.hip compiles for jpk_dev_jam_update and
jpk_jam_update) on the CPU under AddressSanitizer + UBSan: a stand-alone program (tests/jam_update_plan_host.cpp, header only) compares
the argument verdict, the class of every frame, the pieces and the passes with a brute-force byte map -- one owner per raw byte, one class
per frame -- on crafted cases and on 2000 random indexes with random writes.  No Python extension; the sanitizer runtimes are linked
statically and the binary is run directly in the unchanged environment."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_update_plan_against_a_byte_map_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "jam_update_plan_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "jam_update_plan_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "all-ok 0" in r.stdout and "FAIL" not in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    c = re.search(r"^crafted (\d+) refused (\d+)$", r.stdout, re.M)
    assert c and int(c.group(1)) == 34 and int(c.group(2)) == 9, r.stdout[-500:]
    # the random cases reach every outcome (conditions on the generator, not on the plan): all three frame classes in one case, a frame
    # made wholly covered by more than one write, refused writes
    m = re.search(r"^random 2000 all3 (\d+) multi (\d+) refused (\d+)$", r.stdout, re.M)
    assert m and int(m.group(1)) >= 200 and int(m.group(2)) >= 50 and int(m.group(3)) >= 100, r.stdout[-500:]
