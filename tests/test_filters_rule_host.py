"""The writer's filter choice (jampack_amd/csrc/prestage_rules.hpp) and its host encoder (prestage.cpp) on the CPU under AddressSanitizer +
UBSan: a stand-alone program (tests/filters_rule_host.cpp, prestage.cpp compiled into it) checks lg12 against log2 for all 65 536
arguments and the reorder index against Filters::Reorder's loop, and encodes and decodes in heap buffers of exact size at the lengths
where a piece is empty, short, full or one byte more, holding every piece's header against the argmin of the candidates' own costs.
No Python extension; the sanitizer runtimes are linked statically and the binary is run directly in the unchanged environment."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rule_and_host_encoder_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "filters_rule_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "filters_rule_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "all-ok 0" in r.stdout and "FAIL" not in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert "lg12 checked 65536" in r.stdout and "reorder checked 352" in r.stdout
    m = re.search(r"^trip checked 96 filtered (\d+) stored (\d+)$", r.stdout, re.M)
    assert m and int(m.group(1)) >= 50 and int(m.group(2)) >= 30, r.stdout[-500:]      # both outcomes of the choice ran
