"""The shared rules of the pre-stages (jampack_amd/csrc/prestage_rules.hpp) on the CPU under AddressSanitizer + UBSan: a stand-alone
program (tests/prestage_rules_host.cpp) runs the LPX kernel's serial walk -- tiles, ring, ring_back, step -- exactly as lane 0 does and
compares it with the direct-indexed host form, checks the part cut against the reference's loop and the LEB128 code at its class edges.
Both forms call the same step and update, so that comparison checks the tile and ring indexing, not the model; the model is checked on
tests/golden/golden_lpx_predicted.npz, the reference's own Lpx::Encode output for an input on which it predicts (oracle.pyoracle.Ref().lpx_encode
of jampack_amd.corpus.make("runs", 70003, 83): five parts, each longer than a tile), which both forms must decode and reproduce.
No Python extension; the sanitizer runtimes are linked statically and the binary is run directly in the unchanged environment."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^lpx (\w+) (\d+) enc_stretch (\d+) enc_tile_cross (\d+) enc_ring_cross (\d+) dec_stretch (\d+) dec_tile_cross (\d+) dec_ring_cross (\d+)$")
LENS = list(range(10)) + [65_536, 65_540, 327_680, 327_684, 360_001]
KINDS = ["zeros", "rep4k", "text", "random"]


def test_kernel_walk_part_cut_and_leb_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "prestage_rules_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "prestage_rules_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden_lpx_predicted.npz"))
    stream, plain = str(tmp_path / "runs.stream"), str(tmp_path / "runs.plain")
    z["runs_70003_stream"].tofile(stream)
    z["runs_70003_plain"].tofile(plain)
    r = subprocess.run([exe, stream, plain], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "all-ok 0" in r.stdout and "FAIL" not in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert "parts checked 4101" in r.stdout and "leb checked 10" in r.stdout
    g = re.search(r"^golden 70003 bytes changed (\d+) stretch (\d+)$", r.stdout, re.M)
    assert g and int(g.group(1)) > 10_000 and 2 * int(g.group(2)) > 70_003, g          # the reference predicted, and changed bytes
    rows = {(m.group(1), int(m.group(2))): [int(x) for x in m.groups()[2:]] for m in map(LINE.match, r.stdout.splitlines()) if m}
    assert sorted(rows) == sorted((k, n) for k in KINDS for n in LENS)
    # The comparison must not be one of pass-through copies.  On zeros the model predicts nearly every byte.  The 4 KiB repeat of RANDOM
    # bytes stays in as an equality input, but the model never predicts on it (every table slot sees ~16 contexts in turn and misses:
    # 0 bytes in stretches, in this program and in the host encoder before the rules moved), so it cannot carry this assertion.
    for n in LENS:
        if n >= 65_536:
            es, _, _, ds, _, _ = rows[("zeros", n)]
            assert 2 * es > n and 2 * ds > n, (n, es, ds)
    for tile_cross, ring_cross in ((1, 2), (4, 5)):                     # columns of the encoder, of the decoder
        assert sum(rows[("zeros", n)][tile_cross] for n in LENS) >= 1
        assert sum(rows[("zeros", n)][ring_cross] for n in LENS) >= 1
