"""Indexes of damaged .jam archives and salvage, host side (no GPU): the new entries are exported and bound; jpk_jam_index_recover on
oracle-built archives -- undamaged, the hostile cases of test_jam_archive_host and further damage -- against the brute-force model of
jam_resync_model.py and the tiling invariant, under the default search limits and (in a child process with JPK_DEBUG_HOOKS=1) under
limits a few bytes wide; and the argument checks, which come before any device is looked for."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import jam_resync_model as jm
from test_jam_archive_host import _archive, _starts, hostile_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
NEW = ("jpk_dev_jam_index_recover", "jpk_jam_index_recover", "jpk_jam_index_gaps", "jpk_jam_index_gap", "jpk_dev_jam_salvage", "jpk_jam_salvage",
       "jpk_debug_jam_scan", "jpk_debug_jam_recover_limits")


@pytest.fixture(scope="module")
def jam():
    import jampack_amd
    return jampack_amd


@pytest.fixture(scope="module")
def arch(jam, oracle):
    """the archive of test_jam_archive_host: five frames of 6 000 bytes, the last one short"""
    data = jam.corpus.make("text", 4 * 6000 + 2345, 71)
    return _archive(oracle, data, MiB, 6000), data


def test_new_entries_are_exported_declared_and_bound(jam):
    from jampack_amd._lib import _SIGS
    header = open(os.path.join(ROOT, "include", "jampack_abi.h")).read()
    lib = C.CDLL(jam.LIB_PATH)
    for name in NEW:
        assert re.search(r"JPK_API\s+[\w\s\*]+\b" + name + r"\(", header), f"{name} not declared"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _SIGS, f"{name} has no ctypes signature"
    for name in ("jam_recover_index", "jam_salvage", "JAM_GAP_NOFRAME", "JAM_GAP_STAGE"):
        assert hasattr(jam, name), name
    for name in ("jam_recover_index", "jam_salvage", "jam_scan"):
        assert hasattr(jam.Context, name), name
    assert (jam.JAM_GAP_NOFRAME, jam.JAM_GAP_STAGE) == (0, 1)
    assert re.search(r"#define\s+JPK_JAM_GAP_NOFRAME\s+0\b", header) and re.search(r"#define\s+JPK_JAM_GAP_STAGE\s+1\b", header)


def _same_table(jam, a):
    ref, ix = jam.jam_index(a), jam.jam_recover_index(a)
    assert ref.bad_frame == -1
    assert (ix.frames, ix.raw_len, ix.archive_len, ix.bad_frame, ix.kind) == (ref.frames, ref.raw_len, len(a), -1, 0)
    assert [ix.frame(k) for k in range(ix.frames)] == [ref.frame(k) for k in range(ref.frames)]
    assert ix.gaps == [] and ref.gaps == []
    jm.check_tiling(ix, len(a))


def test_undamaged_and_empty_archives_give_the_plain_table(jam, arch):
    a, data = arch
    _same_table(jam, a)
    assert jam.jam_recover_index(a).frames == 5
    _same_table(jam, np.zeros(0, dtype=np.uint8))


def _expect(jam, b, frames, gaps, name):
    """the recovered index of b holds exactly these frames [(payload_off, psize)] and gaps, agrees with the model and tiles the archive"""
    ix = jam.jam_recover_index(b)
    assert jm.table(ix) == (frames, gaps), name
    assert jm.model(jam, b) == (frames, gaps), name
    jm.check_tiling(ix, len(b))
    return ix


def test_hostile_cases_are_indexed_past_the_damage(jam, arch):
    a, data = arch
    s = _starts(a)
    fr = [(o + 15, (s + [len(a)])[k + 1] - o - 15) for k, o in enumerate(s)]
    seen = set()
    for name, b, k in hostile_cases(a):
        seen.add(name)
        if name in ("magic", "blocksize_low", "blocksize_high", "negative_payload", "payload_above_max"):
            ix = _expect(jam, b, [fr[0], fr[1], fr[3], fr[4]], [(s[2], s[3] - s[2], 2, 0)], name)
            assert [ix.frame(f)[:2] for f in range(4)] == [(0, 6000), (6000, 6000), (12000, 6000), (18000, 2345)], name
        elif name == "payload_past_end":
            _expect(jam, b, fr[:4], [(s[4], len(b) - s[4], 4, 0)], name)
        elif name.startswith("trailing_"):
            _expect(jam, b, fr, [(len(a), int(name.split("_")[1]), 5, 0)], name)
        else:
            assert name == "truncated_header"
            _expect(jam, b, fr[:2], [(s[2], 9, 2, 0)], name)
    assert len(seen) == 10


def test_further_damage_against_the_model(jam, arch):
    a, data = arch
    s = _starts(a)
    for name, b in jm.damage_cases(a):
        ix = jam.jam_recover_index(b)
        assert jm.table(ix) == jm.model(jam, b), name
        jm.check_tiling(ix, len(b))
        if name == "two_lost":
            assert ix.gaps == [(s[1], s[3] - s[1], 1, 0)] and ix.frames == 3
        if name == "first_lost":
            assert ix.gaps == [(0, s[1], 0, 0)] and ix.frames == 4
        if name == "fourteen_bytes":
            assert (ix.frames, ix.gaps) == (0, [(0, 14, 0, 0)])
        if name == "inserted_37":
            assert ix.frames == 5 and ix.gaps == [(s[2], 37, 2, 0)]
        if name in ("decoy_in_lost_payload", "first_payload_byte", "psize_minus_1"):
            assert ix.frames == 4 and ix.gaps == [(s[2], s[3] - s[2], 2, 0)], name
        if name == "decoy_flood":
            assert ix.frames == 5 and ix.gaps == [(s[2], 600, 2, 0)]


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import jampack_amd as jam
import jam_resync_model as jm
z = np.load(sys.argv[2])
out = {}
assert jam.lib().jpk_debug_jam_recover_limits(-1, 0) == -1 and jam.lib().jpk_debug_jam_recover_limits(0, -1) == -1
for w, k in ((4096, 4), (64, 4), (15, 1), (0, 0)):
    assert jam.lib().jpk_debug_jam_recover_limits(w, k) == 0
    for name in z.files:
        ix = jam.jam_recover_index(z[name])
        jm.check_tiling(ix, len(z[name]))
        out[f"{name}/{w}/{k}"] = [[list(f) for f in jm.table(ix)[0]], [list(g) for g in ix.gaps]]
print("RESULT " + json.dumps(out))
"""


def test_the_index_does_not_depend_on_window_or_candidate_cap(jam, arch, tmp_path):
    """the same archives under limits (4096, 4) -- the decoy flood then takes ten rounds of four candidates --, (64, 4) and (15, 1), set
    through jpk_debug_jam_recover_limits in a child process: every index equals the one of the default limits"""
    a, data = arch
    cases = dict(jm.damage_cases(a))
    cases.update({name: b for name, b, _ in hostile_cases(a)})
    cases["undamaged"] = a
    path = str(tmp_path / "cases.npz")
    np.savez(path, **cases)
    env = dict(os.environ, JPK_DEBUG_HOOKS="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    got = json.loads(r.stdout.split("RESULT ", 1)[1])
    assert len(got) == 4 * len(cases)
    for name, b in cases.items():
        ix = jam.jam_recover_index(b)
        want = [[list(f) for f in jm.table(ix)[0]], [list(g) for g in ix.gaps]]
        for w, k in ((4096, 4), (64, 4), (15, 1), (0, 0)):
            assert got[f"{name}/{w}/{k}"] == want, (name, w, k)
    # without JPK_DEBUG_HOOKS the hook refuses
    if "JPK_DEBUG_HOOKS" not in os.environ:
        assert jam.lib().jpk_debug_jam_recover_limits(64, 4) == -1


def test_a_deep_flip_leaves_the_frame_in_the_index(jam, arch):
    a, data = arch
    b = jm.deep_flip(a)
    assert b.tobytes() != a.tobytes()
    ix, ref = jam.jam_recover_index(b), jam.jam_index(a)
    assert ix.gaps == [] and [ix.frame(k) for k in range(5)] == [ref.frame(k) for k in range(5)]


def _recover(lib, a, in_len, kind, verify, h=True, g=True):
    hp, gp = C.c_void_p(), C.c_int32(-7)
    rc = lib.jpk_jam_index_recover(a.ctypes.data if a is not None else None, in_len, kind, verify, C.byref(hp) if h else None, C.byref(gp) if g else None)
    if hp:
        lib.jpk_jam_index_destroy(hp)
    return rc, gp.value


def test_argument_checks(jam, arch):
    a, data = arch
    lib = jam.lib()
    assert _recover(lib, a, len(a), 0, 0) == (0, 0)
    assert _recover(lib, a, len(a), 0, 0, g=False)[0] == 0             # gaps may be NULL
    assert _recover(lib, a, len(a), 1, 0)[0] == -1                     # stock-CLI archives are not recovered
    assert _recover(lib, a, len(a), 3, 0)[0] == -1 and _recover(lib, a, len(a), -1, 0)[0] == -1
    assert _recover(lib, a, len(a), 0, 1)[0] == -1                     # a plain index verifies nothing
    assert _recover(lib, a, len(a), 2, 2)[0] == -1
    assert _recover(lib, a, len(a), 0, 0, h=False)[0] == -1
    assert _recover(lib, None, len(a), 0, 0)[0] == -1 and _recover(lib, a, -1, 0, 0)[0] == -1
    assert _recover(lib, None, 0, 0, 0) == (0, 0)
    assert lib.jpk_dev_jam_index_recover(None, a.ctypes.data, len(a), 0, 0, C.byref(C.c_void_p()), None) == -1
    assert lib.jpk_jam_index_gaps(None) == -1 and lib.jpk_jam_index_gap(None, 0, None, None, None, None) == -1
    ref = jam.jam_index(a)
    assert lib.jpk_jam_index_gaps(ref._h) == 0 and ref.gaps == []
    ix = jam.jam_recover_index(hostile_cases(a)[0][1])
    assert lib.jpk_jam_index_gaps(ix._h) == 1
    for g in (-1, 1, 2, 1 << 30):
        assert lib.jpk_jam_index_gap(ix._h, g, None, None, None, None) == -1, g
    assert lib.jpk_jam_index_gap(ix._h, 0, None, None, None, None) == 0


def test_kind_2_of_a_plain_archive_makes_no_device_call(jam, arch):
    """an archive without a staged frame is indexed by the walk alone (where no GPU is visible a device call would be JPK_E_DEVICE_NONE)"""
    a, data = arch
    for name, b in [("undamaged", a)] + [(n, x) for n, x, _ in hostile_cases(a)] + jm.damage_cases(a):
        for verify in (False, True):
            i2, i0 = jam.jam_recover_index(b, jam.JAM_INDEX_STAGED, verify), jam.jam_recover_index(b)
            assert i2.kind == 2 and i0.kind == 0
            assert jm.table(i2) == jm.table(i0), name
            assert [i2.frame(k) for k in range(i2.frames)] == [i0.frame(k) for k in range(i0.frames)], name
            assert all(i2.frame_kind(k) == 0 for k in range(i2.frames))


def test_salvage_refuses_its_arguments_before_it_looks_for_a_device(jam, arch):
    a, data = arch
    lib = jam.lib()
    ix = jam.jam_recover_index(a)
    out = np.full(len(data) + 64, 0xA5, dtype=np.uint8)
    n, failed = C.c_int64(-7), C.c_int32(-7)
    st = (C.c_int32 * 5)()
    call = lambda h, p, ln, o, cap, np_: lib.jpk_jam_salvage(h, p, ln, o, cap, np_, st, C.byref(failed))
    assert call(None, a.ctypes.data, len(a), out.ctypes.data, len(out), C.byref(n)) == -1
    assert call(ix._h, a.ctypes.data, len(a) - 1, out.ctypes.data, len(out), C.byref(n)) == -1     # not the indexed archive
    assert call(ix._h, None, len(a), out.ctypes.data, len(out), C.byref(n)) == -1
    assert call(ix._h, a.ctypes.data, len(a), None, len(out), C.byref(n)) == -1
    assert call(ix._h, a.ctypes.data, len(a), out.ctypes.data, -1, C.byref(n)) == -1
    assert call(ix._h, a.ctypes.data, len(a), out.ctypes.data, len(out), None) == -1
    assert n.value == -7
    assert call(ix._h, a.ctypes.data, len(a), out.ctypes.data, len(data) - 1, C.byref(n)) == -2    # the capacity answer
    assert n.value == len(data) and (out == 0xA5).all()
    assert lib.jpk_dev_jam_salvage(None, ix._h, a.ctypes.data, len(a), out.ctypes.data, len(out), C.byref(n), st, C.byref(failed)) == -1
    # an index without raw bytes is salvaged without a device
    e = jam.jam_recover_index(a[:14])
    assert lib.jpk_jam_salvage(e._h, a.ctypes.data, 14, None, 0, C.byref(n), None, C.byref(failed)) == 0 and (n.value, failed.value) == (0, 0)
    got, status = jam.jam_salvage(a[:14])
    assert len(got) == 0 and status == []
