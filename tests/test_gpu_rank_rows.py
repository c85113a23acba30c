"""k_dec_rank (ans_dec_rank.hip) on the crafted texts of rank_rows_model: row top-ups, bucket ends, ranks at and above 64.  -m gpu

test_rank_rows_model.py shows, from the inputs alone, which arms of the kernel's row scheme every text reaches (fast iterations with and
without zeros, the exit for a rank >= 64, inserts and front drops below and above 64, runs past the known entries, top-ups full, cut and
into an empty row, landings on the current and on another symbol, the tail) and which single-token changes of the scheme each text would
expose.  Here the kernel decodes them, bit-exact against the oracle (which test_oracle_vs_ref.py pins to the reference build), on guarded
buffers:
  * the probe entry, in place, the rank array 0, 1, 3 and 15 bytes behind an aligned address, the frequency table 4 bytes off a 16-byte
    boundary; and the encoder on the same texts;
  * the product path (headers -> rANS -> RLE0 -> k_dec_rank with the chunk's own offsets) at exact capacity, and three two-chunk images
    whose chunks reach, by the model run per chunk, the arms named in IMAGE_REACH -- asserted before the GPU is called;
  * the host entry;
  * hostile arrays (every entry but the buckets' first ones overwritten; the reference is defined on them and the model shows that the
    walk ends) in a child process under a time limit, each followed by a valid decode on the same context.  They reach the two arms no
    valid stream reaches: visits with uniq == 0 and a list whose first two positions hold the same symbol."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import rank_rows_model as M
from stage_guard import Guarded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEADS = (0, 1, 3, 15)

# image -> (events chunk one reaches, events chunk two reaches), by rank_rows_model.walk on each chunk's own rank array
IMAGE_REACH = {
    "zeros+ladder": (("run-past-known-64", "topup-full", "topup-cut", "topup-empty-row", "land-current", "drop-behind-zeros", "last-drop"),
                     ("fast-exit-64", "insert>=64", "drop>=64", "used-64", "zero-progress", "land-other", "land-current", "topup-cut")),
    # chunk one: the zero run, the ladder's arms, and a tail of front drops; chunk two: a fresh list of 256 in the middle of a round
    "ladder-split": (("run-past-known-64", "fast-exit-64", "insert>=64", "drop>=64", "used-64", "zero-progress", "general-tail"),
                     ("fast-exit-64", "drop>=64", "drop<64", "general-tail", "last-drop")),
    "sizes-split": (("run-past-known-64", "fast-zeros", "insert<64", "topup-cut", "land-other", "general-tail"),
                    ("fast-zeros", "insert<64", "topup-cut", "land-other", "drop-behind-zeros", "general-tail")),
}


@pytest.fixture(scope="module")
def gpu():
    import torch
    import jampack_amd as jam
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    yield torch, jam, ctx
    ctx.close()


@functools.lru_cache(maxsize=None)
def _expect(name):
    """(R, freq) of a crafted text from the oracle: computed once, shared, left unchanged"""
    from oracle.pyoracle import Oracle
    r, f = Oracle().rank_encode(M.crafted(name))
    f = f.astype("<i4")
    r.setflags(write=False)
    f.setflags(write=False)
    return r, f


def _rank_decode(torch, ctx, r, f, lead, what):
    g_r = Guarded(torch, np.array(r), lead)
    g_f = Guarded(torch, np.array(f), 4)                             # int32[256]: 4-byte aligned, off the 16-byte boundary
    ctx.rank_decode(g_r.ptr, g_f.ptr, len(r))
    g_f.check_unchanged(what + " freq")
    return g_r


def _ans_decode_exact(torch, ctx, oracle, t, what):
    enc = oracle.ans_encode(np.array(t))
    g_in = Guarded(torch, enc, 1)
    g_out = Guarded(torch, None, 5, cap=len(t))
    assert ctx.ans_decode(g_in.ptr, len(enc), g_out.ptr, len(t)) == len(t), what
    g_out.check_output(t, what=what)
    g_in.check_unchanged(what)


@pytest.mark.parametrize("name", M.TEXTS)
def test_probe_entry_in_place(gpu, name):
    torch, jam, ctx = gpu
    t = M.crafted(name)
    r, f = _expect(name)
    for lead in LEADS:
        what = f"rank_decode {name} lead={lead}"
        _rank_decode(torch, ctx, r, f, lead, what).check_output(t, what=what)
    g_t = Guarded(torch, np.array(t), 3)
    g_f = Guarded(torch, None, 4, cap=1024)
    ctx.rank_encode(g_t.ptr, g_f.ptr, len(t))
    g_t.check_output(r, what=f"rank_encode {name}")
    g_f.check_output(f, what=f"rank_encode {name} freq")


@pytest.mark.parametrize("name", M.TEXTS)
def test_product_path_at_exact_capacity(gpu, oracle, name):
    torch, jam, ctx = gpu
    _ans_decode_exact(torch, ctx, oracle, M.crafted(name), f"ans_decode {name}")


@pytest.mark.parametrize("name", M.IMAGES)
def test_two_chunk_images(gpu, oracle, name):
    torch, jam, ctx = gpu
    img = M.image(name)
    assert jam.CHUNK == M.CHUNK < len(img) < 2 * M.CHUNK
    for k, reach in enumerate(IMAGE_REACH[name]):
        c = img[k * M.CHUNK: (k + 1) * M.CHUNK]
        r, f = oracle.rank_encode(c)
        log = []
        T, ev = M.walk(r.tobytes(), f.tolist(), None, log)
        assert T == c.tobytes()
        missing = [e for e in reach if not ev.get(e)]
        assert not missing, (name, k, missing)
        print(name, "chunk", k, len(c), {e: n for e, n in ev.items() if not isinstance(n, set)})
        if name == "ladder-split":                                   # chunk one ends, chunk two starts inside the round robin of 256
            assert len(set(c[-M.TAIL:].tolist())) == M.TAIL and (k == 1 or c[-1] + 1 == img[M.CHUNK])
            tail = {e for at, e in log if at >= len(c) - M.TAIL}
            assert "drop<64" in tail and not tail & {"insert>=64", "drop>=64"}      # the tail cannot reach the packed register (the model's docstring)
            assert max(ev["drop-depths"]) == 255
    _ans_decode_exact(torch, ctx, oracle, img, f"ans_decode {name}")


@pytest.mark.parametrize("name", ["ladder", "sizes-shuffled", "sizes-sorted", "runs-200", "runs-1-150"])
def test_host_entry(gpu, name):
    torch, jam, ctx = gpu
    r, f = _expect(name)
    assert np.array_equal(jam.Postcoder().Decode(r, f), M.crafted(name)), name


_HOSTILE = r"""
import sys
root = sys.argv[1]
sys.path.insert(0, root)
sys.path.insert(0, root + "/tests")
import numpy as np
import torch
if not torch.cuda.is_available():
    print("RANK_ROWS_NO_DEVICE")
    sys.exit(3)
import jampack_amd as jam
import rank_rows_model as M
from oracle.pyoracle import Oracle
from stage_guard import Guarded
from test_gpu_rank_rows import _rank_decode
o = Oracle()
ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
done = 0
for name in M.HOSTILE_FROM:
    t = M.crafted(name)
    vr, vf = o.rank_encode(t)
    vf = vf.astype("<i4")
    for kind in M.HOSTILE_KINDS:
        R, freq = M.hostile(name, kind)
        r, f = np.frombuffer(R, dtype=np.uint8), np.array(freq, dtype="<i4")
        what = "hostile " + name + "/" + kind
        _rank_decode(torch, ctx, r, f, 3, what).check_output(o.rank_decode(r, f), what=what)
        _rank_decode(torch, ctx, vr, vf, 3, what + " then valid").check_output(t, what=what + " then valid")
        print("HOSTILE_OK " + name + "/" + kind, flush=True)
        done += 1
ctx.close()
print("RANK_ROWS_OK %d" % done)
"""


def test_hostile_arrays_equal_the_reference():
    """the arrays of test_rank_rows_model.test_hostile_arrays: the kernel gives the reference's bytes, writes nothing outside them, and the
    context decodes a valid array exactly afterwards.  Nothing here is meant to fail: the input is defined for the reference and the model
    shows that the walk ends; the child and its time limit keep a surprise from taking the session with it"""
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _HOSTILE, ROOT], capture_output=True, text=True)
    n = len(M.HOSTILE_FROM) * len(M.HOSTILE_KINDS)
    assert r.returncode == 0 and f"RANK_ROWS_OK {n}" in r.stdout, f"rc={r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"
    for name in M.HOSTILE_FROM:
        for kind in M.HOSTILE_KINDS:
            assert f"HOSTILE_OK {name}/{kind}" in r.stdout
