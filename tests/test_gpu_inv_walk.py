"""The inverse BWT's kernels (bwt_inv.hip) on the crafted images of inv_walk_model: splitter walk, 256-byte slots, 16-byte flushes, symbol
table, slot ranking, copy-out, the batch form, corrupt images.  -m gpu

test_inv_walk_model.py shows, from the images alone, which cases of the scheme each one reaches (a head that is a splitter, a last splitter
outside the block, sub-lists of exactly 256, 257, 512 and 513 bytes and one of 833, every lut_shift and tile count up to 65 639 bytes, slot
counts below, at and above a power of two, cycles without, with one and with several splitters) and which one-token changes of the scheme
each one would expose.  Here the kernels decode them, bit-exact, on guarded buffers:
  * the single entry at two input and two output leads; the context's counters must be the model's -- inv_overflow_slots depends on where
    the hashed splitters lie and on the order of the stop and the overflow test, so equal counters show that the image reached its case
    on the device;
  * the 120-chain comparator and the fused entry (Ans decode + inverse BWT) on the same images;
  * the batch entry: 35 images in one set of launches, the largest neither first nor last, in both orders, and a batch whose round count is odd;
    in a child process with JPK_INV_BATCH=0 the per-block launches;
  * corrupt images, in a child process under a time limit: each is first walked by the model, whose bounds assertions are the evidence
    that the kernels stay inside their buffers on it; the device must then report exactly the model's status (and for the edit that is
    still valid, the model's other text), leave the guards alone, count the model's overflow slots, decode a valid image afterwards, and
    in a batch fail that block alone.
Nothing here is meant to fault and no mutant runs on the device: the mutants are switches of the CPU model only."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import inv_walk_model as M
from stage_guard import Guarded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEADS = ((0, 0), (0, 7), (13, 0), (13, 7))                         # (input, output) bytes behind a 256-byte-aligned address
STILL_VALID = "swap-valid"
CORRUPT = tuple(n for n in M.EDITED if n != STILL_VALID)
DECODABLE = tuple(M.VALID) + (STILL_VALID,)
FUSED = ("rand-960-256", "rand-1920-256", "rand-1920-257", "rand-4080", "rand-4200", "bits-4200", "rand-8160", "rand-8280", "rand-16320",
         "rand-16440-512", "rand-16440-513", "rand-16440-chain3", "rand-65520", "rand-65639")
AFTER_CORRUPT = "rand-1920-257"                                    # decoded on the same context behind every corrupt image


def _batch_names():
    """every decodable image, the two largest in the middle: the grids are wider than most jobs need and pos_base is non-zero for all but
    the first"""
    names = [n for n in DECODABLE if n not in ("rand-65520", "rand-65639")]
    names.insert(11, "rand-65639")
    names.insert(23, "rand-65520")
    return names


def _mixed_names():
    """the same with every corrupt image in between, the first one right at the start"""
    names = _batch_names()
    for k, c in enumerate(CORRUPT):
        names.insert(4 * k, c)
    return names


@pytest.fixture(scope="module")
def gpu():
    import torch
    import jampack_amd as jam
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    yield torch, jam, ctx
    ctx.close()


@functools.lru_cache(maxsize=None)
def _expect(name):
    """(model result, its text as an array, or None where the model says corrupt): computed once, shared, left unchanged"""
    r = M.crafted_walk(name)
    assert not isinstance(r, str), f"{name}: the model trips on it -- a finding about the kernels, to be read from the code: {r}"
    if r.status != 0:
        return r, None
    t = np.frombuffer(r.text, dtype=np.uint8)
    return r, t


@functools.lru_cache(maxsize=None)
def _stream(name):
    """the oracle's Ans stream of a crafted image"""
    from oracle.pyoracle import Oracle
    s = Oracle().ans_encode(np.array(M.image(name)))
    s.setflags(write=False)
    return s


def _assert_counters(ctx, r, what):
    s = ctx.stats()
    assert s.inv_overflow_slots == r.novf, f"{what}: {s.inv_overflow_slots} overflow slots on the device, the model has {r.novf}"
    assert s.inv_splitters == r.layout["nsplit"] + 1, what


def _single(torch, jam, ctx, name, lead_in, lead_out):
    """one image through ctx.bwt_inverse on guarded buffers -> status; everything the model says about it is asserted"""
    r, t = _expect(name)
    img = np.array(M.image(name))
    cap = len(img) - M.TRAILER
    what = f"bwt_inverse {name} lead_in={lead_in} lead_out={lead_out}"
    g_in = Guarded(torch, img, lead_in)
    g_out = Guarded(torch, None, lead_out, cap=cap)
    try:
        m = ctx.bwt_inverse(g_in.ptr, len(img), g_out.ptr, cap)
        status = 0
    except jam.JampackError as e:
        m, status = 0, e.status
    assert status == r.status, f"{what}: status {status}, the model says {r.status}"
    if status == 0:
        assert m == cap, what
        g_out.check_output(t, used=m, what=what)
    else:
        g_out.check_guards(what)
    g_in.check_unchanged(what)
    _assert_counters(ctx, r, what)
    return status


def _batch(torch, ctx, names, what):
    """one ctx.blocks_decompress call over the images' Ans streams, every output guarded: each block has the model's status and text"""
    streams = [_stream(n) for n in names]
    caps = [len(M.image(n)) - M.TRAILER for n in names]
    g_in = [Guarded(torch, np.array(s), (3 * i) % 16) for i, s in enumerate(streams)]
    g_out = [Guarded(torch, None, (5 * i + 1) % 16, cap=c) for i, c in enumerate(caps)]
    bn, st = ctx.blocks_decompress([g.ptr for g in g_in], [len(s) for s in streams], [g.ptr for g in g_out], caps)
    for i, n in enumerate(names):
        r, t = _expect(n)
        w = f"{what} block {i} {n}"
        assert st[i] == r.status, f"{w}: status {st[i]}, the model says {r.status}"
        if r.status == 0:
            assert bn[i] == caps[i], w
            g_out[i].check_output(t, used=bn[i], what=w)
        else:
            assert bn[i] == 0, w
            g_out[i].check_guards(w)
        g_in[i].check_unchanged(w)


# ---- valid images ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DECODABLE)
def test_single_entry(gpu, oracle, name):
    torch, jam, ctx = gpu
    r, t = _expect(name)
    assert r.status == 0 and r.text == oracle.bwt_inverse(M.image(name)).tobytes()
    for lead_in, lead_out in LEADS:
        assert _single(torch, jam, ctx, name, lead_in, lead_out) == 0


@pytest.mark.parametrize("name", tuple(M.VALID))
def test_comparator_gives_the_same_bytes(gpu, name):
    """(not the still-valid edit: the comparator starts 120 chains from all 120 trailer indices, and 119 of that image's are another text's)"""
    torch, jam, ctx = gpu
    r, t = _expect(name)
    img = np.array(M.image(name))
    g_in = Guarded(torch, img, 5)
    g_out = Guarded(torch, None, 9, cap=len(t))
    m, _ = ctx.bwt_inverse_chains120(g_in.ptr, len(img), g_out.ptr, len(t))
    assert m == len(t)
    g_out.check_output(t, used=m, what=f"chains120 {name}")
    g_in.check_unchanged(f"chains120 {name}")


@pytest.mark.parametrize("name", FUSED)
def test_fused_entry(gpu, name):
    torch, jam, ctx = gpu
    r, t = _expect(name)
    enc = np.array(_stream(name))
    g_in = Guarded(torch, enc, 1)
    g_out = Guarded(torch, None, 5, cap=len(t))
    m = ctx.block_decompress(g_in.ptr, len(enc), g_out.ptr, len(t))
    assert m == len(t)
    g_out.check_output(t, used=m, what=f"block_decompress {name}")
    g_in.check_unchanged(f"block_decompress {name}")
    _assert_counters(ctx, r, f"block_decompress {name}")


def test_the_batch_lists_are_what_the_tests_need():
    names = _batch_names()
    sizes = [len(M.image(n)) for n in names]
    assert len(names) >= 32 and sorted(names) == sorted(DECODABLE)
    assert 0 < sizes.index(max(sizes)) < len(names) - 1 and max(sizes) < 4 << 20
    assert sizes[0] < max(sizes) and sizes[-1] < max(sizes)
    mixed = _mixed_names()
    assert len(mixed) >= 32 and set(CORRUPT) < set(mixed) and mixed[0] in CORRUPT
    assert {M.EDITED[c][0] for c in CORRUPT} <= set(mixed)                       # every corrupt image sits beside the valid one it was made from


def test_batch_entry_in_both_orders(gpu):
    torch, jam, ctx = gpu
    names = _batch_names()
    _batch(torch, ctx, names, "batch")
    _batch(torch, ctx, names[::-1], "batch reversed")


def test_batch_entry_with_an_odd_round_count(gpu):
    """the batch runs the rounds of its largest job and leaves the final distances in buffer pair rounds & 1: the full list ends in A
    (12 rounds), this one -- nothing above 8 280 sorted bytes, three images twice to stay a batch of 32 -- in B (9 rounds)"""
    torch, jam, ctx = gpu
    names = [n for n in _batch_names() if M.crafted_walk(n).n <= 8280]
    names += names[3:6]
    assert len(names) >= 32
    assert max(M.crafted_walk(n).layout["rounds"] for n in names) == 9 and max(M.crafted_walk(n).layout["rounds"] for n in _batch_names()) == 12
    _batch(torch, ctx, names, "batch of 9 rounds")


def _child_lanes():
    import torch
    import jampack_amd as jam
    assert os.environ.get("JPK_INV_BATCH") == "0"
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    names = _batch_names()
    _batch(torch, ctx, names, "per-block launches")
    ctx.close()
    print("INV_WALK_LANES_OK %d" % len(names))


def _child_corrupt():
    import torch
    import jampack_amd as jam
    for name in CORRUPT:                                               # the model first: its bounds assertions hold on every one of them
        assert _expect(name)[0].status == M.E_CORRUPT
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    for name in CORRUPT + (STILL_VALID,):
        status = _single(torch, jam, ctx, name, 3, 6)
        assert _single(torch, jam, ctx, AFTER_CORRUPT, 3, 6) == 0
        print("INV_WALK_EDIT_OK %s %d" % (name, status), flush=True)
    mixed = _mixed_names()
    _batch(torch, ctx, mixed, "mixed batch")
    assert _single(torch, jam, ctx, AFTER_CORRUPT, 0, 0) == 0
    ctx.close()
    print("INV_WALK_CORRUPT_OK %d" % len(mixed))


_CHILD = "import sys; sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tests']; import torch; import test_gpu_inv_walk as t; getattr(t, sys.argv[2])()"


def _run_child(fn, env=None):
    return subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _CHILD, ROOT, fn], env=env, capture_output=True, text=True)


def test_per_block_launches_give_the_same_bytes():
    r = _run_child("_child_lanes", dict(os.environ, JPK_INV_BATCH="0"))
    assert r.returncode == 0 and f"INV_WALK_LANES_OK {len(_batch_names())}" in r.stdout, f"rc={r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"


# ---- corrupt images -------------------------------------------------------------------------------------------------------------------------
def test_corrupt_images_fail_with_the_models_status_and_fail_alone():
    """single entry: JPK_E_CORRUPT exactly where the model's verdict says so (the still-valid edit returns the model's other text), guards
    intact, the model's overflow-slot count, a valid image decoded on the same context afterwards.  Then all of them in one batch of 43.
    Nothing here is meant to fault: the model has walked every image with its bounds assertions on before the device sees one; the child
    and its time limit keep a surprise from taking the session with it"""
    for name in CORRUPT:
        r, t = _expect(name)
        assert r.status == M.E_CORRUPT and t is None
    assert _expect(STILL_VALID)[0].status == 0 and _expect(STILL_VALID)[0].text != _expect(M.EDITED[STILL_VALID][0])[0].text
    r = _run_child("_child_corrupt")
    assert r.returncode == 0 and f"INV_WALK_CORRUPT_OK {len(_mixed_names())}" in r.stdout, f"rc={r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"
    for name in CORRUPT:
        assert f"INV_WALK_EDIT_OK {name} {M.E_CORRUPT}" in r.stdout
    assert f"INV_WALK_EDIT_OK {STILL_VALID} 0" in r.stdout
