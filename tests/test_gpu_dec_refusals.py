"""The rANS decoder's refusals (k_dec_headers in ans_dec.hip, k_dec_rans in ans_dec_rans.hip, k_dec_rle in ans_dec_rank.hip, dec_collect's mapping
of the ST_* bits) on the crafted streams of dec_front_model: REFUSED, one stream per acceptance test, and STILL_ACCEPTED, their accepted
neighbours.  -m gpu

test_dec_front_model.py shows, from the streams alone, that each refused stream trips the one acceptance test it is named for and passes
every other, that the C oracle refuses it too, and which dropped or shifted test each one would expose.  Here the kernels are held to the
model's STATUS (not to the oracle's reason: the header walk of a whole block ends before any payload is looked at, the oracle goes chunk by
chunk), on guarded buffers:
  * the single entry, every refused stream at exact capacity and at input leads 0, 1, 2, 3 and 15 in rotation: the model's status exactly,
    the guards untouched, the input unchanged, nothing at all written where the header walk refused; a valid stream decoded exactly on the
    same context behind every refusal; every accepted neighbour with the oracle's bytes, its length and its chunk count; the
    precedence pair (a corrupt payload in front of a chunk that does not fit is E_CAPACITY, a malformed header under a short capacity
    E_CORRUPT);
  * the batch entry, every refused stream between valid ones in one call and once more reversed on the same arena: each block its own
    status, every valid block exact; then a chain of 1100 chunks in front of a payload-refused stream, so that the launch order is not the
    identity: the status word lands on the refused block and on no other;
  * the sizing pass (jpk_ans_decoded_sizes behind the archive index, and the host's jam.ans_decoded_size): corrupt where the header walk
    refuses, the declared size where only payload or symbols are bad -- the sizing reads no payload;
  * the block entry (Ans decode + inverse BWT, the decoder's buffers behind the caller's in the arena): one refused stream per stage
    beside valid blocks.

Why no stream here leaves a buffer: every one is first walked by the model (dec_front_model.verdict), whose own bounds assertions cover
every read of the input (the header walk's in[p - k] inside the chunk's header, the queue's loads clipped to the input as load() clips
them), every read of the RLE0 symbols (t < rlen, the look-ahead, the backward gather inside the chunk) and every store of a rank (below
olen); the symbols k_dec_rans stores are rlen per chunk, and rlen <= olen, total == olen and the capacity test have sized the buffers
before any chunk is listed.  The rank decoder runs on whatever ranks a refused chunk left, with counts that sum to olen: that it stays
inside olen bytes on any rank array is rank_rows_model's HOSTILE part (test_gpu_rank_rows.py).  Nothing here is meant to fault and no
mutant runs on the device: the mutants are switches of the CPU model only.  The children and their time limit keep a surprise from taking
the session with it."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import dec_front_model as M
from stage_guard import Guarded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_LEADS = (0, 1, 7)
AFTER = "rlen-65"                                                  # decoded on the same context behind every refused stream
PER_STAGE = ("total-olen-plus-1@3", "rans-taken-over-clen", "rle-21-digits-in-the-middle")      # headers, payload, symbols
PAD_BYTES = 600                                                    # a valid chunk in front, so that a frame declares more than the BWT trailer
BLOCK_SIZE = 8 << 20
TRAILER = 480
EMPTY = np.zeros(0, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.pyoracle import Oracle
    return Oracle()


@functools.lru_cache(maxsize=None)
def _verdict(name):
    """(status, reasons, stage) of the model's walk: its bounds assertions have held on the stream once this returns"""
    s, cap = M.crafted(_oracle(), name)
    return M.verdict(s, cap)[:3]


@functools.lru_cache(maxsize=None)
def _accepted(name):
    """the oracle's bytes of an accepted neighbour, as the model gives them too: computed once, shared, left unchanged"""
    s, cap = M.crafted(_oracle(), name)
    want = _oracle().ans_decode(s, cap)
    assert _verdict(name) == (M.OK, (), None) and M.decode(_oracle(), [s], [cap]) == [(M.OK, want.tobytes())]
    want.setflags(write=False)
    return want


def _mixed_names():
    """every refused stream with a valid one behind it"""
    return [n for pair in zip(M.REFUSED, M.BATCH * 9) for n in pair]


def _input(name):
    """(stream, capacity, expected status, expected bytes or None) of a crafted or a valid name"""
    if name in M.REFUSED:
        s, cap = M.crafted(_oracle(), name)
        return s, cap, _verdict(name)[0], None
    if name in M.STILL_ACCEPTED:
        s, cap = M.crafted(_oracle(), name)
        return s, cap, M.OK, _accepted(name)
    s, t = M.stream(_oracle(), name)
    return s, len(t), M.OK, t


def _context():
    import torch
    import jampack_amd as jam
    return torch, jam, jam.Context(0, torch.cuda.current_stream().cuda_stream)


def _decode_one(torch, jam, ctx, name, lead, out_lead):
    """one stream through ctx.ans_decode on guarded buffers at exact capacity -> status; everything the model says about it is asserted"""
    s, cap, status, want = _input(name)
    what = f"ans_decode {name} lead={lead}"
    g_in = Guarded(torch, np.array(s), lead)
    g_out = Guarded(torch, None, out_lead, cap=cap)
    try:
        n, got = ctx.ans_decode(g_in.ptr, len(s), g_out.ptr, cap), M.OK
    except jam.JampackError as e:
        n, got = 0, e.status
    assert got == status, f"{what}: status {got}, the model says {status}"
    if status == M.OK:
        assert n == cap == len(want), what
        g_out.check_output(want, used=n, what=what)
        assert ctx.stats().ans_chunks == len(M.headers(s, cap)[1]), what
    elif _verdict(name)[2] == "headers":
        g_out.check_output(EMPTY, used=0, what=what)              # the header walk refused: nothing at all is written
    else:
        g_out.check_guards(what)
    g_in.check_unchanged(what)
    return got


def _child_single():
    torch, jam, ctx = _context()
    for i, name in enumerate(M.REFUSED):
        status = _decode_one(torch, jam, ctx, name, M.IN_LEADS[i % 5], OUT_LEADS[i % 3])
        assert status != M.OK and _decode_one(torch, jam, ctx, AFTER, M.IN_LEADS[(i + 1) % 5], OUT_LEADS[(i + 1) % 3]) == M.OK
        print("OK %s %d" % (name, status), flush=True)
    for i, name in enumerate(M.STILL_ACCEPTED):
        for lead in M.IN_LEADS if _input(name)[1] < M.CHUNK else M.IN_LEADS[i % 5: i % 5 + 1]:
            assert _decode_one(torch, jam, ctx, name, lead, OUT_LEADS[i % 3]) == M.OK
        print("OK %s 0" % name, flush=True)
    # precedence: the header walk of the whole block ends before any payload is looked at
    for what, (s, cap), status in (("corrupt-payload-then-capacity", _payload_then_capacity(), M.E_CAPACITY),
                                   ("corrupt-header-and-capacity", (M.crafted(_oracle(), "total-olen-plus-1@1")[0], 10), M.E_CORRUPT)):
        assert M.verdict(s, cap)[0] == status and M.verdict(s, cap)[2] == "headers"
        g_in, g_out = Guarded(torch, np.array(s), 2), Guarded(torch, None, 1, cap=cap)
        with pytest.raises(jam.JampackError) as e:
            ctx.ans_decode(g_in.ptr, len(s), g_out.ptr, cap)
        assert e.value.status == status, (what, e.value)
        g_out.check_output(EMPTY, used=0, what=what)
        g_in.check_unchanged(what)
        print("OK %s %d" % (what, status), flush=True)
    ctx.close()


def _payload_then_capacity():
    """chunk 1's payload is corrupt and chunk 2 does not fit: (stream, capacity)"""
    s = np.concatenate((M.crafted(_oracle(), "rans-last-byte-flipped")[0], _oracle().ans_encode(M.side_text())))
    return s, M.T0_LEN + len(M.side_text()) - 1


def _batch(torch, ctx, names, what):
    ins = [_input(n) for n in names]
    g_in = [Guarded(torch, np.array(s), M.IN_LEADS[i % 5]) for i, (s, _, _, _) in enumerate(ins)]
    g_out = [Guarded(torch, None, OUT_LEADS[i % 3], cap=cap) for i, (_, cap, _, _) in enumerate(ins)]
    n, st = ctx.blocks_ans_decode([g.ptr for g in g_in], [len(s) for s, _, _, _ in ins], [g.ptr for g in g_out], [cap for _, cap, _, _ in ins])
    for i, (name, (s, cap, status, want)) in enumerate(zip(names, ins)):
        w = f"{what} block {i} ({name})"
        assert st[i] == status, f"{w}: status {st[i]}, the model says {status}"
        if status == M.OK:
            assert n[i] == cap, w
            g_out[i].check_output(want, used=cap, what=w)
        else:
            assert n[i] == 0, w
            if _verdict(name)[2] == "headers":
                g_out[i].check_output(EMPTY, used=0, what=w)
            else:
                g_out[i].check_guards(w)
        g_in[i].check_unchanged(w)
    return st


def _two_chunks_second_refused():
    side = _oracle().ans_encode(M.side_text())
    s = np.concatenate((side, M.crafted(_oracle(), "rans-last-byte-flipped")[0]))
    cap = len(M.side_text()) + M.T0_LEN
    assert M.verdict(s, cap)[:3] == (M.E_CORRUPT, ("refuse-states",), "payload")
    return s, cap


def _child_batch():
    torch, jam, ctx = _context()
    names = _mixed_names()
    _batch(torch, ctx, names, "mixed batch")
    _batch(torch, ctx, names[::-1], "mixed batch, reversed on the same arena")
    for name in names:
        print("OK %s %d" % (name, _input(name)[2]), flush=True)
    # 1100 chains in front: the launch order is not the identity, and the refused block's status word is its own
    big, t = M.stream(_oracle(), "big-chain")
    two, cap = _two_chunks_second_refused()
    v, vt = M.stream(_oracle(), AFTER)
    g_in = [Guarded(torch, np.array(s), lead) for s, lead in ((big, 1), (two, 2), (v, 3))]
    g_out = [Guarded(torch, None, lead, cap=c) for c, lead in ((len(t), 7), (cap, 1), (len(vt), 0))]
    n, st = ctx.blocks_ans_decode([g.ptr for g in g_in], [len(big), len(two), len(v)], [g.ptr for g in g_out], [len(t), cap, len(vt)])
    assert st == [0, M.E_CORRUPT, 0] and n == [len(t), 0, len(vt)], (st, n)
    assert ctx.stats().ans_chunks == len(M.BIG_CHAIN) + 3
    g_out[0].check_output(t, what="big-chain beside a refused block")
    g_out[1].check_guards("the refused block behind big-chain")
    g_out[2].check_output(vt, what="the valid block behind the refused one")
    for g in g_in:
        g.check_unchanged("big-chain batch")
    print("OK big-chain-batch", flush=True)
    ctx.close()


def _frame(payload):
    """one frame of a plain archive around an Ans payload (the index reads the header and the chunk headers, never the crc)"""
    return np.concatenate((np.frombuffer(_oracle().block_header(0, len(payload), BLOCK_SIZE), dtype=np.uint8), payload))


@functools.lru_cache(maxsize=None)
def _pad():
    return _oracle().ans_encode((np.arange(PAD_BYTES) % 251).astype(np.uint8))


def _sizes_expected(name):
    """(corrupt?, declared bytes) of pad + stream by the model's header walk without a capacity"""
    s = np.concatenate((_pad(), M.crafted(_oracle(), name)[0]))
    status, _, _, totals = M.headers(s, 1 << 40)
    return s, status != M.OK, totals[0]


def _child_sizes():
    torch, jam, ctx = _context()
    for name in list(M.REFUSED) + list(M.STILL_ACCEPTED):
        s, corrupt, declared = _sizes_expected(name)
        a = _frame(s)
        g = Guarded(torch, a, 5)
        ix, host = ctx.jam_index(g.ptr, len(a)), jam.jam_index(a)
        for which, x in (("device", ix), ("host", host)):
            w = f"sizes of {name} ({which})"
            if corrupt:
                assert (x.frames, x.bad_frame) == (0, 0), w
            else:
                assert (x.frames, x.bad_frame) == (1, -1) and x.frame(0)[1] == declared - TRAILER == x.raw_len, (w, x.frame(0), declared)
        g.check_unchanged(name)
        # the host entry on the stream itself
        st, infos, _, totals = M.headers(M.crafted(_oracle(), name)[0], 1 << 40)
        try:
            got = jam.ans_decoded_size(M.crafted(_oracle(), name)[0])
        except jam.JampackError as e:
            got = e.status
        assert got == ((totals[0], len(infos)) if st == M.OK else M.E_CORRUPT), (name, got)
        ix.close()
        host.close()
        print("OK %s %s" % (name, "corrupt" if corrupt else declared), flush=True)
    ctx.close()


def _child_blocks():
    torch, jam, ctx = _context()
    rng = np.random.default_rng(7)
    texts = [rng.integers(0, 256, n).astype(np.uint8) for n in (5000, 3001)] + [np.tile(np.frombuffer(b"refusals ", dtype=np.uint8), 80)]
    valid = [_oracle().compress_block(t) for t in texts]
    streams, caps, want = [], [], []
    for t, v, r in zip(texts, valid, PER_STAGE):
        streams += [v, M.crafted(_oracle(), r)[0]]
        caps += [len(t), 400]                                     # 400 + the trailer is above what any of the three declares
        want += [t, None]
    for _ in range(2):                                            # twice on the same arena
        g_in = [Guarded(torch, np.array(s), (3 * i) % 16) for i, s in enumerate(streams)]
        g_out = [Guarded(torch, None, (5 * i + 1) % 16, cap=c) for i, c in enumerate(caps)]
        n, st = ctx.blocks_decompress([g.ptr for g in g_in], [len(s) for s in streams], [g.ptr for g in g_out], caps)
        assert st == [0, M.E_CORRUPT] * 3, st
        for i, t in enumerate(want):
            w = f"blocks_decompress block {i}"
            if t is None:
                assert n[i] == 0, w
                g_out[i].check_output(EMPTY, used=0, what=w)      # the inverse BWT never ran on it
            else:
                assert n[i] == len(t), w
                g_out[i].check_output(t, used=n[i], what=w)
            g_in[i].check_unchanged(w)
    for r in PER_STAGE:
        print("OK %s %d" % (r, M.E_CORRUPT), flush=True)
    ctx.close()


_CHILD = "import sys; sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tests']; import torch; import test_gpu_dec_refusals as t; getattr(t, sys.argv[2])()"


def _run_child(fn):
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _CHILD, ROOT, fn], capture_output=True, text=True)
    assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"
    return r.stdout.splitlines()


def test_the_model_has_walked_every_stream():
    """before a kernel sees one: the model's verdict, with its bounds assertions on the way, and the stage per refused stream"""
    for name in M.REFUSED:
        status, reasons, stage = _verdict(name)
        assert status == (M.E_CAPACITY if name.startswith("capacity-") else M.E_CORRUPT) and reasons == tuple(sorted(M.REASON[name])), name
        assert _sizes_expected(name)[1] == (stage == "headers" and status == M.E_CORRUPT), name
    for name in M.STILL_ACCEPTED:
        assert len(_accepted(name)) == M.crafted(_oracle(), name)[1] and not _sizes_expected(name)[1]
    assert [_verdict(n)[2] for n in PER_STAGE] == ["headers", "payload", "payload"]
    assert M.REASON[PER_STAGE[1]] == ("refuse-taken-over-clen",) and M.REASON[PER_STAGE[2]] == ("refuse-rle-21-digits",)
    assert max(M.crafted(_oracle(), n)[1] for n in PER_STAGE) <= 400 + TRAILER and len(M.REFUSED) <= 9 * len(M.BATCH)


def test_single_entry_refuses_with_the_models_status():
    out = _run_child("_child_single")
    for name in M.REFUSED:
        assert "OK %s %d" % (name, _verdict(name)[0]) in out, name
    for name in M.STILL_ACCEPTED:
        assert "OK %s 0" % name in out, name
    assert "OK corrupt-payload-then-capacity %d" % M.E_CAPACITY in out and "OK corrupt-header-and-capacity %d" % M.E_CORRUPT in out


def test_batch_entry_refuses_each_block_alone():
    out = _run_child("_child_batch")
    for name in M.REFUSED:
        assert "OK %s %d" % (name, _verdict(name)[0]) in out, name
    assert "OK big-chain-batch" in out


def test_sizing_pass_reads_headers_only():
    out = _run_child("_child_sizes")
    for name in list(M.REFUSED) + list(M.STILL_ACCEPTED):
        corrupt, declared = _sizes_expected(name)[1:]
        assert "OK %s %s" % (name, "corrupt" if corrupt else declared) in out, name


def test_block_entry_with_the_decoders_buffers_behind_the_callers():
    out = _run_child("_child_blocks")
    for name in PER_STAGE:
        assert "OK %s %d" % (name, M.E_CORRUPT) in out, name
