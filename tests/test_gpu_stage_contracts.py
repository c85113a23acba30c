"""The device-buffer stage entries (jpk_dev_*) and the kernel probes at odd addresses, exact capacity and the 1 MiB chunk edge.  -m gpu

Every buffer a call sees sits in a guarded allocation (stage_guard.Guarded): the payload `lead` bytes behind a 256-byte-aligned address,
4 KiB of sentinel in front of it and behind it.  After every call
  (a) the result equals the oracle byte for byte,
  (b) the guards in front of and behind [out, out + out_cap) still hold the sentinel,
  (c) after a success with out_len < out_cap so do the bytes [out + out_len, out + out_cap),
  (d) a const input is unchanged, guards included.
Typed arrays (int32 frequencies and suffix arrays, uint16 symbols, uint32 pairs) keep the alignment of their element type and are moved
off the 16-byte boundary by that much; byte buffers start anywhere.
"""
import numpy as np
import pytest

from stage_guard import Guarded

pytestmark = pytest.mark.gpu

MiB = 1 << 20
TRAILER = 480
E_CAPACITY = -2

BWT_LENGTHS = [1, 2, 7, 15, 16, 17, 31, 33, 119, 120, 121, 4097, 70_001]


@pytest.fixture(scope="module")
def gpu():
    import torch
    import jampack_amd as jam
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    yield torch, jam, ctx
    ctx.close()


def _fails_with_capacity(jam, call):
    with pytest.raises(jam.JampackError) as e:
        call()
    assert e.value.status == E_CAPACITY, e.value
    return True


# ---- forward BWT: the head (mis = 16 - address % 16 bytes, clamped to n), the uint4 body and the tail of the text readers ----------------
def _fwd_expect(oracle, t):
    # below 120 bytes the reference leaves part of the trailer as it found it (bwt.cpp:35): the oracle starts from the sentinel too
    return oracle.bwt_forward(t, prefill=0xA5) if len(t) < 120 else oracle.bwt_forward(t)


def _fwd_one(torch, jam, ctx, t, exp, lead_in, lead_out):
    n = len(t)
    what = f"bwt_forward n={n} lead_in={lead_in} lead_out={lead_out}"
    g_in = Guarded(torch, t, lead_in)
    g_out = Guarded(torch, None, lead_out, cap=n + TRAILER)
    # one byte short is refused before anything runs
    assert _fails_with_capacity(jam, lambda: ctx.bwt_forward(g_in.ptr, n, g_out.ptr, n + TRAILER - 1)), what
    g_out.check_output(np.zeros(0, np.uint8), used=0, what=what + " (cap - 1)")
    m = ctx.bwt_forward(g_in.ptr, n, g_out.ptr, n + TRAILER)
    assert m == n + TRAILER, what
    g_out.check_output(exp, used=m, what=what)
    g_in.check_unchanged(what)


@pytest.mark.parametrize("kind", ["text", "two"])
def test_forward_bwt_at_every_input_residue(gpu, oracle, kind):
    torch, jam, ctx = gpu
    for n in BWT_LENGTHS:
        t = jam.corpus.make(kind, n, 71)
        exp = _fwd_expect(oracle, t)
        for lead_in in range(16):
            _fwd_one(torch, jam, ctx, t, exp, lead_in, (lead_in * 5 + 3) % 16)


def test_forward_bwt_vector_loop_over_many_workgroups(gpu, oracle):
    torch, jam, ctx = gpu
    t = jam.corpus.make("text", MiB + 17, 72)
    exp = oracle.bwt_forward(t)
    for lead_in in (1, 8, 15):
        _fwd_one(torch, jam, ctx, t, exp, lead_in, (lead_in * 5 + 3) % 16)


# ---- inverse BWT ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["text", "two"])
def test_inverse_bwt_at_odd_addresses_and_exact_capacity(gpu, oracle, kind):
    torch, jam, ctx = gpu
    leads_in, leads_out = (0, 1, 3, 8, 13), (0, 1, 7, 15)
    for n in BWT_LENGTHS:
        t = jam.corpus.make(kind, n, 73)
        img = oracle.bwt_forward(t)
        for k in range(20):                                  # 5 and 4 are coprime: round robin meets every pair
            lead_in, lead_out = leads_in[k % 5], leads_out[k % 4]
            what = f"bwt_inverse n={n} lead_in={lead_in} lead_out={lead_out}"
            g_in = Guarded(torch, img, lead_in)
            g_out = Guarded(torch, None, lead_out, cap=n)
            m = ctx.bwt_inverse(g_in.ptr, len(img), g_out.ptr, n)
            assert m == n, what
            g_out.check_output(t, used=m, what=what)
            g_in.check_unchanged(what)
            if k < 4 and n > 1:
                assert _fails_with_capacity(jam, lambda: ctx.bwt_inverse(g_in.ptr, len(img), g_out.ptr, n - 1)), what


# ---- ANS encode / decode: images that end on, one short of and one past the 1 MiB chunk edge ---------------------------------------------
ANS_LENGTHS = [1, 479, 480, 481, MiB - 1, MiB, MiB + 1, 2 * MiB - 1, 2 * MiB, 2 * MiB + 1]
RUN = 5000
RUN_STARTS = (MiB - 2500, MiB - 1, MiB)        # the rank-0 run begins before, on and after the edge; chunks are coded independently


@pytest.fixture(scope="module")
def ans_sources(oracle):
    """(the head of a text block's BWT image, random bytes): made once, never written to"""
    import jampack_amd as jam
    return (oracle.bwt_forward(jam.corpus.make("text", 2 * MiB + 1, 74))[: 2 * MiB + 1].copy(), jam.corpus.make("random", 2 * MiB + 1, 75))


# one case per content and length (the dense chunks of random bytes take the serial decoder longest), one per run start
ANS_CASES = [f"text-{L}" for L in ANS_LENGTHS] + [f"random-{L}" for L in ANS_LENGTHS] + [f"straddle-{s}" for s in RUN_STARTS]
_ANS_CACHE = {}


def _ans_images(oracle, ans_sources, case):
    """[(name, image, the oracle's stream)] of one case -- computed once, shared by the encode and the decode test"""
    if case not in _ANS_CACHE:
        text_image, random_bytes = ans_sources
        content, arg = case.split("-")
        if content == "straddle":
            start, imgs = int(arg), []
            for L in ANS_LENGTHS:
                if L <= start:
                    continue                                 # (the run must lie inside the image: the lengths from 2^20 - 1 up)
                img = text_image[:L].copy()
                img[start: min(start + RUN, L)] = 0x41
                imgs.append((f"straddle start={start} L={L}", img))
        else:
            imgs = [(f"{content} L={arg}", (text_image if content == "text" else random_bytes)[: int(arg)])]
        _ANS_CACHE[case] = [(name, img, oracle.ans_encode(img)) for name, img in imgs]
    return _ANS_CACHE[case]


LEADS_IN, LEADS_OUT = (0, 1, 15), (0, 3, 9)


@pytest.mark.parametrize("case", ANS_CASES)
def test_ans_encode_at_chunk_edges_and_exact_capacity(gpu, oracle, ans_sources, case):
    torch, jam, ctx = gpu
    for i, (name, img, want) in enumerate(_ans_images(oracle, ans_sources, case), ANS_CASES.index(case)):
        L = len(img)
        m = len(want)
        for k in range(3):
            lead_in, lead_out = LEADS_IN[k], LEADS_OUT[(k + i) % 3]
            what = f"ans_encode {name} lead_in={lead_in} lead_out={lead_out}"
            g_in = Guarded(torch, img, lead_in)
            g_out = Guarded(torch, None, lead_out, cap=m)
            got = ctx.ans_encode(g_in.ptr, L, g_out.ptr, m)
            assert got == m, what
            g_out.check_output(want, used=m, what=what)
            g_in.check_unchanged(what)
            g_short = Guarded(torch, None, lead_out, cap=m - 1)
            assert _fails_with_capacity(jam, lambda: ctx.ans_encode(g_in.ptr, L, g_short.ptr, m - 1)), what
            g_short.check_guards(what + " (cap - 1)")
            g_in.check_unchanged(what + " (cap - 1)")


@pytest.mark.parametrize("case", ANS_CASES)
def test_ans_decode_at_chunk_edges_and_exact_capacity(gpu, oracle, ans_sources, case):
    torch, jam, ctx = gpu
    for i, (name, img, stream) in enumerate(_ans_images(oracle, ans_sources, case), ANS_CASES.index(case)):
        L = len(img)
        for k in range(3):
            lead_in, lead_out = LEADS_IN[k], LEADS_OUT[(k + i) % 3]
            what = f"ans_decode {name} lead_in={lead_in} lead_out={lead_out}"
            g_in = Guarded(torch, stream, lead_in)
            g_out = Guarded(torch, None, lead_out, cap=L)
            got = ctx.ans_decode(g_in.ptr, len(stream), g_out.ptr, L)
            assert got == L, what
            g_out.check_output(img, used=L, what=what)
            g_in.check_unchanged(what)
            g_short = Guarded(torch, None, lead_out, cap=L - 1)
            assert _fails_with_capacity(jam, lambda: ctx.ans_decode(g_in.ptr, len(stream), g_short.ptr, L - 1)), what
            g_short.check_guards(what + " (cap - 1)")
            g_in.check_unchanged(what + " (cap - 1)")


# ---- the fused block entries ------------------------------------------------------------------------------------------------------------
# n = 2^20 - 480 makes the BWT image exactly one chunk long, 2^20 - 479 one byte more
@pytest.mark.parametrize("n", [120, 121, 4097, MiB - 480, MiB - 479, 1_300_001])
def test_block_entries_at_odd_addresses_and_exact_capacity(gpu, oracle, n):
    torch, jam, ctx = gpu
    t = jam.corpus.make("text", n, 76)
    want = oracle.compress_block(t)
    m = len(want)
    for lead_in in (1, 15):
        for lead_out in (2, 7):
            what = f"block n={n} lead_in={lead_in} lead_out={lead_out}"
            g_t = Guarded(torch, t, lead_in)
            g_c = Guarded(torch, None, lead_out, cap=m)
            assert ctx.block_compress(g_t.ptr, n, g_c.ptr, m) == m, what
            g_c.check_output(want, used=m, what=what + " compress")
            g_t.check_unchanged(what + " compress")
            g_short = Guarded(torch, None, lead_out, cap=m - 1)
            assert _fails_with_capacity(jam, lambda: ctx.block_compress(g_t.ptr, n, g_short.ptr, m - 1)), what
            g_short.check_guards(what + " compress (cap - 1)")

            g_s = Guarded(torch, want, lead_in)
            g_o = Guarded(torch, None, lead_out, cap=n)
            assert ctx.block_decompress(g_s.ptr, m, g_o.ptr, n) == n, what
            g_o.check_output(t, used=n, what=what + " decompress")
            g_s.check_unchanged(what + " decompress")
            g_short = Guarded(torch, None, lead_out, cap=n - 1)
            assert _fails_with_capacity(jam, lambda: ctx.block_decompress(g_s.ptr, m, g_short.ptr, n - 1)), what
            g_short.check_guards(what + " decompress (cap - 1)")
            g_roomy = Guarded(torch, None, lead_out, cap=n + 1000)
            assert ctx.block_decompress(g_s.ptr, m, g_roomy.ptr, n + 1000) == n, what
            g_roomy.check_output(t, used=n, what=what + " decompress (cap + 1000)")      # the 1000 spare bytes stay untouched
            g_s.check_unchanged(what + " decompress (cap + 1000)")


# ---- the rank coder, in place -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["text", "runs"])
def test_rank_coder_in_place_at_odd_addresses(gpu, oracle, kind):
    torch, jam, ctx = gpu
    for n in (1, 15, 16, 17, 4095, 4096, 4097, 3 * 4096 + 17):
        t = jam.corpus.make(kind, n, 77)
        r, f = oracle.rank_encode(t)
        for lead in (0, 1, 2, 3, 5, 8, 15):
            what = f"rank coder {kind} n={n} lead={lead}"
            g_t = Guarded(torch, t, lead)
            g_f = Guarded(torch, None, 4, cap=1024)                       # int32[256]: 4-byte aligned, off the 16-byte boundary
            ctx.rank_encode(g_t.ptr, g_f.ptr, n)
            g_t.check_output(r, what=what + " encode")
            g_f.check_output(f.astype("<i4"), what=what + " encode freq")
            g_r = Guarded(torch, r, lead)
            g_f = Guarded(torch, f.astype("<i4"), 4)
            ctx.rank_decode(g_r.ptr, g_f.ptr, n)
            g_r.check_output(t, what=what + " decode")
            g_f.check_unchanged(what + " decode freq")


# ---- RLE0 and model probes --------------------------------------------------------------------------------------------------------------
# The ABI names no capacity for the two outputs.  jpk_rle_encode_device runs the stage in the context's arena and copies exactly *rlen
# uint16 symbols to d_rle; jpk_model_pairs_device copies exactly 2 * rlen uint32 words (rlen packed pairs of two) to d_pairs: a caller that
# knows rlen (at most len symbols) needs no more room than that, so the guards stand directly behind rlen symbols and 2 * rlen words.
@pytest.mark.parametrize("kind", ["text", "runs"])
def test_rle_and_model_probes_at_odd_addresses(gpu, oracle, kind):
    torch, jam, ctx = gpu
    for n in (1, 15, 16, 17, 4096, 4097, 70_000):
        r, _ = oracle.rank_encode(jam.corpus.make(kind, n, 78))
        s = oracle.rle_encode(r)
        pairs = oracle.model_pairs(s)
        assert len(pairs) == 2 * len(s)
        for lead in (1, 3, 7, 15):
            what = f"rle/model {kind} n={n} lead={lead}"
            g_r = Guarded(torch, r, lead)
            g_s = Guarded(torch, None, 2, cap=2 * len(s))                 # uint16: 2 bytes off the aligned base
            assert ctx.rle_encode(g_r.ptr, n, g_s.ptr) == len(s), what
            g_s.check_output(s.astype("<u2"), what=what + " rle")
            g_r.check_unchanged(what + " rle")
        for off16, off32 in ((2, 4), (6, 12), (14, 8)):
            what = f"rle/model {kind} n={n} symbols at +{off16} pairs at +{off32}"
            g_s = Guarded(torch, s.astype("<u2"), off16)
            g_p = Guarded(torch, None, off32, cap=8 * len(s))             # uint32: 4 bytes off the aligned base
            ctx.model_pairs(g_s.ptr, len(s), g_p.ptr)
            g_p.check_output(pairs.astype("<u4"), what=what + " pairs")
            g_s.check_unchanged(what + " pairs")


# ---- suffix array probe -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["text", "two"])
def test_suffix_array_probe_at_every_text_residue(gpu, oracle, kind):
    torch, jam, ctx = gpu
    for n in (1, 7, 16, 17, 5000):
        t = jam.corpus.make(kind, n, 79)
        sa = oracle.suffix_array(t).astype("<i4")
        for lead in range(16):
            what = f"suffix_array {kind} n={n} lead={lead}"
            g_t = Guarded(torch, t, lead)
            g_sa = Guarded(torch, None, 4, cap=4 * n)                     # int32[n]: 4 bytes off the aligned base
            ctx.suffix_array(g_t.ptr, n, g_sa.ptr)
            g_sa.check_output(sa, what=what)
            g_t.check_unchanged(what)
