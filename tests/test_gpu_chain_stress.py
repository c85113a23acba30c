"""Stress test of the rANS encoder chain (k_rans_lanes, ans_enc_chain.hip; ans.cpp:189-208).

The chain keeps sixteen batches of step records in flight while other blocks' suffix sorts saturate the memory system; round 3
produced timing-dependent wrong bytes there (about one per 10^6 steps) when records in flight lived in registers.  They live in an
LDS ring now.  This test encodes a 9 MB and a 64 MiB text image 30 times each WHILE another context runs forward BWTs back to
back on a second stream, and wants every output identical to the first, and the first identical to the oracle's (9 MB: the C
restatement, seconds) / the reference build's (64 MiB, when oracle/_ref is present).  -m gpu"""
import hashlib
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPS = 30


def _sha(t, n):
    return hashlib.sha256(t[:n].cpu().numpy().tobytes()).hexdigest()


def _sort_load(torch, jam, stop, err):
    """forward BWTs of a 32 MiB text block, back to back, on a context and stream of its own"""
    try:
        dev = torch.device("cuda", 0)
        s = torch.cuda.Stream(device=dev)
        ctx = jam.Context(0, s.cuda_stream)
        t = jam.corpus.make("text", 32 << 20, 77)
        with torch.cuda.stream(s):
            d_in = torch.from_numpy(t).to(dev)
            d_out = torch.empty(len(t) + 480, dtype=torch.uint8, device=dev)
        s.synchronize()
        first = None
        while not stop.is_set():
            ctx.bwt_forward(d_in, len(t), d_out, len(t) + 480)
            h = _sha(d_out, len(t) + 480)
            if first is None:
                first = h
            elif h != first:
                err.append("the co-running forward BWT changed its output")
                return
        ctx.close()
    except Exception as e:  # noqa: BLE001
        err.append(repr(e))


@pytest.mark.parametrize("nbytes", [9_000_000, 64 << 20])
def test_encode_is_stable_beside_a_running_suffix_sort(nbytes, oracle):
    import torch
    import jampack_amd as jam
    from oracle.pyoracle import Ref
    assert torch.cuda.is_available()
    dev = torch.device("cuda", 0)
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    t = jam.corpus.make("text", nbytes, 8)
    n = len(t)
    d_in = torch.from_numpy(t).to(dev)
    d_bwt = torch.empty(n + 480, dtype=torch.uint8, device=dev)
    assert ctx.bwt_forward(d_in, n, d_bwt, n + 480) == n + 480
    image = d_bwt.cpu().numpy()
    cap = jam.ans_capacity(n + 480)
    d_enc = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_img = torch.empty(n + 480, dtype=torch.uint8, device=dev)

    stop, err = threading.Event(), []
    th = threading.Thread(target=_sort_load, args=(torch, jam, stop, err))
    th.start()
    try:
        shas, lens = [], []
        for _ in range(REPS):
            d_img.copy_(d_bwt)                       # Ans::Encode may scribble on its input (ans.cpp:113): a fresh image every time
            clen = ctx.ans_encode(d_img, n + 480, d_enc, cap)
            lens.append(clen)
            shas.append(_sha(d_enc, clen))
    finally:
        stop.set()
        th.join()
    assert not err, err
    assert len(set(lens)) == 1 and len(set(shas)) == 1, f"{len(set(shas))} different outputs in {REPS} encodes of the same image"
    if nbytes <= 16 << 20:
        want = oracle.ans_encode(image)
        assert lens[0] == len(want) and shas[0] == hashlib.sha256(want.tobytes()).hexdigest()
    elif Ref.available():
        want = Ref().ans_encode(image)
        assert lens[0] == len(want) and shas[0] == hashlib.sha256(want.tobytes()).hexdigest()
    ctx.close()
