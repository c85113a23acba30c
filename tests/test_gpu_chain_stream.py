"""The rANS encode chain on a stream of the device's chain pool (chain_pool.hpp; ans_enc.hip encode_core, enc_single_group).

k_rans_lanes runs on a high-priority stream that the library owns and shares among contexts; the model pass in front of it and the
emit kernels behind it stay on the context's stream, and the host orders the two.  A chain that starts before its model pass has
finished, emit kernels that start before the chain has finished, a pool stream that does not come back after an error, or a pool
that is not rebuilt after jpk_shutdown all show up as wrong bytes or a failed call here.  JPK_CHAIN_STREAMS is read once per
process, so the settings 0 (no pool: the old path) and 1 (every context shares one stream) run in fresh child processes.  -m gpu"""
import hashlib
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
# 0 bytes; below the 120-byte trailer rule; one chunk; two full chunks and a 5-byte one
SINGLE = [("text", 0), ("text", 100), ("text", 300_000), ("text_survey", 2 * MiB + 5)]
GROUP = 8, 128 << 10                 # one group encode: eight 128 KiB blocks through blocks_compress


def _inputs(jam):
    single = [jam.corpus.make(k, n, 40 + i) for i, (k, n) in enumerate(SINGLE)]
    group = [jam.corpus.make("text", GROUP[1], 60 + i) for i in range(GROUP[0])]
    return single, group


def _dev_in(torch, t):
    dev = torch.device("cuda", 0)
    return torch.from_numpy(np.ascontiguousarray(t)).to(dev) if len(t) else torch.empty(1, dtype=torch.uint8, device=dev)


def _compress_one(torch, jam, ctx, t, cap=None):
    cap = cap if cap is not None else jam.ans_capacity(len(t) + jam.TRAILER)
    d_out = torch.empty(max(cap, 1), dtype=torch.uint8, device=torch.device("cuda", 0))
    n = ctx.block_compress(_dev_in(torch, t), len(t), d_out, cap)
    return d_out[:n].cpu().numpy()


def _run_cases(torch, jam):
    """every case of this file on one context: name -> compressed bytes"""
    single, group = _inputs(jam)
    ctx = jam.Context(0)
    out = {}
    for (kind, n), t in zip(SINGLE, single):
        out[f"{kind}:{n}"] = _compress_one(torch, jam, ctx, t)
    caps = [jam.ans_capacity(len(b) + jam.TRAILER) for b in group]
    d_in = [_dev_in(torch, b) for b in group]
    d_out = [torch.empty(c, dtype=torch.uint8, device=torch.device("cuda", 0)) for c in caps]
    n, st = ctx.blocks_compress(d_in, [len(b) for b in group], d_out, caps, 2)
    assert st == [0] * len(group), st
    for i in range(len(group)):
        out[f"group:{i}"] = d_out[i][: n[i]].cpu().numpy()
    ctx.close()
    return out


def _digests(outs):
    return {k: [len(v), hashlib.sha256(v.tobytes()).hexdigest()] for k, v in outs.items()}


def _run_sharing(torch, jam):
    """six host threads, a context each, the same three 3 MiB texts four times each: 72 outputs against one thread's three"""
    texts = [jam.corpus.make(k, 3 * MiB, 70 + i) for i, k in enumerate(("text", "text_survey", "dna"))]
    ctx = jam.Context(0)
    want = [_compress_one(torch, jam, ctx, t) for t in texts]
    ctx.close()
    bad, lock = [], threading.Lock()

    def work(tid):
        try:
            c = jam.Context(0)
            for rep in range(4):
                for i, t in enumerate(texts):
                    if not np.array_equal(_compress_one(torch, jam, c, t), want[i]):
                        with lock:
                            bad.append((tid, rep, i))
            c.close()
        except Exception as e:  # noqa: BLE001
            with lock:
                bad.append((tid, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(6)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    return bad


def child_main(sharing):
    """what a child process runs: the cases' digests (and the sharing run's verdict) as one JSON line"""
    import torch
    assert torch.cuda.is_available()
    import jampack_amd as jam
    res = {"digests": _digests(_run_cases(torch, jam))}
    if sharing:
        res["sharing_bad"] = _run_sharing(torch, jam)
    print("CHAIN_CHILD " + json.dumps(res))


def _child(chain_streams, sharing):
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; "
            f"import test_gpu_chain_stream as m; m.child_main({sharing!r})")
    env = dict(os.environ, JPK_CHAIN_STREAMS=str(chain_streams))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("CHAIN_CHILD ")]
    assert r.returncode == 0 and lines, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(lines[-1][len("CHAIN_CHILD "):])


@pytest.fixture(scope="module")
def here():
    """the cases in this process, with the pool as the library makes it by default"""
    import torch
    import jampack_amd as jam
    assert torch.cuda.is_available()
    assert "JPK_CHAIN_STREAMS" not in os.environ, "the in-process cases are meant to run with the default pool"
    return torch, jam, _run_cases(torch, jam)


def test_bytes_equal_the_oracle(here, oracle):
    torch, jam, outs = here
    single, group = _inputs(jam)
    named = [(f"{k}:{n}", t) for (k, n), t in zip(SINGLE, single)] + [(f"group:{i}", b) for i, b in enumerate(group)]
    for name, t in named:
        want = oracle.ans_encode(oracle.bwt_forward(t) if len(t) >= 120 else oracle.bwt_forward(t, prefill=0))
        got = outs[name]
        assert len(got) == len(want) and np.array_equal(got, want), f"{name}: {len(got)} vs {len(want)} bytes"


def test_no_pool_gives_the_same_bytes(here):
    """JPK_CHAIN_STREAMS=0: everything on the context's stream, the path before the pool"""
    assert _child(0, False)["digests"] == _digests(here[2])


def test_one_shared_stream_gives_the_same_bytes_and_six_threads_share_it(here):
    res = _child(1, True)
    assert res["digests"] == _digests(here[2])
    assert res["sharing_bad"] == [], res["sharing_bad"]


def test_capacity_error_gives_the_pool_stream_back(here, oracle):
    torch, jam, outs = here
    t = _inputs(jam)[0][2]
    want = outs["text:300000"]
    ctx = jam.Context(0)
    with pytest.raises(jam.JampackError) as e:
        _compress_one(torch, jam, ctx, t, cap=len(want) - 1)
    assert e.value.status == -2                                      # JPK_E_CAPACITY
    assert np.array_equal(_compress_one(torch, jam, ctx, t), want)
    ctx.close()


def test_context_on_a_torch_stream(here):
    torch, jam, outs = here
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    t = _inputs(jam)[0][3]
    with torch.cuda.stream(s):
        ctx = jam.Context(0, s.cuda_stream)
        got = _compress_one(torch, jam, ctx, t)
        ctx.close()
    s.synchronize()
    assert np.array_equal(got, outs[f"text_survey:{2 * MiB + 5}"])


def test_pool_is_rebuilt_after_shutdown(here):
    torch, jam, outs = here
    t = _inputs(jam)[0][2]
    want = outs["text:300000"]
    for _ in range(20):
        ctx = jam.Context(0)
        assert np.array_equal(_compress_one(torch, jam, ctx, t), want)
        ctx.close()
    jam.shutdown()
    ctx = jam.Context(0)
    assert np.array_equal(_compress_one(torch, jam, ctx, t), want)
    ctx.close()
