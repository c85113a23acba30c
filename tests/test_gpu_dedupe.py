"""The dedupe of the stock-CLI writer on the device: the k_dd_* kernels through jpk_dev_blocks_lz77_dedupe against the host form of
prestage.cpp, byte for byte, on guarded buffers at odd addresses; the stage chain and whole archives with JPK_CLI_DEDUPE through this
library's decoders and the unmodified reference program `jampack d`; and what the option is for -- fewer suffix-sort rounds.  -m gpu"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dedupe_cases import cases
from stage_guard import SENT, Guarded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "jampack_ref")
MiB = 1 << 20
KiB = 1 << 10
OK, E_CAPACITY = 0, -2
GUARD = 4096


@pytest.fixture(scope="module")
def gpu():
    import torch
    import jampack_amd as jam
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    yield torch, jam, ctx
    ctx.close()


@pytest.fixture(scope="module")
def host(gpu):
    """[(name, block, jpk_lz77_dedupe(block))], computed once"""
    _, jam, _ = gpu
    return [(name, r, jam.Lz77().dedupe(r)) for name, r in cases().items()]


def test_dedupe_device_equals_host(gpu, host):
    torch, jam, ctx = gpu
    names = [name for name, _, _ in host]
    short = names.index("xyx/4096/65")                                 # this block gets one byte less than it needs
    caps = [len(s1) - (1 if i == short else 0) for i, (_, _, s1) in enumerate(host)]
    ins = [Guarded(torch, r, (3 * i + 1) % 16) for i, (_, r, _) in enumerate(host)]
    outs = [Guarded(torch, None, (5 * i + 3) % 16, cap=c) for i, c in enumerate(caps)]
    d_in, d_out, lens = [g.ptr for g in ins], [g.ptr for g in outs], [len(r) for _, r, _ in host]
    out_len, st = ctx.blocks_lz77_dedupe(d_in, lens, d_out, caps)
    found = 0
    for i, (name, r, s1) in enumerate(host):
        if i == short:
            assert (st[i], out_len[i]) == (E_CAPACITY, 0), name
            outs[i].check_output(np.zeros(0, dtype=np.uint8), used=0, what=name)       # nothing of it was written
        else:
            assert (st[i], out_len[i]) == (OK, len(s1)), name
            outs[i].check_output(s1, used=len(s1), what=name)
            found += len(r) + 2 - len(s1)
        ins[i].check_unchanged(name)
    assert found > 4 * MiB                                             # the comparison is not one of stored forms
    k = len(host)
    P, I = C.c_void_p * k, C.c_int32 * k
    ol = I()
    assert jam.lib().jpk_dev_blocks_lz77_dedupe(ctx._h, k, P(*d_in), I(*lens), P(*d_out), I(*caps), ol, None) == E_CAPACITY
    assert list(ol)[short] == 0 and list(ol)[0] == len(host[0][2])


def test_cli_stages_encode_ex_device_equals_host(gpu, host):
    torch, jam, ctx = gpu
    pick = [h for h in host if h[0] in ("xyx/70000/65", "xxxx", "abab", "repeat4k", "tile300", "text", "n/0", "n/1", "lit/135", "zero")]
    for dedupe in (True, False):
        exp = [jam.cli_stages_encode(r, dedupe=dedupe) for _, r, _ in pick]
        short = 2
        caps = [len(e) - (1 if i == short else 0) for i, e in enumerate(exp)]
        ins = [Guarded(torch, r, (3 * i + 1) % 16) for i, (_, r, _) in enumerate(pick)]
        outs = [Guarded(torch, None, (5 * i + 3) % 16, cap=c) for i, c in enumerate(caps)]
        d_in, d_out, lens = [g.ptr for g in ins], [g.ptr for g in outs], [len(r) for _, r, _ in pick]
        out_len, st = ctx.blocks_cli_stages_encode(d_in, lens, d_out, caps, dedupe=dedupe)
        for i, (name, r, _) in enumerate(pick):
            what = f"{name} dedupe={dedupe}"
            if i == short:
                assert (st[i], out_len[i]) == (E_CAPACITY, 0), what
                outs[i].check_output(np.zeros(0, dtype=np.uint8), used=0, what=what)
            else:
                assert (st[i], out_len[i]) == (OK, len(exp[i])), what
                outs[i].check_output(exp[i], used=len(exp[i]), what=what)
            ins[i].check_unchanged(what)
        if not dedupe:                                                 # flags = 0 is the existing entry
            outs2 = [Guarded(torch, None, (5 * i + 3) % 16, cap=c) for i, c in enumerate(caps)]
            k = len(pick)
            P, I = C.c_void_p * k, C.c_int32 * k
            ol, sl = I(), I()
            assert jam.lib().jpk_dev_blocks_cli_stages_encode(ctx._h, k, P(*d_in), I(*lens), P(*[g.ptr for g in outs2]), I(*caps), ol, sl) == OK
            assert list(ol) == out_len and list(sl) == st
            for a, b in zip(outs, outs2):
                assert np.array_equal(a.host()[a.off: a.off + a.cap], b.host()[b.off: b.off + b.cap])


# ---- archives --------------------------------------------------------------------------------------------------------------------
def _dup_data(jam, n=3_300_000, seed=51):
    """every 1 MiB block holds one 300 KiB stretch twice (at an odd distance); the last block is short"""
    data = jam.corpus.make("text", n, seed)
    for o in range(0, n, MiB):
        if o + 300 * KiB + 333_333 + 300 * KiB <= n:
            data[o + 333_333 + 300 * KiB: o + 333_333 + 600 * KiB] = data[o + 1000: o + 1000 + 300 * KiB]
        else:
            data[o + 40_001: o + 40_001 + 100 * KiB] = data[o + 5: o + 5 + 100 * KiB]
    return data


def _dev_compress(gpu, data, bs, cap=None, lead=0, dedupe=True):
    torch, jam, ctx = gpu
    cap = jam.jam_cli_compress_bound(len(data), bs) if cap is None else cap
    d_in = torch.zeros(len(data) + 16, dtype=torch.uint8, device="cuda")
    d_in[lead: lead + len(data)] = torch.from_numpy(data).to("cuda")
    d_out = torch.full((cap + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    n = C.c_int64(-1)
    rc = jam.lib().jpk_dev_jam_cli_compress_ex(ctx._h, d_in.data_ptr() + lead, len(data), bs, d_out.data_ptr(), cap, C.byref(n), 0, 1 if dedupe else 0)
    img = d_out.cpu().numpy()
    return (img[: n.value].copy() if rc == OK else None), rc, bool((img[cap:] == SENT).all())


@pytest.fixture(scope="module")
def dup(gpu):
    _, jam, _ = gpu
    data = _dup_data(jam)
    arch, rc, guard = _dev_compress(gpu, data, MiB, lead=5)
    assert rc == OK and guard
    return data, arch


def test_archive_forms_agree_decode_and_shrink(gpu, dup):
    torch, jam, ctx = gpu
    data, arch = dup
    assert np.array_equal(jam.jam_cli_compress(data, MiB, dedupe=True), arch), "host form"
    frames = [jam.jam_cli_block_write(data[o: o + MiB], MiB, dedupe=True) for o in range(0, len(data), MiB)]
    assert np.array_equal(np.concatenate(frames), arch), "frame by frame"
    assert np.array_equal(jam.jam_cli_decompress(arch), data)
    assert np.array_equal(jam.jam_cli_decompress_all(arch), data)
    d_a = torch.from_numpy(arch).to("cuda")
    d_back = torch.empty(4 * MiB, dtype=torch.uint8, device="cuda")
    assert ctx.jam_cli_decompress(d_a, len(arch), d_back, 4 * MiB) == (len(data), 4, -1)
    assert np.array_equal(d_back[: len(data)].cpu().numpy(), data)
    plain, rc, guard = _dev_compress(gpu, data, MiB, lead=5, dedupe=False)
    assert rc == OK and guard
    assert np.array_equal(plain, jam.jam_cli_compress(data, MiB)), "flags = 0 is the existing writer"
    print(f"archive: {len(plain)} bytes without the dedupe, {len(arch)} with it")
    assert len(arch) < len(plain)


def test_archive_capacity_and_random(gpu, dup):
    _, jam, _ = gpu
    data, arch = dup
    got, rc, guard = _dev_compress(gpu, data, MiB, cap=len(arch))      # exact
    assert rc == OK and guard and np.array_equal(got, arch)
    _, rc, guard = _dev_compress(gpu, data, MiB, cap=len(arch) - 1)
    assert rc == E_CAPACITY and guard
    rnd = jam.corpus.make("random", 2 * MiB + 77, 45)
    a, rc, guard = _dev_compress(gpu, rnd, MiB)
    b, rc2, guard2 = _dev_compress(gpu, rnd, MiB, dedupe=False)
    assert rc == rc2 == OK and guard and guard2 and np.array_equal(a, b)               # nothing to find: not one byte changes


def _ref_decodes(tmp_path, arch, data, flags):
    if not os.path.exists(REF_CLI):
        pytest.skip(f"{os.path.relpath(REF_CLI, ROOT)} not built (reference tree was absent at build time)")
    src, dst = tmp_path / "a.jam", tmp_path / "back.bin"
    arch.tofile(src)
    cmd = [REF_CLI, "d", str(src), str(dst)] + flags
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"{' '.join(cmd)} -> {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    assert np.array_equal(np.fromfile(dst, dtype=np.uint8), data), "the stock CLI decoded other bytes"


@pytest.mark.parametrize("flags", [[], ["-T"]])
def test_stock_cli_decodes_the_archive(gpu, dup, tmp_path, flags):
    data, arch = dup
    _ref_decodes(tmp_path, arch, data, flags)


@pytest.mark.parametrize("flags", [[], ["-T"]])
def test_stock_cli_decodes_a_short_frame_of_a_large_block_size(gpu, tmp_path, flags):
    _, jam, _ = gpu
    data = _dup_data(jam, 2 * MiB, 52)
    data[MiB + 7: 2 * MiB] = data[3: MiB - 4]                          # and one copy that is most of a MiB long
    arch, rc, guard = _dev_compress(gpu, data, 16 * MiB)
    assert rc == OK and guard
    assert int(np.frombuffer(arch[11:15].tobytes(), dtype="<i4")[0]) == 16 * MiB
    _ref_decodes(tmp_path, arch, data, flags)


def test_fewer_sort_rounds(gpu):
    """T | T' with T' = T but for one byte in 100 000: the BWT of the stored chain sorts 100 000-byte repeats, the dedupe's does not"""
    torch, jam, ctx = gpu
    t = jam.corpus.make("text", MiB, 61)
    t2 = t.copy()
    t2[::100_000] ^= 1
    rounds = {}
    for name, block, dedupe in (("stored", np.concatenate([t, t2]), False), ("dedupe", np.concatenate([t, t2]), True), ("alone", t, False)):
        s4 = jam.cli_stages_encode(block, dedupe=dedupe)
        d_in = torch.from_numpy(s4).to("cuda")
        cap = jam.ans_capacity(len(s4) + 480)
        d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        ctx.block_compress(d_in, len(s4), d_out, cap)
        rounds[name] = ctx.stats().sa_rounds
    print(f"sa_rounds: {rounds}")
    assert rounds["dedupe"] < rounds["stored"], rounds
    assert rounds["dedupe"] <= rounds["alone"] + 1, rounds


def test_130_frames_cross_the_pass_edge(gpu):
    """a pass holds 128 frames: 130 frames of 1 MiB, one text tile with a per-frame perturbation and a 200 KiB copy inside"""
    torch, jam, ctx = gpu
    tile = jam.corpus.make("text", MiB, 46)
    tile[700_001: 700_001 + 200 * KiB] = tile[1234: 1234 + 200 * KiB]
    d_in = torch.from_numpy(tile).to("cuda").repeat(130)
    d_in.view(130, MiB)[:, ::4099] ^= torch.arange(130, dtype=torch.uint8, device="cuda")[:, None]
    n = 130 * MiB
    bound = jam.jam_cli_compress_bound(n, MiB)
    d_out = torch.empty(bound, dtype=torch.uint8, device="cuda")
    m = ctx.jam_cli_compress(d_in, n, MiB, d_out, bound, dedupe=True)
    d_back = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert ctx.jam_cli_decompress(d_out, m, d_back, n) == (n, 130, -1)
    assert torch.equal(d_back, d_in)
