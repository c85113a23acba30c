"""The filter choice of the stock-CLI writer on the device: k_enc_filters through jpk_dev_blocks_filters_encode against the host form of
prestage.cpp, byte for byte, on guarded buffers at odd addresses; the stage chain and whole archives with JPK_CLI_FILTERS (alone and with
the dedupe) through this library's decoders -- k_pre_filters then sees type 2 and the widths 3, 4 and 12 from this writer -- and the
unmodified reference program `jampack d`; and what the option is for: smaller archives of sampled and record-shaped data.  -m gpu"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from filter_cases import FBS, MiB, headers, rec, rgb, stereo16, structs12
from stage_guard import SENT, Guarded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "jampack_ref")
OK, E_CAPACITY = 0, -2
GUARD = 4096
LEADS = (1, 3, 7)


@pytest.fixture(scope="module")
def gpu():
    import torch
    import jampack_amd as jam
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    yield torch, jam, ctx
    ctx.close()


def _blocks(jam):
    """(name, S1 bytes): the lengths around the piece edges, of mixed kinds, and one 1 MiB block of 16 pieces"""
    c = jam.corpus
    return [("one", np.array([200], np.uint8)), ("two", np.array([4, 128], np.uint8)), ("rec3/33", rec(33, 3, 1)), ("rec7/65535", rec(65_535, 7, 2)),
            ("text/65536", c.make("text", FBS, 3)), ("rec29/65537", rec(65_537, 29, 4)),
            ("rgb|random|rec32/131079", np.concatenate([rgb(FBS, 5), c.make("random", FBS, 6), rec(7, 32, 7)])), ("stereo16/1MiB", stereo16(MiB))]


def test_filters_encode_device_equals_host(gpu):
    torch, jam, ctx = gpu
    blocks = _blocks(jam)
    exp = [jam.Filters().Encode(x) for _, x in blocks]
    short = 3                                                          # this block gets one byte less than it needs
    caps = [len(e) - (1 if i == short else 0) for i, e in enumerate(exp)]
    ins = [Guarded(torch, x, LEADS[i % 3]) for i, (_, x) in enumerate(blocks)]
    outs = [Guarded(torch, None, LEADS[(i + 1) % 3], cap=c) for i, c in enumerate(caps)]
    d_in, d_out, lens = [g.ptr for g in ins], [g.ptr for g in outs], [len(x) for _, x in blocks]
    out_len, st = ctx.blocks_filters_encode(d_in, lens, d_out, caps)
    kinds = set()
    for i, (name, x) in enumerate(blocks):
        if i == short:
            assert (st[i], out_len[i]) == (E_CAPACITY, 0), name
            outs[i].check_output(np.zeros(0, dtype=np.uint8), used=0, what=name)       # nothing of it was written
        else:
            assert (st[i], out_len[i]) == (OK, len(exp[i])), name
            outs[i].check_output(exp[i], used=len(exp[i]), what=name)
            kinds.update(headers(exp[i], len(x)))
        ins[i].check_unchanged(name)
    assert (0, 0) in kinds and {t for t, w in kinds if w} == {0, 2} and {3, 4, 29} <= {w for _, w in kinds}, kinds   # not a comparison of stored pieces
    k = len(blocks)
    P, I = C.c_void_p * k, C.c_int32 * k
    ol = I()
    assert jam.lib().jpk_dev_blocks_filters_encode(ctx._h, k, P(*d_in), I(*lens), P(*d_out), I(*caps), ol, None) == E_CAPACITY
    assert list(ol)[short] == 0 and list(ol)[0] == len(exp[0])
    # and back through the device decoder: the first type-2 pieces and these widths k_pre_filters gets from this writer
    back = [Guarded(torch, None, LEADS[(i + 2) % 3], cap=len(x)) for i, (_, x) in enumerate(blocks)]
    outs[short] = Guarded(torch, exp[short], 5)
    bl, bs = ctx.blocks_filters_decode([g.ptr for g in outs], [len(e) for e in exp], [g.ptr for g in back], lens)
    for i, (name, x) in enumerate(blocks):
        assert (bs[i], bl[i]) == (OK, len(x)), name
        back[i].check_output(x, used=len(x), what=name)


def _copy_and_rgb(jam):
    x = np.concatenate([rgb(200_000, 3), jam.corpus.make("text", 70_000, 4), stereo16(131_072)])
    x[150_000: 154_096] = x[1000: 5096]                                # a 4 KiB copy inside the rgb data
    return x


@pytest.mark.parametrize("dedupe", [False, True])
def test_cli_stages_encode_with_filters_device_equals_host(gpu, dedupe):
    torch, jam, ctx = gpu
    c = jam.corpus
    pick = [("copy|rgb", _copy_and_rgb(jam)), ("empty", np.zeros(0, np.uint8)), ("one", np.array([9], np.uint8)), ("text", c.make("text", 100_001, 5)),
            ("rec12/65534", rec(65_534, 12, 6)), ("structs12", structs12(140_000, 7)), ("zero", np.zeros(70_000, np.uint8))]
    exp = [jam.cli_stages_encode(r, dedupe=dedupe, filters=True) for _, r in pick]
    assert any(not np.array_equal(e, jam.cli_stages_encode(r, dedupe=dedupe)) for e, (_, r) in zip(exp, pick))
    if dedupe:
        assert len(exp[0]) < len(jam.cli_stages_encode(pick[0][1], filters=True)) - 3000     # the copy left, and what remained was filtered
    short = 4
    caps = [len(e) - (1 if i == short else 0) for i, e in enumerate(exp)]
    ins = [Guarded(torch, r, LEADS[i % 3]) for i, (_, r) in enumerate(pick)]
    outs = [Guarded(torch, None, LEADS[(i + 2) % 3], cap=cp) for i, cp in enumerate(caps)]
    d_in, d_out, lens = [g.ptr for g in ins], [g.ptr for g in outs], [len(r) for _, r in pick]
    out_len, st = ctx.blocks_cli_stages_encode(d_in, lens, d_out, caps, dedupe=dedupe, filters=True)
    for i, (name, r) in enumerate(pick):
        what = f"{name} dedupe={dedupe}"
        if i == short:
            assert (st[i], out_len[i]) == (E_CAPACITY, 0), what
            outs[i].check_output(np.zeros(0, dtype=np.uint8), used=0, what=what)
        else:
            assert (st[i], out_len[i]) == (OK, len(exp[i])), what
            outs[i].check_output(exp[i], used=len(exp[i]), what=what)
        ins[i].check_unchanged(what)


# ---- archives --------------------------------------------------------------------------------------------------------------------
def _dev_compress(gpu, data, bs, flags, lead=0):
    torch, jam, ctx = gpu
    cap = jam.jam_cli_compress_bound(len(data), bs)
    d_in = torch.zeros(len(data) + 16, dtype=torch.uint8, device="cuda")
    d_in[lead: lead + len(data)] = torch.from_numpy(data).to("cuda")
    d_out = torch.full((cap + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    n = C.c_int64(-1)
    rc = jam.lib().jpk_dev_jam_cli_compress_ex(ctx._h, d_in.data_ptr() + lead, len(data), bs, d_out.data_ptr(), cap, C.byref(n), 0, flags)
    img = d_out.cpu().numpy()
    assert rc == OK and (img[cap:] == SENT).all()
    return img[: n.value].copy()


@pytest.fixture(scope="module")
def mixed_archive(gpu):
    """stereo16, text, rgb and a short last frame of structs12: 3.3 MiB in frames of 1 MiB, written on the device with JPK_CLI_FILTERS"""
    _, jam, _ = gpu
    data = np.concatenate([stereo16(MiB), jam.corpus.make("text", MiB, 21), rgb(MiB, 1), structs12(300_000, 1)])
    return data, _dev_compress(gpu, data, MiB, 4, lead=3)


def test_archive_forms_agree_and_decode(gpu, mixed_archive):
    torch, jam, ctx = gpu
    data, arch = mixed_archive
    assert np.array_equal(jam.jam_cli_compress(data, MiB, filters=True), arch), "host-buffer form"
    frames = [jam.jam_cli_block_write(data[o: o + MiB], MiB, filters=True) for o in range(0, len(data), MiB)]
    assert np.array_equal(np.concatenate(frames), arch), "frame by frame"
    d_in = torch.from_numpy(data).to("cuda")
    bound = jam.jam_cli_compress_bound(len(data), MiB)
    d_out = torch.empty(bound, dtype=torch.uint8, device="cuda")
    m = ctx.jam_cli_compress(d_in, len(data), MiB, d_out, bound, filters=True)
    assert np.array_equal(d_out[:m].cpu().numpy(), arch), "Context.jam_cli_compress"
    assert np.array_equal(jam.jam_cli_decompress_all(arch), data)
    assert np.array_equal(jam.jam_cli_decompress(arch), data)
    plain = _dev_compress(gpu, data, MiB, 0, lead=3)
    assert np.array_equal(plain, jam.jam_cli_compress(data, MiB)), "flags = 0 is the existing writer"
    both = _dev_compress(gpu, data, MiB, 5, lead=3)
    assert np.array_equal(both, jam.jam_cli_compress(data, MiB, dedupe=True, filters=True))
    assert np.array_equal(jam.jam_cli_decompress_all(both), data)
    print(f"archive: {len(plain)} bytes stored, {len(arch)} filtered, {len(both)} with the dedupe as well")
    assert len(arch) < 0.7 * len(plain)


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
def test_stock_cli_decodes_the_archive(gpu, mixed_archive, tmp_path, flags):
    data, arch = mixed_archive
    _ref_decodes(tmp_path, arch, data, flags)


# the bars are the CPU test's (test_filters_encode_host.py: 0.475 and 0.359 measured behind the oracle's block compressor); Lpx::Encode is
# now in the chain, and the margin covers it
@pytest.mark.parametrize("name,bar", [("stereo16", 0.60), ("rgb", 0.50)])
def test_filtered_archives_are_smaller(gpu, name, bar):
    data = stereo16(MiB) if name == "stereo16" else rgb(MiB, 1)
    a, b = _dev_compress(gpu, data, MiB, 4), _dev_compress(gpu, data, MiB, 0)
    print(f"{name}: {len(b)} bytes stored, {len(a)} filtered, ratio {len(a) / len(b):.3f}")
    assert len(a) <= bar * len(b), (name, len(a), len(b))


def test_text_archive_does_not_change(gpu):
    _, jam, _ = gpu
    data = jam.corpus.make("text", MiB, 3)
    assert np.array_equal(_dev_compress(gpu, data, MiB, 4), _dev_compress(gpu, data, MiB, 0))
