"""One staged frame through jpk_jam_staged_block_write / _read (the entries stage through the GPU): its header, the stored S2, the
reference's stage decoders, the read.  Archives of staged frames on the device: jpk_dev_jam_staged_compress against the concatenation of
jpk_jam_staged_block_write, the host form against the device form, the round trip through jpk_dev_jam_staged_decompress and through the reference's stage decoders,
archives that mix plain and staged frames, their capacity and corruption answers, the sort rounds the dedupe saves, and the pass
edge: a long archive, and what the plain, the staged and the stock-CLI entries answer when the capacity runs out behind it.  -m gpu"""
import ctypes as C
import struct

import numpy as np
import pytest

import dedupe_cases
import filter_cases
import jam_staged_cases
from jam_staged_cases import FLAGS, MiB, STAGED, header, s2_stored

pytestmark = pytest.mark.gpu

KiB = 1 << 10
OK, E_CAPACITY, E_CORRUPT = 0, -2, -3
SENT = 0xA5


@pytest.fixture(scope="module")
def gpu():
    import torch
    import jampack_amd as jam
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    yield torch, jam, ctx
    ctx.close()


# ---- one frame ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs():
    return jam_staged_cases.inputs()


@pytest.fixture(scope="module")
def frames(gpu, inputs):
    """(name, flags) -> the frame jpk_jam_staged_block_write makes of the input at 1 MiB BlockSize"""
    _, jam, _ = gpu
    return {(name, fl): jam.jam_staged_block_write(t, MiB, flags=fl) for name, t in inputs.items() for fl in FLAGS}


def test_one_frame_header_and_stored_streams(gpu, inputs, frames):
    _, jam, _ = gpu
    s2_len = {}
    for (name, fl), f in frames.items():
        t = inputs[name]
        magic, crc, psize, field = header(f)
        assert magic == b"JAM" and crc == jam.checksum_host(t) and psize == len(f) - 15 and field == MiB | STAGED, (name, fl)
        assert len(f) <= jam.jam_staged_compress_bound(len(t), MiB) or len(t) == 0, (name, fl)
        # the flags decide what is stored: without them S2 is the stored form, byte for byte
        s2 = jam.block_decompress(f[15:], jam.cli_stages_bound(len(t)))
        s2_len[name, fl] = len(s2)
        if fl == 0:
            assert np.array_equal(s2, s2_stored(t)), name
        if not fl & 1:
            assert len(s2) == jam.cli_stages_bound(len(t)) - 2, (name, fl)
    # the dedupe took the repeats out of what the BWT sees (x x x x: three of four), the filter choice found the channels
    assert s2_len["xxxx", 1] < s2_len["xxxx", 0] // 3 and s2_len["xxxx", 5] == s2_len["xxxx", 1]
    assert len(frames["stereo16", 4]) < 0.8 * len(frames["stereo16", 0])


def test_one_frame_reads_back(gpu, inputs, frames):
    """jpk_jam_staged_block_read: the frame alone, with bytes behind it, at exactly the raw size, one byte short, and without bit 30"""
    _, jam, _ = gpu
    for (name, fl), f in frames.items():
        t = inputs[name]
        back, used = jam.jam_staged_block_read(f, max(len(t), 1))
        assert used == len(f) and np.array_equal(back, t), (name, fl)
    f, t = frames["xyx/70000/1000", 5], inputs["xyx/70000/1000"]
    back, used = jam.jam_staged_block_read(np.concatenate([f, f[:40]]), MiB)
    assert used == len(f) and np.array_equal(back, t)
    lib, out, n, used = jam.lib(), np.full(len(t) + 64, SENT, dtype=np.uint8), C.c_int32(0), C.c_int32(0)
    assert lib.jpk_jam_staged_block_read(f.ctypes.data, len(f), out.ctypes.data, len(t) - 1, C.byref(n), C.byref(used)) != OK
    assert (out[len(t) - 1:] == SENT).all()
    g = f.copy()
    g[14] &= 0xBF
    assert lib.jpk_jam_staged_block_read(g.ctypes.data, len(g), out.ctypes.data, len(t), C.byref(n), C.byref(used)) == E_CORRUPT


def test_one_frame_decodes_with_the_reference_stage_decoders(ref, inputs, frames):
    cap = int(MiB * 1.05) + 4096
    for (name, fl), f in frames.items():
        t = inputs[name]
        s1 = ref.filters_decode(ref.decompress_block(f[15:], cap), cap)
        assert np.array_equal(ref.lz77_decompress(s1, max(len(t), 1)), t), (name, fl)


# ---- archives ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data(gpu):
    """2.3 MiB: three frames of 1 MiB BlockSize, the last one short -- repeats for the dedupe, channels for the filter choice"""
    _, jam, _ = gpu
    d = dedupe_cases.cases()
    t = np.concatenate([d["xyx/70000/1000"], filter_cases.stereo16(300_000), d["text"], d["abab"], filter_cases.rec(200_003, 7), d["xxxx"],
                        jam.corpus.make("text", 3 * MiB // 2, 3)])[: 2 * MiB + 300_001]
    assert len(t) == 2 * MiB + 300_001
    return t


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _compress(gpu, t, fl, bs=MiB):
    torch, jam, ctx = gpu
    bound = jam.jam_staged_compress_bound(len(t), bs)
    d_out = torch.full((bound + 64,), SENT, dtype=torch.uint8, device="cuda")
    m = ctx.jam_staged_compress(_dev(torch, t), len(t), bs, d_out, bound, flags=fl)
    img = d_out.cpu().numpy()
    assert (img[m:] == SENT).all()
    return img[:m].copy()


@pytest.fixture(scope="module")
def archives(gpu, data):
    return {fl: _compress(gpu, data, fl) for fl in FLAGS}


def _decode(gpu, arch, cap, check=True):
    """(output buffer image, result of Context.jam_staged_decompress)"""
    torch, jam, ctx = gpu
    d_out = torch.full((cap + 64,), SENT, dtype=torch.uint8, device="cuda")
    res = ctx.jam_staged_decompress(_dev(torch, arch), len(arch), d_out, cap, check=check)
    return d_out.cpu().numpy(), res


@pytest.mark.parametrize("fl", FLAGS)
def test_device_archive_is_the_concatenation_of_block_write(gpu, data, archives, fl):
    _, jam, _ = gpu
    want = np.concatenate([jam.jam_staged_block_write(data[o: o + MiB], MiB, flags=fl) for o in range(0, len(data), MiB)])
    assert np.array_equal(archives[fl], want)
    assert np.array_equal(jam.jam_staged_compress(data, MiB, flags=fl), want)           # the host form
    assert len(want) <= jam.jam_staged_compress_bound(len(data), MiB)
    assert jam.jam_staged_frames(want) == (3, 3 * MiB, -1)
    for o in (11, ):
        assert struct.unpack("<i", bytes(want[o: o + 4]))[0] == MiB | STAGED


@pytest.mark.parametrize("fl", FLAGS)
def test_round_trip_on_the_device_and_the_host(gpu, data, archives, fl):
    _, jam, _ = gpu
    img, res = _decode(gpu, archives[fl], 3 * MiB)
    assert res == (len(data), 3, -1)
    assert np.array_equal(img[: len(data)], data) and (img[len(data):] == SENT).all()
    assert np.array_equal(jam.jam_staged_decompress(archives[fl]), data)
    # exactly the raw size is enough, too
    img, res = _decode(gpu, archives[fl], len(data))
    assert res == (len(data), 3, -1) and np.array_equal(img[: len(data)], data) and (img[len(data):] == SENT).all()


def test_the_flags_do_their_work(archives):
    assert len(archives[1]) < len(archives[0]) and len(archives[4]) < len(archives[0]) and len(archives[5]) < min(len(archives[1]), len(archives[4]))


@pytest.mark.parametrize("fl", FLAGS)
def test_reference_stage_decoders_read_every_frame(gpu, ref, data, archives, fl):
    a, o, k = archives[fl], 0, 0
    cap = int(MiB * 1.05) + 4096
    while o < len(a):
        psize = struct.unpack("<i", bytes(a[o + 7: o + 11]))[0]
        s2 = ref.decompress_block(a[o + 15: o + 15 + psize], cap)
        r = ref.lz77_decompress(ref.filters_decode(s2, cap), MiB)
        assert np.array_equal(r, data[k * MiB: (k + 1) * MiB]), (fl, k)
        o += 15 + psize
        k += 1
    assert k == 3


@pytest.fixture(scope="module")
def mixed(gpu, data):
    """plain | staged (flags 5, shorter than its BlockSize) | plain, and the raw bytes"""
    _, jam, _ = gpu
    parts = [data[:400_000], data[MiB: MiB + 700_001], data[500_000: 500_000 + 300_000]]
    frames = [jam.jam_block_write(parts[0], MiB), jam.jam_staged_block_write(parts[1], MiB, flags=5), jam.jam_block_write(parts[2], MiB)]
    return frames, parts


def test_mixed_archive_decodes(gpu, mixed):
    _, jam, _ = gpu
    frames, parts = mixed
    arch, raw = np.concatenate(frames), np.concatenate(parts)
    bound = 400_000 + MiB + 300_000
    assert jam.jam_staged_frames(arch) == (3, bound, -1)
    assert jam.jam_frames(arch)[2] == 1 and jam.jam_cli_frames(arch)[2] == 1          # the other walks stop at the staged frame
    img, res = _decode(gpu, arch, bound)
    assert res == (len(raw), 3, -1) and np.array_equal(img[: len(raw)], raw) and (img[len(raw):] == SENT).all()
    assert np.array_equal(jam.jam_staged_decompress(arch), raw)
    # staged | plain | staged, and one byte short of the raw size
    arch2 = np.concatenate([frames[1], frames[0], frames[1]])
    raw2 = np.concatenate([parts[1], parts[0], parts[1]])
    img, res = _decode(gpu, arch2, len(raw2))
    assert res == (len(raw2), 3, -1) and np.array_equal(img[: len(raw2)], raw2)
    img, res = _decode(gpu, arch2, len(raw2) - 1, check=False)
    assert res == (2 * MiB + 400_000, 0, -1, E_CAPACITY) and (img == SENT).all()
    img, res = _decode(gpu, arch, len(raw) - 1, check=False)
    assert res == (bound, 0, -1, E_CAPACITY) and (img == SENT).all()


def test_a_bad_frame_1_stops_the_call_behind_frame_0(gpu, mixed):
    frames, parts = mixed
    for name in ("payload", "crc", "bit 30"):
        f1 = frames[1].copy()
        if name == "payload":
            f1[15 + len(f1) // 2] ^= 0x10
        elif name == "crc":
            f1[4] ^= 1
        else:
            f1[14] &= 0xBF                                             # now a plain frame's header in front of a staged payload
        arch = np.concatenate([frames[0], f1, frames[2]])
        img, res = _decode(gpu, arch, 400_000 + MiB + 300_000, check=False)
        assert res == (400_000, 1, 1, E_CORRUPT), (name, res)
        assert np.array_equal(img[:400_000], parts[0]), name


def _bad_frame_2(frames, how):
    f2 = frames[2].copy()
    if how == "crc":
        f2[4] ^= 1
    else:
        f2[15 + len(f2) // 2] ^= 0x10
    return np.concatenate([frames[0], frames[1], f2])


@pytest.mark.parametrize("how", ("crc", "payload"))
def test_a_bad_plain_frame_2_stops_the_call_behind_the_staged_frame_1(gpu, mixed, how):
    """a plain frame fails behind a staged one of the same pass: the staged frame is delivered"""
    frames, parts = mixed
    img, res = _decode(gpu, _bad_frame_2(frames, how), 400_000 + MiB + 300_000, check=False)
    assert res == (400_000 + 700_001, 2, 2, E_CORRUPT), res
    assert np.array_equal(img[: 400_000 + 700_001], np.concatenate(parts[:2]))


def test_the_earlier_plain_failure_wins_over_the_staged_one(gpu, mixed):
    frames, _ = mixed
    f0, f1 = frames[0].copy(), frames[1].copy()
    f0[4] ^= 1
    f1[15 + len(f1) // 2] ^= 0x10
    _, res = _decode(gpu, np.concatenate([f0, f1, frames[2]]), 400_000 + MiB + 300_000, check=False)
    assert res == (0, 0, 0, E_CORRUPT), res


# ---- capacity behind the pass edge: 130 frames of 1 MiB BlockSize, 4096 raw bytes each --------------------------------------------
EDGE_FRAMES, EDGE_RAW, PASS_FRAMES = 130, 4096, 128


@pytest.fixture(scope="module")
def edge(gpu):
    """name -> archive of 130 frames (all plain, plain and staged in turn, all stock-CLI), and the raw bytes they share"""
    _, jam, _ = gpu
    text = jam.corpus.make("text", EDGE_FRAMES * EDGE_RAW, 1000)              # (one call: the generator's start-up is the slow part)
    texts = [text[k * EDGE_RAW: (k + 1) * EDGE_RAW] for k in range(EDGE_FRAMES)]
    assert len({t.tobytes() for t in texts}) == EDGE_FRAMES
    plain = [jam.jam_block_write(t, MiB) for t in texts]
    archives = {"plain": np.concatenate(plain),
                "mixed": np.concatenate([jam.jam_staged_block_write(texts[k], MiB, flags=0) if k & 1 else plain[k] for k in range(EDGE_FRAMES)]),
                "cli": np.concatenate([jam.jam_cli_block_write(t, MiB) for t in texts])}
    return archives, np.concatenate(texts)


def _edge_entry(gpu, entry):
    _, jam, ctx = gpu
    return {"plain": (ctx.jam_decompress, jam.lib().jpk_jam_decompress), "staged": (ctx.jam_staged_decompress, jam.lib().jpk_jam_staged_decompress),
            "cli": (ctx.jam_cli_decompress, jam.lib().jpk_jam_cli_decompress)}[entry]


def _edge_bound(gpu, entry, arch):
    """what the entry's host walk reports for the archive: the raw bytes, or the raw bound of the chained kinds"""
    _, jam, _ = gpu
    k, bound, bad = {"plain": jam.jam_frames, "staged": jam.jam_staged_frames, "cli": jam.jam_cli_frames}[entry](arch)
    assert (k, bad) == (EDGE_FRAMES, -1)
    return bound


def _edge_decode(gpu, entry, arch, cap):
    torch, _, _ = gpu
    d_out = torch.full((EDGE_FRAMES * EDGE_RAW + 64,), SENT, dtype=torch.uint8, device="cuda")
    res = _edge_entry(gpu, entry)[0](_dev(torch, arch), len(arch), d_out, cap, check=False)
    return d_out.cpu().numpy(), res


def _edge_decode_host(gpu, entry, arch, cap):
    """(rc, out_len, frames) of the host entry, called by ctypes"""
    out = np.full(EDGE_FRAMES * EDGE_RAW + 64, SENT, dtype=np.uint8)
    n, nf, bf = C.c_int64(0), C.c_int32(0), C.c_int32(-1)
    rc = _edge_entry(gpu, entry)[1](arch.ctypes.data, len(arch), out.ctypes.data, cap, C.byref(n), C.byref(nf), C.byref(bf))
    return out, (int(rc), n.value, nf.value)


def test_plain_entry_answers_capacity_before_it_touches_anything(gpu, edge):
    archives, raw = edge
    img, res = _edge_decode(gpu, "plain", archives["plain"], len(raw) - 1)
    assert res == (EDGE_FRAMES * EDGE_RAW, 0, -1, E_CAPACITY), res
    assert (img == SENT).all()
    _, res = _edge_decode_host(gpu, "plain", archives["plain"], len(raw) - 1)
    assert res == (E_CAPACITY, EDGE_FRAMES * EDGE_RAW, 0), res


@pytest.mark.parametrize("entry,name", (("staged", "mixed"), ("cli", "cli"), ("staged", "plain")))
def test_chained_entries_answer_capacity_per_pass(gpu, edge, entry, name):
    """one byte short: the first pass of 128 frames stays delivered, the second one is refused and nothing of it is written"""
    archives, raw = edge
    arch, done = archives[name], PASS_FRAMES * EDGE_RAW
    bound = _edge_bound(gpu, entry, arch)
    assert bound == {"mixed": 65 * EDGE_RAW + 65 * MiB, "cli": EDGE_FRAMES * MiB, "plain": EDGE_FRAMES * EDGE_RAW}[name]
    img, res = _edge_decode(gpu, entry, arch, len(raw) - 1)
    assert res == (bound, PASS_FRAMES, -1, E_CAPACITY), res
    assert np.array_equal(img[:done], raw[:done]) and (img[done:] == SENT).all()
    _, res = _edge_decode_host(gpu, entry, arch, len(raw) - 1)
    assert res == (E_CAPACITY, bound, PASS_FRAMES), res


@pytest.mark.parametrize("entry,name", (("plain", "plain"), ("staged", "mixed"), ("cli", "cli"), ("staged", "plain")))
def test_exact_capacity_decodes_across_the_pass_edge(gpu, edge, entry, name):
    archives, raw = edge
    img, res = _edge_decode(gpu, entry, archives[name], len(raw))
    assert res == (len(raw), EDGE_FRAMES, -1, OK), res
    assert np.array_equal(img[: len(raw)], raw) and (img[len(raw):] == SENT).all()
    out, res = _edge_decode_host(gpu, entry, archives[name], len(raw))
    assert res == (OK, len(raw), EDGE_FRAMES) and np.array_equal(out[: len(raw)], raw) and (out[len(raw):] == SENT).all()


@pytest.mark.parametrize("entry,name", (("staged", "mixed"), ("cli", "cli")))
def test_exact_capacity_index_across_the_pass_edge(gpu, edge, entry, name):
    torch, _, ctx = gpu
    archives, raw = edge
    arch = archives[name]
    d_out = torch.full((len(raw) + 64,), SENT, dtype=torch.uint8, device="cuda")
    fn = ctx.jam_staged_decompress_ix if entry == "staged" else ctx.jam_cli_decompress_ix
    n, nf, bf, ix = fn(_dev(torch, arch), len(arch), d_out, len(raw))
    assert (n, nf, bf) == (len(raw), EDGE_FRAMES, -1) and np.array_equal(d_out.cpu().numpy()[: len(raw)], raw)
    assert (ix.frames, ix.bad_frame, ix.raw_len, ix.archive_len) == (EDGE_FRAMES, -1, len(raw), len(arch))
    assert [ix.frame(k)[:2] for k in range(EDGE_FRAMES)] == [(k * EDGE_RAW, EDGE_RAW) for k in range(EDGE_FRAMES)]
    ix.close()


def test_fewer_sort_rounds(gpu):
    """T | T' of test_gpu_dedupe.py: the BWT of the staged frame with the dedupe sorts no 100 000-byte repeats, the plain block's does"""
    torch, jam, ctx = gpu
    t = jam.corpus.make("text", MiB, 61)
    t2 = t.copy()
    t2[::100_000] ^= 1
    block = np.concatenate([t, t2])
    frame = jam.jam_staged_block_write(block, 2 * MiB, flags=1)
    s2 = jam.block_decompress(frame[15:], jam.cli_stages_bound(len(block)))
    rounds = {}
    for name, x in (("plain", block), ("staged", s2)):
        cap = jam.ans_capacity(len(x) + 480)
        d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        m = ctx.block_compress(_dev(torch, x), len(x), d_out, cap)
        rounds[name] = ctx.stats().sa_rounds
        if name == "staged":
            assert np.array_equal(d_out[:m].cpu().numpy(), frame[15:])            # this IS the frame's payload
    print(f"sa_rounds: {rounds}")
    assert rounds["staged"] < rounds["plain"], rounds


def test_130_frames_cross_the_pass_edge(gpu):
    """a pass holds 128 frames: 130 frames of 1 MiB, one text tile with a per-frame perturbation and a 200 KiB copy inside"""
    torch, jam, ctx = gpu
    tile = jam.corpus.make("text", MiB, 46)
    tile[700_001: 700_001 + 200 * KiB] = tile[1234: 1234 + 200 * KiB]
    d_in = torch.from_numpy(tile).to("cuda").repeat(130)
    d_in.view(130, MiB)[:, ::4099] ^= torch.arange(130, dtype=torch.uint8, device="cuda")[:, None]
    n = 130 * MiB
    bound = jam.jam_staged_compress_bound(n, MiB)
    d_out = torch.empty(bound, dtype=torch.uint8, device="cuda")
    m = ctx.jam_staged_compress(d_in, n, MiB, d_out, bound, flags=1)
    d_back = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert ctx.jam_staged_decompress(d_out, m, d_back, n) == (n, 130, -1)
    assert torch.equal(d_back, d_in)
