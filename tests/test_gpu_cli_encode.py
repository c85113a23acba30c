"""The writer of stock-CLI archives on the device: k_enc_lpx / k_enc_wrap through their batch entries against the host encoders of
prestage.cpp, byte for byte, and whole archives (jpk_dev_jam_cli_compress / jpk_jam_cli_compress / jpk_jam_cli_block_write) through
this library's decoders and -- the point of the feature -- through the unmodified reference program `jampack d`.  -m gpu

The batch entries run on guarded allocations (stage_guard.Guarded): the guards around every output hold their sentinel afterwards and
the inputs are unchanged."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from stage_guard import SENT, Guarded
from test_cli_encode_host import STAGE_NS, make

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "jampack_ref")
MiB = 1 << 20
OK, E_CAPACITY = 0, -2
GUARD = 4096
# parts at the 16 KiB tile edge - 1, + 0, + 1 (65 535 / 4 = 16 383, ...), five parts (65 543 = 4 * 16 385 + 3), a part longer than the ring
LPX_LENS = [0, 1, 3, 5, 65_535, 65_536, 65_537, 65_543, 327_685]
# repeat4k: stretches that cross tile edges; runs and tile300 are the inputs on which the model predicts (Lpx::Encode changes bytes)
LPX_KINDS = ["repeat4k", "text", "samples16", "zero", "random", "runs", "tile300"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    import jampack_amd as jam
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    yield torch, jam, ctx
    ctx.close()


@pytest.fixture(scope="module")
def lpx_cases(gpu):
    """[(name, input, jpk_lpx_encode(input))], computed once"""
    _, jam, _ = gpu
    out = []
    for kind in LPX_KINDS:
        for n in LPX_LENS:
            t = make(jam, kind, n, 81)
            out.append((f"{kind}/{n}", t, jam.Lpx().encode(t)))
    # the seams of the kernel's walk: parts of exactly one tile (16 KiB), one tile + 1, exactly the ring (80 KiB), the ring + 1
    for kind in ("zero", "repeat4k"):
        for n in (65_536, 65_540, 327_680, 327_684):
            t = make(jam, kind, n, 82)
            out.append((f"seam {kind}/{n}", t, jam.Lpx().encode(t)))
    return out


@pytest.mark.parametrize("odd", [False, True])
def test_lpx_encode_device_equals_host(gpu, lpx_cases, odd):
    torch, jam, ctx = gpu
    ins = [Guarded(torch, t, (3 * i + 1) % 16 if odd else 0) for i, (_, t, _) in enumerate(lpx_cases)]
    outs = [Guarded(torch, None, (5 * i + 3) % 16 if odd else 0, cap=len(t)) for i, (_, t, _) in enumerate(lpx_cases)]
    st = ctx.blocks_lpx_encode([g.ptr for g in ins], [len(t) for _, t, _ in lpx_cases], [g.ptr for g in outs])
    assert st == [OK] * len(lpx_cases)
    changed = 0
    for (name, t, exp), gi, go in zip(lpx_cases, ins, outs):
        go.check_output(exp, used=len(exp), what=f"lpx encode {name}")
        gi.check_unchanged(name)
        changed += int((exp != t).sum())
    assert changed > 100_000           # the comparison is not one of identities


@pytest.fixture(scope="module")
def stage_cases(gpu):
    """[(n, input, jpk_cli_stages_encode(input))], computed once"""
    _, jam, _ = gpu
    out = []
    for n in STAGE_NS:
        t = np.concatenate([make(jam, "tile300", n // 2, 82), jam.corpus.make("text", n - n // 2, 83)]) if n else np.zeros(0, dtype=np.uint8)
        out.append((n, t, jam.cli_stages_encode(t)))
    return out


def test_cli_stages_encode_device_equals_host(gpu, stage_cases):
    torch, jam, ctx = gpu
    short = 3                                                          # this block gets one byte less than it needs
    caps = [len(s4) - (1 if i == short else 0) for i, (_, _, s4) in enumerate(stage_cases)]
    ins = [Guarded(torch, t, (3 * i + 1) % 16) for i, (_, t, _) in enumerate(stage_cases)]
    outs = [Guarded(torch, None, (5 * i + 3) % 16, cap=c) for i, c in enumerate(caps)]
    d_in, d_out, lens = [g.ptr for g in ins], [g.ptr for g in outs], [n for n, _, _ in stage_cases]
    out_len, st = ctx.blocks_cli_stages_encode(d_in, lens, d_out, caps)
    for i, (n, t, s4) in enumerate(stage_cases):
        what = f"stages n={n}"
        if i == short:
            assert (st[i], out_len[i]) == (E_CAPACITY, 0), what
            outs[i].check_output(np.zeros(0, dtype=np.uint8), used=0, what=what)       # nothing of it was written
        else:
            assert (st[i], out_len[i]) == (OK, len(s4)), what
            assert out_len[i] == jam.cli_stages_bound(n)
            outs[i].check_output(s4, used=len(s4), what=what)
        ins[i].check_unchanged(what)
    # without a status array the call returns the first failing block's status
    k = len(stage_cases)
    P, I = C.c_void_p * k, C.c_int32 * k
    ol = I()
    assert jam.lib().jpk_dev_blocks_cli_stages_encode(ctx._h, k, P(*d_in), I(*lens), P(*d_out), I(*caps), ol, None) == E_CAPACITY
    assert list(ol)[short] == 0 and list(ol)[0] == len(stage_cases[0][2])


# ---- frames and archives ---------------------------------------------------------------------------------------------------------
def _mixed(n, seed):
    from jampack_amd import corpus
    parts = [corpus.make("text", n // 2, seed), corpus.make("samples16", n // 4, seed + 1), corpus.make("runs", n // 8, seed + 2)]
    parts.append(corpus.make("random", n - sum(len(p) for p in parts), seed + 3))
    return np.concatenate(parts)


def _dev_compress(gpu, data, bs, cap=None, lead=0):
    """jpk_dev_jam_cli_compress with `cap` bytes of output in front of a guard -> (archive or None, status, guard ok)"""
    torch, jam, ctx = gpu
    cap = jam.jam_cli_compress_bound(len(data), bs) if cap is None else cap
    d_in = torch.zeros(len(data) + 16, dtype=torch.uint8, device="cuda")
    if len(data):
        d_in[lead: lead + len(data)] = torch.from_numpy(data).to("cuda")
    d_out = torch.full((cap + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    n = C.c_int64(-1)
    rc = jam.lib().jpk_dev_jam_cli_compress(ctx._h, d_in.data_ptr() + lead, len(data), bs, d_out.data_ptr(), cap, C.byref(n), 0)
    img = d_out.cpu().numpy()
    return (img[: n.value].copy() if rc == OK else None), rc, bool((img[cap:] == SENT).all())


@pytest.fixture(scope="module")
def mixed(gpu):
    data = _mixed(3_300_000, 41)
    arch, rc, guard = _dev_compress(gpu, data, MiB, lead=5)
    assert rc == OK and guard
    return data, arch


def test_one_frame_round_trip(gpu):
    _, jam, _ = gpu
    for n in (0, 1, 70_001):
        t = _mixed(n, 43)
        f = jam.jam_cli_block_write(t, MiB)
        assert bytes(f[:3]) == b"JAM" and int(np.frombuffer(f[11:15].tobytes(), dtype="<i4")[0]) == MiB
        back, used = jam.jam_cli_block_read(f, MiB)
        assert used == len(f) and np.array_equal(back, t), n
        # the payload is block_compress of the host stage chain
        assert np.array_equal(f[15:], jam.block_compress(jam.cli_stages_encode(t))), n


def test_archive_decodes_to_its_input(gpu, mixed):
    torch, jam, ctx = gpu
    data, arch = mixed
    assert jam.jam_cli_frames(arch) == (4, 4 * MiB, -1)
    d_a = torch.from_numpy(arch).to("cuda")
    d_back = torch.empty(4 * MiB, dtype=torch.uint8, device="cuda")
    assert ctx.jam_cli_decompress(d_a, len(arch), d_back, 4 * MiB) == (len(data), 4, -1)        # the batched decoder
    assert np.array_equal(d_back[: len(data)].cpu().numpy(), data)
    assert np.array_equal(jam.jam_cli_decompress(arch), data)                                   # frame by frame, pre-stages on the host


def test_archive_bytes_are_those_of_the_other_forms(gpu, mixed):
    _, jam, _ = gpu
    data, arch = mixed
    assert np.array_equal(jam.jam_cli_compress(data, MiB), arch), "host form"
    frames = [jam.jam_cli_block_write(data[o: o + MiB], MiB) for o in range(0, len(data), MiB)]
    assert np.array_equal(np.concatenate(frames), arch), "frame by frame"
    o = 0
    for k, f in enumerate(frames):                                     # each header crc is the checksum of its raw slice
        crc = int(np.frombuffer(arch[o + 3: o + 7].tobytes(), dtype="<u4")[0])
        assert crc == jam.checksum_host(data[k * MiB: (k + 1) * MiB]), k
        o += len(f)
    assert o == len(arch)


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
def test_stock_cli_decodes_the_archive(gpu, mixed, tmp_path, flags):
    data, arch = mixed
    _ref_decodes(tmp_path, arch, data, flags)


@pytest.mark.parametrize("flags", [[], ["-T"]])
def test_stock_cli_decodes_a_short_frame_of_a_large_block_size(gpu, tmp_path, flags):
    """the decoder never sees -b: it sizes its buffers from the header's BlockSize"""
    data = _mixed(2 * MiB, 44)
    arch, rc, guard = _dev_compress(gpu, data, 16 * MiB)
    assert rc == OK and guard
    assert int(np.frombuffer(arch[11:15].tobytes(), dtype="<i4")[0]) == 16 * MiB
    _ref_decodes(tmp_path, arch, data, flags)


def test_empty_capacity_and_bound(gpu, mixed):
    _, jam, _ = gpu
    data, arch = mixed
    e = np.zeros(0, dtype=np.uint8)
    got, rc, guard = _dev_compress(gpu, e, MiB, cap=16)
    assert rc == OK and len(got) == 0 and guard
    assert len(jam.jam_cli_compress(e, MiB)) == 0
    got, rc, guard = _dev_compress(gpu, data, MiB, cap=len(arch))      # exact
    assert rc == OK and guard and np.array_equal(got, arch)
    _, rc, guard = _dev_compress(gpu, data, MiB, cap=len(arch) - 1)
    assert rc == E_CAPACITY and guard
    out = np.full(len(arch) + GUARD, SENT, dtype=np.uint8)
    n = C.c_int64(0)
    assert jam.lib().jpk_jam_cli_compress(data.ctypes.data, len(data), MiB, out.ctypes.data, len(arch) - 1, C.byref(n), 0) == E_CAPACITY
    assert (out[len(arch) - 1:] == SENT).all()
    rnd = jam.corpus.make("random", 2 * MiB + 77, 45)                  # incompressible: the bound still suffices
    got, rc, guard = _dev_compress(gpu, rnd, MiB)
    assert rc == OK and guard and len(got) > len(rnd)
    assert np.array_equal(jam.jam_cli_decompress_all(got), rnd)


def test_130_frames_cross_the_pass_edge(gpu):
    """a pass holds 128 frames: 130 frames of 1 MiB, one text tile with a per-frame perturbation"""
    torch, jam, ctx = gpu
    tile = torch.from_numpy(jam.corpus.make("text", MiB, 46)).to("cuda")
    d_in = tile.repeat(130)
    d_in.view(130, MiB)[:, ::4099] ^= torch.arange(130, dtype=torch.uint8, device="cuda")[:, None]
    n = 130 * MiB
    bound = jam.jam_cli_compress_bound(n, MiB)
    d_out = torch.empty(bound, dtype=torch.uint8, device="cuda")
    m = ctx.jam_cli_compress(d_in, n, MiB, d_out, bound)
    d_back = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert ctx.jam_cli_decompress(d_out, m, d_back, n) == (n, 130, -1)
    assert torch.equal(d_back, d_in)
