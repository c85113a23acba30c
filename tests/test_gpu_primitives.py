"""GPU primitives behind the hot path (scan, radix sort, suffix array) through the C ABI probes.  -m gpu"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    from jampack_amd import Context
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    c = Context(0, torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("n", [1, 63, 64, 100, 4095, 4096, 4097, 70000, 1_000_003, 5_000_000])
def test_exclusive_scan(ctx, n):
    rng = np.random.default_rng(n)
    a = rng.integers(0, 1000, n, dtype=np.uint32)
    d = _dev(a.view(np.int32))
    tot = ctx.exclusive_scan_u32(d, n)
    got = d.cpu().numpy().view(np.uint32)
    exp = np.concatenate(([0], np.cumsum(a, dtype=np.uint64)[:-1])).astype(np.uint32)
    assert tot == int(a.sum(dtype=np.uint64) & 0xFFFFFFFF)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f"first mismatch at {bad[:5]}: got {got[bad[:5]]} exp {exp[bad[:5]]}"


@pytest.mark.parametrize("n,bits", [(1, 64), (100, 64), (4096, 64), (4097, 16), (100_000, 64), (1_000_000, 40), (3_000_001, 64)])
def test_radix_sort_pairs_is_stable_and_sorted(ctx, n, bits):
    rng = np.random.default_rng(n + bits)
    keys = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
    if bits < 64:
        keys &= np.uint64((1 << bits) - 1)
    keys[: n // 3] = keys[n // 2: n // 2 + n // 3]          # plenty of duplicates: stability matters
    vals = np.arange(n, dtype=np.uint32)
    dk, dv = _dev(keys.view(np.int64)), _dev(vals.view(np.int32))
    ctx.sort_pairs_u64(dk, dv, n, 0, bits)
    gk = dk.cpu().numpy().view(np.uint64)
    gv = dv.cpu().numpy().view(np.uint32)
    order = np.argsort(keys, kind="stable")
    bad = np.nonzero(gv != order.astype(np.uint32))[0]
    assert bad.size == 0, f"first mismatch at {bad[:5]}: got {gv[bad[:5]]} exp {order[bad[:5]]}"
    assert np.array_equal(gk, keys[order])


@pytest.mark.parametrize("n", [4095, 4096, 4097, 1_000_003])
def test_exclusive_scan_wraps_mod_2_32(ctx, n):
    """values from the whole 32-bit range: the running sum wraps many times; expected from a 64-bit cumsum reduced mod 2^32"""
    rng = np.random.default_rng(500 + n)
    a = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    d = _dev(a.view(np.int32))
    tot = ctx.exclusive_scan_u32(d, n)
    got = d.cpu().numpy().view(np.uint32)
    inc = np.cumsum(a, dtype=np.uint64)
    exp = (np.concatenate((np.zeros(1, np.uint64), inc[:-1])) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    assert tot == int(inc[-1] & np.uint64(0xFFFFFFFF))
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f"first mismatch at {bad[:5]}: got {got[bad[:5]]} exp {exp[bad[:5]]}"


def test_exclusive_scan_of_words_off_the_16_byte_boundary(ctx):
    """d_data 4 bytes behind an aligned address (uint32 needs no more than its own alignment; the kernels load uint4 from in + base),
    guards directly around the n words"""
    import torch
    from stage_guard import Guarded
    n = 3 * 4096 + 17                                          # whole tiles through the vector path and a ragged one
    rng = np.random.default_rng(77)
    a = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    g = Guarded(torch, a.astype("<u4"), 4)
    assert g.ptr % 16 == 4
    tot = ctx.exclusive_scan_u32(g.ptr, n)
    inc = np.cumsum(a, dtype=np.uint64)
    exp = (np.concatenate((np.zeros(1, np.uint64), inc[:-1])) & np.uint64(0xFFFFFFFF)).astype("<u4")
    assert tot == int(inc[-1] & np.uint64(0xFFFFFFFF))
    g.check_output(exp, what="exclusive_scan_u32 at +4")


# RS_TILE in radix.hip is 4096 pairs: one short of, exactly and one past a tile; one pair; many tiles with a ragged last one
@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, 100_003])
@pytest.mark.parametrize("bit_lo,bit_hi", [(0, 8), (3, 13), (8, 16), (5, 5), (1, 64), (56, 64), (17, 40), (60, 64)])
def test_radix_sort_pairs_on_a_bit_range(ctx, n, bit_lo, bit_hi):
    """keys drawn from all 64 bits: only the bits [bit_lo, bit_hi) may decide the order (a last pass that looks at a whole byte would sort
    on the bits above bit_hi too), the pairs move with all 64 key bits intact, (5, 5) is the empty range: the identity"""
    from stage_guard import bit_range_order
    rng = np.random.default_rng(1000 * bit_lo + bit_hi + n)
    keys = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    keys[: n // 3] = keys[n // 2: n // 2 + n // 3]          # whole-key duplicates on top of the ties inside the range: stability matters
    vals = np.arange(n, dtype=np.uint32)
    dk, dv = _dev(keys.view(np.int64)), _dev(vals.view(np.int32))
    ctx.sort_pairs_u64(dk, dv, n, bit_lo, bit_hi)
    gk = dk.cpu().numpy().view(np.uint64)
    gv = dv.cpu().numpy().view(np.uint32)
    order = bit_range_order(keys, bit_lo, bit_hi)
    bad = np.nonzero(gv != order.astype(np.uint32))[0]
    assert bad.size == 0, f"first mismatch at {bad[:5]}: got {gv[bad[:5]]} exp {order[bad[:5]]}"
    assert np.array_equal(gk, keys[order])


@pytest.mark.parametrize("kind", ["text", "two", "zero", "random", "repeat4k", "dna", "runs"])
@pytest.mark.parametrize("n", [1, 2, 7, 8, 100, 5000, 200_000])
def test_suffix_array_equals_oracle(ctx, oracle, kind, n):
    import torch
    from jampack_amd import corpus
    t = corpus.make(kind, n, 9)
    dt = _dev(t)
    dsa = torch.zeros(n, dtype=torch.int32, device="cuda")
    ctx.suffix_array(dt, n, dsa)
    got = dsa.cpu().numpy()
    exp = oracle.suffix_array(t)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f"{kind} n={n}: first mismatch at {bad[:5]}: got {got[bad[:5]]} exp {exp[bad[:5]]} rounds={ctx.stats().sa_rounds}"


def test_suffix_array_with_embedded_zero_bytes(ctx, oracle):
    import torch
    rng = np.random.default_rng(3)
    t = rng.integers(0, 2, 50_000, dtype=np.uint8)          # only 0x00 / 0x01: short suffixes tie on padded bytes
    t[-9:] = 0
    dt = _dev(t)
    dsa = torch.zeros(len(t), dtype=torch.int32, device="cuda")
    ctx.suffix_array(dt, len(t), dsa)
    assert np.array_equal(dsa.cpu().numpy(), oracle.suffix_array(t))


@pytest.mark.parametrize("onesweep", ["0", "1"])
def test_forward_bwt_with_either_radix_form(onesweep):
    """round 0's radix passes: the one-pass form (decoupled look-back; the default since the packed keys) and the two-pass form
    (JPK_ONESWEEP=0: histogram + scan + scatter per pass) give the reference's images, single blocks and grouped small blocks (eight
    passes).  The switch is read once per process, so each form runs in a child."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    body = (
        "import sys; sys.path.insert(0, %r)\n"
        "import numpy as np, torch, jampack_amd as jam\n"
        "from oracle.pyoracle import Oracle\n"
        "o = Oracle()\n"
        "for kind, n in (('text_survey', 1_000_000), ('zero', 300_000), ('random', 70_001), ('dna', 500_000), ('text', 4096 * 5 + 17), ('two', 4095), ('runs', 200_000)):\n"
        "    t = jam.corpus.make(kind, n, 9)\n"
        "    assert np.array_equal(jam.Bwt().ForwardBwt(t), o.bwt_forward(t)), (kind, n)\n"
        "dev = torch.device('cuda', 0); ctx = jam.Context(0, None)\n"
        "blocks = [jam.corpus.make(['text_survey', 'dna', 'zero', 'random', 'runs'][i %% 5], 50_000 + 33_333 * i, i) for i in range(12)]\n"
        "d_in = [torch.from_numpy(b).to(dev) for b in blocks]\n"
        "caps = [jam.ans_capacity(len(b) + jam.TRAILER) for b in blocks]\n"
        "d_out = [torch.empty(c, dtype=torch.uint8, device=dev) for c in caps]\n"
        "n, st = ctx.blocks_compress(d_in, [len(b) for b in blocks], d_out, caps, 2)\n"
        "assert st == [0] * 12\n"
        "for i, b in enumerate(blocks):\n"
        "    want = o.ans_encode(o.bwt_forward(b))\n"
        "    assert n[i] == len(want) and np.array_equal(d_out[i][: n[i]].cpu().numpy(), want), i\n"
        "print('radix form ok')\n") % root
    env = dict(os.environ, JPK_ONESWEEP=onesweep)
    r = subprocess.run([sys.executable, "-c", body], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "radix form ok" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])
