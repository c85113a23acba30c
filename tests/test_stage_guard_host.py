"""The guard checker and the bit-range sort reference of the GPU contract tests, on plain numpy: runs where there is no GPU."""
import numpy as np
import pytest

from stage_guard import ALIGN, GUARD, SENT, alloc_bytes, bit_range_order, payload_offset, violations


def _standin(base_addr, lead, cap, used):
    """a host stand-in for a guarded device allocation after a clean call that used `used` of `cap` bytes"""
    img = np.full(alloc_bytes(lead, cap), SENT, dtype=np.uint8)
    off = payload_offset(base_addr, lead)
    img[off: off + used] = 0x11
    return img, off


@pytest.mark.parametrize("base_addr", [0, 256, 1 << 40, (1 << 40) + 8, (1 << 40) + 255, 12345])
@pytest.mark.parametrize("lead", [0, 1, 15, 16, 255])
def test_payload_sits_lead_bytes_behind_an_aligned_address_with_guards_round_it(base_addr, lead):
    for cap in (0, 1, 4097):
        off = payload_offset(base_addr, lead)
        assert (base_addr + off - lead) % ALIGN == 0
        assert off >= GUARD and off + cap + GUARD <= alloc_bytes(lead, cap)


def test_one_flipped_byte_is_reported_where_it_is():
    cap, used = 1000, 900
    img, off = _standin((1 << 40) + 8, 3, cap, used)
    assert violations(img, off, cap, used) == []
    assert violations(img, off, cap, None) == []
    places = {
        "front guard, last byte": (off - 1, ("front", off - 1, 1)),
        "front guard, first byte": (0, ("front", 0, 1)),
        "spare capacity, first byte": (off + used, ("spare", 0, 1)),
        "spare capacity, last byte": (off + cap - 1, ("spare", cap - used - 1, 1)),
        "first byte behind out_cap": (off + cap, ("back", 0, 1)),
        "back guard, last byte": (len(img) - 1, ("back", len(img) - 1 - off - cap, 1)),
    }
    for name, (pos, want) in places.items():
        bad = img.copy()
        bad[pos] ^= 0xFF
        assert violations(bad, off, cap, used) == [want], name
    # a failed call owns the whole region: the spare bytes are not looked at, the guards are
    bad = img.copy()
    bad[off + used] ^= 0xFF
    assert violations(bad, off, cap, None) == []
    bad[off + cap] ^= 0xFF
    assert violations(bad, off, cap, None) == [("back", 0, 1)]
    # a byte of the used part that happens to equal the sentinel is no finding, and exact capacity has no spare region
    img[off + 5] = SENT
    assert violations(img, off, cap, used) == []
    assert violations(img, off, used, used) == []


@pytest.mark.parametrize("bit_lo,bit_hi", [(0, 8), (3, 13), (8, 16), (5, 5), (1, 64), (56, 64), (17, 40), (60, 64), (0, 64)])
def test_bit_range_order_equals_a_naive_stable_sort(bit_lo, bit_hi):
    rng = np.random.default_rng(bit_lo * 100 + bit_hi)
    n = 200
    keys = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    keys[:60] = keys[100:160]
    py = [int(k) for k in keys]
    mask = (1 << (bit_hi - bit_lo)) - 1
    naive = sorted(range(n), key=lambda i: (py[i] >> bit_lo) & mask)          # sorted() is stable
    assert bit_range_order(keys, bit_lo, bit_hi).tolist() == naive
    if bit_hi == bit_lo:
        assert naive == list(range(n))
