"""A brute-force model of the resync walk of damaged .jam archives (jampack_amd/csrc/jam_resync.hpp; DESIGN 4.6, "Damaged archives"),
the damaged archives the host and the GPU tests share, and the checks every recovered index must pass.

The model: a frame is valid at offset o iff the bytes there are "JAM" and the library's own frame walk of b[o:] reports at least one
frame; the rest is the loop of the rule written literally -- every offset is tried, there is no window and no candidate cap."""
import numpy as np

MiB = 1 << 20
NOFRAME, STAGE = 0, 1


def _i32(b, at):
    return int(np.frombuffer(bytes(b[at: at + 4]), dtype="<i4")[0])


def put_i32(b, at, v):
    b[at: at + 4] = np.frombuffer(np.int32(v).tobytes(), dtype=np.uint8)


def starts(a):
    o, s = 0, []
    while o < len(a):
        s.append(o)
        o += 15 + _i32(a, o + 7)
    return s


def model(jam, b, staged_ok=False):
    """-> (frames [(payload_off, psize)], gaps [(archive_off, archive_len, frame, NOFRAME)])"""
    walk = jam.jam_staged_frames if staged_ok else jam.jam_frames
    raw = bytes(b)
    n, g, frames, gaps = len(raw), 0, [], []
    while g < n:
        o, x = n, raw.find(b"JAM", g)
        while x >= 0:
            if walk(b[x:])[0] >= 1:
                o = x
                break
            x = raw.find(b"JAM", x + 1)
        if o > g:
            gaps.append((g, o - g, len(frames), NOFRAME))
        if o == n:
            break
        psize = _i32(raw, o + 7)
        frames.append((o + 15, psize))
        g = o + 15 + psize
    return frames, gaps


def table(ix):
    """(frames [(payload_off, psize)], gaps) of a JamIndex, in the model's form"""
    return [ix.frame(k)[2:] for k in range(ix.frames)], list(ix.gaps)


def check_tiling(ix, in_len):
    """frames and gaps tile [0, in_len) in order and without overlap; a gap's `frame` counts the frames in front of it; raw offsets are the
    prefix sums of the frames' raw sizes"""
    spans = [(po - 15, 15 + ps, 0, k) for k, (po, ps) in enumerate(ix.frame(k)[2:] for k in range(ix.frames))]
    spans += [(o, n, 1, f) for o, n, f, _ in ix.gaps]
    spans.sort(key=lambda t: (t[0], -t[2]))            # a gap in front of the frame that starts where it ends
    at, seen = 0, 0
    for o, n, is_gap, k in spans:
        assert o == at and n > 0, (o, at, n)
        assert k == seen, (k, seen, is_gap)
        at += n
        seen += 0 if is_gap else 1
    assert at == in_len and ix.archive_len == in_len, (at, in_len)
    ro = 0
    for k in range(ix.frames):
        assert ix.frame(k)[0] == ro, k
        ro += ix.frame(k)[1]
    assert ix.raw_len == ro and ix.bad_frame == -1


def decoy(psize=100, block_size=MiB, crc=0x12345678):
    return np.frombuffer(b"JAM" + np.uint32(crc).tobytes() + np.int32(psize).tobytes() + np.int32(block_size).tobytes(), dtype=np.uint8)


def deep_flip(a, k=2):
    """a byte flipped deep in frame k's rANS data, not in a chunk header: the frame stays structurally valid and fails its crc"""
    s = starts(a)
    b = a.copy()
    b[s[k] + 15 + _i32(a, s[k] + 7) - 8] ^= 0x10
    return b


def damage_cases(a, seed=5):
    """(name, archive) -- damage beyond hostile_cases, for an archive `a` of five frames"""
    s = starts(a)
    rng = np.random.default_rng(seed)
    junk = lambda n: rng.integers(0, 256, n, dtype=np.uint8)
    out = []
    b = a.copy(); put_i32(b, s[2] + 7, _i32(a, s[2] + 7) - 1)
    out.append(("psize_minus_1", b))
    b = a.copy(); put_i32(b, s[1] + 7, s[3] - s[1] - 15)
    out.append(("psize_swallows_next", b))
    b = a.copy(); b[s[2] + 15] ^= 0x01
    out.append(("first_payload_byte", b))
    out.append(("inserted_37", np.concatenate([a[: s[2]], junk(37), a[s[2]:]])))
    b = a.copy(); b[s[1]] ^= 1; b[s[2] + 1] ^= 1
    out.append(("two_lost", b))
    b = a.copy(); b[2] ^= 1
    out.append(("first_lost", b))
    out.append(("all_random", junk(len(a))))
    out.append(("fourteen_bytes", a[:14].copy()))
    b = a.copy(); b[s[2]] ^= 1; b[s[2] + 15: s[2] + 30] = decoy()
    out.append(("decoy_in_lost_payload", b))
    out.append(("decoy_flood", np.concatenate([a[: s[2]]] + [decoy(crc=i) for i in range(40)] + [a[s[2]:]])))
    return out
