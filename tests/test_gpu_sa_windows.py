"""The doubling rounds of the suffix sort (bwt_fwd_rounds.hip) at the edges of their 1024-slot windows.  -m gpu

The texts are sa_window_model's: test_sa_window_model.py shows, from the inputs alone, that with plain 7-byte keys their round-1 lists
(and the deep texts' round-2 lists) hold groups of exactly 1024 and of 1025, large groups that start on a window's first and last slot, end on a
window edge or end the list, windows with the tail of one large group and the head of the next, lists that end on a window edge or one slot
behind it, and the (passes, digit width) classes of the large groups' radix.  Here the kernels sort them:
  * JPK_KEY_BITS=8 (a child: the switch is read once per process) is the model's premise -- the library's own counts of round 1 and 2 must be
    the model's, so the kinds the model names are the ones the kernels met;
  * the default build in this process (variable-length keys, a depth per group: new_group_depth, gdr / gdw in the same kernels), no reach claim;
  * JPK_SA_WAIT_ROUND=3 JPK_LG_GRID=3 (a child): rounds 1 and 2 enqueued on the bound n -- windows past the list's end -- and three
    workgroups walking hundreds of pieces with a grid stride;
  * three texts as the blocks of one group sort; one text on guarded buffers at odd addresses.
Everything is bit-exact against the oracle (which test_oracle_vs_ref.py pins to the reference build).

Rounds are numbered as the library numbers them: sa_round_active[r] is the list round r STARTS with and sa_round_large[r] the members of groups
above 1024 in it (k_win_count's lc), so index 1 is the model's layout(t, 7) and index 2 its layout(t, 14)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sa_window_model as M
from stage_guard import Guarded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    import torch
    import jampack_amd as jam
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    yield torch, jam, ctx
    ctx.close()


@functools.lru_cache(maxsize=None)
def _expect(name):
    """(suffix array, BWT image) of a crafted text from the oracle: computed once, shared, left unchanged"""
    from oracle.pyoracle import Oracle
    o = Oracle()
    t = M.crafted(name)
    sa, bwt = o.suffix_array(t), o.bwt_forward(t)
    sa.setflags(write=False)
    bwt.setflags(write=False)
    return sa, bwt


def _suffix_array(torch, ctx, t):
    d_t = torch.from_numpy(np.array(t)).cuda()
    d_sa = torch.full((len(t),), -1, dtype=torch.int32, device="cuda")
    ctx.suffix_array(d_t, len(t), d_sa)
    torch.cuda.synchronize()
    return d_sa.cpu().numpy(), ctx.stats()


GROUP = ("edges-56k", "deeper", "one-large")


def _group_streams(torch, jam, ctx):
    """the compressed streams of the GROUP texts as the blocks of one blocks_compress call"""
    blocks = [np.array(M.crafted(name)) for name in GROUP]
    d_in = [torch.from_numpy(b).cuda() for b in blocks]
    caps = [jam.ans_capacity(len(b) + jam.TRAILER) for b in blocks]
    d_out = [torch.empty(c, dtype=torch.uint8, device="cuda") for c in caps]
    n, st = ctx.blocks_compress(d_in, [len(b) for b in blocks], d_out, caps, 2)
    assert st == [0] * len(blocks)
    return [d_out[i][: n[i]].cpu().numpy() for i in range(len(blocks))]


# every text through the suffix-array probe and the host entry of the forward BWT, one JSON line per text; then the group sort
_CHILD = r"""
import json, sys
import numpy as np
import torch
torch.cuda.is_available()
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import jampack_amd as jam
import sa_window_model as M
from oracle.pyoracle import Oracle
from test_gpu_sa_windows import GROUP, _group_streams, _suffix_array
o = Oracle()
ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
for name in M.TEXTS:
    t = M.crafted(name)
    sa, s = _suffix_array(torch, ctx, t)
    bwt = jam.Bwt().ForwardBwt(t)
    print("TEXT " + json.dumps({"name": name, "sa": bool(np.array_equal(sa, o.suffix_array(t))), "bwt": bool(np.array_equal(bwt, o.bwt_forward(t))),
                                "depth": int(s.sa_key_depth), "rounds": int(s.sa_rounds), "active": [int(v) for v in s.sa_round_active[:3]],
                                "large": [int(v) for v in s.sa_round_large[:3]]}), flush=True)
ok = [bool(np.array_equal(got, o.ans_encode(o.bwt_forward(M.crafted(name))))) for name, got in zip(GROUP, _group_streams(torch, jam, ctx))]
print("GROUP " + json.dumps(ok), flush=True)
ctx.close()
print("CHILD_DONE")
"""


def _child(env):
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT}], env=dict(os.environ, **env), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "CHILD_DONE" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    got = {}
    for line in r.stdout.splitlines():
        if line.startswith("TEXT "):
            d = json.loads(line[5:])
            got[d["name"]] = d
            print(d)
    assert list(got) == list(M.TEXTS)
    assert "GROUP [true, true, true]" in r.stdout, r.stdout[-500:]                 # the group sort of GROUP, every block's stream the oracle's
    return got


def _check_against_model(got):
    for name in M.TEXTS:
        d = got[name]
        assert d["sa"] and d["bwt"], d
        assert d["depth"] == M.DEPTH, d
        for r, h in ((1, M.DEPTH), (2, 2 * M.DEPTH)):
            if r == 2 and name not in M.DEEP:
                continue
            s = M.crafted_layout(name, h)
            assert d["rounds"] > r, d
            assert d["active"][r] == int(s.sum()), (name, r, d["active"], int(s.sum()))
            assert d["large"][r] == M.large_members(s), (name, r, d["large"], M.large_members(s))


def test_plain_keys_sort_the_lists_the_model_lays_out():
    """JPK_KEY_BITS=8: suffix array and BWT image are the oracle's, round 0 sorted on 7 bytes, and rounds 1 (every text) and 2 (the deep texts)
    started with as many suffixes, and as many of them in groups above 1024, as the model says"""
    _check_against_model(_child({"JPK_KEY_BITS": "8"}))


def test_rounds_enqueued_on_the_bound_with_three_workgroups_per_piece_kernel():
    """JPK_SA_WAIT_ROUND=3: rounds 1 and 2 run with grids for n suffixes, most of whose windows lie past the list's end (the last one ragged, full,
    or one slot wide); JPK_LG_GRID=3: every k_lg_* workgroup walks a third of the pieces.  The lists are the same lists: the model's counts hold"""
    _check_against_model(_child({"JPK_KEY_BITS": "8", "JPK_SA_WAIT_ROUND": "3", "JPK_LG_GRID": "3"}))


@pytest.mark.parametrize("name", M.TEXTS)
def test_default_keys_equal_the_oracle(gpu, name):
    """variable-length keys where the plan chooses them: a depth per group rides through the same kernels.  No claim about which windows are met"""
    torch, jam, ctx = gpu
    t = M.crafted(name)
    exp_sa, exp_bwt = _expect(name)
    sa, s = _suffix_array(torch, ctx, t)
    print(f"{name}: depth {s.sa_key_depth} order {s.sa_key_order} rounds {s.sa_rounds} active {list(s.sa_round_active[:s.sa_rounds])} "
          f"large {list(s.sa_round_large[:s.sa_rounds])}")
    assert np.array_equal(sa, exp_sa)
    assert np.array_equal(jam.Bwt().ForwardBwt(t), exp_bwt)


def test_three_texts_as_blocks_of_one_group_sort(gpu, oracle):
    """the block number is the sort's top digit and every suffix stops at its block's end: three lists' worth of groups in one list (the children
    repeat it with plain keys)"""
    torch, jam, ctx = gpu
    for name, got in zip(GROUP, _group_streams(torch, jam, ctx)):
        assert np.array_equal(got, oracle.ans_encode(np.array(_expect(name)[1]))), name


def test_guarded_buffers_at_odd_addresses(gpu):
    """the device entry on buffers 3 and 13 bytes behind an aligned address: the image is the oracle's, nothing outside it is written, the text is
    what it was"""
    torch, jam, ctx = gpu
    t = M.crafted("edges-213k")
    g_in = Guarded(torch, np.array(t), 3)
    g_out = Guarded(torch, None, 13, cap=len(t) + jam.TRAILER)
    m = ctx.bwt_forward(g_in.ptr, len(t), g_out.ptr, len(t) + jam.TRAILER)
    torch.cuda.synchronize()
    assert m == len(t) + jam.TRAILER
    g_out.check_output(_expect("edges-213k")[1], used=m, what="bwt_forward edges-213k")
    g_in.check_unchanged("bwt_forward edges-213k")
