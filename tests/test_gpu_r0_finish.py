"""Round 0's finish of the suffix sort (bwt_fwd_r0.hip) at the edges of its 4096-slot tiles, in both forms, and the run-length kernels.  -m gpu

The texts are r0_tile_model's: test_r0_tile_model.py shows, from the inputs alone, that with plain 7-byte keys their sorted lists put a short
suffix on a row's, a wave's and a tile's last slot and on a tile's first, pairs and groups across every kind of edge, singletons on the slots
where the word, the wave or the tile behind decides, tiles without a head, a head 65 and more tiles in front, lists of n = 50, 4095, 4096 k and
4097 slots, and runs over tile edges, whole tiles and the text's end -- and that a kernel which dropped one of the cross-edge rules would
leave another number of survivors, other ranks or other run lengths on them.  Here the kernels sort them:
  * JPK_KEY_BITS=8 (children: the switches are read once per process) is the model's premise, once as the one-pass look-back form
    (JPK_R0_LOOKBACK=1) and once as the two-pass comparator k_r0_count + k_r0_scan + k_r0_finish (JPK_R0_LOOKBACK=0): the suffix array of ALL n
    bytes and the BWT image are the oracle's, round 0 sorted on 7 bytes, and the library's own count of what round 0 left -- sa_round_active[1],
    sa_round_large[1], sa_rounds == 1 when nothing is left -- is the model's; the two forms report the same line for every text, and the
    profiler's launch count of k_r0_* on a text that round 0 sorts completely (1 against 2) shows that each child ran the form it was asked for;
  * the default keys in this process and in a JPK_R0_LOOKBACK=0 child: bit-exact, no reach claim (the variable-length keys move the groups);
  * five texts as the blocks of one group sort (the `bend` branches of r0_end / r0_short, the `blk` branch of run_ends_at), under both forms
    and both kinds of key, every stream the oracle's.
Not reached: see r0_tile_model's docstring (grid strides, the depth of the look-back walk) and test_gpu_big_blocks.py (the tagless form)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import r0_tile_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP = ("long-run", "n-50", "short-tile", "pair-tile", "runs-3tiles")          # the long run and a block below 120 bytes among them


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
    t = np.array(M.crafted(name))
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


def _group_streams(torch, jam, ctx):
    """the compressed streams of the GROUP texts as the blocks of one blocks_compress call"""
    blocks = [np.array(M.crafted(name)) for name in GROUP]
    d_in = [torch.from_numpy(b).cuda() for b in blocks]
    caps = [jam.ans_capacity(len(b) + jam.TRAILER) for b in blocks]
    d_out = [torch.empty(c, dtype=torch.uint8, device="cuda") for c in caps]
    n, st = ctx.blocks_compress(d_in, [len(b) for b in blocks], d_out, caps, 2)
    assert st == [0] * len(blocks)
    return [d_out[i][: n[i]].cpu().numpy() for i in range(len(blocks))]


ONE_ROUND = "rand256-8192"              # no survivors under either kind of key: round 0 is the whole sort
R0_CLASS = "k_r0_*/k_lg_finish/k_cmp_*"  # the profiler's class of k_r0_count and k_r0_finish (PROF_SA_RERANK)

# every text through the suffix-array probe and the host entry of the forward BWT, one JSON line per text; then the group sort
_CHILD = r"""
import json, sys
import numpy as np
import torch
torch.cuda.is_available()
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import jampack_amd as jam
import r0_tile_model as M
from test_gpu_r0_finish import GROUP, ONE_ROUND, R0_CLASS, _expect, _group_streams, _suffix_array
from oracle.pyoracle import Oracle
o = Oracle()
ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
ctx.profile_enable(2)                  # which form is this?  A text that is sorted after round 0 launches nothing else of k_r0_*'s class
_suffix_array(torch, ctx, M.crafted(ONE_ROUND))
print("R0_LAUNCHES %%d" %% {r["name"]: r["launches"] for r in ctx.profile_table()}.get(R0_CLASS, 0), flush=True)
ctx.profile_enable(0)
for name in M.TEXTS:
    t = M.crafted(name)
    exp_sa, exp_bwt = _expect(name)
    sa, s = _suffix_array(torch, ctx, t)
    r = int(s.sa_rounds)
    bwt = jam.Bwt().ForwardBwt(t)
    print("TEXT " + json.dumps({"name": name, "sa": bool(np.array_equal(sa, exp_sa)), "bwt": bool(np.array_equal(bwt, exp_bwt)),
                                "depth": int(s.sa_key_depth), "rounds": r, "active": [int(v) for v in s.sa_round_active[:max(r, 2)]],
                                "large": [int(v) for v in s.sa_round_large[:max(r, 2)]]}), flush=True)
ok = [bool(np.array_equal(got, o.ans_encode(np.array(_expect(name)[1])))) for name, got in zip(GROUP, _group_streams(torch, jam, ctx))]
print("GROUP " + json.dumps(ok), flush=True)
ctx.close()
print("CHILD_DONE")
"""


_RAN = {}


def _child(env):
    """the lines of one child, by text: a child per set of switches, run ONCE and shared by the tests that read it -- a child that failed is
    not started again, its failure is every reader's"""
    if env not in _RAN:
        try:
            _RAN[env] = _run_child(env)
        except BaseException as e:
            _RAN[env] = e
    if isinstance(_RAN[env], BaseException):
        raise _RAN[env]
    return _RAN[env]


def _run_child(env):
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT}], env=dict(os.environ, **dict(env)), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "CHILD_DONE" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    got = {}
    for line in r.stdout.splitlines():
        if line.startswith("TEXT "):
            d = json.loads(line[5:])
            got[d["name"]] = d
            print(d)
    assert list(got) == list(M.TEXTS)
    # the switch was read: one launch of k_r0_finish in the look-back form, k_r0_count + k_r0_finish in the two-pass form
    assert "R0_LAUNCHES %d\n" % (2 if dict(env).get("JPK_R0_LOOKBACK") == "0" else 1) in r.stdout, r.stdout[:300]
    assert "GROUP " + json.dumps([True] * len(GROUP)) in r.stdout, r.stdout[-500:]      # the group sort of GROUP, every block's stream the oracle's
    return got


PLAIN_LOOKBACK = (("JPK_KEY_BITS", "8"), ("JPK_R0_LOOKBACK", "1"))
PLAIN_TWO_PASS = (("JPK_KEY_BITS", "8"), ("JPK_R0_LOOKBACK", "0"))


def _check_against_model(got):
    for name in M.TEXTS:
        d, t = got[name], M.crafted(name)
        left, large = M.survivors(t), M.large_members(t)
        assert d["sa"] and d["bwt"], d
        assert d["depth"] == M.DEPTH, d
        assert d["active"][0] == len(t), d
        assert d["active"][1] == left, (name, d["active"], left)
        assert d["large"][1] == large, (name, d["large"], large)
        assert (d["rounds"] == 1) == M.ends_after_round_0(t), (name, d["rounds"], left)


def test_plain_keys_one_pass_look_back_leaves_what_the_model_counts():
    """JPK_KEY_BITS=8 JPK_R0_LOOKBACK=1: suffix array and BWT image are the oracle's, round 0 sorted on 7 bytes and left as many suffixes, and
    as many of them in groups above 1024, as the model derives from the text; the sort ends after round 0 exactly when none is left"""
    _check_against_model(_child(PLAIN_LOOKBACK))


def test_plain_keys_two_pass_comparator_leaves_what_the_model_counts():
    """JPK_KEY_BITS=8 JPK_R0_LOOKBACK=0: k_r0_count, k_r0_scan and phase 0 of k_r0_finish -- the form the look-back is judged against"""
    _check_against_model(_child(PLAIN_TWO_PASS))


def test_the_two_forms_report_identical_stats():
    one, two = _child(PLAIN_LOOKBACK), _child(PLAIN_TWO_PASS)
    for name in M.TEXTS:
        assert one[name] == two[name], (one[name], two[name])


def test_default_keys_two_pass_comparator_equals_the_oracle():
    """variable-length keys where the plan chooses them, JPK_R0_LOOKBACK=0: bit-exact (asserted in the child's lines), no reach claim"""
    for d in _child((("JPK_R0_LOOKBACK", "0"),)).values():
        assert d["sa"] and d["bwt"], d


@pytest.mark.parametrize("name", M.TEXTS)
def test_default_keys_equal_the_oracle(gpu, name):
    """the default build in this process (look-back form, variable-length keys).  No claim about which slots are met"""
    torch, jam, ctx = gpu
    t = M.crafted(name)
    exp_sa, exp_bwt = _expect(name)
    sa, s = _suffix_array(torch, ctx, t)
    print(f"{name}: depth {s.sa_key_depth} order {s.sa_key_order} rounds {s.sa_rounds} active {list(s.sa_round_active[:s.sa_rounds])} "
          f"large {list(s.sa_round_large[:s.sa_rounds])}")
    assert np.array_equal(sa, exp_sa)
    assert np.array_equal(jam.Bwt().ForwardBwt(t), exp_bwt)


def test_five_texts_as_blocks_of_one_group_sort(gpu, oracle):
    """the block number is the key's low byte, a suffix is short against ITS block's end and a run stops there: the long run, a block below 120
    bytes and three edge texts in one list (the children repeat it under both forms with plain keys, and two-pass with the default keys)"""
    torch, jam, ctx = gpu
    for name, got in zip(GROUP, _group_streams(torch, jam, ctx)):
        assert np.array_equal(got, oracle.ans_encode(np.array(_expect(name)[1]))), name
