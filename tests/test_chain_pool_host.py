"""The chain pool's picking logic (jampack_amd/csrc/chain_pool.hpp, JpkChainPicker) on the CPU, with integer handles.

A stand-alone C++ program with its own main includes the header, is built once with the thread sanitizer and once with the address
and undefined-behaviour sanitizers, and runs 16 threads x 100 000 acquire/release pairs on pools of 1, 2 and 4 handles.  Under the
pool's mutex (the header's audit hooks) it checks at every pick and every release that no count is negative, that the counts add up
to the number of holders, and that the pick is a minimum of the counts at that moment, the lowest index among equals."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jampack_amd", "csrc")

PROGRAM = r"""
#include "chain_pool.hpp"

#include <atomic>
#include <climits>
#include <cstdio>
#include <thread>

static const int THREADS = 16, PAIRS = 100000;

static long run(int n)
{
    std::vector<int> handles;
    for (int i = 0; i < n; i++) handles.push_back(100 + i);
    JpkChainPicker<int> pool(handles);
    long holders = 0;                       // touched inside the audit hooks only, that is under the pool's mutex
    std::atomic<long> bad{0};
    auto counts_ok = [&](const int *c, int m) {
        long sum = 0;
        for (int i = 0; i < m; i++) {
            if (c[i] < 0) bad++;
            sum += c[i];
        }
        if (m != n || sum != holders) bad++;
    };
    auto on_pick = [&](const int *c, int m, int slot) {
        counts_ok(c, m);
        int mn = INT_MAX, first = -1;
        for (int i = 0; i < m; i++)
            if (c[i] < mn) { mn = c[i]; first = i; }
        if (slot != first) bad++;           // a minimum at the time of the pick, ties to the lowest index
        holders++;
    };
    auto on_release = [&](const int *c, int m, int) {
        holders--;
        counts_ok(c, m);
    };
    std::vector<std::thread> th;
    for (int t = 0; t < THREADS; t++)
        th.emplace_back([&, t] {
            for (int k = 0; k < PAIRS; k++) {
                int h = -1, h2 = -1;
                const int s = pool.acquire(&h, on_pick);
                if (s < 0 || s >= n || h != 100 + s) { bad++; continue; }
                if ((k + t) % 7 == 0) {     // now and then two at once, so that counts above one occur in a pool of any size
                    const int s2 = pool.acquire(&h2, on_pick);
                    if (s2 < 0 || s2 >= n || h2 != 100 + s2) bad++;
                    else pool.release(s2, on_release);
                }
                pool.release(s, on_release);
            }
        });
    for (auto &x : th) x.join();
    if (pool.in_flight() != 0 || holders != 0) bad++;
    return bad.load();
}

int main()
{
    JpkChainPicker<int> none(std::vector<int>{});
    int h = 7;
    if (none.acquire(&h) != -1 || none.size() != 0) { printf("empty pool: FAIL\n"); return 1; }
    long bad = 0;
    for (int n : {1, 2, 4}) {
        const long b = run(n);
        printf("pool of %d: %ld violations\n", n, b);
        bad += b;
    }
    printf(bad ? "CHAIN_POOL_FAIL\n" : "CHAIN_POOL_OK\n");
    return bad ? 1 : 0;
}
"""


def _compiler():
    for name in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def _no_aslr():
    """in the child, before the program starts: personality(ADDR_NO_RANDOMIZE), what `setarch -R` does"""
    import ctypes
    libc = ctypes.CDLL(None, use_errno=True)
    cur = libc.personality(0xFFFFFFFF)
    if cur != -1:
        libc.personality(cur | 0x0040000)


@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_picker_invariants_under_sanitizers(sanitize, tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    src, exe = tmp_path / "chain_pool_host.cpp", tmp_path / "chain_pool_host"
    src.write_text(PROGRAM)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-pthread", f"-fsanitize={sanitize}", "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    if "unexpected memory mapping" in r.stderr:
        # the sanitizer's runtime found the program loaded where its shadow layout has no room for it (kernels with more address-space
        # randomisation than the runtime was built for): the same program once more with randomisation off for that one process
        r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, preexec_fn=_no_aslr)
    assert r.returncode == 0 and "CHAIN_POOL_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
