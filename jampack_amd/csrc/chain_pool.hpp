// chain_pool.hpp -- the streams the rANS encode chains (k_rans_lanes) run on: a few high-priority streams per device, owned by the
// library and shared by all contexts.  The runtime keeps a pool of hardware queues per stream priority, so a chain on one of these
// streams does not sit in a normal-priority queue in front of other blocks' wide kernels (abi.hip, header comment).
//
// The picking logic is free of HIP (a template on the handle type: tests/test_chain_pool_host.py runs it on the CPU with integer
// handles under the thread and address sanitizers); the per-device pools of hipStream_t are in abi.hip.
#pragma once
#include <mutex>
#include <utility>
#include <vector>

// N handles and, per handle, the number of chains in flight on it.  acquire() picks the handle with the fewest, ties to the lowest
// index; release() gives it back.  Both run under one mutex and the counts are exact: a host thread that acquired a handle stays
// inside its compress call until its chain has finished, then releases.
template <class Handle> class JpkChainPicker {
  public:
    explicit JpkChainPicker(std::vector<Handle> handles) : handles_(std::move(handles)), busy_(handles_.size(), 0) {}
    JpkChainPicker(const JpkChainPicker &) = delete;
    JpkChainPicker &operator=(const JpkChainPicker &) = delete;
    int size() const { return (int)handles_.size(); }
    const std::vector<Handle> &handles() const { return handles_; }

    // Returns the slot picked (and its handle in *out), -1 when the pool is empty.  `audit(counts, n, slot)` runs under the mutex with
    // the counts as they were when the pick was made (before the pick is counted): the host test's window into the invariant.
    template <class Audit> int acquire(Handle *out, Audit &&audit)
    {
        std::lock_guard<std::mutex> g(mu_);
        const int n = (int)busy_.size();
        if (n == 0) return -1;
        int best = 0;
        for (int i = 1; i < n; i++)
            if (busy_[(size_t)i] < busy_[(size_t)best]) best = i;
        audit((const int *)busy_.data(), n, best);
        busy_[(size_t)best]++;
        *out = handles_[(size_t)best];
        return best;
    }
    int acquire(Handle *out) { return acquire(out, [](const int *, int, int) {}); }

    // `audit(counts, n, slot)` runs under the mutex with the counts after the release
    template <class Audit> void release(int slot, Audit &&audit)
    {
        std::lock_guard<std::mutex> g(mu_);
        busy_[(size_t)slot]--;
        audit((const int *)busy_.data(), (int)busy_.size(), slot);
    }
    void release(int slot) { release(slot, [](const int *, int, int) {}); }

    int in_flight()
    {
        std::lock_guard<std::mutex> g(mu_);
        int s = 0;
        for (int b : busy_) s += b;
        return s;
    }

  private:
    std::mutex mu_;
    std::vector<Handle> handles_;
    std::vector<int> busy_;
};

#ifdef JPK_BUILD
#include "common.hpp"
// The pool of `device` (made on first use: JPK_CHAIN_STREAMS streams, default 4, 1..8, created together with the greatest priority the
// device reports).  Returns the slot and its stream, or -1 when there is no pool -- JPK_CHAIN_STREAMS=0, a device without stream
// priorities, or stream creation failed -- and the caller keeps the chain on its own stream.  The device must be current.
int jpk_chain_acquire(int device, hipStream_t *stream);
void jpk_chain_release(int device, int slot);
// jpk_shutdown: synchronises and destroys every pool; the next acquire builds a new one
void jpk_chain_pools_destroy(void);

// One chain's hold on a pool stream.  Whatever way the holder leaves -- a failed launch, a failed wait -- the stream is synchronised
// before it goes back (the chain reads and writes the context's arena); done() is the way out once the host has seen the chain finish.
struct JpkChainLease {
    jpk_ctx *ctx;
    hipStream_t stream = nullptr;
    int slot = -1;
    explicit JpkChainLease(jpk_ctx *c) : ctx(c)
    {
        slot = jpk_chain_acquire(c->device, &stream);
        if (slot >= 0) c->chain_on_pool = true;
    }
    bool held() const { return slot >= 0; }
    void done()
    {
        if (slot < 0) return;
        jpk_chain_release(ctx->device, slot);
        ctx->chain_on_pool = false;
        slot = -1;
    }
    ~JpkChainLease()
    {
        if (slot < 0) return;
        (void)hipStreamSynchronize(stream);
        done();
    }
    JpkChainLease(const JpkChainLease &) = delete;
    JpkChainLease &operator=(const JpkChainLease &) = delete;
};
#endif
