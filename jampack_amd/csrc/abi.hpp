// abi.hpp -- what crosses the borders between the units of the C ABI (abi.hip, abi_pool.hip, abi_blocks.hip, abi_multi.hip,
// abi_host.hip) and nothing else.  What the archive layer shares with them is in common.hpp.
#pragma once
#include <condition_variable>
#include <mutex>
#include <vector>

#include "common.hpp"

// ---- abi.hip -------------------------------------------------------------------------------------------------
// the kernels are built and tuned for gfx950 only; JPK_ALLOW_ANY_ARCH (presence) lets another device through
bool jpk_arch_ok(const hipDeviceProp_t &prop);
// the test hooks that CHANGE live state work only in a process that sets JPK_DEBUG_HOOKS=1
bool jpk_debug_hooks_on();

// per-block statuses of a batch call: the caller's array, or `local` when the caller passed none -- the call then returns the first
// status that is not JPK_OK
static inline int32_t *jpk_status_or_local(int32_t *status, std::vector<int32_t> &local, int32_t nblocks)
{
    if (status) return status;
    local.assign((size_t)nblocks, 0);
    return local.data();
}
static inline int jpk_first_error(const int32_t *st, int32_t nblocks)
{
    for (int b = 0; b < nblocks; b++) if (st[b] != JPK_OK) return st[b];
    return JPK_OK;
}

// the caller's current device comes back when this leaves scope
struct JpkDeviceRestore {
    int dev = -1;
    JpkDeviceRestore() { if (hipGetDevice(&dev) != hipSuccess) dev = -1; }
    ~JpkDeviceRestore() { if (dev >= 0) (void)hipSetDevice(dev); }
};

// ---- abi_pool.hip --------------------------------------------------------------------------------------------
// bumped by jpk_shutdown: contexts borrowed under an older generation are dead, and are not handed back
uint64_t jpk_pool_generation();
// the batch entries' worker contexts, per device: the library's own, apart from the host-buffer pool
int jpk_batch_ctx_acquire(int device, jpk_ctx **out);
void jpk_batch_ctx_release(int device, jpk_ctx *c, uint64_t generation);

// ---- abi_blocks.hip ------------------------------------------------------------------------------------------
// "block k's input has arrived on the device": set by the copier thread of the multi-device entry (multi_run), waited for -- on the host,
// task by task -- by the workers of jpk_blocks_compress_body, so that block k + 1 is still on its way in while block k is being compressed
struct JpkBlocksReady {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<char> ok;
    bool failed = false;
    explicit JpkBlocksReady(size_t n) : ok(n, 0) {}
    void set(size_t k) { { std::lock_guard<std::mutex> g(mu); ok[k] = 1; } cv.notify_all(); }
    void fail() { { std::lock_guard<std::mutex> g(mu); failed = true; } cv.notify_all(); }
    bool wait(int first, int count)
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] {
            if (failed) return true;
            for (int k = first; k < first + count; k++) if (!ok[(size_t)k]) return false;
            return true;
        });
        return !failed;
    }
};
// jpk_dev_blocks_compress; ready (nullable): the inputs arrive while the call runs
int jpk_blocks_compress_body(jpk_ctx *ctx, int32_t nblocks, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                             const int32_t *out_cap, int32_t *out_len, int32_t *status, int32_t in_flight, JpkBlocksReady *ready);

// ---- abi_multi.hip -------------------------------------------------------------------------------------------
// every device's mutex of the multi-device entries, ascending; released in reverse
struct JpkMultiAllLocks {
    JpkMultiAllLocks();
    ~JpkMultiAllLocks();
    JpkMultiAllLocks(const JpkMultiAllLocks &) = delete;
    JpkMultiAllLocks &operator=(const JpkMultiAllLocks &) = delete;
};
// destroys the communicators and every device's slabs (the caller holds JpkMultiAllLocks and restores the current device)
void jpk_multi_teardown();
// frees the slabs of the devices no multi-device call holds right now (the caller restores the current device)
void jpk_multi_free_unlocked_slabs();
