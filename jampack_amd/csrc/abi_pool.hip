// abi_pool.hip -- the process-wide context pool behind the host-buffer (drop-in) entry points, the batch entries' worker
// contexts, and jpk_init / jpk_shutdown / jpk_release_idle, which own the lifetime of both.
#include <algorithm>
#include <mutex>
#include <vector>

#include "abi.hpp"
#include "chain_pool.hpp"

// ---- the threads' contexts ---------------------------------------------------------------------------------
// Re-entrant from the OpenMP block loop of jampack.cpp:215/313: every calling thread works on a context of its own
// (stream + HBM arena + staging buffers).  Contexts live in a process-wide pool: a thread borrows one on its first
// call and hands it back when it exits, so the arenas persist across thread teams (the reference pays five
// cudaMalloc/cudaFree per block instead, bwt.cpp:195-239).  Threads are dealt round robin over the devices selected
// by jpk_init(device_mask) -- `jampack -t 8` on an 8-GPU node puts one block on each GPU.
namespace {
struct CtxPool {
    std::mutex mu;
    std::vector<int> devices;                       // selected devices (empty = not initialised yet)
    std::vector<std::vector<jpk_ctx *>> idle;       // per selected device: contexts nobody holds
    std::vector<jpk_ctx *> all;                     // every context the pool has created
    uint64_t generation = 1;                        // bumped by jpk_shutdown: borrowed handles of older generations are dead
    uint32_t next_thread = 0;
    int init_rc = JPK_OK;
};
CtxPool &pool() { static CtxPool p; return p; }

// caller holds pool().mu
int pool_select(CtxPool &p, uint64_t mask)
{
    p.devices.clear();
    p.idle.clear();
    const int n = jpk_device_count();
    if (n <= 0) return JPK_E_NODEVICE;
    for (int d = 0; d < n && d < 64; d++) {
        if (mask && !((mask >> d) & 1u)) continue;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) != hipSuccess) continue;
        if (!jpk_arch_ok(prop)) continue;
        p.devices.push_back(d);
    }
    if (p.devices.empty()) return JPK_E_NODEVICE;
    p.idle.resize(p.devices.size());
    return JPK_OK;
}

struct TlsCtx {
    jpk_ctx *ctx = nullptr;
    uint64_t generation = 0;
    size_t slot = 0;
    ~TlsCtx()
    {
        if (!ctx) return;
        CtxPool &p = pool();
        std::lock_guard<std::mutex> g(p.mu);
        if (generation == p.generation && slot < p.idle.size()) p.idle[slot].push_back(ctx);   // else: jpk_shutdown already destroyed it
    }
};
thread_local TlsCtx tls;
}  // namespace

int jpk_tls_ctx(jpk_ctx **out)
{
    CtxPool &p = pool();
    std::lock_guard<std::mutex> g(p.mu);
    if (tls.ctx && tls.generation == p.generation) { *out = tls.ctx; return JPK_OK; }
    tls.ctx = nullptr;
    if (p.devices.empty()) {
        // no jpk_init(): JPK_DEVICE pins one device, otherwise every visible gfx950 device takes part
        uint64_t mask = 0;
        if (const char *e = getenv("JPK_DEVICE")) { const int d = atoi(e); if (d < 0 || d >= 64) return JPK_E_NODEVICE; mask = 1ull << d; }
        JPK_TRY(pool_select(p, mask));
    }
    const size_t slot = (size_t)(p.next_thread++ % p.devices.size());
    jpk_ctx *c = nullptr;
    if (!p.idle[slot].empty()) { c = p.idle[slot].back(); p.idle[slot].pop_back(); }
    else {
        JPK_TRY(jpk_ctx_create(&c, p.devices[slot], nullptr));
        p.all.push_back(c);
    }
    tls.ctx = c; tls.generation = p.generation; tls.slot = slot;
    *out = c;
    return JPK_OK;
}

// the opening of the host-buffer entries: the calling thread's context, its device current, stage_in of at least stage_in_bytes
int jpk_host_enter(jpk_ctx **ctx, size_t stage_in_bytes)
{
    JPK_TRY(jpk_tls_ctx(ctx));
    JPK_HIP(hipSetDevice((*ctx)->device));
    return jpk_buf_ensure(*ctx, &(*ctx)->stage_in, &(*ctx)->stage_in_cap, stage_in_bytes);
}

namespace {
// worker contexts of the batch compress call, per device.  They are the library's own (a list apart from the host-buffer pool:
// a device-API call must not make jpk_init() believe that host-buffer contexts exist); jpk_shutdown destroys them too.
std::vector<std::vector<jpk_ctx *>> &batch_idle() { static std::vector<std::vector<jpk_ctx *>> v(64); return v; }
std::vector<jpk_ctx *> &batch_all() { static std::vector<jpk_ctx *> v; return v; }
}  // namespace

uint64_t jpk_pool_generation()
{
    CtxPool &p = pool();
    std::lock_guard<std::mutex> g(p.mu);
    return p.generation;
}

int jpk_batch_ctx_acquire(int device, jpk_ctx **out)
{
    CtxPool &p = pool();
    std::lock_guard<std::mutex> g(p.mu);
    auto &idle = batch_idle()[(size_t)device];
    if (!idle.empty()) { *out = idle.back(); idle.pop_back(); return JPK_OK; }
    jpk_ctx *c = nullptr;
    JPK_TRY(jpk_ctx_create(&c, device, nullptr));
    batch_all().push_back(c);
    *out = c;
    return JPK_OK;
}
void jpk_batch_ctx_release(int device, jpk_ctx *c, uint64_t generation)
{
    CtxPool &p = pool();
    std::lock_guard<std::mutex> g(p.mu);
    if (generation == p.generation) batch_idle()[(size_t)device].push_back(c);      // else jpk_shutdown already destroyed it
}

extern "C" int jpk_init(uint64_t device_mask)
{
    CtxPool &p = pool();
    std::lock_guard<std::mutex> g(p.mu);
    if (!p.all.empty()) return JPK_E_ARG;           // contexts exist: jpk_shutdown() first
    JPK_TRY(pool_select(p, device_mask));
    p.next_thread = 0;
    return (int)p.devices.size();
}

extern "C" int jpk_init_devices(int32_t *devices, int32_t cap)
{
    CtxPool &p = pool();
    std::lock_guard<std::mutex> g(p.mu);
    const int n = (int)p.devices.size();
    for (int i = 0; i < n && i < cap && devices; i++) devices[i] = p.devices[(size_t)i];
    return n;
}

extern "C" int jpk_thread_device(void)
{
    jpk_ctx *ctx;
    int rc = jpk_tls_ctx(&ctx);
    return rc == JPK_OK ? ctx->device : rc;
}

extern "C" void jpk_shutdown(void)
{
    const JpkMultiAllLocks multi_lock;                          // no multi-device call is using the communicators / slabs destroyed below
    JpkDeviceRestore restore;                                     // (destroying contexts and slabs moves the current device around: ADVICE r5)
    CtxPool &p = pool();
    std::lock_guard<std::mutex> g(p.mu);
    for (jpk_ctx *c : p.all) jpk_ctx_destroy(c);    // synchronises each context's streams first
    p.all.clear();
    p.idle.clear();
    for (jpk_ctx *c : batch_all()) jpk_ctx_destroy(c);      // the batch-compress workers' contexts
    batch_all().clear();
    for (auto &v : batch_idle()) v.clear();
    jpk_chain_pools_destroy();                              // every context is gone: no chain is on a pool stream
    jpk_multi_teardown();
    p.devices.clear();
    p.generation++;
    p.next_thread = 0;
}

// Gives back what the batch entries keep between calls and nobody is using: the idle worker contexts of jpk_dev_blocks_compress /
// jpk_dev_blocks_decompress (an arena of ~54 bytes per block byte each) and the multi-device entries' slabs.  The host-buffer pool's
// contexts stay (threads hold them).  Safe beside running calls: a context that is in use is not in the idle lists.  Returns the
// number of contexts destroyed.
extern "C" int jpk_release_idle(void)
{
    int freed = 0;
    JpkDeviceRestore restore;                                   // jpk_ctx_destroy and the slabs' hipFree set the device: the caller's comes back
    jpk_multi_free_unlocked_slabs();
    CtxPool &p = pool();
    std::lock_guard<std::mutex> g(p.mu);
    for (auto &idle : batch_idle()) {
        for (jpk_ctx *c : idle) {
            auto &all = batch_all();
            all.erase(std::remove(all.begin(), all.end(), c), all.end());
            jpk_ctx_destroy(c);
            freed++;
        }
        idle.clear();
    }
    return freed;
}

