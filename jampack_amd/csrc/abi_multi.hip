// abi_multi.hip -- the multi-GPU engine of the C ABI: jpk_blocks_compress_multi / _ex / jpk_blocks_decompress_multi, their RCCL
// loader, communicator cache, per-device locks and slabs.
#include <dlfcn.h>

#include <chrono>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "abi.hpp"

// ---- jpk_blocks_compress_multi: the block loop of Jampack::Compress over the GPUs of one node, natively ---------------------------
// Blocks are independent (jampack.cpp:215-219), so block b goes to device devices[b mod G] -- one worker thread and context per device,
// the thread moves its blocks in from host memory and compresses them there -- and the only exchange is the gather of the compressed
// blocks on the root (the first device of the mask), in block order = the order of the in-order CompWriteBlock loop
// (jampack.cpp:220-224): sizes are known on the host, so every non-root device sends each block with ONE ncclSend of exactly its
// bytes and the root posts the matching ncclRecv at the block's final offset (grouped: ncclGroupStart/End over a single-process
// communicator from ncclCommInitAll; every pair of GPUs has a direct xGMI link).  RCCL is loaded at first use (dlopen): the library
// has no link-time dependency on it, and a one-device mask never touches it unless JPK_MULTI_FORCE_RCCL=1 asks for the root's own
// blocks to travel through a send/receive to itself (exercises the path on a 1-GPU box).
namespace {
typedef struct jpkNcclComm *jpk_nccl_comm_t;
struct Rccl {
    void *h = nullptr;
    int (*CommInitAll)(jpk_nccl_comm_t *, int, const int *) = nullptr;
    int (*CommDestroy)(jpk_nccl_comm_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void *, size_t, int, int, jpk_nccl_comm_t, hipStream_t) = nullptr;
    int (*Recv)(void *, size_t, int, int, jpk_nccl_comm_t, hipStream_t) = nullptr;
    bool ok = false;
};
constexpr int NCCL_UINT8 = 1;                        // ncclUint8 (rccl.h: ncclInt8 = 0, ncclUint8 = 1)
Rccl &rccl()
{
    static Rccl r = [] {
        Rccl q;
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) { q.h = dlopen(name, RTLD_NOW | RTLD_LOCAL); if (q.h) break; }
        if (!q.h) return q;
        q.CommInitAll = (decltype(q.CommInitAll))dlsym(q.h, "ncclCommInitAll");
        q.CommDestroy = (decltype(q.CommDestroy))dlsym(q.h, "ncclCommDestroy");
        q.GroupStart = (decltype(q.GroupStart))dlsym(q.h, "ncclGroupStart");
        q.GroupEnd = (decltype(q.GroupEnd))dlsym(q.h, "ncclGroupEnd");
        q.Send = (decltype(q.Send))dlsym(q.h, "ncclSend");
        q.Recv = (decltype(q.Recv))dlsym(q.h, "ncclRecv");
        q.ok = q.CommInitAll && q.CommDestroy && q.GroupStart && q.GroupEnd && q.Send && q.Recv;
        return q;
    }();
    return r;
}
// one communicator set per device list, kept until jpk_shutdown
struct MultiComm { std::vector<int> devices; std::vector<jpk_nccl_comm_t> comms; };
std::deque<MultiComm> &multi_comms() { static std::deque<MultiComm> v; return v; }      // (a deque: a call holds a pointer into it while another call, on other devices, adds a set)
std::mutex &multi_mu() { static std::mutex m; return m; }

// devices of the mask that exist among `ndev` visible devices, ascending (mask 0 = all)
std::vector<int> multi_devices(uint64_t mask, int ndev)
{
    std::vector<int> d;
    for (int k = 0; k < ndev && k < 64; k++)
        if (!mask || ((mask >> k) & 1u)) d.push_back(k);
    return d;
}
}  // namespace

// host-logic probe (no device call): owner[b] = the device block b of `nblocks` would run on for `device_mask` when `ndev_visible`
// devices are visible; returns the number of devices taking part (the root is the first of them)
extern "C" int jpk_debug_multi_plan(uint64_t device_mask, int32_t ndev_visible, int32_t nblocks, int32_t *owner)
{
    if (ndev_visible < 0 || nblocks < 0 || (nblocks > 0 && !owner)) return JPK_E_ARG;
    const std::vector<int> dv = multi_devices(device_mask, ndev_visible);
    if (dv.empty()) return JPK_E_NODEVICE;
    for (int b = 0; b < nblocks; b++) owner[b] = dv[(size_t)b % dv.size()];
    return (int)dv.size();
}

// Shared body of the two multi-device entries.  One call at a time PER DEVICE: a call holds the mutexes of the devices of its mask
// (taken in ascending order) from its first device call to its last, so two calls on disjoint device sets -- two files on two halves
// of a node -- run side by side, and calls that share a device queue (round 5: one process-wide mutex).  What the locks protect: the
// per-device slabs and copy streams below, and the RCCL communicators, which are cached per device LIST and are not safe for
// concurrent use -- two calls with the same list share all its devices and therefore exclude each other.  jpk_shutdown takes every
// device's mutex before it destroys slabs and communicators.
namespace {
std::mutex *multi_dev_mu() { static std::mutex m[64]; return m; }
struct MultiLocks {                                          // the devices of a call, ascending; released in reverse
    std::vector<int> held;
    explicit MultiLocks(const std::vector<int> &devs) { for (int d : devs) if (d >= 0 && d < 64) { multi_dev_mu()[d].lock(); held.push_back(d); } }
    ~MultiLocks() { for (size_t k = held.size(); k-- > 0;) multi_dev_mu()[held[k]].unlock(); }
    MultiLocks(const MultiLocks &) = delete;
    MultiLocks &operator=(const MultiLocks &) = delete;
};
// per device: one input slab and one output slab, kept between calls (grown when a larger call arrives), and the stream the inputs
// travel on while the context's stream computes; freed by jpk_shutdown / jpk_release_idle
struct MultiSlab { uint8_t *in = nullptr, *out = nullptr; size_t in_cap = 0, out_cap = 0; hipStream_t copy = nullptr; };
MultiSlab *multi_slabs() { static MultiSlab v[64]; return v; }
int slab_ensure(uint8_t **p, size_t *cap, size_t bytes)
{
    if (*cap >= bytes && *p) return JPK_OK;
    if (*p) { (void)hipFree(*p); *p = nullptr; *cap = 0; }
    const size_t want = jpk_align(bytes + bytes / 8 + 4096, 1 << 20);
    if (hipMalloc((void **)p, want) != hipSuccess) { *p = nullptr; (void)hipGetLastError(); return JPK_E_ALLOC; }
    *cap = want;
    return JPK_OK;
}
// (the caller holds device d's mutex and restores the current device)
void multi_slab_free(int d)
{
    MultiSlab &m = multi_slabs()[d];
    if (!m.in && !m.out && !m.copy) return;
    if (hipSetDevice(d) == hipSuccess) {
        if (m.copy) { (void)hipStreamSynchronize(m.copy); (void)hipStreamDestroy(m.copy); }
        if (m.in) (void)hipFree(m.in);
        if (m.out) (void)hipFree(m.out);
    }
    m = MultiSlab();
}
}  // namespace

JpkMultiAllLocks::JpkMultiAllLocks() { for (int d = 0; d < 64; d++) multi_dev_mu()[d].lock(); }
JpkMultiAllLocks::~JpkMultiAllLocks() { for (int d = 64; d-- > 0;) multi_dev_mu()[d].unlock(); }

void jpk_multi_teardown()
{
    {
        std::lock_guard<std::mutex> lk(multi_mu());
        for (auto &m : multi_comms())
            for (jpk_nccl_comm_t cm : m.comms) if (cm && rccl().ok) (void)rccl().CommDestroy(cm);
        multi_comms().clear();
    }
    for (int d = 0; d < 64; d++) multi_slab_free(d);
}

void jpk_multi_free_unlocked_slabs()
{
    for (int d = 0; d < 64; d++) {
        std::unique_lock<std::mutex> dev_lock(multi_dev_mu()[d], std::try_to_lock);    // a multi-device call in flight on the device keeps its slabs
        if (dev_lock.owns_lock()) multi_slab_free(d);
    }
}

// the output slot that always holds the compressed form of a block of len bytes
size_t jpk_multi_comp_cap(int32_t len) { return (size_t)((int64_t)(len + JPK_TRAILER_BYTES) * 5 / 4) + 4096 + 1400 * ((size_t)(len + JPK_TRAILER_BYTES) / JPK_ANS_CHUNK + 1); }

namespace {
// one call's arguments, and what its steps hand on: per-block statuses and output lengths, the devices taking part (root first)
// and each device's share
struct MultiDev { jpk_ctx *c = nullptr; MultiSlab *slab = nullptr; std::vector<int> blocks; std::vector<size_t> ioff, ooff; int rc = JPK_OK; };
struct MultiCall {
    bool compress; int32_t nblocks; const uint8_t *const *in; const int32_t *in_len, *raw_len; int32_t in_flight;
    int32_t *stp;
    std::vector<int32_t> olen;
    std::vector<int> devs;
    std::vector<MultiDev> dv;
    size_t cap_of(int b) const { return compress ? jpk_multi_comp_cap(in_len[b]) : (size_t)raw_len[b]; }
};

// The worker of device devs[g]: a batch context, the slab layout of its blocks, the copy in, the batch call, the blocks' statuses
// and lengths.  D.rc != JPK_OK: the device failed as a whole.
void multi_device_work(MultiCall &M, int g)
{
    MultiDev &D = M.dv[(size_t)g];
    const bool compress = M.compress;
    const uint8_t *const *in = M.in;
    const int32_t *in_len = M.in_len;
    if (D.blocks.empty()) return;
    const int dev = M.devs[(size_t)g];
    if (hipSetDevice(dev) != hipSuccess) { D.rc = JPK_E_DEVICE; return; }
    if ((D.rc = jpk_batch_ctx_acquire(dev, &D.c)) != JPK_OK) return;
    D.slab = &multi_slabs()[dev];
    size_t itotal = 0, ototal = 0;
    for (int b : D.blocks) {
        D.ioff.push_back(itotal); itotal += jpk_align((size_t)in_len[b] + 64, 256);
        D.ooff.push_back(ototal); ototal += jpk_align(M.cap_of(b), 256);
    }
    if ((D.rc = slab_ensure(&D.slab->in, &D.slab->in_cap, itotal + 256)) != JPK_OK) return;
    if ((D.rc = slab_ensure(&D.slab->out, &D.slab->out_cap, ototal + 256)) != JPK_OK) return;
    if (!D.slab->copy && hipStreamCreateWithFlags(&D.slab->copy, hipStreamNonBlocking) != hipSuccess) { D.slab->copy = nullptr; D.rc = JPK_E_DEVICE; return; }
    const size_t nb = D.blocks.size();
    std::vector<const uint8_t *> din(nb);
    std::vector<uint8_t *> dout(nb);
    std::vector<int32_t> ilen(nb), ocap(nb), ol(nb, 0), stl(nb, JPK_E_DEVICE);
    for (size_t k = 0; k < nb; k++) {
        const int b = D.blocks[k];
        din[k] = D.slab->in + D.ioff[k];
        dout[k] = D.slab->out + D.ooff[k];
        ilen[k] = in_len[b];
        const size_t cap = M.cap_of(b);
        ocap[k] = (int32_t)(cap > 0x7fffffff ? 0x7fffffff : cap);
    }
    int rc;
    if (compress) {
        // Round 6: the inputs travel on the slab's own stream, block by block in the order the batch entry takes them, from a
        // copier thread; a worker of the batch entry waits (on the host) only for the blocks of ITS next task, so block k + 1 is on
        // its way in while block k is being compressed -- the reference's loop overlaps its reads the same way, thread k compresses
        // while thread k + 1 still reads (jampack.cpp:205-224).  Rounds 4-5 copied ALL of a device's blocks in before its first kernel.
        // (Pageable host memory: the runtime stages it through pinned buffers of its own; the copies run at PCIe speed on this box,
        // tools/pcietest.hip.)
        JpkBlocksReady ready(nb);
        std::thread copier([&] {
            if (hipSetDevice(dev) != hipSuccess) { ready.fail(); return; }
            for (size_t k = 0; k < nb; k++) {
                const int b = D.blocks[k];
                if (in_len[b] && (hipMemcpyAsync(D.slab->in + D.ioff[k], in[b], (size_t)in_len[b], hipMemcpyHostToDevice, D.slab->copy) != hipSuccess ||
                                  hipStreamSynchronize(D.slab->copy) != hipSuccess)) { ready.fail(); return; }
                ready.set(k);
            }
        });
        rc = jpk_blocks_compress_body(D.c, (int32_t)nb, din.data(), ilen.data(), dout.data(), ocap.data(), ol.data(), stl.data(), M.in_flight, &ready);
        copier.join();
    } else {
        // the decode is ONE pass over the chunks of all the device's blocks and needs every stream in place; compressed inputs are a
        // fifth of the data and the pass is long: the copies stay in front of it, on the context's stream
        for (size_t k = 0; k < nb; k++) {
            const int b = D.blocks[k];
            if (in_len[b] && hipMemcpyAsync(D.slab->in + D.ioff[k], in[b], (size_t)in_len[b], hipMemcpyHostToDevice, D.c->stream) != hipSuccess) { D.rc = JPK_E_DEVICE; return; }
        }
        rc = jpk_dev_blocks_decompress(D.c, (int32_t)nb, din.data(), ilen.data(), dout.data(), ocap.data(), ol.data(), stl.data());
    }
    for (size_t k = 0; k < nb; k++) {
        const int b = D.blocks[k];
        M.stp[b] = rc != JPK_OK && stl[k] == JPK_OK ? rc : stl[k];
        M.olen[(size_t)b] = M.stp[b] == JPK_OK ? ol[k] : 0;
    }
    if (rc != JPK_OK) D.rc = rc;
}

// What is reported and what is gathered: a block's status is its own; a device that failed as a whole fails all its
// blocks; EVERY block whose status is JPK_OK is gathered -- a corrupt frame among healthy ones costs its own bytes only, the others
// are in d_out at [out_off[b], out_off[b + 1]) as the header promises -- and when the gather itself cannot run (the output buffer
// is too small, RCCL is not there) NO block is reported as done: every status is an error and every range is empty.
// Merges the devices' verdicts into the blocks' statuses and lays the gathered blocks out: out_off[0..nblocks] and *total.
// Returns the first status that is not JPK_OK, a failed device's first.
int multi_merge(MultiCall &M, int64_t *out_off, int64_t *total_out)
{
    int32_t *stp = M.stp;
    int rc_blocks = JPK_OK;
    for (MultiDev &D : M.dv)
        if (D.rc != JPK_OK) {
            if (rc_blocks == JPK_OK) rc_blocks = D.rc;
            for (int b : D.blocks) if (stp[b] == JPK_OK) { stp[b] = D.rc; M.olen[(size_t)b] = 0; }     // a failed device: none of its blocks is reported as done
        }
    if (rc_blocks == JPK_OK) rc_blocks = jpk_first_error(stp, M.nblocks);
    int64_t total = 0;
    for (int b = 0; b < M.nblocks; b++) { out_off[b] = total; total += M.olen[(size_t)b]; }
    out_off[M.nblocks] = total;
    *total_out = total;
    return rc_blocks;
}

// The communicator set of this device list, made on first use.  A communicator set belongs to a device LIST and is used under the
// mutexes of all its devices (the call holds them).  nullptr with *rc = JPK_E_DEVICE: RCCL is not there, or would not start.
const std::vector<jpk_nccl_comm_t> *multi_comms_for(const std::vector<int> &devs, int *rc)
{
    const int G = (int)devs.size();
    const std::vector<jpk_nccl_comm_t> *comms = nullptr;
    std::lock_guard<std::mutex> lk(multi_mu());
    if (!rccl().ok) *rc = JPK_E_DEVICE;
    else {
        for (auto &m : multi_comms()) if (m.devices == devs) comms = &m.comms;
        if (!comms) {
            MultiComm m;
            m.devices = devs;
            m.comms.resize((size_t)G);
            if (rccl().CommInitAll(m.comms.data(), G, devs.data()) != 0) *rc = JPK_E_DEVICE;
            else { multi_comms().push_back(m); comms = &multi_comms().back().comms; }
        }
    }
    return comms;
}

// the gather: root's own blocks are device-to-device copies; the others travel over RCCL, one send / receive pair per block.
// Enqueued on the contexts' streams; comms == nullptr: no RCCL in this call.
int multi_gather(MultiCall &M, const std::vector<jpk_nccl_comm_t> *comms, bool use_rccl, bool force_rccl, uint8_t *d_out, const int64_t *out_off)
{
    const int G = (int)M.devs.size();
    const std::vector<int32_t> &olen = M.olen;
    int rc = JPK_OK;
    if (hipSetDevice(M.devs[0]) != hipSuccess) rc = JPK_E_DEVICE;
    MultiDev &R = M.dv[0];
    hipStream_t rs = R.c ? R.c->stream : nullptr;
    if (rc == JPK_OK && use_rccl && comms) {
        bool grouped = rccl().GroupStart() == 0;
        for (int g = 0; g < G && grouped; g++) {
            MultiDev &D = M.dv[(size_t)g];
            if ((g == 0 && !force_rccl) || !D.c || !D.slab) continue;
            for (size_t k = 0; k < D.blocks.size(); k++) {
                const int b = D.blocks[k];
                if (olen[(size_t)b] == 0) continue;
                if (rccl().Send(D.slab->out + D.ooff[k], (size_t)olen[(size_t)b], NCCL_UINT8, 0, (*comms)[(size_t)g], D.c->stream) != 0) rc = JPK_E_DEVICE;
                if (rccl().Recv(d_out + out_off[b], (size_t)olen[(size_t)b], NCCL_UINT8, g, (*comms)[0], rs) != 0) rc = JPK_E_DEVICE;
            }
        }
        if (!grouped || rccl().GroupEnd() != 0) rc = JPK_E_DEVICE;
    }
    if (rc == JPK_OK && !(use_rccl && force_rccl) && R.c && R.slab)
        for (size_t k = 0; k < R.blocks.size(); k++) {
            const int b = R.blocks[k];
            if (olen[(size_t)b] && hipMemcpyAsync(d_out + out_off[b], R.slab->out + R.ooff[k], (size_t)olen[(size_t)b], hipMemcpyDeviceToDevice, rs) != hipSuccess) rc = JPK_E_DEVICE;
        }
    return rc;
}

// every stream that took part has finished before the slabs can be used by the next call (also on the error paths); the batch
// contexts go back.  Returns rc, or JPK_E_DEVICE when rc was JPK_OK and a stream did not drain.
int multi_drain(MultiCall &M, uint64_t generation, int rc)
{
    for (size_t g = 0; g < M.dv.size(); g++) {
        MultiDev &D = M.dv[g];
        if (!D.c) continue;
        if (hipSetDevice(M.devs[g]) != hipSuccess || hipStreamSynchronize(D.c->stream) != hipSuccess) rc = rc == JPK_OK ? JPK_E_DEVICE : rc;
        jpk_batch_ctx_release(M.devs[g], D.c, generation);
    }
    return rc;
}

// compress: in[b] host blocks of in_len[b] bytes -> compressed blocks; decompress: in[b] host compressed blocks, raw_len[b] = the
// block's decompressed size.  Either way block b runs on devices[b mod G] through the library's batch entry on that device
// (jpk_dev_blocks_compress with `in_flight` blocks in flight and grouped small blocks / jpk_dev_blocks_decompress: one pass over the
// chunks of all its blocks), and the results are gathered in block order on the first device.
int multi_run(bool compress, uint64_t device_mask, int32_t nblocks, const uint8_t *const *in, const int32_t *in_len, const int32_t *raw_len, uint8_t *d_out, int64_t out_cap,
              int64_t *out_off, int32_t *status, int32_t in_flight)
{
    if (nblocks < 0 || out_cap < 0 || !out_off || (nblocks > 0 && (!in || !in_len || !d_out || (!compress && !raw_len)))) return JPK_E_ARG;
    out_off[0] = 0;
    if (nblocks == 0) return JPK_OK;
    for (int b = 0; b < nblocks; b++)
        if (in_len[b] < 0 || (in_len[b] > 0 && !in[b]) || (!compress && raw_len[b] < 0)) return JPK_E_ARG;
    std::vector<int32_t> st_local;
    MultiCall M{compress, nblocks, in, in_len, raw_len, in_flight, jpk_status_or_local(status, st_local, nblocks), std::vector<int32_t>((size_t)nblocks, 0), {}, {}};
    int32_t *stp = M.stp;
    for (int b = 0; b < nblocks; b++) { stp[b] = JPK_E_DEVICE; out_off[b + 1] = 0; }   // a block nobody got to says so (a device whose worker bails out early)
    const int ndev = jpk_device_count();
    if (ndev <= 0) return JPK_E_NODEVICE;
    const std::vector<int> cand = multi_devices(device_mask, ndev);
    const MultiLocks locks(cand);                            // (ascending; before the first device call of this call)
    JpkDeviceRestore restore;                                // the caller's current device comes back on every exit path
    std::vector<int> &devs = M.devs;
    for (int d : cand) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) != hipSuccess) continue;
        if (!jpk_arch_ok(prop)) continue;
        devs.push_back(d);
    }
    if (devs.empty()) return JPK_E_NODEVICE;
    const int G = (int)devs.size();
    const uint64_t generation = jpk_pool_generation();

    M.dv.resize((size_t)G);
    for (int b = 0; b < nblocks; b++) M.dv[(size_t)(b % G)].blocks.push_back(b);
    {
        std::vector<std::thread> th;
        for (int g = 1; g < G; g++) { try { th.emplace_back(multi_device_work, std::ref(M), g); } catch (...) { M.dv[(size_t)g].rc = JPK_E_DEVICE; } }
        multi_device_work(M, 0);
        for (auto &t : th) t.join();
    }
    int64_t total = 0;
    const int rc_blocks = multi_merge(M, out_off, &total);
    int rc = JPK_OK;                                         // of the gather
    if (total > out_cap) rc = JPK_E_CAPACITY;

    static const bool force_rccl = jpk_env_long("JPK_MULTI_FORCE_RCCL", 0) != 0;
    const bool use_rccl = rc == JPK_OK && total > 0 && (G > 1 || force_rccl);
    const std::vector<jpk_nccl_comm_t> *comms = use_rccl ? multi_comms_for(devs, &rc) : nullptr;
    if (rc == JPK_OK && total > 0) rc = multi_gather(M, comms, use_rccl, force_rccl, d_out, out_off);
    rc = multi_drain(M, generation, rc);
    if (rc != JPK_OK) {                                      // no gather: nothing is in d_out, and nobody is told otherwise
        for (int b = 0; b < nblocks; b++) { if (stp[b] == JPK_OK) stp[b] = rc; out_off[b] = 0; }
        out_off[nblocks] = 0;
        return rc;
    }
    return rc_blocks;
}
}  // namespace

// host-logic probe (no device call): takes the device mutexes a multi-device call with this mask would take (bit d = device d; every
// bit counts, whether such a device exists or not), holds them for hold_ms milliseconds and lets go.  Two probes with disjoint masks
// overlap, two that share a bit queue: tests/test_abi_and_host.py.
extern "C" int jpk_debug_multi_lock_probe(uint64_t device_mask, int32_t hold_ms)
{
    if (hold_ms < 0 || hold_ms > 10000) return JPK_E_ARG;
    std::vector<int> devs;
    for (int d = 0; d < 64; d++) if ((device_mask >> d) & 1u) devs.push_back(d);
    const MultiLocks locks(devs);
    std::this_thread::sleep_for(std::chrono::milliseconds(hold_ms));
    return (int)devs.size();
}

extern "C" int jpk_blocks_compress_multi(uint64_t device_mask, int32_t nblocks, const uint8_t *const *in, const int32_t *in_len, uint8_t *d_out, int64_t out_cap,
                                         int64_t *out_off, int32_t *status)
{
    return multi_run(true, device_mask, nblocks, in, in_len, nullptr, d_out, out_cap, out_off, status, 0);
}
extern "C" int jpk_blocks_compress_multi_ex(uint64_t device_mask, int32_t nblocks, const uint8_t *const *in, const int32_t *in_len, uint8_t *d_out, int64_t out_cap,
                                            int64_t *out_off, int32_t *status, int32_t in_flight)
{
    return multi_run(true, device_mask, nblocks, in, in_len, nullptr, d_out, out_cap, out_off, status, in_flight);
}
extern "C" int jpk_blocks_decompress_multi(uint64_t device_mask, int32_t nblocks, const uint8_t *const *in, const int32_t *in_len, const int32_t *raw_len, uint8_t *d_out,
                                           int64_t out_cap, int64_t *out_off, int32_t *status)
{
    return multi_run(false, device_mask, nblocks, in, in_len, raw_len, d_out, out_cap, out_off, status, 0);
}

