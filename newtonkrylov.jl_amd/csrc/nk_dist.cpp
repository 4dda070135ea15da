// nk_dist.cpp -- multi-GPU slab decomposition over RCCL (one process per GPU, xGMI).
//
// The reference has no distributed path; its halo storage pattern is examples/halovector.jl
// (ghost layer around the interior, filled by bc!).  Here the ghost planes of a slab are the
// neighbour ranks' boundary planes, exchanged with grouped ncclSend/ncclRecv before every stencil
// application, and every inner product is completed by an 8-byte ncclAllReduce (the Arnoldi
// scalars are then replicated on all ranks, as the Hessenberg/Givens work is).
#include <fcntl.h>
#include <rccl/rccl.h>
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "nk_internal.hpp"

namespace nk {

struct Comm {
    ncclComm_t comm = nullptr;
};

static int rccl_fail(nk_ctx* c, ncclResult_t r, const char* what) {
    return fail(c, NK_E_RCCL, std::string(what) + ": " + ncclGetErrorString(r));
}

// 3D blocks: rank = (iz py + iy) px + ix; side s = 2 a + hi of axis a = z, y, x (kHaloSides numbering)
int block_nbr(const nk_ctx* c, int side) {
    if (block_self(c)) {  // the self-block rig (NK_HALO_SELF=2): its own neighbour on both sides of every
        // axis in NK_HALO_SELF_AXES (bit 0 z, 1 y, 2 x; default all) -- bench.py --block-of passes the split axes
        static const int axes = env_cfg("NK_HALO_SELF_AXES", 7);
        return (axes >> (side >> 1)) & 1 ? c->rank : -1;
    }
    const int px = c->px, py = c->py, r = c->rank;
    const int ix = r % px, iy = (r / px) % py, iz = r / (px * py), pz = c->nranks / (px * py);
    const int hi = side & 1;
    switch (side >> 1) {
    case 0: return hi ? (iz + 1 < pz ? r + px * py : -1) : (iz > 0 ? r - px * py : -1);
    case 1: return hi ? (iy + 1 < py ? r + px : -1) : (iy > 0 ? r - px : -1);
    default: return hi ? (ix + 1 < px ? r + 1 : -1) : (ix > 0 ? r - 1 : -1);
    }
}

// bc_periodic! (heat_2D.jl:15-26) along the slab axis makes the slabs a ring: the lone slab wraps
// onto itself (a local copy), rank 0's lower neighbour is rank nranks-1 and vice versa.
int halo_exchange(nk_ctx* c, const nk_problem* p, const double* v) {
    const bool ring = p && p->bc == NK_BC_PERIODIC;
    if (!ring && !c->comm && !c->mb_on) return NK_OK;
    Geo g;
    NK_TRY(geometry(c, p, &g));
    double* vv = const_cast<double*>(v);  // only the ghost planes are written
    if (blocks3d(c, g)) {  // 3D blocks: all six ghost layers, through the peer mailbox
        const auto fit = c->faced.find(vv);
        if (fit == c->faced.end()) return fail(c, NK_E_STATE, "3D blocks: a vector allocated before nk_dist_grid has no ghost faces");
        if (face_words(c, p, g) > fit->second)
            return fail(c, NK_E_ARG, "3D blocks: the vector's ghost faces are smaller than this problem's (allocated for another grid)");
        if (!c->mb_on) return fail(c, NK_E_STATE, "3D blocks exchange their ghost faces through the peer mailbox (it is off)");
        const int64_t big = std::max({p->nx * p->ny, p->nx * p->nz, p->ny * p->nz});
        if (big > c->halo_cap) return fail(c, NK_E_ARG, "3D blocks: a ghost face is larger than the IPC inbox (NK_HALO_CAP)");
        return launch_faces_ipc(c, vv, p);
    }
    if (ring && c->nranks <= 1) return launch_periodic_fill(c, vv, g.plane, g.nplanes);
    if (!c->comm && !c->mb_on) return NK_OK;
    if (c->mb_on && g.plane <= c->halo_cap) return launch_halo_ipc(c, vv, g.plane, g.nplanes, ring);
    if (!c->comm) return fail(c, NK_E_ARG, "ghost plane larger than the IPC inbox (NK_HALO_CAP) and no RCCL communicator");
    const size_t pl = (size_t)g.plane;
    const int n = c->nranks;
    const int up = c->rank + 1 < n ? c->rank + 1 : (ring ? 0 : -1);
    const int dn = c->rank > 0 ? c->rank - 1 : (ring ? n - 1 : -1);
    ncclComm_t comm = c->comm->comm;
    if (dn < 0 && up < 0) return NK_OK;  // a lone slab has only physical boundaries
    ncclResult_t r = ncclSuccess;
    auto chk = [&r](ncclResult_t x) {
        if (r == ncclSuccess) r = x;
    };
    // Posting order matters when both neighbours are the same rank (a ring of two): sends go up
    // then down, receives come from below then above, so the FIFO matching per peer pairs my
    // lower ghost with the neighbour's last plane and my upper ghost with its first.
    NK_TRY(launch(c, "halo_rccl", 16.0 * pl * ((dn >= 0) + (up >= 0)), [&] {
        chk(ncclGroupStart());
        if (up >= 0) chk(ncclSend(vv + (size_t)(g.nplanes - 1) * pl, pl, ncclFloat64, up, comm, c->stream));
        if (dn >= 0) chk(ncclSend(vv, pl, ncclFloat64, dn, comm, c->stream));
        if (dn >= 0) chk(ncclRecv(vv - pl, pl, ncclFloat64, dn, comm, c->stream));
        if (up >= 0) chk(ncclRecv(vv + (size_t)g.nplanes * pl, pl, ncclFloat64, up, comm, c->stream));
        chk(ncclGroupEnd());
    }));
    if (r != ncclSuccess) return rccl_fail(c, r, "halo send/recv");
    return NK_OK;
}

int exchange_un(nk_ctx* c, const nk_problem* p) {
    if (!p || !kind_of(p->kind).un || kind_of(p->kind).scheme == 0 || !p->un) return NK_OK;
    return halo_exchange(c, p, p->un);
}

int allreduce_scalar(nk_ctx* c, double* dev, int64_t count) {
    if (!c->comm) return NK_OK;
    ncclResult_t r = ncclSuccess;
    NK_TRY(launch(c, "allreduce", 0.0, [&] {
        r = ncclAllReduce(dev, dev, (size_t)count, ncclFloat64, ncclSum, c->comm->comm, c->stream);
    }));
    if (r != ncclSuccess) return rccl_fail(c, r, "ncclAllReduce");
    return NK_OK;
}

// ---------------------------------------------------------------- peer mailbox (one-shot all-reduce)
// Every reduction scalar goes straight from the producing kernel to every rank's mailbox over
// xGMI (nk_kernels.hip: mb_send / mb_recv); RCCL keeps the halo exchange.  Set up collectively at
// nk_dist_init, verified by a self-test whose verdict all ranks agree on; any failure falls back
// to the RCCL all-reduce.
static size_t mb_region_bytes(int64_t cap) {
    return sizeof(uint64_t) * (kMbWords + kHaloFlagWords) + sizeof(double) * 2 * kHaloSides * (size_t)cap;
}

static int mb_alloc_err(nk_ctx* c) {
    if (c->mb_err) return NK_OK;
    int* h = nullptr;
    NK_HIP(c, hipHostMalloc(&h, 4 * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));
    h[0] = 0;
    NK_HIP(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&c->mb_err_dev), h, 0));
    c->mb_err = h;
    return NK_OK;
}

// my device region: fine-grained device memory whose IPC handle the peers map over xGMI
static int mb_alloc(nk_ctx* c) {
    if (c->mb_dev) return NK_OK;
    NK_HIP(c, hipSetDevice(c->device));
    const char* hc = getenv("NK_HALO_CAP");  // doubles per inbox plane (default 1M: a 1024^2 3D plane)
    c->halo_cap_dev = (hc && *hc) ? atoll(hc) : ((int64_t)1 << 20);
    c->halo_cap_dev = std::max<int64_t>(0, std::min<int64_t>(c->halo_cap_dev, INT32_MAX));  // 32-bit face indexing
    const size_t bytes = mb_region_bytes(c->halo_cap_dev);
    void* p = nullptr;
    if (hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained) != hipSuccess)
        return fail(c, NK_E_NOMEM, "mailbox: fine-grained allocation failed");
    NK_HIP(c, hipMemset(p, 0, bytes));
    c->mb_dev = static_cast<uint64_t*>(p);
    return mb_alloc_err(c);
}

// Host mailbox: the same region layout in a POSIX shared-memory segment, registered with HIP (mapped:
// kernels store to it and poll it with system-scope atomics over PCIe / Infinity Fabric).  Used when a
// peer's device is not visible to this process (a launcher that gives each rank one visible GPU), or
// forced with NK_DIST_MAILBOX=host.  Its ghost-plane inbox is small (NK_HALO_CAP_HOST doubles per plane,
// default 64 Ki): larger planes take RCCL send/recv, while every reduction scalar -- and with it the
// resident MGS sweep's per-pass cross-rank stage -- stays on the mailbox.
struct HostHandle {  // the 64-byte record that stands in for a hipIpcMemHandle_t
    char magic[8];
    char name[40];      // the POSIX shared-memory name (pid, sequence, device and a random nonce)
    uint64_t host;      // the host that owns it (host_identity): a record from another host is refused
    uint64_t bytes;
};
static_assert(sizeof(HostHandle) == 64, "host mailbox handle record");
static const char kHostMagic[8] = {'N', 'K', 'H', 'O', 'S', 'T', 'M', 'B'};
static bool is_host_handle(const char* h) { return std::memcmp(h, kHostMagic, 8) == 0; }
static bool mb_force_host() {
    const char* e = getenv("NK_DIST_MAILBOX");
    return e && std::strcmp(e, "host") == 0;
}

// this host: FNV-1a of the kernel's boot id (a segment name is only meaningful on the kernel -- and the
// boot -- that created it).  The boot id alone: containers of one machine that share /dev/shm
// (--ipc=host) carry different host names but one kernel.  Only where no boot id can be
// read does the host name stand in.
static uint64_t host_identity() {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&h](const char* t, size_t n) {
        for (size_t i = 0; i < n && t[i]; ++i) h = (h ^ (unsigned char)t[i]) * 1099511628211ull;
    };
    char buf[256] = {0};
    bool boot = false;
    if (FILE* f = std::fopen("/proc/sys/kernel/random/boot_id", "r")) {
        boot = std::fgets(buf, sizeof(buf), f) != nullptr && buf[0];
        std::fclose(f);
    }
    if (!boot) {
        std::memset(buf, 0, sizeof(buf));
        if (gethostname(buf, sizeof(buf) - 1) != 0) buf[0] = 0;
    }
    mix(buf, sizeof(buf));
    return h;
}

static uint64_t random_nonce() {
    uint64_t v = 0;
    if (FILE* f = std::fopen("/dev/urandom", "rb")) {
        if (std::fread(&v, sizeof(v), 1, f) != 1) v = 0;
        std::fclose(f);
    }
    return v ^ ((uint64_t)getpid() << 32) ^ (uint64_t)(uintptr_t)&v;
}

static HostHandle host_record(const nk_ctx* c) {
    HostHandle hh{};
    std::memcpy(hh.magic, kHostMagic, 8);
    std::strncpy(hh.name, c->mb_host_name, sizeof(hh.name) - 1);
    hh.host = host_identity();
    hh.bytes = c->mb_host_bytes;
    return hh;
}

// the 64-byte IPC handle of my device region
static int mb_device_record(nk_ctx* c, char out[64]) {
    NK_TRY(mb_alloc(c));
    hipIpcMemHandle_t h;
    NK_HIP(c, hipIpcGetMemHandle(&h, c->mb_dev));
    static_assert(sizeof(h) == 64, "hipIpcMemHandle_t size");
    std::memcpy(out, &h, 64);
    return NK_OK;
}

static int mb_alloc_host(nk_ctx* c) {
    if (c->mb_host_base) return NK_OK;
    NK_HIP(c, hipSetDevice(c->device));
    const char* hc = getenv("NK_HALO_CAP_HOST");
    c->halo_cap_host = (hc && *hc) ? atoll(hc) : ((int64_t)1 << 16);
    c->halo_cap_host = std::max<int64_t>(0, std::min<int64_t>(c->halo_cap_host, INT32_MAX));
    const size_t bytes = mb_region_bytes(c->halo_cap_host);
    static unsigned seq = 0;
    static_assert(sizeof(HostHandle::name) <= sizeof(c->mb_host_name), "host mailbox name");
    std::snprintf(c->mb_host_name, sizeof(HostHandle::name), "/nk_mb_%d_%u_%d_%012llx", (int)getpid(), seq++ % 1000,
                  c->device, (unsigned long long)(random_nonce() & 0xffffffffffffull));
    const int fd = shm_open(c->mb_host_name, O_CREAT | O_EXCL | O_RDWR, 0600);
    if (fd < 0) return fail(c, NK_E_NOMEM, std::string("host mailbox: shm_open failed for ") + c->mb_host_name);
    void* p = MAP_FAILED;
    if (ftruncate(fd, (off_t)bytes) == 0) p = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (p == MAP_FAILED) {
        shm_unlink(c->mb_host_name);
        return fail(c, NK_E_NOMEM, "host mailbox: mapping the shared segment failed");
    }
    std::memset(p, 0, bytes);
    void* d = nullptr;
    if (hipHostRegister(p, bytes, hipHostRegisterMapped) != hipSuccess || hipHostGetDevicePointer(&d, p, 0) != hipSuccess) {
        (void)hipGetLastError();
        munmap(p, bytes);
        shm_unlink(c->mb_host_name);
        return fail(c, NK_E_HIP, "host mailbox: hipHostRegister of the shared segment failed");
    }
    c->mb_host_base = p;
    c->mb_host_bytes = bytes;
    c->mb_host_dev = static_cast<uint64_t*>(d);
    return mb_alloc_err(c);
}

// my region for the next open: the device one (xGMI peers) or the host one
static void mb_use(nk_ctx* c, bool host) {
    c->mb_host = host;
    c->mb_self = host ? c->mb_host_dev : c->mb_dev;
    c->halo_cap = host ? c->halo_cap_host : c->halo_cap_dev;
}

// every peer has mapped my host segment: its name can go (the mappings stay valid)
static void mb_host_unlink(nk_ctx* c) {
    if (c->mb_host_name[0]) shm_unlink(c->mb_host_name);
    c->mb_host_name[0] = 0;
}

static void mb_disable(nk_ctx* c) {
    c->mb_on = false;
    (void)mailbox_bind(c);
    for (void* p : c->mb_opened) (void)hipIpcCloseMemHandle(p);
    c->mb_opened.clear();
    for (auto& m : c->mb_host_maps) {
        (void)hipHostUnregister(m.first);
        munmap(m.first, m.second);
    }
    c->mb_host_maps.clear();
    if (c->mb_peers_dev) (void)hipFree(c->mb_peers_dev);
    c->mb_peers_dev = nullptr;
}

void mb_free(nk_ctx* c) {
    mb_disable(c);
    if (c->mb_dev) (void)hipFree(c->mb_dev);
    c->mb_dev = nullptr;
    if (c->mb_host_base) {
        (void)hipHostUnregister(c->mb_host_base);
        munmap(c->mb_host_base, c->mb_host_bytes);
        mb_host_unlink(c);
    }
    c->mb_host_base = nullptr;
    c->mb_host_dev = nullptr;
    c->mb_self = nullptr;
    if (c->mb_err) (void)hipHostFree(c->mb_err);
    c->mb_err = nullptr;
    c->mb_err_dev = nullptr;
    if (c->mb_wacc) (void)hipFree(c->mb_wacc);
    c->mb_wacc = nullptr;
}

// the region of the two that the agreed mailbox does not use (both when the mailbox is off)
static void mb_free_unused(nk_ctx* c) {
    if ((!c->mb_on || c->mb_host) && c->mb_dev) {
        (void)hipFree(c->mb_dev);
        c->mb_dev = nullptr;
    }
    if ((!c->mb_on || !c->mb_host) && c->mb_host_base) {
        (void)hipHostUnregister(c->mb_host_base);
        munmap(c->mb_host_base, c->mb_host_bytes);
        mb_host_unlink(c);
        c->mb_host_base = nullptr;
        c->mb_host_dev = nullptr;
    }
}

// map a peer's host segment: its device address for my kernels
static int mb_map_host_peer(nk_ctx* c, int r, const char* rec, uint64_t** out) {
    HostHandle h;
    std::memcpy(&h, rec, sizeof(h));
    h.name[sizeof(h.name) - 1] = 0;
    if (h.host != host_identity())  // another host's (or boot's) segment name: never open it here
        return fail(c, NK_E_ARG, "host mailbox: rank " + std::to_string(r) + " runs on another host");
    const int fd = shm_open(h.name, O_RDWR, 0600);
    if (fd < 0) return fail(c, NK_E_HIP, "host mailbox: rank " + std::to_string(r) + "'s segment cannot be opened");
    void* p = mmap(nullptr, h.bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (p == MAP_FAILED) return fail(c, NK_E_HIP, "host mailbox: rank " + std::to_string(r) + "'s segment cannot be mapped");
    void* d = nullptr;
    if (hipHostRegister(p, h.bytes, hipHostRegisterMapped) != hipSuccess || hipHostGetDevicePointer(&d, p, 0) != hipSuccess) {
        (void)hipGetLastError();
        munmap(p, h.bytes);
        return fail(c, NK_E_HIP, "host mailbox: rank " + std::to_string(r) + "'s segment cannot be registered");
    }
    c->mb_host_maps.emplace_back(p, (size_t)h.bytes);
    *out = static_cast<uint64_t*>(d);
    return NK_OK;
}

// open the peers' mailboxes (local: IPC mappings + device table + kernel binding).  busids (optional,
// nranks x 32 chars): each rank's PCI bus id -- a peer on another device must be reachable by
// peer access (xGMI), and every mapping is probed by a host-initiated copy before any kernel
// dereferences it, so a bad mapping disables the mailbox (RCCL fallback) instead of faulting a kernel.
static int mb_open_peers(nk_ctx* c, int rank, int nranks, const char* handles, const char* busids = nullptr) {
    const bool host = is_host_handle(handles + 64 * (size_t)rank);  // my own record names the mode
    NK_TRY(host ? mb_alloc_host(c) : mb_alloc(c));
    mb_disable(c);
    mb_use(c, host);
    std::vector<uint64_t*> peers((size_t)nranks);
    // the resident MGS sweep needs every CU of its grid co-resident: with peers on the same device
    // (no bus ids: the mailbox-only transport, made for ranks on one GPU -- all of them count) it is
    // off, unless NK_RES_SHARED=1 (test rigs) gives every rank's sweep grid CUs / (ranks on the GPU)
    const bool shared_ok = env_cfg("NK_RES_SHARED", 0) != 0;
    int share = busids ? 1 : nranks;
    for (int r = 0; r < nranks; ++r) {
        if (r == rank) {
            peers[r] = c->mb_self;
            continue;
        }
        if (host) {  // host shared memory: reachable from any device, no peer access needed
            if (busids) {
                char bus[33];
                std::memcpy(bus, busids + 32 * (size_t)r, 32);
                bus[32] = 0;
                int dev = -1;
                if (hipDeviceGetByPCIBusId(&dev, bus) == hipSuccess && dev == c->device) ++share;
                else (void)hipGetLastError();
            }
            if (!is_host_handle(handles + 64 * (size_t)r)) {
                mb_disable(c);
                return fail(c, NK_E_ARG, "mailbox: ranks disagree on host / device mailboxes");
            }
            uint64_t* p = nullptr;
            if (mb_map_host_peer(c, r, handles + 64 * (size_t)r, &p) != NK_OK) {
                mb_disable(c);
                return NK_E_HIP;
            }
            peers[r] = p;
            continue;
        }
        if (busids) {
            char bus[33];
            std::memcpy(bus, busids + 32 * (size_t)r, 32);
            bus[32] = 0;
            int dev = -1;
            if (hipDeviceGetByPCIBusId(&dev, bus) != hipSuccess) {
                mb_disable(c);
                return fail(c, NK_E_HIP, "mailbox: rank " + std::to_string(r) + "'s device is not visible here");
            }
            if (dev == c->device) ++share;
            if (dev != c->device) {
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, c->device, dev) != hipSuccess || !can) {
                    mb_disable(c);
                    return fail(c, NK_E_HIP, "mailbox: no peer access to rank " + std::to_string(r) + "'s device");
                }
            }
        }
        hipIpcMemHandle_t h;
        std::memcpy(&h, handles + 64 * (size_t)r, 64);
        void* p = nullptr;
        if (hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
            mb_disable(c);
            return fail(c, NK_E_HIP, "mailbox: hipIpcOpenMemHandle failed for rank " + std::to_string(r));
        }
        c->mb_opened.push_back(p);
        uint64_t probe = 0;
        if (hipMemcpy(&probe, p, sizeof(probe), hipMemcpyDeviceToHost) != hipSuccess) {
            (void)hipGetLastError();
            mb_disable(c);
            return fail(c, NK_E_HIP, "mailbox: rank " + std::to_string(r) + "'s mapping cannot be read");
        }
        peers[r] = static_cast<uint64_t*>(p);
    }
    c->res_share = share;
    c->res_ok = share < 2 || shared_ok;
    // the most ranks on any one GPU, from the same gathered bus ids on every rank (all ranks, no bus ids:
    // assume they share): ranks sharing a GPU spin in their exchange kernels together, and all of those
    // grids must be resident at once -- at 256 blocks x 4 waves, 8 sharing ranks would fill the GPU
    int most = busids ? 1 : nranks;
    for (int r = 0; busids && r < nranks; ++r) {
        int cnt = 0;
        for (int q = 0; q < nranks; ++q) cnt += std::memcmp(busids + 32 * (size_t)r, busids + 32 * (size_t)q, 32) == 0;
        most = std::max(most, cnt);
    }
    c->share_most = most;
    c->xchg_nb = std::max(16, kHaloBlocks / std::max(1, most));
    NK_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->mb_peers_dev), sizeof(uint64_t*) * nranks));
    NK_HIP(c, hipMemcpy(c->mb_peers_dev, peers.data(), sizeof(uint64_t*) * nranks, hipMemcpyHostToDevice));
    *c->mb_err = 0;
    c->mb_on = true;
    return mailbox_bind(c);
}

// a rank whose mailbox is not open still waits out the self-test's timeout on the others: every
// rank reaches the collective verdict, nobody hangs
// one ring exchange of a small 2-plane grid function whose planes hold (rank, plane, index) codes:
// every ghost plane must hold exactly the neighbour's boundary plane
static bool halo_selftest(nk_ctx* c) {
    if (c->nranks < 2) return true;
    constexpr int64_t pl = 300, np = 2;  // 300 doubles: several blocks of the exchange kernel
    double* base = nullptr;
    if (hipMalloc(&base, sizeof(double) * pl * (np + 2)) != hipSuccess) return false;
    std::vector<double> h((size_t)(pl * (np + 2)), -1.0);
    auto code = [](int r, int64_t k, int64_t i) { return 1e6 * (r + 1) + 1e3 * (double)k + (double)i; };
    for (int64_t k = 0; k < np; ++k)
        for (int64_t i = 0; i < pl; ++i) h[(size_t)((k + 1) * pl + i)] = code(c->rank, k, i);
    bool ok = hipMemcpy(base, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice) == hipSuccess &&
              launch_halo_ipc(c, base + pl, pl, np, true) == NK_OK && hipStreamSynchronize(c->stream) == hipSuccess &&
              hipMemcpy(h.data(), base, sizeof(double) * h.size(), hipMemcpyDeviceToHost) == hipSuccess &&
              !*c->mb_err;
    const int lo = (c->rank + c->nranks - 1) % c->nranks, hi = (c->rank + 1) % c->nranks;
    for (int64_t i = 0; ok && i < pl; ++i)
        ok = h[(size_t)i] == code(lo, np - 1, i) && h[(size_t)((np + 1) * pl + i)] == code(hi, 0, i);
    (void)hipFree(base);
    return ok;
}

// min over ranks of a local success flag (RCCL; a context without a communicator decides alone).  Every
// rank always enters the all-reduce -- a local failure contributes 0 -- so no peer is left in it alone.
static bool all_ranks_ok(nk_ctx* c, bool local_ok) {
    if (!c->comm) return local_ok;
    double v = local_ok ? 1.0 : 0.0;
    bool wrote = hipMemcpy(c->scal, &v, sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    if (!wrote) {
        (void)hipGetLastError();
        (void)hipMemsetAsync(c->scal, 0, sizeof(double), c->stream);  // 0.0: this rank is not ok
    }
    if (ncclAllReduce(c->scal, c->scal, 1, ncclFloat64, ncclMin, c->comm->comm, c->stream) != ncclSuccess) return false;
    if (hipMemcpyAsync(c->hpin, c->scal, sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return false;
    return wrote && c->hpin[0] == 1.0;
}

static int mb_verdict(nk_ctx* c, bool local_ok) {
    bool ok = local_ok;
    if (c->mb_on) {
        bool t = false;
        if (mailbox_selftest(c, &t) != NK_OK) t = false;
        ok = ok && t && halo_selftest(c);  // reductions and ghost planes through the peer mappings
    }
    if (c->comm) {  // all ranks must take the same path: min over ranks
        double v = ok ? 1.0 : 0.0;
        NK_HIP(c, hipMemcpy(c->scal, &v, sizeof(double), hipMemcpyHostToDevice));
        if (ncclAllReduce(c->scal, c->scal, 1, ncclFloat64, ncclMin, c->comm->comm, c->stream) != ncclSuccess) v = 0.0;
        else {
            NK_HIP(c, hipMemcpyAsync(c->hpin, c->scal, sizeof(double), hipMemcpyDeviceToHost, c->stream));
            NK_HIP(c, hipStreamSynchronize(c->stream));
            v = c->hpin[0];
        }
        ok = ok && v == 1.0;
    }
    if (c->mb_err) *c->mb_err = 0;
    if (!ok) {
        mb_disable(c);
        return fail(c, NK_E_RCCL, "peer mailbox self-test failed (values did not arrive)");
    }
    return NK_OK;
}

}  // namespace nk

using namespace nk;

extern "C" {

int nk_dist_unique_id(char out[128]) {
    if (!out) return NK_E_ARG;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return NK_E_RCCL;
    static_assert(sizeof(id.internal) == 128, "ncclUniqueId size");
    std::memcpy(out, id.internal, 128);
    return NK_OK;
}

int nk_dist_init(nk_ctx* c, int32_t rank, int32_t nranks, const char id[128]) {
    if (!c || !id || nranks < 1 || rank < 0 || rank >= nranks) return NK_E_ARG;
    if (c->comm) return fail(c, NK_E_STATE, "context already distributed");
    const char* force = getenv("NK_DIST_FORCE");  // 1-rank communicator: exercises the RCCL path on one GPU
    if (nranks == 1 && !(force && *force == '1')) {
        c->rank = 0;
        c->nranks = 1;
        return NK_OK;
    }
    ncclUniqueId uid;
    std::memcpy(uid.internal, id, 128);
    NK_HIP(c, hipSetDevice(c->device));
    Comm* cm = new Comm();
    ncclResult_t r = ncclCommInitRank(&cm->comm, nranks, uid, rank);
    if (r != ncclSuccess) {
        delete cm;
        return rccl_fail(c, r, "ncclCommInitRank");
    }
    c->comm = cm;
    c->rank = rank;
    c->nranks = nranks;
    const char* mbe = getenv("NK_DIST_MAILBOX");
    // one-shot peer all-reduce of the scalars: on by default with several ranks; NK_DIST_MAILBOX=1
    // also turns it on for a forced 1-rank communicator (exercises the path on one GPU), =0 off
    const bool mb_want = (mbe && *mbe == '1') || (nranks > 1 && !(mbe && *mbe == '0'));
    if (mb_want && nranks <= kMbRanks) {
        // per rank: 64-byte IPC handle of the device region, 32-byte PCI bus id of its device, 64-byte
        // record of the host region (the fallback when a peer's device is not visible here), and this
        // rank's NK_DIST_MAILBOX=host vote (one rank asking for the host mailbox moves all of them: the
        // choice is agreed through this allgather, never taken from one rank's environment alone)
        constexpr size_t kRec = 168;
        std::vector<char> all(kRec * nranks, 0);
        // the exchange buffer is the context's reduction scratch (allocated at nk_ctx_create), so no
        // rank can fail an allocation here and leave the others alone in the collectives below
        static_assert(kRec * kMbRanks <= sizeof(double) * kRedCap, "handle records fit one reduction slot");
        char* dbuf = reinterpret_cast<char*>(c->red);
        const bool force_host_here = mb_force_host();
        int rc = NK_OK;
        // (the device handle is always produced: whether to use it is decided after the allgather)
        rc = mb_device_record(c, all.data() + kRec * (size_t)rank);  // (device region)
        if (rc == NK_OK && hipDeviceGetPCIBusId(all.data() + kRec * (size_t)rank + 64, 32, c->device) != hipSuccess)
            rc = NK_E_HIP;
        int rch = mb_alloc_host(c);
        if (rch == NK_OK) {
            const HostHandle hh = host_record(c);
            std::memcpy(all.data() + kRec * (size_t)rank + 96, &hh, sizeof(hh));
        }
        all[kRec * (size_t)rank + 160] = force_host_here ? 1 : 0;
        // allgather the IPC handles: collective, every rank takes part whatever its local state
        (void)hipMemcpy(dbuf + kRec * (size_t)rank, all.data() + kRec * (size_t)rank, kRec, hipMemcpyHostToDevice);
        const ncclResult_t ag = ncclAllGather(dbuf + kRec * (size_t)rank, dbuf, kRec, ncclChar, cm->comm, c->stream);
        if (ag != ncclSuccess || hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(all.data(), dbuf, all.size(), hipMemcpyDeviceToHost) != hipSuccess)
            rc = NK_E_RCCL;
        if (ag != ncclSuccess) {
            // still join the verdict's all-reduce (the other ranks are in it), then report the failure
            (void)mb_verdict(c, false);
            mb_host_unlink(c);
            return rccl_fail(c, ag, "ncclAllGather (mailbox handles)");
        }
        bool force_host = false;
        for (int r = 0; r < nranks; ++r) force_host = force_host || all[kRec * (size_t)r + 160] != 0;
        std::vector<char> handles(64 * (size_t)nranks), hhandles(64 * (size_t)nranks), busids(32 * (size_t)nranks);
        for (int r = 0; r < nranks; ++r) {
            std::memcpy(handles.data() + 64 * (size_t)r, all.data() + kRec * (size_t)r, 64);
            std::memcpy(busids.data() + 32 * (size_t)r, all.data() + kRec * (size_t)r + 64, 32);
            std::memcpy(hhandles.data() + 64 * (size_t)r, all.data() + kRec * (size_t)r + 96, 64);
        }
        // the device regions over xGMI when every rank can map every peer's; else (all ranks together)
        // the host regions
        if (!force_host && rc == NK_OK) rc = mb_open_peers(c, rank, nranks, handles.data(), busids.data());
        // (all_ranks_ok is entered by every rank unless the agreed vote skips it on every rank alike)
        if (force_host || !all_ranks_ok(c, rc == NK_OK)) {
            if (!force_host)
                std::fprintf(stderr, "[nkhip] rank %d: device mailboxes not reachable by every rank (%s); host mailbox\n",
                             rank, c->err.c_str());
            c->err.clear();
            mb_disable(c);
            rc = rch == NK_OK ? mb_open_peers(c, rank, nranks, hhandles.data(), busids.data()) : rch;
        }
        if (mb_verdict(c, rc == NK_OK) != NK_OK) {
            std::fprintf(stderr, "[nkhip] rank %d: peer mailbox off (%s); reductions use ncclAllReduce\n", rank,
                         c->err.c_str());
            c->err.clear();
        }
        mb_host_unlink(c);  // every rank has mapped it (or gave up) by the verdict
        // past the verdict no peer maps the region this rank does not use (device mappings are closed
        // before any rank opens the host ones): free it (96 MiB of fine-grained memory)
        mb_free_unused(c);
    }
    return NK_OK;
}

int nk_dist_mailbox_handle(nk_ctx* c, char out[64]) {
    if (!c || !out) return NK_E_ARG;
    if (mb_force_host() && !c->comm) {  // the mailbox-only transport in host memory (NK_DIST_MAILBOX=host)
        NK_TRY(mb_alloc_host(c));
        const HostHandle hh = host_record(c);
        std::memcpy(out, &hh, sizeof(hh));
        return NK_OK;
    }
    return mb_device_record(c, out);
}

int nk_dist_mailbox_open(nk_ctx* c, int32_t rank, int32_t nranks, const char* handles) {
    if (!c || !handles || nranks < 1 || nranks > kMbRanks || rank < 0 || rank >= nranks) return NK_E_ARG;
    if (c->comm) return fail(c, NK_E_STATE, "nk_dist_init already set up the mailbox of this context");
    c->rank = rank;  // mailbox-only (no RCCL communicator): reductions across ranks, no halo exchange
    c->nranks = nranks;
    const int rc = mb_open_peers(c, rank, nranks, handles);
    const int v = mb_verdict(c, rc == NK_OK);
    mb_host_unlink(c);  // (host mode) every rank has mapped it by the self-test's end
    return v;
}

int nk_dist_mailbox_active(nk_ctx* c) { return (c && c->mb_on) ? 1 : 0; }

int nk_dist_grid(nk_ctx* c, int32_t px, int32_t py, int32_t pz) {
    if (!c || px < 1 || py < 1 || pz < 1) return NK_E_ARG;
    if ((int64_t)px * py * pz != c->nranks)
        return fail(c, NK_E_ARG, "nk_dist_grid: px * py * pz must equal the number of ranks");
    if (!c->allocs.empty() && (px * py > 1) != (c->px * c->py > 1))
        return fail(c, NK_E_STATE, "nk_dist_grid: set the process grid before allocating vectors");
    c->px = px;
    c->py = py;
    return NK_OK;
}

int nk_dist_path(nk_ctx* c, nk_path_info* out) {
    if (!c || !out) return NK_E_ARG;
    std::memset(out, 0, sizeof(*out));
    out->rank = c->rank;
    out->nranks = c->nranks;
    out->device = c->device;
    out->ranks_on_device = c->res_share;
    out->rccl = c->comm ? 1 : 0;
    out->mailbox = c->mb_on ? (c->mb_host ? 2 : 1) : 0;
    // what RAN, from the launches the context counted (not what the configuration would allow)
    out->resident_sweep = c->n_sweep_resident > 0 ? 1 : 0;
    out->resident_blocks = c->res_gran ? c->res_blocks : 0;
    out->halo_in_launch = (c->n_jv_halo_fused > 0 && c->n_jv_halo_separate == 0) ? 1 : 0;
    out->jv_halo_fused = c->n_jv_halo_fused;
    out->jv_halo_separate = c->n_jv_halo_separate;
    out->sweeps_resident = c->n_sweep_resident;
    out->mgs_passes = c->n_mgs_pass;
    out->mailbox_error = (c->mb_err && *(volatile int*)c->mb_err) ? 1 : 0;
    out->jv_fd_f0r = c->n_fd_f0r;
    out->jv_fd_f0_read = c->n_fd_f0_read;
    if (c->mb_wacc) {  // the device's peer-wait counters (after the work enqueued so far)
        unsigned long long w[4] = {0, 0, 0, 0};
        NK_HIP(c, hipStreamSynchronize(c->stream));
        NK_HIP(c, hipMemcpy(w, c->mb_wacc, sizeof(w), hipMemcpyDeviceToHost));
        int khz = 0;  // the device wall clock's rate
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) != hipSuccess || khz <= 0) {
            (void)hipGetLastError();
            khz = 100000;  // 100 MHz, the gfx9 constant
        }
        out->halo_waits = (int64_t)w[1];
        out->reduce_waits = (int64_t)w[3];
        out->halo_wait_us = 1e3 * (double)w[0] / khz;
        out->reduce_wait_us = 1e3 * (double)w[2] / khz;
    }
    out->halo_cap = c->halo_cap;
    if (hipDeviceGetPCIBusId(out->pci_bus_id, (int)sizeof(out->pci_bus_id), c->device) != hipSuccess) {
        (void)hipGetLastError();
        out->pci_bus_id[0] = 0;
    }
    return NK_OK;
}

int nk_dist_free(nk_ctx* c) {
    if (c) mb_free(c);
    if (!c || !c->comm) return NK_OK;
    ncclCommDestroy(c->comm->comm);
    delete c->comm;
    c->comm = nullptr;
    c->nranks = 1;
    c->rank = 0;
    return NK_OK;
}

int nk_dist_allreduce_sum(nk_ctx* c, double* dev_buf, int64_t count) {
    if (!c || !dev_buf || count < 0) return NK_E_ARG;
    return allreduce_scalar(c, dev_buf, count);
}

int nk_halo_exchange(nk_ctx* c, const nk_problem* p, double* v) {
    if (!c || !v) return NK_E_ARG;
    return halo_exchange(c, p, v);
}

}  // extern "C"
