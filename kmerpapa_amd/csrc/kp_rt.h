// kp_rt.h -- the host runtime of libkmerpapa_hip.so: the thread's last error, the HIP error
// macro, device allocation helpers, the environment knobs' reader and the device context
// (kp_create / kp_destroy).  Host code only; every other header with C-ABI entry points
// builds on it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/kmerpapa_hip.h"

static thread_local std::string g_err;

static int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define KP_HIP(expr)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return fail(KP_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                 \
    } while (0)

// an integer knob from the environment; unset (or empty) gives the default
static long env_int(const char *name, long unset) {
    const char *e = getenv(name);
    return e && *e ? atol(e) : unset;
}

// Device memory: plain hipMalloc.  On this platform an allocation of HBM that was used
// before (by this or an earlier process) waits for the driver to wipe it, ~30 ms per GB
// (4-6 s for the 150 GB of a 9-mer pass; fresh HBM 0.05 s per 100 GB), so the library
// allocates the large per-lane buffers once (kp_reserve_lanes) and only grows them.  The
// stream-ordered allocator (hipMallocAsync) skips that wait but is not usable: a 140 GB
// request served from a freed 100 GB pool block returned memory that did not hold what
// was written to it (tools/async_check.hip).
template <typename T>
static hipError_t dmalloc(T **p, size_t bytes) {
    return hipMalloc(reinterpret_cast<void **>(p), std::max<size_t>(bytes, 1));
}

template <typename T>
static int upload(T **dptr, const std::vector<T> &v) {
    size_t bytes = std::max<size_t>(1, v.size()) * sizeof(T);
    KP_HIP(dmalloc(dptr, bytes));
    if (!v.empty()) KP_HIP(hipMemcpy(*dptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return KP_OK;
}

static void dfree(void *p) {
    if (p) (void)hipFree(p);
}

static size_t g_up(size_t x) { return (x + 255) & ~(size_t)255; }

// One device allocation carved into buffers, kept between calls and only grown (re-allocating
// used HBM is slow, see dmalloc above).  reserve() starts a new layout of at most `need`
// bytes, take() hands out its next piece rounded up to 256 bytes, check() fails if the
// pieces taken exceed the allocation (nothing may use them before it passed).  `who`
// prefixes the error text.
struct kp_arena {
    void *base = nullptr;
    size_t bytes = 0;
    size_t used = 0;

    int reserve(const char *who, size_t need) {
        used = 0;
        if (bytes >= need) return KP_OK;
        dfree(base);
        base = nullptr;
        bytes = 0;
        if (hipMalloc(&base, need) != hipSuccess) {
            (void)hipGetLastError();
            base = nullptr;
            return fail(KP_E_NOMEM, std::string(who) + ": cannot allocate " + std::to_string(need >> 20) +
                                        " MiB of device memory");
        }
        bytes = need;
        return KP_OK;
    }
    char *take(size_t n_bytes) {
        char *p = static_cast<char *>(base) + used;
        used += g_up(n_bytes);
        return p;
    }
    int check(const char *who) const {
        return used > bytes ? fail(KP_E_PARITY, std::string(who) + ": arena layout exceeds its size") : KP_OK;
    }
};

// One kp_seq_* session (kp_seq.h): the count columns live on the device (d_tab, in the
// context's arena) or, for the host session, in h_tab.  A plain session has one positive column,
// a typed one three (one per ALT slot, kp_spec.h), and so has an indel session (ins, del_start,
// del_end, kp_indel.h).
struct kp_seq_sess {
    bool active = false;
    int k = 0, fold = 0;
    int both = 0;          // every add comes with its mirror on the other strand (kp_seq_begin_strands / _indel)
    bool indel = false;    // an indel session: kp_seq_indels fills the three positive columns
    int pcols = 1;         // positive columns: 1, or 3 in a typed or an indel session
    uint64_t cells = 0;    // 4^k
    uint64_t centres = 0;  // centres of all work items so far (windows + windows_invalid)
    unsigned long long *d_tab = nullptr;   // [pcols + 1][cells]: positive, background
    unsigned long long *d_stat = nullptr;  // windows, sites, sites skipped
    std::vector<uint64_t> h_tab;
    kp_seq_stats st{};
};

// One kp_pred_* session (kp_pred.h): the lookup table from k-mer code to pattern index lives on
// the device (d_lut, first in the context's arena) or, for the host session, in h_lut.  The
// patterns are kept: growing the arena for a call's counters builds the table again.
struct kp_pred_sess {
    bool active = false;
    bool lut_ok = false;  // d_lut holds the table of `pats`
    int k = 0, fold = 0;
    uint64_t cells = 0;  // 4^k
    std::vector<uint64_t> pats;
    int32_t *d_lut = nullptr;
    std::vector<int32_t> h_lut;
    kp_pred_stats st{};
};

// One kp_spec_* session (kp_spec.h): as kp_pred_sess, with one pattern list for every mutation
// type and a table of 16-byte entries {pattern of slot 0, 1, 2, -1} per k-mer code.
struct kp_spec_sess {
    bool active = false;
    bool lut_ok = false;  // d_lut holds the table of `pats`
    int k = 0, fold = 0;
    uint64_t cells = 0;  // 4^k
    std::vector<uint64_t> pats;
    std::vector<uint32_t> ptype;  // [P] 0..11: 3 * code(REF) + slot
    std::vector<uint32_t> by_type;  // [P] the pattern indices grouped by type, ascending within a type
    uint32_t type_off[13] = {};     // by_type[type_off[t] .. type_off[t + 1]) are the patterns of type t
    int32_t *d_lut = nullptr;     // [cells][4]
    std::vector<int32_t> h_lut;
    kp_spec_stats st{};
    kp_spec_sim_stats sim{};  // of the last kp_spec_simulate call (kp_sim.h)
    kp_spec_null_stats null{};  // of the last kp_spec_null call (kp_null.h)
    kp_spec_coding_stats coding{};  // of the last kp_spec_coding call (kp_coding.h)
    kp_spec_coding_null_stats cnull{};  // of the last kp_spec_coding_null call (kp_cnull.h)
};

// One kp_ispec_* session (kp_ispec.h): as kp_spec_sess, with the insertion and the deletion partition
// in one pattern list and a table of 16-byte entries {ins pattern of c, ins pattern of rc(c), del
// pattern of c, del pattern of rc(c)} per k-mer code c.
struct kp_ispec_sess {
    bool active = false;
    bool lut_ok = false;  // d_lut holds the table of `pats`
    int k = 0;
    uint64_t cells = 0;  // 4^k
    std::vector<uint64_t> pats;
    std::vector<uint32_t> pkind;    // [P] 0 ins, 1 del
    std::vector<uint32_t> by_kind;  // [P] the pattern indices grouped by kind, ascending within a kind
    uint32_t kind_off[3] = {};      // by_kind[kind_off[t] .. kind_off[t + 1]) are the patterns of kind t
    int32_t *d_lut = nullptr;       // [cells][4]
    std::vector<int32_t> h_lut;
    kp_ispec_stats st{};
};

#define KP_SIDE_STREAMS 3

struct kp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // side streams: the lane classes of one pass (device groups of different widths, e.g. a
    // 5-lane and a 1-lane group, or the 4 + 3 split of a 7-penalty group) are independent,
    // so each class runs its launch sequence on a stream of its own and the classes overlap
    hipStream_t side[KP_SIDE_STREAMS] = {nullptr, nullptr, nullptr};
    hipEvent_t side_ev[KP_SIDE_STREAMS] = {nullptr, nullptr, nullptr};
    size_t lds_max = 65536;
    int cus = 256;  // compute units (kp_apply's persistent grid)
    // kp_greedy and kp_apply: one device arena, and the partitions of the last kp_greedy
    // call's lanes (kp_greedy_leaves)
    kp_arena arena;
    std::vector<std::vector<uint64_t>> g_leaves;
    kp_greedy_stats g_stats{};  // of the last kp_greedy call
    // kp_seq_*: the session (its table holds the arena until kp_seq_end) and a second
    // allocation, also only grown, for the contig, its work items and the site positions
    kp_seq_sess seq;
    kp_arena seq_in;
    // kp_pred_*: the session (its lookup table holds the arena until kp_pred_end); the contig,
    // work items, regions and site positions go into seq_in
    kp_pred_sess pred;
    // kp_spec_*: the same for a whole mutation spectrum
    kp_spec_sess spec;
    // kp_ispec_*: the same for an indel model
    kp_ispec_sess ispec;
};

// What every genome scan session checks of a contig (kp_seq.h, kp_pred.h, kp_spec.h and the calls of
// a kp_spec session).  `begin_name` opens the session whose `active` this is
static int scan_check_contig(const std::string &w, bool active, const uint8_t *seq, uint64_t n, const char *begin_name) {
    if (!active) return fail(KP_E_STATE, w + ": no session (" + begin_name + " first)");
    if (n && !seq) return fail(KP_E_ARG, w + ": null sequence");
    if (n >= (1ull << 32)) return fail(KP_E_ARG, w + ": a contig of 2^32 bases or more");
    return KP_OK;
}

// a persistent grid: as many workgroups as are resident at once, at most the units and the knob
static uint64_t scan_grid(kp_ctx *c, uint64_t n_units, int per_cu, const char *knob) {
    uint64_t grid = std::min<uint64_t>(n_units, (uint64_t)c->cus * per_cu);
    const long grid_env = env_int(knob, 0);
    if (grid_env > 0) grid = std::min<uint64_t>(grid, (uint64_t)grid_env);
    return grid;
}

extern "C" {

const char *kp_last_error(void) { return g_err.c_str(); }

int kp_device_count(int *n) {
    if (!n) return fail(KP_E_ARG, "null");
    KP_HIP(hipGetDeviceCount(n));
    return KP_OK;
}

int kp_create(int device, kp_ctx **out) {
    if (!out) return fail(KP_E_ARG, "null out");
    int n = 0;
    KP_HIP(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(KP_E_ARG, "device " + std::to_string(device) + " not present");
    KP_HIP(hipSetDevice(device));
    kp_ctx *c = new kp_ctx();
    c->device = device;
    KP_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    for (auto &e : c->ev) KP_HIP(hipEventCreate(&e));
    for (int i = 0; i < KP_SIDE_STREAMS; ++i) {
        KP_HIP(hipStreamCreateWithFlags(&c->side[i], hipStreamNonBlocking));
        KP_HIP(hipEventCreateWithFlags(&c->side_ev[i], hipEventDisableTiming));
    }
    int lds = 0;
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess && lds > 0)
        c->lds_max = (size_t)lds;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->cus = cus;
    *out = c;
    return KP_OK;
}

int kp_device_mem(kp_ctx *c, uint64_t *free_bytes, uint64_t *total_bytes) {
    if (!c) return fail(KP_E_ARG, "null ctx");
    KP_HIP(hipSetDevice(c->device));
    size_t fr = 0, tot = 0;
    KP_HIP(hipMemGetInfo(&fr, &tot));
    if (free_bytes) *free_bytes = fr;
    if (total_bytes) *total_bytes = tot;
    return KP_OK;
}

void kp_destroy(kp_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (auto e : c->ev)
        if (e) (void)hipEventDestroy(e);
    for (int i = 0; i < KP_SIDE_STREAMS; ++i) {
        if (c->side_ev[i]) (void)hipEventDestroy(c->side_ev[i]);
        if (c->side[i]) (void)hipStreamDestroy(c->side[i]);
    }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    dfree(c->arena.base);
    dfree(c->seq_in.base);
    delete c;
}

}  // extern "C"
