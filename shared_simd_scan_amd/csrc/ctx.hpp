// ctx.hpp -- the context object behind include/mi355_scan.h and what every host-side translation unit of libmi355scan.so
// shares (context.hip, which defines the helpers declared here, capi.hip, extras.hip, comm.hip and the feature units of the
// Makefile's FEATURES table): error reporting, the entry prologue, the context's buffers.
// MI355_ENTER and MI355_LAUNCH (dispatch.hpp) are all an entry point owes the context: the lock, the bound device, the launch record and,
// through the record, the Infinity Cache's repeat state (llc_repeat.hpp), which no launcher but the eq / range path of capi.hip mentions.
#pragma once

#include "../../include/mi355_scan.h"
#include "llc_repeat.hpp"

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace mi355 {
constexpr int kKeySlots = 8; // slots of the upload ring (context.hip upload_list)
}

struct mi355_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int num_cus = 256;
    int max_blocks_per_cu = 0;
    int scan_nt_stores = -1; // -1: by bitmap size (see width_group.hip), 0 plain, 1 non-temporal
    int shared_vpl = 0;  // 0: engine's choice
    int select_kernel = 0; // mi355_scan_select_dev: 1 = the older single-role kernel (A/B); 0 and 2 = decoder / expander roles (select2_kernel)
    int grid_cus = 0;      // persistent grids sized as if the device had this many CUs (tests: long per-wave loops); 0 = num_cus
    unsigned kernel_flags = 0; // experiment switches handed to the kernels (ScanArgs::flags)
    // mi355_tune_dev: blocks per CU measured on THIS device for the large streaming launches; key = tune_key() in capi.hip
    std::map<uint32_t, int> tuned_bpc;
    int scan_burst = 0;  // 0: tiles per store burst by width; 1: one tile per burst
    int llc_resident_mib = -1; // eq / range scan: MiB of Infinity Cache for the part of the column read with the default policy; -1 auto, 0 off
    mi355::LlcRepeat llc; // is an eq / range scan a repeat (auto acts on repeats only), and mi355_ctx_last_llc_divisor: llc_repeat.hpp decides, from the launch record
    int dma_aux = 18; // bits 0-3: policy of the HBM->LDS loads (2 = non-temporal: the column is streamed once);
                      // bit 4: non-temporal stores in decompress
    // Every entry point that touches the state below holds `mu` while it does (the host-pointer flavours from their
    // first copy to their final synchronisation), so one context may be shared by several host threads; contexts are
    // independent of each other.  Recursive: the host-pointer flavours call the *_dev ones.
    std::recursive_mutex mu;
    unsigned long long *hits_scratch = nullptr; // host-pointer API: where the kernels deliver hit counts
    unsigned long long *kernel_scratch = nullptr; // kScratchWords words, all zero between launches (kernels.hpp hits_finalize)
    // key lists (and predicate lists of the shared where-scans) longer than 8 travel through device memory: a ring of
    // kKeySlots pinned host slots and device slots of 3 x (1024 + 8) dwords each -- 1024 + 8 keys, or as many (lo, span,
    // negate) predicate triples -- so uploading a list never waits for the stream (only for the copy that used the slot
    // kKeySlots calls ago)
    int32_t *keys_scratch = nullptr;            // device: kKeySlots x 3 x (1024 + 8) dwords
    int32_t *keys_pinned = nullptr;             // host (pinned): the same
    hipEvent_t key_events[mi355::kKeySlots] = {};
    bool key_used[mi355::kKeySlots] = {};
    int key_next = 0;
    hipEvent_t order_event = nullptr;           // mi355_ctx_set_stream: new stream waits for the old one
    unsigned long long *rowid_ws = nullptr;     // chunk counts of mi355_bitmap_to_rowids_dev / mi355_scan_select_dev / mi355_compact_dev / mi355_top_k_dev
    size_t rowid_ws_entries = 0;
    // Graph capture: a captured memset / kernel node keeps the address of the workspace or pool slot it was recorded with.  A
    // buffer used under capture is marked; when it has to grow later it is retired (freed in mi355_ctx_destroy) instead of freed,
    // so a graph stays valid for as long as its context lives.
    bool rowid_ws_in_graph = false;
    std::vector<void *> retired;
    // host-pointer (drop-in) flavours: grow-only device buffers kept between calls -- no hipMalloc / hipFree per call
    enum { kPoolIn = 0, kPoolOut = 1, kPoolAux = 2, kPoolSlots = 3 };
    void *pool[kPoolSlots] = {};
    size_t pool_bytes[kPoolSlots] = {};
    bool pool_in_graph[kPoolSlots] = {};
    bool is_thread_default = false;
    // mi355_ctx_last_launch: the kernels the most recent compute entry point launched (dispatch.hpp note_launch), cleared when
    // the outermost such call starts (host-pointer flavours and compound calls nest)
    std::string last_launch;
    int call_depth = 0;
};

namespace mi355 {

int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
const char *last_error();

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return ::mi355::fail(MI355_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// a context is bound to one device: make it current for this thread before touching it.  Called by the prologue below, and
// by the two calls that need the device current without being a compute call (mi355_ctx_set_stream, mi355_comm_create).
int bind(mi355_ctx *ctx);
// ctx == NULL -> the calling thread's default context (device 0, the null stream), created on first use and destroyed when
// the thread exits.  Only the prologue calls it.
int resolve(mi355_ctx *&ctx);

// ---- the prologue of every entry point that takes a context ----
// Locked: resolves the default context and holds the context's lock.  On its own it is the prologue of the accessors, which
// neither touch the device nor start a launch record.
struct Locked {
    int rc;
    mi355_ctx *ctx = nullptr;
    explicit Locked(mi355_ctx *&c) : rc(resolve(c))
    {
        if (rc) return;
        ctx = c;
        ctx->mu.lock();
    }
    ~Locked() { if (ctx) ctx->mu.unlock(); }
    Locked(const Locked &) = delete;
    Locked &operator=(const Locked &) = delete;
};

// Entry, through MI355_ENTER(ctx) as an entry point's first line: Locked, then the outermost call on this context (the
// host-pointer flavours, the compound calls and the sharded scans call other entry points with the lock held) starts a new launch
// record (telling llc_repeat.hpp first what the call before left in it) and makes the context's device current.  Nested calls bind nothing: the outermost one did.  kKeepRecord: the memory
// helpers and mi355_ctx_synchronize, which queue work on the context's stream but launch nothing -- the record of the last
// compute call stays readable behind them.
struct Entry : Locked {
    enum Record { kNewRecord, kKeepRecord };
    explicit Entry(mi355_ctx *&c, Record record = kNewRecord) : Locked(c), counted(!rc && record == kNewRecord)
    {
        if (rc) return;
        const bool outermost = ctx->call_depth == 0;
        if (counted) ctx->call_depth++;
        if (!outermost) return;
        if (counted) ctx->llc.call_begins(ctx->last_launch.size()), ctx->last_launch.clear(); // (did the call before end with an eq / range scan?)
        rc = bind(ctx);
    }
    ~Entry() { if (counted) ctx->call_depth--; }
    const bool counted;
};
#define MI355_ENTER(...)                \
    ::mi355::Entry entry_(__VA_ARGS__); \
    if (entry_.rc) return entry_.rc

// Is `stream` being captured into a graph?  The one capture check of the library.  kCaptureUnknown: the runtime would not say
// (e.g. the null stream while another stream captures in global mode); whoever is about to synchronise, allocate, free or copy
// from host memory treats that as kCaptureOn and refuses -- being wrong the other way invalidates somebody's capture.
// *id (nullable) gets the capture's id, 0 unless kCaptureOn.
enum CaptureState { kCaptureOff = 0, kCaptureOn = 1, kCaptureUnknown = 2 };
CaptureState capture_state(hipStream_t stream, unsigned long long *id = nullptr);
inline CaptureState capture_state(mi355_ctx *ctx, unsigned long long *id = nullptr) { return capture_state(ctx->stream, id); }

// ---- the context's buffers (context.hip); the caller holds ctx->mu ----
// grow-only device buffer of the context (host-pointer flavours, temporaries of compound calls)
int pool_get(mi355_ctx *ctx, int slot, size_t bytes, void **out);
// the selection workspace holds at least `entries` words (grown outside capture only; kept alive once a graph points at it)
int rowid_ws_get(mi355_ctx *ctx, uint64_t entries, const char *what);
// A list of P elements of elem_bytes (at most 12: a key, or a (lo, span, negate) triple; P <= kMaxKeys) -> device memory,
// padded to a multiple of 8 elements with copies of the last, asynchronously on the stream, through the ring of kKeySlots
// pinned / device slots.  `what`: the refusal under capture.
int upload_list(mi355_ctx *ctx, const void *src, size_t elem_bytes, unsigned P, const char *what, const void **dev);

// CUs the persistent grids are sized for (option "grid_cus")
inline int grid_cus(const mi355_ctx *ctx) { return ctx->grid_cus > 0 ? ctx->grid_cus : ctx->num_cus; }

// What a launcher outside the width groups (a feature unit of the Makefile's FEATURES table) takes from its context; the groups'
// LaunchReq has the same five among its fields (capi.hip fill_common).
struct LaunchEnv {
    hipStream_t stream;
    int device, num_cus, max_blocks_per_cu; // num_cus: grid_cus(); max_blocks_per_cu: 0 = no cap
    std::string *record;                    // mi355_ctx_last_launch
};
inline LaunchEnv launch_env(mi355_ctx *ctx) { return {ctx->stream, ctx->device, grid_cus(ctx), ctx->max_blocks_per_cu, &ctx->last_launch}; }

} // namespace mi355
