// capi.hip -- implementation of include/mi355_scan.h and include/mi355_columns.h (the C ABI of libmi355scan.so).
//
// Host-side plumbing only: argument checks, device buffers, stream ordering, kernel dispatch by
// width.  All arithmetic of the path happens in the HIP kernels of kernels.hpp; there is no CPU
// implementation of any operation in this library.
#include "ctx.hpp"

#include <cstdlib>
#include <cstring>
#include <vector>

#include "dispatch.hpp"
#include "launch_util.hpp"
#include "shared_plan.hpp"
#include "predicates/where_dispatch.hpp"
#include "predicates/columns_dispatch.hpp"
#include "../../include/mi355_columns.h"
#include "extras/gather.hpp"
#include "kernels.hpp"
#include "extras/aggregate.hpp"
#include "extras/histogram.hpp"

using namespace mi355;

namespace mi355 {

namespace {
thread_local std::string g_err;

// The default context is per THREAD: the reference's functions are stateless and re-entrant (its own
// shared_scan_128_threaded calls scan_128 from an OpenMP loop, src/simd_scan_shared.cpp:25-32), so the drop-in path
// (ctx == NULL everywhere in include/simd_scan.hpp) must be callable from several host threads at once.  Each thread
// gets its own context -- own hit-count scratch, kernel scratch, key ring, device-buffer pool -- on device 0 and the
// null stream; it is destroyed when the thread exits.
struct ThreadDefault {
    mi355_ctx *ctx = nullptr;
    ~ThreadDefault()
    {
        if (ctx) {
            mi355_ctx *c = ctx;
            ctx = nullptr;
            (void)mi355_ctx_destroy(c);
        }
    }
};
thread_local ThreadDefault t_default;
} // namespace

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

const char *last_error() { return g_err.c_str(); }

int resolve(mi355_ctx *&ctx)
{
    if (ctx) return MI355_OK;
    if (!t_default.ctx) {
        int rc = mi355_ctx_create(0, nullptr, &t_default.ctx);
        if (rc != MI355_OK) return rc;
        t_default.ctx->is_thread_default = true;
    }
    ctx = t_default.ctx;
    return MI355_OK;
}

int bind(mi355_ctx *ctx)
{
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != ctx->device) {
        hipError_t e = hipSetDevice(ctx->device);
        if (e != hipSuccess) return fail(MI355_E_HIP, "hipSetDevice(%d): %s", ctx->device, hipGetErrorString(e));
    }
    return MI355_OK;
}

// Is `stream` being captured into a graph?  The one capture check of this file.  kCaptureUnknown: the runtime would not say
// (e.g. the null stream while another stream captures in global mode); whoever is about to synchronise, allocate, free or copy
// from host memory treats that as kCaptureOn and refuses -- being wrong the other way invalidates somebody's capture.
// *id (nullable) gets the capture's id, 0 unless kCaptureOn.
enum CaptureState { kCaptureOff = 0, kCaptureOn = 1, kCaptureUnknown = 2 };
CaptureState capture_state(hipStream_t stream, unsigned long long *id = nullptr)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    unsigned long long cid = 0;
    if (id) *id = 0;
    if (hipStreamGetCaptureInfo(stream, &cap, &cid) != hipSuccess) {
        (void)hipGetLastError(); // the query's own error is not the caller's to report
        return kCaptureUnknown;
    }
    if (cap == hipStreamCaptureStatusNone) return kCaptureOff;
    if (id) *id = cid;
    return kCaptureOn;
}
inline CaptureState capture_state(mi355_ctx *ctx, unsigned long long *id = nullptr) { return capture_state(ctx->stream, id); }

// Growing a buffer of the context synchronises, frees and allocates: none of that may happen on a capturing stream (it would
// invalidate the capture), so it is refused there.  A buffer that a captured node points at (`*in_graph`) is never freed
// while the context lives -- a graph stays valid until its context is destroyed -- but retired to ctx->retired.
int grow_buffer(mi355_ctx *ctx, void **buf, size_t *have, bool *in_graph, size_t want, const char *what)
{
    if (capture_state(ctx) != kCaptureOff)
        return fail(MI355_E_INVALID, "%s: workspace must grow: call once outside capture first (graph capture in progress)", what);
    // whatever still uses the old buffer is ordered on the context's stream
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (*buf) {
        if (*in_graph)
            ctx->retired.push_back(*buf);
        else
            HIP_TRY(hipFree(*buf));
    }
    *buf = nullptr;
    *have = 0;
    *in_graph = false;
    HIP_TRY(hipMalloc(buf, want));
    *have = want;
    return MI355_OK;
}

int pool_get(mi355_ctx *ctx, int slot, size_t bytes, void **out)
{
    if (ctx->pool_bytes[slot] < bytes) {
        const size_t want = (bytes + (bytes >> 3) + 4095) / 4096 * 4096; // 12 % slack: sizes that creep up do not reallocate each call
        if (int rc = grow_buffer(ctx, &ctx->pool[slot], &ctx->pool_bytes[slot], &ctx->pool_in_graph[slot], want, "buffer pool")) return rc;
    }
    if (capture_state(ctx) != kCaptureOff) ctx->pool_in_graph[slot] = true;
    *out = ctx->pool[slot];
    return MI355_OK;
}

} // namespace mi355

namespace {

int check_width(unsigned c)
{
    if (c < 1 || c > 32) return fail(MI355_E_INVALID, "bit width c=%u outside 1..32", c);
    return MI355_OK;
}

// the selection workspace holds at least `entries` words (grown outside capture only; kept alive once a graph points at it)
int rowid_ws_get(mi355_ctx *ctx, uint64_t entries, const char *what)
{
    if (ctx->rowid_ws_entries < entries) {
        size_t bytes = ctx->rowid_ws_entries * sizeof(unsigned long long);
        int rc = grow_buffer(ctx, (void **)&ctx->rowid_ws, &bytes, &ctx->rowid_ws_in_graph, entries * sizeof(unsigned long long), what);
        ctx->rowid_ws_entries = bytes / sizeof(unsigned long long);
        if (rc) return rc;
    }
    if (capture_state(ctx) != kCaptureOff) ctx->rowid_ws_in_graph = true;
    return MI355_OK;
}

hipError_t (*const kGroups[kNumGroups])(const LaunchReq &) = MI355_GROUP_TABLE(launch_group_);
hipError_t (*const kWhereGroups[kNumGroups])(const WhereReq &) = MI355_GROUP_TABLE(launch_where_group_);
hipError_t (*const kColumnsGroups[kNumGroups])(const ColumnsReq &) = MI355_GROUP_TABLE(launch_columns_group_);

// rows from which a launch uses what mi355_tune_dev measured (smaller columns take microseconds whatever the grid)
constexpr uint64_t kTuneMinRows = 50000000ull;

// one entry per kernel shape: op, width, and for the scans whether a bitmap is written and whether a mask is read
inline uint32_t tune_key(int op, unsigned c, bool writes_bitmap, bool reads_mask)
{
    return (uint32_t)op * 64u + c + (writes_bitmap ? 0u : 1u << 12) + (reads_mask ? 1u << 13 : 0u);
}

// what every launcher's request takes from the context (LaunchReq, WhereReq::l, ColumnsReq::l)
void fill_common(mi355_ctx *ctx, LaunchReq &l)
{
    l.stream = ctx->stream;
    l.device = ctx->device;
    l.num_cus = grid_cus(ctx);
    l.record = l.choice_out ? nullptr : &ctx->last_launch; // introspection stays out of the record
    l.max_blocks_per_cu = ctx->max_blocks_per_cu;
    l.scan_nt_stores = ctx->scan_nt_stores;
}

int launch(mi355_ctx *ctx, LaunchReq &r)
{
    if (int rc = bind(ctx)) return rc;
    fill_common(ctx, r);
    r.dma_aux = ctx->dma_aux;
    r.shared_vpl = ctx->shared_vpl;
    r.scan_burst = ctx->scan_burst;
    r.llc_resident_mib = ctx->llc_resident_mib;
    ctx->llc_last_d = -1;
    r.llc_d_out = &ctx->llc_last_d;
    if (r.op == kOpScanEq || r.op == kOpScanRange) {
        // llc_prev is the launch that RUNS directly before this one.  Inside one capture that is the call captured before it
        // (a graph replays its nodes in the order they were captured); a captured call has not run when the capture ends and
        // the context never learns when its graph does, so across the boundary of a capture -- an eager call after a captured
        // one, the first call of a capture, calls of two captures -- nothing is a repeat (llc_prev_capture: the capture's id, 0 = eager).
        // (One host-side query of the stream's capture state per eq / range scan: no device work, no synchronisation.)
        unsigned long long cap_id = 0;
        const bool known = capture_state(ctx, &cap_id) != kCaptureUnknown; // unknown: neither a repeat nor something to repeat
        r.llc_repeat = known && ctx->llc_prev[0] == r.scan.packed && ctx->llc_prev[1] == r.scan.out && ctx->llc_prev[2] == r.scan.and_mask &&
                       ctx->llc_prev_n == r.scan.n && ctx->llc_prev_c == r.c && ctx->llc_prev_capture == cap_id;
        ctx->llc_prev[0] = r.scan.packed, ctx->llc_prev[1] = r.scan.out, ctx->llc_prev[2] = r.scan.and_mask;
        ctx->llc_prev_n = r.scan.n, ctx->llc_prev_c = r.c, ctx->llc_prev_capture = cap_id;
        if (!known) ctx->llc_prev[0] = nullptr;
    } else
        ctx->llc_prev[0] = nullptr; // another kernel's traffic went through the cache
    // the A/B switches of the shared scans (bits 0-8) never reach the selection kernels, whose switches live in bits 9-12 of
    // the option and arrive as their bits 1-4: two TIMING ablations (2 no expansion, 4 no look-back: wrong ids by construction)
    // and two A/B switches of select_kernel's chunk hand-out (8 chunks dealt out by block index as in round 2, 16 no barrier
    // per generation).  Option bits 13.. are further switches of the shared scans; they arrive as their bits 9.. and never reach
    // the selection.  Option bit 16 (kernel bit 12) is read nowhere and stays out; kernel bits 17 and 20 are the launcher's own.
    // (tests/test_kernel_paths.py maps every kernel-side test back through these two expressions.)
    r.scan.flags = r.op == kOpSelect ? ((ctx->kernel_flags >> 8) & 0x1eu) : ((ctx->kernel_flags & 0x1ffu) | ((ctx->kernel_flags >> 4) & 0xdee00u));
    r.scan.scratch = ctx->kernel_scratch;
    if (r.max_blocks_per_cu == 0 && !ctx->tuned_bpc.empty()) {
        const bool scan = r.op == kOpScanEq || r.op == kOpScanRange;
        if ((scan && r.scan.n >= kTuneMinRows) || (r.op == kOpDecompress && r.decomp.n >= kTuneMinRows)) {
            const auto it = ctx->tuned_bpc.find(scan ? tune_key(r.op, r.c, r.scan.out != nullptr, r.scan.and_mask != nullptr)
                                                     : tune_key(r.op, r.c, true, false));
            if (it != ctx->tuned_bpc.end()) r.max_blocks_per_cu = it->second;
        }
    }
    hipError_t e = kGroups[(r.c - 1) / 4](r);
    if (e != hipSuccess) return fail(MI355_E_HIP, "kernel launch (op %d, c=%u): %s", r.op, r.c, hipGetErrorString(e));
    return MI355_OK;
}

constexpr int kKeySlots = 8;
// a slot holds the longest list of either kind: 1024 (+ 8 of padding) keys, or as many (lo, span, negate) predicate triples
constexpr size_t kKeySlotInts = 3 * (kMaxKeys + 8);

// A list of P elements of elem_bytes -> device memory, padded to a multiple of 8 elements with copies of the last,
// asynchronously on the stream, through the ring of kKeySlots pinned / device slots.  `what`: the refusal under capture.
int upload_list(mi355_ctx *ctx, const void *src, size_t elem_bytes, unsigned P, const char *what, const void **dev)
{
    if (capture_state(ctx) != kCaptureOff) return fail(MI355_E_INVALID, "%s", what);
    const int slot = ctx->key_next;
    ctx->key_next = (slot + 1) % kKeySlots;
    if (ctx->key_used[slot]) HIP_TRY(hipEventSynchronize(ctx->key_events[slot])); // the copy out of this slot is done
    uint8_t *h = (uint8_t *)(ctx->keys_pinned + (size_t)slot * kKeySlotInts);
    uint8_t *d = (uint8_t *)(ctx->keys_scratch + (size_t)slot * kKeySlotInts);
    const unsigned npad = (P + 7) / 8 * 8;
    memcpy(h, src, (size_t)P * elem_bytes);
    for (unsigned k = P; k < npad; k++) memcpy(h + k * elem_bytes, (const uint8_t *)src + (size_t)(P - 1) * elem_bytes, elem_bytes);
    HIP_TRY(hipMemcpyAsync(d, h, (size_t)npad * elem_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->key_events[slot], ctx->stream));
    ctx->key_used[slot] = true;
    *dev = d;
    return MI355_OK;
}

// keys: the shared scans' lists of more than 8 keys, and every list of mi355_scan_in_dev
int upload_keys(mi355_ctx *ctx, const int32_t *keys_host, unsigned P, const int32_t **keys_dev)
{
    return upload_list(ctx, keys_host, sizeof(int32_t), P,
                       "this key list is uploaded per call (shared scans: P > 8; IN-list: every P) and cannot be captured into a graph",
                       (const void **)keys_dev);
}

// P > 8 normalised predicates as (lo, span, negate) triples
int upload_preds(mi355_ctx *ctx, const uint32_t *triples_host, unsigned P, const uint32_t **preds_dev)
{
    return upload_list(ctx, triples_host, 3 * sizeof(uint32_t), P,
                       "predicate lists longer than 8 are uploaded per call and cannot be captured into a graph", (const void **)preds_dev);
}

// the kernels of predicates/ take no switch word (their launch records read flags=0x0) and are not tuned per device
int launch_where(mi355_ctx *ctx, WhereReq &r)
{
    if (int rc = bind(ctx)) return rc;
    fill_common(ctx, r.l);
    r.w.s.flags = 0;
    r.w.s.scratch = ctx->kernel_scratch;
    hipError_t e = kWhereGroups[(r.l.c - 1) / 4](r);
    if (e != hipSuccess) return fail(MI355_E_HIP, "kernel launch (shared where-scan, c=%u): %s", r.l.c, hipGetErrorString(e));
    return MI355_OK;
}

// as launch_where: no switch word, not tuned per device
int launch_columns(mi355_ctx *ctx, ColumnsReq &r)
{
    if (int rc = bind(ctx)) return rc;
    fill_common(ctx, r.l);
    r.k.s.flags = 0;
    r.k.s.scratch = ctx->kernel_scratch;
    // bitmap stores as scan2_kernel's: write-through below 768 MiB of bitmap, non-temporal beyond; "scan_nt_stores" overrides
    r.k.nts = (uint32_t)one_pass_store_policy(r.k.s.n / 8, ctx->scan_nt_stores);
    ctx->llc_prev[0] = nullptr; // another kernel's traffic went through the cache
    ctx->llc_last_d = -1;
    hipError_t e = kColumnsGroups[(r.l.c - 1) / 4](r);
    if (e != hipSuccess) return fail(MI355_E_HIP, "kernel launch (column scan, c1=%u c2=%u): %s", r.l.c, r.k.c2, hipGetErrorString(e));
    return MI355_OK;
}

size_t bitmap_bytes(uint64_t n) { return (size_t)((n + 7) / 8); }

} // namespace

extern "C" {

const char *mi355_last_error(void) { return mi355::last_error(); }
const char *mi355_version(void) { return "mi355scan 0.2 (gfx950)"; }

int mi355_device_count(int *count)
{
    if (!count) return fail(MI355_E_INVALID, "count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(MI355_E_NODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return MI355_OK;
}

int mi355_ctx_create(int device, void *hip_stream, mi355_ctx **out)
{
    if (!out) return fail(MI355_E_INVALID, "out is null");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(MI355_E_NODEVICE, "no HIP device visible: this engine has no CPU fallback");
    if (device < 0 || device >= n) return fail(MI355_E_INVALID, "device %d out of range (0..%d)", device, n - 1);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(MI355_E_NODEVICE, "device %d is %s; libmi355scan is built for gfx950 (MI355X) only", device,
                    prop.gcnArchName);
    HIP_TRY(hipSetDevice(device));
    mi355_ctx *c = new mi355_ctx;
    c->device = device;
    c->stream = (hipStream_t)hip_stream;
    c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (const char *s = getenv("MI355_MAX_BLOCKS_PER_CU")) c->max_blocks_per_cu = atoi(s);
    if (const char *s = getenv("MI355_DMA_AUX")) c->dma_aux = atoi(s);
    if (const char *s = getenv("MI355_SCAN_BURST")) c->scan_burst = atoi(s);
    if (const char *s = getenv("MI355_LLC_RESIDENT_MIB")) c->llc_resident_mib = atoi(s);
    if (const char *s = getenv("MI355_SHARED_VPL")) c->shared_vpl = atoi(s);
    if (const char *s = getenv("MI355_KERNEL_FLAGS")) c->kernel_flags = (unsigned)atoi(s);
    // host-pointer flavours: the kernels write the hit counts here, straight into pinned (device-visible) host memory
    hipError_t e = hipHostMalloc((void **)&c->hits_scratch, kMaxKeys * sizeof(unsigned long long), hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void **)&c->kernel_scratch, kScratchWords * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(c->kernel_scratch, 0, kScratchWords * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void **)&c->keys_scratch, kKeySlots * kKeySlotInts * sizeof(int32_t));
    if (e == hipSuccess) e = hipHostMalloc((void **)&c->keys_pinned, kKeySlots * kKeySlotInts * sizeof(int32_t), hipHostMallocDefault);
    for (int i = 0; i < 8 && e == hipSuccess; i++) e = hipEventCreateWithFlags(&c->key_events[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->order_event, hipEventDisableTiming);
    if (e != hipSuccess) {
        if (c->hits_scratch) (void)hipHostFree(c->hits_scratch);
        (void)hipFree(c->kernel_scratch);
        (void)hipFree(c->keys_scratch);
        if (c->keys_pinned) (void)hipHostFree(c->keys_pinned);
        for (int i = 0; i < 8; i++)
            if (c->key_events[i]) (void)hipEventDestroy(c->key_events[i]);
        if (c->order_event) (void)hipEventDestroy(c->order_event);
        delete c;
        return fail(MI355_E_HIP, "hipMalloc(scratch): %s", hipGetErrorString(e));
    }
    *out = c;
    return MI355_OK;
}

int mi355_ctx_destroy(mi355_ctx *ctx)
{
    if (!ctx) return MI355_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->hits_scratch) (void)hipHostFree(ctx->hits_scratch);
    (void)hipFree(ctx->kernel_scratch);
    (void)hipFree(ctx->keys_scratch);
    if (ctx->keys_pinned) (void)hipHostFree(ctx->keys_pinned);
    for (int i = 0; i < 8; i++)
        if (ctx->key_events[i]) (void)hipEventDestroy(ctx->key_events[i]);
    if (ctx->order_event) (void)hipEventDestroy(ctx->order_event);
    (void)hipFree(ctx->rowid_ws);
    for (int i = 0; i < mi355_ctx::kPoolSlots; i++) (void)hipFree(ctx->pool[i]);
    for (void *p : ctx->retired) (void)hipFree(p); // buffers a captured graph pointed at: kept until here
    delete ctx;
    return MI355_OK;
}

int mi355_ctx_synchronize(mi355_ctx *ctx)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MI355_OK;
}

int mi355_ctx_set_stream(mi355_ctx *ctx, void *hip_stream)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    hipStream_t next = (hipStream_t)hip_stream;
    if (next == ctx->stream) return MI355_OK;
    if ((rc = bind(ctx))) return rc;
    // The scratch, the key slots and the buffer pool belong to the context, not to a stream: work already enqueued on
    // the old stream must be ordered before work on the new one.  A stream that is being captured cannot take part in
    // that (and a captured graph is ordered by whoever launches it): then the caller orders the two streams.
    if (capture_state(ctx->stream) == kCaptureOff && capture_state(next) == kCaptureOff && hipStreamQuery(ctx->stream) != hipSuccess) {
        HIP_TRY(hipEventRecord(ctx->order_event, ctx->stream));
        HIP_TRY(hipStreamWaitEvent(next, ctx->order_event, 0));
    }
    (void)hipGetLastError(); // hipStreamQuery's hipErrorNotReady is not a failure
    ctx->stream = next;
    return MI355_OK;
}

int mi355_shard_rows(uint64_t n, unsigned world, unsigned rank, uint64_t *first, uint64_t *count)
{
    if (!first || !count || world < 1 || rank >= world) return fail(MI355_E_INVALID, "bad shard arguments");
    const uint64_t align = 8192;
    uint64_t per = (n + world - 1) / world;
    per = (per + align - 1) / align * align;
    const uint64_t a = (uint64_t)rank * per < n ? (uint64_t)rank * per : n;
    const uint64_t b = (uint64_t)(rank + 1) * per < n ? (uint64_t)(rank + 1) * per : n;
    *first = a;
    *count = b - a;
    return MI355_OK;
}

int mi355_ctx_set_option(mi355_ctx *ctx, const char *name, int value)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    if (!name) return fail(MI355_E_INVALID, "name is null");
    if (!strcmp(name, "max_blocks_per_cu"))
        ctx->max_blocks_per_cu = value;
    else if (!strcmp(name, "dma_aux"))
        ctx->dma_aux = value;
    else if (!strcmp(name, "scan_nt_stores"))
        ctx->scan_nt_stores = value;
    else if (!strcmp(name, "shared_vpl"))
        ctx->shared_vpl = value;
    else if (!strcmp(name, "select_kernel"))
        ctx->select_kernel = value;
    else if (!strcmp(name, "scan_burst"))
        ctx->scan_burst = value;
    else if (!strcmp(name, "llc_resident_mib")) {
        if (value < -1 || value > 1024) return fail(MI355_E_INVALID, "llc_resident_mib=%d outside -1..1024", value);
        ctx->llc_resident_mib = value;
    } else if (!strcmp(name, "kernel_flags"))
        ctx->kernel_flags = (unsigned)value;
    else if (!strcmp(name, "grid_cus")) {
        if (value < 0 || value > ctx->num_cus) return fail(MI355_E_INVALID, "grid_cus=%d outside 0..%d", value, ctx->num_cus);
        ctx->grid_cus = value;
    } else
        return fail(MI355_E_INVALID, "unknown option %s", name);
    return MI355_OK;
}

/* ---- sizing: src/simd_scan.hpp:20-40 ---- */
size_t mi355_compressed_buffer_size(unsigned c, size_t n)
{
    size_t bits = (size_t)c * n;
    return bits / 8 + (bits % 8 != 0) + 256;
}
size_t mi355_decompression_output_buffer_size(size_t n) { return n * 4 + 32; }
size_t mi355_scan_output_buffer_size(size_t n) { return n / 8 + (n % 8 != 0) + 32; }
size_t mi355_bitmap_stride(size_t n) { return (n / 8 + (n % 8 != 0) + 255) / 256 * 256; }

/* ---- device memory ---- */
int mi355_dev_alloc(mi355_ctx *ctx, size_t bytes, void **dptr)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    if (!dptr) return fail(MI355_E_INVALID, "dptr is null");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMalloc(dptr, bytes ? bytes : 1));
    return MI355_OK;
}
int mi355_dev_free(mi355_ctx *ctx, void *dptr)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    HIP_TRY(hipFree(dptr));
    return MI355_OK;
}
int mi355_dev_upload(mi355_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    HIP_TRY(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MI355_OK;
}
int mi355_dev_download(mi355_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    HIP_TRY(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MI355_OK;
}
int mi355_dev_memset(mi355_ctx *ctx, void *dst_dev, int value, size_t bytes)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    HIP_TRY(hipMemsetAsync(dst_dev, value, bytes, ctx->stream));
    return MI355_OK;
}

/* ---- pack / generate ---- */
static int pack_launch(mi355_ctx *ctx, int src, const void *values_dev, uint64_t n, uint64_t first_row, uint64_t param,
                       unsigned c, void *packed_dev)
{
    int rc = check_width(c);
    if (rc) return rc;
    if (!packed_dev) return fail(MI355_E_INVALID, "packed_dev is null");
    if (((uintptr_t)packed_dev & 3) != 0) return fail(MI355_E_INVALID, "packed_dev must be 4-byte aligned");
    if ((src == kSrcU16 || src == kSrcU32) && !values_dev && n) return fail(MI355_E_INVALID, "values_dev is null");
    if (src == kSrcMod && param == 0) return fail(MI355_E_INVALID, "modulus 0");
    if (int brc = bind(ctx)) return brc;
    PackArgs a;
    a.values = values_dev;
    a.n = n;
    a.first_row = first_row;
    a.param = param;
    a.out = (uint32_t *)packed_dev;
    a.out_dwords = mi355_compressed_buffer_size(c, n) / 4; // payload + pad, whole dwords
    a.c = c;
    uint64_t blocks = (a.out_dwords + 255) / 256;
    uint64_t cap = (uint64_t)grid_cus(ctx) * 8;
    unsigned grid = (unsigned)(blocks < cap ? (blocks ? blocks : 1) : cap);
    std::string *const rec = &ctx->last_launch;
    switch (src) {
#define PACK_BY_WIDTH(SRC)                                                                                          \
    do { /* values per output dword: at most floor(31/c) + 2; one block per 8192-value tile, 4 resident per CU */  \
        uint64_t tiles = (n + kPackTile - 1) / kPackTile;                                                           \
        uint64_t tcap = (uint64_t)grid_cus(ctx) * 4;                                                                \
        unsigned tgrid = (unsigned)(tiles < tcap ? (tiles ? tiles : 1) : tcap);                                     \
        if (c >= 16) MI355_LAUNCH(rec, 0, (pack_tiled_kernel<SRC, 3>), dim3(tgrid), dim3(256), 0, ctx->stream, a);    \
        else if (c >= 8) MI355_LAUNCH(rec, 0, (pack_tiled_kernel<SRC, 5>), dim3(tgrid), dim3(256), 0, ctx->stream, a); \
        else if (c >= 4) MI355_LAUNCH(rec, 0, (pack_tiled_kernel<SRC, 9>), dim3(tgrid), dim3(256), 0, ctx->stream, a); \
        else if (c >= 2) MI355_LAUNCH(rec, 0, (pack_tiled_kernel<SRC, 17>), dim3(tgrid), dim3(256), 0, ctx->stream, a); \
        else MI355_LAUNCH(rec, 0, (pack_tiled_kernel<SRC, 32>), dim3(tgrid), dim3(256), 0, ctx->stream, a);           \
    } while (0)
    case kSrcU16: PACK_BY_WIDTH(kSrcU16); break;
    case kSrcU32: PACK_BY_WIDTH(kSrcU32); break;
#undef PACK_BY_WIDTH
    case kSrcMod: MI355_LAUNCH(rec, 0, pack_kernel<kSrcMod>, dim3(grid), dim3(256), 0, ctx->stream, a); break;
    case kSrcSplitmix: MI355_LAUNCH(rec, 0, pack_kernel<kSrcSplitmix>, dim3(grid), dim3(256), 0, ctx->stream, a); break;
    case kSrcIndex: MI355_LAUNCH(rec, 0, pack_kernel<kSrcIndex>, dim3(grid), dim3(256), 0, ctx->stream, a); break;
    default: return fail(MI355_E_INVALID, "unknown pack source %d", src);
    }
    HIP_TRY(hipGetLastError());
    // the trailing (compressed_buffer_size % 4) pad bytes, if any
    size_t total = mi355_compressed_buffer_size(c, n);
    if (total % 4) HIP_TRY(hipMemsetAsync((uint8_t *)packed_dev + total / 4 * 4, 0, total % 4, ctx->stream));
    return MI355_OK;
}

int mi355_pack_u16_dev(mi355_ctx *ctx, const uint16_t *values_dev, uint64_t n, unsigned c, void *packed_dev)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    return pack_launch(ctx, kSrcU16, values_dev, n, 0, 0, c, packed_dev);
}
int mi355_pack_u32_dev(mi355_ctx *ctx, const uint32_t *values_dev, uint64_t n, unsigned c, void *packed_dev)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    return pack_launch(ctx, kSrcU32, values_dev, n, 0, 0, c, packed_dev);
}
int mi355_generate_dev(mi355_ctx *ctx, int kind, uint64_t first_row, uint64_t n, unsigned c, uint64_t param,
                       void *packed_dev)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    int src = kind == MI355_GEN_MOD ? kSrcMod : kind == MI355_GEN_SPLITMIX ? kSrcSplitmix : kind == MI355_GEN_INDEX ? kSrcIndex : -1;
    if (src < 0) return fail(MI355_E_INVALID, "unknown generator kind %d", kind);
    return pack_launch(ctx, src, nullptr, n, first_row, param, c, packed_dev);
}

static int pack_host(mi355_ctx *ctx, int src, const void *values, size_t elem, uint64_t n, unsigned c, void *packed_host)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    if ((rc = check_width(c))) return rc;
    if (!packed_host || (!values && n)) return fail(MI355_E_INVALID, "null pointer");
    if ((rc = bind(ctx))) return rc;
    void *dv = nullptr, *dp = nullptr;
    size_t pbytes = mi355_compressed_buffer_size(c, n);
    if ((rc = pool_get(ctx, mi355_ctx::kPoolIn, n * elem + 16, &dv))) return rc;
    if ((rc = pool_get(ctx, mi355_ctx::kPoolOut, pbytes + 16, &dp))) return rc;
    HIP_TRY(hipMemcpyAsync(dv, values, n * elem, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = pack_launch(ctx, src, dv, n, 0, 0, c, dp))) return rc;
    HIP_TRY(hipMemcpyAsync(packed_host, dp, pbytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MI355_OK;
}
int mi355_pack_u16(mi355_ctx *ctx, const uint16_t *values, uint64_t n, unsigned c, void *packed_host)
{
    return pack_host(ctx, kSrcU16, values, 2, n, c, packed_host);
}
int mi355_pack_u32(mi355_ctx *ctx, const uint32_t *values, uint64_t n, unsigned c, void *packed_host)
{
    return pack_host(ctx, kSrcU32, values, 4, n, c, packed_host);
}

/* ---- decompress ---- */
int mi355_decompress_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, int32_t *out_dev)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    if ((rc = check_width(c))) return rc;
    if (n == 0) return MI355_OK;
    if (!packed_dev || !out_dev) return fail(MI355_E_INVALID, "null device pointer");
    if (((uintptr_t)packed_dev & 15) != 0) return fail(MI355_E_INVALID, "packed_dev must be 16-byte aligned");
    if (((uintptr_t)out_dev & 15) != 0) return fail(MI355_E_INVALID, "out_dev must be 16-byte aligned");
    LaunchReq r{};
    r.op = kOpDecompress;
    r.c = c;
    r.decomp.packed = (const uint8_t *)packed_dev;
    r.decomp.n = n;
    r.decomp.out = out_dev;
    return launch(ctx, r);
}

/* ---- scans (device pointers) ---- */
static int scan_common_dev(mi355_ctx *ctx, int op, const void *packed_dev, uint64_t n, unsigned c, uint32_t k0,
                           uint32_t k1, void *bitmap_dev, uint64_t *hits_dev)
{
    int rc = check_width(c);
    if (rc) return rc;
    if (n == 0) {
        if (hits_dev) HIP_TRY(hipMemsetAsync(hits_dev, 0, sizeof(uint64_t), ctx->stream));
        return MI355_OK;
    }
    if (!packed_dev || !bitmap_dev) return fail(MI355_E_INVALID, "null device pointer");
    if (((uintptr_t)packed_dev & 15) != 0) return fail(MI355_E_INVALID, "packed_dev must be 16-byte aligned");
    if (((uintptr_t)bitmap_dev & 15) != 0) return fail(MI355_E_INVALID, "bitmap_dev must be 16-byte aligned");
    LaunchReq r{};
    r.op = op;
    r.c = c;
    r.scan.packed = (const uint8_t *)packed_dev;
    r.scan.n = n;
    r.scan.out = (uint8_t *)bitmap_dev;
    r.scan.hits = (unsigned long long *)hits_dev;
    r.scan.key[0] = k0;
    r.scan.key[1] = k1;
    r.scan.nkeys = 1;
    return launch(ctx, r);
}

int mi355_scan_eq_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, int32_t key, void *bitmap_dev,
                      uint64_t *hits_dev)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    return scan_common_dev(ctx, kOpScanEq, packed_dev, n, c, (uint32_t)key, 0, bitmap_dev, hits_dev);
}

int mi355_scan_range_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, uint32_t lo, uint32_t hi,
                         void *bitmap_dev, uint64_t *hits_dev)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    if (lo > hi) {
        // empty range: all-zero bitmap, zero hits
        if ((rc = check_width(c))) return rc;
        if (hits_dev) HIP_TRY(hipMemsetAsync(hits_dev, 0, sizeof(uint64_t), ctx->stream));
        if (n && !bitmap_dev) return fail(MI355_E_INVALID, "null device pointer");
        if (n) HIP_TRY(hipMemsetAsync(bitmap_dev, 0, bitmap_bytes(n), ctx->stream));
        return MI355_OK;
    }
    return scan_common_dev(ctx, kOpScanRange, packed_dev, n, c, lo, hi - lo, bitmap_dev, hits_dev);
}

int mi355_shared_scan_eq_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const int32_t *keys_host,
                             unsigned P, int layout, void *out_dev, uint64_t stride_bytes, uint64_t *hits_dev)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    if ((rc = check_width(c))) return rc;
    if (P < 1 || P > (unsigned)kMaxKeys) return fail(MI355_E_INVALID, "P=%u outside 1..%u", P, kMaxKeys);
    if (!keys_host) return fail(MI355_E_INVALID, "keys is null");
    if (layout != MI355_LAYOUT_PER_PREDICATE && layout != MI355_LAYOUT_LINEAR)
        return fail(MI355_E_INVALID, "unknown layout %d", layout);
    if (n == 0) {
        if (hits_dev) HIP_TRY(hipMemsetAsync(hits_dev, 0, P * sizeof(uint64_t), ctx->stream));
        return MI355_OK;
    }
    if (!packed_dev || !out_dev) return fail(MI355_E_INVALID, "null device pointer");
    if (((uintptr_t)packed_dev & 15) != 0) return fail(MI355_E_INVALID, "packed_dev must be 16-byte aligned");
    if (layout == MI355_LAYOUT_PER_PREDICATE) {
        if (((uintptr_t)out_dev & 15) != 0 || (stride_bytes & 15) != 0)
            return fail(MI355_E_INVALID, "out_dev and stride_bytes must be multiples of 16");
        if (stride_bytes < bitmap_bytes(n)) return fail(MI355_E_INVALID, "stride_bytes smaller than ceil(n/8)");
    } else if (((uintptr_t)out_dev & 15) != 0) {
        return fail(MI355_E_INVALID, "out_dev must be 16-byte aligned");
    }
    // one predicate: both layouts are the plain bitmap of that key -- the equality scan kernel does it at twice the speed
    if (P == 1) return scan_common_dev(ctx, kOpScanEq, packed_dev, n, c, (uint32_t)keys_host[0], 0, out_dev, hits_dev);
    LaunchReq r{};
    r.op = kOpSharedScan;
    r.c = c;
    r.scan.packed = (const uint8_t *)packed_dev;
    r.scan.n = n;
    r.scan.out = (uint8_t *)out_dev;
    r.scan.out_stride = stride_bytes;
    r.scan.hits = (unsigned long long *)hits_dev;
    r.scan.nkeys = P;
    r.scan.layout = (uint32_t)layout;
    if (P <= (unsigned)kMaxKeysPerPass) {
        for (unsigned q = 0; q < (unsigned)kMaxKeysPerPass; q++) r.scan.key[q] = (uint32_t)keys_host[q < P ? q : P - 1];
    } else {
        if ((rc = bind(ctx))) return rc;
        if ((rc = upload_keys(ctx, keys_host, P, &r.scan.keys_dev))) return rc;
    }
    return launch(ctx, r);
}

/* ---- predicates and bitmap consumers beyond the reference ---- */
// every comparison is an inclusive range [lo, hi] over the column's domain [0, 2^c), possibly negated: fills
// key[0] = lo, key[1] = hi - lo and the negation word of a scan request.  a and b may be any int64: clamped to
// [-1, 2^32] first, which changes no comparison with a value in [0, 2^32) and keeps a - 1 / a + 1 from overflowing
static void fill_predicate(ScanArgs &sa, unsigned c, int op, int64_t a, int64_t b)
{
    const int64_t vmax = c == 32 ? 0xffffffffll : ((1ll << c) - 1);
    const int64_t kBelow = -1, kAbove = 1ll << 32;
    a = a < kBelow ? kBelow : (a > kAbove ? kAbove : a);
    b = b < kBelow ? kBelow : (b > kAbove ? kAbove : b);
    int64_t lo = 0, hi = vmax;
    bool invert = false, empty = false;
    switch (op) {
    case MI355_CMP_EQ: lo = hi = a; break;
    case MI355_CMP_NE: lo = hi = a; invert = true; break;
    case MI355_CMP_LT: hi = a - 1; break;
    case MI355_CMP_LE: hi = a; break;
    case MI355_CMP_GT: lo = a + 1; break;
    case MI355_CMP_GE: lo = a; break;
    case MI355_CMP_BETWEEN: lo = a; hi = b; break;
    case MI355_CMP_NOT_BETWEEN: lo = a; hi = b; invert = true; break;
    }
    if (lo < 0) lo = 0;
    if (hi > vmax) hi = vmax;
    if (lo > hi) empty = true; // matches nothing (or, negated, everything)
    sa.invert = invert ? 0xffffffffu : 0u;
    if (empty) { // lo above every value: t = x - lo is never <= span 0 unless x == 0xffffffff, which needs c == 32 ...
        sa.key[0] = 0xffffffffu;
        sa.key[1] = 0;
        if (c == 32) { // ... so fold the empty case into the negation flag on the full range
            sa.key[0] = 0;
            sa.key[1] = 0xffffffffu;
            sa.invert = invert ? 0u : 0xffffffffu;
        }
    } else {
        sa.key[0] = (uint32_t)lo;
        sa.key[1] = (uint32_t)(hi - lo);
    }
}

int mi355_scan_combine_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, int op, int64_t a, int64_t b,
                           int mask_op, const void *mask_dev, void *bitmap_dev, uint64_t *hits_dev)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    if ((rc = check_width(c))) return rc;
    if (op < MI355_CMP_EQ || op > MI355_CMP_NOT_BETWEEN) return fail(MI355_E_INVALID, "unknown comparison %d", op);
    if (mask_op < MI355_BITMAP_AND || mask_op > MI355_BITMAP_ANDNOT) return fail(MI355_E_INVALID, "unknown mask op %d", mask_op);
    if (!bitmap_dev && !hits_dev) return fail(MI355_E_INVALID, "bitmap_dev and hits_dev are both null: nothing to compute");
    if (n == 0) {
        if (hits_dev) HIP_TRY(hipMemsetAsync(hits_dev, 0, sizeof(uint64_t), ctx->stream));
        return MI355_OK;
    }
    if (!packed_dev) return fail(MI355_E_INVALID, "null device pointer");
    if (((uintptr_t)packed_dev & 15) || ((uintptr_t)bitmap_dev & 15) || ((uintptr_t)mask_dev & 15))
        return fail(MI355_E_INVALID, "packed_dev, bitmap_dev and mask_dev must be 16-byte aligned");
    LaunchReq r{};
    r.op = kOpScanRange;
    r.c = c;
    r.scan.packed = (const uint8_t *)packed_dev;
    r.scan.n = n;
    r.scan.out = (uint8_t *)bitmap_dev;
    r.scan.hits = (unsigned long long *)hits_dev;
    r.scan.nkeys = 1;
    r.scan.and_mask = (const uint8_t *)mask_dev;
    r.scan.mask_op = (uint32_t)mask_op;
    fill_predicate(r.scan, c, op, a, b);
    return launch(ctx, r);
}

int mi355_scan_select_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, int op, int64_t a, int64_t b, int mask_op,
                          const void *mask_dev, uint64_t first_row, uint64_t *rowids_dev, uint64_t capacity, uint64_t *count_dev)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    if ((rc = check_width(c))) return rc;
    if (op < MI355_CMP_EQ || op > MI355_CMP_NOT_BETWEEN) return fail(MI355_E_INVALID, "unknown comparison %d", op);
    if (mask_op < MI355_BITMAP_AND || mask_op > MI355_BITMAP_ANDNOT) return fail(MI355_E_INVALID, "unknown mask op %d", mask_op);
    if (!count_dev) return fail(MI355_E_INVALID, "count_dev is null");
    if ((rc = bind(ctx))) return rc;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(count_dev, 0, sizeof(uint64_t), ctx->stream));
        return MI355_OK;
    }
    if (!packed_dev || (!rowids_dev && capacity)) return fail(MI355_E_INVALID, "null device pointer");
    if (((uintptr_t)packed_dev & 15) || ((uintptr_t)mask_dev & 15))
        return fail(MI355_E_INVALID, "packed_dev and mask_dev must be 16-byte aligned");
    // one state word per chunk of tiles (decoupled look-back), zeroed in front of the launch
    const uint64_t tile_values = 64 * (uint64_t)scan_vpl((int)c, kModeRange);
    const uint64_t ntiles = (n + tile_values - 1) / tile_values;
    const uint64_t nchunks = (ntiles + select_tiles((int)c) - 1) / select_tiles((int)c);
    // + the chunk-ticket counter on its own line behind them (select_state_words); the same memset zeroes both
    const uint64_t nwords = select_state_words(nchunks);
    if ((rc = rowid_ws_get(ctx, nwords, "mi355_scan_select_dev"))) return rc;
    HIP_TRY(hipMemsetAsync(ctx->rowid_ws, 0, nwords * sizeof(unsigned long long), ctx->stream));
    // the count is written by atomic max (the last chunk's total, or ~0 from a wave that gave up): start it at 0
    HIP_TRY(hipMemsetAsync(count_dev, 0, sizeof(uint64_t), ctx->stream));
    LaunchReq r{};
    r.op = kOpSelect;
    r.c = c;
    r.scan.packed = (const uint8_t *)packed_dev;
    r.scan.n = n;
    r.scan.hits = (unsigned long long *)count_dev;
    r.scan.nkeys = 1;
    r.scan.and_mask = (const uint8_t *)mask_dev;
    r.scan.mask_op = (uint32_t)mask_op;
    r.scan.tile_state = ctx->rowid_ws;
    r.scan.rowids = rowids_dev;
    r.scan.capacity = capacity;
    r.scan.first_row = first_row;
    fill_predicate(r.scan, c, op, a, b);
    // Which kernel: select2_kernel (decoder + expander waves, one look-back per block and generation) is ahead of the
    // single-role select_kernel at every width and selectivity measured (profiles/r03_select_widths.txt: 1.01 - 1.2 x when
    // almost nothing qualifies, 1.2 - 3.3 x from 1/64 up), so it is what runs; option "select_kernel" = 1 keeps the older kernel
    // reachable for A/B runs (0 / 2: select2_kernel).
    r.select_single = ctx->select_kernel == 1;
    return launch(ctx, r);
}

int mi355_scan2_dev(mi355_ctx *ctx, const void *packed1_dev, unsigned c1, int op1, int64_t a1, int64_t b1, const void *packed2_dev,
                    unsigned c2, int op2, int64_t a2, int64_t b2, uint64_t n, int combine_op, void *bitmap_dev, uint64_t *hits_dev)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    if ((rc = check_width(c1)) || (rc = check_width(c2))) return rc;
    if (op1 < MI355_CMP_EQ || op1 > MI355_CMP_NOT_BETWEEN || op2 < MI355_CMP_EQ || op2 > MI355_CMP_NOT_BETWEEN)
        return fail(MI355_E_INVALID, "unknown comparison");
    if (combine_op < MI355_BITMAP_AND || combine_op > MI355_BITMAP_ANDNOT) return fail(MI355_E_INVALID, "unknown combine op %d", combine_op);
    if (!bitmap_dev && !hits_dev) return fail(MI355_E_INVALID, "bitmap_dev and hits_dev are both null: nothing to compute");
    if (n == 0) {
        if (hits_dev) HIP_TRY(hipMemsetAsync(hits_dev, 0, sizeof(uint64_t), ctx->stream));
        return MI355_OK;
    }
    if (!packed1_dev || !packed2_dev) return fail(MI355_E_INVALID, "null device pointer");
    if (((uintptr_t)packed1_dev & 15) || ((uintptr_t)packed2_dev & 15) || ((uintptr_t)bitmap_dev & 15))
        return fail(MI355_E_INVALID, "packed columns and bitmap_dev must be 16-byte aligned");
    if (c1 != c2) {
        // columns of different widths have different tile geometries: two launches, the first predicate's bitmap
        // combined inside the second scan, in place (every wave reads the mask bytes of a tile before it stores them)
        void *tmp = bitmap_dev;
        if (!tmp && (rc = pool_get(ctx, mi355_ctx::kPoolAux, bitmap_bytes(n) + 16, &tmp))) return rc;
        if ((rc = mi355_scan_combine_dev(ctx, packed1_dev, n, c1, op1, a1, b1, MI355_BITMAP_AND, nullptr, tmp, nullptr))) return rc;
        return mi355_scan_combine_dev(ctx, packed2_dev, n, c2, op2, a2, b2, combine_op, tmp, bitmap_dev, hits_dev);
    }
    LaunchReq r{};
    r.op = kOpScan2;
    r.c = c1;
    r.scan.packed = (const uint8_t *)packed1_dev;
    r.scan.packed2 = (const uint8_t *)packed2_dev;
    r.scan.n = n;
    r.scan.out = (uint8_t *)bitmap_dev;
    r.scan.hits = (unsigned long long *)hits_dev;
    r.scan.nkeys = 1;
    r.scan.mask_op = (uint32_t)combine_op;
    ScanArgs second{};
    fill_predicate(second, c2, op2, a2, b2);
    fill_predicate(r.scan, c1, op1, a1, b1);
    r.scan.key2[0] = second.key[0];
    r.scan.key2[1] = second.key[1];
    r.scan.invert2 = second.invert;
    return launch(ctx, r);
}

/* ---- include/mi355_columns.h: a predicate over the row-wise difference of two columns ---- */
// (op, a, b) over d = v1 - v2 -> an inclusive range [lo, hi] INSIDE the domain of d for this width pair,
// [-(2^c2 - 1), 2^c1 - 1], and a negation word.  a and b may be any int64: clamped to [-2^33, 2^33] first, which is outside
// every domain on both sides (no comparison changes) and keeps a - 1 / a + 1 from overflowing.  A range that misses the
// domain is the full range with the negation flipped, so lo <= hi always and hi - lo <= 2^33 - 2: the kernel needs no
// encoding of "empty".  Widths up to 30: lo fits an int32 and the span 31 bits (the 32-bit test is exact); above, 64 bits.
static void fill_difference(ColumnsArgs &k, unsigned c1, unsigned c2, int op, int64_t a, int64_t b)
{
    const int64_t dmin = -((1ll << c2) - 1), dmax = (1ll << c1) - 1;
    const int64_t kLim = 1ll << 33;
    a = a < -kLim ? -kLim : (a > kLim ? kLim : a);
    b = b < -kLim ? -kLim : (b > kLim ? kLim : b);
    int64_t lo = dmin, hi = dmax;
    bool invert = false;
    switch (op) {
    case MI355_CMP_EQ: lo = hi = a; break;
    case MI355_CMP_NE: lo = hi = a; invert = true; break;
    case MI355_CMP_LT: hi = a - 1; break;
    case MI355_CMP_LE: hi = a; break;
    case MI355_CMP_GT: lo = a + 1; break;
    case MI355_CMP_GE: lo = a; break;
    case MI355_CMP_BETWEEN: lo = a; hi = b; break;
    case MI355_CMP_NOT_BETWEEN: lo = a; hi = b; invert = true; break;
    }
    if (lo < dmin) lo = dmin;
    if (hi > dmax) hi = dmax;
    if (lo > hi) { // matches no d (or, negated, every d)
        lo = dmin;
        hi = dmax;
        invert = !invert;
    }
    k.s.invert = invert ? 0xffffffffu : 0u;
    k.lo64 = lo;
    k.span64 = (uint64_t)(hi - lo);
    k.lo = (uint32_t)(uint64_t)lo;  // two's complement low word: (int32)lo when both widths are <= 30
    k.span = (uint32_t)(hi - lo);
}

int mi355_scan_columns_dev(mi355_ctx *ctx, const void *packed1_dev, unsigned c1, const void *packed2_dev, unsigned c2, uint64_t n, int op,
                           int64_t a, int64_t b, int mask_op, const void *mask_dev, void *bitmap_dev, uint64_t *hits_dev)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    if ((rc = check_width(c1)) || (rc = check_width(c2))) return rc;
    if (op < MI355_CMP_EQ || op > MI355_CMP_NOT_BETWEEN) return fail(MI355_E_INVALID, "unknown comparison %d", op);
    if (mask_op < MI355_BITMAP_AND || mask_op > MI355_BITMAP_ANDNOT) return fail(MI355_E_INVALID, "unknown mask op %d", mask_op);
    if (!bitmap_dev && !hits_dev) return fail(MI355_E_INVALID, "bitmap_dev and hits_dev are both null: nothing to compute");
    if (n == 0) {
        if ((rc = bind(ctx))) return rc;
        if (hits_dev) HIP_TRY(hipMemsetAsync(hits_dev, 0, sizeof(uint64_t), ctx->stream));
        return MI355_OK;
    }
    if (!packed1_dev || !packed2_dev) return fail(MI355_E_INVALID, "null device pointer");
    if (((uintptr_t)packed1_dev & 15) || ((uintptr_t)packed2_dev & 15) || ((uintptr_t)bitmap_dev & 15) || ((uintptr_t)mask_dev & 15))
        return fail(MI355_E_INVALID, "packed columns, bitmap_dev and mask_dev must be 16-byte aligned");
    ColumnsReq r{};
    r.l.c = c1;
    r.k.c2 = c2;
    r.k.s.packed = (const uint8_t *)packed1_dev;
    r.k.s.packed2 = (const uint8_t *)packed2_dev;
    r.k.s.n = n;
    r.k.s.out = (uint8_t *)bitmap_dev;
    r.k.s.hits = (unsigned long long *)hits_dev;
    r.k.s.nkeys = 1;
    r.k.s.and_mask = (const uint8_t *)mask_dev;
    r.k.s.mask_op = (uint32_t)mask_op;
    fill_difference(r.k, c1, c2, op, a, b);
    return launch_columns(ctx, r);
}

int mi355_scan_where_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, int op, int64_t a, int64_t b,
                         const void *and_mask_dev, void *bitmap_dev, uint64_t *hits_dev)
{
    return mi355_scan_combine_dev(ctx, packed_dev, n, c, op, a, b, MI355_BITMAP_AND, and_mask_dev, bitmap_dev, hits_dev);
}

// P comparison predicates in one pass (kernels: predicates/where.hpp).  Each predicate goes through fill_predicate, the
// normalisation of the single-predicate scan: (lo, span, negation word).
int mi355_shared_scan_where_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const mi355_predicate *preds_host,
                                unsigned P, int layout, void *out_dev, uint64_t stride_bytes, uint64_t *hits_dev)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    if ((rc = check_width(c))) return rc;
    if (P < 1 || P > (unsigned)kMaxKeys) return fail(MI355_E_INVALID, "P=%u outside 1..%u", P, kMaxKeys);
    if (!preds_host) return fail(MI355_E_INVALID, "preds is null");
    if (layout != MI355_LAYOUT_PER_PREDICATE && layout != MI355_LAYOUT_LINEAR)
        return fail(MI355_E_INVALID, "unknown layout %d", layout);
    bool all_eq = true; // ... with constants the equality call's int32 keys can carry
    const int64_t vmax = c == 32 ? 0xffffffffll : ((1ll << c) - 1);
    for (unsigned k = 0; k < P; k++) {
        const mi355_predicate &p = preds_host[k];
        if (p.op < MI355_CMP_EQ || p.op > MI355_CMP_NOT_BETWEEN) return fail(MI355_E_INVALID, "preds[%u]: unknown comparison %d", k, p.op);
        if (p.reserved != 0) return fail(MI355_E_INVALID, "preds[%u]: reserved must be 0", k);
        if (p.op != MI355_CMP_EQ || ((p.a < 0 || p.a > vmax) ? c == 32 : p.a > 0x7fffffffll)) all_eq = false;
    }
    if (n == 0) {
        if (hits_dev) HIP_TRY(hipMemsetAsync(hits_dev, 0, P * sizeof(uint64_t), ctx->stream));
        return MI355_OK;
    }
    if (!packed_dev || !out_dev) return fail(MI355_E_INVALID, "null device pointer");
    if (((uintptr_t)packed_dev & 15) != 0) return fail(MI355_E_INVALID, "packed_dev must be 16-byte aligned");
    if (layout == MI355_LAYOUT_PER_PREDICATE) {
        if (((uintptr_t)out_dev & 15) != 0 || (stride_bytes & 15) != 0)
            return fail(MI355_E_INVALID, "out_dev and stride_bytes must be multiples of 16");
        if (stride_bytes < bitmap_bytes(n)) return fail(MI355_E_INVALID, "stride_bytes smaller than ceil(n/8)");
    } else if (((uintptr_t)out_dev & 15) != 0) {
        return fail(MI355_E_INVALID, "out_dev must be 16-byte aligned");
    }
    // one predicate: both layouts are its plain bitmap -- the single-predicate scan kernel
    if (P == 1)
        return mi355_scan_combine_dev(ctx, packed_dev, n, c, preds_host[0].op, preds_host[0].a, preds_host[0].b, MI355_BITMAP_AND, nullptr,
                                      out_dev, hits_dev);
    if (all_eq) { // literal equalities: the equality machinery (digit tables at every width, 32 keys per lookup)
        int32_t keys[kMaxKeys];
        for (unsigned k = 0; k < P; k++) keys[k] = (preds_host[k].a < 0 || preds_host[k].a > vmax) ? -1 : (int32_t)preds_host[k].a;
        return mi355_shared_scan_eq_dev(ctx, packed_dev, n, c, keys, P, layout, out_dev, stride_bytes, hits_dev);
    }
    WhereReq r{};
    r.l.op = kOpSharedScan;
    r.l.c = c;
    r.w.s.packed = (const uint8_t *)packed_dev;
    r.w.s.n = n;
    r.w.s.out = (uint8_t *)out_dev;
    r.w.s.out_stride = stride_bytes;
    r.w.s.hits = (unsigned long long *)hits_dev;
    r.w.s.nkeys = P;
    r.w.s.layout = (uint32_t)layout;
    auto normalise = [&](unsigned k, uint32_t *lo, uint32_t *span, uint32_t *neg) {
        ScanArgs one{};
        fill_predicate(one, c, preds_host[k].op, preds_host[k].a, preds_host[k].b);
        *lo = one.key[0];
        *span = one.key[1];
        *neg = one.invert;
    };
    if (P <= (unsigned)kMaxKeysPerPass) {
        for (unsigned q = 0; q < (unsigned)kMaxKeysPerPass; q++) normalise(q < P ? q : P - 1, &r.w.lo[q], &r.w.span[q], &r.w.neg[q]);
    } else {
        uint32_t triples[3 * kMaxKeys];
        for (unsigned k = 0; k < P; k++) normalise(k, &triples[3 * k], &triples[3 * k + 1], &triples[3 * k + 2]);
        if ((rc = bind(ctx))) return rc;
        if ((rc = upload_preds(ctx, triples, P, &r.w.preds_dev))) return rc;
    }
    return launch_where(ctx, r);
}

int mi355_scan_in_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const int32_t *keys_host, unsigned P,
                      int negate, const void *and_mask_dev, void *bitmap_dev, uint64_t *hits_dev)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    if ((rc = check_width(c))) return rc;
    if (P < 1 || P > (unsigned)kMaxKeys) return fail(MI355_E_INVALID, "P=%u outside 1..%u", P, kMaxKeys);
    if (!keys_host) return fail(MI355_E_INVALID, "keys is null");
    if (n == 0) {
        if (hits_dev) HIP_TRY(hipMemsetAsync(hits_dev, 0, sizeof(uint64_t), ctx->stream));
        return MI355_OK;
    }
    if (!packed_dev || !bitmap_dev) return fail(MI355_E_INVALID, "null device pointer");
    if (((uintptr_t)packed_dev & 15) || ((uintptr_t)bitmap_dev & 15) || ((uintptr_t)and_mask_dev & 15))
        return fail(MI355_E_INVALID, "packed_dev, bitmap_dev and and_mask_dev must be 16-byte aligned");
    if ((rc = bind(ctx))) return rc;
    const int32_t *keys_dev = nullptr;
    if ((rc = upload_keys(ctx, keys_host, P, &keys_dev))) return rc; // every P: in_kernel reads the list from device memory only
    LaunchReq r{};
    r.op = kOpScanIn;
    r.c = c;
    r.scan.packed = (const uint8_t *)packed_dev;
    r.scan.n = n;
    r.scan.out = (uint8_t *)bitmap_dev;
    r.scan.hits = (unsigned long long *)hits_dev;
    r.scan.keys_dev = keys_dev;
    r.scan.nkeys = P;
    r.scan.and_mask = (const uint8_t *)and_mask_dev;
    r.scan.invert = negate ? 0xffffffffu : 0u;
    return launch(ctx, r);
}

static int bitmap_launch(mi355_ctx *ctx, int op, const void *a, const void *b, void *out, uint64_t n, uint64_t *count_dev)
{
    if (int brc = bind(ctx)) return brc;
    if (n == 0) {
        if (count_dev) HIP_TRY(hipMemsetAsync(count_dev, 0, sizeof(uint64_t), ctx->stream));
        return MI355_OK;
    }
    if (!a || (op != kBitCount && (!b || !out))) return fail(MI355_E_INVALID, "null device pointer");
    if (((uintptr_t)a & 15) || ((uintptr_t)b & 15) || ((uintptr_t)out & 15))
        return fail(MI355_E_INVALID, "bitmaps must be 16-byte aligned");
    BitmapArgs g;
    g.a = (const uint8_t *)a;
    g.b = (const uint8_t *)b;
    g.out = (uint8_t *)out;
    g.nbytes = bitmap_bytes(n);
    // partial counts go to the (all-zero) hit-count replicas of the context scratch, then to count_dev
    g.count = count_dev ? ctx->kernel_scratch : nullptr;
    uint64_t blocks = (g.nbytes / 16 + 255) / 256;
    const uint64_t cap = (uint64_t)grid_cus(ctx) * 4;
    unsigned grid = (unsigned)(blocks < cap ? (blocks ? blocks : 1) : cap);
    std::string *const rec = &ctx->last_launch;
    switch (op) {
    case kBitAnd: MI355_LAUNCH(rec, 0, bitmap_kernel<kBitAnd>, dim3(grid), dim3(256), 0, ctx->stream, g); break;
    case kBitOr: MI355_LAUNCH(rec, 0, bitmap_kernel<kBitOr>, dim3(grid), dim3(256), 0, ctx->stream, g); break;
    case kBitXor: MI355_LAUNCH(rec, 0, bitmap_kernel<kBitXor>, dim3(grid), dim3(256), 0, ctx->stream, g); break;
    case kBitAndNot: MI355_LAUNCH(rec, 0, bitmap_kernel<kBitAndNot>, dim3(grid), dim3(256), 0, ctx->stream, g); break;
    case kBitCount: MI355_LAUNCH(rec, 0, bitmap_kernel<kBitCount>, dim3(grid), dim3(256), 0, ctx->stream, g); break;
    default: return fail(MI355_E_INVALID, "unknown bitmap op %d", op);
    }
    if (count_dev)
        MI355_LAUNCH(rec, 0, sum_slots_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->kernel_scratch, (unsigned long long *)count_dev);
    HIP_TRY(hipGetLastError());
    return MI355_OK;
}

int mi355_bitmap_combine_dev(mi355_ctx *ctx, int op, const void *a_dev, const void *b_dev, void *out_dev, uint64_t n,
                             uint64_t *count_dev)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    if (op < MI355_BITMAP_AND || op > MI355_BITMAP_ANDNOT) return fail(MI355_E_INVALID, "unknown bitmap op %d", op);
    return bitmap_launch(ctx, op, a_dev, b_dev, out_dev, n, count_dev);
}

int mi355_bitmap_count_dev(mi355_ctx *ctx, const void *bitmap_dev, uint64_t n, uint64_t *count_dev)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    if (!count_dev) return fail(MI355_E_INVALID, "count_dev is null");
    return bitmap_launch(ctx, kBitCount, bitmap_dev, nullptr, nullptr, n, count_dev);
}

int mi355_bitmap_to_rowids_dev(mi355_ctx *ctx, const void *bitmap_dev, uint64_t n, uint64_t first_row, uint64_t *rowids_dev,
                               uint64_t capacity, uint64_t *count_dev)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    if ((rc = bind(ctx))) return rc;
    if (!count_dev) return fail(MI355_E_INVALID, "count_dev is null");
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(count_dev, 0, sizeof(uint64_t), ctx->stream));
        return MI355_OK;
    }
    if (!bitmap_dev || (!rowids_dev && capacity)) return fail(MI355_E_INVALID, "null device pointer");
    if ((uintptr_t)bitmap_dev & 3) return fail(MI355_E_INVALID, "bitmap_dev must be 4-byte aligned");
    RowidArgs g;
    g.bitmap = (const uint8_t *)bitmap_dev;
    g.nbytes = bitmap_bytes(n);
    g.first_row = first_row;
    g.nchunks = (g.nbytes + kRowidChunk - 1) / kRowidChunk;
    const uint64_t ngroups = (g.nchunks + kRowidScanGroup - 1) / kRowidScanGroup;
    const uint64_t ws_entries = g.nchunks + 1 + ngroups; // chunk counts, the total, one total per scan group
    if ((rc = rowid_ws_get(ctx, ws_entries, "mi355_bitmap_to_rowids_dev"))) return rc;
    g.chunk_counts = ctx->rowid_ws;
    g.rowids = rowids_dev;
    g.capacity = capacity;
    uint64_t blocks = (g.nchunks + 3) / 4;
    unsigned grid = (unsigned)(blocks < (uint64_t)grid_cus(ctx) * 8 ? blocks : (uint64_t)grid_cus(ctx) * 8);
    std::string *const rec = &ctx->last_launch;
    MI355_LAUNCH(rec, 0, rowid_count_kernel, dim3(grid), dim3(256), 0, ctx->stream, g);
    MI355_LAUNCH(rec, 0, rowid_scan_kernel, dim3((unsigned)ngroups), dim3(256), 0, ctx->stream, g);
    MI355_LAUNCH(rec, 0, rowid_write_kernel, dim3(grid), dim3(256), 0, ctx->stream, g);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(count_dev, g.chunk_counts + g.nchunks, sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
    return MI355_OK;
}

int mi355_gather_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, uint64_t first_row, const uint64_t *rowids_dev,
                     const uint64_t *count_dev, uint64_t capacity, int32_t *out_dev)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    if ((rc = check_width(c))) return rc;
    if ((rc = bind(ctx))) return rc;
    if (!count_dev) return fail(MI355_E_INVALID, "count_dev is null (the number of ids is read on the device)");
    if (capacity == 0) return MI355_OK;
    if (!packed_dev || !rowids_dev || !out_dev) return fail(MI355_E_INVALID, "null device pointer");
    if ((uintptr_t)packed_dev & 3) return fail(MI355_E_INVALID, "packed_dev must be 4-byte aligned");
    GatherArgs g;
    g.packed = (const uint8_t *)packed_dev;
    g.n = n;
    g.c = c;
    g.first_row = first_row;
    g.rowids = rowids_dev;
    g.count_dev = count_dev;
    g.capacity = capacity;
    g.out = out_dev;
    // the grid is sized for `capacity` (the count is only known on the device); idle blocks leave at once
    const uint64_t blocks = (capacity + 255) / 256;
    const unsigned grid = (unsigned)(blocks < (uint64_t)grid_cus(ctx) * 16 ? blocks : (uint64_t)grid_cus(ctx) * 16);
    MI355_LAUNCH(&ctx->last_launch, 0, gather_kernel, dim3(grid), dim3(256), 0, ctx->stream, g);
    HIP_TRY(hipGetLastError());
    return MI355_OK;
}

int mi355_aggregate_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const void *mask_dev, uint64_t *out_dev)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    if ((rc = check_width(c))) return rc;
    if ((rc = bind(ctx))) return rc;
    if (!out_dev) return fail(MI355_E_INVALID, "out_dev is null");
    if (n && !packed_dev) return fail(MI355_E_INVALID, "null device pointer");
    if (((uintptr_t)packed_dev & 15) || ((uintptr_t)mask_dev & 3)) return fail(MI355_E_INVALID, "packed_dev must be 16-byte, mask_dev 4-byte aligned");
    AggArgs a;
    a.packed = (const uint8_t *)packed_dev;
    a.n = n;
    a.mask = (const uint8_t *)mask_dev;
    a.out = (unsigned long long *)out_dev;
    if (n == 0) {
        MI355_LAUNCH(&ctx->last_launch, 0, aggregate_init_kernel, dim3(1), dim3(1), 0, ctx->stream, a.out);
    } else if (!launch_aggregate_width(c, a, grid_cus(ctx), ctx->stream, &ctx->last_launch)) {
        return fail(MI355_E_INVALID, "width %u", c);
    }
    HIP_TRY(hipGetLastError());
    return MI355_OK;
}

int mi355_histogram_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const void *mask_dev, uint64_t *counts_dev)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    if ((rc = check_width(c))) return rc;
    if (c > (unsigned)kHistogramMaxBits) return fail(MI355_E_INVALID, "histogram: widths up to %d bits (2^c counters in LDS), got %u", kHistogramMaxBits, c);
    if ((rc = bind(ctx))) return rc;
    if (!counts_dev) return fail(MI355_E_INVALID, "counts_dev is null");
    if (n && !packed_dev) return fail(MI355_E_INVALID, "null device pointer");
    if (((uintptr_t)packed_dev & 15) || ((uintptr_t)mask_dev & 3)) return fail(MI355_E_INVALID, "packed_dev must be 16-byte, mask_dev 4-byte aligned");
    HIP_TRY(hipMemsetAsync(counts_dev, 0, sizeof(uint64_t) << c, ctx->stream));
    if (n == 0) return MI355_OK;
    HistArgs a;
    a.packed = (const uint8_t *)packed_dev;
    a.n = n;
    a.mask = (const uint8_t *)mask_dev;
    a.out = (unsigned long long *)counts_dev;
    if (!launch_histogram_width(c, a, grid_cus(ctx), ctx->stream, &ctx->last_launch)) return fail(MI355_E_INVALID, "width %u", c);
    HIP_TRY(hipGetLastError());
    return MI355_OK;
}

/* ---- host-pointer (copying, synchronous) flavours: the drop-in path ----
 * Device buffers come from the context's grow-only pool (no hipMalloc / hipFree per call).  The reference's callers
 * hand over compressed_buffer_size(c, n) bytes, pad included (src/simd_scan.hpp:20-26); only the payload travels, the
 * pad the kernels may touch (<= 15 bytes past the payload) is zeroed on the device. */
static int upload_packed(mi355_ctx *ctx, const void *packed_host, uint64_t n, unsigned c, void **dp)
{
    const size_t payload = (size_t)((n * c + 7) / 8);
    int rc = pool_get(ctx, mi355_ctx::kPoolIn, payload + 256, dp);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(*dp, packed_host, payload, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync((uint8_t *)*dp + payload, 0, 16, ctx->stream));
    return MI355_OK;
}

// ---- load-time tuning ------------------------------------------------------------------------------------------
// The resident blocks per CU at which the streaming kernels run fastest differ between MI355X boxes for the SAME
// binary (equality scan, c = 9: two blocks 3-5 % ahead of one on two boxes, 5 % behind on a third; decompress:
// profiles/r02_decompress_bpc_sweep.txt), so a static default leaves a few per cent behind somewhere.  This call
// measures 1 / 2 / 4 blocks per CU on the caller's own column, back to back as a query stream would issue them
// (isolated launches between event pairs rank the candidates differently), and keeps the winners in the context.
int mi355_tune_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, unsigned what)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    if ((rc = check_width(c))) return rc;
    if (!packed_dev || ((uintptr_t)packed_dev & 15)) return fail(MI355_E_INVALID, "packed_dev must be a 16-byte aligned device pointer");
    if (what == 0 || (what & ~(unsigned)MI355_TUNE_ALL)) return fail(MI355_E_INVALID, "what=%u: a mask of MI355_TUNE_* bits", what);
    if (n < kTuneMinRows) return MI355_OK; // nothing to learn: such launches never consult the table
    if ((rc = bind(ctx))) return rc;
    if (capture_state(ctx) != kCaptureOff)
        return fail(MI355_E_INVALID, "mi355_tune_dev synchronises: not while the stream is being captured into a graph");
    const size_t stride = mi355_bitmap_stride(n);
    void *bitmaps = nullptr, *values = nullptr;
    if ((rc = pool_get(ctx, mi355_ctx::kPoolOut, 2 * stride, &bitmaps))) return rc;
    uint8_t *bitmap = (uint8_t *)bitmaps, *mask = bitmap + stride;
    const uint64_t decomp_rows = n < (1ull << 28) ? n : (1ull << 28); // 1 GiB of output is plenty to rank the grids
    if ((what & MI355_TUNE_DECOMPRESS) && (rc = pool_get(ctx, mi355_ctx::kPoolAux, decomp_rows * 4 + 64, &values))) return rc;
    uint64_t *hits = (uint64_t *)ctx->hits_scratch;
    const uint32_t top = c >= 32 ? 0xffffffffu : (1u << c) - 1;
    const uint32_t lo = top / 4, hi = top / 2;
    HIP_TRY(hipMemsetAsync(mask, 0x5a, stride, ctx->stream));
    struct Shape {
        unsigned bit;
        int op;
        bool bitmap, mask;
    };
    // (mi355_scan_combine_dev and everything built on it -- count-only, fused masks, comparisons -- run the range kernel)
    const Shape shapes[] = {{MI355_TUNE_SCAN, kOpScanEq, true, false},
                            {MI355_TUNE_SCAN, kOpScanRange, true, false},
                            {MI355_TUNE_COUNT, kOpScanRange, false, false},
                            {MI355_TUNE_MASK, kOpScanRange, true, true},
                            {MI355_TUNE_DECOMPRESS, kOpDecompress, true, false}};
    const int cands[3] = {1, 2, 4};
    constexpr int kRounds = 3, kBurst = 6;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) {
        (void)hipEventDestroy(e0);
        return fail(MI355_E_HIP, "hipEventCreate failed");
    }
    const int saved = ctx->max_blocks_per_cu;
    for (const Shape &sh : shapes) {
        if (!(what & sh.bit)) continue;
        auto once = [&]() -> int {
            if (sh.op == kOpDecompress) return mi355_decompress_dev(ctx, packed_dev, decomp_rows, c, (int32_t *)values);
            if (sh.op == kOpScanEq) return mi355_scan_eq_dev(ctx, packed_dev, n, c, (int32_t)lo, bitmap, hits);
            return mi355_scan_combine_dev(ctx, packed_dev, n, c, MI355_CMP_BETWEEN, lo, hi, MI355_BITMAP_AND, sh.mask ? mask : nullptr,
                                          sh.bitmap ? bitmap : nullptr, hits);
        };
        float best[3] = {0, 0, 0};
        for (int round = 0; round < kRounds && rc == MI355_OK; round++)
            for (int k = 0; k < 3 && rc == MI355_OK; k++) {
                ctx->max_blocks_per_cu = cands[k];
                rc = once(); // the first launch after a change of grid is not timed
                if (rc == MI355_OK && hipEventRecord(e0, ctx->stream) != hipSuccess) rc = fail(MI355_E_HIP, "hipEventRecord failed");
                for (int i = 0; i < kBurst && rc == MI355_OK; i++) rc = once();
                if (rc == MI355_OK && (hipEventRecord(e1, ctx->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess))
                    rc = fail(MI355_E_HIP, "hipEventSynchronize failed");
                float ms = 0;
                if (rc == MI355_OK && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && (round == 0 || ms < best[k])) best[k] = ms;
            }
        ctx->max_blocks_per_cu = saved;
        if (rc != MI355_OK) break;
        int win = 0;
        for (int k = 1; k < 3; k++)
            if (best[k] < best[win] * 0.995f) win = k; // a later candidate has to win by more than the timer's noise
        ctx->tuned_bpc[tune_key(sh.op, c, sh.bitmap, sh.mask)] = cands[win];
    }
    ctx->max_blocks_per_cu = saved;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
}

int mi355_tuned_blocks_per_cu(mi355_ctx *ctx, unsigned c, unsigned what, int range)
{
    if (resolve(ctx)) return 0;
    CtxLock lk(ctx->mu);
    uint32_t key;
    if (what == MI355_TUNE_SCAN) key = tune_key(range ? kOpScanRange : kOpScanEq, c, true, false);
    else if (what == MI355_TUNE_COUNT) key = tune_key(kOpScanRange, c, false, false);
    else if (what == MI355_TUNE_MASK) key = tune_key(kOpScanRange, c, true, true);
    else if (what == MI355_TUNE_DECOMPRESS) key = tune_key(kOpDecompress, c, true, false);
    else return 0;
    const auto it = ctx->tuned_bpc.find(key);
    return it == ctx->tuned_bpc.end() ? 0 : it->second;
}

int mi355_decompress(mi355_ctx *ctx, const void *packed_host, uint64_t n, unsigned c, int32_t *out_host)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    if ((rc = check_width(c))) return rc;
    if (n == 0) return MI355_OK;
    if (!packed_host || !out_host) return fail(MI355_E_INVALID, "null pointer");
    if ((rc = bind(ctx))) return rc;
    void *dp = nullptr, *dout = nullptr;
    if ((rc = upload_packed(ctx, packed_host, n, c, &dp))) return rc;
    if ((rc = pool_get(ctx, mi355_ctx::kPoolOut, n * 4, &dout))) return rc;
    if ((rc = mi355_decompress_dev(ctx, dp, n, c, (int32_t *)dout))) return rc;
    HIP_TRY(hipMemcpyAsync(out_host, dout, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MI355_OK;
}

static int scan_host(mi355_ctx *ctx, int op, const void *packed_host, uint64_t n, unsigned c, uint32_t k0, uint32_t k1,
                     uint8_t *bitmap_host, uint64_t *hits)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    if ((rc = check_width(c))) return rc;
    if (hits) *hits = 0;
    if (n == 0) return MI355_OK;
    if (!packed_host || !bitmap_host) return fail(MI355_E_INVALID, "null pointer");
    if ((rc = bind(ctx))) return rc;
    void *dp = nullptr, *db = nullptr;
    if ((rc = upload_packed(ctx, packed_host, n, c, &dp))) return rc;
    if ((rc = pool_get(ctx, mi355_ctx::kPoolOut, bitmap_bytes(n) + 16, &db))) return rc;
    // the kernel delivers the hit count straight into pinned host memory: no second download
    if (op == kOpScanRange)
        rc = mi355_scan_range_dev(ctx, dp, n, c, k0, k1, db, (uint64_t *)ctx->hits_scratch);
    else
        rc = mi355_scan_eq_dev(ctx, dp, n, c, (int32_t)k0, db, (uint64_t *)ctx->hits_scratch);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(bitmap_host, db, bitmap_bytes(n), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (hits) *hits = (uint64_t)ctx->hits_scratch[0];
    return MI355_OK;
}

int mi355_scan_eq(mi355_ctx *ctx, const void *packed_host, uint64_t n, unsigned c, int32_t key, uint8_t *bitmap_host,
                  uint64_t *hits)
{
    return scan_host(ctx, kOpScanEq, packed_host, n, c, (uint32_t)key, 0, bitmap_host, hits);
}
int mi355_scan_range(mi355_ctx *ctx, const void *packed_host, uint64_t n, unsigned c, uint32_t lo, uint32_t hi,
                     uint8_t *bitmap_host, uint64_t *hits)
{
    return scan_host(ctx, kOpScanRange, packed_host, n, c, lo, hi, bitmap_host, hits);
}

// keys (equality) or preds (comparison predicates): exactly one of them is non-null
static int shared_host(mi355_ctx *ctx, const void *packed_host, uint64_t n, unsigned c, const int32_t *keys, unsigned P,
                       int layout, uint8_t *const *outputs, uint8_t *linear_out, uint64_t *hits, const mi355_predicate *preds = nullptr,
                       bool where = false)
{
    int rc = resolve(ctx);
    if (rc) return rc;
    CtxLock lk(ctx->mu);
    CallScope cs(ctx);
    if ((rc = check_width(c))) return rc;
    if (P < 1 || P > (unsigned)kMaxKeys) return fail(MI355_E_INVALID, "P=%u outside 1..%u", P, kMaxKeys);
    if (where ? !preds : !keys) return fail(MI355_E_INVALID, where ? "preds is null" : "keys is null");
    if (hits) memset(hits, 0, P * sizeof(uint64_t));
    if (n == 0) return MI355_OK;
    if (!packed_host || (layout == MI355_LAYOUT_PER_PREDICATE ? !outputs : !linear_out))
        return fail(MI355_E_INVALID, "null pointer");
    if ((rc = bind(ctx))) return rc;
    const size_t nb = bitmap_bytes(n);
    const size_t stride = mi355_bitmap_stride(n);
    void *dp = nullptr, *dout = nullptr;
    if ((rc = upload_packed(ctx, packed_host, n, c, &dp))) return rc;
    if ((rc = pool_get(ctx, mi355_ctx::kPoolOut, (layout == MI355_LAYOUT_PER_PREDICATE ? stride : nb) * P + 16, &dout))) return rc;
    // the reference's shared scans return no counts: only count when the caller asked
    uint64_t *const hits_dev = hits ? (uint64_t *)ctx->hits_scratch : nullptr;
    if ((rc = where ? mi355_shared_scan_where_dev(ctx, dp, n, c, preds, P, layout, dout, stride, hits_dev)
                    : mi355_shared_scan_eq_dev(ctx, dp, n, c, keys, P, layout, dout, stride, hits_dev)))
        return rc;
    if (layout == MI355_LAYOUT_PER_PREDICATE) {
        for (unsigned k = 0; k < P; k++) {
            if (!outputs[k]) return fail(MI355_E_INVALID, "outputs[%u] is null", k);
            HIP_TRY(hipMemcpyAsync(outputs[k], (uint8_t *)dout + k * stride, nb, hipMemcpyDeviceToHost, ctx->stream));
        }
    } else {
        HIP_TRY(hipMemcpyAsync(linear_out, dout, nb * P, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (hits) memcpy(hits, ctx->hits_scratch, P * sizeof(uint64_t));
    return MI355_OK;
}

int mi355_shared_scan_eq(mi355_ctx *ctx, const void *packed_host, uint64_t n, unsigned c, const int32_t *keys,
                         unsigned P, uint8_t *const *outputs, uint64_t *hits)
{
    return shared_host(ctx, packed_host, n, c, keys, P, MI355_LAYOUT_PER_PREDICATE, outputs, nullptr, hits);
}
int mi355_shared_scan_eq_linear(mi355_ctx *ctx, const void *packed_host, uint64_t n, unsigned c, const int32_t *keys,
                                unsigned P, uint8_t *output, uint64_t *hits)
{
    return shared_host(ctx, packed_host, n, c, keys, P, MI355_LAYOUT_LINEAR, nullptr, output, hits);
}

int mi355_shared_scan_where(mi355_ctx *ctx, const void *packed_host, uint64_t n, unsigned c, const mi355_predicate *preds, unsigned P,
                            uint8_t *const *outputs, uint64_t *hits)
{
    return shared_host(ctx, packed_host, n, c, nullptr, P, MI355_LAYOUT_PER_PREDICATE, outputs, nullptr, hits, preds, true);
}
int mi355_shared_scan_where_linear(mi355_ctx *ctx, const void *packed_host, uint64_t n, unsigned c, const mi355_predicate *preds,
                                   unsigned P, uint8_t *output, uint64_t *hits)
{
    return shared_host(ctx, packed_host, n, c, nullptr, P, MI355_LAYOUT_LINEAR, nullptr, output, hits, preds, true);
}

/* ---- introspection ---- */
int mi355_ctx_last_llc_divisor(mi355_ctx *ctx)
{
    if (resolve(ctx) != MI355_OK) return -1;
    CtxLock lk(ctx->mu);
    return ctx->llc_last_d;
}

const char *mi355_ctx_last_launch(mi355_ctx *ctx)
{
    static thread_local std::string copy;
    if (resolve(ctx) != MI355_OK) return nullptr;
    CtxLock lk(ctx->mu);
    copy = ctx->last_launch;
    return copy.c_str();
}

const char *mi355_kernel_name(const char *op, unsigned c)
{
    static thread_local char buf[96];
    if (!op || c < 1 || c > 32) return nullptr;
    if (!strcmp(op, "scan_eq"))
        snprintf(buf, sizeof buf, "mi355::scan_burst_kernel<%u, 0, ", c);
    else if (!strcmp(op, "scan_range"))
        snprintf(buf, sizeof buf, "mi355::scan_burst_kernel<%u, 1, ", c);
    else if (!strcmp(op, "shared_scan"))
        snprintf(buf, sizeof buf, "mi355::shared_lut_kernel<%u, ", c);
    else if (!strcmp(op, "decompress"))
        snprintf(buf, sizeof buf, "mi355::decompress_kernel<%u, ", c);
    else if (!strcmp(op, "pack"))
        snprintf(buf, sizeof buf, "mi355::pack_kernel<");
    else
        return nullptr;
    return buf;
}

const char *mi355_shared_scan_kernel(mi355_ctx *ctx, unsigned c, unsigned P, int layout, int with_hits)
{
    if (resolve(ctx) != MI355_OK) return nullptr;
    if (c < 1 || c > 32 || P < 1 || P > (unsigned)kMaxKeys) return nullptr;
    if (P == 1) return "scan_burst_kernel";
    CtxLock lk(ctx->mu);
    LaunchReq r{};
    int choice = -1;
    unsigned long long dummy = 0;
    r.op = kOpSharedScan;
    r.c = c;
    r.choice_out = &choice;
    r.scan.n = 1;
    r.scan.nkeys = P;
    r.scan.layout = (uint32_t)layout;
    r.scan.hits = with_hits ? &dummy : nullptr;
    if (launch(ctx, r) != MI355_OK) return nullptr;
    return choice >= 0 && choice < 6 ? kSharedFamilyName[choice] : nullptr;
}

const char *mi355_shared_where_kernel(mi355_ctx *ctx, unsigned c, unsigned P, int layout, int with_hits)
{
    if (resolve(ctx) != MI355_OK) return nullptr;
    if (c < 1 || c > 32 || P < 1 || P > (unsigned)kMaxKeys) return nullptr;
    if (P == 1) return "scan_burst_kernel";
    CtxLock lk(ctx->mu);
    WhereReq r{};
    int choice = -1;
    unsigned long long dummy = 0;
    r.l.c = c;
    r.l.choice_out = &choice;
    r.w.s.n = 1;
    r.w.s.nkeys = P;
    r.w.s.layout = (uint32_t)layout;
    r.w.s.hits = with_hits ? &dummy : nullptr;
    if (launch_where(ctx, r) != MI355_OK) return nullptr;
    static const char *const names[] = {"shared_where_lut_kernel", "shared_where_lut_kernel(multi-pass)", "shared_where_chain_kernel"};
    return choice >= 0 && choice < 3 ? names[choice] : nullptr;
}

uint64_t mi355_tile_values(unsigned c)
{
    if (c < 1 || c > 32) return 0;
    return 64 * (uint64_t)scan_vpl((int)c, kModeEq);
}

} // extern "C"
