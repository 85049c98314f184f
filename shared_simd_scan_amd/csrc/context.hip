// context.hip -- the context behind include/mi355_scan.h: its life cycle, options, stream, buffers and capture state, the
// memory helpers and the sizing functions.  Host code only: this translation unit launches no kernel.
#include "ctx.hpp"

#include <cstdlib>
#include <cstring>

#include "checks.hpp"
#include "kernels/tile.hpp" // kMaxKeys, kScratchWords

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

// a slot of the upload ring holds the longest list of either kind: 1024 (+ 8 of padding) keys, or as many (lo, span, negate)
// predicate triples
constexpr size_t kKeySlotInts = 3 * (kMaxKeys + 8);

// everything a context owns on the device and in pinned memory; whatever create got as far as allocating
void release(mi355_ctx *ctx)
{
    if (ctx->hits_scratch) (void)hipHostFree(ctx->hits_scratch);
    (void)hipFree(ctx->kernel_scratch);
    (void)hipFree(ctx->keys_scratch);
    if (ctx->keys_pinned) (void)hipHostFree(ctx->keys_pinned);
    for (int i = 0; i < kKeySlots; i++)
        if (ctx->key_events[i]) (void)hipEventDestroy(ctx->key_events[i]);
    if (ctx->order_event) (void)hipEventDestroy(ctx->order_event);
    (void)hipFree(ctx->rowid_ws);
    for (int i = 0; i < mi355_ctx::kPoolSlots; i++) (void)hipFree(ctx->pool[i]);
    for (void *p : ctx->retired) (void)hipFree(p); // buffers a captured graph pointed at: kept until here
    delete ctx;
}

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

CaptureState capture_state(hipStream_t stream, unsigned long long *id)
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

} // namespace mi355

extern "C" {

const char *mi355_last_error(void) { return mi355::last_error(); }
const char *mi355_version(void) { return "mi355scan 0.2 (gfx950)"; }

int mi355_device_count(int *count)
{
    MI355_CHECK(check_ptr(count, "count"));
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
    MI355_CHECK(check_ptr(out, "out"));
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
    for (int i = 0; i < kKeySlots && e == hipSuccess; i++) e = hipEventCreateWithFlags(&c->key_events[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->order_event, hipEventDisableTiming);
    if (e != hipSuccess) {
        release(c);
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
    release(ctx);
    return MI355_OK;
}

int mi355_ctx_synchronize(mi355_ctx *ctx)
{
    MI355_ENTER(ctx, Entry::kKeepRecord);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MI355_OK;
}

int mi355_ctx_set_stream(mi355_ctx *ctx, void *hip_stream)
{
    Locked lk(ctx);
    if (lk.rc) return lk.rc;
    hipStream_t next = (hipStream_t)hip_stream;
    if (next == ctx->stream) return MI355_OK;
    if (int rc = bind(ctx)) return rc;
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
    MI355_CHECK(check_ptr(first, "first"));
    MI355_CHECK(check_ptr(count, "count"));
    if (world < 1 || rank >= world) return fail(MI355_E_INVALID, "rank %u outside a world of %u", rank, world);
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
    Locked lk(ctx);
    if (lk.rc) return lk.rc;
    MI355_CHECK(check_ptr(name, "name"));
    static const struct { const char *name; int mi355_ctx::*field; } kPlain[] = { // options that take any value
        {"max_blocks_per_cu", &mi355_ctx::max_blocks_per_cu}, {"dma_aux", &mi355_ctx::dma_aux}, {"scan_nt_stores", &mi355_ctx::scan_nt_stores},
        {"shared_vpl", &mi355_ctx::shared_vpl}, {"select_kernel", &mi355_ctx::select_kernel}, {"scan_burst", &mi355_ctx::scan_burst}};
    for (const auto &o : kPlain)
        if (!strcmp(name, o.name)) {
            ctx->*o.field = value;
            return MI355_OK;
        }
    if (!strcmp(name, "llc_resident_mib")) {
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

/* ---- device memory: stream work on the context's device, no launch record of its own ---- */
int mi355_dev_alloc(mi355_ctx *ctx, size_t bytes, void **dptr)
{
    MI355_ENTER(ctx, Entry::kKeepRecord);
    MI355_CHECK(check_ptr(dptr, "dptr"));
    HIP_TRY(hipMalloc(dptr, bytes ? bytes : 1));
    return MI355_OK;
}
int mi355_dev_free(mi355_ctx *ctx, void *dptr)
{
    MI355_ENTER(ctx, Entry::kKeepRecord);
    HIP_TRY(hipFree(dptr));
    return MI355_OK;
}
static int copy_and_wait(mi355_ctx *ctx, void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
    MI355_ENTER(ctx, Entry::kKeepRecord);
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MI355_OK;
}
int mi355_dev_upload(mi355_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes)
{
    return copy_and_wait(ctx, dst_dev, src_host, bytes, hipMemcpyHostToDevice);
}
int mi355_dev_download(mi355_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes)
{
    return copy_and_wait(ctx, dst_host, src_dev, bytes, hipMemcpyDeviceToHost);
}
int mi355_dev_memset(mi355_ctx *ctx, void *dst_dev, int value, size_t bytes)
{
    MI355_ENTER(ctx, Entry::kKeepRecord);
    HIP_TRY(hipMemsetAsync(dst_dev, value, bytes, ctx->stream));
    return MI355_OK;
}

} // extern "C"
