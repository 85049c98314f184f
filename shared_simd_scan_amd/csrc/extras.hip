// extras.hip -- the entry points of include/mi355_scan.h that launch their own kernels instead of going through the width
// groups: pack / generate, bitmap combine / count, bitmap -> row ids, gather, aggregate, histogram.  Their kernels
// (kernels/pack.hpp, kernels/bitmap.hpp, extras/*.hpp) are instantiated here and nowhere else.
#include "ctx.hpp"

#include "checks.hpp"
#include "dispatch.hpp"
#include "launch_util.hpp"
#include "kernels.hpp"
#include "extras/gather.hpp"
#include "extras/aggregate.hpp"
#include "extras/histogram.hpp"

using namespace mi355;

namespace {
// `blocks`, capped at per_cu for each of the CUs the grids are sized for; at_least_one: no blocks still launch one
unsigned capped_grid(mi355_ctx *ctx, uint64_t blocks, int per_cu, bool at_least_one)
{
    const uint64_t cap = (uint64_t)grid_cus(ctx) * per_cu;
    if (at_least_one && blocks == 0) blocks = 1;
    return (unsigned)(blocks < cap ? blocks : cap);
}

// pack_tiled_kernel by width: values per output dword, at most floor(31/c) + 2; one block per 8192-value tile, 4 resident per CU
template <int SRC> void launch_pack_tiled(mi355_ctx *ctx, unsigned c, const PackArgs &a)
{
    const dim3 grid(capped_grid(ctx, (a.n + kPackTile - 1) / kPackTile, 4, true));
    std::string *const rec = &ctx->last_launch;
    if (c >= 16) MI355_LAUNCH(rec, 0, (pack_tiled_kernel<SRC, 3>), grid, dim3(256), 0, ctx->stream, a);
    else if (c >= 8) MI355_LAUNCH(rec, 0, (pack_tiled_kernel<SRC, 5>), grid, dim3(256), 0, ctx->stream, a);
    else if (c >= 4) MI355_LAUNCH(rec, 0, (pack_tiled_kernel<SRC, 9>), grid, dim3(256), 0, ctx->stream, a);
    else if (c >= 2) MI355_LAUNCH(rec, 0, (pack_tiled_kernel<SRC, 17>), grid, dim3(256), 0, ctx->stream, a);
    else MI355_LAUNCH(rec, 0, (pack_tiled_kernel<SRC, 32>), grid, dim3(256), 0, ctx->stream, a);
}
} // namespace

extern "C" {

/* ---- pack / generate ---- */
static int pack_launch(mi355_ctx *ctx, int src, const void *values_dev, uint64_t n, uint64_t first_row, uint64_t param,
                       unsigned c, void *packed_dev)
{
    MI355_CHECK(check_width(c));
    MI355_CHECK(check_dev(packed_dev, 4, "packed_dev"));
    if ((src == kSrcU16 || src == kSrcU32) && n) MI355_CHECK(check_ptr(values_dev, "values_dev"));
    if (src == kSrcMod && param == 0) return fail(MI355_E_INVALID, "param: modulus 0");
    PackArgs a;
    a.values = values_dev;
    a.n = n;
    a.first_row = first_row;
    a.param = param;
    a.out = (uint32_t *)packed_dev;
    a.out_dwords = mi355_compressed_buffer_size(c, n) / 4; // payload + pad, whole dwords
    a.c = c;
    const unsigned grid = capped_grid(ctx, (a.out_dwords + 255) / 256, 8, true);
    std::string *const rec = &ctx->last_launch;
    switch (src) {
    case kSrcU16: launch_pack_tiled<kSrcU16>(ctx, c, a); break;
    case kSrcU32: launch_pack_tiled<kSrcU32>(ctx, c, a); break;
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
    MI355_ENTER(ctx);
    return pack_launch(ctx, kSrcU16, values_dev, n, 0, 0, c, packed_dev);
}
int mi355_pack_u32_dev(mi355_ctx *ctx, const uint32_t *values_dev, uint64_t n, unsigned c, void *packed_dev)
{
    MI355_ENTER(ctx);
    return pack_launch(ctx, kSrcU32, values_dev, n, 0, 0, c, packed_dev);
}
int mi355_generate_dev(mi355_ctx *ctx, int kind, uint64_t first_row, uint64_t n, unsigned c, uint64_t param,
                       void *packed_dev)
{
    MI355_ENTER(ctx);
    int src = kind == MI355_GEN_MOD ? kSrcMod : kind == MI355_GEN_SPLITMIX ? kSrcSplitmix : kind == MI355_GEN_INDEX ? kSrcIndex : -1;
    if (src < 0) return fail(MI355_E_INVALID, "unknown generator kind %d", kind);
    return pack_launch(ctx, src, nullptr, n, first_row, param, c, packed_dev);
}

// host-pointer (copying, synchronous) flavours: device buffers from the context's grow-only pool
static int pack_host(mi355_ctx *ctx, int src, const void *values, size_t elem, uint64_t n, unsigned c, void *packed_host)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c));
    MI355_CHECK(check_ptr(packed_host, "packed_host"));
    if (n) MI355_CHECK(check_ptr(values, "values"));
    void *dv = nullptr, *dp = nullptr;
    size_t pbytes = mi355_compressed_buffer_size(c, n);
    MI355_CHECK(pool_get(ctx, mi355_ctx::kPoolIn, n * elem + 16, &dv));
    MI355_CHECK(pool_get(ctx, mi355_ctx::kPoolOut, pbytes + 16, &dp));
    HIP_TRY(hipMemcpyAsync(dv, values, n * elem, hipMemcpyHostToDevice, ctx->stream));
    MI355_CHECK(pack_launch(ctx, src, dv, n, 0, 0, c, dp));
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

/* ---- bitmap consumers ---- */
// a OP b -> out (+ count), or the count of a alone (kBitCount: b and out unused); names: the arguments as the caller's header has them
static int bitmap_launch(mi355_ctx *ctx, int op, const void *a, const void *b, void *out, uint64_t n, uint64_t *count_dev, const char *a_name)
{
    if (n == 0) {
        if (count_dev) HIP_TRY(hipMemsetAsync(count_dev, 0, sizeof(uint64_t), ctx->stream));
        return MI355_OK;
    }
    MI355_CHECK(check_dev(a, 16, a_name));
    if (op != kBitCount) {
        MI355_CHECK(check_dev(b, 16, "b_dev"));
        MI355_CHECK(check_dev(out, 16, "out_dev"));
    }
    BitmapArgs g;
    g.a = (const uint8_t *)a;
    g.b = (const uint8_t *)b;
    g.out = (uint8_t *)out;
    g.nbytes = bitmap_bytes(n);
    // partial counts go to the (all-zero) hit-count replicas of the context scratch, then to count_dev
    g.count = count_dev ? ctx->kernel_scratch : nullptr;
    const unsigned grid = capped_grid(ctx, (g.nbytes / 16 + 255) / 256, 4, true);
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
    MI355_ENTER(ctx);
    MI355_CHECK(check_bitmap_op(op, "op"));
    return bitmap_launch(ctx, op, a_dev, b_dev, out_dev, n, count_dev, "a_dev");
}

int mi355_bitmap_count_dev(mi355_ctx *ctx, const void *bitmap_dev, uint64_t n, uint64_t *count_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_ptr(count_dev, "count_dev"));
    return bitmap_launch(ctx, kBitCount, bitmap_dev, nullptr, nullptr, n, count_dev, "bitmap_dev");
}

int mi355_bitmap_to_rowids_dev(mi355_ctx *ctx, const void *bitmap_dev, uint64_t n, uint64_t first_row, uint64_t *rowids_dev,
                               uint64_t capacity, uint64_t *count_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_ptr(count_dev, "count_dev"));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(count_dev, 0, sizeof(uint64_t), ctx->stream));
        return MI355_OK;
    }
    MI355_CHECK(check_dev(bitmap_dev, 4, "bitmap_dev"));
    if (capacity) MI355_CHECK(check_ptr(rowids_dev, "rowids_dev"));
    const RowidPlan p = rowid_plan(n);
    MI355_CHECK(rowid_ws_get(ctx, p.words, "mi355_bitmap_to_rowids_dev"));
    RowidArgs g;
    g.bitmap = (const uint8_t *)bitmap_dev;
    g.nbytes = p.nbytes;
    g.first_row = first_row;
    g.nchunks = p.nchunks;
    g.chunk_counts = ctx->rowid_ws;
    g.rowids = rowids_dev;
    g.capacity = capacity;
    const LaunchEnv env = launch_env(ctx);
    launch_rowid_prefix<true>(env, p, g);
    MI355_LAUNCH(env.record, 0, rowid_write_kernel, dim3(rowid_chunk_grid(p, env.num_cus)), dim3(256), 0, ctx->stream, g);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(count_dev, g.chunk_counts + g.nchunks, sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
    return MI355_OK;
}

int mi355_gather_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, uint64_t first_row, const uint64_t *rowids_dev,
                     const uint64_t *count_dev, uint64_t capacity, int32_t *out_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c));
    MI355_CHECK(check_ptr(count_dev, "count_dev")); // the number of ids is read on the device
    if (capacity == 0) return MI355_OK;
    MI355_CHECK(check_dev(packed_dev, 4, "packed_dev"));
    MI355_CHECK(check_ptr(rowids_dev, "rowids_dev"));
    MI355_CHECK(check_ptr(out_dev, "out_dev"));
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
    const unsigned grid = capped_grid(ctx, (capacity + 255) / 256, 16, false);
    MI355_LAUNCH(&ctx->last_launch, 0, gather_kernel, dim3(grid), dim3(256), 0, ctx->stream, g);
    HIP_TRY(hipGetLastError());
    return MI355_OK;
}

// what aggregate and histogram check alike: the result, the column (needed from the first row on) and the optional mask
static int check_column_and_mask(const void *result, const char *result_name, const void *packed_dev, uint64_t n, const void *mask_dev)
{
    MI355_CHECK(check_ptr(result, result_name));
    if (n) MI355_CHECK(check_ptr(packed_dev, "packed_dev"));
    MI355_CHECK(check_aligned(packed_dev, 16, "packed_dev"));
    return check_aligned(mask_dev, 4, "mask_dev");
}

int mi355_aggregate_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const void *mask_dev, uint64_t *out_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c));
    MI355_CHECK(check_column_and_mask(out_dev, "out_dev", packed_dev, n, mask_dev));
    AggArgs a;
    a.packed = (const uint8_t *)packed_dev;
    a.n = n;
    a.mask = (const uint8_t *)mask_dev;
    a.out = (unsigned long long *)out_dev;
    if (n == 0) {
        MI355_LAUNCH(&ctx->last_launch, 0, aggregate_init_kernel, dim3(1), dim3(1), 0, ctx->stream, a.out);
    } else if (launch_aggregate_width(c, launch_env(ctx), a) != hipSuccess) {
        return fail(MI355_E_INVALID, "width %u", c);
    }
    HIP_TRY(hipGetLastError());
    return MI355_OK;
}

int mi355_histogram_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const void *mask_dev, uint64_t *counts_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c, "c", kHistogramMaxBits, " (histogram: 2^c counters in LDS)"));
    MI355_CHECK(check_column_and_mask(counts_dev, "counts_dev", packed_dev, n, mask_dev));
    HIP_TRY(hipMemsetAsync(counts_dev, 0, sizeof(uint64_t) << c, ctx->stream));
    if (n == 0) return MI355_OK;
    HistArgs a;
    a.packed = (const uint8_t *)packed_dev;
    a.n = n;
    a.mask = (const uint8_t *)mask_dev;
    a.out = (unsigned long long *)counts_dev;
    if (launch_histogram_width(c, launch_env(ctx), a) != hipSuccess) return fail(MI355_E_INVALID, "width %u", c);
    HIP_TRY(hipGetLastError());
    return MI355_OK;
}

} // extern "C"
