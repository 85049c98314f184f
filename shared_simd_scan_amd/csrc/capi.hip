// capi.hip -- the scans of include/mi355_scan.h and include/mi355_columns.h that go through the three tables of group launchers
// (width_group.hip, predicates/where_group.hip, predicates/columns_group.hip), their host-pointer flavours, the load-time tuner
// and the introspection calls.  The context itself is context.hip, the entry points with kernels of their own extras.hip.
//
// Host-side plumbing only: argument checks (checks.hpp), predicate normalisation (predicate_norm.hpp), stream ordering, kernel
// dispatch by width.  All arithmetic of the path happens in the HIP kernels of kernels.hpp; there is no CPU implementation of any
// operation in this library, and this translation unit instantiates no kernel.
#include "ctx.hpp"

#include <cstring>

#include "checks.hpp"
#include "dispatch.hpp"
#include "launch_util.hpp"
#include "predicate_norm.hpp"
#include "shared_plan.hpp"
#include "predicates/where_dispatch.hpp"
#include "predicates/columns_dispatch.hpp"
#include "../../include/mi355_columns.h"

using namespace mi355;

namespace {

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
    fill_common(ctx, r);
    r.dma_aux = ctx->dma_aux;
    r.shared_vpl = ctx->shared_vpl;
    r.scan_burst = ctx->scan_burst;
    r.llc_resident_mib = ctx->llc_resident_mib;
    // eq / range: is it a repeat of the launch that runs directly before it (llc_repeat.hpp: the one place that decides, and the
    // only launcher that asks).  One host-side query of the stream's capture state per such scan: no device work, no synchronisation.
    const bool llc_scan = r.op == kOpScanEq || r.op == kOpScanRange;
    const LlcScan llc{r.scan.packed, r.scan.out, r.scan.and_mask, r.scan.n, r.c};
    unsigned long long cap_id = 0;
    const bool cap_known = llc_scan && capture_state(ctx, &cap_id) != kCaptureUnknown;
    int llc_d = -1;
    r.llc_d_out = &llc_d;
    r.llc_repeat = llc_scan && ctx->llc.is_repeat(llc, cap_known, cap_id, ctx->last_launch.size());
    r.scan.flags = kernel_switch_word(ctx->kernel_flags, r.op == kOpSelect); // (switches.hpp: the selection sees only its own)
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
    if (llc_scan) ctx->llc.launched(llc, cap_known, cap_id, llc_d, ctx->last_launch.size());
    return MI355_OK;
}

// what every scan request starts with: the operation, the column, where the bitmap and the counts go, the number of predicates
ScanArgs scan_args(const void *packed_dev, uint64_t n, void *out_dev, uint64_t *hits_dev, unsigned nkeys = 1)
{
    ScanArgs s{};
    s.packed = (const uint8_t *)packed_dev;
    s.n = n;
    s.out = (uint8_t *)out_dev;
    s.hits = (unsigned long long *)hits_dev;
    s.nkeys = nkeys;
    return s;
}
LaunchReq scan_request(int op, unsigned c, const void *packed_dev, uint64_t n, void *out_dev, uint64_t *hits_dev, unsigned nkeys = 1)
{
    LaunchReq r{};
    r.op = op;
    r.c = c;
    r.scan = scan_args(packed_dev, n, out_dev, hits_dev, nkeys);
    return r;
}

void set_predicate(ScanArgs &sa, const ValueTest &t)
{
    sa.key[0] = t.lo;
    sa.key[1] = t.span;
    sa.invert = t.invert;
}

// n == 0: nothing to scan, `words` hit counts of zero
int zero_hits(mi355_ctx *ctx, uint64_t *hits_dev, unsigned words = 1)
{
    if (hits_dev) HIP_TRY(hipMemsetAsync(hits_dev, 0, words * sizeof(uint64_t), ctx->stream));
    return MI355_OK;
}

// key lists (the shared scans' of more than 8 keys, every list of mi355_scan_in_dev) and lists of more than 8 normalised predicates
// ((lo, span, negate) triples) travel through upload_list: what it answers while the stream is being captured
constexpr const char *kKeysUploaded = "this key list is uploaded per call (shared scans: P > 8; IN-list: every P) and cannot be captured into a graph";
constexpr const char *kPredsUploaded = "predicate lists longer than 8 are uploaded per call and cannot be captured into a graph";

// the kernels of predicates/ take no switch word (their launch records read flags=0x0) and are not tuned per device
int launch_where(mi355_ctx *ctx, WhereReq &r)
{
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
    fill_common(ctx, r.l);
    r.k.s.flags = 0;
    r.k.s.scratch = ctx->kernel_scratch;
    // bitmap stores as scan2_kernel's: write-through below 768 MiB of bitmap, non-temporal beyond; "scan_nt_stores" overrides
    r.k.nts = (uint32_t)one_pass_store_policy(r.k.s.n / 8, ctx->scan_nt_stores);
    hipError_t e = kColumnsGroups[(r.l.c - 1) / 4](r);
    if (e != hipSuccess) return fail(MI355_E_HIP, "kernel launch (column scan, c1=%u c2=%u): %s", r.l.c, r.k.c2, hipGetErrorString(e));
    return MI355_OK;
}

} // namespace

extern "C" {

/* ---- decompress ---- */
int mi355_decompress_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, int32_t *out_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c));
    if (n == 0) return MI355_OK;
    MI355_CHECK(check_dev(packed_dev, 16, "packed_dev"));
    MI355_CHECK(check_dev(out_dev, 16, "out_dev"));
    LaunchReq r{};
    r.op = kOpDecompress;
    r.c = c;
    r.decomp.packed = (const uint8_t *)packed_dev;
    r.decomp.n = n;
    r.decomp.out = out_dev;
    return launch(ctx, r);
}

/* ---- scans (device pointers) ---- */
// one range test [k0, k0 + k1] into one bitmap; bitmap_name: what the caller's header calls the bitmap
static int scan_common_dev(mi355_ctx *ctx, int op, const void *packed_dev, uint64_t n, unsigned c, uint32_t k0, uint32_t k1,
                           void *bitmap_dev, uint64_t *hits_dev, const char *bitmap_name = "bitmap_dev")
{
    MI355_CHECK(check_width(c));
    if (n == 0) return zero_hits(ctx, hits_dev);
    MI355_CHECK(check_dev(packed_dev, 16, "packed_dev"));
    MI355_CHECK(check_dev(bitmap_dev, 16, bitmap_name));
    LaunchReq r = scan_request(op, c, packed_dev, n, bitmap_dev, hits_dev);
    r.scan.key[0] = k0;
    r.scan.key[1] = k1;
    return launch(ctx, r);
}

int mi355_scan_eq_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, int32_t key, void *bitmap_dev,
                      uint64_t *hits_dev)
{
    MI355_ENTER(ctx);
    return scan_common_dev(ctx, kOpScanEq, packed_dev, n, c, (uint32_t)key, 0, bitmap_dev, hits_dev);
}

int mi355_scan_range_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, uint32_t lo, uint32_t hi,
                         void *bitmap_dev, uint64_t *hits_dev)
{
    MI355_ENTER(ctx);
    if (lo > hi) {
        // empty range: all-zero bitmap, zero hits
        MI355_CHECK(check_width(c));
        MI355_CHECK(zero_hits(ctx, hits_dev));
        if (n) MI355_CHECK(check_ptr(bitmap_dev, "bitmap_dev"));
        if (n) HIP_TRY(hipMemsetAsync(bitmap_dev, 0, bitmap_bytes(n), ctx->stream));
        return MI355_OK;
    }
    return scan_common_dev(ctx, kOpScanRange, packed_dev, n, c, lo, hi - lo, bitmap_dev, hits_dev);
}

// what the two shared scans check alike, in front of their `n == 0` exit ...
static int check_shared_list(unsigned c, unsigned P, const void *list_host, const char *list_name, int layout)
{
    MI355_CHECK(check_width(c));
    MI355_CHECK(check_count(P));
    MI355_CHECK(check_ptr(list_host, list_name));
    return check_layout(layout);
}
// ... and behind it
static int check_shared_buffers(const void *packed_dev, const void *out_dev, int layout, uint64_t stride_bytes, uint64_t n)
{
    MI355_CHECK(check_dev(packed_dev, 16, "packed_dev"));
    MI355_CHECK(check_dev(out_dev, 16, "out_dev"));
    return check_stride(layout, stride_bytes, n);
}

int mi355_shared_scan_eq_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const int32_t *keys_host,
                             unsigned P, int layout, void *out_dev, uint64_t stride_bytes, uint64_t *hits_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_shared_list(c, P, keys_host, "keys_host", layout));
    if (n == 0) return zero_hits(ctx, hits_dev, P);
    MI355_CHECK(check_shared_buffers(packed_dev, out_dev, layout, stride_bytes, n));
    // one predicate: both layouts are the plain bitmap of that key -- the equality scan kernel does it at twice the speed
    if (P == 1) return scan_common_dev(ctx, kOpScanEq, packed_dev, n, c, (uint32_t)keys_host[0], 0, out_dev, hits_dev, "out_dev");
    LaunchReq r = scan_request(kOpSharedScan, c, packed_dev, n, out_dev, hits_dev, P);
    r.scan.out_stride = stride_bytes;
    r.scan.layout = (uint32_t)layout;
    if (P <= (unsigned)kMaxKeysPerPass) {
        for (unsigned q = 0; q < (unsigned)kMaxKeysPerPass; q++) r.scan.key[q] = (uint32_t)keys_host[q < P ? q : P - 1];
    } else {
        MI355_CHECK(upload_list(ctx, keys_host, sizeof(int32_t), P, kKeysUploaded, (const void **)&r.scan.keys_dev));
    }
    return launch(ctx, r);
}

/* ---- predicates and bitmap consumers beyond the reference ---- */
// every comparison is an inclusive range [lo, hi] over the column's domain [0, 2^c), possibly negated: normalise_predicate
// (predicate_norm.hpp) gives key[0] = lo, key[1] = hi - lo and the negation word of a scan request
int mi355_scan_combine_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, int op, int64_t a, int64_t b,
                           int mask_op, const void *mask_dev, void *bitmap_dev, uint64_t *hits_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c));
    MI355_CHECK(check_cmp(op));
    MI355_CHECK(check_bitmap_op(mask_op, "mask_op"));
    MI355_CHECK(check_some_output(bitmap_dev, hits_dev));
    if (n == 0) return zero_hits(ctx, hits_dev);
    MI355_CHECK(check_dev(packed_dev, 16, "packed_dev"));
    MI355_CHECK(check_aligned(bitmap_dev, 16, "bitmap_dev"));
    MI355_CHECK(check_aligned(mask_dev, 16, "mask_dev"));
    LaunchReq r = scan_request(kOpScanRange, c, packed_dev, n, bitmap_dev, hits_dev);
    r.scan.and_mask = (const uint8_t *)mask_dev;
    r.scan.mask_op = (uint32_t)mask_op;
    set_predicate(r.scan, normalise_predicate(c, op, a, b));
    return launch(ctx, r);
}

int mi355_scan_select_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, int op, int64_t a, int64_t b, int mask_op,
                          const void *mask_dev, uint64_t first_row, uint64_t *rowids_dev, uint64_t capacity, uint64_t *count_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c));
    MI355_CHECK(check_cmp(op));
    MI355_CHECK(check_bitmap_op(mask_op, "mask_op"));
    MI355_CHECK(check_ptr(count_dev, "count_dev"));
    if (n == 0) return zero_hits(ctx, count_dev);
    MI355_CHECK(check_dev(packed_dev, 16, "packed_dev"));
    if (capacity) MI355_CHECK(check_ptr(rowids_dev, "rowids_dev"));
    MI355_CHECK(check_aligned(mask_dev, 16, "mask_dev"));
    // one state word per chunk of tiles (decoupled look-back), zeroed in front of the launch
    const uint64_t tile_values = 64 * (uint64_t)scan_vpl((int)c, kModeRange);
    const uint64_t ntiles = (n + tile_values - 1) / tile_values;
    const uint64_t nchunks = (ntiles + select_tiles((int)c) - 1) / select_tiles((int)c);
    // + the chunk-ticket counter on its own line behind them (select_state_words); the same memset zeroes both
    const uint64_t nwords = select_state_words(nchunks);
    MI355_CHECK(rowid_ws_get(ctx, nwords, "mi355_scan_select_dev"));
    HIP_TRY(hipMemsetAsync(ctx->rowid_ws, 0, nwords * sizeof(unsigned long long), ctx->stream));
    // the count is written by atomic max (the last chunk's total, or ~0 from a wave that gave up): start it at 0
    MI355_CHECK(zero_hits(ctx, count_dev));
    LaunchReq r = scan_request(kOpSelect, c, packed_dev, n, nullptr, count_dev);
    r.scan.and_mask = (const uint8_t *)mask_dev;
    r.scan.mask_op = (uint32_t)mask_op;
    r.scan.tile_state = ctx->rowid_ws;
    r.scan.rowids = rowids_dev;
    r.scan.capacity = capacity;
    r.scan.first_row = first_row;
    set_predicate(r.scan, normalise_predicate(c, op, a, b));
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
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c1, "c1"));
    MI355_CHECK(check_width(c2, "c2"));
    MI355_CHECK(check_cmp(op1, "op1"));
    MI355_CHECK(check_cmp(op2, "op2"));
    MI355_CHECK(check_bitmap_op(combine_op, "combine_op"));
    MI355_CHECK(check_some_output(bitmap_dev, hits_dev));
    if (n == 0) return zero_hits(ctx, hits_dev);
    MI355_CHECK(check_dev(packed1_dev, 16, "packed1_dev"));
    MI355_CHECK(check_dev(packed2_dev, 16, "packed2_dev"));
    MI355_CHECK(check_aligned(bitmap_dev, 16, "bitmap_dev"));
    if (c1 != c2) {
        // columns of different widths have different tile geometries: two launches, the first predicate's bitmap
        // combined inside the second scan, in place (every wave reads the mask bytes of a tile before it stores them)
        void *tmp = bitmap_dev;
        if (!tmp) MI355_CHECK(pool_get(ctx, mi355_ctx::kPoolAux, bitmap_bytes(n) + 16, &tmp));
        MI355_CHECK(mi355_scan_combine_dev(ctx, packed1_dev, n, c1, op1, a1, b1, MI355_BITMAP_AND, nullptr, tmp, nullptr));
        return mi355_scan_combine_dev(ctx, packed2_dev, n, c2, op2, a2, b2, combine_op, tmp, bitmap_dev, hits_dev);
    }
    LaunchReq r = scan_request(kOpScan2, c1, packed1_dev, n, bitmap_dev, hits_dev);
    r.scan.packed2 = (const uint8_t *)packed2_dev;
    r.scan.mask_op = (uint32_t)combine_op;
    set_predicate(r.scan, normalise_predicate(c1, op1, a1, b1));
    const ValueTest second = normalise_predicate(c2, op2, a2, b2);
    r.scan.key2[0] = second.lo;
    r.scan.key2[1] = second.span;
    r.scan.invert2 = second.invert;
    return launch(ctx, r);
}

/* ---- include/mi355_columns.h: a predicate over the row-wise difference of two columns ---- */
// normalise_difference (predicate_norm.hpp): (op, a, b) over d = v1 - v2 -> an inclusive range inside the domain of d for this
// width pair and a negation word; the kernel needs no encoding of "empty"
int mi355_scan_columns_dev(mi355_ctx *ctx, const void *packed1_dev, unsigned c1, const void *packed2_dev, unsigned c2, uint64_t n, int op,
                           int64_t a, int64_t b, int mask_op, const void *mask_dev, void *bitmap_dev, uint64_t *hits_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c1, "c1"));
    MI355_CHECK(check_width(c2, "c2"));
    MI355_CHECK(check_cmp(op));
    MI355_CHECK(check_bitmap_op(mask_op, "mask_op"));
    MI355_CHECK(check_some_output(bitmap_dev, hits_dev));
    if (n == 0) return zero_hits(ctx, hits_dev);
    MI355_CHECK(check_dev(packed1_dev, 16, "packed1_dev"));
    MI355_CHECK(check_dev(packed2_dev, 16, "packed2_dev"));
    MI355_CHECK(check_aligned(bitmap_dev, 16, "bitmap_dev"));
    MI355_CHECK(check_aligned(mask_dev, 16, "mask_dev"));
    ColumnsReq r{};
    r.l.c = c1;
    r.k.c2 = c2;
    r.k.s = scan_args(packed1_dev, n, bitmap_dev, hits_dev);
    r.k.s.packed2 = (const uint8_t *)packed2_dev;
    r.k.s.and_mask = (const uint8_t *)mask_dev;
    r.k.s.mask_op = (uint32_t)mask_op;
    const DifferenceTest t = normalise_difference(c1, c2, op, a, b);
    r.k.s.invert = t.invert;
    r.k.lo64 = t.lo64;
    r.k.span64 = t.span64;
    r.k.lo = t.lo;
    r.k.span = t.span;
    return launch_columns(ctx, r);
}

int mi355_scan_where_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, int op, int64_t a, int64_t b,
                         const void *and_mask_dev, void *bitmap_dev, uint64_t *hits_dev)
{
    return mi355_scan_combine_dev(ctx, packed_dev, n, c, op, a, b, MI355_BITMAP_AND, and_mask_dev, bitmap_dev, hits_dev);
}

// P comparison predicates in one pass (kernels: predicates/where.hpp).  Each predicate goes through normalise_predicate, the
// normalisation of the single-predicate scan: (lo, span, negation word).
int mi355_shared_scan_where_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const mi355_predicate *preds_host,
                                unsigned P, int layout, void *out_dev, uint64_t stride_bytes, uint64_t *hits_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_shared_list(c, P, preds_host, "preds_host", layout));
    int32_t keys[kMaxKeys];
    bool all_eq = true; // literal equalities with constants the equality call's int32 keys can carry (equality_key)
    for (unsigned k = 0; k < P; k++) {
        const mi355_predicate &p = preds_host[k];
        if (check_cmp(p.op)) return fail(MI355_E_INVALID, "preds_host[%u].op: unknown comparison %d", k, p.op);
        if (p.reserved != 0) return fail(MI355_E_INVALID, "preds_host[%u].reserved must be 0", k);
        all_eq = all_eq && equality_key(c, p.op, p.a, &keys[k]);
    }
    if (n == 0) return zero_hits(ctx, hits_dev, P);
    MI355_CHECK(check_shared_buffers(packed_dev, out_dev, layout, stride_bytes, n));
    // one predicate: both layouts are its plain bitmap -- the single-predicate scan kernel
    if (P == 1)
        return mi355_scan_combine_dev(ctx, packed_dev, n, c, preds_host[0].op, preds_host[0].a, preds_host[0].b, MI355_BITMAP_AND, nullptr,
                                      out_dev, hits_dev);
    // literal equalities: the equality machinery (digit tables at every width, 32 keys per lookup)
    if (all_eq) return mi355_shared_scan_eq_dev(ctx, packed_dev, n, c, keys, P, layout, out_dev, stride_bytes, hits_dev);
    WhereReq r{};
    r.l.op = kOpSharedScan;
    r.l.c = c;
    r.w.s = scan_args(packed_dev, n, out_dev, hits_dev, P);
    r.w.s.out_stride = stride_bytes;
    r.w.s.layout = (uint32_t)layout;
    auto normalise = [&](unsigned k) { return normalise_predicate(c, preds_host[k].op, preds_host[k].a, preds_host[k].b); };
    if (P <= (unsigned)kMaxKeysPerPass) {
        for (unsigned q = 0; q < (unsigned)kMaxKeysPerPass; q++) {
            const ValueTest t = normalise(q < P ? q : P - 1);
            r.w.lo[q] = t.lo, r.w.span[q] = t.span, r.w.neg[q] = t.invert;
        }
    } else {
        uint32_t triples[3 * kMaxKeys];
        for (unsigned k = 0; k < P; k++) {
            const ValueTest t = normalise(k);
            triples[3 * k] = t.lo, triples[3 * k + 1] = t.span, triples[3 * k + 2] = t.invert;
        }
        MI355_CHECK(upload_list(ctx, triples, 3 * sizeof(uint32_t), P, kPredsUploaded, (const void **)&r.w.preds_dev));
    }
    return launch_where(ctx, r);
}

int mi355_scan_in_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const int32_t *keys_host, unsigned P,
                      int negate, const void *and_mask_dev, void *bitmap_dev, uint64_t *hits_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c));
    MI355_CHECK(check_count(P));
    MI355_CHECK(check_ptr(keys_host, "keys_host"));
    if (n == 0) return zero_hits(ctx, hits_dev);
    MI355_CHECK(check_dev(packed_dev, 16, "packed_dev"));
    MI355_CHECK(check_dev(bitmap_dev, 16, "bitmap_dev"));
    MI355_CHECK(check_aligned(and_mask_dev, 16, "and_mask_dev"));
    LaunchReq r = scan_request(kOpScanIn, c, packed_dev, n, bitmap_dev, hits_dev, P);
    MI355_CHECK(upload_list(ctx, keys_host, sizeof(int32_t), P, kKeysUploaded, (const void **)&r.scan.keys_dev)); // every P: in_kernel reads the list from device memory only
    r.scan.and_mask = (const uint8_t *)and_mask_dev;
    r.scan.invert = negate ? 0xffffffffu : 0u;
    return launch(ctx, r);
}

/* ---- host-pointer (copying, synchronous) flavours: the drop-in path ----
 * Device buffers come from the context's grow-only pool (no hipMalloc / hipFree per call).  The reference's callers
 * hand over compressed_buffer_size(c, n) bytes, pad included (src/simd_scan.hpp:20-26); only the payload travels, the
 * pad the kernels may touch (<= 15 bytes past the payload) is zeroed on the device. */
static int upload_packed(mi355_ctx *ctx, const void *packed_host, uint64_t n, unsigned c, void **dp)
{
    const size_t payload = (size_t)((n * c + 7) / 8);
    MI355_CHECK(pool_get(ctx, mi355_ctx::kPoolIn, payload + 256, dp));
    HIP_TRY(hipMemcpyAsync(*dp, packed_host, payload, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync((uint8_t *)*dp + payload, 0, 16, ctx->stream));
    return MI355_OK;
}

int mi355_decompress(mi355_ctx *ctx, const void *packed_host, uint64_t n, unsigned c, int32_t *out_host)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c));
    if (n == 0) return MI355_OK;
    MI355_CHECK(check_ptr(packed_host, "packed_host"));
    MI355_CHECK(check_ptr(out_host, "out_host"));
    void *dp = nullptr, *dout = nullptr;
    MI355_CHECK(upload_packed(ctx, packed_host, n, c, &dp));
    MI355_CHECK(pool_get(ctx, mi355_ctx::kPoolOut, n * 4, &dout));
    MI355_CHECK(mi355_decompress_dev(ctx, dp, n, c, (int32_t *)dout));
    HIP_TRY(hipMemcpyAsync(out_host, dout, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MI355_OK;
}

static int scan_host(mi355_ctx *ctx, int op, const void *packed_host, uint64_t n, unsigned c, uint32_t k0, uint32_t k1,
                     uint8_t *bitmap_host, uint64_t *hits)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c));
    if (hits) *hits = 0;
    if (n == 0) return MI355_OK;
    MI355_CHECK(check_ptr(packed_host, "packed_host"));
    MI355_CHECK(check_ptr(bitmap_host, "bitmap_host"));
    void *dp = nullptr, *db = nullptr;
    MI355_CHECK(upload_packed(ctx, packed_host, n, c, &dp));
    MI355_CHECK(pool_get(ctx, mi355_ctx::kPoolOut, bitmap_bytes(n) + 16, &db));
    // the kernel delivers the hit count straight into pinned host memory: no second download
    if (op == kOpScanRange)
        MI355_CHECK(mi355_scan_range_dev(ctx, dp, n, c, k0, k1, db, (uint64_t *)ctx->hits_scratch));
    else
        MI355_CHECK(mi355_scan_eq_dev(ctx, dp, n, c, (int32_t)k0, db, (uint64_t *)ctx->hits_scratch));
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
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c));
    MI355_CHECK(check_count(P));
    MI355_CHECK(where ? check_ptr(preds, "preds") : check_ptr(keys, "keys"));
    if (hits) memset(hits, 0, P * sizeof(uint64_t));
    if (n == 0) return MI355_OK;
    MI355_CHECK(check_ptr(packed_host, "packed_host"));
    MI355_CHECK(layout == MI355_LAYOUT_PER_PREDICATE ? check_ptr(outputs, "outputs") : check_ptr(linear_out, "output"));
    const size_t nb = bitmap_bytes(n);
    const size_t stride = mi355_bitmap_stride(n);
    void *dp = nullptr, *dout = nullptr;
    MI355_CHECK(upload_packed(ctx, packed_host, n, c, &dp));
    MI355_CHECK(pool_get(ctx, mi355_ctx::kPoolOut, (layout == MI355_LAYOUT_PER_PREDICATE ? stride : nb) * P + 16, &dout));
    // the reference's shared scans return no counts: only count when the caller asked
    uint64_t *const hits_dev = hits ? (uint64_t *)ctx->hits_scratch : nullptr;
    MI355_CHECK(where ? mi355_shared_scan_where_dev(ctx, dp, n, c, preds, P, layout, dout, stride, hits_dev)
                      : mi355_shared_scan_eq_dev(ctx, dp, n, c, keys, P, layout, dout, stride, hits_dev));
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

// ---- load-time tuning ------------------------------------------------------------------------------------------
// The resident blocks per CU at which the streaming kernels run fastest differ between MI355X boxes for the SAME
// binary (equality scan, c = 9: two blocks 3-5 % ahead of one on two boxes, 5 % behind on a third; decompress:
// profiles/r02_decompress_bpc_sweep.txt), so a static default leaves a few per cent behind somewhere.  This call
// measures 1 / 2 / 4 blocks per CU on the caller's own column, back to back as a query stream would issue them
// (isolated launches between event pairs rank the candidates differently), and keeps the winners in the context.
int mi355_tune_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, unsigned what)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c));
    MI355_CHECK(check_dev(packed_dev, 16, "packed_dev"));
    if (what == 0 || (what & ~(unsigned)MI355_TUNE_ALL)) return fail(MI355_E_INVALID, "what=%u: a mask of MI355_TUNE_* bits", what);
    if (n < kTuneMinRows) return MI355_OK; // nothing to learn: such launches never consult the table
    if (capture_state(ctx) != kCaptureOff)
        return fail(MI355_E_INVALID, "mi355_tune_dev synchronises: not while the stream is being captured into a graph");
    const size_t stride = mi355_bitmap_stride(n);
    void *bitmaps = nullptr, *values = nullptr;
    MI355_CHECK(pool_get(ctx, mi355_ctx::kPoolOut, 2 * stride, &bitmaps));
    uint8_t *bitmap = (uint8_t *)bitmaps, *mask = bitmap + stride;
    const uint64_t decomp_rows = n < (1ull << 28) ? n : (1ull << 28); // 1 GiB of output is plenty to rank the grids
    if (what & MI355_TUNE_DECOMPRESS) MI355_CHECK(pool_get(ctx, mi355_ctx::kPoolAux, decomp_rows * 4 + 64, &values));
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
    int rc = MI355_OK;
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
    Locked lk(ctx);
    if (lk.rc) return 0;
    uint32_t key;
    if (what == MI355_TUNE_SCAN) key = tune_key(range ? kOpScanRange : kOpScanEq, c, true, false);
    else if (what == MI355_TUNE_COUNT) key = tune_key(kOpScanRange, c, false, false);
    else if (what == MI355_TUNE_MASK) key = tune_key(kOpScanRange, c, true, true);
    else if (what == MI355_TUNE_DECOMPRESS) key = tune_key(kOpDecompress, c, true, false);
    else return 0;
    const auto it = ctx->tuned_bpc.find(key);
    return it == ctx->tuned_bpc.end() ? 0 : it->second;
}

/* ---- introspection ---- */
int mi355_ctx_last_llc_divisor(mi355_ctx *ctx)
{
    Locked lk(ctx);
    if (lk.rc) return -1;
    return ctx->llc.last_divisor(ctx->last_launch.size());
}

const char *mi355_ctx_last_launch(mi355_ctx *ctx)
{
    static thread_local std::string copy;
    Locked lk(ctx);
    if (lk.rc) return nullptr;
    copy = ctx->last_launch;
    return copy.c_str();
}

const char *mi355_kernel_name(const char *op, unsigned c)
{
    static thread_local char buf[96];
    if (!op || c < 1 || c > 32) return nullptr;
    static const char *const kPrefix[][2] = {{"scan_eq", "mi355::scan_burst_kernel<%u, 0, "}, {"scan_range", "mi355::scan_burst_kernel<%u, 1, "},
                                             {"shared_scan", "mi355::shared_lut_kernel<%u, "}, {"decompress", "mi355::decompress_kernel<%u, "}};
    if (!strcmp(op, "pack")) return "mi355::pack_kernel<";
    for (const auto &p : kPrefix)
        if (!strcmp(op, p[0])) {
            snprintf(buf, sizeof buf, p[1], c);
            return buf;
        }
    return nullptr;
}

const char *mi355_shared_scan_kernel(mi355_ctx *ctx, unsigned c, unsigned P, int layout, int with_hits)
{
    Locked lk(ctx);
    if (lk.rc || c < 1 || c > 32 || P < 1 || P > (unsigned)kMaxKeys) return nullptr;
    if (P == 1) return "scan_burst_kernel";
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
    Locked lk(ctx);
    if (lk.rc || c < 1 || c > 32 || P < 1 || P > (unsigned)kMaxKeys) return nullptr;
    if (P == 1) return "scan_burst_kernel";
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
