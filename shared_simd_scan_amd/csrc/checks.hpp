// checks.hpp -- the argument checks of the C entry points, one of each kind.  Each returns MI355_OK, or MI355_E_INVALID with a
// message that names the argument as the public header does.  Host code only.
#pragma once

#include "ctx.hpp"
#include "kernels/tile.hpp" // kMaxKeys

namespace mi355 {

// `if (int rc = ...) return rc;` for a chain of checks
#define MI355_CHECK(expr) do { if (int rc_ = (expr)) return rc_; } while (0)

// bit width of a packed column: 1..32, or 1..max where a kernel keeps 2^c of something in LDS (`why` says what)
inline int check_width(unsigned c, const char *name = "c", unsigned max = 32, const char *why = "")
{
    if (c < 1 || c > max) return fail(MI355_E_INVALID, "bit width %s=%u outside 1..%u%s", name, c, max, why);
    return MI355_OK;
}

// number of keys / predicates of a shared scan or an IN list
inline int check_count(unsigned P)
{
    if (P < 1 || P > (unsigned)kMaxKeys) return fail(MI355_E_INVALID, "P=%u outside 1..%d", P, kMaxKeys);
    return MI355_OK;
}

inline int check_layout(int layout)
{
    if (layout != MI355_LAYOUT_PER_PREDICATE && layout != MI355_LAYOUT_LINEAR) return fail(MI355_E_INVALID, "unknown layout %d", layout);
    return MI355_OK;
}

// MI355_CMP_*
inline int check_cmp(int op, const char *name = "op")
{
    if (op < MI355_CMP_EQ || op > MI355_CMP_NOT_BETWEEN) return fail(MI355_E_INVALID, "%s: unknown comparison %d", name, op);
    return MI355_OK;
}

// MI355_BITMAP_*: how a scan's result meets a mask, how two predicates or two bitmaps combine
inline int check_bitmap_op(int op, const char *name)
{
    if (op < MI355_BITMAP_AND || op > MI355_BITMAP_ANDNOT) return fail(MI355_E_INVALID, "%s: unknown bitmap op %d", name, op);
    return MI355_OK;
}

inline int check_ptr(const void *p, const char *name)
{
    if (!p) return fail(MI355_E_INVALID, "pointer %s is null", name);
    return MI355_OK;
}

// the one alignment test: null passes (optional operands; required ones go through check_ptr or check_dev)
inline int check_aligned(const void *p, unsigned bytes, const char *name)
{
    if ((uintptr_t)p & (bytes - 1)) return fail(MI355_E_INVALID, "pointer %s must be %u-byte aligned", name, bytes);
    return MI355_OK;
}

// a required device pointer: there, and aligned
inline int check_dev(const void *p, unsigned bytes, const char *name)
{
    MI355_CHECK(check_ptr(p, name));
    return check_aligned(p, bytes, name);
}

// a scan computes a bitmap, a count, or both
inline int check_some_output(const void *bitmap_dev, const void *hits_dev)
{
    if (!bitmap_dev && !hits_dev) return fail(MI355_E_INVALID, "bitmap_dev and hits_dev are both null: nothing to compute");
    return MI355_OK;
}

inline size_t bitmap_bytes(uint64_t n) { return (size_t)((n + 7) / 8); }
inline uint64_t packed_bytes(uint64_t n, unsigned c) { return (n * c + 7) / 8; } // n values of c bits (n c wraps only beyond what memory holds)

// do the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte?  (an output that overlaps an input a kernel reads while it writes)
inline bool ranges_overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a_bytes && b_bytes && pa < pb + b_bytes && pb < pa + a_bytes;
}

// an output must not share a byte with an input that the kernel reads while it writes (`what`: the column, the table, ...)
inline int check_no_overlap(const void *out, uint64_t out_bytes, const char *out_name, const void *in, uint64_t in_bytes, const char *in_name, const char *what)
{
    if (ranges_overlap(out, out_bytes, in, in_bytes))
        return fail(MI355_E_INVALID, "%s overlaps %s: the %s is read while the result is written", out_name, in_name, what);
    return MI355_OK;
}

// the per-predicate layout puts bitmap k at out_dev + k * stride_bytes: every one of them 16-byte aligned and long enough
inline int check_stride(int layout, uint64_t stride_bytes, uint64_t n)
{
    if (layout != MI355_LAYOUT_PER_PREDICATE) return MI355_OK;
    if (stride_bytes & 15) return fail(MI355_E_INVALID, "stride_bytes must be a multiple of 16 (every bitmap 16-byte aligned)");
    if (stride_bytes < bitmap_bytes(n)) return fail(MI355_E_INVALID, "stride_bytes smaller than ceil(n/8)");
    return MI355_OK;
}

} // namespace mi355
