"""The reference routes of test_large_columns.py: every feature entry point's operation restated in plain torch over decoded values,
slice by slice, so that a column of more than 2^32 rows is checked at full size on the device by code that shares nothing with
the kernels -- no packed reads, no tiles, no 32-bit offsets (row ids and sums are int64 throughout).  Every function takes tensors
on any device; test_large_columns.py runs each of them on the CPU against the numpy expectations of support.py and of the entry
points' own test files, so a wrong route fails without a GPU.

A route that has to remember something from one slice to the next (a running sum, the open run, the ties already taken) is a small
class whose step() takes the slices in row order."""
import torch

DENSE = 64  # up to this many groups or table entries a route reduces group by group instead of scattering


def u32(t):
    """decoded values as decompress leaves them (int32, a 32-bit value's top bit in the sign) -> int64 in 0..2^32 - 1"""
    return t.to(torch.int64) & 0xFFFFFFFF


def _weights(device):
    return torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=device)


def pack_bitmap(bits):
    """bool[m] -> the canonical bitmap, uint8[ceil(m / 8)]: bit i = byte i / 8, bit i % 8; the bits behind m are zero"""
    m = bits.numel()
    if m % 8:
        bits = torch.cat([bits, torch.zeros(8 - m % 8, dtype=torch.bool, device=bits.device)])
    return (bits.view(-1, 8).to(torch.int32) * _weights(bits.device)).sum(dim=1).to(torch.uint8)


def unpack_bitmap(data, m):
    """uint8[>= ceil(m / 8)] -> bool[m]"""
    nb = (m + 7) // 8
    shifts = torch.arange(8, dtype=torch.int32, device=data.device)
    return ((data[:nb].to(torch.int32)[:, None] >> shifts) & 1).to(torch.bool).view(-1)[:m]


def bitmap_of_rows(rows, n, pad=32, invert=False):
    """the canonical bitmap of n rows with exactly the sorted, distinct `rows` (int64) set -- with invert: exactly those clear --
    followed by `pad` zero bytes: how the tests make a sparse mask, or a nearly-all-ones one, without a bool per row"""
    nb = (n + 7) // 8
    data = torch.zeros(nb + pad, dtype=torch.uint8, device=rows.device)
    byte, inverse = torch.unique_consecutive(rows >> 3, return_inverse=True)
    acc = torch.zeros(byte.numel(), dtype=torch.int64, device=rows.device)
    acc.index_add_(0, inverse, torch.ones_like(rows) << (rows & 7))  # distinct rows: distinct bits of a byte, so + is OR
    data[byte] = acc.to(torch.uint8)
    if invert:
        data[:nb] = ~data[:nb]
        if n % 8:
            data[nb - 1] &= (1 << (n % 8)) - 1
    return data


_POP = [bin(i).count("1") for i in range(256)]


def popcount(data, step=1 << 28):
    """the number of set bits of a uint8 tensor, as an int"""
    lut = torch.tensor(_POP, dtype=torch.int64, device=data.device)
    data = data.reshape(-1)
    return sum(int(lut[data[i: i + step].long()].sum().item()) for i in range(0, data.numel(), step))


def pack_values(v, c):
    """int64[m] values below 2^c -> their packed stream, uint8[ceil(m * c / 8)]: value i in bits [i * c, i * c + c) of a
    little-endian bit string, the bits behind the last value zero.  Eight values make c whole bytes; byte j of such a group is
    the OR of the parts of the values that overlap bits [8 j, 8 j + 8)"""
    m = v.numel()
    if m % 8:
        v = torch.cat([v, torch.zeros(8 - m % 8, dtype=v.dtype, device=v.device)])
    g = v.to(torch.int64).view(-1, 8)
    out = torch.zeros((g.shape[0], c), dtype=torch.uint8, device=v.device)
    for i in range(8):
        lo = i * c
        for j in range(lo // 8, (lo + c - 1) // 8 + 1):
            s = lo - 8 * j
            part = (g[:, i] << s) if s >= 0 else (g[:, i] >> -s)
            out[:, j] |= (part & 0xFF).to(torch.uint8)
    return out.view(-1)[: (m * c + 7) // 8]


def pred(v, op, a, b=0):
    between = (v >= a) & (v <= b)
    return {"==": v == a, "!=": v != a, "<": v < a, "<=": v <= a, ">": v > a, ">=": v >= a, "between": between, "not_between": ~between}[op]


def fit(r, co, miss):
    """r where it is a value of co bits, else miss -> (values int64, the number of rows replaced)"""
    bad = (r < 0) | (r >= (1 << co))
    return torch.where(bad, torch.full_like(r, miss), r), int(bad.sum().item())


def member(set_bytes, v, set_bits):
    """bool: v < set_bits and bit v of the bitmap set"""
    inside = v < set_bits
    idx = torch.where(inside, v, torch.zeros_like(v))
    bit = (set_bytes[idx >> 3].to(torch.int64) >> (idx & 7)) & 1
    return inside & (bit != 0)


def table_value(table, v, miss):
    """table[v] where v is an entry of the decoded table (int64[rows]), else miss"""
    inside = v < table.numel()
    idx = torch.where(inside, v, torch.zeros_like(v))
    return torch.where(inside, table[idx].to(torch.int64), torch.full_like(v, miss))


class Grouped:
    """sum, count, min, max of values per key in group_aggregate's layout (an empty group: 0, 0, -1 = ~0, 0), over slices; a row
    whose key is >= groups reaches no group and is counted in `dropped`.  Sums wrap like the uint64 they stand for"""

    def __init__(self, groups, device):
        self.groups, self.dropped = groups, 0
        self.sum = torch.zeros(groups, dtype=torch.int64, device=device)
        self.count = torch.zeros(groups, dtype=torch.int64, device=device)
        self.min = torch.full((groups,), (1 << 62), dtype=torch.int64, device=device)
        self.max = torch.full((groups,), -1, dtype=torch.int64, device=device)

    def step(self, keys, values, sel=None):
        if sel is not None:
            keys, values = keys[sel], values[sel]
        inside = keys < self.groups
        self.dropped += int((~inside).sum().item())
        if self.groups <= DENSE:  # a few groups: one masked reduction per group (scattering 2^27 rows onto a few words crawls)
            for g in range(self.groups):
                v = values[keys == g]
                if v.numel():
                    self.sum[g] += v.sum()
                    self.count[g] += v.numel()
                    self.min[g] = torch.minimum(self.min[g], v.min())
                    self.max[g] = torch.maximum(self.max[g], v.max())
            return
        keys, values = keys[inside], values[inside]
        self.sum.index_add_(0, keys, values)
        self.count += torch.bincount(keys, minlength=self.groups)
        self.min.scatter_reduce_(0, keys, values, "amin")
        self.max.scatter_reduce_(0, keys, values, "amax")

    def table(self):
        empty = self.count == 0
        mn = torch.where(empty, torch.full_like(self.min, -1), self.min)
        mx = torch.where(empty, torch.zeros_like(self.max), self.max)
        return torch.stack([self.sum, self.count, mn, mx], dim=1)


class RunningSum:
    """r_i = k + the sum of x_j + b over the selected rows j <= i (j < i when exclusive), over slices"""

    def __init__(self, b=0, k=0, exclusive=False):
        self.b, self.total, self.exclusive = b, k, exclusive

    def step(self, v, sel=None):
        term = v + self.b
        if sel is not None:
            term = torch.where(sel, term, torch.zeros_like(term))
        r = torch.cumsum(term, dim=0) + self.total
        self.total = int(r[-1].item())
        return r - term if self.exclusive else r


class Delta:
    """r_i = x_i - x_(i-1) + k with x_(-1) = first, over slices"""

    def __init__(self, first=0, k=0):
        self.prev, self.k = first, k

    def step(self, v):
        before = torch.cat([torch.tensor([self.prev], dtype=v.dtype, device=v.device), v[:-1]])
        self.prev = int(v[-1].item())
        return v - before + self.k


class Runs:
    """the runs of a column over slices -> values and ends (the row behind every run's last row), int64, in row order"""

    def __init__(self):
        self.values, self.ends, self.last, self.rows = [], [], None, 0

    def step(self, v):
        if self.last is not None and int(v[0].item()) != self.last:
            dev = v.device
            self.values.append(torch.tensor([self.last], dtype=torch.int64, device=dev))
            self.ends.append(torch.tensor([self.rows], dtype=torch.int64, device=dev))
        cut = torch.nonzero(v[1:] != v[:-1]).view(-1)  # row cut[j] of the slice is a run's last row
        self.values.append(v[cut])
        self.ends.append(cut + 1 + self.rows)
        self.last, self.rows = int(v[-1].item()), self.rows + v.numel()

    def tables(self):
        dev = self.values[0].device
        values = torch.cat(self.values + [torch.tensor([self.last], dtype=torch.int64, device=dev)])
        ends = torch.cat(self.ends + [torch.tensor([self.rows], dtype=torch.int64, device=dev)])
        return values, ends


def run_of_rows(ends, first, last):
    """for every row of [first, last) the number of ends <= the row: the run it lies in, len(ends) behind the last run"""
    rows = torch.arange(first, last, dtype=torch.int64, device=ends.device)
    return torch.searchsorted(ends, rows, right=True)


def run_decode(values, ends, first, last, miss):
    """the rows [first, last) of the column that the runs encode; miss behind the last run -> (values, rows behind the last run)"""
    j = run_of_rows(ends, first, last)
    out = table_value(values, j, miss)
    return out, int((j >= ends.numel()).sum().item())


def search_sorted(table, v, side="left", exact=False, miss=0):
    """-> (positions, found): numpy.searchsorted of v in the sorted int64 table; with exact a row that is not found gets miss"""
    left = torch.searchsorted(table, v, right=False)
    right = torch.searchsorted(table, v, right=True)
    found = right > left
    pos = left if side == "left" else right
    if exact:
        pos = torch.where(found, pos, torch.full_like(pos, miss))
    return pos, found


def top_k_result(hist, k, largest):
    """from the counts of the qualifying rows per value (int64[2^c]) -> [m, threshold, rows strictly beyond it, rows equal to it]"""
    counts = hist.tolist()
    total = sum(counts)
    m = min(k, total)
    if m == 0:
        return [0, 0, 0, 0]
    order = range(len(counts) - 1, -1, -1) if largest else range(len(counts))
    beyond = 0
    for value in order:
        if beyond + counts[value] >= m:
            return [m, value, beyond, counts[value]]
        beyond += counts[value]
    raise AssertionError("unreachable")


def top_k_result_wide(hist_high, hist_low_of, k, largest, low_bits=16):
    """top_k_result for values too wide for one table of counts, in two levels: hist_high counts the qualifying rows by
    value >> low_bits; hist_low_of(h) -> the counts by the low bits of the qualifying rows whose high part is h"""
    m, high, beyond_high, _ = top_k_result(hist_high, k, largest)
    if m == 0:
        return [0, 0, 0, 0]
    _, low, beyond_low, equal = top_k_result(hist_low_of(high), m - beyond_high, largest)
    return [m, (high << low_bits) | low, beyond_high + beyond_low, equal]


class TopK:
    """the bitmap of top_k over slices, from top_k_result: every qualifying row beyond the threshold, and of those equal to it the
    first m - beyond by row id"""

    def __init__(self, result, largest):
        self.m, self.T, beyond, _ = result
        self.left, self.largest = self.m - beyond, largest

    def step(self, v, qual=None):
        if qual is None:
            qual = torch.ones_like(v, dtype=torch.bool)
        if self.m == 0:
            return torch.zeros_like(qual)
        beyond = qual & ((v > self.T) if self.largest else (v < self.T))
        tie = qual & (v == self.T)
        rank = torch.cumsum(tie.to(torch.int64), dim=0)  # 1-based among this slice's ties
        take = tie & (rank <= self.left)
        self.left -= int(take.sum().item())
        return beyond | take


def sort_rows(rows, v, descending=False):
    """row ids and values of the qualifying rows (in row order) -> (row ids, values) by value, then by row id"""
    order = torch.sort(v, stable=True, descending=descending).indices
    return rows[order], v[order]


class KeyIndex:
    """the first or last selected row of every key < table_rows, over slices, and key_index's counts"""

    def __init__(self, table_rows, keep, device):
        self.table_rows, self.keep = table_rows, keep
        self.row = torch.full((table_rows,), (1 << 62) if keep == "first" else -1, dtype=torch.int64, device=device)
        self.outside = self.inside = 0

    def step(self, keys, first, sel=None):
        rows = torch.arange(first, first + keys.numel(), dtype=torch.int64, device=keys.device)
        if sel is not None:
            keys, rows = keys[sel], rows[sel]
        inside = keys < self.table_rows
        self.outside += int((~inside).sum().item())
        self.inside += int(inside.sum().item())
        if self.table_rows <= DENSE:  # as in Grouped
            for j in range(self.table_rows):
                r = rows[keys == j]
                if r.numel():
                    self.row[j] = torch.minimum(self.row[j], r[0]) if self.keep == "first" else torch.maximum(self.row[j], r[-1])
            return
        self.row.scatter_reduce_(0, keys[inside], rows[inside], "amin" if self.keep == "first" else "amax")

    def table(self, ct, miss, first_row=0):
        """-> (table int64[table_rows], [members, selected rows outside the table, inside it, members whose id did not fit])"""
        has = (self.row >= 0) & (self.row < (1 << 62))
        ids = self.row + first_row
        fits = has & (ids < (1 << ct))
        table = torch.where(fits, ids, torch.full_like(ids, miss))
        return table, [int(has.sum().item()), self.outside, self.inside, int((has & ~fits).sum().item())]


class SetRanks:
    """table[j] = the number of members below j when j is a member and that fits ct bits, else miss, over slices of the set's
    bits; counts = [members, members whose rank did not fit]"""

    def __init__(self, ct, miss):
        self.ct, self.miss, self.counts = ct, miss, [0, 0]

    def step(self, bits):
        rank = torch.cumsum(bits.to(torch.int64), dim=0) - 1 + self.counts[0]
        fits = bits & (rank < (1 << self.ct))
        self.counts[0] += int(bits.sum().item())
        self.counts[1] += int((bits & ~fits).sum().item())
        return torch.where(fits, rank, torch.full_like(rank, self.miss))


def value_set(flags, v, set_bits, sel=None):
    """marks in flags (bool[set_bits]) the values of the selected rows -> the number of selected rows whose value is >= set_bits"""
    if sel is not None:
        v = v[sel]
    inside = v < set_bits
    flags[v[inside]] = True
    return int((~inside).sum().item())


def aggregate(acc, v, sel=None):
    """folds a slice into acc = [sum, count, min, max] (python ints; start from [0, 0, -1, 0]; min -1 stands for no row yet)"""
    if sel is not None:
        v = v[sel]
    if v.numel() == 0:
        return acc
    lo, hi = int(v.min().item()), int(v.max().item())
    return [acc[0] + int(v.sum().item()), acc[1] + v.numel(), lo if acc[2] < 0 else min(acc[2], lo), max(acc[3], hi)]
