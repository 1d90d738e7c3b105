"""DISTINCT / LIMIT n OFFSET m BY on the CPU: the reference of tests/test_gpu_limit_by.py.

LimitByTransform::transform, with the key itself in place of its SipHash128: walk the rows in row order; a row whose filter byte is zero
gets 0 and counts nowhere; any other row reads its key's counter c; if c < offset + length the counter becomes c + 1 and the row passes
iff c >= offset, else the row gets 0.  Counters persist over blocks.  DISTINCT is length 1, offset 0.  A key is the column's raw bits
zero-extended to 64 bits.  Two forms: a plain loop (LimitByLoop) and a vectorised one (LimitByRef: stable argsort by key, rank within
run, carry dictionary); test_limit_by_ref.py holds them against each other."""
import numpy as np

# the constants of clickhouse_amd/csrc/limit_by_host.h the GPU tests straddle (test_limit_by_ref.py asserts they agree)
LB_TILE = 1024
LB_CAP_MIN = 2048
LB_NONE = 0xFFFFFFFF

KEY_DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64]
_UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}

# (length, offset, blocks of keys, the filter of every block): the reference restated by hand
VECTORS = [
    (1, 0, [[5, 5, 7, 0, 7, 0], [0, 9, 5, 9]], [[1, 0, 1, 1, 0, 0], [0, 1, 0, 0]]),
    (2, 1, [[1, 1, 1, 1, 2, 2], [2, 2, 1, 3, 3, 3, 3]], [[0, 1, 1, 0, 0, 1], [1, 0, 0, 0, 1, 1, 0]]),
]


def bits(keys):
    """the raw bits of an integer array, zero-extended to UInt64"""
    keys = np.ascontiguousarray(keys)
    return keys.view(_UNSIGNED[keys.dtype.itemsize]).astype(np.uint64)


class LimitByLoop:
    """the definition, row by row"""

    def __init__(self, length, offset=0):
        self.length, self.offset = int(length), int(offset)
        self.count = {}

    def filter_block(self, keys, row_begin=0, row_end=None, filter=None):
        keys = bits(keys)
        row_end = keys.shape[0] if row_end is None else row_end
        out = np.zeros(row_end - row_begin, dtype=np.uint8)
        bound = self.offset + self.length
        for i in range(row_begin, row_end):
            if filter is not None and filter[i] == 0:
                continue
            k = int(keys[i])
            c = self.count.get(k, 0)
            if c < bound:
                self.count[k] = c + 1
                out[i - row_begin] = c >= self.offset
        return out, int(out.sum())

    def keys(self):
        return sum(1 for c in self.count.values() if c > 0)


class LimitByRef:
    """the same, vectorised: a row's occurrence number is its key's carried counter + its rank among the block's entered rows of that key"""

    def __init__(self, length, offset=0):
        self.length, self.offset = int(length), int(offset)
        self.count = {}

    def filter_block(self, keys, row_begin=0, row_end=None, filter=None):
        keys = bits(keys)
        row_end = keys.shape[0] if row_end is None else row_end
        n = row_end - row_begin
        out = np.zeros(n, dtype=np.uint8)
        k = keys[row_begin:row_end]
        rows = np.arange(n) if filter is None else np.flatnonzero(np.asarray(filter)[row_begin:row_end] != 0)
        if rows.shape[0] == 0:
            return out, 0
        k = k[rows]
        order = np.argsort(k, kind="stable")
        sk = k[order]
        head = np.concatenate(([True], sk[1:] != sk[:-1]))
        starts = np.flatnonzero(head)
        seg = np.cumsum(head) - 1
        rank = np.arange(sk.shape[0]) - starts[seg]
        lens = np.diff(np.concatenate((starts, [sk.shape[0]])))
        bound = self.offset + self.length
        carry = np.fromiter((self.count.get(int(x), 0) for x in sk[starts]), dtype=np.int64, count=starts.shape[0])
        occ = carry[seg] + rank
        out[rows[order]] = (occ >= self.offset) & (occ < bound)
        for x, c, ln in zip(sk[starts], carry, lens):
            self.count[int(x)] = min(int(c) + int(ln), bound)
        return out, int(out.sum())

    def keys(self):
        return sum(1 for c in self.count.values() if c > 0)
