"""Reference for uniqExact / count(DISTINCT) under GROUP BY: a set of (key bits, value bits), plain Python and numpy.

Two values are the same when their bits are (the reference's HashSet cell compares with bitEquals): +0.0 and -0.0 are two values, two
NaNs with one payload are one, NaNs with different payloads differ, and a Float32 is its 32 bits, not the Float64 it widens to.  Keys
are their bits zero-extended to 64.  A row enters when its filter byte is non-zero; a group exists only through a row that entered."""
import numpy as np

_UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def bits(arr):
    """the raw bits of every element, zero-extended to uint64"""
    arr = np.ascontiguousarray(arr)
    return arr.view(_UNSIGNED[arr.dtype.itemsize]).astype(np.uint64)


def from_bits(words, dtype):
    """the inverse of bits() for values that came from `dtype`"""
    dtype = np.dtype(dtype)
    return np.asarray(words, dtype=np.uint64).astype(_UNSIGNED[dtype.itemsize]).view(dtype)


class UniqExactRef:
    def __init__(self, key_dtype, value_dtype):
        self.key_dtype = None if key_dtype is None else np.dtype(key_dtype)
        self.value_dtype = np.dtype(value_dtype)
        self.pairs = set()   # {(key bits, value bits)}; without key the key bits are 0

    def add(self, keys, values, row_begin=0, row_end=None, filter=None):
        values = np.asarray(values)
        assert values.dtype == self.value_dtype
        row_end = len(values) if row_end is None else row_end
        v = bits(values)[row_begin:row_end]
        if self.key_dtype is None:
            k = np.zeros(len(v), dtype=np.uint64)
        else:
            keys = np.asarray(keys)
            assert keys.dtype == self.key_dtype and len(keys) == len(values)
            k = bits(keys)[row_begin:row_end]
        if filter is not None:
            keep = np.asarray(filter, dtype=np.uint8)[row_begin:row_end] != 0
            k, v = k[keep], v[keep]
        self.pairs.update(zip(k.tolist(), v.tolist()))
        return self

    def merge(self, other):
        assert (self.key_dtype, self.value_dtype) == (other.key_dtype, other.value_dtype)
        self.pairs |= other.pairs
        return self

    def __len__(self):
        return len(self.pairs)

    def finalize(self):
        """{key bits: distinct values}; without key {None: size}, also for the empty set"""
        if self.key_dtype is None:
            return {None: len(self.pairs)}
        out = {}
        for k, _ in self.pairs:
            out[k] = out.get(k, 0) + 1
        return out

    def counts_for_keys(self, keys):
        """per row of keys its distinct count, 0 for a key the set lacks"""
        fin = self.finalize()
        return np.array([fin.get(k, 0) for k in bits(np.asarray(keys, dtype=self.key_dtype)).tolist()], dtype=np.uint64)
