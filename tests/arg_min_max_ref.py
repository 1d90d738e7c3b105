"""argMin(arg, val) / argMax(arg, val) restated in row order: AggregateFunctionArgMinMax.h `add` / `merge` / `insertResultInto` over
SingleValueDataFixed (SingleValueData.cpp setIfGreater / setIfSmaller), one state per key, plain numpy and Python ints.

A state is `{has, val key, arg}`.  The val key is the device's convention (include/chgpu.h, CHGPU_AGG_ARG_MIN): val mapped to an
unsigned 64-bit integer that sorts like val -- unsigned: itself; signed: sign bit flipped; floats: the IEEE total-order fold after the
zero's sign is folded away (the reference's > and < call the two zeros equal), Float32 after its exact widening -- and complemented for
argMin, so both functions are "strictly greater key replaces".  NaN therefore has its total-order place, the documented deviation.
`arg` is kept as the raw bits of the row's value (a numpy scalar of arg's dtype), never as a number: a NaN payload or a -0.0 comes
back as it went in.

This module is the reference of tests/test_gpu_arg_min_max.py; tests/test_arg_min_max_ref.py pins it on hand-written cases."""
import numpy as np

M64 = (1 << 64) - 1
SIGN = 1 << 63


def val_key_array(val, is_min):
    """the order keys of a val column as a uint64 array (complemented for argMin)"""
    v = np.asarray(val)
    if v.dtype.kind == "f":
        bits = v.astype(np.float64).view(np.uint64).copy()
        bits[(bits << np.uint64(1)) == 0] = 0  # -0.0 == +0.0
        neg = (bits >> np.uint64(63)) != 0
        keys = np.where(neg, ~bits, bits ^ np.uint64(SIGN))
    elif v.dtype.kind == "i":
        keys = v.astype(np.int64).view(np.uint64) ^ np.uint64(SIGN)
    else:
        keys = v.astype(np.uint64)
    return ~keys if is_min else keys


def val_keys(val, is_min):
    """the same as Python ints"""
    return [int(k) for k in val_key_array(val, is_min)]


class State:
    """SingleValueDataFixed result + value of one group"""
    __slots__ = ("has", "key", "arg")

    def __init__(self):
        self.has, self.key, self.arg = False, 0, None

    def add(self, key, arg):
        if not self.has or key > self.key:  # setIfGreater / setIfSmaller: strictly
            self.has, self.key, self.arg = True, key, arg

    def merge(self, other):
        if other.has and (not self.has or other.key > self.key):
            self.has, self.key, self.arg = True, other.key, other.arg

    def copy(self):
        s = State()
        s.has, s.key, s.arg = self.has, self.key, self.arg
        return s


class Ref:
    """one argMin or argMax aggregate over keyed rows; keys None = without key (one group, key None)"""

    def __init__(self, is_min, arg_dtype):
        self.is_min = bool(is_min)
        self.arg_dtype = np.dtype(arg_dtype)
        self.states = {}

    def add_block(self, keys, arg, val, mask=None, row_begin=0, row_end=None):
        arg = np.asarray(arg)
        n = len(arg)
        row_end = n if row_end is None else row_end
        vk = val_keys(val, self.is_min)
        kl = [None] * n if keys is None else [int(k) for k in np.asarray(keys)]
        for i in range(row_begin, row_end):
            if mask is not None and not mask[i]:
                continue
            self.states.setdefault(kl[i], State()).add(vk[i], arg[i])

    def add_block_find_only(self, keys, arg, val, overflow):
        """a no_more_keys block: a key the table lacks goes to the State `overflow`, or is dropped when that is None"""
        arg = np.asarray(arg)
        vk = val_keys(val, self.is_min)
        for i, k in enumerate(int(k) for k in np.asarray(keys)):
            st = self.states.get(k, overflow)
            if st is not None:
                st.add(vk[i], arg[i])

    def merge(self, other, find_only=False, overflow=None):
        """mergeDataImpl in the source's key order (dict order = insertion order); find_only: mergeDataNoMoreKeysImpl"""
        for k, st in other.states.items():
            if find_only and k not in self.states:
                if overflow is not None:
                    overflow.merge(st)
                continue
            self.states.setdefault(k, State()).merge(st)

    def result_of(self, state):
        """insertResultInto: arg, or arg's default for a state without a value"""
        return state.arg if state is not None and state.has else self.arg_dtype.type(0)

    def result(self):
        """{key: arg as a numpy scalar}"""
        return {k: self.result_of(st) for k, st in self.states.items()}

    def result_bytes(self):
        return {k: np.asarray(v, dtype=self.arg_dtype).tobytes() for k, v in self.result().items()}


def group_reference_arrays(keys, arg, val, is_min, mask=None):
    """one block, vectorised (the large shapes): (group keys ascending, row index of each group's winner) -- the first row among those
    that hold the extremum"""
    keys = np.asarray(keys)
    vk = val_key_array(val, is_min)
    rows = np.arange(len(keys)) if mask is None else np.flatnonzero(mask)
    # sort by (key, val key descending, row ascending): the first of every key run wins
    order = rows[np.lexsort((rows, ~vk[rows], keys[rows]))]
    k_sorted = keys[order]
    first = np.ones(len(order), dtype=bool)
    first[1:] = k_sorted[1:] != k_sorted[:-1]
    return k_sorted[first], order[first]


def group_reference(keys, arg, val, is_min, mask=None):
    """{key: row index of the winner}"""
    k, r = group_reference_arrays(keys, arg, val, is_min, mask)
    return dict(zip(k.tolist(), r.tolist()))
