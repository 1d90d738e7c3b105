"""Geometry, generators and a plain numpy reference for chgpu_join_probe_chain (clickhouse_amd/csrc/join_chain.h).  No device here.

The constants restate the header's (tests/test_chain_cases.py reads them out of the header and compares, so a retune fails there
instead of moving every crafted case off its edge).  The reference does not go through oracle.HashJoin, so that it also serves tens of
millions of rows; test_chain_cases.py checks it against the oracle run join by join."""
from dataclasses import dataclass, field

import numpy as np

# ---- the chain's constants (join_chain.h) ---------------------------------------------------------------------------------------
JC_MAX_STEPS = 8
JC_MAX_CARRY = 8
JC_SLICE_BYTES = 142 * 1024
JC_SLICE_BITS = JC_SLICE_BYTES * 8
JC_MAX_SLICES = 4
JC_QPT = 16
JC_THREADS = 1024
JCT_QUEUE = 1024
JCT_COAL_MIN = 96
JCT_WAVES = 4
LDS_MIN_ROWS = 1 << 20      # below this many probe rows no step takes the LDS sweep
KEYSET_LIMIT = 1 << 25      # a key set / a dense prefilter exists for build sides whose largest key is below this

PART_ROWS = JC_THREADS * JC_QPT * 4       # rows one workgroup of k_chain_lds takes per turn
UNIT_ROWS = 64 * JC_QPT * 4               # rows of one wave of a part = what one wave of k_chain_tail / k_chain_indexes takes per turn
UNITS_PER_PART = JC_THREADS // 64
QUARTER_ROWS = UNIT_ROWS // 4
LDS_MAX_KEY = JC_MAX_SLICES * JC_SLICE_BITS - 1   # the largest max_key whose bitmap still fits the LDS sweep (dense_bits <= 4 slices)

JOIN_INNER, JOIN_LEFT = 0, 1
STRICT_ANY, STRICT_ALL, STRICT_SEMI, STRICT_ANTI = 0, 1, 2, 3
NO_ROW = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---- geometry -------------------------------------------------------------------------------------------------------------------
def dense_bits(max_key: int) -> int:
    """bits of the step's bitmap: a multiple of 32 above the largest key"""
    return (max_key + 32) // 32 * 32


def n_slices(max_key: int) -> int:
    return (dense_bits(max_key) + JC_SLICE_BITS - 1) // JC_SLICE_BITS


def slice_ranges(max_key: int):
    """[(lo, nb)] of every LDS slice of the bitmap"""
    db = dense_bits(max_key)
    return [(s * JC_SLICE_BITS, min(JC_SLICE_BITS, db - s * JC_SLICE_BITS)) for s in range(n_slices(max_key))]


def fits_lds(max_key: int) -> bool:
    return max_key < KEYSET_LIMIT and dense_bits(max_key) <= JC_MAX_SLICES * JC_SLICE_BITS


def unit_row(lane, bit):
    """row inside a unit of bit `bit` (= 4 * kb + b) of lane `lane`'s alive word: (kb * 64 + lane) * 4 + b"""
    return ((bit >> 2) * 64 + lane) * 4 + (bit & 3)


def unit_lane_bit(row):
    """inverse of unit_row: (lane, bit) of a row offset inside a unit"""
    quad, b = row >> 2, row & 3
    return quad & 63, 4 * (quad >> 6) + b


def quarter_rows(quarter: int) -> np.ndarray:
    """the unit's row offsets whose bits live in bits [16 * quarter, 16 * quarter + 16) of the lane words (one queue pass of k_chain_tail)"""
    lane, bit = np.meshgrid(np.arange(64), np.arange(16 * quarter, 16 * quarter + 16), indexing="ij")
    return np.sort(unit_row(lane, bit).ravel())


def locate(row: int) -> dict:
    """where a row lives: what a failing case prints for its first differing row"""
    off = row % UNIT_ROWS
    lane, bit = unit_lane_bit(off)
    return dict(row=row, part=row // PART_ROWS, unit=row // UNIT_ROWS, wave=(row // UNIT_ROWS) % UNITS_PER_PART, lane=int(lane), bit=int(bit),
                quarter=int(bit) // 16)


def alive_per_unit_quarter(alive: np.ndarray) -> np.ndarray:
    """[units, 4] alive rows per unit and quarter (the last unit padded with dead rows)"""
    n = alive.shape[0]
    units = (n + UNIT_ROWS - 1) // UNIT_ROWS
    a = np.zeros(units * UNIT_ROWS, dtype=bool)
    a[:n] = alive
    a = a.reshape(units, UNIT_ROWS)
    return np.stack([a[:, quarter_rows(q)].sum(axis=1) for q in range(4)], axis=1)


def kept_per_part(flt: np.ndarray) -> np.ndarray:
    n = flt.shape[0]
    parts = (n + PART_ROWS - 1) // PART_ROWS
    return np.add.reduceat(flt.astype(np.int64), np.arange(parts) * PART_ROWS) if n else np.zeros(0, dtype=np.int64)


# ---- the reference --------------------------------------------------------------------------------------------------------------
def canon(keys: np.ndarray) -> np.ndarray:
    """keys as the join compares them: the column's bytes zero-extended (a negative Int32 matches itself and nothing else)"""
    keys = np.ascontiguousarray(keys)
    return keys.view(np.dtype(f"u{keys.dtype.itemsize}"))


@dataclass
class Step:
    kind: int
    strictness: int
    build: list                      # [(keys, null_map | None, join_mask | None)] per build block; [] = no block at all
    probe: np.ndarray
    null_map: np.ndarray = None      # of the probe column
    dtype: np.dtype = field(default=None)
    _index: tuple = field(default=None, repr=False, compare=False)   # build_index's result, shared by the copies `on` makes

    def on(self, probe, null_map=None, kind=None, strictness=None):
        """the same build side (and its sorted index) probed with another column, or under another kind / strictness"""
        st = Step(self.kind if kind is None else kind, self.strictness if strictness is None else strictness, self.build, probe, null_map, self.dtype)
        build_index(self)
        st._index = self._index
        return st

    def __post_init__(self):
        self.dtype = np.dtype(self.probe.dtype if self.dtype is None else self.dtype)
        self.build = [b if isinstance(b, tuple) else (b, None, None) for b in self.build]

    @property
    def filters(self) -> bool:       # LEFT ANY / LEFT ALL keep every left row
        return self.kind == JOIN_INNER or self.strictness in (STRICT_SEMI, STRICT_ANTI)


def build_index(step: Step):
    """(sorted distinct valid build keys as u64, the (block << 32 | row) id of the FIRST valid row holding each, any key twice)"""
    if step._index is not None:
        return step._index
    ks, ids = [], []
    for b, (keys, nm, jm) in enumerate(step.build):
        k = canon(np.asarray(keys, dtype=step.dtype)).astype(np.uint64)
        valid = np.ones(k.shape[0], dtype=bool)
        if nm is not None:
            valid &= np.asarray(nm) == 0
        if jm is not None:
            valid &= np.asarray(jm) != 0
        rows = np.flatnonzero(valid).astype(np.uint64)
        ks.append(k[valid])
        ids.append((np.uint64(b) << np.uint64(32)) | rows)
    if not ks:
        ks, ids = [np.zeros(0, dtype=np.uint64)], [np.zeros(0, dtype=np.uint64)]
    k, i = np.concatenate(ks), np.concatenate(ids)
    order = np.argsort(k, kind="stable")          # stable: the first inserted row of a key comes first
    k, i = k[order], i[order]
    first = np.ones(k.shape[0], dtype=bool)
    first[1:] = k[1:] != k[:-1]
    step._index = (k[first], i[first], bool((~first).any()))
    return step._index


def build_stats(step: Step):
    """(max_key, has_zero) over the valid build rows: what the chain sizes the step's bitmap by"""
    uk, _, _ = build_index(step)
    return (int(uk[-1]) if uk.shape[0] else 0), bool(uk.shape[0] and uk[0] == 0)


def _present(uk: np.ndarray, probe: np.ndarray) -> np.ndarray:
    if uk.shape[0] == 0:
        return np.zeros(probe.shape[0], dtype=bool)
    top = int(uk[-1])
    if top < (1 << 28):                            # a boolean presence table over the build keys
        table = np.zeros(top + 2, dtype=bool)
        table[uk.astype(np.int64)] = True
        if top + 1 > np.iinfo(probe.dtype).max:    # every value of the type indexes the table
            return table[probe]
        return table[np.minimum(probe, probe.dtype.type(top + 1))]
    p = probe.astype(np.uint64)                    # wide keys: binary search in the sorted distinct build keys
    pos = np.searchsorted(uk, p)
    pos[pos == uk.shape[0]] = 0
    return uk[pos] == p


def step_found(step: Step) -> np.ndarray:
    """found = not null and present (HashJoinMethodsImpl.h:451-452)"""
    uk, _, _ = build_index(step)
    found = _present(uk, canon(step.probe))
    if step.null_map is not None:
        found &= np.asarray(step.null_map) == 0
    return found


def step_filter(step: Step) -> np.ndarray:
    if not step.filters:
        return np.ones(step.probe.shape[0], dtype=bool)
    found = step_found(step)
    return ~found if step.strictness == STRICT_ANTI else found


def step_rowids(step: Step, idx: np.ndarray) -> np.ndarray:
    """the matched build row of every survivor: (block << 32) | row, NO_ROW at a miss, under a null and for every row of an ANTI step"""
    out = np.full(idx.shape[0], NO_ROW, dtype=np.uint64)
    if step.strictness == STRICT_ANTI or idx.shape[0] == 0:
        return out
    uk, ids, _ = build_index(step)
    if uk.shape[0] == 0:
        return out
    p = canon(step.probe)[idx].astype(np.uint64)
    pos = np.searchsorted(uk, p)
    pos[pos == uk.shape[0]] = 0
    hit = uk[pos] == p
    if step.null_map is not None:
        hit &= np.asarray(step.null_map)[idx] == 0
    out[hit] = ids[pos[hit]]
    return out


def chain_reference(steps, carries=(), payloads=None) -> dict:
    """filter = AND over the filtering steps; indexes ascending; per step the matched row id; carried columns at the survivors;
    payloads[s] (one-block build sides): the column's value at the matched row, 0 at a miss"""
    n = steps[0].probe.shape[0]
    flt = np.ones(n, dtype=bool)
    for st in steps:
        assert st.probe.shape[0] == n
        flt &= step_filter(st)
    idx = np.flatnonzero(flt)
    rowids = [step_rowids(st, idx) for st in steps]
    out = dict(filter=flt, kept=int(idx.shape[0]), indexes=idx.astype(np.uint64), rowids=rowids, carry=[np.asarray(c)[idx] for c in carries])
    if payloads is not None:
        pay = []
        for rid, col in zip(rowids, payloads):
            if col is None:
                pay.append(None)
                continue
            miss = rid == NO_ROW
            row = np.where(miss, np.uint64(0), rid & np.uint64(0xFFFFFFFF)).astype(np.int64)
            vals = col[row] if col.shape[0] else np.zeros(row.shape[0], dtype=col.dtype)
            pay.append(np.where(miss, col.dtype.type(0), vals).astype(col.dtype))
        out["payload"] = pay
    return out


# ---- generators -----------------------------------------------------------------------------------------------------------------
def slice_edge_keys(max_key: int) -> np.ndarray:
    """the keys where the sweep's arithmetic turns: both ends of every slice and their neighbours, the bitmap's end, the wrapped ones"""
    ks = {0, 1, max_key - 1, max_key, max_key + 1, dense_bits(max_key) - 1, dense_bits(max_key), dense_bits(max_key) + 1, 1 << 31, (1 << 31) - 1, (1 << 31) + 1,
          0xFFFFFFFF, 0xFFFFFFFE, KEYSET_LIMIT - 1, KEYSET_LIMIT}
    for s in range(JC_MAX_SLICES + 1):
        lo = s * JC_SLICE_BITS
        ks |= {lo - 1, lo, lo + 1, lo + 31, lo + 32}
    for lo, nb in slice_ranges(max_key):
        ks |= {lo - 1, lo, lo + nb - 1, lo + nb}
    return np.array(sorted(k for k in ks if 0 <= k <= 0xFFFFFFFF), dtype=np.uint32)


def build_keys(rng, max_key: int, count: int, with_zero: bool, must=(), avoid=()) -> np.ndarray:
    """`count` distinct nonzero keys <= max_key in random order: max_key itself, every key of `must` that fits, none of `avoid`; the zero
    key on top when asked for"""
    must = {int(k) for k in must if 0 < int(k) <= max_key} | {max_key}
    avoid = {int(k) for k in avoid} - {max_key}
    must -= avoid
    count = max(count, len(must))
    assert count <= max_key - len(avoid)
    have = np.array(sorted(must), dtype=np.uint64)
    while have.shape[0] < count:
        more = rng.integers(1, max_key, size=count - have.shape[0] + 64, endpoint=True, dtype=np.uint64)
        if avoid:
            more = more[~np.isin(more, np.array(sorted(avoid), dtype=np.uint64))]
        have = np.unique(np.concatenate([have, more]))
    extra = np.setdiff1d(have, np.array(sorted(must), dtype=np.uint64))
    keep = np.concatenate([np.array(sorted(must), dtype=np.uint64), rng.permutation(extra)[:count - len(must)]])
    if with_zero:
        keep = np.concatenate([keep, np.zeros(1, dtype=np.uint64)])
    return rng.permutation(keep)


def alternating_edge_build(rng, max_key: int, count: int, with_zero: bool) -> np.ndarray:
    """a build side that holds every second edge key of slice_edge_keys(max_key) and provably none of the others: each edge is probed as
    a hit next to a miss"""
    e = [int(k) for k in slice_edge_keys(max_key) if 0 < k < max_key]
    return build_keys(rng, max_key, min(count, max_key - len(e[1::2])), with_zero, must=e[0::2], avoid=e[1::2])


def probe_mix(rng, n: int, bk: np.ndarray, hit_rate, miss_top: int, dtype=np.uint32) -> np.ndarray:
    """n probe keys: with probability hit_rate (a scalar, or one value per row) a build key, otherwise a random key in [0, miss_top]"""
    bk = np.asarray(bk)
    draw = np.uint32 if miss_top <= 0xFFFFFFFF else np.uint64
    other = rng.integers(0, miss_top, size=n, endpoint=True, dtype=draw).astype(dtype, copy=False)
    if bk.shape[0] == 0:
        return other
    hit = rng.random(n, dtype=np.float32) < hit_rate
    other[hit] = bk[rng.integers(0, bk.shape[0], size=int(hit.sum()))].astype(dtype)
    return other


def plant(rng, probe: np.ndarray, keys, copies: int = 3, rows=None) -> np.ndarray:
    """every key of `keys` written `copies` times at random rows of `probe` (or at `rows`, cycling through the keys); returns the rows"""
    keys = np.asarray(keys).astype(probe.dtype)
    if rows is None:
        rows = rng.choice(probe.shape[0], size=min(probe.shape[0], keys.shape[0] * copies), replace=False)
    rows = np.asarray(rows)
    probe[rows] = np.resize(keys, rows.shape[0])
    return rows


def per_part_rates(n: int, lo: float = 0.15, hi: float = 0.95, salt: int = 0) -> np.ndarray:
    """one hit rate per row, constant inside a part and different between neighbouring parts and between parts a grid apart: a sweep that
    reads another part's keys changes the number of survivors of the part, not just which rows survive"""
    parts = (n + PART_ROWS - 1) // PART_ROWS
    p = np.arange(parts, dtype=np.int64) + 7919 * salt
    rate = lo + (hi - lo) * (((p * 2654435761) % 1009) / 1008.0)
    return np.repeat(rate.astype(np.float32), PART_ROWS)[:n]


def unit_alive_column(rng, n: int, hit_key: int, miss_key: int, plan: dict, fill_rate: float = 0.5, dtype=np.uint32) -> np.ndarray:
    """A probe column for a SEMI step whose build side holds hit_key and not miss_key.  plan: {unit: (a0, a1, a2, a3) | total}: the unit
    gets exactly a_q alive rows in quarter q (a total is spread over the quarters at random), at random places of the quarter (through
    the row mapping of the alive words).  Other units: every row alive with probability fill_rate."""
    col = np.where(rng.random(n) < fill_rate, hit_key, miss_key).astype(dtype)
    for unit, want in plan.items():
        base = unit * UNIT_ROWS
        assert base + UNIT_ROWS <= n, "planned units are whole units"
        if np.isscalar(want):
            pick = rng.choice(UNIT_ROWS, size=int(want), replace=False)
            want = tuple(int(np.isin(pick, quarter_rows(q)).sum()) for q in range(4))
        col[base:base + UNIT_ROWS] = miss_key
        for q, a in enumerate(want):
            rows = quarter_rows(q)
            col[base + rng.choice(rows, size=int(a), replace=False)] = hit_key
    return col
