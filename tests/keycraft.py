"""Key sets with a chosen placement for the hash-placed GROUP BY and join plans, the wide-key dictionary and the String dictionary.

Every placement function below copies one in the HIP sources, and each is a bijection of the key (xorshift-33 is its own inverse on
64 bits, the multipliers are odd), so a key with a chosen home slot, slice, partition or LDS cell is made by inverting it rather than
by searching.  A plain helper module for the tests, numpy only."""
import numpy as np

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1

# intHash64, the join table's placement: chgpu_internal.h:232 and :234 (dev_intHash64)
INTHASH_MUL1 = 0xFF51AFD7ED558CCD
INTHASH_MUL2 = 0xC4CEB9FE1A85EC53
# the radix join's placement: join_kernels.hip:2554 (join_radix_slot)
RADIX_MULT = 0x9E3779B97F4A7C15
# the join's slice geometry: join_kernels.hip:2546 (JPL2_LG_CELLS, JPL2_TAIL, JPL2_TILE = jpart_sort_tile(false), JPL2_LG_P1) and
# join_kernels.hip:1320 (JBS_TILE = jpart_sort_tile(true), JBS_MAX_OVERFLOW)
LG_SLICE_CELLS = 12
SLICE_CELLS = 1 << LG_SLICE_CELLS
SLICE_TAIL = 256
PROBE_TILE = 16384
BUILD_TILE = 8192
LG_P1 = 6
MAX_OVERFLOW = 1 << 20
# the lg_cap range the LDS-staged probe, the slice build and the radix join take: join_kernels.hip:2546 (JPL2_LG_CELLS + JPL2_LG_P1 .. + 7)
LG_CAP_MIN = LG_SLICE_CELLS + LG_P1
LG_CAP_MAX = LG_SLICE_CELLS + LG_P1 + 7
# the region probe: join_kernels.hip:2242 (JPR_MAX_REGIONS) and :2478 (R doubles from 8 while a region exceeds region_kib)
MAX_REGIONS = 512
# GROUP BY partitions and LDS cells: agg_kernels.hip:658 (GBP_MULT), :659 (GBP_MULT1); 64-bit keys :661 / :680, 32-bit keys :670 / :678
GBP_MULT = 0x9E3779B97F4A7C15
GBP_MULT1 = 0xC2B2AE3D27D4EB4F


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def _mul(x, c):
    return _u64(x) * np.uint64(c)  # wraps mod 2^64


def inv_odd(c, bits=64):
    """the inverse of an odd constant mod 2^bits"""
    assert c & 1
    return pow(c, -1, 1 << bits)


def _xs33(x):
    x = _u64(x)
    return x ^ (x >> np.uint64(33))  # its own inverse: the shifted-in half never reaches the bits it came from


# ---- join ---------------------------------------------------------------------------------------------------------------------
def int_hash64(x):
    """dev_intHash64 (the murmur finalizer)"""
    x = _xs33(x)
    x = _xs33(_mul(x, INTHASH_MUL1))
    return _xs33(_mul(x, INTHASH_MUL2))


def int_hash64_inv(h):
    x = _mul(_xs33(h), inv_odd(INTHASH_MUL2))
    x = _mul(_xs33(x), inv_odd(INTHASH_MUL1))
    return _xs33(x)


def pow2ceil(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def join_capacity_for(rows, cap_shift=1):
    """join_capacity_for: pow2ceil(n + 3n/7 + 1) << 1 cells"""
    return pow2ceil(rows + rows * 3 // 7 + 1) << cap_shift


def join_lg_cap(rows):
    return join_capacity_for(rows).bit_length() - 1


def join_home(keys, lg_cap):
    """the table's home slot: intHash64(key) & (cap - 1)"""
    return int_hash64(keys) & np.uint64((1 << lg_cap) - 1)


def radix_slot(keys, lg_cap):
    """join_radix_slot: the top lg_cap bits of key * RADIX_MULT"""
    return _mul(keys, RADIX_MULT) >> np.uint64(64 - lg_cap)


def radix_slot_inv(slots, lg_cap, low):
    """keys whose radix slot is `slots`; `low` fills the 64 - lg_cap product bits below it"""
    y = (_u64(slots) << np.uint64(64 - lg_cap)) | (_u64(low) & np.uint64((1 << (64 - lg_cap)) - 1))
    return _mul(y, inv_odd(RADIX_MULT))


def partition_of_slot(slots, lg_cap, lg_p=LG_P1):
    """first-level partition (of 2^lg_p) of a home / radix slot: its top bits"""
    return _u64(slots) >> np.uint64(lg_cap - lg_p)


def region_count(lg_cap, region_kib=1024):
    """R of join_probe_agg_regions"""
    r = 8
    while r < MAX_REGIONS and ((1 << lg_cap) * 16) // r > region_kib * 1024:
        r <<= 1
    return r


def _distinct_free(rng, n, bits, exclude=()):
    """n distinct random integers below 2^bits, none in `exclude`"""
    assert bits >= 1 and n + len(exclude) <= (1 << bits)
    got = np.empty(0, dtype=np.uint64)
    ex = _u64(list(exclude))
    while got.shape[0] < n:
        more = rng.integers(0, 1 << bits, size=2 * (n - got.shape[0]) + 16, dtype=np.uint64) if bits < 64 else \
            rng.integers(0, 2**64 - 1, size=2 * (n - got.shape[0]) + 16, dtype=np.uint64, endpoint=True)
        got = np.unique(np.concatenate([got, more]))
        if ex.shape[0]:
            got = got[~np.isin(got, ex)]
    return rng.permutation(got)[:n]


def _keys_from_slots(rng, slots, lg_cap, placement):
    """one distinct nonzero key per entry of `slots` (slots may repeat), placed there by intHash64 ('hash') or the radix multiply ('radix')"""
    slots = _u64(slots)
    n = slots.shape[0]
    for _ in range(8):
        hi = _distinct_free(rng, n, 64 - lg_cap)  # the free bits of the hash value: distinct, so the keys are distinct whatever the slots
        if placement == "hash":
            keys = int_hash64_inv((hi << np.uint64(lg_cap)) | slots)
        else:
            keys = radix_slot_inv(slots, lg_cap, hi)
        if not np.any(keys == 0):
            return keys
    raise AssertionError("could not avoid the zero key")


def keys_at_slots(rng, slots, lg_cap, placement="hash"):
    """distinct nonzero keys, key i placed at slots[i]"""
    return _keys_from_slots(rng, slots, lg_cap, placement)


def keys_in_partition(rng, n, lg_cap, part, placement="hash", lg_p=LG_P1):
    """n distinct keys, all in first-level partition `part` (of 2^lg_p)"""
    span = 1 << (lg_cap - lg_p)
    slots = np.uint64(part * span) + rng.integers(0, span, size=n, dtype=np.uint64)
    return _keys_from_slots(rng, slots, lg_cap, placement)


def keys_in_partitions(rng, counts, lg_cap, placement="hash", lg_p=LG_P1):
    """{partition: n}: e.g. {p: few, p + 2: many} with p + 1 empty, so that a tile spans three partitions"""
    return np.concatenate([keys_in_partition(rng, n, lg_cap, p, placement, lg_p) for p, n in counts.items()])


def keys_in_slice(rng, n, lg_cap, slice_no, placement="hash"):
    """n distinct keys whose home slots all lie in one 4096-cell slice"""
    slots = np.uint64(slice_no * SLICE_CELLS) + rng.integers(0, SLICE_CELLS, size=n, dtype=np.uint64)
    return _keys_from_slots(rng, slots, lg_cap, placement)


def keys_at_slice_end(rng, n, lg_cap, slice_no, last_cells=1, placement="hash"):
    """n distinct keys homed in the last `last_cells` cells of a slice: their linear-probing chain runs on into the cells behind it
    (the LDS probe stages JPL2_TAIL = 256 of them)"""
    slots = np.uint64((slice_no + 1) * SLICE_CELLS - last_cells) + rng.integers(0, last_cells, size=n, dtype=np.uint64)
    return _keys_from_slots(rng, slots, lg_cap, placement)


def keys_in_region(rng, n, lg_cap, region, regions, placement="hash"):
    lg_r = regions.bit_length() - 1
    return keys_in_partition(rng, n, lg_cap, region, placement, lg_r)


def linear_probe_cells(homes, cap):
    """the cells a linear-probing table fills for keys with these home slots (the set does not depend on the insertion order)"""
    occ = np.zeros(cap, dtype=bool)
    for h in np.sort(_u64(homes)).tolist():
        c = h
        while occ[c % cap]:
            c += 1
        occ[c % cap] = True
    return occ


# ---- GROUP BY -----------------------------------------------------------------------------------------------------------------
def gbp_part64(keys, p, mult=GBP_MULT):
    """gbp_part for 8-byte keys: bits 52.. of key * mult, masked to P partitions"""
    return (_mul(keys, mult) >> np.uint64(52)) & np.uint64(p - 1)


def gbp_cell64(keys, s):
    """gbp_cell for 8-byte keys: bits 20.. of key * GBP_MULT, masked to S cells"""
    return (_mul(keys, GBP_MULT) >> np.uint64(20)) & np.uint64(s - 1)


def _m32(mult):
    return ((mult >> 32) | 1) & M32


def _h32(keys, mult):
    return (_u64(keys) * np.uint64(_m32(mult))) & np.uint64(M32)


def gbp_part32(keys, p, mult=GBP_MULT):
    """gbp_part for keys of <= 4 bytes: __umulhi(key * ((mult >> 32) | 1), P)"""
    return (_h32(keys, mult) * np.uint64(p)) >> np.uint64(32)


def gbp_cell32(keys, p, s):
    """gbp_cell for keys of <= 4 bytes: __umulhi(key * m * P, S) (the partition's bits shifted out); RANGE mode passes P = 1"""
    h = (_h32(keys, GBP_MULT) * np.uint64(p)) & np.uint64(M32)
    return (h * np.uint64(s)) >> np.uint64(32)


def gbp_inv64(y, mult=GBP_MULT):
    """the key whose product with `mult` is y"""
    return _mul(y, inv_odd(mult))


def gbp_inv32(h, mult=GBP_MULT):
    """the 32-bit key whose product with the 32-bit multiplier is h"""
    return (_u64(h) * np.uint64(inv_odd(_m32(mult), 32))) & np.uint64(M32)


def gb_keys64_top(rng, n, top_bits, top, mult=GBP_MULT):
    """n distinct nonzero 64-bit keys whose product with `mult` has `top` in its top `top_bits` bits: one partition for every
    P <= 2^top_bits (bits 52.. pick the partition)"""
    assert top_bits <= 12
    low = _distinct_free(rng, n, 64 - top_bits, exclude=(0,) if top == 0 else ())
    return gbp_inv64((np.uint64(top) << np.uint64(64 - top_bits)) | low, mult)


def gb_keys64_on_cell(rng, n, cell_bits, cell):
    """n distinct 64-bit keys on one LDS home cell for every S <= 2^cell_bits (bits 20.. of key * GBP_MULT), in random partitions"""
    free = _distinct_free(rng, n, 64 - cell_bits, exclude=(0,))
    lo = free & np.uint64((1 << 20) - 1)
    hi = free >> np.uint64(20)
    y = (hi << np.uint64(20 + cell_bits)) | (np.uint64(cell) << np.uint64(20)) | lo
    return gbp_inv64(y)


def gb_keys32_top(rng, n, top_bits, top, mult=GBP_MULT):
    """n distinct nonzero UInt32 keys whose 32-bit product has `top` in its top `top_bits` bits: one partition for P <= 2^top_bits,
    and one LDS cell too for P * S <= 2^top_bits"""
    low = _distinct_free(rng, n, 32 - top_bits, exclude=(0,) if top == 0 else ())
    return gbp_inv32((np.uint64(top) << np.uint64(32 - top_bits)) | low, mult).astype(np.uint32)


# ---- the wide-key dictionary (keys128 / keys256) ---------------------------------------------------------------------------------
# kd_tag: keydict_kernels.hip:127-128 (word 0: xor, multiply, xorshift-31), :131-132 (every later word: xor, multiply, xorshift-29),
# :135 (the 20-bit test hook), :136 (low bit forced to 1); the home cell: keydict_kernels.hip:165, :227 and :419
KD_TAG_XOR0 = 0x9E3779B97F4A7C15
KD_TAG_MUL0 = 0xBF58476D1CE4E5B9
KD_TAG_SHIFT0 = 31
KD_TAG_MUL = 0x94D049BB133111EB
KD_TAG_SHIFT = 29
KD_WEAK_MASK = 0xFFFFF
KD_HOME_MULT = 0x9E3779B97F4A7C15
KD_HOME_SHIFT = 20
KD_NO_ID = 0xFFFFFFFF


def _xs(x, s):
    x = _u64(x)
    return x ^ (x >> np.uint64(s))


def _xs_inv(y, s):
    """undo x ^= x >> s: x = y ^ (y >> s) ^ (y >> 2s) ^ ..."""
    y = _u64(y)
    x = y
    for _ in range(64 // s + 1):
        x = y ^ (x >> np.uint64(s))
    return x


def keydict_running_hash(words):
    """kd_tag's running value after the words given: uint64[n, q], q >= 1 leading words of the packed key"""
    words = _u64(words)
    h = _xs(_mul(words[..., 0] ^ np.uint64(KD_TAG_XOR0), KD_TAG_MUL0), KD_TAG_SHIFT0)
    for q in range(1, words.shape[-1]):
        h = _xs(_mul(h ^ words[..., q], KD_TAG_MUL), KD_TAG_SHIFT)
    return h


def keydict_tag(words, weak=False):
    """kd_tag of packed keys uint64[n, W] (W = 2: keys128, W = 4: keys256); weak: the 20-bit form of the test hook"""
    h = keydict_running_hash(words)
    if weak:
        h = h & np.uint64(KD_WEAK_MASK)
    return h | np.uint64(1)


def keydict_home(tags, capacity):
    """the home cell of a tag in a table of `capacity` cells (a power of two)"""
    return (_mul(_u64(tags) >> np.uint64(1), KD_HOME_MULT) >> np.uint64(KD_HOME_SHIFT)) & np.uint64(capacity - 1)


def keydict_last_word(prefix_words, tag, zero_words_after=0):
    """the 64-bit word which, put behind the leading words uint64[n, q], gives a key whose full tag is exactly `tag` (odd); with
    zero_words_after = z the key goes on with z zero words (a keys256 key of three UInt64 columns: q = 2, z = 1).  Every step of kd_tag
    is a bijection of the running value, so this undoes them from the end: the xorshift-29, the multiply, the xor."""
    tag = _u64(tag)
    assert np.all(tag & np.uint64(1) == 1)
    inv = inv_odd(KD_TAG_MUL)
    h = tag
    for _ in range(zero_words_after):
        h = _mul(_xs_inv(h, KD_TAG_SHIFT), inv)        # the value before a zero word was mixed in
    return _mul(_xs_inv(h, KD_TAG_SHIFT), inv) ^ keydict_running_hash(prefix_words)


def keydict_same_tag_keys(rng, n, w, tag, cols=None):
    """n distinct packed keys uint64[n, w] with one full 64-bit tag; cols < w: only the first `cols` words are free, the rest zero"""
    cols = w if cols is None else cols
    assert 2 <= cols <= w
    prefix = np.stack([_distinct_free(rng, n, 64) for _ in range(cols - 1)], axis=1)     # distinct prefixes: distinct keys
    last = keydict_last_word(prefix, np.full(n, tag, dtype=np.uint64), w - cols)
    keys = np.concatenate([prefix, last[:, None], np.zeros((n, w - cols), dtype=np.uint64)], axis=1)
    assert np.all(keydict_tag(keys) == np.uint64(tag))
    return keys


def keydict_tag_with_home(rng, cell_bits, lg, n=1):
    """n distinct tags whose home cell has `cell_bits` in its low `lg` bits: the cell `cell_bits & (capacity - 1)` of every capacity up to
    2^lg at once (all ones: the last cell of each).  tag >> 1 is what is multiplied, so it has to stay below 2^63: the free bits are
    drawn again until it does."""
    assert 0 <= cell_bits < (1 << lg) and KD_HOME_SHIFT + lg <= 64
    inv = inv_odd(KD_HOME_MULT)
    got = np.empty(0, dtype=np.uint64)
    while got.shape[0] < n:
        free = rng.integers(0, 2**64 - 1, size=4 * n + 16, dtype=np.uint64, endpoint=True)
        keep = ~(np.uint64(((1 << lg) - 1) << KD_HOME_SHIFT))
        y = (free & keep) | (np.uint64(cell_bits) << np.uint64(KD_HOME_SHIFT))
        t = _mul(y, inv)
        t = t[t < np.uint64(1 << 63)]
        got = np.unique(np.concatenate([got, (t << np.uint64(1)) | np.uint64(1)]))
    return rng.permutation(got)[:n]


# ---- the string dictionary (chgpu_string_dictionary_encode) -----------------------------------------------------------------------
# str_hash_bytes: string_kernels.hip:27-44 (the seed and the length multiplier :29, the word multiplier and the xorshift :33-34 and
# :39-40, intHash64 :42, the low bit forced to 1 :43); the home cell: string_kernels.hip:107 and :142; the table size: :207-209.
# Plain Python ints over bytes: the strings are few and short.
STR_SEED = 0x9E3779B97F4A7C15
STR_LEN_MUL = 0xFF51AFD7ED558CCD
STR_WORD_MUL = 0xC4CEB9FE1A85EC53
STR_SHIFT = 29
STR_CAP_MIN = 1024
STR_CELLS_PER_ROW = 2


def _int_hash64_py(x):
    x ^= x >> 33
    x = (x * INTHASH_MUL1) & M64
    x ^= x >> 33
    x = (x * INTHASH_MUL2) & M64
    return x ^ (x >> 33)


def _int_hash64_inv_py(h):
    x = ((h ^ (h >> 33)) * inv_odd(INTHASH_MUL2)) & M64
    x = ((x ^ (x >> 33)) * inv_odd(INTHASH_MUL1)) & M64
    return x ^ (x >> 33)


def _str_mix(h, word):
    h = ((h ^ word) * STR_WORD_MUL) & M64
    return h ^ (h >> STR_SHIFT)


def _str_running(data):
    """str_hash_bytes' running value after every byte of `data`, before intHash64"""
    n = len(data)
    h = STR_SEED ^ ((n * STR_LEN_MUL) & M64)
    full = n - n % 8
    for i in range(0, full, 8):
        h = _str_mix(h, int.from_bytes(data[i:i + 8], "little"))
    if n % 8:
        h = _str_mix(h, int.from_bytes(data[full:], "little"))       # the tail, zero extended: the kernel masks its 8-byte load
    return h


def str_raw_hash(data):
    """str_hash_bytes before its last line: the value whose bit 0 the tag overwrites"""
    return _int_hash64_py(_str_running(bytes(data)))


def str_hash(data):
    """str_hash_bytes: the 64-bit tag of a value (without its terminating zero); never 0"""
    return str_raw_hash(data) | 1


def str_table_cap(rows):
    """cells of the table chgpu_string_dictionary_encode builds for a column of `rows` rows"""
    cap = STR_CAP_MIN
    while cap < STR_CELLS_PER_ROW * rows:
        cap <<= 1
    return cap


def str_home(tag, cap):
    """the home cell of a tag in a table of `cap` cells"""
    return (tag >> 1) & (cap - 1)


def str_with_raw_hash(raw, prefix=b""):
    """prefix + 8 bytes whose raw hash is exactly `raw`: every step of str_hash_bytes is a bijection of the last full word (xor, an odd
    multiplier, the xorshift, intHash64), so they are undone from the end.  The 8 bytes may hold zeros: ColumnString is binary-safe."""
    prefix = bytes(prefix)
    assert len(prefix) % 8 == 0 and 0 <= raw <= M64
    n = len(prefix) + 8
    h = STR_SEED ^ ((n * STR_LEN_MUL) & M64)
    for i in range(0, len(prefix), 8):
        h = _str_mix(h, int.from_bytes(prefix[i:i + 8], "little"))
    y = _int_hash64_inv_py(raw)
    y = y ^ (y >> STR_SHIFT) ^ (y >> (2 * STR_SHIFT))                # undoes x ^= x >> 29 (3 * 29 > 64)
    word = ((y * inv_odd(STR_WORD_MUL)) & M64) ^ h
    return prefix + word.to_bytes(8, "little")


def str_with_home(cell, cap, salt, prefix=b""):
    """a string homed at `cell` of a table of `cap` cells; distinct salts (below 2^63 / cap) give distinct tags, hence distinct
    strings.  The salt fills the tag's bits above the home cell's: salts 1 << k are tags that differ in one high bit only."""
    lg = cap.bit_length() - 1
    assert cap == 1 << lg and 0 <= cell < cap and 0 <= salt < (1 << (63 - lg))
    return str_with_raw_hash((salt << (lg + 1)) | (cell << 1) | 1, prefix)


def str_tag_twins(tag, prefix_a=b"", prefix_b=b""):
    """two different strings with one tag: the raw hashes `tag` and `tag ^ 1` differ in bit 0 only, which the tag overwrites"""
    assert tag & 1
    a, b = str_with_raw_hash(tag, prefix_a), str_with_raw_hash(tag ^ 1, prefix_b)
    assert a != b
    return a, b
