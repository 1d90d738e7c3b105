"""Builders of compressed frames whose every field is given, for the decoders of clickhouse_amd/csrc/compress_kernels.hip: LZ4 blocks written
sequence by sequence around the constants that choose a path in k_lz4_decode, malformed variants of one block, Delta / DoubleDelta /
Gorilla / T64 inputs at short and odd sizes, and codec frames with one header field changed.  No GPU and no assertions about a decoder here: tests/test_frame_craft.py checks every builder
against the C oracle (oracle.compression) and asserts what the sets cover; tests/test_gpu_frame_decoder_edges.py sends them to the device.

Nothing is imported from the kernel.  The four constants it branches on, restated once:"""
import struct
import zlib

import numpy as np

from oracle import compression as OC

LZ_IN = 1024                # compress_kernels.hip:39   static constexpr u32 LZ_IN = 1024      (input window bytes per wave)
LZ_RING = 4096              # compress_kernels.hip:40   static constexpr u32 LZ_RING = 4096    (output ring bytes per wave)
LZ_CHUNK = LZ_RING // 2     # compress_kernels.hip:42   static constexpr u32 LZ_CHUNK = LZ_RING / 2   (ring-served matches: offset <= LZ_CHUNK)
LZ_FAST_FAR = LZ_RING - 64  # compress_kernels.hip:152  the largest offset the fast path serves from the ring
FAST_IN, FAST_OUT = 64, 32  # compress_kernels.hip:139  the fast path wants 64 readable window bytes and 32 free output bytes

END = 70                    # literals of the closing sequence where a case does not say otherwise: with its token and length byte, 64 input
                            # bytes behind the token of a fast-path-shaped sequence in front of it, so that the fast path does take that one
SHORT_END = 12              # ... of the blocks that get one field changed


# ---- 1. LZ4 blocks, sequence by sequence -------------------------------------------------------------------------------------------------
def _length_bytes(rest):
    out = bytearray()
    while rest >= 255:
        out.append(255)
        rest -= 255
    out.append(rest)
    return bytes(out)


class Lz4Builder:
    """an LZ4 block and the bytes it decodes to, grown together.  Literals are drawn from a generator seeded by `seed`; `prefix` replaces the
    first bytes of the first literal run (a codec stage's header, when the block is the general stage of CODEC(Delta, LZ4))."""

    def __init__(self, seed, prefix=b""):
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.blk, self.out, self.prefix = bytearray(), bytearray(), bytes(prefix)

    def _literals(self, n):
        lits = self.rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        if self.prefix:
            if n < len(self.prefix):
                raise ValueError("the first literal run is shorter than the prefix")
            lits, self.prefix = self.prefix + lits[len(self.prefix):], b""
        return lits

    def seq(self, literal_len, offset, match_len):
        """token, literal-length bytes, literals, offset, match-length bytes; the expected output grows by the literals and the match"""
        if match_len < 4 or not 1 <= offset <= min(65535, len(self.out) + literal_len):
            raise ValueError(("no such sequence", literal_len, offset, match_len, len(self.out)))
        self.blk.append((min(literal_len, 15) << 4) | min(match_len - 4, 15))
        if literal_len >= 15:
            self.blk += _length_bytes(literal_len - 15)
        lits = self._literals(literal_len)
        self.blk += lits
        self.out += lits
        self.blk += struct.pack("<H", offset)
        if match_len - 4 >= 15:
            self.blk += _length_bytes(match_len - 19)
        start = len(self.out) - offset
        if offset >= match_len:
            self.out += self.out[start:start + match_len]
        else:  # an overlapping match is the `offset` bytes before it, repeated
            period = bytes(self.out[start:])
            self.out += (period * (match_len // offset + 1))[:match_len]
        return self

    def end(self, literal_len):
        """the closing sequence: literals only -> (block, decoded bytes)"""
        self.blk.append(min(literal_len, 15) << 4)
        if literal_len >= 15:
            self.blk += _length_bytes(literal_len - 15)
        lits = self._literals(literal_len)
        self.blk += lits
        self.out += lits
        return bytes(self.blk), bytes(self.out)


class Lz4Case:
    """a named recipe: the (literal_len, offset, match_len) of every sequence and the closing literal length"""

    def __init__(self, name, seqs, end=END):
        self.name, self.seqs, self.end = name, list(seqs), end

    @property
    def decoded_len(self):
        return sum(lit + ml for lit, _, ml in self.seqs) + self.end

    def build(self, prefix=b""):
        b = Lz4Builder(zlib.crc32(self.name.encode()), prefix)
        for lit, offset, ml in self.seqs:
            b.seq(lit, offset, ml)
        return b.end(self.end)


def _fast_followers(have, offsets):
    """fast-path-shaped sequences (3 literals, match length 7) that read what the sequences before them left in the ring, at every offset
    of `offsets` the output is long enough for"""
    out = []
    for o in offsets:
        if o <= have + 3:
            out.append((3, o, 7))
            have += 10
    return out


RING_OFFSETS = (2047, 2048, 2049, 4031, 4032, 4033, 4095, 4096, 4097, 65535)


def ring_limit_cases():
    cases = []
    for offset in RING_OFFSETS:
        lengths = (4, 19, 5000, 7000) if offset == 65535 else (4, 18, 19, offset - 1, offset, offset + 1, 2 * offset + 3)
        for extra in (0, 5):
            for ml in lengths:
                seqs = [(offset + extra, offset, ml)]
                seqs += _fast_followers(offset + extra + ml, (1, 3, 8, 2048, 4032))
                cases.append(Lz4Case(f"ring o={offset} lit=+{extra} ml={ml}", seqs))
    return cases


LONG_LITERALS = (14, 15, 16, 269, 270, 271, 524, 525, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 9000)


def long_literal_cases():
    cases = []
    for lit in LONG_LITERALS:
        for offset in sorted({1, lit, min(lit, LZ_CHUNK), min(lit, LZ_FAST_FAR)}):
            cases.append(Lz4Case(f"literals lit={lit} o={offset}", [(lit, offset, 9), (3, 8, 7)]))
    return cases


LONG_MATCHES = (2047, 2048, 2049, 4095, 4096, 4097, 4100, 6145, 10000)
LONG_MATCH_OFFSETS = (1, 2, 3, 7, 63, 64, 65, 100, 2047, 2048, 2049, 3000, 4097, 5000)


def long_match_cases():
    cases = []
    for ml in LONG_MATCHES:
        for offset in LONG_MATCH_OFFSETS:
            seqs = [(offset, offset, ml)]  # the source is the literals of the same sequence
            seqs += _fast_followers(offset + ml, (1, 5, 2048, 2049, 4032, 4033))
            cases.append(Lz4Case(f"match ml={ml} o={offset}", seqs))
    return cases


HEADER_SHIFTS = tuple(range(0, 1100, 7))


def window_end_cases(shifts=HEADER_SHIFTS):
    """one literal run of shift + 1 bytes pushes 120 short sequences (and one with two literal-length bytes and three match-length bytes)
    along the input, so that every header field lies across the end of the first 1024-byte window in some case"""
    cases = []
    for shift in shifts:
        rng = np.random.Generator(np.random.PCG64(1000 + shift))
        seqs, have = [(shift + 1, 1, 4)], shift + 5
        for _ in range(120):
            lit, ml = int(rng.integers(0, 15)), int(rng.integers(4, 19))
            far = min(have + lit, LZ_FAST_FAR)
            offset = int(rng.integers(1, min(far, 16) + 1)) if rng.random() < 0.5 else int(rng.integers(1, far + 1))
            seqs.append((lit, offset, ml))
            have += lit + ml
        seqs.append((273, int(rng.integers(1, min(have + 273, LZ_FAST_FAR) + 1)), 530))
        cases.append(Lz4Case(f"window shift={shift}", seqs))
    # In the series above a literal run carries the input position past the window's end far more often than a header does, so nearly
    # every fetch is made for an offset field and none for a length byte.  The same long sequence (token, literal-length bytes 255 3, 273
    # literals, offset, match-length bytes 255 255 1) placed by hand: its token at `at`, with the end of the first window in[0, 1024)
    # behind the token, between the literal-length bytes, inside the offset, and in front of each match-length byte.
    for at in (LZ_IN - 3, LZ_IN - 2, LZ_IN - 1, LZ_IN, LZ_IN - 281, LZ_IN - 280, LZ_IN - 279, LZ_IN - 278, LZ_IN - 277, LZ_IN - 276):
        lit = next(n for n in range(15, at) if 1 + len(_length_bytes(n - 15)) + n + 2 == at)
        cases.append(Lz4Case(f"window long sequence at={at}", [(lit, 1, 4), (273, 100, 530), (3, 1, 7), (3, 600, 7)]))
    return cases


def frame_end_cases():
    """the last fast-path-shaped sequence ends 5 .. 39 bytes before the frame's end"""
    return [Lz4Case(f"frame end tail={tail}", [(80, 5, 6)] + [(2, 5, 6)] * 30, end=tail) for tail in range(5, 40)]


LZ4_GROUPS = {"ring_limits": ring_limit_cases, "long_literals": long_literal_cases, "long_matches": long_match_cases,
              "window_end": window_end_cases, "frame_end": frame_end_cases}


def walk_sequences(block, with_offset_position=False):
    """the sequences of a well-formed block: (literal_len, offset, match_len, input position of the token) each; the closing sequence has
    offset 0 and match_len 0.  with_offset_position=True appends the input position of the two-byte offset field (None in the last)."""
    out, ip = [], 0
    while ip < len(block):
        at = ip
        token = block[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            while True:
                b = block[ip]
                ip += 1
                lit += b
                if b != 255:
                    break
        ip += lit
        if ip >= len(block):
            out.append((lit, 0, 0, at) + ((None,) if with_offset_position else ()))
            break
        offset_at = ip
        offset = block[ip] | (block[ip + 1] << 8)
        ip += 2
        ml = token & 15
        if ml == 15:
            while True:
                b = block[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        out.append((lit, offset, ml + 4, at) + ((offset_at,) if with_offset_position else ()))
    return out


def decoder_trace(block, decoded_len):
    """how a decoder that keeps LZ_IN input bytes at hand reads a well-formed block, by the rules of compress_kernels.hip:92-115, :139
    and :152: a sequence of fast-path shape (fewer than 15 literals, a match below 19 from at most LZ_FAST_FAR back) whose next 64 input
    bytes are at hand, with 32 output bytes free, is read in one go; otherwise the token, every length byte and the two offset bytes are
    asked for one field at a time, and a field that is not wholly at hand makes the window begin anew at that field.
    -> (refills, fast): refills = [(field, input position, bytes of the field that were still at hand)], field one of "token", "literal
    length", "offset", "match length"; fast = the token positions of the sequences read in one go.  A coverage instrument for the crafted
    set, not a decoder."""
    refills, fast, ip, op, base, have = [], set(), 0, 0, 0, 0
    isz = len(block)

    def want(field, pos, need):
        nonlocal base, have
        if pos < base or pos + need > base + have:
            refills.append((field, pos, max(0, base + have - pos) if pos >= base else 0))
            base, have = pos, min(isz - pos, LZ_IN)

    while True:
        if ip >= base and ip + FAST_IN <= base + have and op + FAST_OUT <= decoded_len:
            lit, mlt = block[ip] >> 4, block[ip] & 15
            if lit != 15 and mlt != 15:
                offset = block[ip + 1 + lit] | (block[ip + 2 + lit] << 8)
                if 1 <= offset <= min(op + lit, LZ_FAST_FAR):
                    fast.add(ip)
                    ip, op = ip + 3 + lit, op + lit + mlt + 4
                    continue
        want("token", ip, 1)
        token = block[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            while True:
                want("literal length", ip, 1)
                b = block[ip]
                ip += 1
                lit += b
                if b != 255:
                    break
        ip, op = ip + lit, op + lit
        if ip >= isz:
            return refills, fast
        want("offset", ip, 2)
        ip += 2
        ml = token & 15
        if ml == 15:
            while True:
                want("match length", ip, 1)
                b = block[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        op += ml + 4


def lz4_frame(block, decoded_len):
    return OC._framed(OC._stage(OC.METHOD_LZ4, block, decoded_len))


def none_frame(raw):
    return OC._framed(OC._stage(OC.METHOD_NONE, raw, len(raw)))


def delta_stage_prefix(stage_len, width):
    """the first 11 bytes of a Delta stage of stage_len bytes: its own 9-byte header, element width, bytes_to_skip.  Whatever bytes follow
    are a valid Delta payload, so any crafted block whose first literal run begins with these decodes to a Delta stage."""
    return struct.pack("<BII", OC.METHOD_DELTA, stage_len, stage_len - 11) + bytes([width, (stage_len - 11) % width])


def delta_lz4_frame(case, width):
    """the case's block as the general stage of CODEC(Delta(width), LZ4) -> (frame, the column bytes the oracle decodes the stage to)"""
    n = case.decoded_len
    block, stage = case.build(delta_stage_prefix(n, width))
    inner = OC._stage(OC.METHOD_LZ4, block, n)
    return OC._framed(OC._stage(OC.METHOD_MULTIPLE, bytes([2, OC.METHOD_DELTA, OC.METHOD_LZ4]) + inner, n - 11)), OC.delta_decode(stage[9:], n - 11)


def small_block_pool(n=64):
    """distinct small blocks, 50 .. 300 decoded bytes: even ones of fast-path shape only (fewer than 15 literals, matches below 19), odd
    ones with a long literal run or a long match in them.  Every first literal run has room for a Delta stage's 11 header bytes."""
    pool = []
    for i in range(n):
        rng = np.random.Generator(np.random.PCG64(7000 + i))
        target = int(rng.integers(50, 200))
        seqs, have = [], 0
        while have < target:
            lit, ml = int(rng.integers(0, 15)), int(rng.integers(4, 19))
            if not seqs:
                lit = int(rng.integers(11, 15))
            if i % 2 and len(seqs) == 1:
                lit, ml = (int(rng.integers(15, 40)), ml) if i % 4 == 1 else (lit, int(rng.integers(19, 60)))
            offset = int(rng.integers(1, min(have + lit, 16 if rng.random() < 0.5 else 300) + 1))
            seqs.append((lit, offset, ml))
            have += lit + ml
        pool.append(Lz4Case(f"pool {i}", seqs, end=int(rng.integers(5, 20))))
    return pool


# ---- 3. one well-formed block, one field changed ------------------------------------------------------------------------------------------
def _malformed_base(target, end=SHORT_END):
    """four sequences (the first on the general path, three of fast-path shape), then `target`, then the closing literals ->
    (block, decoded bytes, input position of the target's token, output position where the target begins)"""
    pre = [(70, 9, 40), (3, 5, 7), (2, 1, 5), (14, 20, 18)]
    case = Lz4Case("malformed base %r %d" % (target, end), pre + [target], end)
    block, raw = case.build()
    at = walk_sequences(block)[len(pre)][3]
    return block, raw, at, sum(lit + ml for lit, _, ml in pre)


def malformed_lz4_cases():
    """-> [(name, method, payload, claimed decoded size, well-formed payload, its decoded bytes)].  Next to each case: the check of
    k_lz4_decode that refuses it, found by following the case through the kernel's code (line numbers of compress_kernels.hip)."""
    cases = []

    def add(name, bad_block, claimed, block, raw):
        cases.append((name, OC.METHOD_LZ4, bytes(bad_block), claimed, block, raw))

    # Fewer than 64 input bytes follow the target in every truncated case, so `ip + 64 <= in_base + in_len` (:139) fails and the target
    # is parsed by the general path.
    block, raw, at, _ = _malformed_base((3, 5, 7))
    # the token says 3 literals and 0 bytes are left: `lit > isz - ip` (:197)
    add("ends after a token with literals", block[:at + 1], len(raw), block, raw)
    # after the 3 literals one byte is left: ip < isz, so no normal end (:211); `window(ip, 2)` is false for pos + 2 > isz (:93, :213)
    add("ends after one offset byte", block[:at + 1 + 3 + 1], len(raw), block, raw)
    block, raw, at, _ = _malformed_base((0, 5, 7))
    # the token says 0 literals and the input is used up: the loop ends as after a last sequence (:211), then `op != osz` (:264)
    add("ends after a token without literals", block[:at + 1], len(raw), block, raw)
    block, raw, at, _ = _malformed_base((300, 5, 7))
    # the token's 15 and the byte 255 are read, the chain goes on and `window(ip, 1)` is false at ip == isz (:121)
    assert block[at + 1] == 255
    add("ends inside a literal-length chain", block[:at + 2], len(raw), block, raw)
    block, raw, at, _ = _malformed_base((3, 5, 300))
    # token, 3 literals, offset, the byte 255 of the match length: `window(ip, 1)` is false at ip == isz (:121)
    assert block[at + 1 + 3 + 2] == 255
    add("ends inside a match-length chain", block[:at + 1 + 3 + 2 + 1], len(raw), block, raw)

    # the closing sequence's literal length 12 -> 13
    block, raw, _, _ = _malformed_base((3, 5, 7))
    close = walk_sequences(block)[-1][3]
    bad = bytearray(block)
    bad[close] = 13 << 4
    # 12 input bytes are left, and the output (claimed one byte longer) has room for 13: `lit > isz - ip` alone is true (:197)
    add("literal length one more than the input left", bad, len(raw) + 1, block, raw)
    # one more input byte so that 13 are there; the output has room for 12: `lit > osz - op` alone is true (:197)
    add("literal length one more than the output left", bad + b"\x00", len(raw), block, raw)

    # The target has fast-path shape and 72 input bytes behind it, so the fast path looks at it first: `offset - 1 < min(op + lit, 4032)`
    # (:152) is false for offset 0 (offset - 1 wraps to 2^32 - 1) and for offset op + lit + 1, and the general path takes it over.
    block, raw, at, op = _malformed_base((3, 5, 7), end=70)
    bad = bytearray(block)
    bad[at + 4:at + 6] = struct.pack("<H", 0)
    add("offset 0", bad, len(raw), block, raw)                                   # `offset == 0` (:227)
    bad = bytearray(block)
    bad[at + 4:at + 6] = struct.pack("<H", op + 3 + 1)
    add("offset one more than the output so far", bad, len(raw), block, raw)     # `offset > op` (:227), op counted behind the 3 literals

    # match length 30 -> 30 + 12 + 1: the 30 and the closing 12 literals are all the output left; one length byte either way
    block, raw, at, _ = _malformed_base((3, 5, 30))
    bad = bytearray(block)
    assert bad[at + 6] == 30 - 19
    bad[at + 6] = 30 + SHORT_END + 1 - 19
    add("match length one more than the output left", bad, len(raw), block, raw)  # `ml > osz - op` (:227)

    # a valid block under a header that claims one byte more or fewer
    block, raw, _, _ = _malformed_base((3, 5, 7))
    add("header claims one byte more", block, len(raw) + 1, block, raw)          # everything decodes; `op != osz` (:264)
    add("header claims one byte fewer", block, len(raw) - 1, block, raw)         # the closing 12 literals: `lit > osz - op` (:197)
    block, raw, _, _ = _malformed_base((3, 5, 7), end=0)                          # ... and a block that closes with an empty literal run
    add("header claims one byte more, last bytes a match", block, len(raw) + 1, block, raw)   # `op != osz` (:264)
    add("header claims one byte fewer, last bytes a match", block, len(raw) - 1, block, raw)  # the last match: `ml > osz - op` (:227)

    # method NONE: `isz != osz` (:78)
    rng = np.random.Generator(np.random.PCG64(77))
    stored = rng.integers(0, 256, size=100, dtype=np.uint8).tobytes()
    cases.append(("stored frame claims one byte more", OC.METHOD_NONE, stored, 101, stored, stored))
    cases.append(("stored frame claims one byte fewer", OC.METHOD_NONE, stored, 99, stored, stored))
    return cases


def malformed_file(case):
    """-> (the file with the malformed frame between two well-formed frames of 9 KiB each way, the same file with the well-formed frame
    in its place, the bytes that one decodes to)"""
    name, method, payload, claimed, good_payload, raw = case
    sides = []
    for tag in ("before", "after"):
        b, r = Lz4Case(f"neighbour {tag} {name}", [(9000, 2048, 300)]).build()
        sides.append((lz4_frame(b, len(r)), r))
    bad = OC._framed(OC._stage(method, payload, claimed))
    good = OC._framed(OC._stage(method, good_payload, len(raw)))
    return sides[0][0] + bad + sides[1][0], sides[0][0] + good + sides[1][0], sides[0][1] + raw + sides[1][1]


# ---- 4. Delta, DoubleDelta and Gorilla at short and odd sizes ---------------------------------------------------------------------------
WIDTHS = (1, 2, 4, 8)
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
DELTA_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 193)


def delta_values(width, k, seed):
    """k values over the full width whose running sum of deltas wraps in every block of 64 deltas that has a value in front of it: the
    value in front of each block (and the first value) has the top bit, the block's first value does not"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.integers(0, 2**(8 * width), size=k, dtype=np.uint64)
    top = np.uint64(1 << (8 * width - 1))
    for i in [1] + list(range(64, k, 64)):
        if i < k:
            x[i - 1] |= top
            x[i] &= ~top
    return x.astype(UINT[width])


def delta_raws(width):
    """-> [(skip, k, raw bytes)]: raw length skip + k * width, for every skip below the width"""
    out = []
    for skip in range(width):
        for k in DELTA_COUNTS:
            rng = np.random.Generator(np.random.PCG64(31 * width + skip))
            out.append((skip, k, rng.integers(0, 256, size=skip, dtype=np.uint8).tobytes() + delta_values(width, k, 100 * width + 10 * skip + k).tobytes()))
    return out


def delta_lz4_frame_of_raw(raw, width):
    st1 = OC._stage(OC.METHOD_DELTA, OC.delta_encode(raw, width), len(raw))
    block, _ = Lz4Builder(0, st1).end(len(st1))  # the stage as one literal run: this test is about the Delta stage
    return OC._framed(OC._stage(OC.METHOD_MULTIPLE, bytes([2, OC.METHOD_DELTA, OC.METHOD_LZ4]) + OC._stage(OC.METHOD_LZ4, block, len(st1)), len(raw)))


def _truncate(values, width):
    return (np.asarray(values, dtype=np.int64).astype(np.uint64) & np.uint64((1 << (8 * width)) - 1 if width < 8 else 2**64 - 1)).astype(UINT[width])


def stream_raws(codec, width):
    """raw byte strings for one DoubleDelta ("dd") or Gorilla ("gorilla") frame each -> [(name, raw)]"""
    from test_compression import dd_compat_sequence
    dt = UINT[width]
    rng = np.random.Generator(np.random.PCG64(500 + width + (0 if codec == "dd" else 10)))
    out = []
    for n in range(1, 600):   # one-bit codes behind the header values
        v = _truncate(1000 + 37 * np.arange(n), width) if codec == "dd" else np.full(n, 0x5A5A5A5A5A5A5A5A & ((1 << (8 * width)) - 1), dtype=dt)
        out.append((f"constant n={n}", v.tobytes()))
    corners = dd_compat_sequence({1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[width]).view(dt)
    for n in range(1, 131):
        out.append((f"ramp n={n}", _truncate(np.cumsum(rng.integers(0, 50, size=n)), width).tobytes()))
        out.append((f"full n={n}", rng.integers(0, 256, size=n * width, dtype=np.uint8).tobytes()))
        out.append((f"corners n={n}", np.resize(corners, n).tobytes()))
    for skip in range(1, width):  # bytes_to_skip: raw lengths that are no multiple of the width
        for n in (0, 1, 2, 3, 10, 83 // width):
            out.append((f"skip={skip} n={n}", rng.integers(0, 256, size=skip, dtype=np.uint8).tobytes() + _truncate(np.cumsum(rng.integers(0, 9, size=n)), width).tobytes()))
    return out


def stream_frame(codec, raw, width):
    method, enc = (OC.METHOD_DOUBLE_DELTA, OC.double_delta_encode) if codec == "dd" else (OC.METHOD_GORILLA, OC.gorilla_encode)
    return OC._framed(OC._stage(method, enc(raw, width), len(raw)))


def bit_stream_len(codec, payload, width):
    """bytes of the bit stream in a DoubleDelta / Gorilla payload: what follows [width][bytes_to_skip][skipped][items u32][first value] and,
    for DoubleDelta, [first delta] (each part only as far as the payload has it)"""
    rest = len(payload) - 2 - payload[1]
    for part in (4, width) + ((width,) if codec == "dd" else ()):
        rest -= min(rest, part)
    return rest


# ---- 5. T64 over every bit width and type cookie -------------------------------------------------------------------------------------------
T64_TYPES = (np.uint8, np.uint16, np.uint32, np.uint64, np.int8, np.int16, np.int32, np.int64)
T64_COUNTS = (63, 64, 65, 257)
# MagicNumber of the types that are stored as an integer type (CompressionCodecT64.cpp:75-160) -> that type
T64_ALIAS_COOKIES = {13: np.uint16, 14: np.uint32, 15: np.int64, 17: np.int8, 18: np.int16, 19: np.int32, 20: np.int64, 21: np.uint32, 22: np.int32}


def t64_num_bits(payload):
    """num_bits as the reference computes it from the cookie, min and max of an encoded payload (getValuableBitsNumber)"""
    magic = payload[0] & 0x7F
    signed = magic in (6, 7, 8, 9, 15, 17, 18, 19, 20, 22)
    mn, mx = struct.unpack_from("<qq" if signed else "<QQ", payload, 1)
    if signed and mn < 0 <= mx:
        return (mx if mn + mx >= 0 else ~mn).bit_length() + 1
    return ((mn ^ mx) & (2**64 - 1)).bit_length()


def _between(rng, lo, hi, count):
    """count Python integers in [lo, hi] with both ends among them"""
    span = hi - lo
    vals = [lo + (int(rng.integers(0, 2**62)) * int(rng.integers(0, 2**62))) % (span + 1) for _ in range(count)]
    vals[int(rng.integers(0, count))] = lo
    free = [i for i in range(count) if vals[i] != lo] or [0]
    vals[free[int(rng.integers(0, len(free)))]] = hi
    return vals


def t64_sequences(dtype):
    """-> [(name, wanted num_bits, values)] for one integer type: for every num_bits an unsigned (or, signed type, all-negative) range that
    differs in exactly that many bits below a random upper part, for signed types ranges across zero on both sides of `min + max >= 0`,
    and ranges of one value (num_bits 0); 63 / 64 / 65 / 257 values each (1 .. 5 blocks), one value for the one-value ranges too"""
    dt = np.dtype(dtype)
    bits, signed = 8 * dt.itemsize, dt.kind == "i"
    rng = np.random.Generator(np.random.PCG64(900 + bits + signed))
    out = []

    def add(name, nb, vals):
        out.append((name, nb, np.array([v & (2**bits - 1) for v in vals], dtype=np.uint64).astype(UINT[dt.itemsize]).view(dt)))

    for nb in range(1, bits + 1):
        for count in T64_COUNTS:
            if not (signed and nb == bits):  # (a signed range that differs in the sign bit crosses zero)
                upper = (int(rng.integers(0, 2**62)) << nb) & (2**bits - 1)
                if signed:
                    upper |= 1 << (bits - 1)  # all negative
                lo = upper | int(rng.integers(0, 1 << (nb - 1)))
                hi = upper | (1 << (nb - 1)) | int(rng.integers(0, 1 << (nb - 1)))
                vals = _between(rng, lo, hi, count)
                add(f"{dt.name} nb={nb} n={count} one sign", nb, [v - (1 << bits) for v in vals] if signed else vals)
            if signed:
                # min + max >= 0: num_bits = bits of max + 1; min + max < 0: bits of ~min + 1
                mx = (1 << (nb - 2)) + int(rng.integers(0, 1 << (nb - 2))) if nb >= 2 else 0
                if nb >= 2:
                    add(f"{dt.name} nb={nb} n={count} across zero, max decides", nb, _between(rng, -int(rng.integers(1, mx + 1)), mx, count))
                mn = -1 - mx
                add(f"{dt.name} nb={nb} n={count} across zero, min decides", nb, _between(rng, mn, int(rng.integers(0, -mn)), count))
    for count in (1,) + T64_COUNTS:
        for v in (0, 42, -5 if signed else 2**bits - 1):
            add(f"{dt.name} nb=0 n={count} v={v}", 0, [v] * count)
    return out


def t64_frame(values, variant_bit, cookie=None):
    payload = bytearray(OC.t64_encode(values, variant_bit))
    if cookie is not None:
        payload[0] = (payload[0] & 0x80) | cookie
    return OC._framed(OC._stage(OC.METHOD_T64, bytes(payload), values.nbytes))


def t64_small_pool():
    """small sequences of every type for a file of very many T64 frames"""
    pool = []
    for dt in T64_TYPES:
        seqs = t64_sequences(dt)
        pool += [s for s in seqs if s[2].shape[0] <= 65][::max(1, len(seqs) // 12)][:8]
    return pool


# ---- 6. one well-formed codec frame, one header field changed -----------------------------------------------------------------------------
CODEC_NAMES = {OC.METHOD_DELTA: "Delta", OC.METHOD_T64: "T64", OC.METHOD_DOUBLE_DELTA: "DoubleDelta", OC.METHOD_GORILLA: "Gorilla"}
GENERAL_NAMES = {OC.METHOD_LZ4: "LZ4", OC.METHOD_NONE: "NONE"}
WIDTH_SKIP_CODECS = (OC.METHOD_DELTA, OC.METHOD_DOUBLE_DELTA, OC.METHOD_GORILLA)


def codec_column(codec, n=130, seed=0):
    """n UInt32 values of the kind the codec is for: three T64 blocks, the last of two values; bit-stream codes of several lengths"""
    rng = np.random.Generator(np.random.PCG64(600 + codec + seed))
    if codec == OC.METHOD_T64:
        return rng.integers(70_000, 75_000, size=n).astype(np.uint32)
    if codec == OC.METHOD_GORILLA:
        return (1000.0 + np.cumsum(rng.integers(-3, 4, size=n)) * 0.5).astype(np.float32).view(np.uint32)
    return np.cumsum(rng.integers(0, 300, size=n)).astype(np.uint32)


def codec_payload(codec, values):
    if codec == OC.METHOD_T64:
        return OC.t64_encode(values)
    enc = {OC.METHOD_DELTA: OC.delta_encode, OC.METHOD_DOUBLE_DELTA: OC.double_delta_encode, OC.METHOD_GORILLA: OC.gorilla_encode}[codec]
    return enc(values.tobytes() if isinstance(values, np.ndarray) else values, 4)


def stage_bytes(codec, payload, out_size, method=None, csize_off=0, dsize_off=0):
    """a codec stage as the general-purpose stage in front of it yields it: its own 9-byte header (each field can be set off) + payload"""
    return struct.pack("<BII", codec if method is None else method, OC.HEADER + len(payload) + csize_off, out_size + dsize_off) + bytes(payload)


def codec_frame(codec, payload, out_size, general=None, stage=None):
    """general None: the frame that IS one application of the codec.  Otherwise CODEC(codec, general) as a Multiple frame whose general
    stage (LZ4: one literal run; NONE: stored) yields `stage` (default: the well-formed stage of payload and out_size)."""
    if general is None:
        return OC._framed(OC._stage(codec, bytes(payload), out_size))
    st1 = stage_bytes(codec, payload, out_size) if stage is None else stage
    block = st1 if general == OC.METHOD_NONE else Lz4Builder(0, st1).end(len(st1))[0]
    return OC._framed(OC._stage(OC.METHOD_MULTIPLE, bytes([2, codec, general]) + OC._stage(general, block, len(st1)), out_size))


# The cases of malformed_codec_cases that the C oracle decodes without complaint (to bytes nobody asked for) and the kernel refuses: the
# oracle reads a stage's payload as far as the buffer goes whatever the stage's compressed size says, takes the stage's method byte as
# it stands, and does not check bytes_to_skip < width (what Delta and Gorilla read behind two bytes too many, it refuses for other
# reasons).  tests/test_frame_craft.py asserts this set.
KERNEL_STRICTER_THAN_ORACLE = frozenset(
    [f"{c} behind {g}: stage header, compressed size one more" for c in CODEC_NAMES.values() for g in GENERAL_NAMES.values()]
    + [f"{c} behind {g}: stage header, compressed size one fewer" for c in ("DoubleDelta", "Gorilla") for g in GENERAL_NAMES.values()]
    + ["DoubleDelta: bytes_to_skip == width"])


def malformed_codec_cases():
    """-> [(name, codec, malformed frame, well-formed twin, the bytes the twin decodes to)].  Every malformed frame has a valid checksum
    and outer sizes that hold, so the host's frame walk accepts it; the name says which field was changed and the comment next to the case
    which check of compress_kernels.hip refuses it.  No case rests on an access out of range: each is refused by a comparison of header
    fields with the frame's sizes before the bytes in question are touched."""
    cases = []
    DELTA, T64, DD, GOR = OC.METHOD_DELTA, OC.METHOD_T64, OC.METHOD_DOUBLE_DELTA, OC.METHOD_GORILLA

    def add(name, codec, bad, good, raw):
        cases.append((f"{CODEC_NAMES[codec]}{name}", codec, bad, good, raw))

    # -- the stage header behind a general-purpose stage: codec_io() --
    for codec in CODEC_NAMES:
        raw = codec_column(codec).tobytes()
        pay = codec_payload(codec, codec_column(codec))
        for general, gname in GENERAL_NAMES.items():
            good = codec_frame(codec, pay, len(raw), general)

            def stage_case(what, stage):
                add(f" behind {gname}: stage header, {what}", codec, codec_frame(codec, pay, len(raw), general, stage), good, raw)

            other = DELTA if codec != DELTA else T64
            stage_case("method byte of another codec", stage_bytes(codec, pay, len(raw), method=other))       # `h[0] != M`
            stage_case("compressed size one more", stage_bytes(codec, pay, len(raw), csize_off=1))            # `csize != ssz`
            stage_case("compressed size one fewer", stage_bytes(codec, pay, len(raw), csize_off=-1))          # `csize != ssz`
            stage_case("decompressed size one more", stage_bytes(codec, pay, len(raw), dsize_off=1))          # `dsize != job.out_size`
            stage_case("decompressed size one fewer", stage_bytes(codec, pay, len(raw), dsize_off=-1))        # `dsize != job.out_size`
            stage_case("a stage of 8 bytes", stage_bytes(codec, pay, len(raw))[:8])                           # `ssz < 9`

    # -- [width][bytes_to_skip][skipped bytes]: Delta behind LZ4, DoubleDelta and Gorilla as frames of their own --
    for codec in WIDTH_SKIP_CODECS:
        general = OC.METHOD_LZ4 if codec == DELTA else None
        raw = codec_column(codec).tobytes()[:-2]      # 129 values and 2 bytes in front of them: bytes_to_skip = 2
        pay = codec_payload(codec, raw)
        assert pay[:2] == bytes([4, 2])
        good = codec_frame(codec, pay, len(raw), general)

        def changed(at, value):
            return pay[:at] + bytes([value]) + pay[at + 1:]

        for w in (0, 3, 16):
            add(f": width {w}", codec, codec_frame(codec, changed(0, w), len(raw), general), good, raw)      # width not 1 / 2 / 4 / 8
        add(": bytes_to_skip == width", codec, codec_frame(codec, changed(1, 4), len(raw), general), good, raw)   # `skip < width`
        # 3 bytes in front of 4-byte values are all skipped bytes: [4][3][3 bytes] (and items = 0 for DoubleDelta and Gorilla).  The same payload in
        # a frame that promises 2 bytes of output (the Delta stage's own header too): the width is valid, skip < width and `2 + skip <= isz`
        # hold, `skip <= osz` alone refuses it -- before the skipped bytes are copied, which would write one byte into the next frame's output
        tiny = raw[:3]
        tpay = codec_payload(codec, tiny)
        assert tpay[:2] == bytes([4, 3]) and len(tpay) >= 5
        add(": bytes_to_skip larger than the output", codec, codec_frame(codec, tpay, 2, general), codec_frame(codec, tpay, 3, general), tiny)
        # [width][1] and nothing else: `2 + skip <= isz`
        add(": a payload of two bytes, bytes_to_skip 1", codec, codec_frame(codec, bytes([4, 1]), len(raw), general), good, raw)

    # -- Delta: the deltas against the output --
    raw = codec_column(DELTA).tobytes()[:-2]
    pay = codec_payload(DELTA, raw)
    good = codec_frame(DELTA, pay, len(raw), OC.METHOD_LZ4)
    # bytes_to_skip 2 -> 1: the deltas are as many as out_size - skip, 4 * 129 + 1 of them: `n_bytes % w`
    add(": deltas not a multiple of the width", DELTA, codec_frame(DELTA, bytes([4, 1]) + pay[2:], len(raw), OC.METHOD_LZ4), good, raw)
    add(": deltas one element short", DELTA, codec_frame(DELTA, pay[:-4], len(raw), OC.METHOD_LZ4), good, raw)               # `n_bytes != out_size - skip`
    add(": deltas one element beyond", DELTA, codec_frame(DELTA, pay + bytes(4), len(raw), OC.METHOD_LZ4), good, raw)        # `n_bytes != out_size - skip`

    # -- DoubleDelta: every store is checked against the output's end (`d + width > d_end`, three places) --
    raw = codec_column(DD).tobytes()
    pay = codec_payload(DD, raw)
    good = codec_frame(DD, pay, len(raw))
    add(": output too small for the first value", DD, codec_frame(DD, pay, 3), good, raw)
    add(": output too small for the second value", DD, codec_frame(DD, pay, 7), good, raw)
    add(": output one value smaller than items", DD, codec_frame(DD, pay, len(raw) - 4), good, raw)

    # -- Gorilla --
    raw = codec_column(GOR).tobytes()
    pay = codec_payload(GOR, raw)
    good = codec_frame(GOR, pay, len(raw))
    assert struct.unpack_from("<I", pay, 2)[0] == 130
    add(": items one more than the output has room for", GOR, codec_frame(GOR, pay[:2] + struct.pack("<I", 131) + pay[6:], len(raw)), good, raw)   # `items * width > osz - skip`
    # two equal values: the stream is the bit 0.  With 10 in its place the second value asks for the previous window of leading and trailing
    # zeros, and there is none yet: `lz == 0 && db == 0 && tz == 0`
    two = np.array([0x40490FDB, 0x40490FDB], dtype=np.uint32).tobytes()
    tpay = codec_payload(GOR, two)
    assert len(tpay) == 2 + 4 + 4 + 1 and tpay[-1] == 0
    add(": control bits 10 before any window", GOR, codec_frame(GOR, tpay[:-1] + b"\x80", 8), codec_frame(GOR, tpay, 8), two)

    # -- T64 --
    values = codec_column(T64)
    raw, pay = values.tobytes(), codec_payload(T64, values)
    good = codec_frame(T64, pay, len(raw))
    nb = t64_num_bits(pay)
    assert len(pay) == 17 + 3 * 8 * nb and nb >= 9
    for cookie in (0, 0x7F):
        add(f": cookie {cookie:#x}", T64, codec_frame(T64, bytes([cookie]) + pay[1:], len(raw)), good, raw)   # no such MagicNumber: `default: bad = true`
    add(": a payload of 16 bytes", T64, codec_frame(T64, pay[:16], len(raw)), good, raw)                      # `isz < 17`
    add(": output not a multiple of the width", T64, codec_frame(T64, pay, len(raw) + 1), good, raw)          # `osz % width`
    add(": body one byte long", T64, codec_frame(T64, pay + b"\x00", len(raw)), good, raw)                    # `body % shift`
    add(": body one byte short", T64, codec_frame(T64, pay[:-1], len(raw)), good, raw)                        # `body % shift`
    add(": body one block short", T64, codec_frame(T64, pay[:-8 * nb], len(raw)), good, raw)                  # `num_full * 64 + tail != n`
    add(": body one block long", T64, codec_frame(T64, pay + bytes(8 * nb), len(raw)), good, raw)             # `num_full * 64 + tail != n`
    return cases


def quiet_codec_cases():
    """DoubleDelta and Gorilla frames whose payload ends early: the reference returns without an error and so does the kernel.
    -> [(name, codec, frame, bytes the format defines -- the skipped bytes and the values decoded before the payload ended; the frame
    promises more output than that, and what stands behind them is not defined)]"""
    cases = []
    for codec in (OC.METHOD_DOUBLE_DELTA, OC.METHOD_GORILLA):
        head = 2 if codec == OC.METHOD_DOUBLE_DELTA else 1      # values in front of the bit stream
        # one-bit codes only (a constant step / a constant value), head + 8 * 16 values behind 2 skipped bytes: a stream of 16 whole bytes
        n = head + 128
        v = (1000 + 37 * np.arange(n)).astype(np.uint32) if codec == OC.METHOD_DOUBLE_DELTA else np.full(n, 0x40490FDB, dtype=np.uint32)
        raw = b"\xAB\xCD" + v.tobytes()
        pay = codec_payload(codec, raw)
        at = 2 + 2 + 4 + 4 * head                             # where the bit stream begins
        assert len(pay) == at + 16 and pay[:2] == bytes([4, 2])

        def add(what, payload, defined):
            cases.append((f"{CODEC_NAMES[codec]}: {what}", codec, codec_frame(codec, payload, len(raw)), raw[:defined]))

        add("the stream ends after 5 of its 16 bytes", pay[:at + 5], 2 + 4 * (head + 40))
        add("the payload ends inside items", pay[:2 + 2 + 3], 2)
        add("the payload ends inside the first value", pay[:2 + 2 + 4 + 3], 2)
        if codec == OC.METHOD_DOUBLE_DELTA:
            add("the payload ends inside the first delta", pay[:2 + 2 + 4 + 4 + 3], 2 + 4)
        add("items is 0", pay[:4] + bytes(4) + pay[8:], 2)
    return cases


def empty_stage_file(codec):
    """three CODEC(codec, NONE) frames that promise 4 bytes each and whose stored stage is 0 bytes long: no stage header at all (`ssz < 9`
    in codec_io).  The call's stage buffer has no bytes to hold, and the codec kernels must still take these frames as theirs."""
    return codec_frame(codec, b"", 4, OC.METHOD_NONE, stage=b"") * 3


def codec_payload_of(frame):
    """-> (the codec's payload as its kernel sees it, the output size the frame promises), for a frame made by codec_frame"""
    _, csize, out_size = struct.unpack_from("<BII", frame, OC.CHECKSUM)
    body = frame[OC.CHECKSUM + OC.HEADER:OC.CHECKSUM + csize]
    if frame[OC.CHECKSUM] != OC.METHOD_MULTIPLE:
        return body, out_size
    general, gsize, stage_size = struct.unpack_from("<BII", body, 3)
    block = body[3 + OC.HEADER:3 + gsize]
    stage = block if general == OC.METHOD_NONE else OC.lz4_decompress(block, stage_size)
    return stage[OC.HEADER:], out_size


def codec_neighbours(like):
    """two well-formed frames of the codec chain of the frame `like` (CODEC(codec) or CODEC(codec, general)) to stand on both sides of a
    malformed one -> [(frame, bytes)]"""
    codec, general = like[OC.CHECKSUM], None
    if codec == OC.METHOD_MULTIPLE:
        codec, general = like[OC.CHECKSUM + OC.HEADER + 1], like[OC.CHECKSUM + OC.HEADER + 2]
    out = []
    for seed in (1, 2):
        v = codec_column(codec, 200 + seed, seed)
        out.append((codec_frame(codec, codec_payload(codec, v), v.nbytes, general), v.tobytes()))
    return out
