"""Builders of compressed frames whose every field is given, for the decoders of clickhouse_amd/csrc/compress_kernels.hip: LZ4 blocks written
sequence by sequence around the constants that choose a path in k_lz4_decode, malformed variants of one block, and Delta / DoubleDelta /
Gorilla / T64 inputs at short and odd sizes.  No GPU and no assertions about a decoder here: tests/test_frame_craft.py checks every builder
against the C oracle (oracle.compression) and asserts what the sets cover; tests/test_gpu_frame_decoder_edges.py sends them to the device.

Nothing is imported from the kernel.  The four constants it branches on, restated once:"""
import struct
import zlib

import numpy as np

from oracle import compression as OC

LZ_IN = 1024                # compress_kernels.hip:82   static constexpr u32 LZ_IN = 1024      (input window bytes per wave)
LZ_RING = 4096              # compress_kernels.hip:83   static constexpr u32 LZ_RING = 4096    (output ring bytes per wave)
LZ_CHUNK = LZ_RING // 2     # compress_kernels.hip:85   static constexpr u32 LZ_CHUNK = LZ_RING / 2   (ring-served matches: offset <= LZ_CHUNK)
LZ_FAST_FAR = LZ_RING - 64  # compress_kernels.hip:168  the largest offset the fast path serves from the ring
FAST_IN, FAST_OUT = 64, 32  # compress_kernels.hip:155  the fast path wants 64 readable window bytes and 32 free output bytes

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
    """how a decoder that keeps LZ_IN input bytes at hand reads a well-formed block, by the rules of compress_kernels.hip:121-144, :155
    and :168: a sequence of fast-path shape (fewer than 15 literals, a match below 19 from at most LZ_FAST_FAR back) whose next 64 input
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

    # Fewer than 64 input bytes follow the target in every truncated case, so `ip + 64 <= in_base + in_len` (:155) fails and the target
    # is parsed by the general path.
    block, raw, at, _ = _malformed_base((3, 5, 7))
    # the token says 3 literals and 0 bytes are left: `lit > isz - ip` (:225)
    add("ends after a token with literals", block[:at + 1], len(raw), block, raw)
    # after the 3 literals one byte is left: ip < isz, so no normal end (:254); `window(ip, 2)` is false for pos + 2 > isz (:122, :256)
    add("ends after one offset byte", block[:at + 1 + 3 + 1], len(raw), block, raw)
    block, raw, at, _ = _malformed_base((0, 5, 7))
    # the token says 0 literals and the input is used up: the loop ends as after a last sequence (:254), then `op != osz` (:349)
    add("ends after a token without literals", block[:at + 1], len(raw), block, raw)
    block, raw, at, _ = _malformed_base((300, 5, 7))
    # the token's 15 and the byte 255 are read, the chain goes on and `window(ip, 1)` is false at ip == isz (:213)
    assert block[at + 1] == 255
    add("ends inside a literal-length chain", block[:at + 2], len(raw), block, raw)
    block, raw, at, _ = _malformed_base((3, 5, 300))
    # token, 3 literals, offset, the byte 255 of the match length: `window(ip, 1)` is false at ip == isz (:269)
    assert block[at + 1 + 3 + 2] == 255
    add("ends inside a match-length chain", block[:at + 1 + 3 + 2 + 1], len(raw), block, raw)

    # the closing sequence's literal length 12 -> 13
    block, raw, _, _ = _malformed_base((3, 5, 7))
    close = walk_sequences(block)[-1][3]
    bad = bytearray(block)
    bad[close] = 13 << 4
    # 12 input bytes are left, and the output (claimed one byte longer) has room for 13: `lit > isz - ip` alone is true (:225)
    add("literal length one more than the input left", bad, len(raw) + 1, block, raw)
    # one more input byte so that 13 are there; the output has room for 12: `lit > osz - op` alone is true (:225)
    add("literal length one more than the output left", bad + b"\x00", len(raw), block, raw)

    # The target has fast-path shape and 72 input bytes behind it, so the fast path looks at it first: `offset - 1 < min(op + lit, 4032)`
    # (:168) is false for offset 0 (offset - 1 wraps to 2^32 - 1) and for offset op + lit + 1, and the general path takes it over.
    block, raw, at, op = _malformed_base((3, 5, 7), end=70)
    bad = bytearray(block)
    bad[at + 4:at + 6] = struct.pack("<H", 0)
    add("offset 0", bad, len(raw), block, raw)                                   # `offset == 0` (:282)
    bad = bytearray(block)
    bad[at + 4:at + 6] = struct.pack("<H", op + 3 + 1)
    add("offset one more than the output so far", bad, len(raw), block, raw)     # `offset > op` (:282), op counted behind the 3 literals

    # match length 30 -> 30 + 12 + 1: the 30 and the closing 12 literals are all the output left; one length byte either way
    block, raw, at, _ = _malformed_base((3, 5, 30))
    bad = bytearray(block)
    assert bad[at + 6] == 30 - 19
    bad[at + 6] = 30 + SHORT_END + 1 - 19
    add("match length one more than the output left", bad, len(raw), block, raw)  # `ml > osz - op` (:282)

    # a valid block under a header that claims one byte more or fewer
    block, raw, _, _ = _malformed_base((3, 5, 7))
    add("header claims one byte more", block, len(raw) + 1, block, raw)          # everything decodes; `op != osz` (:349)
    add("header claims one byte fewer", block, len(raw) - 1, block, raw)         # the closing 12 literals: `lit > osz - op` (:225)
    block, raw, _, _ = _malformed_base((3, 5, 7), end=0)                          # ... and a block that closes with an empty literal run
    add("header claims one byte more, last bytes a match", block, len(raw) + 1, block, raw)   # `op != osz` (:349)
    add("header claims one byte fewer, last bytes a match", block, len(raw) - 1, block, raw)  # the last match: `ml > osz - op` (:282)

    # method NONE: `isz != osz` (:107)
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
