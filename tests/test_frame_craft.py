"""tests/frame_craft.py against the C oracle, without a GPU: every crafted LZ4 block decodes to the bytes its builder kept, every malformed
case is refused, every codec input round-trips -- and the sets cover what tests/test_gpu_frame_decoder_edges.py relies on them to cover."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frame_craft as F  # noqa: E402
from oracle import compression as OC  # noqa: E402


@pytest.fixture(scope="module")
def built():
    """{group: [(case, block, decoded bytes)]}, built once"""
    return {g: [(c,) + c.build() for c in make()] for g, make in F.LZ4_GROUPS.items()}


def test_every_crafted_block_decodes_in_the_oracle_to_the_builders_bytes(built):
    total = 0
    for group, cases in built.items():
        assert len({c.name for c, _, _ in cases}) == len(cases), group
        for case, block, raw in cases:
            assert len(raw) == case.decoded_len, case.name
            assert OC.lz4_decompress(block, len(raw)) == raw, case.name
            total += 1
    assert total >= 490
    # the same blocks with a Delta stage's header in front: the stage the oracle decodes is the builder's
    for case in F.ring_limit_cases()[:20] + F.small_block_pool():
        for w in (1, 8):
            frame, want = F.delta_lz4_frame(case, w)
            assert OC.read_frames(frame) == want, (case.name, w)


def test_the_walk_returns_what_the_builder_was_given(built):
    for cases in built.values():
        for case, block, _ in cases:
            got = F.walk_sequences(block)
            assert [s[:3] for s in got] == case.seqs + [(case.end, 0, 0)], case.name
            assert got[0][3] == 0 and all(a[3] < b[3] for a, b in zip(got, got[1:]))


def test_the_crafted_set_covers_the_paths_it_is_meant_for(built):
    seqs = [s for cases in built.values() for _, block, _ in cases for s in F.walk_sequences(block, with_offset_position=True)]
    offsets = {s[1] for s in seqs}
    assert {F.LZ_CHUNK, F.LZ_CHUNK + 1, F.LZ_FAST_FAR, F.LZ_FAST_FAR + 1} <= offsets            # 2048, 2049, 4032, 4033
    # a literal run longer than the ring, then at once a match the ring serves
    assert any(lit > F.LZ_RING and 0 < off <= F.LZ_CHUNK for lit, off, _, _, _ in seqs)
    # a literal run that leaves the window, and one inside it
    assert any(lit > F.LZ_IN for lit, *_ in seqs) and any(15 <= lit < F.LZ_IN for lit, *_ in seqs)
    # far matches (read from the output buffer) that overlap themselves, and that do not; matches longer than the ring on both paths
    assert any(off > F.LZ_CHUNK and ml > off for _, off, ml, _, _ in seqs) and any(off > F.LZ_CHUNK and 0 < ml <= off for _, off, ml, _, _ in seqs)
    assert any(off > F.LZ_CHUNK and ml > F.LZ_RING for _, off, ml, _, _ in seqs) and any(0 < off <= F.LZ_CHUNK and ml > F.LZ_RING for _, off, ml, _, _ in seqs)
    # ring-served matches of more than one chunk, with a period that is a power of two and one that is not
    assert any(ml > F.LZ_CHUNK and off == 64 for _, off, ml, _, _ in seqs) and any(ml > F.LZ_CHUNK and off == 65 for _, off, ml, _, _ in seqs)
    # header fields against the window end: the first window of a frame is in[0, 1024), so positions 1023 and 1024 are its last byte and
    # the first byte behind it (positions == 1023 / 0 mod 1024 in general)
    tokens = {s[3] for s in seqs}
    assert F.LZ_IN - 1 in tokens and F.LZ_IN in tokens
    assert any(t % F.LZ_IN == F.LZ_IN - 1 for t in tokens) and any(t and t % F.LZ_IN == 0 for t in tokens)
    assert any(s[4] == F.LZ_IN - 1 for s in seqs)                                                 # an offset field with one byte on each side
    # ... by the window rule of the kernel as frame_craft.decoder_trace restates it, a fetch is made for every kind of header field, for
    # an offset field with none and with one of its bytes still at hand, for the first and the second literal-length byte and for each
    # of three match-length bytes
    refills = [(field, had, at - s[3]) for _, block, raw in built["window_end"] for field, at, had in F.decoder_trace(block, len(raw))[0] if at
               for s in F.walk_sequences(block) if s[3] <= at < s[3] + 1 + 2 + s[0] + 2 + 3]
    assert {("token", 0), ("offset", 0), ("offset", 1)} <= {r[:2] for r in refills}
    assert {1, 2} <= {r[2] for r in refills if r[0] == "literal length"}
    assert {273 + 5, 273 + 6, 273 + 7} <= {r[2] for r in refills if r[0] == "match length"}
    # fast-path-shaped sequences that end 5 .. 39 bytes before the frame's end: both sides of the 32 free output bytes
    tails = {case.end for case, _, _ in built["frame_end"]}
    assert tails == set(range(5, 40)) and min(tails) < F.FAST_OUT - 18 and max(tails) > F.FAST_OUT


def test_the_sequences_behind_a_long_run_are_read_by_the_fast_path(built):
    """the (3 literals, match 7) sequences that follow a long literal run or match are there to read, through the fast path, what that run
    left in the ring: by the rules frame_craft.decoder_trace restates, each of them up to offset 4032 is read in one go and 4033 is not"""
    behind = {}
    for group in ("ring_limits", "long_literals", "long_matches"):
        for case, block, raw in built[group]:
            fast = F.decoder_trace(block, len(raw))[1]
            seqs = F.walk_sequences(block)
            assert seqs[0][3] not in fast
            for lit, off, ml, at in seqs[1:-1]:
                assert (lit, ml) == (3, 7) and (at in fast) == (off <= F.LZ_FAST_FAR), (case.name, off)
                for kind, is_kind in (("far match", seqs[0][1] > F.LZ_CHUNK), ("ring match longer than the ring", seqs[0][1] <= F.LZ_CHUNK and seqs[0][2] > F.LZ_RING),
                                      ("literals longer than the ring", seqs[0][0] > F.LZ_RING),
                                      ("far match longer than the ring", seqs[0][1] > F.LZ_CHUNK and seqs[0][2] > F.LZ_RING)):
                    if is_kind and at in fast:
                        behind.setdefault(kind, set()).add(off)
    assert behind["far match"] >= {1, 3, 8, 2048, F.LZ_FAST_FAR} and behind["literals longer than the ring"] >= {1, 3, 8, 2048, F.LZ_FAST_FAR}
    assert behind["ring match longer than the ring"] >= {1, 5, 2048, 2049, F.LZ_FAST_FAR}
    assert behind["far match longer than the ring"] >= {1, 5, 2048, 2049, F.LZ_FAST_FAR}   # (beyond 2048 only the fast path reads the ring)
    # in the frame-end group the input decides: a sequence is read in one go only while 64 input bytes lie behind its token, and the closing
    # literals are fewer, so the last sequences of every case go the general way whatever output is left (no well-formed block has 64 input
    # bytes that yield fewer than 32 output bytes)
    for case, block, raw in built["frame_end"]:
        fast = F.decoder_trace(block, len(raw))[1]
        seqs = F.walk_sequences(block)
        assert seqs[1][3] in fast and seqs[-2][3] not in fast


def test_the_small_block_pool_is_small_distinct_and_of_both_shapes():
    pool = F.small_block_pool()
    blocks = [c.build() for c in pool]
    assert len({b for b, _ in blocks}) == len(pool) >= 64
    assert all(50 <= len(raw) <= 300 for _, raw in blocks)
    fast_only = [all(lit < 15 and ml < 19 for lit, _, ml in c.seqs) for c in pool]
    assert sum(fast_only) >= 20 and len(pool) - sum(fast_only) >= 20
    for (b, raw) in blocks:
        assert OC.lz4_decompress(b, len(raw)) == raw


def test_the_oracle_refuses_every_malformed_case():
    cases = F.malformed_lz4_cases()
    assert len({c[0] for c in cases}) == len(cases) >= 11
    for case in cases:
        name, method, payload, claimed, good_payload, raw = case
        if method == OC.METHOD_LZ4:
            assert OC.lz4_decompress(good_payload, len(raw)) == raw, name
            with pytest.raises(ValueError):
                OC.lz4_decompress(payload, claimed)
        bad_file, good_file, want = F.malformed_file(case)
        frames = OC.parse_frames(bad_file)                       # the checksums are right: only the decoder can tell
        assert len(frames) == 3 and frames[0][3] >= 8192 and frames[2][3] >= 8192 and frames[0][2] >= 8192 and frames[2][2] >= 8192
        with pytest.raises(ValueError):
            OC.read_frames(bad_file)
        assert OC.read_frames(good_file) == want, name


@pytest.mark.parametrize("width", F.WIDTHS)
def test_delta_inputs_wrap_in_every_block_and_round_trip(width):
    seen = set()
    for skip, k, raw in F.delta_raws(width):
        assert len(raw) == skip + k * width
        seen.add((skip, k))
        x = np.frombuffer(raw[skip:], dtype=F.UINT[width])
        for lo in range(0, k, 64):                               # the 64 deltas one wave step sums
            i = np.arange(max(lo, 1), min(lo + 64, k))
            if i.size:
                assert (x[i] < x[i - 1]).any(), (width, skip, k, lo)   # a value below the one before it: the running sum wrapped
        assert OC.read_frames(F.delta_lz4_frame_of_raw(raw, width)) == raw
    assert seen == {(s, k) for s in range(width) for k in F.DELTA_COUNTS}


@pytest.mark.parametrize("width", F.WIDTHS)
@pytest.mark.parametrize("codec", ["dd", "gorilla"])
def test_stream_inputs_round_trip_and_cover_every_short_stream_length(codec, width):
    lengths, skips = set(), set()
    for name, raw in F.stream_raws(codec, width):
        frame = F.stream_frame(codec, raw, width)
        payload = frame[OC.CHECKSUM + OC.HEADER:]
        assert payload[0] == width and payload[1] == len(raw) % width
        assert OC.read_frames(frame) == raw, (codec, width, name)
        lengths.add(F.bit_stream_len(codec, payload, width))
        skips.add(payload[1])
    assert set(range(72)) <= lengths, sorted(set(range(72)) - lengths)   # every queue depth 0 .. 6 of 8-byte words in front of every tail 0 .. 7, and more
    assert skips == set(range(width))


@pytest.mark.parametrize("dtype", F.T64_TYPES)
def test_t64_inputs_take_every_num_bits(dtype):
    bits = 8 * np.dtype(dtype).itemsize
    seqs = F.t64_sequences(dtype)
    for bit in (False, True):
        seen = {}
        for name, nb, values in seqs:
            payload = OC.t64_encode(values, bit)
            assert F.t64_num_bits(payload) == nb, name
            assert struct.unpack_from("<q" if values.dtype.kind == "i" else "<Q", payload, 1)[0] == int(values.min()), name
            assert OC.t64_decode(payload, values.nbytes) == values.tobytes(), name
            seen.setdefault(nb, set()).add(values.shape[0])
        assert sorted(seen) == list(range(bits + 1))
        assert all(seen[nb] >= set(F.T64_COUNTS) for nb in range(1, bits + 1)) and seen[0] >= {1} | set(F.T64_COUNTS)
    if np.dtype(dtype).kind == "i":   # every num_bits from ranges across zero too, each side of `min + max >= 0` (1 only where min decides)
        for side, first in (("max decides", 2), ("min decides", 1)):
            assert {nb for name, nb, _ in seqs if side in name} == set(range(first, bits + 1))


def test_t64_alias_cookies_decode_like_their_integer_type():
    for cookie, dt in F.T64_ALIAS_COOKIES.items():
        values = next(v for _, nb, v in F.t64_sequences(dt) if nb == 5 and v.shape[0] == 65)
        for bit in (False, True):
            frame = F.t64_frame(values, bit, cookie)
            assert frame[OC.CHECKSUM + OC.HEADER] & 0x7F == cookie and frame[OC.CHECKSUM + OC.HEADER] >> 7 == int(bit)
            assert OC.read_frames(frame) == values.tobytes() == OC.read_frames(F.t64_frame(values, bit)), cookie
    assert len(F.t64_small_pool()) >= 32


def test_every_malformed_codec_case_has_the_recorded_verdict_of_the_oracle():
    """the well-formed twin of every case decodes to the expected bytes; the malformed frame passes the frame walk (sizes and checksum hold)
    and the oracle either refuses it or -- the cases of KERNEL_STRICTER_THAN_ORACLE, no others -- decodes it to something"""
    cases = F.malformed_codec_cases()
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names) and F.KERNEL_STRICTER_THAN_ORACLE <= set(names)
    for codec, cname in F.CODEC_NAMES.items():
        for general in F.GENERAL_NAMES.values():                 # six stage-header cases per codec and general-purpose stage
            assert sum(n.startswith(f"{cname} behind {general}: stage header") for n in names) == 6
    for cname in ("Delta", "DoubleDelta", "Gorilla"):
        assert {f"{cname}: width {w}" for w in (0, 3, 16)} | {f"{cname}: bytes_to_skip == width", f"{cname}: bytes_to_skip larger than the output",
                                                               f"{cname}: a payload of two bytes, bytes_to_skip 1"} <= set(names)
    # the four conditions of the [width][bytes_to_skip] check, restated: each of its cases fails exactly the one its name states
    named = {"width": 0, "bytes_to_skip == width": 1, "bytes_to_skip larger than the output": 2, "a payload of two bytes": 3}
    seen = set()
    for name, codec, bad, good, raw in cases:
        which = [k for what, k in named.items() if f": {what}" in name]
        if which:
            pay, osz = F.codec_payload_of(bad)
            holds = (pay[0] in (1, 2, 4, 8), pay[1] < pay[0], pay[1] <= osz, 2 + pay[1] <= len(pay))
            failing = [k for k in range(4) if not holds[k]]
            assert failing == which or (name.endswith("width 0") and failing == [0, 1]), (name, holds)   # (no skip is below width 0)
            seen.add((codec, which[0]))
            pay, osz = F.codec_payload_of(good)
            assert pay[0] in (1, 2, 4, 8) and pay[1] < pay[0] and pay[1] <= osz and 2 + pay[1] <= len(pay), name
    assert seen == {(c, k) for c in F.WIDTH_SKIP_CODECS for k in range(4)}
    accepted = set()
    for name, codec, bad, good, raw in cases:
        assert len(raw) <= 4 * 300 and OC.read_frames(good) == raw, name
        assert len(OC.parse_frames(bad)) == 1, name
        try:
            OC.read_frames(bad)
            accepted.add(name)
        except ValueError:
            pass
    assert accepted == F.KERNEL_STRICTER_THAN_ORACLE
    chains = set()
    for name, codec, bad, good, raw in cases:
        sides = F.codec_neighbours(good)
        chains.add(tuple(f for f, _ in sides))
        assert all(OC.read_frames(f) == r and len(r) <= 4 * 300 for f, r in sides), name
    assert len(chains) == 4 * 2 + 3                              # every codec behind LZ4 and NONE; T64, DoubleDelta and Gorilla alone


def test_the_oracle_ends_the_quiet_codec_cases_without_an_error_behind_the_defined_bytes():
    cases = F.quiet_codec_cases()
    assert len(cases) == 9 and len({c[0] for c in cases}) == 9
    for name, codec, frame, defined in cases:
        got = OC.read_frames(frame)                              # no error
        assert len(got) > len(defined) >= 2 and got[:len(defined)] == defined, name
        assert not any(got[len(defined):]), name                 # nothing was decoded behind them (the oracle's buffer begins as zeros)


def test_the_oracle_refuses_frames_whose_codec_stage_is_empty():
    for codec in F.CODEC_NAMES:
        buf = F.empty_stage_file(codec)
        frames = OC.parse_frames(buf)
        assert len(frames) == 3 and all(f[0] == OC.METHOD_MULTIPLE and f[3] == 4 for f in frames)
        with pytest.raises(ValueError):
            OC.read_frames(buf)
