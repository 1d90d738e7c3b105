"""The frame decoders of compress_kernels.hip at their window, ring and bit-stream edges: crafted LZ4 blocks around LZ_IN / LZ_RING /
LZ_CHUNK and the fast path's limits, more frames than the grid has waves (a wave's second frame finds the first one's bytes in its LDS
ring and window), malformed variants of one block between well-formed neighbours, the Delta stage at every skip and block count, DoubleDelta
and Gorilla streams of every short length, T64 at every num_bits and under every type cookie, and codec frames with one header field
changed (or a payload that ends early) between well-formed neighbours.

Every input comes from tests/frame_craft.py; tests/test_frame_craft.py asserts, without a GPU, that the C oracle decodes each of them to
the expected bytes (or refuses it) and that the sets cover the paths named here.  Every comparison is byte for byte."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frame_craft as F  # noqa: E402
from oracle import compression as OC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


@pytest.fixture(scope="module")
def ctx(ch):
    c = ch.Context(0)
    yield c
    c.close()


def _decode(ch, ctx, buf):
    from clickhouse_amd import compression as CC
    frames = CC.parse_frames(buf)
    return CC.decompress_frames(ctx, ctx.upload(np.frombuffer(buf, dtype=np.uint8)), frames).numpy().tobytes(), len(frames)


def _check_file(ch, ctx, named, what=""):
    """named = [(name, frame, the bytes it decodes to)]: one file, one device call, compared frame by frame"""
    got, n = _decode(ch, ctx, b"".join(f for _, f, _ in named))
    assert n == len(named) and len(got) == sum(len(w) for _, _, w in named), (what, n, len(got))
    if got == b"".join(w for _, _, w in named):
        return
    at = 0
    for name, _, want in named:
        part = got[at:at + len(want)]
        if part != want:
            k = next(i for i in range(len(want)) if part[i] != want[i])
            pytest.fail(f"{what}: frame '{name}' ({len(want)} bytes at {at}) differs first at byte {k}: got {part[k]}, want {want[k]}; "
                        f"{sum(a != b for a, b in zip(part, want))} bytes differ")
        at += len(want)


# ---- crafted LZ4 frames ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(F.LZ4_GROUPS))
def test_crafted_lz4_frames(ch, ctx, group):
    named = []
    for case in F.LZ4_GROUPS[group]():
        block, raw = case.build()
        named.append((case.name, F.lz4_frame(block, len(raw)), raw))
    _check_file(ch, ctx, named, group)
    # stored frames of 1 / 63 / 64 / 65 bytes in between: every crafted frame begins at another output offset, odd ones among them
    rng = np.random.Generator(np.random.PCG64(3))
    mixed = []
    for i, item in enumerate(named):
        stored = rng.integers(0, 256, size=(1, 63, 64, 65)[i % 4], dtype=np.uint8).tobytes()
        mixed += [(f"stored {len(stored)}", F.none_frame(stored), stored), item]
    _check_file(ch, ctx, mixed, group + ", stored frames in between")


def test_ring_limit_blocks_through_the_stage_buffer(ch, ctx):
    """the same blocks as the general stage of CODEC(Delta(1), LZ4): k_lz4_decode writes the stage buffer (post = 0x92)"""
    named = [(case.name,) + F.delta_lz4_frame(case, 1) for case in F.ring_limit_cases()]
    _check_file(ch, ctx, named, "ring_limits behind Delta(1)")


@functools.lru_cache(maxsize=None)
def _pool(kind):
    if kind == "t64":
        return [(name, F.t64_frame(v, bit), v.tobytes()) for name, _, v in F.t64_small_pool() for bit in (False, True)]
    named = []
    for case in F.small_block_pool():
        if kind == "lz4":
            block, raw = case.build()
            named.append((case.name, F.lz4_frame(block, len(raw)), raw))
        else:
            named.append((case.name,) + F.delta_lz4_frame(case, {"delta1": 1, "delta8": 8}[kind]))
    return named


@pytest.mark.parametrize("kind", ["lz4", "delta1", "delta8", "t64"])
def test_more_frames_than_waves(ch, ctx, kind):
    """k_lz4_decode and k_delta_decode run min(ceil(frames / 4), CUs * 8) workgroups of four waves, k_t64_decode at most 4096 workgroups:
    with more than 32 * CUs frames every wave (every workgroup of the T64 kernel) takes a second and a third frame"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * 32 * cus + 37
    if n > 70_000:
        pytest.fail(f"{cus} compute units want {n} frames: give this test a smaller pool before it runs on such a device")
    assert n > 32 * cus and (kind != "t64" or n > 4096)
    pool = _pool(kind)
    order = np.random.Generator(np.random.PCG64(11)).integers(0, len(pool), size=n)
    stride = 32 * cus if kind != "t64" else 4096
    assert (order[:-stride] != order[stride:]).mean() > 0.9     # the frames one wave takes in turn differ
    want = b"".join(pool[i][2] for i in order)
    got, frames = _decode(ch, ctx, b"".join(pool[i][1] for i in order))
    assert frames == n and len(got) == len(want)
    if got != want:
        at = 0
        for j, i in enumerate(order):
            w = pool[i][2]
            assert got[at:at + len(w)] == w, f"{kind}: frame {j} of {n} ('{pool[i][0]}', the {j // stride + 1}. of its wave) differs"
            at += len(w)


# ---- malformed crafted LZ4 frames ----------------------------------------------------------------------------------------------------------
_MALFORMED = F.malformed_lz4_cases()


@pytest.mark.parametrize("case", _MALFORMED, ids=[c[0] for c in _MALFORMED])
def test_malformed_lz4_frame_between_well_formed_ones_is_refused(ch, ctx, case):
    """one field of one block changed (frame_craft.malformed_lz4_cases names the check of k_lz4_decode that refuses each); frames of 9 KiB
    stand on both sides in the same buffers.  The context then decodes the well-formed file."""
    from clickhouse_amd import compression as CC
    bad_file, good_file, want = F.malformed_file(case)
    with pytest.raises(ValueError):
        OC.read_frames(bad_file)
    frames = CC.parse_frames(bad_file)   # sizes and checksums are in order
    with pytest.raises(ch.ChgpuError) as e:
        CC.decompress_frames(ctx, ctx.upload(np.frombuffer(bad_file, dtype=np.uint8)), frames)
    assert e.value.code == ch._capi.ERR_BAD_ARGUMENTS
    got, n = _decode(ch, ctx, good_file)
    assert n == 3 and got == want


# ---- Delta, DoubleDelta, Gorilla at short and odd sizes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("width", F.WIDTHS)
def test_delta_at_every_skip_and_block_count(ch, ctx, width):
    named = [(f"Delta({width}) skip={skip} k={k}", F.delta_lz4_frame_of_raw(raw, width), raw) for skip, k, raw in F.delta_raws(width)]
    assert OC.read_frames(b"".join(f for _, f, _ in named)) == b"".join(r for _, _, r in named)
    _check_file(ch, ctx, named, f"Delta({width})")


@pytest.mark.parametrize("width", F.WIDTHS)
@pytest.mark.parametrize("codec", ["dd", "gorilla"])
def test_short_bit_streams(ch, ctx, codec, width):
    """one frame per encoder call, all frames of a width in one file: a lane per frame, 64 streams of different lengths side by side"""
    named = []
    for name, raw in F.stream_raws(codec, width):
        frame = F.stream_frame(codec, raw, width)
        decoded = OC.read_frames(frame)
        assert decoded == raw, (codec, width, name)
        named.append((f"{codec} width={width} {name}", frame, decoded))
    _check_file(ch, ctx, named, f"{codec} width={width}")


# ---- T64 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", F.T64_TYPES, ids=[np.dtype(t).name for t in F.T64_TYPES])
def test_t64_at_every_num_bits(ch, ctx, dtype):
    named = []
    for name, nb, values in F.t64_sequences(dtype):
        for bit in (False, True):
            frame = F.t64_frame(values, bit)
            assert F.t64_num_bits(frame[OC.CHECKSUM + OC.HEADER:]) == nb
            named.append((f"{name} {'bit' if bit else 'byte'} variant", frame, values.tobytes()))
    assert OC.read_frames(b"".join(f for _, f, _ in named)) == b"".join(r for _, _, r in named)
    _check_file(ch, ctx, named, np.dtype(dtype).name)


@pytest.mark.parametrize("cookie", sorted(F.T64_ALIAS_COOKIES))
def test_t64_alias_cookies_decode_like_their_integer_type(ch, ctx, cookie):
    dt = F.T64_ALIAS_COOKIES[cookie]
    picked = [s for s in F.t64_sequences(dt) if s[2].shape[0] in (1, 65)][::3]
    assert len(picked) >= 8
    plain, alias = [], []
    for name, _, values in picked:
        for bit in (False, True):
            plain.append((name, F.t64_frame(values, bit), values.tobytes()))
            alias.append((f"cookie {cookie}: {name}", F.t64_frame(values, bit, cookie), values.tobytes()))
            assert alias[-1][1][OC.CHECKSUM + OC.HEADER] & 0x7F == cookie != plain[-1][1][OC.CHECKSUM + OC.HEADER] & 0x7F
    assert OC.read_frames(b"".join(f for _, f, _ in alias)) == b"".join(r for _, _, r in alias)
    _check_file(ch, ctx, plain, f"integer cookie of {np.dtype(dt).name}")
    _check_file(ch, ctx, alias, f"cookie {cookie}")


# ---- malformed and early-ending codec frames ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", list(F.CODEC_NAMES), ids=list(F.CODEC_NAMES.values()))
def test_malformed_codec_frame_between_well_formed_ones_is_refused(ch, ctx, codec):
    """one header field of one codec frame changed (frame_craft.malformed_codec_cases names the field, and the check of the kernel that
    refuses it); well-formed frames of the same codec chain stand on both sides.  The context then decodes the well-formed twins."""
    from clickhouse_amd import compression as CC
    cases = [c for c in F.malformed_codec_cases() if c[1] == codec]
    assert len(cases) >= 20
    not_refused, twins = [], []
    for name, _, bad, good, raw in cases:
        (before, raw_b), (after, raw_a) = F.codec_neighbours(good)
        bad_file = before + bad + after
        frames = CC.parse_frames(bad_file)   # sizes and checksums are in order
        assert len(frames) == 3, name
        try:
            CC.decompress_frames(ctx, ctx.upload(np.frombuffer(bad_file, dtype=np.uint8)), frames)
            not_refused.append(name)
        except ch.ChgpuError as e:
            assert e.code == ch._capi.ERR_BAD_ARGUMENTS, name
        twins += [(f"before {name}", before, raw_b), (name, good, raw), (f"after {name}", after, raw_a)]
    assert not not_refused
    _check_file(ch, ctx, twins, f"the well-formed twins of {F.CODEC_NAMES[codec]}")


def test_codec_payloads_that_end_early_end_quietly(ch, ctx):
    """DoubleDelta / Gorilla payloads that end before `items` values, before the first value or the first delta, or with items 0: no error,
    as in the reference, and the bytes the format defines stand in the frame's place.  What lies behind them is not compared."""
    cases = F.quiet_codec_cases()
    named = []
    for name, codec, frame, defined in cases:
        (before, raw_b), (after, raw_a) = F.codec_neighbours(frame)
        named += [(before, raw_b, len(raw_b)), (frame, defined, len(OC.read_frames(frame))), (after, raw_a, len(raw_a))]
    got, n = _decode(ch, ctx, b"".join(f for f, _, _ in named))
    assert n == len(named) and len(got) == sum(size for _, _, size in named)
    at = 0
    for i, (_, defined, size) in enumerate(named):
        assert got[at:at + len(defined)] == defined, cases[i // 3][0] + ("" if i % 3 == 1 else ": a neighbour")
        at += size


@pytest.mark.parametrize("codec", list(F.CODEC_NAMES), ids=list(F.CODEC_NAMES.values()))
def test_a_file_whose_codec_stages_are_all_empty_is_refused(ch, ctx, codec):
    """no byte of stage output in the whole call: every codec still takes the frames as stages of its own and refuses them (none has a
    stage header), and the context then decodes a well-formed file of the same chain"""
    from clickhouse_amd import compression as CC
    buf = F.empty_stage_file(codec)
    frames = CC.parse_frames(buf)
    assert len(frames) == 3 and all(f[4] == codec and f[5] == 0 and f[3] == 4 for f in frames)
    with pytest.raises(ch.ChgpuError) as e:
        CC.decompress_frames(ctx, ctx.upload(np.frombuffer(buf, dtype=np.uint8)), frames)
    assert e.value.code == ch._capi.ERR_BAD_ARGUMENTS
    like = F.codec_frame(codec, F.codec_payload(codec, F.codec_column(codec)), 4 * 130, OC.METHOD_NONE)
    _check_file(ch, ctx, [(f"neighbour {i}", f, r) for i, (f, r) in enumerate(F.codec_neighbours(like))], "after the empty stages")
