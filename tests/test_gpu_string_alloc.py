"""The ColumnString entry points behind their allocations: `test_string_fail_alloc` = N makes allocation N of a call answer OOM (the
numbered allocations of pair_pool.h), so every early return behind an allocation runs once, and the same call must then go through
and equal a reference that never saw the failure.  Next to it: the KernelLaunches a call of each entry point adds, pinned.

One column of 257 rows with duplicates serves every call but the sort, whose column shares its first 8-byte word among many values so
that the sort needs a second round."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import string_ref as sr  # noqa: E402
import string_sort_ref as ssr  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = 257


def _values():
    rng = random.Random(257)
    pool = [bytes(rng.choice(b"abc%") for _ in range(n)) for n in (0, 1, 3, 7, 8, 9, 15, 16, 17, 24, 40)] + [b"abcabc", b"xabcx", b"abc"]
    return [rng.choice(pool) for _ in range(ROWS)]


def _sort_values():
    rng = random.Random(258)
    tails = (b"", b"a", b"b", b"aaaaaaaa", b"aaaaaaaab", b"aaaaaaaaa", b"aaaaaaaabb")   # the last three share their first word, too
    return [b"sameword" + rng.choice(tails) for _ in range(ROWS)]


VALUES = _values()
SORT_VALUES = _sort_values()
MASK = (np.arange(ROWS) % 3 != 1).astype(np.uint8)
INDEX = (np.arange(ROWS, dtype=np.uint64) * 101 + 7) % ROWS


def _dictionary_ref(values):
    seen = {}
    ids = [seen.setdefault(v, len(seen)) for v in values]
    return list(seen), ids


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


@pytest.fixture(scope="module")
def ctx(ch):
    c = ch.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def calls(ch, ctx):
    """name -> (call, reference); every call returns plain host values"""
    col = ch.ColumnString.from_values(ctx, VALUES)
    sort_col = ch.ColumnString.from_values(ctx, SORT_VALUES)
    mask, index = ctx.upload(MASK), ctx.upload(INDEX)

    def encode():
        lc = col.dictionary_encode()
        return list(lc.dictionary), [int(i) for i in lc.indexes.numpy()]

    def predicate(fn, ref):
        return (lambda: [int(x) for x in fn().numpy()]), [int(ref(v)) for v in VALUES]

    return {
        "dictionary_encode": (encode, _dictionary_ref(VALUES)),
        "filter": (lambda: col.filter(mask).to_list(), [v for v, m in zip(VALUES, MASK) if m]),
        "index": (lambda: col.index(index).to_list(), [VALUES[int(i)] for i in INDEX]),
        "get_permutation": (lambda: [int(i) for i in sort_col.get_permutation().numpy()], ssr.get_permutation(SORT_VALUES)),
        "compare": predicate(lambda: col.compare(ch.LT, b"abc"), lambda v: sr.cmp_ref(ch.LT, v, b"abc")),
        "like_equals": predicate(lambda: col.like(b"abc"), lambda v: v == b"abc"),
        "like_general": predicate(lambda: col.like(b"a_c%c"), lambda v: sr.like_bytes(b"a_c%c", v)),
        "contains": predicate(lambda: col.contains(b"abc"), lambda v: b"abc" in v),
        "starts_with": predicate(lambda: col.starts_with(b"abc"), lambda v: v.startswith(b"abc")),
        "ends_with": predicate(lambda: col.ends_with(b"bc"), lambda v: v.endswith(b"bc")),
    }


# allocations of one call, all behind the refusal hook: the call's one pool allocation and its two result columns
EXACT = {"dictionary_encode": 3, "filter": 3, "index": 3}
NAMES = ["dictionary_encode", "filter", "index", "get_permutation", "compare", "like_equals", "like_general", "contains", "starts_with", "ends_with"]


def test_the_sort_column_needs_a_second_round():
    active = []
    assert ssr.word_round_model(SORT_VALUES, stats=active) == ssr.get_permutation(SORT_VALUES)
    assert len(active) >= 2 and active[0] == ROWS, active


@pytest.mark.parametrize("name", NAMES)
def test_a_refused_allocation_is_an_error_and_the_same_call_then_succeeds(ch, ctx, calls, name):
    call, want = calls[name]
    failed_at = []
    for nth in range(1, 256):
        ctx.set_option("test_string_fail_alloc", nth)
        refused = None
        try:
            got = call()
        except ch.ChgpuError as e:
            refused = e
        finally:
            ctx.set_option("test_string_fail_alloc", 0)
        if refused is None:
            assert got == want   # the call makes fewer than nth allocations: it went through
            break
        assert refused.code == ch._capi.ERR_OOM and "test_string_fail_alloc" in str(refused), (nth, str(refused))
        failed_at.append(nth)
        assert call() == want   # nothing of the failed call is left behind
    k = len(failed_at)
    assert k >= 1 and failed_at == list(range(1, k + 1)), failed_at
    if name in EXACT:
        assert k == EXACT[name], (name, k)
    if name == "get_permutation":
        # two rounds: the result, the segment table, two columns of active rows; per round two key columns, nine passes or more, the
        # round's flags and the next segment table; the second round's two columns of active rows
        assert k >= 4 + 2 * (2 + 9 + 2) + 2, k


LAUNCHES = {"dictionary_encode": 8, "filter": 9, "index": 6, "get_permutation": 133, "compare": 2, "like_equals": 2, "like_general": 2,
            "contains": 3, "starts_with": 2, "ends_with": 2}


@pytest.mark.parametrize("name", NAMES)
def test_the_kernel_launches_of_a_call_are_as_they_were(ctx, calls, name):
    """The constants are the KernelLaunches one call added on these columns in a run of the commit before string_column.h.  The
    counter's bookkeeping is uneven (a scan counts its three kernels, the filter's sizes kernel is counted with its move kernel, the
    walk over the offsets counts one) and is kept as it was."""
    call, want = calls[name]
    before = ctx.counters()["KernelLaunches"]
    assert call() == want
    delta = ctx.counters()["KernelLaunches"] - before
    print(f"KernelLaunches[{name}] = {delta}")
    assert delta == LAUNCHES[name], (name, delta)
