"""tests/versioned_collapsing_ref.py against itself, without a GPU: the queue and the closed form agree on every sign sequence of up to 12
rows and on random groups, hand-written groups give the rows the contract names, a group emits |cp - cn| rows of the majority sign in
order, the same key under two versions does not cancel, and max_balance is the longest the queue was."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_sorted_ref as R  # noqa: E402
import versioned_collapsing_ref as V  # noqa: E402


def signs_of(text):
    return [1 if c == "+" else -1 for c in text]


def test_queue_and_closed_form_agree_on_every_short_sequence():
    cases = 0
    for n in range(13):
        for signs in itertools.product((1, -1), repeat=n):
            assert V.queue_of(signs) == V.closed_form_of(signs), signs
            cases += 1
    assert cases == 2**13 - 1


def test_queue_and_closed_form_agree_on_random_groups():
    rng = np.random.Generator(np.random.PCG64(1))
    for _ in range(300):
        n = int(rng.integers(1, 201))
        p = (0.5, 0.9, 0.1)[int(rng.integers(0, 3))]
        signs = np.where(rng.random(n) < p, 1, -1).tolist()
        assert V.queue_of(signs) == V.closed_form_of(signs)


@pytest.mark.parametrize("text, survivors, longest", [
    ("+", [0], 1), ("-", [0], 1), ("+-", [], 1), ("-+", [], 1), ("++-", [0], 2), ("+--+", [], 1), ("--+++", [4], 2),
    ("+++--", [0], 3), ("-+-+-", [4], 1), ("++--++", [4, 5], 2), ("+-++-+", [2, 5], 2)])
def test_hand_written_groups(text, survivors, longest):
    assert V.queue_of(signs_of(text)) == (survivors, longest)
    assert V.closed_form_of(signs_of(text)) == (survivors, longest)
    key = np.zeros(len(text), dtype=np.int64)
    sign = np.array(signs_of(text), dtype=np.int8)
    d = R.describe([key], [(0, False, 1)])
    for form in (V.versioned_cursor(d, [0, len(text)], sign), V.versioned_vector(d, sign)):
        assert form[0].dtype == np.uint64 and form[0].tolist() == survivors and form[1] == longest


def test_a_group_emits_the_majority_sign_in_order():
    rng = np.random.Generator(np.random.PCG64(2))
    for _ in range(200):
        signs = np.where(rng.random(int(rng.integers(1, 60))) < 0.5, 1, -1)
        kept, _ = V.queue_of(signs.tolist())
        cp, cn = int((signs == 1).sum()), int((signs == -1).sum())
        assert len(kept) == abs(cp - cn) and kept == sorted(kept)
        assert all(signs[t] == (1 if cp > cn else -1) for t in kept)


def _both(cols, spec, offs, sign):
    d = R.describe(cols, spec)
    a, b = V.versioned_cursor(d, offs, sign), V.versioned_vector(d, sign)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    return a


def test_two_versions_of_one_key_do_not_cancel():
    key = np.array([7, 7, 7, 7], dtype=np.int64)
    version = np.array([1, 2, 1, 2], dtype=np.uint32)
    sign = np.array([1, 1, -1, 1], dtype=np.int8)
    spec = [(0, False, 1), (1, False, 1)]
    rows, balance = _both([key, version], spec, [0, 2, 4], sign)
    assert rows.tolist() == [1, 3] and balance == 2          # (7, 1): + then - cancel; (7, 2): two + stay
    rows, balance = _both([key], [(0, False, 1)], [0, 2, 4], sign)
    assert rows.tolist() == [0, 3] and balance == 2          # without the version one group: + + - +


def test_max_balance_is_the_longest_queue_over_all_groups():
    key = np.array([1] * 6 + [2] * 5 + [3], dtype=np.int64)
    sign = np.array(signs_of("++-+++" + "----+" + "+"), dtype=np.int8)
    rows, balance = _both([key], [(0, False, 1)], [0, 12], sign)
    assert balance == 4 and rows.tolist() == [0, 3, 4, 5, 6, 7, 8, 11]
    assert _both([key[:0]], [(0, False, 1)], [0, 0], sign[:0]) [1] == 0


def test_cursor_and_vector_agree_on_merged_runs():
    rng = np.random.Generator(np.random.PCG64(3))
    spec = [(0, True, 1), (1, False, 1)]
    for lens in ([40, 0, 70, 25], [1], [200], [3, 3, 3, 3, 3]):
        offs = R.offsets_of(lens)
        n = int(offs[-1])
        cols = R.sort_runs([R.random_column(rng, np.float64, n, 4), R.random_column(rng, np.uint16, n, 2)], spec, offs)
        sign = np.where(rng.random(n) < 0.6, 1, -1).astype(np.int8)
        rows, _ = _both(cols, spec, offs, sign)
        assert len(rows) <= n


def test_a_bad_sign_names_the_lowest_row():
    from merge_fold_ref import BadValue
    key = np.zeros(5, dtype=np.int64)
    sign = np.array([1, -1, 0, 1, 2], dtype=np.int8)
    d = R.describe([key], [(0, False, 1)])
    for call in (lambda: V.versioned_cursor(d, [0, 5], sign), lambda: V.versioned_vector(d, sign)):
        with pytest.raises(BadValue) as e:
            call()
        assert e.value.row == 2
