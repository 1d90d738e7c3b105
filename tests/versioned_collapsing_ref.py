"""TEST INFRASTRUCTURE ONLY — the merge of VersionedCollapsingMergeTree (VersionedCollapsingAlgorithm) restated twice on the CPU, as
include/chgpu.h states it, with an unbounded queue.

versioned_cursor   the queue, row by row: rows arrive in merged order, a group ends where the row differs from its predecessor on a key
                   column (the version is the last of them); a row that meets an empty queue or one of its own sign is pushed, a row of
                   the other sign removes the queue's back row, and the group's end emits the queue front to back.
versioned_vector   the closed form, vectorised: B = the running sum of the signs inside a group; a row of sign s survives iff
                   s * B >= 1 and s * B_u >= s * B for every later row u of the group (a backward running minimum / maximum).

Both return (surviving concatenated row numbers as UInt64 in merged order, max_balance = the largest |B| = the longest the queue ever
was).  queue_of / closed_form_of do the same for ONE group given as its sign sequence and return positions.  A description is
merge_sorted_ref's; a sign outside +-1 raises merge_fold_ref.BadValue(row) for the lowest such row.
"""
from __future__ import annotations

import numpy as np

from merge_fold_ref import U64, _merged_groups, _rows, check_sign, merged_groups_vector


def queue_of(signs):
    """one group's signs in merged order -> (surviving positions, the longest the queue was)"""
    queue, longest = [], 0
    sign_in_queue = 0
    for t, s in enumerate(signs):
        if not queue:
            sign_in_queue = s
            queue.append(t)
        elif s == sign_in_queue:
            queue.append(t)
        else:
            queue.pop()
        longest = max(longest, len(queue))
    return queue, longest


def closed_form_of(signs):
    """the same from the balance: positions t with s_t * B_t >= 1 and s_t * B_u >= s_t * B_t for every u > t"""
    s = np.asarray(signs, dtype=np.int64)
    n = len(s)
    if n == 0:
        return [], 0
    b = np.cumsum(s)
    later_min = np.full(n, np.iinfo(np.int64).max)
    later_max = np.full(n, np.iinfo(np.int64).min)
    later_min[:-1] = np.minimum.accumulate(b[::-1])[::-1][1:]
    later_max[:-1] = np.maximum.accumulate(b[::-1])[::-1][1:]
    keep = np.where(s > 0, (b >= 1) & (later_min >= b), (b <= -1) & (later_max <= b))
    return np.flatnonzero(keep).tolist(), int(np.abs(b).max())


def versioned_cursor(description, run_offsets, sign):
    check_sign(sign)
    sg = np.asarray(sign).tolist()
    out, queue, longest = [], [], 0
    sign_in_queue = 0
    for row, head in _merged_groups(description, run_offsets):
        if head:
            out.extend(queue)
            queue = []
        if not queue:
            sign_in_queue = sg[row]
            queue.append(row)
        elif sg[row] == sign_in_queue:
            queue.append(row)
        else:
            queue.pop()
        longest = max(longest, len(queue))
    out.extend(queue)
    return _rows(out), longest


def versioned_vector(description, sign):
    check_sign(sign)
    perm, starts, ends = merged_groups_vector(description)
    n = len(perm)
    if n == 0:
        return _rows([]), 0
    s = np.asarray(sign)[perm].astype(np.int64)
    lens = ends - starts + 1
    total = np.cumsum(s)
    b = total - np.repeat(total[starts] - s[starts], lens)            # the balance: the sum since the group's head
    # backward running extrema inside a group: put every group on its own level (groups later in M higher for the minimum, lower for
    # the maximum; |b| <= n) so that one accumulate from the far end never takes a value from behind a head, then take the level off
    span = 2 * n + 2
    level = np.repeat(np.arange(len(starts), dtype=np.int64), lens) * span
    run_min = np.minimum.accumulate((b + level)[::-1])[::-1] - level    # min over u >= t of the group
    run_max = np.maximum.accumulate((b - level)[::-1])[::-1] + level
    tail = np.zeros(n, dtype=bool)
    tail[ends] = True
    later_min = np.where(tail, np.iinfo(np.int64).max, np.append(run_min[1:], 0))
    later_max = np.where(tail, np.iinfo(np.int64).min, np.append(run_max[1:], 0))
    keep = np.where(s > 0, (b >= 1) & (later_min >= b), (b <= -1) & (later_max <= b))
    return perm[keep].astype(U64), int(np.abs(b).max())
