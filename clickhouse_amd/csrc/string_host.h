// string_host.h — the parts of the ColumnString operators (string_kernels.hip, string_sort_kernels.hip) that need no device: how each
// call's one pool allocation is divided into its sub-buffers.  Every layout is ONE list, a function over a cursor: run with base 0 it
// gives the bytes to ask of the pool, run with the allocation's address it gives the pointers, so the two cannot disagree.  Every
// sub-buffer starts on a 256-byte boundary and takes a multiple of 256 bytes (the pool's size classes are multiples of 1024, so
// rounding the last one up never changes a call's class).  Plain C++, so that tests/string_layout_driver.cpp runs them under a sanitizer.
#pragma once

#include <cstddef>
#include <cstdint>

struct StrCursor
{
    uintptr_t base; // 0: sizing only, every pointer comes out NULL
    size_t used = 0;
    template <class T>
    void take(T *& p, uint64_t count)
    {
        p = base ? (T *)(base + used) : nullptr;
        used += ((size_t)count * sizeof(T) + 255) / 256 * 256;
    }
};

struct StrDictLayout // chgpu_string_dictionary_encode: n rows, cap cells
{
    uint64_t * hash, * rep_row;     // [n]
    uint32_t * is_first;            // [n]
    uint64_t * prefix;              // [n]
    uint64_t * tags;                // [cap]
    unsigned long long * first_row; // [cap]
    uint32_t * fail;
    uint64_t * total;
    char * scan_tmp;
};

static inline size_t str_dict_lay(uintptr_t base, uint64_t n, uint64_t cap, size_t scan_tmp_bytes, StrDictLayout * l)
{
    StrCursor c{base};
    c.take(l->hash, n), c.take(l->rep_row, n), c.take(l->is_first, n), c.take(l->prefix, n), c.take(l->tags, cap), c.take(l->first_row, cap);
    c.take(l->fail, 1), c.take(l->total, 1), c.take(l->scan_tmp, scan_tmp_bytes);
    return c.used;
}

// What a layout pass (str_layout_values, string_column.h) brings back in one piece.  The sizes kernel raises the flags.
struct StrLayoutWords
{
    uint64_t bytes;     // the scan's total: chars of the result
    uint64_t bad_index; // an index at or behind the source's rows
    uint64_t too_long;  // a value of 4 GiB or more
    uint64_t rows;      // filter: the kept-row scan's total
};

struct StrValuesLayout // chgpu_string_index: n values of the result; chgpu_string_filter (`kept`): n rows of the source
{
    uint32_t * flag = nullptr;    // [n] filter: the row is kept
    uint64_t * row_pos = nullptr; // [n] filter: its row in the result
    uint32_t * sizes;             // [n] bytes of every value, its zero among them (filter: 0 for a row that is not kept)
    uint64_t * pos;               // [n] where it starts in the result's chars
    StrLayoutWords * words;
    char * scan_tmp;
};

static inline size_t str_values_lay(uintptr_t base, uint64_t n, bool kept, size_t scan_tmp_bytes, StrValuesLayout * l)
{
    StrCursor c{base};
    if (kept)
        c.take(l->flag, n), c.take(l->row_pos, n);
    c.take(l->sizes, n), c.take(l->pos, n), c.take(l->words, 1), c.take(l->scan_tmp, scan_tmp_bytes);
    return c.used;
}

struct SsSegs // the string sort's segments, device arrays of one entry per segment (a kernel argument)
{
    uint64_t * start; // first position of the segment in the output permutation
    uint64_t * first; // index of its first row in the active arrays
    uint64_t * depth; // words every row of the segment is known to share (and to have)
    uint64_t * adv;   // further words all of its rows share (k_ss_lcp); SS_NONE: no pair of rows looked
    uint64_t * head;  // index of its head row in the previous round's sorted arrays
};

static inline size_t ss_segs_lay(uintptr_t base, uint64_t cap, SsSegs * t)
{
    StrCursor c{base};
    c.take(t->start, cap), c.take(t->first, cap), c.take(t->depth, cap), c.take(t->adv, cap), c.take(t->head, cap);
    return c.used;
}

struct SsRoundLayout // flags and scans of one round of the string sort over m active rows
{
    uint32_t * new_head, * active; // [m]
    uint64_t * seg_no, * slot;     // [m]
    uint64_t * totals;             // [0] segments, [1] active rows of the next round
    char * scan_tmp;
};

static inline size_t ss_round_lay(uintptr_t base, uint64_t m, size_t scan_tmp_bytes, SsRoundLayout * l)
{
    StrCursor c{base};
    c.take(l->new_head, m), c.take(l->active, m), c.take(l->seg_no, m), c.take(l->slot, m), c.take(l->totals, 2), c.take(l->scan_tmp, scan_tmp_bytes);
    return c.used;
}
