// nsk_alloc.h -- the books of a graph handle's device arrays: what dev_alloc hands out and the bytes it counts for;
// nsk_graph_info.device_bytes is the running total.  Plain C++, no HIP calls (tests/test_alloc_ledger_cpu.py).
#pragma once

#include <cassert>
#include <cstddef>
#include <cstdint>
#include <vector>

struct NskLedger {
    struct Entry { void *ptr, *raw; int64_t bytes; };      // ptr: handed out; raw: the allocation (they differ under NSK_ALLOC_ALIGN)
    std::vector<Entry> entries;                            // oldest first (nsk_graph_destroy frees what is left)
    int64_t total = 0;
    void add(void *ptr, void *raw, size_t bytes) { entries.push_back({ptr, raw, (int64_t)bytes}); total += (int64_t)bytes; }
    // takes the entry of a pointer handed out off the books and returns its allocation (nullptr: null, or not on them)
    void *remove(void *ptr) {
        for (size_t i = entries.size(); ptr && i-- > 0;)
            if (entries[i].ptr == ptr) {
                const Entry e = entries[i];
                total -= e.bytes;
                entries.erase(entries.begin() + (std::ptrdiff_t)i);
                return e.raw;
            }
        return nullptr;
    }
    void *pop() { const Entry e = entries.back(); entries.pop_back(); total -= e.bytes; return e.raw; }     // the newest entry
};

// Scoped rollback of a set-up that allocates several arrays: destroyed without commit(), it takes every entry beyond the
// `mark` entries the ledger had at its construction off the books, newest first, and hands the allocation to free_raw.
// (Free an OLDER array only after commit(): inside the scope it would shift the mark by one.)
struct NskRollback {
    NskLedger &ledger;
    void (*free_raw)(void *);
    size_t mark;
    NskRollback(NskLedger &l, void (*f)(void *)) : ledger(l), free_raw(f), mark(l.entries.size()) {}
    NskRollback(const NskRollback &) = delete;
    ~NskRollback() { assert(mark == (size_t)-1 || ledger.entries.size() >= mark); while (ledger.entries.size() > mark) free_raw(ledger.pop()); }
    void commit() { mark = (size_t)-1; }
};
