// fs_db_table.h -- the offsets / lengths table of a target database against its byte buffer (fsgpu_db_check_table): plain C++, no device
// call, no HIP header, so that a host-only program can be built from it alone.
#ifndef FS_DB_TABLE_H
#define FS_DB_TABLE_H
#include <algorithm>
#include <cstdint>
#include <vector>

#ifndef FSGPU_MAX_SEQ_LEN
#define FSGPU_MAX_SEQ_LEN 65535
#endif

// -1 when every entry lies inside the buffer, no two entries share a byte and offsets[n] <= bytes; else the index of the first bad entry
// (n for offsets[n]).  An entry is tested as offset > bytes || length > bytes - offset: the sum of an offset and a length is formed only
// for entries that have passed, so an offset near 2^64 cannot wrap into the buffer.  Without the arrays (offsets NULL, or lengths NULL with n > 0)
// nothing is read and the answer is 0: no table is a table whose first entry is bad.
static inline int64_t fsDbCheckTable(const uint64_t *offsets, const int32_t *lengths, uint64_t n, uint64_t bytes) {
    if (!offsets || (!lengths && n)) return 0;
    auto outside = [&](uint64_t t) {
        return lengths[t] < 0 || lengths[t] > FSGPU_MAX_SEQ_LEN || offsets[t] > bytes || (uint64_t) lengths[t] > bytes - offsets[t];
    };
    // one pass: the first entry outside the buffer, and whether every entry with residues begins at or behind the end of all before it --
    // the order of every padded database, in which no two entries can share a byte
    uint64_t bad = n, end = 0;
    bool ordered = true;
    for (uint64_t t = 0; t < n; t++) {
        if (outside(t)) { if (bad == n) bad = t; continue; }
        if (lengths[t] == 0) continue;
        if (offsets[t] < end) ordered = false;
        end = std::max(end, offsets[t] + (uint64_t) lengths[t]);
    }
    // Any other order is sorted by address.  The entry reported for shared bytes is the one of lowest index that BEGINS inside another (of
    // two that begin at one address, the later in the table).  Entries without residues hold no byte, entries outside the buffer are
    // reported as such: neither takes part.
    uint64_t shared = n;
    if (!ordered) {
        std::vector<uint64_t> idx;
        idx.reserve(n);
        for (uint64_t t = 0; t < n; t++) if (!outside(t) && lengths[t] > 0) idx.push_back(t);
        std::sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) { return offsets[a] != offsets[b] ? offsets[a] < offsets[b] : a < b; });
        end = 0;
        for (uint64_t t : idx) {
            if (offsets[t] < end) shared = std::min(shared, t);
            end = std::max(end, offsets[t] + (uint64_t) lengths[t]);
        }
    }
    const uint64_t first = std::min(bad, shared);
    if (first < n) return (int64_t) first;
    return offsets[n] <= bytes ? -1 : (int64_t) n;
}
#endif
