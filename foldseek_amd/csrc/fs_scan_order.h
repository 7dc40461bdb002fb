// fs_scan_order.h -- private, host only, no HIP: the order fsgpu_sw_scan_c runs the targets of a database in, and the sub-batching of its queries.
// Stand-alone so that tests/scan_order_check.cpp can run it under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

// All target ids, longest first, equal lengths by ascending id (the key of swSortLongestFirst): neighbours share a wave of k_sw3, so they should
// be of similar length.  Lengths lie in 0 .. maxLen (the database table was checked at load): one counting sort, O(n + maxLen).
inline void fsScanOrder(const int32_t *lengths, uint64_t n, int maxLen, std::vector<uint32_t> &order) {
    std::vector<uint64_t> first((size_t) maxLen + 2, 0);
    for (uint64_t i = 0; i < n; i++) first[(size_t) (maxLen - lengths[i]) + 1]++;
    for (size_t l = 1; l < first.size(); l++) first[l] += first[l - 1];
    order.resize(n);
    for (uint64_t i = 0; i < n; i++) order[first[(size_t) (maxLen - lengths[i])]++] = (uint32_t) i;
}

// Queries per sub-batch: ids and records of a query take 20 bytes per target on the device; a sub-batch stays under `budget` bytes, under 2^31 pairs
// (k_sw3 reads a workgroup's first pair as an int) and under 65535 queries, and holds at least one query.
inline int fsScanQueriesPerBatch(uint64_t n, uint64_t budget) {
    if (n == 0) return 65535;
    uint64_t k = budget / (20 * n);
    const uint64_t byPairs = 0x7fffffffull / n;
    if (k > byPairs) k = byPairs;
    if (k > 65535) k = 65535;
    return k < 1 ? 1 : (int) k;
}
