// scan_order_check.cpp -- the host-only pieces of fsgpu_sw_scan_c (foldseek_amd/csrc/fs_scan_order.h) as a stand-alone program, for a build with
// -fsanitize=address,undefined (tests/test_scan_cases.py).  Reads a file of length tables: u64 count, then per table u64 n, i32 maxLen, i32 lengths[n];
// prints the order of every table on one line.  With no argument it runs its own checks of the sub-batch sizes and of the order on seeded tables.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fs_scan_order.h"

static bool isOrder(const std::vector<int32_t> &len, const std::vector<uint32_t> &order) {
    if (order.size() != len.size()) return false;
    std::vector<char> seen(len.size(), 0);
    for (size_t k = 0; k < order.size(); k++) {
        if (order[k] >= len.size() || seen[order[k]]) return false;
        seen[order[k]] = 1;
        if (k > 0) {
            const int32_t a = len[order[k - 1]], b = len[order[k]];
            if (a < b || (a == b && order[k - 1] > order[k])) return false;
        }
    }
    return true;
}

static int selfCheck() {
    uint64_t state = 88172645463325252ull;
    auto rnd = [&] { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
    for (int t = 0; t < 200; t++) {
        const size_t n = (size_t) (rnd() % 300);
        const int maxLen = t % 5 == 0 ? 0 : (int) (rnd() % (t % 7 == 0 ? 65536 : 40));
        std::vector<int32_t> len(n);
        for (int32_t &l : len) l = (int32_t) (rnd() % ((uint64_t) maxLen + 1));
        std::vector<uint32_t> order(3, 7u);                      // stale content of another size goes
        fsScanOrder(len.data(), n, maxLen, order);
        if (!isOrder(len, order)) { fprintf(stderr, "table %d: not the longest-first order\n", t); return 1; }
    }
    struct { uint64_t n, budget; int want; } cases[] = {
        {0, 1, 65535}, {1, 0, 1}, {1, 19, 1}, {1, 40, 2}, {96, 20 * 96, 1}, {96, 20 * 96 * 9 + 5, 9}, {1000000, 1ull << 30, 53},
        {1, ~0ull, 65535}, {0x7fffffffull, ~0ull, 1}, {0x40000000ull, ~0ull, 1}, {0x3fffffffull, ~0ull, 2}, {100000, 1ull << 40, 21474},
    };
    for (const auto &c : cases) {
        const int got = fsScanQueriesPerBatch(c.n, c.budget);
        if (got != c.want) { fprintf(stderr, "fsScanQueriesPerBatch(%llu, %llu) = %d, expected %d\n", (unsigned long long) c.n, (unsigned long long) c.budget, got, c.want); return 1; }
        if (c.n > 0 && (uint64_t) got * c.n > 0x7fffffffull && got > 1) { fprintf(stderr, "more than 2^31 - 1 pairs in a sub-batch\n"); return 1; }
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return selfCheck();
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t count = 0;
    if (fread(&count, 8, 1, f) != 1) return 2;
    for (uint64_t t = 0; t < count; t++) {
        uint64_t n = 0;
        int32_t maxLen = 0;
        if (fread(&n, 8, 1, f) != 1 || fread(&maxLen, 4, 1, f) != 1) return 2;
        std::vector<int32_t> len(n);
        if (n && fread(len.data(), 4, n, f) != n) return 2;
        std::vector<uint32_t> order;
        fsScanOrder(len.data(), n, maxLen, order);
        for (uint32_t id : order) printf("%u ", id);
        printf("\n");
    }
    fclose(f);
    return 0;
}
