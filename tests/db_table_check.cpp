// Stand-alone host program around fsDbCheckTable (foldseek_amd/csrc/fs_db_table.h) for tests/test_db_table_host.py, which builds it with
// -fsanitize=address,undefined and runs it over the tables of tests/db_cases.py: the function reads n + 1 offsets and n lengths and nothing else,
// whatever the offsets say, and no arithmetic of it overflows.  The arrays are copied into heap blocks of their exact size, so that one element
// too many is a report.  Input (a file): u64 tables, then per table u64 n, u64 bytes, (n + 1) u64 offsets, n i32 lengths.  Output: one answer per line.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fs_db_table.h"

static bool get(FILE *f, void *p, size_t size) { return size == 0 || fread(p, size, 1, f) == 1; }

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s tables.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint64_t tables = 0;
    if (!get(f, &tables, 8)) return 2;
    for (uint64_t k = 0; k < tables; k++) {
        uint64_t n = 0, bytes = 0;
        if (!get(f, &n, 8) || !get(f, &bytes, 8)) return 2;
        uint64_t *offsets = (uint64_t *) malloc((n + 1) * sizeof(uint64_t));
        int32_t *lengths = (int32_t *) malloc(n ? n * sizeof(int32_t) : 1);
        if (!offsets || !lengths || !get(f, offsets, (n + 1) * 8) || !get(f, lengths, n * 4)) return 2;
        printf("%lld\n", (long long) fsDbCheckTable(offsets, lengths, n, bytes));
        free(offsets);
        free(lengths);
    }
    fclose(f);
    return 0;
}
