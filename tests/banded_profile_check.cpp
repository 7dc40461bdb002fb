// tests/banded_profile_check.cpp -- TEST INFRASTRUCTURE: fsh::bandedBacktraceProfile (foldseek_amd/csrc/host/banded_backtrace.cpp) in a stand-alone
// program, compiled with -fsanitize=address,undefined (tests/test_profile_cases.py).  Reads rectangles from a binary file and prints one path per line
// ("-" where the function returns false).  File: i32 count, then per rectangle
//   i32 L, qStart, qLen, dbLen, score, gapOpen, gapExtend; int8 pAA[21 * L]; int8 p3Di[21 * L]; u8 tAA[dbLen]; u8 t3Di[dbLen]
// Every array is handed over in a heap block of exactly its size, so that a read past either end is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "hostlib.h"

template <class T>
static bool take(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: banded_profile_check <rectangles>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    for (int32_t r = 0; r < count; r++) {
        int32_t h[7];
        if (fread(h, 4, 7, f) != 7) { fprintf(stderr, "rectangle %d: short header\n", r); return 2; }
        const int L = h[0], qStart = h[1], qLen = h[2], dbLen = h[3], score = h[4], go = h[5], ge = h[6];
        if (L <= 0 || qStart < 0 || qLen <= 0 || qStart + qLen > L || dbLen <= 0) { fprintf(stderr, "rectangle %d: bad header\n", r); return 2; }
        std::vector<int8_t> pA, p3;
        std::vector<uint8_t> tA, t3;
        if (!take(f, pA, (size_t) 21 * L) || !take(f, p3, (size_t) 21 * L) || !take(f, tA, (size_t) dbLen) || !take(f, t3, (size_t) dbLen)) {
            fprintf(stderr, "rectangle %d: short body\n", r); return 2;
        }
        std::string path;
        const bool ok = fsh::bandedBacktraceProfile(pA.data(), p3.data(), L, qStart, qLen, tA.data(), t3.data(), dbLen, score, go, ge, path);
        printf("%s\n", ok ? path.c_str() : "-");
    }
    fclose(f);
    return 0;
}
