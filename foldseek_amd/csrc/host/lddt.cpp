// lddt.cpp -- host half of the LDDT path: the C-alpha entry decoder (Coordinate16::read, F/src/commons/Coordinate16.h:15-57) and the ordered
// average over the per-column values the device returns (LDDTScoreResult, F/src/commons/LDDT.h:102-119).  The all-pairs part is k_lddt.hpp.
#include "hostlib.h"

#include <cmath>
#include <cstring>

extern "C" {

int fshost_ca_decode(const char *entry, size_t entryLen, int L, float *out) {
    if (!entry || !out || L <= 0) return -1;
    const size_t n = (size_t) L;
    if (entryLen >= 3 * n * sizeof(float)) { memcpy(out, entry, 3 * n * sizeof(float)); return 0; }
    if (entryLen < 3 * (sizeof(int32_t) + (n - 1) * sizeof(int16_t))) return -1;
    const char *data = entry;
    for (int axis = 0; axis < 3; axis++) {
        int32_t start, diffSum = 0;
        memcpy(&start, data, sizeof(int32_t));
        data += sizeof(int32_t);
        float *o = out + (size_t) axis * n;
        o[0] = start / 1000.0f;
        for (size_t i = 1; i < n; i++) {
            int16_t d;
            memcpy(&d, data, sizeof(int16_t));
            data += sizeof(int16_t);
            diffSum += d;
            o[i] = (start + diffSum) / 1000.0f;
        }
    }
    return 0;
}

double fshost_lddt_average(const float *cols, int alignLength, int *scoreLength) {
    float sum = 0.0f;
    int len = alignLength;
    for (int i = 0; i < alignLength; i++) {
        if (std::isnan(cols[i])) len--;
        else sum += cols[i];
    }
    if (scoreLength) *scoreLength = len;
    // volatile: the division happens at run time on this machine's unit (0 / 0 is the x86 default NaN, sign bit set), not in the compiler
    volatile float num = sum, den = (float) len;
    return (double) (num / den);
}

} // extern "C"
