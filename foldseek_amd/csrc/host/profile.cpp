// profile.cpp -- entries of a profile database (DBTYPE_HMM_PROFILE, what result2profile writes for the later rounds of an iterative search) as the
// aligners read them: Sequence::mapProfile (M/src/commons/Sequence.cpp:301-340) and the profile branch of SmithWaterman::ssw_init
// (M/src/alignment/StripedSmithWaterman.cpp:1364-1425).  GAP_POS_SCORING is not defined in the reference build: the two gap bytes of a record are not read.
#include "hostlib.h"

#include <cstdio>

extern "C" {

int fshost_profile_decode(const char *entry, size_t len, uint8_t *codes, uint8_t *consensus, int8_t *profile, int8_t *profileRev, char *err, size_t errCap) {
    auto refuse = [&](int rc, const char *what, size_t at, int value) {
        if (err && errCap) snprintf(err, errCap, what, at, value);
        return rc;
    };
    if (!entry && len) return refuse(FSHOST_PROFILE_E_ARG, "profile entry: null pointer with %zu bytes (%d)", len, 0);
    if (len % FSHOST_PROFILE_RECORD != 0)
        return refuse(FSHOST_PROFILE_E_LENGTH, "profile entry: %zu bytes are not a multiple of the record size %d", len, FSHOST_PROFILE_RECORD);
    const size_t L = len / FSHOST_PROFILE_RECORD;
    if (L > (size_t) FSGPU_MAX_SEQ_LEN) return refuse(FSHOST_PROFILE_E_LENGTH, "profile entry: %zu positions, more than %d", L, FSGPU_MAX_SEQ_LEN);
    const unsigned char *rec = (const unsigned char *) entry;
    for (size_t i = 0; i < L; i++) {
        const unsigned char *r = rec + i * FSHOST_PROFILE_RECORD;
        if (r[20] >= FSGPU_ALPHABET) return refuse(FSHOST_PROFILE_E_LETTER, "profile entry: query letter at position %zu is %d, above 20", i, (int) r[20]);
        if (r[21] >= FSGPU_ALPHABET) return refuse(FSHOST_PROFILE_E_LETTER, "profile entry: consensus letter at position %zu is %d, above 20", i, (int) r[21]);
    }
    for (size_t i = 0; i < L; i++) {
        const unsigned char *r = rec + i * FSHOST_PROFILE_RECORD;
        if (codes) codes[i] = r[20];
        if (consensus) consensus[i] = r[21];
        for (int a = 0; a < FSGPU_ALPHABET; a++) {
            // profile_for_alignment = (short) score / 4: C division, towards zero; the X row is set to 0 whatever the entry holds
            const int8_t v = a < 20 ? (int8_t) ((int) (signed char) r[a] / 4) : (int8_t) 0;
            if (profile) profile[(size_t) a * L + i] = v;
            if (profileRev) profileRev[(size_t) a * L + (L - 1 - i)] = v;
        }
    }
    return (int) L;
}

int fshost_profile_bias(const int8_t *profile, int L) {
    if (!profile || L <= 0) return 0;
    int lo = 0;
    for (size_t k = 0; k < (size_t) 20 * L; k++) if (profile[k] < lo) lo = profile[k];
    return -lo;
}

} // extern "C"
