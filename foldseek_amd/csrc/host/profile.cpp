// profile.cpp -- entries of a profile database (DBTYPE_HMM_PROFILE, what result2profile writes for the later rounds of an iterative search) as the
// aligners read them: Sequence::mapProfile (M/src/commons/Sequence.cpp:301-340) and the profile branch of SmithWaterman::ssw_init
// (M/src/alignment/StripedSmithWaterman.cpp:1364-1425).  GAP_POS_SCORING is not defined in the reference build: the two gap bytes of a record are not read.
#include "hostlib.h"

#include <cstdio>
#include <cstring>

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

// the same, and the 20 score bytes of every position as they stand in the entry: what the k-mer generator reads (Sequence.cpp:308-310, `short` without the division)
int fshost_profile_decode_raw(const char *entry, size_t len, uint8_t *codes, uint8_t *consensus, int8_t *profile, int8_t *profileRev, int8_t *scores, char *err, size_t errCap) {
    const int L = fshost_profile_decode(entry, len, codes, consensus, profile, profileRev, err, errCap);
    if (L <= 0 || !scores) return L;
    for (int i = 0; i < L; i++) memcpy(scores + (size_t) i * 20, entry + (size_t) i * FSHOST_PROFILE_RECORD, 20);
    return L;
}

// Prefiltering::getKmerThreshold, profile branch (Prefiltering.cpp:1050-1079; Foldseek's externalThreshold has no profile row): the products are taken
// in double, the difference is stored in a float and cut to an int, as there
int fshost_kmer_threshold_profile(float sensitivity, int kmerSize, int contextPseudoCounts) {
    float base; double step;
    if (contextPseudoCounts) {
        if (kmerSize == 5) { base = 97.75f; step = 8.75; } else if (kmerSize == 6) { base = 132.75f; step = 8.75; } else if (kmerSize == 7) { base = 158.75f; step = 9.75; } else return -1;
    } else {
        if (kmerSize == 5) { base = 108.8f; step = 4.7; } else if (kmerSize == 6) { base = 134.35f; step = 6.15; } else if (kmerSize == 7) { base = 149.15f; step = 6.85; } else return -1;
    }
    const float best = (float) ((double) base - (double) sensitivity * step);
    return (int) best;
}

// what fsgpu_kmer_search_profile takes of one 3Di profile entry: letters, raw score rows, the ungapped profile [L][21] (UngappedAlignment::createProfile,
// profile branch: the alignment profile position-major, X column 0, no bias correction) and the threshold of every window, max(kmerThrBase, 0)
int fshost_kmer_query_prepare_profile(const char *entry, size_t len, int kmerThrBase, int kmerSize, int spaced, uint8_t *codes, int8_t *scores, int8_t *profile,
                                      int32_t *kmerThr, char *err, size_t errCap) {
    if (kmerSize != 6) { if (err && errCap) snprintf(err, errCap, "profile k-mer query: only k = 6 is implemented (k = %d)", kmerSize); return FSHOST_PROFILE_E_ARG; }
    const int L = fshost_profile_decode(entry, len, codes, nullptr, nullptr, nullptr, err, errCap);
    if (L < 0) return L;
    for (int i = 0; i < L; i++) {
        const signed char *r = (const signed char *) entry + (size_t) i * FSHOST_PROFILE_RECORD;
        if (scores) memcpy(scores + (size_t) i * 20, r, 20);
        if (profile) { for (int a = 0; a < 20; a++) profile[(size_t) i * 21 + a] = (int8_t) ((int) r[a] / 4); profile[(size_t) i * 21 + 20] = 0; }
    }
    if (kmerThr) *kmerThr = kmerThrBase > 0 ? kmerThrBase : 0;
    const int windows = L - (spaced ? 10 : 6) + 1;
    return windows > 0 ? windows : 0;
}

int fshost_profile_bias(const int8_t *profile, int L) {
    if (!profile || L <= 0) return 0;
    int lo = 0;
    for (size_t k = 0; k < (size_t) 20 * L; k++) if (profile[k] < lo) lo = profile[k];
    return -lo;
}

} // extern "C"
