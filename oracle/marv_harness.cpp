// marv_harness.cpp -- TEST ONLY.  `class Marv` (include/marv.h, foldseek_amd/csrc/host/marv_shim.cpp) behind a C boundary, so that tests/marv_lib.py
// reaches it through ctypes without the reference binary around it.  Every function forwards one call and nothing else: no clamp, no sort, no default.
// Marv::scan writes into the caller's Result records directly.  Nothing here is linked into the product.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "marv.h"

extern "C" {

size_t marvh_sizeof_result() { return sizeof(Marv::Result); }

void *marvh_create(size_t dbEntries, int alphabetSize, int maxSeqLength, size_t maxSeqs, int alignmentType) {
    return new Marv(dbEntries, alphabetSize, maxSeqLength, maxSeqs, (Marv::AlignmentType) alignmentType);
}

void marvh_destroy(void *m) { delete static_cast<Marv *>(m); }

void *marvh_load_db(void *m, char *data, size_t *offset, int32_t *length, size_t dbByteSize) {
    return static_cast<Marv *>(m)->loadDb(data, offset, length, dbByteSize);
}

void *marvh_load_db_other(void *m, char *data, size_t dbByteSize, void *otherdb) { return static_cast<Marv *>(m)->loadDb(data, dbByteSize, otherdb); }

void marvh_set_db(void *m, void *dbhandle) { static_cast<Marv *>(m)->setDb(dbhandle); }

void marvh_set_db_with_allocation(void *m, void *dbhandle, const char *allocationinfo) {
    static_cast<Marv *>(m)->setDbWithAllocation(dbhandle, std::string(allocationinfo));
}

// the handle's length; its first min(length, capacity) bytes go to out
size_t marvh_db_memory_handle(void *m, char *out, size_t capacity) {
    const std::string h = static_cast<Marv *>(m)->getDbMemoryHandle();
    if (out && capacity && !h.empty()) memcpy(out, h.data(), h.size() < capacity ? h.size() : capacity);
    return h.size();
}

size_t marvh_scan(void *m, const char *sequence, size_t sequenceLength, int8_t *pssm, void *results, int *numOverflows, double *seconds, double *gcups) {
    const Marv::Stats st = static_cast<Marv *>(m)->scan(sequence, sequenceLength, pssm, static_cast<Marv::Result *>(results));
    *numOverflows = st.numOverflows; *seconds = st.seconds; *gcups = st.gcups;
    return st.results;
}

} // extern "C"
