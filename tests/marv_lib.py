"""ctypes bindings for oracle/libmarvh.so: `class Marv` (include/marv.h + foldseek_amd/csrc/host/marv_shim.cpp) behind the forwarding C functions of
oracle/marv_harness.cpp.  Test infrastructure only.  The library is built on first use when it is missing (make -C oracle libmarvh.so), as
oracle_lib.load_oracle does for libfso.so.

Marv.scan hands the shim a record array of capacity max_seqs followed by CANARIES records it must never touch; a Marv::die() ends the process, so
the refusals run in a child (refusal_child below is what the child executes)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
LIB_PATH = os.path.join(ORACLE_DIR, "libmarvh.so")

RESULT_DT = np.dtype([("id", np.uint32), ("score", np.int32), ("qEndPos", np.int32), ("dbEndPos", np.int32)])       # Marv::Result
GAPLESS, SMITH_WATERMAN, GAPLESS_SMITH_WATERMAN = 0, 1, 2                                                          # Marv::AlignmentType
CANARIES = 8
CANARY = (0xDEADBEEF, -559038737, 0x5A5A5A5A, -0x5A5A5A5B)

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", ORACLE_DIR, "libmarvh.so"])
    L = C.CDLL(LIB_PATH)
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
    sig = {
        "marvh_sizeof_result": (sz, []),
        "marvh_create": (vp, [sz, i32, i32, sz, i32]),
        "marvh_destroy": (None, [vp]),
        "marvh_load_db": (vp, [vp, vp, vp, vp, sz]),
        "marvh_load_db_other": (vp, [vp, vp, sz, vp]),
        "marvh_set_db": (None, [vp, vp]),
        "marvh_set_db_with_allocation": (None, [vp, vp, C.c_char_p]),
        "marvh_db_memory_handle": (sz, [vp, vp, sz]),
        "marvh_scan": (sz, [vp, vp, sz, vp, vp, C.POINTER(i32), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    assert L.marvh_sizeof_result() == RESULT_DT.itemsize
    _lib = L
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Marv:
    """one Marv object.  FSGPU_MARV_SHARDS is read by the constructor: set it (monkeypatch.setenv) before this one runs."""

    def __init__(self, db_entries, max_seqs, alphabet=21, max_seq_length=0, alignment_type=GAPLESS):
        self.max_seqs, self.db_entries = int(max_seqs), int(db_entries)
        self._keep = []
        self.h = load().marvh_create(self.db_entries, alphabet, max_seq_length, self.max_seqs, alignment_type)

    def load_db(self, data, offsets, lengths):
        """data: uint8 buffer (its size is the dbByteSize passed on), offsets [n + 1], lengths [n]; the shim borrows data and lengths, kept alive here"""
        d = np.ascontiguousarray(data, np.uint8)
        off = np.ascontiguousarray(offsets, np.uint64)
        ln = np.ascontiguousarray(lengths, np.int32)
        assert len(off) == self.db_entries + 1 and len(ln) == self.db_entries
        self._keep.append((d, off, ln))
        return load().marvh_load_db(self.h, _ptr(d), _ptr(off), _ptr(ln), d.size)

    def load_db_other(self, other, nbytes=0):
        return load().marvh_load_db_other(self.h, None, nbytes, other)

    def set_db(self, handle):
        load().marvh_set_db(self.h, handle)

    def set_db_with_allocation(self, handle, info=b""):
        load().marvh_set_db_with_allocation(self.h, handle, info)

    def db_memory_handle(self):
        buf = np.zeros(64, np.uint8)
        n = load().marvh_db_memory_handle(self.h, _ptr(buf), buf.size)
        return bytes(buf[:min(n, buf.size)]), n

    def scan(self, sequence, pssm):
        """-> (the records scan reported, all max_seqs + CANARIES records of the buffer, (results, numOverflows, seconds, gcups))"""
        seq = np.ascontiguousarray(sequence, np.uint8)
        p = None if pssm is None else np.ascontiguousarray(pssm, np.int8)
        buf = np.zeros(self.max_seqs + CANARIES, RESULT_DT)
        buf[:] = CANARY
        nov, sec, gc = C.c_int(-7), C.c_double(-7.0), C.c_double(-7.0)
        n = load().marvh_scan(self.h, _ptr(seq), len(seq), _ptr(p), _ptr(buf), C.byref(nov), C.byref(sec), C.byref(gc))
        return buf[:min(n, len(buf))].copy(), buf, (int(n), nov.value, sec.value, gc.value)

    def close(self):
        if self.h:
            load().marvh_destroy(self.h)
            self.h = None


def untouched(records):
    want = np.zeros(len(records), RESULT_DT)
    want[:] = CANARY
    return records.tobytes() == want.tobytes()


# ---- the refusals: what the child process runs ------------------------------------------------------------------------------------------------------
def _tiny_db():
    """three targets (5, 6 and 9 residues) in the padded layout"""
    lens = np.array([5, 6, 9], np.int32)
    off = np.zeros(4, np.uint64)
    off[1:] = np.cumsum((lens.astype(np.int64) + 3) // 4 * 4)
    data = np.full(int(off[-1]), 20, np.uint8)
    for k, n in enumerate(lens):
        data[int(off[k]):int(off[k]) + n] = (np.arange(n) * 3 + k) % 20
    return data, off, lens


def _unknown_profile(L):
    """a profile no built-in matrix gives: matrix entry 3 on letter (i mod 20), -3 elsewhere, zero X row, no composition bias"""
    p = np.full((21, L), -3, np.int8)
    p[np.arange(L) % 20, np.arange(L)] = 3
    p[20] = 0
    return p


REFUSALS = {
    # name: (shards, what stderr must hold)
    "alignment_type_1": (1, "only AlignmentType::GAPLESS"),
    "alignment_type_2": (1, "only AlignmentType::GAPLESS"),
    "alphabet_20": (1, "alphabet size 20 is not supported"),
    "scan_before_setdb": (1, "scan before setDb"),
    "null_handle": (1, "setDb: null database handle"),
    "residue_code_21": (1, "query residue code out of range"),
    "x_row_beyond_8": (1, "X row is not a plain composition bias"),
    "column_at_query_x": (1, "does not come from a substitution matrix with a zero X row"),
    "entry_outside_buffer_2_shards": (2, "an entry lies outside the data buffer"),
    "entry_outside_buffer_1_shard": (1, "an entry lies outside the data buffer"),
    "max_seqs_0": (1, "maxSeqs == 0"),
    "blosum_like_other_scale": (1, "a matrix with a non-zero X row"),
}


def refusal_child(name, blosum_profile=None):
    """runs in a fresh process: one Marv, the one refused call.  Reaching the end is the failure (exit status 3)."""
    data, off, lens = _tiny_db()
    seq = np.arange(6, dtype=np.uint8)
    if name.startswith("alignment_type"):
        Marv(3, 10, alignment_type={"1": SMITH_WATERMAN, "2": GAPLESS_SMITH_WATERMAN}[name[-1]])
    elif name == "alphabet_20":
        Marv(3, 10, alphabet=20)
    elif name == "scan_before_setdb":
        m = Marv(3, 10)
        m.load_db(data, off, lens)
        m.scan(seq, _unknown_profile(6))
    elif name == "null_handle":
        Marv(3, 10).set_db(None)
    elif name.startswith("entry_outside_buffer"):
        m = Marv(3, 10)
        bad = off.copy()
        bad[2] = data.size - 4                        # nine residues from here run past the buffer's end
        m.set_db(m.load_db(data, bad, lens))
    else:
        m = Marv(3, 0 if name == "max_seqs_0" else 10)
        m.set_db(m.load_db(data, off, lens))
        p = _unknown_profile(6)
        if name == "residue_code_21":
            seq[3] = 21
        elif name == "x_row_beyond_8":
            p[:, 2] += 9
        elif name == "column_at_query_x":
            seq[4] = 20
        elif name == "blosum_like_other_scale":
            p = np.frombuffer(bytes.fromhex(blosum_profile), np.int8).reshape(21, -1)
            seq = np.arange(p.shape[1], dtype=np.uint8) % 20
        m.scan(seq, p)
    sys.stderr.write("the call returned\n")
    sys.exit(3)
