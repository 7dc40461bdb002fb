"""fsgpu_db_check_table (include/fsgpu.h), the host-only check every table passes before fsgpu_db_load / fsgpu_db_adopt_device allocate or launch anything:
every shape of tests/db_cases.py is a good table, every refusal is refused at the index the definition gives (the FIRST bad entry when several are bad),
and the tables the project's other producers make still pass.  The same function, built into a stand-alone program with AddressSanitizer and
UndefinedBehaviorSanitizer, answers the same over the same tables, the offsets near 2^64 included.  The frozen model answers of `longest`
(tests/golden/db_v1) are re-computed live for every ninth case.  No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import db_cases as D
import marv_cases as MC
from foldseek_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCOP = os.path.join(ROOT, "tests", "golden", "scop_v1")


def _table(db):
    return np.ascontiguousarray(db.offsets, np.uint64), np.ascontiguousarray(db.lengths, np.int32), int(np.asarray(db.data3di).size)


def _scop_table(index, data):
    """the table modules.cpp makes of a padded database on disk: offsets as the index has them, residues = index length - 2, end = size of the data file"""
    rows = [tuple(int(x) for x in ln.split()) for ln in open(os.path.join(SCOP, index))]
    size = os.path.getsize(os.path.join(SCOP, data))
    return np.array([r[1] for r in rows] + [size], np.uint64), np.array([r[2] - 2 for r in rows], np.int32), size


def _random_tables():
    """small random tables, good and bad: the function against its definition"""
    rng = np.random.default_rng(20261101)
    out = []
    for k in range(300):
        n, nbytes = int(rng.integers(1, 9)), int(rng.integers(0, 60))
        ln = rng.integers(0, 12, n).astype(np.int32)
        off = rng.integers(0, max(1, nbytes + 3), n + 1).astype(np.uint64)
        if k % 3 == 0:                                                      # mostly good ones: back to back, in a random order of entries
            order = rng.permutation(n)
            at = 0
            for t in order:
                off[t] = at
                at += int(ln[t]) + int(rng.integers(0, 3))
            nbytes, off[n] = at, at - int(rng.integers(0, 2)) if at else 0
        if k % 7 == 0:
            ln[int(rng.integers(0, n))] = int(rng.choice([-1, D.MAX_LEN + 1, -2 ** 31]))
        if k % 11 == 0:
            off[int(rng.integers(0, n + 1))] = np.uint64(2 ** 64 - int(rng.integers(1, 20)))
        out.append((off, ln, nbytes))
    return out


def _all_tables():
    """[(name, offsets, lengths, bytes, expected answer or None)]"""
    out = [(name, *_table(D.shape(name).db), -1) for name in D.NAMES]
    out += [(r.name, *_table(r.db), r.index if r.index is not None else -1) for r in D.refusals()]      # a table without entries is good: the entries refuse n == 0 themselves
    out += [(f"random{k}", *t, None) for k, t in enumerate(_random_tables())]
    return out


@pytest.mark.parametrize("name", D.NAMES)
def test_every_shape_is_a_good_table(name):
    off, ln, nbytes = _table(D.shape(name).db)
    assert api.db_check_table(off, ln, nbytes) == -1
    assert D.check_table_model(off, ln, nbytes) == -1


def test_the_shapes_are_what_their_names_say():
    """the layouts the other tests rely on, asserted from the tables themselves"""
    odd, gaps, desc = (D.shape(f"bytes_{w}").db for w in ("odd", "gaps", "descending"))
    assert int(odd.offsets[0]) == 1 and (np.diff(odd.offsets[:-1]) == odd.lengths[:-1]).all() and (odd.offsets[:-1] % 4 != 0).sum() >= 6
    g = gaps.offsets[1:-1] - (gaps.offsets[:-2] + gaps.lengths[:-1])
    assert g.min() >= 1 and g.max() > 3 and g.max() <= 70
    inside = np.zeros(gaps.data3di.size, bool)
    for i in range(gaps.n):
        inside[int(gaps.offsets[i]):int(gaps.offsets[i]) + int(gaps.lengths[i])] = True
    assert (gaps.data3di[~inside] < 20).all() and (~inside).sum() > 100          # the gaps hold residues that would score
    assert (np.diff(desc.offsets[:-1]) < 0).all()
    for a, b in ((odd, gaps), (odd, desc)):                                       # the same residues in all three
        assert all(D.entry(a, i).tobytes() == D.entry(b, i).tobytes() for i in range(a.n))
    assert D.shape("all_empty").db.data3di.size == 0 and D.shape("all_empty").db.n == 9
    assert sorted(D.shape("empty_stripe").db.lengths)[8] == 0                   # by length, the first stripe of eight holds no residue
    lens = {w: D.shape(f"order_{w}").db.lengths for w in ("ascending", "equal", "descending", "strict", "ties")}
    assert (np.diff(lens["ascending"]) >= 0).all() and (np.diff(lens["descending"]) <= 0).all() and (np.diff(lens["strict"]) < 0).all()
    assert len(set(lens["equal"].tolist())) == 1 and sorted(lens["ties"].tolist()) == sorted(lens["ascending"].tolist())
    assert not (np.diff(lens["ties"]) >= 0).all() and not (np.diff(lens["ties"]) <= 0).all()
    c = D.shape("codes").db
    assert set(range(21)) | set(range(32, 53)) <= set(D.entry(c, 0).tolist()) and set(D.entry(c, 0, "aa").tolist()) == set(D.entry(c, 0).tolist())
    assert (D.entry(c, 1) >= 32).all() and (D.entry(c, 1, "aa") >= 32).all() and 52 in D.entry(c, 2).tolist()
    assert set(D.entry(c, 3).tolist()) == set(range(21, 32)) | set(range(53, 256)) == set(D.entry(c, 3, "aa").tolist())
    lo = D.shape("longest")
    assert sorted(lo.db.lengths.tolist())[-6:] == [1000, 32767, 32768, 32769, 65534, 65535]
    assert int(lo.db.lengths.max()) == D.MAX_LEN == api.FSGPU_MAX_SEQ_LEN
    assert int(D.sw_want("longest", 300, 0, 1)["dbEnd"].max()) == 65534 and 32770 in D.sw_want("longest", 40, 0, 1)["dbEnd"].tolist()


@pytest.mark.parametrize("r", D.refusals(), ids=lambda r: r.name)
def test_refusals_name_the_first_bad_entry(r):
    off, ln, nbytes = _table(r.db)
    want = -1 if r.index is None else r.index
    assert api.db_check_table(off, ln, nbytes) == want
    assert D.check_table_model(off, ln, nbytes) == want


def test_no_table_at_all_is_a_bad_first_entry():
    """NULL arrays (include/fsgpu.h): 0, nothing is read; a table without entries is good while its end lies inside the buffer"""
    L = api.lib()
    one = np.zeros(2, np.uint64)
    assert L.fsgpu_db_check_table(None, None, 0, 10) == 0 and L.fsgpu_db_check_table(None, None, 3, 10) == 0
    assert L.fsgpu_db_check_table(one.ctypes.data, None, 1, 10) == 0
    assert L.fsgpu_db_check_table(one.ctypes.data, None, 0, 10) == -1
    assert api.db_check_table(np.array([11], np.uint64), np.zeros(0, np.int32), 10) == 0


def test_the_function_equals_its_definition_on_random_tables():
    got = [(api.db_check_table(*t), D.check_table_model(*t)) for t in _random_tables()]
    assert all(a == b for a, b in got), [(k, a, b) for k, (a, b) in enumerate(got) if a != b][:5]
    assert sum(a == -1 for a, _ in got) >= 40 and sum(a >= 0 for a, _ in got) >= 100


def test_the_tables_of_the_other_producers_pass():
    """synth.make_db / make_db_fast, the databases of marv_cases (padded, and cut behind the last residue as the Marv shim receives them) and the two padded
    databases the reference wrote (tests/golden/scop_v1: db_pad_ss in ascending memory order, db_pad linked to the source's data in the source's order)"""
    for db in (synth.make_db(300, seed=5), synth.make_db_fast(2000, seed=6), MC.world()["db"], MC.other_db(), MC.small_db(2)):
        assert api.db_check_table(*_table(db)) == -1
    db = MC.world()["db"]
    data, off = MC.unpadded(db)
    assert api.db_check_table(off, db.lengths, data.size) == -1
    ss, aa = _scop_table("db_pad_ss.index", "db_pad_ss"), _scop_table("db_pad.index", "db")
    assert api.db_check_table(*ss) == -1 and api.db_check_table(*aa) == -1
    assert (np.diff(ss[0][:-1].astype(np.int64)) > 0).all() and not (np.diff(aa[0][:-1].astype(np.int64)) > 0).all()      # the second is NOT in memory order
    assert ((aa[0][:-1] % 4) != 0).any()


def test_sanitized_standalone_program_agrees(tmp_path):
    """the function alone in a host program of its own under ASan + UBSan: plain C++ built from fs_db_table.h, no HIP header, no device call -- it never
    touches a GPU, wherever the suite runs -- and no Python process involved in the run.  The runtimes are linked statically."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe, blob = str(tmp_path / "db_table_check"), str(tmp_path / "tables.bin")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "foldseek_amd", "csrc"), os.path.join(ROOT, "tests", "db_table_check.cpp"), "-o", exe])
    tables = _all_tables()
    with open(blob, "wb") as f:
        f.write(struct.pack("<Q", len(tables)))
        for _, off, ln, nbytes, _ in tables:
            f.write(struct.pack("<QQ", len(ln), nbytes) + np.ascontiguousarray(off, np.uint64).tobytes() + np.ascontiguousarray(ln, np.int32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, blob], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and p.stderr == "", p.stderr[-2000:]
    got = [int(x) for x in p.stdout.split()]
    assert len(got) == len(tables)
    for (name, off, ln, nbytes, want), g in zip(tables, got):
        assert g == api.db_check_table(off, ln, nbytes), name
        assert want is None or g == want, (name, g, want)


def test_frozen_answers_equal_the_live_models_on_every_ninth_case():
    """tests/golden/db_v1/answers.npz against the models, now: every ninth (key, row) of the frozen arrays"""
    keys = D.frozen_keys()
    assert set(k for k, _ in keys) == set(D.frozen())
    cases = [(k, row) for k, _ in keys for row in range(len(D.frozen()[k]))]
    picked = cases[::9]
    assert len(picked) >= 20
    sh = D.shape("longest")
    m3, mA = D.K.matrices()
    by_key = {}
    for k, row in picked:
        by_key.setdefault(k, []).append(row)
    for k, rows in by_key.items():
        parts = k.split("/")
        if parts[1] == "scan":
            pssm, cap = D.scan_profile(int(parts[2]))
            ids = np.array(rows)
            sub = synth.PaddedDB(D.scan_bytes(sh.db.data3di), None, np.append(sh.db.offsets[ids], 0), sh.db.lengths[ids])
            assert (D.gm.scores(pssm, cap, sub) == D.frozen()[k][ids]).all(), k
        elif parts[1] == "sw":
            L, rev, aa = int(parts[2]), int(parts[3]), int(parts[4])
            ids = D.sw_ids(sh, L)[np.array(rows)]
            live = D.K.live(m3, mA if aa else None, D.query(L), bool(rev), [D.aligner_target(sh.db, int(i)) for i in ids], D.GO, D.GE)
            assert [[int(r[f]) for f in D.SW_FIELDS] for r in live] == D.frozen()[k][np.array(rows)].tolist(), k
        else:
            l3, lA = (np.asarray(m, np.int64).tolist() for m in (m3, mA))
            targets = [D.aligner_target(sh.db, i)[::-1] for i in range(sh.db.n)]
            pairs = D.diag_pairs(sh)
            for row in rows:
                r = D.dm.rescore_pair(D.diag_queries(sh), targets, pairs[row], l3, lA)
                assert [r[f] for f in D.dm.FIELDS] == D.frozen()[k][row].tolist(), (k, row, pairs[row])
