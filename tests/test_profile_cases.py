"""The seeded world of the profile-query alignment entries (tests/profile_cases.py, answers frozen in tests/golden/profile_align_v1) without a device:

1. the frozen files belong to the seed, and the world contains what it is there for (profile_cases.conditions, and the facts the generator measured on the
   model's functions, measured again);
2. the live model (tests/align_model.py's accept loop over tests/profile_model.py's ProfileWorld) reproduces the frozen answers of two queries for every
   parameter set;
3. the live model equals every line of the six frozen runs of the reference binary's structurealign on this world;
4. fsh::bandedBacktraceProfile, compiled into a stand-alone program with ASan + UBSan (tests/banded_profile_check.cpp), gives profile_model.banded_path's
   path for the world's longgap, row, col and slot rectangles, every rectangle whose band had to double, both gap costs, one-row / one-column rectangles and
   narrow rectangles whose path the `edge` slot quirk decides."""
import collections
import functools
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import align_model as A
import profile_cases as K
import profile_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = (K.NAMED_QUERY, 5)


@functools.lru_cache(maxsize=None)
def frozen():
    return K.Frozen()


@functools.lru_cache(maxsize=None)
def live():
    return K.Live()


# ---- 1. the frozen files and the world -------------------------------------------------------------------------------------------------------------------------
def test_world_is_what_the_issue_of_its_tests_needs():
    w = K.world()
    assert [len(pm.decode(e[0])[0]) for e in w["entries"]] == K.Q_LENGTHS + [K.SAT_LEN]
    assert all(12 <= len(x) <= 40 for x in w["lists"][:7]) and len(w["lists"][K.SAT_QUERY]) == 2
    kinds = collections.Counter(w["kinds"])
    assert set(kinds) == {"identity", "piece", "dup", "tail", "near", "random", "edge", "xhead", "xmid", "longgap", "row", "col", "slot"}
    for t, kind in zip(w["targets"], w["kinds"]):
        assert 1 <= len(t[0]) == len(t[1]) and (len(t[0]) <= 420 or kind == "identity")
    assert len(w["targets"][w["identity"][6]][0]) == 1025
    # the entries: scores at both extremes on every tenth position, the query letters are the master's, one query's consensus letters differ
    for q, (ea, e3) in enumerate(w["entries"][:7]):
        for e, master in ((ea, w["masters"][q][0]), (e3, w["masters"][q][1])):
            rec = np.frombuffer(e, np.uint8).reshape(-1, K.RECORD)
            s = rec[:, :20].view(np.int8)
            assert (rec[:, 20] == master).all() and ((rec[:, 21] != rec[:, 20]).any() == (q == 4))
            assert np.isin(s[::10], (-128, 127)).all() and ((s[::10] == 127).sum(axis=1) <= 1).all()
            on_master = s[np.arange(0, len(s), 10), master[::10]]
            assert (on_master[1:] == 127).all() and on_master[0] == (-128 if q == K.NAMED_QUERY else 127)          # the named query's position 0 is spoilt
            assert not np.isin(np.delete(s, np.arange(0, len(s), 10), axis=0), (-128, 127)).any()
    keys = w["keys"]
    assert len(set(keys.tolist())) == len(keys) and (np.diff(keys.astype(np.int64)) < 0).any()


def test_frozen_files_belong_to_the_seed_and_meet_the_conditions():
    F = frozen()
    assert json.load(open(os.path.join(K.GOLD, "MANIFEST.json")))["seed"] == K.SEED
    assert set(K.REFERENCE_SETS) <= set(F.names) and len(F.names) == 30
    K.conditions(F)
    accepted = {n: F.count(n).get("accepted", 0) + F.count(n).get("accepted as identity", 0) for n in F.names}
    assert accepted["default"] == accepted["no_bt"] >= 120 and accepted["e_all"] == sum(F.n), accepted
    for name in F.names:                                   # fwd records depend on the gap costs alone; looked-at pairs lie inside the selection
        assert (F.fwd(name) == F.fwd("default")).all() == (name != "gap8_2"), name
        assert all(F.looked(name)[q] <= F.selection(name, q) for q in range(len(F.n))), name


def test_the_generators_facts_measured_again():
    F = frozen()
    assert K.measure_facts(F) == F.facts
    widths = [x[2] for x in F.facts["doublings"]]
    assert max(len(x) for x in widths) >= 3, widths        # a band that had to double three times and more


# ---- 2. the live model on a sample -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", frozen().names)
def test_live_model_reproduces_the_frozen_answers(name):
    F = frozen()
    P = F.params(name)
    for q in SAMPLE + ((K.SAT_QUERY,) if name in ("default", "e_all") else ()):
        r = live().query(q, P)
        recs, cigars, hits = F.records(name, q)
        assert r.records.tobytes() == recs.tobytes() and r.cigars == cigars and r.hit_of_record == hits.tolist(), (name, q)
        assert (r.fwd.view(np.int32).reshape(-1, 4) == F.fwd(name, q)).all() and (r.rev.view(np.int32).reshape(-1, 4) == F.rev(name, q)).all(), (name, q)
        assert r.reversed == F.looked(name)[q] and r.outcomes == F.outcomes(name, q), (name, q)


# ---- 3. the reference binary's runs on this world -----------------------------------------------------------------------------------------------------------------
def _manifest():
    return json.load(open(os.path.join(K.GOLD, "MANIFEST.json")))


@pytest.mark.parametrize("run", sorted(_manifest()["runs"]))
def test_model_equals_every_line_of_the_reference_run(run):
    """the parameters are read back from the recorded parameter string; the reference treats no hit as the identity (two different databases)"""
    m = _manifest()["runs"][run]
    par = m["parameters"]
    get = lambda flag: par[par.index(flag) + 1]  # noqa: E731
    f32 = lambda x: float(np.float32(float(x)))  # noqa: E731
    go, ge = int(get("--gap-open").split(",")[0].split(":")[1]), int(get("--gap-extend").split(",")[0].split(":")[1])
    P = K.params(evalThr=float(get("-e")), covThr=f32(get("-c")), covMode=int(get("--cov-mode")), seqIdThr=f32(get("--min-seq-id")),
                 seqIdMode=int(get("--seq-id-mode")), alnLenThr=int(get("--min-aln-len")), maxAccept=int(get("--max-accept")),
                 maxRejected=int(get("--max-rejected")), gapOpen=go, gapExtend=ge, addBacktrace=int(get("-a")))
    assert P == frozen().params(m["set"]), "the parameter string names the set exactly"
    want = K.read_db(os.path.join(K.GOLD, run))
    assert sorted(want) == list(range(len(K.world()["entries"])))
    n = 0
    for q, r in enumerate(live().run(P, identity=-1)):
        text = "".join(A.line(rec, cig) + "\n" for rec, cig in zip(r.records, r.cigars))
        assert text == want[q].decode(), (run, q)
        n += len(r.records)
    assert n == m["lines"] > 0


# ---- 4. bandedBacktraceProfile under the sanitizers ------------------------------------------------------------------------------------------------------------------
def _rectangles():
    """[(what, L, qStart, qLen, dbLen, score, go, ge, pAA int8 [21, L], p3Di int8 [21, L], tAA, t3Di)]"""
    F, w = frozen(), K.world()
    doubled = {(q, k) for q, k, _ in F.facts["doublings"]}
    out = []
    for name in ("e_all", "gap8_2"):
        P = F.params(name)
        for q in range(len(F.n)):
            aF, sF = pm.decode(w["entries"][q][0])[2], pm.decode(w["entries"][q][1])[2]
            recs, cigars, hits = F.records(name, q)
            for rec, cig, k in zip(recs, cigars, hits):
                t = int(w["lists"][q][k])
                if not (w["kinds"][t] in ("longgap", "row", "col", "slot") or (q, int(k)) in doubled):
                    continue
                qs, qe, ds, de = (int(rec[f]) for f in ("qStartPos", "qEndPos", "dbStartPos", "dbEndPos"))
                ta, t3 = w["targets"][t]
                out.append(((name, q, int(k), w["kinds"][t], cig), aF.shape[1], qs, qe - qs + 1, de - ds + 1, int(F.fwd(name, q)[k][0]), P["gapOpen"], P["gapExtend"],
                            aF, sF, ta[ds:de + 1], t3[ds:de + 1]))
    # one-row and one-column rectangles of 1, 2, 5 and 40 cells, rows 20 .. of the 80-position query against the start of its identity target; the score
    # asked for is the best single cell, which any band reaches
    aF, sF = pm.decode(w["entries"][2][0])[2], pm.decode(w["entries"][2][1])[2]
    ta, t3 = w["targets"][w["identity"][2]]
    for n in (1, 2, 5, 40):
        for q_len, db_len in ((1, n), (n, 1)):
            m = (sF.astype(np.int64)[:, 21:21 + q_len][t3[21:21 + db_len].astype(np.int64)].T + aF.astype(np.int64)[:, 21:21 + q_len][ta[21:21 + db_len].astype(np.int64)].T)
            assert m.max() > 0
            out.append((("one line", q_len, db_len), aF.shape[1], 21, q_len, db_len, int(m.max()), 10, 1, aF, sF, ta[21:21 + db_len], t3[21:21 + db_len]))
    # narrow rectangles (2 .. 5 columns, more rows than columns) cut out of the same query and target, asked for the score of their last cell: the path runs
    # down the last column, whose H and E of the row above the `edge` slot clears.  Kept: those whose path the model's quirk decides.
    decided = 0
    for q_len in range(3, 12):
        for db_len in range(2, 6):
            for qs in range(0, 60, 3):
                for ds in range(0, 60, 7):
                    m = (sF.astype(np.int64)[:, qs:qs + q_len][t3[ds:ds + db_len].astype(np.int64)].T + aF.astype(np.int64)[:, qs:qs + q_len][ta[ds:ds + db_len].astype(np.int64)].T)
                    if q_len <= db_len or m[0, 0] <= 0 or m[-1, -1] <= 0:
                        continue
                    score = int(m[-1, -1])
                    if pm.banded_path(m, q_len, db_len, score) != pm.banded_path(m, q_len, db_len, score, edge_slot=False):
                        decided += 1
                        out.append((("edge slot", q_len, db_len, qs, ds), aF.shape[1], qs, q_len, db_len, score, 10, 1, aF, sF, ta[ds:ds + db_len], t3[ds:ds + db_len]))
    assert decided >= 10, decided
    return out


def test_banded_backtrace_profile_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe, blob = str(tmp_path / "banded_profile_check"), str(tmp_path / "rectangles.bin")
    host = os.path.join(ROOT, "foldseek_amd", "csrc", "host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                           "-I", host, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "banded_profile_check.cpp"),
                           os.path.join(host, "banded_backtrace.cpp"), "-o", exe])
    rects = _rectangles()
    kinds = collections.Counter(r[0][3] if len(r[0]) == 5 and r[0][0] != "edge slot" else r[0][0] for r in rects)
    assert kinds["longgap"] >= 20 and kinds["row"] >= 7 and kinds["col"] >= 2 and kinds["slot"] >= 10 and kinds["one line"] == 8 and kinds["edge slot"] >= 10, kinds
    with open(blob, "wb") as f:
        f.write(struct.pack("<i", len(rects)))
        for _, L, qs, ql, dl, score, go, ge, aF, sF, ta, t3 in rects:
            f.write(struct.pack("<7i", L, qs, ql, dl, score, go, ge))
            for a in (np.ascontiguousarray(aF, np.int8), np.ascontiguousarray(sF, np.int8), np.ascontiguousarray(ta, np.uint8), np.ascontiguousarray(t3, np.uint8)):
                f.write(a.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, blob], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and p.stderr == "", p.stderr[-2000:]
    lines = p.stdout.split("\n")[:-1]
    assert len(lines) == len(rects)
    for (what, L, qs, ql, dl, score, go, ge, aF, sF, ta, t3), got in zip(rects, lines):
        m = sF.astype(np.int64)[:, qs:qs + ql][t3.astype(np.int64)].T + aF.astype(np.int64)[:, qs:qs + ql][ta.astype(np.int64)].T
        want = pm.banded_path(m, ql, dl, score, go, ge)
        assert got == (want if want is not None else "-"), (what, got[:80], (want or "-")[:80])
        if what[0] in ("e_all", "gap8_2"):
            assert K.compress(got) == what[4], what
