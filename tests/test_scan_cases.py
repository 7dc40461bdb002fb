"""What tests/scan_cases.py must contain for tests/test_sw_scan_gpu.py to mean something, asserted from tests/sw_model.py alone; a sample of the frozen
records re-run live; and the scan's stand-alone host code (foldseek_amd/csrc/fs_scan_order.h) built into a program of its own with AddressSanitizer and
UndefinedBehaviorSanitizer.  No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np

import scan_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_database_and_the_queries_are_what_the_issue_names():
    d = S.db()
    lens = d.lengths.tolist()
    assert d.n <= 400 and all(L in lens for L in S.FIXED_LENGTHS)
    assert sum(1 for k in d.kind if k == "random") == S.N_RANDOM and all(20 <= lens[i] <= 420 for i in range(d.n) if d.kind[i] == "random")
    assert sum(1 for k in d.kind if k == "piece") >= 20
    assert [len(q.q3) for q in S.queries()] == [1, 31, 32, 33, 200, 512, 513, 1024, 1025]
    assert lens != sorted(lens) and lens != sorted(lens, reverse=True)                    # ids are not in length order
    # targets on both sides of the planner's thresholds (64 lanes above 896 columns, 16 lanes up to FSGPU_SW3_MID = 512)
    assert any(L > 896 for L in lens) and any(512 < L <= 896 for L in lens) and any(0 < L <= 512 for L in lens)
    assert S.other_db().n == 40 != d.n
    assert S.wide_db().n > 2 * 4096


def test_every_cutoff_but_the_extremes_keeps_some_targets_and_drops_some():
    N = S.db().n
    for cfg in S.CONFIGS:
        for i, recs in enumerate(S.records(cfg)):
            assert len(recs) == N
            cuts = S.cutoffs(recs)
            assert cuts["zero"] == 0 and cuts["max"] == 32767 and cuts["occurs+1"] == cuts["occurs"] + 1
            assert (recs["score"] == cuts["occurs"]).any(), "a score that occurs"
            assert len(S.expected(recs, 0)[0]) == N                                       # the empty target included: it scores 0
            for kind in ("occurs", "occurs+1", "median"):
                ids, kept = S.expected(recs, cuts[kind])
                assert 0 < len(ids) < N, (S.config_name(cfg), S.Q_LENGTHS[i], kind, cuts[kind], len(ids))
                assert (kept["score"] >= cuts[kind]).all() and (np.diff(ids.astype(np.int64)) > 0).all()
            assert len(S.expected(recs, cuts["occurs"])[0]) > len(S.expected(recs, cuts["occurs+1"])[0])      # score + 1 drops the pairs AT the score
    empty = int(np.flatnonzero(S.db().lengths == 0)[0])
    assert all(tuple(int(r[empty][f]) for f in S.FIELDS) == (0, 0, 0, 1) for cfg in S.CONFIGS for r in S.records(cfg))


def test_some_survivors_run_in_the_reverse_of_their_id_order():
    """the scan runs the targets longest first and answers in id order: the host's sort is tested only if the two orders disagree among survivors"""
    order = S.longest_first().tolist()
    rank = {t: k for k, t in enumerate(order)}
    assert sorted(order) == list(range(S.db().n))
    for cfg in S.CONFIGS:
        found = False
        for recs in S.records(cfg):
            for kind in ("occurs", "median"):
                ids = S.expected(recs, S.cutoffs(recs)[kind])[0].tolist()
                found |= any(rank[a] > rank[b] for a, b in zip(ids, ids[1:]))
        assert found, S.config_name(cfg)
    recs = S.records(S.CONFIGS[0])[4]
    ids = S.expected(recs, S.cutoffs(recs)["occurs"])[0].tolist()
    assert len(ids) == 2                                                                  # named: the two best hits of the 200-residue query


def test_the_inflated_case_saturates_int16_and_the_int32_score_decides():
    recs = S.sat_records()
    two, one = recs["word"] == 2, recs["word"] == 1
    assert two.any() and one.any() and (recs["score"][two] > 32767).all() and (recs["score"][one] < 32767).all()
    # under the cutoff 32767 the survivors are exactly the re-run pairs: the int16 pass says 32767 for all of them, their int32 records are the answer
    ids, kept = S.expected(recs, 32767)
    assert ids.tolist() == np.flatnonzero(two).tolist() and (kept["word"] == 2).all()
    ids, kept = S.expected(recs, S.SAT_CUTOFFS[1])
    assert 0 < len(ids) < len(recs) and (kept["word"] == 1).any() and (kept["word"] == 2).any()
    assert len(S.sat_case()[2].q3) <= 512                                                 # a k_sw3 pair, not the profile path


def test_a_sample_of_the_frozen_records_live():
    rng = np.random.default_rng(5)
    N = S.db().n
    short = np.flatnonzero(S.db().lengths <= 120)
    for cfg in S.CONFIGS:
        frozen = S.records(cfg)
        for qi in (0, 3, 4, 6, 8):
            ids = np.concatenate([rng.choice(short, 5, replace=False), rng.choice(N, 2, replace=False)])
            live = S.live_records(cfg, qi, ids)
            assert [tuple(int(r[f]) for f in S.FIELDS) for r in live] == [tuple(int(frozen[qi][int(t)][f]) for f in S.FIELDS) for t in ids], (S.config_name(cfg), qi)
    ids = np.concatenate([rng.choice(short, 5, replace=False), np.flatnonzero(S.sat_records()["word"] == 2)[:2]])
    live = S.live_sat(ids)
    assert [tuple(int(r[f]) for f in S.FIELDS) for r in live] == [tuple(int(S.sat_records()[int(t)][f]) for f in S.FIELDS) for t in ids]
    w = S.wide_records()
    assert len(np.unique(w["score"])) > 10 and 0 < len(S.expected(w, S.cutoffs(w)["median"])[0]) < len(w)


def test_scan_order_and_sub_batches_under_the_sanitizers(tmp_path):
    """fs_scan_order.h in a stand-alone program with ASan + UBSan: its own checks, then the orders of this file's tables against the definition"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe, blob = str(tmp_path / "scan_order_check"), str(tmp_path / "tables.bin")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "foldseek_amd", "csrc"), os.path.join(ROOT, "tests", "scan_order_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and p.stderr == "", p.stderr[-2000:]
    tables = [S.db().lengths, S.other_db().lengths, S.wide_db().lengths, np.zeros(0, np.int32), np.zeros(5, np.int32), np.array([65535, 0, 65535], np.int32)]
    with open(blob, "wb") as f:
        f.write(struct.pack("<Q", len(tables)))
        for ln in tables:
            f.write(struct.pack("<Qi", len(ln), int(ln.max()) if len(ln) else 0) + np.ascontiguousarray(ln, np.int32).tobytes())
    p = subprocess.run([exe, blob], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and p.stderr == "", p.stderr[-2000:]
    lines = p.stdout.split("\n")
    for ln, line in zip(tables, lines):
        want = sorted(range(len(ln)), key=lambda i: (-int(ln[i]), i))
        assert [int(x) for x in line.split()] == want
    assert [int(x) for x in lines[0].split()] == S.longest_first().tolist()
