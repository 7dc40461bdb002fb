"""TM-score without a GPU: the independent model (tests/tm_model.py) against what the REFERENCE BINARY printed and decided (tests/golden/tm_v1, generator
tests/golden/make_tm_golden.py), and the host pieces of this repository's TM path against the model.

  * every alntmscore / qtmscore / ttmscore / rmsd field of the reference's convertalis on the 144 pairs of the 12 example structures and on the crafted
    database, byte for byte: from the LIVE model for all of them (once per session), and from the model's frozen raw answers, which must equal the live ones;
  * a spread sample of the frozen corpus and edge answers against the live model;
  * every --tmscore-threshold decision (two thresholds, three modes) and every --sort-by-structure-bits score, LDDT column and order of the reference's
    structurealign, from ca_v1's unfiltered records;
  * fshost_tm_params / fshost_tm_finish / fshost_tm_normalization == the model; the new symbols and struct layouts; the --exact-tmscore refusal.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import lddt_cases as K
import lddt_model as M
import tm_cases as TC
import tm_model as T
from foldseek_amd import api

BIN = os.path.join(K.ROOT, "foldseek_amd", "bin", "fsgpu-modules")


def _rows(name):
    return [l.rstrip("\n").split("\t") for l in open(os.path.join(TC.GOLD, name))]


def test_frozen_model_answers_reproduce_every_reference_field():
    _, tasks = TC.fixture_tasks()
    raw = TC.frozen_raw("fixture")
    rows = _rows("conv_tm.m8") + _rows("conv_tm_crafted.m8")
    assert len(rows) == 144 + len(TC.crafted_records()) and 3 * len(rows) == len(tasks) == len(raw)
    for r, row in enumerate(rows):
        assert TC.text_fields(raw[3 * r:3 * r + 3], [t[5] for t in tasks[3 * r:3 * r + 3]]) == row[3:7], row
    crafted = rows[144:]
    assert any(r[3] == "INF" for r in crafted)                         # one aligned column: normLen 0 in alntmscore
    assert any(r[3:6] == ["0.000E+00"] * 3 for r in crafted)           # every pair beyond score_d8
    assert sum(r[6] == "0.000E+00" for r in crafted) >= 3              # self-alignments


def test_live_model_reproduces_every_reference_field_and_the_frozen_answers():
    """the LIVE model on all 144 pairs and every crafted record, three normalisations each (computed once per session: tm_cases.live_fixture_raw)"""
    _, tasks = TC.fixture_tasks()
    raw, live = TC.frozen_raw("fixture"), TC.live_fixture_raw()
    rows = _rows("conv_tm.m8") + _rows("conv_tm_crafted.m8")
    assert len(live) == len(raw) == 3 * len(rows)
    for r, row in enumerate(rows):
        assert TC.text_fields(live[3 * r:3 * r + 3], [t[5] for t in tasks[3 * r:3 * r + 3]]) == row[3:7], row
        assert live[3 * r:3 * r + 3].tobytes() == raw[3 * r:3 * r + 3].tobytes(), row


@pytest.mark.parametrize("which", ["corpus", "edge"])
def test_live_model_reproduces_a_sample_of_the_frozen_task_lists(which):
    queries, targets, tasks = TC.corpus() if which == "corpus" else TC.edge()
    raw = TC.frozen_raw(which)
    assert len(raw) == len(tasks)
    only = set(range(0, len(tasks), 41)) if which == "corpus" else set(range(2, len(tasks), 7))
    live = TC.model_raw(queries, targets, tasks, only)
    for k in sorted(only):
        assert live[k].tobytes() == raw[k].tobytes(), (which, k)
    if which == "corpus":
        counts = sorted(set(int(v) for v in raw[:, 0]))
        assert counts[:9] == list(range(1, 10)) and {15, 17, 33, 41, 65, 81, 129, 161} <= set(counts) and max(counts) >= 290


def test_crafted_records_take_the_branches_they_were_made_for():
    """re-derived with the live model: no relief below four pairs, the relief loop on distant residues, the classical Kabsch() on a single pair"""
    C_ = TC.crafted_coords()
    seen = {}
    for q, t, qs, ts, cig in TC.crafted_records():
        n = M.expand(cig).count("M")
        if n > 7:
            continue
        stats = {}
        xtm, ytm = T.pairs(C_[q], C_[t], qs, ts, M.expand(cig))
        T.tm_raw(xtm, ytm, C_[q].shape[1], stats)
        seen[(q, t, cig)] = stats
    assert all(s.get("relief", 0) == 0 for (q, t, cig), s in seen.items() if M.expand(cig).count("M") < 4)
    assert seen[(2, 3, "1M")].get("fallback", 0) > 0
    assert seen[(2, 4, "4M")].get("relief", 0) > 10
    assert T.frag_lengths(161) == [161, 80, 40, 20, 10, 4] and T.frag_lengths(3) == [3] and T.frag_lengths(5) == [5, 4]
    assert T.frag_starts(161, 80) == [0, 40, 80, 81] and T.frag_starts(41, 20) == [0, 21] and T.frag_starts(80, 40) == [0, 40]


def _unfiltered():
    """ca_v1's aln_l0: per record (query, fields, TM-score per mode, avgLddtScore)"""
    _, tasks = TC.fixture_tasks()
    raw = TC.live_fixture_raw()
    out = []
    for r, ((q, f), cols) in enumerate(zip(TC.result_records(K.read_db, "aln_l0"), K.model_columns("db", "aln_l0"))):
        tms = []
        for m in range(3):
            n, s1, s2, _ = TC.as_floats(raw[3 * r + m])
            tms.append(T.tm_finish(n, s1, s2, tasks[3 * r + m][5]))
        out.append((q, f, tms, M.average(cols)[0]))
    return out


@pytest.mark.parametrize("name,thr,mode", [("aln_sb0_t07_m0", 0.7, 0), ("aln_sb0_t07_m1", 0.7, 1), ("aln_sb0_t07_m2", 0.7, 2), ("aln_sb0_t08_m0", 0.8, 0)])
def test_model_reproduces_reference_threshold_decisions(name, thr, mode):
    """tmscore < tmScoreThr compares a double with a float widened to double (structurealign.cpp:393); the kept records are unchanged"""
    thr = float(np.float32(thr))
    mine = [(q, f) for q, f, tms, _ in _unfiltered() if not tms[mode] < thr]
    ref = TC.result_records(TC.read_db, name)
    assert mine == ref and 0 < len(ref) < 144 and len(ref) == TC.MANIFEST["runs"][name]["lines"]


@pytest.mark.parametrize("name,tm_thr,lddt_thr", [("aln_sb1", 0.0, 0.0), ("aln_sb1_l05_t07", 0.7, 0.5)])
def test_model_reproduces_reference_structure_bits(name, tm_thr, lddt_thr):
    """score = (int) (score * sqrt(avgLddt * tm)) (dbcov = avgLddt is not part of a result line), order: score descending, dbLen ascending, dbKey ascending"""
    tm_thr, lddt_thr = float(np.float32(tm_thr)), float(np.float32(lddt_thr))
    per_q = {}
    for q, f, tms, avg in _unfiltered():
        if tms[0] < tm_thr or avg < lddt_thr:
            continue
        g = list(f)
        g[1] = str(int(int(f[1]) * math.sqrt(avg * tms[0])))
        per_q.setdefault(q, []).append(g)
    mine = []
    for q in sorted(per_q):
        mine += [(q, g) for g in sorted(per_q[q], key=lambda g: (-int(g[1]), int(g[9]), int(g[0])))]
    ref = TC.result_records(TC.read_db, name)
    assert len(ref) == TC.MANIFEST["runs"][name]["lines"]
    assert mine == ref


def test_host_scalars_equal_the_model():
    for nl in list(range(0, 400)) + [1000, 5000, 65535]:
        with np.errstate(all="ignore"):
            _, sd8, d0, d0s = T.search_params(nl)
            std = T.standard_params(nl)
        assert api.tm_params(nl).tobytes() == np.array([sd8, std, d0, d0s], np.float32).tobytes(), nl
    rng = np.random.default_rng(1)
    for _ in range(2000):
        n, nl = int(rng.integers(0, 400)), int(rng.integers(0, 500))
        s1, s2 = np.float32(rng.random()), np.float32(rng.random() * 1.2)
        a, b = T.tm_finish(n, s1, s2, nl), api.tm_finish(n, s1, s2, nl)
        assert a == b or (a != a and b != b), (n, nl, s1, s2, a, b)
    assert [api.tm_normalization(m, 10, 20, 30) for m in range(5)] == [10, 20, 30, 0, 0]
    assert [T.normalization(m, 10, 20, 30) for m in range(3)] == [10, 20, 30]
    assert T.sstr(api.tm_finish(1, 1.0, 1.0, 0)) == "INF"


def test_api_mirrors_the_new_symbols_and_structs():
    assert "fsgpu_tm_batch" in api.exported_symbols()
    names = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    for sym in ("fsgpu_tm_batch", "fshost_tm_finish", "fshost_tm_params", "fshost_tm_normalization"):
        assert f" T {sym}\n" in names, sym
        assert hasattr(api.lib(), sym)
    assert C.sizeof(api.TmTask) == 56
    assert [f[0] for f in api.TmTask._fields_] == ["query", "tLen", "tOff", "qStart", "dbStart", "btOff", "btLen", "scoreD8", "d0Std", "d0", "d0Search", "reserved"]
    assert api.TmTask.btOff.offset == 24 and api.TmTask.scoreD8.offset == 36 and api.TmTask.d0Search.offset == 48
    assert hasattr(api.Context, "tm_batch")
    assert C.sizeof(api.Params) == 80                              # fshost_params is unchanged


def test_exact_tmscore_is_refused_before_a_device_is_opened(tmp_path):
    """the device computes the approximate TM-score only: --exact-tmscore 1 is refused whenever a TM-score would be computed (a threshold, structure bits,
    a TM column) and stays without effect otherwise; a non-zero threshold is still refused by structurerescorediagonal"""
    pos = [os.path.join(K.GOLD, "db"), os.path.join(K.GOLD, "db"), os.path.join(K.GOLD, "pref"), str(tmp_path / "out")]
    run = lambda args: subprocess.run([BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)  # noqa: E731
    r = run(["structurealign"] + pos + ["--tmscore-threshold", "0.5", "--exact-tmscore", "1", "--sort-by-structure-bits", "0"])
    assert r.returncode == 1 and "structurealign: --exact-tmscore 1 is not implemented on the device path (supported: 0)" in r.stderr
    r = run(["structurealign"] + pos + ["--exact-tmscore", "1"])                    # structure bits are the default, and both _ca exist
    assert r.returncode == 1 and "--exact-tmscore 1 is not implemented" in r.stderr
    r = run(["structurealign"] + pos + ["--tmscore-threshold-mode", "3"])
    assert r.returncode == 1 and "Error in argument --tmscore-threshold-mode" in r.stderr
    r = run(["structurerescorediagonal"] + pos + ["--tmscore-threshold", "0.5"])
    assert r.returncode == 1 and "structurerescorediagonal: --tmscore-threshold 0.5 is not implemented on the device path (supported: 0|0.0|0.000)" in r.stderr
    r = run(["convertalis", pos[0], pos[1], os.path.join(K.GOLD, "aln_l0"), str(tmp_path / "o.m8"), "--format-output", "query,ttmscore", "--exact-tmscore", "1"])
    assert r.returncode == 1 and "convertalis: --exact-tmscore 1 is not implemented" in r.stderr
    assert not os.path.exists(tmp_path / "out.index") and not os.path.exists(tmp_path / "o.m8")
