"""Superposition and exact TM-score without a GPU: the independent model (tests/tm_exact_model.py) against what the REFERENCE BINARY wrote
(tests/golden/tm_exact_v1, generator tests/golden/make_tm_exact_golden.py), and the host pieces of this repository against the model.

  * the model's frozen raw answers reproduce every text field of the reference's aln2tmscore result DBs and of its convertalis
    (alntmscore, qtmscore, ttmscore, rmsd, u, t) with --exact-tmscore 0 and 1, byte for byte, for the 144 records of ca_v1 and the crafted records;
  * the LIVE model equals the frozen answers on every crafted record and on one normalisation of each of the 144 records, in both modes, and on a
    spread sample of the corpus (whose tie statistics it reproduces as well);
  * the crafted records take their branches in exact mode too;
  * fshost_tm_exact_params / fshost_tm_exact_finish == the model; symbols and struct layouts; the argument errors of the aln2tmscore module.
"""
import ctypes as C
import functools
import multiprocessing
import os
import subprocess

import numpy as np
import pytest

import lddt_cases as K
import tm_cases as TC
import tm_exact_cases as XC
import tm_exact_model as X
import tm_model as T
from foldseek_amd import api

BIN = os.path.join(K.ROOT, "foldseek_amd", "bin", "fsgpu-modules")
N_CA = 144


def _rows(name):
    return [l.rstrip("\n").split("\t") for l in open(os.path.join(XC.GOLD, name))]


@pytest.mark.parametrize("is_exact", [False, True])
def test_frozen_model_answers_reproduce_every_convertalis_field(is_exact):
    _, tasks = XC.fixture_tasks()
    raw = XC.frozen_raw("fixture", is_exact)
    x = int(is_exact)
    rows = _rows(f"conv_x{x}.m8") + _rows(f"conv_x{x}_crafted.m8")
    assert len(rows) == N_CA + len(TC.crafted_records()) and 3 * len(rows) == len(tasks) == len(raw)
    for r, row in enumerate(rows):
        assert X.convertalis_fields(raw[3 * r:3 * r + 3], [t[5] for t in tasks[3 * r:3 * r + 3]], is_exact) == row[2:8], row
    crafted = rows[N_CA:]
    assert any(r[2] == "INF" for r in crafted)                         # one aligned column: normLen 0 in alntmscore, in both modes
    assert sum(r[5] == "0.000E+00" for r in crafted) >= 3              # self-alignments


def test_frozen_model_answers_reproduce_the_aln2tmscore_result_dbs():
    """(a): the reference's aln2tmscore writes the approximate score of normalisation 0 and the superposition that reached it"""
    _, tasks = XC.fixture_tasks()
    raw = XC.frozen_raw("fixture", False)
    r = 0
    for name, recs in (("a2t_ca", K.records("aln_l0")), ("a2t_crafted", TC.crafted_records())):
        got = XC.read_gold_db(name)
        want = {}
        for q, t, _, _, _ in recs:
            want.setdefault(q, []).append(X.aln2tmscore_line(t, raw[3 * r], tasks[3 * r][5], False))
            r += 1
        assert sorted(got) == sorted(want)
        for q in want:
            assert got[q].decode() == "".join(l + "\n" for l in want[q]), (name, q)
        assert np.fromfile(os.path.join(XC.GOLD, name + ".dbtype"), np.int32)[0] == 102          # DBTYPE_TMSCORE
    assert 3 * r == len(tasks)


@functools.lru_cache(maxsize=None)
def _live(which, is_exact, only):
    """the live model on the chosen tasks of a list, on a process pool (an exact task of 150 pairs takes about a second) -> {index: row + ties}"""
    cq, ct, tasks = XC.LISTS[which]()
    args = XC.task_args(cq, ct, tasks, is_exact, set(only))
    with multiprocessing.get_context("fork").Pool(min(8, os.cpu_count() or 1)) as pool:
        return dict(zip(sorted(only), pool.map(XC.model_row, args, chunksize=2)))


def _fixture_sample():
    """every crafted record with its three normalisations, and normalisation r mod 3 of record r of the 144"""
    return tuple([3 * r + r % 3 for r in range(N_CA)] + list(range(3 * N_CA, 3 * (N_CA + len(TC.crafted_records())))))


@pytest.mark.parametrize("is_exact", [False, True])
def test_live_model_equals_the_frozen_fixture_answers(is_exact):
    raw = XC.frozen_raw("fixture", is_exact)
    live = _live("fixture", is_exact, _fixture_sample())
    assert len(live) == N_CA + 3 * len(TC.crafted_records())
    for k, row in live.items():
        assert row[:X.RAW_COLS].tobytes() == raw[k].tobytes(), (k, row, raw[k])


@pytest.mark.parametrize("is_exact", [False, True])
def test_live_model_equals_a_sample_of_the_frozen_corpus(is_exact):
    """a spread sample: every 37th task (all pair counts come by: the counts cycle with period 24) and the first self-alignments"""
    _, _, tasks = XC.corpus()
    raw = XC.frozen_raw("corpus", is_exact)
    assert len(raw) == len(tasks)
    only = tuple(sorted(set(range(0, len(tasks), 37)) | {3, 10, 17, 24}))
    live = _live("corpus", is_exact, only)
    ties = XC.frozen_ties()
    for k, row in live.items():
        assert row[:X.RAW_COLS].tobytes() == raw[k].tobytes(), (k, row, raw[k])
        if is_exact:
            assert row[X.RAW_COLS:].tolist() == ties[k].tolist(), k


def test_the_corpus_shows_the_first_maximum_rule():
    """self-alignments and exact rigid copies: the exact search's maximum is reached by several starts with bit-distinct superpositions that lie in
    more than one block of starts, so a wrong tie rule or a wrong reduction across workgroups changes t / u"""
    _, _, tasks = XC.corpus()
    ties = XC.frozen_ties()
    assert ties.shape == (len(tasks), 3)
    assert int(((ties[:, 0] >= 2) & (ties[:, 1] >= 2) & (ties[:, 2] >= 2)).sum()) >= 10
    counts = {t[4].count("M") for t in tasks}
    assert set(XC.boundary_counts()) | set(range(1, 10)) | {31, 32, 33, 63, 64, 65, 127, 128, 129} <= counts and any(c >= 295 for c in counts)
    lo, hi = XC.boundary_counts()[2:4]
    assert XC.total_starts(lo) <= XC.STARTS_PER_BLOCK < XC.total_starts(hi)
    assert (XC.total_starts(28), XC.total_starts(29)) == (63, 66)
    text = open(os.path.join(K.ROOT, "foldseek_amd", "csrc", "k_tm_exact.hpp")).read()
    assert "constexpr int kTmSpWaves = 2;" in text and "kTmSpBlock = 64 * kTmSpWaves" in text and XC.STARTS_PER_BLOCK == 128


def test_crafted_records_take_their_branches_in_exact_mode():
    coords = TC.crafted_coords()
    by = {}
    for q, t, qs, ts, cig in TC.crafted_records():
        bt = TC.M.expand(cig)
        xtm, ytm = T.pairs(coords[q], coords[t], qs, ts, bt)
        stats = {}
        nl = TC.norm_lengths(qs, ts, bt, coords[q].shape[1], coords[t].shape[1])[0]
        res = X.exact(xtm, ytm, nl, stats)
        by[(q, t, cig)] = (res, stats, nl)
    names = {l.split()[1]: int(l.split()[0]) for l in open(os.path.join(TC.GOLD, "tmdb.lookup"))}
    qs_, ts_, tf = names["qshort"], names["tshort"], names["tfar"]
    for cig in ("1M", "2M", "3M"):
        assert by[(qs_, ts_, cig)][1].get("relief", 0) == 0                  # n_ali > 3 is false: the relief loop is never entered
    one = by[(qs_, ts_, "1M")]
    assert one[2] == 0 and one[1].get("fallback", 0) > 0                     # normLen 0; a single pair: NaN rotation -> the classical Kabsch()
    assert np.isposinf(one[0]["scores"][0]) and T.sstr(X.exact_finish(1, one[0]["scores"][0], one[0]["rms"])[0]) == "INF"
    assert one[0]["source"] == X.SRC_EXACT
    assert by[(qs_, tf, "4M")][1].get("relief", 0) > 10                      # the relief loop walks far
    self12 = by[(qs_, qs_, "12M")]
    assert self12[1].get("relief", 0) == 0 and float(X.exact_finish(12, self12[0]["scores"][0], self12[0]["rms"])[1]) == 0.0
    # a self-alignment: every start reaches the same score; the first one (ordinal 0) keeps the superposition
    assert self12[0]["ord"] == 0 and XC.ties_of(self12[1], self12[0]["scores"][0])[0] == XC.total_starts(12)


def test_zero_pairs_is_the_contract_of_the_entry_not_the_reference():
    empty = np.zeros((3, 0), np.float32)
    for res in (X.approximate(empty, empty, 10), X.exact(empty, empty, 10)):
        n, s0, s1, rms, source, t, u = X.row_fields(X.raw_row(res))
        assert (n, float(s0), float(s1), float(rms), source) == (0, -1.0, -1.0, 0.0, X.SRC_NONE)
        assert t.tolist() == [0, 0, 0] and u.reshape(3, 3).tolist() == np.eye(3).tolist()


def test_host_exact_params_equal_the_model():
    for nl in list(range(0, 401)) + [1000, 5000, 65535]:
        got = api.tm_exact_params(nl)
        want = np.array(X.exact_params(nl), np.float32)
        assert got.tobytes() == want.tobytes(), (nl, got, want)
    assert api.tm_exact_params(0)[1] == 0.0


def test_host_exact_finish_equals_the_model():
    rng = np.random.default_rng(20261022)
    cases = [(int(n), np.float32(s), np.float32(r)) for n, s, r in zip(rng.integers(1, 2000, 500), rng.random(500), rng.random(500) * 900)]
    cases += [(1, np.float32("inf"), np.float32(0)), (7, np.float32(-1), np.float32(0)), (3, np.float32(0.25), np.float32(1e-9)), (0, np.float32(-1), np.float32(0))]
    for n, s, r in cases:
        tm, rmsd = api.tm_exact_finish(n, s, r)
        wtm, wrmsd = X.exact_finish(n, s, r)
        assert np.float64(tm).tobytes() == np.float64(wtm).tobytes() and np.float32(rmsd).tobytes() == np.float32(wrmsd).tobytes(), (n, s, r)
        assert tm == float(s)


def test_symbols_and_struct_layouts():
    out = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for sym in ("fsgpu_tm_superpose_batch", "fshost_tm_exact_params", "fshost_tm_exact_finish", "fsmod_aln2tmscore", "fsgpu_tm_batch"):
        assert sym in names, sym
    assert "fsgpu_tm_superpose_batch" in api.exported_symbols()
    assert C.sizeof(api.TmResult) == 68 and api.TmResult.score.offset == 8 and api.TmResult.rms.offset == 16
    assert api.TmResult.t.offset == 20 and api.TmResult.u.offset == 32 and api.TmResult.source.offset == 4
    assert C.sizeof(api.TmTask) == 56                                  # fsgpu_tm_task is unchanged
    assert (api.TM_SRC_NONE, api.TM_SRC_KABSCH, api.TM_SRC_SEARCH1, api.TM_SRC_SEARCH2, api.TM_SRC_EXACT) == (0, 1, 2, 3, 4)
    header = open(os.path.join(K.ROOT, "include", "fsgpu.h")).read()
    for k, name in enumerate(("NONE", "KABSCH", "SEARCH1", "SEARCH2", "EXACT")):
        assert f"#define FSGPU_TM_SRC_{name} {k}" in header
    assert hasattr(api.Context, "tm_superpose_batch")
    lib = api.lib()
    assert lib.fsgpu_tm_superpose_batch.argtypes[9] is C.c_int and lib.fshost_tm_exact_finish.restype is C.c_double


def test_aln2tmscore_argument_errors_come_before_a_device_is_opened(tmp_path):
    db, aln, out = os.path.join(K.GOLD, "db"), os.path.join(K.GOLD, "aln_l0"), str(tmp_path / "out")
    run = lambda args: subprocess.run([BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)  # noqa: E731
    r = run([])
    assert r.returncode != 0 and "aln2tmscore" in r.stderr                              # the usage line names the module
    r = run(["aln2tmscore", db, db, aln])
    assert r.returncode == 1 and "usage: aln2tmscore <queryDB> <targetDB> <alignmentDB> <outDB>" in r.stderr
    r = run(["aln2tmscore", db, db, aln, out, "--tmscore-threshold-mode", "3"])
    assert r.returncode == 1 and "Error in argument --tmscore-threshold-mode" in r.stderr
    r = run(["aln2tmscore", db, db, aln, out, "--exact-tmscore", "2"])
    assert r.returncode == 1 and "Error in argument --exact-tmscore" in r.stderr
    r = run(["aln2tmscore", db, db, aln, out, "--gpus", "2"])
    assert r.returncode == 1 and "aln2tmscore: --gpus 2 is not implemented for this module" in r.stderr
    r = run(["aln2tmscore", db, db, aln, out, "--no-such-flag", "1"])
    assert r.returncode == 1
    # a database without C-alpha coordinates: the sequence files alone
    bare = str(tmp_path / "bare")
    for ext in ("", ".index", ".dbtype"):
        with open(bare + ext, "wb") as f:
            f.write(open(db + ext, "rb").read())
    r = run(["aln2tmscore", bare, bare, aln, out])
    assert r.returncode == 1 and "has no C-alpha coordinates (no <db>_ca)" in r.stderr
    r = run(["aln2tmscore", db, bare, aln, out])
    assert r.returncode == 1 and "bare has no C-alpha coordinates" in r.stderr
    # records that cannot be answered are refused before a device is opened too: no backtrace, no M column
    for name, rec, msg in (("nobt", "1\t100\t0.500\t1.000E-05\t0\t9\t{ql}\t0\t9\t{tl}\n", "Backtrace cigar is missing in the alignment result. Please recompute the alignment with the -a flag."),
                           ("nom", "1\t100\t0.500\t1.000E-05\t0\t1\t{ql}\t0\t1\t{tl}\t2I2D\n", "has no M column")):
        lens = {int(l.split()[0]): int(l.split()[2]) - 2 for l in open(db + ".index")}
        entry = rec.format(ql=lens[0], tl=lens[1]).encode() + b"\0"
        p = str(tmp_path / name)
        open(p, "wb").write(entry)
        open(p + ".index", "w").write(f"0\t0\t{len(entry)}\n")
        open(p + ".dbtype", "wb").write(np.int32(5).tobytes())
        r = run(["aln2tmscore", db, db, p, out])
        assert r.returncode == 1 and msg in r.stderr, (name, r.stderr)
    assert not os.path.exists(out) and not os.path.exists(out + ".index")
