"""fsgpu_tm_superpose_batch (k_tm_pairs + k_tm_sp_search + k_tm_sp_finish) called directly through Context.tm_superpose_batch, and the aln2tmscore module,
against the independent model (tests/tm_exact_model.py, held to the reference binary's output by the fixture generator and tests/test_tm_exact_model.py).
Device results are compared with the model's frozen answers as float BIT patterns: the pair count, the raw scores, the raw rms, the source code and all
twelve numbers of t / u, approximate and exact.

Tolerated: on the seeded corpus at most 2 tasks may differ per mode, and those must still print identical SSTR text in every field.  The only operations
whose results cannot be argued from IEEE rules are the double-precision atan2 / cos / sin of the eigen step (device library here, glibc in the model and
the reference).  The fixture tasks allow no difference.  Measured on an MI355X: one corpus task differs in each mode, in the last bit of one number of
t / u, with the same text; the corpus seed was fixed with the existing fsgpu_tm_batch alone (tm_exact_cases.CORPUS_SEED)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lddt_cases as K
import tm_cases as TC
import tm_exact_cases as XC
import tm_exact_model as X
import tm_model as T
from foldseek_amd import api

pytestmark = pytest.mark.gpu

BIN = os.path.join(K.ROOT, "foldseek_amd", "bin", "fsgpu-modules")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def _differing(got, want):
    return [k for k in range(len(want)) if got[k].tobytes() != want[k].tobytes()]


def _describe(k, task, got, want):
    return f"task {k} (pairs {want[0]}, normLen {task[5]}): device {X.row_fields(got)} model {X.row_fields(want)}"


@pytest.mark.parametrize("is_exact", [False, True])
def test_all_fixture_tasks_in_one_call(ctx, is_exact):
    """the 144 records of the 12 example structures and the crafted records, three normalisations each, as ONE call: zero mismatches"""
    coords, tasks = XC.fixture_tasks()
    want = XC.frozen_raw("fixture", is_exact)
    assert len(tasks) == len(want) == 3 * (144 + len(TC.crafted_records()))
    got = XC.raw_of_device(ctx.tm_superpose_batch(coords, coords, tasks, exact=is_exact))
    bad = _differing(got, want)
    for k in bad:
        print(_describe(k, tasks[k], got[k], want[k]))
    assert not bad
    print("kernel ms (pairs, search, finish):", [ctx.kernel_ms(w) for w in (18, 19, 20)])
    assert ctx.kernel_ms(18) >= 0 and ctx.kernel_ms(19) > 0 and ctx.kernel_ms(20) >= 0
    if not is_exact:                                   # the scores and the rmsd are what the existing entry returns
        old = TC.raw_of_device(ctx.tm_batch(coords, coords, tasks))
        assert old.tobytes() == np.ascontiguousarray(got[:, :4]).tobytes()
        print("fsgpu_tm_batch kernel ms (pairs, search):", [ctx.kernel_ms(w) for w in (16, 17)])
        assert set(got[:, 4].tolist()) <= {X.SRC_KABSCH, X.SRC_SEARCH1, X.SRC_SEARCH2}
    else:
        assert set(got[:, 4].tolist()) <= {X.SRC_KABSCH, X.SRC_EXACT} and (got[:, 2] == np.float32(-1).view(np.uint32)).all()


@pytest.mark.parametrize("is_exact", [False, True])
def test_seeded_corpus(ctx, is_exact):
    """2 024 small hits (tm_exact_cases.corpus): pair counts 1-9, around the block boundaries of the exact search, 31-33, 63-65, 127-129, about 300; gaps,
    start cells, rigid motions, noise from none to unrelated, self-alignments and exact rigid copies"""
    queries, targets, tasks = XC.corpus()
    want = XC.frozen_raw("corpus", is_exact)
    assert len(tasks) == len(want) >= 2000
    if is_exact:                                       # from the model: ties between starts with different rotations, in more than one block of starts
        ties = XC.frozen_ties()
        assert int(((ties[:, 0] >= 2) & (ties[:, 1] >= 2) & (ties[:, 2] >= 2)).sum()) >= 10
    got = XC.raw_of_device(ctx.tm_superpose_batch(queries, targets, tasks, exact=is_exact))
    assert (got[:, 0] == want[:, 0]).all()
    bad = _differing(got, want)
    for k in bad:
        print(_describe(k, tasks[k], got[k], want[k]))
    print(f"exact = {int(is_exact)}: {len(bad)} of {len(tasks)} tasks differ; in the scores or the rms: {len(_differing(got[:, :4], want[:, :4]))}; "
          f"with other text: {sum(XC.row_text(got[k], tasks[k][5], is_exact) != XC.row_text(want[k], tasks[k][5], is_exact) for k in bad)}")
    assert len(bad) <= 2
    for k in bad:
        assert XC.row_text(got[k], tasks[k][5], is_exact) == XC.row_text(want[k], tasks[k][5], is_exact)
    if not is_exact:
        old = TC.raw_of_device(ctx.tm_batch(queries, targets, tasks))
        assert old.tobytes() == np.ascontiguousarray(got[:, :4]).tobytes()


def test_lds_limit_and_growing_workspaces(ctx):
    """a hit AT the LDS limit and one just past it (pairs and masks in global memory) in exact mode, between two small calls on one context: the partial
    and mask workspaces grow, and stale data lies behind the smaller call that follows"""
    queries, targets, tasks = XC.edge()
    want = XC.frozen_raw("edge", True)
    assert [int(w[0]) for w in want] == [XC.LDS_PAIRS, XC.LDS_PAIRS + 1]
    cq, ct, ctasks = XC.corpus()
    small = list(range(0, 48))
    sq, st = [cq[ctasks[k][0]] for k in small], [ct[ctasks[k][1]] for k in small]
    stasks = [(i, i) + ctasks[k][2:] for i, k in enumerate(small)]
    swant = XC.frozen_raw("corpus", True)[small]
    assert not _differing(XC.raw_of_device(ctx.tm_superpose_batch(sq, st, stasks, exact=True)), swant)
    got = XC.raw_of_device(ctx.tm_superpose_batch(queries, targets, tasks, exact=True))
    bad = _differing(got, want)
    for k in bad:
        print(_describe(k, tasks[k], got[k], want[k]))
    assert not bad
    assert not _differing(XC.raw_of_device(ctx.tm_superpose_batch(sq, st, stasks, exact=True)), swant)
    got = XC.raw_of_device(ctx.tm_superpose_batch(queries, targets, tasks, exact=False))
    assert not _differing(got, XC.frozen_raw("edge", False))


@pytest.mark.parametrize("is_exact", [False, True])
def test_empty_call_and_zero_pair_task(ctx, is_exact):
    rng = np.random.default_rng(11)
    q, t = TC._walk(rng, 20), TC._walk(rng, 20)
    assert ctx.tm_superpose_batch([q], [t], [], exact=is_exact) == []
    assert ctx.tm_superpose_batch([], [], [], exact=is_exact) == []
    tasks = [(0, 0, 2, 3, "IIDDD", 20), (0, 0, 0, 0, "M" * 20, 20), (0, 0, 0, 0, "", 0)]
    got = XC.raw_of_device(ctx.tm_superpose_batch([q], [t], tasks, exact=is_exact))
    want = XC.model_raw([q], [t], tasks, is_exact)
    assert got.tobytes() == want.tobytes()
    for k in (0, 2):                                   # scores -1, rms 0, source "none", the identity
        n, s0, s1, rms, source, tt, uu = X.row_fields(got[k])
        assert (n, float(s0), float(s1), float(rms), source) == (0, -1.0, -1.0, 0.0, api.TM_SRC_NONE)
        assert tt.tolist() == [0, 0, 0] and uu.reshape(3, 3).tolist() == np.eye(3).tolist()


@pytest.mark.parametrize("is_exact", [False, True])
def test_bad_tasks_are_refused_not_run(ctx, is_exact):
    """the argument checks of fsgpu_tm_batch: an error from the entry, nothing launched, and the context goes on working"""
    rng = np.random.default_rng(3)
    q, t = TC._walk(rng, 20), TC._walk(rng, 20)
    for task in ((0, 0, 0, 0, "M" * 21, 20), (0, 0, 5, 0, "M" * 16, 20), (0, 0, 0, 18, "MMD", 20), (0, 0, 0, 18, "MMX", 20), (0, 0, -1, 0, "M", 20),
                 (1, 0, 0, 0, "M", 20)):
        with pytest.raises(api.FsgpuError):
            ctx.tm_superpose_batch([q], [t], [task], exact=is_exact)
    good = [float(v) for v in (api.tm_exact_params(20) if is_exact else api.tm_params(20))]
    for slot in range(4):
        for bad in (float("nan"), float("inf"), 0.0, -1.0):
            if is_exact and slot == 1 and bad == 0.0:
                continue                               # Lnorm 0 is what a one-column alignment has
            par = list(good)
            par[slot] = bad
            with pytest.raises(api.FsgpuError):
                ctx.tm_superpose_batch([q], [t], [(0, 0, 0, 0, "M" * 20, 20)], exact=is_exact, params=[par])
    task = [(0, 0, 0, 0, "M" * 20, 20)]
    assert XC.raw_of_device(ctx.tm_superpose_batch([q], [t], task, exact=is_exact)).tobytes() == XC.model_raw([q], [t], task, is_exact).tobytes()


# ---- the module ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def work(tmp_path_factory):
    w = tmp_path_factory.mktemp("a2t")
    for src, prefixes in ((K.GOLD, ("db", "aln_l0")), (TC.GOLD, ("tmdb", "tmaln"))):
        for f in os.listdir(src):
            if f.startswith(prefixes) and not f.startswith("db_pad") and (not f.startswith("aln_l0") or f.split(".")[0] == "aln_l0"):
                shutil.copy(os.path.join(src, f), w / f)
    return w


def _run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


@pytest.mark.parametrize("name,db,aln", [("a2t_ca", "db", "aln_l0"), ("a2t_crafted", "tmdb", "tmaln")])
def test_aln2tmscore_equals_the_reference_result_db(work, name, db, aln):
    out = str(work / ("mine_" + name))
    r = _run([BIN, "aln2tmscore", str(work / db), str(work / db), str(work / aln), out, "--threads", "1", "--compressed", "0", "-v", "1"])
    assert r.returncode == 0, r.stderr
    for ext in ("", ".index", ".dbtype"):
        assert open(out + ext, "rb").read() == open(os.path.join(XC.GOLD, name + ext), "rb").read(), ext


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_aln2tmscore_exact_equals_the_reference_convertalis_columns(work, mode):
    """--exact-tmscore 1: the score of every line is the alntmscore / qtmscore / ttmscore column of the reference's convertalis --exact-tmscore 1 for the
    same record; with mode 2 the t and u text is its t and u columns (which convertalis computes with the target length); in every mode the whole line
    is what the frozen model gives"""
    _, tasks = XC.fixture_tasks()
    raw = XC.frozen_raw("fixture", True)
    r0 = 0
    for db, aln, conv, recs in (("db", "aln_l0", "conv_x1.m8", K.records("aln_l0")), ("tmdb", "tmaln", "conv_x1_crafted.m8", TC.crafted_records())):
        out = str(work / f"mine_x_{db}_{mode}")
        r = _run([BIN, "aln2tmscore", str(work / db), str(work / db), str(work / aln), out, "--exact-tmscore", "1", "--tmscore-threshold-mode", str(mode)])
        assert r.returncode == 0, r.stderr
        rows = [l.rstrip("\n").split("\t") for l in open(os.path.join(XC.GOLD, conv))]
        got = TC.result_records(lambda n: _read_db(n), out)
        assert len(got) == len(rows) == len(recs)
        for k, ((q, fields), row, rec) in enumerate(zip(got, rows, recs)):
            f = fields[0].split(" ")
            assert q == rec[0] and int(f[0]) == rec[1]
            assert f[1] == row[2 + mode], (k, f, row)
            if mode == 2:
                assert ",".join(f[2:5]) == row[7] and ",".join(f[5:14]) == row[6], (k, f, row)
            task = 3 * (r0 + k) + mode
            assert " ".join(f) == X.aln2tmscore_line(rec[1], raw[task], tasks[task][5], True), (k, f)
        r0 += len(recs)


def _read_db(path):
    data = open(path, "rb").read()
    out = {}
    for line in open(path + ".index"):
        k, off, ln = line.split()
        out[int(k)] = data[int(off):int(off) + int(ln) - 1]
    return out
