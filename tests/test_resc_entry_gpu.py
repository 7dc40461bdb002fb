"""fshost_search_rescore_diagonal_batch (Search.rescore_diagonal_batch) and the structurerescorediagonal module against the independent model of the
reference's per-query body (tests/resc_model.py), on the seeded world of tests/resc_cases.py whose gates are decided at their edges and on the frozen runs
of the reference binary.  Everything expected here was frozen by tests/golden/make_resc_golden.py (tests/golden/resc_v1); the model is held to the
reference binary by tests/test_resc_model.py, which also pins what the world contains.  Compared exactly: count, order and every record field as bit
patterns (float coverage and identity, the double e-value), backtraceLen, the backtrace strings, nres, and the bytes behind results[q][nres[q]].
No tolerance anywhere: the kernel below is integer arithmetic, the e-value is computed on the host."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import resc_cases as K
from foldseek_amd import api, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "foldseek_amd", "bin", "fsgpu-modules")
FIELDS = ("dbKey", "score", "qcov", "dbcov", "seqId", "eval", "alnLength", "qStartPos", "qEndPos", "qLen", "dbStartPos", "dbEndPos", "dbLen")
MANIFEST = json.load(open(os.path.join(K.GOLD, "MANIFEST.json")))
KIND_TEXT = {"undefined": "negative diagonal with a target longer than the query", "no overlap": "diagonal outside the sequences"}


def pack(targets):
    """PaddedDB in id order, every entry padded to a multiple of four with X"""
    lens = np.array([len(a) for a, _ in targets], np.int32)
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum((lens.astype(np.int64) + 3) // 4 * 4)
    d3, da = np.full(off[-1], 20, np.uint8), np.full(off[-1], 20, np.uint8)
    for k, (a, s) in enumerate(targets):
        d3[off[k]:off[k] + lens[k]] = s
        da[off[k]:off[k] + lens[k]] = a
    return synth.PaddedDB(d3, da, off, lens)


@pytest.fixture(scope="module")
def env():
    w = K.world()
    ctx = api.Context(0)
    ctx.load_db(pack(w["targets"]))
    assert ctx.residues == sum(len(a) for a, _ in w["targets"])          # what the model's e-values were computed with
    yield dict(w=w, ctx=ctx, frozen={t: K.Frozen(t) for t in K.ATYPES})
    ctx.close()


def make_params(atype, S):
    P = S["P"]
    par = api.default_params()
    par.alignmentType, par.addBacktrace, par.skipUndefinedDiagonals = atype, P["addBacktrace"], int(S["skip"])
    par.evalThr, par.covThr, par.covMode = P["evalThr"], P["covThr"], P["covMode"]
    par.seqIdThr, par.seqIdMode, par.alnLenThr = P["seqIdThr"], P["seqIdMode"], P["alnLenThr"]
    par.maxAccept, par.maxRejected = P["maxAccept"], P["maxRejected"]
    assert np.float32(par.covThr) == np.float32(P["covThr"]) and np.float32(par.seqIdThr) == np.float32(P["seqIdThr"]) and par.evalThr == P["evalThr"]
    return par


def same_records(got, bts, want, where):
    rec, want_bt, _ = want
    assert len(got) == len(rec), (where, len(got), len(rec))
    for f in FIELDS:
        g, x = np.ascontiguousarray(got[f]), np.ascontiguousarray(rec[f])
        assert g.dtype == x.dtype, (where, f)
        if g.tobytes() != x.tobytes():
            k = int(np.flatnonzero(g != x)[0]) if (g != x).any() else 0
            raise AssertionError(f"{where}: field {f} of record {k}: got {got[k]}, want {rec[k]}")
    assert list(bts) == list(want_bt), where
    assert [int(x) for x in got["backtraceLen"]] == [len(b) for b in want_bt], where


def canary_intact(s, counts, where):
    """the result buffers hold n[q] + 1 records; nothing behind nres[q] was written"""
    bufs, nres = s.last_rescore
    assert len(bufs) == len(counts) == len(nres)
    for q, (b, n) in enumerate(zip(bufs, counts)):
        assert len(b) == n + 1 and 0 <= nres[q] <= n, (where, q)
        assert (b[nres[q]:].view(np.uint8) == api.Search.RESCORE_CANARY).all(), (where, q, "bytes behind nres[q] were written")


def call(env, s, F, names, identity=True):
    """one library call with the named lists -> what rescore_diagonal_batch returns"""
    w = env["w"]
    ls = [F.list_of(n) for n in names]
    ident = [w["identity"][q] for q, _, _, _ in ls] if identity is True else identity
    out = s.rescore_diagonal_batch([w["queries"][q][0] for q, _, _, _ in ls], [w["queries"][q][1] for q, _, _, _ in ls], [t for _, t, _, _ in ls], [d for _, _, d, _ in ls],
                                   identity=ident)
    canary_intact(s, [len(t) for _, t, _, _ in ls], names)
    return out


def _cases():
    F = K.Frozen(2)
    return [(t, n) for t in K.ATYPES for n in F.names]


@pytest.mark.parametrize("atype,name", _cases())
def test_entry_equals_the_model(env, atype, name):
    """every parameter set: thresholds AT a hit's value and one representable number beyond it for every comparison of the loop, both counter limits, the skip
    rule inside a run of rejections and behind the cut.  All lists of the set in ONE call, then each alone; a set the model refuses is refused here, with
    the model's query, target key, diagonal and case in the text, and the same handle answers the next call"""
    F = env["frozen"][atype]
    S = F.set(name)
    s = api.Search(env["ctx"], make_params(atype, S), keys=env["w"]["keys"])
    try:
        ident = True if S["identity"] else [-1] * len(S["lists"])
        if S["error"]:
            bad = S["lists"].index(S["error"]["list"])
            with pytest.raises(api.FsgpuError) as e:
                call(env, s, F, S["lists"], ident)
            text = str(e.value)
            assert e.value.rc == api.FSGPU_E_UNSUPPORTED, text
            assert f"query {bad} target key {S['error']['key']} diagonal {S['error']['diagonal']}:" in text and KIND_TEXT[S["error"]["kind"]] in text, text
            good = [n for n in S["lists"] if n != S["error"]["list"]] or ["q5"]
            res, bts = call(env, s, F, good, True)
            D = env["frozen"][atype]
            for k, n in enumerate(good):
                want = F.records(name, S["lists"].index(n)) if n in S["lists"] else D.records("default", K.DEFINED.index(n))
                same_records(res[k], bts[k], want, (atype, name, "after the refusal", n))
            return
        res, bts = call(env, s, F, S["lists"], ident)
        for k, n in enumerate(S["lists"]):
            same_records(res[k], bts[k], F.records(name, k), (atype, name, "one call", n))
        for k, n in enumerate(S["lists"]):
            r1, b1 = call(env, s, F, [n], ident if ident is True else [-1])
            same_records(r1[0], b1[0], F.records(name, k), (atype, name, "alone", n))
    finally:
        s.close()


@pytest.mark.parametrize("atype", K.ATYPES)
def test_three_hundred_queries_in_one_call(env, atype):
    """the world's lists repeated in a shuffled order with empty lists in between: the concatenation of queries padded to a multiple of four, the base[]
    offsets of every query's pairs, and n[q] == 0 (nres 0, nothing written)"""
    F, w = env["frozen"][atype], env["w"]
    rng = np.random.default_rng(K.SEED + 300)
    names = [K.DEFINED[int(i)] for i in rng.integers(0, len(K.DEFINED), 300)]
    empty = set(int(i) for i in rng.choice(300, 40, replace=False)) | {0, 299}
    S = F.set("e1e-3")
    s = api.Search(env["ctx"], make_params(atype, S), keys=w["keys"])
    try:
        ls = [F.list_of(n) for n in names]
        ts = [t[:0] if k in empty else t for k, (_, t, _, _) in enumerate(ls)]
        ds = [d[:0] if k in empty else d for k, (_, _, d, _) in enumerate(ls)]
        res, bts = s.rescore_diagonal_batch([w["queries"][q][0] for q, _, _, _ in ls], [w["queries"][q][1] for q, _, _, _ in ls], ts, ds,
                                            identity=[w["identity"][q] for q, _, _, _ in ls])
        canary_intact(s, [len(t) for t in ts], "300 queries")
        assert sum(len(r) for r in res) > 1000
        for k, n in enumerate(names):
            if k in empty:
                assert len(res[k]) == 0 and s.last_rescore[1][k] == 0
            else:
                same_records(res[k], bts[k], F.records("e1e-3", K.DEFINED.index(n)), (atype, "300 queries", k, n))
    finally:
        s.close()


@pytest.mark.parametrize("atype", K.ATYPES)
def test_identity_argument(env, atype):
    """identityId == NULL and -1 everywhere are the same thing; the identity is a target INDEX (every key of this world differs from its index)"""
    F, w = env["frozen"][atype], env["w"]
    assert all(int(w["keys"][i]) != i for i in w["identity"])
    s = api.Search(env["ctx"], make_params(atype, F.set("ident_sid")), keys=w["keys"])
    try:
        for ident in (None, [-1] * len(K.DEFINED)):
            res, bts = call(env, s, F, K.DEFINED, ident)
            for k, n in enumerate(K.DEFINED):
                same_records(res[k], bts[k], F.records("ident_sid_noid", k), (atype, "no identity", ident is None, n))
        res, bts = call(env, s, F, K.DEFINED, True)
        for k, n in enumerate(K.DEFINED):
            same_records(res[k], bts[k], F.records("ident_sid", k), (atype, "identity", n))
        assert any(len(F.records("ident_sid", k)[0]) != len(F.records("ident_sid_noid", k)[0]) for k in range(len(K.DEFINED)))
        # the keys of the identity targets in place of their indices: no target has that index as its own query's, nothing is accepted as identity
        res, bts = call(env, s, F, K.DEFINED, [int(w["keys"][i]) for i in w["identity"]])
        assert all(int(w["keys"][i]) >= len(w["targets"]) for i in w["identity"])
        for k, n in enumerate(K.DEFINED):
            same_records(res[k], bts[k], F.records("ident_sid_noid", k), (atype, "keys as identity", n))
    finally:
        s.close()


def _raw(s, qa, q3, L, ts, ds, n):
    """the C entry with one query and arguments the binding would not build: -> (rc, error text, nres)"""
    res = np.zeros(max(1, len(ts)) + 1, api.RESULT_DT)
    P = C.c_void_p * 1
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    Ls, ns, nres = np.array([L], np.int32), np.array([n], np.int32), np.full(1, -7, np.int32)
    rc = api.lib().fshost_search_rescore_diagonal_batch(s.h, 1, C.cast(P(ptr(qa)), C.c_void_p), C.cast(P(ptr(q3)), C.c_void_p), Ls.ctypes.data, None,
                                                        C.cast(P(ptr(ts)), C.c_void_p), C.cast(P(ptr(ds)), C.c_void_p), ns.ctypes.data,
                                                        C.cast(P(ptr(res)), C.c_void_p), nres.ctypes.data)
    return rc, api.lib().fshost_search_error(s.h).decode(), int(nres[0])


def test_refusals_leave_the_handle_usable(env):
    """a target id equal to the database size, L == 0, n[q] < 0, a null query pointer: FSGPU_E_ARG with a text that names the query; after each of them the
    same handle answers a correct call with the model's records"""
    F, w = env["frozen"][2], env["w"]
    S = F.set("default")
    s = api.Search(env["ctx"], make_params(2, S), keys=w["keys"])
    try:
        q, ts, ds, _ = F.list_of("q5")
        qa, q3 = (np.ascontiguousarray(x) for x in w["queries"][q])
        ts, ds = np.ascontiguousarray(ts), np.ascontiguousarray(ds)

        def good(after):
            res, bts = call(env, s, F, ["q4", "q5"], True)
            same_records(res[1], bts[1], F.records("default", K.DEFINED.index("q5")), after)
            same_records(res[0], bts[0], F.records("default", K.DEFINED.index("q4")), after)

        bad = ts.copy()
        bad[7] = len(w["targets"])
        with pytest.raises(api.FsgpuError, match="target id out of range: query 1 entry 7") as e:
            s.rescore_diagonal_batch([qa, qa], [q3, q3], [ts, bad], [ds, ds])
        assert e.value.rc == api.FSGPU_E_ARG
        good("after a target id past the database")
        for what, args, needle in (("L == 0", (qa, q3, 0, ts, ds, len(ts)), "query 0: length 0"), ("n < 0", (qa, q3, len(qa), ts, ds, -1), "query 0: list length -1"),
                                   ("null AA", (None, q3, len(qa), ts, ds, len(ts)), "query 0: null sequence"),
                                   ("null 3Di", (qa, None, len(qa), ts, ds, len(ts)), "query 0: null sequence")):
            rc, text, nres = _raw(s, *args)
            assert rc == api.FSGPU_E_ARG and needle in text and nres == -7, (what, rc, text, nres)
            good("after " + what)
        rc, text, nres = _raw(s, qa, q3, len(qa), ts, ds, len(ts))                       # the same raw call with nothing wrong
        assert rc == 0 and nres == len(F.records("default", K.DEFINED.index("q5"))[0])
    finally:
        s.close()


def test_interleaved_with_the_alignment_entry(env):
    """align_batch with backtraces, the rescoring call, align_batch again, on ONE handle: the cigar buffer is shared and every call clears it -- each call's
    backtraces, read before the next call, are its own"""
    F, w = env["frozen"][2], env["w"]
    S = F.set("default")
    qs = [3, 5]
    qa, q3 = [w["queries"][q][0] for q in qs], [w["queries"][q][1] for q in qs]
    lists = [np.unique(F.list_of(f"q{q}")[1]) for q in qs]
    ident = [w["identity"][q] for q in qs]
    fresh = api.Search(env["ctx"], make_params(2, S), keys=w["keys"])
    try:
        want, want_bt = fresh.align_batch(qa, q3, lists, identity=ident, with_backtrace=True)
    finally:
        fresh.close()
    assert sum(len(r) for r in want) >= 10 and all(len(b) > 0 for bs in want_bt for b in bs)
    s = api.Search(env["ctx"], make_params(2, S), keys=w["keys"])
    try:
        for step in range(2):
            res, bts = s.align_batch(qa, q3, lists, identity=ident, with_backtrace=True)
            assert [r.tobytes() for r in res] == [r.tobytes() for r in want] and bts == want_bt, ("align_batch", step)
            r2, b2 = call(env, s, F, ["q5", "q3", "q9"], True)
            for k, n in enumerate(["q5", "q3", "q9"]):
                same_records(r2[k], b2[k], F.records("default", K.DEFINED.index(n)), ("rescoring between alignments", step, n))
            assert int(r2[0]["backtraceOff"].min()) == 0                               # the buffer was cleared, not appended to
    finally:
        s.close()


# ---- the module ------------------------------------------------------------------------------------------------------------------------------------------------------
def read_db(path):
    t = int.from_bytes(open(path + ".dbtype", "rb").read(4), "little", signed=True)
    data = open(path, "rb").read()
    out = {}
    for line in open(path + ".index"):
        k, off, ln = line.split()
        out[int(k)] = data[int(off):int(off) + int(ln) - 1]
    return t, out


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """the reference-written example databases, the same files once more under a second path, and the frozen prefilter lists"""
    d = tmp_path_factory.mktemp("resc")
    for f in os.listdir(K.SCOP):
        if (f.startswith("db") and not f.startswith("db_pad")) or f.startswith("pref_kmer"):
            shutil.copy(os.path.join(K.SCOP, f), d / f)
            if f.startswith("db"):
                shutil.copy(os.path.join(K.SCOP, f), d / ("db2" + f[2:]))
    for f in os.listdir(K.GOLD):
        if f.startswith("pref_resc_edges"):
            shutil.copy(os.path.join(K.GOLD, f), d / f)
    return d


@pytest.mark.parametrize("name", sorted(MANIFEST["runs"]))
def test_module_equals_the_reference_binary(work, name):
    """fsgpu-modules structurerescorediagonal with the argument vectors the reference binary was run with, on the inputs it read: every result DB byte for byte"""
    run = MANIFEST["runs"][name]
    out = str(work / ("mine_" + name))
    r = subprocess.run([BIN, run["module"]] + [str(work / p) for p in run["positional"]] + [out] + run["parameters"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    want_t, want = read_db(os.path.join(K.GOLD, name))
    got_t, got = read_db(out)
    assert got_t == want_t and sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k] == want[k], f"{name}: entry {k}\nwant {want[k][:300]!r}\ngot  {got[k][:300]!r}"
    assert sum(len(v) for v in want.values()) > 0


@pytest.mark.parametrize("extra", [[], ["--max-accept", "4", "--max-rejected", "3", "-e", "1e-3"], ["-c", "0.6", "--cov-mode", "1", "--max-rejected", "2"]])
def test_module_skips_undefined_pairs_like_the_model(work, extra):
    """--undefined-diagonals skip on the UNRESTRICTED k-mer prefilter lists (297 undefined pairs among them), with limits that make the counter rule decide
    what is written: the model with the skip rule on, byte for byte"""
    run = dict(MANIFEST["runs"]["e_cov0"], positional=["db", "db", "pref_kmer"])
    par = list(run["parameters"])
    par[par.index("-c") + 1] = "0"
    for i in range(0, len(extra), 2):
        par[par.index(extra[i]) + 1] = extra[i + 1]
    run["parameters"] = par
    pref = K.read_pref(os.path.join(K.SCOP, "pref_kmer"))
    want, res = K.model_db(run, pref, skip=True)
    skipped = sum(o.startswith("skipped") for r in res.values() for o in r.outcomes)
    assert skipped >= (250 if not extra else 5), skipped
    out = str(work / f"mine_skip_{len(extra)}_{extra[1] if extra else 'x'}")
    r = subprocess.run([BIN, "structurerescorediagonal"] + [str(work / p) for p in run["positional"]] + [out] + par + ["--undefined-diagonals", "skip"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    _, got = read_db(out)
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k] == want[k], f"entry {k}\nwant {want[k][:300]!r}\ngot  {got[k][:300]!r}"
