"""Profile queries without a device: fshost_profile_decode and fshost_profile_bias against tests/profile_model.py byte for byte, the decoder's
refusals, the new entries in the library and the binding; the model against the frozen runs of the reference binary on profile queries
(tests/golden/profile_v1: every prefilter record, the score and end positions of every alignment); the modules' refusals."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import gapless_model as gm
import profile_model as pm
from foldseek_amd import api


def crafted_entries():
    """{name: entry bytes}: one position; every score at its extremes; scores whose quarter rounds towards zero; 600 positions of the maximum; a long one"""
    rng = np.random.default_rng(20261020)
    out = {}
    out["L1"] = pm.encode(np.arange(-10, 10, dtype=np.int8).reshape(20, 1), [7], consensus=[3], neff=200)
    ext = np.where(rng.random((20, 40)) < 0.5, -128, 127).astype(np.int8)
    out["extremes"] = pm.encode(ext, rng.integers(0, 21, 40), consensus=rng.integers(0, 21, 40))
    out["towards zero"] = pm.encode(np.tile(np.arange(-9, 11, dtype=np.int8)[:, None], (1, 5)), [20, 0, 1, 2, 3])
    out["max600"] = pm.encode(np.full((20, 600), 127, np.int8), np.zeros(600, np.uint8))
    out["random1025"] = pm.encode(rng.integers(-128, 128, (20, 1025)).astype(np.int8), rng.integers(0, 21, 1025))
    return out


def _with_gap_bytes(entry):
    """the same entry with bytes 22 .. 24 of every record set: neff and the two gap bytes are not part of the answer"""
    rec = np.frombuffer(entry, np.uint8).reshape(-1, pm.RECORD).copy()
    rec[:, 22:] = np.arange(len(rec), dtype=np.int64)[:, None] * 7 % 251 + 1
    return rec.tobytes()


@pytest.mark.parametrize("name", sorted(crafted_entries()))
def test_decode_equals_the_model(name):
    entry = crafted_entries()[name]
    want = pm.decode(entry)
    for e in (entry, _with_gap_bytes(entry)):
        got = api.profile_decode(e)
        for g, w, what in zip(got, want, ("codes", "consensus", "profile", "reversed profile")):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (name, what)
    assert not want[2][20].any() and (want[3] == want[2][:, ::-1]).all()
    assert api.profile_bias(want[2]) == pm.bias(want[2]) and 0 <= pm.bias(want[2]) <= 32


def test_what_the_crafted_entries_are_for():
    e = crafted_entries()
    assert pm.decode(e["L1"])[2].shape == (21, 1) and pm.decode(e["L1"])[0][0] == 7 and pm.decode(e["L1"])[1][0] == 3
    assert set(np.unique(pm.decode(e["extremes"])[2][:20])) == {-32, 31}
    # C division: -9 .. -5 -> -2 / -1, -3 .. 3 -> 0 (a floor division would give -1 for -3 .. -1)
    assert pm.decode(e["towards zero"])[2][:20, 0].tolist() == [-2, -2, -1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2]
    assert pm.bias(pm.decode(e["max600"])[2]) == 0 and pm.cap(pm.decode(e["max600"])[2]) == 255
    assert pm.bias(pm.decode(e["extremes"])[2]) == 32 and pm.cap(pm.decode(e["extremes"])[2]) == 223


def test_outputs_are_optional_and_an_empty_entry_has_no_positions():
    entry = crafted_entries()["extremes"]
    buf = np.frombuffer(entry, np.uint8)
    L = len(buf) // pm.RECORD
    f = api.lib().fshost_profile_decode
    assert f(api._ptr(buf), len(buf), None, None, None, None, None, 0) == L
    rev = np.zeros((21, L), np.int8)
    assert f(api._ptr(buf), len(buf), None, None, None, api._ptr(rev), None, 0) == L and (rev == pm.decode(entry)[3]).all()
    assert f(None, 0, None, None, None, None, None, 0) == 0
    assert all(len(x.ravel()) == 0 for x in api.profile_decode(b""))


@pytest.mark.parametrize("cut", (1, 24, 26, 25 * 40 - 1))
def test_a_length_that_is_no_multiple_of_the_record_size_is_refused(cut):
    entry = crafted_entries()["extremes"][:cut]
    with pytest.raises(pm.Damaged) as m:
        pm.decode(entry)
    assert m.value.kind == "length"
    with pytest.raises(api.FsgpuError) as e:
        api.profile_decode(entry)
    assert "not a multiple of the record size 25" in str(e.value) and str(cut) in str(e.value)


@pytest.mark.parametrize("byte, what", ((20, "query letter"), (21, "consensus letter")))
@pytest.mark.parametrize("value", (21, 255))
def test_a_letter_above_20_is_refused(byte, what, value):
    rec = np.frombuffer(crafted_entries()["extremes"], np.uint8).reshape(-1, pm.RECORD).copy()
    rec[17, byte] = value
    with pytest.raises(pm.Damaged) as m:
        pm.decode(rec.tobytes())
    assert m.value.kind == "letter"
    codes = np.full(len(rec), 99, np.uint8)
    err = C.create_string_buffer(200)
    rc = api.lib().fshost_profile_decode(api._ptr(rec), rec.size, api._ptr(codes), None, None, None, err, len(err))
    assert rc < 0 and (codes == 99).all(), "a refused entry writes nothing"
    assert f"{what} at position 17 is {value}, above 20" in err.value.decode()
    with pytest.raises(api.FsgpuError):
        api.profile_decode(rec.tobytes())


def test_new_symbols_in_the_library_and_the_binding():
    L = api.lib()
    for sym in ("fsgpu_sw_multi_dir_p", "fsgpu_sw_multi_p", "fshost_profile_decode", "fshost_profile_bias"):
        assert getattr(L, sym).argtypes is not None, sym
    assert {"fsgpu_sw_multi_dir_p", "fsgpu_sw_multi_p"} <= set(api.exported_symbols())
    assert callable(api.Context.sw_multi_dir_p) and callable(api.Context.sw_multi_p)


# ---- the frozen reference runs (tests/golden/profile_v1, generator tests/golden/make_profile_golden.py) -------------------------------------------------
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "profile_v1")
BIN = os.path.join(os.path.dirname(api.LIB_PATH), "bin", "fsgpu-modules")
LETTERS = "ACDEFGHIKLMNPQRSTVWYX"


def read_db(name):
    data = open(os.path.join(GOLD, name), "rb").read()
    out = {}
    for line in open(os.path.join(GOLD, name + ".index")):
        k, off, ln = line.split()
        out[int(k)] = data[int(off):int(off) + int(ln) - 1]
    return out


def seq_db(name):
    """{key: codes} of a sequence database; lower-case (soft-masked) letters keep their letter here"""
    return {k: np.array([LETTERS.index(chr(c).upper()) if chr(c).upper() in LETTERS else 20 for c in v.rstrip(b"\n")], np.uint8) for k, v in read_db(name).items()}


class _Db:
    """the PaddedDB-like view tests/gapless_model.py reads"""
    def __init__(self, seqs):
        self.keys = sorted(seqs)
        self.lengths = np.array([len(seqs[k]) for k in self.keys], np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths)])[:-1]
        self.data3di = np.concatenate([seqs[k] for k in self.keys]) if self.keys else np.zeros(0, np.uint8)


@pytest.mark.parametrize("query, target, frozen", (("profile_0_ss", "db_ss", "ppref"), ("cprof_ss", "ctarget_ss", "cpref")))
def test_model_equals_every_frozen_prefilter_record(query, target, frozen):
    """hit lists, scores and order of the reference's ungappedprefilter with a profile query: the pssm is the decoded profile, the cap 255 - bias"""
    run = json.load(open(os.path.join(GOLD, "MANIFEST.json")))["runs"][frozen]
    par = run["parameters"]
    min_score, max_res = int(par[par.index("--min-ungapped-score") + 1]), int(par[par.index("--max-seqs") + 1])
    db = _Db(seq_db(target))
    want = read_db(frozen)
    profiles = read_db(query)
    assert sorted(want) == sorted(profiles)
    for key, entry in profiles.items():
        _, _, prof, _ = pm.decode(entry)
        hits = gm.select(pm.gapless_scores(prof, db), min_score, -1, max_res)
        text = "".join(f"{db.keys[int(h['id'])]}\t{int(h['score'])}\t0\n" for h in hits)
        assert text == want[key].decode(), (frozen, key)


_WORLDS = {}


def _world(query, target, cov_thr, cov_mode):
    """one ProfileWorld per (databases, coverage rule): the runs of a query database share its Smith-Waterman records and trace-backs"""
    key = (query, target, cov_thr, cov_mode)
    if key not in _WORLDS:
        tA, t3 = seq_db(target), seq_db(target + "_ss")
        keys = sorted(t3)
        W = pm.ProfileWorld([(tA[k], t3[k]) for k in keys], keys, cov_thr, cov_mode)
        base = _WORLDS.get((query, target))
        if base is not None:
            W._sw = base._sw                                                 # the records do not depend on the coverage rule
        _WORLDS.setdefault((query, target), W)
        _WORLDS[key] = W
    return _WORLDS[key]


_ALIGN_RUNS = sorted(n for n, r in json.load(open(os.path.join(GOLD, "MANIFEST.json")))["runs"].items() if r["module"] == "structurealign")


@pytest.mark.parametrize("frozen", _ALIGN_RUNS)
def test_model_equals_every_line_of_every_frozen_alignment_run(frozen):
    """tests/align_model.py's accept loop over a ProfileWorld (tests/profile_model.py: records from the tables, mu / lambda from the query letters,
    alignStartPosBacktrace<PROFILE> -- reverse-pass start cell, the no-cigar rule below the coverage threshold, the banded trace-back, the identity
    count) against the reference's result DB, whole entries: hit lists, scores, e-values, identities, start and end positions, backtraces, order.
    The run's own parameters are read from the generator's record: both alignment types, -a 0 and 1, the thresholds, --max-accept / --max-rejected,
    and the crafted profiles (one position, the extremes, the saturating one, 1025 positions)."""
    import align_model as am
    run = json.load(open(os.path.join(GOLD, "MANIFEST.json")))["runs"][frozen]
    par = run["parameters"]
    get = lambda flag: par[par.index(flag) + 1]  # noqa: E731
    q, t, pref = run["positional"]
    P = am.params(evalThr=float(get("-e")), covThr=float(get("-c")), covMode=int(get("--cov-mode")), seqIdThr=float(get("--min-seq-id")),
                  seqIdMode=int(get("--seq-id-mode")), alnLenThr=int(get("--min-aln-len")), maxAccept=int(get("--max-accept")),
                  maxRejected=int(get("--max-rejected")), altAlignment=int(get("--alt-ali")))
    W = _world(q, t, P["covThr"], P["covMode"])
    index_of = {int(k): i for i, k in enumerate(W.keys)}
    pA, p3, want = read_db(q), read_db(q + "_ss"), read_db(frozen)
    with_bt = int(get("-a")) != 0
    n = 0
    for key, body in sorted(read_db(pref).items()):
        hits = [index_of[int(l.split("\t")[0])] for l in body.decode().splitlines()]
        text = ""
        if hits:
            qa, q3 = W.add_query(pA[key], p3[key])
            res = am.align_query(W, qa, q3, hits, P, identity=-1)
            text = "".join(am.line(rec, cig if with_bt else None) + "\n" for rec, cig in zip(res.records, res.cigars))
            n += len(res.records)
        assert text == want[key].decode(), (frozen, key)
    assert sorted(want) == sorted(read_db(pref)) and n == run["lines"]


# ---- refusals: by name, before a device is opened (this test runs without one) --------------------------------------------------------------------------
def _module(args):
    return subprocess.run([BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


@pytest.fixture()
def work(tmp_path):
    w = tmp_path / "profile"
    shutil.copytree(GOLD, w)
    return w


@pytest.mark.parametrize("args, words", (
    (["prefilter", "profile_0_ss", "db_ss", "out"], ("prefilter:", "profile database", "k-mer generator")),
    (["search", "profile_0", "db", "out", "--prefilter-mode", "0"], ("search:", "profile database", "k-mer generator", "--prefilter-mode 1")),
    (["search", "profile_0", "db", "out", "--prefilter-mode", "2"], ("search:", "profile database", "exhaustive")),
    (["search", "profile_0", "db", "out", "--exhaustive-search", "1"], ("search:", "profile database", "exhaustive")),
    (["search", "profile_0", "db", "out", "--prefilter-mode", "1", "--alt-ali", "1"], ("search:", "profile database", "--alt-ali")),
    (["structurealign", "profile_0", "db", "ppref", "out", "--alt-ali", "2"], ("structurealign:", "profile database", "--alt-ali")),
    (["structurerescorediagonal", "profile_0", "db", "ppref", "out"], ("structurerescorediagonal:", "profile database")),
    (["ungappedprefilter", "profile_0_ss", "db_ss", "out", "--gpu-server", "1"], ("ungappedprefilter:", "profile database", "gpuserver")),
))
def test_modules_refuse_by_name_what_they_do_not_do_with_a_profile_query(work, args, words):
    names = {"profile_0", "profile_0_ss", "db", "db_ss", "ppref", "out"}
    r = _module([str(work / a) if a in names else a for a in args])
    assert r.returncode != 0 and all(w in r.stderr for w in words), r.stderr
    assert "HIP" not in r.stderr and "GPU" not in r.stderr, "refused before a device is opened"
    assert not os.path.exists(work / "out") and not os.path.exists(work / "out.index")


def test_one_profile_database_of_the_two_is_refused(work):
    for ext in ("", ".index", ".dbtype"):
        shutil.copy(work / ("db_ss" + ext), work / ("half_ss" + ext))
        shutil.copy(work / ("profile_0" + ext), work / ("half" + ext))
    for module, args in (("structurealign", [str(work / "half"), str(work / "db"), str(work / "ppref"), str(work / "out")]),
                         ("search", [str(work / "half"), str(work / "db"), str(work / "out"), "--prefilter-mode", "1"])):
        r = _module([module] + args)
        assert r.returncode != 0 and "only one of" in r.stderr and "both must be" in r.stderr, r.stderr
