"""Profile queries in the k-mer prefilter, without a device: the model of tests/kmer_profile_model.py against itself (the lexicographic claim the
device kernels rest on), the host functions against the model, and the frozen reference runs of tests/golden/profile_kmer_v1 (generator
tests/golden/make_profile_kmer_golden.py) against the conditions they were made for."""
import json
import os

import numpy as np
import pytest

import kmer_profile_model as km
import profile_model as pm
from foldseek_amd import api

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "profile_kmer_v1")
SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "profile_v1")
FOUND_DIAGONALS = 1000000          # QueryMatcher.cpp:44, max(1e6, targets)
MAX_DB_MATCHES = 2000000           # QueryMatcher.cpp:45


def read_db(path):
    data, out = open(path, "rb").read(), {}
    for line in open(path + ".index"):
        k, off, ln = line.split()
        out[int(k)] = data[int(off):int(off) + int(ln) - 1]
    return out


def manifest():
    return json.load(open(os.path.join(GOLD, "MANIFEST.json")))


def flag(par, name):
    return par[par.index(name) + 1]


def seeded_rows(rng, kind):
    if kind == 0:
        sc = rng.integers(-128, 128, (6, 20))                          # the whole range of a score byte
    elif kind == 1:
        sc = rng.choice(np.array([-7, 9]), (6, 20))                    # two-valued rows: ties everywhere
    elif kind == 2:
        sc = rng.choice(np.array([-128, 127]), (6, 20), p=[0.9, 0.1])  # the extremes
    elif kind == 3:
        sc = rng.integers(-3, 4, (6, 20))                              # a narrow range: many equal sums
    else:
        sc = np.full((6, 20), -60) + rng.integers(-8, 9, (6, 20))      # one favoured letter per row, like a real profile
        sc[np.arange(6), rng.integers(0, 20, 6)] = 70 + rng.integers(-8, 9, 6)
    return km.sort_rows(sc)


def test_the_literal_product_is_the_lexicographic_set():
    """generateKmerList's level-by-level product, with its per-level cap, gives exactly: all rank tuples with sum >= thr, in lexicographic order of the
    ranks, the first 8 388 607 of them -- on 2 400 seeded positions (ties, extremes, empty and one-element lists) and on the capped flat position"""
    rng = np.random.default_rng(20261103)
    sizes = []
    for k in range(2400):
        s, l = seeded_rows(rng, k % 5)
        top = int(s[:, 0].sum())
        mode = k % 7
        if mode == 0:
            thr = top + 1                                              # nothing reaches it
        elif mode == 1:
            thr = top                                                  # the all-top tuple, and its ties
        else:
            thr = top - int(rng.integers(1, 13))
            while km.count_ge(s, thr) > 20000:                         # (keeps the test quick; the capped case is the flat position below)
                thr += 1
        thr = km.window_threshold(thr)
        lit, lex = km.generate_literal(s, l, thr), km.generate_lex(s, l, thr)
        assert len(lit) == len(lex) == min(km.count_ge(s, thr), km.CAP), (k, thr)
        assert (lit == lex).all(), (k, thr)
        assert len(set(lit.tolist())) == len(lit), k                  # a k-mer appears once
        sizes.append(len(lit))
    sizes = np.array(sizes)
    assert (sizes == 0).sum() >= 100 and (sizes == 1).sum() >= 50 and (sizes > 1000).sum() >= 50, np.bincount(np.minimum(sizes, 3))
    # the flat position: all 64e6 tuples pass, every level is cut at the cap
    s, l = km.sort_rows(np.full((6, 20), 20))
    lit, lex = km.generate_literal(s, l, 75), km.generate_lex(s, l, 75)
    assert len(lit) == km.CAP == 8388607 and km.count_ge(s, 75) == 20 ** 6 and (lit == lex).all()
    # an all-equal row comes out of the network untouched; the first tuples vary the LAST row fastest
    assert (l == np.arange(20)).all() and (lit[:3] == [0, 20 ** 5, 2 * 20 ** 5]).all()


def test_the_sorting_network_is_not_stable_and_the_library_restates_it():
    rng = np.random.default_rng(7)
    sc = np.concatenate([rng.integers(-2, 3, (400, 20)), rng.integers(-128, 128, (200, 20)), rng.choice(np.array([-128, 127]), (100, 20))]).astype(np.int8)
    ms, ml = km.sort_rows(sc)
    assert (np.diff(ms.astype(np.int32), axis=1) <= 0).all() and (np.sort(ml, axis=1) == np.arange(20)).all()
    assert (np.take_along_axis(sc.astype(np.int16), ml.astype(np.int64), 1) == ms).all()
    stable = np.argsort(-sc.astype(np.int32), axis=1, kind="stable")
    assert (stable != ml).any(), "ties are left where the network leaves them, which is not letter order"
    gs, gl = api.kmer_profile_sort_rows(sc)
    assert (gs == ms).all() and (gl == ml).all()


@pytest.mark.parametrize("context", [False, True])
def test_threshold_rule(context):
    for k in (5, 6, 7):
        for s in np.arange(1.0, 10.01, 0.1):
            assert api.kmer_threshold_profile(float(np.float32(s)), k, context) == km.kmer_threshold(float(np.float32(s)), k, context), (k, s)
    assert api.kmer_threshold_profile(9.5, 4, context) == -1
    assert km.kmer_threshold(9.5, 6, True) == 49 and km.kmer_threshold(9.5, 6, False) == 75 and km.kmer_threshold(4, 6, False) == 109
    assert km.kmer_threshold(9.5, 6, False, k_score=-5) == -5 and km.window_threshold(-5) == 0 and km.window_threshold(1000) == 1000


def entries():
    out = list(read_db(os.path.join(GOLD, "kprof_ss")).values()) + list(read_db(os.path.join(SRC, "profile_0_ss")).values())
    rng = np.random.default_rng(11)
    for L in (0, 1, 9, 10, 37):
        out.append(pm.encode(rng.integers(-128, 128, (20, L)).astype(np.int8), rng.integers(0, 21, L)))
    return out


def test_raw_decode_and_prepare_against_the_model():
    for e in entries():
        codes, cons, prof, rev, raw = api.profile_decode_raw(e)
        c0, k0, p0, r0 = pm.decode(e)
        assert (codes == c0).all() and (cons == k0).all() and (prof == p0).all() and (rev == r0).all()
        assert raw.dtype == np.int8 and (raw == km.raw_scores(e)).all()
        for spaced in (0, 1):
            for thr in (75, -5, 1000):
                seq, rows, ungapped, t = api.kmer_query_prepare_profile(e, thr, 6, spaced)
                assert (seq == km.letters(e)).all() and (rows == km.raw_scores(e)).all() and (ungapped == km.ungapped_profile(e)).all()
                assert t == km.window_threshold(thr)
        if len(codes):
            assert not km.ungapped_profile(e)[:, 20].any() and km.QUERY_BIAS == 0
    with pytest.raises(api.FsgpuError):
        api.kmer_query_prepare_profile(entries()[0], 75, 7, 1)
    with pytest.raises(api.FsgpuError):
        api.profile_decode_raw(entries()[0][:-1])


def test_windows_and_the_x_rule():
    e = read_db(os.path.join(GOLD, "ksmall_ss"))
    note = manifest()["crafted"]["ksmall_ss"]
    for k, what in note.items():
        codes = km.letters(e[int(k)])
        if "offset" in what:
            o = int(what.rsplit(" ", 1)[1])
            assert codes[o] == 20 and len(codes) == 10
            assert km.windows(codes, 1) == [(0, o in km.pattern(1))]                       # the four unused offsets of the spaced pattern do not count
            assert [x for _, x in km.windows(codes, 0)] == [i <= o < i + 6 for i in range(5)]
        else:
            L = int(what.split()[1])
            assert len(km.windows(codes, 1)) == max(0, L - 9) and len(km.windows(codes, 0)) == max(0, L - 5)
    assert km.pattern(1) == [0, 1, 3, 5, 8, 9] and km.pattern(0) == [0, 1, 2, 3, 4, 5]


def test_manifest_conditions():
    m = manifest()
    runs = m["runs"]
    assert {"e_s95", "e_s4", "e_nospace", "e_diag0", "e_max5", "c_s95", "c_s4", "c_nospace", "c_diag0", "c_max5", "c_k60", "c_khuge", "c_kneg"} <= set(runs)
    for name, r in runs.items():
        assert r["index_kmer_threshold"] == 0, name                                      # Prefiltering.cpp:555-557
        if r["expect_empty"]:
            assert r["lines"] == 0 and r["kmers_per_pos"] == 0 and r["kmer_threshold"] > 6 * 127, name
        else:
            assert r["queries_with_hits"] >= 1 and r["lines"] >= 1, name                 # every setting has a query with hits
        assert r["overflows"] == 0, name                                                 # no query refills databaseHits
        assert r["targets"] < FOUND_DIAGONALS // 2, name                                 # result size < foundDiagonalsSize / 2: never the unstable std::sort
    assert [n for n, r in runs.items() if r["expect_empty"]] == ["c_khuge"]
    # the cap: the flat query's one window has MAX_KMER_RESULT_SIZE - 1 similar k-mers (the module prints k-mers per position = that / L, 6 decimals)
    flat = m["flat"]
    assert abs(flat["kmers_per_pos"] * flat["length"] - km.CAP) < 1e-4 and flat["overflows"] == 0
    # the truncated-score rescoring ran: with --max-seqs 5, queries with at least 5 targets at 255 or above
    assert runs["c_max5"]["truncated_queries"] and runs["e_max5"]["truncated_queries"]
    for name in ("c_max5", "e_max5"):
        res = read_db(os.path.join(GOLD, name))
        for q in runs[name]["truncated_queries"]:
            scores = [int(l.split("\t")[1]) for l in res[q].decode().splitlines()]
            assert len(scores) == 5 and min(scores) >= 255, (name, q)


def test_model_thresholds_equal_the_printed_ones():
    m = manifest()
    seen = set()
    for name, r in m["runs"].items():
        par = r["parameters"]
        qdb = r["positional"][0]
        where = SRC if qdb == "profile_0_ss" else GOLD
        dbtype = int.from_bytes(open(os.path.join(where, qdb + ".dbtype"), "rb").read()[:4], "little")
        assert dbtype & 0xffff == 2
        context = bool((dbtype >> 16) & 0x7FFE & 4)
        ks = int(flag(par, "--k-score").split("prof:")[1])
        want = km.kmer_threshold(float(flag(par, "-s")), int(flag(par, "-k")), context, None if ks == 2147483647 else ks)
        assert want == r["kmer_threshold"], name
        assert want == (ks if ks != 2147483647 else api.kmer_threshold_profile(float(flag(par, "-s")), 6, context)), name
        seen.add((context, ks != 2147483647, flag(par, "-s")))
    assert {(False, False, "9.5"), (False, False, "4"), (True, False, "9.5"), (False, True, "9.5")} <= seen


def test_the_model_reproduces_the_printed_kmers_per_position():
    """the module prints (similar k-mers of the run) / (sum of query lengths): the model's lists, counted, give the same figure for the small runs"""
    m = manifest()
    for name in ("c_small", "c_small_nospace", "c_kneg"):
        r = m["runs"][name]
        spaced = int(flag(r["parameters"], "--spaced-kmer-mode"))
        db = read_db(os.path.join(GOLD, r["positional"][0]))
        total = per = 0.0
        for k in sorted(db):
            s, l = km.sort_rows(km.raw_scores(db[k]))
            n = sum(min(km.count_ge(km.position_rows(s, l, st, spaced)[0], km.window_threshold(r["kmer_threshold"])), km.CAP)
                    for st, x in km.windows(km.letters(db[k]), spaced) if not x)
            per += n / len(km.letters(db[k])); total += 1
        assert abs(per / total - r["kmers_per_pos"]) < 1e-3 * max(1.0, r["kmers_per_pos"]), (name, per / total, r["kmers_per_pos"])
