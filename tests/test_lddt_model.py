"""LDDT without a GPU: the independent float32 model (tests/lddt_model.py) against what the REFERENCE BINARY printed and decided (tests/golden/ca_v1,
generator tests/golden/make_ca_golden.py), and the host pieces of this repository's LDDT path against the model.

  * every `lddt` and `lddtfull` value of the reference's convertalis on the 144 pairs of the 12 example structures and on the crafted database (raw-float
    entry, NaN columns, an alignment with no scored column, distances of exactly 15.0, |d| of exactly 0.5 / 1 / 2 / 4, pairs that tell the fused
    distance from the unfused one);
  * every --lddt-threshold decision of the reference's structurealign (0.5 / 0.7 / 0.8; one real pair sits at 0.49996, printed as 5.000E-01, and is dropped at 0.5);
  * fshost_ca_decode == the model's decoder on every frozen C-alpha entry, fshost_lddt_average == the model's average;
  * the new symbols and struct layouts in foldseek_amd/api.py.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lddt_cases as K
import lddt_model as M
from foldseek_amd import api

BIN = os.path.join(K.ROOT, "foldseek_amd", "bin", "fsgpu-modules")


def _check_text(db, aln, text_name):
    rows = [l.split("\t") for l in K.frozen_text(text_name).decode().splitlines()]
    recs, cols, nm = K.records(aln), K.model_columns(db, aln), K.names(db)
    assert len(rows) == len(recs) > 0
    for row, (q, t, qs, ts, cig), c in zip(rows, recs, cols):
        assert (row[0], row[1]) == (nm[q], nm[t])
        avg, n = M.average(c)
        assert row[3] == M.lddt_text(avg), (nm[q], nm[t], row[3], repr(avg))
        # with no scored column the reference prints the float in front of an empty array: frozen as 0.000
        assert row[4] == (M.lddtfull(c) if n > 0 else "0.000"), (nm[q], nm[t])
    return rows


def test_model_reproduces_reference_lddt_of_the_example_structures():
    rows = _check_text("db", "aln_l0", "conv_lddt.m8")
    assert len(rows) == 144


def test_model_reproduces_reference_lddt_of_the_crafted_database():
    rows = _check_text("cdb", "caln", "conv_crafted.m8")
    assert any(r[3] == "-NAN" for r in rows)                       # the alignment whose every column is isolated
    assert any(",0.000," in r[4] for r in rows)                    # a NaN column in the middle
    exact = [r for r in rows if (r[0], r[1], r[2]) == ("qexact", "texact", "7")][0]
    assert exact[4] == "0.750,0.625,0.375,0.125,0.000"             # |d| exactly 0.5 / 1 / 2 / 4 count 3 / 2 / 1 / 0 quarters; two columns at exactly 15.0 are NaN


def test_crafted_records_tell_the_fused_distance_from_the_unfused_one():
    C_ = K.coords("cdb")
    differ = 0
    for q, t, qs, ts, cig in K.records("caln"):
        if q != 6:
            continue
        a, b = M.columns(C_[q], C_[t], qs, ts, cig, True), M.columns(C_[q], C_[t], qs, ts, cig, False)
        differ += not K.same_bits(a, b)
    assert differ > 0
    # ... and the 12 example structures cannot
    Cdb = K.coords("db")
    for (q, t, qs, ts, cig), want in list(zip(K.records("aln_l0"), K.model_columns("db", "aln_l0")))[:12]:
        assert K.same_bits(M.columns(Cdb[q], Cdb[t], qs, ts, cig, False), want)


@pytest.mark.parametrize("name,thr", [("aln_l05", 0.5), ("aln_l07", 0.7), ("aln_l08", 0.8)])
def test_model_reproduces_reference_threshold_decisions(name, thr):
    """avgLddtScore < lddtThr compares a double with a float widened to double (structurealign.cpp:404)"""
    kept = {(q, t) for q, t, _, _, _ in K.records(name)}
    thr = float(np.float32(thr))
    mine = set()
    for (q, t, _, _, _), c in zip(K.records("aln_l0"), K.model_columns("db", "aln_l0")):
        if not M.average(c)[0] < thr:
            mine.add((q, t))
    assert mine == kept and len(kept) == K.MANIFEST["runs"][name]["lines"]
    if name == "aln_l05":
        dropped = {(q, t) for q, t, _, _, _ in K.records("aln_l0")} - kept
        assert dropped == {(1, 4)}
        avg = [M.average(c)[0] for (q, t, _, _, _), c in zip(K.records("aln_l0"), K.model_columns("db", "aln_l0")) if (q, t) == (1, 4)][0]
        assert 0.4999 < avg < 0.5 and M.lddt_text(avg) == "5.000E-01"


@pytest.mark.parametrize("db", ["db", "db_pad", "cdb"])
def test_ca_decode_equals_the_model_decoder(db):
    L = K.lengths(db if db != "db_pad" else "db_pad_ss")
    entries = K.read_db(db + "_ca")
    assert len(entries) >= 8
    for k, e in entries.items():
        for entry in (e, e + b"\0"):                               # as stored: with or without the terminator
            got = api.ca_decode(entry, L[k])
            assert got.tobytes() == M.decode(entry, L[k]).tobytes(), (db, k)
    with pytest.raises(api.FsgpuError):
        api.ca_decode(entries[min(entries)][:40], L[min(entries)])


def test_lddt_average_equals_the_model_average():
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 7, 150, 1000):
        c = rng.integers(0, 600, n).astype(np.float32) * np.float32(0.25) * (np.float32(1.0) / rng.integers(1, 60, n).astype(np.float32))
        for nan_every in (0, 3, 1):
            d = c.copy()
            if nan_every:
                d[::nan_every] = np.nan
            got, gn = api.lddt_average(d)
            want, wn = M.average(d)
            assert gn == wn
            assert np.float64(got).tobytes() == np.float64(want).tobytes() or (got != got and want != want and np.signbit(got) == np.signbit(want))
    assert M.lddt_text(api.lddt_average(np.zeros(0, np.float32))[0]) == "-NAN"


def test_api_mirrors_the_new_symbols_and_structs():
    assert "fsgpu_lddt_batch" in api.exported_symbols()
    L = api.lib()
    for sym in ("fsgpu_lddt_batch", "fshost_ca_decode", "fshost_lddt_average", "fshost_search_bind_ca", "fshost_search_set_query_ca"):
        assert hasattr(L, sym), sym
    assert C.sizeof(api.LddtQuery) == 16 and C.sizeof(api.LddtTask) == 48
    assert [f[0] for f in api.LddtTask._fields_] == ["query", "tLen", "tOff", "qStart", "dbStart", "btOff", "btLen", "reserved", "outOff"]
    assert api.LddtTask.outOff.offset == 40 and api.LddtTask.btOff.offset == 24 and api.LddtQuery.L.offset == 8
    assert hasattr(api.Context, "lddt_batch")
    p = api.Params()
    L.fshost_params_default(C.byref(p))
    assert C.sizeof(api.Params) == 80                              # the layout bench.py and the adapters share is unchanged


def test_modules_flag_handling_without_a_device(tmp_path):
    """structurerescorediagonal keeps refusing a non-zero --lddt-threshold with its own message; structurealign no longer refuses the flag at
    parse time (without a device it gets as far as opening one); both before anything is written"""
    pos = [os.path.join(K.GOLD, "db"), os.path.join(K.GOLD, "db"), os.path.join(K.GOLD, "pref"), str(tmp_path / "out")]
    r = subprocess.run([BIN, "structurerescorediagonal"] + pos + ["--lddt-threshold", "0.5"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "structurerescorediagonal: --lddt-threshold 0.5 is not implemented" in r.stderr
    r = subprocess.run([BIN, "structurealign"] + pos + ["--lddt-threshold", "1.5"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "Error in argument --lddt-threshold" in r.stderr
    r = subprocess.run([BIN, "convertalis", pos[0], pos[1], os.path.join(K.GOLD, "aln_l0"), str(tmp_path / "o.m8"), "--format-output", "query,qca"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "column qca is not implemented" in r.stderr
    assert not os.path.exists(tmp_path / "out.index") and not os.path.exists(tmp_path / "o.m8")
