"""The frozen long cases of the block aligner (tests/golden/ba_long/long_cases.txt.gz, long_model.txt; generator: oracle/ba_kat/make_long_cases.py) and the inputs
tests/test_btrace_model_gpu.py builds from them, checked without a GPU: the frozen answers are the independent model's (tests/ba_model.py), the host
restatement (host/block_aligner.cpp through oracle/ba_kat/ba_kat.cpp) agrees with every one of them -- 1000 residues and more, block sizes up to 1024 --,
the classes the device test needs are present in the numbers the generator promised, and the matrix tables handed to the device are the ones the host
code builds."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import btrace_cases as B
from btrace_cases import G
from foldseek_amd import api

STRIDE = 9          # every 9th long case goes through the model again: 42 of 378, about a minute of Python


def _model_line(case_line):
    name, go, ge, qa, q3, qbias, ta, t3, target = G.parse_case(case_line)
    fA, _ = G.load_matrix(os.path.join(B.KAT, "mat_aa.txt"))
    f3, _ = G.load_matrix(os.path.join(B.KAT, "mat_3di.txt"))
    attempts, res, cigar = G.ladder(qa, q3, qbias, ta, t3, go, ge, target, fA, f3)
    return G.answer_line(name, res, cigar, attempts), G.classify(attempts, target), max(a[2] for a in attempts)


def _check_subset(offset):
    lines = B.long_lines()
    frozen = open(os.path.join(B.LONG, "long_model.txt")).read().splitlines()
    n = 0
    for k in range(offset, len(lines), 2 * STRIDE):
        got, cls, largest = _model_line(lines[k])
        assert got == frozen[k], (k, got[:200], frozen[k][:200])
        assert (cls, largest) == G.name_info(lines[k].split()[1])[:2], (k, cls, largest, lines[k].split()[1])
        n += 1
    return n


def test_frozen_long_answers_are_the_models_even_half():
    """BlockModel again on every 18th long case from the first on: the frozen line (score, end cell, CIGAR, block sizes tried) and the class and largest
    block in the case's name are what the model says"""
    assert _check_subset(0) >= 20


def test_frozen_long_answers_are_the_models_odd_half():
    """... and from the 10th on: together every 9th case, at least 40"""
    assert _check_subset(STRIDE) >= 20
    assert len(range(0, len(B.long_lines()), STRIDE)) >= 40


def test_restatement_agrees_with_the_model_on_all_long_cases(tmp_path):
    """host/block_aligner.cpp through oracle/ba_kat/ba_kat.cpp over ALL long cases against the model's frozen answers, line for line: the host-side
    check now reaches past 1000 residues and through the retry ladder up to starting size 1024"""
    for fn in ("mat_aa.txt", "mat_3di.txt"):
        shutil.copy(os.path.join(B.KAT, fn), tmp_path / fn)
    lines = B.long_lines()
    (tmp_path / "cases.txt").write_text("".join(lines))
    exe = str(tmp_path / "ba_kat_ours")
    host = os.path.join(B.ROOT, "foldseek_amd", "csrc", "host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-mavx2", "-mfma", "-I" + host, "-o", exe, os.path.join(B.KAT, "ba_kat.cpp"), os.path.join(host, "block_aligner.cpp")])
    ours = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    frozen = open(os.path.join(B.LONG, "long_model.txt")).read().splitlines()
    assert len(ours) == len(frozen) == len(lines)
    bad = [(a[:200], b[:200]) for a, b in zip(ours, frozen) if a != b]
    assert not bad, (len(bad), bad[:3])
    assert max(len(ln.split()[4]) for ln in lines) >= 1000


def test_census_of_the_frozen_long_cases():
    """the classes the device test relies on are there: conditions on the inputs that the model alone decided"""
    cases = B.long_cases()
    c = G.census([(x.name, x.attempts, min(len(x.rqa), len(x.rta))) for x in cases])
    assert all(c[k] >= G.MINIMA[k] for k in G.MINIMA), c
    for x in cases:
        assert (x.score != x.target) == bool(x.lowered), x.name                    # the lowered requests, and only they, are overshot
        assert x.score >= x.target and (not x.lowered or x.cls in "AB"), x.name
        if x.cls == "A":
            assert x.attempts <= 3 and x.largest <= 128, x.name
        if x.cls == "B":
            assert x.attempts <= 5 and 128 < max(x.largest, 32 << (x.attempts - 1)) and x.largest <= 512, x.name
        if x.cls == "C":
            assert x.attempts > 5 or x.largest > 512, x.name
    for fn in (os.path.join(B.LONG, "long_cases.txt.gz"), os.path.join(B.LONG, "long_model.txt"), os.path.join(B.KAT, "cases_classes.txt")):
        assert os.path.getsize(fn) < 1000000, fn
    # the short cases (cases.txt): every one has a class, and the answers they are held to reach the requested score
    short = B.short_cases()
    assert len(short) == 586 and all(x.score == x.target for x in short)


def test_device_tables_equal_the_host_codes():
    """the [27][32] tables and letter maps the GPU test hands to fsgpu_block_backtrace, built in numpy from the matrix files, against what
    block_new_simple_aamatrix + block_set_aamatrix leave behind (search.cpp fills the device's tables exactly so): byte for byte"""
    L = C.CDLL(api.LIB_PATH)
    L.block_new_simple_aamatrix.restype = C.c_void_p
    L.block_new_simple_aamatrix.argtypes = [C.c_int8, C.c_int8]
    L.block_set_aamatrix.argtypes = [C.c_void_p, C.c_uint8, C.c_uint8, C.c_int8]
    L.block_aamatrix_scores.restype = C.POINTER(C.c_int8)
    L.block_aamatrix_scores.argtypes = [C.c_void_p]
    L.block_free_aamatrix.argtypes = [C.c_void_p]
    tA, t3, lA, l3 = B.device_tables()
    for fn, mine in (("mat_aa.txt", tA), ("mat_3di.txt", t3)):
        letters, m = B.matrix_text(os.path.join(B.KAT, fn))
        assert letters == B.LETTERS
        h = L.block_new_simple_aamatrix(1, -1)
        for a in range(len(letters)):
            for b in range(len(letters)):
                L.block_set_aamatrix(h, ord(letters[a]), ord(letters[b]), int(m[a, b]))
        theirs = np.ctypeslib.as_array(L.block_aamatrix_scores(h), (27 * 32,)).copy()
        L.block_free_aamatrix(h)
        assert mine.dtype == np.int8 and mine.shape == (27, 32)
        assert mine.tobytes() == theirs.tobytes(), fn
    assert lA.dtype == np.uint8 and lA.tolist() == l3.tolist() == [ord(c) - ord("A") for c in "ACDEFGHIKLMNPQRSTVWYX"]


def test_block_backtrace_entry_points_are_bound():
    """fsgpu_block_backtrace, its footprint switch and fsgpu_live_devices are in the ctypes table and in the list of exported symbols; the structures have
    the C layout of include/fsgpu.h"""
    L = api.lib()
    names = api.exported_symbols()
    for fn in ("fsgpu_block_backtrace", "fsgpu_block_backtrace_footprint", "fsgpu_live_devices"):
        assert fn in names and getattr(L, fn).argtypes is not None, fn
    for fn in names:
        assert hasattr(L, fn), fn
    assert (C.sizeof(api.BtQuery), C.sizeof(api.BtTask), C.sizeof(api.BtRes)) == (40, 20, 32)
    assert api.BtRes.btOff.offset == 24 and api.BtQuery.L.offset == 32
    assert 0 <= L.fsgpu_live_devices() <= 64               # (a counter of this process: callable without a device)
