"""Every instantiation of the profile path's kernels -- k_sw<R, HAS_AA, Pk16>, k_sw<R, HAS_AA, I32> and k_sw2<R, HAS_AA>, R in {1, 2, 3, 4, 6, 8}: 36
kernels -- against tests/sw_model.py on the world of tests/sw_prof_cases.py, exactly: score, qEnd, dbEnd and word of every pair, no pair skipped,
through fsgpu_sw_batch, fsgpu_sw_batch_seqs, fsgpu_sw_multi_dir (both directions, with selections) and fsgpu_sw_multi.  Which kernels a call launched
is read from Context.sw_kernel_counts(): a call may move the slots of its own class and AA setting only, and the sweep moves all 36.
tests/test_sw_prof_cases.py asserts on the CPU what the world holds for each of them."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sw_prof_cases as K
from foldseek_amd import api

pytestmark = pytest.mark.gpu
FIELDS = ("score", "qEnd", "dbEnd", "word")
CASES = [(R, aa) for R in K.CLASSES for aa in (True, False)]
IDS = [f"{R}-{'aa' if aa else '3di'}" for R, aa in CASES]
PK16, I32, SW2 = 0, 1, 2


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    c.load_db(K.db())
    yield c
    c.close()


def same(got, want, what, q):
    """every pair of one query: on a mismatch the class, L, the target's length and both records"""
    tl = K.db().lengths[q.ids.astype(np.int64)]
    bad = [k for k in range(len(want)) if any(int(got[k][f]) != int(want[k][f]) for f in FIELDS)]
    assert len(got) == len(want) and not bad, \
        (what, q.name, f"class R={q.cls} L={q.L} gaps {q.go}/{q.ge}", f"{len(bad)} of {len(want)} pairs differ",
         [(k, f"target of {int(tl[k])}", "device", tuple(int(got[k][f]) for f in FIELDS), "model", tuple(int(want[k][f]) for f in FIELDS)) for k in bad[:6]])


def members(R, aa, long=False):
    return [q for q in K.world() if q.aa == aa and ((q.kind == "long") if long else (q.cls == R and q.kind != "long"))]


def api_q(q):
    return (q.pAf, q.p3f, q.pAr, q.p3r, q.L, q.ids)


class Moved:
    """the slots of sw_kernel_counts() that a block of calls moved"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.before = self.ctx.sw_kernel_counts()
        return self

    def __exit__(self, *exc):
        after = self.ctx.sw_kernel_counts()
        self.slots = {k for k in after if after[k] != self.before[k]}
        assert all(after[k] >= self.before[k] for k in after)


def saturates(q):
    return bool((K.want(q, 0)["word"] == 2).any() or (K.want(q, 1)["word"] == 2).any())


# ---- one query per call -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,aa", CASES, ids=IDS)
def test_sw_batch(ctx, R, aa):
    qs = members(R, aa)
    assert {q.sec for q in qs} == {"a", "b", "c"}
    for q in qs:
        with Moved(ctx) as m:
            f, r = ctx.sw_batch(q.pAf, q.p3f, q.pAr, q.p3r, q.ids, q.go, q.ge)
        same(f, K.want(q, 0), "sw_batch fwd", q)
        same(r, K.want(q, 1), "sw_batch rev", q)
        assert m.slots == ({(PK16, aa, R), (I32, aa, R)} if saturates(q) else {(PK16, aa, R)}), (q.name, m.slots)


@pytest.mark.parametrize("R,aa", CASES, ids=IDS)
def test_sw_batch_seqs_targets_back_to_back(ctx, R, aa):
    d = K.db()
    odd = 0
    for q in members(R, aa):
        t3, tA = K.targets(q)
        odd += int((np.cumsum([len(t) for t in t3])[:-1] % 2 == 1).sum())
        with Moved(ctx) as m:
            f, r = ctx.sw_batch_seqs(q.pAf, q.p3f, q.pAr, q.p3r, tA if aa else None, t3, q.go, q.ge)
        same(f, K.want(q, 0), "sw_batch_seqs fwd", q)
        same(r, K.want(q, 1), "sw_batch_seqs rev", q)
        assert m.slots == ({(PK16, aa, R), (I32, aa, R)} if saturates(q) else {(PK16, aa, R)}), (q.name, m.slots)
    assert odd >= 10 and d.n > 0                    # unpadded, back to back: targets start at odd offsets


# ---- several queries per call -----------------------------------------------------------------------------------------------------------------------
def gap_groups(qs):
    out = {}
    for q in qs:
        out.setdefault((q.go, q.ge), []).append(q)
    return out


def multi_dir(ctx, qs, what):
    """both directions of one call's queries (one gap-cost setting): all pairs, then two selections that cut through the saturated pairs"""
    go, ge = qs[0].go, qs[0].ge
    for d in (0, 1):
        got = ctx.sw_multi_dir([api_q(q) for q in qs], d, gap_open=go, gap_extend=ge)
        for q, g in zip(qs, got):
            same(g, K.want(q, d), (what, "sw_multi_dir", d), q)
    cut = 0
    for part in (0, 1):
        sel = [np.arange(part, len(q.ids), 2, dtype=np.int32) if (i + part) % 3 else np.zeros(0, np.int32) for i, q in enumerate(qs)]
        for d in (0, 1):
            got = ctx.sw_multi_dir([api_q(q) for q in qs], d, selections=sel, gap_open=go, gap_extend=ge)
            for q, g, s in zip(qs, got, sel):
                w = K.want(q, d)
                mask = np.zeros(len(w), bool); mask[s] = True
                for k in np.flatnonzero(mask):
                    assert tuple(int(g[k][f]) for f in FIELDS) == tuple(int(w[k][f]) for f in FIELDS), \
                        (what, "selected", q.name, f"class R={q.cls} L={q.L}", int(k), int(K.db().lengths[int(q.ids[k])]), "device", g[k], "model", w[k])
                assert not g[~mask].tobytes().strip(b"\0"), (what, q.name, "unselected entries written")
                cut += int(len(s) > 0 and (w["word"][mask] == 2).any() and (w["word"][~mask] == 2).any())
    return cut


@pytest.mark.parametrize("R,aa", CASES, ids=IDS)
def test_sw_multi_dir_class_by_class(ctx, R, aa):
    cut = 0
    for (go, ge), qs in gap_groups(members(R, aa)).items():
        with Moved(ctx) as m:
            cut += multi_dir(ctx, qs, f"class {R}")
        allowed = {(SW2, aa, R), (PK16, aa, R), (I32, aa, R)}
        assert (SW2, aa, R) in m.slots and m.slots <= allowed and ((go, ge) != (10, 1) or m.slots == allowed), ((go, ge), m.slots)
    assert cut >= 4                                  # selections with saturated pairs on both sides of the cut


@pytest.mark.parametrize("R,aa", CASES, ids=IDS)
def test_sw_multi(ctx, R, aa):
    for (go, ge), qs in gap_groups(members(R, aa)).items():
        with Moved(ctx) as m:
            f, r = ctx.sw_multi([api_q(q) for q in qs], go, ge)
        for q, gf, gr in zip(qs, f, r):
            same(gf, K.want(q, 0), "sw_multi fwd", q)
            same(gr, K.want(q, 1), "sw_multi rev", q)
        assert m.slots <= {(SW2, aa, R), (PK16, aa, R), (I32, aa, R)} and (SW2, aa, R) in m.slots, m.slots


@pytest.mark.parametrize("aa", (True, False), ids=["aa", "3di"])
def test_row_tiles_saturating(ctx, aa):
    """513 and 1025 rows: two and three row tiles of R = 8, re-run in int32 with borders between the tiles"""
    qs = members(8, aa, long=True)
    assert [q.L for q in qs] == [513, 1025] and all(saturates(q) for q in qs)
    with Moved(ctx) as m:
        for q in qs:
            f, r = ctx.sw_batch(q.pAf, q.p3f, q.pAr, q.p3r, q.ids, q.go, q.ge)
            same(f, K.want(q, 0), "sw_batch fwd", q)
            same(r, K.want(q, 1), "sw_batch rev", q)
            t3, tA = K.targets(q)
            f, r = ctx.sw_batch_seqs(q.pAf, q.p3f, q.pAr, q.p3r, tA if aa else None, t3, q.go, q.ge)
            same(f, K.want(q, 0), "sw_batch_seqs fwd", q)
            same(r, K.want(q, 1), "sw_batch_seqs rev", q)
        multi_dir(ctx, qs, "row tiles")
        f, r = ctx.sw_multi([api_q(q) for q in qs])
        for q, gf, gr in zip(qs, f, r):
            same(gf, K.want(q, 0), "sw_multi fwd", q)
            same(gr, K.want(q, 1), "sw_multi rev", q)
    assert m.slots == {(PK16, aa, 8), (I32, aa, 8)}, m.slots


def test_all_classes_in_one_call_and_all_36_kernels(ctx):
    """one sw_multi_dir call per AA setting and direction over every query of the world at 10 / 1, row-tiled ones included: every class's k_sw2, and
    through the re-run of the saturated pairs every class's k_sw in int16 and in int32"""
    before = ctx.sw_kernel_counts()
    assert len(before) == 36
    for aa in (True, False):
        qs = [q for q in K.world() if q.aa == aa and (q.go, q.ge) == (10, 1)]
        assert {q.cls for q in qs} == set(K.CLASSES) and len(qs) >= 70
        with Moved(ctx) as m:
            cut = multi_dir(ctx, qs, "all classes")
        assert m.slots == {(kind, aa, R) for kind in (PK16, I32, SW2) for R in K.CLASSES}, m.slots
        assert cut >= 12
    after = ctx.sw_kernel_counts()
    assert all(after[k] > before[k] for k in after), {k: after[k] - before[k] for k in after}
    # counters only: a clone starts at zero and leaves its parent's alone
    c = ctx.clone()
    try:
        assert not any(c.sw_kernel_counts().values())
        q = members(2, True)[0]
        c.sw_batch(q.pAf, q.p3f, q.pAr, q.p3r, q.ids, q.go, q.ge)
        assert c.sw_kernel_counts()[(PK16, True, 2)] == 1 and sum(c.sw_kernel_counts().values()) == 1 and ctx.sw_kernel_counts() == after
    finally:
        c.close()


# ---- FSGPU_SW2_PAIRS: read once per process, so each setting runs in a child --------------------------------------------------------------------------
CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import sw_prof_cases as K
from foldseek_amd import api
ctx = api.Context(0)
ctx.load_db(K.db())
bad = 0
for R in (1, 6):
    qs = [q for q in K.section("a") if q.cls == R and q.aa and (q.go, q.ge) == (10, 1)]
    assert len(qs) >= 4
    before = ctx.sw_kernel_counts()
    for d in (0, 1):
        got = ctx.sw_multi_dir([(q.pAf, q.p3f, q.pAr, q.p3r, q.L, q.ids) for q in qs], d)
        for q, g in zip(qs, got):
            w = K.want(q, d)
            for k in range(len(w)):
                if tuple(int(g[k][f]) for f in ("score", "qEnd", "dbEnd", "word")) != tuple(int(w[k][f]) for f in ("score", "qEnd", "dbEnd", "word")):
                    bad += 1
                    print("differs:", q.name, "class", R, "L", q.L, "dir", d, "pair", k, "target of", int(K.db().lengths[int(q.ids[k])]), "device", g[k], "model", w[k])
    after = ctx.sw_kernel_counts()
    if {k for k in after if after[k] != before[k]} != {(2, True, R)}:
        bad += 1
        print("kernels moved:", {k: after[k] - before[k] for k in after if after[k] != before[k]})
ctx.close()
sys.exit(1 if bad else 0)
"""


@pytest.mark.parametrize("pairs", (16, 32))
def test_sw2_pairs_per_workgroup(pairs):
    """section (a)'s 3Di + AA calls of classes 1 and 6 with 16 and 32 pairs per workgroup (8 and 16 waves share one LDS image)"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, FSGPU_SW2_PAIRS=str(pairs))
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(here)] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    p = subprocess.run([sys.executable, "-c", CHILD, here], env=env, cwd=os.path.dirname(here), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (pairs, p.returncode, p.stdout[-3000:], p.stderr[-3000:])
