"""--tmscore-threshold, --sort-by-structure-bits 1 and the alntmscore / qtmscore / ttmscore / rmsd columns at module level, on REFERENCE-WRITTEN databases with
a C-alpha database (tests/golden/ca_v1) against the reference's outputs frozen in tests/golden/tm_v1 (generator tests/golden/make_tm_golden.py):
`fsgpu-modules` runs with the positional arguments and the complete parameter strings the reference binary was run with, and every entry of every result
DB / every byte of the text output must be the reference's.  Under structure bits the TM-score and the LDDT show in the SCORE column and in the order of a
query's hits; a threshold shows in which hits survive (144 / 128 / 103 / 99 / 72 lines)."""
import os
import shutil
import subprocess

import pytest

import lddt_cases as K
import tm_cases as TC

pytestmark = pytest.mark.gpu

BIN = os.path.join(K.ROOT, "foldseek_amd", "bin", "fsgpu-modules")
BITS_WARNING = "C-alpha database\nDisabling --sort-by-structure-bits\n"


def read_db(path):
    t = int.from_bytes(open(path + ".dbtype", "rb").read(4), "little", signed=True)
    data = open(path, "rb").read()
    out = {}
    for line in open(path + ".index"):
        k, off, ln = line.split()
        out[int(k)] = data[int(off):int(off) + int(ln) - 1]
    return t, out


@pytest.fixture()
def work(tmp_path):
    """a private copy of ca_v1's frozen DBs with the links the reference's makepaddedseqdb workflow makes, and tm_v1's outputs and crafted DB next to them"""
    w = tmp_path / "tm"
    shutil.copytree(K.GOLD, w)
    for link, target in K.MANIFEST["links"].items():
        os.symlink(str(w / target), str(w / link))
    for f in os.listdir(TC.GOLD):
        shutil.copy(os.path.join(TC.GOLD, f), w / f)
    return w


def _run(cmd, dev=None):
    env = dict(os.environ, FSGPU_BT_PASS2="1")
    if dev is not None:
        env["FSGPU_DEVICE_BACKTRACE"] = str(dev)
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)


def _same_db(got_path, want_path):
    want_t, want = read_db(want_path)
    got_t, got = read_db(got_path)
    assert got_t == want_t and sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k] == want[k], f"entry {k}\nwant {want[k][:300]!r}\ngot  {got[k][:300]!r}"
    return sum(len(v.decode().splitlines()) for v in got.values())


_ALIGN = sorted(n for n, r in TC.MANIFEST["runs"].items() if r["module"] == "structurealign")


@pytest.mark.parametrize("dev", [0, 1])
@pytest.mark.parametrize("name", _ALIGN)
def test_structurealign_equals_reference_result_db(work, name, dev):
    """every frozen parameter set (structure bits with and without thresholds, a threshold alone in the modes 0 / 1 / 2, --max-rejected 2: the hit-by-hit
    path, --alt-ali 2: alternative alignments keep their own scores, the padded target), backtraces by the host (dev 0) and by the device (dev 1) aligner"""
    run = TC.MANIFEST["runs"][name]
    out = str(work / f"mine_{dev}_{name}")
    r = _run([BIN, "structurealign"] + [str(work / p) for p in run["positional"]] + [out] + run["parameters"], dev)
    assert r.returncode == 0, r.stderr
    assert _same_db(out, str(work / name)) == run["lines"]
    assert "Disabling" not in r.stderr


@pytest.mark.parametrize("dev", [0, 1])
@pytest.mark.parametrize("name", _ALIGN)
def test_fused_search_equals_reference_result_db(work, name, dev):
    """`search` at every frozen parameter set: with the ungapped prefilter at --min-ungapped-score 0 it hands the aligner the 144 pairs the frozen prefilter
    DB holds, in its order"""
    run = TC.MANIFEST["runs"][name]
    par = run["parameters"]
    get = lambda flag: par[par.index(flag) + 1]  # noqa: E731
    target, pref = run["positional"][1], run["positional"][2]
    out, outp = str(work / f"mine_search_{dev}_{name}"), str(work / f"mine_search_{dev}_{name}_pref")
    cmd = [BIN, "search", str(work / "db"), str(work / target), out, outp, "--prefilter-mode", "1", "--min-ungapped-score", "0", "-a", "1", "--alignment-type", "2",
           "--threads", "2", "--max-seqs", "1000", "-e", "10"]
    for flag in ("--sort-by-structure-bits", "--tmscore-threshold", "--tmscore-threshold-mode", "--lddt-threshold", "--alt-ali", "--max-rejected"):
        cmd += [flag, get(flag)]
    r = _run(cmd, dev)
    assert r.returncode == 0, r.stderr
    assert read_db(outp) == read_db(str(work / pref))
    assert _same_db(out, str(work / name)) == run["lines"]
    assert "Disabling" not in r.stderr


def test_convertalis_tm_columns_equal_reference_text(work):
    for name in ("conv_tm.m8", "conv_tm_crafted.m8"):
        run = TC.MANIFEST["convert_runs"][name]
        out = str(work / ("mine_" + name))
        r = _run([BIN, "convertalis"] + [str(work / p) for p in run["positional"]] + [out] + run["parameters"])
        assert r.returncode == 0, r.stderr
        want, got = open(os.path.join(TC.GOLD, name), "rb").read(), open(out, "rb").read()
        if got != want:
            for i, (a, b) in enumerate(zip(want.split(b"\n"), got.split(b"\n"))):
                assert a == b, f"{name}: line {i + 1}\nwant {a[:300]!r}\ngot  {b[:300]!r}"
        assert got == want
    # single columns (the rmsd alone is asked with the target length), next to an LDDT column
    out = str(work / "mine_short.m8")
    r = _run([BIN, "convertalis", str(work / "db"), str(work / "db"), str(work / "aln_l0"), out, "--format-output", "query,rmsd,lddt,qtmscore"])
    assert r.returncode == 0, r.stderr
    tm = [l.split(b"\t") for l in open(os.path.join(TC.GOLD, "conv_tm.m8"), "rb").read().splitlines()]
    ld = [l.split(b"\t") for l in K.frozen_text("conv_lddt.m8").splitlines()]
    assert open(out, "rb").read() == b"".join(b"\t".join((a[0], a[6], b[3], a[4])) + b"\n" for a, b in zip(tm, ld))
    r = _run([BIN, "convertalis", str(work / "db"), str(work / "db"), str(work / "aln_l0"), str(work / "o.m8"), "--format-output", "query,rmsd", "--exact-tmscore", "1"])
    assert r.returncode == 1 and "--exact-tmscore 1 is not implemented" in r.stderr
    for col in ("u", "t", "qca", "tca"):
        r = _run([BIN, "convertalis", str(work / "db"), str(work / "db"), str(work / "aln_l0"), str(work / "o.m8"), "--format-output", "query," + col])
        assert r.returncode == 1 and f"column {col} is not implemented" in r.stderr
    assert not os.path.exists(work / "o.m8")


def test_without_ca_structure_bits_warn_and_the_refusals_stay(work):
    """without <db>_ca: structure bits are switched off with the reference's warning and the run equals --sort-by-structure-bits 0; --tmscore-threshold > 0
    and the TM columns keep the refusals this path gave before (the reference would warn and carry on: README)"""
    for f in os.listdir(work):
        if f.startswith("db_ca"):
            os.remove(work / f)
    run = TC.MANIFEST["runs"]["aln_sb1"]
    out = str(work / "mine_noca")
    r = _run([BIN, "structurealign"] + [str(work / p) for p in run["positional"]] + [out] + run["parameters"])
    assert r.returncode == 0, r.stderr
    assert BITS_WARNING in r.stderr
    assert _same_db(out, str(work / "aln_l0")) == 144
    run = TC.MANIFEST["runs"]["aln_sb0_t07_m0"]
    r = _run([BIN, "structurealign"] + [str(work / p) for p in run["positional"]] + [str(work / "mine_noca2")] + run["parameters"])
    assert r.returncode == 1 and "structurealign: --tmscore-threshold 0.7 is not implemented on the device path (supported: 0|0.0|0.000)" in r.stderr
    assert not os.path.exists(work / "mine_noca2.index")
    r = _run([BIN, "convertalis", str(work / "db"), str(work / "db"), str(work / "aln_l0"), str(work / "o.m8"), "--format-output", "query,target,alntmscore"])
    assert r.returncode == 1 and "convertalis: column alntmscore is not implemented on this path (needs the C-alpha, taxonomy or multimer data)" in r.stderr
    assert not os.path.exists(work / "o.m8")
