"""`fsgpu-modules structurealign` with profile queries on the seeded world of tests/profile_cases.py, written as databases from the seed: run with the
positional arguments and the complete parameter strings the reference binary was run with (tests/golden/profile_align_v1/MANIFEST.json, generator
tests/golden/make_profile_align_golden.py), every result DB must be the reference's byte for byte: data, index and type.  The six runs: the defaults,
coverage modes 1 and 2 with the threshold AT a hit's start-to-end coverage, --seq-id-mode 1 with the threshold at a hit's identity, --min-aln-len at a
hit's length, gap costs 8 / 2 -- over X next to the aligned stretch, long indels, single-cell alignments and prefixes at every border of the SW kernels."""
import json
import os
import subprocess

import pytest

import profile_cases as K
from test_profile_modules_gpu import BIN, _same_files, _with

pytestmark = pytest.mark.gpu

RUNS = json.load(open(os.path.join(K.GOLD, "MANIFEST.json")))["runs"]


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    w = tmp_path_factory.mktemp("profile_align")
    K.write_world(w)
    return w


@pytest.mark.parametrize("threads", (1, 4))
@pytest.mark.parametrize("name", sorted(RUNS))
def test_structurealign_equals_reference_result_db(work, name, threads):
    run = RUNS[name]
    out = str(work / f"mine_{name}_{threads}")
    r = subprocess.run([BIN, "structurealign"] + [str(work / p) for p in run["positional"]] + [out] + _with(run["parameters"], **{"--threads": threads}) + ["--gpus", "1"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    _same_files(out, os.path.join(K.GOLD, name))
