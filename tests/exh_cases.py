"""tests/exh_cases.py -- the exhaustive search's cases (TEST INFRASTRUCTURE): the world of tests/align_cases.py with EVERY target in every query's list
(lists = 0 .. n-1, the order of fake_pref's lines), the parameter sets, and the frozen answers of tests/align_model.py (tests/golden/exh_v1, written by
tests/golden/make_exh_golden.py).  Per set and query: the model's records and CIGARs in output order, and the number of targets alignStructure's first
e-value gate would let through -- the survivors of the device's selection."""
import json
import os

import numpy as np

import align_cases as AC

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "exh_v1")
ATYPES = (2, 0)
NAMED_QUERY = AC.NAMED_QUERY


def n_queries():
    return len(AC.Q_LENGTHS)                      # the world's ninth list repeats the named query for a purpose of its own: not needed here


def all_targets():
    return np.arange(len(AC.world()["targets"]), dtype=np.uint32)


class Live:
    """tests/align_model.py over all targets"""

    def __init__(self, atype):
        import align_model as A
        self.A, self.w = A, AC.world()
        self.W = A.World(self.w["targets"], keys=self.w["keys"], alignment_type=atype)
        self._runs = {}

    def query(self, q, P):
        k = (q, tuple(sorted(P.items())))
        if k not in self._runs:
            qa, q3 = self.w["queries"][q]
            self._runs[k] = self.A.align_query(self.W, qa, q3, all_targets(), P, identity=self.w["identity"][q])
        return self._runs[k]

    def evalue_fwd(self, q, target):
        qa, q3 = self.w["queries"][q]
        r = self.query(q, self.A.params())
        return self.W.evalue(self.W.query(qa, q3), int(r.fwd[target]["score"]) & 0xFFFFFFFF)

    def survivors(self, q, P):
        """targets whose forward e-value is not above the threshold: what the first e-value gate lets through, whatever the gates before it say"""
        qa, q3 = self.w["queries"][q]
        r = self.query(q, self.A.params())
        qq = self.W.query(qa, q3)
        return sum(1 for t in range(len(r.fwd)) if not self.W.evalue(qq, int(r.fwd[t]["score"]) & 0xFFFFFFFF) > P["evalThr"])


def derive(live):
    """{name: params}: defaults; -e at the forward e-value of a named hit (the median accepted piece of the named query) and the next double below it;
    -e 1e300 (the cutoff is 0: everything survives); -c 0.8; --max-accept 3; --alt-ali 2"""
    A = live.A
    sets = {"default": A.params()}
    r = live.query(NAMED_QUERY, sets["default"])
    acc = [i for i in range(len(r.records)) if live.w["kinds"][r.hit_of_record[i]] == "piece"]
    assert len(acc) >= 8
    i = sorted(acc, key=lambda i: (float(r.records[i]["eval"]), i))[len(acc) // 2]
    ef = float(live.evalue_fwd(NAMED_QUERY, r.hit_of_record[i]))
    sets["efwd_eq"] = A.params(evalThr=ef)
    sets["efwd_below"] = A.params(evalThr=float(np.nextafter(np.float64(ef), -np.inf)))
    sets["e1e300"] = A.params(evalThr=1e300)
    sets["c08"] = A.params(covThr=0.8)
    sets["acc3"] = A.params(maxAccept=3)
    sets["alt2"] = A.params(altAlignment=2)
    return sets


def save(atype, sets, live):
    import align_model as A
    os.makedirs(GOLD, exist_ok=True)
    arrays, cigs, meta = {}, [], {}
    for name, P in sets.items():
        for q in range(n_queries()):
            r = live.query(q, P)
            arrays[f"{name}/{q}/rec"] = r.records
            arrays[f"{name}/{q}/cig"] = np.arange(len(cigs), len(cigs) + len(r.cigars), dtype=np.int32)
            cigs += list(r.cigars)
        arrays[f"{name}/surv"] = np.array([live.survivors(q, P) for q in range(n_queries())], np.int64)
        meta[name] = AC._hex(P)
    arrays["cigars"] = np.frombuffer("\n".join(cigs).encode(), np.uint8)
    np.savez_compressed(os.path.join(GOLD, f"answers_t{atype}.npz"), **arrays)
    json.dump(dict(seed=AC.SEED, targets=len(AC.world()["targets"]), rec_dt=[list(x) for x in A.REC_DT.descr], sets=meta), open(os.path.join(GOLD, f"sets_t{atype}.json"), "w"),
              indent=0, sort_keys=True)


class Frozen:
    def __init__(self, atype):
        j = json.load(open(os.path.join(GOLD, f"sets_t{atype}.json")))
        assert j["seed"] == AC.SEED and j["targets"] == len(AC.world()["targets"]), "the world changed: run tests/golden/make_exh_golden.py"
        self.meta = j["sets"]
        self.names = list(self.meta)
        z = np.load(os.path.join(GOLD, f"answers_t{atype}.npz"))
        self.z = {k: z[k] for k in z.files}
        self.cigars = bytes(self.z["cigars"]).decode().split("\n")

    def params(self, name):
        return AC._unhex(self.meta[name])

    def records(self, name, q):
        return self.z[f"{name}/{q}/rec"], [self.cigars[i] for i in self.z[f"{name}/{q}/cig"]]

    def survivors(self, name):
        return [int(x) for x in self.z[f"{name}/surv"]]
