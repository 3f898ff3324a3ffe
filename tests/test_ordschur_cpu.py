"""CPU: the selections, the expected order and the inputs of the ordschur tests (tests/ordschur_ref.py) are sound
with the reference alone.

``scipy.linalg.lapack.dtrsen`` / ``ztrsen`` reorder ``scipy.linalg.schur``'s (T, Z) of every named matrix of
tests/schur_ref.py under every selection, and the constructed quasi-triangular inputs with Z = I.  For each case:
``info == 0``; ``check_structure`` accepts the new T; the figures r = ||A - Z T Z^H||_F / (n eps ||A||_F) and
o = ||Z^H Z - I||_F / (n eps) are at most 2/3, or within 1.25 of what tests/golden/ordschur_ref_figures.json
records (the rule of tests/test_schur_cpu.py); and the new eigenvalues are the stable partition of the old ones,
position by position, within 2 n eps ||A||_F.

    python tests/test_ordschur_cpu.py        # rewrites tests/golden/ordschur_ref_figures.json
"""
import json
import os

import numpy as np
import pytest

import ordschur_ref as O
import schur_ref as S
from test_schur_cpu import run as schur_run

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ordschur_ref_figures.json")
_runs = {}


def case_inputs(kind, key):
    """(A, T, Z) of a case: a named matrix with LAPACK's Schur form, or a constructed T with Z = I."""
    if kind == "named":
        T, Z, _, _ = schur_run(key)
        return S.matrix(key), T, Z
    T = O.pairs(*key)
    return T, T, np.eye(T.shape[0])


def case_id(kind, key, sel):
    return f"{key}:{sel}" if kind == "named" else f"pairs{key[0]}{'o' if key[1] else 'e'}:{sel}"


def run(kind, key, sel):
    """xTRSEN on one case, once per session: dict(info, m, T, r, o, d, bound, sdim)."""
    cid = case_id(kind, key, sel)
    if cid not in _runs:
        A, T, Z = case_inputs(kind, key)
        mask = O.selection(T, sel)
        ts, qs, w, m, info = O.trsen(T, Z, mask)
        r, o = S.figures(A, ts, qs)
        _runs[cid] = dict(info=info, m=m, T=ts, r=r, o=o, d=O.order_error(A, w, O.expected_order(T, mask)),
                          dblocks=O.order_error(A, S.block_eigenvalues(ts), O.expected_order(T, mask)),
                          bound=S.value_bound(A), sdim=int(mask.sum()), real=not np.iscomplexobj(T))
    return _runs[cid]


def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


CASES = [("named", nm, sel) for nm in S.NAMES for sel in O.SELECTIONS] + \
        [("pairs", key, sel) for key in O.pairs_cases() for sel in O.SELECTIONS]


@pytest.mark.parametrize("kind,key,sel", CASES, ids=[case_id(*c) for c in CASES])
def test_lapack_meets_the_conditions(kind, key, sel):
    res = run(kind, key, sel)
    rec = recorded()[case_id(kind, key, sel)]
    print(f"{case_id(kind, key, sel)}: info={res['info']} r={res['r']:.3g} o={res['o']:.3g} d={res['d']:.3g} "
          f"(bound {res['bound']:.3g}) recorded r={rec['r']:.3g} o={rec['o']:.3g}")
    assert res["info"] == 0
    assert res["m"] == res["sdim"]
    S.check_structure(res["T"], res["real"])
    for key_ in ("r", "o"):
        assert np.isfinite(res[key_])
        assert res[key_] <= 2.0 / 3.0 or res[key_] <= 1.25 * rec[key_]
    assert res["d"] <= res["bound"]
    assert res["dblocks"] <= res["bound"]


def test_selections_respect_blocks():
    T = O.pairs(95, True)
    for sel in O.SELECTIONS:
        m = O.selection(T, sel)
        assert np.array_equal(m, O.pair_rule(T, m))
    assert O.selection(T, "all").all() and not O.selection(T, "none").any()
    assert O.selection(T, "last").sum() == 2 and O.selection(T, "last")[-1]
    one = np.zeros(95, dtype=bool)
    one[2] = True   # the second row of the pair on rows 1, 2
    assert np.array_equal(np.nonzero(O.pair_rule(T, one))[0], [1, 2])


def test_constructed_inputs_are_standard():
    for n, first in O.pairs_cases():
        T = O.pairs(n, first)
        S.check_structure(T, True)
        starts = [k for k, sz in O.blocks(T) if sz == 2]
        assert starts == list(range(1 if first else 0, n - 1, 2))


if __name__ == "__main__":
    out = {}
    for c in CASES:
        res_ = run(*c)
        out[case_id(*c)] = {"r": res_["r"], "o": res_["o"], "d_over_bound": res_["d"] / res_["bound"] if res_["bound"] else 0.0,
                            "info": res_["info"]}
    with open(GOLDEN, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("cases", len(out), "max r", max(v["r"] for v in out.values()), "max o", max(v["o"] for v in out.values()),
          "max d/bound", max(v["d_over_bound"] for v in out.values()), "worst info", max(v["info"] for v in out.values()))
