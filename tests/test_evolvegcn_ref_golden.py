"""CPU: the EvolveGCN-H restatement of the tests (tests/_evolvegcn_ref.py) against the real reference's fixtures G13
(tests/golden/make_golden_evolvegcn.py) — the pin that makes it a checker for the sizes the fixtures do not cover."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _evolvegcn_ref as ref  # noqa: E402
from _util import golden, golden_names, max_rel_err  # noqa: E402

SMALL_EDGE = [n for n in golden_names("g13_egcn_small_") if "reg" not in n]


def _layers(d):
    return len(d["hidden"]) - 1


def _idx_match(rec, d, prefix=""):
    """the restatement's selections equal the reference's wherever the reference's score is not tied"""
    for layer in (1, 2):
        if f"{prefix}idx{layer}" not in d.files:
            continue
        got = np.stack([i.numpy() for l, i in rec if l == layer])
        want, ys = d[f"{prefix}idx{layer}"], d[f"{prefix}ysel{layer}"]
        for t in range(want.shape[0]):
            untied = np.array([np.sum(ys[t] == ys[t, j]) == 1 for j in range(ys.shape[1])])
            np.testing.assert_array_equal(got[t][untied], want[t][untied], err_msg=f"layer {layer}, slice {t}")


@pytest.mark.parametrize("name", SMALL_EDGE)
def test_small_edge_cases(name):
    d = golden(name)
    T, N, layers = int(d["T"]), int(d["N"]), _layers(d)
    A = ref.sparse_slices(d, N)
    rec = []
    logits, loss, grads, Ws = ref.train_step(A, torch.tensor(d["X"]), d, layers, d["edges"], d["target"], d["weight"],
                                             record=rec)
    assert max_rel_err(logits, d["logits"]) <= 1e-6
    assert abs(float(loss) - float(d["loss"])) <= 1e-6 * abs(float(d["loss"]))
    for n in ref.names(layers):
        assert max_rel_err(grads[n], d["d" + n]) <= 1e-6, n
    for q, w in enumerate(Ws):
        assert max_rel_err(w.detach(), d[f"W_T{q + 1}"]) <= 1e-9
    _idx_match(rec, d)
    # the validation call: 3 slices with the W the training call returned, Y zero beyond them (ef:66)
    q = ref.params(d, layers, grad=False)
    W02 = torch.tensor(d["W_T2"]) if layers == 2 else None
    Y, Wv = ref.embed(A[:3], torch.tensor(d["X"][:3]), q, torch.tensor(d["W_T1"]), T, W02)
    assert max_rel_err(ref.edge_logits(Y, d["edges_val"], q["U"]), d["logits_val"]) <= 1e-6
    for i, w in enumerate(Wv):
        assert max_rel_err(w, d[f"W_val{i + 1}"]) <= 1e-9


def test_small_regression_case():
    d = golden("g13_egcn_small_reg_n50")
    T, N = int(d["T"]), int(d["N"])
    A = ref.sparse_slices(d, N)
    q = ref.params(d, 1, grad=False)
    Y, _ = ref.embed(A, torch.tensor(d["X"]), q, torch.tensor(d["W_init"]), T)
    out = (Y @ torch.tensor(d["lin_w0"]).t() + torch.tensor(d["lin_b0"])).squeeze(2)
    assert max_rel_err(out, d["out"]) <= 1e-6
    np.testing.assert_array_equal(d["out_call"], d["out"])          # no W_init: the training output (ef:342)
    Y, _ = ref.embed(A[:3], torch.tensor(d["X"][:3]), q, torch.tensor(d["W_call"]), T)
    out = (Y @ torch.tensor(d["lin_w0"]).t() + torch.tensor(d["lin_b0"])).squeeze(2)
    assert max_rel_err(out, d["out_call_w"]) <= 1e-6
    assert list(d["param_names"]) == ref.names(1) + ["lin1.weight", "lin1.bias"]


def test_chess_lp_against_g13():
    from _g10 import G10
    g, d = G10(), golden("g13_egcn_chess_lp")
    A = [torch.sparse_coo_tensor(torch.tensor(np.stack([i, j])), torch.tensor(v, dtype=torch.float64), (g.N, g.N)).coalesce()
         for i, j, v in _slices(g, range(g.T - 1))]
    edges, target = ref.lp_edges(g, d)
    rec = []
    logits, loss, grads, Ws = ref.train_step(A, torch.tensor(g.X[:g.T - 1]), d, 1, edges, target, d["weight"], T=g.T - 1,
                                             record=rec)
    assert max_rel_err(logits, d["logits"]) <= 1e-6
    assert abs(float(loss) - float(d["loss"])) <= 1e-6 * abs(float(d["loss"]))
    for n in ref.names(1):
        assert max_rel_err(grads[n], d["d" + n]) <= 1e-6, n
    _idx_match(rec, d)


def _slices(g, rng):
    k, i, j, v = g.C()
    return [(i[k == s], j[k == s], v[k == s]) for s in rng]


def test_fixture_records():
    for name in golden_names("g13_egcn_"):
        d = golden(name)
        assert "min_gap" in d.files, name
    d = golden("g13_egcn_chess")
    assert list(d["param_names"]) == ref.names(2)
    assert list(d["param_dtypes"]) == ["torch.float64"] * 20 + ["torch.float32"]
