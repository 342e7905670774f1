"""CPU: the WD-GCN restatement of the tests (tests/_wdgcn_ref.py) against the real reference's fixtures G12
(tests/golden/make_golden_wdgcn.py) — the pin that makes it a checker for the sizes the fixtures do not cover."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wdgcn_ref as ref  # noqa: E402
from _util import golden, golden_names, max_rel_err  # noqa: E402

SMALL_EDGE = [n for n in golden_names("g12_wdgcn_small_") if "reg" not in n]


def _coo(d, T):
    k, i, j, v = d["A_k"], d["A_i"], d["A_j"], d["A_v"]
    return [(i[k == s], j[k == s], v[k == s]) for s in range(T)]


def _params(d):
    return {n: torch.from_numpy(d[n + "0"]) for n in ref.NAMES}


@pytest.mark.parametrize("name", SMALL_EDGE)
def test_small_edge_cases(name):
    d = golden(name)
    T = int(d["T"])
    AX = ref.compute_AX(_coo(d, T), d["X"], T)
    logits, loss, grads = ref.train_step(AX, _params(d), d["h_init"], d["c_init"], d["U"], d["edges"], d["target"], d["weight"])
    assert max_rel_err(logits, d["logits"]) <= 1e-6
    assert abs(float(loss) - float(d["loss"])) <= 1e-6 * abs(float(d["loss"]))
    for n in ref.NAMES:
        assert max_rel_err(grads[n], d["d" + n]) <= 1e-5, n
    # the validation call: 3 slices, AX zero-padded to the model's T
    AXv = ref.compute_AX(_coo(d, 3), d["X"][:3], T)
    Z = ref.lstm(AXv, _params(d), torch.from_numpy(d["h_init"]), torch.from_numpy(d["c_init"]))
    assert max_rel_err(ref.edge_logits(Z, d["edges_val"], torch.from_numpy(d["U"])), d["logits_val"]) <= 1e-6


def test_small_regression_case():
    d = golden("g12_wdgcn_small_reg_h6_n50")
    T = int(d["T"])
    AX = ref.compute_AX(_coo(d, T), d["X"], T)
    y = ref.reg_forward(AX, _params(d), d["h_init"], d["c_init"], d["lin_w0"], d["lin_b0"])
    assert max_rel_err(y, d["out"]) <= 1e-6
    # __call__(A, X) passes no edges: the training window's output whatever it is handed (wgf:131-138)
    np.testing.assert_array_equal(d["out_call"], d["out"])
    # lin1 is a submodule built before the parameters are drawn: nn.Module lists the 13 own parameters first
    assert list(d["param_order"]) == list(ref.NAMES) + ["lin1.weight", "lin1.bias"]


def test_chess_fp32_form_and_fp64_truth():
    from _g10 import G10
    g, d = G10(), golden("g12_wdgcn_chess")
    k, i, j, v = g.C()
    coo = [(i[k == s], j[k == s], v[k == s]) for s in range(g.T)]
    AX = ref.compute_AX(coo, g.X[:g.T], g.T)
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    p = _params(d)
    logits, loss, grads = ref.train_step(AX, p, d["h_init"], d["c_init"], d["U"], g.edges_train, g.target_train, g.class_weights)
    assert max_rel_err(logits, d["logits"]) <= 1e-5
    assert abs(float(loss) - float(d["loss"])) <= 1e-5 * abs(float(d["loss"]))
    for n in ref.NAMES:
        assert max_rel_err(grads[n], d["d" + n]) <= 1e-4, n
    _, loss64, grads64 = ref.train_step(AX, p, d["h_init"], d["c_init"], d["U"], g.edges_train, g.target_train,
                                        g.class_weights, dtype=torch.float64)
    assert abs(float(loss64) - float(d["loss64"])) <= 1e-12 * abs(float(d["loss64"]))
    for n in ref.NAMES:
        assert max_rel_err(grads64[n], d["d" + n + "64"]) <= 1e-10, n
