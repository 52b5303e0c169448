"""CPU-only: tests/dtw_ref.py -- the definition spx_batch_dtw is held to (tests/test_gpu_dtw.py) -- against the reference's known
answers (dynamic_time_warping_test.cc:30-80), against the reference's own thresholds on its own test pair (sonic_test.cc:639-724),
against the older numpy restatement (sonic_props.dtw), and against two mutants."""
import numpy as np
import pytest

import dtw_cases
import dtw_ref
import sonic_props as sp

A5 = [0.0, 1.0, 2.0, 3.0, 4.0]
KNOWN = {
    "identical": (A5, A5, 0.0, [0, 1, 2, 3, 4], [0, 1, 2, 3, 4]),
    "shifted": (A5, [-2.0, -1.0, 0.0, 1.0, 2.0], 6.0, [0, 0, 0, 1, 2, 3, 4], [0, 1, 2, 3, 4, 4, 4]),
    "downsampled": (A5, [0.0, 2.0, 4.0], 2.0, [0, 1, 2, 3, 4], [0, 0, 1, 1, 2]),
}


@pytest.mark.parametrize("case", sorted(KNOWN))
def test_reference_known_answers(case):
    """dim = 1: the Euclidean cost is fabs exactly."""
    a, b, cost, p1, p2 = KNOWN[case]
    r = dtw_ref.dtw(a, b, 1)
    assert float(r["cost"]) == cost
    assert r["path"][:, 0].tolist() == p1 and r["path"][:, 1].tolist() == p2
    assert r["n_path"] == len(p1) and r["n_local"] == max(0, len(p1) - 2)


def test_local_cost_is_sequential_float32():
    """The sum is added one term after another in a float: 2^24 followed by 4 096 ones stays 2^24 (2^24 + 1 is a tie and rounds
    back to the even 2^24), where a sum that adds the ones to each other first does not."""
    a = np.zeros(4097, np.float32)
    b = np.ones(4097, np.float32)
    a[0] = 4097.0   # t = 4096, t * t = 2^24
    d = dtw_ref.local_cost(a, b)
    assert float(d) == 4096.0
    assert float(np.sqrt(((a - b) ** 2).sum(dtype=np.float32))) != 4096.0


@pytest.mark.parametrize("n_a,n_b,dim", [(17, 13, 60), (5, 9, 240), (30, 30, 1), (8, 8, 3)])
def test_matrix_form_of_the_local_costs_is_the_scalar_form(n_a, n_b, dim):
    """dtw_cases.local_costs (what the GPU tests feed the definition's recurrence at large dim) equals dtw_ref.local_cost, bit for
    bit, and so does everything computed from it."""
    rng = np.random.default_rng(n_a * 1000 + dim)
    a = (rng.standard_normal((n_a, dim)) * 100).astype(np.float32)
    b = (rng.standard_normal((n_b, dim)) * 100).astype(np.float32)
    d = dtw_cases.local_costs(a, b)
    want = np.array([[dtw_ref.local_cost(ra, rb) for rb in b] for ra in a], np.float32)
    assert np.array_equal(d.view(np.uint32), want.view(np.uint32))
    r, q = dtw_ref.dtw(a, b, 2), dtw_cases.answer(a, b, 2)
    assert dtw_ref.same_bits(r["cost"], q["cost"]) and np.array_equal(r["path"], q["path"])


def test_matrix_form_on_the_tapestry_pair():
    rows = dtw_cases.tapestry_rows()
    r, q = dtw_cases.tapestry_answer("linear"), dtw_cases.answer(rows["original"], rows["linear"])
    assert dtw_ref.same_bits(r["cost"], q["cost"]) and np.array_equal(r["path"], q["path"])


def test_zero_denominators_are_ieee():
    r = dtw_ref.dtw([1.0], [2.0], 1)
    assert r["n_path"] == 1 and r["n_local"] == 0 and float(r["cost"]) == 1.0
    assert np.isnan(r["slope"]) and np.isnan(r["local_mean"]) and np.isnan(r["local_std"])
    # a does not advance: every x is 0, the denominator is 0
    r = dtw_ref.dtw([1.0], [1.0, 2.0, 3.0, 4.0], 1)
    assert r["path"].tolist() == [[0, 0], [0, 1], [0, 2], [0, 3]] and r["n_local"] == 2
    assert np.isnan(r["slope"]) and np.isnan(r["local_mean"])
    assert dtw_ref.same_bits(np.float32("nan"), -np.float32("nan")) and not dtw_ref.same_bits(0.0, -0.0)


@pytest.mark.parametrize("name", ["linear", "nonlinear"])
def test_tapestry_passes_the_reference_thresholds(name):
    r = dtw_cases.tapestry_answer(name)
    print(name, "cost %r slope %r mean %r std %r n_path %d" % (float(r["cost"]), float(r["slope"]), float(r["local_mean"]),
                                                               float(r["local_std"]), r["n_path"]))
    dtw_cases.reference_thresholds(name, r)


def test_summation_order_is_observable_on_real_data():
    """On the linear pair the definition's cost differs in its bit pattern from sonic_props.dtw's (numpy's pairwise sum of the
    squared differences) while the paths are equal: a kernel that tree-reduces the sum cannot pass the GPU test."""
    rows = dtw_cases.tapestry_rows()
    r = dtw_cases.tapestry_answer("linear")
    cost, p1, p2 = sp.dtw(rows["original"], rows["linear"])
    assert r["path"][:, 0].tolist() == p1 and r["path"][:, 1].tolist() == p2
    assert dtw_ref.bits(r["cost"]) != dtw_ref.bits(np.float32(cost)), (float(r["cost"]), cost)
    assert abs(float(r["cost"]) - cost) <= 4.0


def test_mutant_nonstrict_ties_changes_the_downsampled_case():
    """Ties no longer go along the diagonal: the down-sampled case's path changes (its cost, 2, does not: the known costs alone
    would not see the tie rule)."""
    a, b, cost, p1, p2 = KNOWN["downsampled"]
    r = dtw_ref.dtw(a, b, 1, rule=dtw_ref.NONSTRICT_TIES)
    assert float(r["cost"]) == cost
    assert (r["path"][:, 0].tolist(), r["path"][:, 1].tolist()) != (p1, p2)


def test_mutant_swapped_up_left_changes_the_shifted_case():
    """Up and left swapped in the direction test: the shifted case's path runs down the first column instead of along the first row."""
    a, b, cost, p1, p2 = KNOWN["shifted"]
    r = dtw_ref.dtw(a, b, 1, rule=dtw_ref.SWAPPED_UP_LEFT)
    assert float(r["cost"]) == cost
    assert (r["path"][:, 0].tolist(), r["path"][:, 1].tolist()) != (p1, p2)
