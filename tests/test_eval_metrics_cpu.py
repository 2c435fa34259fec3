"""The evaluation surface without a GPU: metrics.f1_from_confusion against
sklearn, the numpy model of the kernels' argmax rule (tests/eval_cases.py)
against torch.max with each of its mutants caught by a named case, and
SGC.evaluate / SGC.predict on CPU tensors against the literal expressions."""
import numpy as np
import pytest
import sklearn.metrics as sklearn_metrics
import torch

import eval_cases as ec


# ---- f1_from_confusion -------------------------------------------------------------

def _cm(y, p, C):
    return np.bincount(np.asarray(y) * C + np.asarray(p), minlength=C * C).reshape(C, C)


def _f1_cases():
    rng = np.random.default_rng(0)
    y = rng.integers(0, 41, 5000)
    p = np.where(rng.random(5000) < 0.6, y, rng.integers(0, 41, 5000))
    yield "random_41", y, p, 41
    yield "class_only_in_predictions", [0, 0, 1, 1, 1], [0, 2, 1, 1, 2], 4
    yield "class_only_in_labels", [0, 1, 2, 2, 2], [0, 1, 1, 0, 0], 4
    yield "class_absent_from_both", [0, 0, 3, 3], [0, 3, 3, 3], 5
    yield "single_class", [2, 2, 2], [2, 2, 2], 3
    yield "everything_wrong", [0, 1, 2, 0], [1, 2, 0, 2], 3


@pytest.mark.parametrize("name,y,p,C", list(_f1_cases()), ids=[c[0] for c in _f1_cases()])
def test_f1_from_confusion_matches_sklearn(name, y, p, C):
    from sgc_amd.metrics import f1_from_confusion
    micro, macro = f1_from_confusion(_cm(y, p, C))
    ref_micro = sklearn_metrics.f1_score(y, p, average="micro")
    ref_macro = sklearn_metrics.f1_score(y, p, average="macro")
    assert abs(micro - ref_micro) <= 1e-12, (micro, ref_micro)
    assert abs(macro - ref_macro) <= 1e-12, (macro, ref_macro)


def test_f1_from_confusion_empty():
    from sgc_amd.metrics import f1_from_confusion
    assert f1_from_confusion(np.zeros((3, 3), np.int64)) == (0.0, 0.0)


# ---- the argmax model against torch.max -----------------------------------------------

NAN, INF = float("nan"), float("inf")

# name -> (Z rows over CP columns, C, the mutant the case must catch or None)
ARGMAX_CASES = {
    "issue_example": ([[1, 3, 3, 2], [NAN, 5, NAN, 1], [2, 2, 2, 2]], 4, None),
    "tie_in_lane": ([[0, 7, 7, 1, 0, 0]], 6, "last_on_tie"),            # classes 1, 2: lane group 0
    "nan_first_class": ([[NAN, 9, 1, 2, 3, 4]], 6, "nan_ignored"),
    "nan_later_class": ([[5, 1, 2, 3, 4, NAN, 0, 0]], 8, "nan_ignored"),
    "tie_across_groups_3_4": ([[0, 0, 0, 6, 6, 0, 0, 0]], 8, "ge_across_groups"),
    "tie_across_tiles_15_16": ([[0] * 15 + [4, 4] + [0] * 3], 20, None),
    "all_negative_padded_zero": ([[-3, -1, -2, 0, 0, 0, 0, 0]], 3, "padded_may_win"),
    "minus_inf_everywhere_but_one": ([[-INF, -INF, 2, -INF]], 4, None),
    "plus_inf_one_class": ([[1, INF, 3, 2]], 4, None),
    "signed_zeros_tie": ([[-0.0, 0.0, -1.0]], 3, None),
}


@pytest.mark.parametrize("name", sorted(ARGMAX_CASES))
def test_argmax_model_equals_torch_max(name):
    rows, C, _ = ARGMAX_CASES[name]
    Z = np.array(rows, dtype=np.float32)
    ref = torch.from_numpy(Z[:, :C].copy()).max(1)[1].numpy()
    assert np.array_equal(ec.argmax_model(Z, C), ref), (name, ec.argmax_model(Z, C), ref)


def test_argmax_model_on_random_ties_and_nans():
    rng = np.random.default_rng(3)
    Z = rng.integers(-2, 3, (300, 41)).astype(np.float32)  # many exact ties
    Z[rng.random(Z.shape) < 0.02] = NAN
    ref = torch.from_numpy(Z).max(1)[1].numpy()
    assert np.array_equal(ec.argmax_model(Z), ref)


@pytest.mark.parametrize("name", sorted(n for n, c in ARGMAX_CASES.items() if c[2]))
def test_each_argmax_mutant_is_caught_by_its_case(name):
    rows, C, mutant = ARGMAX_CASES[name]
    Z = np.array(rows, dtype=np.float32)
    ref = torch.from_numpy(Z[:, :C].copy()).max(1)[1].numpy()
    assert not np.array_equal(ec.argmax_model(Z, C, mutant=mutant), ref), (name, mutant)


def test_every_argmax_mutant_has_a_case():
    caught = {c[2] for c in ARGMAX_CASES.values() if c[2]}
    assert caught == set(ec.MUTANTS) - {"rows_past_m"}


def test_count_model_and_its_mutant():
    rng = np.random.default_rng(5)
    C, M = 7, 37  # a ragged last tile: 11 rows missing
    y, p = rng.integers(0, C, M), rng.integers(0, C, M)
    cm, counts = ec.count_model(y, p, C)
    assert np.array_equal(cm, sklearn_metrics.confusion_matrix(y, p, labels=np.arange(C)))
    assert counts.tolist() == [M, int((y == p).sum())]
    cm_bad, counts_bad = ec.count_model(y, p, C, mutant="rows_past_m")
    assert counts_bad[0] == 48 and cm_bad[0, 0] == cm[0, 0] + 11
    # a label outside [0, C) leaves its row out
    y2 = y.copy()
    y2[3], y2[20] = -1, C
    cm2, counts2 = ec.count_model(y2, p, C)
    assert counts2[0] == M - 2 and cm2.sum() == M - 2


# ---- the generators ------------------------------------------------------------------

def test_tie_operands_tie_the_two_largest_logits():
    for dtype in ec.DTYPES:
        for pair in ec.tie_pairs(41):
            X, W, b = ec.tie_operands(37, 66, 41, dtype, pair, seed=1)
            Z = ec.int_logits(X.float(), W, b)
            if pair == "all":
                assert (Z == 0).all()
                continue
            odd = Z[1::2]
            top = np.sort(odd, axis=1)[:, -2:]
            assert (top[:, 0] == top[:, 1]).all() and (odd.argmax(1) == pair[0]).all()
            assert (odd[:, pair[1]] == top[:, 1]).all()


def test_tie_pairs_cover_the_edges():
    assert ec.tie_pairs(1) == ["all"]
    assert ec.tie_pairs(2) == [(0, 1), "all"]
    assert ec.tie_pairs(17) == [(0, 1), (3, 4), (15, 16), (8, 16), "all"]
    assert ec.tie_pairs(41) == [(0, 1), (3, 4), (15, 16), (20, 40), "all"]


def test_decided_rule():
    Z = np.array([[0.0, 1.0, 0.5], [0.0, 1.0, 1.0 - 1e-7]])
    assert ec.decided_rows(Z, 1e-6).tolist() == [True, False]
    assert ec.check_random([1, 2], Z, 1e-6) == (1, 0, 0)
    assert ec.check_random([0, 0], Z, 1e-6) == (1, 1, 1)


# ---- SGC.evaluate / SGC.predict on CPU tensors ------------------------------------------

@pytest.mark.parametrize("dtype", ec.DTYPES, ids=[ec.IDS[d] for d in ec.DTYPES])
def test_evaluate_and_predict_on_cpu_equal_the_literal_expressions(dtype):
    from sgc_amd.metrics import accuracy, f1
    from sgc_amd.models import SGC
    torch.manual_seed(0)
    M, K, C = 333, 20, 7
    model = SGC(K, C)
    x = torch.randn(M, K).to(dtype)
    y = torch.randint(0, C, (M,))
    with torch.no_grad():
        out = model(x)
    ev = model.evaluate(x, y)
    assert torch.equal(model.predict(x), out.max(1)[1])
    assert torch.equal(ev.accuracy(), accuracy(out, y))
    assert ev.accuracy().dtype == torch.float64 and ev.accuracy().dim() == 0
    micro, macro = ev.f1()
    ref_micro, ref_macro = f1(out, y)
    assert abs(micro - ref_micro) <= 1e-12 and abs(macro - ref_macro) <= 1e-12
    assert int(ev.count) == M and int(ev.correct) == int((out.max(1)[1] == y).sum())
    assert np.array_equal(ev.confusion.numpy(),
                          sklearn_metrics.confusion_matrix(y.numpy(), out.max(1)[1].numpy(),
                                                           labels=np.arange(C)))
    ref_loss = torch.nn.functional.cross_entropy(out, y)
    assert abs(float(ev.loss) - float(ref_loss)) <= 1e-6 * abs(float(ref_loss))
    assert not ev.loss.requires_grad


def test_evaluate_raises_on_an_out_of_range_label():
    from sgc_amd.models import SGC
    model = SGC(5, 3)
    x = torch.randn(4, 5)
    with pytest.raises(IndexError):
        model.evaluate(x, torch.tensor([0, 1, 3, 2]))
    # torch's default ignore_index is no exception: evaluate skips no label
    with pytest.raises(IndexError, match="Target -100 is out of bounds"):
        model.evaluate(x, torch.tensor([0, 1, -100, 2]))
    model.evaluate(x, torch.tensor([0, 1, 0, 2]))  # class 0 itself is a label like any other


def test_linear_eval_cpu_leaves_bad_label_rows_out():
    from sgc_amd.propagate import linear_eval
    torch.manual_seed(1)
    x, W = torch.randn(6, 4), torch.randn(3, 4)
    y = torch.tensor([0, 1, 5, 2, -1, 1])
    ev = linear_eval(x, W, None, y)
    assert ev.counts[0].item() == 4 and ev.confusion.sum().item() == 4
    assert torch.isnan(ev.loss)
    only = linear_eval(x, W)
    assert only.confusion is None and only.counts is None and only.loss is None
    assert torch.equal(only.pred, (x @ W.t()).max(1)[1])
