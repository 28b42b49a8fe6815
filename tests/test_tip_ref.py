"""CPU checks of the Tip-Adapter oracle (tests/tip_ref.py): it equals the published dense formulation, the winner rule is the first
strict maximum, and the search cases of tests/test_hip_tip.py are decidable: at every grid point at least 99 % of the rows have a
float64 margin above twice the logit bound, so the device's counts are pinned between `sure` and `sure + undecided`."""
import numpy as np
import pytest
import torch

from tests import tip_ref as R


def published(F, y, K, key_cls, W, n_cls, alpha, beta, s):
    """The published code in float64 torch: exp(-beta (1 - F K^T)) @ one_hot, F.cross_entropy, autograd to the keys."""
    F, W = torch.from_numpy(np.asarray(F, np.float64)), torch.from_numpy(np.asarray(W, np.float64))
    K = torch.from_numpy(np.asarray(K, np.float64)).requires_grad_(True)
    one_hot = torch.nn.functional.one_hot(torch.from_numpy(np.asarray(key_cls, np.int64)), n_cls).double()
    affinity = F @ K.t()
    cache_logits = ((-1) * (beta - beta * affinity)).exp() @ one_hot
    z = s * F @ W.t() + cache_logits * alpha
    loss = torch.nn.functional.cross_entropy(z, torch.from_numpy(np.asarray(y, np.int64)))
    loss.backward()
    return z.detach().numpy(), float(loss.detach()), K.grad.numpy()


@pytest.mark.parametrize("case", [(1, 64, (1, 1)), (17, 8, (1, 3, 0, 2, 9)), (33, 12, (2,) * 7 + (0, 1))], ids=str)
@pytest.mark.parametrize("hp", R.HEAD_HPARAMS + [(0.0, 2.0)], ids=str)
def test_reference_is_the_published_formulation(case, hp):
    N, D, counts = case
    alpha, beta = hp
    c = R.make_case(N, D, counts, R.SIGMA, R.case_seed(*case))
    ref = R.train(c["F"], c["y"], c["K"], c["key_ptr"], c["key_cls"], c["W"], alpha, beta)
    z, loss, dK = published(c["F"], c["y"], c["K"], c["key_cls"], c["W"], len(counts), alpha, beta, R.SCALE)
    np.testing.assert_allclose(ref["z"], z, rtol=1e-13, atol=1e-12)
    np.testing.assert_allclose(R.logits(c["F"], c["K"], c["key_ptr"], c["W"], alpha, beta), z, rtol=1e-13, atol=1e-12)
    assert abs(ref["loss"] - loss) <= 1e-12 * (1 + abs(loss))
    np.testing.assert_allclose(ref["dK"], dK, rtol=1e-10, atol=1e-15)
    if beta == 0.0:      # the cache term is alpha n_c, the gradient 0
        np.testing.assert_array_equal(R.seg_sum(ref["A"], c["key_ptr"]), np.diff(c["key_ptr"])[None, :].repeat(N, 0))
        assert not ref["dK"].any()


def test_key_table_is_a_stable_sort():
    labels = [3, 0, 3, 1, 0, 5, 3]
    order, key_ptr = R.key_table(labels, 7)
    assert order.tolist() == [1, 4, 3, 0, 2, 6, 5]
    assert key_ptr.tolist() == [0, 2, 3, 3, 6, 6, 7, 7]


def test_winner_is_the_first_strict_maximum():
    counts = np.array([[1, 5, 5], [5, 2, 5], [0, 5, 1]])
    assert R.winner(counts) == (0, 1)
    best, win = -1, None
    for b in range(3):          # the published loop
        for a in range(3):
            if counts[b, a] > best:
                best, win = counts[b, a], (b, a)
    assert win == R.winner(counts)
    assert R.winner(np.zeros((4, 2), np.int64)) == (0, 0)


def test_published_grid():
    betas, alphas = R.published_grid()
    assert len(betas) == 200 and len(alphas) == 20
    assert betas[0] == 0.1 and alphas[0] == 0.1
    assert abs(betas[-1] - (199 * 6.9 / 200 + 0.1)) < 1e-15 and abs(alphas[-1] - (19 * 2.9 / 20 + 0.1)) < 1e-15


@pytest.mark.parametrize("case", R.SEARCH_CASES, ids=str)
def test_search_cases_are_decidable(case):
    N, D, counts = case
    c = R.make_case(N, D, counts, R.SIGMA, R.case_seed(*case))
    betas, alphas = np.float32(R.SEARCH_BETAS), np.float32(R.SEARCH_ALPHAS)
    s = R.search(c["F"], c["y"], c["K"], c["key_ptr"], c["W"], betas, alphas)
    share = 1.0 - s["undecided"].max() / N
    acc = s["counts"] / N
    print(f"{case[:2]}: decided share >= {share:.4%}, accuracy {acc.min():.3f} .. {acc.max():.3f}")
    assert share >= 0.99
    assert len(np.unique(s["counts"])) > 1      # the grid matters: these cases are unbalanced
    if N <= 257:
        assert not s["undecided"].any()         # tests/test_hip_tip.py compares these with tip_logits point by point


def test_published_grid_case_is_decidable():
    case = R.SEARCH_CASES[0]
    c = R.make_case(*case, R.SIGMA, R.case_seed(*case))
    betas, alphas = R.published_grid()
    s = R.search(c["F"], c["y"], c["K"], c["key_ptr"], c["W"], np.float32(betas), np.float32(alphas))
    # 4 000 grid points walk some row's two best classes through a tie: with 96 rows one undecided row is already 1.04 % of a grid
    # point, so the share is taken over the whole grid here; the device test brackets every count by `sure` and `undecided` anyway
    assert 1.0 - s["undecided"].sum() / (case[0] * s["undecided"].size) >= 0.99
    assert len(np.unique(s["counts"])) > 1


def test_winner_case_has_one_best_grid_point():
    """tests/test_hip_tip_adapter.py asserts that search_hp returns the reference's winner: every device count lies within `undecided`
    of the reference's, so the winner is pinned when it leads every other grid point by more than twice the undecided rows."""
    d = R.make_case(*R.WINNER_CASE, R.WINNER_SIGMA, R.WINNER_SEED)
    betas, alphas = R.published_grid(step=R.WINNER_STEP)
    s = R.search(d["F"], d["y"], d["K"], d["key_ptr"], d["W"], np.float32(betas), np.float32(alphas))
    wb, wa = R.winner(s["counts"])
    others = s["counts"].copy()
    others[wb, wa] = -1
    assert s["counts"][wb, wa] - others.max() > 2 * s["undecided"].max()
    assert (wb, wa) != (0, 0) and len(np.unique(s["counts"])) > 5
