"""The chunk planner of the per-image text towers (mvlpt_amd.per_image_text), CPU only.  `PerImageTextCLIP.chunks` is a greedy cut over
per-image range widths; CoCoOp and TPT used to plan with a binary search over a uniform image count.  With every range full the two
give the same chunks whenever the engine's workspace figure does not decrease with the sequence count: that condition is what lets one
planner serve all three models, so it is a test (tests/test_hip_per_image_text.py asserts the condition itself on a live engine)."""
from types import SimpleNamespace

import pytest


def affine(S, L, save):
    return 4096 + S * L * (96 if save else 8)


def stepped(S, L, save):
    """Flat over runs of 48 sequences, then a jump: equal figures for neighbouring image counts."""
    return 1024 + -(-S // 48) * 48 * L * (96 if save else 8)


def planner(workspace_bytes, n_cls, budget):
    from mvlpt_amd.per_image_text import PerImageTextCLIP
    model = PerImageTextCLIP()
    model.engine = SimpleNamespace(text_workspace_bytes=workspace_bytes)
    model.prompt_learner = SimpleNamespace(n_cls=n_cls)
    model.max_text_workspace_bytes = budget
    return model


def uniform_images_per_chunk(workspace_bytes, budget, B, n_cls, L, save):
    """The rule the binary search implemented: the largest n <= min(B, MAX_SEQUENCES_PER_TOWER // n_cls) whose full-range tower fits
    the budget, and at least 1."""
    from mvlpt_amd.model import MAX_SEQUENCES_PER_TOWER
    fitting = [n for n in range(1, min(B, MAX_SEQUENCES_PER_TOWER // n_cls) + 1) if workspace_bytes(n * n_cls, L, save) <= budget]
    return max(fitting, default=1)


def check(workspace_bytes, budget, B, n_cls, L, save):
    model = planner(workspace_bytes, n_cls, budget)
    n = uniform_images_per_chunk(workspace_bytes, budget, B, n_cls, L, save)
    want = [(g0, min(B, g0 + n), (min(B, g0 + n) - g0) * n_cls) for g0 in range(0, B, n)]
    assert model.chunks([0] * B, [n_cls] * B, L, save) == want, (budget, B, n_cls, save)
    assert model.images_per_chunk(B, L, save) == n
    return n


@pytest.mark.parametrize("workspace_bytes", [affine, stepped])
@pytest.mark.parametrize("n_cls", [1, 5, 100])
@pytest.mark.parametrize("B", [1, 7, 100])
def test_greedy_chunks_over_full_ranges_are_the_uniform_chunks(workspace_bytes, n_cls, B):
    L = 77
    for save in (False, True):
        need = [workspace_bytes(n * n_cls, L, save) for n in range(1, B + 1)]
        budgets = {need[0] // 2, need[0] - 1, need[-1] + 1, 2 * need[-1]}      # below one image's need ... above the whole batch's
        for b in need[::max(1, B // 12)] + need[-2:]:
            budgets |= {b - 1, b, b + 1}
        seen = {check(workspace_bytes, budget, B, n_cls, L, save) for budget in sorted(budgets)}
        assert {1, B} <= seen                                                # both ends of the sweep were reached


@pytest.mark.parametrize("workspace_bytes", [affine, stepped])
def test_the_sequence_limit_binds_before_the_budget(workspace_bytes):
    from mvlpt_amd.model import MAX_SEQUENCES_PER_TOWER
    L, B = 77, 10
    for save in (False, True):
        n_cls = MAX_SEQUENCES_PER_TOWER // 6 - 1               # six images stay under the limit, seven do not
        budget = 2 * workspace_bytes(B * n_cls, L, save)
        assert check(workspace_bytes, budget, B, n_cls, L, save) == 6
        assert check(workspace_bytes, workspace_bytes(4 * n_cls, L, save), B, n_cls, L, save) == 4      # and the budget where it is tighter
        assert check(workspace_bytes, budget, 3, MAX_SEQUENCES_PER_TOWER + 1, L, save) == 1             # one image alone is over the limit
