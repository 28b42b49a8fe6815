"""CPU checks of the host side of the text tower's shared prefix (TRAINER.MVLPT.TEXT_SHARED_PREFIX, Engine.set_text_shared_prefix):
the prefix length read off the prompt learner's layout tables for every class-token position, the cases that give none, what reaches
the engine, and the clamping rule the engine applies (restated in mvlpt_amd.model.clamp_shared_prefix)."""
import types

import pytest
import torch

from tests import deep_text_ref as R
from tests.fake_engine import OracleEngine, OracleFrozenCLIP

NAMES = ["dog", "great white shark", "grand piano", "cat", "big old oak tree"]
N_CTX = 4


def _learner(position="middle", csc=False, n_ctx=N_CTX):
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.model import MultitaskVLPromptLearner
    from mvlpt_amd.weights import make_state_dict
    arch = R.deep_arch()
    sd = make_state_dict(arch, seed=11)
    clip = OracleFrozenCLIP(sd, arch)
    clip.engine = OracleEngine(sd, arch)
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (32, 32)
    T = cfg.TRAINER.MVLPT
    T.COOP.N_CTX, T.COOP.CSC, T.COOP.CLASS_TOKEN_POSITION = n_ctx, csc, position
    T.VPT.N_CTX, T.PROJECT_METHOD, T.PROJECT_DIM = 0, "identity", 64
    return MultitaskVLPromptLearner(cfg, NAMES, clip), clip


class _Recorder:
    def __init__(self):
        self.calls = []

    def set_text_shared_prefix(self, p):
        self.calls.append(int(p))


ANY = -10 ** 9      # a threshold every class table passes (five classes of 77 positions ADD rows under a shared prefix)


def _model(pl, clip, enabled=True, min_rows=ANY):
    return types.SimpleNamespace(engine=_Recorder(), clip_model=clip, text_shared_prefix=enabled, prompt_learner=pl,
                                 shared_prefix_min_rows=min_rows)


def test_config_default_is_on():
    from mvlpt_amd.config import get_cfg_default
    assert get_cfg_default().TRAINER.MVLPT.TEXT_SHARED_PREFIX is True


@pytest.mark.parametrize("position,want", [("middle", 1 + N_CTX // 2), ("end", 1 + N_CTX), ("front", 1)])
def test_prefix_length_from_the_layout(position, want):
    from mvlpt_amd.model import shared_prefix_len
    pl, _ = _learner(position)
    assert shared_prefix_len(pl.layout, pl.token_prefix, generic=True) == want
    # the columns counted hold the prefix entry or a context entry, the next one does not (or differs between classes)
    lay = pl.layout
    assert bool((lay[:, :want] <= 0).all()) and bool((lay[:, :want] == lay[:1, :want]).all())
    assert bool((lay[:, want] > 0).any()) or not bool((lay[:, want] == lay[0, want]).all())


def test_class_specific_context_gives_none():
    from mvlpt_amd.model import apply_text_shared_prefix, shared_prefix_len
    pl, clip = _learner("end", csc=True)
    assert shared_prefix_len(pl.layout, pl.token_prefix, generic=False) == 0
    m = _model(pl, clip)
    assert apply_text_shared_prefix(m, pl, pl.layout, generic=pl.ctx.dim() == 2) == 0 and m.engine.calls == [0]


def test_one_differing_prefix_row_gives_none():
    from mvlpt_amd.model import shared_prefix_len
    pl, _ = _learner("end")
    tp = pl.token_prefix.clone()
    assert shared_prefix_len(pl.layout, tp, generic=True) == 1 + N_CTX
    flat = tp.view(tp.shape[0], -1)
    flat[3, 7] = torch.nextafter(flat[3, 7], flat[3, 7] + 1)      # one bit in one row
    assert shared_prefix_len(pl.layout, tp, generic=True) == 0
    tz = pl.token_prefix.clone()
    tz.view(tz.shape[0], -1)[:, 0] = 0.0
    assert shared_prefix_len(pl.layout, tz, generic=True) == 1 + N_CTX
    tz.view(tz.shape[0], -1)[0, 0] = -0.0                       # equal as numbers, not as bits
    assert shared_prefix_len(pl.layout, tz, generic=True) == 0


def test_a_differing_layout_column_ends_the_prefix():
    from mvlpt_amd.model import shared_prefix_len
    pl, _ = _learner("end")
    lay = pl.layout.clone()
    lay[2, 2], lay[2, 3] = lay[2, 3].clone(), lay[2, 2].clone()      # class 2 has two context rows swapped
    assert shared_prefix_len(lay, pl.token_prefix, generic=True) == 2


def test_switch_off_gives_none_and_the_engine_hears_it():
    from mvlpt_amd.model import apply_text_shared_prefix, shared_prefix_len
    pl, clip = _learner("middle")
    assert shared_prefix_len(pl.layout, pl.token_prefix, generic=True, enabled=False) == 0
    off, on = _model(pl, clip, enabled=False), _model(pl, clip)
    assert apply_text_shared_prefix(off, pl, pl.layout, generic=True) == 0 and off.engine.calls == [0]
    assert apply_text_shared_prefix(on, pl, pl.layout, generic=True) == 1 + N_CTX // 2 and on.engine.calls == [1 + N_CTX // 2]
    # the table is read back once: the second call answers from the cache, a class shard has its own entry
    key = on._shared_prefix[0]
    assert apply_text_shared_prefix(on, pl, pl.layout, generic=True) == 1 + N_CTX // 2 and on._shared_prefix[0] == key
    assert apply_text_shared_prefix(on, pl, pl.layout, generic=True, classes=(1, 4)) == 1 + N_CTX // 2 and on._shared_prefix[0] != key
    # deep prompts / a non-generic context at the call site: the engine is told 0 whatever the cache holds
    assert apply_text_shared_prefix(on, pl, pl.layout, generic=False) == 0 and on.engine.calls[-1] == 0


def test_a_class_table_that_removes_too_few_rows_runs_in_full():
    """C * P - (L - P) rows leave the forward; below the model's threshold (MIN_SHARED_PREFIX_ROWS by default) the engine is told 0."""
    from mvlpt_amd.model import MIN_SHARED_PREFIX_ROWS, apply_text_shared_prefix
    assert MIN_SHARED_PREFIX_ROWS == 512
    pl, clip = _learner("end")
    C_, L, P = pl.layout.shape[0], pl.layout.shape[1], 1 + N_CTX
    saved = C_ * P - (L - P)
    for min_rows, want in ((saved, P), (saved + 1, 0), (ANY, P)):
        m = _model(pl, clip, min_rows=min_rows)
        assert apply_text_shared_prefix(m, pl, pl.layout, generic=True) == want and m.engine.calls == [want], (min_rows, want)
    default = types.SimpleNamespace(engine=_Recorder(), clip_model=clip, text_shared_prefix=True)      # five classes: far below 512
    assert apply_text_shared_prefix(default, pl, pl.layout, generic=True) == 0 and default.engine.calls == [0]
    # the headline's table (100 classes, L = 77, P = 9) and the 2191-class one at P = 3 are above it
    assert 100 * 9 - (77 - 9) >= MIN_SHARED_PREFIX_ROWS and 2191 * 3 - (30 - 3) >= MIN_SHARED_PREFIX_ROWS


def test_an_engine_without_the_setting_is_left_alone():
    from mvlpt_amd.model import apply_text_shared_prefix
    pl, clip = _learner("middle")
    m = types.SimpleNamespace(engine=object(), clip_model=clip, text_shared_prefix=True)
    assert apply_text_shared_prefix(m, pl, pl.layout, generic=True) == 0


@pytest.mark.parametrize("prefix,L,Lg,want", [
    (9, 77, 24, 9),       # the headline: 9 <= 24 - 9
    (17, 77, 24, 12),     # "end" with 16 context rows: lowered to Lg / 2
    (17, 77, 77, 17),
    (4, 12, 12, 4),
    (9, 20, 11, 5),       # P <= Lg - P
    (3, 20, 5, 2),        # Lg - P >= 3 and P <= Lg - P
    (2, 20, 4, 1),        # Lg - P >= 3
    (1, 20, 3, 0),        # nothing fits
    (40, 20, 20, 10),     # never the whole sequence
    (0, 77, 24, 0),
])
def test_clamping_rule(prefix, L, Lg, want):
    from mvlpt_amd.model import TEXT_MIN_L, clamp_shared_prefix
    assert TEXT_MIN_L == 3
    p = clamp_shared_prefix(prefix, L, Lg)
    assert p == want
    assert p == 0 or (p <= Lg - p and Lg - p >= 3 and p < L and p <= prefix)
    # the largest such value
    if p < min(prefix, L - 1):
        q = p + 1
        assert not (q <= Lg - q and Lg - q >= 3)
