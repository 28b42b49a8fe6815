"""distributed.FlatParameters (the values' twin of FlatGradients) and build_optimizer's new names, on the CPU: the parameters become
views of one buffer at FlatGradients' offsets and stay leaf nn.Parameters with their state_dict keys; whatever copies in place keeps
the views; torch.optim on top of them trains exactly as on separate tensors."""
import pytest
import torch

from mvlpt_amd.config import get_cfg_default
from mvlpt_amd.distributed import FlatGradients, FlatParameters
from mvlpt_amd.trainer import build_optimizer


def _module():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.Linear(5, 2))
    m[1].bias.requires_grad_(False)
    return m


def test_values_become_views_at_the_gradients_offsets():
    m = _module()
    want = {k: v.clone() for k, v in m.state_dict().items()}
    fp, fg = FlatParameters(m.parameters()), FlatGradients(m.parameters())
    assert fp.intact() and fp.flat.numel() == fg.flat.numel() == 15 + 5 + 10
    assert [p is q for p, q in zip(fp.params, fg.params)] == [True] * 3 and all(p is not m[1].bias for p in fp.params)
    off = 0
    for p, v, o in zip(fp.params, fp.views, fp.offsets):
        assert isinstance(p, torch.nn.Parameter) and p.is_leaf and p.requires_grad
        assert o == off and p.data_ptr() == fp.flat.data_ptr() + 4 * off == v.data_ptr()
        off += p.numel()
    assert list(m.state_dict()) == list(want) and all(torch.equal(v, want[k]) for k, v in m.state_dict().items())
    m(torch.randn(4, 3)).sum().backward()
    fg.zero_()                                                 # adopts the gradients: same offsets as the values
    for p, o in zip(fg.params, fp.offsets):
        assert p.grad.data_ptr() == fg.flat.data_ptr() + 4 * o


def test_in_place_loads_keep_the_views_and_attach_adopts_a_replaced_tensor():
    m = _module()
    fp = FlatParameters(m.parameters())
    other = {k: torch.randn_like(v) for k, v in m.state_dict().items()}
    m.load_state_dict(other)
    assert fp.intact() and torch.equal(fp.flat[:15].view(5, 3), other["0.weight"])
    with torch.no_grad():
        m[0].weight.add_(1.0)
    assert fp.intact() and torch.equal(fp.views[0], other["0.weight"] + 1.0)
    m[0].weight.data = torch.zeros(5, 3)                       # storage of its own again
    assert not fp.intact()
    fp.attach()
    assert fp.intact() and torch.equal(fp.flat[:15], torch.zeros(15))
    with pytest.raises(TypeError):
        FlatParameters([torch.nn.Parameter(torch.zeros(2, dtype=torch.float64))])


def test_torch_optim_over_the_views_trains_as_over_separate_tensors():
    a, b = _module(), _module()
    FlatParameters(b.parameters())
    x = torch.randn(6, 3)
    oa, ob = torch.optim.SGD(a.parameters(), lr=0.1, momentum=0.9), torch.optim.SGD(b.parameters(), lr=0.1, momentum=0.9)
    for _ in range(3):
        for m, o in ((a, oa), (b, ob)):
            o.zero_grad()
            m(x).pow(2).sum().backward()
            o.step()
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))


def test_build_optimizer_names():
    m = _module()
    cfg = get_cfg_default()
    assert cfg.OPTIM.FUSED is False
    cfg.OPTIM.NAME = "adamw"
    opt = build_optimizer(m, cfg.OPTIM)
    assert type(opt) is torch.optim.AdamW and opt.param_groups[0]["weight_decay"] == cfg.OPTIM.WEIGHT_DECAY
    cfg.OPTIM.NAME = "rmsprop"
    with pytest.raises(ValueError):
        build_optimizer(m, cfg.OPTIM)
    cfg.OPTIM.FUSED = True                                     # refused by name / by request before any device is needed
    with pytest.raises(ValueError):
        build_optimizer(m, cfg.OPTIM)
    cfg.OPTIM.NAME, cfg.OPTIM.AMSGRAD = "adam", True
    with pytest.raises(ValueError):
        build_optimizer(m, cfg.OPTIM, (None, None))
    cfg.OPTIM.AMSGRAD = False
    with pytest.raises(ValueError):
        build_optimizer(m, cfg.OPTIM)                          # the fused route needs the flat buffers
