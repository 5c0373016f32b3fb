"""CPU suite: the optimiser state conversions of ldmseg_amd/optim.py (`state_from_torch` / `state_to_torch`, plain functions on
dicts of tensors) carry a torch.optim.AdamW state without loss: a state stepped three times, converted to the library's packed form
and back, loaded into a second torch AdamW, continues bitwise like the first."""
import copy

import pytest
import torch


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    shapes = [(5, 3), (7,), (2, 2, 3), (4,), (6,)]
    return [torch.randn(s, generator=g).requires_grad_(True) for s in shapes]


def _groups(ps):
    # two groups with their own lr / weight_decay; ps[3] never gets a gradient, so it never gets a state entry
    return [{"params": ps[:2], "lr": 3e-3, "weight_decay": 0.05}, {"params": ps[2:], "lr": 1e-2, "weight_decay": 0.0, "betas": (0.8, 0.99)}]


def _set_grads(ps, step):
    g = torch.Generator().manual_seed(100 + step)
    for i, p in enumerate(ps):
        p.grad = None if i == 3 else torch.randn(p.shape, generator=g) * 10.0 ** (-step)


def test_three_torch_steps_survive_the_round_trip_bitwise():
    from ldmseg_amd.optim import state_from_torch, state_to_torch
    a = _params()
    opt_a = torch.optim.AdamW(_groups(a), eps=1e-8)
    for step in range(3):
        _set_grads(a, step)
        opt_a.step()
    packed = state_from_torch(opt_a.state_dict())
    # the packed form: integer steps, index lists, the four hyper-parameters per group; no entry for the parameter without gradient
    assert sorted(packed["state"]) == [0, 1, 2, 4]
    assert all(s["step"] == 3 and isinstance(s["step"], int) for s in packed["state"].values())
    assert [g["params"] for g in packed["param_groups"]] == [[0, 1], [2, 3, 4]]
    assert packed["param_groups"][0] == {"lr": 3e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.05, "params": [0, 1]}
    assert packed["param_groups"][1]["betas"] == (0.8, 0.99) and packed["param_groups"][1]["weight_decay"] == 0.0
    back = state_to_torch(packed)
    ref = opt_a.state_dict()
    assert set(back["state"]) == set(ref["state"])
    for i, s in ref["state"].items():
        assert set(back["state"][i]) == set(s)
        for k in s:
            assert back["state"][i][k].dtype == s[k].dtype and torch.equal(back["state"][i][k], s[k]), (i, k)
    for gb, gr in zip(back["param_groups"], ref["param_groups"]):
        assert {k: gb[k] for k in gr} == dict(gr)                      # every key torch keeps, with torch's value
    # a second torch optimiser over copies of the parameters, with other hyper-parameters until the load
    b = [p.detach().clone().requires_grad_(True) for p in a]
    opt_b = torch.optim.AdamW([{"params": b[:2]}, {"params": b[2:]}], lr=1.0, weight_decay=0.5)
    opt_b.load_state_dict(copy.deepcopy(back))
    _set_grads(a, 3)
    _set_grads(b, 3)
    opt_a.step()
    opt_b.step()
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), i
    for i in (0, 1, 2, 4):
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(opt_a.state[a[i]][k], opt_b.state[b[i]][k]), (i, k)
    assert b[3] not in opt_b.state or not opt_b.state[b[3]]


def test_the_library_optimiser_speaks_the_same_layout_without_a_device():
    """AdamW.state_dict() / load_state_dict() on CPU tensors (no step is taken: that needs the device): torch's dict goes in, the
    same dict comes out, and torch's optimiser accepts it"""
    from ldmseg_amd.optim import AdamW
    a = _params()
    opt_a = torch.optim.AdamW(_groups(a))
    for step in range(2):
        _set_grads(a, step)
        opt_a.step()
    b = [p.detach().clone().requires_grad_(True) for p in a]
    ours = AdamW([{"params": b[:2]}, {"params": b[2:]}], lr=0.5)
    groups = ours.param_groups
    assert ours.param_groups[0]["lr"] == 0.5 and ours.param_groups[0]["weight_decay"] == 1e-2 and ours.state_dict()["state"] == {}
    ours.load_state_dict(opt_a.state_dict())
    assert ours.param_groups is groups and groups[0]["lr"] == 3e-3 and groups[1]["betas"] == (0.8, 0.99)
    assert ours.state[b[0]]["step"] == 2 and b[3] not in ours.state
    sd = ours.state_dict()
    ref = opt_a.state_dict()
    assert sd["param_groups"] == ref["param_groups"]
    for i, s in ref["state"].items():
        for k in s:
            assert torch.equal(sd["state"][i][k], s[k]), (i, k)
    assert ours.state[b[0]]["exp_avg"].data_ptr() != opt_a.state[a[0]]["exp_avg"].data_ptr()      # loaded moments are copies
    torch.optim.AdamW([{"params": b[:2]}, {"params": b[2:]}]).load_state_dict(sd)
    ours.zero_grad()
    with pytest.raises(ValueError):
        ours.load_state_dict({"state": {}, "param_groups": ref["param_groups"][:1]})
    with pytest.raises(ValueError):
        AdamW([{"params": b[:2], "momentum": 0.9}])


@pytest.mark.parametrize("key", ["amsgrad", "maximize"])
def test_unsupported_variants_are_refused(key):
    from ldmseg_amd.optim import state_from_torch
    p = torch.zeros(3, requires_grad=True)
    opt = torch.optim.AdamW([p], **{key: True})
    p.grad = torch.ones(3)
    opt.step()
    with pytest.raises(NotImplementedError):
        state_from_torch(opt.state_dict())
