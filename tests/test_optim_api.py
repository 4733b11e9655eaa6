"""CPU: E.Adam's argument checks, its state layout against torch.optim.Adam's, and the bars of tests/adam_restatement.py held by
torch's own fp32 Adam (what guards the bars the device kernel is held to in test_gpu_optim.py)."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_restatement as R  # noqa: E402

NUMELS = (1, 3, 5, 4095, 4097, 100003)


def _no_device(monkeypatch):
    """No device exists where this runs, and none may be asked for: every route to the library raises."""
    from e2e_multi_view_matching_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_lib, "context", no_device)
    monkeypatch.setattr(_lib, "load_library", no_device)


def _params(numels=(5, 7), dtype=torch.float32):
    gen = torch.Generator().manual_seed(11)
    return [torch.randn(n, generator=gen, dtype=dtype).requires_grad_() for n in numels]


@pytest.mark.parametrize("foreach", [False, True])
def test_torch_adam_in_fp32_holds_the_bars(foreach):
    """Five steps, gradient scales 1e-6 .. 50 with zeros and entries at the clip value, clip 0.1, numel 1 .. 100003, two groups
    (lr 1e-4 / 1e-5): every step of torch.optim.Adam is within the bars of its fp64 restatement from its own previous state."""
    ps = _params(NUMELS)
    opt = torch.optim.Adam([{"params": ps[:3], "lr": 1e-4}, {"params": ps[3:], "lr": 1e-5}], foreach=foreach)
    worst = [0.0, 0.0, 0.0]
    for k in range(5):
        before = []
        for i, p in enumerate(ps):
            p.grad = R.make_grad(p.shape, 100 * k + i, R.SCALES[(i + k) % 4])
            st = opt.state.get(p, {})
            before.append((p.detach().clone(), p.grad.clone(), st["exp_avg"].clone() if st else torch.zeros_like(p),
                           st["exp_avg_sq"].clone() if st else torch.zeros_like(p)))
        torch.nn.utils.clip_grad_value_(ps, R.CLIP)
        opt.step()
        for i, p in enumerate(ps):
            ref = R.adam_step(*before[i], step=k, lr=1e-4 if i < 3 else 1e-5, clip=R.CLIP)
            st = opt.state[p]
            assert float(st["step"]) == k + 1
            r = R.ratios(ref, p, st["exp_avg"], st["exp_avg_sq"])
            worst = [max(a, b) for a, b in zip(worst, r)]
    print("torch.optim.Adam (foreach=%s): worst error / bar  m %.3f  v %.3f  p %.3f" % (foreach, *worst))
    assert max(worst) <= 1.0, worst


BAD_OPTIONS = [
    ({"weight_decay": 0.01}, "weight_decay"), ({"amsgrad": True}, "amsgrad"), ({"maximize": True}, "maximize"),
    ({"capturable": True}, "capturable"), ({"differentiable": True}, "differentiable"), ({"lr": torch.tensor(1e-3)}, "tensor-valued lr"),
    ({"lr": -1e-3}, "learning rate"), ({"betas": (1.0, 0.999)}, "betas"), ({"betas": (0.9, -0.1)}, "betas"), ({"eps": -1e-8}, "epsilon"),
    ({"grad_clip": 0.0}, "grad_clip"), ({"grad_clip": -0.1}, "grad_clip"), ({"grad_clip": float("inf")}, "grad_clip"),
    ({"grad_clip": float("nan")}, "grad_clip"), ({"grad_clip": "0.1"}, "grad_clip"),
]


@pytest.mark.parametrize("kw,match", BAD_OPTIONS)
def test_bad_options_are_value_errors_at_construction_and_on_load(kw, match, monkeypatch):
    import e2e_multi_view_matching_amd as E
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match=match):
        E.Adam(_params(), **kw)
    opt = E.Adam(_params())
    with pytest.raises(ValueError, match=match):  # ... and as a group's own option
        opt.add_param_group({"params": _params((3,)), **kw})
    assert len(opt.param_groups) == 1
    sd = opt.state_dict()
    sd["param_groups"][0].update(kw)
    with pytest.raises(ValueError, match=match):
        opt.load_state_dict(sd)
    assert all(opt.param_groups[0][k] == opt.defaults[k] for k in kw)  # nothing was taken over


def test_options_of_the_whole_step_must_agree_between_groups(monkeypatch):
    import e2e_multi_view_matching_amd as E
    _no_device(monkeypatch)
    opt = E.Adam(_params(), grad_clip=0.1)
    for kw in ({"grad_clip": None}, {"skip_nonfinite": True}, {"betas": (0.8, 0.999)}, {"eps": 1e-6}):
        with pytest.raises(ValueError, match="same in every param group"):
            opt.add_param_group({"params": _params((3,)), **kw})
    opt.add_param_group({"params": _params((3,)), "lr": 1e-4})  # the reference's second group
    assert [g["lr"] for g in opt.param_groups] == [1e-3, 1e-4]


def test_step_rejects_what_the_kernel_cannot_take_before_any_device_call(monkeypatch):
    import e2e_multi_view_matching_amd as E
    _no_device(monkeypatch)

    def with_grad(p, g=None):
        p.grad = torch.ones_like(p) if g is None else g
        return p

    cases = {
        "contiguous float32": [with_grad(_params((4,), torch.float64)[0])],
        "contiguous float32 ": [with_grad(torch.zeros(4, 3).t().requires_grad_())],
        "sparse": [with_grad(_params((6,))[0], torch.ones(6).to_sparse())],
        "one device": [with_grad(_params((4,))[0]), with_grad(torch.zeros(4, device="meta", requires_grad=True))],
    }
    for match, ps in cases.items():
        opt = E.Adam(ps)
        with pytest.raises(ValueError, match=match.strip()):
            opt.step()
        assert len(opt.state) == 0
    opt = E.Adam(_params())
    opt.param_groups[0]["lr"] = torch.tensor(1e-3)  # (what a scheduler could leave behind)
    opt.param_groups[0]["params"][0].grad = torch.ones(5)
    with pytest.raises(ValueError, match="tensor-valued lr"):
        opt.step()


def test_step_on_cpu_parameters_raises_and_creates_no_state(monkeypatch):
    import e2e_multi_view_matching_amd as E
    _no_device(monkeypatch)
    ps = _params()
    opt = E.Adam(ps, grad_clip=0.1, skip_nonfinite=True)
    assert opt.step() is None and len(opt.state) == 0  # no gradient anywhere: nothing to do, as in torch
    for p in ps:
        p.grad = torch.ones_like(p)
    keep = [p.detach().clone() for p in ps]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert len(opt.state) == 0 and opt.counters() == (0, 0)
    assert all(torch.equal(a, b) and b._version == 0 for a, b in zip(keep, ps))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.has_finite_gradients(ps)
    assert E.has_finite_gradients(torch.nn.Linear(2, 2)) is True  # no gradients: the reference's answer, no device needed


def _stepped_torch_adam(ps, groups=2, steps=2):
    if groups == 2:
        opt = torch.optim.Adam([{"params": ps[:1]}, {"params": ps[1:], "lr": 1e-4}], lr=1e-3)
    else:
        opt = torch.optim.Adam(ps, lr=1e-3)
    for k in range(steps):
        for i, p in enumerate(ps):
            p.grad = R.make_grad(p.shape, 10 * k + i, 1.0)
        opt.step()
    return opt


def test_state_dicts_go_both_ways_between_torch_adam_and_this_one(monkeypatch):
    import e2e_multi_view_matching_amd as E
    _no_device(monkeypatch)
    ps = _params((5, 7, 1))
    topt = _stepped_torch_adam(ps)
    sd = copy.deepcopy(topt.state_dict())
    mine = E.Adam([{"params": [p.detach().clone().requires_grad_() for p in ps[:1]]},
                   {"params": [p.detach().clone().requires_grad_() for p in ps[1:]], "lr": 1e-4}], grad_clip=0.1, skip_nonfinite=True)
    mine.load_state_dict(sd)
    out = mine.state_dict()
    assert sorted(out["state"]) == sorted(sd["state"]) == [0, 1, 2]
    for i in sd["state"]:
        assert sorted(out["state"][i]) == ["exp_avg", "exp_avg_sq", "step"]
        for k, v in sd["state"][i].items():
            got = out["state"][i][k]
            assert torch.is_tensor(got) and got.dtype == torch.float32 and got.shape == v.shape and torch.equal(got, v), (i, k)
        assert out["state"][i]["step"].dim() == 0 and float(out["state"][i]["step"]) == 2.0
    for g_t, g_m in zip(sd["param_groups"], out["param_groups"]):
        assert set(g_m) == set(g_t) | {"grad_clip", "skip_nonfinite"}
        assert all(g_m[k] == g_t[k] for k in g_t)
        assert g_m["grad_clip"] == 0.1 and g_m["skip_nonfinite"] is True  # what the checkpoint does not say stays as constructed
    # ... and back: torch.optim.Adam takes this optimiser's dict (its two extra group keys included) and steps on
    back = torch.optim.Adam([{"params": [p.detach().clone().requires_grad_() for p in ps[:1]]},
                             {"params": [p.detach().clone().requires_grad_() for p in ps[1:]]}])
    back.load_state_dict(copy.deepcopy(out))
    assert [g["lr"] for g in back.param_groups] == [1e-3, 1e-4]
    for i, p in enumerate(q for g in back.param_groups for q in g["params"]):
        p.grad = R.make_grad(p.shape, 20 + i, 1.0)
    for i, p in enumerate(ps):
        p.grad = R.make_grad(p.shape, 20 + i, 1.0)
    back.step()
    topt.step()
    for a, b in zip(ps, (q for g in back.param_groups for q in g["params"])):
        assert torch.equal(a, b) and float(back.state[b]["step"]) == 3.0


def test_a_one_group_checkpoint_loads_into_two_groups_the_way_load_ckpt_does_it(monkeypatch):
    """helpers.load_ckpt (stage 1 -> stage 2): the saved dict has one group, the new optimiser two; the missing group is appended
    as a deep copy of the new optimiser's own and the dict is loaded."""
    import e2e_multi_view_matching_amd as E
    _no_device(monkeypatch)
    ps = _params((5, 7))
    old = copy.deepcopy(_stepped_torch_adam(ps[:1], groups=1).state_dict())
    opt = E.Adam([p.detach().clone().requires_grad_() for p in ps[:1]], lr=1e-3, grad_clip=0.1, skip_nonfinite=True)
    opt.add_param_group({"params": [ps[1].detach().clone().requires_grad_()], "lr": 1e-4})
    new = opt.state_dict()
    for n in range(len(old["param_groups"]), len(new["param_groups"])):
        old["param_groups"].append(copy.deepcopy(new["param_groups"][n]))
    opt.load_state_dict(old)
    assert [g["lr"] for g in opt.param_groups] == [1e-3, 1e-4]
    assert all(g["grad_clip"] == 0.1 and g["skip_nonfinite"] is True for g in opt.param_groups)
    p0, p1 = (g["params"][0] for g in opt.param_groups)
    assert float(opt.state[p0]["step"]) == 2.0 and opt.state[p0]["exp_avg"].abs().sum() > 0
    assert p1 not in opt.state  # created by its first step


def test_the_header_and_the_binding_declare_the_two_entries():
    from e2e_multi_view_matching_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "e2emv.h")).read()
    assert "#define E2EMV_OPTIM_CHUNK 4096" in hdr
    assert len(_lib.SIGNATURES["e2emv_adam_step"][1]) == 16 and len(_lib.SIGNATURES["e2emv_grads_finite"][1]) == 6
