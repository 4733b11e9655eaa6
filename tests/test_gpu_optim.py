"""GPU: e2emv_adam_step / e2emv_grads_finite (csrc/optim.hip) and their front E.Adam / E.has_finite_gradients against the fp64
restatement of tests/adam_restatement.py, step by step from the device's own previous state, at the sizes where the kernels change
path: below / at / above a vector of four, a chunk, two chunks and a tail, an empty tensor, a tensor whose storage is not 16-byte
aligned (the scalar path), and more chunks than the grid has workgroups."""
import copy
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

C = 4096
LRS = (1e-4, 1e-5)
# (the first tensor is the 0-dim one, the last the longest; index 5 is empty, index 9 starts 4 bytes off a 16-byte boundary)
SHAPES = [(), (1,), (3,), (4,), (5,), (0,), (C - 1,), (C,), (C + 1,), "misaligned", (2 * C + 3,)]
SPLIT = 6  # group 0: SHAPES[:6] at lr 1e-4, group 1: the rest at 1e-5
MISALIGNED = SHAPES.index("misaligned")


def test_the_chunk_size_is_the_headers():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "#define E2EMV_OPTIM_CHUNK %d " % C in open(os.path.join(root, "include", "e2emv.h")).read()


def _make_params(gpu):
    gen = torch.Generator().manual_seed(3)
    ps = []
    for s in SHAPES:
        if s == "misaligned":
            p = torch.empty(C + 6, device=gpu)[1:]
            p.copy_(torch.randn(C + 5, generator=gen))
            assert p.data_ptr() % 16 == 4
        else:
            p = torch.randn(s, generator=gen).to(gpu)
        ps.append(p.requires_grad_())
    return ps


def _make(gpu, **kw):
    import e2e_multi_view_matching_amd as E
    ps = _make_params(gpu)
    opt = E.Adam([{"params": ps[:SPLIT], "lr": LRS[0]}, {"params": ps[SPLIT:], "lr": LRS[1]}], **kw)
    return ps, opt


def _lr(i):
    return LRS[0] if i < SPLIT else LRS[1]


def _set_grads(ps, k):
    for i, p in enumerate(ps):
        p.grad = R.make_grad(p.shape, 1000 * k + i, R.SCALES[(i + k) % 4]).to(p.device)


def _snapshot(ps, opt):
    out = []
    for p in ps:
        st = opt.state.get(p, {})
        out.append((p.detach().clone(), None if p.grad is None else p.grad.clone(), st["exp_avg"].clone() if st else torch.zeros_like(p),
                    st["exp_avg_sq"].clone() if st else torch.zeros_like(p), float(st["step"]) if st else 0.0))
    return out


def _check_against_restatement(ps, opt, before, clip, what, keep=None, factor=1.0):
    worst = [0.0, 0.0, 0.0]
    for i, p in enumerate(ps):
        b = before[i]
        ref = R.adam_step(b[0], b[1], b[2], b[3], step=b[4], lr=_lr(i), clip=clip)
        st = opt.state[p]
        r = R.ratios(ref, p, st["exp_avg"], st["exp_avg_sq"], keep=None if keep is None else keep.get(i))
        worst = [max(a, x) for a, x in zip(worst, r)]
    print("%s: worst error / bar  m %.3f  v %.3f  p %.3f" % (what, *worst))
    assert max(worst) <= factor, (what, worst)


def _assert_unchanged(ps, opt, before):
    for i, p in enumerate(ps):
        b = before[i]
        assert torch.equal(p.detach(), b[0]), i
        st = opt.state.get(p, {})
        if st:
            assert torch.equal(st["exp_avg"], b[2]) and torch.equal(st["exp_avg_sq"], b[3]) and float(st["step"]) == b[4], i


@pytest.mark.parametrize("clip", [R.CLIP, None])
def test_five_steps_each_within_the_bars_of_the_restatement(gpu, clip):
    ps, opt = _make(gpu, grad_clip=clip)
    for k in range(5):
        _set_grads(ps, k)
        before = _snapshot(ps, opt)
        versions = [p._version for p in ps]
        opt.step()
        for i, p in enumerate(ps):
            st = opt.state[p]
            assert st["step"].device == p.device and st["step"].dtype == torch.float32 and st["step"].dim() == 0
            assert float(st["step"]) == k + 1, (i, k)
            assert p._version > versions[i]
            assert torch.equal(p.grad, before[i][1])  # the clip happens inside the step: the gradient is read, not written
        _check_against_restatement(ps, opt, before, clip, f"clip {clip} step {k + 1}")
    assert opt.counters() == (5, 0)
    assert not any(g["skip_nonfinite"] for g in opt.param_groups)


def test_step_does_not_synchronise_with_the_host(gpu):
    """``torch.cuda.set_sync_debug_mode("error")`` around steps two and three (the first creates the state), the third after a change
    of the learning rate, which makes the library upload its table again; counters() is the call that does synchronise."""
    ps, opt = _make(gpu, grad_clip=R.CLIP, skip_nonfinite=True)
    _set_grads(ps, 0)
    opt.step()
    _set_grads(ps, 1)
    before = _snapshot(ps, opt)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()
        opt.param_groups[1]["lr"] = LRS[1] * 0.5
        opt.step()
        with pytest.raises(RuntimeError):
            opt.counters()
    finally:
        torch.cuda.set_sync_debug_mode("default")
        opt.param_groups[1]["lr"] = LRS[1]
    assert opt.counters() == (3, 0)
    assert all(float(opt.state[p]["step"]) == 3.0 for p in ps)
    assert not torch.equal(ps[-1].detach(), before[-1][0])


def _poison(ps, where, value):
    if where == "last":
        ps[-1].grad.view(-1)[-1] = value
    else:
        ps[0].grad.fill_(value)  # (0-dim: its element 0)


@pytest.mark.parametrize("where,value", [("last", float("nan")), ("first", float("inf"))])
def test_a_nonfinite_gradient_anywhere_skips_the_whole_step(gpu, where, value):
    ps, opt = _make(gpu, grad_clip=R.CLIP, skip_nonfinite=True)
    K = 2
    for k in range(K):
        _set_grads(ps, k)
        opt.step()
    _set_grads(ps, K)
    _poison(ps, where, value)
    before = _snapshot(ps, opt)
    opt.step()
    _assert_unchanged(ps, opt, before)
    assert opt.counters() == (K, 1)
    _set_grads(ps, K + 1)  # the next clean step is step K + 1 of every tensor
    before = _snapshot(ps, opt)
    assert all(b[4] == K for b in before)
    opt.step()
    assert all(float(opt.state[p]["step"]) == K + 1 for p in ps)
    _check_against_restatement(ps, opt, before, R.CLIP, f"clean step after a skipped one ({where})")
    assert opt.counters() == (K + 1, 1)


def test_a_skipped_first_step_leaves_zero_moments_and_step_zero(gpu):
    ps, opt = _make(gpu, skip_nonfinite=True)
    _set_grads(ps, 0)
    _poison(ps, "last", float("-inf"))
    keep = [p.detach().clone() for p in ps]
    opt.step()
    for p, q in zip(ps, keep):
        st = opt.state[p]
        assert torch.equal(p.detach(), q) and float(st["step"]) == 0.0
        assert not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    assert opt.counters() == (0, 1)


def test_without_the_gate_a_nan_reaches_exactly_its_own_element(gpu):
    ps, opt = _make(gpu, grad_clip=R.CLIP, skip_nonfinite=False)
    _set_grads(ps, 0)
    opt.step()
    _set_grads(ps, 1)
    _poison(ps, "last", float("nan"))
    before = _snapshot(ps, opt)
    opt.step()
    last = len(ps) - 1
    n = ps[last].numel()
    for i, p in enumerate(ps):
        st = opt.state[p]
        for t in (p.detach(), st["exp_avg"], st["exp_avg_sq"]):
            bad = torch.isnan(t.view(-1)).nonzero().view(-1).tolist()
            assert bad == ([n - 1] if i == last else []), (i, bad)
        assert float(st["step"]) == 2.0
    keep = {last: torch.arange(n) != n - 1}
    _check_against_restatement(ps, opt, before, R.CLIP, "every other element of the NaN step", keep=keep)
    assert opt.counters() == (2, 0)


def test_a_parameter_without_a_gradient_keeps_its_bits_and_gets_no_state(gpu):
    ps, opt = _make(gpu, grad_clip=R.CLIP, skip_nonfinite=True)
    idle = (3, 8)
    for k in range(2):
        _set_grads(ps, k)
        for i in idle:
            ps[i].grad = None
        keep = {i: (ps[i].detach().clone(), ps[i]._version) for i in idle}
        before = _snapshot(ps, opt)
        opt.step()
        for i in idle:
            assert torch.equal(ps[i].detach(), keep[i][0]) and ps[i]._version == keep[i][1] and ps[i] not in opt.state
        active = [i for i in range(len(ps)) if i not in idle]
        worst = [0.0, 0.0, 0.0]
        for i in active:
            b = before[i]
            ref = R.adam_step(b[0], b[1], b[2], b[3], step=b[4], lr=_lr(i), clip=R.CLIP)
            st = opt.state[ps[i]]
            assert float(st["step"]) == k + 1
            worst = [max(a, x) for a, x in zip(worst, R.ratios(ref, ps[i], st["exp_avg"], st["exp_avg_sq"]))]
        assert max(worst) <= 1.0, worst
    # a parameter that joins later starts at step 1 while its neighbours are at step 3
    _set_grads(ps, 2)
    before = _snapshot(ps, opt)
    opt.step()
    assert [float(opt.state[p]["step"]) for p in ps] == [1.0 if i in idle else 3.0 for i in range(len(ps))]
    _check_against_restatement(ps, opt, before, R.CLIP, "mixed step counts")


def test_step_four_continues_on_torch_adam_from_the_devices_state(gpu):
    ps, opt = _make(gpu)
    for k in range(3):
        _set_grads(ps, k)
        opt.step()
    cpu = [p.detach().cpu().clone().requires_grad_() for p in ps]
    topt = torch.optim.Adam([{"params": cpu[:SPLIT], "lr": LRS[0]}, {"params": cpu[SPLIT:], "lr": LRS[1]}])
    topt.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert all(float(topt.state[q]["step"]) == 3.0 for q in cpu)
    _set_grads(ps, 3)
    for p, q in zip(ps, cpu):
        q.grad = p.grad.cpu().clone()
    before = _snapshot(ps, opt)
    opt.step()
    topt.step()
    worst = [0.0, 0.0, 0.0]
    for i, (p, q) in enumerate(zip(ps, cpu)):
        b = before[i]
        ref = R.adam_step(b[0], b[1], b[2], b[3], step=3, lr=_lr(i))
        assert float(topt.state[q]["step"]) == 4.0 == float(opt.state[p]["step"])
        for key, got_d, got_c, bar in zip("mvp", (opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], p),
                                          (topt.state[q]["exp_avg"], topt.state[q]["exp_avg_sq"], q), R.bars(ref)):
            err = (got_d.detach().cpu().double() - got_c.detach().cpu().double()).abs()
            assert bool((err <= 2 * bar).all()), (i, key, float((err - 2 * bar).max()))  # each side within its own bar of `ref`
        worst = [max(a, x) for a, x in zip(worst, R.ratios(ref, p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]))]
    assert max(worst) <= 1.0, worst


POSITIONS = [(0, 0), (len(SHAPES) - 1, 2 * C + 2), (MISALIGNED, C + 4), (8, C), (7, 1234)]


def _c_grads_finite(gpu, grads):
    from e2e_multi_view_matching_amd import _lib
    ctx = _lib.context(gpu)
    flag = torch.full((1,), 7, dtype=torch.int32, device=gpu)
    n = len(grads)
    ctx.call("e2emv_grads_finite", n, (ctypes.c_void_p * max(n, 1))(*[g.data_ptr() for g in grads]),
             (ctypes.c_int64 * max(n, 1))(*[g.numel() for g in grads]), _lib.ptr(flag), _lib.stream_ptr(gpu))
    return int(flag.item())


def test_the_finite_gradient_check_finds_one_bad_value_at_every_position(gpu):
    import e2e_multi_view_matching_amd as E
    ps = _make_params(gpu)
    _set_grads(ps, 0)
    assert E.has_finite_gradients(ps) is True
    assert _c_grads_finite(gpu, [p.grad for p in ps]) == 0
    assert _c_grads_finite(gpu, []) == 0
    for (i, e) in POSITIONS:
        for value in (float("nan"), float("-inf")):
            flat = ps[i].grad.view(-1)
            good = flat[e].clone()
            flat[e] = value
            assert E.has_finite_gradients(ps) is False, (i, e, value)
            assert _c_grads_finite(gpu, [p.grad for p in ps]) == 1, (i, e, value)
            flat[e] = good
    assert E.has_finite_gradients(ps) is True
    net = torch.nn.Linear(3, 2).to(gpu)  # a module, as the reference passes it; half-precision gradients are widened
    assert E.has_finite_gradients(net) is True
    net.weight.grad = torch.zeros(2, 3, device=gpu)
    net.bias.grad = torch.tensor([1.0, float("inf")], device=gpu)
    assert E.has_finite_gradients(net) is False
    net.bias.grad = None
    assert E.has_finite_gradients(net) is True


def test_more_chunks_than_workgroups(gpu):
    """2049 chunks and a tail: the grid is capped at 2048 workgroups, so one of them walks on to a second chunk."""
    import e2e_multi_view_matching_amd as E
    n = 2049 * C + 5
    gen = torch.Generator().manual_seed(9)
    p = torch.randn(n, generator=gen).to(gpu).requires_grad_()
    opt = E.Adam([p], lr=1e-4, grad_clip=R.CLIP, skip_nonfinite=True)
    p.grad = (torch.randn(n, generator=gen) * 0.05).to(gpu)
    before = (p.detach().clone(), p.grad.clone(), torch.zeros_like(p), torch.zeros_like(p))
    opt.step()
    ref = R.adam_step(*before, step=0, lr=1e-4, clip=R.CLIP)
    r = R.ratios(ref, p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])
    assert max(r) <= 1.0, r
    p.grad[-1] = float("nan")  # ... and the last element of the last chunk is seen by the gate
    keep = p.detach().clone()
    opt.step()
    assert torch.equal(p.detach(), keep) and opt.counters() == (1, 1)


def test_the_next_forward_runs_on_the_stepped_weights(gpu):
    import e2e_multi_view_matching_amd as E
    from e2e_multi_view_matching_amd.synthetic import make_tuples
    torch.manual_seed(5)
    cfg = {"GNN_layers": ["self", "cross"], "sinkhorn_iterations": 20, "conf_mlp": True, "frozen_batchnorm": True}
    model = E.MultiViewMatcher(cfg).to(gpu).train()
    twin = copy.deepcopy(model)
    data = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in make_tuples(batch=1, tuple_size=2, n_kpts=16, seed=3).items()}
    first = model(data)["scores_0_1"]
    (-first[:, :-1, :-1].diagonal(dim1=1, dim2=2).mean()).backward()
    stepped = [p for p in model.parameters() if p.grad is not None]
    assert len(stepped) > 10
    versions = {id(p): p._version for p in stepped}
    old = [p.detach().clone() for p in stepped]
    opt = E.Adam(model.parameters(), lr=1e-2, grad_clip=R.CLIP, skip_nonfinite=True)
    opt.step()
    assert opt.counters() == (1, 0)
    assert all(p._version > versions[id(p)] for p in stepped)
    assert sum(not torch.equal(p.detach(), q) for p, q in zip(stepped, old)) > 10
    with torch.no_grad():
        for q, p in zip(twin.parameters(), model.parameters()):
            q.data.copy_(p.data)
    second = model(data)["scores_0_1"].detach()
    want = twin(data)["scores_0_1"].detach()
    assert torch.equal(second, want)
    assert not torch.equal(second, first.detach())  # (the step was large enough to show in the scores)


def test_the_c_entries_refuse_bad_tables_and_the_context_lives_on(gpu):
    from e2e_multi_view_matching_amd import _lib
    ctx = _lib.context(gpu)
    lib = ctx.lib
    s = _lib.stream_ptr(gpu)
    t = [torch.ones(8, device=gpu), torch.ones(8, device=gpu), torch.zeros(8, device=gpu), torch.zeros(8, device=gpu)]  # p, g, m, v
    step = torch.zeros((), device=gpu)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    one = lambda x: (ctypes.c_void_p * 1)(x.data_ptr())  # noqa: E731
    null = (ctypes.c_void_p * 1)(None)
    numel, lr = (ctypes.c_int64 * 1)(8), (ctypes.c_float * 1)(1e-3)
    tabs = [one(x) for x in t] + [one(step)]

    def adam(n=1, tables=tabs, ne=numel, h=ctx.h):
        return lib.e2emv_adam_step(h, n, *tables, ne, lr, 0.9, 0.999, 1e-8, 0.0, 1, None, s)

    assert adam(h=None) == _lib.EINVAL
    for k in range(5):
        assert adam(tables=tabs[:k] + [None] + tabs[k + 1:]) == _lib.EINVAL  # a NULL table
        assert adam(tables=tabs[:k] + [null] + tabs[k + 1:]) == _lib.EINVAL  # a NULL entry
    assert adam(ne=None) == _lib.EINVAL
    assert adam(n=-1) == _lib.ESHAPE
    assert adam(ne=(ctypes.c_int64 * 1)(-1)) == _lib.ESHAPE
    assert lib.e2emv_grads_finite(None, 1, one(t[1]), numel, _lib.ptr(flag), s) == _lib.EINVAL
    assert lib.e2emv_grads_finite(ctx.h, 1, None, numel, _lib.ptr(flag), s) == _lib.EINVAL
    assert lib.e2emv_grads_finite(ctx.h, 1, null, numel, _lib.ptr(flag), s) == _lib.EINVAL
    assert lib.e2emv_grads_finite(ctx.h, 1, one(t[1]), numel, None, s) == _lib.EINVAL
    assert lib.e2emv_grads_finite(ctx.h, -1, one(t[1]), numel, _lib.ptr(flag), s) == _lib.ESHAPE
    assert lib.e2emv_grads_finite(ctx.h, 1, one(t[1]), (ctypes.c_int64 * 1)(-1), _lib.ptr(flag), s) == _lib.ESHAPE
    torch.cuda.synchronize()
    assert all(bool((x == y).all()) for x, y in zip(t, (1, 1, 0, 0))) and float(step) == 0.0  # nothing was launched
    assert adam() == _lib.OK  # the context is usable: one step with g = 1 moves p by lr (m / sqrt(v) = 1 after the bias corrections)
    torch.cuda.synchronize()
    assert float(step) == 1.0 and abs(float(t[0][0]) - (1.0 - 1e-3)) < 1e-6
    assert abs(float(t[2][0]) - 0.1) < 1e-7 and abs(float(t[3][0]) - 1e-3) < 1e-9
