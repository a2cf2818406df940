"""gscream_amd.adam without a GPU: the fp64 oracle the GPU tests measure against (pinned to torch's rule), the torch path of the class,
the state layout it shares with torch.optim.Adam, the host-side scalars of the kernel, and gsr_adam_step's argument checks."""
import copy
import ctypes
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def adam_oracle(p, g, m, v, lr, betas, eps, t):
    """One Adam step in fp64 (numpy arrays in, t = the step count after its increment):
    -> (p*, m*, v*, D*, ss) with D* the denominator sqrt(v*) / sqrt(1 - beta2^t) + eps and ss the step size lr / (1 - beta1^t)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2 = float(betas[0]), float(betas[1])
    with np.errstate(all="ignore"):
        ms = b1 * m + (1.0 - b1) * g
        vs = b2 * v + (1.0 - b2) * g * g
        D = np.sqrt(vs) / math.sqrt(1.0 - b2 ** t) + eps
        ss = lr / (1.0 - b1 ** t)
        ps = p - ss * ms / D
    return ps, ms, vs, D, ss


def groups_of(tensors, **kw):
    return [{"params": [tensors[0]], "lr": 0.01, "betas": (0.8, 0.99), **kw}, {"params": list(tensors[1:]), "lr": 0.002, **kw}]


def fresh(dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(sh, generator=g, dtype=dtype)) for sh in ((7, 3), (5,), (2, 3, 4))]


def set_grads(params, seed):
    g = torch.Generator().manual_seed(seed)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g, dtype=p.dtype)


def test_the_oracle_is_torchs_rule():
    """adam_oracle against torch.optim.Adam on float64 CPU parameters over 5 steps: 1e-12 relative."""
    p = torch.nn.Parameter(torch.randn(1000, generator=torch.Generator().manual_seed(1), dtype=torch.float64))
    lr, betas, eps = 0.0075, (0.9, 0.999), 1e-15
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps)
    po, m, v = p.detach().numpy().copy(), np.zeros(1000), np.zeros(1000)
    for t in range(1, 6):
        p.grad = torch.randn(1000, generator=torch.Generator().manual_seed(10 + t), dtype=torch.float64) * 10.0 ** (t - 3)
        po, m, v, _D, _ss = adam_oracle(po, p.grad.numpy(), m, v, lr, betas, eps, t)
        opt.step()
        st = opt.state[p]
        for got, want in ((p.detach().numpy(), po), (st["exp_avg"].numpy(), m), (st["exp_avg_sq"].numpy(), v)):
            assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), t
        assert float(st["step"]) == t


def test_cpu_tensors_take_the_torch_path_bit_for_bit():
    from gscream_amd.adam import Adam
    a, b = fresh(), fresh()
    mine, ref = Adam(groups_of(a), eps=1e-15), torch.optim.Adam(groups_of(b), eps=1e-15)
    assert isinstance(mine, torch.optim.Adam) and mine.last_path is None
    for t in range(3):
        set_grads(a, t)
        set_grads(b, t)
        if t == 1:
            a[1].grad = b[1].grad = None  # skipped: its step stays behind
        mine.step()
        ref.step()
        assert mine.last_path == "torch"
        for x, y in zip(a, b):
            assert torch.equal(x, y)
            sx, sy = mine.state[x], ref.state[y]
            assert set(sx) == set(sy) == {"step", "exp_avg", "exp_avg_sq"} and float(sx["step"]) == float(sy["step"])
            assert torch.equal(sx["exp_avg"], sy["exp_avg"]) and torch.equal(sx["exp_avg_sq"], sy["exp_avg_sq"])
    assert float(mine.state[a[1]]["step"]) == 2.0
    assert mine.step(lambda: torch.tensor(3.5)) == 3.5  # the closure's value is returned


def test_state_dicts_interchange_and_from_optimizer_shares_the_state():
    from gscream_amd.adam import Adam
    a, b, c = fresh(), fresh(), fresh()
    mine, ref = Adam(groups_of(a, name="x"), eps=1e-15), torch.optim.Adam(groups_of(b, name="x"), eps=1e-15)
    set_grads(a, 0)
    set_grads(b, 0)
    mine.step()
    ref.step()
    sd_mine, sd_ref = mine.state_dict(), ref.state_dict()
    assert sd_mine["param_groups"] == sd_ref["param_groups"]
    assert sd_mine["state"].keys() == sd_ref["state"].keys()
    for k in sd_ref["state"]:
        for s in ("step", "exp_avg", "exp_avg_sq"):
            x, y = sd_mine["state"][k][s], sd_ref["state"][k][s]
            assert x.dtype == y.dtype and x.device == y.device and torch.equal(x, y), (k, s)
    # torch's class loads this class's dict and goes on as this class does, and the other way round
    other_ref, other_mine = torch.optim.Adam(groups_of(c, name="x"), eps=1e-15), Adam(groups_of(fresh(), name="x"), eps=1e-15)
    other_ref.load_state_dict(copy.deepcopy(sd_mine))  # (a dict loaded as it is shares its host-side `step` tensors)
    other_mine.load_state_dict(copy.deepcopy(sd_ref))
    d = [g["params"] for g in other_mine.param_groups]
    d = d[0] + d[1]
    for ps in (a, b, c, d):
        set_grads(ps, 1)
    for o in (mine, ref, other_ref, other_mine):
        o.step()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for x, y, z in zip(c, d, a):  # (c and d started from the same seed as a and took the moments of step 1)
        assert torch.equal(x, y) and float(other_ref.state[x]["step"]) == float(other_mine.state[y]["step"]) == 2.0
        assert torch.equal(other_ref.state[x]["exp_avg"], mine.state[z]["exp_avg"])
    adopted = Adam.from_optimizer(ref)
    assert type(adopted) is Adam and adopted.param_groups is ref.param_groups and adopted.state is ref.state
    assert adopted.param_groups[0] is ref.param_groups[0] and adopted.state[b[0]] is ref.state[b[0]] and adopted.defaults is ref.defaults
    set_grads(b, 2)
    set_grads(a, 2)
    adopted.step()
    mine.step()
    assert adopted.last_path == "torch" and float(ref.state[b[0]]["step"]) == 3.0
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    with pytest.raises(TypeError):
        Adam.from_optimizer(torch.optim.SGD(fresh(), lr=0.1))


@pytest.mark.parametrize("t", [1, 2, 1000, 30000])
def test_the_scalars_are_the_doubles_rounded_once(t):
    from gscream_amd.adam import adam_scalars
    f = np.float32
    for lr, (b1, b2), eps in ((0.0075, (0.9, 0.999), 1e-15), (0.0, (0.9, 0.999), 1e-15), (1.2345e-4, (0.8, 0.99), 1e-8)):
        want = (f(b1), f(1 - b1), f(b2), f(1 - b2), f(math.sqrt(1 - b2 ** t)), f(eps), f(-(lr / (1 - b1 ** t))))
        got = adam_scalars(lr, (b1, b2), eps, t)
        assert len(got) == 7 and all(isinstance(x, float) for x in got)
        assert [f(x).view(np.int32) for x in got] == [w.view(np.int32) for w in want]     # (bits: lr = 0 gives -0.0)
        assert all(float(f(x)) == x for x in got)                                            # exactly representable in fp32
        assert adam_scalars(lr, (b1, b2), eps, torch.tensor(float(t))) == got                # the state's `step` tensor as it is
    assert float(f(0.9)) != 0.9 and float(f(1 - 0.999)) != float(f(1) - f(0.999))            # rounded once, from the double


def test_header_binding_and_library_have_the_step(native_lib):
    from gscream_amd import _abi, _native
    hdr = _abi.header()
    assert hdr.constants["GSR_ABI_VERSION"] == 9 and _native.ABI_VERSION == 9 and native_lib.gsr_abi_version() == 9
    assert hdr.functions["gsr_adam_step"][0] == "int" and "gsr_adam_step" in _native.EXPORTED_SYMBOLS and hasattr(native_lib, "gsr_adam_step")
    assert hdr.constants["GSR_ADAM_MAX_TENSORS"] == _native.ADAM_MAX_TENSORS == 32
    T = _native.AdamTensor
    assert ctypes.sizeof(T) == 64 and [n for n, _ in T._fields_] == ["p", "g", "m", "v", "n", "b1", "c1", "b2", "c2", "s2", "e", "a"]
    assert T.n.offset == 32 and T.b1.offset == 36 and T.a.offset == 60


def test_argument_checks_without_a_gpu(native_lib):
    """Everything gsr_adam_step rejects, it rejects before launching; what it accepts here launches nothing."""
    from gscream_amd import _native
    step, err = native_lib.gsr_adam_step, native_lib.gsr_last_error
    k = (0.9, 0.1, 0.999, 0.001, 0.03, 1e-15, -0.01)
    table = (_native.AdamTensor * 33)(*[(256, 512, 768, 1024, 4) + k for _ in range(33)])
    assert step(0, None, None) == 0 and step(0, table, None) == 0
    assert step(33, table, None) == -1 and b"n_tensors=33" in err()
    assert step(-1, table, None) == -1 and b"n_tensors=-1" in err()
    assert step(1, None, None) == -1 and b"NULL" in err()
    for field in ("p", "g", "m", "v"):
        bad = (_native.AdamTensor * 2)((256, 512, 768, 1024, 0) + k, (256, 512, 768, 1024, 4) + k)
        setattr(bad[1], field, None)
        assert step(2, bad, None) == -1 and b"tensor 1 has a NULL pointer" in err(), field
    for n in (-1, -2 ** 31, 2 ** 31 - 1):
        bad = (_native.AdamTensor * 1)((256, 512, 768, 1024, n) + k)
        assert step(1, bad, None) == -1 and b"bad size" in err(), n
    bad = (_native.AdamTensor * 1)((256, 514, 768, 1024, 4) + k)
    assert step(1, bad, None) == -1 and b"aligned" in err()
    empty = (_native.AdamTensor * 3)(*[(None, None, None, None, 0) + k for _ in range(3)])
    assert step(3, empty, None) == 0  # zero-length tensors: nothing to launch
