"""gscream_amd.adam.Adam on the HIP path (gsr_adam_step, gscream_amd/csrc/adam.hip).

Bounds against the fp64 oracle of tests/test_adam.py, evaluated from the fp32 state before each step.  u = 2^-24 (the unit roundoff of
fp32), tau = 2^-149 (its smallest denormal), A = |beta1 m| + |(1 - beta1) g|, D* and ss the oracle's denominator and step size:

    |m' - m*| <= 4u A + 4 tau
    |v' - v*| <= 5u v* + 4 tau
    |p' - p*| <= 2u |p*| + 16u ss A / D* + 4 tau

The constants count the roundings of the kernel's sequence (each at most u relative, or tau / 2 absolute where a result is denormal):
  m' = fl(fl(m b1) + fl(g c1)): b1 rounded from the double and the product rounded, 2u on |beta1 m|; the same for c1 and its product,
       2u on |(1 - beta1) g|; the sum, u on |m'| <= A.  3 first-order terms -> 4u A.
  v' = fl(fl(v b2) + fl(fl(c2 g) g)): b2 and one product, 2u on beta2 v; c2 and two products, 3u on (1 - beta2) g^2; the sum, u on v*
       (every summand is >= 0, so their sum is v*).  At most 3u v* + u v* = 4 first-order terms -> 5u v*.
  p' = fl(p + fl(fl(a m') / d)), d = fl(fl(sqrt(v') / s2) + e): sqrt halves v''s 4u to 2u and rounds (u), s2 is rounded from the double
       (u), the division rounds (u), e is rounded (u on its summand) and the sum rounds (u): at most 6u on D*.  The numerator carries
       m''s 3u A, a rounded from the double (u |m*|) and the product (u |m*|); the quotient rounds (u).  With |m*| <= A that is
       (3 + 1 + 1 + 1 + 6) u = 12 first-order terms on ss A / D* -> 16u ss A / D*.  The final sum rounds once: u |p'| -> 2u |p*|.
The tau terms cover products that land among the denormals ((c2 g) g for |g| < 1e-19).  A denormal v' feeds the square root with
a relative error far above u, which matters only while sqrt(v') / s2 is not small against eps, i.e. for updates below 1e-6 |lr|: the
parameters here are standard normal, as a model's are, so 2u |p*| covers it."""
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.test_adam import adam_oracle  # noqa: E402
from tests.test_anchor_grow import PARAMS, Standin  # noqa: E402

from gscream_amd import adam as _AD  # noqa: E402
from gscream_amd.adam import Adam  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U, TAU = 2.0 ** -24, 2.0 ** -149
VEC, ONE = 4 * _AD.CHUNK_UNITS, _AD.CHUNK_UNITS  # floats per block on the 16-byte path and on the float-by-float path
SIZES = [0, 1, 3, 4, 5, ONE - 1, ONE, ONE + 1, 2 * ONE + 3, VEC - 1, VEC, VEC + 1, 2 * VEC + 3]


@pytest.fixture
def HIP(monkeypatch):
    """torch's step made to raise: these tests must run the kernel."""
    def no_fallback(*a, **k):
        raise AssertionError("took torch's step")
    monkeypatch.setattr(_AD, "_torch_step", no_fallback)
    return _AD


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def on_device(a, offset=0):
    """A contiguous fp32 device tensor with the values of `a`; offset = 1: a view one float into its storage (4-byte aligned only)."""
    a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    if not offset:
        return a.to(DEV)
    store = torch.zeros(a.numel() + offset, dtype=torch.float32, device=DEV)
    view = store[offset:].view(a.shape)
    view.copy_(a)
    assert (view.data_ptr() % 16 == 4 * offset or not a.numel()) and view.is_contiguous()
    return view


def inputs(n, seed):
    """p standard normal; |g| log-uniform in 1e-30 .. 1e15 with a random sign; m of g's magnitude within a decade, of the opposite sign in
    half of the rows; v about g^2 within two decades, zero in a third of the rows; every seventh row g = m = v = 0."""
    r = np.random.default_rng(seed)
    g = 10.0 ** r.uniform(-30, 15, n) * r.choice([-1.0, 1.0], n)
    m = np.abs(g) * 10.0 ** r.uniform(-1, 1, n) * np.where(np.arange(n) % 2 == 0, -np.sign(g), r.choice([-1.0, 1.0], n))
    v = np.minimum(g * g * 10.0 ** r.uniform(-2, 2, n), 1e36)
    v[np.arange(n) % 3 == 1] = 0.0
    dead = np.arange(n) % 7 == 3
    g[dead] = m[dead] = v[dead] = 0.0
    return [a.astype(np.float32) for a in (r.standard_normal(n), g, m, v)]


def next_grad(g, seed):
    r = np.random.default_rng(seed)
    return (g * 2.0 ** r.uniform(-1, 1, g.shape) * r.choice([-1.0, 1.0], g.shape)).astype(np.float32)


def make(specs, cls=Adam, **kw):
    """specs: [(n, seed, group dict, t0, offset)] -> (optimiser with one group per distinct dict, [(param, g0 array)]).  The state is set
    as torch keeps it: `step` on the host, the moments shaped like the parameter."""
    groups, rows = {}, []
    for n, seed, group, t0, offset in specs:
        p, g, m, v = inputs(n, seed)
        param = nn.Parameter(on_device(p, offset))
        groups.setdefault(id(group), dict(group, params=[]))["params"].append(param)
        rows.append((param, g, (t0, on_device(m, offset), on_device(v, offset)), offset))
    opt = cls(list(groups.values()), **kw)
    for param, _g, (t0, m, v), _o in rows:
        opt.state[param] = {"step": torch.tensor(float(t0)), "exp_avg": m, "exp_avg_sq": v}
    return opt, rows


def settings_of(opt, param):
    grp = next(g for g in opt.param_groups if any(q is param for q in g["params"]))
    return grp["lr"], grp["betas"], grp["eps"]


def worst_ratios(before, after, lr, betas, eps, t):
    """max over the elements of |error| / bound for m', v', p' (<= 1 passes), from fp64 copies of the fp32 state."""
    p0, g, m0, v0 = before
    p1, m1, v1 = after
    ps, ms, vs, D, ss = adam_oracle(p0, g, m0, v0, lr, betas, eps, t)
    A = np.abs(betas[0] * m0) + np.abs((1.0 - betas[0]) * g)
    rm = np.abs(m1 - ms) / (4 * U * A + 4 * TAU)
    rv = np.abs(v1 - vs) / (5 * U * vs + 4 * TAU)
    rp = np.abs(p1 - ps) / (2 * U * np.abs(ps) + 16 * U * ss * A / D + 4 * TAU)
    dead = (g == 0) & (m0 == 0) & (v0 == 0)
    assert np.array_equal(p1[dead], p0[dead])  # rows never seen: p compares equal
    if lr == 0:
        assert np.array_equal(p1, p0)
    return [float(r.max()) if r.size else 0.0 for r in (rm, rv, rp)]


def run_steps(opt, rows, steps=3, check=True):
    """`steps` consecutive steps with fresh gradients; the bounds are checked from the fp32 state before each one."""
    worst = [0.0, 0.0, 0.0]
    grads = [g for _p, g, _s, _o in rows]
    for k in range(steps):
        before = []
        for i, (param, _g, _s, offset) in enumerate(rows):
            if k:
                grads[i] = next_grad(grads[i], 1000 * k + i)
            param.grad = on_device(grads[i], offset)
            st = opt.state[param]
            before.append((f64(param), grads[i].astype(np.float64), f64(st["exp_avg"]), f64(st["exp_avg_sq"]), float(st["step"])))
        opt.step()
        if not check:
            continue
        for (param, _g, _s, _o), (p0, g, m0, v0, t0) in zip(rows, before):
            st = opt.state[param]
            assert float(st["step"]) == t0 + 1 and st["step"].device.type == "cpu"
            lr, betas, eps = settings_of(opt, param)
            r = worst_ratios((p0, g, m0, v0), (f64(param), f64(st["exp_avg"]), f64(st["exp_avg_sq"])), lr, betas, eps, t0 + 1)
            worst = [max(a, b) for a, b in zip(worst, r)]
    return worst


G_DEFAULT = {"lr": 0.0075, "betas": (0.9, 0.999), "eps": 1e-15}
G_ZERO_LR = {"lr": 0.0, "betas": (0.9, 0.999), "eps": 1e-15}          # the reference's anchor group
G_OTHER = {"lr": 1.6e-4, "betas": (0.8, 0.99), "eps": 1e-8}


# ---- bounds ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t0", [0, 1, 999, 29999])
def test_three_steps_stay_within_the_rounding_bounds(t0, HIP):
    """Every size at which the kernel takes another path, aligned and one float off, in three groups, from step t0."""
    specs = []
    for i, n in enumerate(SIZES):
        specs.append((n, 10 * i, G_DEFAULT, t0, 0))
        specs.append((n, 10 * i + 1, G_OTHER, t0, 1))
    specs += [(VEC + 2, 500, G_ZERO_LR, t0, 0), (ONE + 2, 501, G_ZERO_LR, t0, 1), (777, 502, G_DEFAULT, t0 + 5, 0)]  # (another step in G_DEFAULT)
    opt, rows = make(specs)
    assert len(opt.param_groups) == 3 and len(rows) == 29
    worst = run_steps(opt, rows)
    print(f"t0={t0}: worst |error| / bound  m' {worst[0]:.3f}  v' {worst[1]:.3f}  p' {worst[2]:.3f}")
    assert opt.last_path == "hip"
    assert max(worst) <= 1.0, worst


def test_nan_and_inf_gradients_give_the_oracles_pattern(HIP):
    n = 3 * 50
    specs = [(n, 1, G_DEFAULT, 3, 0), (n, 2, G_ZERO_LR, 3, 1)]
    opt, rows = make(specs)
    before = []
    for param, g, _s, offset in rows:
        g = g.copy()
        g[0::3], g[1::3], g[2::3] = np.nan, np.inf, -np.inf
        param.grad = on_device(g, offset)
        st = opt.state[param]
        before.append((f64(param), g.astype(np.float64), f64(st["exp_avg"]), f64(st["exp_avg_sq"])))
    opt.step()
    for (param, _g, _s, _o), b in zip(rows, before):
        lr, betas, eps = settings_of(opt, param)
        ps, ms, vs, _D, _ss = adam_oracle(*b, lr, betas, eps, 4)
        st = opt.state[param]
        for got, want, what in ((f64(st["exp_avg"]), ms, "m"), (f64(st["exp_avg_sq"]), vs, "v"), (f64(param), ps, "p")):
            assert np.array_equal(np.isnan(got), np.isnan(want)), what
            assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want)), what
        assert np.isnan(ps).all() and np.isnan(ms[0::3]).all() and np.isposinf(ms[1::3]).all() and np.isneginf(ms[2::3]).all()


def test_the_bits_are_the_fp32_sequence_of_the_header(HIP):
    """Stricter than the bounds: every operation of the rule is a correctly rounded IEEE fp32 operation in the stated order (no
    contraction, no flushing), so numpy's fp32 arithmetic on the host gives the same bits."""
    opt, rows = make([(2 * VEC + 3, 7, G_DEFAULT, 11, 0), (2 * ONE + 3, 8, G_OTHER, 999, 1)])
    want = []
    for param, g, (t0, m, v), offset in rows:
        param.grad = on_device(g, offset)
        lr, betas, eps = settings_of(opt, param)
        b1, c1, b2, c2, s2, e, a = (np.float32(x) for x in _AD.adam_scalars(lr, betas, eps, t0 + 1))
        p0, m0, v0 = (t.detach().cpu().numpy() for t in (param, m, v))
        with np.errstate(all="ignore"):
            m1 = m0 * b1 + g * c1
            v1 = v0 * b2 + (c2 * g) * g
            d = np.sqrt(v1) / s2 + e
            p1 = p0 + (a * m1) / d
        assert m1.dtype == v1.dtype == p1.dtype == np.float32
        want.append((p1, m1, v1))
    opt.step()
    for (param, _g, _s, _o), (p1, m1, v1) in zip(rows, want):
        st = opt.state[param]
        for got, w, what in ((st["exp_avg"], m1, "m"), (st["exp_avg_sq"], v1, "v"), (param, p1, "p")):
            got = got.detach().cpu().numpy()
            off = np.flatnonzero(got.view(np.int32) != w.view(np.int32))
            assert off.size == 0, (what, off.size, off[:4], got[off[:4]], w[off[:4]])


# ---- tables ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [33, 65])
def test_more_tensors_than_one_table_holds(count, HIP, monkeypatch):
    """33 and 65 tensors with gradients: two and three launches."""
    calls = []
    real = _AD._native.run
    opt, rows = make([(5 + i, i, G_DEFAULT if i % 2 else G_OTHER, i, int(i % 3 == 0)) for i in range(count)])
    monkeypatch.setattr(_AD._native, "run", lambda name, *a: (calls.append((name, a[1])), real(name, *a))[1])
    worst = run_steps(opt, rows, steps=1)
    assert calls == [("gsr_adam_step", 32)] * (count // 32) + [("gsr_adam_step", count % 32)]
    assert max(worst) <= 1.0, worst


def test_a_parameter_without_a_gradient_is_left_alone(HIP):
    opt, rows = make([(VEC + 1, 1, G_DEFAULT, 4, 0), (VEC + 1, 2, G_DEFAULT, 4, 0), (VEC + 1, 3, G_DEFAULT, 4, 0)])
    middle = rows[1][0]
    del opt.state[middle]
    kept = bits(middle).clone()
    for i in (0, 2):
        rows[i][0].grad = on_device(rows[i][1])
    old = [bits(rows[i][0]).clone() for i in (0, 2)]
    opt.step()
    assert opt.last_path == "hip" and middle not in opt.state and middle.grad is None and torch.equal(bits(middle), kept)
    for i, o in zip((0, 2), old):
        assert float(opt.state[rows[i][0]]["step"]) == 5.0 and not torch.equal(bits(rows[i][0]), o)
    # state is created lazily, as torch creates it
    middle.grad = on_device(rows[1][1])
    rows[0][0].grad = rows[2][0].grad = None
    opt.step()
    st = opt.state[middle]
    assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 1.0 and st["step"].device.type == "cpu"
    assert st["exp_avg"].shape == middle.shape and st["exp_avg"].device == middle.device and float(opt.state[rows[0][0]]["step"]) == 5.0
    lr, betas, eps = settings_of(opt, middle)
    z = np.zeros(VEC + 1)
    r = worst_ratios((kept.view(torch.float32).cpu().numpy().astype(np.float64), rows[1][1].astype(np.float64), z, z),
                     (f64(middle), f64(st["exp_avg"]), f64(st["exp_avg_sq"])), lr, betas, eps, 1)
    assert max(r) <= 1.0, r


def test_a_non_contiguous_gradient_is_made_contiguous(HIP):
    n = 70
    opt, rows = make([(n * n, 4, G_DEFAULT, 2, 0)])
    param, g = rows[0][0], rows[0][1]
    twin_opt, twin_rows = make([(n * n, 4, G_DEFAULT, 2, 0)])
    wide = torch.zeros(n * n, 2, device=DEV)
    wide[:, 0] = on_device(g)
    param.grad = wide[:, 0]
    assert not param.grad.is_contiguous()
    twin_rows[0][0].grad = on_device(g)
    opt.step()
    twin_opt.step()
    assert opt.last_path == "hip" and torch.equal(bits(param), bits(twin_rows[0][0]))
    assert torch.equal(bits(opt.state[param]["exp_avg_sq"]), bits(twin_opt.state[twin_rows[0][0]]["exp_avg_sq"]))
    assert not param.grad.is_contiguous() and torch.equal(param.grad, wide[:, 0])  # the gradient itself is not replaced


# ---- against torch on the device -----------------------------------------------------------------------------------------------
def test_against_torchs_adam_on_the_device(HIP):
    """The same inputs through torch.optim.Adam(foreach=False): both results lie within the bounds, so they differ by at most twice each."""
    specs = [(n, 3 * i, (G_DEFAULT, G_OTHER, G_ZERO_LR)[i % 3], 7, 0) for i, n in enumerate(SIZES)]
    mine, rows = make(specs)
    ref, ref_rows = make(specs, cls=torch.optim.Adam, foreach=False)
    worst = [0.0, 0.0, 0.0]
    for k in range(3):
        befores = []
        for (param, g, _s, _o), (q, _g, _t, _p) in zip(rows, ref_rows):
            gk = g if k == 0 else next_grad(g, 50 + k)
            param.grad, q.grad = on_device(gk), on_device(gk)
            sp, sq = mine.state[param], ref.state[q]
            with torch.no_grad():  # each step starts from the same fp32 state
                q.copy_(param)
                sq["exp_avg"].copy_(sp["exp_avg"])
                sq["exp_avg_sq"].copy_(sp["exp_avg_sq"])
            befores.append((f64(q), gk.astype(np.float64), f64(sq["exp_avg"]), f64(sq["exp_avg_sq"])))
        mine.step()
        ref.step()
        for (param, _g, _s, _o), (q, _g2, _t, _p), (p0, g, m0, v0) in zip(rows, ref_rows, befores):
            sp, sq = mine.state[param], ref.state[q]
            assert set(sp) == set(sq) and float(sp["step"]) == float(sq["step"]) == 8 + k and sp["step"].dtype == sq["step"].dtype
            lr, betas, eps = settings_of(mine, param)
            ps, ms, vs, D, ss = adam_oracle(p0, g, m0, v0, lr, betas, eps, 8 + k)
            A = np.abs(betas[0] * m0) + np.abs((1.0 - betas[0]) * g)
            r = [np.abs(f64(sp["exp_avg"]) - f64(sq["exp_avg"])) / (2 * (4 * U * A + 4 * TAU)),
                 np.abs(f64(sp["exp_avg_sq"]) - f64(sq["exp_avg_sq"])) / (2 * (5 * U * vs + 4 * TAU)),
                 np.abs(f64(param) - f64(q)) / (2 * (2 * U * np.abs(ps) + 16 * U * ss * A / D + 4 * TAU))]
            worst = [max(a, float(b.max()) if b.size else 0.0) for a, b in zip(worst, r)]
    print(f"worst |hip - torch| / (2 bound)  m' {worst[0]:.3f}  v' {worst[1]:.3f}  p' {worst[2]:.3f}")
    assert mine.state.keys() == {r[0] for r in rows}
    assert max(worst) <= 1.0, worst


def test_the_same_inputs_give_the_same_bits(HIP):
    specs = [(n, 5 * i, (G_DEFAULT, G_OTHER)[i % 2], 3, i % 2) for i, n in enumerate(SIZES)] + [(300_000, 99, G_DEFAULT, 3, 0)]
    out = []
    for _ in range(2):
        opt, rows = make(specs)
        run_steps(opt, rows, steps=2, check=False)
        out.append([(bits(p).clone(), bits(opt.state[p]["exp_avg"]).clone(), bits(opt.state[p]["exp_avg_sq"]).clone()) for p, _g, _s, _o in rows])
    for a, b in zip(*out):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- host stops --------------------------------------------------------------------------------------------------------------
def test_step_does_not_stop_the_host(HIP):
    specs = [(n, i, (G_DEFAULT, G_OTHER, G_ZERO_LR)[i % 3], 2, i % 2) for i, n in enumerate(SIZES)]
    opt, rows = make(specs)
    run_steps(opt, rows, steps=1, check=False)  # library loading and first allocations out of the way
    fresh = nn.Parameter(torch.randn(VEC + 5, device=DEV))  # state still to be created
    opt.add_param_group(dict(G_OTHER, params=[fresh]))
    fresh.grad = torch.randn(VEC + 5, 2, device=DEV)[:, 1]   # and a gradient to be made contiguous
    for param, g, _s, offset in rows:
        param.grad = on_device(g, offset)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert opt.last_path == "hip" and float(opt.state[fresh]["step"]) == 1.0 and float(opt.state[rows[0][0]]["step"]) == 4.0
    assert all(s["step"].device.type == "cpu" for s in opt.state.values())


# ---- fallbacks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["amsgrad", "weight_decay", "float64", "force_torch"])
def test_fallbacks_take_torchs_step_and_equal_torchs_class(case):
    def build(cls):
        g = torch.Generator().manual_seed(5)
        ps = [nn.Parameter(torch.randn(sh, generator=g).to(DEV)) for sh in ((300, 3), (VEC + 1,), (17,))]
        if case == "float64":
            ps[2] = nn.Parameter(ps[2].detach().double())
        groups = [{"params": ps[:1], "lr": 0.01}, {"params": ps[1:], "lr": 0.002}]
        if case == "amsgrad":
            groups[1]["amsgrad"] = True
        if case == "weight_decay":
            groups[0]["weight_decay"] = 0.01
        return cls(groups, eps=1e-15), ps
    mine, a = build(Adam)
    ref, b = build(torch.optim.Adam)
    if case == "force_torch":
        mine.force_torch = True
    for k in range(2):
        g = torch.Generator().manual_seed(k)
        for x, y in zip(a, b):
            x.grad = torch.randn(x.shape, generator=g, dtype=x.dtype).to(DEV)
            y.grad = x.grad.clone()
        mine.step()
        ref.step()
        assert mine.last_path == "torch"
    for x, y in zip(a, b):
        assert torch.equal(x, y) and set(mine.state[x]) == set(ref.state[y])
        for s in mine.state[x]:
            assert torch.equal(mine.state[x][s], ref.state[y][s]), (case, s)
    if case == "force_torch":  # and back
        mine.force_torch = False
        for x in a:
            x.grad = torch.ones_like(x)
        mine.step()
        assert mine.last_path == "hip" and float(mine.state[a[0]]["step"]) == 3.0


# ---- with densification ------------------------------------------------------------------------------------------------------
def standin(N=300, K=10, F=32, seed=0):
    """A stand-in model of N anchors under this optimiser, with statistics that make adjust_anchor grow and prune."""
    g = torch.Generator().manual_seed(seed)
    m = Standin(n_offsets=K, feat_dim=F, voxel_size=0.005, update_depth=3, update_init_factor=16, update_hierachy_factor=4)
    t = dict(anchor=torch.round((torch.rand(N, 3, generator=g) * 2 - 1) * 10.0 / 0.005) * 0.005, offset=torch.randn(N, K, 3, generator=g),
             anchor_feat=torch.randn(N, F, generator=g), opacity=torch.zeros(N, 1), uncertainty=torch.zeros(N, 1),
             scaling=torch.randn(N, 6, generator=g) * 0.5 - 3.5, rotation=torch.randn(N, 4, generator=g))
    groups = []
    for p in PARAMS:
        setattr(m, "_" + p, nn.Parameter(t[p].float().to(DEV)))
        groups.append({"params": [getattr(m, "_" + p)], "lr": 0.0 if p == "anchor" else 0.01, "name": p})
    m.mlp_color = nn.Linear(3, 2).to(DEV)
    groups.insert(3, {"params": list(m.mlp_color.parameters()), "lr": 0.002, "name": "mlp_color"})
    m.optimizer = Adam(groups, lr=0.0, eps=1e-15)
    i = torch.arange(N, device=DEV).view(-1, 1)
    m.anchor_demon = torch.where(i % 3 == 2, torch.zeros_like(i), torch.full_like(i, 100)).float()   # two thirds were seen 100 times
    m.opacity_accum = torch.where(i % 3 == 0, torch.zeros_like(i), torch.full_like(i, 30)).float()   # a third of them never contributed
    m.uncertainty_accum = torch.zeros(N, 1, device=DEV)
    m.offset_denom = torch.full((N * K, 1), 60.0, device=DEV)
    m.offset_gradient_accum = (torch.rand(N * K, 1, generator=g) * 0.06).to(DEV)  # mean gradient norm up to 0.001: above 0.0002 for most
    return m


def backward(m):
    loss = sum(((getattr(m, "_" + p) - 0.3) ** 2).mean() for p in PARAMS) + sum((w ** 2).sum() for w in m.mlp_color.parameters())
    loss.backward()


@pytest.mark.parametrize("how", ["adjust_anchor", "prune_anchor"])
def test_densification_re_keys_this_optimiser_like_torchs(how, HIP):
    from gscream_amd import anchor_adjust as AA
    m = standin()
    opt, N0 = m.optimizer, 300
    backward(m)
    opt.step()
    opt.zero_grad(set_to_none=True)
    assert opt.last_path == "hip" and all(float(opt.state[getattr(m, "_" + p)]["step"]) == 1.0 for p in PARAMS)
    old_feat, old_moment = m._anchor_feat.detach().clone(), opt.state[m._anchor_feat]["exp_avg"].clone()
    torch.manual_seed(0)
    with torch.no_grad():
        if how == "adjust_anchor":
            AA.adjust_anchor(m, check_interval=100, success_threshold=0.8, grad_threshold=0.0002, min_opacity=0.005)
        else:
            AA.prune_anchor(m, (torch.arange(N0, device=DEV) % 3 == 0))
    assert AA.last_path == "hip" and m.optimizer is opt
    N1 = int(m._anchor.shape[0])
    kept = (torch.arange(N0, device=DEV) % 3 != 0)
    assert N1 > int(kept.sum()) if how == "adjust_anchor" else N1 == int(kept.sum())  # real growth; a third pruned
    assert torch.equal(m._anchor_feat[:int(kept.sum())].detach(), old_feat[kept])
    assert torch.equal(opt.state[m._anchor_feat]["exp_avg"][:int(kept.sum())], old_moment[kept])
    for p in PARAMS:
        t = getattr(m, "_" + p)
        st = opt.state[t]
        assert t.shape[0] == N1 and t.grad is None and next(g for g in opt.param_groups if g["name"] == p)["params"][0] is t
        assert st["exp_avg"].shape == t.shape and st["exp_avg_sq"].shape == t.shape and float(st["step"]) == 1.0  # new N, step kept
    # the new parameters have no gradient: a step skips them (and everything else: the MLP's gradients were cleared)
    snapshot = {p: bits(getattr(m, "_" + p)).clone() for p in PARAMS}
    opt.step()
    assert opt.last_path == "hip"
    for p in PARAMS:
        assert torch.equal(bits(getattr(m, "_" + p)), snapshot[p]) and float(opt.state[getattr(m, "_" + p)]["step"]) == 1.0
    backward(m)
    opt.step()
    assert opt.last_path == "hip" and len(opt.state) == len(PARAMS) + 2
    for p in PARAMS:
        t, st = getattr(m, "_" + p), opt.state[getattr(m, "_" + p)]
        assert float(st["step"]) == 2.0 and t.isfinite().all() and st["exp_avg"].isfinite().all() and st["exp_avg_sq"].isfinite().all(), p
        assert p == "anchor" or not torch.equal(bits(t), snapshot[p]), p  # (the anchors' rate is 0, as in the reference)
    assert all(w.isfinite().all() for w in m.mlp_color.parameters())


# ---- under the chain ---------------------------------------------------------------------------------------------------------
def this_adam(groups):
    return Adam(groups, lr=0.0, eps=1e-15)


def test_the_loss_falls_and_the_psnr_rises_under_this_optimiser(HIP):
    """What tests/test_gpu_fit.py asserts for torch's Adam."""
    from gscream_amd import fit as F
    from gscream_amd import set_tuning
    set_tuning()
    s, info = F.scene_fitted(3, 208, 117, iters=200, n_student=20_000, n_teacher=80_000, V=8, return_info=True, optimizer=this_adam)
    print("loss", info["loss"], "psnr", info["psnr_first"], info["psnr_last"], "ms per iteration", info["ms_per_iteration"])
    assert np.isfinite(info["loss"]).all()
    assert info["loss"][-1] < 0.7 * info["loss"][0], info["loss"]
    assert info["psnr_last"] > info["psnr_first"] + 3.0, (info["psnr_first"], info["psnr_last"])


def test_a_second_run_under_this_optimiser_gives_the_same_model(HIP):
    from gscream_amd import fit as F
    a, ia = F.scene_fitted(5, 160, 90, iters=40, n_student=8_000, n_teacher=30_000, V=4, return_info=True, optimizer=this_adam)
    b, ib = F.scene_fitted(5, 160, 90, iters=40, n_student=8_000, n_teacher=30_000, V=4, return_info=True, optimizer=this_adam)
    assert ia["gaussians"] == ib["gaussians"]
    for k in ("means3D", "scales", "opacities", "colors"):
        assert np.array_equal(a[k], b[k]), k
