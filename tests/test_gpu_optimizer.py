"""Momentum SGD on the GPU: rod_sgd_momentum and rod_grad_sqnorm against restatements of their
contract (include/rod.h), and the optimiser through Trainer: graph replay under a changing
learning rate, resume from a checkpoint, and the frozen set."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import config
from rod import ops
from rod.checkpoint import load_variables, save_variables
from rod.data import synthetic_batch
from rod.trainer import Trainer

pytestmark = pytest.mark.gpu

f32 = np.float32
BIG = 4 * 256 * 4096 + 8     # one group past a single pass of the 4096 x 256-thread grid: the stride loop runs
U = 2.0 ** -24               # unit roundoff of fp32 (round to nearest)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def make_flags(n):
    """One byte per 4 elements: a random mix of {frozen, trainable} x {no decay, decay} plus runs
    of zero-flag groups (what alignment padding would carry)."""
    ng = n // 4
    if ng == 1:
        return np.array([3], np.uint8)
    if ng == 2:
        return np.array([3, 0], np.uint8)
    rng = np.random.default_rng(100 + n)
    fl = rng.integers(0, 4, ng).astype(np.uint8)
    fl[rng.integers(0, ng, max(1, ng // 16))] = 0
    fl[ng // 3:ng // 3 + 5] = 0
    fl[0], fl[1], fl[2], fl[-1] = 3, 1, 2, 3           # every combination, and a live last group
    fl.setflags(write=False)
    return fl


@functools.lru_cache(maxsize=None)
def make_data(n, steps=3):
    """(p0, m0, [g per step]): gradients of spread 3, so clip 5 bites on ~10% of them."""
    rng = np.random.default_rng(n)
    p = rng.standard_normal(n).astype(f32)
    m = (0.5 * rng.standard_normal(n)).astype(f32)
    gs = [(3.0 * rng.standard_normal(n)).astype(f32) for _ in range(steps)]
    for a in [p, m] + gs:
        a.setflags(write=False)
    return p, m, gs


def ref_step(p, g, m, flags, lr, scale, mu, wd, clip, nesterov):
    """The contract of rod_sgd_momentum in fp32 numpy: every line one rounded operation."""
    tr = np.repeat(flags & 1, 4).astype(bool)
    dc = np.repeat(flags & 2, 4).astype(bool)
    with np.errstate(invalid='ignore', over='ignore'):
        d = g
        if scale is not None:
            d = d * f32(scale)
        d = np.where(np.isnan(d), d, np.minimum(np.maximum(d, f32(-clip)), f32(clip)))
        d = np.where(dc, d + f32(wd) * p, d)
        mn = d if m is None else f32(mu) * m + d
        u = d + f32(mu) * mn if nesterov else mn
        pn = p - f32(lr) * u
    assert pn.dtype == np.float32 and mn.dtype == np.float32
    return np.where(tr, pn, p), (None if m is None else np.where(tr, mn, m))


def dev_t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def scalar(v, dev):
    return torch.tensor([v], dtype=torch.float32, device=dev)


# ------------------------------------------------------------------ 1. the update kernel, bit-exact
@pytest.mark.parametrize('scale', [None, 0.37])
@pytest.mark.parametrize('clip', [5.0, math.inf])
@pytest.mark.parametrize('nesterov', [False, True])
@pytest.mark.parametrize('n', [4, 8, 1020, BIG])
def test_update_matches_the_formula_bit_exact(dev, n, nesterov, clip, scale):
    p0, m0, gs = make_data(n)
    flags = make_flags(n)
    lr, mu, wd = 1e-2, 0.9, 1e-4
    p, m, fl = dev_t(p0, dev), dev_t(m0, dev), dev_t(flags, dev)
    lr_d = scalar(lr, dev)
    sc_d = None if scale is None else scalar(scale, dev)
    rp, rm = p0, m0
    for k, g in enumerate(gs):
        ops.sgd_momentum_(p, dev_t(g, dev), m, fl, lr_d, sc_d, mu, wd, clip, nesterov)
        rp, rm = ref_step(rp, g, rm, flags, lr, scale, mu, wd, clip, nesterov)
        assert same_bits(p.cpu().numpy(), rp), (k, 'p')
        assert same_bits(m.cpu().numpy(), rm), (k, 'm')
    assert not same_bits(rp, p0)


# ------------------------------------------------------------------ 2. reduction to rod_sgd_clip
@pytest.mark.parametrize('with_buffer', [False, True])
@pytest.mark.parametrize('n', [1020, BIG])
def test_reduces_to_sgd_clip(dev, n, with_buffer):
    p0, _, gs = make_data(n)
    g = dev_t(gs[0], dev)
    pa, pb = dev_t(p0, dev), dev_t(p0, dev)
    ops.sgd_clip_(pa, g, 1e-2, 5.0)
    fl = torch.full((n // 4,), 1, dtype=torch.uint8, device=dev)          # every group trainable
    m = torch.zeros(n, device=dev) if with_buffer else None
    ops.sgd_momentum_(pb, g, m, fl, scalar(1e-2, dev), None, 0.0, 0.0, 5.0, False)
    assert same_bits(pa.cpu().numpy(), pb.cpu().numpy())
    assert not same_bits(pa.cpu().numpy(), p0)


# ------------------------------------------------------------------ 3. frozen groups
def test_frozen_groups_are_untouched(dev):
    n = 1020
    p0, m0, gs = make_data(n)
    flags = make_flags(n)
    frozen = ~np.repeat(flags & 1, 4).astype(bool)
    assert frozen.sum() >= 40 and (~frozen).sum() >= 40
    g = gs[0].copy()
    g[frozen] = 1e30
    g[np.flatnonzero(frozen)[::3]] = np.nan
    p, m, fl, gd = dev_t(p0, dev), dev_t(m0, dev), dev_t(flags, dev), dev_t(g, dev)
    # with norm clipping: the norm must skip the frozen slices too
    sc, ws = scalar(-1.0, dev), ops.grad_sqnorm_workspace(dev)
    ops.grad_sqnorm_(gd, fl, 10.0, sc, ws)
    ops.sgd_momentum_(p, gd, m, fl, scalar(1e-2, dev), sc, 0.9, 1e-4, 5.0, True)
    pn, mn, s = p.cpu().numpy(), m.cpu().numpy(), float(sc.item())
    assert 0.0 < s < 1.0
    assert same_bits(pn[frozen], p0[frozen]) and same_bits(mn[frozen], m0[frozen])
    rp, rm = ref_step(p0, np.where(frozen, f32(0), g), m0, flags, 1e-2, s, 0.9, 1e-4, 5.0, True)
    assert same_bits(pn, rp) and same_bits(mn, rm)
    assert np.isfinite(pn).all() and not same_bits(pn[~frozen], p0[~frozen])


# ------------------------------------------------------------------ 4. NaN
def test_nan_gradient(dev):
    n = 1020
    p0, m0, gs = make_data(n)
    flags = make_flags(n)
    tr = np.repeat(flags & 1, 4).astype(bool)
    bad = int(np.flatnonzero(tr)[17])
    g = gs[0].copy()
    g[bad] = np.nan
    fl, gd = dev_t(flags, dev), dev_t(g, dev)
    # norm clipping off: that element alone, in p and in m
    p, m = dev_t(p0, dev), dev_t(m0, dev)
    ops.sgd_momentum_(p, gd, m, fl, scalar(1e-2, dev), None, 0.9, 1e-4, 5.0, False)
    pn, mn = p.cpu().numpy(), m.cpu().numpy()
    only = np.zeros(n, bool)
    only[bad] = True
    assert np.array_equal(np.isnan(pn), only) and np.array_equal(np.isnan(mn), only)
    rp, rm = ref_step(p0, g, m0, flags, 1e-2, None, 0.9, 1e-4, 5.0, False)
    assert same_bits(pn[~only], rp[~only]) and same_bits(mn[~only], rm[~only])
    # norm clipping on: the scale is NaN and poisons every trainable element (and no frozen one)
    for poison in (np.nan, np.inf, -np.inf):
        g[bad] = poison
        gd = dev_t(g, dev)
        p, m = dev_t(p0, dev), dev_t(m0, dev)
        sc, ws = scalar(1.0, dev), ops.grad_sqnorm_workspace(dev)
        ops.grad_sqnorm_(gd, fl, 10.0, sc, ws)
        assert math.isnan(sc.item()), poison
        ops.sgd_momentum_(p, gd, m, fl, scalar(1e-2, dev), sc, 0.9, 1e-4, 5.0, False)
        pn, mn = p.cpu().numpy(), m.cpu().numpy()
        assert np.array_equal(np.isnan(pn), tr) and np.array_equal(np.isnan(mn), tr), poison
        assert same_bits(pn[~tr], p0[~tr]) and same_bits(mn[~tr], m0[~tr])


# ------------------------------------------------------------------ 5. the norm kernel
@pytest.mark.parametrize('n', [4, 1020, BIG])
def test_grad_sqnorm_scale(dev, n):
    _, _, gs = make_data(n)
    g, flags = gs[0], make_flags(n)
    tr = np.repeat(flags & 1, 4).astype(bool)
    norm = math.sqrt(float((g[tr].astype(np.float64) ** 2).sum()))
    gd, fl, ws = dev_t(g, dev), dev_t(flags, dev), ops.grad_sqnorm_workspace(dev)
    # Summation order implemented (include/rod.h): a thread adds the squares of its groups in a
    # chain of C = ceil(groups / (1024 * 256)) additions per lane, then 2 pairing levels, 8 tree
    # levels, and in stage 2 again 2 pairing and 8 tree levels: D = 20.  Every g^2 passes through
    # 1 (the square) + C + D roundings and all terms are >= 0, so the sum is off by at most
    # (1 + C + D) U relatively (U = 2^-24, second order ~1e-12 ignored against it).  sqrt halves
    # that and adds <= 2 U, the division adds U: the scale is within ((1 + C + D) / 2 + 3) U =
    # (C + D + 7) / 2 U <= (C + D) U as C + D >= 7.  The bound asserted is (C + D) 2^-24.
    C, D = -(-(n // 4) // (1024 * 256)), 20
    assert C == (5 if n == BIG else 1)
    tol = (C + D) * U
    for clip_norm in (norm / 3.0, norm * 0.999, norm * 2.0):
        sc = scalar(-1.0, dev)
        ops.grad_sqnorm_(gd, fl, clip_norm, sc, ws)
        got = sc.cpu().numpy()[0]
        want = min(1.0, clip_norm / max(norm, float(np.finfo(f32).tiny)))
        print('n=%d clip_norm/norm=%.3f rel err %.3e (bound %.3e)' % (n, clip_norm / norm, abs(got - want) / want, tol))
        if clip_norm > norm:
            assert got == f32(1.0)                     # below the threshold: exactly 1
        else:
            assert abs(float(got) - want) <= tol * want, (got, want)
        # deterministic: a second run, same bits (stale workspace, other scale value before)
        sc2 = scalar(7.0, dev)
        ops.grad_sqnorm_(gd, fl, clip_norm, sc2, ws)
        assert same_bits(sc2.cpu().numpy(), sc.cpu().numpy())
    # a zero gradient: norm 0, scale 1
    sc = scalar(-1.0, dev)
    ops.grad_sqnorm_(torch.zeros(n, device=dev), fl, 1.0, sc, ws)
    assert sc.item() == 1.0


# ------------------------------------------------------------------ 6. torch.optim.SGD, fp64
@pytest.mark.parametrize('nesterov', [False, True])
def test_against_torch_sgd_fp64(dev, nesterov):
    n = 1020
    p0, m0, gs = make_data(n)
    g = gs[0]
    # hyperparameters exactly representable in fp32, so both sides use the same numbers
    lr, mu, wd, clip = (float(f32(v)) for v in (1e-2, 0.9, 1e-4, 5.0))
    p, m = dev_t(p0, dev), dev_t(m0, dev)
    fl = torch.full((n // 4,), 3, dtype=torch.uint8, device=dev)
    ops.sgd_momentum_(p, dev_t(g, dev), m, fl, scalar(lr, dev), None, mu, wd, clip, nesterov)

    q = torch.nn.Parameter(torch.from_numpy(p0.astype(np.float64)))
    q.grad = torch.from_numpy(g.astype(np.float64))
    torch.nn.utils.clip_grad_value_([q], clip)
    opt = torch.optim.SGD([q], lr=lr, momentum=mu, nesterov=nesterov, weight_decay=wd)
    opt.state[q]['momentum_buffer'] = torch.from_numpy(m0.astype(np.float64))
    opt.step()
    q64, m64 = q.detach().numpy(), opt.state[q]['momentum_buffer'].numpy()

    # fp32 roundings of the formula, each relative to the magnitude of its own result (U = 2^-24),
    # propagated through the (linear) formula; exact values from the fp64 run:
    #   d = c + wd*p      E_d <= U |wd p| + U |d|                 (c = clip(g) is exact)
    #   m = mu*m0 + d     E_m <= E_d + U |mu m0| + U |m|
    #   u = d + mu*m      E_u <= E_d + mu E_m + U |mu m| + U |u|  (nesterov; else u = m, E_u = E_m)
    #   p = p0 - lr*u     E_p <= lr E_u + U |lr u| + U |p|
    # i.e. the issue's four roundings per result (product, sum, product, sum) plus the ones
    # inherited from d and m.  (1 + 2^-20) covers the second-order terms.
    c = np.clip(g.astype(np.float64), -clip, clip)
    p64_0, m64_0 = p0.astype(np.float64), m0.astype(np.float64)
    d = c + wd * p64_0
    E_d = U * np.abs(wd * p64_0) + U * np.abs(d)
    E_m = E_d + U * np.abs(mu * m64_0) + U * np.abs(m64)
    if nesterov:
        u = d + mu * m64
        E_u = E_d + mu * E_m + U * np.abs(mu * m64) + U * np.abs(u)
    else:
        u, E_u = m64, E_m
    E_p = lr * E_u + U * np.abs(lr * u) + U * np.abs(q64)
    slack = 1.0 + 2.0 ** -20
    err_m = np.abs(m.cpu().numpy().astype(np.float64) - m64)
    err_p = np.abs(p.cpu().numpy().astype(np.float64) - q64)
    print('max err/bound: m %.3f  p %.3f' % ((err_m / E_m).max(), (err_p / E_p).max()))
    assert (err_m <= E_m * slack).all() and (err_p <= E_p * slack).all()
    assert np.abs(q64 - p64_0).max() > 1e-3


# ------------------------------------------------------------------ through Trainer
H, W, B = 160, 288, 2
CFG = dict(momentum=0.9, weight_decay=1e-4, clip_norm=10.0, warmup_steps=3, fix_learning_rate=False)


def new_trainer(dev, **kw):
    return Trainer((H, W), B, dtype=torch.bfloat16, device=dev, seed=2, **{**CFG, **kw})


def snapshot(tr):
    st = tr.net.store
    torch.cuda.synchronize()
    return (st.flat.clone(), tr.opt.mom.clone(), st.flat_buf.clone(), tr.opt.global_step)


@pytest.fixture(scope='module')
def batch(dev):
    return synthetic_batch(B, H, W, dev, seed=21)


@pytest.fixture(scope='module')
def eager_run(dev, batch):
    """Five eager steps of the configured trainer: the state after each, and the rate each applied."""
    tr = new_trainer(dev)
    assert tr.opt.entry == 'rod_sgd_momentum'
    states, rates = [], []
    for _ in range(5):
        tr.step(*batch)
        states.append(snapshot(tr))
        rates.append(tr.opt.hyper[0].item())
    return states, rates


# ------------------------------------------------------------------ 7. graph replay honours the schedule
def test_graph_replay_applies_the_schedule(dev, batch, eager_run):
    states, rates = eager_run
    tg = new_trainer(dev)
    for k in range(5):
        tg.step_graphed(*batch)
        flat, mom, buf, step = snapshot(tg)
        assert torch.equal(flat, states[k][0]), k
        assert torch.equal(mom, states[k][1]), k
        assert torch.equal(buf, states[k][2]) and step == states[k][3] == k + 1
        assert tg.opt.hyper[0].item() == rates[k] == f32(tg.opt.applied_lr(k)), k
    assert tg._graph is not None                       # steps 1..4 were replays of one capture
    assert len(tg._graphs) == 1
    assert len(set(rates)) >= 3, rates                 # the warm-up: lr/3, 2 lr/3, lr
    assert torch.isfinite(states[-1][0]).all() and states[-1][1].abs().max() > 0


# ------------------------------------------------------------------ 8. resume
@pytest.mark.parametrize('fmt', ['torch', 'tf'])
def test_resume_from_checkpoint(dev, batch, eager_run, tmp_path, fmt):
    states, _ = eager_run
    a = new_trainer(dev)
    for _ in range(2):
        a.step(*batch)
    path = os.path.join(str(tmp_path), 'mobilenet_v2.model')
    save_variables(a.net.store, path, a.opt.global_step, fmt, optimizer=a.opt)
    b = new_trainer(dev)
    b.opt.global_step = load_variables(b.net.store, path, optimizer=b.opt)
    assert b.opt.global_step == 2
    for _ in range(2):
        b.step(*batch)
    flat, mom, buf, step = snapshot(b)
    assert step == states[3][3] == 4
    assert torch.equal(flat, states[3][0])
    assert torch.equal(mom, states[3][1])
    assert torch.equal(buf, states[3][2])


# ------------------------------------------------------------------ 9. the frozen set, end to end
def test_frozen_set_end_to_end(dev, batch):
    lr, wd = 1e-3, 1e-2
    # (momentum on, so that the optimiser keeps the buffer m this test reads; from m = 0 the first
    # step's m = 0.9 * 0 + d is d itself)
    tr = Trainer((H, W), B, dtype=torch.bfloat16, device=dev, seed=2, train_range=config.train_range.ALL,
                 fix_refine=True, weight_decay=wd, momentum=0.9, learning_rate=lr)
    st = tr.net.store
    before = {n: p.detach().cpu().numpy().copy() for n, p in st.params.items()}
    tr.step(*batch)
    torch.cuda.synchronize()
    after = {n: p.detach().cpu().numpy() for n, p in st.params.items()}
    grad = {n: p._rod_grad.cpu().numpy() for n, p in st.params.items()}
    mom = tr.opt.state_dict()
    frozen = [n for n in before if 'backbone' in n or 'refine' in n]
    head = [n for n in before if n not in frozen]
    assert frozen and head and all(st.params[n].requires_grad == (n in head) for n in before)
    for n in frozen:
        assert same_bits(after[n], before[n]), n
        assert not mom[n].numpy().any(), n

    def clipped(g):
        return np.minimum(np.maximum(g, f32(-5.0)), f32(5.0))
    # a head weight: decayed; d = clip(g) + wd*p, m = 0.9*0 + d, p = p - lr*m
    ws = [n for n in head if n.endswith('/weights') and not same_bits(after[n], before[n])]
    assert ws
    n = ws[0]
    d = clipped(grad[n]) + f32(wd) * before[n]
    m = f32(0.9) * np.zeros_like(d) + d
    assert same_bits(mom[n].numpy(), m) and same_bits(after[n], before[n] - f32(lr) * m)
    # a BatchNorm beta: no decay term, the change is exactly -lr * m
    betas = [n for n in head if n.endswith('/beta') and not same_bits(after[n], before[n])]
    assert betas
    n = betas[0]
    m = mom[n].numpy()
    assert same_bits(m, f32(0.9) * np.zeros_like(m) + clipped(grad[n]))
    assert same_bits(after[n], before[n] - f32(lr) * m)
