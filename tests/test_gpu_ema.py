"""The weight EMA on the GPU: rod_sgd_momentum_ema against the restatement of its contract
(tests/ema_ref.py, include/rod.h) and against rod_sgd_momentum / rod_sgd_clip, and the average
through Trainer: graph replay under the num_updates warm-up, the frozen set, resume, ema_scope,
the stale padded head weights, and the command lines."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import config
from ema_ref import device_rate, f32, ref_step_ema
from nets.catch_net import CatchNet, factory
from rod import ops
from rod.checkpoint import load_variables, save_variables
from rod.data import synthetic_batch
from rod.trainer import Trainer

pytestmark = pytest.mark.gpu

BIG = 4 * 256 * 4096 + 8     # one group past a single pass of the 4096 x 256-thread grid: the stride loop runs
RATES = [f32(0.9), f32(9.0 / 11.0), f32(1e-4)]
SENTINEL = f32(-1234.5)
bf16 = torch.bfloat16


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
    """(p0, m0, e0, [g per step]): gradients of spread 3, so clip 5 bites on ~10% of them; frozen
    groups carry NaN in every gradient and a sentinel in the shadow."""
    rng = np.random.default_rng(n)
    frozen = ~np.repeat(make_flags(n) & 1, 4).astype(bool)
    p = rng.standard_normal(n).astype(f32)
    m = (0.5 * rng.standard_normal(n)).astype(f32)
    e = (p + 0.3 * rng.standard_normal(n)).astype(f32)
    e[frozen] = SENTINEL
    gs = [(3.0 * rng.standard_normal(n)).astype(f32) for _ in range(steps)]
    for g in gs:
        g[frozen] = np.nan
    for a in [p, m, e] + gs:
        a.setflags(write=False)
    return p, m, e, gs


def dev_t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def scalar(v, dev):
    return torch.tensor([v], dtype=torch.float32, device=dev)


# ------------------------------------------------------------------ 1. the fused kernel, bit-exact
@pytest.mark.parametrize('with_mom', [True, False])
@pytest.mark.parametrize('scale', [None, 0.37])
@pytest.mark.parametrize('nesterov', [False, True])
@pytest.mark.parametrize('n', [4, 8, 1020, BIG])
def test_fused_update_matches_the_formula_bit_exact(dev, n, nesterov, scale, with_mom):
    p0, m0, e0, gs = make_data(n)
    flags = make_flags(n)
    frozen = ~np.repeat(flags & 1, 4).astype(bool)
    lr, wd, clip = 1e-2, 1e-4, 5.0
    mu = 0.9 if with_mom else 0.0       # (no buffer: m = d, and nesterov's u = d + 0 * d)
    p, e, fl = dev_t(p0, dev), dev_t(e0, dev), dev_t(flags, dev)
    m = dev_t(m0, dev) if with_mom else None
    q, qm = dev_t(p0, dev), (dev_t(m0, dev) if with_mom else None)      # rod_sgd_momentum on the same inputs
    lr_d, rate_d = scalar(lr, dev), scalar(0.0, dev)
    sc_d = None if scale is None else scalar(scale, dev)
    rp, rm, re = p0, (m0 if with_mom else None), e0
    for k, g in enumerate(gs):
        rate_d.fill_(float(RATES[k]))                                     # the host's write ahead of the step
        gd = dev_t(g, dev)
        ops.sgd_momentum_ema_(p, gd, m, e, fl, lr_d, sc_d, rate_d, mu, wd, clip, nesterov)
        ops.sgd_momentum_(q, gd, qm, fl, lr_d, sc_d, mu, wd, clip, nesterov)
        rp, rm, re = ref_step_ema(rp, g, rm, re, flags, lr, scale, RATES[k], mu, wd, clip, nesterov)
        pn, en = p.cpu().numpy(), e.cpu().numpy()
        assert same_bits(pn, rp), (k, 'p')
        assert same_bits(en, re), (k, 'e')
        assert same_bits(pn, q.cpu().numpy()), (k, 'p against rod_sgd_momentum')
        if with_mom:
            mn = m.cpu().numpy()
            assert same_bits(mn, rm), (k, 'm')
            assert same_bits(mn, qm.cpu().numpy()), (k, 'm against rod_sgd_momentum')
            assert same_bits(mn[frozen], m0[frozen])
        assert same_bits(pn[frozen], p0[frozen]) and same_bits(en[frozen], e0[frozen]), k
        assert np.isfinite(pn).all() and np.isfinite(en).all()
    assert not same_bits(rp[~frozen], p0[~frozen]) and not same_bits(re[~frozen], e0[~frozen])
    if frozen.any():
        assert (e.cpu().numpy()[frozen] == SENTINEL).all()


# ------------------------------------------------------------------ 2. rate 0
def test_rate_zero_keeps_the_average(dev):
    n = 1020
    p0, m0, e0, gs = make_data(n)
    flags = make_flags(n)
    p, m, e, fl = dev_t(p0, dev), dev_t(m0, dev), dev_t(e0, dev), dev_t(flags, dev)
    ops.sgd_momentum_ema_(p, dev_t(gs[0], dev), m, e, fl, scalar(1e-2, dev), None, scalar(0.0, dev), 0.9, 1e-4, 5.0,
                          False)
    assert same_bits(e.cpu().numpy(), e0)
    tr = np.repeat(flags & 1, 4).astype(bool)
    assert not same_bits(p.cpu().numpy()[tr], p0[tr])


# ------------------------------------------------------------------ 3. reduction to rod_sgd_clip
@pytest.mark.parametrize('n', [1020, BIG])
def test_reduces_to_sgd_clip(dev, n):
    rng = np.random.default_rng(n + 1)
    p0 = rng.standard_normal(n).astype(f32)
    g = dev_t((3.0 * rng.standard_normal(n)).astype(f32), dev)
    pa, pb = dev_t(p0, dev), dev_t(p0, dev)
    ops.sgd_clip_(pa, g, 1e-2, 5.0)
    fl = torch.full((n // 4,), 1, dtype=torch.uint8, device=dev)          # every group trainable
    e = dev_t(p0, dev)
    ops.sgd_momentum_ema_(pb, g, None, e, fl, scalar(1e-2, dev), None, scalar(0.25, dev), 0.0, 0.0, 5.0, False)
    assert same_bits(pa.cpu().numpy(), pb.cpu().numpy())
    assert not same_bits(pa.cpu().numpy(), p0) and not same_bits(e.cpu().numpy(), p0)


# ------------------------------------------------------------------ through Trainer
H, W, B = 160, 288, 2
# (the CFG of tests/test_gpu_optimizer.py)
CFG = dict(momentum=0.9, weight_decay=1e-4, clip_norm=10.0, warmup_steps=3, fix_learning_rate=False)
EMA = dict(ema_decay=0.999, ema_warmup=True)


def new_trainer(dev, **kw):
    return Trainer((H, W), B, dtype=bf16, device=dev, seed=2, **{**CFG, **EMA, **kw})


def snapshot(tr):
    st = tr.net.store
    torch.cuda.synchronize()
    return dict(flat=st.flat.clone(), mom=tr.opt.mom.clone(), ema=None if tr.opt.ema is None else tr.opt.ema.clone(),
                buf=st.flat_buf.clone(), step=tr.opt.global_step)


@pytest.fixture(scope='module')
def batch(dev):
    return synthetic_batch(B, H, W, dev, seed=21)


@pytest.fixture(scope='module')
def eager_run(dev, batch):
    """Five eager steps of the configured trainer: the state after each, and the EMA rate each applied."""
    tr = new_trainer(dev)
    assert tr.opt.entry == 'rod_sgd_momentum_ema'
    states, rates = [], []
    for _ in range(5):
        tr.step(*batch)
        states.append(snapshot(tr))
        rates.append(tr.opt.hyper[2].item())
    return states, rates


def eval_forward(net, cfg, img):
    """Eval-mode forward in bf16 without autograd (the inference path): the outputs, concatenated."""
    with torch.no_grad():
        x = ops.normalize_image(img, bf16)
        out = factory(x, 'mobilenet_v2', False, cfg, bf16, net=net).get_output()
    out = out if isinstance(out[0], torch.Tensor) else [t for grp in out for t in grp]
    torch.cuda.synchronize()
    return torch.cat([t.reshape(-1).float() for t in out])


# ------------------------------------------------------------------ 4. eager against graphed
def test_graph_replay_follows_the_decay_schedule(dev, batch, eager_run):
    states, rates = eager_run
    tg = new_trainer(dev)
    plain = new_trainer(dev, ema_decay=0.0)            # the same training without the average
    assert plain.opt.entry == 'rod_sgd_momentum' and plain.opt.ema is None
    for k in range(5):
        tg.step_graphed(*batch)
        plain.step(*batch)
        s, sp = snapshot(tg), snapshot(plain)
        for key in ('flat', 'mom', 'ema', 'buf'):
            assert torch.equal(s[key], states[k][key]), (k, key)
        assert s['step'] == states[k]['step'] == k + 1
        assert tg.opt.hyper[2].item() == rates[k] == device_rate(0.999, k), k
        assert torch.equal(s['flat'], sp['flat']) and torch.equal(s['mom'], sp['mom']), k   # training is unchanged
    assert tg._graph is not None and len(tg._graphs) == 1     # steps 1..4 were replays of one capture
    assert len(set(rates)) == 5, rates                          # 0.9, 9/11, 0.75, ...: a baked-in rate fails
    assert rates[:3] == [f32(0.9), f32(1.0 - 2.0 / 11.0), f32(0.75)]
    assert torch.isfinite(states[-1]['ema']).all() and not torch.equal(states[-1]['ema'], states[-1]['flat'])


# ------------------------------------------------------------------ 5. the default optimiser plus EMA
def test_default_optimizer_plus_ema(dev, batch):
    a = Trainer((H, W), B, dtype=bf16, device=dev, seed=2)
    b = Trainer((H, W), B, dtype=bf16, device=dev, seed=2, ema_decay=0.99)
    assert a.opt.entry == 'rod_sgd_clip' and b.opt.entry == 'rod_sgd_momentum_ema' and b.opt.mom is None
    e0 = b.opt.ema.clone()
    assert torch.equal(e0, b.net.store.flat)
    for _ in range(3):
        a.step(*batch)
        b.step(*batch)
    torch.cuda.synchronize()
    assert torch.equal(a.net.store.flat, b.net.store.flat)
    assert not torch.equal(a.net.store.flat, e0)
    assert not torch.equal(b.opt.ema, b.net.store.flat) and not torch.equal(b.opt.ema, e0)
    assert torch.isfinite(b.opt.ema).all()


# ------------------------------------------------------------------ 6. the frozen set
def test_frozen_set_keeps_its_average(dev, batch):
    tr = Trainer((H, W), B, dtype=bf16, device=dev, seed=2, train_range=config.train_range.ALL, fix_refine=True,
                 ema_decay=0.99)
    e0 = tr.opt.ema_state_dict()
    for _ in range(2):
        tr.step(*batch)
    torch.cuda.synchronize()
    e1 = tr.opt.ema_state_dict()
    frozen = [n for n in e0 if 'backbone' in n or 'refine' in n]
    head = [n for n in e0 if n not in frozen]
    assert frozen and head
    for n in frozen:
        assert torch.equal(e1[n], e0[n]), n
    moved = [n for n in head if not torch.equal(e1[n], e0[n])]
    assert any(n.startswith('det') for n in moved) and any(n.startswith('clf') for n in moved), moved[:5]
    assert len(moved) >= len(head) // 2


# ------------------------------------------------------------------ 7. resume
@pytest.mark.parametrize('fmt', ['torch', 'tf'])
def test_resume_from_checkpoint(dev, batch, eager_run, tmp_path, fmt):
    states, _ = eager_run
    a = new_trainer(dev)
    for _ in range(2):
        a.step(*batch)
    path = os.path.join(str(tmp_path), 'mobilenet_v2.model')
    save_variables(a.net.store, path, a.opt.global_step, fmt, optimizer=a.opt)
    b = new_trainer(dev)
    b.opt.ema.fill_(7.0)
    b.opt.global_step = load_variables(b.net.store, path, optimizer=b.opt)
    assert b.opt.global_step == 2
    for _ in range(2):
        b.step(*batch)
    s = snapshot(b)
    assert s['step'] == states[3]['step'] == 4
    for key in ('flat', 'mom', 'ema', 'buf'):
        assert torch.equal(s[key], states[3][key]), key


# ------------------------------------------------------------------ 8. ema_scope
def test_ema_scope(dev, batch, eager_run, tmp_path):
    states, _ = eager_run
    tr = new_trainer(dev)
    for _ in range(3):
        tr.step_graphed(*batch)
    before = snapshot(tr)
    st, opt, net = tr.net.store, tr.opt, tr.net
    img = batch[0]
    # eval-mode activations of a network three steps from its random start vanish under the initial
    # moving statistics: calibrate them for the comparison, and put the trained ones back after it
    with torch.no_grad():
        net.calibrate_batchnorm(ops.normalize_image(img, bf16))
    path = os.path.join(str(tmp_path), 'mobilenet_v2.model')
    save_variables(st, path, opt.global_step, optimizer=opt)
    ptrs = (st.flat.data_ptr(), opt.ema.data_ptr())
    outside = eval_forward(net, tr.config_dict, img)
    with opt.ema_scope():
        inside = eval_forward(net, tr.config_dict, img)
        assert torch.equal(st.flat, before['ema']) and torch.equal(opt.ema, before['flat'])
        with pytest.raises(RuntimeError, match='ema_scope'):
            opt.step()
        with pytest.raises(RuntimeError, match='ema_scope'):
            tr.step_graphed(*batch)
    again = eval_forward(net, tr.config_dict, img)
    assert torch.isfinite(inside).all() and not torch.equal(inside, outside)
    print('eval outputs that differ under the average: %d of %d' % (int((inside != outside).sum()), inside.numel()))
    assert torch.equal(again, outside)
    fresh = CatchNet('mobilenet_v2', tr.config_dict, dev, seed=5)
    load_variables(fresh.store, path, use_ema=True)
    assert torch.equal(eval_forward(fresh, tr.config_dict, img), inside)
    raw = CatchNet('mobilenet_v2', tr.config_dict, dev, seed=5)
    load_variables(raw.store, path)
    assert torch.equal(eval_forward(raw, tr.config_dict, img), outside)
    # after the scope: the previous bits, the same pointers, and the same capture replays
    with torch.no_grad():
        st.flat_buf.copy_(before['buf'])
    assert torch.equal(st.flat, before['flat']) and torch.equal(opt.ema, before['ema'])
    assert (st.flat.data_ptr(), opt.ema.data_ptr()) == ptrs and opt.global_step == 3
    g = tr._graph
    for k in (3, 4):
        tr.step_graphed(*batch)
        s = snapshot(tr)
        for key in ('flat', 'mom', 'ema', 'buf'):
            assert torch.equal(s[key], states[k][key]), (k, key)
    assert tr._graph is g and len(tr._graphs) == 1


# ------------------------------------------------------------------ 9. stale padded head weights
def test_eval_after_a_step_reads_the_updated_head_weights(dev, batch, tmp_path):
    """evaluate -> train -> evaluate in one process: the update kernels write the flat buffer
    without bumping the tensors' version counters, so the heads' zero-padded 3x3 weights
    (ops._cinpad_weights; the refine head's 36 -> 36 convs) must follow the store's version."""
    tr = Trainer((H, W), B, dtype=bf16, device=dev, seed=2, learning_rate=0.05)
    st, net, img = tr.net.store, tr.net, batch[0]
    with torch.no_grad():
        net.calibrate_batchnorm(ops.normalize_image(img, bf16))
    first = eval_forward(net, tr.config_dict, img)
    padded = [n for n, p in st.params.items() if getattr(p, '_rod_cinpad', None) is not None]
    assert padded and all(st.params[n].shape[-1] % 8 for n in padded), padded     # the Cin-padded route ran
    w0 = {n: st.params[n].detach().clone() for n in padded}
    tr.step(*batch)
    torch.cuda.synchronize()
    assert all(not torch.equal(st.params[n].detach(), w0[n]) for n in padded)     # the step moved them
    second = eval_forward(net, tr.config_dict, img)
    fresh = CatchNet('mobilenet_v2', tr.config_dict, dev, seed=5)
    path = os.path.join(str(tmp_path), 'mobilenet_v2.model')
    save_variables(st, path, 1)
    load_variables(fresh.store, path)
    want = eval_forward(fresh, tr.config_dict, img)
    assert not torch.equal(second, first)
    assert torch.equal(second, want), int((second != want).sum())


# ------------------------------------------------------------------ 10. the command lines
def test_command_lines(dev, tmp_path):
    import evaluate
    import train
    size = ['--img_height=300', '--img_width=300', '--synthetic=True']

    def run_train(tdir, extra):
        train.main(size + ['--batch_size=1', '--train_range=ALL', '--checkpoint_refine=None', '--max_number_of_steps=3',
                           '--save_every_n_steps=4', '--train_dir=' + tdir, '--summary_dir=' + str(tmp_path / 'summ')]
                   + extra)
        return os.path.join(tdir, 'mobilenet_v2.model')

    def run_eval(cdir, name, extra):
        edir = str(tmp_path / name)
        res = evaluate.main(size + ['--batch_size=2', '--num_images=4', '--select_threshold=0.05',
                                    '--checkpoint_path=' + cdir, '--eval_dir=' + edir] + extra)
        ev = json.load(open(os.path.join(edir, 'eval.json')))
        return res, {k: v for k, v in ev.items() if k not in ('seconds', 'checkpoint')}

    ck = run_train(str(tmp_path / 'ema'), ['--ema_decay=0.99'])
    sd = torch.load(ck, weights_only=True)
    assert set(sd) == {'variables', 'global_step', 'ema'} and sd['global_step'] == 4
    heads = [n for n in sd['ema'] if n.startswith(('det', 'clf'))]
    assert heads and any(not torch.equal(sd['ema'][n], sd['variables'][n]) for n in heads)
    res_ema, ev_ema = run_eval(str(tmp_path / 'ema'), 'eval_ema', ['--use_ema=True'])
    assert all(math.isfinite(v) for v in res_ema)
    # without the flag: what the same variables give from a checkpoint in today's format
    res_raw, ev_raw = run_eval(str(tmp_path / 'ema'), 'eval_raw', [])
    del sd['ema']
    os.makedirs(str(tmp_path / 'stripped'))
    torch.save(sd, str(tmp_path / 'stripped' / 'mobilenet_v2.model'))
    res_old, ev_old = run_eval(str(tmp_path / 'stripped'), 'eval_old', [])
    assert res_raw == res_old and ev_raw == ev_old
    # a checkpoint trained without --ema_decay: the flag is an error that names it
    plain = run_train(str(tmp_path / 'plain'), [])
    assert set(torch.load(plain, weights_only=True)) == {'variables', 'global_step'}
    with pytest.raises(ValueError, match=r'plain.*--use_ema'):
        run_eval(str(tmp_path / 'plain'), 'eval_err', ['--use_ema=True'])
