"""Host side of the weight EMA (no GPU): the decay schedule, the option checks, the path
selection, the restatement against fp64, the argument guards of rod_sgd_momentum_ema, its
roofline bytes, the checkpoint round trip of the average and the CLI defaults."""
import math
import os

import numpy as np
import pytest
import torch

from ema_ref import device_rate, ema_decay_at, ema_lines, f32
from rod import _abi, ops
from rod import checkpoint as ck
from rod.params import ParamStore
from utils import net_tools

U = 2.0 ** -24               # unit roundoff of fp32 (round to nearest)


def small_store(seed=0):
    """Sizes 6 and 5 are no multiple of the 4-element group: their last group holds padding."""
    rng = np.random.default_rng(seed)
    st = ParamStore()
    for name, shape in (('backbone/Conv/weights', (2, 1, 1, 3)),
                        ('backbone/Conv/BatchNorm/gamma', (2,)),
                        ('backbone/dw/depthwise/depthwise_weights', (3, 3, 2)),
                        ('refine/deconv/weight_1', (2, 2, 1, 2)),
                        ('head/Conv/weights', (1, 1, 1, 5)),
                        ('head/Conv/biases', (1,))):
        st.add(name, rng.standard_normal(shape).astype(np.float32))
    st.add_buffer('backbone/Conv/BatchNorm/moving_mean', rng.standard_normal(2).astype(np.float32))
    return st.finalize('cpu')


def _record_calls(monkeypatch):
    calls = []
    monkeypatch.setattr(_abi, 'call', lambda name, *a: calls.append((name, a)) or 0)
    monkeypatch.setattr(_abi, 'query', lambda name, *a: 4096)
    monkeypatch.setattr(ops, 'stream', lambda: 0)
    return calls


# ------------------------------------------------------------------ the decay schedule
@pytest.mark.parametrize('warmup', [True, False])
def test_decay_schedule_closed_form(warmup):
    st = small_store()
    decay = 0.999
    opt = net_tools.optimizer(st, 8, 1e-3, ema_decay=decay, ema_warmup=warmup)
    for step in (0, 1, 2, 3, 8, 100, 8989, 8990, 8991, 8992, 10 ** 6):
        want = min(decay, (1 + step) / (10 + step)) if warmup else decay
        assert opt.ema_decay_at(step) == want == ema_decay_at(decay, step, warmup), step
        assert opt.ema_rate(step) == float(f32(1.0 - want)) == float(device_rate(decay, step, warmup)), step
    if warmup:    # 0.1, 2/11, 0.25, ... rising to the cap, which (1 + s) / (10 + s) crosses at s = 8990
        assert [opt.ema_decay_at(s) for s in (0, 1, 2)] == [0.1, 2 / 11, 0.25]
        assert opt.ema_decay_at(8989) < decay and opt.ema_decay_at(8991) == decay
    # default step argument: the next step; the device value was written at construction and
    # follows global_step on refresh()
    assert opt.hyper.shape == (3,) and opt.hyper[2].item() == f32(1.0 - opt.ema_decay_at(0))
    opt.global_step = 5
    assert opt.ema_decay_at() == opt.ema_decay_at(5)
    opt.refresh()
    assert opt.hyper[2].item() == f32(1.0 - opt.ema_decay_at(5))
    assert opt.hyper[0].item() == f32(1e-3) and opt.hyper[1].item() == 1.0       # lr and scale stay put


@pytest.mark.parametrize('bad', [-0.1, 1.0, float('nan')])
def test_bad_ema_decay(bad):
    with pytest.raises(ValueError, match='ema_decay'):
        net_tools.optimizer(small_store(), 8, 1e-3, ema_decay=bad)


# ------------------------------------------------------------------ defaults and selection
@pytest.mark.parametrize('kw,entry', [(dict(), 'rod_sgd_clip'), (dict(momentum=0.9), 'rod_sgd_momentum'),
                                      (dict(weight_decay=1e-4), 'rod_sgd_momentum'),
                                      (dict(clip_norm=10.0), 'rod_sgd_momentum'),
                                      (dict(warmup_steps=3), 'rod_sgd_momentum'),
                                      (dict(fix_learning_rate=False), 'rod_sgd_momentum'),
                                      (dict(momentum=0.9, nesterov=True), 'rod_sgd_momentum')])
def test_ema_off_is_todays_optimizer(monkeypatch, kw, entry):
    st = small_store()
    opt = net_tools.optimizer(st, 8, 2e-3, ema_decay=0.0, **kw)
    assert opt.entry == entry
    assert opt.ema is None and opt.ema_state_dict() == {}
    assert opt.hyper is None if entry == 'rod_sgd_clip' else opt.hyper.shape == (2,)
    calls = _record_calls(monkeypatch)
    opt._ws = torch.zeros(1024)
    opt.step()
    assert [c[0] for c in calls] == (['rod_grad_sqnorm'] if 'clip_norm' in kw else []) + [entry]
    with pytest.raises(RuntimeError, match='ema_decay'):
        with opt.ema_scope():
            pass


@pytest.mark.parametrize('kw', [dict(), dict(momentum=0.9, nesterov=True, weight_decay=1e-4, clip_norm=10.0)])
def test_ema_selects_the_fused_entry(monkeypatch, kw):
    st = small_store()
    opt = net_tools.optimizer(st, 8, 2e-3, ema_decay=0.99, **kw)
    assert opt.entry == 'rod_sgd_momentum_ema'
    assert (opt.mom is not None) == ('momentum' in kw)
    assert opt.ema.data_ptr() != st.flat.data_ptr() and torch.equal(opt.ema, st.flat)   # padding included
    assert opt.flags.numel() * 4 == st.numel
    np.testing.assert_array_equal(opt.flags.numpy(), st.group_flags())
    calls = _record_calls(monkeypatch)
    opt._ws = torch.zeros(1024)
    v = st.version
    opt.step()
    assert [c[0] for c in calls] == (['rod_grad_sqnorm'] if 'clip_norm' in kw else []) + ['rod_sgd_momentum_ema']
    a = calls[-1][1]
    assert a[0] is st.flat and a[1] is st.flat_grad and a[2] is opt.mom and a[3] is opt.ema and a[4] is opt.flags
    assert a[5] == st.numel and a[6].data_ptr() == opt.hyper.data_ptr()
    assert (a[7] is None) == ('clip_norm' not in kw)
    assert a[8].data_ptr() == opt.hyper.data_ptr() + 8 and a[8].numel() == 1
    assert a[9:] == (kw.get('momentum', 0.0), kw.get('weight_decay', 0.0), 5.0, 1 if 'nesterov' in kw else 0, 0)
    assert (opt.global_step, st.version) == (1, v + 1)
    opt.refresh()                                        # the host rewrote the rate for step 1
    assert opt.hyper[2].item() == f32(1.0 - 2 / 11)


def test_ema_scope_swaps_in_place():
    st = small_store()
    opt = net_tools.optimizer(st, 8, 1e-3, ema_decay=0.9)
    with torch.no_grad():
        opt.ema.mul_(0.5)
    raw, avg = st.flat.clone(), opt.ema.clone()
    ptrs, v = (st.flat.data_ptr(), opt.ema.data_ptr()), st.version
    with opt.ema_scope():
        assert torch.equal(st.flat, avg) and torch.equal(opt.ema, raw) and st.version == v + 1
        assert torch.equal(st.params['head/Conv/weights'].reshape(-1), avg[st.offsets['head/Conv/weights'][0]:][:5])
        with pytest.raises(RuntimeError, match='ema_scope'):
            opt.step()
    assert torch.equal(st.flat, raw) and torch.equal(opt.ema, avg) and st.version == v + 2
    assert (st.flat.data_ptr(), opt.ema.data_ptr()) == ptrs and opt.global_step == 0


# ------------------------------------------------------------------ the restatement against fp64
def test_restatement_against_fp64():
    """k = 50 steps of e = e - r (e - p) with a changing p and a changing rate.  Per step, with the
    exact (fp64) values e, p, r of that step and e' = e - r (e - p):
        t1 = fl(e - p)      error <= U |e - p|           (+ the inherited E: the same e enters)
        t2 = fl(r t1)       error <= U |r (e - p)|       (+ r E)
        e' = fl(e - t2)     error <= U |e'|              (+ E - r E)
    so E' <= (1 - r) E + U |e - p| r + U |r (e - p)| + U |e'|  <=  (1 - r) E + U|e - p| + U|r(e - p)|
    + U|e'| (r <= 1), the bound asserted, with (1 + 2^-20) for the second-order terms."""
    n, k = 1024, 50
    rng = np.random.default_rng(7)
    e32 = rng.standard_normal(n).astype(f32)
    e64 = e32.astype(np.float64)
    E = np.zeros(n)
    p = rng.standard_normal(n).astype(f32)
    for step in range(k):
        p = (p + 0.1 * rng.standard_normal(n)).astype(f32)
        r = device_rate(0.999, step)                      # 0.9, 9/11, 0.75, ...: fp32, exact in fp64
        e32 = ema_lines(e32, p, r)
        p64, r64 = p.astype(np.float64), float(r)
        d64 = e64 - p64
        n64 = e64 - r64 * d64
        E = (1.0 - r64) * E + U * np.abs(d64) + U * np.abs(r64 * d64) + U * np.abs(n64)
        e64 = n64
        err = np.abs(e32.astype(np.float64) - e64)
        assert (err <= E * (1.0 + 2.0 ** -20)).all(), (step, (err / E).max())
    print('max err/bound after %d steps: %.3f' % (k, (err / E).max()))
    assert np.abs(e64 - p.astype(np.float64)).max() > 1e-3          # the average lags: a real test


# ------------------------------------------------------------------ the entry's guards
def test_new_entry_guards_its_arguments():
    """Argument validation returns before any HIP call (no GPU here: a launch would fail otherwise)."""
    buf = torch.zeros(16)[:8]        # host memory: only its (64-byte aligned) address is looked at
    assert buf.data_ptr() % 16 == 0
    mis = buf.data_ptr() + 4

    def call(param=buf, grad=buf, mom=buf, ema=buf, flags=buf, n=8, lr=buf, scale=None, rate=buf, mu=0.9, clip=5.0):
        _abi.call('rod_sgd_momentum_ema', param, grad, mom, ema, flags, n, lr, scale, rate, mu, 0.0, clip, 0, None)
    with pytest.raises(RuntimeError, match='rod_sgd_momentum_ema.*multiple of 4'):
        call(n=6)
    with pytest.raises(RuntimeError, match='rod_sgd_momentum_ema: ema and ema_rate'):
        call(ema=None)
    with pytest.raises(RuntimeError, match='rod_sgd_momentum_ema: ema and ema_rate'):
        call(rate=None)
    with pytest.raises(RuntimeError, match='rod_sgd_momentum_ema: lr'):
        call(lr=None)
    with pytest.raises(RuntimeError, match='rod_sgd_momentum_ema.*aligned'):
        call(ema=mis)
    with pytest.raises(RuntimeError, match='rod_sgd_momentum_ema.*momentum buffer'):
        call(mom=None)
    for bad in (-1.0, float('nan')):
        with pytest.raises(RuntimeError, match='rod_sgd_momentum_ema: clip'):
            call(clip=bad)
    call(n=0)                        # nothing to do: no launch, no error
    assert 'rod_sgd_momentum_ema' not in _abi.DEFERRING
    assert 'rod_sgd_momentum_ema' in _abi.exported_symbols()


def test_roofline_counts_the_new_entry():
    from rod import roofline
    n = 1024
    m = object()
    a = (0, 0, m, 0, 0, n, 0, None, 0, .9, 0., 5., 0, 0)
    assert roofline.cost('rod_sgd_momentum_ema', a)[0] == 28 * n + n // 4
    assert roofline.cost('rod_sgd_momentum_ema', a[:2] + (None,) + a[3:])[0] == 20 * n + n // 4
    assert roofline.design_bytes('rod_sgd_momentum_ema', a) >= 28 * n + n // 4


# ------------------------------------------------------------------ checkpoints
@pytest.mark.parametrize('fmt', ['torch', 'tf'])
def test_checkpoint_round_trip_of_the_average(tmp_path, fmt):
    a = small_store()
    oa = net_tools.optimizer(a, 8, 1e-3, momentum=0.9, ema_decay=0.99)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for n, (o, k) in a.offsets.items():
            oa.ema[o:o + k].copy_(torch.randn(k, generator=g))
    path = os.path.join(str(tmp_path), 'model.ckpt')
    ck.save_variables(a, path, 7, fmt, optimizer=oa)
    want = oa.ema_state_dict()
    assert set(want) == set(a.params) and all(want[n].shape == a.params[n].shape for n in want)

    # the average survives, bit for bit, beside the variables and the momentum
    b = small_store(seed=1)
    ob = net_tools.optimizer(b, 8, 1e-3, momentum=0.9, ema_decay=0.99)
    ob.ema.fill_(3.0)
    assert ck.load_variables(b, path, optimizer=ob) == 7
    assert torch.equal(b.flat, a.flat) and torch.equal(b.flat_buf, a.flat_buf)
    for n, (o, k) in b.offsets.items():
        assert torch.equal(ob.ema[o:o + k], want[n].reshape(-1)), n
        assert not ob.ema[o + k:(o + k + 3) // 4 * 4].any()
    if fmt == 'tf':
        raw = ck.read_tf_bundle(path)
        assert raw['backbone/Conv/weights/ExponentialMovingAverage'].shape == (1, 1, 3, 2)
        assert raw['backbone/dw/depthwise/depthwise_weights/ExponentialMovingAverage'].shape == (3, 3, 2, 1)
        np.testing.assert_array_equal(raw['backbone/Conv/weights/ExponentialMovingAverage'],
                                      want['backbone/Conv/weights'].numpy().transpose(1, 2, 3, 0))
    else:
        assert set(torch.load(path, weights_only=True)) == {'variables', 'global_step', 'optimizer', 'ema'}

    # use_ema: the variables take the averages, the buffers load as they are; no optimiser needed
    c = small_store(seed=2)
    assert ck.load_variables(c, path, use_ema=True) == 7
    for n, (o, k) in c.offsets.items():
        assert torch.equal(c.flat[o:o + k], want[n].reshape(-1)), n
    assert torch.equal(c.flat_buf, a.flat_buf) and not torch.equal(c.flat, a.flat)
    # ... and without the flag the same checkpoint loads as it always did
    c2 = small_store(seed=2)
    ck.load_variables(c2, path)
    assert torch.equal(c2.flat, a.flat)

    # names_regex restricts both the use_ema load and the restored average
    d = small_store(seed=3)
    d0 = d.flat.clone()
    ck.load_variables(d, path, names_regex=r'backbone.+', use_ema=True)
    e = small_store(seed=3)
    oe = net_tools.optimizer(e, 8, 1e-3, ema_decay=0.5)
    oe.ema.fill_(3.0)
    ck.load_variables(e, path, names_regex=r'backbone.+', optimizer=oe)
    for n, (o, k) in d.offsets.items():
        inside = n.startswith('backbone')
        assert torch.equal(d.flat[o:o + k], want[n].reshape(-1) if inside else d0[o:o + k]), n
        assert torch.equal(oe.ema[o:o + k], want[n].reshape(-1) if inside else torch.full((k,), 3.0)), n
        assert torch.equal(e.flat[o:o + k], a.flat[o:o + k] if inside else d0[o:o + k]), n

    # a checkpoint written with EMA off holds no average: nothing added to either format ...
    path2 = os.path.join(str(tmp_path), 'plain.ckpt')
    off = net_tools.optimizer(a, 8, 1e-3, momentum=0.9)
    ck.save_variables(a, path2, 9, fmt, optimizer=off)
    if fmt == 'tf':
        assert not any(k.endswith('/ExponentialMovingAverage') for k in ck.read_tf_bundle(path2))
    else:
        assert set(torch.load(path2, weights_only=True)) == {'variables', 'global_step', 'optimizer'}
    # ... use_ema on it raises, naming the checkpoint and the flag ...
    with pytest.raises(ValueError, match=r'plain\.ckpt.*--use_ema'):
        ck.load_variables(small_store(), path2, use_ema=True)
    # ... and an EMA optimiser starts every average from the restored value
    ob.ema.fill_(3.0)
    assert ck.load_variables(b, path2, optimizer=ob) == 9
    assert torch.equal(ob.ema, b.flat) and torch.equal(b.flat, a.flat)


def test_variable_missing_from_the_stored_average(tmp_path):
    a = small_store()
    oa = net_tools.optimizer(a, 8, 1e-3, ema_decay=0.99)
    with torch.no_grad():
        oa.ema.mul_(0.25)
    path = os.path.join(str(tmp_path), 'model.ckpt')
    ck.save_variables(a, path, 3, optimizer=oa)
    sd = torch.load(path, weights_only=True)
    del sd['ema']['head/Conv/weights']
    torch.save(sd, path)
    b = small_store(seed=1)
    ob = net_tools.optimizer(b, 8, 1e-3, ema_decay=0.99)
    ck.load_variables(b, path, optimizer=ob)
    for n, (o, k) in b.offsets.items():
        src = a.flat if n == 'head/Conv/weights' else oa.ema
        assert torch.equal(ob.ema[o:o + k], src[o:o + k]), n
    # use_ema: that variable keeps its own (restored) value
    c = small_store(seed=2)
    ck.load_variables(c, path, use_ema=True)
    o, k = c.offsets['head/Conv/weights']
    assert torch.equal(c.flat[o:o + k], a.flat[o:o + k])
    o, k = c.offsets['head/Conv/biases']
    assert torch.equal(c.flat[o:o + k], oa.ema[o:o + k])


# ------------------------------------------------------------------ command lines
def test_parser_defaults():
    import evaluate
    import predict
    import train
    F = train.parse([])
    assert (F.ema_decay, F.ema_warmup) == (0.0, True)
    F = train.parse(['--ema_decay=0.999', '--ema_warmup=False'])
    assert (F.ema_decay, F.ema_warmup) == (0.999, False)
    for bad in ('1.0', '-0.5', 'nan'):
        with pytest.raises(SystemExit):
            train.parse(['--ema_decay=' + bad])
    assert evaluate.parse([]).use_ema is False and evaluate.parse(['--use_ema', 'True']).use_ema is True
    assert predict.parse([]).use_ema is False and predict.parse(['--use_ema=True']).use_ema is True
    # neutral flags build the default optimiser
    D0 = train.parse([])
    opt = net_tools.optimizer(small_store(), 8, D0.learning_rate, ema_decay=D0.ema_decay, ema_warmup=D0.ema_warmup)
    assert opt.entry == 'rod_sgd_clip' and opt.ema is None
    assert math.isclose(net_tools.optimizer(small_store(), 8, 1e-3, ema_decay=0.5).ema_rate(100), 0.5)
