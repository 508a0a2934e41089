"""Host side of the momentum-SGD optimiser (no GPU): the learning-rate schedule, the group
flags, the path selection, the CLI defaults and the checkpoint round trip of the momentum."""
import os

import numpy as np
import pytest
import torch

from rod import _abi, ops
from rod import checkpoint as ck
from rod.params import FLAG_DECAY, FLAG_TRAINABLE, ParamStore, default_decay
from utils import net_tools

T, D = FLAG_TRAINABLE, FLAG_DECAY


def small_store():
    """Sizes 6 and 5 are no multiple of the 4-element group: their last group holds padding."""
    rng = np.random.default_rng(0)
    st = ParamStore()
    for name, shape in (('backbone/Conv/weights', (2, 1, 1, 3)),            # 6  -> groups 0-1
                        ('backbone/Conv/BatchNorm/gamma', (2,)),            # 2  -> group  2
                        ('backbone/Conv/BatchNorm/beta', (2,)),             # 2  -> group  3
                        ('backbone/dw/depthwise/depthwise_weights', (3, 3, 2)),   # 18 -> groups 4-8
                        ('refine/deconv/weight_1', (2, 2, 1, 2)),           # 8  -> groups 9-10
                        ('head/Conv/weights', (1, 1, 1, 5)),                # 5  -> groups 11-12
                        ('head/Conv/biases', (1,)),                         # 1  -> group  13
                        ('head/se/bottleneck_fc/kernel', (4, 1)),           # 4  -> group  14
                        ('head/se/bottleneck_fc/bias', (1,))):              # 1  -> group  15
        st.add(name, rng.standard_normal(shape).astype(np.float32))
    st.add_buffer('backbone/Conv/BatchNorm/moving_mean', np.arange(2, dtype=np.float32))
    return st.finalize('cpu')


def test_applied_rate_closed_form():
    st = small_store()
    lr, batch, warm = 1e-2, 8, 5
    opt = net_tools.optimizer(st, batch, lr, fix_learning_rate=False, warmup_steps=warm)
    period = 20000 // batch                       # 2500 steps per staircase level
    for step in (0, 1, 3, 4, 5, 6, period - 1, period, period + 1, 2 * period - 1, 2 * period, 2 * period + 7):
        want = lr * 0.97 ** (step // period) * min(1.0, (step + 1) / warm)
        assert opt.applied_lr(step) == pytest.approx(want, rel=1e-15), step
    # over the warm-up boundary: strictly rising, then flat
    r = [opt.applied_lr(s) for s in range(7)]
    assert r[0] == pytest.approx(lr / 5) and all(a < b for a, b in zip(r[:4], r[1:5])) and r[4] == r[5] == r[6] == lr
    # the two staircase boundaries
    assert opt.applied_lr(period - 1) == lr and opt.applied_lr(period) == pytest.approx(lr * 0.97)
    assert opt.applied_lr(2 * period - 1) == pytest.approx(lr * 0.97)
    assert opt.applied_lr(2 * period) == pytest.approx(lr * 0.97 ** 2)
    # default step argument: the next step
    opt.global_step = period
    assert opt.applied_lr() == opt.applied_lr(period)
    # a fixed rate with warm-up only; and the plain fixed rate
    fixed = net_tools.optimizer(st, batch, lr, warmup_steps=2)
    assert [fixed.applied_lr(s) for s in (0, 1, 2, 10 * period)] == [lr / 2, lr, lr, lr]
    assert net_tools.optimizer(st, batch, lr).applied_lr(10 * period) == lr


def test_decayed_lr_unchanged():
    st = small_store()
    opt = net_tools.optimizer(st, 20, 1e-3)
    for step in (0, 999, 1000, 1001, 2500, 123456):
        assert opt.decayed_lr(step) == 1e-3 * 0.97 ** (step // (20000 / 20))
    opt.global_step = 2000
    assert opt.decayed_lr() == 1e-3 * 0.97 ** 2.0
    assert opt.summary_lr(2000) == opt.decayed_lr(2000)      # the default run's summary record, as before
    new = net_tools.optimizer(st, 20, 1e-3, momentum=0.9)
    assert new.decayed_lr(2000) == opt.decayed_lr(2000)
    assert new.summary_lr(2000) == new.applied_lr(2000) == 1e-3   # the rate actually applied


def test_default_decay_names():
    yes = ['backbone/MobilenetV2/Conv/weights', 'head/se/recover_fc/kernel', 'refine/deconv/weight_0',
           'refine/deconv/weight_12']
    no = ['backbone/MobilenetV2/expanded_conv_3/depthwise/depthwise_weights', 'a/BatchNorm/gamma',
          'a/BatchNorm/beta', 'a/Conv/biases', 'head/se/recover_fc/bias', 'weights', 'a/weight_', 'a/weights_1']
    assert all(default_decay(n) for n in yes) and not any(default_decay(n) for n in no)


def test_group_flags():
    st = small_store()
    assert st.numel == 64 and st.numel % 4 == 0
    want = np.array([T | D] * 2 + [T, T] + [T] * 5 + [T | D] * 2 + [T | D] * 2 + [T] + [T | D] + [T], np.uint8)
    got = st.group_flags()
    assert got.dtype == np.uint8 and got.shape == (st.numel // 4,)
    np.testing.assert_array_equal(got, want)
    # every group belongs to exactly one parameter (no group of padding alone), and the padding
    # elements inside a parameter's last group are zero in the parameter buffer
    cover = np.zeros(st.numel // 4, int)
    for name, (o, n) in st.offsets.items():
        assert o % 4 == 0
        cover[o // 4:(o + n + 3) // 4] += 1
        assert not st.flat[o + n:(o + n + 3) // 4 * 4].any()
    assert (cover == 1).all()
    # a custom predicate
    np.testing.assert_array_equal(st.group_flags(lambda n: n.endswith('beta')) & D,
                                  np.array([0] * 3 + [D] + [0] * 12, np.uint8))
    # frozen variables lose bit 0 (and keep bit 1); set_trainable is seen by the optimiser
    opt = net_tools.optimizer(st, 8, 1e-3, weight_decay=1e-4)
    np.testing.assert_array_equal(opt.flags.numpy(), want)
    st.set_trainable(lambda n: not n.startswith(('backbone', 'refine')))
    frozen = want.copy()
    frozen[:11] &= D
    np.testing.assert_array_equal(st.group_flags(), frozen)
    assert not (st.group_flags()[:11] & T).any() and (st.group_flags()[11:] & T).all()
    opt.refresh()
    np.testing.assert_array_equal(opt.flags.numpy(), frozen)


def test_train_parse_defaults():
    import train
    F = train.parse([])
    # today's defaults
    assert (F.learning_rate, F.batch_size, F.fix_refine, F.train_range, F.hip_graph, F.save_format) == \
        (1e-3, 20, True, 'REFINE', True, 'torch')
    # the new flags at their neutral values
    assert (F.momentum, F.nesterov, F.weight_decay, F.clip_norm, F.warmup_steps, F.fix_learning_rate) == \
        (0.0, False, 0.0, None, 0, True)
    F = train.parse(['--momentum=0.9', '--nesterov=True', '--weight_decay=1e-4', '--clip_norm=10',
                     '--warmup_steps=500', '--fix_learning_rate=False'])
    assert (F.momentum, F.nesterov, F.weight_decay, F.clip_norm, F.warmup_steps, F.fix_learning_rate) == \
        (0.9, True, 1e-4, 10.0, 500, False)
    # neutral flags build the default optimiser
    st = small_store()
    D0 = train.parse([])
    opt = net_tools.optimizer(st, 8, D0.learning_rate, fix_learning_rate=D0.fix_learning_rate, momentum=D0.momentum,
                              nesterov=D0.nesterov, weight_decay=D0.weight_decay, clip_norm=D0.clip_norm,
                              warmup_steps=D0.warmup_steps)
    assert opt.entry == 'rod_sgd_clip'


def _record_calls(monkeypatch):
    calls = []
    monkeypatch.setattr(_abi, 'call', lambda name, *a: calls.append((name, a)) or 0)
    monkeypatch.setattr(_abi, 'query', lambda name, *a: 4096)
    monkeypatch.setattr(ops, 'stream', lambda: 0)
    return calls


def test_default_optimizer_is_todays_path(monkeypatch):
    st = small_store()
    opt = net_tools.optimizer(st, 8, 2e-3)
    assert opt.entry == 'rod_sgd_clip'
    assert opt.mom is None and opt.flags is None and opt.hyper is None and opt.state_dict() == {}
    calls = _record_calls(monkeypatch)
    v = st.version
    opt.step()
    assert [c[0] for c in calls] == ['rod_sgd_clip']
    name, a = calls[0]
    assert a[0] is st.flat and a[1] is st.flat_grad and a[2:] == (st.numel, 2e-3, 5.0, 0)
    assert (opt.global_step, st.version) == (1, v + 1)


@pytest.mark.parametrize('kw', [dict(momentum=0.9), dict(weight_decay=1e-4), dict(clip_norm=10.0),
                                dict(warmup_steps=3), dict(fix_learning_rate=False),
                                dict(momentum=0.9, nesterov=True)])
def test_any_option_selects_the_momentum_entry(monkeypatch, kw):
    st = small_store()
    opt = net_tools.optimizer(st, 8, 2e-3, **kw)
    assert opt.entry == 'rod_sgd_momentum'
    assert (opt.mom is not None) == ('momentum' in kw)
    if opt.mom is not None:
        assert opt.mom.shape == st.flat.shape and not opt.mom.any()
    assert opt.flags.numel() * 4 == st.numel and opt.hyper.dtype == torch.float32
    assert opt.hyper[0].item() == np.float32(opt.applied_lr(0))     # written at construction
    calls = _record_calls(monkeypatch)
    opt._ws = torch.zeros(1024)
    opt.step()
    names = [c[0] for c in calls]
    assert names == (['rod_grad_sqnorm'] if 'clip_norm' in kw else []) + ['rod_sgd_momentum']
    a = calls[-1][1]
    assert a[2] is opt.mom and a[4] == st.numel and a[5].data_ptr() == opt.hyper.data_ptr()
    assert (a[6] is None) == ('clip_norm' not in kw)
    if 'warmup_steps' in kw:                                        # the host rewrote the rate for step 1
        opt.refresh()
        assert opt.hyper[0].item() == np.float32(2e-3 * 2 / 3)


def test_bad_options():
    st = small_store()
    for kw in (dict(nesterov=True), dict(momentum=-0.1), dict(clip_norm=0.0), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            net_tools.optimizer(st, 8, 1e-3, **kw)


def test_new_entries_guard_their_arguments():
    """Argument validation returns before any HIP call."""
    buf = torch.zeros(16)[:8]        # host memory: only its (64-byte aligned) address is looked at
    assert buf.data_ptr() % 16 == 0
    with pytest.raises(RuntimeError, match='multiple of 4'):
        _abi.call('rod_sgd_momentum', buf, buf, buf, buf, 6, buf, None, 0.9, 0.0, 5.0, 0, None)
    with pytest.raises(RuntimeError, match='momentum buffer'):
        _abi.call('rod_sgd_momentum', buf, buf, None, buf, 8, buf, None, 0.9, 0.0, 5.0, 0, None)
    with pytest.raises(RuntimeError, match='lr'):
        _abi.call('rod_sgd_momentum', buf, buf, buf, buf, 8, None, None, 0.9, 0.0, 5.0, 0, None)
    with pytest.raises(RuntimeError, match='aligned'):
        _abi.call('rod_sgd_momentum', 4, 16, 16, buf, 8, buf, None, 0.9, 0.0, 5.0, 0, None)
    with pytest.raises(RuntimeError, match='multiple of 4'):
        _abi.call('rod_grad_sqnorm', buf, buf, -4, 1.0, buf, buf, None)
    with pytest.raises(RuntimeError, match='clip_norm'):
        _abi.call('rod_grad_sqnorm', buf, buf, 8, float('nan'), buf, buf, None)
    with pytest.raises(RuntimeError, match='workspace'):
        _abi.call('rod_grad_sqnorm', buf, buf, 8, 1.0, buf, None, None)
    assert _abi.query('rod_grad_sqnorm_workspace') == 4096
    assert 'rod_sgd_momentum' not in _abi.DEFERRING and 'rod_grad_sqnorm' not in _abi.DEFERRING


def test_roofline_counts_the_new_entries():
    from rod import roofline
    n = 1024
    m = object()
    assert roofline.cost('rod_sgd_momentum', (0, 0, m, 0, n, 0, None, .9, 0., 5., 0, 0))[0] == 20 * n + n // 4
    assert roofline.cost('rod_sgd_momentum', (0, 0, None, 0, n, 0, None, 0., 0., 5., 0, 0))[0] == 12 * n + n // 4
    assert roofline.cost('rod_grad_sqnorm', (0, 0, n, 1.0, 0, 0, 0))[0] == 4 * n + n // 4


@pytest.mark.parametrize('fmt', ['torch', 'tf'])
def test_checkpoint_round_trip_of_the_momentum(tmp_path, fmt):
    a = small_store()
    oa = net_tools.optimizer(a, 8, 1e-3, momentum=0.9)
    g = torch.Generator().manual_seed(1)
    oa.mom.copy_(torch.randn(a.numel, generator=g))
    path = os.path.join(str(tmp_path), 'model.ckpt')
    ck.save_variables(a, path, 7, fmt, optimizer=oa)
    want = oa.state_dict()
    assert set(want) == set(a.params)

    b = small_store()
    with torch.no_grad():
        b.flat.zero_()
    ob = net_tools.optimizer(b, 8, 1e-3, momentum=0.9)
    ob.mom.fill_(3.0)
    assert ck.load_variables(b, path, optimizer=ob) == 7
    assert torch.equal(b.flat, a.flat) and torch.equal(b.flat_buf, a.flat_buf)
    for n, (o, k) in b.offsets.items():
        assert torch.equal(ob.mom[o:o + k], want[n].reshape(-1)), n        # bit-identical, layout restored
        assert not ob.mom[o + k:(o + k + 3) // 4 * 4].any()
    if fmt == 'tf':
        raw = ck.read_tf_bundle(path)
        # the slot goes through the variable's own layout transform ([Cout,kh,kw,Cin] -> HWIO)
        assert raw['backbone/Conv/weights/Momentum'].shape == (1, 1, 3, 2)
        assert raw['backbone/dw/depthwise/depthwise_weights/Momentum'].shape == (3, 3, 2, 1)
        np.testing.assert_array_equal(raw['backbone/Conv/weights/Momentum'],
                                      want['backbone/Conv/weights'].numpy().transpose(1, 2, 3, 0))
    else:
        assert set(torch.load(path, weights_only=True)) == {'variables', 'global_step', 'optimizer'}

    # a partial restore touches only the matching variables' momentum
    c = small_store()
    oc = net_tools.optimizer(c, 8, 1e-3, momentum=0.9)
    oc.mom.fill_(3.0)
    ck.load_variables(c, path, names_regex=r'backbone.+', optimizer=oc)
    for n, (o, k) in c.offsets.items():
        assert torch.equal(oc.mom[o:o + k], want[n].reshape(-1) if n.startswith('backbone') else torch.full((k,), 3.0))

    # a checkpoint with state loads into a default-optimiser run (state ignored) ...
    d = small_store()
    od = net_tools.optimizer(d, 8, 1e-3)
    assert ck.load_variables(d, path, optimizer=od) == 7 and od.state_dict() == {}
    assert ck.load_variables(small_store(), path) == 7                     # ... and through today's call

    # a state-less checkpoint (a default run's, or today's call) loads with momentum zero
    path2 = os.path.join(str(tmp_path), 'plain.ckpt')
    ck.save_variables(a, path2, 9, fmt)
    if fmt == 'torch':
        assert set(torch.load(path2, weights_only=True)) == {'variables', 'global_step'}
    path3 = os.path.join(str(tmp_path), 'default.ckpt')
    ck.save_variables(a, path3, 9, fmt, optimizer=od)
    for p in (path2, path3):
        ob.mom.fill_(3.0)
        assert ck.load_variables(b, p, optimizer=ob) == 9
        assert not ob.mom.any()
