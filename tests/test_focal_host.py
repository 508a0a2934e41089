"""Focal loss, the parts that need no GPU: the numpy restatement (tests/focal_ref.py) against
torch.autograd in float64 and against plain cross-entropy, the CLI flags, the host layers' mode
check and the argument checks of rod_softmax_focal / rod_focal_loss (they return before any HIP
call, as in tests/test_abi.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import focal_ref as fr  # noqa: E402


def _autograd(c, alpha, gamma):
    """(clf_loss, d clf_loss / d logits) of the textbook form in float64: -a (1 - p_t)^gamma log p_t."""
    K = c['K']
    x = torch.from_numpy(c['logits'].astype(np.float64)).reshape(-1, K).requires_grad_(True)
    pos = torch.from_numpy(c['pos'].reshape(-1) != 0)
    t = torch.from_numpy(np.where(c['pos'] != 0, c['lbl'], 0).reshape(-1).astype(np.int64))
    lp = torch.log_softmax(x, 1).gather(1, t[:, None])[:, 0]
    a = torch.where(pos, torch.tensor(alpha, dtype=torch.float64), torch.tensor(1 - alpha, dtype=torch.float64))
    w = (1 - lp.exp()).clamp_min(0) ** gamma
    loss = (-a * w * lp).sum() / max(int(pos.sum()), 1)
    (g,) = torch.autograd.grad(loss, x)
    return loss.item(), g.numpy().reshape(c['logits'].shape)


@pytest.mark.parametrize('gamma', [0.0, 0.5, 2.0, 5.0])
@pytest.mark.parametrize('name', ['base', 'K2', 'sat', 'satwrong', 'nopos', 'allpos'])
def test_closed_form_gradient_is_autograd(name, gamma):
    c = fr.case(name)
    ref = fr.focal(c['logits'], c['lbl'], c['pos'], 0.25, gamma)
    loss, g = _autograd(c, 0.25, gamma)
    np.testing.assert_allclose(ref['clf_loss'], loss, rtol=1e-12)
    rows = np.ones(c['B'] * c['A'], bool)
    if name == 'sat' and 0 < gamma < 1:
        # q == 0 with gamma < 1: autograd multiplies the infinite slope of q^gamma at 0 by lp == 0 (NaN);
        # the definition takes the limit, 0, which the reference's own precondition asserts (focal_ref.case)
        rows[c['pick']] = False
        assert np.isnan(g.reshape(-1, c['K'])[c['pick']]).all()
    K = c['K']
    np.testing.assert_allclose(ref['grad'].reshape(-1, K)[rows], g.reshape(-1, K)[rows], rtol=1e-9, atol=1e-15)


def test_gamma_zero_is_half_cross_entropy():
    c = fr.case('base')
    ref = fr.focal(c['logits'], c['lbl'], c['pos'], 0.5, 0.0)
    x = torch.from_numpy(c['logits'].astype(np.float64)).reshape(-1, c['K'])
    t = torch.from_numpy(np.where(c['pos'] != 0, c['lbl'], 0).reshape(-1).astype(np.int64))
    ce = torch.nn.functional.cross_entropy(x, t, reduction='sum').item()
    np.testing.assert_allclose(ref['clf_loss'], 0.5 * ce / ref['norm'], rtol=1e-12)
    assert ref['norm'] == int((c['pos'] != 0).sum())


def test_float32_evaluation_reaches_the_gradient_bound():
    """The float32 evaluation of the same formula against float64: the bound the GPU test applies
    to the fp32 kernel (1e-5 |ref| + 1e-8) is reachable in float32."""
    for name in ('base', 'sat', 'satwrong', 'K2', 'K16'):
        c = fr.case(name)
        for gamma in (0.0, 0.5, 2.0, 5.0):
            r64 = fr.focal(c['logits'], c['lbl'], c['pos'], 0.25, gamma)
            r32 = fr.focal_f32(c['logits'], c['lbl'], c['pos'], 0.25, gamma)
            ex = fr.grad_excess(r32['grad'], r64['grad'], 1e-5)
            print('%s gamma %g: float32 worst error / bound %.3f' % (name, gamma, ex))
            assert ex <= 1.0, (name, gamma, ex)
            np.testing.assert_allclose(r32['clf_loss'], r64['clf_loss'], rtol=1e-5)


def test_train_flags():
    import train
    F = train.parse([])
    assert (F.clf_loss, F.focal_alpha, F.focal_gamma) == ('hnm', 0.25, 2.0)
    F = train.parse(['--train_range=ALL', '--clf_loss=focal'])
    assert (F.clf_loss, F.focal_alpha, F.focal_gamma) == ('focal', 0.25, 2.0)
    F = train.parse(['--train_range', 'ALL', '--clf_loss', 'focal', '--focal_alpha', '0.5', '--focal_gamma', '0'])
    assert (F.clf_loss, F.focal_alpha, F.focal_gamma) == ('focal', 0.5, 0.0)
    for bad in (['--focal_gamma', '-1'], ['--focal_alpha', '1.5'], ['--focal_gamma', 'inf'], ['--focal_gamma', 'nan'],
                ['--focal_alpha', 'nan'], ['--clf_loss', 'ohem']):
        with pytest.raises(SystemExit):
            train.parse(['--train_range', 'ALL', '--clf_loss', 'focal'] + bad)
    with pytest.raises(SystemExit):
        train.parse(['--clf_loss', 'focal', '--train_range', 'REFINE'])
    with pytest.raises(SystemExit):
        train.parse(['--clf_loss', 'focal'])            # the default range is REFINE
    with pytest.raises(SystemExit):
        train.parse(['--focal_gamma', '1'])


def test_train_flag_messages(capsys):
    import train
    for argv, word in ((['--train_range', 'ALL', '--clf_loss', 'focal', '--focal_gamma', '-1'], '--focal_gamma'),
                       (['--train_range', 'ALL', '--clf_loss', 'focal', '--focal_alpha', '1.5'], '--focal_alpha'),
                       (['--clf_loss', 'focal', '--train_range', 'REFINE'], 'no classifier loss')):
        with pytest.raises(SystemExit):
            train.parse(argv)
        assert word in ' '.join(capsys.readouterr().err.split())


def test_det_clf_loss_refuses_unknown_mode():
    from utils import net_tools
    with pytest.raises(ValueError, match="'hnm' or 'focal'"):
        net_tools.det_clf_loss(None, [torch.zeros(1, 1)], None, None, None, None, None, clf_loss='ohem')


def test_trainer_signature_has_the_focal_options():
    import inspect

    from rod.trainer import Trainer
    p = inspect.signature(Trainer.__init__).parameters
    assert (p['clf_loss'].default, p['focal_alpha'].default, p['focal_gamma'].default) == ('hnm', 0.25, 2.0)
    p = inspect.signature(__import__('utils.net_tools', fromlist=['x']).det_clf_loss).parameters
    assert (p['clf_loss'].default, p['focal_alpha'].default, p['focal_gamma'].default) == ('hnm', 0.25, 2.0)


def _focal_args(entry, B=1, A=8, K=11, alpha=0.25, gamma=2.0):
    if entry == 'rod_softmax_focal':
        return (None, None, None, alpha, gamma, None, None, None, B, A, K, 0, None)
    return (None, None, None, None, alpha, gamma, None, None, None, B, A, K, 0, None)


@pytest.mark.parametrize('entry', ['rod_softmax_focal', 'rod_focal_loss'])
def test_argument_refusals_name_the_argument(entry):
    from rod import _abi
    for kw, word in ((dict(K=17), 'K must be in 2..16'), (dict(K=1), 'K must be in 2..16'),
                     (dict(gamma=-0.5), 'gamma must be finite and >= 0'),
                     (dict(gamma=float('inf')), 'gamma must be finite'), (dict(gamma=float('nan')), 'gamma must be'),
                     (dict(alpha=1.5), r'alpha must be in \[0, 1\]'), (dict(alpha=-0.1), 'alpha must be in'),
                     (dict(alpha=float('nan')), 'alpha must be in'), (dict(B=0), 'B and A must be > 0'),
                     (dict(A=-3), 'B and A must be > 0')):
        with pytest.raises(RuntimeError, match=entry + ': ' + word):
            _abi.call(entry, *_focal_args(entry, **kw))
    with pytest.raises(RuntimeError, match='NULL'):      # valid scalars, no buffers: still before any launch
        _abi.call(entry, *_focal_args(entry))
    with pytest.raises(RuntimeError, match='B and A must be > 0'):
        _abi.call('rod_focal_count', None, None, None, 0, 5, None)
    with pytest.raises(RuntimeError, match='NULL'):
        _abi.call('rod_focal_count', None, None, None, 2, 5, None)
    assert _abi.query('rod_softmax_focal_workspace', 8, 129915) >= 256 + 2048 * 16
    assert _abi.query('rod_softmax_focal_workspace', 1, 37) >= 256 + 16
