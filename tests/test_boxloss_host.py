"""IoU / GIoU / DIoU / CIoU box loss, the parts that need no GPU: the numpy restatement
(tests/boxloss_ref.py) against finite differences and analytic facts, the float32 restatement's own
error (which sets the GPU test's bounds), the CLI flags, the host layers' mode check and the argument
checks of rod_box_iou_loss (they return before any HIP call, as in tests/test_abi.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boxloss_ref as br  # noqa: E402

KINDS = list(br.KINDS)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['base', 'inside', 'outside', 'disjoint', 'thin'])
def test_closed_form_gradient_is_finite_differences(name, kind):
    """Central differences of the float64 row loss in each component of s, step 1e-6, CIoU's alpha held at
    its value at s (the definition: alpha is a constant in the gradient).  Error of the difference
    quotient: rounding 2**-53 |row| / step <= 1e-9 for |row| <= 3, truncation step^2 / 6 |f'''| <= 1e-9
    for third derivatives up to 6e3; the bound is 1e-6 of the row's largest component + 1e-7, a hundred
    times that.  Rows within 1e-4 anchor sizes of a max / min tie are not differentiable within the step
    and are left out (at most 2 per case; `same`, all ties, is left out altogether).
    Measured worst error / bound: 2.7e-4 .. 6.8e-4, 4.9e-3 on thin (0 for disjoint / iou)."""
    c = br.case(name)
    w, sc, step = 0.75, 3.0, 1e-6
    s0 = br.summed_offsets(c['ro'], c['do']).astype(np.float64)
    a = (c['anc'], None, None, c['cbox'], c['pos'], c['lvl_off'], kind, w, sc)
    ref = br.box_loss(*a, s=s0)
    fd = np.zeros_like(ref['grad'])
    for k in range(4):
        e = np.zeros(4)
        e[k] = step
        hi, lo = br.box_loss(*a, s=s0 + e, alpha=ref['alpha']), br.box_loss(*a, s=s0 - e, alpha=ref['alpha'])
        fd[..., k] = (hi['row'] - lo['row']) / (2 * step) * (w / sc)
    keep = (c['pos'] != 0) & (ref['tie'] > 1e-4)
    assert ((c['pos'] != 0) & ~keep).sum() <= 2 and keep.sum() > 100
    ex = br.grad_excess(fd[keep], ref['grad'][keep], 1e-6, floor=1e-7)
    print('%s %s: finite differences worst error / bound %.2e' % (name, kind, ex))
    assert ex <= 1.0, (name, kind, ex)
    assert np.abs(ref['grad'][keep]).max() > 1e-3 or (name == 'disjoint' and kind == 'iou')


def test_same_box_has_zero_loss():
    for bf16 in (False, True):
        c = br.case('same', bf16)
        for kind in KINDS:
            for T in (np.float64, np.float32):
                r = br.box_loss(c['anc'], c['ro'], c['do'], c['cbox'], c['pos'], c['lvl_off'], kind, dtype=T)
                assert not r['row'].any() and r['total'] == 0.0 and not r['lvl'].any()
                assert (r['iou'][c['pos'] != 0] == 1.0).all()


def test_disjoint_boxes_move_only_under_the_enclosing_terms():
    c = br.case('disjoint')
    m = c['pos'] != 0
    assert not br.reference('disjoint', 'iou')['grad'].any()
    for kind in ('giou', 'diou', 'ciou'):
        g = br.reference('disjoint', kind)['grad']
        assert (np.abs(g[m]).max(-1) > 1e-4).all() and not g[~m].any()


@pytest.mark.parametrize('name', br.CASES)
def test_ciou_ge_diou_ge_iou_row_by_row(name):
    r = {k: br.reference(name, k)['row'] for k in KINDS}
    assert (r['ciou'] >= r['diou']).all() and (r['diou'] >= r['iou']).all()
    assert (r['giou'] >= r['iou'] - 1e-15).all()           # (C - U) / C >= 0 up to the rounding of C - U
    if name not in ('nopos', 'same', 'disjoint'):
        assert (r['ciou'] > r['diou']).any() and (r['diou'] > r['iou']).any()


def test_float32_restatement_error():
    """The float32 evaluation of the same formula against float64, on every case, kind and both
    roundings of the inputs: gradient error beyond FLOOR relative to the row's largest component,
    level-sum error beyond LOSS_FLOOR relative to the sum.  Measured: gradient 2.11e-5 on `thin` (a box
    0.01 wide at a coordinate near 0.5: cx +- w/2 loses 6 bits), <= 4.1e-6 elsewhere; losses 1.62e-6 on
    `thin`, <= 1.5e-7 elsewhere.  E32_GRAD = 2.5e-5 and E32_LOSS = 2e-6 are these rounded up, and they
    are tight: the measured worst is above half of each."""
    wg = wl = 0.0
    for name in br.CASES:
        for bf16 in (False, True):
            c = br.case(name, bf16)
            for kind in KINDS:
                a = (c['anc'], c['ro'], c['do'], c['cbox'], c['pos'], c['lvl_off'], kind, 1.0, 3.0)
                r64, r32 = br.reference(name, kind, bf16), br.box_loss(*a, dtype=np.float32)
                d = np.abs(r32['grad'] - r64['grad'])
                rm = np.abs(r64['grad']).max(-1, keepdims=True)
                with np.errstate(all='ignore'):
                    eg = float(np.where(d > br.FLOOR, (d - br.FLOOR) / rm, 0.0).max())
                el = 0.0
                for x, y in zip(list(r32['lvl']) + [r32['total']], list(r64['lvl']) + [r64['total']]):
                    if abs(x - y) > br.LOSS_FLOOR:
                        el = max(el, (abs(x - y) - br.LOSS_FLOOR) / abs(y))
                if eg > 5e-6 or el > 5e-7:
                    print('%s %s bf16=%s: float32 gradient error %.2e, loss error %.2e' % (name, kind, bf16, eg, el))
                wg, wl = max(wg, eg), max(wl, el)
                assert br.grad_excess(r32['grad'], r64['grad'], br.E32_GRAD) <= 1.0, (name, kind, bf16)
    print('float32 restatement: worst gradient error %.3e, worst loss error %.3e' % (wg, wl))
    assert br.E32_GRAD / 2 < wg <= br.E32_GRAD and br.E32_LOSS / 2 < wl <= br.E32_LOSS


def _args(B=1, A=8, L=1, kind=1, weight=1.0, scale=1.0, lvl=None):
    lvl = np.array([0, A] if lvl is None else lvl, np.int32)
    return (None, None, None, None, None, lvl, L, kind, weight, scale, None, None, None, B, A, 0, None)


def test_argument_refusals_name_the_argument():
    from rod import _abi
    for kw, word in ((dict(kind=4), 'kind must be 0'), (dict(kind=-1), 'kind must be 0'),
                     (dict(scale=0.0), 'scale must be non-zero'),
                     (dict(weight=-0.5), 'weight must be finite and >= 0'),
                     (dict(weight=float('inf')), 'weight must be finite'), (dict(weight=float('nan')), 'weight must be'),
                     (dict(B=0), 'B and A must be > 0'), (dict(A=-3), 'B and A must be > 0'),
                     (dict(L=0), 'levels: L=0 out of range'), (dict(L=9, lvl=[0] * 9 + [8]), 'levels: L=9 out of range'),
                     (dict(L=2, lvl=[0, 9, 8]), 'levels: offsets must be monotone'),
                     (dict(L=2, lvl=[1, 4, 8]), r'levels: offsets must span \[0, A\]'),
                     (dict(L=2, lvl=[0, 4, 7]), r'levels: offsets must span \[0, A\]')):
        with pytest.raises(RuntimeError, match=word):
            _abi.call('rod_box_iou_loss', *_args(**kw))
    with pytest.raises(RuntimeError, match='rod_box_iou_loss: kind'):
        _abi.call('rod_box_iou_loss', *_args(kind=7))
    with pytest.raises(RuntimeError, match='lvl_off is a host array'):
        _abi.call('rod_box_iou_loss', *(_args()[:5] + (None,) + _args()[6:]))
    with pytest.raises(RuntimeError, match='NULL'):      # valid scalars and levels, no buffers: before any launch
        _abi.call('rod_box_iou_loss', *_args())
    assert _abi.query('rod_box_iou_loss_workspace', 8, 129915) == _abi.query('rod_smoothl1_workspace', 8, 129915)
    assert _abi.lib().rod_abi_version() >= 27


def test_train_flags():
    import train
    F = train.parse([])
    assert (F.loc_loss, F.loc_loss_weight) == ('smooth_l1', 1.0)
    for k in KINDS:
        F = train.parse(['--train_range=ALL', '--loc_loss=' + k])
        assert (F.loc_loss, F.loc_loss_weight, F.clf_loss) == (k, 1.0, 'hnm')
    F = train.parse(['--train_range', 'ALL', '--loc_loss', 'ciou', '--loc_loss_weight', '2.5', '--clf_loss', 'focal'])
    assert (F.loc_loss, F.loc_loss_weight, F.clf_loss) == ('ciou', 2.5, 'focal')
    assert train.parse(['--train_range', 'ALL', '--loc_loss', 'giou', '--loc_loss_weight', '0']).loc_loss_weight == 0.0
    for bad in (['--loc_loss_weight', '-1'], ['--loc_loss_weight', 'inf'], ['--loc_loss_weight', 'nan'],
                ['--loc_loss', 'eiou']):
        with pytest.raises(SystemExit):
            train.parse(['--train_range', 'ALL', '--loc_loss', 'giou'] + bad)
    with pytest.raises(SystemExit):
        train.parse(['--loc_loss', 'giou', '--train_range', 'REFINE'])
    with pytest.raises(SystemExit):
        train.parse(['--loc_loss', 'giou'])              # the default range is REFINE
    with pytest.raises(SystemExit):
        train.parse(['--train_range', 'ALL', '--loc_loss_weight', '2'])


def test_train_flag_messages(capsys):
    import train
    for argv, word in ((['--train_range', 'ALL', '--loc_loss', 'giou', '--loc_loss_weight', '-1'], '--loc_loss_weight must be'),
                       (['--train_range', 'ALL', '--loc_loss_weight', '2'], 'needs --loc_loss'),
                       (['--loc_loss', 'giou', '--train_range', 'REFINE'], 'no ODM box loss')):
        with pytest.raises(SystemExit):
            train.parse(argv)
        assert word in ' '.join(capsys.readouterr().err.split())


def test_host_layers_refuse_unknown_names():
    from rod import ops
    from rod.trainer import Trainer
    from utils import net_tools
    with pytest.raises(ValueError, match="loc_loss must be 'smooth_l1', 'iou'"):
        net_tools.det_clf_loss(None, [torch.zeros(1, 1)], None, None, None, None, None, loc_loss='x')
    with pytest.raises(ValueError, match='kind must be one of'):
        ops.box_iou_loss(None, None, None, None, None, (0, 1), 'x', 1.0, 1.0)
    import inspect
    p = inspect.signature(Trainer.__init__).parameters
    assert (p['loc_loss'].default, p['loc_loss_weight'].default) == ('smooth_l1', 1.0)
    p = inspect.signature(net_tools.det_clf_loss).parameters
    assert (p['loc_loss'].default, p['loc_loss_weight'].default, p['refine_flat'].default) == ('smooth_l1', 1.0, None)
