"""rod_softmax_focal / rod_focal_count / rod_focal_loss (csrc/loss.hip) and the layers above
them, against tests/focal_ref.py in float64.

Shapes are the ones at which the kernel can go wrong, not the workload's (focal_ref.case): 3 x 781
rows of 11 classes = 25,773 elements (no multiple of a 16-byte vector in either dtype, 10 blocks of
256 rows with a last block of 39), 37 rows (one partial block, less than a wave), exactly 256 rows,
K = 2 and 16, a logits / gradient pointer 4 bytes (fp32) or 2 bytes (bf16) off 16-byte alignment.

Bounds (those of tests/test_gpu_loss_edges.py).  Exact: n_pos, n_neg, norm.  Losses rtol 1e-5.
fp32 gradient |got - ref| <= 1e-5 |ref| + 1e-8; bf16: the reference is evaluated at the rounded
logits and the gradient is one bf16 rounding (unit roundoff 2**-8) of such a value:
2**-8 |ref| + 1e-8.  The float32 numpy evaluation of the same formula reaches 0.05 of the fp32
bound on these inputs for every gamma (tests/test_focal_host.py).  Worst error / bound of the
kernel, measured on the MI355X (printed by _check): fp32 0.02 .. 0.05 on the base, K = 2, K = 16 and
saturated cases for gamma 0, 0.5, 2 and 5, 0.18 with 256 rows, 0.35 without positives (norm 1: larger
gradients against the same floor); bf16 0.92 .. 0.994, i.e. the bf16 rounding itself.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import focal_ref as fr  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
GAMMAS = [0.0, 0.5, 2.0, 5.0]
ALPHAS = [0.25, 0.5, 1.0]


def _dev(x, dev, dtype=None):
    t = torch.from_numpy(np.array(x)).to(dev)     # a copy: the case arrays are read-only
    return t if dtype is None else t.to(dtype)


def _offset_view(t, off):
    """A contiguous copy of t whose data pointer is `off` elements past a fresh allocation."""
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=t.device)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() == buf.data_ptr() + off * t.element_size() and buf.data_ptr() % 16 == 0
    return v


def _run(c, dev, dt, alpha, gamma, off=0):
    from rod import ops
    lg = _dev(c['logits'], dev, dt)
    if off:
        lg = _offset_view(lg, off)
    lg.requires_grad_(True)
    out, clf = ops.softmax_focal(lg, _dev(c['lbl'], dev), _dev(c['pos'], dev), alpha, gamma)
    clf.backward()
    o = out.detach().cpu().numpy()
    assert clf.item() == o[2] and lg.grad.dtype == dt and lg.grad.shape == lg.shape
    return o, lg.grad


def _check(o, grad, ref, bf16, what=''):
    assert (int(o[4]), int(o[6]), int(o[7])) == (ref['n_pos'], ref['n_neg'], ref['norm']) and o[3] == 0 and o[5] == 0
    for j, key in enumerate(('pos_loss', 'neg_loss', 'clf_loss')):
        np.testing.assert_allclose(o[j], ref[key], rtol=1e-5, atol=0, err_msg=key)
    g = grad.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all() and np.isfinite(o).all()
    ex = fr.grad_excess(g, ref['grad'], 2.0 ** -8 if bf16 else 1e-5)
    print('%s bf16=%s: gradient worst error / bound %.3f' % (what, bf16, ex))
    assert ex <= 1.0, (what, ex)


@pytest.mark.parametrize('alpha', ALPHAS)
@pytest.mark.parametrize('gamma', GAMMAS)
def test_base_fp32(dev, gamma, alpha):
    c = fr.case('base')
    ref = fr.focal(c['logits'], c['lbl'], c['pos'], alpha, gamma)
    o, grad = _run(c, dev, torch.float32, alpha, gamma)
    _check(o, grad, ref, False, 'base g%g a%g' % (gamma, alpha))
    if alpha == 1.0:     # the negatives carry weight 1 - alpha == 0: rows exactly zero
        assert ref['neg_loss'] == 0.0 and o[1] == 0.0
        assert not grad.cpu().numpy()[c['pos'] == 0].any() and grad.cpu().numpy()[c['pos'] != 0].any()


@pytest.mark.parametrize('gamma', GAMMAS)
def test_base_bf16(dev, gamma):
    c = fr.case('base', True)
    ref = fr.focal(c['logits'], c['lbl'], c['pos'], 0.25, gamma)
    o, grad = _run(c, dev, torch.bfloat16, 0.25, gamma)
    _check(o, grad, ref, True, 'base g%g' % gamma)


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('name', ['R37', 'R256', 'K2', 'K16', 'nopos', 'allpos'])
def test_shapes_and_counts(dev, name, bf16):
    c = fr.case(name, bf16)
    for gamma in (2.0, 0.5):
        ref = fr.focal(c['logits'], c['lbl'], c['pos'], 0.25, gamma)
        o, grad = _run(c, dev, torch.bfloat16 if bf16 else torch.float32, 0.25, gamma)
        _check(o, grad, ref, bf16, '%s g%g' % (name, gamma))
        if name == 'nopos':
            assert o[7] == 1 and o[0] == 0.0 and o[4] == 0
        if name == 'allpos':
            assert o[1] == 0.0 and o[6] == 0


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('gamma', GAMMAS)
@pytest.mark.parametrize('name', ['sat', 'satwrong'])
def test_saturated_rows(dev, name, gamma, bf16):
    c = fr.case(name, bf16)
    ref = fr.focal(c['logits'], c['lbl'], c['pos'], 0.25, gamma)
    pick, K = c['pick'], c['K']
    if name == 'sat':
        # q == 0 exactly: the loss is 0, and the gradient is 0 for every gamma > 0, 0.5 included; at
        # gamma == 0 (plain cross-entropy) it is -a p_k on the other classes, p_k = exp(-100) / s ~ 1e-44
        assert (ref['q'][pick] == 0).all() and not ref['fl'][pick].any()
        gp = np.abs(ref['grad'].reshape(-1, K)[pick])
        assert gp.max() < 1e-40 if gamma == 0 else not gp.any()
    else:
        assert (ref['lp'][pick] < -99).all() and (ref['pt'][pick] < 1e-37).all()
        assert np.abs(ref['grad'].reshape(-1, K)[pick]).max() > 1e-3
    o, grad = _run(c, dev, torch.bfloat16 if bf16 else torch.float32, 0.25, gamma)
    _check(o, grad, ref, bf16, '%s g%g' % (name, gamma))
    if name == 'sat':
        gk = np.abs(grad.float().cpu().numpy().reshape(-1, K)[pick])
        assert gk.max() < 1e-40 if gamma == 0 else not gk.any()


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['fp32-4B', 'bf16-2B'])
def test_unaligned_pointers(dev, dt):
    """Logits one element (4 / 2 bytes) past a 16-byte boundary with an aligned gradient (the op),
    then logits AND gradient at different offsets (the entry itself): the scalar head / tail of
    every block's span and the two LDS shifts."""
    from rod import _abi, ops
    bf16 = dt == torch.bfloat16
    c = fr.case('base', bf16)
    ref = fr.focal(c['logits'], c['lbl'], c['pos'], 0.25, 2.0)
    o, grad = _run(c, dev, dt, 0.25, 2.0, off=1)
    _check(o, grad, ref, bf16, 'logits+1')
    aligned, galigned = _run(c, dev, dt, 0.25, 2.0)
    assert np.array_equal(o.view(np.uint32), aligned.view(np.uint32)) and torch.equal(grad, galigned)
    B, A, K = c['B'], c['A'], c['K']
    lg = _offset_view(_dev(c['logits'], dev, dt), 3)
    gbuf = torch.zeros(lg.numel() + 16, dtype=dt, device=dev)
    g = gbuf[2:2 + lg.numel()].view(lg.shape)
    out = torch.empty(8, dtype=torch.float32, device=dev)
    ws = ops.workspace(_abi.query('rod_softmax_focal_workspace', B, A), dev)
    _abi.call('rod_softmax_focal', lg, _dev(c['lbl'], dev), _dev(c['pos'], dev), 0.25, 2.0, out, g, ws, B, A, K,
              ops.dtcode(lg), ops.stream())
    assert torch.equal(g, galigned) and np.array_equal(out.cpu().numpy().view(np.uint32), aligned.view(np.uint32))
    assert not gbuf[:2].any() and not gbuf[2 + lg.numel():].any()     # nothing written outside the gradient


def test_refuses_k17_and_bad_scalars(dev):
    from rod import ops
    rng = np.random.default_rng(5)
    c = fr.case('base')
    lbl, pos = _dev(c['lbl'], dev), _dev(c['pos'], dev)
    lg17 = _dev(rng.normal(0, 1, (3, 781, 17)).astype(f32), dev)
    with pytest.raises(RuntimeError, match='K must be in 2..16'):
        ops.softmax_focal(lg17, lbl, pos, 0.25, 2.0)
    with pytest.raises(RuntimeError, match='K must be in 2..16'):
        ops.focal_lockstep([(lg17, lbl, pos)], 0.25, 2.0, lambda ts: None)
    lg = _dev(c['logits'], dev)
    with pytest.raises(RuntimeError, match='gamma must be'):
        ops.softmax_focal(lg, lbl, pos, 0.25, -1.0)
    with pytest.raises(RuntimeError, match='alpha must be'):
        ops.softmax_focal(lg, lbl, pos, 1.5, 2.0)


def test_no_grad_path(dev):
    from rod import _abi, ops
    c = fr.case('base')
    o, _ = _run(c, dev, torch.float32, 0.25, 2.0)
    lg = _dev(c['logits'], dev).requires_grad_(True)
    calls, real = [], _abi.call
    _abi.call = lambda name, *a: (calls.append((name, a)), real(name, *a))[1]
    try:
        with torch.no_grad():
            out, clf = ops.softmax_focal(lg, _dev(c['lbl'], dev), _dev(c['pos'], dev), 0.25, 2.0)
    finally:
        _abi.call = real
    assert [n for n, _ in calls] == ['rod_softmax_focal'] and calls[0][1][6] is None     # grad = NULL
    assert np.array_equal(out.cpu().numpy().view(np.uint32), o.view(np.uint32)) and not clf.requires_grad


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_deterministic(dev, dt):
    c = fr.case('base', dt == torch.bfloat16)
    a, ga = _run(c, dev, dt, 0.25, 2.0)
    b, gb = _run(c, dev, dt, 0.25, 2.0)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and torch.equal(ga, gb)


def test_lockstep_two_shards(dev):
    """B = 4 as two shards of 2 with an exchange that sums the int32 counts across the list."""
    from rod import ops
    c = fr.case('B4')
    full, gfull = _run(c, dev, torch.float32, 0.25, 2.0)
    _check(full, gfull, fr.focal(c['logits'], c['lbl'], c['pos'], 0.25, 2.0), False, 'B4')
    lg, lbl, pos = _dev(c['logits'], dev), _dev(c['lbl'], dev), _dev(c['pos'], dev)
    seen = []

    def exchange(ts):
        assert all(t.dtype == torch.int32 and t.shape == (2,) for t in ts)
        seen.append([t.cpu().tolist() for t in ts])
        tot = ts[0].clone()
        for t in ts[1:]:
            tot += t
        for t in ts:
            t.copy_(tot)
    sl = [slice(0, 2), slice(2, 4)]
    res = ops.focal_lockstep([tuple(t[s].contiguous() for t in (lg, lbl, pos)) for s in sl], 0.25, 2.0, exchange)
    assert len(seen) == 1                                        # one exchange
    for (n_pos, n_neg), s in zip(seen[0], sl):                   # each shard's own counts went in
        assert n_pos == int((c['pos'][s] != 0).sum()) and n_pos + n_neg == 2 * c['A']
    outs = np.stack([o.cpu().numpy() for o, _ in res])
    for j in (4, 6, 7):                                          # the global counts and norm on both shards
        assert (outs[:, j] == full[j]).all(), (j, outs[:, j], full[j])
    for (_, g), s in zip(res, sl):
        assert torch.equal(g, gfull[s])
    for j in (0, 1, 2):
        np.testing.assert_allclose(outs[:, j].astype(np.float64).sum(), full[j], rtol=1e-6)
    # one shard is the single call
    ((o1, g1),) = ops.focal_lockstep([(lg, lbl, pos)], 0.25, 2.0, exchange)
    assert np.array_equal(o1.cpu().numpy().view(np.uint32), full.view(np.uint32)) and torch.equal(g1, gfull)


def test_dp_op_matches_single(dev):
    from rod import ops
    c = fr.case('base')
    full, gfull = _run(c, dev, torch.float32, 0.25, 2.0)
    lg = _dev(c['logits'], dev).requires_grad_(True)
    out, clf = ops.softmax_focal_dp(lg, _dev(c['lbl'], dev), _dev(c['pos'], dev), 0.25, 2.0, lambda ts: None)
    clf.backward()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), full.view(np.uint32)) and torch.equal(lg.grad, gfull)


def test_graph_replay(dev):
    from rod import ops
    ca, cb = fr.case('base'), fr.case('sat')
    eager = [_run(c, dev, torch.float32, 0.25, 2.0) for c in (ca, cb)]
    s_lg = _dev(ca['logits'], dev).requires_grad_(True)
    s_lbl, s_pos = _dev(ca['lbl'], dev), _dev(ca['pos'], dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, clf = ops.softmax_focal(s_lg, s_lbl, s_pos, 0.25, 2.0)
        (grad,) = torch.autograd.grad(clf, s_lg)
    for c, (o, gr) in ((ca, eager[0]), (cb, eager[1]), (ca, eager[0])):
        with torch.no_grad():
            s_lg.copy_(_dev(c['logits'], dev))
        s_lbl.copy_(_dev(c['lbl'], dev))
        s_pos.copy_(_dev(c['pos'], dev))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.detach().cpu().numpy().view(np.uint32), o.view(np.uint32)) and torch.equal(grad, gr)


def _recorded(fn):
    from rod import _abi
    calls, real = [], _abi.call
    _abi.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        res = fn()
    finally:
        _abi.call = real
    return res, calls


_HNM_ENTRIES = ('rod_softmax_ce_hnm', 'rod_iou_factor_bwd', 'rod_hnm_rows', 'rod_hnm_begin', 'rod_hnm_radix_hist',
                'rod_hnm_radix_scan', 'rod_hnm_loss')


def test_launch_audit_op(dev):
    """Forward + backward of the op is ONE librod entry."""
    c = fr.case('base')
    _, calls = _recorded(lambda: _run(c, dev, torch.float32, 0.25, 2.0))
    assert calls == ['rod_softmax_focal']


def test_launch_audit_refine_trained(dev):
    """The ODM chain with refine_out trained (fix_refine=False): with focal loss nothing reaches
    refine_out through the classifier loss (no rod_iou_factor_bwd), the smooth-L1 path still does."""
    import test_gpu_loss_edges as le
    from rod import graph, ops
    c = le.grad_case('plain')

    def chain():
        ro = le._dev(c['ro'], dev).requires_grad_(True)
        dgt, dpos, dlbl, iou = ops.det_targets(le._dev(c['anc'], dev), ro, le._dev(c['rgt'], dev),
                                               le._dev(c['cbox'], dev), le._dev(c['label'], dev),
                                               le._dev(c['rpos'], dev), c['lvl_off'], c['thr'])
        do = le._dev(c['det_out'], dev).requires_grad_(True)
        lg = le._dev(c['logits'], dev).requires_grad_(True)
        _, det_tot = ops.smooth_l1_masked(do, dgt, dpos, c['lvl_off'], c['bs'])
        out, clf = ops.softmax_focal(lg, dlbl, dpos, 0.25, 2.0)
        graph.backward(graph.scalar_sum(det_tot, clf))
        return ro.grad, lg.grad, out, dpos, dlbl
    (g_ro, g_lg, out, dpos, dlbl), calls = _recorded(chain)
    assert calls.count('rod_softmax_focal') == 1 and 'rod_det_targets_bwd' in calls
    assert not any(n in calls for n in _HNM_ENTRIES), calls
    ref = fr.focal(c['logits'], dlbl.cpu().numpy(), dpos.cpu().numpy(), 0.25, 2.0)
    _check(out.cpu().numpy(), g_lg, ref, False, 'chain')
    # refine_out's gradient is the smooth-L1 one alone: zero off the ODM positives
    assert g_ro is not None and not g_ro.cpu().numpy()[dpos.cpu().numpy() == 0].any()


def test_trainer_focal(dev):
    import config
    from rod.data import synthetic_batch
    from rod.trainer import Trainer
    H, W, B = 288, 512, 2
    kw = dict(dtype=torch.float32, device=dev, train_range=config.train_range.ALL, seed=5)
    batch = synthetic_batch(B, H, W, dev, seed=6)
    ta = Trainer((H, W), B, clf_loss='focal', **kw)
    losses, calls = _recorded(lambda: ta.losses(*batch))
    assert calls.count('rod_softmax_focal') == 1 and not any(n in calls for n in _HNM_ENTRIES)
    clf_out = ta.last_out[2]
    logits = np.concatenate([t.detach().cpu().numpy().reshape(B, -1, config.total_obj_n) for t in clf_out], 1)
    _, dpos, dlbl, _ = ta.last_targets[1].flat
    ref = fr.focal(logits, dlbl.cpu().numpy(), dpos.cpu().numpy(), 0.25, 2.0)
    assert ref['n_pos'] > 0
    np.testing.assert_allclose(losses[3].item(), ref['clf_loss'], rtol=1e-5)
    from utils import net_tools
    st = net_tools.det_clf_loss.last_stats.cpu().numpy()
    assert (int(st[4]), int(st[6]), int(st[7])) == (ref['n_pos'], ref['n_neg'], ref['norm'])
    # one eager step then one graphed step == two eager steps, bit for bit
    tb = Trainer((H, W), B, clf_loss='focal', **kw)
    ta.step(*batch)
    assert ta.graph_mode() == 'full'
    ta.step_graphed(*batch)
    assert hasattr(ta, '_graph')
    tb.step(*batch)
    tb.step(*batch)
    torch.cuda.synchronize()
    assert torch.equal(ta.net.store.flat, tb.net.store.flat)
    # the default trainer still runs the hard-negative mining
    td = Trainer((H, W), B, **kw)
    _, calls = _recorded(lambda: td.losses(*batch))
    assert 'rod_softmax_ce_hnm' in calls and 'rod_softmax_focal' not in calls
