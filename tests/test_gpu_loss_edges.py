"""The ODM loss kernels op by op at their edges, fp32 and bf16, against oracle/post.py.

  rod_det_targets / rod_det_targets_bwd            (csrc/detect.hip)
  rod_softmax_ce_hnm, rod_hnm_*, rod_iou_factor_bwd (csrc/loss.hip)
  rod_smoothl1_masked, rod_boxes_convert            (csrc/targets.hip)
  rod_decode / rod_softmax with bf16 inputs         (csrc/detect.hip)

All of them take an arbitrary [A, 4] anchor table and arbitrary level offsets, so the edges
are built on a synthetic table of 781 anchors (levels of 1, 6, 256, 513 and 5 anchors) with
dyadic coordinates: exact ties (IoU exactly 0, 0.5 or 1, shared box edges) are then the same
ties in float32 and in the float64 reference.

Bounds.  Bit-exact: the ODM targets, every integer decision and the hard-negative threshold.
fp32: losses rtol 1e-5, logits gradient rtol 1e-5 + 1e-8, smooth-L1 gradient rtol 1e-6 (one
rounding: * (1/scale) against / scale).  bf16 inputs: the reference is evaluated at the
rounded inputs; the kernels convert to fp32 first, so decisions stay bit-exact and a bf16
gradient is one more rounding of a value already within 1e-5: 2**-8 |ref| + 1e-8 (2**-8 is
the unit roundoff of bf16, so this bound has next to no headroom: worst error / bound 0.97).
The refine_out gradient (section 4) is bounded elementwise by the reference's own
float32-against-float64 scatter, see _scatter_tol.

Every case asserts the precondition of the edge it is there for on the reference side, so a
case that stops exercising its edge fails.  The input builders and references are plain
numpy / PyTorch-CPU functions (the *_case functions and _oracle_grad); only the test bodies
touch the device.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import post as op
from oracle.targets import exp_cr

pytestmark = pytest.mark.gpu
f32 = np.float32

LVL5 = (0, 1, 7, 263, 776, 781)                  # level sizes 1, 6, 256, 513, 5
LVL1 = (0, 781)
LVL8 = (0, 1, 7, 135, 263, 519, 776, 780, 781)   # one-anchor levels first and last
B, A, K = 3, 781, 11


def _bf(x):
    """float32 array rounded to bfloat16 (round to nearest even) and back."""
    return torch.from_numpy(np.array(x, f32)).to(torch.bfloat16).float().numpy()


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return d


def _thaw(d):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}


@functools.lru_cache(None)
def _layout(K=K):
    """The common layout (read-only arrays): dyadic anchors, cbox = anchor + small centre
    noise with about half of the rows shifted far away (IoU exactly 0, many ties at the group
    minimum), refine_out ~ N(0, 0.15), refine_pos ~ Bernoulli(0.6), labels in 1..K-1."""
    rng = np.random.default_rng(20)
    q = lambda lo, hi, shape: (rng.integers(lo, hi + 1, shape) / 64.0).astype(f32)
    anc = np.concatenate([q(8, 56, (A, 2)), q(4, 32, (A, 2))], 1)
    cbox = np.broadcast_to(anc, (B, A, 4)).copy()
    cbox[..., :2] += rng.normal(0, 0.02, (B, A, 2)).astype(f32)
    far = rng.random((B, A)) < 0.5
    cbox[..., 0] += np.where(far, f32(4), f32(0))
    return _frozen(dict(
        anc=anc, cbox=cbox, far=far, K=K, bs=float(B), lvl_off=LVL5, thr=(0.5,) * 5,
        ro=rng.normal(0, 0.15, (B, A, 4)).astype(f32), rgt=rng.normal(0, 0.3, (B, A, 4)).astype(f32),
        rpos=(rng.random((B, A)) < 0.6).astype(np.int32), label=rng.integers(1, K, (B, A)).astype(np.int32),
        logits=rng.normal(0, 2.0, (B, A, K)).astype(f32), det_out=rng.normal(0, 0.3, (B, A, 4)).astype(f32)))


def _with_levels(c, lvl_off):
    c['lvl_off'] = tuple(lvl_off)
    c['thr'] = (0.5,) * (len(lvl_off) - 1)
    return c


def _targets(c):
    """(det_gt, det_pos, det_lbl, iou) of the numpy oracle."""
    return op.det_groundtruth(c['anc'], c['lvl_off'], c['thr'], c['ro'], c['rgt'], c['cbox'], c['label'], c['rpos'])


def _dev(x, dev, dtype=None):
    t = torch.from_numpy(np.array(x)).to(dev)     # a copy: the case arrays are read-only
    return t if dtype is None else t.to(dtype)


# ------------------------------------------------------------------ 1. det_targets forward
def det_targets_case(name):
    if name in ('common', 'common_bf16', 'L1', 'L8', 'L8_bf16'):
        c = _thaw(_layout())
        if name.startswith('L1'):
            _with_levels(c, LVL1)
        if name.startswith('L8'):
            _with_levels(c, LVL8)
        if name.endswith('bf16'):
            c['ro'] = _bf(c['ro'])
        r = _targets(c)
        assert r[1].sum() > 100 and (r[3] == 0).sum() > 500 and np.isfinite(r[3]).all()
        return c, r
    assert name == 'edges'
    # two levels over the same four 1x1 / 2x2 anchors: threshold 0.5 and the next float above
    unit = [0.5, 0.5, 1.0, 1.0]
    anc = np.array([unit, unit, unit, [1.0, 1.0, 2.0, 2.0]] * 2, f32)
    gts = np.array([[0.5, 0.5, 1.0, 0.5],    # 1 x 0.5 inside: inter 0.5, union 1, iou == 0.5
                    [0.5, 0.5, 1.0, 1.0],    # cbox == anchor: iou == 1
                    [0.5, 1.5, 1.0, 1.0],    # shared edge x == 1: inter == 0
                    [2.5, 1.0, 1.0, 2.0]], f32)   # shared edge y == 2 of the 2x2 anchor
    c = dict(anc=anc, cbox=np.tile(gts, (2, 1))[None], ro=np.zeros((1, 8, 4), f32),
             rgt=np.arange(32, dtype=f32).reshape(1, 8, 4) / 8, label=np.arange(1, 9, dtype=np.int32)[None],
             rpos=np.ones((1, 8), np.int32), lvl_off=(0, 4, 8), thr=(f32(0.5), np.nextafter(f32(0.5), f32(1))))
    r = _targets(c)
    assert r[3][0].tolist() == [0.5, 1.0, 0.0, 0.0] * 2
    assert r[1][0].tolist() == [1, 1, 0, 0, 0, 1, 0, 0]   # iou == thr is positive, one ulp above is not
    return c, r


@pytest.mark.parametrize('name', ['common', 'common_bf16', 'L1', 'L8', 'L8_bf16', 'edges'])
def test_det_targets_bit_exact(dev, name):
    from rod import ops
    c, ref = det_targets_case(name)
    dt = torch.bfloat16 if name.endswith('bf16') else torch.float32
    got = ops.det_targets(_dev(c['anc'], dev), _dev(c['ro'], dev, dt), _dev(c['rgt'], dev), _dev(c['cbox'], dev),
                          _dev(c['label'], dev), _dev(c['rpos'], dev), c['lvl_off'], c['thr'])
    assert got[0].dtype == torch.float32 and got[3].dtype == torch.float32
    for g, r, what in zip(got, ref, ('det_gt', 'det_pos', 'det_lbl', 'iou')):
        np.testing.assert_array_equal(g.cpu().numpy(), r, err_msg=what)


# ------------------------------------------------------------------ 2. softmax_ce_hnm
def _hnm_inputs(lvl_off=LVL5, K=K):
    c = _with_levels(_thaw(_layout(K)), lvl_off)
    _, pos, lbl, iou = _targets(c)
    return dict(logits=c['logits'], pos=pos.copy(), lbl=lbl.copy(), iou=iou, lvl_off=c['lvl_off'], bs=c['bs'], K=K)


@functools.lru_cache(None)
def hnm_case(name, bf16=False):
    """(inputs, det_clf_loss reference) of one hard-negative-mining case; preconditions are
    asserted on the reference.  Read-only."""
    rng = np.random.default_rng(31)
    h = _hnm_inputs(LVL1 if name == 'L1' else LVL8 if name == 'L8' else LVL5,
                    2 if name == 'K2' else 16 if name == 'K16' else K)
    Kc = h['K']
    relabel = lambda: (rng.integers(1, Kc, (B, A)) * h['pos']).astype(np.int32)
    if name == 'nopos':
        h['pos'][:] = 0
        h['lbl'][:] = 0
    elif name == 'allpos':
        h['pos'][:] = 1
        h['lbl'] = relabel()
    elif name in ('clamped', 'p0_one_thr'):
        h['pos'] = (rng.random((B, A)) < 0.6).astype(np.int32)
        h['lbl'] = relabel()
    elif name == 'ties':
        h['logits'] = np.round(h['logits'] * f32(0.3)).astype(f32)
    elif name == 'mixed':          # image 0 all positive, image 1 without positives
        h['pos'][0] = 1
        h['pos'][1] = 0
        h['lbl'] = relabel()
    elif name == 'p0_zero_thr':    # two positives: k = 9 falls inside the run of p0 == 0
        h['pos'][:] = 0
        h['pos'][0, 300] = h['pos'][2, 500] = 1
        h['lbl'] = relabel()
    elif name == 'L8':             # the one-anchor last level holds a positive
        h['pos'][:, 780] = 1
        h['lbl'][:, 780] = 3
    if name.startswith('p0_'):
        neg = np.argwhere(h['pos'] == 0)
        pick = neg[rng.permutation(len(neg))[:80]]
        mx = h['logits'][..., 1:].max(-1)
        for j, (b, a) in enumerate(pick):
            h['logits'][b, a, 0] = mx[b, a] + (f32(200) if j % 2 else f32(-200))
    if bf16:
        h['logits'] = _bf(h['logits'])
    z4 = np.zeros((B, A, 4), f32)
    ref = op.det_clf_loss(z4, z4, h['pos'], h['logits'], h['lbl'], h['iou'], h['lvl_off'], h['bs'])
    # ---- preconditions
    flat_pos = h['pos'].reshape(-1) != 0
    e, s, _ = op.softmax_rows(h['logits'].reshape(-1, Kc))
    nv = np.where(flat_pos, f32(1), (e[:, 0:1] / s)[:, 0])
    n_neg = int((~flat_pos).sum())
    thr = f32(ref['max_hard_pred'])
    assert np.isfinite(ref['g_logits']).all() and np.isfinite([ref['pos_loss'], ref['neg_loss']]).all()
    if name in ('normal', 'L1', 'L8', 'K2', 'K16'):
        assert ref['n_pos'] > 100 and 0 < ref['k'] < n_neg and ref['n_neg_selected'] == ref['k'] - 1
    if name == 'nopos':
        assert ref['n_pos'] == 0 and ref['k'] == B and ref['pos_loss'] == 0.0 and ref['n_neg_selected'] < ref['k']
    if name == 'allpos':
        assert n_neg == 0 and ref['k'] == 0 and thr == 0 and ref['n_neg_selected'] == 0 and ref['neg_loss'] == 0.0
    if name in ('clamped', 'p0_one_thr'):
        assert ref['k'] == n_neg > 0 and thr == nv[~flat_pos].max()
    if name == 'ties':
        assert ((nv == thr) & ~flat_pos).sum() > 1 and ref['n_neg_selected'] < ref['k'] - 1
    if name == 'mixed':
        assert h['pos'][0].all() and not h['pos'][1].any() and 0 < ref['k'] <= n_neg
    if name.startswith('p0_'):
        assert ((nv == 0) & ~flat_pos).sum() >= 30 and ((nv == 1) & ~flat_pos).sum() >= 30
    if name == 'p0_zero_thr':
        assert thr == 0 and ref['k'] == 9 and ref['n_neg_selected'] == 0
    if name == 'p0_one_thr':       # negatives with p0 == 1 tie with the positives' 1.0 and are not selected
        assert thr == 1 and ref['n_neg_selected'] == n_neg - ((nv == 1) & ~flat_pos).sum()
    if name == 'L8':               # constant-IoU group: factor 0, zero loss and zero gradient
        assert (ref['iouf'].reshape(B, A)[:, 780] == 0).all() and not ref['negmask'].reshape(B, A)[:, 780].any()
    return _frozen(h), ref


HNM_CASES = ['normal', 'nopos', 'allpos', 'clamped', 'ties', 'mixed', 'p0_edges', 'p0_zero_thr', 'p0_one_thr',
             'K2', 'K16', 'L1', 'L8']


def _hnm_dev_args(h, dev, dt):
    return (_dev(h['logits'], dev, dt), _dev(h['lbl'], dev), _dev(h['pos'], dev), _dev(h['iou'], dev))


def _run_hnm(h, dev, dt):
    from rod import ops
    lg, lbl, pos, iou = _hnm_dev_args(h, dev, dt)
    lg.requires_grad_(True)
    out, clf = ops.softmax_ce_hnm(lg, lbl, pos, iou, h['lvl_off'], h['bs'])
    clf.backward()
    o = out.detach().cpu().numpy()
    assert clf.item() == o[2] and lg.grad.dtype == dt
    return o, lg.grad


def _check_hnm(o, grad, ref, bf16):
    assert int(o[5]) == ref['k'] and int(o[4]) == ref['n_pos']
    assert o[3] == f32(ref['max_hard_pred'])
    assert int(o[6]) == ref['n_neg_selected']
    for j, key in enumerate(('pos_loss', 'neg_loss', 'clf_loss')):
        np.testing.assert_allclose(o[j], ref[key], rtol=1e-5, atol=0, err_msg=key)
    g = grad.float().cpu().numpy()
    r = ref['g_logits']
    if bf16:   # one bf16 rounding (unit roundoff 2**-8) of a value within 1e-5: derived, not measured
        bad = np.abs(g - r) > 2.0 ** -8 * np.abs(r) + 1e-8
        assert not bad.any(), (int(bad.sum()), np.abs(g - r)[bad][:5], r[bad][:5])
    else:
        np.testing.assert_allclose(g, r, rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize('name', HNM_CASES)
def test_softmax_ce_hnm_edges(dev, name):
    h, ref = hnm_case(name)
    o, grad = _run_hnm(h, dev, torch.float32)
    _check_hnm(o, grad, ref, False)
    if name == 'nopos':
        assert o[0] == 0.0
    if name == 'allpos':
        assert o[1] == 0.0 and o[3] == 0.0 and o[5] == 0 and o[6] == 0
    if name == 'L8':
        assert not grad[:, 780].cpu().numpy().any()


@pytest.mark.parametrize('name', ['normal', 'ties', 'clamped'])
def test_softmax_ce_hnm_bf16(dev, name):
    h, ref = hnm_case(name, True)
    o, grad = _run_hnm(h, dev, torch.bfloat16)
    _check_hnm(o, grad, ref, True)


def test_softmax_ce_hnm_refuses_k17(dev):
    from rod import ops
    rng = np.random.default_rng(5)
    h, _ = hnm_case('normal')
    h = dict(h, logits=rng.normal(0, 1, (B, A, 17)).astype(f32))
    lg, lbl, pos, iou = _hnm_dev_args(h, dev, torch.float32)
    with pytest.raises(RuntimeError, match='K <= 16'):
        ops.softmax_ce_hnm(lg, lbl, pos, iou, h['lvl_off'], h['bs'])
    with pytest.raises(RuntimeError):
        ops.hnm_lockstep([(lg, lbl, pos, iou)], h['lvl_off'], h['bs'], B, lambda ts: None)


@pytest.mark.parametrize('shards', [1, 3])
@pytest.mark.parametrize('name', ['nopos', 'ties', 'clamped', 'mixed'])
def test_hnm_lockstep_edges(dev, name, shards):
    """The split rod_hnm_* entries (the batch over `shards` emulated ranks, the exchange
    summing the int32 counts and histograms) against the single-launch entry."""
    from rod import ops
    h, ref = hnm_case(name)
    full, gfull = _run_hnm(h, dev, torch.float32)
    assert int(full[5]) == ref['k'] and full[3] == f32(ref['max_hard_pred'])
    lg, lbl, pos, iou = _hnm_dev_args(h, dev, torch.float32)

    def exchange(ts):
        tot = ts[0].clone()
        for t in ts[1:]:
            tot += t
        for t in ts:
            t.copy_(tot)
    per = B // shards
    sl = [slice(r * per, (r + 1) * per) for r in range(shards)]
    res = ops.hnm_lockstep([tuple(t[s].contiguous() for t in (lg, lbl, pos, iou)) for s in sl], h['lvl_off'], h['bs'],
                           B, exchange)
    outs = np.stack([o.cpu().numpy() for o, _ in res])
    for j in (3, 4, 5):
        assert (outs[:, j].view(np.uint32) == full[j:j + 1].view(np.uint32)).all(), (j, outs[:, j], full[j])
    assert int(outs[:, 6].sum()) == int(full[6]) == ref['n_neg_selected']
    np.testing.assert_allclose(outs[:, 0].sum(), ref['pos_loss'], rtol=1e-5)
    np.testing.assert_allclose(outs[:, 1].sum(), ref['neg_loss'], rtol=1e-5)
    assert torch.equal(torch.cat([g for _, g in res]), gfull)


# ------------------------------------------------------------------ 3. smooth_l1_masked
def _run_sl1(dev, pred, target, mask, lvl_off, scale, dt=torch.float32, target_grad=False):
    from rod import ops
    p = _dev(pred, dev, dt).requires_grad_(True)
    t = _dev(target, dev).requires_grad_(target_grad)
    vec, tot = ops.smooth_l1_masked(p, t, _dev(mask, dev), lvl_off, scale)
    tot.backward()
    L = len(lvl_off) - 1
    assert tot.item() == vec[L].item() and p.grad.dtype == dt
    return vec.cpu().numpy().astype(np.float64), p.grad, t.grad


@functools.lru_cache(None)
def smooth_l1_case(bf16=False):
    """Common layout; the last level (5 anchors) has no masked-in row and holds huge
    predictions, as do all masked-out rows of image 1."""
    c = _thaw(_layout())
    dgt, pos, _, _ = _targets(c)
    pred, mask = c['det_out'].copy(), pos.copy()
    mask[:, 776:] = 0
    rng = np.random.default_rng(7)
    huge = (10.0 ** rng.uniform(0, 30, (B, A, 4)) * rng.choice([-1, 1], (B, A, 4))).astype(f32)
    out = mask == 0
    out[0] = out[2] = False
    out[:, 776:] = True
    pred[out] = huge[out]
    if bf16:
        pred = _bf(pred)
    assert np.isfinite(pred).all() and np.abs(pred[out]).max() > 1e29 and (mask[:, :776].sum(0) > 0).any()
    lv, tot = op.smooth_l1_levels(pred, dgt, mask, LVL5, float(B))
    ref = op.det_clf_loss(pred, dgt, mask, c['logits'], np.zeros((B, A), np.int32), np.zeros((B, A), f32), LVL5,
                          float(B))
    assert all(v > 0 for v in lv[1:4]) and lv[4] == 0.0 and abs(tot - ref['det_loss']) <= 1e-12 * tot
    return _frozen(dict(pred=pred, target=dgt, mask=mask, out=out)), lv, tot, ref['g_det']


def test_smooth_l1_levels_and_masked_rows(dev):
    s, lv, tot, g_ref = smooth_l1_case()
    vec, g, gt = _run_sl1(dev, s['pred'], s['target'], s['mask'], LVL5, float(B), target_grad=True)
    np.testing.assert_allclose(vec[:5], lv, rtol=1e-5, atol=0)
    np.testing.assert_allclose(vec[5], tot, rtol=1e-5)
    assert vec[4] == 0.0                                   # a level with no masked-in row
    g = g.cpu().numpy()
    assert not g[s['mask'] == 0].any() and np.isfinite(g).all()   # masked-out rows, |pred| up to 1e30
    np.testing.assert_allclose(g, g_ref, rtol=1e-6, atol=0)
    assert gt.dtype == torch.float32 and np.array_equal(gt.cpu().numpy(), -g)   # d/d target == -d/d pred


def test_smooth_l1_kink(dev):
    """d == 0, +-1 exactly and |d| one ulp either side of 1, scale 3 (not a power of two)."""
    one = f32(1)
    up, dn = np.nextafter(one, f32(2)), np.nextafter(one, f32(0))
    d = np.array([0, 1, -1, up, -up, dn, -dn, 0.5, -0.5, 3, -3, 0], f32).reshape(1, 3, 4)
    pred = np.zeros_like(d)                                 # target - pred == d exactly
    mask = np.ones((1, 3), np.int32)
    vec, g, _ = _run_sl1(dev, pred, d, mask, (0, 1, 3), 3.0)
    ref = (-mask[..., None].astype(f32) * np.clip(d, -1, 1) / f32(3)).astype(f32)
    np.testing.assert_allclose(g.cpu().numpy(), ref, rtol=1e-6, atol=0)
    assert g.cpu().numpy()[0, 0, 0] == 0 and (np.abs(g.cpu().numpy().reshape(-1)[1:7]) > 0.33333).all()
    lv, tot = op.smooth_l1_levels(pred, d, mask, (0, 1, 3), 3.0)
    np.testing.assert_allclose(vec[:2], lv, rtol=1e-5, atol=0)
    np.testing.assert_allclose(vec[2], tot, rtol=1e-5)


def test_smooth_l1_bf16(dev):
    s, lv, tot, g_ref = smooth_l1_case(True)
    vec, g, _ = _run_sl1(dev, s['pred'], s['target'], s['mask'], LVL5, float(B), dt=torch.bfloat16)
    np.testing.assert_allclose(vec[:5], lv, rtol=1e-5, atol=0)
    np.testing.assert_allclose(vec[5], tot, rtol=1e-5)
    g = g.float().cpu().numpy()
    assert not g[s['mask'] == 0].any()
    assert (np.abs(g - g_ref) <= 2.0 ** -8 * np.abs(g_ref) + 1e-8).all()


# ------------------------------------------------------------------ 4. d / d refine_out
GRAD_CASES = ['plain', 'tie_pos', 'tie_neg', 'touch', 'const_group', 'one_pos']
TIE = (400, 401)       # two anchors of the 513-anchor level
TOUCH = slice(300, 340)


@functools.lru_cache(None)
def grad_case(name, bf16=False):
    """Inputs of one refine_out-gradient case with the oracle targets (det_gt, det_pos,
    det_lbl, iou), the hard-negative mask and the preconditions of the case.  Read-only."""
    c = _thaw(_layout())
    c['det_out'] *= f32(3)         # see _scatter_tol
    i, j = TIE
    if name == 'tie_shift':
        # tie_pos for the one-branch tests: every adjusted box about 0.8 of its anchor's size
        # and 0.1 .. 0.2 anchor sizes off centre, so that no coordinate of d iou / d refine_out
        # passes through zero on the positives (with the layout's N(0, 0.15) the height and
        # width derivatives do, and clf_loss alone then leaves 1.6 % of the live elements
        # under the absolute term; see _scatter_tol)
        rng = np.random.default_rng(77)
        sg = rng.choice([-1, 1], (B, A, 2))
        c['ro'][..., :2] = (sg * rng.uniform(0.1, 0.2, (B, A, 2))).astype(f32)
        c['ro'][..., 2:] = rng.normal(-0.2, 0.05, (B, A, 2)).astype(f32)
    if name in ('tie_pos', 'tie_neg', 'tie_shift'):
        # identical anchors, cbox == anchor, refine_out == 0: IoU exactly 1 on both, every box
        # edge ties (the <= / >= rules), reduce_max splits its gradient over the two
        c['anc'][j] = c['anc'][i]
        c['cbox'][0, (i, j)] = c['anc'][i]
        c['ro'][0, (i, j)] = 0
        c['rpos'][0, (i, j)] = 0 if name == 'tie_neg' else 1
        c['label'][0, (i, j)] = (2, 7)
    if name == 'touch':
        # cbox one anchor height below: the shared edge gives ihr == 0 exactly, iw == w > 0
        c['ro'][1, TOUCH] = 0
        c['cbox'][1, TOUCH] = c['anc'][TOUCH]
        c['cbox'][1, TOUCH, 0] += c['anc'][TOUCH, 2]
    if name == 'const_group':      # every row of (image 2, the 256-anchor level) far away
        c['cbox'][2, 7:263] = c['anc'][7:263] + np.array([4, 0, 0, 0], f32)
    if name == 'one_pos':          # the one-anchor level of image 0 holds a positive (IoU 1)
        c['cbox'][0, 0] = c['anc'][0]
        c['ro'][0, 0] = 0
        c['rpos'][0, 0] = 1
    if bf16:
        for k in ('ro', 'det_out', 'logits'):
            c[k] = _bf(c[k])
    dgt, pos, lbl, iou = _targets(c)
    if name == 'one_pos':          # exactly one positive in (image 0, the 6-anchor level)
        grp = np.flatnonzero(pos[0, 1:7]) + 1
        assert len(grp) >= 1
        c['rpos'][0, grp[1:]] = 0
        dgt, pos, lbl, iou = _targets(c)
        assert pos[0, 1:7].sum() == 1 and pos[0, 0] == 1 and iou[0, 0] == 1
    ref = op.det_clf_loss(c['det_out'], dgt, pos, c['logits'], lbl, iou, c['lvl_off'], c['bs'])
    assert pos.sum() > 100 and ref['n_neg_selected'] > 100 and np.isfinite(iou).all()
    if name in ('tie_pos', 'tie_neg', 'tie_shift'):
        u = iou[0, 263:776]
        assert iou[0, i] == 1 and iou[0, j] == 1 and (u == u.max()).sum() == 2 and u.max() == 1
        assert (u == u.min()).sum() > 100 and u.min() == 0
        assert pos[0, i] == pos[0, j] == (0 if name == 'tie_neg' else 1)
    if name == 'touch':
        assert (iou[1, TOUCH] == 0).all()
    if name == 'const_group':
        assert (iou[2, 7:263] == 0).all() and not pos[2, 7:263].any()
    c.update(det_pos=pos, det_lbl=lbl, negmask=ref['negmask'], iou=iou)
    return _frozen(c)


def _oracle_grad(c, det_pos, det_lbl, negmask, T, which='both'):
    """d (det_loss + clf_loss) / d refine_out of odm_losses_torch in dtype T (PyTorch-CPU)."""
    t = lambda k: torch.from_numpy(c[k].copy()).to(T)
    ro = t('ro').requires_grad_(True)
    _, dl, cl = op.odm_losses_torch(c['anc'].copy(), c['lvl_off'], ro, t('det_out'), t('logits'), c['rgt'].copy(),
                                    c['cbox'].copy(), c['rpos'].copy(), np.array(det_pos), np.array(det_lbl),
                                    np.array(negmask), c['bs'])
    loss = {'both': dl + cl, 'det': dl, 'clf': cl}[which]
    return torch.autograd.grad(loss, ro)[0].double().numpy()


def _live(c):
    """The rows over which _scatter_tol takes its median and its share: the ODM positives
    (smooth-L1 through det_gt, CE * d factor / d iou) and the rows at the maximum of a
    non-constant group (d den).  The IoU factor is invariant under an affine map of its group's
    IoUs, so on a row that is neither positive nor at an extreme of its group the mean / sd
    terms cancel and the reference holds rounding residue of that cancellation (|ref| ~ 1e-8).
    The rows at the group minimum receive the reduce_min split, but where the box is far away
    d iou is exactly 0 and so is the gradient.  The exception is the 'touch' case: its touching
    rows sit at the minimum with d iou != 0 (ihr >= 0) and carry |ref| up to 0.12.  They are
    not counted as live (their gradients spread down to zero); like every other element they
    are bounded by tol_abs, about 1e-4 of their size, which is what catches a wrong
    reduce_min split."""
    live = c['det_pos'] != 0
    for l in range(len(c['lvl_off']) - 1):
        u = c['iou'][:, c['lvl_off'][l]:c['lvl_off'][l + 1]]
        mx = u.max(1, keepdims=True)
        live[:, c['lvl_off'][l]:c['lvl_off'][l + 1]] |= (u == mx) & (mx > u.min(1, keepdims=True))
    return live


def _scatter_tol(g64, g32, live):
    """Elementwise bound |got - ref| <= tol_rel |ref| + tol_abs from the reference's own
    float32 scatter (odm_losses_torch in float32 against itself in float64, same inputs; 4x, as
    in the step tests): tol_abs = 4 x the largest absolute float32 error among the elements with
    |ref| below the median, tol_rel = 4 x the largest relative error among the rest.  The float32
    error of (u - mean)/sd, ^4 and the group sums depends on their conditioning and cannot be
    derived.  The median is that of the live rows (_live): four fifths of the elements are
    exactly zero or cancellation residue, which would put a median over everything at zero and
    the residue under the relative term; so they all fall below the median and under tol_abs.
    Condition for a case to be usable, measured on the reference alone: tol_rel <= 1e-3, and
    for at least 99 % of the live elements the absolute term is itself below 1e-3 |ref|, i.e.
    they are checked relatively at that level.  A case whose reference scatter does not allow
    that needs other inputs, not a wider bound (which is why section 4 uses 3 x the layout's
    det_out: fewer positives with a smooth-L1 gradient near zero)."""
    a, err = np.abs(g64), np.abs(g32 - g64)
    P = np.broadcast_to(live[..., None], a.shape) & (a > 0)
    small = a < np.median(a[P])
    tol_abs = 4 * float(err[small].max())
    tol_rel = 4 * float((err[~small] / a[~small]).max())
    share = float((tol_abs <= 1e-3 * a[P]).mean())
    return tol_rel, tol_abs, share


def _chain(dev, c, dt, which='both'):
    """The op-level chain; returns (refine_out.grad, det_pos, det_lbl, softmax_ce_hnm stats,
    names of the librod entries called during backward)."""
    from rod import _abi, graph, ops
    ro = _dev(c['ro'], dev, dt).requires_grad_(True)
    dgt, dpos, dlbl, iou = ops.det_targets(_dev(c['anc'], dev), ro, _dev(c['rgt'], dev), _dev(c['cbox'], dev),
                                           _dev(c['label'], dev), _dev(c['rpos'], dev), c['lvl_off'], c['thr'])
    do = _dev(c['det_out'], dev, dt).requires_grad_(True)
    lg = _dev(c['logits'], dev, dt).requires_grad_(True)
    _, det_tot = ops.smooth_l1_masked(do, dgt, dpos, c['lvl_off'], c['bs'])
    out, clf = ops.softmax_ce_hnm(lg, dlbl, dpos, iou, c['lvl_off'], c['bs'])
    loss = {'both': lambda: graph.scalar_sum(det_tot, clf), 'det': lambda: det_tot, 'clf': lambda: clf}[which]()
    calls, real = [], _abi.call
    _abi.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        graph.backward(loss)    # seed 1: the autograd functions assume it, the loss is not scaled
    finally:
        _abi.call = real
    return ro.grad, dpos.cpu().numpy(), dlbl.cpu().numpy(), out.cpu().numpy(), calls


def _check_refine_grad(dev, name, bf16, which='both'):
    c = grad_case(name, bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    got, dpos, dlbl, stats, calls = _chain(dev, c, dt, which)
    # the integer decisions come from the HIP forward (they equal the oracle's bit for bit)
    np.testing.assert_array_equal(dpos, c['det_pos'])
    np.testing.assert_array_equal(dlbl, c['det_lbl'])
    assert int(stats[6]) == int(c['negmask'].sum())
    g64 = _oracle_grad(c, dpos, dlbl, c['negmask'], torch.float64, which)
    g32 = _oracle_grad(c, dpos, dlbl, c['negmask'], torch.float32, which)
    tol_rel, tol_abs, share = _scatter_tol(g64, g32, _live(c))
    assert got.dtype == dt
    g = got.float().cpu().numpy().astype(np.float64)
    err = np.abs(g - g64)
    bound = (tol_rel + (2.0 ** -8 if bf16 else 0.0)) * np.abs(g64) + tol_abs
    print('%s bf16=%s %s: tol_rel %.3g tol_abs %.3g share %.4f max|ref| %.4g median %.3g worst err/bound %.3g'
          % (name, bf16, which, tol_rel, tol_abs, share, np.abs(g64).max(), np.median(np.abs(g64[g64 != 0])),
             (err / np.maximum(bound, 1e-300)).max()))
    assert np.isfinite(g).all() and np.isfinite(g64).all()
    # the case is usable (see _scatter_tol); measured on the reference alone
    assert tol_rel <= 1e-3 and share >= 0.99, (tol_rel, tol_abs, share)
    # observed over the twelve full-chain cases (reference scatter): tol_rel 1.2e-5 .. 2.5e-5,
    # tol_abs 5.3e-6 .. 1.0e-5, share 0.9909 .. 0.9945; max |ref| 393, on the tied anchors 70,
    # median of the live elements 0.3.  tie_shift, det branch alone: 5.5e-7, 9.9e-8, 1.0000;
    # clf branch alone: 2.0e-5, 1.1e-5, 0.9976
    bad = err > bound
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5], g[bad][:5], g64[bad][:5])
    return c, g, g64, calls


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('name', GRAD_CASES)
def test_refine_out_grad_elementwise(dev, name, bf16):
    c, g, g64, calls = _check_refine_grad(dev, name, bf16)
    assert 'rod_iou_factor_bwd' in calls and 'rod_det_targets_bwd' in calls
    i, j = TIE
    if name in ('tie_pos', 'tie_neg'):
        # the two tied anchors carry large gradients, each checked on its own: different ones
        # when positive (their CE differs), the bare even split of d den when not
        assert np.abs(g64[0, i]).max() > 10 and np.abs(g64[0, j]).max() > 10
        assert np.allclose(g64[0, i], g64[0, j], rtol=1e-2) == (name == 'tie_neg')
    if name == 'touch':            # max(., 0) passes the gradient at ihr == 0
        assert (g64[1, TOUCH, 0] != 0).all()
    if name == 'const_group':
        assert not g64[2, 7:263].any() and not g[2, 7:263].any()
    if name == 'one_pos':
        # a one-anchor group has constant IoU: nothing comes through the IoU factor, the
        # positive anchor keeps the smooth-L1 gradient through det_gt alone
        solo = _oracle_grad(c, c['det_pos'], c['det_lbl'], c['negmask'], torch.float64, 'det')
        assert np.array_equal(g64[:, 0], solo[:, 0]) and g64[0, 0].any() and not g[c['det_pos'][:, 0] == 0, 0].any()


@pytest.mark.parametrize('which', ['det', 'clf'])
def test_refine_out_grad_one_branch(dev, which):
    """Backward from the smooth-L1 total alone (g_iou is None: no rod_iou_factor_bwd) and
    from clf_loss alone (g_det_gt is None), on the tie at the group maximum."""
    c, g, g64, calls = _check_refine_grad(dev, 'tie_shift', False, which)
    assert 'rod_det_targets_bwd' in calls
    assert ('rod_iou_factor_bwd' in calls) == (which == 'clf')
    if which == 'det':
        assert not g[c['det_pos'] == 0].any()


def test_refine_out_grad_not_asked(dev):
    """A refine_out that requires grad but whose targets feed the losses detached: no
    gradient (None) and neither backward kernel is launched.  Autograd then never reaches
    _DetTargets.backward, so its early return for g_gt and g_iou both None is NOT exercised
    here; what is covered is _SoftmaxCEHNM.backward with needs_input_grad[3] false, which
    must not launch rod_iou_factor_bwd."""
    from rod import _abi, ops
    c = grad_case('plain')
    ro = _dev(c['ro'], dev).requires_grad_(True)
    dgt, dpos, dlbl, iou = ops.det_targets(_dev(c['anc'], dev), ro, _dev(c['rgt'], dev), _dev(c['cbox'], dev),
                                           _dev(c['label'], dev), _dev(c['rpos'], dev), c['lvl_off'], c['thr'])
    assert dgt.requires_grad and iou.requires_grad and not dpos.requires_grad
    do = _dev(c['det_out'], dev).requires_grad_(True)
    lg = _dev(c['logits'], dev).requires_grad_(True)
    _, det_tot = ops.smooth_l1_masked(do, dgt.detach(), dpos, c['lvl_off'], c['bs'])
    _, clf = ops.softmax_ce_hnm(lg, dlbl, dpos, iou.detach(), c['lvl_off'], c['bs'])
    calls, real = [], _abi.call
    _abi.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        grads = torch.autograd.grad([det_tot, clf], [ro, do, lg], [torch.ones_like(det_tot), torch.ones_like(clf)],
                                    allow_unused=True)
    finally:
        _abi.call = real
    assert grads[0] is None and grads[1] is not None and grads[2] is not None
    assert 'rod_det_targets_bwd' not in calls and 'rod_iou_factor_bwd' not in calls


# ------------------------------------------------------------------ 5. small related items
def test_decode_and_softmax_bf16_bit_exact(dev):
    from rod import ops
    c = _layout()
    a, b = _bf(c['ro']), _bf(c['det_out'])
    anc, o = c['anc'], a + b
    centre = np.stack([o[..., 0] * anc[:, 2] + anc[:, 0], o[..., 1] * anc[:, 3] + anc[:, 1],
                       exp_cr(o[..., 2]) * anc[:, 2], exp_cr(o[..., 3]) * anc[:, 3]], -1)
    for corner, ref in ((True, op.decode_corner(anc, o)), (False, centre)):
        got = ops.decode(_dev(anc, dev), _dev(a, dev, torch.bfloat16), _dev(b, dev, torch.bfloat16),
                         to_corner=corner)
        assert got.dtype == torch.float32 and ref.dtype == f32
        np.testing.assert_array_equal(got.cpu().numpy(), ref)
    got = ops.decode(_dev(c['anc'], dev), _dev(a, dev, torch.bfloat16), to_corner=True)
    np.testing.assert_array_equal(got.cpu().numpy(), op.decode_corner(c['anc'], a))
    for Kc, lg in ((K, _bf(c['logits'])), (2, _bf(c['logits'][..., :2])), (16, _bf(_layout(16)['logits']))):
        e, s, _ = op.softmax_rows(lg)
        p = ops.softmax(_dev(lg, dev, torch.bfloat16), Kc)
        assert p.dtype == torch.float32
        np.testing.assert_array_equal(p.cpu().numpy(), (e / s).astype(f32))


def test_boxes_convert_bit_exact(dev):
    from rod import ops
    rng = np.random.default_rng(3)
    ctr = np.concatenate([rng.uniform(0, 1, (B, 300, 2)), rng.uniform(0, 0.5, (B, 300, 2))], -1).astype(f32)
    ctr[0, 0, 2:] = 0          # a zero-size box
    ctr[0, 1, 2] = 0
    two = f32(2)
    cor = np.stack([ctr[..., 0] - ctr[..., 2] / two, ctr[..., 1] - ctr[..., 3] / two,
                    ctr[..., 0] + ctr[..., 2] / two, ctr[..., 1] + ctr[..., 3] / two], -1)
    got = ops.boxes_convert(_dev(ctr, dev), False).cpu().numpy()
    np.testing.assert_array_equal(got, cor)
    assert (got[0, 0, :2] == got[0, 0, 2:]).all()
    back = np.stack([(cor[..., 0] + cor[..., 2]) / two, (cor[..., 1] + cor[..., 3]) / two,
                     cor[..., 2] - cor[..., 0], cor[..., 3] - cor[..., 1]], -1)
    got = ops.boxes_convert(_dev(cor, dev), True).cpu().numpy()
    np.testing.assert_array_equal(got, back)
    assert (got[0, 0, 2:] == 0).all()
