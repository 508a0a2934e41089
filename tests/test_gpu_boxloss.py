"""rod_box_iou_loss (csrc/targets.hip) and the layers above it, against tests/boxloss_ref.py in float64.

Shapes are the ones at which the kernel can go wrong, not the workload's (boxloss_ref.case): B=3 and
levels of 37, 256 and 488 anchors (less than two waves per image; B*Al an exact multiple of the 256-row
block; a partial last block), one level, the library's 8 levels with five of them empty, pointers one
element off the row vector's alignment.

Bounds (boxloss_ref: M = 4, E32_GRAD = 2.5e-5, E32_LOSS = 2e-6, FLOOR = LOSS_FLOOR = 1e-7; E32 is the
float32 numpy restatement's own worst error against float64, measured by tests/test_boxloss_host.py):
  per-level losses and total   |got - ref| <= M E32_LOSS |ref| + LOSS_FLOOR
  fp32 gradient                |got - ref| <= M E32_GRAD max_k |ref[row, k]| + FLOOR
  bf16 gradient                the reference at the bf16-rounded refine_out / det_out (s summed in fp32),
                               the bound plus one bf16 rounding of the gradient, 2**-8 |ref|.
Worst error / bound of the kernel, measured on the MI355X (printed by _check), over the four kinds:
fp32 losses 0.002 .. 0.022 (thin 0.20), fp32 gradient 0.003 .. 0.036 on base, allpos, disjoint, inside,
outside, L1 and Lmax, 0.15 .. 0.21 on thin, 0.27 .. 0.47 on far, and on `same` 0.01 except GIoU 0.97: the
gradient cancels to zero there and the float32 restatement itself is left with 9.7e-8 against the 1e-7
floor.  bf16 losses <= 0.075, bf16 gradient 0.70 .. 0.97, i.e. the bf16 rounding itself.  Trainer (giou,
300x300, B=2): d_loss 2.729612, 0.11 of its bound.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boxloss_ref as br  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = list(br.KINDS)
W, SC = 1.0, 3.0          # weight and scale of boxloss_ref.reference


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


def _inputs(c, dev, dt, off=0):
    ro, do = _dev(c['ro'], dev, dt), _dev(c['do'], dev, dt)
    if off:
        ro, do = _offset_view(ro, off), _offset_view(do, off)
    return _dev(c['anc'], dev), ro, do, _dev(c['cbox'], dev), _dev(c['pos'], dev)


def _run(c, dev, dt, kind, weight=W, scale=SC, off=0, refine_grad=False):
    """-> ([L+1] losses as numpy, d / d det_out, d / d refine_out or None)."""
    from rod import ops
    anc, ro, do, cbox, pos = _inputs(c, dev, dt, off)
    do.requires_grad_(True)
    ro.requires_grad_(refine_grad)
    vec, tot = ops.box_iou_loss(anc, ro, do, cbox, pos, c['lvl_off'], kind, weight, scale)
    tot.backward()
    v = vec.detach().cpu().numpy()
    assert tot.item() == v[-1] and do.grad.dtype == dt and do.grad.shape == do.shape and v.shape == (len(c['lvl_off']),)
    return v, do.grad, ro.grad


def _check(v, grad, ref, bf16, what=''):
    got = np.concatenate([ref['lvl'], [ref['total']]])
    el = float((np.abs(v.astype(np.float64) - got) / (br.M * br.E32_LOSS * np.abs(got) + br.LOSS_FLOOR)).max())
    g = grad.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all() and np.isfinite(v).all()
    eg = br.grad_excess(g, ref['grad'], br.M * br.E32_GRAD, extra=2.0 ** -8 if bf16 else 0.0)
    print('%s bf16=%s: loss worst error / bound %.3f, gradient %.3f' % (what, bf16, el, eg))
    assert el <= 1.0 and eg <= 1.0, (what, el, eg)


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', br.CASES)
def test_cases_against_float64(dev, name, kind, bf16):
    c = br.case(name, bf16)
    v, grad, _ = _run(c, dev, torch.bfloat16 if bf16 else torch.float32, kind)
    _check(v, grad, br.reference(name, kind, bf16), bf16, '%s %s' % (name, kind))
    m = c['pos'] != 0
    assert not grad.float().cpu().numpy()[~m].any()          # rows off the mask: exact zeros
    if name == 'same':
        assert not v.any()                                  # prediction == target: exactly 0 in fp32 too
    if name == 'nopos':
        assert not v.any() and not grad.float().cpu().numpy().any()


@pytest.mark.parametrize('kind', KINDS)
def test_weight_zero_and_doubling(dev, kind):
    c = br.case('base')
    v0, g0, _ = _run(c, dev, torch.float32, kind, weight=0.0)
    assert not v0.any() and not g0.cpu().numpy().any()
    v1, g1, _ = _run(c, dev, torch.float32, kind, weight=1.0)
    v2, g2, _ = _run(c, dev, torch.float32, kind, weight=2.0)
    assert v1[-1] > 0.1 and g1.abs().max() > 1e-2
    # 2 w / scale and 2 w sum / scale are each one rounding from twice the single-weight values
    np.testing.assert_allclose(v2, 2.0 * v1.astype(np.float64), rtol=2.0 ** -22, atol=0)
    np.testing.assert_allclose(g2.cpu().numpy(), 2.0 * g1.cpu().numpy().astype(np.float64), rtol=2.0 ** -22, atol=0)


def test_kind0_is_one_minus_det_targets_iou(dev):
    """With det_out = 0 the prediction is the adjusted anchor of rod_det_targets and the kernel's jaccard
    is the same chain of operations: the row values 1 - iou agree bit for bit, and the level sums differ
    only in how they are added: the kernel adds a block's 256 rows in fp32 as a tree (8 levels, plus the
    two roundings of the four-wave sum: 10 roundings of 2**-24 on sums of positive terms), then in
    float64, then weight * sum / scale in fp32 (2 more): rtol 12 * 2**-24 against the float64 sum."""
    from rod import ops
    c = br.case('base')
    anc, _, _, cbox, pos = _inputs(c, dev, torch.float32)
    s = _dev(br.summed_offsets(c['ro'], c['do']), dev)
    L = len(c['lvl_off']) - 1
    _, dpos, _, iou = ops.det_targets(anc, s, torch.zeros_like(s), cbox, pos, pos, c['lvl_off'],
                                      np.zeros(L, np.float32))
    assert torch.equal(dpos, pos)
    with torch.no_grad():
        vec, _ = ops.box_iou_loss(anc, s, torch.zeros_like(s), cbox, pos, c['lvl_off'], 'iou', W, SC)
    one = (1.0 - iou.cpu().numpy().astype(np.float32)).astype(np.float64) * (c['pos'] != 0)
    want = np.array([one[:, c['lvl_off'][l]:c['lvl_off'][l + 1]].sum() * W / SC for l in range(L)])
    np.testing.assert_allclose(vec.cpu().numpy()[:L], want, rtol=12 * 2.0 ** -24, atol=0)
    np.testing.assert_allclose(vec.cpu().numpy()[L], want.sum(), rtol=14 * 2.0 ** -24, atol=0)


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['fp32-4B', 'bf16-2B'])
@pytest.mark.parametrize('kind', ['giou', 'ciou'])
def test_unaligned_pointers(dev, dt, kind):
    """refine_out / det_out one element (4 / 2 bytes) past a 16-byte boundary (the op: the scalar path with
    an aligned gradient), then the gradient off alignment too (the entry itself): bit-identical results
    and nothing written outside the gradient."""
    from rod import _abi, ops
    bf16 = dt == torch.bfloat16
    c = br.case('base', bf16)
    aligned, galigned, _ = _run(c, dev, dt, kind)
    v, grad, _ = _run(c, dev, dt, kind, off=1)
    assert np.array_equal(v.view(np.uint32), aligned.view(np.uint32)) and torch.equal(grad, galigned)
    anc, ro, do, cbox, pos = _inputs(c, dev, dt, off=1)
    B, A, L = c['B'], c['A'], len(c['lvl_off']) - 1
    gbuf = torch.zeros(ro.numel() + 16, dtype=dt, device=dev)
    g = gbuf[1:1 + ro.numel()].view(ro.shape)
    out = torch.empty(L + 1, dtype=torch.float32, device=dev)
    ws = ops.workspace(_abi.query('rod_box_iou_loss_workspace', B, A), dev)
    _abi.call('rod_box_iou_loss', anc, ro, do, cbox, pos, np.ascontiguousarray(c['lvl_off'], dtype=np.int32), L,
              br.KINDS[kind], W, SC, out, g, ws, B, A, ops.dtcode(ro), ops.stream())
    assert torch.equal(g, galigned) and np.array_equal(out.cpu().numpy().view(np.uint32), aligned.view(np.uint32))
    assert not gbuf[:1].any() and not gbuf[1 + ro.numel():].any()
    # the fp32 tables off alignment (anchors, cbox) take the scalar path as well
    anc1, cbox1 = _offset_view(anc, 1), _offset_view(cbox, 1)
    with torch.no_grad():
        vec, _ = ops.box_iou_loss(anc1, _dev(c['ro'], dev, dt), _dev(c['do'], dev, dt), cbox1, pos, c['lvl_off'],
                                  kind, W, SC)
    assert np.array_equal(vec.cpu().numpy().view(np.uint32), aligned.view(np.uint32))


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_gradient_plumbing(dev, dt):
    from rod import _abi, ops
    c = br.case('base', dt == torch.bfloat16)
    v, g_do, none = _run(c, dev, dt, 'ciou')
    assert none is None
    v2, g_do2, g_ro2 = _run(c, dev, dt, 'ciou', refine_grad=True)
    assert g_ro2 is not None and torch.equal(g_ro2, g_do2) and torch.equal(g_do2, g_do)       # also: two runs
    assert np.array_equal(v.view(np.uint32), v2.view(np.uint32))
    # only refine_out asks for a gradient: it still gets it
    anc, ro, do, cbox, pos = _inputs(c, dev, dt)
    ro.requires_grad_(True)
    _, tot = ops.box_iou_loss(anc, ro, do, cbox, pos, c['lvl_off'], 'ciou', W, SC)
    tot.backward()
    assert torch.equal(ro.grad, g_do) and do.grad is None
    # the no-grad path passes grad = NULL and returns the same loss bit for bit
    calls, real = [], _abi.call
    _abi.call = lambda name, *a: (calls.append((name, a)), real(name, *a))[1]
    try:
        with torch.no_grad():
            vec, tot = ops.box_iou_loss(anc, ro, do, cbox, pos, c['lvl_off'], 'ciou', W, SC)
    finally:
        _abi.call = real
    assert [n for n, _ in calls] == ['rod_box_iou_loss'] and calls[0][1][11] is None
    assert np.array_equal(vec.cpu().numpy().view(np.uint32), v.view(np.uint32)) and not tot.requires_grad


def test_graph_replay(dev):
    from rod import ops
    names = ('base', 'far', 'inside', 'base')
    eager = {n: _run(br.case(n), dev, torch.float32, 'ciou', refine_grad=True) for n in set(names)}
    c0 = br.case('allpos')
    anc, ro, do, cbox, pos = _inputs(c0, dev, torch.float32)
    ro.requires_grad_(True)
    do.requires_grad_(True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vec, tot = ops.box_iou_loss(anc, ro, do, cbox, pos, c0['lvl_off'], 'ciou', W, SC)
        g_ro, g_do = torch.autograd.grad(tot, (ro, do))
    for n in names[1:]:
        c = br.case(n)
        with torch.no_grad():
            for dst, key in ((anc, 'anc'), (ro, 'ro'), (do, 'do'), (cbox, 'cbox'), (pos, 'pos')):
                dst.copy_(_dev(c[key], dev))
        g.replay()
        torch.cuda.synchronize()
        v, gd, gr = eager[n]
        assert np.array_equal(vec.detach().cpu().numpy().view(np.uint32), v.view(np.uint32))
        assert torch.equal(g_do, gd) and torch.equal(g_ro, gr)


def _recorded(fn):
    from rod import _abi
    calls, real = [], _abi.call
    _abi.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        res = fn()
    finally:
        _abi.call = real
    return res, calls


def test_launch_audit_op(dev):
    """Forward + backward of the op is ONE librod entry (two kernels: the loss pass and the finalize)."""
    c = br.case('base')
    _, calls = _recorded(lambda: _run(c, dev, torch.float32, 'giou', refine_grad=True))
    assert calls == ['rod_box_iou_loss']


def _trainer_inputs(tr, B):
    cat = lambda ts: np.concatenate([t.detach().float().cpu().numpy().reshape(B, -1, 4) for t in ts], 1)   # noqa: E731
    refine_out, det_out, _ = tr.last_out
    dgt = tr.last_targets[1]
    return (tr.table.center_np, cat(refine_out), cat(det_out), dgt.cbox.cpu().numpy(), dgt.flat[1].cpu().numpy(),
            tuple(int(x) for x in tr.table.lvl_off))


@pytest.mark.parametrize('fix_refine', [True, False], ids=['fix_refine', 'train_refine'])
def test_trainer_giou(dev, fix_refine):
    import config
    from rod.data import synthetic_batch
    from rod.trainer import Trainer
    from utils import net_tools
    H, Wd, B = 300, 300, 2
    kw = dict(dtype=torch.float32, device=dev, train_range=config.train_range.ALL, seed=5, fix_refine=fix_refine)
    batch = synthetic_batch(B, H, Wd, dev, seed=6)
    tr = Trainer((H, Wd), B, loc_loss='giou', loc_loss_weight=1.5, **kw)
    losses, calls = _recorded(lambda: tr.losses(*batch))
    # the refine loss is the one smooth-L1 left: none for the ODM
    assert calls.count('rod_box_iou_loss') == 1 and calls.count('rod_smoothl1_masked') == 1
    a = _trainer_inputs(tr, B)
    ref = br.box_loss(*a, 'giou', 1.5, float(B))
    assert (a[4] != 0).sum() > 0 and ref['total'] > 0
    got = np.concatenate([ref['lvl'], [ref['total']]])
    vec = net_tools.det_clf_loss.last_det_per_layer.cpu().numpy().astype(np.float64)
    assert losses[2].item() == vec[-1]
    el = float((np.abs(vec - got) / (br.M * br.E32_LOSS * np.abs(got) + br.LOSS_FLOOR)).max())
    print('trainer giou fix_refine=%s: d_loss %.6f, worst error / bound %.3f' % (fix_refine, losses[2].item(), el))
    assert el <= 1.0
    tr.step(*batch)
    assert tr.graph_mode() == 'full'
    _, calls = _recorded(lambda: [tr.step_graphed(*batch) for _ in range(3)])
    out = tr.step_graphed(*batch)
    torch.cuda.synchronize()
    assert hasattr(tr, '_graph') and all(np.isfinite(x.item()) for x in out)
    assert calls.count('rod_box_iou_loss') == 1            # captured once, replayed after
    if not fix_refine:
        # the refine net gets its ODM gradient from the box loss pass: three aliases of refine_out
        assert 'rod_det_targets_bwd' in calls              # (the IoU factor of the mining still reaches it)


def test_trainer_default_is_the_parent_path(dev):
    import config
    from rod import ops
    from rod.data import synthetic_batch
    from rod.trainer import Trainer
    H, Wd, B = 300, 300, 2
    kw = dict(dtype=torch.float32, device=dev, train_range=config.train_range.ALL, seed=5)
    batch = synthetic_batch(B, H, Wd, dev, seed=6)
    td, te = Trainer((H, Wd), B, **kw), Trainer((H, Wd), B, loc_loss='smooth_l1', **kw)
    ld, calls = _recorded(lambda: td.losses(*batch))
    le = te.losses(*batch)
    assert 'rod_box_iou_loss' not in calls and calls.count('rod_smoothl1_masked') == 2
    assert all(torch.equal(x, y) for x, y in zip(ld, le))
    det_gt, det_pos, _, _ = td.last_targets[1].flat
    with torch.no_grad():
        pred = ops.levels_concat([t.detach() for t in td.last_out[1]], 4)
        _, tot = ops.smooth_l1_masked(pred, det_gt, det_pos, td.table.lvl_off, float(B))
    assert torch.equal(tot, ld[2].detach())
