"""Anchor matching and hard NMS at their exact-tie edges, bit-exact against the oracle.

  rod_match_anchors / rod_match_anchors_nn   (csrc/targets.hip)  oracle.targets.refine_groundtruth{,_nn}_flat
  rod_select_topk_nms, both front ends       (csrc/nms.hip)      oracle.post.detected_bboxes
  rod_select_topk_softnms, candidate stage   (csrc/nms.hip)      tests/softnms_ref.py

Both kernels take arbitrary tables, so every edge is built on a few hundred to a few thousand
anchors with dyadic coordinates and scores written directly as float32: an IoU that equals a
threshold, two boxes that tie for an anchor, a score that equals select_threshold and a run of
equal scores across the top_k cut are then the same ties in the kernel and in the reference.

Every comparison is np.testing.assert_array_equal (NaN positions included); there are no
tolerances.  The input builders and references are plain numpy (the *_case functions; read-only
results, computed once); only the test bodies touch the device.  Every case asserts, on the
reference side, the precondition of the edge it is there for, so a case that stops exercising its
edge fails; tests/test_match_oracle_host.py runs all of these preconditions without a GPU.

One decision these cases cannot see: the switch from sorting a candidate list whole to radix
select (n <= 4096).  Both branches are correct for any list of at least top_k entries, so at
n == 4096 either gives the same output; n4096 / n4097 pin each branch on its side of the switch.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import softnms_ref as sr  # noqa: E402
from test_gpu_loss_edges import LVL1, LVL5, LVL8  # noqa: E402,F401

from oracle import post as op  # noqa: E402
from oracle import targets as ot  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
A = 781
HALF = f32(0.5)
HALF_UP = np.nextafter(f32(0.5), f32(1))
HALF_DN = np.nextafter(f32(0.5), f32(0))
# thresholds of the LVL8 cases: 0.5 and the next float above it on different levels of one call
# (the one-anchor first level above, the one-anchor last level at 0.5), level 4 at 0
THR8 = (HALF_UP, HALF, HALF, HALF_UP, f32(0), HALF, HALF_UP, HALF)
UNIT = (0.5, 0.5, 1.0, 1.0)              # the unit anchor (cy, cx, h, w)
HALF_BOX = (0.5, 0.5, 1.0, 0.5)          # 1 x 0.5 inside it: inter 0.5, union 1, IoU == 0.5
UNIT_AT = (0, 1, 3, 6, 7, 50, 134, 135, 200, 262, 300, 519, 600, 775, 776, 779, 780)   # every LVL8 level
FAR = slice(263, 291)                    # anchors of the thr == 0 level moved away: every IoU is 0


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return d


def _dev(x, dev):
    return torch.from_numpy(np.array(x)).to(dev)     # a copy: the case arrays are read-only


# ------------------------------------------------------------------ 1, 2. anchor matching
def _table(seed=41, n=A):
    """Dyadic anchors (multiples of 1/64) in centre form; the corner form is exact."""
    rng = np.random.default_rng(seed)
    q = lambda lo, hi, shape: (rng.integers(lo, hi + 1, shape) / 64.0).astype(f32)
    return np.concatenate([q(8, 56, (n, 2)), q(4, 32, (n, 2))], 1)


def _random_boxes(rng, shape):
    q = lambda lo, hi: (rng.integers(lo, hi + 1, shape + (2,)) / 64.0).astype(f32)
    return np.concatenate([q(8, 56), q(4, 40)], -1)


def _match_inputs(center, lvl_off, thr, gt, lbl, n):
    center = np.asarray(center, f32)
    corner = ot.center_to_corner(center)
    # anc_center and anc_corner are exactly consistent
    np.testing.assert_array_equal(ot.corner_to_center(corner), center)
    assert (corner * 128 == np.round(corner * 128)).all()
    gt = np.asarray(gt, f32)
    assert len(thr) == len(lvl_off) - 1 and lvl_off[-1] == center.shape[0]
    return dict(anc_center=center, anc_corner=corner, lvl_off=tuple(lvl_off), thr=tuple(f32(t) for t in thr), gt=gt,
                lbl=np.asarray(lbl, np.int32).reshape(gt.shape[:2]), n=np.asarray(n, np.int32))


def match_ref(c, nn=False):
    """(off [B,A,4], cbox [B,A,4], lbl [B,A], pos [B,A]) of the flat oracle, image by image
    over the first n[b] boxes."""
    fn = ot.refine_groundtruth_nn_flat if nn else ot.refine_groundtruth_flat
    per = [fn(c['anc_corner'], c['anc_center'], c['lvl_off'], c['thr'], c['gt'][b, :c['n'][b]], c['lbl'][b, :c['n'][b]])
           for b in range(len(c['n']))]
    return tuple(np.stack(x) for x in zip(*per))


def _jac(c, b):
    """[n, A] IoU of image b's boxes with every anchor, as the oracle computes it."""
    return np.stack([ot.jaccard(c['anc_corner'], ot.center_to_corner(g)) for g in c['gt'][b, :c['n'][b]]], 0)


def _dist(c, b):
    """[n, A] NEAREST_NEIGHBOR distance, as the oracle computes it."""
    with np.errstate(all='ignore'):
        sq = np.stack([ot.encode_flat(c['anc_center'], g) for g in c['gt'][b, :c['n'][b]]], 0) ** 2
        return ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + sq[..., 3]


def _level_mask(lvl_off, pick):
    m = np.zeros(lvl_off[-1], bool)
    for l in pick:
        m[lvl_off[l]:lvl_off[l + 1]] = True
    return m


def _lvl8_table():
    center = _table()
    center[list(UNIT_AT)] = UNIT
    center[FAR, 0] += f32(4)
    return center


MATCH_CASES = ['thr_eq', 'ties', 'counts', 'A1', 'A257', 'G1', 'G300', 'poison']
NN_CASES = ['ties', 'counts', 'poison', 'A1']
NEG_INF = f32(-np.inf)


@functools.lru_cache(None)
def match_case(name, nn=False):
    """(inputs, reference) of one matching case, JACCARD_BIGGER or (nn) NEAREST_NEIGHBOR; the
    preconditions of the case are asserted on the reference.  Read-only."""
    rng = np.random.default_rng(53)
    if name == 'thr_eq':
        # the half box is box 1; boxes 0 and 2 are small (IoU 1/32 with the unit anchor)
        gt = [[(0.25, 0.25, 0.125, 0.25), HALF_BOX, (0.75, 0.75, 0.25, 0.125)]]
        c = _match_inputs(_lvl8_table(), LVL8, THR8, gt, [[3, 5, 7]], [3])
    elif name == 'ties':
        # 80 anchors of the 513-anchor level centred at (0.5, 0.5): boxes 1, 3 are mirror images
        # about that centre and 5 is a duplicate of 3; 2 and 4 are exact duplicates elsewhere
        center = _table()
        center[300:380, :2] = 0.5
        center[300:380, 2:] = (rng.integers(8, 33, (80, 2)) / 64.0).astype(f32)
        gt = [[(0.125, 0.875, 0.125, 0.125), (0.4375, 0.5, 0.25, 0.25), (0.25, 0.25, 0.25, 0.25),
               (0.5625, 0.5, 0.25, 0.25), (0.25, 0.25, 0.25, 0.25), (0.5625, 0.5, 0.25, 0.25)]]
        c = _match_inputs(center, LVL5, (0.125,) * 5, gt, [[1, 2, 3, 4, 5, 6]], [6])
    elif name == 'counts':
        # n = (0, 1, G, 3): the slots g >= n hold NaN boxes and label -1
        n = (0, 1, 7, 3)
        gt, lbl = _random_boxes(rng, (4, 7)), rng.integers(1, 11, (4, 7))
        for b in range(4):
            gt[b, n[b]:] = np.nan
            lbl[b, n[b]:] = -1
        c = _match_inputs(_lvl8_table(), LVL8, THR8, gt, lbl, n)
    elif name == 'A1':
        c = _match_inputs([UNIT], (0, 1), (HALF,), [[HALF_BOX]], [[9]], [1])
    elif name == 'A257':       # one full block plus one anchor, which is a level of its own
        gt, center = _random_boxes(rng, (2, 7)), _table()[:257]
        center[256] = gt[0, 2]
        c = _match_inputs(center, (0, 256, 257), (0.25, 0.125), gt, rng.integers(1, 11, (2, 7)), (7, 4))
    elif name == 'G1':
        c = _match_inputs(_table(), LVL5, (0.25,) * 5, _random_boxes(rng, (2, 1)), [[4], [8]], (1, 1))
    elif name == 'G300':       # more boxes than the 256 threads that stage them
        c = _match_inputs(_table(), LVL5, (0.25,) * 5, _random_boxes(rng, (2, 300)), rng.integers(1, 11, (2, 300)),
                          (300, 257))
    else:
        assert name == 'poison'
        zh1, zh2 = (0.25, 0.25, 0.0, 0.25), (0.75, 0.5, 0.0, 0.125)
        box, zw, pad = (0.5, 0.5, 0.5, 0.5), (0.5, 0.75, 0.25, 0.0), (0.0, 0.0, 0.0, 0.0)
        gt = [[zh1, box, zh2],                     # two zero-height boxes: P = 2 on channel 2
              [zh1, zw, box],                      # one zero-height, one zero-width
              [(0.5, 0.5, 0.0, 0.5), pad, pad],    # n = 1: the only box has h == 0
              [zh1, zh2, pad]]                     # nothing but two zero-height boxes
        c = _match_inputs(_lvl8_table(), LVL8, THR8, gt, [[2, 4, 6], [3, 5, 7], [9, 0, 0], [8, 1, 0]], (3, 3, 1, 2))
    assert np.isfinite(c['gt'][..., :2][np.arange(c['gt'].shape[1])[None] < c['n'][:, None]]).all()
    ref = match_ref(c, nn)
    off, cbox, lbl, pos = ref
    zero_lvl = _level_mask(c['lvl_off'], [l for l, t in enumerate(c['thr']) if t == 0])
    unit = np.zeros(c['anc_center'].shape[0], bool)
    if len(c['lvl_off']) == 9:
        unit[list(UNIT_AT)] = True
    # ---- preconditions
    if nn:
        assert (pos[c['n'] > 0] == 1).all()
    if name == 'thr_eq':
        jac = _jac(c, 0)
        at_half = _level_mask(LVL8, [l for l, t in enumerate(THR8) if t == HALF])
        above = _level_mask(LVL8, [l for l, t in enumerate(THR8) if t == HALF_UP])
        assert (jac.max(0)[unit] == HALF).all() and (jac.argmax(0)[unit] == 1).all()
        for l in range(8):         # every level holds an anchor at the equality
            assert unit[LVL8[l]:LVL8[l + 1]].any()
        assert pos[0, 0] == 0 and pos[0, 780] == 1      # the one-anchor levels
        assert (unit & at_half).sum() >= 5 and (unit & above).sum() >= 5
        assert (pos[0, unit & at_half] == 1).all() and (lbl[0, unit & at_half] == 5).all()
        assert (pos[0, unit & above] == 0).all() and not off[0, unit & above].any()
        # thr == 0: everything is positive, an anchor whose IoUs are all 0 takes box 0
        assert (pos[0, zero_lvl] == 1).all() and (jac[:, FAR] == 0).all()
        assert (lbl[0, FAR] == 3).all() and (cbox[0, FAR] == c['gt'][0, 0]).all()
        assert (pos[0] == 0).sum() > 100
    if name == 'ties' and not nn:
        jac = _jac(c, 0)
        mx = jac.max(0)
        tied = ((jac == mx).sum(0) >= 2) & (mx > 0)
        first, last = jac.argmax(0), 5 - jac[::-1].argmax(0)
        assert tied.sum() >= 50 and (tied & (pos[0] == 1)).sum() >= 50
        assert (first[tied] == 1).sum() >= 50 and (first[tied] == 2).sum() >= 10    # mirror images, duplicates
        assert ((jac == mx).sum(0) == 3).sum() >= 50                                # 1, 3 and 5 tie
        assert (last[tied] != first[tied]).all()
        sel = tied & (pos[0] == 1)
        assert (lbl[0, sel] == c['lbl'][0][first[sel]]).all() and (lbl[0, sel] != c['lbl'][0][last[sel]]).all()
        assert (cbox[0, sel] == c['gt'][0][first[sel]]).all()
    if name == 'ties' and nn:
        d = _dist(c, 0)
        mn = d.min(0)
        tied = (d == mn).sum(0) >= 2
        first, last = d.argmin(0), 5 - d[::-1].argmin(0)
        assert np.isfinite(d).all() and tied.sum() >= 50 and len(set(first[tied])) >= 2
        assert (lbl[0, tied] == c['lbl'][0][first[tied]]).all() and (last[tied] != first[tied]).all()
    if name == 'counts':
        assert c['n'].tolist() == [0, 1, 7, 3] and c['gt'].shape[1] == 7
        assert all(not x[0].any() for x in ref)                   # n == 0: all-zero outputs
        assert all(np.isnan(c['gt'][b, c['n'][b]:]).all() and (c['lbl'][b, c['n'][b]:] == -1).all() for b in range(4))
        assert all(pos[b].sum() > 50 for b in (1, 2, 3)) and np.isfinite(off).all()
        assert (lbl[1][pos[1] == 1] == c['lbl'][1, 0]).all() and (lbl >= 0).all()
        assert len(set(lbl[2][pos[2] == 1])) >= 3
    if name == 'A1':
        assert pos.tolist() == [[1]] and lbl.tolist() == [[9]] and off.shape == (1, 1, 4)
        assert nn or _jac(c, 0)[0, 0] == HALF
    if name in ('A257', 'G1', 'G300'):
        assert all(20 < pos[b].sum() for b in range(2)) and (pos == 0).sum() > 20
    if name == 'A257':
        assert pos[0, 256] == 1 and lbl[0, 256] == c['lbl'][0, 2]
    if name == 'G300':         # boxes past the first staging pass win anchors
        assert (_jac(c, 0).argmax(0)[pos[0] == 1] >= 256).sum() >= 10 and (lbl[1][pos[1] == 1] > 0).all()
    if name == 'poison':
        assert np.isfinite(cbox).all()
        own = lambda b: (pos[b] == 1) & (lbl[b] == c['lbl'][b, 0])        # matched to box 0, the poisoned one
        if not nn:
            # image 0, P == 2: NaN also where the anchor's own box is one of the poisoned
            assert np.isnan(off[0, :, 2]).all() and (own(0) & zero_lvl).sum() >= 20
            assert np.isfinite(off[0][..., (0, 1, 3)]).all()
            # image 1: -inf survives on channel 2 where box 0 is matched, NaN on channel 3
            assert np.isnan(off[1, :, 3]).all() and (own(1) & zero_lvl).sum() >= 20
            assert (off[1, own(1), 2] == NEG_INF).all() and np.isnan(off[1, ~own(1), 2]).all()
            # image 2: the single h == 0 box is matched throughout the thr == 0 level and nowhere else
            assert (pos[2] == 1).tolist() == zero_lvl.tolist()
            assert (off[2, zero_lvl, 2] == NEG_INF).all() and np.isnan(off[2, ~zero_lvl, 2]).all()
            assert (own(3) & zero_lvl).sum() >= 20 and np.isnan(off[3, :, 2]).all()
        else:
            d = [_dist(c, b) for b in range(4)]
            assert not any(np.isnan(x).any() for x in d)
            assert np.isnan(off[0, :, 2]).all() and (lbl[0] == 4).all()           # the finite box wins
            assert np.isnan(off[1][..., 2:]).all() and (lbl[1] == 7).all()
            assert np.isinf(d[2]).all() and (off[2, :, 2] == NEG_INF).all() and (lbl[2] == 9).all()   # d = inf, matched
            assert np.isinf(d[3]).all() and np.isnan(off[3, :, 2]).all() and (lbl[3] == 8).all()      # first of two inf
            assert np.isfinite(off[2][..., (0, 1, 3)]).all()
    return _frozen(c), ref


def _run_match(dev, c, nn):
    from rod import ops
    got = ops.match_anchors(_dev(c['anc_corner'], dev), _dev(c['anc_center'], dev), c['lvl_off'], c['thr'],
                            _dev(c['gt'], dev), _dev(c['lbl'], dev), _dev(c['n'], dev), nearest=nn)
    return [g.cpu().numpy() for g in got]


def _check_match(dev, name, nn):
    c, ref = match_case(name, nn)
    got = _run_match(dev, c, nn)
    for g, r, what in zip(got, ref, ('off', 'cbox', 'lbl', 'pos')):
        assert g.dtype == r.dtype and g.shape == r.shape
        np.testing.assert_array_equal(g, r, err_msg=what)       # NaN positions included
    if name == 'counts':       # the padded slots are never read: zeros there give the same output
        z = dict(c, gt=np.nan_to_num(c['gt'], nan=0.0), lbl=np.maximum(c['lbl'], 0))
        assert not np.isnan(z['gt']).any() and np.isnan(c['gt']).any()
        for g, g0, what in zip(got, _run_match(dev, z, nn), ('off', 'cbox', 'lbl', 'pos')):
            np.testing.assert_array_equal(g, g0, err_msg=what + ' (zero padding)')


@pytest.mark.parametrize('name', MATCH_CASES)
def test_match_anchors_edges(dev, name):
    _check_match(dev, name, False)


@pytest.mark.parametrize('name', NN_CASES)
def test_match_anchors_nn_edges(dev, name):
    _check_match(dev, name, True)


# ------------------------------------------------------------------ 3. select + top_k + hard NMS
POOL = np.array([[0, j / 8, 1 / 8, (j + 1) / 8] for j in range(8)], f32)    # 8 disjoint boxes, y in [0, 1/8]


def _cells(n, g=128, row0=16):
    """n pairwise disjoint (IoU exactly 0) cells of a g x g grid, below the POOL band."""
    i = np.arange(n)
    r, col = row0 + i // g, i % g
    assert r.max() < g
    return (np.stack([r, col, r + 1, col + 1], 1) / g).astype(f32)


def _blank(B, A_, K):
    """No score, every anchor a cell of its own: nothing is selected, nothing overlaps."""
    return np.zeros((B, A_, K), f32), np.broadcast_to(_cells(A_), (B, A_, 4)).copy()


def _nms(probs, boxes, sel, nms, top_k, keep, **extra):
    assert probs.dtype == f32 and boxes.dtype == f32 and (probs >= 0).all() and (probs <= 1).all()
    return dict(probs=probs, boxes=boxes, sel=float(f32(sel)), nms=float(f32(nms)), top_k=top_k, keep=keep, **extra)


def _tie_cut(A_, top_k, fill, seed):
    """Class 1: top_k - 8 distinct scores above 0.5 on boxes of the POOL (they suppress each
    other down to 8), then a run of 16 anchors at exactly 0.5, scattered over the index range,
    each in a cell of its own: the 8 of lower index are inside top_k and survive.  fill: how
    many further anchors hold a score in [0.125, 0.5) (candidates past the cut)."""
    rng = np.random.default_rng(seed)
    n_above, run = top_k - 8, 16
    probs, boxes = _blank(1, A_, 3)
    perm = rng.permutation(A_)
    above, tied, rest = perm[:n_above], np.sort(perm[n_above:n_above + run]), perm[n_above + run:][:fill]
    probs[0, above, 1] = 0.5 + (1 + rng.permutation(n_above)) * 2.0 ** -12
    probs[0, tied, 1] = 0.5
    probs[0, rest, 1] = 0.125 + rng.permutation(len(rest)) * 2.0 ** -14
    boxes[0, above] = POOL[rng.permutation(n_above) % 8]
    few = rng.choice(A_, 30, replace=False)
    probs[0, few, 2] = 0.25 + (1 + rng.permutation(30)) * 2.0 ** -6
    return _nms(probs, boxes, 0.125, 0.5, top_k, 64, tied=tied)


def cut_sets(c):
    """(admitted, rejected) anchors of a tie-cut case's run; asserts that the cut falls inside it."""
    s = c['probs'][0, :, 1]
    order = np.argsort(-s, kind='stable')
    k, tied = c['top_k'], c['tied']
    assert s[order[k - 1]] == s[order[k]] == HALF and (s[tied] == HALF).all() and (s == HALF).sum() == len(tied) >= 8
    take = k - int((s > HALF).sum())
    assert 0 < take < len(tied) and tied[-1] - tied[0] > len(s) // 2 and (np.diff(tied) > 0).all()
    assert set(order[:k]) & set(tied) == set(tied[:take])
    return tied[:take], tied[take:]


NMS_CASES = ['select_eq', 'nms_half', 'nms_below_half', 'nms_one', 'chains', 'degenerate', 'cut64', 'cut400_radix',
             'cut1024', 'n4096', 'n4097', 'A2049', 'A1', 'A5', 'B3_counts', 'keep_cap', 'keep_pad', 'keep1', 'topk1',
             'K2', 'K33', 'K34', 'sel0']
SOFT_CASES = ['select_eq', 'cut64', 'cut400_radix', 'cut1024', 'n4096', 'n4097']


@functools.lru_cache(None)
def nms_case(name):
    """(inputs, detected_bboxes reference) of one NMS case; the preconditions of the case are
    asserted on the reference.  Read-only."""
    rng = np.random.default_rng(67)
    if name == 'select_eq':
        probs, boxes = _blank(1, 300, 3)
        thr = f32(0.3)
        below = np.nextafter(thr, f32(0))
        for cls in (1, 2):
            pick = rng.permutation(300)[:60]
            probs[0, pick[:20], cls] = thr
            probs[0, pick[20:40], cls] = below
            probs[0, pick[40:], cls] = thr + (1 + np.arange(20)) * f32(2.0 ** -6)
        c = _nms(probs, boxes, thr, 0.5, 100, 100)
    elif name in ('nms_half', 'nms_below_half', 'nms_one'):
        # pairs (X, the half of X): IoU exactly 0.5; pairs of duplicates: IoU exactly 1
        probs, boxes = _blank(1, 300, 2)
        pick = rng.permutation(300)[:40].reshape(4, 10)
        for j in range(10):
            y, x, s = (j // 4) / 4.0, (j % 4) / 4.0, 2.0 ** -(3 + j % 3)
            boxes[0, pick[0, j]] = (y, x, y + s, x + s)
            boxes[0, pick[1, j]] = (y, x, y + s, x + s / 2)
            boxes[0, pick[2, j]] = boxes[0, pick[3, j]] = (y + s, x, y + 2 * s, x + s / 4)
        probs[0, pick.reshape(-1), 1] = 0.5 + rng.permutation(40) * f32(2.0 ** -7)
        c = _nms(probs, boxes, 0.25, {'nms_half': HALF, 'nms_below_half': HALF_DN, 'nms_one': 1.0}[name], 100, 100,
                 pick=pick)
    elif name == 'chains':
        # X = [0, 4], Y = [1, 5], Z = [2, 6] along x: IoU(X,Y) = IoU(Y,Z) = 3/5, IoU(X,Z) = 2/6
        probs, boxes = _blank(1, 300, 2)
        pick = rng.permutation(300)[:36].reshape(3, 12)
        for j in range(12):
            for i in range(3):
                boxes[0, pick[i, j]] = (j / 16, (8 * (j % 5) + i) / 64, (j + 1) / 16, (8 * (j % 5) + i + 4) / 64)
                probs[0, pick[i, j], 1] = 0.75 - i * 0.125 + j * 2.0 ** -8
        c = _nms(probs, boxes, 0.25, 0.5, 100, 100, pick=pick)
    elif name == 'degenerate':
        probs, boxes = _blank(1, 300, 2)
        p = rng.permutation(300)[:8]
        boxes[0, p[0]] = (0.5, 0.25, 0.5, 0.75)       # zero height, top score, inside p[1]
        boxes[0, p[1]] = (0.25, 0.25, 0.75, 0.75)
        boxes[0, p[2]] = (0.3125, 0.5, 0.6875, 0.5)         # zero width, below p[1] in score
        boxes[0, p[3]] = (0.25, 0.0, 0.125, 0.125)    # ymin > ymax
        boxes[0, p[4]] = (0.125, 0.0, 0.25, 0.125)    # the same box, upright, lower score: suppressed
        boxes[0, p[5]] = (1.0, 1.0, 0.875, 0.875)     # both axes inverted
        boxes[0, p[6]] = (0.875, 0.875, 1.0, 0.9375)  # half of it: IoU 0.5, kept at 0.5
        boxes[0, p[7]] = (0.25, 0.25, 0.25, 0.25)     # a point
        probs[0, p, 1] = np.array([0.96875, 0.875, 0.75, 0.9375, 0.5, 0.90625, 0.4375, 0.984375], f32)
        c = _nms(probs, boxes, 0.25, 0.5, 100, 100, pick=p)
    elif name == 'cut64':
        c = _tie_cut(700, 64, 100, 3)
    elif name == 'cut400_radix':
        c = _tie_cut(4300, 400, 4300, 4)
    elif name == 'cut1024':
        c = _tie_cut(1500, 1024, 1500, 5)
    elif name in ('n4096', 'n4097'):
        n = int(name[1:])
        probs, boxes = _blank(1, 4300, 3)
        pick = rng.permutation(4300)[:n]
        probs[0, pick, 1] = 0.125 + rng.permutation(n) * 2.0 ** -13
        dup = pick[rng.random(n) < 0.9]
        boxes[0, dup] = POOL[rng.integers(0, 8, len(dup))]
        c = _nms(probs, boxes, 0.125, 0.5, 400, 64)
    elif name == 'A2049':      # the compaction tile plus one: the last anchor holds the top score
        probs, boxes = _blank(1, 2049, 3)
        pick = rng.permutation(2048)[:150]
        probs[0, pick, 1] = 0.25 + rng.permutation(150) * 2.0 ** -9
        probs[0, 2048, 1:] = (0.9375, 0.5)
        probs[0, 2047, 2] = 0.75
        c = _nms(probs, boxes, 0.25, 0.5, 100, 100)
    elif name == 'A1':
        c = _nms(np.array([[[0.0625, 0.9375]]], f32), np.array([[[0.25, 0.25, 0.5, 0.75]]], f32), 0.25, 0.5, 400, 200)
    elif name == 'A5':
        probs, boxes = _blank(1, 5, 3)
        probs[0, :, 1] = (0.5, 0.0, 0.75, 0.125, 0.5)
        probs[0, :, 2] = 0.0625
        c = _nms(probs, boxes, 0.25, 0.5, 400, 200)
    elif name == 'B3_counts':
        counts = ((0, 5, 300), (700, 1, 17), (64, 0, 129))
        probs, boxes = _blank(3, 700, 4)
        for b in range(3):
            dup = rng.random(700) < 0.7
            boxes[b, dup] = POOL[rng.integers(0, 8, int(dup.sum()))]
            for k, n in enumerate(counts[b]):
                probs[b, rng.permutation(700)[:n], k + 1] = 0.25 + (1 + rng.permutation(n)) * 2.0 ** -11
        c = _nms(probs, boxes, 0.25, 0.5, 64, 32, counts=counts)
    elif name in ('keep_cap', 'keep_pad', 'keep1', 'topk1'):
        probs, boxes = _blank(1, 300, 3)
        for cls in (1, 2):
            pick = rng.permutation(300)[:50]
            probs[0, pick, cls] = 0.25 + (1 + rng.permutation(50)) * 2.0 ** -7
        dup = rng.permutation(300)[:100]
        boxes[0, dup] = POOL[rng.integers(0, 8, 100)]
        top_k, keep = {'keep_cap': (100, 10), 'keep_pad': (100, 200), 'keep1': (100, 1), 'topk1': (1, 5)}[name]
        c = _nms(probs, boxes, 0.25, 0.5, top_k, keep)
    elif name in ('K2', 'K33', 'K34'):
        K = int(name[1:])
        probs, boxes = _blank(1, 300, K)
        on = rng.random((1, 300, K)) < 0.1
        probs[on] = (0.25 + rng.integers(0, 2048, int(on.sum())) / 4096.0).astype(f32)
        dup = rng.permutation(300)[:150]
        boxes[0, dup] = POOL[rng.integers(0, 8, 150)]
        c = _nms(probs, boxes, 0.25, 0.5, 64, 16)
    else:
        assert name == 'sel0'  # every anchor passes, exact-zero scores included, boxes unmasked
        probs, boxes = _blank(1, 300, 3)
        pick = rng.permutation(300)[:40]
        probs[0, pick, 1] = 0.125 + rng.permutation(40) * 2.0 ** -7
        boxes[0, ::3] = POOL[rng.integers(0, 8, 100)]
        c = _nms(probs, boxes, 0.0, 0.5, 100, 100)
    ref = op.detected_bboxes(c['probs'], c['boxes'], c['sel'], c['nms'], c['top_k'], c['keep'])
    s_ref, b_ref, kept = ref
    B, A_, K = c['probs'].shape
    # the survivors that passed the select threshold (the oracle also lists the zeroed entries of top_k)
    kept = {bc: [int(i) for i in v if c['probs'][bc[0], i, bc[1]] >= f32(c['sel'])] for bc, v in kept.items()}
    n_cand = (c['probs'][..., 1:] >= f32(c['sel'])).sum(1)          # [B, K-1]
    iou = lambda i, j: op.tf_nms_iou(c['boxes'][0, i], c['boxes'][0, j])
    # ---- preconditions
    if name == 'select_eq':
        thr, below = f32(c['sel']), np.nextafter(f32(c['sel']), f32(0))
        for cls in (1, 2):
            p = c['probs'][0, :, cls]
            assert (p == thr).sum() == 20 and (p == below).sum() == 20 and below < thr
            assert set(np.flatnonzero(p == thr)) <= set(kept[(0, cls)]) and len(kept[(0, cls)]) == 40
            assert not set(np.flatnonzero(p == below)) & set(kept[(0, cls)])
            assert (s_ref[0, cls - 1] == thr).sum() == 20 and not s_ref[0, cls - 1, 40:].any()
    if name in ('nms_half', 'nms_below_half', 'nms_one'):
        pick, k = c['pick'], set(kept[(0, 1)])
        assert all(iou(pick[0, j], pick[1, j]) == HALF and iou(pick[2, j], pick[3, j]) == 1 for j in range(10))
        assert len(k) == {'nms_half': 30, 'nms_below_half': 20, 'nms_one': 40}[name]
        assert f32(c['nms']) == {'nms_half': HALF, 'nms_below_half': HALF_DN, 'nms_one': f32(1)}[name]
        assert all((pick[0, j] in k) + (pick[1, j] in k) == (2 if name != 'nms_below_half' else 1) for j in range(10))
        assert all((pick[2, j] in k) + (pick[3, j] in k) == (2 if name == 'nms_one' else 1) for j in range(10))
    if name == 'chains':
        pick, k, t = c['pick'], set(kept[(0, 1)]), f32(c['nms'])
        good = [j for j in range(12) if iou(pick[0, j], pick[1, j]) > t and iou(pick[1, j], pick[2, j]) > t
                and 0 < iou(pick[0, j], pick[2, j]) <= t and pick[0, j] in k and pick[1, j] not in k and pick[2, j] in k]
        assert len(good) >= 10 and len(k) == 24
    if name == 'degenerate':
        p, k = c['pick'], kept[(0, 1)]
        assert set(k) == set(p) - {p[4]} and k[0] == p[7] and k[1] == p[0]
        assert iou(p[3], p[4]) == 1 and iou(p[5], p[6]) == HALF and iou(p[0], p[1]) == 0 and iou(p[1], p[2]) == 0
        assert (b_ref[0, 0, 2] == c['boxes'][0, p[3]]).all() and b_ref[0, 0, 2, 0] > b_ref[0, 0, 2, 2]   # as given
    if name.startswith('cut'):
        admitted, rejected = cut_sets(c)
        k = set(kept[(0, 1)])
        assert set(admitted) <= k and not set(rejected) & k and len(k) == 8 + len(admitted) and len(admitted) == 8
        assert n_cand[0, 0] == {'cut64': 56 + 16 + 100, 'cut400_radix': 4300, 'cut1024': 1500}[name]
        assert c['top_k'] == {'cut64': 64, 'cut400_radix': 400, 'cut1024': 1024}[name]
    if name in ('n4096', 'n4097'):
        assert n_cand[0].tolist() == [int(name[1:]), 0]     # a class with no candidate next to the full one
        assert 16 < len(kept[(0, 1)]) < c['keep'] and not s_ref[0, 1].any()
    if name == 'A2049':
        assert kept[(0, 1)][0] == 2048 and kept[(0, 2)] == [2047, 2048] and len(kept[(0, 1)]) == 100
    if name == 'A1':
        assert kept[(0, 1)] == [0] and s_ref[0, 0, 0] == f32(0.9375) and not s_ref[0, 0, 1:].any()
    if name == 'A5':
        assert kept[(0, 1)] == [2, 0, 4] and s_ref[0, 0, :5].tolist() == [0.75, 0.5, 0.5, 0, 0]
        assert not b_ref[0, 0, 3:].any() and not s_ref[0, 1].any()
    if name == 'B3_counts':
        assert n_cand.tolist() == [list(r) for r in c['counts']]
        assert len(set(len(kept[(b, cls)]) for b in range(3) for cls in (1, 2, 3))) >= 5
    if name == 'keep_cap':     # the cap is reached with survivors left
        more = op.detected_bboxes(c['probs'], c['boxes'], c['sel'], c['nms'], c['top_k'], 200)[2]
        assert all(len(kept[(0, cls)]) == 10 < len(more[(0, cls)]) for cls in (1, 2))
    if name == 'keep_pad':
        assert all(10 < len(kept[(0, cls)]) < 50 for cls in (1, 2)) and not s_ref[0, :, 50:].any()
    if name == 'keep1':
        assert all(kept[(0, cls)] == [int(np.argmax(c['probs'][0, :, cls]))] for cls in (1, 2))
    if name == 'topk1':
        assert all(len(kept[(0, cls)]) == 1 for cls in (1, 2)) and not s_ref[0, :, 1:].any()
    if name in ('K2', 'K33', 'K34'):
        assert s_ref.shape == (1, K - 1, 16) and (n_cand[0] > 10).all() and (s_ref[0, :, 3] > 0).all()
    if name == 'sel0':
        k = kept[(0, 1)]
        zero = [i for i in k if c['probs'][0, i, 1] == 0]
        assert c['sel'] == 0 and n_cand[0].tolist() == [300, 300] and len(zero) >= 10 and len(k) < 100
        assert all(b_ref[0, 0, j].any() for j in range(len(k)))            # a zero score keeps its box
        assert max(zero) < 100 and kept[(0, 2)][0] == 0                    # the lower indices fill top_k
    return _frozen(c), ref


def _nms_args(c, dev):
    return _dev(c['probs'], dev), _dev(c['boxes'], dev), c['sel'], c['top_k'], c['keep'], c['nms']


@pytest.mark.parametrize('compact', [True, False])
@pytest.mark.parametrize('name', NMS_CASES)
def test_select_topk_nms_edges(dev, name, compact):
    """compact=True passes the workspace: the candidate-list front end, except for K = 34 and
    select_threshold = 0, which fall back to the direct kernel (the output is the same)."""
    from rod import ops
    c, (s_ref, b_ref, _) = nms_case(name)
    s, b = ops.select_topk_nms(*_nms_args(c, dev), compact=compact)
    np.testing.assert_array_equal(s.cpu().numpy(), s_ref)
    np.testing.assert_array_equal(b.cpu().numpy(), b_ref)


# ------------------------------------------------------------------ 4. Soft-NMS front end
@functools.lru_cache(None)
def soft_case(name, method):
    """The inputs of nms_case(name) with the softnms_ref reference; what the hard case asserts
    about the candidate selection is asserted on the emitted anchors."""
    c, _ = nms_case(name)
    ref = sr.soft_detected_bboxes(c['probs'], c['boxes'], c['sel'], c['nms'], c['top_k'], c['keep'], method)
    emitted = set(ref[2][(0, 1)][0])
    if name == 'select_eq':
        p = c['probs'][0, :, 1]
        assert set(np.flatnonzero(p == f32(c['sel']))) <= emitted and len(emitted) == 40
    if name.startswith('cut'):
        admitted, rejected = cut_sets(c)
        assert set(admitted) <= emitted and not set(rejected) & emitted
    if name in ('n4096', 'n4097'):
        assert len(emitted) > 16 and ref[2][(0, 2)] == ([], sr.EXHAUSTED)
    return c, ref


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
@pytest.mark.parametrize('name', SOFT_CASES)
def test_select_topk_soft_nms_front_end(dev, name, method):
    from rod import ops
    c, (s_ref, b_ref, _) = soft_case(name, method)
    for compact in (True, False):
        s, b = ops.select_topk_soft_nms(*_nms_args(c, dev), method, compact=compact)
        np.testing.assert_array_equal(s.cpu().numpy(), s_ref, err_msg='compact=%s' % compact)
        np.testing.assert_array_equal(b.cpu().numpy(), b_ref, err_msg='compact=%s' % compact)
