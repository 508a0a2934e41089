"""What tests/test_gpu_match_nms_edges.py rests on, checked without a GPU: the flat-table forms
of the matching oracle equal its per-layer forms bit for bit on the product's 300x300 anchors,
and every case of the GPU file builds, with the precondition of its edge holding on the
reference (the *_case functions assert them)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_match_nms_edges as edges  # noqa: E402

from oracle import anchors as oa  # noqa: E402
from oracle import net as onet  # noqa: E402
from oracle import targets as ot  # noqa: E402

f32 = np.float32
THR6 = (0.5, 0.5, 0.4, 0.3, 0.0, 0.5)


def _anchors(H, W):
    init = oa.init_anchor(6, (H, W))
    chain = oa.feat_sizes((H, W), [s for (_, s, _, _, _) in onet.SPEC])
    return [oa.anchors_one_layer((H, W), chain[t - 1], init[i]) for i, t in enumerate(onet.TAPS)]


def _flat_table(anchors):
    corner = np.concatenate([np.stack(oa.anchor_corners(l), -1).reshape(-1, 4) for l in anchors])
    center = np.concatenate([np.stack(np.broadcast_arrays(*oa.anchor_centers(l)), -1).reshape(-1, 4) for l in anchors])
    off = np.cumsum([0] + [int(np.prod(np.broadcast_shapes(*(np.shape(v) for v in l)))) for l in anchors])
    return corner.astype(f32), center.astype(f32), tuple(int(o) for o in off)


def _random_gt(rng, G, degenerate):
    """One image of boxes as tests/test_gpu_kernels.py draws them (corner form, clipped)."""
    cy, cx = rng.uniform(0.05, 0.95, G), rng.uniform(0.05, 0.95, G)
    h = np.exp(rng.uniform(np.log(0.01), np.log(0.6), G))
    w = np.exp(rng.uniform(np.log(0.01), np.log(0.6), G))
    corner = np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], -1).clip(0, 1).astype(f32)
    if degenerate:
        corner[0, 2] = corner[0, 0]    # zero height
    return ot.corner_to_center(corner), rng.choice([1, 2, 3, 4, 6, 8, 10], size=G).astype(np.int32)


@pytest.mark.parametrize('nn', [False, True])
@pytest.mark.parametrize('G,degenerate', [(24, False), (24, True), (1, False), (1, True), (0, False)])
def test_flat_oracle_equals_layer_oracle(G, degenerate, nn):
    anchors = _anchors(300, 300)
    corner, center, lvl_off = _flat_table(anchors)
    assert lvl_off[-1] == corner.shape[0] == center.shape[0] > 10000 and len(lvl_off) == 7
    cb, lab = _random_gt(np.random.default_rng(7 + G), max(G, 1), degenerate)
    cb, lab = cb[:G], lab[:G]
    if nn:
        flat = ot.refine_groundtruth_nn_flat(corner, center, lvl_off, THR6, cb, lab)
    else:
        flat = ot.refine_groundtruth_flat(corner, center, lvl_off, THR6, cb, lab)
    assert [x.shape for x in flat] == [(lvl_off[-1], 4), (lvl_off[-1], 4), (lvl_off[-1],), (lvl_off[-1],)]
    assert [x.dtype for x in flat] == [f32, f32, np.int32, np.int32]
    if G == 0:
        assert not any(x.any() for x in flat)
        return
    layer = ot.refine_groundtruth_nn(anchors, cb, lab) if nn else ot.refine_groundtruth(anchors, cb, lab, THR6)
    for got, per_layer, k in zip(flat, layer, (4, 4, 1, 1)):
        ref = np.concatenate([x.reshape(-1, k) for x in per_layer])
        np.testing.assert_array_equal(got.reshape(-1, k), ref)     # NaN positions included
    if degenerate:
        assert not np.isfinite(flat[0][:, 2]).any() and (G == 1 or np.isnan(flat[0][:, 2]).any())
    else:
        assert np.isfinite(flat[0]).all()
    assert 0 < flat[3].sum() and (nn or flat[3].sum() < lvl_off[-1])


@pytest.mark.parametrize('name', edges.MATCH_CASES)
def test_match_case_preconditions(name):
    c, ref = edges.match_case(name)
    assert ref[0].shape == c['gt'].shape[:1] + (c['anc_center'].shape[0], 4)


@pytest.mark.parametrize('name', edges.NN_CASES)
def test_match_nn_case_preconditions(name):
    c, ref = edges.match_case(name, True)
    assert ref[3].dtype == np.int32


@pytest.mark.parametrize('name', edges.NMS_CASES)
def test_nms_case_preconditions(name):
    c, (s_ref, b_ref, kept) = edges.nms_case(name)
    B, A, K = c['probs'].shape
    assert s_ref.shape == (B, K - 1, c['keep']) and b_ref.shape == (B, K - 1, c['keep'], 4)
    assert 1 <= c['top_k'] <= 1024 and 1 <= c['keep'] <= 1024


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
@pytest.mark.parametrize('name', edges.SOFT_CASES)
def test_soft_case_preconditions(name, method):
    c, (s_ref, b_ref, info) = edges.soft_case(name, method)
    assert s_ref.shape == (1, 2, c['keep'])
