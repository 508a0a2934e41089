"""Host side of the mosaic augmentation (no GPU): the draws of TrainAugmenter, the fixed-shape box
rule, the numpy box reference on hand-computed cases, the argument guards of rod_mosaic_images /
rod_mosaic_boxes, the host wrapper's table checks, the roofline row and the CLI flags."""
import numpy as np
import pytest
import torch

from mosaic_ref import f32, mosaic_boxes, tile_rects
from rod import _abi, dataio, ops
from rod.data import synthetic_boxes
from utils.data_pileline_tools import TrainAugmenter

HW = (96, 160)


def _batch(B, seed=0, raw=(120, 200)):
    corner, labels, n = synthetic_boxes(B, seed=seed)
    return np.tile(np.array(raw, np.int32), (B, 1)), corner, labels, n


# ------------------------------------------------------------------ the draws
def test_mosaic_off_draws_what_the_default_augmenter_draws():
    """mosaic_prob = 0: sample() is today's sequence, and sample_mosaic() is that sequence as tile 0
    of one-tile images, over several batches."""
    a, b, c = TrainAugmenter(HW, seed=5), TrainAugmenter(HW, seed=5, mosaic_prob=0.0), TrainAugmenter(HW, seed=5)
    for k in range(4):
        hw, corner, _, n = _batch(4, seed=k)
        want = a.sample(hw, corner, n)
        for x, y in zip(want, b.sample(hw, corner, n)):
            np.testing.assert_array_equal(x, y)
        tile_src, crop, ref, mode, colour, center = c.sample_mosaic(hw, corner, n)
        for x, y in zip(want, (crop[:, 0], ref[:, 0], mode[:, 0], colour[:, 0])):
            np.testing.assert_array_equal(x, y)
        assert (center == HW).all() and (tile_src[:, 0] == np.arange(4)).all()


def test_mosaic_on_keeps_the_base_sequence_of_tile_0():
    a = TrainAugmenter(HW, seed=7)
    m = TrainAugmenter(HW, seed=7, mosaic_prob=1.0)
    for k in range(4):
        hw, corner, _, n = _batch(5, seed=10 + k)
        want = a.sample(hw, corner, n)
        tile_src, crop, ref, mode, colour, center = m.sample_mosaic(hw, corner, n)
        for x, y in zip(want, (crop[:, 0], ref[:, 0], mode[:, 0], colour[:, 0])):
            np.testing.assert_array_equal(x, y)
        assert crop.shape == (5, 4, 4) and ref.shape == (5, 4, 4) and mode.shape == (5, 4, 2)
        assert colour.shape == (5, 4, 3) and colour.dtype == np.float32 and center.shape == (5, 2)


def test_draws_are_deterministic_per_seed():
    hw, corner, _, n = _batch(6, seed=1)
    one = TrainAugmenter(HW, seed=3, mosaic_prob=0.5).sample_mosaic(hw, corner, n)
    two = TrainAugmenter(HW, seed=3, mosaic_prob=0.5).sample_mosaic(hw, corner, n)
    other = TrainAugmenter(HW, seed=4, mosaic_prob=0.5).sample_mosaic(hw, corner, n)
    for x, y in zip(one, two):
        np.testing.assert_array_equal(x, y)
    assert any(not np.array_equal(x, y) for x, y in zip(one, other))


@pytest.mark.parametrize('B', [1, 2, 4, 7])
def test_tile_sources_and_centres(B):
    lo, hi = 0.25, 0.75
    aug = TrainAugmenter(HW, seed=B, mosaic_prob=1.0, mosaic_center=(lo, hi))
    seen = set()
    for k in range(6):
        hw, corner, _, n = _batch(B, seed=20 + k)
        tile_src, crop, ref, mode, colour, center = aug.sample_mosaic(hw, corner, n)
        assert (tile_src[:, 0] == np.arange(B)).all()                      # tile 0 is always b
        assert ((tile_src >= 0) & (tile_src < B)).all()
        for b in range(B):
            if B >= 4:                                                      # three others, distinct
                assert len(set(tile_src[b].tolist())) == 4
        for size, c in zip(HW, center.T):
            assert (c >= lo * size).all() and (c <= hi * size).all() and (c >= 1).all() and (c <= size - 1).all()
        seen.update(map(tuple, center.tolist()))
        # every tile's crop lies inside its source and its distort_bbox is that window
        for b in range(B):
            for t in range(4):
                H, W = hw[tile_src[b, t]]
                y, x, h, w = crop[b, t]
                assert 0 <= y and 0 <= x and h > 0 and w > 0 and y + h <= H and x + w <= W
                np.testing.assert_array_equal(ref[b, t], np.array([f32(y) / f32(H), f32(x) / f32(W),
                                                                   f32(y + h) / f32(H), f32(x + w) / f32(W)], f32))
                assert mode[b, t, 0] in (0, 1) and mode[b, t, 1] in (0, 1, 2, 3)
    assert len(seen) > 1


def test_centre_is_clamped_into_the_canvas():
    hw, corner, _, n = _batch(4)
    for rng_, want in (((0.0, 0.0), (1, 1)), ((1.0, 1.0), (HW[0] - 1, HW[1] - 1))):
        center = TrainAugmenter(HW, seed=0, mosaic_prob=1.0, mosaic_center=rng_).sample_mosaic(hw, corner, n)[5]
        assert (center == want).all()


def test_mosaic_probability_mixes_plain_and_mosaic_images():
    aug = TrainAugmenter(HW, seed=2, mosaic_prob=0.5)
    hw, corner, _, n = _batch(64, seed=3)
    center = aug.sample_mosaic(hw, corner, n)[5]
    plain = (center == HW).all(1)
    assert 10 < plain.sum() < 54
    assert ((center[~plain] >= 1) & (center[~plain] <= np.array(HW) - 1)).all()


@pytest.mark.parametrize('kw', [dict(mosaic_prob=-0.1), dict(mosaic_prob=1.5), dict(mosaic_prob=float('nan')),
                                dict(mosaic_center=(0.8, 0.2)), dict(mosaic_center=(-0.1, 0.5)),
                                dict(mosaic_min_px=-1.0)])
def test_bad_settings(kw):
    with pytest.raises(ValueError, match='mosaic'):
        TrainAugmenter(HW, seed=0, **kw)


# ------------------------------------------------------------------ the fixed-shape box rule
def test_gout_rule():
    n = np.array([10, 20, 30, 40], np.int32)
    tile_src = np.array([[0, 1, 2, 3], [1, 0, 2, 3], [2, 0, 1, 3], [3, 0, 1, 2]], np.int32)
    mosaic = np.tile(np.array([40, 80], np.int32), (4, 1))
    plain = np.tile(np.array(HW, np.int32), (4, 1))
    assert dataio.mosaic_gout(n, tile_src, mosaic, HW) == 128                 # 100 boxes: next multiple of 64
    assert dataio.mosaic_gout(n, tile_src, plain, HW) == 64                   # tile 0 alone: at most 40
    assert dataio.mosaic_gout(n // 2, tile_src, mosaic, HW) == 64             # 50 fit gmax
    assert dataio.mosaic_gout(n, tile_src, mosaic, HW, gmax=192) == 192
    assert dataio.mosaic_gout(np.array([16] * 4), tile_src, mosaic, HW) == 64     # exactly 64
    assert dataio.mosaic_gout(np.array([16, 16, 16, 17]), tile_src, mosaic, HW) == 128
    mixed = np.array([[40, 80], HW, HW, HW], np.int32)
    assert dataio.mosaic_gout(np.array([1, 1, 1, 70]), tile_src, mixed, HW) == 128
    assert dataio.mosaic_gout(np.zeros(4, np.int32), tile_src, mosaic, HW) == 64


def test_tile_rectangles():
    assert tile_rects(3, 5, 10, 20) == [(0, 0, 3, 5), (0, 5, 3, 15), (3, 0, 7, 5), (3, 5, 7, 15)]
    np.testing.assert_array_equal(ops.mosaic_tiles([[3, 5], [10, 20]], (10, 20)),
                                  [tile_rects(3, 5, 10, 20), tile_rects(10, 20, 10, 20)])
    assert [r[2] * r[3] for r in tile_rects(10, 20, 10, 20)] == [200, 0, 0, 0]


# ------------------------------------------------------------------ the box reference, by hand
def test_box_reference_by_hand():
    """Canvas 8 x 16, centre (4, 8): every tile is 4 x 8.  All values are dyadic, so the expected
    numbers below are exact."""
    boxes = np.zeros((2, 4, 4), f32)
    labels = np.array([[1, 2, 3, 4], [5, 6, 7, 8]], np.int32)
    boxes[0, 0] = [0.25, 0.25, 0.75, 0.75]      # inside: kept as is by the identity crop
    boxes[0, 1] = [0.5, 0.5, 0.5, 0.75]         # zero height: score 0, dropped
    boxes[1, 0] = [0.0, 0.0, 0.5, 0.5]
    boxes[1, 1] = [0.25, 0.5, 0.75, 1.5]        # straddles the right edge: half inside
    n = np.array([2, 2], np.int32)
    tile_src = np.array([0, 1, 1, 0], np.int32)
    ref = np.array([[0, 0, 1, 1]] * 4, f32)
    ref[2] = [0, 0, 0.5, 0.5]                   # tile 2 sees the top-left quarter of source 1
    mode = np.array([[0, 0], [1, 0], [0, 0], [0, 0]], np.int32)
    bo, lo, k = mosaic_boxes(boxes, labels, n, tile_src, ref, mode, (4, 8), 8, 16, gout=8, threshold=0.3)
    want = [
        ([0.125, 0.125, 0.375, 0.375], 1),      # tile 0: box * (4, 8) / (8, 16)
        ([0.0, 0.75, 0.25, 1.0], 5),            # tile 1, flipped: x (0.5, 1) -> * 8 + 8 -> / 16
        ([0.125, 0.5, 0.375, 0.75], 6),         # tile 1, flipped and clipped: x (-0.5, 0.5) -> (0, 0.5)
        ([0.5, 0.0, 1.0, 0.5], 5),              # tile 2: [0, 0, 1, 1] of the quarter -> the whole tile
        ([0.625, 0.625, 0.875, 0.875], 1),      # tile 3: box * (4, 8) + (4, 8)
    ]
    # source 1's second box under tile 2's crop: [0.5, 1, 1.5, 3] -> inside 0.5 x 0 -> dropped
    assert k == len(want)
    np.testing.assert_array_equal(bo[:k], np.array([w for w, _ in want], f32))
    assert lo[:k].tolist() == [l for _, l in want] and not bo[k:].any() and not lo[k:].any()

    # the overlap score equal to the threshold is dropped (strict >), a hair above is kept
    assert mosaic_boxes(boxes, labels, n, tile_src, ref, mode, (4, 8), 8, 16, gout=8, threshold=0.5)[2] == 4
    # the size floor: tile 0's box is 2 x 4 tile pixels: min_px 2 keeps it (>=), 2.5 drops it
    assert mosaic_boxes(boxes, labels, n, tile_src, ref, mode, (4, 8), 8, 16, gout=8, min_px=2.0)[2] == 5
    b25 = mosaic_boxes(boxes, labels, n, tile_src, ref, mode, (4, 8), 8, 16, gout=8, min_px=2.5)
    assert b25[2] == 1 and b25[1][0] == 5 and b25[0][0].tolist() == [0.5, 0.0, 1.0, 0.5]
    # truncation in visiting order, tail zero
    b3 = mosaic_boxes(boxes, labels, n, tile_src, ref, mode, (4, 8), 8, 16, gout=3)
    assert b3[2] == 3 and b3[1].tolist() == [1, 5, 6]
    np.testing.assert_array_equal(b3[0], bo[:3])


def test_box_reference_one_tile_is_the_plain_chain():
    from oracle import augment as oa
    rng = np.random.default_rng(0)
    G = 20
    c, s = rng.uniform(0, 1, (1, G, 2)), rng.uniform(0, 0.5, (1, G, 2))
    boxes = np.concatenate([c - s / 2, c + s / 2], -1).astype(f32)
    labels = rng.integers(1, 11, (1, G)).astype(np.int32)
    ref = np.array([[0.1, 0.2, 0.7, 0.9]] * 4, f32)
    for flip in (0, 1):
        mode = np.array([[flip, 0]] * 4, np.int32)
        bo, lo, k = mosaic_boxes(boxes, labels, [G], [0, 9, 9, 9], ref, mode, (33, 47), 33, 47, gout=G)
        rb, rl = oa.process_boxes(boxes[0], labels[0], G, ref[0], flip)
        assert k == len(rb) and 0 < k < G
        np.testing.assert_array_equal(bo[:k], rb)
        np.testing.assert_array_equal(lo[:k], rl)


# ------------------------------------------------------------------ the entries' guards
def test_new_entries_guard_their_arguments():
    """Argument validation returns before any HIP call (no GPU here: a launch would fail otherwise)."""
    assert _abi.lib().rod_abi_version() >= 30
    assert {'rod_mosaic_images', 'rod_mosaic_boxes', 'rod_mosaic_workspace'} <= set(_abi.exported_symbols())
    buf = torch.zeros(64)[:32]       # host memory: only its (64-byte aligned) address is looked at
    assert buf.data_ptr() % 16 == 0

    def images(S=2, B=2, Ho=8, Wo=8, out=buf, dtype=0, **null):
        a = dict(src=buf, src_off=buf, src_hw=buf, tile_src=buf, crop=buf, mode=buf, colour=buf, center=buf,
                 workspace=buf)
        a.update(null)
        _abi.call('rod_mosaic_images', a['src'], a['src_off'], a['src_hw'], a['tile_src'], a['crop'], a['mode'],
                  a['colour'], a['center'], a['workspace'], out, S, B, Ho, Wo, 1, dtype, None)
    for kw in (dict(B=0), dict(S=0), dict(Ho=0), dict(Wo=-1), dict(B=1 << 20)):
        with pytest.raises(RuntimeError, match='rod_mosaic_images: bad shape'):
            images(**kw)
    for name in ('src', 'src_off', 'src_hw', 'tile_src', 'crop', 'mode', 'colour', 'center', 'workspace'):
        with pytest.raises(RuntimeError, match='rod_mosaic_images: null argument'):
            images(**{name: None})
    with pytest.raises(RuntimeError, match='rod_mosaic_images: null argument'):
        images(out=None)
    with pytest.raises(RuntimeError, match='rod_mosaic_images: out must be 16-byte aligned'):
        images(out=buf.data_ptr() + 4)

    def boxes(S=2, B=2, G=8, Gout=8, Ho=8, Wo=8, bo=buf, **null):
        a = dict(boxes=buf[16:], labels=buf[16:], n=buf, tile_src=buf, ref=buf, mode=buf, center=buf, lo=buf, no=buf)
        a.update(null)
        _abi.call('rod_mosaic_boxes', a['boxes'], a['labels'], a['n'], a['tile_src'], a['ref'], a['mode'],
                  a['center'], bo, a['lo'], a['no'], S, B, G, Gout, Ho, Wo, 0.3, 0.0, None)
    for kw in (dict(B=0), dict(S=0), dict(G=0), dict(Gout=0), dict(Ho=0), dict(Wo=0)):
        with pytest.raises(RuntimeError, match='rod_mosaic_boxes: bad shape'):
            boxes(**kw)
    for name in ('boxes', 'labels', 'n', 'tile_src', 'ref', 'mode', 'center', 'lo', 'no'):
        with pytest.raises(RuntimeError, match='rod_mosaic_boxes: null argument'):
            boxes(**{name: None})
    with pytest.raises(RuntimeError, match='rod_mosaic_boxes: null argument'):
        boxes(bo=None)
    with pytest.raises(RuntimeError, match='rod_mosaic_boxes: in-place'):
        boxes(bo=buf[16:])


def test_workspace_query_is_host_only_and_sized_for_4b_tiles():
    q = lambda *a: _abi.query('rod_mosaic_workspace', *a)
    assert q(0, 8, 8) == 0 and q(2, 0, 8) == 0
    for B, Ho, Wo in ((1, 8, 8), (3, 96, 128), (8, 720, 1280)):
        nblk = min(1024, max(1, Ho * Wo // 1024))
        assert q(B, Ho, Wo) == (4 * B * nblk * 24 + 255) // 256 * 256 + 4 * B * 12
        assert q(B, Ho, Wo) >= _abi.query('rod_augment_workspace', 4 * B, Ho, Wo)


def test_wrapper_checks_the_tables_of_non_empty_tiles(monkeypatch):
    calls = []
    monkeypatch.setattr(_abi, 'call', lambda name, *a: calls.append(name) or 0)
    monkeypatch.setattr(_abi, 'query', lambda name, *a: 4096)
    monkeypatch.setattr(ops, 'stream', lambda: 0)
    src = torch.zeros((2, 10, 12, 3), dtype=torch.uint8)
    tile_src = np.array([[0, 1, 1, 0]], np.int32)
    crop = np.tile(np.array([0, 0, 10, 12], np.int32), (1, 4, 1))
    mode, colour = np.zeros((1, 4, 2), np.int32), np.zeros((1, 4, 3), f32)

    def run(tile_src=tile_src, crop=crop, center=(3, 4)):
        return ops.mosaic_images(src, tile_src, crop, mode, colour, [center], (6, 8))
    assert run().shape == (1, 6, 8, 3) and calls == ['rod_mosaic_images']
    for bad in ((0, 4), (3, 0), (7, 4), (3, 9)):
        with pytest.raises(ValueError, match='center'):
            run(center=bad)
    with pytest.raises(ValueError, match='tile_src'):
        run(tile_src=np.array([[0, 2, 1, 0]], np.int32))
    with pytest.raises(ValueError, match='tile_src'):
        run(tile_src=np.array([[0, 1, -1, 0]], np.int32))
    bad_crop = crop.copy()
    bad_crop[0, 3] = [5, 0, 6, 12]
    with pytest.raises(ValueError, match='crop window'):
        run(crop=bad_crop)
    # ... but the rows of empty tiles are not looked at: centre (6, 8) leaves tile 0 alone
    junk_src = np.array([[0, 99, -5, 7]], np.int32)
    assert run(tile_src=junk_src, crop=bad_crop, center=(6, 8)).shape == (1, 6, 8, 3)
    # centre (6, 4): tiles 0 and 1 live, 2 and 3 empty
    assert run(tile_src=np.array([[0, 1, 99, 99]], np.int32), crop=bad_crop, center=(6, 4)).shape == (1, 6, 8, 3)
    with pytest.raises(ValueError, match='tile_src'):
        run(tile_src=junk_src, center=(6, 4))
    boxes = torch.zeros((2, 8, 4))
    with pytest.raises(ValueError, match='tile_src'):
        ops.mosaic_boxes(boxes, torch.zeros((2, 8), dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                         np.array([[0, 2, 1, 0]]), np.zeros((1, 4, 4)), mode, [(3, 4)], (6, 8))
    with pytest.raises(ValueError, match='center'):
        ops.mosaic_boxes(boxes, torch.zeros((2, 8), dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                         tile_src, np.zeros((1, 4, 4)), mode, [(0, 4)], (6, 8))
    bo, lo, no = ops.mosaic_boxes(boxes, torch.zeros((2, 8), dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                                  tile_src, np.zeros((1, 4, 4)), mode, [(3, 4)], (6, 8), gout=24)
    assert bo.shape == (1, 24, 4) and lo.shape == (1, 24) and no.shape == (1,)


def test_roofline_row_has_the_bytes_of_the_plain_pass():
    from rod import roofline
    B, Ho, Wo = 8, 720, 1280
    for dt, es in ((0, 4), (1, 2)):
        plain = roofline.cost('rod_augment_images', (0,) * 8 + (B, Ho, Wo, 1, dt, 0))
        mosaic = roofline.cost('rod_mosaic_images', (0,) * 10 + (B, B, Ho, Wo, 1, dt, 0))
        assert mosaic == plain == ((es + 1) * B * Ho * Wo * 3, 0)


# ------------------------------------------------------------------ the sources and the command line
def test_sources_take_the_settings():
    src = dataio.AugmentedSource(2, HW, torch.device('cpu'), torch.float32, seed=1, n_distinct=1, raw_hw=(20, 30),
                                 mosaic_prob=1.0, mosaic_center=(0.4, 0.6), mosaic_min_px=3.0, mosaic_stop_step=2)
    assert src.mosaic.on and src.aug.mosaic_center == (0.4, 0.6) and src.aug.mosaic_min_px == 3.0
    hw, corner, _, n = _batch(2)
    assert (src.mosaic.draw(hw, corner, n)[5] < HW).all()           # steps 0 and 1: mosaic
    assert (src.mosaic.draw(hw, corner, n)[5] < HW).all()
    assert (src.mosaic.draw(hw, corner, n)[5] == HW).all()          # from step 2 on: plain, same tables
    off = dataio.AugmentedSource(2, HW, torch.device('cpu'), torch.float32, seed=1, n_distinct=1, raw_hw=(20, 30))
    assert not off.mosaic.on
    resumed = dataio.AugmentedSource(2, HW, torch.device('cpu'), torch.float32, seed=1, n_distinct=1,
                                     raw_hw=(20, 30), mosaic_prob=1.0, mosaic_stop_step=2, start_step=5)
    assert (resumed.mosaic.draw(hw, corner, n)[5] == HW).all()
    with pytest.raises(ValueError, match='mosaic_prob'):
        dataio.make_source(None, 2, HW, torch.device('cpu'), synthetic=True, mosaic_prob=0.5)


def test_parser_flags():
    import train
    F = train.parse([])
    assert (F.mosaic_prob, F.mosaic_center, F.mosaic_min_px, F.mosaic_stop_step) == (0.0, (0.25, 0.75), 2.0, 0)
    F = train.parse(['--mosaic_prob=0.5', '--mosaic_center', '0.3,0.7', '--mosaic_min_px=4', '--mosaic_stop_step=90'])
    assert (F.mosaic_prob, F.mosaic_center, F.mosaic_min_px, F.mosaic_stop_step) == (0.5, (0.3, 0.7), 4.0, 90)
    for bad in (['--mosaic_prob=1.5'], ['--mosaic_prob=-0.1'], ['--mosaic_prob=nan'],
                ['--mosaic_center=0.8,0.2'], ['--mosaic_center=0.5'], ['--mosaic_center=a,b'],
                ['--mosaic_center=0.5,1.5'], ['--mosaic_min_px=-1'], ['--mosaic_stop_step=-3'],
                ['--mosaic_prob=0.5', '--augment=False']):
        with pytest.raises(SystemExit):
            train.parse(bad)
