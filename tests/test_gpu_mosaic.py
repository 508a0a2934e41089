"""Mosaic augmentation on the GPU (rod_mosaic_images / rod_mosaic_boxes, ABI 30).

Bar.  Images: the rectangle of every tile is BIT FOR BIT what rod_augment_images writes for that
tile's source, crop, mode and colour at the tile's size, in fp32 and in normalised bf16 (the
entries share their device functions and the partition of the contrast sums).  Independently,
against the numpy restatement (tests/mosaic_ref.py over oracle/augment.py): exact without colour
ops, within 1e-3 on the 0-255 scale with them (the oracle's contrast mean is an f64 sum in another
order; every other op is float32 per operation in both) — the tolerances of test_gpu_augment.py.
Boxes, labels and counts: bit-exact against tests/mosaic_ref.py."""
import numpy as np
import pytest
import torch

import mosaic_ref as mr
from rod import ops

pytestmark = pytest.mark.gpu

HW = [(37, 53), (64, 48), (5, 9), (120, 200)]      # ragged sources, packed in one buffer
ORDERINGS = [0, 1, 2, 3, -1]


@pytest.fixture(scope='module')
def sources(dev):
    rng = np.random.default_rng(11)
    srcs = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in HW]
    off = np.cumsum([0] + [s.size for s in srcs])[:-1].astype(np.int64)
    flat = torch.from_numpy(np.concatenate([s.reshape(-1) for s in srcs])).to(dev)
    return srcs, flat, np.array(HW, np.int32), off


def _tables(seed, centers, colour=True):
    """Random tile tables for the given centres.  Image 0 uses source 3 for tiles 1 and 2 under
    different flips; the colour orderings cycle through all four and -1."""
    rng = np.random.default_rng(seed)
    B = len(centers)
    tile_src = rng.integers(0, len(HW), (B, 4)).astype(np.int32)
    tile_src[0] = [0, 3, 3, 1]
    crop = np.zeros((B, 4, 4), np.int32)
    mode = np.zeros((B, 4, 2), np.int32)
    col = np.zeros((B, 4, 3), np.float32)
    for b in range(B):
        for t in range(4):
            H, W = HW[tile_src[b, t]]
            h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
            crop[b, t] = [int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w]
            mode[b, t] = [int(rng.integers(0, 2)), ORDERINGS[(4 * b + t) % 5] if colour else -1]
            col[b, t] = [rng.uniform(-0.8, 0.8), rng.uniform(0.5, 1.0), rng.uniform(0.5, 1.0)]
    mode[0, 1, 0], mode[0, 2, 0] = 0, 1
    return tile_src, crop, mode, col, np.array(centers, np.int32)


def _pasted(flat, hw, off, tables, Ho, Wo, **kw):
    """The yardstick: one rod_augment_images call per non-empty tile at the tile's size, pasted."""
    tile_src, crop, mode, col, center = tables
    out = None
    for b in range(len(center)):
        for t, (oy0, ox0, th, tw) in enumerate(mr.tile_rects(int(center[b, 0]), int(center[b, 1]), Ho, Wo)):
            if th == 0 or tw == 0:
                continue
            s = tile_src[b, t]
            tile = ops.augment_images(flat, crop[b, t][None], mode[b, t][None], col[b, t][None], (th, tw),
                                      src_hw=hw[s][None], src_off=off[s][None], **kw)
            if out is None:
                out = torch.full((len(center), Ho, Wo, 3), float('nan'), dtype=tile.dtype, device=tile.device)
            out[b, oy0:oy0 + th, ox0:ox0 + tw] = tile[0]
    return out


def _mosaic(flat, hw, off, tables, Ho, Wo, **kw):
    tile_src, crop, mode, col, center = tables
    return ops.mosaic_images(flat, tile_src, crop, mode, col, center, (Ho, Wo), src_hw=hw, src_off=off, **kw)


def _poison_empty_tiles(tables, Ho, Wo):
    """Out-of-range source indices and crop rows for every empty tile: they must not be read."""
    tile_src, crop, mode, col, center = (a.copy() for a in tables)
    n = 0
    for b in range(len(center)):
        for t, (_, _, th, tw) in enumerate(mr.tile_rects(int(center[b, 0]), int(center[b, 1]), Ho, Wo)):
            if th == 0 or tw == 0:
                tile_src[b, t] = 1 << 20 if t & 1 else -7
                crop[b, t] = [1 << 20, 1 << 20, 1 << 24, 1 << 24]
                mode[b, t] = [1, 3]
                n += 1
    assert n > 0
    return tile_src, crop, mode, col, center


# canvas 33 x 47: 1551 pixels, no multiple of 4 -> the scalar store path; one-block sums.
# canvas 96 x 128: the vector path; centre (64, 96) gives tile 0 6144 pixels -> 6 sum blocks,
# (1, 1) gives tile 3 12065 pixels -> 11, and the other tiles of those images surplus blocks that exit.
CANVAS = {
    (33, 47): [(1, 1), (32, 46), (16, 21), (16, 24), (33, 47), (33, 20), (9, 47)],
    (96, 128): [(64, 96), (1, 1), (95, 127), (50, 63), (96, 128), (40, 64), (96, 30)],
}


@pytest.mark.parametrize('kw', [dict(), dict(dtype=torch.bfloat16, normalize=True)], ids=['fp32', 'bf16norm'])
@pytest.mark.parametrize('Ho,Wo', list(CANVAS))
def test_tiles_equal_the_plain_entry_bit_for_bit(dev, sources, Ho, Wo, kw):
    """Every centre where it can go wrong, in one batch that mixes mosaic and plain images: (1, 1),
    (Ho-1, Wo-1), cx % 4 != 0 (a thread's four pixels straddle two tiles), cx % 4 == 0, (Ho, Wo) and
    centres on one canvas edge (two tiles).  The empty tiles carry out-of-range rows."""
    _, flat, hw, off = sources
    tables = _tables(Ho, CANVAS[(Ho, Wo)])
    assert {0, 1, 2, 3, -1} <= set(tables[2][..., 1].reshape(-1).tolist())
    want = _pasted(flat, hw, off, tables, Ho, Wo, **kw)
    got = _mosaic(flat, hw, off, _poison_empty_tiles(tables, Ho, Wo), Ho, Wo, **kw)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert not torch.isnan(want.float()).any()
    np.testing.assert_array_equal(got.float().cpu().numpy(), want.float().cpu().numpy())


@pytest.mark.parametrize('kw', [dict(), dict(dtype=torch.bfloat16, normalize=True)], ids=['fp32', 'bf16norm'])
def test_one_tile_batch_is_the_plain_batch(dev, sources, kw):
    """center = (Ho, Wo) for every image: one rod_augment_images call over the batch, bit for bit."""
    _, flat, hw, off = sources
    Ho, Wo = 40, 60
    tile_src, crop, mode, col, center = _tables(3, [(Ho, Wo)] * 4)
    tile_src[:, 0] = [2, 0, 3, 1]
    for b in range(4):                       # tile 0's crop must lie in ITS source
        H, W = HW[tile_src[b, 0]]
        crop[b, 0] = [H // 4, W // 5, H - H // 4, W - W // 5]
    s = tile_src[:, 0]
    want = ops.augment_images(flat, crop[:, 0], mode[:, 0], col[:, 0], (Ho, Wo), src_hw=hw[s], src_off=off[s], **kw)
    got = _mosaic(flat, hw, off, (tile_src, crop, mode, col, center), Ho, Wo, **kw)
    np.testing.assert_array_equal(got.float().cpu().numpy(), want.float().cpu().numpy())


@pytest.mark.parametrize('colour', [False, True])
def test_images_against_the_numpy_restatement(dev, sources, colour):
    srcs, flat, hw, off = sources
    Ho, Wo = 33, 47
    tables = _tables(5 + colour, CANVAS[(Ho, Wo)], colour)
    tile_src, crop, mode, col, center = tables
    got = _mosaic(flat, hw, off, tables, Ho, Wo).cpu().numpy()
    ref = np.stack([mr.mosaic_image(srcs, tile_src[b], crop[b], mode[b], col[b], center[b], Ho, Wo, False)
                    for b in range(len(center))])
    if colour:
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-3)
    else:
        np.testing.assert_array_equal(got, ref)


def test_wrapper_rejects_bad_tables_of_live_tiles(dev, sources):
    _, flat, hw, off = sources
    tables = _tables(1, [(10, 10)])
    bad = [a.copy() for a in tables]
    bad[0][0, 2] = len(HW)
    with pytest.raises(ValueError, match='tile_src'):
        _mosaic(flat, hw, off, bad, 20, 20)
    bad = [a.copy() for a in tables]
    bad[1][0, 3] = [0, 0, 1000, 4]
    with pytest.raises(ValueError, match='crop window'):
        _mosaic(flat, hw, off, bad, 20, 20)
    bad = [a.copy() for a in tables]
    bad[4][0] = [0, 10]
    with pytest.raises(ValueError, match='center'):
        _mosaic(flat, hw, off, bad, 20, 20)


# ------------------------------------------------------------------ boxes
def _box_sources(G, S=6):
    rng = np.random.default_rng(G)
    n = rng.integers(0, G + 1, S).astype(np.int32)
    n[0], n[1] = 0, G
    c = rng.uniform(0, 1, (S, G, 2))
    s = rng.uniform(0, 0.5, (S, G, 2))
    boxes = np.concatenate([c - s / 2, c + s / 2], -1).astype(np.float32)
    boxes[:, ::7, 2] = boxes[:, ::7, 0]            # zero-height boxes: safe_divide -> score 0
    labels = rng.integers(1, 11, (S, G)).astype(np.int32)
    return rng, boxes, labels, n


def _check_boxes(dev, boxes, labels, n, tile_src, ref, mode, center, Ho, Wo, gout, **kw):
    bo, lo, no = ops.mosaic_boxes(torch.from_numpy(boxes).to(dev), torch.from_numpy(labels).to(dev),
                                  torch.from_numpy(np.asarray(n, np.int32)).to(dev), tile_src, ref, mode, center,
                                  (Ho, Wo), gout=gout, **kw)
    assert bo.shape == (len(center), gout, 4) and lo.shape == (len(center), gout)
    bo, lo, no = bo.cpu().numpy(), lo.cpu().numpy(), no.cpu().numpy()
    counts = []
    for b in range(len(center)):
        rb, rl, rn = mr.mosaic_boxes(boxes, labels, n, tile_src[b], ref[b], mode[b], center[b], Ho, Wo, gout, **kw)
        assert no[b] == rn
        np.testing.assert_array_equal(bo[b], rb)       # the zero tail included
        np.testing.assert_array_equal(lo[b], rl)
        counts.append(rn)
    return counts


@pytest.mark.parametrize('G', [8, 64, 100])
def test_boxes_bit_exact(dev, G):
    """Sources with n = 0 and n = G, zero-height boxes, flips, boxes straddling the crop edge
    (clipped), plain and two-tile images beside full mosaics; G > 64 takes several wave rounds."""
    rng, boxes, labels, n = _box_sources(G)
    Ho, Wo = 96, 160
    center = np.array([(40, 70), (1, 1), (95, 159), (96, 160), (96, 33), (51, 160), (30, 101)], np.int32)
    B = len(center)
    tile_src = rng.integers(0, len(n), (B, 4)).astype(np.int32)
    tile_src[0] = [1, 0, 1, 2]                      # the full source twice, the empty one once
    tile_src[3, 1:] = [-3, 77, 1 << 20]             # empty tiles: never read
    y0, x0 = rng.uniform(0, 0.5, (B, 4)), rng.uniform(0, 0.5, (B, 4))
    ref = np.stack([y0, x0, y0 + rng.uniform(0.3, 0.5, (B, 4)), x0 + rng.uniform(0.3, 0.5, (B, 4))], -1)
    ref = ref.astype(np.float32)
    ref[2, 0] = [0, 0, 1, 1]
    mode = np.stack([rng.integers(0, 2, (B, 4)), np.zeros((B, 4))], -1).astype(np.int32)
    mode[0, :, 0] = [0, 1, 1, 0]
    full = _check_boxes(dev, boxes, labels, n, tile_src, ref, mode, center, Ho, Wo, 4 * G)
    assert max(full) > 0
    # min_px > 0 removes some more
    floor = _check_boxes(dev, boxes, labels, n, tile_src, ref, mode, center, Ho, Wo, 4 * G, min_px=6.0)
    assert sum(floor) < sum(full)
    # Gout smaller than the kept count: truncated in visiting order, tail zero
    small = max(1, max(full) // 2)
    cut = _check_boxes(dev, boxes, labels, n, tile_src, ref, mode, center, Ho, Wo, small)
    assert max(cut) == small and max(full) > small


def test_boxes_exact_ties_and_clipping(dev):
    """The dyadic hand case of test_mosaic_host.py: a score equal to the threshold is dropped, a
    size equal to min_px is kept, a box over the crop edge is clipped."""
    boxes = np.zeros((2, 4, 4), np.float32)
    labels = np.array([[1, 2, 3, 4], [5, 6, 7, 8]], np.int32)
    boxes[0, 0] = [0.25, 0.25, 0.75, 0.75]
    boxes[0, 1] = [0.5, 0.5, 0.5, 0.75]
    boxes[1, 0] = [0.0, 0.0, 0.5, 0.5]
    boxes[1, 1] = [0.25, 0.5, 0.75, 1.5]
    n = np.array([2, 2], np.int32)
    tile_src = np.array([[0, 1, 1, 0]], np.int32)
    ref = np.array([[[0, 0, 1, 1]] * 4], np.float32)
    ref[0, 2] = [0, 0, 0.5, 0.5]
    mode = np.array([[[0, 0], [1, 0], [0, 0], [0, 0]]], np.int32)
    center = np.array([[4, 8]], np.int32)
    assert _check_boxes(dev, boxes, labels, n, tile_src, ref, mode, center, 8, 16, 8) == [5]
    assert _check_boxes(dev, boxes, labels, n, tile_src, ref, mode, center, 8, 16, 8, threshold=0.5) == [4]
    assert _check_boxes(dev, boxes, labels, n, tile_src, ref, mode, center, 8, 16, 8, min_px=2.0) == [5]
    assert _check_boxes(dev, boxes, labels, n, tile_src, ref, mode, center, 8, 16, 8, min_px=2.5) == [1]
    assert _check_boxes(dev, boxes, labels, n, tile_src, ref, mode, center, 8, 16, 3) == [3]


@pytest.mark.parametrize('G', [8, 100])
def test_one_tile_boxes_are_the_plain_entry(dev, G):
    rng, boxes, labels, n = _box_sources(G)
    S = len(n)
    Ho, Wo = 33, 47
    y0, x0 = rng.uniform(0, 0.5, S), rng.uniform(0, 0.5, S)
    ref0 = np.stack([y0, x0, y0 + rng.uniform(0.3, 0.5, S), x0 + rng.uniform(0.3, 0.5, S)], 1).astype(np.float32)
    mode0 = np.stack([rng.integers(0, 2, S), np.zeros(S)], 1).astype(np.int32)
    tb, tl, tn = (torch.from_numpy(a).to(dev) for a in (boxes, labels, n))
    wb, wl, wn = ops.augment_boxes(tb, tl, tn, ref0, mode0)
    tile_src = np.repeat(np.arange(S, dtype=np.int32)[:, None], 4, 1)
    gb, gl, gn = ops.mosaic_boxes(tb, tl, tn, tile_src, np.repeat(ref0[:, None], 4, 1), np.repeat(mode0[:, None], 4, 1),
                                  np.tile(np.array([Ho, Wo], np.int32), (S, 1)), (Ho, Wo))
    assert torch.equal(gb, wb) and torch.equal(gl, wl) and torch.equal(gn, wn)


# ------------------------------------------------------------------ end to end
def test_mosaic_source_trains(dev):
    """The CLI's training source with mosaic on: augmented batches through one Trainer step."""
    from rod.dataio import AugmentedSource, mosaic_gout
    from rod.trainer import Trainer
    H, W, B = 96, 160, 2
    src = AugmentedSource(B, (H, W), dev, torch.bfloat16, seed=4, n_distinct=1, raw_hw=(120, 200), mosaic_prob=1.0)
    tr = Trainer((H, W), B, dtype=torch.bfloat16, device=dev, seed=1)
    x, bo, lo, no = next(src)
    tile_src, _, _, _, _, center = src.aug.last_params
    assert ((center >= 1) & (center < (H, W))).all()
    gout = mosaic_gout(src.raw[0][3], tile_src, center, (H, W))
    assert x.dtype == torch.bfloat16 and x.shape == (B, H, W, 3)
    assert bo.shape == (B, gout, 4) and lo.shape == (B, gout) and gout % 64 == 0
    assert float(x.float().abs().max()) < 1.5 and int(no.max()) <= gout and int(no.max()) > 0
    loss = tr.step(x, bo, lo, no)[0]
    assert np.isfinite(loss.item())


def test_mosaic_batches_replay_one_graph(dev):
    """B = 4: every image's tiles are the four images of the batch, so the box tensor keeps one
    shape and consecutive batches replay the captured step without re-capture."""
    from rod.dataio import AugmentedSource
    from rod.trainer import Trainer
    H, W, B = 96, 160, 4
    src = AugmentedSource(B, (H, W), dev, torch.bfloat16, seed=6, n_distinct=1, raw_hw=(120, 200), mosaic_prob=1.0)
    gout = max(64, -(-int(src.raw[0][3].sum()) // 64) * 64)
    tr = Trainer((H, W), B, dtype=torch.bfloat16, device=dev, seed=1)
    losses, centers = [], []
    for _ in range(3):                      # eager (set-up), capture + replay, replay
        x, bo, lo, no = next(src)
        assert bo.shape == (B, gout, 4)
        centers.append(src.aug.last_params[5].copy())
        losses.append(tr.step_graphed(x, bo, lo, no)[0].item())
    assert len(tr._graphs) == 1 and np.isfinite(losses).all()
    assert not np.array_equal(centers[1], centers[2])       # two different batches went through it
