"""Host mirror of the reference's utils/data_pileline_tools.py (same module name, typo kept).

The reference decodes one image at a time on 4 CPU threads and runs the TF image ops per
image.  Here a batch of decoded uint8 images already on the device goes through two librod
launches per step (rod_augment_images, rod_augment_boxes); only the random parameters are
drawn on the host:

  prepare_data_train / process_raw_data_train  data_pileline_tools.py:45-108
  prepare_data_test                            data_pileline_tools.py:18-43
"""
import numpy as np
import torch

from rod import ops
from utils.augmentation import process


class TrainAugmenter(object):
    """process_raw_data_train for batches (data_pileline_tools.py:76-108):

        distorted_bounding_box_crop(min_object_covered=0.4, aspect_ratio_range=(0.6, 1.67))
        -> resize_image(out_shape, BILINEAR, align_corners=False)
        -> random_flip_left_right
        -> apply_with_random_selector(distort_color(fast_mode=False), 4 orderings)
        -> clip boxes to [0, 1]

    and, fused when `dtype` is given, train.py:126 `(2/255) * imgs - 1` cast to DTYPE.
    `seed` drives the per-image draws (numpy); the colour magnitudes come from Python's
    `random`, once per augmenter, as the reference draws them once per graph.

    Mosaic (opt-in, mosaic_prob > 0; rod_mosaic_images / rod_mosaic_boxes): with that probability
    output image b becomes four tiles around a centre drawn on the integers of
    [lo * size, hi * size] (mosaic_center = (lo, hi), clamped to [1, size - 1]) — tile 0 image b
    itself, tiles 1-3 three other images of the same batch — each tile with its own crop, flip
    and colour draw by the rules above; boxes smaller than mosaic_min_px tile pixels are dropped.
    Everything mosaic adds is drawn from a second generator, so the draws of tile 0 are the
    sequence a plain augmenter of the same seed draws."""

    def __init__(self, out_shape, seed=0, py_random=None, mosaic_prob=0.0, mosaic_center=(0.25, 0.75),
                 mosaic_min_px=2.0):
        import random
        self.out_shape = tuple(out_shape)
        self.rng = np.random.default_rng(seed)
        self.color = process.ColorDistorter(py_random if py_random is not None else random.Random(seed))
        lo, hi = (float(v) for v in mosaic_center)
        if not 0.0 <= float(mosaic_prob) <= 1.0:       # (a NaN fails both comparisons)
            raise ValueError('mosaic_prob must be in [0, 1], got %r' % (mosaic_prob,))
        if not 0.0 <= lo <= hi <= 1.0:
            raise ValueError('mosaic_center must be 0 <= lo <= hi <= 1, got %r' % (mosaic_center,))
        if not 0.0 <= float(mosaic_min_px) < float('inf'):
            raise ValueError('mosaic_min_px must be finite and >= 0, got %r' % (mosaic_min_px,))
        self.mosaic_prob, self.mosaic_center, self.mosaic_min_px = float(mosaic_prob), (lo, hi), float(mosaic_min_px)
        self.mosaic_rng = np.random.default_rng([int(seed) & 0xFFFFFFFF, 0x6D6F7361])   # 'mosa'

    def sample(self, src_hw, boxes, n):
        """Per-image parameters: crop [B,4], distort_bbox [B,4], mode [B,2], colour [B,3]."""
        B = len(src_hw)
        crop = np.zeros((B, 4), np.int32)
        ref = np.zeros((B, 4), np.float32)
        mode = np.zeros((B, 2), np.int32)
        colour = np.zeros((B, 3), np.float32)
        for b in range(B):
            H, W = int(src_hw[b][0]), int(src_hw[b][1])
            crop[b], ref[b] = process.distorted_bounding_box_crop(self.rng, H, W, boxes[b][:int(n[b])],
                                                                  min_object_covered=0.4,
                                                                  aspect_ratio_range=(0.6, 1.67))
            mode[b, 0] = int(self.rng.uniform(0, 1) < .5)       # random_flip_left_right
            mode[b, 1], colour[b] = self.color.sample(self.rng)  # apply_with_random_selector
        return crop, ref, mode, colour

    def _draw(self, rng, H, W, boxes):
        """One image's crop, distort_bbox, flip and colour draw from `rng`, in sample()'s order."""
        crop, ref = process.distorted_bounding_box_crop(rng, H, W, boxes, min_object_covered=0.4,
                                                        aspect_ratio_range=(0.6, 1.67))
        flip = int(rng.uniform(0, 1) < .5)
        ordering, colour = self.color.sample(rng)
        return crop, ref, (flip, ordering), colour

    def _center(self, size):
        lo, hi = self.mosaic_center
        a, b = int(np.ceil(lo * size)), int(np.floor(hi * size))
        c = int(self.mosaic_rng.integers(a, b + 1)) if b >= a else int(round(.5 * (lo + hi) * size))
        return min(max(c, 1), max(size - 1, 1))

    def sample_mosaic(self, src_hw, boxes, n):
        """Tile tables of a batch: tile_src [B,4], crop [B,4,4], distort_bbox [B,4,4], mode [B,4,2],
        colour [B,4,3], center [B,2].  Tile 0 of image b is image b with sample()'s draws (from the
        same generator, in the same order); a non-mosaic image has center = out_shape, i.e. tile 0
        alone.  The other tiles' rows of such an image repeat tile 0's and are never read."""
        B = len(src_hw)
        Ho, Wo = self.out_shape
        crop0, ref0, mode0, colour0 = self.sample(src_hw, boxes, n)
        tile_src = np.repeat(np.arange(B, dtype=np.int32)[:, None], 4, 1)
        crop, ref = np.repeat(crop0[:, None], 4, 1), np.repeat(ref0[:, None], 4, 1)
        mode, colour = np.repeat(mode0[:, None], 4, 1), np.repeat(colour0[:, None], 4, 1)
        center = np.tile(np.array([Ho, Wo], np.int32), (B, 1))
        rng = self.mosaic_rng
        for b in range(B):
            if not (self.mosaic_prob > 0 and Ho > 1 and Wo > 1 and rng.uniform(0, 1) < self.mosaic_prob):
                continue
            center[b] = self._center(Ho), self._center(Wo)
            if B >= 4:      # three other images, distinct
                others = np.delete(np.arange(B), b)
                tile_src[b, 1:] = rng.choice(others, 3, replace=False)
            else:           # too few for that: any image of the batch, with replacement
                tile_src[b, 1:] = rng.integers(0, B, 3)
            for t in range(1, 4):
                s = int(tile_src[b, t])
                crop[b, t], ref[b, t], mode[b, t], colour[b, t] = self._draw(
                    rng, int(src_hw[s][0]), int(src_hw[s][1]), boxes[s][:int(n[s])])
        return tile_src, crop, ref, mode, colour, center

    def mosaic(self, images, boxes, labels, n, dtype=None, params=None, gout=None):
        """__call__ through the mosaic entries (images [B, H, W, 3] are the batch's own sources)."""
        boxes = np.asarray(boxes, np.float32)
        B, H, W, _ = images.shape
        src_hw = np.tile(np.array([H, W], np.int32), (B, 1))
        tile_src, crop, ref, mode, colour, center = params if params is not None else \
            self.sample_mosaic(src_hw, boxes, n)
        img = ops.mosaic_images(images, tile_src, crop, mode, colour, center, self.out_shape,
                                dtype=dtype if dtype is not None else torch.float32, normalize=dtype is not None)
        bo, lo, no = ops.mosaic_boxes(boxes, labels, n, tile_src, ref, mode, center, self.out_shape, gout=gout,
                                      threshold=process.BBOX_CROP_OVERLAP, min_px=self.mosaic_min_px)
        self.last_params = (tile_src, crop, ref, mode, colour, center)
        return img, bo, lo, no

    def __call__(self, images, boxes, labels, n, dtype=None, params=None):
        """images: uint8 [B, H, W, 3] device tensor; boxes [B, G, 4] / labels [B, G] / n [B] as
        HOST arrays (annotations come from the reader on the host).  Returns device tensors
        (image, boxes, labels, n): image float 0-255 [B, Ho, Wo, 3], or the normalised
        network input in `dtype`."""
        boxes = np.asarray(boxes, np.float32)
        B, H, W, _ = images.shape
        src_hw = np.tile(np.array([H, W], np.int32), (B, 1))
        crop, ref, mode, colour = params if params is not None else self.sample(src_hw, boxes, n)
        img = ops.augment_images(images, crop, mode, colour, self.out_shape,
                                 dtype=dtype if dtype is not None else torch.float32, normalize=dtype is not None)
        bo, lo, no = ops.augment_boxes(boxes, labels, n, ref, mode, threshold=process.BBOX_CROP_OVERLAP)
        self.last_params = (crop, ref, mode, colour)
        return img, bo, lo, no


def process_raw_data_train(images, labels, bboxes, n, out_shape, seed=0, dtype=None):
    """One-shot form of TrainAugmenter (argument order of the reference: image, labels, bboxes)."""
    return TrainAugmenter(out_shape, seed)(images, bboxes, labels, n, dtype=dtype)


def prepare_data_test(images, out_shape, dtype=None):
    """resize_image(config.img_size, BILINEAR, align_corners=False) only (data_pileline_tools.py:39-40);
    boxes are unchanged.  With `dtype`, fused (2/255)x - 1 (evaluate.py / predict.py:98)."""
    B, H, W, _ = images.shape
    crop = np.tile(np.array([0, 0, H, W], np.int32), (B, 1))
    mode = np.tile(np.array([0, -1], np.int32), (B, 1))
    return ops.augment_images(images, crop, mode, np.zeros((B, 3), np.float32), out_shape,
                              dtype=dtype if dtype is not None else torch.float32, normalize=dtype is not None)
