"""Numpy restatement of the mosaic augmentation (rod_mosaic_images / rod_mosaic_boxes, ABI 30),
float32 per operation.

Tile t = 2 * (yo >= cy) + (xo >= cx) owns output pixel (yo, xo) of an Ho x Wo canvas with centre
(cy, cx): rectangles (oy0, ox0, th, tw) below.  The box side is written out in full; the image
side pastes oracle.augment.process_image results computed at the size of each tile."""
import numpy as np

from oracle import augment as oa

f32 = np.float32


def tile_rects(cy, cx, Ho, Wo):
    """(oy0, ox0, th, tw) of tiles 0..3."""
    return [(0, 0, cy, cx), (0, cx, cy, Wo - cx), (cy, 0, Ho - cy, cx), (cy, cx, Ho - cy, Wo - cx)]


def mosaic_image(srcs, tile_src, crop, mode, colour, center, Ho, Wo, normalize):
    """One output image [Ho, Wo, 3] float32: srcs a list of uint8 [H, W, 3]; tile_src [4], crop [4, 4],
    mode [4, 2], colour [4, 3]; center (cy, cx)."""
    out = np.zeros((Ho, Wo, 3), f32)
    for t, (oy0, ox0, th, tw) in enumerate(tile_rects(int(center[0]), int(center[1]), Ho, Wo)):
        if th == 0 or tw == 0:
            continue
        out[oy0:oy0 + th, ox0:ox0 + tw] = oa.process_image(srcs[int(tile_src[t])], crop[t], mode[t][0], mode[t][1],
                                                           colour[t], th, tw, normalize)
    return out


def mosaic_boxes(boxes, labels, n, tile_src, ref, mode, center, Ho, Wo, gout, threshold=0.3, min_px=0.0):
    """One output image: boxes [S, G, 4] / labels [S, G] / n [S] of the sources; tile_src [4], ref [4, 4],
    mode [4, 2].  Returns (boxes [gout, 4] float32, labels [gout] int32, n_out)."""
    bo = np.zeros((gout, 4), f32)
    lo = np.zeros(gout, np.int32)
    kept = 0
    zero, one = f32(0), f32(1)
    with np.errstate(divide='ignore', invalid='ignore'):
        for t, (oy0, ox0, th, tw) in enumerate(tile_rects(int(center[0]), int(center[1]), Ho, Wo)):
            if th == 0 or tw == 0:
                continue
            s = int(tile_src[t])
            r = np.asarray(ref[t], f32)
            sh, sw = f32(r[2] - r[0]), f32(r[3] - r[1])
            for i in range(int(n[s])):
                b = np.asarray(boxes[s][i], f32)
                # bboxes_resize
                y0, x0 = f32(f32(b[0] - r[0]) / sh), f32(f32(b[1] - r[1]) / sw)
                y1, x1 = f32(f32(b[2] - r[0]) / sh), f32(f32(b[3] - r[1]) / sw)
                # bboxes_filter_overlap: intersection with the unit box over the box's own area
                ih = max(f32(min(y1, one) - max(y0, zero)), zero)
                iw = max(f32(min(x1, one) - max(x0, zero)), zero)
                inter = f32(ih * iw)
                vol = f32(f32(y1 - y0) * f32(x1 - x0))
                score = f32(inter / vol) if vol > 0 else zero
                keep = bool(score > f32(threshold))
                if mode[t][0]:
                    x0, x1 = f32(one - x1), f32(one - x0)
                y0, x0, y1, x1 = (min(max(v, zero), one) for v in (y0, x0, y1, x1))
                # the size floor, in tile pixels, on the clipped box
                keep = keep and bool(f32(f32(y1 - y0) * f32(th)) >= f32(min_px)) and \
                    bool(f32(f32(x1 - x0) * f32(tw)) >= f32(min_px))
                if not keep:
                    continue
                if th != Ho:
                    y0, y1 = (f32(f32(f32(v * f32(th)) + f32(oy0)) / f32(Ho)) for v in (y0, y1))
                if tw != Wo:
                    x0, x1 = (f32(f32(f32(v * f32(tw)) + f32(ox0)) / f32(Wo)) for v in (x0, x1))
                if kept < gout:
                    bo[kept] = (y0, x0, y1, x1)
                    lo[kept] = labels[s][i]
                kept += 1
    return bo, lo, min(kept, gout)
