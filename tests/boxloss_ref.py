"""IoU / GIoU / DIoU / CIoU regression loss of the ODM box restated in numpy (the semantics of
include/rod.h, rod_box_iou_loss): row losses, per-level sums, the total and the closed-form gradient.

    s = f32(refine_out) + f32(det_out)                       (summed in float32, as rod_decode)
    cy = s0 ah + acy, cx = s1 aw + acx, h = exp(s2) ah, w = exp(s3) aw
    p = (cy - h/2, cx - w/2, cy + h/2, cx + w/2), g likewise from cbox = (gcy, gcx, gh, gw)
    I = max(min(py1, gy1) - max(py0, gy0), 0) max(min(px1, gx1) - max(px0, gx0), 0)
    U = (px1 - px0)(py1 - py0) - I + (gy1 - gy0)(gx1 - gx0), IoU = I / U
    eh = max(py1, gy1) - min(py0, gy0), ew likewise, C = eh ew, c2 = eh^2 + ew^2
    rho2 = (cy - gcy)^2 + (cx - gcx)^2
    v = (4 / pi^2) (atan(gw / gh) - atan(w / h))^2, alpha = v / ((1 - IoU) + v), 0 when v == 0
    iou: 1 - IoU   giou: 1 - IoU + (C - U) / C   diou: 1 - IoU + rho2 / c2   ciou: diou + alpha v
    lvl[l] = weight sum_rows / scale, total = sum_l lvl[l]; grad = d total / d s with alpha held
    constant; at ties max passes to the prediction when p >= g, min when p <= g, max(., 0) at >= 0.

box_loss(...) evaluates it in float64 (the reference), box_loss(..., dtype=np.float32) the same
formula operation by operation in float32 with exp and atan rounded once from float64 (the
library's exp_cr), which is what a float32 implementation can be expected to reach.

Error measure of a gradient (grad_excess): a row's four components share their intermediate
quantities (one IoU, one enclosing box), so a component that is small because its terms cancel carries
the absolute error of the large ones: the error is taken relative to the row's largest component,
|got - ref| / (rel * max_k |ref[row, k]| + floor).

E32_GRAD / E32_LOSS are the float32 restatement's worst such error against float64 (beyond the
absolute floors below) over every case and kind, rounded up (measured and asserted by tests/test_boxloss_host.py); the GPU test's bounds
are M times them.
"""
import numpy as np

KINDS = {'iou': 0, 'giou': 1, 'diou': 2, 'ciou': 3}
MAXL = 8                     # the library's maximum level count (csrc/box_common.h)
# measured by tests/test_boxloss_host.py::test_float32_restatement_error and rounded up: the worst case is
# `thin` (2.11e-5 / 1.62e-6: a box 0.01 wide at a coordinate of 0.5 loses 6 bits in cx +- w/2), the
# others stay below 4.1e-6 / 1.5e-7
E32_GRAD = 2.5e-5            # relative to the row's largest gradient component
E32_LOSS = 2e-6              # relative, per-level sums and total
M = 4                        # the kernel's bound = M * E32: FMA contraction, differently rounded exp / atan
# absolute floors: a gradient component is a sum of terms of size weight / scale = 1/3 that may cancel
# (disjoint boxes, prediction == target), each rounded to 2**-24 / 3 = 2e-8 in float32; a level sum of
# rows that are each exactly 0 stays exactly 0, one that cancels to nearly 0 keeps the rows' 6e-8
FLOOR = 1e-7
LOSS_FLOOR = 1e-7


def _cr(fn, x, T):
    """fn evaluated in float64 and rounded once to T (exp_cr)."""
    return fn(np.asarray(x, np.float64)).astype(T)


def summed_offsets(ro, do):
    """refine_out + det_out in float32 (inputs: float32 arrays holding fp32 or bf16-rounded values)."""
    return np.asarray(ro, np.float32) + np.asarray(do, np.float32)


def box_loss(anc, ro, do, cbox, pos, lvl_off, kind, weight=1.0, scale=1.0, dtype=np.float64, s=None, alpha=None):
    """anc [A, 4] centre form; ro / do [B, A, 4]; cbox [B, A, 4]; pos [B, A]; kind: name or 0..3.
    s: the summed offsets given directly (finite differences); alpha: CIoU's alpha given (held).
    -> dict(row [B, A], lvl [L], total, grad [B, A, 4] float64, iou, alpha, tie [B, A])."""
    kind = KINDS.get(kind, kind)
    assert kind in (0, 1, 2, 3)
    T = np.dtype(dtype).type
    s = (summed_offsets(ro, do) if s is None else np.asarray(s)).astype(T)
    az = np.asarray(anc, np.float32).astype(T)[None]
    gz = np.asarray(cbox, np.float32).astype(T)
    m = np.asarray(pos) != 0
    two, one, zero = T(2), T(1), T(0)
    k4 = T(np.float32(4 / np.pi ** 2)) if T is np.float32 else T(4 / np.pi ** 2)
    with np.errstate(all='ignore'):
        cy, cx = s[..., 0] * az[..., 2] + az[..., 0], s[..., 1] * az[..., 3] + az[..., 1]
        h, w = _cr(np.exp, s[..., 2], T) * az[..., 2], _cr(np.exp, s[..., 3], T) * az[..., 3]
        py0, px0, py1, px1 = cy - h / two, cx - w / two, cy + h / two, cx + w / two
        gy0, gx0 = gz[..., 0] - gz[..., 2] / two, gz[..., 1] - gz[..., 3] / two
        gy1, gx1 = gz[..., 0] + gz[..., 2] / two, gz[..., 1] + gz[..., 3] / two
        ph, pw = py1 - py0, px1 - px0
        ap = pw * ph
        ihr = np.minimum(py1, gy1) - np.maximum(py0, gy0)
        iwr = np.minimum(px1, gx1) - np.maximum(px0, gx0)
        ih, iw = np.maximum(ihr, zero), np.maximum(iwr, zero)
        I = ih * iw
        U = ap - I + (gy1 - gy0) * (gx1 - gx0)
        iou = I / U
        row = one - iou
        q = I / (U * U)
        d_I, d_ap = -(one / U + q), q
        z = np.zeros_like(row)
        d_eh, d_ew, d_cy, d_cx, d_h, d_w = z, z, z, z, z, z
        al = z
        if kind != 0:
            eh, ew = np.maximum(py1, gy1) - np.minimum(py0, gy0), np.maximum(px1, gx1) - np.minimum(px0, gx0)
            if kind == 1:
                C = eh * ew
                row = row + (C - U) / C
                invC, dC = one / C, U / (C * C)
                d_I, d_ap = d_I + invC, d_ap - invC
                d_eh, d_ew = dC * ew, dC * eh
            else:
                c2 = eh * eh + ew * ew
                dy, dx = cy - gz[..., 0], cx - gz[..., 1]
                rho2 = dy * dy + dx * dx
                row = row + rho2 / c2
                d_c2, ir = -(rho2 / (c2 * c2)), one / c2
                d_eh, d_ew = d_c2 * (two * eh), d_c2 * (two * ew)
                d_cy, d_cx = ir * (two * dy), ir * (two * dx)
                if kind == 3:
                    dat = _cr(np.arctan, gz[..., 3] / gz[..., 2], T) - _cr(np.arctan, w / h, T)
                    v = k4 * (dat * dat)
                    al = np.where(v == 0, zero, v / ((one - iou) + v)) if alpha is None else np.asarray(alpha).astype(T)
                    row = row + al * v
                    tv, hw2 = al * ((two * k4) * dat), h * h + w * w
                    d_w, d_h = -(tv * (h / hw2)), tv * (w / hw2)
        d_ih, d_iw = np.where(ihr >= 0, d_I * iw, zero), np.where(iwr >= 0, d_I * ih, zero)
        d_py1, d_py0 = np.where(py1 <= gy1, d_ih, zero), np.where(py0 >= gy0, -d_ih, zero)
        d_px1, d_px0 = np.where(px1 <= gx1, d_iw, zero), np.where(px0 >= gx0, -d_iw, zero)
        d_py1 = d_py1 + np.where(py1 >= gy1, d_eh, zero)
        d_py0 = d_py0 + np.where(py0 <= gy0, -d_eh, zero)
        d_px1 = d_px1 + np.where(px1 >= gx1, d_ew, zero)
        d_px0 = d_px0 + np.where(px0 <= gx0, -d_ew, zero)
        d_px1, d_px0 = d_px1 + d_ap * ph, d_px0 - d_ap * ph
        d_py1, d_py0 = d_py1 + d_ap * pw, d_py0 - d_ap * pw
        d_cy, d_cx = d_cy + (d_py0 + d_py1), d_cx + (d_px0 + d_px1)
        d_h, d_w = d_h + (d_py1 - d_py0) / two, d_w + (d_px1 - d_px0) / two
        gs = T(weight) / T(scale)
        g = np.stack([d_cy * az[..., 2] * gs, d_cx * az[..., 3] * gs, d_h * h * gs, d_w * w * gs], -1)
        # distance to the nearest tie of a max / min / max(., 0), in units of the anchor's size
        tie = np.minimum.reduce([np.abs(py1 - gy1), np.abs(py0 - gy0), np.abs(ihr)]) / az[..., 2]
        tie = np.minimum(tie, np.minimum.reduce([np.abs(px1 - gx1), np.abs(px0 - gx0), np.abs(iwr)]) / az[..., 3])
    row = np.where(m, row, zero)
    grad = np.where(m[..., None], g, zero).astype(np.float64)
    L = len(lvl_off) - 1
    row64 = row.astype(np.float64)
    lvl = np.array([float(T(weight) * T(row64[:, lvl_off[l]:lvl_off[l + 1]].sum()) / T(scale)) for l in range(L)])
    return dict(row=row64, lvl=lvl, total=float(lvl.sum()), grad=grad, iou=np.where(m, iou, zero).astype(np.float64),
                alpha=np.where(m, al, zero).astype(np.float64), tie=np.where(m, tie, np.inf).astype(np.float64))


def bf16_round(x):
    """float32 array rounded to bfloat16 (nearest even) and back."""
    import torch
    return torch.from_numpy(np.array(x, np.float32)).to(torch.bfloat16).float().numpy()


def grad_excess(got, ref, rel, floor=FLOOR, extra=0.0):
    """max over the elements of |got - ref| / (rel * rowmax|ref| + extra * |ref| + floor): <= 1 passes."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bound = rel * np.abs(ref).max(-1, keepdims=True) + extra * np.abs(ref) + floor
    return float((np.abs(got - ref) / bound).max())


CASES = ('base', 'nopos', 'allpos', 'disjoint', 'inside', 'outside', 'same', 'thin', 'far', 'L1', 'Lmax')
LVL3 = (0, 37, 293, 781)
_CACHE = {}


def case(name, bf16=False):
    """Inputs of one case (read-only arrays; B=3, levels of 37, 256 and 488 anchors, A=781, unless the
    name says otherwise): anchors in centre form inside the unit image, about 10 % positives, cbox 0
    off the positives (as rod_match_anchors writes it), refine_out ~ N(0, 0.2) and det_out the rest
    of the summed offset s.  bf16: refine_out / det_out rounded to bfloat16.
      base      s = encode(target) + noise of a per-row size in (0, 1.2): IoU spread over (0, 1)
      nopos / allpos
      disjoint  the target 3 anchor sizes away: IoU exactly 0
      inside    the prediction strictly inside the target     outside  the reverse
      same      target = anchor, refine_out = -det_out: s == 0 exactly, prediction == target in
                every precision, every max / min at its tie
      thin      anchors and targets of aspect 1:50 and 50:1
      far       |s2|, |s3| up to 8
      L1        one level of 37 anchors      Lmax  8 levels, five of them empty
    The preconditions of each edge are asserted here on the float64 reference."""
    key = (name, bf16)
    if key in _CACHE:
        return _CACHE[key]
    f32 = np.float32
    rng = np.random.default_rng(2019)
    B = 3
    lvl_off = {'L1': (0, 37), 'Lmax': (0, 37, 37, 293, 293, 293, 781, 781, 781)}.get(name, LVL3)
    A = lvl_off[-1]
    anc = np.stack([rng.uniform(0.1, 0.9, A), rng.uniform(0.1, 0.9, A), rng.uniform(0.05, 0.4, A),
                    rng.uniform(0.05, 0.4, A)], -1).astype(f32)
    if name == 'thin':
        tall = rng.random(A) < 0.5
        anc[:, 2] = np.where(tall, 0.5, 0.01)
        anc[:, 3] = np.where(tall, 0.01, 0.5)
    pos = (rng.random((B, A)) < 0.1).astype(np.int32)
    if name == 'nopos':
        pos[:] = 0
    if name == 'allpos':
        pos[:] = 1
    u = lambda lo, hi, n=4: rng.uniform(lo, hi, (B, A, n))     # noqa: E731
    t = np.concatenate([u(-0.3, 0.3, 2), u(-0.5, 0.5, 2)], -1)  # the target's encoding against the anchor
    s = t + rng.uniform(0, 1.2, (B, A, 1)) * rng.normal(0, 0.5, (B, A, 4))
    if name == 'disjoint':
        t[..., :2] = 3.0
        t[..., 2:] = 0.0
        s = u(-0.1, 0.1)
    if name == 'inside':
        t[..., :2] = 0.0
        t[..., 2:] = np.log(2.0)
        s = np.concatenate([u(-0.2, 0.2, 2), u(-0.5, 0.0, 2)], -1)
    if name == 'outside':
        t = np.concatenate([u(-0.1, 0.1, 2), np.full((B, A, 2), np.log(0.4))], -1)
        s = np.concatenate([u(-0.1, 0.1, 2), u(0.0, 0.5, 2)], -1)
    if name == 'same':
        t[:] = 0.0
        s[:] = 0.0
    if name == 'thin':
        t[..., 2:] = u(-0.2, 0.2, 2)
        s = t + u(-0.2, 0.2)
    if name == 'far':
        s[..., 2:] = u(-8.0, 8.0, 2)
    a64 = anc.astype(np.float64)[None]
    cbox = np.stack([t[..., 0] * a64[..., 2] + a64[..., 0], t[..., 1] * a64[..., 3] + a64[..., 1],
                     np.exp(t[..., 2]) * a64[..., 2], np.exp(t[..., 3]) * a64[..., 3]], -1).astype(f32)
    if name == 'same':
        cbox = np.broadcast_to(anc[None], (B, A, 4)).copy()
    cbox[pos == 0] = 0
    ro = rng.normal(0, 0.2, (B, A, 4)).astype(f32)
    if bf16:
        ro = bf16_round(ro)
    do = (s.astype(f32) - ro).astype(f32)
    if bf16:
        do = bf16_round(do)
    m = pos != 0
    ref = {k: box_loss(anc, ro, do, cbox, pos, lvl_off, k) for k in KINDS}
    r0 = ref['iou']
    for k in KINDS:
        assert np.isfinite(ref[k]['grad']).all() and np.isfinite(ref[k]['row']).all(), (name, k)
    if name not in ('nopos', 'allpos'):
        assert 0.05 * B * A < m.sum() < 0.15 * B * A
    if name == 'base':
        i = r0['iou'][m]
        assert i.min() < 0.05 and i.max() > 0.95 and 0.3 < np.median(i) < 0.8
        assert -(-B * 37 // 256) == 1 and B * 256 % 256 == 0 and B * 488 % 256 == 184
    if name == 'nopos':
        assert not m.any() and r0['total'] == 0.0
    if name == 'allpos':
        assert m.all()
    if name == 'disjoint':
        assert not r0['iou'].any() and (r0['row'][m] == 1.0).all()
    if name in ('inside', 'outside', 'disjoint'):
        assert r0['tie'][m].min() > 1e-3
    if name == 'same':
        assert not summed_offsets(ro, do).any() and all(not ref[k]['row'].any() for k in KINDS)
        assert (r0['tie'][m] == 0).all()
    if name == 'thin':
        r = cbox[m][:, 2] / cbox[m][:, 3]
        assert ((r > 20) | (r < 1 / 20)).all() and (r > 50).any() and (r < 1 / 50).any()
    if name == 'far':
        a = np.abs(summed_offsets(ro, do)[..., 2:][m])
        assert 7.5 < a.max() < 8.2
    for v in (anc, ro, do, cbox, pos):
        v.flags.writeable = False
    _CACHE[key] = dict(anc=anc, ro=ro, do=do, cbox=cbox, pos=pos, lvl_off=lvl_off, B=B, A=A)
    return _CACHE[key]


_REF = {}


def reference(name, kind, bf16=False, weight=1.0, scale=3.0):
    """box_loss in float64 on case(name, bf16), computed once and shared (read-only)."""
    key = (name, kind, bf16, weight, scale)
    if key not in _REF:
        c = case(name, bf16)
        r = box_loss(c['anc'], c['ro'], c['do'], c['cbox'], c['pos'], c['lvl_off'], kind, weight, scale)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.flags.writeable = False
        _REF[key] = r
    return _REF[key]
