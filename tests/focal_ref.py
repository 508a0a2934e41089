"""Focal loss of the ODM classifier restated in numpy (the semantics of include/rod.h,
rod_softmax_focal): row loss, the three normalised sums and the closed-form gradient.

    m = max_k x, e_k = exp(x_k - m), s = sum e_k, p_k = e_k / s, q = (s - e_t) / s,
    lp = (x_t - m) - log(s), a = alpha if pos else 1 - alpha,
    w = q^gamma (1 when gamma == 0, 0 when q == 0 and gamma > 0), FL = -a w lp,
    dFL/dx_k = a (delta_kt - p_k) (gamma q^(gamma-1) p_t lp - w)   [delta_tt - p_t = q; the first
               term of the bracket is 0 when q == 0],
    norm = max(n_pos, 1); pos_loss = sum_pos FL / norm, neg_loss = sum_neg FL / norm,
    clf_loss = pos_loss + neg_loss, grad = dFL/dx / norm.

focal(...) evaluates it in float64 (the reference), focal(..., dtype=np.float32) the same
formula operation by operation in float32 (exp and log correctly rounded, as the library's
exp_cr / log_cr), which is what a float32 implementation can be expected to reach.
"""
import numpy as np


def focal(logits, det_lbl, det_pos, alpha, gamma, n_pos=None, dtype=np.float64):
    """logits [..., K]; det_lbl / det_pos [...] -> dict(fl [R], pos_loss, neg_loss, clf_loss,
    n_pos, n_neg, norm, grad [..., K] float64, q [R]).  n_pos: the global positive count when the
    rows are one shard of a larger batch (default: this call's own)."""
    T = np.dtype(dtype).type
    K = logits.shape[-1]
    x = np.asarray(logits, np.float64).reshape(-1, K).astype(T)
    pos = np.asarray(det_pos).reshape(-1) != 0
    t = np.where(pos, np.asarray(det_lbl).reshape(-1), 0).astype(np.int64)
    assert ((t >= 0) & (t < K)).all()
    R = x.shape[0]
    rows = np.arange(R)
    alpha, gamma = T(alpha), T(gamma)
    m = x.max(1)
    d = x - m[:, None]
    e = np.exp(d.astype(np.float64)).astype(T)          # exp_cr: float64, rounded once
    s = np.zeros(R, T)
    for k in range(K):                                   # the kernel's summation order
        s = s + e[:, k]
    et = e[rows, t]
    p = e / s[:, None]
    pt = et / s
    q = (s - et) / s
    lp = d[rows, t] - np.log(s.astype(np.float64)).astype(T)
    a = np.where(pos, alpha, T(1) - alpha).astype(T)
    zero = q == 0
    with np.errstate(divide='ignore', invalid='ignore'):
        if gamma == 0:
            w = np.ones(R, T)
            t1 = np.zeros(R, T)
        else:
            w = np.where(zero, T(0), np.power(q, gamma)).astype(T)
            t1 = np.where(zero, T(0), gamma * (w / q) * pt * lp).astype(T)
    fl = -(a * w * lp)
    npos_local = int(pos.sum())
    n_pos = npos_local if n_pos is None else int(n_pos)
    norm = max(n_pos, 1)
    delta = -p
    delta[rows, t] = q
    coef = a * (t1 - w) / T(norm)
    grad = (delta * coef[:, None]).astype(np.float64).reshape(logits.shape)
    fl64 = fl.astype(np.float64)
    pos_loss = float(fl64[pos].sum() / norm)
    neg_loss = float(fl64[~pos].sum() / norm)
    return dict(fl=fl64, pos_loss=pos_loss, neg_loss=neg_loss, clf_loss=pos_loss + neg_loss, n_pos=n_pos,
                n_neg=R - npos_local, norm=norm, grad=grad, q=q.astype(np.float64), pt=pt.astype(np.float64),
                lp=lp.astype(np.float64))


def focal_f32(logits, det_lbl, det_pos, alpha, gamma, n_pos=None):
    """The same formula evaluated in float32."""
    return focal(logits, det_lbl, det_pos, alpha, gamma, n_pos=n_pos, dtype=np.float32)


def bf16_round(x):
    """float32 array rounded to bfloat16 (nearest even) and back."""
    import torch
    return torch.from_numpy(np.array(x, np.float32)).to(torch.bfloat16).float().numpy()


SHAPES = {'R37': (1, 37, 11), 'R256': (1, 256, 11), 'K2': (3, 781, 2), 'K16': (3, 781, 16), 'B4': (4, 781, 11)}
CASES = ('base', 'R37', 'R256', 'K2', 'K16', 'sat', 'satwrong', 'nopos', 'allpos')
_CACHE = {}


def case(name, bf16=False):
    """Inputs of one case (read-only arrays): logits ~ N(0, 2) float32 [B, A, K], about 10 % positives with
    labels in 1..K-1 (0 on the negatives).  B=3, A=781, K=11 unless the name says otherwise:
    25,773 elements (no multiple of 4 or 8), 10 blocks of 256 rows, the last of 39 rows.
      sat       40 rows (positive and negative) whose target logit is 100 above the others: q == 0
      satwrong  40 rows with a NON-target logit 100 above the others: p_t denormal or 0, lp ~ -100
      nopos / allpos
    The preconditions of each edge are asserted here on the float64 reference."""
    key = (name, bf16)
    if key in _CACHE:
        return _CACHE[key]
    B, A, K = SHAPES.get(name, (3, 781, 11))
    rng = np.random.default_rng(2017)
    logits = rng.normal(0, 2.0, (B, A, K)).astype(np.float32)
    pos = (rng.random((B, A)) < 0.1).astype(np.int32)
    if name == 'nopos':
        pos[:] = 0
    if name == 'allpos':
        pos[:] = 1
    lbl = (rng.integers(1, K, (B, A)) * pos).astype(np.int32)
    t = np.where(pos != 0, lbl, 0)
    if name in ('sat', 'satwrong'):
        flat, tf = logits.reshape(-1, K), t.reshape(-1)
        pick = np.concatenate([np.flatnonzero(pos.reshape(-1) != 0)[:20], np.flatnonzero(pos.reshape(-1) == 0)[:20]])
        for r in pick:
            c = tf[r] if name == 'sat' else (tf[r] + 1) % K
            flat[r, c] = np.float32(np.delete(flat[r], c).max() + 100)
    if bf16:
        logits = bf16_round(logits)
    ref = focal(logits, lbl, pos, 0.25, 2.0)
    assert np.isfinite(ref['grad']).all() and np.isfinite(ref['fl']).all()
    if name in ('base', 'K2', 'K16', 'sat', 'satwrong', 'B4'):
        assert 100 < ref['n_pos'] < ref['n_neg']
    if name in ('R37', 'R256'):
        assert 0 < ref['n_pos'] < ref['n_neg'] and B * A == int(name[1:])
    if name == 'base':
        assert (B * A * K) % 4 != 0 and -(-B * A // 256) == 10 and B * A % 256 == 39
    if name == 'sat':
        assert (ref['q'][pick] == 0).all() and (ref['q'] == 0).sum() == 40
        assert not ref['fl'][pick].any() and not ref['grad'].reshape(-1, K)[pick].any()
        assert not focal(logits, lbl, pos, 0.25, 0.5)['grad'].reshape(-1, K)[pick].any()
    if name == 'satwrong':
        assert (ref['pt'][pick] < 1e-37).all() and (ref['lp'][pick] < -99).all() and (ref['q'][pick] == 1).all()
    if name == 'nopos':
        assert ref['n_pos'] == 0 and ref['norm'] == 1 and ref['pos_loss'] == 0.0 and ref['neg_loss'] > 0
    if name == 'allpos':
        assert ref['n_neg'] == 0 and ref['neg_loss'] == 0.0 and ref['pos_loss'] > 0
    for v in (logits, lbl, pos):
        v.flags.writeable = False
    _CACHE[key] = dict(logits=logits, lbl=lbl, pos=pos, B=B, A=A, K=K, pick=pick if name.startswith('sat') else None)
    return _CACHE[key]


def grad_excess(got, ref, rel, floor=1e-8):
    """max over the elements of |got - ref| / (rel |ref| + floor): <= 1 passes."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (rel * np.abs(ref) + floor)).max())
