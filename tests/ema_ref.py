"""The contract of rod_sgd_momentum_ema (include/rod.h) restated in fp32 numpy, one rounded
operation per line: the lines of rod_sgd_momentum in their order, then the three lines of the
average on the value just written.  Shared by tests/test_ema_host.py and tests/test_gpu_ema.py."""
import numpy as np

f32 = np.float32


def ema_lines(e, p, rate):
    """e - rate * (e - p) in three fp32 operations, each rounded on its own (fp32 arrays in, the
    rate an fp32 scalar)."""
    rate = f32(rate)
    with np.errstate(invalid='ignore', over='ignore'):
        t = e - p
        t = rate * t
        en = e - t
    assert en.dtype == np.float32
    return en


def ref_step_ema(p, g, m, e, flags, lr, scale, rate, mu, wd, clip, nesterov):
    """One call of rod_sgd_momentum_ema: (p, m, e) after it.  m may be None (mu == 0); groups
    without bit 0 of their flag keep p, m and e."""
    tr = np.repeat(flags & 1, 4).astype(bool)
    dc = np.repeat(flags & 2, 4).astype(bool)
    with np.errstate(invalid='ignore', over='ignore'):
        d = g
        if scale is not None:
            d = d * f32(scale)
        d = np.where(np.isnan(d), d, np.minimum(np.maximum(d, f32(-clip)), f32(clip)))
        d = np.where(dc, d + f32(wd) * p, d)
        mn = d if m is None else f32(mu) * m + d
        u = d + f32(mu) * mn if nesterov else mn
        pn = p - f32(lr) * u
    assert pn.dtype == np.float32 and mn.dtype == np.float32
    en = ema_lines(e, pn, rate)
    return np.where(tr, pn, p), (None if m is None else np.where(tr, mn, m)), np.where(tr, en, e)


def ema_decay_at(decay, step, warmup=True):
    """tf.train.ExponentialMovingAverage's decay with num_updates = step."""
    return min(decay, (1.0 + step) / (10.0 + step)) if warmup else decay


def device_rate(decay, step, warmup=True):
    """What the device holds for the update of step `step`: float32(1 - decay), in Python floats."""
    return f32(1.0 - ema_decay_at(decay, step, warmup))
