"""The BatchNorm partial-statistics slab ([nparts][3][C] of count, mean, M2; csrc/bnstat_common.h)
as each of its fused producers writes it, at the smallest shapes where each form can go wrong:
the pivot's 8-row edge, the 32- / 64-row wave strips and the 128-row tile of the tiled conv, ragged
last tiles of the streaming 1x1, the narrowest MFMA stem, row strips around DW_RB of the direct
depthwise forward, and 7 / 8 / 9 / 17 tile columns (below one run of 8, one run, one run plus a
column, three runs) of the column-tile depthwise forwards, stored and recomputed.

For every producer and shape:
  (a) y with statistics equals y without, bit for bit;
  (b) every count is a non-negative integer and the counts of a channel sum to exactly M;
  (c) parts with count 0 have mean = M2 = 0;
  (d) the parts merged on the host in float64 (Chan) agree with the float64 mean and biased
      variance of the stored y.

The bound of (d) comes from the reference, not from the producers: the unfused statistics pass
(rod_bn_stat_parts, bn_stats_kernel: the parts rod_bn_stats reduces) runs on the same stored y, its
parts go through the same host merge, and its error against float64 is the yardstick; a fused
producer may err 4x that (its parts are smaller tiles, so more merge steps).  Where the reference
happens to be exact (one row; a handful of rows), the yardstick is floored at one fp32 ulp, 2^-23:
both write fp32 parts, so neither can be asked for better than the slab's own rounding.  Errors
are relative to the channel's scale: |mean - mean64| / (|mean64| + std64) and
|var - var64| / (var64 + mean64^2).

Measured on MI355X, largest over each group's cases, in units of 2^-23 (every case prints its
own as `bnstat <name>: ref (mean, var) fused (mean, var) ulp`):
  conv1x1    reference mean 2.37 var 14.28 | fused mean 0.75 var 2.36
  stream     reference mean 0.02 var 0.29 | fused mean 0.01 var 0.24
  stem       reference mean 0.17 var 0.44 | fused mean 0.41 var 3.68
  dw direct  reference mean 0.24 var 1.19 | fused mean 0.61 var 3.00
  dw lx      reference mean 0.29 var 1.01 | fused mean 0.41 var 1.40
  dw rc      reference mean 0.32 var 2.17 | fused mean 0.50 var 1.51
The column-tile cases assert the plan they mean to hit: one part per image, that is one strip and
one column tile, so P = Wo + halo columns exactly (a re-plan that split the map would fail the case
instead of quietly turning it into another).  The recompute forward reaches 17 columns at C = 48
(12 channel vectors a block); at C = 96 its plan prefers 24 vectors and 10 columns, so 7 / 8 / 9
run at C = 96 and 17 at C = 48.  Cout = 36 never reaches a fused epilogue (not a multiple of 8: the
direct-store kernel, then the separate statistics pass), so that case checks (a)-(c) and the
dispatch, and (d) compares the reference with itself.
"""
import numpy as np
import pytest
import torch

from rod import _abi, ops

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
ULP = 2.0 ** -23


def _merge64(parts):
    """Chan merge of [nparts][3][C] in float64, part order; parts with count 0 skipped."""
    p = parts.detach().cpu().double().numpy()
    C = p.shape[2]
    n, mu, m2 = np.zeros(C), np.zeros(C), np.zeros(C)
    for q in p:
        nb, mb, qb = q
        nn = n + nb
        safe = np.where(nn > 0, nn, 1.0)
        d = mb - mu
        mu = np.where(nb > 0, mu + d * nb / safe, mu)
        m2 = np.where(nb > 0, m2 + qb + d * d * n * nb / safe, m2)
        n = nn
    return n, mu, m2 / np.where(n > 0, n, 1.0)


def _err(parts, mean64, var64):
    _, mu, var = _merge64(parts)
    std = np.sqrt(var64)
    em = np.max(np.abs(mu - mean64) / (np.abs(mean64) + std + 1e-300))
    ev = np.max(np.abs(var - var64) / (var64 + mean64 ** 2 + 1e-300))
    return float(em), float(ev)


def _check(name, y, y_plain, parts, dev):
    C = y.shape[-1]
    M = y.numel() // C
    torch.cuda.synchronize()
    assert torch.equal(y, y_plain), name                                          # (a)
    p = parts.detach().cpu()
    cnt = p[:, 0, :]
    assert bool((cnt >= 0).all()) and torch.equal(cnt, cnt.round()), name         # (b)
    assert torch.equal(cnt.double().sum(0), torch.full((C,), float(M), dtype=torch.float64)), name
    empty = cnt == 0
    assert bool((p[:, 1, :][empty] == 0).all()) and bool((p[:, 2, :][empty] == 0).all()), name   # (c)
    y64 = y.detach().reshape(M, C).cpu().double().numpy()                         # (d)
    mean64, var64 = y64.mean(0), y64.var(0)
    nref = ops._sync_nparts(M)
    ref = torch.empty((nref, 3, C), dtype=torch.float32, device=dev)
    _abi.call("rod_bn_stat_parts", y.contiguous(), M, C, ref, nref, ops.dtcode(y), ops.stream())
    torch.cuda.synchronize()
    rm, rv = _err(ref, mean64, var64)
    fm, fv = _err(parts, mean64, var64)
    print('bnstat %s: ref (%.2f, %.2f) fused (%.2f, %.2f) ulp' % (name, rm / ULP, rv / ULP, fm / ULP, fv / ULP))
    assert fm <= 4 * max(rm, ULP), (name, fm / ULP, rm / ULP)
    assert fv <= 4 * max(rv, ULP), (name, fv / ULP, rv / ULP)


def _conv_case(name, dev, dtype, N, H, W, Cin, Cout, ks, seed, bias=True):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, H, W, Cin, generator=g) + 0.5).to(dev, dtype)
    w = (torch.randn(Cout, ks, ks, Cin, generator=g) / np.sqrt(ks * ks * Cin)).to(dev)
    b = (torch.randn(Cout, generator=g) * 0.3).to(dev) if bias else None
    y, parts = ops.conv2d(x, w, b, ks, want_stats=True)
    _check(name, y, ops.conv2d(x, w, b, ks), parts, dev)


# one Cout per N tile of the tiled kernel's menu (32 .. 192 in steps of 32, 256, and 128-wide tiles
# above 256), and 36: not a multiple of 8, the direct-store kernel
@pytest.mark.parametrize('dtype', [torch.float32, bf16])
@pytest.mark.parametrize('Cout', [32, 64, 96, 128, 160, 192, 256, 384, 36])
def test_conv_tiled_parts(dev, dtype, Cout):
    for M in (1, 7, 8, 9, 31, 32, 33, 127, 128, 129):
        _conv_case('conv1x1 M=%d Cout=%d %s' % (M, Cout, dtype), dev, dtype, 1, 1, M, 16, Cout, 1, 100 + M + Cout)


@pytest.mark.parametrize('tail', [1, 7, 8, 9])
def test_conv_stream_parts(dev, tail):
    M = 65536 + tail
    _conv_case('stream M=65536+%d' % tail, dev, bf16, 1, 1, M, 16, 96, 1, 200 + tail, bias=False)


def test_stem_parts(dev):
    _conv_case('stem 2x128', dev, bf16, 1, 2, 128, 3, 32, 3, 300)


def _dw_case(name, dev, dtype, N, H, W, C, stride, seed, one_tile=False):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, H, W, C, generator=g) + 0.3).to(dev, dtype)
    w = (torch.randn(3, 3, C, generator=g) * 0.3).to(dev)
    y, parts = ops.dw3x3(x, w, stride, want_stats=True)
    if one_tile:   # one strip, one column tile per image: P = Wo + halo
        assert parts.shape[0] == N, (name, parts.shape[0])
    _check(name, y, ops.dw3x3(x, w, stride), parts, dev)


# C = 6: no pack divides it, the direct kernel one channel a thread; DW_RB = 8 output rows a block
@pytest.mark.parametrize('dtype', [torch.float32, bf16])
@pytest.mark.parametrize('stride', [1, 2])
def test_dw_direct_parts(dev, dtype, stride):
    for Ho in (7, 8, 9):
        for Wo in (1, 3):
            _dw_case('dw direct s%d Ho=%d Wo=%d %s' % (stride, Ho, Wo, dtype), dev, dtype, 2, Ho * stride,
                     Wo * stride, 6, stride, 400 + Ho * 4 + Wo)


# tile columns P = Wo + halo (2 at stride 1, 1 at stride 2) on maps narrower than a block
def _wo_of(P, stride):
    return P - (2 if stride == 1 else 1)


@pytest.mark.parametrize('dtype', [torch.float32, bf16])
@pytest.mark.parametrize('stride', [1, 2])
def test_dw_lx_parts(dev, dtype, stride):
    for P in (7, 8, 9, 17):
        Wo = _wo_of(P, stride)
        _dw_case('dw lx s%d P=%d %s' % (stride, P, dtype), dev, dtype, 2, 5 * stride, Wo * stride, 16, stride, 500 + P,
                 one_tile=True)
    _dw_case('dw lx s%d one row %s' % (stride, dtype), dev, dtype, 1, stride, 6 * stride, 16, stride, 520, one_tile=True)


def _rc_case(name, dev, N, H, W, Cin, C, stride, seed):
    code = ops.dtcode(torch.empty(1, dtype=bf16))
    assert _abi.lib().rod_dw3x3_fwd_rc_supported(N, H, W, C, Cin, stride, code), name
    g = torch.Generator().manual_seed(seed)
    M = N * H * W
    x = (torch.randn(N, H, W, Cin, generator=g) * 1.4 + 0.1).to(dev, bf16)
    w_e = (torch.randn(C, 1, 1, Cin, generator=g) * 0.3).to(dev)
    wt0 = ops._prep(w_e, 0, bf16, C, Cin, 1)
    ye = torch.empty((1, 1, M, C), dtype=bf16, device=dev)
    ops.conv_fwd_raw(x.view(1, 1, M, Cin), wt0, None, ye, 1, 1, M, Cin, C, 1, None, None)
    yf = ye.float().view(M, C)
    epro = (yf.mean(0), torch.rsqrt(yf.var(0, unbiased=False) + 1e-3), (torch.rand(C, generator=g) + 0.5).to(dev),
            (torch.randn(C, generator=g) * 0.5 + 0.5).to(dev), ops.ROD_ACT_RELU6)
    wd = (torch.randn(3, 3, C, generator=g) * 0.3).to(dev)
    Ho, pt = ops.same_pad(H, stride)
    Wo, pl = ops.same_pad(W, stride)
    nparts = _abi.lib().rod_dw3x3_fwd_stat_parts(N, Ho, Wo, C, stride, code)
    assert nparts == N, (name, nparts)   # one strip, one column tile per image: P = Wo + halo
    outs = []
    for parts in (torch.full((nparts, 3, C), -7.0, device=dev), None):
        y = torch.empty((N, Ho, Wo, C), dtype=bf16, device=dev)
        _abi.call('rod_dw3x3_fwd_rc', x, *ops._pro_args(None), wt0, Cin, *ops._pro_args(epro), wd, y, parts, N, H, W, C,
                  stride, pt, pl, Ho, Wo, code, ops.stream())
        outs.append((y, parts))
    _check(name, outs[0][0], outs[1][0], outs[0][1], dev)


@pytest.mark.parametrize('stride', [1, 2])
def test_dw_rc_parts(dev, stride):
    for P, C in ((7, 96), (8, 96), (9, 96), (17, 48)):
        Wo = _wo_of(P, stride)
        _rc_case('dw rc s%d P=%d C=%d' % (stride, P, C), dev, 2, 5 * stride, Wo * stride, 16, C, stride, 600 + P)
    _rc_case('dw rc s%d one row' % stride, dev, 1, stride, 6 * stride, 24, 144, stride, 620)
