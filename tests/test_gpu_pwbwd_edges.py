"""The fused 1x1 backwards (rod_pw_bwd, _rc, _gred, _gred_rc, _gred_dyp) at the edges of their
32-row tile bookkeeping, every kernel form at every row count of ROWS: below a 16-row half, exactly
a half, a half plus a row, a tile, a tile plus a row, more tiles than one block's four waves, and
several blocks with a ragged tail.  The oracle is the unfused chain of test_gpu_pwbwd.py
(pwbwd_ref.unfused_chain) with its bars: dx bit-identical, dw / db 1e-5 normwise, the input
BatchNorm's sums 1e-5 against float64 sums over the kernel's own dx.  Each case asserts the
dispatch it means to hit from the library's queries and the shape rules of pwbwd.hip."""
import os
import sys

import pytest
import torch

from rod import _abi, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pwbwd_ref import nerr, unfused_chain, xsums64  # noqa: E402

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
NONE, RELU6, LEAKY = ops.ROD_ACT_NONE, ops.ROD_ACT_RELU6, ops.ROD_ACT_LEAKY

ROWS = [1, 15, 16, 17, 31, 32, 33, 129, 4 * 32 * 3 + 5]
FWD_ROWS = 65536   # the streaming forward's smallest M: the y the recompute forms reproduce


def _cdiv(a, b):
    return -(-a // b)


def stream_blocks(M):   # pw_bwd_stream_blocks
    return max(1, min(_cdiv(_cdiv(M, 32), 4), 3 * 256))


def gred_rowblocks(M, Cin, nw):   # pw_bwd_gred_rowblocks
    return max(1, min(_cdiv(_cdiv(M, 32), 4), max(1, 768 // (Cin // nw))))


def block_plan(Cin, Cout, bias):   # (nx, wt) of pw_bwd_plan
    nco, nci, nxt = _cdiv(Cout, 16), _cdiv(Cin + (1 if bias else 0), 16), _cdiv(Cin, 16)
    nx = 2 if nxt <= 2 else 4 if nxt <= 4 else 8 if nxt <= 8 else 12
    per = _cdiv(nco * nci, 4)
    return nx, 4 if per <= 4 else 6 if per <= 6 else 8 if per <= 8 else 16


def _streams(M, Cin, Cout):
    return bool(_abi.lib().rod_pw_bwd_rc_supported(M, Cin, Cout, ops.dtcode(torch.empty(1, dtype=bf16))))


def test_row_counts_cover_more_than_one_block():
    """The last two row counts give every streaming / column-grouped launch more than one block
    (and the one before them a single block with all four waves busy)."""
    for M, more in zip(ROWS, [False] * 7 + [True, True]):
        assert (stream_blocks(M) > 1) == more
        assert ops.pw_bwd_gred_parts(M, 16, 96, bf16) == stream_blocks(M)
        for Cin, Cout, nw in ((32, 16, 32), (64, 64, 32), (144, 24, 48), (96, 24, 32)):
            assert (gred_rowblocks(M, Cin, nw) > 1) == more
            assert ops.pw_bwd_gred_parts(M, Cin, Cout, bf16) == gred_rowblocks(M, Cin, nw)
    assert _cdiv(ROWS[6], 32) <= 4 < _cdiv(ROWS[7], 32)


def _bn(C, g, dev):
    return ((torch.randn(C, generator=g) * 0.2).to(dev), (torch.rand(C, generator=g) + 0.5).to(dev),
            (torch.rand(C, generator=g) + 0.5).to(dev), (torch.randn(C, generator=g) * 0.2).to(dev))


def _case(dev, M, Cin, Cout, act, xact, seed, forward_y=False, dz_shift=0.0):
    """Inputs of one backward; forward_y: y is the expand output the streaming forward stores for
    these rows (the first M of a FWD_ROWS-row launch), else random."""
    g = torch.Generator().manual_seed(seed * 1000 + M)
    x = (torch.randn(M, Cin, generator=g) * 1.5 + 0.3).to(dev, bf16)
    w = (torch.randn(Cout, 1, 1, Cin, generator=g) * 0.25).to(dev)
    xpro = None if xact is None else (*_bn(Cin, g, dev), xact)
    wt0 = ops._prep(w, 0, bf16, Cout, Cin, 1)
    if forward_y:
        R = max(M, FWD_ROWS)
        xp = torch.zeros(R, Cin, dtype=bf16, device=dev)
        xp[:M] = x
        yp = torch.empty((1, 1, R, Cout), dtype=bf16, device=dev)
        ops.conv_fwd_raw(xp.view(1, 1, R, Cin), wt0, None, yp, 1, 1, R, Cin, Cout, 1, None, xpro)
        y = yp.view(R, Cout)[:M].contiguous()
    else:
        y = (torch.randn(M, Cout, generator=g) * 2 + 0.5).to(dev, bf16)
    dz = torch.randn(M, Cout, generator=g).to(dev, bf16)
    mean = y.float().mean(0)
    rstd = torch.rsqrt(y.float().var(0, unbiased=False) + 1e-3)
    gamma = (torch.rand(Cout, generator=g) + 0.5).to(dev) if act != LEAKY else None
    beta = (torch.randn(Cout, generator=g) * 0.3).to(dev)
    coef = ops.bn_bwd_reduce(dz, y, mean, rstd, gamma, beta, act, False, False)
    if dz_shift:
        # The bias gradient is the column sum of dy, and with the coefficients of this very dz the
        # BatchNorm backward makes that sum cancel to the bf16 rounding residue of dy: its fp32
        # summation error (~n 2^-24 sum|dy|) is then as large as the value, and the normwise bar
        # would compare noise with noise.  The apply takes the coefficients as an input, so the
        # backward is run on dz + shift with the coefficients of dz: sum dy ~ n a shift, against
        # which 1e-5 is a real bar.  Both the chain and the fused kernel see the same inputs.  The
        # BatchNorm-consistent bias path (coefficients of the applied dz) is test_gpu_pwbwd.py's
        # 64 -> 128 and 96 -> 128 cases.
        dz = (dz.float() + dz_shift).to(bf16)
    wt1 = ops._prep(w, 1, bf16, Cout, Cin, 1)
    return dict(bn=(dz, y, mean, rstd, gamma, beta, act, coef), x=x, xpro=xpro, wt1=wt1, wt0=wt0)


STREAM = [  # (Cin, Cout, input prologue act or None, dx wanted)
    pytest.param(16, 96, None, True, id='pro_off'),
    pytest.param(24, 144, RELU6, True, id='pro_relu6'),
    pytest.param(16, 96, NONE, True, id='pro_xl'),
    pytest.param(16, 96, None, False, id='no_dx'),
]


@pytest.mark.parametrize('M', ROWS)
@pytest.mark.parametrize('Cin,Cout,xact,want_dx', STREAM)
def test_stream_forms(dev, M, Cin, Cout, xact, want_dx):
    assert ops.pw_bwd_supported(Cin, Cout, bf16) and _streams(M, Cin, Cout)
    c = _case(dev, M, Cin, Cout, RELU6, xact, 1)
    _, dx_ref, dw_ref, _ = unfused_chain(*c['bn'], c['x'], c['xpro'], c['wt1'])
    dw = torch.full((Cout, Cin), float('nan'), device=dev)
    dx = ops.pw_bwd(*c['bn'], c['x'], c['xpro'], c['wt1'], want_dx, dw, None)
    if want_dx:
        assert torch.equal(dx, dx_ref), nerr(dx.float(), dx_ref.float())
    else:
        assert dx is None
    assert nerr(dw, dw_ref) < 1e-5, nerr(dw, dw_ref)


@pytest.mark.parametrize('M', ROWS)
@pytest.mark.parametrize('Cin,Cout,xact', [pytest.param(16, 96, NONE, id='16x96'), pytest.param(24, 144, None, id='24x144')])
def test_stream_rc_against_stored_y(dev, M, Cin, Cout, xact):
    assert _streams(M, Cin, Cout)
    c = _case(dev, M, Cin, Cout, RELU6, xact, 2, forward_y=True)
    outs = []
    for rc in (False, True):
        dw = torch.full((Cout, Cin), float('nan'), device=dev)
        dx = ops.pw_bwd(*c['bn'], c['x'], c['xpro'], c['wt1'], True, dw, None, wt0=c['wt0'] if rc else None)
        outs.append((dx, dw))
    (dx0, dw0), (dx1, dw1) = outs
    assert torch.equal(dx0, dx1), nerr(dx1.float(), dx0.float())
    assert torch.equal(dw0, dw1), nerr(dw1, dw0)


@pytest.mark.parametrize('M', ROWS)
@pytest.mark.parametrize('xact', [pytest.param(NONE, id='xl'), pytest.param(RELU6, id='relu6')])
def test_stream_xg_forms(dev, M, xact):
    """The 16 -> 96 expand with the input BatchNorm's sums, y read and y recomputed."""
    Cin, Cout = 16, 96
    nparts = ops.pw_bwd_gred_parts(M, Cin, Cout, bf16)
    assert _streams(M, Cin, Cout) and nparts == stream_blocks(M)
    c = _case(dev, M, Cin, Cout, RELU6, xact, 3, forward_y=True)
    _, dx_ref, dw_ref, _ = unfused_chain(*c['bn'], c['x'], c['xpro'], c['wt1'])
    outs = []
    for rc in (False, True):
        dw = torch.full((Cout, Cin), float('nan'), device=dev)
        dx, xparts = ops.pw_bwd_gred(*c['bn'], c['x'], c['xpro'], c['wt1'], dw, wt0=c['wt0'] if rc else None)
        assert xparts.shape == (nparts, 2, Cin)
        assert torch.equal(dx, dx_ref), (rc, nerr(dx.float(), dx_ref.float()))
        assert nerr(dw, dw_ref) < 1e-5, (rc, nerr(dw, dw_ref))
        s_g, s_gx = xsums64(dx, c['x'], c['xpro'])
        p = xparts.double().sum(0)
        assert nerr(p[0], s_g) < 1e-5, (rc, nerr(p[0], s_g))
        assert nerr(p[1], s_gx) < 1e-5, (rc, nerr(p[1], s_gx))
        outs.append((dx, dw, xparts))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


GRED = [  # (Cin, Cout, output BatchNorm act, group width): FAST = linear output, ReLU6 input, 32 columns
    pytest.param(32, 16, NONE, 32, id='fast'),
    pytest.param(64, 64, NONE, 32, id='fast_kt2'),
    pytest.param(144, 24, NONE, 48, id='elem_nw48'),
    pytest.param(96, 24, LEAKY, 32, id='elem_leaky'),
]


@pytest.mark.parametrize('M', ROWS)
@pytest.mark.parametrize('Cin,Cout,act,nw', GRED)
def test_gred_forms_and_dyp(dev, M, Cin, Cout, act, nw):
    """The column-grouped kernel: dx form against the unfused chain, dyp form against dy and the
    dx form's dw / sums bit for bit."""
    assert Cin != 16 and (nw == 32) == (Cin % 32 == 0) and Cin % nw == 0   # pw_bwd_gred_nw, not the expand form
    nparts = ops.pw_bwd_gred_parts(M, Cin, Cout, bf16)
    assert nparts == gred_rowblocks(M, Cin, nw)
    c = _case(dev, M, Cin, Cout, act, RELU6, 4)
    dy, dx_ref, dw_ref, _ = unfused_chain(*c['bn'], c['x'], c['xpro'], c['wt1'])
    dw = torch.full((Cout, Cin), float('nan'), device=dev)
    dx, xparts = ops.pw_bwd_gred(*c['bn'], c['x'], c['xpro'], c['wt1'], dw)
    assert xparts.shape == (nparts, 2, Cin)
    assert torch.equal(dx, dx_ref), nerr(dx.float(), dx_ref.float())
    assert nerr(dw, dw_ref) < 1e-5, nerr(dw, dw_ref)
    s_g, s_gx = xsums64(dx, c['x'], c['xpro'])
    p = xparts.double().sum(0)
    assert nerr(p[0], s_g) < 1e-5, nerr(p[0], s_g)
    assert nerr(p[1], s_gx) < 1e-5, nerr(p[1], s_gx)
    dw2 = torch.full((Cout, Cin), float('nan'), device=dev)
    dyp, xparts2 = ops.pw_bwd_gred(*c['bn'], c['x'], c['xpro'], c['wt1'], dw2, dyp=True)
    assert torch.equal(dyp, dy), nerr(dyp.float(), dy.float())
    assert torch.equal(dw2, dw) and torch.equal(xparts2, xparts)


BLOCK = [  # (Cin, Cout, act, input prologue act or None, bias, weight tiles per wave)
    pytest.param(64, 128, LEAKY, None, True, 16, id='bias_nci5'),    # Cin + 1 = 65: the ones column opens a fifth tile
    pytest.param(32, 64, NONE, RELU6, False, 4, id='wt4'),
    pytest.param(32, 192, RELU6, RELU6, False, 6, id='32x192'),
    pytest.param(96, 128, LEAKY, LEAKY, False, 16, id='wt16'),
]


@pytest.mark.parametrize('M', ROWS)
@pytest.mark.parametrize('Cin,Cout,act,xact,bias,wt', BLOCK)
def test_block_kernel_forms(dev, M, Cin, Cout, act, xact, bias, wt):
    assert ops.pw_bwd_supported(Cin, Cout, bf16) and not _streams(M, Cin, Cout)
    assert block_plan(Cin, Cout, bias)[1] == wt
    c = _case(dev, M, Cin, Cout, act, xact, 5, dz_shift=0.5 if bias else 0.0)
    _, dx_ref, dw_ref, db_ref = unfused_chain(*c['bn'], c['x'], c['xpro'], c['wt1'], bias)
    dw = torch.full((Cout, Cin), float('nan'), device=dev)
    db = torch.full((Cout,), float('nan'), device=dev) if bias else None
    dx = ops.pw_bwd(*c['bn'], c['x'], c['xpro'], c['wt1'], True, dw, db)
    assert torch.equal(dx, dx_ref), nerr(dx.float(), dx_ref.float())
    assert nerr(dw, dw_ref) < 1e-5, nerr(dw, dw_ref)
    if bias:
        assert nerr(db, db_ref) < 1e-5, nerr(db, db_ref)
