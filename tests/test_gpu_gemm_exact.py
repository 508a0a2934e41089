"""rod_conv_fwd (tiled, split-K, direct-store, streaming and stem forms), the same entry with mode-1
weights as backward-data, and rod_conv_wgrad with its bias column sum, pinned to float64 EXACTLY at
their tile edges.

The operands are small integers (tests/gemm_ref.py), so an honest implementation is bit-identical
to the float64 reference under any summation order, tile shape or split count: every assertion
here is torch.equal or a guard check, with no tolerance anywhere.  Each case first asserts, from
the dispatch plan restated in gemm_ref and the library's queries, the kernel form it means to hit.
Outputs and workspaces of the direct ABI calls are guarded allocations of exactly the documented
size; the public path (ops.conv2d forward and backward) runs beside them wherever it reaches the
form.

rod_common.h's from_f32 is a plain float -> bf16 conversion (round to nearest even), which is what
the reference's single final rounding uses.
"""
import pytest
import torch

import gemm_ref as gr
from gemm_ref import BF16, F32
from rod import _abi, ops

pytestmark = pytest.mark.gpu

DT = {BF16: torch.bfloat16, F32: torch.float32}


def _id(c):
    return '-'.join('x'.join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c)


def _same(got, want, what, cols_per_tile=128):
    """torch.equal with the mismatching (row, channel) pattern in the failure message."""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    g2, w2 = got.reshape(-1, got.shape[-1]).float(), want.reshape(-1, want.shape[-1]).float()
    bad = (g2 != w2).nonzero()
    rows, cols = sorted(set(bad[:, 0].tolist())), sorted(set(bad[:, 1].tolist()))
    first = [(r, c, float(g2[r, c]), float(w2[r, c])) for r, c in bad[:8].tolist()]
    raise AssertionError(
        f'{what}: {len(bad)} of {g2.numel()} differ; rows {rows[:24]} ({len(rows)}; 128-row tiles '
        f'{sorted(set(r // 128 for r in rows))[:8]}, 32-row steps {sorted(set(r // 32 for r in rows))[:8]}), '
        f'cols {cols[:24]} ({len(cols)}; {cols_per_tile}-col tiles {sorted(set(c // cols_per_tile for c in cols))[:8]}); '
        f'first (row, col, got, want): {first}')


def _pro_dev(pro, dev):
    if pro is None:
        return None
    mean, rstd, gamma, beta, act = pro
    return (mean.to(dev), rstd.to(dev), gamma.to(dev), beta.to(dev), act)


def _prep(G, dev, w, mode, dtype):
    """rod_conv_weight_prep into a guarded operand; the layout and the values must be exact."""
    Cout, ks, _, Cin = w.shape
    wd = w.to(dev).contiguous()
    wt = G.alloc(w.numel(), dtype, f'wt{mode}')
    _abi.call('rod_conv_weight_prep', wd, wt, Cout, Cin, ks, mode, ops.dtcode(wt), ops.stream())
    torch.cuda.synchronize()
    assert torch.equal(wt.cpu().float(), gr.prep_reference(w, mode).reshape(-1)), f'weight_prep mode {mode}'
    return wt


def abi_forward(G, dev, dt, case, bias, mode=0, use_ws=True, stats=False, dldx=0, dldy=0, xoff=0, yoff=0):
    """rod_conv_fwd by a direct call on guarded buffers -> y [M][Cout] on the CPU.  mode 1: the
    backward-data form (dy in, mode-1 weights, Cin and Cout swapped, no bias or prologue) -> dx."""
    N, H, W, Cin, Cout, ks = case.geo
    dtype, M = DT[dt], case.M
    src, ci, co, pro = (case.x, Cin, Cout, case.pro) if mode == 0 else (case.dy, Cout, Cin, None)
    assert not (mode == 1 and bias)
    ldx, ldy = ci + dldx, co + dldy
    x = G.rows(src.reshape(M, ci).to(dtype), ldx, 'x', xoff)
    wt = _prep(G, dev, case.w, mode, dtype)
    b = case.bias.to(dev) if bias else None
    yflat, y = G.out_rows(M, co, ldy, dtype, 'dx' if mode else 'y', yoff)
    nb = _abi.query('rod_conv_fwd_workspace', N, H, W, ci, co, ks)
    assert nb == gr.fwd_workspace_bytes(N, H, W, ci, co, ks)
    ws = G.alloc(nb // 4, torch.float32, 'fwd workspace') if (use_ws and nb) else None
    parts = G.alloc(gr.cdiv(M, 128) * 3 * co, torch.float32, 'stat parts') if stats else None
    prod = _pro_dev(pro, dev)
    _abi.call('rod_conv_fwd', x, *ops._pro_args(prod), wt, b, yflat, ws, parts, *ops._gred_args(None), N, H, W, ci, co,
              ks, ldx if dldx else 0, ldy if dldy else 0, ops.dtcode(yflat), ops.stream())
    torch.cuda.synchronize()
    assert gr.gaps_untouched(yflat, M, co, ldy), 'columns between Cout and ldy were written'
    return y.cpu()


def abi_wgrad(G, dev, dt, case, dldx=0, dldy=0, xoff=0, doff=0):
    """rod_conv_wgrad by a direct call on guarded buffers -> (dw [Cout,ks,ks,Cin], db [Cout]) on the CPU."""
    N, H, W, Cin, Cout, ks = case.geo
    dtype, M = DT[dt], case.M
    ldx, lddy = Cin + dldx, Cout + dldy
    x = G.rows(case.x.reshape(M, Cin).to(dtype), ldx, 'x', xoff)
    dy = G.rows(case.dy.reshape(M, Cout).to(dtype), lddy, 'dy', doff)
    dw = G.alloc(Cout * case.K, torch.float32, 'dw')
    db = G.alloc(Cout, torch.float32, 'db')
    nb = _abi.query('rod_conv_wgrad_workspace', N, H, W, Cin, Cout, ks)
    assert nb == gr.wgrad_workspace_bytes(N, H, W, Cin, Cout, ks)
    ws = G.alloc(nb // 4, torch.float32, 'wgrad workspace')
    prod = _pro_dev(case.pro, dev)
    _abi.call('rod_conv_wgrad', x, *ops._pro_args(prod), dy, dw, db, ws, N, H, W, Cin, Cout, ks, ldx if dldx else 0,
              lddy if dldy else 0, ops.dtcode(x), ops.stream())
    torch.cuda.synchronize()
    return dw.cpu().view(Cout, ks, ks, Cin), db.cpu()


def ops_conv(G, dev, dt, case, bias, want_stats=False, backward=False):
    """The public path: ops.conv2d (a Pending input for the prologue) and, on request, its backward
    with the parameters' gradient slots guarded -> dict(y[, dx, dw, db]) on the CPU."""
    N, H, W, Cin, Cout, ks = case.geo
    dtype = DT[dt]
    xd = case.x.to(dev, dtype).requires_grad_(backward)
    wd = case.w.to(dev).requires_grad_(True)
    wd._rod_grad = G.alloc(case.w.numel(), torch.float32, 'ops dw').view(case.w.shape)
    bd = None
    if bias:
        bd = case.bias.to(dev).requires_grad_(True)
        bd._rod_grad = G.alloc(Cout, torch.float32, 'ops db')
    xin = xd
    if case.pro is not None:
        assert not backward   # the public backward continues through the BatchNorm: not this GEMM alone
        mean, rstd, gamma, beta, act = _pro_dev(case.pro, dev)
        xin = ops.Pending(xd, mean, rstd, gamma, beta, act, False)
    y = ops.conv2d(xin, wd, bd, ks, want_stats)
    if want_stats:
        y = y[0]
    out = dict(y=y.detach().reshape(case.M, Cout).cpu())
    if backward:
        y.backward(case.dy.to(dev, dtype))
        torch.cuda.synchronize()
        out.update(dx=xd.grad.reshape(case.M, Cin).cpu(), dw=wd._rod_grad.cpu(), db=bd._rod_grad.cpu() if bias else None)
    return out


def _want(ref, key, dt, case):
    t = ref[key]
    if key in ('y', 'dx'):
        return t.reshape(case.M, -1).to(DT[dt])   # one rounding to nearest even (bf16), none for fp32
    return t


def check_forward(dev, dt, case, path, use_ws=True, biases=(False, True), stats=False, public=True, **ld):
    """Every bias setting through the direct call (and the public path): y == float64 reference."""
    G = gr.Guarded(dev)
    bn = path.get('bn', 128)
    for bias in biases:
        ref = gr.reference(case, bias=bias, grads=False)
        want = _want(ref, 'y', dt, case)
        y = abi_forward(G, dev, dt, case, bias, use_ws=use_ws, **ld)
        _same(y, want, f'y (direct call, bias={bias}, {path})', bn)
        if stats:
            ys = abi_forward(G, dev, dt, case, bias, use_ws=use_ws, stats=True, **ld)
            _same(ys, y, f'y with statistics vs plain y (bias={bias})', bn)
            _same(ys, want, f'y with statistics (bias={bias})', bn)
        if public:
            _same(ops_conv(G, dev, dt, case, bias)['y'], want, f'y (ops.conv2d, bias={bias})', bn)
            if stats:
                _same(ops_conv(G, dev, dt, case, bias, want_stats=True)['y'], want, f'y (ops.conv2d stats, bias={bias})', bn)
    G.check()


def check_wgrad(dev, dt, case, **ld):
    G = gr.Guarded(dev)
    ref = gr.reference(case, bias=True)
    dw, db = abi_wgrad(G, dev, dt, case, **ld)
    _same(dw.reshape(case.geo[4], -1), ref['dw'].reshape(case.geo[4], -1), 'dw (rows co, cols k)', 64)
    _same(db.reshape(1, -1), ref['db'].reshape(1, -1), 'db', 256)
    G.check()
    return ref


# ---------------------------------------------------------------- 1: tiled vector form
@pytest.mark.parametrize('c', gr.CLASS1, ids=_id)
def test_fwd_tiled_vector(dev, c):
    dt, nhw, ci, co = c
    case = gr.Case(*nhw, ci, co, 1)
    path = gr.fwd_path(dt == BF16, *nhw, ci, co, 1, bias=True)
    assert path['kernel'] == 'tiled' and path['form'] == 'vector', path
    assert _abi.query('rod_conv_fwd_workspace', *nhw, ci, co, 1) == 0
    assert _abi.lib().rod_conv_fwd_stream_ok(case.M, ci, co, ops.dtcode(torch.empty(0, dtype=DT[dt]))) == 0
    check_forward(dev, dt, case, path, stats=True)


# ---------------------------------------------------------------- 2: direct-store form
@pytest.mark.parametrize('c', gr.CLASS2, ids=_id)
def test_fwd_direct_store(dev, c):
    dt, nhw, ks, ci, co = c
    case = gr.Case(*nhw, ci, co, ks)
    path = gr.fwd_path(dt == BF16, *nhw, ci, co, ks, ws=False, bias=True)
    assert path['kernel'] == 'tiled' and path['form'] == 'direct', path
    # the public path reaches the form only where the plan does not split: without a workspace here
    public = gr.fwd_path(dt == BF16, *nhw, ci, co, ks, ws=True, bias=True) == path
    check_forward(dev, dt, case, path, use_ws=False, public=public)


# ---------------------------------------------------------------- 3: split-K
@pytest.mark.parametrize('c', gr.CLASS3, ids=_id)
def test_fwd_split_k(dev, c):
    dt, nhw, ks, ci, co, pa = c
    case = gr.Case(*nhw, ci, co, ks, pro_act=pa)
    path = gr.fwd_path(dt == BF16, *nhw, ci, co, ks, pro=pa, bias=True)
    assert path['kernel'] == 'split' and path['splits'] > 1, path
    assert _abi.query('rod_conv_fwd_workspace', *nhw, ci, co, ks) == path['splits'] * case.M * co * 4
    flat = gr.fwd_path(dt == BF16, *nhw, ci, co, ks, pro=pa, bias=True, ws=False)
    assert flat['kernel'] == 'tiled', flat
    G = gr.Guarded(dev)
    for bias in (False, True):
        want = _want(gr.reference(case, bias=bias, grads=False), 'y', dt, case)
        y_split = abi_forward(G, dev, dt, case, bias, use_ws=True)
        y_flat = abi_forward(G, dev, dt, case, bias, use_ws=False)
        _same(y_split, want, f'y split-K (bias={bias}, {path})')
        _same(y_flat, want, f'y unsplit (bias={bias}, {flat})', flat['bn'])
        _same(y_split, y_flat, 'split-K vs unsplit')
        _same(ops_conv(G, dev, dt, case, bias)['y'], want, f'y (ops.conv2d, bias={bias})')
    G.check()


# ---------------------------------------------------------------- 4: 3x3 borders
@pytest.mark.parametrize('c', gr.CLASS4, ids=_id)
def test_fwd_3x3_borders(dev, c):
    ci, co, pa = c
    for nhw in gr.C4_MAPS:
        case = gr.Case(*nhw, ci, co, 3, pro_act=pa)
        path = gr.fwd_path(True, *nhw, ci, co, 3, pro=pa, bias=True)
        assert path['kernel'] == ('split' if ci == 36 else 'tiled'), path
        assert path['va'] == (ci % 8 == 0) and path['vy'] == (co % 8 == 0)
        check_forward(dev, BF16, case, path)
        if path['kernel'] == 'split':   # and the unsplit kernel on the same shape
            flat = gr.fwd_path(True, *nhw, ci, co, 3, pro=pa, bias=True, ws=False)
            check_forward(dev, BF16, case, flat, use_ws=False, public=False)


# ---------------------------------------------------------------- 5: stem forms
@pytest.mark.parametrize('c', gr.CLASS5, ids=_id)
def test_fwd_stem(dev, c):
    dt, nhw, co = c
    case = gr.Case(*nhw, 3, co, 3)
    path = gr.fwd_path(dt == BF16, *nhw, 3, co, 3, bias=True)
    fused = gr.fwd_path(dt == BF16, *nhw, 3, co, 3, bias=True, stats=True)
    if dt == BF16 and co == 32:
        assert path['kernel'] == 'stem_mfma' and fused['kernel'] == 'stem_mfma', path
        assert fused['fuse'] == (nhw[2] % 128 == 0)
    else:
        assert path['kernel'] == 'stem_valu' and path['co'] == co, path
    check_forward(dev, dt, case, path, stats=True)


# ---------------------------------------------------------------- 6: streaming 1x1
@pytest.mark.parametrize('c', gr.CLASS6, ids=_id)
def test_fwd_streaming(dev, c):
    M, K, co, pa = c
    case = gr.Case(1, 1, M, K, co, 1, pro_act=pa)
    path = gr.fwd_path(True, 1, 1, M, K, co, 1, pro=pa)
    ok = _abi.lib().rod_conv_fwd_stream_ok(M, K, co, _abi.ROD_BF16)
    assert ok == gr.stream_ok(M, K, co, True)
    if (K, co) == (64, 80):
        assert ok == 0 and path['kernel'] == 'tiled'        # no group width divides 80: the tiled kernel
    elif (K, co) == (8, 16):
        assert ok == 0 and path['kernel'] == 'tiled'        # one 16-wide tile is below the narrowest group
    elif (K, co) == (40, 24):
        assert path['kernel'] == 'proj' and (path['kt'], path['nt']) == (2, 2), path
    else:
        assert ok == 1 and path['kernel'] == 'stream', path
    assert _abi.query('rod_conv_fwd_workspace', 1, 1, M, K, co, 1) == 0
    check_forward(dev, BF16, case, path, biases=(False,))


# ---------------------------------------------------------------- 7: backward-data (and the rest) through ops
@pytest.mark.parametrize('c', gr.CLASS7, ids=_id)
def test_backward_through_ops(dev, c):
    dt, nhw, ks, ci, co = c
    case = gr.Case(*nhw, ci, co, ks)
    bwd = gr.fwd_path(dt == BF16, *nhw, co, ci, ks)     # mode-1 weights: Cin and Cout swapped
    assert bwd['kernel'] in ('tiled', 'split'), bwd
    assert _abi.query('rod_conv_fwd_workspace', *nhw, co, ci, ks) == \
        (bwd['splits'] * case.M * ci * 4 if bwd['kernel'] == 'split' else 0)
    ref = gr.reference(case, bias=True)
    G = gr.Guarded(dev)
    got = ops_conv(G, dev, dt, case, True, backward=True)
    _same(got['y'], _want(ref, 'y', dt, case), 'y (ops.conv2d)')
    _same(got['dx'], _want(ref, 'dx', dt, case), f'dx (ops.conv2d backward, {bwd})', bwd.get('bn', 128))
    _same(got['dw'].reshape(co, -1), ref['dw'].reshape(co, -1), 'dw (ops.conv2d backward)', 64)
    _same(got['db'].reshape(1, -1), ref['db'].reshape(1, -1), 'db (ops.conv2d backward)', 256)
    # the same backward-data GEMM on guarded buffers, with and without its workspace
    want = _want(ref, 'dx', dt, case)
    _same(abi_forward(G, dev, dt, case, False, mode=1), want, 'dx (direct call)', bwd.get('bn', 128))
    if bwd['kernel'] == 'split':
        _same(abi_forward(G, dev, dt, case, False, mode=1, use_ws=False), want, 'dx (direct call, unsplit)')
    G.check()


# ---------------------------------------------------------------- 8: weight and bias gradient
@pytest.mark.parametrize('c', gr.CLASS8, ids=_id)
def test_wgrad(dev, c):
    dt, nhw, ks, ci, co, pa = c
    case = gr.Case(*nhw, ci, co, ks, pro_act=pa)
    path = gr.wgrad_path(dt == BF16, *nhw, ci, co, ks, pro=pa)
    if ks == 3 and ci == 3:
        assert path['kernel'] == ('stem_wgrad' if dt == BF16 and co == 32 else 'wgrad_cin3'), path
    else:
        assert path['kernel'] == 'wgrad' and path['va'] == (ks == 1 or ci % 8 == 0), path
        assert path['vd'] == (co % gr.vec_elems(dt == BF16) == 0)
        if (case.M, ci, co) == (1025, 72, 72):
            assert (path['natural'], path['splits'], path['xcd']) == (9, 16, True)
    ref = check_wgrad(dev, dt, case)
    if pa is None:    # the public path writes the same gradients into the parameters' slots
        G = gr.Guarded(dev)
        got = ops_conv(G, dev, dt, case, True, backward=True)
        _same(got['dw'].reshape(co, -1), ref['dw'].reshape(co, -1), 'dw (ops.conv2d backward)', 64)
        _same(got['db'].reshape(1, -1), ref['db'].reshape(1, -1), 'db (ops.conv2d backward)', 256)
        G.check()


# ---------------------------------------------------------------- 9: leading dimensions, unaligned bases
@pytest.mark.parametrize('c', gr.CLASS9, ids=_id)
def test_leading_dimensions(dev, c):
    dt, nhw, ks, ci, co, dlx, dly, xo, yo = c
    bf = dt == BF16
    ev = gr.vec_elems(bf)
    case = gr.Case(*nhw, ci, co, ks)
    for use_ws in (True, False):
        path = gr.fwd_path(bf, *nhw, ci, co, ks, ldx=ci + dlx, ldy=co + dly, ax=not xo, ay=not yo, ws=use_ws, bias=True)
        assert path['va'] == (xo == 0 and (ci + dlx) % ev == 0 and (ks == 1 or ci % 8 == 0)), path
        assert path['vy'] == (yo == 0 and (co + dly) % ev == 0), path
        if path['kernel'] == 'tiled':
            assert path['form'] == ('vector' if path['va'] and path['vb'] and path['vy'] else 'direct')
        if use_ws and path['kernel'] != 'split':
            continue     # no split plan: one run covers it
        check_forward(dev, dt, case, path, use_ws=use_ws, public=False, dldx=dlx, dldy=dly, xoff=xo, yoff=yo)
    wp = gr.wgrad_path(bf, *nhw, ci, co, ks, ldx=ci + dlx, lddy=co + dly, ax=not xo, ad=not yo)
    assert wp['kernel'] == 'wgrad' and wp['va'] == path['va'] and wp['vd'] == path['vy'], wp
    check_wgrad(dev, dt, case, dldx=dlx, dldy=dly, xoff=xo, doff=yo)
