"""CPU checks of tests/gemm_ref.py: the float64 reference against an explicit im2col matmul, the
exactness bound of every parametrised case, the restated dispatch plan against the library's
host-only queries, and that the case tables of test_gpu_gemm_exact.py contain the dispatch classes
they claim."""
import pytest
import torch

import gemm_ref as gr
from gemm_ref import BF16, F32
from rod import _abi


def _all_cases():
    """(N, H, W, Cin, Cout, ks, pro_act) of every case of every class."""
    out = []
    out += [(*nhw, ci, co, 1, None) for (_, nhw, ci, co) in gr.CLASS1]
    out += [(*nhw, ci, co, ks, None) for (_, nhw, ks, ci, co) in gr.CLASS2]
    out += [(*nhw, ci, co, ks, pa) for (_, nhw, ks, ci, co, pa) in gr.CLASS3]
    out += [(*nhw, ci, co, 3, pa) for (ci, co, pa) in gr.CLASS4 for nhw in gr.C4_MAPS]
    out += [(*nhw, 3, co, 3, None) for (_, nhw, co) in gr.CLASS5]
    out += [(1, 1, M, K, co, 1, pa) for (M, K, co, pa) in gr.CLASS6]
    out += [(*nhw, ci, co, ks, None) for (_, nhw, ks, ci, co) in gr.CLASS7]
    out += [(*nhw, ci, co, ks, pa) for (_, nhw, ks, ci, co, pa) in gr.CLASS8]
    out += [(*c[1], c[3], c[4], c[2], None) for c in gr.CLASS9]
    return sorted(set(out), key=lambda t: tuple(-1 if v is None else v for v in t))


ALL = _all_cases()


@pytest.mark.parametrize('geo,pro', [((2, 3, 5, 5, 7, 3), None), ((3, 2, 1, 8, 4, 3), gr.ACT_RELU6),
                                     ((1, 4, 3, 6, 5, 1), gr.ACT_NONE)])
def test_reference_equals_im2col_matmul(geo, pro):
    c = gr.Case(*geo, pro_act=pro, seed=1)
    for bias in (False, True):
        ref = gr.reference(c, bias=bias)
        assert torch.equal(ref['y'].double(), gr.im2col_matmul(c, bias=bias))
    # the gradients against the same im2col: dw = dy^T A, db = column sums of dy
    N, H, W, Cin, Cout, ks = geo
    nb = gr.Case(*geo, pro_act=pro, seed=1)
    nb.w, nb.bias = torch.zeros_like(c.w), torch.zeros_like(c.bias)
    dyf = c.dy.double().reshape(-1, Cout)
    assert torch.equal(ref['db'].double(), dyf.sum(0))
    for co in range(Cout):   # A's columns one at a time: y of a one-hot weight is the im2col column
        for k in range(0, ks * ks * Cin, max(1, ks * ks * Cin // 5)):
            nb.w.zero_()
            nb.w.view(Cout, -1)[co, k] = 1.0
            col = gr.im2col_matmul(nb, bias=False).reshape(-1, Cout)[:, co]
            assert float(ref['dw'].view(Cout, -1)[co, k]) == float((dyf[:, co] * col).sum())
    if pro is not None:   # the prologue's border: a padded tap contributes 0, not act(beta)
        assert float(c.pro[3].abs().min()) >= 1


def test_prep_reference_layouts():
    w = torch.arange(4 * 3 * 3 * 5, dtype=torch.float32).reshape(4, 3, 3, 5)
    w1 = gr.prep_reference(w, 1).reshape(5, 3, 3, 4)
    for ci in range(5):
        for i in range(3):
            for j in range(3):
                for co in range(4):
                    assert w1[ci, i, j, co] == w[co, 2 - i, 2 - j, ci]
    assert torch.equal(gr.prep_reference(w, 0), w.reshape(4, 45))


def test_exactness_bound_of_every_case():
    assert len(ALL) > 150
    for (N, H, W, Cin, Cout, ks, pa) in ALL:
        M, K = N * H * W, ks * ks * Cin
        amax = 3 if pa is None else 6 if pa == gr.ACT_RELU6 else 8
        bound = 3 * amax * max(K, M, ks * ks * Cout) + 8
        assert bound < gr.EXACT // 4, (N, H, W, Cin, Cout, ks, pa, bound)
        if M < 4096:   # the tensors themselves only for the small cases
            c = gr.Case(N, H, W, Cin, Cout, ks, pro_act=pa)
            assert c.bound() == bound
            assert float(c.conv_input().abs().max()) <= amax
            for t in (c.x, c.w, c.dy, c.bias):
                assert torch.equal(t, t.round()) and torch.equal(t.bfloat16().float(), t)
            assert float(c.bias.abs().max()) <= 8 and float(c.x.abs().max()) <= 3


def test_plan_agrees_with_library_queries():
    L = _abi.lib()
    for (N, H, W, Cin, Cout, ks, _) in ALL:
        assert _abi.query('rod_conv_fwd_workspace', N, H, W, Cin, Cout, ks) == \
            gr.fwd_workspace_bytes(N, H, W, Cin, Cout, ks), (N, H, W, Cin, Cout, ks)
        assert _abi.query('rod_conv_wgrad_workspace', N, H, W, Cin, Cout, ks) == \
            gr.wgrad_workspace_bytes(N, H, W, Cin, Cout, ks), (N, H, W, Cin, Cout, ks)
        # backward-data: the same entry with Cin and Cout swapped
        assert _abi.query('rod_conv_fwd_workspace', N, H, W, Cout, Cin, ks) == \
            gr.fwd_workspace_bytes(N, H, W, Cout, Cin, ks)
        for dt, bf in ((0, False), (1, True)):
            assert L.rod_conv_fwd_stream_ok(N * H * W, ks * ks * Cin, Cout, dt) == \
                gr.stream_ok(N * H * W, ks * ks * Cin, Cout, bf)
    # a sweep around the plans' thresholds, beyond the tables
    for M in (1, 127, 128, 129, 1024, 1025, 16384, 65535, 65536, 65613):
        for Cin in (3, 8, 36, 64, 96, 104, 264, 1920):
            for Cout in (12, 16, 32, 80, 96, 144, 264, 576):
                for ks in (1, 3):
                    a = (1, 1, M, Cin, Cout, ks)
                    assert _abi.query('rod_conv_fwd_workspace', *a) == gr.fwd_workspace_bytes(*a), a
                    assert _abi.query('rod_conv_wgrad_workspace', *a) == gr.wgrad_workspace_bytes(*a), a
                    assert L.rod_conv_fwd_stream_ok(M, ks * ks * Cin, Cout, 1) == gr.stream_ok(M, ks * ks * Cin, Cout, True)
    # the stem plan's max(splits, nblk)
    for nhw in ((2, 2, 5), (2, 2, 256), (8, 64, 300), (1, 9, 129)):
        a = (*nhw, 3, 32, 3)
        assert _abi.query('rod_conv_wgrad_workspace', *a) == gr.wgrad_workspace_bytes(*a), a


def _fwd(dt, nhw, ks, ci, co, **kw):
    return gr.fwd_path(dt == BF16, *nhw, ci, co, ks, **kw)


def test_class1_table_contains_its_tile_classes():
    paths = [(_fwd(dt, nhw, 1, ci, co), dt, nhw, ci, co) for (dt, nhw, ci, co) in gr.CLASS1]
    assert all(p['kernel'] == 'tiled' and p['form'] == 'vector' for p, *_ in paths)
    bf = [p for p, dt, *_ in paths if dt == BF16]
    assert {p['bn'] for p in bf} == {32, 64, 96, 128, 192, 256}
    assert {p['bn'] for p, dt, *_ in paths if dt == F32} >= {32, 64, 128, 256}
    assert any(p['bn'] == 128 and p['ragged_n'] and p['empty_blocks'] for p in bf)      # 264 / 392 at M 129, 257
    assert any(p['gy'] == 4 for p in bf) and any(p['gy'] == 3 for p in bf)
    assert any(p['M'] % 128 and p['M'] > 128 for p in bf)
    assert any(p['K'] % 32 for p in bf) and any(p['K'] < 32 for p in bf)


def test_class2_table_is_direct_store():
    seen = set()
    for (dt, nhw, ks, ci, co) in gr.CLASS2:
        p = _fwd(dt, nhw, ks, ci, co, ws=False)
        assert p['kernel'] == 'tiled' and p['form'] == 'direct', (dt, nhw, ks, ci, co)
        assert dt == F32 or not p['vy']      # bf16: Cout % 8 != 0 throughout
        seen.add((dt, p['va'], p['bn']))
    for dt in (BF16, F32):
        assert {va for d, va, _ in seen if d == dt} == {True, False}
    assert {bn for d, _, bn in seen if d == BF16} == {32, 64, 96, 128}
    assert {c[1] for c in gr.CLASS2} == set(gr.C2_MAPS)
    assert not any(ks == 3 and ci == 3 and co in (32, 64) for (_, _, ks, ci, co) in gr.CLASS2)


def test_class3_table_splits():
    ps = [(_fwd(dt, nhw, ks, ci, co, pro=pa, bias=True), dt, pa) for (dt, nhw, ks, ci, co, pa) in gr.CLASS3]
    assert all(p['kernel'] == 'split' and p['splits'] > 1 for p, *_ in ps)
    for dt in (BF16, F32):
        mine = [p for p, d, _ in ps if d == dt]
        assert any(p['ragged'] for p in mine) and any(not p['ragged'] for p in mine)
        assert any(p['K'] % 32 for p in mine)
        assert any(p['va'] and p['vb'] for p in mine) and any(not p['va'] and not p['vb'] for p in mine)
    bf = [(p, pa) for p, d, pa in ps if d == BF16]
    assert any(p['ragged'] and p['va'] and p['vb'] for p, _ in bf)           # vector operands, ragged last split
    assert any(pa is not None and p['va'] for p, pa in bf) and any(pa is not None and not p['va'] for p, pa in bf)
    assert any(p['M'] > 128 for p, _ in bf)                                     # more than one M tile
    # without the workspace the same shapes take the unsplit tiled kernel
    assert all(_fwd(dt, nhw, ks, ci, co, pro=pa, bias=True, ws=False)['kernel'] == 'tiled'
               for (dt, nhw, ks, ci, co, pa) in gr.CLASS3)


def test_class4_to_6_tables():
    assert len(gr.C4_MAPS) == 9
    kinds = {_fwd(BF16, nhw, 3, ci, co, pro=pa)['kernel'] for (ci, co, pa) in gr.CLASS4 for nhw in gr.C4_MAPS}
    assert kinds == {'tiled', 'split'}
    assert any(pa is not None for (_, _, pa) in gr.CLASS4)
    st = [(_fwd(dt, nhw, 3, 3, co, stats=s), dt, nhw) for (dt, nhw, co) in gr.CLASS5 for s in (False, True)]
    assert any(p['kernel'] == 'stem_mfma' and p['fuse'] for p, *_ in st)
    assert any(p['kernel'] == 'stem_mfma' and not p['fuse'] and nhw[2] % 128 for p, _, nhw in st)
    assert {p['co'] for p, dt, _ in st if p['kernel'] == 'stem_valu' and dt == F32} == {32, 64}
    assert all(p['kernel'] in ('stem_mfma', 'stem_valu') for p, *_ in st)
    s6 = {(M, K, co, pa): gr.fwd_path(True, 1, 1, M, K, co, 1, pro=pa) for (M, K, co, pa) in gr.CLASS6}
    assert s6[(gr.BIG + 77, 64, 80, None)]['kernel'] == 'tiled' and gr.stream_ok(gr.BIG + 77, 64, 80, True) == 0
    assert {(p['kt'], p['nt']) for p in s6.values() if p['kernel'] == 'stream'} >= {(2, 9), (3, 12), (1, 6)}
    assert any(p['kernel'] == 'stream' and k[3] is not None for k, p in s6.items())
    assert any(p['kernel'] == 'proj' for p in s6.values())
    assert any(p['kernel'] == 'tiled' and k[3] is not None for k, p in s6.items())
    assert all(k[0] in (gr.BIG, gr.BIG + 77) for k in s6)


def test_class7_and_9_tables():
    fw = [_fwd(dt, nhw, ks, ci, co, bias=True) for (dt, nhw, ks, ci, co) in gr.CLASS7]
    bw = [_fwd(dt, nhw, ks, co, ci) for (dt, nhw, ks, ci, co) in gr.CLASS7]     # mode 1: Cin and Cout swapped
    assert any(p['kernel'] == 'split' for p in bw) and any(p['kernel'] == 'split' for p in fw)
    assert any(p['kernel'] == 'tiled' and p['form'] == 'direct' for p in bw)
    assert any(p['kernel'] == 'tiled' and p['form'] == 'vector' and p['empty_blocks'] for p in bw)
    assert any(ks == 3 and ci != co for (_, _, ks, ci, co) in gr.CLASS7)
    va9, vy9, vd9 = set(), set(), set()
    for (dt, nhw, ks, ci, co, dlx, dly, xo, yo) in gr.CLASS9:
        p = gr.fwd_path(dt == BF16, *nhw, ci, co, ks, ldx=ci + dlx, ldy=co + dly, ax=not xo, ay=not yo, ws=False)
        q = gr.wgrad_path(dt == BF16, *nhw, ci, co, ks, ldx=ci + dlx, lddy=co + dly, ax=not xo, ad=not yo)
        va9.add((dt, dlx, xo, p['va']))
        vy9.add((dt, dly, yo, p['vy']))
        vd9.add((dt, dly, yo, q['vd']))
        assert q['va'] == p['va']
    assert (BF16, 8, 0, True) in va9 and (BF16, 3, 0, False) in va9 and (BF16, 0, 1, False) in va9
    assert (F32, 8, 0, True) in va9 and (F32, 3, 0, False) in va9
    assert (BF16, 8, 0, True) in vy9 and (BF16, 1, 0, False) in vy9 and (BF16, 0, 1, False) in vy9
    assert (BF16, 8, 0, True) in vd9 and (BF16, 3, 0, False) in vd9 and (BF16, 0, 1, False) in vd9


def test_class8_table_contains_its_plans():
    ps = [(gr.wgrad_path(dt == BF16, *nhw, ci, co, ks, pro=pa), dt, nhw, ks, ci, co, pa)
          for (dt, nhw, ks, ci, co, pa) in gr.CLASS8]
    for dt in (BF16, F32):
        mine = [p for p, d, *_ in ps if d == dt and p['kernel'] == 'wgrad']
        assert any(p['empty'] > 0 and p['xcd'] for p in mine)                       # 9 splits rounded up to 16
        assert any(p['splits'] == 9 and p['tiles'] == 1 for p in mine)              # a single tile: no round-up
        assert any(p['M'] % p['chunk'] and p['splits'] > 1 for p in mine)           # ragged last split
        assert any(p['va'] and p['vd'] for p in mine) and any(not p['va'] for p in mine)
        assert any(not p['vd'] for p in mine)
        assert any(p['walk'] for p in mine)
        assert any(p['K'] % 64 and p['ktiles'] > 1 for p in mine)
    e = gr.wgrad_path(True, 1, 1, 1025, 72, 72, 1)
    assert (e['natural'], e['splits'], e['tiles']) == (9, 16, 4)
    bf = [(p, pa) for p, d, _, _, _, _, pa in ps if d == BF16]
    assert sum(p['kernel'] == 'stem_wgrad' for p, _ in bf) == len(gr.C8_STEM_W)
    assert any(p['kernel'] == 'wgrad_cin3' for p, _ in bf)
    assert any(p['kernel'] == 'wgrad_cin3' for p, d, *_ in ps if d == F32)
    assert any(pa is not None and p['walk'] for p, pa in bf) and any(pa is not None and not p['va'] for p, pa in bf)
    assert {co for (_, _, _, _, co, _) in gr.CLASS8} >= {8, 12, 36, 64, 66, 72, 264, 320}
    assert {nhw[2] for (dt, nhw, ks, _, _, _) in gr.CLASS8 if ks == 1 and nhw[:2] == (1, 1)} >= set(gr.C8_M)


def test_guarded_allocator_on_the_cpu():
    g = gr.Guarded('cpu')
    a = g.alloc(10, torch.float32, 'a')
    b = g.alloc(7, torch.bfloat16, 'b', offset=1)
    assert a.numel() == 10 and b.numel() == 7 and b.data_ptr() % 16 == 2
    a.zero_()
    b.zero_()
    g.check()
    flat, v = g.out_rows(3, 4, 6, torch.float32, 'rows')
    assert flat.numel() == 2 * 6 + 4
    v.fill_(1.0)
    assert gr.gaps_untouched(flat, 3, 4, 6)
    flat[4] = 0.0
    assert not gr.gaps_untouched(flat, 3, 4, 6)
    g.check()
    g.bufs[0][1][g.bufs[0][2] + 10] = 0.0   # one element past the view
    with pytest.raises(AssertionError, match='guard of a'):
        g.check()
