"""The C-ABI library loads and exports every symbol include/rod.h declares (CPU-only:
no kernel is launched; argument validation paths return before any HIP call)."""
import ctypes

import numpy as np
import pytest

from rod import _abi


def test_library_exports_every_declared_symbol():
    lib = _abi.lib()
    protos = _abi.parse_header()
    assert len(protos) >= 20
    for name in protos:
        assert hasattr(lib, name), name
    nm = ctypes.CDLL(_abi.LIB_PATH)
    for name in protos:
        getattr(nm, name)


def test_abi_version():
    import re
    want = int(re.search(r'#define ROD_ABI_VERSION (\d+)', open(_abi.HEADER_PATH).read()).group(1))
    assert _abi.lib().rod_abi_version() == want


def test_invalid_arguments_raise_with_message():
    with pytest.raises(RuntimeError, match='bad shape'):
        _abi.call('rod_dw3x3_fwd', None, None, None, None, None, 0, None, None, None, 0, 8, 8, 8, 1, 1, 1, 8, 8, 0,
                  None)
    with pytest.raises(RuntimeError, match='ksize'):
        _abi.call('rod_conv_fwd', None, None, None, None, None, 0, None, None, None, None, None,
                  None, None, None, None, None, 0, None, 1, 4, 4, 8, 8, 5, 0, 0, 0, None)
    with pytest.raises(RuntimeError, match='dtype'):
        _abi.call('rod_conv_weight_prep', None, None, 8, 8, 1, 0, 7, None)
    with pytest.raises(RuntimeError, match='offsets'):
        _abi.call('rod_match_anchors', None, None, np.array([0, 5, 9], np.int32), np.zeros(2, np.float32), 2,
                  None, None, None, None, None, None, None, 1, 10, 4, None)


def test_level_offsets_must_be_monotone():
    """Every entry that takes a level table fills it through one check set: the ODM target and
    classifier-loss entries reject non-monotone offsets too (the ODM targets look a level up by them)."""
    lvl, thr, buf = np.array([0, 5, 3, 10], np.int32), np.zeros(3, np.float32), np.zeros(1, np.float32)
    for name, args in (
            ('rod_det_targets', (None,) * 6 + (lvl, thr, 3, None, None, None, None, 1, 10, 0, None)),
            ('rod_softmax_ce_hnm', (None,) * 4 + (lvl, 3, 1.0, None, None, None, 1, 10, 4, 0, None)),
            ('rod_iou_factor_bwd', (None,) * 4 + (lvl, 3, 1.0, buf, 1, 10, 4, 0, None)),
            ('rod_hnm_loss', (None,) * 4 + (lvl, 3, 1.0, None, None, None, None, 1, 10, 4, 0, None)),
            ('rod_smoothl1_masked', (None,) * 3 + (lvl, 3, 1.0, buf, None, None, buf, 1, 10, 0, None)),
            ('rod_match_anchors_nn', (None, None, lvl, 3) + (None,) * 7 + (1, 10, 4, None))):
        with pytest.raises(RuntimeError, match='levels: offsets must be monotone'):
            _abi.call(name, *args)


def test_workspace_queries_are_host_only():
    assert _abi.query('rod_bn_stats_workspace', 1000, 64) > 0
    assert _abi.query('rod_conv_wgrad_workspace', 2, 16, 16, 32, 64, 3) >= 4 * 64 * 9 * 32
    assert _abi.query('rod_dw3x3_bwd_filter_workspace', 2, 8, 8, 96) >= 4 * 9 * 96


def test_ir_block_policy_is_host_only():
    """The fused-block support / persistent-variant queries run on the host, and the eval
    backbone's preference picks the blocks measured faster fused."""
    import torch

    from nets.backbone.mobilenet_v2 import layer_plan
    from rod import ops
    bf16 = torch.bfloat16

    def picked():
        return [idx for (idx, kind, s, cin, inner, cout, res, sc) in layer_plan()
                if kind == 'ir' and inner > cin and ops.ir_block_preferred(cin, inner, cout, s, res, bf16)]
    # by default the 16..32-channel blocks take the chain with the expand output recomputed
    # (ops.rc_eval_ok, measured faster); without it the fused kernel takes the ones measured
    # faster fused than the plain chain
    assert picked() == [], picked()
    ops._DISABLE.add('rcinf')
    try:
        assert picked() == [3, 4, 6, 7], picked()
    finally:
        ops._DISABLE.discard('rcinf')
    ops._DISABLE.add('rcinf1')
    try:
        assert picked() == [4, 6, 7], picked()   # the stride-1 ones fused, block 1 (stride 2) recomputed
    finally:
        ops._DISABLE.discard('rcinf1')
    assert ops.ir_block_supported(64, 384, 64, 1, True, bf16)
    assert not _abi.lib().rod_ir_block_persistent(64, 384, 64, 1, 1, 1)    # parameters exceed LDS
    assert _abi.lib().rod_ir_block_persistent(32, 192, 32, 1, 1, 1)
    assert not ops.ir_block_preferred(24, 144, 24, 1, True, torch.float32)


def test_dw_fused_pw_plan_query():
    """Host-only plan query: bf16 stride-1 tiles of <= 32 columns x 48 channels, cout % 8 == 0 <= 32."""
    from rod import ops
    q = _abi.lib().rod_dw3x3_bwd_fused_pw_supported
    assert q(8, 360, 640, 144, 24, ops.ROD_ACT_RELU6, ops.ROD_ACT_RELU6, 1) and q(8, 720, 1280, 32, 16, ops.ROD_ACT_RELU6, ops.ROD_ACT_RELU6, 1) and q(8, 180, 320, 192, 32, ops.ROD_ACT_RELU6, ops.ROD_ACT_RELU6, 1)
    assert not q(8, 360, 640, 144, 24, ops.ROD_ACT_RELU6, ops.ROD_ACT_RELU6, 0)          # fp32
    assert not q(8, 90, 160, 384, 64, ops.ROD_ACT_RELU6, ops.ROD_ACT_RELU6, 1)           # cout 64: two MFMA k steps
    assert not q(8, 360, 640, 144, 20, ops.ROD_ACT_RELU6, ops.ROD_ACT_RELU6, 1)          # cout % 8
    assert not q(8, 360, 640, 144, 24, ops.ROD_ACT_NONE, ops.ROD_ACT_RELU6, 1)
