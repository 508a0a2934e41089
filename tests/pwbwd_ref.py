"""The unfused librod chain the fused 1x1 backwards replace — rod_bn_bwd_apply (dy written) ->
rod_conv_fwd with the mode-1 weights (dx) -> rod_conv_wgrad (dw, db) — as the oracle shared by
test_gpu_pwbwd.py and test_gpu_pwbwd_edges.py."""
import torch

from rod import ops


def nerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def unfused_chain(dz, y, mean, rstd, gamma, beta, act, coef, x, xpro, wt1, bias=False):
    """(dy, dx, dw, db or None) of the unfused backward on the same inputs."""
    M, Cout = y.shape
    Cin = x.shape[1]
    dev = y.device
    dy = torch.empty_like(y)
    ops._abi.call('rod_bn_bwd_apply', dz, y, mean, rstd, gamma, beta, coef, dy, M, Cout, act, ops.dtcode(y),
                  ops.stream())
    dx = torch.empty_like(x)
    ops.conv_fwd_raw(dy, wt1, None, dx, 1, 1, M, Cout, Cin, 1)
    dw = torch.empty(Cout, Cin, device=dev)
    db = torch.empty(Cout, device=dev) if bias else None
    wsz = ops._abi.query('rod_conv_wgrad_workspace', 1, 1, M, Cin, Cout, 1)
    ops._abi.call('rod_conv_wgrad', x, *ops._pro_args(xpro), dy, dw, db, ops.workspace(wsz, dev), 1, 1, M, Cin,
                  Cout, 1, 0, 0, ops.dtcode(x), ops.stream())
    return dy, dx, dw, db


def xsums64(dx, x, xpro):
    """The input BatchNorm's backward sums (sum g, sum g*xhat) over (dx, x) in float64."""
    xm, xr, xg, xb, xact = xpro
    xd = x.double()
    xs = xr.double() * xg.double()
    zx = xd * xs + (xb.double() - xm.double() * xs)
    if xact == ops.ROD_ACT_RELU6:
        gx = dx.double() * ((zx > 0) & (zx < 6))
    else:
        assert xact == ops.ROD_ACT_NONE
        gx = dx.double()
    return gx.sum(0), (gx * ((xd - xm.double()) * xr.double())).sum(0)
