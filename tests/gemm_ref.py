"""Helpers of the exact base-GEMM tests (test_gemm_ref_host.py, test_gpu_gemm_exact.py).

Integer-valued operands make rod_conv_fwd / rod_conv_wgrad bit-identical to float64 under any
summation order, tile shape or split count, so every bar is equality:

  * x, w, dy are integers in [-3, 3], bias integers in [-8, 8] (exact in bf16 and fp32); the exact
    BatchNorm prologue (mean 0, rstd 1, gamma in {1, 2}, beta a non-zero integer in [-2, 2], act NONE
    or RELU6) keeps the conv input a small integer too;
  * every partial sum stays far below 2^24 (`Case.bound`, asserted per case), so fp32 accumulation
    is exact on the bf16 MFMA path and on the fp32 16x16x4 path alike;
  * the reference is torch.nn.functional.conv2d in float64 on the CPU with autograd for dx / dw /
    db; the float64 -> float32 round trip is asserted lossless and bf16 outputs are that float32
    rounded once to nearest-even.

The module also restates gemm.hip's dispatch arithmetic in Python (split_plan, wgrad_plan, the
forward N-tile menus, pw_stream_groups, the va / vb / vy / vd predicates), so a test can assert which
kernel form its shape reaches, and provides a guarded allocator whose check() finds any write
outside the exact extent of an output or workspace.  No GPU is needed to import it.
"""
import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU6 = 0, 1
BK = 32           # k depth of an LDS step (gemm.hip)
WG_T = 64         # co / k tile of conv_wgrad_kernel
SW_TW = 128       # stem kernels: pixels per block row
PRO_MAXC = 2048
EXACT = 1 << 24   # integers below this magnitude are exact in fp32


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ dispatch arithmetic restated
def split_plan(M, Cout, K):
    """(splits, kper) of rod_conv_fwd's split-K."""
    tiles = cdiv(M, 128) * cdiv(Cout, 128)
    ksteps = cdiv(K, BK)
    if tiles >= 128 or ksteps < 8:
        return 1, K
    splits = min(ksteps // 2, cdiv(256, tiles))
    if splits < 2:
        return 1, K
    per = cdiv(ksteps, splits)
    return cdiv(ksteps, per), per * BK


def fwd_workspace_bytes(N, H, W, Cin, Cout, ks):
    M = N * H * W
    splits, _ = split_plan(M, Cout, ks * ks * Cin)
    return splits * M * Cout * 4 if splits > 1 else 0


def wgrad_plan(M, Cin, Cout, ks):
    """dict(ctiles, ktiles, chunk, splits, natural) of conv_wgrad_kernel's grid; `natural` is the
    split count before the round-up to a multiple of 8 (splits past it are empty)."""
    K = ks * ks * Cin
    ctiles, ktiles = cdiv(Cout, WG_T), cdiv(K, WG_T)
    tiles = ctiles * ktiles
    splits = max(1, min(cdiv(2048, tiles), cdiv(M, 128)))
    chunk = cdiv(cdiv(M, splits), BK) * BK
    natural = splits = cdiv(M, chunk)
    if tiles > 1 and splits >= 8:
        splits = (splits + 7) // 8 * 8
    return dict(ctiles=ctiles, ktiles=ktiles, tiles=tiles, chunk=chunk, splits=splits, natural=natural)


def stem_wgrad_plan(N, H, W):
    xb = cdiv(W, SW_TW)
    rb = max(1, cdiv(N * H * xb, 2048))
    yb = cdiv(H, rb)
    return dict(xb=xb, yb=yb, rb=rb, nblk=N * yb * xb)


def wgrad_workspace_bytes(N, H, W, Cin, Cout, ks):
    M = N * H * W
    splits = wgrad_plan(M, Cin, Cout, ks)['splits']
    if ks == 3 and Cin == 3 and Cout == 32:
        splits = max(splits, stem_wgrad_plan(N, H, W)['nblk'])
    part = (splits * Cout * ks * ks * Cin + 3) // 4 * 4
    cchunk = max(64, cdiv(M, 512))
    return (part + cdiv(M, cchunk) * Cout) * 4


def pw_stream_groups(M, K, Cout, gred=False):
    """(groups, MFMA tiles per group) of the streaming 1x1 kernel; (0, 0) when it does not apply."""
    if K > 96 or K % 8 or Cout % 16 or M < 65536:
        return 0, 0
    for c in ((3, 2, 4, 6, 9, 12, 8) if gred else (12, 9, 6, 8, 4, 3, 2)):
        if Cout % (16 * c) == 0:
            return Cout // (16 * c), c
    return 0, 0


def stream_ok(M, K, Cout, bf16):
    return int(bool(bf16) and pw_stream_groups(M, K, Cout)[0] > 0)


def pw_proj_ok(M, K, Cout, act):
    """pw_proj_launch's own conditions (ROD_PW_PROJ left alone)."""
    if K > 192 or K % 8 or Cout > 32 or Cout % 8 or M < 65536:
        return False
    return cdiv(K, 32) > 1 and act == ACT_RELU6


def vec_elems(bf16):
    return 8 if bf16 else 4


def pred_va(bf16, aligned, ldx, ks, Cin):
    return bool(aligned and ldx % vec_elems(bf16) == 0 and (ks == 1 or Cin % 8 == 0))


def pred_vb(bf16, K):
    return K % vec_elems(bf16) == 0


def pred_vy(bf16, aligned, ldy):
    return bool(aligned and ldy % vec_elems(bf16) == 0)


pred_vd = pred_vy   # dy rows of the weight gradient: the same test on lddy


def fwd_tile(va, vb, vy, Cout):
    """('vector' | 'direct', BN) of the tiled forward kernel."""
    if va and vb and vy:
        return 'vector', (cdiv(Cout, 32) * 32 if Cout <= 192 else 256 if Cout <= 256 else 128)
    return 'direct', (cdiv(Cout, 32) * 32 if Cout <= 96 else 128)


def fwd_grid(M, Cout, bn):
    gx, gy = cdiv(M, 128), cdiv(Cout, bn)
    if gy > 1:
        gx = (gx + 7) // 8 * 8
    return gx, gy


def fwd_path(bf16, N, H, W, Cin, Cout, ks, ldx=0, ldy=0, ax=True, ay=True, ws=True, pro=None, bias=False,
             stats=False):
    """The kernel rod_conv_fwd launches (conv_fwd_typed without gred / epilogue / BatchNorm-backward
    arguments).  pro: None or the prologue's activation code; ws: a workspace is passed."""
    ldx, ldy = ldx or Cin, ldy or Cout
    M, K = N * H * W, ks * ks * Cin
    va, vb, vy = pred_va(bf16, ax, ldx, ks, Cin), pred_vb(bf16, K), pred_vy(bf16, ay, ldy)
    p = dict(va=va, vb=vb, vy=vy, M=M, K=K, stats_separate=False)
    splits, kper = split_plan(M, Cout, K)
    if bf16 and pro is None and ks == 3 and Cin == 3 and Cout == 32 and vy:
        return dict(p, kernel='stem_mfma', fuse=bool(stats and W % SW_TW == 0))
    if ws and splits > 1 and not (ks == 3 and Cin == 3):
        return dict(p, kernel='split', splits=splits, kper=kper, ragged=K % kper != 0)
    if stats and not (va and vb and vy):
        return dict(fwd_path(bf16, N, H, W, Cin, Cout, ks, ldx, ldy, ax, ay, ws, pro, bias, False), stats_separate=True)
    if pro is None and ks == 3 and Cin == 3 and vy:
        if not bf16 and Cout == 32:
            return dict(p, kernel='stem_valu', co=32)
        if Cout == 64:
            return dict(p, kernel='stem_valu', co=64)
    if bf16 and ks == 1 and not bias and va and vb and vy:
        if pro is not None and Cin <= PRO_MAXC and pw_proj_ok(M, K, Cout, pro):
            return dict(p, kernel='proj', kt=cdiv(K, 32), nt=cdiv(Cout, 16))
        ng, nt = pw_stream_groups(M, K, Cout)
        if (pro is None or K <= 32) and ng > 0:
            return dict(p, kernel='stream', ng=ng, nt=nt, kt=3 if K > 64 else 2 if K > 32 else 1)
    form, bn = fwd_tile(va, vb, vy, Cout)
    gx, gy = fwd_grid(M, Cout, bn)
    return dict(p, kernel='tiled', form=form, bn=bn, gx=gx, gy=gy, empty_blocks=gy > 1 and gx > cdiv(M, 128),
                ragged_n=Cout % bn != 0)


def wgrad_path(bf16, N, H, W, Cin, Cout, ks, ldx=0, lddy=0, ax=True, ad=True, pro=None):
    """The kernel rod_conv_wgrad launches (wgrad_typed)."""
    ldx, lddy = ldx or Cin, lddy or Cout
    M = N * H * W
    va, vd = pred_va(bf16, ax, ldx, ks, Cin), pred_vd(bf16, ad, lddy)
    p = dict(wgrad_plan(M, Cin, Cout, ks), va=va, vd=vd, M=M, K=ks * ks * Cin)
    if bf16 and pro is None and ks == 3 and Cin == 3 and Cout == 32 and vd:
        return dict(p, kernel='stem_wgrad', **stem_wgrad_plan(N, H, W))
    if pro is None and ks == 3 and Cin == 3 and vd:
        return dict(p, kernel='wgrad_cin3')
    return dict(p, kernel='wgrad', walk=ks == 3 and va, xcd=p['tiles'] > 1 and p['splits'] % 8 == 0,
                empty=p['splits'] - p['natural'])


# ------------------------------------------------------------------ integer cases and float64 reference
class Case:
    """One conv: x [N,H,W,Cin], w [Cout,ks,ks,Cin], dy [N,H,W,Cout], bias [Cout] as float32 CPU
    tensors holding integers; pro = None or (mean, rstd, gamma, beta, act)."""

    def __init__(self, N, H, W, Cin, Cout, ks, pro_act=None, seed=0):
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * (N * H * W) + 131 * Cin + 17 * Cout + ks)

        def ints(shape, lo, hi):
            return torch.randint(lo, hi + 1, shape, generator=g).float()
        self.geo = (N, H, W, Cin, Cout, ks)
        self.x = ints((N, H, W, Cin), -3, 3)
        self.w = ints((Cout, ks, ks, Cin), -3, 3)
        self.dy = ints((N, H, W, Cout), -3, 3)
        self.bias = ints((Cout,), -8, 8)
        self.pro = None
        if pro_act is not None:
            beta = ints((Cin,), 1, 2) * (ints((Cin,), 0, 1) * 2 - 1)     # +-1, +-2: never 0
            self.pro = (torch.zeros(Cin), torch.ones(Cin), ints((Cin,), 1, 2), beta, pro_act)

    @property
    def M(self):
        return self.geo[0] * self.geo[1] * self.geo[2]

    @property
    def K(self):
        return self.geo[5] ** 2 * self.geo[3]

    def amax(self):
        """Largest magnitude of the conv input (after the prologue)."""
        if self.pro is None:
            return 3
        return 6 if self.pro[4] == ACT_RELU6 else 3 * 2 + 2

    def bound(self):
        """Upper bound of every partial sum of y, dx, dw and db: each product is at most 3 * amax
        (9 without a prologue), each output sums at most max(K, ks^2 Cout, M) of them, plus the bias."""
        N, H, W, Cin, Cout, ks = self.geo
        return 3 * self.amax() * max(self.K, ks * ks * Cout, self.M) + 8

    def conv_input(self, dtype=torch.float64):
        """x after the exact prologue act(fma(x, gamma, beta)) (x itself without one)."""
        a = self.x.to(dtype)
        if self.pro is not None:
            _, _, gamma, beta, act = self.pro
            a = a * gamma.to(dtype) + beta.to(dtype)
            if act == ACT_RELU6:
                a = a.clamp(0, 6)
        return a


def _lossless32(t64):
    t32 = t64.float()
    assert torch.equal(t32.double(), t64), 'float64 -> float32 round trip lost bits'
    return t32


def reference(case, bias=True, grads=True):
    """float64 conv2d (SAME) and autograd; returns float32 dict(y, dx, dw, db) (dx: the gradient wrt
    the conv input, i.e. wrt the prologue's output when there is one)."""
    assert case.bound() < EXACT, case.geo
    ks = case.geo[5]
    a = case.conv_input().requires_grad_(grads)
    w = case.w.double().requires_grad_(grads)
    b = case.bias.double().requires_grad_(grads) if bias else None
    y = F.conv2d(a.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), b, padding=ks // 2).permute(0, 2, 3, 1)
    out = dict(y=_lossless32(y.detach().contiguous()))
    assert float(out['y'].abs().max()) < EXACT
    if grads:
        y.backward(case.dy.double())
        out.update(dx=_lossless32(a.grad), dw=_lossless32(w.grad), db=_lossless32(b.grad) if bias else None)
        assert max(float(out['dx'].abs().max()), float(out['dw'].abs().max())) < EXACT
    return out


def im2col_matmul(case, bias=True):
    """y by an explicit im2col and one float64 matmul (k = (i*3 + j)*Cin + ci, the kernels' order)."""
    N, H, W, Cin, Cout, ks = case.geo
    a = case.conv_input()
    p = ks // 2
    ap = F.pad(a, (0, 0, p, p, p, p))
    cols = [ap[:, i:i + H, j:j + W, :] for i in range(ks) for j in range(ks)]
    A = torch.cat(cols, dim=3).reshape(N * H * W, ks * ks * Cin)
    y = A @ case.w.double().reshape(Cout, ks * ks * Cin).t()
    if bias:
        y = y + case.bias.double()
    return y.reshape(N, H, W, Cout)


def prep_reference(w, mode):
    """rod_conv_weight_prep's operand layout: mode 0 [Cout][ks*ks*Cin]; mode 1 (backward-data)
    [Cin][ks*ks*Cout] with the taps flipped."""
    Cout, ks, _, Cin = w.shape
    if mode == 0:
        return w.reshape(Cout, ks * ks * Cin).clone()
    return w.flip(1, 2).permute(3, 1, 2, 0).reshape(Cin, ks * ks * Cout).contiguous()


# ------------------------------------------------------------------ guarded allocator
SENTINEL = {torch.bfloat16: -17.0, torch.float32: -12345.0}
GUARD_BYTES = 512


class Guarded:
    """Tensors of exactly the requested element count inside larger buffers whose every other
    element holds a sentinel; check() asserts that nothing outside the views was written."""

    def __init__(self, device):
        self.device = device
        self.bufs = []

    def alloc(self, numel, dtype, name, offset=0):
        """A flat view of `numel` elements, pre-filled with the sentinel too.  The view starts
        16-byte aligned plus `offset` elements."""
        pad = GUARD_BYTES // torch.empty(0, dtype=dtype).element_size()
        buf = torch.full((pad + offset + numel + pad,), SENTINEL[dtype], dtype=dtype, device=self.device)
        assert buf.data_ptr() % 16 == 0
        self.bufs.append((name, buf, pad + offset, numel))
        return buf[pad + offset:pad + offset + numel]

    def rows(self, t, ld, name, offset=0):
        """A copy of the 2-D CPU tensor t [M][C] as a row-strided device view with leading
        dimension ld >= C: exactly (M-1)*ld + C elements, the columns between C and ld sentinels."""
        M, C = t.shape
        flat = self.alloc((M - 1) * ld + C, t.dtype, name, offset)
        v = flat.as_strided((M, C), (ld, 1))
        v.copy_(t)
        return v

    def out_rows(self, M, C, ld, dtype, name, offset=0):
        flat = self.alloc((M - 1) * ld + C, dtype, name, offset)
        return flat, flat.as_strided((M, C), (ld, 1))

    def check(self):
        for name, buf, lo, n in self.bufs:
            s = SENTINEL[buf.dtype]
            ok = bool(((buf[:lo] == s).all() & (buf[lo + n:] == s).all()).item())
            assert ok, f'guard of {name} overwritten'


def gaps_untouched(flat, M, C, ld):
    """The columns between C and ld of a row-strided output still hold the sentinel."""
    if ld == C or M < 2:
        return True
    g = flat[:(M - 1) * ld].view(M - 1, ld)[:, C:]
    return bool((g == SENTINEL[flat.dtype]).all().item())


# ------------------------------------------------------------------ case tables (shared by both tests)
def _m(M):
    return (1, 1, M)


BF16, F32 = 'bf16', 'f32'

# class 1: tiled vector form, ks = 1.  (dtype, NHW, Cin, Cout)
C1_M = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257)
C1_COUT = (8, 32, 40, 96, 104, 192, 200, 256, 264, 392)
C1_CIN = (8, 24, 32, 40, 72)
CLASS1 = ([(BF16, _m(M), 64, 64) for M in C1_M] +
          [(BF16, _m(M), 64, co) for M in (17, 129, 257) for co in C1_COUT] +
          [(BF16, _m(129), ci, 64) for ci in C1_CIN] +
          [(F32, _m(M), 64, 64) for M in (1, 17, 129)] +
          [(F32, _m(129), 64, co) for co in (8, 40, 104, 200, 264)] +
          [(F32, _m(257), 64, 392)] +
          [(F32, _m(129), ci, 64) for ci in (8, 24, 40)])

# class 2: direct-store form (run without a workspace, so a deep K does not split).
# (dtype, NHW, ks, Cin, Cout)
C2_MAPS = ((2, 1, 2), (2, 2, 3), (2, 3, 5), (1, 5, 9))
C2_COUT = (4, 12, 36, 66, 99, 132)
C2_SRC = ((1, 128), (3, 3), (3, 36), (3, 99))


def _class2():
    out = []
    for i, co in enumerate(C2_COUT):
        for j, (ks, ci) in enumerate(C2_SRC):
            nhw = C2_MAPS[(i + j) % 4]
            out.append((BF16, nhw, ks, ci, co))
            # fp32 rows are 16 bytes at Cout % 4 == 0: only the shapes whose plan is still direct-store
            if (i + j) % 3 == 0 and fwd_path(False, *nhw, ci, co, ks, ws=False)['kernel'] == 'tiled' and \
                    fwd_path(False, *nhw, ci, co, ks, ws=False)['form'] == 'direct':
                out.append((F32, nhw, ks, ci, co))
    return out


CLASS2 = _class2()

# class 3: split-K.  (dtype, NHW, ks, Cin, Cout, pro_act)
CLASS3 = [(BF16, (2, 3, 5), 1, 1920, 320, None), (BF16, (2, 2, 3), 3, 128, 128, None),
          (BF16, (2, 3, 5), 3, 36, 36, None), (BF16, (2, 3, 5), 3, 99, 12, None),
          (BF16, (2, 3, 5), 1, 264, 40, None), (BF16, (1, 1, 129), 1, 264, 136, None),
          (BF16, (2, 3, 5), 3, 40, 16, ACT_RELU6), (BF16, (2, 3, 5), 3, 36, 36, ACT_NONE),
          (BF16, (2, 2, 3), 1, 264, 40, ACT_RELU6),
          (F32, (2, 3, 5), 3, 36, 36, None), (F32, (2, 2, 3), 3, 128, 128, None), (F32, (2, 3, 5), 3, 99, 12, None),
          (F32, (2, 3, 5), 3, 40, 16, ACT_RELU6)]

# class 4: 3x3 borders, N = 3, every H, W in {1, 2, 3}.  (Cin, Cout, pro_act)
C4_MAPS = tuple((3, h, w) for h in (1, 2, 3) for w in (1, 2, 3))
CLASS4 = [(ci, co, pa) for (ci, co) in ((8, 16), (8, 36), (36, 16), (36, 36)) for pa in (None, ACT_NONE, ACT_RELU6)]

# class 5: stem forms.  (dtype, NHW, Cout)
CLASS5 = ([(BF16, (2, h, w), 32) for w in (5, 127, 128, 129, 256) for h in (1, 2, 9)] +
          [(F32, (2, 2, w), co) for co in (32, 64) for w in (5, 64, 65, 129)] + [(BF16, (2, 2, 65), 64)])

# class 6: streaming 1x1 (bf16, no bias).  (M, K, Cout, pro_act)
BIG = 65536
CLASS6 = [(BIG + 77, 8, 16, None), (BIG + 77, 40, 144, None), (BIG + 77, 96, 576, None), (BIG + 77, 64, 80, None),
          (BIG, 40, 144, None), (BIG + 77, 8, 16, ACT_RELU6), (BIG + 77, 16, 96, ACT_RELU6), (BIG, 16, 96, ACT_NONE),
          (BIG + 77, 40, 24, ACT_RELU6)]

# class 7: backward through ops.conv2d (dx by the mode-1 weights, dw, db).  (dtype, NHW, ks, Cin, Cout)
CLASS7 = [(BF16, _m(129), 1, 64, 264), (BF16, _m(257), 1, 392, 64), (BF16, (2, 3, 5), 1, 128, 36),
          (BF16, (2, 3, 5), 3, 36, 12), (BF16, (3, 2, 3), 3, 8, 16), (BF16, (3, 3, 1), 3, 36, 16),
          (BF16, (2, 3, 5), 1, 320, 1920), (BF16, (2, 3, 5), 1, 1920, 320), (BF16, (2, 2, 3), 3, 128, 128),
          (BF16, (2, 3, 5), 3, 99, 12), (BF16, (2, 3, 5), 3, 12, 99),
          (F32, _m(129), 1, 64, 264), (F32, (2, 3, 5), 3, 36, 12), (F32, (2, 3, 5), 1, 1920, 320),
          (F32, (3, 2, 3), 3, 8, 16)]

# class 8: weight and bias gradient.  (NHW, ks, Cin, Cout, pro_act); dtype: fp32 as well on every third
C8_M = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1025)
C8_STEM_W = (5, 127, 128, 129, 256)
CLASS8 = ([(_m(M), 1, 64, 64, None) for M in C8_M] +
          [(_m(M), 1, 72, 72, None) for M in (1, 63, 64, 65, 1025)] +
          [(_m(129), 1, 64, co, None) for co in (8, 72, 264)] +
          [(_m(1025), 1, 64, 264, None), (_m(65), 1, 64, 320, None), (_m(1025), 1, 8, 12, None)] +
          [((2, 3, 5), 3, 24, 64, None), ((2, 3, 5), 3, 40, 64, None), ((1, 5, 9), 3, 24, 72, None)] +
          [((2, 3, 5), 3, 36, 64, None), ((2, 3, 5), 3, 99, 64, None)] +
          [((2, 3, 5), 1, 64, co, None) for co in (12, 36, 66)] + [((2, 3, 5), 3, 36, 12, None)] +
          [((2, 2, 65), 3, 3, 64, None)] +
          [((2, 2, w), 3, 3, 32, None) for w in C8_STEM_W] +
          [(nhw, 3, 16, 24, None) for nhw in ((40, 1, 2), (7, 3, 5), (5, 2, 3), (3, 1, 1))] +
          [((7, 3, 5), 3, 72, 72, None)] +
          [((5, 2, 3), 3, 8, 16, ACT_RELU6), ((5, 2, 3), 3, 8, 16, ACT_NONE), ((5, 2, 3), 3, 36, 16, ACT_RELU6),
           ((2, 3, 5), 1, 40, 24, ACT_RELU6)])
CLASS8 = [(BF16,) + c for c in CLASS8] + [(F32,) + c for i, c in enumerate(CLASS8) if i % 3 == 0 or c[3] == 66]

# class 9: leading dimensions and unaligned bases, direct ABI calls.
# (dtype, NHW, ks, Cin, Cout, dldx, dldy, xoff, yoff): ldx = Cin + dldx, ldy / lddy = Cout + dldy
C9_LD = ((8, 0, 0, 0), (3, 0, 0, 0), (0, 8, 0, 0), (0, 1, 0, 0), (0, 3, 0, 0), (8, 8, 0, 0), (3, 3, 0, 0), (0, 0, 1, 0),
         (0, 0, 0, 1), (8, 8, 1, 1))
CLASS9 = ([(BF16, _m(129), 1, 64, 64) + ld for ld in C9_LD] +
          [(BF16, (2, 3, 5), 3, 8, 16) + ld for ld in C9_LD] +
          [(F32, _m(129), 1, 64, 64) + ld for ld in C9_LD[:7:2] + C9_LD[7:9]] +
          [(BF16, (2, 3, 5), 3, 36, 12) + ld for ld in ((3, 0, 0, 0), (0, 3, 0, 0), (0, 0, 1, 1))])
