"""Float64 reference of the convolutional prenets' layers (the reference project's src/module.py:7-90: Conv2d / Conv1d,
ReLU, 2x2 max pooling; the batch-1 definition of decoding, src/decode.py:88) in plain torch - never built on conv_ops -
and the case table shared by tests/test_conv_plan_cpu.py, tests/test_conv_reference_cpu.py and
tests/test_conv_variants_gpu.py.

A case is a convolution over x [B,C,H,W] held on the device in some LAYOUT, i.e. element strides (sb, sh, sw, sc) of
conv_ops.Geom:
    'cl'      contiguous channels-last [B,H,W,C]
    'btcf'    the [B,T,C*F] feature tensor read in place (H = T, W = F): sw = 1, sc = F - how VGGExtractor reads its input
    'cnn'     CNNExtractor's training geometry: B = 1, W = the batch, x = [batch, T, D] read in place (sb = 0)
    'packed'  CNNExtractor's packed-inference geometry: W = 1, x = [B, T, D] read in place (sw = 0)
and a ROUTE through conv_ops (ConvFn / conv_len):
    'direct'     csrc/conv3x3.hip implicit GEMMs (asrk_conv3x3_f32 / _wgrad_f32 / _len_f32)
    'first'      the 1-3 plane first layer (asrk_conv3x3_first_f32 / _first_wgrad_f32 / _first_len_f32)
    'im2col_cl'  asrk_im2col_cl_f32 (+ col2im_cl, weight reorder) + asrk_gemm_f32
    'im2col_ld'  asrk_im2col_ld_f32 (+ col2im) + asrk_gemm_f32, K padded to a multiple of 4
`env` holds the knobs that force a route (conv_ops reads them at call time).  `plan` names, per launch family
('fwd', 'dgrad', 'wgrad'), the fields of asrk_conv3x3_plan_info the row is there for; test_conv_plan_cpu holds every row
to them and the table as a whole to the list of properties below.  A re-tune of wgrad_lds, the 80-KB budget, the cost
model of wgrad_plan or the tile size moves SHAPES in this table, not assertions.

What the weight-gradient planner does with shapes under the size limit (scan of asrk_conv3x3_plan_info over B 1..6,
H 2..400, W in {6, 13, 20, 40}, every channel pair, <= 11 MB per activation): the cost model picks TH below thmax
wherever all tiles fit one trip (smaller tiles, same trip count - e.g. every (1, 2..3, W) shape) and in most multi-trip
shapes; TH == thmax with a ragged last row tile needs e.g. (3, 43, 40, 128, 128).  More than one trip needs more than
512 / splits tiles: 3 x 341 x 40 positions at splits = 1 are the smallest W = 40 shape that walks (10.5 MB), so the
walk rows are the largest of the table.  With 64 -> 64 or 64 -> 128 channels no shape under the limit makes EVERY
workgroup walk exactly two tiles (that takes 1024 / 512 tiles with TH == thmax); the 128 -> 128 row does.

W = 128 cannot have a ragged last tile (every tile is one row): it is the row with H * W an exact multiple of 128.

Criterion of the GPU test (bound): the hard limits of tests/test_conv_gpu.py - helpers.rel_err < 1e-4 on outputs,
< 1e-3 on gradients - AND rel_err <= max(F * e32, 4 * 2**-24), e32 = rel_err of conv_reference evaluated in float32 on
the CPU against its own float64 run on the row's inputs, F one constant per tensor kind
(tests/test_conv_variants_gpu.py records the measured ratios)."""
import collections
import zlib

import torch
import torch.nn.functional as F

F64 = torch.float64
HARD = dict(y=1e-4, dx=1e-3, dw=1e-3, db=1e-3)
FLOOR = 4 * 2.0 ** -24
PLAN_FIELDS = ('supported', 'TH', 'tiles_img', 'ntiles', 'gx', 'gy', 'most', 'fewest', 'lds', 'ws', 'thmax')
PLAN_LEN = 12


def bound(e32, factor, kind):
    return min(max(factor * e32, FLOOR), HARD[kind])


# ------------------------------------------------------------------------------------------------ the references
def conv_reference(x_bchw, w, b, stride, pad, relu):
    """Conv2d(stride, padding=pad) (+ ReLU) of src/module.py in the dtype of its arguments"""
    y = F.conv2d(x_bchw, w, b, stride=stride, padding=pad)
    return F.relu(y) if relu else y


def conv_len_reference(x, w, b, stride, pad, relu, hlen, out_hlen):
    """image i is clamp(hlen[i], 0, H) rows high: the input rows beyond read as zero, the output rows >= out_hlen[i]
    are exactly zero"""
    B, _, H, _ = x.shape
    hv = torch.as_tensor(hlen, dtype=torch.int64).clamp(0, H).view(B, 1, 1, 1)
    x = torch.where(torch.arange(H).view(1, 1, H, 1) < hv, x, torch.zeros_like(x))
    y = conv_reference(x, w, b, stride, pad, relu)
    ho = torch.as_tensor(out_hlen, dtype=torch.int64).view(B, 1, 1, 1)
    return torch.where(torch.arange(y.shape[2]).view(1, 1, -1, 1) < ho, y, torch.zeros_like(y))


# ------------------------------------------------------------------------------------------------ the case table
Case = collections.namedtuple('Case', 'name route B H W C Cout k s p relu layout grads env plan mode hlen why')


def _c(name, route, B, H, W, C, Cout, k=(3, 3), s=(1, 1), p=(1, 1), relu=True, layout='cl', grads='xwb', env=(),
       plan=None, mode='train', hlen=None, why=''):
    return Case(name, route, B, H, W, C, Cout, k, s, p, relu, layout, grads, tuple(env), plan or {}, mode, hlen, why)


NODIRECT = (('ASRK_CONV_DIRECT', '0'),)
NOCL = (('ASRK_CONV_CL', '0'),)


def _d(name, B, H, W, C=64, Cout=64, th=None, **kw):
    """a direct row whose forward and data-gradient tiles touch at most `th` rows"""
    plan = dict(kw.pop('plan', {}))
    plan.setdefault('fwd', dict(TH=th))
    plan.setdefault('dgrad', dict(TH=th))
    return _c(name, 'direct', B, H, W, C, Cout, plan=plan, **kw)


# forward / data gradient (kind 0): B = 2 so the image offset matters; H * W > 128 and H * W % 128 != 0 unless stated
DIRECT_CASES = [
    _d('d_w1', 2, 130, 1, th=128, plan=dict(wgrad=dict(TH=36, thmax=73, tiles_img=4)), why='W = 1; wgrad H % TH != 0'),
    _d('d_w2', 2, 67, 2, th=64),
    _d('d_w3', 2, 45, 3, th=44),
    _d('d_w6', 2, 23, 6, th=22),
    _d('d_w13_norelu', 2, 21, 13, th=11, relu=False, why='no ReLU: no xmask / ymask'),
    _d('d_w20_128x128', 2, 23, 20, 128, 128, th=8),
    _d('d_w33_128x64', 2, 9, 33, 128, 64, th=5, why='data gradient 64 -> 128: two channel passes; forward too'),
    _d('d_w40', 2, 7, 40, th=4),
    _d('d_w40_64x128_exact', 2, 16, 40, 64, 128, th=4, why='H * W = 5 * 128'),
    _d('d_w40_bias_only', 2, 7, 40, th=4, grads='b', why='dw == NULL'),
    _d('d_w64', 2, 3, 64, th=2),
    _d('d_w65', 2, 3, 65, th=3),
    _d('d_w100', 2, 3, 100, th=3),
    _d('d_w127', 2, 3, 127, th=2),
    _d('d_w128', 2, 3, 128, th=1, plan=dict(wgrad=dict(TH=1, thmax=1, lds=141408)), why='the largest wgrad LDS plan'),
    _d('d_small', 2, 5, 13, th=11, why='H * W < 128'),
    _d('d_h1', 2, 1, 40, th=4, why='H = 1'),
    _c('d_w129_im2col', 'im2col_cl', 2, 3, 129, 64, 64, plan=dict(fwd=dict(supported=0), wgrad=dict(supported=0)),
       why='W > 128: asrk_conv3x3_supported == 0, the fallback itself runs'),
]

# weight gradient (kind 1): the tile walk.  most / fewest: tiles walked by the busiest / idlest workgroup
WGRAD_CASES = [
    _d('w_s1_walk', 3, 341, 40, 64, 64, th=4,
       plan=dict(wgrad=dict(gy=1, gx=512, ntiles=1023, most=2, fewest=1, TH=1, thmax=2)), why='cost model: TH < thmax'),
    _d('w_s2_walk', 6, 85, 40, 64, 128, th=4, plan=dict(wgrad=dict(gy=2, gx=256, ntiles=510, most=2, fewest=1, TH=1))),
    _d('w_s4_walk', 5, 151, 20, 128, 128, th=8,
       plan=dict(wgrad=dict(gy=4, gx=128, ntiles=255, most=2, fewest=1, TH=3, thmax=6)), why='and H % TH != 0'),
    _d('w_s4_even2', 4, 316, 13, 128, 128, th=11,
       plan=dict(wgrad=dict(gy=4, gx=128, ntiles=256, most=2, fewest=2, TH=5, thmax=9)), why='every workgroup: 2 tiles'),
    _d('w_thmax_ragged', 3, 43, 40, 128, 128, th=4,
       plan=dict(wgrad=dict(gy=4, most=1, TH=2, thmax=2, tiles_img=22)), why='TH == thmax, H % TH != 0'),
]


def _first_rows():
    rows = []
    shapes = [(1, 64, 2, 7, 40, 3), (2, 128, 2, 5, 64, 2), (3, 64, 2, 3, 65, 1), (1, 128, 2, 3, 128, 1),
              (2, 64, 2, 5, 13, 5), (3, 128, 2, 7, 40, 3)]
    for C, Cout, B, H, W, th in shapes:
        for layout in ('cl', 'btcf'):
            base = 'f_c%d_%d_w%d_%s' % (C, Cout, W, layout)
            plan = dict(fwd=dict(TH=th, gy=Cout // 64), wgrad=dict(TH=th, gy=Cout // 64, most=1))
            rows.append(_c(base, 'first', B, H, W, C, Cout, layout=layout, plan=plan))
            rows.append(_c(base + '_ld', 'im2col_ld', B, H, W, C, Cout, layout=layout, env=NODIRECT,
                           why='K = %d padded to %d' % (9 * C, (9 * C + 3) // 4 * 4)))
    rows.append(_c('f_walk', 'first', 1030, 3, 13, 2, 64, layout='btcf',
                   plan=dict(wgrad=dict(gx=1024, ntiles=1030, most=2, fewest=1, TH=3)), why='1030 tiles over 1024 groups'))
    return rows


FIRST_CASES = _first_rows()

# the generic route
GENERIC_CASES = [
    _c('g_5x5s3p2', 'im2col_ld', 2, 11, 10, 7, 9, k=(5, 5), s=(3, 3), p=(2, 2), relu=False),
    _c('g_2x2s3_cl', 'im2col_cl', 2, 11, 10, 8, 9, k=(2, 2), s=(3, 3), p=(0, 0), why='inputs no window reads: dx == 0'),
    _c('g_2x2s3_ld', 'im2col_ld', 2, 11, 10, 8, 9, k=(2, 2), s=(3, 3), p=(0, 0), env=NOCL, why='ASRK_CONV_CL=0'),
    _c('g_full', 'im2col_cl', 2, 3, 4, 4, 5, k=(5, 6), relu=False, why='kernel == padded input: one output position'),
    _c('g_cnn_odd', 'im2col_ld', 1, 31, 3, 10, 12, k=(4, 1), s=(2, 1), p=(1, 0), relu=False, layout='cnn'),
    _c('g_cnn_odd_cl', 'im2col_cl', 1, 31, 3, 12, 12, k=(4, 1), s=(2, 1), p=(1, 0), relu=False, layout='cnn'),
]
UNCOVERED = ('g_2x2s3_cl', 'g_2x2s3_ld')

# length-aware inference: B = 5, hlen = [H, last row ends inside a 128-position tile, hlen * W % 128 == 0, 0, 1]
LEN_CASES = [
    _c('l_direct', 'direct', 5, 37, 40, 64, 64, mode='len', hlen=(37, 23, 16, 0, 1)),
    _c('l_direct_128x64', 'direct', 5, 37, 20, 128, 64, relu=False, mode='len', hlen=(37, 23, 32, 0, 1)),
    _c('l_direct_cl', 'im2col_cl', 5, 37, 40, 64, 64, env=NODIRECT, mode='len', hlen=(37, 23, 16, 0, 1)),
    _c('l_first_btcf', 'first', 5, 37, 40, 3, 64, layout='btcf', mode='len', hlen=(37, 23, 16, 0, 1)),
    _c('l_first_cl_128', 'first', 5, 37, 40, 1, 128, mode='len', hlen=(37, 23, 16, 0, 1)),
    _c('l_first_ld', 'im2col_ld', 5, 37, 40, 3, 64, layout='btcf', env=NODIRECT, mode='len', hlen=(37, 23, 16, 0, 1)),
    # the CNN geometry: stride 2, out_hlen = hlen // 2 given explicitly (CNNExtractor._forward_packed)
    _c('l_cnn_cl', 'im2col_cl', 5, 37, 1, 40, 16, k=(4, 1), s=(2, 1), p=(1, 0), relu=False, layout='packed', mode='len',
       hlen=(37, 23, 16, 0, 1)),
    _c('l_cnn_ld', 'im2col_ld', 5, 37, 1, 10, 16, k=(4, 1), s=(2, 1), p=(1, 0), relu=False, layout='packed', mode='len',
       hlen=(37, 23, 16, 0, 1)),
]

# partial gradient requests: requires_grad on one of (weight, bias, input) only
PARTIAL_BASES = ('d_w40', 'f_c3_128_w40_btcf')
PARTIAL_GRADS = ('w', 'b', 'x')

TRAIN_CASES = DIRECT_CASES + WGRAD_CASES + FIRST_CASES + GENERIC_CASES
CASES = TRAIN_CASES + LEN_CASES
BY_NAME = {c.name: c for c in CASES}
REPEAT = [c for c in TRAIN_CASES if c.route in ('direct', 'first') and 'w' in c.grads]     # bit-identical dW / db twice


def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def out_hw(c):
    return out_size(c.H, c.k[0], c.s[0], c.p[0]), out_size(c.W, c.k[1], c.s[1], c.p[1])


def out_hlen_of(c, hlen=None):
    """None where the layer keeps the height (conv_len then uses hlen itself), else the explicit list"""
    hlen = c.hlen if hlen is None else hlen
    return None if out_hw(c) == (c.H, c.W) else tuple(max(0, min(h, c.H)) // 2 for h in hlen)


def strides(c):
    """(sb, sh, sw, sc) of the layout, in elements"""
    B, H, W, C = c.B, c.H, c.W, c.C
    return {'cl': (H * W * C, W * C, C, 1), 'btcf': (H * C * W, C * W, 1, W), 'cnn': (0, C, H * C, 1),
            'packed': (H * C, C, 0, 1)}[c.layout]


def layout_index(c):
    """int64 [B,C,H,W]: the element of the flat device tensor that holds x[b,c,h,w]"""
    sb, sh, sw, sc = strides(c)
    ar = lambda n, st, shape: (torch.arange(n) * st).view(shape)
    return (ar(c.B, sb, (-1, 1, 1, 1)) + ar(c.C, sc, (1, -1, 1, 1)) + ar(c.H, sh, (1, 1, -1, 1))
            + ar(c.W, sw, (1, 1, 1, -1)))


def plan_queries(c):
    """launch family -> the arguments (kind, B, H, W, C, Cout) of asrk_conv3x3_plan_info that describe it"""
    if c.k != (3, 3) or c.s != (1, 1) or c.p != (1, 1):
        return {}
    if c.C <= 3:
        return dict(fwd=(2, c.B, c.H, c.W, c.C, c.Cout), wgrad=(3, c.B, c.H, c.W, c.C, c.Cout))
    return dict(fwd=(0, c.B, c.H, c.W, c.C, c.Cout), dgrad=(0, c.B, c.H, c.W, c.Cout, c.C),
                wgrad=(1, c.B, c.H, c.W, c.C, c.Cout))


def uncovered_inputs(c):
    """bool [H,W]: input positions no window of the convolution reads"""
    Ho, Wo = out_hw(c)
    rows, cols = torch.zeros(c.H, dtype=torch.bool), torch.zeros(c.W, dtype=torch.bool)
    for o in range(Ho):
        for t in range(c.k[0]):
            h = o * c.s[0] - c.p[0] + t
            if 0 <= h < c.H:
                rows[h] = True
    for o in range(Wo):
        for t in range(c.k[1]):
            w = o * c.s[1] - c.p[1] + t
            if 0 <= w < c.W:
                cols[w] = True
    return ~(rows.view(-1, 1) & cols.view(1, -1))


GATE_EPS = 1e-4


def near_zero_preactivations(c, t):
    """bool [B,Cout,Ho,Wo]: outputs whose float64 pre-activation lies within GATE_EPS of 0.  The ReLU gate of the
    gradients is discontinuous there: any float32 evaluation (the CPU's, whose error is e32, or a kernel's) may round
    such a sum to the other side of 0, and one flipped gate moves dx / dw / db by a whole term, far outside any bound
    derived from rounding.  With pre-activations of unit scale and float32 sums good to about 1e-6, a row of 10^6
    outputs has such an element more often than not, so dy is set to 0 at them (about 1 output in 10^4): the gate's
    value then matters to no gradient, and y itself is still compared everywhere."""
    pre = conv_reference(t['x'].double(), t['w'].double(), t['b'].double(), c.s, c.p, False)
    return pre.abs() < GATE_EPS


_inputs = {}


def make_inputs(c):
    """-> dict of float32 CPU tensors x [B,C,H,W], w [Cout,C,KH,KW] scaled by 1 / (3 sqrt(Cin)), b, dy [B,Cout,Ho,Wo];
    seeded by the row's name, made once and never modified.  dy is random, and 0 where a ReLU's pre-activation is
    within GATE_EPS of 0 (near_zero_preactivations).  Length rows: the input rows beyond hlen are random and
    far from zero (3 * randn + 1)."""
    if c.name not in _inputs:
        g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
        Ho, Wo = out_hw(c)
        t = dict(x=torch.randn(c.B, c.C, c.H, c.W, generator=g),
                 w=torch.randn(c.Cout, c.C, c.k[0], c.k[1], generator=g) / (3 * c.C ** 0.5),
                 b=torch.randn(c.Cout, generator=g) * 0.1,
                 dy=torch.randn(c.B, c.Cout, Ho, Wo, generator=g))
        if c.relu and c.mode == 'train':
            t['dy'][near_zero_preactivations(c, t)] = 0.0
        if c.hlen is not None:
            for i, h in enumerate(c.hlen):
                h = max(0, min(h, c.H))
                t['x'][i, :, h:] = 3.0 * torch.randn(c.C, c.H - h, c.W, generator=g) + 1.0
        _inputs[c.name] = t
    return _inputs[c.name]


def reference_of(c, t, dtype=F64, grads=None, hlen=None):
    """training rows -> dict y / dx / dw / db (the gradients `grads` asks for; default: the row's);
    length rows -> dict y"""
    x, w, b = (t[k].detach().clone().to(dtype) for k in ('x', 'w', 'b'))
    if c.mode == 'len':
        hlen = c.hlen if hlen is None else hlen
        oh = out_hlen_of(c, hlen)
        return dict(y=conv_len_reference(x, w, b, c.s, c.p, c.relu, hlen, hlen if oh is None else oh))
    grads = c.grads if grads is None else grads
    x.requires_grad_('x' in grads), w.requires_grad_('w' in grads), b.requires_grad_('b' in grads)
    y = conv_reference(x, w, b, c.s, c.p, c.relu)
    y.backward(t['dy'].to(dtype))
    out = dict(y=y.detach())
    for k, v in (('x', x), ('w', w), ('b', b)):
        if k in grads:
            out['d' + k] = v.grad
    return out


def pool_ties_input():
    """[2,64,8,14] through ReLU: about half the entries are exactly 0, so many 2x2 windows tie at 0"""
    g = torch.Generator().manual_seed(77)
    return torch.randn(2, 64, 8, 14, generator=g).relu(), torch.randn(2, 64, 4, 7, generator=g)


def relu_zero_input():
    """a ReLU output y with exact zeros (+0 and -0) and the gradient that meets it"""
    g = torch.Generator().manual_seed(78)
    y = torch.randn(5000, generator=g).relu()
    y[::7] = -0.0
    return y, torch.randn(5000, generator=g)
