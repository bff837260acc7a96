"""GPU: every kernel variant of the per-step attention / decoder kernels (csrc/attention.hip: location convolution,
loc / dot energies + masked softmax, context, the pointwise LSTM cell, the embedding look-up; each with its backward)
called through the C entry points with raw tensors, and the autograd plumbing of decoder_ops over three chained steps,
against the float64 reference and on the case tables of tests/attention_reference.py.
tests/test_attention_plan_cpu.py holds every energy row to the launch geometry it names, and every energy row asks
asrk_attn_energy_plan again on the device before it runs, so no row passes on another branch's arithmetic.

Criterion, per tensor: helpers.rel_err < 1e-3 (outputs) / 2e-3 (gradients), the hard limits of tests/test_cfg3_gpu.py,
AND rel_err <= max(F * e32, 8 * 2**-24), e32 = rel_err of the float32 CPU run of the same reference against its float64
run on the row's inputs, F = 32 (the factor tests/test_conv_variants_gpu.py settled on for tile-ordered f32 sums).
Every test prints e32, the bound, the device error and device / e32 (pytest -s, lines starting ATTNVAR).

Buffer discipline of every direct call: each output is carved out of a larger allocation with 64 sentinel floats on both
sides (and sentinel padding columns where ctx_stride > Dv) that must survive; `+=` buffers (dkey_acc, dWp_acc, dwe_acc,
dbe_acc, dWc_acc, dW_acc) are pre-filled with random values R of the gradient's own scale and must hold R + gradient;
buffers the launcher zeroes or the kernel plainly stores (dq, dc, dprev, c, attn, e, ctx, dattn, cell outputs) are
pre-filled with NaN and must hold no NaN.  The direct energy backward is fed attention rows that sum to 0.5, not 1, so
that dbe = sum_t de is a real quantity under the normal bound; one true-softmax row per mode keeps |dbe| to
max(32 |dbe of the float32 CPU run|, 32 * 2**-24 * sum |de|).

Exact where the code promises it (torch.equal): attn == 0 and e == -inf beyond the length, dkey_acc rows beyond the
length bit-identical to their pre-fill, dc == 0 beyond the length, every guard band, the ordered embedding gradient
against a sequential float32 host accumulation and over two runs (in a child process: ASRK_DETERMINISTIC is read once),
replicas of expand_tape.  dq, dc over heads, dWc, dWp, dwe, dbe and the default embedding gradient are f32 atomics: no
bitwise repeatability is asserted for them (tests/test_determinism_gpu.py).

Largest device / e32 per tensor kind, as measured on the MI355X (ATTNVAR-MAX lines, printed after the last test):

    tensor     largest device / e32   where
    c          1.86                   c_ks_gt_t
    dprev      1.59                   c_t130_ks100
    dWc        1.92                   c_t130_ks100
    e          1.59                   d_bn1_t9
    attn       4.07                   d_bn1_t9
    dkey       2.51                   chain_loc_n2 (1.07 l_a64 among the direct rows)
    dq         2.27                   l_a64
    dc         2.23                   l_a65
    dWp        20.59                  l_shrink
    dwe        2.63                   l_bn1024 (2.48 in another run)
    dbe        18.27                  l_bn1024 (12.43, 17.22 in other runs: the order of the atomics)
    ctx        1.79                   chain_loc_n2 (1.00 in every direct row)
    dattn      1.00                   x_d1_t1
    dvalue     2.30                   chain_loc_n2
    gates, cell, h, dc_prev 1.00; dgates 1.63 (cell_1_256_dh)
    dW         8.32                   emb_130_10_5
    cell chain: dx 2.00, dc0 2.26, db 1.95, dw_ih 1.00, dw_hh 0.86, dh0 0.73, h 0.72, c 0.99

(378 figures over 93 tests; e32 2e-8 ... 8e-7.  No tensor kind needed a factor of its own.  The two large ratios are
sums over many workgroups that the CPU library adds blockwise: dWp of l_shrink is 128 rows x 16 chunks = 2048 per-
workgroup partial sums added by f32 atomics, one after the other, into each element, dbe of l_bn1024 is 4096 per-wave
sums added the same way; dW of emb_130_10_5 adds 26 rows per id by atomics.  On the true-softmax rows |dbe| was 5e-8
(direct) ... 1.2e-6 (chain_loc_n2) against limits of 2.4e-5 ... 2.0e-4.)
"""
import ctypes
import importlib
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import PKG_NAME
from helpers import rel_err
import attention_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD, SENT = 64, 777.25
NAN = float('nan')
F = {}                      # tensor kind -> its own factor (none needed: every kind holds R.FACTOR)
_ref, _worst = {}, {}


@pytest.fixture(scope="module")
def lib(ops):
    return importlib.import_module(PKG_NAME + "._lib")


@pytest.fixture(scope="module")
def dops(pkg, ops):
    return importlib.import_module(pkg.__name__ + ".decoder_ops")


@pytest.fixture(scope="module", autouse=True)
def report_largest_ratios():
    """after the module's last test: the largest device / e32 per tensor kind (the docstring's table)"""
    yield
    for k in sorted(_worst):
        print("ATTNVAR-MAX %-18s %6.2f  %s" % (k, _worst[k][0], _worst[k][1]))


# ------------------------------------------------------------------------------------------------ helpers
def carve(shape, fill=NAN):
    """-> (view of `shape` inside a larger allocation, the allocation): GUARD sentinel floats on both sides"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * GUARD,), SENT, dtype=torch.float32, device=DEV)
    view = flat[GUARD:GUARD + n].view(shape)
    if isinstance(fill, torch.Tensor):
        view.copy_(fill.view(shape))
    else:
        view.fill_(fill)
    return view, flat


def guards_intact(*flats):
    for flat in flats:
        g = torch.cat([flat[:GUARD], flat[flat.numel() - GUARD:]]).cpu()
        assert torch.equal(g, torch.full_like(g, SENT)), "a write outside the buffer"


def all_nan(*views):
    return all(bool(torch.isnan(v).all()) for v in views)


def no_nan(v):
    return not bool(torch.isnan(v).any())


def cached(name, make):
    """references are computed once, shared by the tests that need them and never modified"""
    if name not in _ref:
        _ref[name] = make()
    return _ref[name]


def kind_of(k, label=''):
    """the tensor kind of the report: step and layer numbers dropped, the cell chain's tensors kept apart"""
    return ('cell_chain.' if label == 'cell_chain' else '') + re.sub(r'\d+$', '', k)


def judge(label, got, ref, r32):
    bad = []
    for k, v in got.items():
        e32 = rel_err(r32[k], ref[k])
        err = rel_err(v.detach().double().cpu(), ref[k])
        b = R.bound(e32, k, F.get(kind_of(k), R.FACTOR))
        ratio = err / e32 if e32 > 0 else 0.0
        print("ATTNVAR %s | %s | e32 %.3e | bound %.3e | device %.3e | device/e32 %.2f" % (label, k, e32, b, err, ratio))
        if e32 * R.FACTOR > R.FLOOR and ratio > _worst.get(kind_of(k, label), (0.0, ''))[0]:
            _worst[kind_of(k, label)] = (ratio, label)
        if not (err < (R.HARD_GRAD if k.startswith('d') else R.HARD_OUT) and err <= b):
            bad.append((k, err, b))
    assert not bad, (label, bad)


def scaled_prefill(unit, ref):
    """random values of the gradient's own scale (float32), so that R + gradient loses neither"""
    return (unit * max(float(ref.abs().max()), 1e-30)).float()


def d(t):
    return t.to(DEV)


def live_plan(L, c, bwd):
    tpb, chunks, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    rc = L.asrk_attn_energy_plan(c.loc, bwd, c.B * c.N, c.T, c.A, c.K, ctypes.byref(tpb), ctypes.byref(chunks), ctypes.byref(lds))
    return (tpb.value, chunks.value) if rc == 0 else None


# ------------------------------------------------------------------------------------------------ location convolution
@pytest.mark.parametrize("case", R.CONV_CASES, ids=lambda c: c.name)
def test_loc_conv_row(ops, lib, case):
    c = case
    L, p, st = ops._L(), ops._p, ops._stream
    t = R.conv_inputs(c)
    ref = cached(c.name, lambda: R.conv_reference_of(c, t))
    r32 = cached(c.name + '/32', lambda: R.conv_reference_of(c, t, torch.float32))
    RdWc = scaled_prefill(t['RdWc'], ref['dWc'])
    prev, Wc, dc = d(t['prev']), d(t['Wc']), d(t['dc'])
    cv, cf = carve((c.B, c.T, c.K))
    lib.check(L.asrk_loc_conv_fwd_f32(p(prev), p(Wc), p(cv), c.B, c.N, c.T, c.K, c.ks, st()), "loc_conv")
    dpv, dpf = carve((c.B, c.N, c.T))
    dwv, dwf = carve((c.K, c.N, 2 * c.ks + 1), RdWc)
    lib.check(L.asrk_loc_conv_bwd_f32(p(dc), p(prev), p(Wc), None if c.skip == 'dprev' else p(dpv),
                                      None if c.skip == 'dWc' else p(dwv), c.B, c.N, c.T, c.K, c.ks, st()), "loc_conv_bwd")
    ops.check_errors()
    guards_intact(cf, dpf, dwf)
    assert no_nan(cv)
    got = dict(c=cv)
    full = dict(ref, dWc=RdWc.double() + ref['dWc'])
    full32 = dict(r32, dWc=RdWc + r32['dWc'])
    if c.skip == 'dprev':
        assert all_nan(dpv)
    else:
        assert no_nan(dpv)
        got['dprev'] = dpv
    if c.skip == 'dWc':
        assert torch.equal(dwv.cpu(), RdWc)
    else:
        got['dWc'] = dwv
    judge(c.name, got, full, full32)


# ------------------------------------------------------------------------------------------------ energies + softmax
def _energy_device_inputs(c, t):
    names = ('key', 'q', 'lens') + (('c', 'Wp', 'we', 'be') if c.loc else ())
    return {k: d(t[k]) for k in names}


def _finite_e(e):
    return torch.where(torch.isinf(e), torch.zeros_like(e), e)


@pytest.mark.parametrize("case", R.ENERGY_CASES, ids=lambda c: c.name)
def test_energy_forward_row(ops, lib, case):
    c = case
    L, p, st = ops._L(), ops._p, ops._stream
    assert live_plan(L, c, 0) == c.fwd
    t = R.energy_inputs(c)
    ref = cached(c.name + '/f', lambda: R.energy_forward_of(c, t))
    r32 = cached(c.name + '/f32', lambda: R.energy_forward_of(c, t, torch.float32))
    x = _energy_device_inputs(c, t)
    BN = c.B * c.N
    av, af = carve((BN, c.T))
    ev, ef = carve((BN, c.T))
    lib.check(L.asrk_attn_energy_fwd_f32(c.loc, p(x['key']), p(x['q']), p(x.get('c')), p(x.get('Wp')), p(x.get('we')),
                                         p(x.get('be')), p(x['lens']), p(av), p(ev), c.B, c.N, c.T, c.A, c.K, c.temp, st()),
              "attn_energy")
    ops.check_errors()
    guards_intact(af, ef)
    mask = R.frame_mask(t['lens'], c.N, c.T)
    a, e = av.cpu(), ev.cpu()
    assert no_nan(a) and no_nan(e)
    assert torch.equal(a[mask], torch.zeros(int(mask.sum())))                          # exactly 0 beyond the length
    assert torch.equal(e[mask], torch.full((int(mask.sum()),), float('-inf')))         # exactly -inf beyond the length
    assert bool(torch.isfinite(e[~mask]).all()) and float(a[~mask].min()) > 0
    fin = lambda r: dict(e=_finite_e(r['e']), attn=r['attn'])
    judge(c.name, dict(e=_finite_e(e), attn=a), fin(ref), fin(r32))


@pytest.mark.parametrize("case", [c for c in R.ENERGY_CASES if c.bwd is not None], ids=lambda c: c.name)
def test_energy_backward_row(ops, lib, case):
    c = case
    L, p, st = ops._L(), ops._p, ops._stream
    assert live_plan(L, c, 1) == c.bwd
    t = R.energy_inputs(c)
    ref = cached(c.name + '/b', lambda: R.energy_backward_of(c, t))
    r32 = cached(c.name + '/b32', lambda: R.energy_backward_of(c, t, torch.float32))
    x = _energy_device_inputs(c, t)
    BN = c.B * c.N
    acc = ('dkey',) + (('dWp', 'dwe') + (() if c.softmax else ('dbe',)) if c.loc else ())
    pre = {k: scaled_prefill(t['R' + k], ref[k]) for k in acc}
    if c.loc and c.softmax:
        pre['dbe'] = torch.zeros(1)
    dkv, dkf = carve((BN, c.T, c.A), pre['dkey'])
    dqv, dqf = carve((BN, c.A))
    flats = [dkf, dqf]
    o = {}
    if c.loc:
        for k, shape, fill in (('dc', (c.B, c.T, c.K), NAN), ('dWp', (c.A, c.K), pre['dWp']), ('dwe', (c.A,), pre['dwe']),
                               ('dbe', (1,), pre['dbe'])):
            o[k], f = carve(shape, fill)
            flats.append(f)
    attn, dattn = d(t['attn']), d(t['dattn'])      # named: a temporary would be freed, and its block reused, before the launch
    lib.check(L.asrk_attn_energy_bwd_f32(c.loc, p(x['key']), p(x['q']), p(x.get('c')), p(x.get('Wp')), p(x.get('we')),
                                         p(x['lens']), p(attn), p(dattn), p(dkv), p(dqv), p(o.get('dc')),
                                         p(o.get('dWp')), p(o.get('dwe')), p(o.get('dbe')), c.B, c.N, c.T, c.A, c.K,
                                         c.temp, st()), "attn_energy_bwd")
    ops.check_errors()
    guards_intact(*flats)
    mask = R.frame_mask(t['lens'], c.N, c.T)
    dk = dkv.cpu()
    assert torch.equal(dk[mask], pre['dkey'][mask])                 # rows beyond the length: bit-identical to the pre-fill
    assert no_nan(dqv)
    got = dict(dkey=dk, dq=dqv)
    full, full32 = dict(ref), dict(r32)
    if c.loc:
        dc = o['dc'].cpu()
        assert no_nan(dc)
        bmask = R.frame_mask(t['lens'], 1, c.T)
        assert torch.equal(dc[bmask], torch.zeros(int(bmask.sum()), c.K))              # exactly 0 beyond the length
        got.update(dc=dc, dWp=o['dWp'], dwe=o['dwe'])
        if c.softmax:
            dbe, noise = abs(float(o['dbe'])), float(ref['de'].abs().sum())
            lim = max(32 * abs(float(r32['dbe'])), 32 * 2.0 ** -24 * noise)
            print("ATTNVAR %s | dbe (softmax) | float32 CPU %.3e | limit %.3e | device %.3e" % (c.name, abs(float(r32['dbe'])), lim, dbe))
            assert dbe <= lim
        else:
            got['dbe'] = o['dbe']
    for k in acc:
        full[k] = pre[k].double() + ref[k]
        full32[k] = pre[k] + r32[k]
    judge(c.name, got, full, full32)


# ------------------------------------------------------------------------------------------------ context
@pytest.mark.parametrize("case", R.CTX_CASES, ids=lambda c: c.name)
def test_context_row(ops, lib, case):
    c = case
    L, p, st = ops._L(), ops._p, ops._stream
    t = R.ctx_inputs(c)
    ref = cached(c.name, lambda: R.ctx_reference_of(c, t))
    r32 = cached(c.name + '/32', lambda: R.ctx_reference_of(c, t, torch.float32))
    stride = c.Dv + c.pad
    cv, cf = carve((c.BN, stride), SENT)
    cv[:, :c.Dv] = NAN
    attn, value = d(t['attn']), d(t['value'])
    lib.check(L.asrk_attn_context_fwd_f32(p(attn), p(value), p(cv), c.BN, c.T, c.Dv, stride, st()), "attn_context")
    g = torch.full((c.BN, stride), NAN, device=DEV)                  # a read of the padding columns poisons dattn
    g[:, :c.Dv] = d(t['dctx'])
    dv, df = carve((c.BN, c.T))
    lib.check(L.asrk_attn_context_bwd_f32(p(g), p(value), p(dv), c.BN, c.T, c.Dv, stride, st()), "attn_context_bwd")
    ops.check_errors()
    guards_intact(cf, df)
    pad = cv[:, c.Dv:].cpu()
    assert torch.equal(pad, torch.full_like(pad, SENT))              # the padding columns are not ours
    assert no_nan(cv[:, :c.Dv]) and no_nan(dv)
    judge(c.name, dict(ctx=cv[:, :c.Dv], dattn=dv), ref, r32)


# ------------------------------------------------------------------------------------------------ LSTM cell
@pytest.mark.parametrize("mode", R.CELL_MODES)
@pytest.mark.parametrize("shape", R.CELL_SHAPES, ids=lambda s: "%dx%d" % s)
def test_lstm_cell(ops, lib, shape, mode):
    B, H = shape
    L, p, st = ops._L(), ops._p, ops._stream
    t = R.cell_inputs(B, H)
    name = 'cell_%d_%d_%s' % (B, H, mode)
    ref = cached(name, lambda: R.cell_reference_of(t, mode))
    r32 = cached(name + '/32', lambda: R.cell_reference_of(t, mode, torch.float32))
    gv, gf = carve((B, 4 * H), t['gates'])
    cv, cf = carve((B, H))
    hv, hf = carve((B, H))
    c_prev = d(t['c_prev'])
    lib.check(L.asrk_lstm_cell_fwd_f32(p(gv), p(c_prev), p(cv), p(hv), B, H, st()), "lstm_cell")
    act = gv.clone()
    dgv, dgf = carve((B, 4 * H), act)
    dcv, dcf = carve((B, H))
    dh = d(t['dh']) if mode in ('both', 'dh') else None
    dc = d(t['dc']) if mode in ('both', 'dc') else None
    lib.check(L.asrk_lstm_cell_bwd_f32(p(dgv), p(c_prev), p(cv), p(dh), p(dc), p(dcv), B, H, st()), "lstm_cell_bwd")
    ops.check_errors()
    guards_intact(gf, cf, hf, dgf, dcf)
    for v in (act, cv, hv, dgv, dcv):                                # pre-activations of +-30 and +-90 included
        assert bool(torch.isfinite(v).all())
    judge(name, dict(gates=act, cell=cv, h=hv, dgates=dgv, dc_prev=dcv), ref, r32)


# ------------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("shape", R.EMB_SHAPES, ids=lambda s: "n%d_D%d_V%d" % s)
def test_embedding(ops, lib, shape):
    n, D, V = shape
    L, p, st = ops._L(), ops._p, ops._stream
    t = R.emb_inputs(n, D, V)
    name = 'emb_%d_%d_%d' % shape
    ref = cached(name, lambda: R.emb_reference_of(t))
    r32 = cached(name + '/32', lambda: R.emb_reference_of(t, torch.float32))
    RdW = scaled_prefill(t['RdW'], ref['dW'])
    idx, W, dout = d(t['idx']), d(t['W']), d(t['dout'])
    ov, of = carve((n, D))
    lib.check(L.asrk_embedding_fwd_f32(p(idx), p(W), p(ov), n, D, V, st()), "embedding")
    wv, wf = carve((V, D), RdW)
    lib.check(L.asrk_embedding_bwd_f32(p(idx), p(dout), p(wv), n, D, V, st()), "embedding_bwd")
    ops.check_errors()
    guards_intact(of, wf)                                            # ids -1 and V write nowhere
    out = ov.cpu()
    bad = (t['idx'] < 0) | (t['idx'] >= V)
    assert torch.equal(out, ref['emb'].float())                      # a gather is exact; out-of-range ids give zero rows
    assert float(out[bad].abs().sum()) == 0.0
    untouched = torch.ones(V, dtype=torch.bool)
    untouched[t['idx'][~bad]] = False
    assert torch.equal(wv.cpu()[untouched], RdW[untouched])          # rows no id names keep their pre-fill
    judge(name, dict(emb=out, dW=wv), dict(ref, dW=RdW.double() + ref['dW']), dict(r32, dW=RdW + r32['dW']))


def test_ordered_embedding_gradient_in_a_fresh_process(ops):
    """ASRK_DETERMINISTIC=1 (read once, at the library's first use): embedding_bwd_ordered_kernel equals a sequential
    float32 host accumulation bit for bit, twice"""
    env = dict(os.environ, ASRK_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "attention_emb_worker.py")], capture_output=True, text=True,
                       env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert [l for l in r.stdout.splitlines() if l.startswith("ORDERED")] == ["ORDERED %d %d %d ok" % s for s in R.EMB_SHAPES]


# ------------------------------------------------------------------------------------------------ refusals
def test_launchers_refuse_on_the_host_and_write_nothing(ops, lib):
    """argument sets every launcher rejects before any device call: the documented status, NaN-pre-filled outputs
    untouched; B == 0 is ASRK_OK and writes nothing"""
    L, p, st = ops._L(), ops._p, ops._stream
    nanb = lambda *s: torch.full(s, NAN, device=DEV)
    inp = lambda *s: torch.zeros(s, device=DEV)
    EINVAL, ESHAPE = -1, -2
    outs = []

    def conv(B, N, T, K, ks, drop=None, only='fb'):
        a = dict(prev=inp(max(B, 1), max(N, 1), T), Wc=inp(K, max(N, 1), 2 * ks + 1), c=nanb(max(B, 1), T, K),
                 dc=inp(max(B, 1), T, K), dprev=nanb(max(B, 1), max(N, 1), T), dWc=nanb(K, max(N, 1), 2 * ks + 1))
        outs.extend(('conv%s %s' % ((B, N, T, K, ks, drop, only), k), a[k]) for k in ('c', 'dprev', 'dWc'))
        if drop:
            a[drop] = None
        r = []
        if 'f' in only:
            r.append(L.asrk_loc_conv_fwd_f32(p(a['prev']), p(a['Wc']), p(a['c']), B, N, T, K, ks, st()))
        if 'b' in only:
            r.append(L.asrk_loc_conv_bwd_f32(p(a['dc']), p(a['prev']), p(a['Wc']), p(a['dprev']), p(a['dWc']), B, N, T, K,
                                             ks, st()))
        return tuple(r)

    assert conv(2, 0, 8, 3, 2) == (EINVAL, EINVAL)                                  # N = 0
    assert conv(2, 4, 8, 4, 2000) == (ESHAPE, ESHAPE)                               # LDS over 60 KB
    assert conv(2, 1, 8, 3, 2, drop='Wc') == (EINVAL, EINVAL)                       # a null required pointer
    assert conv(2, 1, 8, 3, 2, drop='c', only='f') == (EINVAL,)
    assert conv(2, 1, 8, 3, 2, drop='dc', only='b') == (EINVAL,)
    assert conv(0, 1, 8, 3, 2) == (0, 0)                                            # B = 0

    def energy(loc, B, N, T, A, K, temp, drop=None, only='fb'):
        b, n = max(B, 1), max(N, 1)
        a = dict(key=inp(b * n, T, A), q=inp(b * n, A), c=inp(b, T, max(K, 1)), Wp=inp(A, max(K, 1)), we=inp(A), be=inp(1),
                 lens=torch.full((b,), T, dtype=torch.int64, device=DEV), attn=nanb(b * n, T), e=nanb(b * n, T),
                 attn_in=inp(b * n, T), dattn=inp(b * n, T), dkey=nanb(b * n, T, A), dq=nanb(b * n, A),
                 dc=nanb(b, T, max(K, 1)), dWp=nanb(A, max(K, 1)), dwe=nanb(A), dbe=nanb(1))
        outs.extend(('energy%s %s' % ((loc, B, N, T, A, K, temp, drop, only), k), a[k])
                    for k in ('attn', 'e', 'dkey', 'dq', 'dc', 'dWp', 'dwe', 'dbe'))
        if drop:
            a[drop] = None
        if not loc:
            for k in ('c', 'Wp', 'we', 'be', 'dc', 'dWp', 'dwe', 'dbe'):
                a[k] = None
        r = []
        if 'f' in only:
            r.append(L.asrk_attn_energy_fwd_f32(loc, p(a['key']), p(a['q']), p(a['c']), p(a['Wp']), p(a['we']), p(a['be']),
                                                p(a['lens']), p(a['attn']), p(a['e']), B, N, T, A, K, temp, st()))
        if 'b' in only:
            r.append(L.asrk_attn_energy_bwd_f32(loc, p(a['key']), p(a['q']), p(a['c']), p(a['Wp']), p(a['we']), p(a['lens']),
                                                p(a['attn_in']), p(a['dattn']), p(a['dkey']), p(a['dq']), p(a['dc']),
                                                p(a['dWp']), p(a['dwe']), p(a['dbe']), B, N, T, A, K, temp, st()))
        return tuple(r)

    for loc in (1, 0):
        assert energy(loc, 2, 1, 8, 20, 3, 0.0) == (EINVAL, EINVAL)                 # temperature = 0
        assert energy(loc, 2, 0, 8, 20, 3, 1.0) == (EINVAL, EINVAL)                 # N = 0
        assert energy(loc, 2, 1, 8, 20, 3, 1.0, drop='key') == (EINVAL, EINVAL)     # a null required pointer
        assert energy(loc, 2, 1, 8, 20, 3, 1.0, drop='lens') == (EINVAL, EINVAL)
        assert energy(loc, 0, 1, 8, 20, 3, 1.0) == (0, 0)                           # B = 0
    assert energy(1, 2, 1, 8, 20, 3, 1.0, drop='Wp') == (EINVAL, EINVAL)
    assert energy(1, 2, 1, 8, 20, 3, 1.0, drop='dq', only='b') == (EINVAL,)
    assert energy(1, 2, 1, 8, 20, 3, 1.0, drop='dbe', only='b') == (EINVAL,)
    assert energy(1, 2, 1, 8, 20, 3, 1.0, drop='e', only='f') == (EINVAL,)
    assert energy(1, 2, 1, 8, 20, 0, 1.0) == (EINVAL, EINVAL)                       # loc with K = 0
    assert energy(1, 5, 1, 9, 20, 17, 1.0, only='b') == (ESHAPE,)                   # K = 17 on the loc backward
    assert energy(1, 4, 1, 8, 430, 16, 1.0, only='b') == (ESHAPE,)                  # backward LDS over 150 KB at tpb 8
    for args, status, _ in R.ENERGY_REFUSED:                                        # the plan refuses the same sizes
        loc, bwd, BN, T, A, K = args
        if BN > 0 and T > 0 and A > 0:
            assert energy(loc, BN, 1, T, A, K, 1.0, only='b' if bwd else 'f') == (status,), args

    def ctxcall(BN, T, Dv, stride, drop=None, only='fb'):
        a = dict(attn=inp(max(BN, 1), T), value=inp(max(BN, 1), T, Dv), ctx=nanb(max(BN, 1), max(stride, Dv)),
                 dctx=inp(max(BN, 1), max(stride, Dv)), dattn=nanb(max(BN, 1), T))
        outs.extend(('context%s %s' % ((BN, T, Dv, stride, drop, only), k), a[k]) for k in ('ctx', 'dattn'))
        if drop:
            a[drop] = None
        r = []
        if 'f' in only:
            r.append(L.asrk_attn_context_fwd_f32(p(a['attn']), p(a['value']), p(a['ctx']), BN, T, Dv, stride, st()))
        if 'b' in only:
            r.append(L.asrk_attn_context_bwd_f32(p(a['dctx']), p(a['value']), p(a['dattn']), BN, T, Dv, stride, st()))
        return tuple(r)

    assert ctxcall(2, 5, 40, 39) == (EINVAL, EINVAL)                                # ctx_stride < Dv
    assert ctxcall(1, 15361, 1, 1, only='f') == (ESHAPE,)                           # T * 4 bytes over 60 KB of LDS
    assert ctxcall(2, 5, 40, 40, drop='ctx', only='f') == (EINVAL,)
    assert ctxcall(2, 5, 40, 40, drop='dattn', only='b') == (EINVAL,)
    assert ctxcall(2, 5, 40, 40, drop='value') == (EINVAL, EINVAL)
    assert ctxcall(0, 5, 40, 40) == (0, 0)

    g, c, h, dcp = nanb(3, 20), nanb(3, 5), nanb(3, 5), nanb(3, 5)
    outs.extend(zip(('cell gates', 'cell c', 'cell h', 'cell dc_prev'), (g, c, h, dcp)))
    cp = inp(3, 5)
    assert L.asrk_lstm_cell_fwd_f32(p(g), p(cp), p(c), None, 3, 5, st()) == EINVAL
    assert L.asrk_lstm_cell_fwd_f32(p(g), p(cp), p(c), p(h), 3, 0, st()) == EINVAL
    assert L.asrk_lstm_cell_fwd_f32(p(g), p(cp), p(c), p(h), 0, 5, st()) == 0
    assert L.asrk_lstm_cell_bwd_f32(p(g), p(cp), p(c), None, None, None, 3, 5, st()) == EINVAL
    assert L.asrk_lstm_cell_bwd_f32(p(g), p(cp), p(c), None, None, p(dcp), 0, 5, st()) == 0
    idx = torch.zeros(4, dtype=torch.int64, device=DEV)
    out, dW = nanb(4, 6), nanb(3, 6)
    outs.extend([('embedding out', out), ('embedding dW', dW)])
    W, g46 = inp(3, 6), inp(4, 6)
    assert L.asrk_embedding_fwd_f32(p(idx), p(W), None, 4, 6, 3, st()) == EINVAL
    assert L.asrk_embedding_fwd_f32(p(idx), p(W), p(out), 4, 0, 3, st()) == EINVAL
    assert L.asrk_embedding_fwd_f32(p(idx), p(W), p(out), 0, 6, 3, st()) == 0
    assert L.asrk_embedding_bwd_f32(p(idx), p(g46), None, 4, 6, 3, st()) == EINVAL
    assert L.asrk_embedding_bwd_f32(p(idx), p(g46), p(dW), 4, 6, 0, st()) == EINVAL
    assert L.asrk_embedding_bwd_f32(p(idx), p(g46), p(dW), 0, 6, 3, st()) == 0
    ops.check_errors()
    torch.cuda.synchronize()
    written = [name for name, v in outs if not all_nan(v)]
    assert len(outs) > 50 and not written, written


# ------------------------------------------------------------------------------------------------ autograd plumbing
def _chain_device(dops, cc, t):
    s = R.CHAIN
    names = R.chain_params(cc)
    dv = {k: d(t[k]).clone().requires_grad_(True) for k in names}
    loc_w = tuple(dv[k] for k in ('Wc', 'Wp', 'we', 'be')) if cc.loc else ()
    tape = dops.AttnTape('loc' if cc.loc else 'dot', dv['key'].detach(), dv['value'].detach(), d(t['lens']), cc.N, s['temp'],
                         tuple(w.detach() for w in loc_w) if cc.loc else None)
    token = dops.AttnHubFn.apply(tape, dv['key'], dv['value'], *loc_w)
    prev, attns, ctxs = (dv['prev0'] if cc.loc else None), [], []
    for l in range(s['L']):
        attn, ctx = dops.AttnStepFn.apply(tape, token, dv['q%d' % l], prev)
        attns.append(attn)
        ctxs.append(ctx)
        prev = attn if cc.loc else None
    return dv, tape, attns, ctxs


@pytest.mark.parametrize("case", R.CHAIN_CASES, ids=lambda c: c.name)
def test_three_chained_steps_through_the_hub(ops, dops, case):
    """attn_l is the prev_att of step l + 1, a fresh q per step; the loss reads the contexts of steps 0 and 2 and the
    attention of step 2, so step 1 is used through the chain only.  Every gradient: each q, prev0, key, value (the hub's
    batched L-step GEMM), Wc, Wp, we; be under the softmax limit"""
    cc = case
    t = R.chain_inputs(cc)
    ref = cached('chain_' + cc.name, lambda: R.chain_reference_of(cc, t))
    r32 = cached('chain_' + cc.name + '/32', lambda: R.chain_reference_of(cc, t, torch.float32))
    dv, tape, attns, ctxs = _chain_device(dops, cc, t)
    dt = {k: d(v) for k, v in t.items()}
    R.chain_loss(dt, attns, ctxs, torch.float32).backward()
    ops.check_errors()
    assert attns[0].shape == (R.CHAIN['B'], cc.N, R.CHAIN['T']) and tape.attn_steps == [] and tape.dctx_steps == []
    got = {'attn%d' % l: a for l, a in enumerate(attns)}
    got.update({'ctx%d' % l: c for l, c in enumerate(ctxs)})
    for k in R.chain_params(cc):
        g = dv[k].grad
        if k == 'q1' and not cc.loc:
            assert g is None or float(g.abs().max()) == 0.0          # dot energies: step 1 reaches nothing in the loss
            continue
        assert g is not None, k
        got['d' + k] = g
    if cc.loc:
        _, noise = cached('chain_' + cc.name + '/de', lambda: R.chain_manual_grads(cc, t))
        dbe = abs(float(got.pop('dbe')))
        lim = max(32 * abs(float(r32['dbe'])), 32 * 2.0 ** -24 * noise)
        print("ATTNVAR chain_%s | dbe (softmax) | float32 CPU %.3e | limit %.3e | device %.3e" % (cc.name, abs(float(r32['dbe'])), lim, dbe))
        assert dbe <= lim
    mask = R.frame_mask(t['lens'], cc.N, R.CHAIN['T']).view(R.CHAIN['B'], cc.N, -1)
    for a in attns:
        assert float(a.detach().cpu()[mask].abs().max()) == 0.0
    judge('chain_' + cc.name, got, ref, r32)


@pytest.mark.parametrize("case", [R.CHAIN_CASES[1], R.CHAIN_CASES[4]], ids=lambda c: c.name)
def test_attn_step_infer_and_expand_tape(ops, dops, case):
    """attn_step_infer against AttnStepFn's forward on the same inputs, and expand_tape(tape, 5) of a one-utterance
    tape: the five replicas' rows are identical to each other and within the bound of the reference"""
    cc = case
    s = R.CHAIN
    t = R.chain_inputs(cc)
    ref = cached('chain_' + cc.name, lambda: R.chain_reference_of(cc, t))
    r32 = cached('chain_' + cc.name + '/32', lambda: R.chain_reference_of(cc, t, torch.float32))
    loc_w = tuple(d(t[k]) for k in ('Wc', 'Wp', 'we', 'be')) if cc.loc else None
    mode = 'loc' if cc.loc else 'dot'
    tape = dops.AttnTape(mode, d(t['key']), d(t['value']), d(t['lens']), cc.N, s['temp'], loc_w)
    prev = d(t['prev0']) if cc.loc else None
    attn, ctx = dops.attn_step_infer(tape, d(t['q0']), prev)
    assert not attn.requires_grad and not ctx.requires_grad
    judge('infer_' + cc.name, dict(attn0=attn, ctx0=ctx), ref, r32)
    with torch.no_grad():
        a_fn, c_fn = dops.AttnStepFn.apply(tape, torch.zeros((), device=DEV), d(t['q0']), prev)
    judge('stepfn_' + cc.name, dict(attn0=a_fn, ctx0=c_fn), ref, r32)
    assert torch.equal(attn, a_fn) and torch.equal(ctx, c_fn)          # the same launches, and none of them uses atomics
    b, N, n = 1, cc.N, 5                                              # the utterance of length 33
    rows = slice(b * N, (b + 1) * N)
    one = dops.AttnTape(mode, d(t['key'][rows]).contiguous(), d(t['value'][rows]).contiguous(), d(t['lens'][b:b + 1]), N,
                        s['temp'], loc_w)
    big = dops.expand_tape(one, n)
    assert (big.B, big.BN, big.N, big.T, big.A, big.Dv) == (n, n * N, N, s['T'], s['A'], s['Dv'])
    assert big.lens.tolist() == [33] * n
    for i in range(n):
        assert torch.equal(big.key[i * N:(i + 1) * N], one.key) and torch.equal(big.value[i * N:(i + 1) * N], one.value)
    a5, c5 = dops.attn_step_infer(big, d(t['q0'][rows]).repeat(n, 1), prev[b:b + 1].repeat(n, 1, 1) if cc.loc else None)
    ops.check_errors()
    for i in range(1, n):
        assert torch.equal(a5[i], a5[0]) and torch.equal(c5[i * N:(i + 1) * N], c5[:N])
    sub = lambda r: dict(attn0=r['attn0'][b:b + 1], ctx0=r['ctx0'][rows])
    judge('expand_' + cc.name, dict(attn0=a5[:1], ctx0=c5[:N]), sub(ref), sub(r32))


def test_three_chained_cell_steps_and_tape_capacity(ops, dops):
    """LSTMCellStepFn at B = 5, In = 13, H = 9: three chained steps, the middle one used through the chain only; the
    weight and bias gradients come from CellHubFn's batched GEMMs; a fourth step raises"""
    t = R.cell_chain_inputs()
    ref = cached('cell_chain', lambda: R.cell_chain_reference_of(t))
    r32 = cached('cell_chain/32', lambda: R.cell_chain_reference_of(t, torch.float32))
    dv = {k: d(t[k]).clone().requires_grad_(True) for k in R.CELL_CHAIN_PARAMS}
    w = [dv[k] for k in ('w_ih', 'w_hh', 'b_ih', 'b_hh')]
    tape = dops.CellTape(*[x.detach() for x in w], 5, 3)
    token = dops.CellHubFn.apply(tape, *w)
    h, c, hs = dv['h0'], dv['c0'], []
    for l in range(3):
        h, c = dops.LSTMCellStepFn.apply(tape, token, dv['x%d' % l], h, c)
        hs.append(h)
    with pytest.raises(RuntimeError, match="capacity"):
        dops.LSTMCellStepFn.apply(tape, token, dv['x0'], h, c)
    assert tape.used == 3
    ((hs[0] * d(t['g_h0'])).sum() + (hs[2] * d(t['g_h2'])).sum() + (c * d(t['g_c2'])).sum()).backward()
    ops.check_errors()
    got = dict(h_last=hs[2], cell_last=c)
    got.update({'d' + k: dv[k].grad for k in R.CELL_CHAIN_PARAMS})
    judge('cell_chain', got, ref, r32)
